"""GPU: per-episode domain randomisation through the env (envs/events.py, manager_based_rl_env.py) -- the drift, elevation and visual
tasks with wheel friction in mode reset and the base mass in mode interval: after reset() and after every step the four constant rows
and the layer's block are the reference (tests/event_rand_reference.py) driven by the flags the step returned, byte for byte (the
terms draw uniformly: nothing is approximate).  Then collect_step against step on a twin, the refusals of everything that runs more
than one env step per launch, the all-startup config (no layer, constant rows that never change) and the mdp functions called
directly.  64 to 130 envs, episodes of 6 steps so that every env resets several times in a run."""
import numpy as np
import pytest
import torch

from tests import event_rand_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DRIFT, ELEV, VISUAL = "Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0"


def _episodic(cfg):
    """friction per episode, base mass on a timer of two to five steps"""
    if not hasattr(cfg.events, "change_wheel_friction"):          # the shipped visual config only resets: take the reference's randomised events
        from wheeledlab_amd.tasks.visual.mushr_visual_env_cfg import VisualEventsRandomCfg
        cfg.events = VisualEventsRandomCfg()
    step = cfg.sim.dt * cfg.decimation
    cfg.events.change_wheel_friction.mode = "reset"
    cfg.events.add_base_mass.mode, cfg.events.add_base_mass.interval_range_s = "interval", (2 * step, 5 * step)


def _env(task, n=64, seed=11, steps_per_episode=6, edit=_episodic):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    cfg = registry.parse_env_cfg(task, device=DEV, num_envs=n)
    cfg.seed = seed
    cfg.episode_length_s = (steps_per_episode - 0.5) * cfg.sim.dt * cfg.decimation      # ceil -> steps_per_episode steps
    if edit is not None:
        edit(cfg)
    env = registry.make(task, cfg=cfg)
    assert env.max_episode_length == steps_per_episode
    return env


def _words(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _consts(env):
    from wheeledlab_amd import _abi as A
    return _words(env._batch.state[A.S_MU_S:A.S_MASS + 1])


def _tab(env):
    return [dict(zip(R.FIELDS, row)) for row in env._event_rand.table.terms]


@pytest.mark.parametrize("task,n", [(DRIFT, 130), (ELEV, 65), (VISUAL, 64)])
def test_constant_rows_follow_the_reference_step_by_step(task, n):
    env = _env(task, n)
    layer, b = env._event_rand, env._batch
    assert layer is not None and env._event_direct is None and not env.can_collect_rollout()
    tab = _tab(env)
    assert [(t["target"], t["mode"]) for t in tab] == [(R.MU, R.RESET), (R.MASS_BASE, R.INTERVAL)] and layer.table.names == ("change_wheel_friction", "add_base_mass")
    case = R.Case(tab, None, has_b=True, has_mask=False)
    mats = R.materials(tab[0], b.seed)
    dt = float(np.float32(env.step_dt))

    def check(ref, what):
        assert R.check(_consts(env), _words(layer.block), ref, what=what) == 0.0
        c = _consts(env)[:, :n].view(np.float32)
        assert all(((c[0, e] == mats[0]) & (c[1, e] == mats[1])).any() for e in range(n)), f"{what}: a material that is no bucket's"
        return ref
    # construction: the startup's rows, the parts that sum to its mass row, the first timers
    parts = _words(layer.block[0:2])[:, :n].view(np.float32)
    c0 = _consts(env)[:, :n].view(np.float32)
    assert np.array_equal((parts[0] + parts[1]).astype(np.float32).view(np.uint32), c0[R.C_MASS].view(np.uint32))
    z = np.zeros(n, bool)
    ref = R.apply(tab, R.State(n, len(tab), c0, parts), z, None, None, 0, b.seed, 0, 0.0, b.env_offset)
    R.check(_consts(env), _words(layer.block), ref, what="construction")
    env.reset()
    ref = check(R.apply(tab, ref, np.ones(n, bool), None, None, 0, b.seed, b.step_count, 0.0, b.env_offset), "reset")
    assert ref.fired[0].all() and not ref.fired[1].any()
    g = torch.Generator(device=DEV).manual_seed(3)
    resets, fires, seen = 0, 0, set()
    for k in range(20):
        _, _, term, trunc, _ = env.step(torch.rand(n, 2, device=DEV, generator=g) * 2 - 1)
        ref = check(R.apply(tab, ref, term.cpu().numpy(), trunc.cpu().numpy(), None, 0, b.seed, b.step_count, dt, b.env_offset), f"{task} step {k}")
        assert np.array_equal(ref.fired[0], (term | trunc).cpu().numpy())
        resets, fires = resets + int(ref.fired[0].sum()), fires + int(ref.fired[1].sum())
        seen |= set(_consts(env)[0, :n].tolist())
    assert resets >= 3 * n and fires >= 2 * n                                # every env reset at least three times, every timer ran out
    if task != ELEV:                                                           # (the elevation config's friction ranges are points)
        assert len(seen) > 3                                                    # an env no longer keeps the material it drew first
    with pytest.raises(ValueError, match="event"):
        env.rollout_policy(None, None) if task == DRIFT else env.collect_rollout(None, None)


def _runner(task, n, K, edit, **kw):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    env = _env(task, n, edit=edit)
    env.action_space.low, env.action_space.high = -1.0, 1.0
    agent = registry.load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.num_steps_per_env = K
    return OnPolicyRunner(RslRlVecEnvWrapper(ClipAction(env)), agent, device=DEV, **kw)


@pytest.mark.parametrize("task", [DRIFT, ELEV])
def test_collect_step_and_step_give_identical_rows_and_training_runs(task):
    n, K = 64, 8
    torch.manual_seed(0)
    runner, twin = _runner(task, n, K, _episodic), _runner(task, n, K, _episodic)      # the twin never learns: its env is stepped by hand
    base, tbase = runner.env.unwrapped, twin.env.unwrapped
    assert base._event_rand is not None and not runner.fused and runner.kernel_policy and not base.can_collect_rollout()
    obs, _ = runner.env.get_observations()
    for it in range(2):
        with torch.inference_mode():
            obs = runner._collect_stepwise(obs)
        st = runner.storage
        for k in range(K):
            tobs, _, dones, _ = twin.env.step(st.actions[k])
            assert np.array_equal(_words(tobs), _words(st.observations[k + 1])), (it, k)
            assert torch.equal(dones.bool(), st.dones[k].bool())
        assert np.array_equal(_words(base._batch.state), _words(tbase._batch.state))           # the constant rows among them
        assert np.array_equal(_words(base._event_rand.block), _words(tbase._event_rand.block))
        assert (st.terminated | st.time_outs).any()
    hist = runner.learn(2, verbose=False)
    assert runner.collection_paths == ["stepwise", "stepwise"]
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("value_function", "surrogate", "mean_step_reward")), h


def test_fused_and_persistent_entry_points_refuse_the_layer():
    with pytest.raises(ValueError, match="event"):
        _runner(DRIFT, 64, 8, _episodic, fused=True)
    runner = _runner(DRIFT, 64, 8, _episodic)
    assert not runner.fused
    with pytest.raises(ValueError, match="event"):
        runner.env.unwrapped.rollout_policy(runner.actor_critic.fused(), runner.storage)
    erunner = _runner(ELEV, 64, 8, _episodic)
    assert not erunner.env.unwrapped.can_collect_rollout()
    with pytest.raises(ValueError, match="event"):
        erunner.env.unwrapped.collect_rollout(erunner.actor_critic.fused(), erunner.storage)
    assert _runner(DRIFT, 64, 8, None).fused                                  # the shipped config still takes the fused collector


@pytest.mark.parametrize("task", [DRIFT, ELEV, VISUAL])
def test_all_startup_config_builds_no_layer_and_its_constants_never_change(task):
    env = _env(task, 64, edit=None)
    assert env._event_rand is None and env._event_direct is None and env._flat.events is None
    before = _consts(env).copy()
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(50):
        env.step(torch.rand(64, 2, device=DEV, generator=g) * 2 - 1)
    assert np.array_equal(_consts(env), before)


@pytest.mark.parametrize("edit", [None, _episodic])
def test_direct_calls_change_exactly_the_named_envs(edit):
    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import SceneEntityCfg
    n = 70
    env = _env(DRIFT, n, edit=edit)
    env.reset()
    ids = torch.tensor([0, 3, 64, 69], device=DEV)
    hit = np.zeros(n, bool)
    hit[ids.cpu().numpy()] = True
    state0 = _words(env._batch.state).copy()
    mdp.randomize_rigid_body_mass(env, ids, asset_cfg=SceneEntityCfg("robot", body_names=["base_link"]), mass_distribution_params=(5.0, 6.0), operation="abs")
    state1 = _words(env._batch.state)
    rows = np.ones(A.S_COUNT, bool)
    rows[A.S_MASS] = False
    assert np.array_equal(state0[rows], state1[rows]) and np.array_equal(state0[A.S_MASS, ~np.pad(hit, (0, env._batch.stride - n))], state1[A.S_MASS, ~np.pad(hit, (0, env._batch.stride - n))])
    m = state1[A.S_MASS, :n].view(np.float32)
    assert ((m[hit] >= 5.0) & (m[hit] <= 6.0)).all() and (m[~hit] < 5.0).all()
    layer = env._event_rand or env._event_direct
    assert (env._event_rand is None) == (edit is None) and layer is not None
    assert np.array_equal((layer.part_base + layer.part_wheels).cpu().numpy().view(np.uint32), state1[A.S_MASS, :n])
    again = m.copy()
    mdp.randomize_rigid_body_mass(env, ids, asset_cfg=SceneEntityCfg("robot", body_names=["base_link"]), mass_distribution_params=(5.0, 6.0), operation="abs")
    m2 = _words(env._batch.state)[A.S_MASS, :n].view(np.float32)
    assert (m2[hit] != again[hit]).all() and np.array_equal(m2[~hit], again[~hit])       # a second call draws again
    mdp.randomize_rigid_body_material(env, slice(0, 5), (0.8, 0.9), (0.6, 0.7), (0.0, 0.0), 4, make_consistent=True)
    mdp.randomize_actuator_gains(env, None, damping_distribution_params=(0.5, 2.0), operation="scale", distribution="log_uniform")
    s = _words(env._batch.state).view(np.float32)
    assert ((s[A.S_MU_S, :5] >= 0.8) & (s[A.S_MU_S, :5] <= np.float32(0.9))).all() and (s[A.S_MU_S, 5:n] < 0.8).all()
    base = env._flat.startup.throttle_damping
    assert ((s[A.S_DAMP, :n] >= 0.5 * base * (1 - 1e-6)) & (s[A.S_DAMP, :n] <= 2.0 * base * (1 + 1e-6))).all()
    with pytest.raises(ValueError, match="randomize_rigid_body_material"):
        mdp.randomize_rigid_body_material(env, ids, (0.8, 0.9), (0.6, 0.7), (0.0, 0.5), 4)

"""GPU: observation corruption through the env (envs/corruption.py, manager_based_rl_env.py) -- every task with corruption on as the
twin of an env without: the same seed and actions give the same state, rewards and flags bit for bit, and the noisy env's row is the
reference (tests/obs_corrupt_reference.py) applied to the twin's clean row with the env's (seed, step, env_offset): exact on the
uniform and constant columns, within the Gaussian tolerance (derived in tests/test_gpu_obs_corrupt.py) elsewhere.  Then last_action
beyond +-1, the drift task's own fused Gaussian left alone, a plugin term, history behind the noise, the runner's collect_step path and
a short training run.  64 envs, 4-step episodes so time-outs fall inside every run."""
import os

import numpy as np
import pytest
import torch

from tests import obs_corrupt_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DRIFT, ELEV, VISUAL, DEPTH = "Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0", "Isaac-MushrVisualDepthRL-v0"


def _env(task, n=64, seed=11, steps_per_episode=4, edit=None):
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


def _tab(env):
    """the env's table as the reference's list of dicts"""
    return [dict(zip(R.FIELDS, row)) for row in env._corruption.layout.terms]


def _state(env):
    return _words(env._batch.state)


def _noise_cfgs():
    from wheeledlab_amd.envs import managers_cfg as M
    return M


def _clean(cfg):
    cfg.observations.policy.enable_corruption = False


def _on(cfg):
    cfg.observations.policy.enable_corruption = True


def _drift_noisy(cfg):
    M = _noise_cfgs()
    pol = cfg.observations.policy
    pol.enable_corruption = True
    pol.base_lin_vel_term.noise = M.UniformNoiseCfg(n_min=-0.1, n_max=0.1)
    pol.base_ang_vel_term.noise = M.NoiseModelWithAdditiveBiasCfg(noise_cfg=M.GaussianNoiseCfg(mean=0.0, std=0.4),
                                                                  bias_noise_cfg=M.UniformNoiseCfg(n_min=-0.05, n_max=0.05))


def _elev_noisy(cfg):
    M = _noise_cfgs()
    from wheeledlab_amd.envs.configclass import fields_of
    cfg.observations.policy.enable_corruption = True
    for i, (_, t) in enumerate((k, v) for k, v in fields_of(cfg.observations.policy) if hasattr(v, "func")):
        t.noise = M.GaussianNoiseCfg(mean=0.0, std=0.01 * (i + 1))


def _twin_run(task, edit_clean, edit_noisy, K=12, act_scale=1.0, n=64, with_history=None):
    """env A clean, env B with the layer: same seed, same K actions, two rounds (the second starts from reset() on a used bias block)"""
    a, b = _env(task, n, edit=edit_clean), _env(task, n, edit=edit_noisy)
    assert a._corruption is None and b._corruption is not None and not b.can_collect_rollout()
    tab, L = _tab(b), b._corruption.layout
    assert L.D == a._batch.OBS_DIM + sum(int(a._eval_obs_term(t).shape[1]) for _, t in a._custom_obs) == a._obs_dim
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = (torch.rand(K, n, 2, device=DEV, generator=g) * 2 - 1) * act_scale
    bias = np.zeros((n, max(L.Db, 0)), np.float32)
    worst, timeouts, rows = 0.0, 0, []
    for rnd in range(2):
        oa, _ = a.reset()
        ob, _ = b.reset()
        assert np.array_equal(_state(a), _state(b))
        res = R.apply(tab, _words(oa["policy"]), bias, np.ones(n, bool), b._batch.seed, b._batch.step_count, b._batch.env_offset, L.enable, state=_state(a))
        worst = max(worst, R.check(_words(b._corruption.row), res, what=f"{task} reset {rnd}"))
        bias = res.bias
        for k in range(K):
            torch.manual_seed(100 + k)            # (the visual task draws its camera augmentation from torch's generator, once per step)
            oa, ra_, ta, ua, _ = a.step(actions[k])
            torch.manual_seed(100 + k)
            ob, rb_, tb, ub, _ = b.step(actions[k])
            assert torch.equal(ta, tb) and torch.equal(ua, ub) and np.array_equal(_words(ra_), _words(rb_))
            assert np.array_equal(_state(a), _state(b)), (rnd, k)                   # noise touches the observation only
            assert b._batch.step_count == a._batch.step_count == rnd * K + k + 1
            flags = (ta | ua).cpu().numpy()
            timeouts += int(ua.sum())
            res = R.apply(tab, _words(oa["policy"]), bias, flags, b._batch.seed, b._batch.step_count, b._batch.env_offset, L.enable, state=_state(a))
            got = _words(b._corruption.row)
            worst = max(worst, R.check(got, res, what=f"{task} round {rnd} step {k}"))
            if L.Db:
                R.check_bias(b._corruption.bias.cpu().numpy(), res)
            bias = res.bias
            rows.append((got.copy(), flags.copy()))
            if with_history is None:
                assert ob["policy"].data_ptr() == b._corruption.row.data_ptr()
                c1 = _words(b.observation_manager.compute()["policy"]).copy()       # reading draws nothing new
                c2 = _words(b.observation_manager.compute()["policy"]).copy()
                assert np.array_equal(c1, c2) and np.array_equal(c1, got)
    assert timeouts >= n                                                            # time-outs happened inside the run
    print(f"\nOBSCORRUPT env {task}: largest Gaussian error / tolerance {worst:.4f}")
    return a, b, rows, tab


def test_drift_with_uniform_noise_and_a_bias_model():
    a, b, rows, tab = _twin_run(DRIFT, _clean, _drift_noisy)
    assert [t["noise_kind"] for t in tab] == [R.GAUSSIAN, R.GAUSSIAN, R.UNIFORM, R.GAUSSIAN, R.NONE] and b._corruption.layout.Db == 3
    assert b._batch.p.enable_corruption == 0 and a._batch.p.enable_corruption == 0
    from wheeledlab_amd.rl import RslRlVecEnvWrapper
    assert RslRlVecEnvWrapper(b).num_obs == 14


def test_elevation_with_a_gaussian_on_every_term():
    a, b, rows, tab = _twin_run(ELEV, _clean, _elev_noisy)
    assert all(t["noise_kind"] == R.GAUSSIAN for t in tab) and [t["width"] for t in tab] == [2, 3, 3, 3, 2, 676]
    assert tab[4]["state_row"] >= 0 and tab[5]["clip_hi"] == 10.0


@pytest.mark.parametrize("task", [VISUAL, DEPTH])
def test_visual_tasks_with_their_declared_noise(task):
    a, b, rows, tab = _twin_run(task, _clean, _on, K=8)
    assert [t["noise_kind"] for t in tab] == [R.NONE, R.UNIFORM, R.UNIFORM, R.UNIFORM]
    assert [(t["noise_a"], t["noise_b"]) for t in tab[1:]] == [R.uniform(-0.1, 0.1)[1:]] * 3


def test_visual_last_action_noise_comes_before_the_clip():
    K = 7                                                                           # the last step is no time-out: its actions are still in the state
    a, b, rows, tab = _twin_run(VISUAL, _clean, _on, K=K, act_scale=1.5)
    # the reference (through state_row) says clip(a + n); say it once more by hand on the last step and show clip(clip(a) + n) differs
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = (torch.rand(K, 64, 2, device=DEV, generator=g) * 2 - 1) * 1.5
    row = b._corruption.layout.terms[3][15]
    raw = b._batch.state[row:row + 2, :64].T.cpu().numpy()
    got, flags = rows[-1]
    run = ~flags
    assert run.sum() >= 32
    assert np.array_equal(raw[run], actions[-1].cpu().numpy()[run]) and (np.abs(raw[run]) > 1).any()       # the state keeps the raw action
    t = tab[3]
    cols = np.arange(t["off"], t["off"] + 2)
    env_ids = (np.arange(64, dtype=np.uint64) + np.uint64(b._batch.env_offset))
    d = R.draw(t["noise_kind"], t["noise_a"], t["noise_b"], R.words(env_ids, b._batch.step_count, R.S_NOISE, b._batch.seed, cols))[0]
    before = np.clip(raw + d, np.float32(-1), np.float32(1)).astype(np.float32)
    after = np.clip(np.clip(raw, -1, 1).astype(np.float32) + d, np.float32(-1), np.float32(1)).astype(np.float32)
    out = got.view(np.float32)[:, cols]
    assert np.array_equal(out[run], before[run]) and not np.array_equal(out[run], after[run])


def test_drift_with_its_shipped_gaussian_builds_nothing_and_keeps_the_in_kernel_noise():
    """What this holds: no layer is built, the row returned IS the step kernel's own buffer (no launch behind it), the kernel's
    parameters still carry enable_corruption = 1, and the noise on the row is the step's own draw (streams 4 and 5 of
    oracle/philox.normal12) to the accuracy of the device's Box-Muller.  That shows the in-kernel noise is still the source; it is
    not by itself bit-identity.  Bit-identity of the drift outputs rests on the drift tests that were there before and are
    unchanged (tests/test_gpu_drift_parity.py and the drift goldens): the step kernel's source, its parameters
    (tests/test_obs_corrupt_cpu.py holds enable_corruption and noise_std of the shipped config) and its launch are what they were."""
    env = _env(DRIFT)
    assert env._corruption is None and env._batch.p.enable_corruption == 1 and env.cfg.observations.policy.enable_corruption
    clean = _env(DRIFT, edit=_clean)
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = torch.rand(6, 64, 2, device=DEV, generator=g) * 2 - 1
    on, _ = env.reset()
    oc, _ = clean.reset()
    from oracle import philox as PH
    std = np.repeat(np.float32([0.1, 0.1, 0.5, 0.4]), 3)
    for k in range(6):
        on, r1, t1, u1, _ = env.step(actions[k])
        oc, r2, t2, u2, _ = clean.step(actions[k])
        assert on["policy"].data_ptr() == env._batch.obs.data_ptr()              # the step's own row: no launch behind it
        assert torch.equal(t1, t2) and torch.equal(u1, u2) and np.array_equal(_words(r1), _words(r2))
        # the in-kernel noise: 12 normals of streams 4 and 5 at the step the kernel ran (oracle/philox.normal12)
        z = PH.normal12(np.arange(64), env._batch.step_count - 1, env._batch.seed).T
        diff = on["policy"].cpu().numpy()[:, :12] - oc["policy"].cpu().numpy()[:, :12]
        np.testing.assert_allclose(diff, z * std, rtol=0, atol=2e-5 + 1e-6 * np.abs(oc["policy"].cpu().numpy()[:, :12]).max())
        assert np.array_equal(_words(on["policy"])[:, 12:], _words(oc["policy"])[:, 12:])
    assert env.can_collect_rollout() is False and _env(ELEV).can_collect_rollout()           # (drift never could; elevation still can)


def test_plugin_term_with_constant_noise_clip_and_scale_behind_the_elevation_layout():
    M = _noise_cfgs()
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import ObservationTermCfg as ObsTerm
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg, RayCasterCfg

    def scene(cfg):
        cfg.scene.patch = RayCasterCfg(pattern_cfg=GridPatternCfg(resolution=0.25, size=(0.5, 0.5)), max_distance=20.0)

    def clean(cfg):
        scene(cfg)
        cfg.observations.policy.patch = ObsTerm(func=mdp.height_scan, params=dict(sensor_cfg=M.SceneEntityCfg("patch")))

    def noisy(cfg):
        scene(cfg)
        cfg.observations.policy.enable_corruption = True
        cfg.observations.policy.patch = ObsTerm(func=mdp.height_scan, params=dict(sensor_cfg=M.SceneEntityCfg("patch")),
                                                noise=M.ConstantNoiseCfg(bias=0.05, operation="add"), clip=(-0.5, 0.5), scale=2.0)
    a, b, rows, tab = _twin_run(ELEV, clean, noisy, K=6)
    t = tab[6]
    assert (t["off"], t["noise_kind"], t["noise_op"], t["noise_a"], t["clip_lo"], t["clip_hi"], t["scale"], t["has_scale"]) == \
        (689, R.CONSTANT, R.ADD, R.f32(0.05), -0.5, 0.5, 2.0, 1) and t["width"] == 9
    assert all(x["noise_kind"] == R.NONE for x in tab[:6])                        # the fused terms: untouched or clipped again
    clean_row = _words(a.obs_buf["policy"]).view(np.float32)[:, 689:]
    want = (np.clip(clean_row + np.float32(0.05), np.float32(-0.5), np.float32(0.5)) * np.float32(2.0)).astype(np.float32)
    assert np.array_equal(_words(b.obs_buf["policy"])[:, 689:], want.view(np.uint32))        # exact, by hand as well


def test_history_stacks_the_corrupted_rows_and_redraws_nothing():
    from tests import obs_history_reference as H

    def noisy(cfg):
        _drift_noisy(cfg)
        cfg.observations.policy.history_length = 3
    a, b, rows, tab = _twin_run(DRIFT, _clean, noisy, K=8, with_history=3)
    htab, D, Dh = H.table([3, 3, 3, 3, 2], [3] * 5)
    assert b._history is not None and b.observation_manager.group_obs_dim["policy"] == (Dh,) == (42,)
    # replay the second round: frame f of the stacked row holds the bytes of the corrupted row of the step it was drawn at
    b.reset()
    prev = H.push_closed(htab, _words(b._corruption.row), None, np.ones(64, bool))
    assert np.array_equal(_words(b.obs_buf["policy"]), prev)
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = torch.rand(8, 64, 2, device=DEV, generator=g) * 2 - 1
    for k in range(8):
        ob, _, t, u, _ = b.step(actions[k])
        prev = H.push_closed(htab, _words(b._corruption.row), prev, (t | u).cpu().numpy())
        assert np.array_equal(_words(ob["policy"]), prev), k
        c = _words(b.observation_manager.compute()["policy"])
        assert np.array_equal(c, prev)


# ---- the runner ------------------------------------------------------------------------------------------------------

def _runner(task, n, K, edit, agent_over=None, **kw):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    env = _env(task, n, edit=edit)
    env.action_space.low, env.action_space.high = -1.0, 1.0
    agent = registry.load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    agent.num_steps_per_env = K
    for k, v in (agent_over or {}).items():
        setattr(agent, k, v)
    return OnPolicyRunner(RslRlVecEnvWrapper(ClipAction(env)), agent, device=DEV, **kw)


def test_collect_step_equals_step_on_a_twin_and_training_runs(tmp_path):
    n, K = 64, 8
    torch.manual_seed(0)
    runner = _runner(ELEV, n, K, _elev_noisy, agent_over=dict(empirical_normalization=True), log_dir=str(tmp_path))
    twin = _runner(ELEV, n, K, _elev_noisy, agent_over=dict(empirical_normalization=True))       # never learns: its env is stepped by hand
    base, tbase = runner.env.unwrapped, twin.env.unwrapped
    assert base._corruption is not None and not base.can_collect_rollout() and runner.kernel_policy and not runner.fused
    assert runner.obs_normalizer is not None and runner.storage.observations.shape == (K + 1, n, 689)
    # collection alone, twice (the update would normalise the stored rows in place): the runner's collect_step path against step() on the twin
    obs, _ = runner.env.get_observations()
    for it in range(2):
        with torch.inference_mode():
            obs = runner._collect_stepwise(obs)
        st = runner.storage
        if it == 0:
            assert np.array_equal(_words(st.observations[0]), _words(tbase.obs_buf["policy"]))
        for k in range(K):
            tobs, rew, dones, _ = twin.env.step(st.actions[k])
            assert np.array_equal(_words(tobs), _words(st.observations[k + 1])), (it, k)         # row for row
            assert torch.equal(dones.bool(), st.dones[k].bool())
        assert np.array_equal(_words(base.obs_buf["policy"]), _words(st.observations[K]))       # the env caught up with the storage
        assert np.array_equal(_words(base._corruption.bias), _words(tbase._corruption.bias))
        flags = (st.terminated | st.time_outs)
        assert flags.any() and not flags.all()
    hist = runner.learn(2, verbose=False)                                           # two stepwise PPO iterations
    assert runner.collection_paths == ["stepwise", "stepwise"]
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("value_function", "surrogate", "mean_step_reward")), h
    assert int(runner.obs_normalizer.count) == 2 * K * n
    path = os.path.join(str(tmp_path), "models", "model_0.pt")
    runner.save(path)
    other = _runner(ELEV, n, K, _elev_noisy, agent_over=dict(empirical_normalization=True))
    other.load(path)
    for k, v in runner.actor_critic.state_dict().items():
        assert torch.equal(other.actor_critic.state_dict()[k], v), k
    for k, v in runner.obs_normalizer.state_dict().items():
        assert torch.equal(other.obs_normalizer.state_dict()[k], v), k
    with pytest.raises(ValueError, match="corruption"):
        base.collect_rollout(runner.actor_critic.fused(), runner.storage)


def test_fused_collection_is_refused_with_corruption():
    with pytest.raises(ValueError, match="corruption"):
        _runner(DRIFT, 64, 8, _drift_noisy, fused=True)
    runner = _runner(DRIFT, 64, 8, _drift_noisy)
    assert not runner.fused
    with pytest.raises(ValueError, match="corruption"):
        runner.env.unwrapped.rollout_policy(runner.actor_critic.fused(), runner.storage)
    assert _runner(DRIFT, 64, 8, None).fused                                        # the shipped config still takes the fused collector

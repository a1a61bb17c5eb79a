"""GPU: the observation-history push (csrc/wl_obs_history.hip) against the reference (tests/obs_history_reference.py), byte for byte as
uint32 -- the kernel alone on guarded buffers, the env (step / reset / compute) as the twin of an env without history, the runner's
collect_step path inside the rollout storage, and a short training run at the stacked width."""
import os

import numpy as np
import pytest
import torch

from tests import obs_history_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7FC0BEEF            # a NaN pattern: what `next` and its guard rows hold before the launch


def _lib():
    from wheeledlab_amd import _abi as A
    return A, A.load()


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).to(DEV)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _inputs(rng, shape):
    """special words, none of them the guard word: an output the launch skipped then still reads GUARD and differs from the reference"""
    x = R.special_words(rng, shape)
    x[x == GUARD] ^= np.uint32(1)
    return x


def _ctable(A, tab):
    return (A.WlObsHistoryTerm * len(tab))(*[A.WlObsHistoryTerm(*(int(v) for v in t)) for t in tab])


def _flag_patterns(n, rng):
    z, o = np.zeros(n, bool), np.ones(n, bool)
    alt = np.arange(n) % 2 == 1
    last = z.copy()
    last[-1] = True
    rnd = rng.random(n) < 0.3
    # (reset_a, reset_b or None)
    return [("none", z, z), ("all", o, z), ("alternating", alt, None), ("last env", last, None), ("b only", z, alt),
            ("a and b", rnd, ~rnd & alt), ("b NULL, none", z, None)]


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("name", list(R.TABLES))
def test_push_kernel_equals_the_reference_and_writes_nothing_else(name, n):
    A, lib = _lib()
    tab, D, Dh = R.table(*R.TABLES[name])
    ct = _ctable(A, tab)
    assert lib.wl_obs_history_width(ct, len(tab), D) == Dh
    rng = np.random.default_rng(n * 131 + len(name))
    guard_rows = 2
    stream = A.stream(torch.device(DEV))
    cases = 0
    for stride_extra, offset in ((0, 0), (5, 1), (0, 2), (3, 3)):          # a strided obs; `next` at every place inside a 16-byte line
        stride = D + stride_extra
        obs_w = _inputs(rng, (n, stride))
        prev_w = _inputs(rng, (n, Dh))
        obs, prev = _dev(obs_w), _dev(prev_w)
        for label, ra_w, rb_w in _flag_patterns(n, rng):
            for with_prev in (True, False):
                if not with_prev and label not in ("none", "alternating"):
                    continue
                ra = torch.from_numpy(ra_w.copy()).to(DEV)
                rb = None if rb_w is None else torch.from_numpy(rb_w.copy()).to(DEV)
                total = n * Dh
                lo = guard_rows * Dh + (offset - guard_rows * Dh) % 4       # `next` starts `offset` words into a 16-byte line
                buf = torch.full((lo + total + guard_rows * Dh,), GUARD, dtype=torch.int32, device=DEV)
                assert buf.data_ptr() % 16 == 0
                nxt = buf[lo:lo + total]
                assert (nxt.data_ptr() // 4) % 4 == offset
                outs = []
                for _ in range(2):                                            # two calls on equal input: equal bytes
                    nxt.fill_(GUARD)
                    rc = lib.wl_obs_history_push(n, D, obs.data_ptr(), stride, ct, len(tab), prev.data_ptr() if with_prev else None,
                                                 nxt.data_ptr(), ra.data_ptr(), None if rb is None else rb.data_ptr(), stream)
                    assert rc == 0, (rc, label)
                    torch.cuda.synchronize()
                    outs.append(_host(buf).copy())
                got = outs[0]
                assert np.array_equal(outs[0], outs[1])
                fresh = ra_w | rb_w if rb_w is not None else ra_w
                want = R.push_closed(tab, obs_w, prev_w if with_prev else None, fresh)
                inner = got[lo:lo + total].reshape(n, Dh)
                bad = inner != want
                assert not bad.any(), (name, n, label, with_prev, offset, int(bad.sum()), np.argwhere(bad)[:4].tolist())
                assert (got[:lo] == GUARD).all() and (got[lo + total:] == GUARD).all()        # every guard word unchanged
                # (every output written: a word the launch skipped would still read GUARD, which is not among the inputs)
                assert np.array_equal(_host(obs), obs_w) and np.array_equal(_host(prev), prev_w)
                assert np.array_equal(ra.cpu().numpy(), ra_w) and (rb is None or np.array_equal(rb.cpu().numpy(), rb_w))
                cases += 1
    assert cases == 4 * 9


def test_storage_rows_k_and_k_plus_1_are_accepted_and_a_row_onto_itself_is_refused():
    A, lib = _lib()
    tab, D, Dh = R.table(*R.TABLES["elevation"])
    ct = _ctable(A, tab)
    n = 3
    rng = np.random.default_rng(0)
    rows_w = R.special_words(rng, (2, n, Dh))
    obs_w = R.special_words(rng, (n, D))
    rows, obs = _dev(rows_w), _dev(obs_w)
    ra = torch.zeros(n, dtype=torch.bool, device=DEV)
    s = A.stream(torch.device(DEV))
    assert lib.wl_obs_history_push(n, D, obs.data_ptr(), D, ct, len(tab), rows[0].data_ptr(), rows[0].data_ptr(), ra.data_ptr(), None, s) == -1
    assert lib.wl_obs_history_push(n, D, obs.data_ptr(), D, ct, len(tab), rows[0].data_ptr(), rows[1].data_ptr(), ra.data_ptr(), None, s) == 0
    torch.cuda.synchronize()
    got = _host(rows)
    assert np.array_equal(got[0], rows_w[0]) and np.array_equal(got[1], R.push_closed(tab, obs_w, rows_w[0], np.zeros(n, bool)))


@pytest.mark.parametrize("which", ["reset_a", "reset_b"])
@pytest.mark.parametrize("where", ["first bytes", "last bytes"])
def test_reset_flags_inside_next_are_refused_and_nothing_is_launched(which, where):
    """what the launch stores may touch nothing it reads: flag bytes that lie on `next` are WL_EINVAL, and `next` keeps every word"""
    A, lib = _lib()
    tab, D, Dh = R.table(*R.TABLES["elevation"])
    ct = _ctable(A, tab)
    n = 3
    rng = np.random.default_rng(1)
    obs, prev = _dev(R.special_words(rng, (n, D))), _dev(R.special_words(rng, (n, Dh)))
    nxt = torch.full((n * Dh,), GUARD, dtype=torch.int32, device=DEV)
    inside = nxt.view(torch.uint8)                                           # n * Dh * 4 bytes
    lying = inside[:n] if where == "first bytes" else inside[n * Dh * 4 - 1:]      # (the last: one byte of the n overlaps)
    good = torch.zeros(n, dtype=torch.bool, device=DEV)
    ra, rb = (lying, good) if which == "reset_a" else (good, lying)
    s = A.stream(torch.device(DEV))
    rc = lib.wl_obs_history_push(n, D, obs.data_ptr(), D, ct, len(tab), prev.data_ptr(), nxt.data_ptr(), ra.data_ptr(), rb.data_ptr(), s)
    assert rc == -1                                                          # WL_EINVAL
    torch.cuda.synchronize()
    assert (_host(nxt) == GUARD).all()
    # flags that end where `next` begins, or begin where it ends, touch nothing of it: accepted
    buf = torch.full((n * Dh + 8,), 0, dtype=torch.int32, device=DEV)
    nxt2 = buf[4:4 + n * Dh]
    before, after = buf[:4].view(torch.uint8)[16 - n:], buf[4 + n * Dh:].view(torch.uint8)[:n]
    assert before.data_ptr() + n == nxt2.data_ptr() and after.data_ptr() == nxt2.data_ptr() + n * Dh * 4
    assert lib.wl_obs_history_push(n, D, obs.data_ptr(), D, ct, len(tab), prev.data_ptr(), nxt2.data_ptr(), before.data_ptr(), after.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_host(nxt2).reshape(n, Dh), R.push_closed(tab, _host(obs).reshape(n, D), _host(prev).reshape(n, Dh), np.zeros(n, bool)))


# ---- the env ---------------------------------------------------------------------------------------------------------

def _env(task, n, seed=11, steps_per_episode=4, edit=None):
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


def _twin_run(task, tab, edit_both, edit_history, n=64, K=12, shape=None, custom_term=None):
    """env A without history, env B with: same seed, same K actions; the reference is fed A's rows and flags"""
    a = _env(task, n, edit=edit_both)

    def edit_b(cfg):
        if edit_both is not None:
            edit_both(cfg)
        edit_history(cfg)
    b = _env(task, n, edit=edit_b)
    D = int(tab[:, 1].sum())
    Dh = int((tab[:, 1] * tab[:, 2]).sum())
    shape = shape or (Dh,)
    assert a._history is None and b._history is not None
    assert a.observation_manager.group_obs_dim["policy"] == (D,) and b.observation_manager.group_obs_dim["policy"] == shape
    assert b.single_observation_space["policy"].shape == shape and b.observation_space["policy"].shape == (n, *shape)
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = torch.rand(K, n, 2, device=DEV, generator=g) * 2 - 1
    timeouts = custom = 0
    for rnd in range(2):                                                      # the second round starts from reset() on a filled history
        oa, _ = a.reset()
        ob, _ = b.reset()
        assert ob["policy"].shape == (n, *shape)
        prev = R.push_closed(tab, _words(oa["policy"]), None, np.ones(n, bool))
        assert np.array_equal(_words(ob["policy"]).reshape(n, Dh), prev), ("reset", rnd)
        for k in range(K):
            oa, ra_, ta, ua, _ = a.step(actions[k])
            ob, rb_, tb, ub, _ = b.step(actions[k])
            assert torch.equal(ta, tb) and torch.equal(ua, ub) and torch.equal(ra_, rb_)
            flags = (ta | ua).cpu().numpy()
            timeouts += int(ua.sum())
            if custom_term is not None:
                custom += int(b.termination_manager.get_term(custom_term).sum())
            prev = R.push_closed(tab, _words(oa["policy"]), prev, flags)
            got = _words(ob["policy"]).reshape(n, Dh)
            assert np.array_equal(got, prev), (rnd, k, int((got != prev).sum()))
    assert timeouts >= n                                                       # time-outs happened inside the run
    assert custom_term is None or custom >= n                                  # and so did the torch termination term
    return a, b


def test_drift_env_with_group_history_is_the_reference_on_its_twins_rows():
    tab, D, Dh = R.table(*R.TABLES["drift_h3"])
    assert (D, Dh) == (14, 42)

    def hist(cfg):
        cfg.observations.policy.history_length = 3
    a, b = _twin_run("Isaac-MushrDriftRL-v0", tab, None, hist)
    from wheeledlab_amd.rl import RslRlVecEnvWrapper
    assert RslRlVecEnvWrapper(b).num_obs == 42 and RslRlVecEnvWrapper(a).num_obs == 14


def test_elevation_env_with_term_history_and_a_plugin_term():
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import ObservationTermCfg as ObsTerm
    from wheeledlab_amd.envs.managers_cfg import TerminationTermCfg as DoneTerm
    tab, D, Dh = R.table([2, 3, 3, 3, 2, 676, 2], [1, 1, 1, 1, 1, 2, 3])
    assert (D, Dh) == (691, 689 + 676 + 6)

    def both(cfg):
        cfg.observations.policy.speed = ObsTerm(func=lambda env: mdp.base_lin_vel(env)[:, :2], clip=(-2.0, 2.0), scale=0.5)
        # a torch termination term: the even envs end after two steps (the odd ones time out after four); its flags must refill too
        cfg.terminations.two_steps = DoneTerm(func=lambda env: (env.episode_length_buf == 2)
                                              & (torch.arange(env.num_envs, device=env.device) % 2 == 0))

    def hist(cfg):
        cfg.observations.policy.elevation_map.history_length = 2
        cfg.observations.policy.speed.history_length = 3
    _twin_run("Isaac-MushrElevationRL-v0", tab, both, hist, custom_term="two_steps")


def test_group_history_unflattened_is_time_major():
    tab, D, Dh = R.table([14], [3])

    def hist(cfg):
        cfg.observations.policy.history_length = 3
        cfg.observations.policy.flatten_history_dim = False
    a, b = _twin_run("Isaac-MushrDriftRL-v0", tab, None, hist, shape=(3, 14))
    obs = b.obs_buf["policy"]
    assert obs.shape == (64, 3, 14)
    assert np.array_equal(_words(obs[:, 2]), _words(a.obs_buf["policy"]))     # the newest frame is the twin's row
    from wheeledlab_amd.rl import RslRlVecEnvWrapper
    with pytest.raises(ValueError, match="flat"):
        RslRlVecEnvWrapper(b)


def test_compute_reads_without_pushing():
    def hist(cfg):
        cfg.observations.policy.history_length = 3
    a, b = (_env("Isaac-MushrDriftRL-v0", 64, edit=hist) for _ in range(2))
    g = torch.Generator(device=DEV).manual_seed(9)
    actions = torch.rand(6, 64, 2, device=DEV, generator=g) * 2 - 1
    a.reset(), b.reset()
    for k in range(6):
        oa, *_ = a.step(actions[k])
        ob, *_ = b.step(actions[k])
        c1 = _words(b.observation_manager.compute()["policy"]).copy()
        c2 = _words(b.observation_manager.compute(update_history=True)["policy"]).copy()
        assert np.array_equal(c1, c2) and np.array_equal(c1, _words(ob["policy"]))
        assert np.array_equal(_words(oa["policy"]), _words(ob["policy"])), k    # the env that was read equals the env that was not


def test_off_means_off():
    from wheeledlab_amd.policy import RolloutStorage
    from wheeledlab_amd.rl import RslRlVecEnvWrapper
    for task, D in (("Isaac-MushrDriftRL-v0", 14), ("Isaac-MushrElevationRL-v0", 689)):
        env = _env(task, 64)
        assert env._history is None and env.observation_manager.group_obs_dim["policy"] == (D,) == (env._batch.OBS_DIM,)
        assert env.single_observation_space["policy"].shape == (D,)
        w = RslRlVecEnvWrapper(env)
        assert w.num_obs == D
        assert RolloutStorage(4, 64, w.num_obs, 2, DEV).observations.shape == (5, 64, D)
        obs, _ = env.reset()
        assert obs["policy"].shape == (64, D) and obs["policy"].data_ptr() == env._batch.obs.data_ptr()
    assert _env("Isaac-MushrElevationRL-v0", 64).can_collect_rollout()


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


def _group_h(h):
    def edit(cfg):
        cfg.observations.policy.history_length = h
    return edit


def test_collect_step_pushes_inside_the_storage():
    n, K = 64, 8
    tab, D, Dh = R.table([2, 3, 3, 3, 2, 676], [2] * 6)
    torch.manual_seed(0)
    runner = _runner("Isaac-MushrElevationRL-v0", n, K, _group_h(2))
    base = runner.env.unwrapped
    assert runner.kernel_policy and not runner.fused and not base.can_collect_rollout()
    assert runner.storage.observations.shape == (K + 1, n, Dh) and runner.actor_critic.actor[0].in_features == Dh == 1378
    runner.learn(1, verbose=False)
    assert runner.collection_paths == ["stepwise"]
    st = runner.storage
    rows = _words(st.observations)
    flags = (st.terminated | st.time_outs).cpu().numpy()
    assert flags.any() and not flags.all()
    for k in range(K):
        # the newest frame of every term of row k + 1 is the raw row of that step
        raw = np.concatenate([rows[k + 1][:, d + (h - 1) * w:d + h * w] for _, w, h, d in tab], axis=1)
        want = R.push_closed(tab, raw, rows[k], flags[k])
        assert np.array_equal(rows[k + 1], want), k
        # and a running env's older frame is the frame it saw one step earlier
        run = ~flags[k]
        assert np.array_equal(rows[k + 1][run][:, 26:26 + 676], rows[k][run][:, 26 + 676:26 + 2 * 676])
    assert np.array_equal(_words(base.obs_buf["policy"]), rows[K])              # the env caught up with the storage
    with pytest.raises(ValueError, match="history"):
        base.collect_rollout(runner.actor_critic.fused(), st)


def test_fused_collection_is_refused_with_history():
    with pytest.raises(ValueError, match="history"):
        _runner("Isaac-MushrDriftRL-v0", 64, 8, _group_h(3), fused=True)
    runner = _runner("Isaac-MushrDriftRL-v0", 64, 8, _group_h(3))
    assert not runner.fused
    with pytest.raises(ValueError, match="history"):
        runner.env.unwrapped.rollout_policy(runner.actor_critic.fused(), runner.storage)


def test_training_smoke_with_history_and_empirical_normalisation(tmp_path):
    n, K = 64, 16
    torch.manual_seed(0)
    runner = _runner("Isaac-MushrDriftRL-v0", n, K, _group_h(3), agent_over=dict(empirical_normalization=True), log_dir=str(tmp_path))
    assert runner.actor_critic.actor[0].in_features == 42 and runner.obs_normalizer is not None
    hist = runner.learn(2, verbose=False)
    assert runner.collection_paths == ["stepwise", "stepwise"]
    for h in hist:
        assert all(np.isfinite(h[k]) for k in ("value_function", "surrogate", "mean_step_reward")), h
    assert int(runner.obs_normalizer.count) == 2 * K * n and runner.obs_normalizer._mean.shape[-1] == 42
    path = os.path.join(str(tmp_path), "models", "model_1.pt")
    assert os.path.exists(path)
    other = _runner("Isaac-MushrDriftRL-v0", n, K, _group_h(3), agent_over=dict(empirical_normalization=True))
    other.load(path)
    for k, v in runner.actor_critic.state_dict().items():
        assert torch.equal(other.actor_critic.state_dict()[k], v), k
    for k, v in runner.obs_normalizer.state_dict().items():
        assert torch.equal(other.obs_normalizer.state_dict()[k], v), k
    assert other.actor_critic.actor[0].weight.shape == (64, 42)
    # the play policy (torch, normalise then act) on the last stored row (raw) against the runner's own policy step on it
    obs = runner.storage.observations[K].clone()
    view = runner.actor_critic.fused()
    a, mu = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
    logp, val = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    view.act(obs, a, mu, logp, val, 1, 2, deterministic=True)
    with torch.no_grad():
        for r in (runner, other):
            got = r.get_inference_policy(device=DEV)(obs)
            torch.testing.assert_close(got, mu, rtol=0, atol=3e-4)            # the policy-step bar of tests/test_gpu_actor_act.py

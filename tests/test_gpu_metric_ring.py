"""The metric ring under every persistent launch path -- rollout(persistent=True) of the three tasks, DriftBatch.rollout_policy
and ElevBatch.collect_rollout -- as core.ring_plan lays it out: a launch clears the slots it folds away, and a run whose length
is a multiple of the ring is the same as explicit launches of 1 and K - 1 steps, with a warning."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, R, STEP0 = 64, 4, 5
COUNTS = slice(8, 16)          # WL_M_RESETS .. WL_M_EPLEN: integer-valued, exact whatever the order of the float atomics
SENTINEL = float("nan")       # stale counts: anything added to them stays NaN
PATHS = ["drift", "elev", "visual", "rollout_policy", "collect_rollout"]


def _batch(path, slots):
    from wheeledlab_amd.core import DriftBatch, ElevBatch, VisualBatch
    task = {"rollout_policy": "drift", "collect_rollout": "elev"}.get(path, path)
    env = {"drift": DriftBatch, "elev": ElevBatch, "visual": VisualBatch}[task](N, device=DEV, seed=11, metrics_slots=slots)
    env.reset()
    L = env.p.max_episode_length            # episodes that end inside the rollout: counts for the ring to book
    env.episode_len[:N] = torch.arange(N, device=DEV, dtype=torch.int32) % 8 + (L - 8)
    env.step_count = STEP0                  # the launch's own slot is STEP0 % R, not the ring's first
    env.metrics_raw.fill_(SENTINEL)         # counts of an earlier pass over the ring ...
    env.metrics_raw[STEP0 % slots] = 0      # ... but the launch's own slot, which its predecessor cleared
    return env


def _path(path, K):
    """(storage, run(env, storage, k0, k): steps k0 .. k0 + k - 1 as one call of the path, outputs(storage)) for twin batches"""
    if path == "rollout_policy":
        from wheeledlab_amd.policy import ActorCritic, RolloutStorage
        ac = ActorCritic(device=DEV, seed=3)
        ac.std.copy_(torch.tensor([0.6, 0.9]))

        def make(env):
            env.observe()
            return RolloutStorage(K, N, device=DEV)

        def run(env, st, k0, k):
            env.rollout_policy(ac, st, evaluate_critic=False, start=k0, count=k)
    elif path == "collect_rollout":
        from wheeledlab_amd.policy import RolloutStorage
        from wheeledlab_amd.rl.ppo import ActorCritic
        torch.manual_seed(5)
        D = 689
        ac = ActorCritic(D, D, 2, activation="elu").to(DEV)
        view = ac.fused()
        view.planes = False

        def make(env):
            st = RolloutStorage(K, N, D, 2, DEV)
            st.observations[0].copy_(env.observe())
            return st

        def run(env, st, k0, k):
            env.collect_rollout(view, st, start=k0, count=k)
    else:
        actions = torch.rand(K, N, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 2 - 1

        def make(env):
            return (torch.zeros(K, N, env.OBS_DIM, device=DEV), torch.zeros(K, N, device=DEV),
                    torch.zeros(K, N, dtype=torch.bool, device=DEV), torch.zeros(K, N, dtype=torch.bool, device=DEV),
                    torch.zeros(K, N, dtype=torch.long, device=DEV))

        def run(env, st, k0, k):
            o, r, te, tr, d = (t[k0:k0 + k] for t in st)
            env.rollout(actions[k0:k0 + k], o, r, te, tr, dones_out=d, persistent=True)

    def outputs(st):
        if isinstance(st, tuple):
            return st
        return st.observations, st.actions, st.mu, st.actions_log_prob, st.rewards, st.terminated, st.time_outs, st.dones
    return make, run, outputs


def _same_batch(ea, eb, oa, ob):
    for i, (x, y) in enumerate(zip(oa, ob)):
        assert torch.equal(x, y), i
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.episode_len, eb.episode_len) and ea.step_count == eb.step_count


@pytest.mark.parametrize("path", PATHS)
def test_launch_clears_the_slots_it_folds_away(path):
    """K % R != 0: one launch.  The slots of steps STEP0 + 1 .. STEP0 + K - 1 (host) and the one after them (kernel) read
    zero; slot STEP0 % R holds the launch's counts -- those of the same launch on a batch without a ring."""
    K = 3
    make, run, outputs = _path(path, K)
    ea, eb = _batch(path, R), _batch(path, 1)
    eb.metrics_raw.zero_()
    sa, sb = make(ea), make(eb)
    run(ea, sa, 0, K)
    run(eb, sb, 0, K)
    torch.cuda.synchronize()
    _same_batch(ea, eb, outputs(sa), outputs(sb))
    cur = STEP0 % R
    for s in range(R):
        if s != cur:
            assert float(ea.metrics_raw[s].abs().sum()) == 0.0, s
    assert float(eb.metrics_raw[0, :, 8].sum()) > 0          # resets happened
    assert torch.equal(ea.metrics_raw[cur, :, COUNTS], eb.metrics_raw[0, :, COUNTS])
    torch.testing.assert_close(ea.metrics_raw[cur], eb.metrics_raw[0], rtol=1e-6, atol=1e-4)


@pytest.mark.parametrize("path", PATHS)
def test_ring_multiple_runs_as_one_and_the_rest(path):
    """K % R == 0: the C ABI refuses the one launch (its slot and the slot it clears coincide); the host runs launches of
    1 and K - 1 steps and warns.  Everything equals a twin batch run as those two launches explicitly."""
    K = 2 * R
    make, run, outputs = _path(path, K)
    ea, eb = _batch(path, R), _batch(path, R)
    sa, sb = make(ea), make(eb)
    with pytest.warns(UserWarning, match="first step's episode counts"):
        run(ea, sa, 0, K)
    run(eb, sb, 0, 1)
    run(eb, sb, 1, K - 1)
    torch.cuda.synchronize()
    _same_batch(ea, eb, outputs(sa), outputs(sb))
    assert ea.step_count == STEP0 + K
    assert torch.equal(ea.metrics_raw[..., COUNTS], eb.metrics_raw[..., COUNTS])
    torch.testing.assert_close(ea.metrics_raw, eb.metrics_raw, rtol=1e-6, atol=1e-4)
    assert bool(torch.isfinite(ea.metrics_raw).all())         # no slot kept the earlier pass's counts
    assert float(ea.metrics_raw[(STEP0 + 1) % R, :, 8].sum()) > 0

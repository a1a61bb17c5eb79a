"""The elevation collector (ElevBatch.collect_rollout, wl_elev_collect_rollout) keeps each env's policy input to its own 689 features.
Its actor reads a block's observation rows from LDS in 16-feature chunks; the last chunk (features 688 .. 703) ends past the 689th.
Those lanes' weights are zero, but 0 x Inf / NaN is NaN: what they read must be zero too, not the next env's row (nor, for the last
row of a block, whatever else lies in LDS -- which made the collector's outputs depend on the kernels that ran before it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K, D = 64, 2, 689


def _collect(poison):
    from wheeledlab_amd.core import ElevBatch
    from wheeledlab_amd.policy import RolloutStorage
    from wheeledlab_amd.rl.ppo import ActorCritic
    env = ElevBatch(N, device=DEV, seed=11)
    env.reset()
    torch.manual_seed(5)
    view = ActorCritic(D, D, 2, activation="elu").to(DEV).fused()
    view.planes = False
    st = RolloutStorage(K, N, D, 2, DEV)
    st.observations[0].copy_(env.observe())
    for e, v in poison.items():
        st.observations[0, e, :12] = v
    env.collect_rollout(view, st, start=0, count=K)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_a_non_finite_observation_stays_in_its_own_env(value):
    """envs 1, 17, 33, 49 start with non-finite proprioception: the first-step policy outputs of every other env are those of a
    clean run, bit for bit (before the fix envs 0, 16, 32, 48 -- the rows before them -- drew NaN actions)"""
    bad = {1: value, 17: value, 33: value, 49: value}
    clean, dirty = _collect({}), _collect(bad)
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[list(bad)] = False
    assert torch.isfinite(clean.mu[0]).all() and torch.isfinite(clean.actions[0]).all()
    assert torch.equal(dirty.mu[0][keep], clean.mu[0][keep])
    assert torch.equal(dirty.actions[0][keep], clean.actions[0][keep])
    assert torch.equal(dirty.actions_log_prob[0][keep], clean.actions_log_prob[0][keep])

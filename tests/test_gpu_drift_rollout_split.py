"""The two-role drift rollout kernel (`pytest -m gpu`): rollout-kernel launches run a STATE wavefront (action term, physics,
terminations, the reset's and the pushes' state changes) and an OUTPUT wavefront (rewards, episode sums, metrics, observation,
every store) per 16 envs, the output work of step k beside step k + 1, handed over through LDS behind one block barrier per step.
FLAG_ROLLOUT_ONE_ROLE keeps the single-role kernel.  Both compute what K calls of step() compute.

Every comparison is between TWIN batches built with the same seed and parameters (the method of test_gpu_drift_rollout_plan.py):
observation, reward, terminated, truncated and `dones` rows of every step, the whole state matrix, episode_len and step_count
with torch.equal; the metric counts exactly; the episode sums to 1e-5 relative (float atomics arrive in another order: <= 64
additions per shard at these sizes, 64 x 2^-24 = 4e-6 of the sum at the worst).

max_episode_length is 3 and both push intervals are (0, 2 step_dt), the batches start with the episode lengths staggered and
both timers at 0: every step has resets, time-outs and both pushes, and each case with K n >= 2 asserts that they occurred.

Shapes: n = 1 (a lone quad), 15 (a block one quad short), 16 (an exact block), 17 (a second block with one quad), 40 (several
blocks, a ragged last one); K = 2 (pipeline prologue and epilogue, nothing between), 3 (odd: slot parity), 5 (steady state),
1027 at n = 17 (across the 1024-step chunk boundary)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle.layout import PX, TIMER_HF, TIMER_LF, VX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
M_SUMS, M_COUNTS = slice(0, 8), slice(8, 16)
M_NONFINITE = 14     # WL_M_NONFINITE


@pytest.fixture(scope="module")
def A():
    from wheeledlab_amd import _abi
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return _abi


def _params(**change):
    from wheeledlab_amd import params as PP
    p = PP.drift_params()
    dt = float(np.float32(p.sim_dt) * np.float32(p.decimation))
    p.max_episode_length, p.enable_pushes, p.log_episode_sums = 3, 1, 1
    p.hf_interval[0], p.hf_interval[1], p.lf_interval[0], p.lf_interval[1] = 0.0, 2 * dt, 0.0, 2 * dt
    for name, value in change.items():
        obj = p
        *path, last = name.split("__")
        for part in path:
            obj = getattr(obj, part)
        assert getattr(obj, last) != value, (name, value)     # "switched to its OTHER value"
        setattr(obj, last, value)
    return p, dt


def _batch(n, ring=1, flags=0, change=(), dones=True, poison=False):
    from wheeledlab_amd.core import DriftBatch
    env = DriftBatch(n, device=DEV, seed=SEED, params=_params(**dict(change))[0], metrics_slots=ring)
    env.set_flags(flags)
    env.set_dones_output(dones)
    env.reset()
    env.state[TIMER_HF].zero_()
    env.state[TIMER_LF].zero_()
    env.episode_len[:n] = ((1 - torch.arange(n, device=DEV)) % 3).to(torch.int32)   # env 2 times out in step 0, env 0 in step 1
    if poison:
        env.state[VX, 3] = float("nan")
        env.state[PX, 9] = float("inf")
    return env


def _actions(K, n):
    g = torch.Generator().manual_seed(100 * K + n)
    return ((torch.rand(K, n, 2, generator=g) * 2 - 1) * 1.2).to(DEV).contiguous()


def _end(env, rows):
    torch.cuda.synchronize()
    return dict(rows=rows, state=env.state.clone(), ep=env.episode_len.clone(), steps=env.step_count, metrics=env.metrics.double().cpu())


def _stepped(env, acts):
    """K calls of step(); -> the end state with rows [K, ...] of every step and the events that occurred"""
    n, dt = env.n, _params()[1]
    rows = [[] for _ in range(5)]
    ev = torch.zeros(4, dtype=torch.long, device=DEV)    # resets, time-outs, hf pushes, lf pushes
    for a in acts:
        hf0, lf0 = env.state[TIMER_HF, :n].clone(), env.state[TIMER_LF, :n].clone()
        obs, rew, te, tr = env.step(a)
        for r, t in zip(rows, (obs, rew, te, tr, env.dones)):
            r.append(t.clone())
        quiet = ~(te | tr)
        ev += torch.stack([(te | tr).sum(), tr.sum(), (quiet & (env.state[TIMER_HF, :n] > hf0 - 0.5 * dt)).sum(),
                           (quiet & (env.state[TIMER_LF, :n] > lf0 - 0.5 * dt)).sum()])
    out = _end(env, [torch.stack(r) for r in rows])
    out["events"] = dict(zip(("resets", "timeouts", "hf", "lf"), ev.tolist()))
    return out


def _rolled(env, acts, split=None, persistent=False, dones=True):
    """rollout() into [K, ...] storage rows, as one call or as calls of `split` steps"""
    K, n = acts.shape[:2]
    rows = [torch.zeros(K, n, 14, device=DEV), torch.zeros(K, n, device=DEV), torch.zeros(K, n, dtype=torch.bool, device=DEV),
            torch.zeros(K, n, dtype=torch.bool, device=DEV), torch.full((K, n), -1, dtype=torch.long, device=DEV)]
    k0 = 0
    for k in split or (K,):
        o, r, te, tr, dn = (t[k0:k0 + k] for t in rows)
        env.rollout(acts[k0:k0 + k], o, r, te, tr, dones_out=dn if dones else None, persistent=persistent)
        k0 += k
    assert k0 == K
    return _end(env, rows)


def _occurred(ref, K, n, pushes=True):
    e = ref["events"]
    print(f"K = {K}, n = {n}: {e}")
    if pushes:
        assert e["hf"] >= 1 and e["lf"] >= 1, e
    if K * n >= 2:
        assert e["resets"] >= 1 and e["timeouts"] >= 1, e


def _same_metrics(got, want, where):
    assert torch.equal(got[..., M_COUNTS], want[..., M_COUNTS]), (where, got[..., M_COUNTS], want[..., M_COUNTS])
    d, scale = (got[..., M_SUMS] - want[..., M_SUMS]).abs(), torch.maximum(got[..., M_SUMS].abs(), want[..., M_SUMS].abs())
    assert bool((d <= 1e-5 * scale).all()), (where, got[..., M_SUMS], want[..., M_SUMS])


def _same(got, want, where, dones=True, metrics=True):
    names = ("obs", "reward", "terminated", "truncated", "dones")
    for name, g, w in zip(names[:5 if dones else 4], got["rows"], want["rows"]):
        assert torch.equal(g, w), (where, name, (g != w).nonzero()[:4].tolist())
    assert torch.equal(got["state"], want["state"]), (where, "state", (got["state"] != want["state"]).nonzero()[:4].tolist())
    assert torch.equal(got["ep"], want["ep"]) and got["steps"] == want["steps"], (where, "episode_len / step_count")
    if metrics:
        _same_metrics(got["metrics"], want["metrics"], where)


CASES = [(K, n) for K in (2, 3, 5) for n in (1, 15, 16, 17, 40)]


@lru_cache(maxsize=None)
def _ref(K, n):
    return _stepped(_batch(n), _actions(K, n))


@pytest.mark.parametrize("K,n", CASES)
def test_two_roles_equal_one_role_and_k_steps(A, K, n):
    ref = _ref(K, n)
    _occurred(ref, K, n)
    two = _rolled(_batch(n), _actions(K, n))
    one = _rolled(_batch(n, flags=A.FLAG_ROLLOUT_ONE_ROLE), _actions(K, n))
    _same(two, one, f"K = {K}, n = {n}: two roles against one role")
    _same(two, ref, f"K = {K}, n = {n}: two roles against step()")


def test_across_the_chunk_boundary(A):
    n, K = 17, A.DRIFT_ROLLOUT_CHUNK_STEPS + 3
    assert K == 1027
    acts = _actions(K, n)
    ref = _stepped(_batch(n), acts)
    _occurred(ref, K, n)
    two = _rolled(_batch(n), acts)
    _same(two, _rolled(_batch(n, flags=A.FLAG_ROLLOUT_ONE_ROLE), acts), f"rollout({K}): two roles against one role")
    _same(two, ref, f"rollout({K}): two roles against step()")


def test_persistent_launch_on_a_metric_ring(A):
    n, K, R = 17, 6, 4
    acts = _actions(K, n)
    _occurred(_ref(K, n), K, n)
    two = _rolled(_batch(n, ring=R), acts, persistent=True)
    one = _rolled(_batch(n, ring=R, flags=A.FLAG_ROLLOUT_ONE_ROLE), acts, persistent=True)
    assert two["metrics"].shape == (R, 16) and float(two["metrics"][:, 8].sum()) >= 1
    _same(two, one, "persistent, ring of 4: two roles against one role")
    _same(two, _ref(K, n), "persistent, ring of 4: two roles against step()", metrics=False)   # (the stepped twin has no ring)


@pytest.mark.parametrize("change", ["log_episode_sums=0", "enable_pushes=0", "enable_corruption=0", "dones_out=None", "vehicle__drive=1"])
def test_one_parameter_switched(A, change):
    n, K = 17, 5
    name, value = change.split("=")
    dones = name != "dones_out"
    ch = () if not dones else ((name, int(value)),)
    acts = _actions(K, n)
    ref = _stepped(_batch(n, change=ch), acts)
    _occurred(ref, K, n, pushes=name != "enable_pushes")
    two = _rolled(_batch(n, change=ch, dones=dones), acts, dones=dones)
    one = _rolled(_batch(n, change=ch, dones=dones, flags=A.FLAG_ROLLOUT_ONE_ROLE), acts, dones=dones)
    if not dones:
        assert bool((two["rows"][4] == -1).all()) and bool((one["rows"][4] == -1).all())     # the optional row: left alone
    _same(two, one, f"{change}: two roles against one role", dones=dones)
    _same(two, ref, f"{change}: two roles against step()", dones=dones)


def test_non_finite_state_crosses_the_hand_off(A):
    n, K = 17, 5
    acts = _actions(K, n)
    ref = _stepped(_batch(n, poison=True), acts)
    _occurred(ref, K, n)
    assert ref["metrics"][M_NONFINITE] == 2, ref["metrics"]
    assert bool(ref["rows"][2][0, 3]) and bool(ref["rows"][2][0, 9])            # both terminated in step 0 ..
    assert bool(torch.isfinite(ref["state"][:23, :n]).all())                      # .. and were reset to finite rows
    two = _rolled(_batch(n, poison=True), acts)
    one = _rolled(_batch(n, poison=True, flags=A.FLAG_ROLLOUT_ONE_ROLE), acts)
    _same(two, one, "non-finite rows: two roles against one role")
    _same(two, ref, "non-finite rows: two roles against step()")


def test_two_calls_back_to_back(A):
    n, K = 17, 5
    acts = _actions(K, n)
    _occurred(_ref(K, n), K, n)
    whole = _rolled(_batch(n), acts)
    parts = _rolled(_batch(n), acts, split=(3, 2))
    _same(parts, whole, "rollout(3) + rollout(2) against rollout(5)")
    _same(parts, _rolled(_batch(n, flags=A.FLAG_ROLLOUT_ONE_ROLE), acts, split=(3, 2)), "3 + 2: two roles against one role")
    _same(parts, _ref(K, n), "rollout(3) + rollout(2) against step()")

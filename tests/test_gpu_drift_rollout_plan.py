"""wl_drift_rollout's launch plan (`pytest -m gpu`): DriftBatch.rollout() with K >= 2 pre-staged steps, ONE metric accumulator
and a batch that steps in the quad form runs as launches of the persistent rollout kernel (at most DRIFT_ROLLOUT_CHUNK_STEPS
steps each); everything else -- a metric ring, a forced lane or streaming form, FLAG_STEP_LAUNCHES, K = 1 -- keeps one launch of
the step kernel per step.  Either way the call computes what K calls of step() compute.

Every comparison is between TWIN batches built with the same seed and parameters: observation, reward, terminated, truncated
and `dones` rows of every step, the whole state matrix, episode_len and step_count with torch.equal; the metric counts
(resets, time-outs, terminations, non-finite, episode-length sum: integers in fp32) exactly; the episode sums to 1e-5 relative
(float atomics arrive in another order: <= 64 additions per shard at these sizes, 64 x 2^-24 = 4e-6 of the sum at the worst).

max_episode_length is 3 and both push intervals are (0, 2 step_dt), the batches start with the episode lengths staggered and
both timers at 0: a third of the envs times out per step, every env is pushed both ways in step 0 and every one to two steps
after.  The stepped twin counts what happened -- resets and time-outs from its flags, a push where an env that did not reset has
its timer re-armed (above `before - step_dt / 2`; not re-armed it is `before - step_dt`) -- and each test asserts that all of it
occurred.  The one case without a reset is K = 1 at n = 1: a single env-step cannot show both, a reset re-arms the timers too."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle.layout import TIMER_HF, TIMER_LF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
M_SUMS, M_COUNTS = slice(0, 8), slice(8, 16)


@pytest.fixture(scope="module")
def A():
    from wheeledlab_amd import _abi
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return _abi


def _params():
    from wheeledlab_amd import params as PP
    p = PP.drift_params()
    dt = float(np.float32(p.sim_dt) * np.float32(p.decimation))
    p.max_episode_length, p.enable_pushes, p.log_episode_sums = 3, 1, 1
    p.hf_interval[0], p.hf_interval[1], p.lf_interval[0], p.lf_interval[1] = 0.0, 2 * dt, 0.0, 2 * dt
    return p, dt


def _batch(n, ring=1, lanes=0, flags=0):
    from wheeledlab_amd.core import DriftBatch
    env = DriftBatch(n, device=DEV, seed=SEED, params=_params()[0], metrics_slots=ring)
    env.set_lanes(lanes)
    env.set_flags(flags)
    env.reset()
    env.state[TIMER_HF].zero_()
    env.state[TIMER_LF].zero_()
    env.episode_len[:n] = ((1 - torch.arange(n, device=DEV)) % 3).to(torch.int32)   # env 2 times out in step 0, env 0 in step 1
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


def _rolled(env, acts, split=None):
    """rollout() into [K, ...] storage rows, as one call or as calls of `split` steps"""
    K, n = acts.shape[:2]
    rows = [torch.zeros(K, n, 14, device=DEV), torch.zeros(K, n, device=DEV), torch.zeros(K, n, dtype=torch.bool, device=DEV),
            torch.zeros(K, n, dtype=torch.bool, device=DEV), torch.full((K, n), -1, dtype=torch.long, device=DEV)]
    k0 = 0
    for k in split or (K,):
        o, r, te, tr, dn = (t[k0:k0 + k] for t in rows)
        env.rollout(acts[k0:k0 + k], o, r, te, tr, dones_out=dn)
        k0 += k
    assert k0 == K
    return _end(env, rows)


def _occurred(ref, K, n):
    e = ref["events"]
    print(f"K = {K}, n = {n}: {e}")
    assert e["hf"] >= 1 and e["lf"] >= 1, e
    if K * n >= 2:
        assert e["resets"] >= 1 and e["timeouts"] >= 1, e
    m = ref["metrics"]
    assert m.dim() == 2 or (m[8] == e["resets"] and m[9] == e["timeouts"])    # (a ring holds its last R - 1 steps only)


def _same_metrics(got, want, where):
    assert torch.equal(got[..., M_COUNTS], want[..., M_COUNTS]), (where, got[..., M_COUNTS], want[..., M_COUNTS])
    d, scale = (got[..., M_SUMS] - want[..., M_SUMS]).abs(), torch.maximum(got[..., M_SUMS].abs(), want[..., M_SUMS].abs())
    assert bool((d <= 1e-5 * scale).all()), (where, got[..., M_SUMS], want[..., M_SUMS])


def _same(got, want, where):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "dones"), got["rows"], want["rows"]):
        assert torch.equal(g, w), (where, name, (g != w).nonzero()[:4].tolist())
    assert torch.equal(got["state"], want["state"]), (where, "state", (got["state"] != want["state"]).nonzero()[:4].tolist())
    assert torch.equal(got["ep"], want["ep"]) and got["steps"] == want["steps"], (where, "episode_len / step_count")
    _same_metrics(got["metrics"], want["metrics"], where)


# a lone quad, either side of a 16-env wavefront, a second wavefront in a 64-thread block; 2049: the first size in 128-thread blocks
CASES = [(K, n) for K in (1, 2, 3, 37) for n in (1, 15, 16, 17, 33)] + [(3, 2049)]


@lru_cache(maxsize=None)
def _ref(K, n):
    return _stepped(_batch(n), _actions(K, n))


@lru_cache(maxsize=None)
def _plan(K, n):
    return _rolled(_batch(n), _actions(K, n))


@pytest.mark.parametrize("K,n", CASES)
def test_rollout_equals_k_steps(A, K, n):
    ref = _ref(K, n)
    _occurred(ref, K, n)
    _same(_plan(K, n), ref, f"K = {K}, n = {n}: rollout() against step()")


@pytest.mark.parametrize("K,n", CASES)
def test_rollout_equals_per_step_launches(A, K, n):
    old = _rolled(_batch(n, flags=A.FLAG_STEP_LAUNCHES), _actions(K, n))
    _occurred(_ref(K, n), K, n)
    _same(_plan(K, n), old, f"K = {K}, n = {n}: rollout() against rollout() with FLAG_STEP_LAUNCHES")
    _same(old, _ref(K, n), f"K = {K}, n = {n}: rollout() with FLAG_STEP_LAUNCHES against step()")


def test_rollout_in_place_rows_hold_the_last_step(A):
    K, n = 5, 33
    ref = _ref(K, n)
    _occurred(ref, K, n)
    env = _batch(n)
    env.rollout(_actions(K, n))              # no storage: the batch's own rows, overwritten each step
    got = _end(env, [t.clone() for t in (env.obs, env.reward, env.terminated, env.truncated, env.dones)])
    last = dict(ref, rows=[r[K - 1] for r in ref["rows"]])
    _same(got, last, "in-place rollout(5) against the stepped twin's last step")
    env2 = _batch(n)
    env2.set_dones_output(False)             # the optional row: left alone
    env2.dones.fill_(-7)
    env2.rollout(_actions(K, n))
    torch.cuda.synchronize()
    assert bool((env2.dones == -7).all()) and torch.equal(env2.obs, got["rows"][0]) and torch.equal(env2.state, got["state"])


def test_rollout_continues_where_the_last_one_ended(A):
    n = 17
    acts = _actions(12, n)
    whole = _rolled(_batch(n), acts)
    parts = _rolled(_batch(n), acts, split=(5, 7))
    ref = _stepped(_batch(n), acts)
    _occurred(ref, 12, n)
    _same(parts, whole, "rollout(5) + rollout(7) against rollout(12)")
    _same(whole, ref, "rollout(12) against step()")


def test_rollout_longer_than_one_launch_is_chunked(A):
    n, K = 17, A.DRIFT_ROLLOUT_CHUNK_STEPS + 3
    acts = _actions(K, n)
    ref = _stepped(_batch(n), acts)
    _occurred(ref, K, n)
    _same(_rolled(_batch(n), acts), ref, f"rollout({K}) against step()")


@pytest.mark.parametrize("K", [6, 8])
def test_metric_ring_keeps_per_step_slots(A, K):
    n, R = 33, 4
    acts = _actions(K, n)
    ref = _stepped(_batch(n, ring=R), acts)
    _occurred(ref, K, n)
    got = _rolled(_batch(n, ring=R), acts)
    assert got["metrics"].shape == (R, 16)
    _same(got, ref, f"ring of {R}, K = {K}: every slot against the stepped twin's")
    # the ring holds the last R - 1 steps (the slot behind the last step is cleared): counts are spread over slots, not folded
    assert int((ref["metrics"][:, 8] > 0).sum()) >= 2, ref["metrics"][:, 8]


@pytest.mark.parametrize("form", ["lanes1", "lanes2", "stream", "step_launches_no_stream"])
def test_forced_forms_keep_their_step_kernel(A, form):
    K, n = 3, 65
    kw = {"lanes1": dict(lanes=1), "lanes2": dict(lanes=2), "stream": dict(flags=A.FLAG_STREAM),
          "step_launches_no_stream": dict(flags=A.FLAG_STEP_LAUNCHES | A.FLAG_NO_STREAM)}[form]
    acts = _actions(K, n)
    ref = _stepped(_batch(n, **kw), acts)
    _occurred(ref, K, n)
    _same(_rolled(_batch(n, **kw), acts), ref, f"{form}: rollout() against step()")

"""The drift step's post-physics tail in every kernel form against tests/drift_tail_reference.py (`pytest -m gpu`).

Each checked step starts from a host copy of the state.  A TWIN batch -- the same form, state, actions and seed, with terminations,
time-outs and pushes switched off in its parameter block -- stores the state after physics, which the step under test overwrites
where an env resets or is pushed: the same instantiation on the same inputs integrates bit for bit the same, which the test asserts
on every env the step neither reset nor pushed.  From there nothing of the physics' error enters a comparison:

  1. the observation row is the observation of the state the step STORED (every env: reset, pushed, neither), against float64 at
     the reference's bound and against `wl_drift_observe` on the same rows at twice that (two fp32 sides);
  2. flags, reward, episode sums, episode length, timers, last action, reset pose and the pushed velocities follow from the
     post-physics rows by the reference's tail, exactly where its table says exact;
  3. the metric counts are exact, the episode-sum metrics within their bound; a car with a NaN velocity (case C) counts once,
     is force-reset, earns 0 and leaves its neighbours alone;
  4. across forms, from the same pre-step state: flags, episode length, timers and reset poses bit for bit; observations and
     rewards within twice the bound where the two forms' physics gave the same bits (and the observations of every reset env:
     they do not depend on the physics); lanes = 2 and the streaming form bit for bit in everything.
Envs the reference's `near_threshold` marks are excused, counted, printed, and held under 1 % of the batch per step; that cap is
checked on the CPU for these inputs by tests/test_drift_tail_reference_cpu.py.  Cases A / B / C, sizes: drift_tail_reference.py."""
import numpy as np
import pytest
import torch

import drift_tail_reference as REF
from oracle.layout import ACT0, EPSUM0, PX, QW, TIMER_HF, TIMER_LF, VX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K, SEED = REF.N_ENVS, REF.K_STEPS, 5
CAP = 0.01


@pytest.fixture(scope="module")
def A():
    from wheeledlab_amd import _abi
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return _abi


def _copy(p):
    return type(p).from_buffer_copy(p)


def _twin_params(p):
    """the same step with nothing after the physics: no termination, no time-out, no push"""
    q = _copy(p)
    q.r_out, q.r_in, q.max_episode_length, q.enable_pushes = 1e18, 0.0, 10 ** 9, 0
    return q


def _batch(p, lanes=0, flags=0, ring=1, startup=None):
    from wheeledlab_amd.core import DriftBatch
    env = DriftBatch(N, device=DEV, seed=SEED, params=p, metrics_slots=ring, startup=startup)
    env.set_lanes(lanes)
    env.set_flags(flags)
    return env


def _case(tag):
    """-> params, host rows [S_COUNT, stride] and episode lengths of the case's start"""
    from wheeledlab_amd import params as PP
    p = REF.apply_case(PP.drift_params(), tag)
    env = _batch(p)
    env.reset()
    torch.cuda.synchronize()
    st, ep = env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy()
    REF.prepare_case(tag, st, ep, N, p)
    return p, st, ep, env.ref_table.cpu().numpy()


def _load(env, st, ep, step):
    env.state.copy_(torch.from_numpy(st))
    env.episode_len.copy_(torch.from_numpy(ep))
    env.step_count = step
    env.metrics_raw.zero_()


def _post_rows(twin, pre):
    """the rows after physics from the twin; a car that went in non-finite comes out non-finite (the twin force-reset it)"""
    post = twin.state.cpu().numpy()[:, :N].copy()
    post[VX, ~np.isfinite(pre[:ACT0, :N]).all(0)] = np.nan
    return post


def _tail(p, ref, pre, pre_ep, post, a, k):
    return REF.tail(post, pre_ep[:N], pre[EPSUM0:EPSUM0 + 8, :N], pre[ACT0:ACT0 + 2, :N], a, p, SEED, k, np.arange(N),
                    timers=(pre[TIMER_HF, :N], pre[TIMER_LF, :N]), ref_table=ref)


def _got(env, obs, rew, te, tr, metrics=True):
    return dict(state=env.state.cpu().numpy()[:, :N].copy(), ep_len=env.episode_len.cpu().numpy()[:N].copy(), obs=obs.cpu().numpy().copy(),
                reward=rew.cpu().numpy().copy(), terminated=te.cpu().numpy().astype(bool), truncated=tr.cpu().numpy().astype(bool),
                metrics=(env.metrics.double().cpu().numpy() if env.metrics_slots == 1 else env.metrics.double().sum(0).cpu().numpy()) if metrics else None)


class Tally:
    def __init__(self, name):
        self.name, self.excused, self.worst, self.steps, self.resets, self.pushed = name, 0, 0.0, 0, 0, 0

    def step(self, got, t, post, p, noise, where):
        fails, excused, worst = REF.check_step(got, t, post, p, noise, where=where)
        assert not fails, fails
        assert excused < CAP * N, (where, excused)
        self.excused, self.worst, self.steps = self.excused + excused, max(self.worst, worst), self.steps + 1
        self.resets += int(t["done"].sum())
        self.pushed += int((t["hf_fire"] | t["lf_fire"]).sum())
        # an env the step neither reset nor pushed: the twin's rows ARE the stored rows (what makes the twin a witness)
        quiet = ~(t["done"] | t["hf_fire"] | t["lf_fire"]) & ~REF.near_threshold(t)
        assert np.array_equal(got["state"][:ACT0][:, quiet], post[:ACT0][:, quiet]), where

    def report(self):
        print(f"{self.name}: {self.steps} steps, {self.resets} resets, {self.pushed} pushed envs, {self.excused} excused "
              f"(cap {CAP * N:.1f} per step), worst |got - ref| / bound {self.worst:.3f}")


def _observe_check(env, got, t, p, noise_t, noise, where):
    """the step's row against wl_drift_observe on the rows the step stored: two fp32 sides, twice the bound"""
    mine = env.observe(noise_t).cpu().numpy().astype(np.float64)
    o = REF.observation(got["state"], got["state"][ACT0:ACT0 + 2], p, noise, REF.events_of(t))
    d = np.abs(got["obs"].astype(np.float64) - mine)
    d[:, 3:6] = np.where(o["wrap_near"], np.minimum(d[:, 3:6], np.abs(REF.TWO_PI - d[:, 3:6])), d[:, 3:6])
    live = ~REF.near_threshold(t)
    bad = (d > 2 * o["bound"]) & live[:, None]
    assert not bad.any(), (where, np.argwhere(bad)[:4].tolist(), float((d / np.maximum(2 * o["bound"], 1e-300))[bad].max()))


FORMS = [("quad", 4, 0), ("lane", 1, 0), ("lane2", 2, 0), ("stream", 0, 1)]


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_step_forms_tail_and_observation_against_float64(A, tag):
    p, st, ep, ref = _case(tag)
    envs = {name: (_batch(_copy(p), lanes, flags), _batch(_twin_params(p), lanes, flags)) for name, lanes, flags in FORMS}
    tally = {name: Tally(f"case {tag} {name}") for name, _, _ in FORMS}
    for k in range(K):
        a = REF.case_actions(k, N)
        noise = REF.case_noise(k, st.shape[1]) if tag == "C" else None
        a_t = torch.from_numpy(a).to(DEV)
        noise_t = None if noise is None else torch.from_numpy(noise).to(DEV)
        res = {}
        for name, (env, twin) in envs.items():
            _load(env, st, ep, k)
            _load(twin, st, ep, k)
            out = [x.clone() for x in env.step(a_t, noise_t)]
            twin.step(a_t, noise_t)
            torch.cuda.synchronize()
            got, post = _got(env, *out), _post_rows(twin, st)
            t = _tail(env.p, ref, st, ep, post, a, k)
            where = f"case {tag} {name} step {k}: "
            tally[name].step(got, t, post, env.p, None if noise is None else noise[:, :N], where)
            _observe_check(env, got, t, env.p, noise_t, None if noise is None else noise[:, :N], where)
            res[name] = (got, t, post)
        # ---- across forms, from the same pre-step state ----
        near = np.zeros(N, bool)
        for got, t, post in res.values():
            near |= REF.near_threshold(t)
        live = ~near
        g0, t0, post0 = res["quad"]
        for name in ("lane", "lane2", "stream"):
            g, t, post = res[name]
            for key in ("terminated", "truncated", "ep_len"):
                assert np.array_equal(g[key][live], g0[key][live]), (tag, k, name, key)
            rows = [TIMER_HF, TIMER_LF]
            assert np.array_equal(g["state"][rows][:, live], g0["state"][rows][:, live]), (tag, k, name, "timers")
            done = t["done"] & t0["done"] & live
            assert np.array_equal(g["state"][PX:QW + 4][:, done], g0["state"][PX:QW + 4][:, done]), (tag, k, name, "reset pose")
            same_phys = (post[:ACT0] == post0[:ACT0]).all(0) & live
            o = REF.observation(g0["state"], g0["state"][ACT0:ACT0 + 2], p, None if noise is None else noise[:, :N], REF.events_of(t0))
            d = np.abs(g["obs"].astype(np.float64) - g0["obs"])
            d[:, 3:6] = np.where(o["wrap_near"], np.minimum(d[:, 3:6], np.abs(REF.TWO_PI - d[:, 3:6])), d[:, 3:6])
            m = (same_phys | done)[:, None]
            assert not ((d > 2 * o["bound"]) & m).any(), (tag, k, name, "obs", float((d / np.maximum(2 * o["bound"], 1e-300))[m.repeat(14, 1)].max()))
            dr = np.abs(g["reward"].astype(np.float64) - g0["reward"])
            assert (dr[same_phys] <= 2 * t0["reward_b"][same_phys]).all(), (tag, k, name, "reward")
        for key in ("state", "obs", "reward", "terminated", "truncated", "ep_len"):     # the same arithmetic: bit for bit (NaN == NaN)
            assert np.array_equal(res["lane2"][0][key], res["stream"][0][key], equal_nan=key in ("state", "obs", "reward")), (tag, k, key)
        if tag == "C" and k == 0:     # the NaN car: counted once, force-reset, 0 reward
            for name, (g, t, post) in res.items():
                e = REF.NAN_ENV
                assert g["terminated"][e] and g["reward"][e] == 0.0 and g["metrics"][14] == 1.0, name
                assert np.isfinite(g["state"][:, e]).all() and (g["state"][VX:ACT0, e] == 0).all(), name
        st, ep = envs["quad"][0].state.cpu().numpy().copy(), envs["quad"][0].episode_len.cpu().numpy().copy()
    for t in tally.values():
        t.report()
        assert t.resets > N // 2
    if tag == "B":
        assert tally["quad"].pushed > 4 * N


@pytest.mark.parametrize("lanes", [4, 1])
def test_f1tenth_step_tail_against_float64(A, lanes):
    """drive = 1 instantiations, the parameter block the registry flattens; noise-tensor mode, seven-step episodes"""
    from test_gpu_drift_parity import _f1tenth_batch
    env, flat = _f1tenth_batch(N, seed=SEED)
    p = flat.params
    p.max_episode_length = REF.MAX_LEN
    p.enable_corruption = 1
    env.set_lanes(lanes)
    twin = _batch(_twin_params(p), lanes, startup=flat.startup)
    ref = env.ref_table.cpu().numpy()
    st, ep = env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy()
    ep[:N] = np.arange(N) % REF.MAX_LEN
    tally = Tally(f"f1tenth lanes {lanes}")
    for k in range(4):
        a, noise = REF.case_actions(k, N), REF.case_noise(k, st.shape[1])
        a_t, noise_t = torch.from_numpy(a).to(DEV), torch.from_numpy(noise).to(DEV)
        _load(env, st, ep, k)
        _load(twin, st, ep, k)
        out = [x.clone() for x in env.step(a_t, noise_t)]
        twin.step(a_t, noise_t)
        torch.cuda.synchronize()
        got, post = _got(env, *out), _post_rows(twin, st)
        t = _tail(p, ref, st, ep, post, a, k)
        tally.step(got, t, post, p, noise[:, :N], f"f1tenth lanes {lanes} step {k}: ")
        _observe_check(env, got, t, p, noise_t, noise[:, :N], f"f1tenth lanes {lanes} step {k}: ")
        st, ep = env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy()
    tally.report()
    assert tally.resets > N // 4


def _outputs(n_steps):
    return (torch.zeros(n_steps, N, 14, device=DEV), torch.zeros(n_steps, N, device=DEV),
            torch.zeros(n_steps, N, dtype=torch.bool, device=DEV), torch.zeros(n_steps, N, dtype=torch.bool, device=DEV))


def test_rollout_is_the_stepping_form_bit_for_bit(A):
    """wl_drift_rollout is K launches of the step the first test checks: hold it to them bit for bit (case B)"""
    p, st, ep, _ = _case("B")
    e1, e2 = _batch(_copy(p)), _batch(_copy(p))
    _load(e1, st, ep, 0)
    _load(e2, st, ep, 0)
    acts = torch.from_numpy(np.stack([REF.case_actions(k, N) for k in range(K)])).to(DEV)
    out = _outputs(K)
    e1.rollout(acts, *out)
    for k in range(K):
        o = e2.step(acts[k])
        for x, y in zip(o, (out[0][k], out[1][k], out[2][k], out[3][k])):
            assert torch.equal(x, y), k
    assert torch.equal(e1.state, e2.state) and torch.equal(e1.episode_len, e2.episode_len) and torch.equal(e1.metrics[8:], e2.metrics[8:])


@pytest.mark.parametrize("ring", [1, 4])
def test_persistent_rollout_tail_against_float64(A, ring):
    """K = 6 steps in one launch (case B).  The rows between its steps never reach memory: the same launch cut after k steps
    (k = 1 .. 6, each from the same start) stores them, its outputs being the first k of the long one's bit for bit; a one-step
    launch of the twin parameters from those rows stores the state after step k's physics."""
    p, st0, ep0, ref = _case("B")
    acts_np = np.stack([REF.case_actions(k, N) for k in range(K)])
    acts = torch.from_numpy(acts_np).to(DEV)
    full = _batch(_copy(p), ring=ring)
    _load(full, st0, ep0, 0)
    out = _outputs(K)
    full.rollout(acts, *out, persistent=True)
    torch.cuda.synchronize()
    tally = Tally(f"persistent rollout ring {ring}")
    st, ep = st0, ep0
    total, total_b = np.zeros(16), np.zeros(16)
    for k in range(K):
        cut = _batch(_copy(p), ring=ring)
        _load(cut, st0, ep0, 0)
        o = _outputs(k + 1)
        cut.rollout(acts[:k + 1].contiguous(), *o, persistent=True)
        twin = _batch(_twin_params(p), ring=ring)
        _load(twin, st, ep, k)
        twin.rollout(acts[k:k + 1].contiguous(), *_outputs(1), persistent=True)
        torch.cuda.synchronize()
        for x, y in zip(o, out):
            assert torch.equal(x, y[:k + 1]), (ring, k)
        got, post = _got(cut, out[0][k], out[1][k], out[2][k], out[3][k], metrics=False), _post_rows(twin, st)
        t = _tail(p, ref, st, ep, post, acts_np[k], k)
        tally.step(got, t, post, p, None, f"persistent ring {ring} step {k}: ")
        flags_same = np.array_equal(got["terminated"], t["terminated"])
        total, total_b = total + t["metrics"], total_b + t["metrics_b"] + (REF.U * np.abs(total) if flags_same else np.inf)
        st, ep = cut.state.cpu().numpy().copy(), cut.episode_len.cpu().numpy().copy()
    assert np.array_equal(full.state.cpu().numpy(), st) and full.step_count == K
    m = full.metrics.double().cpu().numpy()
    if ring > 1:      # every step's metrics in the launch's first slot; the successor's slot is clean
        assert (m[K % ring] == 0).all() and (m[1] == 0).all()
        m = m[0]
    if np.isfinite(total_b).all():
        assert np.array_equal(m[8:], total[8:]), (m[8:], total[8:])
        assert (np.abs(m[:8] - total[:8]) <= total_b[:8] + K * REF.U * np.abs(total[:8])).all(), (m[:8], total[:8], total_b[:8])
    tally.report()
    assert tally.resets > N // 2 and tally.pushed > 4 * N


def test_policy_rollout_first_step_tail_against_float64(A):
    """wl_drift_rollout_policy, one step (case B): the action is the policy's own draw, read back from the storage"""
    from wheeledlab_amd.policy import ActorCritic, RolloutStorage
    p, st, ep, ref = _case("B")
    ac = ActorCritic(device=DEV, seed=2)
    res = []
    for params in (_copy(p), _twin_params(p)):
        env = _batch(params)
        _load(env, st, ep, 0)
        env.observe()
        store = RolloutStorage(1, N, device=DEV)
        env.rollout_policy(ac, store, evaluate_critic=False)
        torch.cuda.synchronize()
        res.append((env, store))
    (env, store), (twin, store_t) = res
    assert torch.equal(store.actions[0], store_t.actions[0])
    a = store.actions[0].cpu().numpy()
    got, post = _got(env, store.observations[1], store.rewards[0], store.terminated[0], store.time_outs[0]), _post_rows(twin, st)
    t = _tail(env.p, ref, st, ep, post, a, 0)
    tally = Tally("policy rollout step 0")
    tally.step(got, t, post, env.p, None, "policy rollout step 0: ")
    tally.report()
    assert tally.resets > 20 and tally.pushed > N // 2

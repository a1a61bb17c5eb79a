"""The visual and visual-depth steps' post-physics tail in every kernel form against tests/visual_tail_reference.py (`pytest -m gpu`),
through core.VisualBatch and core.VisualDepthBatch.

Each checked step starts from a host copy of the rows.  A TWIN batch -- the same form, rows, actions, seed and step, with nothing
after the physics: max_episode_length = 10^9 and, in its WlTravMap, a spacing so large that out_of_map cannot fire (the map does not
enter the physics on either ground) -- stores the state after physics, which the step under test overwrites where an env resets:
the same instantiation on the same inputs integrates bit for bit the same, which the test asserts on every env the step did not
reset.  A car that went in non-finite is marked non-finite (the twin force-reset it).  From there nothing of the physics' error
enters a comparison:

  1. flags, reward, episode sums, episode length, reset pose and velocities, wheel and steering rows and last action follow from the
     post-physics rows by the reference's tail, exactly where its table says exact and within the bound elsewhere;
  2. the traversable_reward and out_of_map of every finite env also equal `wl_visual_mdp` on the post-physics rows bit for bit (the
     step's own: out_of_map from `terminated`, traversable_reward from the reward where its weight is not zero);
  3. metric counts are exact, episode-sum metrics within their bound, rings summed;
  4. the eight proprioceptive values are those of the state the step STORED, against float64 at the reference's bound and against
     `wl_visual_observe` / `wl_visual_depth_observe` on the same rows at twice that (the depth task's are written by the step
     kernel's `prop` path, the plane's by visual_obs_kernel or the persistent kernel's render groups);
  5. on the plane the 3200 camera values equal `observe()` of the stored rows bit for bit, resetting envs included;
  6. across forms, from the same pre-step rows: flags, lengths and reset poses bit for bit, rewards within twice the bound where the
     two forms' physics gave the same bits.
Forms at N = 293 (18 x 16 + 5 envs in the quad form's blocks, 73 x 4 + 1 in the persistent form's).  Plane: set_lanes 0, 4 and 1,
FLAG_STREAM (which selects the lane form) and FLAG_NO_STREAM (the cache-allocating observation kernel), a one-step
`rollout(persistent=True)` with metric rings of 1 and 4, with the LDS bit map and with `_map.bits = None`.  Heightfield: lanes 0 (the
reset-helper wavefront) and lanes 1 (the cached lane sampler).  The K-step `rollout` and `rollout(persistent=True)` against their
one-step chains bit for bit.  The instantiations chosen by size get one staged step each at the smallest size that launches them.

No comparison of this tail has a threshold band (tests/visual_tail_reference.py): ZERO envs are excused, in every form and step.

Case C puts non-finite cars on a heightfield.  The guarantee relied on: HeightFieldGround::cell_of and HeightFieldGroundCached::
sample_wheel (wl_heightfield.h) clamp a contact coordinate into the lattice with fminf(fmaxf(u, 0.f), n - 1 - 1e-3f) before the
conversion to the cell index -- fmaxf(NaN, 0) = 0, +-inf clamp to the ends -- so a non-finite car's gathers stay on the grid;
tests/test_gpu_elev_tail.py case C runs the same samplers with such cars.  Cases A / B / C, sizes: visual_tail_reference.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import visual_tail_reference as REF
from oracle.layout import ACT0, PX, VX, WX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K, SEED = REF.N_ENVS, REF.K_STEPS, 5
MIN_EVENTS = 4
FLAG_STREAM, FLAG_NO_STREAM = 1, 2
# name -> (lanes, flags, metric ring, how the step is launched, the LDS bit map offered)
PLANE_FORMS = {"quad": (0, 0, 1, "step", True), "quad_lanes4": (4, 0, 1, "step", True), "lane": (1, 0, 1, "step", True),
               "lane_by_stream": (0, FLAG_STREAM, 1, "step", True), "quad_no_stream": (0, FLAG_NO_STREAM, 1, "step", True),
               "lane_no_stream": (1, FLAG_NO_STREAM, 1, "step", True), "persistent": (0, 0, 1, "persistent", True),
               "persistent_ring4": (0, 0, 4, "persistent", True), "persistent_bytes": (0, 0, 1, "persistent", False)}
FIELD_FORMS = {"helper": (0, 0, 1, "step", True), "lane_cached": (1, 0, 1, "step", True)}
SAME_KERNEL = (("quad", "quad_lanes4"), ("quad", "quad_no_stream"), ("lane", "lane_by_stream"), ("lane", "lane_no_stream"),
               ("persistent", "persistent_ring4"), ("persistent", "persistent_bytes"))


def _forms(tag):
    return FIELD_FORMS if tag == "C" else PLANE_FORMS


@pytest.fixture(scope="module")
def field():
    """case C's DeviceHeightField, built once for the module"""
    from wheeledlab_amd import _abi
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    return REF.case_field("C").device(DEV)


def _batch(tag, field, n=N, lanes=0, flags=0, ring=1, bits=True):
    from wheeledlab_amd import params as PP
    from wheeledlab_amd.core import VisualBatch, VisualDepthBatch
    m = REF.case_map(tag)
    kw = dict(device=DEV, params=REF.apply_case(PP.visual_params(), tag, 0), seed=SEED, trav_map=m.trav, spacing=(float(m.rs), float(m.cs)),
              metrics_slots=ring)
    env = VisualDepthBatch(n, heightfield=field, max_depth=20.0, **kw) if tag == "C" else VisualBatch(n, **kw)
    env.set_lanes(lanes)
    env.set_flags(flags)
    if tag == "B":
        env.set_dones_output(False)
    if not bits:
        env._map.bits = None
    return env


def _twin(env, tag, k):
    """IN PLACE: the same step with nothing after the physics -- no time-out, no border"""
    REF.apply_case(env.p, tag, k).max_episode_length = 10 ** 9
    env._map.row_spacing = env._map.col_spacing = 1.0e6
    return env


def _start(tag, field, n=N):
    """-> host rows [S_COUNT, stride] and episode lengths of a freshly reset batch"""
    env = _batch(tag, field, n)
    env.reset()
    torch.cuda.synchronize()
    return env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy()


def _load(env, st, ep, step):
    env.state.copy_(torch.from_numpy(st))
    env.episode_len.copy_(torch.from_numpy(ep))
    env.step_count = step
    env.metrics_raw.zero_()
    env.dones.zero_()


def _launch(env, how, a_t, tag):
    """one step in the given way -> (obs, reward, terminated, truncated, dones or None) as fresh tensors"""
    n = env.n
    if how == "step":
        out = [x.clone() for x in env.step(a_t)]
        return out + [None if tag == "B" else env.dones.clone()]
    out = (torch.zeros(1, n, env.OBS_DIM, device=DEV), torch.zeros(1, n, device=DEV), torch.zeros(1, n, dtype=torch.bool, device=DEV),
           torch.zeros(1, n, dtype=torch.bool, device=DEV))
    dones = None if tag == "B" else torch.zeros(1, n, dtype=torch.long, device=DEV)
    env.rollout(a_t[None].contiguous(), *out, dones_out=dones, persistent=True)
    return [x[0] for x in out] + [None if dones is None else dones[0]]


def _got(env, obs, rew, te, tr, dones, cam):
    n = env.n
    m = env.metrics.double()
    o = obs.cpu().numpy()
    return dict(state=env.state.cpu().numpy()[:, :n].copy(), ep_len=env.episode_len.cpu().numpy()[:n].copy(), prop=o[:, -REF.PROP_DIM:].copy(),
                cam=o[:, :-REF.PROP_DIM].copy() if cam else None, reward=rew.cpu().numpy().copy(), terminated=te.cpu().numpy().astype(bool),
                truncated=tr.cpu().numpy().astype(bool), dones=None if dones is None else dones.cpu().numpy().astype(bool),
                metrics=(m if env.metrics_slots == 1 else m.sum(0)).cpu().numpy())


def _post_rows(twin, pre):
    """the rows after physics from the twin; a car that went in non-finite comes out non-finite (the twin force-reset it)"""
    n = twin.n
    post = twin.state.cpu().numpy()[:, :n].copy()
    post[VX, ~np.isfinite(pre[:ACT0, :n]).all(0)] = np.nan
    return post


def _tail(tag, p, st, ep, post, a, k, n=N):
    fld = REF.case_field(tag)
    return REF.tail(post, REF.book_of(st[:, :n], ep[:n]), REF.processed_action(p, a), p, REF.case_map(tag), SEED, k, np.arange(n), fld)


def _mdp_check(env, got, t, post, p, where):
    """wl_visual_mdp on the post-physics positions: its traversable_reward and out_of_map are the reference's and the step's own"""
    n = env.n
    stride = ((n + 63) // 64) * 64
    fin = t["finite"]
    P = torch.zeros(3, stride)
    P[:, :n] = torch.from_numpy(np.where(fin[None], post[PX:PX + 3], 0).astype(np.float32))
    vb = torch.zeros(3, stride)
    P, vb = P.to(DEV), vb.to(DEV)
    terms, oom = torch.zeros(2, stride, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    xi, yi = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    rc = env.lib.wl_visual_mdp(C.byref(env.p), C.byref(env._map), n, stride, P.data_ptr(), vb.data_ptr(), terms.data_ptr(), oom.data_ptr(),
                               xi.data_ptr(), yi.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    trav, out = terms[0, :n].cpu().numpy().astype(np.float64), oom.cpu().numpy().astype(bool)
    assert np.array_equal(trav[fin], t["terms"][0][fin]) and np.array_equal(out[fin], t["oom"][fin]), where
    assert np.array_equal(got["terminated"][fin], out[fin]), where
    w0, w1 = float(np.float32(p.weight[0])), float(np.float32(p.weight[1]))
    if w0 != 0:      # the step's own traversable_reward, from its reward: +-1 apart by |w0| dt, against a bound five orders below
        implied = (got["reward"].astype(np.float64) - w1 * t["terms"][1] * t["dt"]) / (w0 * t["dt"])
        assert np.array_equal(np.rint(implied[fin]), trav[fin]) and np.abs(implied - np.rint(implied))[fin].max() < 1e-3, where


def _observe_check(env, got, where):
    """the step's row against observe() on the rows the step stored: the camera bit for bit (plane), the eight values at twice the
    bound (two fp32 sides)"""
    mine = env.observe().cpu().numpy()
    if got["cam"] is not None:
        assert np.array_equal(got["cam"], mine[:, :-REF.PROP_DIM]), (where, "camera", np.argwhere(got["cam"] != mine[:, :-REF.PROP_DIM])[:4].tolist())
    _, o_b = REF.proprio(got["state"])
    d = np.abs(got["prop"].astype(np.float64) - mine[:, -REF.PROP_DIM:])
    assert (d <= 2 * o_b).all(), (where, np.argwhere(~(d <= 2 * o_b))[:4].tolist())


class Tally:
    def __init__(self, name):
        self.name, self.excused, self.worst, self.steps, self.per, self.events = name, 0, 0.0, 0, {}, {}

    def step(self, tag, got, t, post, p, cls, a, where):
        fails, excused, worst, per = REF.check_step(got, t, p, where=where)
        assert not fails, fails
        assert excused == 0, (where, excused)
        for key, r in per.items():
            self.per[key] = max(self.per.get(key, 0.0), r)
        self.worst, self.steps = max(self.worst, worst), self.steps + 1
        for key, c in REF.events_of(tag, t, cls, post, a).items():
            self.events[key] = self.events.get(key, 0) + c
        # an env the step did not reset: the twin's rows ARE the stored rows (what makes the twin a witness)
        quiet = ~t["done"]
        assert np.array_equal(got["state"][:ACT0][:, quiet], post[:ACT0][:, quiet]), where

    def report(self):
        print(f"{self.name}: {self.steps} steps, 0 excused, worst |got - ref| / bound {self.worst:.3f} ("
              + ", ".join(f"{key} {r:.3f}" for key, r in self.per.items()) + "); " + ", ".join(f"{key} {c}" for key, c in self.events.items()))
        assert self.worst <= 1.0


def _one_step(tag, name, form, env, twin, st, ep, a, k, cls, tally):
    """load, launch the step and its twin, hold the step to the reference -> (got, tail, post-physics rows)"""
    how = form[3]
    a_t = torch.from_numpy(a).to(DEV)
    REF.apply_case(env.p, tag, k)
    _twin(twin, tag, k)
    _load(env, st, ep, k)
    _load(twin, st, ep, k)
    out = _launch(env, how, a_t, tag)
    _launch(twin, how, a_t, tag)
    torch.cuda.synchronize()
    got, post = _got(env, *out, cam=tag != "C"), _post_rows(twin, st)
    if tag == "B":
        assert int(env.dones.sum()) == 0                                   # no `dones` row: nothing is written anywhere in its place
    t = _tail(tag, env.p, st, ep, post, a, k, env.n)
    where = f"case {tag} {name} n {env.n} step {k}: "
    tally.step(tag, got, t, post, env.p, cls, a, where)
    _mdp_check(env, got, t, post, env.p, where)
    _observe_check(env, got, where)
    return got, t, post


def _bad_cars_check(tag, name, got, t):
    """the non-finite cars: terminated, 0 reward, counted once and in none of M_TERM*, rows clean, wheels and steering zeroed"""
    bad = list(REF.BAD_ENVS[tag])
    if not bad:
        assert got["metrics"][14] == 0
        return
    assert got["terminated"][bad].all() and (got["reward"][bad] == 0).all(), name
    assert np.isfinite(got["state"][:, bad]).all() and (got["state"][VX:ACT0 + 2][:, bad] == 0).all(), name
    assert got["metrics"][14] == len(bad) and got["metrics"][10] == t["oom"].sum() and (got["metrics"][11:14] == 0).all(), name


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_step_forms_tail_and_proprioception_against_float64(field, tag):
    forms = _forms(tag)
    st, ep = _start(tag, field)
    envs = {name: (_batch(tag, field, N, *f[:3], bits=f[4]), _batch(tag, field, N, *f[:3], bits=f[4])) for name, f in forms.items()}
    tally = {name: Tally(f"case {tag} {name}") for name in forms}
    base = next(iter(forms))
    for k in range(K):
        cls = REF.stage_step(tag, k, st, ep, N)
        a = REF.case_actions(tag, k, N)
        res = {name: _one_step(tag, name, forms[name], *envs[name], st, ep, a, k, cls, tally[name]) for name in forms}
        # ---- across forms, from the same pre-step rows and actions ----
        g0, t0, post0 = res[base]
        for name in forms:
            g, t, post = res[name]
            _bad_cars_check(tag, name, g, t)
            for key in ("terminated", "truncated", "ep_len"):
                assert np.array_equal(g[key], g0[key]), (tag, k, name, key)
            done = t["done"] & t0["done"]
            assert np.array_equal(g["state"][PX:WX + 3][:, done], g0["state"][PX:WX + 3][:, done]), (tag, k, name, "reset pose and velocities")
            same_phys = ((post[:ACT0] == post0[:ACT0]) | ~t0["finite"][None]).all(0)
            dr = np.abs(g["reward"].astype(np.float64) - g0["reward"])
            assert (dr <= 2 * t0["reward_b"])[same_phys].all(), (tag, k, name, "reward")
        for x, y in SAME_KERNEL:                                           # the same step kernel: bit for bit
            if x in res:
                for key in ("state", "reward", "terminated", "truncated", "ep_len", "prop"):
                    assert np.array_equal(res[x][0][key], res[y][0][key]), (tag, k, x, y, key)
        st, ep = np.zeros_like(st), ep.copy()
        st[:, :N], ep[:N] = g0["state"], g0["ep_len"]
        st[3, N:] = 1
    for name, t in tally.items():
        t.report()
        assert all(c >= MIN_EVENTS for c in t.events.values()), (name, t.events)
        assert t.events["resets"] > N // 2
        if tag == "A":
            assert t.events["spawned on a white cell"] == t.events["resets"]


@pytest.mark.parametrize("tag,how,lanes", [("C", "step", 0), ("C", "step", 1), ("A", "persistent", 0)])
def test_non_finite_cars_leave_their_neighbours_alone(field, tag, how, lanes):
    """first step of the case, the helper-wavefront and lane forms on the heightfield and the persistent kernel on the plane: with
    and without the non-finite cars every other env's rows and outputs are the same bits (their quad blocks' and helper blocks' too)"""
    st, ep = _start(tag, field)
    REF.stage_step(tag, 0, st, ep, N)
    bad = list(REF.BAD_ENVS[tag])
    clean = st.copy()
    clean[:ACT0, bad] = clean[:ACT0, [b + 1 for b in bad]]
    assert np.isfinite(clean[:ACT0, :N]).all() and not np.isfinite(st[:ACT0, bad]).all(0).any()
    a_t = torch.from_numpy(REF.case_actions(tag, 0, N)).to(DEV)
    others = np.ones(N, bool)
    others[bad] = False
    outs = []
    for rows in (st, clean):
        env = _batch(tag, field, N, lanes)
        _load(env, rows, ep, 0)
        o = _launch(env, how, a_t, tag)
        torch.cuda.synchronize()
        outs.append(_got(env, *o, cam=tag != "C"))
    for key in ("state", "prop", "cam", "reward", "terminated", "truncated", "ep_len"):
        if outs[0][key] is not None:
            x, y = (g[key][..., others] if key == "state" else g[key][others] for g in outs)
            assert np.array_equal(x, y), (tag, how, lanes, key)
    assert outs[0]["metrics"][14] == len(bad) and outs[1]["metrics"][14] == 0


def _rows(env, n_steps):
    n = env.n
    return (torch.zeros(n_steps, n, env.OBS_DIM, device=DEV), torch.zeros(n_steps, n, device=DEV),
            torch.zeros(n_steps, n, dtype=torch.bool, device=DEV), torch.zeros(n_steps, n, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("tag,persistent,ring", [("A", False, 1), ("A", True, 1), ("B", True, 4), ("B", False, 1), ("C", False, 1)])
def test_k_step_launches_are_their_one_step_chains_bit_for_bit(field, tag, persistent, ring):
    """`rollout` and `rollout(persistent=True)` of K steps against K one-step launches of the form the first test holds to float64,
    from the case's staged first step (non-finite cars, border cars and time-outs included)"""
    st, ep = _start(tag, field)
    REF.stage_step(tag, 0, st, ep, N)
    acts = torch.from_numpy(np.stack([REF.case_actions(tag, k, N) for k in range(K)])).to(DEV)
    e1, e2 = _batch(tag, field, ring=ring), _batch(tag, field, ring=ring)
    for e in (e1, e2):
        _load(e, st, ep, 0)
    out = _rows(e1, K)
    e1.rollout(acts, *out, persistent=persistent)
    for k in range(K):
        o = _rows(e2, 1)
        e2.rollout(acts[k:k + 1].contiguous(), *o, persistent=persistent)
        for x, y in zip(o, out):
            assert torch.equal(x[0], y[k]), (tag, k)
    torch.cuda.synchronize()
    assert torch.equal(e1.state, e2.state) and torch.equal(e1.episode_len, e2.episode_len)
    if ring == 1:
        m1, m2 = e1.metrics, e2.metrics
        assert torch.equal(m1[8:], m2[8:])
        assert torch.allclose(m1[:8], m2[:8], rtol=1e-5, atol=1e-5)        # sums of the same values in another order
        assert float(m1[8]) == float((out[2] | out[3]).sum()) and float(m1[14]) >= len(REF.BAD_ENVS[tag])
    assert int((out[2] | out[3]).sum()) > N // 2 and torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()


# the instantiations the launchers choose by size, each at the smallest size that launches it: (case, envs, forms)
SIZED = [("A", 2049, ("quad", "persistent", "persistent_bytes")),     # quad blocks of 128 threads; persistent, 16 envs per block
         ("A", 1025, ("persistent", "persistent_bytes")),             # persistent, 8 envs per block (both with and without the LDS bit map)
         ("A", 8193, ("quad",)),                    # quad blocks of 256 threads
         ("C", 8193, ("helper",))]                  # lanes 0 above 8192 envs: the heightfield quad form WITHOUT the helper wavefront


@pytest.mark.parametrize("tag,n,names", SIZED, ids=[f"{t}-{n}" for t, n, _ in SIZED])
def test_instantiations_chosen_by_size_one_staged_step(field, tag, n, names):
    st, ep = _start(tag, field, n)
    cls = REF.stage_step(tag, 0, st, ep, n)
    a = REF.case_actions(tag, 0, n)
    forms = _forms(tag)
    for name in names:
        f = forms[name]
        tally = Tally(f"case {tag} {name} at {n} envs")
        env, twin = _batch(tag, field, n, *f[:3], bits=f[4]), _batch(tag, field, n, *f[:3], bits=f[4])
        got, t, _ = _one_step(tag, name, f, env, twin, st, ep, a, 0, cls, tally)
        _bad_cars_check(tag, name, got, t)
        tally.report()
        assert tally.events["resets"] > n // 8 and tally.events["left +x"] >= MIN_EVENTS and tally.events["time-out and out_of_map"] >= MIN_EVENTS

"""The elevation step's post-physics tail in every kernel form against tests/elev_tail_reference.py (`pytest -m gpu`), through the
C ABI (core.ElevBatch).

Each checked step starts from a host copy of the rows.  A TWIN batch -- the same form, rows, actions, seed and step, with
everything after the physics switched off in its parameter copy (no termination, no time-out) -- stores the state after physics,
which the step under test overwrites where an env resets: the same instantiation on the same inputs integrates bit for bit the same,
which the test asserts on every env the step did not reset.  From there nothing of the physics' error enters a comparison:

  1. flags, reward, episode sums, episode length, timer, targets, level, reset pose and velocities follow from the post-physics
     rows by the reference's tail, exactly where its table says exact;
  2. CMD_BX / CMD_BY and the 13 proprioceptive values are those of the state the step STORED (every env: reset, resampled, neither),
     against float64 at the reference's bound and against `wl_elev_observe` on the same rows at twice that (two fp32 sides);
  3. the 676 scan values equal `wl_elev_observe` on the stored rows bit for bit, resetting envs included;
  4. the metric counts are exact, the episode-sum metrics within their bound, rings summed;
  5. across forms, from the same pre-step rows: flags, episode length, level, timers, targets and reset poses bit for bit; rewards
     and the 13 values within twice the bound where the two forms' physics gave the same bits (the 13 values of every reset env).
Forms: the fused step + scan launch (lanes 0 and 4), the lane-form step + scan launch with FLAG_STREAM and FLAG_NO_STREAM, a one-step
`rollout(persistent=True)` with metric rings of 1 and 4, a one-step `collect_rollout` with an ELU and a ReLU actor; the K-step
`rollout`, `rollout(persistent=True)` and `collect_rollout` against their one-step chains bit for bit.
Envs the reference's `near_threshold` marks are excused, counted, printed, and held under 1 % of the batch per step; that cap is
checked on the CPU for these inputs by tests/test_elev_tail_reference_cpu.py.  Cases A / B / C, sizes: elev_tail_reference.py."""
import numpy as np
import pytest
import torch

import elev_tail_reference as REF
from oracle import heightfield as OH
from oracle.layout import ACT0, CMD_TIMER, PX, QW, TGT_H, TGT_X, VX, WX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K, SEED = REF.N_ENVS, REF.K_STEPS, 5
CAP = 0.01
# name -> (lanes, flags, metric ring, how the step is launched)
FORMS = {"fused": (0, 0, 1, "step"), "quad": (4, 0, 1, "step"), "lane_stream": (1, 1, 1, "step"), "lane_no_stream": (1, 2, 1, "step"),
         "persistent": (0, 0, 1, "persistent"), "persistent_ring4": (0, 0, 4, "persistent"),
         "collect_elu": (0, 0, 1, "elu"), "collect_relu": (0, 0, 1, "relu")}
SAME_ACTIONS = ("fused", "quad", "lane_stream", "lane_no_stream", "persistent", "persistent_ring4")


@pytest.fixture(scope="module")
def fields():
    """tag -> (DeviceHeightField, what the reference takes): built once for the module"""
    import heightfield_cases
    from wheeledlab_amd import _abi
    from wheeledlab_amd.core import DeviceHeightField, generate_heightfield
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _abi.load()
    out = {}
    hf = OH.make_terrain()
    out["A"] = (DeviceHeightField(hf, DEV), REF.field_of(hf))
    gen = generate_heightfield(REF.tile_cfg(), DEV)
    torch.cuda.synchronize()
    out["B"] = (gen, REF.field_of((gen.heights.cpu().numpy().copy(), gen.x0, gen.y0, gen.cell, gen.outside_z)))
    g1 = heightfield_cases.get("G1")
    out["C"] = (g1.device(DEV), g1)
    return out


@pytest.fixture(scope="module")
def actors():
    from wheeledlab_amd.rl.ppo import ActorCritic
    out = {}
    for act in ("elu", "relu"):
        torch.manual_seed(3)
        ac = ActorCritic(REF.OBS_DIM, REF.OBS_DIM, 2, activation=act).to(DEV)
        view = ac.fused()
        view.planes = False
        out[act] = (ac, view)
    return out


def _twin(q):
    """IN PLACE: the same step with nothing after the physics -- no termination, no time-out"""
    q.min_height, q.stuck_wheel_spin, q.upright_cos, q.goal_dist, q.max_episode_length = -1e30, 1e30, -2.0, 0.0, 10 ** 9
    return q


def _batch(tag, fields, lanes=0, flags=0, ring=1):
    from wheeledlab_amd import params as PP
    from wheeledlab_amd.core import ElevBatch, TerrainLevels
    tl = TerrainLevels(REF.tile_cfg(), N, DEV, 0, None, None, SEED) if tag == "B" else None
    env = ElevBatch(N, device=DEV, params=REF.apply_case(PP.elev_params(), tag, 0), seed=SEED, heightfield=fields[tag][0], metrics_slots=ring,
                    terrain_levels=tl)
    env.set_lanes(lanes)
    env.set_flags(flags)
    return env


def _start(tag, fields):
    """-> host rows [S_COUNT, stride], episode lengths and levels of a freshly reset batch, and the level tables for the reference"""
    env = _batch(tag, fields)
    env.reset()
    torch.cuda.synchronize()
    st, ep = env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy()
    lv = tables = None
    if env.levels is not None:
        lv = env.levels.level.cpu().numpy().copy()
        tables = dict(type=env.levels.type.cpu().numpy().copy(), origins=env.levels.origins.cpu().numpy().copy(), rows=REF.TILE_ROWS, cols=REF.TILE_COLS)
    return st, ep, lv, tables


def _load(env, st, ep, lv, step):
    env.state.copy_(torch.from_numpy(st))
    env.episode_len.copy_(torch.from_numpy(ep))
    if lv is not None:
        env.levels.level.copy_(torch.from_numpy(lv))
    env.step_count = step
    env.metrics_raw.zero_()


def _launch(env, how, a_t, actors):
    """one step in the given way -> (obs [n, 689], reward, terminated, truncated, actions [n, 2]) as fresh tensors"""
    if how == "step":
        o = env.step(a_t)
        return [x.clone() for x in o] + [a_t]
    if how == "persistent":
        out = (torch.zeros(1, N, REF.OBS_DIM, device=DEV), torch.zeros(1, N, device=DEV), torch.zeros(1, N, dtype=torch.bool, device=DEV),
               torch.zeros(1, N, dtype=torch.bool, device=DEV))
        env.rollout(a_t[None].contiguous(), *out, persistent=True)
        return [x[0] for x in out] + [a_t]
    from wheeledlab_amd.policy import RolloutStorage
    store = RolloutStorage(1, N, REF.OBS_DIM, 2, DEV)
    store.observations[0].copy_(env.observe())
    env.collect_rollout(actors[how][1], store, start=0, count=1, deterministic=True)
    return [store.observations[1], store.rewards[0], store.terminated[0], store.time_outs[0], store.actions[0]]


def _got(env, obs, rew, te, tr):
    m = env.metrics.double()
    return dict(state=env.state.cpu().numpy()[:, :N].copy(), ep_len=env.episode_len.cpu().numpy()[:N].copy(), obs=obs.cpu().numpy().copy(),
                reward=rew.cpu().numpy().copy(), terminated=te.cpu().numpy().astype(bool), truncated=tr.cpu().numpy().astype(bool),
                level=None if env.levels is None else env.levels.level.cpu().numpy().copy(),
                metrics=(m if env.metrics_slots == 1 else m.sum(0)).cpu().numpy())


def _post_rows(twin, pre):
    """the rows after physics from the twin; a car that went in non-finite comes out non-finite (the twin force-reset it)"""
    post = twin.state.cpu().numpy()[:, :N].copy()
    post[VX, ~np.isfinite(pre[:ACT0, :N]).all(0)] = np.nan
    return post


class Tally:
    def __init__(self, name):
        self.name, self.excused, self.worst, self.steps, self.resets, self.resampled = name, 0, 0.0, 0, 0, 0
        self.flags, self.per = np.zeros(4, int), {}

    def step(self, got, t, post, p, where):
        fails, excused, worst, per = REF.check_step(got, t, p, where=where)
        assert not fails, fails
        for key, r in per.items():
            self.per[key] = max(self.per.get(key, 0.0), r)
        assert excused < CAP * N, (where, excused)
        self.excused, self.worst, self.steps = self.excused + excused, max(self.worst, worst), self.steps + 1
        self.resets, self.resampled, self.flags = self.resets + int(t["done"].sum()), self.resampled + int(t["expired"].sum()), self.flags + t["flags"].sum(1)
        # an env the step did not reset: the twin's rows ARE the stored rows (what makes the twin a witness)
        quiet = ~t["done"] & ~REF.near_threshold(t) & (got["terminated"] == t["terminated"])
        assert np.array_equal(got["state"][:ACT0][:, quiet], post[:ACT0][:, quiet]), where

    def report(self):
        print(f"{self.name}: {self.steps} steps, {self.resets} resets (low / stuck / rolled / at goal {self.flags.tolist()}), {self.resampled} resampled, "
              f"{self.excused} excused (cap {CAP * N:.1f} per step), worst |got - ref| / bound {self.worst:.3f} ("
              + ", ".join(f"{key} {r:.3f}" for key, r in self.per.items()) + ")")


def _observe_check(env, got, t, p, where):
    """the step's row against wl_elev_observe on the rows the step stored: the 13 values at twice the bound (two fp32 sides; the quad
    and lane forms evaluate the Euler angles differently), the 676 scan values bit for bit"""
    mine = env.observe().cpu().numpy()
    assert np.array_equal(got["obs"][:, 13:], mine[:, 13:]), (where, "scan", np.argwhere(got["obs"][:, 13:] != mine[:, 13:])[:4].tolist())
    o = REF.observation(got["state"], p)
    d = np.abs(got["obs"][:, :13].astype(np.float64) - mine[:, :13])
    d[:, 2:5] = np.where(o["wrap_near"], np.minimum(d[:, 2:5], np.abs(REF.TWO_PI - d[:, 2:5])), d[:, 2:5])
    live = ~REF.near_threshold(t)
    bad = ~(d <= 2 * o["bound"]) & live[:, None]
    assert not bad.any(), (where, np.argwhere(bad)[:4].tolist())


def _tail(p, field, tables, st, ep, lv, post, a, k):
    levels = None if tables is None else dict(tables, level=lv[:N])
    return REF.tail(post, REF.book_of(st[:, :N], ep[:N]), REF.processed_action(p, a), p, SEED, k, np.arange(N), field, levels)


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_step_forms_tail_and_observation_against_float64(fields, actors, tag):
    st, ep, lv, tables = _start(tag, fields)
    field = fields[tag][1]
    envs = {name: (_batch(tag, fields, lanes, flags, ring), _batch(tag, fields, lanes, flags, ring)) for name, (lanes, flags, ring, _) in FORMS.items()}
    tally = {name: Tally(f"case {tag} {name}") for name in FORMS}
    for k in range(K):
        REF.stage_step(tag, k, st, ep, N, lv)
        a = REF.case_actions(tag, k, N)
        a_t = torch.from_numpy(a).to(DEV)
        res = {}
        for name, (env, twin) in envs.items():
            how = FORMS[name][3]
            REF.apply_case(env.p, tag, k)
            _twin(REF.apply_case(twin.p, tag, k))
            _load(env, st, ep, lv, k)
            _load(twin, st, ep, lv, k)
            out = _launch(env, how, a_t, actors)
            out_t = _launch(twin, how, a_t, actors)
            torch.cuda.synchronize()
            assert torch.equal(out[4], out_t[4]), (tag, k, name, "the twin acted otherwise")
            got, post = _got(env, *out[:4]), _post_rows(twin, st)
            t = _tail(env.p, field, tables, st, ep, lv, post, out[4].cpu().numpy(), k)
            where = f"case {tag} {name} step {k}: "
            tally[name].step(got, t, post, env.p, where)
            _observe_check(env, got, t, env.p, where)
            res[name] = (got, t, post)
        # ---- across forms, from the same pre-step rows and actions ----
        near = np.zeros(N, bool)
        for name in SAME_ACTIONS:
            near |= REF.near_threshold(res[name][1])
        live = ~near
        g0, t0, post0 = res["fused"]
        o0 = REF.observation(g0["state"], envs["fused"][0].p)
        for name in SAME_ACTIONS[1:]:
            g, t, post = res[name]
            for key in ("terminated", "truncated", "ep_len") + (("level",) if lv is not None else ()):
                assert np.array_equal(g[key][live], g0[key][live]), (tag, k, name, key)
            rows = [TGT_X, TGT_X + 1, TGT_H, CMD_TIMER]
            assert np.array_equal(g["state"][rows][:, live], g0["state"][rows][:, live], equal_nan=True), (tag, k, name, "timers and targets")
            done = t["done"] & t0["done"] & live
            assert np.array_equal(g["state"][PX:WX + 3][:, done], g0["state"][PX:WX + 3][:, done]), (tag, k, name, "reset pose and velocities")
            same_phys = (post[:ACT0] == post0[:ACT0]).all(0) & live
            d = np.abs(g["obs"][:, :13].astype(np.float64) - g0["obs"][:, :13])
            d[:, 2:5] = np.where(o0["wrap_near"], np.minimum(d[:, 2:5], np.abs(REF.TWO_PI - d[:, 2:5])), d[:, 2:5])
            m = (same_phys | done)[:, None]
            assert not (~(d <= 2 * o0["bound"]) & m).any(), (tag, k, name, "the 13 values")
            with np.errstate(invalid="ignore"):
                dr = np.abs(g["reward"].astype(np.float64) - g0["reward"])
                ok = (dr <= 2 * t0["reward_b"]) | (np.isnan(g["reward"]) & np.isnan(g0["reward"])) | (g["reward"] == g0["reward"])
            assert ok[same_phys].all(), (tag, k, name, "reward")
        for key in ("state", "obs", "reward", "terminated", "truncated", "ep_len"):     # the same kernel: bit for bit (NaN == NaN)
            for x, y in (("fused", "quad"), ("lane_stream", "lane_no_stream"), ("persistent", "persistent_ring4")):
                assert np.array_equal(res[x][0][key], res[y][0][key], equal_nan=key in ("state", "obs", "reward")), (tag, k, x, y, key)
        if tag == "C":     # the non-finite cars: counted once, in none of M_TERM*, force-reset, 0 reward, rows clean
            for name, (g, t, post) in res.items():
                for e in (REF.NAN_ENV, REF.INF_ENV):
                    assert g["terminated"][e] and g["reward"][e] == 0.0, (name, e)
                    assert np.isfinite(g["state"][:, e]).all() and (g["state"][WX:ACT0 + 2, e] == 0).all(), (name, e)
                assert g["metrics"][14] == 2.0 and g["metrics"][10:14].sum() == t["flags"].sum(), name
        st, ep = np.zeros_like(st), ep.copy()
        st[:, :N], ep[:N] = g0["state"], g0["ep_len"]
        st[QW, N:] = 1
        if lv is not None:
            lv = g0["level"].copy()
    for name, t in tally.items():
        t.report()
        # (the collector's actor drives otherwise: its cars are rarely stuck; the three staged flags still fire)
        assert t.resets > N // 2 and (t.flags[[0, 2, 3]] >= 10).all() and t.resampled >= 20
        assert name not in SAME_ACTIONS or t.flags[1] >= 10
    if tag == "B":
        assert tally["fused"].resampled > N


def test_non_finite_cars_leave_their_neighbours_alone(fields):
    """case C, first step, fused and lane forms: with and without the NaN and the inf car every other env's rows and outputs are the
    same bits"""
    st, ep, lv, _ = _start("C", fields)
    REF.stage_step("C", 0, st, ep, N, lv)
    clean = st.copy()
    clean[VX, REF.NAN_ENV], clean[VX + 1, REF.INF_ENV] = 0.1, 0.1
    a_t = torch.from_numpy(REF.case_actions("C", 0, N)).to(DEV)
    others = np.ones(N, bool)
    others[[REF.NAN_ENV, REF.INF_ENV]] = False
    for lanes in (0, 1):
        outs = []
        for rows in (st, clean):
            env = _batch("C", fields, lanes)
            _load(env, rows, ep, lv, 0)
            o = [x.clone() for x in env.step(a_t)]
            torch.cuda.synchronize()
            outs.append(_got(env, *o))
        for key in ("state", "obs", "reward", "terminated", "truncated", "ep_len"):
            x, y = (g[key][..., others] if key == "state" else g[key][others] for g in outs)
            assert np.array_equal(x, y, equal_nan=True), (lanes, key)
        assert outs[0]["metrics"][14] == 2 and outs[1]["metrics"][14] == 0


def _rows(n_steps):
    return (torch.zeros(n_steps, N, REF.OBS_DIM, device=DEV), torch.zeros(n_steps, N, device=DEV),
            torch.zeros(n_steps, N, dtype=torch.bool, device=DEV), torch.zeros(n_steps, N, dtype=torch.bool, device=DEV))


def _chain_start(tag, fields):
    st, ep, lv, _ = _start(tag, fields)
    REF.stage_step(tag, 0, st, ep, N, lv)
    return st, ep, lv


def _same_end(e1, e2, counts_only_from=8):
    assert np.array_equal(e1.state.cpu().numpy(), e2.state.cpu().numpy(), equal_nan=True) and torch.equal(e1.episode_len, e2.episode_len)
    if e1.levels is not None:
        assert torch.equal(e1.levels.level, e2.levels.level)
    m1 = e1.metrics if e1.metrics_slots == 1 else e1.metrics.sum(0)
    m2 = e2.metrics if e2.metrics_slots == 1 else e2.metrics.sum(0)
    assert torch.equal(m1[counts_only_from:], m2[counts_only_from:])
    assert torch.allclose(m1[:counts_only_from], m2[:counts_only_from], rtol=1e-5, atol=1e-5, equal_nan=True)       # sums of the same values in another order


@pytest.mark.parametrize("tag,persistent,ring", [("A", False, 1), ("B", False, 1), ("B", True, 1), ("B", True, 4), ("C", True, 1)])
def test_k_step_launches_are_their_one_step_chains_bit_for_bit(fields, tag, persistent, ring):
    """`rollout` and `rollout(persistent=True)` of K steps against K one-step launches of the form the first test holds to float64"""
    st, ep, lv = _chain_start(tag, fields)
    acts = torch.from_numpy(np.stack([REF.case_actions(tag, k, N) for k in range(K)])).to(DEV)
    e1, e2 = _batch(tag, fields, ring=ring), _batch(tag, fields, ring=ring)
    for e in (e1, e2):
        REF.apply_case(e.p, tag, K - 1)
        _load(e, st, ep, lv, 0)
    out = _rows(K)
    e1.rollout(acts, *out, persistent=persistent)
    for k in range(K):
        o = _rows(1)
        e2.rollout(acts[k:k + 1].contiguous(), *o, persistent=persistent)
        for x, y in zip(o, out):
            assert torch.equal(x[0], y[k]) or (x.dtype == torch.float32 and np.array_equal(x[0].cpu().numpy(), y[k].cpu().numpy(), equal_nan=True)), (tag, k)
    torch.cuda.synchronize()
    if ring == 1:
        _same_end(e1, e2)
    else:      # a ring keeps its last steps only: the rows and the levels are what is compared
        assert torch.equal(e1.state, e2.state) and torch.equal(e1.episode_len, e2.episode_len) and torch.equal(e1.levels.level, e2.levels.level)
    assert int(out[2].sum() + out[3].sum()) > N // 2


@pytest.mark.parametrize("act", ["elu", "relu"])
def test_k_step_collection_is_its_one_step_chain_bit_for_bit(fields, actors, act):
    from wheeledlab_amd.policy import RolloutStorage
    tag = "B"
    st, ep, lv = _chain_start(tag, fields)
    e1, e2 = _batch(tag, fields), _batch(tag, fields)
    stores = RolloutStorage(K, N, REF.OBS_DIM, 2, DEV), RolloutStorage(K, N, REF.OBS_DIM, 2, DEV)
    for e, s in zip((e1, e2), stores):
        REF.apply_case(e.p, tag, K - 1)
        _load(e, st, ep, lv, 0)
        s.observations[0].copy_(e.observe())
    e1.collect_rollout(actors[act][1], stores[0], start=0, count=K, deterministic=True)
    for k in range(K):
        e2.collect_rollout(actors[act][1], stores[1], start=k, count=1, deterministic=True)
    torch.cuda.synchronize()
    for name in ("observations", "actions", "rewards", "terminated", "time_outs"):
        x, y = getattr(stores[0], name), getattr(stores[1], name)
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), name
    _same_end(e1, e2)
    assert int(stores[0].terminated.sum() + stores[0].time_outs.sum()) > N // 2

"""tests/visual_tail_reference.py (the visual and visual-depth steps' tail in float64) held to the numpy oracle
(oracle/visual_step.step) on exactly the inputs of tests/test_gpu_visual_tail.py, to the reference project's golden terms and
flags and their edge sets, its bound shown to accept the correct wiring (restated in fp32 numpy, two summation orders) and to reject
sixteen modelled wiring defects on the cases' own rows; every staged event of the cases occurs, and no env is excused."""
import numpy as np
import pytest

import visual_tail_reference as REF
from oracle import elev_step as OE
from oracle import env_step as ES
from oracle import visual_step as VS
from oracle.layout import ACT0, EPSUM0, PX, QW, S_COUNT, STEER_POS, STEER_VEL, VX, WHEEL, WX
from tests import parity_predicates as PRED
from tests.parity_predicates import edge_golden  # noqa: F401  (fixture)

F = np.float32
SEED = 5
N, K = REF.N_ENVS, REF.K_STEPS
MIN_EVENTS = 4


@pytest.fixture()
def oracle_takes_non_finite_cars(monkeypatch):
    """the visual oracle on a heightfield with cars that may be non-finite, and without its compiled depth image: the wheels of a
    non-finite car sample the terrain at (0, 0) instead of at NaN (the oracle's sampler indexes with the coordinate; such a car stays
    non-finite through its other rows and is scrubbed and reset), and the observation keeps its eight proprioceptive values"""
    ground = OE.ground_fn

    def safe_ground(hf, probe=None):
        g = ground(hf, probe)
        return lambda xy: g(np.where(np.isfinite(xy), xy, F(0)).astype(F))

    def prop_only(p, state, hf, max_depth):
        v_b, w_b = ES.body_velocities(state)
        return np.concatenate([np.zeros((state.shape[1], 4800), F), v_b, w_b, np.clip(state[ACT0:ACT0 + 2].T, F(-1), F(1))], -1).astype(F)
    monkeypatch.setattr(OE, "ground_fn", safe_ground)
    monkeypatch.setattr(VS, "observe_depth", prop_only)
    return safe_ground


def _oracle_params(tag, k):
    return REF.apply_case(VS.visual_params(), tag, k)


def oracle_steps(tag, safe_ground, n=N, steps=K, seed=SEED):
    """the case's steps on the oracle: yields (k, p, staged classes, pre rows, pre ep_len, post-physics rows, actions, oracle outputs)"""
    m, fld = REF.case_map(tag), REF.case_field(tag)
    hf = None if fld is None else fld.oracle()
    p = _oracle_params(tag, 0)
    st = VS.init_state(p, n, seed, stride=n)
    ep = np.zeros(n, np.int32)
    VS.reset_envs(p, st, ep, m.cells, np.arange(n), seed, 0, hf=hf)
    for k in range(steps):
        p = _oracle_params(tag, k)
        cls = REF.stage_step(tag, k, st, ep, n)
        a = REF.case_actions(tag, k, n)
        pre, pre_ep = st.copy(), ep.copy()
        post = st.copy()
        with np.errstate(all="ignore"):
            steer_t, wheel_t = ES.fwd_targets(p, ES.apply_action(p, post, a))
            ES.integrate(p, post, steer_t, wheel_t, *(() if hf is None else (safe_ground(hf),)))
            met = np.zeros(16)
            obs, rew, term, trunc, _ = VS.step(p, st, ep, m.trav, m.cells, a, seed, k, met, hf=hf, max_depth=20.0)
        got = dict(state=st.copy(), ep_len=ep.copy(), prop=obs[:, -REF.PROP_DIM:], reward=rew, terminated=term, truncated=trunc, metrics=met)
        yield k, p, cls, pre, pre_ep, post, a, got


def _tail(tag, p, pre, pre_ep, post, a, k, extra=0):
    fld = REF.case_field(tag)
    return REF.tail(post, REF.book_of(pre, pre_ep), REF.processed_action(p, a), p, REF.case_map(tag), SEED, k, np.arange(pre.shape[1]),
                    None if fld is None else REF.field_of(fld), extra)


def _add(total, ev):
    for key, c in ev.items():
        total[key] = total.get(key, 0) + c


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_reference_agrees_with_the_oracle_on_the_gpu_tests_inputs(tag, oracle_takes_non_finite_cars):
    """flags, reward, sums, lengths, stored rows, metrics and the eight values against oracle/visual_step.step; every staged event
    occurs; nobody is excused"""
    worst, total = 0.0, {}
    for k, p, cls, pre, pre_ep, post, a, got in oracle_steps(tag, oracle_takes_non_finite_cars):
        t = _tail(tag, p, pre, pre_ep, post, a, k, REF.ORACLE_EXTRA)
        log = bool(p.log_episode_sums)
        if not log:      # the oracle clears the sum rows at a reset and flushes them whatever the switch says: the kernels' rule is the reference's
            got["metrics"] = None
        fails, excused, w, _ = REF.check_step(got, t, p, extra=REF.ORACLE_EXTRA, floor_ulps=2, where=f"{tag} step {k}: ", epsum_rows=log)
        assert not fails, fails
        assert excused == 0
        worst = max(worst, w)
        _add(total, REF.events_of(tag, t, cls, post, a))
        if tag == "A":
            assert total["spawned on a white cell"] == total["resets"]
    print(f"case {tag}: worst ratio {worst:.3f}, 0 excused; " + ", ".join(f"{key} {c}" for key, c in total.items()))
    assert all(c >= MIN_EVENTS for c in total.values()), total
    assert total["resets"] > N // 2


def _golden_rows(pos, vb):
    n = pos.shape[0]
    post = np.zeros((S_COUNT, n), F)
    post[PX:PX + 3], post[QW], post[VX:VX + 3] = pos.T, 1, vb.T            # the identity rotation: R^T v is v itself, exactly
    return post


def _golden_tail(m, pos, vb):
    p = VS.visual_params()
    p.max_episode_length = 10 ** 9
    n = pos.shape[0]
    book = dict(ep_len=np.zeros(n, np.int32), epsum=np.zeros((2, n), F))
    return REF.tail(_golden_rows(pos, vb), book, np.zeros((2, n), F), p, m, 1, 0, np.arange(n))


def test_terms_and_flags_match_the_reference_projects_goldens(golden):
    g = golden("visual_mdp")
    t = _golden_tail(REF.case_map("A"), g["pos"], g["lin_vel_b"])
    assert t["finite"].all()
    np.testing.assert_array_equal(t["terms"][0].astype(F), g["traversable_reward"])
    np.testing.assert_array_equal(t["terms"][1].astype(F), g["forward_vel"])
    np.testing.assert_array_equal(t["oom"], g["out_of_map"])
    np.testing.assert_array_equal(t["terminated"], g["out_of_map"])
    want = (g["traversable_reward"].astype(np.float64) * 5.0 + g["forward_vel"].astype(np.float64) * 7.0) * float(F(0.02) * F(10))
    assert (np.abs(t["reward"] - want) <= 1e-12 * (1 + np.abs(want))).all()
    assert (t["terms"][0] > 0).sum() >= 4 and (t["terms"][0] < 0).sum() >= 4 and t["oom"].sum() >= 4


def test_terms_and_flags_match_the_reference_projects_edge_goldens(edge_golden):  # noqa: F811
    """the square geometries of the edge sets: cell lines, the map's edges +- ulps, the far field.  Points the goldens' own excusal
    predicates mark (tests/parity_predicates.py: a half extent that differs between the fp32 and the float64 spacing, quotients
    beyond the integer range) and non-finite points (a non-finite car has no terms here) are left out"""
    tr, md = edge_golden("visual_trav_edges"), edge_golden("visual_mdp_edges")
    full = edge_golden.task_map()
    checked = 0
    for gi, (rows, cols, rs, cs) in enumerate(tr["geoms"]):
        rows, cols, pre = int(rows), int(cols), f"g{gi}_"
        if rows != cols:
            continue
        trav = full if gi == 0 else np.unpackbits(tr[pre + "map_packed"])[: rows * cols].reshape(rows, cols).astype(bool)
        m = REF.travmap(trav, (rs, cs))
        pos, vb = md[pre + "pos"], md[pre + "lin_vel_b"]
        fin = np.isfinite(pos).all(1) & np.isfinite(vb).all(1)
        with np.errstate(all="ignore"):
            ex_id = PRED.map_index_excused(pos[:, 0], rows, rs) | PRED.map_index_excused(pos[:, 1], cols, cs) | (np.abs(pos[:, :2]).max(1) >= 2.0 ** 30)
            ex_oom = PRED.out_of_map_excused(pos[:, 0], rows, rs) | PRED.out_of_map_excused(pos[:, 1], cols, cs)
        safe = np.where((fin & ~ex_id)[:, None], pos, 0).astype(F)
        t = _golden_tail(m, safe, np.where(fin[:, None], vb, 0).astype(F))
        ok = fin & ~ex_id
        np.testing.assert_array_equal(t["terms"][0][ok].astype(F), md[pre + "traversable_reward"][ok], err_msg=pre)
        np.testing.assert_array_equal(t["terms"][1][fin].astype(F), md[pre + "forward_vel"][fin], err_msg=pre)
        t2 = _golden_tail(m, np.where(fin[:, None], pos, 0).astype(F), np.where(fin[:, None], vb, 0).astype(F))
        ok = fin & ~ex_oom
        np.testing.assert_array_equal(t2["oom"][ok], md[pre + "out_of_map"][ok], err_msg=pre)
        assert ok.sum() > ok.size // 2 and (fin & ~ex_id).sum() > ok.size // 2
        xy = tr[pre + "xy"]
        with np.errstate(all="ignore"):
            okx = np.isfinite(xy).all(1) & ~(PRED.map_index_excused(xy[:, 0], rows, rs) | PRED.map_index_excused(xy[:, 1], cols, cs)) & \
                (np.abs(xy).max(1) < 2.0 ** 30)
        xi, yi = REF.map_id(m, xy[okx, 0], xy[okx, 1])
        np.testing.assert_array_equal(xi, tr[pre + "x_idx"][okx], err_msg=pre)
        np.testing.assert_array_equal(yi, tr[pre + "y_idx"][okx], err_msg=pre)
        np.testing.assert_array_equal(m.trav[yi, xi], tr[pre + "trav"][okx], err_msg=pre)
        checked += 1
    assert checked >= 3


# ---- the kernel's wiring restated in fp32 numpy, and broken one defect at a time --------------------------------------------------
def _mat32(q):
    w, x, y, z = q
    x2, y2, z2 = x + x, y + y, z + z
    wx, wy, wz = w * x2, w * y2, w * z2
    dz, dy = F(1) - z * z2, F(1) - y * y2
    return np.array([[-y * y2 + dz, x * y2 - wz, x * z2 + wy], [x * y2 + wz, -x * x2 + dz, y * z2 - wx], [x * z2 - wy, y * z2 + wx, -x * x2 + dy]], F)


def _mul_t(R, v, order):
    idx = (2, 1, 0) if order == 0 else (0, 1, 2)
    out = []
    for i in range(3):
        acc = (R[idx[0], i] * v[idx[0]]).astype(F)
        for j in idx[1:]:
            acc = (R[j, i].astype(np.float64) * v[j] + acc).astype(F) if order == 0 else (acc + (R[j, i] * v[j]).astype(F)).astype(F)
        out.append(acc)
    return np.stack(out)


DEFECTS = ["a transposed map lookup", "row and column spacing swapped", ">= in out_of_map", "a time-out one step late",
           "a non-finite car counted under TERM0", "a non-finite car's reward not zeroed", "a zero weight multiplying a non-finite term",
           "step_dt dropped", "sums not cleared at reset", "sums flushed before the step's contribution",
           "EPLEN taking the pre-increment length", "last action kept through a reset", "a finite car's wheels zeroed at reset",
           "a non-finite car's wheels kept", "the spawn without the terrain lift", "the yaw and the cell drawn from each other's uniform"]


def emulate(t, post, pre, pre_ep, a_proc, p, m, field, step, defect=None, order=0):
    """the stored rows, outputs and metrics of one step as the kernel wires them, in fp32 numpy, every decision its own (only the
    non-finite rule and the Philox draw come from the reference)"""
    n = post.shape[1]
    fin = t["finite"]
    dt = F(t["dt"])
    with np.errstate(all="ignore"):
        postf = np.where(fin[None], post[:ACT0], F(0)).astype(F)
        postf[QW] = np.where(fin, postf[QW], F(1))
        vb = np.where(fin[None], _mul_t(_mat32(postf[QW:QW + 4]), postf[VX:VX + 3], order), _mul_t(_mat32(post[QW:QW + 4]), post[VX:VX + 3], order))
    mm = REF.travmap(m.trav, (m.cs, m.rs)) if defect == "row and column spacing swapped" else m
    ep_new = pre_ep.astype(np.int64) + 1
    trunc = (pre_ep if defect == "a time-out one step late" else ep_new) >= int(p.max_episode_length)
    x, y = postf[PX], postf[PX + 1]
    if defect == ">= in out_of_map":
        hw, hh = REF.half_extent(mm)
        oom = (x >= hw) | (x <= -hw) | (y >= hh) | (y <= -hh)
    else:
        oom = REF.out_of_map(mm, x, y)
    oom = oom & fin
    xi, yi = REF.map_id(mm, x, y)
    trav = m.trav[xi, yi] if defect == "a transposed map lookup" else m.trav[yi, xi]
    T = np.stack([np.where(fin, np.where(trav, F(1), F(-1)), F(0)), vb[0]]).astype(F)
    term = ~fin | oom
    done = term | trunc
    log = bool(p.log_episode_sums)
    eps_in = pre[EPSUM0:EPSUM0 + 2].astype(F) if log else np.zeros((2, n), F)
    reward, eps = np.zeros(n, F), np.zeros((2, n), F)
    with np.errstate(all="ignore"):
        for i in range(2):
            w = F(p.weight[i])
            guard = (w != 0) & fin
            if defect == "a non-finite car's reward not zeroed":
                guard = np.full(n, w != 0)
            elif defect == "a zero weight multiplying a non-finite term":
                guard = ~((w != 0) & ~fin)
            c = np.where(guard, (T[i] * w).astype(F) * (F(1) if defect == "step_dt dropped" else dt), F(0)).astype(F)
            reward = (reward + c).astype(F)
            eps[i] = (eps_in[i] + c).astype(F) if log else F(0)
    met = np.zeros(16)
    flushed = eps_in if defect == "sums flushed before the step's contribution" else eps
    met[:2] = flushed[:, done].astype(np.float64).sum(1)
    met[8], met[9], met[10], met[14] = done.sum(), (trunc & done).sum(), (oom & done).sum(), (~fin).sum()
    if defect == "a non-finite car counted under TERM0":
        met[10], met[14] = met[10] + (~fin).sum(), 0
    met[15] = (pre_ep if defect == "EPLEN taking the pre-increment length" else ep_new)[done].sum()
    rd = REF.reset_draw(p, mm, SEED, step, np.arange(n), field, swap_uniforms=defect == "the yaw and the cell drawn from each other's uniform",
                        lift=defect != "the spawn without the terrain lift")
    st = np.zeros((S_COUNT, n), F)
    st[:ACT0] = postf
    d = done[None]
    st[PX:PX + 3], st[QW:QW + 4] = np.where(d, rd["pos"], postf[PX:PX + 3]), np.where(d, rd["q"], postf[QW:QW + 4])
    st[VX:VX + 3], st[WX:WX + 3] = np.where(d, F(0), postf[VX:VX + 3]), np.where(d, F(0), postf[WX:WX + 3])
    rows = list(range(WHEEL, WHEEL + 4)) + [STEER_POS, STEER_VEL]
    raw = post[rows].astype(F)
    if defect == "a non-finite car's wheels kept":
        st[rows] = raw
    elif defect == "a finite car's wheels zeroed at reset":
        st[rows] = np.where(d, F(0), raw)
    else:
        st[rows] = np.where((done & ~fin)[None], F(0), raw)
    act = np.asarray(a_proc, F).copy() if defect == "last action kept through a reset" else np.where(d, F(0), np.asarray(a_proc, F)).astype(F)
    st[ACT0:ACT0 + 2] = act
    if log:
        st[EPSUM0:EPSUM0 + 2] = eps if defect == "sums not cleared at reset" else np.where(d, F(0), eps)
    else:
        st[EPSUM0:EPSUM0 + 2] = pre[EPSUM0:EPSUM0 + 2]
    with np.errstate(all="ignore"):
        Ro = _mat32(st[QW:QW + 4])
        prop = np.concatenate([_mul_t(Ro, st[VX:VX + 3], order), _mul_t(Ro, st[WX:WX + 3], order), np.clip(act, -1, 1)]).T.astype(F)
    return dict(state=st, ep_len=np.where(done, 0, ep_new), prop=prop, reward=reward, terminated=term, truncated=trunc, dones=done, metrics=met)


def _defect_inputs(safe_ground):
    """every step of the three cases; on cases A and B eight finite cars are moved EXACTLY onto a border after the physics (what a
    `>=` in out_of_map decides otherwise: no physics lands a car there on purpose)"""
    out = []
    for tag in ("A", "B", "C"):
        m, fld = REF.case_map(tag), REF.case_field(tag)
        field = None if fld is None else REF.field_of(fld)
        hw, hh = REF.half_extent(m)
        for k, p, cls, pre, pre_ep, post, a, _ in oracle_steps(tag, safe_ground):
            post = post.copy()
            if tag != "C":
                on = [e for e in range(8, N, 9) if np.isfinite(post[:ACT0, e]).all() and cls[e] == -1][:8]
                for i, e in enumerate(on):
                    post[PX + i % 2, e] = (hw, hh)[i % 2] * (1 if i < 4 else -1)
            a_proc = REF.processed_action(p, a)
            t = REF.tail(post, REF.book_of(pre, pre_ep), a_proc, p, m, SEED, k, np.arange(N), field)
            out.append((tag, k, p, m, field, t, post, pre, pre_ep, a_proc))
    return out


def test_bound_accepts_the_correct_wiring_and_rejects_sixteen_defects(oracle_takes_non_finite_cars):
    cases = _defect_inputs(oracle_takes_non_finite_cars)
    assert len(DEFECTS) == 16
    for order in range(2):
        for tag, k, p, m, field, t, post, pre, pre_ep, a_proc in cases:
            fails, excused, w, _ = REF.check_step(emulate(t, post, pre, pre_ep, a_proc, p, m, field, k, None, order), t, p, where=f"{tag} step {k}: ")
            assert not fails and excused == 0 and w <= 1.0, (order, fails)
    for defect in DEFECTS:
        caught = {}
        for tag, k, p, m, field, t, post, pre, pre_ep, a_proc in cases:
            fails, _, _, _ = REF.check_step(emulate(t, post, pre, pre_ep, a_proc, p, m, field, k, defect), t, p)
            caught[tag] = caught.get(tag, 0) + bool(fails)
        print(f"{defect}: rejected on {caught} of {K} steps per case")
        assert sum(caught.values()) >= 1, defect

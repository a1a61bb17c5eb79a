"""tests/elev_tail_reference.py (the elevation step's tail in float64) held to the numpy oracle (oracle/elev_step.py, and with
terrain levels tests/terrain_levels_reference.py) on the inputs of tests/test_gpu_elev_tail.py, to the reference project's golden
terms and flags, its bound shown to accept the correct wiring (in fp32, two summation orders) and to reject fourteen modelled wiring
defects, and the share of envs `near_threshold` excuses on those inputs held under 1 % per step."""
import numpy as np
import pytest

import elev_tail_reference as REF
import terrain_levels_reference as TLR
from oracle import elev_step as OS
from oracle import env_step as ES
from oracle import heightfield as OH
from oracle.layout import ACT0, CMD_BX, CMD_BY, CMD_TIMER, EPSUM0, PX, QW, S_COUNT, STEER_POS, STEER_VEL, TGT_H, TGT_X, TGT_Y, VX, WHEEL, WX
from tests import parity_predicates as PRED
from tests.parity_predicates import edge_golden  # noqa: F401  (fixture)

F = np.float32
SEED = 5
CAP = 0.01
N, K = REF.N_ENVS, REF.K_STEPS


def case_field(tag):
    """-> the oracle's field tuple (decoded fp32 heights, x0, y0, cell, outside_z) of a case; B: the generator's float64 reference
    codes (the device's differ from them by one code at well under 1 % of the points: tests/terrain_gen_reference.py)"""
    if tag == "A":
        return OH.make_terrain() + (0.0,)
    if tag == "C":
        import heightfield_cases
        return heightfield_cases.get("G1").oracle()
    import terrain_gen_reference as TG
    from wheeledlab_amd.envs import terrain_gen_cfg as G
    cfg = REF.tile_cfg()
    geo = G.lattice(cfg)
    codes = np.rint(TG.reference(TG.params_dict(cfg), G.tile_table(cfg)).t).astype(np.int16)
    return (codes.astype(F) * F(geo["z_scale"]), F(geo["x0"]), F(geo["y0"]), F(geo["cell"]), 0.0)


def case_levels(tag, n):
    """the level tables of a case as the references take them (None: off); C runs the oracle's levels path on ONE tile at the origin,
    which is the plain step (tests/test_terrain_levels_cpu.py) with a ground sampler that takes non-finite cars"""
    if tag == "A":
        return None
    if tag == "C":
        return dict(level=np.zeros(n, np.int32), type=np.zeros(n, np.int32), origins=np.zeros((1, 2), F), rows=1, cols=1)
    from wheeledlab_amd.envs import terrain_levels as TL
    cfg = REF.tile_cfg()
    level, types = TL.initial_assignment(cfg, n, seed=SEED)
    return dict(level=level.copy(), type=types, origins=TL.tile_origins(cfg), rows=REF.TILE_ROWS, cols=REF.TILE_COLS)


def _oracle_params(tag, k):
    return REF.apply_case(OS.elev_params(), tag, k)


def oracle_steps(tag, n=N, steps=K, seed=SEED):
    """the case's steps on the oracle: yields (k, p, pre rows, pre ep_len, pre levels, post-physics rows, actions, oracle outputs)"""
    hf = case_field(tag)
    levels = case_levels(tag, n)
    p = _oracle_params(tag, 0)
    st = OS.init_state(p, n, seed, stride=n)
    ep = np.zeros(n, np.int32)
    if levels is None:
        OS.reset_envs(p, st, ep, hf, np.arange(n), seed, 0)
    else:
        TLR.reset_envs(p, st, ep, hf, np.arange(n), seed, 0, levels)
    OS.update_command(st)
    for k in range(steps):
        p = _oracle_params(tag, k)
        REF.stage_step(tag, k, st, ep, n, None if levels is None else levels["level"])
        a = REF.case_actions(tag, k, n)
        pre, pre_ep = st.copy(), ep.copy()
        pre_lv = None if levels is None else dict(levels, level=levels["level"].copy())
        post = st.copy()
        with np.errstate(all="ignore"):
            steer_t, wheel_t = ES.fwd_targets(p, ES.apply_action(p, post, a))
            ES.integrate(p, post, steer_t, wheel_t, TLR.ground_fn(hf))
            met = np.zeros(16)
            obs, rew, term, trunc, _ = TLR.step(p, st, ep, hf, a, seed, k, levels, met)
        got = dict(state=st.copy(), ep_len=ep.copy(), obs=obs, reward=rew, terminated=term, truncated=trunc, metrics=met,
                   level=None if levels is None else levels["level"].copy())
        yield k, p, hf, pre, pre_ep, pre_lv, post, a, got


def _tail(tag, p, hf, pre, pre_ep, pre_lv, post, a, k, extra=0):
    lv = pre_lv if tag == "B" else None
    return REF.tail(post, REF.book_of(pre, pre_ep), REF.processed_action(p, a), p, SEED, k, np.arange(pre.shape[1]), REF.field_of(hf), lv, extra)


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_reference_agrees_with_the_oracle_and_excuses_under_one_percent(tag):
    """tail, command and observation against the oracle's step on the GPU test's inputs; the excusal cap of those inputs; the
    level move against tests/terrain_levels_reference.py (case B)"""
    worst, ev, moved = 0.0, np.zeros(8, int), 0
    for k, p, hf, pre, pre_ep, pre_lv, post, a, got in oracle_steps(tag):
        t = _tail(tag, p, hf, pre, pre_ep, pre_lv, post, a, k, REF.ORACLE_EXTRA)
        if tag == "C":
            got["metrics"] = None           # the oracle counts a non-finite car's comparisons among M_TERM*: the kernels' rule is the reference's
            got["level"] = None
        fails, excused, w, _ = REF.check_step(got, t, p, extra=REF.ORACLE_EXTRA, floor_ulps=2, where=f"{tag} step {k}: ")
        assert not fails, fails
        assert excused < CAP * N, (tag, k, excused, {key: int(t[key].sum()) for key in REF.NEAR_KEYS})
        worst = max(worst, w)
        ev += [t["done"].sum(), *t["flags"].sum(1), t["truncated"].sum(), (t["done"] & t["expired"]).sum(), t["expired"].sum()]
        if tag == "B":
            moved += int((t["level"] != pre_lv["level"]).sum())
    print(f"case {tag}: worst ratio {worst:.3f}; resets {ev[0]}, low / stuck / rolled / at goal {ev[1:5].tolist()}, timed out {ev[5]}, "
          f"resampled {ev[7]} ({ev[6]} in the step of a reset)")
    assert ev[0] > N // 2 and ev[5] >= N // 4                                  # the cases do what they are for
    assert (ev[1:5] >= 10).all(), ev[1:5]
    assert ev[7] >= 20
    if tag == "B":
        assert ev[6] > N // 4 and moved > N // 4


def test_level_rule_is_the_levels_reference():
    """every outcome x every row of a 3-row table, the wrap draw included"""
    n = 36
    e = np.arange(n)
    level = (e % 3).astype(np.int32)
    at_goal, failed = (e // 3) % 2 == 1, (e // 6) % 2 == 1
    levels = dict(level=level, type=np.zeros(n, np.int32), origins=np.zeros((3, 2), F), rows=3, cols=1)
    want = TLR.next_levels(levels, e, at_goal, failed, 9, 4)
    up, down, stay = at_goal, failed & ~at_goal, ~failed & ~at_goal
    assert (want[stay] == level[stay]).all() and (want[down] == np.maximum(level[down] - 1, 0)).all()
    assert (want[up & (level < 2)] == level[up & (level < 2)] + 1).all()
    draw = TLR.uniform_below(REF.PH.philox4x32(e, 4, TLR.S_LEVEL, 9)[0], 3)
    assert (want[up & (level == 2)] == draw[up & (level == 2)]).all()
    # the tail takes the same rule: flags[3] is "at goal", terminated is "failed"
    p = REF.apply_case(OS.elev_params(), "B")
    hf = REF.field_of(OH.make_terrain())
    post = np.zeros((S_COUNT, n), F)
    post[QW], post[PX + 2] = 1, 0.3
    book = dict(ep_len=np.zeros(n, np.int32), cb=np.where(at_goal, F(0.1), F(9.0))[None].repeat(2, 0).astype(F), epsum=np.zeros((4, n), F),
                tgt=np.zeros((3, n), F), timer=np.ones(n, F))
    post[QW:QW + 4, failed] = np.array([0.70710678, 0.70710678, 0, 0], F)[:, None]        # on its side
    t = REF.tail(post, book, np.zeros((2, n), F), p, 9, 4, e, hf, levels)
    np.testing.assert_array_equal(t["flags"][3], at_goal)
    np.testing.assert_array_equal(t["level"], want)


def _golden_terms(g, timed_out):
    n = g["pos"].shape[0]
    p = OS.elev_params()
    q = g["quat"].T
    return REF.elev_terms(p, REF.f64(g["pos"].T), REF.f64(q), REF.f64(g["lin_vel_w"].T), REF.f64(g["joint_vel"][:, 2:6].T), g["command"][:, :2].T,
                          timed_out if timed_out is not None else np.zeros(n, bool), vb=g["lin_vel_b"].T), p


def _check_golden(g, tm, timed_out):
    near = tm["near_stuck"] | tm["near_goal"] | tm["near_elev"] | tm["near_fall"]
    ok = ~near
    assert ok.sum() > ok.size // 2
    fl, T, B = tm["flags"], tm["T"], tm["B"]
    np.testing.assert_array_equal(fl[0], g["below_min_height"] if "below_min_height" in g else g["pos"][:, 2] < F(0.15))
    np.testing.assert_array_equal(fl[1][ok], g["stuck"][ok])
    np.testing.assert_array_equal(fl[3][ok], g["close_to_goal"][ok])
    if "upright_r33" in g:
        ex = PRED.rollover_norm_excused(g["quat"], g["upright_r33"]) | tm["near_roll"]
    else:
        ex = (np.abs(g["upright_penalty"]) <= 1e-2) & (g["upright_penalty"] != 0) | tm["near_roll"]
    np.testing.assert_array_equal(fl[2][~ex], g["upright_bool"][~ex])
    with np.errstate(invalid="ignore"):
        want = g["goal_progress_rate"].astype(np.float64)
        fin = np.isfinite(want) & np.isfinite(T[0]) & ok
        err = np.abs(T[0] - want)
        bound = 2 * B[0] + REF.ORACLE_EXTRA * REF.U * (5 + np.abs(T[0] - 5)) + REF.ulp(np.nan_to_num(want))    # two fp32 sides, torch's own roundings
        assert (err[fin] <= bound[fin]).all(), float((err[fin] / bound[fin]).max())
        assert (np.isnan(want) == np.isnan(T[0]))[ok].all()
    np.testing.assert_array_equal(T[1][ok].astype(F), g["higher_elevation"][ok])        # pos.z - 0.19 rounded once: the golden's own value
    np.testing.assert_array_equal(T[2][ok] > 0.5, g["is_falling_penalty"][ok])
    pen = g["stuck"] & ~timed_out if timed_out is not None else g["stuck"]
    np.testing.assert_array_equal(T[3][ok] > 0.5, pen[ok])


def test_terms_and_flags_match_the_reference_projects_goldens(golden):
    g = golden("elevation_mdp")
    tm, _ = _golden_terms(g, None)
    _check_golden(g, tm, None)
    assert tm["flags"][3].sum() >= 4 and tm["flags"][1].sum() >= 1 and tm["flags"][2].sum() >= 10


def test_terms_and_flags_match_the_reference_projects_edge_goldens(edge_golden):  # noqa: F811
    g = edge_golden("elevation_mdp_edges")
    for to in (None, g["timed_out"]):
        tm, _ = _golden_terms(g, to)
        _check_golden(g, tm, to)


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


def _yaw_cs32(q):
    w, x, y, z = q
    a = (F(1) - F(2) * (z * z + y * y)).astype(F)
    b = (F(2) * (w * z + x * y)).astype(F)
    inv = (F(1) / np.sqrt(a * a + b * b)).astype(F)
    return a * inv, b * inv


DEFECTS = ["this step's command used by the rewards", "episode sums not cleared on reset", "timer counted down before the reset re-arms it",
           "command frame from the pre-reset yaw", "command frame from the pre-reset position", "resampled target not offset by the tile origin",
           "a resetting env's resample on its old tile", "stuck penalty not gated by the time-out", "falling read from the world vz",
           "M_TERM counted for a non-finite car", "last action not zeroed on reset", "the 13 values from the pre-reset state",
           "nan_to_num missing on the goal", "a reward contribution with dt applied twice"]


def emulate(t, post, pre, pre_ep, pre_lv, a_proc, p, defect=None, order=0):
    """the stored rows, outputs and metrics of one step as the kernel wires them, in fp32, from the reference's decisions and draws"""
    n = post.shape[1]
    f = lambda x: np.asarray(x, F)                                           # noqa: E731
    done, fin, rd = t["done"], t["finite"], t["reset"]
    dt = F(t["dt"])
    postf = np.where(fin[None], post[:ACT0], F(0)).astype(F)
    postf[QW] = np.where(fin, postf[QW], F(1))
    pos, q, v, ww, wheel = postf[PX:PX + 3], postf[QW:QW + 4], postf[VX:VX + 3], postf[WX:WX + 3], postf[WHEEL:WHEEL + 4]
    R = _mat32(q)
    vb = _mul_t(R, v, order)
    # ---- the stored rows ----
    st = np.zeros((S_COUNT, n), F)
    dyn = f(np.nan_to_num(t["dyn"]))
    st[:ACT0] = np.where(done[None], dyn, postf)
    bad = (done & ~fin)[None]
    st[WHEEL:WHEEL + 4] = np.where(bad, F(0), st[WHEEL:WHEEL + 4])
    st[STEER_POS:STEER_VEL + 1] = np.where(bad, F(0), st[STEER_POS:STEER_VEL + 1])
    act = f(a_proc).copy() if defect == "last action not zeroed on reset" else f(t["last_action"])
    st[ACT0:ACT0 + 2] = act
    # command manager
    rs = F(p.cmd_resample_s)
    tgt = np.where(done[None], f(rd["tgt"]), pre[TGT_X:TGT_H + 1]).astype(F)
    if defect == "timer counted down before the reset re-arms it":
        dec = (pre[CMD_TIMER] - dt).astype(F)
        expired = (dec <= 0) & ~done
        timer = np.where(done | expired, rs, dec).astype(F)
    else:
        dec = (np.where(done, rs, pre[CMD_TIMER]).astype(F) - dt).astype(F)
        expired = dec <= 0
        timer = np.where(expired, rs, dec).astype(F)
    u = REF.PH.uniform4(np.arange(n), t["step"], REF.ES_CMD_RESAMPLE, t["seed"])
    new = np.stack([ES.sym(u[0], p.cmd_xy), ES.sym(u[1], p.cmd_xy), ES.sym(u[2], p.cmd_heading)]).astype(F)
    if pre_lv is not None and defect != "resampled target not offset by the tile origin":
        lv = pre_lv["level"] if defect == "a resetting env's resample on its old tile" else t["level"]
        o = REF.origins(pre_lv, lv)
        new[0], new[1] = (o[0] + new[0]).astype(F), (o[1] + new[1]).astype(F)
    tgt = np.where(expired[None], new, tgt).astype(F)
    st[TGT_X:TGT_H + 1], st[CMD_TIMER] = tgt, timer
    q_cmd = postf[QW:QW + 4] if defect == "command frame from the pre-reset yaw" else st[QW:QW + 4]
    p_cmd = postf[PX:PX + 2] if defect == "command frame from the pre-reset position" else st[PX:PX + 2]
    c, s = _yaw_cs32(q_cmd)
    with np.errstate(all="ignore"):
        dx, dy = tgt[0] - p_cmd[0], tgt[1] - p_cmd[1]
        st[CMD_BX], st[CMD_BY] = c * dx + s * dy, -s * dx + c * dy
        # ---- terms, reward, sums ----
        cb = st[CMD_BX:CMD_BX + 2] if defect == "this step's command used by the rewards" else pre[CMD_BX:CMD_BX + 2]
        gx, gy = cb[0] - pos[0], cb[1] - pos[1]
        T = f(t["terms"]).copy()
        T[0] = F(p.progress_offset) + (v[0] * gx + v[1] * gy) / np.sqrt(gx * gx + gy * gy)
        z = pos[2] - F(p.elev_z0)
        T[1] = np.clip(np.where((z > F(p.elev_min)) & (vb[0] > F(p.elev_min_vel)), z, F(0)), F(0), F(1))
        T[2] = ((v[2] if defect == "falling read from the world vz" else vb[2]) > F(p.fall_vel)).astype(F)
        T[3] = (t["flags"][1] if defect == "stuck penalty not gated by the time-out" else t["flags"][1] & ~t["truncated"]).astype(F)
        T = np.where(fin[None], T, F(0)).astype(F)
        w = np.array([F(p.weight[i]) for i in range(4)])
        cdt = dt * dt if defect == "a reward contribution with dt applied twice" else dt
        cdt = np.array([dt, cdt, dt, dt], F)                                # the defect on ONE term's contribution
        contrib = np.where((w != 0)[:, None] & fin[None], (T * w[:, None]).astype(F) * cdt[:, None], F(0)).astype(F)
        reward = np.zeros(n, F)
        for i in range(4):
            reward = (reward + contrib[i]).astype(F)
        eps = (pre[EPSUM0:EPSUM0 + 4] * F(bool(p.log_episode_sums)) + contrib).astype(F) * F(bool(p.log_episode_sums))
    met = np.zeros(16)
    met[:4] = eps[:, done].astype(np.float64).sum(1)
    met[8], met[9], met[14], met[15] = done.sum(), t["truncated"].sum(), (~fin).sum(), t["ep_len_end"][done].sum()
    raw = REF.elev_terms(p, REF.f64(post[PX:PX + 3]), REF.f64(post[QW:QW + 4]), REF.f64(post[VX:VX + 3]), REF.f64(post[WHEEL:WHEEL + 4]),
                         REF.f64(pre[CMD_BX:CMD_BX + 2]), t["truncated"])["flags"] if defect == "M_TERM counted for a non-finite car" else t["flags"]
    if defect == "M_TERM counted for a non-finite car":
        raw = raw | ~fin[None] & np.array([True, False, False, False])[:, None]       # -inf < min_height: the unguarded comparison counts
    met[10:14] = (raw & done[None]).sum(1)
    st[EPSUM0:EPSUM0 + 4] = eps if defect == "episode sums not cleared on reset" else np.where(done[None], F(0), eps)
    # ---- observation ----
    src = np.where(done[None], np.concatenate([postf, st[ACT0:]]), st) if defect == "the 13 values from the pre-reset state" else st
    src = src.astype(F)
    qo = src[QW:QW + 4]
    Ro = _mat32(qo)
    with np.errstate(all="ignore"):
        g = np.stack([st[CMD_BX] - src[PX], st[CMD_BY] - src[PX + 1]]).astype(F)
        if defect != "nan_to_num missing on the goal":
            g = np.nan_to_num(g, nan=0.0).astype(F)
    e = np.stack([np.arctan2(F(2) * (qo[0] * qo[1] + qo[2] * qo[3]), F(1) - F(2) * (qo[1] * qo[1] + qo[2] * qo[2])),
                  np.arcsin(np.clip(F(2) * (qo[0] * qo[2] - qo[3] * qo[1]), -1, 1)),
                  np.arctan2(F(2) * (qo[0] * qo[3] + qo[1] * qo[2]), F(1) - F(2) * (qo[2] * qo[2] + qo[3] * qo[3]))]).astype(F)
    e = np.where(e < 0, e + F(REF.TWO_PI), e).astype(F)
    cl = F(p.obs_clip)
    obs = np.concatenate([g, e, np.clip(_mul_t(Ro, src[VX:VX + 3], order), -cl, cl), np.clip(_mul_t(Ro, src[WX:WX + 3], order), -cl, cl),
                          np.clip(act, -1, 1)]).T.astype(F)
    return dict(state=st, ep_len=t["ep_len"], obs=obs, reward=reward, terminated=t["terminated"], truncated=t["truncated"], metrics=met,
                level=t["level"])


def _defect_inputs():
    """case B's tiles and resamples in the step of a reset with case C's bookkeeping, non-finite cars and commands"""
    out = []
    for k, p, hf, pre, pre_ep, pre_lv, post, a, got in oracle_steps("B", steps=4):
        p.weight[0], p.weight[1], p.weight[2], p.weight[3], p.obs_clip = -30.0, 700.0, 3.0, 11.0, 1.0
        if k == 1:
            p.cmd_resample_s = 0.05          # below the step's dt: everybody resamples, resetting envs too
        pre, post = pre.copy(), post.copy()
        n = pre.shape[1]
        pre[EPSUM0:EPSUM0 + 4] = (0.01 * (1 + np.arange(4))[:, None] * (1 + np.arange(n))[None]).astype(F)
        post[VX, REF.NAN_ENV], post[PX + 2, REF.INF_ENV] = np.nan, -np.inf
        pre[TGT_X, 14], pre[TGT_Y, 21] = np.nan, np.nan
        pre[CMD_TIMER, 14], pre[CMD_TIMER, 21] = 5.0, 5.0
        a_proc = REF.processed_action(p, a)
        t = REF.tail(post, REF.book_of(pre, pre_ep), a_proc, p, SEED, k, np.arange(n), REF.field_of(hf), pre_lv)
        t["seed"], t["step"] = SEED, k
        out.append((p, t, post, pre, pre_ep, pre_lv, a_proc))
    return out


def test_bound_accepts_the_correct_wiring_and_rejects_fourteen_defects():
    cases = _defect_inputs()
    for order in range(2):
        for p, t, post, pre, pre_ep, pre_lv, a_proc in cases:
            fails, _, w, _ = REF.check_step(emulate(t, post, pre, pre_ep, pre_lv, a_proc, p, None, order), t, p)
            assert not fails, (order, fails)
    for defect in DEFECTS:
        caught = 0
        for p, t, post, pre, pre_ep, pre_lv, a_proc in cases:
            fails, _, _, _ = REF.check_step(emulate(t, post, pre, pre_ep, pre_lv, a_proc, p, defect), t, p)
            caught += bool(fails)
        print(f"{defect}: rejected on {caught} of {len(cases)} steps")
        assert caught >= 1, defect

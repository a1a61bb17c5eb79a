"""tests/drift_tail_reference.py (the drift step's tail in float64) held to the numpy oracle and to the reference project's golden
reward terms, its bound shown to reject eight modelled wiring defects of the kernel's carried-along observation path and to accept
the correct form in four summation orders, the documented error of atan2_fast measured on the host build of wl_math.h, and the share
of envs `near_threshold` excuses on the inputs of tests/test_gpu_drift_tail.py held under 1 % per step."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import drift_tail_reference as REF
from oracle import drift_step as OS
from oracle import env_step as ES
from oracle import params as OP
from oracle.layout import ACT0, DRIFT_ROWS, EPSUM0, PX, QW, STEER_POS, TIMER_HF, TIMER_LF, VX, WX

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SEED = 5
CAP = 0.01


def _ref_table(seed):
    import torch
    from wheeledlab_amd.core import stadium_reference_poses
    t = np.zeros((3, 32), F)
    g = torch.Generator().manual_seed(seed)
    t[:, :20] = stadium_reference_poses(torch.rand(20, generator=g)).numpy()
    return t


def oracle_steps(tag, n=REF.N_ENVS, K=REF.K_STEPS, seed=SEED):
    """the case's K steps on the oracle: yields (k, p, pre rows, pre ep_len, post-physics rows, actions, noise, oracle outputs)"""
    p = REF.apply_case(OP.drift_params(), tag)
    ref = _ref_table(seed)
    st = OS.init_state(p, n, seed, stride=n)
    ep = np.zeros(st.shape[1], np.int32)
    OS.reset_envs(p, st, ep, ref, np.arange(n), seed, 0)
    REF.prepare_case(tag, st, ep, n, p)
    for k in range(K):
        a = REF.case_actions(k, n)
        noise = REF.case_noise(k, st.shape[1])[:, :n] if tag == "C" else None
        pre, pre_ep = st.copy(), ep.copy()
        post = st.copy()
        with np.errstate(all="ignore"):
            steer_t, wheel_t = OS.targets(p, ES.apply_action(p, post, a))
            ES.integrate(p, post, steer_t, wheel_t)
            met = np.zeros(16)
            obs, rew, term, trunc, _ = OS.step(p, st, ep, ref, a, seed, k, met, noise)
        got = dict(state=st[:, :n].copy(), ep_len=ep[:n].copy(), obs=obs, reward=rew, terminated=term, truncated=trunc, metrics=met)
        yield k, p, ref, pre[:, :n], pre_ep[:n], post[:, :n], a, noise, got


def _tail(p, ref, pre, pre_ep, post, a, k, seed=SEED):
    n = pre.shape[1]
    return REF.tail(post, pre_ep, pre[EPSUM0:EPSUM0 + 8], pre[ACT0:ACT0 + 2], a, p, seed, k, np.arange(n),
                    timers=(pre[TIMER_HF], pre[TIMER_LF]), ref_table=ref)


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_reference_agrees_with_the_oracle_and_excuses_under_one_percent(tag):
    """observation and tail against oracle/drift_step.py on the GPU test's inputs; the excusal cap of those inputs"""
    worst, events = 0.0, np.zeros(4, int)
    for k, p, ref, pre, pre_ep, post, a, noise, got in oracle_steps(tag):
        t = _tail(p, ref, pre, pre_ep, post, a, k)
        fails, excused, w = REF.check_step(got, t, post, p, noise, extra_roundings=REF.ORACLE_EXTRA, floor_ulps=2, where=f"{tag} step {k}: ")
        assert not fails, fails
        assert excused < CAP * pre.shape[1], (tag, k, excused)
        worst = max(worst, w)
        events += [t["done"].sum(), t["terminated"].sum(), t["hf_fire"].sum(), (t["done"] & t["lf_fire"]).sum()]
    print(f"case {tag}: worst ratio {worst:.3f}; resets {events[0]}, terminated {events[1]}, hf pushes {events[2]}, lf pushes on a reset step {events[3]}")
    assert events[0] > REF.N_ENVS // 2                                     # the cases do what they are for
    if tag == "A":
        assert events[1] >= 10
    if tag == "B":
        assert events[2] > 4 * REF.N_ENVS and events[3] > REF.N_ENVS // 2
    if tag == "C":
        assert events[1] >= 1


def test_reward_terms_match_the_reference_projects_goldens(golden):
    """the float64 terms against the reference project's own outputs (the goldens of test_oracle_golden_drift.py)"""
    for tag in ("n256", "edges"):
        g = golden(f"drift_mdp_{tag}")
        n = g["pos"].shape[0]
        p = OP.drift_params()
        p.weight[3] = 0.0
        # the goldens' body-frame inputs are drawn independently of their quaternion: with the identity rotation the tail's own
        # body-frame values ARE the golden inputs (v_b, w_b); the world yaw rate of track_progress_rate is run separately
        post = np.zeros((DRIFT_ROWS, n), F)
        post[PX:PX + 3], post[QW], post[VX:VX + 3], post[WX:WX + 3] = g["pos"].T, 1.0, g["lin_vel_b"].T, g["ang_vel_b"].T
        post[STEER_POS] = g["joint_pos"][:, 0]
        same_steer = g["joint_pos"][:, 0] == g["joint_pos"][:, 1]
        args = (np.zeros(n, np.int32), np.zeros((8, n), F), np.zeros((2, n), F), g["actions"], p, 1, 0, np.arange(n))
        kw = dict(timers=(np.ones(n, F), np.ones(n, F)), ref_table=_ref_table(1))
        t = REF.tail(post, *args, **kw)
        post_w = post.copy()
        post_w[WX:WX + 3] = g["ang_vel_w"].T
        fin = t["finite"]
        np.testing.assert_array_equal(REF.tail(post_w, *args, **kw)["terms"][2][fin], g["track_progress_rate"][fin])
        ok = ~REF.near_threshold(t) & fin
        assert ok.sum() > n // 2, (tag, int(ok.sum()))
        np.testing.assert_array_equal(t["terminated"][ok], g["cart_off_track"][ok])
        names = ["side_slip", "vel_dist", None, "turn_left_go_right", "energy_through_turn", "cross_track_dist"]
        for i, name in enumerate(names):
            if name is None:
                continue
            m = ok & (same_steer if name == "turn_left_go_right" else True)
            err = np.abs(t["terms"][i] - g[name])[m]
            bound = 2 * t["terms_b"][i] + REF.ulp(g[name])       # two fp32 sides (the golden one is torch) and the golden value's own rounding
            assert (err <= bound[m]).all(), (tag, name, float((err / np.maximum(bound[m], 1e-300)).max()))


# ---- the kernel's carried-along observation path, restated in fp32 numpy -------------------------------------------------------
def _dot3(a, b, order):
    """sum_j a_j b_j in fp32 in one of four orders: the kernel's fma chain (emulated in float64 -> one rounding per fma), its
    mirror, left to right with rounded products, pairwise"""
    if order < 2:
        idx = (2, 1, 0) if order == 0 else (0, 1, 2)
        acc = (a[idx[0]] * b[idx[0]]).astype(F)
        for j in idx[1:]:
            acc = (a[j].astype(np.float64) * b[j] + acc).astype(F)
        return acc
    pr = [(a[j] * b[j]).astype(F) for j in range(3)]
    return ((pr[0] + pr[1]).astype(F) + pr[2]).astype(F) if order == 2 else (pr[0] + (pr[1] + pr[2]).astype(F)).astype(F)


def _mat32(q):
    w, x, y, z = q
    x2, y2, z2 = x + x, y + y, z + z
    wx, wy, wz = w * x2, w * y2, w * z2
    dz, dy = F(1) - z * z2, F(1) - y * y2
    return np.array([[-y * y2 + dz, x * y2 - wz, x * z2 + wy], [x * y2 + wz, -x * x2 + dz, y * z2 - wx], [x * z2 - wy, y * z2 + wx, -x * x2 + dy]], F)


def emulate(t, post, pre, p, defect=None, order=0, quad=True):
    """the stored rows, observation and metrics of one step as the kernel wires them, from the reference's decisions and draws"""
    n = post.shape[1]
    f = lambda x: np.asarray(x, F)                                        # noqa: E731
    done, rd = t["done"], t["reset"]
    R = _mat32(f(post[QW:QW + 4]))
    vb = np.stack([_dot3(R[:, i], f(post[VX:VX + 3]), order) for i in range(3)])
    wb = np.stack([_dot3(R[:, i], f(post[WX:WX + 3]), order) for i in range(3)])
    st = f(post[:DRIFT_ROWS]).copy()
    qn = np.stack([np.cos(0.5 * rd["yaw"]), 0 * rd["yaw"], 0 * rd["yaw"], np.sin(0.5 * rd["yaw"])]).astype(F)
    st[PX:PX + 3] = np.where(done, f(rd["pos"]), st[PX:PX + 3])
    st[QW:QW + 4] = np.where(done, qn, st[QW:QW + 4])
    st[VX:VX + 6] = np.where(done, F(0), st[VX:VX + 6])
    vb, wb = np.where(done, F(0), vb), np.where(done, F(0), wb)
    cy, sy = qn[0] * qn[0] - qn[3] * qn[3], F(2) * qn[0] * qn[3]
    zero, one = np.zeros(n, F), np.ones(n, F)
    Ry = np.array([[cy, -sy, zero], [sy, cy, zero], [zero, zero, one]], F)
    Ro = R if defect == "push rotated by the pre-reset R" else np.where(done, Ry, R)
    dv = f(np.concatenate([t["dv"], np.zeros((1, n))]))
    st[VX:VX + 2] += dv[:2]
    Rp = Ro.transpose(1, 0, 2) if defect == "Ro transposed in the push increment" else Ro
    vb = np.stack([(_dot3(Rp[:, i], dv, order) + vb[i]).astype(F) for i in range(3)])
    for dw in (f(t["dw_hf"]), f(t["dw_lf"])):
        st[WX + 2] += dw
        if defect == "dwz added to wb_o.z":
            wb[2] = wb[2] + dw
        else:
            wb = (dw * Ro[2] + wb).astype(F)
    act = f(t["last_action"]).copy()
    if defect == "last action not zeroed on reset":
        a = f(pre["action"]).T
        act = np.clip(a, -1, 1) if p.action.clip_wrapper else a
    st[ACT0:ACT0 + 2] = act
    dt = F(t["dt"])
    st[TIMER_HF], st[TIMER_LF] = f(t["timer_hf"]), f(t["timer_lf"])
    if defect == "lf timer from lf_next on a reset step" and p.enable_pushes:
        lf_next = f(pre["timers"][1]) - dt
        st[TIMER_LF] = np.where(done & ~t["lf_fire"], lf_next, st[TIMER_LF])
    # bookkeeping
    w = np.array([F(p.weight[i]) for i in range(7)])
    T = f(t["terms"])
    c = np.where((w != 0)[:, None] & t["finite"], (T * w[:, None]).astype(F) * dt, F(0)).astype(F)
    ce = c.copy()
    if defect == "a w == 0 term still added to epsum":
        ce = np.where((w == 0)[:, None], T * dt, c).astype(F)
    reward = np.zeros(n, F)
    for i in range(7):
        reward = reward + c[i]
    eps = f(pre["epsum"][:7]) * F(bool(p.log_episode_sums)) + ce
    met = np.zeros(16)
    rows = np.zeros_like(eps) if defect == "epsum cleared before it reaches the metric" else eps
    met[:7] = rows[:, done].astype(np.float64).sum(1)
    met[8], met[9], met[10], met[14], met[15] = done.sum(), t["truncated"].sum(), t["terminated"].sum(), (~t["finite"]).sum(), t["ep_len_end"][done].sum()
    st[EPSUM0:EPSUM0 + 7] = np.where(done, F(0), eps)
    # observation
    q = st[QW:QW + 4]
    e = np.stack([np.arctan2(F(2) * (q[0] * q[1] + q[2] * q[3]), F(1) - F(2) * (q[1] * q[1] + q[2] * q[2])),
                  np.arcsin(np.clip(F(2) * (q[0] * q[2] - q[3] * q[1]), -1, 1)),
                  np.arctan2(F(2) * (q[0] * q[3] + q[1] * q[2]), F(1) - F(2) * (q[2] * q[2] + q[3] * q[3]))]).astype(F)
    e = np.where(e < 0, e + F(REF.TWO_PI), e).astype(F)
    yaw = f(rd["yaw"])
    if quad:
        e[2] = np.where(done, yaw - F(REF.TWO_PI) * np.floor(yaw * F(1 / REF.TWO_PI)), e[2])
    if defect == "Euler yaw left unwrapped after a reset":
        e[2] = np.where(done, yaw, e[2])
    obs = np.concatenate([st[PX:PX + 3], e, vb, wb, np.clip(act, -1, 1)]).T.astype(F)
    return dict(state=st, ep_len=t["ep_len"], obs=obs, reward=reward, terminated=t["terminated"], truncated=t["truncated"], metrics=met)


DEFECTS = ["Ro transposed in the push increment", "push rotated by the pre-reset R", "dwz added to wb_o.z", "last action not zeroed on reset",
           "Euler yaw left unwrapped after a reset", "a w == 0 term still added to epsum", "epsum cleared before it reaches the metric",
           "lf timer from lf_next on a reset step"]


def _defect_inputs():
    """case B's pushes and tilted cars with case C's bookkeeping: every defect has something to act on"""
    out = []
    for k, p, ref, pre, pre_ep, post, a, noise, got in oracle_steps("B"):
        p.weight[2], p.weight[0], p.log_episode_sums = 0.0, -10.0, 1
        pre = pre.copy()
        n = pre.shape[1]
        pre[EPSUM0:EPSUM0 + 7] = (0.01 * (1 + np.arange(7))[:, None] * (1 + np.arange(n))[None]).astype(F)
        if k == 2:      # one step with the default (long) lf interval: envs that reset and do not fire the lf push
            p.lf_interval[0], p.lf_interval[1] = 0.8, 1.2
        t = _tail(p, ref, pre, pre_ep, post, a, k)
        out.append((p, t, post, dict(action=a, timers=(pre[TIMER_HF], pre[TIMER_LF]), epsum=pre[EPSUM0:EPSUM0 + 8])))
    return out


def test_bound_accepts_the_correct_path_in_four_summation_orders_and_rejects_eight_defects():
    cases = _defect_inputs()
    for order in range(4):
        for quad in (True, False):
            for p, t, post, pre in cases:
                fails, _, _ = REF.check_step(emulate(t, post, pre, p, None, order, quad), t, post, p)
                assert not fails, (order, quad, fails)
    for defect in DEFECTS:
        caught = 0
        for p, t, post, pre in cases:
            fails, _, _ = REF.check_step(emulate(t, post, pre, p, defect), t, post, p)
            caught += bool(fails)
        print(f"{defect}: rejected on {caught} of {len(cases)} steps")
        assert caught >= 1, defect


# ---- the documented error of atan2_fast, measured on the host build ----------------------------------------------------------------
def test_atan2_fast_on_the_host_build_stays_within_its_documented_error(tmp_path):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host probe")
    out = tmp_path / "libwl_drift_tail_host.so"
    subprocess.run([CLANG, "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), os.path.join(ROOT, "tests", "host_sim", "drift_tail_host.cpp"),
                    "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    rng = np.random.RandomState(0)
    n = 1 << 22
    mag, ang = 10.0 ** rng.uniform(-6, 3, n), rng.uniform(-np.pi, np.pi, n)
    y, x = (mag * np.sin(ang)).astype(F), (mag * np.cos(ang)).astype(F)
    k = n // 16
    y[:k], x[k:2 * k] = 0, 0                                               # both axes
    y[2 * k:3 * k], y[3 * k:4 * k] = x[2 * k:3 * k], -x[3 * k:4 * k]           # the octant seams
    y[4 * k:5 * k] *= F(1e-4)
    x[5 * k:6 * k] *= F(1e-4)
    got = np.zeros(n, F)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    lib.hs_atan2_fast(n, ptr(y), ptr(x), ptr(got))
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err = np.abs(got - want)
    print(f"atan2_fast, host build, {n} arguments: max abs error {err.max():.3e} ({err[np.abs(want) < np.pi / 4].max():.3e} where nothing unfolds)")
    assert err.max() <= 3 * REF.U * np.pi + REF.ATAN2_ERR
    assert err[np.abs(want) < np.pi / 4].max() <= REF.ATAN2_ERR + REF.U * np.pi / 4
    # the Euler angles of tilted cars through the same build, against the reference and ITS bound
    q = rng.normal(size=(4096, 4))
    q[:, 1:3] *= 0.2
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    e = np.zeros((4096, 3), F)
    lib.hs_euler_xyz(4096, ptr(q), ptr(e))
    ref, m = REF.euler(q.T)
    d = np.abs(e.T - ref)
    d = np.minimum(d, np.abs(REF.TWO_PI - d))
    assert (d <= REF.N_EULER * REF.U * m + REF.ATAN2_ERR + REF.HW_REL).all(), float((d / (REF.N_EULER * REF.U * m + REF.ATAN2_ERR + REF.HW_REL)).max())

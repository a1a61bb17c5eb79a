"""The post-physics tail of the drift step restated in float64 (test infrastructure: never imported by the product).

`drift_env_step` (wheeledlab_amd/csrc/wl_drift_env.h) from "terminations" to "back to memory form": terminations, the seven
reward terms, reward, episode sums, the episode metrics, the reset draw, the two interval pushes, the timers, and the 14-dim
observation row.  Inputs are the fp32 rows a step stores (oracle/layout.py); everything is computed in float64 and every branch
is decided in float64.  The draws come from oracle/philox.py with the word layout at the top of wl_drift_env.h (event block:
x pose index | x, y y | yaw, z hf | lf timer, w lf kick | lf timer; WL_RS_NOISE1: z hf dvx | dvy, w hf kick | hf timer).

Bound.  An element passes when |got - ref| <= n U m + E: U = 2^-24, n = the fp32 roundings on the element's longest path in the
kernel source, m = the first-order magnitude (the sum of the absolute values of the terms and partial products on that path, as
tests/ppo_reference.py does), E = the absolute allowance of the approximate intrinsics on the path.  That is the issue's tau m
with tau = n U + E / m.  Nothing here was tuned against GPU output.

Intrinsics (wl_math.h documents each figure; the documented one is used):
  atan2_fast   1.3e-7 abs (polynomial in fp32 Horner form; its rcp, the product t = mn rcp(mx) and the two unfolding
               subtractions are counted as roundings of pi on top).  Measured, wl_math.h built for the host
               (tests/host_sim/drift_tail_host.cpp) against float64 atan2 over 4 194 304 arguments (both signs of both
               arguments, |y| <> |x|, both axes, magnitudes 1e-6 .. 1e3; tests/test_drift_tail_reference_cpu.py repeats the
               measurement and asserts it): 3.45e-7 abs in all and 1.37e-7 where |result| < pi / 4 (no unfolding; the
               result's own rounding included); the allowance 3 U pi + ATAN2_ERR = 5.6e-7 + 1.3e-7 = 6.9e-7 covers it.  The host build divides exactly where the device uses
               v_rcp_f32 (1 ulp): HW_REL covers it.
  sincos_fast  1e-6 abs (v_sin_f32 / v_cos_f32; "~1e-6 abs").  On the path of a RESET env only: the stored quaternion is
               (cos, 0, 0, sin)(yaw / 2) from sincos_fast while the quad form's observation takes the yaw itself and both forms
               build the push frame Ro from w^2 - z^2, 2 w z.  |w^2 + z^2 - 1| <= 2 sqrt2 eps moves the yaw read back from the
               stored quaternion by <= 4 sqrt2 eps (6 SINCOS_ERR allowed) and a rotated push increment by <= 2 sqrt2 eps |dv|
               (4 SINCOS_ERR |dv| allowed).
  fsqrt, rcp, rsq   1 ulp = 2^-23 relative ("1 ulp class").

Roundings per element, counted from wl_drift_env.h / wl_math.h / wl_drift_terms.h (fma = one rounding):
  element                       n    path
  obs pos                       0    stored value (+1: the noise fma, every noisy element)
  obs euler x, y, z             7    argument pair 3 (w x, fma, 1 - 2(..) as product + fma) | t = mn rcp 1 | unfold 2 | wrap 1;
                                     m = (m_ay + m_ax) / hypot(ax, ay) + 2 pi;  E = ATAN2_ERR + HW_REL (+ 6 SINCOS_ERR: yaw, reset)
  obs base lin vel              5    rotation entry 2 (product, fma) | mul_t 3; +3 on an hf push (v += dv, two fmas);
                                     m = sum_j mR_ji (|v_j| + 2 |dv_j|);  E = 4 SINCOS_ERR sum|dv| (reset)
  obs base ang vel              5    stored ww = mul(R, wb): 3 | entry 2 (the float64 side rotates the STORED ww back);
                                     +3 per push; m = sum_j mR_ji sum_k mR_jk |wb_k| + 2 mR_2i |dwz|;  E = 4 SINCOS_ERR |dwz| (reset)
  obs last action               0    v_med3 of the stored value
  term side_slip                8    body velocity 5 | atan2 as above (arguments already rounded: 0 + 1 + 2);  E as euler
  term vel_dist                 9    body velocity 5 | x^2 + y^2 2 | gs - target 1 | fma 1;  E = HW_REL gs 2 |gs - target|
  term progress                 0    stored ww.z
  term turn_left_go_right       6    body rate 5 | product 1
  term energy_through_turn      8    body velocity 5 | dot 3
  term cross_track_dist         5    dy 1 | x x, fma 2 | - r 1 | + offset 1;  E = HW_REL on the square root
  reward                        +9   per term: t w, (t w) dt 2 | seven chained adds 7
  episode sum                   +3   contribution 2 | the add 1
  metric WL_M_EPSUM0..7         episode sum + (episodes ended + WL_M_SHARDS) adds, m = sum of |contributions| (any order)
  timers                        re-armed: one fmaf of a 16-bit uniform = the float64 value rounded once: EXACT; decremented: 1
  push increments               (2 u - 1) vel: the float64 product rounded once: EXACT
  reset pose                    position, yaw: one fmaf each: EXACT as values; the quaternion SINCOS_ERR + 2 U
The terms, the reward and the sums are propagated item by item in `tail` (every rounding above times the magnitude of ITS operands,
a term's error through the next operation's slope), which is the same first-order bound without lumping a path into one m.
The numpy oracle (oracle/drift_step.py) spends more roundings on some paths (a rotation entry is 4 operations, einsum sums and
products round separately: 6 per rotated component, Euler arguments 4): ORACLE_EXTRA is added when the oracle is the other side.

Thresholds.  A fp32 kernel may decide otherwise than float64 where a decision lies within its own bound of the threshold:
`near_threshold` marks those envs from the reference's own quantities: the circular ends of cart_off_track (d^2 against r_in^2,
r_out^2; on the straights |x| is compared with the radius as stored: no band), the side-slip gates (|angle| against slip_min and
slip_max, |v_bx| against slip_min_vx), a timer within 1 ulp of (timer, step_dt) of 1e-6.  ep_len + 1 >= max is an integer
comparison: its band is empty, no env is excused for it.  An Euler angle within its bound of the wrap at 0 / 2 pi may come out a
turn away: `observation` returns that mask per angle and the caller compares those on the circle."""
import numpy as np

from oracle import philox as PH
from oracle.layout import ACT0, EPSUM0, PX, QW, STEER_POS, VX, WX, M_COUNT, M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS, M_TERM0, M_TIMEOUTS

F = np.float32
U = 2.0 ** -24
ATAN2_ERR = 1.3e-7
SINCOS_ERR = 1e-6
HW_REL = 2.0 ** -23
TWO_PI = 2.0 * np.pi
M_SHARDS = 32
N_TERMS = 7
# roundings (table above)
N_EULER, N_BODY, N_PUSH, N_NOISE = 7, 5, 3, 1
N_TERM = dict(side_slip=8, vel_dist=9, tlgr=6, energy=8, cross_track=5)
N_CONTRIB, N_REWARD_ADDS, N_EPSUM_ADD = 2, 7, 1
ORACLE_EXTRA = 4          # numpy: rotation entry 4 instead of 2, rotated component 5 instead of 3 (see the docstring)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def fp(x):
    """a parameter as the kernel holds it: the fp32 value, in float64"""
    return np.float64(np.float32(x))


def step_dt(p):
    """the kernel's step_dt = sim_dt * (float)decimation, one fp32 product"""
    return np.float64(F(p.sim_dt) * F(p.decimation))


def rotation(q):
    """q [4, n] -> R [3, 3, n] (body -> world), mR: the magnitudes of its entries' terms"""
    w, x, y, z = f64(q)
    a = np.abs
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    mR = np.array([[1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(z * w)), 2 * (a(x * z) + a(y * w))],
                   [2 * (a(x * y) + a(z * w)), 1 + 2 * (x * x + z * z), 2 * (a(y * z) + a(x * w))],
                   [2 * (a(x * z) + a(y * w)), 2 * (a(y * z) + a(x * w)), 1 + 2 * (x * x + y * y)]])
    return R, mR


def to_body(R, v):
    """R^T v: [3, n]"""
    return np.einsum("jin,jn->in", R, v)


def atan2_m(ay, ax, may, max_):
    """the magnitude of atan2_fast(ay, ax) on arguments whose own magnitudes are may, max_"""
    r = np.sqrt(np.maximum(ax * ax + ay * ay, 1e-300))
    return (may + max_) / r + TWO_PI


def wrap(a):
    return np.where(a < 0, a + TWO_PI, a)


def euler(q):
    """-> angles [3, n] wrapped as wrap_2pi does, m [3, n]"""
    w, x, y, z = f64(q)
    a = np.abs
    ry, rx = 2 * (w * x + y * z), 1 - 2 * (x * x + y * y)
    sp = 2 * (w * y - z * x)
    cp2 = np.maximum(1 - sp * sp, 0.0)
    cp = np.sqrt(cp2)
    yy, yx = 2 * (w * z + x * y), 1 - 2 * (y * y + z * z)
    ang = np.stack([np.arctan2(ry, rx), np.arctan2(sp, cp), np.arctan2(yy, yx)])
    m_sp = 2 * (a(w * y) + a(z * x))
    m_cp = (1 + sp * sp) / np.maximum(2 * cp, 1e-300) + cp        # sqrt of a rounded 1 - sp^2, then its own ulp
    m = np.stack([atan2_m(ry, rx, 2 * (a(w * x) + a(y * z)), 1 + 2 * (x * x + y * y)),
                  atan2_m(sp, cp, m_sp, m_cp),
                  atan2_m(yy, yx, 2 * (a(w * z) + a(x * y)), 1 + 2 * (y * y + z * z))])
    return wrap(ang), m


def observation(state_rows, last_action, params, noise=None, events=None, extra_roundings=0):
    """The 14-dim row of a STORED state: rows [>= 13, n] fp32 (layout.py), last_action [2, n] fp32 (the stored rows), noise
    [12, n] standard normals or None.  events (what the step did to the env after physics; None: nothing): dict(reset bool [n],
    dv [2, n], dw [n]: the absolute push increments, pushes [n]: how many pushes).  -> dict(obs [n, 14], m, bound, wrap_near
    [n, 3]: the angle is within its bound of the wrap)."""
    s = f64(state_rows)
    n = s.shape[1]
    p = params
    ev = events or {}
    reset = np.asarray(ev.get("reset", np.zeros(n, bool)))
    dv = f64(ev.get("dv", np.zeros((2, n))))
    dw = f64(ev.get("dw", np.zeros(n)))
    pushes = f64(ev.get("pushes", np.zeros(n)))
    hf = (np.abs(dv).sum(0) > 0).astype(np.float64)
    R, mR = rotation(s[QW:QW + 4])
    v, ww = s[VX:VX + 3], s[WX:WX + 3]
    vb, wb = to_body(R, v), to_body(R, ww)
    mv = np.abs(v).copy()
    mv[:2] += 2 * np.abs(dv)
    m_vb = np.einsum("jin,jn->in", mR, mv)
    m_ww = np.einsum("jkn,kn->jn", mR, np.abs(wb))
    m_wb = np.einsum("jin,jn->in", mR, m_ww) + 2 * mR[2] * dw[None]
    e, m_e = euler(s[QW:QW + 4])
    val = np.concatenate([s[PX:PX + 3], e, vb, wb])                                   # [12, n]
    m = np.concatenate([np.abs(s[PX:PX + 3]), m_e, m_vb, m_wb])
    nr = np.concatenate([np.zeros((3, n)), np.full((3, n), float(N_EULER)), N_BODY + N_PUSH * hf[None].repeat(3, 0),
                         N_BODY + N_PUSH * pushes[None].repeat(3, 0)])
    nr[3:] += extra_roundings
    E = np.zeros((12, n))
    E[3:6] = ATAN2_ERR + HW_REL
    E[5] += np.where(reset, 6 * SINCOS_ERR, 0.0)
    E[6:9] = np.where(reset, 4 * SINCOS_ERR * np.abs(dv).sum(0), 0.0)[None]
    E[9:12] = np.where(reset, 4 * SINCOS_ERR * dw, 0.0)[None]
    if noise is not None and p.enable_corruption:
        z = f64(noise)[:12]
        std = np.repeat([fp(p.noise_std[k]) for k in range(4)], 3)[:, None]
        val = val + std * z
        m = m + np.abs(std * z)
        nr = nr + N_NOISE
        nr[:3] += extra_roundings
    act = np.clip(f64(last_action), -1.0, 1.0)
    bound = nr * U * m + E
    wrap_near = (np.minimum(e, TWO_PI - e) <= bound[3:6]).T
    z2 = np.zeros((2, n))
    return dict(obs=np.concatenate([val, act]).T, m=np.concatenate([m, np.abs(act)]).T, bound=np.concatenate([bound, z2]).T,
                wrap_near=wrap_near)


def _cart_off_track(x, y, p):
    """-> off [n] bool, near [n] bool (the circular ends within their band)"""
    s, r_in, r_out = fp(p.straight), fp(p.r_in), fp(p.r_out)
    straight = np.abs(y) < s
    dy = np.where(y > 0, y - s, y + s)
    d2 = dy * dy + x * x
    ro2, ri2 = np.float64(F(r_out) * F(r_out)), np.float64(F(r_in) * F(r_in))   # the kernel's r * r, one fp32 product
    off = np.where(straight, (np.abs(x) > r_out) | (np.abs(x) < r_in), (d2 > ro2) | (d2 < ri2))
    band = U * (2 * np.abs(dy) * (np.abs(y) + s) + 2 * (dy * dy + x * x))
    near = ~straight & ((np.abs(d2 - ro2) <= band) | (np.abs(d2 - ri2) <= band))
    return off, near


def reset_draw(p, ref_table, seed, step, gid):
    """reset_from_block: -> pos [3, n], yaw [n] (fp32-exact values), q [4, n] (float64 cos / sin of yaw / 2), the re-armed timers"""
    u = PH.uniform8(gid, step, PH.S_DRIFT_EVENTS, seed)
    n_ref = int(p.num_ref_points)
    idx = np.minimum((u[0] * F(n_ref)).astype(np.int32), n_ref - 1)          # the kernel's fp32 product, as the oracle
    ref = f64(ref_table)
    once = lambda x: f64(x.astype(F))                                         # noqa: E731 -- one fmaf: the exact value rounded once
    px = once((2 * f64(u[1]) - 1) * fp(p.pos_noise) + ref[0, idx])
    py = once((2 * f64(u[2]) - 1) * fp(p.pos_noise) + ref[1, idx])
    yaw = once((2 * f64(u[3]) - 1) * fp(p.yaw_noise) + ref[2, idx])
    q = np.stack([np.cos(0.5 * yaw), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(0.5 * yaw)])
    return dict(pos=np.stack([px, py, np.zeros_like(px)]), yaw=yaw, q=q, timer_hf=rearm(p.hf_interval, u[4]),
                timer_lf=rearm(p.lf_interval, u[5]))


def rearm(interval, u):
    """fmaf(u, hi - lo, lo): hi - lo is one fp32 subtraction, the fma the exact value rounded once"""
    lo, span = fp(interval[0]), np.float64(F(interval[1]) - F(interval[0]))
    return f64((f64(u) * span + lo).astype(F))


def sym(u, a):
    """(2 u - 1) a: 2 u - 1 is exact in fp32 for a 16-bit uniform, the product rounds once"""
    return f64(((2 * f64(u) - 1) * fp(a)).astype(F))


def tail(post_state, ep_len, epsum, last_action, action, params, seed, step, gid, timers=None, ref_table=None):
    """The tail from the post-physics rows.  post_state [>= 19, n] fp32: the rows after physics, before reset and pushes;
    ep_len [n] and epsum [8, n] as they stood BEFORE the step; last_action: the rows stored before the step (the tail does not
    read them: kept for the call's symmetry); action [n, 2]: this step's raw action; timers (hf, lf) [n] before the step;
    ref_table [3, 32].  -> dict, every float quantity with its bound under the same key + "_b"."""
    p = params
    s = f64(post_state)
    n = s.shape[1]
    gid = np.asarray(gid)
    dt = step_dt(p)
    a = np.abs
    finite = np.isfinite(s[:ACT0]).all(0)
    sf = np.where(finite[None], s[:ACT0], 0.0)           # the terms of a non-finite env are not used: keep the arithmetic quiet
    pos, q, v, ww, th = sf[PX:PX + 3], sf[QW:QW + 4], sf[VX:VX + 3], sf[WX:WX + 3], sf[STEER_POS]
    off, near_track = _cart_off_track(pos[0], pos[1], p)
    terminated = ~finite | off
    ep_new = np.asarray(ep_len).astype(np.int64) + 1
    truncated = ep_new >= int(p.max_episode_length)
    done = terminated | truncated
    # ---- terms ----
    R, mR = rotation(q)
    vb, wb = to_body(R, v), to_body(R, ww)
    d_vb = N_BODY * U * np.einsum("jin,jn->in", mR, a(v))
    m_ww = np.einsum("jkn,kn->jn", mR, a(wb))
    d_wb = N_BODY * U * np.einsum("jin,jn->in", mR, m_ww)
    T, B = np.zeros((N_TERMS, n)), np.zeros((N_TERMS, n))
    # side_slip
    ang = a(np.arctan2(vb[1], vb[0]))
    hyp = np.sqrt(np.maximum(vb[0] ** 2 + vb[1] ** 2, 1e-300))
    b_ang = (d_vb[0] + d_vb[1]) / hyp + 3 * U * np.pi + HW_REL + ATAN2_ERR
    smin, smax, svx = fp(p.slip_min), fp(p.slip_max), fp(p.slip_min_vx)
    gate = (a(vb[0]) < svx) | (ang > smax)
    ss = np.where(gate, 0.0, ang)
    T[0], B[0] = np.where(ss < smin, 0.0, ss), b_ang
    moving = hyp > 1e-12
    near_slip = moving & ((a(a(vb[0]) - svx) <= d_vb[0]) | ((a(vb[0]) >= svx - d_vb[0]) & ((a(ang - smax) <= b_ang) | (a(ang - smin) <= b_ang))))
    # vel_dist
    gs = np.sqrt(vb[0] ** 2 + vb[1] ** 2)
    d_gs = (a(vb[0]) * d_vb[0] + a(vb[1]) * d_vb[1]) / np.maximum(gs, 1e-300) + (2 * U + HW_REL) * gs
    d_gs = np.where(gs > 0, d_gs, d_vb[0] + d_vb[1])
    tg, so = fp(p.speed_target), fp(p.speed_offset)
    dd = gs - tg
    T[1] = dd * dd + so
    B[1] = 2 * a(dd) * (d_gs + U * (gs + a(tg))) + U * (dd * dd + a(so))
    # progress, turn_left_go_right
    T[2] = ww[2]
    th_ = fp(p.tlgr_thresh)
    c = np.clip(wb[2], -th_, th_)
    T[3] = np.maximum(-th * c, 0.0)
    B[3] = a(th) * d_wb[2] + U * a(th * c)
    # energy_through_turn
    on_turn = a(pos[1]) > fp(p.straight)
    e3 = (vb ** 2).sum(0)
    T[4] = np.where(on_turn, e3, 0.0)
    B[4] = np.where(on_turn, 2 * (a(vb) * d_vb).sum(0) + 3 * U * e3, 0.0)
    # cross_track_dist
    st, rl, co, cp_ = fp(p.straight), fp(p.r_line), fp(p.ctd_offset), fp(p.ctd_p)
    x, y = pos[0], pos[1]
    dy = np.where(y > 0, y - st, y + st)
    rad = np.sqrt(dy * dy + x * x)
    d_lin = a(np.where(x > 0, x - rl, x + rl))
    d_arc = a(rad - rl)
    lin = a(y) < st
    d = np.where(lin, d_lin, d_arc)
    d_rad = (a(dy) * U * (a(y) + st) + 2 * U * (dy * dy + x * x)) / np.maximum(rad, 1e-300) + HW_REL * rad
    b_d = np.where(lin, U * (a(x) + rl), d_rad + U * (rad + rl))
    ctd = d + co
    b_ctd = b_d + U * (d + a(co))
    if cp_ == 1.0:
        T[5], B[5] = ctd, b_ctd
    else:
        with np.errstate(invalid="ignore"):
            T[5] = np.power(ctd, cp_)
            B[5] = a(cp_) * np.power(a(ctd), cp_ - 1) * b_ctd + 4 * U * a(T[5])      # powf: 2 ulp
    T[6] = (terminated & ~truncated).astype(np.float64)
    T = np.where(finite[None], T, 0.0)
    B = np.where(finite[None], B, 0.0)
    # ---- reward, episode sums ----
    w = np.array([fp(p.weight[i]) for i in range(N_TERMS)])
    live = (w != 0)[:, None] & finite[None]
    contrib = np.where(live, T * w[:, None] * dt, 0.0)
    contrib_b = np.where(live, a(w[:, None] * dt) * B + N_CONTRIB * U * a(contrib), 0.0)
    reward = contrib.sum(0)
    reward_b = contrib_b.sum(0) + N_REWARD_ADDS * U * a(contrib).sum(0)
    eps0 = f64(epsum)[:8].copy()
    log = bool(p.log_episode_sums)
    eps = np.where(log, eps0, 0.0)
    eps_end = eps.copy()
    eps_end[:N_TERMS] += contrib
    eps_end_b = np.zeros((8, n))
    eps_end_b[:N_TERMS] = contrib_b + np.where(live, N_EPSUM_ADD * U * (a(eps[:N_TERMS]) + a(contrib)), 0.0)
    eps_new = np.where(done[None], 0.0, eps_end)          # what the step stores (when log_episode_sums)
    eps_new[N_TERMS:] = eps0[N_TERMS:]                    # the step reads, clears and reports the seven term rows only
    # ---- metrics ----
    met, met_b = np.zeros(M_COUNT), np.zeros(M_COUNT)
    nd = int(done.sum())
    met[M_EPSUM0:M_EPSUM0 + N_TERMS] = eps_end[:N_TERMS, done].sum(1)
    met_b[M_EPSUM0:M_EPSUM0 + N_TERMS] = eps_end_b[:N_TERMS, done].sum(1) + (nd + M_SHARDS) * U * a(eps_end[:N_TERMS, done]).sum(1)
    met[M_RESETS], met[M_TIMEOUTS], met[M_TERM0] = nd, truncated.sum(), terminated.sum()
    met[M_NONFINITE], met[M_EPLEN] = (~finite).sum(), ep_new[done].sum()
    # ---- reset, pushes, timers ----
    rd = reset_draw(p, ref_table, seed, step, gid)
    t_hf0, t_lf0 = f64(timers[0]), f64(timers[1])
    t_hf = np.where(done, rd["timer_hf"], t_hf0)
    t_lf = np.where(done, rd["timer_lf"], t_lf0)
    eps6 = np.float64(F(1e-6))
    dv, dw_hf, dw_lf = np.zeros((2, n)), np.zeros(n), np.zeros(n)
    hf_fire = lf_fire = np.zeros(n, bool)
    near_timer = np.zeros(n, bool)
    if p.enable_pushes:
        u = PH.uniform8(gid, step, PH.S_NOISE1, seed)[4:]
        hf_dec = t_hf - dt
        hf_fire = hf_dec < eps6
        near_timer |= a(hf_dec - eps6) <= U * (a(t_hf) + dt)
        dv = np.where(hf_fire[None], np.stack([sym(u[0], p.hf_vel_x), sym(u[1], p.hf_vel_y)]), 0.0)
        dw_hf = np.where(hf_fire, sym(u[2], p.hf_vel_yaw), 0.0)
        t_hf = np.where(hf_fire, rearm(p.hf_interval, u[3]), hf_dec)
        u = PH.uniform8(gid, step, PH.S_DRIFT_EVENTS, seed)[6:]
        lf_dec = t_lf - dt
        lf_fire = lf_dec < eps6
        near_timer |= a(lf_dec - eps6) <= U * (a(t_lf) + dt)
        dw_lf = np.where(lf_fire, sym(u[0], p.lf_vel_yaw), 0.0)
        t_lf = np.where(lf_fire, rearm(p.lf_interval, u[1]), lf_dec)
    act = f64(action).T
    if p.action.clip_wrapper:
        act = np.clip(act, -1.0, 1.0)
    last_new = np.where(done[None], 0.0, act)
    return dict(finite=finite, terminated=terminated, truncated=truncated, done=done, terms=T, terms_b=B, contrib=contrib,
                contrib_b=contrib_b, reward=reward, reward_b=reward_b, epsum_end=eps_end, epsum_end_b=eps_end_b, epsum=eps_new,
                ep_len=np.where(done, 0, ep_new), ep_len_end=ep_new, metrics=met, metrics_b=met_b, reset=rd,
                timer_hf=t_hf, timer_lf=t_lf, hf_fire=hf_fire, lf_fire=lf_fire, dv=dv, dw_hf=dw_hf, dw_lf=dw_lf, last_action=last_new,
                near_track=near_track & finite, near_slip=near_slip & finite, near_timer=near_timer, dt=dt)


def near_threshold(t):
    """envs a correct fp32 kernel may decide otherwise than float64 (see the module docstring), from the tail's own quantities"""
    return t["near_track"] | t["near_slip"] | t["near_timer"]


def events_of(t):
    """what `observation` needs to know about the step that stored the state"""
    return dict(reset=t["done"], dv=np.abs(t["dv"]), dw=np.abs(t["dw_hf"]) + np.abs(t["dw_lf"]),
                pushes=t["hf_fire"].astype(np.float64) + t["lf_fire"].astype(np.float64))


def stored_state(t, post_state, params):
    """the rows a correct step stores, from the tail's result and the post-physics rows: [DRIFT_ROWS, n] float64 plus a bound
    of the same shape (0 = the value is exact)"""
    from oracle.layout import DRIFT_ROWS, TIMER_HF, TIMER_LF, WHEEL, STEER_VEL
    s = f64(post_state)[:DRIFT_ROWS].copy()
    n = s.shape[1]
    b = np.zeros_like(s)
    done, fin, rd = t["done"], t["finite"], t["reset"]
    s[PX:PX + 3] = np.where(done[None], rd["pos"], s[PX:PX + 3])
    s[QW:QW + 4] = np.where(done[None], rd["q"], s[QW:QW + 4])
    b[QW:QW + 4] = np.where(done[None], SINCOS_ERR + 2 * U, 0.0)
    b[[QW + 1, QW + 2]] = 0.0
    s[VX:VX + 6] = np.where(done[None], 0.0, s[VX:VX + 6])
    bad = done & ~fin
    s[WHEEL:WHEEL + 4] = np.where(bad[None], 0.0, s[WHEEL:WHEEL + 4])
    s[STEER_POS] = np.where(bad, 0.0, s[STEER_POS])
    s[STEER_VEL] = np.where(bad, 0.0, s[STEER_VEL])
    pre = np.abs(s[VX:VX + 6]).copy()
    s[VX:VX + 2] += t["dv"]
    s[WX + 2] += t["dw_hf"] + t["dw_lf"]
    # v += dv may be one fma with the increment's product or two roundings: 2 U on the terms; on a reset env 0 + dv is exact
    b[VX:VX + 2] = np.where(done[None], 0.0, 2 * U * (pre[:2] + np.abs(t["dv"])) * (t["dv"] != 0))
    both = (t["dw_hf"] != 0) & (t["dw_lf"] != 0)
    b[WX + 2] = np.where(done & ~both, 0.0, 4 * U * (pre[5] + np.abs(t["dw_hf"]) + np.abs(t["dw_lf"])) * ((t["dw_hf"] != 0) | (t["dw_lf"] != 0)))
    s[ACT0:ACT0 + 2] = t["last_action"]
    s[TIMER_HF], s[TIMER_LF] = t["timer_hf"], t["timer_lf"]
    if params.enable_pushes:      # re-armed by a push: exact; decremented: one fp32 subtraction, held to 1 ulp
        b[TIMER_HF] = np.where(t["hf_fire"], 0.0, ulp(s[TIMER_HF]))
        b[TIMER_LF] = np.where(t["lf_fire"], 0.0, ulp(s[TIMER_LF]))
    if params.log_episode_sums:
        s[EPSUM0:EPSUM0 + 8] = t["epsum"]
        b[EPSUM0:EPSUM0 + 8] = np.where(done[None], 0.0, t["epsum_end_b"])
    return s, b


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def check_step(got, t, post_state, params, noise=None, scale=1.0, extra_roundings=0, floor_ulps=0, where=""):
    """One stored step against the reference.  got: dict(state [>= 35, n] fp32 rows after the step, ep_len [n], obs [n, 14],
    reward [n], terminated, truncated [n] bool, metrics [16]: this step's increments, or None); t = tail(...) of the same step;
    post_state: the rows after physics.  `scale` multiplies the float bounds (2: two fp32 sides); floor_ulps: ulps allowed on the stored rows the kernel forms with
    ONE fma where the other side (the numpy oracle) rounds twice.  Envs in near_threshold(t) are
    excused from everything but the wrap and range checks.  -> (list of failure strings, number of excused envs, worst ratio)."""
    from oracle.layout import DRIFT_ROWS
    fails = []
    near = near_threshold(t)
    ok = ~near
    n = ok.size
    worst = 0.0

    def hold(name, g, r, b, mask=None, floor=0.0):
        nonlocal worst
        g, r, b = f64(g), f64(r), f64(b) * scale + floor
        err = np.abs(g - r)
        bad = ~(err <= b)                       # a NaN fails
        if mask is not None:
            bad &= mask
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
        if mask is not None:
            ratio = np.where(mask, ratio, 0.0)
        fin = ratio[np.isfinite(ratio)]
        worst = max(worst, float(fin.max(initial=0.0)))
        if bad.any():
            i = np.argwhere(bad)[0]
            fails.append(f"{where}{name}: {int(bad.sum())} outside the bound, first at {tuple(int(k) for k in i)}: got {g[tuple(i)]!r} want "
                         f"{r[tuple(i)]!r} bound {b[tuple(i)]:.3e}")

    st = np.asarray(got["state"])[:DRIFT_ROWS]
    # decisions
    for name in ("terminated", "truncated"):
        d = np.asarray(got[name]).astype(bool) != t[name]
        if (d & ok).any():
            fails.append(f"{where}{name}: {int((d & ok).sum())} decisions differ away from a threshold, first env {int(np.argmax(d & ok))}")
    same = (np.asarray(got["terminated"]).astype(bool) == t["terminated"]) & (np.asarray(got["truncated"]).astype(bool) == t["truncated"])
    live = ok & same
    hold("reward", got["reward"], t["reward"], t["reward_b"], live)
    if not np.array_equal(np.asarray(got["ep_len"])[live], t["ep_len"][live]):
        fails.append(f"{where}ep_len differs")
    want, wb_ = stored_state(t, post_state, params)
    rows = DRIFT_ROWS if params.log_episode_sums else EPSUM0
    fin_rows = np.isfinite(want[:rows]).all(0)
    want_f = np.where(fin_rows[None], want[:rows], 0.0)
    hold("stored state", st[:rows], want_f, wb_[:rows] + floor_ulps * ulp(want_f) / scale, (live & fin_rows)[None].repeat(rows, 0))
    # observation of the stored state
    o = observation(st, st[ACT0:ACT0 + 2], params, noise, events_of(t), extra_roundings)
    g_obs, r_obs = f64(got["obs"]), o["obs"].copy()
    turn = np.zeros_like(r_obs, dtype=bool)
    turn[:, 3:6] = o["wrap_near"]
    if noise is None or not params.enable_corruption:
        if not ((g_obs[:, 3:6] >= 0) & (g_obs[:, 3:6] <= TWO_PI + 1e-6)).all():
            fails.append(f"{where}an Euler angle of the observation is outside [0, 2 pi]")
    d = g_obs - r_obs
    r_obs = np.where(turn & (np.abs(d) > np.pi), r_obs + TWO_PI * np.sign(d), r_obs)     # within reach of the wrap: a turn away is the same angle
    hold("observation", g_obs, r_obs, o["bound"], live[:, None].repeat(14, 1))
    # metrics
    if got.get("metrics") is not None and same.all():
        m = f64(got["metrics"])
        cnt = [M_RESETS, M_TIMEOUTS, M_TERM0, M_NONFINITE, M_EPLEN]
        if not np.array_equal(m[cnt], t["metrics"][cnt]):
            fails.append(f"{where}metric counts {m[cnt].tolist()} != {t['metrics'][cnt].tolist()}")
        if True:
            hold("metric episode sums", m[:8], t["metrics"][:8], t["metrics_b"][:8])
    return fails, int(near.sum()), worst


# ---- the cases of tests/test_gpu_drift_tail.py (and of the excusal cap in tests/test_drift_tail_reference_cpu.py) ----------------
N_ENVS, K_STEPS, MAX_LEN = 256 + 37, 6, 7
NAN_ENV = 101


def apply_case(p, tag):
    """edit a parameter set IN PLACE (the product's ctypes struct or the oracle's namespace: same field names)"""
    dt = float(F(p.sim_dt) * F(p.decimation))
    p.max_episode_length = MAX_LEN
    if tag == "A":       # quiet
        p.enable_pushes, p.enable_corruption = 0, 0
    elif tag == "B":     # every step pushes, the step of a reset included
        p.enable_corruption = 0
        p.hf_interval[0], p.hf_interval[1], p.lf_interval[0], p.lf_interval[1] = 0.0, dt, 0.0, dt
        p.hf_vel_x, p.hf_vel_y, p.hf_vel_yaw, p.lf_vel_yaw = 1.0, 0.7, 1.3, 0.9
    elif tag == "C":     # bookkeeping
        p.weight[2], p.weight[0] = 0.0, -10.0
        p.log_episode_sums, p.enable_corruption = 1, 1
    return p


def prepare_case(tag, st, ep, n, p):
    """edit the host copy of a freshly reset batch IN PLACE: st [rows, stride] fp32, ep [stride] int32"""
    from oracle.mathlib import quat_from_euler_xyz
    ep[:n] = np.arange(n) % MAX_LEN                       # a seventh of the batch times out per step
    if tag == "A":
        k = np.arange(24)
        r = np.where(k % 2 == 0, p.r_out + 0.01 * (1 + k), p.r_in - 0.01 * (1 + k // 2)).astype(F)
        ang = (0.26 * k).astype(F)
        st[PX, 40:64] = r * np.cos(ang)
        st[PX + 1, 40:64] = np.where(np.sin(ang) >= 0, p.straight, -p.straight) * (k % 3 != 0) + r * np.sin(ang) * (k % 3 != 0)
    elif tag == "B":
        k = np.arange(n)[::5]
        yaw = 2 * np.arctan2(st[QW + 3, k], st[QW, k])
        st[QW:QW + 4, k] = quat_from_euler_xyz(0.3 * np.where(k % 2, 1, -1), 0.3 * np.where(k % 3, 1, -1), yaw).T
    elif tag == "C":
        st[EPSUM0:EPSUM0 + N_TERMS, :n] = (0.01 * (1 + np.arange(N_TERMS))[:, None] * (1 + np.arange(n))[None]).astype(F)
        st[VX, NAN_ENV] = np.nan


def case_actions(k, n):
    rng = np.random.RandomState(100 + k)
    a = rng.uniform(-1.2, 1.2, (n, 2)).astype(F)
    a[:, 0] = np.abs(a[:, 0])
    return a


def case_noise(k, stride):
    return np.random.RandomState(200 + k).normal(size=(12, stride)).astype(F)

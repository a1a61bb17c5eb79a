"""The post-physics tail of the elevation step restated in float64 (test infrastructure: never imported by the product).

`elev_env_step` (wheeledlab_amd/csrc/wl_elev_env.h) from `veh_post` on, in its own order: the four terminations and the non-finite
rule, the four reward terms (both read the command the PREVIOUS step left), reward and episode sums, the episode metrics, the
curriculum's level (decided before the spawn), the reset draw, the command count-down / resample (after the reset: a resetting
env's resample lands on its new tile), the command re-expressed from the post-reset position and yaw, and the 13 proprioceptive
values of the post-reset state with the zeroed last action.  Inputs are the fp32 rows a step stores (oracle/layout.py); every
operation and every branch is float64.  One thing of fp32 is part of the DEFINITION, not of the error: its range.  A squared goal
distance or a dot product beyond FLT_MAX is +-inf, as in the reference project's fp32 torch (a command of 1e30 m gives progress =
offset + v.g * 0 in fp32, where float64 would divide two finite numbers); `rng` applies it.

The blocks the visual task shares through wl_implicit_task.h are functions of their own: `finite_rule`, `weigh_rewards`,
`episode_end_metrics`, `veh_reset`.  (`finite_rule`: veh_post tests the SUM of the car's rows; a row that is NaN or infinite makes
the sum so, which is what is restated.  Sixteen finite rows whose fp32 sum overflows would also count as non-finite: rows of
1e37 and more, which no case here holds.)

Bound.  An element passes when |got - ref| <= n U m + E (tests/drift_tail_reference.py's method: U = 2^-24, n = the fp32 roundings
on the element's longest path, m = the first-order magnitude propagated item by item, E = the intrinsics' documented error;
-ffp-contract=fast: where the source does not spell the fma the UNFUSED path is counted).  Nothing was tuned against GPU output.

Roundings per element (wl_math.h: mat_from_quat, mul_t, atan2_fast; wl_elev_env.h: elev_terms, yaw_cs, write_elev_prop;
wl_implicit_task.h: veh_post, weigh_rewards):
  element                      n    path
  R entry                      3    diagonal: q.y y2 | 1 - . | fma (off-diagonal: product | fma = 2; the diagonal's count is used)
  vb, wb (mul_t)               6    entry 3 | product, fma, fma 3;  m = sum_j mR_ji |v_j|
  wheel_sum                    3    three adds of four spins, any order (quad_sum is a butterfly, the lane form left to right)
  gx, gy (goal vector)         1    cb - pos;  m = |cb| + |pos|
  goal distance                +3   gx^2 | fma | correctly rounded sqrtf
  term goal_progress           gx, gy 1 | dot 2 | g2 2 | rsq HW_REL | product 1 | + offset 1
  term higher_elevation        1    pos.z - elev_z0 (the clamp is exact)
  term falling, stuck_penalty  0    0 / 1
  reward                       per term t w, (t w) dt 2 | four chained adds 4
  episode sum                  contribution 2 | the add 1
  metric WL_M_EPSUM0..3        episode sum + (episodes ended + WL_M_SHARDS) adds, m = sum of |sums| (any order)
  reset x, y, targets          (2 u - 1) a: the float64 product rounded once (2 u - 1 is exact for a 24-bit u): EXACT; with levels
                               add_unfused(origin, .): one more fp32 add of two known fp32 values: EXACT
  reset vx, vy                 one fmaf of a uniform: EXACT
  reset z                      fmaxf(reset_z, zt + clearance): the contact sampler's bound (tests/heightfield_reference.py) + 1
  reset quaternion             (cos, 0, 0, sin)(yaw / 2): SINCOS_ERR + 3 U (the revolutions product, the results); x, y EXACT zeros
  timer                        re-armed: cmd_resample_s itself: EXACT.  Counted down: timer - sim_dt (float)decimation, which the
                               compiler may contract into one fma with the UNROUNDED product: 2 U (|timer| + dt)
  level, episode length        integers: EXACT
  CMD_BX / CMD_BY              yaw_cs: a 3 (m 1 + 2 (y^2 + z^2)), b 2 (m 2 (|w z| + |x y|)), a^2 + b^2 2, rsq HW_REL, product 1;
                               dx, dy 1 each; fma + product 2
  obs goal                     1    cb - pos of the STORED command, nan_to_num
  obs euler                    7    drift_tail_reference.euler (the same wl_math.h paths);  E = ATAN2_ERR + HW_REL
  obs base lin / ang vel       6    as vb, of the stored v / ww; clamp exact
  obs last action              0    clamp of the stored value
The numpy oracle (oracle/elev_step.py) rounds every product and sum of a rotation and of a dot product separately:
ORACLE_EXTRA more roundings on every float element when the oracle is the other side.

Thresholds.  `near_threshold(t)` marks, from the float64 quantities and their bounds, the envs where a correct fp32 kernel may
decide otherwise:
  pos.z against min_height     pos.z is a stored row and min_height a parameter: the comparison is exact, its band EMPTY
  stuck                        min(vb.x, cap) within d(vb.x) of stuck_min_vel while the wheel gate is open or near, or the wheel
                               sum within 3 U sum|spin| of stuck_wheel_spin while the velocity gate is open or near
  R33 against upright_cos      3 U (1 + 2 (x^2 + y^2))
  goal distance / goal_dist    d(distance) from the table; a goal within 1e-19 m (g2 leaves fp32's normal range: rsq(0))
  higher_elevation's gates     z against elev_min: U (|pos.z| + |z0|); vb.x against elev_min_vel: d(vb.x)
  fall_vel gate                vb.z within d(vb.z)
  timer against 0              the counted-down timer within its bound of 0
ep_len + 1 >= max_episode_length and the level rule compare integers: no band.  An Euler angle within its bound of the 0 / 2 pi seam
is compared on the circle (`observation` returns the mask per angle)."""
from types import SimpleNamespace

import numpy as np

import heightfield_reference as HR
import terrain_levels_reference as TLR
from drift_tail_reference import ATAN2_ERR, HW_REL, SINCOS_ERR, TWO_PI, U, euler, f64, fp, rotation, step_dt, to_body, ulp
from oracle import philox as PH
from oracle.layout import (ACT0, CMD_BX, CMD_BY, CMD_TIMER, EPSUM0, PX, QW, S_COUNT, STEER_POS, STEER_VEL, TGT_H, TGT_X, TGT_Y, VX,
                           WHEEL, WX, M_COUNT, M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS, M_TERM0, M_TIMEOUTS)

F = np.float32
FLT_MAX = float(np.finfo(F).max)
M_SHARDS = 32
N_TERMS, N_FLAGS = 4, 4
OBS_DIM = 13 + 26 * 26
ES_RESET, ES_CMD_RESET, ES_CMD_RESAMPLE = 0, 1, 2          # wl_elev_env.h ElevStream (ES_LEVEL = 3: terrain_levels_reference)
N_BODY, N_WHEEL, N_R33, N_EULER = 6, 3, 3, 7
N_CONTRIB, N_REWARD_ADDS, N_EPSUM_ADD = 2, 4, 1
ORACLE_EXTRA = 4
GOAL_TINY = 1e-19


def rng(x):
    """fp32's range as part of the definition: beyond FLT_MAX is +-inf"""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > FLT_MAX, np.sign(x) * np.inf, x)


def once(x):
    """a float64 value the kernel forms with ONE fp32 rounding"""
    return f64(np.asarray(x, np.float64).astype(F))


def sym(u, a):
    return once((2 * f64(u) - 1) * fp(a))


def field_of(hf, outside_z=None):
    """what heightfield_reference takes, from an oracle tuple (decoded fp32 heights, x0, y0, cell[, outside_z]) or a
    heightfield_cases.Field"""
    if hasattr(hf, "heights"):
        return hf
    h, x0, y0, cell, *rest = hf
    h = np.asarray(h, F)
    oz = float(rest[0]) if rest else 0.0
    return SimpleNamespace(heights=h, x0=float(F(x0)), y0=float(F(y0)), cell=float(F(cell)), nx=h.shape[1], ny=h.shape[0],
                           outside_z=float(F(oz if outside_z is None else outside_z)))


def book_of(state, ep_len):
    """the pre-step bookkeeping of a state matrix [S_COUNT, n]"""
    s = np.asarray(state)
    return dict(ep_len=np.asarray(ep_len), cb=s[CMD_BX:CMD_BX + 2], epsum=s[EPSUM0:EPSUM0 + N_TERMS], tgt=s[TGT_X:TGT_H + 1], timer=s[CMD_TIMER])


# ---- the blocks wl_implicit_task.h shares with the visual task ------------------------------------------------------------------
def finite_rule(post):
    """veh_post: the car is finite when the SUM of its integrated rows is (a NaN or an inf anywhere makes it NaN or inf)"""
    return np.isfinite(f64(post)[:ACT0]).all(0)


def weigh_rewards(weight, T, B, finite, dt, log, epsum_in):
    """-> contrib, contrib_b, reward, reward_b, epsum_end, epsum_end_b: weight x term x step_dt summed (nothing for a non-finite car
    or a zero weight) and the episode sums that carry it"""
    a = np.abs
    w = np.array([fp(weight[i]) for i in range(T.shape[0])])
    live = (w != 0)[:, None] & finite[None]
    with np.errstate(invalid="ignore", over="ignore"):
        contrib = np.where(live, rng(rng(T * w[:, None]) * dt), 0.0)
        contrib_b = np.where(live, a(w[:, None] * dt) * B + N_CONTRIB * U * a(contrib), 0.0)
        reward = contrib.sum(0)
        reward_b = contrib_b.sum(0) + N_REWARD_ADDS * U * a(contrib).sum(0)
        eps = np.where(log, f64(epsum_in), 0.0)
        eps_end = np.where(log, eps + contrib, 0.0)
        eps_end_b = np.where(log, contrib_b + N_EPSUM_ADD * U * (a(eps) + a(contrib)), 0.0)
    return contrib, contrib_b, reward, reward_b, eps_end, eps_end_b


def episode_end_metrics(eps_end, eps_end_b, done, truncated, finite, flags, ep_new):
    """an ending episode into the metrics: its sums, the reset, a time-out, the flags of a FINITE car, a non-finite car, its length"""
    met, met_b = np.zeros(M_COUNT), np.zeros(M_COUNT)
    nd, k = int(done.sum()), eps_end.shape[0]
    with np.errstate(invalid="ignore"):
        met[M_EPSUM0:M_EPSUM0 + k] = eps_end[:, done].sum(1)
        met_b[M_EPSUM0:M_EPSUM0 + k] = eps_end_b[:, done].sum(1) + (nd + M_SHARDS) * U * np.abs(eps_end[:, done]).sum(1)
    met[M_RESETS], met[M_TIMEOUTS] = nd, (truncated & done).sum()
    for i, fl in enumerate(flags):
        met[M_TERM0 + i] = (fl & finite & done).sum()
    met[M_NONFINITE], met[M_EPLEN] = (~finite & done).sum(), ep_new[done].sum()
    return met, met_b


def veh_reset(post, done, finite, pos, pos_b, q, q_b, v):
    """the dynamic rows [ACT0, n] a step stores: a resetting env takes the drawn pose and velocity, its angular velocity is zeroed,
    a non-finite car's wheel spins and steering too -> rows, bound (0 = exact)"""
    s = f64(post)[:ACT0].copy()
    b = np.zeros_like(s)
    d = done[None]
    s[PX:PX + 3], b[PX:PX + 3] = np.where(d, pos, s[PX:PX + 3]), np.where(d, pos_b, 0.0)
    s[QW:QW + 4], b[QW:QW + 4] = np.where(d, q, s[QW:QW + 4]), np.where(d, q_b, 0.0)
    s[VX:VX + 3] = np.where(d, v, s[VX:VX + 3])
    s[WX:WX + 3] = np.where(d, 0.0, s[WX:WX + 3])
    bad = (done & ~finite)[None]
    s[WHEEL:WHEEL + 4] = np.where(bad, 0.0, s[WHEEL:WHEEL + 4])
    s[STEER_POS:STEER_VEL + 1] = np.where(bad, 0.0, s[STEER_POS:STEER_VEL + 1])
    return s, b


# ---- the elevation task's own ----------------------------------------------------------------------------------------------------
def elev_terms(p, pos, q, v, wheel, cb, truncated, extra=0, vb=None):
    """elev_terms + what veh_post recomputes for it -> dict(flags [4, n], T, B [4, n], near masks).  vb: the body-frame velocity as
    an INPUT (the reference project's goldens draw it independently of the quaternion) instead of R^T v"""
    a = np.abs
    nb = N_BODY + extra
    R, mR = rotation(q)
    if vb is None:
        vb = to_body(R, v)
        d_vb = nb * U * np.einsum("jin,jn->in", mR, a(v))
    else:
        vb, d_vb = f64(vb), np.zeros_like(f64(vb))
    ws = wheel.sum(0)
    d_ws = (N_WHEEL + extra) * U * a(wheel).sum(0)
    cap, vmin, spin = fp(p.stuck_vel_cap), fp(p.stuck_min_vel), fp(p.stuck_wheel_spin)
    vx_c = np.minimum(vb[0], cap)
    g_vel, g_spin = vx_c < vmin, ws > spin
    n_vel = (a(vx_c - vmin) <= d_vb[0]) & (vb[0] < cap + d_vb[0])
    n_spin = a(ws - spin) <= d_ws
    stuck = g_vel & g_spin
    near_stuck = (n_vel & (g_spin | n_spin)) | (n_spin & (g_vel | n_vel))
    low = pos[2] < fp(p.min_height)
    up = R[2][2]
    roll = up <= fp(p.upright_cos)
    near_roll = a(up - fp(p.upright_cos)) <= (N_R33 + extra) * U * mR[2][2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gx, gy = f64(cb[0]) - pos[0], f64(cb[1]) - pos[1]
        d_gx, d_gy = (1 + extra) * U * (a(f64(cb[0])) + a(pos[0])), (1 + extra) * U * (a(f64(cb[1])) + a(pos[1]))
        g2 = rng(gx * gx + gy * gy)
        dist = np.sqrt(g2)
        ok = np.isfinite(dist) & (dist > 0)
        safe = np.where(ok, dist, 1.0)
        d_g = np.where(ok, (a(gx) * d_gx + a(gy) * d_gy) / safe, 0.0)
        d_dist = d_g + (2 + extra) * U * np.where(ok, dist, 0.0)
        goal = dist < fp(p.goal_dist)
        near_goal = (a(dist - fp(p.goal_dist)) <= d_dist) | (dist <= GOAL_TINY)
        dot = rng(v[0] * gx + v[1] * gy)
        d_dot = a(v[0]) * d_gx + a(v[1]) * d_gy + (2 + extra) * U * (a(v[0] * gx) + a(v[1] * gy))
        inv = np.where(np.isinf(g2), 0.0, 1.0 / dist)                         # rsq(inf) = 0, rsq(0) = inf
        prog = dot * inv
        off = fp(p.progress_offset)
        T0 = off + prog
        rel = d_g / safe + (1 + extra) * U + HW_REL
        B0 = np.where(ok, d_dot / safe + a(prog) * (rel + U) + U * (a(off) + a(prog)), 0.0)
    z0, emin, eminv = fp(p.elev_z0), fp(p.elev_min), fp(p.elev_min_vel)
    z = pos[2] - z0
    d_z = (1 + extra) * U * (a(pos[2]) + a(z0))
    T1 = np.clip(np.where((z > emin) & (vb[0] > eminv), z, 0.0), 0.0, 1.0)
    near_elev = ((a(z - emin) <= d_z) & (vb[0] > eminv - d_vb[0])) | ((a(vb[0] - eminv) <= d_vb[0]) & (z > emin - d_z))
    fall = fp(p.fall_vel)
    T2 = (vb[2] > fall).astype(np.float64)
    near_fall = a(vb[2] - fall) <= d_vb[2]
    T3 = (stuck & ~truncated).astype(np.float64)
    n = pos.shape[1]
    T, B = np.stack([T0, T1, T2, T3]), np.stack([B0, np.where(T1 > 0, d_z, 0.0), np.zeros(n), np.zeros(n)])
    return dict(flags=np.stack([low, stuck, roll, goal]), T=T, B=B, vb=vb, d_vb=d_vb, near_stuck=near_stuck, near_roll=near_roll,
                near_goal=near_goal, near_elev=near_elev, near_fall=near_fall)


_slopes = {}


def _contact_ztol(field, x, y):
    """heightfield_reference.contact_bounds' height tolerance, with the field's slope map computed once per field"""
    if id(field) not in _slopes:
        _slopes[id(field)] = (field, HR.slope_map(field)[0], float(np.abs(field.heights).max()))
    _, s, hmax = _slopes[id(field)]
    u, v = HR._uv(field, x, y)
    i, j = HR._cell_index(field, u, v)
    return 4 * HR.ulp32(hmax) + s[j, i] * field.cell * HR.pos_err(field, x, y)


def reset_draw(p, field, seed, step, gid, origin=None):
    """draw_elev_reset / draw_elev_reset_local + place_elev_reset (origin [2, n] fp32: the env's NEW tile centre, or None)"""
    u = PH.uniform4(gid, step, ES_RESET, seed)
    c = PH.uniform4(gid, step, ES_CMD_RESET, seed)
    x, y = sym(u[0], p.reset_xy), sym(u[1], p.reset_xy)
    tx, ty = sym(c[0], p.cmd_xy), sym(c[1], p.cmd_xy)
    if origin is not None:
        o = f64(origin)
        x, y, tx, ty = once(o[0] + x), once(o[1] + y), once(o[0] + tx), once(o[1] + ty)
    zt, _, _ = HR.sample64(field, x.astype(F), y.astype(F), guard=True)
    ztol = _contact_ztol(field, x.astype(F), y.astype(F))
    clr, rz = fp(p.spawn_clearance), fp(p.reset_z)
    z = np.maximum(rz, zt + clr)
    z_b = ztol + U * (np.abs(zt) + clr)
    yaw = sym(u[2], p.reset_yaw)
    zero = np.zeros_like(yaw)
    q = np.stack([np.cos(0.5 * yaw), zero, zero, np.sin(0.5 * yaw)])
    q_b = np.stack([zero + SINCOS_ERR + 3 * U, zero, zero, zero + SINCOS_ERR + 3 * U])
    lo, span = fp(p.reset_vel[0]), np.float64(F(p.reset_vel[1]) - F(p.reset_vel[0]))
    vx, vy = once(f64(u[3]) * span + lo), once(f64(c[3]) * span + lo)
    return dict(pos=np.stack([x, y, z]), pos_b=np.stack([zero, zero, z_b]), q=q, q_b=q_b, v=np.stack([vx, vy, zero]),
                tgt=np.stack([tx, ty, sym(c[2], p.cmd_heading)]))


def origins(levels, level):
    """tile_origin: [2, n] fp32 centres of tile (level, type), both indices clamped"""
    rows, cols = int(levels["rows"]), int(levels["cols"])
    t = np.clip(level, 0, rows - 1).astype(np.int64) * cols + np.clip(levels["type"], 0, cols - 1)
    return np.asarray(levels["origins"], F).reshape(-1, 2)[t].T


def tail(post, book, action, p, seed, step, gid, field, levels=None, extra=0):
    """The tail from the post-physics rows.  post [>= ACT0, n] fp32; book: book_of(pre-step state); action [2, n]: the processed action
    the step stores; field: field_of(..); levels: dict(level [n] BEFORE the step, type [n], origins, rows, cols) or None.
    -> dict, every float quantity with its bound under the same key + "_b"."""
    s = f64(post)
    n = s.shape[1]
    gid = np.asarray(gid)
    dt = step_dt(p)
    finite = finite_rule(post)
    sf = np.where(finite[None], s[:ACT0], 0.0)
    sf[QW] = np.where(finite, sf[QW], 1.0)
    ep_new = np.asarray(book["ep_len"]).astype(np.int64) + 1
    truncated = ep_new >= int(p.max_episode_length)
    tm = elev_terms(p, sf[PX:PX + 3], sf[QW:QW + 4], sf[VX:VX + 3], sf[WHEEL:WHEEL + 4], f64(book["cb"]), truncated, extra)
    flags = tm["flags"] & finite[None]                                    # a non-finite car's comparisons are not used
    terminated = ~finite | flags.any(0)
    done = terminated | truncated
    T, B = np.where(finite[None], tm["T"], 0.0), np.where(finite[None], tm["B"], 0.0)
    log = bool(p.log_episode_sums)
    contrib, contrib_b, reward, reward_b, eps_end, eps_end_b = weigh_rewards(p.weight, T, B, finite, dt, log, f64(book["epsum"])[:N_TERMS])
    met, met_b = episode_end_metrics(eps_end, eps_end_b, done, truncated, finite, flags, ep_new)
    # ---- curriculum, reset ----
    level = None
    origin = None
    if levels is not None:
        level = np.asarray(levels["level"]).astype(np.int32).copy()
        ids = np.nonzero(done)[0]
        if len(ids):
            level[ids] = TLR.next_levels(dict(levels, level=level.copy()), ids, flags[3], terminated, seed, step, int(gid[0]))
        origin = origins(levels, level)
    rd = reset_draw(p, field, seed, step, gid, origin)
    dyn, dyn_b = veh_reset(np.where(finite[None], s[:ACT0], np.nan), done, finite, rd["pos"], rd["pos_b"], rd["q"], rd["q_b"], rd["v"])
    # ---- command manager ----
    rs = fp(p.cmd_resample_s)
    tgt = np.where(done[None], rd["tgt"], f64(book["tgt"]))
    t_in = np.where(done, rs, f64(book["timer"]))
    t_dec = t_in - dt
    t_dec_b = 2 * U * (np.abs(t_in) + dt)
    expired = t_dec <= 0
    near_timer = np.abs(t_dec) <= t_dec_b
    u = PH.uniform4(gid, step, ES_CMD_RESAMPLE, seed)
    new = np.stack([sym(u[0], p.cmd_xy), sym(u[1], p.cmd_xy), sym(u[2], p.cmd_heading)])
    if origin is not None:
        new[0], new[1] = once(f64(origin[0]) + new[0]), once(f64(origin[1]) + new[1])
    tgt = np.where(expired[None], new, tgt)
    timer = np.where(expired, rs, t_dec)
    timer_b = np.where(expired, 0.0, t_dec_b)
    act = np.where(done[None], 0.0, f64(action))
    eps_new = np.where(done[None], 0.0, eps_end)
    return dict(finite=finite, flags=flags, terminated=terminated, truncated=truncated, done=done, terms=T, terms_b=B, contrib=contrib,
                contrib_b=contrib_b, reward=reward, reward_b=reward_b, epsum_end=eps_end, epsum_end_b=eps_end_b, epsum=eps_new,
                ep_len=np.where(done, 0, ep_new), ep_len_end=ep_new, metrics=met, metrics_b=met_b, reset=rd, level=level, dyn=dyn,
                dyn_b=dyn_b, tgt=tgt, timer=timer, timer_b=timer_b, expired=expired, last_action=act, dt=dt,
                near_stuck=tm["near_stuck"] & finite, near_roll=tm["near_roll"] & finite, near_goal=tm["near_goal"] & finite,
                near_elev=tm["near_elev"] & finite, near_fall=tm["near_fall"] & finite, near_timer=near_timer)


NEAR_KEYS = ("near_stuck", "near_roll", "near_goal", "near_elev", "near_fall", "near_timer")


def near_threshold(t):
    """envs a correct fp32 kernel may decide otherwise than float64 (module docstring), from the tail's own quantities"""
    out = np.zeros(t["done"].shape, bool)
    for k in NEAR_KEYS:
        out |= t[k]
    return out


def stored_state(t, p):
    """the rows a correct step stores, except CMD_BX / CMD_BY (a function of the STORED rows: `command`): [S_COUNT, n] float64, a
    bound of the same shape (0 = exact) and the rows that are held"""
    n = t["done"].size
    s, b = np.zeros((S_COUNT, n)), np.zeros((S_COUNT, n))
    s[:ACT0], b[:ACT0] = t["dyn"], t["dyn_b"]
    s[ACT0:ACT0 + 2] = t["last_action"]
    rows = list(range(ACT0 + 2)) + [TGT_X, TGT_Y, TGT_H, CMD_TIMER]
    s[TGT_X:TGT_H + 1], s[CMD_TIMER], b[CMD_TIMER] = t["tgt"], t["timer"], t["timer_b"]
    if p.log_episode_sums:
        s[EPSUM0:EPSUM0 + N_TERMS] = t["epsum"]
        b[EPSUM0:EPSUM0 + N_TERMS] = np.where(t["done"][None], 0.0, t["epsum_end_b"])
        rows += list(range(EPSUM0, EPSUM0 + N_TERMS))
    return s, b, np.array(rows)


def command(state, extra=0):
    """CMD_BX / CMD_BY of a STORED state: the target re-expressed in the yaw-aligned base frame -> cb [2, n], bound"""
    a = np.abs
    s = f64(state)
    w, x, y, z = s[QW:QW + 4]
    ca, cbb = 1 - 2 * (y * y + z * z), 2 * (w * z + x * y)
    r = np.sqrt(np.maximum(ca * ca + cbb * cbb, 1e-300))
    c, sn = ca / r, cbb / r
    d_cs = ((3 + extra) * U * (1 + 2 * (y * y + z * z)) + (2 + extra) * U * 2 * (a(w * z) + a(x * y))) / r + (2 + extra) * U + HW_REL
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = s[TGT_X] - s[PX], s[TGT_Y] - s[PX + 1]
        d_dx, d_dy = (1 + extra) * U * (a(s[TGT_X]) + a(s[PX])), (1 + extra) * U * (a(s[TGT_Y]) + a(s[PX + 1]))
        cb = np.stack([rng(c * dx + sn * dy), rng(-sn * dx + c * dy)])
        m = a(c * dx) + a(sn * dy), a(sn * dx) + a(c * dy)
        bound = np.stack([(a(dx) + a(dy)) * d_cs + a(c) * d_dx + a(sn) * d_dy + (2 + extra) * U * m[0],
                          (a(dx) + a(dy)) * d_cs + a(sn) * d_dx + a(c) * d_dy + (2 + extra) * U * m[1]])
    return cb, bound


def observation(state, p, extra=0):
    """the 13 proprioceptive values of a STORED state -> dict(obs [n, 13], bound [n, 13], wrap_near [n, 3])"""
    a = np.abs
    s = f64(state)
    n = s.shape[1]
    clip = fp(p.obs_clip)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.stack([s[CMD_BX] - s[PX], s[CMD_BY] - s[PX + 1]])
        g_b = (1 + extra) * U * np.stack([a(s[CMD_BX]) + a(s[PX]), a(s[CMD_BY]) + a(s[PX + 1])])
        g = np.clip(np.where(np.isnan(g), 0.0, g), -FLT_MAX, FLT_MAX)
        g_b = np.where(np.isfinite(g_b), g_b, 0.0)
    e, m_e = euler(s[QW:QW + 4])
    e_b = (N_EULER + extra) * U * m_e + ATAN2_ERR + HW_REL
    R, mR = rotation(s[QW:QW + 4])
    vb, wb = to_body(R, s[VX:VX + 3]), to_body(R, s[WX:WX + 3])
    nb = (N_BODY + extra) * U
    vb_b, wb_b = nb * np.einsum("jin,jn->in", mR, a(s[VX:VX + 3])), nb * np.einsum("jin,jn->in", mR, a(s[WX:WX + 3]))
    act = np.clip(s[ACT0:ACT0 + 2], -1.0, 1.0)
    obs = np.concatenate([g, e, np.clip(vb, -clip, clip), np.clip(wb, -clip, clip), act])
    bound = np.concatenate([g_b, e_b, vb_b, wb_b, np.zeros((2, n))])
    wrap_near = (np.minimum(e, TWO_PI - e) <= e_b).T
    return dict(obs=obs.T, bound=bound.T, wrap_near=wrap_near)


def _ulp(x):
    """the fp32 spacing at x (0 where x is not finite, the largest binade's at FLT_MAX)"""
    return ulp(np.clip(np.nan_to_num(x, posinf=0, neginf=0), -1e38, 1e38))


def _hold(name, g, r, b, mask, fails, where, floor=0.0):
    """|g - r| <= b on `mask`; where the reference is NaN or infinite the value must be that -> the worst finite ratio"""
    g, r, b = f64(g), f64(r), f64(b) + floor
    with np.errstate(invalid="ignore", divide="ignore"):
        special = ~np.isfinite(r)
        same = (np.isnan(r) & np.isnan(g)) | (r == g)
        err = np.abs(g - r)
        bad = np.where(special, ~same, ~(err <= b)) & mask
        ratio = np.where(special | ~mask, 0.0, np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0)))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        fails.append(f"{where}{name}: {int(bad.sum())} outside the bound, first at {i}: got {g[i]!r} want {r[i]!r} bound {b[i]:.3e}")
    fin = ratio[np.isfinite(ratio)]
    return float(fin.max(initial=0.0))


def check_step(got, t, p, scale=1.0, extra=0, floor_ulps=0, where=""):
    """One stored step against the reference.  got: dict(state [S_COUNT, n] fp32 rows after the step, ep_len [n], obs [n, >= 13],
    reward [n], terminated, truncated [n] bool, level [n] or None, metrics [16]: this step's increments, or None); t = tail(...) of
    the same step (extra roundings are given to `tail` by the caller; `extra` here goes to `command` / `observation`).  Envs in
    near_threshold(t) are excused from everything but the range checks.  -> (failure strings, excused envs, worst ratio, {element:
    its worst ratio})."""
    fails = []
    per = {}
    near = near_threshold(t)
    ok = ~near
    for name in ("terminated", "truncated"):
        d = (np.asarray(got[name]).astype(bool) != t[name]) & ok
        if d.any():
            fails.append(f"{where}{name}: {int(d.sum())} decisions differ away from a threshold, first env {int(np.argmax(d))}")
    same = (np.asarray(got["terminated"]).astype(bool) == t["terminated"]) & (np.asarray(got["truncated"]).astype(bool) == t["truncated"])
    live = ok & same
    per["reward"] = _hold("reward", got["reward"], t["reward"], scale * t["reward_b"], live, fails, where, floor_ulps * _ulp(t["reward"]))
    if not np.array_equal(np.asarray(got["ep_len"])[live], t["ep_len"][live]):
        fails.append(f"{where}ep_len differs")
    if t["level"] is not None and not np.array_equal(np.asarray(got["level"])[live], t["level"][live]):
        fails.append(f"{where}level differs: {np.nonzero((np.asarray(got['level']) != t['level']) & live)[0][:4].tolist()}")
    st = np.asarray(got["state"])
    want, wb_, rows = stored_state(t, p)
    fl = floor_ulps * _ulp(want[rows])
    per["stored state"] = _hold("stored state", st[rows], want[rows], scale * wb_[rows], live[None].repeat(len(rows), 0), fails, where, fl)
    cb, cb_b = command(st, extra)
    per["command"] = _hold("command", st[CMD_BX:CMD_BX + 2], cb, scale * cb_b, live[None].repeat(2, 0), fails, where,
                           floor_ulps * _ulp(cb))
    o = observation(st, p, extra)
    g_obs, r_obs = f64(got["obs"])[:, :13], o["obs"].copy()
    if not ((g_obs[:, 2:5] >= 0) & (g_obs[:, 2:5] <= TWO_PI + 1e-6)).all():
        fails.append(f"{where}an Euler angle of the observation is outside [0, 2 pi]")
    turn = np.zeros_like(r_obs, dtype=bool)
    turn[:, 2:5] = o["wrap_near"]
    d = g_obs - r_obs
    r_obs = np.where(turn & (np.abs(d) > np.pi), r_obs + TWO_PI * np.sign(d), r_obs)
    per["observation"] = _hold("observation", g_obs, r_obs, scale * o["bound"], live[:, None].repeat(13, 1), fails, where,
                               floor_ulps * _ulp(r_obs))
    if got.get("metrics") is not None and same.all():
        m = f64(got["metrics"])
        cnt = [M_RESETS, M_TIMEOUTS, M_TERM0, M_TERM0 + 1, M_TERM0 + 2, M_TERM0 + 3, M_NONFINITE, M_EPLEN]
        if not np.array_equal(m[cnt], t["metrics"][cnt]):
            fails.append(f"{where}metric counts {m[cnt].tolist()} != {t['metrics'][cnt].tolist()}")
        k = slice(M_EPSUM0, M_EPSUM0 + N_TERMS)
        per["metric episode sums"] = _hold("metric episode sums", m[k], t["metrics"][k], scale * t["metrics_b"][k], np.ones(N_TERMS, bool), fails, where)
    return fails, int(near.sum()), max(per.values()), per


# ---- the cases of tests/test_gpu_elev_tail.py (and of the excusal cap in tests/test_elev_tail_reference_cpu.py) ------------------
N_ENVS, K_STEPS, MAX_LEN = 288 + 5, 6, 7
NAN_ENV, INF_ENV = 101, 202
BAD_CMD = {14: np.nan, 21: np.inf, 28: -np.inf, 35: 1e30, 42: -3e38}       # env -> command / target value (envs = 0 mod 7: no time-out in K steps)
TILE_ROWS, TILE_COLS, TILE_RESET_XY, TILE_CMD_XY = 3, 2, 1.0, 2.0          # case B: as tests/test_gpu_terrain_levels.py


def tile_cfg():
    """case B's generated terrain: 3 rows x 2 columns of 3.2 m tiles inside a 1 m frame"""
    from wheeledlab_amd.envs.terrain_gen_cfg import TerrainGeneratorCfg
    return TerrainGeneratorCfg(seed=4, num_rows=TILE_ROWS, num_cols=TILE_COLS, size=(3.2, 3.2), border_width=1.0)


def apply_case(p, tag, k=0):
    """edit a parameter set IN PLACE for step k of a case (the product's ctypes struct or the oracle's namespace: same field names)"""
    dt = float(F(p.sim_dt) * F(p.decimation))
    p.max_episode_length = MAX_LEN
    if tag == "A":       # thresholds moved so that every flag fires for a visible share of cars just reset
        p.stuck_min_vel, p.stuck_wheel_spin, p.goal_dist = -0.05, 2.0, 1.5
    elif tag == "B":     # tiles; on the second half of the run every env resamples every step, the step of its reset included
        p.reset_xy, p.cmd_xy = TILE_RESET_XY, TILE_CMD_XY
        p.cmd_resample_s = 0.5 * dt if k >= K_STEPS // 2 else 10.0
    elif tag == "C":     # reward and observation edges; spawns and goals inside field G1 (off-centre) and a little beyond it
        p.reset_xy, p.cmd_xy = 7.5, 9.0
        for i, w in enumerate((-30.0, 700.0, 0.0, 11.0)):
            p.weight[i] = w
        p.obs_clip = 1.0
        p.log_episode_sums = 0 if k == K_STEPS - 1 else 1
    return p


def stage_step(tag, k, st, ep, n, levels=None):
    """hand-set rows of step k IN PLACE, on the host copy of the state the step starts from: st [S_COUNT, stride] fp32, ep int32"""
    from oracle.mathlib import quat_from_euler_xyz
    e = np.arange(n)
    if k == 0:
        ep[:n] = e % MAX_LEN                                  # a seventh of the batch times out per step
        if tag == "C":
            st[EPSUM0:EPSUM0 + N_TERMS, :n] = (0.01 * (1 + np.arange(N_TERMS))[:, None] * (1 + e)[None]).astype(F)
        if tag == "B" and levels is not None:                 # rows 0, middle and top: "up from the top" draws, "down from 0" stays
            levels[:n] = e % TILE_ROWS
    cls = np.where(e % K_STEPS == k, (e // K_STEPS) % 8, -1)  # a sixth of the batch is staged per step, in eight classes
    m = cls == 0                                              # rolled past 60 degrees, clear of the ground
    yaw = 2 * np.arctan2(st[QW + 3, :n], st[QW, :n])
    st[QW:QW + 4, :n] = np.where(m[None], quat_from_euler_xyz(np.full(n, 1.25), np.full(n, 0.1), yaw).T, st[QW:QW + 4, :n]).astype(F)
    st[PX + 2, :n] += np.where(m, F(0.3), F(0))
    m = cls == 1                                              # beyond the field's edge: on the outside plane, below min_height
    st[PX, :n] = np.where(m, F(400.0), st[PX, :n])
    m = cls == 2                                              # goal within goal_dist (the command minus the WORLD position: the task's quirk)
    st[CMD_BX, :n] = np.where(m, st[PX, :n] + F(0.11), st[CMD_BX, :n])
    st[CMD_BY, :n] = np.where(m, st[PX + 1, :n] - F(0.07), st[CMD_BY, :n])
    m = cls == 3                                              # wheels spinning in the air
    st[PX + 2, :n] = np.where(m, F(3.0), st[PX + 2, :n])
    st[VX:VX + 3, :n] = np.where(m[None], F(0), st[VX:VX + 3, :n])
    st[WHEEL:WHEEL + 4, :n] = np.where(m[None], F(30.0), st[WHEEL:WHEEL + 4, :n])
    m = (cls == 4) | (cls == 5)                               # command timer about to expire
    st[CMD_TIMER, :n] = np.where(m, F(0.05), st[CMD_TIMER, :n])
    if tag == "C":
        st[VX, NAN_ENV], st[VX + 1, INF_ENV] = np.nan, np.inf
        for env, val in BAD_CMD.items():
            st[CMD_BX, env], st[TGT_X, env] = val, val
        st[CMD_BY, 14] = np.inf


def case_actions(tag, k, n):
    rng_ = np.random.RandomState(300 + k)
    a = rng_.uniform(-1.2, 1.2, (n, 2)).astype(F)
    a[:, 0] = np.abs(a[:, 0]) * F(0.6) + F(0.2)
    if tag == "C":
        a[::9] *= F(2.5)                                      # raw actions well beyond +-1
    return a


def processed_action(p, a):
    """what the step stores as the last action: process_action's clip (the ClipAction wrapper) -> [2, n]"""
    a = np.asarray(a, F)
    return (np.clip(a, -1, 1) if p.action.clip_wrapper else a).T

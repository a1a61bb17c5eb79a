"""The post-physics tail of the visual and visual-depth steps restated in float64 (test infrastructure: never imported by the product).

`visual_env_step` (wheeledlab_amd/csrc/wl_visual_env.h) from `veh_post` on, in its own order: the time-out, `out_of_map` and the
non-finite rule, the two reward terms (traversable_reward, forward_vel), reward and episode sums, the episode metrics, the reset
draw (a random traversable cell, a random yaw, on a heightfield the lift onto the terrain under the cell), the rows the step stores
and the eight proprioceptive values of the post-reset state with the zeroed last action.  Inputs are the fp32 rows a step stores
(oracle/layout.py); every operation is float64 -- except where fp32 is part of the DEFINITION and not of the error:
  * `out_of_map` compares two fp32 values (a stored position against 0.5f * (float)rows * spacing, formed as the kernel forms it);
  * `traversable` is the reference project's fp32 `get_map_id` -- (x + 0.5 width + 0.5 spacing) / spacing in fp32, truncated, clamped,
    map[yi][xi] -- computed in numpy float32 as oracle/visual_mdp.py does, on the fp32 spacing the kernel is handed;
  * the spawn cell is min((int)(u.x * (float)n_cells), n_cells - 1) with the fp32 product.
The blocks wl_implicit_task.h shares with the elevation task come from tests/elev_tail_reference.py: `finite_rule`,
`weigh_rewards` (T = 2), `episode_end_metrics` (the single flag `oom`), `veh_reset` (v = 0).

Bound.  An element passes when |got - ref| <= n U m + E (tests/drift_tail_reference.py's method: U = 2^-24, n = the fp32 roundings on
the element's longest path, m = the first-order magnitude propagated item by item, E = the intrinsics' documented error;
-ffp-contract=fast: where the source does not spell the fma the UNFUSED path is counted).  Nothing was tuned against GPU output.

Roundings per element (wl_math.h: mat_from_quat, mul_t, sincos_rev; wl_visual_env.h: visual_env_step, draw_visual_reset,
visual_reset_pose; wl_implicit_task.h: veh_post, weigh_rewards, episode_end_metrics, veh_reset, store_veh_rows):
  element                      n    path
  truncated                    0    ep_len + 1 >= max_episode_length: integers, EXACT
  out_of_map                   0    a strict comparison of two fp32 values: EXACT, no band; false for a non-finite car
  term traversable_reward      0    +-1 from the fp32 lookup above: EXACT, no band; 0 for a non-finite car
  R entry                      3    diagonal: q.y y2 | 1 - . | fma (off-diagonal: 2; the diagonal's count is used)
  term forward_vel (vb.x)      6    entry 3 | product, fma, fma 3 (elev_tail_reference.N_BODY);  m = sum_j mR_j0 |v_j|
  reward                       per term t w, (t w) dt 2 | the shared bound's four chained adds (two terms need two: an upper bound)
  episode sum                  contribution 2 | the add 1
  metric WL_M_EPSUM0..1        episode sum + (episodes ended + WL_M_SHARDS) adds, m = sum of |sums| (any order); slots 2..7 stay 0
  metric counts, WL_M_EPLEN    integers in fp32 (< 2^24): EXACT
  reset x, y                   ((float)ix - (float)(cols / 2)) * row_spacing, ((float)iy - (float)(rows / 2)) * col_spacing with
                               integer halves: an exact difference, the float64 product rounded once: EXACT
  reset z                      the plane: reset_z itself: EXACT.  A heightfield: reset_z + zt: the contact sampler's bound
                               (tests/heightfield_reference.py) + 1
  reset quaternion             (cos, 0, 0, sin) of u.y / 2 revolutions: SINCOS_ERR + 3 U (the halved uniform is exact, the
                               results); x, y EXACT zeros
  reset velocities             v = 0, ww = 0: EXACT.  A finite car keeps its wheel spins and steering rows (the post-physics
                               bits); a non-finite car's are zeroed: EXACT
  last action                  0 for a resetting env, else the processed action: EXACT
  episode length               0 for a resetting env, else ep_len + 1: EXACT
  WL_S_EPSUM0..1               as "episode sum", 0 for a resetting env; with log_episode_sums = 0 the rows are NOT written: the
                               pre-step bits, EXACT
  prop base lin / ang vel      6    mul_t(R, v), mul_t(R, ww) of the STORED (post-reset) state, not clamped
  prop last action             0    clamp of the stored value
The numpy oracle (oracle/visual_step.py) rounds every product and sum of a rotation separately: ORACLE_EXTRA more roundings on
every float element when the oracle is the other side.

Thresholds.  No comparison on this path has a band: both sides of `out_of_map` and every operand of the map lookup are fp32 values
the kernel and this module form by the same correctly rounded operations (0.5f * x and the halves are exact, so a contraction
changes nothing), and the time-out compares integers.  `near_threshold` therefore marks NOTHING, and the tests hold that zero
envs are excused.  (Positions beyond the range where `int` conversion is defined are not staged:
tests/parity_predicates.py::map_index_excused covers them against the goldens.)

A quirk that is pinned, not fixed: with an ODD map size the reference project's own formulas put a spawn one cell off its table
entry -- x = (ix - 50) s, and the lookup's (x + 50.5 s + 0.5 s) / s = ix + 1 truncates to cell ix + 1.  The kernel and
oracle/visual_step.reset_envs both reproduce that (case B, 101^2); "spawned on a white cell" holds on the even-sized map of case A
only."""
from types import SimpleNamespace

import numpy as np

import heightfield_reference as HR
from drift_tail_reference import SINCOS_ERR, U, f64, fp, rotation, step_dt, to_body
from elev_tail_reference import (M_SHARDS, N_BODY, ORACLE_EXTRA, _hold, _ulp, episode_end_metrics, field_of, finite_rule, once,  # noqa: F401
                                 processed_action, veh_reset, weigh_rewards)
from oracle import philox as PH
from oracle.layout import (ACT0, EPSUM0, PX, QW, S_COUNT, STEER_POS, VX, WHEEL, WX, M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS, M_TERM0,
                           M_TIMEOUTS)

F = np.float32
N_TERMS = 2                     # WL_VR_TRAVERSABLE, WL_VR_FORWARD_VEL
PROP_DIM = 8
VS_RESET = 0                    # the reset draw's Philox stream


# ---- the traversability map --------------------------------------------------------------------------------------------------------
def travmap(trav, spacing):
    """what the references take of a WlTravMap: the bool map [rows][cols], its traversable cells (iy, ix) in np.nonzero order and the
    two spacings as the fp32 values the kernel is handed"""
    trav = np.ascontiguousarray(np.asarray(trav, bool))
    ys, xs = trav.nonzero()
    return SimpleNamespace(trav=trav, cells=np.stack([ys, xs], -1).astype(np.int32), rows=trav.shape[0], cols=trav.shape[1],
                           rs=F(spacing[0]), cs=F(spacing[1]))


def half_extent(m):
    """out_of_map's two fp32 thresholds, formed as the kernel forms them: 0.5f * (float)rows * row_spacing, 0.5f * (float)cols * col_spacing"""
    return F(0.5) * F(F(m.rows) * m.rs), F(0.5) * F(F(m.cols) * m.cs)


def out_of_map(m, x, y):
    x, y = np.asarray(x, F), np.asarray(y, F)
    hw, hh = half_extent(m)
    with np.errstate(invalid="ignore"):
        return (x > hw) | (x < -hw) | (y > hh) | (y < -hh)


def map_id(m, x, y):
    """get_map_id in fp32 -> xi, yi (finite inputs within int range)"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    width, height = F(F(m.rows) * m.rs), F(F(m.cols) * m.cs)
    with np.errstate(all="ignore"):
        fx = (x + F(0.5) * width + F(0.5) * m.rs) / m.rs
        fy = (y + F(0.5) * height + F(0.5) * m.cs) / m.cs
        assert fx.dtype == F and fy.dtype == F
        return np.clip(fx.astype(np.int64), 0, m.rows - 1), np.clip(fy.astype(np.int64), 0, m.cols - 1)


def traversable(m, x, y):
    xi, yi = map_id(m, x, y)
    return m.trav[yi, xi]


def book_of(state, ep_len):
    """the pre-step bookkeeping of a state matrix [S_COUNT, n]"""
    s = np.asarray(state)
    return dict(ep_len=np.asarray(ep_len), epsum=s[EPSUM0:EPSUM0 + N_TERMS])


_slopes = {}


def _contact_ztol(field, x, y):
    """heightfield_reference.contact_bounds' height tolerance, the field's slope map computed once per field"""
    if id(field) not in _slopes:
        _slopes[id(field)] = (field, HR.slope_map(field)[0], float(np.abs(field.heights).max()))
    _, s, hmax = _slopes[id(field)]
    u, v = HR._uv(field, x, y)
    i, j = HR._cell_index(field, u, v)
    return 4 * HR.ulp32(hmax) + s[j, i] * field.cell * HR.pos_err(field, x, y)


def reset_draw(p, m, seed, step, gid, field=None, swap_uniforms=False, lift=True):
    """draw_visual_reset + visual_reset_pose -> dict(pos, pos_b, q, q_b, cell (iy, ix)).  (swap_uniforms / lift: the modelled defects
    of tests/test_visual_tail_reference_cpu.py)"""
    u = PH.uniform4(np.asarray(gid), step, VS_RESET, seed)
    ux, uy = (u[1], u[0]) if swap_uniforms else (u[0], u[1])
    n_cells = len(m.cells)
    k = np.minimum((np.asarray(ux, F) * F(n_cells)).astype(np.int64), n_cells - 1)
    iy, ix = m.cells[k, 0].astype(np.int64), m.cells[k, 1].astype(np.int64)
    x, y = once((ix - m.cols // 2) * f64(m.rs)), once((iy - m.rows // 2) * f64(m.cs))
    zero = np.zeros_like(x)
    rz = fp(p.reset_z)
    z, z_b = zero + rz, zero.copy()
    if field is not None and lift:
        zt, _, _ = HR.sample64(field, x.astype(F), y.astype(F), guard=True)
        z = rz + zt
        z_b = _contact_ztol(field, x.astype(F), y.astype(F)) + U * (np.abs(zt) + abs(rz))
    half = np.pi * f64(uy)                                                 # yaw / 2 = u / 2 revolutions
    q = np.stack([np.cos(half), zero, zero, np.sin(half)])
    q_b = np.stack([zero + SINCOS_ERR + 3 * U, zero, zero, zero + SINCOS_ERR + 3 * U])
    return dict(pos=np.stack([x, y, z]), pos_b=np.stack([zero, zero, z_b]), q=q, q_b=q_b, cell=np.stack([iy, ix]))


def tail(post, book, action, p, m, seed, step, gid, field=None, extra=0):
    """The tail from the post-physics rows.  post [>= ACT0, n] fp32; book: book_of(pre-step state); action [2, n]: the processed
    action the step stores; m: travmap(..); field: field_of(..) on a heightfield, None on the plane.
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
    x32, y32 = sf[PX].astype(F), sf[PX + 1].astype(F)
    oom = finite & out_of_map(m, x32, y32)
    trav = traversable(m, x32, y32) & finite
    R, mR = rotation(sf[QW:QW + 4])
    vb = to_body(R, sf[VX:VX + 3])
    d_vb = (N_BODY + extra) * U * np.einsum("jin,jn->in", mR, np.abs(sf[VX:VX + 3]))
    T = np.where(finite[None], np.stack([np.where(trav, 1.0, -1.0), vb[0]]), 0.0)
    B = np.where(finite[None], np.stack([np.zeros(n), d_vb[0]]), 0.0)
    terminated = ~finite | oom
    done = terminated | truncated
    log = bool(p.log_episode_sums)
    eps_in = f64(book["epsum"])[:N_TERMS]
    contrib, contrib_b, reward, reward_b, eps_end, eps_end_b = weigh_rewards(p.weight, T, B, finite, dt, log, eps_in)
    met, met_b = episode_end_metrics(eps_end, eps_end_b, done, truncated, finite, [oom], ep_new)
    rd = reset_draw(p, m, seed, step, gid, field)
    dyn, dyn_b = veh_reset(np.where(finite[None], s[:ACT0], np.nan), done, finite, rd["pos"], rd["pos_b"], rd["q"], rd["q_b"], 0.0)
    act = np.where(done[None], 0.0, f64(action))
    return dict(finite=finite, oom=oom, traversable=trav, terminated=terminated, truncated=truncated, done=done, terms=T, terms_b=B,
                contrib=contrib, contrib_b=contrib_b, reward=reward, reward_b=reward_b, epsum_in=eps_in, epsum_end=eps_end,
                epsum_end_b=eps_end_b, epsum=np.where(done[None], 0.0, eps_end), ep_len=np.where(done, 0, ep_new), ep_len_end=ep_new,
                metrics=met, metrics_b=met_b, reset=rd, dyn=dyn, dyn_b=dyn_b, last_action=act, dt=dt, vb=vb, d_vb=d_vb)


def near_threshold(t):
    """envs a correct fp32 kernel may decide otherwise than this module: none (module docstring)"""
    return np.zeros(t["done"].shape, bool)


def stored_state(t, p):
    """the rows a correct step stores: [S_COUNT, n] float64, a bound of the same shape (0 = exact) and the rows that are held.  With
    log_episode_sums = 0 the WL_S_EPSUM rows are the pre-step ones, untouched"""
    n = t["done"].size
    s, b = np.zeros((S_COUNT, n)), np.zeros((S_COUNT, n))
    s[:ACT0], b[:ACT0] = t["dyn"], t["dyn_b"]
    s[ACT0:ACT0 + 2] = t["last_action"]
    rows = list(range(ACT0 + 2)) + list(range(EPSUM0, EPSUM0 + N_TERMS))
    if p.log_episode_sums:
        s[EPSUM0:EPSUM0 + N_TERMS] = t["epsum"]
        b[EPSUM0:EPSUM0 + N_TERMS] = np.where(t["done"][None], 0.0, t["epsum_end_b"])
    else:
        s[EPSUM0:EPSUM0 + N_TERMS] = t["epsum_in"]
    return s, b, np.array(rows)


def proprio(state, extra=0):
    """the eight proprioceptive values of a STORED state: base_lin_vel | base_ang_vel | last_action clamped -> [n, 8], bound [n, 8]"""
    s = f64(state)
    n = s.shape[1]
    R, mR = rotation(s[QW:QW + 4])
    nb = (N_BODY + extra) * U
    vb, wb = to_body(R, s[VX:VX + 3]), to_body(R, s[WX:WX + 3])
    vb_b = nb * np.einsum("jin,jn->in", mR, np.abs(s[VX:VX + 3]))
    wb_b = nb * np.einsum("jin,jn->in", mR, np.abs(s[WX:WX + 3]))
    return np.concatenate([vb, wb, np.clip(s[ACT0:ACT0 + 2], -1.0, 1.0)]).T, np.concatenate([vb_b, wb_b, np.zeros((2, n))]).T


COUNT_SLOTS = [M_RESETS, M_TIMEOUTS, M_TERM0, M_TERM0 + 1, M_TERM0 + 2, M_TERM0 + 3, M_NONFINITE, M_EPLEN]


def check_step(got, t, p, scale=1.0, extra=0, floor_ulps=0, where="", epsum_rows=True):
    """One stored step against the reference.  got: dict(state [S_COUNT, n] fp32 rows after the step, ep_len [n], prop [n, 8],
    reward [n], terminated, truncated [n] bool, dones [n] or None, metrics [16]: this step's increments, or None); t = tail(...) of
    the same step (extra roundings are given to `tail` by the caller; `extra` here goes to `proprio`).  epsum_rows = False leaves the
    WL_S_EPSUM rows out (the oracle clears them at a reset whatever log_episode_sums says).
    -> (failure strings, excused envs, worst ratio, {element: its worst ratio})."""
    fails, per = [], {}
    near = near_threshold(t)
    live = ~near
    for name in ("terminated", "truncated"):
        d = (np.asarray(got[name]).astype(bool) != t[name]) & live
        if d.any():
            fails.append(f"{where}{name}: {int(d.sum())} decisions differ, first env {int(np.argmax(d))}")
    if got.get("dones") is not None and not np.array_equal(np.asarray(got["dones"]).astype(bool)[live], t["done"][live]):
        fails.append(f"{where}dones is not terminated | truncated")
    per["reward"] = _hold("reward", got["reward"], t["reward"], scale * t["reward_b"], live, fails, where, floor_ulps * _ulp(t["reward"]))
    if not np.array_equal(np.asarray(got["ep_len"])[live], t["ep_len"][live]):
        fails.append(f"{where}ep_len differs: envs {np.nonzero((np.asarray(got['ep_len']) != t['ep_len']) & live)[0][:4].tolist()}")
    st = np.asarray(got["state"])
    want, wb_, rows = stored_state(t, p)
    if not epsum_rows:
        rows = rows[rows < EPSUM0]
    fl = floor_ulps * _ulp(want[rows])
    per["stored state"] = _hold("stored state", st[rows], want[rows], scale * wb_[rows], live[None].repeat(len(rows), 0), fails, where, fl)
    o, o_b = proprio(st, extra)
    per["proprioception"] = _hold("proprioception", f64(got["prop"])[:, :PROP_DIM], o, scale * o_b, live[:, None].repeat(PROP_DIM, 1), fails,
                                  where, floor_ulps * _ulp(o))
    if got.get("metrics") is not None:
        mt = f64(got["metrics"])
        if not np.array_equal(mt[COUNT_SLOTS], t["metrics"][COUNT_SLOTS]):
            fails.append(f"{where}metric counts {mt[COUNT_SLOTS].tolist()} != {t['metrics'][COUNT_SLOTS].tolist()}")
        if (mt[M_EPSUM0 + N_TERMS:M_RESETS] != 0).any():
            fails.append(f"{where}episode-sum metrics of terms the task does not have: {mt[M_EPSUM0 + N_TERMS:M_RESETS].tolist()}")
        k = slice(M_EPSUM0, M_EPSUM0 + N_TERMS)
        per["metric episode sums"] = _hold("metric episode sums", mt[k], t["metrics"][k], scale * t["metrics_b"][k], np.ones(N_TERMS, bool),
                                           fails, where)
    return fails, int(near.sum()), max(per.values()), per


# ---- the cases of tests/test_gpu_visual_tail.py and tests/test_visual_tail_reference_cpu.py -----------------------------------------
N_ENVS, K_STEPS = 288 + 5, 6
MAX_LEN = {"A": 7, "B": 3, "C": 7}
NAN_VX_ENV, INF_PX_ENV, INF_WHEEL_ENV, NAN_STEER_ENV = 101, 202, 150, 77     # 101 and 150 share no quad block; 77 sits in a third
BAD_ENVS = {"A": (NAN_VX_ENV, INF_PX_ENV), "B": (), "C": (NAN_VX_ENV, INF_PX_ENV, INF_WHEEL_ENV, NAN_STEER_ENV)}
N_CLASSES = 10                                                             # staged classes per step (stage_step)
C_WEIGHTS, C_WEIGHTS_SWAPPED, C_SWAP_STEP = (0.0, -3.0), (-4.0, 0.0), 2
_maps = {}


def case_map(tag):
    """the case's map as `travmap`: A the task's 500^2 golden map at 0.5 m; B an asymmetric one-cell pattern, white iff
    (3 ix + 5 iy) mod 7 < 3, 101^2 at (0.3, 0.4); C 80^2 at 0.5 m in blocks of 2 x 3 cells"""
    if tag not in _maps:
        if tag == "A":
            import os
            g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visual_trav.npz"))
            _maps[tag] = travmap(np.unpackbits(g["full_map_packed"])[: 500 * 500].reshape(500, 500).astype(bool), (0.5, 0.5))
        elif tag == "B":
            iy, ix = np.mgrid[:101, :101]
            _maps[tag] = travmap((3 * ix + 5 * iy) % 7 < 3, (0.3, 0.4))
        else:
            iy, ix = np.mgrid[:80, :80]
            _maps[tag] = travmap((3 * (ix // 2) + 5 * (iy // 3)) % 7 < 4, (0.5, 0.5))
    return _maps[tag]


def case_field(tag):
    """the case's heightfield (heightfield_cases.Field) or None on the plane"""
    if tag != "C":
        return None
    import heightfield_cases
    return heightfield_cases.get("G1")


def apply_case(p, tag, k=0):
    """edit a parameter set IN PLACE for step k of a case (the product's ctypes struct or the oracle's namespace: same field names;
    the oracle's also carries the map geometry, as the fp32 spacings the kernel is handed)"""
    p.max_episode_length = MAX_LEN[tag]
    if hasattr(p, "map_rows"):
        m = case_map(tag)
        p.map_rows, p.map_cols, p.row_spacing, p.col_spacing = m.rows, m.cols, float(m.rs), float(m.cs)
    if tag == "C":       # a zero and a negative weight; on one step the pair the other way round, so that the zero weight meets the
        w = C_WEIGHTS_SWAPPED if k == C_SWAP_STEP else C_WEIGHTS          # term a non-finite car leaves NaN (forward_vel)
        p.weight[0], p.weight[1] = w
        p.log_episode_sums = 0 if k == K_STEPS - 1 else 1
    return p


def _terrain_z(tag, x, y):
    fld = case_field(tag)
    if fld is None:
        return np.zeros_like(x)
    from oracle import heightfield as OH
    h, x0, y0, cell, outside = fld.oracle()
    return OH.sample(h, x0, y0, cell, x, y, outside=outside)[0].astype(F)


def stage_step(tag, k, st, ep, n):
    """hand-set rows of step k IN PLACE, on the host copy of the state the step starts from: st [S_COUNT, stride] fp32, ep int32.
    A sixth of the batch is staged per step, in N_CLASSES classes -> the class of every env (-1: not staged):
      0..7  within 0.5 m of the +x, -x, +y, -y border (class // 2), heading along its velocity of 3 m/s outward (even) or inward
            (odd), wheels rolling; the outward cars stand 0.02 .. 0.5 m from the border: some cross it within the step, some do not
      8     as an outward car 5 cm from a border, in the last step of its episode: time-out and out_of_map in the same step
      9     A, B: 10 km outside the map; C: beyond the heightfield's edge (on its outside plane) but inside the map"""
    m = case_map(tag)
    hw, hh = (float(v) for v in half_extent(m))
    e = np.arange(n)
    if k == 0:
        ep[:n] = e % MAX_LEN[tag]                                          # a seventh (B: a third) of the batch times out per step
        if tag == "C":
            st[EPSUM0:EPSUM0 + N_TERMS, :n] = (0.01 * (1 + np.arange(N_TERMS))[:, None] * (1 + e)[None]).astype(F)
    j = e // K_STEPS
    cls = np.where(e % K_STEPS == k, j % N_CLASSES, -1)
    border = (cls >= 0) & (cls <= 8)
    side = np.where(cls == 8, (j // N_CLASSES) % 4, cls // 2)
    outward = (cls % 2 == 0) | (cls == 8)
    d = np.where(cls == 8, 0.05, np.where(outward, 0.02 + 0.48 * ((e * 7919) % 97) / 97.0, 0.25))
    along = np.where(side < 2, hw, hh) - d                                 # the coordinate across the border
    other = ((e * 131) % 61 / 61.0 - 0.5) * np.where(side < 2, hh, hw)      # the one along it: spread over the middle half
    sgn = np.where(side % 2 == 0, 1.0, -1.0)
    x = np.where(side < 2, sgn * along, other)
    y = np.where(side < 2, other, sgn * along)
    dirx, diry = np.where(side < 2, sgn, 0.0) * np.where(outward, 1, -1), np.where(side < 2, 0.0, sgn) * np.where(outward, 1, -1)
    yaw = np.arctan2(diry, dirx)
    far = cls == 9
    if tag == "C":
        fld = case_field(tag)
        x, y = np.where(far, ((e * 37) % 53 / 53.0 - 0.5) * 30.0, x), np.where(far, fld.y0 - 1.0 - (e % 7), y)
    else:
        x = np.where(far, hw + 1.0e4, x)
        y = np.where(far, other, y)
    on = border | far
    z = _terrain_z(tag, x.astype(F), y.astype(F)) + F(0.1)
    st[PX, :n], st[PX + 1, :n] = np.where(on, x, st[PX, :n]).astype(F), np.where(on, y, st[PX + 1, :n]).astype(F)
    st[PX + 2, :n] = np.where(on, z, st[PX + 2, :n]).astype(F)
    q = np.stack([np.cos(0.5 * yaw), 0 * yaw, 0 * yaw, np.sin(0.5 * yaw)])
    st[QW:QW + 4, :n] = np.where(border[None], q, st[QW:QW + 4, :n]).astype(F)
    st[VX, :n], st[VX + 1, :n] = np.where(border, 3.0 * dirx, st[VX, :n]).astype(F), np.where(border, 3.0 * diry, st[VX + 1, :n]).astype(F)
    st[VX + 2, :n] = np.where(border, 0.0, st[VX + 2, :n]).astype(F)
    st[WX:WX + 3, :n] = np.where(border[None], 0.0, st[WX:WX + 3, :n]).astype(F)
    st[WHEEL:WHEEL + 4, :n] = np.where(border[None], 60.0, st[WHEEL:WHEEL + 4, :n]).astype(F)   # 3 m/s on 5 cm wheels
    st[STEER_POS:STEER_POS + 2, :n] = np.where(border[None], 0.0, st[STEER_POS:STEER_POS + 2, :n]).astype(F)
    ep[:n] = np.where(cls == 8, MAX_LEN[tag] - 1, ep[:n])
    bad = BAD_ENVS[tag]
    if bad:                                                                # the non-finite cars, every step
        st[VX, NAN_VX_ENV], st[PX, INF_PX_ENV] = np.nan, np.inf
        cls[[NAN_VX_ENV, INF_PX_ENV]] = -2
    if len(bad) == 4:
        st[WHEEL + 2, INF_WHEEL_ENV], st[STEER_POS, NAN_STEER_ENV] = -np.inf, np.nan
        cls[[INF_WHEEL_ENV, NAN_STEER_ENV]] = -2
    return cls


def case_actions(tag, k, n):
    rng_ = np.random.RandomState(500 + k)
    a = rng_.uniform(-1.2, 1.2, (n, 2)).astype(F)
    a[:, 0] = np.abs(a[:, 0]) * F(0.6) + F(0.2)
    if tag == "C":
        a[::9] *= F(2.5)                                                   # raw actions up to +-3
    return a


EVENTS = {"A": ("resets", "time-outs", "left +x", "left -x", "left +y", "left -y", "stayed +x", "stayed -x", "stayed +y", "stayed -y",
                "time-out and out_of_map", "10 km outside", "non-finite", "spawned on a white cell", "white", "black"),
          "B": ("resets", "time-outs", "left +x", "left -x", "left +y", "left -y", "stayed +x", "stayed -x", "stayed +y", "stayed -y",
                "time-out and out_of_map", "10 km outside", "white", "black"),
          "C": ("resets", "time-outs", "left +x", "left -x", "left +y", "left -y", "stayed +x", "stayed -x", "stayed +y", "stayed -y",
                "time-out and out_of_map", "beyond the field inside the map", "non-finite", "raw action beyond 1", "white", "black",
                "reset onto the terrain", "reset beyond the field")}


def events_of(tag, t, cls, post, raw_action):
    """how often each staged event of the case occurred in one step -> {name: count} over EVENTS[tag]"""
    ev = {"resets": t["done"].sum(), "time-outs": t["truncated"].sum(), "time-out and out_of_map": (t["truncated"] & t["oom"]).sum(),
          "white": (t["terms"][0] > 0).sum(), "black": (t["terms"][0] < 0).sum(), "non-finite": (~t["finite"]).sum()}
    for s, name in enumerate(("+x", "-x", "+y", "-y")):
        staged = (cls == 2 * s) | (cls == 2 * s + 1)
        ev["left " + name], ev["stayed " + name] = (staged & t["oom"]).sum(), (staged & t["finite"] & ~t["oom"]).sum()
    ev["10 km outside"] = ((cls == 9) & t["oom"]).sum()
    m = case_map(tag)
    iy, ix = t["reset"]["cell"]
    with np.errstate(invalid="ignore"):
        pos = t["dyn"][PX:PX + 3]
        ev["spawned on a white cell"] = (t["done"] & m.trav[iy, ix] & traversable(m, pos[0].astype(F), pos[1].astype(F))).sum()
        fld = case_field(tag)
        if fld is not None:
            xl, xh, yl, yh = fld.extent()
            inside = lambda x, y: (x > xl) & (x < xh) & (y > yl) & (y < yh)                      # noqa: E731
            px, py = f64(post[PX]), f64(post[PX + 1])
            ev["beyond the field inside the map"] = (t["finite"] & ~t["oom"] & ~inside(px, py)).sum()
            ev["reset onto the terrain"] = (t["done"] & inside(pos[0], pos[1])).sum()
            ev["reset beyond the field"] = (t["done"] & ~inside(pos[0], pos[1])).sum()
    ev["raw action beyond 1"] = (np.abs(np.asarray(raw_action)) > 1).any(1).sum()
    return {k: int(ev[k]) for k in EVENTS[tag]}

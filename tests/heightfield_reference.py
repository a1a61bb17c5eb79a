"""The terrain samplers restated in float64 -- TEST INFRASTRUCTURE, never imported by the product.  Inputs are what a kernel is handed
(fp32 positions, poses, field placement, decoded fp32 heights); every operation after that is float64, so the only error left in a
comparison is the kernel's.  Two definitions, written down here because they differ at the far border:

  contact samplers (wl_heightfield.h: HeightFieldGround::sample_full, HeightFieldGroundCached, the reset draws) -- `guard=True`:
      u, v are clamped to [0, n - 1 - 1e-3] where the bound is the fp32 value (float)(n - 1) - 1e-3f the device computes, and the
      cell index to n - 2.  On a field 32 770 or more points wide the bound rounds to n - 1 itself: the guard is gone, and only the
      cell clamp (which changes nothing inside the field) keeps the read on the grid.
  height scan (wl_elev_scan_dev.h::scan_cell / scan_value, every scan form) -- `guard=False`: no clamp; the ray's own cell and fraction.

Both are `inside` for u in [0, nx - 1) and v in [0, ny - 1); outside, the contact samplers return outside_z and a +z normal, the scan
a miss (+inf, clipped to obs_clip).  The two agree except within 1e-3 cell of the far border lines, where the guard flattens the
surface: at cell 0.1 m and a border slope of 1 that is 1e-4 m, so the scan must be held to the guard-free definition.

Bounds (derived, not fitted):
  * position: a grid coordinate is formed from metres in a handful of fp32 roundings.  Two of them happen in METRES -- the ray's
    offset added to the root position, the origin subtracted -- and cost half an ulp of those magnitudes each, in cells
    (ulp32(|w|) + ulp32(|w - origin|)) / (2 cell), which is MANY ulps of u where the origin is near the point (u small, |w| large);
    the rest -- the product with the rounded 1 / cell, the ray lattice's two multiply-adds -- half an ulp of u each.  Taken twice
    over: (ulp32(|w|) + ulp32(|w - origin|)) / cell + 4 ulp32(max(|u|, |v|, 1)) cells.  The yaw's cos / sin are fp32 results of a
    handful of roundings (<= 2^-21 each) and turn the ray's lever arm |lx| + |ly| metres: 2^-21 (|lx| + |ly|) / cell more.
  * height: that position error times the steepest slope of the bilinear surface around the point (the 3 x 3 cells about it: the
    error can move the point into a neighbour), plus 2e-5 m for the fp32 blend, scale and the observation's add / subtract.
A ray whose float64 (u, v) lies within the position error of a border line may land on either side: it is excused by that predicate
(counted), never by a count.  Normals jump across cell lines: a contact point within the position error of one is excused for its
normal, and so is its inside flag within the error of a border line."""
import numpy as np

F = np.float32
SCAN_ABS = 2e-5            # m: fp32 blend + scale + the observation's arithmetic (values within +-10 m)
N_RAYS = 26


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F)).astype(np.float64)


def _decoded(field):
    return np.asarray(field.heights, np.float64)


def slope_map(field):
    """[ny - 1, nx - 1] per cell, max over the 3 x 3 cells about it of |dz/dx| + |dz/dy| of the bilinear patch (m / m), and the same of
    its twist |(h11 - h01) - (h10 - h00)| / cell (what moves the normal with the position)"""
    h = _decoded(field)
    dx = np.abs(np.diff(h, axis=1)) / field.cell           # [ny, nx - 1]
    dy = np.abs(np.diff(h, axis=0)) / field.cell           # [ny - 1, nx]
    s = np.maximum(dx[:-1], dx[1:]) + np.maximum(dy[:, :-1], dy[:, 1:])
    t = np.abs((h[1:, 1:] - h[1:, :-1]) - (h[:-1, 1:] - h[:-1, :-1])) / field.cell

    def grow(a):
        p = np.pad(a, 1, mode="edge")
        return np.max([p[j:j + a.shape[0], i:i + a.shape[1]] for j in range(3) for i in range(3)], 0)
    return grow(s), grow(t)


def _uv(field, x, y):
    return ((np.asarray(x, F).astype(np.float64) - field.x0) / field.cell, (np.asarray(y, F).astype(np.float64) - field.y0) / field.cell)


def pos_err(field, wx, wy, lever=0.0):
    """the bound on a device grid coordinate's error, in cells, for world points (wx, wy) reached over a lever arm (module docstring)"""
    wx, wy = np.asarray(wx, np.float64), np.asarray(wy, np.float64)
    u, v = (wx - field.x0) / field.cell, (wy - field.y0) / field.cell
    metres = ulp32(np.maximum(np.abs(wx), np.abs(wy))) + ulp32(np.maximum(np.abs(wx - field.x0), np.abs(wy - field.y0)))
    return metres / field.cell + 4 * ulp32(np.maximum(np.maximum(np.abs(u), np.abs(v)), 1.0)) + 2.0 ** -21 * np.asarray(lever) / field.cell


def _cell_index(field, u, v):
    """the cell whose slope governs (u, v) -- clamped onto the grid"""
    i = np.clip(np.floor(np.nan_to_num(u)), 0, field.nx - 2).astype(np.int64)
    j = np.clip(np.floor(np.nan_to_num(v)), 0, field.ny - 2).astype(np.int64)
    return i, j


def bilinear64(field, u, v, guard):
    """-> z, normal [.., 3], inside for grid coordinates (u, v) in float64 (see the module's two definitions)"""
    h = _decoded(field)
    nx, ny = field.nx, field.ny
    inside = (u >= 0) & (v >= 0) & (u < nx - 1) & (v < ny - 1)
    if guard:
        gu = float(F(nx - 1) - F(1e-3))
        gv = float(F(ny - 1) - F(1e-3))
        uc, vc = np.clip(u, 0, gu), np.clip(v, 0, gv)
    else:
        uc, vc = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    uc, vc = np.nan_to_num(uc), np.nan_to_num(vc)
    i = np.minimum(np.floor(uc), nx - 2).astype(np.int64)
    j = np.minimum(np.floor(vc), ny - 2).astype(np.int64)
    fu, fv = uc - i, vc - j
    h00, h10, h01, h11 = h[j, i], h[j, i + 1], h[j + 1, i], h[j + 1, i + 1]
    a = h00 + fu * (h10 - h00)
    b = h01 + fu * (h11 - h01)
    z = a + fv * (b - a)
    dzdx = ((h10 - h00) + fv * ((h11 - h01) - (h10 - h00))) / field.cell
    dzdy = (b - a) / field.cell
    n = np.stack([-dzdx, -dzdy, np.ones_like(z)], -1)
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    z = np.where(inside, z, field.outside_z)
    n = np.where(inside[..., None], n, np.array([0.0, 0.0, 1.0]))
    return z, n, inside


def sample64(field, x, y, guard=True):
    """bilinear height and unit normal of the decoded grid at fp32 world points (x, y) -> z, n [.., 3], inside"""
    u, v = _uv(field, x, y)
    return bilinear64(field, u, v, guard)


def contact_bounds(field, x, y, lever=0.0):
    """per point: (z tolerance m, normal tolerance, position error in cells, excuse-normal, excuse-inside) of a contact sampler"""
    u, v = _uv(field, x, y)
    pos = pos_err(field, np.asarray(x, F), np.asarray(y, F), lever)
    s, t = slope_map(field)
    i, j = _cell_index(field, u, v)
    hmax = float(np.abs(field.heights).max())
    ztol = 4 * ulp32(hmax) + s[j, i] * field.cell * pos
    ntol = 1e-6 + 8 * ulp32(hmax) / field.cell + t[j, i] * pos
    near_line = (np.abs(u - np.rint(u)) <= pos) | (np.abs(v - np.rint(v)) <= pos)
    guard_u, guard_v = float(F(field.nx - 1) - F(1e-3)), float(F(field.ny - 1) - F(1e-3))
    near_guard = (np.abs(u - guard_u) <= pos) | (np.abs(v - guard_v) <= pos)     # the clamp's kink, inside the last cell
    near_border = _near_border(field, u, v, pos)
    return ztol, ntol, pos, near_line | near_guard | near_border, near_border


def _near_border(field, u, v, pos):
    lu, lv = field.nx - 1, field.ny - 1
    in_u = (u >= -pos) & (u <= lu + pos)
    in_v = (v >= -pos) & (v <= lv + pos)
    return (((np.abs(u) <= pos) | (np.abs(u - lu) <= pos)) & in_v) | (((np.abs(v) <= pos) | (np.abs(v - lv) <= pos)) & in_u)


def scan_rays(p, state):
    """-> (world x, world y) [n, 676] float64 of the rays of every env (x fastest), their lever arms |lx| + |ly| [676], from the pose
    rows of the SoA state (root position 0..2, quaternion w x y z 3..6) in float64"""
    st = np.asarray(state, F).astype(np.float64)
    w, qx, qy, qz = st[3], st[4], st[5], st[6]
    a = 1.0 - 2.0 * (qy * qy + qz * qz)
    b = 2.0 * (w * qz + qx * qy)
    r = np.sqrt(a * a + b * b)
    c, s = a / r, b / r
    g = float(F(-0.5) * F(p.scan_size)) + np.arange(N_RAYS) * float(F(p.scan_res))
    lx, ly = np.tile(g, N_RAYS), np.repeat(g, N_RAYS)
    wx = st[0][:, None] + c[:, None] * lx[None] - s[:, None] * ly[None]
    wy = st[1][:, None] + s[:, None] * lx[None] + c[:, None] * ly[None]
    return wx, wy, np.abs(lx) + np.abs(ly)


def scan64(p, state, field):
    """the 26 x 26 height scan of `state`'s poses over `field` in float64 -> (value [n, 676], tolerance [n, 676] m, excused [n, 676]).
    value: -(pz - hz - scan_offset) + (pz - elev_z0) = hz + scan_offset - elev_z0 on a hit, +inf on a miss, clipped to +-obs_clip.
    excused: rays within the position error of a border line (hit or miss either way; a hit is then held to `tolerance` of the
    surface continued to the border)"""
    wx, wy, lever = scan_rays(p, state)
    u, v = (wx - field.x0) / field.cell, (wy - field.y0) / field.cell
    hz, _, inside = bilinear64(field, u, v, guard=False)
    clip = float(F(p.obs_clip))
    val = np.where(inside, hz + float(F(p.scan_offset)) - float(F(p.elev_z0)), np.inf)
    val = np.clip(val, -clip, clip)
    pos = pos_err(field, wx, wy, lever[None])
    s, _ = slope_map(field)
    i, j = _cell_index(field, u, v)
    tol = SCAN_ABS + s[j, i] * field.cell * pos
    excused = _near_border(field, u, v, pos)
    # the excused rays' value if they land inside: the surface at the nearest point of the grid (within `pos` of theirs)
    uc = np.clip(u, 0, field.nx - 1 - 1e-9)
    vc = np.clip(v, 0, field.ny - 1 - 1e-9)
    hz_edge, _, _ = bilinear64(field, uc, vc, guard=False)
    edge_val = np.clip(hz_edge + float(F(p.scan_offset)) - float(F(p.elev_z0)), -clip, clip)
    return val, tol, excused, edge_val


def check_scan(got, p, state, field, where=""):
    """hold a device scan [n, 676] to scan64 -> number of excused rays (printed by the caller).  Every ray not excused: equal misses,
    hits within the tolerance.  Excused rays: a miss, or a hit within the tolerance of the surface at the border."""
    val, tol, ex, edge_val = scan64(p, state, field)
    got = np.asarray(got, np.float64)
    miss_ref, miss_got = val == float(F(p.obs_clip)), got == float(F(p.obs_clip))
    err = np.abs(got - val)
    hit_ok = err <= tol
    bad = ~ex & ~hit_ok
    if bad.any():
        k = np.argwhere(bad)[0]
        raise AssertionError(f"{where}: {int(bad.sum())} ray(s) off the float64 scan; first env {k[0]} ray {k[1]}: got {got[tuple(k)]!r}, "
                             f"want {val[tuple(k)]!r} +- {tol[tuple(k)]:.3g} (miss ref {bool(miss_ref[tuple(k)])}, got {bool(miss_got[tuple(k)])})")
    ex_ok = miss_got | (np.abs(got - edge_val) <= tol)
    assert (ex_ok | ~ex).all(), (where, int((ex & ~ex_ok).sum()))
    return int(ex.sum())

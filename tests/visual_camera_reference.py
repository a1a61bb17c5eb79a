"""The visual task's grey camera (wl_visual_cam_dev.h::render_image) restated in float64 -- TEST INFRASTRUCTURE, never imported by the product.
Inputs are what the kernel is handed (fp32 pose rows, fp32 intrinsics and augmentation values, the byte map, the fp32 spacing), widened
to float64; every operation after that is float64, so the only error left in a comparison is the kernel's.  Two stages:

GEOMETRY -- `classes()`: one of {BLACK, WHITE, SKY} per pixel of the cropped 40 x 80 image.
    R    = I + 2 [..] of the quaternion as given (mat_from_quat's polynomial: no renormalisation)
    o    = pos + R cam_pos
    d    = R (1, -(col + 0.5 - cx) / fx, -(row + 0.5 - cy) / fy),   row = 20 .. 59 of the full image
    sky  = not (d_z < -1e-6f)
    t    = -o_z / d_z;   h = o + t d          (no t > 0 test: a camera below the plane sees the plane behind it, as the kernel does)
    on   = |h_x| <= N s / 2 and |h_y| <= N s / 2
    cell = clamp(trunc((h + N s / 2 + s / 2) / s), 0, N - 1) per axis (TraversabilityHashmapUtil.get_map_id), value map[yi, xi]
    class = sky ? SKY : (on and value ? WHITE : BLACK)
`acceptable()` says per pixel which classes a correct fp32 kernel may answer: the classes met in the box hit +- e_pos in x and in y (cell
lines, the map's edge, the upper index clamp: black off the map, and the cells of the box's part on the map counted in a summed-area table,
so a far pixel over uniform ground keeps ONE class however wide its box), and all three when |d_z + 1e-6| <= e_dir.  `check_explained()`
demands that every kernel pixel is in its set: zero unexplained, the ambiguous ones counted.

The two bounds, counted from render_image (eps = 2^-24, half an ulp relative; `rcp` is the 1-ulp hardware reciprocal: 2 eps; the rows of
R are |q|^2 long, 1 for the fp32-normalised quaternions of the tests; L = sqrt(1 + dy^2 + max_row dz^2) >= |d|):

    value                     operations                                                    bound
    R entry                   fl(w a2) or fl(1 - fl(a a2)), then one fma; magnitudes <= 1   3 eps                       (absolute)
    o                         dot(): 3 roundings of <= |cam|_1, entries 3 eps |cam|_1,      eps (|o|_max + 6 |cam|_1)   = e_o
                              the add to pos
    dy, dz0                   rcp(fx | fy) 2 eps, (col + .5) - cx 1, the product 1          4 eps                       (relative)
    d after the fma3 set-up   two fma: 2 eps L;  entries: 3 eps (1 + |dy| + |dz|);          eps (2 L + 3 (1 + |dy| + |dz|) + 4 sqrt(dy^2 + dz^2))
                              dy / dz0: 4 eps |dy c1_i + dz0 c2_i| <= 4 eps sqrt(dy^2 + dz^2)
    dstep                     kstep = fl(-3 rcp(fy)) 3 eps, the product 1, the entry 3      7 eps |kstep|,  |kstep| = 3 / fy
    d after k <= 13 adds      k dstep errors, k roundings of |d| <= L                       eps k (L + 21 / fy)
      => e_dir = eps ((2 + k) L + 3 (1 + |dy| + |dz|_max) + 4 sqrt(dy^2 + dz_max^2) + 21 k / fy),  k = (row - 20) // 3
         (31 eps in the middle of the bottom row, 42 eps at its corners, at the default intrinsics)
    t = -o_z rcp(d_z)         rcp 2 eps, product 1, d_z's own error amplified by            |t| (3 eps + e_dir / dzl) + e_o / dzl,
                              1 / |d_z|, o_z's by the same                                   dzl = |d_z| - e_dir  = e_t
    h = fma(t, d, o)          e_t |d_i| + (|t| + e_t) e_dir + e_o, the fma's rounding       ... + eps |h_i|
    u = fma(h, inv, off inv)  inv = rcp(s) 2 eps on |h| / s = A;  off = fl(.5 fl(N s) + .5 s) eps (3 A + 6 M) cells,  M = N / 2 + 0.5
                              2 eps, off inv: + 2 eps + 1 = 5 eps on M;  the fma 1 on A + M
    half extent .5 fl(N s)    one rounding                                                  eps N s / 2
      => e_pos (metres, per axis) = e_h + s eps (3 A + 6 M) + eps N s / 2
That is C eps (|o| + |t| |d| (1 + |d| / |d_z|)) with C between 20 and 45 (a first guess before counting was 40).  Nothing in the table is
fitted to a kernel's output: it was checked against this float64 statement and the CPU emulations only.

Measured on the case lists of tests/visual_camera_cases.py (tests/test_visual_camera_reference_cpu.py prints them; the MI355X gave the
same counts): ambiguous pixels per case of 204 800 -- golden map 0 - 6 (<= 2.9e-5, at most 2 in one image; level, tilted, flipped,
0.05 - 5 m and below the plane, map border, shifted intrinsics); one-cell pattern 2 - 97 (<= 4.7e-4, at most 10 in one image) -- against a
cap of 1e-3 per case and 16 per image.  The fp32 emulation differs from float64 in 0 - 4 pixels per case, the MI355X kernel in 0 - 10,
every one of them ambiguous.  Stage 2: the emulation's worst pixel sits at 0.09 of its bound.

CHAIN -- `chain(p, classes)`: the augmentation from a class image, as torchvision defines it (oracle/visual_step.camera), no shortcut:
    v = 0 | 1 | sky;  brightness(x) = clip(b x, 0, 1);  contrast(x) = clip(c x + (1 - c) 0.9999f mean(x), 0, 1)
    x = contrast(brightness(v))  or, contrast_first, brightness(contrast(v));   GaussianBlur(5, sigma) with reflect padding when sigma > 0
    (weights exp(-(j / sigma)^2 / 2) / sum, rows of the image first then columns);   out = (0.9999f x - 0.5) / 0.5
Every step is monotone and 1-Lipschitz in the pixel values (the clamps included), so an error passes through without a branch to
excuse.  Bound per pixel, operations counted from render_image's longest path (contrast > 1 or contrast first: no fold):
    the mean's share    14 in-lane adds + 6 shuffle adds + 4 over the wavefronts = 24, x 0.9999f, x fl(1 / 3200) (2), 1 - c, the product: 29
                        roundings on |cm| = |(1 - c) mean| (x b when the brightness product follows), x 2 in the output
    the pixel's share   the brightness product 1, the blend's fma 1, the second brightness product or the folded blend 1, 2 x 5 taps 10,
                        x 0.9999f and - 0.5 2: 15 roundings on m = 2 W(m_x) + 1, m_x = c a + |cm| the blend's first-order magnitude
                        (x max(b, 1) when the brightness product follows) and W the maximum over the pixel's reflected 5 x 5 window
                        (the identity without blur);  3 roundings on the plain path
    the weights         e_j = __expf(a_j), a_j = -q^2 / 2 with q = j / sigma correctly rounded: 3 eps |a_j| from the argument,
                        (2 + 1.173 |a_j|) ulp = CUDA's documented bound for __expf (the hardware exp2 of a rounded product is inside it),
                        2^-126 for a flushed denormal; the sum 5 eps, the division 1, the product 1:
                        dW = sum_j w_j (rho_j + sum_i rho_i w_i + 7 eps), twice (two passes), x 2 in the output, on W(m_x)
    bound = eps (2 x 29 |cm| + 15 m) + 4 dW W(m_x)                                          (~ 1e-6 - 4e-6 for values in [0, 1])

PROPRIOCEPTION -- `tail()`: R^T v, R^T w (mul_t: 3 roundings + the entries' 3 eps each: 6 eps |v|_1) and clip(last action, -1, 1), exact.
"""
import numpy as np

F = np.float32
EPS = 2.0 ** -24
IMG_H, IMG_W, CROP = 40, 80, 20
N_PIX = IMG_H * IMG_W
BLACK, WHITE, SKY = 0, 1, 2
SKY_DZ = float(F(-1e-6))
GREY = float(F(0.9999))
ROWS_PER_PASS = 3                      # render_image: 256 threads = 3 image rows per pass, d advanced by dstep between passes
MEAN_OPS, PIXEL_OPS, PLAIN_OPS = 29, 15, 3


def _w(x):
    """an fp32 input widened"""
    return np.asarray(x, F).astype(np.float64)


def intrinsics(p):
    return dict(cx=float(F(p.cx)), cy=float(F(p.cy)), fx=float(F(p.fx)), fy=float(F(p.fy)), cam=_w(list(p.cam_pos)), sky=float(F(p.sky)))


def rot64(quat):
    """[n, 4] (w, x, y, z) -> [n, 3, 3] body -> world, mat_from_quat's polynomial on the quaternion as given"""
    q = _w(quat)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def geometry(p, pos, quat):
    """-> dict: R [n,3,3], o [n,3], d [n,40,80,3], dy [80], dz [40], hit [n,40,80], t, hx, hy [n,40,80] (t = 0 where not hit)"""
    k = intrinsics(p)
    R = rot64(quat)
    o = _w(pos) + R @ k["cam"]
    dy = -((np.arange(IMG_W) + 0.5 - k["cx"]) / k["fx"])
    dz = -((np.arange(CROP, CROP + IMG_H) + 0.5 - k["cy"]) / k["fy"])
    db = np.stack([np.ones((IMG_H, IMG_W)), np.broadcast_to(dy[None, :], (IMG_H, IMG_W)), np.broadcast_to(dz[:, None], (IMG_H, IMG_W))], -1)
    d = np.einsum("nij,rcj->nrci", R, db)
    hit = d[..., 2] < SKY_DZ
    with np.errstate(all="ignore"):
        t = np.where(hit, -o[:, None, None, 2] / np.where(hit, d[..., 2], -1.0), 0.0)
        hx = o[:, None, None, 0] + t * d[..., 0]
        hy = o[:, None, None, 1] + t * d[..., 1]
    return dict(R=R, o=o, d=d, dy=dy, dz=dz, hit=hit, t=t, hx=hx, hy=hy, quat=np.asarray(quat, F))


def ground_class(trav, spacing, hx, hy):
    """BLACK / WHITE of plane points in float64: on_map, then get_map_id's cell and map[yi, xi]"""
    trav = np.asarray(trav, bool)
    n, s = trav.shape[0], float(F(spacing))
    half = n * s / 2
    with np.errstate(all="ignore"):
        on = (np.abs(hx) <= half) & (np.abs(hy) <= half)
        xi = np.clip(np.trunc(np.nan_to_num((hx + half + s / 2) / s, nan=0.0, posinf=1e18, neginf=-1e18)), 0, n - 1).astype(np.int64)
        yi = np.clip(np.trunc(np.nan_to_num((hy + half + s / 2) / s, nan=0.0, posinf=1e18, neginf=-1e18)), 0, n - 1).astype(np.int64)
    return np.where(on & trav[yi, xi], WHITE, BLACK).astype(np.int8)


def classes(p, trav, spacing, pos, quat, geom=None):
    """[n, 40, 80] int8 in {BLACK, WHITE, SKY}"""
    g = geom or geometry(p, pos, quat)
    return np.where(g["hit"], ground_class(trav, spacing, g["hx"], g["hy"]), SKY).astype(np.int8)


def error_bounds(p, trav, spacing, geom):
    """-> (e_x, e_y [n,40,80] metres: how far a correct kernel's hit may lie from the float64 one, inf where it cannot be said;
    e_dir [n,40,80]: the same for a ray direction's component) -- the module docstring's table"""
    k = intrinsics(p)
    n, s = np.asarray(trav).shape[0], float(F(spacing))
    o, d, t = geom["o"], geom["d"], geom["t"]
    cam1 = np.abs(k["cam"]).sum()
    e_o = EPS * (np.abs(o).max(-1) + 6 * cam1)[:, None, None]
    ady, dzm = np.abs(geom["dy"])[None, :], np.abs(geom["dz"]).max()
    L = np.sqrt(1 + ady ** 2 + dzm ** 2)
    kk = (np.arange(IMG_H) // ROWS_PER_PASS)[:, None]
    e_dir = EPS * ((2 + kk) * L + 3 * (1 + ady + dzm) + 4 * np.sqrt(ady ** 2 + dzm ** 2) + 7 * ROWS_PER_PASS * kk / k["fy"])
    e_dir = e_dir[None] * np.maximum(1.0, (_w(geom["quat"]) ** 2).sum(-1))[:, None, None]     # rows of R: |q|^2 long
    with np.errstate(all="ignore"):
        dzl = np.abs(d[..., 2]) - e_dir
        ok = geom["hit"] & (dzl > 0)
        dzl = np.where(ok, dzl, 1.0)
        e_t = np.abs(t) * (3 * EPS + e_dir / dzl) + e_o / dzl
        M = n / 2 + 0.5
        out = []
        for i, h in ((0, geom["hx"]), (1, geom["hy"])):
            e_h = e_t * np.abs(d[..., i]) + (np.abs(t) + e_t) * e_dir + e_o + EPS * np.abs(h)
            e = e_h + s * EPS * (3 * np.abs(h) / s + 6 * M) + EPS * n * s / 2
            out.append(np.where(ok & np.isfinite(e), e, np.inf))
    return out[0], out[1], e_dir


def box_classes(trav, spacing, hx, hy, ex, ey):
    """-> (black, white) bool: the ground classes met in the box [hx - ex, hx + ex] x [hy - ey, hy + ey] -- off the map (black), and the
    cells of the box's part on the map, counted in a summed-area table (e may be infinite: the whole plane)"""
    trav = np.asarray(trav, bool)
    n, s = trav.shape[0], float(F(spacing))
    half = n * s / 2
    sat = np.zeros((n + 1, n + 1), np.int64)
    sat[1:, 1:] = trav.cumsum(0).cumsum(1)
    with np.errstate(all="ignore"):
        lo_x, hi_x, lo_y, hi_y = hx - ex, hx + ex, hy - ey, hy + ey
        off = ~((lo_x >= -half) & (hi_x <= half) & (lo_y >= -half) & (hi_y <= half))          # (a NaN is off the map too)
        some = (hi_x >= -half) & (lo_x <= half) & (hi_y >= -half) & (lo_y <= half)

        def idx(v):
            v = np.clip(np.nan_to_num(v, nan=0.0, posinf=half, neginf=-half), -half, half)
            return np.clip(np.trunc((v + half + s / 2) / s), 0, n - 1).astype(np.int64)
        x0, x1, y0, y1 = idx(lo_x), idx(hi_x), idx(lo_y), idx(hi_y)
    white = sat[y1 + 1, x1 + 1] - sat[y0, x1 + 1] - sat[y1 + 1, x0] + sat[y0, x0]
    area = (x1 - x0 + 1) * (y1 - y0 + 1)
    return off | (some & (white < area)), some & (white > 0)


def acceptable(p, trav, spacing, pos, quat, geom=None):
    """[n, 40, 80, 3] bool: the classes a correct fp32 kernel may answer for each pixel"""
    g = geom or geometry(p, pos, quat)
    ex, ey, e_dir = error_bounds(p, trav, spacing, g)
    acc = np.zeros(g["t"].shape + (3,), bool)
    near_sky = np.abs(g["d"][..., 2] - SKY_DZ) <= e_dir
    hit = g["hit"]
    acc[..., SKY] = ~hit | near_sky
    black, white = box_classes(trav, spacing, g["hx"], g["hy"], ex, ey)
    acc[..., BLACK] = (hit & black) | near_sky        # a ray the kernel takes for a hit at the threshold lands anywhere
    acc[..., WHITE] = (hit & white) | near_sky
    return acc


def ambiguous(acc):
    return acc.sum(-1) > 1


def check_explained(got_classes, acc, nominal=None, where=""):
    """every pixel's class must be in its acceptable set -> (ambiguous pixels, pixels that differ from the nominal class)"""
    got = np.asarray(got_classes).astype(np.int64)
    ok = np.take_along_axis(acc, got[..., None], -1)[..., 0]
    if not ok.all():
        bad = np.argwhere(~ok)
        e, r, c = bad[0]
        raise AssertionError(f"{where}: {len(bad)} unexplained pixel(s) in {len(np.unique(bad[:, 0]))} image(s); first: env {e} row {r} col {c} "
                             f"got class {got[e, r, c]}, acceptable {np.flatnonzero(acc[e, r, c]).tolist()}"
                             + ("" if nominal is None else f", float64 class {nominal[e, r, c]}"))
    differ = 0 if nominal is None else int((got != nominal).sum())
    return int(ambiguous(acc).sum()), differ


def class_values(p, cls):
    return np.where(cls == SKY, float(F(p.sky)), (cls == WHITE).astype(np.float64))


def blur_weights(sigma):
    j = np.arange(-2, 3, dtype=np.float64)
    e = np.exp(-0.5 * (j / float(F(sigma))) ** 2)
    return e / e.sum()


def weights_error(sigma):
    """sum_j of the bound on |w_j(kernel) - w_j| (module docstring: the weights)"""
    j = np.arange(-2, 3, dtype=np.float64)
    a = 0.5 * (j / float(F(sigma))) ** 2
    e = np.exp(-a)
    w = e / e.sum()
    rho = EPS * 3 * a + 2 * EPS * (2 + 1.173 * a) + 2.0 ** -126 / np.maximum(e, 1e-300) * (e < 2.0 ** -126)
    rho = np.minimum(rho, 1.0)
    return float((w * (rho + (rho * w).sum() + 7 * EPS)).sum())


def _reflect_windows(x, axis):
    pad = [(0, 0)] * x.ndim
    pad[axis] = (2, 2)
    xp = np.pad(x, pad, mode="reflect")
    n = x.shape[axis]
    return [np.take(xp, np.arange(j, j + n), axis=axis) for j in range(5)]


def blur(x, w):
    """separable 5-tap correlation with reflect padding: along the columns of a row (axis 2), then along the rows (axis 1)"""
    for axis in (2, 1):
        x = sum(wj * xj for wj, xj in zip(w, _reflect_windows(x, axis)))
    return x


def window_max(x):
    for axis in (2, 1):
        x = np.max(_reflect_windows(x, axis), 0)
    return x


def chain(p, cls, with_bound=False):
    """the augmentation chain on class images [n, 40, 80] -> [n, 40, 80] float64 (and the per-pixel bound)"""
    b, c, sigma, cfirst = float(F(p.brightness)), float(F(p.contrast)), float(F(p.blur_sigma)), bool(getattr(p, "contrast_first", 0))
    v = class_values(p, np.asarray(cls))

    def brightness(x):
        return np.clip(x * b, 0.0, 1.0)

    def contrast(x):
        cm = (1.0 - c) * (GREY * x.mean((1, 2), keepdims=True))
        return np.clip(c * x + cm, 0.0, 1.0), cm
    if cfirst:
        x, cm = contrast(v)
        m_x = (c * v + np.abs(cm)) * max(b, 1.0)
        cm = cm * b
        x = brightness(x)
    else:
        a = brightness(v)
        x, cm = contrast(a)
        m_x = c * a + np.abs(cm)
    blurred = sigma > 0.0
    if blurred:
        x = blur(x, blur_weights(sigma))
    out = (x * GREY - 0.5) / 0.5
    if not with_bound:
        return out
    if c == 1.0 and not blurred:
        return out, np.full(out.shape, PLAIN_OPS * EPS * 2.0)
    wm = window_max(m_x) if blurred else m_x
    dW = weights_error(sigma) if blurred else 0.0
    return out, EPS * (2 * MEAN_OPS * np.abs(cm) + PIXEL_OPS * (2 * wm + 1)) + 4 * dW * wm


def tail(quat, lin_vel, ang_vel, last_action):
    """-> ([n, 8] float64, bound [n, 8]): base_lin_vel, base_ang_vel (body frame), last action clipped to +-1"""
    R = rot64(quat)
    v, w = _w(lin_vel), _w(ang_vel)
    vb, wb = np.einsum("nji,nj->ni", R, v), np.einsum("nji,nj->ni", R, w)
    act = np.clip(_w(last_action), -1.0, 1.0)
    bv = 6 * EPS * np.abs(v).sum(-1, keepdims=True) * np.ones(3)
    bw = 6 * EPS * np.abs(w).sum(-1, keepdims=True) * np.ones(3)
    return np.concatenate([vb, wb, act], -1), np.concatenate([bv, bw, np.zeros_like(act)], -1)

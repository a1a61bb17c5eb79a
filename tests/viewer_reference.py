"""Numpy restatement of the viewer camera (wheeledlab_amd/csrc/wl_viewer_dev.h, include/wheeledlab_amd_viewer.h) in float64 -- TEST
INFRASTRUCTURE, never imported by the product.  Heightfield ground depth comes from oracle.depth.depth() (the exact walk, pinned
pixel for pixel to the depth kernel); the plane, the trav-map / checker albedo, the car hits (chassis box + four wheel spheres), the
tie rule (nearest; at equal distance a car beats the ground and the lower env id beats a higher one) and the shading are stated
here.  Cars are only tested on the pixels of their projected bounding sphere (with a margin), which is what keeps 4096 cars cheap."""
import numpy as np

from oracle import depth as OD
from oracle.mathlib import matrix_from_quat

SKY = np.array([0.62, 0.76, 0.92])
CHECKER = np.array([[0.56, 0.56, 0.52], [0.40, 0.41, 0.38]])
TRAV = np.array([[0.16, 0.16, 0.17], [0.86, 0.86, 0.84]])
WHEEL = np.array([0.10, 0.10, 0.11])
HIGHLIGHT = np.array([1.00, 0.84, 0.10])
PALETTE = np.array([[0.85, 0.20, 0.18], [0.18, 0.45, 0.85], [0.20, 0.70, 0.30], [0.80, 0.45, 0.10],
                    [0.60, 0.25, 0.75], [0.10, 0.70, 0.70], [0.85, 0.35, 0.60], [0.55, 0.55, 0.20]])
F32 = np.float32


def _camera(p):
    q = np.array(list(p.cam_quat), np.float32)[None]
    R = matrix_from_quat(q).astype(np.float64)[0]
    o = np.array(list(p.cam_pos), np.float64)
    H, W = p.height, p.width
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    db = np.stack([np.ones_like(rows), -((cols + 0.5 - p.cx) / p.fx), -((rows + 0.5 - p.cy) / p.fy)], -1)
    return o, R, db @ R.T          # [H, W, 3] world directions (body x component 1)


def trav_albedo(m, row_spacing, col_spacing, x, y, with_bit=False):
    """the map lookup of wl_visual_env.h::map_id in float32 (truncation toward zero, clamp); with_bit: also the traversability bit"""
    rows, cols = m.shape
    rs, cs = F32(row_spacing), F32(col_spacing)
    width, height = F32(rows) * rs, F32(cols) * cs
    fx = (F32(x) + F32(0.5) * width + F32(0.5) * rs) / rs
    fy = (F32(y) + F32(0.5) * height + F32(0.5) * cs) / cs
    xi = np.clip(np.trunc(np.clip(np.nan_to_num(fx, nan=-1.0), -1, rows)), 0, rows - 1).astype(np.int64)
    yi = np.clip(np.trunc(np.clip(np.nan_to_num(fy, nan=-1.0), -1, cols)), 0, cols - 1).astype(np.int64)
    bit = (m[yi, xi] != 0).astype(np.int64)
    return (TRAV[bit], bit) if with_bit else TRAV[bit]


def checker_albedo(size, x, y, with_bit=False):
    with np.errstate(invalid="ignore"):
        k = np.floor(x / size) + np.floor(y / size)
    bit = np.where(np.isfinite(k) & (np.abs(k) < 1.6e7), np.nan_to_num(k).astype(np.int64) & 1, 0)
    return (CHECKER[bit], bit) if with_bit else CHECKER[bit]


def field_normal(hf, x, y):
    h, x0, y0, cell = hf[:4]
    h = np.asarray(h, np.float64)
    ny, nx = h.shape
    u, v = (x - x0) / cell, (y - y0) / cell
    inside = (u >= 0) & (v >= 0) & (u < nx - 1) & (v < ny - 1)
    uc, vc = np.clip(u, 0, nx - 1 - 1e-3), np.clip(v, 0, ny - 1 - 1e-3)
    i, j = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
    fu, fv = uc - i, vc - j
    h00, h10, h01, h11 = h[j, i], h[j, i + 1], h[j + 1, i], h[j + 1, i + 1]
    a, b = h00 + fu * (h10 - h00), h01 + fu * (h11 - h01)
    dzdx = ((h10 - h00) + fv * ((h11 - h01) - (h10 - h00))) / cell
    dzdy = (b - a) / cell
    n = np.stack([-dzdx, -dzdy, np.ones_like(dzdx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[~inside] = (0.0, 0.0, 1.0)
    return n


def geometry(p):
    wheels = np.array([[p.half_wheelbase_f, p.half_track, p.wheel_z], [p.half_wheelbase_f, -p.half_track, p.wheel_z],
                       [-p.half_wheelbase_r, p.half_track, p.wheel_z], [-p.half_wheelbase_r, -p.half_track, p.wheel_z]], np.float64)
    bc, bh = np.array(list(p.box_center), np.float64), np.array(list(p.box_half), np.float64)
    r = max(np.linalg.norm(bc) + np.linalg.norm(bh), max(np.linalg.norm(w) + p.wheel_radius for w in wheels))
    return bc, bh, wheels, float(p.wheel_radius), r * 1.001 + 1e-4


def _car_hits(ol, dl, bc, bh, wheels, wr):
    """ray (local) -> (t [m] or inf, part: 4 box / 0..3 wheel / -1, local normal [m, 3], box face entered: 2 axis + (dl[axis] > 0))"""
    m = ol.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(dl != 0, 1.0 / np.where(dl != 0, dl, 1.0), 1e30)
        a_, b_ = (-bh - (ol - bc)) * inv, (bh - (ol - bc)) * inv
    lo, hi = np.minimum(a_, b_), np.maximum(a_, b_)
    axis = np.argmax(lo, 1)
    tn, tf = lo.max(1), hi.min(1)
    t = np.where((tn > 0) & (tn <= tf), tn, np.inf)
    part = np.where(np.isfinite(t), 4, -1)
    n = np.zeros((m, 3))
    pos_dir = dl[np.arange(m), axis] > 0
    n[np.arange(m), axis] = np.where(pos_dir, -1.0, 1.0)
    face = 2 * axis + pos_dir
    a = (dl * dl).sum(1)
    for w, c in enumerate(wheels):
        oc = ol - c
        b = (dl * oc).sum(1)
        cc = (oc * oc).sum(1) - wr * wr
        disc = b * b - a * cc
        ok = (disc >= 0) & (cc > 0) & (b < 0)
        tw = np.where(ok, cc / (np.sqrt(np.maximum(disc, 0)) - b + (~ok)), np.inf)
        better = ok & (tw > 0) & (tw < t)
        t = np.where(better, tw, t)
        part = np.where(better, w, part)
        with np.errstate(invalid="ignore"):
            n = np.where(better[:, None], (ol + tw[:, None] * dl - c) / wr, n)
    face = np.where(part == 4, face, -1)
    return t, part, n, face


def tie_reach(t):
    """the depth-tie window: a surface whose hit lies within this distance of the best one's may win the pixel in fp32"""
    return t * (1 + 1e-5) + 1e-6


def _scene(p, pos, quat, hf=None, trav=None, dx=0.0, dy=0.0, field_t=None):
    """the frame with the principal point shifted by (dx, dy) pixels, and per pixel: the colour key [H, W, 4] (id, part: 4 box /
    0..3 wheel / -1 ground or sky, box face entered or -1, albedo cell), the runner-up surface (t2, id2): the nearest of every
    other car, the ground (also just beyond the far clip) and the sky at the far clip, and the heightfield's distance field_t
    (given: used as it is)"""
    if dx or dy:
        p = type(p).from_buffer_copy(p)
        p.cx, p.cy = p.cx + dx, p.cy + dy
    H, W, far = p.height, p.width, float(p.far_clip)
    reach = tie_reach(far)
    o, Rc, d = _camera(p)
    # ground
    if field_t is not None:
        tg = field_t
    elif hf is not None:
        from types import SimpleNamespace
        cam = SimpleNamespace(cam_pos=(0.0, 0.0, 0.0), fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy)
        ext = float(np.nextafter(np.float32(reach), np.float32(np.inf)))     # the walk runs on a little: a ground just beyond the clip
        tg = OD.depth(cam, np.array(list(p.cam_pos), np.float32)[None], np.array(list(p.cam_quat), np.float32)[None], hf[:4], ext,
                      outside_z=hf[4], img_h=H, img_w=W)[0].astype(np.float64)
        tg = np.where(tg < ext, tg, np.inf)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            tg = np.where(o[2] <= p.plane_z, 0.0, np.where(d[..., 2] < 0, (p.plane_z - o[2]) / d[..., 2], np.inf))
    hit = tg < far
    best_t = np.where(hit, tg, far)
    best_id = np.where(hit, -1, -2).astype(np.int32)
    sec_t = np.where(hit, far, tg)
    sec_id = np.where(hit, -2, -1).astype(np.int32)
    x, y = o[0] + best_t * d[..., 0], o[1] + best_t * d[..., 1]
    normal = field_normal(hf, x, y) if hf is not None else np.broadcast_to([0.0, 0.0, 1.0], (H, W, 3)).copy()
    if trav is not None:
        albedo, bit = trav_albedo(trav[0], trav[1], trav[2], x, y, with_bit=True)
    else:
        albedo, bit = checker_albedo(p.checker, x, y, with_bit=True)
    albedo = np.where(hit[..., None], albedo, SKY)
    cell = bit.astype(np.int64)
    if hf is not None:
        ny, nx = np.asarray(hf[0]).shape
        with np.errstate(invalid="ignore"):
            u, v = (x - hf[1]) / hf[3], (y - hf[2]) / hf[3]
        inside = (u >= 0) & (v >= 0) & (u < nx - 1) & (v < ny - 1)
        ij = np.where(inside, np.floor(np.where(inside, v, 0)) * (nx - 1) + np.floor(np.where(inside, u, 0)), -1).astype(np.int64)
        cell = 2 * (ij + 1) + cell
    cell = np.where(hit, cell, -1)
    part = np.full((H, W), -1, np.int64)
    face = np.full((H, W), -1, np.int64)
    # cars, in id order: a strictly nearer hit wins, so at equal distance the lower id keeps the pixel; a car at the ground's distance wins
    bc, bh, wheels, wr, rb = geometry(p)
    pos = np.asarray(pos, np.float64)
    Rs = matrix_from_quat(np.asarray(quat, np.float32)).astype(np.float64)
    fwd, right, down = Rc[:, 0], -Rc[:, 1], -Rc[:, 2]
    for e in range(pos.shape[0]):
        rel = pos[e] - o
        z, xr, yd = rel @ fwd, rel @ right, rel @ down
        if not (z + rb > 0 and z - rb < reach):
            continue
        if z - rb > 1e-3:
            us = [(xr + s * rb) / (z + q * rb) for s in (-1, 1) for q in (-1, 1)]
            vs = [(yd + s * rb) / (z + q * rb) for s in (-1, 1) for q in (-1, 1)]
            c0, c1 = int(np.floor(p.fx * min(us) + p.cx - 0.5)) - 2, int(np.ceil(p.fx * max(us) + p.cx - 0.5)) + 2
            r0, r1 = int(np.floor(p.fy * min(vs) + p.cy - 0.5)) - 2, int(np.ceil(p.fy * max(vs) + p.cy - 0.5)) + 2
            c0, c1, r0, r1 = max(c0, 0), min(c1, W - 1), max(r0, 0), min(r1, H - 1)
            if c0 > c1 or r0 > r1:
                continue
        else:
            c0, c1, r0, r1 = 0, W - 1, 0, H - 1
        sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        shp = best_t[sl].shape
        dd = d[sl].reshape(-1, 3)
        R = Rs[e]
        ol = np.broadcast_to((o - pos[e]) @ R, dd.shape)
        dl = dd @ R
        t, cpart, nl, cface = _car_hits(ol, dl, bc, bh, wheels, wr)
        bt, bi = best_t[sl].reshape(-1), best_id[sl].reshape(-1)
        st, si = sec_t[sl].reshape(-1), sec_id[sl].reshape(-1)
        win = (cpart >= 0) & (t < far) & ((t < bt) | ((t == bt) & (bi < 0)))
        second = ~win & (cpart >= 0) & ((t < st) | ((t == st) & (si < 0)))
        if not (win.any() or second.any()):
            continue
        sec_t[sl] = np.where(win, bt, np.where(second, t, st)).reshape(shp)
        sec_id[sl] = np.where(win, bi, np.where(second, e, si)).reshape(shp)
        if not win.any():
            continue
        gid = e + p.id_offset
        col = HIGHLIGHT if gid == p.env_index else PALETTE[gid % len(PALETTE)]
        alb = np.where((cpart == 4)[:, None], col, WHEEL)
        nw = nl @ R.T
        best_t[sl] = np.where(win, t, bt).reshape(shp)
        best_id[sl] = np.where(win, e, bi).reshape(shp)
        normal[sl] = np.where(win[:, None], nw, normal[sl].reshape(-1, 3)).reshape(normal[sl].shape)
        albedo[sl] = np.where(win[:, None], alb, albedo[sl].reshape(-1, 3)).reshape(albedo[sl].shape)
        part[sl] = np.where(win, cpart, part[sl].reshape(-1)).reshape(shp)
        face[sl] = np.where(win, cface, face[sl].reshape(-1)).reshape(shp)
        cell[sl] = np.where(win, -1, cell[sl].reshape(-1)).reshape(shp)
    sun = np.array(list(p.sun), np.float64)
    sun /= np.linalg.norm(sun)
    k = np.where(best_id == -2, 1.0, p.ambient + (1 - p.ambient) * np.maximum((normal * sun).sum(-1), 0.0))
    rgb = np.clip(np.floor(k[..., None] * albedo * 255 + 0.5), 0, 255).astype(np.uint8)
    key = np.stack([best_id.astype(np.int64), part, face, cell], -1)
    return dict(rgb=rgb, depth=best_t.astype(np.float32), id=best_id, key=key, t2=sec_t, id2=sec_id, field_t=tg if hf is not None else None)


def render(p, pos, quat, hf=None, trav=None):
    """p: WlViewerParams; pos [N, 3], quat [N, 4] (w, x, y, z) float32 of the cars; hf: (heights [ny, nx], x0, y0, cell, outside_z)
    for heightfield ground (plane z = p.plane_z otherwise); trav: (map [rows, cols], row_spacing, col_spacing) or None (checker)
    -> rgb uint8 [H, W, 3], depth float32 [H, W], id int32 [H, W]"""
    s = _scene(p, pos, quat, hf, trav)
    return s["rgb"], s["depth"], s["id"]


# The silhouette excuse's principal-point shift [px].  Measured on the host build of wl_viewer_dev.h (tests/test_viewer_host_cpu.py
# ::test_fp32_ray_spread_is_below_delta, all seven host scenes, built once with -ffp-contract=off and once with -ffp-contract=fast as
# hipcc compiles device code): a shift of 1e-4 px explains every pixel (fp32 rounding of the ray, the camera and car rotations and the
# car-relative origin, ~1e-7 relative, times fx ~ 1e2 .. 1e3 px).  That is the host compiler's rounding of the same source, not the
# device's own instructions; the device frames are held at DELTA by the GPU tests and pass there.  DELTA leaves a factor of 10.
DELTA = 1e-3


def acceptable(p, pos, quat, hf=None, trav=None, delta=DELTA):
    """What a correct fp32 kernel may answer at each pixel, decided from the float64 reference's own state (never from a count):

    - silhouette: any id the reference shows at the pixel with the principal point shifted by +-delta pixels in x or in y (car edges,
      the horizon, sky or ground at the far clip).  delta = DELTA = 1e-3 px by default, ten times the fp32 spread the host build of the
      device functions shows (see DELTA); it may not be larger than 1e-3 px.
    - depth tie: along the nominal ray, the runner-up surface (another car, the ground, the sky at the far clip) when its hit lies
      within tie_reach(t_best) = t_best (1 + 1e-5) + 1e-6: a wheel sphere touching the plane, two cars with identical poses.
    - colour: the key (id, part, box face, albedo cell: checker parity / traversability bit / heightfield cell) of each render; colour
      is held to 2 LSB wherever the key is the same in all five renders, unless a depth tie let another surface than the nominal win.
    - grazing (heightfield ground): ground or sky pixels whose depth depth_cases.mismatch calls grazing against oracle.depth.  The
      shifted renders keep the nominal heightfield distance (the walk's own sub-pixel edges are what this predicate covers), which
      keeps a 1280 x 720 terrain frame to one oracle.depth call; cars and the plane are shifted.

    -> dict for check_explained"""
    assert 0.0 <= delta <= 1e-3, "the silhouette excuse may not grow beyond 1e-3 px"
    shifts = ((0.0, 0.0), (delta, 0.0), (-delta, 0.0), (0.0, delta), (0.0, -delta))
    sc = [_scene(p, pos, quat, hf, trav)]
    sc += [_scene(p, pos, quat, hf, trav, dx, dy, sc[0]["field_t"]) for dx, dy in shifts[1:]]
    nom = sc[0]
    tie = nom["t2"] <= tie_reach(nom["depth"].astype(np.float64))
    key_same = np.ones(nom["id"].shape, bool)
    for s in sc[1:]:
        key_same &= (s["key"] == nom["key"]).all(-1)
    return dict(nominal=(nom["rgb"], nom["depth"], nom["id"]), ids=np.stack([s["id"] for s in sc]),
                depths=np.stack([s["depth"] for s in sc]).astype(np.float64), tie=tie, t2=nom["t2"], id2=nom["id2"], key_same=key_same,
                field=hf is not None, far=float(p.far_clip))


def check_explained(got, acc, what="", depth_tol=(2e-4, 2e-4), lsb=2):
    """Zero unexplained pixels: every pixel's id is acceptable (acceptable()); its depth is within depth_tol of that surface's distance
    (the nominal one, that id's distance in a shifted render, or the runner-up's); its colour within `lsb` wherever it is not excused.
    -> the numbers of excused pixels by kind (printed)"""
    rg, dg, ig = (np.asarray(a) for a in got)
    rw, dw, iw = acc["nominal"]
    ids, depths, tie = acc["ids"], acc["depths"], acc["tie"]
    dg64 = dg.astype(np.float64)

    def near(t):
        return np.abs(dg64 - t) <= depth_tol[0] + depth_tol[1] * np.abs(t)

    id_ok = (ids == ig).any(0)
    by_tie = tie & (acc["id2"] == ig)
    id_ok |= by_tie
    depth_ok = ((ids == ig) & near(depths)).any(0) | (by_tie & near(acc["t2"]))
    grazing = np.zeros_like(id_ok)
    if acc["field"]:
        # the ground walk against the double oracle: rays grazing a crest (depth_cases.mismatch, as the terrain test uses it)
        import depth_cases as DC
        bad, _ = DC.mismatch(dg, dw, acc["far"])
        grazing = (iw < 0) & (ig < 0) & ~(id_ok & depth_ok) & bad
    explained = (id_ok & depth_ok) | grazing
    colour_held = acc["key_same"] & ~(tie & (ig != iw)) & ~grazing       # a tie excuses colour only where another surface won
    cerr = np.abs(rg.astype(np.int32) - rw.astype(np.int32)).max(-1)
    colour_bad = colour_held & (cerr > lsb)
    counts = dict(n=int(ig.size), silhouette=int((~(ids == ids[0]).all(0)).sum()), tie=int(tie.sum()),
                  colour_excused=int((~colour_held).sum()), grazing=int(grazing.sum()), other_id=int((ig != iw).sum()),
                  unexplained=int((~explained).sum()), colour_bad=int(colour_bad.sum()))
    print("explained", what, counts)
    if counts["unexplained"] or counts["colour_bad"]:
        r, c = np.nonzero(~explained | colour_bad)
        ex = [(int(a), int(b), int(ig[a, b]), float(dg[a, b]), int(iw[a, b]), float(dw[a, b]), ids[:, a, b].tolist(), int(acc["id2"][a, b]),
               float(acc["t2"][a, b]), tuple(rg[a, b]), tuple(rw[a, b])) for a, b in list(zip(r, c))[:8]]
        raise AssertionError(f"{what}: {counts}; first (row, col, id, depth, ref id, ref depth, ids, id2, t2, rgb, ref rgb): {ex}")
    return counts


def compare(got, want, depth_tol=(2e-4, 2e-4), lsb=2):
    """(rgb, depth, id) pairs -> dict: share of pixels whose ids agree, and on those the worst depth / colour error beyond the bounds"""
    (rg, dg, ig), (rw, dw, iw) = got, want
    same = ig == iw
    derr = np.abs(dg.astype(np.float64) - dw.astype(np.float64))
    dbad = same & (derr > depth_tol[0] + depth_tol[1] * np.abs(dw.astype(np.float64)))
    cbad = same & (np.abs(rg.astype(np.int32) - rw.astype(np.int32)).max(-1) > lsb)
    return dict(id_match=float(same.mean()), depth_bad=int(dbad.sum()), colour_bad=int(cbad.sum()), n=int(same.size))

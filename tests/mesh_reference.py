"""Float64 restatement of the mesh rasteriser (include/wheeledlab_amd_terrain.h, csrc/wl_terrain.hip) and the predicate the device
heights are held to.

`rasterize` evaluates the header's contract straight: for every face with a valid index triple, finite vertices and non-zero
projected area, every lattice point of its bounding box is tested against the closed triangle and takes the largest plane height;
`fill_z` where nothing covers it.  Lattice point (i, j) is at float64(float32 x0) + i * float64(float32 cell), as the header says.

`acceptable(h, ...)` is the predicate: a (point, face) pair is MARGINAL when the point lies within `MARGIN` (1 nm) of the face's
closed triangle boundary -- inside by at most 1 nm or outside by at most 1 nm, measured as a float64 distance to an edge line.  At a
point with marginal pairs any maximum over the DEFINITELY covering faces plus a non-empty subset of the marginal ones is accepted; the
empty subset (`fill_z` where no face definitely covers the point) only where one of the near edges is a boundary edge of the mesh
(one face only), so that a hole along an edge two faces share is never excused.  Everywhere else |h - h_ref| <= 1e-6 m * max(1,
|h_ref|).  Excused points are counted and printed."""
from __future__ import annotations

import numpy as np

MARGIN = 1e-9
RTOL = 1e-6
PAIRS_PER_PASS = 1 << 22


def lattice_axes(x0, y0, cell, nx, ny):
    c = np.float64(np.float32(cell))
    return np.float64(np.float32(x0)) + np.arange(nx) * c, np.float64(np.float32(y0)) + np.arange(ny) * c


def _faces_ok(v, f):
    """valid faces (index triple in range, finite vertices) and their float64 corners [F, 3, 3]"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    v = np.asarray(v, np.float32).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    tri = np.zeros((f.shape[0], 3, 3))
    tri[ok] = v[f[ok]].astype(np.float64)
    ok &= np.isfinite(tri).all((1, 2))
    return ok, tri


def _edge_keys(tri):
    """per face and edge (ab, bc, ca) a hashable key of its endpoint coordinates in lexicographic order"""
    keys = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        pa, pb = tri[:, a, :2], tri[:, b, :2]
        swap = (pb[:, 0] < pa[:, 0]) | ((pb[:, 0] == pa[:, 0]) & (pb[:, 1] < pa[:, 1]))
        lo, hi = np.where(swap[:, None], pb, pa), np.where(swap[:, None], pa, pb)
        keys.append(np.concatenate([lo, hi], 1))
    return keys


def _passes(tri, x0, y0, cell, nx, ny, pad):
    """yields (face ids, ii, jj) of the (face, lattice point) pairs of every face's bounding box widened by `pad` metres, in passes
    of at most PAIRS_PER_PASS pairs (a face larger than that alone, in bands of rows)"""
    c = np.float64(np.float32(cell))
    ox, oy = np.float64(np.float32(x0)), np.float64(np.float32(y0))
    lo, hi = tri[:, :, :2].min(1) - pad, tri[:, :, :2].max(1) + pad
    i0 = np.clip(np.floor((lo[:, 0] - ox) / c), 0, nx).astype(np.int64)
    i1 = np.clip(np.ceil((hi[:, 0] - ox) / c), -1, nx - 1).astype(np.int64)
    j0 = np.clip(np.floor((lo[:, 1] - oy) / c), 0, ny).astype(np.int64)
    j1 = np.clip(np.ceil((hi[:, 1] - oy) / c), -1, ny - 1).astype(np.int64)
    w, h = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    n = w * h
    ids = np.nonzero(n > 0)[0]
    big = ids[n[ids] > PAIRS_PER_PASS]
    small = ids[n[ids] <= PAIRS_PER_PASS]
    cum = np.cumsum(n[small])
    start = 0
    while start < small.size:
        stop = int(np.searchsorted(cum, (cum[start - 1] if start else 0) + PAIRS_PER_PASS, side="right"))
        stop = max(stop, start + 1)
        sel = small[start:stop]
        cnt = n[sel]
        rep = np.repeat(np.arange(sel.size), cnt)
        k = np.arange(rep.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        yield sel[rep], i0[sel][rep] + k % w[sel][rep], j0[sel][rep] + k // w[sel][rep]
        start = stop
    for t in big:
        band = max(1, PAIRS_PER_PASS // int(w[t]))
        for jb in range(int(j0[t]), int(j1[t]) + 1, band):
            jj, ii = np.meshgrid(np.arange(jb, min(jb + band, int(j1[t]) + 1)), np.arange(i0[t], i1[t] + 1), indexing="ij")
            yield np.full(ii.size, t), ii.ravel(), jj.ravel()


def _evaluate(tri, area, fid, ii, jj, xs, ys):
    """signed distances (inside positive) of the points to the three edge lines of their faces [3, P], and the plane heights [P]"""
    t = tri[fid]
    s = np.sign(area[fid])
    px, py = xs[ii], ys[jj]
    e, d = [], []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ex, ey = t[:, b, 0] - t[:, a, 0], t[:, b, 1] - t[:, a, 1]
        ev = s * (ex * (py - t[:, a, 1]) - ey * (px - t[:, a, 0]))
        e.append(ev)
        d.append(ev / np.hypot(ex, ey))
    e_ab, e_bc, e_ca = e
    wsum = e_ab + e_bc + e_ca
    z = (e_bc * t[:, 0, 2] + e_ca * t[:, 1, 2] + e_ab * t[:, 2, 2]) / np.where(wsum == 0, 1.0, wsum)
    return np.stack(d), z


def _prepare(vertices, faces):
    """the faces the contract rasterises (valid, non-zero projected area): corners [F', 3, 3] and twice their signed areas"""
    ok, tri = _faces_ok(vertices, faces)
    area = (tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 1, 1] - tri[:, 0, 1]) * (tri[:, 2, 0] - tri[:, 0, 0])
    ok &= area != 0
    return tri[ok], area[ok]


def rasterize(vertices, faces, x0, y0, cell, nx, ny, fill_z=0.0, *, reduce="max", closed=True):
    """the header's contract in float64 -> heights float64 [ny, nx].  `reduce` / `closed` exist for the modelled defects only
    (reduce="min": the lowest surface; closed=False: open triangles, the points on every edge left out)"""
    tri, area = _prepare(vertices, faces)
    xs, ys = lattice_axes(x0, y0, cell, nx, ny)
    init = -np.inf if reduce == "max" else np.inf
    out = np.full(nx * ny, init)
    for fid, ii, jj in _passes(tri, x0, y0, cell, nx, ny, 0.0):
        d, z = _evaluate(tri, area, fid, ii, jj, xs, ys)
        cov = (d >= 0).all(0) if closed else (d > 0).all(0)
        (np.maximum if reduce == "max" else np.minimum).at(out, (jj * nx + ii)[cov], z[cov])
    out[~np.isfinite(out)] = fill_z
    return out.reshape(ny, nx)


def acceptable(h, vertices, faces, x0, y0, cell, nx, ny, fill_z=0.0, *, label="", verbose=True):
    """-> bool [ny, nx]: where `h` is an answer the contract allows (module docstring); prints the count of excused points"""
    h = np.asarray(h, np.float64).reshape(ny, nx)
    tri, area = _prepare(vertices, faces)
    xs, ys = lattice_axes(x0, y0, cell, nx, ny)
    # boundary edges: endpoint pairs that belong to one face only
    keys = _edge_keys(tri)
    allk = np.concatenate(keys, 0) if tri.shape[0] else np.zeros((0, 4))
    _, inv, cnt = np.unique(allk, axis=0, return_inverse=True, return_counts=True)
    boundary = (cnt[inv.ravel()] == 1).reshape(3, -1) if tri.shape[0] else np.zeros((3, 0), bool)
    hi_def = np.full(nx * ny, -np.inf)
    m_idx, m_z, m_bnd = [], [], []
    for fid, ii, jj in _passes(tri, x0, y0, cell, nx, ny, 2 * MARGIN):
        d, z = _evaluate(tri, area, fid, ii, jj, xs, ys)
        dmin = d.min(0)
        flat = jj * nx + ii
        sure = dmin > MARGIN
        np.maximum.at(hi_def, flat[sure], z[sure])
        marg = (dmin >= -MARGIN) & ~sure
        if marg.any():
            near = np.abs(d[:, marg]) <= MARGIN
            m_idx.append(flat[marg])
            m_z.append(z[marg])
            m_bnd.append((near & boundary[:, fid[marg]]).any(0))
    h = h.ravel()
    has_def = np.isfinite(hi_def)
    want = np.where(has_def, hi_def, fill_z)
    close = lambda a, b: np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b))  # noqa: E731
    ok = close(h, want)
    excusable = np.zeros(nx * ny, bool)
    if m_idx:
        mi, mz, mb = np.concatenate(m_idx), np.concatenate(m_z), np.concatenate(m_bnd)
        excusable[mi] = True
        # a marginal face's height: accepted where it would be the maximum (not below the definite ones)
        cand = mz >= np.where(has_def[mi], hi_def[mi], -np.inf) - RTOL * np.maximum(1.0, np.abs(mz))
        hit = np.zeros(nx * ny, bool)
        hit[mi[cand & close(h[mi], mz)]] = True
        # no face definitely covers the point and every marginal one is marginal: fill only next to a boundary edge
        fill_ok = np.zeros(nx * ny, bool)
        fill_ok[mi[mb]] = True
        no_fill = excusable & ~has_def & ~fill_ok
        ok = np.where(no_fill, hit, ok | hit)
    if verbose:
        print(f"[mesh_reference]{' ' + label if label else ''}: {int((excusable & ok).sum())} of {nx * ny} points excused as "
              f"marginal, {int((~ok).sum())} unacceptable")
    return ok.reshape(ny, nx)


def triangulate_grid(height, x0, y0, cell, alternate=True, xs=None, ys=None):
    """a lattice of heights [ny, nx] -> (vertices float32 [nx * ny, 3], faces int32 [2 (nx - 1) (ny - 1), 3]): vertex (i, j) at
    (x0 + i cell, y0 + j cell) computed in float64 and rounded to float32 (or at xs[i], ys[j]); each cell split along a diagonal
    that alternates in a checkerboard (or always the same one)"""
    h = np.asarray(height)
    ny, nx = h.shape
    if xs is None:
        xs = np.float64(x0) + np.arange(nx) * np.float64(cell)
    if ys is None:
        ys = np.float64(y0) + np.arange(ny) * np.float64(cell)
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    v = np.stack([X.ravel(), Y.ravel(), h.ravel()], 1).astype(np.float32)
    j, i = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    a = (j * nx + i).ravel()
    b, c, d = a + 1, a + nx, a + nx + 1
    flip = ((i + j) % 2 == 1).ravel() if alternate else np.zeros(a.size, bool)
    f1 = np.where(flip[:, None], np.stack([a, b, d], 1), np.stack([a, b, c], 1))
    f2 = np.where(flip[:, None], np.stack([a, d, c], 1), np.stack([b, d, c], 1))
    return v, np.concatenate([f1, f2]).astype(np.int32)


def bridge():
    """a ground square at z 0 and a deck at z 1 over its middle third (an overhang: the deck is a separate surface)"""
    v = np.array([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0],
                  [-1.1, -3.3, 1], [1.1, -3.3, 1], [1.1, 3.3, 1], [-1.1, 3.3, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return v, f


def box_on_plane():
    """a 2 x 2 m box 0.5 m tall with vertical walls (zero-area faces) on a plane at z 0; its edges lie on lattice lines of 0.25 m"""
    v = [[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]]
    f = [[0, 1, 2], [0, 2, 3]]
    lo = [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]]
    hi = [[x, y, 0.5] for x, y, _ in lo]
    v += lo + hi
    f += [[8, 9, 10], [8, 10, 11]]                 # the top
    for k in range(4):                             # the walls, both windings
        a, b = 4 + k, 4 + (k + 1) % 4
        f += [[a, b, b + 4], [a, b + 4, a + 4]] if k % 2 else [[b, a, b + 4], [b + 4, a, a + 4]]
    return np.array(v, np.float32), np.array(f, np.int32)

"""Integer restatement of the flat-patch finder and the deal (include/wheeledlab_amd_terrain.h, csrc/wl_flat_patch_dev.h): numpy over
the SAME WlPatchTile rows and parameters the kernel takes.  Written from the header's rule, not from the device code: every attempt
of a slot at once (no rounds, no lanes), the draws from terrain_gen_reference's Philox4x32, indices and codes in int64.  The only
floats are the three of a result, one fp32 rounding each: x = x0 + fl(i * cell), z = fl(code * z_scale).

`find(codes, tiles, n_patches, seed)` -> (ij int64 [T, P, 2], tries int32 [T, P]); `outputs` -> what the kernel stores for them."""
import numpy as np

import terrain_gen_reference as TR

TS_PATCH, TS_PATCH_DEAL = 14, 15


def below(word, n):
    """a 32-bit word reduced to [0, n): the high half of word * n"""
    return ((np.asarray(word, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def disc(radius_cells: int, radius2: int):
    dj, di = np.mgrid[-radius_cells:radius_cells + 1, -radius_cells:radius_cells + 1]
    m = di * di + dj * dj <= radius2
    return di[m], dj[m]


def accepted(codes, T, i, j):
    """the acceptance test of attempts centred on (i, j) (arrays): bool"""
    ny, nx = codes.shape
    di, dj = disc(int(T["radius_cells"]), int(T["radius2"]))
    c = codes.astype(np.int64)[np.clip(j[:, None] + dj, 0, ny - 1), np.clip(i[:, None] + di, 0, nx - 1)]
    lo, hi = c.min(1), c.max(1)
    return (hi - lo <= int(T["max_diff_codes"])) & (lo >= int(T["z_lo_code"])) & (hi <= int(T["z_hi_code"]))


def attempts(T, t, k, n, seed, stream=TS_PATCH):
    """the centres attempts 0 .. n - 1 of slot k of tile t test"""
    x = TR.philox(t, k, np.arange(n), stream, seed)
    return int(T["i_lo"]) + below(x[0], int(T["i_hi"]) - int(T["i_lo"]) + 1), int(T["j_lo"]) + below(x[1], int(T["j_hi"]) - int(T["j_lo"]) + 1)


def find(codes, tiles, n_patches, seed, stream=TS_PATCH, max_tries=None):
    """max_tries: override every tile's own (an int)"""
    ij = np.zeros((len(tiles), n_patches, 2), np.int64)
    tries = np.full((len(tiles), n_patches), -1, np.int32)
    for t, T in enumerate(tiles):
        n = int(T["max_tries"]) if max_tries is None else int(max_tries)
        for k in range(n_patches):
            ij[t, k] = (int(T["i_lo"]) + int(T["i_hi"])) // 2, (int(T["j_lo"]) + int(T["j_hi"])) // 2
            if n > 0:
                i, j = attempts(T, t, k, n, seed, stream)
                ok = accepted(codes, T, i, j)
                if ok.any():
                    a = int(np.argmax(ok))
                    ij[t, k], tries[t, k] = (i[a], j[a]), a
    return ij, tries


def outputs(codes, ij, x0, y0, cell, z_scale):
    """-> (xy float32 [T, P, 2], z float32 [T, P]): each product rounded to fp32 before the sum"""
    f = np.float32
    i, j = ij[..., 0], ij[..., 1]
    xy = np.stack([f(x0) + i.astype(f) * f(cell), f(y0) + j.astype(f) * f(cell)], -1).astype(f)
    return xy, (codes[j, i].astype(f) * f(z_scale)).astype(f)


def deal(gid, cols, world_envs, n_patches, epoch, seed):
    """type[e] of global env ids `gid`: the column's block of n_patches virtual columns + a slot from Philox(gid, epoch, DEAL)"""
    gid = np.asarray(gid, np.int64)
    w = TR.philox(gid, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, TS_PATCH_DEAL, seed)[0]
    return ((gid * cols // world_envs) * n_patches + below(w, n_patches)).astype(np.int32)

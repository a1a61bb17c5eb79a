"""Float64 / integer restatement of the procedural-terrain generator (include/wheeledlab_amd_terrain.h, csrc/wl_terrain_gen_dev.h):
numpy over the whole lattice from the SAME WlTerrainGenParams fields and tile table the kernel takes.  Written from the header's
formulas, not from the device code: integer quantities in int64, the three continuous forms in float64, the draws from a Philox4x32
of its own (vectorised over counters; tests pin it to oracle.philox).

`reference(params, tiles)` -> Reference: `t` the height of every point in CODE units before the final rounding (t = h64 / z_scale
for the float64 height h64), `exact` where t is an integer by construction (stairs, obstacles, per-cell noise, border), `e` the fp32
evaluation bound of the point's formula in codes, `tile` the tile index (-1: border).

The fp32 bounds (eps = 2^-24: one correctly rounded fp32 operation, relative; the device's a / b is budgeted at 1 ulp = 2 eps):
  sloped      off = slope * d: d an exact small integer, slope the SAME float32 in both, one product rounding:
              e = eps * |off|
  noise,      fu, fv one division each (2 eps); p, q: |fu error| * |l10 - l00| <= 2 eps * 2 H, + the fma's eps * H (H = the largest
  bilinear    |level|); q - p: both errors + eps * 2 H; the last fma: |q - p error| + |fv error| * 2 H + |p error| + eps * H
              = (16 + 6) eps H:  e = 22 * eps * H; but 0 where the spacing D is a power of two and 2 H D^2 < 2^24: fu, fv
              are then k / D exactly and no operation rounds (half-integer heights, common there, are ties both sides break to even)
  wave        x = 2 m / n in [0, 2): 2 eps * 2; through sinpi / cospi: pi * 2^-22 each; the device library documents sinpif and
              cospif at 1 ulp, budgeted here at 2 ulp of a value <= 1: 2^-22 each; their sum: 2 (pi + 1) 2^-22 + eps * 2; times the
              amplitude A: + eps * 2 A:  e = A * (2 pi + 3) * 2^-22
None of them comes from a device run."""
from dataclasses import dataclass

import numpy as np

TT_RANDOM_UNIFORM, TT_PYRAMID_SLOPED, TT_PYRAMID_STAIRS, TT_DISCRETE_OBSTACLES, TT_WAVE = range(5)
TF_INVERTED = 1
TS_UNIFORM, TS_OBSTACLES = 11, 12
EPS = 2.0 ** -24
_M = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, seed, rounds=7):
    """Philox4x32 on broadcastable counter arrays, key = the seed's words -> uint64 arrays (32-bit values) x 4"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) & _M for c in (c0, c1, c2, c3)))
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & _M, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & _M
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


@dataclass
class Reference:
    t: np.ndarray        # float64 [ny, nx]: code units, clamped to +-32767
    exact: np.ndarray    # bool: an integer by construction
    e: np.ndarray        # float64: fp32 evaluation bound, codes
    tile: np.ndarray     # int64: tile index, -1 on the border

    @property
    def codes(self):
        return np.rint(self.t).astype(np.int16)

    def near_half(self):
        """points of the continuous forms whose t lies within e of a half-integer: where an fp32 evaluation may round the other way"""
        return ~self.exact & (self.e > 0) & (np.abs(np.abs(self.t - np.floor(self.t)) - 0.5) <= self.e)     # (e = 0: the fp32 value is t)


def _ring(P, T, u, v):
    side = min(P["tile_nx"], P["tile_ny"])
    d_plat = max((side - int(T["platform"])) // 2, 0)
    return np.minimum(np.minimum(np.minimum(u, P["tile_nx"] - 1 - u), np.minimum(v, P["tile_ny"] - 1 - v)), d_plat)


def _tile(P, T, t, u, v):
    """-> (offset float64, exact bool, e float64) on the tile's local grids u, v (int64, broadcast)"""
    kind, sgn = int(T["type"]), -1 if int(T["flags"]) & TF_INVERTED else 1
    zero = np.zeros(np.broadcast(u, v).shape)
    if kind == TT_RANDOM_UNIFORM:
        n, lo, step, D = int(T["n_levels"]), int(T["code_lo"]), int(T["step_codes"]), int(T["step_cells"])

        def level(a, b):
            return (lo + step * (philox(t, a, b, TS_UNIFORM, P["seed"])[0] % np.uint64(n)).astype(np.int64)).astype(np.float64)
        if D == 1:
            return level(u, v) + zero, True, zero
        a, b = u // D, v // D
        fu, fv = (u - a * D) / D, (v - b * D) / D
        p = level(a, b) + fu * (level(a + 1, b) - level(a, b))
        q = level(a, b + 1) + fu * (level(a + 1, b + 1) - level(a, b + 1))
        H = max(abs(lo), abs(lo + step * (n - 1)))
        # a power-of-two spacing makes fu, fv dyadic (k / D) and every operation above exact in fp32 while 2 H D^2 < 2^24: the
        # fp32 value IS t, ties included (both sides round half to even)
        dyadic = D & (D - 1) == 0 and 2 * H * D * D < 2 ** 24
        return p + fv * (q - p), False, zero + (0.0 if dyadic else 22 * EPS * H)
    if kind == TT_PYRAMID_SLOPED:
        off = float(np.float32(T["slope"])) * _ring(P, T, u, v).astype(np.float64)
        return sgn * off, False, EPS * np.abs(off)
    if kind == TT_PYRAMID_STAIRS:
        return (sgn * int(T["step_codes"]) * (_ring(P, T, u, v) // int(T["step_cells"]))).astype(np.float64), True, zero
    if kind == TT_DISCRETE_OBSTACLES:
        lo, hi, n = int(T["size_lo"]), int(T["size_hi"]), int(T["n_levels"])
        off = np.zeros(np.broadcast(u, v).shape, np.int64)
        for k in range(int(T["n_obstacles"])):
            x = [int(w) for w in philox(t, k, 0, TS_OBSTACLES, P["seed"])]
            w, l = lo + (x[0] & 0xFFFF) % (hi - lo + 1), lo + (x[0] >> 16) % (hi - lo + 1)
            pu, pv = x[1] % (P["tile_nx"] - w + 1), x[2] % (P["tile_ny"] - l + 1)
            inside = (u >= pu) & (u < pu + w) & (v >= pv) & (v < pv + l)
            off = np.where(inside, int(T["code_lo"]) + int(T["step_codes"]) * (x[3] % n), off)
        plat = int(T["platform"])
        pu0, pv0 = (P["tile_nx"] - plat) // 2, (P["tile_ny"] - plat) // 2
        on_platform = (u >= pu0) & (u < pu0 + plat) & (v >= pv0) & (v < pv0 + plat)
        return np.where(on_platform, 0, off).astype(np.float64), True, zero
    if kind == TT_WAVE:
        nw, A = int(T["num_waves"]), float(np.float32(T["amplitude"]))
        xu, xv = 2.0 * ((nw * u) % P["tile_nx"]) / P["tile_nx"], 2.0 * ((nw * v) % P["tile_ny"]) / P["tile_ny"]
        return A * (np.sin(np.pi * xu) + np.cos(np.pi * xv)), False, zero + abs(A) * (2 * np.pi + 3) * 2.0 ** -22
    raise ValueError(f"tile type {kind}")


def reference(params: dict, tiles) -> Reference:
    """params: the WlTerrainGenParams fields (nx, ny, tile_nx, tile_ny, border, rows, cols, base_code, seed); tiles: the table"""
    P = {k: int(params[k]) for k in ("nx", "ny", "tile_nx", "tile_ny", "border", "rows", "cols", "base_code", "seed")}
    assert P["nx"] == P["rows"] * P["tile_nx"] + 2 * P["border"] and P["ny"] == P["cols"] * P["tile_ny"] + 2 * P["border"]
    ny, nx = P["ny"], P["nx"]
    off, exact, e = np.zeros((ny, nx)), np.ones((ny, nx), bool), np.zeros((ny, nx))
    tile = np.full((ny, nx), -1, np.int64)
    u, v = np.arange(P["tile_nx"], dtype=np.int64)[None, :], np.arange(P["tile_ny"], dtype=np.int64)[:, None]
    for r in range(P["rows"]):
        for c in range(P["cols"]):
            t = r * P["cols"] + c
            i0, j0 = P["border"] + r * P["tile_nx"], P["border"] + c * P["tile_ny"]
            sl = (slice(j0, j0 + P["tile_ny"]), slice(i0, i0 + P["tile_nx"]))
            off[sl], exact[sl], e[sl] = _tile(P, tiles[t], t, u, v)
            tile[sl] = t
    return Reference(np.clip(P["base_code"] + off, -32767, 32767), exact, e, tile)


def check_codes(codes, ref: Reference, label=""):
    """The issue's acceptance rule; raises AssertionError, returns the number of points with c != rint(t).
    exact points: c == t.  Others: c == rint(t), or |c - t| <= 0.5 + e; never more than 1 from rint(t); at most 1 % of any tile."""
    c = np.asarray(codes).astype(np.int64)
    want = np.rint(ref.t).astype(np.int64)
    assert c.shape == want.shape, (label, c.shape, want.shape)
    bad = ref.exact & (c != want)
    assert not bad.any(), (label, "discrete points differ", int(bad.sum()), np.argwhere(bad)[:5])
    diff = c != want
    assert np.abs(c - want).max(initial=0) <= 1, (label, "a code more than 1 from rint(t)")
    out = diff & (np.abs(c - ref.t) > 0.5 + ref.e)
    assert not out.any(), (label, "outside 0.5 + e", int(out.sum()), np.argwhere(out)[:5])
    for t in np.unique(ref.tile[ref.tile >= 0]):
        m = ref.tile == t
        assert diff[m].sum() <= 0.01 * m.sum(), (label, f"tile {t}: {int(diff[m].sum())} of {int(m.sum())} points differ from rint(t)")
    return int(diff.sum())


def near_half_by_tile(ref: Reference):
    """{tile: (points within e of a half-integer, points)} for the tiles of continuous types"""
    nh = ref.near_half()
    return {int(t): (int(nh[ref.tile == t].sum()), int((ref.tile == t).sum())) for t in np.unique(ref.tile[ref.tile >= 0])
            if not ref.exact[ref.tile == t].all()}


def params_dict(cfg) -> dict:
    """the WlTerrainGenParams fields of a TerrainGeneratorCfg, as `reference` takes them"""
    from wheeledlab_amd.envs import terrain_gen_cfg as G
    return {k: v for k, v in G.lattice(cfg).items() if k in ("nx", "ny", "tile_nx", "tile_ny", "border", "rows", "cols", "base_code", "seed")}


def all_types_cfg(seed=3, curriculum=True, **kw):
    """The test grid: all five types, both inversions and the noise per cell and interpolated (spacing 3 and 4), one per column, three rows of
    difficulty; tiles of 47 x 38 points (no multiple of the 64 x 4 launch patch) inside a 3-point border.  The ranges keep every
    height within about 1 m of the base at 2^-13 m per code: slopes up to 0.5 over 14 cells, waves up to 0.1 m, interpolated noise
    within +-0.05 m -- small enough that the fp32 bounds above leave well under 1 % of a tile within e of a half-integer (counted,
    printed and asserted by tests/test_terrain_gen_host_sim_cpu.py)."""
    from wheeledlab_amd.envs import terrain_gen_cfg as G
    subs = {"noise": G.HfRandomUniformTerrainCfg(noise_range=(-0.02, 0.03), noise_step=0.005),
            "noise_interp3": G.HfRandomUniformTerrainCfg(noise_range=(-0.03, 0.05), noise_step=0.005, downsampled_scale=0.15),
            "noise_interp4": G.HfRandomUniformTerrainCfg(noise_range=(-0.03, 0.05), noise_step=0.005, downsampled_scale=0.2),
            "slope": G.HfPyramidSlopedTerrainCfg(slope_range=(0.1, 0.5), platform_width=0.5),
            "slope_inv": G.HfInvertedPyramidSlopedTerrainCfg(slope_range=(0.1, 0.5), platform_width=0.5),
            "stairs": G.HfPyramidStairsTerrainCfg(step_height_range=(0.01, 0.04), step_width=0.15, platform_width=0.5),
            "stairs_inv": G.HfInvertedPyramidStairsTerrainCfg(step_height_range=(0.01, 0.04), step_width=0.15, platform_width=0.5),
            "boxes": G.HfDiscreteObstaclesTerrainCfg(num_obstacles=12, obstacle_width_range=(0.15, 0.5), platform_width=0.4),
            "boxes_fixed": G.HfDiscreteObstaclesTerrainCfg(num_obstacles=64, obstacle_height_mode="fixed", obstacle_width_range=(0.1, 0.3),
                                                           platform_width=0.4),
            "wave": G.HfWaveTerrainCfg(amplitude_range=(0.03, 0.1), num_waves=3)}
    args = dict(seed=seed, curriculum=curriculum, size=(2.35, 1.9), border_width=0.15, num_rows=3, num_cols=len(subs), sub_terrains=subs)
    args.update(kw)
    return G.TerrainGeneratorCfg(**args)


def downstream_cfg(seed=12, **kw):
    """The 800 x 800 default grid with gentler waves, under a seed for which NO point of the reference lies within its fp32 bound of a
    half-integer (counted from the reference alone; the tests assert it): by the acceptance rule the device's codes must then EQUAL
    rint(t) everywhere, so that whole batches can be compared bit for bit on the generated field and on the reference's codes."""
    from wheeledlab_amd.envs import terrain_gen_cfg as G
    subs = G.default_sub_terrains()
    subs["wave"] = G.HfWaveTerrainCfg(proportion=0.2, amplitude_range=(0.02, 0.06), num_waves=2)
    return G.TerrainGeneratorCfg(seed=seed, sub_terrains=subs, **kw)

"""Procedural terrains: IsaacLab's `TerrainGeneratorCfg` surface (a grid of sub-terrains of rising difficulty, int16 codes x a
vertical scale) resolved on the host into the descriptor table the device generator reads (include/wheeledlab_amd_terrain.h:
WlTerrainGenParams + one WlTerrainTile per tile; csrc/wl_terrain_gen.hip).  Host-only and importable without a device: configs,
`lattice` (the grid's geometry), `tile_table` (type and difficulty of every tile, every range resolved to cells and codes, in
float64) and `check_covers` (the field against a task's reset square).

A DESIGNED generator: the five `Hf*TerrainCfg` classes carry the names and meanings of isaaclab.terrains.height_field, but the
draws come from the library's Philox4x32 keyed by (seed, tile, index), not from IsaacLab's numpy stream, and the default ranges are
scaled for a 1/10-scale car on 5 cm wheels (IsaacLab's 5 - 23 cm stairs are walls to it).  Rows advance along x (difficulty),
columns along y (terrain types), as IsaacLab lays its grid out."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi as A
from ..terrain import BASE_Z, Z_SCALE
from .configclass import configclass

TS_TABLE = 13      # Philox stream of the tile table's own draws (difficulty jitter, type choice); the kernel's are _abi.TS_*

TILE_DTYPE = np.dtype([(n, np.float32 if n in ("slope", "amplitude", "difficulty") else np.int32, (2,) if n == "pad" else ())
                       for n, _ in A.WlTerrainTile._fields_])
assert TILE_DTYPE.itemsize == 64


def philox4x32(c0, c1: int, c2: int, c3: int, seed: int, rounds: int = 7):
    """the library's generator (csrc/wl_rng.h) on python integers: counter (c0, c1, c2, c3), key = the seed's two words.  The
    package's one statement of it: no product exceeds 64 bits, so `c0` may as well be a uint64 array (terrain_levels.philox_word0)"""
    m = 0xFFFFFFFF
    c0, c1, c2, c3, k0, k1 = c0 & m, c1 & m, c2 & m, c3 & m, seed & m, (seed >> 32) & m
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def _u01(word: int) -> float:
    return (word >> 8) * 2.0 ** -24        # [0, 1), 24 bits: wl_rng.h u01


def _lerp(rng, d: float) -> float:
    return float(rng[0]) + (float(rng[1]) - float(rng[0])) * d


def _cells(metres: float, scale: float, lo: int = 0) -> int:
    return max(lo, int(round(float(metres) / scale)))


@configclass
class HfTerrainBaseCfg:
    proportion: float = 1.0
    flat_patch_sampling: dict | None = None     # {name: FlatPatchSamplingCfg}: level ground to find on this sub-terrain's tiles

    def resolve(self, difficulty: float, gen) -> dict:       # -> the WlTerrainTile fields this type sets
        raise NotImplementedError


@configclass
class HfRandomUniformTerrainCfg(HfTerrainBaseCfg):
    """heights from {noise_range[0], + noise_step, ...} up to noise_range[1], one draw per `downsampled_scale` metres (None: per
    cell), bilinear between the draws.  Like IsaacLab's, independent of the difficulty."""
    noise_range: tuple = (-0.01, 0.02)
    noise_step: float = 0.005
    downsampled_scale: float | None = None

    def resolve(self, difficulty, gen):
        vs = gen.vertical_scale
        step = max(1, int(round(self.noise_step / vs)))
        lo, hi = int(round(self.noise_range[0] / vs)), int(round(self.noise_range[1] / vs))
        if hi < lo:
            raise ValueError(f"noise_range {self.noise_range}: upper end below the lower")
        down = 1 if self.downsampled_scale is None else _cells(self.downsampled_scale, gen.horizontal_scale, 1)
        return dict(type=A.TT_RANDOM_UNIFORM, code_lo=lo, step_codes=step, n_levels=(hi - lo) // step + 1, step_cells=down)


@configclass
class HfPyramidSlopedTerrainCfg(HfTerrainBaseCfg):
    """a pyramid of slope (rise over run) slope_range[0] .. [1] with the difficulty, flat `platform_width` metres in the middle"""
    slope_range: tuple = (0.0, 0.3)
    platform_width: float = 1.0
    inverted: bool = False

    def resolve(self, difficulty, gen):
        slope = _lerp(self.slope_range, difficulty) * gen.horizontal_scale / gen.vertical_scale      # codes per cell
        return dict(type=A.TT_PYRAMID_SLOPED, flags=A.TF_INVERTED if self.inverted else 0, slope=np.float32(slope),
                    platform=_cells(self.platform_width, gen.horizontal_scale))


@configclass
class HfInvertedPyramidSlopedTerrainCfg(HfPyramidSlopedTerrainCfg):
    inverted: bool = True


@configclass
class HfPyramidStairsTerrainCfg(HfTerrainBaseCfg):
    """steps of `step_width` metres, step_height_range[0] .. [1] metres high with the difficulty, up to the platform"""
    step_height_range: tuple = (0.005, 0.03)
    step_width: float = 0.3
    platform_width: float = 1.0
    inverted: bool = False

    def resolve(self, difficulty, gen):
        return dict(type=A.TT_PYRAMID_STAIRS, flags=A.TF_INVERTED if self.inverted else 0,
                    step_codes=int(round(_lerp(self.step_height_range, difficulty) / gen.vertical_scale)),
                    step_cells=_cells(self.step_width, gen.horizontal_scale, 1), platform=_cells(self.platform_width, gen.horizontal_scale))


@configclass
class HfInvertedPyramidStairsTerrainCfg(HfPyramidStairsTerrainCfg):
    inverted: bool = True


@configclass
class HfDiscreteObstaclesTerrainCfg(HfTerrainBaseCfg):
    """`num_obstacles` axis-aligned boxes with sides in obstacle_width_range, the later one on top; height H = obstacle_height_range
    [0] .. [1] with the difficulty: "fixed" = H, "choice" = one of four evenly spaced levels from -H (a pit) to +H"""
    obstacle_height_mode: str = "choice"
    obstacle_width_range: tuple = (0.25, 0.75)
    obstacle_height_range: tuple = (0.01, 0.04)
    num_obstacles: int = 20
    platform_width: float = 1.0

    def resolve(self, difficulty, gen):
        h = int(round(_lerp(self.obstacle_height_range, difficulty) / gen.vertical_scale))
        if self.obstacle_height_mode == "fixed":
            levels = dict(code_lo=h, step_codes=0, n_levels=1)
        elif self.obstacle_height_mode == "choice":
            levels = dict(code_lo=-h, step_codes=(2 * h) // 3, n_levels=4)
        else:
            raise ValueError(f"obstacle_height_mode '{self.obstacle_height_mode}': 'fixed' or 'choice'")
        hs = gen.horizontal_scale
        return dict(type=A.TT_DISCRETE_OBSTACLES, n_obstacles=int(self.num_obstacles), size_lo=_cells(self.obstacle_width_range[0], hs, 1),
                    size_hi=_cells(self.obstacle_width_range[1], hs, 1), platform=_cells(self.platform_width, hs), **levels)


@configclass
class HfWaveTerrainCfg(HfTerrainBaseCfg):
    """amplitude * (sin + cos) with `num_waves` whole periods across the tile; amplitude_range[0] .. [1] metres with the difficulty"""
    amplitude_range: tuple = (0.0, 0.15)
    num_waves: int = 2

    def resolve(self, difficulty, gen):
        return dict(type=A.TT_WAVE, num_waves=int(self.num_waves), amplitude=np.float32(_lerp(self.amplitude_range, difficulty) / gen.vertical_scale))


def default_sub_terrains() -> dict:
    return {"random_rough": HfRandomUniformTerrainCfg(proportion=0.2), "pyramid_slope": HfPyramidSlopedTerrainCfg(proportion=0.1),
            "pyramid_slope_inv": HfInvertedPyramidSlopedTerrainCfg(proportion=0.1), "pyramid_stairs": HfPyramidStairsTerrainCfg(proportion=0.1),
            "pyramid_stairs_inv": HfInvertedPyramidStairsTerrainCfg(proportion=0.1), "boxes": HfDiscreteObstaclesTerrainCfg(proportion=0.2),
            "wave": HfWaveTerrainCfg(proportion=0.2)}


@configclass
class TerrainGeneratorCfg:
    """num_rows x num_cols tiles of `size` metres on a lattice of `horizontal_scale` metres inside a flat frame of `border_width`
    metres, centred on the origin; z = code * vertical_scale.  The defaults give the 800 x 800 lattice at 0.05 m (40 x 40 m) of the
    synthetic field, flat parts at its BASE_Z."""
    seed: int = 0
    curriculum: bool = True
    size: tuple = (8.0, 8.0)
    border_width: float = 0.0
    num_rows: int = 5
    num_cols: int = 5
    horizontal_scale: float = 0.05
    vertical_scale: float = Z_SCALE
    sub_terrains: dict = default_sub_terrains()     # (configclass deep-copies every default per instance: nothing is shared)
    difficulty_range: tuple = (0.0, 1.0)
    base_height: float = BASE_Z
    flat_patch_sampling: dict | None = None     # {name: FlatPatchSamplingCfg} for every sub-terrain that sets none under that name


def lattice(cfg) -> dict:
    """the grid's geometry: WlTerrainGenParams' integers, and the placement (x0, y0, cell, z_scale) of the heightfield"""
    hs, vs = float(cfg.horizontal_scale), float(cfg.vertical_scale)
    if not (math.isfinite(hs) and hs > 0 and math.isfinite(vs) and vs > 0):
        raise ValueError("TerrainGeneratorCfg: horizontal_scale and vertical_scale must be positive and finite")
    rows, cols = int(cfg.num_rows), int(cfg.num_cols)
    tile_nx, tile_ny, border = _cells(cfg.size[0], hs), _cells(cfg.size[1], hs), _cells(cfg.border_width, hs)
    if rows < 1 or cols < 1 or tile_nx < 2 or tile_ny < 2:
        raise ValueError(f"TerrainGeneratorCfg: {rows} x {cols} tiles of {tile_nx} x {tile_ny} points (at least 1 x 1 tiles of 2 x 2)")
    base = int(round(float(cfg.base_height) / vs))
    if abs(base) > 32767:
        raise ValueError(f"base_height {cfg.base_height} m does not fit 16-bit codes of {vs:g} m")
    nx, ny = rows * tile_nx + 2 * border, cols * tile_ny + 2 * border
    return dict(nx=nx, ny=ny, tile_nx=tile_nx, tile_ny=tile_ny, border=border, rows=rows, cols=cols, base_code=base,
                seed=int(cfg.seed) & (2 ** 64 - 1), x0=-0.5 * nx * hs, y0=-0.5 * ny * hs, cell=hs, z_scale=vs)


def _tile_choices(cfg, geo, names, cum) -> list:
    """(index into `names`, difficulty) of every tile, by tile_table's rule"""
    d_lo, d_hi = (float(v) for v in cfg.difficulty_range)
    rows, cols = geo["rows"], geo["cols"]
    out = []
    for r in range(rows):
        for c in range(cols):
            w = philox4x32(r * cols + c, 0, 0, TS_TABLE, geo["seed"])
            if cfg.curriculum:
                k, d = int(np.searchsorted(cum, (c + 0.5) / cols, side="right")), d_lo + (d_hi - d_lo) * (r + _u01(w[0])) / rows
            else:
                k, d = int(np.searchsorted(cum, _u01(w[1]), side="right")), d_lo + (d_hi - d_lo) * _u01(w[0])
            out.append((min(k, len(names) - 1), d))
    return out


def _cumulative_proportions(cfg):
    names = list(cfg.sub_terrains)
    if not names:
        raise ValueError("TerrainGeneratorCfg.sub_terrains is empty")
    prop = np.array([float(cfg.sub_terrains[n].proportion) for n in names], np.float64)
    if not (np.isfinite(prop).all() and (prop >= 0).all() and prop.sum() > 0):
        raise ValueError("sub-terrain proportions must be non-negative with a positive sum")
    cum = np.cumsum(prop / prop.sum())
    cum[-1] = 1.0
    return names, cum


def tile_names(cfg) -> list:
    """the sub_terrains key of every tile (tile t = row * num_cols + col), by tile_table's rule"""
    names, cum = _cumulative_proportions(cfg)
    return [names[k] for k, _ in _tile_choices(cfg, lattice(cfg), names, cum)]


def tile_table(cfg) -> np.ndarray:
    """-> WlTerrainTile [num_rows * num_cols] as a structured array (TILE_DTYPE; tile t = row * num_cols + col).
    curriculum=True: a column's type follows the cumulative proportions (column c takes the first type whose cumulative share
    exceeds (c + 1/2) / num_cols: the column's centre, which no rounding of the shares can put on a boundary) and the difficulty rises with the row: lo + (hi - lo) * (row + U) / num_rows, U in [0, 1) word 0 of
    Philox(t, 0, 0, TS_TABLE).  Otherwise both are drawn per tile: difficulty lo + (hi - lo) * U, type from word 1 against the
    cumulative proportions.  Each type then maps its ranges linearly in the difficulty to cells and codes (its `resolve`)."""
    geo = lattice(cfg)
    names, cum = _cumulative_proportions(cfg)
    rows, cols = geo["rows"], geo["cols"]
    table = np.zeros(rows * cols, TILE_DTYPE)
    table["step_cells"], table["n_levels"], table["size_lo"], table["size_hi"] = 1, 1, 1, 1
    choice = _tile_choices(cfg, geo, names, cum)
    for r in range(rows):
        for c in range(cols):
            t = r * cols + c
            k, d = choice[t]
            for key, val in cfg.sub_terrains[names[k]].resolve(d, cfg).items():
                table[key][t] = val
            table["difficulty"][t] = d
            side = min(geo["tile_nx"], geo["tile_ny"])
            table["platform"][t] = min(int(table["platform"][t]), side)
            table["size_hi"][t] = min(int(table["size_hi"][t]), side)
            table["size_lo"][t] = min(int(table["size_lo"][t]), int(table["size_hi"][t]))
    return table


def type_names(cfg, table) -> list:
    """the sub_terrains key of every tile of `table` (same order), found again from its type and flags"""
    out = []
    probe = {n: s.resolve(0.0, cfg) for n, s in cfg.sub_terrains.items()}
    for row in table:
        out.append(next(n for n, p in probe.items() if p["type"] == row["type"] and p.get("flags", 0) == row["flags"]))
    return out


def gen_params(cfg) -> "A.WlTerrainGenParams":
    g = lattice(cfg)
    return A.WlTerrainGenParams(g["nx"], g["ny"], g["tile_nx"], g["tile_ny"], g["border"], g["rows"], g["cols"], g["base_code"], g["seed"])


def check_covers(cfg, x_range, y_range=None, what: str = "the task's reset square"):
    """raise ValueError unless the generated lattice spans x_range = (lo, hi) and y_range (default: the same) in metres"""
    g = lattice(cfg)
    for axis, o, n, (want_lo, want_hi) in (("x", g["x0"], g["nx"], x_range), ("y", g["y0"], g["ny"], y_range or x_range)):
        lo, hi = o, o + (n - 1) * g["cell"]
        if lo > want_lo + 1e-9 or hi < want_hi - 1e-9:
            raise ValueError(f"the generated terrain spans {axis} in [{lo:g}, {hi:g}] m and does not cover {what}, "
                             f"[{want_lo:g}, {want_hi:g}] m: raise num_rows / num_cols, size or border_width")


# ---- flat patches: level ground to spawn on (include/wheeledlab_amd_terrain.h WlPatchTile; csrc/wl_flat_patch.hip) -----------------

PATCH_DTYPE = np.dtype([(n, np.int32, (2,) if n == "pad" else ()) for n, _ in A.WlPatchTile._fields_])
assert PATCH_DTYPE.itemsize == 48
_CODE_LIMIT = 2 ** 30      # z bounds beyond every 16-bit code: "no bound"


@configclass
class FlatPatchSamplingCfg:
    """IsaacLab's isaaclab.terrains.FlatPatchSamplingCfg: `num_patches` points per tile about which the ground within `patch_radius`
    metres (a list: the largest) varies by at most `max_height_diff` metres and lies within `z_range`; centres within x_range /
    y_range metres of the tile's centre.  z_range is measured from the generator's base_height (from z = 0 on a field that was
    not generated).  Ours: `max_tries` attempts per patch (IsaacLab's loop runs a fixed count and raises) and `on_failure` -- "centre":
    a slot without an accepted attempt takes the centre of its window and is counted (FlatPatches.failed); "raise": a ValueError
    that names the tile."""
    num_patches: int = 8
    patch_radius: float | list = 0.15
    x_range: tuple = (-1e6, 1e6)
    y_range: tuple = (-1e6, 1e6)
    z_range: tuple = (-1e6, 1e6)
    max_height_diff: float = 0.02
    max_tries: int = 4096
    on_failure: str = "centre"


def as_patch_cfg(c) -> FlatPatchSamplingCfg:
    """a FlatPatchSamplingCfg from itself or from its fields as a dict (what a command-line override gives), validated"""
    if isinstance(c, dict):
        c = FlatPatchSamplingCfg(**c)
    if not isinstance(c, FlatPatchSamplingCfg):
        raise ValueError(f"flat_patch_sampling entries are FlatPatchSamplingCfg (or its fields as a dict), got {type(c).__name__}")
    r = patch_radius(c)
    if int(c.num_patches) < 1:
        raise ValueError(f"FlatPatchSamplingCfg.num_patches {c.num_patches}: at least 1")
    if not (math.isfinite(r) and r >= 0):
        raise ValueError(f"FlatPatchSamplingCfg.patch_radius {c.patch_radius}: non-negative and finite")
    if not (math.isfinite(float(c.max_height_diff)) and float(c.max_height_diff) >= 0):
        raise ValueError(f"FlatPatchSamplingCfg.max_height_diff {c.max_height_diff}: non-negative and finite")
    if not 0 <= int(c.max_tries) <= A.PATCH_MAX_TRIES:
        raise ValueError(f"FlatPatchSamplingCfg.max_tries {c.max_tries}: 0 .. {A.PATCH_MAX_TRIES}")
    if c.on_failure not in ("centre", "raise"):
        raise ValueError(f"FlatPatchSamplingCfg.on_failure '{c.on_failure}': 'centre' or 'raise'")
    return c


def patch_radius(c) -> float:
    r = c.patch_radius
    return float(max(r)) if isinstance(r, (list, tuple)) else float(r)


def resolve_patch_tile(c, cell: float, z_scale: float, extent, centre, z_base: float = 0.0, what: str = "the field") -> dict:
    """The WlPatchTile fields of one window, in float64: `extent` = (i0, i1, j0, j1), the inclusive lattice rectangle the patch DISCS
    may touch (a tile, or the whole field); `centre` = (xc, yc) in LATTICE units (metres from lattice point (0, 0) over the cell),
    what x_range / y_range are measured from.  radius_cells = ceil(r / cell - 1e-9) rounds the radius UP to whole cells, so the
    tested disc of lattice points covers the metric one; radius2 = floor((r / cell)^2 + 1e-9); max_diff_codes = floor(d / z_scale +
    1e-9).  The window of patch centres is the extent inset by radius_cells, cut to the ranges."""
    c = as_patch_cfg(c)
    q = patch_radius(c) / cell
    rc, r2 = int(math.ceil(q - 1e-9)), int(math.floor(q * q + 1e-9))
    if rc > A.PATCH_MAX_RADIUS:
        raise ValueError(f"patch_radius {patch_radius(c):g} m is {rc} cells of {cell:g} m: at most {A.PATCH_MAX_RADIUS}")
    i0, i1, j0, j1 = extent
    lo, hi = [], []
    for a0, a1, mid, rng, axis in ((i0, i1, centre[0], c.x_range, "x"), (j0, j1, centre[1], c.y_range, "y")):
        w_lo = max(a0 + rc, int(math.ceil(mid + float(rng[0]) / cell - 1e-9)))
        w_hi = min(a1 - rc, int(math.floor(mid + float(rng[1]) / cell + 1e-9)))
        if w_lo > w_hi:
            raise ValueError(f"flat patches on {what}: no patch centre is left in {axis} (points {a0} .. {a1} inset by the radius of "
                             f"{rc} cells, cut to {axis}_range {tuple(rng)}): lower patch_radius or widen the range")
        lo.append(w_lo)
        hi.append(w_hi)
    z = [(z_base + float(v)) / z_scale for v in c.z_range]
    return dict(i_lo=lo[0], i_hi=hi[0], j_lo=lo[1], j_hi=hi[1], radius_cells=rc, radius2=r2,
                max_diff_codes=min(int(math.floor(float(c.max_height_diff) / z_scale + 1e-9)), _CODE_LIMIT),
                z_lo_code=int(max(-_CODE_LIMIT, min(_CODE_LIMIT, math.ceil(z[0] - 1e-9)))),
                z_hi_code=int(max(-_CODE_LIMIT, min(_CODE_LIMIT, math.floor(z[1] + 1e-9)))), max_tries=int(c.max_tries))


def patch_names(cfg) -> list:
    """every name under which the generator or one of its sub-terrains asks for flat patches, sorted"""
    names = set(cfg.flat_patch_sampling or ())
    for s in cfg.sub_terrains.values():
        names |= set(s.flat_patch_sampling or ())
    return sorted(names)


def patch_table(cfg, name: str):
    """-> (WlPatchTile [rows * cols] as a structured array, num_patches, raise_on bool [rows * cols], labels): the windows of the
    patches called `name` on every tile of a generated grid.  A tile's sampling is its sub-terrain's flat_patch_sampling[name], else
    the generator's; a tile with neither gets max_tries = 0 and a window holding its centre alone: every slot takes the centre.
    Every sampling under one name must ask for the same num_patches (one table, one stride)."""
    geo = lattice(cfg)
    subs = tile_names(cfg)
    default = (cfg.flat_patch_sampling or {}).get(name)
    per_tile = [((cfg.sub_terrains[s].flat_patch_sampling or {}).get(name) or default) for s in subs]
    per_tile = [None if c is None else as_patch_cfg(c) for c in per_tile]
    counts = sorted({int(c.num_patches) for c in per_tile if c is not None})
    if not counts:
        raise ValueError(f"no flat_patch_sampling named '{name}' on the generator or any of its sub-terrains")
    if len(counts) > 1:
        raise ValueError(f"flat patches '{name}': num_patches differs between sub-terrains ({counts}); one table needs one count")
    rows, cols, tnx, tny, b = geo["rows"], geo["cols"], geo["tile_nx"], geo["tile_ny"], geo["border"]
    table = np.zeros(rows * cols, PATCH_DTYPE)
    raise_on, labels = np.zeros(rows * cols, bool), []
    for r in range(rows):
        for c in range(cols):
            t = r * cols + c
            labels.append(f"tile {t} (row {r}, column {c}, '{subs[t]}')")
            extent = (b + r * tnx, b + (r + 1) * tnx - 1, b + c * tny, b + (c + 1) * tny - 1)
            centre = (b + (r + 0.5) * tnx, b + (c + 0.5) * tny)        # where envs.terrain_levels.tile_origins puts the tile's origin
            if per_tile[t] is None:
                fields = dict(i_lo=int(centre[0]), i_hi=int(centre[0]), j_lo=int(centre[1]), j_hi=int(centre[1]), z_lo_code=-_CODE_LIMIT,
                              z_hi_code=_CODE_LIMIT)
            else:
                fields = resolve_patch_tile(per_tile[t], geo["cell"], geo["z_scale"], extent, centre, float(cfg.base_height), labels[-1])
                raise_on[t] = per_tile[t].on_failure == "raise"
            for key, val in fields.items():
                table[key][t] = val
    return table, counts[0], raise_on, labels


def field_patch_table(c, nx: int, ny: int, x0: float, y0: float, cell: float, z_scale: float):
    """the one-tile table of a field that was not generated (a height array, a rasterised mesh): the window is the field inset by
    the radius, cut to x_range / y_range in WORLD metres; z_range from z = 0.  Same return as patch_table."""
    c = as_patch_cfg(c)
    fields = resolve_patch_tile(c, cell, z_scale, (0, int(nx) - 1, 0, int(ny) - 1), (-float(x0) / cell, -float(y0) / cell), 0.0, "the field")
    table = np.zeros(1, PATCH_DTYPE)
    for key, val in fields.items():
        table[key][0] = val
    return table, int(c.num_patches), np.array([c.on_failure == "raise"]), ["the field"]

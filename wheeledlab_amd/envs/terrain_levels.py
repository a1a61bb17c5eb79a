"""Terrain curriculum, host side: the tables a generated terrain's levels start from (include/wheeledlab_amd.h WlTerrainLevels)
and the checks a config must pass.  numpy only and importable without a device; the rule that moves an env between rows lives in
the step kernels (csrc/wl_elev_env.h next_level) and, restated, in tests/terrain_levels_reference.py.

IsaacLab's names: `terrain_origins` [rows, cols] are the tile centres, `terrain_levels` / `terrain_types` the row / column of
every env, `env_origins` the centres gathered per env (isaaclab.terrains.TerrainImporter with a curriculum generator)."""
from __future__ import annotations

import numpy as np

from .terrain_gen_cfg import lattice, philox4x32

LEVEL_STREAM = 3       # csrc/wl_elev_env.h ES_LEVEL: the Philox stream of the initial levels (step 0) and of the wrap draw (the step)


def philox_word0(gid, step: int, stream: int, seed: int, rounds: int = 7) -> np.ndarray:
    """word 0 of the library's Philox4x32 (terrain_gen_cfg.philox4x32, here on an array of counters) for (gid, step lo, step hi, stream)"""
    c0 = np.asarray(gid, np.uint64)
    # (flat: numpy's mixed arithmetic of a 0-d uint64 and a python integer has not always stayed in integers)
    return philox4x32(c0.reshape(-1), step, step >> 32, stream, seed, rounds)[0].astype(np.uint32).reshape(c0.shape)


def uniform_below(word, n: int) -> np.ndarray:
    """a 32-bit word reduced to [0, n): the high half of word * n (what __umulhi gives the kernel)"""
    return ((np.asarray(word, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def tile_origins(cfg) -> np.ndarray:
    """-> float32 [rows * cols, 2]: the centre (x, y) of tile row * cols + col in metres.  Rows advance along x (difficulty),
    columns along y (type), as the generator lays them out: x = x0 + (border + (row + 1/2) tile_nx) cell."""
    g = lattice(cfg)
    x = g["x0"] + (g["border"] + (np.arange(g["rows"]) + 0.5) * g["tile_nx"]) * g["cell"]
    y = g["y0"] + (g["border"] + (np.arange(g["cols"]) + 0.5) * g["tile_ny"]) * g["cell"]
    return np.stack(np.meshgrid(x, y, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)


def clamp_max_init(cfg, max_init_terrain_level) -> int:
    rows = int(cfg.num_rows)
    return rows - 1 if max_init_terrain_level is None else min(max(int(max_init_terrain_level), 0), rows - 1)


def initial_assignment(cfg, n_envs: int, env_offset: int = 0, world_envs: int | None = None, max_init_terrain_level=None, seed: int = 42):
    """-> (level int32 [n], type int32 [n]) of envs env_offset .. env_offset + n of a world of `world_envs` envs, keyed by the
    GLOBAL env id so that shards hold what the one big batch holds: type = gid * cols // world_envs (contiguous blocks per
    column: IsaacLab's floor(arange / (n / cols))), level = a Philox word (gid, step 0, LEVEL_STREAM) reduced to
    [0, max_init_terrain_level] (clamped to rows - 1; None: rows - 1)."""
    world = int(n_envs) if world_envs is None else int(world_envs)
    gid = int(env_offset) + np.arange(int(n_envs), dtype=np.int64)
    if world < 1 or gid.size and gid[-1] >= world:
        raise ValueError(f"world_envs {world} does not hold envs {env_offset} .. {env_offset + n_envs - 1}")
    cols = int(cfg.num_cols)
    types = (gid * cols // world).astype(np.int32)
    level = uniform_below(philox_word0(gid, 0, LEVEL_STREAM, int(seed) & (2 ** 64 - 1)), clamp_max_init(cfg, max_init_terrain_level) + 1)
    return level, types


def check_curriculum(cfg, reset_xy: float, cmd_xy: float):
    """what a generated terrain must satisfy to carry levels; each failure a ValueError naming the quantity"""
    if cfg is None:
        raise ValueError('terrain levels need a generated terrain: scene.terrain.terrain_type = "generator" with a terrain_generator')
    if not cfg.curriculum:
        raise ValueError("terrain levels need TerrainGeneratorCfg.curriculum = True: without it the rows are not ordered by difficulty")
    g = lattice(cfg)
    half = 0.5 * min(g["tile_nx"], g["tile_ny"]) * g["cell"]
    if float(reset_xy) > half + 1e-9:
        raise ValueError(f"reset_xy {float(reset_xy):g} m: the spawn square leaves its tile (half the shorter tile side is {half:g} m)")
    o = tile_origins(cfg).astype(np.float64)
    for axis, k, lo, n in (("x", 0, g["x0"], g["nx"]), ("y", 1, g["y0"], g["ny"])):
        hi = lo + (n - 1) * g["cell"]
        if o[:, k].min() - float(cmd_xy) < lo - 1e-9 or o[:, k].max() + float(cmd_xy) > hi + 1e-9:
            raise ValueError(f"cmd_xy {float(cmd_xy):g} m: the goal square of an outer tile leaves the lattice in {axis} "
                             f"([{lo:g}, {hi:g}] m): lower it or widen border_width")

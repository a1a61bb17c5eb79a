"""CPU checks of procedural terrains (wheeledlab_amd/envs/terrain_gen_cfg.py, include/wheeledlab_amd_terrain.h): the tile table
(types by proportion, difficulty along rows, seeds, ranges at their ends), the descriptor layouts against the header, the argument
refusals of the C entry points before any launch, the three Philox statements against each other, and the env surface's errors
(a field that does not cover the reset square, a generator beside another terrain source)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import terrain_gen_reference as TR
from conftest import ROOT
from oracle import philox as OP
from wheeledlab_amd import _abi as A
from wheeledlab_amd.envs import terrain_gen_cfg as G
from wheeledlab_amd.terrain import BASE_Z, Z_SCALE


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def test_column_types_follow_the_proportions():
    subs = {"a": G.HfWaveTerrainCfg(proportion=5.0), "b": G.HfPyramidStairsTerrainCfg(proportion=3.0),
            "c": G.HfInvertedPyramidSlopedTerrainCfg(proportion=2.0)}
    cfg = G.TerrainGeneratorCfg(num_rows=4, num_cols=10, size=(4.0, 4.0), sub_terrains=subs)
    names = np.array(G.type_names(cfg, G.tile_table(cfg))).reshape(4, 10)
    assert (names == names[0]).all()                                  # a column is one type
    assert list(names[0]) == ["a"] * 5 + ["b"] * 3 + ["c"] * 2
    # without a curriculum the type is drawn per tile: over many tiles the shares approach the proportions
    cfg = G.TerrainGeneratorCfg(curriculum=False, num_rows=40, num_cols=40, size=(1.0, 1.0), sub_terrains=subs, seed=5)
    names = np.array(G.type_names(cfg, G.tile_table(cfg)))
    share = {n: float((names == n).mean()) for n in subs}
    assert abs(share["a"] - 0.5) < 0.05 and abs(share["b"] - 0.3) < 0.05 and abs(share["c"] - 0.2) < 0.05, share
    assert (names.reshape(40, 40) != names.reshape(40, 40)[0]).any()


def test_difficulty_rises_along_rows_inside_its_range():
    cfg = G.TerrainGeneratorCfg(num_rows=6, num_cols=4, size=(7.0, 10.0), difficulty_range=(0.2, 0.9), seed=11)
    d = G.tile_table(cfg)["difficulty"].reshape(6, 4).astype(np.float64)
    assert (np.diff(d, axis=0) > 0).all()
    assert (d >= 0.2).all() and (d < 0.9).all()
    lo = 0.2 + 0.7 * np.arange(6)[:, None] / 6
    assert (d >= lo - 1e-6).all() and (d < lo + 0.7 / 6).all()        # row r: its own sixth of the range, jittered inside it
    assert len(np.unique(d)) == d.size                               # the jitter is per tile
    free = G.tile_table(cfg.replace(curriculum=False))["difficulty"].reshape(6, 4)
    assert (free >= 0.2).all() and (free < 0.9).all() and not (np.diff(free, axis=0) > 0).all()


def test_same_seed_same_table_another_seed_another():
    a, b = G.tile_table(G.TerrainGeneratorCfg(seed=7)), G.tile_table(G.TerrainGeneratorCfg(seed=7))
    c = G.tile_table(G.TerrainGeneratorCfg(seed=8))
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a.dtype == G.TILE_DTYPE and a.shape == (25,)
    big = G.tile_table(G.TerrainGeneratorCfg(seed=2 ** 40 + 7))        # the high word of the seed is part of the key
    assert big.tobytes() != a.tobytes()


def test_ranges_resolve_to_their_ends():
    gen = G.TerrainGeneratorCfg(horizontal_scale=0.05, vertical_scale=2.0 ** -13)
    s = G.HfPyramidSlopedTerrainCfg(slope_range=(0.1, 0.4), platform_width=1.0)
    assert s.resolve(0.0, gen)["slope"] == np.float32(0.1 * 0.05 * 8192) and s.resolve(1.0, gen)["slope"] == np.float32(0.4 * 0.05 * 8192)
    assert s.resolve(0.5, gen)["slope"] == np.float32(0.25 * 0.05 * 8192) and s.resolve(0.0, gen)["platform"] == 20
    assert s.resolve(0.0, gen)["flags"] == 0 and G.HfInvertedPyramidSlopedTerrainCfg().resolve(0.0, gen)["flags"] == A.TF_INVERTED
    st = G.HfPyramidStairsTerrainCfg(step_height_range=(0.01, 0.03), step_width=0.3)
    assert (st.resolve(0.0, gen)["step_codes"], st.resolve(1.0, gen)["step_codes"]) == (82, 246) and st.resolve(0.3, gen)["step_cells"] == 6
    assert G.HfInvertedPyramidStairsTerrainCfg().resolve(1.0, gen)["flags"] == A.TF_INVERTED
    w = G.HfWaveTerrainCfg(amplitude_range=(0.0, 0.125), num_waves=3)
    assert w.resolve(0.0, gen)["amplitude"] == 0.0 and w.resolve(1.0, gen)["amplitude"] == 1024.0 and w.resolve(1.0, gen)["num_waves"] == 3
    o = G.HfDiscreteObstaclesTerrainCfg(obstacle_height_range=(0.01, 0.04), obstacle_width_range=(0.25, 0.75), num_obstacles=9)
    r0, r1 = o.resolve(0.0, gen), o.resolve(1.0, gen)
    assert (r0["code_lo"], r0["step_codes"], r0["n_levels"]) == (-82, 54, 4) and (r1["code_lo"], r1["step_codes"]) == (-328, 218)
    assert (r0["size_lo"], r0["size_hi"], r0["n_obstacles"]) == (5, 15, 9)
    f = o.replace(obstacle_height_mode="fixed").resolve(1.0, gen)
    assert (f["code_lo"], f["step_codes"], f["n_levels"]) == (328, 0, 1)
    with pytest.raises(ValueError, match="obstacle_height_mode"):
        o.replace(obstacle_height_mode="random").resolve(0.5, gen)
    u = G.HfRandomUniformTerrainCfg(noise_range=(-0.01, 0.02), noise_step=0.005, downsampled_scale=0.2).resolve(0.7, gen)
    assert (u["code_lo"], u["step_codes"], u["n_levels"], u["step_cells"]) == (-82, 41, 7, 4)        # -82 + 41 * 6 = 164 = rint(0.02 * 8192)
    # and through the table: a one-row grid at a pinned difficulty
    for d, want in ((0.0, 82), (1.0, 246)):
        cfg = G.TerrainGeneratorCfg(num_rows=1, num_cols=1, difficulty_range=(d, d), sub_terrains={"s": st})
        assert int(G.tile_table(cfg)["step_codes"][0]) == want


def test_default_lattice_is_the_synthetic_fields():
    geo = G.lattice(G.TerrainGeneratorCfg())
    assert (geo["nx"], geo["ny"], geo["x0"], geo["y0"], geo["cell"], geo["z_scale"]) == (800, 800, -20.0, -20.0, 0.05, Z_SCALE)
    assert geo["base_code"] == int(np.rint(BASE_Z / Z_SCALE))
    geo = G.lattice(G.TerrainGeneratorCfg(size=(2.35, 1.9), border_width=0.15, num_rows=3, num_cols=9))
    assert (geo["nx"], geo["ny"], geo["tile_nx"], geo["tile_ny"], geo["border"]) == (3 * 47 + 6, 9 * 38 + 6, 47, 38, 3)


def test_descriptor_layouts_match_the_header(tmp_path):
    probe = tmp_path / "probe.c"
    body = ""
    for st in (A.WlTerrainTile, A.WlTerrainGenParams):
        body += " ".join(f'printf("%zu ", offsetof({st.__name__}, {n}));' for n, _ in st._fields_) + f' printf("%zu ", sizeof({st.__name__}));'
    consts = ("WL_TT_RANDOM_UNIFORM", "WL_TT_PYRAMID_SLOPED", "WL_TT_PYRAMID_STAIRS", "WL_TT_DISCRETE_OBSTACLES", "WL_TT_WAVE", "WL_TT_COUNT",
              "WL_TF_INVERTED", "WL_TS_UNIFORM", "WL_TS_OBSTACLES", "WL_TERRAIN_MAX_OBSTACLES", "WL_TERRAIN_MAX_OFFSET")
    body += " ".join(f'printf("%d ", (int){c});' for c in consts)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_terrain.h"\n' f"int main(){{{body} return 0;}}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for st in (A.WlTerrainTile, A.WlTerrainGenParams):
        want += [getattr(st, n).offset for n, _ in st._fields_] + [C.sizeof(st)]
    want += [A.TT_RANDOM_UNIFORM, A.TT_PYRAMID_SLOPED, A.TT_PYRAMID_STAIRS, A.TT_DISCRETE_OBSTACLES, A.TT_WAVE, A.TT_COUNT, A.TF_INVERTED,
             A.TS_UNIFORM, A.TS_OBSTACLES, A.TERRAIN_MAX_OBSTACLES, A.TERRAIN_MAX_OFFSET]
    assert got == want
    assert C.sizeof(A.WlTerrainTile) == G.TILE_DTYPE.itemsize == 64
    for n, _ in A.WlTerrainTile._fields_:
        assert G.TILE_DTYPE.fields[n][1] == getattr(A.WlTerrainTile, n).offset
    assert (TR.TT_RANDOM_UNIFORM, TR.TT_PYRAMID_SLOPED, TR.TT_PYRAMID_STAIRS, TR.TT_DISCRETE_OBSTACLES, TR.TT_WAVE, TR.TF_INVERTED, TR.TS_UNIFORM,
            TR.TS_OBSTACLES) == (A.TT_RANDOM_UNIFORM, A.TT_PYRAMID_SLOPED, A.TT_PYRAMID_STAIRS, A.TT_DISCRETE_OBSTACLES, A.TT_WAVE, A.TF_INVERTED,
                                 A.TS_UNIFORM, A.TS_OBSTACLES)


def test_generator_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    cfg = TR.all_types_cfg()
    table = np.ascontiguousarray(G.tile_table(cfg))
    tp = table.ctypes.data_as(C.c_void_p)
    ok = G.gen_params(cfg)
    assert lib.wl_terrain_gen_check(C.byref(ok), tp) == 0 and lib.wl_terrain_gen_check(C.byref(ok), None) == 0
    assert lib.wl_terrain_gen_check(None, tp) == -1
    fake = C.c_void_p(0x1000)                       # never dereferenced: every call below is refused before a launch
    assert lib.wl_terrain_generate(None, fake, fake, None) == -1
    assert lib.wl_terrain_generate(C.byref(ok), None, fake, None) == -1 and lib.wl_terrain_generate(C.byref(ok), fake, None, None) == -1
    assert lib.wl_terrain_generate(C.byref(ok), C.c_void_p(0x1002), fake, None) == -3 and lib.wl_terrain_generate(C.byref(ok), fake, C.c_void_p(0x1001), None) == -3
    for field, value in (("nx", ok.nx + 1), ("ny", ok.ny - 1), ("tile_nx", 1), ("tile_ny", 0), ("border", -1), ("rows", 0), ("cols", -2),
                         ("base_code", 32768), ("base_code", -40000), ("nx", 1)):
        p = G.gen_params(cfg)
        setattr(p, field, value)
        assert lib.wl_terrain_gen_check(C.byref(p), None) == -1 and lib.wl_terrain_generate(C.byref(p), fake, fake, None) == -1, field
    side = min(ok.tile_nx, ok.tile_ny)
    kinds = {int(t): k for k, t in enumerate(table["type"])}          # one tile of every type
    for kind, field, value in ((A.TT_RANDOM_UNIFORM, "n_levels", 0), (A.TT_RANDOM_UNIFORM, "step_cells", 0), (A.TT_RANDOM_UNIFORM, "code_lo", 40000),
                               (A.TT_RANDOM_UNIFORM, "step_codes", 30000), (A.TT_PYRAMID_SLOPED, "slope", np.nan), (A.TT_PYRAMID_SLOPED, "slope", 1e6),
                               (A.TT_PYRAMID_SLOPED, "platform", side + 1), (A.TT_PYRAMID_STAIRS, "step_cells", 0), (A.TT_PYRAMID_STAIRS, "step_codes", 20000),
                               (A.TT_PYRAMID_STAIRS, "platform", -1), (A.TT_DISCRETE_OBSTACLES, "n_obstacles", 65), (A.TT_DISCRETE_OBSTACLES, "size_lo", 0),
                               (A.TT_DISCRETE_OBSTACLES, "size_hi", side + 1), (A.TT_DISCRETE_OBSTACLES, "n_levels", 0), (A.TT_WAVE, "amplitude", np.inf),
                               (A.TT_WAVE, "amplitude", 20000.0), (A.TT_WAVE, "num_waves", -1), (A.TT_WAVE, "type", 9), (A.TT_WAVE, "flags", 2)):
        bad = table.copy()
        bad[field][kinds[kind]] = value
        assert lib.wl_terrain_gen_check(C.byref(ok), bad.ctypes.data_as(C.c_void_p)) == -1, (kind, field, value)


def test_three_philox_statements_agree():
    for seed in (0, 42, 2 ** 40 + 12345):
        ids = np.array([0, 1, 7, 2 ** 31 + 5], np.uint64)
        for c1, c2, c3 in ((0, 0, G.TS_TABLE), (5, 0, A.TS_OBSTACLES), (17, 33, A.TS_UNIFORM)):
            want = OP.philox4x32(ids, c1 | (c2 << 32), c3, seed)
            got = np.stack([w.astype(np.uint32) for w in TR.philox(ids, c1, c2, c3, seed)])
            assert np.array_equal(got, want)
            for k, t in enumerate(ids):
                assert G.philox4x32(int(t), c1, c2, c3, seed) == tuple(int(w) for w in want[:, k])


def _env_cfg(task, gen, **terrain):
    from wheeledlab_amd import registry, tasks  # noqa: F401
    cfg = registry.parse_env_cfg(task, device="cuda:0", num_envs=8)
    cfg.scene.terrain.terrain_type, cfg.scene.terrain.terrain_generator = "generator", gen
    for k, v in terrain.items():
        setattr(cfg.scene.terrain, k, v)
    return cfg


@pytest.mark.parametrize("task", ["Isaac-MushrElevationRL-v0", "Isaac-MushrVisualDepthRL-v0"])
def test_generator_reaches_the_batch_arguments_and_must_cover_the_reset_square(task):
    from wheeledlab_amd import registry, tasks  # noqa: F401
    from wheeledlab_amd.envs.flatten import flatten_cfg
    plain = registry.parse_env_cfg(task, device="cuda:0", num_envs=8)
    assert plain.scene.terrain.terrain_generator is None and plain.scene.terrain.terrain_type != "generator"      # the defaults stay
    assert flatten_cfg(plain).extra["terrain_generator"] is None
    gen = G.TerrainGeneratorCfg(seed=4)
    x = flatten_cfg(_env_cfg(task, gen)).extra
    assert x["terrain_generator"] is gen and x["heightfield"] is None and x["mesh_path"] is None
    assert flatten_cfg(_env_cfg(task, {"seed": 9, "num_rows": 5})).extra["terrain_generator"].seed == 9      # a command-line dict
    # 4 x 4 tiles of 8 m: +-16 m, inside the +-19 m (elevation) / -20 .. 19.5 m (visual depth) the tasks reset over
    with pytest.raises(ValueError, match="does not cover"):
        flatten_cfg(_env_cfg(task, G.TerrainGeneratorCfg(num_rows=4, num_cols=4)))
    with pytest.raises(ValueError, match="does not cover"):
        flatten_cfg(_env_cfg(task, G.TerrainGeneratorCfg(num_rows=5, num_cols=4)))            # short in y alone
    flatten_cfg(_env_cfg(task, G.TerrainGeneratorCfg(num_rows=4, num_cols=4, border_width=4.0)))   # the border counts
    with pytest.raises(ValueError, match="terrain_generator"):
        flatten_cfg(_env_cfg(task, None))
    forgot = _env_cfg(task, gen)
    forgot.scene.terrain.terrain_type = plain.scene.terrain.terrain_type       # a generator nobody switched on is not ignored
    with pytest.raises(ValueError, match='terrain_type is not "generator"'):
        flatten_cfg(forgot)


@pytest.mark.parametrize("task", ["Isaac-MushrElevationRL-v0", "Isaac-MushrVisualDepthRL-v0"])
def test_generator_excludes_the_other_terrain_sources(task, tmp_path):
    from wheeledlab_amd.envs.flatten import flatten_cfg
    gen = G.TerrainGeneratorCfg()
    field = (np.zeros((8, 8), np.float32), -1.0, -1.0, 0.25)
    with pytest.raises(ValueError, match="generator"):
        flatten_cfg(_env_cfg(task, gen, heightfield=field))
    with pytest.raises(ValueError, match="generator"):
        flatten_cfg(_env_cfg(task, gen, mesh_path=str(tmp_path / "t.obj")))


def test_terrain_resample_interval_is_a_run_option():
    from wheeledlab_amd.configs.runs import resolve_run
    assert resolve_run("RSS_ELEV_CONFIG").train.terrain_resample_interval == 0
    run = resolve_run("RSS_ELEV_CONFIG", ["train.terrain_resample_interval=5", "env.scene.terrain.terrain_type=generator",
                                          "env.scene.terrain.terrain_generator={'seed': 3}"])
    assert run.train.terrain_resample_interval == 5 and run.env.scene.terrain.terrain_generator == {"seed": 3}


def test_regenerate_and_generate_need_a_device():
    import torch

    from wheeledlab_amd.core import DeviceHeightField, generate_heightfield
    with pytest.raises(A.HipExtensionMissing):
        generate_heightfield(G.TerrainGeneratorCfg(), "cpu")
    geo = G.lattice(G.TerrainGeneratorCfg())
    field = DeviceHeightField((torch.zeros(800, 800, dtype=torch.int16), geo["x0"], geo["y0"], geo["cell"], geo["z_scale"]), "cpu")
    with pytest.raises(A.HipExtensionMissing):
        field.regenerate(G.TerrainGeneratorCfg())


def test_config_instances_share_no_defaults():
    a, b = G.TerrainGeneratorCfg(), G.TerrainGeneratorCfg()
    assert a.sub_terrains is not b.sub_terrains and a.sub_terrains["wave"] is not b.sub_terrains["wave"]
    a.sub_terrains["wave"].num_waves = 7
    del a.sub_terrains["boxes"]
    assert b.sub_terrains["wave"].num_waves == 2 and "boxes" in b.sub_terrains and "boxes" in G.TerrainGeneratorCfg().sub_terrains

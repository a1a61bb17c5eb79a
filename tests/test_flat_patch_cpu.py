"""Flat patches, host side: the C layout of the new structs (and that the step ABI did not move), every refusal of the host check and
of the two launch entry points (refused before a launch: no device needed), the config resolution, the virtual-column layout the
terrain-levels tables take, the deal across shards, and the refusals of the env config."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import flat_patch_reference as FR
from tests import terrain_levels_reference as REF
from wheeledlab_amd import _abi as A
from wheeledlab_amd.envs import terrain_gen_cfg as G
from wheeledlab_amd.envs import terrain_levels as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -3


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def sampling(**kw):
    return G.FlatPatchSamplingCfg(**{**dict(num_patches=8, patch_radius=0.15, max_height_diff=0.02, max_tries=1024), **kw})


def gen_cfg(**kw):
    return G.TerrainGeneratorCfg(**{**dict(seed=4, num_rows=3, num_cols=2, size=(3.2, 3.2), border_width=1.0,
                                           flat_patch_sampling={"init_pos": sampling()}), **kw})


def test_layout_matches_the_header_and_the_step_abi_stands(tmp_path):
    probe = tmp_path / "probe.c"
    structs = {"WlPatchTile": A.WlPatchTile, "WlFlatPatchParams": A.WlFlatPatchParams}
    body = " ".join(f'printf("%zu ", offsetof({s}, {n}));' for s, cls in structs.items() for n, _ in cls._fields_)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_terrain.h"\n'
                     f'int main(){{{body} printf("%zu %zu %d %d %d %d %d %d %d %d %zu %zu\\n", sizeof(WlPatchTile), sizeof(WlFlatPatchParams), '
                     "(int)WL_TERRAIN_VERSION, (int)WL_ABI_VERSION, (int)WL_ABI_REVISION, (int)WL_TS_PATCH, (int)WL_TS_PATCH_DEAL, (int)WL_PATCH_MAX_RADIUS, "
                     "(int)WL_PATCH_MAX_TRIES, (int)WL_PATCH_MAX_SLOTS, sizeof(WlElevParams), sizeof(WlTerrainLevels)); return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(cls, n).offset for cls in structs.values() for n, _ in cls._fields_] + [
        C.sizeof(A.WlPatchTile), C.sizeof(A.WlFlatPatchParams), A.WL_TERRAIN_VERSION, A.WL_ABI_VERSION, A.WL_ABI_REVISION, A.TS_PATCH, A.TS_PATCH_DEAL,
        A.PATCH_MAX_RADIUS, A.PATCH_MAX_TRIES, A.PATCH_MAX_SLOTS, C.sizeof(A.WlElevParams), C.sizeof(A.WlTerrainLevels)]
    assert got == want
    assert C.sizeof(A.WlPatchTile) == 48 and G.PATCH_DTYPE.itemsize == 48 and C.sizeof(A.WlFlatPatchParams) == 24
    assert [A.WL_ABI_VERSION, A.WL_ABI_REVISION] == [24, 1] and A.WL_TERRAIN_VERSION == 3
    assert [n for n, _ in A.WlTerrainLevels._fields_] == ["level", "type", "origins", "rows", "cols"]      # the step kernels' tables: as they were
    lib = _lib()
    assert lib.wl_version() == 24 and lib.wl_revision() == 1 and lib.wl_terrain_version() == 3
    assert (FR.TS_PATCH, FR.TS_PATCH_DEAL) == (A.TS_PATCH, A.TS_PATCH_DEAL)


def test_every_refusal_of_the_check_and_the_entry_points():
    lib = _lib()
    nx, ny = 40, 33
    fake = 0x1000                                 # never dereferenced: every launch below is refused before it

    def field(**kw):
        v = dict(height=fake, nx=nx, ny=ny, x0=-1.0, y0=-0.8, cell=0.05, outside_z=0.0, z_scale=2.0 ** -13, pair=None)
        v.update(kw)
        return A.WlHeightField(*[v[n] for n, _ in A.WlHeightField._fields_])

    def params(**kw):
        v = dict(n_tiles=2, n_patches=8, stream=A.TS_PATCH, reserved=0, seed=5)
        v.update(kw)
        return A.WlFlatPatchParams(*[v[n] for n, _ in A.WlFlatPatchParams._fields_])

    def tiles(**kw):
        t = np.zeros(2, G.PATCH_DTYPE)
        for k, v in dict(i_lo=3, i_hi=36, j_lo=3, j_hi=29, radius_cells=3, radius2=9, max_diff_codes=163, z_lo_code=-2 ** 30, z_hi_code=2 ** 30,
                         max_tries=100).items():
            t[k] = v
        for k, v in kw.items():
            t[k][1] = v
        return t

    def check(hf=None, p=None, t="good"):
        t = tiles() if isinstance(t, str) else t
        return lib.wl_flat_patch_check(C.byref(hf or field()), C.byref(p or params()), None if t is None else t.ctypes.data_as(C.c_void_p))

    def launch(hf=None, p=None, ptrs=(fake, fake, fake, fake)):
        return lib.wl_flat_patches(C.byref(hf or field()), C.byref(p or params()), *[C.c_void_p(q) if q else None for q in ptrs], None)

    assert check() == 0 and check(t=None) == 0
    assert lib.wl_flat_patch_check(None, C.byref(params()), None) == EINVAL and lib.wl_flat_patch_check(C.byref(field()), None, None) == EINVAL
    # the field and the parameters: the check and the launch refuse alike
    for kw in (dict(height=None), dict(nx=0), dict(ny=-1), dict(nx=70000, ny=70000), dict(cell=0.0), dict(cell=math.nan), dict(cell=math.inf),
               dict(z_scale=0.0), dict(z_scale=-1.0), dict(x0=math.nan), dict(y0=math.inf)):
        assert check(hf=field(**kw)) == EINVAL and launch(hf=field(**kw)) == EINVAL, kw
    for kw in (dict(n_tiles=0), dict(n_patches=0), dict(n_tiles=-3), dict(n_tiles=1 << 12, n_patches=(1 << 10) + 1), dict(reserved=1)):
        assert check(p=params(**kw), t=None) == EINVAL and launch(p=params(**kw)) == EINVAL, kw
    assert check(p=params(n_tiles=1 << 12, n_patches=1 << 10), t=None) == 0                  # the largest count
    assert check(hf=field(height=fake + 1)) == EALIGN and launch(hf=field(height=fake + 1)) == EALIGN
    assert lib.wl_flat_patch_check(C.byref(field()), C.byref(params()), C.c_void_p(fake + 2)) == EALIGN      # (refused before it is read)
    # the descriptors: empty windows, discs that leave the lattice, radius, tries
    for kw in (dict(i_lo=37), dict(j_lo=30), dict(i_lo=2), dict(j_lo=2), dict(i_hi=37), dict(j_hi=30), dict(i_lo=-5, i_hi=-4),
               dict(i_lo=2 ** 31 - 2, i_hi=2 ** 31 - 1), dict(radius_cells=-1), dict(radius_cells=65), dict(radius2=10), dict(radius2=-1),
               dict(max_diff_codes=-1), dict(max_tries=-1), dict(max_tries=65537)):
        assert check(t=tiles(**kw)) == EINVAL, kw
    for kw in (dict(max_tries=0), dict(max_tries=65536), dict(radius_cells=0, radius2=0, i_lo=0, i_hi=39, j_lo=0, j_hi=32), dict(radius2=0),
               dict(z_lo_code=5, z_hi_code=-5)):
        assert check(t=tiles(**kw)) == 0, kw
    wide = np.zeros(1, G.PATCH_DTYPE)
    for k, v in dict(i_lo=64, i_hi=64, j_lo=64, j_hi=64, radius_cells=64, radius2=4096, max_tries=1).items():
        wide[k] = v
    assert check(hf=field(nx=129, ny=129), p=params(n_tiles=1), t=wide) == 0
    # the launch's own pointers
    for k in range(4):
        assert launch(ptrs=tuple(None if i == k else fake for i in range(4))) == EINVAL, k
        assert launch(ptrs=tuple(fake + 2 if i == k else fake for i in range(4))) == EALIGN, k
    # the deal
    deal = lambda n=64, off=0, world=64, cols=2, P=8, out=fake: lib.wl_flat_patch_deal(n, off, world, cols, P, 0, 9, C.c_void_p(out) if out else None, None)  # noqa: E731
    for kw in (dict(n=-1), dict(off=-1), dict(world=0), dict(n=33, off=32), dict(cols=0), dict(P=0), dict(cols=1 << 16, P=(1 << 14) + 1), dict(out=None)):
        assert deal(**kw) == EINVAL, kw
    assert deal(out=fake + 2) == EALIGN
    assert deal(n=0) == 0                                                                     # nothing to deal, nothing launched


def test_config_resolution():
    cfg = gen_cfg()
    geo = G.lattice(cfg)
    table, P, raise_on, labels = G.patch_table(cfg, "init_pos")
    assert P == 8 and len(table) == 6 and not raise_on.any() and labels[3].startswith("tile 3 (row 1, column 1")
    assert geo["tile_nx"] == 64 and geo["border"] == 20
    # 0.15 m at 0.05 m: 3 cells, 9; 0.02 m at 2^-13 m: 163 codes; the tile inset by the radius
    assert (table["radius_cells"] == 3).all() and (table["radius2"] == 9).all() and (table["max_diff_codes"] == 163).all()
    for r in range(3):
        for c in range(2):
            T = table[r * 2 + c]
            assert (T["i_lo"], T["i_hi"], T["j_lo"], T["j_hi"]) == (20 + 64 * r + 3, 20 + 64 * r + 60, 20 + 64 * c + 3, 20 + 64 * c + 60)
    assert lib_check(geo, table, P) == 0
    # a radius between whole cells rounds UP for the square and down for the squared bound; a list takes the largest
    T = G.patch_table(gen_cfg(flat_patch_sampling={"init_pos": sampling(patch_radius=[0.05, 0.12])}), "init_pos")[0][0]
    assert (T["radius_cells"], T["radius2"]) == (3, 5)                  # 2.4 cells: ceil = 3, floor(5.76) = 5
    T = G.patch_table(gen_cfg(flat_patch_sampling={"init_pos": sampling(patch_radius=0.0, max_height_diff=0.0)}), "init_pos")[0][0]
    assert (T["radius_cells"], T["radius2"], T["max_diff_codes"], T["i_lo"]) == (0, 0, 0, 20)
    # ranges about the tile's centre (tile 0: point 20 + 32 = 52) cut the window; z_range counts from the base height
    s = sampling(x_range=(-0.5, 0.25), y_range=(-1e6, 0.0), z_range=(-0.01, 0.03))
    T = G.patch_table(gen_cfg(flat_patch_sampling={"init_pos": s}), "init_pos")[0][0]
    assert (T["i_lo"], T["i_hi"], T["j_lo"], T["j_hi"]) == (42, 57, 23, 52)
    base = cfg.base_height / geo["z_scale"]
    assert (T["z_lo_code"], T["z_hi_code"]) == (math.ceil(base - 0.01 * 8192 - 1e-9), math.floor(base + 0.03 * 8192 + 1e-9))
    # a sub-terrain's own sampling wins over the generator's; a tile with neither takes its centre without a search
    subs = G.default_sub_terrains()
    subs["wave"].flat_patch_sampling = {"init_pos": sampling(max_tries=7, on_failure="raise")}
    both = G.TerrainGeneratorCfg(seed=1, num_rows=2, num_cols=7, size=(3.0, 3.0), sub_terrains=subs, flat_patch_sampling={"init_pos": sampling()})
    table, _, raise_on, _ = G.patch_table(both, "init_pos")
    names = G.tile_names(both)
    assert names == G.type_names(both, G.tile_table(both))
    assert [int(t) for t in table["max_tries"]] == [7 if n == "wave" else 1024 for n in names] and raise_on.tolist() == [n == "wave" for n in names]
    only = G.TerrainGeneratorCfg(seed=1, num_rows=2, num_cols=7, size=(3.0, 3.0), sub_terrains=subs)
    table = G.patch_table(only, "init_pos")[0]
    for T, n in zip(table, names):
        assert int(T["max_tries"]) == (7 if n == "wave" else 0)
        if n != "wave":
            assert T["i_lo"] == T["i_hi"] == (T["i_lo"] // 60) * 60 + 30 and T["j_lo"] == T["j_hi"]
    assert G.patch_names(both) == ["init_pos"] and G.patch_names(G.TerrainGeneratorCfg()) == []
    subs["boxes"].flat_patch_sampling = {"target": sampling(num_patches=3)}
    assert G.patch_names(G.TerrainGeneratorCfg(sub_terrains=subs)) == ["init_pos", "target"]
    # a plain field: the window is the field inset by the radius, the ranges are world metres
    table, P, raise_on, _ = G.field_patch_table(dict(num_patches=4, patch_radius=0.1, x_range=(-0.5, 1e6), on_failure="raise"), 40, 33, -1.0, -0.8, 0.05, 2.0 ** -13)
    assert P == 4 and raise_on.all() and tuple(int(table[k][0]) for k in ("i_lo", "i_hi", "j_lo", "j_hi")) == (10, 37, 2, 30)
    # refusals name the quantity
    for kw, match in ((dict(num_patches=0), "num_patches"), (dict(patch_radius=-0.1), "patch_radius"), (dict(patch_radius=4.0), "patch_radius"),
                      (dict(max_height_diff=-1.0), "max_height_diff"), (dict(max_tries=70000), "max_tries"), (dict(on_failure="ignore"), "on_failure"),
                      (dict(patch_radius=1.7), "no patch centre"), (dict(x_range=(5.0, 6.0)), "x_range")):
        with pytest.raises(ValueError, match=match):
            G.patch_table(gen_cfg(flat_patch_sampling={"init_pos": sampling(**kw)}), "init_pos")
    with pytest.raises(ValueError, match="target"):
        G.patch_table(cfg, "target")
    subs = G.default_sub_terrains()
    subs["wave"].flat_patch_sampling = {"init_pos": sampling(num_patches=4)}
    with pytest.raises(ValueError, match="num_patches differs"):
        G.patch_table(G.TerrainGeneratorCfg(sub_terrains=subs, flat_patch_sampling={"init_pos": sampling()}), "init_pos")


def test_table_follows_the_tile_types_and_goals_count_every_tile():
    """a sub-terrain's own sampling without a curriculum: the seed draws every tile's type, so the table of one seed is not the next's
    (what core.FlatPatches resolves again at a redraw: its key holds the seed exactly then); and the goal check counts the unsearched
    tiles' one-point windows"""
    from wheeledlab_amd.core import FlatPatches
    from wheeledlab_amd.envs.flatten import check_patch_goals
    subs = G.default_sub_terrains()
    subs["boxes"].flat_patch_sampling = {"init_pos": sampling(max_tries=64, on_failure="raise")}
    make = lambda seed, curriculum: G.TerrainGeneratorCfg(seed=seed, curriculum=curriculum, num_rows=3, num_cols=4, size=(3.0, 3.0),   # noqa: E731
                                                          border_width=0.5, sub_terrains=subs)
    a, b = make(1, False), make(2, False)
    assert G.tile_names(a) != G.tile_names(b) and "boxes" in G.tile_names(a) and "boxes" in G.tile_names(b)
    ta, tb = G.patch_table(a, "init_pos"), G.patch_table(b, "init_pos")
    assert ta[1] == tb[1] == 8 and not np.array_equal(ta[0]["max_tries"], tb[0]["max_tries"]) and ta[3] != tb[3]
    for cfg_, (table, _, raise_on, labels) in ((a, ta), (b, tb)):
        names = G.tile_names(cfg_)
        assert [int(t) for t in table["max_tries"]] == [64 if n == "boxes" else 0 for n in names] and raise_on.tolist() == [n == "boxes" for n in names]
        assert all(f"'{n}'" in lab for n, lab in zip(names, labels))
    assert FlatPatches._table_key(a) != FlatPatches._table_key(b)                                  # no curriculum: the seed counts
    assert FlatPatches._table_key(make(1, True)) == FlatPatches._table_key(make(2, True))          # columns fix the types: it does not
    assert FlatPatches._table_key(make(1, True)) != FlatPatches._table_key(make(1, True).replace(num_rows=4))
    assert FlatPatches._table_key(a, sampling=False) == FlatPatches._table_key(a.replace(flat_patch_sampling={"init_pos": sampling()}), sampling=False)
    # goals: a searched tile in the middle does not excuse an unsearched one at the edge
    geo = G.lattice(a)
    table = ta[0]
    edge = int(np.argmin(np.where(table["max_tries"] == 0, table["i_lo"], 10 ** 9)))
    reach = min(int(table["i_lo"][edge]), int(table["j_lo"][edge])) * geo["cell"]                  # its centre's distance to the lattice's near edge
    assert (table["max_tries"] > 0).any() and table["max_tries"][edge] == 0
    searched_reach = min(int(table["i_lo"][table["max_tries"] > 0].min()), int(table["j_lo"][table["max_tries"] > 0].min())) * geo["cell"]
    far = min(int(geo["nx"] - 1 - table["i_hi"].max()), int(geo["ny"] - 1 - table["j_hi"].max())) * geo["cell"]
    check_patch_goals(table, geo["nx"], geo["ny"], geo["cell"], min(reach, far) - 0.01)
    if reach < min(searched_reach, far):
        with pytest.raises(ValueError, match="cmd_xy"):
            check_patch_goals(table, geo["nx"], geo["ny"], geo["cell"], reach + 0.01)
    one = np.zeros(2, G.PATCH_DTYPE)
    for k, v in dict(i_lo=(2, 20), i_hi=(2, 30), j_lo=(25, 20), j_hi=(25, 30), max_tries=(0, 100)).items():
        one[k] = v
    check_patch_goals(one[1:], 51, 51, 0.1, 2.0)
    with pytest.raises(ValueError, match="cmd_xy"):
        check_patch_goals(one, 51, 51, 0.1, 0.5)                                                   # the unsearched tile's centre is 0.2 m from the edge


def lib_check(geo, table, P):
    hf = A.WlHeightField(0x1000, geo["nx"], geo["ny"], geo["x0"], geo["y0"], geo["cell"], 0.0, geo["z_scale"], None)
    p = A.WlFlatPatchParams(len(table), P, A.TS_PATCH, 0, 5)
    return _lib().wl_flat_patch_check(C.byref(hf), C.byref(p), np.ascontiguousarray(table).ctypes.data_as(C.c_void_p))


def test_virtual_columns_deal_and_types():
    rows, cols, P, n, seed = 3, 2, 8, 70, 9
    cfg = gen_cfg()
    # the finder's xy buffer [tile][k][2] read as the origins table of cols * P columns: entry (level, col * P + slot) is patch `slot` of
    # tile level * cols + col -- by the lookup the step kernels and their reference use (row * cols_virtual + type)
    xy = np.arange(rows * cols * P * 2, dtype=np.float32).reshape(rows * cols, P, 2)
    level, col = TL.initial_assignment(cfg, n, 0, n, None, seed)
    types = FR.deal(np.arange(n), cols, n, P, 0, seed)
    assert types.dtype == np.int32 and types.min() >= 0 and types.max() < cols * P
    np.testing.assert_array_equal(types // P, col)                                     # terrain_types == type // P: the real grid's column
    assert len(np.unique(types % P)) == P                                              # every slot is dealt
    levels = dict(level=level, type=types, origins=xy.reshape(-1, 2), rows=rows, cols=cols * P)
    np.testing.assert_array_equal(REF.origins_of(levels, np.arange(n)), xy[level * cols + col, types % P])
    # two shards hold what the one batch holds, in every epoch; an epoch changes the slots and never the columns
    for epoch in (0, 1, 2 ** 33 + 5):
        whole = FR.deal(np.arange(n), cols, n, P, epoch, seed)
        parts = [FR.deal(off + np.arange(m), cols, n, P, epoch, seed) for off, m in ((0, 32), (32, 38))]
        np.testing.assert_array_equal(np.concatenate(parts), whole)
        np.testing.assert_array_equal(whole // P, col)
    assert (FR.deal(np.arange(n), cols, n, P, 1, seed) != types).any()
    # the slot is the high half of word 0 of Philox(gid, epoch, 0, 15) times P
    w = TL.philox_word0(np.arange(n), 0, A.TS_PATCH_DEAL, seed)
    np.testing.assert_array_equal(types % P, TL.uniform_below(w, P))


def test_flatten_refusals_and_the_resolved_task():
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.tasks.elevation import MushrElevationRLEnvCfg, MushrElevationTerrainLevelsEnvCfg

    def cfg(reset=0.1, cmd=3.5, patches=True, cls=MushrElevationTerrainLevelsEnvCfg, **kw):
        c = cls()
        c.events.set_goal.func = mdp.reset_root_state_from_terrain
        c.events.set_goal.params["pose_range"].update(x=(-reset, reset), y=(-reset, reset))
        c.commands.goal_pose.ranges.pos_x = c.commands.goal_pose.ranges.pos_y = (-cmd, cmd)
        if patches and c.scene.terrain.terrain_generator is not None:
            # (8 m tiles without a frame: patch centres within 0.4 m of the tile's centre leave the 3.5 m goal square on the lattice)
            c.scene.terrain.terrain_generator.flat_patch_sampling = {"init_pos": sampling(**{**dict(x_range=(-0.4, 0.4), y_range=(-0.4, 0.4)), **kw})}
        return c

    flat = flatten_cfg(cfg())
    assert flat.extra["flat_patches"] == dict(names=["init_pos"], sampling=None, spawn=True)
    assert abs(flat.params.reset_xy - 0.1) < 1e-7 and flat.extra["terrain_levels"]["name"] == "terrain_levels"
    with pytest.raises(ValueError, match="init_pos"):
        flatten_cfg(cfg(patches=False))
    c = cfg(patches=False)
    c.scene.terrain.terrain_generator.flat_patch_sampling = {"target": sampling()}
    with pytest.raises(ValueError, match="init_pos"):
        flatten_cfg(c)
    with pytest.raises(ValueError, match="reset_xy"):
        flatten_cfg(cfg(reset=0.11))                       # sqrt(2) * 0.11 = 0.156 m > 0.15 m
    flatten_cfg(cfg(reset=0.106))                          # sqrt(2) * 0.106 = 0.1499 m
    with pytest.raises(ValueError, match="cmd_xy"):
        flatten_cfg(cfg(cmd=3.6))                          # the last tile's centre is 3.95 m from the lattice's last point: 0.4 + 3.6 > 3.95
    with pytest.raises(ValueError, match="cmd_xy"):
        flatten_cfg(cfg(x_range=(-1e6, 1e6)))              # patches anywhere on an outer tile: the goal square leaves the lattice
    flatten_cfg(cfg(cmd=3.55))
    # a pose_range without x / y spawns on the patch
    c = cfg()
    del c.events.set_goal.params["pose_range"]["x"], c.events.set_goal.params["pose_range"]["y"]
    assert flatten_cfg(c).params.reset_xy == 0.0
    # a height array: scene.terrain carries the sampling; a generator refuses it there
    c = cfg(cls=MushrElevationRLEnvCfg)
    with pytest.raises(ValueError, match="init_pos"):
        flatten_cfg(c)
    c.scene.terrain.flat_patch_sampling = {"init_pos": dict(num_patches=4, patch_radius=0.2), "target": sampling()}
    x = flatten_cfg(c).extra["flat_patches"]
    assert x["names"] == ["init_pos", "target"] and x["spawn"] and x["sampling"]["init_pos"].num_patches == 4
    c = cfg()
    c.scene.terrain.flat_patch_sampling = {"init_pos": sampling()}
    with pytest.raises(ValueError, match="flat_patch_sampling"):
        flatten_cfg(c)
    # patches without the reset term are found and exposed, and nothing else changes; none at all: nothing
    c = MushrElevationTerrainLevelsEnvCfg()
    c.scene.terrain.terrain_generator.flat_patch_sampling = {"target": sampling()}
    assert flatten_cfg(c).extra["flat_patches"] == dict(names=["target"], sampling=None, spawn=False)
    assert flatten_cfg(MushrElevationTerrainLevelsEnvCfg()).extra["flat_patches"] is None
    assert flatten_cfg(MushrElevationRLEnvCfg()).extra["flat_patches"] is None


OVERRIDES = ["env_setup.num_envs=64", "env.scene.terrain.terrain_type=generator",
             "env.scene.terrain.terrain_generator={'flat_patch_sampling': {'init_pos': {'num_patches': 8, 'patch_radius': 0.15, "
             "'max_height_diff': 0.02, 'x_range': (-0.4, 0.4), 'y_range': (-0.4, 0.4)}}}",
             "env.events.set_goal.func=reset_root_state_from_terrain", "env.events.set_goal.params.pose_range.x=(-0.1,0.1)",
             "env.events.set_goal.params.pose_range.y=(-0.1,0.1)", "env.commands.goal_pose.ranges.pos_x=(-3.5,3.5)",
             "env.commands.goal_pose.ranges.pos_y=(-3.5,3.5)"]


def test_training_script_overrides_switch_the_patches_on():
    """what `scripts/train_rl.py -r RSS_ELEV_CONFIG <overrides>` resolves (README): with and without the terrain-levels term"""
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.flatten import flatten_cfg
    for extra in ([], ["env.curriculum.terrain_levels=terrain_levels_goal", "env.scene.terrain.max_init_terrain_level=1"]):
        run = resolve_run("RSS_ELEV_CONFIG", OVERRIDES + extra)
        flat = flatten_cfg(run.env)
        assert run.env.events.set_goal.func is mdp.reset_root_state_from_terrain
        assert flat.extra["flat_patches"] == dict(names=["init_pos"], sampling=None, spawn=True) and ("terrain_levels" in flat.extra) == bool(extra)
        assert abs(flat.params.reset_xy - 0.1) < 1e-7 and flat.params.cmd_xy == 3.5
    with pytest.raises(ValueError, match="not an event term"):
        flatten_cfg(resolve_run("RSS_ELEV_CONFIG", OVERRIDES[:3] + ["env.events.set_goal.func=time_out"]).env)


def test_training_config_carries_the_redeal_interval():
    from wheeledlab_amd.configs.runs import resolve_run
    assert resolve_run("RSS_ELEV_CONFIG", []).train.patch_redeal_interval == 1
    assert resolve_run("RSS_ELEV_CONFIG", ["train.patch_redeal_interval=4"]).train.patch_redeal_interval == 4

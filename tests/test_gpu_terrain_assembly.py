"""field.assemble_terrain against the env that calls it, in its three table layouts -- the curriculum's grid, a generated grid as one
row, a height array as one tile -- bit for bit, without writing into the config's entries; and the three TerrainLevels constructors
setting one set of attributes.  8 envs on a generated field of 2 x 3 tiles of 47 x 38 points (tests/terrain_gen_reference.py's tile)."""
import numpy as np
import pytest
import torch

from wheeledlab_amd.envs import terrain_gen_cfg as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, ROWS, COLS, P = 8, 7, 2, 3, 4
# the spawn square's corner stays on the patch (sqrt(2) * 0.1 <= 0.15 m) and the goal square about the outermost patch centre (0.4 m from
# its tile's centre) on the lattice: 0.4 + 0.5 <= 0.95 (half the shorter tile side) + 0.15 (the border)
RESET_XY, CMD_XY, WINDOW = 0.1, 0.5, (-0.4, 0.4)


def sampling(**kw):
    return G.FlatPatchSamplingCfg(**{**dict(num_patches=P, max_tries=256, x_range=WINDOW, y_range=WINDOW), **kw})


def generator_cfg():
    return G.TerrainGeneratorCfg(seed=4, num_rows=ROWS, num_cols=COLS, size=(2.35, 1.9), border_width=0.15,
                                 flat_patch_sampling={"init_pos": sampling(), "target": sampling(num_patches=3)})


def env_cfg(case: str):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.tasks.elevation import MushrElevationRLEnvCfg, MushrElevationTerrainLevelsEnvCfg
    cfg = MushrElevationTerrainLevelsEnvCfg() if case == "curriculum" else MushrElevationRLEnvCfg()
    cfg.sim.device, cfg.num_envs, cfg.scene.num_envs, cfg.seed = DEV, N, N, SEED
    cfg.events.set_goal.func = mdp.reset_root_state_from_terrain
    cfg.events.set_goal.params["pose_range"].update(x=(-RESET_XY, RESET_XY), y=(-RESET_XY, RESET_XY))
    cfg.commands.goal_pose.ranges.pos_x = cfg.commands.goal_pose.ranges.pos_y = (-CMD_XY, CMD_XY)
    t = cfg.scene.terrain
    if case == "array":          # the generated field's heights as a plain array: one tile, its windows about the field's centre
        from wheeledlab_amd.field import generate_heightfield
        hf = generate_heightfield(generator_cfg(), DEV)
        t.heightfield = (hf.heights.cpu().numpy(), hf.x0, hf.y0, hf.cell)
        t.flat_patch_sampling = {"init_pos": sampling(), "target": sampling(num_patches=3)}
    else:
        t.terrain_type, t.terrain_generator = "generator", generator_cfg()
    return cfg


@pytest.mark.parametrize("case", ["curriculum", "generator", "array"])
def test_assembly_equals_what_the_env_holds(case):
    from wheeledlab_amd import registry
    from wheeledlab_amd.field import DeviceHeightField, assemble_terrain
    env = registry.make("Isaac-MushrElevationRL-v0", cfg=env_cfg(case))
    b, extra = env._batch, env._flat.extra
    assert (extra.get("terrain_levels") is not None) == (case == "curriculum") and (extra["terrain_generator"] is None) == (case == "array")
    before = dict(extra)
    hf, levels, patches = assemble_terrain(extra, env._flat.params.cmd_xy, N, DEV, 0, N, SEED)
    assert list(extra) == list(before) and all(extra[k] is before[k] for k in before)
    assert isinstance(hf, DeviceHeightField) and torch.equal(hf.codes, b.hf.codes) and hf.z_scale == b.hf.z_scale
    assert sorted(patches) == sorted(b.flat_patches) == ["init_pos", "target"]
    for name, fp in patches.items():
        mine = b.flat_patches[name]
        assert fp.hf is hf and (fp.n_tiles, fp.n_patches, fp.seed) == (mine.n_tiles, mine.n_patches, mine.seed) == (
            1 if case == "array" else ROWS * COLS, P if name == "init_pos" else 3, mine.seed)
        for what in ("xy", "z", "tries"):
            got, want = getattr(fp, what), getattr(mine, what)
            assert got.data_ptr() != want.data_ptr() and torch.equal(got, want), (name, what)
    assert patches["init_pos"].seed == SEED and patches["target"].seed not in (SEED, 0)
    for lv, fp in ((levels, patches["init_pos"]), (b.levels, b.flat_patches["init_pos"])):
        assert lv.origins.data_ptr() == fp.xy.data_ptr() and lv.patches is fp               # the finder's own buffer
        assert (lv.rows, lv.tile_cols, lv.cols, lv.grid) == {"curriculum": (ROWS, COLS, COLS * P, None), "generator": (1, ROWS * COLS, ROWS * COLS * P, (ROWS, COLS)),
                                                            "array": (1, 1, P, None)}[case]
    for what in ("level", "type", "origins", "tile_origins"):
        assert torch.equal(getattr(levels, what), getattr(b.levels, what)), what
    assert (levels.env_offset, levels.world_envs, levels.seed, levels.max_init_terrain_level) == (
        b.levels.env_offset, b.levels.world_envs, b.levels.seed, b.levels.max_init_terrain_level) == (0, N, SEED, 1 if case == "curriculum" else 0)
    assert len(torch.unique(levels.type)) > 1                                               # (the deal ran: not the zeros it starts from)


def test_every_terrain_levels_constructor_sets_the_same_attributes():
    from wheeledlab_amd.envs import terrain_levels as TL
    from wheeledlab_amd.field import TerrainLevels, find_flat_patches, generate_heightfield
    gen = generator_cfg()
    fp = find_flat_patches(generate_heightfield(gen, DEV), gen, SEED)
    level, types = TL.initial_assignment(gen, N)
    made = {"config": TerrainLevels(gen, N, DEV), "config, patches": TerrainLevels(gen, N, DEV, flat_patches=fp),
            "on_patches": TerrainLevels.on_patches(fp, N, 1, ROWS * COLS, tile_origins=TL.tile_origins(gen), device=DEV, grid=(ROWS, COLS)),
            "from_tables": TerrainLevels.from_tables(level, types, TL.tile_origins(gen), ROWS, COLS, device=DEV)}
    names = set(vars(made["config"]))
    assert {"level", "type", "origins", "struct", "rows", "cols", "tile_cols", "tile_origins", "grid", "patches", "n_patches", "env_offset",
            "world_envs", "seed", "max_init_terrain_level", "device"} <= names
    for how, tl in made.items():
        assert set(vars(tl)) == names, how
        assert (tl.patches, tl.n_patches) == ((fp, P) if "patches" in how else (None, 1)), how
        assert (tl.env_offset, tl.world_envs, tl.seed) == (0, N, 42) and tl.grid_shape == (ROWS, COLS), how
    np.testing.assert_array_equal(made["config"].level.cpu().numpy(), made["config, patches"].level.cpu().numpy())

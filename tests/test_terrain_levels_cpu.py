"""Terrain curriculum, host side: the origins table, the initial assignment, the config checks, the reference against the oracle it
is composed from, and the C layout of the new member."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import elev_step as OS
from oracle import heightfield as OH
from tests import terrain_levels_reference as REF
from wheeledlab_amd import _abi as A
from wheeledlab_amd.envs import terrain_levels as TL
from wheeledlab_amd.envs.terrain_gen_cfg import TerrainGeneratorCfg, lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(**kw):
    return TerrainGeneratorCfg(**{**dict(seed=1, num_rows=3, num_cols=2, size=(3.2, 1.6), border_width=1.0), **kw})


def test_origins_are_the_tile_centres_of_the_lattice():
    c = cfg()
    g = lattice(c)
    o = TL.tile_origins(c)
    assert o.shape == (6, 2) and o.dtype == np.float32
    for row in range(3):
        for col in range(2):
            x = g["x0"] + (g["border"] + (row + 0.5) * g["tile_nx"]) * g["cell"]
            y = g["y0"] + (g["border"] + (col + 0.5) * g["tile_ny"]) * g["cell"]
            np.testing.assert_array_equal(o[row * 2 + col], np.float32([x, y]))
    # rows advance along x, columns along y; the grid is centred
    assert np.all(np.diff(o.reshape(3, 2, 2)[:, 0, 0]) > 0) and np.all(np.diff(o.reshape(3, 2, 2)[0, :, 1]) > 0)
    np.testing.assert_allclose(o.reshape(3, 2, 2)[1, :, 0], 0.0, atol=1e-6)


def test_initial_assignment():
    c = cfg(num_rows=5, num_cols=4)
    level, types = TL.initial_assignment(c, 64, max_init_terrain_level=2, seed=7)
    assert level.dtype == np.int32 and types.dtype == np.int32
    np.testing.assert_array_equal(types, np.repeat(np.arange(4), 16))            # contiguous blocks, IsaacLab's floor(arange / (n / cols))
    assert level.min() >= 0 and level.max() <= 2 and len(np.unique(level)) == 3
    np.testing.assert_array_equal(level, TL.uniform_below(REF.PH.philox4x32(np.arange(64), 0, REF.S_LEVEL, 7)[0], 3))
    assert TL.initial_assignment(c, 64, max_init_terrain_level=99, seed=7)[0].max() <= 4       # clamped to rows - 1
    assert TL.initial_assignment(c, 64, max_init_terrain_level=0, seed=7)[0].max() == 0
    full = TL.initial_assignment(c, 4096, seed=7)[0]                                            # None: every row
    assert sorted(np.unique(full)) == [0, 1, 2, 3, 4]
    # two shards of 32 hold what the batch of 64 holds
    a, b = (TL.initial_assignment(c, 32, off, 64, 2, 7) for off in (0, 32))
    np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), level)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), types)
    with pytest.raises(ValueError, match="world_envs"):
        TL.initial_assignment(c, 32, 48, 64)
    # an env count that the columns do not divide
    np.testing.assert_array_equal(TL.initial_assignment(cfg(num_cols=3), 10)[1], np.arange(10) * 3 // 10)


def test_validation_errors_name_the_quantity():
    with pytest.raises(ValueError, match="generator"):
        TL.check_curriculum(None, 1.0, 1.0)
    with pytest.raises(ValueError, match="curriculum"):
        TL.check_curriculum(cfg(curriculum=False), 0.5, 0.5)
    with pytest.raises(ValueError, match="reset_xy"):
        TL.check_curriculum(cfg(), 0.9, 0.5)               # the shorter tile side is 1.6 m
    with pytest.raises(ValueError, match="cmd_xy"):
        TL.check_curriculum(cfg(), 0.8, 1.9)               # 0.8 m tile half + 1 m frame in y
    TL.check_curriculum(cfg(), 0.8, 1.7)


def test_reference_with_one_tile_at_the_origin_is_the_oracle():
    n, seed = 64, 5
    hf = OH.make_terrain()
    p = OS.elev_params()
    p.max_episode_length = 2                               # resets inside the three steps
    p.cmd_resample_s = 0.25                                # and a resampled goal
    states = []
    for levels in (None, dict(level=np.zeros(n, np.int32), type=np.zeros(n, np.int32), origins=np.zeros((1, 2), np.float32), rows=1, cols=1)):
        st = OS.init_state(p, n, seed)
        ep = np.zeros(n, np.int32)
        OS.reset_envs(p, st, ep, hf, np.arange(n), seed, 0)
        OS.update_command(st)
        outs = []
        rng = np.random.RandomState(0)
        for k in range(3):
            a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
            outs.append(REF.step(p, st, ep, hf, a, seed, k, levels)[:4])
        states.append((st, ep, outs))
        if levels is not None:
            assert not levels["level"].any()
    (sa, ea, oa), (sb, eb, ob) = states
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(ea, eb)
    assert (ea == 0).any()
    for x, y in zip(oa, ob):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


def test_level_rule():
    lv = dict(level=np.array([0, 1, 2, 2, 1, 0, 1], np.int32), type=np.zeros(7, np.int32), origins=np.zeros((3, 2), np.float32), rows=3, cols=1)
    goal = np.array([1, 1, 1, 0, 0, 0, 1], bool)
    fail = np.array([0, 0, 0, 1, 0, 1, 1], bool)
    got = REF.next_levels(lv, np.arange(7), goal, fail, 11, 4)
    wrap = TL.uniform_below(TL.philox_word0(np.arange(7), 4, TL.LEVEL_STREAM, 11), 3)[2]
    np.testing.assert_array_equal(got, [1, 2, wrap, 1, 1, 0, 2])
    assert 0 <= wrap < 3
    np.testing.assert_array_equal(TL.philox_word0(np.arange(7), 4, 3, 11), REF.PH.philox4x32(np.arange(7), 4, 3, 11)[0])


def test_terrain_levels_layout_matches_header(tmp_path):
    probe = tmp_path / "probe.c"
    fields = [n for n, _ in A.WlTerrainLevels._fields_]
    body = " ".join(f'printf("%zu ", offsetof(WlTerrainLevels, {n}));' for n in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd.h"\n'
                     f'int main(){{{body} printf("%zu %zu %zu %d\\n", sizeof(WlTerrainLevels), offsetof(WlElevParams, levels), sizeof(WlElevParams),'
                     ' (int)WL_ABI_REVISION); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(A.WlTerrainLevels, n).offset for n in fields] + [C.sizeof(A.WlTerrainLevels), A.WlElevParams.levels.offset,
                                                                     C.sizeof(A.WlElevParams), A.WL_ABI_REVISION]
    assert got == want
    assert A.WlElevParams._fields_[-1][0] == "levels"            # the trailing member: everything before it is where it was
    from wheeledlab_amd.params import elev_params
    z = elev_params().levels
    assert not z.level and not z.type and not z.origins and z.rows == 0 and z.cols == 0      # off unless asked for


def test_training_script_overrides_switch_the_levels_on():
    """what `scripts/train_rl.py -r RSS_ELEV_CONFIG <overrides>` resolves (README): no new task id, no new run config"""
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.flatten import flatten_cfg
    ov = ["env_setup.num_envs=64", "env.scene.terrain.terrain_type=generator", "env.scene.terrain.terrain_generator={}",
          "env.scene.terrain.max_init_terrain_level=1", "env.events.set_goal.params.pose_range.x=(-1.5,1.5)",
          "env.events.set_goal.params.pose_range.y=(-1.5,1.5)", "env.commands.goal_pose.ranges.pos_x=(-3.5,3.5)",
          "env.commands.goal_pose.ranges.pos_y=(-3.5,3.5)", "env.curriculum.terrain_levels=terrain_levels_goal"]
    run = resolve_run("RSS_ELEV_CONFIG", ov)
    flat = flatten_cfg(run.env)
    assert flat.extra["terrain_levels"] == dict(name="terrain_levels", max_init_terrain_level=1)
    assert flat.extra["terrain_generator"].num_rows == 5 and flat.params.reset_xy == 1.5 and flat.params.cmd_xy == 3.5
    assert run.env.curriculum.terrain_levels.func is mdp.terrain_levels_goal
    assert [n for n, _ in flat.curriculum] == ["more_goal", "more_falling_pen"]          # not a boundary term: fused rollouts are not cut for it
    # without the term nothing changes; a wrong name and a missing generator are refused
    assert "terrain_levels" not in flatten_cfg(resolve_run("RSS_ELEV_CONFIG", ov[:-1]).env).extra
    with pytest.raises(ValueError, match="terrain_levels_goal"):
        flatten_cfg(resolve_run("RSS_ELEV_CONFIG", ov[:-1] + ["env.curriculum.terrain_levels=time_out"]).env)
    with pytest.raises(ValueError, match="generator"):
        flatten_cfg(resolve_run("RSS_ELEV_CONFIG", ["env.curriculum.terrain_levels=terrain_levels_goal"]).env)

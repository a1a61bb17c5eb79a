"""Flat patches on the GPU (include/wheeledlab_amd_terrain.h, csrc/wl_flat_patch.hip): the finder against the integer restatement
(tests/flat_patch_reference.py) on the device's own codes, exactly; its determinism across runs and redraws; the refusals; the step
kernels -- unchanged -- spawning on patches through the virtual-column tables, in every form against tests/terrain_levels_reference.py
under the predicates of tests/test_gpu_terrain_levels.py, step by step and as launches of several steps; the deal; a walled course;
and the env surface.  The finder tests here are the ones that cover the wavefront's part of the search -- the 64-bit ballot, the
lowest-set-bit pick, the masking of lanes past max_tries (100 is no multiple of 64) and rounds beyond the first: the host simulation
(tests/test_flat_patch_host_sim_cpu.py) runs the same header as a wavefront of ONE lane."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import flat_patch_reference as FR
import terrain_gen_reference as TR
from oracle import elev_step as OS
from tests import parity_predicates as PRED
from tests import terrain_levels_reference as REF
from tests import test_gpu_terrain_levels as LV
from wheeledlab_amd import _abi as A
from wheeledlab_amd.envs import terrain_gen_cfg as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, PATCH_SEED, P = 9, 5, 8
ROWS, COLS = LV.ROWS, LV.COLS
# the spawn square's corner stays on the patch: sqrt(2) * 0.1 <= 0.15 m; the goal square about the outermost patch centre (1.45 m from
# its tile's centre, tiles of 3.2 m inside a 1 m frame) stays on the lattice: 1.45 + 1.0 <= 1.6 + 1.0 - one cell
RADIUS, MAX_DIFF, RESET_XY, CMD_XY = 0.15, 0.02, 0.1, 1.0
PX, QW, TGT_X, CMD_TIMER = LV.PX, LV.QW, LV.TGT_X, LV.CMD_TIMER
# a spawn is origin + (2 u - 1) reset_xy rounded once to fp32: half an ulp of a coordinate below 4 m on top of reset_xy
SPAWN_SLACK = 2.0 ** -22


def sampling(**kw):
    return G.FlatPatchSamplingCfg(**{**dict(num_patches=P, patch_radius=RADIUS, max_height_diff=MAX_DIFF, max_tries=1024), **kw})


def reference_of(hf, table, n_patches, seed):
    """the restatement on the DEVICE's codes -> (xy, z, tries, ij)"""
    codes = hf.codes.cpu().numpy()
    ij, tries = FR.find(codes, table, n_patches, seed)
    xy, z = FR.outputs(codes, ij, hf.x0, hf.y0, hf.cell, hf.z_scale)
    return xy, z, tries, ij


def assert_equals_reference(fp, ref):
    np.testing.assert_array_equal(fp.tries.cpu().numpy(), ref[2])
    np.testing.assert_array_equal(fp.xy.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(fp.z.cpu().numpy(), ref[1])


# ---- 1. the finder ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_types():
    from wheeledlab_amd.core import generate_heightfield
    hf = generate_heightfield(TR.all_types_cfg(), DEV)
    torch.cuda.synchronize()
    return hf


@pytest.mark.parametrize("max_tries", [1024, 100])
def test_finder_equals_the_reference_on_the_devices_codes(all_types, max_tries):
    from wheeledlab_amd.core import find_flat_patches
    cfg = TR.all_types_cfg(flat_patch_sampling={"init_pos": sampling(max_tries=max_tries)})
    fp = find_flat_patches(all_types, cfg, PATCH_SEED)
    ref = reference_of(all_types, fp.table, P, PATCH_SEED)
    assert_equals_reference(fp, ref)
    tries = ref[2]
    assert (tries < 0).all(1).any() and (tries == 0).all(1).any() and (tries >= (64 if max_tries > 64 else 1)).any()      # the branches are there
    assert fp.failed == int((tries < 0).sum()) and tuple(fp.positions().shape) == (30, P, 3)
    # the stored height is the decoded grid's value at the patch
    ij = ref[3]
    np.testing.assert_array_equal(fp.z.cpu().numpy(), all_types.heights.cpu().numpy()[ij[..., 1], ij[..., 0]])


# ---- 2. determinism -----------------------------------------------------------------------------------------------------

def test_runs_and_redraws_give_the_same_bytes():
    from wheeledlab_amd.core import find_flat_patches, generate_heightfield
    cfg = TR.all_types_cfg(flat_patch_sampling={"init_pos": sampling()})
    hf = generate_heightfield(cfg, DEV)
    fp = find_flat_patches(hf, cfg, PATCH_SEED)
    first = [t.clone() for t in (fp.xy, fp.z, fp.tries)]
    ptrs = [t.data_ptr() for t in (fp.xy, fp.z, fp.tries)]
    for t in (fp.xy, fp.z, fp.tries):
        t.fill_(-3)
    fp.find()
    assert all(torch.equal(a, b) for a, b in zip(first, (fp.xy, fp.z, fp.tries)))
    hf.regenerate(cfg.seed + 8)                                   # the field's refresh() finds the patches again, in place
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in (fp.xy, fp.z, fp.tries)] == ptrs
    assert not torch.equal(fp.tries, first[2])
    assert_equals_reference(fp, reference_of(hf, fp.table, P, PATCH_SEED))
    hf.regenerate(cfg.seed)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, (fp.xy, fp.z, fp.tries)))
    # a set that is gone is not searched any more; a field without patches launches nothing for them
    del fp
    hf.refresh()
    assert hf._shared["patches"] == []


def test_a_redraw_that_moves_the_tile_types_resolves_the_table_again():
    """a sub-terrain's own sampling without a curriculum: another seed puts the searched type on other tiles.  The set resolves its table
    again from the field's config, into the same device buffer, and the search equals the reference on the NEW table"""
    from wheeledlab_amd.core import find_flat_patches, generate_heightfield
    subs = G.default_sub_terrains()
    subs["boxes"].flat_patch_sampling = {"init_pos": sampling(max_tries=256)}
    cfg = G.TerrainGeneratorCfg(seed=1, curriculum=False, num_rows=3, num_cols=4, size=(3.0, 3.0), border_width=0.5, sub_terrains=subs)
    hf = generate_heightfield(cfg, DEV)
    fp = find_flat_patches(hf, cfg, PATCH_SEED)
    old_table, tiles_ptr, xy_ptr = fp.table.copy(), fp.tiles.data_ptr(), fp.xy.data_ptr()
    assert_equals_reference(fp, reference_of(hf, fp.table, P, PATCH_SEED))
    hf.regenerate(2)
    torch.cuda.synchronize()
    want = G.patch_table(cfg.replace(seed=2), "init_pos")
    assert not np.array_equal(want[0], old_table) and np.array_equal(fp.table, want[0]) and fp.labels == want[3]
    assert (fp.tiles.data_ptr(), fp.xy.data_ptr()) == (tiles_ptr, xy_ptr)
    assert bytes(fp.tiles.cpu().numpy()) == want[0].tobytes()
    ref = reference_of(hf, want[0], P, PATCH_SEED)
    assert_equals_reference(fp, ref)
    names = G.tile_names(hf.generator)
    searched = np.array([n == "boxes" for n in names])
    assert (ref[2][~searched] < 0).all() and (ref[2][searched] >= 0).any() and fp.failed == int((ref[2][searched] < 0).sum())
    # a config that changes the counts cannot keep the addresses; one that lays other tiles out without the sampling is refused too
    with pytest.raises(ValueError, match="fixed addresses"):
        subs4 = G.default_sub_terrains()
        subs4["boxes"].flat_patch_sampling = {"init_pos": sampling(num_patches=4)}
        hf.regenerate(cfg.replace(sub_terrains=subs4))
    with pytest.raises(ValueError, match="neither carries the sampling"):
        hf.regenerate(cfg.replace(sub_terrains=G.default_sub_terrains()))
    hf.regenerate(cfg)
    torch.cuda.synchronize()
    assert np.array_equal(fp.table, old_table)
    assert_equals_reference(fp, reference_of(hf, old_table, P, PATCH_SEED))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(all_types):
    from wheeledlab_amd.core import find_flat_patches
    lib = A.load()
    hf = all_types
    fp = find_flat_patches(hf, TR.all_types_cfg(flat_patch_sampling={"init_pos": sampling(max_tries=64)}), PATCH_SEED)
    outs = (fp.xy, fp.z, fp.tries)
    for t in outs:
        t.fill_(-3)
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good_ptrs = [fp.tiles.data_ptr(), fp.xy.data_ptr(), fp.z.data_ptr(), fp.tries.data_ptr()]

    def field(**kw):
        s = hf.struct
        v = {n: getattr(s, n) for n, _ in A.WlHeightField._fields_}
        v.update(kw)
        return A.WlHeightField(*[v[n] for n, _ in A.WlHeightField._fields_])

    def call(hf_=None, p=None, ptrs=None):
        return lib.wl_flat_patches(C.byref(hf_ or field()), C.byref(p or fp.params), *[C.c_void_p(q) if q else None for q in (ptrs or good_ptrs)], stream)

    rcs = [call(hf_=field(**kw)) for kw in (dict(height=None), dict(nx=0), dict(ny=0), dict(cell=0.0), dict(cell=float("nan")), dict(z_scale=0.0),
                                           dict(x0=float("inf")))]
    rcs += [call(p=A.WlFlatPatchParams(*v)) for v in ((0, P, 14, 0, 5), (30, 0, 14, 0, 5), (-1, P, 14, 0, 5), (1 << 12, (1 << 10) + 1, 14, 0, 5), (30, P, 14, 1, 5))]
    rcs += [call(ptrs=[None if i == k else q for i, q in enumerate(good_ptrs)]) for k in range(4)]
    assert rcs == [-1] * len(rcs)
    assert [call(ptrs=[q + 2 if i == k else q for i, q in enumerate(good_ptrs)]) for k in range(4)] == [-3] * 4
    assert call(hf_=field(height=hf.struct.height + 1)) == -3
    assert lib.wl_flat_patches(None, C.byref(fp.params), *[C.c_void_p(q) for q in good_ptrs], stream) == -1
    assert lib.wl_flat_patches(C.byref(field()), None, *[C.c_void_p(q) for q in good_ptrs], stream) == -1
    # the deal
    types = torch.full((70,), -3, dtype=torch.int32, device=DEV)
    deal = lambda n=70, off=0, world=70, cols=2, pp=P, out=types.data_ptr(): lib.wl_flat_patch_deal(  # noqa: E731
        n, off, world, cols, pp, 0, SEED, C.c_void_p(out) if out else None, stream)
    assert [deal(**kw) for kw in (dict(n=-1), dict(off=-1), dict(world=0), dict(world=69), dict(off=1), dict(cols=0), dict(pp=0),
                                  dict(cols=1 << 16, pp=(1 << 14) + 1), dict(out=None))] == [-1] * 9
    assert deal(out=types.data_ptr() + 2) == -3
    torch.cuda.synchronize()
    assert all(bool((t == -3).all()) for t in outs + (types,))
    assert call() == 0 and deal() == 0                             # ... and the same calls, unbroken, write
    torch.cuda.synchronize()
    assert not bool((fp.tries == -3).any()) and not bool((types == -3).any())


# ---- 4. the step kernels on virtual columns --------------------------------------------------------------------------------

def steps_cfg():
    return LV.gen_cfg().replace(flat_patch_sampling={"init_pos": sampling()})


def params(p):
    p.reset_xy, p.cmd_xy = RESET_XY, CMD_XY
    return p


@pytest.fixture(scope="module")
def patched_field():
    from wheeledlab_amd.core import find_flat_patches, generate_heightfield
    hf = generate_heightfield(steps_cfg(), DEV)
    fp = find_flat_patches(hf, steps_cfg(), PATCH_SEED)
    torch.cuda.synchronize()
    ref = reference_of(hf, fp.table, P, PATCH_SEED)
    print("[flat-patch] 3 x 2 grid, accepted attempts:", ref[2].tolist())
    assert (ref[2] >= 0).all()                                     # from the reference: every slot of the 48 found its patch
    assert_equals_reference(fp, ref)
    assert fp.failed == 0
    return hf, fp, (hf.heights.cpu().numpy().copy(), hf.x0, hf.y0, hf.cell, hf.outside_z)


def make_env(hf, fp, n, env_offset=0, world=None):
    from wheeledlab_amd import params as PP
    from wheeledlab_amd.core import ElevBatch, TerrainLevels
    tl = TerrainLevels(steps_cfg(), n, DEV, env_offset, world, None, SEED, flat_patches=fp)
    env = ElevBatch(n, device=DEV, params=params(PP.elev_params()), seed=SEED, env_offset=env_offset, heightfield=hf, terrain_levels=tl)
    env.reset()
    return env


def force_resets(env):
    """time-outs in the first and in the second step, goals resampled in the first (cars spawned at rest under throttle add their own ends)"""
    n = env.n
    env.episode_len[0:n:3] = env.p.max_episode_length - 1
    env.episode_len[1:n:3] = env.p.max_episode_length - 2
    env.state[CMD_TIMER, 2:n:3] = 0.05
    torch.cuda.synchronize()


def trajectory(env, form, K):
    """K single steps -> [(state before, outputs, state after)], snapshots = (state, episode_len, level)"""
    out = []
    for _ in range(K):
        pre = LV.snapshot(env)
        obs, rew, term, trunc = LV.run(env, form, 1)
        out.append((pre, (obs[0], rew[0], term[0], trunc[0]), LV.snapshot(env)))
    return out


def own_patch(env, fp, level):
    """[n, 2]: the patch of every env's slot on the tile of `level`"""
    t, tl = env.levels.type.cpu().numpy().astype(np.int64), env.levels
    return fp.xy.cpu().numpy()[level.astype(np.int64) * tl.tile_cols + t // tl.n_patches, t % tl.n_patches]


K_STEPS = 3


@pytest.mark.parametrize("n", [64, 70])
def test_every_form_spawns_on_patches_and_equals_the_reference(patched_field, n):
    hf, fp, hf_np = patched_field
    first = None
    for form in LV.FORMS:
        env = make_env(hf, fp, n)
        tl = env.levels
        assert tl.cols == COLS * P and tl.origins.data_ptr() == fp.xy.data_ptr() and tl.tile_cols == COLS and tuple(tl.tile_origins.shape) == (6, 2)
        types = tl.type.cpu().numpy()
        np.testing.assert_array_equal(types, FR.deal(np.arange(n), COLS, n, P, 0, SEED))
        np.testing.assert_array_equal(tl.terrain_types.cpu().numpy(), types // P)
        st0 = env.state.cpu().numpy()
        assert (np.abs(st0[PX:PX + 2, :n].T - own_patch(env, fp, tl.level.cpu().numpy())) <= RESET_XY + SPAWN_SLACK).all(), form
        force_resets(env)
        steps = trajectory(env, form, K_STEPS)
        # the reference: each step from the state THIS form stood in before it
        refs, origins = [], fp.xy.cpu().numpy().reshape(-1, 2)
        for k, (pre, _, _) in enumerate(steps):
            st, ep, lv = (x.copy() for x in pre)
            stride = st.shape[1]
            levels = dict(level=np.zeros(stride, np.int32), type=np.zeros(stride, np.int32), origins=origins, rows=ROWS, cols=COLS * P)
            levels["level"][:n], levels["type"][:n] = lv, types
            a = np.zeros((stride, 2), np.float32)
            a[:] = LV.ACTION
            st[:, n:] = 0
            st[QW, n:] = 1
            probe = {}
            o_obs, o_rew, o_term, o_trunc, _ = REF.step(params(OS.elev_params()), st, ep, hf_np, a, SEED, k, levels, probe=probe)
            refs.append(dict(state=st, ep=ep, level=levels["level"][:n].copy(), obs=o_obs[:n], rew=o_rew[:n], term=o_term[:n], trunc=o_trunc[:n],
                             probe=probe))
        if first is None:
            first = steps
        else:
            # how far the forms stand apart (printed: with a reset_xy that is no power of two the spawn's product is not exact, and a
            # form that contracts origin + (2 u - 1) reset_xy places it an ulp from one that does not)
            gap = [float(np.nanmax(np.abs(a[2][0][:41, :n] - b[2][0][:41, :n]))) for a, b in zip(steps, first)]
            rows = np.nonzero(np.nanmax(np.abs(steps[0][2][0][:41, :n] - first[0][2][0][:41, :n]), 1) > 0)[0].tolist()
            print(f"[flat-patch] n {n}: {form} against {LV.FORMS[0]}: largest state difference per step {gap}; rows differing after step 0: {rows}")
        ended_any = np.zeros(n, bool)
        for k, ((pre, (obs, rew, term, trunc), (got, ep, lv)), ref) in enumerate(zip(steps, refs)):
            where = f"{form} step {k}"
            np.testing.assert_array_equal(lv, ref["level"], err_msg=where)
            np.testing.assert_array_equal(term, ref["term"], err_msg=where)
            np.testing.assert_array_equal(trunc, ref["trunc"], err_msg=where)
            np.testing.assert_array_equal(ep[:n], ref["ep"][:n], err_msg=where)
            ok, n_ex = PRED.check_state(got, ref["state"], ref["probe"], n, np.ones(n, bool), where=where)
            assert n_ex <= 1, (where, n_ex)
            assert PRED.state_error(got, ref["state"], n)[:, ok].max() <= 1.0, where
            np.testing.assert_allclose(got[35:41, :n][:, ok], ref["state"][35:41, :n][:, ok], rtol=5e-4, atol=2e-3, err_msg=where)
            np.testing.assert_allclose(rew[ok], ref["rew"][ok], rtol=2e-3, atol=5e-2, err_msg=where)
            d = np.abs(obs - ref["obs"])[ok]
            d[:, 2:5] = np.minimum(d[:, 2:5], np.abs(2 * np.pi - d[:, 2:5]))
            assert d[:, :13].max() < 3e-3, (where, d[:, :13].max())
            scan_bad = d[:, 13:] > 2e-3
            assert scan_bad.sum() <= 4 and scan_bad.any(1).sum() <= 2, (where, int(scan_bad.sum()))
            # after a reset the car stands within reset_xy of its own patch of the tile its level now names; goals about the same patch
            ended = term | trunc
            ended_any |= ended
            o = own_patch(env, fp, lv)
            assert (np.abs(got[PX:PX + 2, :n].T - o)[ended] <= RESET_XY + SPAWN_SLACK).all(), where
            redrawn = ended | (pre[0][CMD_TIMER, :n] <= 0.1)
            assert (np.abs(got[TGT_X:TGT_X + 2, :n].T - o)[redrawn] <= CMD_XY + SPAWN_SLACK).all(), where
            if form != LV.FORMS[0]:                               # the discrete outcome is the same in every form
                assert np.array_equal(term, first[k][1][2]) and np.array_equal(trunc, first[k][1][3]) and np.array_equal(lv, first[k][2][2]), where
        assert ended_any[0:n:3].all() and ended_any[1:n:3].all() and len(np.unique(steps[-1][2][2])) > 1, form


@pytest.mark.parametrize("form", ["rollout", "persistent", "collect"])
def test_one_launch_of_k_steps_equals_k_launches_on_patches(patched_field, form):
    """the launches that span several steps -- a reset onto a patch and the steps after it inside ONE launch -- against the same form
    stepped singly (which the test above holds to the reference step by step): every output and the whole state, bit for bit"""
    hf, fp, _ = patched_field
    n, K = 70, 6
    envs = [make_env(hf, fp, n) for _ in range(2)]
    for env in envs:
        force_resets(env)
        env.episode_len[n // 2:n] = env.p.max_episode_length - 1 - torch.arange(n - n // 2, device=DEV, dtype=torch.int32) % (K - 1)
    many = LV.run(envs[0], form, K)
    single = [LV.run(envs[1], form, 1) for _ in range(K)]       # (the same form: across forms a spawn may differ in its last bit)
    single = tuple(np.concatenate([x[i] for x in single]) for i in range(4))
    assert LV.same(many, single)
    assert LV.same(LV.snapshot(envs[0]), LV.snapshot(envs[1]))
    ended = many[2] | many[3]
    assert ended[:K - 1].any(1).all() and ended[:, n // 2:].any(0).all()         # resets in the launch's early steps, stepped on within it
    st, lv = envs[0].state.cpu().numpy(), envs[0].levels.level.cpu().numpy()
    fresh = ended[K - 1]
    assert (np.abs(st[PX:PX + 2, :n].T - own_patch(envs[0], fp, lv))[fresh] <= RESET_XY + SPAWN_SLACK).all()


# ---- 5. the deal ---------------------------------------------------------------------------------------------------------

def test_redeal_equals_the_reference_in_two_shards(patched_field):
    from wheeledlab_amd.core import TerrainLevels
    hf, fp, _ = patched_field
    n, parts = 70, ((0, 32), (32, 38))
    shards = [TerrainLevels(steps_cfg(), m, DEV, off, n, None, SEED, flat_patches=fp) for off, m in parts]
    whole = TerrainLevels(steps_cfg(), n, DEV, 0, n, None, SEED, flat_patches=fp)
    for epoch in (0, 3, 2 ** 33 + 1):
        for tl in shards + [whole]:
            level = tl.level.clone()
            tl.redeal(epoch)
            assert torch.equal(tl.level, level)
        want = FR.deal(np.arange(n), COLS, n, P, epoch, SEED)
        np.testing.assert_array_equal(whole.type.cpu().numpy(), want)
        np.testing.assert_array_equal(torch.cat([s.type for s in shards]).cpu().numpy(), want)
        np.testing.assert_array_equal(whole.terrain_types.cpu().numpy(), np.arange(n) * COLS // n)
    assert len({tuple(FR.deal(np.arange(n), COLS, n, P, e, SEED)) for e in (0, 3)}) == 2


# ---- 6. a walled course ------------------------------------------------------------------------------------------------------

def test_no_patch_and_no_car_by_the_wall():
    """a 40 x 33-point field (what a rasterised OBJ course is to the kernels) with a wall 0.3 m high across it: the one-row table"""
    from wheeledlab_amd import params as PP
    from wheeledlab_amd.core import DeviceHeightField, ElevBatch, TerrainLevels, find_flat_patches
    nx, ny, cell, z_scale = 40, 33, 0.05, 2.0 ** -13
    wall = (18, 21)                                                 # lattice columns i of the wall, inclusive
    codes = np.full((ny, nx), 819, np.int16)                        # 0.1 m
    codes[:, wall[0]:wall[1] + 1] = 819 + 2458                      # + 0.3 m
    hf = DeviceHeightField((codes, -1.0, -0.8, cell, z_scale), DEV)
    fp = find_flat_patches(hf, sampling(num_patches=16, max_tries=256), PATCH_SEED)
    ref = reference_of(hf, fp.table, 16, PATCH_SEED)
    assert_equals_reference(fp, ref)
    assert (ref[2] >= 0).all() and (ref[2] > 0).any() and fp.failed == 0      # some first attempts met the wall and were turned down
    i = ref[3][..., 0]
    assert ((i < wall[0] - 3) | (i > wall[1] + 3)).all()                      # no disc of 3 cells touches the wall
    n = 64
    tl = TerrainLevels.on_patches(fp, n, device=DEV, seed=SEED)
    assert (tl.rows, tl.cols, tl.tile_cols) == (1, 16, 1) and len(np.unique(tl.type.cpu().numpy())) > 8
    p = params(PP.elev_params())
    p.cmd_xy = 0.5
    env = ElevBatch(n, device=DEV, params=p, seed=SEED, heightfield=hf, terrain_levels=tl)
    env.reset()
    env.episode_len[:] = env.p.max_episode_length - 1              # everybody ends in the step and is reset by the kernel
    a = torch.zeros(n, 2, device=DEV)
    for form in (1, 4, 0):
        env.set_lanes(form)
        _, _, term, trunc = env.step(a)
        torch.cuda.synchronize()
        assert bool((term | trunc).all())
        env.episode_len[:] = env.p.max_episode_length - 1
        x = env.state[PX, :n].cpu().numpy().astype(np.float64)
        xw = (-1.0 + wall[0] * cell, -1.0 + wall[1] * cell)
        gap = np.where(x < xw[0], xw[0] - x, x - xw[1])
        # a patch centre is at least 4 cells from the wall's nearest column, the car within reset_xy of it
        assert (gap >= 4 * cell - RESET_XY - SPAWN_SLACK).all(), (form, gap.min())
        assert bool((env.levels.level == 0).all())                  # one row: the level stays where it is
        o = own_patch(env, fp, np.zeros(n, np.int64))
        assert (np.abs(env.state[PX:PX + 2, :n].cpu().numpy().T - o) <= RESET_XY + SPAWN_SLACK).all()


# ---- 7. the env surface ----------------------------------------------------------------------------------------------------

def patch_env_cfg(n=64, seed=7, **kw):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.tasks.elevation import MushrElevationTerrainLevelsEnvCfg
    cfg = MushrElevationTerrainLevelsEnvCfg()
    cfg.sim.device, cfg.num_envs, cfg.scene.num_envs, cfg.seed = DEV, n, n, seed
    cfg.events.set_goal.func = mdp.reset_root_state_from_terrain
    cfg.events.set_goal.params["pose_range"].update(x=(-0.1, 0.1), y=(-0.1, 0.1))
    cfg.scene.terrain.terrain_generator.flat_patch_sampling = {
        "init_pos": sampling(**{**dict(x_range=(-0.4, 0.4), y_range=(-0.4, 0.4)), **kw}), "target": sampling(num_patches=3, max_tries=64)}
    return cfg


def test_env_surface_and_two_ppo_iterations():
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    spec = importlib.util.spec_from_file_location("train_rl", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_rl.py"))
    train_rl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_rl)
    n = 64
    env = registry.make("Isaac-MushrElevationRL-v0", cfg=patch_env_cfg(n))
    env.reset()
    b, t = env._batch, env.scene.terrain
    fp = b.flat_patches["init_pos"]
    pos = t.flat_patches["init_pos"]
    assert tuple(pos.shape) == (5, 5, P, 3) and tuple(t.flat_patches["target"].shape) == (5, 5, 3, 3) and sorted(t.flat_patches) == ["init_pos", "target"]
    assert torch.equal(pos[..., :2].reshape(25, P, 2), fp.xy) and b.levels.origins.data_ptr() == fp.xy.data_ptr()
    assert_equals_reference(fp, reference_of(b.hf, fp.table, P, 7))
    types = t.terrain_types
    assert types.dtype == torch.int32 and 0 <= int(types.min()) and int(types.max()) < 5
    assert torch.equal(types, torch.div(b.levels.type, P, rounding_mode="floor"))
    assert t.terrain_levels.data_ptr() == b.levels.level.data_ptr() and int(t.terrain_levels.max()) <= 1
    assert tuple(t.terrain_origins.shape) == (5, 5, 3) and tuple(env.scene.env_origins.shape) == (n, 3)
    # every car stands within reset_xy of its own patch, and its tile's centre is the env's origin
    own = fp.xy[b.levels.level.long() * 5 + types.long(), (b.levels.type % P).long()]
    assert bool(((b.state[PX:PX + 2, :n].T - own).abs() <= 0.1 + SPAWN_SLACK).all())
    assert bool(((own - env.scene.env_origins[:, :2]).abs() <= 0.4 + 2.0 ** -18).all())      # (two fp32 ulps of coordinates below 32 m)
    # a redraw finds the patches again in place and deals again
    before, type0 = fp.xy.clone(), b.levels.type.clone()
    env.regenerate_terrain()
    assert b.levels.origins.data_ptr() == fp.xy.data_ptr() and not torch.equal(fp.xy, before) and not torch.equal(b.levels.type, type0)
    assert_equals_reference(fp, reference_of(b.hf, fp.table, P, 7))
    own = fp.xy[b.levels.level.long() * 5 + t.terrain_types.long(), (b.levels.type % P).long()]
    assert bool(((b.state[PX:PX + 2, :n].T - own).abs() <= 0.1 + SPAWN_SLACK).all())
    # two PPO iterations through the collector launch, the patches dealt again before the second
    assert env.can_collect_rollout()
    env.action_space.low, env.action_space.high = -1.0, 1.0
    torch.manual_seed(0)
    hook = train_rl.patch_redealer(env, 1)
    assert hook is not None and train_rl.patch_redealer(env, 0) is None
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ClipAction(env)), registry.load_cfg_from_registry("Isaac-MushrElevationRL-v0", "rsl_rl_cfg_entry_point"),
                            device=DEV)
    type1 = b.levels.type.clone()
    hist = runner.learn(2, verbose=False, before_iteration=hook)
    assert len(hist) == 2 and all(np.isfinite(h["value_function"]) for h in hist) and all("Curriculum/terrain_levels" in h for h in hist)
    np.testing.assert_array_equal(b.levels.type.cpu().numpy(), FR.deal(np.arange(n), 5, n, P, 1, 7))
    assert not torch.equal(b.levels.type, type1) and torch.equal(t.terrain_types, torch.div(type1, P, rounding_mode="floor"))


def test_patches_without_levels_are_exposed_and_the_rest_says_why():
    """a "target" set alone: no reset term spawns on it, no curriculum -- the batch carries no level tables"""
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.tasks.elevation import MushrElevationRLEnvCfg
    cfg = MushrElevationRLEnvCfg()
    cfg.sim.device, cfg.num_envs, cfg.scene.num_envs, cfg.seed = DEV, 64, 64, 7
    cfg.scene.terrain.terrain_type = "generator"
    cfg.scene.terrain.terrain_generator = G.TerrainGeneratorCfg(flat_patch_sampling={"target": sampling(num_patches=3, max_tries=64)})
    env = registry.make("Isaac-MushrElevationRL-v0", cfg=cfg)
    env.reset()
    t = env.scene.terrain
    assert env._batch.levels is None and tuple(t.flat_patches["target"].shape) == (5, 5, 3, 3) and t.terrain_type == "generator"
    for name in ("terrain_levels", "terrain_types", "terrain_origins", "env_origins"):
        with pytest.raises(RuntimeError, match="carries no terrain levels"):
            getattr(t, name)
    assert tuple(env.scene.env_origins.shape) == (64, 3) and not bool(env.scene.env_origins.any())


def test_on_failure_raise_names_the_tile():
    from wheeledlab_amd import registry
    cfg = patch_env_cfg(on_failure="raise", max_tries=64)
    gen = cfg.scene.terrain.terrain_generator
    gen.sub_terrains = {"wave": G.HfWaveTerrainCfg(amplitude_range=(0.1, 0.15), num_waves=16)}      # 0.5 m waves 0.4 m high: level nowhere
    gen.num_rows, gen.num_cols, gen.size = 5, 5, (8.0, 8.0)
    with pytest.raises(ValueError, match=r"tile 0 \(row 0, column 0, 'wave'\) has no level ground"):
        registry.make("Isaac-MushrElevationRL-v0", cfg=cfg)

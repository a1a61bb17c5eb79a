"""The flat-patch finder's DEVICE header (wheeledlab_amd/csrc/wl_flat_patch_dev.h) compiled for the host through the stand-in
<hip/hip_runtime.h> (tests/host_sim/flat_patch_host.cpp: a wavefront of one lane) and held, slot by slot, to the integer restatement
(tests/flat_patch_reference.py) for EXACT equality of xy, z and tries -- on the all-types grid of the generator's tests, codes =
rint of its float64 reference heights.  From the reference alone it first asserts that the grid reaches every branch of the search.
With one lane a round is one attempt: the draw, the disc test, the window's centre and the
three floats are what this covers; the ballot, the pick of the lowest set bit and the lane masking run only on the device
(tests/test_gpu_flat_patches.py).  Test infrastructure only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import flat_patch_reference as FR
import terrain_gen_reference as TR
from wheeledlab_amd import _abi as A
from wheeledlab_amd.envs import terrain_gen_cfg as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
RADIUS, MAX_DIFF, P, PATCH_SEED = 0.15, 0.02, 8, 5


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host simulation")
    out = tmp_path_factory.mktemp("host_sim") / "libwl_flat_patch_host.so"
    # -ffp-contract=off: the header keeps its one product out of contraction itself; nothing else may be fused here or on the device
    subprocess.run([CLANG, "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), os.path.join(ROOT, "tests", "host_sim", "flat_patch_host.cpp"),
                    "-o", str(out)], check=True)
    return C.CDLL(str(out))


def grid_cfg(max_tries):
    return TR.all_types_cfg(flat_patch_sampling={"init_pos": G.FlatPatchSamplingCfg(num_patches=P, patch_radius=RADIUS, max_height_diff=MAX_DIFF,
                                                                                    max_tries=max_tries)})


@pytest.fixture(scope="module")
def grid():
    """the codes, and per max_tries the patch table and the reference's result (computed once)"""
    cfg = grid_cfg(1024)
    codes = TR.reference(TR.params_dict(cfg), G.tile_table(cfg)).codes
    out = {}
    for tries in (1024, 100):
        table, n_patches, _, _ = G.patch_table(grid_cfg(tries), "init_pos")
        assert n_patches == P and (table["max_tries"] == tries).all() and (table["radius_cells"] == 3).all() and (table["radius2"] == 9).all()
        out[tries] = (table,) + FR.find(codes, table, P, PATCH_SEED)
    return cfg, codes, out


def test_the_grid_reaches_every_branch(grid):
    cfg, codes, out = grid
    names = G.tile_names(cfg)
    _, _, tries = out[1024]
    print("[flat-patch] accepted attempt per slot (1024 tries):", {f"{t} {names[t]}": tries[t].tolist() for t in range(len(names))})
    assert any((tries[t] == 0).all() for t in range(len(names)))                          # all slots at the first attempt
    assert all((tries[t] < 0).all() for t in range(len(names)) if names[t] == "wave")      # all slots failed
    assert any((tries[t] < 0).any() and (tries[t] >= 0).any() for t in range(len(names)))  # both kinds in one tile
    assert (tries >= 64).any()                                                             # accepted in a later round of 64
    short = out[100][2]
    assert ((short < 0) & (tries >= 0)).any() and ((short >= 0) == ((tries >= 0) & (tries < 100))).all()
    assert np.array_equal(short[short >= 0], tries[short >= 0])


@pytest.mark.parametrize("max_tries", [1024, 100])
def test_host_sim_equals_the_reference(hostlib, grid, max_tries):
    cfg, codes, out = grid
    table, ij, tries = out[max_tries]
    geo = G.lattice(cfg)
    want_xy, want_z = FR.outputs(codes, ij, geo["x0"], geo["y0"], geo["cell"], geo["z_scale"])
    codes_c = np.ascontiguousarray(codes)
    hf = A.WlHeightField(codes_c.ctypes.data, geo["nx"], geo["ny"], geo["x0"], geo["y0"], geo["cell"], 0.0, geo["z_scale"], None)
    p = A.WlFlatPatchParams(len(table), P, A.TS_PATCH, 0, PATCH_SEED)
    xy = np.full((len(table), P, 2), np.nan, np.float32)
    z = np.full((len(table), P), np.nan, np.float32)
    got = np.full((len(table), P), -7, np.int32)
    assert hostlib.hs_flat_patches(C.byref(hf), C.byref(p), table.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p),
                                   z.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p)) == 0
    np.testing.assert_array_equal(got, tries)
    np.testing.assert_array_equal(xy, want_xy)
    np.testing.assert_array_equal(z, want_z)
    # every accepted patch is level by the rule, read off the codes directly
    di, dj = FR.disc(3, 9)
    for t, k in zip(*np.nonzero(tries >= 0)):
        c = codes[ij[t, k, 1] + dj, ij[t, k, 0] + di].astype(int)
        assert c.max() - c.min() <= int(MAX_DIFF / geo["z_scale"] + 1e-9)


def test_host_deal_equals_the_reference(hostlib):
    for n, off, world, cols, n_patches, epoch, seed in ((70, 0, 70, 2, 8, 0, 9), (35, 35, 70, 3, 5, 2 ** 33 + 7, 2 ** 40 + 1), (64, 0, 64, 1, 1, 3, 0)):
        got = np.full(n, -1, np.int32)
        assert hostlib.hs_flat_patch_deal(n, off, world, cols, n_patches, C.c_uint64(epoch), C.c_uint64(seed), got.ctypes.data_as(C.c_void_p)) == 0
        np.testing.assert_array_equal(got, FR.deal(off + np.arange(n), cols, world, n_patches, epoch, seed))
        assert got.min() >= 0 and got.max() < cols * n_patches

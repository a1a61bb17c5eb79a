"""CPU checks of mesh terrains: the terrain header's layout and symbols, argument refusals before any launch, the OBJ reader on
every face form, the float64 reference (tests/mesh_reference.py) on closed forms, its predicate rejecting modelled defects, and the
task configs carrying `mesh_path`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_reference as MR
from conftest import ROOT
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_terrain.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def test_terrain_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in A.WlMeshRasterParams._fields_]
    probe = tmp_path / "probe.c"
    body = " ".join(f'printf("%zu ", offsetof(WlMeshRasterParams, {n}));' for n in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_terrain.h"\n'
                     f'int main(){{{body} printf("%zu %d %d %d %d %d\\n", sizeof(WlMeshRasterParams), (int)WL_TERRAIN_VERSION,'
                     ' (int)WL_TERRAIN_TILE, (int)WL_TERRAIN_MAX_TILES_PER_FACE, (int)WL_TERRAIN_MAX_SIDE, (int)WL_TERRAIN_STATUS_WORDS);'
                     ' return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(A.WlMeshRasterParams, n).offset for n in fields] + [
        C.sizeof(A.WlMeshRasterParams), A.WL_TERRAIN_VERSION, A.TERRAIN_TILE, A.TERRAIN_MAX_TILES_PER_FACE, A.TERRAIN_MAX_SIDE,
        A.TERRAIN_STATUS_WORDS]
    assert got == want


def test_terrain_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.TERRAIN_SIGNATURES)
    assert not declared & (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES))      # outside the drop-in step boundary
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_terrain_version() == A.WL_TERRAIN_VERSION


def test_mesh_raster_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    S = lib.wl_mesh_raster_scratch_bytes
    assert S(-1, 8, 8) == -1 and S(4, 1, 8) == -1 and S(4, 8, 1) == -1
    assert S(4, A.TERRAIN_MAX_SIDE, 8) == -1 and S(4, 8, A.TERRAIN_MAX_SIDE) == -1
    assert S(4, 65536, 65536) == -1                                   # nx * ny > 2^31 - 1
    assert S(4, A.TERRAIN_MAX_SIDE - 1, 2) > 0 and S(0, 2, 2) > 0
    need = S(4, 8, 8)
    fake = 1 << 20                 # never dereferenced: every call below is refused before any launch
    good = dict(p=A.WlMeshRasterParams(0.0, 0.0, 0.1, 8, 8, 0.0), v=fake, nv=4, f=fake, nf=4, s=fake, nb=need, h=fake, st=fake)

    def call(**kw):
        a = {**good, **kw}
        return lib.wl_mesh_raster(C.byref(a["p"]) if a["p"] is not None else None, a["v"], a["nv"], a["f"], a["nf"], a["s"], a["nb"],
                                  a["h"], a["st"], None)
    P = A.WlMeshRasterParams
    inf, nan = float("inf"), float("nan")
    assert call(p=None) == -1
    assert call(v=None) == -1 and call(f=None) == -1 and call(s=None) == -1 and call(h=None) == -1 and call(st=None) == -1
    for cell in (0.0, -0.1, inf, nan):
        assert call(p=P(0.0, 0.0, cell, 8, 8, 0.0)) == -1
    for nx, ny in ((1, 8), (8, 1), (0, 8), (A.TERRAIN_MAX_SIDE, 8), (8, A.TERRAIN_MAX_SIDE), (65536, 65536)):
        assert call(p=P(0.0, 0.0, 0.1, nx, ny, 0.0)) == -1
    assert call(nf=-1) == -1 and call(nv=-1) == -1
    assert call(nb=need - 1) == -1                                   # scratch too small
    for fz in (inf, -inf, nan):
        assert call(p=P(0.0, 0.0, 0.1, 8, 8, fz)) == -1
    for x0 in (inf, nan):
        assert call(p=P(x0, 0.0, 0.1, 8, 8, 0.0)) == -1 and call(p=P(0.0, x0, 0.1, 8, 8, 0.0)) == -1
    # misalignment
    assert call(s=fake + 8) == -3 and call(v=fake + 2) == -3 and call(f=fake + 1) == -3
    assert call(h=fake + 2) == -3 and call(st=fake + 2) == -3


def test_load_obj_every_face_form(tmp_path):
    from wheeledlab_amd.terrain import load_obj
    p = tmp_path / "m.obj"
    p.write_text("# a comment\n"
                 "mtllib x.mtl\no thing\ng group\n"
                 "v 0 0 0\nv 1 0 0.5\nv 1 1 1   # trailing comment\nv 0 1 2\n"
                 "vt 0 0\nvt 1 0\nvn 0 0 1\n"
                 "usemtl m\ns off\n"
                 "f 1 2 3\n"
                 "f 1/1 3/2 4/1\n"
                 "f 1/1/1 2/2/1 4/1/1\n"
                 "f 2//1 3//1 4//1\n"
                 "v 2 0 3\nv 2 1 4\n"
                 "f -5 -2 -1 -4\n"                # a quad with relative indices: 2 5 6 3
                 "f 1 2 5 6 4\n"                   # a pentagon
                 "l 1 2\nvp 0.5\n")
    v, f = load_obj(str(p))
    assert v.dtype == np.float32 and f.dtype == np.int32
    np.testing.assert_array_equal(v, np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 1], [0, 1, 2], [2, 0, 3], [2, 1, 4]], np.float32))
    np.testing.assert_array_equal(f, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3],
                                               [1, 4, 5], [1, 5, 2],
                                               [0, 1, 4], [0, 4, 5], [0, 5, 3]], np.int32))


def test_load_obj_empty_and_malformed(tmp_path):
    from wheeledlab_amd.terrain import load_obj
    p = tmp_path / "e.obj"
    p.write_text("# nothing\n")
    v, f = load_obj(str(p))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    with pytest.raises(ValueError):
        load_obj(str(p))
    p.write_text("v 0 0\n")
    with pytest.raises(ValueError):
        load_obj(str(p))


# ---- the float64 reference on closed forms ----

def _grid(nx=21, ny=17, cell=0.25, x0=-2.5, y0=-2.0):
    return x0, y0, cell, nx, ny


def test_reference_tilted_plane_is_the_plane():
    x0, y0, cell, nx, ny = _grid()
    a, b, c = 0.3, -0.2, 1.5
    corners = np.array([[-3.1, -2.6], [3.3, -2.6], [3.3, 2.7], [-3.1, 2.7]])
    v = np.c_[corners, a * corners[:, 0] + b * corners[:, 1] + c].astype(np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    h = MR.rasterize(v, f, x0, y0, cell, nx, ny)
    xs, ys = MR.lattice_axes(x0, y0, cell, nx, ny)
    want = a * xs[None, :] + b * ys[:, None] + c
    np.testing.assert_allclose(h, want, atol=2e-6)
    assert MR.acceptable(h, v, f, x0, y0, cell, nx, ny).all()


def test_reference_square_pyramid_apex_and_edges():
    # apex at the origin 2 m up over a 4 x 4 m base: h = 2 (1 - max(|x|, |y|) / 2) inside, fill outside
    v = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0], [0, 0, 2]], np.float32)
    f = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32)
    x0, y0, cell, nx, ny = -3.0, -3.0, 0.25, 25, 25
    h = MR.rasterize(v, f, x0, y0, cell, nx, ny, fill_z=-1.0)
    xs, ys = MR.lattice_axes(x0, y0, cell, nx, ny)
    m = np.maximum(np.abs(xs[None, :]), np.abs(ys[:, None]))
    want = np.where(m <= 2, 2 * (1 - m / 2), -1.0)
    np.testing.assert_allclose(h, want, atol=1e-12)
    assert h[12, 12] == 2.0                       # the apex, a lattice point
    assert MR.acceptable(h, v, f, x0, y0, cell, nx, ny, fill_z=-1.0).all()


def test_reference_bridge_gives_the_top_layer():
    v, f = MR.bridge()
    x0, y0, cell, nx, ny = -4.0, -4.0, 0.5, 17, 17
    h = MR.rasterize(v, f, x0, y0, cell, nx, ny, fill_z=-5.0)
    xs, ys = MR.lattice_axes(x0, y0, cell, nx, ny)
    X, Y = np.meshgrid(xs, ys)
    want = np.where((np.abs(X) <= 1.1) & (np.abs(Y) <= 3.3), 1.0, np.where((np.abs(X) <= 3) & (np.abs(Y) <= 3), 0.0, -5.0))
    np.testing.assert_array_equal(h, want)


def test_reference_box_walls_give_the_top_on_its_boundary():
    v, f = MR.box_on_plane()
    x0, y0, cell, nx, ny = -2.0, -2.0, 0.25, 17, 17
    h = MR.rasterize(v, f, x0, y0, cell, nx, ny)
    xs, ys = MR.lattice_axes(x0, y0, cell, nx, ny)
    X, Y = np.meshgrid(xs, ys)
    inside = (np.abs(X) <= 1) & (np.abs(Y) <= 1)
    np.testing.assert_array_equal(h, np.where(inside, 0.5, 0.0))
    assert (h[np.isclose(np.abs(X), 1) & (np.abs(Y) <= 1)] == 0.5).all()      # the cliff edge on a lattice line: the top
    ok = MR.acceptable(h, v, f, x0, y0, cell, nx, ny)
    assert ok.all()


# ---- the predicate rejects modelled defects ----

def _wavy(nx=24, ny=20, cell=0.1):
    rng = np.random.default_rng(3)
    xs = np.arange(nx) * cell
    ys = np.arange(ny) * cell
    hgt = np.sin(xs[None, :] * 2.0) * np.cos(ys[:, None] * 1.5) + 0.05 * rng.standard_normal((ny, nx))
    return MR.triangulate_grid(hgt, 0.0, 0.0, cell)


def test_predicate_rejects_a_dropped_triangle():
    v, f = _wavy()
    lat = (0.0, 0.0, 0.05, 45, 37)
    good = MR.rasterize(v, f, *lat, fill_z=-3.0)
    assert MR.acceptable(good, v, f, *lat, fill_z=-3.0).all()
    bad = MR.rasterize(v, np.delete(f, 101, 0), *lat, fill_z=-3.0)
    assert not MR.acceptable(bad, v, f, *lat, fill_z=-3.0).all()


def test_predicate_rejects_min_instead_of_max():
    v, f = MR.bridge()
    lat = (-4.0, -4.0, 0.5, 17, 17)
    assert not MR.acceptable(MR.rasterize(v, f, *lat, reduce="min"), v, f, *lat).all()


def test_predicate_rejects_holes_on_shared_edges():
    v, f = _wavy()
    lat = (0.0, 0.0, 0.05, 45, 37)           # every other lattice point on a grid vertex, others on shared edges
    bad = MR.rasterize(v, f, *lat, fill_z=-3.0, closed=False)
    ok = MR.acceptable(bad, v, f, *lat, fill_z=-3.0)
    assert not ok.all()
    assert not ok[1:-1, 1:-1].all()          # in the interior, not only on the mesh boundary


def test_predicate_rejects_half_a_cell_offset():
    v, f = _wavy()
    x0, y0, cell, nx, ny = 0.0, 0.0, 0.05, 45, 37
    bad = MR.rasterize(v, f, x0 + cell / 2, y0, cell, nx, ny)
    assert not MR.acceptable(bad, v, f, x0, y0, cell, nx, ny).all()


def test_predicate_rejects_x_and_y_swapped():
    v, f = _wavy()
    lat = (0.0, 0.0, 0.05, 40, 40)
    bad = MR.rasterize(v, f, *lat).T
    assert not MR.acceptable(bad, v, f, *lat).all()


def test_predicate_rejects_fill_ignored():
    v, f = _wavy()
    lat = (-0.5, -0.5, 0.05, 60, 60)         # the lattice reaches beyond the mesh
    bad = MR.rasterize(v, f, *lat, fill_z=0.0)
    assert not MR.acceptable(bad, v, f, *lat, fill_z=-3.0).all()
    assert MR.acceptable(MR.rasterize(v, f, *lat, fill_z=-3.0), v, f, *lat, fill_z=-3.0).all()


def test_triangulated_field_rasterises_to_itself():
    x0, y0, cell = -1.0, -1.0, 0.0625
    rng = np.random.default_rng(0)
    hgt = (np.rint(rng.standard_normal((9, 11)) * 4096) / 8192).astype(np.float32)
    for alternate in (True, False):
        v, f = MR.triangulate_grid(hgt, x0, y0, cell, alternate=alternate)
        np.testing.assert_array_equal(MR.rasterize(v, f, x0, y0, cell, 11, 9), hgt)


# ---- configs ----

def test_mesh_path_reaches_the_batch_arguments(tmp_path):
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.tasks.elevation.mushr_elevation_env_cfg import MushrElevationRLEnvCfg
    from wheeledlab_amd.tasks.visual_depth.mushr_visual_depth_env_cfg import MushrVisualDepthRLEnvCfg
    for cls in (MushrElevationRLEnvCfg, MushrVisualDepthRLEnvCfg):
        cfg = cls()
        assert cfg.scene.terrain.mesh_path is None and cfg.scene.terrain.mesh_cell == 0.05
        x = flatten_cfg(cfg).extra
        assert x["heightfield"] is None and x["mesh_path"] is None          # neither: the synthetic field, as before
        cfg.scene.terrain.mesh_path = str(tmp_path / "t.obj")
        cfg.scene.terrain.mesh_cell = 0.1
        x = flatten_cfg(cfg).extra
        assert x["mesh_path"] == str(tmp_path / "t.obj") and x["mesh_cell"] == 0.1 and x["heightfield"] is None
        cfg.scene.terrain.heightfield = (np.zeros((4, 4), np.float32), 0.0, 0.0, 0.1)
        with pytest.raises(ValueError, match="not both"):
            flatten_cfg(cfg)
        cfg.scene.terrain.heightfield = None
        cfg.scene.terrain.mesh_cell = 0.0
        with pytest.raises(ValueError):
            flatten_cfg(cfg)

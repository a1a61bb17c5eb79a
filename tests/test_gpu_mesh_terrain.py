"""GPU: mesh terrains (include/wheeledlab_amd_terrain.h, csrc/wl_terrain.hip via core.mesh_heightfield) -- the exact round trip of a
triangulated field through the codes, the pair table, both heightfield tasks and the env surface; the bench field at 0.05 m; an
unaligned rotated mesh and the geometric edge cases against the float64 predicate (tests/mesh_reference.py::acceptable); every
binning branch (the scan's carry past one pass, K and K + 1 tiles, the entry budget's overflow into the big list, more records than
one LDS chunk, two lattice-wide faces beside 200 000 small ones); invalid faces; run-to-run byte identity."""
import numpy as np
import pytest
import torch

import mesh_reference as MR
from wheeledlab_amd import _abi as A
from wheeledlab_amd.core import DeviceHeightField, ElevBatch, VisualDepthBatch, mesh_heightfield
from wheeledlab_amd.terrain import synthetic_heightfield

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = A.TERRAIN_MAX_TILES_PER_FACE


def _check(v, f, cell, lattice, fill_z=0.0, label="", stats=None):
    h, x0, y0, c = mesh_heightfield(v, f, cell, DEV, lattice=lattice, fill_z=fill_z, stats=stats)
    ny, nx = h.shape
    ok = MR.acceptable(h.cpu().numpy(), v, f, x0, y0, c, nx, ny, fill_z, label=label)
    assert ok.all(), (label, int((~ok).sum()), np.argwhere(~ok)[:5])
    return h


@pytest.fixture(scope="module")
def field_mesh():
    hgt, x0, y0, cell = synthetic_heightfield(800, cell=0.0625)
    v, f = MR.triangulate_grid(hgt, x0, y0, cell)
    return (hgt, x0, y0, cell), v, f


def test_round_trip_is_exact(field_mesh):
    field, v, f = field_mesh
    h, x0, y0, cell = mesh_heightfield(v, f, field[3], DEV)
    assert (x0, y0, cell) == (field[1], field[2], field[3]) and tuple(h.shape) == (800, 800)
    assert np.array_equal(h.cpu().numpy().view(np.uint32), field[0].view(np.uint32))
    a, b = DeviceHeightField((h, x0, y0, cell), DEV), DeviceHeightField(field, DEV)
    assert a.z_scale == b.z_scale and torch.equal(a.codes, b.codes) and torch.equal(a.pairs, b.pairs)


def _same_rollout(make, mesh_hf, field, n=64, steps=50):
    envs = [make(mesh_hf), make(field)]
    for e in envs:
        e.reset()
    g = torch.Generator(device=DEV).manual_seed(11)
    for _ in range(steps):
        a = torch.rand(n, 2, device=DEV, generator=g) * 2 - 1
        outs = [[t.clone() for t in e.step(a)] for e in envs]
        for x, y in zip(*outs):
            assert torch.equal(x, y)


def test_round_trip_steps_elevation_and_depth_bit_identically(field_mesh):
    field, v, f = field_mesh
    mesh_hf = mesh_heightfield(v, f, field[3], DEV)
    _same_rollout(lambda hf: ElevBatch(64, device=DEV, seed=5, heightfield=hf), mesh_hf, field)
    _same_rollout(lambda hf: VisualDepthBatch(64, device=DEV, seed=5, heightfield=hf), mesh_hf, field)


def test_round_trip_through_the_env_surface(field_mesh, tmp_path):
    from wheeledlab_amd import registry, tasks  # noqa: F401
    field, v, f = field_mesh
    obj = tmp_path / "field.obj"
    with open(obj, "w") as fh:
        fh.write("# triangulated synthetic field\n")
        np.savetxt(fh, v, fmt="v %.9g %.9g %.9g")
        np.savetxt(fh, f + 1, fmt="f %d %d %d")
    for task in ("Isaac-MushrElevationRL-v0", "Isaac-MushrVisualDepthRL-v0"):
        envs = []
        for src in ("mesh", "field"):
            cfg = registry.parse_env_cfg(task, device=DEV, num_envs=32)
            if src == "mesh":
                cfg.scene.terrain.mesh_path, cfg.scene.terrain.mesh_cell = str(obj), field[3]
            else:
                cfg.scene.terrain.heightfield = field
            envs.append(registry.make(task, cfg=cfg))
        for e in envs:
            e.reset()
        g = torch.Generator(device=DEV).manual_seed(2)
        for _ in range(20):
            a = torch.rand(32, 2, device=DEV, generator=g) * 2 - 1
            r = [e.step(a) for e in envs]
            assert torch.equal(r[0][0]["policy"], r[1][0]["policy"])
            for x, y in zip(r[0][1:4], r[1][1:4]):
                assert torch.equal(x, y)


def test_bench_field_at_5cm_within_one_code():
    hgt, x0, y0, cell = synthetic_heightfield()
    c32 = np.float64(np.float32(cell))
    xs = np.float64(np.float32(x0)) + np.arange(800) * c32
    ys = np.float64(np.float32(y0)) + np.arange(800) * c32
    v, f = MR.triangulate_grid(hgt, x0, y0, cell, xs=xs, ys=ys)
    h, *_ = mesh_heightfield(v, f, cell, DEV, lattice=(x0, y0, 800, 800))
    got, want = DeviceHeightField((h, x0, y0, cell), DEV), DeviceHeightField((hgt, x0, y0, cell), DEV)
    d = (got.codes.int() - want.codes.int()).abs()
    print(f"[mesh] bench field at 0.05 m: {int((d > 0).sum())} of {d.numel()} codes differ, max |diff| {int(d.max())}")
    assert int(d.max()) <= 1


def unaligned_mesh(seed=0):
    rng = np.random.default_rng(seed)
    nx, ny, s = 300, 200, 0.137
    gx, gy = np.meshgrid(np.arange(nx) * s, np.arange(ny) * s)
    gx, gy = gx + rng.uniform(-0.04, 0.04, gx.shape), gy + rng.uniform(-0.04, 0.04, gy.shape)
    z = 0.5 * np.sin(gx * 0.7) * np.cos(gy * 0.9) + 0.02 * rng.standard_normal(gx.shape)
    th = np.deg2rad(17.0)
    X, Y = np.cos(th) * gx - np.sin(th) * gy - 15.0, np.sin(th) * gx + np.cos(th) * gy - 12.0
    v, f = MR.triangulate_grid(z, 0, 0, 1)
    v[:, 0], v[:, 1] = X.ravel(), Y.ravel()
    return v, f


def test_unaligned_rotated_mesh_and_determinism():
    v, f = unaligned_mesh()
    h1 = _check(v, f, 0.1, None, label="unaligned 17 deg")
    h2, *_ = mesh_heightfield(v, f, 0.1, DEV)
    assert torch.equal(h1.view(torch.int32), h2.view(torch.int32))


def test_geometry_edge_cases():
    v, f = MR.bridge()
    _check(v, f, 0.1, (-4.0, -4.0, 81, 81), fill_z=-2.0, label="bridge")
    # an overhang: the deck's far end hangs over open ground
    v2 = v.copy()
    v2[4:, 0] += 2.5
    _check(v2, f, 0.1, (-4.0, -4.0, 101, 81), fill_z=-2.0, label="overhang")
    v, f = MR.box_on_plane()
    _check(v, f, 0.25, (-2.0, -2.0, 17, 17), label="box 0.25")
    _check(v, f, 0.05, (-2.5, -2.5, 101, 101), label="box 0.05")
    # both windings mixed, with zero-area, needle and duplicate faces
    v, f = unaligned_mesh(1)
    f = f.copy()
    f[::3] = f[::3, ::-1]
    rng = np.random.default_rng(4)
    pick = rng.integers(0, f.shape[0], 500)
    zero = np.stack([f[pick, 0], f[pick, 0], f[pick, 1]], 1)                       # repeated vertex
    needle_v = np.concatenate([v[f[pick, 0]], v[f[pick, 0]] + np.float32([1e-4, 3.0, 0.1])])
    needle_v[500:, 0] += np.float32(1e-6)
    needle_f = np.stack([np.arange(500), np.arange(500, 1000), f[pick, 1] * 0], 1) + v.shape[0]
    needle_f[:, 2] = f[pick, 2]
    vv = np.concatenate([v, needle_v]).astype(np.float32)
    ff = np.concatenate([f, zero, f[pick], f[pick, ::-1], needle_f]).astype(np.int32)
    _check(vv, ff, 0.1, None, label="windings, zero-area, needles, duplicates")
    # partly or entirely outside an explicit lattice
    _check(v, f, 0.07, (-5.0, -3.0, 97, 83), label="clipped")
    _check(v, f, 0.07, (100.0, 100.0, 20, 20), fill_z=3.5, label="all outside")
    # 2 x 2 and a non-square lattice that is no multiple of the tile
    _check(v, f, 0.5, (0.1, 0.2, 2, 2), label="2 x 2")
    _check(v, f, 0.09, (-10.0, -8.0, 37, 53), label="37 x 53")
    # the empty mesh
    h, *_ = mesh_heightfield(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.1, DEV, lattice=(0.0, 0.0, 19, 21), fill_z=-0.75)
    assert tuple(h.shape) == (21, 19) and bool((h == -0.75).all())


def test_big_list_threshold_k_and_k_plus_one():
    # lattice-index rectangle [floor(min), ceil(max)] with cell 1 and origin 0: 8 x 8 tiles = K, then 13 x 5 tiles = K + 1
    lat = (0.0, 0.0, 300, 300)
    for verts, big in (([[0.25, 0.25, 1.0], [126.5, 0.25, 2.0], [0.25, 126.5, 3.0]], 0),
                       ([[0.25, 0.25, 1.0], [206.5, 0.25, 2.0], [0.25, 78.5, 3.0]], 1)):
        st = {}
        _check(np.float32(verts), np.int32([[0, 1, 2]]), 1.0, lat, fill_z=-1.0, label=f"{'K + 1' if big else 'K'} tiles", stats=st)
        assert st["binned"] == 1 and st["big"] == big and st["entries"] == (0 if big else K)


def test_a_tile_with_more_records_than_one_chunk():
    rng = np.random.default_rng(7)
    n = 700                                             # every face inside tile (0, 0): 700 records, three LDS chunks
    c = rng.uniform(2.0, 13.0, (n, 1, 2))
    v = np.concatenate([c + rng.uniform(-1.9, 1.9, (n, 3, 2)), rng.uniform(0, 2, (n, 3, 1))], 2).reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    st = {}
    _check(v, f, 1.0, (0.0, 0.0, 32, 32), fill_z=-1.0, label="crowded tiles", stats=st)
    assert st["binned"] == n and st["big"] == 0 and st["entries"] == n


def test_entry_budget_overflow_matches_two_halves():
    # 40 000 faces of 8 x 8 tiles: 2.56 M entries > the budget of max(8 F, 2^21) -> the rest goes to the big list.  A maximum does
    # not care which list a face came from: the launch equals the maximum of its two halves (each within budget), bit for bit.
    rng = np.random.default_rng(9)
    n = 40000
    o = rng.integers(0, 119, (n, 1, 2)) * 16.0           # rectangles start on a tile: exactly 8 x 8 tiles each
    shape = np.array([[0.25, 0.25], [126.5, 0.25], [0.25, 126.5]])
    xy = o + np.where(rng.random((n, 1, 1)) < 0.5, shape, shape[:, ::-1])
    v = np.concatenate([xy, rng.uniform(0, 5, (n, 3, 1))], 2).reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    lat = (0.0, 0.0, 2048, 2048)
    st, s1, s2 = {}, {}, {}
    h, *_ = mesh_heightfield(v, f, 1.0, DEV, lattice=lat, fill_z=-1.0, stats=st)
    a, *_ = mesh_heightfield(v, f[: n // 2], 1.0, DEV, lattice=lat, fill_z=-1.0, stats=s1)
    b, *_ = mesh_heightfield(v, f[n // 2:], 1.0, DEV, lattice=lat, fill_z=-1.0, stats=s2)
    print("[mesh] budget overflow:", st, "halves:", s1["big"], s2["big"])
    assert st["binned"] == n and st["big"] > 0 and st["entries"] <= 1 << 21 and s1["big"] == s2["big"] == 0
    assert torch.equal(h, torch.maximum(a, b))


def mixed_mesh(seed=5):
    """two faces covering a 4096 x 4096 lattice of 0.01 m beside 200 000 small ones"""
    rng = np.random.default_rng(seed)
    L = 40.96
    big_v = np.float32([[-0.5, -0.5, 0.05], [L + 0.5, -0.5, 0.15], [L + 0.5, L + 0.5, 0.1], [-0.5, L + 0.5, 0.0]])
    n = 200000
    c = rng.uniform(0.05, L - 0.06, (n, 1, 2))               # every small face on the lattice
    small = np.concatenate([c + rng.uniform(-0.04, 0.04, (n, 3, 2)), rng.uniform(0.0, 0.4, (n, 3, 1))], 2).reshape(-1, 3)
    v = np.concatenate([big_v, small]).astype(np.float32)
    f = np.concatenate([[[0, 1, 2], [0, 2, 3]], 4 + np.arange(3 * n).reshape(n, 3)]).astype(np.int32)
    return v, f, (0.0, 0.0, 4096, 4096)


def test_mixed_mesh_on_4096_and_determinism():
    v, f, lat = mixed_mesh()
    st = {}
    h1 = _check(v, f, 0.01, lat, label="mixed 4096^2", stats=st)
    assert st["big"] == 2 and st["binned"] == f.shape[0]
    h2, *_ = mesh_heightfield(v, f, 0.01, DEV, lattice=lat)
    assert torch.equal(h1.view(torch.int32), h2.view(torch.int32))


def test_invalid_faces_raise():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1]])
    lat = (0.0, 0.0, 8, 8)
    for bad_f in ([[0, 1, 4]], [[0, -1, 2]], [[0, 1, 2], [1, 3, 2 ** 31 - 1]]):
        with pytest.raises(ValueError, match="faces"):
            mesh_heightfield(v, np.int32(bad_f), 0.2, DEV, lattice=lat)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[3, 2] = bad
        with pytest.raises(ValueError, match="faces"):
            mesh_heightfield(w, np.int32([[0, 1, 2], [1, 3, 2]]), 0.2, DEV, lattice=lat)
    torch.cuda.synchronize()
    h, *_ = mesh_heightfield(v, np.int32([[0, 1, 2], [1, 3, 2]]), 0.2, DEV, lattice=lat)       # the device is still fine
    assert bool(torch.isfinite(h).all())

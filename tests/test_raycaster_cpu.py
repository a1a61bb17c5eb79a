"""CPU checks of the ray caster: the patterns' counts, order and directions, the configs' defaults, which scene attributes become
views, the header's layout and symbols, every argument refusal of wl_raycast_scan before any launch, and the device's per-ray
functions (wl_raycast_dev.h) compiled for the host and held to the float64 reference (tests/raycaster_reference.py: oracle/depth.c
one ray per table entry; a float64 bilinear for the column form).  Yardstick for walked rays: lidar_reference.check."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import heightfield_cases as HC
from tests import lidar_reference as LR
from tests import raycaster_reference as RR
from tests.raycaster_host import host_scan, hostlib  # noqa: F401  (the fixture)
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_raycaster.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


class _B:
    n, device = 4, "cpu"


# ---- 1. patterns and configs -----------------------------------------------------------------------------------------

def test_grid_counts_and_orderings():
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg
    assert GridPatternCfg(size=(2.5, 2.5), resolution=0.1).counts() == (26, 26) and 26 * 26 == 676 == A.ELEV_SCAN_N ** 2
    g = GridPatternCfg(size=(1.0, 0.6), resolution=0.1)
    assert g.counts() == (11, 7) and g.ordering == "xy" and g.direction == (0.0, 0.0, -1.0)
    s, d = g.rays()
    assert s.shape == d.shape == (77, 3) and (d == [0.0, 0.0, -1.0]).all() and (s[:, 2] == 0).all()
    x, y = -0.5 + 0.1 * np.arange(11), -0.3 + 0.1 * np.arange(7)
    np.testing.assert_allclose(s[:, 0].reshape(7, 11), np.repeat(x[None], 7, 0), atol=1e-15)       # "xy": x fastest
    np.testing.assert_allclose(s[:, 1].reshape(7, 11), np.repeat(y[:, None], 11, 1), atol=1e-15)
    np.testing.assert_allclose(s.mean(0), 0.0, atol=1e-15)                                           # centred on 0
    t, _ = GridPatternCfg(size=(1.0, 0.6), resolution=0.1, ordering="yx").rays()
    np.testing.assert_array_equal(t.reshape(11, 7, 3).transpose(1, 0, 2).reshape(77, 3), s)          # "yx": y fastest, same points
    assert not np.array_equal(t, s)
    with pytest.raises(ValueError):
        GridPatternCfg(size=(1.0, 1.0), resolution=0.1, ordering="zz").rays()
    with pytest.raises(ValueError):
        GridPatternCfg(size=(1.0, 1.0), resolution=0.0).rays()


def test_a_slanted_grid_direction_is_normalised_and_the_start_plane_kept():
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg
    s, d = GridPatternCfg(size=(1.0, 0.6), resolution=0.1, direction=(0.6, 0.0, -1.6)).rays()
    np.testing.assert_allclose(d, np.repeat([[0.6 / np.hypot(0.6, 1.6), 0.0, -1.6 / np.hypot(0.6, 1.6)]], 77, 0), atol=1e-15)
    assert (s[:, 2] == 0).all()
    _, d = GridPatternCfg(size=(0.2, 0.2), resolution=0.1, direction=(0.0, 0.0, -3.0)).rays()
    assert (d == [0.0, 0.0, -1.0]).all()                 # exactly vertical: what selects the column form
    with pytest.raises(ValueError):
        GridPatternCfg(size=(1.0, 1.0), resolution=0.1, direction=(0.0, 0.0, 0.0)).rays()


def _visual_pattern(width=80, height=60):
    """a pinhole pattern with the visual camera's intrinsics (fx = width focal / aperture: an aperture of `width` makes focal = fx)"""
    from wheeledlab_amd.envs.sensors_cfg import PinholeCameraPatternCfg
    from wheeledlab_amd.params import visual_params
    p = visual_params()
    sx, sy = width / 80, height / 60
    return p, PinholeCameraPatternCfg(width=width, height=height, focal_length=p.fx * sx, horizontal_aperture=float(width),
                                      vertical_aperture=height * p.fx * sx / (p.fy * sy),
                                      horizontal_aperture_offset=(p.cx * sx - width / 2) / (p.fx * sx),
                                      vertical_aperture_offset=(p.cy * sy - height / 2) / (p.fy * sy))


def test_pinhole_pattern_is_the_visual_cameras_rays():
    from wheeledlab_amd.envs.sensors_cfg import PinholeCameraPatternCfg
    p, pat = _visual_pattern()
    np.testing.assert_allclose(pat.intrinsics(), (p.fx, p.fy, p.cx, p.cy), rtol=1e-12)
    s, d = pat.rays()
    assert s.shape == d.shape == (4800, 3) and (s == 0).all()
    np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    rows, cols = np.divmod(np.arange(4800), 80)                                                     # row-major
    body = np.stack([np.ones(4800), -((cols + 0.5 - p.cx) / p.fx), -((rows + 0.5 - p.cy) / p.fy)], 1)   # depth_pixel_ray_body
    np.testing.assert_allclose(d / d[:, :1], body, atol=1e-14)
    # defaults: square pixels, principal point in the middle
    fx, fy, cx, cy = PinholeCameraPatternCfg(width=40, height=30, focal_length=24.0, horizontal_aperture=20.955).intrinsics()
    assert fx == pytest.approx(40 * 24.0 / 20.955) and fy == pytest.approx(fx) and (cx, cy) == (20.0, 15.0)


def _rot(q):
    return LR._mat64(np.asarray(q, np.float64))


def test_camera_conventions():
    """the mount in the world convention (x forward, y left, z up) is offset_rot times the convention's quaternion: its rotation holds
    the world-convention axes in the convention's coordinates"""
    from wheeledlab_amd.envs.sensors_cfg import CAMERA_CONVENTION_TO_WORLD as T
    np.testing.assert_allclose(_rot(T["world"]), np.eye(3), atol=1e-15)
    # ros: z forward, x right, y down -> forward = +z, left = -x, up = -y
    np.testing.assert_allclose(_rot(T["ros"]), np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]]).T, atol=1e-15)
    # opengl: -z forward, x right, y up -> forward = -z, left = -x, up = +y
    np.testing.assert_allclose(_rot(T["opengl"]), np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]]).T, atol=1e-15)


def test_ray_caster_cfg_defaults_and_alignment():
    from wheeledlab_amd.envs.sensors_cfg import (GridPatternCfg, LidarPatternCfg, RayCasterCameraCfg, RayCasterCfg, pattern_rays)
    c = RayCasterCfg()
    assert c.offset_pos == (0.0, 0.0, 0.0) and c.offset_rot == (1.0, 0.0, 0.0, 0.0) and c.attach_yaw_only is True
    assert c.max_distance == 1e6 and c.ray_alignment is None and isinstance(c.pattern_cfg, GridPatternCfg)
    assert c.alignment() == "yaw" and RayCasterCfg(attach_yaw_only=False).alignment() == "base"
    assert RayCasterCfg(attach_yaw_only=False, ray_alignment="world").alignment() == "world"
    assert RayCasterCfg(ray_alignment="base").alignment() == "base"
    with pytest.raises(ValueError):
        RayCasterCfg(ray_alignment="pitch").alignment()
    s, d = pattern_rays(LidarPatternCfg())
    assert (s == 0).all() and d.shape == (360, 3)
    with pytest.raises(TypeError):
        pattern_rays(object())
    cam = RayCasterCameraCfg()
    assert cam.data_types == ["distance_to_image_plane"] and cam.offset_convention == "ros" and cam.depth_clipping_behavior == "max"
    assert cam.max_distance == 1e6 and (cam.pattern_cfg.width, cam.pattern_cfg.height) == (80, 60)


# ---- 2. scene --------------------------------------------------------------------------------------------------------

def test_scene_registers_ray_casters_on_every_task_and_keeps_the_fused_scanner():
    from wheeledlab_amd import registry, tasks  # noqa: F401
    from wheeledlab_amd.envs.scene import RayCasterCameraView, RayCasterView, RayCasterSensorView, SceneView
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg, RayCasterCameraCfg, RayCasterCfg
    front = RayCasterCfg(offset_pos=(0.6, 0.0, 0.3), pattern_cfg=GridPatternCfg(size=(1.0, 0.6), resolution=0.1))
    cfg = registry.parse_env_cfg("Isaac-MushrElevationRL-v0", device="cpu", num_envs=4)
    cfg.scene.front_scan = front
    cfg.scene.depth_cam = RayCasterCameraCfg()
    scene = SceneView(_B(), cfg.scene, task="elevation")
    assert type(scene["front_scan"]) is RayCasterSensorView and scene["front_scan"].cfg is front
    assert type(scene.sensors["height_scanner"]) is RayCasterView                 # the fused scan, as before
    assert type(scene["depth_cam"]) is RayCasterCameraView and scene["depth_cam"].data.image_shape == (60, 80)
    assert {"front_scan", "depth_cam", "height_scanner"} <= set(scene.keys())
    plain = SceneView(_B(), registry.parse_env_cfg("Isaac-MushrElevationRL-v0", device="cpu", num_envs=4).scene, task="elevation")
    assert "front_scan" not in plain.sensors
    drift = registry.parse_env_cfg("Isaac-MushrDriftRL-v0", device="cpu", num_envs=4)
    drift.scene.front_scan = front
    scene = SceneView(_B(), drift.scene, task="drift")
    assert type(scene["front_scan"]) is RayCasterSensorView and scene["front_scan"].data.caching is True
    for mode, want in (("max", 1e6), ("zero", 0.0), ("none", float("inf"))):
        drift.scene.cam = RayCasterCameraCfg(depth_clipping_behavior=mode)
        assert SceneView(_B(), drift.scene, task="drift")["cam"].data.beyond == want


# ---- 3. the C boundary -----------------------------------------------------------------------------------------------

def test_raycast_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in A.WlRayCastParams._fields_]
    probe = tmp_path / "probe.c"
    body = " ".join(f'printf("%zu ", offsetof(WlRayCastParams, {n}));' for n in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_raycaster.h"\n'
                     f'int main(){{{body} printf("%zu %d %d %d %d %d\\n", sizeof(WlRayCastParams), (int)WL_RAYCASTER_VERSION, '
                     '(int)WL_RAYCAST_MAX_RAYS, (int)WL_RAYCAST_ALIGN_BASE, (int)WL_RAYCAST_ALIGN_YAW, (int)WL_RAYCAST_ALIGN_WORLD); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(A.WlRayCastParams, n).offset for n in fields] + [C.sizeof(A.WlRayCastParams), A.WL_RAYCASTER_VERSION, A.RAYCAST_MAX_RAYS,
                                                                     A.RAYCAST_ALIGNMENTS["base"], A.RAYCAST_ALIGNMENTS["yaw"],
                                                                     A.RAYCAST_ALIGNMENTS["world"]]
    assert got == want and fields == ["offset_pos", "offset_quat", "n_rays", "max_distance", "alignment", "vertical"]


def test_raycast_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.RAYCASTER_SIGNATURES) == {"wl_raycast_scan", "wl_raycast_version"}
    assert not declared & (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES))
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_raycast_version() == 2 == A.WL_RAYCASTER_VERSION
    for gone in ("wl_lidar_scan", "wl_lidar_version"):      # the lidar scans through wl_raycast_scan: its own entry is retired
        assert not hasattr(lib, gone), gone


def test_raycast_scan_refuses_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    fake = 1 << 20                 # never dereferenced: every call below returns before any launch
    P, B, H = A.WlRayCastParams, A.WlEnvBuffers, A.WlHeightField
    params = lambda pos=(0.0, 0.0, 0.2), quat=(1.0, 0.0, 0.0, 0.0), nr=676, md=10.0, al=0, vert=0: P(
        (C.c_float * 3)(*pos), (C.c_float * 4)(*quat), nr, md, al, vert)
    bufs = lambda state=fake, stride=128, n=100: B(state, fake, None, fake, stride, n, 0, 1, 0, 0)
    field = lambda nx=800, ny=800, cell=0.05, zs=2.0 ** -13, h=fake, pair=fake: H(h, nx, ny, -20.0, -20.0, cell, 0.0, zs, pair)
    good = dict(p=params(), b=bufs(), hf=field(), pyr=fake, starts=fake, dirs=fake, scale=None, dist=fake, hits=fake)
    column = dict(p=params(al=1, vert=1), dirs=None)

    def call(**kw):
        a = {**good, **kw}
        ref = lambda s: C.byref(s) if s is not None else None
        return lib.wl_raycast_scan(ref(a["p"]), ref(a["b"]), ref(a["hf"]), a["pyr"], a["starts"], a["dirs"], a["scale"], a["dist"],
                                   a["hits"], None)
    inf, nan = float("inf"), float("nan")
    empty = bufs(n=0)
    # n == 0: WL_OK, nothing launched -- in every legal shape of the call
    assert call(b=empty) == 0 and call(b=empty, p=params(nr=A.RAYCAST_MAX_RAYS)) == 0
    assert call(b=empty, hits=None) == 0 and call(b=empty, dist=None) == 0 and call(b=empty, scale=fake) == 0
    for al in (1, 2):
        assert call(b=empty, p=params(al=al)) == 0 and call(b=empty, p=params(al=al, vert=1), dirs=None) == 0
    assert call(b=empty, p=params(al=1, vert=1, quat=(0.8, 0.0, 0.0, 0.6)), dirs=None) == 0          # a mount about z
    for k in ("p", "b", "hf", "pyr", "dirs"):
        assert call(**{k: None}) == -1, k
    # no start table: every ray leaves the sensor origin -- legal in the general form only
    assert call(b=empty, starts=None) == 0 and call(b=empty, starts=None, hits=None, scale=fake) == 0
    assert call(starts=None, p=params(al=1, vert=1), dirs=None) == -1 and call(b=empty, starts=None, p=params(al=1, vert=1), dirs=None) == -1
    assert call(dist=None, hits=None) == -1                                # both outputs NULL
    assert call(b=bufs(state=None)) == -1 and call(hf=field(h=None)) == -1
    for nr in (0, -1, A.RAYCAST_MAX_RAYS + 1):
        assert call(p=params(nr=nr)) == -1, nr
    for md in (0.0, -1.0, inf, nan):
        assert call(p=params(md=md)) == -1, md
    for pos in ((nan, 0.0, 0.0), (0.0, inf, 0.0)):
        assert call(p=params(pos=pos)) == -1
    for quat in ((0.0, 0.0, 0.0, 0.0), (nan, 0.0, 0.0, 0.0), (inf, 0.0, 0.0, 0.0), (1e30, 1e30, 0.0, 0.0)):
        assert call(p=params(quat=quat)) == -1, quat
    for al in (-1, 3):
        assert call(p=params(al=al)) == -1, al
    # the column form: yaw or world alignment, a mount about z alone, no directions, the pair table
    assert call(b=empty, **column) == 0
    assert call(p=params(al=0, vert=1), dirs=None) == -1                    # vertical with base alignment
    assert call(p=params(al=1, vert=1, quat=(0.9914449, 0.0, 0.1305262, 0.0)), dirs=None) == -1     # vertical with a tilted mount
    assert call(p=params(al=2, vert=1, quat=(0.9914449, 0.1305262, 0.0, 0.0)), dirs=None) == -1
    assert call(p=params(al=1, vert=1)) == -1                               # directions given with vertical
    assert call(p=params(al=1, vert=2), dirs=None) == -1
    assert call(hf=field(pair=None), **column) == -1
    assert call(b=empty, hf=field(pair=None)) == 0                          # the walk does not read the pair table
    assert call(hf=field(pair=fake + 2), **column) == -3
    # the heightfield checks of wl_visual_depth
    for f in (field(nx=1), field(ny=1), field(cell=0.0), field(cell=inf), field(zs=0.0), field(zs=nan), field(nx=16386, ny=4),
              field(nx=4, ny=16386)):
        assert call(hf=f) == -1
    assert call(b=bufs(n=-1)) == -1
    assert call(b=bufs(stride=64, n=100)) == -1                            # stride below n
    assert call(b=bufs(stride=1 << 24, n=100)) == -1                       # rows beyond one 32-bit buffer resource
    assert call(b=bufs(stride=200064, n=200000), p=params(nr=A.RAYCAST_MAX_RAYS)) == -1      # more waves than a grid holds
    for k, v in (("pyr", fake + 2), ("starts", fake + 1), ("dirs", fake + 2), ("scale", fake + 1), ("dist", fake + 2), ("hits", fake + 3)):
        assert call(**{k: v}) == -3, k
    assert call(b=bufs(state=fake + 2)) == -3
    # a lidar's shape of the call: no start table, distances only, no scale
    lidar = dict(starts=None, scale=None, hits=None)
    assert call(b=empty, **lidar) == 0 and call(**lidar, dist=None) == -1 and call(**lidar, dist=fake + 2) == -3
    assert call(**lidar, dirs=None) == -1 and call(**lidar, dirs=fake + 1) == -3 and call(**lidar, p=params(md=inf)) == -1


# ---- 5. the device functions on the host -----------------------------------------------------------------------------

def _fields():
    from oracle import heightfield as HF
    yield "bench", HF.make_terrain(), 0.0, None
    for g in ("G1", "G4b", "G6"):
        f = HC.get(g)
        yield g, (f.heights, f.x0, f.y0, f.cell), f.outside_z, f.z_scale


# one mount per pattern: every alignment, a tilted and a turned mount
MOUNTS = {"grid11x7": dict(offset_pos=(0.6, 0.0, 0.3), offset_rot=(0.9238795, 0.0, 0.0, 0.3826834), alignment="yaw"),
          "lidar360": dict(offset_pos=(0.1, -0.05, 0.25), offset_rot=(0.9914449, 0.0, 0.1305262, 0.0), alignment="base"),
          "pinhole8x12": dict(offset_pos=(0.23, 0.0, 0.18), alignment="world")}


def check_hits(dist, hits, o, w, scale, max_distance):
    """the hit points belong to the distances: start + t direction where the ray hit (fp32 of the coordinates' size), +inf on a miss"""
    sc = 1.0 if scale is None else np.asarray(scale, np.float64)[None]
    t = dist.astype(np.float64) / sc
    miss = ~(t < max_distance * (1 - 1e-6))
    near = t < max_distance * (1 - 1e-5)
    assert np.isinf(hits[np.isinf(hits).any(-1)]).all() and not np.isinf(hits[near]).any()
    assert (np.isinf(hits).all(-1) <= miss).all()
    p = o + t[..., None] * w
    tol = 8 * np.spacing(np.float32(np.abs(p[near]).max() + t[near].max()))
    np.testing.assert_allclose(hits[near], p[near], rtol=0, atol=float(tol))


@pytest.mark.parametrize("max_distance", [5.0, 30.0])
def test_walked_rays_on_the_host_match_the_oracle(hostlib, max_distance):
    """bench field and G1, G4b, G6; the three patterns, each on its own mount and alignment; poses beyond the grid's edge too"""
    pats = RR.patterns()
    for i, (name, field, oz, zs) in enumerate(_fields()):
        pos, quat = LR.poses(48, seed=60 + i, field=field, outside_z=oz, margin=1.0)
        hit_any = miss_any = False
        for pname, (starts, dirs, scale) in pats.items():
            mount = MOUNTS[pname]
            dist, hits = host_scan(hostlib, field, pos, quat, starts, dirs, max_distance, oz, zs, scale=scale, **mount)
            want = RR.distances(pos, quat, starts, dirs, field, max_distance, oz, scale=None, **mount)
            sc = np.ones(len(starts)) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
            # un-scaled; a miss is what the hit point says it is (max_distance x scale / scale need not round back to max_distance)
            t = np.where(np.isinf(hits[..., 0]), max_distance, dist / sc[None])
            LR.check(t, want, max_distance, (name, pname))
            assert (dist >= 0).all() and (dist <= max_distance * sc[None] * (1 + 1e-7)).all()
            check_hits(dist, hits, *RR.world_rays(pos, quat, starts, dirs, **mount), scale, max_distance)
            hit_any, miss_any = hit_any or (want < max_distance).any(), miss_any or (want >= max_distance).any()
        assert hit_any and miss_any, name


def test_no_start_table_on_the_host_equals_a_table_of_zeros(hostlib):
    """a lidar fan on the bench field, tilted mount, base and yaw alignment: the same bits with and without the start table"""
    from oracle import heightfield as HF
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    field = HF.make_terrain()
    pos, quat = LR.poses(16, seed=80, field=field, margin=1.0)
    dirs = LidarPatternCfg(channels=4, vertical_fov_range=(-15.0, 5.0), horizontal_res=3.0).directions()
    for alignment in ("base", "yaw"):
        mount = dict(offset_pos=(0.1, -0.05, 0.25), offset_rot=(0.9914449, 0.0, 0.1305262, 0.0), alignment=alignment)
        table = host_scan(hostlib, field, pos, quat, np.zeros_like(dirs), dirs, 10.0, **mount)
        none = host_scan(hostlib, field, pos, quat, None, dirs, 10.0, **mount)
        for a, b in zip(table, none):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert (table[0] < 10.0).any() and (table[0] == 10.0).any()


# the elevation scanner's grid 20 m above the car and a look-ahead grid 0.3 m above it (30 m: past the relief of every field here, so that no column misses)
COLUMNS = {"26x26@20m": (dict(size=(2.5, 2.5), resolution=0.1), dict(offset_pos=(0.0, 0.0, 20.0), alignment="yaw"), 30.0),
           "11x7@0.3m": (dict(size=(1.0, 0.6), resolution=0.1), dict(offset_pos=(0.6, 0.0, 0.3), offset_rot=(0.9238795, 0.0, 0.0, 0.3826834),
                                                                   alignment="yaw"), 30.0),
           "11x7world": (dict(size=(1.0, 0.6), resolution=0.1), dict(offset_pos=(0.0, 0.0, 0.3), alignment="world"), 30.0)}


def check_column(dist, hits, pos, quat, starts, field, max_distance, oz, mount, what):
    """the column form against float64: hit xy and z within raycaster_reference.column_bounds, the distance within the z bound plus
    two roundings of the start height (its sum and the difference); no ray of the reference misses"""
    t, o, z = RR.column(pos, quat, starts, field, max_distance, oz, **mount)
    assert (t < max_distance).all(), what
    xy_tol, z_tol = RR.column_bounds(field, o)
    exy = np.abs(hits[..., :2].astype(np.float64) - o[..., :2]).max()
    above = t > 0
    ez = np.abs(hits[..., 2].astype(np.float64) - np.where(above, z, o[..., 2]))
    t_tol = z_tol + 2 * float(np.spacing(np.float32(np.abs(o[..., 2]).max())))
    et = np.abs(dist.astype(np.float64) - t).max()
    print(f"column form {what}: xy err {exy:.2e} (bound {xy_tol:.2e}), z err {ez.max():.2e} (bound {z_tol:.2e}), t err {et:.2e} (bound {t_tol:.2e})")
    assert np.isfinite(hits).all() and exy <= xy_tol and ez.max() <= z_tol + (0 if above.all() else t_tol) and et <= t_tol, what


def test_column_form_on_the_host_matches_float64_bilinear_and_the_walk(hostlib):
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg
    for i, (name, field, oz, zs) in enumerate(_fields()):
        pos, quat = LR.poses(48, seed=70 + i, field=field, outside_z=oz, margin=1.0)
        for cname, (grid, mount, md) in COLUMNS.items():
            starts, dirs = GridPatternCfg(**grid).rays()
            dist, hits = host_scan(hostlib, field, pos, quat, starts, dirs, md, oz, zs, vertical=True, **mount)
            check_column(dist, hits, pos, quat, starts, field, md, oz, mount, (name, cname))
            # the same rays through the walk, and the oracle's walk: the reference alone (walk against float64 bilinear) first
            t64, _, _ = RR.column(pos, quat, starts, field, md, oz, **mount)
            want = RR.distances(pos, quat, starts, dirs, field, md, oz, **mount)
            LR.check(want, t64, md, ("reference alone", name, cname))
            walked, _ = host_scan(hostlib, field, pos, quat, starts, dirs, md, oz, zs, vertical=False, **mount)
            LR.check(walked, want, md, ("walk", name, cname))
            LR.check(dist, walked, md, ("column vs walk", name, cname))


def test_host_closed_forms_on_the_plane(hostlib):
    """z = 0 plane: a level car's vertical grid reads its sensor height; pitched with base alignment h / cos; yaw alignment ignores the
    tilt; world alignment ignores the yaw too"""
    from oracle.mathlib import quat_from_euler_xyz
    from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg
    plane = (np.zeros((3, 3), np.float32), np.float32(-1.0), np.float32(-1.0), np.float32(1.0))
    starts, dirs = GridPatternCfg(size=(1.0, 0.6), resolution=0.1).rays()
    e = np.array([[0.0, 0.0, 0.0], [0.0, 0.3, 0.0], [0.2, -0.25, 1.1]], np.float32)
    quat = quat_from_euler_xyz(e[:, 0], e[:, 1], e[:, 2]).astype(np.float32)
    pos = np.array([[3.0, -2.0, 0.32], [3.0, -2.0, 0.32], [150.0, 40.0, 0.07]], np.float32)
    h = pos[:, 2].astype(np.float64) + 0.25
    base, hb = host_scan(hostlib, plane, pos, quat, starts, dirs, 30.0, offset_pos=(0.0, 0.0, 0.25), alignment="base")
    np.testing.assert_allclose(base[0], h[0], rtol=1e-6)
    # pitched by 0.3: the sensor sits at z + 0.25 cos, its rays lean by 0.3 and start x sin lower / higher along the grid's x
    want = (pos[1, 2] + 0.25 * np.cos(0.3) - starts[:, 0] * np.sin(0.3)) / np.cos(0.3)
    np.testing.assert_allclose(base[1], want, rtol=1e-5)
    np.testing.assert_allclose(hb[..., 2], 0.0, atol=1e-6)
    for vertical in (False, True):
        yaw, hy = host_scan(hostlib, plane, pos, quat, starts, dirs, 30.0, offset_pos=(0.0, 0.0, 0.25), alignment="yaw", vertical=vertical)
        np.testing.assert_allclose(yaw, np.repeat(h[:, None], 77, 1), rtol=1e-6)
        world, hw = host_scan(hostlib, plane, pos, quat, starts, dirs, 30.0, offset_pos=(0.0, 0.0, 0.25), alignment="world", vertical=vertical)
        np.testing.assert_allclose(world, np.repeat(h[:, None], 77, 1), rtol=1e-6)
        np.testing.assert_allclose(hw[..., :2] - pos[:, None, :2], np.repeat(starts[None, :, :2], 3, 0), atol=2e-5)    # unrotated
        assert np.abs(hy[2, :, :2] - pos[2, None, :2] - starts[None, :, :2]).max() > 0.1                              # yaw turns them

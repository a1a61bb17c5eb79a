"""CPU checks of the lidar: the beam pattern's count and order, LidarCfg's defaults, the scene's views, and the device's per-ray
functions (wl_raycast_dev.h) compiled for the host, driven with a lidar's table (no starts) and held to the float64 reference
(tests/lidar_reference.py: oracle/depth.c one ray per beam).  The C entry a lidar scans through is the ray caster's
(tests/test_raycaster_cpu.py: layout, symbols, every argument refusal)."""
import math

import numpy as np
import pytest

from tests import heightfield_cases as HC
from tests import lidar_reference as LR
from tests import raycaster_host as RH
from tests.raycaster_host import hostlib  # noqa: F401  (the fixture)


# ---- pattern and config ----------------------------------------------------------------------------------------------

def test_360_degree_pattern_has_one_beam_per_degree_and_no_duplicate_azimuth():
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    el, az = LidarPatternCfg(channels=1, vertical_fov_range=(0.0, 0.0), horizontal_fov_range=(-180.0, 180.0), horizontal_res=1.0).angles()
    assert len(az) == 360 and (el == 0).all()
    np.testing.assert_allclose(az, -180.0 + np.arange(360), atol=1e-9)
    assert len(np.unique(np.round(np.mod(az, 360.0), 9))) == 360          # -180 and +180 are one direction: only one of them
    el, az = LidarPatternCfg(horizontal_fov_range=(0.0, 360.0), horizontal_res=0.5).angles()
    assert len(az) == 720 and az[0] == 0.0 and az[-1] == 359.5


def test_count_rule_of_open_patterns():
    """span not 360: ceil(span / res) + 1 azimuths, both ends included (the documented formula, pinned)"""
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    _, az = LidarPatternCfg(horizontal_fov_range=(-135.0, 135.0), horizontal_res=0.25).angles()
    assert len(az) == 1081 and az[0] == -135.0 and az[-1] == 135.0 and np.allclose(np.diff(az), 0.25)
    _, az = LidarPatternCfg(horizontal_fov_range=(-135.0, 135.0), horizontal_res=1.0).angles()
    assert len(az) == 271
    _, az = LidarPatternCfg(horizontal_fov_range=(-45.0, 45.0), horizontal_res=0.7).angles()     # res does not divide the span
    assert len(az) == math.ceil(90.0 / 0.7) + 1 and az[0] == -45.0 and az[-1] == 45.0 and (np.diff(az) <= 0.7).all()
    _, az = LidarPatternCfg(horizontal_fov_range=(10.0, 10.0)).angles()                          # a single azimuth
    assert list(az) == [10.0]
    with pytest.raises(ValueError):
        LidarPatternCfg(horizontal_res=0.0).angles()


def test_multi_channel_pattern_is_channel_major_and_unit():
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    pat = LidarPatternCfg(channels=16, vertical_fov_range=(-15.0, 15.0), horizontal_fov_range=(-180.0, 180.0), horizontal_res=1.0)
    el, az = pat.angles()
    assert len(el) == 16 * 360
    np.testing.assert_allclose(el.reshape(16, 360), np.repeat(np.linspace(-15.0, 15.0, 16)[:, None], 360, 1))
    np.testing.assert_allclose(az.reshape(16, 360), np.repeat((-180.0 + np.arange(360))[None], 16, 0), atol=1e-9)
    d = pat.directions()
    np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    np.testing.assert_allclose(np.degrees(np.arcsin(d[:, 2])), el, atol=1e-9)
    np.testing.assert_allclose(np.degrees(np.arctan2(d[:, 1], d[:, 0])).reshape(16, 360)[:, 1:], az.reshape(16, 360)[:, 1:], atol=1e-9)
    # azimuth 0 looks along +x, +90 along +y (left), elevation +15 up; beam 270 is channel 0 (-15 degrees) at azimuth +90
    c, s = math.cos(math.radians(15)), math.sin(math.radians(15))
    np.testing.assert_allclose(d[15 * 360 + 180], [c, 0.0, s], atol=1e-15)
    np.testing.assert_allclose(d[270], [0.0, c, -s], atol=1e-15)


def test_lidar_cfg_defaults_and_miss_values():
    from wheeledlab_amd.envs.scene import LidarData
    from wheeledlab_amd.envs.sensors_cfg import LidarCfg
    c = LidarCfg()
    assert c.pattern_cfg.channels == 1 and c.pattern_cfg.horizontal_fov_range == (-180.0, 180.0) and c.pattern_cfg.horizontal_res == 1.0
    assert len(c.pattern_cfg.directions()) == 360
    assert c.offset_pos == (0.0, 0.0, 0.18) and c.offset_rot == (1.0, 0.0, 0.0, 0.0) and c.attach_yaw_only is False
    assert (c.min_range, c.max_range, c.miss_value) == (0.1, 10.0, "max")
    assert LidarCfg().pattern_cfg is not c.pattern_cfg                   # per-instance defaults

    class _B:
        n, device = 4, "cpu"
    for mode, want in (("max", None), ("zero", 0.0), ("none", float("inf"))):
        assert LidarData(_B(), LidarCfg(miss_value=mode)).beyond == want
    with pytest.raises(KeyError):
        LidarData(_B(), LidarCfg(miss_value="nan"))


def test_scene_registers_every_lidar_under_its_attribute_name():
    from wheeledlab_amd import registry, tasks  # noqa: F401
    from wheeledlab_amd.envs.scene import LidarView, SceneView
    from wheeledlab_amd.envs.sensors_cfg import LidarCfg
    cfg = registry.parse_env_cfg("Isaac-MushrElevationRL-v0", device="cpu", num_envs=4)
    cfg.scene.lidar = LidarCfg()
    cfg.scene.rear_lidar = LidarCfg(offset_rot=(0.0, 0.0, 0.0, 1.0))

    class _B:
        n, device = 4, "cpu"
    scene = SceneView(_B(), cfg.scene, task="elevation")
    assert isinstance(scene["lidar"], LidarView) and isinstance(scene.sensors["rear_lidar"], LidarView)
    assert scene["rear_lidar"].cfg.offset_rot == (0.0, 0.0, 0.0, 1.0) and "height_scanner" in scene.sensors
    assert "lidar" not in SceneView(_B(), registry.parse_env_cfg("Isaac-MushrElevationRL-v0", device="cpu", num_envs=4).scene,
                                    task="elevation").sensors


# ---- the device functions on the host --------------------------------------------------------------------------------

def host_scan(hostlib, field, pos, quat, dirs, max_range, outside_z=0.0, z_scale=None, offset_pos=(0.0, 0.0, 0.18),
              offset_rot=(1.0, 0.0, 0.0, 0.0), yaw_only=False):
    """ranges [n, B]: the ray caster's host simulation without a start table (every beam leaves the sensor origin), as LidarScanner
    calls the kernel"""
    return RH.host_scan(hostlib, field, pos, quat, None, dirs, max_range, outside_z, z_scale, offset_pos=offset_pos,
                        offset_rot=offset_rot, alignment="yaw" if yaw_only else "base")[0]


@pytest.mark.parametrize("max_range", [10.0, 30.0])
def test_device_beams_on_the_host_match_the_oracle(hostlib, max_range):
    """bench field and two non-bench fields, a planar and a 16-channel pattern, a tilted mount and the yaw-only flag"""
    from oracle import heightfield as HF
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    planar = LidarPatternCfg().directions()
    multi = LidarPatternCfg(channels=16, vertical_fov_range=(-15.0, 15.0), horizontal_res=4.0).directions()
    mounts = (dict(), dict(offset_pos=(0.1, -0.05, 0.25), offset_rot=(0.9914449, 0.0, 0.1305262, 0.0)), dict(yaw_only=True))
    bench = HF.make_terrain()
    fields = [(bench, 0.0, None)] + [((HC.get(g).heights, HC.get(g).x0, HC.get(g).y0, HC.get(g).cell), HC.get(g).outside_z,
                                      HC.get(g).z_scale) for g in ("G1", "G4b")]
    for i, (field, oz, zs) in enumerate(fields):
        pos, quat = LR.poses(48, seed=30 + i, field=field, outside_z=oz, margin=1.0)
        for dirs in (planar, multi):
            for mount in mounts:
                got = host_scan(hostlib, field, pos, quat, dirs, max_range, oz, zs, **mount)
                want = LR.ranges(pos, quat, dirs, field, max_range, oz, **mount)
                LR.check(got, want, max_range, (i, len(dirs), mount))
                assert (got >= 0).all() and (got <= max_range).all()


def test_host_beams_closed_forms_on_the_plane(hostlib):
    """z = 0 plane, level sensor at height h: horizontal beams read max_range, a beam pitched down by theta reads h / sin(theta)"""
    plane = (np.zeros((3, 3), np.float32), np.float32(-1.0), np.float32(-1.0), np.float32(1.0))
    th = np.radians([0.0, 2.0, 5.0, 10.0, 30.0, 60.0, 90.0])
    az = np.radians(np.arange(0, 360, 45.0))
    dirs = np.stack([np.outer(np.cos(th), np.cos(az)).ravel(), np.outer(np.cos(th), np.sin(az)).ravel(), np.repeat(-np.sin(th), len(az))], 1)
    pos = np.array([[3.0, -2.0, 0.32], [150.0, 40.0, 0.07]], np.float32)
    quat = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], np.float32)
    got = host_scan(hostlib, plane, pos, quat, dirs, 30.0).reshape(2, len(th), len(az))
    for e in range(2):
        h = float(pos[e, 2]) + 0.18
        assert (got[e, 0] == 30.0).all()
        want = np.minimum(h / np.sin(th[1:]), 30.0)
        np.testing.assert_allclose(got[e, 1:], np.repeat(want[:, None], len(az), 1), rtol=1e-5)

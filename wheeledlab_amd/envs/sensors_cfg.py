"""Sensor / command config classes named as in `isaaclab.sensors` / `isaaclab.envs.mdp.commands` (values only)."""
from .configclass import MISSING, configclass


@configclass
class GridPatternCfg:
    size: tuple = MISSING
    resolution: float = MISSING
    direction: tuple = (0.0, 0.0, -1.0)


@configclass
class RayCasterCfg:
    prim_path: str = ""
    offset_pos: tuple = (0.0, 0.0, 0.0)
    attach_yaw_only: bool = True
    pattern_cfg: GridPatternCfg = GridPatternCfg(size=(1.0, 1.0), resolution=0.1)
    mesh_prim_paths: list = []
    debug_vis: bool = False


@configclass
class PinholeCameraCfg:
    focal_length: float = 24.0
    horizontal_aperture: float = 20.955
    vertical_aperture: float = 15.29
    clipping_range: tuple = (0.01, 1e2)


@configclass
class TiledCameraCfg:
    prim_path: str = ""
    update_period: float = 0.0
    height: int = 60
    width: int = 80
    data_types: list = ["rgb"]
    spawn: PinholeCameraCfg = PinholeCameraCfg()
    offset_pos: tuple = (0.0, 0.0, 0.0)
    offset_rot: tuple = (1.0, 0.0, 0.0, 0.0)
    offset_convention: str = "ros"
    body_pos: tuple = (0.23, 0.0, 0.18)   # pose of the camera in the base frame (designed: camera_link is in the missing USD)
    # what a depth pixel beyond the far clipping plane reads: "max" (the far distance), "zero", or "none" (+inf) -- the switch of
    # IsaacLab's camera cfgs [IsaacLab-recalled; its own default is "none"]; "max" here keeps observation rows finite
    depth_clipping_behavior: str = "max"
    debug_vis: bool = False


@configclass
class LidarPatternCfg:
    """Beam directions of a spinning lidar, IsaacLab's `LidarPatternCfg` field names (degrees).  Beams are channel-major: all azimuths
    of the lowest channel, then the next channel up.  Channels: `channels` elevations evenly from vertical_fov_range[0] to [1] (one
    channel: the first).  Azimuths: ceil(span / horizontal_res) + 1 evenly from horizontal_fov_range[0] to [1], both ends included,
    except that a span of 360 degrees drops the last one (it is the first again) [IsaacLab-recalled: the count rule of its
    `lidar_pattern`, not checked against its source here; tests/test_lidar_cpu.py pins this formula].  360 at 1 degree: 360 beams;
    270 at 0.25 degrees: 1081."""
    channels: int = 1
    vertical_fov_range: tuple = (0.0, 0.0)
    horizontal_fov_range: tuple = (-180.0, 180.0)
    horizontal_res: float = 1.0

    def angles(self):
        """(elevation, azimuth) of every beam in degrees, float64 numpy [B] each, channel-major"""
        import math

        import numpy as np
        lo, hi = (float(a) for a in self.horizontal_fov_range)
        span = hi - lo
        if not (int(self.channels) >= 1 and float(self.horizontal_res) > 0 and span >= 0):
            raise ValueError(f"lidar pattern: channels >= 1, horizontal_res > 0, horizontal_fov_range ascending (got {self})")
        n_az = math.ceil(span / float(self.horizontal_res) - 1e-9) + 1
        az = np.linspace(lo, hi, n_az)
        if abs(span - 360.0) < 1e-6 and n_az > 1:
            az = az[:-1]
        el = np.linspace(float(self.vertical_fov_range[0]), float(self.vertical_fov_range[1]), int(self.channels))
        e, a = np.meshgrid(el, az, indexing="ij")
        return e.reshape(-1), a.reshape(-1)

    def directions(self):
        """unit beam directions in the sensor frame (x forward, y left, z up), float64 numpy [B, 3], channel-major"""
        import numpy as np
        e, a = (np.deg2rad(v) for v in self.angles())
        return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1)


@configclass
class LidarCfg:
    """A lidar of the scene: range scans of every env against the terrain (sensors.LidarScanner, csrc/wl_lidar.hip), exposed as
    `env.scene.sensors[name].data` with `output["linear_depth"]` [N, B] -- what `mdp.lidar_ranges` / `mdp.lidar_ranges_normalized`
    read, the latter with `min_range` / `max_range` -- and `ray_hits_w`, `pos_w`, `quat_w`.  Opt-in: `cfg.scene.lidar = LidarCfg()`.
    Terrain only (the heightfield of the elevation and visual-depth tasks, the z = 0 plane of the others), not other cars.
    The defaults are a single-channel 360 degree scanner at 1 degree and 10 m, the class of planar lidar a MuSHR car carries, mounted
    0.18 m above the base link: DESIGNED values -- the robots' USDs, which would place the sensor, are not available."""
    prim_path: str = ""
    pattern_cfg: LidarPatternCfg = LidarPatternCfg()
    offset_pos: tuple = (0.0, 0.0, 0.18)           # sensor origin in the body frame (m)
    offset_rot: tuple = (1.0, 0.0, 0.0, 0.0)       # sensor frame against the body (w, x, y, z)
    attach_yaw_only: bool = False                  # True: only the body's yaw turns the offset and the beams
    min_range: float = 0.1
    max_range: float = 10.0
    # what a beam that meets nothing within max_range reads: "max" (max_range), "zero", or "none" (+inf) -- like the camera's
    # depth_clipping_behavior; "max" keeps observation rows finite
    miss_value: str = "max"
    mesh_prim_paths: list = []
    debug_vis: bool = False


@configclass
class UniformPose2dCommandRanges:
    pos_x: tuple = MISSING
    pos_y: tuple = MISSING
    heading: tuple = MISSING


@configclass
class UniformPose2dCommandCfg:
    asset_name: str = "robot"
    simple_heading: bool = True
    resampling_time_range: tuple = MISSING
    ranges: UniformPose2dCommandRanges = MISSING
    debug_vis: bool = False
    Ranges = UniformPose2dCommandRanges

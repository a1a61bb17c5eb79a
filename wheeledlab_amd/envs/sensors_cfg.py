"""Sensor / command config classes named as in `isaaclab.sensors` / `isaaclab.envs.mdp.commands` (values only)."""
from .configclass import MISSING, configclass


@configclass
class GridPatternCfg:
    """Parallel rays from a grid of points in the sensor's z = 0 plane, IsaacLab's `GridPatternCfg` field names.  Points per axis:
    floor((size + 1e-9) / resolution) + 1 at -size / 2 + i resolution (IsaacLab's `arange(-s / 2, s / 2 + 1e-9, res)` [recalled]):
    2.5 m at 0.1 m is 26 per axis.  `ordering` "xy": x fastest (what RayCasterData documents), "yx": y fastest.  `direction` is
    normalised; every ray starts in the z = 0 plane whatever the direction."""
    size: tuple = MISSING
    resolution: float = MISSING
    direction: tuple = (0.0, 0.0, -1.0)
    ordering: str = "xy"

    def counts(self):
        """(points along x, points along y)"""
        import math
        res = float(self.resolution)
        if not (res > 0 and all(float(s) >= 0 for s in self.size)):
            raise ValueError(f"grid pattern: resolution > 0 and size >= 0 (got {self})")
        return tuple(int(math.floor((float(s) + 1e-9) / res)) + 1 for s in self.size[:2])

    def rays(self):
        """(starts [R, 3], unit directions [R, 3]) in the sensor frame, float64 numpy"""
        import numpy as np
        if self.ordering not in ("xy", "yx"):
            raise ValueError(f"grid pattern ordering {self.ordering!r} ('xy' or 'yx')")
        nx, ny = self.counts()
        x = -0.5 * float(self.size[0]) + float(self.resolution) * np.arange(nx)
        y = -0.5 * float(self.size[1]) + float(self.resolution) * np.arange(ny)
        if self.ordering == "xy":
            gy, gx = np.meshgrid(y, x, indexing="ij")
        else:
            gx, gy = np.meshgrid(x, y, indexing="ij")
        starts = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(nx * ny)], 1)
        d = np.asarray(self.direction, np.float64)
        n = np.linalg.norm(d)
        if not (np.isfinite(n) and n > 0):
            raise ValueError(f"grid pattern direction {self.direction} is not a direction")
        return starts, np.repeat((d / n)[None], nx * ny, 0)


@configclass
class PinholeCameraPatternCfg:
    """One ray through every pixel centre of a pinhole camera, row-major (IsaacLab's `PinholeCameraPatternCfg` field names; lengths in
    one unit, as USD's millimetres).  fx = width focal_length / horizontal_aperture, fy = height focal_length / vertical_aperture
    (`None`: square pixels, horizontal_aperture height / width), cx = width / 2 + horizontal_aperture_offset fx, cy = height / 2 +
    vertical_aperture_offset fy [IsaacLab-recalled: the inverse of its `from_intrinsic_matrix`].  The rays are given in the WORLD
    convention of a camera frame (x forward along the optical axis, y left, z up): pixel (row, col) looks along
    (1, -(col + 0.5 - cx) / fx, -(row + 0.5 - cy) / fy), normalised -- the visual camera's rays (csrc/wl_depth_dev.h)."""
    focal_length: float = 24.0
    horizontal_aperture: float = 20.955
    vertical_aperture: float = None
    horizontal_aperture_offset: float = 0.0
    vertical_aperture_offset: float = 0.0
    width: int = MISSING
    height: int = MISSING

    def intrinsics(self):
        """(fx, fy, cx, cy) in pixels"""
        w, h = int(self.width), int(self.height)
        va = self.vertical_aperture if self.vertical_aperture is not None else float(self.horizontal_aperture) * h / w
        if not (w >= 1 and h >= 1 and float(self.focal_length) > 0 and float(self.horizontal_aperture) > 0 and float(va) > 0):
            raise ValueError(f"pinhole pattern: width, height >= 1, focal length and apertures > 0 (got {self})")
        fx, fy = w * float(self.focal_length) / float(self.horizontal_aperture), h * float(self.focal_length) / float(va)
        return fx, fy, w / 2 + float(self.horizontal_aperture_offset) * fx, h / 2 + float(self.vertical_aperture_offset) * fy

    def rays(self):
        """(starts [H W, 3] (zeros), unit directions [H W, 3]) in the sensor frame (world convention), float64 numpy, row-major"""
        import numpy as np
        fx, fy, cx, cy = self.intrinsics()
        r, c = np.meshgrid(np.arange(int(self.height)), np.arange(int(self.width)), indexing="ij")
        d = np.stack([np.ones(r.size), -((c.reshape(-1) + 0.5 - cx) / fx), -((r.reshape(-1) + 0.5 - cy) / fy)], 1)
        return np.zeros_like(d), d / np.linalg.norm(d, axis=1, keepdims=True)


@configclass
class RayCasterCfg:
    """A ray caster of the scene (sensors.RayCaster, csrc/wl_raycast.hip): `pattern_cfg` is a GridPatternCfg, a LidarPatternCfg (all
    rays from the sensor origin) or a PinholeCameraPatternCfg.  `ray_alignment` "base" (the body's full rotation turns offset and
    rays), "yaw" (its yaw alone) or "world" (none); `None`: "yaw" if attach_yaw_only else "base".  Every RayCasterCfg attribute of a
    scene config becomes `env.scene.sensors[name]` on every task; the elevation task's own `height_scanner` stays the fused scan."""
    prim_path: str = ""
    offset_pos: tuple = (0.0, 0.0, 0.0)
    offset_rot: tuple = (1.0, 0.0, 0.0, 0.0)       # sensor frame against the body (w, x, y, z)
    attach_yaw_only: bool = True
    ray_alignment: str = None
    pattern_cfg: GridPatternCfg = GridPatternCfg(size=(1.0, 1.0), resolution=0.1)
    max_distance: float = 1e6
    mesh_prim_paths: list = []
    debug_vis: bool = False

    def alignment(self) -> str:
        a = self.ray_alignment if self.ray_alignment is not None else ("yaw" if self.attach_yaw_only else "base")
        if a not in ("base", "yaw", "world"):
            raise ValueError(f"ray_alignment {a!r} ('base', 'yaw' or 'world')")
        return a


def pattern_rays(pattern_cfg):
    """(starts, unit directions) [R, 3] float64 of any pattern a ray caster accepts; a lidar pattern's beams leave the origin"""
    import numpy as np
    if isinstance(pattern_cfg, LidarPatternCfg):
        d = pattern_cfg.directions()
        return np.zeros_like(d), d
    if isinstance(pattern_cfg, (GridPatternCfg, PinholeCameraPatternCfg)):
        return pattern_cfg.rays()
    raise TypeError(f"a ray caster takes a GridPatternCfg, LidarPatternCfg or PinholeCameraPatternCfg, not {type(pattern_cfg).__name__}")


# sensor frame in the WORLD convention (x forward, y left, z up) against the same camera's frame in each convention (w, x, y, z):
# offset_rot_world = offset_rot (x) CAMERA_CONVENTION_TO_WORLD[convention].  "ros": z forward, x right, y down; "opengl": -z forward,
# x right, y up (IsaacLab's three offset conventions)
CAMERA_CONVENTION_TO_WORLD = {"world": (1.0, 0.0, 0.0, 0.0), "ros": (0.5, 0.5, -0.5, 0.5), "opengl": (0.5, -0.5, 0.5, 0.5)}


@configclass
class RayCasterCameraCfg:
    """A depth camera of any resolution and intrinsics as a ray caster (IsaacLab's `RayCasterCameraCfg`): `env.scene.sensors[name]
    .data.output["distance_to_image_plane" | "distance_to_camera"]` [N, H, W, 1], `intrinsic_matrices`, `pos_w`, `quat_w_ros` /
    `quat_w_world`.  The body's full rotation turns the camera.  `offset_rot` is read in `offset_convention`; what a pixel beyond
    `max_distance` reads is `depth_clipping_behavior`'s, as TiledCameraCfg."""
    prim_path: str = ""
    pattern_cfg: PinholeCameraPatternCfg = PinholeCameraPatternCfg(width=80, height=60)
    data_types: list = ["distance_to_image_plane"]
    offset_pos: tuple = (0.0, 0.0, 0.0)
    offset_rot: tuple = (1.0, 0.0, 0.0, 0.0)
    offset_convention: str = "ros"
    max_distance: float = 1e6
    depth_clipping_behavior: str = "max"
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
    """A lidar of the scene: range scans of every env against the terrain (sensors.LidarScanner, csrc/wl_raycast.hip), exposed as
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

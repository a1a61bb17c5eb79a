"""The sensors that read a DeviceHeightField from the poses of any batch: DepthCamera (the visual task's pinhole camera as a depth
image), LidarScanner (range scans) and RayCaster (any ray table: grids, lidar fans, pinhole images), and the per-batch cache of
cameras (_cached_depth_camera, keyed by _field_key).  A sensor takes a batch as an argument; this module imports field, never core.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _abi as A
from .field import DeviceHeightField, _canonical_device


class DepthCamera:
    """The visual task's pinhole camera rendering distance_to_image_plane against a heightfield (wl_visual_depth): its parameters
    and a view of the field (`hf`: its own outside plane, the field's buffers and its one bound pyramid), renders the poses of ANY
    batch (rows WL_S_PX.. / WL_S_QW.. of its state matrix).  Reference hook: mdp_sensors/observations.py:89-95; camera
    visual/mushr_visual_env_cfg.py:230-246."""

    IMG_H, IMG_W = 60, 80

    def __init__(self, heightfield, device="cuda:0", params: A.WlVisualParams | None = None, outside_z: float | None = None):
        from .params import visual_params
        self.lib = A.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("DepthCamera needs a HIP device; there is no CPU path")
        self.p = params if params is not None else visual_params()
        self.hf = DeviceHeightField(heightfield, self.device, outside_z)     # a tuple (quantised here) or a batch's own `.hf` (shared)
        self.height, self._hf = self.hf.heights, self.hf.struct
        self._pyr = self.hf.pyramid.data_ptr()    # resolved once: the field rebuilds its pyramid in place (refresh), never moves it

    pyramid = property(lambda self: self.hf.pyramid)

    def build_pyramid(self):
        """the field's derived tables (the pyramid among them) from its codes as they are now"""
        self.hf.refresh()

    def render(self, batch, max_depth: float = 20.0, out: torch.Tensor | None = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(batch.n, self.IMG_H, self.IMG_W, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == batch.n * self.IMG_H * self.IMG_W
        A.check(self.lib.wl_visual_depth(C.byref(self.p), C.byref(batch._bufs), C.byref(self._hf), self._pyr,
                                         float(max_depth), out.data_ptr(), A.stream(self.device)), "wl_visual_depth")
        return out


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


class RayCaster:
    """A ray caster (envs.sensors_cfg.RayCasterCfg or RayCasterCameraCfg) casting its table of rays against the terrain from the poses
    of ANY batch (wl_raycast_scan).  Owns the table, built once from the pattern: `ray_starts` / `ray_dirs` [R, 3] in the sensor
    frame (`ray_starts` None: all zero, no table is loaded) and, for a pinhole pattern, `ray_scale` [R] (each ray's cosine to the
    optical axis: distances come out as distances to the image plane).  `vertical` -- every direction exactly (0, 0, -1), alignment yaw or world, mount about z only -- is decided here
    and selects the kernel's column form (one bilinear sample per ray instead of a walk); `vertical=False` forces the walk.
    scan() -> (distances [n, R], hits [n, R, 3]): the distance clipped at max_distance (max_distance on a miss, 0 from under the
    terrain; times ray_scale), the hit point (+inf on a miss)."""
    _plane = None

    def camera_of(self, batch) -> DepthCamera:
        """the terrain the batch's cars stand on, as CameraData does it: the visual-depth task's own camera, the elevation task's
        heightfield, else the z = 0 plane (a 3 x 3 zero grid: beyond it the outside plane is z = 0 as well)"""
        if getattr(batch, "camera", None) is not None:
            return batch.camera
        if batch.hf is not None:
            return _cached_depth_camera(batch, batch.hf)
        if self._plane is None:       # one tensor per sensor: the batch's camera cache keys on it
            self._plane = (torch.zeros(3, 3, dtype=torch.float32, device=self.device), -1.0, -1.0, 1.0)
        return _cached_depth_camera(batch, self._plane)

    def __init__(self, cfg, device="cuda:0", vertical: bool | None = None):
        import numpy as np

        from .envs.sensors_cfg import CAMERA_CONVENTION_TO_WORLD, PinholeCameraPatternCfg, RayCasterCameraCfg, pattern_rays
        self.lib = A.load()
        self.device = _canonical_device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("RayCaster needs a HIP device; there is no CPU path")
        self.cfg = cfg
        starts, dirs = pattern_rays(cfg.pattern_cfg)
        self.n_rays = int(dirs.shape[0])
        if not 1 <= self.n_rays <= A.RAYCAST_MAX_RAYS:
            raise ValueError(f"a ray pattern of {self.n_rays} rays (1 .. {A.RAYCAST_MAX_RAYS})")
        self.max_distance = float(cfg.max_distance)
        if not (math.isfinite(self.max_distance) and self.max_distance > 0):
            raise ValueError(f"ray caster max_distance must be positive and finite, got {cfg.max_distance}")
        q = tuple(float(v) for v in cfg.offset_rot)
        is_camera = isinstance(cfg, RayCasterCameraCfg)
        if is_camera:
            if cfg.offset_convention not in CAMERA_CONVENTION_TO_WORLD:
                raise ValueError(f"offset_convention {cfg.offset_convention!r} (one of {sorted(CAMERA_CONVENTION_TO_WORLD)})")
            q = _quat_mul(q, CAMERA_CONVENTION_TO_WORLD[cfg.offset_convention])
        qn = math.sqrt(sum(v * v for v in q))
        if not (math.isfinite(qn) and qn > 0):
            raise ValueError(f"ray caster offset_rot must be a non-zero quaternion, got {cfg.offset_rot}")
        self.alignment = "base" if is_camera else cfg.alignment()
        column = bool((dirs == np.array([0.0, 0.0, -1.0])).all()) and self.alignment in ("yaw", "world") and q[1] == 0.0 and q[2] == 0.0
        if vertical and not column:
            raise ValueError("the column form needs directions (0, 0, -1), yaw or world alignment and a mount about z alone")
        self.vertical = column if vertical is None else bool(vertical)
        to_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).contiguous().to(self.device)
        self.ray_starts, self.ray_dirs = to_dev(starts), to_dev(dirs)
        # image-plane distance = Euclidean distance x the ray's x component (the optical axis is the sensor's +x)
        self.ray_scale = to_dev(dirs[:, 0]) if isinstance(cfg.pattern_cfg, PinholeCameraPatternCfg) else None
        self.params = A.WlRayCastParams((C.c_float * 3)(*[float(v) for v in cfg.offset_pos]), (C.c_float * 4)(*[v / qn for v in q]),
                                        self.n_rays, self.max_distance, A.RAYCAST_ALIGNMENTS[self.alignment], int(self.vertical))

    def scan(self, batch, camera: DepthCamera | None = None, dist: torch.Tensor | bool = True, hits: torch.Tensor | bool = True):
        """one launch over the batch's current poses -> (distances or None, hits or None); `dist` / `hits`: a tensor to fill, True for
        a new one, False to leave that output out; `camera`: another terrain (a DepthCamera) than the batch's own"""
        cam = camera if camera is not None else self.camera_of(batch)
        if dist is True:
            dist = torch.empty(batch.n, self.n_rays, dtype=torch.float32, device=self.device)
        if hits is True:
            hits = torch.empty(batch.n, self.n_rays, 3, dtype=torch.float32, device=self.device)
        dist, hits = (None if dist is False else dist), (None if hits is False else hits)
        for t, shape in ((dist, (batch.n, self.n_rays)), (hits, (batch.n, self.n_rays, 3))):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.shape == shape)
        ptr = lambda t: None if t is None else t.data_ptr()
        A.check(self.lib.wl_raycast_scan(C.byref(self.params), C.byref(batch._bufs), C.byref(cam._hf), cam._pyr, ptr(self.ray_starts),
                                         None if self.vertical else self.ray_dirs.data_ptr(), ptr(self.ray_scale), ptr(dist), ptr(hits),
                                         A.stream(self.device)), "wl_raycast_scan")
        return dist, hits

    def render(self, batch, camera: DepthCamera | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """distances [batch.n, R]"""
        return self.scan(batch, camera, dist=True if out is None else out, hits=False)[0]

    def hits(self, batch, camera: DepthCamera | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """hit points [batch.n, R, 3] in the world, +inf on a miss"""
        return self.scan(batch, camera, dist=False, hits=True if out is None else out)[1]


class LidarScanner(RayCaster):
    """A lidar (envs.sensors_cfg.LidarCfg) scanning the terrain from the poses of ANY batch: the RayCaster of its beam pattern -- every
    beam from the sensor origin (`ray_starts` None: no start table), attach_yaw_only as yaw or base alignment, max_range as
    max_distance -- always walked: a fan that points straight down on a yaw mount stays a lidar, it does not switch to the column
    form.  `cfg` is the LidarCfg.
    render() -> ranges [n, B], the raw scan: the hit's Euclidean range clipped at max_range, max_range on a miss, 0 from under
    the terrain (what a miss reads in the scene is LidarData's business)."""

    def __init__(self, cfg=None, device="cuda:0"):
        from .envs.sensors_cfg import LidarCfg, RayCasterCfg
        lidar = cfg if cfg is not None else LidarCfg()
        super().__init__(RayCasterCfg(pattern_cfg=lidar.pattern_cfg, offset_pos=lidar.offset_pos, offset_rot=lidar.offset_rot,
                                      attach_yaw_only=bool(lidar.attach_yaw_only), max_distance=lidar.max_range), device, vertical=False)
        self.cfg = lidar
        self.ray_starts = None        # every beam leaves the sensor origin: no start table, the kernel loads none

    n_beams = property(lambda self: self.n_rays)
    beam_dirs = property(lambda self: self.ray_dirs)
    max_range = property(lambda self: self.max_distance)

    def render(self, batch, out: torch.Tensor | None = None, camera: DepthCamera | None = None) -> torch.Tensor:
        """ranges [batch.n, B] of the batch's current poses; `camera`: another terrain (a DepthCamera) than the batch's own"""
        return super().render(batch, camera, out)


def _field_key(heightfield) -> tuple:
    """What tells one `heightfield` argument from another (pure: needs no device).  A DeviceHeightField: its shared buffers' identity and
    the view's outside plane -- it refreshes its tables in place, so no version.  A tuple is a SNAPSHOT: the array object, placement,
    shape, vertical scale (the same codes under another one are another field) and -- for tensors -- the in-place version counter."""
    if isinstance(heightfield, DeviceHeightField):
        return id(heightfield._shared), heightfield.outside_z
    h, x0, y0, cell = heightfield[:4]
    return (id(h), float(x0), float(y0), float(cell), tuple(h.shape), getattr(h, "_version", None),
            float(heightfield[4]) if len(heightfield) > 4 else None)


def _cached_depth_camera(batch, heightfield) -> DepthCamera:
    """one DepthCamera per batch and array (or shared buffers): built on first use, and again when _field_key tells the argument
    from the last one -- a newer snapshot of an array replaces the older (a tuple becomes a DeviceHeightField of its own)"""
    cache = batch.__dict__.setdefault("_depth_cameras", {})
    key = _field_key(heightfield)
    hit = cache.get(key[0])
    if hit is None or hit[0] != key:
        # (the entry holds the argument alive: an id is only unique among live objects)
        hit = cache[key[0]] = (key, heightfield, DepthCamera(heightfield, batch.device, batch.p if isinstance(batch.p, A.WlVisualParams) else None))
    return hit[2]

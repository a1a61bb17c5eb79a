"""The viewer camera: one world camera that draws every env of a batch (wl_viewer_render, include/wheeledlab_amd_viewer.h) -- what
IsaacLab's viewport shows at `cfg.viewer.eye -> lookat`, for env.render() and video recording.

Every task uses env_spacing 0, so all cars share one world frame and one camera sees them all.  The ground is the batch's own: the
plane z = 0 (drift: a two-tone 1 m checker; visual: the traversability map as albedo) or the heightfield through the depth camera's
bound pyramid (elevation; visual-depth with the map's albedo).  Rendering only reads the pose rows of the state matrix."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi as A

# designed: the Kit viewport's default perspective camera is taken as 18.147 mm focal length over a 20.955 mm horizontal aperture,
# i.e. 60 degrees (from memory; not checked against a running Kit)
DEFAULT_HFOV_DEG = 60.0
DEFAULT_FAR_CLIP = 500.0
# designed chassis box of the MuSHR car in its root frame (the root rests on the ground at nominal load): centre, half extents
CHASSIS_CENTER = (0.0, 0.0, 0.09)
CHASSIS_HALF = (0.22, 0.10, 0.045)
SUN = (0.35, -0.45, 0.82)
AMBIENT = 0.35


def look_at(eye, lookat):
    """camera pose of a look-at: -> (pos [3] float32, quat [4] float32 (w, x, y, z)) of the camera body frame, whose +x is the optical
    axis f = normalise(lookat - eye), +y the image's left (-right, right = normalise(f x z), with y as the up vector when f is
    parallel to z) and +z the image's up"""
    e = np.asarray(eye, np.float64)
    f = np.asarray(lookat, np.float64) - e
    n = np.linalg.norm(f)
    if not n > 0:
        raise ValueError("viewer eye and lookat coincide")
    f /= n
    right = np.cross(f, [0.0, 0.0, 1.0])
    if np.linalg.norm(right) < 1e-9:
        right = np.cross(f, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    R = np.stack([f, -right, up], 1)          # columns: body x, y, z in the world
    return e.astype(np.float32), quat_from_matrix(R).astype(np.float32)


def quat_from_matrix(R):
    """(w, x, y, z) of a rotation matrix (Shepperd's branch on the largest diagonal term), w >= 0"""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q)
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def intrinsics(width, height, hfov_deg=DEFAULT_HFOV_DEG):
    """fx = fy = (W / 2) / tan(hfov / 2), cx = W / 2, cy = H / 2"""
    f = 0.5 * width / math.tan(math.radians(hfov_deg) / 2)
    return f, f, 0.5 * width, 0.5 * height


def viewer_params(width, height, eye, lookat, vehicle=None, hfov_deg=DEFAULT_HFOV_DEG, far_clip=DEFAULT_FAR_CLIP, ground=A.VIEWER_PLANE,
                  plane_z=0.0, checker=1.0, env_index=0, id_offset=0) -> A.WlViewerParams:
    """WlViewerParams of a look-at camera; `vehicle`: the batch's WlVehicleParams (wheel spheres), default the MuSHR car's"""
    if vehicle is None:
        from .params import mushr_vehicle
        vehicle = mushr_vehicle()
    p = A.WlViewerParams()
    p.width, p.height = int(width), int(height)
    pos, quat = look_at(eye, lookat)
    p.cam_pos[:] = [float(v) for v in pos]
    p.cam_quat[:] = [float(v) for v in quat]
    p.fx, p.fy, p.cx, p.cy = intrinsics(width, height, hfov_deg)
    p.far_clip, p.ground, p.plane_z, p.checker = float(far_clip), int(ground), float(plane_z), float(checker)
    p.sun[:] = list(SUN)
    p.ambient = AMBIENT
    p.box_center[:], p.box_half[:] = list(CHASSIS_CENTER), list(CHASSIS_HALF)
    p.half_wheelbase_f, p.half_wheelbase_r = vehicle.half_wheelbase_f, vehicle.half_wheelbase_r
    p.half_track, p.wheel_z, p.wheel_radius = vehicle.half_track, vehicle.wheel_z, vehicle.wheel_radius
    p.env_index, p.id_offset = int(env_index), int(id_offset)
    return p


class Viewer:
    """Owns the frame's scratch; renders any batch of this package (DriftBatch, ElevBatch, VisualBatch, VisualDepthBatch) from a
    look-at camera.  A heightfield ground is the batch's DeviceHeightField and its own bound pyramid (built on first use)."""

    def __init__(self, device="cuda:0", resolution=(1280, 720), hfov_deg: float = DEFAULT_HFOV_DEG, far_clip: float = DEFAULT_FAR_CLIP):
        self.lib = A.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("the viewer needs a HIP device; there is no CPU path")
        self.width, self.height = int(resolution[0]), int(resolution[1])
        self.hfov_deg, self.far_clip = float(hfov_deg), float(far_clip)
        self._scratch = None

    def _scratch_for(self, n):
        need = int(self.lib.wl_viewer_scratch_bytes(self.width, self.height, int(n)))
        if need <= 0:
            raise A.WlError(f"viewer frame {self.width} x {self.height} of {n} envs is outside the supported range")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch, need

    def _pyramid(self, batch):
        return batch.hf.struct, batch.hf.pyramid

    def params(self, batch, eye, lookat, env_index: int = 0) -> A.WlViewerParams:
        return viewer_params(self.width, self.height, eye, lookat, batch.p.vehicle, self.hfov_deg, self.far_clip,
                             ground=A.VIEWER_HEIGHTFIELD if batch.hf is not None else A.VIEWER_PLANE, env_index=env_index,
                             id_offset=int(batch.env_offset))

    def render(self, batch, eye, lookat, env_index: int = 0, out=None, depth=None, ids=None) -> torch.Tensor:
        """-> uint8 [H, W, 3] on the device (`out` if given); optional `depth` float32 [H, W] (distance along the optical axis,
        far_clip for the sky) and `ids` int32 [H, W] (env index, -1 ground, -2 sky) are filled when passed"""
        H, W = self.height, self.width
        if out is None:
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
        for t, dt, shape in ((out, torch.uint8, (H, W, 3)), (depth, torch.float32, (H, W)), (ids, torch.int32, (H, W))):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"viewer output must be a contiguous {dt} tensor of shape {shape} on {self.device}")
        p = self.params(batch, eye, lookat, env_index)
        scratch, need = self._scratch_for(batch.n)
        hf, pyr = (None, None)
        if p.ground == A.VIEWER_HEIGHTFIELD:
            hf, pyr = self._pyramid(batch)
        m = getattr(batch, "_map", None)
        A.check(self.lib.wl_viewer_render(C.byref(p), C.byref(batch._bufs), C.byref(hf) if hf is not None else None,
                                          pyr.data_ptr() if pyr is not None else None, C.byref(m) if m is not None else None,
                                          scratch.data_ptr(), need, out.data_ptr(), depth.data_ptr() if depth is not None else None,
                                          ids.data_ptr() if ids is not None else None, A.stream(self.device)), "wl_viewer_render")
        return out

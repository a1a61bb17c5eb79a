"""The lidar's float64 reference -- TEST INFRASTRUCTURE.  No new restatement of the walk: oracle/depth.c (wl_oracle_depth) called
with a 1 x 1 image (cx = cy = 0.5, the camera at the root) casts exactly ONE ray along the body +x axis of the quaternion it is handed,
and with a unit direction that ray's parameter at the hit is its range.  So every beam becomes one "camera": the sensor origin as the
root position, and a quaternion whose +x axis is the beam's world direction (built in float64, rounded to float32).

The sensor frame is restated here in float64 from the header's definition (include/wheeledlab_amd_raycaster.h): origin = pos + R offset,
rotation R mount, with R the body's rotation or, with yaw_only, its yaw alone."""
from types import SimpleNamespace

import numpy as np

from oracle import depth as D
from oracle import heightfield as HF
from oracle.mathlib import matrix_from_quat, quat_from_euler_xyz

_ONE_RAY = SimpleNamespace(cam_pos=(0.0, 0.0, 0.0), fx=1.0, fy=1.0, cx=0.5, cy=0.5)


def _mat64(q):
    w, x, y, z = (np.asarray(q, np.float64)[..., i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def sensor_frames(pos, quat, offset_pos=(0.0, 0.0, 0.18), offset_rot=(1.0, 0.0, 0.0, 0.0), yaw_only=False):
    """float64 sensor origins [n, 3] and rotations sensor -> world [n, 3, 3] of roots at pos [n, 3] / quat [n, 4] (float32 values)"""
    q = np.asarray(quat, np.float32).astype(np.float64)
    R = _mat64(q)
    if yaw_only:
        yaw = np.arctan2(R[:, 1, 0], R[:, 0, 0])
        c, s = np.cos(yaw), np.sin(yaw)
        z, o = np.zeros_like(c), np.ones_like(c)
        R = np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)
    m = np.asarray(offset_rot, np.float64)
    mount = _mat64(m / np.linalg.norm(m))
    origin = np.asarray(pos, np.float32).astype(np.float64) + R @ np.asarray(offset_pos, np.float64)
    return origin, R @ mount


def x_axis_quat(w):
    """unit quaternions [.., 4] (w, x, y, z) whose rotation takes +x to the unit vectors w [.., 3] (float64)"""
    w = np.asarray(w, np.float64)
    flip = w[..., 0] < 0                        # near -x the shortest arc degenerates: turn by pi about z first
    v = np.where(flip[..., None], w * np.array([-1.0, -1.0, 1.0]), w)
    q = np.stack([1.0 + v[..., 0], np.zeros_like(v[..., 0]), -v[..., 2], v[..., 1]], -1)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    qf = np.stack([-q[..., 3], -q[..., 2], q[..., 1], q[..., 0]], -1)     # (0, 0, 0, 1) x q
    return np.where(flip[..., None], qf, q)


def ranges(pos, quat, dirs, field, max_range, outside_z=0.0, **mount):
    """oracle ranges [n, B] float32 of beams dirs [B, 3] (sensor frame) from roots pos / quat over field = (heights, x0, y0, cell)"""
    origin, M = sensor_frames(pos, quat, **mount)
    w = np.einsum("nij,bj->nbi", M, np.asarray(dirs, np.float64))
    w /= np.linalg.norm(w, axis=-1, keepdims=True)
    n, B = w.shape[:2]
    q = x_axis_quat(w).astype(np.float32).reshape(-1, 4)
    o = np.repeat(origin.astype(np.float32), B, 0)
    return D.depth(_ONE_RAY, o, q, field, max_range, outside_z=outside_z, img_h=1, img_w=1).reshape(n, B)


def poses(n, seed, field, outside_z=0.0, margin=0.0, tilt=0.15, lift=(0.04, 0.3)):
    """-> pos [n, 3], quat [n, 4] float32: roots `lift` above the terrain (the bilinear field, outside_z beyond it) at uniform xy over the
    grid's extent widened by `margin` metres, N(0, tilt) roll / pitch, uniform yaw"""
    h, x0, y0, cell = field[:4]
    ny, nx = np.shape(h)
    rng = np.random.RandomState(seed)
    lo, hi = np.array([x0, y0], np.float64) - margin, np.array([x0 + (nx - 1) * cell, y0 + (ny - 1) * cell], np.float64) + margin
    xy = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
    z, _, _ = HF.sample(h, x0, y0, cell, xy[:, 0], xy[:, 1], outside=outside_z)
    pos = np.concatenate([xy, (z + rng.uniform(*lift, n))[:, None]], 1).astype(np.float32)
    e = np.stack([rng.normal(0, tilt, n), rng.normal(0, tilt, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    return pos, np.ascontiguousarray(quat_from_euler_xyz(e[:, 0], e[:, 1], e[:, 2]).astype(np.float32))


def mismatch(got, want, max_range):
    """(relative error [n, B], hit / miss disagreement [n, B] bool) -- the yardstick of tests/test_gpu_depth_parity.py: the 0.999
    quantile of the relative error and the fraction of disagreements both below 1e-4"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-3)
    return rel, (g < max_range) != (w < max_range)


def check(got, want, max_range, what=""):
    rel, flip = mismatch(got, want, max_range)
    q = float(np.quantile(rel, 0.999))
    assert q < 1e-4 and flip.mean() < 1e-4, (what, q, int(flip.sum()), flip.size, float(rel.max()))
    return rel, flip


def matrix(quat):
    return matrix_from_quat(np.asarray(quat, np.float32))

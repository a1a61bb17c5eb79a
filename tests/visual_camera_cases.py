"""Poses, maps, intrinsics and augmentation settings of the camera tests (tests/visual_camera_reference.py) -- shared by the CPU test, which
checks the cap on excused pixels for every case list, and the GPU test, which runs them.  Everything is fp32 as the kernel is handed it."""
import os
from types import SimpleNamespace

import numpy as np

F = np.float32
N_POSES = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visual_trav.npz")

# (brightness, contrast, blur sigma, contrast before brightness)
AUG_EXISTING = ((1.0, 1.0, 0.0, 0), (1.4, 0.85, 1.7, 0), (0.5, 1.15, 0.4, 0), (1.4, 0.85, 1.7, 1), (1.7, 1.2, 0.0, 1), (0.4, 1.2, 3.0, 1))
AUG_EXTREMES = ((1.0, 0.9, 0.1, 0), (1.0, 0.9, 5.0, 0),                                          # sigma's ends
                (0.2, 0.9, 1.0, 0), (1.8, 0.9, 1.0, 0),                                          # brightness's
                (1.3, 0.8, 1.0, 0), (1.3, 0.8, 1.0, 1), (1.3, 1.2, 1.0, 0), (1.3, 1.2, 1.0, 1),  # contrast's, both orders
                (1.3, 1.0, 1.5, 0),                                                              # contrast 1 with blur
                (0.7, 1.1, 0.0, 0),                                                              # contrast != 1 without blur
                (1.6, 1.0, 0.0, 1), (1.6, 1.0, 2.0, 1))                                          # contrast_first with contrast 1
AUGS = AUG_EXISTING + AUG_EXTREMES


def default_params():
    """the camera's fields of WlVisualParams at the task's defaults (oracle/visual_step.visual_params)"""
    return SimpleNamespace(cam_pos=[0.23, 0.0, 0.18], fx=80 * 1.9299999475479126 / 3.8959999084472656,
                           fy=60 * 1.9299999475479126 / 2.453000068664551, cx=40.0, cy=30.0, sky=0.5,
                           brightness=1.0, contrast=1.0, blur_sigma=0.0, contrast_first=0)


INTRINSICS = {
    "default": {},
    "shifted": dict(cx=37.3, cy=33.1, fx=default_params().fx * 1.2, fy=default_params().fy * 0.85, cam_pos=[0.2, 0.07, 0.25]),
    "sky0": dict(sky=0.0),
    "sky1": dict(sky=1.0),
}


def params(intr="default", aug=(1.0, 1.0, 0.0, 0)):
    p = default_params()
    for k, v in INTRINSICS[intr].items():
        setattr(p, k, v)
    p.brightness, p.contrast, p.blur_sigma, p.contrast_first = aug
    return p


def pattern_map(n):
    """one-cell pattern without a symmetry: white iff (3 ix + 5 iy) mod 7 < 3 -- every cell line is a class edge somewhere, and a
    transposed or mirrored lookup reads another class"""
    iy, ix = np.mgrid[0:n, 0:n]
    return (3 * ix + 5 * iy) % 7 < 3


def maps():
    """name -> (map [N, N] bool, spacing)"""
    g = np.load(GOLDEN)
    golden = np.unpackbits(g["full_map_packed"])[: 500 * 500].reshape(500, 500).astype(bool)
    return {"golden": (golden, 0.5), "pat500": (pattern_map(500), 0.5), "pat101": (pattern_map(101), 0.3),
            "pat64": (pattern_map(64), 1.0), "pat600": (pattern_map(600), 0.5)}


def quat_rpy(roll, pitch, yaw):
    """[n, 4] fp32 (w, x, y, z) of R = Rz(yaw) Ry(pitch) Rx(roll), normalised in fp32"""
    roll, pitch, yaw = (np.asarray(a, np.float64) * 0.5 for a in np.broadcast_arrays(roll, pitch, yaw))
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1).astype(F)
    return (q / np.sqrt((q * q).sum(-1, keepdims=True, dtype=F))).astype(F)


def _xy(rng, n, half, margin):
    return rng.uniform(-(half - margin), half - margin, (n, 2))


def poses(kind, n_map, spacing, seed=0):
    """-> (pos [64, 3], quat [64, 4]) fp32 for a square map of n_map cells of `spacing` metres"""
    rng = np.random.RandomState(1000 + seed)
    n, half = N_POSES, n_map * spacing / 2
    yaw = (np.arange(n) + rng.uniform(0, 1, n)) * (2 * np.pi / n)                     # over the circle
    if kind == "level":                                                               # reset poses: a cell's centre, z 0.1, yawed
        ij = rng.randint(0, n_map, (n, 2))
        pos = np.concatenate([(ij - n_map // 2) * spacing, np.full((n, 1), 0.1)], -1)
        q = quat_rpy(0.0, 0.0, yaw)
    elif kind == "tilt":                                                              # roll +-0.6, pitch +-0.5 (+-0.6 at the ends)
        pos = np.concatenate([_xy(rng, n, half, 3.0), rng.uniform(0.05, 0.4, (n, 1))], -1)
        roll, pitch = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n)
        roll[:4], pitch[:4] = (0.6, -0.6, 0.6, -0.6), (0.6, 0.6, -0.6, -0.6)
        q = quat_rpy(roll, pitch, yaw)
    elif kind == "down":                                                              # nose down: the whole image is near ground
        pos = np.concatenate([_xy(rng, n, half, 4.0), rng.uniform(0.05, 1.5, (n, 1))], -1)
        q = quat_rpy(rng.uniform(-0.3, 0.3, n), rng.uniform(0.7, 1.3, n), yaw)
    elif kind == "flipped":                                                           # on a side, on the roof, nose down / up
        pos = np.concatenate([_xy(rng, n, half, 3.0), rng.uniform(0.05, 0.4, (n, 1))], -1)
        roll = np.choose(np.arange(n) % 4, [np.pi / 2, -np.pi / 2, np.pi, 0.0]) + rng.uniform(-0.05, 0.05, n)
        pitch = np.where(np.arange(n) % 4 == 3, np.where(np.arange(n) % 8 == 3, np.pi / 2, -np.pi / 2), 0.0) + rng.uniform(-0.05, 0.05, n)
        roll[:8], pitch[:8] = roll[:8].round(6), pitch[:8].round(6)
        roll[:4], pitch[:4] = (np.pi / 2, -np.pi / 2, np.pi, 0.0), (0.0, 0.0, 0.0, np.pi / 2)   # and each exactly
        q = quat_rpy(roll, pitch, yaw)
    elif kind == "height":                                                            # z 0.05 .. 5, camera AT z = 0, camera below it
        z = np.geomspace(0.05, 5.0, n)
        roll, pitch = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.5, n)
        z[:16], roll[:16], pitch[:16] = -0.18, 0.0, 0.0                               # level: o_z = fl(-0.18f + 0.18f) = 0 exactly
        z[16:32] = -rng.uniform(0.2, 2.0, 16)                                         # below the plane
        pos = np.concatenate([_xy(rng, n, half, 6.0), z[:, None]], -1)
        q = quat_rpy(roll, pitch, yaw)
    elif kind == "border":                                                            # within +-2 m of every edge and corner
        k = np.arange(n)
        off = rng.uniform(-2.0, 2.0, (n, 2))
        along = rng.uniform(-half, half, n)
        sx, sy = np.where(k % 2, 1.0, -1.0), np.where((k // 2) % 2, 1.0, -1.0)
        x = np.where(k % 8 < 4, sx * half + off[:, 0], along)
        y = np.where(k % 8 < 4, sy * half + off[:, 1], np.where(k % 8 < 6, along, sy * half + off[:, 1]))
        x = np.where((k % 8 >= 4) & (k % 8 < 6), sx * half + off[:, 0], x)
        pos = np.stack([x, y, rng.uniform(0.05, 0.6, n)], -1)
        pos[-1] = (1.0e4, -3.0e3, 0.1)                                                # and one car 10 km away
        pos[-2] = (half, -half, 0.1)                                                  # one exactly on a corner
        q = quat_rpy(rng.uniform(-0.4, 0.4, n), rng.uniform(0.1, 1.0, n), yaw)
    else:
        raise KeyError(kind)
    return pos.astype(F), q


# (map, pose kind, intrinsics): the horizon is in view only over the golden map, whose paths are many cells wide -- over the one-cell
# pattern the rows under the horizon (|d_z| ~ 1e-2: a hit error of centimetres) would be ambiguous by the dozen per image, which is the
# reference's fault, not a kernel's; there the cars look down ("down", "border") and every cell line in the image is a sharp test
CASES = (
    ("golden", "level", "default"), ("golden", "tilt", "default"), ("golden", "flipped", "default"), ("golden", "height", "default"),
    ("golden", "border", "default"), ("golden", "down", "shifted"), ("golden", "tilt", "sky0"), ("golden", "tilt", "sky1"),
    ("pat500", "down", "default"), ("pat500", "border", "default"), ("pat500", "down", "shifted"),
    ("pat101", "down", "default"), ("pat101", "border", "default"),
    ("pat64", "down", "default"), ("pat64", "border", "default"),
    ("pat600", "down", "default"), ("pat600", "border", "default"),
)
# the forms tests' start (n = 40): tilted cars and cars at the map's edge
FORMS_N = 40


def forms_poses(n_map, spacing):
    pt, qt = poses("tilt", n_map, spacing, seed=7)
    pb, qb = poses("border", n_map, spacing, seed=7)
    pos, q = np.concatenate([pt[:20], pb[:20]]), np.concatenate([qt[:20], qb[:20]])
    pos[:, 2] = np.maximum(pos[:, 2], F(0.08))
    return pos, q


def velocities(n, seed=0):
    """linear, angular velocity and last action [n, 3 | 3 | 2] fp32; actions reach beyond +-1"""
    rng = np.random.RandomState(2000 + seed)
    act = rng.uniform(-1.6, 1.6, (n, 2))
    act[:4] = ((1.0, -1.0), (1.0000001, -1.0000001), (0.99999994, 3.0), (-2.5, 0.0))
    return rng.uniform(-3, 3, (n, 3)).astype(F), rng.uniform(-4, 4, (n, 3)).astype(F), act.astype(F)

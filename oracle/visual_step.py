"""Fused visual env.step() + camera observation -- numpy restatement of `wl_visual_step` (order: IsaacLab
ManagerBasedRLEnv.step() with the plugins of wheeledlab_tasks/visual/mushr_visual_env_cfg.py).
The camera is DESIGNED: the reference renders an RGB image of the black/white traversability plane with RTX
(:230-246) and augments it with torchvision (mdp_sensors/observations.py:75-87); here each pixel is one ray against
the z = 0 plane with a map lookup, followed by the same brightness / contrast / Gaussian-blur / grayscale / normalise
chain (saturation and hue jitter are identities on a grey image)."""
import math

import numpy as np

from . import env_step as ES
from . import philox as PH
from . import vehicle as V
from . import visual_mdp as VM
from .layout import ACT0, DAMP, EPSUM0, MASS, MU_D, MU_S, PX, QW, S_COUNT, VX
from .layout import M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS, M_TERM0, M_TIMEOUTS  # noqa: F401 -- re-exported
from .mathlib import F, f32, matrix_from_quat
from .params import NS, mushr_action, mushr_vehicle

IMG_H, IMG_W, CROP = 60, 80, 20
N_PIX = (IMG_H - CROP) * IMG_W
OBS_DIM = N_PIX + 8


def visual_params():
    """MushrVisualRLEnvCfg (:412-444)"""
    return NS(
        sim_dt=0.02, decimation=10, max_episode_length=math.ceil(10.0 / (0.02 * 10)),           # :435-439
        action=mushr_action(1), vehicle=mushr_vehicle(drive=1, motor_limit=0.25, substeps=1, ground_mu=(2.0, 2.0), implicit=1),   # h = sim.dt
        weight=[5.0, 7.0, 0, 0, 0, 0, 0, 0],                                                    # :375-385
        map_rows=500, map_cols=500, row_spacing=0.5, col_spacing=0.5,                          # :70-76
        reset_z=0.1,                                                                            # :203
        cam_pos=[0.23, 0.0, 0.18], fx=80 * 1.9299999475479126 / 3.8959999084472656,
        fy=60 * 1.9299999475479126 / 2.453000068664551, cx=40.0, cy=30.0,                      # :230-241 (pose: designed)
        sky=0.5, brightness=1.0, contrast=1.0, blur_sigma=0.0, contrast_first=0,
        log_episode_sums=1,
    )


def spawn_cells(trav):
    """indices of traversable cells in np.nonzero order: [M, 2] = (iy, ix) (utils/__init__.py:193)"""
    ys, xs = np.asarray(trav).nonzero()
    return np.stack([ys, xs], -1).astype(np.int32)


def reset_envs(p, state, episode_len, cells, ids, seed, step, env_offset=0, hf=None):
    """hf: the visual-depth extension task's heightfield terrain -- the reset pose is lifted onto it (z 0.1 above the ground)"""
    if len(ids) == 0:
        return
    gid = np.asarray(ids) + env_offset
    u = PH.uniform4(gid, step, 0, seed)
    k = np.minimum((u[0] * F(len(cells))).astype(np.int64), len(cells) - 1)
    iy, ix = cells[k, 0], cells[k, 1]
    state[PX, ids] = (ix.astype(F) - F(p.map_cols // 2)) * F(p.row_spacing)          # generate_random_poses :198-199
    state[PX + 1, ids] = (iy.astype(F) - F(p.map_rows // 2)) * F(p.col_spacing)
    state[PX + 2, ids] = F(p.reset_z)
    if hf is not None:
        from . import heightfield as H
        h, x0, y0, cell, outside = H.unpack(hf)
        zt, _, _ = H.sample(h, x0, y0, cell, state[PX, ids], state[PX + 1, ids], outside=outside)
        state[PX + 2, ids] = (F(p.reset_z) + zt.astype(F)).astype(F)
    yaw = u[1] * F(2.0 * math.pi)                                                     # U(0, 360) deg
    state[QW, ids], state[QW + 1, ids], state[QW + 2, ids], state[QW + 3, ids] = np.cos(yaw * F(.5)), 0, 0, np.sin(yaw * F(.5))
    state[VX:VX + 6, ids] = 0
    state[ACT0:ACT0 + 2, ids] = 0
    state[EPSUM0:EPSUM0 + 8, ids] = 0
    episode_len[ids] = 0


def gaussian_kernel5(sigma):
    x = np.linspace(-2, 2, 5)
    k = np.exp(-0.5 * (x / sigma) ** 2)
    return (k / k.sum()).astype(F)


def camera(p, state, trav):
    """-> [n, 3200] normalised grey image rows (cropped 40 x 80, row-major)"""
    n = state.shape[1]
    R = matrix_from_quat(state[QW:QW + 4].T)
    o = state[PX:PX + 3].T + np.einsum("nij,j->ni", R, f32(p.cam_pos))
    rows = np.arange(CROP, IMG_H, dtype=np.float32)
    cols = np.arange(IMG_W, dtype=np.float32)
    dy = -((cols + F(0.5) - F(p.cx)) / F(p.fx))               # body y (left positive) of the ray, x_cam = right
    dz = -((rows + F(0.5) - F(p.cy)) / F(p.fy))               # body z, y_cam = down
    db = np.stack([np.ones((len(rows), len(cols)), F), np.broadcast_to(dy[None, :], (len(rows), len(cols))),
                   np.broadcast_to(dz[:, None], (len(rows), len(cols)))], -1).reshape(-1, 3)
    dw = np.einsum("nij,pj->npi", R, db).astype(F)            # [n, pix, 3]
    hit = dw[..., 2] < F(-1e-6)
    t = np.where(hit, -o[:, None, 2] / np.where(hit, dw[..., 2], F(-1)), F(0)).astype(F)
    hx = o[:, None, 0] + t * dw[..., 0]
    hy = o[:, None, 1] + t * dw[..., 1]
    half_w, half_h = F(p.map_rows * p.row_spacing / 2), F(p.map_cols * p.col_spacing / 2)
    on_map = hit & (np.abs(hx) <= half_w) & (np.abs(hy) <= half_h)
    tv = VM.get_traversability(trav, np.stack([hx.reshape(-1), hy.reshape(-1)], -1), num_rows=p.map_rows,
                               num_cols=p.map_cols, row_spacing=p.row_spacing, col_spacing=p.col_spacing).reshape(n, -1)
    img = np.where(hit, np.where(on_map & tv, F(1), F(0)), F(p.sky)).astype(F)
    # torchvision ColorJitter.forward: the ops run in the order of a torch.randperm(4) drawn per call (mdp_sensors/observations.py:21,
    # 82: one call per batch).  adjust_brightness: blend with zeros = clamp(b x); adjust_contrast: blend with the mean of the
    # grayscale image, clamp.  Hue is the identity on a grey image, saturation a scale within 1.8e-4 of 1 (tests/test_oracle_
    # golden_elev_visual.py::test_saturation_and_hue_on_a_grey_image): only the brightness / contrast order is modelled.
    def brightness(x):
        return np.clip(x * F(p.brightness), 0, 1)

    def contrast(x):
        if p.contrast == 1.0:
            return x
        mean = (x * F(0.9999)).mean(-1, keepdims=True, dtype=np.float32)    # grayscale mean (0.2989+0.587+0.114)
        return np.clip(F(p.contrast) * x + (F(1) - F(p.contrast)) * mean, 0, 1)
    img = brightness(contrast(img)) if getattr(p, "contrast_first", 0) else contrast(brightness(img))
    if p.blur_sigma > 0:
        k = gaussian_kernel5(p.blur_sigma)
        im = img.reshape(n, IMG_H - CROP, IMG_W)
        pad = np.pad(im, ((0, 0), (0, 0), (2, 2)), mode="reflect")
        im = sum(k[j] * pad[:, :, j:j + IMG_W] for j in range(5))
        pad = np.pad(im, ((0, 0), (2, 2), (0, 0)), mode="reflect")
        im = sum(k[j] * pad[:, j:j + IMG_H - CROP, :] for j in range(5))
        img = im.reshape(n, -1)
    return ((img * F(0.9999) - F(0.5)) / F(0.5)).astype(F)


def observe(p, state, trav):
    v_b, w_b = ES.body_velocities(state)
    return np.concatenate([camera(p, state, trav), v_b, w_b, np.clip(state[ACT0:ACT0 + 2].T, F(-1), F(1))], -1).astype(F)


def observe_depth(p, state, hf, max_depth):
    """observation of the visual-depth extension task (BASELINE config 5): distance_to_image_plane 60 x 80 against the heightfield
    (oracle/depth.c) | base_lin_vel | base_ang_vel | last_action.  hf: a 5-tuple carries the field's outside_z"""
    from . import depth as D
    from . import heightfield as H
    v_b, w_b = ES.body_velocities(state)
    img = D.depth(p, state[PX:PX + 3].T.copy(), state[QW:QW + 4].T.copy(), H.unpack(hf)[:4], max_depth,
                  H.unpack(hf)[4]).reshape(state.shape[1], -1)
    return np.concatenate([img, v_b, w_b, np.clip(state[ACT0:ACT0 + 2].T, F(-1), F(1))], -1).astype(F)


def step(p, state, episode_len, trav, cells, actions, seed, step_count, metrics=None, env_offset=0, hf=None, max_depth=None, probe=None):
    """hf / max_depth: the visual-depth extension task -- the same step on the heightfield terrain `hf` (wheel contacts through
    heightfield.sample, reset onto the terrain), observation = observe_depth"""
    n = state.shape[1]
    steer_t, wheel_t = ES.fwd_targets(p, ES.apply_action(p, state, actions))
    ground = V.flat_ground
    if hf is not None:
        from .elev_step import ground_fn
        ground = ground_fn(hf, probe)
    b = ES.integrate(p, state, steer_t, wheel_t, ground, probe)
    truncated, finite = ES.count_step(p, state, episode_len)
    width, height = p.map_rows * p.row_spacing, p.map_cols * p.col_spacing
    oom = VM.out_of_map(b.pos, width, height)
    terminated = oom | ~finite
    safe = np.where(finite[:, None], b.pos, 0).astype(F)
    kw = dict(num_rows=p.map_rows, num_cols=p.map_cols, row_spacing=p.row_spacing, col_spacing=p.col_spacing)
    terms = np.stack([np.where(VM.get_traversability(trav, safe[:, :2], **kw), F(1), F(-1)), b.v_b[:, 0]]).astype(F)
    terms, reward = ES.book_rewards(p, state, terms, finite)
    # M_TERM0: cars that left the map, the non-finite ones not among them
    ids = ES.end_episodes(state, episode_len, metrics, terminated | truncated, truncated, finite, [(oom & finite).sum()])
    reset_envs(p, state, episode_len, cells, ids, seed, step_count, env_offset, hf)
    obs = observe(p, state, trav) if hf is None else observe_depth(p, state[:, :n], hf, max_depth)
    return obs, reward, terminated, truncated, dict(terms=terms, finite=finite)


def init_state(p, n, seed=0, stride=None, wheel_mu=(0.5, 0.5), mass=3.0):
    """VisualEventsCfg (:253-262) has only the reset event: no randomisation; wheel material = PhysX default 0.5/0.5
    (the USD's own material is unknown), throttle damping 1000 (hound.py:19)"""
    stride = stride or ((n + 63) // 64) * 64
    s = np.zeros((S_COUNT, stride), F)
    s[QW] = 1
    s[MU_S], s[MU_D], s[DAMP], s[MASS] = wheel_mu[0], wheel_mu[1], 1000.0, mass
    return s

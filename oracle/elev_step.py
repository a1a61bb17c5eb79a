"""Fused elevation env.step() -- numpy restatement of what `wl_elev_step` (+ the height-scan kernel) does, in the
order of IsaacLab's ManagerBasedRLEnv.step() with the reference's elevation plugins
(wheeledlab_tasks/elevation/mushr_elevation_env_cfg.py)."""
import numpy as np

from . import elev_mdp as E
from . import env_step as ES
from . import heightfield as H
from . import philox as PH
from .env_step import sym
from .layout import ACT0, CMD_BX, CMD_BY, CMD_TIMER, DAMP, EPSUM0, MASS, MU_D, MU_S, PX, QW, S_COUNT, TGT_H, TGT_X, TGT_Y, VX
from .layout import M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS, M_TERM0, M_TIMEOUTS  # noqa: F401 -- re-exported
from .mathlib import F, f32, euler_xyz_from_quat
from .params import NS, mushr_action, mushr_vehicle

S_RESET, S_CMD_RESET, S_CMD_RESAMPLE = 0, 1, 2
N_RAYS = 26
OBS_DIM = 13 + N_RAYS * N_RAYS


def elev_params():
    """MushrElevationRLEnvCfg (:438-469) flattened"""
    import math
    return NS(
        sim_dt=0.01, decimation=10, max_episode_length=math.ceil(20.0 / (0.01 * 10)),          # :461-465
        action=mushr_action(1), vehicle=mushr_vehicle(drive=1, motor_limit=0.25, substeps=1, ground_mu=(1.0, 1.0), implicit=1),
        weight=[200.0, 5000.0, 0.0, -200.0, 0.0, 0.0, 0.0, 0.0],                                # :286-305
        min_height=0.15, stuck_min_vel=0.02, stuck_wheel_spin=5.0, stuck_vel_cap=1.2,           # :356-366, :155-157
        upright_cos=math.cos(math.radians(60.0)), goal_dist=0.5,                                # :368-376
        fall_vel=0.10, elev_z0=0.19, elev_min=0.1, elev_min_vel=0.1, progress_offset=5.0,       # :166-173, :239-254
        reset_xy=19.0, reset_yaw=3.14, reset_vel=[0.1, 0.2], reset_z=0.25, spawn_clearance=0.06,  # :409-419, :147-149
        cmd_xy=19.0, cmd_heading=3.14, cmd_resample_s=10.0,                                     # :425-435
        scan_size=2.5, scan_res=0.1, scan_offset=0.084, obs_clip=10.0,                          # :74-82, :139
        log_episode_sums=1,
    )


def ground_fn(hf, probe=None):
    """probe (see vehicle.substep): `cell_margin` -- per env the smallest distance, in cells, of a wheel's sample point from a
    cell line of the grid (where the bilinear surface's normal jumps), minimised over every call.  hf: heightfield.unpack's forms
    (a 5-tuple carries the field's outside_z)"""
    h, x0, y0, cell, outside = H.unpack(hf)

    def g(xy):
        z, n, _ = H.sample(h, x0, y0, cell, xy[:, 0], xy[:, 1], outside=outside)
        if probe is not None:
            u = (f32(xy[:, 0]) - F(x0)) / F(cell)
            v = (f32(xy[:, 1]) - F(y0)) / F(cell)
            d = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
            probe["cell_margin"] = np.minimum(probe.get("cell_margin", np.inf), d)
        return z, n
    return g


def yaw_cs(q):
    """cos / sin of the yaw of IsaacLab's yaw_quat(q), without the atan2 round trip"""
    q = f32(q)
    a = F(1) - F(2) * (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    b = F(2) * (q[:, 0] * q[:, 3] + q[:, 1] * q[:, 2])
    inv = F(1) / np.sqrt(a * a + b * b)
    return (a * inv).astype(F), (b * inv).astype(F)


def update_command(state, ids=slice(None)):
    """UniformPose2dCommand._update_command: target in the yaw-aligned base frame (isaaclab, unpinned)"""
    c, s = yaw_cs(state[QW:QW + 4, ids].T)
    dx = state[TGT_X, ids] - state[PX, ids]
    dy = state[TGT_Y, ids] - state[PX + 1, ids]
    state[CMD_BX, ids] = c * dx + s * dy
    state[CMD_BY, ids] = -s * dx + c * dy


def reset_envs(p, state, episode_len, hf, ids, seed, step, env_offset=0):
    if len(ids) == 0:
        return
    gid = np.asarray(ids) + env_offset
    u = PH.uniform4(gid, step, S_RESET, seed)
    x, y = sym(u[0], p.reset_xy), sym(u[1], p.reset_xy)
    h, x0, y0, cell, outside = H.unpack(hf)
    zt, _, _ = H.sample(h, x0, y0, cell, x, y, outside=outside)
    state[PX, ids], state[PX + 1, ids] = x, y
    state[PX + 2, ids] = np.maximum(F(p.reset_z), zt + F(p.spawn_clearance))
    yaw = sym(u[2], p.reset_yaw)
    state[QW, ids], state[QW + 1, ids], state[QW + 2, ids], state[QW + 3, ids] = np.cos(yaw * F(.5)), 0, 0, np.sin(yaw * F(.5))
    state[VX:VX + 6, ids] = 0
    lo, hi = F(p.reset_vel[0]), F(p.reset_vel[1])
    c = PH.uniform4(gid, step, S_CMD_RESET, seed)
    state[VX, ids] = lo + u[3] * (hi - lo)
    state[VX + 1, ids] = lo + c[3] * (hi - lo)
    state[ACT0:ACT0 + 2, ids] = 0
    state[EPSUM0:EPSUM0 + 8, ids] = 0
    episode_len[ids] = 0
    state[TGT_X, ids], state[TGT_Y, ids] = sym(c[0], p.cmd_xy), sym(c[1], p.cmd_xy)
    state[TGT_H, ids] = sym(c[2], p.cmd_heading)
    state[CMD_TIMER, ids] = F(p.cmd_resample_s)


def height_map(p, state, hf):
    """E1: 26 x 26 yaw-aligned grid of terrain heights relative to the base plane, clipped (x fastest).  Sampled WITHOUT the contact
    samplers' far-border guard, as wl_elev_scan_dev.h::scan_cell does; a ray off the grid misses (+inf, clipped), whatever outside_z is"""
    n = state.shape[1]
    k = np.arange(N_RAYS, dtype=np.float32)
    g = (F(-0.5 * p.scan_size) + k * F(p.scan_res)).astype(F)
    lx = np.tile(g, N_RAYS)
    ly = np.repeat(g, N_RAYS)
    c, s = yaw_cs(state[QW:QW + 4].T)
    wx = state[PX][:, None] + c[:, None] * lx[None] - s[:, None] * ly[None]
    wy = state[PX + 1][:, None] + s[:, None] * lx[None] + c[:, None] * ly[None]
    z, _, inside = H.sample(*H.unpack(hf)[:4], wx.reshape(-1), wy.reshape(-1), guard=False)
    z, inside = z.reshape(n, -1), inside.reshape(n, -1)
    rz = state[PX + 2]
    val = E.world_height_map(rz, z, rz, p.scan_offset, p.elev_z0)
    val = np.where(inside, val, F(np.inf))
    return np.clip(val, -F(p.obs_clip), F(p.obs_clip)).astype(F)


def observe(p, state, hf):
    q = state[QW:QW + 4].T
    v_b, w_b = ES.body_velocities(state)
    goal = E.goal_relative_xyz(state[PX:PX + 3].T, state[CMD_BX:CMD_BX + 2].T)
    c = F(p.obs_clip)
    return np.concatenate([goal, np.stack(euler_xyz_from_quat(q), -1), np.clip(v_b, -c, c), np.clip(w_b, -c, c),
                           np.clip(state[ACT0:ACT0 + 2].T, F(-1), F(1)), height_map(p, state, hf)], -1).astype(F)


def step(p, state, episode_len, hf, actions, seed, step_count, metrics=None, env_offset=0, probe=None):
    n = state.shape[1]
    steer_t, wheel_t = ES.fwd_targets(p, ES.apply_action(p, state, actions))
    b = ES.integrate(p, state, steer_t, wheel_t, ground_fn(hf, probe), probe)
    truncated, finite = ES.count_step(p, state, episode_len)
    pos, v_b = b.pos, b.v_b
    cmd = state[CMD_BX:CMD_BX + 2].T                     # command as left by the PREVIOUS step's command update
    t_low = E.root_height_below_minimum(pos, p.min_height)
    t_stuck = np.logical_and(np.minimum(v_b[:, 0], F(p.stuck_vel_cap)) < F(p.stuck_min_vel),
                             b.wheel.sum(-1) > F(p.stuck_wheel_spin))
    t_roll = b.R[:, 2, 2] <= F(p.upright_cos)   # the fp32 tie at cos 60 deg is rolled over (elev_mdp.upright_penalty)
    t_goal = E.close_to_goal(pos, cmd, p.goal_dist)
    flags = (t_low, t_stuck, t_roll, t_goal)
    terminated = t_low | t_stuck | t_roll | t_goal | ~finite
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.stack([E.goal_progress_rate(pos, b.v, cmd), E.higher_elevation(pos, v_b),
                          E.is_falling_penalty(v_b, p.fall_vel).astype(F),
                          (t_stuck & ~truncated).astype(F)]).astype(F)
    terms, reward = ES.book_rewards(p, state, terms, finite)
    # M_TERM0..3: each flag over ALL envs, whatever else ended the episode
    ids = ES.end_episodes(state, episode_len, metrics, terminated | truncated, truncated, finite, [t.sum() for t in flags])
    reset_envs(p, state, episode_len, hf, ids, seed, step_count, env_offset)
    # command manager: count down, resample expired targets, re-express every target in the base frame
    state[CMD_TIMER] -= F(p.sim_dt) * F(p.decimation)
    exp = state[CMD_TIMER] <= 0
    if exp.any():
        u = PH.uniform4(np.arange(n) + env_offset, step_count, S_CMD_RESAMPLE, seed)
        state[TGT_X] = np.where(exp, sym(u[0], p.cmd_xy), state[TGT_X])
        state[TGT_Y] = np.where(exp, sym(u[1], p.cmd_xy), state[TGT_Y])
        state[TGT_H] = np.where(exp, sym(u[2], p.cmd_heading), state[TGT_H])
        state[CMD_TIMER] = np.where(exp, F(p.cmd_resample_s), state[CMD_TIMER])
    update_command(state)
    obs = observe(p, state, hf)
    return obs, reward, terminated, truncated, dict(terms=terms, terms_flags=flags, finite=finite)


def init_state(p, n, seed=0, stride=None, env_offset=0):
    """startup events (:387-407): wheel friction (2.0, 1.0) fixed, base mass += U(0.2, 0.5); throttle damping 1000
    (hound.py:19, not randomised in this task).  Keyed by the global env id (oracle/startup.py)."""
    from . import startup
    stride = stride or ((n + 63) // 64) * 64
    s = np.zeros((S_COUNT, stride), F)
    s[QW] = 1
    s[MU_S, :n], s[MU_D, :n], s[DAMP, :n], s[MASS, :n], _ = startup.draw(n, seed, env_offset, **startup.ELEV)
    return s

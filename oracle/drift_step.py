"""Fused drift env.step() -- numpy restatement of what ONE launch of `wl_drift_step` does, in the order of
IsaacLab's ManagerBasedRLEnv.step() with the reference's plugins.  Operates on the same
SoA state matrix as the kernel (rows = include/wheeledlab_amd.h WlStateField)."""
import numpy as np

from . import drift_mdp as M
from . import env_step as ES
from . import philox as PH
from . import vehicle as V
from .layout import ACT0, DAMP, DRIFT_ROWS, EPSUM0, MASS, MU_D, MU_S, PX, QW, TIMER_HF, TIMER_LF, VX, WX
from .layout import (STEER_POS, STEER_VEL, WHEEL, M_COUNT, M_EPLEN, M_EPSUM0, M_NONFINITE, M_RESETS,  # noqa: F401 -- re-exported
                     M_TERM0, M_TIMEOUTS)
from .mathlib import F


def targets(p, a_raw):
    proc = M.process_actions(a_raw, p.action)
    if p.action.map == 0:
        steer, wr = M.rwd_targets(proc[:, 0], proc[:, 1], p.action)
        wheel = np.concatenate([wr, np.zeros_like(wr)], -1)
    else:
        steer, wheel = M.fwd_targets(proc[:, 0], proc[:, 1], p.action)
        if p.action.map == 2:   # base-class AckermannAction: the joints take angles; the single-track model steers by their
            steer = np.stack([proc[:, 1], proc[:, 1]], -1)   # centre-line equivalent atan(L / R) = delta
    return steer[:, 0].astype(F), wheel.astype(F)


def reset_envs(p, state, episode_len, ref_table, ids, seed, step, env_offset=0):
    """in-kernel reset (drifting/mdp/events.py:119-133 + manager resets); ids = env indices to reset"""
    if len(ids) == 0:
        return
    gid = np.asarray(ids) + env_offset
    u = PH.uniform8(gid, step, PH.S_DRIFT_EVENTS, seed)    # [0..3] index, x, y, yaw | [4..5] timers | [6..7] the lf push's (step)
    n_ref = p.num_ref_points
    idx = np.minimum((u[0] * F(n_ref)).astype(np.int32), n_ref - 1)
    state[PX + 0, ids] = ref_table[0, idx] + (F(2) * u[1] - F(1)) * F(p.pos_noise)
    state[PX + 1, ids] = ref_table[1, idx] + (F(2) * u[2] - F(1)) * F(p.pos_noise)
    state[PX + 2, ids] = 0
    yaw = ref_table[2, idx] + (F(2) * u[3] - F(1)) * F(p.yaw_noise)
    state[QW, ids] = np.cos(yaw * F(0.5))
    state[QW + 1, ids] = 0
    state[QW + 2, ids] = 0
    state[QW + 3, ids] = np.sin(yaw * F(0.5))
    state[VX:VX + 6, ids] = 0
    state[ACT0:ACT0 + 2, ids] = 0
    state[EPSUM0:EPSUM0 + 8, ids] = 0
    episode_len[ids] = 0
    state[TIMER_HF, ids] = F(p.hf_interval[0]) + u[4] * (F(p.hf_interval[1]) - F(p.hf_interval[0]))
    state[TIMER_LF, ids] = F(p.lf_interval[0]) + u[5] * (F(p.lf_interval[1]) - F(p.lf_interval[0]))


def observe(p, state, normals):
    v_b, w_b = ES.body_velocities(state)
    return M.blind_obs(p, state[PX:PX + 3].T, state[QW:QW + 4].T, v_b, w_b, state[ACT0:ACT0 + 2].T, normals)


def step(p, state, episode_len, ref_table, actions, seed, step_count, metrics=None, noise=None, env_offset=0,
         ground=V.flat_ground):
    """state [DRIFT_ROWS, n] float32 and episode_len [n] int32 are updated IN PLACE.
    -> obs [n,14], reward [n], terminated [n] bool, truncated [n] bool, info dict"""
    n = state.shape[1]
    steer_t, wheel_t = targets(p, ES.apply_action(p, state, actions))
    b = ES.integrate(p, state, steer_t, wheel_t, ground)
    truncated, finite = ES.count_step(p, state, episode_len)
    terminated = np.logical_or(M.cart_off_track(b.pos, p.straight, p.r_in, p.r_out), ~finite)

    terms = M.drift_terms(p, b.pos, b.v_b, b.wb, b.ww, np.stack([b.th, b.th], -1), terminated, truncated)
    terms, reward = ES.book_rewards(p, state, terms, finite)

    done = np.logical_or(terminated, truncated)
    # M_TERM0: every terminated car, the non-finite ones included
    ids = ES.end_episodes(state, episode_len, metrics, done, truncated, finite, [terminated.sum()])
    reset_envs(p, state, episode_len, ref_table, ids, seed, step_count, env_offset)

    step_dt = F(p.sim_dt) * F(p.decimation)
    if p.enable_pushes:
        gid = np.arange(n) + env_offset
        state[TIMER_HF] -= step_dt
        fire = state[TIMER_HF] < F(1e-6)
        u = PH.uniform8(gid, step_count, PH.S_NOISE1, seed)[4:]       # words z, w of the block whose x, y are normals 8..11
        state[VX] += np.where(fire, ES.sym(u[0], p.hf_vel_x), F(0))
        state[VX + 1] += np.where(fire, ES.sym(u[1], p.hf_vel_y), F(0))
        state[WX + 2] += np.where(fire, ES.sym(u[2], p.hf_vel_yaw), F(0))
        state[TIMER_HF] = np.where(fire, F(p.hf_interval[0]) + u[3] * (F(p.hf_interval[1]) - F(p.hf_interval[0])),
                                   state[TIMER_HF])
        state[TIMER_LF] -= step_dt
        fire = state[TIMER_LF] < F(1e-6)
        u = PH.uniform8(gid, step_count, PH.S_DRIFT_EVENTS, seed)[6:]  # word w of the event block
        state[WX + 2] += np.where(fire, ES.sym(u[0], p.lf_vel_yaw), F(0))
        state[TIMER_LF] = np.where(fire, F(p.lf_interval[0]) + u[1] * (F(p.lf_interval[1]) - F(p.lf_interval[0])),
                                   state[TIMER_LF])

    normals = None
    if p.enable_corruption:
        normals = noise if noise is not None else PH.normal12(np.arange(n) + env_offset, step_count, seed)
    obs = observe(p, state, normals)
    return obs, reward, terminated, truncated, dict(terms=terms, done=done, finite=finite)


def init_state(p, n, seed=0, stride=None, env_offset=0):
    """startup events (mushr_drift_env_cfg.py:98-119,145-154): wheel friction U(0.3,0.5) in 20 buckets with
    mu_d <= mu_s, rear throttle damping U(10,50), base mass += U(0.3,0.5) -> fresh state matrix.  Keyed by the global
    env id (oracle/startup.py), like the product's wl_startup_randomize."""
    from . import startup
    stride = stride or ((n + 63) // 64) * 64
    s = np.zeros((DRIFT_ROWS, stride), F)
    s[QW] = 1
    s[MU_S, :n], s[MU_D, :n], s[DAMP, :n], s[MASS, :n], _ = startup.draw(n, seed, env_offset, **startup.DRIFT)
    return s

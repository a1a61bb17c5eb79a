"""The env.step() skeleton the drift, elevation and visual oracles share -- plain functions each task's `step` calls in its own
order, as the device's task kernels call csrc/wl_implicit_task.h: action row, vehicle integration, step counter, reward booking,
episode ends.  What a task's `step` spells out itself is what is specific to that task.  Rows: oracle/layout.py."""
import numpy as np

from . import drift_mdp as M
from . import vehicle as V
from .layout import (ACT0, DAMP, EPSUM0, MASS, MU_D, MU_S, PX, QW, STEER_POS, STEER_VEL, VX, WHEEL, WX, M_EPLEN, M_EPSUM0,
                     M_NONFINITE, M_RESETS, M_TERM0, M_TIMEOUTS)
from .mathlib import F, f32, matrix_from_quat
from .params import NS


def sym(u, a):
    """uniform [0, 1) -> uniform [-a, a)"""
    return (F(2) * u - F(1)) * F(a)


def to_body(R, w):
    """world-frame vectors [n, 3] in the body frames R [n, 3, 3]: R^T w"""
    return np.einsum("nji,nj->ni", R, w).astype(F)


def body_velocities(state):
    """-> base_lin_vel, base_ang_vel [n, 3] of the rows as they stand"""
    R = matrix_from_quat(state[QW:QW + 4].T)
    return to_body(R, state[VX:VX + 3].T), to_body(R, state[WX:WX + 3].T)


def apply_action(p, state, actions):
    """ClipAction wrapper; the raw action is the last_action row of the next observation.  -> raw action [n, 2]"""
    a_raw = M.clip_action(actions) if p.action.clip_wrapper else f32(actions)
    state[ACT0:ACT0 + 2] = a_raw.T
    return a_raw


def fwd_targets(p, a_raw):
    """the 4WD action term (elevation, visual) -> steering target [n], wheel velocity targets [n, 4]"""
    proc = M.process_actions(a_raw, p.action)
    steer2, wheel_t = M.fwd_targets(proc[:, 0], proc[:, 1], p.action)
    return steer2[:, 0], wheel_t


def integrate(p, state, steer_t, wheel_t, ground=V.flat_ground, probe=None):
    """decimation x substeps vehicle sub-steps on the rows, IN PLACE: root pose -> centre of mass, world -> body angular velocity, the
    loop, and back.  -> R, pos (root), v (world), v_b, wb (body), ww (world), wheel [n, 4], th (steering angle) after the step"""
    vp = p.vehicle
    q = state[QW:QW + 4].T.copy()
    R = matrix_from_quat(q)
    c = f32([0, 0, vp.cg_z])
    x = (state[PX:PX + 3].T + R @ c).astype(F)
    v = state[VX:VX + 3].T.copy()
    wb = to_body(R, state[WX:WX + 3].T)
    wheel = state[WHEEL:WHEEL + 4].T.copy()
    th, om = state[STEER_POS].copy(), state[STEER_VEL].copy()
    h = F(p.sim_dt) / F(vp.substeps)
    for _ in range(p.decimation * vp.substeps):
        x, q, v, wb, wheel, th, om = V.substep(x, q, v, wb, wheel, th, om, steer_t, wheel_t, state[MASS], state[MU_S], state[MU_D],
                                               state[DAMP], vp, h, ground, probe)
    R = matrix_from_quat(q)
    ww = np.einsum("nij,nj->ni", R, wb).astype(F)
    pos = (x - R @ c).astype(F)
    state[PX:PX + 3], state[QW:QW + 4], state[VX:VX + 3], state[WX:WX + 3] = pos.T, q.T, v.T, ww.T
    state[WHEEL:WHEEL + 4] = wheel.T
    state[STEER_POS], state[STEER_VEL] = th, om
    return NS(R=R, pos=pos, v=v, v_b=to_body(R, v), wb=wb, ww=ww, wheel=wheel, th=th)


def count_step(p, state, episode_len):
    """episode_len += 1 IN PLACE -> truncated (time_out), finite (no inf / nan in a car's integrated rows) [n] bool"""
    episode_len += 1
    return M.time_out(episode_len, p.max_episode_length), np.isfinite(state[:ACT0]).all(0)


def book_rewards(p, state, terms, finite):
    """terms [k, n] zeroed for non-finite cars, RewardManager.compute, episode sums (log_episode_sums) -> terms, reward [n].
    Every term's contribution is added to its episode-sum row, a zero weight's included: it is +0.0 and leaves the row's bits as
    they are (a row starts at +0.0 and cannot become -0.0), the same values as adding the non-zero weights' rows alone."""
    terms = np.where(finite[None], terms, F(0)).astype(F)
    reward, contrib = M.reward_sum(p, terms)
    if p.log_episode_sums:
        state[EPSUM0:EPSUM0 + len(terms)] += contrib
    return terms, reward


def end_episodes(state, episode_len, metrics, done, truncated, finite, term_counts):
    """metric block of the episodes that end with this step, then the non-finite cars' rows scrubbed so that the task's reset starts
    from clean ones.  term_counts: what the TASK adds to M_TERM0.. (which of its flags, over which envs, is its own rule).
    -> ids of the envs to reset"""
    ids = np.nonzero(done)[0]
    if metrics is not None and len(ids):
        metrics[M_EPSUM0:M_EPSUM0 + 8] += state[EPSUM0:EPSUM0 + 8, ids].astype(np.float64).sum(1)
        metrics[M_RESETS] += len(ids)
        metrics[M_TIMEOUTS] += truncated.sum()
        for k, c in enumerate(term_counts):
            metrics[M_TERM0 + k] += c
        metrics[M_NONFINITE] += (~finite).sum()
        metrics[M_EPLEN] += episode_len[ids].sum()
    if (~finite).any():
        bad = np.nonzero(~finite)[0]
        state[:ACT0, bad] = 0
        state[QW, bad] = 1
    return ids

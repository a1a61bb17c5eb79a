"""The terrain curriculum's step in numpy fp32: oracle.elev_step.step's body with per-env terrain levels -- the executable form of
the rule in include/wheeledlab_amd.h (WlTerrainLevels) and DESIGN.md.  Composed from the oracle's own pieces (env_step, elev_mdp,
philox, heightfield.sample); what is new here is `next_levels`, `reset_envs` (spawn and goal about the tile's centre) and the goal
resample about it.  `levels` = dict(level int32 [n] (updated IN PLACE), type int32 [n], origins float32 [rows * cols, 2], rows,
cols) or None (off: exactly oracle.elev_step.step)."""
import numpy as np

from oracle import elev_mdp as E
from oracle import elev_step as OE
from oracle import env_step as ES
from oracle import heightfield as H
from oracle import philox as PH
from oracle.env_step import sym
from oracle.layout import ACT0, CMD_BX, CMD_TIMER, EPSUM0, PX, QW, TGT_H, TGT_X, TGT_Y, VX
from oracle.mathlib import F

S_LEVEL = 3     # csrc/wl_elev_env.h ES_LEVEL


def uniform_below(word, n):
    return ((np.asarray(word, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def next_levels(levels, ids, at_goal, failed, seed, step, env_offset=0):
    """the level every ending episode moves to: up at the goal, else down (not below 0) after a failure, else unchanged; a level
    that reaches `rows` becomes a uniform one from word 0 of Philox(gid, step, S_LEVEL, seed)"""
    rows = int(levels["rows"])
    lv = np.clip(levels["level"][ids], 0, rows - 1).astype(np.int64)
    up = at_goal[ids]
    down = failed[ids] & ~up
    lv = np.where(up, lv + 1, np.where(down, np.maximum(lv - 1, 0), lv))
    word = PH.philox4x32(np.asarray(ids) + env_offset, step, S_LEVEL, seed)[0]
    return np.where(lv >= rows, uniform_below(word, rows), lv).astype(np.int32)


def origins_of(levels, ids):
    rows, cols = int(levels["rows"]), int(levels["cols"])
    t = np.clip(levels["level"][ids], 0, rows - 1).astype(np.int64) * cols + np.clip(levels["type"][ids], 0, cols - 1)
    return levels["origins"][t].astype(F)


def reset_envs(p, state, episode_len, hf, ids, seed, step, levels, env_offset=0):
    """oracle.elev_step.reset_envs with the spawn square and the goal square about the env's tile centre (levels as they stand)"""
    if len(ids) == 0:
        return
    gid = np.asarray(ids) + env_offset
    o = origins_of(levels, ids)
    u = PH.uniform4(gid, step, OE.S_RESET, seed)
    x, y = (o[:, 0] + sym(u[0], p.reset_xy)).astype(F), (o[:, 1] + sym(u[1], p.reset_xy)).astype(F)
    h, x0, y0, cell, outside = H.unpack(hf)
    zt, _, _ = H.sample(h, x0, y0, cell, x, y, outside=outside)
    state[PX, ids], state[PX + 1, ids] = x, y
    state[PX + 2, ids] = np.maximum(F(p.reset_z), zt + F(p.spawn_clearance))
    yaw = sym(u[2], p.reset_yaw)
    state[QW, ids], state[QW + 1, ids], state[QW + 2, ids], state[QW + 3, ids] = np.cos(yaw * F(.5)), 0, 0, np.sin(yaw * F(.5))
    state[VX:VX + 6, ids] = 0
    lo, hi = F(p.reset_vel[0]), F(p.reset_vel[1])
    c = PH.uniform4(gid, step, OE.S_CMD_RESET, seed)
    state[VX, ids] = lo + u[3] * (hi - lo)
    state[VX + 1, ids] = lo + c[3] * (hi - lo)
    state[ACT0:ACT0 + 2, ids] = 0
    state[EPSUM0:EPSUM0 + 8, ids] = 0
    episode_len[ids] = 0
    state[TGT_X, ids], state[TGT_Y, ids] = (o[:, 0] + sym(c[0], p.cmd_xy)).astype(F), (o[:, 1] + sym(c[1], p.cmd_xy)).astype(F)
    state[TGT_H, ids] = sym(c[2], p.cmd_heading)
    state[CMD_TIMER, ids] = F(p.cmd_resample_s)


def ground_fn(hf, probe=None):
    """oracle.elev_step.ground_fn for cars that may be non-finite: their wheels sample the terrain at (0, 0) instead of at NaN (the
    oracle's sampler indexes with the coordinate; such a car stays non-finite through its other rows and is scrubbed and reset)"""
    g = OE.ground_fn(hf, probe)
    return lambda xy: g(np.where(np.isfinite(xy), xy, F(0)).astype(F))


def step(p, state, episode_len, hf, actions, seed, step_count, levels=None, metrics=None, env_offset=0, probe=None):
    """one env.step(); state, episode_len and levels["level"] are updated in place -> obs, reward, terminated, truncated, info"""
    if levels is None:
        return OE.step(p, state, episode_len, hf, actions, seed, step_count, metrics, env_offset, probe)
    n = state.shape[1]
    steer_t, wheel_t = ES.fwd_targets(p, ES.apply_action(p, state, actions))
    b = ES.integrate(p, state, steer_t, wheel_t, ground_fn(hf, probe), probe)
    truncated, finite = ES.count_step(p, state, episode_len)
    pos, v_b = b.pos, b.v_b
    cmd = state[CMD_BX:CMD_BX + 2].T
    t_low = E.root_height_below_minimum(pos, p.min_height)
    t_stuck = np.logical_and(np.minimum(v_b[:, 0], F(p.stuck_vel_cap)) < F(p.stuck_min_vel), b.wheel.sum(-1) > F(p.stuck_wheel_spin))
    t_roll = b.R[:, 2, 2] <= F(p.upright_cos)
    t_goal = E.close_to_goal(pos, cmd, p.goal_dist)
    flags = (t_low, t_stuck, t_roll, t_goal)
    terminated = t_low | t_stuck | t_roll | t_goal | ~finite
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.stack([E.goal_progress_rate(pos, b.v, cmd), E.higher_elevation(pos, v_b), E.is_falling_penalty(v_b, p.fall_vel).astype(F),
                          (t_stuck & ~truncated).astype(F)]).astype(F)
    terms, reward = ES.book_rewards(p, state, terms, finite)
    ids = ES.end_episodes(state, episode_len, metrics, terminated | truncated, truncated, finite, [t.sum() for t in flags])
    # the curriculum BEFORE the reset events (IsaacLab _reset_idx), from the outcome the step has just computed
    if len(ids):
        levels["level"][ids] = next_levels(levels, ids, np.asarray(t_goal), t_low | t_stuck | t_roll | ~finite, seed, step_count, env_offset)
    reset_envs(p, state, episode_len, hf, ids, seed, step_count, levels, env_offset)
    state[CMD_TIMER] -= F(p.sim_dt) * F(p.decimation)
    exp = state[CMD_TIMER] <= 0
    if exp.any():
        u = PH.uniform4(np.arange(n) + env_offset, step_count, OE.S_CMD_RESAMPLE, seed)
        o = origins_of(levels, np.arange(n))
        state[TGT_X] = np.where(exp, (o[:, 0] + sym(u[0], p.cmd_xy)).astype(F), state[TGT_X])
        state[TGT_Y] = np.where(exp, (o[:, 1] + sym(u[1], p.cmd_xy)).astype(F), state[TGT_Y])
        state[TGT_H] = np.where(exp, sym(u[2], p.cmd_heading), state[TGT_H])
        state[CMD_TIMER] = np.where(exp, F(p.cmd_resample_s), state[CMD_TIMER])
    OE.update_command(state)
    obs = OE.observe(p, state, hf)
    return obs, reward, terminated, truncated, dict(terms=terms, terms_flags=flags, finite=finite)

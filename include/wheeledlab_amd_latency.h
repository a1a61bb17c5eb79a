/* wheeledlab_amd_latency.h -- action latency: every env applies the policy's action a per-env, per-episode number of control steps late.
 * Two small launches around the step launch: `push` before it (the policy's action into the env's ring, the delayed action out), and
 * `finish` after it (the policy's own action back into the state's last-action rows and the observation's last_action columns; the lag of
 * the envs the step reset drawn again).  The step kernels are untouched: they take `applied` as their action and never learn of the lag.
 *
 * This is a restatement of IsaacLab's isaaclab.utils.buffers.DelayBuffer (over CircularBuffer) as DelayedPDActuator uses it, from its
 * documented behaviour; IsaacLab is not vendored with the reference, so the restatement is UNPINNED: no golden of theirs holds it.
 * ONE DELIBERATE DIFFERENCE: the lag counts CONTROL steps (env.step() calls), not physics steps -- the fused steps take one action per
 * env step, and a physics-step lag that is no multiple of `decimation` would change the target in mid-step.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h).  Same conventions as that header: device pointers, `stream` a
 * hipStream_t (NULL = the default stream), asynchronous on that stream, the caller owns every buffer, return 0 (WL_OK) or a negative
 * WL_E* code, arguments validated before any launch.
 *
 * THE LAYER BLOCK.  uint32 words, component-major like the state and with the state's stride: row r of env e is block[r * stride + e].
 *     0, 1   lag[c]    the lag of action component c, in [min_delay, max_delay]
 *     2      pushes    actions pushed since the env's last reset, saturating at max_delay + 1
 *     3      head      the ring slot of the latest push
 *     4      drawn     how often the env's lags have been drawn
 *     5 + 2 s + c      ring slot s (0 .. max_delay), component c: the action words as the policy gave them
 * wl_action_latency_width(max_delay) = 5 + 2 (max_delay + 1) rows.  The caller zeroes the block; a `finish` with every flag set
 * (env.reset(): no step, every env resets) draws every env's first lags.
 *
 * PUSH, per env e (before the step).  action and applied are [n][2] rows of 32-bit words.
 *     if pushes == 0:  every ring slot = action[e] (CircularBuffer.append after a reset), head = 0, pushes = 1
 *     else:            head = (head + 1) mod (max_delay + 1), ring[head] = action[e], pushes = min(pushes + 1, max_delay + 1)
 *     applied[e][c] = ring[(head - min(lag[c], pushes - 1)) mod (max_delay + 1)][c]
 * Words are moved, never computed with: NaN payloads, -0.0, infinities and denormals arrive in `applied` as they left the policy, and
 * `action` itself is only read.  A lag word above max_delay (a block the caller did not get from `finish`) is read as max_delay.
 *
 * FINISH, per env e (after the step), with reset = reset_a[e] | reset_b[e] as the step returned them:
 *     reset:      pushes = 0; both lags drawn again (below), ++drawn.  WL_S_ACT0/1 and the last_action columns keep the step's zeros
 *                 (IsaacLab's ActionManager.reset).
 *     otherwise:  s_c = clip_wrapper ? clamp(action[e][c], -1, 1) : action[e][c];  WL_S_ACT0 + c = s_c;
 *                 row[e * row_pitch + last_action_col + c] = clamp(s_c, -1, 1)   (skipped when last_action_col == -1)
 *                 -- what the step would have stored had it been handed action[e] with zero latency: its ClipAction folding, its (-1, 1)
 *                 clip of the observation column, by the same instruction (the median of three, which maps a quiet NaN to -1).  This is
 *                 IsaacLab's last_action: the action manager's `action`, the policy's, not the actuator's delayed target.
 *
 * THE LAG DRAW.  Stateless Philox4x32 (csrc/wl_rng.h, 7 rounds), key = (seed low, seed high), counter
 * (uint32(env_offset + e), drawn, 0, WL_AL_STREAM), words w0 .. w3.  span = max_delay - min_delay + 1,
 *     lag[c] = min_delay + min(int(u01(w_c) * span), span - 1),  u01(w) = (w >> 8) * 2^-24, the product in fp32;
 * with per_component == 0 both components take w0.  Stream id 20 (WL_RS_ACT_LAG of wl_rng.h) is no other draw's.  Nothing depends on n,
 * the launch geometry, the sharding or the step a reset falls on.
 *
 * One lane per env, no atomics; each launch stores only what the lists above name. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_ACTLAT_VERSION 1
#define WL_ACTLAT_MAX_DELAY 16      /* control steps; a larger max_delay is refused */
#define WL_ACTLAT_HEAD_ROWS 5       /* lag0, lag1, pushes, head, drawn */
#define WL_AL_STREAM 20

/* Host only.  The rows (words per env) of the layer block, 5 + 2 (max_delay + 1), or WL_EINVAL: max_delay outside
 * [0, WL_ACTLAT_MAX_DELAY]. */
int64_t wl_action_latency_width(int32_t max_delay);

/* One launch over envs 0 .. n - 1: action and applied float [n][2], block [width][stride] (above).
 * WL_EINVAL: NULL action / applied / block, n < 1, stride < n, max_delay outside [0, WL_ACTLAT_MAX_DELAY], or any two of applied, action
 * and the block overlapping (applied may not alias the policy's action); WL_EALIGN: a stride that is no multiple of 64, or action,
 * applied or block not 4-byte aligned. */
int wl_action_latency_push(int32_t n, const float* action, float* applied, float* block, int64_t stride, int32_t max_delay, void* stream);

/* One launch over envs 0 .. n - 1: action float [n][2] (the policy's, as `push` took it), state float [WL_S_COUNT][stride], row the
 * observation rows [n][row_pitch] (may be NULL when last_action_col == -1), reset_a / reset_b byte flags [n]; reset_b may be NULL.
 * WL_EINVAL: NULL action / state / block / reset_a, row NULL with a column, n < 1, stride < n, stride * 4 * WL_S_COUNT beyond 2^31 - 1,
 * min_delay < 0, min_delay > max_delay, max_delay above WL_ACTLAT_MAX_DELAY, per_component or clip_wrapper outside {0, 1}, row_pitch < 1
 * or last_action_col outside [-1, row_pitch - 2], or any two of the two action rows of the state, the row, the block, the action and the
 * flag arrays overlapping; WL_EALIGN: a stride that is no multiple of 64, or action, state, row or block not 4-byte aligned. */
int wl_action_latency_finish(int32_t n, const float* action, float* state, int64_t stride, float* row, int64_t row_pitch,
                             int32_t last_action_col, float* block, const uint8_t* reset_a, const uint8_t* reset_b, int32_t min_delay,
                             int32_t max_delay, int32_t per_component, int32_t clip_wrapper, uint64_t seed, uint64_t env_offset, void* stream);

/* WL_ACTLAT_VERSION of the library */
int wl_action_latency_version(void);

#ifdef __cplusplus
}
#endif

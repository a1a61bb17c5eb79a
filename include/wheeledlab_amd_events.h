/* wheeledlab_amd_events.h -- per-episode domain randomisation: IsaacLab's randomize_rigid_body_material, randomize_actuator_gains and
 * randomize_rigid_body_mass as EventTerms of mode "reset" and "interval", applied to the per-env constant rows of the state matrix
 * (WL_S_MU_S, WL_S_MU_D, WL_S_DAMP, WL_S_MASS) in one launch per env step.  The step kernels only read those rows; this launch runs
 * between two of them: after the step launch (whose in-kernel reset has already happened, and whose flags say which envs it reset) and
 * before the next one.
 *
 * This is a restatement of IsaacLab's EventManager (apply(mode="reset" | "interval"), reset()) and mdp.events from their documented
 * behaviour; neither is vendored with the reference, so the restatement is UNPINNED: no golden of theirs holds it.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h).  Same conventions as that header: device pointers, `stream` a
 * hipStream_t (NULL = the default stream), asynchronous on that stream, the caller owns every buffer, return 0 (WL_OK) or a negative
 * WL_E* code, arguments validated before any launch.
 *
 * THE LAYER BLOCK.  uint32 / float words, component-major like the state and with the state's stride: row r of env e is
 * block[r * stride + e].  Rows 0, 1: part_base, part_wheels (float): the two parts of the mass row.  Then four rows per term k:
 *     2 + 4 k  time_left (float)   interval terms: the time to the next application
 *     3 + 4 k  applied  (uint32)   how often the term has been applied to the env
 *     4 + 4 k, 5 + 4 k  (uint32)   reset terms: the step of the last application, low and high word;
 *                                  interval terms: `drawn`, how often the env's timer has been drawn (low word; the high word stays 0)
 * wl_event_rand_width() = 2 + 4 n_terms rows.  The caller zeroes the block, fills the part rows when a mass term is in the table
 * (so that part_base + part_wheels is the mass row); a call without flags and with step_dt = 0 gives every interval term its first
 * time_left.
 *
 * PER CALL AND ENV e, with reset = reset_a[e] | reset_b[e] and forced_k = mask[e] and bit k of mask_terms:
 *   1. the reset terms, in table order.  Term k is applied when forced_k, or when reset and one of: min_step_count_between_reset == 0,
 *      applied == 0 (never applied), step - last_step >= min_step_count_between_reset.  It then stores last_step = step.
 *   2. the interval terms, in table order.  id = uint32(env_offset + e), with is_global_time == 1: 0xffffffff.
 *          if drawn == 0 (the timer was never drawn), or reset and is_global_time == 0 (the env's new episode; not an application):
 *              time_left = T(id, drawn), ++drawn
 *          time_left -= step_dt;  if time_left < 1e-6: apply, time_left = T(id, drawn), ++drawn
 *      With global time every lane keeps its own copy of the one timer and computes the same value; resets do not touch it.
 *      forced_k applies the term as well and leaves its timer alone.  (A call outside a step passes step_dt = 0.)
 *      T(id, c) = fmaf(u01(x), fp32(interval_hi - interval_lo), interval_lo), x the first word of the Philox block with counter
 *      (id, c, 0, WL_ER_STREAM_TIMER | k << 8).
 *   This is the order of IsaacLab's step(): _reset_idx (reset events, then EventManager.reset) and then the interval events.  Where two
 *   terms hit one target in one call the later one wins.
 *   An application of term k to env e draws from the block with counter (uint32(env_offset + e), applied, 0, WL_ER_STREAM_VALUE | k << 8)
 *   (words w0 .. w3), and then ++applied.  Stateless Philox4x32 (csrc/wl_rng.h, 7 rounds), key = (seed low, seed high).  Stream ids 18 and
 *   19 (WL_RS_EVENT_VALUE / WL_RS_EVENT_TIMER of wl_rng.h) are no other draw's.  Nothing depends on n, the launch geometry, the sharding or
 *   the step an application falls on.
 *       MU           bucket = min(int(u01(w0) * num_buckets), num_buckets - 1); (m0, m1) = u01 of the first two words of the block
 *                    (bucket, 0, 0, WL_RS_STARTUP_BUCKET): the materials of wl_startup_randomize, whichever mode picks from them.
 *                    mu_s = fmaf(m0, mu_s_hi - mu_s_lo, mu_s_lo), mu_d likewise; make_consistent: mu_d = min(mu_d, mu_s).
 *       DAMP         WL_S_DAMP = op(base, d(w0))
 *       MASS_BASE    part_base = op(base, d(w0))
 *       MASS_WHEELS  (abs only) part_wheels = (d(w0) + d(w1)) + (d(w2) + d(w3))
 *       op: add base + d | scale base * d | abs d.   After a mass part changed: WL_S_MASS = part_base + part_wheels.
 *       d(w): uniform      fmaf(u01(w), fp32(p1 - p0), p0)                                        p = (lo, hi)
 *             log_uniform  exp(fmaf(u01(w), b, a)), a = fp32(ln p0), b = fp32(ln p1 - ln p0), the logarithms in double on the host
 *             gaussian     fmaf(z, p1, p0), p = (mean, std), z the first normal of box_muller_open (wl_rng.h) on the two halves of w
 *   Every operation is rounded on its own; the only fused ones are the fmaf above.
 *   The launch stores only the four constant rows and the block; a lane with nothing to apply stores nothing but a changed time_left
 *   (and a redrawn timer's count).  One lane per env, no atomics. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_EVENTRAND_VERSION 1
#define WL_EVENTRAND_MAX_TERMS 8
#define WL_ER_STREAM_VALUE 18
#define WL_ER_STREAM_TIMER 19
#define WL_ER_GLOBAL_ID 0xffffffffu

enum WlEventTarget { WL_ER_MU = 0, WL_ER_DAMP = 1, WL_ER_MASS_BASE = 2, WL_ER_MASS_WHEELS = 3 };
enum WlEventMode { WL_ER_RESET = 0, WL_ER_INTERVAL = 1 };
enum WlEventOp { WL_ER_ADD = 0, WL_ER_SCALE = 1, WL_ER_ABS = 2 };
enum WlEventDist { WL_ER_UNIFORM = 0, WL_ER_LOG_UNIFORM = 1, WL_ER_GAUSSIAN = 2 };

typedef struct WlEventRandTerm {
    int32_t target;                        /* WlEventTarget */
    int32_t mode;                          /* WlEventMode */
    int32_t op;                            /* WlEventOp; MASS_WHEELS: WL_ER_ABS.  MU ignores op, dist, p0, p1 and base (they are still checked) */
    int32_t dist;                          /* WlEventDist */
    float p0, p1;                          /* uniform, log_uniform: (lo, hi), lo <= hi, log_uniform lo > 0; gaussian: (mean, std), std >= 0 */
    float base;                            /* the default value the operation applies to */
    float interval_lo, interval_hi;        /* interval terms: 0 < interval_lo <= interval_hi, seconds; reset terms: not read */
    int32_t is_global_time;                /* 0 | 1 */
    int32_t min_step_count_between_reset;  /* >= 0 */
    float mu_s_lo, mu_s_hi, mu_d_lo, mu_d_hi;   /* MU: the static and dynamic friction ranges */
    int32_t num_buckets;                   /* MU: >= 1 */
    int32_t make_consistent;               /* MU: 0 | 1 */
} WlEventRandTerm;

/* Host only.  The rows (floats per env) of the layer block, 2 + 4 n_terms, or WL_EINVAL: terms NULL, n_terms outside
 * [1, WL_EVENTRAND_MAX_TERMS], an enum out of range, p0 > p1 (uniform, log_uniform), log_uniform with p0 <= 0, a negative std, a
 * non-abs operation on MASS_WHEELS, an interval term with interval_lo > interval_hi or interval_lo <= 0, is_global_time or
 * make_consistent outside {0, 1}, a negative min_step_count_between_reset, MU with num_buckets < 1 or a friction range with lo > hi,
 * any parameter that is not finite. */
int64_t wl_event_rand_width(const WlEventRandTerm* terms, int32_t n_terms);

/* One launch over envs 0 .. n - 1: state float [WL_S_COUNT][stride], block [width][stride] (above), reset_a / reset_b / mask byte
 * flags [n]; reset_b and mask may be NULL.  `terms` is HOST memory: the table travels with the launch by value, so the call may be
 * captured into a graph.  mask_terms: bit k set = mask[e] forces term k.
 * WL_EINVAL: NULL state / block / reset_a / terms, n < 1, stride < n, stride * 4 * WL_S_COUNT beyond 2^31 - 1, a table
 * wl_event_rand_width refuses, mask_terms with a bit at or above n_terms, a step_dt that is negative or not finite, or any two of
 * the state's constant rows, the block and the flag arrays overlapping; WL_EALIGN: a stride that is not a multiple of 64, state or
 * block not 4-byte aligned. */
int wl_event_rand_apply(int32_t n, float* state, int64_t stride, const WlEventRandTerm* terms, int32_t n_terms, float* block,
                        const uint8_t* reset_a, const uint8_t* reset_b, const uint8_t* mask, uint32_t mask_terms, uint64_t seed,
                        uint64_t step, float step_dt, uint64_t env_offset, void* stream);

/* WL_EVENTRAND_VERSION of the library */
int wl_event_rand_version(void);

#ifdef __cplusplus
}
#endif

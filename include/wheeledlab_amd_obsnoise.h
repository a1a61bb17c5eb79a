/* wheeledlab_amd_obsnoise.h -- observation corruption: the noise models, clip and scale of IsaacLab's ObservationManager
 * (isaaclab.utils.noise: constant / uniform / Gaussian noise with operation add / scale / abs, and the per-episode additive bias of
 * NoiseModelWithAdditiveBiasCfg) applied to the clean observation row in one launch per env step.  In IsaacLab's order it comes first:
 * term -> noise -> clip -> scale -> history.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): it runs once per env step on the stepwise path, between the fused
 * step's observation and the history push / the policy step.  Same conventions as that header: device pointers, `stream` a hipStream_t
 * (NULL = the default stream), asynchronous on that stream, the caller owns every buffer, return 0 (WL_OK) or a negative WL_E* code,
 * arguments validated before any launch.
 *
 * THE DRAWS.  Stateless Philox4x32 (csrc/wl_rng.h philox_block, 7 rounds), key = (seed low, seed high), counter =
 *     (uint32(env_offset + e), step low, step high, stream | (c >> 2) << 8)
 * for column c of env e: columns 4 b .. 4 b + 3 of a row share block b and column c takes word c & 3 of it.  stream is
 * WL_OC_STREAM_NOISE (16) for the per-step noise and WL_OC_STREAM_BIAS (17) for the per-episode bias (WL_RS_OBS_NOISE / WL_RS_OBS_BIAS of
 * wl_rng.h) -- ids no other draw of the library uses (the steps' and the policy's 0 .. 10, the terrain's 11 .. 15).  Nothing depends on n, the launch geometry or the sharding.
 * From its word w a column draws
 *     constant:  d = a
 *     uniform :  d = fmaf(u01(w), b, a)            u01(w) = (w >> 8) 2^-24 in [0, 1);  a = n_min, b = fp32(n_max - n_min)
 *     Gaussian:  d = fmaf(z, b, a)                 a = mean, b = std;  z = r cos(2 pi u1), r = sqrt(-2 ln u0),
 *                                                  u0 = ((w & 0xffff) + 1/2) 2^-16, u1 = ((w >> 16) + 1/2) 2^-16   (|z| <= 4.86)
 * (box_muller_open of wl_rng.h on the two halves of the word; its first normal).
 *
 * PER ELEMENT, in this order, every operation rounded on its own (no contraction but the fmaf above):
 *   1. x = obs[e][c], or with state_row >= 0:  x = state[(state_row + j) * state_stride + e], j = c - off
 *   2. if enable: noise   y = x + d | x * d | d   (operation add | scale | abs; abs keeps a NaN x: the non-finite-env metric downstream
 *      must still see it), then with a bias model  y = y + bias[e][bias_off + j]
 *      (bias_per_component 0: bias[e][bias_off]).  With reset_a[e] | reset_b[e] set the bias element is first drawn afresh (the same
 *      d of the bias kind, from the bias stream, at column c -- per_component 0: at column off) and STORED.  enable == 0: nothing is
 *      drawn, nothing is stored.
 *   3. clip:  y = y < clip_lo ? clip_lo : y;  y = y > clip_hi ? clip_hi : y   (a NaN stays a NaN); then scale: y = y * scale.  Both
 *      whether or not enable is set.
 *   4. a term without noise (or enable == 0), clip and scale copies its 32-bit words unchanged. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_OBSCORRUPT_VERSION 1
#define WL_OBSCORRUPT_MAX_TERMS 64
#define WL_OBSCORRUPT_MAX_DIM (1 << 20)       /* D: 1 .. WL_OBSCORRUPT_MAX_DIM */
#define WL_OC_STREAM_NOISE 16
#define WL_OC_STREAM_BIAS 17

enum WlObsCorruptKind { WL_OC_NONE = 0, WL_OC_CONSTANT = 1, WL_OC_UNIFORM = 2, WL_OC_GAUSSIAN = 3 };
enum WlObsCorruptOp { WL_OC_ADD = 0, WL_OC_SCALE = 1, WL_OC_ABS = 2 };

typedef struct WlObsCorruptTerm {
    int32_t off;                 /* first column of the term: the terms tile [0, D) in order */
    int32_t width;               /* its columns: >= 1 */
    int32_t noise_kind;          /* WlObsCorruptKind */
    int32_t noise_op;            /* WlObsCorruptOp */
    float noise_a, noise_b;      /* constant: (bias, -); uniform: (n_min, fp32(n_max - n_min)); Gaussian: (mean, std) */
    int32_t bias_kind;           /* WlObsCorruptKind; WL_OC_NONE: no bias model.  Needs noise_kind != WL_OC_NONE */
    int32_t bias_per_component;  /* 1: width floats of bias per env, 0: one */
    float bias_a, bias_b;        /* as noise_a, noise_b */
    int32_t bias_off;            /* first float of the term in an env's bias row: the running sum over the terms before it */
    int32_t has_scale;           /* 0: no scale (`scale` must be 1) */
    float clip_lo, clip_hi;      /* -inf, +inf: no clip.  clip_lo <= clip_hi, no NaN */
    float scale;
    int32_t state_row;           /* < 0: read the obs row; else the first of `width` rows of the component-major state */
} WlObsCorruptTerm;

/* Host only.  Db, the floats of bias per env (packed: only terms with a bias model take part; 0 without any), or WL_EINVAL: terms
 * NULL, n_terms outside [1, WL_OBSCORRUPT_MAX_TERMS], D outside [1, WL_OBSCORRUPT_MAX_DIM], a width < 1, the terms not tiling [0, D)
 * in order without gap or overlap, a kind or operation outside its enum, a bias model on a term without noise, a bias_off that is
 * not the running sum, clip_lo > clip_hi or a NaN bound, a parameter or scale that is not finite, has_scale 0 with scale != 1. */
int64_t wl_obs_corrupt_width(const WlObsCorruptTerm* terms, int32_t n_terms, int32_t D);

/* out[e] = the corrupted row of env e (obs float [n][obs_stride], out float [n][out_stride], D <= both strides; state float
 * [rows][state_stride], n <= state_stride, needed only when a term has state_row >= 0; bias float [n][Db], needed only when
 * Db > 0; reset_a / reset_b byte flags [n], reset_b may be NULL).  `terms` is HOST memory: the table travels with the launch by
 * value, so the call may be captured into a graph.  One launch, no atomics; a bias element is stored by the one lane that owns it.
 * `out` may be exactly `obs` with out_stride == obs_stride (in place) or disjoint from it.
 * WL_EINVAL: NULL obs / out / reset_a / terms, n < 1, a stride < D, a table wl_obs_corrupt_width refuses, a state_row term without
 * `state`, with state_stride < n or with state_row + width beyond the WL_S_COUNT rows of the state, Db > 0 without `bias`,
 * n * stride >= 2^31 - 16 for either stride, `out` overlapping `obs` in part, `bias` overlapping `obs`, or what the launch stores
 * (`out`, `bias`) overlapping each other, reset_a, reset_b or the state rows a state_row term reads; WL_EALIGN: a float pointer not
 * 4-byte aligned. */
int wl_obs_corrupt_apply(int32_t n, int32_t D, const float* obs, int64_t obs_stride, const WlObsCorruptTerm* terms, int32_t n_terms,
                         const float* state, int64_t state_stride, float* bias, const uint8_t* reset_a, const uint8_t* reset_b,
                         float* out, int64_t out_stride, uint64_t seed, uint64_t step, uint64_t env_offset, int32_t enable, void* stream);

/* WL_OBSCORRUPT_VERSION of the library */
int wl_obs_corrupt_version(void);

#ifdef __cplusplus
}
#endif

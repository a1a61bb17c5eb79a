/* wheeledlab_amd_history.h -- observation history: the last H frames of every observation term stacked into one policy row, kept per env
 * and refilled when the env resets (the behaviour of IsaacLab's history_length / flatten_history_dim, backed there by a per-env
 * circular buffer).
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): it runs once per env step on the stepwise collection path, between
 * the fused step's observation and the policy step.  Same conventions as that header: device pointers, `stream` a hipStream_t (NULL =
 * the default stream), asynchronous on that stream, the caller owns every buffer, return 0 (WL_OK) or a negative WL_E* code,
 * arguments validated before any launch.
 *
 * A raw observation row of D floats is cut into terms; term k takes columns [src_off, src_off + width) of it and keeps `frames`
 * of them.  The stacked row of Dh = sum_k width_k * frames_k floats is term-major, oldest frame first inside each term:
 *     [ term0 frame t-H0+1 .. term0 frame t | term1 frame t-H1+1 .. term1 frame t | .. ]
 * and term k starts at column dst_off_k = sum_{i<k} width_i * frames_i of it.  One term covering the whole row gives the time-major
 * [H][D] layout. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_OBSHIST_VERSION 1
#define WL_OBSHIST_MAX_TERMS 64
#define WL_OBSHIST_MAX_FRAMES 64
#define WL_OBSHIST_MAX_DIM (1 << 20)       /* D: 1 .. WL_OBSHIST_MAX_DIM */

typedef struct WlObsHistoryTerm {
    int32_t src_off;   /* first column of the term in the raw row */
    int32_t width;     /* its columns: >= 1 */
    int32_t frames;    /* frames kept: 1 .. WL_OBSHIST_MAX_FRAMES */
    int32_t dst_off;   /* first column of the term in the stacked row */
} WlObsHistoryTerm;

/* Host only.  The stacked width Dh of a table over raw rows of D floats, or WL_EINVAL: terms NULL, n_terms outside
 * [1, WL_OBSHIST_MAX_TERMS], D outside [1, WL_OBSHIST_MAX_DIM], a width < 1, frames outside [1, WL_OBSHIST_MAX_FRAMES], the terms
 * not tiling [0, D) in order without gap or overlap, or a dst_off that is not the running sum. */
int64_t wl_obs_history_width(const WlObsHistoryTerm* terms, int32_t n_terms, int32_t D);

/* next[e] = the stacked row of env e after its raw row obs[e] (obs float [n][obs_stride], D <= obs_stride; prev, next float [n][Dh]):
 *   reset_a[e] | reset_b[e] non-zero, or prev == NULL: every frame of every term = the term's columns of obs[e];
 *   otherwise: frames 1 .. H-1 of prev[e] move to 0 .. H-2, the term's columns of obs[e] become frame H-1.
 * reset_a / reset_b are byte flags [n] (reset_b may be NULL).  `terms` is HOST memory: the table travels with the launch by value,
 * so the call may be captured into a graph.  A pure permuted copy: bits in, bits out; one launch, no atomics.
 * WL_EINVAL: NULL obs / next / reset_a / terms, n < 1, obs_stride < D, a table wl_obs_history_width refuses, n * Dh or
 * n * obs_stride >= 2^31, `next` overlapping `prev` or `obs`; WL_EALIGN: a float pointer not 4-byte aligned. */
int wl_obs_history_push(int32_t n, int32_t D, const float* obs, int64_t obs_stride, const WlObsHistoryTerm* terms, int32_t n_terms,
                        const float* prev, float* next, const uint8_t* reset_a, const uint8_t* reset_b, void* stream);

/* WL_OBSHIST_VERSION of the library */
int wl_obs_history_version(void);

#ifdef __cplusplus
}
#endif

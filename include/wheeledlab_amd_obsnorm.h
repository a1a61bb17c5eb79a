/* wheeledlab_amd_obsnorm.h -- empirical observation normalisation: running per-feature moments of a rollout's observations, and
 * the normalisation folded into the first-layer weights the fused collectors read.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): it runs once per learning iteration, between collection and the
 * update.  Same conventions as that header: device pointers, `stream` a hipStream_t (NULL = the default stream), every entry point
 * asynchronous on that stream, the caller owns every buffer, return 0 (WL_OK) or a negative WL_E* code, arguments validated before
 * any launch.
 *
 * State per feature c (rsl_rl.modules.EmpiricalNormalization): mean_c, var_c, std_c = sqrt(var_c) as float [D], count as ONE int64;
 * inv_std_c = 1 / (std_c + eps) is kept beside them because every reader wants it.  An observation is normalised as
 * (x - mean_c) * inv_std_c.  A batch of m rows with batch mean mb and biased batch variance vb is merged as
 *     count += m;  rate = m / count;  d = mb - mean;  mean += rate * d;  var += rate * (vb - var + d * (mb - mean_new))
 * (the pooled-moments merge: K merges of n rows end where one merge of K * n rows ends), and not at all once count >= until. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_OBSNORM_VERSION 1
#define WL_OBSNORM_MAX_DIM (1 << 20)       /* D: 1 .. WL_OBSNORM_MAX_DIM */
#define WL_OBSNORM_MAX_ROWS (1 << 23)      /* rows per accumulate call (a float64 sum of at most 2^23 terms) */

/* bytes of `scratch` wl_obsnorm_accumulate needs for a [rows][D] matrix with this row stride (floats); < 0: a WL_E* code */
int64_t wl_obsnorm_scratch_bytes(int64_t rows, int32_t D, int64_t row_stride);

/* One pass over the float matrix x[rows][row_stride] (D <= row_stride features per row), every element read once:
 *   out      NULL, or float [rows][row_stride] (may be x itself): out[r][c] = (x[r][c] - mean[c]) * inv_std[c] in float
 *   sums     double [2][D]: sums[0][c] = sum_r (x[r][c] - mean[c]), sums[1][c] = sum_r (x[r][c] - mean[c])^2, accumulated in double
 *            about the float mean as it stands
 *   scratch  wl_obsnorm_scratch_bytes(rows, D, row_stride) bytes: per-workgroup double partial sums, which a second launch adds in
 *            a fixed order -- no atomics: two calls on equal input give equal bytes
 * Rows narrower than a wavefront (D < 64) that lie back to back (row_stride == D) are read as one run, D * (64 / D) lanes of a
 * wavefront across 64 / D rows; everything else one lane per column.
 * WL_EINVAL: a NULL pointer (out excepted), rows outside [1, WL_OBSNORM_MAX_ROWS], D outside [1, WL_OBSNORM_MAX_DIM],
 * row_stride < D; WL_EALIGN: a float pointer not 4-byte aligned, scratch or sums not 8-byte aligned. */
int wl_obsnorm_accumulate(int64_t rows, int32_t D, const float* x, int64_t row_stride, const float* mean, const float* inv_std, float* out,
                          double* scratch, double* sums, void* stream);

/* The merge above in double from the float state and the sums of wl_obsnorm_accumulate over batch_count rows (of every rank, when the
 * sums were all-reduced); mean, var, std and inv_std = 1 / (std + eps) are each rounded once to float.  `count` is a device int64 and
 * the `until` test reads it on the device: when *count >= until nothing is written, else *count += batch_count.
 * WL_EINVAL: a NULL pointer, D out of range, batch_count < 1, until < 0, eps not positive and finite; WL_EALIGN as above (sums and
 * count 8-byte aligned). */
int wl_obsnorm_update(int32_t D, const double* sums, int64_t batch_count, int64_t until, double eps, float* mean, float* var, float* std,
                      float* inv_std, int64_t* count, void* stream);

/* The normalisation folded into a first layer in nn.Linear's layout (w1 float [H][D], b1 float [H]):
 *   w1_out[j][c] = w1[j][c] * inv_std[c]
 *   b1_out[j]    = b1[j] - sum_c w1[j][c] * mean[c] * inv_std[c]      (the sum in double, in a fixed order)
 * so that w1_out x + b1_out = w1 ((x - mean) * inv_std) + b1.  w1_out / b1_out must not overlap w1 / b1.
 * WL_EINVAL: a NULL pointer, D out of range, H outside [1, 65535]; WL_EALIGN: a pointer not 4-byte aligned. */
int wl_obsnorm_fold(int32_t D, int32_t H, const float* w1, const float* b1, const float* mean, const float* inv_std, float* w1_out,
                    float* b1_out, void* stream);

/* WL_OBSNORM_VERSION of the library */
int wl_obsnorm_version(void);

#ifdef __cplusplus
}
#endif

// wl_obs_norm.hip -- empirical observation normalisation (include/wheeledlab_amd_obsnorm.h) for gfx950.
//
// accumulate is the hot path: one pass over the rollout's observation block (524 288 x 689 floats for the elevation agent at 4096
// envs), each element read once, optionally written back normalised, its two moments about the frozen mean summed in double.  Two
// mappings, chosen by obsnorm_plan() from the shape alone:
//   wide    (D >= 64 or strided rows) block = ONE wavefront = 64 consecutive columns of a row chunk: consecutive lanes read
//           consecutive addresses of a row (rows are not 16-byte aligned when D is odd, so the loads stay dwords), a lane keeps its
//           column's two sums in registers down the chunk with OBSNORM_UNROLL rows in flight.  Grid = strips x chunks, strips fastest
//           so that neighbouring workgroups read neighbouring segments of the same rows.
//   narrow  (D < 64, rows back to back) the matrix is one run of floats; a wavefront uses D * (64 / D) lanes over 64 / D rows per
//           load (56 of 64 lanes at D = 14), so a lane keeps ONE column for its whole walk; the lanes and wavefronts of a workgroup
//           that share a column are added through LDS in a fixed order.
// Each workgroup stores one double partial per column and moment; a second launch adds the partials in a fixed order.  No atomics
// anywhere: the result is a function of the input bytes.  update and fold are small: one workgroup, and one workgroup per output row.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_obsnorm.h"
#include "wl_kernel_common.h"
#include "wl_obs_norm_dev.h"

namespace {

template <bool WRITE>
__global__ void __launch_bounds__(64) obsnorm_wide_kernel(const float* x, float* out, const float* __restrict__ mean,
                                                          const float* __restrict__ inv_std, double* __restrict__ scratch, const int64_t rows,
                                                          const int D, const int64_t row_stride, const int64_t rows_per_chunk) {
    const int c = blockIdx.x * 64 + (int)threadIdx.x;
    if (c >= D) return;
    const float m = mean[c], is = inv_std[c];
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t r = r0; r < r1; r += OBSNORM_UNROLL) {
        float v[OBSNORM_UNROLL];
#pragma unroll
        for (int u = 0; u < OBSNORM_UNROLL; ++u) v[u] = r + u < r1 ? x[(r + u) * row_stride + c] : m;   // past the end: adds +0
#pragma unroll
        for (int u = 0; u < OBSNORM_UNROLL; ++u) {
            obsnorm_add(v[u], m, s1, s2);
            if (WRITE && r + u < r1) out[(r + u) * row_stride + c] = obsnorm_apply(v[u], m, is);
        }
    }
    scratch[((int64_t)blockIdx.y * 2 + 0) * D + c] = s1;
    scratch[((int64_t)blockIdx.y * 2 + 1) * D + c] = s2;
}

template <bool WRITE>
__global__ void __launch_bounds__(64 * OBSNORM_NARROW_WAVES) obsnorm_narrow_kernel(const float* x, float* out, const float* __restrict__ mean,
                                                                                   const float* __restrict__ inv_std,
                                                                                   double* __restrict__ scratch, const int64_t total,
                                                                                   const int D, const int lanes, const int64_t loads,
                                                                                   const int64_t loads_per_wave) {
    __shared__ double sh[2][64 * OBSNORM_NARROW_WAVES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const bool active = lane < lanes;
    const int c = active ? lane % D : 0;
    const float m = mean[c], is = inv_std[c];
    const int64_t i0 = ((int64_t)blockIdx.x * OBSNORM_NARROW_WAVES + wave) * loads_per_wave;
    const int64_t i1 = i0 + loads_per_wave < loads ? i0 + loads_per_wave : loads;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = i0; i < i1; i += OBSNORM_UNROLL) {
        float v[OBSNORM_UNROLL];
        bool ok[OBSNORM_UNROLL];
#pragma unroll
        for (int u = 0; u < OBSNORM_UNROLL; ++u) {
            const int64_t k = (i + u) * lanes + lane;
            ok[u] = active && i + u < i1 && k < total;
            v[u] = ok[u] ? x[k] : m;
        }
#pragma unroll
        for (int u = 0; u < OBSNORM_UNROLL; ++u) {
            obsnorm_add(v[u], m, s1, s2);
            if (WRITE && ok[u]) out[(i + u) * lanes + lane] = obsnorm_apply(v[u], m, is);
        }
    }
    sh[0][threadIdx.x] = s1;
    sh[1][threadIdx.x] = s2;
    __syncthreads();
    if ((int)threadIdx.x < D) {   // column t: wavefront by wavefront, its lanes t, t + D, ... in order
        double a1 = 0.0, a2 = 0.0;
        for (int w = 0; w < OBSNORM_NARROW_WAVES; ++w)
            for (int l = (int)threadIdx.x; l < lanes; l += D) {
                a1 += sh[0][w * 64 + l];
                a2 += sh[1][w * 64 + l];
            }
        scratch[((int64_t)blockIdx.x * 2 + 0) * D + threadIdx.x] = a1;
        scratch[((int64_t)blockIdx.x * 2 + 1) * D + threadIdx.x] = a2;
    }
}

// sums[i] = sum over the partials p of scratch[p][i], i in [0, 2 D): four quarters of the partials side by side, then the quarters in order
__global__ void __launch_bounds__(256) obsnorm_sum_kernel(const double* __restrict__ scratch, double* __restrict__ sums, const int D,
                                                          const int partials) {
    __shared__ double sh[4][64];
    const int i = blockIdx.x * 64 + (int)threadIdx.x, q = (int)threadIdx.y;
    const int per = (partials + 3) / 4;
    const int p1 = (q + 1) * per < partials ? (q + 1) * per : partials;
    // partial p holds [2][D] doubles and sums is [2][D]: the same flat index on both sides
    double s = 0.0;
    if (i < 2 * D)
        for (int p = q * per; p < p1; ++p) s += scratch[(int64_t)p * 2 * D + i];
    sh[q][threadIdx.x] = s;
    __syncthreads();
    if (q == 0 && i < 2 * D) sums[i] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one workgroup: every lane reads the count before any lane may advance it
__global__ void __launch_bounds__(1024) obsnorm_update_kernel(const int D, const double* __restrict__ sums, const int64_t batch_count,
                                                              const int64_t until, const double eps, float* __restrict__ mean,
                                                              float* __restrict__ var, float* __restrict__ sd, float* __restrict__ inv_std,
                                                              int64_t* count) {
    const int64_t seen = *count;
    __syncthreads();
    if (seen >= until) return;
    const int64_t now = seen + batch_count;
    for (int c = (int)threadIdx.x; c < D; c += (int)blockDim.x) {
        const ObsNormState s = obsnorm_merge(sums[c], sums[D + c], (double)batch_count, (double)now, mean[c], var[c], eps);
        mean[c] = s.mean;
        var[c] = s.var;
        sd[c] = s.std;
        inv_std[c] = s.inv_std;
    }
    if (threadIdx.x == 0) *count = now;
}

// one workgroup per output row j: lanes stride the columns, the double terms of b'[j] meet in LDS and are added in a fixed order
__global__ void __launch_bounds__(256) obsnorm_fold_kernel(const int D, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                           float* __restrict__ w1_out, float* __restrict__ b1_out) {
    __shared__ double sh[256];
    const int j = blockIdx.x;
    const float* w = w1 + (int64_t)j * D;
    float* wo = w1_out + (int64_t)j * D;
    double s = 0.0;
    for (int c = (int)threadIdx.x; c < D; c += 256) {
        const float wv = w[c], is = inv_std[c];
        wo[c] = obsnorm_fold_weight(wv, is);
        s += obsnorm_fold_term(wv, mean[c], is);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) b1_out[j] = (float)((double)b1[j] - sh[0]);
}

inline bool dims_ok(int64_t rows, int D, int64_t row_stride) {
    return rows >= 1 && rows <= WL_OBSNORM_MAX_ROWS && D >= 1 && D <= WL_OBSNORM_MAX_DIM && row_stride >= D &&
           row_stride <= (int64_t)1 << 40;
}

}  // namespace

extern "C" {

int wl_obsnorm_version(void) { return WL_OBSNORM_VERSION; }

int64_t wl_obsnorm_scratch_bytes(int64_t rows, int32_t D, int64_t row_stride) {
    if (!dims_ok(rows, D, row_stride)) return WL_EINVAL;
    return (int64_t)obsnorm_plan(rows, D, row_stride).partials * 2 * D * (int64_t)sizeof(double);
}

int wl_obsnorm_accumulate(int64_t rows, int32_t D, const float* x, int64_t row_stride, const float* mean, const float* inv_std, float* out,
                          double* scratch, double* sums, void* stream) {
    if (!x || !mean || !inv_std || !scratch || !sums || !dims_ok(rows, D, row_stride)) return WL_EINVAL;
    if (!aligned(x, 4) || !aligned(mean, 4) || !aligned(inv_std, 4) || !aligned(out, 4) || !aligned(scratch, 8) || !aligned(sums, 8))
        return WL_EALIGN;
    const ObsNormPlan p = obsnorm_plan(rows, D, row_stride);
    hipStream_t s = (hipStream_t)stream;
    clear_error();
    if (p.narrow) {
        const int lanes = p.rows_per_load * D;
        const int64_t loads = (rows + p.rows_per_load - 1) / p.rows_per_load;
        const dim3 grid((unsigned)p.partials), block(64 * OBSNORM_NARROW_WAVES);
        if (out)
            obsnorm_narrow_kernel<true><<<grid, block, 0, s>>>(x, out, mean, inv_std, scratch, rows * D, D, lanes, loads, p.per_partial);
        else
            obsnorm_narrow_kernel<false><<<grid, block, 0, s>>>(x, out, mean, inv_std, scratch, rows * D, D, lanes, loads, p.per_partial);
    } else {
        const dim3 grid((unsigned)p.strips, (unsigned)p.partials), block(64);
        if (out)
            obsnorm_wide_kernel<true><<<grid, block, 0, s>>>(x, out, mean, inv_std, scratch, rows, D, row_stride, p.per_partial);
        else
            obsnorm_wide_kernel<false><<<grid, block, 0, s>>>(x, out, mean, inv_std, scratch, rows, D, row_stride, p.per_partial);
    }
    if (launch_status() != WL_OK) return WL_ELAUNCH;
    obsnorm_sum_kernel<<<dim3((unsigned)((2 * (int64_t)D + 63) / 64)), dim3(64, 4), 0, s>>>(scratch, sums, D, p.partials);
    return launch_status();
}

int wl_obsnorm_update(int32_t D, const double* sums, int64_t batch_count, int64_t until, double eps, float* mean, float* var, float* std,
                      float* inv_std, int64_t* count, void* stream) {
    if (!sums || !mean || !var || !std || !inv_std || !count || D < 1 || D > WL_OBSNORM_MAX_DIM || batch_count < 1 || until < 0) return WL_EINVAL;
    if (!(eps > 0.0 && eps < (double)INFINITY)) return WL_EINVAL;
    if (!aligned(sums, 8) || !aligned(count, 8) || !aligned(mean, 4) || !aligned(var, 4) || !aligned(std, 4) || !aligned(inv_std, 4))
        return WL_EALIGN;
    clear_error();
    obsnorm_update_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(D, sums, batch_count, until, eps, mean, var, std, inv_std, count);
    return launch_status();
}

int wl_obsnorm_fold(int32_t D, int32_t H, const float* w1, const float* b1, const float* mean, const float* inv_std, float* w1_out,
                    float* b1_out, void* stream) {
    if (!w1 || !b1 || !mean || !inv_std || !w1_out || !b1_out || D < 1 || D > WL_OBSNORM_MAX_DIM || H < 1 || H > 65535) return WL_EINVAL;
    if (!aligned(w1, 4) || !aligned(b1, 4) || !aligned(mean, 4) || !aligned(inv_std, 4) || !aligned(w1_out, 4) || !aligned(b1_out, 4))
        return WL_EALIGN;
    clear_error();
    obsnorm_fold_kernel<<<(unsigned)H, 256, 0, (hipStream_t)stream>>>(D, w1, b1, mean, inv_std, w1_out, b1_out);
    return launch_status();
}

}  // extern "C"

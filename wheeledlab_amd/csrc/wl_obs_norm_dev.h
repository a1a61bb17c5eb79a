// wl_obs_norm_dev.h -- the arithmetic of the observation normaliser (see wl_obs_norm.hip): one element's contribution to the
// moments, the merge of a batch into the running state, and one term of the folded first layer.  __host__ __device__ and a header
// of its own so that tests/host_sim can compile the same functions for the host and hold them against the float64 reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace {

#define WL_ON __host__ __device__ __forceinline__

// the launch shape of wl_obsnorm_accumulate: a function of (rows, D, row_stride) alone, so equal input takes equal summation order
struct ObsNormPlan {
    int narrow;             // 1: the matrix as one contiguous run, D * (64 / D) lanes of a wavefront across 64 / D rows
    int rows_per_load;      // narrow: rows one wave-load covers (64 / D)
    int strips;             // wide: 64-column strips
    int partials;           // workgroups that each write one [2][D] double partial: narrow blocks, or wide row chunks
    int64_t per_partial;    // narrow: wave-loads per wavefront; wide: rows per chunk
};

constexpr int OBSNORM_TARGET_WAVES = 4096;   // 256 CUs x 4 SIMDs x 4: the row chunks fill the chip several times
constexpr int OBSNORM_MAX_CHUNKS = 1024;     // wide: the sum launch walks a quarter of the partials per lane, 256 at the most
constexpr int OBSNORM_NARROW_WAVES = 4;      // wavefronts per narrow workgroup
constexpr int OBSNORM_UNROLL = 8;            // loads in flight per lane

WL_ON ObsNormPlan obsnorm_plan(int64_t rows, int D, int64_t row_stride) {
    ObsNormPlan p{};
    if (D < 64 && row_stride == D) {
        p.narrow = 1;
        p.rows_per_load = 64 / D;
        const int64_t loads = (rows + p.rows_per_load - 1) / p.rows_per_load;
        // at least OBSNORM_UNROLL wave-loads per wavefront, at most 256 workgroups (their partials are summed by one launch)
        int64_t blocks = (loads + OBSNORM_NARROW_WAVES * OBSNORM_UNROLL - 1) / (OBSNORM_NARROW_WAVES * OBSNORM_UNROLL);
        blocks = blocks < 1 ? 1 : blocks > 256 ? 256 : blocks;
        p.per_partial = (loads + blocks * OBSNORM_NARROW_WAVES - 1) / (blocks * OBSNORM_NARROW_WAVES);
        p.partials = (int)((loads + p.per_partial * OBSNORM_NARROW_WAVES - 1) / (p.per_partial * OBSNORM_NARROW_WAVES));
        return p;
    }
    p.strips = (D + 63) / 64;
    int64_t chunks = (OBSNORM_TARGET_WAVES + p.strips - 1) / p.strips;
    const int64_t most = (rows + 2 * OBSNORM_UNROLL - 1) / (2 * OBSNORM_UNROLL);   // at least two unrolled trips per chunk
    chunks = chunks > most ? most : chunks;
    chunks = chunks > OBSNORM_MAX_CHUNKS ? OBSNORM_MAX_CHUNKS : chunks;
    chunks = chunks < 1 ? 1 : chunks;
    p.per_partial = (rows + chunks - 1) / chunks;
    p.partials = (int)((rows + p.per_partial - 1) / p.per_partial);
    return p;
}

// one element about the frozen float mean: d = x - mean in double (exact up to double's rounding), s1 += d, s2 += d^2
WL_ON void obsnorm_add(float x, float mean, double& s1, double& s2) {
    const double d = (double)x - (double)mean;
    s1 += d;
    s2 = fma(d, d, s2);
}

// the normalised value, in float: one rounding in the difference, one in the product
WL_ON float obsnorm_apply(float x, float mean, float inv_std) { return (x - mean) * inv_std; }

struct ObsNormState {
    float mean, var, std, inv_std;
};

// the pooled-moments merge of a batch of m rows with s1 = sum (x - mean), s2 = sum (x - mean)^2 into a state that has seen
// count_new - m rows; mean and var rounded once from double
WL_ON ObsNormState obsnorm_merge(double s1, double s2, double m, double count_new, float mean, float var, double eps) {
    const double rate = m / count_new;
    const double d = s1 / m;                              // batch mean - mean
    const double vb = fmax(s2 / m - d * d, 0.0);          // biased batch variance (about its own mean)
    const double mean_new = (double)mean + rate * d;
    const double var_new = (double)var + rate * (vb - (double)var + d * (d - rate * d));   // d - rate d = batch mean - mean_new
    // std and inv_std are functions of the ROUNDED variance: a state restored from (mean, var) alone has the same bits
    const float var32 = (float)var_new;
    const double sd = sqrt((double)var32);
    return ObsNormState{(float)mean_new, var32, (float)sd, (float)(1.0 / (sd + eps))};
}

// the folded first layer: W'[j][c], and the term of b'[j] that column c takes away
WL_ON float obsnorm_fold_weight(float w, float inv_std) { return w * inv_std; }
WL_ON double obsnorm_fold_term(float w, float mean, float inv_std) { return (double)w * (double)mean * (double)inv_std; }

}  // namespace

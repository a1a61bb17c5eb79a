// wl_obs_corrupt.hip -- observation corruption (include/wheeledlab_amd_obsnoise.h) for gfx950: noise, per-episode bias, clip and scale
// of every term of the observation row in one launch per env step.
//
// Lane i of the grid owns Philox block i % nblk of env i / nblk: four consecutive columns of one row, whose four words are the four
// words of ONE block -- one generator call per lane and none where the lane's columns draw nothing (no noise, constant noise, enable
// off).  Consecutive lanes own consecutive 16 bytes of a row, so a wavefront reads and writes 1 KiB of consecutive addresses.  A
// lane's four columns start on a 16-byte line only where the row pitch allows it: with 3208 columns every row does, with 689 (odd)
// every fourth row does, every other fourth sits on an 8-byte boundary and the odd rows on 4 -- the lane looks at its own address and
// moves its words as one dwordx4, two dwordx2 or four dwords (the row's tail, D % 4 columns, as dwords).  The table (at most 64 terms,
// packed to 48 bytes each) arrives by value with the launch -- nothing is staged, so the call can be captured -- and every workgroup
// keeps it in LDS; a lane finds the term of its first column by six halvings and walks on from there (wl_obs_corrupt_dev.h).  One
// 32-bit division per lane.  No atomics; a bias element is stored only by the lane that owns its column.  Plain stores: the row is read
// again at once by the history push or the policy step (the non-temporal hint measured 26 - 28 % slower for the history push's rows).
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_obsnoise.h"
#include "wl_kernel_common.h"
#include "wl_obs_corrupt_dev.h"

namespace {

struct ObsCorruptTable {
    ObsCorruptDevTerm t[WL_OBSCORRUPT_MAX_TERMS];
};
static_assert(sizeof(ObsCorruptTable) + sizeof(ObsCorruptArgs) + 32 <= 4096, "the launch's arguments must fit a kernel's 4 KiB");

typedef uint32_t oc_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t oc_u32x2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(kBlock) obs_corrupt_kernel(const ObsCorruptArgs a, uint32_t* out, const int64_t out_stride, const ObsCorruptTable tab) {
    __shared__ ObsCorruptDevTerm t[WL_OBSCORRUPT_MAX_TERMS];
    layer_table_to_lds(t, tab, a.n_terms);
    const unsigned gid = blockIdx.x * kBlock + threadIdx.x;        // (unsigned: the last block may reach past 2^31)
    if (gid >= (unsigned)a.lanes) return;
    const int lane = (int)gid;
    const int e = (int)((unsigned)lane / (unsigned)a.nblk);
    const int c0 = (lane - e * a.nblk) * OBSCORRUPT_SLOT;
    const int count = a.D - c0 < OBSCORRUPT_SLOT ? a.D - c0 : OBSCORRUPT_SLOT;
    // (`out` may be `obs`: no __restrict__, and every lane reads its own four words before it writes them)
    const uint32_t* src = a.obs + (int64_t)e * a.obs_stride + c0;
    uint32_t* dst = out + (int64_t)e * out_stride + c0;
    uint32_t x[OBSCORRUPT_SLOT] = {0u, 0u, 0u, 0u}, v[OBSCORRUPT_SLOT] = {0u, 0u, 0u, 0u};
    if (count == OBSCORRUPT_SLOT) {
        const unsigned al = (unsigned)(uintptr_t)src & 15u;
        if (al == 0u) {
            const oc_u32x4 q = *(const oc_u32x4*)src;
            x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
        } else if (al == 8u) {
            const oc_u32x2 q0 = *(const oc_u32x2*)src, q1 = *(const oc_u32x2*)(src + 2);
            x[0] = q0.x, x[1] = q0.y, x[2] = q1.x, x[3] = q1.y;
        } else {
            x[0] = src[0], x[1] = src[1], x[2] = src[2], x[3] = src[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < OBSCORRUPT_SLOT - 1; ++i)      // (static indices: the words stay in registers)
            if (i < count) x[i] = src[i];
    }
    obscorrupt_lane(e, c0, count, a, t, x, v);
    if (count == OBSCORRUPT_SLOT) {
        const unsigned al = (unsigned)(uintptr_t)dst & 15u;
        if (al == 0u) {
            const oc_u32x4 q = {v[0], v[1], v[2], v[3]};
            *(oc_u32x4*)dst = q;
        } else if (al == 8u) {
            const oc_u32x2 q0 = {v[0], v[1]}, q1 = {v[2], v[3]};
            *(oc_u32x2*)dst = q0;
            *(oc_u32x2*)(dst + 2) = q1;
        } else {
            dst[0] = v[0], dst[1] = v[1], dst[2] = v[2], dst[3] = v[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < OBSCORRUPT_SLOT - 1; ++i)
            if (i < count) dst[i] = v[i];
    }
}

}  // namespace

extern "C" {

int wl_obs_corrupt_version(void) { return WL_OBSCORRUPT_VERSION; }

int64_t wl_obs_corrupt_width(const WlObsCorruptTerm* terms, int32_t n_terms, int32_t D) {
    const int64_t w = obscorrupt_width(terms, n_terms, D);
    return w < 0 ? (int64_t)WL_EINVAL : w;
}

int wl_obs_corrupt_apply(int32_t n, int32_t D, const float* obs, int64_t obs_stride, const WlObsCorruptTerm* terms, int32_t n_terms,
                         const float* state, int64_t state_stride, float* bias, const uint8_t* reset_a, const uint8_t* reset_b,
                         float* out, int64_t out_stride, uint64_t seed, uint64_t step, uint64_t env_offset, int32_t enable, void* stream) {
    if (!obs || !out || !reset_a || !terms || n < 1) return WL_EINVAL;
    const int64_t Db = obscorrupt_width(terms, n_terms, D);
    if (Db < 0 || obs_stride < D || out_stride < D) return WL_EINVAL;
    if (Db > 0 && !bias) return WL_EINVAL;
    for (int k = 0; k < n_terms; ++k) {
        if (terms[k].state_row < 0) continue;
        if (!state || state_stride < n || (int64_t)terms[k].state_row + terms[k].width > WL_S_COUNT) return WL_EINVAL;
    }
    const int64_t limit = ((int64_t)1 << 31) - 16;
    if ((int64_t)n * obs_stride >= limit || (int64_t)n * out_stride >= limit || (int64_t)n * (Db > 0 ? Db : 1) >= limit) return WL_EINVAL;
    const int64_t obs_bytes = ((int64_t)(n - 1) * obs_stride + D) * 4, out_bytes = ((int64_t)(n - 1) * out_stride + D) * 4;
    // what the launch stores (`out`, the bias block) may touch nothing else it reads: the raw rows -- unless they ARE `out`, in place
    // with equal strides, where every lane reads its own words before it writes them --, the flags and the state rows of the table
    const bool in_place = (const float*)out == obs && out_stride == obs_stride;
    Span spans[5 + WL_OBSCORRUPT_MAX_TERMS] = {{out, out_bytes},
                                               {Db > 0 ? bias : nullptr, (int64_t)n * Db * 4},
                                               {in_place ? nullptr : obs, obs_bytes},
                                               {reset_a, n},
                                               {reset_b, n}};      // then one per term: NULL without a state row
    for (int k = 0; k < n_terms; ++k) {
        if (terms[k].state_row < 0) continue;
        const int64_t words = (int64_t)(terms[k].width - 1) * state_stride + n;      // rows state_row .. state_row + width - 1, n of each
        spans[5 + k] = Span{state + (int64_t)terms[k].state_row * state_stride, words * 4};
    }
    if (any_overlap(spans, 2)) return WL_EINVAL;
    if (!aligned(obs, 4) || !aligned(out, 4) || !aligned(state, 4) || !aligned(bias, 4)) return WL_EALIGN;
    ObsCorruptArgs a{};
    a.obs = (const uint32_t*)obs;
    a.state = (const uint32_t*)state;
    a.bias = bias;
    a.reset_a = reset_a;
    a.reset_b = reset_b;
    a.obs_stride = obs_stride;
    a.state_stride = state_stride;
    a.seed = seed;
    a.step = step;
    a.env0 = (uint32_t)env_offset;
    a.n = n;
    a.D = D;
    a.Db = (int32_t)Db;
    a.n_terms = n_terms;
    a.nblk = (D + OBSCORRUPT_SLOT - 1) / OBSCORRUPT_SLOT;
    a.lanes = (int32_t)((int64_t)n * a.nblk);        // <= n * obs_stride < 2^31
    a.enable = enable != 0;
    ObsCorruptTable tab{};
    for (int k = 0; k < n_terms; ++k) tab.t[k] = obscorrupt_pack(terms[k]);
    const unsigned grid = (unsigned)(((int64_t)a.lanes + kBlock - 1) / kBlock);      // (in 64 bits: lanes may come within 16 of 2^31)
    clear_error();
    obs_corrupt_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(a, (uint32_t*)out, out_stride, tab);
    return launch_status();
}

}  // extern "C"

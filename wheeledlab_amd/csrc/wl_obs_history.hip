// wl_obs_history.hip -- the observation-history push (include/wheeledlab_amd_history.h) for gfx950.
//
// One launch per env step: the new stacked rows [n][Dh] are a permuted copy of the previous stacked rows and the raw rows.  The flat
// output block is cut into 16-byte lines of `next`; lane i of the grid owns line i, so a wavefront stores 1 KiB of consecutive
// addresses as one dwordx4 per lane.  `next` is a storage row in general and need not start on a line (Dh and n * Dh are no multiples
// of 4 in general: 14 * 3 = 42, 689 * 2): the first and the last line are then partial and go out as dwords.  The reads are dword gathers: the shift by one frame
// (width_k columns) breaks any alignment the stores have, and consecutive lanes still read consecutive addresses except where a
// line crosses a term or a row.  The table (at most 64 terms of 16 bytes) arrives by value with the launch -- nothing is staged, so
// the call can be captured -- and every workgroup keeps it in LDS; a lane finds the term of its first output by six halvings and
// walks on from there (wl_obs_history_dev.h).  No loop depends on data, no wavefront waits for another, no atomics.
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_history.h"
#include "wl_kernel_common.h"
#include "wl_obs_history_dev.h"

namespace {

struct ObsHistTable {
    WlObsHistoryTerm t[WL_OBSHIST_MAX_TERMS];
};

typedef uint32_t obshist_u32x4 __attribute__((ext_vector_type(4)));

// plain stores: the row is read again at once (the next push, the policy step); with the non-temporal hint the launch measured 26 - 28 %
// slower at the elevation and visual shapes
__global__ void __launch_bounds__(kBlock) obshist_push_kernel(const ObsHistArgs a, uint32_t* __restrict__ next, const ObsHistTable tab) {
    __shared__ WlObsHistoryTerm t[WL_OBSHIST_MAX_TERMS];
    layer_table_to_lds(t, tab, a.n_terms);
    const int slot = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (slot >= a.slots) return;
    uint32_t v[OBSHIST_SLOT];
    int j0;
    const int count = obshist_gather(slot, a, t, v, j0);
    if (count == OBSHIST_SLOT) {
        const obshist_u32x4 q = {v[0], v[1], v[2], v[3]};
        *(obshist_u32x4*)(next + j0) = q;
    } else {
        for (int i = 0; i < count; ++i) next[j0 + i] = v[i];
    }
}

}  // namespace

extern "C" {

int wl_obs_history_version(void) { return WL_OBSHIST_VERSION; }

int64_t wl_obs_history_width(const WlObsHistoryTerm* terms, int32_t n_terms, int32_t D) {
    const int64_t w = obshist_width(terms, n_terms, D);
    return w < 0 ? (int64_t)WL_EINVAL : w;
}

int wl_obs_history_push(int32_t n, int32_t D, const float* obs, int64_t obs_stride, const WlObsHistoryTerm* terms, int32_t n_terms,
                        const float* prev, float* next, const uint8_t* reset_a, const uint8_t* reset_b, void* stream) {
    if (!obs || !next || !reset_a || !terms || n < 1) return WL_EINVAL;
    const int64_t Dh = obshist_width(terms, n_terms, D);
    if (Dh < 0 || obs_stride < D) return WL_EINVAL;
    const int64_t limit = ((int64_t)1 << 31) - 16;
    if ((int64_t)n * Dh >= limit || (int64_t)n * obs_stride >= limit) return WL_EINVAL;
    // what the launch stores (`next`) may touch nothing it reads: the raw rows, the previous stacked rows, the flags
    const int64_t row_bytes = (int64_t)n * Dh * 4;
    const Span spans[] = {{next, row_bytes}, {obs, (int64_t)n * obs_stride * 4}, {prev, row_bytes}, {reset_a, n}, {reset_b, n}};
    if (any_overlap(spans, 1)) return WL_EINVAL;
    if (!aligned(obs, 4) || !aligned(prev, 4) || !aligned(next, 4)) return WL_EALIGN;
    ObsHistArgs a{};
    a.obs = (const uint32_t*)obs;
    a.prev = (const uint32_t*)prev;
    a.reset_a = reset_a;
    a.reset_b = reset_b;
    a.obs_stride = obs_stride;
    a.n = n;
    a.Dh = (int32_t)Dh;
    a.n_terms = n_terms;
    a.shift = (int32_t)(((uintptr_t)next >> 2) & 3);
    a.total = (int32_t)((int64_t)n * Dh);
    a.slots = (a.total + a.shift + OBSHIST_SLOT - 1) / OBSHIST_SLOT;
    ObsHistTable tab{};
    for (int k = 0; k < n_terms; ++k) tab.t[k] = terms[k];
    const unsigned grid = (unsigned)((a.slots + kBlock - 1) / kBlock);
    clear_error();
    obshist_push_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(a, (uint32_t*)next, tab);
    return launch_status();
}

}  // extern "C"

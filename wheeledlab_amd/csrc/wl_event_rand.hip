// wl_event_rand.hip -- per-episode domain randomisation (include/wheeledlab_amd_events.h) for gfx950: the reset- and interval-mode
// friction, throttle-damping and mass events of every env in one launch per env step, between two step launches.
//
// One lane per env, no atomics: a lane reads its env's flags and, per term, at most four words of the layer block; it stores only what it
// changed.  Every row is component-major, so a wavefront's accesses to a row are 256 consecutive bytes.  Almost every lane of almost every
// call has nothing to apply (an env resets once per episode): the common path is the flag bytes, one timer word per interval term, and
// out.  The table (at most 8 terms, 48 bytes each) arrives by value with the launch -- nothing is staged, so the call can be captured --
// and every workgroup keeps it in LDS, where the term loop indexes it.  The draws are the per-env body's (wl_event_rand_dev.h).
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_events.h"
#include "wl_kernel_common.h"
#include "wl_event_rand_dev.h"

namespace {

struct EventRandTable {
    EventRandDevTerm t[WL_EVENTRAND_MAX_TERMS];
};

__global__ void __launch_bounds__(kBlock) event_rand_kernel(const EventRandArgs a, const EventRandTable tab) {
    __shared__ EventRandDevTerm t[WL_EVENTRAND_MAX_TERMS];
    layer_table_to_lds(t, tab, a.n_terms);
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.n) return;
    eventrand_env(e, a, t);
}

}  // namespace

extern "C" {

int wl_event_rand_version(void) { return WL_EVENTRAND_VERSION; }

int64_t wl_event_rand_width(const WlEventRandTerm* terms, int32_t n_terms) {
    const int64_t w = eventrand_width(terms, n_terms);
    return w < 0 ? (int64_t)WL_EINVAL : w;
}

int wl_event_rand_apply(int32_t n, float* state, int64_t stride, const WlEventRandTerm* terms, int32_t n_terms, float* block,
                        const uint8_t* reset_a, const uint8_t* reset_b, const uint8_t* mask, uint32_t mask_terms, uint64_t seed,
                        uint64_t step, float step_dt, uint64_t env_offset, void* stream) {
    if (!state || !block || !reset_a || !terms || n < 1 || stride < n) return WL_EINVAL;
    const int64_t rows = eventrand_width(terms, n_terms);
    if (rows < 0) return WL_EINVAL;
    if (stride * 4 * WL_S_COUNT > 0x7fffffffLL) return WL_EINVAL;
    if (n_terms < 32 && (mask_terms >> n_terms) != 0u) return WL_EINVAL;
    if (!(step_dt >= 0.f) || !layer_finite(step_dt)) return WL_EINVAL;
    // what the launch stores (the four constant rows, the block) may touch nothing else it reads or stores
    static_assert(WL_S_MU_D == WL_S_MU_S + 1 && WL_S_DAMP == WL_S_MU_S + 2 && WL_S_MASS == WL_S_MU_S + 3, "the constant rows are adjacent");
    const Span spans[] = {{state + (int64_t)WL_S_MU_S * stride, (3 * stride + n) * 4},
                          {block, ((rows - 1) * stride + n) * 4},
                          {reset_a, n},
                          {reset_b, n},
                          {mask, n}};
    if (any_overlap(spans, 2)) return WL_EINVAL;
    if (stride % 64 != 0 || !aligned(state, 4) || !aligned(block, 4)) return WL_EALIGN;
    EventRandArgs a{};
    a.state = state;
    a.block = (uint32_t*)block;
    a.reset_a = reset_a;
    a.reset_b = reset_b;
    a.mask = mask;
    a.stride = stride;
    a.seed = seed;
    a.step = step;
    a.step_dt = step_dt;
    a.env0 = (uint32_t)env_offset;
    a.mask_terms = mask_terms;
    a.n = n;
    a.n_terms = n_terms;
    EventRandTable tab{};
    for (int k = 0; k < n_terms; ++k) tab.t[k] = eventrand_pack(terms[k]);
    clear_error();
    event_rand_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(a, tab);
    return launch_status();
}

}  // extern "C"

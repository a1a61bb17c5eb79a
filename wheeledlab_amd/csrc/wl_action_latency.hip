// wl_action_latency.hip -- action latency (include/wheeledlab_amd_latency.h) for gfx950: per-env delayed actions as two launches around
// the step launch, which itself is untouched.
//
// One lane per env, no atomics.  Both kernels are data movement: `push` loads its env's 8 action bytes and four words of the layer block,
// stores two ring words (the whole ring on the first push after a reset) and the 8 bytes of `applied`; `finish` loads the flag bytes and
// the action and stores two state words and two row words, or -- on the lanes the step reset, once per episode -- one Philox block and
// four block words.  Every block and state row is component-major, so a wavefront's accesses to a row are 256 consecutive bytes; the
// [n][2] action rows are 512 consecutive bytes per wavefront.  The bodies are the per-env ones of wl_action_latency_dev.h.
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_latency.h"
#include "wl_kernel_common.h"
#include "wl_action_latency_dev.h"

namespace {

__global__ void __launch_bounds__(kBlock) action_latency_push_kernel(const ActLatPushArgs a) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.n) return;
    actlat_push_env(e, a);
}

__global__ void __launch_bounds__(kBlock) action_latency_finish_kernel(const ActLatFinishArgs a) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.n) return;
    actlat_finish_env(e, a);
}

}  // namespace

extern "C" {

int wl_action_latency_version(void) { return WL_ACTLAT_VERSION; }

int64_t wl_action_latency_width(int32_t max_delay) {
    const int64_t w = actlat_width(max_delay);
    return w < 0 ? (int64_t)WL_EINVAL : w;
}

int wl_action_latency_push(int32_t n, const float* action, float* applied, float* block, int64_t stride, int32_t max_delay, void* stream) {
    if (!action || !applied || !block || n < 1 || stride < n) return WL_EINVAL;
    const int64_t rows = actlat_width(max_delay);
    if (rows < 0) return WL_EINVAL;
    if (stride * 4 * rows > 0x7fffffffLL) return WL_EINVAL;
    const Span spans[] = {{applied, (int64_t)n * 8}, {block, ((rows - 1) * stride + n) * 4}, {action, (int64_t)n * 8}};
    if (any_overlap(spans, 2)) return WL_EINVAL;
    if (stride % 64 != 0 || !aligned(action, 4) || !aligned(applied, 4) || !aligned(block, 4)) return WL_EALIGN;
    ActLatPushArgs a{};
    a.action = (const uint32_t*)action;
    a.applied = (uint32_t*)applied;
    a.block = (uint32_t*)block;
    a.stride = stride;
    a.n = n;
    a.max_delay = max_delay;
    clear_error();
    action_latency_push_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(a);
    return launch_status();
}

int wl_action_latency_finish(int32_t n, const float* action, float* state, int64_t stride, float* row, int64_t row_pitch,
                             int32_t last_action_col, float* block, const uint8_t* reset_a, const uint8_t* reset_b, int32_t min_delay,
                             int32_t max_delay, int32_t per_component, int32_t clip_wrapper, uint64_t seed, uint64_t env_offset, void* stream) {
    if (!action || !state || !block || !reset_a || n < 1 || stride < n) return WL_EINVAL;
    const int64_t rows = actlat_width(max_delay);
    if (rows < 0 || min_delay < 0 || min_delay > max_delay) return WL_EINVAL;
    if (stride * 4 * WL_S_COUNT > 0x7fffffffLL) return WL_EINVAL;
    if ((per_component != 0 && per_component != 1) || (clip_wrapper != 0 && clip_wrapper != 1)) return WL_EINVAL;
    if (row_pitch < 1 || last_action_col < -1 || (int64_t)last_action_col > row_pitch - 2) return WL_EINVAL;
    if (last_action_col >= 0 && !row) return WL_EINVAL;
    // what the launch stores (the two action rows of the state, the row, the block) may touch nothing else it reads or stores
    static_assert(WL_S_ACT1 == WL_S_ACT0 + 1, "the last-action rows are adjacent");
    const Span spans[] = {{state + (int64_t)WL_S_ACT0 * stride, (stride + n) * 4},
                          {last_action_col >= 0 ? row : nullptr, (((int64_t)n - 1) * row_pitch + last_action_col + 2) * 4},
                          {block, ((rows - 1) * stride + n) * 4},
                          {action, (int64_t)n * 8},
                          {reset_a, n},
                          {reset_b, n}};
    if (any_overlap(spans, 3)) return WL_EINVAL;
    if (stride % 64 != 0 || !aligned(action, 4) || !aligned(state, 4) || !aligned(block, 4) || (last_action_col >= 0 && !aligned(row, 4))) return WL_EALIGN;
    ActLatFinishArgs a{};
    a.action = action;
    a.state = state;
    a.row = row;
    a.block = (uint32_t*)block;
    a.reset_a = reset_a;
    a.reset_b = reset_b;
    a.stride = stride;
    a.row_pitch = row_pitch;
    a.seed = seed;
    a.env0 = (uint32_t)env_offset;
    a.n = n;
    a.col = last_action_col;
    a.min_delay = min_delay;
    a.max_delay = max_delay;
    a.per_component = per_component;
    a.clip_wrapper = clip_wrapper;
    clear_error();
    action_latency_finish_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(a);
    return launch_status();
}

}  // extern "C"

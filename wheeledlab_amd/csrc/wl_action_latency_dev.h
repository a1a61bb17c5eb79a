// wl_action_latency_dev.h -- the per-env bodies of the action-latency layer (see wl_action_latency.hip and, for the contract,
// include/wheeledlab_amd_latency.h): what one lane (one env) reads, moves, draws and stores in `push` and in `finish`.  A header of its
// own so that tests/host_sim can compile the same code for the host (through the stand-in hip_runtime.h) and hold it against the
// reference.
//
// Actions travel as 32-bit words; the only arithmetic is the clamp of `finish` (clampf of wl_math.h: the instruction the step kernels
// clip the last action with) and the lag draw's one fp32 product.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wheeledlab_amd_latency.h"
#include "wl_layer_common.h"
#include "wl_rng.h"

#pragma clang fp contract(off)

namespace {

static_assert(WL_RS_ACT_LAG == WL_AL_STREAM && WL_AL_STREAM == 20, "the lag draw's stream id is 20");
constexpr int AL_LAG = 0, AL_PUSHES = 2, AL_HEAD = 3, AL_DRAWN = 4, AL_RING = WL_ACTLAT_HEAD_ROWS;

// the rows of the layer block, or -1
WL_HD int64_t actlat_width(int max_delay) {
    return max_delay < 0 || max_delay > WL_ACTLAT_MAX_DELAY ? -1 : (int64_t)AL_RING + 2 * ((int64_t)max_delay + 1);
}

struct ActLatPushArgs {
    const uint32_t* action;     // [n][2], the policy's
    uint32_t* applied;          // [n][2]
    uint32_t* block;            // component-major [width][stride]
    int64_t stride;
    int32_t n, max_delay;
};

struct ActLatFinishArgs {
    const float* action;        // [n][2], the policy's
    float* state;               // component-major [WL_S_COUNT][stride]
    float* row;                 // [n][row_pitch]; not read when col < 0
    uint32_t* block;
    const uint8_t* reset_a;
    const uint8_t* reset_b;     // may be NULL
    int64_t stride, row_pitch;
    uint64_t seed;
    uint32_t env0;              // uint32(env_offset)
    int32_t n, col, min_delay, max_delay, per_component, clip_wrapper;
};

// Env e before the step: the policy's action into the ring, the delayed action out.  Words the caller did not get from these launches
// (a head or a lag beyond the ring) are read as the ring's last slot, so no index leaves the block.
WL_DEV void actlat_push_env(int e, const ActLatPushArgs& a) {
    const int64_t s = a.stride;
    const uint32_t slots = (uint32_t)a.max_delay + 1u;
    uint32_t* B = a.block + e;
    const uint32_t a0 = a.action[2 * (int64_t)e], a1 = a.action[2 * (int64_t)e + 1];
    uint32_t pushes = B[AL_PUSHES * s], head = B[AL_HEAD * s];
    uint32_t lag0 = B[(AL_LAG + 0) * s], lag1 = B[(AL_LAG + 1) * s];
    if (pushes == 0u) {         // the first push after a reset fills the ring
        for (uint32_t k = 0; k < slots; ++k) {
            B[(AL_RING + 2 * (int64_t)k) * s] = a0;
            B[(AL_RING + 2 * (int64_t)k + 1) * s] = a1;
        }
        head = 0u, pushes = 1u;
    } else {
        head = head + 1u < slots ? head + 1u : 0u;
        B[(AL_RING + 2 * (int64_t)head) * s] = a0;
        B[(AL_RING + 2 * (int64_t)head + 1) * s] = a1;
        pushes = pushes < slots ? pushes + 1u : slots;
    }
    B[AL_PUSHES * s] = pushes;
    B[AL_HEAD * s] = head;
    lag0 = lag0 < pushes - 1u ? lag0 : pushes - 1u;
    lag1 = lag1 < pushes - 1u ? lag1 : pushes - 1u;
    const uint32_t s0 = head >= lag0 ? head - lag0 : head + slots - lag0, s1 = head >= lag1 ? head - lag1 : head + slots - lag1;
    // (a lag of 0 reads the word just stored: the same lane's store, in program order)
    a.applied[2 * (int64_t)e] = lag0 == 0u ? a0 : B[(AL_RING + 2 * (int64_t)s0) * s];
    a.applied[2 * (int64_t)e + 1] = lag1 == 0u ? a1 : B[(AL_RING + 2 * (int64_t)s1 + 1) * s];
}

WL_DEV uint32_t actlat_lag(uint32_t w, int min_delay, int span) {
    const int pick = (int)(u01(w) * (float)span);
    return (uint32_t)(min_delay + (pick < span - 1 ? pick : span - 1));
}

// Env e after the step: a reset env forgets its ring and draws its lags again; any other gets the policy's action into the state's
// last-action rows and the row's last_action columns, as the step stores them.
WL_DEV void actlat_finish_env(int e, const ActLatFinishArgs& a) {
    const int64_t s = a.stride;
    uint32_t* B = a.block + e;
    const bool reset = WL_LAYER_RESET(a, e);
    if (reset) {
        const uint32_t drawn = B[AL_DRAWN * s];
        const U4 w = philox_block(a.env0 + (uint32_t)e, (uint64_t)drawn, (uint32_t)WL_RS_ACT_LAG, a.seed);
        const int span = a.max_delay - a.min_delay + 1;
        B[(AL_LAG + 0) * s] = actlat_lag(w.x, a.min_delay, span);
        B[(AL_LAG + 1) * s] = actlat_lag(a.per_component ? w.y : w.x, a.min_delay, span);
        B[AL_PUSHES * s] = 0u;
        B[AL_DRAWN * s] = drawn + 1u;
        return;
    }
    float a0 = a.action[2 * (int64_t)e], a1 = a.action[2 * (int64_t)e + 1];
    if (a.clip_wrapper) {       // process_action (wl_drift_terms.h): the ClipAction wrapper folded into the step
        a0 = clampf(a0, -1.f, 1.f);
        a1 = clampf(a1, -1.f, 1.f);
    }
    a.state[(int64_t)WL_S_ACT0 * s + e] = a0;
    a.state[(int64_t)WL_S_ACT1 * s + e] = a1;
    if (a.col >= 0) {
        float* r = a.row + (int64_t)e * a.row_pitch + a.col;
        r[0] = clampf(a0, -1.f, 1.f);
        r[1] = clampf(a1, -1.f, 1.f);
    }
}

}  // namespace

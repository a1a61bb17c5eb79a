// wl_event_rand_dev.h -- the per-env body of the per-episode domain randomisation (see wl_event_rand.hip and, for the contract,
// include/wheeledlab_amd_events.h): the table check, the packed form of a term, the draws, and what one lane (one env) reads, decides,
// draws and stores.  A header of its own so that tests/host_sim can compile the same code for the host (through the stand-in
// hip_runtime.h) and hold it against the reference.
//
// Roundings are explicit: the library builds with -ffp-contract=fast, and `base * d` followed by `part_base + part_wheels` must be two
// roundings on the device, on the host and in the reference -- so contraction is off from here to the end of the translation unit and
// every fused operation that is meant is an fmaf.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/wheeledlab_amd_events.h"
#include "wl_layer_common.h"
#include "wl_rng.h"

#pragma clang fp contract(off)

namespace {

// a term as the kernel carries it: 48 bytes.  code: bits 0-1 target, 2 mode, 3-4 operation, 5-6 distribution, 7 global time, 8 consistent
struct EventRandDevTerm {
    uint32_t code;
    float a, b, base;               // the draw's two constants (uniform: lo, span; log_uniform: ln lo, ln hi - ln lo; gaussian: mean, std)
    float int_lo, int_span;         // the timer: lo, fp32(hi - lo)
    int32_t min_steps;
    float mu_s_lo, mu_s_span, mu_d_lo, mu_d_span;
    int32_t nb;
};
constexpr uint32_t ER_GLOBAL = 1u << 7, ER_CONSISTENT = 1u << 8;
WL_HD int er_target(uint32_t code) { return (int)(code & 3u); }
WL_HD int er_mode(uint32_t code) { return (int)((code >> 2) & 1u); }
WL_HD int er_op(uint32_t code) { return (int)((code >> 3) & 3u); }
WL_HD int er_dist(uint32_t code) { return (int)((code >> 5) & 3u); }

constexpr int ER_ROWS_HEAD = 2, ER_ROWS_PER_TERM = 4;   // part_base, part_wheels; then time_left, applied, last_step / drawn (two words)

// the validated table -> the rows of the layer block, or -1
WL_HD int64_t eventrand_width(const WlEventRandTerm* t, int n_terms) {
    if (!t || n_terms < 1 || n_terms > WL_EVENTRAND_MAX_TERMS) return -1;
    for (int k = 0; k < n_terms; ++k) {
        const WlEventRandTerm& q = t[k];
        if (q.target < WL_ER_MU || q.target > WL_ER_MASS_WHEELS || q.mode < WL_ER_RESET || q.mode > WL_ER_INTERVAL) return -1;
        if (q.op < WL_ER_ADD || q.op > WL_ER_ABS || q.dist < WL_ER_UNIFORM || q.dist > WL_ER_GAUSSIAN) return -1;
        if (!layer_finite(q.p0) || !layer_finite(q.p1) || !layer_finite(q.base) || !layer_finite(q.interval_lo) || !layer_finite(q.interval_hi)) return -1;
        if (!layer_finite(q.mu_s_lo) || !layer_finite(q.mu_s_hi) || !layer_finite(q.mu_d_lo) || !layer_finite(q.mu_d_hi)) return -1;
        if (q.dist == WL_ER_GAUSSIAN ? q.p1 < 0.f : q.p0 > q.p1) return -1;
        if (q.dist == WL_ER_LOG_UNIFORM && !(q.p0 > 0.f)) return -1;
        if (q.target == WL_ER_MASS_WHEELS && q.op != WL_ER_ABS) return -1;
        if (q.mode == WL_ER_INTERVAL && (q.interval_lo > q.interval_hi || !(q.interval_lo > 0.f))) return -1;
        if ((q.is_global_time != 0 && q.is_global_time != 1) || (q.make_consistent != 0 && q.make_consistent != 1)) return -1;
        if (q.min_step_count_between_reset < 0) return -1;
        if (q.target == WL_ER_MU && (q.num_buckets < 1 || q.mu_s_lo > q.mu_s_hi || q.mu_d_lo > q.mu_d_hi)) return -1;
    }
    return ER_ROWS_HEAD + (int64_t)ER_ROWS_PER_TERM * n_terms;
}

// host: the spans and logarithms are formed here, once (the logarithms in double, rounded to fp32)
inline EventRandDevTerm eventrand_pack(const WlEventRandTerm& q) {
    EventRandDevTerm d;
    d.code = (uint32_t)q.target | ((uint32_t)q.mode << 2) | ((uint32_t)q.op << 3) | ((uint32_t)q.dist << 5) | (q.is_global_time ? ER_GLOBAL : 0u) |
             (q.make_consistent ? ER_CONSISTENT : 0u);
    if (q.dist == WL_ER_UNIFORM) {
        d.a = q.p0, d.b = q.p1 - q.p0;
    } else if (q.dist == WL_ER_LOG_UNIFORM) {
        const double l0 = std::log((double)q.p0), l1 = std::log((double)q.p1);
        d.a = (float)l0, d.b = (float)(l1 - l0);
    } else {
        d.a = q.p0, d.b = q.p1;
    }
    d.base = q.base;
    d.int_lo = q.interval_lo, d.int_span = q.interval_hi - q.interval_lo;
    d.min_steps = q.min_step_count_between_reset;
    d.mu_s_lo = q.mu_s_lo, d.mu_s_span = q.mu_s_hi - q.mu_s_lo;
    d.mu_d_lo = q.mu_d_lo, d.mu_d_span = q.mu_d_hi - q.mu_d_lo;
    d.nb = q.num_buckets;
    return d;
}

// what a launch needs besides the table
struct EventRandArgs {
    float* state;               // component-major [WL_S_COUNT][stride]
    uint32_t* block;            // component-major [2 + 4 n_terms][stride]
    const uint8_t* reset_a;
    const uint8_t* reset_b;     // may be NULL
    const uint8_t* mask;        // may be NULL
    int64_t stride;
    uint64_t seed, step;
    float step_dt;
    uint32_t env0;              // uint32(env_offset)
    uint32_t mask_terms;
    int32_t n, n_terms;
};

WL_DEV float er_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
WL_DEV uint32_t er_as_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// e^x as 2^(x log2 e): v_exp_f32 on the device
WL_DEV float er_exp(float x) {
    const float y = x * 1.44269504088896340736f;
#ifdef WL_HOST_SIM
    return (float)std::exp2((double)y);
#else
    return __builtin_amdgcn_exp2f(y);
#endif
}

// the draw d of a distribution from its word (wheeledlab_amd_events.h)
WL_DEV float eventrand_draw(int dist, float a, float b, uint32_t w) {
    if (dist == WL_ER_GAUSSIAN) {
        float z0, z1;
        box_muller_open(u16_lo(w), u16_hi(w), z0, z1);
        return fmaf(z0, b, a);
    }
    const float x = fmaf(u01(w), b, a);
    return dist == WL_ER_LOG_UNIFORM ? er_exp(x) : x;
}

WL_DEV float eventrand_op(int op, float base, float d) { return op == WL_ER_ADD ? base + d : op == WL_ER_SCALE ? base * d : d; }

WL_DEV float eventrand_timer(uint32_t id, uint32_t drawn, int k, const EventRandDevTerm& q, uint64_t seed) {
    const U4 w = philox_block(id, (uint64_t)drawn, (uint32_t)WL_RS_EVENT_TIMER | ((uint32_t)k << 8), seed);
    return fmaf(u01(w.x), q.int_span, q.int_lo);
}

// Env e of the launch: the reset terms, then the interval terms, each in table order; the constant rows and the mass parts it changed are
// stored at the end, so that of two terms on one target the later one is what the rows hold.
WL_DEV void eventrand_env(int e, const EventRandArgs& a, const EventRandDevTerm* t) {
    const uint32_t env = a.env0 + (uint32_t)e;
    const bool reset = WL_LAYER_RESET(a, e);
    const bool masked = a.mask != nullptr && a.mask[e] != 0;
    const int64_t s = a.stride;
    float mu_s = 0.f, mu_d = 0.f, damp = 0.f, part_base = 0.f, part_wheels = 0.f;
    bool set_mu = false, set_damp = false, set_base = false, set_wheels = false;
    for (int pass = WL_ER_RESET; pass <= WL_ER_INTERVAL; ++pass) {
        for (int k = 0; k < a.n_terms; ++k) {
            const EventRandDevTerm q = t[k];
            if (er_mode(q.code) != pass) continue;
            uint32_t* row = a.block + (int64_t)(ER_ROWS_HEAD + ER_ROWS_PER_TERM * k) * s + e;      // time_left; + s applied; + 2 s, + 3 s the two words
            const bool forced = masked && ((a.mask_terms >> k) & 1u) != 0;
            uint32_t applied;
            if (pass == WL_ER_RESET) {
                if (!(reset || forced)) continue;
                applied = row[s];
                if (!forced && q.min_steps > 0 && applied != 0u) {
                    const uint64_t last = (uint64_t)row[2 * s] | ((uint64_t)row[3 * s] << 32);
                    if (a.step - last < (uint64_t)q.min_steps) continue;
                }
                row[2 * s] = (uint32_t)a.step;
                row[3 * s] = (uint32_t)(a.step >> 32);
            } else {
                const bool global = (q.code & ER_GLOBAL) != 0;
                const uint32_t id = global ? WL_ER_GLOBAL_ID : env;
                const uint32_t tl0 = row[0], drawn0 = row[2 * s];
                float tl = er_as_float(tl0);
                uint32_t drawn = drawn0;
                if (drawn == 0u || (!global && reset)) tl = eventrand_timer(id, drawn++, k, q, a.seed);   // never drawn, or the env's new episode
                tl = tl - a.step_dt;
                const bool fire = tl < 1e-6f;
                if (fire) tl = eventrand_timer(id, drawn++, k, q, a.seed);
                if (er_as_bits(tl) != tl0) row[0] = er_as_bits(tl);
                if (drawn != drawn0) row[2 * s] = drawn;
                if (!(fire || forced)) continue;
                applied = row[s];
            }
            const U4 w = philox_block(env, (uint64_t)applied, (uint32_t)WL_RS_EVENT_VALUE | ((uint32_t)k << 8), a.seed);
            row[s] = applied + 1u;
            const int target = er_target(q.code), op = er_op(q.code), dist = er_dist(q.code);
            if (target == WL_ER_MU) {
                const int pick = (int)(u01(w.x) * (float)q.nb);
                const int bucket = pick < q.nb - 1 ? pick : q.nb - 1;
                const U4 m = philox_block((uint32_t)bucket, 0, (uint32_t)WL_RS_STARTUP_BUCKET, a.seed);   // the bucket's material: the startup path's
                mu_s = fmaf(u01(m.x), q.mu_s_span, q.mu_s_lo);
                mu_d = fmaf(u01(m.y), q.mu_d_span, q.mu_d_lo);
                if (q.code & ER_CONSISTENT) mu_d = fminf(mu_d, mu_s);
                set_mu = true;
            } else if (target == WL_ER_DAMP) {
                damp = eventrand_op(op, q.base, eventrand_draw(dist, q.a, q.b, w.x));
                set_damp = true;
            } else if (target == WL_ER_MASS_BASE) {
                part_base = eventrand_op(op, q.base, eventrand_draw(dist, q.a, q.b, w.x));
                set_base = true;
            } else {
                part_wheels = (eventrand_draw(dist, q.a, q.b, w.x) + eventrand_draw(dist, q.a, q.b, w.y)) +
                              (eventrand_draw(dist, q.a, q.b, w.z) + eventrand_draw(dist, q.a, q.b, w.w));
                set_wheels = true;
            }
        }
    }
    float* S = a.state + e;
    if (set_mu) {
        S[(int64_t)WL_S_MU_S * s] = mu_s;
        S[(int64_t)WL_S_MU_D * s] = mu_d;
    }
    if (set_damp) S[(int64_t)WL_S_DAMP * s] = damp;
    if (set_base || set_wheels) {
        uint32_t* parts = a.block + e;
        if (set_base) parts[0] = er_as_bits(part_base);
        else part_base = er_as_float(parts[0]);
        if (set_wheels) parts[s] = er_as_bits(part_wheels);
        else part_wheels = er_as_float(parts[s]);
        S[(int64_t)WL_S_MASS * s] = part_base + part_wheels;
    }
}

}  // namespace

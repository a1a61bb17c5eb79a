// wl_obs_corrupt_dev.h -- the per-element body of the observation corruption (see wl_obs_corrupt.hip and, for the contract,
// include/wheeledlab_amd_obsnoise.h): the table check, the packed form of a term, the draws, and what one lane (one Philox block: four
// columns of one env) reads, computes and -- for the bias -- stores.  A header of its own so that tests/host_sim can compile the same
// arithmetic for the host (through the stand-in hip_runtime.h) and hold it against the reference.
//
// Roundings are explicit: the library builds with -ffp-contract=fast, and `x * n + bias` must be two roundings on the device, on the
// host and in the reference -- so contraction is off from here to the end of the translation unit and every fused operation that is
// meant is an fmaf.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/wheeledlab_amd_obsnoise.h"
#include "wl_layer_common.h"
#include "wl_rng.h"

#pragma clang fp contract(off)

namespace {

constexpr int OBSCORRUPT_SLOT = 4;   // columns per lane: the four words of one Philox block

// a term as the kernel carries it: 48 bytes, so that 64 of them and the launch's other arguments stay below the 4 KiB a kernel's
// arguments may take.  code: bits 0-1 noise kind, 2-3 operation, 4-5 bias kind, 6 bias per component, 7 scale, 8 clip
struct ObsCorruptDevTerm {
    int32_t off, width;
    uint32_t code;
    float noise_a, noise_b, bias_a, bias_b;
    int32_t bias_off;
    float clip_lo, clip_hi, scale;
    int32_t state_row;
};
constexpr uint32_t OC_PER_COMPONENT = 1u << 6, OC_SCALE = 1u << 7, OC_CLIP = 1u << 8;
WL_HD int oc_noise_kind(uint32_t code) { return (int)(code & 3u); }
WL_HD int oc_op(uint32_t code) { return (int)((code >> 2) & 3u); }
WL_HD int oc_bias_kind(uint32_t code) { return (int)((code >> 4) & 3u); }

WL_HD bool oc_kind_ok(int32_t kind, float a, float b) {
    if (kind < WL_OC_NONE || kind > WL_OC_GAUSSIAN) return false;
    return kind == WL_OC_NONE || (layer_finite(a) && (kind == WL_OC_CONSTANT || layer_finite(b)));
}

// the validated table -> Db, the floats of bias per env, or -1
WL_HD int64_t obscorrupt_width(const WlObsCorruptTerm* t, int n_terms, int D) {
    if (!t || n_terms < 1 || n_terms > WL_OBSCORRUPT_MAX_TERMS || D < 1 || D > WL_OBSCORRUPT_MAX_DIM) return -1;
    int64_t off = 0, bias = 0;
    for (int k = 0; k < n_terms; ++k) {
        const WlObsCorruptTerm& q = t[k];
        if (q.width < 1 || q.width > D || q.off != off) return -1;
        if (!oc_kind_ok(q.noise_kind, q.noise_a, q.noise_b) || !oc_kind_ok(q.bias_kind, q.bias_a, q.bias_b)) return -1;
        if (q.noise_op < WL_OC_ADD || q.noise_op > WL_OC_ABS) return -1;
        if (q.bias_kind != WL_OC_NONE && q.noise_kind == WL_OC_NONE) return -1;
        if (q.bias_per_component != 0 && q.bias_per_component != 1) return -1;
        if (q.bias_off != bias) return -1;
        if (!(q.clip_lo <= q.clip_hi)) return -1;                       // (a NaN bound fails the comparison)
        if (!layer_finite(q.scale) || (q.has_scale != 0 && q.has_scale != 1) || (!q.has_scale && q.scale != 1.f)) return -1;
        off += q.width;
        if (q.bias_kind != WL_OC_NONE) bias += q.bias_per_component ? q.width : 1;
    }
    return off == D ? bias : -1;
}

WL_HD ObsCorruptDevTerm obscorrupt_pack(const WlObsCorruptTerm& q) {
    ObsCorruptDevTerm d;
    d.off = q.off;
    d.width = q.width;
    d.code = (uint32_t)q.noise_kind | ((uint32_t)q.noise_op << 2) | ((uint32_t)q.bias_kind << 4) | (q.bias_per_component ? OC_PER_COMPONENT : 0u) |
             (q.has_scale ? OC_SCALE : 0u) | ((q.clip_lo > -INFINITY || q.clip_hi < INFINITY) ? OC_CLIP : 0u);
    d.noise_a = q.noise_a, d.noise_b = q.noise_b, d.bias_a = q.bias_a, d.bias_b = q.bias_b;
    d.bias_off = q.bias_off;
    d.clip_lo = q.clip_lo, d.clip_hi = q.clip_hi, d.scale = q.scale;
    d.state_row = q.state_row < 0 ? -1 : q.state_row;
    return d;
}

// what a launch needs besides the table
struct ObsCorruptArgs {
    const uint32_t* obs;
    const uint32_t* state;      // component-major [rows][state_stride]; NULL without a state_row term
    float* bias;                // [n][Db]; NULL with Db == 0
    const uint8_t* reset_a;
    const uint8_t* reset_b;     // may be NULL
    int64_t obs_stride, state_stride;
    uint64_t seed, step;
    uint32_t env0;              // uint32(env_offset)
    int32_t n, D, Db, n_terms;
    int32_t nblk;               // (D + 3) / 4: Philox blocks (lanes) per env
    int32_t lanes;              // n * nblk < 2^31
    int32_t enable;
};

// the term of column c: the last k with off_k <= c, six halvings over at most 64 entries
WL_DEV int obscorrupt_seek(int c, const ObsCorruptDevTerm* t, int n_terms) {
    int k = 0;
#pragma unroll
    for (int step = WL_OBSCORRUPT_MAX_TERMS / 2; step > 0; step >>= 1) {
        const int m = k + step;
        if (m < n_terms && t[m].off <= c) k = m;
    }
    return k;
}

WL_DEV uint32_t oc_word(const U4& b, int i) { return i == 0 ? b.x : i == 1 ? b.y : i == 2 ? b.z : b.w; }

// the draw d of a kind from its word (wheeledlab_amd_obsnoise.h)
WL_DEV float obscorrupt_draw(int kind, float a, float b, uint32_t w) {
    if (kind == WL_OC_UNIFORM) return fmaf(u01(w), b, a);
    if (kind == WL_OC_GAUSSIAN) {
        float z0, z1;
        box_muller_open(u16_lo(w), u16_hi(w), z0, z1);
        return fmaf(z0, b, a);
    }
    return a;
}

// clip (a NaN fails both comparisons and stays), then scale
WL_DEV float obscorrupt_clip_scale(float y, const ObsCorruptDevTerm& q) {
    if (q.code & OC_CLIP) {
        y = y < q.clip_lo ? q.clip_lo : y;
        y = y > q.clip_hi ? q.clip_hi : y;
    }
    if (q.code & OC_SCALE) y = y * q.scale;
    return y;
}

WL_DEV float oc_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
WL_DEV uint32_t oc_as_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Lane `lane` of the launch: env e = lane / nblk, columns c0 = 4 (lane % nblk) .. c0 + count - 1 of its row.  x[0 .. count) hold the words
// of obs[e][c0 ..] on entry (the caller loads them as wide as the address allows; columns of a state_row term are read here instead);
// v[0 .. count) are the words of out[e][c0 ..].  A bias element of a resetting env is drawn and stored here, by the lane whose column owns it.
WL_DEV void obscorrupt_lane(int e, int c0, int count, const ObsCorruptArgs& a, const ObsCorruptDevTerm* t, const uint32_t (&x)[OBSCORRUPT_SLOT],
                            uint32_t (&v)[OBSCORRUPT_SLOT]) {
    const uint32_t env = a.env0 + (uint32_t)e;
    const uint32_t blk = (uint32_t)c0 >> 2;
    const bool reset = WL_LAYER_RESET(a, e);
    int k = obscorrupt_seek(c0, t, a.n_terms);
    U4 wn{}, wb{};
    bool have_n = false;
    uint32_t have_b = 0xFFFFFFFFu;          // the block of the bias stream `wb` holds
#pragma unroll
    for (int i = 0; i < OBSCORRUPT_SLOT; ++i) {
        if (i >= count) break;
        const int c = c0 + i;
        while (c >= t[k].off + t[k].width) ++k;
        const ObsCorruptDevTerm q = t[k];
        const int j = c - q.off;
        const uint32_t xb = q.state_row >= 0 ? a.state[(int64_t)(q.state_row + j) * a.state_stride + e] : x[i];
        const int kind = a.enable ? oc_noise_kind(q.code) : WL_OC_NONE;
        if (kind == WL_OC_NONE && !(q.code & (OC_CLIP | OC_SCALE))) {
            v[i] = xb;                        // untouched: bits in, bits out
            continue;
        }
        float y = oc_as_float(xb);
        if (kind != WL_OC_NONE) {
            if (kind != WL_OC_CONSTANT && !have_n) {
                wn = philox_block(env, a.step, (uint32_t)WL_RS_OBS_NOISE | (blk << 8), a.seed);
                have_n = true;
            }
            const float d = obscorrupt_draw(kind, q.noise_a, q.noise_b, oc_word(wn, i));
            const int op = oc_op(q.code);
            y = op == WL_OC_ADD ? y + d : op == WL_OC_SCALE ? y * d : (y != y ? y : d);   // abs: the draw alone -- but a NaN in stays a NaN
            const int bkind = oc_bias_kind(q.code);
            if (bkind != WL_OC_NONE) {
                const bool per = (q.code & OC_PER_COMPONENT) != 0;
                float* slot = a.bias + (int64_t)e * a.Db + q.bias_off + (per ? j : 0);
                float bv;
                if (reset) {
                    const int bc = per ? c : q.off;                 // the column whose word the element is drawn from
                    if (bkind != WL_OC_CONSTANT && have_b != ((uint32_t)bc >> 2)) {
                        have_b = (uint32_t)bc >> 2;
                        wb = philox_block(env, a.step, (uint32_t)WL_RS_OBS_BIAS | (have_b << 8), a.seed);
                    }
                    bv = obscorrupt_draw(bkind, q.bias_a, q.bias_b, oc_word(wb, bc & 3));
                    if (bc == c) *slot = bv;                         // its owner stores it; the term's other columns only use it
                } else {
                    bv = *slot;
                }
                y = y + bv;
            }
        }
        v[i] = oc_as_bits(obscorrupt_clip_scale(y, q));
    }
}

}  // namespace

// wl_visual_cam_dev.h -- the visual task's camera: the 3208-dim observation of ONE env by a group of threads.  3200 camera rays
// against the z = 0 plane with a traversability-map lookup each; the 40 x 80 image is staged in LDS (12.8 KB) so that the contrast
// mean (group reduction) and the separable 5x5 Gaussian blur never leave the CU; the row is written once with contiguous dword
// stores -- 12.8 KB / env, ~98 % of the task's HBM bytes.  The kernels that call render_image (block = env, and the render groups of
// the persistent rollout) are in wl_visual.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_visual_env.h"   // CamPose

namespace {

constexpr int kImgH = WL_VIS_IMG_H - WL_VIS_CROP, kImgW = WL_VIS_IMG_W;
// threads that render one image (whole wavefronts, whole image rows per pass)
#ifndef WL_CAM_THREADS
#define WL_CAM_THREADS 256
#endif
constexpr int kCam = WL_CAM_THREADS;

// render-path lookup: map_id's cell function (wl_visual_env.h) with reciprocal spacing (the camera is designed, not parity-pinned)
struct MapFast {
    float off_x, off_y, inv_rs, inv_cs, half_w, half_h;
};
WL_DEV MapFast map_fast(const WlTravMap& m) {
    const float width = (float)m.rows * m.row_spacing, height = (float)m.cols * m.col_spacing;
    return MapFast{0.5f * width + 0.5f * m.row_spacing, 0.5f * height + 0.5f * m.col_spacing, rcp(m.row_spacing),
                   rcp(m.col_spacing), 0.5f * width, 0.5f * height};
}

// (BlockSync / GroupSync -- how the wavefronts that render one image meet -- are in wl_kernel_common.h)
// sum over the GT threads (whole wavefronts) that render one image
template <int GT, class SYNC>
WL_DEV float group_sum(float v, float* scratch /* [GT / 64], this group's */, int gt, SYNC& sync) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    sync();
    if ((gt & 63) == 0) scratch[gt >> 6] = v;
    sync();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < GT / 64; ++w) t += scratch[w];
    return t;
}

// how a pixel's map cell is read: a byte gather from the global map, or one bit of the LDS-resident copy of the whole map
// (WlTravMap.bits: the camera's 3200 divergent byte gathers per image were what bound it -- one lane per cycle and CU through
// the texture addresser; an LDS read costs a thirty-second of that)
// `masked(k, on)`: the cell, or false for a pixel that is off the map.  Global form (round 6): the byte map through a buffer resource
// -- a 32-bit lane offset instead of a 64-bit address (v_mad_u64_u32 + v_lshl_add_u64 per pixel went), and an off-map pixel asks for
// an offset outside the buffer (the bounds check returns 0 = not traversable) instead of branching around its gather: with the branch
// the compiler waited for every pixel's gather inside it (`s_waitcnt vmcnt(0)` fourteen times per lane), now a lane's fourteen are in
// flight together as the loop was written for.
struct GlobalMapLookup {
    __amdgpu_buffer_rsrc_t rsrc;
    WL_DEV explicit GlobalMapLookup(const WlTravMap& m)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(m.map), 0, m.rows * m.cols, 0x00020000)) {}
    WL_DEV bool masked(int k, bool on) const { return __builtin_amdgcn_raw_buffer_load_b8(rsrc, on ? k : -1, 0, 0) != 0; }
};
struct LdsBitLookup {
    const uint32_t* bits;
    WL_DEV bool masked(int k, bool on) const {
        const int kk = on ? k : 0;
        return on && ((bits[kk >> 5] >> (kk & 31)) & 1u);
    }
};
constexpr int kMapWords = WL_VIS_LDS_MAP_CELLS / 32;   // 32 KB of LDS
// all threads of the block copy the bit map into LDS (coalesced dwords; the caller syncs).  Every request of a thread is issued
// before the first LDS write (rolled, the copy was a chain of ~10 dependent L2 round trips per block: slower than the gathers
// it replaces).
template <int THREADS>
WL_DEV void stage_map_bits(const WlTravMap& m, uint32_t* lds) {
    constexpr int kPer = (kMapWords + THREADS - 1) / THREADS;
    const int n_words = (m.rows * m.cols + 31) >> 5;
    uint32_t w[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int idx = (int)threadIdx.x + k * THREADS;
        w[k] = idx < n_words ? m.bits[idx] : 0u;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int idx = (int)threadIdx.x + k * THREADS;
        if (idx < kMapWords) lds[idx] = w[k];
    }
}

WL_DEV int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// the rendered image with its two reflected border columns on either side: pitch 84 floats = 21 sixteen-byte slots, so
// the 8-float window of a 4 x 4 output patch is two aligned ds_read_b128 and, 4 rows x 21 slots being 4 mod 16, the 16-lane
// groups a b128 read is served in (lanes of one patch row + 8 lanes of the next) hit 16 distinct slots.  (With the
// unpadded [40][80] image each of the 64 reads per thread was a 4-byte read at a lane stride of 4 floats: 8-way conflicts.)
constexpr int kPitch = kImgW + 4, kImgPix = kImgH * kPitch, kImgFloats = kImgPix + 8;   // + the blur's five tap weights (render_image)

// VisualObsCfg.PolicyCfg (:38-58): camera (3200) | base_lin_vel (3) | base_ang_vel (3) | last_action clip +-1 (2) of ONE env,
// by a group of GT threads (gt = thread in the group; `img` [kImgFloats] and `red` [GT / 64] are the group's LDS).  Two
// `sync()`s inside when the augmentation needs the whole image; a group without an env (`valid` false) renders its
// neighbour's pose and stores nothing.
// STREAM: the observation block is far larger than the caches (> 256 MB of rows per launch): non-temporal row stores
template <int GT, bool STREAM = false, class SYNC, class LOOKUP>
WL_DEV void render_image(const WlVisualParams& p, const WlTravMap& m, const LOOKUP& lookup, const CamPose& cp, float* __restrict__ row,
                         float* img, float* red, const int gt, const bool valid, SYNC& sync) {
    const V3 pos = v3(cp.px, cp.py, cp.pz);
    const Quat q{cp.qw, cp.qx, cp.qy, cp.qz};
    const Mat3 R = mat_from_quat(q);
    const V3 o = pos + mul(R, v3(p.cam_pos[0], p.cam_pos[1], p.cam_pos[2]));
    const MapFast mf = map_fast(m);
    const float inv_fx = rcp(p.fx), inv_fy = rcp(p.fy);
    const bool plain = p.contrast == 1.f && !(p.blur_sigma > 0.f);   // no augmentation that needs the whole image
    // torchvision draws the order of ColorJitter's ops per call: contrast before brightness when set (only matters with a blend)
    const bool cfirst = p.contrast_first != 0 && p.contrast != 1.f;
    // proprioception: the last lane (its wave renders the fewest pixels)
    if (gt == GT - 1 && valid) store_proprio(row + WL_VIS_NPIX, R, v3(cp.vx, cp.vy, cp.vz), v3(cp.wx, cp.wy, cp.wz), cp.a0, cp.a1);
    // ---- render: one ray per pixel against the z = 0 plane.  d = R (1, dy(col), dz(row)) ----
    const V3 c0 = v3(R.r0.x, R.r1.x, R.r2.x), c1 = v3(R.r0.y, R.r1.y, R.r2.y), c2 = v3(R.r0.z, R.r1.z, R.r2.z);
    float part = 0.f;
    // Thread -> one image column and every third row (GT = 256: 240 of the threads, 3 rows x 80 columns per pass, 14 passes):
    // the ray direction then advances by a constant vector per pass (3 adds instead of 2 conversions + 8 fma), and the
    // lanes of a wavefront still store consecutive columns.  Software-pipelined like the height scan: every pixel of
    // this lane computes its map cell and issues its byte gather first (14 in flight per lane), then all are shaded and
    // stored -- rolled, each pixel paid the gather latency in turn.
    constexpr int kRowsPerPass = GT / kImgW, kIter = (kImgH + kRowsPerPass - 1) / kRowsPerPass;
    const int tc = gt % kImgW, tr = gt / kImgW;
    const bool lane_on = tr < kRowsPerPass;
    const float dy = -(((float)tc + 0.5f - p.cx) * inv_fx), dz0 = -(((float)(tr + WL_VIS_CROP) + 0.5f - p.cy) * inv_fy);
    V3 d = fma3(dz0, c2, fma3(dy, c1, c0));
    // (a product of its own: under -ffp-contract=fast a bare product feeding the `d + dstep` below is fused into that add per
    // instantiation -- the block = env kernel and the persistent kernel then disagree in the last bit of a ray direction and, one
    // image in 20 000, about the map cell a pixel falls into)
    const float kstep = -(float)kRowsPerPass * inv_fy;
    const V3 dstep = v3(fmaf(kstep, c2.x, 0.f), fmaf(kstep, c2.y, 0.f), fmaf(kstep, c2.z, 0.f));
    const float mx = mf.off_x * mf.inv_rs, my = mf.off_y * mf.inv_cs;   // cell = (int)(h * inv + off * inv)
    bool cell[kIter];
    bool hit[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const float t = -o.z * rcp(fminf(d.z, -1e-6f));
        const float hx = fmaf(t, d.x, o.x), hy = fmaf(t, d.y, o.y);
        hit[it] = d.z < -1e-6f;                                         // else: sky
        const bool on_map = hit[it] && fabsf(hx) <= mf.half_w && fabsf(hy) <= mf.half_h;
        // on the map |h| <= half extent, so h * inv + (n / 2 + 0.5) lies in [0.5, n + 0.5]: the conversion truncates, only the upper
        // clamp can bind (off the map the index is not used); 24-bit multiply (full rate; rows, cols < 2^23)
        const int xi = min((int)fmaf(hx, mf.inv_rs, mx), m.rows - 1);
        const int yi = min((int)fmaf(hy, mf.inv_cs, my), m.cols - 1);
        cell[it] = lookup.masked(__mul24(yi, m.cols) + xi, on_map);     // white path on black (utils/__init__.py:47-50)
        d = d + dstep;
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int r = tr + it * kRowsPerPass;
        if (lane_on && r < kImgH) {
            float v = hit[it] ? (cell[it] ? 1.f : 0.f) : p.sky;
            if (!cfirst) v = clampf(v * p.brightness, 0.f, 1.f);       // ColorJitter brightness (before the contrast blend)
            if (plain) {
                if (valid) {   // grayscale + Normalize([0.5], [0.5]) straight to HBM
                    if constexpr (STREAM) __builtin_nontemporal_store((v * 0.9999f - 0.5f) * 2.f, row + r * kImgW + tc);
                    else row[r * kImgW + tc] = (v * 0.9999f - 0.5f) * 2.f;
                }
            } else {
                img[r * kPitch + 2 + tc] = v;      // (the two border columns on either side stay unwritten: the edge patches reflect when they read)
                part += v;
            }
        }
    }
    if (plain) return;
    // ---- augmentation on the LDS-resident image.  One 4 x 4 output patch per thread (10 x 20 patches = 200 threads):
    // the 8 x 8 input neighbourhood is read once (contrast blend applied on the fly), both passes of the separable 5-tap
    // Gaussian run in registers, and each patch row leaves as one 16-byte store.
    // GaussianBlur(5, sigma), torchvision's kernel1d: the five exponentials once per image (lanes 0 - 4, through LDS) instead of once per
    // thread -- with the division and the normalisation they were 100 vector instructions + 11 quarter-rate ones of every thread's ~1000,
    // in a launch that is bound by vector issue (round 6).  Same operations on the same values: same bits.
    float* wl = img + kImgPix;
    if (gt < 5 && p.blur_sigma > 0.f) {
        const float x = (float)(gt - 2) / p.blur_sigma;
        wl[gt] = __expf(-0.5f * x * x);
    }
    const float mean = 0.9999f * group_sum<GT>(part, red, gt, sync) * (1.f / (float)(kImgH * kImgW));   // also orders the img / weight writes
    const float cc = p.contrast, cm = (1.f - p.contrast) * mean;   // ColorJitter contrast: blend with the grey mean
    // a blend TOWARDS the mean (contrast <= 1) stays inside [0, 1], its clamp is the identity, and the blur is linear with
    // weights summing to one: blur(cc v + cm) = cc blur(v) + cm -- applied to the 16 outputs instead of the 64 inputs
    const bool fold = cc <= 1.f && cc >= 0.f && !cfirst;   // (contrast first: the brightness clamp sits between blend and blur)
    const float oc_ = fold ? cc : 1.f, om_ = fold ? cm : 0.f;
    float w[5] = {0.f, 0.f, 1.f, 0.f, 0.f};
    if (p.blur_sigma > 0.f) {
        float wsum = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            w[j] = wl[j];
            wsum += w[j];
        }
        const float inv = 1.f / wsum;
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] *= inv;
    }
    constexpr int kPatchCols = kImgW / 4, kPatches = (kImgH / 4) * kPatchCols;
    if (gt < kPatches && valid) {
        const int pr = (gt / kPatchCols) * 4, pc = (gt % kPatchCols) * 4;
        // reflect padding (torchvision) of the columns, at READ time: only the first and last patch of a row see columns outside the
        // image (-2 -> 2, -1 -> 1; 80 -> 78, 81 -> 77), four selects per row for them -- written at render time the four border
        // columns cost every pixel of every thread two compound tests and two predicated LDS writes (round 6: ~110 instructions per thread)
        const bool left = pc == 0, right = pc == kImgW - 4;
        float hrow[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4* line = reinterpret_cast<const float4*>(img + reflect(pr + i - 2, kImgH) * kPitch + pc);   // columns pc - 2 .. pc + 5
            const float4 lo4 = line[0], hi4 = line[1];
            float v[8] = {left ? hi4.x : lo4.x, left ? lo4.w : lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, right ? hi4.x : hi4.z, right ? lo4.w : hi4.w};
            if (!fold) {   // contrast > 1 can leave [0, 1]: the clamp sits between the blend and the blur
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = clampf(fmaf(cc, v[j], cm), 0.f, 1.f);
                if (cfirst) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = clampf(v[j] * p.brightness, 0.f, 1.f);
                }
            }
#pragma unroll
            for (int o = 0; o < 4; ++o)
                hrow[i][o] = fmaf(w[0], v[o], fmaf(w[1], v[o + 1], fmaf(w[2], v[o + 2], fmaf(w[3], v[o + 3], w[4] * v[o + 4]))));
        }
#pragma unroll
        for (int orow = 0; orow < 4; ++orow) {
            float4 out4;
            float* o4 = reinterpret_cast<float*>(&out4);
#pragma unroll
            for (int oc = 0; oc < 4; ++oc) {
                const float g = fmaf(w[0], hrow[orow][oc], fmaf(w[1], hrow[orow + 1][oc], fmaf(w[2], hrow[orow + 2][oc],
                                fmaf(w[3], hrow[orow + 3][oc], w[4] * hrow[orow + 4][oc]))));
                o4[oc] = (fmaf(oc_, g, om_) * 0.9999f - 0.5f) * 2.f;   // (folded contrast,) grayscale + Normalize([0.5], [0.5])
            }
            // row base = e * 3208 floats = e * 12832 B (16-B aligned), patch column is a multiple of 4 floats
            if constexpr (STREAM) {
                typedef float wl_f4v __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(wl_f4v{out4.x, out4.y, out4.z, out4.w}, reinterpret_cast<wl_f4v*>(row + (pr + orow) * kImgW + pc));
            } else {
                *reinterpret_cast<float4*>(row + (pr + orow) * kImgW + pc) = out4;
            }
        }
    }
}

WL_DEV CamPose load_cam_pose(const Rows& S, const int e) {
    return CamPose{S.ld(WL_S_PX, e), S.ld(WL_S_PX + 1, e), S.ld(WL_S_PX + 2, e), S.ld(WL_S_QW, e), S.ld(WL_S_QX, e),
                   S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e), S.ld(WL_S_VX, e), S.ld(WL_S_VX + 1, e), S.ld(WL_S_VX + 2, e),
                   S.ld(WL_S_WX, e), S.ld(WL_S_WX + 1, e), S.ld(WL_S_WX + 2, e), S.ld(WL_S_ACT0, e), S.ld(WL_S_ACT1, e)};
}

}  // namespace

// wl_visual.hip -- visual task (wheeledlab_tasks/visual/mushr_visual_env_cfg.py) for gfx950: the kernels, their launches and the
// C entry points.  One env's step is in wl_visual_env.h, the camera in wl_visual_cam_dev.h.
//
// Two launches per env.step() (ONE for K steps of an open-loop rollout: visual_rollout_persistent_kernel):
//   1. visual_step_kernel (lane = env): visual_env_step.
//   2. visual_obs_kernel  (block = env): the 3208-dim observation, render_image.
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_visual_env.h"
#include "wl_visual_cam_dev.h"

namespace {

// The visual-depth step's quad form at <= 8192 envs: QB = 128 physics threads + a helper wavefront that draws the block's resets
// (on the plane the draw is one round trip shorter and the helper bought nothing: visual env.step 35.4 against 35.2 us, same box).
constexpr int kHelperQB = 128, kHelperThreads = kHelperQB + 64;
template <int LANES, int QB = kBlock /* quad form: threads per block (see drift_step_kernel) */, class Ground = FlatGround>
__global__ void __launch_bounds__(kBlock) visual_step_kernel(const WlVisualParams p_arg, const VehDerived vd_arg, const WlEnvBuffers b,
                                                             const WlTravMap m, const float2* __restrict__ actions,
                                                             const WlStepOut out, const uint64_t seed, const uint64_t step,
                                                             const Ground ground = Ground{}, const int prop_stride = 0, const int prop_offset = 0) {
    __shared__ float blk_metrics[WL_M_COUNT];
    WlVisualParams p = p_arg;
    VehDerived vd = vd_arg;
    if constexpr (LANES == 4) visual_kernarg_copy(p, vd, p_arg, vd_arg);
    constexpr int kEnvs = (LANES == 4 ? QB : kBlock) / LANES;
    constexpr bool kHelper = LANES == 4 && QB == kHelperQB && !Ground::kFlat;
    __shared__ ResetHelper<VisReset, kHelper ? kEnvs : 1> resets;
    const int wid = LANES == 1 ? 0 : (threadIdx.x & 3);
    const bool lead = LANES == 1 || wid == 0;
    const int e = blockIdx.x * kEnvs + threadIdx.x / LANES;
    if (threadIdx.x < WL_M_COUNT) blk_metrics[threadIdx.x] = 0.f;
    if constexpr (kHelper) resets.init();
    const int m_slot = b.metrics_slots > 1 ? (int)(step % (uint64_t)b.metrics_slots) : 0;
    if (b.metrics_slots > 1) clear_metric_slot(b, (m_slot + 1) % b.metrics_slots);
    __syncthreads();
    const Rows S = make_rows(b.state, b.stride);
    // the helper's part: the wavefront behind the physics threads -- or, in a launch without it (block-uniform test), wavefront 0
    // ahead of its physics: the same draws, and no second copy of them in the kernel
    if constexpr (kHelper) {
        const int helper0 = blockDim.x >= kHelperThreads ? QB : 0;
        if ((unsigned)((int)threadIdx.x - helper0) < 64u) {
            const int j = (int)threadIdx.x - helper0, ej = blockIdx.x * kEnvs + j;
            resets.publish(j, j < kEnvs && ej < b.n_envs,
                           [&] { return visual_reset_pose(p_arg, m, ground, (uint32_t)(b.env_offset + ej), step, seed); });
        }
    }
    if ((!kHelper || threadIdx.x < QB) && e < b.n_envs) {
        VehRows<LANES> rows = load_veh_rows<LANES>(S, e, wid);
        const HelperReset<VisReset, kHelper ? kEnvs : 1> reset_src{&resets, (int)(blockIdx.x * kEnvs), kHelper};
        visual_env_step<LANES, Ground>(p, vd, b, m, actions[e], rows, out, seed, step, S, e, wid, lead, blk_metrics, ground,
                                       prop_stride > 0 ? out.obs + (int64_t)e * prop_stride + prop_offset : nullptr, reset_src);
    }
    __syncthreads();
    block_metrics_flush(blk_metrics, b, m_slot);   // threads 0..15 = wavefront 0 of the block
}

// block = env: the observation of the state as it stands (reset / first observation / lane-form steps); map cells by byte
// gathers from global memory (maps too large for LDS, or no bit map supplied)
// MINW = 7: seven wavefronts per SIMD (72 VGPRs + 24 bytes of scratch) instead of the six that the free allocation (73 -> 80 VGPRs)
// allows -- round 4, env.step() in us at 4096 / 65 536 / 262 144 envs: 49.2 -> 49.0 / 415.5 -> 400 / 1606 -> 1543 (eight, 64 VGPRs + 40
// bytes: 49.6 / 408 / 1614).  The small launches keep the free allocation: nothing to win there, and their scratch rows reach the fabric
// (counter traffic of the 4096-env step 1.19 -> 1.40 x algorithmic).
#ifndef WL_CAM_MIN_WAVES
#define WL_CAM_MIN_WAVES 7
#endif
#ifndef WL_CAM_MIN_WAVES_ENVS
#define WL_CAM_MIN_WAVES_ENVS 32768
#endif
template <bool STREAM, int MINW = 1>
__global__ void __launch_bounds__(kCam, MINW) visual_obs_kernel(const WlVisualParams p, const WlEnvBuffers b, const WlTravMap m,
                                                                float* __restrict__ obs) {
    __shared__ __attribute__((aligned(16))) float img[kImgFloats];
    __shared__ float red[kCam / 64];
    const int e = blockIdx.x;
    const CamPose cp = load_cam_pose(make_rows(b.state, b.stride), e);
    BlockSync sync;
    render_image<kCam, STREAM>(p, m, GlobalMapLookup(m), cp, obs + (int64_t)e * WL_VIS_OBS_DIM, img, red, (int)threadIdx.x, true, sync);
}
// (Round 3: the same camera with the whole map in LDS as one bit per cell -- persistent blocks of three render groups, map staged
// once per block -- measured SLOWER than the byte gathers at 4096 envs: 26.1 against 18.2 us plain, 38.3 against 28.1 us
// augmented.  The gathers were not what bound it: 52.6 MB of observation rows in 18 us are 2.9 TB/s of stores, and the LDS form
// gives up a quarter of the resident wavefronts for its 32 KB.  In the persistent rollout below, where the blocks are resident
// for the whole rollout anyway, the LDS map does pay: 29.0 -> 26.0 us per step plain, 37.5 -> 35.9 augmented.)

// K env.step()s in ONE launch with pre-staged actions [K][n][2] (open-loop rollouts; quad form, n <= 32 768), the visual
// counterpart of elev_rollout_persistent_kernel.  Block = 16 envs, 1024 threads.  Wavefront 0 steps them (through the
// state rows, which stay in this CU's cache: the camera, not the physics, is the longer leg here) and leaves each step's
// poses in one of two LDS buffers; the other twelve wavefronts -- three groups of GT = 256 threads, one image per group
// and pass -- render step k WHILE wavefront 0 already integrates step k + 1.  One s_barrier per step and wavefront; the
// render groups meet among themselves through GroupSync.  Episode metrics of all K steps go to ring slot `slots.cur`.
// (GT is visual_obs_kernel's: a group of 320 threads -- 4 image rows per pass, fifteen render wavefronts -- advances the
// ray direction in different increments, and rays that graze a cell edge then resolve differently: not bit-identical.)
constexpr int kPersistGroups = (1024 - 64) / kCam, kPersistThreads = 64 + kPersistGroups * kCam;
template <int EPB, bool LDSMAP>
__global__ void __launch_bounds__(kPersistThreads) visual_rollout_persistent_kernel(
    const WlVisualParams p_arg, const VehDerived vd_arg, const WlEnvBuffers b, const WlTravMap m, const float2* __restrict__ actions,
    const WlStepOut out, const int64_t obs_step_stride, const int64_t vec_step_stride, const int n_steps, const uint64_t seed,
    const uint64_t step0, const MetricSlots slots) {
    constexpr int GT = kCam, kGroups = kPersistGroups, kPasses = (EPB + kGroups - 1) / kGroups;
    static_assert(GT % 64 == 0 && GT >= kImgW && kGroups >= 1 && 4 * EPB <= 64, "whole wavefronts per render group; one physics wavefront");
    __shared__ float blk_metrics[WL_M_COUNT];
    __shared__ CamPose pose[2][EPB];
    __shared__ __attribute__((aligned(16))) float img[kGroups * kImgFloats];
    __shared__ float red[kGroups * (GT / 64)];
    __shared__ int arrivals[kGroups];
    __shared__ uint32_t mapbits[LDSMAP ? kMapWords : 1];
    const int tid = threadIdx.x;
    if (tid < WL_M_COUNT) blk_metrics[tid] = 0.f;
    if (tid < kGroups) arrivals[tid] = 0;
    if (b.metrics_slots > 1) clear_metric_slot(b, slots.next);
    if constexpr (LDSMAP) stage_map_bits<kPersistThreads>(m, mapbits);
    __syncthreads();
    const int e0 = blockIdx.x * EPB;
    if (tid < 64) {
        const int wid = tid & 3, e = e0 + (tid >> 2);
        const bool valid = tid < 4 * EPB && e < b.n_envs;
        const Rows S = make_rows(b.state, b.stride);
        WlVisualParams p;
        VehDerived vd;
        visual_kernarg_copy(p, vd, p_arg, vd_arg);
#pragma unroll 1
        for (int k = 0; k < n_steps; ++k) {
            if (valid) {
                const WlStepOut o = step_out_at(out, k, obs_step_stride, vec_step_stride);
                const float2 a = actions[(int64_t)k * b.n_envs + e];
                VehRows<4> rows = load_veh_rows<4>(S, e, wid);
                const CamPose cp = visual_env_step<4>(p, vd, b, m, a, rows, o, seed, step0 + (uint64_t)k, S, e, wid, wid == 0, blk_metrics);
                if (wid == 0) pose[k & 1][tid >> 2] = cp;
            }
            __syncthreads();   // barrier k: the poses of step k are published
        }
        block_metrics_flush(blk_metrics, b, slots.cur);   // only this wavefront accumulated
        return;
    }
    // ---- the other wavefronts: the camera of step k, one step behind the physics ----
    const int t = tid - 64, grp = t / GT, gt = t % GT;
    const int n_here = min(EPB, b.n_envs - e0);
    const bool plain = p_arg.contrast == 1.f && !(p_arg.blur_sigma > 0.f);
    GroupSync sync{arrivals + min(grp, kGroups - 1), 0, GT / 64};
#pragma unroll 1
    for (int k = 0; k < n_steps; ++k) {
        __syncthreads();       // barrier k (also: every group is done with its previous image)
        if (grp >= kGroups) continue;   // wavefronts left over when the block is no whole number of groups
        float* obs_k = out.obs + k * obs_step_stride;
#pragma unroll 1
        for (int pass = 0; pass < kPasses; ++pass) {
            const int j = pass * kGroups + grp;
            if (j >= n_here) break;                    // group-uniform: GroupSync involves this group only
            if (pass > 0 && !plain) sync();            // the previous image is still being read by the blur
            const CamPose cp = pose[k & 1][j];
            int gtl = gt;
            asm volatile("" : "+v"(gtl));              // per-pass copy: keeps the pixel / patch bookkeeping from being hoisted out of
                                                       // the loops and held in ~50 registers across them
            const auto lookup = [&] {
                if constexpr (LDSMAP) return LdsBitLookup{mapbits};
                else return GlobalMapLookup(m);
            }();
            render_image<GT>(p_arg, m, lookup, cp, obs_k + (int64_t)(e0 + j) * WL_VIS_OBS_DIM, img + grp * kImgFloats,
                             red + grp * (GT / 64), gtl, true, sync);
        }
    }
}

template <class Ground = FlatGround>
__global__ void __launch_bounds__(kBlock) visual_reset_kernel(const WlVisualParams p, const WlEnvBuffers b, const WlTravMap m,
                                                              const uint8_t* __restrict__ mask, uint64_t seed, uint64_t step,
                                                              const Ground ground = Ground{}) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= b.n_envs) return;
    if (mask && !mask[e]) return;
    const Rows S = make_rows(b.state, b.stride);
    const VisReset rd = visual_reset_pose(p, m, ground, (uint32_t)(b.env_offset + e), step, seed);
    store_reset_rows(S, b, e, rd.pos, rd.q, v3(0.f, 0.f, 0.f));
}

__global__ void __launch_bounds__(kBlock) visual_mdp_kernel(const WlVisualParams p, const WlTravMap m, int n, int64_t stride,
                                                            const float* __restrict__ pos, const float* __restrict__ vb,
                                                            float* __restrict__ terms, uint8_t* __restrict__ oom,
                                                            int32_t* __restrict__ x_idx, int32_t* __restrict__ y_idx) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const float x = pos[e], y = pos[stride + e];
    int xi, yi;
    map_id(m, x, y, xi, yi);
    x_idx[e] = xi;
    y_idx[e] = yi;
    terms[e] = m.map[yi * m.cols + xi] ? 1.f : -1.f;
    terms[stride + e] = vb[e];
    oom[e] = out_of_map(m, x, y) ? 1 : 0;
}

// ---- launches ----
template <int V>
using Int = std::integral_constant<int, V>;

// one step launch on Ground.  Lane form: <1, kBlock>.  Quad form on the plane: launch_quad's three block sizes; on a heightfield: the
// helper-wavefront form (kHelperQB physics threads in blocks of kHelperThreads) up to 8192 envs, <4, kBlock> beyond.
template <class Ground>
inline void launch_visual_step(const WlVisualParams* p, const VehDerived& vd, const WlEnvBuffers* b, const WlTravMap* m, const float* actions,
                               const WlStepOut& out, uint64_t seed, uint64_t step, const Ground& g, int prop_stride, int prop_offset,
                               hipStream_t hs) {
    const int n = b->n_envs;
    const auto launch = [&](auto lanes, auto qb, int grid, int threads) {
        visual_step_kernel<decltype(lanes)::value, decltype(qb)::value, Ground><<<grid, threads, 0, hs>>>(
            *p, vd, *b, *m, (const float2*)actions, out, seed, step, g, prop_stride, prop_offset);
    };
    if (use_quad(b)) {
        if constexpr (Ground::kFlat) launch_quad(n, [&](auto qb, int qgrid) { launch(Int<4>{}, qb, qgrid, qb.value); });
        else if (n <= 8192) launch(Int<4>{}, Int<kHelperQB>{}, (n * 4 + kHelperQB - 1) / kHelperQB, kHelperThreads);
        else launch(Int<4>{}, Int<kBlock>{}, grid_for(n * 4), kBlock);
    } else {
        launch(Int<1>{}, Int<kBlock>{}, grid_for(n), kBlock);
    }
}

#ifndef WL_VIS_STREAM_BYTES
#define WL_VIS_STREAM_BYTES 0ll
#endif
inline void launch_visual_obs(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, float* obs, hipStream_t hs) {
    // non-temporal rows at every size unless WL_FLAG_NO_STREAM asks otherwise (rounds 1-3: only beyond the 256 MB Infinity Cache, > 20 000
    // envs, where they are worth 12 %; round 4, env.step() in us with / without: 4096 envs 49.2 / 50.7, 8192: 72.2 / 73.5, 16 384: 117.6 / 119.8)
    with_bool(use_streaming(b, (int64_t)b->n_envs * WL_VIS_OBS_DIM * 4, WL_VIS_STREAM_BYTES), [&](auto stream) {
        with_bool(b->n_envs > WL_CAM_MIN_WAVES_ENVS, [&](auto dense) {
            visual_obs_kernel<decltype(stream)::value, decltype(dense)::value ? WL_CAM_MIN_WAVES : 1><<<b->n_envs, kCam, 0, hs>>>(*p, *b, *m, obs);
        });
    });
}

inline bool lds_map_ok(const WlTravMap* m) { return m->bits != nullptr && (int64_t)m->rows * m->cols <= WL_VIS_LDS_MAP_CELLS; }

// ---- argument checks ----
// the map bytes of a SQUARE map: the lookup clamps x to rows - 1 and y to cols - 1 but reads map[y][x] of a [rows][cols] array
// (traversability_utils.py:78-88); past the shorter side the reference raises IndexError, and the kernels would read outside
// the allocation
inline bool trav_map_ok(const WlTravMap* m) { return m && m->map && m->rows > 0 && m->rows == m->cols; }

int check_visual(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m) {
    const int rc = check_implicit_env(p, b);
    if (rc != WL_OK) return rc;
    if (!trav_map_ok(m) || !m->cells || m->n_cells <= 0) return WL_EINVAL;
    // the camera indexes the map by 24-bit multiplies and reads it through a buffer resource of rows * cols bytes
    if (m->rows >= (1 << 23) || m->cols >= (1 << 23) || (int64_t)m->rows * m->cols > 0x7fffffffLL) return WL_EINVAL;
    return WL_OK;
}
// .. and the heightfield of the visual-depth task (pair: the contact sampler's table, wl_heightfield_pairs)
int check_visual_hf(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const WlHeightField* hf) {
    const int rc = check_visual(p, b, m);
    return rc != WL_OK ? rc : heightfield_args_ok(hf, HF_PAIRS);
}

}  // namespace

extern "C" {

int wl_visual_step(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const float* actions,
                   const WlStepOut* out, uint64_t seed, uint64_t step, void* stream) {
    return wl_visual_rollout(p, b, m, actions, out, 0, 0, 1, seed, step, stream);
}

int wl_visual_rollout(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const float* actions,
                      const WlStepOut* out, int64_t obs_step_stride, int64_t vec_step_stride, int32_t n_steps, uint64_t seed,
                      uint64_t step0, void* stream) {
    int rc = check_visual(p, b, m);
    if (rc != WL_OK) return rc;
    if (!actions || !step_out_ok(out) || n_steps < 0) return WL_EINVAL;
    const VehDerived vd = derive_vehicle(p->vehicle, p->sim_dt, p->decimation);
    clear_error();
    for (int k = 0; k < n_steps; ++k) {
        const WlStepOut o = step_out_at(*out, k, obs_step_stride, vec_step_stride);
        const hipStream_t hs = (hipStream_t)stream;
        launch_visual_step(p, vd, b, m, actions + (int64_t)k * b->n_envs * 2, o, seed, step0 + (uint64_t)k, FlatGround{}, 0, 0, hs);
        launch_visual_obs(p, b, m, o.obs, hs);
    }
    return launch_status();
}

int wl_visual_rollout_persistent(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const float* actions,
                                 const WlStepOut* out, int64_t obs_step_stride, int64_t vec_step_stride, int32_t n_steps,
                                 uint64_t seed, uint64_t step0, void* stream) {
    int rc = check_visual(p, b, m);
    if (rc != WL_OK) return rc;
    if (!use_quad(b)) return WL_EINVAL;   // the quad form's (n <= 32 768)
    if (!actions || !step_out_ok(out) || n_steps < 0) return WL_EINVAL;
    if (n_steps > 1 && obs_step_stride < (int64_t)b->n_envs * WL_VIS_OBS_DIM) return WL_EINVAL;   // the camera runs a step behind: rows must differ
    if (ring_aliases(b, n_steps)) return WL_EINVAL;
    clear_error();
    // envs per block: one round of blocks on the 256 CUs (a block's thirteen-plus wavefronts at 128 VGPRs fill a CU)
    const VehDerived vd = derive_vehicle(p->vehicle, p->sim_dt, p->decimation);
    const MetricSlots ms = metric_slots(b, step0, (uint64_t)n_steps);
    const int n = b->n_envs;
    const hipStream_t hs = (hipStream_t)stream;
    const auto launch = [&](auto envs) {   // envs per block: a std::integral_constant
        constexpr int E = decltype(envs)::value;
        with_bool(lds_map_ok(m), [&](auto lds) {
            visual_rollout_persistent_kernel<E, decltype(lds)::value><<<(n + E - 1) / E, kPersistThreads, 0, hs>>>(
                *p, vd, *b, *m, (const float2*)actions, *out, obs_step_stride, vec_step_stride, n_steps, seed, step0, ms);
        });
    };
    if (n <= 1024) launch(Int<4>{});
    else if (n <= 2048) launch(Int<8>{});
    else launch(Int<16>{});
    return launch_status();
}

int wl_visual_reset(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const uint8_t* mask, uint64_t seed,
                    uint64_t step, void* stream) {
    int rc = check_visual(p, b, m);
    if (rc != WL_OK) return rc;
    clear_error();
    visual_reset_kernel<FlatGround><<<grid_for(b->n_envs), kBlock, 0, (hipStream_t)stream>>>(*p, *b, *m, mask, seed, step, FlatGround{});
    return launch_status();
}

int wl_visual_observe(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, float* obs, void* stream) {
    int rc = check_visual(p, b, m);
    if (rc != WL_OK) return rc;
    if (!obs) return WL_EINVAL;
    clear_error();
    launch_visual_obs(p, b, m, obs, (hipStream_t)stream);
    return launch_status();
}

/* ---- the visual-depth extension task (BASELINE config 5): the visual task's step on a heightfield terrain; the observation row is
 * [ depth image 4800 | base_lin_vel 3 | base_ang_vel 3 | last_action 2 ]: this launch writes the last 8, wl_depth.hip the image ---- */
int wl_visual_step_hf(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const WlHeightField* hf, const float* actions,
                      const WlStepOut* out, uint64_t seed, uint64_t step, void* stream) {
    const int rc = check_visual_hf(p, b, m, hf);
    if (rc != WL_OK) return rc;
    if (!actions || !step_out_ok(out)) return WL_EINVAL;
    const VehDerived vd = derive_vehicle(p->vehicle, p->sim_dt, p->decimation);
    clear_error();
    launch_visual_step(p, vd, b, m, actions, *out, seed, step, make_ground(hf), WL_VISDEPTH_OBS_DIM, WL_VISDEPTH_NPIX, (hipStream_t)stream);
    return launch_status();
}

int wl_visual_reset_hf(const WlVisualParams* p, const WlEnvBuffers* b, const WlTravMap* m, const WlHeightField* hf, const uint8_t* mask,
                       uint64_t seed, uint64_t step, void* stream) {
    const int rc = check_visual_hf(p, b, m, hf);
    if (rc != WL_OK) return rc;
    clear_error();
    visual_reset_kernel<HeightFieldGround><<<grid_for(b->n_envs), kBlock, 0, (hipStream_t)stream>>>(*p, *b, *m, mask, seed, step, make_ground(hf));
    return launch_status();
}

int wl_visual_mdp(const WlVisualParams* p, const WlTravMap* m, int32_t n, int64_t stride, const float* pos,
                  const float* lin_vel_b, float* terms, uint8_t* out_of_map_, int32_t* x_idx, int32_t* y_idx, void* stream) {
    if (!p || !trav_map_ok(m) || n <= 0 || stride < n || !pos || !lin_vel_b || !terms || !out_of_map_ || !x_idx || !y_idx)
        return WL_EINVAL;
    clear_error();
    visual_mdp_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(*p, *m, n, stride, pos, lin_vel_b, terms, out_of_map_,
                                                                        x_idx, y_idx);
    return launch_status();
}

}  // extern "C"

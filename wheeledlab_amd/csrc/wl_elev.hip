// wl_elev.hip -- elevation task (wheeledlab_tasks/elevation/mushr_elevation_env_cfg.py) for gfx950.
//
// Launches per env.step():
//   quad form (n <= 32 768): ONE -- elev_step_scan_kernel: block = 16 envs; wavefront 0 steps them (one quad of lanes per
//      env: 4WD action term -> decimation x substeps of the rigid body + 4 tyre contacts on the heightfield (bilinear
//      height + normal gathers, L2-resident grid) -> terminations -> rewards -> in-kernel reset -> goal-command update),
//      then all 8 wavefronts cast the 16 x 676 height rays from the poses wavefront 0 left in LDS.  Round 2: 30.3 ->
//      27.8 us per step at 4096 envs against the two launches below (the scan no longer pays its own launch gap, wave
//      ramp and pose-row latency; a first fused version with 4 wavefronts and 4 batches of gathers per lane gained nothing).
//   lane form: TWO --
//   1. elev_step_kernel  (lane = env): the same step; state is read once / written once, sub-steps stay in VGPRs; also
//      writes the 13 proprioceptive values of the observation row.
//   2. elev_scan_kernel (block = env): the 26 x 26 yaw-aligned height rays, four per lane, written as 16-byte words -- this
//      launch carries ~90 % of the task's HBM bytes (2.7 KB / env).  One 8-byte gather of four height codes per ray from the
//      row-pair table; the terrain is 16-bit codes x z_scale since round 5 (wl_heightfield.h).  (Round 2 history: staging the env's
//      terrain patch in LDS -- its bounding box fetched row by row with coalesced 8-byte requests, corners read from
//      the tile -- was measured slower in every form tried: block per env 15.8 us, persistent blocks with the next
//      env's pose prefetched 18 us, against 11.3 us for the gathers; round 2, DESIGN.md section 6.  Round 3: the same for the
//      PHYSICS -- the 24 x 24 grid points under each car staged in LDS by all eight wavefronts of the fused kernel, the wheel
//      contacts of the 20 sub-steps reading their corners from there: + 2.7 us for the staging and NOTHING back per sub-step
//      (1.12 against 1.09 us per decimation step): the sub-step is a dependent VALU chain, its two gathers per wheel are
//      already hidden behind it.)
#include <hip/hip_runtime.h>

#include <type_traits>

// Debug builds only (tools/build_variants.sh ... -DWL_FUSED_TIMELINE=1; tools/fused_timeline.py): lane 0 of a wavefront stamps
// the 100 MHz wall clock into wl_timeline[block][slot] at the phase boundaries of the fused step + scan launch.
#ifndef WL_FUSED_TIMELINE
#define WL_FUSED_TIMELINE 0
#endif
#if WL_FUSED_TIMELINE
__device__ unsigned long long wl_timeline[2048][16];
#define WL_TL(slot) do { if ((threadIdx.x & 63) == 0) wl_timeline[blockIdx.x & 2047][slot] = wall_clock64(); } while (0)
#else
#define WL_TL(slot) do { } while (0)
#endif


#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_actor_dev.h"
#include "wl_rng.h"
#include "wl_implicit_task.h"
#include "wl_elev_scan_dev.h"   // the height scan: an env's lattice frame, a ray, a quad of rays
#include "wl_elev_env.h"        // one env's step: terms, reset draws, levels, bookkeeping, elev_env_step

namespace {

// (lane form: 110 VGPRs = 4 wavefronts per SIMD.  Squeezed to 96 / 80 registers for 5 / 6 wavefronts the kernel spills 60 / 128 bytes
// of scratch per lane and the step at 262 144 envs goes from 650 to 664 / 782 us: round 3.)
#ifndef WL_ELEV_LANE_WAVES
#define WL_ELEV_LANE_WAVES 1
#endif
// lane = env (the quad form of the step is elev_step_scan_kernel's wavefront 0)
template <bool LEVELS>
__global__ void __launch_bounds__(kBlock, WL_ELEV_LANE_WAVES) elev_step_kernel(const ElevHead h_arg, const VehDerived vd_arg, const WlEnvBuffers b,
                                                           const HeightFieldGround ground, const float2* __restrict__ actions,
                                                           const WlStepOut out, const uint64_t seed, const uint64_t step,
                                                           const WlTerrainLevels tl_arg) {
    __shared__ float blk_metrics[WL_M_COUNT];
    const WlElevParams& p = elev_args(h_arg);
    VehDerived vd = vd_arg;   // (a copy, not the argument itself: read in place, one of its scalar loads is issued elsewhere)
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (threadIdx.x < WL_M_COUNT) blk_metrics[threadIdx.x] = 0.f;
    const int m_slot = b.metrics_slots > 1 ? (int)(step % (uint64_t)b.metrics_slots) : 0;
    if (b.metrics_slots > 1) clear_metric_slot(b, (m_slot + 1) % b.metrics_slots);
    __syncthreads();
    const Rows S = make_rows(b.state, b.stride);
    if (e < b.n_envs) {
        VehRows<1> rows = load_veh_rows<1>(S, e, 0);
        (void)elev_env_step<1, LEVELS>(p, vd, b, ground, actions[e], rows, out, seed, step, S, e, 0, true, blk_metrics, tl_arg);
    }
    __syncthreads();
    block_metrics_flush(blk_metrics, b, m_slot);   // threads 0..15 = wavefront 0 of the block
}

// world_height_map (:44-48): the 26 x 26 yaw-aligned height scan, clipped to +-10, into obs[e][13:689].  One block per
// env; the env's 13 proprioceptive values are written by the lane-per-env kernels (step / prop).
// (Rounds 1 - 3: 128 threads per env, 5.3 rays per lane, dword stores.)
constexpr int kScanThreads = 192;                       // threads per env: 169 quads of rays -> one quad per lane, three wavefronts
template <bool STREAM>   // observation rows of the launch beyond the Infinity Cache: non-temporal stores
__global__ void __launch_bounds__(kScanThreads) elev_scan_kernel(const WlElevParams p, const WlEnvBuffers b, const HeightFieldGround ground,
                                                                 float* __restrict__ obs) {
    const int e = blockIdx.x, tid = threadIdx.x;
    if (tid >= kScanQuads) return;
    const Rows S = make_rows(b.state, b.stride);
    const float px = S.ld(WL_S_PX, e), py = S.ld(WL_S_PY, e), pz = S.ld(WL_S_PZ, e);
    const Quat q{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    float c, s;
    yaw_cs(q, c, s);
    const ScanFrame fr = scan_frame(p, ground, ScanPose{px, py, pz, c, s});
    const ScanField sf = scan_field(ground.f);
    ScanRay cr[4];
    scan_quad_request(fr, ground.f, sf, tid, cr);     // this lane's four rays: their 8 gathers in flight together
    scan_quad_store<STREAM>(obs + (int64_t)e * WL_ELEV_OBS_DIM + 13, tid, scan_quad_value(p, cr, sf.z_scale, pz));
}
#ifndef WL_ELEV_FUSED_MAX_ENVS
#define WL_ELEV_FUSED_MAX_ENVS 12288
#endif
#ifndef WL_ELEV_STREAM_BYTES
#define WL_ELEV_STREAM_BYTES 0ll
#endif
// The gathers at every size (round 6): with the row-pair table a ray is one lane address, and the gather scan passed the LDS-patch
// scan (the env's footprint staged by LDS-DMA; measured, dropped: DESIGN.md section 7) at every size.
inline void launch_elev_scan(const WlElevParams* p, const WlEnvBuffers* b, const HeightFieldGround& g, float* obs, hipStream_t hs) {
    // non-temporal map rows at every size unless WL_FLAG_NO_STREAM asks otherwise (round 4: 2 - 3 % of the step from 4096 envs up; the rows
    // are not read again by this launch, and an XCD's L2 does not survive the launch boundary anyway)
    const bool stream = use_streaming(b, (int64_t)b->n_envs * WL_ELEV_OBS_DIM * 4, WL_ELEV_STREAM_BYTES);
    if (stream) elev_scan_kernel<true><<<b->n_envs, kScanThreads, 0, hs>>>(*p, *b, g, obs);
    else elev_scan_kernel<false><<<b->n_envs, kScanThreads, 0, hs>>>(*p, *b, g, obs);
}

// env.step() AND the height scan as ONE launch (quad form, n <= 32 768): block = 16 envs, 8 wavefronts.  Wavefront 0
// steps them (16 quads of lanes: elev_env_step<4>) while wavefront 1 draws their reset poses (ResetHelper), and leaves each
// env's post-step lattice frame in LDS; then all eight wavefronts cast the 16 x 169 quads of rays (flat index over (env, quad),
// one quad per lane and batch: the scan phase below).  Against the two-launch form this removes the scan kernel's own start
// (launch gap, wave ramp, the pose rows' first-touch latency) from the step's dependent chain, and one physics wavefront per CU
// spreads the step over 256 CUs instead of 64 (4096 envs).
constexpr int kFusedThreads = 512, kFusedEnvs = 16;

template <bool LEVELS>
__global__ void __launch_bounds__(kFusedThreads) elev_step_scan_kernel(const ElevHead h_arg, const VehDerived vd_arg,
                                                                       const WlEnvBuffers b, const HeightFieldGround ground,
                                                                       const float2* __restrict__ actions, const WlStepOut out,
                                                                       const uint64_t seed, const uint64_t step, const WlTerrainLevels tl_arg) {
    const WlElevParams& p_arg = elev_args(h_arg);
    __shared__ float blk_metrics[WL_M_COUNT];
    __shared__ ScanFrame frame[kFusedEnvs];
    __shared__ ResetHelper<ElevReset, kFusedEnvs> resets;     // the block's 16 reset draws, by wavefront 1 while wavefront 0 integrates
    const int tid = threadIdx.x;
    if (tid < 64) WL_TL(0);
    resets.init();
    if (tid < WL_M_COUNT) blk_metrics[tid] = 0.f;
    const int m_slot = b.metrics_slots > 1 ? (int)(step % (uint64_t)b.metrics_slots) : 0;
    if (b.metrics_slots > 1) clear_metric_slot(b, (m_slot + 1) % b.metrics_slots);
    const int e0 = blockIdx.x * kFusedEnvs;
    __syncthreads();
    if (tid < 64) {
        const int wid = tid & 3, e = e0 + (tid >> 2);
        if (e < b.n_envs) {
            // ONE memory round trip in front of the physics instead of four in series (parameter block, derived block, action,
            // state rows -- each waited for where it was first used): the state rows and the action are requested first (they
            // need only scalar arguments), the two argument structs right behind them as one burst, and a basic-block boundary
            // keeps the instruction selector from sinking the requests back to their first uses (as in drift_step_kernel).
            // (the action through a buffer resource, like the state rows: as a plain global load the scheduler parked it behind
            // the parameter block, waiting for a register the burst still had in flight -- a second round trip)
            float2 a;
            float2* ap = const_cast<float2*>(actions);
            asm volatile("" : "+s"(ap));   // launder the read-only / no-alias argument: its loads are otherwise free to cross the boundary below
            const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(ap, 0, b.n_envs * 8, 0x00020000);
            a.x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ar, e * 8, 0, 0));
            a.y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ar, e * 8, 4, 0));
            const Rows S = make_rows(b.state, b.stride);
            VehRows<4> rows = load_veh_rows<4>(S, e, wid);
            WlElevParams p;
            VehDerived vd;
            elev_kernarg_copy(p, vd);
            int go = 1;
            asm volatile("" : "+s"(go) : : "memory");
            if (go) {
                keep_scalar_common(p, p_arg);
                vd.n_sub = vd_arg.n_sub;
                // the block's ONE meeting point sits in the middle of this wavefront's step: as soon as the pose it leaves behind is
                // known (after a reset's draw) the lattice frames go to LDS and the other seven wavefronts start casting rays, while
                // this one weights its rewards, writes outputs, metrics and state rows and then joins them for a smaller share
                // (fused_scan_share).  Round 6, tools/fused_timeline.py: the bookkeeping was 1.1 us of every launch with seven
                // wavefronts waiting behind it.  (Every block has an env, so wavefront 0 always gets here, and elev_env_step calls
                // `pose` exactly once on every path: one s_barrier per wavefront.)
                auto pose = [&](const V3& pos_out, const Quat& q_out) {
                    float yc, ys;
                    yaw_cs(q_out, yc, ys);
                    if (wid == 0) frame[tid >> 2] = scan_frame(p, ground, ScanPose{pos_out.x, pos_out.y, pos_out.z, yc, ys});
                    WL_TL(3);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                };
                const HelperReset<ElevReset, kFusedEnvs> reset_src{&resets, e0, true};
                (void)elev_env_step<4, LEVELS>(p, vd, b, ground, a, rows, out, seed, step, S, e, wid, wid == 0, blk_metrics, tl_arg, nullptr, nullptr, reset_src, pose);
            }
        }
        WL_TL(4);
        static_assert(WL_M_COUNT <= 64, "wavefront 0 flushes the block's metrics alone");
        block_metrics_flush(blk_metrics, b, m_slot);
    } else {
        if (tid < 128) {      // wavefront 1: the block's reset draws, in the shadow of the physics
            const int j = tid - 64;
            // (levels on: the origin-free part -- the tile is known only once the stepping wavefront has the episode's outcome)
            const uint32_t gid = (uint32_t)(b.env_offset + e0 + j);
            if constexpr (LEVELS) resets.publish(j, j < kFusedEnvs && e0 + j < b.n_envs, [&] { return draw_elev_reset_local(p_arg, gid, step, seed); });
            else resets.publish(j, j < kFusedEnvs && e0 + j < b.n_envs, [&] { return draw_elev_reset(p_arg, ground, gid, step, seed); });
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (tid >= kFusedThreads - 64) WL_TL(8);
    }
    // ---- the scan ----
    const WlElevParams& p = p_arg;
    const int n_here = min(kFusedEnvs, b.n_envs - e0);
    const ScanField sf = scan_field(ground.f);
    // flat index over (env, quad of rays): 16 x 169 quads / 512 lanes = 5.3 per lane, ONE quad (4 eight-byte gathers) per batch:
    // request, blend, store, next.  (Rounds 2 - 3, single rays: 1 / 2 / 3 batches of gathers 28.4 / 26.2 / 25.9 us per step at 4096
    // envs; round 6, 10 sub-steps: 1 / 2 / 3 / 6 batches 21.4 / 21.3 / 21.3 / 20.2 us.)
    // What bounds the phase (round 6, tools/fused_timeline.py: wall-clock stamps inside the launch; tools/tcp_pass.sh: TA / TCP
    // counters): NOT its stores -- 0.2 - 0.4 us from a wavefront's last store to its acknowledgement; 11.3 MB written with nothing
    // in front of them cost 1.8 - 2.9 us on top of an empty launch (tools/microbench/row_burst.hip), and that overlaps the phase --
    // but the TEXTURE UNIT's address rate: with two 4-byte gathers per ray the phase took 6.1 - 6.8 us, the unit was busy 16 000
    // cycles per CU (all of it), 57 cache accesses per 64-lane gather instruction, L1 hit rate 0.91.  One 8-byte gather per ray
    // (the row-pair table): 4.2 - 4.5 us = 10 816 lane addresses per CU; the phase's ~1000 vector instructions per wavefront are 1.8 us
    // of pipe at two wavefronts per SIMD, so it is still the unit's -- fewer lane addresses (an LDS patch) would be the next step.
    // Measured and dropped in round 6: the same loop software-pipelined (quad k + 1 requested before quad k is blended and stored:
    // 21.0 against 20.5 us, and 19.1 against 18.6 with the pair table -- the older wavefronts of a SIMD run ahead and the younger
    // ones finish alone); store cache policies sc1 / nt / write-through (equal); a wavefront per env with the rays in 7 x 9 blocks of
    // neighbours (21.1 us).
    // 43 chunks of 64 ray quads (the last one holds 16) in six rounds; the wavefronts of a round take NEIGHBOURING chunks (what is in
    // flight on the CU at a time then covers ~3 envs' patches of the table; with a contiguous range per wavefront -- 16 envs' patches
    // at once -- the phase took 4.8 instead of 4.2 us: L1).  Wavefront 0, busy with its bookkeeping, sits out the first two rounds:
    // rounds 0 - 1: wavefronts 1 - 7 (7 chunks each), rounds 2 - 4: all eight, round 5: wavefronts 0 - 4 -- per SIMD (wavefronts s and
    // s + 4) 11 chunks, or 10 + the bookkeeping.
    constexpr int kAll = kFusedEnvs * kScanQuads, kChunks = (kAll + 63) / 64;
    static_assert(kChunks == 43 && kFusedThreads == 512, "the shares below are for 16 envs x 169 quads on eight wavefronts");
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const bool mine = r < 2 ? wave != 0 : (r < 5 || wave <= 4);      // wavefront-uniform
        if (mine) {
            const int chunk = r < 2 ? 7 * r + wave - 1 : 14 + 8 * (r - 2) + wave;
            const int idx = chunk * 64 + lane;
            int j, q;
            scan_quad_slot(min(idx, kAll - 1), j, q);
            const ScanFrame fr = frame[min(j, n_here - 1)];
            ScanRay cr[4];
            scan_quad_request(fr, ground.f, sf, q, cr);
            if (idx < kAll && j < n_here)
                scan_quad_store<WL_FUSED_SCAN_NT>(out.obs + (int64_t)(e0 + j) * WL_ELEV_OBS_DIM + 13, q, scan_quad_value(p, cr, sf.z_scale, fr.pz));
        }
    }
#if WL_FUSED_TIMELINE
    if (tid < 64) WL_TL(5);
    if (tid >= kFusedThreads - 64) WL_TL(9);
    __builtin_amdgcn_s_waitcnt(0);
    if (tid < 64) WL_TL(6);
    if (tid >= kFusedThreads - 64) WL_TL(10);
#endif
}

// K env.step()s in ONE launch with pre-staged actions [K][n][2] (open-loop rollouts: sampling-based planners, system
// identification, the bench; quad form, n <= 32 768).  Block = 16 envs.  Wavefront 0 keeps their rows and bookkeeping in
// registers across the K steps (VehRows / ElevBook: no state round trip, no launch boundary per step) and leaves each
// step's poses in one of two LDS buffers; wavefronts 1..7 cast the height rays of step k WHILE wavefront 0 already
// integrates step k + 1 -- with actions that do not depend on the observations the scan is off the critical path.  One
// s_barrier per step and wavefront: at barrier k wavefront 0 has finished step k, the others the scan of step k - 1.
// Episode metrics of all K steps go to ring slot `slots.cur`, `slots.next` is cleared for the next launch.
constexpr int kScanLanes = kFusedThreads - 64;
template <bool LEVELS>
__global__ void __launch_bounds__(kFusedThreads) elev_rollout_persistent_kernel(const ElevHead h_arg, const VehDerived vd_arg,
                                                                                const WlEnvBuffers b, const HeightFieldGround ground,
                                                                                const float2* __restrict__ actions, const WlStepOut out,
                                                                                const int64_t obs_step_stride, const int64_t vec_step_stride,
                                                                                const int n_steps, const uint64_t seed, const uint64_t step0,
                                                                                const MetricSlots slots, const WlTerrainLevels tl_arg) {
    __shared__ float blk_metrics[WL_M_COUNT];
    __shared__ ScanFrame frame[2][kFusedEnvs];
    const WlElevParams& p_arg = elev_args(h_arg);
    const int tid = threadIdx.x;
    if (tid < WL_M_COUNT) blk_metrics[tid] = 0.f;
    if (b.metrics_slots > 1) clear_metric_slot(b, slots.next);
    __syncthreads();
    const int e0 = blockIdx.x * kFusedEnvs;
    if (tid < 64) {
        const int wid = tid & 3, e = e0 + (tid >> 2);
        const bool valid = e < b.n_envs;
        const Rows S = make_rows(b.state, b.stride);
        VehRows<4> rows;
        ElevBook book;
        WlElevParams p;
        VehDerived vd;
        if (valid) {
            rows = load_veh_rows<4>(S, e, wid);
            elev_kernarg_copy(p, vd);
            keep_scalar_common(p, p_arg);
            vd.n_sub = vd_arg.n_sub;
            book = load_elev_book<4>(p, b, S, e);
        }
        for (int k = 0; k < n_steps; ++k) {
            if (valid) {
                const WlStepOut o = step_out_at(out, k, obs_step_stride, vec_step_stride);
                const float2 a = actions[(int64_t)k * b.n_envs + e];
                const ScanPose sp = elev_env_step<4, LEVELS, true>(p, vd, b, ground, a, rows, o, seed, step0 + (uint64_t)k, S, e, wid, wid == 0,
                                                           blk_metrics, tl_arg, &book);
                if (wid == 0) frame[k & 1][tid >> 2] = scan_frame(p, ground, sp);
            }
            __syncthreads();   // barrier k: the poses of step k are published
        }
        if (valid) store_elev_state<4>(p, b, S, e, wid, wid == 0, rows, book);
        block_metrics_flush(blk_metrics, b, slots.cur);   // only this wavefront accumulated
        return;
    }
    // ---- wavefronts 1..7: the scan of step k, one step behind the physics ----
    const WlElevParams& p = p_arg;
    const int t7 = tid - 64;
    constexpr int kAll = kFusedEnvs * kScanQuads;
    constexpr int kBatches = 3, kSlots = (kAll + kScanLanes - 1) / kScanLanes, kBatch = (kSlots + kBatches - 1) / kBatches;
    const int n_here = min(kFusedEnvs, b.n_envs - e0);
    const ScanField sf = scan_field(ground.f);
    for (int k = 0; k < n_steps; ++k) {
        __syncthreads();       // barrier k
        float* obs_k = out.obs + k * obs_step_stride;
#pragma unroll
        for (int part = 0; part < kBatches; ++part) {
            ScanRay cr[kBatch][4];
            float pz[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                int j, q;
                scan_quad_slot(min(t7 + (part * kBatch + i) * kScanLanes, kAll - 1), j, q);
                const ScanFrame fr = frame[k & 1][min(j, n_here - 1)];
                pz[i] = fr.pz;
                scan_quad_request(fr, ground.f, sf, q, cr[i]);
            }
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int idx = t7 + (part * kBatch + i) * kScanLanes;
                int j, q;
                scan_quad_slot(idx, j, q);
                if (idx < kAll && j < n_here) scan_quad_store<WL_FUSED_SCAN_NT>(obs_k + (int64_t)(e0 + j) * WL_ELEV_OBS_DIM + 13, q, scan_quad_value(p, cr[i], sf.z_scale, pz[i]));
            }
        }
    }
}

// ---- the runner's collection, K x { actions = actor(obs) -> env.step -> storage rows } (modified_rsl_rl_runner.py:70-80), as ONE launch ----
// Block = 16 envs, eight wavefronts, K steps in a loop.  What makes the policy step cheap enough to live inside the env's
// block: the ACTOR's first-layer matrix (64 x 689 f32 = 176 KB) is held in the block's REGISTERS for the whole launch (each
// of the eight wavefronts keeps the MFMA A fragments of its 5 - 6 sixteen-feature chunks: <= 96 VGPRs; a CU's register
// file is 512 KB), and the block's 16 observation rows live in LDS, where the scan writes them.  Per step and block:
//   A  all eight wavefronts: partial layer-1 products of the actor from registers x LDS rows (<= 96 MFMAs each), to LDS
//   B  wavefront 0: sums them, layers 2 - 3 (tail weights parked in LDS), draw, log-prob, storage rows; then the 16 envs'
//      physics as in elev_rollout_persistent_kernel (rows and bookkeeping parked in LDS between steps: registers are the
//      scarce resource here -- every wavefront's allocation carries the 96 weight registers)
//   D  all wavefronts: the 16 x 676 height rays of the post-step poses, into the storage's next observation row AND the LDS rows
// Three s_barriers per step.  (A one-launch-per-step collector, both first-layer matrices streamed from L2 for 16 rows per
// step and block -- 90 MB per step chip-wide -- was bound by exactly that: DESIGN.md section 7.)
// The CRITIC is not in here: its values are not needed to step, and the caller evaluates all K + 1 observation rows in one
// batched pass afterwards.  Measured with the critic inside (its first layer streamed from L2 by wavefronts 1..7 beside
// the physics, wavefront 1 finishing the net): 55 us per step against 33.7 without -- not the streaming itself (pacing it
// and cache-policy bits changed nothing) but its registers: the allocator answered with 85 - 160 spills, part of them
// inside the sub-step loop of the lone physics wavefront.
// Arithmetic: layer 1 is summed in eight partial sums per unit (wl_actor_critic_act: four): equal to that kernel to rounding,
// not bit for bit; the env.step is elev_env_step's.
// what the collector kernel's policy phase reads and fills: rows k of an rsl_rl RolloutStorage
struct PolicyIo {
    WlMlp actor, critic;
    const float* std;
    const float* obs_in;   // [n][689] observation row k
    float *actions, *mu, *log_prob, *values;
    int deterministic;
};

constexpr int kColWavesA = 8;                                                  // wavefronts sharing the actor's first layer
constexpr int kColChunks = (WL_ELEV_OBS_DIM + 15) / 16;                        // 44 (the last holds one feature)
constexpr int kColMaxA = (kColChunks + kColWavesA - 1) / kColWavesA;           // 6
// LDS row of one env's observation: the 44 chunks' 704 floats (the last chunk's 15 features past the 689th read the row's own
// zeroed pad -- with a 692-float row they read the next row, and row 15 read past the tile into part_a, where 0 x a NaN / Inf
// left there is NaN), + 4 so that the 16 rows start 4 banks apart (a multiple of 64 floats would put them all on one bank)
constexpr int kTilePitch = kColChunks * 16 + 4;                                 // 708 floats: 16-byte aligned LDS rows
static_assert(kTilePitch % 4 == 0 && kTilePitch % 64 == 4 && kTilePitch >= kColChunks * 16, "row layout");
constexpr int kPartFloats = kColWavesA * kMlpTiles * 64 * 4;                   // one net's partial accumulators
constexpr int kTailFloats = (kMlpTiles * kMlpHidSteps + kMlpHidSteps) * 64;    // an MlpTail, [value][lane]
constexpr int kCarryWords = 20 + 3 + WL_ER_NTERMS + 4 + 2;                      // wavefront 0's rows + bookkeeping (carry_io), [word][lane]
constexpr int kColLdsFloats = kFusedEnvs * kTilePitch + kPartFloats + kTailFloats + kCarryWords * 64 + kFusedEnvs * 13 +
                              kFusedEnvs * 8 + kFusedEnvs * 2 + WL_M_COUNT + 4;
WL_DEV int col_chunk_begin(int w, int waves) { return w * (kColChunks / waves) + min(w, kColChunks % waves); }

// wavefront-private values parked in LDS, one column per lane (no barrier: the lane that writes is the lane that reads).
// Field by field: a memcpy through a word array left the array on the stack.
struct LdsColumn {
    float* base;
    int lane, i;
    WL_DEV void put(float v) { base[(i++) * 64 + lane] = v; }
    WL_DEV void put(int v) { base[(i++) * 64 + lane] = __int_as_float(v); }
    WL_DEV void get(float& v) { v = base[(i++) * 64 + lane]; }
    WL_DEV void get(int& v) { v = __float_as_int(base[(i++) * 64 + lane]); }
};
template <bool PUT, class T>
WL_DEV void col_io(LdsColumn& c, T& v) {
    if constexpr (PUT) c.put(v); else c.get(v);
}
template <bool PUT>
WL_DEV void tail_io(float* base, int lane, MlpTail& W) {
    LdsColumn c{base, lane, 0};
#pragma unroll
    for (int t = 0; t < kMlpTiles; ++t)
#pragma unroll
        for (int i = 0; i < kMlpHidSteps; ++i) col_io<PUT>(c, W.w2[t][i]);
#pragma unroll
    for (int i = 0; i < kMlpHidSteps; ++i) col_io<PUT>(c, W.w3[i]);
}
template <bool PUT>
WL_DEV void carry_io(float* base, int lane, VehRows<4>& r, ElevBook& k) {
    LdsColumn c{base, lane, 0};
    col_io<PUT>(c, r.mass), col_io<PUT>(c, r.mu_s), col_io<PUT>(c, r.mu_d), col_io<PUT>(c, r.damp);
    col_io<PUT>(c, r.pos.x), col_io<PUT>(c, r.pos.y), col_io<PUT>(c, r.pos.z);
    col_io<PUT>(c, r.v.x), col_io<PUT>(c, r.v.y), col_io<PUT>(c, r.v.z);
    col_io<PUT>(c, r.ww.x), col_io<PUT>(c, r.ww.y), col_io<PUT>(c, r.ww.z);
    col_io<PUT>(c, r.q.w), col_io<PUT>(c, r.q.x), col_io<PUT>(c, r.q.y), col_io<PUT>(c, r.q.z);
    col_io<PUT>(c, r.wheel[0]), col_io<PUT>(c, r.th), col_io<PUT>(c, r.om);
    col_io<PUT>(c, k.ep_len), col_io<PUT>(c, k.cb[0]), col_io<PUT>(c, k.cb[1]);
#pragma unroll
    for (int i = 0; i < WL_ER_NTERMS; ++i) col_io<PUT>(c, k.epsum[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) col_io<PUT>(c, k.tgt[i]);
    col_io<PUT>(c, k.act[0]), col_io<PUT>(c, k.act[1]);
}

template <int ACT, bool LEVELS>
__global__ void __launch_bounds__(kFusedThreads) elev_collect_rollout_kernel(const ElevHead h_arg, const VehDerived vd, const WlEnvBuffers b,
                                                                             const HeightFieldGround ground, const WlStepOut out,
                                                                             const int n_steps, const uint64_t seed, const uint64_t step0,
                                                                             const PolicyIo pio, const MetricSlots slots, const WlTerrainLevels tl_arg) {
    const WlElevParams& p = elev_args(h_arg);
    extern __shared__ __attribute__((aligned(16))) float col_lds[];
    float* obs_tile = col_lds;                                   // [16][kTilePitch]
    float* part_a = obs_tile + kFusedEnvs * kTilePitch;          // [8][4][64][4]
    float* tail_a = part_a + kPartFloats;                        // the actor's MlpTail, [85][64]
    float* carry = tail_a + kTailFloats;                         // wavefront 0's VehRows + ElevBook between steps, [words][64]
    float* prop = carry + kCarryWords * 64;                      // [16][13]
    ScanFrame* frame = reinterpret_cast<ScanFrame*>(prop + kFusedEnvs * 13);   // [16] (7 floats each, 8 reserved)
    float2* act_lds = reinterpret_cast<float2*>(prop + kFusedEnvs * 13 + kFusedEnvs * 8);
    float* blk_metrics = reinterpret_cast<float*>(act_lds + kFusedEnvs);
    constexpr int D = WL_ELEV_OBS_DIM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;
    const int e0 = blockIdx.x * kFusedEnvs, n = b.n_envs;
    const int n_here = min(kFusedEnvs, n - e0);
    if (tid < WL_M_COUNT) blk_metrics[tid] = 0.f;
    if (b.metrics_slots > 1) clear_metric_slot(b, slots.next);
    // the block's first observation rows -> LDS (rows past the batch and the pad columns: zero)
    for (int i = tid; i < kFusedEnvs * kTilePitch; i += kFusedThreads) {
        const int r = i / kTilePitch, c = i - r * kTilePitch;
        obs_tile[i] = (r < n_here && c < D) ? pio.obs_in[(int64_t)(e0 + r) * D + c] : 0.f;
    }
    // every wavefront: its chunks of the actor's first layer as MFMA A fragments (unit 16 t + m, features 16 c + 4 g ..)
    const int a0 = col_chunk_begin(wave, kColWavesA), a1 = col_chunk_begin(wave + 1, kColWavesA);
    f32x4 ra[kColMaxA][kMlpTiles];
#pragma unroll
    for (int j = 0; j < kColMaxA; ++j)
#pragma unroll
        for (int t = 0; t < kMlpTiles; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = 16 * (a0 + j) + 4 * g + q;
                ra[j][t][q] = (a0 + j < a1 && f < D) ? pio.actor.w1[(int64_t)(16 * t + m) * D + f] : 0.f;
            }
    // wavefront 0: the actor's tail weights and the envs' rows / bookkeeping, parked in LDS between their uses
    const int wid = tid & 3, e = e0 + (tid >> 2);
    const bool phys = wave == 0 && e < n;
    const Rows S = make_rows(b.state, b.stride);
    if (wave == 0) {
        MlpTail Wa;
        load_tail(pio.actor, lane, Wa);
        tail_io<true>(tail_a, lane, Wa);
        if (phys) {
            VehRows<4> rows = load_veh_rows<4>(S, e, wid);
            ElevBook book = load_elev_book<4>(p, b, S, e);
            carry_io<true>(carry, lane, rows, book);
        }
    }
    const ScanField sf = scan_field(ground.f);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < n_steps; ++k) {
        const uint64_t step = step0 + (uint64_t)k;
        const int64_t kn = (int64_t)k * n;
        // ---- A: actor layer 1, partial sums (all eight wavefronts) ----
        {
            f32x4 h[kMlpTiles];
#pragma unroll
            for (int t = 0; t < kMlpTiles; ++t) h[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < kColMaxA; ++j)
                if (a0 + j < a1) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(obs_tile + m * kTilePitch + 16 * (a0 + j) + 4 * g);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int t = 0; t < kMlpTiles; ++t) h[t] = mfma4(ra[j][t][q], x[q], h[t]);
                }
#pragma unroll
            for (int t = 0; t < kMlpTiles; ++t) *reinterpret_cast<f32x4*>(part_a + ((wave * kMlpTiles + t) * 64 + lane) * 4) = h[t];
        }
        __syncthreads();   // barrier 1: the actor's partial sums are in LDS
        if (wave == 0) {
            // ---- B: the rest of the actor, the draw, the storage rows; then the physics ----
            {
                f32x4 h[kMlpTiles];
#pragma unroll
                for (int t = 0; t < kMlpTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[t][r] = pio.actor.b1[16 * t + 4 * g + r];
#pragma unroll
                for (int w = 0; w < kColWavesA; ++w)
#pragma unroll
                    for (int t = 0; t < kMlpTiles; ++t) h[t] += *reinterpret_cast<const f32x4*>(part_a + ((w * kMlpTiles + t) * 64 + lane) * 4);
                MlpTail Wa;
                tail_io<false>(tail_a, lane, Wa);
                const f32x4 o4 = eval_tail<ACT>(Wa, h, lane);
                if (g == 0) {
                    float z0 = 0.f, z1 = 0.f;
                    if (!pio.deterministic) {
                        const F4 u = philox_uniform4((uint32_t)(b.env_offset + e0 + m), step, WL_RS_POLICY, seed);
                        box_muller(u.x, u.y, z0, z1);
                    }
                    const float std0 = pio.std[0], std1 = pio.std[1];
                    const float2 av = make_float2(fmaf(std0, z0, o4[0]), fmaf(std1, z1, o4[1]));
                    act_lds[m] = av;
                    if (e0 + m < n) {
                        reinterpret_cast<float2*>(pio.actions)[kn + e0 + m] = av;
                        reinterpret_cast<float2*>(pio.mu)[kn + e0 + m] = make_float2(o4[0], o4[1]);
                        pio.log_prob[kn + e0 + m] = fmaf(-0.5f, fmaf(z0, z0, z1 * z1), -(log_fast(std0) + log_fast(std1)) - kLog2PiA);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // act_lds: written by lanes 0..15, read by all 64 below
            __builtin_amdgcn_wave_barrier();
            if (phys) {
                const WlStepOut o = step_out_at(out, k, (int64_t)n * D, n);
                const float2 a = act_lds[tid >> 2];
                VehRows<4> rows;
                ElevBook book;
                carry_io<false>(carry, lane, rows, book);
                const ScanPose sp = elev_env_step<4, LEVELS, true>(p, vd, b, ground, a, rows, o, seed, step, S, e, wid, wid == 0, blk_metrics, tl_arg, &book,
                                                           prop + (tid >> 2) * 13);
                carry_io<true>(carry, lane, rows, book);
                if (wid == 0) frame[tid >> 2] = scan_frame(p, ground, sp);
            }
        }
        __syncthreads();   // barrier 2: poses and proprioception of step k published; nobody reads the old observation rows any more
        // ---- D: the next observation rows: proprioception from wavefront 0, the height scan by everyone ----
        int tl = tid;
        asm volatile("" : "+v"(tl));   // per-step copy: keeps the 22 rays' index arithmetic of a thread inside the loop (registers)
        if (tl < kFusedEnvs * 13) {
            const int r = tl / 13, c = tl - r * 13;
            obs_tile[r * kTilePitch + c] = prop[tl];
        }
        {
            constexpr int kAll = kFusedEnvs * kScanQuads;
            constexpr int kBatches = 3, kSlots = (kAll + kFusedThreads - 1) / kFusedThreads, kBatch = (kSlots + kBatches - 1) / kBatches;
            float* obs_k = out.obs + kn * D;
#pragma unroll
            for (int part = 0; part < kBatches; ++part) {
                ScanRay cr[kBatch][4];
                float pz[kBatch];
#pragma unroll
                for (int i = 0; i < kBatch; ++i) {
                    int j, q;
                    scan_quad_slot(min(tl + (part * kBatch + i) * kFusedThreads, kAll - 1), j, q);
                    const ScanFrame fr = frame[min(j, n_here - 1)];
                    pz[i] = fr.pz;
                    scan_quad_request(fr, ground.f, sf, q, cr[i]);
                }
#pragma unroll
                for (int i = 0; i < kBatch; ++i) {
                    const int idx = tl + (part * kBatch + i) * kFusedThreads;
                    int j, q;
                    scan_quad_slot(idx, j, q);
                    if (idx < kAll && j < n_here) {
                        const wl_float4_u v = scan_quad_value(p, cr[i], sf.z_scale, pz[i]);
                        scan_quad_store<WL_FUSED_SCAN_NT>(obs_k + (int64_t)(e0 + j) * D + 13, q, v);
                        float* t4 = obs_tile + j * kTilePitch + 13 + 4 * q;
                        t4[0] = v.x, t4[1] = v.y, t4[2] = v.z, t4[3] = v.w;
                    }
                }
            }
        }
        __syncthreads();   // barrier 3: the observation rows of step k + 1 are complete
    }
    if (wave == 0) {
        if (phys) {
            VehRows<4> rows;
            ElevBook book;
            carry_io<false>(carry, lane, rows, book);
            store_elev_state<4>(p, b, S, e, wid, wid == 0, rows, book);
        }
        block_metrics_flush(blk_metrics, b, slots.cur);   // only this wavefront accumulated
    }
}

// proprioceptive part only, lane per env: used by wl_elev_observe (reset / get_observations path)
__global__ void __launch_bounds__(kBlock) elev_prop_kernel(const WlElevParams p, const WlEnvBuffers b, float* __restrict__ obs) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= b.n_envs) return;
    const Rows S = make_rows(b.state, b.stride);
    const V3 pos = ld3(S, WL_S_PX, e);
    const Quat q{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    const Mat3 R = mat_from_quat(q);
    write_elev_prop<1>(p, obs + (int64_t)e * WL_ELEV_OBS_DIM, pos, q, mul_t(R, ld3(S, WL_S_VX, e)), mul_t(R, ld3(S, WL_S_WX, e)),
                       S.ld(WL_S_CMD_BX, e), S.ld(WL_S_CMD_BY, e), S.ld(WL_S_ACT0, e), S.ld(WL_S_ACT1, e), 0, true);
}

__global__ void __launch_bounds__(kBlock) elev_reset_kernel(const WlElevParams p, const WlEnvBuffers b, const HeightFieldGround ground,
                                                            const uint8_t* __restrict__ mask, uint64_t seed, uint64_t step) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= b.n_envs) return;
    if (mask && !mask[e]) return;
    const Rows S = make_rows(b.state, b.stride);
    const uint32_t gid = (uint32_t)(b.env_offset + e);
    ElevReset rd;
    if (p.levels.level) {      // on the env's tile as it stands: a masked reset is no episode end, the level stays
        rd = draw_elev_reset_local(p, gid, step, seed);
        place_elev_reset(p, ground, rd, tile_origin(p.levels, e, p.levels.level[e]));
    } else {
        rd = draw_elev_reset(p, ground, gid, step, seed);
    }
    store_reset_rows(S, b, e, rd.pos, rd.q, v3(rd.vx, rd.vy, 0.f));
    S.st(WL_S_TGT_X, e, rd.tgt_x);
    S.st(WL_S_TGT_Y, e, rd.tgt_y);
    S.st(WL_S_TGT_H, e, rd.tgt_h);
    S.st(WL_S_CMD_TIMER, e, p.cmd_resample_s);
    float c, sn;
    yaw_cs(rd.q, c, sn);
    const float dx = rd.tgt_x - rd.pos.x, dy = rd.tgt_y - rd.pos.y;
    S.st(WL_S_CMD_BX, e, fmaf(c, dx, sn * dy));
    S.st(WL_S_CMD_BY, e, fmaf(-sn, dx, c * dy));
}

__global__ void __launch_bounds__(kBlock) elev_mdp_kernel(const WlElevParams p, int n, int64_t stride, const float* __restrict__ pos,
                                                          const float* __restrict__ quat, const float* __restrict__ vb_,
                                                          const float* __restrict__ vw_, const float* __restrict__ wheel,
                                                          const float* __restrict__ cmd, const uint8_t* __restrict__ timed_out,
                                                          int n_rays, const float* __restrict__ sensor_z,
                                                          const float* __restrict__ hit_z, float* __restrict__ terms,
                                                          uint8_t* __restrict__ flags, float* __restrict__ goal_rel,
                                                          float* __restrict__ hmap) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const V3 P = v3(pos[e], pos[stride + e], pos[2 * stride + e]);
    const Quat q{quat[e], quat[stride + e], quat[2 * stride + e], quat[3 * stride + e]};
    const V3 vb = v3(vb_[e], vb_[stride + e], vb_[2 * stride + e]);
    const V3 vw = v3(vw_[e], vw_[stride + e], vw_[2 * stride + e]);
    const float ws = wheel[e] + wheel[stride + e] + wheel[2 * stride + e] + wheel[3 * stride + e];
    const float cbx = cmd[e], cby = cmd[stride + e];
    const Mat3 R = mat_from_quat(q);
    const ElevTerms tm = elev_terms(p, P, R.r2.z, vb, vw, ws, cbx, cby, timed_out ? timed_out[e] != 0 : false);
#pragma unroll
    for (int i = 0; i < WL_ER_NTERMS; ++i) terms[i * stride + e] = tm.t[i];
#pragma unroll
    for (int i = 0; i < WL_ET_NTERMS; ++i) flags[i * stride + e] = tm.flag[i] ? 1 : 0;
    const float gx = cbx - P.x, gy = cby - P.y;
    goal_rel[e] = nan_to_num(gx);
    goal_rel[stride + e] = nan_to_num(gy);
    if (hit_z) {
        const float sz = sensor_z[e];
        for (int k = 0; k < n_rays; ++k) hmap[k * stride + e] = -(sz - hit_z[k * stride + e] - p.scan_offset) + (P.z - p.elev_z0);
    }
}

// WlTerrainLevels: all zero (off), or all of it
int check_levels(const WlTerrainLevels& tl) {
    if (!tl.level) return (tl.type || tl.origins || tl.rows != 0 || tl.cols != 0) ? WL_EINVAL : WL_OK;
    if (!tl.type || !tl.origins || tl.rows < 1 || tl.cols < 1 || (int64_t)tl.rows * tl.cols > 0x3fffffffLL) return WL_EINVAL;
    if (((uintptr_t)tl.level & 3u) || ((uintptr_t)tl.type & 3u) || ((uintptr_t)tl.origins & 3u)) return WL_EALIGN;
    return WL_OK;
}
// Which LEVELS instantiation a launch takes -- without terrain levels, the code that never knew of them.  Calls launch(lv) with lv a
// std::true_type / std::false_type (a template argument of the kernel).
template <class F>
inline void launch_levels(const WlElevParams* p, F&& launch) {
    if (p->levels.level != nullptr) launch(std::true_type{});
    else launch(std::false_type{});
}
int check_elev(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf) {
    int rc = check_implicit_env(p, b);
    if (rc == WL_OK) rc = heightfield_args_ok(hf, HF_PAIRS);
    return rc != WL_OK ? rc : check_levels(p->levels);
}

// pair[j][i] = code[j][i] | code[min(j + 1, ny - 1)][i] << 16
__global__ void __launch_bounds__(256) heightfield_pairs_kernel(const int16_t* __restrict__ height, uint32_t* __restrict__ pair, int nx, int ny) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)nx * ny) return;
    const int64_t up = k + nx < (int64_t)nx * ny ? k + nx : k;
    pair[k] = (uint32_t)(uint16_t)height[k] | (uint32_t)(uint16_t)height[up] << 16;
}


}  // namespace

extern "C" {
#if WL_FUSED_TIMELINE
int wl_debug_fused_timeline(unsigned long long* host_dst /* [2048][16] */) {
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(wl_timeline), sizeof(unsigned long long) * 2048 * 16);
}
#endif

int wl_heightfield_pairs(const WlHeightField* hf, uint32_t* pair_out, void* stream) {
    if (!hf || !hf->height || !pair_out || hf->nx < 2 || hf->ny < 2) return WL_EINVAL;
    if ((uintptr_t)pair_out & 3u) return WL_EALIGN;
    clear_error();
    const int64_t n = (int64_t)hf->nx * hf->ny;
    heightfield_pairs_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(hf->height, pair_out, hf->nx, hf->ny);
    return launch_status();
}

int wl_elev_step(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* actions,
                 const WlStepOut* out, uint64_t seed, uint64_t step, void* stream) {
    return wl_elev_rollout(p, b, hf, actions, out, 0, 0, 1, seed, step, stream);
}

int wl_elev_rollout(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* actions,
                    const WlStepOut* out, int64_t obs_step_stride, int64_t vec_step_stride, int32_t n_steps, uint64_t seed,
                    uint64_t step0, void* stream) {
    int rc = check_elev(p, b, hf);
    if (rc != WL_OK) return rc;
    if (!actions || !step_out_ok(out) || n_steps < 0) return WL_EINVAL;
    const HeightFieldGround g = make_ground(hf);
    const VehDerived vd = derive_vehicle(p->vehicle, p->sim_dt, p->decimation);
    // step + scan in one launch up to three 16-env blocks per CU; beyond, the lane-form step + the scan launch (round 6, us per step, fused /
    // two launches, profiles/r06_fused_crossover.txt: 8192 envs 30.9 / 43.8, 12 288: 44.8 / 48.5, 16 384: 58.9 / 52.4, 32 768: 114.5 / 72.2;
    // round 4: 8192 envs 48.5 fused; 16 384 envs 92.5 / 75.4)
    const bool quad = use_quad(b) && (b->lanes == 4 || b->n_envs <= WL_ELEV_FUSED_MAX_ENVS);
    const ElevHead h = elev_head(p);
    const dim3 fused_grid((b->n_envs + kFusedEnvs - 1) / kFusedEnvs), lane_grid(grid_for(b->n_envs));
    clear_error();
    for (int k = 0; k < n_steps; ++k) {
        const WlStepOut o = step_out_at(*out, k, obs_step_stride, vec_step_stride);
        const float2* a = (const float2*)(actions + (int64_t)k * b->n_envs * 2);
        // (one launch_levels per kernel, not one around the if: keeps the emission order of the kernels)
        if (quad) {   // step + scan in one launch
            launch_levels(p, [&](auto lv) {
                elev_step_scan_kernel<decltype(lv)::value><<<fused_grid, kFusedThreads, 0, (hipStream_t)stream>>>(h, vd, *b, g, a, o, seed, step0 + (uint64_t)k, p->levels);
            });
        } else {
            launch_levels(p, [&](auto lv) {
                elev_step_kernel<decltype(lv)::value><<<lane_grid, kBlock, 0, (hipStream_t)stream>>>(h, vd, *b, g, a, o, seed, step0 + (uint64_t)k, p->levels);
            });
            launch_elev_scan(p, b, g, o.obs, (hipStream_t)stream);
        }
    }
    return launch_status();
}

int wl_elev_collect_rollout(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const WlMlp* actor, const WlMlp* critic,
                            const float* std, const WlCollectIo* io, const WlStepOut* out, int32_t n_steps, int32_t deterministic,
                            uint64_t seed, uint64_t step0, void* stream) {
    int rc = check_elev(p, b, hf);
    if (rc != WL_OK) return rc;
    if (!use_quad(b)) return WL_EINVAL;   // the quad form's (n <= 32 768); beyond: act + step
    if (!actor || !critic || !std || !io || !io->obs_in || !io->actions || !io->mu || !io->log_prob || !io->values || n_steps < 0) return WL_EINVAL;
    if (!step_out_ok(out)) return WL_EINVAL;
    for (const WlMlp* m : {actor, critic})
        if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->w3 || !m->b3 || m->hidden != kMlpHidden || m->in_dim != WL_ELEV_OBS_DIM ||
            (m->activation != WL_ACT_ELU && m->activation != WL_ACT_RELU))
            return WL_EINVAL;
    if (actor->out_dim != 2 || critic->out_dim != 1 || actor->activation != critic->activation) return WL_EINVAL;
    if (((uintptr_t)io->actions & 7u) || ((uintptr_t)io->mu & 7u) || ((uintptr_t)io->obs_in & 3u)) return WL_EALIGN;
    // rows k of a [K + 1][n][689] observation block: the kernel writes row k + 1 where the caller's policy would read it
    if (out->obs != io->obs_in + (int64_t)b->n_envs * WL_ELEV_OBS_DIM) return WL_EINVAL;
    if (ring_aliases(b, n_steps)) return WL_EINVAL;
    const HeightFieldGround g = make_ground(hf);
    const VehDerived vd = derive_vehicle(p->vehicle, p->sim_dt, p->decimation);
    const PolicyIo pio{*actor, *critic, std, io->obs_in, io->actions, io->mu, io->log_prob, io->values, deterministic};
    const int grid = (b->n_envs + kFusedEnvs - 1) / kFusedEnvs;
    const size_t lds_bytes = (size_t)kColLdsFloats * 4;
    using Kernel = void (*)(ElevHead, VehDerived, WlEnvBuffers, HeightFieldGround, WlStepOut, int, uint64_t, uint64_t, PolicyIo, MetricSlots, WlTerrainLevels);
    static const Kernel kernels[2][2] = {{elev_collect_rollout_kernel<WL_ACT_RELU, false>, elev_collect_rollout_kernel<WL_ACT_RELU, true>},
                                         {elev_collect_rollout_kernel<WL_ACT_ELU, false>, elev_collect_rollout_kernel<WL_ACT_ELU, true>}};
    static bool attr_set = false;
    if (!attr_set) {
        for (const auto& row : kernels)
            for (const Kernel k : row) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        attr_set = true;
    }
    const MetricSlots ms = metric_slots(b, step0, (uint64_t)n_steps);
    clear_error();
    launch_levels(p, [&](auto lv) {
        kernels[actor->activation == WL_ACT_ELU][decltype(lv)::value]<<<grid, kFusedThreads, lds_bytes, (hipStream_t)stream>>>(
            elev_head(p), vd, *b, g, *out, n_steps, seed, step0, pio, ms, p->levels);
    });
    return launch_status();
}

int wl_elev_rollout_persistent(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* actions,
                               const WlStepOut* out, int64_t obs_step_stride, int64_t vec_step_stride, int32_t n_steps, uint64_t seed,
                               uint64_t step0, void* stream) {
    int rc = check_elev(p, b, hf);
    if (rc != WL_OK) return rc;
    if (!use_quad(b)) return WL_EINVAL;   // the quad form's (n <= 32 768)
    if (!actions || !step_out_ok(out) || n_steps < 0) return WL_EINVAL;
    if (n_steps > 1 && obs_step_stride < (int64_t)b->n_envs * WL_ELEV_OBS_DIM) return WL_EINVAL;   // the scan runs a step behind: rows must differ
    if (ring_aliases(b, n_steps)) return WL_EINVAL;
    clear_error();
    launch_levels(p, [&](auto lv) {
        elev_rollout_persistent_kernel<decltype(lv)::value><<<(b->n_envs + kFusedEnvs - 1) / kFusedEnvs, kFusedThreads, 0, (hipStream_t)stream>>>(
            elev_head(p), derive_vehicle(p->vehicle, p->sim_dt, p->decimation), *b, make_ground(hf), (const float2*)actions, *out, obs_step_stride,
            vec_step_stride, n_steps, seed, step0, metric_slots(b, step0, (uint64_t)n_steps), p->levels);
    });
    return launch_status();
}

int wl_elev_reset(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const uint8_t* mask, uint64_t seed,
                  uint64_t step, void* stream) {
    int rc = check_elev(p, b, hf);
    if (rc != WL_OK) return rc;
    clear_error();
    elev_reset_kernel<<<grid_for(b->n_envs), kBlock, 0, (hipStream_t)stream>>>(*p, *b, make_ground(hf), mask, seed, step);
    return launch_status();
}

int wl_elev_observe(const WlElevParams* p, const WlEnvBuffers* b, const WlHeightField* hf, float* obs, void* stream) {
    int rc = check_elev(p, b, hf);
    if (rc != WL_OK) return rc;
    if (!obs) return WL_EINVAL;
    clear_error();
    elev_prop_kernel<<<grid_for(b->n_envs), kBlock, 0, (hipStream_t)stream>>>(*p, *b, obs);
    launch_elev_scan(p, b, make_ground(hf), obs, (hipStream_t)stream);
    return launch_status();
}

int wl_elev_mdp(const WlElevParams* p, int32_t n, int64_t stride, const float* pos, const float* quat, const float* lin_vel_b,
                const float* lin_vel_w, const float* wheel_vel, const float* command, const uint8_t* timed_out, int32_t n_rays,
                const float* sensor_z, const float* hit_z, float* terms, uint8_t* flags, float* goal_rel, float* height_map,
                void* stream) {
    if (!p || n <= 0 || stride < n || !pos || !quat || !lin_vel_b || !lin_vel_w || !wheel_vel || !command || !terms || !flags ||
        !goal_rel)
        return WL_EINVAL;
    if (hit_z && (!sensor_z || !height_map || n_rays <= 0)) return WL_EINVAL;
    clear_error();
    elev_mdp_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(*p, n, stride, pos, quat, lin_vel_b, lin_vel_w, wheel_vel,
                                                                      command, timed_out, n_rays, sensor_z, hit_z, terms, flags,
                                                                      goal_rel, height_map);
    return launch_status();
}

}  // extern "C"

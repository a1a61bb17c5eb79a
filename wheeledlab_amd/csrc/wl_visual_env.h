// wl_visual_env.h -- device code of ONE visual-task env.step() (wheeledlab_tasks/visual/mushr_visual_env_cfg.py) on a register image
// of the env's state rows: 4WD action term -> sub-steps on the flat plane (or a heightfield) -> time_out / out_of_map ->
// traversable_reward (byte-map gather) + forward_vel -> reset onto a random traversable cell.  The traversability-map lookups, the
// reset draw, what the camera takes over from the step (CamPose), the quad form's argument head and visual_env_step<LANES, Ground,
// RESET_SRC> itself.  The kernels are in wl_visual.hip, the camera in wl_visual_cam_dev.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_rng.h"
#include "wl_implicit_task.h"

namespace {

// TraversabilityHashmapUtil.get_map_id (visual/utils/traversability_utils.py:83-88): float32 arithmetic, truncation
// toward zero (`.long()`), clamp to the map.
WL_DEV void map_id(const WlTravMap& m, float x, float y, int& xi, int& yi) {
    const float width = (float)m.rows * m.row_spacing, height = (float)m.cols * m.col_spacing;
    const float fx = (x + 0.5f * width + 0.5f * m.row_spacing) / m.row_spacing;
    const float fy = (y + 0.5f * height + 0.5f * m.col_spacing) / m.col_spacing;
    // float -> int conversion saturates on gfx950 (v_cvt_i32_f32), NaN -> 0: both end up clamped like torch's long()
    xi = min(max((int)fx, 0), m.rows - 1);
    yi = min(max((int)fy, 0), m.cols - 1);
}
WL_DEV bool traversable(const WlTravMap& m, float x, float y) {
    int xi, yi;
    map_id(m, x, y, xi, yi);
    return m.map[yi * m.cols + xi] != 0;   // map[y_idx, x_idx] (:78)
}
// out_of_map (mushr_visual_env_cfg.py:390-398)
WL_DEV bool out_of_map(const WlTravMap& m, float x, float y) {
    const float hw = 0.5f * (float)m.rows * m.row_spacing, hh = 0.5f * (float)m.cols * m.col_spacing;
    return x > hw || x < -hw || y > hh || y < -hh;
}

struct VisReset {
    V3 pos;
    Quat q;
};
// visual/mdp/events.py:11-42 + generate_random_poses (utils/__init__.py:188-202): random traversable cell, z 0.1,
// yaw U(0, 360 deg), zero velocity
WL_DEV VisReset draw_visual_reset(const WlVisualParams& p, const WlTravMap& m, uint32_t gid, uint64_t step, uint64_t seed) {
    const F4 u = philox_uniform4(gid, step, 0, seed);
    const int k = min((int)(u.x * (float)m.n_cells), m.n_cells - 1);
    const int iy = m.cells[2 * k], ix = m.cells[2 * k + 1];
    VisReset r;
    r.pos = v3(((float)ix - (float)(m.cols / 2)) * m.row_spacing, ((float)iy - (float)(m.rows / 2)) * m.col_spacing, p.reset_z);
    float s, c;
    sincos_rev(0.5f * u.y, s, c);   // yaw = 2 pi u  ->  yaw / 2 = u / 2 revolutions
    r.q = Quat{c, 0.f, 0.f, s};
    return r;
}
// a resetting env's new pose: the draw + (on a heightfield) the lift onto the terrain under the spawn cell
template <class Ground>
WL_DEV VisReset visual_reset_pose(const WlVisualParams& p, const WlTravMap& m, const Ground& ground, uint32_t gid, uint64_t step, uint64_t seed) {
    VisReset rd = draw_visual_reset(p, m, gid, step, seed);
    if constexpr (!Ground::kFlat) {     // z 0.1 above the plane -> 0.1 above the terrain under the spawn cell
        float zt;
        V3 nt;
        ground.sample(rd.pos.x, rd.pos.y, zt, nt);
        rd.pos.z += zt;
    }
    return rd;
}

// what the camera needs of an env after its step: exactly the values the step leaves in the state rows (post-reset)
struct CamPose {
    float px, py, pz, qw, qx, qy, qz, vx, vy, vz, wx, wy, wz, a0, a1;
};

// the 8 proprioceptive observation values (VisualObsCfg.PolicyCfg :38-58): base_lin_vel (3) | base_ang_vel (3) | last_action clipped
// to +-1 (2), from the body's rotation and its world-frame velocities.  (The step writes them on a heightfield, the camera on the
// plane; wl_depth.hip visual_depth_prop_kernel keeps its own copy: through this function its machine code changes)
WL_DEV void store_proprio(float* t, const Mat3& R, V3 v, V3 w, float a0, float a1) {
    const V3 vb = mul_t(R, v), wb = mul_t(R, w);
    t[0] = vb.x, t[1] = vb.y, t[2] = vb.z, t[3] = wb.x, t[4] = wb.y, t[5] = wb.z;
    t[6] = clampf(a0, -1.f, 1.f), t[7] = clampf(a1, -1.f, 1.f);
}

// the quad form's argument head (latency form): both argument structs as ONE burst of vector loads instead of dependent scalar-load
// round trips (two copies: a wait in the middle, see kernarg_vector_copy2); the integer fields that steer scalar control flow stay
// with the scalar copy of the arguments
WL_DEV void visual_kernarg_copy(WlVisualParams& p, VehDerived& vd, const WlVisualParams& p_arg, const VehDerived& vd_arg) {
    kernarg_vector_copy2(0, p, vd);
    keep_scalar_common(p, p_arg);
    vd.n_sub = vd_arg.n_sub;
}

// one env.step() of env e (lane form: one lane; quad form: the four lanes of a quad, wid = wheel).  Ground: the flat plane of the
// reference's task, or a heightfield (the visual-depth extension task, BASELINE config 5: wheel contacts by bilinear gathers as in
// the elevation task, reset poses lifted onto the terrain; `prop`: the env's 8 proprioceptive observation values are written
// there -- the depth image next to them comes from wl_depth.hip).  `rows` are the env's rows as loaded; they leave as stored.
// RESET_SRC: where a resetting env's pose comes from (wl_implicit_task.h).  By default drawn on the spot; the quad-form step kernel of
// the small batches on a heightfield has a helper wavefront draw the block's resets while the physics runs (round 6): the draw is two
// or three DEPENDENT memory round trips (Philox -> the spawn-cell table -> on a heightfield the terrain under the cell) behind the last
// sub-step, with mean episodes of ~50 steps every other block of 32 envs has one per step, and the launch is as long as its slowest block.
template <int LANES, class Ground = FlatGround, class RESET_SRC = InlineReset>
WL_DEV CamPose visual_env_step(const WlVisualParams& p, const VehDerived& vd, const WlEnvBuffers& b, const WlTravMap& m, float2 a,
                               VehRows<LANES>& rows, const WlStepOut& out, const uint64_t seed, const uint64_t step, const Rows& S,
                               const int e, const int wid, const bool lead, float* blk_metrics, const Ground ground = Ground{},
                               float* __restrict__ prop = nullptr, const RESET_SRC& reset_src = RESET_SRC()) {
    const WlVehicleParams& vp = p.vehicle;
    const uint32_t gid = (uint32_t)(b.env_offset + e);
    const EnvConst ec = veh_env_const<LANES>(p.action, vp, vd, a, rows, wid);
    VehState s = veh_state<LANES>(vp, rows);
    // bookkeeping rows: the quad form (one wavefront per SIMD, registers to spare) requests them BEFORE the physics loop
    // and finds them landed behind it; the lane form fetches them after it (registers are worth more there)
    int ep_len_in = 0;
    float epsum_in[WL_VR_NTERMS];
#pragma unroll
    for (int i = 0; i < WL_VR_NTERMS; ++i) epsum_in[i] = 0.f;
    auto fetch_bookkeeping = [&]() {
        ep_len_in = b.episode_len[e];
        if (p.log_episode_sums) {
#pragma unroll
            for (int i = 0; i < WL_VR_NTERMS; ++i) epsum_in[i] = S.ld(WL_S_EPSUM0 + i, e);
        }
    };
    if constexpr (LANES == 4) fetch_bookkeeping();
    veh_integrate<LANES>(vp, vd, ec, s, ground, wid);
    if constexpr (LANES != 4) {
        asm volatile("" ::: "memory");
        fetch_bookkeeping();
    }
    VehPost v = veh_post<LANES>(vp, s);
    int ep_len = ep_len_in + 1;
    const bool truncated = ep_len >= p.max_episode_length;
    const bool oom[1] = {v.finite && out_of_map(m, v.pos.x, v.pos.y)};
    const bool terminated = !v.finite || oom[0];
    float t[WL_VR_NTERMS];
    t[WL_VR_TRAVERSABLE] = v.finite ? (traversable(m, v.pos.x, v.pos.y) ? 1.f : -1.f) : 0.f;   // :309-312
    t[WL_VR_FORWARD_VEL] = v.vb.x;                                                              // :370-371
    float epsum[WL_VR_NTERMS];
    const float reward = weigh_rewards(p.weight, t, v.finite, p.sim_dt * (float)p.decimation, p.log_episode_sums != 0, epsum_in, epsum);
    if (lead) write_step_flags(out, e, reward, terminated, truncated);
    float a0 = a.x, a1 = a.y;
    if (terminated || truncated) {
        if (lead) episode_end_metrics(blk_metrics, epsum, truncated, v.finite, oom, ep_len);
        const VisReset rd = reset_src(e, [&] { return visual_reset_pose(p, m, ground, gid, step, seed); });
        veh_reset(s, v, epsum, rd.pos, rd.q, v3(0.f, 0.f, 0.f));
        ep_len = 0;
        a0 = a1 = 0.f;
    }
    veh_rows_from(rows, s, v);
    store_veh_rows<LANES>(S, e, wid, lead, rows, a0, a1, p.log_episode_sums != 0, epsum);
    if (lead) {
        b.episode_len[e] = ep_len;
        if (prop) store_proprio(prop, mat_from_quat(s.q), s.v, v.ww, a0, a1);   // of the post-reset state
    }
    return CamPose{v.pos.x, v.pos.y, v.pos.z, s.q.w, s.q.x, s.q.y, s.q.z, s.v.x, s.v.y, s.v.z, v.ww.x, v.ww.y, v.ww.z, a0, a1};
}

}  // namespace

// wl_implicit_task.h -- what the elevation task (wl_elev.hip) and the visual task (wl_visual.hip) share: both step the same vehicle
// with the linearly implicit integrator on the same WL_S_* state rows.  Plain building blocks that each task's env step calls in
// its own order (elevation hands its pose to the fused launch's height scan before it weights its rewards), the helper wavefront
// that draws a block's resets while the physics runs, the per-step outputs of a rollout, and the host-side argument check of the
// env buffers.
#pragma once
#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_drift_terms.h"   // process_action / joint_targets (shared action term)
#include "wl_vehicle.h"
#include "wl_heightfield.h"

namespace {

// the dynamic rows of an env as the step needs them at its start (requested in one go, ahead of the parameter block)
template <int LANES>
struct VehRows {
    float mass, mu_s, mu_d, damp;
    V3 pos, v, ww;
    Quat q;
    float wheel[LANES == 1 ? 4 : 1];
    float th, om;
};
template <int LANES>
WL_DEV VehRows<LANES> load_veh_rows(const Rows& S, int e, int wid) {
    VehRows<LANES> r;
    r.mass = S.ld(WL_S_MASS, e), r.mu_s = S.ld(WL_S_MU_S, e), r.mu_d = S.ld(WL_S_MU_D, e), r.damp = S.ld(WL_S_DAMP, e);
    r.pos = ld3(S, WL_S_PX, e);
    r.q = Quat{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    r.v = ld3(S, WL_S_VX, e);
    r.ww = ld3(S, WL_S_WX, e);
    if constexpr (LANES == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r.wheel[i] = S.ld(WL_S_WHEEL_BL + i, e);
    } else {
        r.wheel[0] = S.ld(WL_S_WHEEL_BL + wid, e);
    }
    r.th = S.ld(WL_S_STEER_POS, e);
    r.om = S.ld(WL_S_STEER_VEL, e);
    return r;
}
// the vehicle half of the row store: the wheel spins (each lane of a quad its own), and by the lead lane the body, the steering,
// the last action and the episode sums
template <int LANES, int N>
WL_DEV void store_veh_rows(const Rows& S, int e, int wid, bool lead, const VehRows<LANES>& r, float a0, float a1, bool log_sums,
                           const float (&epsum)[N]) {
    if constexpr (LANES == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) S.st(WL_S_WHEEL_BL + i, e, r.wheel[i]);
    } else {
        S.st(WL_S_WHEEL_BL + wid, e, r.wheel[0]);
    }
    if (lead) {
        st3(S, WL_S_PX, e, r.pos);
        S.st(WL_S_QW, e, r.q.w);
        S.st(WL_S_QX, e, r.q.x);
        S.st(WL_S_QY, e, r.q.y);
        S.st(WL_S_QZ, e, r.q.z);
        st3(S, WL_S_VX, e, r.v);
        st3(S, WL_S_WX, e, r.ww);
        S.st(WL_S_STEER_POS, e, r.th);
        S.st(WL_S_STEER_VEL, e, r.om);
        S.st(WL_S_ACT0, e, a0);
        S.st(WL_S_ACT1, e, a1);
        if (log_sums) {
#pragma unroll
            for (int i = 0; i < N; ++i) S.st(WL_S_EPSUM0 + i, e, epsum[i]);
        }
    }
}

// the action term and the env's constants of the step; `a` leaves as the processed action (what the step stores as the last action)
template <int LANES>
WL_DEV EnvConst veh_env_const(const WlActionParams& ap, const WlVehicleParams& vp, const VehDerived& vd, float2& a,
                              const VehRows<LANES>& r, int wid) {
    float v_t, delta;
    process_action(ap, a.x, a.y, v_t, delta);
    EnvConst ec;
    joint_targets(ap, v_t, delta, ec.steer_target, ec.wheel_target);
    env_const_rows(ec, vp, vd, r.mass, r.mu_s, r.mu_d, r.damp);
    if constexpr (LANES == 4) env_const_lane(ec, vp, vd, wid);
    return ec;
}
// the integrator's state from the rows (root position -> centre of mass, world -> body angular velocity)
template <int LANES>
WL_DEV VehState veh_state(const WlVehicleParams& vp, const VehRows<LANES>& r) {
    VehState s;
    s.q = r.q;
    s.v = r.v;
#pragma unroll
    for (int i = 0; i < (LANES == 1 ? 4 : 1); ++i) s.wheel[i] = r.wheel[i];
    s.th = r.th;
    s.om = r.om;
    const Mat3 R = mat_from_quat(s.q);
    s.x = r.pos + vp.cg_z * v3(R.r0.z, R.r1.z, R.r2.z);
    s.wb = mul_t(R, r.ww);
    return s;
}

#ifndef WL_WHEEL_CORNER_CACHE
#define WL_WHEEL_CORNER_CACHE 1
#endif
// decimation x sub-steps of the linearly implicit integrator
template <int LANES, class Ground>
WL_DEV void veh_integrate(const WlVehicleParams& vp, const VehDerived& vd, const EnvConst& ec, VehState& s, const Ground& ground, int wid) {
    if constexpr (LANES == 1 && !Ground::kFlat && WL_WHEEL_CORNER_CACHE) {   // lane form on a heightfield: see HeightFieldGroundCached
        const HeightFieldGroundCached cached(ground);
        vehicle_integrate<LANES, HeightFieldGroundCached, true, -1, true>(vp, vd, ec, s, cached, wid);
    } else {
        vehicle_integrate<LANES, Ground, true, -1, true>(vp, vd, ec, s, ground, wid);
    }
}

// the body as the integrator leaves it: root position, world angular and body-frame linear velocity, and whether the car is finite
struct VehPost {
    Mat3 R;
    V3 pos, ww, vb;
    float wheel_sum;
    bool finite;
};
template <int LANES>
WL_DEV VehPost veh_post(const WlVehicleParams& vp, const VehState& s) {
    VehPost o;
    o.R = mat_from_quat(s.q);
    o.ww = mul(o.R, s.wb);
    o.pos = s.x - vp.cg_z * v3(o.R.r0.z, o.R.r1.z, o.R.r2.z);
    if constexpr (LANES == 1) o.wheel_sum = s.wheel[0] + s.wheel[1] + s.wheel[2] + s.wheel[3];
    else o.wheel_sum = quad_sum(s.wheel[0]);
    const float chk = o.pos.x + o.pos.y + o.pos.z + s.q.w + s.q.x + s.q.y + s.q.z + s.v.x + s.v.y + s.v.z + o.ww.x + o.ww.y +
                      o.ww.z + o.wheel_sum + s.th + s.om;
    o.finite = __builtin_isfinite(chk);
    o.vb = mul_t(o.R, s.v);
    return o;
}

// the step's reward (weight x term x step_dt summed; nothing for a non-finite car) and the episode sums that carry it
template <int N>
WL_DEV float weigh_rewards(const float* weight, const float (&t)[N], bool finite, float step_dt, bool log_sums,
                           const float (&epsum_in)[N], float (&epsum)[N]) {
    float reward = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float w = weight[i];
        const float c = (w != 0.f && finite) ? t[i] * w * step_dt : 0.f;
        reward += c;
        epsum[i] = log_sums ? epsum_in[i] + c : 0.f;
    }
    return reward;
}
// the env's reward and flags of the step (lead lane)
WL_DEV void write_step_flags(const WlStepOut& out, int e, float reward, bool terminated, bool truncated) {
    out.reward[e] = reward;
    out.terminated[e] = terminated ? 1 : 0;
    out.truncated[e] = truncated ? 1 : 0;
    if (out.dones) out.dones[e] = (terminated || truncated) ? 1 : 0;
}
// an ending episode into the block's metrics (lead lane): its reward sums, the reset, a time-out, the termination terms that fired
// (counted for a finite car only), a non-finite car, the episode's length
template <int N, int T>
WL_DEV void episode_end_metrics(float* blk_metrics, const float (&epsum)[N], bool truncated, bool finite, const bool (&flag)[T], int ep_len) {
#pragma unroll
    for (int i = 0; i < N; ++i) atomicAdd(&blk_metrics[WL_M_EPSUM0 + i], epsum[i]);
    atomicAdd(&blk_metrics[WL_M_RESETS], 1.f);
    if (truncated) atomicAdd(&blk_metrics[WL_M_TIMEOUTS], 1.f);
#pragma unroll
    for (int k = 0; k < T; ++k)
        if (finite && flag[k]) atomicAdd(&blk_metrics[WL_M_TERM0 + k], 1.f);
    if (!finite) atomicAdd(&blk_metrics[WL_M_NONFINITE], 1.f);
    atomicAdd(&blk_metrics[WL_M_EPLEN], (float)ep_len);
}
// a resetting env: the episode sums restart, a non-finite car's wheel spins and steering are zeroed, the drawn pose and velocity
// replace the body's
template <int N>
WL_DEV void veh_reset(VehState& s, VehPost& o, float (&epsum)[N], V3 pos, Quat q, V3 v) {
#pragma unroll
    for (int i = 0; i < N; ++i) epsum[i] = 0.f;
    if (!o.finite) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s.wheel[i] = 0.f;
        s.th = s.om = 0.f;
    }
    o.pos = pos;
    s.q = q;
    s.v = v;
    o.ww = v3(0.f, 0.f, 0.f);
}
// the env's new rows from the step's state
template <int LANES>
WL_DEV void veh_rows_from(VehRows<LANES>& r, const VehState& s, const VehPost& o) {
    r.pos = o.pos, r.q = s.q, r.v = s.v, r.ww = o.ww, r.th = s.th, r.om = s.om;
#pragma unroll
    for (int i = 0; i < (LANES == 1 ? 4 : 1); ++i) r.wheel[i] = s.wheel[i];
}

// ---- where a resetting env's draw comes from: `src(e, draw)` with `draw()` the task's own draw for env e ----
// A helper wavefront draws the block's resets while the physics runs (round 6): the draw depends on (seed, env, step) and the terrain
// only, and with a reset somewhere in nearly every launch the elevation draw's ~0.9 us (two Philox blocks, a terrain sample's round
// trip, sin / cos) was on the fused launch's critical path (the visual draw: wl_visual_env.h visual_env_step).  ResetHelper lives in LDS.
struct InlineReset {
    template <class F>
    WL_DEV auto operator()(int, F draw) const { return draw(); }
};
template <class DRAW, int N>
struct ResetHelper {
    int ready;
    DRAW slot[N];
    WL_DEV void init() {   // before the block's first barrier
        if (threadIdx.x == 0) ready = 0;
    }
    // lane j of the helper wavefront: env j's draw into slot j (if the block has that env), then, behind every lane's slot, the flag
    template <class F>
    WL_DEV void publish(int j, bool have, F draw) {
        if (have) slot[j] = draw();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (j == 0) __hip_atomic_store(&ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // env j's draw: the helper set the flag long ago (its draws take ~1.5 us, this is ~8 us into the launch); the loop is the guarantee
    WL_DEV DRAW take(int j) {
        while (__hip_atomic_load(&ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
        return slot[j];
    }
};
// the physics side of a ResetHelper (`on`, a compile-time constant at every use: false draws on the spot instead)
template <class DRAW, int N>
struct HelperReset {
    ResetHelper<DRAW, N>* h;
    int e0;
    bool on;
    template <class F>
    WL_DEV DRAW operator()(int e, F draw) const { return on ? h->take(e - e0) : draw(); }
};

// the env-buffer half of check_elev / check_visual (P: their parameter struct)
template <class P>
inline int check_implicit_env(const P* p, const WlEnvBuffers* b) {
    if (!p || !b || !b->state || !b->episode_len || !b->metrics) return WL_EINVAL;
    if (b->n_envs <= 0 || b->stride < b->n_envs || b->metrics_slots < 1) return WL_EINVAL;
    if (b->stride % 64 != 0 || ((uintptr_t)b->state & 15u)) return WL_EALIGN;
    if (b->stride * 4 * WL_S_COUNT > 0x7fffffffLL || (b->lanes != 0 && b->lanes != 1 && b->lanes != 4)) return WL_EINVAL;
    if (!flags_ok(b)) return WL_EINVAL;
    if (p->decimation <= 0 || p->vehicle.substeps <= 0 || !(p->sim_dt > 0.f)) return WL_EINVAL;
    if (p->vehicle.implicit != 1 || !(p->vehicle.susp_fmax > 0.f)) return WL_EINVAL;   // these kernels step the linearly implicit integrator (wl_vehicle.h)
    return WL_OK;
}

}  // namespace

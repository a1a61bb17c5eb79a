// wl_elev_env.h -- device code of ONE elevation-task env.step() on a register image of the env's state rows: the mdp terms, the
// proprioceptive observation values, the reset draws and the terrain curriculum's levels, the env's bookkeeping (ElevBook), the
// step kernels' argument head and elev_env_step<LANES, LEVELS, PERSIST> itself.  The kernels are in wl_elev.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_rng.h"
#include "wl_implicit_task.h"
#include "wl_elev_scan_dev.h"

#ifndef WL_TL   // the fused launch's timeline stamps (debug builds: wl_elev.hip defines it before it includes this header)
#define WL_TL(slot) do { } while (0)
#endif

namespace {

enum ElevStream : uint32_t { ES_RESET = 0, ES_CMD_RESET = 1, ES_CMD_RESAMPLE = 2, ES_LEVEL = 3 /* the terrain curriculum's wrap draw */ };

// cos / sin of the yaw of IsaacLab's yaw_quat(q) without the atan2 round trip
WL_DEV void yaw_cs(Quat q, float& c, float& s) {
    // every multiply-add spelled out: under -ffp-contract=fast the compiler picks WHICH product of a sum of products it fuses per
    // inlining site, and two sites of one kernel then round differently (round 4: the first and the later envs of a persistent
    // scan block disagreed in the last bit)
    const float a = fmaf(-2.f, fmaf(q.z, q.z, q.y * q.y), 1.f), hb = fmaf(q.w, q.z, q.x * q.y), b = hb + hb;
    const float inv = rsq(fmaf(a, a, b * b));
    c = a * inv;
    s = b * inv;
}

WL_DEV float sym(float u, float a) { return (2.f * u - 1.f) * a; }

// torch.nan_to_num(x, nan=0) (:55): nan -> 0, and +-inf -> +-FLT_MAX (its default posinf / neginf)
WL_DEV float nan_to_num(float x) { return x != x ? 0.f : fminf(fmaxf(x, -3.40282347e38f), 3.40282347e38f); }

struct ElevTerms {
    float t[WL_ER_NTERMS];
    bool flag[WL_ET_NTERMS];
};

// elevation mdp terms (citations: mushr_elevation_env_cfg.py)
WL_DEV ElevTerms elev_terms(const WlElevParams& p, V3 pos, float up_dot, V3 vb, V3 vw, float wheel_sum, float cbx, float cby,
                            bool timed_out) {
    ElevTerms r;
    const float gx = cbx - pos.x, gy = cby - pos.y;   // goal vector: base-frame command minus world position (:50-55 quirk)
    r.flag[WL_ET_BELOW_MIN_HEIGHT] = pos.z < p.min_height;                                            // :356-359
    r.flag[WL_ET_STUCK] = fminf(vb.x, p.stuck_vel_cap) < p.stuck_min_vel && wheel_sum > p.stuck_wheel_spin;   // :342-347
    // :217-222, 339-340: rad2deg(arccos(R33)) > 60 in fp32 is 60.000004 at R33 = 0.5 exactly, so the tie counts as rolled over
    r.flag[WL_ET_ROLLOVER] = up_dot <= p.upright_cos;
    const float g2 = fmaf(gx, gx, gy * gy);
    // :268-273: torch.norm of a 2-vector is the correctly rounded sqrt of fma(y, y, x * x) -- that product order, not v_sqrt_f32
    r.flag[WL_ET_AT_GOAL] = sqrtf(fmaf(gy, gy, gx * gx)) < p.goal_dist;
    r.t[WL_ER_GOAL_PROGRESS] = p.progress_offset + fmaf(vw.x, gx, vw.y * gy) * rsq(g2);   // :239-249
    const float z = pos.z - p.elev_z0;
    r.t[WL_ER_HIGHER_ELEVATION] = clampf((z > p.elev_min && vb.x > p.elev_min_vel) ? z : 0.f, 0.f, 1.f);       // :166-173
    r.t[WL_ER_FALLING] = vb.z > p.fall_vel ? 1.f : 0.f;                                               // :251-254
    r.t[WL_ER_STUCK_PENALTY] = (r.flag[WL_ET_STUCK] && !timed_out) ? 1.f : 0.f;                       // :301-305
    return r;
}

// the 13 proprioceptive observation values of ElevationObsCfg.ConcatObs (:61-73), written straight into the env's
// observation row by the lane-per-env kernels (step / prop); the block-per-env scan kernel adds the 676 map values
template <int LANES>
WL_DEV void write_elev_prop(const WlElevParams& p, float* __restrict__ row, V3 pos, Quat q, V3 vb, V3 wb, float cbx, float cby,
                            float a0, float a1, int wid, bool lead, float* row2 = nullptr /* a second copy (the collector's LDS tile) */) {
    V3 eu;
    if constexpr (LANES == 4) {   // roll / pitch / yaw as one lane-parallel atan2 (asin x = atan2(x, sqrt(1 - x^2)))
        const float sp = 2.f * (q.w * q.y - q.z * q.x);
        const float ay = wid == 1 ? 2.f * (q.w * q.x + q.y * q.z) : wid == 2 ? sp : 2.f * (q.w * q.z + q.x * q.y);
        const float ax = wid == 1 ? 1.f - 2.f * (q.x * q.x + q.y * q.y) : wid == 2 ? fsqrt(fmaxf(1.f - sp * sp, 0.f))
                                                                                  : 1.f - 2.f * (q.y * q.y + q.z * q.z);
        const float ang = atan2_fast(ay, ax);
        eu = v3(wrap_2pi(quad_bcast<1>(ang)), wrap_2pi(quad_bcast<2>(ang)), wrap_2pi(quad_bcast<3>(ang)));
    } else {
        eu = euler_xyz_from_quat(q);
    }
    if (!lead) return;
    const float gx = cbx - pos.x, gy = cby - pos.y;
    const float v[13] = {nan_to_num(gx), nan_to_num(gy),
                         eu.x, eu.y, eu.z,
                         clampf(vb.x, -p.obs_clip, p.obs_clip), clampf(vb.y, -p.obs_clip, p.obs_clip), clampf(vb.z, -p.obs_clip, p.obs_clip),
                         clampf(wb.x, -p.obs_clip, p.obs_clip), clampf(wb.y, -p.obs_clip, p.obs_clip), clampf(wb.z, -p.obs_clip, p.obs_clip),
                         clampf(a0, -1.f, 1.f), clampf(a1, -1.f, 1.f)};
#pragma unroll
    for (int i = 0; i < 13; ++i) row[i] = v[i];
    if (row2) {
#pragma unroll
        for (int i = 0; i < 13; ++i) row2[i] = v[i];
    }
}

struct ElevReset {
    V3 pos;
    Quat q;
    float vx, vy, tgt_x, tgt_y, tgt_h;
};

// ---- terrain curriculum (WlTerrainLevels; IsaacLab TerrainImporter.update_env_origins + mdp.terrain_levels) -------------------------
// a + b as an addition of its own: under -ffp-contract=fast `origin + (2 u - 1) a` becomes an fma at one inlining site and not at
// the next (see yaw_cs), and every form must place a spawn on the same bits
WL_DEV float add_unfused(float a, float b) {
    float r;
    {
#pragma clang fp contract(off)
        r = a + b;
    }
    return r;
}
struct TileOrigin {
    float x, y;
};
// the centre of tile (level, type[e]); both indices clamped to the table
WL_DEV TileOrigin tile_origin(const WlTerrainLevels& tl, int e, int level) {
    const int row = min(max(level, 0), tl.rows - 1), col = min(max(tl.type[e], 0), tl.cols - 1);
    const float* o = tl.origins + 2 * (row * tl.cols + col);
    return TileOrigin{o[0], o[1]};
}
// the env's level as its lead lane sees it (a quad's other lanes take the lead's value: the lead is the one that writes level[])
template <int LANES>
WL_DEV int load_level(const WlTerrainLevels& tl, int e) {
    int lv = tl.level[e];
    if constexpr (LANES == 4) lv = __builtin_amdgcn_update_dpp(0, lv, 0, 0xF, 0xF, true);   // quad_perm [0, 0, 0, 0]
    return lv;
}
// the level an env moves to when its episode ends: up at the goal, down (not below 0) after a failure, unchanged after a time-out;
// past the top row: a uniform row
WL_DEV int next_level(const WlTerrainLevels& tl, int level, bool at_goal, bool failed, uint32_t gid, uint64_t step, uint64_t seed) {
    int lv = min(max(level, 0), tl.rows - 1);
    if (at_goal) lv += 1;
    else if (failed) lv = max(lv - 1, 0);
    if (lv >= tl.rows) lv = (int)__umulhi(philox_block(gid, step, ES_LEVEL, seed).x, (uint32_t)tl.rows);
    return lv;
}

// stands a drawn car at (x, y) on the terrain
WL_DEV void stand_elev_reset(const WlElevParams& p, const HeightFieldGround& g, ElevReset& r, float x, float y) {
    float zt;
    V3 n;
    g.sample(x, y, zt, n);
    r.pos = v3(x, y, fmaxf(p.reset_z, zt + p.spawn_clearance));
}
// isaaclab reset_root_state_uniform with the ranges of :409-419 + UniformPose2dCommand resample (:425-435).  STAND: the car is stood
// on the terrain where it is drawn; otherwise pos.x / pos.y (and tgt_x / tgt_y) stay OFFSETS from a tile's centre for place_elev_reset
// (`g` is read only when STAND: the origin-free wrapper passes nullptr)
template <bool STAND>
WL_DEV ElevReset draw_elev_reset_at(const WlElevParams& p, const HeightFieldGround* g, uint32_t gid, uint64_t step, uint64_t seed) {
    const F4 u = philox_uniform4(gid, step, ES_RESET, seed);
    const F4 c = philox_uniform4(gid, step, ES_CMD_RESET, seed);
    ElevReset r;
    const float x = sym(u.x, p.reset_xy), y = sym(u.y, p.reset_xy);
    if constexpr (STAND) stand_elev_reset(p, *g, r, x, y);
    else r.pos = v3(x, y, 0.f);
    float s, cc;
    sincos_fast(0.5f * sym(u.z, p.reset_yaw), s, cc);
    r.q = Quat{cc, 0.f, 0.f, s};
    r.vx = fmaf(u.w, p.reset_vel[1] - p.reset_vel[0], p.reset_vel[0]);
    r.vy = fmaf(c.w, p.reset_vel[1] - p.reset_vel[0], p.reset_vel[0]);
    r.tgt_x = sym(c.x, p.cmd_xy);
    r.tgt_y = sym(c.y, p.cmd_xy);
    r.tgt_h = sym(c.z, p.cmd_heading);
    return r;
}
// the part of a reset's draw that does not depend on where the env's tile is; place_elev_reset adds the centre and stands the car
WL_DEV ElevReset draw_elev_reset_local(const WlElevParams& p, uint32_t gid, uint64_t step, uint64_t seed) {
    return draw_elev_reset_at<false>(p, nullptr, gid, step, seed);
}
WL_DEV ElevReset draw_elev_reset(const WlElevParams& p, const HeightFieldGround& g, uint32_t gid, uint64_t step, uint64_t seed) {
    return draw_elev_reset_at<true>(p, &g, gid, step, seed);
}
WL_DEV void place_elev_reset(const WlElevParams& p, const HeightFieldGround& g, ElevReset& r, TileOrigin o) {
    stand_elev_reset(p, g, r, add_unfused(o.x, r.pos.x), add_unfused(o.y, r.pos.y));
    r.tgt_x = add_unfused(o.x, r.tgt_x);
    r.tgt_y = add_unfused(o.y, r.tgt_y);
}

// the bookkeeping rows of an env (episode length, goal command, episode sums) + the last action: with VehRows everything a
// persistent rollout carries in registers from step to step
struct ElevBook {
    int ep_len;
    float cb[2], epsum[WL_ER_NTERMS], tgt[4];   // tgt: target x, y, heading, resample timer
    float act[2];
};
template <int LANES>
WL_DEV void store_elev_state(const WlElevParams& p, const WlEnvBuffers& b, const Rows& S, int e, int wid, bool lead,
                             const VehRows<LANES>& r, const ElevBook& k) {
    store_veh_rows<LANES>(S, e, wid, lead, r, k.act[0], k.act[1], p.log_episode_sums != 0, k.epsum);
    if (lead) {
        S.st(WL_S_CMD_BX, e, k.cb[0]);
        S.st(WL_S_CMD_BY, e, k.cb[1]);
        S.st(WL_S_TGT_X, e, k.tgt[0]);
        S.st(WL_S_TGT_Y, e, k.tgt[1]);
        S.st(WL_S_TGT_H, e, k.tgt[2]);
        S.st(WL_S_CMD_TIMER, e, k.tgt[3]);
        b.episode_len[e] = k.ep_len;
    }
}
template <int LANES>
WL_DEV ElevBook load_elev_book(const WlElevParams& p, const WlEnvBuffers& b, const Rows& S, int e) {
    ElevBook k;
    k.ep_len = b.episode_len[e];
    k.cb[0] = S.ld(WL_S_CMD_BX, e);
    k.cb[1] = S.ld(WL_S_CMD_BY, e);
#pragma unroll
    for (int i = 0; i < WL_ER_NTERMS; ++i) k.epsum[i] = p.log_episode_sums ? S.ld(WL_S_EPSUM0 + i, e) : 0.f;
    k.tgt[0] = S.ld(WL_S_TGT_X, e);
    k.tgt[1] = S.ld(WL_S_TGT_Y, e);
    k.tgt[2] = S.ld(WL_S_TGT_H, e);
    k.tgt[3] = S.ld(WL_S_CMD_TIMER, e);
    k.act[0] = k.act[1] = 0.f;
    return k;
}

// one env.step() of env `e` (all LANES lanes of the env take part): the body of the step kernels below.
// PERSIST: the env's rows and bookkeeping live in `rows` / `*carry` across calls (persistent rollout): nothing is loaded
// from or stored to the state matrix here, both are updated in place.
// How the fused launch takes the step apart (round 6): `pose(pos, q)` is called with the env's pose as the step leaves it (AFTER a
// reset, if the env resets) as soon as that pose is known -- before the rewards are weighted, the outputs, the metrics and the state
// rows are written -- so that the launch can hand the height scan its lattice frames and let the other wavefronts start while this one
// finishes its bookkeeping.  `reset_src` supplies a resetting env's draw (wl_implicit_task.h): drawn here by default, by the fused
// launch's helper wavefront there.
static_assert(sizeof(WlElevParams) % alignof(VehDerived) == 0, "VehDerived follows WlElevParams in the argument block without a gap");
// What the step kernels take as their first argument: WlElevParams WITHOUT its trailing `levels` member, so that a launch without
// terrain levels has the argument block -- and, with LEVELS = false, the code -- it had before the member existed.  The member
// travels as the kernels' LAST argument and is read (scalar loads) only by the LEVELS = true instantiations, at resets.
constexpr int kElevHeadBytes = (int)offsetof(WlElevParams, log_episode_sums) + 4;
struct ElevHead {
    uint32_t w[kElevHeadBytes / 4];
};
static_assert(offsetof(WlElevParams, levels) >= (size_t)kElevHeadBytes && alignof(ElevHead) == 4, "levels is the trailing member");
inline ElevHead elev_head(const WlElevParams* p) {
    ElevHead h;
    __builtin_memcpy(&h, p, sizeof(h));
    return h;
}
// the argument read as the parameter struct: every field but `levels` is there
WL_DEV const WlElevParams& elev_args(const ElevHead& h) { return reinterpret_cast<const WlElevParams&>(h); }
// the vector copy of the head and of the derived block behind it (kernarg_vector_copy2), as a parameter struct in registers
WL_DEV void elev_kernarg_copy(WlElevParams& p, VehDerived& vd) {
    ElevHead h;
    kernarg_vector_copy2(0, h, vd);
    __builtin_memcpy(&p, &h, sizeof(h));
}
struct NoPose {
    WL_DEV void operator()(const V3&, const Quat&) const {}
};
template <int LANES, bool LEVELS, bool PERSIST = false, class RESET = InlineReset, class POSE = NoPose>
WL_DEV ScanPose elev_env_step(const WlElevParams& p, const VehDerived& vd, const WlEnvBuffers& b, const HeightFieldGround& ground,
                              const float2 action, VehRows<LANES>& rows, const WlStepOut& out, const uint64_t seed,
                              const uint64_t step, const Rows& S, const int e, const int wid, const bool lead, float* blk_metrics,
                              const WlTerrainLevels& tl /* the kernel's scalar argument: read at resets only, when LEVELS */,
                              ElevBook* carry = nullptr, float* prop2 = nullptr, const RESET& reset_src = RESET(), const POSE& pose = POSE()) {
    const WlVehicleParams& vp = p.vehicle;
    const uint32_t gid = (uint32_t)(b.env_offset + e);
    float2 a = action;
    const EnvConst ec = veh_env_const<LANES>(p.action, vp, vd, a, rows, wid);
    VehState s = veh_state<LANES>(vp, rows);
    // Bookkeeping rows (episode length, goal command, episode sums): the lane form fetches them after the physics loop --
    // it runs several wavefronts per SIMD and the registers are worth more than the latency; the quad form is one wavefront
    // per SIMD with registers to spare, so it requests them BEFORE the loop and finds them landed behind it.
    int ep_len_in = 0;
    float cb_in[2] = {0.f, 0.f}, epsum_in[WL_ER_NTERMS], tgt_in[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < WL_ER_NTERMS; ++i) epsum_in[i] = 0.f;
    auto fetch_bookkeeping = [&]() {
        if constexpr (PERSIST) {
            ep_len_in = carry->ep_len;
            cb_in[0] = carry->cb[0], cb_in[1] = carry->cb[1];
#pragma unroll
            for (int i = 0; i < WL_ER_NTERMS; ++i) epsum_in[i] = carry->epsum[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) tgt_in[i] = carry->tgt[i];
            return;
        }
        ep_len_in = b.episode_len[e];
        cb_in[0] = S.ld(WL_S_CMD_BX, e);
        cb_in[1] = S.ld(WL_S_CMD_BY, e);
        if (p.log_episode_sums) {
#pragma unroll
            for (int i = 0; i < WL_ER_NTERMS; ++i) epsum_in[i] = S.ld(WL_S_EPSUM0 + i, e);
        }
        tgt_in[0] = S.ld(WL_S_TGT_X, e);
        tgt_in[1] = S.ld(WL_S_TGT_Y, e);
        tgt_in[2] = S.ld(WL_S_TGT_H, e);
        tgt_in[3] = S.ld(WL_S_CMD_TIMER, e);
    };
    if constexpr (LANES == 4) {
        fetch_bookkeeping();
        WL_TL(1);
    }
    veh_integrate<LANES>(vp, vd, ec, s, ground, wid);
    if constexpr (LANES == 4) WL_TL(2);
    if constexpr (LANES != 4) {
        asm volatile("" ::: "memory");
        fetch_bookkeeping();
    }
    VehPost v = veh_post<LANES>(vp, s);
    int ep_len = ep_len_in + 1;
    const bool truncated = ep_len >= p.max_episode_length;
    // terminations / rewards use the command as the PREVIOUS step's command update left it (IsaacLab step order)
    float cbx = cb_in[0], cby = cb_in[1];
    const ElevTerms tm = elev_terms(p, v.pos, v.R.r2.z, v.vb, s.v, v.wheel_sum, cbx, cby, truncated);
    const bool terminated = !v.finite || tm.flag[0] || tm.flag[1] || tm.flag[2] || tm.flag[3];
    // the pose the step leaves behind first (a reset replaces it): whoever waits for it is served before the bookkeeping.  `pose` is
    // called exactly once on every path -- unconditionally, with nothing above it that returns -- because the fused launch's holds the
    // block's one s_barrier: keep it that way.
    const bool reset_now = terminated || truncated;
    ElevReset rd{};
    [[maybe_unused]] int level_now = 0;      // LEVELS and reset_now: the level the env leaves this step on
    if (reset_now) {
        if constexpr (LEVELS) {
            // the curriculum first (IsaacLab _reset_idx: curriculum terms before the reset events), then the spawn on the new tile.
            // The origin-free draw may come from the helper wavefront; the level needs this step's outcome, so it is decided here.
            level_now = next_level(tl, load_level<LANES>(tl, e), tm.flag[WL_ET_AT_GOAL], terminated, gid, step, seed);
            if (lead) tl.level[e] = level_now;
            rd = reset_src(e, [&] { return draw_elev_reset_local(p, gid, step, seed); });
            place_elev_reset(p, ground, rd, tile_origin(tl, e, level_now));
        } else {
            rd = reset_src(e, [&] { return draw_elev_reset(p, ground, gid, step, seed); });
        }
        v.pos = rd.pos;
    }
    pose(v.pos, reset_now ? rd.q : s.q);
    const float step_dt = p.sim_dt * (float)p.decimation;
    float epsum[WL_ER_NTERMS];
    const float reward = weigh_rewards(p.weight, tm.t, v.finite, step_dt, p.log_episode_sums != 0, epsum_in, epsum);
    if (lead) write_step_flags(out, e, reward, terminated, truncated);
    float a0 = a.x, a1 = a.y;
    float tgt_x = tgt_in[0], tgt_y = tgt_in[1], tgt_h = tgt_in[2], cmd_timer = tgt_in[3];
    if (reset_now) {
        if (lead) episode_end_metrics(blk_metrics, epsum, truncated, v.finite, tm.flag, ep_len);
        veh_reset(s, v, epsum, rd.pos, rd.q, v3(rd.vx, rd.vy, 0.f));
        tgt_x = rd.tgt_x;
        tgt_y = rd.tgt_y;
        tgt_h = rd.tgt_h;
        cmd_timer = p.cmd_resample_s;
        ep_len = 0;
        a0 = a1 = 0.f;
    }
    // command manager: count down, resample expired targets, re-express the target in the yaw-aligned base frame
    cmd_timer -= step_dt;
    if (cmd_timer <= 0.f) {
        const F4 u = philox_uniform4(gid, step, ES_CMD_RESAMPLE, seed);
        tgt_x = sym(u.x, p.cmd_xy);
        tgt_y = sym(u.y, p.cmd_xy);
        if constexpr (LEVELS) {      // the goal square sits on the env's tile
            const TileOrigin o = tile_origin(tl, e, reset_now ? level_now : load_level<LANES>(tl, e));
            tgt_x = add_unfused(o.x, tgt_x);
            tgt_y = add_unfused(o.y, tgt_y);
        }
        tgt_h = sym(u.z, p.cmd_heading);
        cmd_timer = p.cmd_resample_s;
    }
    {
        float c, sn;
        yaw_cs(s.q, c, sn);
        const float dx = tgt_x - v.pos.x, dy = tgt_y - v.pos.y;
        cbx = fmaf(c, dx, sn * dy);
        cby = fmaf(-sn, dx, c * dy);
    }
    {   // the env's new rows: kept (persistent rollout) or written back
        veh_rows_from(rows, s, v);
        ElevBook k;
        k.ep_len = ep_len;
        k.cb[0] = cbx, k.cb[1] = cby;
#pragma unroll
        for (int i = 0; i < WL_ER_NTERMS; ++i) k.epsum[i] = epsum[i];
        k.tgt[0] = tgt_x, k.tgt[1] = tgt_y, k.tgt[2] = tgt_h, k.tgt[3] = cmd_timer;
        k.act[0] = a0, k.act[1] = a1;
        if constexpr (PERSIST) *carry = k;
        else store_elev_state<LANES>(p, b, S, e, wid, lead, rows, k);
    }
    // proprioceptive part of the observation, from the post-reset state (all lanes of a quad take part)
    const Mat3 R2 = mat_from_quat(s.q);
    write_elev_prop<LANES>(p, out.obs + (int64_t)e * WL_ELEV_OBS_DIM, v.pos, s.q, mul_t(R2, s.v), mul_t(R2, v.ww), cbx, cby, a0, a1,
                           wid, lead, prop2);
    float yc, ys;
    yaw_cs(s.q, yc, ys);
    return ScanPose{v.pos.x, v.pos.y, v.pos.z, yc, ys};
}

}  // namespace

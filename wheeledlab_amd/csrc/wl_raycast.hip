// wl_raycast.hip -- the ray caster (include/wheeledlab_amd_raycaster.h) for gfx950: any table of rays from every env's sensor against
// the terrain solid.  The walk and the pyramid are the depth camera's (wl_depth_dev.h::cast_ray: the bound pyramid, then the exact
// bilinear-patch intersection; with a unit direction the ray parameter at the hit is the Euclidean range), the bilinear sampler the
// contact samplers', included unchanged; this file maps table entries to lanes and stores what they report.  A lidar is a table of
// this entry: zero starts, no scale, distances only (sensors.LidarScanner).
//
// General form.  Block = ONE wavefront = 64 consecutive rays of one env (a lidar fan is channel-major: neighbouring lanes are
// neighbouring azimuths of one channel, whose ground tracks cross neighbouring cells -- the lanes walk together and share cache
// lines).  Single-wavefront blocks for the depth kernel's reason (wl_depth.hip): walk lengths vary a lot from wave to wave, and the
// dispatcher refills a single-wave block's slot the moment it is done.  env x wave is flattened into blockIdx.x (n > 65 535 envs).
// The pose is read and the sensor frame built once per wave (wave-uniform); each lane loads its start and direction, walks its ray and
// stores its distance and / or hit point non-temporally (consecutive lanes, consecutive floats of dist[e]), so that the scan does not
// push the pyramid and the heights out of L2 (the depth kernel's measured rule).
//
// Column form (p.vertical).  Lane = ray, same flattening, no pyramid access, no barriers, no LDS: the lane's world (x, y) from the
// yaw rotation of its start, one 8-byte pair-table gather (hf_corners), the bilinear blend.  Block = 64 as well: a wave is ~300
// instructions (31 VGPRs, no scratch; most of them the wave-uniform frame and the stores) around ONE gather, so nothing but the
// number of waves in flight hides that gather's latency, and single-wave blocks are what the dispatcher packs most freely; the frame
// is per env, and with one wave per block it is computed once per block.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_raycaster.h"
#include "wl_kernel_common.h"
#include "wl_raycast_dev.h"

namespace {

struct RayCastOut {
    const float* scale;   // [n_rays] or nullptr
    float* dist;          // [n_envs][n_rays] or nullptr
    float* hits;          // [n_envs][n_rays][3] or nullptr
};

WL_DEV SensorFrame wave_frame(const WlRayCastParams& p, const WlEnvBuffers& b, int e) {
    const Rows S = make_rows(b.state, b.stride);
    const Quat q{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    const Mat3 mount = mat_from_quat(Quat{p.offset_quat[0], p.offset_quat[1], p.offset_quat[2], p.offset_quat[3]});
    return raycast_frame(p, mount, ld3(S, WL_S_PX, e), q);
}

WL_DEV void store_ray(const WlRayCastParams& p, const RayCastOut& o, int e, int k, const RayCastHit& r) {
    const int64_t at = (int64_t)e * p.n_rays + k;
    if (o.dist) __builtin_nontemporal_store(o.scale ? r.t * o.scale[k] : r.t, o.dist + at);
    if (o.hits) {
        __builtin_nontemporal_store(r.hit.x, o.hits + 3 * at);
        __builtin_nontemporal_store(r.hit.y, o.hits + 3 * at + 1);
        __builtin_nontemporal_store(r.hit.z, o.hits + 3 * at + 2);
    }
}

__global__ void __launch_bounds__(64) raycast_walk_kernel(const WlRayCastParams p, const WlEnvBuffers b, const DepthGrid g, const Pyramid py,
                                                          const float* __restrict__ buf, const unsigned buf_bytes,
                                                          const float* __restrict__ starts, const float* __restrict__ dirs,
                                                          const RayCastOut out, const int waves) {
    const int e = blockIdx.x / waves, w = blockIdx.x - e * waves;
    const SensorFrame s = wave_frame(p, b, e);
    const int k = w * 64 + (int)threadIdx.x;
    if (k >= p.n_rays) return;
    // no start table (wave-uniform): every ray leaves the sensor origin, and the lane loads its direction alone
    const V3 st = starts ? v3(starts[3 * k], starts[3 * k + 1], starts[3 * k + 2]) : v3(0.f, 0.f, 0.f);
    const V3 d = v3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
    const FieldMem mem{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(buf), 0, (int)buf_bytes, 0x00020000)};
    store_ray(p, out, e, k, raycast_walk(g, py, pyramid_head(g, py, mem), mem, s, st, d, p.max_distance));
}

__global__ void __launch_bounds__(64) raycast_column_kernel(const WlRayCastParams p, const WlEnvBuffers b, const HeightFieldGround gr,
                                                            const float* __restrict__ starts, const RayCastOut out, const int waves) {
    const int e = blockIdx.x / waves, w = blockIdx.x - e * waves;
    const SensorFrame s = wave_frame(p, b, e);
    const int k = w * 64 + (int)threadIdx.x;
    if (k >= p.n_rays) return;
    store_ray(p, out, e, k, raycast_column(gr, s, v3(starts[3 * k], starts[3 * k + 1], starts[3 * k + 2]), p.max_distance));
}

inline bool aligned4(const void* q) { return ((uintptr_t)q & 3u) == 0; }

}  // namespace

extern "C" {

int wl_raycast_version(void) { return WL_RAYCASTER_VERSION; }

int wl_raycast_scan(const WlRayCastParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid, const float* ray_starts,
                    const float* ray_dirs, const float* ray_scale, float* dist_out, float* hits_out, void* stream) {
    if (!p || !b || !b->state || !pyramid || (!dist_out && !hits_out) || b->n_envs < 0) return WL_EINVAL;
    if (p->n_rays < 1 || p->n_rays > WL_RAYCAST_MAX_RAYS || !(p->max_distance > 0.f && p->max_distance < INFINITY)) return WL_EINVAL;
    if (p->alignment < WL_RAYCAST_ALIGN_BASE || p->alignment > WL_RAYCAST_ALIGN_WORLD || (p->vertical != 0 && p->vertical != 1)) return WL_EINVAL;
    float qn = 0.f;
    for (int i = 0; i < 4; ++i) qn += p->offset_quat[i] * p->offset_quat[i];
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(p->offset_pos[i])) return WL_EINVAL;
    if (!(qn > 0.f && qn < INFINITY)) return WL_EINVAL;
    if ((ray_dirs == nullptr) != (p->vertical == 1)) return WL_EINVAL;      // directions: NULL if and only if the column form
    if (!ray_starts && p->vertical) return WL_EINVAL;                       // starts: NULL (all zero) in the general form only
    if (p->vertical && (p->alignment == WL_RAYCAST_ALIGN_BASE || p->offset_quat[1] != 0.f || p->offset_quat[2] != 0.f)) return WL_EINVAL;
    int rc = heightfield_args_ok(hf, HF_PYRAMID);
    if (rc != WL_OK) return rc;
    if (p->vertical && (rc = heightfield_args_ok(hf, HF_PAIRS)) != WL_OK) return rc;
    if (b->stride < b->n_envs || b->stride > 0x7fffffffLL / (4 * WL_S_COUNT)) return WL_EINVAL;   // Rows: one 32-bit buffer resource
    const int waves = (p->n_rays + 63) / 64;
    if ((int64_t)b->n_envs * waves > 0x7fffffffLL) return WL_EINVAL;
    if (!aligned4(b->state) || !aligned4(pyramid) || !aligned4(ray_starts) || !aligned4(ray_dirs) || !aligned4(ray_scale) ||
        !aligned4(dist_out) || !aligned4(hits_out))
        return WL_EALIGN;
    if (b->n_envs == 0) return WL_OK;
    WlRayCastParams q = *p;
    const float inv = 1.f / sqrtf(qn);
    for (int i = 0; i < 4; ++i) q.offset_quat[i] *= inv;
    const RayCastOut out{ray_scale, dist_out, hits_out};
    const unsigned grid = (unsigned)((int64_t)b->n_envs * waves);
    clear_error();
    if (q.vertical) {
        raycast_column_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(q, *b, make_ground(hf), ray_starts, out, waves);
    } else {
        const Pyramid py = make_pyramid(hf->nx, hf->ny);
        const unsigned bytes = (unsigned)(pyramid_total_floats(hf->nx, hf->ny) * 4);
        raycast_walk_kernel<<<grid, 64, 0, (hipStream_t)stream>>>(q, *b, make_depth_grid(hf), py, pyramid, bytes, ray_starts, ray_dirs, out,
                                                                  waves);
    }
    return launch_status();
}

}  // extern "C"

// wl_lidar.hip -- lidar range scans against the terrain (include/wheeledlab_amd_lidar.h) for gfx950.
//
// Each beam is one ray of the depth camera's walk (wl_depth_dev.h::cast_ray: the bound pyramid, then the exact bilinear-patch
// intersection) with a unit direction, so its parameter at the hit is the Euclidean range.  The walk, the pyramid and the terrain
// solid are the camera's, unchanged; this file only maps beams to lanes.
//
// Mapping: block = ONE wavefront = 64 consecutive beams of one env (channel-major: neighbouring lanes are neighbouring azimuths of
// one channel, whose ground tracks cross neighbouring cells -- the lanes walk together and share cache lines).  Single-wavefront
// blocks for the depth kernel's reason (wl_depth.hip): walk lengths vary a lot from wave to wave, and the dispatcher refills a
// slot the moment its wave is done.  env x wave is flattened into blockIdx.x (n > 65 535 envs).  The pose is read and the sensor
// frame built once per wave (wave-uniform values); each lane rotates its beam, walks it, and stores its range (consecutive lanes,
// consecutive floats of ranges[e]).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_lidar.h"
#include "wl_kernel_common.h"
#include "wl_lidar_dev.h"

namespace {

__global__ void __launch_bounds__(64) lidar_scan_kernel(const WlLidarParams p, const WlEnvBuffers b, const DepthGrid g, const Pyramid py,
                                                        const float* __restrict__ buf, const unsigned buf_bytes,
                                                        const float* __restrict__ dirs, float* __restrict__ ranges, const int waves) {
    const int e = blockIdx.x / waves, w = blockIdx.x - e * waves;
    const Rows S = make_rows(b.state, b.stride);
    const Quat q{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    const Mat3 mount = mat_from_quat(Quat{p.offset_quat[0], p.offset_quat[1], p.offset_quat[2], p.offset_quat[3]});
    const LidarPose s = lidar_pose(p, mount, ld3(S, WL_S_PX, e), q);
    const int k = w * 64 + (int)threadIdx.x;
    if (k >= p.n_beams) return;
    const V3 d = v3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
    const FieldMem mem{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(buf), 0, (int)buf_bytes, 0x00020000)};
    const float r = lidar_beam(g, py, pyramid_head(g, py, mem), mem, s, d, p.max_range);
    // non-temporal: the scan must not push the pyramid and the heights out of L2 (the depth kernel's measured rule)
    __builtin_nontemporal_store(r, ranges + (int64_t)e * p.n_beams + k);
}

inline bool aligned4(const void* q) { return ((uintptr_t)q & 3u) == 0; }

}  // namespace

extern "C" {

int wl_lidar_version(void) { return WL_LIDAR_VERSION; }

int wl_lidar_scan(const WlLidarParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid, const float* beam_dirs,
                  float* ranges_out, void* stream) {
    if (!p || !b || !b->state || !pyramid || !beam_dirs || !ranges_out || b->n_envs < 0) return WL_EINVAL;
    if (p->n_beams < 1 || p->n_beams > WL_LIDAR_MAX_BEAMS || !(p->max_range > 0.f && p->max_range < INFINITY)) return WL_EINVAL;
    float qn = 0.f;
    for (int i = 0; i < 4; ++i) qn += p->offset_quat[i] * p->offset_quat[i];
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(p->offset_pos[i])) return WL_EINVAL;
    if (!(qn > 0.f && qn < INFINITY)) return WL_EINVAL;
    const int rc = heightfield_args_ok(hf, HF_PYRAMID);
    if (rc != WL_OK) return rc;
    if (b->stride < b->n_envs || b->stride > 0x7fffffffLL / (4 * WL_S_COUNT)) return WL_EINVAL;   // Rows: one 32-bit buffer resource
    const int waves = (p->n_beams + 63) / 64;
    if ((int64_t)b->n_envs * waves > 0x7fffffffLL) return WL_EINVAL;
    if (!aligned4(b->state) || !aligned4(pyramid) || !aligned4(beam_dirs) || !aligned4(ranges_out)) return WL_EALIGN;
    if (b->n_envs == 0) return WL_OK;
    WlLidarParams q = *p;
    const float inv = 1.f / sqrtf(qn);
    for (int i = 0; i < 4; ++i) q.offset_quat[i] *= inv;
    q.yaw_only = p->yaw_only != 0;
    const Pyramid py = make_pyramid(hf->nx, hf->ny);
    const unsigned bytes = (unsigned)(pyramid_total_floats(hf->nx, hf->ny) * 4);
    clear_error();
    lidar_scan_kernel<<<(unsigned)((int64_t)b->n_envs * waves), 64, 0, (hipStream_t)stream>>>(q, *b, make_depth_grid(hf), py, pyramid, bytes,
                                                                                              beam_dirs, ranges_out, waves);
    return launch_status();
}

}  // extern "C"

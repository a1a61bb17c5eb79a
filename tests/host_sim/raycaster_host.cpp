// TEST INFRASTRUCTURE ONLY: the ray caster's device functions (wheeledlab_amd/csrc/wl_raycast_dev.h: sensor frame, world ray + walk,
// column sample; fp32) compiled for the host through the stand-in hip_runtime.h and driven over arrays, so that
// tests/test_raycaster_cpu.py can hold them against oracle/depth.c and a float64 bilinear without a GPU.
// Built by the test into a scratch directory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>
using std::max;
using std::min;

#include "wl_raycast_dev.h"
#include "pyramid_host.h"

extern "C" {
// pos [n][3], quat [n][4] of the roots; starts, dirs [n_rays][3] (starts NULL: all zero; dirs unused with p->vertical); scale [n_rays] or NULL;
// dist [n][n_rays], hits [n][n_rays][3].  The mount quaternion is normalised and the results are stored as wl_raycast_scan does.
int hs_raycast(const WlRayCastParams* p, const WlHeightField* hf, int n, const float* pos, const float* quat, const float* starts,
               const float* dirs, const float* scale, float* dist, float* hits) {
    WlRayCastParams q = *p;
    float qn = 0.f;
    for (int i = 0; i < 4; ++i) qn += q.offset_quat[i] * q.offset_quat[i];
    const float inv = 1.f / std::sqrt(qn);
    for (int i = 0; i < 4; ++i) q.offset_quat[i] *= inv;
    const Pyramid py = make_pyramid(hf->nx, hf->ny);
    const std::vector<float> buf = host_pyramid(hf);
    const DepthGrid g = make_depth_grid(hf);
    const FieldMem mem{buf.data()};
    const PyrHead hd = pyramid_head(g, py, mem);
    const HeightFieldGround gr = make_ground(hf);
    const Mat3 mount = mat_from_quat(Quat{q.offset_quat[0], q.offset_quat[1], q.offset_quat[2], q.offset_quat[3]});
    for (int e = 0; e < n; ++e) {
        const Quat r{quat[4 * e], quat[4 * e + 1], quat[4 * e + 2], quat[4 * e + 3]};
        const SensorFrame s = raycast_frame(q, mount, v3(pos[3 * e], pos[3 * e + 1], pos[3 * e + 2]), r);
        for (int k = 0; k < q.n_rays; ++k) {
            const V3 st = starts ? v3(starts[3 * k], starts[3 * k + 1], starts[3 * k + 2]) : v3(0.f, 0.f, 0.f);
            const RayCastHit h = q.vertical ? raycast_column(gr, s, st, q.max_distance)
                                            : raycast_walk(g, py, hd, mem, s, st, v3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]), q.max_distance);
            const size_t at = (size_t)e * q.n_rays + k;
            dist[at] = scale ? h.t * scale[k] : h.t;
            hits[3 * at] = h.hit.x, hits[3 * at + 1] = h.hit.y, hits[3 * at + 2] = h.hit.z;
        }
    }
    return 0;
}
}

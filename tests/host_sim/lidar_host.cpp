// TEST INFRASTRUCTURE ONLY: the lidar's device functions (wheeledlab_amd/csrc/wl_lidar_dev.h: sensor pose + per-beam walk, fp32)
// compiled for the host through the stand-in hip_runtime.h and driven over arrays, so that tests/test_lidar_cpu.py can hold them
// against oracle/depth.c without a GPU.  The walk's step hook counts the pyramid cells each beam visits (DESIGN.md's walk lengths).
// Built by the test into a scratch directory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>
using std::max;
using std::min;

static int g_steps = 0;
#define WL_DEPTH_STEP_HOOK(L) (++g_steps)

#include "wl_lidar_dev.h"
#include "pyramid_host.h"

extern "C" {
// pos [n][3], quat [n][4] of the roots; dirs [n_beams][3]; ranges [n][n_beams]; steps (optional) [n][n_beams]: walk steps per beam.
// The mount quaternion is normalised as wl_lidar_scan does.
int hs_lidar(const WlLidarParams* p, const WlHeightField* hf, int n, const float* pos, const float* quat, const float* dirs, float* ranges,
             int* steps) {
    WlLidarParams q = *p;
    float qn = 0.f;
    for (int i = 0; i < 4; ++i) qn += q.offset_quat[i] * q.offset_quat[i];
    const float inv = 1.f / std::sqrt(qn);
    for (int i = 0; i < 4; ++i) q.offset_quat[i] *= inv;
    const Pyramid py = make_pyramid(hf->nx, hf->ny);
    const std::vector<float> buf = host_pyramid(hf);
    const DepthGrid g = make_depth_grid(hf);
    const FieldMem mem{buf.data()};
    const PyrHead hd = pyramid_head(g, py, mem);
    const Mat3 mount = mat_from_quat(Quat{q.offset_quat[0], q.offset_quat[1], q.offset_quat[2], q.offset_quat[3]});
    for (int e = 0; e < n; ++e) {
        const Quat r{quat[4 * e], quat[4 * e + 1], quat[4 * e + 2], quat[4 * e + 3]};
        const LidarPose s = lidar_pose(q, mount, v3(pos[3 * e], pos[3 * e + 1], pos[3 * e + 2]), r);
        for (int k = 0; k < q.n_beams; ++k) {
            g_steps = 0;
            ranges[(size_t)e * q.n_beams + k] = lidar_beam(g, py, hd, mem, s, v3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]), q.max_range);
            if (steps) steps[(size_t)e * q.n_beams + k] = g_steps;
        }
    }
    return 0;
}
}

// TEST INFRASTRUCTURE ONLY: the approximate math of wheeledlab_amd/csrc/wl_math.h that the drift step's tail uses, compiled for the
// host (through the stand-in hip_runtime.h next to this file) and driven over arrays, so that tests/test_drift_tail_reference_cpu.py
// can measure it against float64.  Built by the test into a scratch directory.
#include <hip/hip_runtime.h>

#include "wl_math.h"

extern "C" {
void hs_atan2_fast(int n, const float* y, const float* x, float* out) {
    for (int i = 0; i < n; ++i) out[i] = atan2_fast(y[i], x[i]);
}
void hs_euler_xyz(int n, const float* q /* [n][4] */, float* out /* [n][3] */) {
    for (int i = 0; i < n; ++i) {
        const V3 e = euler_xyz_from_quat(Quat{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]});
        out[3 * i] = e.x, out[3 * i + 1] = e.y, out[3 * i + 2] = e.z;
    }
}
}

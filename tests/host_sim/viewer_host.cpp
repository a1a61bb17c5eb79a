// TEST INFRASTRUCTURE ONLY: the viewer camera's per-ray device functions (wheeledlab_amd/csrc/wl_viewer_dev.h) compiled for the host
// through the stand-in hip_runtime.h, so that tests/test_viewer_host_cpu.py can hold their fp32 arithmetic against the float64
// restatement (tests/viewer_reference.py) without a GPU.  hs_viewer_render is a brute-force serial frame: no binning and no cull, every
// car against every pixel (the binning is the GPU tests' business); the hs_viewer_* probes expose single functions.  Built by the test
// into a scratch directory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>
using std::max;
using std::min;

#include "wl_viewer_dev.h"
#include "pyramid_host.h"

static V3 ld3v(const float* a) { return v3(a[0], a[1], a[2]); }

extern "C" {
// the frame of n cars (pos [n][3], quat [n][4] w, x, y, z): rgb uint8 [H][W][3], depth float [H][W], id int32 [H][W].  hf: the
// heightfield ground (its pyramid is built here) or NULL for the plane; map: the traversability map or NULL for the checker.
int hs_viewer_render(const WlViewerParams* p, const WlHeightField* hf, const WlTravMap* map, int n, const float* pos, const float* quat,
                     uint8_t* rgb, float* depth, int32_t* id) {
    const V3 o = ld3v(p->cam_pos);
    const Mat3 Rc = mat_from_quat(Quat{p->cam_quat[0], p->cam_quat[1], p->cam_quat[2], p->cam_quat[3]});
    const ViewerGeom geom = viewer_geom(*p);
    const V3 sun = viewer_sun(*p);
    std::vector<ViewerCar> cars((size_t)n);
    for (int e = 0; e < n; ++e) {
        ViewerCar& c = cars[(size_t)e];
        c.px = pos[3 * e], c.py = pos[3 * e + 1], c.pz = pos[3 * e + 2], c.id = e;
        c.R = mat_from_quat(Quat{quat[4 * e], quat[4 * e + 1], quat[4 * e + 2], quat[4 * e + 3]});
        c.tx = c.ty = c.pad = 0;
    }
    std::vector<float> buf;
    DepthGrid g{};
    Pyramid py{};
    if (hf) buf = host_pyramid(hf), g = make_depth_grid(hf), py = make_pyramid(hf->nx, hf->ny);
    const FieldMem mem{buf.data()};
    const PyrHead hd = hf ? pyramid_head(g, py, mem) : PyrHead{};
    const WlTravMap m = map ? *map : WlTravMap{};
    for (int row = 0; row < p->height; ++row)
        for (int col = 0; col < p->width; ++col) {
            const V3 d = mul(Rc, viewer_ray_body(*p, row, col));
            const float a = dot(d, d);
            ViewerPix px = hf ? viewer_ground_field(*p, m, map != nullptr, g, py, hd, mem, o, d) : viewer_ground_plane(*p, m, map != nullptr, o, d);
            for (int e = 0; e < n; ++e) viewer_car(*p, geom, cars[(size_t)e], o, d, a, px);
            const size_t pix = (size_t)row * p->width + col;
            viewer_shade(*p, sun, px, rgb + 3 * pix);
            depth[pix] = px.t;
            id[pix] = px.id;
        }
    return 0;
}

// probes: one function over n inputs each
void hs_viewer_sphere_t(int n, const float* o, const float* d, const float* c, const float* r, float* t) {
    for (int k = 0; k < n; ++k) {
        const V3 dk = ld3v(d + 3 * k);
        t[k] = viewer_sphere_t(ld3v(o + 3 * k), dk, dot(dk, dk), ld3v(c + 3 * k), r[k]);
    }
}
void hs_viewer_box_t(int n, const float* o, const float* d, const float* c, const float* h, float* t, int* axis) {
    for (int k = 0; k < n; ++k) t[k] = viewer_box_t(ld3v(o + 3 * k), ld3v(d + 3 * k), ld3v(c + 3 * k), ld3v(h + 3 * k), axis[k]);
}
void hs_viewer_wins(int n, const float* t, const int* id, const float* best_t, const int* best_id, int* out) {
    for (int k = 0; k < n; ++k) {
        ViewerPix px{};
        px.t = best_t[k], px.id = best_id[k];
        out[k] = viewer_wins(t[k], id[k], px) ? 1 : 0;
    }
}
void hs_viewer_traversable(const WlTravMap* m, int n, const float* x, const float* y, int* out) {
    for (int k = 0; k < n; ++k) out[k] = viewer_traversable(*m, x[k], y[k]) ? 1 : 0;
}
// the checker's albedo (no map) at (x, y): 0 the light tone, 1 the dark one
void hs_viewer_checker(const WlViewerParams* p, int n, const float* x, const float* y, int* out) {
    const WlTravMap m{};
    for (int k = 0; k < n; ++k) out[k] = viewer_ground_albedo(*p, m, false, x[k], y[k]).x == kViewerChecker[0][0] ? 0 : 1;
}
void hs_viewer_q8(int n, const float* c, uint8_t* out) {
    for (int k = 0; k < n; ++k) out[k] = viewer_q8(c[k]);
}
}

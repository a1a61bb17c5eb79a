// wl_viewer_dev.h -- the viewer camera's per-ray device functions (see wl_viewer.hip): camera ray, ground (plane or the depth
// walk over the bound pyramid), car hits (chassis box + four wheel spheres), the tie rule and the shading.  A header of its own so
// that tests/host_sim can compile it for the host and hold it against the numpy restatement (tests/viewer_reference.py).
#pragma once
#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_viewer.h"
#include "wl_math.h"
#include "wl_depth_dev.h"       // the heightfield walk (ray_begin / ray_step / ray_result over the bound pyramid)

namespace {

// designed colours (linear 0 .. 1; the frame is their 8-bit quantisation after shading)
constexpr float kViewerSky[3] = {0.62f, 0.76f, 0.92f};
constexpr float kViewerChecker[2][3] = {{0.56f, 0.56f, 0.52f}, {0.40f, 0.41f, 0.38f}};
constexpr float kViewerTrav[2][3] = {{0.16f, 0.16f, 0.17f}, {0.86f, 0.86f, 0.84f}};   // [not traversable, traversable]
constexpr float kViewerWheel[3] = {0.10f, 0.10f, 0.11f};
constexpr float kViewerHighlight[3] = {1.00f, 0.84f, 0.10f};
constexpr int kViewerPalette = 8;
constexpr float kViewerPaletteRgb[kViewerPalette][3] = {
    {0.85f, 0.20f, 0.18f}, {0.18f, 0.45f, 0.85f}, {0.20f, 0.70f, 0.30f}, {0.80f, 0.45f, 0.10f},
    {0.60f, 0.25f, 0.75f}, {0.10f, 0.70f, 0.70f}, {0.85f, 0.35f, 0.60f}, {0.55f, 0.55f, 0.20f}};
constexpr float kViewerNear = 1e-3f;      // a car whose bounding sphere reaches closer than this to the image plane covers every tile

// ids of the `id` output
constexpr int kViewerGround = -1, kViewerSkyId = -2;

// pixel (row, col)'s ray in the camera body frame: the depth camera's model (wl_depth_dev.h::depth_pixel_ray_body)
WL_DEV V3 viewer_ray_body(const WlViewerParams& p, int row, int col) {
    return v3(1.f, -(((float)col + 0.5f - p.cx) / p.fx), -(((float)row + 0.5f - p.cy) / p.fy));
}

// the car geometry every lane needs, in the root frame
struct ViewerGeom {
    V3 box_c, box_h;
    V3 wheel[4];
    float wheel_r, bound_r;     // wheel radius; radius of the sphere about the root origin that holds box and wheels
};
WL_DEV ViewerGeom viewer_geom(const WlViewerParams& p) {
    ViewerGeom g;
    g.box_c = v3(p.box_center[0], p.box_center[1], p.box_center[2]);
    g.box_h = v3(p.box_half[0], p.box_half[1], p.box_half[2]);
    // wheel order: front left, front right, rear left, rear right
    g.wheel[0] = v3(p.half_wheelbase_f, p.half_track, p.wheel_z);
    g.wheel[1] = v3(p.half_wheelbase_f, -p.half_track, p.wheel_z);
    g.wheel[2] = v3(-p.half_wheelbase_r, p.half_track, p.wheel_z);
    g.wheel[3] = v3(-p.half_wheelbase_r, -p.half_track, p.wheel_z);
    g.wheel_r = p.wheel_radius;
    float r = std::sqrt(dot(g.box_c, g.box_c)) + std::sqrt(dot(g.box_h, g.box_h));
    for (int w = 0; w < 4; ++w) r = fmaxf(r, std::sqrt(dot(g.wheel[w], g.wheel[w])) + g.wheel_r);
    g.bound_r = r * 1.001f + 1e-4f;     // a hair over: the cull and the early out must never drop a hit
    return g;
}

// one visible car as the shade pass reads it (64 bytes: four 16-byte LDS reads, every lane the same address)
struct alignas(16) ViewerCar {
    float px, py, pz;
    int id;           // env index in the batch
    Mat3 R;           // body -> world
    int tx, ty;       // the tiles it may cover: columns tx & 0xffff .. tx >> 16, rows ty & 0xffff .. ty >> 16
    int pad;
};
static_assert(sizeof(ViewerCar) == 64, "a car record is four 16-byte slots");

// the running answer of one pixel
struct ViewerPix {
    float t;          // distance along the optical axis (far_clip: nothing)
    int id;           // env index, kViewerGround or kViewerSkyId
    V3 n;             // unit world normal at the hit
    V3 albedo;
};

// the tie rule: nearer wins; at equal distance a car beats the ground and the lower env id beats a higher one
WL_DEV bool viewer_wins(float t, int id, const ViewerPix& px) { return t < px.t || (t == px.t && (px.id < 0 || id < px.id)); }

// the discriminant b^2 - a (|oc|^2 - r^2) of a ray against a sphere, as a r^2 - |d x oc|^2: the textbook form cancels catastrophically
// in fp32 for a small sphere far away (a wheel 50 m off: two terms of ~6e6 for a difference of ~1e-3; measured 1.5 cm depth errors)
WL_DEV float viewer_sphere_disc(V3 d, V3 oc, float a, float r) {
    const V3 x = cross(d, oc);
    return fmaf(a * r, r, -dot(x, x));
}

// the smaller root of |o + t d - c|^2 = r^2 that lies ahead of an origin OUTSIDE the sphere; < 0: none (origin inside, behind,
// missed).  Stable form: t = cc / (sqrt(disc) - b), no cancellation for far, grazing rays.
WL_DEV float viewer_sphere_t(V3 o, V3 d, float a, V3 c, float r) {
    const V3 oc = o - c;
    const float b = dot(d, oc), cc = fmaf(-r, r, dot(oc, oc));
    const float disc = viewer_sphere_disc(d, oc, a, r);
    if (!(disc >= 0.f) || !(cc > 0.f) || !(b < 0.f)) return -1.f;
    return cc / (std::sqrt(disc) - b);
}

// entry parameter of the ray into the axis-aligned box centred at c with half extents h (origin outside); axis of the face entered
WL_DEV float viewer_box_t(V3 o, V3 d, V3 c, V3 h, int& axis) {
    const float ox = o.x - c.x, oy = o.y - c.y, oz = o.z - c.z;
    // a zero direction component: the positive huge reciprocal puts that slab at -huge .. +huge when the origin is inside it and
    // entirely behind or ahead when outside (as the depth walk treats a zero ground-track component)
    const float ix = d.x != 0.f ? 1.f / d.x : 1e30f, iy = d.y != 0.f ? 1.f / d.y : 1e30f, iz = d.z != 0.f ? 1.f / d.z : 1e30f;
    const float ax = (-h.x - ox) * ix, bx = (h.x - ox) * ix, ay = (-h.y - oy) * iy, by = (h.y - oy) * iy;
    const float az = (-h.z - oz) * iz, bz = (h.z - oz) * iz;
    const float nx = fminf(ax, bx), ny = fminf(ay, by), nz = fminf(az, bz);
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    float tn = nx;
    axis = 0;
    if (ny > tn) tn = ny, axis = 1;
    if (nz > tn) tn = nz, axis = 2;
    return (tn > 0.f && tn <= tf) ? tn : -1.f;
}

// one car against the pixel's running answer (world ray o + t d, a = |d|^2)
WL_DEV void viewer_car(const WlViewerParams& p, const ViewerGeom& g, const ViewerCar& car, V3 o, V3 d, float a, ViewerPix& px) {
    const V3 pos = v3(car.px, car.py, car.pz);
    // early out on the bounding sphere: missed, behind, or entered only beyond the current answer
    {
        const V3 oc = o - pos;
        const float b = dot(d, oc), cc = fmaf(-g.bound_r, g.bound_r, dot(oc, oc));
        const float disc = viewer_sphere_disc(d, oc, a, g.bound_r);
        if (!(disc >= 0.f)) return;
        const float sq = std::sqrt(disc);
        if (sq - b <= 0.f) return;                        // the far root is behind the camera
        if (cc > 0.f && cc / (sq - b) > px.t) return;      // origin outside: the near root is already beyond the answer
    }
    const V3 ol = mul_t(car.R, o - pos), dl = mul_t(car.R, d);
    int axis;
    float t = viewer_box_t(ol, dl, g.box_c, g.box_h, axis);
    int part = t > 0.f ? 4 : -1;      // 4: the box, 0 .. 3: a wheel
    V3 wc = g.wheel[0];               // centre of the wheel hit (kept in registers: no dynamic index into g.wheel)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float tw = viewer_sphere_t(ol, dl, a, g.wheel[w], g.wheel_r);
        if (tw > 0.f && (part < 0 || tw < t)) t = tw, part = w, wc = g.wheel[w];
    }
    if (part < 0 || !(t < p.far_clip) || !viewer_wins(t, car.id, px)) return;
    px.t = t;
    px.id = car.id;
    V3 nl;
    if (part == 4) {
        const float s = (axis == 0 ? dl.x : axis == 1 ? dl.y : dl.z) > 0.f ? -1.f : 1.f;
        nl = v3(axis == 0 ? s : 0.f, axis == 1 ? s : 0.f, axis == 2 ? s : 0.f);
        const int gid = car.id + p.id_offset;
        const float* c = gid == p.env_index ? kViewerHighlight : kViewerPaletteRgb[((gid % kViewerPalette) + kViewerPalette) % kViewerPalette];
        px.albedo = v3(c[0], c[1], c[2]);
    } else {
        const float ir = 1.f / g.wheel_r;
        nl = ir * (fma3(t, dl, ol) - wc);
        px.albedo = v3(kViewerWheel[0], kViewerWheel[1], kViewerWheel[2]);
    }
    px.n = mul(car.R, nl);
}

// TraversabilityHashmapUtil.get_map_id (visual/utils/traversability_utils.py:83-88), restated from wl_visual_env.h::map_id (not
// shared: moving it would change the visual task's sources): float32 arithmetic, truncation toward zero, clamp to the map
WL_DEV bool viewer_traversable(const WlTravMap& m, float x, float y) {
    const float width = (float)m.rows * m.row_spacing, height = (float)m.cols * m.col_spacing;
    const float fx = (x + 0.5f * width + 0.5f * m.row_spacing) / m.row_spacing;
    const float fy = (y + 0.5f * height + 0.5f * m.col_spacing) / m.col_spacing;
    const float cx = fminf(fmaxf(fx, -1.f), (float)m.rows), cy = fminf(fmaxf(fy, -1.f), (float)m.cols);   // NaN -> -1 -> 0
    const int xi = min(max((int)cx, 0), m.rows - 1), yi = min(max((int)cy, 0), m.cols - 1);
    return m.map[yi * m.cols + xi] != 0;
}

// the ground's albedo at (x, y): the traversability map when there is one, else the two-tone checker
WL_DEV V3 viewer_ground_albedo(const WlViewerParams& p, const WlTravMap& m, bool has_map, float x, float y) {
    if (has_map) {
        const float* c = kViewerTrav[viewer_traversable(m, x, y) ? 1 : 0];
        return v3(c[0], c[1], c[2]);
    }
    const float inv = 1.f / p.checker;
    const float cx = floorf(x * inv), cy = floorf(y * inv);
    const float k = cx + cy;
    const int odd = (k == k && fabsf(k) < 1.6e7f) ? ((int)k & 1) : 0;
    const float* c = kViewerChecker[odd];
    return v3(c[0], c[1], c[2]);
}

// normal of the heightfield's bilinear patch under (x, y) from the walk's copy of the codes (up outside the grid): the arithmetic of
// wl_heightfield.h::HeightFieldGround::sample_full
WL_DEV V3 viewer_field_normal(const DepthGrid& g, const Pyramid& py, const FieldMem& mem, float x, float y) {
    const float u = (x - g.x0) * g.inv_cell, v = (y - g.y0) * g.inv_cell;
    const bool inside = u >= 0.f && v >= 0.f && u < (float)g.NX && v < (float)g.NY;
    if (!inside) return v3(0.f, 0.f, 1.f);
    const float uc = fminf(u, (float)g.NX - 1e-3f), vc = fminf(v, (float)g.NY - 1e-3f);
    const float fi = floorf(uc), fj = floorf(vc);
    const int i = (int)fi, j = (int)fj;
    const float fu = uc - fi, fv = vc - fj;
    float h00, h10, h01, h11;
    const int k = 2 * py.h0 + j * g.nx + i;
    mem.ldh2(k, g.zs, h00, h10);
    mem.ldh2(k + g.nx, g.zs, h01, h11);
    const float a = fmaf(fu, h10 - h00, h00), b = fmaf(fu, h11 - h01, h01);
    const float dzdx = fmaf(fv, (h11 - h01) - (h10 - h00), h10 - h00) * g.inv_cell;
    const float dzdy = (b - a) * g.inv_cell;
    const float il = 1.f / std::sqrt(fmaf(dzdx, dzdx, fmaf(dzdy, dzdy, 1.f)));
    return v3(-dzdx * il, -dzdy * il, il);
}

// the ground of one pixel (the answer every car then has to beat): plane or heightfield, else sky; the map is read only with has_map
WL_DEV ViewerPix viewer_ground_plane(const WlViewerParams& p, const WlTravMap& m, bool has_map, V3 o, V3 d) {
    ViewerPix px;
    px.t = p.far_clip, px.id = kViewerSkyId, px.n = v3(0.f, 0.f, 1.f), px.albedo = v3(kViewerSky[0], kViewerSky[1], kViewerSky[2]);
    const float t = plane_hit(o.z, d.z, p.plane_z, 0.f, p.far_clip);
    if (t >= 0.f && t < p.far_clip) {
        px.t = t, px.id = kViewerGround;
        px.albedo = viewer_ground_albedo(p, m, has_map, fmaf(t, d.x, o.x), fmaf(t, d.y, o.y));
    }
    return px;
}
WL_DEV ViewerPix viewer_ground_field(const WlViewerParams& p, const WlTravMap& m, bool has_map, const DepthGrid& g, const Pyramid& py, const PyrHead& hd,
                                     const FieldMem& mem, V3 o, V3 d) {
    ViewerPix px;
    px.t = p.far_clip, px.id = kViewerSkyId, px.n = v3(0.f, 0.f, 1.f), px.albedo = v3(kViewerSky[0], kViewerSky[1], kViewerSky[2]);
    const float t = cast_ray(g, py, hd, mem, o, d, p.far_clip);
    if (t < p.far_clip) {
        const float x = fmaf(t, d.x, o.x), y = fmaf(t, d.y, o.y);
        px.t = t, px.id = kViewerGround;
        px.n = viewer_field_normal(g, py, mem, x, y);
        px.albedo = viewer_ground_albedo(p, m, has_map, x, y);
    }
    return px;
}

// Lambert with one sun and an ambient share; the sky is unlit.  -> 8-bit channels
WL_DEV uint8_t viewer_q8(float c) { return (uint8_t)(int)fminf(fmaxf(fmaf(c, 255.f, 0.5f), 0.f), 255.f); }
WL_DEV void viewer_shade(const WlViewerParams& p, V3 sun, const ViewerPix& px, uint8_t* rgb) {
    float k = 1.f;
    if (px.id != kViewerSkyId) k = fmaf(1.f - p.ambient, fmaxf(dot(px.n, sun), 0.f), p.ambient);
    rgb[0] = viewer_q8(k * px.albedo.x);
    rgb[1] = viewer_q8(k * px.albedo.y);
    rgb[2] = viewer_q8(k * px.albedo.z);
}
WL_DEV V3 viewer_sun(const WlViewerParams& p) {
    const V3 s = v3(p.sun[0], p.sun[1], p.sun[2]);
    const float l = std::sqrt(dot(s, s));
    return l > 0.f ? (1.f / l) * s : v3(0.f, 0.f, 1.f);
}

}  // namespace

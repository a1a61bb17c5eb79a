// wl_viewer.hip -- the viewer camera (include/wheeledlab_amd_viewer.h): one world camera drawing every env of a batch, through the
// tile bins of wl_tile_bins.h.
//   bin    one lane per env (the pose rows are SoA: the reads coalesce).  Culls the car's bounding sphere against the image plane,
//          the far clip and the frustum, writes a compact 64-byte record of each visible car, and projects the sphere to a
//          rectangle of 16 x 16-pixel tiles.
//   shade  one workgroup per tile, one lane per pixel: the ground first (plane, or the heightfield walk of wl_depth_dev.h), whose
//          distance is the bound every car must beat; then the tile's cars.
// Every pixel's answer is the minimum of (distance, env id) with the ground ranked after every car -- an order-independent
// reduction, so the frame is byte-identical from run to run.
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_viewer.h"
#include "wl_kernel_common.h"
#include "wl_tile_bins.h"
#include "wl_viewer_dev.h"

namespace {

constexpr int kTile = WL_VIEWER_TILE;
static_assert(kTile == kTileSide, "the header's tile is the bins' tile");

WL_DEV TileSpan tile_span(const ViewerCar& c) { return TileSpan{c.tx & 0xffff, c.tx >> 16, c.ty & 0xffff, c.ty >> 16, c.pad != 0}; }
inline TileLayout viewer_layout(int w, int h, int n) { return tile_layout<ViewerCar>(tiles_of(w), tiles_of(h), n); }

// the camera: world origin and rows of body -> world
struct ViewerCam {
    V3 o;
    Mat3 R;
};
WL_DEV ViewerCam viewer_cam(const WlViewerParams& p) {
    return ViewerCam{v3(p.cam_pos[0], p.cam_pos[1], p.cam_pos[2]), mat_from_quat(Quat{p.cam_quat[0], p.cam_quat[1], p.cam_quat[2], p.cam_quat[3]})};
}

// pixel bounds of a projected extent u in [lo, hi] (image-plane coordinate per unit distance) -> tile range; false: off screen
WL_DEV bool tile_range(float lo, float hi, float f, float c, int n_px, int& t0, int& t1) {
    // pixel k's centre sits at c + f u - 0.5; one pixel of margin on each side covers the rounding of either side's arithmetic
    const float a = floorf(fmaf(f, lo, c - 0.5f)) - 1.f, b = ceilf(fmaf(f, hi, c - 0.5f)) + 1.f;
    if (!(b >= 0.f) || !(a <= (float)(n_px - 1))) return false;
    t0 = (int)fmaxf(a, 0.f) / kTile;
    t1 = (int)fminf(b, (float)(n_px - 1)) / kTile;
    return true;
}

__global__ void __launch_bounds__(kBlock) viewer_bin_kernel(const WlViewerParams p, const WlEnvBuffers b, const TileBins<ViewerCar> bins) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= b.n_envs) return;
    const ViewerCam cam = viewer_cam(p);
    const float r = viewer_geom(p).bound_r;
    const Rows S = make_rows(b.state, b.stride);
    const V3 pos = ld3(S, WL_S_PX, e);
    const Quat q{S.ld(WL_S_QW, e), S.ld(WL_S_QX, e), S.ld(WL_S_QY, e), S.ld(WL_S_QZ, e)};
    const V3 rel = pos - cam.o;
    // camera coordinates: forward (body x), right (-body y), down (-body z) = columns of R
    const float z = dot(rel, v3(cam.R.r0.x, cam.R.r1.x, cam.R.r2.x));
    const float xr = -dot(rel, v3(cam.R.r0.y, cam.R.r1.y, cam.R.r2.y));
    const float yd = -dot(rel, v3(cam.R.r0.z, cam.R.r1.z, cam.R.r2.z));
    if (!(z + r > 0.f) || !(z - r < p.far_clip) || !(xr == xr) || !(yd == yd)) return;     // behind, beyond the far clip, or NaN
    const int TX = (p.width + kTile - 1) / kTile, TY = (p.height + kTile - 1) / kTile;
    int tx0 = 0, tx1 = TX - 1, ty0 = 0, ty1 = TY - 1;
    if (z - r > kViewerNear) {
        // x / z over the sphere's bounding box is extreme at its corners: a conservative rectangle
        const float izn = 1.f / (z - r), izf = 1.f / (z + r);
        const float ulo = fminf((xr - r) * izn, (xr - r) * izf), uhi = fmaxf((xr + r) * izn, (xr + r) * izf);
        const float vlo = fminf((yd - r) * izn, (yd - r) * izf), vhi = fmaxf((yd + r) * izn, (yd + r) * izf);
        if (!tile_range(ulo, uhi, p.fx, p.cx, p.width, tx0, tx1) || !tile_range(vlo, vhi, p.fy, p.cy, p.height, ty0, ty1)) return;
    }
    const int k = atomicAdd(&bins.hdr[0], 1);
    ViewerCar c;
    c.px = pos.x, c.py = pos.y, c.pz = pos.z, c.id = e, c.R = mat_from_quat(q);
    c.tx = tx0 | (tx1 << 16), c.ty = ty0 | (ty1 << 16);
    c.pad = tile_reserve(bins, k, TileSpan{tx0, tx1, ty0, ty1, false}) ? 1 : 0;
    bins.recs[k] = c;
}

template <bool FIELD>
__global__ void __launch_bounds__(kTileLanes) viewer_shade_kernel(const WlViewerParams p, const DepthGrid g, const Pyramid py,
                                                                  const float* __restrict__ pyr, const unsigned pyr_bytes, const WlTravMap m,
                                                                  const int has_map, const TileBins<ViewerCar> bins,
                                                                  uint8_t* __restrict__ rgb, float* __restrict__ depth, int32_t* __restrict__ id) {
    __shared__ ViewerCar cars[kTileLanes];
    const int tile = blockIdx.x, tx = tile % bins.TX, ty = tile / bins.TX;
    const int row = ty * kTile + (threadIdx.x >> 4), col = tx * kTile + (threadIdx.x & 15);
    const ViewerCam cam = viewer_cam(p);
    const ViewerGeom geom = viewer_geom(p);
    const V3 o = cam.o, d = mul(cam.R, viewer_ray_body(p, row, col));
    const float a = dot(d, d);
    ViewerPix px;
    if constexpr (FIELD) {
        const FieldMem mem{__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pyr), 0, (int)pyr_bytes, 0x00020000)};
        px = viewer_ground_field(p, m, has_map != 0, g, py, pyramid_head(g, py, mem), mem, o, d);
    } else {
        px = viewer_ground_plane(p, m, has_map != 0, o, d);
    }
    for_each_tile_record(bins, tile, cars, [&](const ViewerCar& car) { viewer_car(p, geom, car, o, d, a, px); });
    if (row >= p.height || col >= p.width) return;
    const int64_t pix = (int64_t)row * p.width + col;
    uint8_t c[3];
    viewer_shade(p, viewer_sun(p), px, c);
    rgb[3 * pix] = c[0], rgb[3 * pix + 1] = c[1], rgb[3 * pix + 2] = c[2];
    if (depth) depth[pix] = px.t;
    if (id) id[pix] = px.id;
}

}  // namespace

extern "C" {

int wl_viewer_version(void) { return WL_VIEWER_VERSION; }

int64_t wl_viewer_scratch_bytes(int32_t width, int32_t height, int32_t n_envs) {
    if (width <= 0 || height <= 0 || n_envs <= 0 || width > WL_VIEWER_MAX_SIDE || height > WL_VIEWER_MAX_SIDE) return WL_EINVAL;
    return viewer_layout(width, height, n_envs).total;
}

int wl_viewer_render(const WlViewerParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid, const WlTravMap* map,
                     void* scratch, int64_t scratch_bytes, uint8_t* rgb, float* depth, int32_t* id, void* stream) {
    if (!p || !b || !rgb || !scratch || !b->state) return WL_EINVAL;
    const int64_t need = wl_viewer_scratch_bytes(p->width, p->height, b->n_envs);
    if (need <= 0 || scratch_bytes < need) return WL_EINVAL;
    if (b->stride < b->n_envs || b->stride * 4 * WL_S_COUNT > 0x7fffffffLL) return WL_EINVAL;
    if (!finite_pos(p->fx) || !finite_pos(p->fy) || !(p->cx == p->cx) || !(p->cy == p->cy) || !finite_pos(p->far_clip)) return WL_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!finite_pos(p->box_half[k])) return WL_EINVAL;
    if (!finite_pos(p->wheel_radius) || !(p->ambient >= 0.f && p->ambient <= 1.f)) return WL_EINVAL;
    if (p->ground == WL_VIEWER_HEIGHTFIELD) {
        if (!pyramid || heightfield_args_ok(hf, HF_PYRAMID) != WL_OK) return WL_EINVAL;
    } else if (p->ground != WL_VIEWER_PLANE || hf || pyramid || !(p->plane_z == p->plane_z)) {
        return WL_EINVAL;
    }
    if (map) {
        if (!map->map || map->rows <= 0 || map->cols != map->rows || !finite_pos(map->row_spacing) || !finite_pos(map->col_spacing)) return WL_EINVAL;
    } else if (!finite_pos(p->checker)) {
        return WL_EINVAL;
    }
    if (!aligned(scratch, 16)) return WL_EALIGN;
    const TileLayout s = viewer_layout(p->width, p->height, b->n_envs);
    const TileBins<ViewerCar> bins = s.carve<ViewerCar>(scratch);
    const hipStream_t hs = (hipStream_t)stream;
    clear_error();
    if (!tile_bins_build(s, bins, b->n_envs, hs, [&] { viewer_bin_kernel<<<grid_for(b->n_envs), kBlock, 0, hs>>>(*p, *b, bins); }))
        return WL_ELAUNCH;
    const unsigned T = (unsigned)s.T;
    const WlTravMap m = map ? *map : WlTravMap{};
    if (p->ground == WL_VIEWER_HEIGHTFIELD) {
        const Pyramid py = make_pyramid(hf->nx, hf->ny);
        const unsigned bytes = (unsigned)(pyramid_total_floats(hf->nx, hf->ny) * 4);
        viewer_shade_kernel<true><<<T, kTileLanes, 0, hs>>>(*p, make_depth_grid(hf), py, pyramid, bytes, m, map ? 1 : 0, bins, rgb, depth, id);
    } else {
        viewer_shade_kernel<false><<<T, kTileLanes, 0, hs>>>(*p, DepthGrid{}, Pyramid{}, nullptr, 0u, m, map ? 1 : 0, bins, rgb, depth, id);
    }
    return launch_status();
}

}  // extern "C"

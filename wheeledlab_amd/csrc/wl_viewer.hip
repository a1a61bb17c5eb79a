// wl_viewer.hip -- the viewer camera (include/wheeledlab_amd_viewer.h): one world camera drawing every env of a batch.
//
// Four launches per frame after one memset of the counters:
//   1. bin    one lane per env (the pose rows are SoA: the reads coalesce).  Culls the car's bounding sphere against the image plane,
//             the far clip and the frustum, writes a compact 64-byte record of each visible car, and projects the sphere to a
//             rectangle of 16 x 16-pixel tiles.  A car whose rectangle is small (<= kMaxTilesPerCar tiles) and still fits the
//             entry budget is counted into each of its tiles; any other car goes to the BIG list every tile scans.
//   2. scan   one workgroup: exclusive scan of the per-tile counts -> list offsets.
//   3. fill   one lane per record: its index into each of its tiles' lists.
//   4. shade  one workgroup per tile, one lane per pixel: the ground first (plane, or the heightfield walk of wl_depth_dev.h), whose
//             distance is the bound every car must beat; then the tile's cars, staged through LDS 256 records at a time, then the
//             big list, filtered by tile.  Lists are complete: a tile with more cars than one LDS chunk loops over chunks.
// Which lane or block fills which slot of a list is up to the atomics, but every pixel's answer is the minimum of (distance, env id)
// with the ground ranked after every car -- an order-independent reduction, so the frame is byte-identical from run to run.
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_viewer.h"
#include "wl_kernel_common.h"
#include "wl_viewer_dev.h"

namespace {

constexpr int kTile = WL_VIEWER_TILE;
constexpr int kShade = kTile * kTile;          // threads of a shade workgroup = pixels of a tile = records per LDS chunk
constexpr int kMaxTilesPerCar = 64;            // larger rectangles go to the big list
constexpr int kHdrInts = 16;                   // [0] visible cars, [1] big-list cars, [2] list entries reserved

// scratch layout (bytes, every section 16-byte aligned)
struct ViewerScratch {
    int64_t hdr, count, off, recs, big, big_tiles, entries, total;
    int64_t n_entries;
};
inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline ViewerScratch viewer_scratch(int w, int h, int n) {
    const int64_t T = (int64_t)((w + kTile - 1) / kTile) * ((h + kTile - 1) / kTile);
    ViewerScratch s;
    s.n_entries = std::max<int64_t>(8 * (int64_t)n, (int64_t)1 << 21);
    s.hdr = 0;
    s.count = align16(kHdrInts * 4);
    s.off = s.count + align16((T + 1) * 4);
    s.recs = s.off + align16((T + 1) * 4);
    s.big = s.recs + (int64_t)n * (int64_t)sizeof(ViewerCar);
    s.big_tiles = s.big + align16((int64_t)n * 4);
    s.entries = s.big_tiles + align16((int64_t)n * 8);
    s.total = s.entries + align16(s.n_entries * 4);
    return s;
}

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

__global__ void __launch_bounds__(kBlock) viewer_bin_kernel(const WlViewerParams p, const WlEnvBuffers b, int* __restrict__ hdr,
                                                            int* __restrict__ count, ViewerCar* __restrict__ recs, int* __restrict__ big,
                                                            int2* __restrict__ big_tiles, const int n_entries) {
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
    const int k = atomicAdd(&hdr[0], 1);
    const Mat3 R = mat_from_quat(q);
    ViewerCar c;
    c.px = pos.x, c.py = pos.y, c.pz = pos.z, c.id = e, c.R = R;
    c.tx = tx0 | (tx1 << 16), c.ty = ty0 | (ty1 << 16);
    const int nt = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
    bool listed = nt <= kMaxTilesPerCar;
    if (listed) listed = atomicAdd(&hdr[2], nt) + nt <= n_entries;
    c.pad = listed ? 1 : 0;
    recs[k] = c;
    if (listed) {
        const int TXs = TX;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&count[ty * TXs + tx], 1);
    } else {
        const int bi = atomicAdd(&hdr[1], 1);
        big[bi] = k;
        big_tiles[bi] = make_int2(c.tx, c.ty);
    }
}

// exclusive scan of count[0 .. T) into off[0 .. T] (off[T] = the total); count is zeroed for the fill's cursors
__global__ void __launch_bounds__(1024) viewer_scan_kernel(int* __restrict__ count, int* __restrict__ off, const int T) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < T; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < T ? count[i] : 0;
        int s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(s, d, 64);
            if (lane >= d) s += u;
        }
        if (lane == 63) wsum[wid] = s;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wid; ++w) before += wsum[w];
        if (i < T) {
            off[i] = before + s - v;
            count[i] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[T] = carry_s;
}

__global__ void __launch_bounds__(kBlock) viewer_fill_kernel(const WlViewerParams p, const int* __restrict__ hdr, int* __restrict__ cursor,
                                                             const int* __restrict__ off, const ViewerCar* __restrict__ recs,
                                                             int* __restrict__ entries, const int n_max) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_max || k >= hdr[0]) return;
    const ViewerCar& c = recs[k];
    if (!c.pad) return;
    const int TX = (p.width + kTile - 1) / kTile;
    const int tx0 = c.tx & 0xffff, tx1 = c.tx >> 16, ty0 = c.ty & 0xffff, ty1 = c.ty >> 16;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int t = ty * TX + tx;
            entries[off[t] + atomicAdd(&cursor[t], 1)] = k;
        }
}

template <bool FIELD>
__global__ void __launch_bounds__(kShade) viewer_shade_kernel(const WlViewerParams p, const DepthGrid g, const Pyramid py,
                                                              const float* __restrict__ pyr, const unsigned pyr_bytes, const WlTravMap m,
                                                              const int has_map, const int* __restrict__ hdr, const int* __restrict__ off,
                                                              const ViewerCar* __restrict__ recs, const int* __restrict__ entries,
                                                              const int* __restrict__ big, const int2* __restrict__ big_tiles,
                                                              uint8_t* __restrict__ rgb, float* __restrict__ depth, int32_t* __restrict__ id) {
    __shared__ ViewerCar cars[kShade];
    __shared__ int n_sel;
    const int TX = (p.width + kTile - 1) / kTile;
    const int tile = blockIdx.x, tx = tile % TX, ty = tile / TX;
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
    // the tile's own list
    const int beg = off[tile], end = off[tile + 1];
    for (int c0 = beg; c0 < end; c0 += kShade) {
        if (c0 + (int)threadIdx.x < end) cars[threadIdx.x] = recs[entries[c0 + threadIdx.x]];
        __syncthreads();
        const int nc = min(kShade, end - c0);
        for (int j = 0; j < nc; ++j) viewer_car(p, geom, cars[j], o, d, a, px);
        __syncthreads();
    }
    // the big list: every tile filters it by its own rectangle
    const int nb = hdr[1];
    for (int c0 = 0; c0 < nb; c0 += kShade) {
        if (threadIdx.x == 0) n_sel = 0;
        __syncthreads();
        const int k = c0 + threadIdx.x;
        if (k < nb) {
            const int2 r = big_tiles[k];
            if (tx >= (r.x & 0xffff) && tx <= (r.x >> 16) && ty >= (r.y & 0xffff) && ty <= (r.y >> 16))
                cars[atomicAdd(&n_sel, 1)] = recs[big[k]];
        }
        __syncthreads();
        const int nc = n_sel;
        for (int j = 0; j < nc; ++j) viewer_car(p, geom, cars[j], o, d, a, px);
        __syncthreads();
    }
    if (row >= p.height || col >= p.width) return;
    const int64_t pix = (int64_t)row * p.width + col;
    uint8_t c[3];
    viewer_shade(p, viewer_sun(p), px, c);
    rgb[3 * pix] = c[0], rgb[3 * pix + 1] = c[1], rgb[3 * pix + 2] = c[2];
    if (depth) depth[pix] = px.t;
    if (id) id[pix] = px.id;
}

inline bool finite_pos(float x) { return x > 0.f && x < INFINITY; }

}  // namespace

extern "C" {

int wl_viewer_version(void) { return WL_VIEWER_VERSION; }

int64_t wl_viewer_scratch_bytes(int32_t width, int32_t height, int32_t n_envs) {
    if (width <= 0 || height <= 0 || n_envs <= 0 || width > WL_VIEWER_MAX_SIDE || height > WL_VIEWER_MAX_SIDE) return WL_EINVAL;
    return viewer_scratch(width, height, n_envs).total;
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
    if (((uintptr_t)scratch & 15) != 0) return WL_EALIGN;
    const ViewerScratch s = viewer_scratch(p->width, p->height, b->n_envs);
    char* base = static_cast<char*>(scratch);
    int* hdr = reinterpret_cast<int*>(base + s.hdr);
    int* count = reinterpret_cast<int*>(base + s.count);
    int* off = reinterpret_cast<int*>(base + s.off);
    ViewerCar* recs = reinterpret_cast<ViewerCar*>(base + s.recs);
    int* big = reinterpret_cast<int*>(base + s.big);
    int2* big_tiles = reinterpret_cast<int2*>(base + s.big_tiles);
    int* entries = reinterpret_cast<int*>(base + s.entries);
    const int TX = (p->width + kTile - 1) / kTile, TY = (p->height + kTile - 1) / kTile, T = TX * TY;
    const hipStream_t hs = (hipStream_t)stream;
    clear_error();
    if (hipMemsetAsync(base, 0, (size_t)s.off, hs) != hipSuccess) return WL_ELAUNCH;     // header and per-tile counts
    const int n_entries = (int)std::min<int64_t>(s.n_entries, 0x7fffffff);
    viewer_bin_kernel<<<grid_for(b->n_envs), kBlock, 0, hs>>>(*p, *b, hdr, count, recs, big, big_tiles, n_entries);
    viewer_scan_kernel<<<1, 1024, 0, hs>>>(count, off, T);
    viewer_fill_kernel<<<grid_for(b->n_envs), kBlock, 0, hs>>>(*p, hdr, count, off, recs, entries, b->n_envs);
    const WlTravMap m = map ? *map : WlTravMap{};
    if (p->ground == WL_VIEWER_HEIGHTFIELD) {
        const Pyramid py = make_pyramid(hf->nx, hf->ny);
        const unsigned bytes = (unsigned)(pyramid_total_floats(hf->nx, hf->ny) * 4);
        viewer_shade_kernel<true><<<T, kShade, 0, hs>>>(*p, make_depth_grid(hf), py, pyramid, bytes, m, map ? 1 : 0, hdr, off, recs, entries,
                                                        big, big_tiles, rgb, depth, id);
    } else {
        viewer_shade_kernel<false><<<T, kShade, 0, hs>>>(*p, DepthGrid{}, Pyramid{}, nullptr, 0u, m, map ? 1 : 0, hdr, off, recs, entries,
                                                         big, big_tiles, rgb, depth, id);
    }
    return launch_status();
}

}  // extern "C"

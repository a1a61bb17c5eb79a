// wl_terrain.hip -- mesh terrains (include/wheeledlab_amd_terrain.h): rasterise a triangle mesh into the height lattice.
//
// Meshes mix a few huge triangles with millions of small ones, so one lane per triangle walking its footprint would leave one lane
// with millions of points while the rest idle.  The tile bins of wl_tile_bins.h instead:
//   bin     one lane per face: loads and validates its three vertices, sorts them (lexicographic x, y: every edge's canonical
//           order), drops zero projected area, culls against the lattice and writes a 64-byte record of its lattice-index rectangle.
//   raster  one workgroup per tile of 16 x 16 lattice points, one lane per point: a running maximum in registers over the tile's
//           records, each height written once.
// Every point's answer is a maximum: the output does not depend on the order of the lists, and is byte-identical from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_kernel_common.h"
#include "wl_tile_bins.h"

namespace {

constexpr int kTile = WL_TERRAIN_TILE;
static_assert(kTile == kTileSide && WL_TERRAIN_MAX_TILES_PER_FACE == kMaxTilesPerRecord, "the header's tiles are the bins' tiles");
constexpr int kHdrInvalid = 4;                 // the caller's header word: invalid faces

// one binned face: vertices sorted lexicographically by (x, y); `sgn` +1 when (v0, v1, v2) turns counter-clockwise seen from +z
struct MeshTri {
    float x[3], y[3], z[3];
    int sgn;
    int listed;                                // 1: on its tiles' lists, 0: on the big list
    int pad;
    int i0, i1, j0, j1;                        // lattice points its bounding box may cover (inclusive, clamped to the lattice)
};
static_assert(sizeof(MeshTri) == 64, "a record is 64 bytes, its rectangle one 16-byte slot");

WL_DEV TileSpan tile_span(const MeshTri& t) { return TileSpan{t.i0 / kTile, t.i1 / kTile, t.j0 / kTile, t.j1 / kTile, t.listed != 0}; }
inline TileLayout mesh_layout(int n_faces, int nx, int ny) { return tile_layout<MeshTri>(tiles_of(nx), tiles_of(ny), n_faces); }

// The edge function of (a -> b) at p, in double from float coordinates, with ONE rounding sequence whatever the caller: a
// triangle's edges are always taken from their lexicographically smaller endpoint, so two triangles sharing an edge compute the
// same value on it (exactly negated when their windings differ) and a point on it is covered by both.  The fma is written out:
// the build contracts `a * b - c * d` as it likes, and both products rounded differently would break that sharing.
WL_DEV double edge_fn(double ax, double ay, double bx, double by, double px, double py) {
    return fma(bx - ax, py - ay, -((by - ay) * (px - ax)));
}

// the point (i, j) at (px, py) against one record: the running maximum `best`, `hit` once anything covers the point
WL_DEV void raster_tri(const MeshTri& t, int i, int j, double px, double py, float& best, bool& hit) {
    if (i < t.i0 || i > t.i1 || j < t.j0 || j > t.j1) return;
    const double x0 = t.x[0], y0 = t.y[0], x1 = t.x[1], y1 = t.y[1], x2 = t.x[2], y2 = t.y[2];
    // a point ON a vertex takes that vertex's height exactly (the closed triangle covers it)
    float z;
    if (px == x0 && py == y0) {
        z = t.z[0];
    } else if (px == x1 && py == y1) {
        z = t.z[1];
    } else if (px == x2 && py == y2) {
        z = t.z[2];
    } else {
        const double s = (double)t.sgn;
        const double w0 = s * edge_fn(x1, y1, x2, y2, px, py);      // barycentric weights: zero on the opposite edge
        const double w1 = -s * edge_fn(x0, y0, x2, y2, px, py);
        const double w2 = s * edge_fn(x0, y0, x1, y1, px, py);
        if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) return;
        const double W = w0 + w1 + w2;
        if (!(W > 0.0)) return;                                      // a needle whose three edge values all round to zero here
        z = (float)((w0 * (double)t.z[0] + w1 * (double)t.z[1] + w2 * (double)t.z[2]) / W);
    }
    best = hit ? fmaxf(best, z) : z;
    hit = true;
}

WL_DEV bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

__global__ void __launch_bounds__(kBlock) mesh_bin_kernel(const WlMeshRasterParams p, const float* __restrict__ verts, const int n_verts,
                                                          const int* __restrict__ faces, const int n_faces, const TileBins<MeshTri> bins) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
    if ((unsigned)ia >= (unsigned)n_verts || (unsigned)ib >= (unsigned)n_verts || (unsigned)ic >= (unsigned)n_verts) {
        atomicAdd(&bins.hdr[kHdrInvalid], 1);
        return;
    }
    float x[3], y[3], z[3];
    const int idx[3] = {ia, ib, ic};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* v = verts + 3 * (int64_t)idx[k];
        x[k] = v[0], y[k] = v[1], z[k] = v[2];
    }
    if (!finite3(x[0], y[0], z[0]) || !finite3(x[1], y[1], z[1]) || !finite3(x[2], y[2], z[2])) {
        atomicAdd(&bins.hdr[kHdrInvalid], 1);
        return;
    }
    // sort by (x, y): three compare-exchanges
    auto cswap = [&](int a, int b) {
        if (x[b] < x[a] || (x[b] == x[a] && y[b] < y[a])) {
            const float tx = x[a], ty = y[a], tz = z[a];
            x[a] = x[b], y[a] = y[b], z[a] = z[b];
            x[b] = tx, y[b] = ty, z[b] = tz;
        }
    };
    cswap(0, 1);
    cswap(1, 2);
    cswap(0, 1);
    // twice the signed projected area (for coordinates of one magnitude the differences and products are exact in double)
    const double area2 = edge_fn(x[0], y[0], x[1], y[1], x[2], y[2]);
    if (area2 == 0.0) return;                                        // a vertical wall or a degenerate face: nothing to see from above
    // lattice-index rectangle: floor / ceil of the bounding box in lattice units (at most one point wider than the exact one)
    const double cell = p.cell, ox = p.x0, oy = p.y0;
    const double ylo = fmin(fmin((double)y[0], (double)y[1]), (double)y[2]), yhi = fmax(fmax((double)y[0], (double)y[1]), (double)y[2]);
    const double a0 = floor(((double)x[0] - ox) / cell), a1 = ceil(((double)x[2] - ox) / cell);
    const double b0 = floor((ylo - oy) / cell), b1 = ceil((yhi - oy) / cell);
    if (a1 < 0.0 || b1 < 0.0 || a0 > (double)(p.nx - 1) || b0 > (double)(p.ny - 1)) return;   // off the lattice
    MeshTri t;
#pragma unroll
    for (int k = 0; k < 3; ++k) t.x[k] = x[k], t.y[k] = y[k], t.z[k] = z[k];
    t.sgn = area2 > 0.0 ? 1 : -1;
    t.pad = 0, t.listed = 0;
    t.i0 = (int)fmax(a0, 0.0), t.i1 = (int)fmin(a1, (double)(p.nx - 1));
    t.j0 = (int)fmax(b0, 0.0), t.j1 = (int)fmin(b1, (double)(p.ny - 1));
    const int k = atomicAdd(&bins.hdr[0], 1);
    t.listed = tile_reserve(bins, k, tile_span(t)) ? 1 : 0;
    bins.recs[k] = t;
}

__global__ void __launch_bounds__(kTileLanes) mesh_raster_kernel(const WlMeshRasterParams p, const TileBins<MeshTri> bins,
                                                                 float* __restrict__ heights, int* __restrict__ status) {
    __shared__ MeshTri tris[kTileLanes];
    const int tile = blockIdx.x, tx = tile % bins.TX, ty = tile / bins.TX;
    const int i = tx * kTile + (threadIdx.x & (kTile - 1)), j = ty * kTile + (int)(threadIdx.x / kTile);
    const double px = (double)p.x0 + (double)i * (double)p.cell, py = (double)p.y0 + (double)j * (double)p.cell;
    float best = 0.f;
    bool hit = false;
    for_each_tile_record(bins, tile, tris, [&](const MeshTri& t) { raster_tri(t, i, j, px, py, best, hit); });
    if (i < p.nx && j < p.ny) heights[(int64_t)j * p.nx + i] = hit ? best : p.fill_z;
    if (tile == 0 && threadIdx.x == 0) {
        status[0] = bins.hdr[kHdrInvalid], status[1] = bins.hdr[0], status[2] = bins.hdr[1], status[3] = bins.off[gridDim.x];
    }
}

}  // namespace

extern "C" {

int wl_terrain_version(void) { return WL_TERRAIN_VERSION; }

int64_t wl_mesh_raster_scratch_bytes(int32_t n_faces, int32_t nx, int32_t ny) {
    if (n_faces < 0 || nx < 2 || ny < 2 || nx >= WL_TERRAIN_MAX_SIDE || ny >= WL_TERRAIN_MAX_SIDE || (int64_t)nx * ny > 0x7fffffffLL)
        return WL_EINVAL;
    return mesh_layout(n_faces, nx, ny).total;
}

int wl_mesh_raster(const WlMeshRasterParams* p, const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                   void* scratch, int64_t scratch_bytes, float* heights_out, int32_t* status_out, void* stream) {
    if (!p || !scratch || !heights_out || !status_out || n_vertices < 0 || n_faces < 0) return WL_EINVAL;
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return WL_EINVAL;
    if (!finite_pos(p->cell) || !std::isfinite(p->x0) || !std::isfinite(p->y0) || !std::isfinite(p->fill_z)) return WL_EINVAL;
    const int64_t need = wl_mesh_raster_scratch_bytes(n_faces, p->nx, p->ny);
    if (need <= 0 || scratch_bytes < need) return WL_EINVAL;
    if (!aligned(scratch, 16) || !aligned(vertices, 4) || !aligned(faces, 4) || !aligned(heights_out, 4) || !aligned(status_out, 4))
        return WL_EALIGN;
    const TileLayout s = mesh_layout(n_faces, p->nx, p->ny);
    const TileBins<MeshTri> bins = s.carve<MeshTri>(scratch);
    const hipStream_t hs = (hipStream_t)stream;
    clear_error();
    if (!tile_bins_build(s, bins, n_faces, hs,
                         [&] { mesh_bin_kernel<<<grid_for(n_faces), kBlock, 0, hs>>>(*p, vertices, n_vertices, faces, n_faces, bins); }))
        return WL_ELAUNCH;
    mesh_raster_kernel<<<(unsigned)s.T, kTileLanes, 0, hs>>>(*p, bins, heights_out, status_out);
    return launch_status();
}

}  // extern "C"

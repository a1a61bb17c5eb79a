// wl_terrain.hip -- mesh terrains (include/wheeledlab_amd_terrain.h): rasterise a triangle mesh into the height lattice.
//
// Meshes mix a few huge triangles with millions of small ones, so one lane per triangle walking its footprint would leave one lane
// with millions of points while the rest idle.  The viewer's binned pattern (wl_viewer.hip) instead, four launches after one memset
// of the counters:
//   1. bin     one lane per face: loads and validates its three vertices, sorts them (lexicographic x, y: every edge's canonical
//              order), drops zero projected area, culls against the lattice and writes a 64-byte record of its lattice-index
//              rectangle.  A face spanning <= kMaxTilesPerFace tiles of 16 x 16 points, and still within the entry budget, is counted
//              into each of its tiles; any other face goes to the BIG list every tile filters.
//   2. scan    one workgroup: exclusive scan of the per-tile counts (4096 per pass, carried across passes) -> list offsets.
//   3. fill    one lane per record: its index into each of its tiles' lists.
//   4. raster  one workgroup per tile, one lane per lattice point: the tile's records staged through LDS 256 at a time, then the
//              big list filtered by tile; a running maximum in registers, each height written once.
// Which lane fills which slot of a list is up to the atomics, but every point's answer is a maximum: the output does not depend on
// the order, and is byte-identical from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_kernel_common.h"

namespace {

constexpr int kTile = WL_TERRAIN_TILE;
constexpr int kRaster = kTile * kTile;         // threads of a raster workgroup = points of a tile = records per LDS chunk
constexpr int kMaxTilesPerFace = WL_TERRAIN_MAX_TILES_PER_FACE;
constexpr int kScan = 1024;                    // scan workgroup; 4 counts per lane and pass
constexpr int kHdrInts = 16;                   // [0] records, [1] big-list faces, [3] invalid faces, [4..5] entries reserved (uint64)

// one binned face: vertices sorted lexicographically by (x, y); `sgn` +1 when (v0, v1, v2) turns counter-clockwise seen from +z
struct MeshTri {
    float x[3], y[3], z[3];
    int sgn;
    int listed;                                // 1: on its tiles' lists, 0: on the big list
    int pad;
    int i0, i1, j0, j1;                        // lattice points its bounding box may cover (inclusive, clamped to the lattice)
};
static_assert(sizeof(MeshTri) == 64, "a record is 64 bytes: one int4 load of its rectangle at offset 48");

// scratch layout (bytes, every section 16-byte aligned)
struct MeshScratch {
    int64_t hdr, count, off, recs, big, entries, total;
    int64_t n_entries;
};
inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline int64_t tiles_of(int n) { return (n + kTile - 1) / kTile; }
inline MeshScratch mesh_scratch(int n_faces, int nx, int ny) {
    const int64_t T = tiles_of(nx) * tiles_of(ny);
    MeshScratch s;
    s.n_entries = std::min<int64_t>(std::max<int64_t>(8 * (int64_t)n_faces, (int64_t)1 << 21), 0x7fffffff);
    s.hdr = 0;
    s.count = align16(kHdrInts * 4);
    s.off = s.count + align16((T + 1) * 4);
    s.recs = s.off + align16((T + 1) * 4);
    s.big = s.recs + (int64_t)n_faces * (int64_t)sizeof(MeshTri);
    s.entries = s.big + align16((int64_t)n_faces * 4);
    s.total = s.entries + align16(s.n_entries * 4);
    return s;
}

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
                                                          const int* __restrict__ faces, const int n_faces, int* __restrict__ hdr,
                                                          int* __restrict__ count, MeshTri* __restrict__ recs, int* __restrict__ big,
                                                          const int n_entries) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
    if ((unsigned)ia >= (unsigned)n_verts || (unsigned)ib >= (unsigned)n_verts || (unsigned)ic >= (unsigned)n_verts) {
        atomicAdd(&hdr[3], 1);
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
        atomicAdd(&hdr[3], 1);
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
    t.pad = 0;
    t.i0 = (int)fmax(a0, 0.0), t.i1 = (int)fmin(a1, (double)(p.nx - 1));
    t.j0 = (int)fmax(b0, 0.0), t.j1 = (int)fmin(b1, (double)(p.ny - 1));
    const int tx0 = t.i0 / kTile, tx1 = t.i1 / kTile, ty0 = t.j0 / kTile, ty1 = t.j1 / kTile;
    const int64_t nt = (int64_t)(tx1 - tx0 + 1) * (ty1 - ty0 + 1);
    bool listed = nt <= kMaxTilesPerFace;
    if (listed) listed = atomicAdd(reinterpret_cast<unsigned long long*>(hdr + 4), (unsigned long long)nt) + nt <= (uint64_t)n_entries;
    t.listed = listed ? 1 : 0;
    const int k = atomicAdd(&hdr[0], 1);
    recs[k] = t;
    if (listed) {
        const int TX = (p.nx + kTile - 1) / kTile;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&count[ty * TX + tx], 1);
    } else {
        big[atomicAdd(&hdr[1], 1)] = k;
    }
}

// exclusive scan of count[0 .. T) into off[0 .. T] (off[T] = the total), 4096 counts per pass with the carry held in LDS; count is
// zeroed for the fill's cursors.  Last, the status words.
__global__ void __launch_bounds__(kScan) mesh_scan_kernel(int* __restrict__ count, int* __restrict__ off, const int64_t T,
                                                          const int* __restrict__ hdr, int* __restrict__ status) {
    __shared__ int wsum[kScan / 64];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < T; base += 4 * kScan) {
        const int64_t i = base + 4 * (int64_t)threadIdx.x;
        int v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = i + q < T ? count[i + q] : 0;
        const int v4 = v[0] + v[1] + v[2] + v[3];
        int s = v4;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(s, d, 64);
            if (lane >= d) s += u;
        }
        if (lane == 63) wsum[wid] = s;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wid; ++w) before += wsum[w];
        int run = before + s - v4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i + q < T) {
                off[i + q] = run;
                count[i + q] = 0;
                run += v[q];
            }
        __syncthreads();
        if (threadIdx.x == kScan - 1) carry_s = before + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[T] = carry_s;
        status[0] = hdr[3], status[1] = hdr[0], status[2] = hdr[1], status[3] = carry_s;
    }
}

__global__ void __launch_bounds__(kBlock) mesh_fill_kernel(const int* __restrict__ hdr, int* __restrict__ cursor, const int* __restrict__ off,
                                                           const MeshTri* __restrict__ recs, int* __restrict__ entries, const int n_max,
                                                           const int TX) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_max || k >= hdr[0]) return;
    const MeshTri& t = recs[k];
    if (!t.listed) return;
    const int tx0 = t.i0 / kTile, tx1 = t.i1 / kTile, ty0 = t.j0 / kTile, ty1 = t.j1 / kTile;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int c = ty * TX + tx;
            entries[off[c] + atomicAdd(&cursor[c], 1)] = k;
        }
}

__global__ void __launch_bounds__(kRaster) mesh_raster_kernel(const WlMeshRasterParams p, const int* __restrict__ hdr, const int* __restrict__ off,
                                                              const MeshTri* __restrict__ recs, const int* __restrict__ entries,
                                                              const int* __restrict__ big, float* __restrict__ heights) {
    __shared__ MeshTri tris[kRaster];
    __shared__ int n_sel;
    const int TX = (p.nx + kTile - 1) / kTile;
    const int tile = blockIdx.x, tx = tile % TX, ty = tile / TX;
    const int i = tx * kTile + (threadIdx.x & (kTile - 1)), j = ty * kTile + (int)(threadIdx.x / kTile);
    const double px = (double)p.x0 + (double)i * (double)p.cell, py = (double)p.y0 + (double)j * (double)p.cell;
    float best = 0.f;
    bool hit = false;
    // the tile's own list
    const int beg = off[tile], end = off[tile + 1];
    for (int c0 = beg; c0 < end; c0 += kRaster) {
        if (c0 + (int)threadIdx.x < end) tris[threadIdx.x] = recs[entries[c0 + threadIdx.x]];
        __syncthreads();
        const int nc = min(kRaster, end - c0);
        for (int q = 0; q < nc; ++q) raster_tri(tris[q], i, j, px, py, best, hit);
        __syncthreads();
    }
    // the big list: every tile keeps the faces whose rectangle meets its own
    const int nb = hdr[1];
    const int ti0 = tx * kTile, ti1 = ti0 + kTile - 1, tj0 = ty * kTile, tj1 = tj0 + kTile - 1;
    for (int c0 = 0; c0 < nb; c0 += kRaster) {
        if (threadIdx.x == 0) n_sel = 0;
        __syncthreads();
        const int k = c0 + threadIdx.x;
        if (k < nb) {
            const int r = big[k];
            const int4 b = *reinterpret_cast<const int4*>(&recs[r].i0);
            if (b.x <= ti1 && b.y >= ti0 && b.z <= tj1 && b.w >= tj0) tris[atomicAdd(&n_sel, 1)] = recs[r];
        }
        __syncthreads();
        const int nc = n_sel;
        for (int q = 0; q < nc; ++q) raster_tri(tris[q], i, j, px, py, best, hit);
        __syncthreads();
    }
    if (i < p.nx && j < p.ny) heights[(int64_t)j * p.nx + i] = hit ? best : p.fill_z;
}

inline bool finite_pos(float x) { return x > 0.f && x < INFINITY; }
inline bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

}  // namespace

extern "C" {

int wl_terrain_version(void) { return WL_TERRAIN_VERSION; }

int64_t wl_mesh_raster_scratch_bytes(int32_t n_faces, int32_t nx, int32_t ny) {
    if (n_faces < 0 || nx < 2 || ny < 2 || nx >= WL_TERRAIN_MAX_SIDE || ny >= WL_TERRAIN_MAX_SIDE || (int64_t)nx * ny > 0x7fffffffLL)
        return WL_EINVAL;
    return mesh_scratch(n_faces, nx, ny).total;
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
    const MeshScratch s = mesh_scratch(n_faces, p->nx, p->ny);
    char* base = static_cast<char*>(scratch);
    int* hdr = reinterpret_cast<int*>(base + s.hdr);
    int* count = reinterpret_cast<int*>(base + s.count);
    int* off = reinterpret_cast<int*>(base + s.off);
    MeshTri* recs = reinterpret_cast<MeshTri*>(base + s.recs);
    int* big = reinterpret_cast<int*>(base + s.big);
    int* entries = reinterpret_cast<int*>(base + s.entries);
    const int TX = (int)tiles_of(p->nx);
    const int64_t T = tiles_of(p->nx) * tiles_of(p->ny);
    const hipStream_t hs = (hipStream_t)stream;
    clear_error();
    if (hipMemsetAsync(base, 0, (size_t)s.off, hs) != hipSuccess) return WL_ELAUNCH;     // header and per-tile counts
    if (n_faces > 0)
        mesh_bin_kernel<<<grid_for(n_faces), kBlock, 0, hs>>>(*p, vertices, n_vertices, faces, n_faces, hdr, count, recs, big,
                                                              (int)s.n_entries);
    mesh_scan_kernel<<<1, kScan, 0, hs>>>(count, off, T, hdr, status_out);
    if (n_faces > 0) mesh_fill_kernel<<<grid_for(n_faces), kBlock, 0, hs>>>(hdr, count, off, recs, entries, n_faces, TX);
    mesh_raster_kernel<<<(unsigned)T, kRaster, 0, hs>>>(*p, hdr, off, recs, entries, big, heights_out);
    return launch_status();
}

}  // extern "C"

// wl_tile_bins.h -- tile binning: sort 64-byte records into per-tile lists of a 2-D grid of 16 x 16 tiles, one workgroup per tile
// consuming them.  Used by the viewer camera (records: visible cars, tiles of pixels) and the mesh rasteriser (records: faces, tiles
// of lattice points).  Four launches after one memset of the header and the counts:
//   1. bin      the CALLER's kernel: makes record k = atomicAdd(&hdr[0], 1) and calls tile_reserve(bins, k, its tile rectangle):
//               a record of <= kMaxTilesPerRecord tiles that still fits the entry budget is counted into each of its tiles, any
//               other goes to the BIG list every tile filters.  The kernel stores the answer in the record (TileSpan::listed).
//   2. scan     tile_scan_kernel, one workgroup: exclusive scan of the per-tile counts -> list offsets.
//   3. fill     tile_fill_kernel, one lane per record: its index into each of its tiles' lists.
//   4. consume  the CALLER's kernel, one workgroup of kTileLanes per tile: for_each_tile_record() stages the tile's list through LDS
//               one chunk at a time, then the big list filtered by rectangle, and calls visit(record) for each.
// Which lane fills which slot of a list is up to the atomics: a consumer must reduce its records in an order-independent way.
// A record type Rec is 64 bytes and has an overload `TileSpan tile_span(const Rec&)`.
// Header words (int): [0] records, [1] big-list records, [2..3] list entries reserved (one uint64: n records x 64 tiles can pass
// 2^31; more than the lists hold once the budget is exceeded), [4 ..] the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "wl_kernel_common.h"

namespace {

constexpr int kTileSide = 16;
constexpr int kTileLanes = kTileSide * kTileSide;      // threads of a consuming workgroup = records per LDS chunk
constexpr int kMaxTilesPerRecord = 64;                 // larger rectangles go to the big list
constexpr int kTileHdrInts = 16;
constexpr int kTileScan = 1024;                        // scan workgroup; 4 counts per lane and pass

// a record's inclusive tile rectangle, and whether it is on its tiles' lists (else on the big list)
struct TileSpan {
    int tx0, tx1, ty0, ty1;
    bool listed;
};

inline int tiles_of(int n) { return (n + kTileSide - 1) / kTileSide; }

// the carved scratch as the kernels see it
template <class Rec>
struct TileBins {
    int *hdr, *count, *off;                            // off[T + 1]; count[T] doubles as the fill's cursors
    Rec* recs;
    int *big, *entries;
    int TX, n_entries;
};

// scratch layout (bytes, every section 16-byte aligned) of a TX x TY grid and at most n records
struct TileLayout {
    int64_t count, off, recs, big, entries, total;     // the header is at 0
    int64_t T;
    int TX, n_entries;                                 // entry budget max(8 n, 2^21), clamped: off[] is int
    template <class Rec>
    TileBins<Rec> carve(void* scratch) const {
        char* base = static_cast<char*>(scratch);
        auto ints = [&](int64_t o) { return reinterpret_cast<int*>(base + o); };
        return TileBins<Rec>{ints(0), ints(count), ints(off), reinterpret_cast<Rec*>(base + recs), ints(big), ints(entries), TX, n_entries};
    }
};
template <class Rec>
inline TileLayout tile_layout(int TX, int TY, int64_t n) {
    static_assert(sizeof(Rec) == 64, "a record is four 16-byte slots");
    TileLayout s;
    s.TX = TX, s.T = (int64_t)TX * TY;
    s.n_entries = (int)std::min<int64_t>(std::max<int64_t>(8 * n, (int64_t)1 << 21), 0x7fffffff);
    s.count = align16(kTileHdrInts * 4);
    s.off = s.count + align16((s.T + 1) * 4);
    s.recs = s.off + align16((s.T + 1) * 4);
    s.big = s.recs + n * (int64_t)sizeof(Rec);
    s.entries = s.big + align16(n * 4);
    s.total = s.entries + align16((int64_t)s.n_entries * 4);
    return s;
}

// record k covers the tiles of s: count it into each, or append it to the big list.  -> listed
template <class Rec>
WL_DEV bool tile_reserve(const TileBins<Rec>& b, int k, const TileSpan& s) {
    const int64_t nt = (int64_t)(s.tx1 - s.tx0 + 1) * (s.ty1 - s.ty0 + 1);
    bool listed = nt <= kMaxTilesPerRecord;
    if (listed) listed = atomicAdd(reinterpret_cast<unsigned long long*>(b.hdr + 2), (unsigned long long)nt) + nt <= (uint64_t)b.n_entries;
    if (listed) {
        for (int ty = s.ty0; ty <= s.ty1; ++ty)
            for (int tx = s.tx0; tx <= s.tx1; ++tx) atomicAdd(&b.count[ty * b.TX + tx], 1);
    } else {
        b.big[atomicAdd(&b.hdr[1], 1)] = k;
    }
    return listed;
}

// exclusive scan of count[0 .. T) into off[0 .. T] (off[T] = the total), 4096 counts per pass with the carry held in LDS; count is
// zeroed for the fill's cursors
__global__ void __launch_bounds__(kTileScan) tile_scan_kernel(int* __restrict__ count, int* __restrict__ off, const int64_t T) {
    __shared__ int wsum[kTileScan / 64];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < T; base += 4 * kTileScan) {
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
        if (threadIdx.x == kTileScan - 1) carry_s = before + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[T] = carry_s;
}

// hdr[0] is the live record count; n_max bounds the grid
template <class Rec>
__global__ void __launch_bounds__(kBlock) tile_fill_kernel(const TileBins<Rec> b, const int n_max) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_max || k >= b.hdr[0]) return;
    const TileSpan s = tile_span(b.recs[k]);
    if (!s.listed) return;
    for (int ty = s.ty0; ty <= s.ty1; ++ty)
        for (int tx = s.tx0; tx <= s.tx1; ++tx) {
            const int t = ty * b.TX + tx;
            b.entries[b.off[t] + atomicAdd(&b.count[t], 1)] = k;
        }
}

// visit(const Rec&) for every record of `tile`, staged through chunk[kTileLanes] in LDS.  EVERY lane of the workgroup (kTileLanes
// threads) must call it -- it holds barriers -- so a kernel retires its out-of-range lanes only afterwards.
template <class Rec, class Visit>
WL_DEV void for_each_tile_record(const TileBins<Rec>& b, int tile, Rec* chunk, Visit&& visit) {
    __shared__ int n_sel;
    // the tile's own list
    const int beg = b.off[tile], end = b.off[tile + 1];
    for (int c0 = beg; c0 < end; c0 += kTileLanes) {
        if (c0 + (int)threadIdx.x < end) chunk[threadIdx.x] = b.recs[b.entries[c0 + threadIdx.x]];
        __syncthreads();
        const int nc = min(kTileLanes, end - c0);
        for (int j = 0; j < nc; ++j) visit(chunk[j]);
        __syncthreads();
    }
    // the big list: every tile keeps the records whose rectangle holds it
    const int nb = b.hdr[1], tx = tile % b.TX, ty = tile / b.TX;
    for (int c0 = 0; c0 < nb; c0 += kTileLanes) {
        if (threadIdx.x == 0) n_sel = 0;
        __syncthreads();
        const int k = c0 + threadIdx.x;
        if (k < nb) {
            const Rec& r = b.recs[b.big[k]];
            const TileSpan s = tile_span(r);
            if (tx >= s.tx0 && tx <= s.tx1 && ty >= s.ty0 && ty <= s.ty1) chunk[atomicAdd(&n_sel, 1)] = r;
        }
        __syncthreads();
        const int nc = n_sel;
        for (int j = 0; j < nc; ++j) visit(chunk[j]);
        __syncthreads();
    }
}

// Clears the header and the counts, runs `bin` (the caller's launch of its bin kernel over its n inputs), then scan and fill: the
// lists are ready for the caller's consuming kernel on the same stream.  false: the memset was refused.
template <class Rec, class Bin>
inline bool tile_bins_build(const TileLayout& s, const TileBins<Rec>& b, int n, hipStream_t hs, Bin&& bin) {
    if (hipMemsetAsync(b.hdr, 0, (size_t)s.off, hs) != hipSuccess) return false;
    if (n > 0) bin();
    tile_scan_kernel<<<1, kTileScan, 0, hs>>>(b.count, b.off, s.T);
    if (n > 0) tile_fill_kernel<<<grid_for(n), kBlock, 0, hs>>>(b, n);
    return true;
}

}  // namespace

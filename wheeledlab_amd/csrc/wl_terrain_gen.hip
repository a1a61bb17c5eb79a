// wl_terrain_gen.hip -- procedural terrains (include/wheeledlab_amd_terrain.h): a grid of sub-terrains generated straight into the
// 16-bit height codes of a WlHeightField, so that a training run can draw a new terrain between two iterations without a host
// round trip (generation, upload, pair table and pyramid would otherwise sit in every iteration that resamples).
//
// Mapping: one lane per lattice point; a block is a 64 x 4 patch, a wavefront = 64 consecutive points of one row (one 128-byte
// segment of codes per store).  The work is closed-form per point (wl_terrain_gen_dev.h): a few integer divisions by wave-uniform
// divisors, at most four Philox blocks (interpolated noise) or one per rectangle (obstacles: <= 64, the same draws in every lane of
// a tile -- the tile is far wider than a wavefront, so they do not diverge), one descriptor read that the whole tile shares.  An
// 800 x 800 field is 2500 blocks and 1.28 MB of stores: the launch is latency-sized, not bandwidth-sized; nothing is staged.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_kernel_common.h"
#include "wl_terrain_gen_dev.h"

namespace {

constexpr int kPatchX = 64, kPatchY = kBlock / kPatchX;

__global__ void __launch_bounds__(kBlock) terrain_gen_kernel(const TerrainGrid g, const WlTerrainTile* __restrict__ tiles,
                                                             int16_t* __restrict__ codes, const int patches_x) {
    const int by = blockIdx.x / patches_x, bx = blockIdx.x - by * patches_x;
    const int i = bx * kPatchX + (int)(threadIdx.x & (kPatchX - 1)), j = by * kPatchY + (int)(threadIdx.x / kPatchX);
    if (i >= g.nx || j >= g.ny) return;
    codes[(int64_t)j * g.nx + i] = terrain_code(g, tiles, i, j);
}

bool params_ok(const WlTerrainGenParams* p) {
    if (!p) return false;
    if (p->nx < 2 || p->ny < 2 || p->nx >= WL_TERRAIN_MAX_SIDE || p->ny >= WL_TERRAIN_MAX_SIDE || (int64_t)p->nx * p->ny > 0x7fffffffLL)
        return false;
    if (p->tile_nx < 2 || p->tile_ny < 2 || p->border < 0 || p->rows < 1 || p->cols < 1) return false;
    if ((int64_t)p->rows * p->tile_nx + 2 * (int64_t)p->border != p->nx || (int64_t)p->cols * p->tile_ny + 2 * (int64_t)p->border != p->ny)
        return false;
    return p->base_code >= -32767 && p->base_code <= 32767;
}

bool level_range_ok(const WlTerrainTile& t) {   // code_lo + step_codes * k, k < n_levels, within +-WL_TERRAIN_MAX_OFFSET
    if (t.n_levels < 1 || t.n_levels > 65536) return false;
    const int64_t a = t.code_lo, b = (int64_t)t.code_lo + (int64_t)t.step_codes * (t.n_levels - 1);
    return a >= -WL_TERRAIN_MAX_OFFSET && a <= WL_TERRAIN_MAX_OFFSET && b >= -WL_TERRAIN_MAX_OFFSET && b <= WL_TERRAIN_MAX_OFFSET;
}

bool tile_ok(const WlTerrainGenParams* p, const WlTerrainTile& t) {
    const int side = p->tile_nx < p->tile_ny ? p->tile_nx : p->tile_ny, longest = p->tile_nx > p->tile_ny ? p->tile_nx : p->tile_ny;
    if (t.flags & ~WL_TF_INVERTED) return false;
    switch (t.type) {
        case WL_TT_RANDOM_UNIFORM: return t.step_cells >= 1 && t.step_cells <= longest && level_range_ok(t);
        case WL_TT_PYRAMID_SLOPED:
            return t.platform >= 0 && t.platform <= side && std::isfinite(t.slope) && std::fabs((double)t.slope) * side <= WL_TERRAIN_MAX_OFFSET;
        case WL_TT_PYRAMID_STAIRS:
            return t.platform >= 0 && t.platform <= side && t.step_cells >= 1 &&
                   std::llabs((int64_t)t.step_codes) * (side / t.step_cells + 1) <= WL_TERRAIN_MAX_OFFSET;
        case WL_TT_DISCRETE_OBSTACLES:
            return t.platform >= 0 && t.platform <= side && t.n_obstacles >= 0 && t.n_obstacles <= WL_TERRAIN_MAX_OBSTACLES && t.size_lo >= 1 &&
                   t.size_lo <= t.size_hi && t.size_hi <= side && level_range_ok(t);
        case WL_TT_WAVE:
            return t.num_waves >= 0 && (int64_t)t.num_waves * longest <= 0x3fffffffLL && std::isfinite(t.amplitude) &&
                   2.0 * std::fabs((double)t.amplitude) <= WL_TERRAIN_MAX_OFFSET;
        default: return false;
    }
}

}  // namespace

extern "C" {

int wl_terrain_gen_check(const WlTerrainGenParams* p, const WlTerrainTile* tiles_host) {
    if (!params_ok(p)) return WL_EINVAL;
    if (tiles_host)
        for (int64_t t = 0; t < (int64_t)p->rows * p->cols; ++t)
            if (!tile_ok(p, tiles_host[t])) return WL_EINVAL;
    return WL_OK;
}

int wl_terrain_generate(const WlTerrainGenParams* p, const WlTerrainTile* tiles, int16_t* codes_out, void* stream) {
    if (!params_ok(p) || !tiles || !codes_out) return WL_EINVAL;
    if (!aligned(tiles, 4) || !aligned(codes_out, 2)) return WL_EALIGN;
    const TerrainGrid g{p->nx, p->ny, p->tile_nx, p->tile_ny, p->border, p->rows, p->cols, p->base_code, (uint32_t)p->seed,
                        (uint32_t)(p->seed >> 32)};
    const int patches_x = (p->nx + kPatchX - 1) / kPatchX, patches_y = (p->ny + kPatchY - 1) / kPatchY;
    if ((int64_t)patches_x * patches_y > 0x7fffffffLL) return WL_EINVAL;
    clear_error();
    terrain_gen_kernel<<<(unsigned)(patches_x * patches_y), kBlock, 0, (hipStream_t)stream>>>(g, tiles, codes_out, patches_x);
    return launch_status();
}

}  // extern "C"

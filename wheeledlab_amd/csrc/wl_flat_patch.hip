// wl_flat_patch.hip -- flat patches (include/wheeledlab_amd_terrain.h): level ground found on the height lattice, on the device, so
// that a field redrawn in place (wl_terrain_generate) has its spawn points found again between two training iterations without the
// codes crossing the bus; and the deal that hands every env one of them as a virtual column of the terrain-levels tables.
//
// Mapping: one wavefront per slot (tile t, patch k), four slots per block.  A round tests 64 consecutive attempts, one per lane: a
// Philox block, then the disc about the drawn point (a few dozen 16-bit loads at car-sized radii, leaving at the first row that
// breaks a bound); the ballot's lowest set bit is the winner, so the result does not depend on which lane finished first.  The
// loop is bounded by ceil(max_tries / 64) rounds.  A grid of tiles gives a few hundred to a few thousand wavefronts reading a field
// that sits in L2: the launch is latency-sized like the generator's, and nothing is staged in LDS.  Lane 0 stores the slot's four
// words with ordinary vector stores.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/wheeledlab_amd.h"
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_kernel_common.h"
#include "wl_flat_patch_dev.h"

namespace {

constexpr int kWave = 64, kSlotsPerBlock = kBlock / kWave;

struct PatchPlace {
    float x0, y0, cell, z_scale;
};

__global__ void __launch_bounds__(kBlock) flat_patch_kernel(const PatchField f, const PatchPlace g, const PatchKey key,
                                                            const WlPatchTile* __restrict__ tiles, const int n_patches, const int n_slots,
                                                            float* __restrict__ xy_out, float* __restrict__ z_out, int32_t* __restrict__ tries_out) {
    const int slot = blockIdx.x * kSlotsPerBlock + (int)(threadIdx.x / kWave), lane = (int)(threadIdx.x & (kWave - 1));
    if (slot >= n_slots) return;      // (a whole wavefront leaves: nothing below synchronises across wavefronts)
    const int t = slot / n_patches, k = slot - t * n_patches;
    const WlPatchTile T = tiles[t];
    const PatchPoint p = fp_search<kWave>(f, T, key, (uint32_t)t, (uint32_t)k, lane);
    if (lane == 0) {
        xy_out[2 * (int64_t)slot] = fp_world(g.x0, p.i, g.cell);
        xy_out[2 * (int64_t)slot + 1] = fp_world(g.y0, p.j, g.cell);
        z_out[slot] = (float)f.codes[(int64_t)p.j * f.nx + p.i] * g.z_scale;
        tries_out[slot] = p.tries;
    }
}

__global__ void __launch_bounds__(kBlock) flat_patch_deal_kernel(const int n, const int env_offset, const int world_envs, const int cols,
                                                                 const int n_patches, const uint64_t epoch, const uint64_t seed,
                                                                 int32_t* __restrict__ type_out) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    type_out[e] = fp_deal((uint32_t)(env_offset + e), cols, world_envs, n_patches, epoch, seed);
}

bool field_ok(const WlHeightField* hf) {
    if (!hf || !hf->height) return false;
    if (hf->nx < 1 || hf->ny < 1 || (int64_t)hf->nx * hf->ny > 0x7fffffffLL) return false;
    return std::isfinite(hf->x0) && std::isfinite(hf->y0) && finite_pos(hf->cell) && finite_pos(hf->z_scale);
}

bool params_ok(const WlFlatPatchParams* p) {
    return p && p->n_tiles >= 1 && p->n_patches >= 1 && (int64_t)p->n_tiles * p->n_patches <= WL_PATCH_MAX_SLOTS && p->reserved == 0;
}

bool tile_ok(const WlHeightField* hf, const WlPatchTile& t) {
    if (t.i_lo > t.i_hi || t.j_lo > t.j_hi) return false;
    if (t.radius_cells < 0 || t.radius_cells > WL_PATCH_MAX_RADIUS) return false;
    if (t.radius2 < 0 || t.radius2 > t.radius_cells * t.radius_cells) return false;
    // every disc inside the lattice (int64: a window at the far end of int32 must not wrap into range)
    if ((int64_t)t.i_lo - t.radius_cells < 0 || (int64_t)t.i_hi + t.radius_cells > hf->nx - 1) return false;
    if ((int64_t)t.j_lo - t.radius_cells < 0 || (int64_t)t.j_hi + t.radius_cells > hf->ny - 1) return false;
    if (t.max_diff_codes < 0) return false;
    return t.max_tries >= 0 && t.max_tries <= WL_PATCH_MAX_TRIES;
}

}  // namespace

extern "C" {

int wl_flat_patch_check(const WlHeightField* hf, const WlFlatPatchParams* p, const WlPatchTile* tiles_host) {
    if (!field_ok(hf) || !params_ok(p)) return WL_EINVAL;
    if (!aligned(hf->height, 2) || !aligned(tiles_host, 4)) return WL_EALIGN;
    if (tiles_host)
        for (int t = 0; t < p->n_tiles; ++t)
            if (!tile_ok(hf, tiles_host[t])) return WL_EINVAL;
    return WL_OK;
}

int wl_flat_patches(const WlHeightField* hf, const WlFlatPatchParams* p, const WlPatchTile* tiles, float* xy_out, float* z_out,
                    int32_t* tries_out, void* stream) {
    if (!field_ok(hf) || !params_ok(p) || !tiles || !xy_out || !z_out || !tries_out) return WL_EINVAL;
    if (!aligned(hf->height, 2) || !aligned(tiles, 4) || !aligned(xy_out, 4) || !aligned(z_out, 4) || !aligned(tries_out, 4)) return WL_EALIGN;
    const int n_slots = p->n_tiles * p->n_patches;
    const PatchField f{hf->height, hf->nx, hf->ny};
    const PatchPlace g{hf->x0, hf->y0, hf->cell, hf->z_scale};
    const PatchKey key{p->stream, (uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
    clear_error();
    flat_patch_kernel<<<(unsigned)((n_slots + kSlotsPerBlock - 1) / kSlotsPerBlock), kBlock, 0, (hipStream_t)stream>>>(
        f, g, key, tiles, p->n_patches, n_slots, xy_out, z_out, tries_out);
    return launch_status();
}

int wl_flat_patch_deal(int32_t n_envs, int32_t env_offset, int32_t world_envs, int32_t cols, int32_t n_patches, uint64_t epoch,
                       uint64_t seed, int32_t* type_out, void* stream) {
    if (n_envs < 0 || env_offset < 0 || world_envs < 1 || (int64_t)env_offset + n_envs > world_envs) return WL_EINVAL;
    if (cols < 1 || n_patches < 1 || (int64_t)cols * n_patches > 0x40000000LL || !type_out) return WL_EINVAL;
    if (!aligned(type_out, 4)) return WL_EALIGN;
    if (n_envs == 0) return WL_OK;
    clear_error();
    flat_patch_deal_kernel<<<grid_for(n_envs), kBlock, 0, (hipStream_t)stream>>>(n_envs, env_offset, world_envs, cols, n_patches, epoch,
                                                                               seed, type_out);
    return launch_status();
}

}  // extern "C"

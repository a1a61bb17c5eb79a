/* wheeledlab_amd_terrain.h -- mesh terrains: rasterise a triangle mesh into a regular height lattice, the float heights from which a
 * WlHeightField's 16-bit codes are then made.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): a terrain is built once, before any step, and the step kernels
 * read only the codes.  Same conventions as that header: device pointers, `stream` a hipStream_t (NULL = the default stream),
 * return 0 (WL_OK) or a negative WL_E* code, arguments validated before any launch.
 *
 * Semantics.  Lattice point (i, j), 0 <= i < nx, 0 <= j < ny, lies at (x0 + i * cell, y0 + j * cell), evaluated in double from the
 * float parameters (the convention of WlHeightField: heights_out[j][i], world x = x0 + i * cell).  Its height is the LARGEST z, over
 * every triangle whose xy projection contains the point (closed: edges and vertices count), of that triangle's plane at the point;
 * fill_z where no triangle contains it -- what a ray cast straight down from above returns, overhangs collapsed to their top.
 *   - triangles of zero projected area (vertical walls) are skipped; both windings are accepted;
 *   - coverage is watertight: each edge function is evaluated in double with the edge's endpoints in one canonical (lexicographic
 *     x, y) order, so two triangles sharing an edge get exactly negated values on it and a point on the edge is covered by both;
 *   - a point that coincides with a vertex gets that vertex's z exactly;
 *   - a face with an index outside [0, n_vertices) or a non-finite vertex coordinate is skipped and counted in status_out[0].
 * The output is the same byte for byte from run to run (a maximum does not depend on the order the per-tile lists are filled in). */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_TERRAIN_VERSION 3
#define WL_TERRAIN_TILE 16               /* the raster pass fills 16 x 16-point tiles of the lattice, one workgroup each   */
#define WL_TERRAIN_MAX_TILES_PER_FACE 64 /* a face whose lattice rectangle spans more tiles goes to the big list every tile filters */
#define WL_TERRAIN_MAX_SIDE (1 << 23)    /* nx and ny: 2 .. WL_TERRAIN_MAX_SIDE - 1, nx * ny <= 2^31 - 1              */
#define WL_TERRAIN_STATUS_WORDS 4        /* status_out: [0] invalid faces, [1] faces binned (on the lattice, non-zero area),
                                            [2] faces on the big list, [3] per-tile list entries written                  */

typedef struct WlMeshRasterParams {
    float x0, y0;     /* world position of lattice point (0, 0)                                                          */
    float cell;       /* lattice spacing (> 0, finite)                                                                   */
    int32_t nx, ny;   /* lattice points in x and y                                                                      */
    float fill_z;     /* height where no triangle covers a point (finite)                                                */
} WlMeshRasterParams;

/* bytes of device scratch wl_mesh_raster needs for n_faces faces onto an nx x ny lattice; WL_EINVAL for sizes out of range */
int64_t wl_mesh_raster_scratch_bytes(int32_t n_faces, int32_t nx, int32_t ny);

/* Rasterise the mesh onto the lattice of `p`:
 *   vertices     float [n_vertices][3], world frame (x, y, z), metres (NULL allowed when n_vertices == 0)
 *   faces        int32 [n_faces][3], indices into vertices (NULL allowed when n_faces == 0)
 *   scratch      wl_mesh_raster_scratch_bytes(...) bytes of device memory, 16-byte aligned (WL_EALIGN otherwise)
 *   heights_out  float [ny][nx]
 *   status_out   int32 [WL_TERRAIN_STATUS_WORDS], written by the launch (read it after the stream has run it) */
int wl_mesh_raster(const WlMeshRasterParams* p, const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                   void* scratch, int64_t scratch_bytes, float* heights_out, int32_t* status_out, void* stream);

/* ---- procedural terrains: a grid of sub-terrains generated straight into 16-bit height codes (wl_terrain_gen.hip) -------------------
 *
 * The lattice is rows x cols tiles of tile_nx x tile_ny points inside a frame of `border` points: nx = rows * tile_nx + 2 * border,
 * ny = cols * tile_ny + 2 * border (rows advance along x: IsaacLab's difficulty axis; columns along y: its terrain types).  Point
 * (i, j) with (i - border, j - border) inside the grid belongs to tile t = r * cols + c, r = (i - border) / tile_nx, c = (j - border) /
 * tile_ny, at local (u, v) = (i - border - r * tile_nx, j - border - c * tile_ny); every other point is border and gets base_code.
 * codes_out[j][i] = clamp(base_code + off, -32767, 32767), `off` the tile's height in CODES at (u, v), by type (d = min(u, tile_nx -
 * 1 - u, v, tile_ny - 1 - v, d_plat), d_plat = max((min(tile_nx, tile_ny) - platform) / 2, 0): the ring distance from the tile's edge
 * up to the platform; sgn = -1 with WL_TF_INVERTED, else +1):
 *   WL_TT_RANDOM_UNIFORM    L(a, b) = code_lo + step_codes * (W(a, b) mod n_levels), W = word 0 of Philox(t, a, b, WL_TS_UNIFORM);
 *                           step_cells == 1: off = L(u, v); else with a = u / step_cells, fu = (float)(u mod step_cells) /
 *                           (float)step_cells (b, fv alike from v), bilinear in fp32: p = fma(fu, L(a+1, b) - L(a, b), L(a, b)),
 *                           q = the same on row b + 1, off = rint(fma(fv, q - p, p))
 *   WL_TT_PYRAMID_SLOPED    off = sgn * rint(slope * (float)d)                                  (slope: codes per cell, fp32)
 *   WL_TT_PYRAMID_STAIRS    off = sgn * step_codes * (d / step_cells)
 *   WL_TT_DISCRETE_OBSTACLES  rectangles k = 0 .. n_obstacles - 1 from X = Philox(t, k, 0, WL_TS_OBSTACLES): sides w = size_lo +
 *                           (X[0] & 0xffff) mod (size_hi - size_lo + 1), l alike from X[0] >> 16; corner pu = X[1] mod (tile_nx - w + 1),
 *                           pv = X[2] mod (tile_ny - l + 1); height code_lo + step_codes * (X[3] mod n_levels).  off = the height of
 *                           the LAST rectangle containing (u, v), 0 if none -- and 0 on the platform, the centred square of
 *                           `platform` points: (tile_nx - platform) / 2 <= u < (tile_nx - platform) / 2 + platform, v alike
 *   WL_TT_WAVE              off = rint(amplitude * (sinpi(xu) + cospi(xv))), xu = (float)(2 * ((num_waves * u) mod tile_nx)) /
 *                           (float)tile_nx, xv alike: num_waves whole periods across the tile   (amplitude: codes, fp32)
 * Philox(c0, c1, c2, c3) is the library's Philox4x32 (7 rounds) with key (seed low word, seed high word).  Every point is a
 * function of (i, j) and the arguments alone: the output is the same byte for byte from run to run. */
enum { WL_TT_RANDOM_UNIFORM = 0, WL_TT_PYRAMID_SLOPED = 1, WL_TT_PYRAMID_STAIRS = 2, WL_TT_DISCRETE_OBSTACLES = 3, WL_TT_WAVE = 4,
       WL_TT_COUNT = 5 };
#define WL_TF_INVERTED 1                 /* WlTerrainTile.flags: the pyramid descends (sloped, stairs)                      */
#define WL_TS_UNIFORM 11                 /* Philox stream ids (counter word 3)                                              */
#define WL_TS_OBSTACLES 12
#define WL_TERRAIN_MAX_OBSTACLES 64
#define WL_TERRAIN_MAX_OFFSET 32767      /* |code_lo|, |step_codes| * n_levels, |slope| * side, |amplitude| stay below this  */

typedef struct WlTerrainTile {
    int32_t type, flags;
    int32_t platform;      /* points: side of the flat square in the middle (sloped, stairs, obstacles); 0 .. min(tile_nx, tile_ny) */
    int32_t step_cells;    /* stairs: step width; uniform: spacing of the coarse grid (1 = a draw per point); >= 1                */
    int32_t step_codes;    /* stairs: step height; uniform / obstacles: spacing of the height levels                              */
    int32_t code_lo;       /* uniform / obstacles: the lowest level                                                               */
    int32_t n_levels;      /* uniform / obstacles: number of levels (>= 1)                                                        */
    int32_t n_obstacles;   /* obstacles: 0 .. WL_TERRAIN_MAX_OBSTACLES                                                            */
    int32_t size_lo, size_hi; /* obstacles: rectangle sides, points: 1 <= size_lo <= size_hi <= min(tile_nx, tile_ny)              */
    int32_t num_waves;     /* wave: periods across the tile (>= 0)                                                                */
    float slope;           /* sloped: codes per cell (finite)                                                                     */
    float amplitude;       /* wave: codes (finite)                                                                                */
    float difficulty;      /* what the host resolved the descriptor from, in [0, 1]: carried for the caller, never read by the kernel */
    int32_t pad[2];
} WlTerrainTile;           /* 64 bytes */

typedef struct WlTerrainGenParams {
    int32_t nx, ny;            /* lattice points: nx = rows * tile_nx + 2 * border, ny = cols * tile_ny + 2 * border              */
    int32_t tile_nx, tile_ny;  /* points per tile (>= 2)                                                                          */
    int32_t border;            /* points of base_code around the grid (>= 0)                                                      */
    int32_t rows, cols;        /* tiles along x and along y (>= 1)                                                                */
    int32_t base_code;         /* the code of flat ground (|base_code| <= 32767)                                                  */
    uint64_t seed;
} WlTerrainGenParams;

/* Validate the arguments as wl_terrain_generate does, without a launch and without reading device memory: `tiles_host` is a HOST
 * copy of the rows * cols descriptors (NULL: the descriptors are not checked).  WL_OK or WL_EINVAL. */
int wl_terrain_gen_check(const WlTerrainGenParams* p, const WlTerrainTile* tiles_host);

/* Generate the codes: `tiles` WlTerrainTile [rows * cols] and `codes_out` int16 [ny][nx], device pointers (4- and 2-byte aligned:
 * WL_EALIGN otherwise).  The parameters are validated before any launch (WL_EINVAL); the descriptors live in device memory, so the
 * caller validates them with wl_terrain_gen_check -- the kernel itself clamps what it reads from them (loop counts, divisors), so
 * that no descriptor can send it out of bounds.  Allocates nothing, keeps no state. */
int wl_terrain_generate(const WlTerrainGenParams* p, const WlTerrainTile* tiles, int16_t* codes_out, void* stream);

/* ---- flat patches: level ground found on the lattice, to spawn on (wl_flat_patch.hip) -------------------------------------------------
 *
 * For each of n_tiles windows of the lattice, n_patches lattice points whose neighbourhood is level -- IsaacLab's FlatPatchSamplingCfg /
 * TerrainImporter.flat_patches, searched on the device so that a field redrawn in place finds its patches again without a host
 * round trip.  All integers on the lattice: attempt a = 0, 1, ... of slot k of tile t draws X = Philox(t, k, a, params.stream) (the
 * library's Philox4x32, 7 rounds, key = the seed's words) and tests the point i = i_lo + hi32(X[0] * (i_hi - i_lo + 1)), j = j_lo +
 * hi32(X[1] * (j_hi - j_lo + 1)) (hi32: the high half of the 64-bit product).  It is ACCEPTED when, over the lattice points (i + di,
 * j + dj) with |di|, |dj| <= radius_cells and di^2 + dj^2 <= radius2 (indices clamped to the lattice), max code - min code <=
 * max_diff_codes, min code >= z_lo_code and max code <= z_hi_code.  A bilinear cell lies between its corners, so a disc of lattice
 * points that covers the metric disc bounds the surface inside it.  The slot takes the accepted attempt with the LOWEST index below
 * max_tries; with none it takes the window's centre ((i_lo + i_hi) / 2, (j_lo + j_hi) / 2) and is marked failed.  Outputs, for slot
 * s = t * n_patches + k: xy_out[s] = (x0 + fl(i * cell), y0 + fl(j * cell)) in fp32 (the product rounded before the sum), z_out[s] =
 * fl(code(i, j) * z_scale), tries_out[s] = the accepted attempt's index or -1.  One wavefront per slot tests 64 consecutive attempts
 * a round, at most ceil(max_tries / 64) rounds; plain stores, no atomics: the same bytes from run to run.
 *
 * The deal: wl_flat_patch_deal gives env e (global id gid = env_offset + e) the virtual column type_out[e] = (gid * cols / world_envs) *
 * n_patches + hi32(W * n_patches), W = word 0 of Philox(gid, epoch low, epoch high, WL_TS_PATCH_DEAL): with xy_out read as the origins
 * table [rows][cols * n_patches][2] of a WlTerrainLevels of cols * n_patches columns, the step kernels spawn about patches. */
#define WL_TS_PATCH 14                   /* Philox stream ids: the finder's default, and the deal's                          */
#define WL_TS_PATCH_DEAL 15
#define WL_PATCH_MAX_RADIUS 64           /* radius_cells                                                                      */
#define WL_PATCH_MAX_TRIES 65536         /* max_tries                                                                         */
#define WL_PATCH_MAX_SLOTS (1 << 22)     /* n_tiles * n_patches                                                               */

typedef struct WlPatchTile {
    int32_t i_lo, i_hi, j_lo, j_hi;  /* the inclusive lattice window of patch centres                                         */
    int32_t radius_cells;            /* the disc's bounding square: 0 .. WL_PATCH_MAX_RADIUS                                  */
    int32_t radius2;                 /* di^2 + dj^2 <= radius2: 0 .. radius_cells^2                                           */
    int32_t max_diff_codes;          /* largest max - min over the disc (>= 0)                                                */
    int32_t z_lo_code, z_hi_code;    /* every code of the disc within [z_lo_code, z_hi_code]                                  */
    int32_t max_tries;               /* 0 .. WL_PATCH_MAX_TRIES; 0: every slot takes the window's centre                      */
    int32_t pad[2];
} WlPatchTile;                       /* 48 bytes */

typedef struct WlFlatPatchParams {
    int32_t n_tiles, n_patches;      /* >= 1 each, n_tiles * n_patches <= WL_PATCH_MAX_SLOTS                                  */
    uint32_t stream;                 /* Philox stream id (counter word 3): WL_TS_PATCH unless the caller keeps several sets   */
    int32_t reserved;                /* 0                                                                                     */
    uint64_t seed;
} WlFlatPatchParams;                 /* 24 bytes */

/* Validate the arguments as wl_flat_patches does, without a launch and without reading device memory: `tiles_host` is a HOST copy of
 * the n_tiles descriptors (NULL: the descriptors are not checked).  WL_EINVAL: a field without codes or with sizes / placement out of
 * range, counts out of range, an empty window, a disc that leaves the lattice, radius_cells, radius2, max_diff_codes or max_tries out
 * of range.  WL_EALIGN: hf->height not 2-byte or tiles_host not 4-byte aligned. */
int wl_flat_patch_check(const WlHeightField* hf, const WlFlatPatchParams* p, const WlPatchTile* tiles_host);

/* Find the patches: `tiles` WlPatchTile [n_tiles], xy_out float [n_tiles][n_patches][2], z_out float [n_tiles][n_patches], tries_out
 * int32 [n_tiles][n_patches], device pointers, 4-byte aligned (WL_EALIGN otherwise; NULL: WL_EINVAL).  The field and the parameters are
 * validated before the launch and nothing is launched on a refusal; the descriptors live in device memory, so the caller validates
 * them with wl_flat_patch_check -- the kernel clamps what it reads from them (window, radius, tries, every index).  Allocates
 * nothing, keeps no state. */
int wl_flat_patches(const WlHeightField* hf, const WlFlatPatchParams* p, const WlPatchTile* tiles, float* xy_out, float* z_out,
                    int32_t* tries_out, void* stream);

/* Deal every env a slot: type_out int32 [n_envs] (device, 4-byte aligned).  n_envs >= 0, env_offset >= 0, env_offset + n_envs <=
 * world_envs, cols >= 1, n_patches >= 1, cols * n_patches <= 2^30 (WL_EINVAL otherwise; nothing is launched on a refusal). */
int wl_flat_patch_deal(int32_t n_envs, int32_t env_offset, int32_t world_envs, int32_t cols, int32_t n_patches, uint64_t epoch,
                       uint64_t seed, int32_t* type_out, void* stream);

/* WL_TERRAIN_VERSION of the library */
int wl_terrain_version(void);

#ifdef __cplusplus
}
#endif

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

#define WL_TERRAIN_VERSION 1
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

/* WL_TERRAIN_VERSION of the library */
int wl_terrain_version(void);

#ifdef __cplusplus
}
#endif

// TEST INFRASTRUCTURE ONLY: the procedural-terrain generator's device functions (wheeledlab_amd/csrc/wl_terrain_gen_dev.h: one
// lattice point's code from the grid and its tile's descriptor) compiled for the host through the stand-in hip_runtime.h and walked
// over every point, so that tests/test_terrain_gen_host_sim_cpu.py can hold them against the float64 restatement
// (tests/terrain_gen_reference.py) without a GPU.  Built by the test into a scratch directory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "wl_terrain_gen_dev.h"

extern "C" {
// tiles [rows * cols], codes [ny][nx]; the caller has validated the arguments
int hs_terrain_generate(const WlTerrainGenParams* p, const WlTerrainTile* tiles, int16_t* codes) {
    const TerrainGrid g{p->nx, p->ny, p->tile_nx, p->tile_ny, p->border, p->rows, p->cols, p->base_code, (uint32_t)p->seed,
                        (uint32_t)(p->seed >> 32)};
    for (int j = 0; j < g.ny; ++j)
        for (int i = 0; i < g.nx; ++i) codes[(size_t)j * g.nx + i] = terrain_code(g, tiles, i, j);
    return 0;
}
}

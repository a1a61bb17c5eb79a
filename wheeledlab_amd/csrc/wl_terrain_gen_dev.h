// wl_terrain_gen_dev.h -- procedural terrains (include/wheeledlab_amd_terrain.h): the height code of ONE lattice point of a grid of
// sub-terrains, as a function of the point's indices, the grid and its tile's descriptor alone -- no other lane, no memory but the
// descriptor.  Device functions only (wl_terrain_gen.hip maps points to lanes; tests/host_sim/terrain_gen_host.cpp compiles this
// header for the host and walks every point against the float64 restatement, tests/terrain_gen_reference.py).
//
// Integer wherever the quantity is one: lengths in points, discrete heights in codes, the draws.  The three continuous forms (slope,
// wave, interpolated noise) evaluate in fp32 with every fused multiply-add written out, so that the build's contraction setting
// cannot choose a rounding sequence, and round once to a code (rintf: half to even).
#pragma once
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_rng.h"

struct TerrainGrid {
    int nx, ny, tile_nx, tile_ny, border, rows, cols, base_code;
    uint32_t k0, k1;   // the Philox key: the seed's words
};

#ifdef WL_HOST_SIM
WL_DEV float tg_sinpi(float x) { return (float)std::sin(3.14159265358979323846 * (double)x); }
WL_DEV float tg_cospi(float x) { return (float)std::cos(3.14159265358979323846 * (double)x); }
#else
WL_DEV float tg_sinpi(float x) { return sinpif(x); }   // the device library's: 1 ulp in its documentation (arguments in [0, 2) here)
WL_DEV float tg_cospi(float x) { return cospif(x); }
#endif

WL_DEV int tg_min(int a, int b) { return a < b ? a : b; }
WL_DEV int tg_max(int a, int b) { return a > b ? a : b; }
WL_DEV int tg_clamp(int v, int lo, int hi) { return tg_min(tg_max(v, lo), hi); }
// a float height in codes -> its code offset: clamped first, so that the conversion is defined whatever the descriptor held
WL_DEV int tg_round(float h) { return (int)rintf(fminf(fmaxf(h, -65534.f), 65534.f)); }
// (unsigned arithmetic: a descriptor the caller did not validate may overflow it, which then wraps instead of being undefined)
WL_DEV int tg_level(int lo, int step, uint32_t k) { return (int)((uint32_t)lo + (uint32_t)step * k); }

// ring distance from the tile's edge, flat from the platform inwards
WL_DEV int tg_ring(const TerrainGrid& g, int platform, int u, int v) {
    const int side = tg_min(g.tile_nx, g.tile_ny);
    const int d_plat = tg_max((side - tg_clamp(platform, 0, side)) / 2, 0);
    return tg_min(tg_min(tg_min(u, g.tile_nx - 1 - u), tg_min(v, g.tile_ny - 1 - v)), d_plat);
}

WL_DEV int tg_uniform(const TerrainGrid& g, const WlTerrainTile& T, uint32_t t, int u, int v) {
    const uint32_t n = (uint32_t)tg_max(T.n_levels, 1);
    auto level = [&](int a, int b) {
        return tg_level(T.code_lo, T.step_codes, philox4x32(t, (uint32_t)a, (uint32_t)b, WL_TS_UNIFORM, g.k0, g.k1).x % n);
    };
    const int D = tg_max(T.step_cells, 1);
    if (D == 1) return level(u, v);
    const int a = u / D, b = v / D;
    const float fu = (float)(u - a * D) / (float)D, fv = (float)(v - b * D) / (float)D;
    const int l00 = level(a, b), l10 = level(a + 1, b), l01 = level(a, b + 1), l11 = level(a + 1, b + 1);
    const float p = fmaf(fu, (float)(l10 - l00), (float)l00), q = fmaf(fu, (float)(l11 - l01), (float)l01);
    return tg_round(fmaf(fv, q - p, p));
}

WL_DEV int tg_obstacles(const TerrainGrid& g, const WlTerrainTile& T, uint32_t t, int u, int v) {
    const int side = tg_min(g.tile_nx, g.tile_ny);
    const int plat = tg_clamp(T.platform, 0, side);
    const int pu0 = (g.tile_nx - plat) / 2, pv0 = (g.tile_ny - plat) / 2;
    if (u >= pu0 && u < pu0 + plat && v >= pv0 && v < pv0 + plat) return 0;
    const int lo = tg_clamp(T.size_lo, 1, side), hi = tg_clamp(T.size_hi, lo, side);
    const uint32_t span = (uint32_t)(hi - lo + 1), n = (uint32_t)tg_max(T.n_levels, 1);
    const int count = tg_clamp(T.n_obstacles, 0, WL_TERRAIN_MAX_OBSTACLES);
    int off = 0;
    for (int k = 0; k < count; ++k) {
        const U4 x = philox4x32(t, (uint32_t)k, 0u, WL_TS_OBSTACLES, g.k0, g.k1);
        const int w = lo + (int)((x.x & 0xffffu) % span), l = lo + (int)((x.x >> 16) % span);
        const int pu = (int)(x.y % (uint32_t)(g.tile_nx - w + 1)), pv = (int)(x.z % (uint32_t)(g.tile_ny - l + 1));
        if (u >= pu && u < pu + w && v >= pv && v < pv + l) off = tg_level(T.code_lo, T.step_codes, x.w % n);
    }
    return off;
}

WL_DEV int tg_wave(const TerrainGrid& g, const WlTerrainTile& T, int u, int v) {
    const uint32_t nw = (uint32_t)tg_max(T.num_waves, 0);
    const uint32_t mu = (nw * (uint32_t)u) % (uint32_t)g.tile_nx, mv = (nw * (uint32_t)v) % (uint32_t)g.tile_ny;
    const float xu = (float)(2u * mu) / (float)g.tile_nx, xv = (float)(2u * mv) / (float)g.tile_ny;
    return tg_round(T.amplitude * (tg_sinpi(xu) + tg_cospi(xv)));
}

// the tile's height at its local point (u, v), in codes above the base
WL_DEV int terrain_tile_offset(const TerrainGrid& g, const WlTerrainTile& T, uint32_t t, int u, int v) {
    const int sgn = (T.flags & WL_TF_INVERTED) ? -1 : 1;
    switch (T.type) {
        case WL_TT_RANDOM_UNIFORM: return tg_uniform(g, T, t, u, v);
        case WL_TT_PYRAMID_SLOPED: return sgn * tg_round(T.slope * (float)tg_ring(g, T.platform, u, v));
        case WL_TT_PYRAMID_STAIRS: return sgn * tg_level(0, T.step_codes, (uint32_t)(tg_ring(g, T.platform, u, v) / tg_max(T.step_cells, 1)));
        case WL_TT_DISCRETE_OBSTACLES: return tg_obstacles(g, T, t, u, v);
        case WL_TT_WAVE: return tg_wave(g, T, u, v);
        default: return 0;
    }
}

// the code of lattice point (i, j), 0 <= i < nx, 0 <= j < ny
WL_DEV int16_t terrain_code(const TerrainGrid& g, const WlTerrainTile* __restrict__ tiles, int i, int j) {
    const int gi = i - g.border, gj = j - g.border;
    int off = 0;
    if (gi >= 0 && gj >= 0 && gi < g.rows * g.tile_nx && gj < g.cols * g.tile_ny) {
        const int r = gi / g.tile_nx, c = gj / g.tile_ny;
        const uint32_t t = (uint32_t)(r * g.cols + c);
        const WlTerrainTile T = tiles[t];
        off = tg_clamp(terrain_tile_offset(g, T, t, gi - r * g.tile_nx, gj - c * g.tile_ny), -65534, 65534);
    }
    return (int16_t)tg_clamp(g.base_code + off, -32767, 32767);
}

// wl_flat_patch_dev.h -- flat patches (include/wheeledlab_amd_terrain.h): the search of ONE slot of one tile for a lattice point whose
// disc of neighbours is level, as a function of the codes, the tile's descriptor and the launch's key alone.  Device functions only
// (wl_flat_patch.hip maps slots to wavefronts; tests/host_sim/flat_patch_host.cpp compiles this header for the host, a wavefront of
// one lane, and tests/test_flat_patch_host_sim_cpu.py holds it against the integer restatement, tests/flat_patch_reference.py).
//
// Everything up to the result is an integer on the height lattice: the draw (the high half of word * span), the disc (di^2 + dj^2 <=
// radius2), the codes.  The three floats of a result are one rounding each: x = x0 + fl(i * cell) with the product kept out of
// contraction (fp_world), z = fl(code * z_scale).
#pragma once
#include "../../include/wheeledlab_amd_terrain.h"
#include "wl_rng.h"

struct PatchField {
    const int16_t* codes;   // [ny][nx]
    int nx, ny;
};
struct PatchKey {
    uint32_t stream, k0, k1;   // the Philox stream id and the seed's words
};
struct PatchPoint {
    int i, j;
    int tries;   // the accepted attempt's index, -1: none (the point is the window's centre)
};

WL_DEV int fp_min(int a, int b) { return a < b ? a : b; }
WL_DEV int fp_max(int a, int b) { return a > b ? a : b; }
WL_DEV int fp_clamp(int v, int lo, int hi) { return fp_min(fp_max(v, lo), hi); }
WL_DEV uint32_t fp_below(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * n) >> 32); }   // [0, n): what __umulhi gives

// The window as the search uses it: clamped to the lattice and non-empty whatever the descriptor held.
struct PatchWindow {
    int i_lo, j_lo;
    uint32_t ni, nj;
};
WL_DEV PatchWindow fp_window(const PatchField& f, const WlPatchTile& T) {
    const int i_lo = fp_clamp(T.i_lo, 0, f.nx - 1), j_lo = fp_clamp(T.j_lo, 0, f.ny - 1);
    const int i_hi = fp_clamp(T.i_hi, i_lo, f.nx - 1), j_hi = fp_clamp(T.j_hi, j_lo, f.ny - 1);
    return PatchWindow{i_lo, j_lo, (uint32_t)(i_hi - i_lo + 1), (uint32_t)(j_hi - j_lo + 1)};
}

// attempt a of slot k of tile t: the centre it tests
WL_DEV void fp_draw(const PatchWindow& w, const PatchKey& key, uint32_t t, uint32_t k, uint32_t a, int& i, int& j) {
    const U4 x = philox4x32(t, k, a, key.stream, key.k0, key.k1);
    i = w.i_lo + (int)fp_below(x.x, w.ni);
    j = w.j_lo + (int)fp_below(x.y, w.nj);
}

// is the disc about (i, j) level?  Indices clamped to the lattice; leaves as soon as the spread or a bound is broken.
WL_DEV bool fp_flat(const PatchField& f, const WlPatchTile& T, int i, int j) {
    const int rc = fp_clamp(T.radius_cells, 0, WL_PATCH_MAX_RADIUS);
    int lo = 32767, hi = -32768;
    for (int dj = -rc; dj <= rc; ++dj) {
        const int16_t* row = f.codes + (int64_t)fp_clamp(j + dj, 0, f.ny - 1) * f.nx;
        for (int di = -rc; di <= rc; ++di) {
            if (di * di + dj * dj > T.radius2) continue;
            const int c = row[fp_clamp(i + di, 0, f.nx - 1)];
            lo = fp_min(lo, c);
            hi = fp_max(hi, c);
        }
        if (hi - lo > T.max_diff_codes || lo < T.z_lo_code || hi > T.z_hi_code) return false;
    }
    return hi >= lo;   // (a negative radius2 holds no point, not even the centre: nothing to accept)
}

// The slot's search by a wavefront of LANES lanes (`lane` this one's index): rounds of LANES consecutive attempts, one per lane; the
// lowest accepted attempt of the first round that has one wins.  At most ceil(max_tries / LANES) rounds.  Every lane returns the
// same point.
template <int LANES>
WL_DEV PatchPoint fp_search(const PatchField& f, const WlPatchTile& T, const PatchKey& key, uint32_t t, uint32_t k, int lane) {
    const PatchWindow w = fp_window(f, T);
    const int tries = fp_clamp(T.max_tries, 0, WL_PATCH_MAX_TRIES);
    for (int base = 0; base < tries; base += LANES) {
        const int a = base + lane;
        bool ok = false;
        if (a < tries) {
            int i, j;
            fp_draw(w, key, t, k, (uint32_t)a, i, j);
            ok = fp_flat(f, T, i, j);
        }
        const unsigned long long found = __builtin_amdgcn_ballot_w64(ok);
        if (found) {
            PatchPoint p;
            p.tries = base + __builtin_ctzll(found);
            fp_draw(w, key, t, k, (uint32_t)p.tries, p.i, p.j);
            return p;
        }
    }
    return PatchPoint{w.i_lo + (int)(w.ni - 1) / 2, w.j_lo + (int)(w.nj - 1) / 2, -1};
}

// world coordinate of lattice index i: the product rounded to fp32, then the sum -- never one fused operation.  The build contracts
// a * b + c wherever it sees one (-ffp-contract=fast does not honour a pragma), so the product is formed where no contraction can reach
// it: in double it is exact (an index below 2^23 times a 24-bit significand), and its conversion IS the fp32 rounding of i * cell.
WL_DEV float fp_world(float origin, int i, float cell) {
    const float d = (float)((double)i * (double)cell);
    return origin + d;
}

// the slot a global env id is dealt in epoch `epoch`: its tile column's block of P virtual columns, and one of the P in it
WL_DEV int fp_deal(uint32_t gid, int cols, int world_envs, int n_patches, uint64_t epoch, uint64_t seed) {
    const int col = (int)((int64_t)gid * cols / world_envs);
    return col * n_patches + (int)fp_below(philox_block(gid, epoch, WL_TS_PATCH_DEAL, seed).x, (uint32_t)n_patches);
}

// wl_elev_scan_dev.h -- device code of the elevation task's height scan (world_height_map): an env's lattice frame, a ray's cell,
// gather and value, and four rays as one 16-byte word: what every scan form of wl_elev.hip evaluates.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wheeledlab_amd.h"
#include "wl_kernel_common.h"
#include "wl_heightfield.h"

namespace {

// what the height scan needs of an env after its step: root position and the cos / sin of its yaw
struct ScanPose {
    float px, py, pz, c, s;
};

// ---- world_height_map (:44-48): the 26 x 26 yaw-aligned height scan -- what every form below evaluates per ray ------------------
// The rays of one env form a lattice; in GRID units (cells of the heightfield) ray (ix, iy) stands at
// (u0 + ix ux + iy uy, v0 + ix vx + iy vy).  Round 4: the lattice frame is set up once per env (7 floats, what the fused kernels
// keep in LDS) and a ray costs ~35 VALU instructions instead of ~62 (the ray's metres -> rotate -> translate -> grid units chain,
// four float compares for the inside test and 64-bit address arithmetic went; the scan was as much instruction- as gather-bound:
// 676 rays x 62 / 64 lanes = 655 wavefront-instructions per env against ~1100 clocks per env and CU).  Same definition
// (oracle/elev_step.py::height_map, heightfield.py::sample with guard=False); fp32 rounding of the ray position differs by a few ulp
// of the grid coordinate from the metre chain (tests/heightfield_reference.py derives the bound).  The scan has NO far-border guard:
// the contact samplers clamp u, v to n - 1 - 1e-3 (wl_heightfield.h), the scan samples the ray's own cell -- on a border that slopes
// the two differ by up to 1e-3 cell x the slope (1e-4 m at 0.1 m cells and a slope of 1), beyond the scan's 2e-5 m, so the scan's
// definition is the guard-free one (tests/test_gpu_heightfield_geometry.py holds every scan form to it).
struct ScanFrame {
    float u0, v0, ux, vx, uy, vy, pz;
};
WL_DEV ScanFrame scan_frame(const WlElevParams& p, const HeightFieldGround& g, const ScanPose& sp) {
    const float g0 = -0.5f * p.scan_size, k = p.scan_res * g.inv_cell;
    ScanFrame f;
    // (multiply-adds spelled out: see yaw_cs)
    f.u0 = ((sp.px + fmaf(sp.c, g0, -(sp.s * g0))) - g.f.x0) * g.inv_cell;
    f.v0 = ((sp.py + fmaf(sp.s, g0, sp.c * g0)) - g.f.y0) * g.inv_cell;
    f.ux = sp.c * k, f.vx = sp.s * k;
    f.uy = -sp.s * k, f.vy = sp.c * k;
    f.pz = sp.pz;
    return f;
}
// ray index r (< 1024) of the scan -> lattice coordinates, meshgrid "xy": x fastest (r / 26 by multiply-shift: exact, checked)
WL_DEV void scan_ray_xy(int r, float& fix, float& fiy) {
    const int iy = (int)(__umul24((unsigned)r, 1261u) >> 15);
    fix = (float)(r - iy * WL_ELEV_SCAN_N);
    fiy = (float)iy;
}
// the cell a ray falls into: float offset of its lower-left grid point, position inside the cell, inside-the-field flag
struct ScanCell {
    int i, j;      // NOT clamped: outside the field when !inside
    float fu, fv;
    bool inside;
};
WL_DEV ScanCell scan_cell(const ScanFrame& f, const WlHeightField& hf, float fix, float fiy) {
    const float u = fmaf(fix, f.ux, fmaf(fiy, f.uy, f.u0)), v = fmaf(fix, f.vx, fmaf(fiy, f.vy, f.v0));
    const float fl_u = floorf(u), fl_v = floorf(v);
    const int i = (int)fl_u, j = (int)fl_v;      // saturating conversion: far-away rays stay far away
    ScanCell c;
    c.fu = u - fl_u;
    c.fv = v - fl_v;
    // 0 <= u < nx - 1 as ONE unsigned compare per axis; a NaN pose (converted to cell 0) is caught through its NaN fraction
    c.inside = (unsigned)i < (unsigned)(hf.nx - 1) && (unsigned)j < (unsigned)(hf.ny - 1) && (c.fu + c.fv >= 0.f);
    c.i = i, c.j = j;
    return c;
}
// a ray in flight: the gather of its cell's four corner codes, decoded and consumed by scan_value.
// Round 6: ONE 8-byte gather from the row-pair table (WlHeightField.pair): lo = (c00 | c01 << 16), hi = (c10 | c11 << 16).  The
// gathers were bound by the texture unit's address rate -- rocprofv3 on the fused launch at 4096 envs: TA busy 16 000 cycles per CU
// = the whole scan phase, 57 cache accesses per 64-lane gather instruction, L1 hit rate 0.91 -- and a ray cost two of them (rows j
// and j + 1 of the code field); with the pair table it costs one (measured: fused step 20.5 -> 17.5 us, gather-form scan at 262 144
// envs 484 -> 319 us).
struct ScanRay {
    uint32_t lo, hi;
    float fu, fv;
    bool inside;
};
struct ScanField {   // the row-pair table through a buffer resource: one 32-bit lane offset per gather
    __amdgpu_buffer_rsrc_t rsrc;
    float z_scale;
};
WL_DEV ScanField scan_field(const WlHeightField& hf) {
    return ScanField{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(hf.pair), 0, hf.nx * hf.ny * 4, 0x00020000), hf.z_scale};
}
WL_DEV ScanRay scan_request(const ScanFrame& f, const WlHeightField& hf, const ScanField& sf, float fix, float fiy) {
    typedef unsigned wl_u2 __attribute__((ext_vector_type(2)));
    const ScanCell c = scan_cell(f, hf, fix, fiy);
    ScanRay r;
    r.fu = c.fu, r.fv = c.fv, r.inside = c.inside;
    // a ray outside the field asks for whatever address its cell index wraps to: inside the buffer it reads a value nobody uses
    // (the ray is a miss), outside it the resource's bounds check returns 0 -- four clamps per ray saved.  24-bit multiply (full
    // rate; v_mul_lo_u32 is a quarter-rate instruction): exact for every ray inside the field (heightfield_args_ok: nx, ny < 2^23)
    const wl_u2 w = __builtin_amdgcn_raw_buffer_load_b64(sf.rsrc, (__mul24(c.j, hf.nx) + c.i) * 4, 0, 0);
    r.lo = w.x, r.hi = w.y;
    return r;
}
// FOUR consecutive rays per lane, stored as ONE 16-byte word (round 4).  The scan's 676 four-byte stores per env were what bound
// it, whatever the read side did (gathers or an LDS patch, DESIGN.md section 7: 500 us per launch at 262 144 envs either way): a store
// instruction costs the memory pipeline per INSTRUCTION far more than per byte (MI355X_MICROARCH.md: narrow stores are issue-bound,
// a dword store ~6 x a dwordx4 store per byte).  Rays 4 q .. 4 q + 3 of an env (q < 169) are neighbours along x; the scan row has 26
// = 6.5 quads, so a quad starting at ix = 24 continues at (0, iy + 1): ray pairs (0, 1) and (2, 3) never straddle a row.
typedef float wl_float4_u __attribute__((ext_vector_type(4), aligned(4)));   // observation rows are only 4-byte aligned
constexpr int kScanQuads = WL_ELEV_SCAN_N * WL_ELEV_SCAN_N / 4;             // 169
static_assert(WL_ELEV_SCAN_N % 2 == 0 && (WL_ELEV_SCAN_N * WL_ELEV_SCAN_N) % 4 == 0, "ray pairs stay inside a scan row, whole quads per env");
// quad slot (env-in-block x 169 + quad, < 2^13) -> env j, quad q (idx / 169 by multiply-shift: exact, checked)
WL_DEV void scan_quad_slot(int idx, int& j, int& q) {
    j = (int)(__umul24((unsigned)idx, 6205u) >> 20);
    q = idx - j * kScanQuads;
}
// bilinear height under the ray -> the observation value: -(sensor_z - hit_z - offset) + (root_z - plane_init_value), +inf on a
// miss, clipped to +- obs_clip
WL_DEV float scan_value(const WlElevParams& p, const ScanRay& r, float z_scale, float pz) {
    // the blend runs on the CODES and is scaled once (3 instructions per ray fewer than decoding the four corners first; the large-batch
    // scan is VALU-bound since round 5).  Exactly the decode-first value when z_scale is a power of two (terrain.py's default: scaling
    // by 2^k commutes with every rounding); for other scales it differs from it in the last bit -- every scan form shares this function
    const float c00 = (float)(int)(int16_t)(r.lo & 0xffffu), c01 = (float)((int)r.lo >> 16);
    const float c10 = (float)(int)(int16_t)(r.hi & 0xffffu), c11 = (float)((int)r.hi >> 16);
    const float a = fmaf(r.fu, c10 - c00, c00), b = fmaf(r.fu, c11 - c01, c01);
    float hz;
    {
#pragma clang fp contract(off)
        hz = fmaf(r.fv, b - a, a) * z_scale;      // a multiply of its own: not fused into the subtraction below per inlining site
    }
    const float val = r.inside ? (-(pz - hz - p.scan_offset) + (pz - p.elev_z0)) : __builtin_inff();
    return clampf(val, -p.obs_clip, p.obs_clip);
}
// the gathers of the four rays of quad q (4 x 8 B in flight per lane) ...
WL_DEV void scan_quad_request(const ScanFrame& f, const WlHeightField& hf, const ScanField& sf, int q, ScanRay (&r)[4]) {
    float fx0, fy0, fx2, fy2;
    scan_ray_xy(4 * q, fx0, fy0);
    scan_ray_xy(4 * q + 2, fx2, fy2);
    r[0] = scan_request(f, hf, sf, fx0, fy0);
    r[1] = scan_request(f, hf, sf, fx0 + 1.f, fy0);
    r[2] = scan_request(f, hf, sf, fx2, fy2);
    r[3] = scan_request(f, hf, sf, fx2 + 1.f, fy2);
}
// ... and their four values as one 16-byte word
WL_DEV wl_float4_u scan_quad_value(const WlElevParams& p, const ScanRay (&r)[4], float z_scale, float pz) {
    wl_float4_u v;
    v.x = scan_value(p, r[0], z_scale, pz), v.y = scan_value(p, r[1], z_scale, pz), v.z = scan_value(p, r[2], z_scale, pz);
    v.w = scan_value(p, r[3], z_scale, pz);
    return v;
}
#ifndef WL_FUSED_SCAN_NT
#define WL_FUSED_SCAN_NT true     // the fused step + scan launches' map rows as non-temporal stores (round 4, 4096 envs: 25.6 -> 24.7 us per step)
#endif
template <bool STREAM>
WL_DEV void scan_quad_store(float* __restrict__ row_map /* obs row + 13 */, int q, wl_float4_u v) {
    wl_float4_u* dst = reinterpret_cast<wl_float4_u*>(row_map + 4 * q);

    if constexpr (STREAM) __builtin_nontemporal_store(v, dst);
    else *dst = v;
}

}  // namespace

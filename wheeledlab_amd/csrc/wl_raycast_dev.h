// wl_raycast_dev.h -- the ray caster's device functions: the sensor frame of one env, the world ray of one table entry, the walked
// ray and the column sample (see wl_raycast.hip).  A header of its own so that tests/host_sim can compile them for the host and hold
// them against oracle/depth.c.  The walk (wl_depth_dev.h::cast_ray) and the bilinear sampler (wl_heightfield.h::HeightFieldGround)
// are included, not restated.
#pragma once
#include "../../include/wheeledlab_amd_raycaster.h"
#include "wl_depth_dev.h"

namespace {

// the sensor of one env: origin and the rotation sensor -> world (rows)
struct SensorFrame {
    V3 o;
    Mat3 M;
};

WL_DEV Mat3 mat_mul(const Mat3& a, const Mat3& b) {      // a b, row by row: row i of a b = a_i0 b.r0 + a_i1 b.r1 + a_i2 b.r2
    const auto row = [&](V3 r) { return fma3(r.x, b.r0, fma3(r.y, b.r1, r.z * b.r2)); };
    return Mat3{row(a.r0), row(a.r1), row(a.r2)};
}

// the body's rotation, or with yaw_only its yaw alone: the heading of the body's x axis in the world xy plane (IsaacLab's yaw_quat
// keeps the same angle, atan2(2 (w z + x y), 1 - 2 (y^2 + z^2))); a body pointing straight up or down keeps heading 0
WL_DEV Mat3 sensor_body_rotation(Quat q, bool yaw_only) {
    if (!yaw_only) return mat_from_quat(q);
    const float ca = 1.f - 2.f * (q.y * q.y + q.z * q.z), sa = 2.f * (q.w * q.z + q.x * q.y);
    const float n2 = ca * ca + sa * sa;
    const float inv = n2 > 0.f ? rsq(n2) : 0.f;
    const float c = n2 > 0.f ? ca * inv : 1.f, s = sa * inv;
    return Mat3{v3(c, -s, 0.f), v3(s, c, 0.f), v3(0.f, 0.f, 1.f)};
}

// the sensor of a root at `pos` with orientation `q`; `mount`: the mount rotation (offset_quat, unit).  R = the body's rotation, its
// yaw or the identity by p.alignment: origin pos + R offset_pos, rotation R mount
WL_DEV SensorFrame raycast_frame(const WlRayCastParams& p, const Mat3& mount, V3 pos, Quat q) {
    const Mat3 R = p.alignment == WL_RAYCAST_ALIGN_WORLD ? Mat3{v3(1.f, 0.f, 0.f), v3(0.f, 1.f, 0.f), v3(0.f, 0.f, 1.f)}
                                                         : sensor_body_rotation(q, p.alignment == WL_RAYCAST_ALIGN_YAW);
    return SensorFrame{pos + mul(R, v3(p.offset_pos[0], p.offset_pos[1], p.offset_pos[2])), mat_mul(R, mount)};
}

// what one ray reports: its parameter clipped at max_distance and its hit point (+inf on a miss: nothing closer than max_distance)
struct RayCastHit {
    float t;
    V3 hit;
};
WL_DEV RayCastHit raycast_miss_or(float t, float tmax, V3 at) {
    const bool miss = !(t < tmax);
    return RayCastHit{miss ? tmax : t, miss ? v3(INFINITY, INFINITY, INFINITY) : at};
}

// the general form: table entry (start, dir) in the sensor frame -> the world ray, walked through the bound pyramid.  cast_ray with a
// unit direction returns the Euclidean distance of the first hit (tmax on a miss, 0 from under the terrain)
WL_DEV RayCastHit raycast_walk(const DepthGrid& g, const Pyramid& py, const PyrHead& hd, const FieldMem& mem, const SensorFrame& s, V3 start,
                               V3 dir, float tmax) {
    const V3 o = s.o + mul(s.M, start), d = mul(s.M, dir);
    const float t = cast_ray(g, py, hd, mem, o, d, tmax);
    return raycast_miss_or(t, tmax, fma3(t, d, o));
}

// the terrain solid's height over (x, y): HeightFieldGround::sample_height's arithmetic (cell, fractions, one pair-table gather, the
// same blend) on the walk's domain -- inside [0, NX) x [0, NY) in grid units the bilinear patch, outside_z elsewhere.  The contact
// sampler's clamp of the cell coordinate to NX - 1e-3 (it keeps OUTSIDE points on valid addresses) is not taken over: it would
// flatten the last 1e-3 of the last cell, which the walk does not; an outside point reads cell (0, 0) and drops it.
WL_DEV float column_height(const HeightFieldGround& gr, float x, float y) {
    const WlHeightField& f = gr.f;
    const float u = (x - f.x0) * gr.inv_cell, v = (y - f.y0) * gr.inv_cell;
    const bool inside = u >= 0.f && v >= 0.f && u < (float)(f.nx - 1) && v < (float)(f.ny - 1);
    const float uc = inside ? u : 0.f, vc = inside ? v : 0.f;
    const float fi = floorf(uc), fj = floorf(vc);
    HeightFieldGround::Corners c;
    c.inside = inside;
    c.fu = uc - fi;
    c.fv = vc - fj;
    hf_corners(f, (int64_t)((int)fj * f.nx + (int)fi), c.h00, c.h10, c.h01, c.h11);
    return gr.blend(c);
}

// the column form: the ray falls straight down from the world point of its start (s.M turns about z only: the entry point checks);
// ONE bilinear sample of the terrain under it, no walk.  The hit's z is the sampled height itself (not o_z - t); a start on or under
// the terrain is its own hit point, as in the walk.
WL_DEV RayCastHit raycast_column(const HeightFieldGround& gr, const SensorFrame& s, V3 start, float tmax) {
    const V3 o = s.o + mul(s.M, start);
    const float z = column_height(gr, o.x, o.y);
    const float t = fmaxf(o.z - z, 0.f);
    return raycast_miss_or(t, tmax, v3(o.x, o.y, t > 0.f ? z : o.z));
}

}  // namespace

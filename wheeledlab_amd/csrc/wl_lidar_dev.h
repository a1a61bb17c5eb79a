// wl_lidar_dev.h -- the lidar's device functions: the sensor pose of one env and the range of one beam (see wl_lidar.hip).
// A header of its own so that tests/host_sim can compile them for the host and hold them against oracle/depth.c.
#pragma once
#include "../../include/wheeledlab_amd_lidar.h"
#include "wl_depth_dev.h"

namespace {

// the sensor of one env: origin and the rotation sensor -> world (rows)
struct LidarPose {
    V3 o;
    Mat3 M;
};

WL_DEV Mat3 mat_mul(const Mat3& a, const Mat3& b) {      // a b, row by row: row i of a b = a_i0 b.r0 + a_i1 b.r1 + a_i2 b.r2
    const auto row = [&](V3 r) { return fma3(r.x, b.r0, fma3(r.y, b.r1, r.z * b.r2)); };
    return Mat3{row(a.r0), row(a.r1), row(a.r2)};
}

// the body's rotation, or with yaw_only its yaw alone: the heading of the body's x axis in the world xy plane (IsaacLab's yaw_quat
// keeps the same angle, atan2(2 (w z + x y), 1 - 2 (y^2 + z^2))); a body pointing straight up or down keeps heading 0
WL_DEV Mat3 lidar_body_rotation(Quat q, bool yaw_only) {
    if (!yaw_only) return mat_from_quat(q);
    const float ca = 1.f - 2.f * (q.y * q.y + q.z * q.z), sa = 2.f * (q.w * q.z + q.x * q.y);
    const float n2 = ca * ca + sa * sa;
    const float inv = n2 > 0.f ? rsq(n2) : 0.f;
    const float c = n2 > 0.f ? ca * inv : 1.f, s = sa * inv;
    return Mat3{v3(c, -s, 0.f), v3(s, c, 0.f), v3(0.f, 0.f, 1.f)};
}

// the sensor of a root at `pos` with orientation `q`; `mount`: the mount rotation (offset_quat, unit)
WL_DEV LidarPose lidar_pose(const WlLidarParams& p, const Mat3& mount, V3 pos, Quat q) {
    const Mat3 R = lidar_body_rotation(q, p.yaw_only != 0);
    return LidarPose{pos + mul(R, v3(p.offset_pos[0], p.offset_pos[1], p.offset_pos[2])), mat_mul(R, mount)};
}

// the range of one beam: cast_ray with a unit direction returns the Euclidean distance of the first hit (max_range on a miss,
// 0 from under the terrain)
WL_DEV float lidar_beam(const DepthGrid& g, const Pyramid& py, const PyrHead& hd, const FieldMem& mem, const LidarPose& s, V3 d_sensor,
                        float max_range) {
    return cast_ray(g, py, hd, mem, s.o, mul(s.M, d_sensor), max_range);
}

}  // namespace

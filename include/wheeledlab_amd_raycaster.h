/* wheeledlab_amd_raycaster.h -- a ray caster: any table of rays cast from every env's sensor against the terrain solid the depth
 * camera sees (IsaacLab's RayCaster / RayCasterCamera over the terrain: grid, lidar and pinhole patterns are tables of this entry).
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): a scan is an observation read between steps, like the scene
 * camera's depth image.  Same conventions as that header: device pointers, `stream` a hipStream_t (NULL = the default stream), return 0
 * (WL_OK) or a negative WL_E* code, every argument validated before any launch.  A lidar scan is the case ray_starts = NULL (every beam
 * leaves the sensor origin), ray_scale = NULL, dist_out only: dist_out[e][k] is then the range of beam k.
 *
 * Sensor frame.  Env e's root pose is read from rows WL_S_PX.. / WL_S_QW.. of b->state.  With R = the body's rotation (alignment 0,
 * "base"), its yaw alone (1, "yaw": the heading of the body's x axis in the world xy plane, atan2(2 (w z + x y), 1 - 2 (y^2 + z^2)),
 * the angle IsaacLab's yaw_quat keeps: roll and pitch are dropped, and a body pointing straight up or down keeps heading 0), or the
 * identity (2, "world"), and mount = the rotation of offset_quat:   origin o = pos + R offset_pos,   rotation M = R mount.
 * One R turns both the offset and the rays.  IsaacLab's ray caster turns offset_pos by the FULL body rotation and leaves the
 * directions unrotated in its yaw mode [recalled, not checked against its source]; for the vertical rays that mode exists for, both
 * rules agree whenever offset_pos lies on the body z axis and the body is level, and differ by the offset's tilt otherwise.
 *
 * Ray k.  Start o + M ray_starts[k], direction M ray_dirs[k] (ray_dirs are unit vectors: the ray parameter is a Euclidean distance).
 *
 * Result.  t = the parameter of the first point of the ray on or below the terrain solid of wl_visual_depth (bilinear patches of
 * the heightfield, the plane z = hf->outside_z beyond the grid).  dist_out[e][k] = min(t, max_distance) * scale[k] (scale = 1 without
 * ray_scale; a pinhole table passes the cosine to its optical axis, which makes dist_out the distance to the image plane).  A ray
 * that meets nothing within max_distance reads max_distance * scale[k]; a start under the terrain reads 0.  hits_out[e][k] is the hit
 * point start + t direction in the world, +inf in all three components on a miss (as Warp's ray caster reports one).  At least one
 * of dist_out / hits_out must be given.  Only the terrain is seen, not other cars.
 *
 * vertical = 1, the column form.  The caller asserts that every direction is (0, 0, -1): ray_dirs must then be NULL, alignment 1 or 2
 * and the mount a rotation about z alone (offset_quat x = y = 0); anything else is WL_EINVAL.  A ray is then a vertical column over
 * the world point (x, y) of its start, and t = start_z - z_terrain(x, y) from ONE bilinear sample through the row-pair table
 * (hf->pair required; the contact samplers' arithmetic; outside [0, nx - 1) x [0, ny - 1) in grid units the height is outside_z, the
 * domain rule of the walk).  hits_out[..][2] is the sampled height itself, not start_z - t: with the elevation task's scanner 20 m
 * above the car that round trip would cost 2e-6 m.  Clipping, the miss value and "under the terrain reads 0" are as above. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_RAYCASTER_VERSION 2   /* 2: ray_starts may be NULL (every ray leaves the sensor origin) */
#define WL_RAYCAST_MAX_RAYS (1 << 20)   /* n_rays: 1 .. WL_RAYCAST_MAX_RAYS */

#define WL_RAYCAST_ALIGN_BASE 0
#define WL_RAYCAST_ALIGN_YAW 1
#define WL_RAYCAST_ALIGN_WORLD 2

typedef struct WlRayCastParams {
    float offset_pos[3];    /* sensor origin in the body frame, metres                                                */
    float offset_quat[4];   /* sensor frame against the body frame (w, x, y, z); finite, not all zero; normalised here */
    int32_t n_rays;         /* rays per env: 1 .. WL_RAYCAST_MAX_RAYS                                                  */
    float max_distance;     /* metres (> 0, finite)                                                                    */
    int32_t alignment;      /* 0 base: the full body rotation; 1 yaw: its yaw alone; 2 world: none                     */
    int32_t vertical;       /* 1: every direction is (0, 0, -1), the column form (see above); else 0                   */
} WlRayCastParams;

/* One cast per env of b (b->n_envs envs; 0: nothing is launched):
 *   hf, pyramid   the terrain and its bound pyramid (wl_heightfield_build_pyramid), as wl_visual_depth takes them
 *   ray_starts    float [n_rays][3], sensor frame; NULL without p->vertical: all zero, every ray leaves the sensor origin (no loads)
 *   ray_dirs      float [n_rays][3], unit vectors in the sensor frame; NULL if and only if p->vertical
 *   ray_scale     float [n_rays] or NULL
 *   dist_out      float [n_envs][n_rays] or NULL
 *   hits_out      float [n_envs][n_rays][3] or NULL
 * WL_EINVAL: a NULL pointer (p, b, b->state, hf, pyramid, ray_starts with vertical, ray_dirs without, both outputs), ray_dirs given
 * with vertical, n_rays outside [1, WL_RAYCAST_MAX_RAYS], max_distance not positive and finite, a non-finite or zero mount pose,
 * alignment outside 0 .. 2, vertical outside 0 .. 1 or with alignment 0 or a tilted mount or a field without its pair table, a
 * heightfield wl_visual_depth refuses, a batch the state rows cannot address, n_envs * ceil(n_rays / 64) beyond 2^31 - 1;
 * WL_EALIGN: a pointer not 4-byte aligned. */
int wl_raycast_scan(const WlRayCastParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid,
                    const float* ray_starts, const float* ray_dirs, const float* ray_scale, float* dist_out, float* hits_out,
                    void* stream);

/* WL_RAYCASTER_VERSION of the library */
int wl_raycast_version(void);

#ifdef __cplusplus
}
#endif

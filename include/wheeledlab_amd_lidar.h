/* wheeledlab_amd_lidar.h -- a lidar: range scans of every env's sensor against the terrain solid the depth camera sees.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): a scan is an observation read between steps, like the scene
 * camera's depth image.  Same conventions as that header: device pointers, `stream` a hipStream_t (NULL = the default stream),
 * return 0 (WL_OK) or a negative WL_E* code, arguments validated before any launch.
 *
 * Geometry.  Env e's root pose is read from rows WL_S_PX.. / WL_S_QW.. of b->state.  The sensor sits at offset_pos in the body
 * frame, rotated by offset_quat (w, x, y, z; normalised here) against the body; with yaw_only set the body's roll and pitch are
 * dropped and only its yaw turns the offset and the beams.  Beam k points along beam_dirs[k] (a unit vector in the sensor frame).
 *
 * Result.  ranges_out[e][k] is the Euclidean distance from the sensor to the first point of beam k on or below the terrain solid
 * (wl_visual_depth's: bilinear patches of the heightfield, the plane z = hf->outside_z beyond it), clipped at max_range; a beam that
 * meets nothing reads max_range, a sensor under the terrain reads 0 on every beam.  Only the terrain is seen, not other cars (as a
 * ray caster over static meshes). */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_LIDAR_VERSION 1
#define WL_LIDAR_MAX_BEAMS (1 << 20)   /* n_beams: 1 .. WL_LIDAR_MAX_BEAMS */

typedef struct WlLidarParams {
    float offset_pos[3];    /* sensor origin in the body frame, metres                                          */
    float offset_quat[4];   /* sensor frame against the body frame (w, x, y, z); finite, not all zero            */
    int32_t n_beams;        /* beams per scan                                                                    */
    float max_range;        /* metres (> 0, finite)                                                              */
    int32_t yaw_only;       /* 1: only the body's yaw turns the sensor (IsaacLab RayCasterCfg.attach_yaw_only)    */
} WlLidarParams;

/* One scan per env of b (b->n_envs envs; 0: nothing is launched):
 *   hf, pyramid   the terrain and its bound pyramid (wl_heightfield_build_pyramid), as wl_visual_depth takes them
 *   beam_dirs     float [n_beams][3], unit vectors in the sensor frame
 *   ranges_out    float [n_envs][n_beams]
 * WL_EINVAL: a NULL pointer, n_beams outside [1, WL_LIDAR_MAX_BEAMS], max_range not positive and finite, a non-finite or zero mount
 * pose, a heightfield wl_visual_depth refuses, a batch the state rows cannot address; WL_EALIGN: a pointer not 4-byte aligned. */
int wl_lidar_scan(const WlLidarParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid, const float* beam_dirs,
                  float* ranges_out, void* stream);

/* WL_LIDAR_VERSION of the library */
int wl_lidar_version(void);

#ifdef __cplusplus
}
#endif

/* wheeledlab_amd_viewer.h -- the viewer camera: one world camera that draws every env of a batch (the terrain or ground plane and
 * each car as a chassis box plus four wheel spheres) into an RGB frame, for env.render() and video recording.
 *
 * Not part of the drop-in step boundary (include/wheeledlab_amd.h): the viewer only READS a batch's state rows
 * (WL_S_PX .. WL_S_QZ of WlEnvBuffers.state) and never changes state, counters or RNG streams.  Same conventions as that header:
 * device pointers, `stream` a hipStream_t (NULL = the default stream), return 0 (WL_OK) or a negative WL_E* code, arguments
 * validated before any launch.
 *
 * Camera model: that of the depth camera (wl_visual_depth) -- optical axis = camera body +x, image right = body -y, image down =
 * body -z; pixel (r, c) casts the body direction (1, -(c + 0.5 - cx) / fx, -(r + 0.5 - cy) / fy), so the ray parameter IS the
 * distance along the optical axis.  The nearest hit wins; on equal distance the lower env id wins and a car beats the ground,
 * so the frame does not depend on the order in which the per-tile lists were filled. */
#pragma once
#include "wheeledlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WL_VIEWER_VERSION 1
#define WL_VIEWER_MAX_SIDE 8192      /* width and height: 1 .. 8192 pixels */
#define WL_VIEWER_TILE 16            /* the shade pass draws 16 x 16-pixel tiles, one workgroup each */

enum WlViewerGround { WL_VIEWER_PLANE = 0, WL_VIEWER_HEIGHTFIELD = 1 };

typedef struct WlViewerParams {
    int32_t width, height;     /* pixels                                                                                   */
    float cam_pos[3];          /* camera origin in the world                                                               */
    float cam_quat[4];         /* w, x, y, z: camera body frame -> world (body +x = optical axis, +y = image left, +z = up)  */
    float fx, fy, cx, cy;      /* pinhole intrinsics in pixels                                                             */
    float far_clip;            /* > 0: nothing at or beyond this distance along the optical axis is drawn (sky)           */
    int32_t ground;            /* WlViewerGround: WL_VIEWER_HEIGHTFIELD needs the heightfield and its bound pyramid       */
    float plane_z;             /* height of the ground plane (WL_VIEWER_PLANE)                                           */
    float checker;             /* > 0: edge of the two-tone checker (m) the ground shows when no traversability map is given */
    float sun[3];              /* direction towards the sun (normalised by the library)                                   */
    float ambient;             /* 0 .. 1: share of the albedo lit whatever the normal                                    */
    float box_center[3];       /* chassis box in the root frame: centre ...                                              */
    float box_half[3];         /* ... and half extents (> 0)                                                             */
    float half_wheelbase_f, half_wheelbase_r, half_track, wheel_z, wheel_radius;   /* wheel spheres (WlVehicleParams)      */
    int32_t env_index;         /* global env id drawn in the highlight colour (-1: none)                                 */
    int32_t id_offset;         /* global id of env 0 of the batch: keys the palette                                     */
} WlViewerParams;

/* bytes of device scratch wl_viewer_render needs for a width x height frame of n_envs envs; <= 0 for sizes out of range */
int64_t wl_viewer_scratch_bytes(int32_t width, int32_t height, int32_t n_envs);

/* One frame of the batch `b` (rows WL_S_PX .. WL_S_QZ, envs 0 .. n_envs - 1):
 *   hf / pyramid   the heightfield and its bound pyramid (wl_heightfield_build_pyramid) for WL_VIEWER_HEIGHTFIELD, NULL for the plane
 *   map            optional traversability map: the ground's albedo (traversable cells light); NULL: the checker
 *   scratch        wl_viewer_scratch_bytes(...) bytes of device memory, 16-byte aligned
 *   rgb            uint8 [height][width][3]
 *   depth          optional float [height][width]: distance along the optical axis, far_clip where nothing is hit
 *   id             optional int32 [height][width]: env index in the batch, -1 ground, -2 sky */
int wl_viewer_render(const WlViewerParams* p, const WlEnvBuffers* b, const WlHeightField* hf, const float* pyramid,
                     const WlTravMap* map, void* scratch, int64_t scratch_bytes, uint8_t* rgb, float* depth, int32_t* id,
                     void* stream);

/* WL_VIEWER_VERSION of the library */
int wl_viewer_version(void);

#ifdef __cplusplus
}
#endif

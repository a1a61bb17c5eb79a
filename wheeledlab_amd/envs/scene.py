"""Scene / articulation views over the SoA state matrix, exposing the attribute names the reference's term
functions read (`env.scene["robot"].data.root_pos_w`, `.find_joints(...)`, `env.scene.env_origins`, ...; census in
SURVEY.md section 8b).  These are cold-path conveniences for user plugins: [N,k] tensors are assembled from the
[k][N] rows with torch ops on the device.  The fused kernels never go through them."""
from __future__ import annotations

import re

import torch

from .. import _abi as A

MUSHR_JOINT_NAMES = [
    "front_left_wheel_steer", "front_right_wheel_steer",
    "back_left_wheel_throttle", "back_right_wheel_throttle",
    "front_left_wheel_throttle", "front_right_wheel_throttle",
    "front_left_wheel_suspension", "front_right_wheel_suspension",
    "back_left_wheel_suspension", "back_right_wheel_suspension",
]
# rigid bodies of the articulation as far as the reference's terms select them (`body_names=".*wheel_link"`,
# visual/mushr_visual_env_cfg.py:326,336): the root link and the four wheel links, wheels in the state rows' order (bl, br, fl, fr)
MUSHR_BODY_NAMES = ["base_link", "back_left_wheel_link", "back_right_wheel_link", "front_left_wheel_link", "front_right_wheel_link"]


def quat_rotate_inverse(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """body = R(q)^T world, q = (w, x, y, z)"""
    w, u = q[:, 0:1], q[:, 1:4]
    return v * (2.0 * w * w - 1.0) - torch.cross(u, v, dim=-1) * w * 2.0 + u * (u * v).sum(-1, keepdim=True) * 2.0


class ArticulationData:
    def __init__(self, batch, n_joints=len(MUSHR_JOINT_NAMES)):
        self._b = batch
        self._nj = n_joints

    def _rows(self, r0, k):
        b = self._b
        return b.state[r0:r0 + k, : b.n].T.contiguous()

    @property
    def root_pos_w(self):
        return self._rows(A.S_PX, 3)

    root_link_pos_w = root_pos_w

    @property
    def root_quat_w(self):
        return self._rows(A.S_QW, 4)

    root_link_quat_w = root_quat_w

    @property
    def root_lin_vel_w(self):
        return self._rows(A.S_VX, 3)

    root_com_lin_vel_w = root_lin_vel_w

    @property
    def root_ang_vel_w(self):
        return self._rows(A.S_WX, 3)

    root_link_ang_vel_w = root_ang_vel_w
    root_com_ang_vel_w = root_ang_vel_w

    @property
    def root_lin_vel_b(self):
        return quat_rotate_inverse(self.root_quat_w, self.root_lin_vel_w)

    @property
    def root_ang_vel_b(self):
        return quat_rotate_inverse(self.root_quat_w, self.root_ang_vel_w)

    @property
    def root_state_w(self):
        return self._rows(A.S_PX, 13)

    @property
    def root_vel_w(self):
        return self._rows(A.S_VX, 6)

    @property
    def body_pos_w(self):
        """[N, 5, 3]: the root link and the four wheel centres = root pose (+) the vehicle geometry the step kernels use
        (wl_vehicle.h::wheel_contact: wheel centre = root + R (+-half_wheelbase, +-half_track, wheel_z))"""
        v = self._b.p.vehicle
        local = torch.tensor([[0.0, 0.0, 0.0],
                              [-v.half_wheelbase_r, v.half_track, v.wheel_z], [-v.half_wheelbase_r, -v.half_track, v.wheel_z],
                              [v.half_wheelbase_f, v.half_track, v.wheel_z], [v.half_wheelbase_f, -v.half_track, v.wheel_z]],
                             dtype=torch.float32, device=self._b.device)
        q = self.root_quat_w
        w, u = q[:, None, 0:1], q[:, None, 1:4].expand(-1, local.shape[0], -1)
        lv = local[None].expand(q.shape[0], -1, -1)
        # R(q) v = v + 2 w (u x v) + 2 u x (u x v)
        c1 = torch.cross(u, lv, dim=-1)
        return self.root_pos_w[:, None, :] + lv + 2.0 * (w * c1 + torch.cross(u, c1, dim=-1))

    body_link_pos_w = body_pos_w

    @property
    def default_root_state(self):
        d = torch.zeros(self._b.n, 13, device=self._b.device)
        d[:, 3] = 1.0
        return d

    @property
    def joint_pos(self):
        b = self._b
        jp = torch.zeros(b.n, self._nj, device=b.device)
        jp[:, 0] = jp[:, 1] = b.state[A.S_STEER_POS, : b.n]
        return jp  # wheel spin angles are not integrated (no term reads them); suspension deflection is implicit

    @property
    def joint_vel(self):
        b = self._b
        jv = torch.zeros(b.n, self._nj, device=b.device)
        jv[:, 0] = jv[:, 1] = b.state[A.S_STEER_VEL, : b.n]
        jv[:, 2], jv[:, 3] = b.state[A.S_WHEEL_BL, : b.n], b.state[A.S_WHEEL_BR, : b.n]
        jv[:, 4], jv[:, 5] = b.state[A.S_WHEEL_FL, : b.n], b.state[A.S_WHEEL_FR, : b.n]
        return jv


class ArticulationView:
    def __init__(self, batch, joint_names=MUSHR_JOINT_NAMES):
        self._b = batch
        self.joint_names = list(joint_names)   # layout: [steer L, steer R, rear L, rear R, front L, front R, (suspension x4)]
        self.body_names = list(MUSHR_BODY_NAMES)
        self.data = ArticulationData(batch, len(self.joint_names))
        self.num_instances = batch.n

    def find_bodies(self, name_keys, preserve_order=False):
        keys = [name_keys] if isinstance(name_keys, str) else list(name_keys)
        ids = [i for i, n in enumerate(self.body_names) if any(re.fullmatch(k, n) for k in keys)]
        return ids, [self.body_names[i] for i in ids]

    def find_joints(self, name_keys, joint_subset=None, preserve_order=False):
        keys = [name_keys] if isinstance(name_keys, str) else list(name_keys)
        ids, names = [], []
        for i, n in enumerate(self.joint_names):
            if any(re.fullmatch(k, n) for k in keys):
                ids.append(i)
                names.append(n)
        return ids, names

    # plugin reset events (e.g. a user `reset_root_state_*` term) write through these
    def write_root_pose_to_sim(self, pose, env_ids=None):
        ids = slice(None) if env_ids is None else env_ids
        self._b.state[A.S_PX:A.S_PX + 7, ids] = pose.T.to(torch.float32)
        self._b.touch_pose()

    def write_root_velocity_to_sim(self, vel, env_ids=None):
        ids = slice(None) if env_ids is None else env_ids
        self._b.state[A.S_VX:A.S_VX + 6, ids] = vel.T.to(torch.float32)
        self._b.touch_pose()


class RayCasterData:
    """`sensor.data` of the elevation task's height scanner (isaaclab RayCaster, un-vendored): `pos_w` [N, 3] and
    `ray_hits_w` [N, 676, 3], grid order "xy" (x fastest), yaw-aligned -- what `mdp.height_scan` and the reference's
    `world_height_map` (elevation/mushr_elevation_env_cfg.py:44-48) read.  The hit heights come from the scan KERNEL
    (elev_scan_kernel through wl_elev_observe: world_height_map = hit_z + offset - plane_init, +clip on a miss), the hit
    x / y are the grid points themselves (vertical rays); rays that miss the terrain report +inf like Warp's ray caster."""

    def __init__(self, batch, offset_pos):
        self._b, self._off = batch, offset_pos

    @property
    def pos_w(self):
        b = self._b
        return b.state[A.S_PX:A.S_PX + 3, : b.n].T + torch.tensor(self._off, device=b.device, dtype=torch.float32)

    @property
    def ray_hits_w(self):
        b, p = self._b, self._b.p
        n, k = b.n, A.ELEV_SCAN_N
        hmap = b.observe(torch.empty_like(b.obs))[:, 13:]     # scratch buffer: the env's own observation stays untouched
        z = torch.where(hmap >= p.obs_clip, torch.full_like(hmap, float("inf")), hmap - p.scan_offset + p.elev_z0)
        g = -0.5 * p.scan_size + p.scan_res * torch.arange(k, device=b.device, dtype=torch.float32)
        lx, ly = g.repeat(k), g.repeat_interleave(k)
        q = b.state[A.S_QW:A.S_QW + 4, :n]
        ca, sa = 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]), 2.0 * (q[0] * q[3] + q[1] * q[2])
        inv = torch.rsqrt(ca * ca + sa * sa)
        c, s_ = (ca * inv).unsqueeze(1), (sa * inv).unsqueeze(1)
        x = b.state[A.S_PX, :n].unsqueeze(1) + c * lx - s_ * ly
        y = b.state[A.S_PY, :n].unsqueeze(1) + s_ * lx + c * ly
        return torch.stack([x, y, z], dim=-1)


class RayCasterView:
    def __init__(self, batch, cfg):
        self.cfg = cfg
        self.data = RayCasterData(batch, tuple(getattr(cfg, "offset_pos", (0.0, 0.0, 0.0))))
        self.num_instances = batch.n


class CameraData:
    """`sensor.data` of the robot's camera (isaaclab TiledCamera, un-vendored) as far as the reference's observation functions
    read it: `output["distance_to_image_plane"]` [N, 60, 80, 1] (mdp_sensors/observations.py:89-95 `camera_data_depth` /
    `raycast_depth`), rendered on access by the depth ray-cast kernel (wl_visual_depth) against the task's terrain -- the
    heightfield of the elevation task, the z = 0 plane of the others -- and clipped at the camera's far plane."""

    def __init__(self, batch, cfg):
        self._b, self._cam, self._cfg = batch, None, cfg
        # ((batch.step_count, batch.pose_epoch) it was rendered at, image): one render per env.step(), however often read --
        # and a new one after anything that moved cars without a step (reset(), the masked in-step resets of custom
        # terminations, a plugin's write_root_pose_to_sim: they bump pose_epoch)
        self._cached = (None, None)
        self.caching = True              # the env's constructor switches it off around its shape probe of the custom terms
        clip = getattr(getattr(cfg, "spawn", None), "clipping_range", None) or (0.01, 100.0)
        self.far = float(clip[1])
        self.beyond = {"max": None, "zero": 0.0, "none": float("inf")}[getattr(cfg, "depth_clipping_behavior", "max")]

    def _camera(self):
        if self._cam is None:
            from ..sensors import DepthCamera
            b = self._b
            # elevation and visual-depth tasks: the batch's own field (shared: its buffers, its pyramid); else flat ground: any grid at
            # z = 0 (beyond it the outside plane is z = 0 as well)
            hf = b.hf if b.hf is not None else (torch.zeros(3, 3, dtype=torch.float32, device=b.device), -1.0, -1.0, 1.0)
            self._cam = DepthCamera(hf, b.device, b.p if isinstance(b.p, A.WlVisualParams) else self._params_from_cfg())
        return self._cam

    def _params_from_cfg(self):
        """tasks whose batch carries no camera parameters (drift, elevation): intrinsics and mounting pose from the sensor's cfg"""
        from ..params import visual_params
        p, c = visual_params(), self._cfg
        sp = getattr(c, "spawn", None)
        if sp is not None and getattr(sp, "focal_length", None):
            p.fx = c.width * sp.focal_length / sp.horizontal_aperture
            p.fy = c.height * sp.focal_length / sp.vertical_aperture
            p.cx, p.cy = c.width / 2, c.height / 2
        if getattr(c, "body_pos", None) is not None:
            p.cam_pos[0], p.cam_pos[1], p.cam_pos[2] = c.body_pos
        return p

    @property
    def output(self):
        return _CameraOutputs(self)

    def rgb(self):
        """`output["rgb"]` [N, 60, 80, 3] uint8 (mdp_sensors/observations.py:60-62 `camera_data_rgb`): the designed camera's view of the
        black / white traversability plane, all 60 rows, no augmentation -- each pixel one ray against the z = 0 plane with a map lookup
        (white 255 on a traversable cell, black 0 off it or off the map, grey 127 where the ray misses the plane), the model the fused
        observation kernel evaluates for the lower 40 rows (csrc/wl_visual_cam_dev.h, oracle/visual_step.py::camera).  Plain torch: this is
        the un-wired debugging / logging path, not env.step()."""
        b = self._b
        if not hasattr(b, "trav_map"):
            raise KeyError("camera data type 'rgb' needs the visual task's traversability map")
        n, p = b.n, b.p
        q = b.state[A.S_QW:A.S_QW + 4, :n]
        w, x, y, z = q[0], q[1], q[2], q[3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(n, 3, 3)
        cam = torch.tensor(list(p.cam_pos), dtype=torch.float32, device=b.device)
        o = b.state[A.S_PX:A.S_PX + 3, :n].T + R @ cam
        rows = torch.arange(60, dtype=torch.float32, device=b.device)
        cols = torch.arange(80, dtype=torch.float32, device=b.device)
        dy = -((cols + 0.5 - p.cx) / p.fx)
        dz = -((rows + 0.5 - p.cy) / p.fy)
        db = torch.stack([torch.ones(60, 80, device=b.device), dy[None, :].expand(60, 80), dz[:, None].expand(60, 80)], -1).view(-1, 3)
        dw = torch.einsum("nij,pj->npi", R, db)
        hit = dw[..., 2] < -1e-6
        t = torch.where(hit, -o[:, None, 2] / torch.where(hit, dw[..., 2], torch.full_like(dw[..., 2], -1.0)), torch.zeros_like(dw[..., 2]))
        hx, hy = o[:, None, 0] + t * dw[..., 0], o[:, None, 1] + t * dw[..., 1]
        m = b.trav_map
        nr, nc = m.shape
        rs, cs = float(b._map.row_spacing), float(b._map.col_spacing)
        on_map = hit & (hx.abs() <= nr * rs / 2) & (hy.abs() <= nc * cs / 2)
        # the reward terms' lookup (visual/utils/traversability_utils.py:68-88): (x + width / 2 + spacing / 2) / spacing truncated towards
        # zero, clamped, map[y, x]
        ix = torch.clamp(((hx + (nr * rs / 2 + rs / 2)) / rs).long(), 0, nr - 1)
        iy = torch.clamp(((hy + (nc * cs / 2 + cs / 2)) / cs).long(), 0, nc - 1)
        white = on_map & m.bool()[iy, ix]
        grey = torch.where(hit, torch.where(white, 255, 0), 127).to(torch.uint8)
        return grey.view(n, 60, 80, 1).expand(n, 60, 80, 3).contiguous()


class _CameraOutputs:
    def __init__(self, data):
        self._d = data

    def __getitem__(self, key):
        if key == "rgb":
            return self._d.rgb()
        if key != "distance_to_image_plane":
            raise KeyError(f"camera data type {key!r} is not rendered here (the fused observation carries the grey image)")
        d = self._d
        stamp = (getattr(d._b, "step_count", None), getattr(d._b, "pose_epoch", None))
        if not d.caching or None in stamp:
            img = d._camera().render(d._b, d.far)
        else:
            if d._cached[0] != stamp:       # the render is cached per env step; what lies beyond the far plane is applied per read
                d._cached = (stamp, d._camera().render(d._b, d.far))
            img = d._cached[1]
        if d.beyond is not None:
            img = torch.where(img >= d.far, torch.full_like(img, d.beyond), img)
        return img.unsqueeze(-1)

    def keys(self):
        return ["distance_to_image_plane"]


class SensorView:
    """`env.scene.sensors[name]`: the sensor's config and its `data` object, of the subclass's `data_class`"""
    data_class = None

    def __init__(self, batch, cfg):
        self.cfg = cfg
        self.data = self.data_class(batch, cfg)
        self.num_instances = batch.n


class CameraView(SensorView):
    data_class = CameraData


def _quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Hamilton product of (w, x, y, z) quaternions, broadcast over leading dimensions"""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _quat_apply(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """R(q) v, q = (w, x, y, z): v + 2 w (u x v) + 2 u x (u x v)"""
    w, u = q[..., 0:1], q[..., 1:4]
    c = torch.cross(u, v, dim=-1)
    return v + 2.0 * (w * c + torch.cross(u, c, dim=-1))


def _scan_once_per_step(data, scan):
    """`scan()` of a sensor's data object, cached in `data._cached` per (batch.step_count, batch.pose_epoch): one scan per env.step(),
    however often read, and a new one after anything that moved cars without a step (see CameraData); `data.caching` False (the
    env's shape probe) or a batch without those counters: no caching"""
    stamp = (getattr(data._b, "step_count", None), getattr(data._b, "pose_epoch", None))
    if not data.caching or None in stamp:
        return scan()
    if data._cached[0] != stamp:
        data._cached = (stamp, scan())
    return data._cached[1]


class RayCasterSensorData:
    """`sensor.data` of a scene ray caster (envs.sensors_cfg.RayCasterCfg with any pattern; IsaacLab's RayCaster, un-vendored), cast by
    sensors.RayCaster (wl_raycast_scan) against the task's terrain: `ray_hits_w` [N, R, 3] (+inf where a ray meets nothing within
    max_distance, as Warp's ray caster reports a miss) -- what `mdp.height_scan` reads -- `distances` [N, R] (max_distance on a miss),
    `pos_w` [N, 3] and `quat_w` [N, 4] (w, x, y, z) of the sensor.  One scan per (step_count, pose_epoch), like CameraData."""

    def __init__(self, batch, cfg):
        self._b, self._cfg, self._scanner = batch, cfg, None
        self._cached = (None, None)       # ((step_count, pose_epoch), (distances, hits))
        self.caching = True               # the env's constructor switches it off around its shape probe of the custom terms

    def _new_scanner(self):
        from ..sensors import RayCaster
        return RayCaster(self._cfg, self._b.device)

    def scanner(self):
        if self._scanner is None:
            self._scanner = self._new_scanner()
        return self._scanner

    def _scan(self):
        """(distances, hits) of the current poses (cached per env step; do not write into them)"""
        return _scan_once_per_step(self, lambda: self.scanner().scan(self._b))

    def _body_quat(self):
        """what turns the sensor, by the config's alignment (no scanner, no device): the body's rotation ("base": a ray-caster camera,
        a lidar without attach_yaw_only), its yaw alone (IsaacLab's yaw_quat: the heading of the body's x axis in the world xy plane)
        or nothing ("world")"""
        b, cfg = self._b, self._cfg
        q = b.state[A.S_QW:A.S_QW + 4, : b.n].T
        align = cfg.alignment() if hasattr(cfg, "alignment") else "yaw" if getattr(cfg, "attach_yaw_only", False) else "base"
        if align == "base":
            return q
        if align == "world":
            return torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=b.device).expand(b.n, 4)
        w, x, y, z = q.unbind(-1)
        yaw = torch.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
        zero = torch.zeros_like(yaw)
        return torch.stack([torch.cos(0.5 * yaw), zero, zero, torch.sin(0.5 * yaw)], -1)

    @property
    def pos_w(self):
        b = self._b
        off = torch.tensor(self._cfg.offset_pos, dtype=torch.float32, device=b.device).expand(b.n, 3)
        return b.state[A.S_PX:A.S_PX + 3, : b.n].T + _quat_apply(self._body_quat(), off)

    @property
    def quat_w(self):
        """the sensor frame (x forward, y left, z up) in the world"""
        mount = torch.tensor(self.scanner().params.offset_quat[:], dtype=torch.float32, device=self._b.device)
        return _quat_mul(self._body_quat(), mount.expand(self._b.n, 4))

    @property
    def distances(self):
        return self._scan()[0]

    @property
    def ray_hits_w(self):
        return self._scan()[1]


class LidarData(RayCasterSensorData):
    """`sensor.data` of a scene lidar (envs.sensors_cfg.LidarCfg; an IsaacLab RayCaster with a lidar pattern, un-vendored):
    `output["linear_depth"]` [N, B] -- the ranges `mdp.lidar_ranges` / `mdp.lidar_ranges_normalized` read (mdp_sensors/
    observations.py:25-58) -- scanned by sensors.LidarScanner (the ray caster's walk, distances only) against the task's terrain;
    `ray_hits_w` [N, B, 3] rebuilt from the ranges (+inf where a beam meets nothing within max_range, as Warp's ray caster reports a
    miss); `pos_w`, `quat_w` and the one scan per (step_count, pose_epoch) are the ray caster's."""

    def __init__(self, batch, cfg):
        super().__init__(batch, cfg)
        self.max_range = float(cfg.max_range)
        self.beyond = {"max": None, "zero": 0.0, "none": float("inf")}[cfg.miss_value]

    def _new_scanner(self):
        from ..sensors import LidarScanner
        return LidarScanner(self._cfg, self._b.device)

    def _scan(self):
        """(ranges, None): the observation path pays for the distances alone"""
        return _scan_once_per_step(self, lambda: (self.scanner().render(self._b), None))

    def ranges(self) -> torch.Tensor:
        """the raw scan of the current poses: max_range on a miss (cached per env step; do not write into it)"""
        return self._scan()[0]

    @property
    def output(self):
        return _LidarOutputs(self)

    @property
    def ray_hits_w(self):
        r = self.ranges()
        q = self.quat_w
        d = _quat_apply(q[:, None, :].expand(-1, r.shape[1], -1), self.scanner().beam_dirs[None].expand(r.shape[0], -1, -1))
        hits = self.pos_w[:, None, :] + r[..., None] * d
        return torch.where((r >= self.max_range)[..., None], torch.full_like(hits, float("inf")), hits)


class _LidarOutputs:
    def __init__(self, data):
        self._d = data

    def __getitem__(self, key):
        if key != "linear_depth":
            raise KeyError(f"lidar data type {key!r} is not rendered here (the scan gives 'linear_depth')")
        d = self._d
        r = d.ranges()
        if d.beyond is not None:      # what a miss reads is applied per read, the scan itself is cached
            r = torch.where(r >= d.max_range, torch.full_like(r, d.beyond), r)
        return r

    def keys(self):
        return ["linear_depth"]


class RayCasterCameraData(RayCasterSensorData):
    """`sensor.data` of a ray-caster camera (envs.sensors_cfg.RayCasterCameraCfg; IsaacLab's RayCasterCamera, un-vendored):
    `output["distance_to_image_plane"]` / `output["distance_to_camera"]` [N, H, W, 1] -- what `mdp.camera_data_depth` / `raycast_depth`
    read -- `intrinsic_matrices` [N, 3, 3], `pos_w`, `quat_w_world` / `quat_w_ros` / `quat_w_opengl` [N, 4].  A pixel whose ray meets
    nothing within max_distance reads what depth_clipping_behavior says: max_distance, 0 or +inf."""

    def __init__(self, batch, cfg):
        super().__init__(batch, cfg)
        self.beyond = {"max": float(cfg.max_distance), "zero": 0.0, "none": float("inf")}[cfg.depth_clipping_behavior]
        self.image_shape = (int(cfg.pattern_cfg.height), int(cfg.pattern_cfg.width))

    @property
    def output(self):
        return _RayCasterCameraOutputs(self)

    @property
    def intrinsic_matrices(self):
        fx, fy, cx, cy = self._cfg.pattern_cfg.intrinsics()
        k = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32, device=self._b.device)
        return k.expand(self._b.n, 3, 3)

    quat_w_world = RayCasterSensorData.quat_w

    def _quat_w_in(self, convention):
        from .sensors_cfg import CAMERA_CONVENTION_TO_WORLD
        w, x, y, z = CAMERA_CONVENTION_TO_WORLD[convention]
        back = torch.tensor([w, -x, -y, -z], dtype=torch.float32, device=self._b.device)
        return _quat_mul(self.quat_w, back.expand(self._b.n, 4))

    quat_w_ros = property(lambda self: self._quat_w_in("ros"))
    quat_w_opengl = property(lambda self: self._quat_w_in("opengl"))


class _RayCasterCameraOutputs:
    def __init__(self, data):
        self._d = data

    def __getitem__(self, key):
        d = self._d
        if key not in self.keys():
            raise KeyError(f"ray-caster camera data type {key!r} is not rendered here (it gives {self.keys()})")
        dist, hits = d._scan()
        if key == "distance_to_camera":      # the scan is the image-plane distance: Euclidean distance x the ray's cosine
            dist = dist / d.scanner().ray_scale
        # what a miss reads is applied per read, the scan itself is cached
        dist = torch.where(torch.isinf(hits[..., 0]), torch.full_like(dist, d.beyond), dist)
        return dist.view(dist.shape[0], *d.image_shape, 1)

    def keys(self):
        return ["distance_to_image_plane", "distance_to_camera"]


class LidarView(SensorView):
    data_class = LidarData


class RayCasterSensorView(SensorView):
    data_class = RayCasterSensorData


class RayCasterCameraView(SensorView):
    data_class = RayCasterCameraData


class TerrainLevelsView:
    """`env.scene.terrain` of an env that carries terrain levels: the terrain's config (every attribute of it reads through) plus
    IsaacLab's TerrainImporter tensors -- `terrain_levels` / `terrain_types` int32 [n], LIVE (the tensors the step kernels read and
    write), `terrain_origins` [rows, cols, 3] (tile centres, z = the terrain's height there) and `env_origins` [n, 3].  With flat
    patches (field.FlatPatches): `flat_patches[name]` [rows, cols, P, 3], every patch's (x, y, z) as the device found it;
    `terrain_types` is then the tile's column (type // P) and the origins stay the tile centres."""

    def __init__(self, cfg, batch):
        self.__dict__.update(_cfg=cfg, _b=batch)

    def __getattr__(self, name):
        return getattr(self.__dict__["_cfg"], name)

    def __setattr__(self, name, value):
        setattr(self._cfg, name, value)

    def _levels(self, what: str):
        """the batch's level tables; without them (patches that no reset term spawns on, no terrain-levels term) the importer's per-env
        tensors do not exist"""
        lv = self._b.levels
        if lv is None:
            # (not an AttributeError: __getattr__ would take over and report the config's missing attribute instead)
            raise RuntimeError(f"scene.terrain.{what}: this env carries no terrain levels -- its flat patches are exposed (flat_patches) but "
                                 "no reset term spawns on them (mdp.reset_root_state_from_terrain) and there is no terrain_levels curriculum term")
        return lv

    @property
    def flat_patches(self):
        lv, gen = self._b.levels, self._b.hf.generator
        shape = lv.grid_shape if lv is not None else (int(gen.num_rows), int(gen.num_cols)) if gen is not None else (1, 1)
        return {name: fp.positions().reshape(*shape, fp.n_patches, 3) for name, fp in self._b.flat_patches.items()}

    @property
    def terrain_levels(self):
        return self._levels("terrain_levels").terrain_levels

    @property
    def terrain_types(self):
        return self._levels("terrain_types").terrain_types

    @property
    def terrain_origins(self):
        lv, hf = self._levels("terrain_origins"), self._b.hf
        o = lv.tile_origins
        u, v = (o[:, 0] - hf.x0) / hf.cell, (o[:, 1] - hf.y0) / hf.cell
        ny, nx = hf.heights.shape
        i, j = u.floor().long().clamp(0, nx - 2), v.floor().long().clamp(0, ny - 2)
        fu, fv = (u - i).clamp(0, 1), (v - j).clamp(0, 1)
        h = hf.heights
        z = (h[j, i] * (1 - fu) + h[j, i + 1] * fu) * (1 - fv) + (h[j + 1, i] * (1 - fu) + h[j + 1, i + 1] * fu) * fv
        return torch.cat([o, z[:, None]], 1).reshape(*lv.grid_shape, 3)

    @property
    def env_origins(self):
        lv = self._levels("env_origins")
        return self.terrain_origins[lv.terrain_levels.long(), lv.terrain_types.long()]


class SceneView:
    @property
    def env_origins(self):
        """[n, 3]: zeros (env_spacing = 0, mushr_drift_env_cfg.py:373) unless the batch carries terrain levels -- then every env's tile centre"""
        if self._b.levels is not None:
            return self.terrain.env_origins
        return self._zero_origins

    def __init__(self, batch, cfg=None, task: str = "drift"):
        self._b = batch
        self.cfg = cfg
        self.num_envs = batch.n
        self._zero_origins = torch.zeros(batch.n, 3, device=batch.device)
        names = getattr(getattr(cfg, "robot", None), "joint_names", None) or MUSHR_JOINT_NAMES
        self.articulations = {"robot": ArticulationView(batch, names)}
        self.sensors = {}
        if task == "elevation" and getattr(cfg, "height_scanner", None) is not None:
            self.sensors["height_scanner"] = RayCasterView(batch, cfg.height_scanner)
        if getattr(cfg, "camera", None) is not None:
            self.sensors["camera"] = CameraView(batch, cfg.camera)
        from .sensors_cfg import LidarCfg, RayCasterCameraCfg, RayCasterCfg
        # every lidar, ray caster and ray-caster camera of the scene, under its attribute name (the elevation task's fused
        # height_scanner above keeps its own view)
        for name, value in (vars(cfg).items() if cfg is not None else ()):
            if name in self.sensors:
                continue
            if isinstance(value, LidarCfg):
                self.sensors[name] = LidarView(batch, value)
            elif isinstance(value, RayCasterCfg):
                self.sensors[name] = RayCasterSensorView(batch, value)
            elif isinstance(value, RayCasterCameraCfg):
                self.sensors[name] = RayCasterCameraView(batch, value)
        self.terrain = getattr(cfg, "terrain", None)
        if getattr(batch, "levels", None) is not None or getattr(batch, "flat_patches", None):
            self.terrain = TerrainLevelsView(self.terrain, batch)

    def __getitem__(self, key):
        if key in self.articulations:
            return self.articulations[key]
        if key in self.sensors:
            return self.sensors[key]
        if key == "terrain":
            return self.terrain
        raise KeyError(key)

    def keys(self):
        return list(self.articulations) + list(self.sensors) + ["terrain"]

"""DriftBatch, ElevBatch, VisualBatch, VisualDepthBatch: device buffers of one shard of a task's envs + thin calls into the C ABI,
with what they share (_EnvBatch, ring_plan, the startup events).  The terrain a batch stands on is field.py's, the sensors that
read it sensors.py's; their names are re-exported here, where they used to live.

PyTorch is plumbing here: it owns the HBM allocations and the stream; every kernel is ours (csrc/*.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from types import MappingProxyType

import torch

from . import _abi as A
from .field import (DeviceHeightField, FlatPatches, TerrainLevels, _canonical_device, _launch_terrain_generator,  # noqa: F401
                    find_flat_patches, generate_heightfield, mesh_heightfield, pair_table)
from .params import drift_params
from .sensors import DepthCamera, LidarScanner, RayCaster, _cached_depth_camera, _field_key  # noqa: F401
from .terrain import synthetic_heightfield


def stadium_reference_poses(u: torch.Tensor, track_radius: float = 0.8, straight: float = 0.8) -> torch.Tensor:
    """Pre-sampled reset poses on the stadium centre line: arclength u*L -> (x, y, yaw rad), [3, P].
    Follows reset_root_state_along_track.generate_reference_poses (wheeledlab_tasks/drifting/mdp/events.py:33-100):
    four pieces -- right straight (yaw 90 deg), top arc, left straight (yaw 270 deg), bottom arc."""
    r, s = track_radius, straight
    d = u.double() * (2.0 * math.pi * r + 4.0 * s)
    x, y, yaw = torch.empty_like(d), torch.empty_like(d), torch.empty_like(d)
    b1, b2, b3 = 2 * s, 2 * s + math.pi * r, 4 * s + math.pi * r
    m = d < b1
    x[m], y[m], yaw[m] = r, d[m] - s, math.pi / 2
    m = (d >= b1) & (d < b2)
    a = (d[m] - b1) / r
    x[m], y[m], yaw[m] = r * torch.cos(a), s + r * torch.sin(a), math.pi / 2 + a
    m = (d >= b2) & (d < b3)
    x[m], y[m], yaw[m] = -r, s - (d[m] - b2), 1.5 * math.pi
    m = d >= b3
    a = (d[m] - b3) / r
    x[m], y[m], yaw[m] = -r * torch.cos(a), -s - r * torch.sin(a), 1.5 * math.pi + a
    return torch.stack([x, y, yaw]).float()


def apply_startup_events(lib, bufs: "A.WlEnvBuffers", su, seed: int, stream, randomize: bool = True):
    """startup-mode events (domain randomisation, applied once): bucketed wheel friction
    (isaaclab randomize_rigid_body_material), throttle damping (randomize_actuator_gains, "abs"), base mass
    (randomize_rigid_body_mass, "add" onto the chassis mass).  Reference configs: mushr_drift_env_cfg.py:98-119,145-154;
    elevation cfg :387-407; visual cfg :264-299.  One launch of wl_startup_randomize: the draws are keyed by the GLOBAL
    env id (bufs.env_offset + e), so a sharded run holds the same parameter sets as the one big batch."""
    sp = A.WlStartupParams((C.c_float * 2)(*su.wheel_mu_s), (C.c_float * 2)(*su.wheel_mu_d), int(su.mu_buckets),
                           int(bool(su.mu_consistent)), (C.c_float * 2)(*su.damping), float(su.chassis_mass),
                           (C.c_float * 2)(*su.mass_add), int(bool(randomize)), (C.c_float * 2)(*getattr(su, "wheel_mass", (0.0, 0.0))))
    A.check(lib.wl_startup_randomize(C.byref(sp), C.byref(bufs), int(seed), stream), "wl_startup_randomize")


def ring_plan(step0: int, n_steps: int, slots: int):
    """How a persistent launch of `n_steps` steps from step `step0` runs on a metric ring of `slots` slots.  The launch folds all
    its steps into slot step0 % R and clears slot (step0 + n) % R for its successor.  Returns (segments, zero):
    segments -- the launches as (first step, steps): [(0, n)], or [(0, 1), (1, n - 1)] when n is a multiple of R: those two
    slots are then the same and the C ABI refuses the launch (WL_EINVAL).  Like n single steps, the split leaves the ring without
    the first step's counts (a ring of R slots holds R - 1 steps);
    zero -- the slots the host clears before the launches: those of the steps a launch folds away, which would otherwise keep
    the counts of an earlier pass over the ring."""
    if slots <= 1 or n_steps <= 1:
        return [(0, n_steps)], []
    segments = [(0, 1), (1, n_steps - 1)] if n_steps % slots == 0 else [(0, n_steps)]
    zero = sorted({(step0 + k0 + i) % slots for k0, k in segments for i in range(1, k)})
    return segments, zero


class _EnvBatch:
    """What every task's batch holds: n envs resident on one GPU as a SoA state matrix [S_COUNT, stride] (fp32), the per-step
    output rows, the episode-metric accumulators and the WlEnvBuffers / WlStepOut structs that hand them to the C ABI.  A task
    names its C entry points (_C_*) and sets `_args`: WlEnvBuffers and the task's own structs, by reference -- the arguments
    after the params of every reset / step / rollout call.

    `metrics_raw` is what the kernels add into: [slots][WL_M_SHARDS][WL_M_COUNT].  `metrics` is the logical value (sum over the
    shards): [WL_M_COUNT] for one accumulator, [slots][WL_M_COUNT] for a ring; a fresh tensor per read."""

    OBS_DIM: int
    LANES = (0, 1, 4)              # the step-kernel forms set_lanes() accepts
    _C_RESET = _C_STEP = _C_ROLLOUT = _C_PERSISTENT = None
    _PERSISTENT_NEEDS_ROWS = True  # the persistent kernel writes step k's observation while step k + 1 runs
    pose_epoch = 0       # bumped by everything that moves cars WITHOUT advancing step_count (resets, plugin pose writes)
    _out_key = None
    _ring_split_warned = False
    # the terrain a batch carries: a DeviceHeightField, a TerrainLevels, {name: FlatPatches} (ElevBatch and VisualDepthBatch set their own)
    hf = levels = None
    flat_patches = MappingProxyType({})

    def __init__(self, n_envs: int, device, params, seed: int, env_offset: int, metrics_slots: int, ref_table=None):
        self.lib = A.load()  # raises HipExtensionMissing -- no fallback
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing(f"{type(self).__name__} needs a HIP device (device='cuda:N'); there is no CPU path")
        self._stream = partial(A.stream, self.device)      # the current stream as every launch takes it
        self.n = int(n_envs)
        self.stride = ((self.n + 63) // 64) * 64
        self.p, self.seed, self.env_offset, self.step_count = params, int(seed), int(env_offset), 0
        dev = self.device
        self.state = torch.zeros(A.S_COUNT, self.stride, dtype=torch.float32, device=dev)
        self.episode_len = torch.zeros(self.stride, dtype=torch.int32, device=dev)
        self.metrics_slots = int(metrics_slots)
        self.metrics_raw = torch.zeros(self.metrics_slots, A.M_SHARDS, A.M_COUNT, dtype=torch.float32, device=dev)
        self.obs = torch.zeros(self.n, self.OBS_DIM, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(self.n, dtype=torch.float32, device=dev)
        # torch.bool is one byte holding 0 / 1: the kernel's uint8 outputs land in it directly
        self.terminated = torch.zeros(self.n, dtype=torch.bool, device=dev)
        self.truncated = torch.zeros(self.n, dtype=torch.bool, device=dev)
        self.dones = torch.zeros(self.n, dtype=torch.long, device=dev)   # terminated | truncated, as RSL-RL consumes it
        if ref_table is not None:
            self.ref_table = ref_table.to(dev)
        self._bufs = A.WlEnvBuffers(self.state.data_ptr(), self.episode_len.data_ptr(),
                                    None if ref_table is None else self.ref_table.data_ptr(), self.metrics_raw.data_ptr(),
                                    self.stride, self.n, self.env_offset, self.metrics_slots, 0, 0)
        self._out = A.WlStepOut(self.obs.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                self.truncated.data_ptr(), self.dones.data_ptr())
        self._args = (C.byref(self._bufs),)

    @property
    def metrics(self) -> torch.Tensor:
        m = self.metrics_raw.sum(1)
        return m[0] if self.metrics_slots == 1 else m

    def read_metrics(self, zero: bool = True) -> torch.Tensor:
        m = self.metrics
        if zero:
            self.metrics_raw.zero_()
        return m

    def touch_pose(self):
        """anything cached per env.step() from the poses (the scene camera's render) is stale after this"""
        self.pose_epoch = self.pose_epoch + 1

    def set_flags(self, flags: int = 0):
        """WlEnvBuffers.flags (_abi.FLAG_*): force an instantiation the launchers otherwise pick from the batch size -- the
        streaming (non-temporal store) forms or the cache-allocating forms.  0 = by size.  What the tests use to run the large-batch forms at small sizes (and vice versa).
        FLAG_STEP_LAUNCHES keeps DriftBatch.rollout() on one step-kernel launch per step (probes and tests of that kernel);
        FLAG_ROLLOUT_ONE_ROLE keeps its rollout-kernel launches on the single-role kernel (A/B runs, tests of the two-role kernel)."""
        self._bufs.flags = int(flags)

    def set_lanes(self, lanes: int = 0):
        """step-kernel form, one of LANES: 0 = by env count (quad up to 32 768 envs; drift: lane form with packed axles up to
        262 144, with the scalar wheel loop beyond), 1 = lane per env (drift: packed axles), 2 = drift's lane form with the scalar
        wheel loop, 4 = quad per env"""
        assert lanes in self.LANES
        self._bufs.lanes = lanes

    def set_dones_output(self, on: bool = True):
        """the int64 `dones` row (terminated | truncated as RSL-RL's runner consumes it, + 8 B per env-step) of step() /
        in-place rollouts on or off; callers that read the two byte rows do not need it"""
        self._out.dones = self.dones.data_ptr() if on else None

    def reset(self, mask: torch.Tensor | None = None):
        self.touch_pose()
        m = None if mask is None else mask.to(torch.uint8).contiguous()
        A.check(getattr(self.lib, self._C_RESET)(C.byref(self.p), *self._args, None if m is None else m.data_ptr(), self.seed,
                                                 self.step_count, self._stream()), self._C_RESET)

    def _actions(self, actions: torch.Tensor) -> torch.Tensor:
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.shape != (self.n, 2):
            actions = actions.to(torch.float32).reshape(self.n, 2).contiguous()
        return actions

    def step(self, actions: torch.Tensor):
        """actions [n, 2] -> (obs [n, OBS_DIM], reward [n], terminated [n], truncated [n]): the batch's own rows (views)"""
        return self._step(actions)

    def _step(self, actions, *after_actions):
        A.check(getattr(self.lib, self._C_STEP)(C.byref(self.p), *self._args, self._actions(actions).data_ptr(), *after_actions,
                                                C.byref(self._out), self.seed, self.step_count, self._stream()), self._C_STEP)
        self.step_count += 1
        return self.obs, self.reward, self.terminated, self.truncated

    def rollout(self, actions: torch.Tensor, obs_out=None, rew_out=None, term_out=None, trunc_out=None, dones_out=None,
                persistent: bool = False):
        """K fused steps with pre-staged actions [K, n, 2]; optional [K, ...] output storage (else the batch's own rows,
        overwritten): one launch per step (DriftBatch: fewer where the results allow, see its rollout()).
        persistent=True runs them as ONE launch with the state in registers (_C_PERSISTENT: quad form,
        n <= 32 768; the elevation scan / the visual camera of step k overlapped with step k + 1); same results."""
        self._rollout(actions, (obs_out, rew_out, term_out, trunc_out, dones_out), persistent)

    def _rollout(self, actions, rows, persistent):
        K = actions.shape[0]
        assert actions.shape == (K, self.n, 2) and actions.dtype == torch.float32 and actions.is_contiguous()
        if not persistent:
            return self._launch_rollout(self._C_ROLLOUT, actions, rows)
        assert rows[0] is not None or K == 1 or not self._PERSISTENT_NEEDS_ROWS, "a persistent rollout needs per-step output rows"
        segments = self._ring_segments(K)
        if len(segments) == 1:
            return self._launch_rollout(self._C_PERSISTENT, actions, rows)
        for k0, k in segments:
            self._launch_rollout(self._C_PERSISTENT, actions[k0:k0 + k], [None if t is None else t[k0:k0 + k] for t in rows])

    def _launch_rollout(self, fn, actions, rows):
        obs_out, rew_out, term_out, trunc_out, dones_out = rows
        if obs_out is not None:
            key = (obs_out.data_ptr(), rew_out.data_ptr(), term_out.data_ptr(), trunc_out.data_ptr(),
                   None if dones_out is None else dones_out.data_ptr())
            if self._out_key != key:      # the struct of the caller's storage rows, rebuilt when they change
                self._out_key, self._out_rows = key, A.WlStepOut(*key)
            out, os_, vs_ = self._out_rows, self.n * self.OBS_DIM, self.n
        else:
            out, os_, vs_ = self._out, 0, 0
        K = actions.shape[0]
        A.check(getattr(self.lib, fn)(C.byref(self.p), *self._args, actions.data_ptr(), C.byref(out), os_, vs_, K, self.seed,
                                      self.step_count, self._stream()), fn)
        self.step_count += K

    def _ring_segments(self, n_steps: int):
        """the launches (first step, steps) of a persistent run of n_steps steps from step_count (ring_plan), after clearing the
        ring slots they fold away; warns once per batch when the run is split"""
        segments, zero = ring_plan(self.step_count, n_steps, self.metrics_slots)
        if len(segments) > 1 and not self._ring_split_warned:
            import warnings
            warnings.warn(f"a persistent rollout of {n_steps} steps with a metric ring of {self.metrics_slots} slots is run as 1 + "
                          f"{n_steps - 1} steps: the ring then misses the first step's episode counts (choose a rollout length that is "
                          "not a multiple of metrics_slots to keep them)", stacklevel=4)
            self._ring_split_warned = True
        if zero:
            self.metrics_raw[zero] = 0
        return segments


class DriftBatch(_EnvBatch):
    """n drift envs resident on one GPU (csrc/wl_drift.hip)."""

    OBS_DIM = 14
    OBS_TERM_WIDTHS = (3, 3, 3, 3, 2)      # root_pos_w | root_euler_xyz | base_lin_vel | base_ang_vel | last_action
    assert sum(OBS_TERM_WIDTHS) == OBS_DIM
    LANES = (0, 1, 2, 4)           # 2: lane form with the scalar wheel loop (drift only)
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_drift_reset", "wl_drift_step", "wl_drift_rollout", "wl_drift_rollout_persistent"
    _PERSISTENT_NEEDS_ROWS = False

    def __init__(self, n_envs: int, device="cuda:0", params: A.WlDriftParams | None = None, seed: int = 42,
                 env_offset: int = 0, randomize: bool = True, metrics_slots: int = 1, startup=None):
        p = params if params is not None else drift_params()
        # reference poses are drawn ONCE at construction (events.py:31,35)
        ref_table = torch.zeros(3, 32, dtype=torch.float32)
        tr = (startup.track_radius, startup.track_straight) if startup is not None else (0.8, 0.8)
        g = torch.Generator().manual_seed(int(seed))
        ref_table[:, : p.num_ref_points] = stadium_reference_poses(torch.rand(p.num_ref_points, generator=g), *tr)
        super().__init__(n_envs, device, p, seed, env_offset, metrics_slots, ref_table)
        self._startup_events(randomize, startup)

    # startup events (mushr_drift_env_cfg.py:98-119, 145-154)
    def _startup_events(self, randomize: bool, su=None):
        if su is None:  # the RSS drift defaults
            from .envs.flatten import StartupSpec
            su = StartupSpec(wheel_mu_s=(0.3, 0.5), wheel_mu_d=(0.3, 0.5), mu_buckets=20, mu_consistent=True,
                             damping=(10.0, 50.0), mass_add=(0.3, 0.5))
        apply_startup_events(self.lib, self._bufs, su, self.seed, self._stream(), randomize)

    def observe(self, noise: torch.Tensor | None = None) -> torch.Tensor:
        A.check(self.lib.wl_drift_observe(C.byref(self.p), C.byref(self._bufs),
                                          None if noise is None else noise.data_ptr(), self.obs.data_ptr(), self.seed,
                                          self.step_count, self._stream()), "wl_drift_observe")
        return self.obs

    def step(self, actions: torch.Tensor, noise: torch.Tensor | None = None):
        """actions [n,2] fp32 on device -> (obs [n,14], reward [n], terminated u8 [n], truncated u8 [n]) (views)"""
        return self._step(actions, None if noise is None else noise.data_ptr())

    def rollout(self, actions: torch.Tensor, obs_out: torch.Tensor | None = None, rew_out: torch.Tensor | None = None,
                term_out: torch.Tensor | None = None, trunc_out: torch.Tensor | None = None, persistent: bool = False,
                dones_out: torch.Tensor | None = None):
        """K fused steps with pre-staged actions [K,n,2]; optional [K,...] output storage (else overwrite).  Same results as K
        calls of step(), in as few launches as the metric ring allows (wl_drift_rollout): with metrics_slots == 1, K >= 2 and a
        batch that steps in the quad form, launches of the persistent rollout kernel (<= 1024 steps each, the state in registers
        from step to step); with a metric ring, a forced lane / streaming form or FLAG_STEP_LAUNCHES, one launch per step.
        persistent=True asks for ONE launch outright (wl_drift_rollout_persistent): on a metric ring it folds the K steps'
        counts into one slot."""
        self._rollout(actions, (obs_out, rew_out, term_out, trunc_out, dones_out), persistent)

    def rollout_policy(self, actor_critic, storage, evaluate_critic: bool = True, start: int = 0, count: int | None = None):
        """The runner's collection loop (modified_rsl_rl_runner.py:70-80) as one launch: `count` times
        { actor(obs) on the matrix pipe -> sample -> env.step } with the env state and the observation in registers
        (wl_drift_rollout_policy), filling storage rows start .. start + count; then (optionally) the critic over ALL
        observation rows of the storage in one wl_mlp_forward.  Row `start` of storage.observations is seeded with the
        current observation; self.obs ends as the last one."""
        K = storage.n_steps - start if count is None else int(count)
        assert storage.n_envs == self.n and actor_critic.actor.in_dim == self.OBS_DIM and 0 <= start and start + K <= storage.n_steps
        for k0, k in self._ring_segments(K):
            s = start + k0
            storage.observations[s].copy_(self.obs)
            actor, io = actor_critic.actor.struct(), storage.struct(s)
            A.check(self.lib.wl_drift_rollout_policy(C.byref(self.p), C.byref(self._bufs), C.byref(actor),
                                                     actor_critic.std.data_ptr(), C.byref(io), k, self.seed, self.step_count,
                                                     self._stream()), "wl_drift_rollout_policy")
            self.step_count += k
            if k > 0:
                e = s + k
                self.obs.copy_(storage.observations[e])
                self.reward.copy_(storage.rewards[e - 1])
                self.terminated.copy_(storage.terminated[e - 1])
                self.truncated.copy_(storage.time_outs[e - 1])
                self.dones.copy_(storage.dones[e - 1])
        if evaluate_critic:
            storage.values.copy_(actor_critic.critic(storage.observations).squeeze(-1))
        return storage


class ElevBatch(_EnvBatch):
    """n elevation-task envs on one GPU (same SoA state matrix; rows WL_S_CMD_* carry the goal command)."""

    OBS_DIM = A.ELEV_OBS_DIM
    # goal_relative_xyz (x, y) | root_euler_xyz | base_lin_vel | base_ang_vel | last_action | world_height_map
    OBS_TERM_WIDTHS = (2, 3, 3, 3, 2, A.ELEV_SCAN_N * A.ELEV_SCAN_N)
    assert sum(OBS_TERM_WIDTHS) == OBS_DIM
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_elev_reset", "wl_elev_step", "wl_elev_rollout", "wl_elev_rollout_persistent"

    def __init__(self, n_envs: int, device="cuda:0", params: A.WlElevParams | None = None, seed: int = 42,
                 env_offset: int = 0, heightfield=None, metrics_slots: int = 1, startup=None, terrain_levels: TerrainLevels | None = None,
                 flat_patches=None):
        from .params import elev_params
        super().__init__(n_envs, device, params if params is not None else elev_params(), seed, env_offset, metrics_slots)
        self.set_terrain_levels(terrain_levels)
        self.flat_patches = dict(flat_patches or {})
        self.hf = DeviceHeightField(heightfield if heightfield is not None else synthetic_heightfield(), self.device)
        self.height, self._hf = self.hf.heights, self.hf.struct       # the DECODED fp32 grid (what the kernels see); the ABI struct
        self._args = (C.byref(self._bufs), C.byref(self._hf))
        # startup events (elevation cfg :387-407): wheel friction fixed (2.0, 1.0), base mass += U(0.2, 0.5)
        if startup is None:
            from .envs.flatten import StartupSpec
            startup = StartupSpec(wheel_mu_s=(2.0, 2.0), wheel_mu_d=(1.0, 1.0), mu_buckets=5, mu_consistent=False,
                                  damping=(1000.0, 1000.0), mass_add=(0.2, 0.5))
        apply_startup_events(self.lib, self._bufs, startup, self.seed, self._stream())

    def set_terrain_levels(self, levels: TerrainLevels | None):
        """switch the terrain curriculum on (a TerrainLevels of this batch's envs, on its device) or off (None): the batch's
        params carry the tables from here on (WlElevParams.levels; the struct is this batch's own copy when it changes)"""
        if levels is not None and (levels.level.shape[0] != self.n or levels.device != _canonical_device(self.device)):
            raise ValueError(f"terrain levels of {levels.level.shape[0]} envs on {levels.device} for a batch of {self.n} on {self.device}")
        if levels is not None or self.p.levels.level:
            q = type(self.p)()
            C.pointer(q)[0] = self.p            # a copy: a params struct shared with other batches keeps its own tables
            q.levels = levels.struct if levels is not None else A.WlTerrainLevels()
            self.p = q
        self.levels = levels

    def observe(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """observation of the current state into self.obs (or a caller's [n, 689] buffer)"""
        out = self.obs if out is None else out
        A.check(self.lib.wl_elev_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), out.data_ptr(),
                                         self._stream()), "wl_elev_observe")
        return out

    def collect_rollout(self, actor_critic, storage, start: int = 0, count: int | None = None, deterministic: bool = False):
        """rows start .. start + count - 1 of the storage (and observation row start + count) from observation row `start`: the
        runner's whole collection loop as ONE launch (wl_elev_collect_rollout: the actor's first layer in the blocks' registers,
        their observation rows in LDS, the critic beside the physics).  Quad form only (n <= 32 768)."""
        st = storage
        count = st.n_steps - start if count is None else int(count)
        for k0, k in self._ring_segments(count):
            key = (st.observations.data_ptr(), actor_critic.actor.w1.data_ptr(), actor_critic.critic.w1.data_ptr(), actor_critic.std.data_ptr())
            if getattr(self, "_collect_key", None) != key:
                assert st.n_envs == self.n and st.observations.shape[2] == self.OBS_DIM and st.observations.is_contiguous()
                self._collect_key = key
                self._collect_nets = (actor_critic.actor.struct(), actor_critic.critic.struct())
            a, c = self._collect_nets
            obs, s = st.observations, int(start) + k0
            io = A.WlCollectIo(obs[s].data_ptr(), st.actions[s].data_ptr(), st.mu[s].data_ptr(), st.actions_log_prob[s].data_ptr(),
                               st.values[s].data_ptr())
            out = A.WlStepOut(obs[s + 1].data_ptr(), st.rewards[s].data_ptr(), st.terminated[s].data_ptr(), st.time_outs[s].data_ptr(),
                              st.dones[s].data_ptr())
            A.check(self.lib.wl_elev_collect_rollout(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), C.byref(a), C.byref(c),
                                                     actor_critic.std.data_ptr(), C.byref(io), C.byref(out), k, int(bool(deterministic)),
                                                     self.seed, self.step_count, self._stream()), "wl_elev_collect_rollout")
            self.step_count += k


class VisualBatch(_EnvBatch):
    """n visual-task envs on one GPU: flat black/white traversability plane + ray-cast grey camera."""

    OBS_DIM = A.VIS_OBS_DIM
    OBS_TERM_WIDTHS = (A.VIS_NPIX, 3, 3, 2)      # camera | base_lin_vel | base_ang_vel | last_action
    assert sum(OBS_TERM_WIDTHS) == OBS_DIM
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_visual_reset", "wl_visual_step", "wl_visual_rollout", "wl_visual_rollout_persistent"

    def __init__(self, n_envs: int, device="cuda:0", params=None, seed: int = 42, env_offset: int = 0, trav_map=None,
                 spacing=(0.5, 0.5), metrics_slots: int = 1, startup=None, map_kwargs=None):
        import numpy as np

        from .params import visual_params
        from .travmap import generate_traversability_map, spawn_cells
        super().__init__(n_envs, device, params if params is not None else visual_params(), seed, env_offset, metrics_slots)
        dev = self.device
        if trav_map is None:  # generated at construction from a seeded RNG (the reference uses the global numpy RNG)
            trav_map = generate_traversability_map(rng=np.random.RandomState(self.seed), **(map_kwargs or {}))
        trav_map = np.ascontiguousarray(np.asarray(trav_map, dtype=bool))
        if trav_map.ndim != 2 or trav_map.shape[0] != trav_map.shape[1]:
            # map[y_idx, x_idx] with x clamped to rows - 1 and y to cols - 1 (traversability_utils.py:78-88) only stays inside a
            # square map: the reference raises IndexError past the shorter side, and the kernels refuse such a map
            raise ValueError(f"VisualBatch: the traversability map must be square, got {trav_map.shape}")
        self.trav_map = torch.from_numpy(trav_map.astype(np.uint8)).to(dev)
        self.cells = torch.from_numpy(spawn_cells(trav_map)).contiguous().to(dev)
        # one bit per cell (bit k & 31 of word k >> 5, k = iy * cols + ix): what the camera kernels keep in LDS
        bits = np.packbits(np.concatenate([trav_map.reshape(-1), np.zeros((-trav_map.size) % 32, bool)]), bitorder="little")
        self.trav_bits = torch.from_numpy(bits.view(np.int32).copy()).to(dev)
        self._map = A.WlTravMap(self.trav_map.data_ptr(), self.cells.data_ptr(), trav_map.shape[0], trav_map.shape[1],
                                self.cells.shape[0], float(spacing[0]), float(spacing[1]), self.trav_bits.data_ptr())
        self._args = (C.byref(self._bufs), C.byref(self._map))
        if startup is None:
            from .envs.flatten import StartupSpec
            startup = StartupSpec(wheel_mu_s=(0.5, 0.5), wheel_mu_d=(0.5, 0.5), damping=(1000.0, 1000.0), mass_add=(0.0, 0.0))
        apply_startup_events(self.lib, self._bufs, startup, self.seed, self._stream())

    def sample_augmentation(self, generator: torch.Generator | None = None):
        """one (brightness, contrast, blur sigma) per call, like torchvision's ColorJitter(brightness=.8, contrast=.2)
        and GaussianBlur(5, sigma=(0.1, 5)) on a batched tensor (mdp_sensors/observations.py:21-23)"""
        # ColorJitter.forward: fn_idx = torch.randperm(4) over (brightness, contrast, saturation, hue), then the factors; ONE
        # draw per call, i.e. per batch (the reference passes the whole [B, C, H, W] tensor).  Hue / saturation: see the header.
        order = torch.randperm(4, generator=generator).tolist()
        u = torch.rand(3, generator=generator)
        self.p.brightness = float(0.2 + 1.6 * u[0])
        self.p.contrast = float(0.8 + 0.4 * u[1])
        self.p.blur_sigma = float(0.1 + 4.9 * u[2])
        self.p.contrast_first = int(order.index(1) < order.index(0))

    def observe(self) -> torch.Tensor:
        A.check(self.lib.wl_visual_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._map), self.obs.data_ptr(),
                                           self._stream()), "wl_visual_observe")
        return self.obs

    def depth(self, heightfield, max_depth: float = 20.0, out: torch.Tensor | None = None) -> torch.Tensor:
        """distance_to_image_plane of the camera against a heightfield -> [n, 60, 80] (BASELINE config 5); `heightfield` is
        (height [ny, nx], x0, y0, cell) or a DepthCamera (build it once when rendering every step)"""
        cam = heightfield if isinstance(heightfield, DepthCamera) else _cached_depth_camera(self, heightfield)
        return cam.render(self, max_depth, out)


class VisualDepthBatch(VisualBatch):
    """n envs of the visual-DEPTH extension task (BASELINE.json configs[4]; not a reference id): the visual task's step driven on a
    heightfield terrain with the camera's 60 x 80 depth image as the observation -- obs [n, 4808] = distance_to_image_plane |
    base_lin_vel | base_ang_vel | last_action.  Two launches per env.step(): the step (wl_visual_step_hf: lane or quad of lanes
    = env, HeightFieldGround contacts) and the depth ray-cast (wl_visual_depth_rows).  `heightfield`: (height [ny, nx], x0, y0,
    cell), default the synthetic 800 x 800 terrain; the traversability map should cover it (default: an 80 x 80 map of 0.5 m
    cells = the terrain's 40 m square, generated like the reference's from the seed)."""

    OBS_DIM = A.VISDEPTH_OBS_DIM
    OBS_TERM_WIDTHS = (A.VISDEPTH_NPIX, 3, 3, 2)      # depth | base_lin_vel | base_ang_vel | last_action
    assert sum(OBS_TERM_WIDTHS) == OBS_DIM
    _C_RESET = "wl_visual_reset_hf"

    def __init__(self, n_envs: int, device="cuda:0", params=None, seed: int = 42, env_offset: int = 0, trav_map=None,
                 spacing=(0.5, 0.5), metrics_slots: int = 1, startup=None, map_kwargs=None, heightfield=None, max_depth: float = 20.0):
        if trav_map is None and map_kwargs is None:
            map_kwargs = dict(map_size=(80, 80), env_size=(40, 40), sub_group_size=(20, 20), num_walkers=1)
        super().__init__(n_envs, device, params, seed, env_offset, trav_map, spacing, metrics_slots, startup, map_kwargs)
        self.hf = DeviceHeightField(heightfield if heightfield is not None else synthetic_heightfield(), self.device)
        self.height = self.hf.heights
        self.max_depth = float(max_depth)
        self.camera = DepthCamera(self.hf, self.device, self.p)
        self._hf, self._pyr = self.camera._hf, self.camera._pyr
        self._args = (C.byref(self._bufs), C.byref(self._map), C.byref(self._hf))

    def observe(self, out: torch.Tensor | None = None) -> torch.Tensor:
        out = self.obs if out is None else out
        A.check(self.lib.wl_visual_depth_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), self._pyr,
                                                 self.max_depth, out.data_ptr(), self._stream()), "wl_visual_depth_observe")
        return out

    def sample_augmentation(self, generator=None):
        """the depth image is not augmented (mdp_sensors/observations.py:93-95 returns the raw distances)"""

    def step(self, actions: torch.Tensor):
        self._step_into(self._actions(actions).data_ptr(), self._out)
        return self.obs, self.reward, self.terminated, self.truncated

    def _step_into(self, actions_ptr, out):
        A.check(self.lib.wl_visual_depth_step(C.byref(self.p), *self._args, self._pyr, self.max_depth, actions_ptr,
                                              C.byref(out), self.seed, self.step_count, self._stream()), "wl_visual_depth_step")
        self.step_count += 1

    def rollout(self, actions: torch.Tensor, obs_out=None, rew_out=None, term_out=None, trunc_out=None, dones_out=None,
                persistent: bool = False):
        """K steps with pre-staged actions [K, n, 2]; optional [K, ...] output storage (else overwritten in place)"""
        K = actions.shape[0]
        assert actions.shape == (K, self.n, 2) and actions.dtype == torch.float32 and actions.is_contiguous() and not persistent
        for k in range(K):
            out = self._out if obs_out is None else A.WlStepOut(obs_out[k].data_ptr(), rew_out[k].data_ptr(), term_out[k].data_ptr(),
                                                                trunc_out[k].data_ptr(), None if dones_out is None else dones_out[k].data_ptr())
            self._step_into(actions[k].data_ptr(), out)

    def depth(self, heightfield=None, max_depth: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """the task's own terrain unless another heightfield is given"""
        if heightfield is None:
            return self.camera.render(self, self.max_depth if max_depth is None else max_depth, out)
        return super().depth(heightfield, 20.0 if max_depth is None else max_depth, out)

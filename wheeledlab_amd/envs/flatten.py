"""Flatten a manager-based env config into the POD parameter struct of the fused kernel (SURVEY.md section 5 "config /
flags": "a flattening step that turns term cfgs into a POD params struct for the kernel").  Unknown term functions
are not silently dropped: custom reward terms are returned for post-kernel evaluation on the device, anything else
that the kernel cannot express raises."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

from .. import _abi as A
from ..params import MUSHR_CHASSIS_MASS, mushr_vehicle
from .configclass import fields_of
from . import corruption
from . import events as event_rand
from . import latency as action_latency

INT_MAX = 2 ** 31 - 1


@dataclass
class StartupSpec:
    """startup-mode events (domain randomisation applied once at construction)"""
    wheel_mu_s: tuple = (0.4, 0.4)
    wheel_mu_d: tuple = (0.4, 0.4)
    mu_buckets: int = 1
    mu_consistent: bool = True
    damping: tuple = (30.0, 30.0)
    mass_add: tuple = (0.0, 0.0)
    wheel_mass: tuple = (0.0, 0.0)      # each wheel link's mass ("abs"); (0, 0): wheels counted in chassis_mass
    chassis_mass: float = MUSHR_CHASSIS_MASS
    track_radius: float = 0.8
    track_straight: float = 0.8
    throttle_damping: float = 30.0      # the asset's throttle DCMotorCfg.damping / stiffness: what a reset / interval gain term applies
    throttle_stiffness: float = 0.0     # its operation to, and the one stiffness it may name (envs/events.py)


@dataclass
class FlatDriftCfg:
    params: A.WlDriftParams
    startup: StartupSpec
    reward_names: list = field(default_factory=list)        # [(cfg name, slot)]
    custom_rewards: list = field(default_factory=list)      # [(name, term_cfg)] evaluated with torch after the kernel
    custom_terminations: list = field(default_factory=list) # [(name, term_cfg)] torch, on the post-step state views
    custom_obs: list = field(default_factory=list)          # [(name, term_cfg)] torch, concatenated after the fused block
    termination_names: dict = field(default_factory=dict)   # {"time_out": name, 0: name}
    curriculum: list = field(default_factory=list)          # [(name, term_cfg)]
    obs_dim: int = 14
    task: str = "drift"
    extra: dict = field(default_factory=dict)
    corruption: bool = False                                # the corruption layer is built (envs/corruption.py): the step writes the clean row
    events: object = None                                   # envs/events.EventTable of the reset / interval randomisation terms, or None
    latency: object = None                                  # envs/latency.LatencySpec of the action term's latency, or None


def _terms(cfg):
    return [] if cfg is None else [(k, v) for k, v in fields_of(cfg) if hasattr(v, "func")]


def flatten_drift_cfg(cfg) -> FlatDriftCfg:
    p = A.WlDriftParams()
    su = StartupSpec()
    flat = FlatDriftCfg(p, su)
    p.sim_dt, p.decimation = float(cfg.sim.dt), int(cfg.decimation)
    step_dt = float(cfg.sim.dt) * int(cfg.decimation)   # python doubles, exactly as IsaacLab computes max_episode_length
    p.max_episode_length = math.ceil(cfg.episode_length_s / step_dt)

    # ---- action term ----
    act_terms = _named(cfg.actions)
    if len(act_terms) != 1:
        raise NotImplementedError("exactly one action term (throttle_steer) is supported")
    acfg = act_terms[0][1]
    if getattr(acfg.class_type, "wl_map", None) is None:
        raise NotImplementedError(f"action term {acfg.class_type.__name__} has no HIP implementation")
    a = p.action
    a.scale[0], a.scale[1] = acfg.scale
    a.offset[0], a.offset[1] = acfg.offset
    a.bounding = {"clip": 1, "tanh": 2, None: 0}[acfg.bounding_strategy]
    a.no_reverse, a.clip_wrapper, a.map = int(acfg.no_reverse), 0, acfg.class_type.wl_map
    a.base_length, a.base_width, a.wheel_radius = acfg.base_length, acfg.base_width, acfg.wheel_radius

    # ---- vehicle: actuator constants from the robot cfg, friction from the terrain material ----
    robot = cfg.scene.robot
    acts = robot.actuators
    thr = acts["throttle_joints"]
    rwd = "passive_joints" in acts or any(e.startswith("back_") for e in thr.joint_names_expr)
    mat = cfg.scene.terrain.physics_material
    if mat.friction_combine_mode != "multiply":
        raise NotImplementedError("only the 'multiply' friction combine mode is modelled")
    substeps = max(1, math.ceil(float(cfg.sim.dt) / 0.0101))
    p.vehicle = mushr_vehicle(drive=0 if rwd else 1, motor_limit=float(thr.effort_limit), substeps=substeps,
                              ground_mu=(mat.static_friction, mat.dynamic_friction))
    v = p.vehicle
    v.motor_sat, v.motor_vel_limit = float(thr.saturation_effort), float(thr.velocity_limit)
    st = acts["steering_joints"]
    v.steer_kp, v.steer_kd, v.steer_effort, v.steer_vel_limit = st.stiffness, st.damping, st.effort_limit, st.velocity_limit
    v.half_wheelbase_f = v.half_wheelbase_r = acfg.base_length / 2
    v.half_track = acfg.base_width / 2
    v.wheel_radius = acfg.wheel_radius
    su.damping = (float(thr.damping),) * 2
    su.throttle_damping, su.throttle_stiffness = float(thr.damping), float(thr.stiffness or 0.0)

    # ---- rewards ----
    for i in range(A.WL_MAX_REW_TERMS):
        p.weight[i] = 0.0
    # kernel defaults so that disabled terms stay finite
    p.straight, p.r_in, p.r_out, p.r_line = 0.8, 0.0, 1e30, 0.8   # r_in is squared in-kernel: 0 disables it
    p.slip_min, p.slip_max, p.slip_min_vx = 0.25, 0.55, 0.5
    p.speed_target, p.speed_offset, p.tlgr_thresh, p.ctd_offset, p.ctd_p = 3.0, -9.0, math.pi / 4, -1.0, 1.0
    straight_seen = {}
    for name, term in _terms(cfg.rewards):
        f = term.func
        if getattr(f, "wl_kind", None) != "reward":
            flat.custom_rewards.append((name, term))
            continue
        p.weight[f.wl_slot] = float(term.weight)
        flat.reward_names.append((name, f.wl_slot))
        _apply_params(p, f, term.params, straight_seen, name)

    # ---- terminations ----
    has_timeout = False
    for name, term in _terms(cfg.terminations):
        f = term.func
        if getattr(f, "wl_kind", None) != "termination":   # any f(env, **params) -> bool[N]: torch fallback on the state views
            flat.custom_terminations.append((name, term))
            continue
        if f.wl_slot == "time_out":
            if not term.time_out:
                raise NotImplementedError("mdp.time_out must be registered with time_out=True")
            has_timeout = True
        else:
            _apply_params(p, f, term.params, straight_seen, name)
        flat.termination_names[f.wl_slot] = name
    if not has_timeout:
        p.max_episode_length = INT_MAX

    # ---- observations: the built-in 14-dim layout ----
    pol = cfg.observations.policy
    obs_terms = _terms(pol)
    want = ["root_pos_w", "root_euler_xyz", "base_lin_vel", "base_ang_vel", "last_action"]
    got = [getattr(t.func, "__name__", str(t.func)) for _, t in obs_terms]
    if got[:len(want)] != want:
        raise NotImplementedError(f"the policy observation must start with the fused kernel's layout {want} (got {got}); "
                                  "further terms are evaluated with torch and concatenated behind it")
    flat.custom_obs = obs_terms[len(want):]
    # what the step cannot draw itself (uniform noise, a mean, a noise model, noise on last_action, clip / scale on the
    # proprioceptive terms) is the corruption layer's (envs/corruption.py): the step then writes the CLEAN row
    corruption.normalise(obs_terms)
    flat.corruption = corruption.needed(pol, obs_terms, "drift")
    p.enable_corruption = 0 if flat.corruption else int(bool(pol.enable_corruption))
    for i, (_, t) in enumerate(obs_terms[:4]):
        p.noise_std[i] = 0.0 if flat.corruption or t.noise is None else float(t.noise.std)
    if tuple(obs_terms[4][1].clip or ()) != (-1.0, 1.0):
        raise NotImplementedError("last_action must be clipped to (-1, 1) (common/observations.py:52)")

    # ---- events ----
    p.num_ref_points, p.pos_noise, p.yaw_noise = 20, 0.0, 0.0
    p.enable_pushes = 0
    p.hf_interval[0], p.hf_interval[1], p.lf_interval[0], p.lf_interval[1] = 1e9, 1e9, 1e9, 1e9
    p.hf_vel_x = p.hf_vel_y = p.hf_vel_yaw = p.lf_vel_yaw = 0.0
    pushes = []
    for name, term in _terms(cfg.events):
        ev = getattr(term.func, "wl_event", None)
        pr = term.params
        if ev == "reset_along_track" and term.mode == "reset":
            p.num_ref_points = int(pr.get("num_points", 20))
            p.pos_noise, p.yaw_noise = float(pr.get("pos_noise", 0.0)), float(pr.get("yaw_noise", 0.0))
            su.track_radius = float(pr.get("track_radius", 0.8))
            su.track_straight = float(pr.get("track_straight_dist", 0.8))
        elif ev == "wheel_friction" and term.mode == "startup":
            su.wheel_mu_s, su.wheel_mu_d = tuple(pr["static_friction_range"]), tuple(pr["dynamic_friction_range"])
            su.mu_buckets, su.mu_consistent = int(pr["num_buckets"]), bool(pr.get("make_consistent", False))
        elif ev == "actuator_gains" and term.mode == "startup":
            if pr.get("operation", "abs") != "abs":
                raise NotImplementedError("randomize_actuator_gains: only operation='abs'")
            su.damping = tuple(pr["damping_distribution_params"])
        elif ev == "base_mass" and term.mode == "startup":
            if pr.get("operation", "add") != "add":
                raise NotImplementedError("randomize_rigid_body_mass: only operation='add'")
            su.mass_add = tuple(pr["mass_distribution_params"])
        elif ev == "push" and term.mode == "interval":
            pushes.append((name, term))
        elif event_rand.is_episodic(term):      # friction / gains / mass per episode: the layer between steps (envs/events.py)
            continue
        else:
            raise NotImplementedError(f"event term '{name}' ({getattr(term.func, '__name__', term.func)}, mode {term.mode}) "
                                      "has no HIP implementation")
    if len(pushes) > 2:
        raise NotImplementedError("at most two interval push events are fused")
    for slot, (name, term) in enumerate(pushes):
        vr = {k: tuple(v) for k, v in term.params["velocity_range"].items()}
        for k, (lo, hi) in vr.items():
            if abs(lo + hi) > 1e-9:
                raise NotImplementedError(f"push '{name}': only symmetric ranges are fused")
        lo_s, hi_s = term.interval_range_s
        if slot == 0:
            if set(vr) - {"x", "y", "yaw"}:
                raise NotImplementedError(f"push '{name}': only x / y / yaw components are fused")
            p.hf_interval[0], p.hf_interval[1] = lo_s, hi_s
            p.hf_vel_x, p.hf_vel_y, p.hf_vel_yaw = (vr.get(k, (0, 0))[1] for k in ("x", "y", "yaw"))
        else:
            if set(vr) - {"yaw"}:
                raise NotImplementedError(f"push '{name}': the second interval event is yaw-only in the fused kernel")
            p.lf_interval[0], p.lf_interval[1] = lo_s, hi_s
            p.lf_vel_yaw = vr.get("yaw", (0, 0))[1]
        p.enable_pushes = 1
    if p.num_ref_points > 32:
        raise NotImplementedError("at most 32 reference poses")
    flat.events = event_rand.resolve(cfg.events, su, "drift")
    flat.latency = action_latency.resolve(cfg.actions)

    flat.curriculum = _terms(cfg.curriculum)
    p.log_episode_sums = 1
    return flat


def _named(cfg):
    return [(k, v) for k, v in fields_of(cfg) if hasattr(v, "class_type")]


def _apply_params(p, func, params, straight_seen, name):
    for key, fld in func.wl_params.items():
        if key not in params:
            continue
        val = float(params[key])
        if fld in ("straight",):  # shared by several terms: they must agree (they do in the reference, STRAIGHT = 0.8)
            if fld in straight_seen and abs(straight_seen[fld] - val) > 1e-9:
                raise NotImplementedError(f"term '{name}': '{key}'={val} conflicts with {straight_seen[fld]} of another term")
            straight_seen[fld] = val
        setattr(p, fld, val)


# =====================================================================================================================
# elevation / visual tasks
# =====================================================================================================================

@dataclass
class FlatTaskCfg:
    task: str
    params: object
    startup: StartupSpec
    reward_names: list = field(default_factory=list)
    custom_rewards: list = field(default_factory=list)
    custom_terminations: list = field(default_factory=list)
    custom_obs: list = field(default_factory=list)
    termination_names: dict = field(default_factory=dict)
    curriculum: list = field(default_factory=list)
    obs_dim: int = 0
    extra: dict = field(default_factory=dict)
    corruption: bool = False
    events: object = None                                   # as FlatDriftCfg.events
    latency: object = None                                  # as FlatDriftCfg.latency


def _common_vehicle(cfg, p, acfg):
    robot = cfg.scene.robot
    acts = robot.actuators
    thr = acts["throttle_joints"]
    rwd = "passive_joints" in acts or any(e.startswith("back_") for e in thr.joint_names_expr)
    mat = cfg.scene.terrain.physics_material
    if mat.friction_combine_mode != "multiply":
        raise NotImplementedError("only the 'multiply' friction combine mode is modelled")
    # the linearly implicit integrator steps once per sim.dt (the reference's physics rate) up to h = 20 ms, its validated range
    substeps = max(1, math.ceil(float(cfg.sim.dt) / 0.0201))
    p.vehicle = mushr_vehicle(drive=0 if rwd else 1, motor_limit=float(thr.effort_limit), substeps=substeps,
                              ground_mu=(mat.static_friction, mat.dynamic_friction), implicit=1)
    v = p.vehicle
    v.motor_sat, v.motor_vel_limit = float(thr.saturation_effort), float(thr.velocity_limit)
    st = acts["steering_joints"]
    v.steer_kp, v.steer_kd, v.steer_effort, v.steer_vel_limit = st.stiffness, st.damping, st.effort_limit, st.velocity_limit
    v.half_wheelbase_f = v.half_wheelbase_r = acfg.base_length / 2
    v.half_track = acfg.base_width / 2
    v.wheel_radius = acfg.wheel_radius
    return float(thr.damping)


def _action(cfg, p):
    act_terms = _named(cfg.actions)
    if len(act_terms) != 1 or getattr(act_terms[0][1].class_type, "wl_map", None) is None:
        raise NotImplementedError("exactly one RCCarRWD / RCCar4WD action term is supported")
    acfg = act_terms[0][1]
    a = p.action
    a.scale[0], a.scale[1] = acfg.scale
    a.offset[0], a.offset[1] = acfg.offset
    a.bounding = {"clip": 1, "tanh": 2, None: 0}[acfg.bounding_strategy]
    a.no_reverse, a.clip_wrapper, a.map = int(acfg.no_reverse), 0, acfg.class_type.wl_map
    a.base_length, a.base_width, a.wheel_radius = acfg.base_length, acfg.base_width, acfg.wheel_radius
    return acfg


def _startup_events(cfg, su, allowed_reset):
    reset_term = None
    for name, term in _terms(cfg.events):
        ev = getattr(term.func, "wl_event", None)
        pr = term.params
        if ev in allowed_reset and term.mode == "reset":
            reset_term = term
        elif ev == "wheel_friction" and term.mode == "startup":
            su.wheel_mu_s, su.wheel_mu_d = tuple(pr["static_friction_range"]), tuple(pr["dynamic_friction_range"])
            su.mu_buckets, su.mu_consistent = int(pr["num_buckets"]), bool(pr.get("make_consistent", False))
        elif ev == "base_mass" and term.mode == "startup" and "wheel" in str(getattr(pr.get("asset_cfg"), "body_names", "")):
            # randomize_rigid_body_mass on the wheel links (visual/mushr_visual_env_cfg.py:289-298): the four link masses add to the
            # vehicle's mass row; the wheels' ROTATIONAL inertia stays the model's one `wheel_inertia` (not randomised per wheel)
            if pr.get("operation", "add") != "abs":
                raise NotImplementedError("randomize_rigid_body_mass on the wheel links: operation abs")
            su.wheel_mass = tuple(pr["mass_distribution_params"])
        elif ev == "base_mass" and term.mode == "startup":
            if pr.get("operation", "add") == "add":
                su.mass_add = tuple(pr["mass_distribution_params"])
            elif pr["operation"] == "abs":
                su.chassis_mass, su.mass_add = 0.0, tuple(pr["mass_distribution_params"])
            else:
                raise NotImplementedError("randomize_rigid_body_mass: operation add / abs")
        elif ev == "actuator_gains" and term.mode == "startup":
            su.damping = tuple(pr["damping_distribution_params"])
        elif event_rand.is_episodic(term):      # friction / gains / mass per episode: the layer between steps (envs/events.py)
            continue
        else:
            raise NotImplementedError(f"event term '{name}' ({getattr(term.func, '__name__', term.func)}, mode {term.mode}) "
                                      "has no HIP implementation for this task")
    return reset_term


def _sym(rng, what):
    lo, hi = rng
    if abs(lo + hi) > 1e-9:
        raise NotImplementedError(f"{what}: only symmetric ranges are fused")
    return float(hi)


def flatten_elev_cfg(cfg) -> FlatTaskCfg:
    """MushrElevationRLEnvCfg-shaped config -> WlElevParams (reference: elevation/mushr_elevation_env_cfg.py)"""
    from ..params import elev_params
    from . import mdp
    p = elev_params()                                   # term constants that have no config field keep the reference values
    su = StartupSpec(wheel_mu_s=(2.0, 2.0), wheel_mu_d=(1.0, 1.0), mass_add=(0.0, 0.0))
    flat = FlatTaskCfg("elevation", p, su, obs_dim=A.ELEV_OBS_DIM)
    p.sim_dt, p.decimation = float(cfg.sim.dt), int(cfg.decimation)
    p.max_episode_length = math.ceil(cfg.episode_length_s / (float(cfg.sim.dt) * int(cfg.decimation)))
    acfg = _action(cfg, p)
    su.damping = (_common_vehicle(cfg, p, acfg),) * 2
    su.throttle_damping, su.throttle_stiffness = su.damping[0], float(cfg.scene.robot.actuators["throttle_joints"].stiffness or 0.0)
    for i in range(A.WL_MAX_REW_TERMS):
        p.weight[i] = 0.0
    for name, term in _terms(cfg.rewards):
        f = term.func
        if f is mdp.is_terminated_term:
            if term.params.get("term_keys") not in ("stuck", ["stuck"]):
                raise NotImplementedError("is_terminated_term is fused for term_keys='stuck' (:301-305)")
            slot = 3
        elif getattr(f, "wl_kind", None) == "reward" and f in (mdp.goal_progress_rate, mdp.higher_elevation, mdp.is_falling_penalty):
            slot = f.wl_slot
            for key, fld in f.wl_params.items():
                if key in term.params:
                    setattr(p, fld, float(term.params[key]))
        else:
            flat.custom_rewards.append((name, term))
            continue
        p.weight[slot] = float(term.weight)
        flat.reward_names.append((name, slot))
    has_timeout = False
    p.min_height, p.goal_dist, p.upright_cos = -1e30, -1.0, -2.0      # disabled unless the cfg registers the term
    p.stuck_min_vel, p.stuck_wheel_spin = -1e30, 1e30
    for name, term in _terms(cfg.terminations):
        f = term.func
        if f is mdp.time_out:
            has_timeout = True
            flat.termination_names["time_out"] = name
            continue
        if getattr(f, "wl_kind", None) != "termination" or f not in (mdp.root_height_below_minimum, mdp.stuck, mdp.upright_bool, mdp.close_to_goal):
            flat.custom_terminations.append((name, term))     # torch fallback on the state views
            continue
        for key, fld in f.wl_params.items():
            val = float(term.params[key])
            setattr(p, fld, math.cos(math.radians(val)) if fld == "upright_cos" else val)
        flat.termination_names[f.wl_slot] = name
    if not has_timeout:
        p.max_episode_length = INT_MAX
    # observation layout
    want = ["goal_relative_xyz", "root_euler_xyz", "base_lin_vel", "base_ang_vel", "last_action", "world_height_map"]
    obs_terms = _terms(cfg.observations.policy)
    got = [getattr(t.func, "__name__", str(t.func)) for _, t in obs_terms]
    if got[:len(want)] != want:
        raise NotImplementedError(f"the policy observation must start with the fused kernel's layout {want}; got {got}")
    corruption.normalise(obs_terms)
    flat.corruption = corruption.needed(cfg.observations.policy, obs_terms, "elevation")      # the step itself draws no noise
    flat.custom_obs = obs_terms[len(want):]
    hm = obs_terms[5][1]
    p.scan_offset, p.elev_z0 = float(hm.params.get("offset", 0.084)), float(hm.params.get("plane_init_value", 0.19))
    p.obs_clip = float(hm.clip[1])
    if tuple(obs_terms[2][1].clip) != (-p.obs_clip, p.obs_clip) or tuple(obs_terms[3][1].clip) != (-p.obs_clip, p.obs_clip):
        raise NotImplementedError("velocity clips must equal the height-map clip (10)")
    pat = cfg.scene.height_scanner.pattern_cfg
    p.scan_size, p.scan_res = float(pat.size[0]), float(pat.resolution)
    if round(p.scan_size / p.scan_res) + 1 != A.ELEV_SCAN_N or pat.size[0] != pat.size[1]:
        raise NotImplementedError(f"the fused height scan is {A.ELEV_SCAN_N} x {A.ELEV_SCAN_N} rays")
    # events + command
    for name, term in _terms(cfg.events):     # an event by name (a command-line override): mdp.<name> must be an event term
        if isinstance(term.func, str):
            if getattr(getattr(mdp, term.func, None), "wl_event", None) is None:
                raise ValueError(f"events.{name}.func = '{term.func}': not an event term of wheeledlab_amd.envs.mdp")
            term.func = getattr(mdp, term.func)
    rt = _startup_events(cfg, su, ("reset_uniform", "reset_from_terrain"))
    flat.events = event_rand.resolve(cfg.events, su, "elevation")
    flat.latency = action_latency.resolve(cfg.actions)
    from_terrain = rt is not None and getattr(rt.func, "wl_event", None) == "reset_from_terrain"
    if rt is not None:
        pr, vr = rt.params["pose_range"], rt.params["velocity_range"]
        # (from the terrain: the patch is the position; a pose_range without x / y spawns ON it)
        px, py = (pr.get("x", (0.0, 0.0)), pr.get("y", pr.get("x", (0.0, 0.0)))) if from_terrain else (pr["x"], pr["y"])
        p.reset_xy, p.reset_yaw = _sym(px, "reset x"), _sym(pr.get("yaw", (0.0, 0.0)) if from_terrain else pr["yaw"], "reset yaw")
        if tuple(px) != tuple(py) or tuple(vr["x"]) != tuple(vr["y"]):
            raise NotImplementedError("reset ranges must be equal in x and y")
        p.reset_vel[0], p.reset_vel[1] = vr["x"]
    p.reset_z = float(cfg.scene.terrain.height)
    cmd = cfg.commands.goal_pose
    p.cmd_xy, p.cmd_heading = _sym(cmd.ranges.pos_x, "command x"), _sym(cmd.ranges.heading, "command heading")
    p.cmd_resample_s = float(cmd.resampling_time_range[1])
    # the terrain_levels term is the kernels' own (WlElevParams.levels): it runs inside every step, not at curriculum boundaries
    slot = getattr(cfg.curriculum, "terrain_levels", None)
    if isinstance(slot, str):                 # the term by name (a command-line override): mdp.<name> must be the levels term
        if getattr(mdp, slot, None) is not mdp.terrain_levels_goal:
            raise ValueError(f"curriculum.terrain_levels = '{slot}': the terrain-levels term is 'terrain_levels_goal'")
        from .managers_cfg import CurriculumTermCfg
        cfg.curriculum.terrain_levels = CurriculumTermCfg(func=mdp.terrain_levels_goal)
    terms = _terms(cfg.curriculum)
    level_terms = [name for name, term in terms if term.func is mdp.terrain_levels_goal]
    flat.curriculum = [(name, term) for name, term in terms if term.func is not mdp.terrain_levels_goal]
    flat.extra.update(_terrain_source(cfg.scene.terrain, reset_range=None if level_terms or from_terrain else (-p.reset_xy, p.reset_xy)))
    if level_terms:
        from .terrain_levels import check_curriculum
        check_curriculum(flat.extra["terrain_generator"], p.reset_xy, p.cmd_xy)
        flat.extra["terrain_levels"] = dict(name=level_terms[0], max_init_terrain_level=getattr(cfg.scene.terrain, "max_init_terrain_level", None))
    flat.extra["flat_patches"] = _flat_patch_source(cfg.scene.terrain, flat.extra["terrain_generator"], from_terrain, p.reset_xy, p.cmd_xy)
    return flat


def _flat_patch_source(t, gen, from_terrain: bool, reset_xy: float, cmd_xy: float):
    """The flat patches of an elevation scene: None, or dict(names, sampling, spawn) -- `names` every set to find (a generator's and
    its sub-terrains' flat_patch_sampling; scene.terrain.flat_patch_sampling on a field that was not generated), `sampling` the
    latter's {name: FlatPatchSamplingCfg}, `spawn` whether resets use "init_pos" (mdp.reset_root_state_from_terrain).  A spawn must
    stay on its patch and the goal square about every possible patch on the lattice: each failure a ValueError naming the quantity."""
    from . import terrain_gen_cfg as G
    own = getattr(t, "flat_patch_sampling", None)
    if gen is not None:
        if own:
            raise ValueError("scene.terrain.flat_patch_sampling is for height arrays and meshes: a generated terrain takes "
                             "flat_patch_sampling on its TerrainGeneratorCfg or its sub-terrains")
        names, sampling = G.patch_names(gen), None
    else:
        sampling = {k: G.as_patch_cfg(v) for k, v in (own or {}).items()}
        names = sorted(sampling)
    if from_terrain and "init_pos" not in names:
        raise ValueError('reset_root_state_from_terrain needs "init_pos" flat patches: set flat_patch_sampling = {"init_pos": '
                         "FlatPatchSamplingCfg(...)} on the terrain generator, a sub-terrain or scene.terrain")
    if not names:
        return None
    if from_terrain:
        if gen is not None:
            table, _, _, _ = G.patch_table(gen, "init_pos")
            subs, default = G.tile_names(gen), (gen.flat_patch_sampling or {}).get("init_pos")
            radii = [G.patch_radius(G.as_patch_cfg(c)) for c in ((gen.sub_terrains[s].flat_patch_sampling or {}).get("init_pos") or default for s in subs)
                     if c is not None]
            geo = G.lattice(gen)
            check_patch_goals(table, geo["nx"], geo["ny"], geo["cell"], cmd_xy)
        else:
            radii = [G.patch_radius(sampling["init_pos"])]
        if math.sqrt(2.0) * float(reset_xy) > min(radii) + 1e-9:
            raise ValueError(f"reset_xy {float(reset_xy):g} m: the corner of the spawn square, {math.sqrt(2.0) * float(reset_xy):g} m from the patch's "
                             f"centre, leaves the patch (patch_radius {min(radii):g} m): lower pose_range x / y or raise patch_radius")
    return dict(names=names, sampling=sampling, spawn=bool(from_terrain))


def check_patch_goals(table, nx: int, ny: int, cell: float, cmd_xy: float):
    """ValueError unless the goal square (+-cmd_xy) about every point of every window of `table` stays on the lattice -- the
    one-point windows of tiles without a sampling included: cars spawn at their centre and draw goals about it"""
    searched = table
    for axis, lo, hi, n in (("x", "i_lo", "i_hi", nx), ("y", "j_lo", "j_hi", ny)):
        if searched[lo].min() * cell - float(cmd_xy) < -1e-9 or searched[hi].max() * cell + float(cmd_xy) > (n - 1) * cell + 1e-9:
            raise ValueError(f"cmd_xy {float(cmd_xy):g} m: the goal square about an outer flat patch leaves the lattice in {axis} (patch centres "
                             f"span points {int(searched[lo].min())} .. {int(searched[hi].max())} of {n} at {cell:g} m): lower it, narrow "
                             f"{axis}_range or widen border_width")


def _terrain_source(t, reset_range=None, reset_range_y=None) -> dict:
    """the terrain of a heightfield task: `heightfield` (an array), `mesh_path` (an OBJ rasterised at `mesh_cell`), a procedural
    terrain (`terrain_type = "generator"` with `terrain_generator` a TerrainGeneratorCfg, generated on the device), or none of
    them (the synthetic field) -- never two.  `reset_range` (lo, hi) in metres (x; y: `reset_range_y` or the same): where the task
    puts cars at reset, which a generated terrain must cover."""
    hf, mesh = getattr(t, "heightfield", None), getattr(t, "mesh_path", None)
    if hf is not None and mesh is not None:
        raise ValueError("scene.terrain: set `heightfield` or `mesh_path`, not both")
    cell = float(getattr(t, "mesh_cell", 0.05))
    if mesh is not None and not (math.isfinite(cell) and cell > 0):
        raise ValueError("scene.terrain.mesh_cell must be positive and finite")
    gen = None
    if getattr(t, "terrain_type", None) != "generator" and getattr(t, "terrain_generator", None) is not None:
        raise ValueError('scene.terrain.terrain_generator is set but terrain_type is not "generator": set terrain_type = "generator" '
                         "to drive on the generated terrain, or leave terrain_generator None")
    if getattr(t, "terrain_type", None) == "generator":
        gen = getattr(t, "terrain_generator", None)
        if gen is None:
            raise ValueError('scene.terrain.terrain_type = "generator" needs scene.terrain.terrain_generator (a TerrainGeneratorCfg)')
        if hf is not None or mesh is not None:
            raise ValueError('scene.terrain: terrain_type = "generator" excludes `heightfield` and `mesh_path`')
        from .terrain_gen_cfg import TerrainGeneratorCfg, check_covers, tile_table
        if isinstance(gen, dict):                           # a command-line override: the fields that differ from the defaults
            gen = TerrainGeneratorCfg(**gen)
        tile_table(gen)                                     # a config that does not resolve fails here, before any device work
        if reset_range is not None:
            check_covers(gen, reset_range, reset_range_y)
    return dict(heightfield=hf, mesh_path=None if mesh is None else str(mesh), mesh_cell=cell, terrain_generator=gen)


def flatten_visual_cfg(cfg) -> FlatTaskCfg:
    """MushrVisualRLEnvCfg-shaped config -> WlVisualParams (reference: visual/mushr_visual_env_cfg.py)"""
    from ..params import visual_params
    from . import mdp
    p = visual_params()
    su = StartupSpec(wheel_mu_s=(0.5, 0.5), wheel_mu_d=(0.5, 0.5), mass_add=(0.0, 0.0))   # PhysX default material
    flat = FlatTaskCfg("visual", p, su, obs_dim=A.VIS_OBS_DIM)
    p.sim_dt, p.decimation = float(cfg.sim.dt), int(cfg.decimation)
    p.max_episode_length = math.ceil(cfg.episode_length_s / (float(cfg.sim.dt) * int(cfg.decimation)))
    acfg = _action(cfg, p)
    su.damping = (_common_vehicle(cfg, p, acfg),) * 2
    su.throttle_damping, su.throttle_stiffness = su.damping[0], float(cfg.scene.robot.actuators["throttle_joints"].stiffness or 0.0)
    for i in range(A.WL_MAX_REW_TERMS):
        p.weight[i] = 0.0
    for name, term in _terms(cfg.rewards):
        if term.func is mdp.traversable_reward:
            slot = 0
        elif term.func is mdp.forward_vel:
            slot = 1
        else:
            flat.custom_rewards.append((name, term))
            continue
        p.weight[slot] = float(term.weight)
        flat.reward_names.append((name, slot))
    has_timeout, has_oom = False, False
    for name, term in _terms(cfg.terminations):
        if term.func is mdp.time_out:
            has_timeout = True
            flat.termination_names["time_out"] = name
        elif term.func is mdp.out_of_map:
            has_oom = True
            flat.termination_names[0] = name
        else:
            flat.custom_terminations.append((name, term))     # torch fallback on the state views
    if not has_timeout:
        p.max_episode_length = INT_MAX
    flat.extra["out_of_map"] = has_oom
    depth_task = getattr(cfg, "wl_task", "visual") == "visual_depth"
    want = ["raycast_depth" if depth_task else "camera_data_rgb_flattened_aug", "base_lin_vel", "base_ang_vel", "last_action"]
    vis_obs = _terms(cfg.observations.policy)
    got = [getattr(t.func, "__name__", str(t.func)) for _, t in vis_obs]
    if got[:len(want)] != want:
        raise NotImplementedError(f"the policy observation must start with the fused kernel's layout {want}; got {got}")
    corruption.normalise(vis_obs)
    flat.corruption = corruption.needed(cfg.observations.policy, vis_obs, "visual_depth" if depth_task else "visual")
    flat.custom_obs = vis_obs[len(want):]
    cam = cfg.scene.camera
    if (cam.height, cam.width) != (60, 80):
        raise NotImplementedError("the fused camera is 60 x 80")
    p.fx = cam.width * cam.spawn.focal_length / cam.spawn.horizontal_aperture
    p.fy = cam.height * cam.spawn.focal_length / cam.spawn.vertical_aperture
    p.cx, p.cy = cam.width / 2, cam.height / 2
    p.cam_pos[0], p.cam_pos[1], p.cam_pos[2] = cam.body_pos
    _startup_events(cfg, su, ("reset_traversable",))
    flat.events = event_rand.resolve(cfg.events, su, flat.task)
    flat.latency = action_latency.resolve(cfg.actions)
    flat.curriculum = _terms(cfg.curriculum)
    t = cfg.scene.terrain
    flat.extra.update(map=t.traversability_hashmap, map_size=(t.num_rows, t.num_cols), env_size=(t.env_num_rows, t.env_num_cols),
                      group=(t.group_num_rows, t.group_num_cols), walkers=t.num_walkers, spacing=(t.row_spacing, t.col_spacing),
                      augment=bool(getattr(cfg, "augment_camera", True)))
    if depth_task:      # extension task: heightfield terrain + the depth image as observation (tasks/visual_depth)
        flat.task, flat.obs_dim = "visual_depth", A.VISDEPTH_OBS_DIM
        clip = getattr(cam.spawn, "clipping_range", None) or (0.01, 20.0)
        # reset_traversable puts cars on the map's cell centres: (index - n // 2) * spacing
        span = lambda n, s: (-(n // 2) * s, (n - 1 - n // 2) * s)
        flat.extra.update(_terrain_source(t, span(t.num_cols, t.row_spacing), span(t.num_rows, t.col_spacing)), max_depth=float(clip[1]),
                          augment=False)
    return flat


def flatten_cfg(cfg):
    task = getattr(cfg, "wl_task", "drift")
    if task == "elevation":
        return flatten_elev_cfg(cfg)
    if task in ("visual", "visual_depth"):
        return flatten_visual_cfg(cfg)
    f = flatten_drift_cfg(cfg)
    f.task, f.extra = "drift", {}
    return f

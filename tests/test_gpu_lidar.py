"""The lidar on the GPU (wl_raycast_scan through core.LidarScanner and the scene's LidarData): closed forms on the plane, every beam
against the float64 reference (tests/lidar_reference.py: oracle/depth.c, one ray per beam) on the bench field, the non-bench fields
of tests/heightfield_cases.py and a mesh course, the launch's edges, the env surface (`cfg.scene.lidar` + the reference's
`lidar_ranges_normalized` observation) and a short PPO run on the scan.  Yardstick of tests/test_gpu_depth_parity.py: the 0.999
quantile of the relative error and the hit / miss disagreement fraction both below 1e-4."""
import math

import numpy as np
import pytest
import torch

from tests import heightfield_cases as HC
from tests import lidar_reference as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(**kw):
    from wheeledlab_amd.envs.sensors_cfg import LidarCfg, LidarPatternCfg
    pat = kw.pop("pattern", None)
    c = LidarCfg(**kw)
    if pat is not None:
        c.pattern_cfg = LidarPatternCfg(**pat)
    return c


def _scanner(**kw):
    from wheeledlab_amd.core import LidarScanner
    return LidarScanner(_cfg(**kw), DEV)


def _posed(pos, quat):
    """a batch whose state rows carry the given root poses (the scan reads rows WL_S_PX.. / WL_S_QW.. only)"""
    from wheeledlab_amd.core import DriftBatch
    b = DriftBatch(len(pos), device=DEV, seed=1)
    b.state[0:3, : b.n] = torch.from_numpy(np.ascontiguousarray(pos.T)).to(DEV)
    b.state[3:7, : b.n] = torch.from_numpy(np.ascontiguousarray(quat.T)).to(DEV)
    return b


def _camera(field, outside_z=None):
    from wheeledlab_amd.core import DepthCamera
    return DepthCamera(field, DEV, outside_z=outside_z)


def _oracle_field(cam):
    """the decoded fp32 heights every kernel sees, as the oracle takes them"""
    return (cam.height.cpu().numpy(), cam.hf.x0, cam.hf.y0, cam.hf.cell)


def _quat(roll, pitch, yaw):
    from oracle.mathlib import quat_from_euler_xyz
    e = np.asarray([[roll, pitch, yaw]], np.float32)
    return quat_from_euler_xyz(e[:, 0], e[:, 1], e[:, 2]).astype(np.float32)


FAN = dict(channels=7, vertical_fov_range=(-90.0, 0.0), horizontal_fov_range=(-180.0, 180.0), horizontal_res=45.0)


def _fan_dirs():
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    el, az = LidarPatternCfg(**FAN).angles()
    return el, az, LidarPatternCfg(**FAN).directions()


# ---- 1. closed forms on the plane -----------------------------------------------------------------------------------

def test_level_car_on_the_plane_reads_max_range_and_h_over_sin():
    el, az, _ = _fan_dirs()
    assert sorted(set(np.round(el, 6))) == sorted(set(np.round(np.linspace(-90.0, 0.0, 7), 6)))
    sc = _scanner(pattern=FAN, max_range=30.0)
    pos = np.array([[0.0, 0.0, 0.1], [250.0, -40.0, 0.35], [-3.0, 7.0, 0.02]], np.float32)
    quat = np.repeat(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), 3, 0)
    got = sc.render(_posed(pos, quat)).cpu().numpy()
    for e in range(3):
        h = float(np.float32(pos[e, 2]) + np.float32(0.18))
        flat = el == 0.0
        assert (got[e, flat] == 30.0).all()
        th = np.radians(-el[~flat])
        np.testing.assert_allclose(got[e, ~flat], np.minimum(h / np.sin(th), 30.0), rtol=1e-5)


def _plane_closed_form(pos, quat, dirs, max_range, **mount):
    o, M = LR.sensor_frames(pos, quat, **mount)
    w = np.einsum("nij,bj->nbi", M, dirs)
    t = np.where(w[..., 2] < 0, -o[:, None, 2] / np.where(w[..., 2] < 0, w[..., 2], -1.0), np.inf)
    return np.minimum(t, max_range)


@pytest.mark.parametrize("euler", [(0.0, 0.3, 0.0), (0.0, -0.2, 0.0), (0.0, 0.0, 1.1), (0.2, 0.25, -2.4)])
def test_pitched_and_yawed_cars_match_the_closed_form(euler):
    _, _, dirs = _fan_dirs()
    mount = dict(offset_pos=(0.05, -0.02, 0.2), offset_rot=(0.9961947, 0.0, 0.0871557, 0.0))     # pitched 10 degrees down on its mount
    sc = _scanner(pattern=FAN, max_range=30.0, **mount)
    pos = np.array([[1.5, -0.5, 0.15]], np.float32)
    quat = _quat(*euler)
    got = sc.render(_posed(pos, quat)).cpu().numpy()
    want = _plane_closed_form(pos, quat, dirs, 30.0, **mount)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert (want < 30.0).any() and (want == 30.0).any()


def test_attach_yaw_only_ignores_roll_and_pitch():
    el, _, dirs = _fan_dirs()
    sc = _scanner(pattern=FAN, max_range=30.0, attach_yaw_only=True)
    pos = np.array([[0.0, 0.0, 0.1]] * 3, np.float32)
    quat = np.concatenate([_quat(0.0, 0.0, 0.7), _quat(0.3, -0.4, 0.7), _quat(-0.5, 0.2, 0.7)])
    got = sc.render(_posed(pos, quat)).cpu().numpy()
    np.testing.assert_allclose(got[1], got[0], rtol=1e-5)
    np.testing.assert_allclose(got[2], got[0], rtol=1e-5)
    flat = el == 0.0
    assert (got[:, flat] == 30.0).all()
    np.testing.assert_allclose(got[0, ~flat], np.minimum((0.1 + 0.18) / np.sin(np.radians(-el[~flat])), 30.0), rtol=1e-5)
    tilted = _scanner(pattern=FAN, max_range=30.0).render(_posed(pos, quat)).cpu().numpy()
    assert not np.array_equal(tilted[1], tilted[0])           # without the flag the tilt shows


# ---- 2. every beam against the oracle -------------------------------------------------------------------------------

PATTERNS = {"1x360": dict(), "16x360": dict(channels=16, vertical_fov_range=(-15.0, 15.0))}


def _fields():
    from oracle import heightfield as HF
    yield "bench", HF.make_terrain(), 0.0, None
    for g in ("G1", "G2", "G3", "G4a", "G4b", "G6"):
        f = HC.get(g)
        yield g, f, f.outside_z, f


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_every_beam_matches_the_oracle_on_bench_and_non_bench_fields(pattern):
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    dirs = LidarPatternCfg(**PATTERNS[pattern]).directions()
    for i, (name, field, oz, case) in enumerate(_fields()):
        cam = _camera(field) if case is None else _camera(case.device(DEV))
        of = _oracle_field(cam)
        pos, quat = LR.poses(1024, seed=40 + i, field=of, outside_z=oz, margin=1.0)
        b = _posed(pos, quat)
        for mr in (10.0, 30.0):
            got = _scanner(pattern=PATTERNS[pattern], max_range=mr).render(b, camera=cam)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            want = LR.ranges(pos, quat, dirs, of, mr, oz)
            rel, flip = LR.check(got, want, mr, (name, pattern, mr))
            hit = want < mr
            print(f"lidar parity {name} {pattern} max_range={mr}: hit fraction {hit.mean():.3f}, flips {int(flip.sum())} of {flip.size}, "
                  f"p99.9 rel err {np.quantile(rel, 0.999):.2e}")
            assert hit.any() and (got >= 0).all() and (got <= mr).all()


def test_a_field_the_pyramid_cannot_hold_is_refused():
    """G5 (32 800 points wide) is beyond the bound pyramid's layout (nx, ny <= 16 385): the terrain is refused, as for the camera"""
    from wheeledlab_amd import _abi as A
    with pytest.raises(A.WlError):
        _camera(HC.get("G5").device(DEV))


# ---- 3. a mesh course --------------------------------------------------------------------------------------------------

def _walled_box_obj(path, half=5.0, thick=0.2, height=1.0):
    """a 10 m square floor at z = 0 walled in by four boxes (0.2 m thick, 1 m high), as OBJ text"""
    verts, faces = [], []

    def quad(a, b, c, d):
        k = len(verts)
        verts.extend([a, b, c, d])
        faces.extend([(k + 1, k + 2, k + 3), (k + 1, k + 3, k + 4)])

    def box(x0, x1, y0, y1, z):
        quad((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z))                      # top
        for (ax, ay), (bx, by) in (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))):
            quad((ax, ay, 0.0), (bx, by, 0.0), (bx, by, z), (ax, ay, z))              # sides (vertical: skipped by the raster)
    box(-half, half, -half, half, 0.0)
    box(half - thick, half, -half, half, height)
    box(-half, -half + thick, -half, half, height)
    box(-half, half, half - thick, half, height)
    box(-half, half, -half, -half + thick, height)
    path.write_text("".join(f"v {x} {y} {z}\n" for x, y, z in verts) + "".join(f"f {a} {b} {c}\n" for a, b, c in faces))


def test_mesh_course_walls_against_the_oracle_and_the_analytic_distance(tmp_path):
    from wheeledlab_amd.core import mesh_heightfield
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    from wheeledlab_amd.terrain import load_obj
    _walled_box_obj(tmp_path / "course.obj")
    cell = 0.05
    hf = mesh_heightfield(*load_obj(str(tmp_path / "course.obj")), cell, device=DEV)
    cam = _camera(hf)
    of = _oracle_field(cam)
    rng = np.random.RandomState(3)
    n = 64
    pos = np.concatenate([rng.uniform(-3.0, 3.0, (n, 2)), np.full((n, 1), 0.1)], 1).astype(np.float32)
    pos[0] = (0.0, 0.0, 0.1)
    quat = np.concatenate([_quat(0.0, 0.0, 0.0)] + [_quat(0.0, 0.0, y) for y in rng.uniform(-np.pi, np.pi, n - 1)])
    sc = _scanner(max_range=20.0)
    got = sc.render(_posed(pos, quat), camera=cam).cpu().numpy()
    dirs = LidarPatternCfg().directions()
    LR.check(got, LR.ranges(pos, quat, dirs, of, 20.0), 20.0, "mesh course")
    assert (got < 20.0).all()                                   # walled in: every horizontal beam meets a wall
    # the inner wall faces lie at |x| = 4.8 and |y| = 4.8: beams within 30 degrees of a face normal, median range error per face
    o, M = LR.sensor_frames(pos, quat)
    w = np.einsum("nij,bj->nbi", M, dirs)
    for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):
        cosang = sign * w[..., axis]
        sel = cosang > math.cos(math.radians(30.0))
        analytic = (4.8 - sign * o[:, None, axis]) / np.where(sel, cosang, 1.0)
        err = np.median(np.abs(got[sel] - analytic[sel]))
        assert err < cell, (axis, sign, err)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------

def test_under_the_terrain_and_beams_leaving_the_grid():
    from oracle import heightfield as HF
    hf = HF.make_terrain()
    cam = _camera(hf)
    of = _oracle_field(cam)
    z, _, _ = HF.sample(*of, np.array([3.0], np.float32), np.array([4.0], np.float32))
    pos = np.array([[3.0, 4.0, z[0] - 0.6]], np.float32)                   # sensor 0.42 m under the ground
    got = _scanner(max_range=30.0).render(_posed(pos, _quat(0.1, 0.0, 0.3)), camera=cam).cpu().numpy()
    assert (got == 0.0).all()
    # G4b: a 2 x 3 grid of 5 cm cells, outside plane z = -1; a sensor 0.5 m over its middle: shallow beams leave the grid at once and
    # meet the outside plane at (o_z + 1) / sin(theta), steep ones hit the grid
    f = HC.get("G4b")
    cam = _camera(f.device(DEV))
    pos = np.array([[f.x0 + 0.05, f.y0 + 0.025, 0.5 - 0.18]], np.float32)
    q = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    el, az, dirs = _fan_dirs()
    got = _scanner(pattern=FAN, max_range=30.0).render(_posed(pos, q), camera=cam).cpu().numpy()[0]
    shallow = (el < 0) & (el > -60)
    np.testing.assert_allclose(got[shallow], 1.5 / np.sin(np.radians(-el[shallow])), rtol=1e-5)
    assert (got[el == 0.0] == 30.0).all() and (got[el == -90.0] < 0.6).all()
    LR.check(got[None], LR.ranges(pos, q, dirs, _oracle_field(cam), 30.0, -1.0), 30.0, "G4b")


@pytest.mark.parametrize("n_beams,pat", [(1, dict(horizontal_fov_range=(0.0, 0.0))), (63, dict(horizontal_fov_range=(0.0, 62.0))),
                                         (65, dict(horizontal_fov_range=(0.0, 64.0))),
                                         (1081, dict(horizontal_fov_range=(-135.0, 135.0), horizontal_res=0.25))])
def test_beam_counts_that_are_not_multiples_of_64(n_beams, pat):
    from oracle import heightfield as HF
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    hf = HF.make_terrain()
    cam = _camera(hf)
    of = _oracle_field(cam)
    pos, quat = LR.poses(64, seed=5, field=of)
    sc = _scanner(pattern=pat, max_range=30.0)
    assert sc.n_beams == n_beams
    n = len(pos)
    guard = torch.full((n * n_beams + 4096,), float("nan"), device=DEV)
    out = guard[: n * n_beams].view(n, n_beams)
    sc.render(_posed(pos, quat), out=out, camera=cam)
    torch.cuda.synchronize()
    assert torch.isnan(guard[n * n_beams:]).all()                         # nothing written past the last env's row
    LR.check(out.cpu().numpy(), LR.ranges(pos, quat, LidarPatternCfg(**pat).directions(), of, 30.0), 30.0, n_beams)


def test_one_env_and_more_envs_than_a_grid_dimension():
    from oracle import heightfield as HF
    hf = HF.make_terrain()
    cam = _camera(hf)
    of = _oracle_field(cam)
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    dirs = LidarPatternCfg().directions()
    sc = _scanner(max_range=30.0)
    pos, quat = LR.poses(70000, seed=8, field=of)
    one = sc.render(_posed(pos[:1], quat[:1]), camera=cam).cpu().numpy()
    LR.check(one, LR.ranges(pos[:1], quat[:1], dirs, of, 30.0), 30.0, "n=1")
    b = _posed(pos, quat)
    got = sc.render(b, camera=cam)
    torch.cuda.synchronize()
    idx = np.r_[0:64, 65500:65600, 69936:70000]
    LR.check(got.cpu().numpy()[idx], LR.ranges(pos[idx], quat[idx], dirs, of, 30.0), 30.0, "n=70000")
    assert np.array_equal(got.cpu().numpy()[:1], one)
    assert torch.equal(sc.render(b, camera=cam), got)                    # two renders: bit-identical


def test_the_depth_camera_is_unchanged_by_a_scan():
    from oracle import heightfield as HF
    cam = _camera(HF.make_terrain())
    pos, quat = LR.poses(256, seed=9, field=_oracle_field(cam))
    b = _posed(pos, quat)
    pyr = cam.pyramid.clone()
    before = cam.render(b, 30.0).clone()
    _scanner(max_range=30.0, pattern=PATTERNS["16x360"]).render(b, camera=cam)
    after = cam.render(b, 30.0)
    torch.cuda.synchronize()
    assert torch.equal(before, after) and torch.equal(pyr.view(torch.int32), cam.pyramid.view(torch.int32))     # (entries are packed words)


# ---- 5. the env surface ---------------------------------------------------------------------------------------------------

def _env(task, n, **lidar):
    from wheeledlab_amd import registry, tasks  # noqa: F401
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import ObservationTermCfg as ObsTerm
    from wheeledlab_amd.envs.managers_cfg import SceneEntityCfg
    cfg = registry.parse_env_cfg(task, device=DEV, num_envs=n)
    cfg.scene.lidar = _cfg(**lidar)
    cfg.observations.policy.lidar = ObsTerm(func=mdp.lidar_ranges_normalized, params={"sensor_cfg": SceneEntityCfg("lidar")})
    return registry.make(task, cfg=cfg)


def _count_renders(data):
    sc = data.scanner()
    calls = []
    render = sc.render

    def counted(*a, **kw):
        calls.append(1)
        return render(*a, **kw)
    sc.render = counted
    return calls


def test_elevation_env_with_a_lidar_observation():
    from wheeledlab_amd.core import LidarScanner
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import SceneEntityCfg
    n = 256
    env = _env("Isaac-MushrElevationRL-v0", n)
    B = 360
    assert env.observation_manager.group_obs_dim["policy"] == (689 + B,)
    data = env.scene.sensors["lidar"].data
    assert data._cached == (None, None)                                   # the shape probe kept nothing
    calls = _count_renders(data)
    obs, _ = env.reset()
    assert obs["policy"].shape == (n, 689 + B) and len(calls) == 1
    lid = obs["policy"][:, 689:]
    assert float(lid.min()) >= 0.0 and float(lid.max()) <= 1.0
    direct = LidarScanner(data._cfg, DEV).render(env._batch)
    assert torch.equal(mdp.lidar_ranges(env, SceneEntityCfg("lidar")), direct) and len(calls) == 1
    g = torch.Generator(device=DEV).manual_seed(0)
    for k in range(3):
        obs, *_ = env.step(torch.rand(n, 2, device=DEV, generator=g) * 2 - 1)
        for _ in range(3):                                                # however often it is read: one scan per step
            r = mdp.lidar_ranges(env, SceneEntityCfg("lidar"))
        assert len(calls) == 2 + k
        assert torch.equal(r, LidarScanner(data._cfg, DEV).render(env._batch))
        lid = obs["policy"][:, 689:]
        assert float(lid.min()) >= 0.0 and float(lid.max()) <= 1.0 and lid.std() > 0
    hits = data.ray_hits_w
    assert hits.shape == (n, B, 3) and data.pos_w.shape == (n, 3) and data.quat_w.shape == (n, 4)
    miss = r >= data.max_range
    assert torch.isinf(hits[miss]).all() and torch.isfinite(hits[~miss]).all()
    torch.testing.assert_close((hits[~miss] - data.pos_w[:, None, :].expand(-1, B, -1)[~miss]).norm(dim=-1), r[~miss], rtol=1e-5, atol=1e-5)
    # a reset and a plugin's pose write each invalidate the cached scan
    env.reset()
    mdp.lidar_ranges(env, SceneEntityCfg("lidar"))
    assert len(calls) == 5
    robot = env.scene["robot"]
    pose = torch.cat([robot.data.root_pos_w, robot.data.root_quat_w], 1)
    pose[:, 2] += 0.5
    robot.write_root_pose_to_sim(pose)
    lifted = mdp.lidar_ranges(env, SceneEntityCfg("lidar"))
    assert len(calls) == 6 and torch.equal(lifted, LidarScanner(data._cfg, DEV).render(env._batch))
    env.close()


def test_drift_env_sees_the_plane_and_visual_depth_env_its_own_field():
    from wheeledlab_amd.envs import mdp
    from wheeledlab_amd.envs.managers_cfg import SceneEntityCfg
    from wheeledlab_amd.envs.sensors_cfg import LidarPatternCfg
    mount = dict(offset_rot=(0.9961947, 0.0, 0.0871557, 0.0))            # 10 degrees down: the beams reach the ground
    dirs = LidarPatternCfg().directions()
    for task in ("Isaac-MushrDriftRL-v0", "Isaac-MushrVisualDepthRL-v0"):
        n = 64
        env = _env(task, n, max_range=20.0, **mount)
        env.reset()
        for _ in range(3):
            env.step(torch.rand(n, 2, device=DEV) * 2 - 1)
        b = env._batch
        got = mdp.lidar_ranges(env, SceneEntityCfg("lidar")).cpu().numpy()
        st = b.state[:, :n].cpu().numpy()
        if task == "Isaac-MushrDriftRL-v0":
            want = _plane_closed_form(st[0:3].T, st[3:7].T, dirs, 20.0, offset_pos=(0.0, 0.0, 0.18), **mount)
            near = want < 18.0
            np.testing.assert_allclose(got[near], want[near], rtol=1e-5)
            assert near.mean() > 0.3
        else:
            assert env.scene.sensors["lidar"].data.scanner().camera_of(b) is b.camera
            of = _oracle_field(b.camera)
            LR.check(got, LR.ranges(st[0:3].T, st[3:7].T, dirs, of, 20.0, b.camera.hf.outside_z, **mount), 20.0, task)
        env.close()


def test_a_shard_scans_its_rows_of_the_full_batch():
    from wheeledlab_amd.core import ElevBatch
    full = ElevBatch(300, device=DEV, seed=2)
    full.reset()
    full.rollout(torch.rand(3, 300, 2, device=DEV) * 2 - 1)
    shard = ElevBatch(100, device=DEV, seed=2, env_offset=100, heightfield=full.hf)
    shard.state[:, :100] = full.state[:, 100:200]
    sc = _scanner(pattern=PATTERNS["16x360"], max_range=30.0)
    a, s = sc.render(full), sc.render(shard)
    assert torch.equal(a[100:200], s)


# ---- 6. training on the scan ---------------------------------------------------------------------------------------------

def test_two_ppo_iterations_on_the_lidar_observation():
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    torch.manual_seed(0)
    env = _env("Isaac-MushrElevationRL-v0", 256)
    env.action_space.low, env.action_space.high = -1.0, 1.0
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ClipAction(env)), registry.load_cfg_from_registry("Isaac-MushrElevationRL-v0",
                                                                                                   "rsl_rl_cfg_entry_point"), device=DEV)
    assert runner.actor_critic.actor[0].in_features == 689 + 360 and runner.alg._wide
    before = [p.detach().clone() for p in runner.actor_critic.parameters()]
    hist = runner.learn(2, verbose=False)
    assert len(hist) == 2 and all(np.isfinite(h["value_function"]) and np.isfinite(h["surrogate"]) for h in hist)
    assert any(not torch.equal(p, q) for p, q in zip(before, runner.actor_critic.parameters()))

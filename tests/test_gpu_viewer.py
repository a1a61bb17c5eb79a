"""GPU: the viewer camera (wl_viewer_render) against the numpy restatement (tests/viewer_reference.py) and the depth oracle, the
env's render() surface, and video recording through a short PPO run."""
import os

import numpy as np
import pytest
import torch

import depth_cases as DC
import viewer_reference as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set_poses(batch, pos, quat):
    from wheeledlab_amd import _abi as A
    n = pos.shape[0]
    batch.state[A.S_PX:A.S_PZ + 1, :n] = torch.as_tensor(pos.T, device=DEV)
    batch.state[A.S_QW:A.S_QZ + 1, :n] = torch.as_tensor(quat.T, device=DEV)


def _poses(batch):
    from wheeledlab_amd import _abi as A
    st = batch.state[:, :batch.n].cpu().numpy()
    return np.ascontiguousarray(st[A.S_PX:A.S_PZ + 1].T), np.ascontiguousarray(st[A.S_QW:A.S_QZ + 1].T)


def _render(viewer, batch, eye, lookat, env_index=0):
    H, W = viewer.height, viewer.width
    depth = torch.empty(H, W, dtype=torch.float32, device=DEV)
    ids = torch.empty(H, W, dtype=torch.int32, device=DEV)
    rgb = viewer.render(batch, eye, lookat, env_index=env_index, depth=depth, ids=ids)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()


def _reference(viewer, batch, eye, lookat, env_index=0, explain=False):
    p = viewer.params(batch, eye, lookat, env_index)
    pos, quat = _poses(batch)
    hf = None
    if getattr(batch, "hf", None) is not None:
        hf = (batch.hf.heights.cpu().numpy(), batch.hf.x0, batch.hf.y0, batch.hf.cell, batch.hf.outside_z)
    trav = None
    if getattr(batch, "_map", None) is not None:
        trav = (batch.trav_map.cpu().numpy(), float(batch._map.row_spacing), float(batch._map.col_spacing))
    return VR.acceptable(p, pos, quat, hf, trav) if explain else VR.render(p, pos, quat, hf, trav)


def _check(got, want, what, min_ids=0.995, max_bad=2e-3):
    c = VR.compare(got, want)
    print(what, c)
    assert c["id_match"] >= min_ids, (what, c)
    assert c["depth_bad"] <= max_bad * c["n"] and c["colour_bad"] <= max_bad * c["n"], (what, c)
    return c


def _check_explained(got, viewer, batch, eye, lookat, what, env_index=0):
    """the bounds of _check, and every pixel explained by the float64 reference's own state (viewer_reference.check_explained)"""
    acc = _reference(viewer, batch, eye, lookat, env_index, explain=True)
    _check(got, acc["nominal"], what)
    return VR.check_explained(got, acc, what)


def _elev(n, field=None):
    from wheeledlab_amd.core import ElevBatch
    return ElevBatch(n, device=DEV, seed=3, heightfield=field)


def test_terrain_depth_matches_depth_oracle_at_full_resolution():
    """elevation viewer pose (20, -20, 20) -> 0 at 1280 x 720 over the depth-case terrain, no car in view: the depth output is the
    depth oracle's answer for a camera at the eye with the look-at rotation"""
    from types import SimpleNamespace

    from oracle import depth as OD
    from wheeledlab_amd.viewer import Viewer, look_at
    b = _elev(64, DC.on_lattice(DC.terrain()))
    pos = np.tile(np.array([[0.0, 0.0, -5000.0]], np.float32), (64, 1))       # far below and beyond the far clip: culled
    _set_poses(b, pos, np.tile(np.array([[1.0, 0, 0, 0]], np.float32), (64, 1)))
    v = Viewer(DEV, (1280, 720))
    eye, lookat = (20.0, -20.0, 20.0), (0.0, 0.0, 0.0)
    rgb, depth, ids = _render(v, b, eye, lookat)
    assert (ids >= -2).all() and (ids < 0).all()
    p = v.params(b, eye, lookat)
    e, q = look_at(eye, lookat)
    cam = SimpleNamespace(cam_pos=(0.0, 0.0, 0.0), fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy)
    field = (b.hf.heights.cpu().numpy(), b.hf.x0, b.hf.y0, b.hf.cell)
    want = OD.depth(cam, e[None], q[None], field, p.far_clip, outside_z=b.hf.outside_z, img_h=720, img_w=1280)[0]
    bad, err = DC.mismatch(depth, want, p.far_clip)
    print(f"viewer terrain depth: grazing {int(bad.sum())} of {bad.size}, p99.9 err {np.quantile(err, 0.999):.2e}")
    assert bad.mean() < 1e-4 and np.quantile(err, 0.999) < 1e-4
    _check_explained((rgb, depth, ids), v, b, eye, lookat, "terrain")


@pytest.mark.parametrize("mapped", [False, True])
def test_plane_matches_reference(mapped):
    from wheeledlab_amd.core import DriftBatch, VisualBatch
    from wheeledlab_amd.viewer import Viewer
    b = VisualBatch(256, device=DEV, seed=1) if mapped else DriftBatch(256, device=DEV, seed=1)
    b.reset()
    v = Viewer(DEV, (640, 360))
    eye, lookat = ((40.0, 0.0, 45.0), (0.0, 0.0, -3.0)) if mapped else ((4.0, -4.0, 4.0), (0.0, 0.0, 0.0))
    got = _render(v, b, eye, lookat)
    _check_explained(got, v, b, eye, lookat, f"plane mapped={mapped}")
    assert (got[2] >= 0).any() and (got[2] == -1).any()      # cars and ground both in the frame


@pytest.mark.parametrize("eye", [(20.0, -20.0, 20.0), (6.0, -6.0, 5.0)])
def test_cars_on_terrain_match_reference(eye):
    from wheeledlab_amd.viewer import Viewer
    b = _elev(4096, DC.on_lattice(DC.terrain()))
    pos, quat = DC.poses(4096, 11, DC.on_lattice(DC.terrain()))
    _set_poses(b, pos, quat)
    v = Viewer(DEV, (320, 180))
    got = _render(v, b, eye, (0.0, 0.0, 0.0))
    _check_explained(got, v, b, eye, (0.0, 0.0, 0.0), f"cars {eye}")
    assert (got[2] >= 0).sum() > 100


def test_cars_after_physics_match_reference():
    from wheeledlab_amd.viewer import Viewer
    b = _elev(4096)
    b.reset()
    g = torch.Generator(device=DEV).manual_seed(0)
    b.rollout(torch.rand(30, 4096, 2, device=DEV, generator=g) * 2 - 1)
    v = Viewer(DEV, (320, 180))
    for eye in ((20.0, -20.0, 20.0), (8.0, -8.0, 6.0)):
        got = _render(v, b, eye, (0.0, 0.0, 0.0))
        _check_explained(got, v, b, eye, (0.0, 0.0, 0.0), f"after physics {eye}")


def test_crowded_tiles_and_near_cars_are_complete():
    """more cars on one tile than one LDS chunk holds (tile lists span several chunks), and cars near the camera whose rectangles
    go to the big list: the frame still equals the reference, so no car is dropped"""
    from wheeledlab_amd.viewer import Viewer
    from oracle.mathlib import quat_from_euler_xyz
    n = 1500
    rng = np.random.RandomState(4)
    pos = np.zeros((n, 3), np.float32)
    pos[:700, :2] = rng.uniform(-0.05, 0.05, (700, 2))            # a pile at the origin: ~1 tile from 40 m
    pos[700:, :2] = rng.uniform(-3, 3, (800, 2))
    pos[:, 2] = rng.uniform(0.0, 0.3, n)
    quat = quat_from_euler_xyz(np.zeros(n, np.float32), np.zeros(n, np.float32), rng.uniform(-np.pi, np.pi, n).astype(np.float32))
    from wheeledlab_amd.core import DriftBatch
    b = DriftBatch(n, device=DEV, seed=2)
    _set_poses(b, pos, np.ascontiguousarray(quat.astype(np.float32)))
    v = Viewer(DEV, (320, 180))
    for eye, lookat in (((25.0, -25.0, 20.0), (0.0, 0.0, 0.0)), ((1.2, -1.2, 0.8), (0.0, 0.0, 0.0))):
        got = _render(v, b, eye, lookat)
        _check_explained(got, v, b, eye, lookat, f"crowded {eye}")
        assert len(np.unique(got[2][got[2] >= 0])) > 20


def test_two_renders_are_byte_identical():
    from wheeledlab_amd.viewer import Viewer
    b = _elev(4096)
    b.reset()
    v = Viewer(DEV, (640, 360))
    a = _render(v, b, (8.0, -8.0, 6.0), (0.0, 0.0, 0.0))
    c = _render(v, b, (8.0, -8.0, 6.0), (0.0, 0.0, 0.0))
    for x, y in zip(a, c):
        assert x.tobytes() == y.tobytes()


TASKS = ["Isaac-MushrDriftRL-v0", "Isaac-F1TenthDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0",
         "Isaac-MushrVisualDepthRL-v0"]


@pytest.mark.parametrize("task", TASKS)
def test_env_render_every_task(task):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    cfg = registry.parse_env_cfg(task, device=DEV, num_envs=64)
    env = registry.make(task, cfg=cfg, render_mode="rgb_array")
    env.reset()
    img = env.render()
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (720, 1280, 3)
    assert env.metadata["render_fps"] == pytest.approx(1.0 / env.step_dt) and "rgb_array" in env.metadata["render_modes"]
    assert img.std() > 0
    env.close()
    env = registry.make(task, cfg=registry.parse_env_cfg(task, device=DEV, num_envs=64), render_mode=None)
    env.reset()
    assert env.render() is None
    env.close()


@pytest.mark.parametrize("task", ["Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0"])
def test_rendering_does_not_change_the_rollout(task):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    outs = []
    for render in (False, True):
        torch.manual_seed(0)          # the visual task's augmentation draws come from torch's global RNG
        cfg = registry.parse_env_cfg(task, device=DEV, num_envs=256)
        cfg.seed = 9
        env = registry.make(task, cfg=cfg, render_mode="rgb_array")
        obs, _ = env.reset()
        g = torch.Generator(device=DEV).manual_seed(1)
        rec = [obs["policy"].clone()]
        for _ in range(16):
            a = torch.rand(256, 2, device=DEV, generator=g) * 2 - 1
            o, r, te, tr, _ = env.step(a)
            rec += [o["policy"].clone(), r.clone(), te.clone(), tr.clone()]
            if render:
                env.render()
        rec.append(torch.tensor([env.common_step_counter]))
        outs.append([t.cpu() for t in rec])
        env.close()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_asset_root_origin_follows_the_env():
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.viewer import Viewer
    cfg = registry.parse_env_cfg("Isaac-MushrDriftRL-v0", device=DEV, num_envs=128)
    cfg.viewer.origin_type, cfg.viewer.env_index = "asset_root", 5
    cfg.viewer.eye, cfg.viewer.lookat, cfg.viewer.resolution = [1.5, -1.5, 1.2], [0.0, 0.0, 0.0], (320, 180)
    env = registry.make("Isaac-MushrDriftRL-v0", cfg=cfg, render_mode="rgb_array")
    env.reset()
    env.step(torch.zeros(128, 2, device=DEV))
    got = env.render()
    root = env._batch.state[0:3, 5].double().cpu().numpy()
    want = Viewer(DEV, (320, 180)).render(env._batch, np.array([1.5, -1.5, 1.2]) + root, root, env_index=5).cpu().numpy()
    assert np.array_equal(got, want)
    env.close()


def test_training_with_video_records_one_clip_and_keeps_the_fused_path(tmp_path):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    from wheeledlab_amd.video import RecordVideo
    from test_viewer_cpu import _read_apng
    torch.manual_seed(0)
    cfg = registry.parse_env_cfg("Isaac-MushrDriftRL-v0", device=DEV, num_envs=1024)
    cfg.viewer.resolution = (320, 180)
    base = registry.make("Isaac-MushrDriftRL-v0", cfg=cfg, render_mode="rgb_array")
    base.action_space.low, base.action_space.high = -1.0, 1.0
    env = RslRlVecEnvWrapper(ClipAction(base))
    runner = OnPolicyRunner(env, registry.load_cfg_from_registry("Isaac-MushrDriftRL-v0", "rsl_rl_cfg_entry_point"), device=DEV)
    assert runner.fused
    K = runner.num_steps_per_env
    start, L = K + 2, max(1, min(8, K - 4))            # the clip lies inside the second iteration's rollout
    rec = RecordVideo(base, video_folder=str(tmp_path), step_trigger=lambda s: s == start, video_length=L, disable_logger=True,
                      writer="apng")
    hist = runner.learn(3, verbose=False)
    rec.close()
    assert len(hist) == 3
    assert runner.collection_paths == ["fused", "stepwise", "fused"]
    assert os.listdir(tmp_path) == [f"rl-video-step-{start}.png"]
    frames, n = _read_apng(os.path.join(tmp_path, f"rl-video-step-{start}.png"))
    assert n == L and frames.shape == (L, 180, 320, 3)
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])      # the cars move
    base.close()

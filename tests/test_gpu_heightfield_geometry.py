"""The terrain readers on the GPU over heightfields unlike the bench one (tests/heightfield_cases.py), against the float64 restatement
(tests/heightfield_reference.py) and the oracle.  Fields go in as a binder hands them over: a DeviceHeightField with the field's own
outside_z, passed to ElevBatch / VisualDepthBatch.  Poses are written straight into the state rows.
  * the 26 x 26 height scan against scan64 on G1 - G5 (poses beyond every border, straddling borders and corners, on lattice points
    at yaw 0, +-pi/2 and pi, tilted);
  * every scan form (fused step, split launch, persistent rollout, collector) equal to observe() of the state it leaves, on G1 and G5;
  * steps against the oracle on G1 - G3 in both kernel forms, cars spawned over each border; the visual-depth task on G1;
  * settled cars on the exact plane G6 need no excuse; reset heights on G1 against sample64(guard=True).
Mutation seen caught: x0 and y0 swapped in wl_elev_scan_dev.h::scan_frame -- test_height_scan_against_float64[G1] (over a million rays off)."""
import numpy as np
import pytest
import torch

from oracle import elev_step as OE
from oracle import visual_step as OV
from tests import heightfield_cases as HC
from tests import heightfield_reference as R
from tests import parity_predicates as PRED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SCANNED = ["G1", "G2", "G3", "G4a", "G4b", "G5"]


def _elev(field, n, seed=7, lanes=0, flags=0):
    from wheeledlab_amd.core import ElevBatch
    env = ElevBatch(n, device=DEV, seed=seed, heightfield=field.device(DEV))
    assert env.hf.outside_z == F(field.outside_z) and torch.equal(env.hf.codes.cpu(), torch.from_numpy(field.codes))
    env.set_lanes(lanes)
    env.set_flags(flags)
    env.reset()
    return env


def _poses(field, n, seed):
    """[7, n] root position + quaternion: uniform reaching 2 m beyond every border, straddling each border and corner, lattice points
    at yaw 0 / +-pi/2 / pi (rays on grid lines: fu, fv = 0 where scan_res is a multiple of the cell), tilted bodies"""
    rng = np.random.RandomState(seed)
    xl, xh, yl, yh = field.extent()
    x, y = rng.uniform(xl - 2, xh + 2, n), rng.uniform(yl - 2, yh + 2, n)
    k = n // 4
    side, t, d = rng.randint(0, 4, k), rng.uniform(0, 1, k), rng.normal(0, 0.5, k)
    x[:k] = np.where(side < 2, np.where(side == 0, xl, xh) + d, xl + t * (xh - xl))
    y[:k] = np.where(side < 2, yl + t * (yh - yl), np.where(side == 2, yl, yh) + d)
    c = rng.randint(0, 4, k // 2)
    x[k:k + k // 2] = np.where(c & 1, xh, xl) + rng.normal(0, 0.6, k // 2)
    y[k:k + k // 2] = np.where(c & 2, yh, yl) + rng.normal(0, 0.6, k // 2)
    yaw = rng.uniform(-np.pi, np.pi, n)
    m = slice(2 * k, 3 * k)
    x[m] = field.x0 + rng.randint(0, field.nx, k) * field.cell
    y[m] = field.y0 + rng.randint(0, field.ny, k) * field.cell
    yaw[m] = rng.randint(-1, 3, k) * (np.pi / 2)
    roll = np.where(np.arange(n) % 3 == 0, rng.normal(0, 0.2, n), 0.0)
    pitch = np.where(np.arange(n) % 3 == 0, rng.normal(0, 0.2, n), 0.0)
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])
    q[:, m] = np.stack([np.cos(yaw[m] / 2), 0 * yaw[m], 0 * yaw[m], np.sin(yaw[m] / 2)])
    z = rng.uniform(-0.5, 1.5, n)
    return np.concatenate([np.stack([x, y, z]), q]).astype(F)


def _put_poses(env, pose):
    n = pose.shape[1]
    env.state[0:7, :n] = torch.from_numpy(pose).to(DEV)


@pytest.mark.parametrize("name", SCANNED)
def test_height_scan_against_float64(name):
    f = HC.get(name)
    n = 2000
    env = _elev(f, n)
    _put_poses(env, _poses(f, n, seed=sum(map(ord, name))))
    obs = env.observe().cpu().numpy()
    st = env.state[:, :n].cpu().numpy()
    n_ex = R.check_scan(obs[:, 13:], env.p, st, f, where=name)
    print(f"{name}: scan vs float64, {n_ex} border rays excused of {n * 676}")
    hit = obs[:, 13:] < 10
    assert hit.any() and (~hit).any()


@pytest.mark.parametrize("name", ["G1", "G5"])
def test_every_scan_form_equals_observe(A, name):
    """fused step (quad form), split launch (lane-form step + the scan launch), persistent rollout and the collector: each one's
    observation row equals observe() of the state it leaves, bit for bit, and that is scan64's within the bound"""
    from wheeledlab_amd.policy import RolloutStorage
    from wheeledlab_amd.rl.ppo import ActorCritic
    f = HC.get(name)
    n, D = 1000, 689
    torch.manual_seed(3)
    ac = ActorCritic(D, D, 2, activation="elu").to(DEV)
    view = ac.fused()
    view.planes = False
    for form in ("fused", "split", "persistent", "collector"):
        env = _elev(f, n, seed=9, lanes=1 if form == "split" else 4, flags=A.FLAG_NO_STREAM)
        pose = _poses(f, n, seed=5)
        pose[2] = 0.4
        _put_poses(env, pose)
        a = (torch.rand(1, n, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 2 - 1).contiguous()
        if form in ("fused", "split"):
            env.step(a[0])
            got = env.obs.clone()
        elif form == "persistent":
            obs = torch.zeros(1, n, D, device=DEV)
            rew, term, trunc = torch.zeros(1, n, device=DEV), torch.zeros(1, n, dtype=torch.bool, device=DEV), torch.zeros(1, n, dtype=torch.bool, device=DEV)
            env.rollout(a, obs, rew, term, trunc, persistent=True)
            got = obs[0].clone()
        else:
            s = RolloutStorage(1, n, D, 2, DEV)
            s.observations[0].copy_(env.observe())
            env.collect_rollout(view, s, start=0, count=1)
            got = s.observations[1].clone()
        want = env.observe(torch.empty(n, D, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(got[:, 13:], want[:, 13:]), (name, form, int((got[:, 13:] != want[:, 13:]).sum()))
        n_ex = R.check_scan(got[:, 13:].cpu().numpy(), env.p, env.state[:, :n].cpu().numpy(), f, where=f"{name} {form}")
        print(f"{name} {form}: {n_ex} border rays excused")


@pytest.fixture(scope="module")
def A():
    from wheeledlab_amd import _abi
    return _abi


@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
@pytest.mark.parametrize("lanes", [4, 1])
def test_elev_steps_against_oracle(name, lanes):
    """single steps from the device state against the oracle with the field's outside_z, cars spawned over every border so that
    wheels leave the field; every env to the tight bound unless the oracle's own step explains it (tests/parity_predicates.py)"""
    f = HC.get(name)
    n = 512
    env = _elev(f, n, seed=5, lanes=lanes)
    p = OE.elev_params()
    xl, xh, yl, yh = f.extent()
    rng = np.random.RandomState(2)
    st = env.state.cpu().numpy()
    k = n // 2                                   # half the cars astride a border (x or y), the rest where the reset put them
    side, t = rng.randint(0, 4, k), rng.uniform(0.1, 0.9, k)
    st[0, :k] = np.where(side < 2, np.where(side == 0, xl, xh) + rng.uniform(-0.3, 0.3, k), xl + t * (xh - xl))
    st[1, :k] = np.where(side < 2, yl + t * (yh - yl), np.where(side == 2, yl, yh) + rng.uniform(-0.3, 0.3, k))
    z, _, _ = R.sample64(f, st[0, :k], st[1, :k])
    st[2, :k] = z + 0.12
    env.state.copy_(torch.from_numpy(st))
    excused = 0
    for k_ in range(10):
        st = env.state.cpu().numpy().copy()
        ep = env.episode_len.cpu().numpy().copy()
        a = rng.uniform(-1, 1, (n, 2)).astype(F)
        a[:, 0] = np.abs(a[:, 0]) * 0.6 + 0.2
        obs, rew, term, trunc = env.step(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        probe = {}
        o_obs, o_rew, o_term, o_trunc, _ = OE.step(p, st, ep, f.oracle(), a, 5, k_, probe=probe)
        got = env.state.cpu().numpy()
        bad = term.cpu().numpy() != o_term
        assert bad.sum() <= 2, (k_, int(bad.sum()))
        ok, n_ex = PRED.check_state(got, st, probe, n, ~bad, where=f"{name} lanes {lanes} step {k_}")
        excused += n_ex
        np.testing.assert_allclose(rew.cpu().numpy()[ok], o_rew[ok], rtol=2e-3, atol=5e-2)
        # the scan of the DEVICE's post-step state against float64
        R.check_scan(obs[:, 13:].cpu().numpy(), env.p, got[:, :n], f, where=f"{name} lanes {lanes} step {k_}")
    print(f"{name} lanes {lanes}: {excused} env-steps excused of {10 * n}")
    assert excused <= 0.01 * 10 * n, excused
    assert int(env.metrics[8]) > 0                 # resets happened (some over the border / the outside plane)


@pytest.mark.parametrize("lanes", [4, 1])
def test_settled_cars_on_an_exact_plane_need_no_excuse(lanes):
    """G6 (planar on the code lattice, G1's placement and outside_z): no cell-line kinks, all four wheels loaded -- the excused set
    is empty for 16 steps in both forms"""
    f = HC.get("G6")
    n = 256
    from wheeledlab_amd.core import ElevBatch
    env = ElevBatch(n, device=DEV, seed=8, heightfield=f.device(DEV))
    env.set_lanes(lanes)
    p = OE.elev_params()
    for q in (env.p, p):
        q.max_episode_length = 10 ** 9
        q.min_height, q.stuck_min_vel, q.upright_cos, q.goal_dist = -1e9, -1e9, -2.0, -1.0
    env.p.reset_xy = 6.0          # inside the field (y from -7.15 m)
    env.reset()
    rng = np.random.RandomState(1)
    gentle = lambda: np.stack([rng.uniform(0.1, 0.3, n), rng.uniform(-0.3, 0.3, n)], -1).astype(F)
    for _ in range(18):
        env.step(torch.from_numpy(gentle()).to(DEV))
    torch.cuda.synchronize()
    assert int(env.metrics[8]) == 0
    for k in range(16):
        st = env.state.cpu().numpy().copy()
        ep = env.episode_len.cpu().numpy().copy()
        a = gentle()
        env.step(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        probe = {}
        OE.step(p, st, ep, f.oracle(), a, 8, 18 + k, probe=probe)
        got = env.state.cpu().numpy()
        q0 = st[3:7, :n]
        upright = (1.0 - 2.0 * (q0[1] ** 2 + q0[2] ** 2)) > 0.8
        assert upright.mean() > 0.9
        _, n_ex = PRED.check_state(got, st, probe, n, upright, loose=60.0, where=f"G6 step {k}")
        assert n_ex == 0, (k, n_ex)


def test_reset_heights_against_float64():
    """wl_elev_reset and wl_visual_reset_hf lift each spawn onto G1 -- over the field or the outside plane at -0.35 m: the root heights
    equal the rule applied to sample64(guard=True) within the sampler's bound"""
    from wheeledlab_amd.core import VisualDepthBatch
    f = HC.get("G1")
    n = 4096
    env = _elev(f, n, seed=17)
    st = env.state[:, :n].cpu().numpy()
    z, _, inside = R.sample64(f, st[0], st[1])
    ztol, _, _, _, ex_in = R.contact_bounds(f, st[0], st[1])
    want = np.maximum(F(env.p.reset_z), z + float(F(env.p.spawn_clearance)))
    ok = ~ex_in
    assert (np.abs(st[2] - want)[ok] <= ztol[ok] + 1e-6).all(), float(np.abs(st[2] - want)[ok].max())
    assert inside.any() and (~inside).any() and (st[2][~inside] == F(env.p.reset_z)).all()
    vd = VisualDepthBatch(1024, device=DEV, seed=3, heightfield=f.device(DEV))
    vd.reset()
    torch.cuda.synchronize()
    assert vd.hf.outside_z == F(f.outside_z) and vd.camera.hf.outside_z == F(f.outside_z)
    st = vd.state[:, :1024].cpu().numpy()
    z, _, inside = R.sample64(f, st[0], st[1])
    ztol, _, _, _, ex_in = R.contact_bounds(f, st[0], st[1])
    want = z + float(F(vd.p.reset_z))
    assert (np.abs(st[2] - want)[~ex_in] <= ztol[~ex_in] + 1e-6).all(), float(np.abs(st[2] - want)[~ex_in].max())
    assert inside.any() and (~inside).any()                      # spawns south of y0 = -7.15 land on the outside plane


@pytest.mark.parametrize("lanes", [4, 1])
def test_visual_depth_steps_on_g1(lanes):
    """the visual-depth task's step and reset on G1 (outside_z -0.35 for the contacts, the resets and the camera) against the oracle"""
    from wheeledlab_amd.core import VisualDepthBatch
    f = HC.get("G1")
    n = 128
    env = VisualDepthBatch(n, device=DEV, seed=5, heightfield=f.device(DEV), max_depth=20.0)
    env.set_lanes(lanes)
    env.reset()
    trav = env.trav_map.cpu().numpy().astype(bool)
    cells = OV.spawn_cells(trav)
    p = OV.visual_params()
    p.map_rows, p.map_cols = int(env._map.rows), int(env._map.cols)
    rng = np.random.RandomState(0)
    excused = img_bad = 0
    for k in range(8):
        st = env.state.cpu().numpy().copy()
        ep = env.episode_len.cpu().numpy().copy()
        if k == 4:
            ep[: n // 4] = p.max_episode_length - 1          # time-outs: resets onto the field and the outside plane
            env.episode_len.copy_(torch.from_numpy(ep))
        a = rng.uniform(-1, 1, (n, 2)).astype(F)
        a[:, 0] = np.abs(a[:, 0]) * 0.7 + 0.2
        obs, rew, term, trunc = env.step(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        probe = {}
        o_obs, o_rew, o_term, o_trunc, _ = OV.step(p, st, ep, trav, cells, a, 5, k, hf=f.oracle(), max_depth=20.0, probe=probe)
        got = env.state.cpu().numpy()
        np.testing.assert_array_equal(trunc.cpu().numpy(), o_trunc)
        bad = term.cpu().numpy() != o_term
        assert bad.sum() <= 1
        ok, n_ex = PRED.check_state(got, st, probe, n, ~bad, where=f"visual G1 step {k}")
        excused += n_ex
        want = OV.observe_depth(p, got[:, :n].copy(), f.oracle(), 20.0)
        o = obs.cpu().numpy()
        img_bad += int((np.abs(o[:, :4800] - want[:, :4800]) > 2e-4 + 2e-4 * np.abs(want[:, :4800])).sum())
    print(f"visual G1 lanes {lanes}: {excused} env-steps excused, {img_bad} depth pixels off")
    assert excused <= 3 and img_bad < 1e-3 * 8 * n * 4800
    assert int(env.metrics[9]) > 0

"""Visual task on the GPU: traversability lookup / rewards / termination vs the reference's golden outputs, fused step
+ ray-cast camera observation vs the oracle, augmentation chain, depth extension.  Everything through the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import visual_mdp as VM
from oracle import visual_step as OS
from tests import parity_predicates as PRED
from tests.parity_predicates import edge_golden  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def trav(golden):
    g = golden("visual_trav")
    return np.unpackbits(g["full_map_packed"])[: 500 * 500].reshape(500, 500).astype(bool)


def _batch(n, trav, seed=3):
    from wheeledlab_amd.core import VisualBatch
    env = VisualBatch(n, device=DEV, seed=seed, trav_map=trav)
    env.reset()
    torch.cuda.synchronize()
    return env


def test_visual_mdp_kernel_matches_reference_golden(golden, trav):
    env = _batch(64, trav)
    for name, key_pos in (("visual_mdp", "pos"), ("visual_trav", "xy")):
        g = golden(name)
        pos = g[key_pos]
        n = pos.shape[0]
        stride = ((n + 63) // 64) * 64
        P = torch.zeros(3, stride)
        P[: pos.shape[1], :n] = torch.from_numpy(np.ascontiguousarray(pos.T))
        vb = torch.zeros(3, stride)
        if "lin_vel_b" in g:
            vb[:, :n] = torch.from_numpy(np.ascontiguousarray(g["lin_vel_b"].T))
        P, vb = P.to(DEV), vb.to(DEV)
        terms = torch.zeros(2, stride, device=DEV)
        oom = torch.zeros(n, dtype=torch.uint8, device=DEV)
        xi = torch.zeros(n, dtype=torch.int32, device=DEV)
        yi = torch.zeros(n, dtype=torch.int32, device=DEV)
        rc = env.lib.wl_visual_mdp(C.byref(env.p), C.byref(env._map), n, stride, P.data_ptr(), vb.data_ptr(), terms.data_ptr(),
                                   oom.data_ptr(), xi.data_ptr(), yi.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        if name == "visual_mdp":                       # outputs of the reference's reward / termination functions
            np.testing.assert_array_equal(terms[0, :n].cpu().numpy(), g["traversable_reward"])
            np.testing.assert_array_equal(terms[1, :n].cpu().numpy(), g["forward_vel"])
            np.testing.assert_array_equal(oom.cpu().numpy().astype(bool), g["out_of_map"])
        else:                                          # outputs of TraversabilityHashmapUtil.get_map_id / get_traversability
            np.testing.assert_array_equal(xi.cpu().numpy(), g["x_idx"])   # bit-exact incl. cell-boundary cases
            np.testing.assert_array_equal(yi.cpu().numpy(), g["y_idx"])
            np.testing.assert_array_equal(terms[0, :n].cpu().numpy() > 0, g["trav"])


def test_visual_reset_and_camera_match_oracle(trav):
    env = _batch(128, trav, seed=11)
    st = env.state.cpu().numpy()
    p = OS.visual_params()
    o = np.zeros_like(st)
    o[3] = 1
    o[23:27] = st[23:27]
    ep = np.ones(st.shape[1], np.int32)
    cells = OS.spawn_cells(trav)
    OS.reset_envs(p, o, ep, cells, np.arange(128), 11, 0)
    np.testing.assert_allclose(st[:, :128], o[:, :128], rtol=1e-6, atol=2e-6)
    assert trav[VM.get_map_id(st[0, :128], st[1, :128])[1], VM.get_map_id(st[0, :128], st[1, :128])[0]].all()   # spawned on the path
    # a masked reset over preloaded rows: the same values, exactly, in the masked envs and nothing anywhere else
    PRED.check_masked_reset(_batch(70, trav, seed=11), st)
    # (brightness, contrast, blur sigma, contrast before brightness): torchvision's ColorJitter draws the op order per call
    for aug in ((1.0, 1.0, 0.0, 0), (1.4, 0.85, 1.7, 0), (0.5, 1.15, 0.4, 0), (1.4, 0.85, 1.7, 1), (1.7, 1.2, 0.0, 1), (0.4, 1.2, 3.0, 1)):
        env.p.brightness, env.p.contrast, env.p.blur_sigma, env.p.contrast_first = aug
        p.brightness, p.contrast, p.blur_sigma, p.contrast_first = aug
        obs = env.observe().cpu().numpy()
        want = OS.observe(p, st[:, :128].copy(), trav)
        assert obs.shape == (128, 3208)
        d = np.abs(obs - want)
        # pixel rays that graze a cell boundary may resolve to the neighbouring cell (fp32 ray maths): count them
        bad = (d[:, :3200] > 2e-3).mean()
        assert bad < 2e-3, (aug, bad)
        assert d[:, 3200:].max() < 1e-5
        assert np.median(d[:, :3200]) < 1e-5
    # the two orders really differ (brightness 1.4 pushes the sky band over the clamp before / after the blend)
    env.p.brightness, env.p.contrast, env.p.blur_sigma, env.p.contrast_first = 1.4, 0.85, 1.7, 0
    a0 = env.observe().clone()
    env.p.contrast_first = 1
    assert (env.observe() - a0).abs().max() > 1e-2
    # the image shows something: both colours and the sky band are present
    env.p.brightness, env.p.contrast, env.p.blur_sigma, env.p.contrast_first = 1.0, 1.0, 0.0, 0
    img = env.observe()[:, :3200]
    assert (img > 0.9).any() and (img < -0.9).any() and ((img.abs() < 0.05).float().mean() > 0.1)


@pytest.mark.parametrize("lanes", [4, 1])
def test_visual_fused_step_matches_oracle_single_steps(trav, lanes):
    n = 256
    env = _batch(n, trav, seed=5)
    env.set_lanes(lanes)
    p = OS.visual_params()
    cells = OS.spawn_cells(trav)
    rng = np.random.RandomState(0)
    excused = 0
    for k in range(12):
        st = env.state.cpu().numpy().copy()
        ep = env.episode_len.cpu().numpy().copy()
        if k == 6:
            ep[: n // 4] = 49
            st[0, n // 4: n // 2] = 124.9                      # about to leave the map -> out_of_map termination
            st[7, n // 4: n // 2] = 3.0
            env.episode_len.copy_(torch.from_numpy(ep))
            env.state.copy_(torch.from_numpy(st))
        a = rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32)
        met0 = env.metrics.cpu().numpy().astype(np.float64)
        obs, rew, term, trunc = env.step(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        met = np.zeros(16)
        probe = {}
        o_obs, o_rew, o_term, o_trunc, info = OS.step(p, st, ep, trav, cells, a, 5, k, met, probe=probe)
        got = env.state.cpu().numpy()
        np.testing.assert_array_equal(trunc.cpu().numpy(), o_trunc)
        bad = term.cpu().numpy() != o_term
        assert bad.sum() <= 1
        ok = ~bad
        # an env may miss the tight bound only if the ORACLE's step had a wheel within reach of making / breaking contact (the 10 cm spawn
        # drop; tests/parity_predicates.py) -- measured in round 6: none does
        ok, n_ex = PRED.check_state(got, st, probe, n, ok, where=f"step {k}")
        excused += n_ex
        assert PRED.state_error(got, st, n)[:, ok].max() <= 1.0, k
        cell_flip = np.abs(rew.cpu().numpy() - o_rew) > 0.5    # +-1 traversability flips exactly on a cell edge
        assert (cell_flip & ok).sum() <= 1
        sel = ok & ~cell_flip
        np.testing.assert_allclose(rew.cpu().numpy()[sel], o_rew[sel], rtol=2e-3, atol=2e-3)
        d = np.abs(obs.cpu().numpy() - o_obs)[sel]
        assert d[:, 3200:].max() < 3e-3 and (d[:, :3200] > 2e-3).mean() < 5e-3
        if not bad.any():
            dm = env.metrics.cpu().numpy().astype(np.float64) - met0
            np.testing.assert_allclose(dm[8:16], met[8:16], atol=1e-3)
    assert env.metrics[10] > 0 and env.metrics[9] > 0          # both out_of_map and time_out were exercised
    assert excused <= 2, excused                               # (until round 5, 40 explicit sub-steps: up to 2 % of the envs per step, by a count)


def test_visual_full_size_properties_and_depth(trav):
    n = 4096
    env = _batch(n, trav, seed=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    resets = 0
    for k in range(60):
        env.sample_augmentation()
        obs, rew, term, trunc = env.step(torch.rand(n, 2, device=DEV, generator=g) * 2 - 1)
        resets += int((term | trunc).sum())
    torch.cuda.synchronize()
    assert torch.isfinite(env.state[:, :n]).all() and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert (obs[:, :3200].abs() <= 1.0 + 1e-6).all() and (obs[:, 3206:].abs() <= 1).all()
    assert (env.episode_len[:n] < 50).all() and env.metrics[8] == resets and env.metrics[14] == 0
    # depth extension on a flat heightfield == analytic ray/plane distance
    flat = (np.zeros((64, 64), np.float32), -200.0, -200.0, 400.0 / 63)
    dep = env.depth(flat, max_depth=30.0)
    assert dep.shape == (n, 60, 80) and torch.isfinite(dep).all()
    st = env.state[:, :n].cpu().numpy()
    e = int(np.argmax((np.abs(st[0]) < 100) & (np.abs(st[1]) < 100)))
    from oracle.mathlib import matrix_from_quat
    R = matrix_from_quat(st[3:7, e][None])[0]
    o = st[0:3, e] + R @ np.array(list(env.p.cam_pos), np.float32)
    row, col = 50, 40
    d_b = np.array([1.0, -((col + 0.5 - env.p.cx) / env.p.fx), -((row + 0.5 - env.p.cy) / env.p.fy)], np.float32)
    d_w = R @ d_b
    assert d_w[2] < 0
    assert abs(float(dep[e, row, col]) - (-o[2] / d_w[2])) < 0.03


@pytest.mark.parametrize("n", [300, 1500, 4100])
@pytest.mark.parametrize("aug", [(1.0, 1.0, 0.0), (1.3, 0.9, 1.2)])
def test_step_observation_is_the_observation_of_the_stored_state(trav, n, aug):
    """The observation a step returns must be the observation of the state the step stored (wl_visual_observe on it) -- bit for
    bit, every env in its own row, at env counts that take each of the quad launcher's block sizes and leave a partly filled
    last block -- and the quad form's step must agree with the lane form's."""
    ea, eb = _batch(n, trav, seed=9), _batch(n, trav, seed=9)
    eb.set_lanes(1)
    for e in (ea, eb):
        e.p.brightness, e.p.contrast, e.p.blur_sigma = aug
        e.episode_len[:n] = torch.randint(0, 49, (n,), device=DEV, dtype=torch.int32, generator=torch.Generator(device=DEV).manual_seed(2))
    g = torch.Generator(device=DEV).manual_seed(6)
    dones = 0
    for k in range(6):
        a = torch.rand(n, 2, device=DEV, generator=g) * 2.4 - 1.2
        obs, rew, term, trunc = ea.step(a)
        got = obs.clone()
        dones += int((term | trunc).sum())
        assert torch.equal(got, ea.observe()), k
        eb.state.copy_(ea.state)                    # same start for the next comparison
        eb.episode_len.copy_(ea.episode_len)
        if k < 5:
            a2 = torch.rand(n, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(100 + k)) * 2 - 1
            sa, ep = ea.state.clone(), ea.episode_len.clone()
            oa = [t.clone() for t in ea.step(a2)]
            eb.step_count = ea.step_count - 1
            ob = eb.step(a2)
            torch.testing.assert_close(ea.state[:13, :n], eb.state[:13, :n], rtol=5e-4, atol=5e-4)
            torch.testing.assert_close(ea.state[17:21, :n], eb.state[17:21, :n], rtol=5e-4, atol=5e-4)
            # wheel spin = contact speed / r: the body rows' 5e-4 m/s is 1e-2 rad/s at r = 0.05 m
            torch.testing.assert_close(ea.state[13:17, :n], eb.state[13:17, :n], rtol=5e-4, atol=1e-2)
            assert torch.equal(oa[2], ob[2]) and torch.equal(oa[3], ob[3]) and torch.equal(ea.episode_len, eb.episode_len)
            torch.testing.assert_close(oa[1], ob[1], rtol=2e-3, atol=2e-3)
            assert ((oa[0] - ob[0]).abs()[:, :3200] > 2e-3).float().mean() < 5e-3
            dones += int((oa[2] | oa[3]).sum())
    assert dones > 0


@pytest.mark.parametrize("n,K,slots,aug", [(4096, 10, 1, (1.2, 0.9, 1.5)), (1000, 7, 1, (1.0, 1.0, 0.0)), (256, 5, 4, (0.7, 1.1, 0.6))])
def test_persistent_visual_rollout_equals_stepping(trav, n, K, slots, aug):
    """wl_visual_rollout_persistent (K steps in one launch: the camera of step k rendered by twelve wavefronts per block while
    a thirteenth integrates step k + 1; render groups meeting through an LDS counting barrier) against wl_visual_rollout
    (a launch per step): every output row and the final state bit for bit, the episode metrics to summation order -- incl.
    in-rollout resets, a partly filled last block (n = 1000), the metric ring, with and without the augmentation"""
    from wheeledlab_amd.core import VisualBatch
    ea = VisualBatch(n, device=DEV, seed=21, trav_map=trav, metrics_slots=slots)
    eb = VisualBatch(n, device=DEV, seed=21, trav_map=trav, metrics_slots=1)
    g = torch.Generator(device=DEV).manual_seed(4)
    for e in (ea, eb):
        e.reset()
        e.p.brightness, e.p.contrast, e.p.blur_sigma = aug
        e.episode_len[:n] = torch.randint(0, 49, (n,), device=DEV, dtype=torch.int32, generator=torch.Generator(device=DEV).manual_seed(1))
    a = torch.rand(K, n, 2, device=DEV, generator=g) * 2 - 1
    outs = []
    for e, persistent in ((ea, True), (eb, False)):
        obs = torch.zeros(K, n, e.OBS_DIM, device=DEV)
        rew = torch.zeros(K, n, device=DEV)
        term = torch.zeros(K, n, dtype=torch.bool, device=DEV)
        trunc = torch.zeros(K, n, dtype=torch.bool, device=DEV)
        dones = torch.zeros(K, n, dtype=torch.long, device=DEV)
        e.rollout(a, obs, rew, term, trunc, dones_out=dones, persistent=persistent)
        outs.append((obs, rew, term, trunc, dones))
    torch.cuda.synchronize()
    for x, y, name in zip(outs[0], outs[1], ("obs", "reward", "terminated", "truncated", "dones")):
        assert torch.equal(x, y), name
    assert torch.equal(ea.state, eb.state) and torch.equal(ea.episode_len, eb.episode_len) and ea.step_count == eb.step_count == K
    assert int(outs[0][4].sum()) > 0
    ma, mb = ea.metrics_raw.sum((0, 1)), eb.metrics_raw.sum((0, 1))
    if slots > 1:
        assert float(ea.metrics_raw[1:].abs().sum()) == 0.0
    torch.testing.assert_close(ma, mb, rtol=1e-5, atol=1e-3)
    assert torch.equal(ma[8:12], mb[8:12]) and float(ma[8]) == float(outs[0][4].sum())
    # and with too few rows per step the launch is refused (the camera runs a step behind the physics)
    rc = ea.lib.wl_visual_rollout_persistent(C.byref(ea.p), C.byref(ea._bufs), C.byref(ea._map), a.data_ptr(), C.byref(ea._out), 0, 0, 2,
                                             ea.seed, ea.step_count, None)
    assert rc == -1      # WL_EINVAL


@pytest.mark.parametrize("lanes", [4, 1])
def test_settled_cars_need_no_contact_excuse(trav, lanes):
    """Companion of test_visual_fused_step_matches_oracle_single_steps (which excuses up to 2 % of envs per step as wheel
    touch-downs of the 10 cm spawn drop): no resets here (no time-out; nobody reaches the map's edge), the cars settle for 6
    steps, and then the excused set must be EMPTY for 24 steps in both forms of the kernel."""
    n = 256
    env = _batch(n, trav, seed=8)
    env.set_lanes(lanes)
    p = OS.visual_params()
    cells = OS.spawn_cells(trav)
    env.p.max_episode_length = p.max_episode_length = 10 ** 9
    env.state[0:2, :n] *= 0.5                                   # away from the map's edge
    rng = np.random.RandomState(1)
    for _ in range(6):
        env.step(torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)).to(DEV))
    torch.cuda.synchronize()
    assert int(env.metrics[8]) == 0
    for k in range(24):
        st = env.state.cpu().numpy().copy()
        ep = env.episode_len.cpu().numpy().copy()
        # moderate driving: at ground friction 2.0 full-lock turns at full throttle lift the inner wheels -- a contact break of
        # its own, which the other test covers
        a = np.stack([rng.uniform(-0.2, 0.7, n), rng.uniform(-0.5, 0.5, n)], -1).astype(np.float32)
        obs, rew, term, trunc = env.step(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        o_obs, o_rew, o_term, o_trunc, info = OS.step(p, st, ep, trav, cells, a, 8, 6 + k)
        got = env.state.cpu().numpy()
        assert not term.any() and not trunc.any() and not o_term.any() and not o_trunc.any()
        err = PRED.state_error(got, st, n)
        touchy = err.max(0) > 1.0
        assert touchy.sum() == 0, (k, int(touchy.sum()), float(err.max()))
        cell_flip = np.abs(rew.cpu().numpy() - o_rew) > 0.5    # +-1 traversability flips exactly on a cell edge
        assert cell_flip.sum() <= 1
        np.testing.assert_allclose(rew.cpu().numpy()[~cell_flip], o_rew[~cell_flip], rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("aug", [(1.0, 1.0, 0.0), (1.3, 0.9, 1.2)])
def test_lds_bit_map_camera_equals_the_byte_gather_camera(trav, aug):
    """the persistent rollout's camera with the whole traversability map in LDS as one bit per cell (WlTravMap.bits) against the
    camera that gathers bytes from the global map: every observation row bit for bit; observe() / step() (byte gathers either
    way) at env counts that leave the last block partly filled; a map too large for LDS takes the byte path"""
    from wheeledlab_amd.core import VisualBatch
    for n in (1, 64, 1000, 4097):
        ea, eb = _batch(n, trav, seed=4), _batch(n, trav, seed=4)
        eb._map.bits = None                              # byte gathers
        for e in (ea, eb):
            e.p.brightness, e.p.contrast, e.p.blur_sigma = aug
        assert torch.equal(ea.observe(), eb.observe())
        g = torch.Generator(device=DEV).manual_seed(0)
        for k in range(3):
            a = torch.rand(n, 2, device=DEV, generator=g) * 2 - 1
            oa, ob = ea.step(a), eb.step(a)
            assert all(torch.equal(x, y) for x, y in zip(oa, ob)), (n, k)
    K, n = 4, 512
    ea, eb = _batch(n, trav, seed=6), _batch(n, trav, seed=6)
    eb._map.bits = None
    a = torch.rand(K, n, 2, device=DEV) * 2 - 1
    outs = []
    for e in (ea, eb):
        e.p.brightness, e.p.contrast, e.p.blur_sigma = aug
        o = (torch.zeros(K, n, e.OBS_DIM, device=DEV), torch.zeros(K, n, device=DEV), torch.zeros(K, n, dtype=torch.bool, device=DEV),
             torch.zeros(K, n, dtype=torch.bool, device=DEV))
        e.rollout(a, *o, persistent=True)
        outs.append(o)
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    big = np.zeros((600, 600), bool)
    big[::3] = True
    eg = VisualBatch(100, device=DEV, seed=1, trav_map=big)      # 360 000 cells > the 512 x 512 the LDS form holds
    eg.reset()
    el = VisualBatch(100, device=DEV, seed=1, trav_map=big)
    el.reset()
    el._map.bits = None
    assert torch.equal(eg.observe(), el.observe()) and torch.isfinite(eg.observe()).all()


def test_visual_mdp_kernel_matches_reference_edges(edge_golden):
    """map_id / traversable_reward / out_of_map on five geometries (tests/golden/{,seed1000/}visual_*_edges.npz), through a WlTravMap
    built for each: bit for bit, but for the inputs tests/parity_predicates.py excuses (named and counted below); the non-square
    geometry is refused"""
    from wheeledlab_amd.core import VisualBatch
    t, m = edge_golden("visual_trav_edges"), edge_golden("visual_mdp_edges")
    trav = edge_golden.task_map()
    for gi, (rows, cols, rs, cs) in enumerate(t["geoms"]):
        rows, cols, p = int(rows), int(cols), f"g{gi}_"
        mp = trav if gi == 0 else np.unpackbits(t[p + "map_packed"])[: rows * cols].reshape(rows, cols).astype(bool)
        if rows != cols:
            with pytest.raises(ValueError):
                VisualBatch(8, device=DEV, trav_map=mp, spacing=(rs, cs))
            continue
        env = VisualBatch(64, device=DEV, seed=3, trav_map=mp, spacing=(rs, cs))
        for key in ("trav", "mdp"):
            pos = t[p + "xy"] if key == "trav" else m[p + "pos"]
            n = pos.shape[0]
            stride = ((n + 63) // 64) * 64
            P = torch.zeros(3, stride)
            P[: pos.shape[1], :n] = torch.from_numpy(np.ascontiguousarray(pos.T))
            vb = torch.zeros(3, stride)
            if key == "mdp":
                vb[:, :n] = torch.from_numpy(np.ascontiguousarray(m[p + "lin_vel_b"].T))
            P, vb = P.to(DEV), vb.to(DEV)
            terms = torch.zeros(2, stride, device=DEV)
            oom = torch.zeros(n, dtype=torch.uint8, device=DEV)
            xi = torch.zeros(n, dtype=torch.int32, device=DEV)
            yi = torch.zeros(n, dtype=torch.int32, device=DEV)
            assert env.lib.wl_visual_mdp(C.byref(env.p), C.byref(env._map), n, stride, P.data_ptr(), vb.data_ptr(), terms.data_ptr(),
                                         oom.data_ptr(), xi.data_ptr(), yi.data_ptr(), None) == 0
            torch.cuda.synchronize()
            ex_x = PRED.map_index_excused(pos[:, 0], rows, rs)
            ex_y = PRED.map_index_excused(pos[:, 1], cols, cs)
            ex_o = PRED.out_of_map_excused(pos[:, 0], rows, rs) | PRED.out_of_map_excused(pos[:, 1], cols, cs)
            print(f"{p}{key}: x index {ex_x.sum()}, y index {ex_y.sum()}, out_of_map {ex_o.sum()} of {n} excused")
            got_t = terms[0, :n].cpu().numpy()
            if key == "trav":
                np.testing.assert_array_equal(xi.cpu().numpy()[~ex_x], t[p + "x_idx"][~ex_x], err_msg=p)
                np.testing.assert_array_equal(yi.cpu().numpy()[~ex_y], t[p + "y_idx"][~ex_y], err_msg=p)
                ok = ~(ex_x | ex_y)
                np.testing.assert_array_equal((got_t > 0)[ok], t[p + "trav"][ok], err_msg=p)
            else:
                ok = ~(ex_x | ex_y)
                np.testing.assert_array_equal(got_t[ok], m[p + "traversable_reward"][ok], err_msg=p)
                np.testing.assert_array_equal(terms[1, :n].cpu().numpy(), m[p + "forward_vel"], err_msg=p)
                np.testing.assert_array_equal(oom.cpu().numpy().astype(bool)[~ex_o], m[p + "out_of_map"][~ex_o], err_msg=p)
            if gi == 0:   # the task's own geometry: only non-finite / beyond-2^63 inputs are excused
                wild = ~np.isfinite(pos[:, :2]).all(1) | (np.abs(pos[:, :2]) > 1e18).any(1)
                assert not ex_o.any() and wild[ex_x | ex_y].all()
    from wheeledlab_amd import _abi as A
    rect = A.WlTravMap(env.trav_map.data_ptr(), env.cells.data_ptr(), 40, 60, 10, 0.5, 0.5, None)   # refused before any launch
    assert env.lib.wl_visual_mdp(C.byref(env.p), C.byref(rect), 1, 64, P.data_ptr(), vb.data_ptr(), terms.data_ptr(), oom.data_ptr(),
                                 xi.data_ptr(), yi.data_ptr(), None) == -1

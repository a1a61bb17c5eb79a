"""Terrain curriculum on the GPU (WlElevParams.levels): every kernel form against tests/terrain_levels_reference.py and against
each other, through core.ElevBatch.  64 envs = one wavefront of lanes, 16 quads, 4 fused blocks; 70 for the ragged tail.  The
terrain is generated: 3 rows x 2 columns of 64 x 64-point tiles inside a 1 m frame."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import elev_step as OS
from tests import parity_predicates as PRED
from tests import terrain_levels_reference as REF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 9
ROWS, COLS = 3, 2
RESET_XY, CMD_XY = 1.0, 2.0          # inside the 3.2 m tiles; the goal squares of the outer tiles stay on the lattice
# (WlEnvBuffers.lanes = 2 is the drift task's second lane form; the elevation entry points refuse it with WL_EINVAL, as they always have)
FORMS = ("lanes1", "lanes4", "fused", "persistent", "collect")
ACTION = (0.5, 0.1)                  # every env, every step: what the collector's zero-weight actor puts out as its bias
PX, PZ, QW, VX, WHEEL, CMD_BX, TGT_X, CMD_TIMER = 0, 2, 3, 7, 13, 35, 37, 40      # rows of the state matrix (include/wheeledlab_amd.h WlStateField)


def gen_cfg():
    from wheeledlab_amd.envs.terrain_gen_cfg import TerrainGeneratorCfg
    return TerrainGeneratorCfg(seed=4, num_rows=ROWS, num_cols=COLS, size=(3.2, 3.2), border_width=1.0)


@pytest.fixture(scope="module")
def field():
    from wheeledlab_amd.core import generate_heightfield
    hf = generate_heightfield(gen_cfg(), DEV)
    torch.cuda.synchronize()
    return hf, (hf.heights.cpu().numpy().copy(), hf.x0, hf.y0, hf.cell, hf.outside_z)


def params():
    from wheeledlab_amd import params as PP
    p = PP.elev_params()
    p.reset_xy, p.cmd_xy = RESET_XY, CMD_XY
    return p


def oracle_params():
    p = OS.elev_params()
    p.reset_xy, p.cmd_xy = RESET_XY, CMD_XY
    return p


def make_env(hf, n, levels="gen", env_offset=0, world=None, seed=SEED):
    """levels: "gen" (from the generator cfg), None (off) or a TerrainLevels"""
    from wheeledlab_amd.core import ElevBatch, TerrainLevels
    tl = TerrainLevels(gen_cfg(), n, DEV, env_offset, world, None, seed) if levels == "gen" else levels
    env = ElevBatch(n, device=DEV, params=params(), seed=seed, env_offset=env_offset, heightfield=hf, terrain_levels=tl)
    env.reset()
    return env


def run(env, form, K):
    """K steps of ACTION in the given form -> (obs [K, n, 689], reward, terminated, truncated) on the host"""
    n = env.n
    a = torch.tensor(ACTION, device=DEV).expand(K, n, 2).contiguous()
    obs = torch.zeros(K, n, env.OBS_DIM, device=DEV)
    rew = torch.zeros(K, n, device=DEV)
    term, trunc = torch.zeros(K, n, dtype=torch.bool, device=DEV), torch.zeros(K, n, dtype=torch.bool, device=DEV)
    if form == "collect":
        from wheeledlab_amd.policy import RolloutStorage
        from wheeledlab_amd.rl.ppo import ActorCritic
        ac = ActorCritic(env.OBS_DIM, env.OBS_DIM, 2, activation="elu").to(DEV)
        with torch.no_grad():
            for q in ac.parameters():
                q.zero_()
            ac.std.fill_(1.0)
            ac.actor[-1].bias.copy_(torch.tensor(ACTION))
        view = ac.fused()
        view.planes = False
        st = RolloutStorage(K, n, env.OBS_DIM, 2, DEV)
        st.observations[0].copy_(env.observe())
        env.collect_rollout(view, st, start=0, count=K, deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(st.actions[:K], a)
        return st.observations[1:K + 1].cpu().numpy(), st.rewards[:K].cpu().numpy(), st.terminated[:K].cpu().numpy().astype(bool), \
            st.time_outs[:K].cpu().numpy().astype(bool)
    env.set_lanes({"lanes1": 1, "lanes4": 4}.get(form, 0))
    if form in ("persistent", "rollout"):
        env.rollout(a, obs, rew, term, trunc, persistent=form == "persistent")
    else:
        for k in range(K):
            o, r, t, u = env.step(a[k])
            obs[k], rew[k], term[k], trunc[k] = o, r, t, u
    torch.cuda.synchronize()
    return obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()


def snapshot(env):
    lv = None if env.levels is None else env.levels.level.cpu().numpy().copy()
    return env.state.cpu().numpy().copy(), env.episode_len.cpu().numpy().copy(), lv


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. off is off ----------------------------------------------------------------------------------------------------

def force_resets(env):
    """some envs end their episode in the next step (time-out), some resample their goal"""
    n = env.n
    env.episode_len[0:n:3] = env.p.max_episode_length - 1
    env.state[CMD_TIMER, 1:n:3] = 0.05


@pytest.mark.parametrize("form", FORMS)
def test_one_tile_at_the_origin_is_off(field, form):
    """The levels code on a 1 x 1 table whose origin is (0, 0) against the launch with the all-zero member: every output and row
    bit for bit, resets and resampled goals included.  (With the member zero the launchers pick the instantiations compiled
    without the levels code; that THOSE give the parent commit's values is what the existing parity and golden tests hold.)"""
    from wheeledlab_amd.core import TerrainLevels
    hf, _ = field
    n, K = 64, 3
    tl = TerrainLevels.from_tables(np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((1, 2), np.float32), 1, 1, DEV)
    outs = []
    for levels in (None, tl):
        env = make_env(hf, n, levels)
        assert bool(env.p.levels.level) == (levels is not None)
        force_resets(env)
        outs.append(run(env, form, K) + snapshot(env)[:2])
    assert same(outs[0], outs[1])
    assert (outs[0][2] | outs[0][3]).any()
    assert int(tl.level.abs().max()) == 0


# ---- 2. the outcome table, one step, every form -------------------------------------------------------------------------

CASES = {  # env -> (what is set up, level before, expected move)
    0: ("goal", 0, "up"), 1: ("goal", 1, "up"), 2: ("roll", 1, "down"), 3: ("roll", 0, "floor"), 4: ("low", 2, "down"),
    5: ("stuck", 1, "down"), 6: ("nan", 2, "down"), 7: ("nan", 0, "floor"), 8: ("timeout", 1, "stay"), 9: ("goal+roll", 0, "up"),
    10: ("goal", 2, "wrap"), 11: ("none", 2, "keep"), 12: ("timer", 1, "keep"), 13: ("goal", 2, "wrap"), 69: ("goal", 1, "up"),
}


def stage_cases(env):
    """write the table's states into a freshly reset env (rows as the kernels read them)"""
    n = env.n
    st, lv = env.state, env.levels.level
    lv[:] = torch.tensor([CASES.get(e, ("none", e % ROWS, "keep"))[1] for e in range(n)], dtype=torch.int32, device=DEV)
    env.reset()                                     # spawn on the tiles of THESE levels (a masked reset keeps them)
    # everybody rolls forward at 0.5 m/s: a car that spawns at rest under throttle spins its wheels and counts as stuck
    st[VX, :n], st[VX + 1, :n] = 0.5 * (1 - 2 * st[QW + 3, :n] ** 2), 0.5 * (2 * st[QW, :n] * st[QW + 3, :n])
    for e, (what, _, _) in CASES.items():
        if e >= n:
            continue
        if "goal" in what:                          # the command minus the world position is the goal vector (the task's quirk)
            st[CMD_BX, e], st[CMD_BX + 1, e] = st[PX, e], st[PX + 1, e]
        if "roll" in what:
            st[QW:QW + 4, e] = torch.tensor([0.70710678, 0.70710678, 0.0, 0.0], device=DEV)     # on its side, clear of the ground
            st[PZ, e] += 0.3
        if what == "low":                           # on the plane beyond the lattice, below the minimum height
            st[PX, e], st[PZ, e] = 40.0, 0.06
        if what == "stuck":                         # wheels spinning in the air
            st[PZ, e] = 3.0
            st[VX:VX + 3, e] = 0.0
            st[WHEEL:WHEEL + 4, e] = 30.0
        if what == "nan":
            st[VX, e] = float("nan")
        if what == "timeout":
            env.episode_len[e] = env.p.max_episode_length - 1
        if what == "timer":
            st[CMD_TIMER, e] = 0.05
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def outcome_reference(field):
    """the staged table stepped once by the reference, per n (computed once, shared by every form)"""
    hf, hf_np = field
    out = {}
    for n in (64, 70):
        env = make_env(hf, n)
        stage_cases(env)
        st, ep, lv = snapshot(env)
        stride = st.shape[1]
        levels = dict(level=np.zeros(stride, np.int32), type=np.zeros(stride, np.int32), origins=env.levels.origins.cpu().numpy(), rows=ROWS, cols=COLS)
        levels["level"][:n], levels["type"][:n] = lv, env.levels.type.cpu().numpy()
        a = np.zeros((stride, 2), np.float32)
        a[:] = ACTION
        st[:, n:] = 0
        st[QW, n:] = 1
        probe = {}
        lv0 = levels["level"].copy()
        o_obs, o_rew, o_term, o_trunc, info = REF.step(oracle_params(), st, ep, hf_np, a, SEED, 0, levels, probe=probe)
        out[n] = dict(state=st, ep=ep, level=levels["level"][:n].copy(), level0=lv0[:n], obs=o_obs[:n], rew=o_rew[:n], term=o_term[:n],
                      trunc=o_trunc[:n], probe=probe, origins=levels["origins"], type=levels["type"][:n])
    return out


@pytest.mark.parametrize("n", [64, 70])
def test_outcome_table(field, outcome_reference, n):
    hf, _ = field
    ref = outcome_reference[n]
    # the reference's own outcome is the table's (the staging does what it says)
    for e, (what, before, move) in CASES.items():
        if e >= n:
            continue
        after = int(ref["level"][e])
        assert {"up": after == before + 1, "down": after == before - 1, "floor": before == 0 and after == 0, "stay": after == before,
                "keep": after == before, "wrap": 0 <= after < ROWS}[move], (e, what, before, after)
        ended = bool(ref["term"][e] | ref["trunc"][e])
        assert ended == (move != "keep"), (e, what)
        if what == "timeout":
            assert ref["trunc"][e] and not ref["term"][e]
    first = None
    for form in FORMS:
        env = make_env(hf, n)
        stage_cases(env)
        start = snapshot(env)
        obs, rew, term, trunc = run(env, form, 1)
        got, ep, lv = snapshot(env)
        # levels and flags: exact
        np.testing.assert_array_equal(lv, ref["level"], err_msg=form)
        np.testing.assert_array_equal(term[0], ref["term"], err_msg=form)
        np.testing.assert_array_equal(trunc[0], ref["trunc"], err_msg=form)
        np.testing.assert_array_equal(ep[:n], ref["ep"][:n], err_msg=form)
        # state and observation: the bars of tests/test_gpu_elev_parity.py
        ok, n_ex = PRED.check_state(got, ref["state"], ref["probe"], n, np.ones(n, bool), where=form)
        assert n_ex <= 1, (form, n_ex)
        assert PRED.state_error(got, ref["state"], n)[:, ok].max() <= 1.0, form
        np.testing.assert_allclose(got[35:41, :n][:, ok], ref["state"][35:41, :n][:, ok], rtol=5e-4, atol=2e-3, err_msg=form)
        np.testing.assert_allclose(rew[0][ok], ref["rew"][ok], rtol=2e-3, atol=5e-2, err_msg=form)
        d = np.abs(obs[0] - ref["obs"])[ok]
        d[:, 2:5] = np.minimum(d[:, 2:5], np.abs(2 * np.pi - d[:, 2:5]))
        assert d[:, :13].max() < 3e-3, (form, d[:, :13].max())
        scan_bad = d[:, 13:] > 2e-3
        assert scan_bad.sum() <= 4 and scan_bad.any(1).sum() <= 2, (form, int(scan_bad.sum()))
        # spawns inside the env's tile, goals (reset or resampled) inside its goal square
        ended = term[0] | trunc[0]
        o = ref["origins"][lv.astype(np.int64) * COLS + ref["type"]]
        assert (np.abs(got[PX:PX + 2, :n].T - o)[ended] <= RESET_XY).all(), form
        redrawn = ended | (start[0][CMD_TIMER, :n] <= 0.1)
        assert redrawn[12] and not ended[12]
        assert (np.abs(got[TGT_X:TGT_X + 2, :n].T - o)[redrawn] <= CMD_XY).all(), form
        this = (obs, rew, term, trunc, got[:, :n], ep[:n], lv)
        if first is None:
            first = this
        else:
            assert same(first, this), f"{form} differs from {FORMS[0]}"


# ---- 3. continuity ----------------------------------------------------------------------------------------------------

def busy_env(hf, n, **kw):
    """an env whose next steps hold resets of every kind (the staged table) and later time-outs"""
    env = make_env(hf, n, **kw)
    if env.env_offset == 0 and n >= 64:
        stage_cases(env)
    env.episode_len[n // 2:n] = env.p.max_episode_length - torch.arange(1, n - n // 2 + 1, device=DEV, dtype=torch.int32) % 7 - 1
    return env


@pytest.mark.parametrize("form", ["rollout", "persistent", "collect"])
def test_k_steps_equal_single_steps(field, form):
    hf, _ = field
    n, K = 64, 8
    a, b = busy_env(hf, n), busy_env(hf, n)
    many = run(a, form, K)
    single = [run(b, "collect" if form == "collect" else "fused", 1) for _ in range(K)]
    single = tuple(np.concatenate([s[i] for s in single]) for i in range(4))
    assert same(many, single)
    assert same(snapshot(a), snapshot(b))
    assert len(np.unique(a.levels.level.cpu().numpy())) > 1


def test_two_shards_equal_the_batch(field):
    hf, _ = field
    K = 4
    whole = make_env(hf, 64)
    halves = [make_env(hf, 32, env_offset=o, world=64) for o in (0, 32)]
    for env in [whole] + halves:
        env.episode_len[:] = env.p.max_episode_length - 2
    assert torch.equal(torch.cat([h.levels.level for h in halves]), whole.levels.level)
    assert torch.equal(torch.cat([h.levels.type for h in halves]), whole.levels.type)
    w = run(whole, "fused", K)
    h = [run(x, "fused", K) for x in halves]
    assert same(w, tuple(np.concatenate([h[0][i], h[1][i]], 1) for i in range(4)))
    assert torch.equal(torch.cat([x.levels.level for x in halves]), whole.levels.level)
    assert torch.equal(torch.cat([x.state[:, :32] for x in halves], 1), whole.state[:, :64])


def test_masked_reset_keeps_levels_and_spawns_on_the_tile(field):
    hf, _ = field
    env = make_env(hf, 64)
    env.levels.level[:] = torch.arange(64, device=DEV, dtype=torch.int32) % ROWS
    before, lv = env.state.clone(), env.levels.level.clone()
    mask = torch.arange(64, device=DEV) % 2 == 0
    env.step_count = 5
    env.reset(mask)
    torch.cuda.synchronize()
    assert torch.equal(env.levels.level, lv)
    assert torch.equal(env.state[:23, 1:64:2], before[:23, 1:64:2])
    o = env.levels.env_origins_xy()
    assert ((env.state[PX:PX + 2, :64].T - o).abs()[mask] <= RESET_XY).all()
    assert ((env.state[TGT_X:TGT_X + 2, :64].T - o).abs()[mask] <= CMD_XY).all()


def test_abi_refusals_launch_nothing(field):
    from wheeledlab_amd import _abi as A
    hf, _ = field
    env = make_env(hf, 64)
    good = env.p.levels
    start = snapshot(env)
    a = torch.zeros(64, 2, device=DEV)

    def status(**change):
        p = type(env.p)()
        C.pointer(p)[0] = env.p
        lv = A.WlTerrainLevels(good.level, good.type, good.origins, good.rows, good.cols)
        for k, v in change.items():
            setattr(lv, k, v)
        p.levels = lv
        rcs = [env.lib.wl_elev_step(C.byref(p), *env._args, a.data_ptr(), C.byref(env._out), env.seed, 0, env._stream()),
               env.lib.wl_elev_reset(C.byref(p), *env._args, None, env.seed, 0, env._stream()),
               env.lib.wl_elev_rollout_persistent(C.byref(p), *env._args, a.data_ptr(), C.byref(env._out), 0, 0, 1, env.seed, 0, env._stream())]
        assert len(set(rcs)) == 1
        return rcs[0]

    EINVAL, EALIGN = -1, -3
    assert status(type=None) == EINVAL and status(origins=None) == EINVAL
    assert status(rows=0) == EINVAL and status(cols=0) == EINVAL and status(rows=-1) == EINVAL
    assert status(level=None) == EINVAL                      # all or nothing: tables without levels
    assert status(level=good.level + 2) == EALIGN and status(type=good.type + 1) == EALIGN and status(origins=good.origins + 2) == EALIGN
    torch.cuda.synchronize()
    assert same(start, snapshot(env))


# ---- 4. the env surface -------------------------------------------------------------------------------------------------

def make_levels_env(n=64, seed=7):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.tasks.elevation import MushrElevationTerrainLevelsEnvCfg
    cfg = MushrElevationTerrainLevelsEnvCfg()
    cfg.sim.device, cfg.num_envs, cfg.scene.num_envs, cfg.seed = DEV, n, n, seed
    return registry.make("Isaac-MushrElevationRL-v0", cfg=cfg)


def test_env_surface():
    from wheeledlab_amd.envs import terrain_levels as TL
    env = make_levels_env()
    env.reset()
    n, b, t = 64, env._batch, env.scene.terrain
    gen = t.terrain_generator
    assert t.terrain_type == "generator" and t.max_init_terrain_level == 1
    assert t.terrain_levels.data_ptr() == b.levels.level.data_ptr() and t.terrain_types.dtype == torch.int32
    assert int(t.terrain_levels.max()) <= 1
    level0, types = TL.initial_assignment(gen, n, 0, n, 1, 7)
    np.testing.assert_array_equal(t.terrain_levels.cpu().numpy(), level0)
    np.testing.assert_array_equal(t.terrain_types.cpu().numpy(), types)
    assert tuple(t.terrain_origins.shape) == (5, 5, 3) and tuple(env.scene.env_origins.shape) == (n, 3)
    np.testing.assert_array_equal(t.terrain_origins[..., :2].reshape(-1, 2).cpu().numpy(), TL.tile_origins(gen))
    # forced outcomes: the first 16 envs at their goals (four of them on the top row: the wrap), the next 16 on their sides in the
    # air, 16 timing out, 16 running on -- and the same step by the reference
    t.terrain_levels[:4] = 4
    env.reset()                                     # onto the tiles of these levels
    st = b.state
    st[CMD_BX, :16], st[CMD_BX + 1, :16] = st[PX, :16], st[PX + 1, :16]
    st[QW:QW + 4, 16:32] = torch.tensor([0.70710678, 0.70710678, 0.0, 0.0], device=DEV)[:, None]
    st[PZ, 16:32] += 0.3
    b.episode_len[32:48] = env.max_episode_length - 1
    before = t.terrain_levels.clone()
    torch.cuda.synchronize()
    r_state, r_ep, r_lv = snapshot(b)
    ref_levels = dict(level=r_lv, type=t.terrain_types.cpu().numpy(), origins=b.levels.origins.cpu().numpy(), rows=5, cols=5)
    rp = OS.elev_params()
    rp.reset_xy, rp.cmd_xy = 1.5, 3.5
    hf_np = (b.hf.heights.cpu().numpy(), b.hf.x0, b.hf.y0, b.hf.cell, b.hf.outside_z)
    _, _, r_term, r_trunc, _ = REF.step(rp, r_state, r_ep, hf_np, np.zeros((n, 2), np.float32), b.seed, b.step_count, ref_levels)
    _, _, term, trunc, extras = env.step(torch.zeros(n, 2, device=DEV))
    assert bool(term[:32].all()) and bool(trunc[32:48].all()) and not bool((term | trunc)[48:].any())
    np.testing.assert_array_equal(term.cpu().numpy(), r_term)
    np.testing.assert_array_equal(trunc.cpu().numpy(), r_trunc)
    np.testing.assert_array_equal(t.terrain_levels.cpu().numpy(), ref_levels["level"])
    want = before.clone()                            # ... which is the rule: up, down to the floor, stay; past the top a uniform row
    want[4:16] += 1
    want[16:32] = (want[16:32] - 1).clamp(min=0)
    assert torch.equal(t.terrain_levels[4:], want[4:]) and 0 <= int(t.terrain_levels[:4].min()) and int(t.terrain_levels.max()) < 5
    o = t.terrain_origins[t.terrain_levels.long(), t.terrain_types.long()]
    assert torch.equal(env.scene.env_origins, o) and torch.equal(t.env_origins, o)
    assert bool(((st[PX:PX + 2, :n].T - o[:, :2]).abs()[:48] <= 1.5).all())
    assert bool(((st[TGT_X:TGT_X + 2, :n].T - o[:, :2]).abs() <= 3.5).all())
    z = b.hf.heights[((o[:, 1] - b.hf.y0) / b.hf.cell).round().long(), ((o[:, 0] - b.hf.x0) / b.hf.cell).round().long()]
    assert bool((o[:, 2] - z).abs().max() < 0.05)
    assert "Curriculum/terrain_levels" in extras["log"]
    mean = float(t.terrain_levels.float().mean())
    assert float(extras["log"]["Curriculum/terrain_levels"]) == mean
    assert env.episode_log_summary(1)["Curriculum/terrain_levels"] == mean
    kept = t.terrain_levels.clone()
    env.regenerate_terrain()
    assert torch.equal(t.terrain_levels, kept) and torch.equal(env.scene.env_origins[:, :2], o[:, :2])


def test_host_validation():
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.tasks.elevation import MushrElevationTerrainLevelsEnvCfg

    def cfg(**kw):
        c = MushrElevationTerrainLevelsEnvCfg()
        c.sim.device = DEV
        return c

    c = cfg()
    c.scene.terrain.terrain_type, c.scene.terrain.terrain_generator = "heightfield", None
    with pytest.raises(ValueError, match="generator"):
        flatten_cfg(c)
    c = cfg()
    c.scene.terrain.terrain_generator.curriculum = False
    with pytest.raises(ValueError, match="curriculum"):
        flatten_cfg(c)
    c = cfg()
    c.events.set_goal.params["pose_range"].update(x=(-4.5, 4.5), y=(-4.5, 4.5))
    with pytest.raises(ValueError, match="reset_xy"):
        flatten_cfg(c)
    c = cfg()
    c.commands.goal_pose.ranges.pos_x = c.commands.goal_pose.ranges.pos_y = (-4.5, 4.5)
    with pytest.raises(ValueError, match="cmd_xy"):
        flatten_cfg(c)
    assert flatten_cfg(cfg()).extra["terrain_levels"]["name"] == "terrain_levels"


# ---- 5. the training path ------------------------------------------------------------------------------------------------

OVERRIDES = ["env_setup.num_envs=64", "env.scene.terrain.terrain_type=generator", "env.scene.terrain.terrain_generator={}",
             "env.scene.terrain.max_init_terrain_level=1", "env.events.set_goal.params.pose_range.x=(-1.5,1.5)",
             "env.events.set_goal.params.pose_range.y=(-1.5,1.5)", "env.commands.goal_pose.ranges.pos_x=(-3.5,3.5)",
             "env.commands.goal_pose.ranges.pos_y=(-3.5,3.5)", "env.curriculum.terrain_levels=terrain_levels_goal"]


def test_two_ppo_iterations_log_the_term():
    """the env as scripts/train_rl.py builds it from overrides alone (README), through the collector launch"""
    from wheeledlab_amd import registry
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    run_cfg = resolve_run("RSS_ELEV_CONFIG", OVERRIDES + [f"train.device={DEV}"])
    env = registry.make(run_cfg.env_setup.task_name, cfg=run_cfg.env)
    assert env._batch.levels is not None and env._batch.levels.max_init_terrain_level == 1
    assert env.can_collect_rollout()
    env.action_space.low, env.action_space.high = -1.0, 1.0
    torch.manual_seed(0)
    launches, collect = [], env._batch.collect_rollout
    env._batch.collect_rollout = lambda *a, **k: (launches.append(k.get("count")), collect(*a, **k))[1]
    runner = OnPolicyRunner(RslRlVecEnvWrapper(ClipAction(env)), registry.load_cfg_from_registry("Isaac-MushrElevationRL-v0", "rsl_rl_cfg_entry_point"),
                            device=DEV)
    hist = runner.learn(2, verbose=False)
    assert len(hist) == 2 and all(np.isfinite(h["value_function"]) for h in hist)
    assert len(launches) >= 2                                  # the collector launch, not stepping
    lv = env.scene.terrain.terrain_levels
    assert 0 <= int(lv.min()) and int(lv.max()) < 5
    assert all("Curriculum/terrain_levels" in h for h in hist)
    assert hist[-1]["Curriculum/terrain_levels"] == float(lv.float().mean())       # nothing has stepped since the runner logged it

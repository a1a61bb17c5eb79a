"""Every kernel form of the policy step against the float64 reference of tests/policy_reference.py: the actor mean and the
critic's value (the stored old log-prob's mean and v_old), the Gaussian draw, the log-prob, at the shapes where each
launcher instantiation runs and on rows built to expose one feature, one plane or one kink at a time.

  * f32 kernel (wl_actor_critic_act), every (KS, RT): against float64 at the form's tau.
  * bf16 one launch / two launches (wl_actor_critic_act_planes, reserved 0 / 1) and form 2 (values_batched): against the
    split-exact model at the accumulation tau, and against exact float64 at tau + SPLIT_STAGE.
  * probe tails (w2 = I, b2 = 0, w3 selecting units): every output is one layer-1 pre-activation, held to the layer-1 tau.
  * the draw against std z64 from the Philox uniforms, at keys that reach r = 0, the largest r and the zeros of sin / cos;
    the log-prob against float64 from the kernel's own a and mu; deterministic = 1 gives a == mu bit for bit.
  * wl_mlp_forward, the first step of wl_drift_rollout_policy and one-step wl_elev_collect_rollout launches likewise.
Each test prints, per form, the worst ratio |g - g64| / (tau m + floor) and the number of impulse / probe checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_reference as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, STEP, OFF = 42, 99, 512
STD = (0.7, 1.3)


def _ac(nets: dict, D: int, activation: str, std=STD):
    from wheeledlab_amd.policy import ActorCritic
    ac = ActorCritic(D, 2, activation, device=DEV, seed=0)
    _load(ac, nets)
    ac.std.copy_(torch.tensor(std, dtype=torch.float32))
    return ac


def _load(ac, nets: dict):
    for name in ("actor", "critic"):
        m = getattr(ac, name)
        for k in P.FIELDS:
            getattr(m, k).copy_(nets[name][k].reshape(getattr(m, k).shape))


def _run(ac, obs, form, deterministic=False, seed=SEED, step=STEP, off=OFF, planes_fresh=False):
    """one policy step in the named form -> CPU (a, mu, logp, value)"""
    n = obs.shape[0]
    ac.planes = form != "f32"
    ac.planes_two_launch = form == "two"
    out = [torch.full((n, 2), float("nan"), device=DEV), torch.full((n, 2), float("nan"), device=DEV),
           torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)]
    ac.act(obs, *out, seed, step, env_offset=off, deterministic=deterministic, planes_fresh=planes_fresh)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


class Worst:
    def __init__(self, what):
        self.what, self.ratio, self.checks = what, {}, {}

    def add(self, key, got, want, m, tau, count=None):
        w, nv = P.check(got, want, m, tau)
        self.ratio[key] = max(self.ratio.get(key, 0.0), w)
        if count is not None:
            self.checks[key] = self.checks.get(key, 0) + count
        assert nv == 0, (self.what, key, w, nv)

    def report(self):
        print(f"{self.what}: worst " + ", ".join(f"{k} {v:.3g}" for k, v in self.ratio.items()) +
              ("" if not self.checks else " | checks " + ", ".join(f"{k} {v}" for k, v in self.checks.items())))


def _check_step(w, res, x, nets, activation, form, D, n, fam=None, names=None, off=OFF, std=STD):
    a, mu, logp, val = res
    t = P.taus(form, D, n)
    split = form != "f32"
    n_imp = int((fam == names.index("impulse")).sum()) if fam is not None else 0
    for name, got in (("actor", mu), ("critic", val[:, None])):
        ref = P.forward64(nets[name], x, activation, t, split=split)
        w.add(name, got, ref["y"], ref["m_y"], t["out"], count=n_imp * got.shape[1])
        if split:
            ex = P.forward64(nets[name], x, activation, {"z1": t["z1_exact"], "z2": t["z2_exact"]})
            w.add(name + " exact", got, ex["y"], ex["m_y"], t["out_exact"])
    d = P.draw64(np.arange(n) + off, STEP, SEED)
    s = np.asarray(std, dtype=np.float64)
    w.add("draw", a.double() - mu.double(), torch.from_numpy(s[None] * np.stack([d["z0"], d["z1"]], 1)),
          torch.from_numpy(P.draw_allowance(d, std, a.numpy())), 1.0)
    lp, allow = P.logp64(a.numpy(), mu.numpy(), s)
    w.add("logp", logp, torch.from_numpy(lp), torch.from_numpy(allow), 1.0)


def _case(D, n, activation, kind, seed):
    nets = P.make_nets(D, kind, seed=seed)
    kr = P.kink_rows(nets, D, P.taus("f32", D, n)["z1"], seed=seed)
    if kind == "default":
        nets = P.steer_b2(nets, kr, activation)
    x, fam, names = P.batch(D, n, seed=seed, extra=kr)
    return nets, x, fam, names


# ---- the f32 kernel, every (KS, RT) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "trained"])
@pytest.mark.parametrize("D,n", P.F32_CASES)
def test_f32_kernel_against_float64(D, n, kind):
    for activation in ("elu", "relu"):
        nets, x, fam, names = _case(D, n, activation, kind, seed=D + n)
        ac = _ac(nets, D, activation)
        res = _run(ac, x.to(DEV), "f32")
        w = Worst(f"{P.form_name('f32', D, n)} D={D} n={n} {activation} {kind}")
        _check_step(w, res, x, nets, activation, "f32", D, n, fam, names)
        w.report()


# ---- the bf16 forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "trained"])
@pytest.mark.parametrize("D", P.BF16_DS)
def test_bf16_forms_against_the_split_model_and_float64(D, kind):
    for form, ns in (("one", P.BF16_NS), ("two", P.BF16_NS[1:2])):
        for n in ns:
            activation = P.activation_of(D, n)
            nets, x, fam, names = _case(D, n, activation, kind, seed=D + n)
            res = _run(_ac(nets, D, activation), x.to(DEV), form)
            w = Worst(f"{P.form_name(form, D, n)} D={D} n={n} {activation} {kind}")
            _check_step(w, res, x, nets, activation, form, D, n, fam, names)
            w.report()


@pytest.mark.parametrize("D,n", P.WHOLE_CASES)
def test_form2_values_against_the_split_model_and_float64(D, n):
    for activation in ("elu", "relu"):
        nets, x, fam, names = _case(D, n, activation, "default", seed=D)
        ac = _ac(nets, D, activation)
        out = torch.full((n,), float("nan"), device=DEV)
        ac.values_batched(x.to(DEV), out, chunk=2048)
        torch.cuda.synchronize()
        t = P.taus("whole", D, n)
        w = Worst(f"form 2 D={D} n={n} {activation}")
        ref = P.forward64(nets["critic"], x, activation, t, split=True)
        w.add("critic", out.cpu()[:, None], ref["y"], ref["m_y"], t["out"], count=int((fam == names.index("impulse")).sum()))
        ex = P.forward64(nets["critic"], x, activation, {"z1": t["z1_exact"], "z2": t["z2_exact"]})
        w.add("critic exact", out.cpu()[:, None], ex["y"], ex["m_y"], t["out_exact"])
        w.report()


# ---- probe tails: layer 1 on its own -------------------------------------------------------------------------------------------
PROBE_CASES = [("f32", 14, 400), ("f32", 256, 1000), ("f32", 689, 4096), ("f32", 3208, 4097), ("f32", 4808, 5200)] + \
              [(form, D, max(D + 400, 1521)) for D in P.BF16_DS for form in ("one", "two")]


@pytest.mark.parametrize("form,D,n", PROBE_CASES)
def test_probe_tails_hold_every_layer1_unit_to_the_layer1_tau(form, D, n):
    activation = P.activation_of(D, n)
    nets, x, fam, names = _case(D, n, activation, "default", seed=D + 7)
    t = P.taus(form, D, n)
    tau = t["z1"] + 6 * P.U                         # + the two activations on the way out
    allunits = P.probe_tails(nets, [0, 1, 2])
    refs = {}
    for name in ("actor", "critic"):
        eye = dict(allunits[name], w3=torch.eye(64), b3=torch.zeros(64))
        refs[name] = P.forward64(eye, x, activation, t, split=form != "f32")
    ac = _ac(allunits, D, activation)
    obs = x.to(DEV)
    w = Worst(f"probe {P.form_name(form, D, n)} D={D} n={n} {activation}")
    n_imp = int((fam == names.index("impulse")).sum())
    for j in range(64):
        units = [j, (j + 32) % 64, j]
        _load(ac, P.probe_tails(nets, units))
        _, mu, _, val = _run(ac, obs, form, planes_fresh=j > 0)
        ra, rc = refs["actor"], refs["critic"]
        w.add("actor z1", mu, ra["y"][:, units[:2]], ra["m_y"][:, units[:2]], tau, count=2 * n_imp)
        w.add("critic z1", val[:, None], rc["y"][:, units[2:]], rc["m_y"][:, units[2:]], tau, count=n_imp)
    w.report()


# ---- strided rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,D,n", [("f32", 689, 1000), ("f32", 14, 4097), ("one", 689, 3057), ("one", 3208, 1521),
                                      ("two", 65, 1000), ("two", 3208, 1000)])
def test_every_form_on_column_slices(form, D, n):
    """observations that are columns 3 .. 3 + D of a [n, D + 7] matrix: rows 4-byte aligned only"""
    activation = P.activation_of(D, n)
    nets, x, fam, names = _case(D, n, activation, "trained", seed=D + 3)
    wide = torch.randn(n, D + 7)
    wide[:, 3:3 + D] = x
    obs = wide.to(DEV)[:, 3:3 + D]
    assert obs.stride(0) == D + 7
    res = _run(_ac(nets, D, activation), obs, form)
    w = Worst(f"strided {P.form_name(form, D, n)} D={D} n={n}")
    _check_step(w, res, x, nets, activation, form, D, n, fam, names)
    w.report()


def test_form2_on_column_slices():
    import wheeledlab_amd._abi as A
    D, n = 689, 1000
    nets, x, _, _ = _case(D, n, "elu", "default", seed=5)
    ac = _ac(nets, D, "elu")
    wide = torch.randn(n, D + 7)
    wide[:, 3:3 + D] = x
    obs = wide.to(DEV)[:, 3:3 + D]
    dp = (D + 63) // 64 * 64
    w_hi, w_lo = (torch.zeros(128, dp, dtype=torch.int16, device=DEV) for _ in range(2))
    part = torch.zeros(n, 128, device=DEV)
    sc = A.WlActScratch(w_hi.data_ptr(), w_lo.data_ptr(), part.data_ptr(), dp, 1, n, 2)
    a, c = ac.actor.struct(), ac.critic.struct()
    out = torch.full((n,), float("nan"), device=DEV)
    lib = A.load()
    A.check(lib.wl_actor_critic_planes(C.byref(a), C.byref(c), C.byref(sc), None), "planes")
    A.check(lib.wl_actor_critic_act_planes(C.byref(a), C.byref(c), ac.std.data_ptr(), n, obs.data_ptr(), obs.stride(0), None, None,
                                           None, out.data_ptr(), 0, 0, 0, 0, 2, C.byref(sc), None), "act_planes")
    torch.cuda.synchronize()
    t = P.taus("whole", D, n)
    ref = P.forward64(nets["critic"], x, "elu", t, split=True)
    w = Worst("strided form 2 D=689")
    w.add("critic", out.cpu()[:, None], ref["y"], ref["m_y"], t["out"])
    w.report()


# ---- the draw at its edges, the log-prob, deterministic ------------------------------------------------------------------------
@pytest.mark.parametrize("form,D", [("f32", 14), ("f32", 689), ("one", 689), ("one", 3208), ("two", 689)])
def test_draw_and_log_prob_at_the_keys_edges(form, D):
    """each committed key lands on row 16 + 5 of a 64-row launch (second tile); std in {(0.7, 1.3), (1, 1), (1e-3, 50)}"""
    activation = "elu"
    nets = P.make_nets(D, "default", seed=1)
    x = torch.randn(64, D)
    w = Worst(f"draw {form} D={D}")
    for std in ((0.7, 1.3), (1.0, 1.0), (1e-3, 50.0)):
        ac = _ac(nets, D, activation, std)
        s32 = ac.std.cpu().double().numpy()
        for key, env in P.DRAW_KEYS.items():
            off = env - 21
            a, mu, logp, _ = _run(ac, x.to(DEV), form, seed=P.DRAW_SEED, step=P.DRAW_STEP, off=off)
            d = P.draw64(np.arange(64) + off, P.DRAW_STEP, P.DRAW_SEED)
            want = s32[None] * np.stack([d["z0"], d["z1"]], 1)
            w.add("draw", a.double() - mu.double(), torch.from_numpy(want),
                  torch.from_numpy(P.draw_allowance(d, s32, a.numpy())), 1.0, count=1)
            got_key = (a.double() - mu.double())[21].numpy()
            assert np.all(np.abs(got_key - want[21]) <= P.draw_allowance(d, s32, a.numpy())[21]), (key, std, got_key, want[21])
            lp, allow = P.logp64(a.numpy(), mu.numpy(), s32)
            w.add("logp", logp, torch.from_numpy(lp), torch.from_numpy(allow), 1.0)
    w.report()


@pytest.mark.parametrize("form,D,n", [("f32", 689, 4096), ("f32", 14, 17), ("one", 689, 3057), ("one", 3208, 1521), ("two", 3208, 1000),
                                      ("two", 64, 100)])
def test_deterministic_step_gives_a_equal_to_mu_in_every_form(form, D, n):
    nets, x, _, _ = _case(D, n, "relu", "default", seed=D)
    a, mu, _, _ = _run(_ac(nets, D, "relu"), x.to(DEV), form, deterministic=True)
    assert torch.equal(a, mu)
    assert not torch.isnan(mu).any()


# ---- nets independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(689, 4096), (689, 20000), (256, 4096), (14, 20000)])
def test_single_net_launches_equal_the_joint_launch(D, n):
    """nets = 1 / nets = 2 run RT from one net's tile count, the joint launch from both: the feature split (KS) and hence
    every bit must not change (at these sizes the single-net RT differs from the joint one)"""
    assert P.f32_form(D, n, nets=1)[1] != P.f32_form(D, n, nets=3)[1]
    nets, x, _, _ = _case(D, n, "elu", "default", seed=D + n)
    ac = _ac(nets, D, "elu")
    obs = x.to(DEV)
    ac.planes = False
    full = [torch.zeros(n, 2, device=DEV), torch.zeros(n, 2, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    ac.act(obs, *full, 5, 77, env_offset=4096)
    half = [torch.zeros_like(t) for t in full]
    ac.act(obs, *half[:3], None, 5, 77, env_offset=4096, nets=1)
    ac.act(obs, None, None, None, half[3], 5, 77, env_offset=4096, nets=2)
    torch.cuda.synchronize()
    for f, h in zip(full, half):
        assert torch.equal(f, h)


# ---- the other kernels that evaluate the policy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,out_dim", P.MLP_CASES)
def test_mlp_forward_against_float64(in_dim, out_dim):
    from wheeledlab_amd.policy import Mlp
    w = Worst(f"wl_mlp_forward {in_dim} -> {out_dim}")
    for activation in ("elu", "relu"):
        m = Mlp(in_dim, out_dim, activation, device=DEV, generator=torch.Generator().manual_seed(in_dim * 8 + out_dim))
        net = P.mlp64(m)
        pool = P.row_pool(in_dim, seed=in_dim)
        x = torch.cat([pool[k] for k in pool] + [torch.randn(1000, in_dim)])
        t = P.taus("mlp", in_dim)
        y = m(x.to(DEV)).cpu()
        ref = P.forward64({k: v.float() for k, v in net.items()}, x, activation, t)
        w.add(activation, y, ref["y"], ref["m_y"], t["out"], count=in_dim)
        # probe tails: each unit of layer 1 on its own
        m.w2.copy_(torch.eye(64))
        m.b2.zero_()
        m.b3.zero_()
        eye = dict({k: v.float() for k, v in net.items()}, w2=torch.eye(64), b2=torch.zeros(64), w3=torch.eye(64), b3=torch.zeros(64))
        ref = P.forward64(eye, x, activation, t)
        for u0 in range(0, 64, out_dim):
            units = [(u0 + i) % 64 for i in range(out_dim)]
            m.w3.zero_()
            m.w3[torch.arange(out_dim), torch.tensor(units)] = 1.0
            y = m(x.to(DEV)).cpu()
            w.add(activation + " probe", y, ref["y"][:, units], ref["m_y"][:, units], t["z1"] + 6 * P.U, count=out_dim * in_dim)
    w.report()


def test_drift_rollout_first_step_against_float64():
    from wheeledlab_amd.core import DriftBatch
    from wheeledlab_amd.policy import ActorCritic, RolloutStorage
    n = 1000
    env = DriftBatch(n, device=DEV, seed=9)
    env.reset()
    env.observe()
    ac = ActorCritic(device=DEV, seed=2)
    ac.std.copy_(torch.tensor(STD))
    st = RolloutStorage(1, n, device=DEV)
    step0 = env.step_count
    env.rollout_policy(ac, st, evaluate_critic=False)
    torch.cuda.synchronize()
    x = st.observations[0].cpu()
    t = P.taus("mlp", 14)
    nets = {"actor": P.mlp64(ac.actor)}
    ref = P.forward64({k: v.float() for k, v in nets["actor"].items()}, x, "elu", t)
    w = Worst("wl_drift_rollout_policy step 0")
    mu, a = st.mu[0].cpu(), st.actions[0].cpu()
    w.add("actor", mu, ref["y"], ref["m_y"], t["out"])
    d = P.draw64(np.arange(n) + env.env_offset, step0, env.seed)
    s = np.asarray(STD, dtype=np.float64)
    w.add("draw", a.double() - mu.double(), torch.from_numpy(s[None] * np.stack([d["z0"], d["z1"]], 1)),
          torch.from_numpy(P.draw_allowance(d, STD, a.numpy())), 1.0)
    lp, allow = P.logp64(a.numpy(), mu.numpy(), s)
    w.add("logp", st.actions_log_prob[0].cpu(), torch.from_numpy(lp), torch.from_numpy(allow), 1.0)
    w.report()


@pytest.mark.parametrize("n", [4096, 1000])
def test_elev_collector_step_against_float64(n):
    """one-step wl_elev_collect_rollout on designed observation rows: mu against float64, real tails and probe tails"""
    from wheeledlab_amd.core import ElevBatch
    from wheeledlab_amd.policy import ActorCritic, RolloutStorage
    D = 689
    env = ElevBatch(n, device=DEV, seed=4)
    env.reset()
    ac = ActorCritic(D, 2, "elu", device=DEV, seed=3)
    nets, x, fam, names = _case(D, n, "elu", "default", seed=n)
    _load(ac, nets)
    t = P.taus("elev", D)
    w = Worst(f"wl_elev_collect_rollout n={n}")
    eye = dict(P.probe_tails(nets, [0, 1, 2])["actor"], w3=torch.eye(64), b3=torch.zeros(64))
    ref_probe = P.forward64(eye, x, "elu", t)
    ref = P.forward64(nets["actor"], x, "elu", t)
    for j in range(-1, 32):
        if j >= 0:
            _load(ac, P.probe_tails(nets, [2 * j, 2 * j + 1, 0]))
        st = RolloutStorage(1, n, D, 2, DEV)
        st.observations[0].copy_(x.to(DEV))
        env.collect_rollout(ac, st, start=0, count=1, deterministic=True)
        torch.cuda.synchronize()
        mu = st.mu[0].cpu()
        assert torch.equal(mu, st.actions[0].cpu())
        if j < 0:
            w.add("actor", mu, ref["y"], ref["m_y"], t["out"])
        else:
            u = [2 * j, 2 * j + 1]
            w.add("actor z1 probe", mu, ref_probe["y"][:, u], ref_probe["m_y"][:, u], t["z1"] + 6 * P.U,
                  count=2 * int((fam == names.index("impulse")).sum()))
    w.report()

"""The float64 policy-step reference (tests/policy_reference.py) on the CPU: its bound holds for correct fp32 arithmetic in
several summation orders (the kernels' own included), it rejects modelled defects of the kinds a kernel could have, and
the GPU cases of tests/test_gpu_policy_reference.py reach every kernel instantiation the launchers can pick."""
import numpy as np
import pytest
import torch

import policy_reference as P

DS = [14, 64, 65, 689, 1024, 3208, 4808]


# ---- fp32 evaluations --------------------------------------------------------------------------------------------------------
def _act32(z, activation):
    """fp32 activations; ELU as exp(x) - 1 in fp32 (the negative control: no expm1, the kernels' own form, must pass)"""
    if activation == "relu":
        return torch.clamp(z, min=0.0)
    return torch.where(z > 0, z, torch.exp(torch.clamp(z, max=0.0)) - 1.0)     # exp(x) - 1 in fp32


def _tail32(net, z1, activation):
    h = _act32(z1, activation)
    h = _act32(h @ net["w2"].t() + net["b2"], activation)
    return h @ net["w3"].t() + net["b3"]


def _tree(p):
    """pairwise fp32 sum over the last axis"""
    while p.shape[-1] > 1:
        if p.shape[-1] & 1:
            p = torch.cat([p, torch.zeros_like(p[..., :1])], -1)
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def layer1_32(net, x, order, D, n):
    """z1 [rows, 64] in fp32 in one summation order"""
    w, b = net["w1"], net["b1"]
    if order == "numpy":
        return torch.from_numpy(x.numpy() @ w.numpy().T + b.numpy())
    if order == "reversed":
        acc = b.expand(x.shape[0], 64).clone()
        for f in reversed(range(D)):
            acc = acc + x[:, f:f + 1] * w[:, f]
        return acc
    if order == "pairwise":
        return _tree(x[:, None, :] * w[None]) + b
    if order == "kernel":   # the f32 kernel: shares of 16-wide chunks, 4 k-steps of 4-term trees each, the fold
        ks, _ = P.f32_form(D, n)
        n_full = D >> 4
        per = -(-n_full // ks)
        pad = n_full * 16 + 16 - D if D & 15 else 0
        xp, wp = torch.nn.functional.pad(x, (0, pad)), torch.nn.functional.pad(w, (0, pad))
        parts = []
        for k in range(ks):
            acc = b.expand(x.shape[0], 64).clone() if k == 0 else torch.zeros(x.shape[0], 64)
            c0 = min(k * per, n_full)
            chunks = list(range(c0, min(c0 + per, n_full))) + ([n_full] if k == ks - 1 and D & 15 else [])
            for c in chunks:
                for s in range(4):
                    f = [16 * c + 4 * g + s for g in range(4)]
                    acc = _tree(xp[:, None, f] * wp[None, :, f]) + acc
            parts.append(acc)
        h = parts[0]
        for p in parts[1:]:
            h = h + p
        return h
    raise ValueError(order)


def layer1_split32(net, x, D, n):
    """the bf16 one-launch form: x, w1 split into planes, 3 exact products per feature summed as 32-term trees per k-step
    (the MFMA order al.bh, ah.bl, ah.bh) in KS shares, then the fold"""
    dp = -(-D // 64) * 64
    hx, lx = (t.float() for t in P.split_bf16(x))
    hw, lw = (t.float() for t in P.split_bf16(net["w1"]))
    ks, _ = P.bf16_form(D, n)
    steps = dp // 32
    per = -(-steps // ks)
    parts = []
    for k in range(ks):
        acc = net["b1"].expand(x.shape[0], 64).clone() if k == 0 else torch.zeros(x.shape[0], 64)
        for s in range(min(k * per, steps), min(k * per + per, steps)):
            f0 = min(64 * (s >> 1), D - 64) + 32 * (s & 1)
            f = torch.arange(f0, f0 + 32)
            keep = (f >= 64 * (dp // 64 - 1)) | (s >> 1 < dp // 64 - 1) | (D == dp)   # the overlapped chunk's zeros
            for a, bb in ((lw, hx), (hw, lx), (hw, hx)):
                prod = bb[:, None, f] * (a[:, f] * keep)[None]
                acc = _tree(prod) + acc
        parts.append(acc)
    h = parts[0]
    for p in parts[1:]:
        h = h + p
    return h


def _case(D, activation, kind="default"):
    """nets and the row families (impulse rows thinned to ~48, kink rows for this width's f32 form), b2 steered to the
    second layer's kink for the default nets"""
    nets = P.make_nets(D, kind, seed=D)
    pool = P.row_pool(D, seed=D)
    x = torch.cat([pool[k] for k in pool if k != "impulse"] + [pool["impulse"][torch.arange(0, D, max(1, D // 48))]])
    kr = P.kink_rows(nets, D, P.taus("f32", D, x.shape[0] + 128)["z1"], seed=D)
    x = torch.cat([x, kr])
    if kind == "default":
        nets = P.steer_b2(nets, kr, activation)
    return nets, x


@pytest.mark.parametrize("kind", ["default", "trained"])
@pytest.mark.parametrize("activation", ["elu", "relu"])
@pytest.mark.parametrize("D", DS)
def test_bound_holds_for_correct_fp32_arithmetic(D, activation, kind):
    nets, x = _case(D, activation, kind)
    n = x.shape[0]
    worst = {}
    for name in ("actor", "critic"):
        net = nets[name]
        t = P.taus("f32", D, n)
        ref = P.forward64(net, x, activation, t)
        for order in ("numpy", "reversed", "pairwise", "kernel"):
            z1 = layer1_32(net, x, order, D, n)
            for key, g, want, m, tau in (("z1", z1, ref["z1"], ref["m_z1"], t["z1"]),
                                         ("out", _tail32(net, z1, activation), ref["y"], ref["m_y"], t["out"])):
                w, nv = P.check(g, want, m, tau)
                assert nv == 0, (name, order, key, w)
                worst[order] = max(worst.get(order, 0.0), w)
        if D >= 64:   # the bf16 one-launch arithmetic against the split model and against exact float64
            t = P.taus("one", D, n)
            ref_s = P.forward64(net, x, activation, t, split=True)
            ref_x = P.forward64(net, x, activation, {"z1": t["z1_exact"], "z2": t["z2_exact"]})
            z1 = layer1_split32(net, x, D, n)
            y = _tail32(net, z1, activation)
            for key, g, want, m, tau in (("split z1", z1, ref_s["z1"], ref_s["m_z1"], t["z1"]),
                                         ("split out", y, ref_s["y"], ref_s["m_y"], t["out"]),
                                         ("exact z1", z1, ref_x["z1"], ref_x["m_z1"], t["z1_exact"]),
                                         ("exact out", y, ref_x["y"], ref_x["m_y"], t["out_exact"])):
                w, nv = P.check(g, want, m, tau)
                assert nv == 0, (name, key, w)
                worst[key] = max(worst.get(key, 0.0), w)
    print(f"D={D} {activation} {kind}: worst ratio " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) < 1


def test_split_model_equals_a_direct_computation():
    """the 3D-wide contraction of split_operands is sum_f hx hw + lx hw + hx lw, computed here feature by feature"""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(5, 65, generator=g) * 3).float()
    w = torch.randn(64, 65, generator=g).float()
    x3, w3 = P.split_operands(x, w)
    got = x3 @ w3.t()
    want = torch.zeros(5, 64, dtype=torch.float64)
    for f in range(65):
        hx = x[:, f].to(torch.bfloat16).double()
        lx = (x[:, f] - x[:, f].to(torch.bfloat16).float()).to(torch.bfloat16).double()
        hw = w[:, f].to(torch.bfloat16).double()
        lw = (w[:, f] - w[:, f].to(torch.bfloat16).float()).to(torch.bfloat16).double()
        want += hx[:, None] * hw[None] + lx[:, None] * hw[None] + hx[:, None] * lw[None]
    assert torch.allclose(got, want, rtol=1e-15, atol=0)
    # hi + lo carries 16 significant bits: |x - hi - lo| <= 2^-17 |x|
    hx, lx = P.split_bf16(x)
    assert bool(((x.double() - hx - lx).abs() <= 2.0 ** -17 * x.double().abs()).all())
    # the impulse value's lo plane is almost half a bf16 ulp
    h, l = P.split_bf16(torch.tensor([P.IMPULSE_MANTISSA]))
    assert float(h) == 1.0 and float(l) == 2.0 ** -8


# ---- modelled defects ----------------------------------------------------------------------------------------------------------
def _rejects(D, activation, defect, split=False, probe=False):
    """worst ratio and violations of a defective evaluation (the float64 forward of a modified input / net) against the
    reference, at the f32 kernel's tau (split: the one-launch bf16 form's, against the split model)"""
    nets = P.make_nets(D, "default", seed=D)
    pool = P.row_pool(D, seed=D)
    x = torch.cat([pool["impulse"], pool["sparse"], pool["randn"]])
    form = "one" if split else "f32"
    t = P.taus(form, D, x.shape[0])
    worst, nv = 0.0, 0
    for name in ("actor", "critic"):
        net = nets[name]
        ref = P.forward64(net, x, activation, t, split=split)
        if split:
            x3, w3 = P.split_operands(x, net["w1"])
            x3, w3 = defect(x3.clone(), w3.clone())
            bad = P.R.forward(dict(P.mlp64(net), w1=w3), x3, activation)["y"]
        else:
            xb, nb = defect(x.clone(), {k: v.clone() for k, v in net.items()})
            bad = P.forward64(nb, xb, activation, t)["y"]
        w, v = P.check(bad, ref["y"], ref["m_y"], t["out"])
        worst, nv = max(worst, w), nv + v
    return worst, nv


def _drop(f):
    def d(x, n):
        x[:, f] = 0.0
        return x, n
    return d


@pytest.mark.parametrize("activation", ["elu", "relu"])
def test_the_checker_rejects_modelled_defects(activation):
    cases = []
    for D in (14, 689, 3208, 4808):
        ks, _ = P.f32_form(D, D + 128)
        per = -(-(D >> 4) // ks)
        cases.append((f"D={D}: feature D-1 dropped", D, _drop(D - 1), False))
        if ks > 1:
            cases.append((f"D={D}: first feature of share 2 dropped", D, _drop(16 * per), False))
    cases.append(("D=689: 16-wide tail chunk dropped", 689, _drop(slice(16 * (689 >> 4), 689)), False))

    def twice(D):
        def d(x3, w3):
            last = (-(-D // 64) - 1) * 64
            for k in range(3):
                w3[:, k * D + D - 64:k * D + last] *= 2.0     # the overlapped chunk's shared features counted again
            return x3, w3
        return d
    for D in (65, 689):
        cases.append((f"D={D}: overlapped chunk counted twice", D, twice(D), True))
    for D in (689, 3208):
        def no_lx(x3, w3, D=D):
            x3[:, D:2 * D] = 0.0
            return x3, w3

        def no_lw(x3, w3, D=D):
            w3[:, 2 * D:] = 0.0
            return x3, w3
        cases += [(f"D={D}: lo plane of x dropped", D, no_lx, True), (f"D={D}: lo plane of w1 dropped", D, no_lw, True)]

    def bias_twice(x, n):
        n["b1"] = n["b1"] * 2.0
        return x, n
    cases.append(("D=689: bias seeded by two shares", 689, bias_twice, False))
    for what, D, defect, split in cases:
        worst, nv = _rejects(D, activation, defect, split)
        print(f"{what}: worst ratio {worst:.3g}, {nv} violations")
        assert nv > 0, what


def test_the_checker_rejects_draw_and_log_prob_defects():
    n, off = 4096, 8192
    d = P.draw64(np.arange(n) + off, 99, 42)
    std = np.array([0.7, 1.3], dtype=np.float32)
    mu = np.random.default_rng(0).standard_normal((n, 2)).astype(np.float32)
    z = np.stack([d["z0"], d["z1"]], 1).astype(np.float32)
    good = (mu + std[None] * z).astype(np.float32)

    def draw_check(a):
        return P.check(a.astype(np.float64) - mu, std[None] * np.stack([d["z0"], d["z1"]], 1), P.draw_allowance(d, std, a), 1.0)
    w, nv = draw_check(good)
    print(f"correct draw: worst ratio {w:.3g}")
    assert nv == 0
    d_bad = P.draw64(np.arange(n), 99, 42)                         # keyed without env_offset
    assert draw_check((mu + std[None] * np.stack([d_bad["z0"], d_bad["z1"]], 1)).astype(np.float32))[1] > 0
    assert draw_check((mu + std[::-1][None] * z).astype(np.float32))[1] > 0          # std0 / std1 swapped
    lp, allow = P.logp64(good, mu, std)
    lp32 = (-0.5 * (z.astype(np.float32) ** 2).sum(1) - np.log(std).sum() - np.float32(P.LOG_2PI)).astype(np.float32)
    assert P.check(lp32, lp, allow, 1.0)[1] == 0
    assert P.check(lp32 + np.log(std[1]), lp, allow, 1.0)[1] > 0                      # one log sigma missing


def test_draw_keys_reach_their_edges():
    """the committed env ids still give the uniforms they were chosen for (oracle/philox.py is bit exact on the device)"""
    K = P.DRAW_KEYS
    d = P.draw64(np.array(list(K.values())), P.DRAW_STEP, P.DRAW_SEED)
    u0, u1 = dict(zip(K, d["u0"])), dict(zip(K, d["u1"]))
    assert u0["u0=0"] == 0.0 and 1.0 - u0["u0 max"] <= 2.0 ** -19
    assert min(u1["u1~0"], 1 - u1["u1~0"]) < 2.0 ** -21
    for k, t in (("u1~1/4", 0.25), ("u1~1/2", 0.5), ("u1~3/4", 0.75)):
        assert abs(u1[k] - t) < 2.0 ** -21, k


# ---- form coverage ------------------------------------------------------------------------------------------------------------
def test_gpu_cases_reach_every_instantiation():
    f32 = {(ks, rt, a) for D, n in P.F32_CASES for ks, rt in [P.f32_form(D, n)] for a in ("elu", "relu")}
    want_f32 = {(ks, rt, a) for ks in (1, 2, 4) for rt in (1, 2, 4) for a in ("elu", "relu")} - {(4, 4, "elu"), (4, 4, "relu")}
    one = {P.bf16_form(D, n) for D in P.BF16_DS for n in P.BF16_NS}
    two = {P.splits(D) for D in P.BF16_DS}
    print("f32 (KS, RT):", sorted({(k, r) for k, r, _ in f32}), "| bf16 one launch:", sorted(one), "| splits:", sorted(two))
    assert f32 == want_f32
    assert one == {(8, 1), (8, 2), (4, 1), (4, 2), (4, 4)}
    assert {1, 2, 8, 26} <= two
    assert P.WHOLE_CASES
    # (4, 4) is out of the f32 launcher's reach: RT = 4 needs >= 1024 tiles, hence >= 256 joint row blocks, and KS = 4 fewer than 256
    for n in range(16 * 1024, 16 * 1024 * 8, 4099):
        assert P.f32_form(4808, n) != (4, 4)

"""The PPO learners (csrc/wl_ppo.hip, csrc/wl_ppo_wide.hip and the apply stage they share) against the float64 step of
tests/ppo_reference.py, at the minibatch sizes training runs and at the branches' edges.

Gradient rows.  Every element of the row (parameter gradients, the value-loss / surrogate / KL sums) and the squared norm
are held to  |g - g64| <= tau * m(g) + floor,  m = the reference's magnitude pass (first-order: the backward with every
operand replaced by its absolute value), floor = 1e-30 (flushed subnormals).  tau = n 2^-24 + s 2^-16, n = the depth of
the summation tree on the longest path from an input to the element (roundings along it), s = the split-bf16 product
stages on it (each < 2^-16 relative: two plane roundings of 2^-18 and the dropped lo.lo term; the staging test of
test_gpu_ppo_wide.py asserts 2^-16 per operand).  An MFMA adds a K-term tree to its accumulator: a path through it passes
the product (f32 operands; bf16 products are exact), ceil(log2 K) levels and the accumulator add, and every further
instruction on the same accumulator adds one.  Drift kernel (ppo_grad_kernel + ppo_reduce_kernel), per sample:
    layer 1, 4 x 16x16x4 f32: 4 + 3 = 7 | ELU (scale, exp2, - 1): 3 | layer 2, 6 bf16 MFMAs of K 32: 6 + 5 = 11 (stage 1) |
    ELU: 3 | output layer, 8 f32 MFMAs + the bias MFMA + the two accumulators' add: 13 | z = (a - y) / sigma 2, logp 4,
    ratio 3, dl/dlogp 2, delta3 2: 13 | W3^T delta3: 4 | * act'(h2): 1 | W2^T delta2: 11 (stage 2) | * act'(h1): 1
                                                                                                   = 70 at delta1, s = 2
then the weight-gradient MFMAs over the samples: 4 per 16-sample tile on one accumulator, T tiles per wavefront (4 + 4 T
- 1 after the first product), the 16 lanes' and the 4 wavefronts' sums of a block (4 + 4), the reduction's four
interleaved chains of ceil(blocks / 16) rows and its two pairwise levels (+ 4):  n = 70 + 4 T + 3 + 8 + ceil(blocks / 16) + 4.
Wide (wl_ppo_wide.hip): layer 1 is the contraction kernel's 6 bf16 MFMAs per 64-wide K chunk, dp / 64 chunks, + the bias:
6 dp / 64 + 6 (stage 1), so delta1 sits at 6 dp / 64 + 66 with s = 3; the tail's sums are the drift kernel's; dW1 = X^T
delta1 is a fourth stage, 6 MFMAs per chunk of 64 samples over the chunks of one split (6 cps + 5) and the four chains of
the split reduction (ceil(splits / 4) + 2).  One tau per case: the largest.  Branch decisions get the depth of their own
forward path (z1, z2, the loss terms).

Samples within tau * m of a branch (ratio vs 1 +- clip where adv != 0, |v - v_old| vs clip, l1 vs l2 outside the clip
range, ReLU pre-activations vs 0) are moved ahead of the tested minibatch in the permutation (the last minibatch of an
update with four), counted, and must be < 1 % of the rows.  The branch-dense batches put most samples just outside those
bands, on both sides of each branch.

Apply stage: wl_ppo_apply / wl_ppo_wide_apply on hand-set rows: the learning-rate decision and the new lr equal the fp32
evaluation of the rule bit for bit; parameters equal float64 Adam to an ulp of the parameter + 16 u of the update's
magnitude (+ the cancellation in the fp32 bias corrections 1 - beta^t after step 1).  GAE and the rollout bookkeeping against float64 at training sizes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-30
CLIP = 0.2


def _ceil(a, b):
    return -(-a // b)


def tau_drift(mb):
    tiles = _ceil(mb, 16)
    blocks = min(256, _ceil(tiles, 4))
    T = _ceil(tiles, 4 * blocks)
    n = 70 + 4 * T + 3 + 8 + _ceil(blocks, 16) + 4
    return n * R.U + 2 * R.BF16_STAGE, dict(T=T, blocks=blocks, n=n)


def tau_wide(D, mb, splits):
    dp = _ceil(D, 64) * 64
    _, d = tau_drift(mb)
    l1 = 6 * dp // 64 + 6
    chunks = mb // 64
    cps = _ceil(chunks, splits)
    used = _ceil(chunks, cps)
    n_tail = d["n"] - 7 + l1
    n_dw1 = l1 + 60 + 6 * cps + 5 + _ceil(used, 4) + 2
    n = max(n_tail, n_dw1)
    return n * R.U + 4 * R.BF16_STAGE, dict(d, n=n, dp=dp, cps=cps, splits=used)


def tau_branch(D):
    """bands of the branch decisions: the forward path's depth up to each -- z1, z2 (+ 3 + 11 and a split stage), the loss
    terms (+ 3 + 13 + 13) -- with the split stages on it"""
    l1, s1 = (7, 0) if D == 14 else (6 * (_ceil(D, 64) * 64) // 64 + 6, 1)
    return dict(z1=l1 * R.U + s1 * R.BF16_STAGE, z2=(l1 + 14) * R.U + (s1 + 1) * R.BF16_STAGE,
                loss=(l1 + 43) * R.U + (s1 + 1) * R.BF16_STAGE)


def _nets(D, activation, seed):
    from wheeledlab_amd.rl.ppo import ActorCritic
    torch.manual_seed(seed)
    ac = ActorCritic(D, D, 2, activation=activation).to(DEV)      # torch's default initialisation, as training starts
    with torch.no_grad():
        ac.std.copy_(torch.tensor([0.8, 1.1]))
        if activation == "relu":
            # layer-2 biases of +-1.5: a pre-activation within its fp32 band of 0 becomes a 3-sigma event, so that the random
            # rows excuse < 1 %; the branch-dense batches put pre-activations at the kink on purpose
            for net in (ac.actor, ac.critic):
                net[2].bias.copy_(1.5 * torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0))
    return ac


def _batch(ac, rows, D, activation, seed):
    """fp32 rollout-like rows: actions drawn around the float64 policy mean, old log-probs / values / means off the
    current ones"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    obs = r(rows, D)
    if D > 14:
        obs[:, : D // 2] *= 0.05          # mixed magnitudes, like body rates next to a height map
    P = R.nets64(ac)
    with torch.no_grad():
        fa = R.forward(P["actor"], obs.double(), activation)
        fc = R.forward(P["critic"], obs.double(), activation)
    mu = fa["y"].float()
    actions = mu + ac.std.detach() * r(rows, 2)
    z = (actions.double() - fa["y"]) / P["std"]
    logp = (-0.5 * z * z - torch.log(P["std"]) - 0.5 * R.LOG_2PI).sum(1).float()
    # ratios and |v - v_old| well inside the clip range (3 in 4 samples) or well outside it: random data rarely sit in a
    # branch's fp32 band (the branch-dense test puts them there on purpose)
    far = lambda n: torch.where(torch.rand(n, device=DEV, generator=g) < 0.75, 0.005 * r(n),
                                torch.sign(r(n)) * (1.2 + 0.1 * r(n)))
    flat = dict(obs=obs, actions=actions.contiguous(), mu=(mu + 0.05 * r(rows, 2)).contiguous(), logp=(logp + far(rows)).contiguous(),
                adv=r(rows), returns=r(rows), values=(fc["y"][:, 0].float() + far(rows)).contiguous())
    return flat, torch.tensor([0.85, 1.05], device=DEV)


def _bands(ac, flat, sigma_old, activation, tb, chunk=65536):
    """branch_bands of every row, in chunks; tb = tau_branch(D)"""
    P = R.nets64(ac)
    out = []
    rows = flat["adv"].shape[0]
    tau, tau_z = tb["loss"], {"z1": tb["z1"], "z2": tb["z2"]}
    for s in range(0, rows, chunk):
        b = R.to64({k: v[s:s + chunk] for k, v in flat.items()})
        fa, fc = R.forward(P["actor"], b["obs"], activation), R.forward(P["critic"], b["obs"], activation)
        L = R.losses(P, b, sigma_old, fa, fc, CLIP, 1.0, True)
        out.append(R.branch_bands(dict(loss=L, fa=fa, fc=fc, adv=b["adv"]), CLIP, tau, activation, tau_z))
        del fa, fc, L, b
    return {k: torch.cat([o[k] for o in out]) for k in out[0]}


def _perm_excusing(bands, rows, mb, seed):
    """a permutation of the rows whose last minibatch (the one under test) holds no sample inside a band"""
    perm = torch.randperm(rows, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    bad = bands["any"][perm]
    n_bad = int(bad.sum())
    assert n_bad < 0.01 * rows, ("excused share", n_bad / rows)
    assert n_bad <= rows - mb
    perm = torch.cat([perm[bad], perm[~bad]])
    return perm.to(torch.int32), n_bad


def _check_row(got, res, tau, n2_got, n_sum, what):
    """every element + statistics within tau m + floor; the squared norm within its own bound; returns max err / bound"""
    G = res["n_params"]
    g64, m = res["grad"], res["mag"]
    got = got[:G + 3].double()
    bound = tau * m + FLOOR
    err = (got - g64).abs()
    worst = float((err / bound).max())
    assert bool(torch.isfinite(got).all()), what
    # parameter gradients first, then the three loss sums: a failure names which
    for name, sl in (("parameter gradient", slice(0, G)), ("loss sum", slice(G, G + 3))):
        q = err[sl] / bound[sl]
        i = int(q.argmax())
        assert float(q[i]) <= 1.0, (what, name, i, float(got[sl][i]), float(g64[sl][i]), float(m[sl][i]), float(q[i]))
    gp = g64[:G]
    n2 = float((gp * gp).sum())
    n2_bound = float((2 * gp.abs() * tau * m[:G] + (tau * m[:G]) ** 2).sum()) + n_sum * R.U * n2 + FLOOR
    n2_err = abs(float(n2_got) - n2)
    assert n2_err <= n2_bound, (what, "norm2", float(n2_got), n2, n2_bound)
    return max(worst, n2_err / n2_bound)


def _run_drift(ac, flat, perm, mb_start, mb, sigma_old):
    from wheeledlab_amd.rl.ppo import PPO, FusedPpoStep
    fz = FusedPpoStep(ac, PPO(ac))
    grad = fz.gradients(flat, perm, mb_start, mb, sigma_old).clone()
    torch.cuda.synchronize()
    return grad, float(fz.ctrl[2 + fz.parity])


def _reference(ac, flat, perm, mb_start, mb, sigma_old, activation):
    idx = perm[mb_start:mb_start + mb].long()
    b = R.to64({k: v[idx] for k, v in flat.items()})
    return R.minibatch_gradients(R.nets64(ac), b, sigma_old, activation, clip=CLIP)


@pytest.mark.parametrize("activation", ["elu", "relu"])
@pytest.mark.parametrize("mb", [32768, 131072, 16385, 65537])
def test_drift_gradient_row_at_training_sizes(mb, activation):
    """the drift learner's row at the run config's minibatch (1024 envs x 128 steps / 4: two tiles per wavefront), at
    4096 envs (eight), and at ragged sizes that saturate the grid with unequal tile counts per wavefront"""
    rows = 4 * mb
    ac = _nets(14, activation, seed=mb % 1000)
    flat, sigma_old = _batch(ac, rows, 14, activation, seed=mb + 1)
    tau, d = tau_drift(mb)
    bands = _bands(ac, flat, sigma_old, activation, tau_branch(14))
    perm, n_bad = _perm_excusing(bands, rows, mb, seed=mb + 2)
    start = rows - mb
    grad, n2 = _run_drift(ac, flat, perm, start, mb, sigma_old)
    res = _reference(ac, flat, perm, start, mb, sigma_old, activation)
    worst = _check_row(grad, res, tau, n2, 8 + _ceil(10440, 64), f"drift mb {mb}")
    print(f"drift {activation} mb {mb}: T {d['T']} blocks {d['blocks']} n {d['n']} tau {tau:.3g}  max err/bound {worst:.3g}"
          f"  excused {n_bad} / {rows}")


def _run_wide(ac, flat, perm, mb_start, mb, sigma_old, capacity):
    from wheeledlab_amd.rl.ppo import PPO, FusedWidePpoStep
    fz = FusedWidePpoStep(ac, PPO(ac), capacity, mb)
    fz.stage(flat["obs"], perm)
    grad = fz.gradients(flat, perm, mb_start, mb, sigma_old).clone()
    torch.cuda.synchronize()
    out = grad, float(fz.ctrl[fz._A.PPO_CTRL_NORM2 + fz.parity]), fz.splits, fz.dp
    del fz
    return out


@pytest.mark.parametrize("D,capacity,mb", [
    (689, 524288, 131072),     # elevation agent, 4096 envs x 128 steps: 8 tiles per wavefront, 16 K chunks per split
    (689, 131072, 32768),      # elevation agent, 1024 envs: 2 tiles, 4 chunks per split
    (3208, 65536, 16384),      # visual agent, 512 envs: 16 chunks per split
    (4808, 65536, 16384),      # visual-depth agent (VISUAL_DEPTH_CONFIG)
])
def test_wide_gradient_row_at_training_sizes(D, capacity, mb):
    """the wide learner's row where the tail runs several tiles per wavefront and the dW1 contraction's K loop several
    chunks per split (its double-buffered steady state)"""
    from wheeledlab_amd.rl.ppo import FusedWidePpoStep
    ac = _nets(D, "elu", seed=D)
    flat, sigma_old = _batch(ac, capacity, D, "elu", seed=D + capacity)
    dp = _ceil(D, 64) * 64
    tau, d = tau_wide(D, mb, FusedWidePpoStep.pick_splits(dp, mb))
    assert d["cps"] >= 4, d
    bands = _bands(ac, flat, sigma_old, "elu", tau_branch(D))
    perm, n_bad = _perm_excusing(bands, capacity, mb, seed=D + 3)
    del bands
    start = capacity - mb
    grad, n2, splits, dp_k = _run_wide(ac, flat, perm, start, mb, sigma_old, capacity)
    assert dp_k == dp
    res = _reference(ac, flat, perm, start, mb, sigma_old, "elu")
    worst = _check_row(grad, res, tau, n2, 8 + _ceil(10440, 64) + dp * 128 // 256, f"wide D {D} mb {mb}")
    print(f"wide D {D} cap {capacity} mb {mb}: splits {splits} chunks/split {d['cps']} T {d['T']} n {d['n']} tau {tau:.3g}"
          f"  max err/bound {worst:.3g}  excused {n_bad} / {capacity}")
    del flat, res, grad
    torch.cuda.empty_cache()


# ---- branch-dense batches -------------------------------------------------------------------------------------------------
def _place_branches(ac, flat, sigma_old, activation, tb, seed):
    """rewrite the rows so that most samples sit just outside the fp32 band of a branch, on both sides of it.  Row group
    (index mod 16): 0-7 ratio = (1 +- clip)(1 +- k 1e-4) with k 1e-4 >= 1.5 x the band, adv > 0 / < 0; 8 the same with
    adv = 0; 9-12 |v - v_old| = clip (1 +- k 1e-4) with the return beyond v (the clipped square wins outside); 13-14
    l1 = l2 +- 1.5 x the band with |v - v_old| = 1.5 clip; 15 (ReLU) a layer-1 or layer-2 pre-activation of the actor or
    the critic at +- 1.5-3 x its band.  Returns the group of every row and the side each sample should take."""
    rows = flat["adv"].shape[0]
    g = torch.Generator(device=DEV).manual_seed(seed)
    uni = lambda *s: torch.rand(*s, device=DEV, generator=g, dtype=torch.float64)
    grp = torch.arange(rows, device=DEV) % 16
    P = R.nets64(ac)
    if activation == "relu":
        # group 15: a pre-activation of (actor, critic) x (layer 1, layer 2) -- by row / 16 mod 4 -- at 1.5-3 x its band,
        # either sign: Newton steps on the observation feature that moves it most
        sel = grp == 15
        x = flat["obs"][sel].double()
        n_sel = x.shape[0]
        ar = torch.arange(n_sel, device=DEV)
        kind = (torch.nonzero(sel)[:, 0] // 16) % 4
        u = torch.randint(0, 64, (n_sel,), device=DEV, generator=g)
        sign = torch.where((ar // 4) % 2 == 0, 1.0, -1.0).double()     # both signs for every kind
        scale = 1.5 * (1.0 + uni(n_sel))
        for net_i, net in enumerate(("actor", "critic")):
            for layer in (1, 2):
                k = kind == 2 * net_i + layer - 1
                xs, us = x[k], u[k]
                ak = torch.arange(xs.shape[0], device=DEV)
                W = P[net]
                for _ in range(4):
                    f = R.forward(W, xs, activation)
                    z, mz = f[f"z{layer}"][ak, us], f[f"m_z{layer}"][ak, us]
                    dz = W["w1"][us] if layer == 1 else (W["w2"][us][:, :, None] * f["dh1"][:, :, None] * W["w1"][None]).sum(1)
                    feat = dz.abs().argmax(1)
                    target = sign[k] * scale[k] * tb[f"z{layer}"] * mz
                    xs[ak, feat] += (target - z) / dz[ak, feat]
                    xs = xs.float().double()
                x[k] = xs
        flat["obs"][sel] = x.float()
    b = R.to64(flat)
    fa, fc = R.forward(P["actor"], b["obs"], activation), R.forward(P["critic"], b["obs"], activation)
    L = R.losses(P, b, sigma_old, fa, fc, CLIP, 1.0, True)
    # ratio groups
    hi_side = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0, 1], device=DEV)
    out_side = torch.tensor([1, 0, 1, 0, 0, 1, 0, 1, 1], device=DEV)          # 1: the ratio beyond the threshold (away from 1)
    adv_sign = torch.tensor([1.0, 1.0, -1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 0.0], device=DEV, dtype=torch.float64)
    rg = grp <= 8
    gi = grp[rg]
    base = torch.where(hi_side[gi] == 1, 1.0 + CLIP, 1.0 - CLIP).double()
    m_arg = L["m_logp"][rg] + (L["logp"][rg] - torch.log(base)).abs() + 1.0
    tau = tb["loss"]
    band = tau * (1.0 + 2.0 * m_arg)                                            # relative band of the ratio
    k = torch.ceil(1.5 * band / 1e-4) + torch.floor(20 * uni(int(rg.sum())))
    off = k * 1e-4
    away = torch.where(hi_side[gi] == 1, 1.0, -1.0).double() * torch.where(out_side[gi] == 1, 1.0, -1.0).double()
    ratio = base * (1.0 + away * off)
    flat["logp"][rg] = (L["logp"][rg] - torch.log(ratio)).float()
    flat["adv"][rg] = (adv_sign[gi] * (0.2 + b["adv"][rg].abs())).float()
    # |v - v_old| around clip
    v = fc["y"][:, 0]
    vg = (grp >= 9) & (grp <= 12)
    gi = grp[vg]
    s = torch.where((gi == 9) | (gi == 10), 1.0, -1.0).double()
    outside = (gi == 9) | (gi == 11)
    m_dvo = fc["m_y"][vg, 0] + v[vg].abs() + CLIP + 1.0
    k = torch.ceil(1.5 * tau * m_dvo / (CLIP * 1e-4)) + torch.floor(20 * uni(int(vg.sum())))
    dvo = s * CLIP * (1.0 + torch.where(outside, 1.0, -1.0).double() * k * 1e-4)
    flat["values"][vg] = (v[vg] - dvo).float()
    flat["returns"][vg] = (v[vg] + s * (0.5 + uni(int(vg.sum())))).float()      # beyond v on the side of v - v_old
    # l1 = l2 +- band, |dvo| = 1.5 clip
    lg = (grp == 13) | (grp == 14)
    gi = grp[lg]
    n_l = int(lg.sum())
    s = torch.where(uni(n_l) < 0.5, 1.0, -1.0).double()
    vv = v[lg]
    v_old = vv - s * 1.5 * CLIP
    vc = v_old + s * CLIP
    mid = 0.5 * (vv + vc)
    m_l = 4.0 * (vv - vc).abs() * (fc["m_y"][lg, 0] + vv.abs() + mid.abs() + CLIP + 1.0)
    eps = 1.5 * tau * m_l / (2.0 * (vv - vc).abs()) * (1.0 + uni(n_l))
    flat["values"][lg] = v_old.float()
    flat["returns"][lg] = (mid + torch.where(gi == 13, 1.0, -1.0).double() * eps).float()
    return grp


def _branch_counts(res, grp, activation, tb):
    """every branch side is populated in the tested minibatch, and each placed sample is on the side it was put"""
    L = res["loss"]
    adv = res["adv"]
    r = L["ratio"]
    c = {}
    c["ratio>1+c adv>0 (clipped)"] = int(((r > 1 + CLIP) & (adv > 0) & ~L["unclipped"]).sum())
    c["ratio<1+c adv>0"] = int(((r < 1 + CLIP) & (r > 1 + CLIP - 0.05) & (adv > 0) & L["unclipped"]).sum())
    c["ratio>1+c adv<0"] = int(((r > 1 + CLIP) & (adv < 0) & L["unclipped"]).sum())
    c["ratio<1-c adv<0 (clipped)"] = int(((r < 1 - CLIP) & (adv < 0) & ~L["unclipped"]).sum())
    c["ratio>1-c adv<0"] = int(((r > 1 - CLIP) & (r < 1 - CLIP + 0.05) & (adv < 0) & L["unclipped"]).sum())
    c["ratio<1-c adv>0"] = int(((r < 1 - CLIP) & (adv > 0) & L["unclipped"]).sum())
    c["adv=0 at 1+-c"] = int(((adv == 0) & (grp == 8)).sum())
    out = ~L["inside"]
    c["|dvo|>c clipped square"] = int((out & L["take2"] & (grp >= 9) & (grp <= 12)).sum())
    c["|dvo|<=c"] = int((L["inside"] & (grp >= 9) & (grp <= 12)).sum())
    c["l2>l1 outside"] = int((out & L["take2"] & ((grp == 13) | (grp == 14))).sum())
    c["l1>=l2 outside"] = int((out & ~L["take2"] & ((grp == 13) | (grp == 14))).sum())
    if activation == "relu":
        for net, f in (("actor", res["fa"]), ("critic", res["fc"])):
            for k in ("z1", "z2"):
                z, m = f[k][grp == 15], f["m_" + k][grp == 15]
                near = (z.abs() <= 4 * tb[k] * m) & (z.abs() > tb[k] * m)
                c[f"relu {net} {k} just > 0"] = int((near & (z > 0)).any(1).sum())
                c[f"relu {net} {k} just < 0"] = int((near & (z < 0)).any(1).sum())
    return c


@pytest.mark.parametrize("form,activation", [("drift", "elu"), ("drift", "relu"), ("wide", "elu")])
def test_branch_dense_batches(form, activation):
    mb = 32768
    rows = 4 * mb
    D = 14 if form == "drift" else 689
    ac = _nets(D, activation, seed=77)
    flat, sigma_old = _batch(ac, rows, D, activation, seed=78)
    tb = tau_branch(D)
    grp = _place_branches(ac, flat, sigma_old, activation, tb, seed=79)
    bands = _bands(ac, flat, sigma_old, activation, tb)
    perm, n_bad = _perm_excusing(bands, rows, mb, seed=80)
    start = rows - mb
    if form == "drift":
        tau, _ = tau_drift(mb)
        grad, n2 = _run_drift(ac, flat, perm, start, mb, sigma_old)
        n_sum = 8 + _ceil(10440, 64)
    else:
        from wheeledlab_amd.rl.ppo import FusedWidePpoStep
        tau, _ = tau_wide(D, mb, FusedWidePpoStep.pick_splits(704, mb))
        grad, n2, _, _ = _run_wide(ac, flat, perm, start, mb, sigma_old, rows)
        n_sum = 8 + _ceil(10440, 64) + 704 * 128 // 256
    res = _reference(ac, flat, perm, start, mb, sigma_old, activation)
    counts = _branch_counts(res, grp[perm[start:].long()], activation, tb)
    worst = _check_row(grad, res, tau, n2, n_sum, f"branch-dense {form} {activation}")
    print(f"branch-dense {form} {activation}: max err/bound {worst:.3g}  excused {n_bad} / {rows} "
          f"({', '.join(f'{k}: {v}' for k, v in bands.items() if k != 'any' for v in [int(v.sum())])})  sides {counts}")
    assert all(v > 0 for v in counts.values()), counts


# ---- the apply stage on hand-set rows -------------------------------------------------------------------------------------
def _learner(form):
    from wheeledlab_amd.rl.ppo import PPO, FusedPpoStep, FusedWidePpoStep
    if form == "drift":
        ac = _nets(14, "elu", seed=5)
        return ac, FusedPpoStep(ac, PPO(ac))
    ac = _nets(100, "relu", seed=6)
    return ac, FusedWidePpoStep(ac, PPO(ac), 128, 64)


def _apply(fz, form, mb, parity, step):
    call = fz.lib.wl_ppo_apply if form == "drift" else fz.lib.wl_ppo_wide_apply
    rc = call(C.byref(fz._actor), C.byref(fz._critic), fz.ac.std.data_ptr(), int(mb), C.byref(fz.hp), C.byref(fz.state),
              parity, step, fz._stream())
    assert rc == 0
    torch.cuda.synchronize()


def _f32(x):
    return float(np.float32(x))


APPLY_CASES = [
    # name, S_KL / mb (the mean KL), mb, lr_old, norm factor (n2 = f max_grad_norm^2), step, moments
    ("kl = 2 desired", "2d", 1, 1e-3, 0.25, 1, None),
    ("kl = 2 desired + 1 ulp", "2d+", 32768, 1e-3, 0.25, 1, None),
    ("kl = 2 desired - 1 ulp", "2d-", 1, 1e-3, 0.25, 1, None),
    ("kl = desired / 2", "d/2", 32768, 1e-3, 0.25, 1, None),
    ("kl = desired / 2 - 1 ulp", "d/2-", 1, 1e-3, 0.25, 1, None),
    ("kl = desired / 2 + 1 ulp", "d/2+", 32768, 1e-3, 0.25, 1, None),
    ("kl = 0", 0.0, 1, 1e-3, 0.25, 1, None),
    ("kl < 0", -1e-4, 1, 1e-3, 0.25, 1, None),
    ("lr at lr_min, kl high", 1.0, 1, 1e-5, 0.25, 1, None),
    ("lr at lr_max, kl low", 1e-4, 1, 1e-2, 0.25, 1, None),
    ("norm at the knee", 0.0, 1, 1e-3, 1.0, 1, None),
    ("norm above the knee", 0.0, 1, 1e-3, 100.0, 1, None),
    ("step 1e4 after loaded moments", 0.0, 1, 1e-3, 100.0, 10000, "loaded"),
    ("step 2 after loaded moments, kl high", 0.05, 4096, 3e-3, 0.5, 2, "loaded"),
]


@pytest.mark.parametrize("form", ["drift", "wide"])
def test_apply_stage_on_hand_set_rows(form):
    ac, fz = _learner(form)
    A = fz._A
    G = sum(p.numel() for p in ac.parameters())
    hp = fz.hp
    d = np.float32(hp.desired_kl)
    kl_of = {"2d": d * np.float32(2), "2d+": np.nextafter(d * np.float32(2), np.float32(1)),
             "2d-": np.nextafter(d * np.float32(2), np.float32(0)), "d/2": d * np.float32(0.5),
             "d/2-": np.nextafter(d * np.float32(0.5), np.float32(0)), "d/2+": np.nextafter(d * np.float32(0.5), np.float32(1))}
    gen = torch.Generator(device=DEV).manual_seed(12)
    decisions = set()
    for ci, (name, kl, mb, lr_old, nf, step, moments) in enumerate(APPLY_CASES):
        parity = ci & 1
        kl32 = np.float32(kl_of[kl] if isinstance(kl, str) else kl)
        grad = 1e-2 * torch.randn(G, device=DEV, generator=gen)
        grad[torch.rand(G, device=DEV, generator=gen) < 0.1] = 0.0          # zero entries: eps dominates Adam's denominator
        if moments == "loaded":
            fz.adam_m[:G] = 1e-3 * torch.randn(G, device=DEV, generator=gen)
            fz.adam_v[:G] = (1e-3 * torch.randn(G, device=DEV, generator=gen)) ** 2
            fz.adam_m[:G][grad == 0] = 0.0
        else:
            fz.adam_m.zero_()
            fz.adam_v.zero_()
        std_snap = torch.tensor([0.7, 1.3], device=DEV)
        es = -np.float64(np.float32(hp.entropy_coef)) / std_snap.double()
        g64 = grad.double()
        corr = float(((g64[:2] + es) ** 2 - g64[:2] ** 2).sum())
        mgn = float(np.float32(hp.max_grad_norm))
        n2 = _f32(nf * mgn * mgn - corr)                                   # the norm the clipping sees = sqrt(nf) max_grad_norm
        fz.grad.zero_()
        fz.grad[:G] = grad
        fz.grad[G + 2] = float(kl32) * mb                                  # mb a power of two or 1: the mean is exactly kl32
        fz.grad[G] = 1.0
        fz.grad[G + 1] = -0.5
        fz.ctrl.zero_()
        fz.ctrl[A.PPO_CTRL_LR + parity] = lr_old
        fz.ctrl[A.PPO_CTRL_NORM2 + parity] = n2
        fz.ctrl[A.PPO_CTRL_STD:A.PPO_CTRL_STD + 2] = std_snap
        p0 = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).double()
        m0, v0 = fz.adam_m[:G].double(), fz.adam_v[:G].double()
        _apply(fz, form, mb, parity, step)
        lr_want, decision = R.lr_rule_f32(np.float32(fz.grad[G + 2].item()), mb, np.float32(lr_old), d, np.float32(hp.lr_min),
                                          np.float32(hp.lr_max))
        decisions.add(decision)
        lr_got = np.float32(fz.ctrl[A.PPO_CTRL_LR + (parity ^ 1)].item())
        assert lr_got.view(np.uint32) == np.float32(lr_want).view(np.uint32), (form, name, lr_got, lr_want, decision)
        assert float(fz.ctrl[A.PPO_CTRL_NORM2 + (parity ^ 1)]) == 0.0
        p_want, m_want, v_want, upd = R.apply_step(p0, g64, m0, v0, step, float(lr_want), std_snap, n2,
                                                   entropy_coef=float(np.float32(hp.entropy_coef)), max_grad_norm=mgn,
                                                   beta1=float(np.float32(hp.beta1)), beta2=float(np.float32(hp.beta2)),
                                                   eps=float(np.float32(hp.eps)))
        p_got = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).double()
        ulp = torch.from_numpy(np.spacing(np.abs(p_want.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(DEV)
        # + the fp32 bias corrections 1 - beta^t: beta^t is rounded once (powf), the subtraction is exact and leaves that
        # rounding relative to 1 - beta^t (step 2: 500 u of the update through bc2)
        b1, b2 = float(np.float32(hp.beta1)), float(np.float32(hp.beta2))
        rel = 16 * R.U + 2 * R.U * (b1 ** step / (1 - b1 ** step) + b2 ** step / (1 - b2 ** step)) * (step > 1)
        bound = ulp + rel * upd                                            # one fp32 rounding of the result (either binade)
        err = (p_got - p_want).abs()
        assert bool((err <= bound).all()), (form, name, float((err / bound).max()))
        unchanged = (g64 == 0) & (m0 == 0)
        unchanged[:2] = False                                              # std: the entropy term makes its gradient nonzero
        assert bool((p_got[unchanged] == p0[unchanged]).all()), (form, name)
        # the moments: a few roundings of their terms' magnitudes (the entropy term on std, coefficient <= 1)
        ga = g64.abs()
        ga[:2] += es.abs()
        m_mag = float(np.float32(hp.beta1)) * m0.abs() + 0.1 * ga
        v_mag = float(np.float32(hp.beta2)) * v0 + 1e-3 * ga * ga
        assert bool(((fz.adam_m[:G].double() - m_want).abs() <= 8 * R.U * m_mag + FLOOR).all()), (form, name)
        assert bool(((fz.adam_v[:G].double() - v_want).abs() <= 8 * R.U * v_mag + FLOOR).all()), (form, name)
        print(f"apply {form} {name}: lr {lr_old:g} -> {float(lr_got):.9g} ({decision}), max err/bound {float((err / bound).max()):.3g}")
    assert decisions == {"up", "down", "keep"}


# ---- GAE and the rollout bookkeeping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n", [(128, 4096), (128, 4097), (1, 4097), (9, 300)])
def test_gae_and_normalisation_at_training_sizes(K, n):
    """wl_gae's returns vs float64 (n = 5 K + 3 roundings on the recursion's path: delta 3, the carry 2, + the return),
    and the advantage normalisation over all K n values vs float64 of the float64 advantages"""
    from wheeledlab_amd.policy import RolloutStorage
    st = RolloutStorage(K, n, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(K * n)
    st.rewards.copy_(torch.randn(K, n, device=DEV, generator=g))
    st.values.copy_(3.0 * torch.randn(K + 1, n, device=DEV, generator=g))
    st.dones.copy_((torch.rand(K, n, device=DEV, generator=g) < 0.02).long())
    st.dones[0, : n // 8] = 1                          # episodes ending at the first and the last step
    st.dones[K - 1, n // 8: n // 4] = 1
    ret, adv_n = st.compute_returns(0.99, 0.95)
    torch.cuda.synchronize()
    r64, a64, madv, mret = R.gae64(st.rewards, st.values, st.dones, 0.99, 0.95)
    tau = (5 * K + 3) * R.U
    # the raw advantages wl_gae writes (a common scale error would cancel in the normalisation)
    from wheeledlab_amd import _abi as A
    adv_raw, ret_raw = torch.empty_like(st.rewards), torch.empty_like(st.rewards)
    A.check(A.load().wl_gae(K, n, st.rewards.data_ptr(), st.values.data_ptr(), st.dones.data_ptr(), 0.99, 0.95, ret_raw.data_ptr(),
                            adv_raw.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "wl_gae")
    torch.cuda.synchronize()
    assert torch.equal(ret_raw, ret)
    worst_a = float(((adv_raw.double() - a64).abs() / (tau * madv + FLOOR)).max())
    assert worst_a <= 1.0, worst_a
    err = (ret.double() - r64).abs()
    worst = float((err / (tau * mret + FLOOR)).max())
    assert worst <= 1.0, worst
    # normalisation (torch's mean / std of the fp32 advantages; 1024 roundings bound the depth of its reductions here)
    N = K * n
    mean, std = a64.mean(), a64.std()
    tau_m = tau * float(madv.mean()) + 1024 * R.U * float(a64.abs().mean())
    tau_s = (tau * float((a64 - mean).abs().mul(madv).mean()) + 1024 * R.U * float(((a64 - mean) ** 2).mean())) / float(std) + tau_m
    want = (a64 - mean) / (std + 1e-8)
    bound = (tau * madv + tau_m) / float(std) + want.abs() * tau_s / float(std) + 4 * R.U * (want.abs() + 1)
    err_n = (adv_n.double() - want).abs()
    worst_n = float((err_n / bound).max())
    assert worst_n <= 1.0, worst_n
    print(f"gae K {K} n {n}: advantages max err/bound {worst_a:.3g}, returns {worst:.3g}, normalised advantages {worst_n:.3g} (N {N})")


@pytest.mark.parametrize("K,n", [(128, 4097), (1, 300), (9, 4097)])
def test_rollout_bookkeeping_at_training_sizes(K, n):
    """finished-episode returns / lengths, carries, the raw reward sums, the non-finite action count and the time-out
    bootstrap vs float64 / exact counts; dones at t = 0 and t = K - 1, time-outs on a subset of them"""
    from wheeledlab_amd import _abi as A
    g = torch.Generator(device=DEV).manual_seed(K + n)
    rewards = torch.randn(K, n, device=DEV, generator=g)
    values = 2.0 * torch.randn(K, n, device=DEV, generator=g)
    dones = (torch.rand(K, n, device=DEV, generator=g) < 0.05).long()
    dones[0, : n // 8] = 1
    dones[K - 1, n // 8: n // 4] = 1
    time_outs = (dones == 1) & (torch.rand(K, n, device=DEV, generator=g) < 0.5)
    actions = torch.randn(K, n, 2, device=DEV, generator=g)
    actions[K // 2, :7, 0] = float("nan")
    actions[0, 10:13, 1] = float("inf")
    carry_ret = torch.randn(n, device=DEV, generator=g)
    carry_len = torch.randint(0, 50, (n,), device=DEV, generator=g).float()
    r0, cr0, cl0 = rewards.clone(), carry_ret.clone(), carry_len.clone()
    ep_ret, ep_len = torch.zeros(K, n, device=DEV), torch.zeros(K, n, device=DEV)
    nb = _ceil(n, 256)
    stats = torch.zeros(3, nb, device=DEV)
    gamma = 0.99
    lib = A.load()
    A.check(lib.wl_rollout_bookkeeping(K, n, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), time_outs.data_ptr(),
                                       actions.data_ptr(), gamma, carry_ret.data_ptr(), carry_len.data_ptr(), ep_ret.data_ptr(),
                                       ep_len.data_ptr(), stats.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "wl_rollout_bookkeeping")
    torch.cuda.synchronize()
    r64 = r0.double().cpu().numpy()
    d = dones.cpu().numpy()
    ret, ln = cr0.double().cpu().numpy(), cl0.double().cpu().numpy()
    mret = np.abs(ret)
    want_ret, want_len, bound_ret = np.zeros((K, n)), np.zeros((K, n)), np.zeros((K, n))
    for t in range(K):
        ret = ret + r64[t]
        mret = mret + np.abs(r64[t])
        ln = ln + 1
        e = d[t] != 0
        want_ret[t, e], want_len[t, e] = ret[e], ln[e]
        bound_ret[t, e] = (K + 1) * R.U * mret[e]
        ret[e], ln[e], mret[e] = 0.0, 0.0, 0.0
    got_ret, got_len = ep_ret.double().cpu().numpy(), ep_len.double().cpu().numpy()
    assert np.all(np.abs(got_ret - want_ret) <= bound_ret + FLOOR)
    assert np.array_equal(got_len[d != 0], want_len[d != 0])
    assert np.all(np.abs(carry_ret.double().cpu().numpy() - ret) <= (K + 1) * R.U * (mret + 1e-30) + FLOOR)
    assert np.array_equal(carry_len.double().cpu().numpy(), ln)
    # the time-out bootstrap: one fma, r + gamma V, rounded once
    to = time_outs.cpu().numpy()
    boot = r64 + np.float64(np.float32(gamma)) * values.double().cpu().numpy()
    want_r = np.where(to, boot, r64)
    got_r = rewards.double().cpu().numpy()
    assert np.all(np.abs(got_r - want_r) <= 0.5 * np.spacing(np.abs(want_r).astype(np.float32)).astype(np.float64))
    # per-block sums: raw rewards (K + 6 + 2 roundings per lane and block), non-finite components and episode ends exactly
    s = stats.double().cpu().numpy()
    blocks = np.arange(n) // 256
    rs = np.bincount(blocks, r64.sum(0), minlength=nb)
    mrs = np.bincount(blocks, np.abs(r64).sum(0), minlength=nb)
    assert np.all(np.abs(s[0] - rs) <= (K + 8) * R.U * mrs)
    bad = (~np.isfinite(actions.cpu().numpy())).sum(2).sum(0)
    assert np.array_equal(s[1], np.bincount(blocks, bad, minlength=nb).astype(np.float64))
    assert np.array_equal(s[2], np.bincount(blocks, (d != 0).sum(0), minlength=nb).astype(np.float64))
    assert s[1].sum() == 10

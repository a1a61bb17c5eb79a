"""The policy step restated in float64 (test infrastructure: never imported by the product): the actor mean, the Gaussian
draw, the log-prob and the critic's value that every collected transition stores, with a per-form error bound.

Forward.  `ppo_reference.forward` (values and first-order magnitudes m >= |q|, see that module) on float64 copies of the
nets, with its forward-only activation rule: ReLU and ELU are 1-Lipschitz, so where a pre-activation sits within its own
band |z| <= tau m(z) the activation's magnitude is m(z) -- an evaluation may land on either side of the kink -- where the
learner reference (which must also pick the derivative's branch) uses 0.  No row then needs to be excused.

Split-exact layer 1.  The bf16 forms split both operands of layer 1 into bf16 planes (x = hi + lo, round to nearest
even) and sum hx hw + lx hw + hx lw, dropping lo.lo; every such product is exact in fp32.  `split_operands` returns the
three products as one float64 contraction of width 3 D, so `forward` yields the split model's value AND its magnitude.
Each feature enters once with its own weight, whatever chunk holds it (the overlapped last 64-wide chunk holds zeros
for the features its predecessor covers).  Against this model a bf16 form is held to the fp32-accumulation part of tau
only; against exact float64 to that plus one split stage per product, SPLIT_STAGE: each operand's planes miss at most
2^-17 of it and the dropped |lx lw| is up to 2^-16 |x w|, so a product is off by < 2^-15 (1 + 2^-8) of |x w|.  (The
learner reference's 2^-16 per stage holds for its dense sums, not for one product: an impulse row whose lo plane is half
a bf16 ulp reaches 1.4 x 2^-16, measured by tests/test_policy_reference_cpu.py.)

tau per form, counted from the kernels as tests/test_gpu_ppo_reference.py counts: an MFMA adds a K-term tree to its
accumulator -- the product (f32 operands; bf16 products are exact), ceil(log2 K) levels and the accumulator add -- and
every further instruction on the same accumulator adds one.  Layer 1 (depth at the pre-activation z1):
  * f32 kernel (actor_critic_act_kernel): 4 (per + has_last) chained 16x16x4 MFMAs on the bias-seeded accumulator of a
    share: 4 (per + has_last) + 3; then the KS - 1 LDS fold adds (share j > 0: KS - j of them).  The largest share counts.
  * bf16 one launch (act_bf16_kernel): dp / 32 k-steps of 3 MFMAs (K 32: 5 levels) split into KS shares of `per` k-steps:
    3 per + 5; the fold hq = part 0 + part 1 + ... + part KS-1: KS - 1.
  * bf16 two launches (skinny_kernel + act_tail_kernel): 2 chunks of 6 MFMAs per split: 6 chunks + 5; the tail kernel adds
    rounds of 8 splits (3 levels + 1 add each, then one add per later round; the remainder round always runs): 3 + R,
    R = splits // 8 + 1.
  * form 2 (whole-width split, values_batched): 6 dp / 64 + 5, then one round: + 4.
  * wl_mlp_forward / wl_drift_rollout_policy (mlp_eval): 4 k-steps, the bias on feature in_dim: 4 + 3 = 7.
  * wl_elev_collect_rollout: 8 wavefronts' partial sums of <= 6 chunks (4 6 + 3), added one by one onto the bias: + 8.
The tail (eval_tail / mlp_eval): ELU (scale, exp2, - 1) 3 | layer 2, 17 k-steps of 16x16x4: 4 + 16 = 20 | ELU 3 |
layer 3, 17 k-steps on two accumulators (9 and 8) and their add: 4 + 8 + 1 = 13  -> 39 after z1.
tau = n 2^-24 (+ SPLIT_STAGE where a bf16 form is held to exact float64).

The draw.  z0 = r cos(2 pi u1), z1 = r sin(2 pi u1), r = sqrt(-2 log(1 - u0)), (u0, u1) the first two Philox uniforms of
the policy stream (oracle/philox.py, bit exact on the device).  The kernels use the hardware v_log_f32, v_sqrt_f32 and
v_sin / v_cos (sincos_rev); their allowance is fixed here: 2^-20 relative on r, 2^-20 absolute on sin and cos, plus the
roundings of r c and of the fma a = std z + mu.  The log-prob -1/2 (z0^2 + z1^2) - log s0 - log s1 - log 2 pi is checked
against float64 from the kernel's own a and mu with LOG_ALLOW (2^-20 absolute per log_fast) on top of its rounding count.

Not covered: non-finite observations, and values beyond bf16 range (|x| > 3.39e38, where the split's hi overflows).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import ppo_reference as R
from oracle import philox as PH

U, BF16_STAGE, LOG_2PI, FIELDS = R.U, R.BF16_STAGE, R.LOG_2PI, R.NET_FIELDS
FLOOR = 1e-30
SPLIT_STAGE = 2.0 ** -15 + 2.0 ** -23   # one product of split-bf16 operands against the exact one, relative
TAIL = 3 + 20 + 3 + 13          # z1 -> output, see above
DRAW_R = 2.0 ** -20             # v_log_f32 + v_sqrt_f32, relative on r
DRAW_TRIG = 2.0 ** -20          # v_sin_f32 / v_cos_f32 of u1 revolutions, absolute
LOG_ALLOW = 2.0 ** -20          # log_fast(std), absolute per term
S_POLICY = 7                    # wl_rng.h WL_RS_POLICY
# env ids (seed 42, step 1234567) found on the CPU among 2^26 ids (u0 = 0) and 2^20 ids (the rest) with oracle/philox.py
DRAW_SEED, DRAW_STEP = 42, 1234567
DRAW_KEYS = {"u0=0": 13816689, "u0 max": 586372, "u1~0": 732133, "u1~1/4": 205435, "u1~1/2": 646172, "u1~3/4": 242450}


def _ceil(a, b):
    return -(-a // b)


# ---- nets ------------------------------------------------------------------------------------------------------------------
def mlp64(m) -> dict:
    """float64 copy of a wheeledlab_amd.policy.Mlp (w1..b3 tensors, nn.Linear layout) or of a dict of such tensors"""
    get = (lambda k: m[k]) if isinstance(m, dict) else (lambda k: getattr(m, k))
    return {k: get(k).detach().double().cpu().clone() for k in FIELDS}


def nets64(ac) -> dict:
    """the ActorCritic adapter of ppo_reference.nets64 (whose input holds torch Sequentials): std, actor, critic"""
    return {"std": ac.std.detach().double().cpu().clone(), "actor": mlp64(ac.actor), "critic": mlp64(ac.critic)}


def make_nets(D: int, kind: str, seed: int) -> dict:
    """float32 CPU parameters {actor: {w1..b3}, critic: {...}}: "default" = torch.nn.Linear's initialisation, "trained" = the
    weights x 4 and the columns of w1 spread over 1e3"""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        k = 1.0 / math.sqrt(i)
        return (torch.rand(o, i, generator=g) * 2 - 1) * k, (torch.rand(o, generator=g) * 2 - 1) * k

    out = {}
    for name, n_out in (("actor", 2), ("critic", 1)):
        w1, b1 = lin(64, D)
        w2, b2 = lin(64, 64)
        w3, b3 = lin(n_out, 64)
        if kind == "trained":
            col = 10.0 ** (torch.rand(D, generator=g) * 3 - 1.5)
            w1, w2, w3 = 4 * w1 * col[None], 4 * w2, 4 * w3
        out[name] = dict(w1=w1.float(), b1=b1.float(), w2=w2.float(), b2=b2.float(), w3=w3.float(), b3=b3.float())
    return out


def probe_tails(nets: dict, units) -> dict:
    """w2 = I, b2 = 0, w3 rows selecting units (actor: units[0], units[1]; critic: units[2]), b3 = 0: every output is one
    layer-1 pre-activation through the two activations (exact on the positive side)"""
    out = {}
    for name, sel in (("actor", units[:2]), ("critic", units[2:3])):
        p = dict(nets[name])
        p["w2"], p["b2"] = torch.eye(64), torch.zeros(64)
        p["w3"] = torch.zeros(len(sel), 64)
        for i, u in enumerate(sel):
            p["w3"][i, u] = 1.0
        p["b3"] = torch.zeros(len(sel))
        out[name] = p
    return out


# ---- rows ------------------------------------------------------------------------------------------------------------------
def boundaries(D: int) -> list:
    """features on share, 16-wide chunk, 64-wide chunk, split and tail boundaries of every form at width D"""
    b = {0, D - 1, (D >> 4) << 4, max(0, D - 64), min(D - 1, 63)}
    for step in (16, 64, 128):
        for k in range(step, D, step):
            b |= {k - 1, k}
    for ks in (2, 4):
        per = _ceil(D >> 4, ks)
        for k in range(1, ks):
            b |= {min(D - 1, 16 * per * k), min(D - 1, 16 * per * k - 1)}
    for ks in (4, 8):
        dp = _ceil(D, 64) * 64
        per = _ceil(dp // 32, ks)
        for k in range(1, ks):
            s = per * k
            if s < dp // 32:
                f = min(64 * (s >> 1), D - 64) + 32 * (s & 1)
                b |= {max(0, f - 1), f}
    return sorted(x for x in b if 0 <= x < D)


IMPULSE_MANTISSA = 1.0 + 2.0 ** -8 - 2.0 ** -20     # bf16 hi = 1, lo = almost half a bf16 ulp


def row_pool(D: int, seed: int) -> dict:
    """the row families: name -> float32 [rows, D]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(64, D, generator=g)
    x[:, 0::3] *= 30.0
    x[:, 1::3] *= 0.05
    imp = torch.zeros(D, D)
    sc = 2.0 ** torch.randint(-6, 7, (D,), generator=g).double()
    sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0).double()
    imp[torch.arange(D), torch.arange(D)] = (IMPULSE_MANTISSA * sc * sign).float()
    bnd = torch.tensor(boundaries(D))
    sp = torch.zeros(64, D)
    for i in range(64):
        f = bnd[torch.randperm(len(bnd), generator=g)[:8]]
        sp[i, f] = (torch.randn(len(f), generator=g) * 2.0 ** torch.randint(-4, 5, (len(f),), generator=g)).float()
    scan = (0.3 + 1e-3 * torch.randn(32, D, generator=g)).float()
    return {"impulse": imp, "sparse": sp, "scan": scan, "zero": torch.zeros(8, D), "randn": x.float()}


def kink_rows(nets: dict, D: int, tau_z1: float, seed: int) -> torch.Tensor:
    """128 rows: row i puts unit i % 64 of layer 1 (actor for i < 64, critic after) at 0, +-0.5 and +-2 tau m(z1), by moving
    the feature with the largest weight of that unit"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(128, D, generator=g).double()
    k = torch.tensor([0.0, 0.5, -0.5, 2.0, -2.0, 0.0, 1.0, -1.0]).double()
    for i in range(128):
        n = mlp64(nets["actor" if i < 64 else "critic"])
        u = i % 64
        f = int(n["w1"][u].abs().argmax())
        z = float(x[i] @ n["w1"][u] + n["b1"][u])
        m = float(x[i].abs() @ n["w1"][u].abs() + n["b1"][u].abs())
        x[i, f] += (float(k[i % 8]) * tau_z1 * m - z) / float(n["w1"][u, f])
    return x.float()


def steer_b2(nets: dict, rows: torch.Tensor, activation: str) -> dict:
    """b2 set so that unit u of layer 2 sits at 0 for row u (actor) / row 64 + u (critic) of `rows`: the second hidden layer's
    kink with real tails"""
    out = {}
    for j, name in enumerate(("actor", "critic")):
        p = dict(nets[name])
        n = mlp64(p)
        f = R.forward(n, rows[64 * j:64 * j + 64].double(), activation)
        p["b2"] = (n["b2"] - f["z2"].diagonal()).float()
        out[name] = p
    return out


def batch(D: int, n: int, seed: int, extra=None) -> tuple:
    """n rows drawn from the families (all of them, in order, when n is large enough; a random mix otherwise), the rest
    randn.  Returns (rows float32 [n, D], family index per row, family names)"""
    fam = row_pool(D, seed)
    if extra is not None:
        fam["kink"] = extra
    names = list(fam)
    pool = torch.cat([fam[k] for k in names])
    idx = torch.cat([torch.full((fam[k].shape[0],), i) for i, k in enumerate(names)])
    if n <= pool.shape[0]:
        sel = torch.randperm(pool.shape[0], generator=torch.Generator().manual_seed(seed))[:n]
        return pool[sel].contiguous(), idx[sel], names
    g = torch.Generator().manual_seed(seed + 1)
    rest = torch.randn(n - pool.shape[0], D, generator=g)
    return torch.cat([pool, rest]).contiguous(), torch.cat([idx, torch.full((rest.shape[0],), names.index("randn"))]), names


# ---- forms (restated from the launchers) -------------------------------------------------------------------------------------
def f32_form(D: int, n: int, nets: int = 3) -> tuple:
    """(KS, RT) of wl_actor_critic_act (wl_actor.hip, the `rt` / `rt_joint` / `ks` lines of the launcher)"""
    tiles = _ceil(n, 16)
    n_nets = 2 if nets == 3 else 1
    rt = 4 if tiles * n_nets >= 2048 else 2 if tiles * n_nets >= 512 else 1
    rt_joint = 4 if tiles * 2 >= 2048 else 2 if tiles * 2 >= 512 else 1
    rbj = _ceil(tiles, rt_joint)
    ks = 1
    while ks < 4 and rbj * 2 * ks < 1024 and (D >> 4) // (ks * 2) >= 8:
        ks *= 2
    return ks, rt


def bf16_form(D: int, n: int) -> tuple:
    """(KS, RT) of act_bf16_kernel as wl_actor_critic_act_planes picks it (reserved = 0)"""
    dp, tiles = _ceil(D, 64) * 64, _ceil(n, 16)
    if dp >= 1024:
        return (8, 2) if tiles >= 96 else (8, 1)
    return (4, 4) if tiles >= 192 else (4, 2) if tiles >= 96 else (4, 1)


def splits(D: int) -> int:
    """partial sums of the two-launch form (layer1_partials: 2 chunks of 64 per split)"""
    return _ceil(_ceil(D, 64), 2)


def form_name(form: str, D: int, n: int) -> str:
    if form == "f32":
        return "f32 KS%d RT%d" % f32_form(D, n)
    if form == "one":
        return "bf16-one KS%d RT%d" % bf16_form(D, n)
    if form == "two":
        return "bf16-two %d splits" % splits(D)
    return form


# ---- tau ---------------------------------------------------------------------------------------------------------------------
def depth_z1(form: str, D: int, n: int = 1) -> int:
    """roundings on the longest path to a layer-1 pre-activation (module docstring)"""
    if form == "f32":
        ks, _ = f32_form(D, n)
        n_full = D >> 4
        per = _ceil(n_full, ks)
        worst = 0
        for k in range(ks):
            c0 = min(k * per, n_full)
            c = min(c0 + per, n_full) - c0 + (1 if k == ks - 1 and D & 15 else 0)
            fold = ks - 1 if k == 0 else ks - k
            worst = max(worst, (4 * c + 3 if c else 0) + fold)
        return worst
    dp = _ceil(D, 64) * 64
    if form == "one":
        ks, _ = bf16_form(D, n)
        per = _ceil(dp // 32, ks)
        return 3 * per + 5 + ks - 1
    if form == "two":
        s = splits(D)
        chunks = min(2, dp // 64)
        return 6 * chunks + 5 + 3 + s // 8 + 1
    if form == "whole":
        return 6 * (dp // 64) + 5 + 4
    if form == "mlp":
        return 7
    if form == "elev":
        return 4 * 6 + 3 + 8
    raise ValueError(form)


def taus(form: str, D: int, n: int = 1) -> dict:
    """z1: the layer-1 depth; out: to the outputs; split: + the split stage (bf16 forms held to exact float64)"""
    d = depth_z1(form, D, n)
    st = SPLIT_STAGE if form in ("one", "two", "whole") else 0.0
    return dict(z1=d * U, z2=(d + 23) * U, out=(d + TAIL) * U, z1_exact=d * U + st, z2_exact=(d + 23) * U + st,
                out_exact=(d + TAIL) * U + st, n=d)


# ---- float64 forward ---------------------------------------------------------------------------------------------------------
def split_bf16(t: torch.Tensor) -> tuple:
    """f32 -> (hi, lo) bf16 planes as float64, round to nearest even (wl_bf16.h split_bf16_pair)"""
    t = t.float()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def split_operands(x: torch.Tensor, w1: torch.Tensor) -> tuple:
    """(x3 [n, 3D], w3 [64, 3D]) with x3 w3^T = sum_f hx hw + lx hw + hx lw (the split model, lo.lo dropped)"""
    hx, lx = split_bf16(x)
    hw, lw = split_bf16(w1)
    return torch.cat([hx, lx, hx], 1), torch.cat([hw, hw, lw], 1)


def forward64(net: dict, x: torch.Tensor, activation: str, tau: dict, split: bool = False) -> dict:
    """ppo_reference.forward of one net (float32 parameters) on float32 rows, with the forward-only kink rule at the bands of
    `tau`; split: layer 1 is the split-exact model"""
    n = mlp64(net)
    if split:
        x3, w3 = split_operands(x, net["w1"])
        return R.forward(dict(n, w1=w3), x3, activation, kink=tau)
    return R.forward(n, x.double(), activation, kink=tau)


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def draw64(env_ids, step: int, seed: int) -> dict:
    u = PH.uniform4(np.asarray(env_ids, dtype=np.uint64), step, S_POLICY, seed).astype(np.float64)
    r = np.sqrt(-2.0 * np.log1p(-u[0]))
    c, s = np.cos(2.0 * np.pi * u[1]), np.sin(2.0 * np.pi * u[1])
    return dict(u0=u[0], u1=u[1], r=r, z0=r * c, z1=r * s, c=c, s=s)


def draw_allowance(d: dict, std, a) -> np.ndarray:
    """|(a - mu) - std z64| allowed per row and action (a float32 [n, 2]; the difference is taken in float64)"""
    std = np.asarray(std, dtype=np.float64)
    r = d["r"]
    az = []
    for cs, z in ((d["c"], d["z0"]), (d["s"], d["z1"])):
        az.append(DRAW_R * r * np.abs(cs) + r * DRAW_TRIG + 2 * U * np.abs(z))
    return np.stack(az, 1) * std[None] + U * np.abs(np.asarray(a, dtype=np.float64)) + FLOOR


def logp64(a, mu, std) -> tuple:
    """log-prob from the kernel's own a and mu (float32 [n, 2]) in float64, and its bound: the magnitude pass of
    ppo_reference.losses at 8 roundings (z, its square, the sum, the fma pair, the constant) plus LOG_ALLOW per log"""
    a, mu, std = (np.asarray(t, dtype=np.float64) for t in (a, mu, std))
    z = (a - mu) / std[None]
    mz = (np.abs(a) + np.abs(mu)) / std[None]
    lp = -0.5 * (z * z).sum(1) - np.log(std).sum() - LOG_2PI
    m = (np.abs(z) * mz).sum(1) + 2.0 * np.abs(np.log(std)).sum() + LOG_2PI
    return lp, 8 * U * m + 2 * LOG_ALLOW + FLOOR


# ---- the checker -------------------------------------------------------------------------------------------------------------
def check(g, g64, m, tau: float, floor: float = FLOOR) -> tuple:
    """worst |g - g64| / (tau m + floor) and the number of elements above 1"""
    g, g64, m = (torch.as_tensor(t).double() for t in (g, g64, m))
    r = (g - g64).abs() / (tau * m + floor)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return (float(r.max()) if r.numel() else 0.0), int((r > 1).sum())


# ---- the GPU cases (tests/test_gpu_policy_reference.py; tests/test_policy_reference_cpu.py checks what they reach) -----------
F32_CASES = [(14, 1), (14, 17), (14, 4097), (14, 16401), (256, 1000), (256, 4096), (256, 16401), (689, 1), (689, 4096),
             (689, 8192), (689, 16401), (689, 32768), (3208, 4097), (4808, 1000)]
BF16_DS = [64, 65, 127, 128, 129, 689, 960, 1024, 1025, 3208, 4808]
BF16_NS = [1520, 1521, 3056, 3057]              # 95 / 96 and 191 / 192 row tiles
WHOLE_CASES = [(64, 1000), (689, 5000), (3208, 3000)]
MLP_CASES = [(i, o) for i in range(1, 16) for o in range(1, 5)]


def activation_of(D: int, n: int) -> str:
    return "elu" if (D + n) % 2 else "relu"

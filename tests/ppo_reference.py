"""One PPO minibatch step restated in float64 (test infrastructure: never imported by the product, and it calls none of the
product's `PPO` / `ActorCritic` code for the numbers it produces).

What it restates (the step `wl_ppo.hip` / `wl_ppo_wide.hip` and `rl/ppo.py::PPO._step` implement, rsl_rl's PPO.update):
  * the D-64-64-2 actor and D-64-64-1 critic (ELU or ReLU), forward and backward written out layer by layer;
  * the clipped surrogate, the (clipped) value loss and the KL statistic, every sample's branch decided in float64:
    the surrogate takes -adv * ratio where -adv * ratio >= -adv * clamp(ratio) (torch.max picks either on a tie, and on a
    tie both sides have the same gradient unless adv = 0, where both are 0), the value loss takes the clipped square where
    it is strictly larger, and the clamp passes a gradient where |v - v_old| <= clip;
  * the entropy bonus, `clip_grad_norm_` (norm + 1e-6, coefficient clamped at 1), the rsl_rl adaptive-KL rule with its
    lr clamps, and `torch.optim.Adam`.

The magnitude pass.  Every quantity q is carried with a magnitude m(q) >= |q|: leaves (the fp32 inputs) have m = |leaf|
(weights, exact and never rounded on their own, enter products with m = 0 against an operand whose m dominates), and
    m(a + b) = m(a) + m(b),   m(a b) = m(a) |b| + |a| m(b),   m(f(a)) = |f(a)| + |f'(a)| m(a)   (+ the function's own error)
-- the backward with every operand replaced by its absolute value, to first order.  By induction over the expression
graph, an fp32 evaluation in which every operation rounds with relative error <= u and every path from a leaf to q passes
at most n roundings has |fl(q) - q| <= n u m(q); an operation that multiplies operands split into two bf16 planes
(x = hi + lo, 16 significant bits; the dropped lo.lo product and the two plane roundings are < 2^-16 of |a b|) adds 2^-16
per such stage on the path.  So a kernel is held to  |g - g64| <= (n 2^-24 + s 2^-16) m(g) + floor, with n and s
counted from the kernel's own summation trees (the GPU tests do that count).  exp / log get m(exp a) = e^a (1 + m(a))
and m(log a) = 2 |log a| + m(a) / a: the hardware exp2 of a * log2(e) rounds the scaled argument once more (u |a| <=
u m(a), one more rounding on the path) and its result once (u e^a).

Not covered: ratio overflow.  When logp - logp_old is large enough that exp overflows, fp32 and float64 disagree about
where, and torch produces NaN in the gradient there too (inf * 0); the tests keep the ratio finite.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
BF16_STAGE = 2.0 ** -16  # one product of two split-bf16 operands (hi + lo), relative
LOG_2PI = math.log(2.0 * math.pi)
NET_FIELDS = ("w1", "b1", "w2", "b2", "w3", "b3")


def nets64(ac) -> dict:
    """float64 copies of an ActorCritic's parameters (rl/ppo.py: actor.{0,2,4}, critic.{0,2,4}, std)"""
    lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
    out = {"std": ac.std.detach().double().clone()}
    for name, seq in (("actor", ac.actor), ("critic", ac.critic)):
        w = {}
        for i, m in enumerate(lin(seq)):
            w[f"w{i + 1}"] = m.weight.detach().double().clone()
            w[f"b{i + 1}"] = m.bias.detach().double().clone()
        out[name] = w
    return out


def flat_params(P: dict) -> torch.Tensor:
    """torch named_parameters() order: std, actor.{w1,b1,w2,b2,w3,b3}, critic.{...}"""
    return torch.cat([P["std"].reshape(-1)] + [P[n][f].reshape(-1) for n in ("actor", "critic") for f in NET_FIELDS])


def unflat_params(flat: torch.Tensor, like: dict) -> dict:
    out, off = {"std": None, "actor": {}, "critic": {}}, 0
    k = like["std"].numel()
    out["std"], off = flat[:k].clone(), k
    for n in ("actor", "critic"):
        for f in NET_FIELDS:
            k = like[n][f].numel()
            out[n][f] = flat[off:off + k].view_as(like[n][f]).clone()
            off += k
    return out


def _act(z, mz, activation):
    """activation, its derivative, and their magnitudes.  ELU below 0 is exp(z) - 1 and its derivative is taken from the
    output as h + 1 (what the kernels do); ReLU's derivative is exact (0 / 1) -- its kink is a branch, not a rounding."""
    pos = z > 0
    if activation == "elu":
        e = torch.exp(torch.clamp(z, max=0.0))
        h = torch.where(pos, z, e - 1.0)
        mh = torch.where(pos, mz, e * (1.0 + mz) + 1.0)
        d = torch.where(pos, torch.ones_like(z), e)
        md = torch.where(pos, torch.zeros_like(z), mh + 1.0)
    elif activation == "relu":
        h = torch.where(pos, z, torch.zeros_like(z))
        mh = torch.where(pos, mz, torch.zeros_like(z))
        d = pos.to(z.dtype)
        md = torch.zeros_like(z)
    else:
        raise ValueError(activation)
    return h, mh, d, md


def forward(net: dict, x, activation, mx=None, kink=None):
    """layer by layer, values and magnitudes: dict z1, h1, dh1, z2, h2, dh2, y (+ m_*).  kink = {"z1": tau1, "z2": tau2}
    (forward-only callers, tests/policy_reference.py): where |z| <= tau m(z) the activation's magnitude is m(z) -- ReLU and
    ELU are 1-Lipschitz -- instead of the learner's rule above (None: the learner's rule)"""
    w1, b1, w2, b2, w3, b3 = (net[f] for f in NET_FIELDS)
    mx = x.abs() if mx is None else mx
    f = {"x": x, "m_x": mx}

    def act(k):
        h, mh, d, md = _act(f["z" + k], f["m_z" + k], activation)
        if kink is not None:
            mz = f["m_z" + k]
            mh = torch.where(f["z" + k].abs() <= kink["z" + k] * mz, torch.maximum(mh, mz), mh)
        f["h" + k], f["m_h" + k], f["dh" + k], f["m_dh" + k] = h, mh, d, md

    f["z1"] = x @ w1.t() + b1
    f["m_z1"] = mx @ w1.abs().t() + b1.abs()
    act("1")
    f["z2"] = f["h1"] @ w2.t() + b2
    f["m_z2"] = f["m_h1"] @ w2.abs().t() + b2.abs()
    act("2")
    f["y"] = f["h2"] @ w3.t() + b3
    f["m_y"] = f["m_h2"] @ w3.abs().t() + b3.abs()
    return f


def _exp(a, ma):
    e = torch.exp(a)
    return e, e * (1.0 + ma)


def losses(P: dict, b: dict, sigma_old, fa: dict, fc: dict, clip: float, value_loss_coef: float, use_clipped_value_loss: bool):
    """per-sample loss terms, their derivatives with respect to the nets' outputs (already divided by the batch size),
    the branch each sample took, and magnitudes of all of it"""
    B = b["adv"].shape[0]
    inv_b = 1.0 / B
    sig = P["std"]
    so = sigma_old.double()
    y, my = fa["y"], fa["m_y"]
    a = b["actions"]
    z = (a - y) / sig
    mz = (a.abs() + my) / sig
    logp = -0.5 * (z * z).sum(1) - torch.log(sig).sum() - LOG_2PI
    m_logp = (z.abs() * mz).sum(1) + 2.0 * torch.log(sig).abs().sum() + LOG_2PI
    arg = logp - b["logp"]
    m_arg = m_logp + b["logp"].abs()
    ratio, m_ratio = _exp(arg, m_arg)
    adv = b["adv"]
    rc = torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    s1, s2 = -adv * ratio, -adv * rc
    unclipped = s1 >= s2
    surr = torch.where(unclipped, s1, s2)
    m_surr = adv.abs() * torch.where(unclipped, m_ratio, rc)
    dl = torch.where(unclipped, -adv * ratio, torch.zeros_like(ratio)) * inv_b          # d loss / d logp
    m_dl = torch.where(unclipped, adv.abs() * m_ratio, torch.zeros_like(ratio)) * inv_b
    d_mu = dl[:, None] * z / sig                                                        # d loss / d mu
    m_d_mu = (m_dl[:, None] * z.abs() + dl.abs()[:, None] * mz) / sig
    zz1 = z * z - 1.0
    d_sigma = (dl[:, None] * zz1 / sig).sum(0)
    m_d_sigma = ((m_dl[:, None] * zz1.abs() + dl.abs()[:, None] * (2.0 * z.abs() * mz + 1.0)) / sig).sum(0)
    q = sig / so + 1e-5
    dmu = b["mu"] - y
    kl_d = torch.log(q) + (so * so + dmu * dmu) / (2.0 * sig * sig) - 0.5
    m_kl_d = 2.0 * torch.log(q).abs() + 1.0 + (so * so + 2.0 * dmu.abs() * (b["mu"].abs() + my)) / (2.0 * sig * sig) + 0.5
    kl, m_kl = kl_d.sum(1), m_kl_d.sum(1)
    # value loss
    v, mv = fc["y"][:, 0], fc["m_y"][:, 0]
    ret, v_old = b["returns"], b["values"]
    e1, m_e1 = v - ret, mv + ret.abs()
    dvo, m_dvo = v - v_old, mv + v_old.abs()
    inside = dvo.abs() <= clip
    e2 = v_old + torch.clamp(dvo, -clip, clip) - ret
    m_e2 = v_old.abs() + torch.where(inside, m_dvo, torch.full_like(dvo, clip)) + ret.abs()
    l1, l2 = e1 * e1, e2 * e2
    m_l1, m_l2 = 2.0 * e1.abs() * m_e1, 2.0 * e2.abs() * m_e2
    take2 = (l2 > l1) if use_clipped_value_loss else torch.zeros_like(inside)
    vloss = torch.where(take2, l2, l1)
    m_vloss = torch.where(take2, m_l2, m_l1)
    dvl = torch.where(take2, torch.where(inside, 2.0 * e2, torch.zeros_like(e2)), 2.0 * e1)
    m_dvl = torch.where(take2, torch.where(inside, 2.0 * m_e2, torch.zeros_like(e2)), 2.0 * m_e1)
    d_v = (value_loss_coef * inv_b) * dvl
    m_d_v = (value_loss_coef * inv_b) * m_dvl
    return dict(d_mu=d_mu, m_d_mu=m_d_mu, d_v=d_v[:, None], m_d_v=m_d_v[:, None], d_sigma=d_sigma, m_d_sigma=m_d_sigma,
                surr=surr, m_surr=m_surr, kl=kl, m_kl=m_kl, vloss=vloss, m_vloss=m_vloss,
                ratio=ratio, m_ratio=m_ratio, unclipped=unclipped, dvo=dvo, m_dvo=m_dvo, inside=inside,
                l1=l1, l2=l2, m_l1=m_l1, m_l2=m_l2, take2=take2, logp=logp, m_logp=m_logp)


def backward(net: dict, f: dict, d3, md3):
    """weight gradients of one net from d loss / d outputs (values, magnitudes), torch's [out, in] layouts"""
    w2, w3 = net["w2"], net["w3"]
    g = {}
    g["w3"] = d3.t() @ f["h2"]
    g["m_w3"] = md3.t() @ f["h2"].abs() + d3.abs().t() @ f["m_h2"]
    g["b3"], g["m_b3"] = d3.sum(0), md3.sum(0)
    g2, m_g2 = d3 @ w3, md3 @ w3.abs()
    d2 = g2 * f["dh2"]
    m_d2 = m_g2 * f["dh2"].abs() + g2.abs() * f["m_dh2"]
    g["w2"] = d2.t() @ f["h1"]
    g["m_w2"] = m_d2.t() @ f["h1"].abs() + d2.abs().t() @ f["m_h1"]
    g["b2"], g["m_b2"] = d2.sum(0), m_d2.sum(0)
    g1, m_g1 = d2 @ w2, m_d2 @ w2.abs()
    d1 = g1 * f["dh1"]
    m_d1 = m_g1 * f["dh1"].abs() + g1.abs() * f["m_dh1"]
    g["w1"] = d1.t() @ f["x"]
    g["m_w1"] = m_d1.t() @ f["x"].abs()
    g["b1"], g["m_b1"] = d1.sum(0), m_d1.sum(0)
    return g


def to64(b: dict) -> dict:
    return {k: v.double() for k, v in b.items()}


def minibatch_gradients(P: dict, b: dict, sigma_old, activation: str, clip: float = 0.2, value_loss_coef: float = 1.0,
                        use_clipped_value_loss: bool = True) -> dict:
    """d (surrogate + c_v value loss) / d parameters of the minibatch `b` (float64 tensors, rows in minibatch order) in
    named_parameters() order, followed by the value-loss, surrogate and KL SUMS -- the row the gradient kernels write --
    with its magnitude row `mag`; plus the per-sample loss record `loss` (branches, ratio, ...) and the forward passes."""
    fa = forward(P["actor"], b["obs"], activation)
    fc = forward(P["critic"], b["obs"], activation)
    L = losses(P, b, sigma_old, fa, fc, clip, value_loss_coef, use_clipped_value_loss)
    ga = backward(P["actor"], fa, L["d_mu"], L["m_d_mu"])
    gc = backward(P["critic"], fc, L["d_v"], L["m_d_v"])
    row = [L["d_sigma"]] + [ga[f].reshape(-1) for f in NET_FIELDS] + [gc[f].reshape(-1) for f in NET_FIELDS]
    mag = [L["m_d_sigma"]] + [ga["m_" + f].reshape(-1) for f in NET_FIELDS] + [gc["m_" + f].reshape(-1) for f in NET_FIELDS]
    stats = torch.stack([L["vloss"].sum(), L["surr"].sum(), L["kl"].sum()])
    m_stats = torch.stack([L["m_vloss"].sum(), L["m_surr"].sum(), L["m_kl"].sum()])
    return dict(grad=torch.cat(row + [stats]), mag=torch.cat(mag + [m_stats]), n_params=sum(t.numel() for t in row),
                loss=L, fa=fa, fc=fc, adv=b["adv"])


def branch_bands(res: dict, clip: float, tau: float, activation: str, tau_z=None) -> dict:
    """per sample: is any branch decision within the fp32 uncertainty band tau * m of its threshold?  (ratio vs 1 +- clip
    where adv != 0, |v - v_old| vs clip and l1 vs l2 where the value loss is clipped, ReLU pre-activations vs 0; `tau_z`:
    a band of their own for the pre-activations z1 / z2, whose paths are shorter)"""
    L = res["loss"]
    r, mr = L["ratio"], L["m_ratio"]
    live = res["adv"] != 0                     # adv = 0: both sides of the surrogate have gradient 0
    near_ratio = live & (((r - (1.0 + clip)).abs() <= tau * mr) | ((r - (1.0 - clip)).abs() <= tau * mr))
    near_dvo = (L["dvo"].abs() - clip).abs() <= tau * L["m_dvo"]
    # inside the clip range l1 = l2 up to rounding and both sides have the same gradient: only a tie outside it is a branch
    near_l = ~L["inside"] & ((L["l1"] - L["l2"]).abs() <= tau * (L["m_l1"] + L["m_l2"]))
    near_relu = torch.zeros_like(near_ratio)
    if activation == "relu":
        tz = tau_z or {}
        for f in (res["fa"], res["fc"]):
            for k in ("z1", "z2"):
                near_relu |= (f[k].abs() <= tz.get(k, tau) * f["m_" + k]).any(1)
    return dict(ratio=near_ratio, dvo=near_dvo, l=near_l, relu=near_relu, any=near_ratio | near_dvo | near_l | near_relu)


# ---- the apply stage ---------------------------------------------------------------------------------------------------
def lr_rule_f32(kl_sum, mb_size: int, lr_old, desired_kl, lr_min, lr_max):
    """the adaptive-KL rule as the apply kernel evaluates it in fp32: kl = sum * (1 / mb); > 2 desired: lr / 1.5 clamped
    below at lr_min; 0 < kl < desired / 2: lr * 1.5 clamped above at lr_max; otherwise unchanged.  Returns (lr, decision)"""
    f = np.float32
    kl = f(kl_sum) * (f(1.0) / f(mb_size))
    lr_old, d = f(lr_old), f(desired_kl)
    if kl > d * f(2.0):
        return np.maximum(f(lr_min), lr_old / f(1.5)), "down"
    if kl > f(0.0) and kl < d * f(0.5):
        return np.minimum(f(lr_max), lr_old * f(1.5)), "up"
    return lr_old, "keep"


def lr_rule64(kl_mean: float, lr_old: float, desired_kl: float, lr_min: float = 1e-5, lr_max: float = 1e-2) -> float:
    if kl_mean > desired_kl * 2.0:
        return max(lr_min, lr_old / 1.5)
    if 0.0 < kl_mean < desired_kl / 2.0:
        return min(lr_max, lr_old * 1.5)
    return lr_old


def clip_coef(grad, max_norm: float, norm2=None):
    """torch.nn.utils.clip_grad_norm_: coefficient max_norm / (||g|| + 1e-6), clamped at 1"""
    n2 = float((grad * grad).sum()) if norm2 is None else float(norm2)
    return min(1.0, max_norm / (math.sqrt(max(n2, 0.0)) + 1e-6))


def entropy_grad_std(std, entropy_coef: float):
    """d (-c_e * mean entropy) / d std: the Normal's entropy is sum_j (1/2 + log(2 pi)/2 + log std_j)"""
    return -entropy_coef / std


def adam(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64; returns (p, m, v, update magnitude): the last is
    lr / bc1 * m_abs / denom with m_abs = beta1 |m| + (1 - beta1) |g|, the scale of the update's rounding"""
    m_new = beta1 * m + (1.0 - beta1) * g
    v_new = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = v_new.sqrt() / math.sqrt(bc2) + eps
    step_size = lr / bc1
    upd = step_size * m_new / denom
    m_abs = beta1 * m.abs() + (1.0 - beta1) * g.abs()
    return p - upd, m_new, v_new, step_size * m_abs / denom


def apply_step(params, grad, m, v, step: int, lr: float, std_snapshot, norm2, *, entropy_coef=0.005, max_grad_norm=1.0,
               beta1=0.9, beta2=0.999, eps=1e-8):
    """the apply stage on a flat gradient row (parameters first, std the first two): entropy term on the std entries,
    norm clipping with the squared norm `norm2` of the row WITHOUT the entropy term (what the gradient kernels hand over;
    None: computed), Adam.  Returns (params, m, v, update magnitude)"""
    g = grad.clone()
    es = entropy_grad_std(std_snapshot.double(), entropy_coef)
    n2 = float((grad * grad).sum()) if norm2 is None else float(norm2)
    n2 += float(((grad[:2] + es) ** 2 - grad[:2] ** 2).sum())
    g[:2] += es
    coef = clip_coef(g, max_grad_norm, n2)
    return adam(params, g * coef, m, v, step, lr, beta1, beta2, eps)


# ---- GAE -------------------------------------------------------------------------------------------------------------------
def gae64(rewards, values, dones, gamma: float, lam: float):
    """rsl_rl RolloutStorage.compute_returns in float64, with the magnitude of each advantage (the recursion's absolute
    values): returns (returns, advantages, m_advantages, m_returns)"""
    K = rewards.shape[0]
    r, v = rewards.double(), values.double()
    nd = 1.0 - dones.double()
    adv = torch.zeros_like(r)
    madv = torch.zeros_like(r)
    last = torch.zeros_like(r[0])
    mlast = torch.zeros_like(r[0])
    for t in reversed(range(K)):
        delta = r[t] + nd[t] * gamma * v[t + 1] - v[t]
        mdelta = r[t].abs() + nd[t] * gamma * v[t + 1].abs() + v[t].abs()
        last = delta + nd[t] * gamma * lam * last
        mlast = mdelta + nd[t] * gamma * lam * mlast
        adv[t], madv[t] = last, mlast
    return adv + v[:-1], adv, madv, madv + v[:-1].abs()

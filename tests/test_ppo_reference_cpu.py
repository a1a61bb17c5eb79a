"""tests/ppo_reference.py (the float64 PPO step the GPU learner tests hold the kernels to) pinned to torch: float64 autograd
of the loss exactly as rl/ppo.py::PPO._step writes it, and PPO._step itself (clip_grad_norm_ + torch.optim.Adam + the
adaptive-KL rule) on a float64 copy of the nets over several steps.  Small problems, data away from branch ties."""
import copy

import numpy as np
import pytest
import torch

import ppo_reference as R


def _problem(B, D, activation, seed):
    from wheeledlab_amd.rl.ppo import ActorCritic
    torch.manual_seed(seed)
    ac = ActorCritic(D, D, 2, activation=activation).double()
    with torch.no_grad():
        ac.std.copy_(torch.tensor([0.8, 1.1]))
        for p in ac.parameters():
            if p.dim() == 2:
                p.mul_(1.5)
    g = torch.Generator().manual_seed(seed + 1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    obs = r(B, D)
    P = R.nets64(ac)
    fa = R.forward(P["actor"], obs, activation)
    fc = R.forward(P["critic"], obs, activation)
    mu = fa["y"]
    actions = mu + P["std"] * r(B, 2)
    logp = (-0.5 * ((actions - mu) / P["std"]) ** 2 - torch.log(P["std"]) - 0.5 * R.LOG_2PI).sum(1)
    b = dict(obs=obs, actions=actions, mu=mu + 0.05 * r(B, 2), logp=logp + 0.3 * r(B), adv=r(B), returns=r(B),
             values=fc["y"][:, 0] + 0.3 * r(B))
    return ac, b, torch.tensor([0.85, 1.05], dtype=torch.float64)


def _torch_loss(ac, b, sigma_old, clip=0.2, vcoef=1.0, clipped=True):
    """PPO._step's loss terms, line for line (no entropy)"""
    ac.update_distribution(b["obs"])
    logp = ac.get_actions_log_prob(b["actions"])
    value = ac.evaluate(b["obs"]).squeeze(-1)
    mu, sigma = ac.action_mean, ac.action_std
    kl = torch.sum(torch.log(sigma / sigma_old + 1e-5) + (sigma_old.square() + (b["mu"] - mu).square()) / (2.0 * sigma.square()) - 0.5, -1)
    adv = b["adv"]
    ratio = torch.exp(logp - b["logp"])
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    ret, v_old = b["returns"], b["values"]
    if clipped:
        v_clip = v_old + (value - v_old).clamp(-clip, clip)
        value_loss = torch.max((value - ret).square(), (v_clip - ret).square()).mean()
    else:
        value_loss = (ret - value).square().mean()
    return surrogate, vcoef * value_loss, value_loss, kl.mean()


def _away_from_ties(res, clip, activation):
    bands = R.branch_bands(res, clip, 1e-9, activation)
    assert not bool(bands["any"].any())


@pytest.mark.parametrize("activation", ["elu", "relu"])
@pytest.mark.parametrize("D,B,clipped,vcoef", [(14, 300, True, 1.0), (14, 97, False, 0.5), (80, 257, True, 2.0)])
def test_reference_gradients_equal_float64_autograd(activation, D, B, clipped, vcoef):
    ac, b, sigma_old = _problem(B, D, activation, seed=D + B)
    P = R.nets64(ac)
    res = R.minibatch_gradients(P, b, sigma_old, activation, clip=0.2, value_loss_coef=vcoef, use_clipped_value_loss=clipped)
    _away_from_ties(res, 0.2, activation)
    L = res["loss"]
    # the data reach every branch
    assert bool((~L["unclipped"]).any()) and bool(L["unclipped"].any())
    if clipped:
        assert bool(L["take2"].any()) and bool((L["take2"] & ~L["inside"]).any()) and bool((~L["take2"]).any())
    surrogate, vl, value_loss, kl = _torch_loss(ac, b, sigma_old, 0.2, vcoef, clipped)
    ac.zero_grad()
    (surrogate + vl).backward()
    want = torch.cat([p.grad.reshape(-1) for p in ac.parameters()])
    G = res["n_params"]
    assert G == want.numel()
    got = res["grad"]
    torch.testing.assert_close(got[:G], want, rtol=1e-11, atol=1e-13)
    B = b["adv"].shape[0]
    torch.testing.assert_close(got[G:] / B, torch.stack([value_loss, surrogate, kl]).detach(), rtol=1e-12, atol=1e-14)
    # the magnitude row bounds every element and statistic, and is no bound at all when it equals |g| everywhere
    mag = res["mag"]
    assert bool((mag >= got.abs() * (1 - 1e-12)).all())
    assert float((mag[:G] / got[:G].abs().clamp_min(1e-300)).median()) > 1.0


def test_magnitude_pass_bounds_an_fp32_evaluation():
    """the error model itself: the same step evaluated in fp32 (torch autograd on fp32 copies) stays inside
    n 2^-24 m(g) for a generous n -- and far inside: the bound is a worst case"""
    from wheeledlab_amd.rl.ppo import ActorCritic  # noqa: F401
    ac, b, sigma_old = _problem(2000, 14, "elu", seed=7)
    P = R.nets64(ac)
    b32 = {k: v.float() for k, v in b.items()}
    # inputs rounded to fp32 first: both sides start from the same numbers
    b64 = {k: v.double() for k, v in b32.items()}
    ac32 = copy.deepcopy(ac).float()
    P64 = R.nets64(ac32)
    res = R.minibatch_gradients(P64, b64, sigma_old.float().double(), "elu")
    surrogate, vl, _, _ = _torch_loss(ac32, b32, sigma_old.float())
    ac32.zero_grad()
    (surrogate + vl).backward()
    got = torch.cat([p.grad.reshape(-1) for p in ac32.parameters()]).double()
    G = res["n_params"]
    ratio = ((got - res["grad"][:G]).abs() / (4096 * R.U * res["mag"][:G] + 1e-30)).max()
    print("fp32 autograd err / (4096 u m):", float(ratio))
    assert float(ratio) < 1.0
    del P


@pytest.mark.parametrize("activation", ["elu", "relu"])
def test_reference_steps_equal_ppo_step(activation):
    """six PPO._step calls (entropy bonus, clip_grad_norm_, adaptive-KL learning rate with a desired KL that moves it both
    ways and keeps it once, torch.optim.Adam) on a float64 copy of the nets against the reference's apply stage: same learning rates, same
    parameters to float64 rounding"""
    from wheeledlab_amd.rl.ppo import PPO
    ac, b, sigma_old = _problem(400, 14, activation, seed=11)
    ac_t = copy.deepcopy(ac)
    ppo = PPO(ac_t, desired_kl=0.01, max_grad_norm=0.5, fused_update=False)
    assert not ppo._lr_on_device
    P = R.nets64(ac)
    p = R.flat_params(P)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lr = 1e-3
    decisions = set()
    for step in range(1, 7):
        bb = b
        res = R.minibatch_gradients(R.unflat_params(p, P), bb, sigma_old, activation)
        G = res["n_params"]
        kl_mean = float(res["grad"][G + 2]) / 400
        # the desired KL moves the rule through all three outcomes: down, up, up, keep, down, up
        ppo.desired_kl = kl_mean * [0.3, 3.0, 2.5, 1.0, 0.45, 2.2][step - 1]
        lr_new = R.lr_rule64(kl_mean, lr, ppo.desired_kl)
        decisions.add((lr_new > lr) - (lr_new < lr))
        lr = lr_new
        p, m, v, _ = R.apply_step(p, res["grad"][:G], m, v, step, lr, p[:2], None, entropy_coef=0.005, max_grad_norm=0.5)
        ppo._step(bb, sigma_old)
        assert abs(ppo.learning_rate - lr) <= 1e-6 * lr, (step, ppo.learning_rate, lr)   # PPO keeps the lr in an fp32 tensor
        got = torch.cat([q.detach().reshape(-1) for q in ac_t.parameters()])
        torch.testing.assert_close(got, p, rtol=0, atol=1e-6 * lr * step)
    assert decisions == {-1, 0, 1}


def test_apply_stage_pieces():
    """clip coefficient at / below / above the knee, the fp32 lr rule's thresholds and clamps"""
    g = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert R.clip_coef(g, 10.0) == 1.0
    assert abs(R.clip_coef(g, 5.0) - 5.0 / (5.0 + 1e-6)) < 1e-15
    assert abs(R.clip_coef(g, 1.0) - 1.0 / (5.0 + 1e-6)) < 1e-15
    f = np.float32
    d = f(0.01)
    assert R.lr_rule_f32(d * f(2), 1, 1e-3, d, 1e-5, 1e-2)[1] == "keep"
    assert R.lr_rule_f32(np.nextafter(d * f(2), f(1)), 1, 1e-3, d, 1e-5, 1e-2)[1] == "down"
    assert R.lr_rule_f32(d * f(0.5), 1, 1e-3, d, 1e-5, 1e-2)[1] == "keep"
    assert R.lr_rule_f32(np.nextafter(d * f(0.5), f(0)), 1, 1e-3, d, 1e-5, 1e-2)[1] == "up"
    assert R.lr_rule_f32(0.0, 1, 1e-3, d, 1e-5, 1e-2)[1] == "keep"
    assert R.lr_rule_f32(-1e-3, 1, 1e-3, d, 1e-5, 1e-2)[1] == "keep"
    assert R.lr_rule_f32(1.0, 1, 1e-5, d, 1e-5, 1e-2)[0] == f(1e-5)
    assert R.lr_rule_f32(1e-4, 1, 1e-2, d, 1e-5, 1e-2)[0] == f(1e-2)


def test_gae_reference_equals_the_torch_recursion():
    from wheeledlab_amd.policy import RolloutStorage
    K, n = 9, 33
    st = RolloutStorage(K, n, device="cpu")
    g = torch.Generator().manual_seed(3)
    st.rewards.copy_(torch.randn(K, n, generator=g))
    st.values.copy_(torch.randn(K + 1, n, generator=g))
    st.dones.copy_((torch.rand(K, n, generator=g) < 0.2).long())
    st.dones[0, :3] = 1
    st.dones[K - 1, 3:6] = 1
    ret, adv_n = st.compute_returns(0.99, 0.95)
    r64, a64, madv, _ = R.gae64(st.rewards, st.values, st.dones, 0.99, 0.95)
    torch.testing.assert_close(ret.double(), r64, rtol=0, atol=1e-5)
    assert bool((madv >= a64.abs()).all())

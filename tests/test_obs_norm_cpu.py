"""CPU checks of the empirical observation normalisation: the header and its ctypes mirror, every argument refusal before any
launch, the torch module against the float64 reference (tests/obs_norm_reference.py), the runner's order (collect -> merge ->
update -> fold) on the torch path, checkpoints, and the untouched default path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from tests import obs_norm_reference as R
from tests.test_ppo_cpu import CFG, _ToyEnv
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_obsnorm.h")
ON = dict(CFG, empirical_normalization=True)


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


# ---- the C boundary --------------------------------------------------------------------------------------------------

def test_obsnorm_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.OBSNORM_SIGNATURES)
    assert not declared & (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES) | set(A.RAYCASTER_SIGNATURES))
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_obsnorm_version() == 1 == A.WL_OBSNORM_VERSION


def test_obsnorm_constants_match_header_and_the_step_boundary_is_unchanged(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "wheeledlab_amd_obsnorm.h"\nint main(){printf("%d %d %d %d %d\\n", (int)WL_OBSNORM_VERSION, '
                     '(int)WL_OBSNORM_MAX_DIM, (int)WL_OBSNORM_MAX_ROWS, (int)WL_ABI_VERSION, (int)WL_ABI_REVISION); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [A.WL_OBSNORM_VERSION, A.OBSNORM_MAX_DIM, A.OBSNORM_MAX_ROWS, A.WL_ABI_VERSION, A.WL_ABI_REVISION] and got[3:] == [24, 1]


def test_obsnorm_refuses_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    fake = 1 << 20                 # never dereferenced: every call below returns before any launch
    acc = dict(rows=128, D=14, x=fake, stride=14, mean=fake, inv=fake, out=fake, scratch=fake, sums=fake)

    def accumulate(**kw):
        a = {**acc, **kw}
        return lib.wl_obsnorm_accumulate(a["rows"], a["D"], a["x"], a["stride"], a["mean"], a["inv"], a["out"], a["scratch"], a["sums"], None)
    for k in ("x", "mean", "inv", "scratch", "sums"):
        assert accumulate(**{k: None}) == -1, k
    for kw in (dict(rows=0), dict(rows=-1), dict(rows=A.OBSNORM_MAX_ROWS + 1), dict(D=0), dict(D=A.OBSNORM_MAX_DIM + 1), dict(stride=13)):
        assert accumulate(**kw) == -1, kw
    for k in ("x", "mean", "inv", "out"):
        assert accumulate(**{k: fake + 2}) == -3, k
    for k in ("scratch", "sums"):
        assert accumulate(**{k: fake + 4}) == -3, k
    assert lib.wl_obsnorm_scratch_bytes(0, 14, 14) == -1 and lib.wl_obsnorm_scratch_bytes(8, 14, 13) == -1
    # one [2][D] double partial per workgroup: at least one, and a multiple of that size
    for rows, D, stride in ((1, 14, 14), (4099, 14, 14), (2051, 689, 689), (130, 64, 80), (524288, 689, 689)):
        b = lib.wl_obsnorm_scratch_bytes(rows, D, stride)
        assert b >= 16 * D and b % (16 * D) == 0 and b <= 16 * D * 4096, (rows, D, b)

    upd = dict(D=14, sums=fake, m=128, until=10 ** 8, eps=1e-2, mean=fake, var=fake, std=fake, inv=fake, count=fake)

    def update(**kw):
        a = {**upd, **kw}
        return lib.wl_obsnorm_update(a["D"], a["sums"], a["m"], a["until"], a["eps"], a["mean"], a["var"], a["std"], a["inv"], a["count"], None)
    for k in ("sums", "mean", "var", "std", "inv", "count"):
        assert update(**{k: None}) == -1, k
    for kw in (dict(D=0), dict(m=0), dict(until=-1), dict(eps=0.0), dict(eps=float("inf")), dict(eps=float("nan"))):
        assert update(**kw) == -1, kw
    for k in ("sums", "count"):
        assert update(**{k: fake + 4}) == -3, k
    for k in ("mean", "var", "std", "inv"):
        assert update(**{k: fake + 2}) == -3, k

    fld = dict(D=14, H=64, w=fake, b=fake, mean=fake, inv=fake, wo=fake, bo=fake)

    def fold(**kw):
        a = {**fld, **kw}
        return lib.wl_obsnorm_fold(a["D"], a["H"], a["w"], a["b"], a["mean"], a["inv"], a["wo"], a["bo"], None)
    for k in ("w", "b", "mean", "inv", "wo", "bo"):
        assert fold(**{k: None}) == -1 and fold(**{k: fake + 1}) == -3, k
    for kw in (dict(D=0), dict(H=0), dict(H=65536)):
        assert fold(**kw) == -1, kw


# ---- the torch module ------------------------------------------------------------------------------------------------

def _module(D, **kw):
    from wheeledlab_amd.rl.normalizer import EmpiricalNormalization
    return EmpiricalNormalization(D, **kw)


def test_state_dict_has_rsl_rl_keys_shapes_and_initial_values():
    sd = _module(14).state_dict()
    assert list(sd) == ["_mean", "_var", "_std", "count"]
    assert sd["_mean"].shape == sd["_var"].shape == sd["_std"].shape == (1, 14) and sd["count"].shape == () and sd["count"].dtype == torch.int64
    assert all(sd[k].dtype == torch.float32 for k in ("_mean", "_var", "_std"))
    assert (sd["_mean"] == 0).all() and (sd["_var"] == 1).all() and (sd["_std"] == 1).all() and int(sd["count"]) == 0
    m = _module(14)
    assert m.eps == 1e-2 and m.until == 10 ** 8


@pytest.mark.parametrize("D", [14, 689])
def test_update_and_output_equal_the_reference(D):
    nz = _module(D)
    x, _, _ = R.inputs(96, D, seed=D)
    y, _, _ = R.inputs(200, D, seed=D)        # same columns, more rows: the second (warm) merge
    y = y[96:]
    mean, var, count = R.cold(D)
    for batch in (x, y):
        mean32, var32 = nz._mean.numpy()[0].copy(), nz._var.numpy()[0].copy()
        out = nz(torch.from_numpy(batch))                         # training mode: update, then normalise with the new statistics
        mean, var, count = R.update(mean32, var32, count, batch)
        std, inv = R.derived(var)
        for got, want in ((nz._mean, mean), (nz._var, var), (nz._std, std), (nz._inv_std, inv)):
            ok, worst = R.within_ulps(got.numpy()[0], want, 2)
            assert ok, worst
        assert int(nz.count) == count
        want = (R.f64(batch) - R.f64(nz._mean.numpy())) / (R.f64(nz._std.numpy()) + 1e-2)
        ok, worst = R.within_ulps(out.numpy(), want, 4)           # fp32: difference, sum, quotient
        assert ok, worst


def test_sequential_updates_equal_one_pooled_update():
    D, K, n = 14, 8, 96
    x, _, _ = R.inputs(K * n, D, seed=2)
    a, b = _module(D), _module(D)
    for k in range(K):
        a.update(torch.from_numpy(x[k * n:(k + 1) * n]))
    b.update(torch.from_numpy(x))
    assert int(a.count) == int(b.count) == K * n
    for k in ("_mean", "_var", "_std"):
        rel = (getattr(a, k) - getattr(b, k)).abs() / getattr(b, k).abs().clamp_min(1e-30)
        assert float(rel.max()) <= 1e-6, (k, float(rel.max()))
    mean, var, _ = R.sequential(*R.cold(D), x.reshape(K, n, D))
    for k, want in (("_mean", mean), ("_var", var)):
        got = getattr(a, k).double().numpy()[0]
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), (k, float((np.abs(got - want) / np.abs(want)).max()))


def test_until_stops_the_updates_and_eval_freezes_the_statistics():
    x = torch.from_numpy(R.inputs(64, 5, seed=1)[0])
    nz = _module(5, until=100)
    nz(x)
    nz(x)                                             # 64 < 100 before it: merged whole
    assert int(nz.count) == 128
    before = {k: v.clone() for k, v in nz.state_dict().items()}
    nz(x + 3.0)                                       # 128 >= 100: skipped
    assert all(torch.equal(v, before[k]) for k, v in nz.state_dict().items())
    ev = _module(5)
    ev(x)
    before = {k: v.clone() for k, v in ev.state_dict().items()}
    ev.eval()
    y = ev(x + 3.0)
    assert all(torch.equal(v, before[k]) for k, v in ev.state_dict().items())
    assert torch.equal(y, (x + 3.0 - ev._mean) / (ev._std + 1e-2))


def test_cpu_fold_is_the_reference_fold():
    from wheeledlab_amd.rl.ppo import ActorCritic
    D = 14
    ac, nz = ActorCritic(D, D, 2), _module(D)
    nz.update(torch.from_numpy(R.inputs(256, D, seed=4)[0]))
    view = nz.fold(ac)
    assert view is ac.fused() is ac.folded_view() and view is not ac.param_view()
    for m, seq in ((view.actor, ac.actor), (view.critic, ac.critic)):
        wf, bf, babs = R.fold(seq[0].weight.detach().numpy(), seq[0].bias.detach().numpy(), nz._mean.numpy()[0], nz._inv_std.numpy()[0])
        assert R.within_ulps(m.w1.numpy(), wf, 1)[0] and R.within_ulps(m.b1.numpy(), bf, 1, extra=2.0 ** -40 * babs)[0]
        assert m.w1.data_ptr() != seq[0].weight.data_ptr() and m.w2.data_ptr() == seq[2].weight.data_ptr()      # only layer 1 is its own
    p = view.actor.w1.data_ptr()
    nz.update(torch.from_numpy(R.inputs(256, D, seed=5)[0]))
    old = view.actor.w1.clone()
    assert nz.fold(ac).actor.w1.data_ptr() == p and not torch.equal(old, view.actor.w1)       # the same tensors, new values


def test_the_reference_restates_the_folding_limit():
    """DESIGN.md's table: folding costs up to ~1e-4 where a column has |mean| inv_std ~ 1000; normalising first stays at ~1e-5"""
    for D in (14, 689):
        fold_err, first_err, ratio = R.folding_probe(D)
        assert 50.0 < ratio <= 100.0 * 1000.0 and fold_err < 1e-3 and first_err < 1e-4, (D, fold_err, first_err, ratio)


# ---- the runner on the torch path ------------------------------------------------------------------------------------

def test_learner_on_a_normalised_storage_keeps_parameters_finite_and_statistics_untouched():
    from wheeledlab_amd.policy import RolloutStorage
    from wheeledlab_amd.rl.ppo import PPO, ActorCritic
    torch.manual_seed(3)
    K, n, D = 4, 64, 6
    ac, nz = ActorCritic(D, D, 2), _module(D)
    st = RolloutStorage(K, n, obs_dim=D, device="cpu")
    raw = torch.from_numpy(R.inputs((K + 1) * n, D, seed=8)[0]).view(K + 1, n, D)
    st.observations.copy_(raw)
    with torch.no_grad():
        ac.update_distribution(nz.normalize(raw[:K].reshape(K * n, D)))
        a = ac.distribution.sample()
        st.actions.copy_(a.view(K, n, 2))
        st.mu.copy_(ac.action_mean.view(K, n, 2))
        st.actions_log_prob.copy_(ac.get_actions_log_prob(a).view(K, n))
        st.values.copy_(ac.evaluate(nz.normalize(raw.reshape(-1, D))).view(K + 1, n))
    st.rewards.normal_()
    ratio = nz.merge_rollout(st, 1)
    assert int(nz.count) == K * n and ratio == nz.max_ratio()
    assert torch.equal(st.observations[K], raw[K])                                        # row K stays raw
    want = (raw[:K] - 0.0) / (1.0 + 1e-2)                                                 # normalised with the FROZEN (cold) statistics
    assert torch.allclose(st.observations[:K], want, rtol=1e-6, atol=0)
    mean, var, _ = R.update(*R.cold(D), raw[:K].reshape(K * n, D).numpy())
    assert R.within_ulps(nz._mean.numpy()[0], mean, 2)[0] and R.within_ulps(nz._var.numpy()[0], var, 2)[0]
    before = {k: v.clone() for k, v in nz.state_dict().items()}
    PPO(ac).update(st)
    assert all(torch.isfinite(p).all() for p in ac.parameters())
    assert all(torch.equal(v, before[k]) for k, v in nz.state_dict().items())


def test_runner_with_the_switch_on_learns_counts_and_checkpoints_round_trip(tmp_path):
    torch.manual_seed(0)
    runner = _runner(ON, log_dir=str(tmp_path))
    assert runner.obs_normalizer is not None and not runner._folds             # CPU: torch normalises, nothing is folded
    hist = runner.learn(30, verbose=False)
    K, n = 8, 512
    assert int(runner.obs_normalizer.count) == 30 * K * n                      # rows 0 .. K - 1 of every rollout, row K never twice
    assert hist[-1]["mean_step_reward"] > hist[0]["mean_step_reward"] + 1.0 and "obs_norm_max_ratio" in hist[-1]
    assert float((runner.obs_normalizer._mean.abs()).max()) < 0.05 and float((runner.obs_normalizer._std - 1).abs().max()) < 0.05
    path = os.path.join(str(tmp_path), "models", "model_29.pt")
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "obs_norm_state_dict", "critic_obs_norm_state_dict"}
    assert list(ck["obs_norm_state_dict"]) == ["_mean", "_var", "_std", "count"] == list(ck["critic_obs_norm_state_dict"])
    other = _runner(ON, seed=1)
    other.load(path)
    for k, v in runner.obs_normalizer.state_dict().items():
        assert torch.equal(other.obs_normalizer.state_dict()[k], v)
    assert torch.equal(other.obs_normalizer._inv_std, runner.obs_normalizer._inv_std)
    x = torch.randn(16, 4) * 3 + 1
    y = runner.get_inference_policy()(x)
    assert torch.equal(other.get_inference_policy()(x), y)
    assert torch.equal(y, runner.actor_critic.act_inference(runner.obs_normalizer.normalize(x)))     # normalised, in eval mode
    assert not runner.obs_normalizer.training and int(runner.obs_normalizer.count) == 30 * K * n


def _runner(cfg, seed=0, log_dir=None):
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    return OnPolicyRunner(_ToyEnv(seed=seed), cfg, log_dir=log_dir, device="cpu")


def test_checkpoints_of_the_other_kind_are_refused(tmp_path):
    on, off = _runner(ON), _runner(CFG)
    on.save(os.path.join(str(tmp_path), "on.pt"))
    off.save(os.path.join(str(tmp_path), "off.pt"))
    with pytest.raises(ValueError, match="empirical_normalization"):
        off.load(os.path.join(str(tmp_path), "on.pt"))
    with pytest.raises(ValueError, match="empirical_normalization"):
        on.load(os.path.join(str(tmp_path), "off.pt"))


def test_default_path_builds_no_normaliser_and_writes_no_new_keys(tmp_path):
    for cfg in (CFG, dict(CFG, empirical_normalization=False)):
        runner = _runner(cfg, log_dir=str(tmp_path))
        assert runner.obs_normalizer is None and not runner._folds
        hist = runner.learn(1, verbose=False)
        assert "obs_norm_max_ratio" not in hist[0]
        assert runner.actor_critic._folded is None and runner.actor_critic.fused is not None
        ck = torch.load(os.path.join(str(tmp_path), "models", "model_0.pt"), weights_only=False)
        assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    for task in ("Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0"):
        assert registry.load_cfg_from_registry(task, "rsl_rl_cfg_entry_point").empirical_normalization is False


def test_until_reaches_the_runner():
    runner = _runner(dict(ON, empirical_normalization_until=5000))
    runner.learn(3, verbose=False)                   # 4096 rows per iteration: the second merge starts below 5000, the third does not
    assert int(runner.obs_normalizer.count) == 8192

"""GPU: the observation normaliser's kernels (csrc/wl_obs_norm.hip) against the float64 reference (tests/obs_norm_reference.py) at
derived bars, the policy step through folded first layers against float64 normalise-then-MLP at the policy step's own bars
(tests/test_gpu_actor_act.py), and the runner end to end with the switch on (fused drift collector, persistent elevation collector,
checkpoints)."""
import numpy as np
import pytest
import torch

from tests import obs_norm_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 64


def _module(D, mean=None, var=None, count=0, **kw):
    from wheeledlab_amd.rl.normalizer import EmpiricalNormalization
    nz = EmpiricalNormalization(D, **kw).to(DEV)
    if mean is not None:
        nz._mean.copy_(torch.from_numpy(np.asarray(mean, np.float32))[None])
        nz._var.copy_(torch.from_numpy(np.asarray(var, np.float32))[None])
        nz._derive()
        nz.count.fill_(count)
    return nz


def _case(rows, D, stride, warm, seed):
    x, _, _ = R.inputs(rows, D, seed)
    mean0, var0, count0 = R.state(D, seed, warm)
    rng = np.random.default_rng(seed + 7)
    w1 = (rng.uniform(-1, 1, (H, D)) / np.sqrt(D)).astype(np.float32)
    b1 = (rng.uniform(-1, 1, H) / np.sqrt(D)).astype(np.float32)
    wide = rng.normal(size=(rows, stride or D)).astype(np.float32)
    wide[:, :D] = x
    return x, torch.from_numpy(wide).to(DEV), mean0, var0, count0, w1, b1


def _update(nz, sums, m):
    from wheeledlab_amd import _abi as A
    A.check(A.load().wl_obsnorm_update(nz.dim, sums.data_ptr(), m, nz.until, nz.eps, nz._mean.data_ptr(), nz._var.data_ptr(), nz._std.data_ptr(),
                                       nz._inv_std.data_ptr(), nz.count.data_ptr(), None), "wl_obsnorm_update")


def _fold(nz, w1, b1):
    import ctypes as C

    from wheeledlab_amd import _abi as A
    w, b = torch.from_numpy(w1).to(DEV), torch.from_numpy(b1).to(DEV)
    wo, bo = torch.full_like(w, float("nan")), torch.full_like(b, float("nan"))
    A.check(A.load().wl_obsnorm_fold(nz.dim, w.shape[0], w.data_ptr(), b.data_ptr(), nz._mean.data_ptr(), nz._inv_std.data_ptr(), wo.data_ptr(),
                                     bo.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "wl_obsnorm_fold")
    return wo.cpu().numpy(), bo.cpu().numpy()


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("rows,D,stride", R.SHAPES, ids=[f"{r}x{d}" + (f"s{s}" if s else "") for r, d, s in R.SHAPES])
def test_accumulate_update_and_fold_match_the_reference(rows, D, stride, warm):
    x, buf, mean0, var0, count0, w1, b1 = _case(rows, D, stride, warm, seed=100 + rows + D)
    nz = _module(D, mean0, var0, count0)
    view = buf[:, :D]                                              # a strided view when stride is set
    pad = buf[:, D:].clone()
    out = torch.full_like(buf, float("nan"))[:, :D]
    sums = nz._accumulate(view, out)
    again = nz._accumulate(view, None)                             # no output: the same sums, byte for byte
    inplace_buf = buf.clone()
    sums_inplace = nz._accumulate(inplace_buf[:, :D], inplace_buf[:, :D])
    torch.cuda.synchronize()
    assert sums.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() == sums_inplace.cpu().numpy().tobytes()
    assert out.cpu().numpy().tobytes() == inplace_buf[:, :D].cpu().numpy().tobytes()          # in place equals out of place
    assert torch.equal(buf[:, :D].cpu(), torch.from_numpy(x)) and torch.equal(inplace_buf[:, D:], pad)     # input and padding untouched
    out2 = torch.full_like(buf, float("nan"))[:, :D]
    assert nz._accumulate(view, out2).cpu().numpy().tobytes() == sums.cpu().numpy().tobytes() and out2.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    _update(nz, sums, rows)
    w1o, b1o = _fold(nz, w1, b1)
    torch.cuda.synchronize()
    got = dict(sums=sums.cpu().numpy(), mean=nz._mean.cpu().numpy()[0], var=nz._var.cpu().numpy()[0], std=nz._std.cpu().numpy()[0],
               inv_std=nz._inv_std.cpu().numpy()[0], count=int(nz.count), out=out.cpu().numpy(), w1_out=w1o, b1_out=b1o)
    R.check(got, x, mean0, var0, count0, w1, b1, label=f"gpu {rows}x{D}{'s' + str(stride) if stride else ''} {'warm' if warm else 'cold'}")


def test_until_stops_the_update_and_leaves_the_bits():
    x, buf, mean0, var0, count0, _, _ = _case(130, 14, None, True, seed=5)
    nz = _module(14, mean0, var0, count0, until=count0)
    before = {k: v.clone() for k, v in nz.state_dict().items()}
    inv = nz._inv_std.clone()
    sums = nz._accumulate(buf, None)
    _update(nz, sums, 130)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in nz.state_dict().items()) and torch.equal(inv, nz._inv_std)
    nz.until = count0 + 1                                          # below `until` before the batch: merged whole
    _update(nz, sums, 130)
    assert int(nz.count) == count0 + 130 and not torch.equal(nz._mean, before["_mean"])


@pytest.mark.parametrize("D", [14, 689])
def test_merge_rollout_equals_sequential_updates(D):
    """after merge_rollout on a [K = 8, n = 96, D] storage the statistics are the reference's K SEQUENTIAL float64 updates, and its one
    pooled update, each at 2 ulp of fp32 and 1e-6 relative per element (the merge is associative: the two float64 results differ by
    ~1e-13); rows 0 .. K - 1 are normalised in place, row K stays raw"""
    from wheeledlab_amd.policy import RolloutStorage
    K, n = 8, 96
    x, _, _ = R.inputs((K + 1) * n, D, seed=D + 1)
    mean0, var0, count0 = R.state(D, D + 1, warm=True)
    nz = _module(D, mean0, var0, count0)
    inv0 = nz._inv_std.cpu().numpy()[0]
    st = RolloutStorage(K, n, D, 2, DEV)
    st.observations.copy_(torch.from_numpy(x).view(K + 1, n, D))
    ratio = nz.merge_rollout(st, 1)
    torch.cuda.synchronize()
    rows = x[:K * n]
    pooled = R.update(mean0, var0, count0, rows)
    seq = R.sequential(mean0, var0, count0, rows.reshape(K, n, D))
    for name, (mean, var, count) in (("sequential", seq), ("pooled", pooled)):
        for k, want in (("_mean", mean), ("_var", var), ("_std", R.derived(var)[0])):
            got = getattr(nz, k).double().cpu().numpy()[0]
            ok, worst = R.within_ulps(got, want, 2)
            rel = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
            print(f"[merge_rollout D={D} {name} {k}] {worst:.3g} ulp, {rel:.3g} relative", flush=True)
            assert ok and rel <= 1e-6, (name, k, worst, rel)
        assert int(nz.count) == count == count0 + K * n
    got_mean = nz._mean.double().cpu().numpy()[0]
    ok, worst = R.within_ulps(st.observations[:K].cpu().numpy().reshape(K * n, D), R.normalise(rows, mean0, inv0), 4)
    assert ok, worst
    assert torch.equal(st.observations[K].cpu(), torch.from_numpy(x[K * n:]))
    assert ratio == pytest.approx(float(np.abs(got_mean * nz._inv_std.double().cpu().numpy()[0]).max()), rel=1e-6)


# ---- the policy step through folded first layers --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["f32", "bf16-one", "bf16-two"])
@pytest.mark.parametrize("D,n", [(689, 96), (3208, 64), (14, 96)])
def test_folded_policy_step_on_raw_observations_equals_normalise_then_mlp(D, n, form):
    """wl_actor_critic_act / _planes with the folded view on RAW observations against float64 normalise -> MLP (unfolded fp32
    parameters, the same fp32 statistics) at the policy step's own bars (tests/test_gpu_actor_act.py: 3e-4 on mu and values, 1e-3 on
    the log-prob), in every form.  Inputs with |mean| inv_std <= 8, where the folding's own error (at most 3e-5: DESIGN.md) stays an
    order below the bar.  Measured on MI355X: f32 form <= 1.7e-6 (mu / value) and 4e-6 (log-prob), both bf16 forms <= 1.1e-5 and 2.3e-5."""
    from wheeledlab_amd._abi import WlError
    from wheeledlab_amd.rl.ppo import ActorCritic
    torch.manual_seed(D + n)
    rng = np.random.default_rng(D)
    sg = np.exp(rng.normal(0.0, 1.0, D))
    mean = rng.uniform(-8.0, 8.0, D) * sg
    nz = _module(D, mean, sg * sg, 1000)
    assert nz.max_ratio() <= 8.0
    ac = ActorCritic(D, D, 2).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.tensor([0.7, 1.3]))
    view = nz.fold(ac)
    assert view is ac.fused()
    obs = torch.from_numpy((mean + sg * rng.normal(size=(n, D))).astype(np.float32)).to(DEV)
    a, mu = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
    logp, val = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    view.planes, view.planes_two_launch = form != "f32", form == "bf16-two"
    if D < 64 and form != "f32":          # the bf16 forms exist from D = 64 on: the library refuses, nothing falls back
        with pytest.raises(WlError):
            view.act(obs, a, mu, logp, val, 42, 7)
        return
    view.act(obs, a, mu, logp, val, 42, 7)
    torch.cuda.synchronize()
    layers = lambda seq: [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in seq if isinstance(m, torch.nn.Linear)]
    m32, i32 = nz._mean.cpu().numpy()[0], nz._inv_std.cpu().numpy()[0]
    want_mu = R.normalise_then_mlp(obs.cpu().numpy(), m32, i32, layers(ac.actor))
    want_val = R.normalise_then_mlp(obs.cpu().numpy(), m32, i32, layers(ac.critic))[:, 0]
    want_logp = R.log_prob(a.cpu().numpy(), want_mu, ac.std.detach().cpu().numpy())
    e_mu, e_val = np.abs(mu.cpu().numpy() - want_mu).max(), np.abs(val.cpu().numpy() - want_val).max()
    e_logp = np.abs(logp.cpu().numpy() - want_logp).max()
    print(f"[folded act D={D} n={n} {form}] mu {e_mu:.3g} value {e_val:.3g} logp {e_logp:.3g}", flush=True)
    assert e_mu <= 3e-4 and e_val <= 3e-4 and e_logp <= 1e-3, (e_mu, e_val, e_logp)


# ---- end to end -------------------------------------------------------------------------------------------------------

def _env(task, n, seed=42):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    cfg = registry.parse_env_cfg(task, device=DEV, num_envs=n)
    cfg.seed = seed
    env = registry.make(task, cfg=cfg)
    env.action_space.low, env.action_space.high = -1.0, 1.0
    return RslRlVecEnvWrapper(ClipAction(env))


def _agent(task, K):
    from wheeledlab_amd import registry
    cfg = registry.load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    cfg.num_steps_per_env, cfg.empirical_normalization = K, True
    return cfg


def _run_and_check(runner, iterations):
    """runner.learn with a look at every iteration between the merge and the first minibatch: the storage (normalised in place)
    must reproduce its own stored log-probs through the UNFOLDED torch ActorCritic, and row 0's stored log-prob must be that of
    float64 normalise -> actor on the RAW row 0 with the statistics the collection ran with.  Both at 1e-3."""
    nz, ac, st = runner.obs_normalizer, runner.actor_critic, runner.storage
    K, n, D = st.n_steps, st.n_envs, nz.dim
    raw0, frozen, seen, update, merge = [], [], [], runner.alg.update, nz.merge_rollout

    def before_merge(storage, world):        # the storage is still raw here, and the statistics are the ones the collection ran with
        raw0.append(storage.observations[0].clone())
        frozen.append((nz._mean.cpu().numpy()[0].copy(), nz._inv_std.cpu().numpy()[0].copy()))
        return merge(storage, world)

    def spy(storage, *a, **kw):
        with torch.no_grad():
            ac.update_distribution(storage.observations[:K].reshape(K * n, D))
            lp = ac.get_actions_log_prob(storage.actions.reshape(K * n, 2)).reshape(K, n)
            e_torch = float((lp - storage.actions_log_prob).abs().max())
        layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in ac.actor if isinstance(m, torch.nn.Linear)]
        mean, inv = frozen[-1]
        mu = R.normalise_then_mlp(raw0[-1].cpu().numpy(), mean, inv, layers, elu=ac.activation == "elu")
        want = R.log_prob(storage.actions[0].cpu().numpy(), mu, ac.std.detach().cpu().numpy())
        e_ref = float(np.abs(storage.actions_log_prob[0].cpu().numpy() - want).max())
        e_mu = float(np.abs(storage.mu[0].cpu().numpy() - mu).max())
        seen.append((e_torch, e_ref, e_mu))
        return update(storage, *a, **kw)
    runner.alg.update, nz.merge_rollout = spy, before_merge
    hist = runner.learn(iterations, verbose=False)
    print("[obs_norm end to end] per iteration (torch on the normalised storage, float64 on raw row 0: log-prob, mu):", seen, flush=True)
    assert len(seen) == iterations and int(nz.count) == iterations * K * n
    assert all(torch.isfinite(p).all() for p in ac.parameters()) and all(np.isfinite(h["value_function"]) for h in hist)
    assert all("obs_norm_max_ratio" in h for h in hist)
    for e_torch, e_ref, _ in seen:
        assert e_torch <= 1e-3 and e_ref <= 1e-3, seen
    return hist


def test_drift_runner_with_the_switch_on_stays_on_the_fused_collector(tmp_path):
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    task, n, K = "Isaac-MushrDriftRL-v0", 256, 16
    torch.manual_seed(0)
    runner = OnPolicyRunner(_env(task, n), _agent(task, K), log_dir=str(tmp_path), device=DEV)
    assert runner.fused and runner._folds and runner.actor_critic.fused() is runner.actor_critic.folded_view()
    _run_and_check(runner, 2)
    assert runner.collection_paths == ["fused", "fused"] and int(runner.obs_normalizer.count) == 2 * 16 * 256
    # the learner updated the parameters themselves, never the folded copies
    assert runner.alg._fused is not None and runner.alg._fused.view is runner.actor_critic.param_view()
    # checkpoint -> a fresh runner: the same next action means, byte for byte
    path = str(tmp_path / "models" / "model_1.pt")
    other = OnPolicyRunner(_env(task, n), _agent(task, K), device=DEV)
    other.load(path)
    obs = runner.storage.observations[K].clone()
    outs = []
    for r in (runner, other):
        v = r.actor_critic.fused()
        a, mu = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
        logp, val = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        v.act(obs, a, mu, logp, val, 1, 2, deterministic=True)
        outs.append((mu, val, r.get_inference_policy()(obs)))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert torch.equal(runner.actor_critic.fused().actor.w1, other.actor_critic.fused().actor.w1)
    # and the torch inference policy (normalise in eval mode, then the actor) agrees with the folded kernel step
    torch.testing.assert_close(outs[0][2], outs[0][0], rtol=0, atol=3e-4)
    off = OnPolicyRunner(_env(task, n), dict(_agent(task, K).to_dict(), empirical_normalization=False), device=DEV)
    with pytest.raises(ValueError, match="empirical_normalization"):
        off.load(path)


def test_elevation_runner_with_the_switch_on_takes_the_persistent_collector():
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    task, n, K = "Isaac-MushrElevationRL-v0", 64, 8
    torch.manual_seed(0)
    env = _env(task, n)
    base = env.unwrapped
    assert base.can_collect_rollout()
    launches, collect = [], base._batch.collect_rollout
    base._batch.collect_rollout = lambda view, *a, **k: (launches.append(view), collect(view, *a, **k))[1]
    runner = OnPolicyRunner(env, _agent(task, K), device=DEV)
    assert not runner.fused and runner.kernel_policy and runner._folds
    _run_and_check(runner, 1)
    assert len(launches) >= 1 and all(v is runner.actor_critic.folded_view() for v in launches)     # the collector launch, folded view
    assert runner.collection_paths == ["stepwise"] and int(runner.obs_normalizer.count) == K * n

"""TEST INFRASTRUCTURE ONLY: the float64 reference of the empirical observation normaliser (wheeledlab_amd/rl/normalizer.py,
csrc/wl_obs_norm.hip), in numpy.

The update is rsl_rl.modules.EmpiricalNormalization's (2.x), restated from memory (rsl-rl-lib is not vendored; parity with rsl_rl itself is unpinned):
state mean 0 / var 1 / std 1 / count 0, eps 1e-2, output (x - mean) / (std + eps); a batch of m rows with mean mb and biased variance
vb merges as count += m, rate = m / count, d = mb - mean, mean += rate d, var += rate (vb - var + d (mb - mean_new)), std = sqrt(var),
and not at all once count >= until.  Everything here computes in float64 from whatever the caller hands in (the tests hand in the same
fp32 inputs and the same fp32 state the code under test sees)."""
import numpy as np

EPS = 1e-2
UNTIL = 10 ** 8


def f64(a):
    return np.asarray(a, dtype=np.float64)


def cold(D):
    """(mean, var, count) before any batch"""
    return np.zeros(D), np.ones(D), 0


def update(mean, var, count, x, until=UNTIL):
    """one update with the rows of x [m, D]; returns (mean, var, count)"""
    if count >= until:
        return f64(mean), f64(var), count
    x = f64(x)
    m = x.shape[0]
    count = count + m
    rate = m / count
    mb, vb = x.mean(0), x.var(0)
    d = mb - f64(mean)
    mean_new = f64(mean) + rate * d
    var_new = f64(var) + rate * (vb - f64(var) + d * (mb - mean_new))
    return mean_new, var_new, count


def sequential(mean, var, count, xs, until=UNTIL):
    """K updates, one per xs[k] [n, D] -- what rsl_rl does step by step"""
    for x in xs:
        mean, var, count = update(mean, var, count, x, until)
    return mean, var, count


def derived(var, eps=EPS):
    """(std, inv_std) of a variance"""
    std = np.sqrt(f64(var))
    return std, 1.0 / (std + eps)


def sums(x, mean):
    """what wl_obsnorm_accumulate sums: S1 = sum (x - mean), S2 = sum (x - mean)^2, and the scales of their error bars
    sum |x - mean| and S2 itself"""
    d = f64(x) - f64(mean)
    return d.sum(0), (d * d).sum(0), np.abs(d).sum(0)


def normalise(x, mean, inv_std):
    return (f64(x) - f64(mean)) * f64(inv_std)


def act(x, elu=True):
    x = f64(x)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))) if elu else np.maximum(x, 0.0)


def mlp(x, layers, elu=True):
    """layers: [(W [out, in], b [out])] x 3, nn.Linear's layout"""
    h = f64(x)
    for i, (w, b) in enumerate(layers):
        h = h @ f64(w).T + f64(b)
        if i + 1 < len(layers):
            h = act(h, elu)
    return h


def normalise_then_mlp(x, mean, inv_std, layers, elu=True):
    return mlp(normalise(x, mean, inv_std), layers, elu)


def fold(w1, b1, mean, inv_std):
    """(W', b', sum_c |W mean inv_std|): W' x + b' = W ((x - mean) inv_std) + b"""
    t = f64(w1) * (f64(mean) * f64(inv_std))[None, :]
    return f64(w1) * f64(inv_std)[None, :], f64(b1) - t.sum(1), np.abs(t).sum(1)


def log_prob(actions, mu, std):
    a, mu, std = f64(actions), f64(mu), f64(std)
    return (-0.5 * ((a - mu) / std) ** 2 - np.log(std) - 0.5 * np.log(2.0 * np.pi)).sum(-1)


def ulp32(v):
    """the spacing of fp32 at |v| (at least the smallest normal's)"""
    return np.spacing(np.maximum(np.abs(f64(v)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def within_ulps(got, want, ulps, extra=0.0):
    """|got - want| <= ulps * ulp32(want) + extra, elementwise -> (ok, worst error in ulps)"""
    err = np.abs(f64(got) - f64(want))
    return bool((err <= ulps * ulp32(want) + extra).all()), float((np.maximum(err - extra, 0.0) / ulp32(want)).max())


# rows x D (x row stride) of the accumulate tests: fewer rows than one narrow wave-load holds, exactly one load and one over, several
# ragged chunks, one column, the boundary between the two forms, odd unaligned rows over several chunks and strips, a wide agent,
# and a strided view (which takes the wide form)
SHAPES = [(1, 14, None), (3, 14, None), (4, 14, None), (5, 14, None), (4099, 14, None), (257, 1, None), (130, 63, None), (130, 64, None),
          (130, 65, None), (2051, 689, None), (67, 3208, None), (130, 64, 80)]


def columns(D, seed):
    """per-column (mu, sigma): mu ~ N(0, 3), sigma log-normal; with D >= 2 column 0 is constant (sigma = 0), with D >= 3 column 1 has
    mu = 1000 sigma"""
    rng = np.random.default_rng(seed)
    mu, sg = rng.normal(0.0, 3.0, D), np.exp(rng.normal(0.0, 1.0, D))
    if D >= 2:
        sg[0] = 0.0
    if D >= 3:
        mu[1] = 1000.0 * sg[1]
    return mu, sg


def draw(rows, mu, sg, seed):
    """x = fl32(mu + sigma z) [rows, D]"""
    return (mu + sg * np.random.default_rng(seed).normal(size=(rows, len(mu)))).astype(np.float32)


def inputs(rows, D, seed):
    """-> (x fp32 [rows, D], mu, sigma)"""
    mu, sg = columns(D, seed)
    return draw(rows, mu, sg, seed + 1), mu, sg


def state(D, seed, warm):
    """the fp32 state a test starts from: cold (0, 1, count 0), or warmed by a previous batch of 512 rows of the same columns
    -> (mean f32, var f32, count)"""
    if not warm:
        return np.zeros(D, np.float32), np.ones(D, np.float32), 0
    mu, sg = columns(D, seed)
    mean, var, count = update(*cold(D), draw(512, mu, sg, seed + 2))
    return mean.astype(np.float32), var.astype(np.float32), count


def folding_probe(D=689, rows=64, seed=0):
    """the known numerical limit of the folding: max |W' x + b' - reference| in fp32 arithmetic, next to normalising first in fp32.
    Returns (fold error, normalise-first error, max |mean| inv_std)"""
    rng = np.random.default_rng(seed)
    x, _, _ = inputs(rows * 4, D, seed)
    mean, var, _ = update(*cold(D), x)
    _, inv = derived(var)
    w = rng.uniform(-1, 1, (64, D)) / np.sqrt(D)
    b = rng.uniform(-1, 1, 64) / np.sqrt(D)
    ref = normalise(x[:rows], mean, inv) @ w.T + b
    wf, bf, _ = fold(w, b, mean, inv)
    got = x[:rows] @ wf.astype(np.float32).T + bf.astype(np.float32)
    xn = (x[:rows] - mean.astype(np.float32)) * inv.astype(np.float32)
    got2 = xn @ w.astype(np.float32).T + b.astype(np.float32)
    return float(np.abs(got - ref).max()), float(np.abs(got2 - ref).max()), float(np.abs(mean * inv).max())


def inv_std32(var32, eps=EPS):
    """the fp32 inv_std that belongs to an fp32 variance: 1 / (sqrt(var) + eps) in float64, rounded once"""
    return derived(var32, eps)[1].astype(np.float32)


def check(got, x, mean0, var0, count0, w1, b1, until=UNTIL, eps=EPS, label=""):
    """hold one accumulate + update + fold (`got`: sums f64 [2, D]; mean, var, std, inv_std f32 [D]; count; out f32 like x; w1_out,
    b1_out) against float64 from the same fp32 inputs x [rows, D], state (mean0, var0 fp32, count0) and first layer (w1, b1 fp32).
    Bars (derived, not fitted):
      sums      1e-12 relative to sum |x - mean| (S1) and to S2: float64 sums of at most 2^23 terms in another order
      state     2 ulp of fp32: one rounding from a float64 value, plus the rounding of the inputs of 1 / (std + eps)
      out       4 ulp of fp32 of the float64 value formed from the same fp32 mean and inv_std; a column equal to its mean gives 0 (the constant column of every warm case)
      fold      W' 1 ulp; b' 1 ulp + 2^-40 sum |W mean inv_std| (the float64 sum in another order), from the fp32 state `got` holds
    Prints every figure before it asserts; returns them."""
    s1, s2, sabs = sums(x, mean0)
    fig = {}
    fig["S1 rel"] = float((np.abs(got["sums"][0] - s1) / np.maximum(sabs, 1e-300)).max())
    fig["S2 rel"] = float((np.abs(got["sums"][1] - s2) / np.maximum(s2, 1e-300)).max())
    mean1, var1, count1 = update(mean0, var0, count0, x, until)
    std1, inv1 = derived(var1, eps)
    ok = {}
    for k, want in (("mean", mean1), ("var", var1), ("std", std1), ("inv_std", inv1)):
        ok[k], fig[k + " ulp"] = within_ulps(got[k], want, 2)
    inv0 = inv_std32(var0, eps)
    want_out = normalise(x, mean0, inv0)
    ok["out"], fig["out ulp"] = within_ulps(got["out"], want_out, 4)
    exact = f64(x) == f64(mean0)[None, :]
    wf, bf, babs = fold(w1, b1, got["mean"], got["inv_std"])
    ok["w1"], fig["w1 ulp"] = within_ulps(got["w1_out"], wf, 1)
    ok["b1"], fig["b1 ulp"] = within_ulps(got["b1_out"], bf, 1, extra=2.0 ** -40 * babs)
    print(f"[obs_norm {label}]", " ".join(f"{k} {v:.3g}" for k, v in fig.items()), flush=True)
    assert fig["S1 rel"] <= 1e-12 and fig["S2 rel"] <= 1e-12, (label, fig)
    assert int(got["count"]) == count1, (label, int(got["count"]), count1)
    assert all(ok.values()), (label, ok, fig)
    if count0 > 0 and x.shape[1] >= 2:      # a warm state of the same columns holds the constant column's value as its mean, bit for bit
        assert exact[:, 0].all(), label
    assert (np.asarray(got["out"])[exact] == 0.0).all(), label
    return fig

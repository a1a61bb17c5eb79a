"""GPU: the observation-corruption launch (csrc/wl_obs_corrupt.hip) against the reference (tests/obs_corrupt_reference.py) -- the kernel
alone on guarded buffers.  Held to: byte for byte (uint32) on the constant path, the uniform path, pass-through, clip, scale and the
stored bias block whenever the bias kind is constant or uniform; the Gaussian path against the float64 Box-Muller of the same 16-bit
uniforms within a tolerance that is derived, not measured:

  z = r cos(2 pi u1), r = sqrt(-2 ln u0).  The device takes ln from v_log_f32 (log2, times a rounded ln 2), the root from v_sqrt_f32 and
  the cosine from v_cos_f32 of u1 REVOLUTIONS (no 2 pi product).  The allowances are the ones the project already fixes for the policy
  draw (tests/policy_reference.py DRAW_R, DRAW_TRIG; wl_math.h: sqrt / log "1 ulp class", sin / cos "~1e-6 abs"): 2^-20 relative on r,
  2^-20 absolute on the cosine.  With u0 >= 2^-17, r <= R_MAX = sqrt(34 ln 2) = 4.855, so
      |dz| <= r 2^-20 |c| + r 2^-20 + 2^-24 r <= R_MAX (2^-19 + 2^-24) = 9.55e-6 = EZ_DEVICE.
  The column then goes through d = fmaf(z, std, mean), the operation, the bias, the clip and the scale, each one float32 rounding
  (2^-24 of its result) that passes earlier errors on with gain <= 1, |x| (operation scale) and |scale|; the reference evaluates
      tol = |s| (g (std EZ + 2^-24 |d|) + 2^-24 (|y1| + |y2|) + bias_err) + 2^-24 |y3| + 2^-149
  per element (its docstring).  Nothing in it comes from the kernel's output; the largest error seen is printed for DESIGN section 20.

Inputs carry quiet and signalling NaNs of distinct payloads, both infinities, -0.0 and denormals (special_words); in an arithmetic
column any NaN equals any NaN (which operand's payload an addition keeps is not the contract), in an untouched column the words are
compared as they are."""
import numpy as np
import pytest
import torch

from tests import obs_corrupt_reference as R
from tests.obs_history_reference import special_words
from tests.test_obs_corrupt_cpu import check_statistics, stats_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7FC0BEEF            # a NaN pattern: what `out` and its guard rows hold before the launch
TABLES = R.tables()
SEED = 0x0123_4567_89AB_CDEF


def _lib():
    from wheeledlab_amd import _abi as A
    return A, A.load()


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).to(DEV)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _inputs(rng, shape):
    x = special_words(rng, shape)
    x[x == GUARD] ^= np.uint32(1)
    return x


def _ctable(A, tab):
    rows = R.rows(tab)
    return (A.WlObsCorruptTerm * len(rows))(*[A.WlObsCorruptTerm(*r) for r in rows])


class Launch:
    """one table on the device: launches on guarded buffers, every launch held to the reference"""

    def __init__(self, name_or_terms, n, rng):
        self.A, self.lib = _lib()
        self.tab, self.D, self.Db = R.table(TABLES[name_or_terms] if isinstance(name_or_terms, str) else name_or_terms)
        self.ct = _ctable(self.A, self.tab)
        assert self.lib.wl_obs_corrupt_width(self.ct, len(self.tab), self.D) == self.Db
        self.n, self.rng = n, rng
        self.stream = self.A.stream(torch.device(DEV))
        self.state_w = R.state_block(rng, n, stride=n + 5)
        self.state = _dev(self.state_w)
        self.worst = 0.0

    def run(self, obs_w, bias_w, ra_w, rb_w, step, env_offset=0, enable=1, out_extra=0, offset=0, in_place=False, seed=SEED, check=True):
        """-> (out words [n, D], bias float32 [n, Db], Result)"""
        n, D, Db = self.n, self.D, self.Db
        stride = obs_w.shape[1]
        obs = _dev(obs_w)
        bias = torch.from_numpy(np.ascontiguousarray(bias_w, np.float32).copy()).to(DEV) if Db else None
        ra = torch.from_numpy(np.ascontiguousarray(ra_w, bool).copy()).to(DEV)
        rb = None if rb_w is None else torch.from_numpy(np.ascontiguousarray(rb_w, bool).copy()).to(DEV)
        if in_place:
            out, out_stride, buf, lo, total = obs, stride, None, 0, 0
        else:
            out_stride = D + out_extra
            total, guard = n * out_stride, 2 * out_stride
            lo = guard + (offset - guard) % 4                                   # `out` starts `offset` words into a 16-byte line
            buf = torch.full((lo + total + guard,), GUARD, dtype=torch.int32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            out = buf[lo:lo + total]
            assert (out.data_ptr() // 4) % 4 == offset
        rc = self.lib.wl_obs_corrupt_apply(n, D, obs.data_ptr(), stride, self.ct, len(self.tab), self.state.data_ptr(), self.state_w.shape[1],
                                           bias.data_ptr() if Db else None, ra.data_ptr(), None if rb is None else rb.data_ptr(), out.data_ptr(),
                                           out_stride, seed, step, env_offset, enable, self.stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        if in_place:
            full = _host(obs).reshape(n, stride)
            assert np.array_equal(full[:, D:], obs_w[:, D:])                     # the row's padding is not touched
        else:
            got = _host(buf)
            assert (got[:lo] == GUARD).all() and (got[lo + total:] == GUARD).all()   # every guard word unchanged
            full = got[lo:lo + total].reshape(n, out_stride)
            assert (full[:, D:] == GUARD).all()
            assert np.array_equal(_host(obs), obs_w)
        assert np.array_equal(_host(self.state), self.state_w)
        words = full[:, :D].copy()
        new_bias = bias.cpu().numpy() if Db else np.zeros((n, 0), np.float32)
        fresh = np.asarray(ra_w, bool) | (np.asarray(rb_w, bool) if rb_w is not None else False)
        res = R.apply(self.tab, obs_w[:, :D], bias_w, fresh, seed, step, env_offset, enable, state=self.state_w)
        if check:
            self.worst = max(self.worst, R.check(words, res, what=f"n={n} step={step}"))
            if Db:
                R.check_bias(new_bias, res)
            if not enable:
                assert np.array_equal(new_bias.view(np.uint32), np.ascontiguousarray(bias_w, np.float32).view(np.uint32))
        return words, new_bias, res


CASES = [(name, n) for name in TABLES if name != "visual" for n in (1, 3, 64, 65, 257)] + [("visual", 3)]


@pytest.mark.parametrize("name,n", CASES)
def test_kernel_equals_the_reference_and_writes_nothing_else(name, n):
    rng = np.random.default_rng(n * 131 + len(name))
    L = Launch(name, n, rng)
    D, Db = L.D, L.Db
    rnd = lambda p: rng.random(n) < p
    bias = lambda: rng.standard_normal((n, Db)).astype(np.float32)
    a, b = rnd(0.4), rnd(0.3)
    # `out` at each of the four places inside a 16-byte line, strided rows in and out, reset_b NULL, corruption off, in place,
    # env ids and steps beyond 2^32
    w0, _, _ = L.run(_inputs(rng, (n, D)), bias(), a, b, step=7)
    L.run(_inputs(rng, (n, D + 5)), bias(), a, b, step=8, out_extra=3, offset=1)
    L.run(_inputs(rng, (n, D)), bias(), a, None, step=9, offset=2)
    L.run(_inputs(rng, (n, D + 1)), bias(), np.ones(n, bool), None, step=10, enable=0, offset=3)
    L.run(_inputs(rng, (n, D + 2)), bias(), a, b, step=11, in_place=True)
    L.run(_inputs(rng, (n, D)), bias(), b, a, step=(1 << 40) + 12345, env_offset=(1 << 35) + 77, offset=1)
    L.run(_inputs(rng, (n, D)), bias(), np.zeros(n, bool), np.zeros(n, bool), step=(1 << 32), env_offset=(1 << 32) - 2)   # ids wrap through 2^32
    if name == "identity":
        assert L.worst == 0.0
    print(f"\nOBSCORRUPT kernel {name} n={n}: largest Gaussian error / tolerance {L.worst:.4f}")


def test_largest_error_of_the_device_normal():
    """z itself: operation abs with mean 0, std 1 gives d = fmaf(z, 1, 0) = z; 2^20 words"""
    n, D = 1024, 1024
    L = Launch([R.term(D, R.gaussian(0.0, 1.0), op=R.ABS)], n, np.random.default_rng(5))
    words, _, res = L.run(np.zeros((n, D), np.uint32), None, np.zeros(n, bool), None, step=3, check=False)
    z, want = words.view(np.float32).astype(np.float64), res.y64
    err = np.abs(z - want)
    print(f"\nOBSCORRUPT device normal: max |z - z64| = {err.max():.3e} (allowance {R.EZ_DEVICE:.3e}), max |z| = {np.abs(z).max():.4f}")
    assert err.max() <= R.EZ_DEVICE and np.abs(z).max() <= R.R_MAX
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 5 / np.sqrt(2 * z.size)


@pytest.mark.parametrize("name", ["every_constant", "every_uniform", "every_gaussian"])
def test_nan_in_gives_nan_out_for_every_arithmetic_term(name):
    n = 5
    rng = np.random.default_rng(3)
    L = Launch(name, n, rng)
    obs = np.full((n, L.D), 0x7FC00001, np.uint32)
    obs[1] = 0xFF800123                                                        # signalling, negative
    obs[2] = 0x7FFFFFFF
    obs[3] = (np.uint32(0x7FC00000) | rng.integers(1, 1 << 22, L.D).astype(np.uint32))
    for enable in (1, 0):
        words, _, res = L.run(obs, np.zeros((n, L.Db), np.float32), np.ones(n, bool), None, step=4, enable=enable)
        assert np.isnan(words.view(np.float32)).all()                           # with a clip and without, with a scale and without
        assert np.array_equal(words[:, ~res.arith], obs[:, ~res.arith])         # untouched terms keep the payload


@pytest.mark.parametrize("name", ["drift", "elevation", "every_uniform", "every_gaussian"])
def test_sharding_determinism_and_fresh_draws_every_step(name):
    n, a, b = 65, 23, 52
    rng = np.random.default_rng(17)
    L = Launch(name, n, rng)
    obs = np.ascontiguousarray(rng.standard_normal((n, L.D)).astype(np.float32).view(np.uint32))
    bias = rng.standard_normal((n, L.Db)).astype(np.float32)
    ra = rng.random(n) < 0.5
    whole, wbias, res = L.run(obs, bias, ra, None, step=100)
    again, abias, _ = L.run(obs, bias, ra, None, step=100)
    assert np.array_equal(whole, again) and np.array_equal(wbias.view(np.uint32), abias.view(np.uint32))      # same (seed, step): same bytes
    # rows [a, b) of the launch at env_offset 0 == a launch of b - a envs at env_offset a
    S = Launch(name, b - a, rng)
    S.state_w = np.ascontiguousarray(L.state_w[:, a:a + (b - a) + 5])
    S.state = _dev(S.state_w)
    part, pbias, _ = S.run(obs[a:b], bias[a:b], ra[a:b], None, step=100, env_offset=a)
    assert np.array_equal(part, whole[a:b]) and np.array_equal(pbias.view(np.uint32), wbias[a:b].view(np.uint32))
    # the next step: every column with a uniform or Gaussian draw differs (finite inputs; constant noise and the held bias do not)
    nxt, _, _ = L.run(obs, bias, np.zeros(n, bool), None, step=101)
    base, _, _ = L.run(obs, bias, np.zeros(n, bool), None, step=100)
    for t in L.tab:
        cols = slice(t["off"], t["off"] + t["width"])
        drawn = t["noise_kind"] in (R.UNIFORM, R.GAUSSIAN)
        same = (nxt[:, cols] == base[:, cols])
        if not drawn:
            assert same.all()
        elif t["clip_lo"] == -R.INF:                                            # (a clipped column may sit on its bound at both steps)
            assert same.mean() < 0.01, (t["off"], same.mean())
            assert not same.all(0).any()                                        # no column repeats


def test_statistics_of_4096_envs_over_64_steps():
    """one launch sequence on the drift layout: ranges, moments within 5 standard errors for the sample count, correlations between
    adjacent columns, adjacent envs, consecutive steps and a term's noise and its bias below 5 / sqrt(count) -- the checks the
    reference passes on the CPU (tests/test_obs_corrupt_cpu.py)"""
    A, lib = _lib()
    tab, D, Db = stats_table()
    n, K = 4096, 64
    ct = _ctable(A, tab)
    obs = torch.zeros(n, D, dtype=torch.float32, device=DEV)
    outs = torch.zeros(K, n, D, dtype=torch.float32, device=DEV)
    biases = torch.zeros(K, n, Db, dtype=torch.float32, device=DEV)
    ones = torch.ones(n, dtype=torch.uint8, device=DEV)
    s = A.stream(torch.device(DEV))
    for k in range(K):
        assert lib.wl_obs_corrupt_apply(n, D, obs.data_ptr(), D, ct, len(tab), None, 0, biases[k].data_ptr(), ones.data_ptr(), None, outs[k].data_ptr(),
                                        D, 42, 1000 + k, 0, 1, s) == 0
    torch.cuda.synchronize()
    o, b = outs.cpu().numpy(), biases.cpu().numpy()
    check_statistics(o, b, tab)
    u = o[:, :, 6:9]
    assert (u >= np.float32(-0.1)).all() and (u < np.float32(0.1)).all()        # [n_min, n_max) exactly
    # the uniform columns and the uniform bias are the reference's, byte for byte, at a step in the middle
    res = R.apply(tab, np.zeros((n, D), np.uint32), np.zeros((n, Db), np.float32), np.ones(n, bool), 42, 1031, 0, True)
    assert np.array_equal(o[31][:, res.exact].view(np.uint32), res.bits[:, res.exact]) and np.array_equal(b[31].view(np.uint32), res.bias.view(np.uint32))


def test_bias_is_held_for_the_episode_and_redrawn_exactly_on_flagged_steps():
    n, K = 33, 20
    rng = np.random.default_rng(9)
    terms = [R.term(3, R.gaussian(0.0, 0.1), bias=R.uniform(-0.5, 0.5)), R.term(5, R.uniform(-0.1, 0.1), bias=R.gaussian(0.0, 0.3), per_component=False),
             R.term(2), R.term(4, R.constant(0.0), bias=R.uniform(1.0, 2.0), per_component=False)]
    L = Launch(terms, n, rng)
    model = R.BiasModel(L.tab, n)
    bias = np.zeros((n, L.Db), np.float32)
    flags = rng.random((K, n)) < 0.25
    flags[:, 0], flags[:, 1], flags[3:6, 2] = False, True, True
    zeros = np.zeros((n, L.D), np.uint32)
    drawn = np.zeros(n, bool)                                                   # envs whose bias was ever drawn
    for k in range(K):
        enable = int(k != 7)
        a = flags[k] & (np.arange(n) % 2 == 0)
        b = flags[k] & ~a
        words, new, res = L.run(zeros, bias, a, b, step=50 + k, enable=enable)
        changed = (new.view(np.uint32) != bias.view(np.uint32)).any(1)
        if enable:
            assert changed[flags[k]].all() and not changed[~flags[k]].any()     # redrawn on exactly the flagged envs
            want = model.step(flags[k], SEED, 50 + k, 0, True)
            exact = np.array([True, True, True, False, True])                   # (slot 3 is the Gaussian bias: within its tolerance, above)
            assert np.array_equal(new[:, exact].view(np.uint32), want[:, exact].view(np.uint32))
            # one value per env and term across the columns: out - noise is the bias; the constant-noise term shows it directly
            drawn |= flags[k]
            got = words.view(np.float32)[:, 10:14]
            assert (got == new[:, [4]]).all() and (got[drawn] >= 1.0).all() and (got[drawn] < 2.0).all() and (got[~drawn] == 0).all()
        else:
            assert not changed.any()                                            # enable = 0: untouched
        bias = new
    assert (bias[0] == 0).all()                                                 # the env that never reset never drew

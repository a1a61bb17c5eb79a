"""The contract of the observation corruption (include/wheeledlab_amd_obsnoise.h) restated in numpy over oracle/philox.py.

The draws.  Column c of env e at (seed, step) takes word c & 3 of the Philox block with counter (uint32(env_offset + e), step low, step
high, stream | (c >> 2) << 8); stream 16 for the per-step noise, 17 for the per-episode bias.  From its word w
    constant  d = a
    uniform   d = fma(u01(w), b, a), u01 = (w >> 8) 2^-24, a = n_min, b = fp32(n_max - n_min): ONE rounding.  fma_f32 below is exact: the
              product of two 24-bit significands is exact in float64, the sum is taken with its rounding error (TwoSum), and the one case
              in which rounding the float64 sum to float32 differs from rounding the exact value -- the sum sits on a float32 tie and the
              error breaks it -- is resolved by the error's sign.  tests/test_obs_corrupt_cpu.py holds it to rational arithmetic.
    Gaussian  d = a + b z in float64, z = sqrt(-2 ln u0) cos(2 pi u1), u0 = ((w & 0xffff) + 1/2) 2^-16, u1 = ((w >> 16) + 1/2) 2^-16
then y = x + d | x * d | d (abs: a NaN x stays), + bias, clip as two selections (a NaN stays), * scale -- each a float32 rounding.
Columns whose draws are constant or uniform are exact (uint32 words); Gaussian columns carry a float64 value and a tolerance:

  EZ, the error of z on the device: the allowance the project fixes for the hardware v_log_f32 + v_sqrt_f32 (2^-20 relative on r) and
  v_sin_f32 / v_cos_f32 of u1 revolutions (2^-20 absolute; wl_math.h: "~1e-6 abs"), tests/policy_reference.py DRAW_R / DRAW_TRIG: with
  r <= R_MAX = sqrt(34 ln 2) = 4.855 (u0 >= 2^-17), |dz| <= r 2^-20 |c| + r 2^-20 + 2^-24 r (the product's rounding) <= R_MAX (2^-19 + 2^-24).
  On the host (tests/host_sim: log2f within 1 ulp, a rounded ln 2 and its product 1 ulp more, the correctly rounded sqrt halving that and
  adding 1/2: r within 1.75 ulp; cos correctly rounded from double: 2^-25 absolute; the product 1/2 ulp):
  |dz| <= r (1.75 2^-23 + 2^-25 + 2^-24) < R_MAX 2^-22 = EZ_HOST -- "a few ulp".
  Every later float32 operation adds half an ulp of its result, 2^-24 |v|, and passes earlier errors on with gain <= 1 (add, clip),
  |x| (operation scale, on d's error) and |scale|:
      tol = |s| (g (|b| EZ + 2^-24 |d|) + 2^-24 (|y1| + |y2|) + bias_err) + 2^-24 |y3| + 2^-149
  g = 1 | |x| | 1;  y1, y2, y3 the values after the operation, the bias and the scale;  bias_err = 0 for a bias held exactly,
  |b_bias| EZ + 2^-24 |bias| for a Gaussian one drawn in this call.

apply() is a pure function of its inputs (the bias block in, the bias block out); BiasModel is the literal per-env model of the bias
bookkeeping, scalar arithmetic in rationals, that tests hold against it."""
from fractions import Fraction
import math

import numpy as np

from oracle import philox as PH

NONE, CONSTANT, UNIFORM, GAUSSIAN = 0, 1, 2, 3
ADD, SCALE, ABS = 0, 1, 2
S_NOISE, S_BIAS = 16, 17
MAX_TERMS = 64
R_MAX = math.sqrt(34.0 * math.log(2.0))
EZ_DEVICE = R_MAX * (2.0 ** -19 + 2.0 ** -24)
EZ_HOST = R_MAX * 2.0 ** -22
F32, F64, U32 = np.float32, np.float64, np.uint32
INF = float("inf")
FIELDS = ("off", "width", "noise_kind", "noise_op", "noise_a", "noise_b", "bias_kind", "bias_per_component", "bias_a", "bias_b", "bias_off",
          "has_scale", "clip_lo", "clip_hi", "scale", "state_row")       # WlObsCorruptTerm, in order


def f32(v):
    return float(np.float32(v))


def uniform(n_min, n_max):
    """(kind, a, b) of a uniform draw: the span is formed once, in fp32"""
    return (UNIFORM, f32(n_min), float(np.float32(n_max) - np.float32(n_min)))


def gaussian(mean, std):
    return (GAUSSIAN, f32(mean), f32(std))


def constant(bias):
    return (CONSTANT, f32(bias), 0.0)


def term(width, noise=None, op=ADD, bias=None, per_component=True, clip=None, scale=None, state_row=-1):
    nk, na, nb = noise or (NONE, 0.0, 0.0)
    bk, ba, bb = bias or (NONE, 0.0, 0.0)
    lo, hi = clip or (-INF, INF)
    return dict(width=int(width), noise_kind=nk, noise_op=op, noise_a=na, noise_b=nb, bias_kind=bk, bias_per_component=int(bool(per_component)),
                bias_a=ba, bias_b=bb, has_scale=int(scale is not None), clip_lo=f32(lo), clip_hi=f32(hi), scale=1.0 if scale is None else f32(scale),
                state_row=int(state_row))


def table(terms):
    """terms back to back -> (list of dicts with off and bias_off filled in, D, Db)"""
    out, off, boff = [], 0, 0
    for t in terms:
        t = dict(t, off=off, bias_off=boff)
        out.append(t)
        off += t["width"]
        if t["bias_kind"] != NONE:
            boff += t["width"] if t["bias_per_component"] else 1
    return out, off, boff


def rows(tab):
    """the table as tuples in the field order of WlObsCorruptTerm"""
    return [tuple(t[f] for f in FIELDS) for t in tab]


# ---- exact float32 arithmetic ------------------------------------------------------------------------------------------------

def fma_f32(u, b, a):
    """round_to_float32(u * b + a) for float32 arrays, exactly (finite values whose product and sum stay normal in float64)"""
    u, b, a = (np.asarray(v, F32).astype(F64) for v in (u, b, a))
    p = u * b                                   # exact: 24 + 24 bits
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)             # TwoSum: s + err is the exact value
    r = s.astype(F32)
    rd = r.astype(F64)
    other = np.where(s > rd, np.nextafter(r, F32(INF)), np.nextafter(r, F32(-INF))).astype(F64)
    tie = (s != rd) & (np.abs(s - rd) == np.abs(other - s))
    up = np.maximum(rd, other)
    down = np.minimum(rd, other)
    fixed = np.where(err > 0, up, down)
    return np.where(tie & (err != 0), fixed, rd).astype(F32)


def round_fraction_f32(q: Fraction) -> float:
    """the float32 nearest to a rational (ties to even), as a Python float; |q| below the float32 range rounds on the denormal grid"""
    if q == 0:
        return 0.0
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()       # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                        # now 2^e <= q < 2^(e+1)
    g = max(e - 23, -149)                                             # the grid: ulp = 2^g
    m = q / Fraction(2) ** g
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * math.ldexp(n, g)


def u01(w):
    return ((np.asarray(w, U32) >> U32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def z64(w):
    """the float64 Box-Muller normal of a word: radius from its low half, angle from its high half"""
    w = np.asarray(w, U32)
    u0 = ((w & U32(0xFFFF)).astype(F64) + 0.5) * 2.0 ** -16
    u1 = ((w >> U32(16)).astype(F64) + 0.5) * 2.0 ** -16
    return np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)


def words(env_ids, step, stream, seed, cols):
    """uint32 [n, len(cols)]: the word of every column"""
    cols = np.asarray(cols, np.int64)
    out = np.empty((len(env_ids), len(cols)), U32)
    for b in np.unique(cols >> 2):
        blk = PH.philox4x32(env_ids, int(step), stream | (int(b) << 8), int(seed))
        sel = np.nonzero((cols >> 2) == b)[0]
        out[:, sel] = blk[cols[sel] & 3].T
    return out


def draw(kind, a, b, w):
    """-> (float32 draw, exact?) ; a Gaussian draw is float32(float64 value): use draw64 for the value"""
    if kind == CONSTANT:
        return np.full(w.shape, a, F32), True
    if kind == UNIFORM:
        return fma_f32(u01(w), np.full(w.shape, b, F32), np.full(w.shape, a, F32)), True
    return draw64(kind, a, b, w).astype(F32), False


def draw64(kind, a, b, w):
    if kind == GAUSSIAN:
        return a + b * z64(w)
    return draw(kind, a, b, w)[0].astype(F64)


def _chain(x, d, op, bv, t, dt):
    lo, hi, s = dt(t["clip_lo"]), dt(t["clip_hi"]), dt(t["scale"])
    with np.errstate(all="ignore"):
        if d is None:
            y = x
        elif op == ADD:
            y = x + d
        elif op == SCALE:
            y = x * d
        else:
            y = np.where(np.isnan(x), x, d)
        y1 = y
        if bv is not None:
            y = y + bv
        y2 = y
        y = np.where(y < lo, lo, y)
        y = np.where(y > hi, hi, y)
        if t["has_scale"]:
            y = y * s
    return y.astype(dt), y1, y2


class Result:
    """bits uint32 [n, D] (exact columns: the words; others float32 of y64); y64, tol float64 [n, D]; arith bool [D] (False: the column
    is a copy of its input words); exact bool [D]; bias float32 [n, Db] after the call; bias_tol float64 [n, Db] (0: exact)"""


def apply(tab, x_bits, bias, reset, seed, step, env_offset, enable, state=None, ez=EZ_DEVICE):
    tab = list(tab)
    x_bits = np.asarray(x_bits, U32)
    n = x_bits.shape[0]
    D = sum(t["width"] for t in tab)
    env_ids = (np.arange(n, dtype=np.uint64) + np.uint64(int(env_offset) & 0xFFFFFFFFFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    reset = np.asarray(reset, bool)
    r = Result()
    r.bits, r.y64, r.tol = np.zeros((n, D), U32), np.zeros((n, D), F64), np.zeros((n, D), F64)
    r.arith, r.exact = np.zeros(D, bool), np.ones(D, bool)
    r.bias = None if bias is None else np.array(bias, F32, copy=True)
    r.bias_tol = None if bias is None else np.zeros(r.bias.shape, F64)
    half = 2.0 ** -24
    for t in tab:
        off, w = t["off"], t["width"]
        cols = np.arange(off, off + w)
        xb = x_bits[:, cols] if t["state_row"] < 0 else np.asarray(state, U32)[t["state_row"]:t["state_row"] + w, :n].T
        kind = t["noise_kind"] if enable else NONE
        clip = t["clip_lo"] > -INF or t["clip_hi"] < INF
        if kind == NONE and not clip and not t["has_scale"]:
            r.bits[:, cols] = xb
            with np.errstate(all="ignore"):
                r.y64[:, cols] = xb.view(F32).astype(F64)
            continue
        r.arith[cols] = True
        x32 = np.ascontiguousarray(xb).view(F32)
        d32 = d64 = bv32 = bv64 = None
        exact, bias_err = True, 0.0
        if kind != NONE:
            wn = words(env_ids, step, S_NOISE, seed, cols)
            d32, ex = draw(kind, t["noise_a"], t["noise_b"], wn)
            d64 = draw64(kind, t["noise_a"], t["noise_b"], wn)
            exact &= ex
            if t["bias_kind"] != NONE:
                per = bool(t["bias_per_component"])
                slots = t["bias_off"] + (np.arange(w) if per else np.zeros(1, np.int64))
                bias_err = np.zeros((n, len(slots)), F64)
                if reset.any():
                    wbias = words(env_ids, step, S_BIAS, seed, cols if per else cols[:1])
                    fresh, ex = draw(t["bias_kind"], t["bias_a"], t["bias_b"], wbias)
                    sel = np.ix_(reset, slots)
                    r.bias[sel] = fresh[reset]
                    if not ex:
                        r.bias_tol[sel] = (abs(t["bias_b"]) * ez + half * np.abs(fresh.astype(F64)))[reset]
                        bias_err[reset] = r.bias_tol[sel]
                bv32 = np.broadcast_to(r.bias[:, slots], (n, w)) if not per else r.bias[:, slots]
                bv64 = bv32.astype(F64)
                bias_err = np.broadcast_to(bias_err, (n, w))
                exact &= not np.any(bias_err)
        y32, _, _ = _chain(x32, d32, t["noise_op"], bv32, t, F32)
        with np.errstate(invalid="ignore"):       # (a signalling NaN widens to a quiet one)
            x64 = x32.astype(F64)
        y64, y1, y2 = _chain(x64, d64, t["noise_op"], bv64, t, F64)
        r.exact[cols] = exact
        r.bits[:, cols] = y32.view(U32)
        r.y64[:, cols] = y64
        if not exact:
            with np.errstate(all="ignore"):
                g = np.abs(x32.astype(F64)) if t["noise_op"] == SCALE else 1.0
                dz = abs(t["noise_b"]) * ez if kind == GAUSSIAN else 0.0
                inner = g * (dz + half * np.abs(d64)) + half * (np.abs(y1) + np.abs(y2)) + (bias_err + half * np.abs(bv64) if bv64 is not None else 0.0)
                r.tol[:, cols] = abs(t["scale"]) * inner + half * np.abs(y64) + 2.0 ** -149
    return r


def check(got_bits, res, what=""):
    """hold an output [n, D] (uint32) to a Result: untouched columns and exact columns byte for byte -- in an arithmetic column any NaN
    equals any NaN (which operand's payload survives an addition is not the contract) --, Gaussian columns within tol, non-finite
    values of them by class.  -> the largest error / tolerance ratio seen on the Gaussian columns"""
    got_bits = np.asarray(got_bits, U32)
    gf = got_bits.view(F32)
    want = res.bits.view(F32)
    copy = ~res.arith
    assert np.array_equal(got_bits[:, copy], res.bits[:, copy]), f"{what}: an untouched column changed its words"
    ex = res.arith & res.exact
    both_nan = np.isnan(gf) & np.isnan(want)
    bad = (got_bits != res.bits) & ~both_nan
    assert not bad[:, ex].any(), f"{what}: exact columns differ at {np.argwhere(bad[:, ex])[:5].tolist()}"
    ap = res.arith & ~res.exact
    if not ap.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        g = gf[:, ap].astype(F64)
    y, tol = res.y64[:, ap], res.tol[:, ap]
    fin = np.isfinite(y) & np.isfinite(tol)
    assert np.array_equal(np.isnan(g), np.isnan(y)), f"{what}: NaN pattern of the Gaussian columns"
    with np.errstate(all="ignore"):
        err = np.abs(g - y)
    assert np.isfinite(g[fin]).all(), what
    ratio = np.where(fin, err / tol, 0.0)
    assert (ratio <= 1.0).all(), f"{what}: Gaussian columns off by up to {ratio.max():.3g} of the tolerance (abs {np.nanmax(np.where(fin, err, 0)):.3g})"
    return float(ratio.max())


def check_bias(got, res, what=""):
    """the stored bias block: byte for byte where the bias kind is constant or uniform, within bias_tol where it is Gaussian"""
    got = np.asarray(got, F32)
    exact = res.bias_tol == 0
    assert np.array_equal(got.view(U32)[exact], res.bias.view(U32)[exact]), f"{what}: the bias block differs"
    assert (np.abs(got.astype(F64) - res.bias.astype(F64))[~exact] <= res.bias_tol[~exact]).all(), f"{what}: Gaussian bias beyond its tolerance"


class BiasModel:
    """the literal model: per env and bias term a list of values, redrawn -- one scalar Philox call per value, rational arithmetic for
    the uniform draw -- when the env resets while corruption is enabled, untouched otherwise"""

    def __init__(self, tab, n, init=0.0):
        self.tab = [t for t in tab if t["bias_kind"] != NONE and t["noise_kind"] != NONE]
        self.n = n
        self.values = [[[init] * (t["width"] if t["bias_per_component"] else 1) for t in self.tab] for _ in range(n)]

    @staticmethod
    def scalar_draw(kind, a, b, env, step, seed, col):
        if kind == CONSTANT:
            return a
        w = int(PH.philox4x32(np.asarray([env & 0xFFFFFFFF], np.uint64), int(step), S_BIAS | ((col >> 2) << 8), int(seed))[col & 3, 0])
        if kind == UNIFORM:
            return round_fraction_f32(Fraction(w >> 8, 1 << 24) * Fraction(b) + Fraction(a))
        u0, u1 = ((w & 0xFFFF) + 0.5) / 65536.0, ((w >> 16) + 0.5) / 65536.0
        return float(np.float32(a + b * math.sqrt(-2.0 * math.log(u0)) * math.cos(2.0 * math.pi * u1)))

    def step(self, reset, seed, step, env_offset, enable):
        for e in range(self.n):
            if not (enable and reset[e]):
                continue
            for k, t in enumerate(self.tab):
                cols = range(t["off"], t["off"] + t["width"]) if t["bias_per_component"] else [t["off"]]
                self.values[e][k] = [self.scalar_draw(t["bias_kind"], t["bias_a"], t["bias_b"], env_offset + e, step, seed, c) for c in cols]
        return np.asarray([[v for term in env for v in term] for env in self.values], F32).reshape(self.n, -1)


# ---- the tables of the tests -------------------------------------------------------------------------------------------------
ACT_ROW = 20          # any two rows of the test's state block (the env uses WL_S_ACT0)


def _every(kind):
    """every operation x {clip, no clip} x {scale, none} x {no bias, bias per component, bias per env} of one noise kind on widths
    1, 2, 5 in turn (36 terms; all three kinds together would be 108 > 64 terms, so each kind has a table), then the terms that only
    clip, only scale, and do both, and one untouched term"""
    noise = {CONSTANT: constant(0.05), UNIFORM: uniform(-0.1, 0.3), GAUSSIAN: gaussian(0.02, 0.4)}[kind]
    biases = [constant(-0.25), uniform(-0.5, 0.25), gaussian(0.1, 0.2)]
    out, i = [], 0
    for op in (ADD, SCALE, ABS):
        for clip in (None, (-0.75, 0.5)):
            for scale in (None, -1.5):
                for b in (0, 1, 2):
                    bias = None if b == 0 else biases[i % 3]
                    out.append(term((1, 2, 5)[i % 3], noise, op, bias, per_component=b == 1, clip=clip, scale=scale))
                    i += 1
    out += [term(2, clip=(-0.5, 0.5)), term(1, scale=2.5), term(5, clip=(0.0, 1.0), scale=-0.5), term(3)]
    return out


def tables():
    g, u = gaussian, uniform
    return {
        "identity": [term(3), term(2)],
        "drift": [term(3, g(0.0, 0.1)), term(3, g(0.02, 0.1), scale=0.5), term(3, u(-0.1, 0.1)),
                  term(3, g(0.0, 0.4), bias=u(-0.05, 0.05)), term(2, u(-0.1, 0.1), clip=(-1.0, 1.0), state_row=ACT_ROW)],
        "elevation": [term(2, g(0.0, 0.05)), term(3, g(0.0, 0.02)), term(3, g(0.0, 0.1), clip=(-10.0, 10.0)),
                      term(3, g(0.0, 0.1), clip=(-10.0, 10.0)), term(2, g(0.0, 0.05), clip=(-1.0, 1.0), state_row=ACT_ROW),
                      term(676, g(0.0, 0.02), clip=(-10.0, 10.0))],
        "visual_small": [term(40), term(3, u(-0.1, 0.1)), term(3, u(-0.1, 0.1)), term(2, u(-0.1, 0.1), clip=(-1.0, 1.0), state_row=ACT_ROW)],
        "visual": [term(3200), term(3, u(-0.1, 0.1)), term(3, u(-0.1, 0.1)), term(2, u(-0.1, 0.1), clip=(-1.0, 1.0), state_row=ACT_ROW)],
        "every_constant": _every(CONSTANT),
        "every_uniform": _every(UNIFORM),
        "every_gaussian": _every(GAUSSIAN),
    }


def state_block(rng, n, stride=None, n_rows=ACT_ROW + 2):
    """a component-major state [n_rows, stride] of special words whose action rows reach beyond +-1"""
    from tests.obs_history_reference import special_words
    stride = n if stride is None else stride
    s = special_words(rng, (n_rows, stride))
    a = (rng.standard_normal((2, stride)) * 1.5).astype(F32)
    keep = rng.random((2, stride)) < 0.8
    s[ACT_ROW:ACT_ROW + 2] = np.where(keep, a.view(U32), s[ACT_ROW:ACT_ROW + 2])
    return s

"""The contract of the per-episode domain randomisation (include/wheeledlab_amd_events.h) restated in numpy over oracle/philox.py.

State: the four constant rows (mu_s, mu_d, damp, mass), the two mass parts and per term time_left (float32), applied (uint32) and the
two words w2, w3 (reset terms: the step of the last application; interval terms: w2 = drawn, the timer draws so far).  apply() is one
call of wl_event_rand_apply: the reset terms, then the interval terms, each in table order, vectorised over the envs.

Exact (compared as uint32 words): the bucket picks and materials, every uniform draw (fma_f32 of tests/obs_corrupt_reference.py is
one rounding, held there to rational arithmetic), the operations on them (one float32 rounding each, numpy's), the timers, the
counters, the step words.  Carried as a float64 value and a tolerance: what a Gaussian or log_uniform draw reaches.

  Gaussian.  d = fmaf(z, std, mean).  z is within EZ of the float64 Box-Muller value (EZ_DEVICE / EZ_HOST, derived in
  tests/obs_corrupt_reference.py from the allowances the project fixes for v_log_f32, v_sqrt_f32 and v_cos_f32; reused, not refitted);
  the fmaf rounds once:  err(d) = std EZ + 2^-24 |d|.
  log_uniform.  x = fmaf(u, b, a) is exact (a, b are the float32 constants the host formed) and so is y = x * fp32(log2 e), one IEEE
  product the reference repeats; d = 2^y comes from v_exp_f32, a transcendental of the "1 ulp class" (wl_math.h; 1 ulp <= 2^-23
  relative), allowed twice that as the project allows its other hardware transcendentals double their stated class:
  err(d) = EXP_HW |d|, EXP_HW = 2^-22.  On the host exp2 is libm's in double, rounded once: 2^-24 |d| -- inside the same allowance.
  Then every float32 operation adds half an ulp of its result and passes earlier errors on with gain 1 (add, abs, the sums) or |base|
  (scale):
      value   = op(base, d):   err = g err(d) + 2^-24 |value|          g = 1 | |base| | 1  (abs: the value IS d, no further rounding)
      wheels  = (d0 + d1) + (d2 + d3):  err = sum err(d_i) + 2^-24 (|d0 + d1| + |d2 + d3| + |wheels|)
      mass    = part_base + part_wheels: err = err(part_base) + err(part_wheels) + 2^-24 |mass|
  A part or row that was NOT written in a call keeps its stored float32 exactly: its error is what it was stored with, carried along
  in `tol` (so that the mass row of a later call inherits it)."""
import math

import numpy as np

from oracle import philox as PH
from tests.obs_corrupt_reference import EZ_DEVICE, EZ_HOST, fma_f32, u01, z64  # noqa: F401

MU, DAMP, MASS_BASE, MASS_WHEELS = 0, 1, 2, 3
RESET, INTERVAL = 0, 1
ADD, SCALE, ABS = 0, 1, 2
UNIFORM, LOG_UNIFORM, GAUSSIAN = 0, 1, 2
S_VALUE, S_TIMER, S_BUCKET = 18, 19, 9
GLOBAL_ID = 0xFFFFFFFF
MAX_TERMS = 8
EXP_HW = 2.0 ** -22
HALF = 2.0 ** -24
F32, F64, U32 = np.float32, np.float64, np.uint32
LOG2E = np.float32(1.44269504088896340736)
FIELDS = ("target", "mode", "op", "dist", "p0", "p1", "base", "interval_lo", "interval_hi", "is_global_time", "min_step_count_between_reset",
          "mu_s_lo", "mu_s_hi", "mu_d_lo", "mu_d_hi", "num_buckets", "make_consistent")      # WlEventRandTerm, in order
STRUCT = "<iiiifffffiiffffii"
C_MU_S, C_MU_D, C_DAMP, C_MASS = 0, 1, 2, 3          # the rows of State.consts


def f32(v):
    return float(np.float32(v))


def term(target, mode, op=ABS, dist=UNIFORM, p=(0.0, 0.0), base=0.0, interval=(0.0, 0.0), global_time=0, min_steps=0, mu_s=(0.0, 0.0),
         mu_d=(0.0, 0.0), buckets=1, consistent=0):
    return dict(target=target, mode=mode, op=op, dist=dist, p0=f32(p[0]), p1=f32(p[1]), base=f32(base), interval_lo=f32(interval[0]),
                interval_hi=f32(interval[1]), is_global_time=int(global_time), min_step_count_between_reset=int(min_steps), mu_s_lo=f32(mu_s[0]),
                mu_s_hi=f32(mu_s[1]), mu_d_lo=f32(mu_d[0]), mu_d_hi=f32(mu_d[1]), num_buckets=int(buckets), make_consistent=int(consistent))


def rows(tab):
    return [tuple(t[f] for f in FIELDS) for t in tab]


def constants(t):
    """(a, b) of a term's draw as the host forms them, float32"""
    if t["dist"] == UNIFORM:
        return F32(t["p0"]), F32(F32(t["p1"]) - F32(t["p0"]))
    if t["dist"] == LOG_UNIFORM:
        l0, l1 = math.log(float(F32(t["p0"]))), math.log(float(F32(t["p1"])))
        return F32(l0), F32(l1 - l0)
    return F32(t["p0"]), F32(t["p1"])


def span(lo, hi):
    return F32(F32(hi) - F32(lo))


class State:
    """consts float32 [4, n], parts float32 [2, n], tl float32 [K, n], applied / w2 / w3 uint32 [K, n]; v64, tol float64 [6, n]: the
    float64 value and the tolerance of consts (0 .. 3) and parts (4, 5), tol 0 where the float32 is exact"""

    def __init__(self, n, K, consts=None, parts=None):
        self.n, self.K = n, K
        self.consts = np.zeros((4, n), F32) if consts is None else np.array(consts, F32)
        self.parts = np.zeros((2, n), F32) if parts is None else np.array(parts, F32)
        self.tl, self.applied = np.zeros((K, n), F32), np.zeros((K, n), U32)
        self.w2, self.w3 = np.zeros((K, n), U32), np.zeros((K, n), U32)
        self.v64 = np.concatenate([self.consts, self.parts]).astype(F64)
        self.tol = np.zeros((6, n), F64)

    def copy(self):
        s = State.__new__(State)
        s.n, s.K = self.n, self.K
        for k in ("consts", "parts", "tl", "applied", "w2", "w3", "v64", "tol"):
            setattr(s, k, getattr(self, k).copy())
        return s

    def block(self, stride):
        """the layer block as uint32 [2 + 4 K, stride]"""
        b = np.zeros((2 + 4 * self.K, stride), U32)
        b[0:2, :self.n] = self.parts.view(U32)
        for k in range(self.K):
            b[2 + 4 * k, :self.n] = self.tl[k].view(U32)
            b[3 + 4 * k, :self.n], b[4 + 4 * k, :self.n], b[5 + 4 * k, :self.n] = self.applied[k], self.w2[k], self.w3[k]
        return b


def _block(ids, c1, stream, seed):
    """Philox words uint32 [4, n] with per-env counter word c1 (array)"""
    ids, c1 = np.asarray(ids, np.uint64), np.asarray(c1, np.uint64)
    out = np.zeros((4, len(ids)), U32)
    for c in np.unique(c1):
        sel = c1 == c
        out[:, sel] = PH.philox4x32(ids[sel], int(c), stream, int(seed))
    return out


def _timer(t, k, ids, drawn, seed):
    w = _block(ids, drawn, S_TIMER | (k << 8), seed)[0]
    n = len(w)
    return fma_f32(u01(w), np.full(n, span(t["interval_lo"], t["interval_hi"])), np.full(n, F32(t["interval_lo"])))


def _draw(t, w, ez):
    """-> (float32 draw, float64 value, error) of one word array"""
    a, b = constants(t)
    n = len(w)
    if t["dist"] == GAUSSIAN:
        d64 = float(a) + float(b) * z64(w)
        return d64.astype(F32), d64, abs(float(b)) * ez + HALF * np.abs(d64)
    x = fma_f32(u01(w), np.full(n, b), np.full(n, a))
    if t["dist"] == UNIFORM:
        return x, x.astype(F64), np.zeros(n)
    y = (x * LOG2E).astype(F32)
    d64 = np.exp2(y.astype(F64))
    return d64.astype(F32), d64, EXP_HW * np.abs(d64)


def _op(op, base, d):
    return base + d if op == ADD else base * d if op == SCALE else d


def materials(t, seed):
    """(mu_s, mu_d) float32 [num_buckets]: the bucket materials, the startup path's"""
    nb = t["num_buckets"]
    m = PH.philox4x32(np.arange(nb, dtype=np.uint64), 0, S_BUCKET, int(seed))
    mu_s = fma_f32(u01(m[0]), np.full(nb, span(t["mu_s_lo"], t["mu_s_hi"])), np.full(nb, F32(t["mu_s_lo"])))
    mu_d = fma_f32(u01(m[1]), np.full(nb, span(t["mu_d_lo"], t["mu_d_hi"])), np.full(nb, F32(t["mu_d_lo"])))
    if t["make_consistent"]:
        mu_d = np.minimum(mu_d, mu_s)
    return mu_s, mu_d


def apply(tab, st, reset_a, reset_b, mask, mask_terms, seed, step, step_dt, env_offset, ez=EZ_DEVICE):
    """one call -> the new State (the input is left alone); .fired bool [K, n]: the applications of this call"""
    s = st.copy()
    n = s.n
    ids = (np.arange(n, dtype=np.uint64) + np.uint64(int(env_offset) & 0xFFFFFFFFFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    reset = np.asarray(reset_a, bool).copy()
    if reset_b is not None:
        reset |= np.asarray(reset_b, bool)
    masked = np.zeros(n, bool) if mask is None else np.asarray(mask, bool)
    dt = F32(step_dt)
    s.fired = np.zeros((len(tab), n), bool)
    touched_part = np.zeros(n, bool)
    for mode in (RESET, INTERVAL):
        for k, t in enumerate(tab):
            if t["mode"] != mode:
                continue
            forced = masked & bool((mask_terms >> k) & 1)
            if mode == RESET:
                last = s.w2[k].astype(np.uint64) | (s.w3[k].astype(np.uint64) << np.uint64(32))
                age = (np.uint64(step) - last) & np.uint64(0xFFFFFFFFFFFFFFFF)
                ok = np.ones(n, bool) if t["min_step_count_between_reset"] == 0 else (s.applied[k] == 0) | (age >= np.uint64(t["min_step_count_between_reset"]))
                ap = forced | (reset & ok)
                s.w2[k][ap], s.w3[k][ap] = U32(step & 0xFFFFFFFF), U32(step >> 32)
            else:
                tid = np.full(n, GLOBAL_ID, np.uint64) if t["is_global_time"] else ids
                first = (s.w2[k] == 0) | (reset & (not t["is_global_time"]))
                if first.any():
                    s.tl[k][first] = _timer(t, k, tid[first], s.w2[k][first], seed)
                    s.w2[k][first] += U32(1)
                s.tl[k] = (s.tl[k] - dt).astype(F32)
                fire = s.tl[k] < F32(1e-6)
                if fire.any():
                    s.tl[k][fire] = _timer(t, k, tid[fire], s.w2[k][fire], seed)
                    s.w2[k][fire] += U32(1)
                ap = fire | forced
            if not ap.any():
                continue
            s.fired[k] = ap
            w = _block(ids[ap], s.applied[k][ap], S_VALUE | (k << 8), seed)
            s.applied[k][ap] += U32(1)
            base = F32(t["base"])
            if t["target"] == MU:
                nb = t["num_buckets"]
                bucket = np.minimum((u01(w[0]) * F32(nb)).astype(F32).astype(np.int64), nb - 1)
                mu_s, mu_d = materials(t, seed)
                for r, v in ((C_MU_S, mu_s[bucket]), (C_MU_D, mu_d[bucket])):
                    s.consts[r][ap], s.v64[r][ap], s.tol[r][ap] = v, v.astype(F64), 0.0
                continue
            if t["target"] == MASS_WHEELS:
                d = [_draw(t, w[i], ez) for i in range(4)]
                with np.errstate(all="ignore"):
                    a32, b32 = (d[0][0] + d[1][0]).astype(F32), (d[2][0] + d[3][0]).astype(F32)
                    v32 = (a32 + b32).astype(F32)
                    a64, b64 = d[0][1] + d[1][1], d[2][1] + d[3][1]
                v64 = a64 + b64
                err = sum(x[2] for x in d)
                err = np.where(err > 0, err + HALF * (np.abs(a64) + np.abs(b64) + np.abs(v64)), 0.0)
                slot = 5
            else:
                d32, d64, derr = _draw(t, w[0], ez)
                with np.errstate(all="ignore"):
                    v32 = _op(t["op"], base, d32).astype(F32)
                v64 = _op(t["op"], float(base), d64)
                g = abs(float(base)) if t["op"] == SCALE else 1.0
                err = np.where(derr > 0, g * derr + (0.0 if t["op"] == ABS else HALF * np.abs(v64)), 0.0)
                slot = C_DAMP if t["target"] == DAMP else 4
            v64 = np.where(err > 0, v64, v32.astype(F64))          # an exact value IS its float32: what a later sum starts from
            if slot == C_DAMP:
                s.consts[C_DAMP][ap] = v32
            else:
                s.parts[slot - 4][ap] = v32
                touched_part |= ap
            s.v64[slot][ap], s.tol[slot][ap] = v64, err
    if touched_part.any():
        m = touched_part
        with np.errstate(all="ignore"):
            s.consts[C_MASS][m] = (s.parts[0][m] + s.parts[1][m]).astype(F32)
        e = s.tol[4][m] + s.tol[5][m]
        s.v64[C_MASS][m] = np.where(e > 0, s.v64[4][m] + s.v64[5][m], s.consts[C_MASS][m].astype(F64))
        s.tol[C_MASS][m] = np.where(e > 0, e + HALF * np.abs(s.v64[C_MASS][m]), 0.0)
    return s


def check(consts_words, block_words, want, what=""):
    """hold the four constant rows (uint32 [4, n]) and the block (uint32 [2 + 4 K, >= n]) of the device or the host program to a State:
    timers, counters and step words byte for byte; values byte for byte where tol == 0, else within tol of v64.  -> the largest
    error / tolerance ratio"""
    n, K = want.n, want.K
    blk = np.asarray(block_words, U32)[:, :n]
    for k in range(K):
        assert np.array_equal(blk[2 + 4 * k], want.tl[k].view(U32)), f"{what}: time_left of term {k}"
        assert np.array_equal(blk[3 + 4 * k], want.applied[k]), f"{what}: applied of term {k}"
        assert np.array_equal(blk[4 + 4 * k], want.w2[k]) and np.array_equal(blk[5 + 4 * k], want.w3[k]), f"{what}: step / drawn words of term {k}"
    got = np.concatenate([np.asarray(consts_words, U32)[:, :n], blk[0:2]])
    ref = np.concatenate([want.consts, want.parts]).view(U32)
    exact = want.tol == 0
    assert np.array_equal(got[exact], ref[exact]), f"{what}: exact values differ at {np.argwhere((got != ref) & exact)[:5].tolist()}"
    if exact.all():
        return 0.0
    g = got.view(F32).astype(F64)
    ratio = np.where(exact, 0.0, np.abs(g - want.v64) / np.where(exact, 1.0, want.tol))
    slot, env = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    where = f"row {('mu_s', 'mu_d', 'damp', 'mass', 'part_base', 'part_wheels')[slot]} of env {env}: {g[slot, env]!r} against {want.v64[slot, env]!r} +- {want.tol[slot, env]:.3g}"
    assert np.isfinite(g[~exact]).all() and (ratio <= 1.0).all(), f"{what}: off by up to {ratio.max():.3g} of the tolerance ({where})"
    check.worst = max(getattr(check, "worst", (0.0, "")), (float(ratio.max()), f"{what}: {where}"))
    return float(ratio.max())


# ---- the cases of the tests ----------------------------------------------------------------------------------------------------
FRICTION = dict(mu_s=(0.3, 0.9), mu_d=(0.2, 0.7), buckets=20, consistent=1)
CHASSIS = 3.0
EDGE_DT = F32(2.0 ** -30)                             # the timer edge: a step of 2^-30 s, so that timer and result share the binade of 1e-6
EDGE_T = F32(F32(1e-6) + EDGE_DT)                     # exact (both are multiples of 2^-43 below 2^-19): EDGE_T - EDGE_DT == float32(1e-6), NOT < 1e-6
EDGE_T_BELOW = np.nextafter(EDGE_T, F32(0))           # EDGE_T_BELOW - EDGE_DT is the float32 next below 1e-6: it fires


class Case:
    """tab; has_b / has_mask: whether reset_b / mask are passed at all; calls(n, rng) -> [dict(step, dt, ra, rb, mask, mask_terms)]"""

    def __init__(self, tab, calls, has_b=True, has_mask=False):
        self.tab, self.calls, self.has_b, self.has_mask = tab, calls, has_b, has_mask

    def initial(self, n, rng):
        """a state as the host layer leaves it: constants of a startup, parts that sum to the mass row bit for bit"""
        parts = np.stack([CHASSIS + rng.random(n) * 0.5, rng.random(n) * 0.4]).astype(F32)
        consts = np.stack([0.3 + 0.6 * rng.random(n), 0.2 + 0.5 * rng.random(n), 10 + 40 * rng.random(n), np.zeros(n)]).astype(F32)
        consts[C_MASS] = parts[0] + parts[1]
        return State(n, len(self.tab), consts, parts)


def _call(n, step, dt, ra=None, rb=None, mask=None, mask_terms=0):
    z = np.zeros(n, bool)
    return dict(step=int(step), dt=float(F32(dt)), ra=z if ra is None else np.asarray(ra, bool), rb=z if rb is None else np.asarray(rb, bool),
                mask=z if mask is None else np.asarray(mask, bool), mask_terms=int(mask_terms))


def _one_at_a_time(K):
    """every term forced alone, on every env, so that the rows show ITS value; then all at once"""
    def calls(n, rng):
        one = np.ones(n, bool)
        return [_call(n, 100 + k, 0.0, mask=one, mask_terms=1 << k) for k in range(K)] + [_call(n, 200, 0.0, mask=rng.random(n) < 0.5, mask_terms=(1 << K) - 1)]
    return calls


def cases():
    T, U, L, G = term, UNIFORM, LOG_UNIFORM, GAUSSIAN
    far = (50.0, 60.0)                                 # an interval no test reaches
    mu_reset = T(MU, RESET, **FRICTION)
    out = {}

    def flags(n, rng):
        one, r = np.ones(n, bool), lambda p: rng.random(n) < p
        return [_call(n, 3, 0.02),                                       # no flag set
                _call(n, 4, 0.02, ra=one, rb=one),                       # all flags set
                _call(n, 5, 0.02, rb=r(0.4)),                            # flags only in reset_b
                _call(n, 6, 0.02, ra=r(0.4), rb=r(0.3)),
                _call(n, 7, 0.02), _call(n, 8, 0.02, ra=r(0.2)), _call(n, (1 << 40) + 9, 0.02, rb=r(0.2))]
    tab3 = [mu_reset, T(DAMP, RESET, ABS, U, (10.0, 50.0)), T(MASS_BASE, INTERVAL, ADD, U, (0.3, 0.5), base=CHASSIS, interval=(0.05, 0.15))]
    out["flags"] = Case(tab3, flags)
    out["reset_b_null"] = Case(tab3, lambda n, rng: [_call(n, 3 + i, 0.02, ra=rng.random(n) < 0.4) for i in range(4)], has_b=False)
    out["mask_only"] = Case(tab3, lambda n, rng: [_call(n, 3, 0.0, mask=rng.random(n) < 0.5, mask_terms=7), _call(n, 4, 0.02, mask=rng.random(n) < 0.5, mask_terms=5),
                                                   _call(n, 5, 0.02, mask=np.ones(n, bool), mask_terms=0)], has_mask=True)
    # one term of each target, operation and distribution: damping and the chassis part in all nine combinations, the wheels in all three
    # distributions, friction in both modes
    pu, pl, pg = (10.0, 50.0), (5.0, 80.0), (30.0, 4.0)
    every1 = [T(DAMP, RESET, op, d, p, base=1.5) for op in (ADD, SCALE, ABS) for d, p in ((U, pu), (L, pl))] + [mu_reset, T(MASS_WHEELS, RESET, ABS, U, (0.03, 0.08))]
    every2 = [T(DAMP, INTERVAL, op, G, pg, base=1.5, interval=far) for op in (ADD, SCALE, ABS)] + [
        T(MASS_BASE, INTERVAL, ADD, U, (0.3, 0.5), base=CHASSIS, interval=far), T(MASS_BASE, RESET, SCALE, L, (0.8, 1.25), base=CHASSIS),
        T(MASS_BASE, INTERVAL, ABS, G, (3.2, 0.1), interval=far, global_time=1), T(MASS_WHEELS, INTERVAL, ABS, G, (0.05, 0.005), interval=far),
        T(MASS_WHEELS, RESET, ABS, L, (0.02, 0.09))]
    every3 = [T(MASS_BASE, RESET, ADD, L, (0.1, 0.9), base=CHASSIS), T(MASS_BASE, RESET, ADD, G, (0.4, 0.05), base=CHASSIS),
              T(MASS_BASE, RESET, SCALE, U, (0.9, 1.1), base=CHASSIS), T(MASS_BASE, RESET, SCALE, G, (1.0, 0.05), base=CHASSIS),
              T(MASS_BASE, RESET, ABS, U, (2.5, 3.5)), T(MASS_BASE, RESET, ABS, L, (2.5, 3.5)),
              T(MU, INTERVAL, interval=far, mu_s=(0.5, 0.5), mu_d=(0.1, 0.8), buckets=1, consistent=0)]
    for name, tab in (("every1", every1), ("every2", every2), ("every3", every3)):
        out[name] = Case(tab, _one_at_a_time(len(tab)), has_mask=True)
    # two terms on one target in one call: the interval term fires every call (its timer is one step long) and wins over the reset term
    # although it stands first in the table; of the two reset friction terms the later one wins
    same = [T(DAMP, INTERVAL, ABS, U, (30.0, 40.0), interval=(0.02, 0.02)), T(DAMP, RESET, ABS, U, (10.0, 20.0)), mu_reset,
            T(MU, RESET, mu_s=(1.0, 1.5), mu_d=(1.0, 1.2), buckets=3)]
    out["same_target"] = Case(same, lambda n, rng: [_call(n, 1, 0.02, ra=np.ones(n, bool)), _call(n, 2, 0.02, ra=rng.random(n) < 0.5)])
    # both mass parts, in different modes: the row is the sum of the parts
    parts = [T(MASS_BASE, RESET, ADD, U, (0.3, 0.5), base=CHASSIS), T(MASS_WHEELS, INTERVAL, ABS, U, (0.05, 0.1), interval=(0.03, 0.09))]
    out["mass_parts"] = Case(parts, lambda n, rng: [_call(n, 1 + i, 0.02, ra=rng.random(n) < 0.3, rb=rng.random(n) < 0.1) for i in range(8)])
    # min_step_count_between_reset = 5: never applied (step 10) -> applies; 4 steps later (count - 1) -> not; 5 steps later (count) -> applies
    ms = [T(DAMP, RESET, ABS, U, (10.0, 50.0), min_steps=5), T(MU, RESET, min_steps=5, **FRICTION)]

    def min_steps(n, rng):
        one, odd = np.ones(n, bool), np.arange(n) % 2 == 1
        return [_call(n, 10, 0.02, ra=one & ~odd), _call(n, 14, 0.02, ra=one), _call(n, 15, 0.02, rb=one), _call(n, 19, 0.02, ra=one), _call(n, (1 << 33) + 20, 0.02, ra=one)]
    out["min_steps"] = Case(ms, min_steps)
    # a timer that lands ON 1e-6 (does not fire: the comparison is <) next to one that lands on the float32 below it (fires)
    edge = [T(DAMP, INTERVAL, ABS, U, (10.0, 50.0), interval=(EDGE_T, EDGE_T)), T(MASS_BASE, INTERVAL, ADD, U, (0.3, 0.5), base=CHASSIS, interval=(EDGE_T_BELOW, EDGE_T_BELOW)),
            T(MU, INTERVAL, interval=(EDGE_T, EDGE_T), global_time=1, **FRICTION)]
    out["timer_edge"] = Case(edge, lambda n, rng: [_call(n, 0, 0.0)] + [_call(n, 1 + i, EDGE_DT) for i in range(4)])
    # one shared timer and one timer per env, with resets in between
    gl = [T(DAMP, INTERVAL, ABS, U, (10.0, 50.0), interval=(0.05, 0.1), global_time=1), T(MASS_BASE, INTERVAL, ADD, G, (0.4, 0.05), base=CHASSIS, interval=(0.05, 0.1)),
          T(MU, INTERVAL, interval=(0.03, 0.2), global_time=0, **FRICTION)]
    out["global_time"] = Case(gl, lambda n, rng: [_call(n, 0, 0.0)] + [_call(n, 1 + i, 0.02, ra=rng.random(n) < 0.25) for i in range(12)])
    # 20 consecutive calls, every kind of term, flags that change from call to call
    mix = [mu_reset, T(DAMP, RESET, SCALE, L, (0.5, 2.0), base=30.0, min_steps=3), T(MASS_BASE, INTERVAL, ADD, U, (0.3, 0.5), base=CHASSIS, interval=(0.04, 0.12)),
           T(MASS_WHEELS, RESET, ABS, G, (0.05, 0.005)), T(DAMP, INTERVAL, ADD, G, (0.0, 2.0), base=30.0, interval=(0.06, 0.06), global_time=1),
           T(MU, INTERVAL, interval=(0.02, 0.3), mu_s=(0.3, 0.9), mu_d=(0.2, 0.7), buckets=7), T(MASS_BASE, RESET, ABS, U, (2.8, 3.4), min_steps=2),
           T(MASS_WHEELS, INTERVAL, ABS, L, (0.02, 0.09), interval=(0.1, 0.2))]

    def lockstep(n, rng):
        r = lambda p: rng.random(n) < p
        return [_call(n, 50 + i, 0.02, ra=r(0.3 if i % 3 else 0.0), rb=r(0.1 if i % 4 else 0.9), mask=r(0.2 if i % 5 == 2 else 0.0), mask_terms=0xA5 if i % 2 else 0xFF)
                for i in range(20)]
    out["lockstep"] = Case(mix, lockstep, has_mask=True)
    return out


def run(case, st, calls, seed, env_offset, ez=EZ_DEVICE):
    """the states after each call"""
    out = []
    for c in calls:
        st = apply(case.tab, st, c["ra"], c["rb"] if case.has_b else None, c["mask"] if case.has_mask else None, c["mask_terms"], seed, c["step"],
                   c["dt"], env_offset, ez=ez)
        out.append(st)
    return out

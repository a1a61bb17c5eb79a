"""TEST INFRASTRUCTURE ONLY: the contract of include/wheeledlab_amd_latency.h in numpy over oracle/philox.py, stated twice -- vectorised
(push / finish on a State) and per env in plain Python over a collections.deque that a reset clears and whose first push fills it
(EnvDeque) -- plus the case list that the host program (tests/host_sim/action_latency_host.cpp) and the device
(tests/test_gpu_action_latency.py) both run.  Everything is integer draws and word copies: every comparison is byte for byte as uint32.

The one piece of arithmetic is the clamp of `finish`, the median of three (clampf of wl_math.h, v_med3_f32 on the device).  On ordinary
numbers, infinities, -0.0 and denormals it is the clamp; a quiet NaN comes out as -1 on the device and in the host stand-in alike
(the median of a set with a NaN is the minimum of the other two).  For a SIGNALLING NaN the answer is the platform's, not the body's:
the CDNA ISA manual defines V_MED3_F32 with a NaN operand as V_MIN3_F32 = min(min(x, -1), 1), and V_MIN_F32 in IEEE mode (the mode of a
compute kernel) returns a signalling operand QUIETED, so min(sNaN, -1) is a quiet NaN and min(that, 1) = +1: SNAN_DEVICE.  The host
stand-in builds the median from libm's fmin / fmax, whose answer for a signalling NaN depends on whether the compiler inlines them;
the CPU test asks the stand-in's own function (not the body under test) and passes the answer in as `snan`."""
import collections
from dataclasses import dataclass

import numpy as np

from oracle import philox

CAP = 16
HEAD_ROWS = 5
STREAM = 20
ONE, MINUS_ONE = np.float32(1.0).view(np.uint32), np.float32(-1.0).view(np.uint32)
SNAN_DEVICE = ONE
S_ACT0 = 19            # WL_S_ACT0 of include/wheeledlab_amd.h (the tests check it against the header)


def width(max_delay):
    return -1 if not 0 <= max_delay <= CAP else HEAD_ROWS + 2 * (max_delay + 1)


@dataclass(frozen=True)
class P:
    """the parameters of a layer"""
    lo: int
    hi: int
    per: bool = False

    @property
    def slots(self):
        return self.hi + 1


def draw_lags(env_ids, drawn, seed, p):
    """-> uint32 [2, n]: the lags of envs `env_ids` (global ids, uint32) on their draw number `drawn`"""
    env_ids, drawn = np.asarray(env_ids, np.uint32), np.asarray(drawn, np.uint32)
    w = np.zeros((4, env_ids.size), np.uint32)
    for d in np.unique(drawn):
        m = drawn == d
        w[:, m] = philox.philox4x32(env_ids[m], int(d), STREAM, seed)
    span = p.hi - p.lo + 1
    u = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    pick = np.minimum((u * np.float32(span)).astype(np.float32).astype(np.int64), span - 1)
    lag = (p.lo + pick).astype(np.uint32)
    return np.stack([lag[0], lag[1] if p.per else lag[0]])


def clamp_words(w, snan=SNAN_DEVICE):
    """the median of (x, -1, 1) on float32 words (module docstring)"""
    w = np.asarray(w, np.uint32)
    f = w.view(np.float32)
    nan = np.isnan(f)
    with np.errstate(invalid="ignore"):
        out = np.where(f < np.float32(-1), MINUS_ONE, np.where(f > np.float32(1), ONE, w)).astype(np.uint32)
    quiet = (w & np.uint32(0x00400000)) != 0
    out[nan & quiet] = MINUS_ONE
    out[nan & ~quiet] = snan
    return out


@dataclass
class State:
    """the layer block of n envs"""
    n: int
    p: P
    lag: np.ndarray = None
    pushes: np.ndarray = None
    head: np.ndarray = None
    drawn: np.ndarray = None
    ring: np.ndarray = None        # [slots, 2, n]

    def __post_init__(self):
        z = lambda *s: np.zeros(s, np.uint32)
        if self.lag is None:
            self.lag, self.pushes, self.head, self.drawn, self.ring = z(2, self.n), z(self.n), z(self.n), z(self.n), z(self.p.slots, 2, self.n)

    def copy(self):
        return State(self.n, self.p, self.lag.copy(), self.pushes.copy(), self.head.copy(), self.drawn.copy(), self.ring.copy())

    def block(self, stride, fill=0):
        """uint32 [width, stride]: rows lag0, lag1, pushes, head, drawn, then slot s component c at 5 + 2 s + c"""
        b = np.full((width(self.p.hi), stride), fill, np.uint32)
        b[0:2, :self.n], b[2, :self.n], b[3, :self.n], b[4, :self.n] = self.lag, self.pushes, self.head, self.drawn
        b[HEAD_ROWS:, :self.n] = self.ring.reshape(-1, self.n)
        return b


def push(st, action):
    """action uint32 [n, 2] -> (the state after the push, applied uint32 [n, 2])"""
    st, slots, e = st.copy(), st.p.slots, np.arange(st.n)
    a = np.asarray(action, np.uint32).T                     # [2, n]
    first = st.pushes == 0
    st.ring[:, :, first] = a[None, :, first]
    st.head = np.where(first, 0, (st.head + 1) % slots).astype(np.uint32)
    st.ring[st.head[~first], :, e[~first]] = a[:, ~first].T
    st.pushes = np.where(first, 1, np.minimum(st.pushes + 1, slots)).astype(np.uint32)
    back = np.minimum(st.lag, st.pushes - 1)                # [2, n]
    slot = (st.head[None, :] + slots - back) % slots
    applied = np.stack([st.ring[slot[c], c, e] for c in (0, 1)], axis=1)
    return st, applied


def finish(st, action, act_rows, row, col, reset, clip_wrapper, seed, env_offset, snan=SNAN_DEVICE):
    """action uint32 [n, 2]; act_rows uint32 [2, n] (WL_S_ACT0/1); row uint32 [n, pitch] or None; reset bool [n] -> (state, act_rows, row)"""
    st, act_rows, reset = st.copy(), act_rows.copy(), np.asarray(reset, bool)
    row = None if row is None else row.copy()
    ids = (np.uint64(env_offset) + np.arange(st.n, dtype=np.uint64)).astype(np.uint32)
    if reset.any():
        st.lag[:, reset] = draw_lags(ids[reset], st.drawn[reset], seed, st.p)
        st.pushes[reset] = 0
        st.drawn[reset] += np.uint32(1)
    s = np.asarray(action, np.uint32).T
    s = clamp_words(s, snan) if clip_wrapper else s
    act_rows[:, ~reset] = s[:, ~reset]
    if row is not None and col >= 0:
        row[~reset, col:col + 2] = clamp_words(s, snan).T[~reset]
    return st, act_rows, row


class EnvDeque:
    """one env, in plain Python: IsaacLab's DelayBuffer over a CircularBuffer of max_delay + 1 actions"""

    def __init__(self, env_id, p, seed):
        self.id, self.p, self.seed = int(env_id) & 0xFFFFFFFF, p, seed
        self.dq = collections.deque(maxlen=p.slots)
        self.lag, self.pushes, self.drawn = [0, 0], 0, 0

    def reset(self):
        self.dq.clear()
        self.pushes = 0
        w = [int(x) for x in philox.philox4x32(np.array([self.id], np.uint32), self.drawn, STREAM, self.seed)[:, 0]]
        span = self.p.hi - self.p.lo + 1
        lag = [self.p.lo + min(int(np.float32(np.float32((x >> 8)) * np.float32(2.0 ** -24)) * np.float32(span)), span - 1) for x in w]
        self.lag = [lag[0], lag[1] if self.p.per else lag[0]]
        self.drawn += 1

    def push(self, a):
        """a: the action's two words -> the applied action's two words"""
        a = (int(a[0]), int(a[1]))
        if not self.dq:                                    # the first push after a reset fills the buffer
            self.dq.extend([a] * self.p.slots)
        else:
            self.dq.append(a)
        self.pushes = min(self.pushes + 1, self.p.slots)
        return tuple(self.dq[-1 - min(self.lag[c], self.pushes - 1)][c] for c in (0, 1))


# ---- the case list ---------------------------------------------------------------------------------------------------------

QNAN = [0x7FC00001, 0xFFC12345, 0x7FFFFFFF]
SNAN = [0x7F800001, 0xFF812345, 0x7FBFFFFF]
SPECIALS = QNAN + SNAN + [0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000,     # -0, 0, inf, -inf, denormals
                          0x3F800000, 0xBF800000, 0x3F800001, 0xBF800001, 0x40490FDB, 0xC0490FDB, 0x3F000000]     # +-1, just beyond, +-pi, 0.5


def random_actions(rng, n, specials=False):
    """uint32 [n, 2]: normal actions of scale 2 (a good part beyond +-1); specials: every entry one of SPECIALS in turn, shuffled"""
    if not specials:
        return (rng.standard_normal((n, 2)) * 2).astype(np.float32).view(np.uint32)
    w = np.array(SPECIALS, np.uint32)[(np.arange(2 * n) + rng.integers(0, len(SPECIALS))) % len(SPECIALS)]
    return rng.permutation(w).reshape(n, 2)


@dataclass
class Case:
    p: P
    clip_wrapper: int = 0
    pitch: int = 14
    col: int = 12
    has_b: bool = True
    flags: str = "random"          # none | all | b_only | random
    pairs: int = 4
    specials: bool = False

    def with_p(self, p):
        return Case(p, self.clip_wrapper, self.pitch, self.col, self.has_b, self.flags, self.pairs, self.specials)

    def calls(self, n, rng):
        """the operations: a finish with every flag set (env.reset()), then `pairs` push / finish pairs.  -> [dict(kind, action, ra, rb)]"""
        z = np.zeros(n, bool)
        ops = [dict(kind="finish", action=np.zeros((n, 2), np.uint32), ra=np.ones(n, bool), rb=z.copy())]
        for k in range(self.pairs):
            a = random_actions(rng, n, self.specials)
            ra, rb = z.copy(), z.copy()
            if self.flags == "all":
                ra[:] = True
            elif self.flags == "b_only":
                rb = rng.random(n) < 0.5
            elif self.flags == "random":                  # about one reset per env every 5 steps: they fall at every ring position
                ra, rb = rng.random(n) < 0.12, rng.random(n) < 0.1
            if not self.has_b:
                rb = z.copy()
            ops += [dict(kind="push", action=a, ra=z, rb=z), dict(kind="finish", action=a, ra=ra, rb=rb)]
        return ops


def cases():
    c = {"no_flag": Case(P(0, 3), flags="none"),
         "all_flags": Case(P(0, 3, True), flags="all"),
         "flags_in_b": Case(P(1, 2), flags="b_only"),
         "b_null": Case(P(0, 3), has_b=False),
         "col_none": Case(P(1, 3), col=-1),
         "specials_raw": Case(P(1, 1), specials=True, pairs=5),
         "specials_clip": Case(P(0, 2, True), clip_wrapper=1, specials=True, pairs=5),
         "clip": Case(P(0, 3), clip_wrapper=1),
         "lockstep": Case(P(0, 3, True), pairs=20)}
    for k in range(4):                                      # the column at each place of a 16-byte line (rows of 12 words: 48 bytes)
        c[f"col_at_{k}"] = Case(P(0, 2), pitch=12, col=4 + k)
    return c


DELAYS = [(0, 0), (1, 1), (0, 3), (CAP, CAP)]


@dataclass
class Snap:
    st: State
    applied: np.ndarray
    act_rows: np.ndarray
    row: np.ndarray


def run(case, st, act_rows, row, ops, seed, env_offset, snan=SNAN_DEVICE):
    """-> [Snap] after every operation; `applied` is the last push's (zeros before the first)"""
    out, applied = [], np.zeros((st.n, 2), np.uint32)
    for op in ops:
        if op["kind"] == "push":
            st, applied = push(st, op["action"])
        else:
            st, act_rows, new_row = finish(st, op["action"], act_rows, row if case.col >= 0 else None, case.col, op["ra"] | op["rb"],
                                           case.clip_wrapper, seed, env_offset, snan)
            row = row if new_row is None else new_row
        out.append(Snap(st, applied.copy(), act_rows.copy(), None if row is None else row.copy()))
    return out

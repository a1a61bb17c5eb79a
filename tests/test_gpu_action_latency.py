"""GPU: the two action-latency launches (csrc/wl_action_latency.hip) against the reference (tests/action_latency_reference.py) -- the
kernels alone, through ctypes, on guarded buffers.  Everything is integer draws and word copies: every comparison is byte for byte as
uint32.  Every state row other than WL_S_ACT0/1, every row column other than last_action, the padding of every block row and the
policy's action itself are compared with a copy taken before the call; every buffer sits between guard rows of NaN words; every launch
is synchronised and its status checked.

Shapes: n in {1, 63, 64, 65, 130} at strides 64, 64, 64, 128, 192 -- one lane, a wavefront less one, a full one, one more, and a
count that is no multiple of anything with two rows of padding."""
import numpy as np
import pytest
import torch

from tests import action_latency_reference as R
from tests.test_action_latency_cpu import check_snapshot, words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7FC0BEEF
SHAPES = [(1, 64), (63, 64), (64, 64), (65, 128), (130, 192)]
CASES = R.cases()
SEED = 0x0123_4567_89AB_CDEF


def _lib():
    from wheeledlab_amd import _abi as A
    return A, A.load()


def _flags(x):
    return torch.from_numpy(np.ascontiguousarray(x, bool).copy()).to(DEV)


class Guarded:
    """words of any shape on the device between two guard regions of NaN words (each at least 256 bytes, a multiple of 16)"""

    def __init__(self, w):
        self.shape, g = w.shape, max(64, 2 * w.shape[-1] + (-2 * w.shape[-1]) % 4)
        self.g = g
        self.buf = torch.full((g + w.size + g,), GUARD, dtype=torch.int32, device=DEV)
        self.buf[g:g + w.size] = torch.from_numpy(w.reshape(-1).view(np.int32).copy()).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * g

    def write(self, w):
        self.buf[self.g:self.g + w.size] = torch.from_numpy(np.ascontiguousarray(w, np.uint32).reshape(-1).view(np.int32).copy()).to(DEV)

    def read(self):
        w = self.buf.cpu().numpy().view(np.uint32)
        assert (w[:self.g] == GUARD).all() and (w[-self.g:] == GUARD).all(), "a guard word changed"
        return w[self.g:-self.g].reshape(self.shape).copy()


class Launch:
    """one case on the device: the state matrix, the row, the block and `applied` live there from operation to operation, every
    operation held to the reference"""

    def __init__(self, case, n, stride, rng, env_offset=0):
        self.A, self.lib = _lib()
        A = self.A
        self.case, self.n, self.stride, self.env_offset = case, n, stride, env_offset
        assert self.lib.wl_action_latency_width(case.p.hi) == R.width(case.p.hi)
        block = R.State(n, case.p).block(stride, fill=0xDEADBEEF)
        block[:, :n] = 0
        s, r = words(rng, A.S_COUNT, stride), words(rng, n, case.pitch)
        self.state, self.row, self.block = Guarded(s), Guarded(r), Guarded(block)
        self.applied, self.action = Guarded(np.zeros((n, 2), np.uint32)), Guarded(np.zeros((n, 2), np.uint32))
        assert self.row.ptr % 16 == 0                      # (col_at_k: the column's place in a 16-byte line is what the case says)
        self.stream = A.stream(torch.device(DEV))
        self.ref = R.Snap(R.State(n, case.p), np.zeros((n, 2), np.uint32), s[A.S_ACT0:A.S_ACT1 + 1, :n].copy(), r.copy())

    def op(self, o, k=0):
        n, case, p = self.n, self.case, self.case.p
        self.action.write(o["action"])
        s0, r0, b0 = self.state.read(), self.row.read(), self.block.read()
        if o["kind"] == "push":
            rc = self.lib.wl_action_latency_push(n, self.action.ptr, self.applied.ptr, self.block.ptr, self.stride, p.hi, self.stream)
        else:
            ra, rb = _flags(o["ra"]), _flags(o["rb"]) if case.has_b else None
            rc = self.lib.wl_action_latency_finish(n, self.action.ptr, self.state.ptr, self.stride, self.row.ptr if case.col >= 0 else None, case.pitch,
                                                   case.col, self.block.ptr, ra.data_ptr(), None if rb is None else rb.data_ptr(), p.lo, p.hi, int(p.per),
                                                   case.clip_wrapper, SEED, self.env_offset, self.stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        want = R.run(case, self.ref.st, self.ref.act_rows, self.ref.row, [o], SEED, self.env_offset)[0]
        if o["kind"] == "finish":
            want.applied = self.ref.applied                # (a finish leaves `applied` alone)
        got = (self.applied.read(), self.state.read(), self.row.read(), self.block.read())
        assert np.array_equal(self.action.read(), o["action"])                                  # the policy's tensor is untouched
        check_snapshot(f"n={n} op {k} ({o['kind']})", n, case, want, *got, s0, r0, b0)
        self.ref = want
        return got


@pytest.mark.parametrize("n,stride", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_reference_and_write_nothing_else(name, n, stride):
    case = CASES[name]
    rng = np.random.default_rng(n * 7 + len(name))
    L = Launch(case, n, stride, rng, env_offset=11)
    for k, o in enumerate(case.calls(n, rng)):
        applied, _, _, _ = L.op(o, k)
        if case.specials and o["kind"] == "push":          # NaN payloads, -0.0, infinities and denormals arrive as they left
            assert set(applied.ravel().tolist()) <= set(R.SPECIALS) | {0}


@pytest.mark.parametrize("n,stride", SHAPES)
@pytest.mark.parametrize("lo,hi", R.DELAYS)
@pytest.mark.parametrize("per", [False, True])
def test_every_delay_range_shared_and_per_component(lo, hi, per, n, stride):
    case = CASES["lockstep"].with_p(R.P(lo, hi, per))
    case.pairs = 8 if hi < R.CAP else 2 * R.CAP + 4        # (the cap: long enough for the ring to wrap)
    rng = np.random.default_rng(n + 13 * hi + per)
    L = Launch(case, n, stride, rng, env_offset=(1 << 32) - 3)
    for k, o in enumerate(case.calls(n, rng)):
        applied, _, _, block = L.op(o, k)
        if lo == hi == 0 and o["kind"] == "push":          # zero lag: applied is the policy's action
            assert np.array_equal(applied, o["action"])
    lag = block[0:2, :n]
    assert lag.min() >= lo and lag.max() <= hi and (per or np.array_equal(lag[0], lag[1]))


def test_sharding_two_launches_of_65_equal_one_of_130_byte_for_byte():
    case = CASES["lockstep"]
    ops = case.calls(130, np.random.default_rng(9))
    whole = Launch(case, 130, 192, np.random.default_rng(11), env_offset=0)
    a, b = Launch(case, 65, 128, np.random.default_rng(12), env_offset=0), Launch(case, 65, 128, np.random.default_rng(13), env_offset=65)
    for k, o in enumerate(ops):
        aw, _, _, bw = whole.op(o, k)
        parts = [sh.op(dict(o, action=o["action"][lo:lo + 65], ra=o["ra"][lo:lo + 65], rb=o["rb"][lo:lo + 65]), k) for sh, lo in ((a, 0), (b, 65))]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), aw)
        assert np.array_equal(np.concatenate([p[3][:, :65] for p in parts], axis=1), bw[:, :130])


def test_bad_arguments_return_their_code_and_launch_nothing():
    A, lib = _lib()
    n, stride, D, pitch, col = 130, 192, 3, 14, 12
    rows = R.width(D)
    rng = np.random.default_rng(2)
    state, row, block = Guarded(words(rng, A.S_COUNT, stride)), Guarded(words(rng, n, pitch)), Guarded(words(rng, rows, stride))
    action, applied = Guarded(words(rng, n, 2)), Guarded(words(rng, n, 2))
    flags = torch.ones(2, 256, dtype=torch.uint8, device=DEV)
    before = [g.read() for g in (state, row, block, action, applied)]
    base = dict(n=n, action=action.ptr, applied=applied.ptr, state=state.ptr, stride=stride, row=row.ptr, pitch=pitch, col=col, block=block.ptr,
                ra=flags[0].data_ptr(), rb=flags[1].data_ptr(), lo=1, hi=D, per=1, clip=0)
    stream = A.stream(torch.device(DEV))

    def push(**kw):
        a = {**base, **kw}
        return lib.wl_action_latency_push(a["n"], a["action"], a["applied"], a["block"], a["stride"], a["hi"], stream)

    def finish(**kw):
        a = {**base, **kw}
        return lib.wl_action_latency_finish(a["n"], a["action"], a["state"], a["stride"], a["row"], a["pitch"], a["col"], a["block"], a["ra"], a["rb"],
                                            a["lo"], a["hi"], a["per"], a["clip"], SEED, 0, stream)
    for k in ("action", "applied", "block"):
        assert push(**{k: None}) == -1, k
    for k in ("action", "state", "block", "ra", "row"):
        assert finish(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(n=-1), dict(stride=128), dict(hi=R.CAP + 1, lo=0), dict(hi=-1, lo=-1)):
        assert push(**kw) == -1 and finish(**kw) == -1, kw
    for kw in (dict(lo=D + 1), dict(lo=-1), dict(per=2), dict(clip=-1), dict(pitch=0), dict(col=-2), dict(col=pitch - 1)):
        assert finish(**kw) == -1, kw
    assert push(stride=130) == -3 and finish(stride=193) == -3
    assert push(applied=base["applied"] + 2) == -3 and finish(row=base["row"] + 2) == -3 and finish(state=base["state"] + 1) == -3
    acts = state.ptr + A.S_ACT0 * stride * 4
    for kw in (dict(applied=base["action"]), dict(applied=base["action"] + 8), dict(applied=base["block"] + 64), dict(action=base["block"])):
        assert push(**kw) == -1, kw
    for kw in (dict(block=acts), dict(row=acts + 8), dict(action=acts), dict(ra=acts + 4), dict(rb=block.ptr + 64), dict(action=row.ptr), dict(row=block.ptr)):
        assert finish(**kw) == -1, kw
    torch.cuda.synchronize()
    for g, w in zip((state, row, block, action, applied), before):
        assert np.array_equal(g.read(), w)                                                        # nothing was launched
    assert bool((flags == 1).all())

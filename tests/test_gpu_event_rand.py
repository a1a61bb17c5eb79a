"""GPU: the per-episode domain randomisation launch (csrc/wl_event_rand.hip) against the reference (tests/event_rand_reference.py) --
the kernel alone, through ctypes, on guarded buffers.  Held to: byte for byte (uint32) on timers, counters, step words, bucket
materials, every uniform value and what the operations make of it; a Gaussian or log_uniform value against its float64 value within
the tolerance the reference derives (EZ_DEVICE of tests/obs_corrupt_reference.py for the Box-Muller normal, EXP_HW for v_exp_f32 --
nothing in either comes from the kernel's output; the largest error seen is printed for DESIGN section 21).  Every row the launch
does not own is compared byte for byte with a copy made before the call, every launch is synchronised and its status checked.

Shapes: n in {1, 63, 64, 65, 130} at strides 64, 64, 64, 128, 192 -- one lane, a wavefront less one, a full one, one more, and a
count that is no multiple of anything with two rows of padding."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import event_rand_reference as R
from tests.test_event_rand_cpu import _bad_tables, check_untouched, state_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7FC0BEEF
SHAPES = [(1, 64), (63, 64), (64, 64), (65, 128), (130, 192)]
CASES = R.cases()
SEED = 0x0123_4567_89AB_CDEF


def _lib():
    from wheeledlab_amd import _abi as A
    return A, A.load()


def _ctable(A, tab):
    rows = R.rows(tab)
    return (A.WlEventRandTerm * len(rows))(*[A.WlEventRandTerm(*r) for r in rows])


def _flags(x):
    return torch.from_numpy(np.ascontiguousarray(x, bool).copy()).to(DEV)


class Guarded:
    """words [rows, stride] on the device between two guard regions"""

    def __init__(self, words):
        self.shape, g = words.shape, 2 * words.shape[1]
        self.g = g
        self.buf = torch.full((g + words.size + g,), GUARD, dtype=torch.int32, device=DEV)
        self.buf[g:g + words.size] = torch.from_numpy(words.reshape(-1).view(np.int32).copy()).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * g

    def read(self):
        w = self.buf.cpu().numpy().view(np.uint32)
        assert (w[:self.g] == GUARD).all() and (w[-self.g:] == GUARD).all(), "a guard word changed"
        return w[self.g:-self.g].reshape(self.shape).copy()


class Launch:
    """one case on the device: the state matrix and the block live there from call to call, every call held to the reference"""

    def __init__(self, case, n, stride, rng, env_offset=0, init=None):
        self.A, self.lib = _lib()
        self.case, self.n, self.stride, self.env_offset = case, n, stride, env_offset
        self.ct, self.K = _ctable(self.A, case.tab), len(case.tab)
        assert self.lib.wl_event_rand_width(self.ct, self.K) == 2 + 4 * self.K
        self.ref = case.initial(n, rng) if init is None else init
        block = self.ref.block(stride)
        block[:, n:] = 0xDEADBEEF
        self.state, self.block = Guarded(state_words(rng, self.ref, stride)), Guarded(block)
        self.stream = self.A.stream(torch.device(DEV))
        self.worst = 0.0

    def call(self, c):
        A, n = self.A, self.n
        s0, b0 = self.state.read(), self.block.read()
        ra, rb, mask = _flags(c["ra"]), _flags(c["rb"]) if self.case.has_b else None, _flags(c["mask"]) if self.case.has_mask else None
        rc = self.lib.wl_event_rand_apply(n, self.state.ptr, self.stride, self.ct, self.K, self.block.ptr, ra.data_ptr(), None if rb is None else rb.data_ptr(),
                                          None if mask is None else mask.data_ptr(), c["mask_terms"], SEED, c["step"], c["dt"], self.env_offset, self.stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        s1, b1 = self.state.read(), self.block.read()
        want = R.run(self.case, self.ref, [c], SEED, self.env_offset)[0]
        check_untouched(s0, b0, s1, b1, n)
        consts = slice(A.S_MU_S, A.S_MASS + 1)
        self.worst = max(self.worst, R.check(s1[consts], b1, want, what=f"n={n} step={c['step']}"))
        quiet = ~want.fired.any(0)
        assert np.array_equal(s1[consts, :n][:, quiet], s0[consts, :n][:, quiet])               # nothing applied: nothing stored
        assert np.array_equal(b1[0:2, :n][:, quiet], b0[0:2, :n][:, quiet])
        self.ref = want
        return s1, b1, want


@pytest.mark.parametrize("n,stride", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_reference_and_writes_nothing_else(name, n, stride):
    case = CASES[name]
    rng = np.random.default_rng(n * 7 + len(name))
    L = Launch(case, n, stride, rng, env_offset=11)
    A = L.A
    for c in case.calls(n, rng):
        s1, b1, want = L.call(c)
        if name == "mass_parts":                                  # the row is the sum of the parts, on the device's own words
            parts = b1[0:2, :n].view(np.float32)
            assert np.array_equal(s1[A.S_MASS, :n], (parts[0] + parts[1]).astype(np.float32).view(np.uint32))
        if name == "same_target" and c["step"] == 1:              # the interval term wins over the reset term, the later friction term over the earlier
            damp, mu_s = s1[A.S_DAMP, :n].view(np.float32), s1[A.S_MU_S, :n].view(np.float32)
            assert ((damp >= 30) & (damp <= 40)).all() and (mu_s >= 1.0).all() and want.fired.all()
        if name == "timer_edge" and c["step"] == 1:               # ON 1e-6: not fired; the float32 below: fired
            assert (b1[2, :n] == np.float32(1e-6).view(np.uint32)).all() and (b1[3, :n] == 0).all() and (b1[3 + 4, :n] == 1).all()
    if name in ("flags", "reset_b_null", "mask_only", "same_target", "mass_parts", "min_steps", "timer_edge"):
        assert L.worst == 0.0                                      # uniform draws only: nothing is approximate
    print(f"\nEVENTRAND kernel {name} n={n}: largest error / tolerance {L.worst:.4f}; the largest so far: {getattr(R.check, 'worst', (0.0, ''))}")


def test_min_step_count_at_count_minus_one_at_count_and_never_applied():
    case, n = CASES["min_steps"], 130
    rng = np.random.default_rng(1)
    L = Launch(case, n, 192, rng)
    even = np.arange(n) % 2 == 0
    fired = [L.call(c)[2].fired[0] for c in case.calls(n, rng)]
    applied = L.block.read()[3, :n]
    # step 10 (never applied) -> 14 (count - 1: refused) -> 15 (count: applied) -> 19 (refused) -> far later (applied)
    assert [bool(f[even].all()) for f in fired] == [True, False, True, False, True] and not fired[1][even].any()
    assert [bool(f[~even].all()) for f in fired] == [False, True, False, True, True] and not fired[2][~even].any()
    assert (applied == 3).all()


def test_sharding_two_calls_of_65_equal_one_of_130_byte_for_byte():
    case = CASES["lockstep"]
    rng = np.random.default_rng(9)
    calls = case.calls(130, rng)
    init = case.initial(130, np.random.default_rng(10))
    whole = Launch(case, 130, 192, np.random.default_rng(11), env_offset=0, init=init)

    def shard(lo):
        sub = R.State(65, len(case.tab), init.consts[:, lo:lo + 65], init.parts[:, lo:lo + 65])
        return Launch(case, 65, 128, np.random.default_rng(12 + lo), env_offset=lo, init=sub)
    a, b = shard(0), shard(65)
    A = whole.A
    consts = slice(A.S_MU_S, A.S_MASS + 1)
    for c in calls:
        sw, bw, _ = whole.call(c)
        parts = [sh.call(dict(c, ra=c["ra"][lo:lo + 65], rb=c["rb"][lo:lo + 65], mask=c["mask"][lo:lo + 65])) for sh, lo in ((a, 0), (b, 65))]
        assert np.array_equal(np.concatenate([p[0][consts, :65] for p in parts], axis=1), sw[consts, :130])
        assert np.array_equal(np.concatenate([p[1][:, :65] for p in parts], axis=1), bw[:, :130])


@pytest.mark.parametrize("which", ["visual", "drift"])
def test_startup_tie_the_part_rows_sum_to_the_startup_mass_row_bit_for_bit(which):
    from wheeledlab_amd.core import apply_startup_events
    from wheeledlab_amd.envs.events import EventRandomizer, EventTable
    from wheeledlab_amd.envs.flatten import StartupSpec
    A, lib = _lib()
    su = {"visual": StartupSpec(wheel_mu_s=(0.4, 0.6), wheel_mu_d=(0.4, 0.6), mu_buckets=10, mu_consistent=False, damping=(1000.0, 1000.0), chassis_mass=0.0,
                                mass_add=(1.0, 3.0), wheel_mass=(0.01, 0.3)),
          "drift": StartupSpec(wheel_mu_s=(0.3, 0.5), wheel_mu_d=(0.3, 0.5), mu_buckets=20, mu_consistent=True, damping=(10.0, 50.0), mass_add=(0.3, 0.5))}[which]
    for n, stride, off in ((130, 192, 0), (65, 128, 65), (1, 64, 7)):
        state = torch.zeros(A.S_COUNT, stride, dtype=torch.float32, device=DEV)
        bufs = A.WlEnvBuffers(state.data_ptr(), None, None, None, stride, n, off, 1, 0, 0)
        apply_startup_events(lib, bufs, su, 42, A.stream(torch.device(DEV)))
        batch = SimpleNamespace(n=n, stride=stride, state=state, seed=42, env_offset=off, step_count=0)
        table = EventTable((tuple(R.rows([R.term(R.MASS_BASE, R.RESET, R.ADD, R.UNIFORM, (0.3, 0.5), base=su.chassis_mass)])[0]),), ("add_base_mass",))
        before = state.clone()
        layer = EventRandomizer(table, batch, su, 0.02)
        torch.cuda.synchronize()
        assert torch.equal(state, before)                                                        # building the layer changes no row of the state
        pb, pw = layer.part_base.cpu().numpy(), layer.part_wheels.cpu().numpy()
        mass = state[A.S_MASS, :n].cpu().numpy()
        assert np.array_equal((pb + pw).astype(np.float32).view(np.uint32), mass.view(np.uint32))
        assert (pw > 0).all() if which == "visual" else (pw == 0).all()
        assert (pb >= su.chassis_mass + su.mass_add[0]).all() and (pb <= np.float32(su.chassis_mass + su.mass_add[1])).all()


def test_bad_arguments_return_their_code_and_launch_nothing():
    A, lib = _lib()
    good, bads = _bad_tables()
    n, stride, K = 130, 192, len(good)
    rows = 2 + 4 * K
    rng = np.random.default_rng(2)
    init = R.Case(good, None).initial(n, rng)
    state, block = Guarded(state_words(rng, init, stride)), Guarded(rng.integers(0, 1 << 32, size=(rows, stride), dtype=np.uint64).astype(np.uint32))
    flags = torch.ones(3, 256, dtype=torch.uint8, device=DEV)
    s0, b0 = state.read(), block.read()
    base = dict(n=n, state=state.ptr, stride=stride, terms=_ctable(A, good), n_terms=K, block=block.ptr, ra=flags[0].data_ptr(), rb=flags[1].data_ptr(),
                mask=flags[2].data_ptr(), mask_terms=(1 << K) - 1, dt=0.02)

    def apply(**kw):
        a = {**base, **kw}
        return lib.wl_event_rand_apply(a["n"], a["state"], a["stride"], a["terms"], a["n_terms"], a["block"], a["ra"], a["rb"], a["mask"], a["mask_terms"],
                                       SEED, 7, a["dt"], 0, A.stream(torch.device(DEV)))
    for k in ("state", "block", "ra", "terms"):
        assert apply(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(n=-1), dict(stride=128), dict(n_terms=0), dict(n_terms=9), dict(mask_terms=1 << K), dict(dt=-0.02), dict(dt=float("nan"))):
        assert apply(**kw) == -1, kw
    for what, tab in bads:
        assert apply(terms=_ctable(A, tab)) == -1, what
    assert apply(stride=130) == -3 and apply(stride=193) == -3
    for k in ("state", "block"):
        assert apply(**{k: base[k] + 2}) == -3, k
    consts = state.ptr + A.S_MU_S * stride * 4
    for kw in (dict(block=consts), dict(block=consts + (3 * stride + n) * 4 - 4), dict(ra=consts + 8), dict(rb=block.ptr + 64), dict(mask=block.ptr + ((rows - 1) * stride + n) * 4 - 1)):
        assert apply(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(state.read(), s0) and np.array_equal(block.read(), b0) and bool((flags == 1).all())      # nothing was launched

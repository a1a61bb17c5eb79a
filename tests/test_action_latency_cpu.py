"""CPU checks of the action-latency layer: the reference's two statements against each other and on hand cases, the lag draws' statistics,
the header and its ctypes mirror, wl_action_latency_width and every argument refusal of the two launches before any launch,
envs/latency.resolve on configs (None for every shipped config, every refusal, dict overrides through the training script's path), and
the per-env bodies compiled for the host as a stand-alone program (tests/host_sim/action_latency_host.cpp) -- plain and under
-fsanitize=address,undefined -- against the reference (tests/action_latency_reference.py) over the case list the GPU test runs.

Everything is integer draws and word copies: every comparison is byte for byte as uint32."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import action_latency_reference as R
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_latency.h")
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(ROOT, "tests", "host_sim", "action_latency_host.cpp")
CASES = R.cases()
SEED = 0x0123_4567_89AB_CDEF
STAT_SEED = 2026           # the statistics test's seed: chosen so that the reference passes, here on the CPU


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


# ---- the reference holds itself ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [R.P(0, 3), R.P(0, 3, True), R.P(2, 2), R.P(1, R.CAP, True)])
def test_the_vectorised_and_the_per_env_statement_agree_over_40_steps_of_random_resets(p):
    n, off = 37, (1 << 32) - 5                         # (ids wrap through 2^32)
    rng = np.random.default_rng(p.hi * 3 + p.per)
    envs = [R.EnvDeque(off + e, p, SEED) for e in range(n)]
    st = R.State(n, p)
    act, dummy = np.zeros((2, n), np.uint32), None
    st, act, _ = R.finish(st, np.zeros((n, 2), np.uint32), act, dummy, -1, np.ones(n, bool), 0, SEED, off)
    for d in envs:
        d.reset()
    for _ in range(40):
        a = R.random_actions(rng, n)
        st, applied = R.push(st, a)
        assert np.array_equal(applied, np.array([d.push(a[e]) for e, d in enumerate(envs)], np.uint32))
        reset = rng.random(n) < 0.15
        st, act, _ = R.finish(st, a, act, dummy, -1, reset, 0, SEED, off)
        for e in np.flatnonzero(reset):
            envs[e].reset()
        assert np.array_equal(st.lag, np.array([d.lag for d in envs], np.uint32).T)
        assert np.array_equal(st.pushes, [d.pushes for d in envs]) and np.array_equal(st.drawn, [d.drawn for d in envs])
        assert np.array_equal(act[:, ~reset], a.T[:, ~reset])


def _drive(p, actions, resets, n=1, seed=SEED, lag=None):
    """one env batch through reset_all and then push / finish per step -> applied per step [steps, n, 2] (as float32)"""
    st = R.State(n, p)
    act = np.zeros((2, n), np.uint32)
    st, act, _ = R.finish(st, np.zeros((n, 2), np.uint32), act, None, -1, np.ones(n, bool), 0, seed, 0)
    out = []
    for a, r in zip(actions, resets):
        if lag is not None:
            st.lag[:] = np.asarray(lag, np.uint32).reshape(2, 1)
        w = np.asarray(a, np.float32).reshape(n, 2).view(np.uint32)
        st, applied = R.push(st, w)
        st, act, _ = R.finish(st, w, act, None, -1, np.full(n, bool(r)), 0, seed, 0)
        out.append(applied.view(np.float32))
    return np.array(out), st


def test_reference_semantics_on_small_hand_cases():
    seq = [[k + 1.0, -(k + 1.0)] for k in range(7)]
    none = [False] * 7
    # lag 0 is the identity
    got, _ = _drive(R.P(0, 3), seq, none, lag=(0, 0))
    assert np.array_equal(got[:, 0], np.float32(seq))
    # lag 2 after a reset: the first action three times, then two behind
    got, _ = _drive(R.P(2, 2), seq, none)
    assert got[:, 0, 0].tolist() == [1, 1, 1, 2, 3, 4, 5] and got[:, 0, 1].tolist() == [-1, -1, -1, -2, -3, -4, -5]
    # a reset in mid-ring (after step 3): the ring is forgotten, the env starts over with action 5
    got, _ = _drive(R.P(2, 2), seq, [False, False, False, True, False, False, False])
    assert got[:, 0, 0].tolist() == [1, 1, 1, 2, 5, 5, 5]
    # per_component: two lags from one block, and the components trail by their own lag; shared: one lag for both
    lags = R.draw_lags(np.arange(4096, dtype=np.uint32), np.zeros(4096, np.uint32), SEED, R.P(0, 3, True))
    assert (lags[0] != lags[1]).any() and set(np.unique(lags)) == {0, 1, 2, 3}
    shared = R.draw_lags(np.arange(4096, dtype=np.uint32), np.zeros(4096, np.uint32), SEED, R.P(0, 3, False))
    assert np.array_equal(shared[0], shared[1]) and np.array_equal(shared[0], lags[0])
    got, _ = _drive(R.P(0, 3, True), seq, none, lag=(1, 3))
    assert got[:, 0, 0].tolist() == [1, 1, 2, 3, 4, 5, 6] and got[:, 0, 1].tolist() == [-1, -1, -1, -1, -2, -3, -4]
    # the clamp of the reference on the words that matter
    w = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x3F800001, 0xBF800001, 0x7FC00001, 0x3F000000], np.uint32)
    assert R.clamp_words(w).tolist() == [0x80000000, 0x00000001, R.ONE, R.MINUS_ONE, R.ONE, R.MINUS_ONE, R.MINUS_ONE, 0x3F000000]


def test_draws_depend_on_nothing_but_the_env_id_and_the_count():
    """sharding in the reference: 130 envs at once equal two shards of 65 with env_offset 0 and 65, byte for byte"""
    case, n = CASES["lockstep"], 130
    ops = case.calls(n, np.random.default_rng(3))
    rng = np.random.default_rng(4)
    act, row = rng.integers(0, 1 << 32, (2, n), np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, (n, case.pitch), np.uint64).astype(np.uint32)
    whole = R.run(case, R.State(n, case.p), act, row, ops, SEED, 0)

    def shard(lo, hi):
        sub = [dict(o, action=o["action"][lo:hi], ra=o["ra"][lo:hi], rb=o["rb"][lo:hi]) for o in ops]
        return R.run(case, R.State(hi - lo, case.p), act[:, lo:hi], row[lo:hi], sub, SEED, lo)
    a, b = shard(0, 65), shard(65, 130)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(np.concatenate([x.st.block(65), y.st.block(65)], axis=1), w.st.block(130))
        assert np.array_equal(np.concatenate([x.applied, y.applied]), w.applied) and np.array_equal(np.concatenate([x.row, y.row]), w.row)
        assert np.array_equal(np.concatenate([x.act_rows, y.act_rows], axis=1), w.act_rows)


@pytest.mark.parametrize("lo,hi", [(0, 3), (2, 2)])
def test_lag_histogram_over_4096_envs_and_8_episodes(lo, hi):
    n, eps = 4096, 8
    ids = np.tile(np.arange(n, dtype=np.uint32), eps)
    drawn = np.repeat(np.arange(eps, dtype=np.uint32), n)
    lag = R.draw_lags(ids, drawn, STAT_SEED, R.P(lo, hi, True)).astype(np.int64)          # [2, eps * n]
    assert lag.min() >= lo and lag.max() <= hi
    count, span = lag.shape[1], hi - lo + 1
    if span == 1:
        assert (lag == lo).all()
        return
    q = 1.0 / span
    se = np.sqrt(q * (1 - q) / count)
    for c in (0, 1):
        freq = np.bincount(lag[c] - lo, minlength=span) / count
        assert (np.abs(freq - q) < 5 * se).all(), (c, freq)
    corr = lambda x, y: float(np.corrcoef(x, y)[0, 1])
    bound = 5 / np.sqrt(count)
    assert abs(corr(lag[0], lag[1])) < bound                                                # between the two components
    per_ep = lag.reshape(2, eps, n)
    assert abs(corr(per_ep[0, :, :-1].ravel(), per_ep[0, :, 1:].ravel())) < bound           # between adjacent envs
    assert abs(corr(per_ep[0, :-1].ravel(), per_ep[0, 1:].ravel())) < bound                 # between an env's consecutive episodes


# ---- the C boundary --------------------------------------------------------------------------------------------------

def test_latency_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.ACTLAT_SIGNATURES) == {"wl_action_latency_version", "wl_action_latency_width", "wl_action_latency_push", "wl_action_latency_finish"}
    others = (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES) | set(A.OBSNORM_SIGNATURES) | set(A.RAYCASTER_SIGNATURES)
              | set(A.OBSHIST_SIGNATURES) | set(A.OBSCORRUPT_SIGNATURES) | set(A.EVENTRAND_SIGNATURES))
    assert not declared & others
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_action_latency_version() == 1 == A.WL_ACTLAT_VERSION


def _probe(tmp_path, include, names):
    probe = tmp_path / f"probe_{include.replace('.', '_')}.c"
    probe.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{include}"\n'
                     f'int main(){{int v[] = {{{", ".join("(int)" + x for x in names)}}};\n'
                     'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%d ", v[i]); return 0;}\n')
    exe = tmp_path / (probe.stem + ".exe")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_latency_header_matches_the_python_mirror_and_the_step_boundary_is_unchanged(tmp_path):
    """the header declares no struct (its arguments are scalars and pointers): the probe holds its constants, the state rows it names and
    the sizes of the step boundary's structs, which this header includes and must leave as they are"""
    got = _probe(tmp_path, "wheeledlab_amd_latency.h", ("WL_ACTLAT_VERSION", "WL_ACTLAT_MAX_DELAY", "WL_ACTLAT_HEAD_ROWS", "WL_AL_STREAM", "WL_S_ACT0",
                                                         "WL_S_ACT1", "WL_S_COUNT", "WL_ABI_VERSION", "WL_ABI_REVISION", "sizeof(WlEnvBuffers)",
                                                         "sizeof(WlStepOut)", "sizeof(WlActionParams)", "sizeof(WlDriftParams)"))
    assert got == [A.WL_ACTLAT_VERSION, A.ACTLAT_MAX_DELAY, A.ACTLAT_HEAD_ROWS, A.AL_STREAM, A.S_ACT0, A.S_ACT1, A.S_COUNT, A.WL_ABI_VERSION,
                   A.WL_ABI_REVISION, C.sizeof(A.WlEnvBuffers), C.sizeof(A.WlStepOut), C.sizeof(A.WlActionParams), C.sizeof(A.WlDriftParams)]
    assert got[:4] == [1, R.CAP, R.HEAD_ROWS, R.STREAM] and R.CAP >= 16 and got[4] == R.S_ACT0 and got[7:9] == [24, 1]
    # wheeledlab_amd.h itself: the same values through the step boundary's header alone
    alone = _probe(tmp_path, "wheeledlab_amd.h", ("WL_S_ACT0", "WL_S_ACT1", "WL_S_COUNT", "WL_ABI_VERSION", "WL_ABI_REVISION", "sizeof(WlEnvBuffers)",
                                                  "sizeof(WlStepOut)", "sizeof(WlActionParams)", "sizeof(WlDriftParams)"))
    assert alone == got[4:]
    # the stream id is appended to wl_rng.h and is no other draw's; nothing before it is renumbered
    rng_h = open(os.path.join(ROOT, "wheeledlab_amd", "csrc", "wl_rng.h")).read()
    # (written as the id after WL_RS_EVENT_TIMER, which is 19; wl_action_latency_dev.h asserts the value 20 when the library is compiled)
    ids = re.findall(r"(WL_RS_[A-Z0-9_]+) = (\d+)", rng_h)
    assert [v for _, v in ids] == ["0", "4", "5", "7", "8", "9", "10", "16", "17", "18", "19"] and ids[-1] == ("WL_RS_EVENT_TIMER", "19")
    assert len(re.findall(r"\bWL_RS_ACT_LAG = WL_RS_EVENT_TIMER \+ 1 \};", rng_h)) == 1 and len(re.findall(r"\bWL_RS_[A-Z0-9_]+ = ", rng_h)) == 12
    dev_h = open(os.path.join(ROOT, "wheeledlab_amd", "csrc", "wl_action_latency_dev.h")).read()
    assert "static_assert(WL_RS_ACT_LAG == WL_AL_STREAM && WL_AL_STREAM == 20" in dev_h
    terrain_h = open(os.path.join(ROOT, "include", "wheeledlab_amd_terrain.h")).read()
    assert 20 not in {int(v) for v in re.findall(r"#define WL_TS_[A-Z_]+ (\d+)", terrain_h)}


def test_width_accepts_delays_up_to_the_cap_and_refuses_more():
    lib = _lib()
    for d in range(R.CAP + 1):
        assert lib.wl_action_latency_width(d) == R.width(d) == 5 + 2 * (d + 1)
    for d in (-1, R.CAP + 1, 1 << 20, -(1 << 31)):
        assert lib.wl_action_latency_width(d) == -1 == R.width(d)


def test_launches_refuse_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    n, stride, D, pitch, col = 130, 192, 3, 14, 12
    rows = R.width(D)
    M = 1 << 20
    fake = 1 << 24                     # never dereferenced: every call below returns before any launch
    base = dict(n=n, action=fake, applied=fake + M, state=fake + 2 * M, stride=stride, row=fake + 3 * M, pitch=pitch, col=col, block=fake + 4 * M,
                ra=fake + 5 * M, rb=fake + 5 * M + 4096, lo=1, hi=D, per=1, clip=0)

    def push(**kw):
        a = {**base, **kw}
        return lib.wl_action_latency_push(a["n"], a["action"], a["applied"], a["block"], a["stride"], a["hi"], None)

    def finish(**kw):
        a = {**base, **kw}
        return lib.wl_action_latency_finish(a["n"], a["action"], a["state"], a["stride"], a["row"], a["pitch"], a["col"], a["block"], a["ra"], a["rb"],
                                            a["lo"], a["hi"], a["per"], a["clip"], 42, 0, None)
    for k in ("action", "applied", "block"):
        assert push(**{k: None}) == -1, k
    for k in ("action", "state", "block", "ra", "row"):
        assert finish(**{k: None}) == -1, k
    common = (dict(n=0), dict(n=-1), dict(stride=128), dict(stride=64, n=65), dict(hi=R.CAP + 1, lo=0), dict(hi=-1, lo=-1))
    for kw in common:
        assert push(**kw) == -1 and finish(**kw) == -1, kw
    for kw in (dict(lo=D + 1), dict(lo=-1), dict(per=2), dict(per=-1), dict(clip=2), dict(pitch=0), dict(col=-2), dict(col=pitch - 1), dict(col=pitch),
               dict(stride=1 << 25, n=1 << 25)):
        assert finish(**kw) == -1, kw
    for kw in (dict(stride=129, n=129), dict(stride=130), dict(stride=193)):                # a stride that is no multiple of 64
        assert push(**kw) == -3 and finish(**kw) == -3, kw
    for k in ("action", "applied", "block"):
        for off in (1, 2, 3):
            assert push(**{k: base[k] + off}) == -3, (k, off)
    for k in ("action", "state", "block", "row"):
        for off in (1, 2, 3):
            assert finish(**{k: base[k] + off}) == -3, (k, off)
    bbytes = ((rows - 1) * stride + n) * 4
    # push: applied on the policy's action, on the block; the block on the action
    for kw in (dict(applied=base["action"]), dict(applied=base["action"] + 8 * n - 4), dict(applied=base["action"] - 8 * n + 4),
               dict(applied=base["block"] + bbytes - 4), dict(block=base["applied"] - bbytes + 4), dict(action=base["block"] + 64)):
        assert push(**kw) == -1, kw
    # finish: the block, the row, the action and the flags on the two action rows of the state or on each other
    acts = base["state"] + A.S_ACT0 * stride * 4
    abytes, rbytes = (stride + n) * 4, ((n - 1) * pitch + col + 2) * 4
    for kw in (dict(block=acts), dict(block=acts + abytes - 4), dict(block=acts - bbytes + 4), dict(row=acts + 8), dict(row=acts - rbytes + 4),
               dict(action=acts + 64), dict(ra=acts + abytes - 1), dict(rb=acts - n + 1),
               dict(row=base["block"] + 128), dict(action=base["block"] + bbytes - 4), dict(ra=base["block"] + 5), dict(rb=base["block"] - n + 1),
               dict(action=base["row"] + rbytes - 4), dict(ra=base["row"] + 1), dict(rb=base["row"] + rbytes - 1)):
        assert finish(**kw) == -1, kw
    # (the block may lie on the state's other rows; reset_b may be NULL and the row is not looked at without a column: those calls launch
    # -- tests/test_gpu_action_latency.py makes them on real buffers)


# ---- the device bodies on the host ---------------------------------------------------------------------------------------

def _build(out, *flags):
    cxx = CLANG if (os.path.exists(CLANG) or shutil.which(CLANG)) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler to build the host simulation")
    subprocess.run([cxx, "-O1", "-std=c++17", *flags, "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), SRC, "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_sim") / "action_latency_host")


def host_snan(exe, env=None):
    """what the stand-in's median of three makes of a signalling NaN (tests/action_latency_reference.py says why it is asked); the quiet
    one is fixed"""
    s, q = (int(v) for v in subprocess.run([exe, "--med3"], capture_output=True, text=True, check=True, env=env).stdout.split())
    assert q == R.MINUS_ONE and s in (R.ONE, R.MINUS_ONE)
    return np.uint32(s)


def words(rng, *shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def run_host(exe, tmp, case, n, stride, state, row, block, ops, seed, env_offset, env=None):
    """-> None (max_delay was refused) or [(applied, state, row, block) words] after every operation"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    p = case.p
    with open(fin, "wb") as f:
        f.write(struct.pack("<10q", n, stride, p.lo, p.hi, int(p.per), case.clip_wrapper, case.pitch, case.col, int(case.has_b), len(ops)))
        f.write(struct.pack("<2Q", seed, env_offset))
        f.write(np.ascontiguousarray(state, np.uint32).tobytes())
        if case.col >= 0:
            f.write(np.ascontiguousarray(row, np.uint32).tobytes())
        f.write(np.ascontiguousarray(block, np.uint32).tobytes())
        for o in ops:
            f.write(struct.pack("<q", 0 if o["kind"] == "push" else 1))
            f.write(np.ascontiguousarray(o["action"], np.uint32).tobytes())
            if o["kind"] == "finish":
                f.write(np.ascontiguousarray(o["ra"], np.uint8).tobytes())
                if case.has_b:
                    f.write(np.ascontiguousarray(o["rb"], np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, env=env)
    raw = open(fout, "rb").read()
    rows = struct.unpack("<q", raw[:8])[0]
    if rows < 0:
        assert len(raw) == 8
        return None
    out, q = [], 8

    def take(*shape):
        nonlocal q
        a = np.frombuffer(raw[q:q + 4 * int(np.prod(shape))], np.uint32).reshape(shape)
        q += a.nbytes
        return a
    for _ in ops:
        out.append((take(n, 2), take(A.S_COUNT, stride), take(n, case.pitch) if case.col >= 0 else None, take(rows, stride)))
    assert q == len(raw)
    return out


def check_snapshot(what, n, case, want, applied, state, row, block, state0, row0, block0):
    """one operation's result against the reference, and everything the launch does not own against the copy taken before it"""
    assert np.array_equal(applied, want.applied), what
    assert np.array_equal(block[:, :n], want.st.block(n)), what
    assert np.array_equal(state[A.S_ACT0:A.S_ACT1 + 1, :n], want.act_rows), what
    keep = np.ones(state.shape[0], bool)
    keep[A.S_ACT0:A.S_ACT1 + 1] = False
    assert np.array_equal(state[keep], state0[keep]) and np.array_equal(state[:, n:], state0[:, n:]), what       # every other state row, the padding
    assert np.array_equal(block[:, n:], block0[:, n:]), what
    if row is not None:
        assert np.array_equal(row, want.row if case.col >= 0 else row0), what
        cols = np.ones(row.shape[1], bool)
        if case.col >= 0:
            cols[case.col:case.col + 2] = False
        assert np.array_equal(row[:, cols], row0[:, cols]), what                                                   # every other column


def _check_host(exe, tmp, case, n, stride, env_offset=11, env=None, seed_salt=0):
    rng = np.random.default_rng(n * 7 + case.p.hi + seed_salt)
    ops = case.calls(n, rng)
    state, row = words(rng, A.S_COUNT, stride), words(rng, n, case.pitch)
    block = R.State(n, case.p).block(stride, fill=0xDEADBEEF)
    block[:, :n] = 0
    got = run_host(exe, tmp, case, n, stride, state, row, block, ops, SEED, env_offset, env=env)
    want = R.run(case, R.State(n, case.p), state[A.S_ACT0:A.S_ACT1 + 1, :n], row, ops, SEED, env_offset, snan=host_snan(exe, env))
    s0, r0, b0 = state, row, block
    for k, (w, (applied, s1, r1, b1)) in enumerate(zip(want, got)):
        check_snapshot(f"n={n} op {k} ({ops[k]['kind']})", n, case, w, applied, s1, r1, b1, s0, r0, b0)
        s0, r0, b0 = s1, (r1 if r1 is not None else r0), b1


@pytest.mark.parametrize("name", list(CASES))
def test_host_bodies_equal_the_reference(exe, tmp_path, name):
    for n, stride in ((1, 64), (5, 64), (67, 128)):
        _check_host(exe, str(tmp_path), CASES[name], n, stride)
    _check_host(exe, str(tmp_path), CASES[name], 3, 64, env_offset=(1 << 35) + (1 << 32) - 2)      # ids wrap through 2^32


@pytest.mark.parametrize("lo,hi", R.DELAYS)
@pytest.mark.parametrize("per", [False, True])
def test_host_bodies_at_every_delay_range(exe, tmp_path, lo, hi, per):
    _check_host(exe, str(tmp_path), CASES["lockstep"].with_p(R.P(lo, hi, per)), 67, 128)


def test_host_program_refuses_a_delay_over_the_cap(exe, tmp_path):
    case = R.Case(R.P(0, R.CAP + 1))
    assert run_host(exe, str(tmp_path), case, 2, 64, np.zeros((A.S_COUNT, 64), np.uint32), np.zeros((2, 14), np.uint32), np.zeros((1, 64), np.uint32), [], 1, 0) is None


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path / "action_latency_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, case in CASES.items():
        _check_host(exe, str(tmp_path), case, 1, 64, env=env)
        _check_host(exe, str(tmp_path), case, 64, 64, env=env)              # the exact size: env 63 is the last word of every row
    _check_host(exe, str(tmp_path), CASES["lockstep"].with_p(R.P(R.CAP, R.CAP, True)), 64, 64, env=env)


# ---- config resolution ---------------------------------------------------------------------------------------------------

TASKS = ("Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0", "Isaac-MushrVisualDepthRL-v0")
RUNS = ("RSS_DRIFT_CONFIG", "RSS_ELEV_CONFIG", "RSS_VISUAL_CONFIG", "VISUAL_DEPTH_CONFIG")


def _cfg(task="Isaac-MushrDriftRL-v0"):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    return registry.parse_env_cfg(task, device="cpu", num_envs=4)


def test_resolve_is_none_for_every_shipped_config_and_for_zero_delays():
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs.actions import ActionLatencyCfg
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.envs.latency import resolve
    for task in TASKS:
        cfg = _cfg(task)
        assert cfg.actions.throttle_steer.latency is None and resolve(cfg.actions) is None and flatten_cfg(cfg).latency is None, task
    for run in RUNS:
        assert flatten_cfg(resolve_run(run, []).env).latency is None, run
    cfg = _cfg()
    for zero in (ActionLatencyCfg(), ActionLatencyCfg(min_delay=0, max_delay=0, per_component=True), {}, {"min_delay": 0, "max_delay": 0}):
        cfg.actions.throttle_steer.latency = zero
        assert resolve(cfg.actions) is None and flatten_cfg(cfg).latency is None
    assert (ActionLatencyCfg().min_delay, ActionLatencyCfg().max_delay, ActionLatencyCfg().per_component) == (0, 0, False)


def test_resolve_builds_the_spec():
    from wheeledlab_amd.envs.actions import ActionLatencyCfg
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.envs.latency import LatencySpec
    for task in TASKS:
        cfg = _cfg(task)
        cfg.actions.throttle_steer.latency = ActionLatencyCfg(min_delay=1, max_delay=3, per_component=True)
        assert flatten_cfg(cfg).latency == LatencySpec(1, 3, True, "throttle_steer"), task
    cfg = _cfg()
    cfg.actions.throttle_steer.latency = {"max_delay": np.int64(A.ACTLAT_MAX_DELAY)}
    assert flatten_cfg(cfg).latency == LatencySpec(0, A.ACTLAT_MAX_DELAY, False, "throttle_steer")
    cfg.actions.throttle_steer.latency = {"min_delay": 2.0, "max_delay": 2}                 # 2.0 from a command line is 2
    assert flatten_cfg(cfg).latency == LatencySpec(2, 2, False, "throttle_steer")


def test_resolve_refusals_name_the_action_term():
    import torch
    from wheeledlab_amd.envs.actions import ActionLatencyCfg
    from wheeledlab_amd.envs.flatten import flatten_cfg
    bad = (dict(min_delay=-1, max_delay=2), dict(min_delay=0, max_delay=-1), dict(min_delay=1.5, max_delay=2), dict(min_delay=0, max_delay="3"),
           dict(min_delay=True, max_delay=2), dict(min_delay=3, max_delay=2), dict(min_delay=0, max_delay=A.ACTLAT_MAX_DELAY + 1),
           dict(min_delay=torch.tensor([0, 1]), max_delay=3), dict(min_delay=0, max_delay=np.array([1, 2])), dict(min_delay=0, max_delay=torch.tensor(2)),
           dict(min_delay=0, max_delay=(1, 2)), dict(min_delay=0, max_delay=2, per_component=1), dict(min_delay=0, max_delay=float("nan")),
           dict(min_delay=0, max_delay=2, lag=1))
    for kw in bad:
        for form in ("dict", "cfg"):
            if form == "cfg" and "lag" in kw:
                continue
            cfg = _cfg()
            cfg.actions.throttle_steer.latency = dict(kw) if form == "dict" else ActionLatencyCfg(**kw)
            with pytest.raises(ValueError, match="throttle_steer"):
                flatten_cfg(cfg)
    cfg = _cfg()
    cfg.actions.throttle_steer.latency = 3
    with pytest.raises(ValueError, match="throttle_steer"):
        flatten_cfg(cfg)
    with pytest.raises(ValueError, match="tensor-valued"):
        cfg.actions.throttle_steer.latency = dict(min_delay=torch.tensor([0, 1]), max_delay=3)
        flatten_cfg(cfg)


def test_train_script_override_reaches_the_spec():
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.envs.latency import LatencySpec
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.actions.throttle_steer.latency={'min_delay': 1, 'max_delay': 3}"])
    assert flatten_cfg(run.env).latency == LatencySpec(1, 3, False, "throttle_steer")
    run = resolve_run("RSS_ELEV_CONFIG", ["env.actions.throttle_steer.latency={'max_delay': 2, 'per_component': True}"])
    assert flatten_cfg(run.env).latency == LatencySpec(0, 2, True, "throttle_steer")
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.actions.throttle_steer.latency={'min_delay': 4, 'max_delay': 3}"])
    with pytest.raises(ValueError, match="throttle_steer"):
        flatten_cfg(run.env)

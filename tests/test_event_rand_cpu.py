"""CPU checks of the per-episode domain randomisation: the header and its ctypes mirror, wl_event_rand_width on good and bad tables,
every argument refusal of wl_event_rand_apply before any launch, envs/events.resolve on configs (the accepted forms, every refusal, dict
and string overrides), and the per-env body compiled for the host as a stand-alone program (tests/host_sim/event_rand_host.cpp) --
plain and under -fsanitize=address,undefined -- against the reference (tests/event_rand_reference.py) over the case list the GPU test
runs.

On the host the stand-in's log2, sqrt and cos are libm's (EZ_HOST of tests/obs_corrupt_reference.py) and exp2 is libm's in double,
rounded once (2^-24 relative, inside the reference's EXP_HW); everything that is not a Gaussian or log_uniform value is byte for byte."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import event_rand_reference as R
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_events.h")
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(ROOT, "tests", "host_sim", "event_rand_host.cpp")
CASES = R.cases()
SEED = 0x0123_4567_89AB_CDEF


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def _ctable(rows):
    rows = list(rows)
    return (A.WlEventRandTerm * max(len(rows), 1))(*[A.WlEventRandTerm(*r) for r in rows])


# ---- the reference holds itself ----------------------------------------------------------------------------------------

def test_case_list_covers_what_it_claims():
    seen = set()
    for c in CASES.values():
        assert 1 <= len(c.tab) <= R.MAX_TERMS
        seen |= {(t["target"], t["op"], t["dist"]) for t in c.tab if t["target"] != R.MU}
        seen |= {("mode", t["target"], t["mode"]) for t in c.tab}
    for target in (R.DAMP, R.MASS_BASE):
        for op in (R.ADD, R.SCALE, R.ABS):
            for d in (R.UNIFORM, R.LOG_UNIFORM, R.GAUSSIAN):
                assert (target, op, d) in seen
    assert all((R.MASS_WHEELS, R.ABS, d) in seen for d in (R.UNIFORM, R.LOG_UNIFORM, R.GAUSSIAN))
    assert all(("mode", t, m) in seen for t in (R.MU, R.DAMP, R.MASS_BASE, R.MASS_WHEELS) for m in (R.RESET, R.INTERVAL))


def test_timer_edge_lands_on_1e6_exactly_and_on_the_float_below():
    """step_dt and the drawn timers are chosen here, on the CPU: dt = 2^-30 s and T = 1e-6f + 2^-30 (a timer of zero span draws its lower
    bound); a float32 pair that lands on 1e-6 exactly exists, and the float32 below T lands on the float32 below 1e-6"""
    one = np.float32(1e-6)
    assert np.float32(R.EDGE_T - R.EDGE_DT) == one and not (np.float32(R.EDGE_T - R.EDGE_DT) < one)
    below = np.float32(R.EDGE_T_BELOW - R.EDGE_DT)
    assert below < one and np.nextafter(below, np.float32(1)) == one            # the float32 adjacent to 1e-6 from below
    case = CASES["timer_edge"]
    n = 3
    st = R.run(case, case.initial(n, np.random.default_rng(0)), case.calls(n, None), SEED, 0)
    # call 0 draws the timers; call 1: term 0 and the global term sit ON 1e-6 and do not fire, term 1 fires; call 2: they fire
    assert (st[1].tl[0].view(np.uint32) == one.view(np.uint32)).all() and not st[1].fired[0].any() and not st[1].fired[2].any()
    assert st[1].fired[1].all() and st[2].fired[0].all() and st[2].fired[2].all()


def test_reference_semantics_on_small_hand_cases():
    rng = np.random.default_rng(5)
    n = 6
    case = CASES["same_target"]
    calls = case.calls(n, rng)
    st = R.run(case, case.initial(n, rng), calls, SEED, 0)
    assert ((st[0].consts[R.C_DAMP] >= 30) & (st[0].consts[R.C_DAMP] <= 40)).all()          # the interval term wins: the later pass
    assert (st[0].consts[R.C_MU_S] >= 1.0).all()                                             # of two reset terms the later in the table
    case = CASES["min_steps"]
    st = R.run(case, case.initial(n, rng), case.calls(n, rng), SEED, 0)
    even = np.arange(n) % 2 == 0
    assert [s.fired[0][even].all() for s in st] == [True, False, True, False, True]
    assert [s.fired[0][~even].all() for s in st] == [False, True, False, True, True]
    assert not st[1].fired[0][even].any() and not st[3].fired[0][even].any()
    case = CASES["global_time"]
    st = R.run(case, case.initial(n, rng), case.calls(n, rng), SEED, 3)
    for s in st:
        assert len(set(s.tl[0].view(np.uint32).tolist())) == 1 and (s.fired[0].all() or not s.fired[0].any())   # one timer, every lane
    assert any(s.fired[0].all() for s in st) and len({tuple(s.tl[2].tolist()) for s in st}) > 1
    case = CASES["mass_parts"]
    for s in R.run(case, case.initial(n, rng), case.calls(n, rng), SEED, 0):
        assert np.array_equal(s.consts[R.C_MASS], (s.parts[0] + s.parts[1]).astype(np.float32))


def test_draws_depend_on_nothing_but_the_env_id_and_the_count():
    """sharding in the reference: envs 0 .. 9 at once equal two halves with env_offset 0 and 5"""
    case = CASES["lockstep"]
    n = 10
    calls = case.calls(n, np.random.default_rng(3))
    init = case.initial(n, np.random.default_rng(4))
    whole = R.run(case, init, calls, SEED, 0)[-1]

    def half(lo, hi):
        st = R.State(hi - lo, len(case.tab), init.consts[:, lo:hi], init.parts[:, lo:hi])
        sub = [dict(c, ra=c["ra"][lo:hi], rb=c["rb"][lo:hi], mask=c["mask"][lo:hi]) for c in calls]
        return R.run(case, st, sub, SEED, lo)[-1]
    a, b = half(0, 5), half(5, 10)
    for k in ("consts", "parts", "tl", "applied", "w2", "w3"):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=1).view(np.uint32), getattr(whole, k).view(np.uint32)), k


# ---- the C boundary --------------------------------------------------------------------------------------------------

def test_events_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.EVENTRAND_SIGNATURES) == {"wl_event_rand_version", "wl_event_rand_width", "wl_event_rand_apply"}
    others = (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES) | set(A.OBSNORM_SIGNATURES) | set(A.RAYCASTER_SIGNATURES)
              | set(A.OBSHIST_SIGNATURES) | set(A.OBSCORRUPT_SIGNATURES))
    assert not declared & others
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_event_rand_version() == 1 == A.WL_EVENTRAND_VERSION


def test_events_header_matches_the_ctypes_struct_and_the_step_boundary_is_unchanged(tmp_path):
    fields = [f for f, _ in A.WlEventRandTerm._fields_]
    assert tuple(fields) == R.FIELDS and struct.calcsize(R.STRUCT) == C.sizeof(A.WlEventRandTerm)
    probe = tmp_path / "probe.c"
    offs = ", ".join(f"(int)offsetof(WlEventRandTerm, {f})" for f in fields)
    names = ("WL_EVENTRAND_VERSION", "WL_EVENTRAND_MAX_TERMS", "WL_ER_STREAM_VALUE", "WL_ER_STREAM_TIMER", "WL_ER_MU", "WL_ER_DAMP", "WL_ER_MASS_BASE",
             "WL_ER_MASS_WHEELS", "WL_ER_RESET", "WL_ER_INTERVAL", "WL_ER_ADD", "WL_ER_SCALE", "WL_ER_ABS", "WL_ER_UNIFORM", "WL_ER_LOG_UNIFORM",
             "WL_ER_GAUSSIAN", "WL_S_MU_S", "WL_S_MU_D", "WL_S_DAMP", "WL_S_MASS", "WL_ABI_VERSION", "WL_ABI_REVISION")
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_events.h"\n'
                     f'int main(){{int v[] = {{{", ".join("(int)" + x for x in names)}, (int)sizeof(WlEventRandTerm), {offs}}};\n'
                     'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%d ", v[i]); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = A.WlEventRandTerm
    assert got == [A.WL_EVENTRAND_VERSION, A.EVENTRAND_MAX_TERMS, A.ER_STREAM_VALUE, A.ER_STREAM_TIMER, A.ER_MU, A.ER_DAMP, A.ER_MASS_BASE, A.ER_MASS_WHEELS,
                   A.ER_RESET, A.ER_INTERVAL, A.ER_ADD, A.ER_SCALE, A.ER_ABS, A.ER_UNIFORM, A.ER_LOG_UNIFORM, A.ER_GAUSSIAN, A.S_MU_S, A.S_MU_D, A.S_DAMP,
                   A.S_MASS, A.WL_ABI_VERSION, A.WL_ABI_REVISION, C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert got[:4] == [1, R.MAX_TERMS, R.S_VALUE, R.S_TIMER] and got[20:23] == [24, 1, 68]
    assert (R.MU, R.DAMP, R.MASS_BASE, R.MASS_WHEELS, R.RESET, R.INTERVAL, R.ADD, R.SCALE, R.ABS, R.UNIFORM, R.LOG_UNIFORM, R.GAUSSIAN) == tuple(got[4:16])
    # the two stream ids are appended to wl_rng.h and are no other draw's; nothing before them is renumbered
    rng_h = open(os.path.join(ROOT, "wheeledlab_amd", "csrc", "wl_rng.h")).read()
    ids = re.findall(r"(WL_RS_[A-Z0-9_]+) = (\d+)", rng_h)
    assert ids[-2:] == [("WL_RS_EVENT_VALUE", "18"), ("WL_RS_EVENT_TIMER", "19")] and len({v for _, v in ids}) == len(ids)
    assert [v for _, v in ids[:-2]] == ["0", "4", "5", "7", "8", "9", "10", "16", "17"] and ("WL_RS_STARTUP_BUCKET", str(R.S_BUCKET)) in ids
    terrain_h = open(os.path.join(ROOT, "include", "wheeledlab_amd_terrain.h")).read()
    assert not {18, 19} & {int(v) for v in re.findall(r"#define WL_TS_[A-Z_]+ (\d+)", terrain_h)}


def _good():
    T = R.term
    return [T(R.MU, R.RESET, **R.FRICTION), T(R.DAMP, R.INTERVAL, R.SCALE, R.LOG_UNIFORM, (0.5, 2.0), base=30.0, interval=(1.0, 2.0)),
            T(R.MASS_BASE, R.RESET, R.ADD, R.GAUSSIAN, (0.4, 0.05), base=3.0, min_steps=4), T(R.MASS_WHEELS, R.INTERVAL, R.ABS, R.UNIFORM, (0.03, 0.08), interval=(4.0, 4.0), global_time=1)]


def _bad_tables():
    good = _good()

    def bad(k, **kw):
        t = [dict(x) for x in good]
        t[k].update(kw)
        return t
    inf, nan = float("inf"), float("nan")
    return good, (("unknown target", bad(0, target=4)), ("negative target", bad(0, target=-1)), ("unknown mode", bad(1, mode=2)), ("negative mode", bad(1, mode=-1)),
                  ("unknown operation", bad(1, op=3)), ("negative operation", bad(2, op=-1)), ("unknown distribution", bad(2, dist=3)),
                  ("negative distribution", bad(2, dist=-1)), ("lo > hi", bad(3, p0=0.09)), ("log_uniform lo > hi", bad(1, p0=2.5)),
                  ("negative std", bad(2, p1=-0.01)), ("log_uniform lo 0", bad(1, p0=0.0)), ("log_uniform lo < 0", bad(1, p0=-1.0)),
                  ("interval_lo > interval_hi", bad(1, interval_lo=3.0)), ("interval_lo 0", bad(1, interval_lo=0.0)), ("interval_lo < 0", bad(3, interval_lo=-1.0)),
                  ("num_buckets 0", bad(0, num_buckets=0)), ("num_buckets < 0", bad(0, num_buckets=-3)), ("add on the wheels", bad(3, op=R.ADD)),
                  ("scale on the wheels", bad(3, op=R.SCALE)), ("NaN p0", bad(2, p0=nan)), ("infinite p1", bad(3, p1=inf)), ("NaN base", bad(1, base=nan)),
                  ("infinite interval_hi", bad(1, interval_hi=inf)), ("NaN interval_lo", bad(1, interval_lo=nan)), ("NaN friction bound", bad(0, mu_s_lo=nan)),
                  ("infinite friction bound", bad(0, mu_d_hi=inf)), ("friction lo > hi", bad(0, mu_s_lo=1.0)), ("dynamic friction lo > hi", bad(0, mu_d_lo=0.9)),
                  ("is_global_time 2", bad(3, is_global_time=2)), ("make_consistent -1", bad(0, make_consistent=-1)),
                  ("negative min_step_count", bad(2, min_step_count_between_reset=-1)))


def test_width_accepts_good_tables_and_refuses_bad_ones():
    lib = _lib()
    width = lambda tab, n_terms=None: lib.wl_event_rand_width(_ctable(R.rows(tab)), len(tab) if n_terms is None else n_terms)
    for name, c in CASES.items():
        assert width(c.tab) == 2 + 4 * len(c.tab), name
    good, bads = _bad_tables()
    assert width(good) == 18
    for what, tab in bads:
        assert width(tab) == -1, what
    assert width(good, 0) == -1 and width(good * 2) == 34 and width(good * 2 + good[:1]) == -1 and lib.wl_event_rand_width(None, 2) == -1
    ok = [dict(good[0], p0=5.0, p1=1.0)]             # (friction ignores the distribution parameters, but they are still checked)
    assert width(ok) == -1


def test_apply_refuses_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    good, bads = _bad_tables()
    n, stride = 130, 192
    rows = 2 + 4 * len(good)
    fake = 1 << 24                     # never dereferenced: every call below returns before any launch
    base = dict(n=n, state=fake, stride=stride, terms=_ctable(R.rows(good)), n_terms=len(good), block=fake + (1 << 20), ra=fake + (2 << 20),
                rb=fake + (2 << 20) + 4096, mask=fake + (2 << 20) + 8192, mask_terms=0xF, dt=0.02)

    def apply(**kw):
        a = {**base, **kw}
        return lib.wl_event_rand_apply(a["n"], a["state"], a["stride"], a["terms"], a["n_terms"], a["block"], a["ra"], a["rb"], a["mask"], a["mask_terms"],
                                       42, 7, a["dt"], 0, None)
    for k in ("state", "block", "ra", "terms"):
        assert apply(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(n=-1), dict(stride=128), dict(stride=64, n=65), dict(n_terms=0), dict(n_terms=9), dict(mask_terms=0x10), dict(mask_terms=1 << 31),
               dict(dt=-0.02), dict(dt=float("nan")), dict(dt=float("inf")), dict(stride=1 << 25, n=1 << 25)):
        assert apply(**kw) == -1, kw
    for what, tab in bads:
        assert apply(terms=_ctable(R.rows(tab))) == -1, what
    for kw in (dict(stride=129, n=129), dict(stride=130), dict(stride=191 + 2)):            # a stride that is no multiple of 64
        assert apply(**kw) == -3, kw
    for k in ("state", "block"):
        for off in (1, 2, 3):
            assert apply(**{k: base[k] + off}) == -3, (k, off)
    consts = fake + A.S_MU_S * stride * 4
    cbytes, bbytes = (3 * stride + n) * 4, ((rows - 1) * stride + n) * 4
    for kw in (dict(block=consts), dict(block=consts + cbytes - 4), dict(block=consts - bbytes + 4),                 # the block on the constant rows
               dict(ra=consts + 8), dict(rb=consts + cbytes - 1), dict(mask=consts - n + 1),                          # a flag array on them
               dict(ra=base["block"] + bbytes - 1), dict(rb=base["block"] - n + 1), dict(mask=base["block"] + 64)):   # and on the block
        assert apply(**kw) == -1, kw
    # (the block may lie on the state's dynamic rows' side as long as it misses the four constant rows; reset_b and mask may be NULL:
    # those calls launch -- tests/test_gpu_event_rand.py makes them on real buffers)


# ---- the device body on the host ---------------------------------------------------------------------------------------

def _build(out, *flags):
    cxx = CLANG if (os.path.exists(CLANG) or shutil.which(CLANG)) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler to build the host simulation")
    subprocess.run([cxx, "-O1", "-std=c++17", *flags, "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), SRC, "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_sim") / "event_rand_host")


def pack_table(tab):
    return b"".join(struct.pack(R.STRUCT, *r) for r in R.rows(tab))


def state_words(rng, init, stride):
    """a whole state matrix of recognisable words with the constant rows of `init`"""
    s = rng.integers(0, 1 << 32, size=(A.S_COUNT, stride), dtype=np.uint64).astype(np.uint32)
    s[A.S_MU_S:A.S_MASS + 1, :init.n] = init.consts.view(np.uint32)
    return s


def run_host(exe, tmp, case, n, stride, state, block, calls, seed, env_offset, env=None):
    """-> None (the table was refused) or [(state words, block words)] after every call"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", n, stride, len(case.tab), int(case.has_b), int(case.has_mask), max((c["mask_terms"] for c in calls), default=0), len(calls)))
        f.write(struct.pack("<2Q", seed, env_offset))
        f.write(pack_table(case.tab))
        f.write(np.ascontiguousarray(state, np.uint32).tobytes())
        f.write(np.ascontiguousarray(block, np.uint32).tobytes())
        for c in calls:
            f.write(struct.pack("<Qd", c["step"], c["dt"]))
            f.write(np.ascontiguousarray(c["ra"], np.uint8).tobytes())
            if case.has_b:
                f.write(np.ascontiguousarray(c["rb"], np.uint8).tobytes())
            if case.has_mask:
                f.write(np.ascontiguousarray(c["mask"], np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, env=env)
    raw = open(fout, "rb").read()
    rows = struct.unpack("<q", raw[:8])[0]
    if rows < 0:
        assert len(raw) == 8
        return None
    out, p = [], 8
    for _ in calls:
        s = np.frombuffer(raw[p:p + 4 * A.S_COUNT * stride], np.uint32).reshape(A.S_COUNT, stride)
        p += s.nbytes
        b = np.frombuffer(raw[p:p + 4 * rows * stride], np.uint32).reshape(rows, stride)
        p += b.nbytes
        out.append((s, b))
    assert p == len(raw)
    return out


def check_untouched(state0, block0, state1, block1, n):
    """everything but the four constant rows and the block's first n columns is what it was, byte for byte"""
    keep = np.ones(state0.shape[0], bool)
    keep[A.S_MU_S:A.S_MASS + 1] = False
    assert np.array_equal(state0[keep], state1[keep]) and np.array_equal(state0[:, n:], state1[:, n:])
    assert np.array_equal(block0[:, n:], block1[:, n:])


def _check_host(exe, tmp, name, n, stride, env_offset=11, env=None):
    case = CASES[name]
    rng = np.random.default_rng(n * 7 + len(name))
    init = case.initial(n, rng)
    calls = case.calls(n, rng)
    same_bits = {c["mask_terms"] for c in calls}
    groups = [calls] if len(same_bits) == 1 else [[c] for c in calls]          # (the program takes one mask_terms per run)
    state, block = state_words(rng, init, stride), init.block(stride)
    block[:, n:] = 0xDEADBEEF
    st, worst = init, 0.0
    for group in groups:
        got = run_host(exe, tmp, case, n, stride, state, block, group, SEED, env_offset, env=env)
        for c, (s1, b1) in zip(group, got):
            want = R.run(case, st, [c], SEED, env_offset, ez=R.EZ_HOST)[0]
            check_untouched(state, block, s1, b1, n)
            worst = max(worst, R.check(s1[A.S_MU_S:A.S_MASS + 1], b1, want, what=f"{name} n={n} step={c['step']}"))
            quiet = ~want.fired.any(0)
            assert np.array_equal(s1[A.S_MU_S:A.S_MASS + 1, :n][:, quiet], state[A.S_MU_S:A.S_MASS + 1, :n][:, quiet])      # nothing applied: nothing stored
            # the program's own words go on (so that an inexact value stays the program's), the reference keeps its float64
            st, state, block = want, s1, b1
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_host_body_equals_the_reference(exe, tmp_path, name):
    for n, stride in ((1, 64), (5, 64), (67, 128)):
        _check_host(exe, str(tmp_path), name, n, stride)
    _check_host(exe, str(tmp_path), name, 3, 64, env_offset=(1 << 35) + (1 << 32) - 2)      # ids wrap through 2^32


def test_host_program_refuses_a_bad_table(exe, tmp_path):
    good, bads = _bad_tables()
    for what, tab in bads[::5]:
        case = R.Case(tab, None)
        assert run_host(exe, str(tmp_path), case, 2, 64, np.zeros((A.S_COUNT, 64), np.uint32), np.zeros((2 + 4 * len(tab), 64), np.uint32), [], 1, 0) is None, what


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path / "event_rand_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for name in CASES:
        _check_host(exe, str(tmp_path), name, 1, 64, env=env)
        _check_host(exe, str(tmp_path), name, 64, 64, env=env)              # the exact size: env 63 is the last word of every row


# ---- config resolution ---------------------------------------------------------------------------------------------------

TASKS = {"Isaac-MushrDriftRL-v0": "drift", "Isaac-MushrElevationRL-v0": "elevation", "Isaac-MushrVisualRL-v0": "visual",
         "Isaac-MushrVisualDepthRL-v0": "visual_depth"}


def _cfg(task="Isaac-MushrDriftRL-v0"):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    return registry.parse_env_cfg(task, device="cpu", num_envs=4)


def _visual_random(task="Isaac-MushrVisualRL-v0"):
    """the visual config with the reference's randomised events (the shipped one only resets)"""
    from wheeledlab_amd.tasks.visual.mushr_visual_env_cfg import VisualEventsRandomCfg
    cfg = _cfg(task)
    cfg.events = VisualEventsRandomCfg()
    return cfg


def _row(table, name):
    return dict(zip(R.FIELDS, table.terms[table.names.index(name)]))


def test_resolve_is_none_for_every_shipped_config_and_startup_terms_stay():
    from wheeledlab_amd.envs.events import resolve
    from wheeledlab_amd.envs.flatten import flatten_cfg
    for task in TASKS:
        flat = flatten_cfg(_cfg(task))
        assert flat.events is None and resolve(_cfg(task).events, flat.startup, TASKS[task]) is None, task
    flat = flatten_cfg(_cfg())
    assert (flat.startup.wheel_mu_s, flat.startup.mu_buckets, flat.startup.damping, flat.startup.mass_add) == ((0.3, 0.5), 20, (10.0, 50.0), (0.3, 0.5))
    assert flat.startup.throttle_damping == _cfg().scene.robot.actuators["throttle_joints"].damping and flat.startup.throttle_stiffness == 0.0


def test_resolve_builds_the_table_of_reset_and_interval_terms():
    from wheeledlab_amd.envs.flatten import flatten_cfg
    from wheeledlab_amd.params import MUSHR_CHASSIS_MASS
    cfg = _cfg()
    ev = cfg.events
    ev.change_wheel_friction.mode = "reset"
    ev.change_wheel_friction.min_step_count_between_reset = 7
    ev.add_base_mass.mode, ev.add_base_mass.interval_range_s, ev.add_base_mass.is_global_time = "interval", (4.0, 8.0), True
    ev.randomize_gains.mode = "reset"
    ev.randomize_gains.params.update(operation="scale", distribution="log_uniform", damping_distribution_params=(0.5, 2.0),
                                     stiffness_distribution_params=(0.0, 0.0))
    flat = flatten_cfg(cfg)
    T = flat.events
    assert T.names == ("change_wheel_friction", "randomize_gains", "add_base_mass") and T.has_mass        # the config's order
    f = _row(T, "change_wheel_friction")
    assert (f["target"], f["mode"], f["num_buckets"], f["make_consistent"], f["min_step_count_between_reset"]) == (R.MU, R.RESET, 20, 1, 7)
    assert (f["mu_s_lo"], f["mu_s_hi"], f["mu_d_lo"], f["mu_d_hi"]) == tuple(R.f32(v) for v in (0.3, 0.5, 0.3, 0.5))
    g = _row(T, "randomize_gains")
    thr = cfg.scene.robot.actuators["throttle_joints"]
    assert (g["target"], g["mode"], g["op"], g["dist"], g["p0"], g["p1"], g["base"]) == (R.DAMP, R.RESET, R.SCALE, R.LOG_UNIFORM, 0.5, 2.0, R.f32(thr.damping))
    m = _row(T, "add_base_mass")
    assert (m["target"], m["mode"], m["op"], m["dist"], m["p0"], m["p1"]) == (R.MASS_BASE, R.INTERVAL, R.ADD, R.UNIFORM, R.f32(0.3), R.f32(0.5))
    assert (m["base"], m["interval_lo"], m["interval_hi"], m["is_global_time"]) == (R.f32(MUSHR_CHASSIS_MASS), 4.0, 8.0, 1)
    # what moved to the layer no longer feeds the startup: the asset's own values stay until the first application
    assert flat.startup.wheel_mu_s == (0.4, 0.4) and flat.startup.mass_add == (0.0, 0.0) and flat.startup.damping == (thr.damping, thr.damping)
    lib = _lib()
    assert lib.wl_event_rand_width(_ctable(T.terms), 3) == 14
    # the visual config: wheel masses (abs on the wheel links) and an abs chassis
    cfg = _visual_random()
    cfg.events.add_wheel_mass.mode = "reset"
    cfg.events.add_base_mass.mode = "reset"
    flat = flatten_cfg(cfg)
    w, b = _row(flat.events, "add_wheel_mass"), _row(flat.events, "add_base_mass")
    assert (w["target"], w["op"], w["p0"], w["p1"]) == (R.MASS_WHEELS, R.ABS, R.f32(0.01), R.f32(0.3)) and (b["target"], b["op"]) == (R.MASS_BASE, R.ABS)
    assert flat.startup.wheel_mass == (0.0, 0.0)
    for task in ("Isaac-MushrElevationRL-v0", "Isaac-MushrVisualDepthRL-v0"):
        cfg = _cfg(task) if task.startswith("Isaac-MushrElev") else _visual_random(task)
        cfg.events.change_wheel_friction.mode = "interval"
        cfg.events.change_wheel_friction.interval_range_s = (0.5, 1.0)
        assert flatten_cfg(cfg).events.names == ("change_wheel_friction",)


def test_resolve_refusals_name_the_term():
    import torch
    from wheeledlab_amd.envs.flatten import flatten_cfg

    def refused(edit, task="Isaac-MushrDriftRL-v0", name=None, exc=ValueError):
        cfg = _visual_random(task) if "Visual" in task else _cfg(task)
        name = edit(cfg.events) or name
        with pytest.raises(exc, match=name):
            flatten_cfg(cfg)

    def friction(**kw):
        def edit(ev):
            ev.change_wheel_friction.mode = "reset"
            ev.change_wheel_friction.params.update(kw)
            return "change_wheel_friction"
        return edit

    def gains(**kw):
        def edit(ev):
            ev.randomize_gains.mode = "reset"
            ev.randomize_gains.params.update(kw)
            return "randomize_gains"
        return edit

    def mass(mode="reset", interval=None, **kw):
        def edit(ev):
            ev.add_base_mass.mode, ev.add_base_mass.interval_range_s = mode, interval
            ev.add_base_mass.params.update(kw)
            return "add_base_mass"
        return edit
    refused(friction(restitution_range=(0.0, 0.1)))
    refused(friction(static_friction_range=torch.tensor([0.3, 0.5])))
    refused(friction(dynamic_friction_range=(0.5, 0.3)))
    refused(friction(num_buckets=0))
    refused(friction(num_buckets=torch.tensor(4)))
    refused(gains(stiffness_distribution_params=(0.0, 10.0)))
    refused(gains(damping_distribution_params=np.array([10.0, 50.0])))
    refused(gains(damping_distribution_params=(torch.tensor(10.0), torch.tensor(50.0))))
    refused(gains(damping_distribution_params=(50.0, 10.0)))
    refused(gains(damping_distribution_params=(0.0, 10.0), distribution="log_uniform"))
    refused(gains(damping_distribution_params=(10.0, -1.0), distribution="gaussian"))
    refused(gains(distribution="normal"))
    refused(gains(operation="multiply"))
    refused(mass("interval", None))                                       # an interval term without interval_range_s
    refused(mass("interval", (0.0, 1.0)))
    refused(mass("interval", (2.0, 1.0)))
    refused(mass("interval", torch.tensor([1.0, 2.0])))
    refused(mass(mass_distribution_params=(float("nan"), 1.0)))

    def wheels_add(ev):
        ev.add_wheel_mass.mode = "reset"
        ev.add_wheel_mass.params["operation"] = "add"
        return "add_wheel_mass"
    refused(wheels_add, task="Isaac-MushrVisualRL-v0")
    # every other unsupported term still raises as before
    def push_reset(ev):
        ev.push_robots_hf.mode = "reset"
        return "push_robots_hf"
    refused(push_reset, exc=NotImplementedError)

    def unknown_mode(ev):
        ev.add_base_mass.mode = "prestartup"
        return "add_base_mass"
    refused(unknown_mode, exc=NotImplementedError)


def test_train_script_overrides_reach_the_table():
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs.flatten import flatten_cfg
    assert flatten_cfg(resolve_run("RSS_DRIFT_CONFIG", []).env).events is None
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.events.change_wheel_friction.mode=reset"])
    assert flatten_cfg(run.env).events.names == ("change_wheel_friction",)
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.events.add_base_mass.mode=interval", "env.events.add_base_mass.interval_range_s=(4.0,8.0)",
                                           "env.events.add_base_mass.params.mass_distribution_params=(0.1,0.2)"])
    m = _row(flatten_cfg(run.env).events, "add_base_mass")
    assert (m["mode"], m["interval_lo"], m["interval_hi"], m["p0"], m["p1"]) == (R.INTERVAL, 4.0, 8.0, R.f32(0.1), R.f32(0.2))
    # a dict override replaces the parameters as a whole
    run = resolve_run("RSS_ELEV_CONFIG", ["env.events.add_base_mass.mode=reset",
                                          "env.events.add_base_mass.params={'mass_distribution_params': (3.0, 0.2), 'operation': 'abs', 'distribution': 'gaussian'}"])
    m = _row(flatten_cfg(run.env).events, "add_base_mass")
    assert (m["target"], m["op"], m["dist"], m["p0"], m["p1"]) == (R.MASS_BASE, R.ABS, R.GAUSSIAN, 3.0, R.f32(0.2))
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.events.add_base_mass.mode=interval"])
    with pytest.raises(ValueError, match="add_base_mass"):
        flatten_cfg(run.env)

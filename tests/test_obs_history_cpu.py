"""CPU checks of the observation history: the two statements of the contract against each other (tests/obs_history_reference.py),
the header and its ctypes mirror, wl_obs_history_width on good and bad tables, every argument refusal of wl_obs_history_push before
any launch, the config resolution (envs/history.py), and the device index map compiled for the host as a stand-alone program
(tests/host_sim/obs_history_host.cpp) -- plain and under -fsanitize=address,undefined -- against the reference."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import obs_history_reference as R
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_history.h")
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(ROOT, "tests", "host_sim", "obs_history_host.cpp")


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def _ctable(tab):
    tab = np.asarray(tab, np.int32).reshape(-1, 4)
    return (A.WlObsHistoryTerm * max(len(tab), 1))(*[A.WlObsHistoryTerm(*(int(v) for v in t)) for t in tab])


# ---- the reference holds itself ----------------------------------------------------------------------------------------

def _reset_patterns(rng, K, n):
    r = rng.random((K, n)) < 0.2
    r[0, 0] = True                      # a reset on step 0
    r[5:8, 1] = True                    # resets on consecutive steps
    r[:, 2] = False                     # an env that never resets
    r[:, 3] = True                      # and one that always does
    return r


@pytest.mark.parametrize("name", list(R.TABLES))
def test_closed_form_and_deque_model_agree_over_40_steps(name):
    widths, frames = R.TABLES[name]
    tab, D, Dh = R.table(widths, frames)
    rng = np.random.default_rng(len(name) + D)
    K, n = 40, 6
    resets = _reset_patterns(rng, K, n)
    obs = R.special_words(rng, (K, n, D))
    model, prev = R.DequeModel(tab, n), None
    for k in range(K):
        want = model.push(obs[k], resets[k])
        prev = R.push_closed(tab, obs[k], prev, resets[k])
        assert prev.dtype == np.uint32 and prev.shape == (n, Dh)
        assert np.array_equal(prev, want), (name, k)
    # the never-reset env holds, oldest first, its last H frames of every term
    for s, w, h, d in tab:
        for f in range(h):
            assert np.array_equal(prev[2, d + f * w:d + (f + 1) * w], obs[K - h + f, 2, s:s + w])


def test_special_words_carry_what_arithmetic_would_lose():
    x = R.special_words(np.random.default_rng(0), (64, 64))
    f = x.view(np.float32)
    nan = np.isnan(f)
    assert nan.sum() > 100 and len(np.unique(x[nan])) > 100                       # distinct payloads
    assert ((x & 0x7FC00000) == 0x7F800000)[nan].any()                           # signalling ones among them
    assert (x == 0x80000000).any() and np.isinf(f).any() and ((x & 0x7F800000) == 0)[x & 0x007FFFFF != 0].any()


# ---- the C boundary --------------------------------------------------------------------------------------------------

def test_history_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.OBSHIST_SIGNATURES) == {"wl_obs_history_version", "wl_obs_history_width", "wl_obs_history_push"}
    others = set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES) | set(A.OBSNORM_SIGNATURES) | set(A.RAYCASTER_SIGNATURES)
    assert not declared & others
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_obs_history_version() == 1 == A.WL_OBSHIST_VERSION


def test_history_header_matches_the_ctypes_struct_and_the_step_boundary_is_unchanged(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_history.h"\n'
                     'int main(){printf("%d %d %d %d %d %d %d %d %d %d %d\\n", (int)WL_OBSHIST_VERSION, (int)WL_OBSHIST_MAX_TERMS, '
                     '(int)WL_OBSHIST_MAX_FRAMES, (int)WL_OBSHIST_MAX_DIM, (int)sizeof(WlObsHistoryTerm), (int)offsetof(WlObsHistoryTerm, src_off), '
                     '(int)offsetof(WlObsHistoryTerm, width), (int)offsetof(WlObsHistoryTerm, frames), (int)offsetof(WlObsHistoryTerm, dst_off), '
                     '(int)WL_ABI_VERSION, (int)WL_ABI_REVISION); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = A.WlObsHistoryTerm
    assert got == [A.WL_OBSHIST_VERSION, A.OBSHIST_MAX_TERMS, A.OBSHIST_MAX_FRAMES, A.OBSHIST_MAX_DIM, C.sizeof(T), T.src_off.offset,
                   T.width.offset, T.frames.offset, T.dst_off.offset, A.WL_ABI_VERSION, A.WL_ABI_REVISION]
    assert got[:5] == [1, 64, 64, 1 << 20, 16] and got[9:] == [24, 1]
    assert got[2] & (got[2] - 1) == 0                                          # a power of two


def test_width_accepts_good_tables_and_refuses_bad_ones():
    lib = _lib()

    def width(tab, D, n_terms=None):
        tab = np.asarray(tab, np.int32).reshape(-1, 4)
        return lib.wl_obs_history_width(_ctable(tab), len(tab) if n_terms is None else n_terms, D)
    for name, (widths, frames) in R.TABLES.items():
        tab, D, Dh = R.table(widths, frames)
        assert width(tab, D) == Dh, name
    assert [R.table(*R.TABLES[k])[2] for k in ("drift_h3", "elevation", "time_major")] == [42, 689 + 676, 56]
    good, D, _ = R.table([3, 3, 2], [2, 1, 4])
    assert width(good, D) == 6 + 3 + 8

    def bad(row, col, val):
        t = good.copy()
        t[row, col] = val
        return t
    for what, tab, d in (("gap", bad(1, 0, 4), D), ("overlap", bad(1, 0, 2), D), ("wrong dst_off", bad(2, 3, 8), D),
                         ("dst_off overlap", bad(1, 3, 5), D), ("frames 0", bad(0, 2, 0), D), ("frames above the maximum", bad(0, 2, 65), D),
                         ("negative frames", bad(2, 2, -1), D), ("width 0", bad(1, 1, 0), D), ("D too small", good, D - 1),
                         ("D too large", good, D + 1), ("D 0", good, 0), ("first term not at 0", bad(0, 0, 1), D)):
        assert width(tab, d) == -1, what
    assert width(good, D, n_terms=0) == -1 and lib.wl_obs_history_width(None, 3, D) == -1
    big, Db, Dhb = R.table([1] * 64, [2] * 64)
    assert width(big, Db) == Dhb == 128
    over, Do, _ = R.table([1] * 65, [2] * 65)
    assert width(over, Do) == -1                                              # n_terms 65
    top, Dt, Dht = R.table([5], [64])
    assert width(top, Dt) == Dht == 320


def test_push_refuses_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    tab, D, Dh = R.table(*R.TABLES["drift_h3"])
    ct = _ctable(tab)
    n = 64
    fake = 1 << 24                     # never dereferenced: every call below returns before any launch
    base = dict(n=n, D=D, obs=fake, stride=D, terms=ct, n_terms=len(tab), prev=fake + (1 << 20), next=fake + (2 << 20), ra=fake + (3 << 20),
                rb=fake + (3 << 20) + 4096)

    def push(**kw):
        a = {**base, **kw}
        return lib.wl_obs_history_push(a["n"], a["D"], a["obs"], a["stride"], a["terms"], a["n_terms"], a["prev"], a["next"], a["ra"], a["rb"], None)
    for k in ("obs", "next", "ra", "terms"):
        assert push(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(n=-1), dict(stride=D - 1), dict(D=D + 1), dict(D=0), dict(n_terms=0), dict(n_terms=len(tab) - 1), dict(n_terms=65)):
        assert push(**kw) == -1, kw
    row = n * Dh * 4
    for kw in (dict(prev=base["next"]), dict(prev=base["next"] + row - 4), dict(prev=base["next"] - row + 4),      # prev / next overlap
               dict(obs=base["next"]), dict(obs=base["next"] + row - 4)):                                        # obs / next overlap
        assert push(**kw) == -1, kw
    for k in ("obs", "prev", "next"):
        for off in (1, 2, 3):
            assert push(**{k: base[k] + off}) == -3, (k, off)
    assert push(n=(1 << 31) // Dh + 1, prev=None, next=1 << 40) == -1                                         # n * Dh past 2^31
    bad = tab.copy()
    bad[2, 2] = 0
    assert push(terms=_ctable(bad)) == -1
    # (the calls that ARE accepted -- adjacent rows, a NULL prev, a NULL reset_b, a strided obs, a `next` off the 16-byte line -- launch:
    # tests/test_gpu_obs_history.py makes them on real buffers)


# ---- config resolution -----------------------------------------------------------------------------------------------

def _group(task="Isaac-MushrDriftRL-v0"):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.envs.configclass import fields_of
    cfg = registry.parse_env_cfg(task, device="cpu", num_envs=4)
    pol = cfg.observations.policy
    return pol, [(k, v) for k, v in fields_of(pol) if hasattr(v, "func")]


def _widths(task):
    from wheeledlab_amd import core
    return list({"Isaac-MushrDriftRL-v0": core.DriftBatch, "Isaac-MushrElevationRL-v0": core.ElevBatch,
                 "Isaac-MushrVisualRL-v0": core.VisualBatch}[task].OBS_TERM_WIDTHS)


def test_config_fields_exist_with_their_defaults_and_off_resolves_to_nothing():
    from wheeledlab_amd.envs.history import resolve
    from wheeledlab_amd.envs.managers_cfg import ObservationGroupCfg, ObservationTermCfg
    t, g = ObservationTermCfg(func=len), ObservationGroupCfg()
    assert (t.history_length, t.flatten_history_dim) == (0, True) and (g.history_length, g.flatten_history_dim) == (None, True)
    for task in ("Isaac-MushrDriftRL-v0", "Isaac-MushrElevationRL-v0", "Isaac-MushrVisualRL-v0"):
        pol, terms = _group(task)
        assert len(terms) == len(_widths(task))
        assert resolve(pol, terms, _widths(task)) is None
        for h in (0, 1):                                                       # 0 and 1: one frame, nothing to build
            pol.history_length = h
            assert resolve(pol, terms, _widths(task)) is None


def test_group_history_gives_the_three_tasks_their_widths():
    from wheeledlab_amd import core
    from wheeledlab_amd.envs.history import resolve
    for task, D in (("Isaac-MushrDriftRL-v0", 14), ("Isaac-MushrElevationRL-v0", 689), ("Isaac-MushrVisualRL-v0", 3208)):
        assert sum(_widths(task)) == D
        pol, terms = _group(task)
        pol.history_length = 4
        L = resolve(pol, terms, _widths(task))
        assert (L.D, L.Dh, L.frames, L.shape) == (D, 4 * D, 0, (4 * D,)) and len(L.terms) == len(terms)
        tab, D2, Dh2 = R.table(_widths(task), [4] * len(terms))
        assert np.array_equal(np.asarray(L.terms), tab) and L.names == tuple(n for n, _ in terms)
    assert sum(core.VisualDepthBatch.OBS_TERM_WIDTHS) == core.VisualDepthBatch.OBS_DIM == 4808
    assert core.ElevBatch.OBS_TERM_WIDTHS == (2, 3, 3, 3, 2, 676) and core.DriftBatch.OBS_TERM_WIDTHS == (3, 3, 3, 3, 2)


def test_group_override_beats_term_values_and_mixed_term_lengths_resolve():
    from wheeledlab_amd.envs.history import resolve
    from wheeledlab_amd.envs.managers_cfg import ObservationTermCfg as ObsTerm
    pol, terms = _group()
    for (_, t), h in zip(terms, (1, 3, 5, 0, 3)):
        t.history_length = h
    L = resolve(pol, terms, _widths("Isaac-MushrDriftRL-v0"))
    tab, _, Dh = R.table(*R.TABLES["mixed"])
    assert np.array_equal(np.asarray(L.terms), tab) and L.Dh == Dh == 3 + 9 + 15 + 3 + 6 and L.shape == (Dh,)
    # a plugin term behind the fused layout takes part like any other
    pol.extra = ObsTerm(func=len, history_length=2)
    terms2 = terms + [("extra", pol.extra)]
    L2 = resolve(pol, terms2, _widths("Isaac-MushrDriftRL-v0") + [4])
    assert L2.Dh == Dh + 8 and L2.terms[-1] == (14, 4, 2, Dh)
    # the group's value overrides every term's, both fields
    terms[0][1].flatten_history_dim = False
    pol.history_length = 2
    L3 = resolve(pol, terms2, _widths("Isaac-MushrDriftRL-v0") + [4])
    assert L3.Dh == 2 * 18 and all(t[2] == 2 for t in L3.terms) and L3.frames == 0
    pol.flatten_history_dim = False                                            # time-major: one pseudo-term over the row
    L4 = resolve(pol, terms2, _widths("Isaac-MushrDriftRL-v0") + [4])
    assert L4.terms == ((0, 18, 2, 0),) and L4.shape == (2, 18) and L4.Dh == 36
    pol.history_length = 1
    assert resolve(pol, terms2, _widths("Isaac-MushrDriftRL-v0") + [4]) is None


def test_every_value_error_of_the_config():
    from wheeledlab_amd.envs.history import resolve
    w = _widths("Isaac-MushrDriftRL-v0")
    for bad in (-1, 65):
        pol, terms = _group()
        terms[2][1].history_length = bad
        with pytest.raises(ValueError, match=terms[2][0]):                     # names the term
            resolve(pol, terms, w)
        pol, terms = _group()
        pol.history_length = bad
        with pytest.raises(ValueError, match="policy"):
            resolve(pol, terms, w)
    pol, terms = _group()
    terms[1][1].history_length, terms[1][1].flatten_history_dim = 2, False
    with pytest.raises(ValueError, match=f"{terms[1][0]}.*concatenate_terms"):
        resolve(pol, terms, w)
    pol, terms = _group()
    terms[0][1].history_length = 2.5
    with pytest.raises(ValueError, match=terms[0][0]):
        resolve(pol, terms, w)


def test_train_script_override_reaches_the_group():
    from wheeledlab_amd.configs.runs import resolve_run
    run = resolve_run("RSS_DRIFT_CONFIG", ["env.observations.policy.history_length=4"])
    assert run.env.observations.policy.history_length == 4 and run.env.observations.policy.flatten_history_dim is True


# ---- the device index map on the host --------------------------------------------------------------------------------

def _build(out, *flags):
    cxx = CLANG if (os.path.exists(CLANG) or shutil.which(CLANG)) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler to build the host simulation")
    subprocess.run([cxx, "-O1", "-std=c++17", *flags, "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), SRC, "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_sim") / "obs_history_host")


def run_host(exe, tmp, tab, D, obs, prev, ra, rb, shift=0, env=None):
    n, stride = obs.shape
    tab = np.asarray(tab, np.int32).reshape(-1, 4)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", n, D, stride, len(tab), int(prev is not None), int(rb is not None), shift))
        f.write(tab.tobytes())
        f.write(np.ascontiguousarray(obs, np.uint32).tobytes())
        if prev is not None:
            f.write(np.ascontiguousarray(prev, np.uint32).tobytes())
        f.write(np.ascontiguousarray(ra, np.uint8).tobytes())
        if rb is not None:
            f.write(np.ascontiguousarray(rb, np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, env=env)
    raw = open(fout, "rb").read()
    Dh = struct.unpack("<q", raw[:8])[0]
    if Dh < 0:
        assert len(raw) == 8
        return None
    m = n * Dh
    nxt = np.frombuffer(raw[8:8 + 4 * m], np.uint32).reshape(n, Dh)
    writes = np.frombuffer(raw[8 + 4 * m:8 + 5 * m], np.uint8).reshape(n, Dh)
    whole = struct.unpack("<q", raw[8 + 5 * m:])[0]
    return nxt, writes, whole


def _case(name, n, seed, stride_extra=0):
    tab, D, Dh = R.table(*R.TABLES[name])
    rng = np.random.default_rng(seed)
    obs = R.special_words(rng, (n, D + stride_extra))
    prev = R.special_words(rng, (n, Dh))
    ra, rb = rng.random(n) < 0.3, rng.random(n) < 0.2
    return tab, D, Dh, obs, prev, ra, rb


def _check_host(exe, tmp, name, n, shift, with_prev=True, with_b=True, stride_extra=0, env=None):
    tab, D, Dh, obs, prev, ra, rb = _case(name, n, seed=n + shift + len(name), stride_extra=stride_extra)
    got = run_host(exe, tmp, tab, D, obs, prev if with_prev else None, ra, rb if with_b else None, shift, env=env)
    nxt, writes, whole = got
    want = R.push_closed(tab, obs, prev if with_prev else None, ra | rb if with_b else ra)
    assert np.array_equal(nxt, want), (name, n, shift)
    assert (writes == 1).all()                                                 # every output produced exactly once
    total = n * Dh
    assert whole == max(0, (total + shift) // 4 - (1 if shift else 0))                # all lines but a partial head and tail go out whole


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(R.TABLES))
def test_host_index_map_equals_the_reference(exe, tmp_path, name, shift):
    for n in (1, 3, 65):
        _check_host(exe, str(tmp_path), name, n, shift)
    _check_host(exe, str(tmp_path), name, 5, shift, with_prev=False)
    _check_host(exe, str(tmp_path), name, 5, shift, with_b=False, stride_extra=3)


def test_host_program_refuses_a_bad_table(exe, tmp_path):
    tab, D, Dh, obs, prev, ra, rb = _case("drift_h3", 2, 1)
    tab = tab.copy()
    tab[3, 3] += 1
    assert run_host(exe, str(tmp_path), tab, D, obs, prev, ra, rb) is None


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path / "obs_history_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for name in R.TABLES:
        for n, shift in ((1, 0), (3, 3), (65, 1)):
            _check_host(exe, str(tmp_path), name, n, shift, env=env)
        _check_host(exe, str(tmp_path), name, 4, 2, with_prev=False, with_b=False, stride_extra=5, env=env)

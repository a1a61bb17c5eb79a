"""The observation normaliser's device arithmetic (wheeledlab_amd/csrc/wl_obs_norm_dev.h: moments of one element, the merge, the
folded first layer, the launch plan) compiled for the host as a stand-alone program (tests/host_sim/obs_norm_host.cpp) and held
against the float64 reference (tests/obs_norm_reference.py) on the shapes of the GPU test -- and the same program built with
-fsanitize=address,undefined."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import obs_norm_reference as R

CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(ROOT, "tests", "host_sim", "obs_norm_host.cpp")
H = 64


def _build(out, *flags):
    cxx = CLANG if (os.path.exists(CLANG) or shutil.which(CLANG)) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler to build the host simulation")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), SRC, "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("host_sim") / "obs_norm_host")


def run(exe, tmp, x, mean0, var0, count0, w1, b1, until=R.UNTIL, merges=1, env=None):
    """x [rows, stride] fp32 (the first D = len(mean0) columns are features) -> the program's outputs as a dict"""
    rows, stride = x.shape
    D = len(mean0)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7q", rows, D, H, stride, count0, until, merges) + struct.pack("<d", R.EPS))
        for a in (mean0, var0, x, w1, b1):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.run([exe, fin, fout], check=True, env=env)
    raw = open(fout, "rb").read()
    off = 0

    def take(dt, *shape):
        nonlocal off
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        a = np.frombuffer(raw[off:off + n], dt).reshape(shape)
        off += n
        return a
    got = dict(sums=take(np.float64, 2, D), mean=take(np.float32, D), var=take(np.float32, D), std=take(np.float32, D),
               inv_std=take(np.float32, D), count=int(take(np.int64, 1)[0]), out=take(np.float32, rows, stride)[:, :D],
               w1_out=take(np.float32, H, D), b1_out=take(np.float32, H), plan=take(np.int64, 3))
    assert off == len(raw)
    return got


def case(rows, D, stride, warm, seed):
    x, _, _ = R.inputs(rows, D, seed)
    mean0, var0, count0 = R.state(D, seed, warm)
    rng = np.random.default_rng(seed + 7)
    w1 = (rng.uniform(-1, 1, (H, D)) / np.sqrt(D)).astype(np.float32)
    b1 = (rng.uniform(-1, 1, H) / np.sqrt(D)).astype(np.float32)
    xs = x
    if stride is not None:
        xs = rng.normal(size=(rows, stride)).astype(np.float32)
        xs[:, :D] = x
    return x, xs, mean0, var0, count0, w1, b1


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("rows,D,stride", R.SHAPES, ids=[f"{r}x{d}" + (f"s{s}" if s else "") for r, d, s in R.SHAPES])
def test_host_arithmetic_matches_the_reference(exe, tmp_path, rows, D, stride, warm):
    x, xs, mean0, var0, count0, w1, b1 = case(rows, D, stride, warm, seed=100 + rows + D)
    got = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1)
    R.check(got, x, mean0, var0, count0, w1, b1, label=f"host {rows}x{D} {'warm' if warm else 'cold'}")
    narrow, partials, per = (int(v) for v in got["plan"])
    assert narrow == int(D < 64 and stride is None) and partials >= 1
    if narrow:      # every wave-load of 64 // D rows lies in exactly one wavefront's share
        assert partials * 4 * per >= -(-rows // (64 // D)) > (partials - 1) * 4 * per
    else:           # every row lies in exactly one chunk
        assert partials * per >= rows > (partials - 1) * per


def test_host_until_stops_the_updates_and_leaves_the_bits(exe, tmp_path):
    x, xs, mean0, var0, count0, w1, b1 = case(130, 14, None, True, seed=5)
    got = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1, until=count0)
    assert got["count"] == count0 and got["mean"].tobytes() == mean0.tobytes() and got["var"].tobytes() == var0.tobytes()
    got = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1, until=count0 + 1)      # below `until` before the batch: merged whole
    assert got["count"] == count0 + 130


def test_host_sequential_merges_equal_the_pooled_one(exe, tmp_path):
    """K = 8 merges of n = 96 rows against the reference's 8 sequential updates (2 ulp) and against ONE merge of the 768 rows (1e-6)"""
    x, xs, mean0, var0, count0, w1, b1 = case(768, 14, None, False, seed=9)
    seq = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1, merges=8)
    one = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1)
    mean, var, count = R.sequential(mean0, var0, count0, x.reshape(8, 96, 14))
    # every intermediate state is rounded to fp32 (8 roundings of <= 0.5 ulp on top of the 2-ulp bar of one merge)
    for k, want in (("mean", mean), ("var", var)):
        ok, worst = R.within_ulps(seq[k], want, 2 + 4)
        assert ok, (k, worst)
        rel = np.abs(R.f64(seq[k]) - R.f64(one[k])) / np.maximum(np.abs(R.f64(one[k])), 1e-30)
        assert rel.max() <= 1e-6, (k, rel.max())
    assert seq["count"] == one["count"] == count == 768


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path / "obs_norm_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for rows, D, stride in ((5, 14, None), (130, 65, None), (130, 64, 80)):
        x, xs, mean0, var0, count0, w1, b1 = case(rows, D, stride, True, seed=3)
        got = run(exe, str(tmp_path), xs, mean0, var0, count0, w1, b1, env=env)
        R.check(got, x, mean0, var0, count0, w1, b1, label=f"sanitized {rows}x{D}")

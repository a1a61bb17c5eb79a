"""Terrain samplers on heightfields unlike the bench one (tests/heightfield_cases.py: non-square, off-centre, coarse and fine cells,
sloped borders, non-zero outside_z, one- and two-cell fields, a 32 800-point strip) against the float64 restatement
(tests/heightfield_reference.py).  On CPU: the oracle's `sample` / `height_map`, and the DEVICE contact samplers of wl_heightfield.h
compiled for the host (tests/host_sim/vehicle_host.cpp::hs_heightfield_probe) -- once plainly, once under AddressSanitizer and
UndefinedBehaviorSanitizer, which shows that no read leaves the code or row-pair table, G5's far end included.
Mutations of wl_heightfield.h these tests were seen to catch (the pre-existing suite passes with each):
  * nx and ny swapped in sample_full's index and inside test -- test_device_contact_samplers_against_float64 on G1 - G3, G4b, G5 and
    the sanitizer build;
  * outside_z ignored by sample_full (0 beyond the grid) -- test_device_contact_samplers_against_float64 on G1, G2, G4a, G4b."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import elev_step as OE
from oracle import heightfield as OH
from tests import heightfield_cases as HC
from tests import heightfield_reference as R
from tests.depth_cases import hf_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
F = np.float32
PROBED = ["G1", "G2", "G3", "G4a", "G4b", "G5"]
ALL = PROBED + ["G6"]


def _points(field, n, seed, margin=2.0):
    """uniform points reaching `margin` m beyond every border, points straddling each border line and corner, and grid points"""
    rng = np.random.RandomState(seed)
    xl, xh, yl, yh = field.extent()
    x = rng.uniform(xl - margin, xh + margin, n)
    y = rng.uniform(yl - margin, yh + margin, n)
    k = n // 4
    side = rng.randint(0, 4, k)
    t = rng.uniform(0, 1, k)
    d = rng.normal(0, 2 * field.cell, k)
    x[:k] = np.where(side < 2, np.where(side == 0, xl, xh) + d, xl + t * (xh - xl))
    y[:k] = np.where(side < 2, yl + t * (yh - yl), np.where(side == 2, yl, yh) + d)
    corner = rng.randint(0, 4, k // 4)
    x[k:k + k // 4] = np.where(corner & 1, xh, xl) + rng.normal(0, field.cell, k // 4)
    y[k:k + k // 4] = np.where(corner & 2, yh, yl) + rng.normal(0, field.cell, k // 4)
    m = k // 2
    i, j = rng.randint(0, field.nx, m), rng.randint(0, field.ny, m)
    x[2 * k:2 * k + m] = field.x0 + i * field.cell
    y[2 * k:2 * k + m] = field.y0 + j * field.cell
    return x.astype(F), y.astype(F)


def _check_contact(field, x, y, z, n, inside, where):
    """a contact sampler's z / normal / inside [N] against sample64(guard=True) -> (excused normals, excused inside flips)"""
    zr, nr, ir = R.sample64(field, x, y, guard=True)
    ztol, ntol, _, ex_n, ex_in = R.contact_bounds(field, x, y)
    flip = (np.asarray(inside, bool) != ir)
    assert not (flip & ~ex_in).any(), (where, int((flip & ~ex_in).sum()))
    ok = ~flip
    dz = np.abs(np.asarray(z, np.float64) - zr)
    bad = ok & (dz > ztol)
    assert not bad.any(), (where, int(bad.sum()), float(dz[bad].max()), x[bad][:3], y[bad][:3])
    dn = np.abs(np.asarray(n, np.float64) - nr).max(-1)
    badn = ok & ~ex_n & (dn > ntol)
    assert not badn.any(), (where, int(badn.sum()), float(dn[badn].max()))
    return int((ok & ex_n & (dn > ntol)).sum()), int(flip.sum())


@pytest.mark.parametrize("name", ALL)
def test_oracle_sample_and_height_map_against_float64(name):
    """the oracle's contact sampler (guard, outside_z) and its height scan (no guard, misses) hold the float64 definitions on every
    geometry -- G5's far end too, where the guard vanishes in fp32 and the oracle used to index past the grid"""
    f = HC.get(name)
    x, y = _points(f, 20000, seed=len(name) + 7)
    z, n, inside = OH.sample(f.heights, F(f.x0), F(f.y0), F(f.cell), x, y, outside=f.outside_z)
    ex = _check_contact(f, x, y, z, n, inside, name)
    print(f"{name}: oracle sample, excused normals / inside flips {ex}")
    assert (inside.mean() > 0.05 or name.startswith("G4")) and (~inside).any()
    assert (z[~inside] == F(f.outside_z)).all()
    # height scan: poses anywhere, on and beyond the borders, any yaw, some tilted
    p = OE.elev_params()
    m = 400
    st = np.zeros((41, m), F)
    st[0], st[1] = _points(f, m, seed=3)
    rng = np.random.RandomState(4)
    st[2] = rng.uniform(-0.5, 1.5, m)
    q = rng.normal(size=(4, m))
    q[1:3] *= 0.15
    st[3:7] = (q / np.linalg.norm(q, axis=0)).astype(F)
    got = OE.height_map(p, st, f.oracle())
    n_ex = R.check_scan(got, p, st, f, where=name)
    print(f"{name}: oracle height_map, {n_ex} border rays excused of {got.size}")
    hit = got < 10
    assert hit.any() and (~hit).any()


def test_guard_is_what_separates_the_scan_from_the_contacts():
    """G1 rises with a slope of 1 through its far borders: within 1e-3 cell of them the guarded (contact) and guard-free (scan)
    definitions differ by up to 1e-3 cell x 0.1 m x 1 = 1e-4 m, more than the scan's bound there (2e-5 m + the slope times the
    position error) -- which is why the scan is held to the guard-free definition, the one wl_elev_scan_dev.h implements"""
    f = HC.get("G1")
    v = np.linspace(0.5, f.ny - 1.5, 4001)
    u = np.full_like(v, f.nx - 1 - 1e-6)
    zg, _, _ = R.bilinear64(f, u, v, guard=True)
    zs, _, _ = R.bilinear64(f, u, v, guard=False)
    tol = R.SCAN_ABS + R.slope_map(f)[0][-1].max() * f.cell * R.pos_err(f, f.extent()[1], f.extent()[3])
    assert np.abs(zg - zs).max() > tol, (float(np.abs(zg - zs).max()), float(tol))


# ---- the device contact samplers compiled for the host ------------------------------------------------------------------------

def _build(out, sanitize=False):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host simulation")
    srcs = [os.path.join(ROOT, "tests", "host_sim", "vehicle_host.cpp")]
    flags = ["-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
             "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc")]
    if sanitize:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
        srcs.append(os.path.join(ROOT, "tests", "host_sim", "heightfield_probe_main.cpp"))
    else:
        flags += ["-fPIC", "-shared"]
    subprocess.run([CLANG, *flags, *srcs, "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module")
def probe_lib(tmp_path_factory):
    lib = C.CDLL(str(_build(tmp_path_factory.mktemp("hf_probe") / "libwl_hf_probe.so")))
    lib.hs_heightfield_probe.restype = None
    return lib


def _wheel_paths(field, n_paths, n_pts, seed):
    """straight wheel paths of ~0.37 cell per sample through a point of the border (corners included) or of the field, at any heading:
    every path crosses cell lines, and most cross a border line"""
    rng = np.random.RandomState(seed)
    xl, xh, yl, yh = field.extent()
    t = rng.uniform(0, 1, n_paths)
    side = rng.randint(0, 6, n_paths)
    ax = np.select([side == 0, side == 1, side == 4], [np.full(n_paths, xl), np.full(n_paths, xh), rng.uniform(xl, xh, n_paths)],
                   xl + t * (xh - xl))
    ay = np.select([side == 2, side == 3, side == 4], [np.full(n_paths, yl), np.full(n_paths, yh), rng.uniform(yl, yh, n_paths)],
                   yl + t * (yh - yl))
    c = np.arange(0, n_paths, 11)
    ax[c], ay[c] = np.where(rng.rand(len(c)) < 0.5, xl, xh), np.where(rng.rand(len(c)) < 0.5, yl, yh)
    ang = rng.uniform(-np.pi, np.pi, n_paths)
    ang[::7] = np.round(ang[::7] / (np.pi / 2)) * (np.pi / 2)          # along the lattice
    s = (np.arange(n_pts) - n_pts / 2) * 0.37 * field.cell
    x = ax[:, None] + np.cos(ang)[:, None] * s[None]
    y = ay[:, None] + np.sin(ang)[:, None] * s[None]
    return np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)


def _probe(lib, field, x, y):
    hs, keep = hf_struct((field.heights, field.x0, field.y0, field.cell), field.outside_z, field.z_scale)
    assert np.array_equal(keep[0], field.codes)
    n_paths, n_pts = x.shape
    z, zc = np.zeros_like(x), np.zeros_like(x)
    nrm, nc = np.zeros(x.shape + (3,), F), np.zeros(x.shape + (3,), F)
    inside = np.zeros(x.shape, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.hs_heightfield_probe(C.byref(hs), n_paths, n_pts, ptr(x), ptr(y), ptr(z), ptr(nrm), ptr(inside), ptr(zc), ptr(nc))
    return z, nrm, inside.astype(bool), zc, nc


@pytest.mark.parametrize("name", PROBED)
def test_device_contact_samplers_against_float64(probe_lib, name):
    """HeightFieldGround::sample_full and the lane form's HeightFieldGroundCached (four wheels per sampler, each keeping its cell)
    along wheel paths over cell lines and every border: heights and normals within the derived bound of sample64(guard=True),
    outside_z beyond the grid, and the cached form bit for bit the uncached one"""
    f = HC.get(name)
    x, y = _wheel_paths(f, 64, 600, seed=sum(map(ord, name)))
    z, n, inside, zc, nc = _probe(probe_lib, f, x, y)
    assert np.array_equal(z.view(np.int32), zc.view(np.int32)) and np.array_equal(n.view(np.int32), nc.view(np.int32)), name
    ex = _check_contact(f, x.ravel(), y.ravel(), z.ravel(), n.reshape(-1, 3), inside.ravel(), name)
    print(f"{name}: device contact samplers, excused normals / inside flips {ex} of {x.size} points")
    assert inside.any() and (~inside).any() and (z[~inside] == F(f.outside_z)).all()
    assert (n[~inside] == F([0, 0, 1])).all()


def test_device_contact_samplers_under_sanitizers(probe_lib, tmp_path):
    """the same probe built with -fsanitize=address,undefined around tables of exactly nx * ny codes / pairs: no read leaves them
    on any geometry -- including the far end of G5, where the guard vanishes and the cell index reaches nx - 1 -- and the results
    are the plain build's bit for bit"""
    exe = _build(tmp_path / "hf_probe_asan", sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in PROBED:
        f = HC.get(name)
        x, y = _wheel_paths(f, 16, 300, seed=5)
        if name == "G5":        # straight over the far end, on every row of the strip
            xs = (f.extent()[1] + np.linspace(-3, 3, 300)).astype(F)
            for r in range(16):
                x[r] = xs
                y[r] = F(f.y0 + (r / 15.0) * (f.ny - 1) * f.cell * 1.1 - 0.01)
        inp, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
        with open(inp, "wb") as fh:
            np.array([f.nx, f.ny, x.shape[0], x.shape[1]], np.int32).tofile(fh)
            np.array([f.x0, f.y0, f.cell, f.outside_z, f.z_scale], F).tofile(fh)
            np.ascontiguousarray(f.codes, np.int16).tofile(fh)
            x.tofile(fh)
            y.tofile(fh)
        r = subprocess.run([str(exe), str(inp), str(out)], env=env, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        k = x.size
        raw = np.fromfile(out, np.uint8)
        assert raw.size == 32 * k + k
        fl = raw[:32 * k].view(F)
        z, nrm, zc, nc = fl[:k], fl[k:4 * k], fl[4 * k:5 * k], fl[5 * k:]
        want = _probe(probe_lib, f, x, y)
        assert np.array_equal(z.view(np.int32), want[0].ravel().view(np.int32)) and np.array_equal(zc.view(np.int32), want[3].ravel().view(np.int32))
        assert np.array_equal(nrm.view(np.int32), want[1].ravel().view(np.int32)) and np.array_equal(nc.view(np.int32), want[4].ravel().view(np.int32))
        assert np.array_equal(raw[32 * k:].astype(bool), want[2].ravel())

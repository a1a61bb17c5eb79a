"""The viewer camera's DEVICE functions (wheeledlab_amd/csrc/wl_viewer_dev.h) compiled for the host (tests/host_sim/viewer_host.cpp)
and held against the float64 restatement (tests/viewer_reference.py) without a GPU: a brute-force serial frame (no binning, no cull)
must leave zero unexplained pixels (viewer_reference.acceptable / check_explained) on the plane with the checker and with the visual
task's map, on the depth-case terrain with cars, on a crowded pile and with the eye 5 cm from a chassis; and the single functions --
ray / sphere and ray / box algebra, the tie rule, the map lookup, the checker, the 8-bit quantisation -- against closed forms."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_cases as DC
import viewer_reference as VR
from oracle import visual_mdp as OVM
from oracle.mathlib import quat_from_euler_xyz
from wheeledlab_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")


def _build(tmp_path_factory, contract):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host simulation")
    out = tmp_path_factory.mktemp("host_sim") / f"libwl_viewer_host_{contract}.so"
    # -ffp-contract=off: every product rounded, an independent rounding pattern of the device source (the kernels contract to fma);
    # the "fast" build rounds as hipcc's default contraction does
    subprocess.run([CLANG, "-O1", "-std=c++17", f"-ffp-contract={contract}", "-fPIC", "-shared",
                    "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"), "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_sim", "viewer_host.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    vp = C.c_void_p
    lib.hs_viewer_render.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.hs_viewer_sphere_t.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    lib.hs_viewer_box_t.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
    lib.hs_viewer_wins.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    lib.hs_viewer_traversable.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.hs_viewer_checker.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.hs_viewer_q8.argtypes = [C.c_int, vp, vp]
    for f in ("hs_viewer_sphere_t", "hs_viewer_box_t", "hs_viewer_wins", "hs_viewer_traversable", "hs_viewer_checker", "hs_viewer_q8"):
        getattr(lib, f).restype = None
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _build(tmp_path_factory, "off")


@pytest.fixture(scope="module")
def lib_fma(tmp_path_factory):
    return _build(tmp_path_factory, "fast")


def _ptr(a):
    return a.ctypes.data


def _params(w, h, eye, lookat, ground=A.VIEWER_PLANE, **kw):
    from wheeledlab_amd.viewer import viewer_params
    p = viewer_params(w, h, eye, lookat, ground=ground)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _host_render(lib, p, pos, quat, field=None, trav=None):
    pos = np.ascontiguousarray(pos, np.float32)
    quat = np.ascontiguousarray(quat, np.float32)
    H, W = p.height, p.width
    rgb, depth, ids = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W), np.int32)
    keep = []
    hfs = m = None
    if field is not None:
        hfs, keep = DC.hf_struct(field)
    if trav is not None:
        mp = np.ascontiguousarray(trav[0], np.uint8)
        keep.append(mp)
        m = A.WlTravMap(mp.ctypes.data, None, mp.shape[0], mp.shape[1], 0, float(trav[1]), float(trav[2]), None)
    rc = lib.hs_viewer_render(C.byref(p), C.byref(hfs) if hfs is not None else None, C.byref(m) if m is not None else None, len(pos),
                              _ptr(pos), _ptr(quat), _ptr(rgb), _ptr(depth), _ptr(ids))
    assert rc == 0
    return rgb, depth, ids


def _random_cars(n, seed, span, z=(0.0, 0.3)):
    rng = np.random.RandomState(seed)
    pos = np.zeros((n, 3), np.float32)
    pos[:, :2] = rng.uniform(-span, span, (n, 2))
    pos[:, 2] = rng.uniform(*z, n)
    eul = np.stack([rng.normal(0, 0.1, n), rng.normal(0, 0.1, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    return pos, np.ascontiguousarray(quat_from_euler_xyz(eul[:, 0], eul[:, 1], eul[:, 2]).astype(np.float32))


def _crowded(n=1500, seed=4):
    """the pile of tests/test_gpu_viewer.py::test_crowded_tiles_and_near_cars_are_complete"""
    rng = np.random.RandomState(seed)
    pos = np.zeros((n, 3), np.float32)
    k = n * 7 // 15
    pos[:k, :2] = rng.uniform(-0.05, 0.05, (k, 2))
    pos[k:, :2] = rng.uniform(-3, 3, (n - k, 2))
    pos[:, 2] = rng.uniform(0.0, 0.3, n)
    quat = quat_from_euler_xyz(np.zeros(n, np.float32), np.zeros(n, np.float32), rng.uniform(-np.pi, np.pi, n).astype(np.float32))
    return pos, np.ascontiguousarray(quat.astype(np.float32))


def _map():
    from wheeledlab_amd.travmap import generate_traversability_map
    return generate_traversability_map(rng=np.random.RandomState(1)).astype(np.uint8), 0.5, 0.5


def _scenes():
    """(name, params, pos, quat, field for the host (or None), hf tuple for the reference (or None), trav)"""
    field = DC.on_lattice(DC.terrain())
    hf = (field[0], field[1], field[2], field[3], 0.0)
    out = []
    pos, quat = _random_cars(48, 1, 3.0)
    out.append(("plane checker", _params(128, 72, (4.0, -4.0, 4.0), (0.0, 0.0, 0.0)), pos, quat, None, None, None))
    pos, quat = _random_cars(96, 2, 6.0)
    out.append(("plane trav map", _params(128, 72, (40.0, 0.0, 45.0), (0.0, 0.0, -3.0)), pos, quat, None, None, _map()))
    pos, quat = DC.poses(96, 11, field)
    for eye in ((20.0, -20.0, 20.0), (6.0, -6.0, 5.0)):
        out.append((f"terrain {eye}", _params(128, 72, eye, (0.0, 0.0, 0.0), ground=A.VIEWER_HEIGHTFIELD), pos, quat, field, hf, None))
    pos, quat = _crowded()
    for eye in ((25.0, -25.0, 20.0), (1.2, -1.2, 0.8)):
        out.append((f"crowded {eye}", _params(96, 54, eye, (0.0, 0.0, 0.0)), pos, quat, None, None, None))
    # the eye 5 cm from the chassis' +x face (box centre 0.09 m up, half extents 0.22, 0.10, 0.045), looking back at it
    pos = np.array([[0.0, 0.0, 0.0], [0.6, 0.3, 0.0]], np.float32)
    quat = np.array([[1.0, 0.0, 0.0, 0.0], [0.92387953, 0.0, 0.0, 0.38268343]], np.float32)
    out.append(("eye 5 cm from a chassis", _params(96, 54, (0.27, 0.02, 0.1), (0.0, 0.0, 0.08)), pos, quat, None, None, None))
    return out


SCENES = _scenes()


@pytest.mark.parametrize("k", range(len(SCENES)), ids=[s[0] for s in SCENES])
def test_host_frame_has_no_unexplained_pixel(lib, k):
    name, p, pos, quat, field, hf, trav = SCENES[k]
    got = _host_render(lib, p, pos, quat, field, trav)
    counts = VR.check_explained(got, VR.acceptable(p, pos, quat, hf, trav), name)
    assert (got[2] >= 0).sum() > 20, name                     # cars in view
    if name.startswith("eye 5 cm"):
        assert (got[2] == 0).mean() > 0.5 and counts["n"] == 96 * 54


def test_fp32_ray_spread_is_below_delta(lib, lib_fma):
    """the measurement behind viewer_reference.DELTA: every pixel of all seven host scenes is explained with a principal-point shift of
    1e-4 px, for the host build without contraction and with fma contraction (hipcc's default for device code) -- DELTA = 1e-3 px keeps
    a factor of ten.  This is the host compiler's rounding of the device source; the device's own arithmetic is held at DELTA by the GPU
    tests (tests/test_gpu_viewer.py, tests/test_gpu_viewer_edges.py)"""
    for build in (lib, lib_fma):
        for name, p, pos, quat, field, hf, trav in SCENES:
            got = _host_render(build, p, pos, quat, field, trav)
            VR.check_explained(got, VR.acceptable(p, pos, quat, hf, trav, delta=1e-4), name + " at 1e-4 px")
    with pytest.raises(AssertionError):
        VR.acceptable(p, pos, quat, delta=2e-3)


def _sphere_t(lib, o, d, c, r):
    o, d, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (len(r), 3))) for a in (o, d, c))
    r = np.ascontiguousarray(r, np.float32)
    t = np.zeros(len(r), np.float32)
    lib.hs_viewer_sphere_t(len(r), _ptr(o), _ptr(d), _ptr(c), _ptr(r), _ptr(t))
    return t


def _sphere_root(o, d, c, r):
    """the near root in float64 from the float32 inputs; nan: none ahead of an outside origin"""
    o, d, c, r = (np.asarray(a, np.float32).astype(np.float64) for a in (o, d, c, r))
    oc = o - c
    a, b, cc = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum(-1) - r * r
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / a
    return np.where((disc >= 0) & (cc > 0) & (b < 0), t, np.nan)


def test_sphere_t_small_far_spheres_grazing_rays_and_inside(lib):
    rng = np.random.RandomState(0)
    n = 4000
    # a 5 cm wheel 20 .. 80 m off, rays through random points of its disc (the cancellation of the textbook discriminant)
    dist = rng.uniform(20.0, 80.0, n)
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    c = (dirn * dist[:, None]).astype(np.float32)
    r = np.full(n, 0.05, np.float32)
    aim = c + (rng.uniform(-0.049, 0.049, (n, 3))).astype(np.float32)
    d = (aim / np.linalg.norm(aim, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)   # |d| != 1
    o = np.zeros((n, 3), np.float32)
    got, want = _sphere_t(lib, o, d, c, r), _sphere_root(o, d, c, r)
    hit = np.isfinite(want)
    assert hit.mean() > 0.5
    # where both see the sphere, the distance is good to 1e-6 relative (measured 2.5e-7: a few fp32 ulps of t, not of t^2 -- the
    # stable form).  A hit on one side only within 1e-5 relative of the silhouette.
    both = hit & (got > 0)
    rel = np.abs(got[both] - want[both]) / want[both]
    print("sphere_t: max relative error", rel.max(), "of", both.sum())
    assert rel.max() < 1e-6, rel.max()
    oc = o.astype(np.float64) - c
    dd = d.astype(np.float64)
    miss_dist = np.linalg.norm(np.cross(dd / np.linalg.norm(dd, axis=1, keepdims=True), oc), axis=1)
    disagree = hit != (got > 0)
    assert (np.abs(miss_dist[disagree] - 0.05) < 1e-5 * 0.05 * dist[disagree]).all()
    # grazing: rays passing at 0.05 (1 -+ 1e-4) from the centre: hit inside, miss outside
    for s, want_hit in ((1 - 1e-4, True), (1 + 1e-4, False)):
        c1 = np.array([[30.0, 0.05 * s, 0.0]], np.float32)
        t = _sphere_t(lib, [[0, 0, 0]], [[1, 0, 0]], c1, [0.05])
        assert (t[0] > 0) == want_hit, (s, t)
        if want_hit:
            assert abs(t[0] - _sphere_root([0, 0, 0], [1, 0, 0], c1[0], 0.05)) < 2e-3       # sqrt of a grazing disc: |dt| ~ r sqrt(2 eps)
    # origin inside the sphere (at its centre's side, and a hair inside its surface looking in), and a sphere behind: no hit
    t = _sphere_t(lib, [[0.0, 0, 0], [0.0499, 0, 0], [0, 0, 0]], [[1.0, 0, 0], [-1, 0, 0], [1, 0, 0]],
                  [[0.01, 0.02, 0.0], [0, 0, 0], [-3, 0, 0]], [0.05, 0.05, 0.05])
    assert (t < 0).all(), t


def _box_t(lib, o, d, c, h):
    n = len(o)
    o, d, c, h = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (n, 3))) for a in (o, d, c, h))
    t, ax = np.zeros(n, np.float32), np.zeros(n, np.int32)
    lib.hs_viewer_box_t(n, _ptr(o), _ptr(d), _ptr(c), _ptr(h), _ptr(t), _ptr(ax))
    return t, ax


def test_box_t_zero_components_faces_and_inside(lib):
    c, h = [0.0, 0.0, 0.09], [0.22, 0.10, 0.045]
    # axis-aligned rays (two exactly zero components: the 1e30 branch) entering each face; inside vs outside the zero slabs
    o = [[-2.0, 0.05, 0.1], [2.0, -0.05, 0.1], [0.1, -3.0, 0.06], [0.1, 3.0, 0.12], [0.0, 0.0, 4.0], [0.1, 0.0, -1.0],
         [-2.0, 0.2, 0.1], [0.0, 0.0, 0.2]]
    d = [[1.0, 0, 0], [-2.0, 0, 0], [0, 1.0, 0], [0, -0.5, 0], [0, 0, -1.0], [0, 0, 1.0], [1.0, 0, 0], [0, 0, 1.0]]
    t, ax = _box_t(lib, o, d, [c] * 8, [h] * 8)
    want_t = [2.0 - 0.22, (2.0 - 0.22) / 2, 3.0 - 0.10, (3.0 - 0.10) / 0.5, 4.0 - 0.135, 1.0 + 0.045]
    np.testing.assert_allclose(t[:6], want_t, rtol=1e-6)
    assert ax[:6].tolist() == [0, 0, 1, 1, 2, 2]
    assert t[6] < 0               # outside the y slab (0.2 > 0.10) with d.y == 0: the slab lies entirely to the side
    assert t[7] < 0               # the box is behind
    # origin ON a slab face looking in (tn = 0 is not ahead: no hit), and origin inside the box: no hit
    t, _ = _box_t(lib, [[-0.22, 0.0, 0.09], [0.0, 0.0, 0.09], [0.1, -0.05, 0.1]], [[1.0, 0, 0], [1.0, 0.3, 0.1], [0, 0, -1.0]], [c] * 3,
                  [h] * 3)
    assert (t < 0).all(), t
    # an oblique ray: the face entered is the slab with the largest entry parameter
    rng = np.random.RandomState(1)
    n = 2000
    o = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    o[np.all(np.abs(o - np.array(c, np.float32)) < np.array(h, np.float32) + 0.01, axis=1)] += 1.0
    tgt = (np.array(c) + rng.uniform(-1, 1, (n, 3)) * np.array(h)).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    t, ax = _box_t(lib, o, d, [c] * n, [h] * n)
    od, dd = o.astype(np.float64), d.astype(np.float64)
    lo = np.minimum((np.array(c) - h - od) / dd, (np.array(c) + h - od) / dd)
    assert (t > 0).all()
    np.testing.assert_allclose(t, lo.max(1), rtol=2e-6, atol=1e-7)
    clear = np.sort(lo, 1)[:, 2] - np.sort(lo, 1)[:, 1] > 1e-5          # the entry face is unambiguous
    assert (ax[clear] == lo.argmax(1)[clear]).all()


def test_wins_tie_rule(lib):
    t = np.array([1.0, 1.0, 1.0, 1.0, 0.999, 1.001, 1.0, np.nextafter(np.float32(1), np.float32(2))], np.float32)
    cid = np.array([3, 3, 2, 4, 9, 0, 7, 0], np.int32)
    bt = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    bid = np.array([-1, -2, 3, 3, 0, 9, 7, -1], np.int32)
    out = np.zeros(8, np.int32)
    lib.hs_viewer_wins(8, _ptr(t), _ptr(cid), _ptr(bt), _ptr(bid), _ptr(out))
    # car = ground: car; car = sky at far: car; lower id beats higher at equal t, not the reverse; nearer always; farther never;
    # the same id again does not win; one float step behind the ground does not
    assert out.tolist() == [1, 1, 1, 0, 1, 0, 0, 0]


def test_traversable_matches_the_map_rule(lib):
    rng = np.random.RandomState(3)
    m = (rng.rand(500, 500) < 0.5).astype(np.uint8)
    mp = A.WlTravMap(m.ctypes.data, None, 500, 500, 0, 0.5, 0.5, None)
    # cell boundaries of the 0.5 m grid (x = k / 2 - 0.25 +- one float step), outside the map, far outside
    k = np.arange(-510, 511)
    edge = (k * 0.5 - 0.25).astype(np.float32)
    xs = np.concatenate([edge, np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf)),
                         np.float32([-1e6, 1e6, -125.25, 125.25, 124.75])])
    X, Y = np.meshgrid(xs, xs[::37])
    X, Y = np.ascontiguousarray(X.ravel(), np.float32), np.ascontiguousarray(Y.ravel(), np.float32)
    got = np.zeros(X.size, np.int32)
    lib.hs_viewer_traversable(C.byref(mp), X.size, _ptr(X), _ptr(Y), _ptr(got))
    want = OVM.get_traversability(m, np.stack([X, Y], 1)).astype(np.int32)
    np.testing.assert_array_equal(got, want)
    # NaN clamps to cell 0 of that axis
    nan = np.float32([np.nan, np.nan, 3.0])
    ys = np.float32([2.0, np.nan, np.nan])
    got = np.zeros(3, np.int32)
    lib.hs_viewer_traversable(C.byref(mp), 3, _ptr(nan), _ptr(ys), _ptr(got))
    xi, yi = OVM.get_map_id(np.float32([0.0, 0.0, 3.0]), np.float32([2.0, 0.0, 0.0]))
    xi[:2], yi[1:] = 0, 0
    assert got.tolist() == m[yi, xi].tolist()


def test_checker_cutoff(lib):
    p = _params(8, 8, (4.0, -4.0, 4.0), (0.0, 0.0, 0.0), checker=1.0)
    # k = floor(x) + floor(y): parity below |k| = 1.6e7, the light tone at and beyond it (fp32 integers lose their parity there)
    xs = np.float32([0.5, 1.5, -0.5, -1.5, 15999999.0, 16000001.0, -16000001.0, 8e6, np.nan])
    ys = np.float32([0.5, 0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 8e6, 0.0])
    got = np.zeros(len(xs), np.int32)
    lib.hs_viewer_checker(C.byref(p), len(xs), _ptr(xs), _ptr(ys), _ptr(got))
    assert got.tolist() == [0, 1, 1, 0, 1, 0, 0, 0, 0]
    _, bit = VR.checker_albedo(1.0, xs.astype(np.float64), ys.astype(np.float64), with_bit=True)
    assert bit.tolist() == got.tolist()


def test_q8_rounding_boundaries(lib):
    k = np.arange(256, dtype=np.float64)
    mid = ((k + 0.5) / 255).astype(np.float32)                 # the rounding boundary between k and k + 1
    c = np.concatenate([mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf)),
                        np.float32([-1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf])])
    c = np.ascontiguousarray(c, np.float32)
    got = np.zeros(c.size, np.uint8)
    lib.hs_viewer_q8(c.size, _ptr(c), _ptr(got))
    # fmaf(c, 255, 0.5) rounded once, then truncated and clamped: the double statement of the same
    want = np.clip(np.floor(np.float32(np.clip(c.astype(np.float64) * 255 + 0.5, -1e30, 1e30))), 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(got, want)
    assert got[-7:].tolist() == [0, 0, 0, 255, 255, 255, 0]

"""GPU: the viewer camera's binning paths and geometric edge cases, every frame held to the float64 reference with zero unexplained
pixels (tests/viewer_reference.py::acceptable / check_explained): the scan's carry across 1024-tile chunks, partial tiles in both
directions down to one pixel and up to the 8192-pixel side, a car's silhouette and its bin rectangle's first pixel swept across tile
seams in 1/8-pixel steps, the entry budget's overflow into the big list (shown by the scratch header), shard ids (palette and highlight
by global id), near and far edges, cars placed from their silhouettes 0.1 .. 0.9 px outside each frustum side, and cars on the
heightfield at 1280 x 720."""
import numpy as np
import pytest
import torch

import depth_cases as DC
import viewer_reference as VR
from oracle.mathlib import matrix_from_quat, quat_from_euler_xyz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16


def _camera(p):
    """(origin, body -> world rotation) of the viewer params, float64"""
    R = matrix_from_quat(np.array([list(p.cam_quat)], np.float32)).astype(np.float64)[0]
    return np.array(list(p.cam_pos), np.float64), R


def unproject(p, col, row, dist, lift=0.0):
    """world points at distance `dist` along the optical axis on the rays of (fractional) pixel (col, row), lowered by `lift` (a car
    root lowered by its box centre's height puts the chassis on the ray)"""
    o, R = _camera(p)
    col, row, dist = (np.asarray(a, np.float64) for a in (col, row, dist))
    body = np.stack([np.ones_like(col), -((col + 0.5 - p.cx) / p.fx), -((row + 0.5 - p.cy) / p.fy)], -1)
    return (o + dist[..., None] * (body @ R.T) - np.array([0.0, 0.0, lift])).astype(np.float32)


def yaw_quat(yaw):
    yaw = np.asarray(yaw, np.float32)
    z = np.zeros_like(yaw)
    return np.ascontiguousarray(quat_from_euler_xyz(z, z, yaw).astype(np.float32))


def cam_yaw(p):
    _, R = _camera(p)
    return float(np.arctan2(R[1, 0], R[0, 0]))


def _drift(pos, quat, env_offset=0):
    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.core import DriftBatch
    n = pos.shape[0]
    b = DriftBatch(n, device=DEV, seed=2, env_offset=env_offset)
    b.state[A.S_PX:A.S_PZ + 1, :n] = torch.as_tensor(np.ascontiguousarray(pos.T), device=DEV)
    b.state[A.S_QW:A.S_QZ + 1, :n] = torch.as_tensor(np.ascontiguousarray(quat.T), device=DEV)
    return b


def _render(v, b, eye, lookat, env_index=0):
    H, W = v.height, v.width
    depth = torch.empty(H, W, dtype=torch.float32, device=DEV)
    ids = torch.empty(H, W, dtype=torch.int32, device=DEV)
    rgb = v.render(b, eye, lookat, env_index=env_index, depth=depth, ids=ids)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()


def _frame(v, b, eye, lookat, pos, quat, what, env_index=0, hf=None):
    """render on the device; every pixel explained by the reference over (pos, quat) (default: the batch's own poses)"""
    got = _render(v, b, eye, lookat, env_index)
    p = v.params(b, eye, lookat, env_index)
    acc = VR.acceptable(p, pos, quat, hf)
    print("compare", what, VR.compare(got, acc["nominal"]))        # what the count-based bounds of test_gpu_viewer.py::_check see
    counts = VR.check_explained(got, acc, what)
    return got, counts


def _viewer(w, h, far_clip=None):
    from wheeledlab_amd.viewer import Viewer
    return Viewer(DEV, (w, h)) if far_clip is None else Viewer(DEV, (w, h), far_clip=far_clip)


def _params(w, h, eye, lookat, far_clip=500.0):
    from wheeledlab_amd.viewer import viewer_params
    return viewer_params(w, h, eye, lookat, far_clip=far_clip)


# a camera 30 m up looking level: the ground only below the horizon at ~90 m and more, cars in front of it everywhere in the frame
LEVEL_EYE, LEVEL_AT = (0.0, 0.0, 30.0), (100.0, 0.0, 30.0)


def spread_cars(p, n, seed, dist=(10.0, 25.0), corners=True):
    """n cars on the rays of random pixels (and of the four corner pixels) at random distances, random yaw"""
    rng = np.random.RandomState(seed)
    col = rng.uniform(0, p.width, n) - 0.5
    row = rng.uniform(0, p.height, n) - 0.5
    if corners:
        col[:4], row[:4] = [0, p.width - 1, 0, p.width - 1], [0, 0, p.height - 1, p.height - 1]
    pos = unproject(p, col, row, rng.uniform(*dist, n), lift=0.09)
    return pos, yaw_quat(rng.uniform(-np.pi, np.pi, n))


def _tiles_hit(ids, W):
    r, c = np.nonzero(ids >= 0)
    return np.unique((r // TILE) * ((W + TILE - 1) // TILE) + c // TILE)


@pytest.mark.parametrize("size", [(1280, 720), (1920, 1080)])
def test_scan_carries_across_1024_tile_chunks(size):
    """3600 and 8160 tiles: the scan's carry from chunk to chunk; cars in every chunk and in the last tile (bottom right)"""
    W, H = size
    v = _viewer(W, H)
    p = _params(W, H, LEVEL_EYE, LEVEL_AT)
    pos, quat = spread_cars(p, 300, 1, dist=(15.0, 40.0))
    b = _drift(pos, quat)
    got, _ = _frame(v, b, LEVEL_EYE, LEVEL_AT, pos, quat, f"scan {W}x{H}")
    T = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    hit = _tiles_hit(got[2], W)
    assert set(range((T + 1023) // 1024)) <= set((hit // 1024).tolist())
    assert T - 1 in hit


@pytest.mark.parametrize("size", [(1, 1), (15, 9), (17, 33), (1279, 719), (8192, 16)])
def test_partial_tiles_in_both_directions(size):
    """frame sides that are not multiples of 16 (and a single pixel, and the 8192-pixel side limit): cars on the partial right column
    and the partial bottom row of tiles"""
    W, H = size
    v = _viewer(W, H)
    p = _params(W, H, LEVEL_EYE, LEVEL_AT)
    rng = np.random.RandomState(W + H)
    n = 40
    col = np.concatenate([np.full(n // 4, W - 1.0), rng.uniform(0, W, n // 4) - 0.5, np.full(n // 4, W - 1.0), rng.uniform(0, W, n // 4) - 0.5])
    row = np.concatenate([rng.uniform(0, H, n // 4) - 0.5, np.full(n // 4, H - 1.0), np.full(n // 4, H - 1.0), rng.uniform(0, H, n // 4) - 0.5])
    # distances: cars a few pixels across or more in every frame (fx is 0.87 px at one pixel wide, 13 px at 15), some of them small
    dist = np.full(n, 6.0) if W == 1 else rng.uniform(0.5, 3.0, n) if W < 64 else rng.uniform(3.0, 40.0, n)
    jit = 0.5 if W > 1 else 0.0
    pos = unproject(p, col + rng.uniform(-jit, jit, n), row + rng.uniform(-jit, jit, n), dist, lift=0.09)
    quat = yaw_quat(rng.uniform(-np.pi, np.pi, n))
    b = _drift(pos, quat)
    got, _ = _frame(v, b, LEVEL_EYE, LEVEL_AT, pos, quat, f"partial {W}x{H}")
    ids = got[2]
    assert (ids[:, -1] >= 0).any() and (ids[-1, :] >= 0).any()          # cars drawn in the last column and the last row


def test_tile_seam_sweep():
    """one car stepped in 1/8-pixel increments so that its silhouette's left edge crosses the tile seam at column 160, then its top edge
    the seam at row 96: silhouette pixels on either side of a seam are binned, every frame exact.  (The bin rectangle starts ~16 px
    before the silhouette here: test_bin_rectangle_start_sweep moves the rectangle's own first pixel across a seam.)"""
    W, H = 320, 180
    v = _viewer(W, H)
    eye, at = (0.0, 0.0, 1.0), (10.0, 0.0, 1.0)
    p = _params(W, H, eye, at)
    dist = 4.0
    px_m = dist / p.fx                                   # metres per pixel at that distance
    yaw = yaw_quat([cam_yaw(p)])
    frames = 0
    for axis in (0, 1):
        for k in range(-16, 17):
            # the car's left edge (the wheels and box reach half_track + wheel radius ~ 0.15 m to the side, the box 0.22 m ahead) or
            # its top (0.135 m above the root) near the seam, moved by k / 8 pixel
            if axis == 0:
                c0 = 160.0 + 0.15 / px_m + k / 8.0
                pos = unproject(p, [c0 - 0.5], [60.0], [dist])
            else:
                r0 = 96.0 + 0.135 / px_m + k / 8.0
                pos = unproject(p, [100.0], [r0 - 0.5], [dist])
            b = _drift(pos, yaw)
            got, _ = _frame(v, b, eye, at, pos, yaw, f"seam axis {axis} step {k}")
            frames += 1
            ids = got[2]
            cols = np.nonzero((ids == 0).any(0))[0]
            rows = np.nonzero((ids == 0).any(1))[0]
            assert len(cols) and len(rows)
    assert frames == 66


def test_bin_rectangle_start_sweep():
    """a car far enough away (12 m) that its silhouette lies within a few pixels of its bin rectangle's first column / row, stepped in
    1/8-pixel increments so that the rectangle's first pixel crosses the seam at column 160, then at row 96: in some frames the car's
    pixels fall in the rectangle's first tile, so a rectangle one tile short there drops them; every frame exact"""
    W, H = 320, 180
    v = _viewer(W, H)
    eye, at = (0.0, 0.0, 1.0), (10.0, 0.0, 1.0)
    p = _params(W, H, eye, at)
    dist = 12.0
    yaw = yaw_quat([cam_yaw(p) + 0.4])
    first_tile_frames = 0
    for axis in (0, 1):
        def pos_at(s):
            return unproject(p, [s], [100.0], [dist], lift=0.09) if axis == 0 else unproject(p, [200.0], [s], [dist], lift=0.09)

        def start(s):                                   # the rectangle's first column (axis 0) or row (axis 1), unrounded
            return _bin_rect(p, pos_at(s))[0, 2 * axis]
        seam = 160.0 if axis == 0 else 96.0
        lo, hi = seam - 40.0, seam + 40.0               # the car centre sits ~10 px after its rectangle's start: bisect to the seam
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if start(mid) < seam else (lo, mid)
        for k in range(-12, 13):
            pos = pos_at(hi + k / 8.0)
            b = _drift(pos, yaw)
            got, _ = _frame(v, b, eye, at, pos, yaw, f"rectangle start axis {axis} step {k}")
            rect = _bin_rect(p, pos)[0]
            cover = (got[2] == 0).any(0) if axis == 0 else (got[2] == 0).any(1)       # columns / rows holding car pixels
            lines = np.nonzero(cover)[0]
            assert len(lines)
            first = int(max(rect[2 * axis], 0)) // TILE
            first_tile_frames += int(lines[0] // TILE == first)
    print("frames with car pixels in the rectangle's first tile:", first_tile_frames, "of 50")
    assert first_tile_frames >= 4, first_tile_frames


def test_entry_budget_overflow_goes_to_the_big_list():
    """65536 cars as 36 distinct poses repeated with bit-identical float32 poses, each covering 40 .. 64 tiles: the entries reserved
    exceed max(8 N, 2^21), so late cars go to the big list.  By the tie rule the lowest env id of each group wins every pixel, so the
    frame is the reference over the 36 distinct poses"""
    W, H = 320, 180
    eye, at = (0.0, 0.0, 3.0), (10.0, 0.0, 3.0)
    p = _params(W, H, eye, at)
    G, N = 36, 65536
    gc, gr = np.meshgrid(np.linspace(60, 260, 6), np.linspace(40, 140, 6))
    rng = np.random.RandomState(7)
    dist = rng.uniform(2.3, 2.4, G)
    gpos = unproject(p, gc.ravel(), gr.ravel(), dist)
    gquat = yaw_quat(rng.uniform(-np.pi, np.pi, G))
    nt = _tile_counts(p, gpos)
    assert (nt >= 40).all() and (nt <= 64).all(), nt
    grp = np.arange(N) % G
    pos, quat = gpos[grp], gquat[grp]
    b = _drift(pos, quat)
    v = _viewer(W, H)
    got, _ = _frame(v, b, eye, at, gpos, gquat, "entry budget overflow")
    hdr = v._scratch[:12].view(torch.int32).cpu().numpy()      # wl_viewer.hip kHdrInts: visible cars, big-list cars, entries reserved
    budget = max(8 * N, 1 << 21)
    print("viewer scratch header", hdr.tolist(), "budget", budget)
    assert hdr[0] == N and hdr[1] > 0 and hdr[2] > budget
    assert set(np.unique(got[2][got[2] >= 0]).tolist()) <= set(range(G))


def _bin_rect(p, pos):
    """each car's pixel rectangle as the bin pass computes it, in float64 and before clamping to the frame: [n, 4] first / last column,
    first / last row (the bounding sphere's corner rectangle, one pixel of margin)"""
    from wheeledlab_amd.viewer import CHASSIS_CENTER, CHASSIS_HALF
    wheel = np.array([p.half_wheelbase_f, p.half_track, p.wheel_z])
    r = max(np.linalg.norm(CHASSIS_CENTER) + np.linalg.norm(CHASSIS_HALF), np.linalg.norm(wheel) + p.wheel_radius) * 1.001 + 1e-4
    o, R = _camera(p)
    rel = pos.astype(np.float64) - o
    z, xr, yd = rel @ R[:, 0], -(rel @ R[:, 1]), -(rel @ R[:, 2])
    out = []
    for zi, xi, yi in zip(z, xr, yd):
        us = [(xi + s * r) / (zi + q * r) for s in (-1, 1) for q in (-1, 1)]
        vs = [(yi + s * r) / (zi + q * r) for s in (-1, 1) for q in (-1, 1)]
        out.append([np.floor(p.fx * min(us) + p.cx - 0.5) - 1, np.ceil(p.fx * max(us) + p.cx - 0.5) + 1,
                    np.floor(p.fy * min(vs) + p.cy - 0.5) - 1, np.ceil(p.fy * max(vs) + p.cy - 0.5) + 1])
    return np.array(out)


def _tile_counts(p, pos):
    """tiles of each car's rectangle (the chosen poses keep away from the limits where float64 and the bin pass's fp32 could differ)"""
    rect = _bin_rect(p, pos)
    tx = np.minimum(rect[:, 1], p.width - 1).astype(int) // TILE - np.maximum(rect[:, 0], 0).astype(int) // TILE + 1
    ty = np.minimum(rect[:, 3], p.height - 1).astype(int) // TILE - np.maximum(rect[:, 2], 0).astype(int) // TILE + 1
    return tx * ty


def test_shard_ids_palette_and_highlight_follow_the_global_id():
    """a shard (env_offset 1003): palette and highlight keyed by the global id, the id output local"""
    W, H = 320, 180
    eye, at = (0.0, 0.0, 3.0), (10.0, 0.0, 1.0)
    p = _params(W, H, eye, at)
    pos, quat = spread_cars(p, 64, 5, dist=(3.0, 9.0), corners=False)
    v = _viewer(W, H)
    b = _drift(pos, quat, env_offset=1003)
    hi, _ = _frame(v, b, eye, at, pos, quat, "shard highlight 1008", env_index=1008)
    none, _ = _frame(v, b, eye, at, pos, quat, "shard no highlight", env_index=-1)
    local, _ = _frame(v, b, eye, at, pos, quat, "shard local index", env_index=5)
    ids = hi[2]
    assert ids.max() < 64 and (ids == 5).sum() > 20
    assert np.array_equal(hi[2], none[2]) and np.array_equal(hi[1], none[1])
    diff = (hi[0] != none[0]).any(-1)
    assert diff.any() and (ids[diff] == 5).all()              # the highlight falls on global id 1008 = local 5, nowhere else
    assert np.array_equal(local[0], none[0])                   # env_index is global: local 5 of this shard is not 5
    b0 = _drift(pos, quat, env_offset=0)
    zero, _ = _frame(v, b0, eye, at, pos, quat, "shard offset 0", env_index=-1)
    assert np.array_equal(zero[2], ids) and (zero[0] != none[0]).any()     # same ids, other palette entries


def _near_far_scenes():
    """(name, eye, lookat, far_clip, pos, quat): the camera inside a chassis box and inside a wheel sphere; a car whose bounding
    sphere straddles the image plane; the far clip through a car; cars behind the camera"""
    from wheeledlab_amd.params import mushr_vehicle
    vh = mushr_vehicle()
    W, H = 320, 180
    rng = np.random.RandomState(9)
    base = np.zeros((24, 3), np.float32)
    base[:, :2] = rng.uniform(-3, 3, (24, 2))
    bq = yaw_quat(rng.uniform(-np.pi, np.pi, 24))
    out = []
    root = np.array([[1.0, 0.5, 0.0]], np.float32)
    q0 = yaw_quat([0.3])
    R0 = matrix_from_quat(q0).astype(np.float64)[0]
    inbox = root[0] + R0 @ np.array([0.05, 0.02, 0.1])
    out.append(("eye inside a chassis", tuple(inbox), tuple(inbox + [1.0, 0.3, -0.2]), 500.0, np.concatenate([root, base]),
                np.concatenate([q0, bq])))
    inwheel = root[0] + R0 @ np.array([vh.half_wheelbase_f, vh.half_track + 0.03, vh.wheel_z + 0.01])     # outside the box
    out.append(("eye inside a wheel", tuple(inwheel), tuple(inwheel + [-1.0, -0.4, -0.3]), 500.0, np.concatenate([root, base]),
                np.concatenate([q0, bq])))
    # the bounding sphere (r ~ 0.34 m) straddles the image plane: the root 0.2 m ahead of the eye, 0.25 m below and to the side
    eye, at = (0.0, 0.0, 0.45), (5.0, 0.0, 0.2)
    p = _params(W, H, eye, at)
    strad = unproject(p, [230.0], [170.0], [0.2])
    out.append(("sphere straddles the image plane", eye, at, 500.0, np.concatenate([strad, base]), np.concatenate([q0, bq])))
    # far clip at 12 m through cars standing 11.8 .. 12.2 m ahead
    eye, at = (0.0, 0.0, 1.5), (10.0, 0.0, 1.0)
    p = _params(W, H, eye, at, far_clip=12.0)
    cut = unproject(p, np.linspace(40, 280, 9), np.full(9, 60.0), np.linspace(11.8, 12.2, 9))
    out.append(("far clip through cars", eye, at, 12.0, cut, yaw_quat(rng.uniform(-np.pi, np.pi, 9))))
    eye, at = (0.0, 0.0, 3.0), (10.0, 0.0, 3.0)
    p = _params(W, H, eye, at)
    # behind the camera (and one straddling the eye's plane from behind)
    behind = unproject(p, rng.uniform(0, W, 12), rng.uniform(0, H, 12), -rng.uniform(0.3, 20.0, 12))
    out.append(("cars behind the camera", eye, at, 500.0, np.concatenate([behind, base]), np.concatenate([yaw_quat(np.zeros(12)), bq])))
    return out


NEAR_FAR = _near_far_scenes()


@pytest.mark.parametrize("k", range(len(NEAR_FAR)), ids=[s[0] for s in NEAR_FAR])
def test_near_far_and_frustum_edges(k):
    name, eye, at, far, pos, quat = NEAR_FAR[k]
    v = _viewer(320, 180, far_clip=far)
    b = _drift(pos, quat)
    got, _ = _frame(v, b, eye, at, pos, quat, name)
    ids = got[2]
    if name == "cars behind the camera":
        assert not (ids[ids >= 0] < 12).any()
    if name == "sphere straddles the image plane":
        assert (ids == 0).any()
    if name == "far clip through cars":
        assert (ids >= 0).any() and (got[1][ids >= 0] < 12.0).all()


def _grown(p, side, extra):
    """p's frame with `extra` pixels added beyond one side (0 left, 1 right, 2 top, 3 bottom); every other pixel keeps its ray"""
    q = type(p).from_buffer_copy(p)
    if side == 0:
        q.width, q.cx = q.width + extra, q.cx + extra
    elif side == 1:
        q.width += extra
    elif side == 2:
        q.height, q.cy = q.height + extra, q.cy + extra
    else:
        q.height += extra
    return q


def _edge_line(p, side):
    """the frame's last column or row on one side as a frame of its own (same rays)"""
    q = type(p).from_buffer_copy(p)
    if side == 0:
        q.width = 1
    elif side == 1:
        q.width, q.cx = 1, q.cx - (p.width - 1)
    elif side == 2:
        q.height = 1
    else:
        q.height, q.cy = 1, q.cy - (p.height - 1)
    return q


def place_outside(p, side, across, dist, quat, off):
    """a car at `dist`, centred on row (left / right) or column (top / bottom) `across`, placed from its silhouette in the float64
    reference: bisect its centre's pixel coordinate until its last pixel in the frame leaves the frame's edge line, then move it `off`
    pixels further out"""
    out = -1.0 if side in (0, 2) else 1.0
    edge = 0.0 if side in (0, 2) else (p.width - 1.0 if side == 1 else p.height - 1.0)
    line = _edge_line(p, side)

    def pos_at(s):
        col, row = (s, across) if side < 2 else (across, s)
        return unproject(p, [col], [row], [dist], lift=0.09)

    def covers(s):
        return (VR.render(line, pos_at(s), quat)[2] == 0).any()

    lo, hi = edge, edge + out * 200.0            # covers the edge line at lo, not at hi
    assert covers(lo) and not covers(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if covers(mid) else (lo, mid)
    return pos_at(hi + out * off)[0]


def test_cars_within_a_pixel_outside_each_frustum_side():
    """cars whose silhouettes end 0.1 .. 0.9 px beyond each side of the frame (placed from the reference's own silhouette): absent from
    the frame, present in the frame one pixel larger on that side, and absent from the kernel's frame"""
    W, H = 320, 180
    eye, at = LEVEL_EYE, LEVEL_AT
    p = _params(W, H, eye, at)
    rng = np.random.RandomState(12)
    offs = np.linspace(0.1, 0.9, 5)
    pos, quat, side_of = [], [], []
    for side in range(4):
        across = np.linspace(25, 155, 5) if side < 2 else np.linspace(40, 280, 5)
        for k in range(5):
            q = yaw_quat([rng.uniform(-np.pi, np.pi)])
            pos.append(place_outside(p, side, across[k], rng.uniform(4.0, 10.0), q, offs[k]))
            quat.append(q[0])
            side_of.append(side)
    pos, quat, side_of = np.array(pos, np.float32), np.ascontiguousarray(quat, np.float32), np.array(side_of)
    assert not (VR.render(p, pos, quat)[2] >= 0).any()
    for side in range(4):
        seen = set(np.unique(VR.render(_grown(p, side, 1), pos, quat)[2]).tolist())
        assert set(np.nonzero(side_of == side)[0].tolist()) <= seen, (side, seen)
    v = _viewer(W, H)
    b = _drift(pos, quat)
    got, _ = _frame(v, b, eye, at, pos, quat, "cars within a pixel outside the frustum")
    assert not (got[2] >= 0).any()


def test_cars_on_heightfield_at_full_resolution():
    """the elevation task's viewer pose over the depth-case terrain with cars from DC.poses at 1280 x 720: the multi-chunk scan with
    the field walk"""
    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.core import ElevBatch
    field = DC.on_lattice(DC.terrain())
    n = 1024
    b = ElevBatch(n, device=DEV, seed=3, heightfield=field)
    pos, quat = DC.poses(n, 11, field, span=12.0)
    b.state[A.S_PX:A.S_PZ + 1, :n] = torch.as_tensor(np.ascontiguousarray(pos.T), device=DEV)
    b.state[A.S_QW:A.S_QZ + 1, :n] = torch.as_tensor(np.ascontiguousarray(quat.T), device=DEV)
    v = _viewer(1280, 720)
    hf = (b.hf.heights.cpu().numpy(), b.hf.x0, b.hf.y0, b.hf.cell, b.hf.outside_z)
    eye, at = (20.0, -20.0, 20.0), (0.0, 0.0, 0.0)
    got, _ = _frame(v, b, eye, at, pos, quat, "heightfield 1280x720", hf=hf)
    assert (got[2] >= 0).sum() > 5000 and len(_tiles_hit(got[2], 1280)) > 300

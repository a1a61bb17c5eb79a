"""Which envs MAY miss the tight HIP-vs-oracle bound of a heightfield step, decided from the ORACLE's own state (verdict of round 5:
an excuse must be a predicate, not a count).  The model has two discontinuities a last-bit difference between the two arithmetics can
land on different sides of:
  * a wheel making or breaking contact: the normal force max(k pen - c v_n, 0) has a kink at 0 and the implicit integrator's contact
    count jumps there -- the env is excusable if some wheel comes within FZ_EPS newtons of the switch at some sub-step;
  * a wheel's sample point crossing a cell line of the grid: the bilinear surface's normal jumps there -- excusable if some wheel comes
    within CELL_EPS cells of a line at some sub-step.
Both margins are recorded by the oracle (oracle/vehicle.py::substep `probe`, oracle/elev_step.py::ground_fn `probe`).  The thresholds are
~100 x what rounding can move a wheel (1e-6 m, 1e-4 N) and far below what the dynamics do in a sub-step."""
import os

import numpy as np
import pytest

FZ_EPS = 0.02        # N     (static load per wheel: 8.3 N)
CELL_EPS = 2e-3      # cells (0.1 mm at the 5 cm grid)


def contact_changed(probe, n):
    """bool [n]: the in-contact pattern of the four wheels changed between sub-steps of the step (a touch-down or a lift-off)"""
    masks = np.stack(probe["contact"])[:, :n]
    return (masks != masks[0]).any(0)


def explainable(probe, n):
    """bool [n]: the oracle's step of the env passed within the thresholds of one of the two discontinuities (a wheel that did make or
    break contact inside the step passed through the first)"""
    fz = np.asarray(probe.get("fz_margin", np.full(n, np.inf)))[:n]
    cell = np.asarray(probe.get("cell_margin", np.full(n, np.inf)))[:n]
    return (fz < FZ_EPS) | (cell < CELL_EPS) | contact_changed(probe, n)


WHEEL_ROWS, WHEEL_RADIUS = slice(13, 17), 0.05


def state_error(got, want, n, rows=21, tight=5e-4):
    """|got - want| in units of the bound: `tight` absolute + relative on every row of the state.  The four wheel-spin rows are held to
    2 x tight of CONTACT SPEED instead: a spin is a contact speed over r = 0.05 m (1e-3 m/s is 2e-2 rad/s), and the spin solve divides by
    A0 + K r^2 with K the tyre's secant stiffness -- the one place where the step's rounding is amplified (measured, device physics
    compiled for the host vs this oracle, 4096 random states, 10 x 20 ms: spins to 1.8e-2 rad/s where every body row holds 1e-4)"""
    atol = np.full((rows, 1), tight)
    rtol = np.full((rows, 1), tight)
    atol[WHEEL_ROWS], rtol[WHEEL_ROWS] = 2 * tight / WHEEL_RADIUS, 2 * tight
    return np.abs(got[:rows, :n] - want[:rows, :n]) / (atol + rtol * np.abs(want[:rows, :n]))


def check_state(got, want, probe, n, ok, rows=21, tight=5e-4, loose=400.0, where=""):
    """every env in `ok` holds rows [0, rows) of the state to `tight` (state_error) -- except envs the predicate explains, which are held
    to `loose` x that bound and must be few.  -> (mask of the envs that met the tight bound, number excused)"""
    err = state_error(got, want, n, rows, tight)
    touchy = (err.max(0) > 1.0) & ok
    ex = explainable(probe, n)
    unexplained = touchy & ~ex
    if unexplained.any():
        e = int(np.argmax(np.where(unexplained, err.max(0), 0)))
        raise AssertionError(f"{where}: {int(unexplained.sum())} env(s) miss the bound with no discontinuity in reach; worst env {e}: "
                             f"{float(err[:, e].max()):.2f} x the bound in row {int(err[:, e].argmax())}, fz_margin "
                             f"{float(np.asarray(probe['fz_margin'])[e]):.4f} N, cell_margin {float(np.asarray(probe.get('cell_margin', [np.inf] * n))[e]):.5f}")
    assert err[:, touchy].max(initial=0) < loose, (where, float(err[:, touchy].max()))
    return ok & ~touchy, int(touchy.sum())


# ---- edge goldens (tests/golden/{,seed1000/,seed2024/}elevation_mdp_edges.npz, visual_*_edges.npz): the inputs a kernel may answer otherwise, each
# decided from the inputs and the reference's own values ------------------------------------------------------------------------

def rollover_norm_excused(quat, ref_r33, tie=0.5):
    """rows where the quaternion's norm error alone moves R33 across cos 60 deg: the reference divides by |q|^2
    (matrix_from_quat), the kernels and the oracle use the unit-quaternion form 1 - 2 (x^2 + y^2)"""
    q = np.asarray(quat, np.float64)
    unnorm = 1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2)
    return (np.asarray(ref_r33) <= tie) != (unnorm <= tie)


def map_index_excused(coord, cells, spacing):
    """one axis of get_map_id: (coord + cells * spacing / 2 + spacing / 2) / spacing, judged in float64 from the fp32 input.
    Excused: a quotient that is not finite or beyond 2^63, where torch's float -> int64 `.long()` has no defined value (x86 gives
    INT64_MIN, which clamps to cell 0); and, on geometries whose half extent cells * spacing / 2 is not the same fp32 number when
    formed from the fp32 spacing (the kernels) as from the float64 one (the reference), a quotient within (cells + |q|) 2^-21 of an
    integer (a cell line)"""
    c = np.asarray(coord, np.float64)
    half64 = np.float32(cells * spacing / 2.0)
    half32 = np.float32(0.5) * np.float32(np.float32(cells) * np.float32(spacing))
    with np.errstate(all="ignore"):
        q = (c + cells * spacing / 2.0 + spacing / 2.0) / spacing
        wild = ~np.isfinite(q) | (np.abs(q) >= 2.0 ** 63)
        near = np.abs(q - np.round(q)) <= (cells + np.abs(q)) * 2.0 ** -21
    return wild | (near & (half64 != half32))


def out_of_map_excused(coord, cells, spacing):
    """one axis of out_of_map: |coord| between the fp32 half extent formed from the float64 spacing (the reference) and the one
    formed from the fp32 spacing (the kernels), both included"""
    a = np.abs(np.asarray(coord, np.float32))
    h64 = np.float32(cells * spacing / 2.0)
    h32 = np.float32(0.5) * np.float32(np.float32(cells) * np.float32(spacing))
    return (h64 != h32) & (a >= min(h64, h32)) & (a <= max(h64, h32))


# rows every task's reset writes (csrc/wl_kernel_common.h::store_reset_rows): pose, linear and angular velocity, last action,
# the WL_MAX_REW_TERMS episode sums
RESET_SHARED_ROWS = tuple(range(0, 13)) + (19, 20) + tuple(range(27, 35))


def check_masked_reset(env, full_state, own_rows=()):
    """A masked reset of `env` -- 70 envs (the last wavefront is partial), fresh (step 0), every row and the episode lengths
    preloaded with non-zero values, every third env masked in -- against `full_state`: the state [rows, >= 70] an unmasked reset
    of a batch with the same seed left at step 0, which the caller has held to the oracle (a draw depends on the env's global
    index, the seed and the step, not on the batch size).  The drawn rows are thus exact against the kernel's own unmasked output,
    which meets the oracle within the caller's tolerance; the zeroed and the untouched rows are exact in absolute terms.  Exact values:
      masked in:  RESET_SHARED_ROWS and the task's `own_rows` equal full_state (so the velocities / actions / sums a reset zeroes
                  are 0 although they were not before), episode_len 0, every other row as preloaded;
      masked out, and the padding columns up to the stride: everything as preloaded."""
    import torch
    n = env.n
    assert n == 70 and env.step_count == 0
    rows, stride = env.state.shape
    r, e = torch.arange(rows, dtype=torch.float32)[:, None], torch.arange(stride, dtype=torch.float32)[None, :]
    env.state.copy_((1.0 + 0.25 * r + e / 128.0).to(env.state.device))        # > 0 everywhere, distinct per row and env
    env.episode_len.copy_((5 + torch.arange(stride, dtype=torch.int32)).to(env.state.device))
    before, ep_before = env.state.clone(), env.episode_len.clone()
    mask = torch.arange(n, device=env.state.device) % 3 == 0
    env.reset(mask)
    torch.cuda.synchronize()
    got, ep = env.state.cpu(), env.episode_len.cpu()
    before, ep_before = before.cpu(), ep_before.cpu()
    inn = torch.zeros(stride, dtype=torch.bool)
    inn[:n] = mask.cpu()
    assert torch.equal(got[:, ~inn], before[:, ~inn]) and torch.equal(ep[~inn], ep_before[~inn])
    written = sorted(set(RESET_SHARED_ROWS) | set(own_rows))
    kept = [i for i in range(rows) if i not in written]
    want = torch.as_tensor(full_state)[:, :n][:, mask.cpu()]
    assert torch.equal(got[written][:, inn], want[written])
    assert (got[list(range(10, 13)) + [19, 20] + list(range(27, 35))][:, inn] == 0).all() and (ep[inn] == 0).all()
    assert torch.equal(got[kept][:, inn], before[kept][:, inn])
    assert int(inn.sum()) == 24


# The edge sets live under tests/golden/ only: tests/golden/*_edges.npz (input seeds as generated) and tests/golden/seed1000/*_edges.npz
# (WL_GOLDEN_SEED_OFFSET=1000), or WL_GOLDEN_DIR alone when it is set (the fresh-seed rerun of test_oracle_golden_drift.py).  The
# edge values themselves are fixed; only their random filler follows the offset.
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SEED1000 = os.path.join(_GOLDEN, "seed1000")
# WL_GOLDEN_DIR = tests/golden_seed1000 (the conftest's second set): its edge files are the ones under tests/golden/seed1000
_EDGE_DIR_OF = {os.path.realpath(os.path.join(_GOLDEN, os.pardir, "golden_seed1000")): _SEED1000}
EDGE_SETS = ([_EDGE_DIR_OF.get(os.path.realpath(os.environ["WL_GOLDEN_DIR"]), os.environ["WL_GOLDEN_DIR"])] if os.environ.get("WL_GOLDEN_DIR")
             else [_GOLDEN, _SEED1000])


@pytest.fixture(scope="session", params=EDGE_SETS, ids=["edges" if d == _GOLDEN else "edges_" + os.path.basename(d.rstrip("/")) for d in EDGE_SETS])
def edge_golden(request):
    """edge_golden(name) -> the arrays of <set>/<name>.npz; edge_golden.task_map() -> the task's 500 x 500 map (the same in every set)"""
    def load(name):
        return dict(np.load(os.path.join(request.param, name + ".npz")))

    def task_map():
        g = np.load(os.path.join(_GOLDEN, "visual_trav.npz"))
        return np.unpackbits(g["full_map_packed"])[: 500 * 500].reshape(500, 500).astype(bool)
    load.task_map = task_map
    return load

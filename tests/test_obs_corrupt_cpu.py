"""CPU checks of the observation corruption: the reference against itself (tests/obs_corrupt_reference.py: the exact fma against
rational arithmetic, the vectorised bias bookkeeping against the per-env model, the statistics the GPU test asks of the device), the
header and its ctypes mirror, wl_obs_corrupt_width on good and bad tables, every argument refusal of wl_obs_corrupt_apply before any
launch, the config classes and envs/corruption.resolve, and the per-element body compiled for the host as a stand-alone program
(tests/host_sim/obs_corrupt_host.cpp) -- plain and under -fsanitize=address,undefined -- against the reference.

The Gaussian path on the host: the stand-in's log2, sqrt and cos are libm's, so z is within EZ_HOST = R_MAX 2^-22 of the float64
Box-Muller value (derived in the reference's docstring: r within 1.75 ulp, cos within 2^-25, their product 1/2 ulp), a few ulp; the
comparison uses the reference's tolerance formula with that EZ.  Everything else is byte for byte."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from tests import obs_corrupt_reference as R
from tests.obs_history_reference import special_words
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_obsnoise.h")
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(ROOT, "tests", "host_sim", "obs_corrupt_host.cpp")
TABLES = R.tables()


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def _ctable(rows):
    rows = list(rows)
    return (A.WlObsCorruptTerm * max(len(rows), 1))(*[A.WlObsCorruptTerm(*r) for r in rows])


# ---- the reference holds itself ----------------------------------------------------------------------------------------

def test_fma_f32_is_one_rounding_against_rational_arithmetic():
    rng = np.random.default_rng(1)
    u = R.u01(rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32))
    b = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 3, 4000)).astype(np.float32)
    a = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 3, 4000)).astype(np.float32)
    # a float64 sum that lands ON a float32 tie while the exact value does not: u b = 1 - 2^-46, a = 2^24 + 2 -> exactly 2^24 + 3 - 2^-46,
    # just below the midpoint of 2^24 + 2 and 2^24 + 4; float64 rounds the sum to the midpoint and ties-to-even then picks 2^24 + 4
    u[:2] = np.float32(1 + 2.0 ** -23)
    b[:2] = np.float32([1 - 2.0 ** -23, -(1 - 2.0 ** -23)])
    a[:2] = np.float32([2.0 ** 24 + 2, -(2.0 ** 24 + 2)])
    got = R.fma_f32(u, b, a)
    twice = (u.astype(np.float64) * b.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    for i in range(len(u)):
        want = R.round_fraction_f32(Fraction(float(u[i])) * Fraction(float(b[i])) + Fraction(float(a[i])))
        assert float(got[i]) == want, (i, float(u[i]), float(b[i]), float(a[i]))
    assert (twice[:2] != got[:2]).all() and list(got[:2]) == [2.0 ** 24 + 2, -(2.0 ** 24 + 2)]      # rounded twice, both come out wrong


def test_round_fraction_f32_on_known_values():
    assert R.round_fraction_f32(Fraction(1, 3)) == float(np.float32(1.0 / 3.0))
    assert R.round_fraction_f32(Fraction(1) + Fraction(1, 1 << 24)) == 1.0                       # tie to even
    assert R.round_fraction_f32(Fraction(1) + Fraction(3, 1 << 24)) == float(np.float32(1 + 2.0 ** -22))
    assert R.round_fraction_f32(Fraction(-5, 1 << 150)) == -float(np.float32(2.0 ** -148)) and R.round_fraction_f32(Fraction(0)) == 0.0


def _reset_patterns(rng, K, n):
    r = rng.random((K, n)) < 0.2
    r[0, 0] = True                      # a reset on step 0
    r[5:8, 1] = True                    # resets on consecutive steps
    r[:, 2] = False                     # an env that never resets
    r[:, 3] = True                      # and one that always does
    return r


@pytest.mark.parametrize("name", ["drift", "every_uniform", "every_gaussian"])
def test_vectorised_bias_and_per_env_model_agree_over_40_steps(name):
    tab, D, Db = R.table(TABLES[name])
    rng = np.random.default_rng(D)
    K, n, seed, off = 40, 6, 1234567, 3
    resets = _reset_patterns(rng, K, n)
    model, bias = R.BiasModel(tab, n), np.zeros((n, Db), np.float32)
    state = R.state_block(rng, n)
    drawn_at = np.full(n, -1)
    for k in range(K):
        enable = k % 7 != 3                        # a step with corruption off: nothing is drawn, nothing is stored
        x = special_words(rng, (n, D))
        res = R.apply(tab, x, bias, resets[k], seed, 100 + k, off, enable, state=state)
        want = model.step(resets[k], seed, 100 + k, off, enable)
        assert np.array_equal(res.bias.view(np.uint32), want.view(np.uint32)), (name, k)
        changed = (res.bias.view(np.uint32) != bias.view(np.uint32)).any(1)
        assert not changed[~(resets[k] & enable)].any()                 # held for the episode
        drawn_at[resets[k] & enable] = k
        bias = res.bias
    assert drawn_at[2] == -1 and (bias[2] == 0).all() and drawn_at[3] == K - 1
    # per env and term: one value across the columns
    res = R.apply(tab, special_words(rng, (n, D)), bias, np.ones(n, bool), seed, 7, off, True, state=state)
    for t in tab:
        if t["bias_kind"] != R.NONE and not t["bias_per_component"]:
            assert Db > 0 and res.bias[:, t["bias_off"]].shape == (n,)


def _stats(noise, bias, n_env, K, what):
    """the checks of the GPU statistics test on arrays noise [K, n, w], bias [n, w]: moments within 5 standard errors, correlations
    below 5 / sqrt(count)"""
    kind, a, b = what
    flat = noise.reshape(-1).astype(np.float64)
    m = flat.size
    if kind == R.UNIFORM:
        mean, sd, kurt = a + b / 2, b / np.sqrt(12.0), 1.8
        assert (flat >= a).all() and (flat < np.float64(np.float32(a) + np.float32(b))).all()
    else:
        mean, sd, kurt = a, b, 3.0
    assert abs(flat.mean() - mean) <= 5 * sd / np.sqrt(m)
    assert abs(flat.std() - sd) <= 5 * sd * np.sqrt((kurt - 1) / (4 * m))

    def corr(p, q):
        p, q = p.reshape(-1).astype(np.float64), q.reshape(-1).astype(np.float64)
        return abs(np.corrcoef(p, q)[0, 1]), 5 / np.sqrt(p.size)
    pairs = [(noise[:, :, :-1], noise[:, :, 1:]), (noise[:, :-1], noise[:, 1:]), (noise[:-1], noise[1:])]
    if bias is not None:
        pairs.append((noise, np.broadcast_to(bias[None], noise.shape)))
    for p, q in pairs:
        c, bound = corr(p, q)
        assert c < bound, (c, bound)


def stats_table():
    """the drift layout with a noise on every term the statistics can see: Gaussian, Gaussian, uniform, Gaussian + uniform bias, uniform"""
    return R.table([R.term(3, R.gaussian(0.0, 0.1)), R.term(3, R.gaussian(0.0, 0.1)), R.term(3, R.uniform(-0.1, 0.1)),
                    R.term(3, R.gaussian(0.0, 0.4), bias=R.uniform(-0.05, 0.05)), R.term(2, R.uniform(-0.1, 0.1))])


def check_statistics(outs, biases, tab):
    """outs float32 [K, n, D] of zero inputs with every reset flag set (the noise itself; the bias term: noise + bias); biases [K, n, Db]"""
    K, n, _ = outs.shape
    for t in tab:
        cols = slice(t["off"], t["off"] + t["width"])
        x = outs[:, :, cols].astype(np.float64)
        bias = None
        if t["bias_kind"] != R.NONE:
            b = biases[:, :, t["bias_off"]:t["bias_off"] + t["width"]].astype(np.float64)
            x = x - b                                   # exact to an ulp: the noise of the step
            _stats(b, None, n, K, (t["bias_kind"], t["bias_a"], t["bias_b"]))
            c = abs(np.corrcoef(x.reshape(-1), b.reshape(-1))[0, 1])      # a term's per-step noise against its bias
            assert c < 5 / np.sqrt(x.size), c
        _stats(x, bias, n, K, (t["noise_kind"], t["noise_a"], t["noise_b"]))


def test_reference_passes_the_statistics_asked_of_the_device():
    tab, D, Db = stats_table()
    n, K = 4096, 64
    outs, biases = [], []
    x, bias = np.zeros((n, D), np.uint32), np.zeros((n, Db), np.float32)
    for k in range(K):
        res = R.apply(tab, x, bias, np.ones(n, bool), 42, 1000 + k, 0, True)
        outs.append(res.bits.view(np.float32))
        biases.append(res.bias)
    check_statistics(np.stack(outs), np.stack(biases), tab)


# ---- the C boundary --------------------------------------------------------------------------------------------------

def test_obsnoise_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.OBSCORRUPT_SIGNATURES) == {"wl_obs_corrupt_version", "wl_obs_corrupt_width", "wl_obs_corrupt_apply"}
    others = (set(A.SIGNATURES) | set(A.VIEWER_SIGNATURES) | set(A.TERRAIN_SIGNATURES) | set(A.OBSNORM_SIGNATURES) | set(A.RAYCASTER_SIGNATURES)
              | set(A.OBSHIST_SIGNATURES))
    assert not declared & others
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_obs_corrupt_version() == 1 == A.WL_OBSCORRUPT_VERSION


def test_obsnoise_header_matches_the_ctypes_struct_and_the_step_boundary_is_unchanged(tmp_path):
    fields = [f for f, _ in A.WlObsCorruptTerm._fields_]
    assert tuple(fields) == R.FIELDS
    probe = tmp_path / "probe.c"
    offs = ", ".join(f"(int)offsetof(WlObsCorruptTerm, {f})" for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_obsnoise.h"\n'
                     'int main(){int v[] = {(int)WL_OBSCORRUPT_VERSION, (int)WL_OBSCORRUPT_MAX_TERMS, (int)WL_OBSCORRUPT_MAX_DIM, '
                     '(int)WL_OC_STREAM_NOISE, (int)WL_OC_STREAM_BIAS, (int)WL_OC_NONE, (int)WL_OC_CONSTANT, (int)WL_OC_UNIFORM, (int)WL_OC_GAUSSIAN, '
                     '(int)WL_OC_ADD, (int)WL_OC_SCALE, (int)WL_OC_ABS, (int)WL_S_ACT0, (int)WL_ABI_VERSION, (int)WL_ABI_REVISION, '
                     f'(int)sizeof(WlObsCorruptTerm), {offs}}};\n'
                     'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%d ", v[i]); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = A.WlObsCorruptTerm
    assert got == [A.WL_OBSCORRUPT_VERSION, A.OBSCORRUPT_MAX_TERMS, A.OBSCORRUPT_MAX_DIM, A.OC_STREAM_NOISE, A.OC_STREAM_BIAS, A.OC_NONE, A.OC_CONSTANT,
                   A.OC_UNIFORM, A.OC_GAUSSIAN, A.OC_ADD, A.OC_SCALE, A.OC_ABS, A.S_ACT0, A.WL_ABI_VERSION, A.WL_ABI_REVISION, C.sizeof(T)] + \
        [getattr(T, f).offset for f in fields]
    assert got[:5] == [1, 64, 1 << 20, R.S_NOISE, R.S_BIAS] and got[13:16] == [24, 1, 64]
    assert (R.NONE, R.CONSTANT, R.UNIFORM, R.GAUSSIAN, R.ADD, R.SCALE, R.ABS) == tuple(got[5:12])
    # the stream ids are new: no other Philox draw of the library uses them (wl_rng.h, the task enums, the terrain header)
    rng_h = open(os.path.join(ROOT, "wheeledlab_amd", "csrc", "wl_rng.h")).read()
    ids = {int(v) for v in re.findall(r"WL_RS_[A-Z0-9_]+ = (\d+)", rng_h)}
    assert {16, 17} <= ids and len(re.findall(r"WL_RS_[A-Z0-9_]+ = (\d+)", rng_h)) == len(ids)
    terrain_h = open(os.path.join(ROOT, "include", "wheeledlab_amd_terrain.h")).read()
    assert not {16, 17} & {int(v) for v in re.findall(r"#define WL_TS_[A-Z_]+ (\d+)", terrain_h)}


def test_width_accepts_good_tables_and_refuses_bad_ones():
    lib = _lib()

    def width(tab, D, n_terms=None):
        rows = R.rows(tab)
        return lib.wl_obs_corrupt_width(_ctable(rows), len(rows) if n_terms is None else n_terms, D)
    for name, terms in TABLES.items():
        tab, D, Db = R.table(terms)
        assert width(tab, D) == Db, name
    assert [R.table(TABLES[k])[1:] for k in ("drift", "elevation", "visual", "identity")] == [(14, 3), (689, 0), (3208, 0), (5, 0)]
    good, D, Db = R.table([R.term(3, R.uniform(-1, 1), bias=R.constant(0.5)), R.term(2, R.gaussian(0, 1), bias=R.uniform(0, 1), per_component=False),
                           R.term(4, clip=(-1.0, 1.0), scale=2.0)])
    assert width(good, D) == Db == 4

    def bad(k, **kw):
        t = [dict(x) for x in good]
        t[k].update(kw)
        return t
    inf, nan = float("inf"), float("nan")
    for what, tab, d in (("gap", bad(1, off=4), D), ("overlap", bad(1, off=2), D), ("width 0", bad(1, width=0), D), ("negative width", bad(0, width=-3), D),
                         ("unknown noise kind", bad(0, noise_kind=4), D), ("negative kind", bad(0, noise_kind=-1), D),
                         ("unknown bias kind", bad(0, bias_kind=7), D), ("unknown operation", bad(0, noise_op=3), D),
                         ("negative operation", bad(1, noise_op=-1), D), ("clip_lo > clip_hi", bad(2, clip_lo=1.0, clip_hi=-1.0), D),
                         ("NaN clip", bad(2, clip_lo=nan), D), ("bias_off not the running sum", bad(1, bias_off=2), D),
                         ("bias_off of a later term", bad(2, bias_off=3), D), ("bias without noise", bad(2, bias_kind=R.CONSTANT), D),
                         ("per_component 2", bad(0, bias_per_component=2), D), ("infinite parameter", bad(0, noise_b=inf), D),
                         ("NaN parameter", bad(1, noise_a=nan), D), ("NaN scale", bad(2, scale=nan), D), ("scale without its flag", bad(2, has_scale=0), D),
                         ("D too small", good, D - 1), ("D too large", good, D + 1), ("D 0", good, 0), ("D above the maximum", good, (1 << 20) + 1),
                         ("first term not at 0", bad(0, off=1), D)):
        assert width(tab, d) == -1, what
    assert width(good, D, n_terms=0) == -1 and lib.wl_obs_corrupt_width(None, 3, D) == -1
    big, Dbig, Dbb = R.table([R.term(1, R.constant(1.0), bias=R.constant(1.0))] * 64)
    assert width(big, Dbig) == Dbb == 64
    over, Do, _ = R.table([R.term(1)] * 65)
    assert width(over, Do) == -1                                              # n_terms 65
    wide, Dw, _ = R.table([R.term(1 << 20)])
    assert width(wide, Dw) == 0


def test_apply_refuses_bad_arguments_without_a_gpu():
    """every defect alone is refused with its code before anything is launched (no GPU here: a launch would fail as WL_ELAUNCH)"""
    lib = _lib()
    tab, D, Db = R.table(TABLES["drift"])
    ct = _ctable(R.rows(tab))
    n = 64
    fake = 1 << 24                     # never dereferenced: every call below returns before any launch
    base = dict(n=n, D=D, obs=fake, ostride=D, terms=ct, n_terms=len(tab), state=fake + (1 << 20), sstride=n, bias=fake + (2 << 20), ra=fake + (3 << 20),
                rb=fake + (3 << 20) + 4096, out=fake + (4 << 20), outstride=D, enable=1)

    def apply(**kw):
        a = {**base, **kw}
        return lib.wl_obs_corrupt_apply(a["n"], a["D"], a["obs"], a["ostride"], a["terms"], a["n_terms"], a["state"], a["sstride"], a["bias"], a["ra"],
                                        a["rb"], a["out"], a["outstride"], 42, 7, 0, a["enable"], None)
    for k in ("obs", "out", "ra", "terms", "state", "bias"):
        assert apply(**{k: None}) == -1, k
    for kw in (dict(n=0), dict(n=-1), dict(ostride=D - 1), dict(outstride=D - 1), dict(D=D + 1), dict(D=0), dict(n_terms=0), dict(n_terms=len(tab) - 1),
               dict(n_terms=65), dict(sstride=n - 1)):
        assert apply(**kw) == -1, kw
    rows = ((n - 1) * D + D) * 4
    for kw in (dict(out=fake + 4), dict(out=fake + rows - 4), dict(out=fake - rows + 4),                          # out / obs overlap in part
               dict(out=fake, outstride=D + 2, ostride=D),                                                         # the same start, another pitch
               dict(out=base["bias"]), dict(out=base["bias"] + n * Db * 4 - 4)):                                 # out / bias overlap
        assert apply(**kw) == -1, kw
    # what the launch stores (out, bias) on what it reads: the flags, the two state rows of last_action, and bias on obs
    act = base["state"] + tab[4]["state_row"] * n * 4
    for kw in (dict(out=base["ra"] - rows + 4), dict(out=base["rb"] + n - 4), dict(bias=base["ra"] + n - 4), dict(bias=base["rb"] - n * Db * 4 + 4),
               dict(out=act - rows + 4), dict(out=act + 2 * n * 4 - 4), dict(bias=act + 2 * n * 4 - 4), dict(bias=act - n * Db * 4 + 4),
               dict(bias=fake + rows - 4), dict(bias=fake - n * Db * 4 + 4)):
        assert apply(**kw) == -1, kw
    for k in ("obs", "out", "state", "bias"):
        for off in (1, 2, 3):
            assert apply(**{k: base[k] + off}) == -3, (k, off)
    assert apply(n=(1 << 31) // D + 1, sstride=1 << 30, out=1 << 40) == -1                                       # n * stride past 2^31
    assert apply(ostride=1 << 26) == -1 and apply(outstride=1 << 26) == -1
    bad = R.rows(tab)
    bad[2] = bad[2][:2] + (9,) + bad[2][3:]
    assert apply(terms=_ctable(bad)) == -1
    far = [dict(t) for t in tab]
    far[4]["state_row"] = A.S_COUNT - 1                                       # two rows from the last row of the state
    assert apply(terms=_ctable(R.rows(far))) == -1
    # a table without bias or state terms needs neither buffer
    tab2, D2, _ = R.table(TABLES["identity"])
    ok_args = dict(terms=_ctable(R.rows(tab2)), n_terms=len(tab2), D=D2, ostride=D2, outstride=D2, state=None, bias=None)
    assert apply(**ok_args, n=0) == -1 and apply(**ok_args, ra=None) == -1
    # (the calls that ARE accepted -- in place, strided rows, a NULL reset_b, `out` off the 16-byte line -- launch:
    # tests/test_gpu_obs_corrupt.py makes them on real buffers)


# ---- config classes and resolution -------------------------------------------------------------------------------------

def _group(task="Isaac-MushrDriftRL-v0"):
    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    from wheeledlab_amd.envs.configclass import fields_of
    cfg = registry.parse_env_cfg(task, device="cpu", num_envs=4)
    pol = cfg.observations.policy
    return cfg, pol, [(k, v) for k, v in fields_of(pol) if hasattr(v, "func")]


TASKS = {"Isaac-MushrDriftRL-v0": "drift", "Isaac-MushrElevationRL-v0": "elevation", "Isaac-MushrVisualRL-v0": "visual",
         "Isaac-MushrVisualDepthRL-v0": "visual_depth"}


def _widths(task):
    from wheeledlab_amd import core
    return list({"drift": core.DriftBatch, "elevation": core.ElevBatch, "visual": core.VisualBatch,
                 "visual_depth": core.VisualDepthBatch}[TASKS[task]].OBS_TERM_WIDTHS)


def test_config_classes_have_isaaclab_field_names_and_defaults():
    from wheeledlab_amd.envs import managers_cfg as M
    assert M.NoiseCfg().operation == "add" and M.ConstantNoiseCfg().bias == 0.0 and M.ConstantNoiseCfg().operation == "add"
    assert M.GaussianNoiseCfg is M.AdditiveGaussianNoiseCfg and M.UniformNoiseCfg is M.AdditiveUniformNoiseCfg
    g, u = M.GaussianNoiseCfg(std=0.5, operation="scale"), M.UniformNoiseCfg(n_min=-2.0)
    assert (g.mean, g.std, g.operation, u.n_min, u.n_max, u.operation) == (0.0, 0.5, "scale", -2.0, 1.0, "add")
    m = M.NoiseModelWithAdditiveBiasCfg(noise_cfg=g, bias_noise_cfg=u)
    assert m.sample_bias_per_component is True and m.noise_cfg is g and m.bias_noise_cfg is u and isinstance(m, M.NoiseModelCfg)
    assert M.NoiseModelCfg(noise_cfg=u).noise_cfg is u


def test_resolve_is_none_for_every_shipped_config_and_the_fused_drift_gaussian():
    from wheeledlab_amd.envs.corruption import resolve
    from wheeledlab_amd.envs.flatten import flatten_cfg
    for task, kind in TASKS.items():
        cfg, pol, terms = _group(task)
        assert resolve(pol, terms, _widths(task), kind) is None, task
        assert flatten_cfg(cfg).corruption is False
    cfg, pol, terms = _group()
    assert pol.enable_corruption and all(t.noise is not None for _, t in terms[:4])       # the shipped drift noise: fused in the step
    flat = flatten_cfg(cfg)
    assert flat.params.enable_corruption == 1 and [round(flat.params.noise_std[i], 6) for i in range(4)] == [0.1, 0.1, 0.5, 0.4]


def test_resolve_builds_a_layout_for_each_trigger():
    from wheeledlab_amd.envs import managers_cfg as M
    from wheeledlab_amd.envs.corruption import resolve
    from wheeledlab_amd.envs.flatten import flatten_cfg
    w = _widths("Isaac-MushrDriftRL-v0")

    def drift(change):
        cfg, pol, terms = _group()
        change(pol, terms)
        L = resolve(pol, terms, w, "drift")
        flat = flatten_cfg(cfg)
        assert L is not None and flat.corruption and flat.params.enable_corruption == 0 and all(flat.params.noise_std[i] == 0 for i in range(4))
        assert (L.D, len(L.terms)) == (14, 5) and L.names == tuple(n for n, _ in terms)
        assert L.terms[4][R.FIELDS.index("state_row")] == A.S_ACT0 and L.terms[4][12:14] == (-1.0, 1.0)
        return L
    L = drift(lambda pol, t: setattr(t[2][1], "noise", M.UniformNoiseCfg(n_min=-0.1, n_max=0.1)))                 # uniform noise
    assert L.terms[2][2:6] == (A.OC_UNIFORM, A.OC_ADD, R.f32(-0.1), float(np.float32(0.1) - np.float32(-0.1))) and L.Db == 0 and L.enable
    assert L.terms[0][2:6] == (A.OC_GAUSSIAN, A.OC_ADD, 0.0, R.f32(0.1))                                          # the others move with it
    L = drift(lambda pol, t: setattr(t[0][1], "noise", M.GaussianNoiseCfg(mean=0.05, std=0.1)))                  # a mean
    assert L.terms[0][4:6] == (R.f32(0.05), R.f32(0.1))
    L = drift(lambda pol, t: setattr(t[1][1], "noise", M.ConstantNoiseCfg(bias=0.1)))                            # a constant bias
    assert L.terms[1][2:5] == (A.OC_CONSTANT, A.OC_ADD, R.f32(0.1))
    L = drift(lambda pol, t: setattr(t[3][1], "noise", M.GaussianNoiseCfg(std=1.1, operation="scale")))          # operation scale
    assert L.terms[3][2:4] == (A.OC_GAUSSIAN, A.OC_SCALE)
    L = drift(lambda pol, t: setattr(t[3][1], "noise", M.NoiseModelCfg(noise_cfg=M.GaussianNoiseCfg(std=0.4))))  # a noise model
    assert L.terms[3][2] == A.OC_GAUSSIAN and L.Db == 0
    model = M.NoiseModelWithAdditiveBiasCfg(noise_cfg=M.GaussianNoiseCfg(std=0.4), bias_noise_cfg=M.UniformNoiseCfg(n_min=-0.05, n_max=0.05))
    L = drift(lambda pol, t: setattr(t[3][1], "noise", model))
    assert L.Db == 3 and L.terms[3][6:11] == (A.OC_UNIFORM, 1, R.f32(-0.05), float(np.float32(0.05) - np.float32(-0.05)), 0)
    model.sample_bias_per_component = False
    assert drift(lambda pol, t: setattr(t[3][1], "noise", model)).Db == 1
    model.bias_noise_cfg = M.GaussianNoiseCfg(std=0.3, operation="scale")                                        # 0 * n: no bias at all
    assert drift(lambda pol, t: setattr(t[3][1], "noise", model)).terms[3][6:10] == (A.OC_CONSTANT, 0, 0.0, 0.0)
    L = drift(lambda pol, t: setattr(t[4][1], "noise", M.UniformNoiseCfg(n_min=-0.1, n_max=0.1)))                # noise on last_action
    assert L.terms[4][2] == A.OC_UNIFORM
    L = drift(lambda pol, t: setattr(t[2][1], "clip", (-3.0, 3.0)))                                              # a clip
    assert L.terms[2][12:14] == (-3.0, 3.0) and L.terms[2][11] == 0
    L = drift(lambda pol, t: setattr(t[0][1], "scale", 0.5))                                                     # a scale
    assert L.terms[0][11] == 1 and L.terms[0][14] == 0.5

    def off(pol, t):                                                                                             # corruption off: the layer still
        pol.enable_corruption = False                                                                            # clips, and draws nothing
        t[2][1].clip = (-3.0, 3.0)
    assert drift(off).enable is False
    # elevation / visual / visual-depth: enable_corruption with any noise on a fused term
    for task, kind in TASKS.items():
        if kind == "drift":
            continue
        cfg, pol, terms = _group(task)
        pol.enable_corruption = True
        if kind == "elevation":
            assert resolve(pol, terms, _widths(task), kind) is None and not flatten_cfg(cfg).corruption      # no noise declared: nothing to build
            terms[1][1].noise = M.GaussianNoiseCfg(std=0.02)
        L = resolve(pol, terms, _widths(task), kind)
        assert L is not None and L.D == sum(_widths(task)) and L.enable and flatten_cfg(cfg).corruption
        la = [i for i, (_, t) in enumerate(terms) if t.func.__name__ == "last_action"][0]
        assert L.terms[la][15] == A.S_ACT0 and L.terms[la][12:14] == (-1.0, 1.0) and all(r[15] == -1 for i, r in enumerate(L.terms) if i != la)
        if kind != "elevation":
            assert [r[2] for r in L.terms] == [A.OC_NONE, A.OC_UNIFORM, A.OC_UNIFORM, A.OC_UNIFORM]              # the declared Unoise
        else:
            assert L.terms[5][12:14] == (-10.0, 10.0)                                                           # the pre-clipped map: clipped again
    # a plugin term: a plain Gaussian stays with the torch chain, anything else moves into the layer
    cfg, pol, terms = _group("Isaac-MushrElevationRL-v0")
    pol.enable_corruption = True
    pol.extra = M.ObservationTermCfg(func=len, noise=M.GaussianNoiseCfg(std=0.1))
    terms2 = terms + [("extra", pol.extra)]
    assert resolve(pol, terms2, _widths("Isaac-MushrElevationRL-v0") + [7], "elevation") is None
    pol.extra.noise, pol.extra.clip, pol.extra.scale = M.ConstantNoiseCfg(bias=0.05), (0.0, 2.0), 0.5
    L = resolve(pol, terms2, _widths("Isaac-MushrElevationRL-v0") + [7], "elevation")
    assert L.D == 689 + 7 and L.terms[6] == (689, 7, A.OC_CONSTANT, A.OC_ADD, R.f32(0.05), 0.0, A.OC_NONE, 1, 0.0, 0.0, 0, 1, 0.0, 2.0, 0.5, -1)
    pol.enable_corruption = False
    assert resolve(pol, terms2, _widths("Isaac-MushrElevationRL-v0") + [7], "elevation") is None


def test_value_errors_name_the_term():
    import torch
    from wheeledlab_amd.envs import managers_cfg as M
    from wheeledlab_amd.envs.corruption import resolve
    from wheeledlab_amd.envs.flatten import flatten_cfg
    w = _widths("Isaac-MushrDriftRL-v0")
    for make in (lambda: M.GaussianNoiseCfg(std=torch.ones(3)), lambda: M.GaussianNoiseCfg(mean=[0.0, 0.1, 0.2]),
                 lambda: M.UniformNoiseCfg(n_min=np.zeros(3)), lambda: M.UniformNoiseCfg(n_max=(1.0, 2.0, 3.0)),
                 lambda: M.ConstantNoiseCfg(bias=torch.zeros(3)), lambda: M.GaussianNoiseCfg(operation="multiply"),
                 lambda: M.NoiseModelWithAdditiveBiasCfg(noise_cfg=M.GaussianNoiseCfg(), bias_noise_cfg=M.GaussianNoiseCfg(std=torch.ones(3))),
                 lambda: M.NoiseModelCfg(noise_cfg=M.NoiseCfg()), lambda: M.UniformNoiseCfg(n_min=1.0, n_max=-1.0), lambda: M.GaussianNoiseCfg(std=-0.1)):
        cfg, pol, terms = _group()
        terms[2][1].noise = make()
        with pytest.raises(ValueError, match=terms[2][0]):
            resolve(pol, terms, w, "drift")
        with pytest.raises(ValueError, match=terms[2][0]):
            flatten_cfg(cfg)
    for field, value in (("scale", torch.ones(3)), ("scale", (1.0, 2.0, 3.0)), ("clip", (torch.zeros(3), torch.ones(3))), ("clip", (1.0, -1.0))):
        cfg, pol, terms = _group()
        setattr(terms[1][1], field, value)
        with pytest.raises(ValueError, match=terms[1][0]):
            resolve(pol, terms, w, "drift")
    cfg, pol, terms = _group()
    with pytest.raises(ValueError, match="widths"):
        resolve(pol, terms, w[:-1], "drift")


def test_existing_refusals_stay():
    from wheeledlab_amd.envs import managers_cfg as M
    from wheeledlab_amd.envs.flatten import flatten_cfg
    cfg, pol, terms = _group()
    terms[2][1].noise = M.UniformNoiseCfg(n_min=-0.1, n_max=0.1)
    terms[4][1].clip = (-2.0, 2.0)
    with pytest.raises(NotImplementedError, match="last_action"):
        flatten_cfg(cfg)
    cfg, pol, terms = _group("Isaac-MushrElevationRL-v0")
    pol.enable_corruption = True
    terms[2][1].noise, terms[2][1].clip = M.GaussianNoiseCfg(std=0.1), (-5.0, 5.0)
    with pytest.raises(NotImplementedError, match="velocity clips"):
        flatten_cfg(cfg)
    cfg, pol, terms = _group("Isaac-MushrVisualRL-v0")
    pol.enable_corruption = True
    pol.base_lin_vel, pol.base_ang_vel = pol.base_ang_vel, pol.base_lin_vel
    with pytest.raises(NotImplementedError, match="layout"):
        flatten_cfg(cfg)


def test_train_script_override_reaches_the_group():
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.envs import managers_cfg as M
    from wheeledlab_amd.envs.flatten import flatten_cfg
    run = resolve_run("RSS_ELEV_CONFIG", ["env.observations.policy.enable_corruption=true"])
    assert run.env.observations.policy.enable_corruption is True and not flatten_cfg(run.env).corruption         # nothing declares a noise
    run = resolve_run("RSS_ELEV_CONFIG", ["env.observations.policy.enable_corruption=true", "env.observations.policy.base_lin_vel.noise={'std': 0.1}",
                                          "env.observations.policy.base_ang_vel.noise={'n_min': -0.2, 'n_max': 0.2, 'operation': 'add'}"])
    assert flatten_cfg(run.env).corruption                                     # the dicts became the configs their fields name
    pol = run.env.observations.policy
    assert isinstance(pol.base_lin_vel.noise, M.GaussianNoiseCfg) and pol.base_lin_vel.noise.std == 0.1 and pol.base_lin_vel.noise.mean == 0.0
    assert isinstance(pol.base_ang_vel.noise, M.UniformNoiseCfg) and pol.base_ang_vel.noise.n_max == 0.2
    run = resolve_run("RSS_ELEV_CONFIG", ["env.observations.policy.enable_corruption=true", "env.observations.policy.base_lin_vel.noise={'sigma': 0.1}"])
    with pytest.raises(ValueError, match="base_lin_vel"):
        flatten_cfg(run.env)


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
    return _build(tmp_path_factory.mktemp("host_sim") / "obs_corrupt_host")


def pack_table(tab):
    return b"".join(struct.pack("<iiiiffiiffiifffi", *r) for r in R.rows(tab))


def run_host(exe, tmp, tab, D, obs, state, bias, ra, rb, seed, step, env_offset, enable, out_stride=None, in_place=False, env=None):
    n, stride = obs.shape
    out_stride = stride if in_place else (D if out_stride is None else out_stride)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    srows, sstride = (0, 0) if state is None else state.shape
    with open(fin, "wb") as f:
        f.write(struct.pack("<10q", n, D, stride, out_stride, len(tab), int(rb is not None), srows, sstride, int(enable), int(in_place)))
        f.write(struct.pack("<3Q", seed, step, env_offset))
        f.write(pack_table(tab))
        f.write(np.ascontiguousarray(obs, np.uint32).tobytes())
        if state is not None:
            f.write(np.ascontiguousarray(state, np.uint32).tobytes())
        f.write(np.ascontiguousarray(bias, np.float32).tobytes())
        f.write(np.ascontiguousarray(ra, np.uint8).tobytes())
        if rb is not None:
            f.write(np.ascontiguousarray(rb, np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, env=env)
    raw = open(fout, "rb").read()
    Db = struct.unpack("<q", raw[:8])[0]
    if Db < 0:
        assert len(raw) == 8
        return None
    m, p = n * out_stride, 8
    out = np.frombuffer(raw[p:p + 4 * m], np.uint32).reshape(n, out_stride)
    p += 4 * m
    nb = np.frombuffer(raw[p:p + 4 * n * Db], np.float32).reshape(n, Db)
    p += 4 * n * Db
    writes = np.frombuffer(raw[p:p + m], np.uint8).reshape(n, out_stride)
    assert p + m == len(raw)
    return out, nb, writes


def _check_host(exe, tmp, name, n, enable=True, with_b=True, stride_extra=0, out_extra=0, in_place=False, env=None, step=5, env_offset=11):
    tab, D, Db = R.table(TABLES[name])
    rng = np.random.default_rng(n + len(name) + stride_extra)
    obs = special_words(rng, (n, D + stride_extra))
    state = R.state_block(rng, n, stride=n + 3)
    bias = rng.standard_normal((n, Db)).astype(np.float32)
    ra, rb = rng.random(n) < 0.4, rng.random(n) < 0.3
    seed = 0x1234_5678_9ABC_DEF0
    got = run_host(exe, tmp, tab, D, obs, state, bias, ra, rb if with_b else None, seed, step, env_offset, enable, out_stride=D + out_extra,
                   in_place=in_place, env=env)
    out, nb, writes = got
    res = R.apply(tab, obs[:, :D], bias, ra | rb if with_b else ra, seed, step, env_offset, enable, state=state, ez=R.EZ_HOST)
    R.check(out[:, :D], res, what=f"{name} n={n}")
    R.check_bias(nb, res, what=f"{name} n={n}")
    assert (writes[:, :D] == 1).all() and (writes[:, D:] == 0).all()
    if not in_place:
        assert (out[:, D:] == 0xDEADBEEF).all()
    else:
        assert np.array_equal(out[:, D:], obs[:, D:])
    if not enable:
        assert np.array_equal(nb.view(np.uint32), bias.view(np.uint32))
    return res


@pytest.mark.parametrize("name", [k for k in TABLES if k != "visual"])
def test_host_body_equals_the_reference(exe, tmp_path, name):
    for n in (1, 3, 9):
        res = _check_host(exe, str(tmp_path), name, n)
    if name.startswith("every"):
        assert res.arith[:-3].all() and not res.arith[-3:].any() and (~res.exact).any()        # (the Gaussian biases of every table)
    if name == "identity":
        assert not res.arith.any()
    _check_host(exe, str(tmp_path), name, 5, enable=False)
    _check_host(exe, str(tmp_path), name, 5, with_b=False, stride_extra=3, out_extra=2)
    _check_host(exe, str(tmp_path), name, 4, in_place=True, stride_extra=1)
    _check_host(exe, str(tmp_path), name, 2, step=(1 << 40) + 3, env_offset=(1 << 33) + 5)


def test_host_nan_in_gives_nan_out_and_clip_keeps_it(exe, tmp_path):
    for name in ("every_constant", "every_uniform", "every_gaussian"):
        tab, D, Db = R.table(TABLES[name])
        n = 3
        obs = np.full((n, D), 0x7FC00001, np.uint32)
        obs[1] = 0xFF800123                                                    # a signalling NaN, negative
        out, _, _ = run_host(exe, str(tmp_path), tab, D, obs, None, np.zeros((n, Db), np.float32), np.ones(n, bool), None, 1, 2, 3, True)
        assert np.isnan(out.view(np.float32)).all(), name


def test_host_program_refuses_a_bad_table(exe, tmp_path):
    tab, D, Db = R.table(TABLES["drift"])
    tab[3]["bias_off"] += 1
    assert run_host(exe, str(tmp_path), tab, D, np.zeros((2, D), np.uint32), np.zeros((R.ACT_ROW + 2, 2), np.uint32), np.zeros((2, Db), np.float32),
                    np.zeros(2, bool), None, 1, 2, 3, True) is None


def test_host_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path / "obs_corrupt_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for name in TABLES:
        if name == "visual":
            continue
        for n in (1, 5):
            _check_host(exe, str(tmp_path), name, n, env=env)
        _check_host(exe, str(tmp_path), name, 4, enable=False, with_b=False, stride_extra=5, out_extra=1, env=env)
        _check_host(exe, str(tmp_path), name, 3, in_place=True, env=env)

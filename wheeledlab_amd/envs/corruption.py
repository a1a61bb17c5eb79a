"""Observation corruption: the noise (`ObservationTermCfg.noise`: a NoiseCfg or a noise model, managers_cfg.py), `clip` and `scale` of
every term of the policy group resolved into the term table of include/wheeledlab_amd_obsnoise.h, and the per-env bias block an env
with corruption owns.  In IsaacLab's ObservationManager order: term -> noise -> clip -> scale -> history.

The layer is built only when the config holds something the fused step kernels cannot express (needed() below); otherwise nothing is
built, no path gains a launch and every output is what it was.  DESIGN.md section 20 states the semantics.  resolve() is arithmetic on
Python scalars and needs no device."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .. import _abi as A
from .layers import BatchLayer
from .managers_cfg import (AdditiveGaussianNoiseCfg, AdditiveUniformNoiseCfg, ConstantNoiseCfg, NoiseCfg, NoiseModelCfg,
                           NoiseModelWithAdditiveBiasCfg)

OPERATIONS = {"add": A.OC_ADD, "scale": A.OC_SCALE, "abs": A.OC_ABS}
# the fused layouts: task -> the terms the step kernel writes, in order (flatten.py checks the config against them)
FUSED_TERMS = {"drift": 5, "elevation": 6, "visual": 4, "visual_depth": 4}


@dataclass(frozen=True)
class CorruptionLayout:
    terms: tuple          # per term the fields of WlObsCorruptTerm, in order: the table of wl_obs_corrupt_apply
    names: tuple          # the term each table entry stands for
    D: int                # the row
    Db: int               # floats of bias per env
    enable: bool          # observations.policy.enable_corruption: off, the layer still clips and scales


def _f32(v) -> float:
    return float(np.float32(v))


def _scalar(v, term: str, what: str) -> float:
    """a Python (or 0-dim numpy) number; tensors and sequences are refused"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"observation term '{term}': {what} must be a Python scalar, got {type(v).__name__} (tensor- and sequence-valued "
                         "noise parameters, clips and scales are not supported)")
    v = float(v)
    if not math.isfinite(v) and "clip" not in what:
        raise ValueError(f"observation term '{term}': {what} is {v}")
    return v


def _noise(cfg, term: str, what: str = "noise"):
    """a NoiseCfg -> (kind, operation, a, b) of the table"""
    if not isinstance(cfg, NoiseCfg):
        raise ValueError(f"observation term '{term}': {what} is {type(cfg).__name__}, not a NoiseCfg")
    op = getattr(cfg, "operation", "add")
    if op not in OPERATIONS:
        raise ValueError(f"observation term '{term}': {what}.operation is {op!r}: one of {sorted(OPERATIONS)}")
    if isinstance(cfg, ConstantNoiseCfg):
        return A.OC_CONSTANT, OPERATIONS[op], _f32(_scalar(cfg.bias, term, f"{what}.bias")), 0.0
    if isinstance(cfg, AdditiveUniformNoiseCfg):
        lo, hi = _scalar(cfg.n_min, term, f"{what}.n_min"), _scalar(cfg.n_max, term, f"{what}.n_max")
        if lo > hi:
            raise ValueError(f"observation term '{term}': {what}.n_min {lo} > n_max {hi}")
        return A.OC_UNIFORM, OPERATIONS[op], _f32(lo), float(np.float32(hi) - np.float32(lo))      # the span: formed once, in fp32
    if isinstance(cfg, AdditiveGaussianNoiseCfg):
        std = _scalar(cfg.std, term, f"{what}.std")
        if std < 0:
            raise ValueError(f"observation term '{term}': {what}.std {std} < 0")
        return A.OC_GAUSSIAN, OPERATIONS[op], _f32(_scalar(cfg.mean, term, f"{what}.mean")), _f32(std)
    raise ValueError(f"observation term '{term}': {what} is a bare {type(cfg).__name__}: ConstantNoiseCfg, UniformNoiseCfg or GaussianNoiseCfg")


def _as_cfg(noise, term: str):
    """a noise given as a dict (a command-line override: `...base_lin_vel.noise={'std': 0.1}`) -> the config it names by its fields:
    std / mean: Gaussian, n_min / n_max: uniform, bias: constant; `operation` goes with any"""
    if not isinstance(noise, dict):
        return noise
    keys = set(noise) - {"operation"}
    for cls, own in ((AdditiveGaussianNoiseCfg, {"mean", "std"}), (AdditiveUniformNoiseCfg, {"n_min", "n_max"}), (ConstantNoiseCfg, {"bias"})):
        if keys and keys <= own:
            return cls(**noise)
    raise ValueError(f"observation term '{term}': noise {noise!r} names no noise config (fields std / mean, n_min / n_max, or bias, and operation)")


def _parse(noise, term: str):
    """ObservationTermCfg.noise -> (noise (kind, op, a, b), bias (kind, a, b) or None, per_component)"""
    if noise is None:
        return (A.OC_NONE, A.OC_ADD, 0.0, 0.0), None, True
    if isinstance(noise, NoiseModelCfg):
        main = _noise(noise.noise_cfg, term, "noise.noise_cfg")
        if not isinstance(noise, NoiseModelWithAdditiveBiasCfg):
            return main, None, True
        kind, op, a, b = _noise(noise.bias_noise_cfg, term, "noise.bias_noise_cfg")
        if op == A.OC_SCALE:              # the bias model applies bias_noise_cfg to ZEROS: 0 * n
            kind, a, b = A.OC_CONSTANT, 0.0, 0.0
        return main, (kind, a, b), bool(noise.sample_bias_per_component)
    return _noise(noise, term), None, True


def _is_plain(noise) -> bool:
    """what the torch chain of a plugin term applies: an additive Gaussian or uniform NoiseCfg"""
    return isinstance(noise, (AdditiveGaussianNoiseCfg, AdditiveUniformNoiseCfg)) and getattr(noise, "operation", "add") == "add"


def _is_fused_gaussian(noise) -> bool:
    """what the drift step draws itself: a zero-mean additive Gaussian"""
    return isinstance(noise, AdditiveGaussianNoiseCfg) and getattr(noise, "operation", "add") == "add" and noise.mean == 0.0


def normalise(terms) -> None:
    """config resolution, the one place a term's config is rewritten: a noise that arrived as a dict (a command-line override) becomes
    the config its fields name, in place.  Idempotent; flatten_cfg() calls it before it asks needed()."""
    for name, t in terms:
        if isinstance(getattr(t, "noise", None), dict):
            t.noise = _as_cfg(t.noise, name)


def _parse_all(terms) -> list:
    """every term's noise parsed once: a tensor-valued parameter is a ValueError here, before any device work"""
    return [_parse(getattr(t, "noise", None), name) for name, t in terms]


def needed(group, terms, task: str) -> bool:
    """does the config hold what the fused kernels refuse or cannot express?  terms: [(name, ObservationTermCfg)] in row order, noises
    as configs (normalise()).  Every noise is validated on the way.  Changes nothing."""
    _parse_all(terms)
    return _needed(group, terms, task)


def _needed(group, terms, task: str) -> bool:
    n_fused = FUSED_TERMS[task]
    enable = bool(getattr(group, "enable_corruption", False))
    fused, plugin = terms[:n_fused], terms[n_fused:]
    if task == "drift":
        for _, t in fused[:4]:
            if (t.noise is not None and not _is_fused_gaussian(t.noise)) or t.clip is not None or t.scale is not None:
                return True
        if fused[4][1].noise is not None:
            return True
    elif enable and any(t.noise is not None for _, t in fused):
        return True
    return enable and any(getattr(t, "noise", None) is not None and not _is_plain(t.noise) for _, t in plugin)


def resolve(group, terms, widths, fused_layout) -> CorruptionLayout | None:
    """group: an ObservationGroupCfg; terms: [(name, ObservationTermCfg)] in the order of the raw row -- the fused terms in layout
    order, then the plugin terms; widths: the columns of each; fused_layout: the task whose step kernel writes the leading terms
    ("drift", "elevation", "visual", "visual_depth").  -> the layout, or None when nothing needs the layer."""
    if len(terms) != len(widths):
        raise ValueError(f"{len(terms)} observation terms but {len(widths)} widths")
    task = str(fused_layout)
    parsed = _parse_all(terms)
    if not _needed(group, terms, task):
        return None
    if len(terms) > A.OBSCORRUPT_MAX_TERMS:
        raise ValueError(f"observation corruption over {len(terms)} terms: at most {A.OBSCORRUPT_MAX_TERMS}")
    n_fused = FUSED_TERMS[task]
    rows, off, boff = [], 0, 0
    for i, ((name, t), w) in enumerate(zip(terms, widths)):
        (kind, op, a, b), bias, per = parsed[i]
        lo, hi = -math.inf, math.inf
        if getattr(t, "clip", None) is not None:
            if not isinstance(t.clip, (tuple, list)) or len(t.clip) != 2:
                raise ValueError(f"observation term '{name}': clip must be (lo, hi)")
            lo, hi = _scalar(t.clip[0], name, "clip[0]"), _scalar(t.clip[1], name, "clip[1]")
            if not lo <= hi:
                raise ValueError(f"observation term '{name}': clip {lo} > {hi}")
        scale = None if getattr(t, "scale", None) is None else _f32(_scalar(t.scale, name, "scale"))
        # last_action of a fused layout: the kernel wrote it CLIPPED; IsaacLab adds the noise before the clip, so the layer reads
        # the raw action from the state
        state_row = A.S_ACT0 if i < n_fused and getattr(t.func, "__name__", "") == "last_action" else -1
        bk, ba, bb = bias or (A.OC_NONE, 0.0, 0.0)
        rows.append((off, int(w), kind, op, a, b, bk, int(per), ba, bb, boff, int(scale is not None), _f32(lo), _f32(hi),
                     1.0 if scale is None else scale, state_row))
        off += int(w)
        if bk != A.OC_NONE:
            boff += int(w) if per else 1
    return CorruptionLayout(tuple(rows), tuple(n for n, _ in terms), off, boff, bool(getattr(group, "enable_corruption", False)))


class ObsCorruption(BatchLayer):
    """the layer of one env batch: the table, the bias block [n, Db] and the launch"""

    def __init__(self, layout: CorruptionLayout, batch):
        import torch
        super().__init__(batch)                                                     # (self.all: env.reset())
        self.layout = layout
        self.table = (A.WlObsCorruptTerm * len(layout.terms))(*[A.WlObsCorruptTerm(*t) for t in layout.terms])
        if self.lib.wl_obs_corrupt_width(self.table, len(layout.terms), layout.D) != layout.Db:
            raise ValueError(f"observation corruption: the term table {layout.terms} is not one of rows of {layout.D}")
        self.bias = torch.zeros(self.n, max(layout.Db, 1), dtype=torch.float32, device=self.device)
        self.row = torch.zeros(self.n, layout.D, dtype=torch.float32, device=self.device)   # the env's own corrupted row
        self.filled = False

    def apply(self, raw, out, reset_a, reset_b=None, step=None):
        """one launch: out = the corrupted raw rows at `step` (None: the batch's step count)"""
        import torch
        L, b = self.layout, self.batch
        assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.shape == (self.n, L.D) and raw.stride(1) == 1, (raw.shape, raw.stride())
        assert out.dtype == torch.float32 and out.shape == (self.n, L.D) and out.stride(1) == 1, (out.shape, out.stride())
        assert reset_a.dtype in (torch.bool, torch.uint8) and reset_a.numel() == self.n
        A.check(self.lib.wl_obs_corrupt_apply(self.n, L.D, raw.data_ptr(), raw.stride(0), self.table, len(L.terms), b.state.data_ptr(),
                                              b.stride, self.bias.data_ptr() if L.Db else None, reset_a.data_ptr(),
                                              None if reset_b is None else reset_b.data_ptr(), out.data_ptr(), out.stride(0), b.seed,
                                              b.step_count if step is None else int(step), b.env_offset, int(L.enable), A.stream(self.device)),
                "wl_obs_corrupt_apply")
        return out

    def corrupt(self, raw, reset_a, reset_b=None):
        """the env's own row advances: -> the corrupted row (the buffer the env keeps until its next step)"""
        self.apply(raw, self.row, reset_a, reset_b)
        self.filled = True
        return self.row

    def adopt(self, rows):
        """the env's row catches up with a collector that corrupted into its own storage"""
        self.row.copy_(rows.reshape(self.n, self.layout.D))
        self.filled = True
        return self.row

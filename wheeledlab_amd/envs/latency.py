"""Action latency: the `latency` field of an action term (actions.ActionLatencyCfg) resolved into the three numbers of
include/wheeledlab_amd_latency.h, and the per-env block and delayed-action buffer an env with latency owns.

The layer is built only when a config asks for it; otherwise nothing is built, no path gains a launch and every output is what it was.
DESIGN.md section 22 states the semantics -- a restatement of IsaacLab's DelayBuffer as DelayedPDActuator uses it, counted in control
steps; IsaacLab is not vendored with the reference: the restatement is unpinned.  resolve() is arithmetic on Python scalars and needs no
device."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _abi as A
from .layers import BatchLayer

FIELDS = ("min_delay", "max_delay", "per_component")
LAST_ACTION_TERM = {"drift": 4, "elevation": 4, "visual": 3, "visual_depth": 3}     # the term's place in the batch's OBS_TERM_WIDTHS


@dataclass(frozen=True)
class LatencySpec:
    min_delay: int
    max_delay: int
    per_component: bool
    name: str             # the action term the latency belongs to


def _delay(v, term: str, what: str) -> int:
    if hasattr(v, "shape") and not isinstance(v, (np.integer, np.floating)):
        raise ValueError(f"action term '{term}': latency.{what} must be a Python integer, got {type(v).__name__} (tensor-valued parameters are not supported)")
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        if isinstance(v, (float, np.floating)) and float(v).is_integer():      # 2.0 from a command line is 2
            v = int(v)
        else:
            raise ValueError(f"action term '{term}': latency.{what} must be an integer number of control steps, got {v!r}")
    if v < 0:
        raise ValueError(f"action term '{term}': latency.{what} is {int(v)}: a delay cannot be negative")
    return int(v)


def resolve_term(name: str, latency) -> LatencySpec | None:
    """the `latency` of action term `name`: None, an ActionLatencyCfg or a dict of its fields -> the spec; None for no latency"""
    if latency is None:
        return None
    if isinstance(latency, dict):
        unknown = set(latency) - set(FIELDS)
        if unknown:
            raise ValueError(f"action term '{name}': latency has no field {sorted(unknown)}: one of {list(FIELDS)}")
        get = lambda k, d: latency.get(k, d)
    elif all(hasattr(latency, k) for k in FIELDS):
        get = lambda k, d: getattr(latency, k)
    else:
        raise ValueError(f"action term '{name}': latency must be an ActionLatencyCfg or a dict of {list(FIELDS)}, got {type(latency).__name__}")
    lo, hi = _delay(get("min_delay", 0), name, "min_delay"), _delay(get("max_delay", 0), name, "max_delay")
    per = get("per_component", False)
    if not isinstance(per, (bool, np.bool_)):
        raise ValueError(f"action term '{name}': latency.per_component must be a bool, got {per!r}")
    if lo > hi:
        raise ValueError(f"action term '{name}': latency.min_delay {lo} > max_delay {hi}")
    if hi > A.ACTLAT_MAX_DELAY:
        raise ValueError(f"action term '{name}': latency.max_delay {hi} is over the cap of {A.ACTLAT_MAX_DELAY} control steps")
    if hi == 0:
        return None
    return LatencySpec(lo, hi, bool(per), name)


def resolve(actions) -> LatencySpec | None:
    """actions: an actions config (cfg.actions) or [(name, ActionTermCfg)] -> the spec of its action term's latency; None without any
    (no `latency`, or min_delay = max_delay = 0)"""
    from .configclass import fields_of
    terms = actions if isinstance(actions, (list, tuple)) else ([] if actions is None else [(k, v) for k, v in fields_of(actions) if hasattr(v, "class_type")])
    specs = [s for s in (resolve_term(name, getattr(term, "latency", None)) for name, term in terms) if s is not None]
    return specs[0] if specs else None


class ActionLatency(BatchLayer):
    """the layer of one env batch: the block [5 + 2 (max_delay + 1), stride], the delayed actions `applied` [n, 2] and the two launches.
    push(action) before the step -> `applied`, what the step is launched on; finish(action, row, flags) after it."""

    def __init__(self, spec: LatencySpec, batch, last_action_col: int | None = None, task: str | None = None):
        import torch
        super().__init__(batch)
        self.spec = spec
        self.rows = int(self.lib.wl_action_latency_width(spec.max_delay))
        if self.rows < 0 or not 0 <= spec.min_delay <= spec.max_delay:
            raise ValueError(f"action latency: delays ({spec.min_delay}, {spec.max_delay}) are refused (at most {A.ACTLAT_MAX_DELAY} control steps)")
        if last_action_col is None:
            last_action_col = -1 if task is None else sum(batch.OBS_TERM_WIDTHS[:LAST_ACTION_TERM[task]])
        self.col = int(last_action_col)
        self.block = torch.zeros(self.rows, self.stride, dtype=torch.float32, device=self.device)       # (words: counters and action bits)
        self.applied = torch.zeros(self.n, 2, dtype=torch.float32, device=self.device)
        self._zero = torch.zeros(self.n, 2, dtype=torch.float32, device=self.device)

    def push(self, action):
        """the policy's action [n, 2] (fp32, contiguous; only read) into the ring -> the delayed action, the layer's own buffer"""
        a = self.batch._actions(action)
        A.check(self.lib.wl_action_latency_push(self.n, a.data_ptr(), self.applied.data_ptr(), self.block.data_ptr(), self.stride,
                                                self.spec.max_delay, A.stream(self.device)), "wl_action_latency_push")
        return self.applied

    def finish(self, action, row, terminated, time_outs=None):
        """after the step: the policy's action into the state's last-action rows and into `row`'s last_action columns (row: [n, D]
        contiguous, or None for the state rows alone); the envs the flags name forget their ring and draw their lags again"""
        import torch
        b = self.batch
        a = b._actions(action)
        assert terminated.dtype in (torch.bool, torch.uint8) and terminated.numel() == self.n and terminated.is_contiguous()
        assert time_outs is None or (time_outs.dtype in (torch.bool, torch.uint8) and time_outs.numel() == self.n and time_outs.is_contiguous())
        col = self.col if row is not None else -1
        if col >= 0:
            assert row.dtype == torch.float32 and row.dim() == 2 and row.shape[0] == self.n and row.is_contiguous()
        A.check(self.lib.wl_action_latency_finish(self.n, a.data_ptr(), b.state.data_ptr(), self.stride, None if col < 0 else row.data_ptr(),
                                                  int(row.shape[1]) if col >= 0 else 2, col, self.block.data_ptr(), terminated.data_ptr(),
                                                  None if time_outs is None else time_outs.data_ptr(), self.spec.min_delay, self.spec.max_delay,
                                                  int(self.spec.per_component), int(b.p.action.clip_wrapper), b.seed, b.env_offset,
                                                  A.stream(self.device)), "wl_action_latency_finish")

    def reset_all(self):
        """the env's first reset: every env resets -- the rings are forgotten, every lag is drawn again; no action is stored"""
        self.finish(self._zero, None, self.all)

    # ---- views for tests and logs
    @property
    def lags(self):
        """[n, 2] int32: the lag of each env's two action components, in control steps"""
        import torch
        return self.block[0:2, :self.n].view(torch.int32).T

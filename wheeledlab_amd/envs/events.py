"""Per-episode domain randomisation: the friction, actuator-gain and mass events of a config in mode "reset" or "interval"
(EventTermCfg.mode, managers_cfg.py) resolved into the term table of include/wheeledlab_amd_events.h, and the per-env block an env with
such terms owns.  Terms in mode "startup" stay the constructor's (flatten.py StartupSpec, wl_startup_randomize).

The layer is built only when a config asks for it; otherwise nothing is built, no path gains a launch and every output is what it was.
DESIGN.md section 21 states the semantics -- a restatement of IsaacLab's EventManager and mdp.events, which are not vendored with the
reference: the restatement is unpinned.  resolve() is arithmetic on Python scalars and needs no device."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .. import _abi as A
from .layers import BatchLayer

KINDS = ("wheel_friction", "actuator_gains", "base_mass")          # the wl_event markers of the three mdp functions
MODES = {"reset": A.ER_RESET, "interval": A.ER_INTERVAL}
OPERATIONS = {"add": A.ER_ADD, "scale": A.ER_SCALE, "abs": A.ER_ABS}
DISTRIBUTIONS = {"uniform": A.ER_UNIFORM, "log_uniform": A.ER_LOG_UNIFORM, "gaussian": A.ER_GAUSSIAN}
FIELDS = tuple(f for f, _ in A.WlEventRandTerm._fields_)


@dataclass(frozen=True)
class EventTable:
    terms: tuple          # per term the fields of WlEventRandTerm, in order: the table of wl_event_rand_apply
    names: tuple          # the config term each entry stands for

    @property
    def has_mass(self) -> bool:
        return any(t[0] in (A.ER_MASS_BASE, A.ER_MASS_WHEELS) for t in self.terms)


def _f32(v) -> float:
    return float(np.float32(v))


def _scalar(v, term: str, what: str) -> float:
    """a Python (or 0-dim numpy) number; tensors and sequences are refused"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"event term '{term}': {what} must be a Python scalar, got {type(v).__name__} (tensor-valued parameters are not supported)")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"event term '{term}': {what} is {v}")
    return v


def _pair(v, term: str, what: str):
    if isinstance(v, (str, bytes, dict)) or not hasattr(v, "__len__") or hasattr(v, "shape") or len(v) != 2:
        raise ValueError(f"event term '{term}': {what} must be a pair (lo, hi) of Python scalars, got {type(v).__name__} "
                         "(tensor-valued parameters are not supported)")
    return _scalar(v[0], term, f"{what}[0]"), _scalar(v[1], term, f"{what}[1]")


def _distribution(params, key: str, term: str, default_op: str):
    """-> (op, dist, p0, p1) of a mass / gain term"""
    op = params.get("operation", default_op)
    if op not in OPERATIONS:
        raise ValueError(f"event term '{term}': operation is {op!r}: one of {sorted(OPERATIONS)}")
    dist = params.get("distribution", "uniform")
    if dist not in DISTRIBUTIONS:
        raise ValueError(f"event term '{term}': distribution is {dist!r}: one of {sorted(DISTRIBUTIONS)}")
    p0, p1 = _pair(params.get(key), term, key)
    if dist == "gaussian":
        if p1 < 0:
            raise ValueError(f"event term '{term}': {key} std {p1} < 0")
    elif p0 > p1:
        raise ValueError(f"event term '{term}': {key} {p0} > {p1}")
    if dist == "log_uniform" and p0 <= 0:
        raise ValueError(f"event term '{term}': {key} {p0} <= 0 under log_uniform")
    return OPERATIONS[op], DISTRIBUTIONS[dist], _f32(p0), _f32(p1)


def is_episodic(term) -> bool:
    """a friction / gain / mass term that runs per episode, not once at construction"""
    return getattr(term.func, "wl_event", None) in KINDS and getattr(term, "mode", None) in MODES


def is_wheel_mass(params) -> bool:
    return "wheel" in str(getattr(params.get("asset_cfg"), "body_names", ""))


def term_row(name: str, term, startup_spec, mode: str | None = None) -> tuple:
    """one config term -> the fields of its WlEventRandTerm; `mode` overrides term.mode (direct calls)"""
    kind = getattr(term.func, "wl_event", None)
    if kind not in KINDS:
        raise ValueError(f"event term '{name}': {getattr(term.func, '__name__', term.func)} is not a friction, actuator-gain or mass randomisation")
    mode = getattr(term, "mode", None) if mode is None else mode
    if mode not in MODES:
        raise ValueError(f"event term '{name}': mode is {mode!r}: one of {sorted(MODES)}")
    pr = dict(term.params or {})
    lo_s = hi_s = 0.0
    if mode == "interval":
        if getattr(term, "interval_range_s", None) is None:
            raise ValueError(f"event term '{name}': mode interval needs interval_range_s")
        lo_s, hi_s = _pair(term.interval_range_s, name, "interval_range_s")
        if lo_s > hi_s or lo_s <= 0:
            raise ValueError(f"event term '{name}': interval_range_s ({lo_s}, {hi_s}) must satisfy 0 < lo <= hi")
    min_steps = getattr(term, "min_step_count_between_reset", 0) or 0
    if isinstance(min_steps, bool) or not isinstance(min_steps, (int, np.integer)) or min_steps < 0:
        raise ValueError(f"event term '{name}': min_step_count_between_reset must be an integer >= 0, got {min_steps!r}")
    row = dict(target=A.ER_MU, mode=MODES[mode], op=A.ER_ABS, dist=A.ER_UNIFORM, p0=0.0, p1=0.0, base=0.0, interval_lo=_f32(lo_s), interval_hi=_f32(hi_s),
               is_global_time=int(bool(getattr(term, "is_global_time", False))), min_step_count_between_reset=int(min_steps), mu_s_lo=0.0, mu_s_hi=0.0,
               mu_d_lo=0.0, mu_d_hi=0.0, num_buckets=1, make_consistent=0)
    if kind == "wheel_friction":
        rest = _pair(pr.get("restitution_range", (0.0, 0.0)), name, "restitution_range")
        if rest != (0.0, 0.0):
            raise ValueError(f"event term '{name}': restitution_range {rest} is not (0, 0): restitution is not modelled")
        s, d = _pair(pr.get("static_friction_range"), name, "static_friction_range"), _pair(pr.get("dynamic_friction_range"), name, "dynamic_friction_range")
        if s[0] > s[1] or d[0] > d[1]:
            raise ValueError(f"event term '{name}': a friction range with lo > hi ({s}, {d})")
        nb = pr.get("num_buckets")
        if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or nb < 1:
            raise ValueError(f"event term '{name}': num_buckets must be an integer >= 1, got {nb!r}")
        row.update(mu_s_lo=_f32(s[0]), mu_s_hi=_f32(s[1]), mu_d_lo=_f32(d[0]), mu_d_hi=_f32(d[1]), num_buckets=int(nb),
                   make_consistent=int(bool(pr.get("make_consistent", False))))
    elif kind == "actuator_gains":
        stiff = pr.get("stiffness_distribution_params")
        if stiff is not None:
            k = float(getattr(startup_spec, "throttle_stiffness", 0.0))
            if _pair(stiff, name, "stiffness_distribution_params") != (k, k):
                raise ValueError(f"event term '{name}': stiffness_distribution_params {tuple(stiff)} is not the asset's value ({k}, {k}): the "
                                 "throttle stiffness is not modelled")
        if pr.get("damping_distribution_params") is None:
            raise ValueError(f"event term '{name}': damping_distribution_params is not set")
        op, dist, p0, p1 = _distribution(pr, "damping_distribution_params", name, "abs")
        row.update(target=A.ER_DAMP, op=op, dist=dist, p0=p0, p1=p1, base=_f32(getattr(startup_spec, "throttle_damping", startup_spec.damping[0])))
    else:
        op, dist, p0, p1 = _distribution(pr, "mass_distribution_params", name, "add")
        if is_wheel_mass(pr):
            if op != A.ER_ABS:
                raise ValueError(f"event term '{name}': randomize_rigid_body_mass on the wheel links: operation abs (the link masses add up)")
            row.update(target=A.ER_MASS_WHEELS, op=op, dist=dist, p0=p0, p1=p1)
        else:
            row.update(target=A.ER_MASS_BASE, op=op, dist=dist, p0=p0, p1=p1, base=_f32(startup_spec.chassis_mass))
    return tuple(row[f] for f in FIELDS)


def resolve(events, startup_spec, task: str = "drift") -> EventTable | None:
    """events: an events config (cfg.events) or [(name, EventTermCfg)]; startup_spec: flatten.StartupSpec (the chassis mass, the asset's
    throttle damping and stiffness); task: for messages.  -> the table of the terms in mode "reset" / "interval" whose func is one of
    the three randomisations, in config order; None without any.  Every other term is left to the caller."""
    from .configclass import fields_of
    terms = events if isinstance(events, (list, tuple)) else ([] if events is None else [(k, v) for k, v in fields_of(events) if hasattr(v, "func")])
    rows, names = [], []
    for name, term in terms:
        if not is_episodic(term):
            continue
        rows.append(term_row(name, term, startup_spec))
        names.append(name)
    if not rows:
        return None
    if len(rows) > A.EVENTRAND_MAX_TERMS:
        raise ValueError(f"{task}: {len(rows)} reset / interval randomisation terms ({', '.join(names)}): at most {A.EVENTRAND_MAX_TERMS}")
    return EventTable(tuple(rows), tuple(names))


class EventRandomizer(BatchLayer):
    """the layer of one env batch: the table, the block [2 + 4 K, stride] and the launch.  An empty table (K = 0) launches nothing; it
    serves direct calls of the mdp functions (apply_ids), which bring their own one-term table."""

    def __init__(self, table: EventTable | None, batch, startup_spec, step_dt: float):
        import torch
        super().__init__(batch)                                                     # (self.all: env.reset(), apply_all())
        self.table = table if table is not None else EventTable((), ())
        self.startup, self.step_dt = startup_spec, float(np.float32(step_dt))
        self.K = len(self.table.terms)
        self.ctable = self._ctable(self.table.terms)
        if self.K and self.lib.wl_event_rand_width(self.ctable, self.K) != 2 + 4 * self.K:
            raise ValueError(f"event randomisation: the term table {self.table.terms} is refused")
        self.block = torch.zeros(2 + 4 * self.K, self.stride, dtype=torch.float32, device=self.device)
        self.none = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self._mask = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self._direct = {}           # a direct call's row -> its own block (its counters go on from call to call)
        self._parts_ready = False
        if self.table.has_mass:
            self.init_parts()
        if self.K:                  # the first time_left of every interval term: no flag, no time
            self._launch(self.ctable, self.K, self.block, self.none, None, None, 0, 0.0)

    @staticmethod
    def _ctable(rows):
        return (A.WlEventRandTerm * max(len(rows), 1))(*[A.WlEventRandTerm(*r) for r in rows])

    def init_parts(self):
        """part_base and part_wheels of the mass row the startup wrote: wl_startup_randomize into a scratch state twice, once with the
        wheel range zeroed and once with the chassis and the base range zeroed.  The draws are keyed by env id and seed alone, so they
        are the startup's own, and the two rows sum bit for bit to its mass row."""
        import torch
        from dataclasses import replace
        from ..core import apply_startup_events
        b = self.batch
        scratch = torch.zeros(A.S_COUNT, self.stride, dtype=torch.float32, device=self.device)
        bufs = A.WlEnvBuffers(scratch.data_ptr(), None, None, None, self.stride, self.n, b.env_offset, 1, 0, 0)
        for row, su in ((0, replace(self.startup, wheel_mass=(0.0, 0.0))), (1, replace(self.startup, chassis_mass=0.0, mass_add=(0.0, 0.0)))):
            apply_startup_events(self.lib, bufs, su, b.seed, A.stream(self.device))
            self.block[row].copy_(scratch[A.S_MASS])
        self._parts_ready = True

    def _launch(self, ctable, K, block, reset_a, reset_b, mask, mask_terms, dt, step=None):
        b = self.batch
        A.check(self.lib.wl_event_rand_apply(self.n, b.state.data_ptr(), self.stride, ctable, K, block.data_ptr(), reset_a.data_ptr(),
                                             None if reset_b is None else reset_b.data_ptr(), None if mask is None else mask.data_ptr(), mask_terms,
                                             b.seed, b.step_count if step is None else int(step), dt, b.env_offset, A.stream(self.device)),
                "wl_event_rand_apply")

    def apply(self, terminated, time_outs=None, dt=None):
        """one launch after a step: the flags the step returned (byte tensors [n]); dt None: the env's step"""
        import torch
        if not self.K:
            return
        assert terminated.dtype in (torch.bool, torch.uint8) and terminated.numel() == self.n and terminated.is_contiguous()
        assert time_outs is None or (time_outs.dtype in (torch.bool, torch.uint8) and time_outs.numel() == self.n and time_outs.is_contiguous())
        self._launch(self.ctable, self.K, self.block, terminated, time_outs, None, 0, self.step_dt if dt is None else float(dt))

    def reset_all(self):
        """the env's first reset: every env resets, no time passes (reset terms are applied, per-env timers drawn again)"""
        self.apply(self.all, None, dt=0.0)

    def apply_all(self):
        """every term to every env, now; no time passes"""
        if self.K:
            self._launch(self.ctable, self.K, self.block, self.none, None, self.all, (1 << self.K) - 1, 0.0)

    def _ids_mask(self, env_ids):
        self._mask.zero_()
        if env_ids is None or isinstance(env_ids, slice):
            self._mask[env_ids if isinstance(env_ids, slice) else slice(None)] = 1
        else:
            self._mask[env_ids] = 1
        return self._mask

    def apply_ids(self, term, env_ids):
        """one term to the envs `env_ids` (indices, a slice or None for all), now: `term` the index or name of a table term, or the row
        of a term that is not in the table (mdp.* called directly, term_row()) -- that one keeps counters of its own"""
        mask = self._ids_mask(env_ids)
        if isinstance(term, str):
            term = self.table.names.index(term)
        if isinstance(term, (int, np.integer)):
            self._launch(self.ctable, self.K, self.block, self.none, None, mask, 1 << int(term), 0.0)
            return
        import torch
        row = tuple(term)
        mass = row[0] in (A.ER_MASS_BASE, A.ER_MASS_WHEELS)
        if mass and not self._parts_ready:
            self.init_parts()
        blk = self._direct.get(row)
        if blk is None:
            blk = self._direct[row] = torch.zeros(6, self.stride, dtype=torch.float32, device=self.device)
        ct = self._ctable([row])
        if self.lib.wl_event_rand_width(ct, 1) != 6:
            raise ValueError(f"event randomisation: the term {dict(zip(FIELDS, row))} is refused")
        if mass:                    # the env's parts travel through the call's own block
            blk[0:2].copy_(self.block[0:2])
        self._launch(ct, 1, blk, self.none, None, mask, 1, 0.0)
        if mass:
            self.block[0:2].copy_(blk[0:2])

    # ---- views for tests and logs
    @property
    def part_base(self):
        return self.block[0, :self.n]

    @property
    def part_wheels(self):
        return self.block[1, :self.n]

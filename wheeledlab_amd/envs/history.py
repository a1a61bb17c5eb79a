"""Observation history: `history_length` / `flatten_history_dim` of an observation group and its terms (managers_cfg.py) resolved
into the term table of include/wheeledlab_amd_history.h, and the pair of stacked-row buffers an env with history owns.

The semantics are IsaacLab's as documented (a per-env circular buffer per term that its first push after a reset fills with that
frame); DESIGN.md section 19 states them.  resolve() is integer arithmetic on widths and needs no device."""
from __future__ import annotations

from dataclasses import dataclass

from .. import _abi as A


@dataclass(frozen=True)
class HistoryLayout:
    terms: tuple          # ((src_off, width, frames, dst_off), ...): the table of wl_obs_history_push
    names: tuple          # the term each table entry stands for
    D: int                # raw row
    Dh: int               # stacked row
    frames: int           # time-major layout: H of the [N, H, D] view; 0: the flat term-major row

    @property
    def shape(self):
        """the per-env shape of obs["policy"]"""
        return (self.frames, self.D) if self.frames else (self.Dh,)


def _frames(value, name) -> int:
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"history_length of '{name}' must be an int, got {value!r}")
    if value < 0 or value > A.OBSHIST_MAX_FRAMES:
        raise ValueError(f"history_length of '{name}' is {value}: outside 0 .. {A.OBSHIST_MAX_FRAMES}")
    return max(1, value)


def table(widths, frames):
    """the term table of per-term widths and frame counts (each >= 1), the terms back to back in both rows"""
    out, src, dst = [], 0, 0
    for w, h in zip(widths, frames):
        out.append((src, int(w), int(h), dst))
        src += int(w)
        dst += int(w) * int(h)
    return tuple(out), src, dst


def resolve(group, terms, widths, group_name: str = "policy") -> HistoryLayout | None:
    """group: an ObservationGroupCfg; terms: [(name, ObservationTermCfg)] in the order of the raw row -- the fused terms in layout
    order, then the plugin terms; widths: the columns of each.  -> the layout, or None when every term keeps one frame (no history:
    the env builds nothing)."""
    if len(terms) != len(widths):
        raise ValueError(f"{len(terms)} observation terms but {len(widths)} widths")
    g = getattr(group, "history_length", None)
    if g is not None:
        h = _frames(g, group_name)
        if h == 1:
            return None
        if not getattr(group, "flatten_history_dim", True):      # one pseudo-term covering the row: [H][D], oldest first
            D = sum(int(w) for w in widths)
            t, _, Dh = table([D], [h])
            return HistoryLayout(t, (group_name,), D, Dh, h)
        frames = [h] * len(terms)
    else:
        frames = []
        for name, term in terms:
            frames.append(_frames(getattr(term, "history_length", 0), name))
            if not getattr(term, "flatten_history_dim", True) and getattr(group, "concatenate_terms", True):
                raise ValueError(f"flatten_history_dim=False on term '{name}' of a group with concatenate_terms=True: a [N, H, w] term does "
                                 f"not concatenate with its neighbours (set history_length and flatten_history_dim=False on the group)")
        if all(h == 1 for h in frames):
            return None
    if len(terms) > A.OBSHIST_MAX_TERMS:
        raise ValueError(f"observation history over {len(terms)} terms: at most {A.OBSHIST_MAX_TERMS}")
    t, D, Dh = table(widths, frames)
    return HistoryLayout(t, tuple(n for n, _ in terms), D, Dh, 0)


class ObsHistory:
    """the stacked rows [n, Dh] of an env with history: two buffers that alternate (the push reads one and writes the other), and the
    launch into a caller's rows (the runner's storage: row k -> row k + 1)"""

    def __init__(self, layout: HistoryLayout, n_envs: int, device):
        import torch
        self.layout, self.n, self.device = layout, int(n_envs), torch.device(device)
        self.lib = A.load()
        self.table = (A.WlObsHistoryTerm * len(layout.terms))(*[A.WlObsHistoryTerm(*t) for t in layout.terms])
        if self.lib.wl_obs_history_width(self.table, len(layout.terms), layout.D) != layout.Dh:
            raise ValueError(f"observation history: the term table {layout.terms} is not one of raw rows of {layout.D}")
        self.bufs = [torch.zeros(self.n, layout.Dh, dtype=torch.float32, device=self.device) for _ in range(2)]
        self.cur = 0
        self.filled = False

    def view(self, rows):
        return rows.view(self.n, *self.layout.shape)

    def current(self):
        return self.view(self.bufs[self.cur])

    def push_into(self, raw, prev, nxt, reset_a, reset_b=None):
        """one launch: nxt = the push of the raw rows onto prev (None: every env fresh)"""
        import torch
        L = self.layout
        assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.shape == (self.n, L.D) and raw.stride(1) == 1, (raw.shape, raw.stride())
        assert nxt.is_contiguous() and nxt.numel() == self.n * L.Dh and (prev is None or (prev.is_contiguous() and prev.numel() == nxt.numel()))
        assert reset_a.dtype in (torch.bool, torch.uint8) and reset_a.numel() == self.n
        A.check(self.lib.wl_obs_history_push(self.n, L.D, raw.data_ptr(), raw.stride(0), self.table, len(L.terms),
                                             None if prev is None else prev.data_ptr(), nxt.data_ptr(), reset_a.data_ptr(),
                                             None if reset_b is None else reset_b.data_ptr(), A.stream(self.device)),
                "wl_obs_history_push")

    def push(self, raw, reset_a, reset_b=None, fresh: bool = False):
        """advance the env's own rows by one frame -> the new stacked observation (a view of the buffer now current)"""
        nxt = self.bufs[1 - self.cur]
        self.push_into(raw, None if fresh else self.bufs[self.cur], nxt, reset_a, reset_b)
        self.cur, self.filled = 1 - self.cur, True
        return self.view(nxt)

    def adopt(self, rows):
        """the env's rows catch up with a collector that pushed inside its own storage"""
        self.bufs[self.cur].copy_(rows.reshape(self.n, self.layout.Dh))
        self.filled = True
        return self.current()

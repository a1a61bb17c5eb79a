"""The between-step layers of an env, composed: the ONE place their order is written.

    delayed(action) -> the step launch -> after(...): events -> latency finish -> corruption -> history

StepLayers is handed ready-made layer objects (events.py, latency.py, corruption.py, history.py -- or stand-ins with their methods), each
None when the config does not ask for it, and holds no buffer of its own.  Straight-line code on purpose: env.step() is bound by what
the host enqueues -- which is also why the layers assert their flag tensors inline: a shared check function took env.step() with one
layer out of the range it had.  Also here: what every layer bound to an env batch starts from (BatchLayer)."""
from __future__ import annotations

from .. import _abi as A

# why the collectors that run more than one env step per launch refuse, by layer, in the order they are asked
REFUSALS = (("history", "observation history is pushed between steps"),
            ("corruption", "observation corruption runs between steps"),
            ("events", "reset / interval event randomisation runs between steps"),
            ("latency", "action latency delays actions between steps"))


class BatchLayer:
    """what a layer bound to an env batch starts from; `all`: every reset flag set, what env.reset() hands the layer"""

    def __init__(self, batch):
        import torch
        self.batch, self.lib = batch, A.load()
        self.n, self.stride, self.device = int(batch.n), int(batch.stride), batch.state.device
        self.all = torch.ones(self.n, dtype=torch.uint8, device=self.device)


class StepLayers:
    __slots__ = ("events", "latency", "corruption", "history", "rewrites_obs")

    def __init__(self, events=None, latency=None, corruption=None, history=None):
        self.events, self.latency, self.corruption, self.history = events, latency, corruption, history
        # collect_step()'s one question: will a layer rewrite the row the step wrote?  (then the step lands it in the batch's own buffer)
        self.rewrites_obs = corruption is not None or history is not None

    def delayed(self, action):
        """before the step: the action it is launched on (with latency the ring's; the policy's goes to after())"""
        return action if self.latency is None else self.latency.push(action)

    def after(self, action, raw, terminated, truncated, prev=None, out=None):
        """after the step, which wrote the row `raw` and the flags -> the observation.  The envs the step reset get their episode's
        constants; last_action becomes the policy's action, in the state and in `raw`, before the corruption reads the state; the
        history stacks the corrupted row.  out None (step()): the env's own row -- the last layer's buffer, or `raw`.  out given
        (collect_step()): the last layer that rewrites the row writes `out`, the history pushing from the stacked row `prev`; when
        nothing rewrites it `raw` is the caller's row already."""
        if self.events is not None:
            self.events.apply(terminated, truncated)
        if self.latency is not None:
            self.latency.finish(action, raw, terminated, truncated)
        c, h = self.corruption, self.history
        if c is not None:
            if h is None and out is not None:
                return c.apply(raw, out, terminated, truncated)
            raw = c.corrupt(raw, terminated, truncated)
        if h is not None:
            if out is None:
                return h.push(raw, terminated, truncated)
            h.push_into(raw, prev, out, terminated, truncated)
            return out
        return raw

    def reset(self, raw_fn, flags):
        """env.reset(), after the batch's own: the reset-mode events on every env, its timers drawn again; every ring forgotten, every
        lag drawn; then the raw row (raw_fn()) with every env's bias drawn; every frame of the history the reset frame (flags: any flag
        tensor of the batch -- a fresh push reads none, but its entry point takes no NULL)"""
        if self.events is not None:
            self.events.reset_all()
        if self.latency is not None:
            self.latency.reset_all()
        raw = raw_fn()
        if self.corruption is not None:
            raw = self.corruption.corrupt(raw, self.corruption.all)
        if self.history is not None:
            raw = self.history.push(raw, flags, fresh=True)
        return raw

    def current(self, raw_fn, flags):
        """the observation as it stands: reading draws and pushes nothing new -- with corruption or history it is the row of the last
        step (before the first reset: the current state's, every reset flag set and every frame the current one)"""
        c, h = self.corruption, self.history
        if h is not None and h.filled:
            return h.current()
        if c is None:
            row = raw_fn()
        else:
            row = c.row if c.filled else c.corrupt(raw_fn(), c.all)
        return row if h is None else h.push(row, flags, fresh=True)

    def adopt(self, rows):
        """after a collection into the caller's storage: the layer that keeps the env's row catches up with `rows`, the last of them;
        None: no layer keeps one (the batch's own row is the env's)"""
        keeper = self.history if self.history is not None else self.corruption
        return None if keeper is None else keeper.adopt(rows)

    def fused_refusal(self):
        """why a collector that runs several env steps in one launch cannot run: the first layer present, or None"""
        for name, why in REFUSALS:
            if getattr(self, name) is not None:
                return f"{why}; use step() or collect_step()"
        return None

"""Empirical observation normalisation: running per-feature moments of the observations, and the normalisation folded into the
first-layer weights the fused collectors read.

`EmpiricalNormalization` is rsl_rl.modules.EmpiricalNormalization's work-alike (2.x; rsl-rl-lib is not vendored, the definition is
restated from memory, and for the tests in tests/obs_norm_reference.py; parity with rsl_rl itself is unpinned): buffers `_mean`, `_var`, `_std` [1, D] and `count`
under rsl_rl's state-dict keys, eps 1e-2, `until` 10^8 samples, output (x - mean) / (std + eps), the pooled-moments update.

What differs, by design: the fused collectors run a whole rollout as one launch and hold the actor's first layer in registers (or as
bf16 planes), so nothing can be merged per step.  The runner keeps the statistics FROZEN during a rollout and merges the K x n raw
observation rows 0 .. K - 1 of the storage once per iteration (`merge_rollout`: the merge is associative, so after every iteration the
statistics are rsl_rl's after the same steps; inside a rollout they lag by at most K steps).  Collection never sees a normalised
observation: it reads raw observations through first layers with the normalisation folded in (`fold`: W' = W diag(inv_std),
b' = b - W' mean).  The learner reads the storage rows normalised in place with the same frozen statistics, through the unfolded
parameters.

On a GPU the merge is csrc/wl_obs_norm.hip (one pass over the rows: normalise in place + float64 moments, a fixed-order sum, the
float64 merge on the device); on the CPU everything here is plain torch in float64."""
from __future__ import annotations

import torch
from torch import nn

RATIO_WARN = 1000.0   # max |mean| inv_std above which the folded first layer cancels visibly


class EmpiricalNormalization(nn.Module):
    def __init__(self, shape, eps: float = 1e-2, until: int | None = 10 ** 8):
        super().__init__()
        D = int(shape[-1] if isinstance(shape, (tuple, list, torch.Size)) else shape)
        self.dim, self.eps, self.until = D, float(eps), int(until) if until is not None else None
        self.register_buffer("_mean", torch.zeros(1, D))
        self.register_buffer("_var", torch.ones(1, D))
        self.register_buffer("_std", torch.ones(1, D))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))
        # 1 / (std + eps): what the kernels multiply by; derived, so not part of the state dict
        self.register_buffer("_inv_std", torch.full((1, D), 1.0 / (1.0 + self.eps)), persistent=False)
        self._scratch = None

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return self._std.squeeze(0).clone()

    # ---- torch path ------------------------------------------------------------------------------------------------------
    def normalize(self, x):
        """(x - mean) / (std + eps) with the statistics as they stand (no update)"""
        return (x - self._mean) / (self._std + self.eps)

    def forward(self, x):
        """rsl_rl's forward: in training mode the rows of x update the statistics first; eval() stops the updates"""
        if self.training:
            self.update(x)
        return self.normalize(x)

    def inverse(self, y):
        return y * (self._std + self.eps) + self._mean

    @torch.no_grad()
    def _sums(self, x):
        """float64 [2, D]: sum (x - mean), sum (x - mean)^2 over the rows of x, about the mean as it stands"""
        d = x.reshape(-1, self.dim).double() - self._mean.double()
        return torch.stack([d.sum(0), (d * d).sum(0)])

    @torch.no_grad()
    def _merge(self, sums, m: int):
        """the pooled-moments merge of m rows in float64 (csrc/wl_obs_norm_dev.h::obsnorm_merge), each result rounded once"""
        if self.until is not None and int(self.count) >= self.until:
            return
        now = int(self.count) + m
        rate = m / now
        d = sums[0] / m
        vb = (sums[1] / m - d * d).clamp_min(0.0)
        mean, var = self._mean.double().squeeze(0), self._var.double().squeeze(0)
        mean_new = mean + rate * d
        var_new = var + rate * (vb - var + d * (d - rate * d))
        self._mean.copy_(mean_new.float()[None])
        self._var.copy_(var_new.float()[None])
        self._derive()
        self.count.fill_(now)

    @torch.no_grad()
    def _derive(self):
        """std and inv_std = 1 / (std + eps) from the ROUNDED variance, in float64, each rounded once: a state restored from a
        checkpoint has the bits of the one that was saved"""
        sd = self._var.double().sqrt()
        self._std.copy_(sd.float())
        self._inv_std.copy_((1.0 / (sd + self.eps)).float())

    @torch.no_grad()
    def update(self, x):
        x = x.reshape(-1, self.dim)
        self._merge(self._sums(x), x.shape[0])

    def load_state_dict(self, state_dict, *a, **kw):
        out = super().load_state_dict(state_dict, *a, **kw)
        std = self._std.clone()
        self._derive()
        self._std.copy_(std)        # the checkpoint's own std stays (ours equals the derived one to the bit)
        return out

    # ---- the runner's per-iteration merge --------------------------------------------------------------------------------
    def max_ratio(self) -> float:
        """max_c |mean_c| inv_std_c: how far the folded first layer has to cancel (one device -> host copy)"""
        return float((self._mean.abs() * self._inv_std).max())

    @torch.no_grad()
    def merge_rollout(self, storage, world: int = 1) -> float:
        """rows 0 .. K - 1 of storage.observations become normalised IN PLACE with the statistics as they stand (the ones the
        collection ran with), then the statistics advance by those K x n (x world) raw rows: one all-reduce of the [2, D] float64
        sums when world > 1, so every rank ends with bit-identical statistics.  Row K (the next rollout's row 0) stays raw and is
        counted with the next rollout.  Returns max_ratio() of the new statistics."""
        K, n = storage.n_steps, storage.n_envs
        x = storage.observations[:K].view(K * n, self.dim)
        if x.is_cuda:
            sums = self._accumulate(x, x)
        else:
            sums = self._sums(x)
            x.copy_(self.normalize(x))
        if world > 1:
            torch.distributed.all_reduce(sums, op=torch.distributed.ReduceOp.SUM)
        if x.is_cuda:
            from .. import _abi as A
            A.check(A.load().wl_obsnorm_update(self.dim, sums.data_ptr(), K * n * world, self.until if self.until is not None else 2 ** 62,
                                               self.eps, self._mean.data_ptr(), self._var.data_ptr(), self._std.data_ptr(),
                                               self._inv_std.data_ptr(), self.count.data_ptr(), A.stream(x.device)), "wl_obsnorm_update")
        else:
            self._merge(sums, K * n * world)
        return self.max_ratio()

    def _accumulate(self, x, out=None):
        """wl_obsnorm_accumulate over the rows of x (a [rows, D] float32 view with unit column stride): -> float64 [2, D] sums about
        the frozen mean; out (x itself: in place) receives the normalised rows"""
        from .. import _abi as A
        lib = A.load()
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.dim and x.stride(1) == 1 and self._mean.is_contiguous()
        assert out is None or (out.shape == x.shape and out.stride() == x.stride() and out.dtype == torch.float32)
        total = None
        for r0 in range(0, x.shape[0], A.OBSNORM_MAX_ROWS):     # a float64 sum of at most 2^23 terms per call
            xs = x[r0:r0 + A.OBSNORM_MAX_ROWS]
            rows, stride = xs.shape[0], xs.stride(0)
            need = int(lib.wl_obsnorm_scratch_bytes(rows, self.dim, stride))
            if need < 0:
                A.check(need, "wl_obsnorm_scratch_bytes")
            if self._scratch is None or self._scratch.numel() * 8 < need or self._scratch.device != x.device:
                self._scratch = torch.empty(need // 8, dtype=torch.float64, device=x.device)
            sums = torch.empty(2, self.dim, dtype=torch.float64, device=x.device)
            A.check(lib.wl_obsnorm_accumulate(rows, self.dim, xs.data_ptr(), stride, self._mean.data_ptr(), self._inv_std.data_ptr(),
                                              None if out is None else out[r0:r0 + rows].data_ptr(), self._scratch.data_ptr(),
                                              sums.data_ptr(), A.stream(x.device)), "wl_obsnorm_accumulate")
            total = sums if total is None else total + sums
        return total

    # ---- the folded first layers -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def fold(self, actor_critic):
        """refresh the folded first-layer tensors of actor_critic.folded_view() from the current parameters and statistics; they
        are written in place, so whatever holds their pointers reads the new values at its next launch"""
        view = actor_critic.folded_view()
        for m, seq in ((view.actor, actor_critic.actor), (view.critic, actor_critic.critic)):
            lin = seq[0]
            w, b = lin.weight.detach(), lin.bias.detach()
            if w.is_cuda:
                from .. import _abi as A
                assert w.is_contiguous() and m.w1.is_contiguous() and m.w1.data_ptr() != w.data_ptr()
                A.check(A.load().wl_obsnorm_fold(self.dim, w.shape[0], w.data_ptr(), b.data_ptr(), self._mean.data_ptr(),
                                                 self._inv_std.data_ptr(), m.w1.data_ptr(), m.b1.data_ptr(), A.stream(w.device)),
                        "wl_obsnorm_fold")
            else:
                mean, inv = self._mean.double().squeeze(0), self._inv_std.double().squeeze(0)
                m.w1.copy_(w * self._inv_std)
                m.b1.copy_((b.double() - (w.double() * (mean * inv)).sum(1)).float())
        return view

"""The contract of the observation-history push (include/wheeledlab_amd_history.h) stated twice, independently, on 32-bit words:

  push_closed   the closed-form index map: for every column of the stacked row, the column of the raw row or of the previous stacked
                row it is a copy of, as numpy index arrays;
  DequeModel    the literal model: per env and term a collections.deque(maxlen=H) that a reset clears and whose first push fills
                it H times.

tests/test_obs_history_cpu.py holds the two against each other; the host simulation, the kernel and the env are held to them.
Everything is uint32: the operation copies floats, so every comparison is byte for byte and the inputs carry NaNs of distinct
payloads, -0.0, infinities and denormals (special_words)."""
from collections import deque

import numpy as np

MAX_TERMS, MAX_FRAMES = 64, 64


def table(widths, frames):
    """[(src_off, width, frames, dst_off)] of terms back to back -> (table [T, 4] int32, D, Dh)"""
    out, src, dst = [], 0, 0
    for w, h in zip(widths, frames):
        out.append((src, w, h, dst))
        src, dst = src + w, dst + w * h
    return np.asarray(out, np.int32).reshape(-1, 4), src, dst


# the tables of the GPU test (tests/test_gpu_obs_history.py) and of the host simulation: name -> (widths, frames)
TABLES = {
    "identity": ([1], [1]),
    "w3h2": ([3], [2]),
    "drift_h3": ([3, 3, 3, 3, 2], [3] * 5),
    "mixed": ([3, 3, 3, 3, 2], [1, 3, 5, 1, 3]),
    "elevation": ([2, 3, 3, 3, 2, 676], [1, 1, 1, 1, 1, 2]),
    "time_major": ([14], [4]),
}


def special_words(rng, shape):
    """uint32 words of random finite floats with, scattered among them, quiet and signalling NaNs of distinct payloads (both signs),
    -0.0, +0.0, both infinities and denormals"""
    x = rng.standard_normal(shape).astype(np.float32).view(np.uint32).copy()
    flat = x.reshape(-1)
    k = max(1, flat.size // 4)
    idx = rng.choice(flat.size, size=k, replace=False)
    kinds = rng.integers(0, 6, size=k)
    payload = (rng.integers(1, 1 << 22, size=k, dtype=np.int64)).astype(np.uint32)
    sign = (rng.integers(0, 2, size=k, dtype=np.int64).astype(np.uint32)) << np.uint32(31)
    vals = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4],
                     [np.uint32(0x7FC00000) | payload | sign,          # quiet NaN, payload
                      np.uint32(0x7F800000) | payload | sign,          # signalling NaN, payload (non-zero mantissa, quiet bit clear)
                      np.uint32(0x80000000) * (payload & np.uint32(1)),   # -0.0 / +0.0
                      np.uint32(0x7F800000) | sign,                    # +-inf
                      (payload & np.uint32(0x007FFFFF)) | sign],       # denormal
                     default=flat[idx]).astype(np.uint32)
    flat[idx] = vals
    return x


def push_closed(tab, obs, prev, reset):
    """tab [T, 4]; obs uint32 [n, >= D] (the first D columns are the raw row); prev uint32 [n, Dh] or None; reset bool [n] ->
    next uint32 [n, Dh]"""
    tab = np.asarray(tab, np.int64).reshape(-1, 4)
    Dh = int((tab[:, 1] * tab[:, 2]).sum())
    col = np.arange(Dh)
    k = np.searchsorted(tab[:, 3], col, side="right") - 1              # the term of every stacked column
    s, w, h, d = tab[k, 0], tab[k, 1], tab[k, 2], tab[k, 3]
    frame, i = (col - d) // w, (col - d) % w
    from_obs = s + i                                                    # the raw column a fresh env copies
    newest = frame == h - 1
    from_prev = np.where(newest, 0, col + w)                            # frame f of the new row is frame f + 1 of the old
    fresh = np.ones(obs.shape[0], bool) if prev is None else np.asarray(reset, bool)
    out = obs[:, from_obs].copy()
    if prev is not None:
        shifted = np.where(newest[None, :], obs[:, from_obs], prev[:, from_prev])
        out = np.where(fresh[:, None], out, shifted)
    return out.astype(np.uint32)


class DequeModel:
    """per env and term a deque(maxlen=H): cleared by a reset, filled H times by its first push"""

    def __init__(self, tab, n):
        self.tab = [tuple(int(v) for v in t) for t in np.asarray(tab).reshape(-1, 4)]
        self.q = [[deque(maxlen=h) for (_, _, h, _) in self.tab] for _ in range(n)]

    def push(self, obs, reset):
        rows = []
        for e, per_term in enumerate(self.q):
            row = []
            for (s, w, h, _), q in zip(self.tab, per_term):
                if reset[e]:
                    q.clear()
                frame = [int(v) for v in obs[e, s:s + w]]
                if not q:
                    for _ in range(h):
                        q.append(frame)
                else:
                    q.append(frame)
                for f in q:             # oldest first
                    row.extend(f)
            rows.append(row)
        return np.asarray(rows, np.uint32)


def time_major(rows, H, D):
    """the [n, H, D] view of the pseudo-term layout"""
    return rows.reshape(rows.shape[0], H, D)


def run(tab, obs_steps, reset_steps):
    """the stacked rows after each step of a run that starts with no history: obs_steps [K, n, D] uint32, reset_steps [K, n] bool
    (reset_steps[k] belongs to the step that produced obs_steps[k]) -> [K, n, Dh]"""
    prev, out = None, []
    for o, r in zip(obs_steps, reset_steps):
        prev = push_closed(tab, o, prev, r)
        out.append(prev)
    return np.stack(out)

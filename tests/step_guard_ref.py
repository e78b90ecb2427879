"""numpy fp64 restatement of the guarded optimizer step
(fpnmt_grad_norm_total + fpnmt_amsgrad_step_guard, include/fpnmt.h):
EmaAMSGradRef's step (tests/ema_ref.py) with, ahead of it,

  total  = sum over the tensors that are not frozen of ||grad * grad_scale||^2
           (a caller-supplied norm, scaled by grad_scale^2, where one is given:
           the embedding's IndexedSlices norm)
  skip   = total is not finite, or exceeds the largest fp32 value (the kernel
           sums in fp32: a norm it cannot represent is a skipped step)
  factor = clip / max(sqrt(total), clip)   if global_clipnorm > 0 else 1

A skipped step changes nothing: parameters, m, v, vhat, the average and
`iterations` stay, n_skipped and consecutive go up by one. An applied step
multiplies every gradient by factor (the per-tensor clip, exclusive with the
global one, runs as before when global_clipnorm is 0), n_applied goes up by
one and consecutive returns to 0.

A reference shared by the CPU and GPU tests; it imports nothing of the
package under test."""
import math

import numpy as np

from ema_ref import EmaAMSGradRef

F32_MAX = float(np.finfo(np.float32).max)


class GuardedAMSGradRef(EmaAMSGradRef):
    def __init__(self, shapes, decay=0.0, global_clipnorm=0.0, **kw):
        super().__init__(shapes, decay, **kw)
        self.global_clip = float(global_clipnorm)
        if self.global_clip > 0 and self.clip > 0:
            raise ValueError("clipnorm (per tensor) and global_clipnorm are exclusive")
        self.sumsq_total = 0.0
        self.clip_factor = 1.0
        self.skipped = 0
        self.consecutive = 0
        self.n_skipped = 0
        self.n_applied = 0

    def total(self, grads, rows=None, norms=None, grad_scale=1.0):
        rows = rows or {}
        tot = 0.0
        with np.errstate(over="ignore", invalid="ignore"):
            for n in grads:
                if rows.get(n, (1.0, 0.0, False))[2]:
                    continue
                if norms and n in norms:
                    tot += float(norms[n]) * grad_scale * grad_scale
                else:
                    tot += float(((np.asarray(grads[n], np.float64) * grad_scale) ** 2).sum())
        return tot

    def apply(self, params, grads, lr_fn, rows=None, norms=None, grad_scale=1.0):
        if self.ema is None:
            self.reset(params)
        tot = self.total({n: grads[n] for n in params}, rows, norms, grad_scale)
        self.sumsq_total = tot
        self.skipped = int(not math.isfinite(tot) or tot > F32_MAX)
        if self.skipped:
            self.clip_factor = 0.0
            self.n_skipped += 1
            self.consecutive += 1
            return
        c = self.global_clip
        self.clip_factor = c / max(math.sqrt(tot), c) if c > 0 else 1.0
        scaled = {n: np.asarray(g, np.float64) * self.clip_factor for n, g in grads.items()}
        super().apply(params, scaled, lr_fn, rows, norms, grad_scale)
        self.n_applied += 1
        self.consecutive = 0

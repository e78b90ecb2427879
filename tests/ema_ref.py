"""numpy fp64 restatement of the optimizer step with weight averaging
(fpnmt_amsgrad_step_ema, include/fpnmt.h): GroupedAMSGradRef's step
(tests/param_groups_ref.py), and after every trainable tensor has its new
value the shadow update of tf.train.ExponentialMovingAverage,

  e      = e + omd_t * (p_new - e)
  omd_t  = max(omd, 9 / (10 + t)) if debias else omd,    t = iterations + 1
  omd    = fp32(1 - decay)

omd is the fp32-rounded value the host hands the kernel (1 - decay in double,
rounded once); everything else is fp64. 1 - omd_t is TF's
decay_t = min(decay, (1 + t) / (10 + t)), since 1 - (1 + t) / (10 + t) =
9 / (10 + t). Frozen tensors keep their shadow. The shadow starts as a copy of
the parameters, as TF initialises a shadow variable.

A reference shared by the CPU and GPU tests; it imports nothing of the
package under test."""
import numpy as np

from param_groups_ref import GroupedAMSGradRef


def one_minus_decay_f32(decay):
    """1 - decay in double, rounded once to fp32 (returned as a Python float)."""
    return float(np.float32(1.0 - float(decay)))


def omd_t(omd, debias, t):
    return max(omd, 9.0 / (10.0 + t)) if debias else omd


class EmaAMSGradRef(GroupedAMSGradRef):
    def __init__(self, shapes, decay, debias=True, **kw):
        super().__init__(shapes, **kw)
        self.omd = one_minus_decay_f32(decay)
        self.debias = bool(debias)
        self.ema = None

    def set_decay(self, decay):
        self.omd = one_minus_decay_f32(decay)

    def reset(self, params):
        self.ema = {n: np.array(p, np.float64, copy=True) for n, p in params.items()}

    def apply(self, params, grads, lr_fn, rows=None, norms=None, grad_scale=1.0):
        if self.ema is None:
            self.reset(params)
        rows = rows or {}
        t = float(self.iterations + 1)
        super().apply(params, grads, lr_fn, rows, norms, grad_scale)
        w = omd_t(self.omd, self.debias, t)
        for n in params:
            if rows.get(n, (1.0, 0.0, False))[2]:
                continue
            e = self.ema[n]
            e += w * (params[n] - e)

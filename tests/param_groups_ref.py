"""numpy fp64 restatement of the grouped optimizer step
(fpnmt_amsgrad_step_groups, include/fpnmt.h): Keras AMSGrad with per-tensor
clip_by_norm, the dense and the sparse (IndexedSlices) moment forms, the bias
correction, and per tensor a rate scale s, a decoupled weight decay w and a
frozen flag (frozen = the tensor and its state are skipped):

  g      = clip(grad * grad_scale)            (t * clip) / max(||t||, clip)
  m, v   = moments(g);  vhat = max(vhat, v)
  alpha  = lr * sqrt(1 - beta2^t) / (1 - beta1^t),   t = iterations + 1
  p_new  = (p - (m * (alpha * s)) / (sqrt(vhat) + eps)) - (lr * s * w) * p

A reference shared by the CPU and GPU tests; it imports nothing of the
package under test."""
import numpy as np


class GroupedAMSGradRef:
    def __init__(self, shapes, beta1=0.9, beta2=0.98, eps=1e-9, clipnorm=1.0, sparse=()):
        """shapes: {name: shape}."""
        self.b1, self.b2, self.eps, self.clip = float(beta1), float(beta2), float(eps), float(clipnorm)
        self.m = {n: np.zeros(s, np.float64) for n, s in shapes.items()}
        self.v = {n: np.zeros(s, np.float64) for n, s in shapes.items()}
        self.vhat = {n: np.zeros(s, np.float64) for n, s in shapes.items()}
        self.sparse = set(sparse)
        self.iterations = 0

    def apply(self, params, grads, lr_fn, rows=None, norms=None, grad_scale=1.0):
        """params / grads: {name: array}; params is updated in place (fp64
        arrays). rows: {name: (lr_scale, weight_decay, frozen)}, missing
        names are (1, 0, False). norms: {name: caller-supplied ||g||^2} (the
        embedding's IndexedSlices norm), scaled by grad_scale^2 like the
        kernel does. lr_fn(iterations) -> the step's rate."""
        rows = rows or {}
        it = self.iterations
        lr = float(lr_fn(it))
        t = float(it + 1)
        alpha = lr * np.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
        for n in params:
            s, w, frozen = rows.get(n, (1.0, 0.0, False))
            if frozen:
                continue
            g = np.asarray(grads[n], np.float64) * grad_scale
            if self.clip > 0:
                if norms and n in norms:
                    ss = float(norms[n]) * grad_scale * grad_scale
                else:
                    ss = float((g ** 2).sum())
                nrm = np.sqrt(ss) if ss > 0 else 0.0
                g = (g * self.clip) / max(nrm, self.clip)
            m, v, vh = self.m[n], self.v[n], self.vhat[n]
            if n in self.sparse:
                m[...] = m * self.b1 + g * (1 - self.b1)
                v[...] = v * self.b2 + (g * g) * (1 - self.b2)
            else:
                m += (g - m) * (1 - self.b1)
                v += (g * g - v) * (1 - self.b2)
            np.maximum(vh, v, out=vh)
            p = params[n]
            new = p - (m * (alpha * s)) / (np.sqrt(vh) + self.eps)
            if w != 0:
                new = new - (lr * s * w) * p
            params[n] = new
        self.iterations += 1

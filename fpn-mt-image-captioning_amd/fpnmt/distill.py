"""Token-level knowledge distillation (not in the reference): what
TrainEngine.set_distill / step_distill keep beside the step.

The student trains on the teachers' next-token distribution at every
teacher-forced position, mixed with the hard-label loss
(fpnmt_xent_distill_fwd_bwd, ops.DistillXentFn):
  loss = (1 - alpha) * smoothed CE + alpha * T^2 * KL(softmax(t / T) || softmax(x / T))
Each teacher runs teacher-forced in inference mode under no_grad (encoder,
decoder, vocabulary projection: TrainEngine._eval_forward's path); several
teachers' logits are folded into the first one's buffer by
fpnmt_logits_ensemble over all B * (T - 1) rows (no `fin`), a single
teacher's raw logits go to the loss kernel as they are (it normalises).
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from ._lib import call, ptr, stream_ptr
from .decode import ENSEMBLE_MODES, ensemble_weights_normalised


def check_alpha(alpha, who="alpha"):
    """alpha as a float in [0, 1]; anything else, NaN included, is refused."""
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must lie in [0, 1], got {alpha!r}") from None
    if not 0.0 <= a <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"{who} must lie in [0, 1], got {alpha!r}")
    return a


def check_temperature(t, who="temperature"):
    """A temperature as a finite float > 0; anything else is refused."""
    try:
        x = float(t)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a finite number > 0, got {t!r}") from None
    if not 0.0 < x < math.inf:  # NaN fails both comparisons
        raise ValueError(f"{who} must be a finite number > 0, got {t!r}")
    return x


def check_teachers(teachers, vocab, device, seq_len=None, mode="prob", weights=None):
    """The teachers as a tuple of Transformers with the student's vocabulary
    on its device (at most FPNMT_ENSEMBLE_MAX; none is allowed: the caller
    then feeds teacher_logits), the fold's mode and the weights normalised,
    one per teacher (the student is not part of the mix)."""
    teachers = tuple(teachers)
    if mode not in ENSEMBLE_MODES:
        raise ValueError(f"ensemble_mode must be 'prob' or 'logprob', got {mode!r}")
    if len(teachers) > L.ENSEMBLE_MAX:
        raise ValueError(f"distillation takes at most {L.ENSEMBLE_MAX} teachers, got {len(teachers)}")
    for i, tr in enumerate(teachers):
        k = getattr(getattr(tr, "final_layer", None), "kernel", None)
        if k is None:
            raise ValueError(f"teacher {i} is not a Transformer: {tr!r}")
        if k.shape[1] != vocab:
            raise ValueError(f"teacher {i} has vocabulary {k.shape[1]}, the student {vocab}")
        if k.device != device:
            raise ValueError(f"teacher {i} is on {k.device}, the student on {device}")
        if seq_len is not None and seq_len > tr.decoder.pos_encoding.shape[0]:
            raise ValueError(f"{seq_len} positions exceed the positional table of teacher {i} "
                             f"({tr.decoder.pos_encoding.shape[0]})")
    if not teachers:
        if weights is not None:
            raise ValueError(f"ensemble_weights={weights!r} given without teachers")
        return teachers, ()
    return teachers, ensemble_weights_normalised(len(teachers), weights)


class DistillDesc:
    """The 16-byte fpnmt_distill_desc on the device and its host mirror
    (alpha, temperature). Allocated once and only ever written in place
    (stream-ordered): captured steps hold its pointer and read the values of
    the moment they replay, like the arena's EmaDesc."""

    def __init__(self, device, alpha, temperature):
        self.table = torch.zeros(4, dtype=torch.float32, device=device)
        self.alpha = check_alpha(alpha)
        self.temperature = check_temperature(temperature)
        self._write()

    def _write(self):
        d = L.DistillDesc()
        d.alpha, d.temperature = self.alpha, self.temperature
        self.table.copy_(torch.frombuffer(bytearray(bytes(d)), dtype=torch.float32))  # in place

    def set_alpha(self, alpha):
        self.alpha = check_alpha(alpha)
        self._write()

    def set_temperature(self, t):
        self.temperature = check_temperature(t)
        self._write()


class Distill:
    """The teachers, the fold and the descriptor of one engine."""

    def __init__(self, student, teachers, alpha, temperature, mode, weights):
        k = student.final_layer.kernel
        self.vocab, self.device = k.shape[1], k.device
        self.teachers, self.weights = check_teachers(teachers, self.vocab, self.device, None, mode, weights)
        self.mode = mode
        self.desc = DistillDesc(self.device, alpha, temperature)
        from . import layers as flayers
        self._layers = [list(flayers.weight_layers(t)) for t in self.teachers]

    def refresh_copies(self, dtype):
        """Before a capture or a replay: a teacher's compute copies made stale
        since its last forward (layers.invalidate_weights(): weights loaded
        into it, a hand edit) are rebuilt here, in the buffers they live in,
        outside the graph; a replay cannot do it lazily."""
        from . import layers as flayers
        for t, wl in zip(self.teachers, self._layers):
            if any(m._gen != flayers._GEN[0] for m in wl):
                flayers.prepare_all(t, dtype)

    def check_len(self, seq_len):
        for i, tr in enumerate(self.teachers):
            if seq_len > tr.decoder.pos_encoding.shape[0]:
                raise ValueError(f"step_distill: {seq_len} positions exceed the positional table of teacher {i} "
                                 f"({tr.decoder.pos_encoding.shape[0]})")

    @torch.no_grad()
    def teacher_logits(self, img, tar_inp, mask):
        """(B, T - 1, V) fp32: the teachers' teacher-forced logits, folded.
        Inference mode: nothing is written, no dropout counter advances."""
        import ctypes as C
        outs = []
        for tr in self.teachers:
            enc = tr.encoder(img, False, None)
            dec, _ = tr.decoder(tar_inp, enc, False, mask, None)
            lg = tr.final_layer(dec)
            if lg.dtype != torch.float32:
                raise TypeError(f"a teacher's vocabulary projection gave {lg.dtype}, expected fp32 logits")
            outs.append(lg.contiguous())
        n = len(outs)
        if n == 1:
            return outs[0]
        rows = outs[0].numel() // self.vocab
        call("fpnmt_logits_ensemble", rows, self.vocab, n, (C.c_void_p * n)(*[ptr(x) for x in outs]),
             (C.c_longlong * n)(*[self.vocab] * n), (C.c_float * n)(*self.weights), ENSEMBLE_MODES[self.mode],
             None, ptr(outs[0]), self.vocab, stream_ptr())
        return outs[0]

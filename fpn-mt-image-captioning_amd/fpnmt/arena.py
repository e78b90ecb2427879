"""Flat parameter arena: every trainable tensor of a model lives in ONE fp32
buffer (params), with matching flat gradient / AMSGrad-state buffers.

Why: the optimizer step becomes one fused multi-tensor kernel over the arena
(fpnmt_grad_sumsq + fpnmt_amsgrad_step), the data-parallel gradient exchange is
a handful of large RCCL all-reduces over contiguous buckets, the gradient
zeroing is one memset, and nothing allocates inside a captured hipGraph.
Parameters stay ordinary ``nn.Parameter`` objects (views into the arena), so
``module.parameters()`` / state dicts behave as usual.

The compute copies of conv / dense weights (bf16 or fp32, kernel layouts)
are refreshed by ``prepare()`` after every optimizer step.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L

ALIGN = 64  # elements (256 B) per segment start: keeps 16-B vector loads aligned
BLOCK_ELEMS = 16384


class SegGroups:
    """The per-segment fpnmt_seg_group device table of an arena (lr_scale,
    weight_decay, frozen) and its host mirror. The table is allocated once
    and only ever written in place (stream-ordered): captured optimizer
    graphs hold its pointer and read the values of the moment they replay."""

    def __init__(self, arena, rows):
        """rows: per segment (group index, lr_scale, weight_decay, frozen),
        as fpnmt.param_groups.assign returns them."""
        n = len(arena.params)
        if len(rows) != n:
            raise ValueError(f"SegGroups: {len(rows)} rows for {n} segments")
        self.group_of = [int(r[0]) for r in rows]
        self.lr_scale = [float(r[1]) for r in rows]
        self.weight_decay = [float(r[2]) for r in rows]
        self.frozen = [bool(r[3]) for r in rows]
        tab = (L.SegGroup * max(1, n))()
        for e, s, w, f in zip(tab, self.lr_scale, self.weight_decay, self.frozen):
            e.lr_scale, e.weight_decay, e.frozen = s, w, int(f)
        raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.int32).view(-1, 4)
        self.table = raw.to(arena.device)  # (nseg, 4) int32: float bits, float bits, flag, 0
        self._f32 = self.table.view(torch.float32)
        self._blk_seg = arena._blk_seg_host

    def _write(self, col, segs, values):
        if not segs:
            return
        dev = self.table.device
        idx = torch.tensor(segs, dtype=torch.int64).to(dev)
        if col == 2:
            self.table[:, 2].index_copy_(0, idx, torch.tensor(values, dtype=torch.int32).to(dev))
        else:
            self._f32[:, col].index_copy_(0, idx, torch.tensor(values, dtype=torch.float32).to(dev))

    def set_lr_scale(self, segs, values):
        for i, v in zip(segs, values):
            self.lr_scale[i] = float(v)
        self._write(0, list(segs), [float(v) for v in values])

    def set_weight_decay(self, segs, values):
        for i, v in zip(segs, values):
            self.weight_decay[i] = float(v)
        self._write(1, list(segs), [float(v) for v in values])

    def set_frozen(self, segs, flag):
        for i in segs:
            self.frozen[i] = bool(flag)
        self._write(2, list(segs), [int(bool(flag))] * len(segs))

    def trim(self, b0, b1):
        """[b0, b1) without its leading and trailing blocks of frozen
        segments (workgroups that would only exit are not launched)."""
        while b0 < b1 and self.frozen[self._blk_seg[b0]]:
            b0 += 1
        while b1 > b0 and self.frozen[self._blk_seg[b1 - 1]]:
            b1 -= 1
        return b0, b1


def check_ema_decay(decay, who="ema_decay"):
    """decay as a float in [0, 1); anything else, NaN included, is refused."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must lie in [0, 1), got {decay!r}") from None
    if not 0.0 <= d < 1.0:  # NaN fails both comparisons
        raise ValueError(f"{who} must lie in [0, 1), got {decay!r}")
    return d


def ema_one_minus_decay(decay):
    """The fp32 value the kernel gets: 1 - decay in double, rounded once."""
    import struct
    return struct.unpack("f", struct.pack("f", 1.0 - check_ema_decay(decay)))[0]


def ema_omd_t(one_minus_decay, debias, t):
    """Host restatement (double) of the kernel's 1 - decay_t at t = iterations
    + 1: TF's min(decay, (1 + t) / (10 + t)) written on 1 - decay."""
    return max(one_minus_decay, 9.0 / (10.0 + t)) if debias else one_minus_decay


class EmaDesc:
    """The 16-byte fpnmt_ema_desc of an arena on its device and its host
    mirror (decay, one_minus_decay, debias). Like SegGroups' table it is
    allocated once and only ever written in place (stream-ordered): captured
    optimizer graphs hold its pointer and read the values of the moment they
    replay."""

    def __init__(self, device, decay, debias=True):
        self.table = torch.zeros(4, dtype=torch.int32, device=device)
        self._f32 = self.table.view(torch.float32)
        self.set(decay, debias)

    def set(self, decay, debias=None):
        self.decay = check_ema_decay(decay)
        self.one_minus_decay = ema_one_minus_decay(self.decay)
        if debias is not None:
            self.debias = bool(debias)
        d = L.EmaDesc()
        d.one_minus_decay, d.debias = self.one_minus_decay, int(self.debias)
        host = torch.frombuffer(bytearray(bytes(d)), dtype=torch.int32)
        self.table.copy_(host)  # in place: the pointer captured graphs hold stays

    def host(self):
        """The descriptor as the device holds it (one_minus_decay, debias)."""
        t = self.table.cpu()
        return float(t.view(torch.float32)[0]), int(t[1])


def check_global_clipnorm(x, who="global_clipnorm"):
    """A global clip norm as a finite float >= 0 (0: no clip, only the
    guard); anything else, NaN and infinity included, is refused."""
    try:
        c = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a finite number >= 0, got {x!r}") from None
    if not 0.0 <= c < math.inf:  # NaN fails both comparisons
        raise ValueError(f"{who} must be a finite number >= 0, got {x!r}")
    return c


class StepGuard:
    """The two device records of the guarded step: the 16-byte
    fpnmt_guard_desc (global_clipnorm, written by the host) and the 32-byte
    fpnmt_guard_state (written by the device: the step's ||g||^2, its clip
    factor, whether it was skipped, and the counters). Both are allocated
    once and the descriptor is only ever written in place (stream-ordered):
    captured optimizer graphs hold the pointers and read the values of the
    moment they replay."""

    def __init__(self, device, global_clipnorm=0.0):
        self.desc = torch.zeros(4, dtype=torch.int32, device=device)
        self.state = torch.zeros(8, dtype=torch.int32, device=device)
        self._i64 = self.state.view(torch.int64)  # [2] n_skipped, [3] n_applied
        self.set(global_clipnorm)

    def set(self, global_clipnorm):
        self.global_clipnorm = check_global_clipnorm(global_clipnorm)
        d = L.GuardDesc()
        d.global_clipnorm = self.global_clipnorm
        self.desc.copy_(torch.frombuffer(bytearray(bytes(d)), dtype=torch.int32))  # in place

    @property
    def skipped(self):
        """This step's verdict as a device int32 scalar (a view of the
        state: no copy, no synchronisation)."""
        return self.state[2]

    def set_counts(self, n_skipped, n_applied):
        self._i64[2:4].copy_(torch.tensor([int(n_skipped), int(n_applied)], dtype=torch.int64))

    def host(self):
        """The state as the device holds it (one read-back)."""
        t = self.state.cpu()
        f, q = t.view(torch.float32), t.view(torch.int64)
        return {"sumsq_total": float(f[0]), "clip_factor": float(f[1]), "skipped": int(t[2]),
                "consecutive": int(t[3]), "n_skipped": int(q[2]), "n_applied": int(q[3])}

    def stats(self):
        """host() with grad_norm = sqrt(sumsq_total) in place of the sum."""
        h = self.host()
        ss = h.pop("sumsq_total")
        return {"grad_norm": math.sqrt(ss) if ss >= 0.0 else float("nan"), **h}


class ParamArena:
    def __init__(self, params, device, sparse_names=()):
        """params: ordered list of (name, nn.Parameter) — shared parameters
        appear once. sparse_names: parameters updated with the Keras sparse
        (IndexedSlices) path — the decoder embedding."""
        self.device = torch.device(device)
        self.names, self.params, self.offsets = [], [], []
        seen = set()
        off = 0
        for name, p in params:
            if id(p) in seen:
                continue
            seen.add(id(p))
            self.names.append(name)
            self.params.append(p)
            self.offsets.append(off)
            off += int(math.ceil(p.numel() / ALIGN) * ALIGN)
        self.total = off
        dev = self.device
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.vhat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)  # Keras `iterations`
        nseg = len(self.params)
        self.sumsq = torch.zeros(max(nseg, 1), dtype=torch.float32, device=dev)
        self.index = {}
        seg_off = []
        flags = []
        sparse = set(sparse_names)
        for i, (name, p, o) in enumerate(zip(self.names, self.params, self.offsets)):
            n = p.numel()
            with torch.no_grad():
                self.flat[o:o + n].copy_(p.detach().reshape(-1).to(dev, torch.float32))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
            self.index[id(p)] = i
            seg_off.append(o)
            flags.append(3 if name in sparse else 0)
        seg_off.append(self.total)
        # segment end = start + numel (padding is never touched)
        ends = [o + p.numel() for o, p in zip(self.offsets, self.params)]
        # blocks that never cross a segment
        blk_seg, blk_start = [], []
        for i, (o, e) in enumerate(zip(self.offsets, ends)):
            s = o
            while s < e:
                blk_seg.append(i)
                blk_start.append(s)
                s += BLOCK_ELEMS
        self.nblocks = len(blk_seg)
        self._blk_seg_host = list(blk_seg)
        # first block of every segment (blocks are in segment order): the
        # optimizer sums a segment's per-block norm partials in block order
        seg_blk0, b = [], 0
        for i in range(nseg):
            seg_blk0.append(b)
            while b < len(blk_seg) and blk_seg[b] == i:
                b += 1
        seg_blk0.append(len(blk_seg))
        self._seg_blk0_host = seg_blk0
        self.seg_blk0 = torch.tensor(seg_blk0, dtype=torch.int32, device=dev)
        self.blk_part = torch.zeros(max(len(blk_seg), 1), dtype=torch.float32, device=dev)
        self.blk_seg = torch.tensor(blk_seg or [0], dtype=torch.int32, device=dev)
        self.blk_start = torch.tensor(blk_start or [0], dtype=torch.int64, device=dev)
        # the kernels clamp block ends at off[seg+1] = END of segment seg
        seg_end = torch.tensor([*ends], dtype=torch.int64)
        self.seg_bounds = torch.zeros(nseg + 1, dtype=torch.int64)
        self.seg_bounds[1:] = seg_end
        self.seg_bounds[0] = 0
        self.seg_bounds = self.seg_bounds.to(dev)
        self.seg_flags = torch.tensor(flags or [0], dtype=torch.int32, device=dev)
        self.preparers = []
        self.ema = None  # enable_ema(): the averaged parameters, this arena's layout
        self.ema_desc = None
        self.guard = None  # enable_guard(): the records of the guarded step

    # ----------------------------------------------------- the step guard
    def enable_guard(self, global_clipnorm=0.0):
        """Allocate the guard's two device records (StepGuard).
        amsgrad_step(..., guard=True) then computes the norm of the whole
        gradient on the device, skips the step when it is not finite and,
        with global_clipnorm > 0, scales every gradient by
        clip / max(||g||, clip) (Keras' global_clipnorm). Called again: the
        new clip norm in place, the counters are kept."""
        if self.guard is None:
            self.guard = StepGuard(self.device, global_clipnorm)
        else:
            self.guard.set(global_clipnorm)
        return self.guard

    def set_global_clipnorm(self, x):
        """A new global clip norm from the next step on, written into the
        device descriptor in place (stream-ordered; no recapture). 0 turns
        the clip off and keeps the guard."""
        if self.guard is None:
            raise ValueError("ParamArena: enable_guard() first")
        self.guard.set(x)

    # ---------------------------------------------------- weight averaging
    def enable_ema(self, decay, debias=True):
        """Allocate the shadow arena `ema` (fp32, the layout of `flat`) and
        its device descriptor. ema starts as a copy of flat, as
        tf.train.ExponentialMovingAverage initialises a shadow variable;
        amsgrad_step(..., ema=True) then keeps
        e += (1 - decay_t) * (p_new - e) inside the optimizer kernel, with
        decay_t = min(decay, (1 + t) / (10 + t)) when debias is set."""
        desc = EmaDesc(self.device, decay, debias)  # refuses a bad decay before anything is allocated
        if self.ema is None:
            self.ema = self.flat.detach().clone()
            self.ema_desc = desc
        else:  # already enabled: new values in place, the average is kept
            self.ema_desc.set(decay, debias)
        return self.ema

    def set_ema_decay(self, decay):
        """A new decay from the next step on, written into the device
        descriptor in place (stream-ordered; no recapture)."""
        if self.ema_desc is None:
            raise ValueError("ParamArena: enable_ema() first")
        self.ema_desc.set(decay)

    def reset_ema(self):
        """ema = flat (a new phase of a recipe starts its average afresh)."""
        if self.ema is None:
            raise ValueError("ParamArena: enable_ema() first")
        with torch.no_grad():
            self.ema.copy_(self.flat)

    def swap_ema(self):
        """flat <-> ema in place (fpnmt_swap_f32): the parameters, which are
        views of flat, then read the averaged values; a second call puts
        both back bit for bit."""
        if self.ema is None:
            raise ValueError("ParamArena: enable_ema() first")
        L.call("fpnmt_swap_f32", L.ptr(self.flat), L.ptr(self.ema), self.total, L.stream_ptr())

    # -------------------------------------------------------------- grads
    def zero_grad(self, max_blocks=0):
        """Gradient arena + the per-tensor sum-of-squares slots to zero (HIP
        zero-fill kernels: no eager-PyTorch kernel inside the replayed step).
        max_blocks > 0: the arena's fill on at most that many workgroups (a
        background trickle beside other work on another stream)."""
        if self.grad.is_cuda:
            from ._lib import call, stream_ptr
            nbytes = self.grad.numel() * self.grad.element_size()
            if max_blocks > 0:
                call("fpnmt_fill_zero_grid", self.grad.data_ptr(), nbytes, int(max_blocks), stream_ptr())
            else:
                call("fpnmt_fill_zero", self.grad.data_ptr(), nbytes, stream_ptr())
            call("fpnmt_fill_zero", self.sumsq.data_ptr(), self.sumsq.numel() * self.sumsq.element_size(),
                 stream_ptr())
        else:  # CPU arenas of the host-only tests
            self.grad.zero_()
            self.sumsq.zero_()

    def seg_of(self, p) -> int:
        return self.index[id(p)]

    def sumsq_slot(self, p):
        i = self.index[id(p)]
        return self.sumsq[i:i + 1]

    # ---------------------------------------------------------- optimizer
    def block_of(self, offset):
        """First optimizer block of the segment starting at `offset` (the
        arena's total: nblocks), for amsgrad_step(blocks=...)."""
        if offset >= self.total:
            return self.nblocks
        i = self.offsets.index(offset)
        return self._seg_blk0_host[i]

    def amsgrad_step(self, lr_schedule, beta1=0.9, beta2=0.98, eps=1e-9, clipnorm=1.0, grad_scale=1.0,
                     preps=None, blocks=None, inc_step=True, max_grid=0, groups=None, ema=False,
                     guard=False):
        """Keras AMSGrad + per-tensor clip_by_norm over the arena. preps: a
        device table of fpnmt_seg_prep (one per segment, layers.FusedPrep)
        whose non-null entries get their bf16 compute copies written by the
        same kernel. blocks: (first, end) block range of whole segments (one
        part of a step updated in parts); inc_step: advance `iterations`
        (only the step's last part); max_grid: at most that many workgroups
        striding over the range (0: one per block). groups: a SegGroups of
        this arena (make_groups): the step through fpnmt_amsgrad_step_groups
        with its per-segment rate scale, decoupled weight decay and frozen
        flags; frozen segments at either end of the range are not launched.
        None: the plain entry points, as before. ema: the step through
        fpnmt_amsgrad_step_ema (with or without groups), which also advances
        the shadow arena of enable_ema(); False: the entry points above.
        guard: the step through fpnmt_amsgrad_step_guard (with or without
        groups and ema) on the records of enable_guard(): always
        fpnmt_grad_sumsq_*, whatever clipnorm is, then fpnmt_grad_norm_total,
        then the guarded kernel. The step is one launch: blocks= must contain
        every block that is not frozen and inc_step must be set (the total
        covers the whole arena, and a step updated in parts cannot be
        undone); clipnorm > 0 together with a global clip norm > 0 is
        refused, as Keras refuses it."""
        if ema and self.ema is None:
            raise ValueError("ParamArena.amsgrad_step(ema=True): enable_ema() first")
        if guard:
            if self.guard is None:
                raise ValueError("ParamArena.amsgrad_step(guard=True): enable_guard() first")
            if not inc_step:
                raise ValueError("ParamArena.amsgrad_step(guard=True): inc_step=False is a step in parts, "
                                 "which the guard cannot skip as a whole")
            if clipnorm > 0 and self.guard.global_clipnorm > 0:
                raise ValueError("ParamArena.amsgrad_step(guard=True): clipnorm (per tensor) and global_clipnorm "
                                 "are exclusive; pass clipnorm=0 with a global clip norm")
            lo, hi = (0, self.nblocks) if groups is None else groups.trim(0, self.nblocks)
            q0, q1 = (0, self.nblocks) if blocks is None else blocks
            if hi > lo and not (q0 <= lo and hi <= q1):
                raise ValueError(f"ParamArena.amsgrad_step(guard=True): blocks={(q0, q1)} leaves blocks that are not "
                                 f"frozen outside (they span [{lo}, {hi}))")
        d = L.AdamDesc()
        d.beta1, d.beta2, d.eps, d.clipnorm = beta1, beta2, eps, clipnorm
        d.grad_scale = grad_scale
        if isinstance(lr_schedule, (int, float)):
            d.sched_d_model = 0.0
            d.const_lr = float(lr_schedule)
        else:
            d.sched_d_model = float(lr_schedule.d_model)
            d.sched_warmup = float(lr_schedule.warmup_steps)
            d.sched_mult = float(lr_schedule.multiplier)
            d.sched_warm_pow = float(lr_schedule.warmup_steps ** -1.5)
        b0, b1 = (0, self.nblocks) if blocks is None else blocks
        s = L.stream_ptr()
        if guard:
            gt = None
            if groups is not None:
                b0, b1 = groups.trim(b0, b1)
                gt = L.ptr(groups.table)
            if b1 > b0:
                if gt is not None:
                    L.call("fpnmt_grad_sumsq_groups", b0, b1 - b0, max_grid, L.ptr(self.blk_seg),
                           L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags), gt,
                           L.ptr(self.grad), grad_scale, L.ptr(self.blk_part), s)
                else:
                    L.call("fpnmt_grad_sumsq_part", b0, b1 - b0, max_grid, L.ptr(self.blk_seg),
                           L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags),
                           L.ptr(self.grad), grad_scale, L.ptr(self.blk_part), s)
            gd, gs = L.ptr(self.guard.desc), L.ptr(self.guard.state)
            L.call("fpnmt_grad_norm_total", self.nblocks, L.ptr(self.blk_seg), L.ptr(self.seg_flags), gt,
                   L.ptr(self.sumsq), L.ptr(self.blk_part), L.ptr(self.seg_blk0), grad_scale, gd, gs, s)
            L.call("fpnmt_amsgrad_step_guard", d, b0, b1 - b0, 1, max_grid, L.ptr(self.blk_seg),
                   L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags),
                   L.ptr(self.flat), L.ptr(self.grad), L.ptr(self.m), L.ptr(self.v), L.ptr(self.vhat),
                   L.ptr(self.sumsq), L.ptr(self.blk_part), L.ptr(self.seg_blk0), L.ptr(self.step),
                   L.ptr(preps) if preps is not None else None, gt, L.ptr(self.ema) if ema else None,
                   L.ptr(self.ema_desc.table) if ema else None, gd, gs, s)
            return
        if ema:
            gt = None
            if groups is not None:
                b0, b1 = groups.trim(b0, b1)
                gt = L.ptr(groups.table)
            if clipnorm > 0 and b1 > b0:
                if gt is not None:
                    L.call("fpnmt_grad_sumsq_groups", b0, b1 - b0, max_grid, L.ptr(self.blk_seg),
                           L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags), gt,
                           L.ptr(self.grad), grad_scale, L.ptr(self.blk_part), s)
                else:
                    L.call("fpnmt_grad_sumsq_part", b0, b1 - b0, max_grid, L.ptr(self.blk_seg),
                           L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags),
                           L.ptr(self.grad), grad_scale, L.ptr(self.blk_part), s)
            L.call("fpnmt_amsgrad_step_ema", d, b0, b1 - b0, 1 if inc_step else 0, max_grid, L.ptr(self.blk_seg),
                   L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags),
                   L.ptr(self.flat), L.ptr(self.grad), L.ptr(self.m), L.ptr(self.v), L.ptr(self.vhat),
                   L.ptr(self.sumsq), L.ptr(self.blk_part), L.ptr(self.seg_blk0), L.ptr(self.step),
                   L.ptr(preps) if preps is not None else None, gt, L.ptr(self.ema), L.ptr(self.ema_desc.table), s)
            return
        if groups is not None:
            b0, b1 = groups.trim(b0, b1)
            gt = L.ptr(groups.table)
            if clipnorm > 0 and b1 > b0:
                L.call("fpnmt_grad_sumsq_groups", b0, b1 - b0, max_grid, L.ptr(self.blk_seg), L.ptr(self.blk_start),
                       BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags), gt, L.ptr(self.grad), grad_scale,
                       L.ptr(self.blk_part), s)
            L.call("fpnmt_amsgrad_step_groups", d, b0, b1 - b0, 1 if inc_step else 0, max_grid, L.ptr(self.blk_seg),
                   L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags),
                   L.ptr(self.flat), L.ptr(self.grad), L.ptr(self.m), L.ptr(self.v), L.ptr(self.vhat),
                   L.ptr(self.sumsq), L.ptr(self.blk_part), L.ptr(self.seg_blk0), L.ptr(self.step),
                   L.ptr(preps) if preps is not None else None, gt, s)
            return
        if clipnorm > 0 and b1 > b0:  # clipnorm 0: no clip_by_norm, no norms needed
            L.call("fpnmt_grad_sumsq_part", b0, b1 - b0, max_grid, L.ptr(self.blk_seg), L.ptr(self.blk_start), BLOCK_ELEMS,
                   L.ptr(self.seg_bounds), L.ptr(self.seg_flags), L.ptr(self.grad), grad_scale,
                   L.ptr(self.blk_part), s)
        L.call("fpnmt_amsgrad_step_part", d, b0, b1 - b0, 1 if inc_step else 0, max_grid, L.ptr(self.blk_seg),
               L.ptr(self.blk_start), BLOCK_ELEMS, L.ptr(self.seg_bounds), L.ptr(self.seg_flags), L.ptr(self.flat),
               L.ptr(self.grad), L.ptr(self.m), L.ptr(self.v), L.ptr(self.vhat), L.ptr(self.sumsq),
               L.ptr(self.blk_part), L.ptr(self.seg_blk0), L.ptr(self.step),
               L.ptr(preps) if preps is not None else None, s)

    def make_groups(self, rows):
        """A SegGroups table for this arena from per-segment (group index,
        lr_scale, weight_decay, frozen) rows (fpnmt.param_groups.assign)."""
        return SegGroups(self, rows)

    # ------------------------------------------------------ compute copies
    def register_preparer(self, fn):
        self.preparers.append(fn)

    def prepare(self):
        for fn in self.preparers:
            fn()

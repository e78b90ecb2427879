"""The training step of the reference (utils/pipeline.py:64-80) as a
hipGraph-replayed MI355X step.

step(img, caption_token):
  tar_inp = tok[:, :-1]; tar_real = tok[:, 1:]            (pipeline.py:66-67)
  mask = create_masks(tar_inp)                              (pipeline.py:69)
  logits = transformer(img, tar_inp, True, mask)            (pipeline.py:72)
  loss = masked CE mean over B*T                            (pipeline.py:50-57,75)
  grads -> [RCCL all-reduce] -> clip_by_norm per tensor -> AMSGrad   (pipeline.py:77-78)
  refresh the bf16/fp32 compute copies of the weights

The first call runs eagerly (warms the autograd engine and the allocator);
the second call captures the whole step into a hipGraph (torch.cuda.CUDAGraph
drives hipGraph on ROCm) and every later call only copies the new batch into
the static input buffers and replays.

step_weighted(img, tok, weights) is the self-critical form of the same step
(not in the reference): tok holds n = tok.shape[0] // B captions per image,
the encoder runs once per image and its output is repeated n times for the
decoder (ops.RepeatRowsFn), and caption r's CE terms are weighted by
weights[r] (ops.WeightedXentFn, still a mean over all rows). Its graphs are
captured per shape beside the plain step's; arena, optimizer state and step
counter are shared, so the two kinds of step can alternate.

step_distill(img, tok, teacher_logits=None) is step() with the loss swapped
for token-level knowledge distillation (not in the reference; set_distill,
fpnmt/distill.py): the teachers run teacher-forced in inference mode ahead
of the student's forward, in the same graph, and the loss is
ops.DistillXentFn. Its graphs are kept beside the others and share the same
arena, optimizer kernel, guard, average and parameter groups.

With world > 1 (or split_backward=True) the step is a sequence of graphs:
  G1      forward + loss + the decoder's backward (stops at the encoder
          output, which enters the decoder as a leaf)
  G2      the encoder's backward from that leaf's gradient (stops at the
          feature extractor's five level outputs, which enter the encoder as
          leaves)
  S1..S5  the feature extractor's backward one stage at a time, in backward
          order: the shared heads, the FPN, then the backbone segments
          C4->C5, C3->C4, input->C3 (FeatureExtractor.staged: every stage
          reads detached leaves of the previous one's outputs)
  G3      clip + AMSGrad + compute-copy refresh
and the gradient arena is ordered decoder, encoder layers, then the feature
extractor stage by stage, so each range's RCCL all-reduce is issued as soon
as its graph ends (the decoder's and vocabulary projection's ~45 M of 105 M
parameters after G1, the encoder layers' after G2, the res5 segment's 15 M
after S3, ...) and runs on RCCL's stream while the next graphs compute; only
the last segment's (input->C3, ~1.4 M at ResNet-50) is exposed. G3 waits for
all of them (stream waits; the host never blocks).
"""
from __future__ import annotations

import contextlib

import torch
import torch.distributed as dist

import fpnmt
from . import _lib as L
from . import dist as fdist
from . import distill as fdistill
from . import layers as flayers
from . import ops
from .arena import ParamArena, check_ema_decay, check_global_clipnorm
from .layers import group_param_order
from . import param_groups as pgroups


class TrainEngine:
    def __init__(self, transformer, schedule, beta1=0.9, beta2=0.98, eps=1e-9, clipnorm=1.0, use_graph=True,
                 group=None, bucket_bytes=fdist.DEFAULT_BUCKET_BYTES, split_backward=None, bucket_dtype=None,
                 sync_bn=True, label_smoothing=0.0, param_groups=None, ema_decay=None, ema_debias=True,
                 global_clipnorm=None, skip_nonfinite=False):
        """param_groups: None runs the plain step (every trainable tensor at
        the schedule's rate, no decay: the reference's optimizer). A list of
        fpnmt.param_groups.ParamGroup (an empty one included) runs the same
        step through fpnmt_amsgrad_step_groups with a per-segment rate scale,
        decoupled weight decay and frozen flags. Every tensor that is
        trainable at construction stays in the arena, frozen ones included:
        optimizer state and checkpoints keep one layout across phases, and
        set_lr_scale / set_weight_decay / set_frozen change a group later.

        ema_decay: None (the default) keeps no average and runs the entry
        points above. A number in [0, 1) keeps an exponential moving average
        of every trainable parameter in a shadow arena (arena.ema, fp32),
        updated inside the optimizer kernel (fpnmt_amsgrad_step_ema) as
        tf.train.ExponentialMovingAverage would after each step:
        e += (1 - decay_t) * (p - e), with decay_t = min(ema_decay,
        (1 + t) / (10 + t)) when ema_debias is set (TF's num_updates form,
        t = the step count) and ema_decay otherwise. Parameters, optimizer
        state and losses are bit for bit those of the engine without it.
        ema_weights() puts the average under the model; set_ema_decay /
        reset_ema change it between steps. Under data parallelism every rank
        keeps its own average: the parameters are bitwise equal across ranks
        after every step, so the averages are too, and nothing is exchanged.

        global_clipnorm / skip_nonfinite: either one turns the step guard on
        (both at their defaults: the step launches what it launched before,
        with the same bits). The optimizer tail then computes the norm of the
        whole gradient on the device (fpnmt_grad_norm_total, after the
        all-reduce under data parallelism, so every rank decides alike) and
        the update goes through fpnmt_amsgrad_step_guard: a step whose
        squared norm is not finite (an Inf or NaN anywhere in the gradient, or
        finite values whose squares overflow fp32) is skipped on the device,
        with no host round trip: parameters, m, v, vhat, the average, the
        compute copies and `iterations` stay as they were, and the counters
        of guard_stats() record it. `iterations` feeds the dropout keys, so
        the step after a skipped one draws the masks the skipped one drew.
        global_clipnorm > 0 also scales every gradient by
        clip / max(||g||, clip), Keras' global_clipnorm
        (tf.clip_by_global_norm); it always skips non-finite steps, since a
        non-finite norm cannot be clipped against. It is exclusive with the
        per-tensor clipnorm > 0, as in Keras, and the guard is exclusive with
        fpnmt.config.early_update, which updates the transformer's segments
        before the backward has produced the rest of the gradient.
        set_global_clipnorm changes the clip between steps.
        Limit: a skipped step's forward pass has already moved the BatchNorm
        moving statistics (MobileNetV2 in training mode). They are buffers,
        not in the arena, and are not rolled back."""
        from models.transformer import create_masks  # noqa: F401 (ensures import path)
        groups_in = pgroups.validate(param_groups) if param_groups is not None else None
        if not 0.0 <= float(label_smoothing) < 1.0:  # NaN fails both comparisons
            raise ValueError(f"TrainEngine: label_smoothing must lie in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = float(label_smoothing)
        if ema_decay is not None:
            ema_decay = check_ema_decay(ema_decay, "TrainEngine: ema_decay")
        self.guard_on = global_clipnorm is not None or bool(skip_nonfinite)
        if global_clipnorm is not None:
            global_clipnorm = check_global_clipnorm(global_clipnorm, "TrainEngine: global_clipnorm")
            if global_clipnorm > 0 and clipnorm > 0:
                raise ValueError("TrainEngine: global_clipnorm and the per-tensor clipnorm are exclusive "
                                 f"(got global_clipnorm={global_clipnorm!r}, clipnorm={clipnorm!r}); pass clipnorm=0")
        if self.guard_on and fpnmt.config.early_update:
            raise ValueError("TrainEngine: global_clipnorm / skip_nonfinite cannot be combined with "
                             "fpnmt.config.early_update (the early part updates the transformer's segments "
                             "before the whole gradient exists)")
        self.model = transformer
        self.schedule = schedule
        self.adam = dict(beta1=beta1, beta2=beta2, eps=eps, clipnorm=clipnorm)
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.bucket_bytes = bucket_bytes
        self.bucket_dtype = bucket_dtype
        dev = next(transformer.parameters()).device
        emb = transformer.decoder.embedding.embeddings
        named = [(n, p) for n, p in transformer.named_parameters() if p.requires_grad]
        named = group_param_order(transformer, named)  # grouped projections: contiguous blocks
        self.split = (self.world > 1) if split_backward is None else bool(split_backward)
        fe_prefix = "encoder.feature_extractor."
        # transformer parameters first (stable: DenseGroups live in the
        # transformer and stay contiguous), then the feature extractor's
        # stage by stage in backward order (one contiguous range per stage)
        stage_pref = transformer.encoder.feature_extractor.stage_prefixes()
        fe = [x for x in named if x[0].startswith(fe_prefix)]
        stage_of = {}
        for n, _ in fe:
            rel = n[len(fe_prefix):]
            stage_of[n] = next((i for i, ps in enumerate(stage_pref) if any(rel.startswith(q) for q in ps)),
                               len(stage_pref))  # unmatched: a last range of its own
        unmatched = [n for n, _ in fe if stage_of[n] == len(stage_pref)]
        if unmatched:
            # every feature-extractor parameter must sit in an exchanged stage
            # range, or DP ranks would drift apart silently
            raise ValueError(f"TrainEngine: feature-extractor parameters outside every stage: {unmatched[:4]}")
        fe.sort(key=lambda x: stage_of[x[0]])  # stable within a stage
        # the decoder side (decoder + vocabulary projection) first: its
        # gradients are complete when G1 ends; then the encoder layers (G2)
        dec_side = [x for x in named if x[0].startswith(("decoder.", "final_layer."))]
        enc_side = [x for x in named if not x[0].startswith(("decoder.", "final_layer.", fe_prefix))]
        named = dec_side + enc_side + fe
        emb_name = [n for n, p in named if p is emb][0]
        self.arena = ParamArena(named, dev, sparse_names=[emb_name])
        fe_idx = [i for i, n in enumerate(self.arena.names) if n.startswith(fe_prefix)]
        self.split_at = self.arena.offsets[fe_idx[0]] if fe_idx else self.arena.total
        offs = self.arena.offsets + [self.arena.total]
        dec_end = offs[len(dec_side)]
        # exchange ranges: [0] the decoder side, [1] the encoder layers, then
        # one per feature-extractor stage
        bounds = [(0, dec_end), (dec_end, self.split_at)]
        for st in range(len(stage_pref) + 1):
            idx = [i for i in fe_idx if stage_of[self.arena.names[i]] == st]
            bounds.append((offs[idx[0]], offs[idx[-1] + 1]) if idx else (0, 0))
        self.ranges = bounds
        transformer.decoder.embedding.sumsq_slot = self.arena.sumsq_slot(emb)
        self.emb_seg = self.arena.seg_of(emb)
        ops.runtime.seed_tensor = self.arena.step
        # parameter groups: the device table is built once (captured graphs
        # hold its pointer); frozen groups lose requires_grad, so autograd
        # prunes their backward, and keep their arena segments
        self.param_groups = groups_in
        self.seg_groups = None
        transformer.encoder.feature_extractor.freeze_backbone_bn = False
        if groups_in is not None:
            rows = pgroups.assign(self.arena.names, self.arena.params, groups_in)
            self.seg_groups = self.arena.make_groups(rows)
            self._check_frozen_set()
            self._apply_frozen()
        # opt-in low-precision buckets: one preallocated staging copy of the
        # gradient arena; each range is cast into it at the end of the graph
        # that produced it and the reduced sum is cast back at the start of the
        # update graph (both casts captured; zeros in the alignment gaps)
        self.low = None
        if bucket_dtype is not None and bucket_dtype != self.arena.grad.dtype and self.world > 1:
            self.low = torch.zeros(self.arena.total, dtype=bucket_dtype, device=dev)
        if self.world > 1:
            # identical initial weights on every rank
            fdist.broadcast_(self.arena.flat, 0, group)
            self.bn_group = None
            if sync_bn and fdist.has_batchnorm(transformer):
                # training-mode BatchNorm (MobileNetV2) over the global batch,
                # as the reference's single-device step computes it. Its
                # collectives run on a communicator of their own: with the
                # split step they sit inside the stage graphs while the
                # gradient ranges' async all-reduces are still in flight on
                # the engine's group, and RCCL does not order two streams'
                # collectives on one communicator
                self.bn_group = fdist.new_group_like(group)
                fdist.set_sync_batchnorm(transformer, self.bn_group)
        # weight averaging: the shadow arena starts as a copy of the (broadcast)
        # parameters; its descriptor is allocated once, captured graphs hold it
        self._ema_open = False
        if ema_decay is not None:
            self.arena.enable_ema(ema_decay, ema_debias)
        # the step guard: its two records are allocated once, captured graphs hold them
        if self.guard_on:
            self.arena.enable_guard(global_clipnorm or 0.0)
        flayers.invalidate_weights()
        self.dtype = None
        self.use_graph = use_graph
        # the optimizer blocks of the transformer's segments (the arena's head,
        # up to the feature extractor's first segment): _early_update's range
        self.early_blocks = self.arena.block_of(self.split_at)
        self._upd_stream = None
        self._early_pending = False
        self.calls = 0
        self.graphs = None
        self.static = None
        self._wsteps = {}  # step_weighted: shapes -> [calls, graphs, static]
        self._esteps = {}  # eval_step: shapes -> [calls, graph, static inputs, outputs]
        self._distill = None  # set_distill: the teachers, the fold and the device descriptor
        self._dsteps = {}  # step_distill: shapes -> [calls, graphs, static]
        self._distill_stats = None
        self._eval_gen = -1  # the compute copies' generation the eval graphs last saw
        self.eval_totals = torch.zeros(3, dtype=torch.float64, device=dev)  # eval_step(accumulate=True)

    # ------------------------------------------------------ parameter groups
    _frozen_layers = {}  # id -> weight layer whose kernel is frozen (their compute copies need no refresh)

    def _group_segs(self, name):
        """Arena segments of the group `name` ("default": the unmatched ones)."""
        if self.seg_groups is None:
            raise ValueError("TrainEngine was built without param_groups")
        names = [g.name for g in self.param_groups]
        if name in names:
            gi = names.index(name)
        elif name == pgroups.DEFAULT_NAME:
            gi = -1
        else:
            raise ValueError(f"no parameter group {name!r}; groups: {names + [pgroups.DEFAULT_NAME]}")
        return [i for i, g in enumerate(self.seg_groups.group_of) if g == gi]

    def _check_frozen_set(self, frozen=None):
        """What can be frozen: nothing, the backbone, or the whole feature
        extractor. The pruning rests on autograd never reaching a frozen
        tensor, which holds for those two sets (the backbone is the model's
        first stage, the extractor its first two); the transformer's fused
        Functions always write their weight gradients, and a trainable layer
        behind an identity shortcut of frozen ones would get no gradient."""
        frozen = self.seg_groups.frozen if frozen is None else frozen
        names = self.arena.names
        got = {names[i] for i, f in enumerate(frozen) if f}
        if not got:
            return
        bb = {n for n in names if n.startswith(pgroups.backbone_prefixes(self.model))}
        fe = {n for n in names if n.startswith(pgroups.FE_PREFIX)}
        if got != bb and got != fe:
            odd = sorted(got - fe) or sorted(got ^ bb)
            raise ValueError("TrainEngine: frozen groups must cover exactly the backbone or the whole feature "
                             f"extractor (param_groups.backbone_group / feature_extractor_group); e.g. {odd[:3]}")

    def _apply_frozen(self):
        """requires_grad of every arena parameter from the frozen flags, the
        backbone's BatchNorm mode, and the set of frozen weight layers."""
        sg = self.seg_groups
        for p, f in zip(self.arena.params, sg.frozen):
            p.requires_grad_(not f)
        fe = self.model.encoder.feature_extractor
        bbp = pgroups.backbone_prefixes(self.model)
        # a frozen backbone's BatchNorm (MobileNetV2) runs in inference mode:
        # no moving-statistics update, no SyncBN collective
        fe.freeze_backbone_bn = any(f for n, f in zip(self.arena.names, sg.frozen) if n.startswith(bbp))
        self._frozen_layers = {id(m): m for m in flayers.weight_layers(self.model)
                               if id(m.kernel) in self.arena.index and sg.frozen[self.arena.index[id(m.kernel)]]}
        self._range_frozen_cache = {}

    def _range_frozen(self, part):
        """Every segment of exchange range `part` is frozen (an empty range is not)."""
        if self.seg_groups is None:
            return False
        hit = self._range_frozen_cache.get(part)
        if hit is None:
            a, b = self.ranges[part]
            segs = [i for i, o in enumerate(self.arena.offsets) if a <= o < b]
            hit = self._range_frozen_cache[part] = bool(segs) and all(self.seg_groups.frozen[i] for i in segs)
        return hit

    def _refresh_frozen_copies(self):
        """Before a capture or a replay: frozen layers are left out of the
        step's compute-copy refresh, so copies made stale since
        (layers.invalidate_weights(): a hand edit, a precision change) are
        rebuilt here, outside the graph."""
        if any(m._gen != flayers._GEN[0] for m in self._frozen_layers.values()):
            flayers.prepare_all(self.model, fpnmt.compute_dtype())

    def set_lr_scale(self, name, s):
        """Group `name` trains at s times the schedule's rate from the next
        step on. Written into the device table in place (stream-ordered): the
        captured graphs are kept and the next replay reads the new value."""
        s = pgroups._finite_nonneg(s, f"set_lr_scale({name!r})")
        segs = self._group_segs(name)
        self.seg_groups.set_lr_scale(segs, [s] * len(segs))

    def set_weight_decay(self, name, w):
        """Group `name` decays with coefficient w (a number, or a callable
        (name, param) -> number such as param_groups.decay_matrices(0.01))
        from the next step on; in place, no recapture, like set_lr_scale."""
        segs = self._group_segs(name)
        vals = [pgroups.decay_of(w, self.arena.names[i], self.arena.params[i], f"set_weight_decay({name!r})")
                for i in segs]
        self.seg_groups.set_weight_decay(segs, vals)

    def set_frozen(self, name, flag):
        """Freeze (flag True) or unfreeze group `name`: flips requires_grad on
        its parameters, so the backward no longer visits them (pruned, not
        masked), and the frozen flag of their segments in the device table.
        The captured step graphs (step, step_weighted, step_distill, the split
        sequence) are dropped, since the autograd graph they recorded changed:
        the next call at a shape runs eagerly and the one after captures, as
        at start-up. Eval graphs are kept. Optimizer state is kept too: a frozen
        group's m, v and vhat stay as they are, and after unfreezing it
        continues from them with the global step counter (its bias correction
        is that of the current step, not of the steps it took part in)."""
        segs = self._group_segs(name)
        flag = bool(flag)
        new = list(self.seg_groups.frozen)
        for i in segs:
            new[i] = flag
        self._check_frozen_set(new)
        if new == self.seg_groups.frozen:
            return
        self.seg_groups.set_frozen(segs, flag)
        self._apply_frozen()
        self.calls = 0
        self.graphs = None
        self.static = None
        self._wsteps = {}
        self._dsteps = {}
        self._distill_stats = None
        flayers.invalidate_weights()  # an unfrozen layer comes back into the refresh

    # ----------------------------------------------------- weight averaging
    def _require_ema(self, who):
        if self.arena.ema is None:
            raise ValueError(f"TrainEngine.{who}: the engine was built without ema_decay")

    @property
    def ema_decay(self):
        """The decay in force (None: no average is kept)."""
        return self.arena.ema_desc.decay if self.arena.ema_desc is not None else None

    def set_ema_decay(self, decay):
        """A new decay in [0, 1) from the next step on. Written into the
        device descriptor in place (stream-ordered): the captured graphs are
        kept and the next replay reads the new value, like set_lr_scale."""
        self._require_ema("set_ema_decay")
        self.arena.set_ema_decay(check_ema_decay(decay, "TrainEngine.set_ema_decay"))

    def reset_ema(self):
        """The average restarts from the current parameters (a new phase of a
        recipe). The step counter, and with it the debias term, goes on."""
        self._require_ema("reset_ema")
        if self._ema_open:
            raise RuntimeError("TrainEngine.reset_ema inside ema_weights(): the arenas are swapped")
        self.arena.reset_ema()

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate, decode or save on the averaged weights:

            with engine.ema_weights():
                engine.eval_step(img, tok)

        On entry the parameter arena and the average are exchanged in place
        (fpnmt_swap_f32: every nn.Parameter stays the view it was, so captured
        eval and decode graphs go on reading the same addresses) and the
        compute copies are rebuilt from the averaged masters; on exit both are
        put back. The exchange is exact, so the training state afterwards is
        bit for bit what it was. step / step_weighted raise while it is open.

        Only parameters are averaged. Buffers are not: BatchNorm moving
        statistics (MobileNetV2) and the frozen-BN folds of the ResNet
        backbone are the model's current ones inside the context too."""
        self._require_ema("ema_weights")
        if self._ema_open:
            raise RuntimeError("TrainEngine.ema_weights: already open")
        self._swap_ema()
        self._ema_open = True
        try:
            yield self
        finally:
            self._ema_open = False
            self._swap_ema()

    def _swap_ema(self):
        self.arena.swap_ema()
        flayers.invalidate_weights()
        # every copy in use is rewritten in the buffer it lives in: graphs that
        # eval_step or a decoder captured read the new values at their next
        # replay, and eval_step has nothing left to refresh
        flayers.prepare_all(self.model, fpnmt.compute_dtype())
        self._eval_gen = flayers._GEN[0]

    def _check_trainable_now(self, who):
        if self._ema_open:
            raise RuntimeError(f"TrainEngine.{who} inside ema_weights(): the model holds the averaged weights")

    # ------------------------------------------------------- the step guard
    def _require_guard(self, who):
        if self.arena.guard is None:
            raise ValueError(f"TrainEngine.{who}: the engine was built without global_clipnorm / skip_nonfinite")

    @property
    def global_clipnorm(self):
        """The global clip norm in force (0: the guard alone; None: no guard)."""
        return self.arena.guard.global_clipnorm if self.arena.guard is not None else None

    def set_global_clipnorm(self, x):
        """A new global clip norm from the next step on (0: no clip, the
        guard stays). Written into the device descriptor in place
        (stream-ordered): the captured graphs are kept and the next replay
        reads the new value, like set_ema_decay."""
        self._require_guard("set_global_clipnorm")
        x = check_global_clipnorm(x, "TrainEngine.set_global_clipnorm")
        if x > 0 and self.adam["clipnorm"] > 0:
            raise ValueError("TrainEngine.set_global_clipnorm: the engine clips per tensor "
                             f"(clipnorm={self.adam['clipnorm']!r}); the two are exclusive")
        self.arena.set_global_clipnorm(x)

    def guard_stats(self):
        """One read-back of the guard's device state: {"grad_norm" (the last
        step's ||g|| over all trainable tensors, after grad_scale; inf or nan
        on a skipped step), "clip_factor" (1 without a global clip, 0 on a
        skipped step), "skipped" (the last step, 0 / 1), "consecutive"
        (skipped steps in a row), "n_skipped", "n_applied"}."""
        self._require_guard("guard_stats")
        return self.arena.guard.stats()

    @property
    def step_skipped(self):
        """The last step's verdict as a device int32 scalar (no
        synchronisation); None without the guard."""
        return self.arena.guard.skipped if self.arena.guard is not None else None

    # ------------------------------------------------------------ pieces
    def _one(self, loss):
        """The loss's seed gradient, kept across steps (loss.backward() would
        fill a fresh one with a kernel launch every step)."""
        one = getattr(self, "_one_t", None)
        if one is None or one.device != loss.device or one.dtype != loss.dtype:
            one = self._one_t = torch.ones((), dtype=loss.dtype, device=loss.device)
        return one

    def _zero_grad_fork(self):
        """arena.zero_grad(), or — zero_grad_overlap_grid > 0 on a GPU — the
        same fill as a trickle of that many workgroups on a side stream forked
        here, so it runs beside the forward pass (which writes no gradient);
        _zero_grad_join() makes the compute stream wait for it before the
        backward. Graph-capturable (wait_stream fork / join)."""
        grid = fpnmt.config.zero_grad_overlap_grid
        if grid <= 0 or not self.arena.grad.is_cuda:
            self.arena.zero_grad()
            return None
        if getattr(self, "_zero_stream", None) is None:
            self._zero_stream = torch.cuda.Stream()
        zs = self._zero_stream
        zs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(zs):
            self.arena.zero_grad(max_blocks=grid)
        return zs

    @staticmethod
    def _zero_grad_join(zs):
        if zs is not None:
            torch.cuda.current_stream().wait_stream(zs)

    def _logits_loss(self, enc_fn, tok, weights, soft=None):
        """targets -> encoder output (enc_fn) -> decoder -> logits -> loss.
        weights None: the plain step's masked CE. Otherwise tok holds
        n = rows / images captions per image: the encoder output is repeated n
        times and caption r's terms are weighted by weights[r].
        soft (step_distill): ("run", img) runs the teachers on img ahead of
        the student's forward, ("given", logits) takes precomputed soft
        targets; the loss is then ops.DistillXentFn."""
        m = self.model
        tar_inp, tar_real, mask = ops.decoder_targets(tok)  # tok[:, :-1], tok[:, 1:], create_masks(tar_inp)
        if soft is not None:
            d = self._distill
            tea = d.teacher_logits(soft[1], tar_inp, mask) if soft[0] == "run" else soft[1]
            dec, _ = m.decoder(tar_inp, enc_fn(), True, mask, None)
            loss, self._distill_stats = ops.DistillXentFn.apply(m.final_layer(dec), tar_real, tea,
                                                                self.label_smoothing, d.desc.table)
            return loss
        enc = enc_fn()
        if weights is None:
            dec, _ = m.decoder(tar_inp, enc, True, mask, None)
            if self.label_smoothing > 0.0:
                return ops.SmoothedXentFn.apply(m.final_layer(dec), tar_real, self.label_smoothing)
            return ops.MaskedXentFn.apply(m.final_layer(dec), tar_real)
        dec, _ = m.decoder(tar_inp, ops.RepeatRowsFn.apply(enc, tok.shape[0] // enc.shape[0]), True, mask, None)
        return ops.WeightedXentFn.apply(m.final_layer(dec), tar_real, weights, tok.shape[1] - 1)

    def _fwd_bwd(self, img, tok, weights=None, soft=None):
        ops.runtime.reset_sites()  # dropout sites numbered from the step's start
        ops.reset_grad_sums()
        zs = self._zero_grad_fork()
        if self.guard_on and fpnmt.config.early_update:
            raise ValueError("TrainEngine: fpnmt.config.early_update cannot be combined with the step guard")
        early = (self.world == 1 and fpnmt.config.early_update and self.arena.flat.is_cuda
                 and 0 < self.early_blocks < self.arena.nblocks)
        ops.runtime.on_transformer_grads = self._early_update if early else None
        try:
            loss = self._logits_loss(lambda: self.model.encoder(img, True, None), tok, weights, soft)
            self._zero_grad_join(zs)
            with L.deferred_reductions(fpnmt.config.defer_reductions), ops.side_wgrad():
                torch.autograd.backward([loss], [self._one(loss)])  # ordered reductions batched at the exit
        finally:
            ops.runtime.on_transformer_grads = None
        self._stage_low(None)
        return loss

    def _early_update(self):
        """Called from the backward (ops.transformer_grads_barrier) once the
        transformer's backward is complete: its queued reductions run now,
        then the transformer's segments (the arena's leading blocks) get their
        clip + AMSGrad + compute-copy refresh on a second stream, overlapping
        the feature extractor's backward on the compute stream. _update joins
        the streams and runs the feature extractor's part (the same kernels
        over the remaining blocks: bitwise the one-launch update)."""
        ops.join_side()
        L.defer_checkpoint()
        if self._upd_stream is None:
            self._upd_stream = torch.cuda.Stream()
        st = self._upd_stream
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            # a few persistent workgroups without LDS (no fused compute-copy
            # refresh: those copies are written in the tail) so the waves sit
            # beside the backward's GEMM blocks; one workgroup per block held
            # every CU slot until it drained (profiles/r05/early_update_r5h.txt)
            self.arena.amsgrad_step(self.schedule, grad_scale=1.0 / self.world, preps=None,
                                    blocks=(0, self.early_blocks), inc_step=False,
                                    max_grid=fpnmt.config.early_update_grid, groups=self.seg_groups,
                                    ema=self.arena.ema is not None, **self.adam)
        self._early_pending = True

    def _fwd_bwd_split(self, img, tok, weights=None, soft=None):
        """G1: forward + loss + the decoder's backward down to the encoder
        output (a leaf of the decoder; with weights, the leaf is the encoder
        output per image, ahead of its repeat)."""
        ops.runtime.reset_sites()
        ops.reset_grad_sums()
        zs = self._zero_grad_fork()
        m = self.model
        side = {}

        def encode():
            feats, stages = m.encoder.feature_extractor.staged(img, training=True)
            leaves = [f.detach().requires_grad_(f.requires_grad) for f in feats]
            enc = m.encoder.from_features(leaves, True, None)
            side.update(stages=stages, leaves=leaves, enc=enc, enc_leaf=enc.detach().requires_grad_(True))
            return side["enc_leaf"]
        loss = self._logits_loss(encode, tok, weights, soft)
        stages, leaves, enc, enc_leaf = side["stages"], side["leaves"], side["enc"], side["enc_leaf"]
        self._zero_grad_join(zs)
        with L.deferred_reductions(fpnmt.config.defer_reductions), ops.side_wgrad():
            torch.autograd.backward([loss], [self._one(loss)])
        self._enc = (enc, enc_leaf)
        self._stages = [(outs, lvs if lvs is not None else leaves) for outs, lvs, _ in stages]
        self._stage_low(0)
        return loss

    def _bwd_encoder(self):
        """G2: the encoder layers' backward from the encoder output's gradient
        down to the feature extractor's level outputs."""
        enc, enc_leaf = self._enc
        if enc_leaf.grad is not None and enc.requires_grad:
            with L.deferred_reductions(fpnmt.config.defer_reductions), ops.side_wgrad():
                torch.autograd.backward([enc], [enc_leaf.grad])
        self._stage_low(1)

    def _bwd_stage(self, i):
        """S_i: one feature-extractor stage's backward from its outputs'
        leaf gradients (left by the stages after it in forward order)."""
        outs, leaves = self._stages[i]
        pairs = [(o, lf.grad) for o, lf in zip(outs, leaves)
                 if o.requires_grad and lf.grad is not None and o.numel() > 0]
        if pairs:
            with L.deferred_reductions(fpnmt.config.defer_reductions), ops.side_wgrad():
                torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
        self._stage_low(2 + i)

    def _stage_low(self, part):
        """Cast the exchange range `part` (None: the whole arena) of the
        gradients into the low-precision staging copy (bucket mode only)."""
        if self.low is None:
            return
        a, b = (0, self.arena.total) if part is None else self.ranges[part]
        if b > a:
            fdist.cast_into(self.low[a:b], self.arena.grad[a:b])

    def _exchange(self, part=None, wait=True):
        """SUM all-reduce of the gradient arena: part 0 = the decoder side's
        range (+ the embedding's sparse-norm accumulator), 1 = the encoder
        layers', part k >= 2 = the feature extractor's stage k-2 range, None =
        all."""
        if self.world <= 1:
            return []
        g = self.arena.grad
        rng = (0, self.arena.total) if part is None else self.ranges[part]
        extra = [self.arena.sumsq[self.emb_seg:self.emb_seg + 1]] if part in (None, 0) else None
        if rng[1] <= rng[0]:
            return []
        if part is not None and self._range_frozen(part):
            return []  # nothing in the range is trained: no gradient, no exchange
        staging = self.low[rng[0]:rng[1]] if self.low is not None else None
        return fdist.allreduce_flat(g[rng[0]:rng[1]], self.bucket_bytes, self.group, extra=extra, wait=wait,
                                    bucket_dtype=self.bucket_dtype, staging=staging)

    def _update(self):
        ops.check_grad_sums()  # no consumer-summed input gradient left parked by the backward(s)
        if self.low is not None:
            fdist.cast_into(self.arena.grad, self.low)  # the reduced sums back into the fp32 arena
        fp = flayers.fused_prep(self.model, self.arena)
        blocks = None
        skip = fp.layers if fp else ()
        if self._early_pending:  # the transformer's part ran beside the backward: join, then the rest
            torch.cuda.current_stream().wait_stream(self._upd_stream)
            self._early_pending = False
            blocks = (self.early_blocks, self.arena.nblocks)
            # the early part wrote no compute copies: only the late part's
            # layers are refreshed by the optimizer kernel
            if fp:
                skip = {id(m) for m in fp._mods
                        if self.arena.offsets[self.arena.index[id(m.kernel)]] >= self.split_at}
        self.arena.amsgrad_step(self.schedule, grad_scale=1.0 / self.world, preps=fp.table if fp else None,
                                blocks=blocks, groups=self.seg_groups, ema=self.arena.ema is not None,
                                guard=self.guard_on, **self.adam)
        if self._frozen_layers:
            # frozen masters do not change: their (fresh) copies need no refresh
            skip = set(skip) | {i for i, m in self._frozen_layers.items() if m._gen == flayers._GEN[0]}
        flayers.prepare_all(self.model, skip=skip)
        if fp:
            fp.mark_fresh()

    def _eager(self, img, tok, weights=None, soft=None):
        if self.split:
            loss = self._fwd_bwd_split(img, tok, weights, soft)
            works = self._exchange(0, wait=False)
            self._bwd_encoder()
            works += self._exchange(1, wait=False)
            for i in range(len(self._stages)):
                if self._range_frozen(2 + i):
                    continue
                self._bwd_stage(i)
                works += self._exchange(2 + i, wait=False)
            for w in works:
                w.wait()
        else:
            loss = self._fwd_bwd(img, tok, weights, soft)
            self._exchange()
        self._update()
        return loss.detach()

    # ---------------------------------------------------------- timeline
    def enable_timeline(self, on=True):
        """Record HIP events around every graph replay and every range's
        exchange of the following replayed split steps (timeline() reads
        them): where each exchange completes against the stage graphs that
        run under it, and what is left exposed before the update graph."""
        self._tl = [] if on else None

    def timeline(self):
        """Per recorded step: the graphs' end times and the exchanges' issue /
        completion times, in ms from the step's start (synchronizes)."""
        torch.cuda.synchronize()
        return [t.read() for t in (self._tl or [])]

    _tl = None

    # -------------------------------------------------------------- step
    def step(self, img, tok):
        """One training step; returns the (device) loss of this batch."""
        self._check_trainable_now("step")
        self.calls += 1
        if not self.use_graph or self.calls == 1:
            import fpnmt
            flayers.prepare_all(self.model, fpnmt.compute_dtype())
            return self._eager(img, tok)
        self._refresh_frozen_copies()
        if self.graphs is None:
            self._capture(img, tok)
        if img.shape != self.static[0].shape or tok.shape != self.static[1].shape:
            # a batch of another shape (the short last batch of an epoch: the
            # loaders keep tf.data's drop_remainder=False) cannot go through
            # the static buffers; tf.function retraces for it, this runs it
            # eagerly on the same arena / optimizer state
            import fpnmt
            flayers.prepare_all(self.model, fpnmt.compute_dtype())
            return self._eager(img, tok)
        self.static[0].copy_(img)
        self.static[1].copy_(tok)
        return self._replay(self.graphs, self.static[2])

    def step_weighted(self, img, tok, weights):
        """One self-critical step: img (B, H, W, 3), tok (B * n, T_full) padded
        captions, n per image in image order, weights (B * n,) fp32 (the
        captions' advantages; any sign). The step is step()'s with the encoder
        run once per image and its output repeated n times, and the loss
        (1 / rows) * sum_r weights[r // (T_full - 1)] * mask_r * ce_r. Returns
        the (device) loss. The first call at a shape runs eagerly, the second
        captures, later ones copy image, tokens and weights into the static
        buffers and replay. The engine's label_smoothing does not apply here:
        a self-critical step has no one-hot target to soften, and its results
        are the same bits whatever label_smoothing is."""
        B = img.shape[0]
        if tok.dim() != 2 or B < 1 or tok.shape[0] % B or tok.shape[0] == 0:
            raise ValueError(f"step_weighted: {tuple(tok.shape)} captions for {B} images")
        if tuple(weights.shape) != (tok.shape[0],) or weights.dtype != torch.float32:
            raise ValueError(f"step_weighted: weights must be fp32 of shape ({tok.shape[0]},), "
                             f"got {weights.dtype} {tuple(weights.shape)}")
        self._check_trainable_now("step_weighted")
        key = (tuple(img.shape), tuple(tok.shape), tok.dtype)
        ent = self._wsteps.setdefault(key, [0, None, None])
        ent[0] += 1
        if not self.use_graph or ent[0] == 1:
            flayers.prepare_all(self.model, fpnmt.compute_dtype())
            return self._eager(img, tok, weights)
        self._refresh_frozen_copies()
        if ent[1] is None:
            ent[1], ent[2] = self._capture(img, tok, weights)
        graphs, static = ent[1], ent[2]
        static[0].copy_(img)
        static[1].copy_(tok)
        static[3].copy_(weights)
        return self._replay(graphs, static[2])

    # ------------------------------------------------------- distillation
    def set_distill(self, teachers, alpha=0.5, temperature=1.0, ensemble_mode="prob", ensemble_weights=None):
        """Turn token-level knowledge distillation on for step_distill (not in
        the reference). teachers: a sequence of Transformers with the
        student's vocabulary on its device, at most fpnmt._lib.ENSEMBLE_MAX;
        they may differ in depth, width and backbone. It may be empty when
        every step_distill call brings teacher_logits. Several teachers are
        folded as the decode-time ensemble is (fpnmt_logits_ensemble,
        ensemble_mode "prob" or "logprob", ensemble_weights one per teacher,
        normalised; the student is not part of the mix). The loss is
        (1 - alpha) * CE at the engine's label_smoothing + alpha *
        temperature^2 * KL(teacher || student) at that temperature; alpha in
        [0, 1], temperature finite > 0. Both live in a 16-byte device record
        allocated here, which set_distill_alpha / set_distill_temperature
        write in place. The engine holds the teachers strongly and never
        writes to them; their compute copies are refreshed outside the graph
        before a step when layers.invalidate_weights() made them stale (new
        weights loaded into a teacher). The positional-table length cannot be
        checked here, where no caption length is known: step_distill checks
        it against its tokens when it runs the teachers (with teacher_logits=
        the teachers are not run and nothing needs the table).
        set_distill(None) clears them and drops the
        distillation graphs; step, step_weighted and eval_step launch what
        they launched before either way."""
        self._dsteps = {}
        self._distill_stats = None
        if teachers is None:
            self._distill = None
            return
        self._distill = fdistill.Distill(self.model, teachers, alpha, temperature, ensemble_mode, ensemble_weights)

    def _require_distill(self, who):
        if self._distill is None:
            raise ValueError(f"TrainEngine.{who}: call set_distill first")
        return self._distill

    def set_distill_alpha(self, alpha):
        """A new alpha from the next step on, written into the device record
        in place (stream-ordered): captured steps are kept and the next
        replay reads the new value, like set_ema_decay."""
        self._require_distill("set_distill_alpha").desc.set_alpha(alpha)

    def set_distill_temperature(self, temperature):
        """A new temperature from the next step on; in place, no recapture."""
        self._require_distill("set_distill_temperature").desc.set_temperature(temperature)

    @property
    def distill_stats(self):
        """The last step_distill's (3,) fp32 device tensor {loss, hard CE
        (without the 1 - alpha), KL (without the alpha T^2)}, means over all
        rows; no synchronisation. None before the first such step. After a
        replayed step it is the graph's static tensor, overwritten by the
        next replay."""
        return self._distill_stats

    def step_distill(self, img, tok, teacher_logits=None):
        """One distillation step: step() with the loss swapped for
        ops.DistillXentFn against the teachers' soft targets. Each teacher
        runs teacher-forced on (img, tok[:, :-1]) in inference mode under
        no_grad, ahead of the student's forward on the compute stream (it
        writes nothing and advances no dropout counter); teacher_logits
        (B, T_full - 1, V) fp32 on the device replaces that pass with
        precomputed soft targets (raw logits or log-probabilities: the kernel
        normalises). Returns the (device) loss; distill_stats holds its
        parts. Per input shape the first call runs eagerly, the second
        captures, later ones copy image, tokens (and teacher_logits) into
        static buffers and replay. Arena, optimizer kernel, guard, average
        and parameter groups are step()'s, so the kinds of step can
        alternate. A NaN in the soft targets makes the loss and the gradient
        NaN: the step guard, when on, skips such a step."""
        d = self._require_distill("step_distill")
        B = img.shape[0]
        if tok.dim() != 2 or tok.shape[0] != B or tok.shape[1] < 2:
            raise ValueError(f"step_distill: {tuple(tok.shape)} captions for {B} images")
        if teacher_logits is None:
            if not d.teachers:
                raise ValueError("step_distill: set_distill was given no teachers; pass teacher_logits")
            d.check_len(tok.shape[1] - 1)
        else:
            want = (B, tok.shape[1] - 1, d.vocab)
            if (not torch.is_tensor(teacher_logits) or tuple(teacher_logits.shape) != want
                    or teacher_logits.dtype != torch.float32 or teacher_logits.device != d.device):
                got = ((teacher_logits.dtype, tuple(teacher_logits.shape), str(teacher_logits.device))
                       if torch.is_tensor(teacher_logits) else type(teacher_logits))
                raise ValueError(f"step_distill: teacher_logits must be fp32 of shape {want} on {d.device}, got {got}")
        self._check_trainable_now("step_distill")
        given = teacher_logits is not None
        key = (tuple(img.shape), tuple(tok.shape), tok.dtype, given)
        ent = self._dsteps.setdefault(key, [0, None, None])
        ent[0] += 1
        if not self.use_graph or ent[0] == 1:
            dt = fpnmt.compute_dtype()
            flayers.prepare_all(self.model, dt)
            if not given:
                for t in d.teachers:
                    flayers.prepare_all(t, dt)
            return self._eager(img, tok, None, ("given", teacher_logits) if given else ("run", img))
        self._refresh_frozen_copies()
        if not given:
            d.refresh_copies(fpnmt.compute_dtype())
        if ent[1] is None:
            ent[1], ent[2] = self._capture(img, tok, None, teacher_logits if given else "run")
        graphs, static = ent[1], ent[2]
        static[0].copy_(img)
        static[1].copy_(tok)
        if given:
            static[4].copy_(teacher_logits)
        loss = self._replay(graphs, static[2])
        self._distill_stats = static[5]
        return loss

    # ---------------------------------------------------------- held out
    def reset_eval_totals(self):
        """Zero the running sums eval_step(accumulate=True) adds to."""
        self.eval_totals.zero_()

    def _eval_forward(self, img, tok, n, accumulate):
        m = self.model
        totals = self.eval_totals if accumulate else torch.empty(3, dtype=torch.float64, device=img.device)
        tar_inp, tar_real, mask = ops.decoder_targets(tok)
        enc = m.encoder(img, False, None)
        if n > 1:
            enc = ops.RepeatRowsFn.apply(enc, n)
        dec, _ = m.decoder(tar_inp, enc, False, mask, None)
        loss, logp, ln, hit = ops.caption_eval(m.final_layer(dec), tar_real, self.label_smoothing, totals,
                                               accumulate)
        return {"loss": loss, "caption_logp": logp, "caption_len": ln, "caption_hit": hit, "totals": totals}

    @torch.no_grad()
    def eval_step(self, img, tok, n_per_image=1, accumulate=False):
        """The held-out form of step(): the loss of (img, tok) without an
        update. The model runs in inference mode (no dropout, BatchNorm on its
        moving statistics), the encoder once per image with n_per_image
        captions each (tok (B * n_per_image, T_full), image-major), and the
        loss launch (fpnmt_xent_smooth_fwd_bwd without a gradient, at the
        engine's label_smoothing) also gives each position's log-probability
        and arg-max hit, which fpnmt_caption_stats sums per caption.

        Returns device tensors only: "loss" (the step's convention: the
        smoothed CE, a mean over all rows), "caption_logp" (rows,) fp32 (the
        unsmoothed teacher-forced log-probability, <end> included),
        "caption_len" / "caption_hit" (rows,) int32, "totals" (3,) f64 = the
        sums of log-probability, tokens and hits. accumulate=True adds the
        sums to the engine's eval_totals (reset_eval_totals() zeroes them) and
        returns that tensor as "totals".

        Nothing is written: no parameter, gradient, optimizer state, moving
        statistic or dropout counter. Per shape the first call runs eagerly,
        the second captures, later ones copy image and tokens into static
        buffers and replay (their outputs are then the graph's static tensors,
        overwritten by the next replay); there is no host synchronisation."""
        B, n = img.shape[0], int(n_per_image)
        if tok.dim() != 2 or B < 1 or n < 1 or tok.shape[0] != B * n or tok.shape[1] < 2:
            raise ValueError(f"eval_step: {tuple(tok.shape)} captions for {B} images x {n}")
        dt = fpnmt.compute_dtype()
        key = (tuple(img.shape), tuple(tok.shape), tok.dtype, img.dtype, n, bool(accumulate), dt)
        ent = self._esteps.setdefault(key, [0, None, None, None])
        ent[0] += 1
        if not self.use_graph or ent[0] == 1:
            flayers.prepare_all(self.model, dt)
            self._eval_gen = flayers._GEN[0]
            return self._eval_forward(img, tok, n, accumulate)
        if self._eval_gen != flayers._GEN[0]:
            # parameters edited by hand / loaded since (a step or a checkpoint
            # restore refreshes the copies itself, in the buffers the graph reads)
            flayers.prepare_all(self.model, dt)
            self._eval_gen = flayers._GEN[0]
        if ent[1] is None:
            s_img, s_tok = img.detach().clone(), tok.detach().clone()
            out = {}
            ent[1] = capture_sequence([lambda: out.update(self._eval_forward(s_img, s_tok, n, accumulate))])[0]
            ent[2], ent[3] = (s_img, s_tok), out
        ent[2][0].copy_(img)
        ent[2][1].copy_(tok)
        ent[1].replay()
        return dict(ent[3])

    def _replay(self, graphs, loss):
        """Replay one captured step (the exchanges between its graphs)."""
        if self.split:
            g1, g2, *gs, g3 = graphs
            tl = _Timeline() if self._tl is not None else None
            g1.replay()
            works = self._exchange(0, wait=False)  # overlaps the next graphs on RCCL's stream
            if tl:
                tl.graph("G1")
                tl.exchange(0, works)
            g2.replay()
            w = self._exchange(1, wait=False)
            works += w
            if tl:
                tl.graph("G2")
                tl.exchange(1, w)
            for i, g in enumerate(gs):
                if g is None:  # a stage whose parameters are all frozen: no backward, no exchange
                    continue
                g.replay()
                w = self._exchange(2 + i, wait=False)
                works += w
                if tl:
                    tl.graph(f"S{i + 1}")
                    tl.exchange(2 + i, w)
            for w in works:
                w.wait()  # the compute stream waits; the host does not block
            if tl:
                tl.graph("waits")
            g3.replay()
            if tl:
                tl.graph("G3")
                self._tl.append(tl)
            return loss
        g_fb, g_up = graphs
        g_fb.replay()
        if g_up is not None:
            self._exchange()
            g_up.replay()
        return loss

    def _capture(self, img, tok, weights=None, soft=None):
        """Capture the step on static copies of its inputs. The plain step's
        graphs become self.graphs / self.static; a weighted step's (graphs,
        static) are returned to step_weighted, a distillation step's (soft:
        "run", or the teacher logits to make a static copy of) to
        step_distill, with the static soft targets and the step's (3,)
        statistics as static[4] and static[5]."""
        s_img = img.detach().clone()
        s_tok = tok.detach().clone()
        s_w = weights.detach().clone() if weights is not None else None
        s_z = None
        if soft is not None:
            s_z = soft.detach().clone() if torch.is_tensor(soft) else None
            soft = ("given", s_z) if s_z is not None else ("run", s_img)
        out = {}
        if self.split:
            def g1():
                out["loss"] = self._fwd_bwd_split(s_img, s_tok, s_w, soft).detach()
            n = len(self.model.encoder.feature_extractor.stage_prefixes())
            live = [i for i in range(n) if not self._range_frozen(2 + i)]
            stage_fns = [(lambda i=i: self._bwd_stage(i)) for i in live]
            got = capture_sequence([g1, self._bwd_encoder] + stage_fns + [self._update])
            stage_graphs = [None] * n  # a wholly frozen stage has no graph
            for i, g in zip(live, got[2:-1]):
                stage_graphs[i] = g
            graphs = got[:2] + stage_graphs + got[-1:]
        elif self.world == 1:
            def g():
                out["loss"] = self._fwd_bwd(s_img, s_tok, s_w, soft).detach()
                self._update()
            graphs = (capture_sequence([g])[0], None)
        else:
            def g1():
                out["loss"] = self._fwd_bwd(s_img, s_tok, s_w, soft).detach()
            graphs = tuple(capture_sequence([g1, self._update]))
        static = (s_img, s_tok, out["loss"], s_w)
        if soft is not None:
            return graphs, static + (s_z, self._distill_stats)
        if weights is None:
            self.graphs, self.static = graphs, static
        return graphs, static


class _Timeline:
    """Events of one split step (TrainEngine.enable_timeline). A graph's
    event is recorded on the compute stream after its replay; an exchange's
    completion on a probe stream made to wait for the collective right after
    it is issued (the probe is otherwise idle, so its event fires when the
    collective ends) — or the gloo worker's own `done` event."""

    def __init__(self):
        self.t0 = self._rec()
        self.graphs, self.exch = [], []

    @staticmethod
    def _rec(stream=None):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream or torch.cuda.current_stream())
        return e

    def graph(self, name):
        self.graphs.append((name, self._rec()))

    def exchange(self, part, works):
        issued = self._rec()
        dones = []
        for w in works:
            ev = getattr(w, "done_event", None)
            if ev is None:
                probe = torch.cuda.Stream()
                with torch.cuda.stream(probe):
                    getattr(w, "work", w).wait()  # the collective itself (not a cast-back)
                    ev = self._rec(probe)
            dones.append(ev)  # a gloo job's `done` is recorded by its worker before Work.wait() returns
        self.exch.append((part, issued, dones))

    def read(self):
        f = lambda e: round(self.t0.elapsed_time(e), 4)
        out = {"graphs": [{"name": n, "end_ms": f(e)} for n, e in self.graphs], "exchanges": []}
        for part, issued, dones in self.exch:
            done = [f(e) for e in dones if e is not None]
            out["exchanges"].append({"range": part, "issued_ms": f(issued), "done_ms": max(done) if done else None})
        return out


def capture_sequence(fns, pool=None):
    """Capture fns[i] into graph i, back to back on one side stream, sharing
    one private memory pool; replay them in the same order.

    torch.cuda.graph() runs gc.collect() + empty_cache() at every capture
    entry: between two captures of one step that can free (and hand out
    again) pool memory an earlier graph still writes, e.g. tensors kept
    alive only through reference cycles of the earlier capture's autograd
    graph — measured as a silently diverging split-backward step once other
    graphs replayed in between. Here the collection runs once, before the
    first capture."""
    import gc
    gc.collect()
    torch.cuda.synchronize()
    pool = pool if pool is not None else torch.cuda.graph_pool_handle()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(st):
        for fn in fns:
            g = torch.cuda.CUDAGraph()
            g.capture_begin(pool=pool)
            try:
                fn()
            finally:
                g.capture_end()
            graphs.append(g)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    return graphs

"""Pipeline: model + optimizer construction, masked CE loss, the training step
and caption prediction (reference: utils/pipeline.py:8-154).

Same members as the reference Pipeline: transformer, learning_rate,
optimizer, train_loss (Keras Mean), ckpt / ckpt_manager / smart_ckpt_saver
(restoring the latest checkpoint at construction), loss, train_step, predict.

Differences that are deliberate and documented:
  - the tokenizer / COCO evaluator (pipeline.py:14-15, dataset.py) are out of
    the hot-path scope: pass target_vocab_size / start / end token ids, or a
    Keras tokenizer JSON with word_index;
  - train_step runs as a replayed hipGraph (fpnmt.train.TrainEngine);
  - predict reproduces the reference's beam procedure, which starts all beams
    identical and therefore equals greedy arg-max decoding with ties to the
    lowest token id (pipeline.py:101-144); it decodes BEAM_SEARCH_N identical
    rows like the reference, on the HIP decode path (fpnmt.decode).
"""
import json
import math

import torch

from common.common_definitions import (BEAM_SEARCH_N, CLIPNORM_MODE, DATADIR, DATATYPE_VAL, DROPOUT_RATE, END_TOKEN,
                                       IMAGE_INPUT_SIZE, START_TOKEN, WARM_UP_STEPS, d_model, dff, num_heads,
                                       num_layers, TOP_K)
import fpnmt
from fpnmt import ops
from fpnmt.checkpoint import Checkpoint, CheckpointManager
from fpnmt.param_groups import recipe_groups
from fpnmt.train import TrainEngine
from models.transformer import Transformer, create_look_ahead_mask
from utils.utils import CustomSchedule, Mean, SmartCheckpointSaver


def clipnorm_for(mode=CLIPNORM_MODE, clipnorm=1.0):
    """utils/pipeline.py:30 Adam(..., clipnorm=1.): 'per_tensor' applies it
    as TF >= 2.4's apply_gradients does (clip_by_norm per gradient); 'none'
    reproduces TF 2.0-2.3 custom loops, which ignored clipnorm."""
    if mode == "per_tensor":
        return clipnorm
    if mode == "none":
        return 0.0
    raise ValueError(f"CLIPNORM_MODE must be 'per_tensor' or 'none', got {mode!r}")


def load_word_index(tokenizer_filename):
    """word_index of a Keras tokenizer JSON (dataset.py:125-135 format)."""
    with open(tokenizer_filename) as f:
        cfg = json.load(f)
    cfg = cfg.get("config", cfg)
    wi = cfg["word_index"]
    return json.loads(wi) if isinstance(wi, str) else wi


class Pipeline:
    def __init__(self, tokenizer_filename=None, checkpoint_path=None, max_seq_len=32, target_vocab_size=None,
                 image_size=IMAGE_INPUT_SIZE, n_layers=num_layers, backbone=None, rate=DROPOUT_RATE,
                 device="cuda", init=None, use_graph=True, clipnorm_mode=CLIPNORM_MODE, max_to_keep=100,
                 data_dir=DATADIR, data_type_val=DATATYPE_VAL, label_smoothing=0.0, param_groups=None,
                 backbone_lr_scale=1.0, freeze=(), weight_decay=0.0, ema_decay=None, ema_debias=True,
                 global_clipnorm=None, skip_nonfinite=False):
        """param_groups (a list of fpnmt.param_groups.ParamGroup), or the
        common cases by keyword: backbone_lr_scale (the CNN backbone at that
        fraction of the transformer's rate), freeze (a subset of {"backbone",
        "feature_extractor"}), weight_decay (decoupled, on matrices only).
        The keywords build the groups "backbone", "feature_extractor" (the
        FPN and heads) and "transformer", whose values
        engine.set_lr_scale / set_weight_decay / set_frozen change later. Not
        in the reference; at the defaults the step is the reference's.

        ema_decay in [0, 1) keeps an exponential moving average of the
        parameters inside the optimizer step (TrainEngine(ema_decay=...),
        ema_debias as in tf.train.ExponentialMovingAverage(num_updates=...));
        eval_step, validate, score_captions, predict_batch and evaluate then
        take weights="ema" to run on the averaged weights, and checkpoints
        carry the average. None (the default): no average, the step as before.

        global_clipnorm / skip_nonfinite turn the step guard on
        (TrainEngine(global_clipnorm=..., skip_nonfinite=...)): a step whose
        gradient holds an Inf or NaN, or whose squared norm overflows fp32, is
        skipped on the device with no host round trip, and global_clipnorm >
        0 clips the gradient by its norm over all tensors (Keras'
        global_clipnorm). The global clip is exclusive with the reference's
        per-tensor one: pass clipnorm_mode="none" with it, e.g.
        Pipeline(clipnorm_mode="none", global_clipnorm=1.0). guard_stats()
        reads the last step's gradient norm and the counters; checkpoints
        carry the counters; train_loss leaves skipped steps out. A skipped
        step's forward pass has already moved the BatchNorm moving statistics
        (MobileNetV2): they are buffers, not parameters, and are not rolled
        back. Both at their defaults: the step as before."""
        if global_clipnorm is not None and float(global_clipnorm) > 0 and clipnorm_for(clipnorm_mode) > 0:
            raise ValueError(f"Pipeline: global_clipnorm={global_clipnorm!r} with clipnorm_mode={clipnorm_mode!r}: "
                             "the per-tensor clip and the global clip are exclusive (as in Keras); "
                             "pass clipnorm_mode='none' with global_clipnorm")
        self.max_seq_len = max_seq_len
        self._metric_eval_src = (data_dir, data_type_val)
        self._metric_eval = None
        self.start_token, self.end_token = START_TOKEN, END_TOKEN
        self.tokenizer = None
        if tokenizer_filename is not None:
            from utils.text import load_tokenizer_from_path
            self.tokenizer = load_tokenizer_from_path(tokenizer_filename)  # pipeline.py:14-15
            wi = self.tokenizer.word_index
            self.start_token, self.end_token = wi["<start>"], wi["<end>"]
            if target_vocab_size is None:
                target_vocab_size = len(wi)
        self.target_vocab_size = target_vocab_size or TOP_K
        input_vocab_size = math.ceil(image_size / 16) ** 2  # pipeline.py:20
        self._arch = dict(n_layers=n_layers, backbone=backbone, input_vocab_size=input_vocab_size)  # load_member
        self.transformer = Transformer(n_layers, d_model, num_heads, dff, input_vocab_size, self.target_vocab_size,
                                       rate, max_seq_len=self.max_seq_len, backbone=backbone, init=init).to(device)
        self.learning_rate = CustomSchedule(dff, WARM_UP_STEPS)  # pipeline.py:29 (d_model arg = dff)
        recipe = recipe_groups(self.transformer, backbone_lr_scale, freeze, weight_decay)
        if param_groups is not None and recipe is not None:
            raise ValueError("Pipeline: give param_groups or backbone_lr_scale / freeze / weight_decay, not both")
        self.engine = TrainEngine(self.transformer, self.learning_rate, beta1=0.9, beta2=0.98, eps=1e-9,
                                  clipnorm=clipnorm_for(clipnorm_mode), use_graph=use_graph,
                                  label_smoothing=label_smoothing,  # not in the reference; 0: its one-hot loss
                                  param_groups=param_groups if param_groups is not None else recipe,
                                  ema_decay=ema_decay, ema_debias=ema_debias,
                                  global_clipnorm=global_clipnorm, skip_nonfinite=skip_nonfinite)
        self.optimizer = self.engine
        self.train_loss = Mean(name="train_loss")  # pipeline.py:35
        self.checkpoint_path = checkpoint_path
        # pipeline.py:38-48: checkpoint + manager, restore the latest if any
        self.ckpt = Checkpoint(transformer=self.transformer, optimizer=self.engine)
        self.ckpt_manager = None
        self.smart_ckpt_saver = None
        if checkpoint_path is not None:
            self.ckpt_manager = CheckpointManager(self.ckpt, checkpoint_path, max_to_keep=max_to_keep)
            self.smart_ckpt_saver = SmartCheckpointSaver(self.ckpt_manager)
            if self.ckpt_manager.latest_checkpoint:
                self.ckpt.restore(self.ckpt_manager.latest_checkpoint)
                print("Latest checkpoint restored!!")

    @property
    def metric_eval(self):
        """pipeline.py:15 MetricEval(DATADIR, DATATYPE_VAL): CIDEr of a results
        file against the ground-truth captions (train.py:76). Built on first
        use: the reference constructs it eagerly, which requires the COCO
        annotation file even for runs that never evaluate."""
        if self._metric_eval is None:
            from dataset import MetricEval
            self._metric_eval = MetricEval(*self._metric_eval_src)
        return self._metric_eval

    def _weights(self, weights):
        """The context a call runs in: weights="model" the trained parameters
        (nothing to do), "ema" the averaged ones (engine.ema_weights(): the
        arenas exchanged and the compute copies rebuilt, both put back at the
        end; buffers such as BatchNorm statistics are not averaged)."""
        import contextlib
        if weights == "model":
            return contextlib.nullcontext()
        if weights != "ema":
            raise ValueError(f"weights must be 'model' or 'ema', got {weights!r}")
        if self.engine.arena.ema is None:
            raise ValueError("weights='ema' needs a Pipeline built with ema_decay")
        return self.engine.ema_weights()

    def loss(self, real, pred):
        """Masked sparse CE from logits, mean over ALL positions (pipeline.py:50-57)."""
        return ops.MaskedXentFn.apply(pred, real)

    def guard_stats(self):
        """The step guard's telemetry (TrainEngine.guard_stats; one
        read-back): grad_norm, clip_factor, skipped, consecutive, n_skipped,
        n_applied. Needs global_clipnorm or skip_nonfinite."""
        return self.engine.guard_stats()

    def train_step(self, img, caption_token):
        """pipeline.py:64-80: one optimizer step, then train_loss(loss)
        (device-side running mean: no host synchronisation per step). With
        the step guard on, a skipped step's loss stays out of train_loss
        (selected on the guard's device word, still without a read-back)."""
        loss = self.engine.step(img, caption_token)
        if self.engine.guard_on:
            self.train_loss(loss, keep=1 - self.engine.step_skipped)
        else:
            self.train_loss(loss)
        return loss

    def train_step_scst(self, img, refs, n_samples=5, baseline="mean", reward=None, temperature=1.0, top_k=0,
                        top_p=1.0, seed=None, image_keys=None):
        """One self-critical (reward-optimising) step, the usual second phase
        after cross-entropy training; not in the reference. Samples n_samples
        captions per image (fpnmt.decode.SampleDecoder, max_seq_len - 1
        positions), scores each on the host, and takes one optimizer step on
        the samples weighted by their advantages (fpnmt.scst,
        TrainEngine.step_weighted: the encoder runs once per image).

        img (B, H, W, 3) on the GPU; refs: per image its reference captions as
        token-id lists (without <start> / <end>). reward: None scores with
        CIDEr-D over refs (utils.cider_reward.CiderDReward, document
        frequencies of this batch), or any callable (image_index,
        candidate_ids) -> float — e.g. a CiderDReward built once over the
        whole training set, behind a lambda that maps the batch index to its
        image key. baseline "mean": each sample against the mean reward of the
        image's other samples (n_samples >= 2); "greedy": against the reward
        of the greedy caption (one more decode). seed None: a new draw every
        call; a given seed repeats its samples.

        Returns {"loss" (device tensor), "reward_mean", "baseline_mean",
        "sample_logp_mean", "samples", "advantages"}. The rewards are computed
        on the host from the sampled ids, which costs the step one host
        synchronisation; train_step has none.

        reward a fpnmt.cider_device.DeviceCiderD (built once over the whole
        training set, on the images' device): the rewards, advantages and
        token rows are computed on the device (fpnmt_ciderd_reward,
        fpnmt_scst_pack) and the step has no read-back and, from its third
        call at a shape on, no host synchronisation. image_keys names the
        images' keys in that corpus (None: the table rows 0 .. B - 1); refs
        is not needed. Returns device tensors only: "loss", "rewards" (B, n)
        f64, "advantages" (B, n) fp32, 0-dim "reward_mean" / "baseline_mean" /
        "sample_logp_mean", and the sampler's "hist" / "slen" / "fin"
        (fpnmt.decode.sampled_ids turns them into id lists); no "samples".
        reward "device" builds such tables from this batch's refs every step
        (the document frequencies of reward None): a convenience, with host
        work for the tables; a corpus-level instance is the intended use."""
        tr = getattr(self, "_scst", None)
        if tr is None:
            from fpnmt.scst import SelfCriticalTrainer
            tr = self._scst = SelfCriticalTrainer(self.transformer, self.engine, self.start_token, self.end_token,
                                                  self.max_seq_len)
        return tr.step(img, refs, n_samples=n_samples, baseline=baseline, reward=reward, temperature=temperature,
                       top_k=top_k, top_p=top_p, seed=seed, image_keys=image_keys)

    # ------------------------------------------------------- distillation
    def set_teachers(self, teachers, alpha=0.5, temperature=1.0, ensemble_mode="prob", ensemble_weights=None):
        """Token-level knowledge distillation (not in the reference): put what
        an ensemble, a larger model or an averaged checkpoint knows into this
        model, which then decodes at single-model cost. teachers: Transformers
        (load_member's results) or Pipelines (their .transformer), with this
        vocabulary on this device, at most fpnmt._lib.ENSEMBLE_MAX; several
        are folded as predict_batch(ensemble=...) folds them (ensemble_mode,
        ensemble_weights one per teacher). train_step_distill then trains on
        (1 - alpha) * the train_step loss + alpha * temperature^2 * KL(teachers
        || model) at that temperature (TrainEngine.set_distill);
        engine.set_distill_alpha / set_distill_temperature anneal either
        between steps. set_teachers(None) turns it off. Checkpoints carry
        neither the teachers nor alpha / temperature: the teachers are
        external models, and a restored pipeline calls set_teachers again."""
        if teachers is not None:
            teachers = [t.transformer if isinstance(t, Pipeline) else t for t in teachers]
        self.engine.set_distill(teachers, alpha, temperature, ensemble_mode, ensemble_weights)

    def train_step_distill(self, img, caption_token, teacher_logits=None):
        """train_step against the teachers' soft targets
        (TrainEngine.step_distill): one optimizer step, then
        train_loss(loss) with the mixed loss, a skipped step left out under
        the step guard as in train_step. teacher_logits (B, T - 1, V) fp32 on
        the device: precomputed soft targets instead of running the
        teachers."""
        loss = self.engine.step_distill(img, caption_token, teacher_logits)
        if self.engine.guard_on:
            self.train_loss(loss, keep=1 - self.engine.step_skipped)
        else:
            self.train_loss(loss)
        return loss

    def distill_stats(self):
        """The last train_step_distill's parts, one read-back: {"loss" (the
        mixed loss), "hard" (the smoothed CE, without the 1 - alpha), "kl"
        (without the alpha T^2)}, means over all positions; with "alpha" and
        "temperature" as set."""
        s = self.engine.distill_stats
        if s is None:
            raise ValueError("Pipeline.distill_stats: no train_step_distill has run")
        loss, hard, kl = s.tolist()
        d = self.engine._distill
        return {"loss": loss, "hard": hard, "kl": kl, "alpha": d.desc.alpha, "temperature": d.desc.temperature}

    # ----------------------------------------------------------- held out
    def eval_step(self, img, caption_token, weights="model"):
        """The loss of one held-out batch without an optimizer step (not in the
        reference): the model in inference mode, nothing written. Returns the
        device tensors of TrainEngine.eval_step: "loss" (comparable with
        train_loss at the same label_smoothing), per caption "caption_logp",
        "caption_len", "caption_hit", and "totals" (3,) f64. weights="ema":
        on the averaged weights (Pipeline(ema_decay=...))."""
        with self._weights(weights):
            return self.engine.eval_step(img, caption_token)

    def validate(self, batches, weights="model"):
        """Held-out loss over an iterable of (img, caption_token) batches, of
        any shapes (a short last batch runs eagerly, as in train_step). The
        sums of log-probability, tokens and arg-max hits accumulate on the
        device; one read-back at the end. Returns fpnmt.evalstats.summarize's
        dict: "token_nll", "perplexity" = exp(token_nll), "token_accuracy",
        "tokens", "captions", "totals". Under data parallelism every rank
        validates its shard; the totals are plain sums and add. An empty
        iterable raises ValueError. weights="ema": on the averaged weights,
        exchanged once around the whole loop."""
        from fpnmt.evalstats import summarize
        eng = self.engine
        eng.reset_eval_totals()
        captions = 0
        with self._weights(weights):
            for img, tok in batches:
                eng.eval_step(img, tok, accumulate=True)
                captions += int(tok.shape[0])
        if captions == 0:
            raise ValueError("validate: no batches")
        return summarize(eng.eval_totals.cpu().tolist(), captions)

    def score_captions(self, images, captions, n_per_image=1, weights="model"):
        """Teacher-forced log-probabilities of given captions: images
        (B, H, W, 3) on the GPU, captions B * n_per_image token-id lists
        without <start> / <end>, image-major. Returns per caption
        (log_probability, length), the final <end> counted: the score
        convention of predict_batch's mode="beam" (length_alpha 0) and
        mode="sample", so n-best lists and external captions can be reranked
        with it. A caption of more than max_seq_len - 1 tokens raises
        ValueError. weights="ema": scored by the averaged weights."""
        from fpnmt.scst import pack_tokens
        caps = [[int(t) for t in c] for c in captions]
        n = int(n_per_image)
        if n < 1 or len(caps) != images.shape[0] * n:
            raise ValueError(f"score_captions: {len(caps)} captions for {images.shape[0]} images x {n_per_image}")
        T = self.max_seq_len
        long = [i for i, c in enumerate(caps) if len(c) > T - 1]
        if long:
            raise ValueError(f"score_captions: caption {long[0]} has {len(caps[long[0]])} tokens, "
                             f"more than max_seq_len - 1 = {T - 1}")
        # <start> ids <end> 0...: T + 1 columns, so that a caption of T - 1 tokens keeps its <end>
        tok = torch.from_numpy(pack_tokens(caps, T + 1, self.start_token, self.end_token, T)).to(images.device)
        with self._weights(weights):
            out = self.engine.eval_step(images, tok, n_per_image=n)
            logp, ln = out["caption_logp"].cpu().tolist(), out["caption_len"].cpu().tolist()
        return list(zip(logp, ln))

    # ------------------------------------------------------------ predict
    @torch.no_grad()
    def predict(self, img, max_seq_len, plot_layer=False, weights="model", ensemble=(), ensemble_mode="prob",
                ensemble_weights=None):
        """Reference beam procedure (pipeline.py:82-154) for one image (h, w, 3):
        BEAM_SEARCH_N beams through the HIP decode path (fpnmt.decode.
        BeamDecoder: K/V cache, on-device softmax / top-k / beam bookkeeping,
        one hipGraph per step, no host round trip per token). Returns
        (token ids without <start> / <end> (int32, on the image's device),
        attention weights). The attention-weight dict of the reference's last
        decoder call (pipeline.py:109, kept for plot_attention_weights) is
        recomputed only when plot_layer is set: one transformer call on the
        identical beams' final prefix (the main model's weights only, also
        under an ensemble); None otherwise. ensemble, ensemble_mode,
        ensemble_weights: as in predict_batch (the greedy decode from the
        combined distribution)."""
        if weights != "model":
            with self._weights(weights):
                return self.predict(img, max_seq_len, plot_layer, ensemble=ensemble, ensemble_mode=ensemble_mode,
                                    ensemble_weights=ensemble_weights)
        ids = self.predict_batch(img[None], max_seq_len, beam_n=BEAM_SEARCH_N, ensemble=ensemble,
                                 ensemble_mode=ensemble_mode, ensemble_weights=ensemble_weights)[0]
        out = torch.tensor(ids, dtype=torch.int32, device=img.device)
        attention_weights = None
        if plot_layer:
            tr = self.transformer
            enc = tr.encoder(img[None], False, None).repeat(BEAM_SEARCH_N, 1, 1)
            # the last call's input: <start> + every token but the final one
            ended = len(ids) < max_seq_len
            prefix = [self.start_token] + (ids if ended else ids[:-1])
            seq = torch.tensor([prefix] * BEAM_SEARCH_N, dtype=torch.int32, device=enc.device)
            _, attention_weights = tr(enc, seq, False, create_look_ahead_mask(seq.shape[1], device=enc.device))
        return out, attention_weights

    @torch.no_grad()
    def predict_batch(self, images, max_seq_len=None, beam_n=BEAM_SEARCH_N, use_graph=True, mode="reference",
                      length_alpha=0.0, n_best=1, n_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=None,
                      no_repeat_ngram=0, repetition_penalty=1.0, min_len=0, banned_tokens=(), weights="model",
                      ensemble=(), ensemble_mode="prob", ensemble_weights=None, beam_groups=1, diversity_penalty=0.0,
                      group_best=False, consensus=None, consensus_weights="uniform", consensus_all=False):
        """predict() for a batch of images (n, h, w, 3) at once: the same
        beam procedure per image (pipeline.py:82-154), with a K/V cache and a
        hipGraph per decode step (fpnmt.decode.BeamDecoder). Returns one
        token-id list per image.

        mode="beam" (not in the reference, whose beams never part) runs a
        beam search proper on the same machinery: beams scored by their sum
        of log-probabilities, finished beams kept, the result ranked by
        score / len^length_alpha. n_best > 1 then returns, per image, the
        n_best (token-id list, score) pairs, best first.

        beam_groups=G > 1 (mode="beam" only; G divides beam_n) makes it a
        diverse beam search: the beams are G groups of beam_n / G, ranked in
        group order at every position on the device
        (fpnmt_beam_step_groups); a group's candidate for a token loses
        diversity_penalty (>= 0; > 0 needs G > 1) for every live beam of an
        earlier group that took that token at that position. Scores stay
        unpenalised log-probability sums, comparable with score_captions.
        n_best ranks all beam_n beams as ever; group_best=True (with
        n_best=1) returns, per image, G (token-id list, score) pairs in
        group order, each the best of its group by score / len^length_alpha.
        mode="sample" and mode="reference" raise ValueError with any of the
        three set.

        mode="sample" draws n_samples captions per image from the model
        (fpnmt.decode.SampleDecoder: temperature, top_k (0: off), top_p (1:
        off); seed None: a counter per decoder, a given seed repeats its
        draws) and returns, per image, n_samples (token-id list,
        log-probability) pairs in sample order; beam_n, length_alpha and
        n_best do not apply.

        Constraints, for mode="beam" and mode="sample" (mode="reference" is
        the reference's own procedure and raises ValueError with any of them
        on), applied on the device inside the step (fpnmt_logits_constrain):
        no_repeat_ngram=g > 0 never lets a g-gram of <start> + caption occur
        twice; repetition_penalty=p != 1 divides a positive logit of a token
        already in the caption by p and multiplies a negative one, once per
        token; min_len keeps <end> out until the caption has min_len tokens;
        banned_tokens are never emitted. The returned scores are then
        log-probabilities under the constrained, renormalised distribution,
        and in sample mode the constraints come before temperature, top_k
        and top_p.

        weights="ema" decodes on the averaged weights (Pipeline(ema_decay=
        ...)); the decoders and their graphs are the ones weights="model"
        uses.

        ensemble (all three modes): further models, Transformers or
        Pipelines (their .transformer), that decode jointly with this one on
        the device, at most fpnmt._lib.ENSEMBLE_MAX models in all; they may
        differ in depth, width, heads and backbone and must share the
        vocabulary and the device. Every position runs each member's decoder
        on the shared tokens and one fpnmt_logits_ensemble folds their logits
        rows: ensemble_mode "prob" into the log of the weighted mean of their
        distributions, "logprob" into the weighted mean of their
        log-probabilities (renormalised by the step). ensemble_weights: one
        positive number per model, this pipeline's first, normalised to sum
        1 (None: equal). Constraints apply to the combined row, and scores
        are log-probabilities under the combined (constrained) distribution;
        mode="reference" decodes greedily from it. ensemble_mode or
        ensemble_weights with an empty ensemble raise ValueError. The
        decoder keeps its members alive. weights="ema" exchanges this
        pipeline's model only, never a member; a model and its own average
        share storage, so to ensemble the two, export_ema the average and
        load_member it.

        consensus (mode="beam" and mode="sample"): a
        fpnmt.cider_device.DeviceCiderD on the images' device makes the
        decode a consensus (minimum-Bayes-risk) decode under CIDEr-D, the
        self-critical reward: per image the candidate (of the beam_n beams or
        the n_samples draws) that agrees most with the others,
        util(s) = sum_{j != s} p_j sim(c_s, c_j) / sum_{j != s} p_j with
        sim the CIDEr-D of c_s against c_j as its only reference under the
        tables' idf, scored and picked on the device
        (fpnmt_ciderd_consensus) before the decode's one read-back. Returns
        one token-id list per image; consensus_all=True returns, per image,
        every candidate as (token-id list, score, utility) by utility
        descending, then index, the scores exactly those of the call without
        consensus (n_best=beam_n / the samples). consensus_weights:
        "uniform" (p = 1) or "posterior" (p = the fp64 softmax per image of
        those scores). The three are post-processing of a decode: decoders,
        their cache keys and graphs are the ones the call without them uses,
        and weights="ema" and ensemble apply as ever. ValueError:
        mode="reference", n_best > 1 or group_best with consensus;
        consensus_weights or consensus_all without it; tables on another
        device (or built for the host only); max_seq_len above the tables'
        max_len; more than fpnmt._lib.CONSENSUS_MAX_CANDS candidates, or
        candidates whose n-gram keys exceed one work-group's LDS
        (DeviceCiderD.consensus_lds_bytes)."""
        if weights != "model":
            with self._weights(weights):
                return self.predict_batch(images, max_seq_len, beam_n, use_graph, mode, length_alpha, n_best,
                                          n_samples, temperature, top_k, top_p, seed, no_repeat_ngram,
                                          repetition_penalty, min_len, banned_tokens, ensemble=ensemble,
                                          ensemble_mode=ensemble_mode, ensemble_weights=ensemble_weights,
                                          beam_groups=beam_groups, diversity_penalty=diversity_penalty,
                                          group_best=group_best, consensus=consensus,
                                          consensus_weights=consensus_weights, consensus_all=consensus_all)
        from fpnmt.decode import BeamDecoder, SampleDecoder, beam_groups_validated, consensus_validated
        T = max_seq_len or self.max_seq_len
        # checked before a decoder is built; they go to decode(), never into a decoder's key
        cons_kw = {}
        if consensus_validated(mode, consensus, consensus_weights, consensus_all,
                               n_samples if mode == "sample" else beam_n, T, getattr(images, "device", None),
                               n_best, group_best):
            cons_kw = dict(consensus=consensus, consensus_weights=consensus_weights, consensus_all=consensus_all)
        try:
            banned = tuple(sorted({int(b) for b in banned_tokens}))
        except (TypeError, ValueError):
            raise ValueError(f"banned_tokens must be a sequence of token ids, got {banned_tokens!r}") from None
        cons = dict(no_repeat_ngram=no_repeat_ngram, repetition_penalty=repetition_penalty, min_len=min_len,
                    banned_tokens=banned)
        ckey = (no_repeat_ngram, repetition_penalty, min_len, banned)
        members = tuple(getattr(m, "transformer", m) for m in ensemble)
        ens = dict(ensemble=members, ensemble_mode=ensemble_mode, ensemble_weights=ensemble_weights)
        ekey = ()
        if not members and (ensemble_mode != "prob" or ensemble_weights is not None):
            # checked here too: a decoder cached under the plain key would not see the arguments
            raise ValueError(f"ensemble_mode={ensemble_mode!r} / ensemble_weights={ensemble_weights!r} given with "
                             "an empty ensemble")
        if members:  # without members every decoder keeps the key it always had
            from fpnmt.decode import ensemble_weights_normalised
            ekey = ("ensemble", tuple(id(m) for m in members), ensemble_mode,
                    ensemble_weights_normalised(1 + len(members), ensemble_weights))
        # checked here too: mode="sample" builds no BeamDecoder, and a cached decoder would not see the arguments
        groups, lam = beam_groups_validated(mode, beam_n, beam_groups, diversity_penalty)
        if group_best and mode != "beam":
            raise ValueError(f"group_best needs mode='beam', got mode={mode!r}")
        if mode == "sample":
            key = (images.shape[0], n_samples, T, use_graph, mode, float(temperature), top_k, float(top_p)) + ckey
            key += ekey
            dec = getattr(self, "_decoders", {}).get(key)
            if dec is None:
                dec = SampleDecoder(self.transformer, images.shape[0], n_samples, T, self.start_token, self.end_token,
                                    use_graph=use_graph, temperature=temperature, top_k=top_k, top_p=top_p, **cons,
                                    **ens)
                self.__dict__.setdefault("_decoders", {})[key] = dec
            return dec.decode(images, seed=seed, **cons_kw)
        key = (images.shape[0], beam_n, T, use_graph, mode, float(length_alpha))
        if ckey != (0, 1.0, 0, ()):  # an unconstrained decoder keeps the key it always had
            key += ckey
        key += ekey
        if (groups, lam) != (1, 0.0):  # a plain beam search keeps the key it always had
            key += ("groups", groups, lam)
        dec = getattr(self, "_decoders", {}).get(key)
        if dec is None:
            dec = BeamDecoder(self.transformer, images.shape[0], beam_n, T, self.start_token, self.end_token,
                              use_graph=use_graph, mode=mode, length_alpha=length_alpha, beam_groups=groups,
                              diversity_penalty=lam, **cons, **ens)
            self.__dict__.setdefault("_decoders", {})[key] = dec
        return dec.decode(images, n_best=n_best, group_best=group_best, **cons_kw)

    def consensus_captions(self, captions_per_image, tables, weights=None):
        """Consensus selection among externally supplied candidates (the
        union of several decodes, say): captions_per_image[i] are image i's
        candidate token-id lists, the same number n for every image; tables
        a fpnmt.cider_device.DeviceCiderD on the GPU; weights None (uniform)
        or per image n non-negative numbers. The candidates are packed on
        the host into the sampler's layout (<start>, the tokens; len = their
        number, fin = 0) and scored by one fpnmt_ciderd_consensus. Returns
        (pick, util): per image the index of the caption of greatest
        utility (ties to the lowest), and per image its n utilities
        (predict_batch states the definition)."""
        import numpy as np
        caps = [[[int(t) for t in c] for c in cs] for cs in captions_per_image]
        b = len(caps)
        if b == 0:
            return [], []
        n = len(caps[0])
        if any(len(cs) != n for cs in caps):
            raise ValueError(f"consensus_captions: every image needs the same number of candidates, got "
                             f"{sorted({len(cs) for cs in caps})}")
        longest = max([len(c) for cs in caps for c in cs] + [1])
        if not hasattr(tables, "consensus_check"):
            raise ValueError(f"consensus_captions: tables must be a fpnmt.cider_device.DeviceCiderD, got "
                             f"{type(tables).__name__}")
        tables.consensus_check(n, longest)
        w = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != (b, n) or not np.all(w >= 0.0):
                raise ValueError(f"consensus_captions: weights must be {b} x {n} non-negative numbers")
        hist = np.zeros((b * n, longest + 1), dtype=np.int32)
        hist[:, 0] = self.start_token
        lens = np.zeros(b * n, dtype=np.int32)
        for r, c in enumerate(c for cs in caps for c in cs):
            hist[r, 1:1 + len(c)] = c
            lens[r] = len(c)
        dev = tables.device
        hist, lens = torch.from_numpy(hist).to(dev), torch.from_numpy(lens).to(dev)
        util = torch.zeros(b * n, dtype=torch.float64, device=dev)
        pick = torch.zeros(b, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            tables.consensus(hist, lens, torch.zeros_like(lens), n, util, pick,
                             weight=None if w is None else torch.from_numpy(w.reshape(-1)).to(dev))
        return pick.tolist(), util.view(b, n).tolist()

    def load_member(self, path, n_layers=None, backbone=None, rate=0.0):
        """A model-only checkpoint (ckpt.write / ckpt.export_ema of any
        pipeline with this vocabulary) as an ensemble member: a bare
        Transformer with this pipeline's vocabulary, max_seq_len and image
        size, on this pipeline's device, restored with
        Checkpoint(transformer).restore(path). n_layers / backbone not given:
        this pipeline's. No TrainEngine and no optimizer state are created;
        restore prepares the compute copies. Pass the result in
        predict_batch(..., ensemble=[member])."""
        arch = self._arch
        if n_layers is None:
            n_layers = arch["n_layers"]
        if backbone is None:
            backbone = arch["backbone"]
        dev = self.transformer.final_layer.kernel.device
        member = Transformer(n_layers, d_model, num_heads, dff, arch["input_vocab_size"], self.target_vocab_size,
                             rate, max_seq_len=self.max_seq_len, backbone=backbone).to(dev)
        Checkpoint(transformer=member).restore(path)
        return member

    def evaluate(self, generator, max_seq_len, weights="model", ensemble=(), ensemble_mode="prob",
                 ensemble_weights=None):
        """pipeline.py:156-175: caption every (img, imgId) of the generator ->
        [{'image_id', 'caption'}] (the MetricEval results format).
        weights="ema": on the averaged weights, exchanged once around the loop.
        ensemble, ensemble_mode, ensemble_weights: as in predict_batch."""
        results = []
        with self._weights(weights):
            for img, img_id in generator:
                result = self.predict(img, max_seq_len, ensemble=ensemble, ensemble_mode=ensemble_mode,
                                      ensemble_weights=ensemble_weights)[0]
                results.append({"image_id": img_id, "caption": self._to_text(result)})
        return results

    def evaluate_img(self, img, max_seq_len, ensemble=(), ensemble_mode="prob", ensemble_weights=None):
        """pipeline.py:177-193. ensemble, ensemble_mode, ensemble_weights: as
        in predict_batch."""
        result = self.predict(img, max_seq_len, ensemble=ensemble, ensemble_mode=ensemble_mode,
                              ensemble_weights=ensemble_weights)[0]
        return [{"image_id": 0, "caption": self._to_text(result)}]

    def _to_text(self, ids):
        if self.tokenizer is None:
            raise ValueError("Pipeline(tokenizer_filename=...) is needed to turn token ids into text")
        return self.tokenizer.sequences_to_texts([[int(t) for t in ids]])[0]

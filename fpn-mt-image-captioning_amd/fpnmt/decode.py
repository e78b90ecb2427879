"""Batched caption decoding: the reference's beam procedure
(utils/pipeline.py:82-154, `Pipeline.predict`) for many images at once with a
K/V cache and one hipGraph per decode step (BASELINE config C5).

Reference semantics kept:
  * every step re-runs the decoder on the beams' sequences; here only the
    newest position is computed — keys/values of earlier positions are
    cached (the causal mask makes them independent of later tokens), and the
    last row of the look-ahead mask keeps every earlier position;
  * beams start identical ([<start>], prob 1); per step softmax of the last
    position, candidates p * beam_prob flattened over beam_n x V, top_k
    (ties to the lower flat index), parents / tokens by // and %, beam_prob =
    the top-k values (a product of probabilities, not logs);
  * the result is the best beam (first argmax of beam_prob) after <start>,
    without <end> when it ends with <end> — per image, frozen at the step the
    reference would `return` (fpnmt_beam_step status flag).
Beams re-rank without moving the cache: every row keeps a table of the cache
rows holding its history's keys/values (fpnmt_decode_attention `src`).

Not reproduced on this path: the attention-weight dict of the last step (the
reference returns it for plotting only).

Those beams never part: they start identical, so top_k picks the same best
token once per beam and the procedure is a greedy decode run beam_n times.
`mode="beam"` keeps the cache, the tables and the graphs and changes the
rule of the step (fpnmt_beam_step_log) and how the result is chosen
(fpnmt_beam_finalize):
  * beams carry a sum of log-probabilities; step 0 starts with beam 0 at 0
    and the others at -inf, so the beams differ from the first token on;
  * a beam that took <end> is finished: it competes with its score as it is
    and is no longer extended; an image stops when all its beams have
    finished (its rows are then frozen while other images decode on);
  * the n-best list ranks the beams by score / len^length_alpha (len counts
    the final <end>; alpha 0: the raw sum), ties to the lower beam.
SampleDecoder draws captions instead (fpnmt_sample_step: temperature, top-k,
nucleus) on the same cache, attention and graphs; its rows never re-rank.

Constrained decoding (mode="beam" and SampleDecoder): no_repeat_ngram,
repetition_penalty, min_len and banned_tokens. With any of them on, a step
calls fpnmt_logits_constrain on the fp32 logits before its step kernel, with
the rows' device-resident history and `fin`, inside the same per-position
graph: a banned token's logit becomes -inf, which both step kernels already
define, and a repeated token's logit is penalised once. Scores are then sums
over the CONSTRAINED logits — beam: score + log_softmax(constrained row);
sample: l_token - logsumexp(constrained l) — the log-probability under the
constrained, renormalised distribution, and in sample mode the constraints
come before temperature, top_k and top_p. With all four at their defaults no
call is made and the graphs are launch for launch what they were.

Ensemble decoding (all modes): `ensemble` names further Transformers that
decode jointly with the main model. What belongs to one model (its geometry,
K/V cache, cross K/V, staged biases) lives in a _Model record and the decoder
holds a list of them, the main model first; tokens, history, cache-row tables,
scores and `fin` stay per decoder, so every member sees the same tokens and
tables. A step then runs every member's _logits one after another on the
current stream, one fpnmt_logits_ensemble that folds the M rows into the
first member's logits buffer ("prob": the log of the weighted mean of the
distributions; "logprob": the weighted mean of the log-probabilities,
renormalised by the step kernel), then the constraints, then the step kernel:
scores are log-probabilities under the combined (and then constrained)
distribution. With an empty `ensemble` the list holds the one model, no call
is made and the graphs are launch for launch what they were.

Diverse beam search (mode="beam", beam_groups=G > 1): the beam_n rows are G
groups of beam_n / G contiguous rows; the last launch of a position is
fpnmt_beam_step_groups instead of fpnmt_beam_step_log, which ranks the groups
in order, each among its own rows, and takes diversity_penalty off a token's
candidates for every live beam of an earlier group that took it at this
position. Scores stay unpenalised log-probability sums; step 0 starts with
each group's first row at 0. With beam_groups=1 the step is
fpnmt_beam_step_log and the graphs are launch for launch what they were.

Consensus decoding (mode="beam" and SampleDecoder; decode(consensus=...)): a
post-processing of one decode, not a property of the decoder. After the
position loop, outside the per-position graphs, one fpnmt_ciderd_consensus
scores an image's beam_n / n_samples candidate rows against each other under
CIDEr-D on the decoder's own hist / len / fin tables and picks the one of
greatest utility; the utilities and picks join the read-back the decode does
anyway. Without `consensus` no launch is added and nothing is allocated.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from ._lib import call, ptr, stream_ptr, dtype_code
from . import compute_dtype


def _gemm(m, n, k, dt, a, lda, b, c, ldc, bias, s):
    g = L.GemmDesc()
    g.m, g.n, g.k, g.batch, g.batch_inner, g.dtype = m, n, k, 1, 1, dt
    g.a_trans, g.b_trans = 0, 0
    g.lda, g.ldb, g.ldc, g.ldr = lda, k, ldc, ldc
    g.alpha, g.act, g.act_alpha, g.accumulate, g.c_f32, g.split_k = 1.0, L.ACT_NONE, 0.0, 0, 0, 1
    call("fpnmt_gemm", g, a, b, c, None, bias, None, s)


ENSEMBLE_MODES = {"prob": 0, "logprob": 1}  # fpnmt_logits_ensemble's mode


def ensemble_weights_normalised(n_models, weights):
    """One weight per model (the main model first) -> the tuple normalised to
    sum 1 in fp64; None: equal weights. ValueError names a bad value."""
    if weights is None:
        return (1.0 / n_models,) * n_models
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError(f"ensemble_weights must be a sequence of numbers, got {weights!r}") from None
    if len(w) != n_models:
        raise ValueError(f"ensemble_weights: {len(w)} weights {weights!r} for {n_models} models (the main model first)")
    for x in w:
        if not (x > 0.0 and math.isfinite(x)):
            raise ValueError(f"ensemble_weights must be finite positive numbers, got {x!r}")
    total = math.fsum(w)
    if not math.isfinite(total):
        raise ValueError(f"ensemble_weights {weights!r}: their sum is not finite")
    return tuple(x / total for x in w)


CONSENSUS_WEIGHTS = ("uniform", "posterior")


def consensus_validated(mode, consensus, consensus_weights="uniform", consensus_all=False, n=1, max_seq_len=1,
                        device=None, n_best=1, group_best=False):
    """The consensus arguments of a decode -> whether a consensus launch
    follows it; ValueError names what does not fit. consensus: None, or the
    DeviceCiderD whose corpus supplies the idf; n candidates per image of up
    to max_seq_len tokens on `device`. Touches no device."""
    if consensus is None:
        if consensus_weights != "uniform" or consensus_all:
            raise ValueError(f"consensus_weights={consensus_weights!r} / consensus_all={consensus_all!r} given "
                             "without consensus= (the DeviceCiderD tables)")
        return False
    if mode not in ("beam", "sample"):
        raise ValueError(f"consensus needs several candidates per image: mode='beam' or mode='sample', got {mode!r}")
    if n_best != 1 or group_best:
        raise ValueError("consensus ranks all candidates itself: it takes neither n_best > 1 nor group_best "
                         "(consensus_all=True returns every candidate)")
    if consensus_weights not in CONSENSUS_WEIGHTS:
        raise ValueError(f"consensus_weights must be one of {CONSENSUS_WEIGHTS}, got {consensus_weights!r}")
    check = getattr(consensus, "consensus_check", None)
    if check is None:
        raise ValueError(f"consensus must be a fpnmt.cider_device.DeviceCiderD, got {type(consensus).__name__}")
    check(n, max_seq_len, device)
    return True


def consensus_ranked(ids, score, util, pick, consensus_all):
    """One image's candidates (token-id lists, scores, utilities in row
    order) -> the chosen ids, or with consensus_all every (ids, score,
    utility) by utility descending, then index."""
    if not consensus_all:
        return ids[pick]
    order = sorted(range(len(ids)), key=lambda r: (-util[r], r))
    return [(ids[r], score[r], util[r]) for r in order]


class _Model:
    """What belongs to ONE model of a decoder: the Transformer, its geometry,
    and (filled by the decoder) its K/V cache `kv`, cross K/V `enc_kv` with
    `Lenc`, and the staged `qkv_bias`."""

    def __init__(self, transformer):
        self.tr = transformer
        dec = transformer.decoder
        self.d = dec.d_model
        self.L = dec.num_layers
        self.heads = dec.dec_layers[0].mha1.num_heads if self.L else 8
        self.depth = self.d // self.heads
        self.kv = self.enc_kv = self.Lenc = None
        self.qkv_bias = []


class _CachedDecoder:
    """What BeamDecoder and SampleDecoder share: the geometry, per model
    (self.models, the one it was given first) the encoder pass with every
    layer's cross K/V, the staged biases, and one decode position through
    embed -> layers -> fp32 logits on the K/V cache; and the fold of several
    models' logits into one row. `beam_n` is the number of rows per image."""

    def __init__(self, transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph=True,
                 ensemble=(), ensemble_mode="prob", ensemble_weights=None):
        self.tr = transformer
        self.n_images, self.beam_n, self.T = n_images, beam_n, max_seq_len
        self.start_token, self.end_token = start_token, end_token
        self.R = n_images * beam_n
        self.V = transformer.final_layer.kernel.shape[1]
        self.models = [_Model(transformer)]
        self._set_ensemble(ensemble, ensemble_mode, ensemble_weights)
        for i, m in enumerate(self.models):
            if max_seq_len > m.tr.decoder.pos_encoding.shape[0]:
                raise ValueError(f"max_seq_len {max_seq_len} exceeds the decoder's positional table"
                                 + (f" (ensemble member {i})" if i else ""))
        self.use_graph = use_graph
        self.dt = None
        self.graphs = None
        self.cons_util = self.cons_pick = None  # allocated by the first consensus launch

    # ----------------------------------------------------------- consensus
    def _consensus(self, tables, weights, hist, lens, fin, score):
        """One fpnmt_ciderd_consensus over the decoder's own state (beam_n
        candidate rows per image), after the position loop and outside its
        graphs. "posterior": the candidates weigh softmax(score) per image,
        in fp64, computed by torch on the device (a dead beam's -inf gives
        0); "uniform" passes no weights. Returns the device tensors util
        (R,) f64 and pick (n_images,) int32."""
        if self.cons_util is None:
            self.cons_util = torch.zeros(self.R, dtype=torch.float64, device=hist.device)
            self.cons_pick = torch.zeros(self.n_images, dtype=torch.int32, device=hist.device)
        w = None
        if weights == "posterior":
            w = torch.softmax(score.double().view(self.n_images, self.beam_n), dim=1).reshape(-1).contiguous()
        return tables.consensus(hist, lens, fin, self.beam_n, self.cons_util, self.cons_pick, weight=w)

    # ------------------------------------------------------------ ensemble
    def _set_ensemble(self, ensemble, mode, weights):
        """Validates the members, the mode and the weights; self.models gains
        a record per member (the decoder holds them strongly)."""
        members = tuple(ensemble)
        if not members:
            if mode != "prob" or weights is not None:
                raise ValueError(f"ensemble_mode={mode!r} / ensemble_weights={weights!r} given with an empty ensemble")
            self.ens_mode = self.ens_weights = None
            return
        if mode not in ENSEMBLE_MODES:
            raise ValueError(f"ensemble_mode must be 'prob' or 'logprob', got {mode!r}")
        n = 1 + len(members)
        if n > L.ENSEMBLE_MAX:
            raise ValueError(f"an ensemble holds at most {L.ENSEMBLE_MAX} models, got {n} (the main model and "
                             f"{len(members)} members)")
        dev = self.tr.final_layer.kernel.device
        for i, tr in enumerate(members):
            k = getattr(getattr(tr, "final_layer", None), "kernel", None)
            if k is None:
                raise ValueError(f"ensemble member {i + 1} is not a Transformer: {tr!r}")
            if k.shape[1] != self.V:
                raise ValueError(f"ensemble member {i + 1} has vocabulary {k.shape[1]}, the main model {self.V}")
            if k.device != dev:
                raise ValueError(f"ensemble member {i + 1} is on {k.device}, the main model on {dev}")
        self.ens_weights = ensemble_weights_normalised(n, weights)
        self.ens_mode = mode
        self.models += [_Model(tr) for tr in members]

    def _combine(self, logits):
        """The members' fp32 logits (R, V), in self.models' order, folded into
        the first one's buffer (fpnmt_logits_ensemble); finished rows, where
        the decoder has a `fin`, are left alone."""
        import ctypes as C
        n = len(logits)
        fin = getattr(self, "fin", None)  # mode="reference" has none: every row is combined
        call("fpnmt_logits_ensemble", self.R, self.V, n, (C.c_void_p * n)(*[ptr(x) for x in logits]),
             (C.c_longlong * n)(*[self.V] * n), (C.c_float * n)(*self.ens_weights), ENSEMBLE_MODES[self.ens_mode],
             ptr(fin), ptr(logits[0]), self.V, stream_ptr())
        return logits[0]

    def _all_logits(self, t, src):
        """Position t's logits row per decode row: the one model's, or the
        fold of every member's."""
        if len(self.models) == 1:
            return self._logits(self.models[0], t, src)
        return self._combine([self._logits(m, t, src) for m in self.models])

    # --------------------------------------------------------- constraints
    def _set_constraints(self, no_repeat_ngram, repetition_penalty, min_len, banned_tokens, need):
        """Validates and stores the four constraints (include/fpnmt.h,
        fpnmt_logits_constrain). need: the finite candidates a row must keep
        whatever the rules ban (beam_n for a beam search, 1 for a draw)."""
        if isinstance(no_repeat_ngram, bool) or int(no_repeat_ngram) != no_repeat_ngram or no_repeat_ngram < 0:
            raise ValueError(f"no_repeat_ngram must be an integer >= 0 (0: off), got {no_repeat_ngram!r}")
        if not (repetition_penalty > 0.0 and math.isfinite(repetition_penalty)):
            raise ValueError(f"repetition_penalty must be a finite positive number, got {repetition_penalty!r}")
        if int(min_len) != min_len or not 0 <= min_len < self.T:
            raise ValueError(f"min_len must be an integer in [0, max_seq_len = {self.T}), got {min_len!r}")
        banned = sorted({int(b) for b in banned_tokens})
        for b in banned:
            if not 0 <= b < self.V or b == self.end_token:
                raise ValueError(f"banned token {b}: outside [0, {self.V}) or the end token {self.end_token}")
        self.no_repeat_ngram, self.repetition_penalty = int(no_repeat_ngram), float(repetition_penalty)
        self.min_len, self.banned_tokens = int(min_len), tuple(banned)
        self.constrained = bool(self.no_repeat_ngram or self.repetition_penalty != 1.0 or self.min_len or banned)
        self.banned_dev = None
        if not self.constrained:
            return
        if self.T > L.CONSTRAIN_MAX_LEN:
            raise ValueError(f"constrained decoding stages at most {L.CONSTRAIN_MAX_LEN} positions, "
                             f"max_seq_len is {self.T}")
        if len(banned) > L.CONSTRAIN_MAX_BANNED:
            raise ValueError(f"at most {L.CONSTRAIN_MAX_BANNED} banned tokens, got {len(banned)}")
        # the most the rules can ban in one row: every history token, the list, <end>
        if self.V - (self.T + 1 + len(banned)) < need:
            raise ValueError(f"vocabulary {self.V} too small: the constraints can ban {self.T + 1 + len(banned)} "
                             f"tokens of a row and {need} must stay")
        if banned:  # built once; the step graphs read it by address
            self.banned_dev = torch.tensor(banned, dtype=torch.int32,
                                           device=self.tr.final_layer.kernel.device)

    def _constrain(self, logits, hist, t):
        """The constraints on the logits of position t, in place, from the
        rows' history table (fpnmt_logits_constrain); finished rows are left
        alone."""
        call("fpnmt_logits_constrain", self.R, self.V, ptr(logits), self.V, ptr(hist), self.T + 1, t, ptr(self.fin),
             self.no_repeat_ngram, self.repetition_penalty, self.min_len, self.end_token, ptr(self.banned_dev),
             len(self.banned_tokens), stream_ptr())

    def _alloc_cache(self, dev):
        for m in self.models:
            m.kv = torch.empty((max(m.L, 1), self.R, self.T, 2 * m.d), dtype=self.dt, device=dev)
        self.tok = torch.empty(self.R, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------- encoder
    def _encode(self, m, images):
        """Encoder of model m once per image (pipeline.py:93-94) and every
        layer's cross K/V from one grouped GEMM (no per-beam tiling: the
        attention maps beam rows to their image)."""
        tr, dec = m.tr, m.tr.decoder
        enc = tr.encoder(images, False, None)  # (n, Lenc, d)
        m.Lenc = enc.shape[1]
        n = enc.shape[0]
        if m.L == 0:
            m.enc_kv = torch.empty((1, 1), dtype=self.dt, device=enc.device)
            return
        grp = dec.cross_kv_group
        stack, _ = grp.stacked(self.dt)
        cols = grp.n * grp.fout  # 2 * L * d
        shape = (n * m.Lenc, cols)
        if m.enc_kv is None or tuple(m.enc_kv.shape) != shape:
            # static buffer: the captured step graphs read it by address
            m.enc_kv = torch.empty(shape, dtype=self.dt, device=enc.device)
            self.graphs = None
        e2 = enc.reshape(n * m.Lenc, m.d).contiguous()
        _gemm(n * m.Lenc, cols, m.d, dtype_code(self.dt), ptr(e2), m.d, ptr(stack), ptr(m.enc_kv), cols,
              ptr(grp.bias_cat()), stream_ptr())

    def _stage_biases(self, m, dev):
        """Each layer's [q|k|v] bias of model m as one vector the step graphs
        read by address: a view when the biases are adjacent (arena order),
        else a static buffer refreshed here, once per decode call, instead of
        a concatenation per layer inside every step."""
        dec = m.tr.decoder
        if len(m.qkv_bias) != m.L:
            m.qkv_bias = [None] * m.L
        for i, lay in enumerate(dec.dec_layers):
            b = lay.qkv_group.bias_cat()
            cur = m.qkv_bias[i]
            if b._base is not None or b.numel() == 0:  # a view of the parameters
                if cur is None or cur.data_ptr() != b.data_ptr():
                    m.qkv_bias[i] = b
                    self.graphs = None
                continue
            if cur is None or cur.shape != b.shape or cur._base is not None:
                m.qkv_bias[i] = torch.empty_like(b, device=dev)
                self.graphs = None
            m.qkv_bias[i].copy_(b)

    def _prepare(self, images):
        """Before the first position of a decode call: buffers for the
        compute dtype, every model's encoder side, the state reset, the step
        graphs."""
        dt = compute_dtype()
        if self.dt != dt:
            self.dt = dt
            self._alloc(images.device)
            for m in self.models:
                m.enc_kv = None
            self.graphs = None
        for m in self.models:
            self._encode(m, images)
            self._stage_biases(m, images.device)
        self._reset()
        if self.use_graph and self.graphs is None:
            self._capture()

    # ------------------------------------------------------------ position
    def _logits(self, m, t, src):
        """Position t of every row through model m: embed self.tok, the
        decoder layers on m's K/V cache, the fp32 logits (R, V). src: the
        rows' cache-row tables (None: every row reads its own cache row)."""
        tr, dec = m.tr, m.tr.decoder
        dt, code, R, T, d = self.dt, dtype_code(self.dt), self.R, self.T, m.d
        s = stream_ptr()
        x = torch.empty((R, d), dtype=dt, device=self.tok.device)
        pe = dec.pos_encoding
        call("fpnmt_embed_posenc_fwd", code, R, 1, d, ptr(self.tok), ptr(dec.embedding.embeddings),
             pe.data_ptr() + t * d * pe.element_size(), ptr(x), s)
        scale = 1.0 / math.sqrt(float(m.depth))
        for i, lay in enumerate(dec.dec_layers):
            grp = lay.qkv_group
            stack, _ = grp.stacked(dt)
            bias = m.qkv_bias[i]
            q = torch.empty((R, d), dtype=dt, device=x.device)
            _gemm(R, d, d, code, ptr(x), d, ptr(stack), ptr(q), d, ptr(bias), s)
            kvl = m.kv[i]
            # this position's key / value straight into the cache (row r, position t)
            _gemm(R, 2 * d, d, code, ptr(x), d, stack.data_ptr() + d * d * stack.element_size(),
                  kvl.data_ptr() + t * 2 * d * kvl.element_size(), T * 2 * d,
                  bias.data_ptr() + d * bias.element_size(), s)
            a = torch.empty((R, d), dtype=dt, device=x.device)
            call("fpnmt_decode_attention", code, R, m.heads, m.depth, t + 1, scale, ptr(q), d, ptr(kvl),
                 T * 2 * d, 2 * d, 0, d, ptr(src), T, 1, ptr(a), d, s)
            out1 = lay.layernorm1(lay.mha1.dense(a), residual=x)
            q2 = lay.mha2.wq(out1)
            a2 = torch.empty((R, d), dtype=dt, device=x.device)
            cols = 2 * m.L * d
            call("fpnmt_decode_attention", code, R, m.heads, m.depth, m.Lenc, scale, ptr(q2), d,
                 ptr(m.enc_kv), m.Lenc * cols, cols, 2 * i * d, 2 * i * d + d, None, 0, self.beam_n, ptr(a2),
                 d, s)
            out2 = lay.layernorm2(lay.mha2.dense(a2), residual=out1)
            x = lay.layernorm3(lay.ffn2(lay.ffn1(out2)), residual=out2)
        return tr.final_layer(x)  # (R, V) fp32

    def _capture(self):
        """One graph per position t (the step's shapes depend on t). The
        first step runs eagerly to build compute copies / workspaces; the
        state it advances is reset before the graphs are replayed."""
        from .train import capture_sequence
        self._step(0)
        torch.cuda.synchronize()
        graphs = capture_sequence([(lambda t=t: self._step(t)) for t in range(self.T)])
        self.graphs = graphs
        self._reset()


def beam_groups_validated(mode, beam_n, beam_groups=1, diversity_penalty=0.0):
    """(beam_groups, diversity_penalty) as (int, float), or ValueError: the
    groups are for mode="beam", divide beam_n, and a penalty is finite,
    >= 0 and needs more than one group to act on."""
    if isinstance(beam_groups, bool) or not isinstance(beam_groups, int):
        raise ValueError(f"beam_groups must be an int, got {beam_groups!r}")
    try:
        lam = float(diversity_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"diversity_penalty must be a number, got {diversity_penalty!r}") from None
    if mode != "beam" and (beam_groups != 1 or lam != 0.0):
        raise ValueError(f"beam_groups / diversity_penalty need mode='beam', got mode={mode!r}")
    if beam_groups < 1 or beam_n % beam_groups != 0:
        raise ValueError(f"beam_groups {beam_groups} must be >= 1 and divide beam_n {beam_n}")
    if not (lam >= 0.0) or lam == float("inf"):
        raise ValueError(f"diversity_penalty must be finite and >= 0, got {diversity_penalty!r}")
    if lam > 0.0 and beam_groups == 1:
        raise ValueError("diversity_penalty > 0 needs beam_groups > 1: one group has no earlier group to differ from")
    return beam_groups, lam


class BeamDecoder(_CachedDecoder):
    """decode(images) -> list of token-id lists, one per image; in
    mode="beam", decode(images, n_best=k) -> per image the k best
    (token ids, score) pairs, best first.

    mode="beam" takes the constraints no_repeat_ngram (0: off),
    repetition_penalty (1: off), min_len (0: off) and banned_tokens: every
    live beam's logits row is constrained before the step ranks it, so a
    beam's score is the sum of log_softmax over the constrained rows — its
    log-probability under the constrained, renormalised distribution.
    mode="reference" is the reference's own procedure and takes none.

    beam_groups=G > 1 (mode="beam") is diverse beam search: the beam_n rows
    are G groups of beam_n / G rows, ranked in group order at every position
    (fpnmt_beam_step_groups); a group's candidate for a token loses
    diversity_penalty for every live beam of an earlier group that took the
    token at this position, and only the group's own beams compete for its
    rows. Scores stay unpenalised log-probability sums. decode(...,
    group_best=True) returns each group's best (token ids, score) in group
    order; n_best ranks all beam_n beams as ever. beam_groups=1 is the plain
    search, launch for launch.

    ensemble: further Transformers that decode jointly with `transformer`
    (at most ENSEMBLE_MAX models in all; any depth, width, heads and
    backbone, the same vocabulary, device and a positional table that holds
    max_seq_len). ensemble_mode "prob" (the default) ranks by the weighted
    mean of the models' distributions, "logprob" by the renormalised weighted
    mean of their log-probabilities; ensemble_weights: one positive number
    per model, the main model first, normalised here (None: equal). Both
    modes take an ensemble: "reference" then decodes greedily from the
    combined distribution. The constraints come after the combine. A member
    is another Transformer object and is NOT exchanged by weights="ema"; only
    the main model is, and it shares storage with its own average: to
    ensemble a model with its average, export_ema the average and load it as
    a member (Pipeline.load_member)."""

    def __init__(self, transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph=True,
                 mode="reference", length_alpha=0.0, no_repeat_ngram=0, repetition_penalty=1.0, min_len=0,
                 banned_tokens=(), ensemble=(), ensemble_mode="prob", ensemble_weights=None, beam_groups=1,
                 diversity_penalty=0.0):
        if mode not in ("reference", "beam"):
            raise ValueError(f"mode must be 'reference' or 'beam', got {mode!r}")
        self.mode, self.length_alpha = mode, float(length_alpha)
        self.beam_groups, self.diversity_penalty = beam_groups_validated(mode, beam_n, beam_groups, diversity_penalty)
        super().__init__(transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph,
                         ensemble, ensemble_mode, ensemble_weights)
        self._set_constraints(no_repeat_ngram, repetition_penalty, min_len, banned_tokens, beam_n)
        if self.constrained and mode != "beam":
            raise ValueError("constrained decoding needs mode='beam': mode='reference' is the reference's own procedure")

    # ---------------------------------------------------------- buffers
    def _alloc(self, dev):
        R, T = self.R, self.T
        self._alloc_cache(dev)
        self.hist = [torch.empty((R, T + 1), dtype=torch.int32, device=dev) for _ in range(2)]
        self.src = [torch.empty((R, T), dtype=torch.int32, device=dev) for _ in range(2)]
        self.prob = torch.empty(R, dtype=torch.float32, device=dev)
        self.result = torch.zeros((self.n_images, T), dtype=torch.int32, device=dev)
        self.result_len = torch.zeros(self.n_images, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.n_images, dtype=torch.int32, device=dev)
        if self.mode == "beam":
            n, K = self.n_images, self.beam_n
            self.score = torch.empty(R, dtype=torch.float32, device=dev)
            self.blen = torch.zeros(R, dtype=torch.int32, device=dev)
            self.fin = torch.zeros(R, dtype=torch.int32, device=dev)
            self.nbest_tok = torch.zeros((n, K, T), dtype=torch.int32, device=dev)
            self.nbest_len = torch.zeros((n, K), dtype=torch.int32, device=dev)
            self.nbest_score = torch.zeros((n, K), dtype=torch.float32, device=dev)

    def _reset(self):
        R = self.R
        self.tok.fill_(self.start_token)
        if self.mode == "beam":
            self.score.fill_(float("-inf"))
            # each group's first row starts alone (one group: the image's first row)
            self.score.view(self.n_images * self.beam_groups, self.beam_n // self.beam_groups)[:, 0] = 0.0
            self.blen.zero_()
            self.fin.zero_()
        else:
            self.prob.fill_(1.0)
        self.hist[0][:, 0] = self.start_token
        self.src[0][:, 0] = torch.arange(R, dtype=torch.int32, device=self.tok.device)
        self.result_len.zero_()
        self.status.zero_()

    # ---------------------------------------------------------------- step
    def _step(self, t):
        T = self.T
        s = stream_ptr()
        hin, hout = self.hist[t % 2], self.hist[(t + 1) % 2]
        sin, sout = self.src[t % 2], self.src[(t + 1) % 2]
        logits = self._all_logits(t, sin)
        if self.mode == "beam":
            if self.constrained:
                self._constrain(logits, hin, t)
            if self.beam_groups > 1:
                call("fpnmt_beam_step_groups", self.n_images, self.beam_n, self.beam_groups, self.diversity_penalty,
                     self.V, ptr(logits), self.V, ptr(self.score), ptr(self.blen), ptr(self.fin), ptr(hin), ptr(hout),
                     T + 1, t, ptr(sin), ptr(sout), T, self.end_token, ptr(self.tok), ptr(self.status), s)
                return
            call("fpnmt_beam_step_log", self.n_images, self.beam_n, self.V, ptr(logits), self.V, ptr(self.score),
                 ptr(self.blen), ptr(self.fin), ptr(hin), ptr(hout), T + 1, t, ptr(sin), ptr(sout), T,
                 self.end_token, ptr(self.tok), ptr(self.status), s)
            return
        call("fpnmt_beam_step", self.n_images, self.beam_n, self.V, ptr(logits), self.V, ptr(self.prob), ptr(hin),
             ptr(hout), T + 1, t, ptr(sin), ptr(sout), T, self.end_token, ptr(self.tok), ptr(self.result), T,
             ptr(self.result_len), ptr(self.status), s)

    # -------------------------------------------------------------- decode
    @torch.no_grad()
    def decode(self, images, check_every=8, n_best=1, group_best=False, consensus=None,
               consensus_weights="uniform", consensus_all=False):
        """images (n_images, H, W, 3) on the GPU -> list of token-id lists;
        n_best > 1 (mode="beam"): per image a list of the n_best
        (token-id list, score) pairs, best first, over all beam_n beams;
        group_best (mode="beam"): per image beam_groups (token-id list,
        score) pairs in group order, each its group's best by
        score / len^length_alpha.

        consensus (mode="beam"; a DeviceCiderD on this device): instead of
        the best-scoring beam, per image the beam that agrees most with the
        image's other beams under CIDEr-D with the tables' idf
        (fpnmt_ciderd_consensus, one launch after the position loop on the
        decoder's own tables). consensus_weights "uniform" weighs the beams
        equally, "posterior" by the fp64 softmax per image of the scores
        this decoder returns (score / len^length_alpha). consensus_all: per
        image every beam as (token ids, score, utility), by utility
        descending, then beam index."""
        if group_best and (self.mode != "beam" or n_best != 1):
            raise ValueError("group_best needs mode='beam' and n_best=1: it returns one caption per group")
        if images.shape[0] != self.n_images:
            raise ValueError(f"expected {self.n_images} images, got {images.shape[0]}")
        if n_best < 1 or n_best > (self.beam_n if self.mode == "beam" else 1):
            raise ValueError(f"n_best {n_best}: mode {self.mode!r} with {self.beam_n} beams gives 1.."
                             f"{self.beam_n if self.mode == 'beam' else 1}")
        with_consensus = consensus_validated(self.mode, consensus, consensus_weights, consensus_all, self.beam_n,
                                             self.T, images.device, n_best, group_best)
        self._prepare(images)
        steps = 0
        for t in range(self.T):
            if self.graphs is not None:
                self.graphs[t].replay()
            else:
                self._step(t)
            steps = t + 1
            if check_every and (t + 1) % check_every == 0 and t + 1 < self.T and bool(self.status.all()):
                break
        if with_consensus:
            return self._consensus_result(steps, consensus, consensus_weights, consensus_all)
        if self.mode == "beam":
            return self._nbest(steps, n_best, group_best)
        lens = self.result_len.tolist()
        res = self.result.cpu()
        return [res[i, :lens[i]].tolist() for i in range(self.n_images)]

    def _nbest(self, steps, n_best, group_best=False):
        """Rank the beams of every image (fpnmt_beam_finalize over the tables
        the last step wrote) and read the n-best list back. group_best: the
        same kernel with every group as an image of its own, and the head of
        each group's list."""
        n, K, T = self.n_images, self.beam_n, self.T
        if group_best:
            G = self.beam_groups
            n, K = n * G, K // G
        call("fpnmt_beam_finalize", n, K, ptr(self.hist[steps % 2]), T + 1, ptr(self.score), ptr(self.blen),
             ptr(self.fin), self.length_alpha, ptr(self.nbest_tok), T, ptr(self.nbest_len), ptr(self.nbest_score),
             stream_ptr())
        if group_best:
            tok = self.nbest_tok.view(n, K, T).cpu()
            lens, score = self.nbest_len.view(n, K).tolist(), self.nbest_score.view(n, K).tolist()
            return [[(tok[i * G + g, 0, :lens[i * G + g][0]].tolist(), score[i * G + g][0]) for g in range(G)]
                    for i in range(self.n_images)]
        tok, lens, score = self.nbest_tok.cpu(), self.nbest_len.tolist(), self.nbest_score.tolist()
        if n_best == 1:
            return [tok[i, 0, :lens[i][0]].tolist() for i in range(n)]
        return [[(tok[i, k, :lens[i][k]].tolist(), score[i][k]) for k in range(n_best)] for i in range(n)]

    def _consensus_result(self, steps, tables, weights, consensus_all):
        """The beams in ROW order with the scores n_best would give them
        (fpnmt_beam_finalize with every row an image of one beam: nothing is
        ranked, and the score is that kernel's own arithmetic), the consensus
        launch over the tables the last step wrote, and the one read-back."""
        n, K, T = self.n_images, self.beam_n, self.T
        hist = self.hist[steps % 2]
        call("fpnmt_beam_finalize", n * K, 1, ptr(hist), T + 1, ptr(self.score), ptr(self.blen), ptr(self.fin),
             self.length_alpha, ptr(self.nbest_tok), T, ptr(self.nbest_len), ptr(self.nbest_score), stream_ptr())
        util, pick = self._consensus(tables, weights, hist, self.blen, self.fin, self.nbest_score)
        tok, lens, score = self.nbest_tok.view(n * K, T).cpu(), self.nbest_len.view(-1).tolist(), \
            self.nbest_score.view(-1).tolist()
        util, pick = util.tolist(), pick.tolist()
        out = []
        for i in range(n):
            rows = range(i * K, (i + 1) * K)
            out.append(consensus_ranked([tok[r, :lens[r]].tolist() for r in rows], [score[r] for r in rows],
                                        [util[r] for r in rows], pick[i], consensus_all))
        return out


class SampleDecoder(_CachedDecoder):
    """Draws n_samples captions per image from the model's distribution on
    the machinery of BeamDecoder: the same K/V cache, decode attention and
    per-position graphs; the last launch of a step is fpnmt_sample_step
    (temperature, top-k, nucleus) instead of a ranking. Rows never re-rank,
    so every row reads its own cache row (no src tables) and one history
    table is updated in place. The uniforms are a function of (seed, row,
    position): the seed lives in a device word the graphs read, so replays
    draw new captions without a re-capture.

    decode(images, seed=None) -> per image n_samples pairs (token ids without
    <start> and a final <end>, log-probability under the model at temperature
    1, unfiltered), in sample order.

    no_repeat_ngram (0: off), repetition_penalty (1: off), min_len (0: off)
    and banned_tokens constrain every live row's logits before the draw, and
    so before temperature, top_k and top_p; the returned log-probability is
    then the sum of l_token - logsumexp(constrained l): the one under the
    constrained, renormalised distribution.

    ensemble, ensemble_mode, ensemble_weights: as for BeamDecoder; the draw
    is from the combined distribution (then the constraints, then
    temperature, top_k and top_p) and the log-probability is the one under
    it."""

    def __init__(self, transformer, n_images, n_samples, max_seq_len, start_token, end_token, use_graph=True,
                 temperature=1.0, top_k=0, top_p=1.0, no_repeat_ngram=0, repetition_penalty=1.0, min_len=0,
                 banned_tokens=(), ensemble=(), ensemble_mode="prob", ensemble_weights=None):
        if n_samples < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        if not (temperature > 0.0 and math.isfinite(temperature)):
            raise ValueError(f"temperature must be a finite positive number, got {temperature!r}")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must lie in (0, 1], got {top_p!r}")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0 (0: off), got {top_k!r}")
        if max_seq_len > 65536:
            raise ValueError(f"max_seq_len {max_seq_len}: the draw counter holds positions below 65536")
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        super().__init__(transformer, n_images, n_samples, max_seq_len, start_token, end_token, use_graph,
                         ensemble, ensemble_mode, ensemble_weights)
        filtered = 0 < self.top_k < self.V or self.top_p < 1.0
        if filtered and self.V > L.SAMPLE_FILTER_MAX_VOCAB:
            raise ValueError(f"top_k / top_p need a vocabulary of at most {L.SAMPLE_FILTER_MAX_VOCAB}, got {self.V}")
        self._set_constraints(no_repeat_ngram, repetition_penalty, min_len, banned_tokens, 1)
        self.n_samples = n_samples
        self._calls = 0

    def _alloc(self, dev):
        R, T = self.R, self.T
        self._alloc_cache(dev)
        self.hist = torch.empty((R, T + 1), dtype=torch.int32, device=dev)
        self.score = torch.empty(R, dtype=torch.float32, device=dev)
        self.slen = torch.zeros(R, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(R, dtype=torch.int32, device=dev)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)

    def _reset(self):
        self.tok.fill_(self.start_token)
        self.hist[:, 0] = self.start_token
        self.score.zero_()
        self.slen.zero_()
        self.fin.zero_()

    def _step(self, t):
        logits = self._all_logits(t, None)
        if self.constrained:
            self._constrain(logits, self.hist, t)
        call("fpnmt_sample_step", self.R, self.V, ptr(logits), self.V, self.temperature, self.top_k, self.top_p, 0,
             ptr(self.seed_dev), ptr(self.score), ptr(self.slen), ptr(self.fin), ptr(self.hist), self.T + 1, t,
             self.end_token, ptr(self.tok), None, stream_ptr())

    @torch.no_grad()
    def decode(self, images, seed=None, check_every=8, consensus=None, consensus_weights="uniform",
               consensus_all=False):
        """images (n_images, H, W, 3) on the GPU -> per image a list of
        n_samples (token-id list, log-probability) pairs. seed None: a
        counter that advances per call; the same seed gives the same draws.

        consensus (a DeviceCiderD on this device): per image ONE token-id
        list, the sample that agrees most with the image's other samples
        under CIDEr-D with the tables' idf — a Monte Carlo estimate of the
        caption of greatest expected CIDEr-D (fpnmt_ciderd_consensus, one
        launch after the position loop on the decoder's own state).
        consensus_weights "uniform" weighs the samples equally (they are
        draws from the model already), "posterior" by the fp64 softmax per
        image of their log-probabilities. consensus_all: per image every
        sample as (token ids, log-probability, utility), by utility
        descending, then sample index. The draws are those of the same call
        without consensus."""
        if images.shape[0] != self.n_images:
            raise ValueError(f"expected {self.n_images} images, got {images.shape[0]}")
        with_consensus = consensus_validated("sample", consensus, consensus_weights, consensus_all, self.n_samples,
                                             self.T, images.device)
        if seed is None:
            seed = self._calls
        self._calls += 1
        self._prepare(images)
        self.seed_dev.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        for t in range(self.T):
            if self.graphs is not None:
                self.graphs[t].replay()
            else:
                self._step(t)
            if check_every and (t + 1) % check_every == 0 and t + 1 < self.T and bool(self.fin.all()):
                break
        if with_consensus:
            util, pick = self._consensus(consensus, consensus_weights, self.hist, self.slen, self.fin, self.score)
        hist, lens = self.hist.tolist(), self.slen.tolist()
        fin, score = self.fin.tolist(), self.score.tolist()
        if with_consensus:
            util, pick = util.tolist(), pick.tolist()
        out = []
        for i in range(self.n_images):
            rows = range(i * self.n_samples, (i + 1) * self.n_samples)
            if with_consensus:
                out.append(consensus_ranked([hist[r][1:1 + lens[r] - fin[r]] for r in rows], [score[r] for r in rows],
                                            [util[r] for r in rows], pick[i], consensus_all))
                continue
            out.append([(hist[r][1:1 + lens[r] - fin[r]], score[r]) for r in rows])
        return out

    @torch.no_grad()
    def decode_device(self, images, seed=None, check_every=0):
        """decode() without the read-back: prepares and replays the same
        positions with the same draws, and returns the decoder's OWN state
        tensors (hist (R, T + 1) int32, slen, fin (R,) int32, score (R,)
        fp32), valid until the next decode of this decoder. Row r's caption
        is hist[r][1 : 1 + slen[r] - fin[r]] (sampled_ids turns the state
        into lists). check_every 0 (the default) runs all positions and polls
        nothing, so the call never waits for the device; a positive value
        keeps decode()'s 4-byte fin.all() poll every that many positions for
        callers who prefer the early exit."""
        if images.shape[0] != self.n_images:
            raise ValueError(f"expected {self.n_images} images, got {images.shape[0]}")
        if seed is None:
            seed = self._calls
        self._calls += 1
        self._prepare(images)
        self.seed_dev.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        for t in range(self.T):
            if self.graphs is not None:
                self.graphs[t].replay()
            else:
                self._step(t)
            if check_every and (t + 1) % check_every == 0 and t + 1 < self.T and bool(self.fin.all()):
                break
        return self.hist, self.slen, self.fin, self.score


def sampled_ids(hist, slen, fin):
    """The state SampleDecoder.decode_device returns -> one token-id list per
    row (without <start> and a final <end>), what decode() returns as ids.
    Reads the three tensors back (one synchronisation)."""
    h, n, f = hist.tolist(), slen.tolist(), fin.tolist()
    return [h[r][1:1 + n[r] - f[r]] for r in range(len(n))]

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


class _CachedDecoder:
    """What BeamDecoder and SampleDecoder share: the geometry, the encoder
    pass with every layer's cross K/V, the staged biases, and one decode
    position through embed -> layers -> fp32 logits on the K/V cache.
    `beam_n` is the number of rows per image."""

    def __init__(self, transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph=True):
        self.tr = transformer
        dec = transformer.decoder
        self.n_images, self.beam_n, self.T = n_images, beam_n, max_seq_len
        self.start_token, self.end_token = start_token, end_token
        self.R = n_images * beam_n
        self.d = dec.d_model
        self.L = dec.num_layers
        self.V = transformer.final_layer.kernel.shape[1]
        self.heads = dec.dec_layers[0].mha1.num_heads if self.L else 8
        self.depth = self.d // self.heads
        if max_seq_len > dec.pos_encoding.shape[0]:
            raise ValueError(f"max_seq_len {max_seq_len} exceeds the decoder's positional table")
        self.use_graph = use_graph
        self.dt = None
        self.graphs = None
        self.qkv_bias = []

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
        self.kv = torch.empty((max(self.L, 1), self.R, self.T, 2 * self.d), dtype=self.dt, device=dev)
        self.tok = torch.empty(self.R, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------- encoder
    def _encode(self, images):
        """Encoder once per image (pipeline.py:93-94) and every layer's cross
        K/V from one grouped GEMM (no per-beam tiling: the attention maps beam
        rows to their image)."""
        tr, dec = self.tr, self.tr.decoder
        enc = tr.encoder(images, False, None)  # (n, Lenc, d)
        self.Lenc = enc.shape[1]
        n = enc.shape[0]
        if self.L == 0:
            self.enc_kv = torch.empty((1, 1), dtype=self.dt, device=enc.device)
            return
        grp = dec.cross_kv_group
        stack, _ = grp.stacked(self.dt)
        cols = grp.n * grp.fout  # 2 * L * d
        shape = (n * self.Lenc, cols)
        if getattr(self, "enc_kv", None) is None or tuple(self.enc_kv.shape) != shape:
            # static buffer: the captured step graphs read it by address
            self.enc_kv = torch.empty(shape, dtype=self.dt, device=enc.device)
            self.graphs = None
        e2 = enc.reshape(n * self.Lenc, self.d).contiguous()
        _gemm(n * self.Lenc, cols, self.d, dtype_code(self.dt), ptr(e2), self.d, ptr(stack), ptr(self.enc_kv), cols,
              ptr(grp.bias_cat()), stream_ptr())

    def _stage_biases(self, dev):
        """Each layer's [q|k|v] bias as one vector the step graphs read by
        address: a view when the biases are adjacent (arena order), else a
        static buffer refreshed here, once per decode call, instead of a
        concatenation per layer inside every step."""
        dec = self.tr.decoder
        if len(self.qkv_bias) != self.L:
            self.qkv_bias = [None] * self.L
        for i, lay in enumerate(dec.dec_layers):
            b = lay.qkv_group.bias_cat()
            cur = self.qkv_bias[i]
            if b._base is not None or b.numel() == 0:  # a view of the parameters
                if cur is None or cur.data_ptr() != b.data_ptr():
                    self.qkv_bias[i] = b
                    self.graphs = None
                continue
            if cur is None or cur.shape != b.shape or cur._base is not None:
                self.qkv_bias[i] = torch.empty_like(b, device=dev)
                self.graphs = None
            self.qkv_bias[i].copy_(b)

    def _prepare(self, images):
        """Before the first position of a decode call: buffers for the
        compute dtype, the encoder side, the state reset, the step graphs."""
        dt = compute_dtype()
        if self.dt != dt:
            self.dt = dt
            self._alloc(images.device)
            self.enc_kv = None
            self.graphs = None
        self._encode(images)
        self._stage_biases(images.device)
        self._reset()
        if self.use_graph and self.graphs is None:
            self._capture()

    # ------------------------------------------------------------ position
    def _logits(self, t, src):
        """Position t of every row: embed self.tok, the decoder layers on the
        K/V cache, the fp32 logits (R, V). src: the rows' cache-row tables
        (None: every row reads its own cache row)."""
        tr, dec = self.tr, self.tr.decoder
        dt, code, R, T, d = self.dt, dtype_code(self.dt), self.R, self.T, self.d
        s = stream_ptr()
        x = torch.empty((R, d), dtype=dt, device=self.tok.device)
        pe = dec.pos_encoding
        call("fpnmt_embed_posenc_fwd", code, R, 1, d, ptr(self.tok), ptr(dec.embedding.embeddings),
             pe.data_ptr() + t * d * pe.element_size(), ptr(x), s)
        scale = 1.0 / math.sqrt(float(self.depth))
        for i, lay in enumerate(dec.dec_layers):
            grp = lay.qkv_group
            stack, _ = grp.stacked(dt)
            bias = self.qkv_bias[i]
            q = torch.empty((R, d), dtype=dt, device=x.device)
            _gemm(R, d, d, code, ptr(x), d, ptr(stack), ptr(q), d, ptr(bias), s)
            kvl = self.kv[i]
            # this position's key / value straight into the cache (row r, position t)
            _gemm(R, 2 * d, d, code, ptr(x), d, stack.data_ptr() + d * d * stack.element_size(),
                  kvl.data_ptr() + t * 2 * d * kvl.element_size(), T * 2 * d,
                  bias.data_ptr() + d * bias.element_size(), s)
            a = torch.empty((R, d), dtype=dt, device=x.device)
            call("fpnmt_decode_attention", code, R, self.heads, self.depth, t + 1, scale, ptr(q), d, ptr(kvl),
                 T * 2 * d, 2 * d, 0, d, ptr(src), T, 1, ptr(a), d, s)
            out1 = lay.layernorm1(lay.mha1.dense(a), residual=x)
            q2 = lay.mha2.wq(out1)
            a2 = torch.empty((R, d), dtype=dt, device=x.device)
            cols = 2 * self.L * d
            call("fpnmt_decode_attention", code, R, self.heads, self.depth, self.Lenc, scale, ptr(q2), d,
                 ptr(self.enc_kv), self.Lenc * cols, cols, 2 * i * d, 2 * i * d + d, None, 0, self.beam_n, ptr(a2),
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


class BeamDecoder(_CachedDecoder):
    """decode(images) -> list of token-id lists, one per image; in
    mode="beam", decode(images, n_best=k) -> per image the k best
    (token ids, score) pairs, best first.

    mode="beam" takes the constraints no_repeat_ngram (0: off),
    repetition_penalty (1: off), min_len (0: off) and banned_tokens: every
    live beam's logits row is constrained before the step ranks it, so a
    beam's score is the sum of log_softmax over the constrained rows — its
    log-probability under the constrained, renormalised distribution.
    mode="reference" is the reference's own procedure and takes none."""

    def __init__(self, transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph=True,
                 mode="reference", length_alpha=0.0, no_repeat_ngram=0, repetition_penalty=1.0, min_len=0,
                 banned_tokens=()):
        if mode not in ("reference", "beam"):
            raise ValueError(f"mode must be 'reference' or 'beam', got {mode!r}")
        self.mode, self.length_alpha = mode, float(length_alpha)
        super().__init__(transformer, n_images, beam_n, max_seq_len, start_token, end_token, use_graph)
        self._set_constraints(no_repeat_ngram, repetition_penalty, min_len, banned_tokens, beam_n)
        if self.constrained and mode != "beam":
            raise ValueError("constrained decoding needs mode='beam': mode='reference' is the reference's own procedure")

    # ---------------------------------------------------------- buffers
    def _alloc(self, dev):
        dt, R, T, d = self.dt, self.R, self.T, self.d
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
            self.score.view(self.n_images, self.beam_n)[:, 0] = 0.0
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
        logits = self._logits(t, sin)
        if self.mode == "beam":
            if self.constrained:
                self._constrain(logits, hin, t)
            call("fpnmt_beam_step_log", self.n_images, self.beam_n, self.V, ptr(logits), self.V, ptr(self.score),
                 ptr(self.blen), ptr(self.fin), ptr(hin), ptr(hout), T + 1, t, ptr(sin), ptr(sout), T,
                 self.end_token, ptr(self.tok), ptr(self.status), s)
            return
        call("fpnmt_beam_step", self.n_images, self.beam_n, self.V, ptr(logits), self.V, ptr(self.prob), ptr(hin),
             ptr(hout), T + 1, t, ptr(sin), ptr(sout), T, self.end_token, ptr(self.tok), ptr(self.result), T,
             ptr(self.result_len), ptr(self.status), s)

    # -------------------------------------------------------------- decode
    @torch.no_grad()
    def decode(self, images, check_every=8, n_best=1):
        """images (n_images, H, W, 3) on the GPU -> list of token-id lists;
        n_best > 1 (mode="beam"): per image a list of the n_best
        (token-id list, score) pairs, best first."""
        if images.shape[0] != self.n_images:
            raise ValueError(f"expected {self.n_images} images, got {images.shape[0]}")
        if n_best < 1 or n_best > (self.beam_n if self.mode == "beam" else 1):
            raise ValueError(f"n_best {n_best}: mode {self.mode!r} with {self.beam_n} beams gives 1.."
                             f"{self.beam_n if self.mode == 'beam' else 1}")
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
        if self.mode == "beam":
            return self._nbest(steps, n_best)
        lens = self.result_len.tolist()
        res = self.result.cpu()
        return [res[i, :lens[i]].tolist() for i in range(self.n_images)]

    def _nbest(self, steps, n_best):
        """Rank the beams of every image (fpnmt_beam_finalize over the tables
        the last step wrote) and read the n-best list back."""
        n, K, T = self.n_images, self.beam_n, self.T
        call("fpnmt_beam_finalize", n, K, ptr(self.hist[steps % 2]), T + 1, ptr(self.score), ptr(self.blen),
             ptr(self.fin), self.length_alpha, ptr(self.nbest_tok), T, ptr(self.nbest_len), ptr(self.nbest_score),
             stream_ptr())
        tok, lens, score = self.nbest_tok.cpu(), self.nbest_len.tolist(), self.nbest_score.tolist()
        if n_best == 1:
            return [tok[i, 0, :lens[i][0]].tolist() for i in range(n)]
        return [[(tok[i, k, :lens[i][k]].tolist(), score[i][k]) for k in range(n_best)] for i in range(n)]


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
    constrained, renormalised distribution."""

    def __init__(self, transformer, n_images, n_samples, max_seq_len, start_token, end_token, use_graph=True,
                 temperature=1.0, top_k=0, top_p=1.0, no_repeat_ngram=0, repetition_penalty=1.0, min_len=0,
                 banned_tokens=()):
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
        super().__init__(transformer, n_images, n_samples, max_seq_len, start_token, end_token, use_graph)
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
        logits = self._logits(t, None)
        if self.constrained:
            self._constrain(logits, self.hist, t)
        call("fpnmt_sample_step", self.R, self.V, ptr(logits), self.V, self.temperature, self.top_k, self.top_p, 0,
             ptr(self.seed_dev), ptr(self.score), ptr(self.slen), ptr(self.fin), ptr(self.hist), self.T + 1, t,
             self.end_token, ptr(self.tok), None, stream_ptr())

    @torch.no_grad()
    def decode(self, images, seed=None, check_every=8):
        """images (n_images, H, W, 3) on the GPU -> per image a list of
        n_samples (token-id list, log-probability) pairs. seed None: a
        counter that advances per call; the same seed gives the same draws."""
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
        hist, lens = self.hist.tolist(), self.slen.tolist()
        fin, score = self.fin.tolist(), self.score.tolist()
        out = []
        for i in range(self.n_images):
            rows = range(i * self.n_samples, (i + 1) * self.n_samples)
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

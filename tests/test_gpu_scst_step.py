"""Self-critical training on the GPU: TrainEngine.step_weighted against the
CPU oracle (fp64 anchor, the fp32 oracle's own error as the noise floor),
its equivalences with the plain step, graph replay / split form /
determinism / alternation with the plain step, the training path's
log-probabilities against the sampler's, one step's effect on the policy,
and Pipeline.train_step_scst's interface."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import _build, _perturbed

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
STATE = ("flat", "m", "v", "vhat", "step")


def _captions(rows, T, vocab, seed, lens=None):
    """(rows, T) padded captions <start>=2 ... <end>=3 0..., of different lengths."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(4, vocab, (rows, T), generator=g)
    tok[:, 0] = 2
    for r in range(rows):
        n = lens[r] if lens else int(torch.randint(3, T + 1, (1,), generator=g))
        tok[r, n - 1] = 3
        tok[r, n:] = 0
    return tok


def _images(b, image, seed):
    return torch.rand(b, image, image, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _grads(m):
    return {n: p.grad.detach().cpu().double().clone() for n, p in m.named_parameters()}


# ------------------------------------------------------------ the oracle
def oracle_weighted(sd, img, tok, w, n, cfg, trainable, dtype=torch.float32):
    """The weighted step restated on the CPU oracle: the encoder once per
    image, repeat_interleave, the weighted mean loss over ALL rows, autograd.
    Returns (loss, {name: grad}, emb_sumsq, per-row log-probabilities);
    with nothing trainable, the loss alone is computed."""
    from oracle import ref_cpu as R
    params = {k: v.to(dtype).detach().clone().requires_grad_(k in trainable) if v.is_floating_point() else v
              for k, v in sd.items()}
    tar_inp, tar_real = tok[:, :-1], tok[:, 1:]
    holder = {}

    def hook(e):
        e.retain_grad()
        holder["e"] = e
        return e

    enc = R.encoder(params, img.to(dtype), cfg, training=True, stats=cfg.get("bn_stats"))
    dec, _ = R.decoder(params, tar_inp, enc.repeat_interleave(n, 0), R.create_masks(tar_inp), cfg,
                       emb_hook=hook if trainable else None)
    logits = dec @ params["final_layer.kernel"] + params["final_layer.bias"]
    ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), tar_real.reshape(-1).long(), reduction="none")
    live = (tar_real.reshape(-1) != 0).to(dtype)
    loss = (ce * live * w.to(dtype).repeat_interleave(tok.shape[1] - 1)).mean()
    if not trainable:
        return loss.detach(), {}, 0.0, (-ce * live).detach()
    loss.backward()
    grads = {k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])) for k in trainable}
    return loss.detach(), grads, float((holder["e"].grad.double() ** 2).sum()), (-ce * live).detach()


def _bars(m, g64, gpu, cpu_sets, bulk_floor=1e-5):
    """The gradient bars of test_gpu_model._train_step_parity: per tensor,
    the GPU's max error against fp64 within 10x the fp32 oracle's (the larger
    of its runs) + 1e-2 of the tensor's max, and the 90th percentile within
    3x the oracle's + bulk_floor of the max. Returns the worst excesses."""
    rows, bulk = [], []
    for n, _ in m.named_parameters():
        t = g64[n].double()
        mx = float(t.abs().max())
        dg = (gpu[n] - t).abs()
        dc = torch.stack([(cs[n].double() - t).abs() for cs in cpu_sets]).amax(0)
        eg, ec = float(dg.max()), float(dc.max())
        rows.append((eg - 10 * ec - 1e-2 * mx - 1e-7, eg / max(mx, 1e-30), ec / max(mx, 1e-30), n))
        if t.numel() >= 16:
            def p90(d, big):
                return float(torch.quantile(d.flatten().float(), 0.9)) if d.numel() < 2 ** 24 else big
            qg, qc = p90(dg, eg), p90(dc, ec)
            bulk.append((qg - 3 * qc - bulk_floor * mx - 1e-8, qg / max(mx, 1e-30), qc / max(mx, 1e-30), n))
    rows.sort(reverse=True)
    bulk.sort(reverse=True)
    return rows, bulk


def test_step_weighted_gradients_against_the_oracle_fp32(parity_record):
    from fpnmt.train import TrainEngine
    B, n, T, vocab, image = 2, 3, 12, 300, 128
    m, sd, cfg = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T)
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    img = _images(B, image, 3)
    tok = _captions(B * n, T, vocab, 4, lens=[12, 5, 3, 9, 12, 7])
    w = torch.tensor([1.3, -0.8, 0.0, -2.1, 0.6, 0.9])
    l64, g64, _, _ = oracle_weighted(sd, img, tok, w, n, cfg, trainable, torch.float64)
    l32, g32, _, _ = oracle_weighted(sd, img, tok, w, n, cfg, trainable)
    _, g32p, _, _ = oracle_weighted(sd, _perturbed(img, 77), tok, w, n, cfg, trainable)
    eng = TrainEngine(m, 0.0, use_graph=False)
    loss = float(eng.step_weighted(img.to(DEV), tok.to(DEV), w.to(DEV)))
    torch.cuda.synchronize()
    rows, bulk = _bars(m, g64, _grads(m), [g32, g32p])
    zero = {k for k in g64 if float(g64[k].abs().max()) < 1e-7}  # structurally zero: relative errors mean nothing
    for r in sorted(rows, key=lambda r: -r[1])[:3]:
        print("grad max rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    for r in sorted(bulk, key=lambda r: -r[1])[:3]:
        print("grad p90 rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    print(f"loss gpu {loss:.7f} oracle32 {float(l32):.7f} oracle64 {float(l64):.7f}")
    parity_record["scst_step_weighted_1L_V300_128_b2_n3"] = {
        "loss_gpu": loss, "loss_oracle32": float(l32), "loss_oracle64": float(l64),
        # relative to the tensor's max |fp64 gradient|, over the tensors with a nonzero gradient
        "grad_max_rel_err_vs_fp64_worst": [{"param": r[3], "gpu": r[1], "cpu_fp32": r[2]}
                                           for r in sorted(rows, key=lambda r: -r[1]) if r[3] not in zero][:5],
        "grad_p90_rel_err_vs_fp64_worst": [{"param": r[3], "gpu": r[1], "cpu_fp32": r[2]}
                                           for r in sorted(bulk, key=lambda r: -r[1]) if r[3] not in zero][:5],
        "grad_structurally_zero": len(zero)}
    assert abs(loss - float(l32)) <= 1e-4 * max(1.0, abs(float(l32)))
    assert rows[0][0] <= 0.0, rows[0]
    assert bulk[0][0] <= 0.0, bulk[0]


# ----------------------------------------------------------- equivalences
def test_unit_weights_one_caption_per_image_is_the_plain_step():
    """n = 1, weights 1: the forward is the plain step's launch for launch
    (the repeat is a copy), so the logits are the same bits; the two loss
    kernels' dlogits are each within u (V + 4X + 10) |coef| of the exact
    softmax gradient (tests/test_gpu_scst_kernels.py), and the backward is
    the same linear map (the forward's masks are fixed) applied to them. Per
    tensor, the gradients therefore agree within twice that relative
    distance (each kernel's from the exact one), taken of the tensor's
    largest gradient; the losses within twice the kernels' B_loss, which is
    at most u (V + 5X + 4 log V + 2) + (rows + 2) u |loss|."""
    from fpnmt.train import TrainEngine
    from models.transformer import create_masks
    B, T, vocab, image = 2, 12, 300, 224
    m, _, _ = _build(num_layers=2, vocab=vocab, image=image, max_seq_len=T)
    img, tok = _images(B, image, 5).to(DEV), _captions(B, T, vocab, 6).to(DEV)
    eng = TrainEngine(m, 0.0, use_graph=False)
    l0 = float(eng.step(img, tok))
    g0 = _grads(m)
    l1 = float(eng.step_weighted(img, tok, torch.ones(B, device=DEV)))
    g1 = _grads(m)
    with torch.no_grad():
        logits, _ = m(img, tok[:, :-1], True, create_masks(tok[:, :-1]))
    X = float(logits.abs().max())
    rel = 2 * U * (vocab + 4 * X + 10)
    worst = max((float((g1[k] - g0[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30), k) for k in g0
                if float(g0[k].abs().max()) > 1e-7)
    print(f"loss {l0:.8f} / {l1:.8f}; worst gradient distance {worst[0]:.3e} of the max ({worst[1]}), bound {rel:.3e}")
    rows = B * (T - 1)
    assert abs(l0 - l1) <= 2 * U * (vocab + 5 * X + 4 * math.log(vocab) + 2 + (rows + 2) * abs(l0))
    assert worst[0] <= rel, worst
    for k in g0:
        if float(g0[k].abs().max()) <= 1e-7:  # structurally zero gradients stay so
            assert float(g1[k].abs().max()) <= 1e-7, k


def test_unit_weights_equal_the_plain_step_on_repeated_images():
    """n = 3, weights 1 against step(img.repeat_interleave(3, 0), tok): the
    same gradient by linearity, summed in another order (the plain step adds
    the three copies' encoder-side contributions inside its weight-gradient
    reductions; the weighted step adds them once, in RepeatRowsFn's backward)
    on a forward of another batch size. The distance allowed is the plain
    step's own fp32 noise at that input, by the bars of _train_step_parity
    with the plain step as the anchor. Its noise floor is the larger of its
    distances from itself under two changes that leave the gradient
    mathematically as it is: the images moved by ~1 ulp (rounding of the
    forward at the same launches), and every (image, caption) row given
    twice — batch 12 instead of 6, the same mean — because the two forms
    under test run the feature extractor at different batch sizes (2 and 6),
    which changes tiles, split-K factors and with them the order of every
    sum over the batch; a sample at one batch size cannot show that noise
    (at first this test took the 1-ulp sample alone, and a reordering of the
    six rows, which moved nothing).
    The loss by that test's loss bar."""
    from fpnmt.train import TrainEngine
    B, n, T, vocab, image = 2, 3, 12, 300, 224
    m, _, _ = _build(num_layers=2, vocab=vocab, image=image, max_seq_len=T)
    img, tok = _images(B, image, 7), _captions(B * n, T, vocab, 8).to(DEV)
    rep = img.repeat_interleave(n, 0)
    eng = TrainEngine(m, 0.0, use_graph=False)
    la = float(eng.step(rep.to(DEV), tok))
    anchor = _grads(m)
    lp = float(eng.step(_perturbed(img, 77).repeat_interleave(n, 0).to(DEV), tok))
    noise = _grads(m)
    lo = float(eng.step(rep.repeat(2, 1, 1, 1).to(DEV), tok.repeat(2, 1)))
    noise_batch = _grads(m)
    lw = float(eng.step_weighted(img.to(DEV), tok, torch.ones(B * n, device=DEV)))
    got = _grads(m)
    rows, bulk = _bars(m, anchor, got, [noise, noise_batch])
    print(f"loss plain {la:.8f} perturbed {lp:.8f} batch 12 {lo:.8f} weighted {lw:.8f}")
    for r in sorted(bulk, key=lambda r: -r[0])[:3]:
        print("grad p90 excess %.2e: weighted %.2e  plain's own %.2e  %s" % r)
    for r in sorted(rows, key=lambda r: -r[1])[:3]:
        print("grad max rel distance: weighted %.2e  plain's own %.2e  %s" % r[1:])
    assert abs(lw - la) <= 1e-4 * max(1.0, abs(la))
    assert rows[0][0] <= 0.0, rows[0]
    assert bulk[0][0] <= 0.0, bulk[0]


# ------------------------------------------- graph, split, determinism
def _sync_state(dst, src):
    from fpnmt import layers as flayers
    with torch.no_grad():
        for nme in STATE:
            getattr(dst.arena, nme).copy_(getattr(src.arena, nme))
    flayers.prepare_all(dst.model)


def _batches(B, n, T, vocab, image, k):
    g = torch.Generator().manual_seed(90)
    out = []
    for i in range(k):
        out.append((_images(B, image, 20 + i).to(DEV), _captions(B * n, T, vocab, 30 + i).to(DEV),
                    (torch.randn(B * n, generator=g) * 1.5).to(DEV)))
    return out


def test_graph_replay_is_bitwise_the_eager_step_bf16():
    """Eager and graph engines put in the same state before every step: the
    first call (eager in both), the capture, and replays after new images,
    tokens and weights were written into the static buffers, with dropout
    (its keys come from the site number and the device step counter). Then
    the same step twice from one state: the same bits."""
    import fpnmt
    from fpnmt.train import TrainEngine
    B, n, T, vocab, image = 2, 3, 12, 300, 224
    m_e, _, _ = _build(num_layers=2, vocab=vocab, image=image, max_seq_len=T, seed=51, rate=0.1)
    m_g, _, _ = _build(num_layers=2, vocab=vocab, image=image, max_seq_len=T, seed=51, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False)
        G = TrainEngine(m_g, 1e-4, use_graph=True)
        losses = []
        for i, (img, tok, w) in enumerate(_batches(B, n, T, vocab, image, 4)):
            _sync_state(G, E)
            le = E.step_weighted(img, tok, w).clone()
            lg = G.step_weighted(img, tok, w).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            for nme in STATE:
                assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (i, nme)
            losses.append(float(le))
        assert len(set(losses)) == 4 and int(E.arena.step) == 4
        assert len(G._wsteps) == 1 and next(iter(G._wsteps.values()))[1] is not None  # captured once, replayed
        s0 = {nme: getattr(G.arena, nme).clone() for nme in STATE}
        img, tok, w = _batches(B, n, T, vocab, image, 1)[0]
        runs = []
        for _ in range(2):
            with torch.no_grad():
                for nme in STATE:
                    getattr(G.arena, nme).copy_(s0[nme])
            from fpnmt import layers as flayers
            flayers.prepare_all(m_g)
            loss = G.step_weighted(img, tok, w).clone()
            torch.cuda.synchronize()
            runs.append((loss, {nme: getattr(G.arena, nme).clone() for nme in STATE}))
        assert torch.equal(runs[0][0], runs[1][0])
        for nme in STATE:
            assert torch.equal(runs[0][1][nme], runs[1][1][nme]), nme
        assert not torch.equal(runs[0][1]["flat"], s0["flat"])
    finally:
        fpnmt.set_precision("fp32")


def test_split_backward_weighted_step_matches_single_graph():
    """The split form (G1 .. G3, what a multi-rank run replays) at world 1
    equals the single-graph form, one step at a time from identical state —
    the assertions of test_split_backward_step_matches_single_graph."""
    from fpnmt.train import TrainEngine
    B, n, T, vocab, image = 2, 3, 12, 300, 224
    m_a, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=12)
    m_b, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=12)
    A = TrainEngine(m_a, 1e-6, use_graph=True)
    Bs = TrainEngine(m_b, 1e-6, use_graph=True, split_backward=True)
    assert Bs.split and not A.split
    img, tok, w = _batches(B, n, T, vocab, image, 1)[0]
    for i in range(4):
        if i:
            _sync_state(Bs, A)
        p0 = A.arena.flat.detach().clone()
        la = float(A.step_weighted(img, tok, w))
        lb = float(Bs.step_weighted(img, tok, w))
        torch.cuda.synchronize()
        da, db = A.arena.flat - p0, Bs.arena.flat - p0
        upd = float(da.abs().mean())
        err = float((da - db).abs().mean())
        print(f"step {i}: loss {la:.7f} / {lb:.7f}; mean |update| {upd:.3e}, mean |d update| {err:.3e}")
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la))
        assert upd > 0 and err <= 0.02 * upd
    assert len(next(iter(Bs._wsteps.values()))[1]) > 2  # a sequence of graphs


def test_plain_and_weighted_steps_alternate_on_one_arena_bf16():
    """P W P W P W W P on a graph engine (both kinds captured, then replayed
    in turn) leaves the arena of the same sequence run eagerly: parameters,
    AMSGrad state and the step counter, bit for bit."""
    import fpnmt
    from fpnmt.train import TrainEngine
    B, n, T, vocab, image = 2, 2, 12, 300, 224
    m_e, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=61, rate=0.1)
    m_g, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=61, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False)
        G = TrainEngine(m_g, 1e-4, use_graph=True)
        batches = _batches(B, n, T, vocab, image, 8)
        for i, kind in enumerate("PWPWPWWP"):
            img, tok, w = batches[i]
            for eng in (E, G):
                if kind == "P":
                    loss = eng.step(img, tok[::n].contiguous())
                else:
                    loss = eng.step_weighted(img, tok, w)
            assert math.isfinite(float(loss))
        torch.cuda.synchronize()
        assert G.graphs is not None and next(iter(G._wsteps.values()))[1] is not None
        assert int(G.arena.step) == 8
        for nme in STATE:
            assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), nme
    finally:
        fpnmt.set_precision("fp32")


# ------------------------------------------- decode path vs training path
SC = dict(n_layers=1, vocab=300, image=128, T=10, B=2, n=3, end_bias=3.0)


@pytest.fixture(scope="module")
def pipeline():
    """A small fp32 pipeline (rate 0) whose engine has lr 0: steps leave the
    parameters as they are."""
    import fpnmt
    from fpnmt.train import TrainEngine
    from test_gpu_beam_search import _pipeline
    fpnmt.set_precision("fp32")
    c = SC
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], 23, c["T"], c["end_bias"])
    pl.engine = pl.optimizer = TrainEngine(pl.transformer, 0.0, use_graph=False)
    return pl, _images(c["B"], c["image"], 9).to(DEV)


def _row_logp(pl, img, tok, w, n):
    """(loss, (rows, T - 1) log-probabilities) of the training path in
    inference mode: the step's forward and loss launch, no backward."""
    from fpnmt import ops
    tr = pl.transformer
    with torch.no_grad():
        tar_inp, tar_real, mask = ops.decoder_targets(tok)
        enc = ops.RepeatRowsFn.apply(tr.encoder(img, True, None), n)
        dec, _ = tr.decoder(tar_inp, enc, True, mask, None)
        loss, logp = ops.WeightedXentFn.apply(tr.final_layer(dec), tar_real, w, tok.shape[1] - 1, True)
    return loss, logp.view(tok.shape[0], tok.shape[1] - 1)


def test_training_path_log_probabilities_equal_the_sampler_score(pipeline):
    """Per sampled caption, the sum of the loss kernel's row_logp over its
    positions (teacher-forced, batched) is the SampleDecoder's score (K/V
    cache, one position at a time): both are fp32 paths whose logits lie
    within eps = 1e-3 of the oracle's, so they differ by at most 2 eps per
    token — the bar of test_sampled_trajectories_follow_the_oracle_fp32."""
    from fpnmt.scst import pack_tokens
    pl, img = pipeline
    c, eps = SC, 1e-3
    drawn = pl.predict_batch(img, c["T"] - 1, use_graph=False, mode="sample", n_samples=c["n"], seed=5)
    ids = [s[0] for per in drawn for s in per]
    score = [s[1] for per in drawn for s in per]
    tok = torch.from_numpy(pack_tokens(ids, c["T"], pl.start_token, pl.end_token, c["T"] - 1)).to(DEV)
    _, logp = _row_logp(pl, img, tok, torch.ones(len(ids), device=DEV), c["n"])
    got = logp.sum(1).cpu().tolist()
    lens = [int((tok[r, 1:] != 0).sum()) for r in range(len(ids))]
    print("lengths", lens, "max |sum row_logp - score|", max(abs(a - b) for a, b in zip(got, score)))
    assert len(set(lens)) > 1
    for r in range(len(ids)):
        assert abs(got[r] - score[r]) <= 2 * eps * lens[r], (r, got[r], score[r])


def _length_reward(_i, ids):
    return -abs(len(ids) - 3.0)


def test_one_step_moves_the_policy_towards_the_reward():
    """Reward: minus the distance of the caption length from 3. The
    surrogate sum_r A_r (-log p(caption r)) of the SAME samples, evaluated
    in inference mode before and after one train_step_scst, must decrease.
    AMSGrad's first update is lr * sign-like per element, so the decrease is
    first-order guaranteed only for a small lr: the CPU oracle (the weighted
    step restated + KerasAMSGrad at the same lr on the same tokens and
    advantages) is asked first and must show the decrease on its own. At
    lr 1e-5 the oracle's surrogate went 36.608 -> 30.432 (measured; the GPU's
    36.608 -> 30.430)."""
    import fpnmt
    from oracle import ref_cpu as R
    from fpnmt.scst import pack_tokens
    from fpnmt.train import TrainEngine
    from test_gpu_beam_search import _pipeline
    fpnmt.set_precision("fp32")
    c, lr, seed = SC, 1e-5, 11
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], 29, c["T"], c["end_bias"])
    pl.engine = pl.optimizer = TrainEngine(pl.transformer, lr, use_graph=False)
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=c["n_layers"], num_heads=8, backbone="resnet50")
    img = _images(c["B"], c["image"], 10)
    out = pl.train_step_scst(img.to(DEV), [[] for _ in range(c["B"])], n_samples=c["n"], reward=_length_reward,
                             seed=seed)
    torch.cuda.synchronize()
    ids = [s[0] for per in out["samples"] for s in per]
    adv = torch.from_numpy(out["advantages"].reshape(-1)).float()
    assert float(adv.abs().max()) > 0, "all samples of an image got the same reward"
    tok = torch.from_numpy(pack_tokens(ids, c["T"], pl.start_token, pl.end_token, c["T"] - 1))
    rows = tok.shape[0] * (c["T"] - 1)
    # the oracle alone
    trainable = [k for k, p in pl.transformer.named_parameters() if p.requires_grad]
    emb = "decoder.embedding.embeddings"
    l_before, grads, sumsq, _ = oracle_weighted(sd, img, tok, adv, c["n"], cfg, set(trainable))
    opt = R.KerasAMSGrad(trainable, [sd[k].shape for k in trainable], sparse=[emb])
    params = {k: v.clone() for k, v in sd.items()}
    opt.apply(params, grads, lambda it: lr, norms={emb: sumsq})
    l_after = oracle_weighted(params, img, tok, adv, c["n"], cfg, set())[0]
    print(f"oracle surrogate {float(l_before) * rows:.6f} -> {float(l_after) * rows:.6f}")
    assert float(l_after) < float(l_before)
    # the GPU: the step's own loss is the surrogate before; the same tokens and weights again after
    s_before = float(out["loss"]) * rows
    s_after = float(_row_logp(pl, img.to(DEV), tok.to(DEV), adv.to(DEV), c["n"])[0]) * rows
    print(f"gpu surrogate {s_before:.6f} -> {s_after:.6f}")
    assert abs(s_before - float(l_before) * rows) <= 1e-4 * rows * max(1.0, abs(float(l_before)))
    assert s_after < s_before


# ---------------------------------------------------------- the interface
def test_train_step_scst_interface(pipeline):
    pl, img = pipeline
    c = SC
    refs = [[[5, 6, 7, 8], [5, 6, 9]], [[10, 11, 12], [10, 13, 12, 14]]]
    a = pl.train_step_scst(img, refs, n_samples=c["n"], seed=3)
    assert set(a) >= {"loss", "reward_mean", "baseline_mean", "sample_logp_mean"}
    assert a["loss"].is_cuda and math.isfinite(float(a["loss"]))
    assert a["sample_logp_mean"] < 0 and a["reward_mean"] >= 0
    assert abs(a["reward_mean"] - a["baseline_mean"]) <= 1e-12  # leave-one-out baselines average to the mean reward
    # the same seed: the same samples and the same loss (lr 0: the same parameters)
    b = pl.train_step_scst(img, refs, n_samples=c["n"], seed=3)
    assert a["samples"] == b["samples"] and torch.equal(a["loss"], b["loss"])
    assert pl.train_step_scst(img, refs, n_samples=c["n"], seed=4)["samples"] != a["samples"]
    # no seed: a new draw every call
    assert pl.train_step_scst(img, refs, n_samples=c["n"])["samples"] != \
        pl.train_step_scst(img, refs, n_samples=c["n"])["samples"]
    # the greedy baseline is the reward of the reference decode's caption
    seen = []

    def reward(i, ids):
        seen.append((i, list(ids)))
        return float(len(ids)) + 0.25 * i

    g = pl.train_step_scst(img, refs, n_samples=1, baseline="greedy", reward=reward, seed=3)
    greedy = pl.predict_batch(img, c["T"] - 1, use_graph=False, mode="reference")
    assert [s for s in seen[-c["B"]:]] == [(i, greedy[i]) for i in range(c["B"])]
    assert abs(g["baseline_mean"] - sum(len(x) + 0.25 * i for i, x in enumerate(greedy)) / c["B"]) <= 1e-12
    assert g["advantages"].shape == (c["B"], 1)
    # sampling filters pass through
    f = pl.train_step_scst(img, refs, n_samples=2, temperature=0.8, top_k=20, top_p=0.9, seed=3)
    assert math.isfinite(float(f["loss"]))
    for kw in (dict(n_samples=0), dict(n_samples=1), dict(baseline="median"), dict(n_samples=1, baseline="best")):
        with pytest.raises(ValueError):
            pl.train_step_scst(img, refs, **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, refs[:1], n_samples=2)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, n_samples=2)

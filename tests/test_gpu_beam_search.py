"""Beam search proper (BeamDecoder mode="beam"): the log-domain step kernel
and the n-best ranking kernel against torch restatements written here, the
whole decoder against a literal CPU beam search on the oracle's model
(full-prefix recompute, no cache, the same rule), graph replay, and the
error paths of the two C entry points."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = float("-inf")


# ------------------------------------------------------------ restatements
def _step_ref(logits, score, blen, fin, t, end, K):
    """One image, one step: log_softmax, a finished beam masked down to its
    own <end> slot, stable descending sort (lower flat index first)."""
    V = logits.shape[1]
    cand = score[:, None] + torch.log_softmax(logits, -1)
    for b in range(K):
        if fin[b]:
            cand[b] = NEG
            cand[b, end] = score[b]
    vals, idx = torch.sort(cand.reshape(-1), descending=True, stable=True)
    par, tok = idx[:K] // V, idx[:K] % V
    pfin = fin[par].bool()
    nfin = (pfin | (tok == end)).to(torch.int32)
    nlen = torch.where(pfin, blen[par], torch.full_like(blen[par], t + 1))
    return vals, par, tok.to(torch.int32), nlen, nfin


def _assert_clear(vals, K, gap):
    """Neighbours among the first K + 1 candidates are either exactly equal
    (the constructed ties, which the index decides) or further apart than
    `gap`: a different id is then a bug, not rounding."""
    v = vals[:K + 1].double()
    d = v[:-1] - v[1:]
    assert bool(((d == 0) | (d > gap) | torch.isnan(d)).all()), d  # nan: -inf next to -inf


def _step_inputs(beam_n, V, t, T, n_img, g):
    R = n_img * beam_n
    return dict(logits=torch.randn(R, V, generator=g),
                hist=torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32),
                src=torch.randint(0, R, (R, T), generator=g, dtype=torch.int32),
                score=torch.zeros(R), blen=torch.full((R,), t, dtype=torch.int32),
                fin=torch.zeros(R, dtype=torch.int32), status=torch.zeros(n_img, dtype=torch.int32),
                tok=torch.full((R,), 1, dtype=torch.int32))


def _run_step(inp, beam_n, V, t, T, n_img, end):
    """Launch fpnmt_beam_step_log on copies of `inp` and compare every image
    with the restatement (a frozen image: with its own rows carried over)."""
    from fpnmt import _lib as L
    d = {k: v.clone().to(DEV) for k, v in inp.items()}
    hout, sout = torch.full_like(d["hist"], -7), torch.full_like(d["src"], -7)
    L.call("fpnmt_beam_step_log", n_img, beam_n, V, d["logits"].data_ptr(), V, d["score"].data_ptr(),
           d["blen"].data_ptr(), d["fin"].data_ptr(), d["hist"].data_ptr(), hout.data_ptr(), T + 1, t,
           d["src"].data_ptr(), sout.data_ptr(), T, end, d["tok"].data_ptr(), d["status"].data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    hout, sout = hout.cpu(), sout.cpu()
    assert not bool(torch.isnan(out["score"]).any())
    for i in range(n_img):
        rows = slice(i * beam_n, (i + 1) * beam_n)
        own = torch.arange(i * beam_n, (i + 1) * beam_n, dtype=torch.int32)
        if int(inp["status"][i]):
            for k in ("score", "blen", "fin", "tok"):
                assert torch.equal(out[k][rows], inp[k][rows]), (i, k)
            assert int(out["status"][i]) == 1
            assert torch.equal(hout[rows, :t + 1], inp["hist"][rows, :t + 1])
            assert torch.equal(sout[rows, :t + 1], inp["src"][rows, :t + 1])
            assert torch.equal(sout[rows, t + 1], own)
            continue
        vals, par, tok, nlen, nfin = _step_ref(inp["logits"][rows], inp["score"][rows], inp["blen"][rows],
                                               inp["fin"][rows], t, end, beam_n)
        _assert_clear(vals, beam_n, 1e-4)
        pr = par + i * beam_n
        assert torch.equal(out["tok"][rows], tok), (i, out["tok"][rows], tok)
        assert torch.equal(hout[rows, :t + 1], inp["hist"][pr, :t + 1])
        assert torch.equal(hout[rows, t + 1], tok)
        assert torch.equal(sout[rows, :t + 1], inp["src"][pr, :t + 1])
        assert torch.equal(sout[rows, t + 1], own)
        assert torch.equal(out["blen"][rows], nlen)
        assert torch.equal(out["fin"][rows], nfin)
        assert int(out["status"][i]) == int(nfin.all())
        assert torch.allclose(out["score"][rows], vals[:beam_n], rtol=1e-5, atol=0), (out["score"][rows], vals[:beam_n])
    return out


def _first_step_case(beam_n, V, t, T, n_img):
    inp = _step_inputs(beam_n, V, t, T, n_img, torch.Generator().manual_seed(100 + beam_n * V))
    inp["score"].fill_(NEG)
    inp["score"][::beam_n] = 0.0
    inp["logits"][0, 7] = inp["logits"][0, 11] = inp["logits"][0].max() + 1
    return inp


STEP_SHAPES = [(1, 37), (4, 200), (16, 1000), (8, 10000)]  # V 37: scalar loads; V 10000: four loads in flight


@pytest.mark.parametrize("beam_n,V", STEP_SHAPES)
def test_beam_step_log_first_step(beam_n, V):
    """t = 0: beam 0 at score 0, the others at -inf and silent, so the new
    beams are the beam_n best first tokens of beam 0 (two of them an exact
    tie inside the row)."""
    n_img, T, t, end = 3, 12, 0, 3
    out = _run_step(_first_step_case(beam_n, V, t, T, n_img), beam_n, V, t, T, n_img, end)
    assert bool(torch.isfinite(out["score"]).all())
    assert out["tok"][:min(beam_n, 2)].tolist() == [7, 11][:beam_n]


@pytest.mark.parametrize("beam_n,V", STEP_SHAPES)
def test_beam_step_log_finished_beams(beam_n, V):
    """t = 5. Image 0: beams 0 and 1 the same row at the same score with two
    equal maxima (four tied candidates, the index decides, at beam_n 4 across
    the cut), one finished beam that scores high and survives, one that
    scores low and is dropped. Image 1: <end> dominates every row, so all its
    beams finish at this step. Image 2: status 1 on entry, with a state no
    step would leave (unsorted scores, a live beam) to show nothing re-ranks
    it."""
    n_img, T, t, end = 3, 12, 5, 3
    out = _run_step(_finished_case(beam_n, V, t, T, n_img, end), beam_n, V, t, T, n_img, end)
    assert out["status"].tolist() == [0, 1, 1]
    assert out["fin"][beam_n:2 * beam_n].tolist() == [1] * beam_n
    if beam_n >= 4:
        # the surviving finished beam leads, unchanged; the low one is gone
        assert float(out["score"][0]) == -1.0 and int(out["blen"][0]) == 3 and int(out["fin"][0]) == 1
        assert int(out["tok"][0]) == end
        assert -1000.0 not in out["score"][:beam_n].tolist()
        assert out["tok"][1:4].tolist() == [7, 11, 7]  # (beam 0, 7), (beam 0, 11), (beam 1, 7)


def _finished_case(beam_n, V, t, T, n_img, end):
    g = torch.Generator().manual_seed(7 + beam_n * V)
    inp = _step_inputs(beam_n, V, t, T, n_img, g)
    R = n_img * beam_n
    inp["score"] = -20.0 - torch.rand(R, generator=g)
    lg = inp["logits"]
    lg[0, 7] = lg[0, 11] = lg[0].max() + 1
    if beam_n >= 4:
        lg[1] = lg[0]
        inp["score"][0] = inp["score"][1] = -18.0  # the four tied candidates lead the live ones
        hi, lo = beam_n - 2, beam_n - 1
        inp["fin"][hi] = inp["fin"][lo] = 1
        inp["score"][hi], inp["score"][lo] = -1.0, -1000.0
        inp["blen"][hi], inp["blen"][lo] = 3, 4
    lg[beam_n:2 * beam_n, end] = 30.0
    inp["status"][2] = 1
    inp["fin"][2 * beam_n:] = 1
    inp["fin"][2 * beam_n] = 0
    return inp


# ---------------------------------------------------------------- finalize
def _finalize_ref(hist, score, blen, fin, alpha, K, T):
    key = score / blen.clamp(min=1).float() ** alpha
    vals, order = torch.sort(key, descending=True, stable=True)
    toks = []
    for b in order.tolist():
        n = int(blen[b]) - int(fin[b])
        toks.append(hist[b, 1:1 + n].tolist())
    return vals, order, toks


def _finalize_case():
    K, T = 4, 12
    g = torch.Generator().manual_seed(3)
    hist = torch.randint(4, 200, (2 * K, T + 1), generator=g, dtype=torch.int32)
    # image 0: beams 0 and 2 tie (same score, same length) -> beam 0 first; the
    # long beam 1 overtakes them under length normalisation. image 1: a beam
    # that used all T positions, one of length 0, two finished ones.
    score = torch.tensor([-4.0, -5.0, -4.0, -9.0, -6.0, -50.0, -2.5, -2.0])
    blen = torch.tensor([3, 8, 3, 12, 12, 0, 6, 2], dtype=torch.int32)
    fin = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1], dtype=torch.int32)
    return K, T, hist, score, blen, fin


@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_beam_finalize(alpha):
    from fpnmt import _lib as L
    K, T, hist, score, blen, fin = _finalize_case()
    n_img = 2
    d = [x.to(DEV) for x in (hist, score, blen, fin)]
    ntok = torch.full((n_img, K, T), -7, dtype=torch.int32, device=DEV)
    nlen = torch.full((n_img, K), -7, dtype=torch.int32, device=DEV)
    nscore = torch.zeros((n_img, K), device=DEV)
    L.call("fpnmt_beam_finalize", n_img, K, d[0].data_ptr(), T + 1, d[1].data_ptr(), d[2].data_ptr(),
           d[3].data_ptr(), alpha, ntok.data_ptr(), T, nlen.data_ptr(), nscore.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    ntok, nlen, nscore = ntok.cpu(), nlen.cpu(), nscore.cpu()
    orders = []
    for i in range(n_img):
        rows = slice(i * K, (i + 1) * K)
        vals, order, toks = _finalize_ref(hist[rows], score[rows], blen[rows], fin[rows], alpha, K, T)
        orders.append(order.tolist())
        assert torch.allclose(nscore[i], vals, rtol=1e-5, atol=0)
        for k in range(K):
            assert int(nlen[i, k]) == len(toks[k])
            assert ntok[i, k, :len(toks[k])].tolist() == toks[k]
            assert ntok[i, k, len(toks[k]):].tolist() == [0] * (T - len(toks[k]))
    # the tie goes to the lower beam, and the two alphas rank differently
    assert orders[0].index(0) + 1 == orders[0].index(2)
    assert orders == ([[0, 2, 1, 3], [3, 2, 0, 1]] if alpha == 0.0 else [[1, 3, 0, 2], [2, 0, 3, 1]])


# ----------------------------------------------------------- whole decoder
def _pipeline(n_layers, vocab, image, seed, T, end_bias):
    """end_bias is added to <end>'s logit: random weights would otherwise
    never end a caption."""
    import fpnmt
    from fpnmt.layers import Init, invalidate_weights
    from utils.pipeline import Pipeline
    pl = Pipeline(max_seq_len=T, target_vocab_size=vocab, image_size=image, n_layers=n_layers, rate=0.0,
                  init=Init(torch.Generator().manual_seed(seed)), use_graph=False)
    with torch.no_grad():
        pl.transformer.final_layer.bias[pl.end_token] += end_bias
    invalidate_weights()
    return pl


def _cpu_logits(sd, cfg, enc, seqs):
    from oracle import ref_cpu as R
    tar = torch.tensor(seqs, dtype=torch.int64)
    logits, _ = R.transformer(sd, enc.repeat(len(seqs), 1, 1), tar, False, R.create_look_ahead_mask(tar.shape[1]), cfg)
    return logits[:, -1, :]


def cpu_beam_search(sd, cfg, enc, T, K, start, end):
    """The rule of fpnmt_beam_step_log, literally: every step re-runs the
    decoder on the live beams' whole prefixes. Returns the final beams
    (seqs, score, len, fin) and the smallest gap between the K-th and the
    (K+1)-th candidate met on the way."""
    V = sd["final_layer.kernel"].shape[1]
    seqs = [[start] for _ in range(K)]
    score = torch.full((K,), NEG)
    score[0] = 0.0
    blen = torch.zeros(K, dtype=torch.int64)
    fin = torch.zeros(K, dtype=torch.bool)
    margin = math.inf
    for t in range(T):
        if bool(fin.all()):
            break
        cand = torch.full((K, V), NEG)
        live = [b for b in range(K) if not fin[b] and score[b] > NEG]
        lp = torch.log_softmax(_cpu_logits(sd, cfg, enc, [seqs[b] for b in live]), -1)
        for n, b in enumerate(live):
            cand[b] = score[b] + lp[n]
        for b in range(K):
            if fin[b]:
                cand[b, end] = score[b]
        vals, idx = torch.sort(cand.reshape(-1), descending=True, stable=True)
        margin = min(margin, float(vals[K - 1] - vals[K]))
        par, tok = (idx[:K] // V).tolist(), (idx[:K] % V).tolist()
        seqs = [seqs[p] + [k] for p, k in zip(par, tok)]
        nfin = torch.tensor([bool(fin[p]) or k == end for p, k in zip(par, tok)])
        blen = torch.tensor([int(blen[p]) if fin[p] else t + 1 for p in par])
        score, fin = vals[:K].clone(), nfin
    return seqs, score, blen, fin, margin


def cpu_nbest(seqs, score, blen, fin, alpha):
    """[(ids, key)] best first, and the smallest gap between two keys."""
    key = score.double() / blen.clamp(min=1).double() ** alpha
    vals, order = torch.sort(key, descending=True, stable=True)
    gap = float((vals[:-1] - vals[1:]).min()) if len(vals) > 1 else math.inf
    out = []
    for b in order.tolist():
        n = int(blen[b]) - int(fin[b])
        out.append((seqs[b][1:1 + n], float(key[b]), int(blen[b])))
    return out, gap


def cpu_greedy(sd, cfg, enc, T, start, end):
    seq = [start]
    for _ in range(T):
        seq.append(int(torch.argmax(_cpu_logits(sd, cfg, enc, [seq])[0])))
        if seq[-1] == end:
            return seq[1:-1]
    return seq[1:]


# end_bias 3.0: the CPU search ends beams at lengths 1..4 on one image and leaves three running to T on the others
C_CFG = dict(n_layers=2, vocab=200, image=256, T=10, n_img=3, K=4, model_seed=13, image_seed=4, end_bias=3.0)


@pytest.fixture(scope="module")
def small_model():
    """The model of test (c) on the GPU, its weights for the CPU oracle, the
    images and the oracle's encoder output per image (computed once)."""
    import fpnmt
    from oracle import ref_cpu as R
    c = C_CFG
    fpnmt.set_precision("fp32")
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=c["n_layers"], num_heads=8, backbone="resnet50")
    imgs = torch.rand(c["n_img"], c["image"], c["image"], 3, generator=torch.Generator().manual_seed(c["image_seed"])) * 2 - 1
    encs = [R.encoder(sd, imgs[i][None], cfg) for i in range(c["n_img"])]
    beams = [cpu_beam_search(sd, cfg, encs[i], c["T"], c["K"], pl.start_token, pl.end_token) for i in range(c["n_img"])]
    return dict(pl=pl, sd=sd, cfg=cfg, imgs=imgs, encs=encs, beams=beams)


@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_decoder_matches_cpu_beam_search_fp32(small_model, alpha):
    """All n-best id lists of the cached, batched, graph-free decoder == the
    literal CPU search; scores within the fp32 logit bound (1e-3) per token.
    The CPU search's margins say the ids are not a matter of rounding."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    got = m["pl"].predict_batch(m["imgs"].to(DEV), c["T"], beam_n=c["K"], use_graph=False, mode="beam",
                                length_alpha=alpha, n_best=c["K"])
    for i in range(c["n_img"]):
        seqs, score, blen, fin, margin = m["beams"][i]
        ref, gap = cpu_nbest(seqs, score, blen, fin, alpha)
        print(f"image {i} alpha {alpha}: step margin {margin:.3e}, key gap {gap:.3e}, lens {blen.tolist()}")
        assert margin > 1e-3 and gap > 1e-3, (i, margin, gap)
        assert [ids for ids, _ in got[i]] == [ids for ids, _, _ in ref], (i, got[i], ref)
        for (_, s), (_, r, n) in zip(got[i], ref):
            assert abs(s - r) <= 1e-3 * max(n, 1), (i, s, r, n)


def test_beam_mode_behaviour(small_model):
    """Four distinct hypotheses per image; beam_n = 1 is the greedy decode;
    the default and mode="reference" are the reference's procedure (the
    oracle's literal predict(), as before)."""
    import fpnmt
    from oracle import ref_cpu as R
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    nb = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"])
    best = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam")
    one = pl.predict_batch(imgs, c["T"], beam_n=1, use_graph=False, mode="beam")
    dflt = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False)
    refm = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="reference")
    assert dflt == refm
    for i in range(c["n_img"]):
        hyps = [tuple(ids) for ids, _ in nb[i]]
        assert len(set(hyps)) == c["K"], hyps
        assert best[i] == nb[i][0][0]
        assert one[i] == cpu_greedy(m["sd"], m["cfg"], m["encs"][i], c["T"], pl.start_token, pl.end_token)
        ref = R.predict(m["sd"], m["imgs"][i], c["T"], m["cfg"], pl.start_token, pl.end_token, beam_n=c["K"])
        assert dflt[i] == ref.tolist(), (i, dflt[i], ref.tolist())
    with pytest.raises(ValueError):
        pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, n_best=2)  # reference mode has one result
    with pytest.raises(ValueError):
        pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"] + 1)


def test_beam_decode_graph_matches_eager_bf16():
    """Graph == eager == a second replay, n-best lists and scores, with
    images that stop at different steps inside the batch (a stopped image's
    rows stay as they are while the graphs replay for the others)."""
    import fpnmt
    fpnmt.set_precision("bf16")
    try:
        T, vocab, image, n_img, K = 12, 300, 224, 5, 8
        pl = _pipeline(2, vocab, image, 17, T, end_bias=3.2)  # measured: the images stop after 5, 3, 4, never, 8 steps
        g = torch.Generator().manual_seed(6)
        imgs = (torch.rand(n_img, image, image, 3, generator=g) * 2 - 1).to(DEV)
        kw = dict(beam_n=K, mode="beam", length_alpha=0.7, n_best=K)
        a = pl.predict_batch(imgs, T, use_graph=False, **kw)
        dec = pl._decoders[(n_img, K, T, False, "beam", 0.7)]
        done = dec.status.cpu().tolist()
        last = dec.blen.cpu().view(n_img, K).max(1).values.tolist()  # the step + 1 at which the last beam finished
        stop = [last[i] if done[i] else T + 1 for i in range(n_img)]
        print("stop steps", stop)
        assert len(set(stop)) > 1, stop
        b = pl.predict_batch(imgs, T, use_graph=True, **kw)
        c = pl.predict_batch(imgs, T, use_graph=True, **kw)  # replay of the captured graphs
        assert a == b == c
        assert all(len(ids) <= T for img in a for ids, _ in img)
    finally:
        fpnmt.set_precision("fp32")


# ------------------------------------------------------------- error paths
def test_beam_entry_points_reject_bad_arguments():
    from fpnmt import _lib as L
    n_img, K, V, T = 1, 4, 200, 12
    R = n_img * K
    f = torch.zeros(R * V, device=DEV)
    i1, i2, i3, i4, i5, i6 = (torch.zeros(R * (T + 1), dtype=torch.int32, device=DEV) for _ in range(6))
    sc = torch.zeros(R, device=DEV)

    def step(beam_n=K, vocab=V, score=sc.data_ptr(), t=0, hist_ld=T + 1):
        return L.lib.fpnmt_beam_step_log(n_img, beam_n, vocab, f.data_ptr(), vocab, score, i1.data_ptr(),
                                         i2.data_ptr(), i3.data_ptr(), i4.data_ptr(), hist_ld, t, i5.data_ptr(),
                                         i6.data_ptr(), T, 3, i1.data_ptr(), i2.data_ptr(), L.stream_ptr())

    for kw, word in ((dict(vocab=3), b"vocab"), (dict(beam_n=17), b"beam_n"), (dict(score=None), b"null"),
                     (dict(t=T, hist_ld=T + 1), b"width")):
        rc = step(**kw)
        assert rc < 0 and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    fin = lambda beam_n=K, score=sc.data_ptr(): L.lib.fpnmt_beam_finalize(  # noqa: E731
        n_img, beam_n, i3.data_ptr(), T + 1, score, i1.data_ptr(), i2.data_ptr(), 0.0, i4.data_ptr(), T,
        i5.data_ptr(), sc.data_ptr(), L.stream_ptr())
    for kw, word in ((dict(beam_n=17), b"beam_n"), (dict(score=None), b"null")):
        rc = fin(**kw)
        assert rc < 0 and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    torch.cuda.synchronize()

"""Diverse beam search (fpnmt_beam_step_groups, BeamDecoder(beam_groups=G),
predict_batch(beam_groups=..., diversity_penalty=..., group_best=...)): the
step kernel against the torch restatement of the rule (diverse_beam_ref.py)
and, where the rule says so, byte for byte against fpnmt_beam_step_log; the
whole decoder against a literal CPU diverse beam search on the oracle's
model; graph replay, constraints and an ensemble with groups; the call log
of the defaults; the entry point's error codes."""
import functools

import pytest
import torch

from diverse_beam_ref import NEG, NONE, assert_clear, cpu_diverse_beam_search, cpu_rank, groups_step_ref
from test_gpu_beam_search import _pipeline

pytestmark = pytest.mark.gpu

DEV = "cuda"
END = 3
N_IMG, T_TAB, T_POS = 3, 12, 5


# ------------------------------------------------------------ step kernel
def _tables(R, V, T, g):
    return dict(hist=torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32),
                src=torch.randint(0, R, (R, T), generator=g, dtype=torch.int32))


def _competing_inputs(K, G, V, n_img=N_IMG, T=T_TAB, t=T_POS):
    """Rows that make the groups compete: per image one base row 2 randn(1, V)
    plus 0.05 randn(K, V) per row (independent random rows never contend for
    a token), scores -0.1 rand(K)."""
    g = torch.Generator().manual_seed(300 + K * V + G)
    R = n_img * K
    logits = torch.cat([2 * torch.randn(1, V, generator=g) + 0.05 * torch.randn(K, V, generator=g)
                        for _ in range(n_img)])
    score = torch.cat([-0.1 * torch.rand(K, generator=g) for _ in range(n_img)])
    return dict(logits=logits, score=score, blen=torch.full((R,), t, dtype=torch.int32),
                fin=torch.zeros(R, dtype=torch.int32), status=torch.zeros(n_img, dtype=torch.int32),
                tok=torch.full((R,), 1, dtype=torch.int32), **_tables(R, V, T, g))


def _launch(inp, n_img, K, G, lam, V, t, T, end=END, entry="fpnmt_beam_step_groups"):
    """One launch on device copies of `inp`; every buffer back on the CPU
    (hout / sout: the out tables, pre-filled with -7)."""
    from fpnmt import _lib as L
    d = {k: v.clone().to(DEV) for k, v in inp.items()}
    hout, sout = torch.full_like(d["hist"], -7), torch.full_like(d["src"], -7)
    head = (n_img, K, G, lam, V) if entry == "fpnmt_beam_step_groups" else (n_img, K, V)
    L.call(entry, *head, d["logits"].data_ptr(), V, d["score"].data_ptr(), d["blen"].data_ptr(),
           d["fin"].data_ptr(), d["hist"].data_ptr(), hout.data_ptr(), T + 1, t, d["src"].data_ptr(), sout.data_ptr(),
           T, end, d["tok"].data_ptr(), d["status"].data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    out["hout"], out["sout"] = hout.cpu(), sout.cpu()
    return out


def _refs(inp, n_img, K, G, lam, t, end=END):
    out = []
    for i in range(n_img):
        rows = slice(i * K, (i + 1) * K)
        out.append(None if int(inp["status"][i]) else
                   groups_step_ref(inp["logits"][rows], inp["score"][rows], inp["blen"][rows], inp["fin"][rows], t,
                                   end, K, G, lam))
    return out


def _check(inp, out, refs, n_img, K, G, t, end=END, gap=1e-4):
    """Every image against the restatement (a frozen image: its own rows
    carried over and nothing else touched)."""
    Kg = K // G
    assert not bool(torch.isnan(out["score"]).any())
    for i in range(n_img):
        rows = slice(i * K, (i + 1) * K)
        own = torch.arange(i * K, (i + 1) * K, dtype=torch.int32)
        hout, sout = out["hout"], out["sout"]
        if refs[i] is None:
            for k in ("score", "blen", "fin", "tok"):
                assert torch.equal(out[k][rows], inp[k][rows]), (i, k)
            assert int(out["status"][i]) == 1
            assert torch.equal(hout[rows, :t + 1], inp["hist"][rows, :t + 1])
            assert torch.equal(hout[rows, t + 1], torch.full((K,), end, dtype=torch.int32))
            assert torch.equal(sout[rows, :t + 1], inp["src"][rows, :t + 1])
            assert torch.equal(sout[rows, t + 1], own)
            continue
        r = refs[i]
        assert_clear(r["sorted"], Kg, gap)
        par = torch.where(r["par"] == NONE, torch.arange(K), r["par"]) + i * K
        assert torch.equal(out["tok"][rows], r["tok"]), (i, out["tok"][rows], r["tok"])
        assert torch.equal(hout[rows, :t + 1], inp["hist"][par, :t + 1]), i
        assert torch.equal(hout[rows, t + 1], r["tok"]), i
        assert torch.equal(sout[rows, :t + 1], inp["src"][par, :t + 1]), i
        assert torch.equal(sout[rows, t + 1], own), i
        assert torch.equal(out["blen"][rows], r["blen"]), (i, out["blen"][rows], r["blen"])
        assert torch.equal(out["fin"][rows], r["fin"]), (i, out["fin"][rows], r["fin"])
        assert int(out["status"][i]) == int(r["fin"].all()), i
        assert torch.allclose(out["score"][rows], r["score"], rtol=1e-5, atol=0), (i, out["score"][rows], r["score"])


# (K, G, V). V 37, 203: scalar loads (203 odd); 200, 1000, 10000: 16-B loads, one to five per thread and row;
# Kg 1, 2, 3, 4 (list lengths 1, 2, 4); V 10000 hashes five tokens onto every filter bit
STEP_SHAPES = [(2, 2, 37), (4, 2, 37), (6, 3, 203), (8, 4, 200), (16, 4, 1000), (16, 16, 1000), (8, 2, 10000),
               (8, 8, 10000)]


@functools.lru_cache(maxsize=None)
def _competing_case(K, G, V, lam):
    inp = _competing_inputs(K, G, V)
    return inp, _refs(inp, N_IMG, K, G, lam, T_POS)


@pytest.mark.parametrize("lam", [0.5, 2.0])
@pytest.mark.parametrize("K,G,V", STEP_SHAPES)
def test_step_matches_the_rule(K, G, V, lam):
    """The kernel against the restatement on rows that compete, and the
    penalty at work: at least one slot differs from the lam = 0 selection."""
    inp, refs = _competing_case(K, G, V, lam)
    _, plain = _competing_case(K, G, V, 0.0)
    moved = sum(int(((a["par"] != b["par"]) | (a["tok"] != b["tok"])).sum()) for a, b in zip(refs, plain))
    print(f"K {K} G {G} V {V} lam {lam}: {moved} of {N_IMG * K} slots differ from lam 0")
    assert moved > 0
    out = _launch(inp, N_IMG, K, G, lam, V, T_POS, T_TAB)
    _check(inp, out, refs, N_IMG, K, G, T_POS)


def test_first_step_from_identical_rows():
    """t = 0 as the decoder starts it: score 0 on each group's first row,
    -inf elsewhere, all rows of an image the same (one prefix). With a
    penalty that outweighs the row's spread the eight beams take the row's
    eight best tokens, two per group, in order."""
    K, G, V, t, lam = 8, 4, 200, 0, 100.0
    Kg = K // G
    inp = _competing_inputs(K, G, V, t=t)
    for i in range(N_IMG):
        inp["logits"][i * K:(i + 1) * K] = inp["logits"][i * K]
    inp["score"].fill_(NEG)
    inp["score"][::Kg] = 0.0
    inp["blen"].zero_()
    refs = _refs(inp, N_IMG, K, G, lam, t)
    out = _launch(inp, N_IMG, K, G, lam, V, t, T_TAB)
    _check(inp, out, refs, N_IMG, K, G, t)
    assert bool(torch.isfinite(out["score"]).all())
    for i in range(N_IMG):
        best = torch.sort(inp["logits"][i * K], descending=True, stable=True).indices[:K]
        assert out["tok"][i * K:(i + 1) * K].tolist() == best.tolist()
        # every child descends from its group's first row, and carries the plain log-probability
        assert out["sout"][i * K:(i + 1) * K, 0].tolist() == [int(inp["src"][i * K + (k // Kg) * Kg, 0]) for k in range(K)]
        lp = torch.log_softmax(inp["logits"][i * K], -1)[best]
        assert torch.allclose(out["score"][i * K:(i + 1) * K], lp, rtol=1e-5, atol=0)


def _finished_case():
    """(8, 4, 200), t = 5, four images.
    Image 0: group 0 has a finished row that scores high and survives (it
    leads its group), group 1 one that scores low and is dropped.
    Image 1: group 0's live row 0 takes <end>; in group 1 row 2 is finished
    and carries itself at its own score, while live row 3's <end>, its best
    token by 1.0, loses lam = 2 and falls behind its second best.
    Image 2: <end> dominates every row: all groups finish (status 1).
    Image 3: status 1 on entry, in a state no step would leave."""
    K, G, V, n_img = 8, 4, 200, 4
    inp = _competing_inputs(K, G, V, n_img=n_img)
    g = torch.Generator().manual_seed(77)
    inp["score"] = -20.0 - torch.rand(n_img * K, generator=g)
    lg, sc, fin, blen = inp["logits"], inp["score"], inp["fin"], inp["blen"]
    fin[1], sc[1], blen[1] = 1, -1.0, 3
    fin[3], sc[3], blen[3] = 1, -1000.0, 4
    r = K  # image 1
    lg[r + 0, END] = lg[r + 0].max() + 30.0
    fin[r + 2], sc[r + 2], blen[r + 2] = 1, -1.0, 2
    top = lg[r + 3].max()
    lg[r + 3, END] = top + 1.0
    lg[2 * K:3 * K, END] = 40.0
    inp["status"][3] = 1
    fin[3 * K:] = 1
    fin[3 * K] = 0
    return inp, K, G, V, n_img


def test_finished_rows_end_token_and_frozen_image():
    lam, t = 2.0, T_POS
    inp, K, G, V, n_img = _finished_case()
    refs = _refs(inp, n_img, K, G, lam, t)
    out = _launch(inp, n_img, K, G, lam, V, t, T_TAB)
    _check(inp, out, refs, n_img, K, G, t)
    assert out["status"].tolist() == [0, 0, 1, 1]
    # image 0: the high finished row leads group 0 unchanged; the low one is gone from group 1
    assert float(out["score"][0]) == -1.0 and int(out["blen"][0]) == 3 and int(out["fin"][0]) == 1
    assert int(out["tok"][0]) == END and int(out["fin"][1]) == 0
    assert -1000.0 not in out["score"][:K].tolist() and out["fin"][2:4].tolist() == [0, 0]
    # image 1: row 0's child ended (a live child: counted); group 1 keeps the carry unpenalised and row 3
    # does not end, which it would without the penalty
    assert int(out["tok"][K]) == END and int(out["fin"][K]) == 1 and int(out["blen"][K]) == t + 1
    assert float(out["score"][K + 2]) == -1.0 and int(out["blen"][K + 2]) == 2 and int(out["tok"][K + 2]) == END
    assert int(out["tok"][K + 3]) != END and int(out["fin"][K + 3]) == 0
    free = _refs(inp, n_img, K, G, 0.0, t)[1]
    assert int(free["tok"][3]) == END and free["cnt"][END] >= 2
    assert refs[1]["cnt"][END] == 1
    # image 2: everything finished at this step
    assert out["fin"][2 * K:3 * K].tolist() == [1] * K and out["tok"][2 * K:3 * K].tolist() == [END] * K


def test_exact_tie_inside_a_group_goes_to_the_lower_flat_index():
    """(16, 4, 1000): rows 0, 1, 2 of group 0 are one row at one score with
    two equal maxima, six tied candidates for four rows: (0, 7), (0, 11),
    (1, 7), (1, 11) win. Group 1 then sees cnt 2 on both tokens."""
    K, G, V, t, lam = 16, 4, 1000, T_POS, 0.5
    inp = _competing_inputs(K, G, V)
    lg = inp["logits"]
    lg[0, 7] = lg[0, 11] = lg[0].max() + 1
    lg[1] = lg[0]
    lg[2] = lg[0]
    inp["score"][0:3] = 0.0
    refs = _refs(inp, N_IMG, K, G, lam, t)
    out = _launch(inp, N_IMG, K, G, lam, V, t, T_TAB)
    _check(inp, out, refs, N_IMG, K, G, t)
    assert out["tok"][:4].tolist() == [7, 11, 7, 11]
    assert out["sout"][:4, :t + 1].tolist() == inp["src"][[0, 0, 1, 1], :t + 1].tolist()
    assert refs[0]["cnt"][7] >= 2 and refs[0]["cnt"][11] >= 2


# ---------------------------------------------------------- byte equality
BUFFERS = ("tok", "hout", "sout", "blen", "fin", "score")


def _bytes_equal(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def _mixed_inputs(K, G, V):
    """The competing rows with a finished row, a row at -inf and one image
    frozen on entry."""
    inp = _competing_inputs(K, G, V)
    inp["fin"][1], inp["score"][1], inp["blen"][1] = 1, -0.01, 2
    inp["score"][K - 1] = NEG
    return inp


@pytest.mark.parametrize("K,V", [(8, 200), (16, 1000)])
def test_one_group_is_beam_step_log_byte_for_byte(K, V):
    inp = _mixed_inputs(K, 1, V)
    inp["status"][2] = 1
    a = _launch(inp, N_IMG, K, 1, 3.0, V, T_POS, T_TAB)
    b = _launch(inp, N_IMG, K, 1, 0.0, V, T_POS, T_TAB, entry="fpnmt_beam_step_log")
    _bytes_equal(a, b, BUFFERS + ("status",))
    assert a["status"].tolist() == [0, 0, 1]


@pytest.mark.parametrize("K,G,V", [(8, 4, 200), (8, 2, 10000)])
def test_zero_penalty_is_beam_step_log_per_group_byte_for_byte(K, G, V):
    """lam = 0: the groups are independent searches over Kg rows, so
    fpnmt_beam_step_log(n_images * G, Kg, ...) on the same buffers writes the
    same bytes (status apart: it is per image there, per group here)."""
    inp = _mixed_inputs(K, G, V)
    a = _launch(inp, N_IMG, K, G, 0.0, V, T_POS, T_TAB)
    per_group = dict(inp, status=torch.zeros(N_IMG * G, dtype=torch.int32))
    b = _launch(per_group, N_IMG * G, K // G, 1, 0.0, V, T_POS, T_TAB, entry="fpnmt_beam_step_log")
    _bytes_equal(a, b, BUFFERS)


# ----------------------------------------------------------- whole decoder
# One seed per image, chosen with end_bias on the CPU oracle so that every cut margin and ranking-key gap of the
# searches below exceeds 2e-3 (two groups often end up with the same caption, a key gap of exactly 0, or meet a
# cut closer than 1e-3; these images do neither). Seed 105 ends beams at lengths 1..4 and leaves two running.
D_CFG = dict(n_layers=2, vocab=200, image=256, T=10, n_img=3, model_seed=13, image_seeds=(105, 104, 113),
             end_bias=3.0, lam=0.5, alpha=0.7)
D_GROUPS = [(4, 2), (6, 3)]


@pytest.fixture(scope="module")
def small_model():
    """The small model of the beam-search test on the GPU, its weights for
    the CPU oracle, the images and the oracle's encoder output per image,
    and the CPU diverse searches (all computed once)."""
    import fpnmt
    from oracle import ref_cpu as R
    c = D_CFG
    fpnmt.set_precision("fp32")
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=c["n_layers"], num_heads=8, backbone="resnet50")
    imgs = torch.stack([torch.rand(c["image"], c["image"], 3, generator=torch.Generator().manual_seed(s))
                        for s in c["image_seeds"]]) * 2 - 1
    encs = [R.encoder(sd, imgs[i][None], cfg) for i in range(c["n_img"])]
    beams = {(K, G): [cpu_diverse_beam_search(sd, cfg, encs[i], c["T"], K, G, c["lam"], pl.start_token, pl.end_token)
                      for i in range(c["n_img"])] for K, G in D_GROUPS}
    return dict(pl=pl, imgs=imgs, beams=beams)


@pytest.mark.parametrize("K,G", D_GROUPS)
def test_decoder_matches_cpu_diverse_beam_search_fp32(small_model, K, G):
    """Every beam of the cached, batched, graph-free decoder == the literal
    CPU search: ids, lengths, fin, scores within the fp32 logit bound (1e-3)
    per token; n-best over all K and group_best equal the CPU rankings. The
    CPU search's margins say the ids are not a matter of rounding."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, D_CFG
    pl, imgs, Kg = m["pl"], m["imgs"].to(DEV), K // G
    kw = dict(beam_n=K, use_graph=False, mode="beam", length_alpha=c["alpha"], beam_groups=G,
              diversity_penalty=c["lam"])
    nbest = pl.predict_batch(imgs, c["T"], n_best=K, **kw)
    dec = pl._decoders[(c["n_img"], K, c["T"], False, "beam", c["alpha"], "groups", G, c["lam"])]
    blen, fin, score = dec.blen.cpu().view(-1, K), dec.fin.cpu().view(-1, K), dec.score.cpu().view(-1, K)
    hist = dec.hist[c["T"] % 2].cpu().view(c["n_img"], K, -1)
    gbest = pl.predict_batch(imgs, c["T"], group_best=True, **kw)
    for i in range(c["n_img"]):
        seqs, rscore, rlen, rfin, margin = m["beams"][(K, G)][i]
        ref, gap = cpu_rank(seqs, rscore, rlen, rfin, c["alpha"], range(K))
        groups = [cpu_rank(seqs, rscore, rlen, rfin, c["alpha"], range(g * Kg, (g + 1) * Kg)) for g in range(G)]
        gap = min([gap] + [x[1] for x in groups])
        print(f"image {i} K {K} G {G}: cut margin {margin:.3e}, key gap {gap:.3e}, lens {rlen.tolist()}")
        assert margin > 1e-3 and gap > 1e-3, (i, margin, gap)
        assert torch.equal(blen[i], rlen) and torch.equal(fin[i], rfin), (i, blen[i], rlen, fin[i], rfin)
        for b in range(K):
            n = int(rlen[b])
            assert hist[i, b, :n + 1].tolist() == seqs[b][:n + 1], (i, b)
            assert abs(float(score[i, b]) - float(rscore[b])) <= 1e-3 * max(n, 1), (i, b)
        assert [ids for ids, _ in nbest[i]] == [ids for ids, _, _ in ref], (i, nbest[i], ref)
        for (_, s), (_, r, n) in zip(nbest[i], ref):
            assert abs(s - r) <= 1e-3 * max(n, 1), (i, s, r, n)
        assert len(gbest[i]) == G
        for (ids, s), (rk, _) in zip(gbest[i], groups):
            assert ids == rk[0][0] and abs(s - rk[0][1]) <= 1e-3 * max(rk[0][2], 1), (i, ids, s, rk[0])
    with pytest.raises(ValueError):
        pl.predict_batch(imgs, c["T"], group_best=True, n_best=2, **kw)


def _bf16_model():
    T, vocab, image, n_img, K = 12, 300, 224, 5, 8
    pl = _pipeline(2, vocab, image, 17, T, end_bias=3.2)
    imgs = (torch.rand(n_img, image, image, 3, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV)
    return pl, imgs, T, n_img, K


def _bigram_repeats(ids, start):
    seq = [start] + list(ids)
    grams = list(zip(seq, seq[1:]))
    return len(grams) != len(set(grams))


def test_diverse_decode_behaviour_bf16():
    """Graph == eager == a second replay with images that stop at different
    steps; one beam per group and lam = 2: the beams of an image start with
    pairwise different tokens; constraints and a two-model ensemble run with
    groups and keep their own promises."""
    import fpnmt
    fpnmt.set_precision("bf16")
    try:
        pl, imgs, T, n_img, K = _bf16_model()
        kw = dict(beam_n=K, mode="beam", length_alpha=0.7, n_best=K, beam_groups=4, diversity_penalty=0.5)
        a = pl.predict_batch(imgs, T, use_graph=False, **kw)
        dec = pl._decoders[(n_img, K, T, False, "beam", 0.7, "groups", 4, 0.5)]
        done = dec.status.cpu().tolist()
        last = dec.blen.cpu().view(n_img, K).max(1).values.tolist()
        stop = [last[i] if done[i] else T + 1 for i in range(n_img)]
        print("stop steps", stop)
        assert len(set(stop)) > 1, stop
        b = pl.predict_batch(imgs, T, use_graph=True, **kw)
        c = pl.predict_batch(imgs, T, use_graph=True, **kw)  # replay of the captured graphs
        assert a == b == c
        assert a != pl.predict_batch(imgs, T, use_graph=False, beam_n=K, mode="beam", length_alpha=0.7, n_best=K)
        # one beam per group
        one = pl.predict_batch(imgs, T, use_graph=False, beam_n=K, mode="beam", beam_groups=K, diversity_penalty=2.0,
                               group_best=True)
        for img in one:
            firsts = [(ids + [pl.end_token])[0] for ids, _ in img]  # an empty caption started with <end>
            assert len(set(firsts)) == K, firsts
        # constraints and an ensemble
        other = _pipeline(1, 300, 224, 18, T, end_bias=1.0)
        cons = dict(no_repeat_ngram=2, min_len=3)
        nb = pl.predict_batch(imgs, T, use_graph=False, ensemble=[other], **kw, **cons)
        assert nb != a
        dec, = [d for k, d in pl._decoders.items() if "ensemble" in k and "groups" in k]
        fin = dec.fin.cpu().bool()
        assert bool(fin.any())
        assert bool((dec.blen.cpu()[fin] >= 4).all())  # min_len 3 tokens, then <end>
        for img in nb:
            for ids, s in img:
                assert not _bigram_repeats(ids, pl.start_token), ids
                assert s < 0.0
    finally:
        fpnmt.set_precision("fp32")


# ---------------------------------------------------------------- call log
def test_call_log_and_decoder_keys(small_model, monkeypatch):
    """The defaults launch fpnmt_beam_step_log T times under the key they
    always had and never the new entry point; with groups the new one runs T
    times as the last launch of each position, after fpnmt_logits_constrain
    when constrained."""
    import fpnmt
    from fpnmt import decode as D
    fpnmt.set_precision("fp32")
    m, c = small_model, D_CFG
    pl, imgs, T, K = m["pl"], m["imgs"].to(DEV), D_CFG["T"], 4
    names = []
    real = D.call
    monkeypatch.setattr(D, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    before = set(getattr(pl, "_decoders", {}))
    base = dict(beam_n=K, use_graph=False, mode="beam", length_alpha=0.25)
    pl.predict_batch(imgs, T, **base)
    pl.predict_batch(imgs, T, beam_groups=1, diversity_penalty=0.0, group_best=False, **base)
    assert set(pl._decoders) - before == {(c["n_img"], K, T, False, "beam", 0.25)}
    assert names.count("fpnmt_beam_step_log") == 2 * T and "fpnmt_beam_step_groups" not in names
    del names[:]
    pl.predict_batch(imgs, T, beam_groups=2, diversity_penalty=0.5, min_len=T - 1, **base)
    steps = [i for i, n in enumerate(names) if n == "fpnmt_beam_step_groups"]
    assert len(steps) == T and "fpnmt_beam_step_log" not in names
    assert names.count("fpnmt_logits_constrain") == T
    assert all(names[i - 1] == "fpnmt_logits_constrain" for i in steps)
    # the last launch of its position: after the last one only the ranking is left
    assert names[steps[-1] + 1:] == ["fpnmt_beam_finalize"]
    for bad in (dict(mode="sample", beam_groups=2), dict(mode="reference", beam_groups=2),
                dict(mode="reference", diversity_penalty=0.5), dict(mode="sample", group_best=True),
                dict(mode="reference", group_best=True), dict(mode="beam", beam_groups=3),
                dict(mode="beam", diversity_penalty=0.5), dict(mode="beam", beam_groups=2, diversity_penalty=-1.0)):
        with pytest.raises(ValueError):
            pl.predict_batch(imgs, T, beam_n=K, use_graph=False, **bad)


# ------------------------------------------------------------- error paths
def test_beam_step_groups_rejects_bad_arguments():
    from fpnmt import _lib as L
    n_img, K, V, T = 1, 4, 200, 12
    R = n_img * K
    f = torch.zeros(R * V, device=DEV)
    i1, i2, i3, i4, i5, i6 = (torch.zeros(R * (T + 1), dtype=torch.int32, device=DEV) for _ in range(6))
    sc = torch.zeros(R, device=DEV)

    def step(beam_n=K, groups=2, lam=0.5, vocab=V, score=sc.data_ptr(), t=0, hist_ld=T + 1, end=3):
        return L.lib.fpnmt_beam_step_groups(n_img, beam_n, groups, lam, vocab, f.data_ptr(), vocab, score,
                                            i1.data_ptr(), i2.data_ptr(), i3.data_ptr(), i4.data_ptr(), hist_ld, t,
                                            i5.data_ptr(), i6.data_ptr(), T, end, i1.data_ptr(), i2.data_ptr(),
                                            L.stream_ptr())

    for kw, code, word in ((dict(vocab=3), L.E_ARG, b"vocab"), (dict(beam_n=17, groups=1), L.E_UNSUPPORTED, b"beam_n"),
                           (dict(score=None), L.E_ARG, b"null"), (dict(t=T, hist_ld=T + 1), L.E_ARG, b"width"),
                           (dict(end=V), L.E_ARG, b"end_token"), (dict(groups=0), L.E_ARG, b"groups"),
                           (dict(groups=-1), L.E_ARG, b"groups"), (dict(groups=3), L.E_ARG, b"groups"),
                           (dict(groups=8), L.E_ARG, b"groups"), (dict(lam=-0.5), L.E_ARG, b"diversity_penalty"),
                           (dict(lam=float("nan")), L.E_ARG, b"diversity_penalty"),
                           (dict(lam=float("inf")), L.E_ARG, b"diversity_penalty")):
        rc = step(**kw)
        assert rc == code and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    torch.cuda.synchronize()

"""Constrained decoding (fpnmt_logits_constrain, BeamDecoder / SampleDecoder /
predict_batch with no_repeat_ngram, repetition_penalty, min_len,
banned_tokens): the kernel bitwise against the numpy statement of the rule
(tests/constrain_ref.py) across the wave boundary of the history, finished
rows, out-of-range ids and the error codes; the whole decoder against a
literal constrained CPU beam search on the oracle's model, the properties of
every returned hypothesis, greedy agreement of the three decoders, the
unconstrained defaults, and graph replay."""
import math

import numpy as np
import pytest
import torch

from constrain_ref import banned_set, constrain_ref
from test_gpu_beam_search import C_CFG, _cpu_logits, _pipeline, cpu_nbest

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = float("-inf")
SENT = np.float32(12345.0)  # padding columns and the guard row: never written

# --------------------------------------------------------------- the kernel
ROWS, VOCAB, LDL, T_HIST, END = 5, 203, 208, 70, 3
POSITIONS = [0, 1, 2, 7, 62, 63, 64, 65]  # t + 1 = 64 / 65: one wave's lanes stop covering the history
TOKENS = list(range(4, 16))  # 12 distinct tokens: repeats and repeated n-grams are frequent
BANNED_LISTS = {0: [], 3: [5, 9, 150], 130: [5, 9] + list(range(60, 188))}  # 130 ids: more than one wave's lanes
_COUNTS = {"banned_by_ngram": 0, "penalised_repeats": 0}


def _buffer(logits):
    """(rows + 1, LDL): the logits, sentinel padding columns, one sentinel guard row."""
    rows, vocab = logits.shape
    buf = np.full((rows + 1, LDL), SENT, dtype=np.float32)
    buf[:rows, :vocab] = logits
    return buf


def _launch(buf, rows, vocab, hist, t, fin, g, p, min_len, end, banned, expect=0):
    """fpnmt_logits_constrain on a device copy of buf; returns the whole buffer back."""
    from fpnmt import _lib as L
    d = torch.from_numpy(buf.copy()).to(DEV)
    h = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).to(DEV)
    f = None if fin is None else torch.tensor(fin, dtype=torch.int32, device=DEV)
    b = torch.tensor(banned, dtype=torch.int32, device=DEV) if len(banned) else None
    rc = L.lib.fpnmt_logits_constrain(rows, vocab, d.data_ptr(), buf.shape[1], h.data_ptr(), hist.shape[1], t,
                                      L.ptr(f), g, p, min_len, end, L.ptr(b), len(banned), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib.fpnmt_last_error())
    return d.cpu().numpy()


def _reference(buf, rows, vocab, hist, t, fin, g, p, min_len, end, banned):
    ref = buf.copy()
    for r in range(rows):
        ref[r, :vocab] = constrain_ref(buf[r, :vocab], hist[r], t, 0 if fin is None else fin[r], g, p, min_len, end,
                                       banned)
    return ref


def _check(buf, rows, vocab, hist, t, fin, g, p, min_len, end, banned, what):
    """Kernel == constrain_ref as uint32 over the WHOLE buffer: the padding
    columns and the guard row hold their sentinel in both."""
    ref = _reference(buf, rows, vocab, hist, t, fin, g, p, min_len, end, banned)
    got = _launch(buf, rows, vocab, hist, t, fin, g, p, min_len, end, banned)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (what, bad[:8].tolist(), [(float(got[i, j]), float(ref[i, j])) for i, j in bad[:8]])
    assert (got[:rows, vocab:] == SENT).all() and (got[rows] == SENT).all(), what
    return ref


def _random_case(t):
    g = np.random.default_rng(500 + t)
    logits = (g.standard_normal((ROWS, VOCAB)) * 3).astype(np.float32)
    hist = g.choice(TOKENS, size=(ROWS, T_HIST + 1)).astype(np.int32)
    hist[:, 0] = 1  # <start>
    return logits, hist


@pytest.mark.parametrize("t", POSITIONS)
def test_kernel_matches_the_rule_bitwise(t):
    """g x p x min_len x banned list at one position, random histories over
    12 tokens, rows 1 and 3 finished in half of the settings."""
    logits, hist = _random_case(t)
    buf = _buffer(logits)
    n = 0
    for g in (0, 1, 2, 3, 4):
        for p in (1.0, 1.3):
            for min_len in (0, t, t + 1):
                for nb, banned in BANNED_LISTS.items():
                    fin = [0, 1, 0, 1, 0] if n % 2 else None
                    n += 1
                    ref = _check(buf, ROWS, VOCAB, hist, t, fin, g, p, min_len, END, banned,
                                 dict(t=t, g=g, p=p, min_len=min_len, nb=nb, fin=fin))
                    if fin is not None:  # finished rows: bit-identical before and after
                        assert (ref[[1, 3]].view(np.uint32) == buf[[1, 3]].view(np.uint32)).all()
                    for r in range(ROWS):
                        if fin is not None and fin[r]:
                            continue
                        if g:
                            _COUNTS["banned_by_ngram"] += len(banned_set(hist[r], t, VOCAB, g, 0, END, ()))
                        if p != 1.0:
                            seen = hist[r, :t + 1].tolist()
                            rep = {j for j in seen if seen.count(j) > 1}
                            _COUNTS["penalised_repeats"] += sum(
                                1 for j in rep if ref[r, j] != NEG and ref[r, j] != buf[r, j])


def test_case_set_bans_and_penalises():
    """The random cases above prove something: the reference banned tokens by
    the n-gram rule and penalised tokens that occur more than once. Runs the
    longest position itself when selected alone."""
    if not _COUNTS["banned_by_ngram"]:
        test_kernel_matches_the_rule_bitwise(65)
    print("case set:", _COUNTS)
    assert _COUNTS["banned_by_ngram"] > 0 and _COUNTS["penalised_repeats"] > 0, _COUNTS


def test_kernel_known_answers():
    """The hand-written histories of tests/test_constrain_rule.py through the kernel."""
    S, A, B = 1, 5, 6
    logits, _ = _random_case(0)
    buf = _buffer(logits)

    def banned_cols(h, g):
        hist = np.zeros((ROWS, T_HIST + 1), dtype=np.int32)
        hist[:] = np.array(h + [0] * (T_HIST + 1 - len(h)), dtype=np.int32)
        got = _check(buf, ROWS, VOCAB, hist, len(h) - 1, None, g, 1.0, 0, END, [], (h, g))
        cols = {tuple(np.nonzero(np.isneginf(got[r, :VOCAB]))[0].tolist()) for r in range(ROWS)}
        assert len(cols) == 1
        return set(cols.pop())

    assert banned_cols([S, A, B, A], 2) == {B}
    assert banned_cols([S, A, A, A], 2) == {A}  # the overlapping match at the last admissible i
    assert banned_cols([S, B, A, A], 2) == {A}
    assert banned_cols([S, A, B, A], 1) == {S, A, B}
    assert banned_cols([A, A, A, A], 4) == {A}
    assert banned_cols([A, A, A, A], 5) == set()  # g = t + 2


def test_kernel_penalty_edge_values_and_ban_beats_penalty():
    """+0, -0, -inf and NaN at penalised columns; a token seen three times is
    penalised once; a token in the history AND the banned list with a
    positive logit ends at -inf."""
    logits, hist = _random_case(7)
    t = 7
    hist[:, 1:8] = np.array([20, 21, 22, 23, 24, 24, 24], dtype=np.int32)
    logits[:, 20], logits[:, 21], logits[:, 22], logits[:, 23], logits[:, 24] = 0.0, -0.0, NEG, np.nan, 5.0
    logits[1, 24] = -5.0
    buf = _buffer(logits)
    got = _check(buf, ROWS, VOCAB, hist, t, None, 0, 1.3, 0, END, [], "edge values")
    want = np.array([0.0, -0.0, NEG, np.nan, np.float32(5.0) / np.float32(1.3)], dtype=np.float32)
    assert (got[0, 20:25].view(np.uint32) == want.view(np.uint32)).all()
    assert got[1, 24] == np.float32(-5.0) * np.float32(1.3)
    got = _check(buf, ROWS, VOCAB, hist, t, None, 0, 1.3, 0, END, [24, 100], "ban beats penalty")
    assert (got[:ROWS, 24] == NEG).all() and (got[:ROWS, 100] == NEG).all()
    got = _check(buf, ROWS, VOCAB, hist, t, None, 2, 1.3, 0, END, [], "n-gram ban beats penalty")
    assert (got[:ROWS, 24] == NEG).all()  # 24 24 was seen, the last token is 24


def test_kernel_ignores_out_of_range_ids():
    """vocab + 1 in every row's history and -2 on rows >= 1: without the range
    check the first would index a padding column of its own row and the second
    a padding column of the row before — sentinels inside the allocation."""
    for t in (7, 65):
        logits, hist = _random_case(t)
        hist[:, 2] = VOCAB + 1
        hist[1:, 4] = -2
        if t == 7:
            hist[:, t] = VOCAB + 1  # the n-gram tail holds it, and an earlier position equals it by value
        else:
            hist[:, 39] = hist[:, t]  # the tail matches at 39 and the token after it is no column
            hist[:, 40] = VOCAB + 1
            hist[2:, t - 1] = -2
        buf = _buffer(logits)
        for g in (1, 2, 3):
            _check(buf, ROWS, VOCAB, hist, t, None, g, 1.3, 0, END, [VOCAB + 1, 9, VOCAB, 205], (t, g))


def test_kernel_all_rules_off_and_single_rows():
    logits, hist = _random_case(7)
    buf = _buffer(logits)
    got = _launch(buf, ROWS, VOCAB, hist, 7, None, 0, 1.0, 7, END, [])  # min_len <= t
    assert (got.view(np.uint32) == buf.view(np.uint32)).all()
    for rows in (1, 4):  # a block that is not full, and exactly one block
        b = _buffer(logits[:rows])
        _check(b, rows, VOCAB, hist[:rows], 7, None, 2, 1.3, 9, END, [5], rows)


def test_constrain_entry_rejects_bad_arguments():
    from fpnmt import _lib as L
    f = torch.zeros(ROWS * LDL, device=DEV)
    h = torch.zeros(ROWS * 2000, dtype=torch.int32, device=DEV)
    bl = torch.zeros(5000, dtype=torch.int32, device=DEV)
    before = f.clone()

    def go(rows=ROWS, vocab=VOCAB, logits=f.data_ptr(), ldl=LDL, hist=h.data_ptr(), hist_ld=T_HIST + 1, t=5, g=2,
           p=1.3, min_len=0, end=END, banned=None, n_banned=0):
        return L.lib.fpnmt_logits_constrain(rows, vocab, logits, ldl, hist, hist_ld, t, None, g, p, min_len, end,
                                            banned, n_banned, L.stream_ptr())

    bad = [(dict(logits=None), b"null"), (dict(hist=None), b"null"), (dict(rows=0), b"rows"), (dict(rows=-1), b"rows"),
           (dict(vocab=0), b"vocab"), (dict(ldl=VOCAB - 1), b"ldl"), (dict(t=-1), b"position"),
           (dict(t=T_HIST + 1), b"width"), (dict(g=-1), b"no_repeat_ngram"), (dict(min_len=-1), b"min_len"),
           (dict(p=0.0), b"repetition_penalty"), (dict(p=-1.0), b"repetition_penalty"),
           (dict(p=float("inf")), b"repetition_penalty"), (dict(p=float("nan")), b"repetition_penalty"),
           (dict(end=VOCAB), b"end_token"), (dict(end=-1), b"end_token"),
           (dict(n_banned=-1, banned=bl.data_ptr()), b"n_banned"), (dict(n_banned=2), b"banned")]
    for kw, word in bad:
        rc = go(**kw)
        assert rc == L.E_ARG and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    rc = go(t=L.CONSTRAIN_MAX_LEN, hist_ld=2000)
    assert rc == L.E_UNSUPPORTED and b"1024" in L.lib.fpnmt_last_error(), rc
    rc = go(banned=bl.data_ptr(), n_banned=L.CONSTRAIN_MAX_BANNED + 1)
    assert rc == L.E_UNSUPPORTED and b"4096" in L.lib.fpnmt_last_error(), rc
    assert go(t=L.CONSTRAIN_MAX_LEN - 1, hist_ld=2000, g=0, p=1.0) == 0  # the last supported position, rules off
    torch.cuda.synchronize()
    assert torch.equal(f, before)


# ----------------------------------------------------------- whole decoder
# The model of the beam tests (tests/test_gpu_beam_search.py C_CFG: 2 layers, V 200, 256^2, T 10, 3 images, K 4,
# model_seed 13, end_bias 3.0) meets both conditions with g = 2, so nothing else was chosen. The CPU searches'
# margins per image (smallest gap between the K-th and the (K+1)-th candidate / smallest key gap), all > 1e-3:
#   min_len 6:        4.0e-2 / 2.3e-2,  7.7e-3 / 1.4e-2,  3.1e-3 / 6.6e-3
#   no_repeat_ngram 2: 5.9e-2 / 2.4e-2,  8.8e-3 / 3.3e-2,  1.9e-2 / 2.6
#   penalty 1.3:      1.3e-1 / 4.7e-3,  6.7e-2 / 2.0e-3,  4.8e-2 / 2.1e-2
#   all three:        4.4e-3 / 1.3e-2,  4.2e-3 / 1.2e-3,  2.0e-3 / 8.1e-3
# (g = 1 and g = 3 miss the bound on this model: key gaps 6.1e-4 and, with all three, 5.3e-5.)
# Each binds: the unconstrained search returns the empty caption on every image (shorter than 6), repeats the
# bigram 122 122 or 105 105 on images 0 and 1, and returns other ids than the penalised search on every image.
CONS = {
    "min_len": dict(min_len=6),
    "ngram": dict(no_repeat_ngram=2),
    "penalty": dict(repetition_penalty=1.3),
    "all": dict(min_len=6, no_repeat_ngram=2, repetition_penalty=1.3),
}
FULL = dict(no_repeat_ngram=0, repetition_penalty=1.0, min_len=0, banned_tokens=())


def _cons(kw):
    return dict(FULL, **kw)


def _constrained_lp(sd, cfg, enc, seqs, t, end, cons):
    """log_softmax of every prefix's last-position logits after constrain_ref."""
    logits = _cpu_logits(sd, cfg, enc, seqs).float().numpy()
    rows = [constrain_ref(logits[n], seqs[n], t, 0, cons["no_repeat_ngram"], cons["repetition_penalty"],
                          cons["min_len"], end, cons["banned_tokens"]) for n in range(len(seqs))]
    return torch.log_softmax(torch.from_numpy(np.stack(rows)), -1)


def cpu_beam_search_constrained(sd, cfg, enc, T, K, start, end, cons):
    """cpu_beam_search of the beam tests with constrain_ref applied to each
    live beam's logits row before log_softmax; nothing else differs."""
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
        lp = _constrained_lp(sd, cfg, enc, [seqs[b] for b in live], t, end, cons)
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


def cpu_greedy_constrained(sd, cfg, enc, T, start, end, cons):
    seq = [start]
    for t in range(T):
        seq.append(int(torch.argmax(_constrained_lp(sd, cfg, enc, [seq], t, end, cons)[0])))
        if seq[-1] == end:
            return seq[1:-1]
    return seq[1:]


def violates(ids, T, start, cons):
    """A returned hypothesis (ids without <start> / <end>) against the properties."""
    if len(ids) < cons["min_len"] and len(ids) != T:
        return "shorter than min_len"
    g = cons["no_repeat_ngram"]
    if g:
        full = [start] + list(ids)
        grams = [tuple(full[i:i + g]) for i in range(len(full) - g + 1)]
        if len(set(grams)) != len(grams):
            return f"a {g}-gram occurs twice"
    if set(ids) & set(cons["banned_tokens"]):
        return "a banned id"
    return None


@pytest.fixture(scope="module")
def small_model():
    import fpnmt
    from oracle import ref_cpu as R
    c = C_CFG
    fpnmt.set_precision("fp32")
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=c["n_layers"], num_heads=8, backbone="resnet50")
    imgs = torch.rand(c["n_img"], c["image"], c["image"], 3, generator=torch.Generator().manual_seed(c["image_seed"])) * 2 - 1
    encs = [R.encoder(sd, imgs[i][None], cfg) for i in range(c["n_img"])]
    return dict(pl=pl, sd=sd, cfg=cfg, imgs=imgs, encs=encs, cache={})


def _cpu_search(m, name):
    """The CPU search of every image under CONS[name] ("none": unconstrained), computed once."""
    if name not in m["cache"]:
        c, pl = C_CFG, m["pl"]
        cons = _cons(CONS.get(name, {}))
        m["cache"][name] = [cpu_beam_search_constrained(m["sd"], m["cfg"], m["encs"][i], c["T"], c["K"],
                                                        pl.start_token, pl.end_token, cons) for i in range(c["n_img"])]
    return m["cache"][name]


@pytest.mark.parametrize("name", list(CONS))
def test_decoder_matches_constrained_cpu_beam_search_fp32(small_model, name):
    """n-best id lists == the literal constrained CPU search, scores within
    the fp32 logit bound (1e-3) per token; the CPU search's margins exceed
    that bound (condition 1) and the constraint binds: the unconstrained CPU
    search violates it or gives other ids on some image (condition 2)."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl = m["pl"]
    cons = _cons(CONS[name])
    got = pl.predict_batch(m["imgs"].to(DEV), c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"],
                           **CONS[name])
    binds = False
    for i in range(c["n_img"]):
        seqs, score, blen, fin, margin = _cpu_search(m, name)[i]
        ref, gap = cpu_nbest(seqs, score, blen, fin, 0.0)
        free, _ = cpu_nbest(*_cpu_search(m, "none")[i][:4], 0.0)
        broke = [violates(ids, c["T"], pl.start_token, cons) for ids, _, _ in free]
        binds = binds or any(broke) or [ids for ids, _, _ in free] != [ids for ids, _, _ in ref]
        print(f"{name} image {i}: step margin {margin:.3e}, key gap {gap:.3e}, lens {blen.tolist()}, "
              f"unconstrained search: {broke}")
        assert margin > 1e-3 and gap > 1e-3, (i, margin, gap)
        assert [ids for ids, _ in got[i]] == [ids for ids, _, _ in ref], (i, got[i], ref)
        for (ids, s), (_, r, n) in zip(got[i], ref):
            assert abs(s - r) <= 1e-3 * max(n, 1), (i, s, r, n)
            assert violates(ids, c["T"], pl.start_token, cons) is None, (i, ids)
    assert binds, name


PROP = dict(no_repeat_ngram=2, repetition_penalty=1.2, min_len=5, banned_tokens=(0, 7, 11, 23))


def test_every_hypothesis_keeps_the_constraints(small_model):
    """Beam (all K hypotheses) and sample (6 samples, top_p 0.9, 2 seeds):
    long enough, no repeated g-gram of <start> + ids, no banned id."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    hyps = []
    for g in (1, 2, 3):
        kw = dict(PROP, no_repeat_ngram=g)
        nb = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"], **kw)
        hyps += [(kw, ids, s) for img in nb for ids, s in img]
        for seed in (1, 2):
            sm = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=6, top_p=0.9, seed=seed, **kw)
            hyps += [(kw, ids, s) for img in sm for ids, s in img]
    assert len(hyps) == 3 * (c["n_img"] * c["K"] + 2 * c["n_img"] * 6)
    for kw, ids, s in hyps:
        assert violates(ids, c["T"], pl.start_token, kw) is None, (kw, ids)
        assert math.isfinite(s) and s < 0.0, (kw, ids, s)
    lens = [len(ids) for _, ids, _ in hyps]
    print("hypothesis lengths", sorted(set(lens)))
    assert min(lens) >= PROP["min_len"] and min(lens) < c["T"], lens  # some captions do end


def test_greedy_agreement(small_model):
    """sample top_k = 1, beam with one beam and the CPU constrained greedy decode agree."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    kw = dict(CONS["all"], banned_tokens=(0, 7))
    beam = pl.predict_batch(imgs, c["T"], beam_n=1, use_graph=False, mode="beam", **kw)
    samp = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=2, top_k=1, **kw)
    free = pl.predict_batch(imgs, c["T"], beam_n=1, use_graph=False, mode="beam")
    for i in range(c["n_img"]):
        cpu = cpu_greedy_constrained(m["sd"], m["cfg"], m["encs"][i], c["T"], pl.start_token, pl.end_token, _cons(kw))
        assert beam[i] == cpu, (i, beam[i], cpu)
        assert [ids for ids, _ in samp[i]] == [cpu, cpu], (i, samp[i], cpu)
    assert beam != free


def test_defaults_make_no_constrain_call(small_model, monkeypatch):
    """All four at their defaults: the same results as without the
    arguments, and no fpnmt_logits_constrain in the step; with one on, one
    call per position."""
    import fpnmt
    from fpnmt import decode as D
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    names = []
    real = D.call
    monkeypatch.setattr(D, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    a = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"])
    b = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"], **FULL)
    assert a == b
    sa = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=3, seed=5)
    sb = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=3, seed=5, **FULL)
    assert sa == sb
    assert "fpnmt_beam_step_log" in names and "fpnmt_sample_step" in names
    assert "fpnmt_logits_constrain" not in names
    del names[:]
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", min_len=c["T"] - 1)
    assert names.count("fpnmt_logits_constrain") == names.count("fpnmt_beam_step_log") == c["T"]
    i = names.index("fpnmt_logits_constrain")
    assert names[i + 1] == "fpnmt_beam_step_log"  # between the logits and the step kernel


def test_constrained_decode_graph_matches_eager_bf16():
    """Eager == captured graphs == a second replay with the constraints on,
    beam (K 4) and sample (6 samples), and the result differs from the
    unconstrained one."""
    import fpnmt
    fpnmt.set_precision("bf16")
    try:
        T, vocab, image, n_img = 12, 300, 224, 3
        pl = _pipeline(2, vocab, image, 17, T, end_bias=3.2)
        g = torch.Generator().manual_seed(6)
        imgs = (torch.rand(n_img, image, image, 3, generator=g) * 2 - 1).to(DEV)
        cons = dict(no_repeat_ngram=2, repetition_penalty=1.2, min_len=5, banned_tokens=(0, 7))
        for kw in (dict(beam_n=4, mode="beam", n_best=4), dict(mode="sample", n_samples=6, top_p=0.9, seed=31)):
            a = pl.predict_batch(imgs, T, use_graph=False, **kw, **cons)
            b = pl.predict_batch(imgs, T, use_graph=True, **kw, **cons)
            c = pl.predict_batch(imgs, T, use_graph=True, **kw, **cons)  # replay of the captured graphs
            assert a == b == c, kw
            free = pl.predict_batch(imgs, T, use_graph=True, **kw)
            assert free != a, kw
            for img in a:
                for ids, _ in img:
                    assert violates(ids, T, pl.start_token, cons) is None, (kw, ids)
    finally:
        fpnmt.set_precision("fp32")


def test_constraint_arguments_are_validated(small_model, monkeypatch):
    """Every ValueError of the decoders, through predict_batch and the constructors."""
    from fpnmt import _lib as L
    from fpnmt.decode import BeamDecoder, SampleDecoder
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    T, V, K = c["T"], c["vocab"], c["K"]
    tr, st, en = pl.transformer, pl.start_token, pl.end_token
    free = [j for j in range(V) if j != en]

    def beam(**kw):
        return [lambda: pl.predict_batch(imgs, T, beam_n=K, use_graph=False, mode="beam", **kw),
                lambda: BeamDecoder(tr, 3, K, T, st, en, use_graph=False, mode="beam", **kw)]

    def sample(**kw):
        return [lambda: pl.predict_batch(imgs, T, use_graph=False, mode="sample", n_samples=2, **kw),
                lambda: SampleDecoder(tr, 3, 2, T, st, en, use_graph=False, **kw)]

    def reference(**kw):
        return [lambda: pl.predict_batch(imgs, T, beam_n=K, use_graph=False, mode="reference", **kw),
                lambda: pl.predict_batch(imgs, T, beam_n=K, use_graph=False, **kw),
                lambda: BeamDecoder(tr, 3, K, T, st, en, use_graph=False, **kw)]

    cases = []
    for kw in (dict(no_repeat_ngram=-1), dict(no_repeat_ngram=1.5), dict(repetition_penalty=0.0),
               dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty=float("nan")), dict(min_len=-1), dict(min_len=T), dict(banned_tokens=(V,)),
               dict(banned_tokens=(-1,)), dict(banned_tokens=(en,))):
        cases += beam(**kw) + sample(**kw)
    # one id more than leaves beam_n (beam) / 1 (sample) tokens a row can always choose from
    cases += beam(banned_tokens=free[:V - T - 1 - K + 1]) + sample(banned_tokens=free[:V - T - 1])
    for kw in (dict(min_len=2), dict(no_repeat_ngram=2), dict(repetition_penalty=1.2), dict(banned_tokens=(0,))):
        cases += reference(**kw)  # that mode is the reference's own procedure
    for n, f in enumerate(cases):
        with pytest.raises(ValueError):
            f()
            print("case", n, "did not raise")
    # the largest admissible lists are accepted
    BeamDecoder(tr, 3, K, T, st, en, use_graph=False, mode="beam", banned_tokens=free[:V - T - 1 - K])
    SampleDecoder(tr, 3, 2, T, st, en, use_graph=False, banned_tokens=free[:V - T - 2])
    # the kernel's fixed sizes: the staged history and the list
    monkeypatch.setattr(L, "CONSTRAIN_MAX_LEN", T - 1)
    for f in beam(min_len=2) + sample(min_len=2):
        with pytest.raises(ValueError, match="positions"):
            f()
    BeamDecoder(tr, 3, K, T, st, en, use_graph=False, mode="beam")  # unconstrained: no limit
    monkeypatch.setattr(L, "CONSTRAIN_MAX_LEN", 1024)
    monkeypatch.setattr(L, "CONSTRAIN_MAX_BANNED", 2)
    for f in beam(banned_tokens=(0, 4, 5)) + sample(banned_tokens=(0, 4, 5)):
        with pytest.raises(ValueError, match="banned tokens"):
            f()

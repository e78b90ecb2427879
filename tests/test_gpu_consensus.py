"""Consensus (minimum-Bayes-risk) caption selection on the device:
fpnmt_ciderd_consensus against utils.cider_reward.CiderDReward.pairwise /
consensus (fp64, host) on rows laid out as the sampler leaves them, its exact
zeros, picks, determinism and independence, error codes and capture; and the
decoders' consensus= / Pipeline.predict_batch end to end on a small model.

Bound of a pair. pair[s][j] is the reward of tests/test_gpu_cider_reward.py
with c_j as the ONLY reference, and the derivation there carries over term by
term (the idf and the Gaussian factor are the host's values bit for bit, no
transcendental function is evaluated, so only the order of the sums, FMA
contraction and the implementation of division and square root differ). With
u = 2^-53 and L the longer of the two captions, every quantity non-negative:
  numerator of one order: at most L products min(w, r) * r: 2 L u between the
    two sides; the two norms: (2 L + 4) u; nh * nr, the division and the
    Gaussian factor: 6 u; the sum over R = 1 reference, the mean of the four
    orders, / R and * 10: (2 R + 12) u = 14 u; a faithfully instead of
    correctly rounded division and square root on the device: 4 u.
Together (4 L + 28) u, stated as that file states it (R / 2 = 0.5):
  |pair_dev - pair_host| <= 4 (L + 7.5) u pair_host.
Bound of a utility. util = num / den, num = sum_{j != s} p_j sim_j and
den = sum_{j != s} p_j, both over ascending j on both sides, m = n - 1 terms.
den: the same inputs added in the same order without a product: bitwise equal.
num: each term's sim within the pair bound of its pair, at most B = 4 (Lmax +
7.5) u relative with Lmax the image's longest candidate; the product p_j *
sim_j rounds once on the host and is contracted into the addition on the
device (one rounding fewer, never more): u; m - 1 additions a side: 2 (m - 1)
u; so num differs by at most (B + (2 m - 1) u) num_host. The division: u on
the host, 2 u (faithful) on the device: 3 u. To first order B + (2 n + 1) u;
the second-order terms are below 2^-40 of that and covered by rounding up to
the count the kernel was specified with:
  |util_dev - util_host| <= (4 (Lmax + 7.5) + 2 n + 4) u util_host.
A host value of exactly 0 has a numerator of exact zeros on both sides: the
device gives exactly 0.0 as well (pairs and utilities).
Picks are compared where the host's top-two margin exceeds twice the bound of
the larger of the two utilities; below it either index is right.

"posterior" weights (the beam end-to-end test): the device's weights are
torch's fp64 softmax of the returned fp32 scores, the host's numpy's. The
normaliser cancels in num / den, which leaves per weight two exponentials
within 1 ulp each and the two divisions: delta = 4 u per weight between the
sides, 8 u in num / den; and den is no longer bitwise equal: 2 (n - 2) u for
its additions. The bound widens by (2 n + 4) u, to
  (4 (Lmax + 7.5) + 4 n + 8) u util_host.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53
START, END = 2, 3

# the five-image corpus and the candidate sets of tests/test_consensus_cpu.py
CORPUS = {
    "a": [[5, 6, 7, 8, 9, 6, 7], [5, 6, 7, 10, 11], [12, 6, 7, 8]],
    "b": [[5, 13, 14, 15, 16], [17, 13, 14, 15, 16, 18]],
    "c": [[5, 6, 19, 20, 21, 22, 23, 24], [5, 6, 19, 25, 21], [26, 27, 19, 20]],
    "d": [[30, 31, 32, 33], [30, 31, 34, 33, 35]],
    "e": [[5, 6, 7, 8, 40, 41], [42, 43, 44, 6, 7]],
}
SETS = {
    "consensus": [[5, 6, 7, 8, 9], [5, 6, 7, 8], [5, 6, 7, 10, 11], [12, 6, 7, 8, 9], [30, 31, 32, 33],
                  [5, 6, 7, 8, 9, 6, 7]],
    "dups": [[5, 13, 14, 15, 16], [5, 13, 14, 15, 16], [17, 13, 14, 15], [50, 51]],
    "short": [[5], [5, 6], [5, 6, 7], [], [5, 6, 7, 8]],
    "disjoint": [[50, 51], [52, 53, 54], [55]],
    "long_repeat": [[6, 7] * 6, [6, 7, 6, 7], [5, 6, 7, 8, 40, 41], [6, 7, 8]],
}
PICK = {"consensus": 0, "short": 2, "long_repeat": 3}


def pair_bound(len_s, len_j, host):
    return 4.0 * (max(len_s, len_j) + 7.5) * U * host


def util_bound(cands, host, posterior=False):
    n = len(cands)
    return (4.0 * (max(len(c) for c in cands) + 7.5) + 2 * n + 4 + (2 * n + 4 if posterior else 0)) * U * host


def sampler_rows(cands, T, ld):
    """hist / slen / fin as fpnmt_sample_step leaves them after T positions
    (tests/test_gpu_cider_reward.py): a caption shorter than T ended (<end>
    follows, then <end> padding, slen counts the <end>, fin 1); one of T
    tokens did not (fin 0); None is a row that was never stepped (slen = fin
    = 0). Columns the kernel must not read hold a token of the corpus."""
    R = len(cands)
    hist = np.full((R, ld), 6, dtype=np.int32)
    hist[:, 0] = START
    slen, fin = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    for r, c in enumerate(cands):
        if c is None:
            continue
        assert len(c) <= T
        hist[r, 1:1 + len(c)] = c
        if len(c) < T:
            hist[r, 1 + len(c):T + 1] = END
            slen[r], fin[r] = len(c) + 1, 1
        else:
            slen[r] = T
    return tuple(torch.from_numpy(a).to(DEV) for a in (hist, slen, fin))


def launch(dev, rows, n, weight=None, want_pair=True):
    """-> util (rows,), pick (images,), pair (images, n, n) or None; the
    outputs start poisoned."""
    hist, slen, fin = rows
    images = hist.shape[0] // n
    util = torch.full((images * n,), 7.0, dtype=torch.float64, device=DEV)
    pick = torch.full((images,), -5, dtype=torch.int32, device=DEV)
    pair = torch.full((images, n, n), 7.0, dtype=torch.float64, device=DEV) if want_pair else None
    if weight is not None and not torch.is_tensor(weight):
        weight = torch.tensor(np.asarray(weight, dtype=np.float64).reshape(-1), device=DEV)
    dev.consensus(hist, slen, fin, n, util, pick, weight=weight, pair=pair)
    return util, pick, pair


def check_image(name, cands, want_pair, want_util, want_pick, util, pick, pair, posterior=False):
    """One image's device outputs against the host's; -> (the largest error
    over its bound, whether the pick was compared)."""
    n = len(cands)
    worst = 0.0
    for s in range(n):
        for j in range(n):
            w, g = want_pair[s][j], float(pair[s][j])
            if w == 0.0:
                assert g == 0.0, (name, s, j, g)
                continue
            b = pair_bound(len(cands[s]), len(cands[j]), w)
            worst = max(worst, abs(g - w) / b)
            assert abs(g - w) <= b, (name, s, j, g, w, abs(g - w) / b)
    bounds = [util_bound(cands, w, posterior) for w in want_util]
    for s in range(n):
        w, g = want_util[s], float(util[s])
        if w == 0.0:
            assert g == 0.0, (name, s, g)
            continue
        worst = max(worst, abs(g - w) / bounds[s])
        assert abs(g - w) <= bounds[s], (name, s, g, w, abs(g - w) / bounds[s])
    assert 0 <= pick < n
    order = sorted(range(n), key=lambda s: (-want_util[s], s))
    compared = n == 1 or want_util[order[0]] - want_util[order[1]] > 2 * bounds[order[0]]
    if compared:
        assert pick == want_pick, (name, pick, want_pick)
    else:  # a near tie: any candidate within the bound of the host's best
        assert want_util[order[0]] - want_util[pick] <= 2 * bounds[order[0]], (name, pick, want_pick)
    return worst, compared


@functools.lru_cache(maxsize=None)
def five():
    from fpnmt.cider_device import DeviceCiderD
    return DeviceCiderD.from_corpus(CORPUS, DEV)


@functools.lru_cache(maxsize=None)
def dense():
    """The seeded random corpus of the table tests: 40 images, 1-6
    references, V = 12 (overlaps, repeats and clipping are dense)."""
    from fpnmt.cider_device import DeviceCiderD
    rng = np.random.default_rng(0)
    refs = [[rng.integers(0, 12, size=int(rng.integers(1, 13))).tolist() for _ in range(int(rng.integers(1, 7)))]
            for _ in range(40)]
    return DeviceCiderD.from_corpus(refs, DEV)


# ---------------------------------------------------- kernel against host (1)
@functools.lru_cache(maxsize=None)
def five_sets_case(masked):
    """The five sets padded to n = 6 with never-stepped rows, and the host's
    answers (computed once). Unweighted, a padding row is an empty candidate
    (it adds to the denominator); masked, the padding weighs 0 and the
    utilities are the unpadded sets' own."""
    host = five().host
    names = list(SETS)
    padded = [SETS[k] + [None] * (6 - len(SETS[k])) for k in names]
    weights = [[1.0] * len(SETS[k]) + [0.0] * (6 - len(SETS[k])) for k in names] if masked else None
    want = []
    for i, cs in enumerate(padded):
        cs = [c or [] for c in cs]
        util, pick = host.consensus(cs, weights[i] if masked else None)
        want.append((cs, host.pairwise(cs), util, pick))
    return names, padded, weights, want


@pytest.mark.parametrize("masked", [False, True], ids=["uniform", "masked"])
@pytest.mark.parametrize("ld", [13, 20])
def test_the_five_sets_in_one_launch(ld, masked):
    """T = 12: finished rows with <end> padding, the 12-token repeated bigram
    unfinished at full width, never-stepped rows, an empty caption, poison in
    the columns that must not be read."""
    names, padded, weights, want = five_sets_case(masked)
    rows = sampler_rows([c for cs in padded for c in cs], 12, ld)
    assert int(rows[2][24]) == 0 and int(rows[1][24]) == 12  # long_repeat's first row did not end
    util, pick, pair = launch(five(), rows, 6, weights)
    util, pick, pair = util.cpu().numpy().reshape(5, 6), pick.cpu().tolist(), pair.cpu().numpy()
    for i, name in enumerate(names):
        cs, want_pair, want_util, want_pick = want[i]
        worst, compared = check_image(name, cs, want_pair, want_util, want_pick, util[i], pick[i], pair[i])
        print(f"{name}: largest error / bound {worst:.3f}, pick {pick[i]} (host {want_pick}, compared {compared})")
        if name in PICK:  # the margins of these sets are far above the bound: a property of the inputs
            assert compared and pick[i] == PICK[name]
        if name == "dups":
            assert not compared and pick[i] in (0, 1)
            assert abs(util[i][0] - util[i][1]) <= util_bound(cs, want_util[0])
        if name == "disjoint":
            assert pick[i] == 0 and np.all(util[i] == 0.0)
            assert np.all(pair[i][~np.eye(6, dtype=bool)] == 0.0)
        if masked:  # the unpadded sets' utilities (tests/test_consensus_cpu.py pins them)
            plain, _ = five().host.consensus(SETS[name])
            assert np.all(want_util[:len(plain)] == plain)
    diag = pair[0].diagonal()
    assert np.all(np.abs(diag - 10.0) <= 1e-12)  # every caption of the consensus set has all four orders


# ---------------------------------------------------- kernel against host (2)
@functools.lru_cache(maxsize=None)
def random_case(n, T=12, images=7, seed=17):
    """images x n candidates over V = 12 of lengths 0 .. T, non-negative
    weights of which three in ten are zero (image 1: all weight on one
    candidate), and the host's answers (computed once). The seed was checked
    on the host alone: the host's own margins let 33 of the 35 picks of
    test_random_weighted_cases be compared."""
    host = dense().host
    rng = np.random.default_rng(seed + n + 1000 * T)
    cands = [[rng.integers(0, 12, size=int(L)).tolist() for L in rng.integers(0, T + 1, size=n)]
             for _ in range(images)]
    cands[0][0] = rng.integers(0, 12, size=T).tolist()  # a row that did not end
    weights = rng.random((images, n)) * (rng.random((images, n)) < 0.7)
    weights[1] = 0.0
    weights[1, n // 2] = 2.5
    want = []
    for i, cs in enumerate(cands):
        util, pick = host.consensus(cs, weights[i])
        want.append((cs, host.pairwise(cs), util, pick))
    return cands, weights, want


def test_random_weighted_cases():
    """7 images a launch at n = 1, 2, 3, 16, 64 (one, a few, a wave's share,
    every wave several candidates). Two candidates with a zero weight or no
    common n-gram tie at 0, so the small n compare fewer picks; over the 35
    images at least 80 % must be compared."""
    compared_all = 0
    for n in (1, 2, 3, 16, 64):
        cands, weights, want = random_case(n)
        rows = sampler_rows([c for cs in cands for c in cs], 12, 13)
        util, pick, pair = launch(dense(), rows, n, weights)
        util, pick, pair = util.cpu().numpy().reshape(7, n), pick.cpu().tolist(), pair.cpu().numpy()
        worst, compared = 0.0, 0
        for i, (cs, want_pair, want_util, want_pick) in enumerate(want):
            w, c = check_image((n, i), cs, want_pair, want_util, want_pick, util[i], pick[i], pair[i])
            worst, compared = max(worst, w), compared + c
        print(f"n = {n}: largest error / bound {worst:.3f}, {compared} of 7 picks compared")
        compared_all += compared
        if n > 1:
            assert util[1][n // 2] == 0.0  # image 1: the only weight is the candidate's own
    assert compared_all >= 0.8 * 35, compared_all


def test_sixty_four_candidates_of_32_tokens():
    """n = 64 at T = 32: 135 KB of LDS, the launch that raises the kernel's
    dynamic LDS bound."""
    cands, weights, want = random_case(64, T=32, images=2)
    rows = sampler_rows([c for cs in cands for c in cs], 32, 33)
    util, pick, pair = launch(dense(), rows, 64, weights)
    util, pick, pair = util.cpu().numpy().reshape(2, 64), pick.cpu().tolist(), pair.cpu().numpy()
    for i, (cs, want_pair, want_util, want_pick) in enumerate(want):
        worst, compared = check_image(i, cs, want_pair, want_util, want_pick, util[i], pick[i], pair[i])
        print(f"image {i}: largest error / bound {worst:.3f}, pick compared {compared}")
    assert check_image(0, *want[0], util[0], pick[0], pair[0])[1]


# ------------------------------------------------ determinism, independence
def test_bitwise_repeatable_and_independent_of_the_other_images():
    dev = dense()
    n = 16
    cands, weights, _ = random_case(n)
    flat = [c for cs in cands for c in cs]
    rows = sampler_rows(flat, 12, 13)
    a = launch(dev, rows, n, weights)
    b = launch(dev, rows, n, weights)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # image 3 alone, and the images in reverse order
    one = tuple(t[3 * n:4 * n].contiguous() for t in rows)
    c = launch(dev, one, n, weights[3])
    assert torch.equal(c[0], a[0][3 * n:4 * n]) and torch.equal(c[1], a[1][3:4]) and torch.equal(c[2], a[2][3:4])
    rev = sampler_rows([c for cs in cands[::-1] for c in cs], 12, 13)
    d = launch(dev, rev, n, weights[::-1].copy())
    assert torch.equal(d[0].view(7, n).flip(0), a[0].view(7, n)) and torch.equal(d[1].flip(0), a[1])
    assert torch.equal(d[2].flip(0), a[2])
    # no weights == all-ones weights, bit for bit; without pair the other outputs are unchanged
    e = launch(dev, rows, n, None)
    f = launch(dev, rows, n, np.ones((7, n)))
    assert all(torch.equal(x, y) for x, y in zip(e, f)) and not torch.equal(e[0], a[0])
    g = launch(dev, rows, n, weights, want_pair=False)
    assert g[2] is None and torch.equal(g[0], a[0]) and torch.equal(g[1], a[1])
    # a wider table with other poison: the same bits
    wide = sampler_rows(flat, 12, 21)
    wide[0][:, 13:] = 9
    h = launch(dev, wide, n, weights)
    assert all(torch.equal(x, y) for x, y in zip(h, a))


# ------------------------------------------------------------- error codes
def test_error_codes_and_no_launch():
    from fpnmt import _lib as L
    dev = five()
    hist, slen, fin = sampler_rows(SETS["consensus"] * 2, 12, 13)
    util = torch.full((12,), 7.0, dtype=torch.float64, device=DEV)
    pick = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    weight = torch.ones(12, dtype=torch.float64, device=DEV)
    big = torch.zeros((64, 66), dtype=torch.int32, device=DEV)
    s = L.stream_ptr()
    t = C.byref(dev.tables)

    def run(tab=t, images=2, n=6, h=hist, ld=13, sl=slen, f=fin, w=weight, u=util, p=pick, pr=None):
        return L.lib.fpnmt_ciderd_consensus(tab, images, n, L.ptr(h), ld, L.ptr(sl), L.ptr(f), L.ptr(w), L.ptr(u),
                                            L.ptr(p), L.ptr(pr), s)

    for kw in (dict(tab=None), dict(h=None), dict(sl=None), dict(f=None), dict(u=None), dict(p=None), dict(n=0),
               dict(n=-1), dict(images=-1), dict(ld=0)):
        assert run(**kw) == L.E_ARG, kw
        assert b"ciderd_consensus" in L.lib.fpnmt_last_error()
    assert run(n=L.CONSENSUS_MAX_CANDS + 1, images=0) == L.E_UNSUPPORTED
    assert b"at most 64" in L.lib.fpnmt_last_error()
    assert run(ld=dev.max_len + 2) == L.E_UNSUPPORTED  # hist_ld - 1 > max_len
    assert b"max_len" in L.lib.fpnmt_last_error()
    assert dev.max_len == 64
    assert run(images=1, n=64, h=big, ld=40) == L.E_UNSUPPORTED  # 64 candidates of 39 tokens: above 160 KB
    assert b"LDS" in L.lib.fpnmt_last_error()
    assert run(images=0) == 0 and run(images=0, n=64, ld=39) == 0
    torch.cuda.synchronize()
    assert util.cpu().tolist() == [7.0] * 12 and pick.cpu().tolist() == [-5, -5]  # nothing was launched
    assert run() == 0 and run(w=None) == 0
    torch.cuda.synchronize()
    assert pick.cpu().tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="at most 64"):
        dev.consensus(big, slen, fin, 65, util, pick)


# ----------------------------------------------------------------- capture
def test_the_launch_replays_in_a_graph():
    dev = dense()
    n = 16
    cands, weights, _ = random_case(n)
    flat = [c for cs in cands for c in cs]
    first, second = sampler_rows(flat, 12, 13), sampler_rows(flat[::-1], 12, 13)
    w = torch.tensor(weights.reshape(-1), device=DEV)
    want1, want2 = launch(dev, first, n, w), launch(dev, second, n, w)
    static = tuple(t.clone() for t in first)
    util = torch.zeros(7 * n, dtype=torch.float64, device=DEV)
    pick = torch.zeros(7, dtype=torch.int32, device=DEV)
    pair = torch.zeros((7, n, n), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.consensus(static[0], static[1], static[2], n, util, pick, weight=w, pair=pair)
    for rows, want in ((first, want1), (second, want2), (first, want1)):
        for dst, src in zip(static, rows):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, x in zip((util, pick, pair), want):
            assert torch.equal(got, x)
    assert not torch.equal(want1[0], want2[0])


# -------------------------------------------------------------- end to end
CFG = dict(n_layers=2, vocab=200, image=256, T=10, n_img=3, K=8, model_seed=13, image_seed=4, end_bias=3.0)


def _pipeline(n_layers, vocab, image, seed, T, end_bias):
    """tests/test_gpu_sample_decode.py's model: end_bias is added to <end>'s
    logit, random weights would otherwise never end a caption."""
    from fpnmt.layers import Init, invalidate_weights
    from utils.pipeline import Pipeline
    pl = Pipeline(max_seq_len=T, target_vocab_size=vocab, image_size=image, n_layers=n_layers, rate=0.0,
                  init=Init(torch.Generator().manual_seed(seed)), use_graph=False)
    with torch.no_grad():
        pl.transformer.final_layer.bias[pl.end_token] += end_bias
    invalidate_weights()
    return pl


@pytest.fixture(scope="module")
def small_model():
    import fpnmt
    from fpnmt.cider_device import DeviceCiderD
    c = CFG
    fpnmt.set_precision("fp32")
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])
    imgs = torch.rand(c["n_img"], c["image"], c["image"], 3,
                      generator=torch.Generator().manual_seed(c["image_seed"])) * 2 - 1
    rng = np.random.default_rng(5)
    # a small synthetic corpus over the vocabulary: 30 images, 3 references of 4 .. 10 tokens
    corpus = [[rng.integers(4, c["vocab"], size=int(rng.integers(4, 11))).tolist() for _ in range(3)]
              for _ in range(30)]
    tables = DeviceCiderD.from_corpus(corpus, DEV, max_len=16)
    return dict(pl=pl, imgs=imgs.to(DEV), tables=tables)


def undo_sort(plain, ranked):
    """ranked: (ids, score, utility) by utility descending, then index ->
    the index in `plain` ((ids, score) in candidate order) of every entry:
    the lowest unused one that holds the entry's ids and score."""
    used, index = set(), []
    for ids, score, _ in ranked:
        r = next(r for r, (i, s) in enumerate(plain) if r not in used and i == ids and s == score)
        used.add(r)
        index.append(r)
    assert sorted(index) == list(range(len(plain)))
    utils = [u for _, _, u in ranked]
    for a in range(len(ranked) - 1):
        assert utils[a] > utils[a + 1] or (utils[a] == utils[a + 1] and index[a] < index[a + 1]), (a, utils, index)
    return index


def check_end_to_end(plain, ranked, chosen, tables, weights_of=None):
    worst = 0.0
    for i, (pl_i, rk_i) in enumerate(zip(plain, ranked)):
        index = undo_sort(pl_i, rk_i)
        cands = [ids for ids, _ in pl_i]
        w = None if weights_of is None else weights_of([s for _, s in pl_i])
        want, _ = tables.host.consensus(cands, w)
        for (ids, score, util), r in zip(rk_i, index):
            assert isinstance(util, float) and isinstance(ids, list)
            if want[r] == 0.0:
                assert util == 0.0, (i, r)
                continue
            b = util_bound(cands, want[r], posterior=weights_of is not None)
            worst = max(worst, abs(util - want[r]) / b)
            assert abs(util - want[r]) <= b, (i, r, util, want[r], abs(util - want[r]) / b)
        assert chosen[i] == rk_i[0][0]
    return worst


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_sample_mode_consensus_end_to_end(small_model, use_graph):
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, CFG
    kw = dict(use_graph=use_graph, mode="sample", n_samples=c["K"], seed=3)
    plain = m["pl"].predict_batch(m["imgs"], c["T"], **kw)
    ranked = m["pl"].predict_batch(m["imgs"], c["T"], consensus=m["tables"], consensus_all=True, **kw)
    chosen = m["pl"].predict_batch(m["imgs"], c["T"], consensus=m["tables"], **kw)
    assert m["pl"].predict_batch(m["imgs"], c["T"], **kw) == plain  # a call without consensus returns what it did
    worst = check_end_to_end(plain, ranked, chosen, m["tables"])
    print(f"sample, use_graph={use_graph}: largest utility error / bound {worst:.3f}; "
          f"utilities {[round(u, 3) for _, _, u in ranked[0]]}")
    assert any(u > 0.0 for img in ranked for _, _, u in img)
    if use_graph:
        eager = m["pl"].predict_batch(m["imgs"], c["T"], consensus=m["tables"], consensus_all=True,
                                      **dict(kw, use_graph=False))
        assert eager == ranked


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_beam_mode_posterior_consensus_end_to_end(small_model, use_graph):
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, CFG
    kw = dict(use_graph=use_graph, mode="beam", beam_n=c["K"], length_alpha=0.7)
    nbest = m["pl"].predict_batch(m["imgs"], c["T"], n_best=c["K"], **kw)
    cons = dict(consensus=m["tables"], consensus_weights="posterior")
    ranked = m["pl"].predict_batch(m["imgs"], c["T"], consensus_all=True, **cons, **kw)
    chosen = m["pl"].predict_batch(m["imgs"], c["T"], **cons, **kw)
    for nb, rk in zip(nbest, ranked):  # the same beams with the same scores
        assert sorted((tuple(i), s) for i, s in nb) == sorted((tuple(i), s) for i, s, _ in rk)

    def softmax64(scores):
        x = np.array(scores, dtype=np.float64)
        e = np.exp(x - x.max())
        return e / e.sum()

    # the host takes the candidates in the n-best order (the beams' row order is not returned)
    worst = check_end_to_end_unordered(nbest, ranked, chosen, m["tables"], softmax64)
    print(f"beam, use_graph={use_graph}: largest utility error / bound {worst:.3f}; "
          f"utilities {[round(u, 3) for _, _, u in ranked[0]]}")
    uniform = m["pl"].predict_batch(m["imgs"], c["T"], consensus=m["tables"], consensus_all=True, **kw)
    assert uniform != ranked  # the weights matter
    if use_graph:
        eager = m["pl"].predict_batch(m["imgs"], c["T"], consensus_all=True, **cons, **dict(kw, use_graph=False))
        assert eager == ranked


def check_end_to_end_unordered(plain, ranked, chosen, tables, weights_of):
    """Beam mode: a utility does not depend on the order of the OTHER
    candidates beyond the order of its sums, which the bound covers, so the
    host may take the candidates in any order."""
    worst = 0.0
    for i, (pl_i, rk_i) in enumerate(zip(plain, ranked)):
        cands = [ids for ids, _ in pl_i]
        want, _ = tables.host.consensus(cands, weights_of([s for _, s in pl_i]))
        used = set()
        utils = [u for _, _, u in rk_i]
        assert all(a >= b for a, b in zip(utils, utils[1:]))
        for ids, score, util in rk_i:
            r = next(r for r, (x, s) in enumerate(pl_i) if r not in used and x == ids and s == score)
            used.add(r)
            if want[r] == 0.0:
                assert util == 0.0, (i, r)
                continue
            b = util_bound(cands, want[r], posterior=True)
            worst = max(worst, abs(util - want[r]) / b)
            assert abs(util - want[r]) <= b, (i, r, util, want[r], abs(util - want[r]) / b)
        assert chosen[i] == rk_i[0][0]
    return worst


def test_consensus_captions_and_the_refusals(small_model):
    m, c = small_model, CFG
    pl, tables = m["pl"], m["tables"]
    sets = [SETS["consensus"], SETS["long_repeat"] + [[], [5]]]
    five_t = five()
    pick, util = pl.consensus_captions(sets, five_t)
    for i, cs in enumerate(sets):
        want, want_pick = five_t.host.consensus(cs)
        assert pick[i] == want_pick
        assert all(abs(g - w) <= util_bound(cs, w) for g, w in zip(util[i], want))
    pick_w, _ = pl.consensus_captions(sets[:1], five_t, weights=[[0.5, 0.1, 0.1, 0.1, 0.1, 0.1]])
    assert pick == [0, 3] and pick_w == [3]
    with pytest.raises(ValueError):
        pl.consensus_captions([SETS["dups"], SETS["short"]], five_t)  # 4 and 5 candidates
    for kw in (dict(mode="reference", consensus=tables), dict(mode="beam", consensus=tables, n_best=2),
               dict(mode="beam", consensus=tables, beam_groups=2, group_best=True),
               dict(mode="sample", n_samples=4, consensus_all=True),
               dict(mode="sample", n_samples=4, consensus_weights="posterior"),
               dict(mode="sample", n_samples=4, consensus=tables, consensus_weights="other"),
               dict(mode="sample", n_samples=65, consensus=tables)):
        with pytest.raises(ValueError):
            pl.predict_batch(m["imgs"], c["T"], **kw)
    with pytest.raises(ValueError, match="max_len"):
        pl.predict_batch(m["imgs"], 17, mode="sample", n_samples=4, consensus=tables)  # T above the tables' max_len

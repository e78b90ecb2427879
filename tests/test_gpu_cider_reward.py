"""The device-side CIDEr-D reward: fpnmt_ciderd_reward against
utils.cider_reward.CiderDReward.score (fp64, host) on rows laid out as the
sampler leaves them, its exact zeros, determinism, defined edge behaviour,
error codes and capture; and fpnmt_scst_pack against fpnmt.scst.pack_tokens /
advantages.

Bound of the reward. The tables (tf * idf, idf, the Gaussian factor) are the
host's values bit for bit (tests/test_cider_tables_cpu.py), and the kernel
evaluates no transcendental function, so only the order of the sums, FMA
contraction (the device code is built with the compiler's default
-ffp-contract=fast: a fused multiply-add has ONE rounding where the host has
two, never more) and the implementation of division and square root differ.
With u = 2^-53, L the larger of the candidate's length and the image's
longest reference length, R the image's number of references, every quantity
non-negative:
  numerator of one order: at most L products min(w, r) * r (at most one
    rounding each) summed in some order: relative error <= L u on either
    side, 2 L u between the two;
  each of the two norms: the square root of such a sum: (L / 2 + 1) u on
    either side, (2 L + 4) u for both norms between the two sides;
  nh * nr, the division: 2 u a side; the Gaussian factor: 1 u a side: 6 u;
  the sum over the references, the mean of the four orders (3 additions, one
    division), / R and * 10: (R + 6) u a side, (2 R + 12) u;
  the device's fp64 division and square root taken as faithfully rounded
    (2 u) instead of correctly rounded (u), two of them: 4 u more.
Together (4 L + 2 R + 26) u to first order; the second-order terms are below
2^-40 of that and covered by rounding the constant up:
  |dev - host| <= 4 (L + R / 2 + 7) u host.
A host score of exactly 0 has a numerator of exact zeros on both sides: the
device gives exactly 0.0 as well.

fpnmt_scst_pack. Token rows: bitwise pack_tokens'. Advantages: within one
fp32 ulp of the larger of |reward| and |baseline| of the host's
advantages(...).astype(float32) on the DEVICE rewards read back (the fp64
leave-one-out sum is ordered differently from numpy's (sum - r) before the
single rounding to fp32). The three means over N = B n rows: two ordered fp64
sums of N terms, (N - 1) u sum|x| each, one division each, and for the
baseline the (n + 1) u by which the two forms of a leave-one-out mean differ:
  |dev - host| <= (2 N + 2 n + 4) u mean|x|.
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

CORPUS = {
    "a": [[5, 6, 7, 8, 9, 6, 7], [5, 6, 7, 10, 11], [12, 6, 7, 8]],
    "b": [[5, 13, 14, 15, 16], [17, 13, 14, 15, 16, 18]],
    "c": [[5, 6, 19, 20, 21, 22, 23, 24], [5, 6, 19, 25, 21], [26, 27, 19, 20]],
    "d": [[30, 31, 32, 33], [30, 31, 34, 33, 35]],
    "e": [[5, 6, 7, 8, 40, 41], [42, 43, 44, 6, 7]],
}
CANDS = {
    "a": [5, 6, 7, 8, 9],
    "b": [5, 13, 14, 14, 14, 16, 99],
    "c": [26, 27, 19, 20],              # one reference verbatim
    "d": [50, 51],                      # nothing in common: exactly 0
    "e": [6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7],  # one repeated bigram, much longer than the references (clipping)
}


def bound(cand_len, ref_lens, host):
    L = max([cand_len] + list(ref_lens))
    return 4.0 * (L + len(ref_lens) / 2.0 + 7.0) * U * host


def sampler_rows(cands, T, ld):
    """hist / slen / fin as fpnmt_sample_step leaves them after T positions:
    a caption shorter than T ended (<end> follows, then <end> padding, slen
    counts the <end>, fin 1); one of T tokens did not (fin 0); None is a row
    that was never stepped (slen = fin = 0). Columns the kernels must not
    read hold a token of the corpus."""
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


def launch(dev, rows, idx, n):
    hist, slen, fin = rows
    out = torch.full((hist.shape[0],), 7.0, dtype=torch.float64, device=DEV)
    dev.reward(hist, slen, fin, idx, n, out)
    return out


def _idx(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def five():
    from fpnmt.cider_device import DeviceCiderD
    return DeviceCiderD.from_corpus(CORPUS, DEV)


@functools.lru_cache(maxsize=None)
def dense():
    """The seeded random corpus of the table tests (40 images, 1-6
    references, V = 12: overlaps, repeats and clipping are dense) plus an
    image with 7 references and one with a single reference."""
    from fpnmt.cider_device import DeviceCiderD
    rng = np.random.default_rng(0)
    refs = [[rng.integers(0, 12, size=int(rng.integers(1, 13))).tolist() for _ in range(int(rng.integers(1, 7)))]
            for _ in range(40)]
    refs.append([rng.integers(0, 12, size=int(rng.integers(3, 13))).tolist() for _ in range(7)])
    refs.append([rng.integers(0, 12, size=9).tolist()])
    return DeviceCiderD.from_corpus(refs, DEV), refs


@functools.lru_cache(maxsize=None)
def dense_case(n):
    """Image slots (a permutation of table rows with repeats, the 7- and the
    1-reference image among them), n candidates each of lengths 0 .. 31, and
    the host's scores (computed once)."""
    dev, refs = dense()
    rng = np.random.default_rng(100 + n)
    slots = rng.permutation(42)[:10].tolist() + [40, 41, 40]
    slots += slots[:2]
    cands = [[rng.integers(0, 12, size=int(L)).tolist() for L in rng.integers(0, 32, size=n)] for _ in slots]
    cands[0][0] = list(refs[slots[0]][0])  # a reference verbatim
    want = dev.host.score(slots, cands)
    return slots, cands, want


def check(got, want, slots, cands, refs_of):
    got = got.cpu().numpy()
    worst, at = 0.0, 0
    for s, cs in zip(slots, cands):
        for c in cs:
            g, w = got[at], want[at]
            at += 1
            if w == 0.0:
                assert g == 0.0, (s, c, g)
                continue
            b = bound(len(c or []), [len(r) for r in refs_of[s]], w)
            worst = max(worst, abs(g - w) / b)
            assert abs(g - w) <= b, (s, c, g, w, abs(g - w) / b)
    assert at == len(got)
    return worst


# ------------------------------------------------------------------ reward
@pytest.mark.parametrize("ld", [13, 20])
def test_reward_on_the_five_image_corpus(ld):
    """n = 3 at T = 12: fin = 1 with <end> padding, fin = 0 at full width
    (the 12-token repeated bigram), slen = 0, length 1, a verbatim reference,
    nothing in common."""
    dev, T = five(), 12
    keys = list(CORPUS)
    cands = [[CANDS["a"], None, [5]], [CANDS["b"], [13], []], [CANDS["c"], CANDS["a"], CORPUS["c"][0]],
             [CANDS["d"], [30, 31, 32, 33], [99]], [CANDS["e"], [6, 7], CANDS["a"]]]
    host_cands = [[c or [] for c in cs] for cs in cands]
    want = dev.host.score(keys, host_cands)
    got = launch(dev, sampler_rows([c for cs in cands for c in cs], T, ld), _idx(range(5)), 3)
    worst = check(got, want, keys, cands, CORPUS)
    print(f"largest |dev - host| / bound: {worst:.3f}")
    g = got.cpu().numpy()
    assert g[1] == 0.0 and g[5] == 0.0 and g[9] == 0.0 and g[11] == 0.0  # slen 0, empty, no overlap (twice)
    assert g[6] > g[0] > 0 and g[12] > 0 and g[10] > g[9]


@pytest.mark.parametrize("n,ld", [(1, 32), (3, 40), (5, 32)])
def test_reward_on_the_dense_corpus(n, ld):
    dev, refs = dense()
    slots, cands, want = dense_case(n)
    got = launch(dev, sampler_rows([c for cs in cands for c in cs], 31, ld), _idx(slots), n)
    worst = check(got, want, slots, cands, refs)
    print(f"n = {n}, hist_ld = {ld}: largest |dev - host| / bound: {worst:.3f}; "
          f"{int((want == 0).sum())} exact zeros of {len(want)}")
    assert (want > 0).sum() > len(want) // 2


def test_a_one_image_corpus_scores_exactly_zero():
    from fpnmt.cider_device import DeviceCiderD
    dev = DeviceCiderD.from_corpus([[[5, 6, 7, 8], [5, 6, 9]]], DEV)
    cands = [[5, 6, 7, 8], [5], [], None, [9, 9, 9, 9, 9, 9]]
    got = launch(dev, sampler_rows(cands, 6, 7), _idx([0]), 5)
    assert got.cpu().tolist() == [0.0] * 5


def test_reward_is_bitwise_repeatable_and_independent_of_the_other_rows():
    dev, _ = dense()
    slots, cands, _ = dense_case(1)
    flat = [cs[0] for cs in cands]
    a = launch(dev, sampler_rows(flat, 31, 32), _idx(slots), 1)
    b = launch(dev, sampler_rows(flat, 31, 32), _idx(slots), 1)
    assert torch.equal(a, b)
    rev = launch(dev, sampler_rows(flat[::-1], 31, 32), _idx(slots[::-1]), 1)
    assert torch.equal(rev.flip(0), a)
    # the same rows as n = 3 groups of one image each
    c = launch(dev, sampler_rows([flat[0]] * 3 + [flat[1]] * 3, 31, 32), _idx(slots[:2]), 3)
    assert torch.equal(c, a[:2].repeat_interleave(3))


def test_an_image_index_out_of_range_scores_zero():
    dev, _ = dense()
    slots, cands, _ = dense_case(3)
    rows = sampler_rows([c for cs in cands for c in cs], 31, 32)
    good = launch(dev, rows, _idx(slots), 3)
    bad_slots = list(slots)
    bad_slots[1], bad_slots[4], bad_slots[7] = 42, -1, 2 ** 31 - 1
    got = launch(dev, rows, _idx(bad_slots), 3)
    want = good.clone().view(-1, 3)
    want[[1, 4, 7]] = 0.0
    assert float(good.view(-1, 3)[[1, 4, 7]].sum()) > 0
    assert torch.equal(got, want.view(-1))


# -------------------------------------------------------------------- pack
def pack(rows, reward, score, b, n, mode, greedy, T, width):
    from fpnmt import _lib as L
    hist, slen, fin = rows
    tok = torch.full((b * n, width), -5, dtype=torch.int64, device=DEV)
    adv = torch.full((b * n,), 7.0, dtype=torch.float32, device=DEV)
    sc = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    L.call("fpnmt_scst_pack", b, n, mode, L.ptr(reward), L.ptr(greedy), L.ptr(hist), hist.stride(0), L.ptr(slen),
           L.ptr(fin), L.ptr(score), START, END, T, L.ptr(tok), width, L.ptr(adv), L.ptr(sc), L.stream_ptr())
    return tok, adv, sc


@pytest.mark.parametrize("width", [13, 7])
def test_pack_token_rows_equal_pack_tokens(width):
    """Rows that ended, rows that did not (T tokens), empty rows (ended at
    once, and never stepped), and a table narrower than the rows."""
    from fpnmt.scst import pack_tokens
    T = 12
    cands = [CANDS["a"], [], CANDS["e"], None, [5], list(range(20, 31)), CANDS["b"], [4] * 12]
    rows = sampler_rows(cands, T, 16)
    reward = torch.zeros(8, dtype=torch.float64, device=DEV)
    score = torch.zeros(8, dtype=torch.float32, device=DEV)
    tok, adv, _ = pack(rows, reward, score, 4, 2, 0, None, T, width)
    want = pack_tokens([c or [] for c in cands], width, START, END, T)
    assert tok.dtype == torch.int64 and np.array_equal(tok.cpu().numpy(), want)
    assert adv.cpu().tolist() == [0.0] * 8  # all rewards equal: exactly 0


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_pack_advantages_and_means(n, baseline):
    from fpnmt.scst import advantages
    dev, _ = dense()
    slots, cands, _ = dense_case(5)
    b = len(slots)
    cands = [cs[:n] for cs in cands]
    cands[2] = [cands[2][0]] * n  # all-equal rewards: advantage exactly 0 under the mean baseline
    rows = sampler_rows([c for cs in cands for c in cs], 31, 32)
    reward = launch(dev, rows, _idx(slots), n)
    g = torch.Generator().manual_seed(n)
    score = -torch.rand(b * n, generator=g) * 20
    greedy = (torch.rand(b, generator=g, dtype=torch.float64) * 3)
    mode = 1 if baseline == "greedy" else 0
    _, adv, sc = pack(rows, reward, score.to(DEV), b, n, mode, greedy.to(DEV) if mode else None, 31, 32)
    r = reward.cpu().numpy().reshape(b, n)
    want, base = advantages(r, baseline, greedy.numpy() if mode else None)
    got = adv.cpu().numpy().reshape(b, n)
    tol = np.spacing(np.maximum(np.abs(r), np.abs(base)).astype(np.float32))
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - want.astype(np.float32)) <= tol)
    if mode == 0:
        assert got[2].tolist() == [0.0] * n
    N = b * n
    sc = sc.cpu().numpy()
    for name, got_s, x in (("reward", sc[0], r), ("baseline", sc[1], base), ("logp", sc[2], score.double().numpy())):
        tol_s = (2 * N + 2 * n + 4) * U * float(np.abs(x).mean())
        print(f"{name} mean {got_s!r} vs {float(x.mean())!r}, |d| / bound {abs(got_s - x.mean()) / tol_s:.3f}")
        assert abs(got_s - float(x.mean())) <= tol_s, name


# ------------------------------------------------------------- error codes
def test_error_codes():
    from fpnmt import _lib as L
    dev = five()
    hist, slen, fin = sampler_rows([CANDS["a"]] * 6, 12, 13)
    idx = _idx([0, 1])
    out = torch.zeros(6, dtype=torch.float64, device=DEV)
    s = L.stream_ptr()
    t = C.byref(dev.tables)

    def reward(tab=t, rows=6, n=3, h=hist, ld=13, sl=slen, f=fin, ix=idx, o=out):
        return L.lib.fpnmt_ciderd_reward(tab, rows, n, L.ptr(h), ld, L.ptr(sl), L.ptr(f), L.ptr(ix), L.ptr(o), s)

    assert reward() == 0
    for kw in (dict(tab=None), dict(h=None), dict(sl=None), dict(f=None), dict(ix=None), dict(o=None),
               dict(n=0), dict(n=-1), dict(n=4), dict(rows=5, n=2)):
        assert reward(**kw) == L.E_ARG, kw
    assert reward(ld=dev.max_len + 2) == L.E_UNSUPPORTED  # hist_ld - 1 > max_len: refused at the call, no launch
    assert b"max_len" in L.lib.fpnmt_last_error()
    adv = torch.zeros(6, device=DEV)
    tok = torch.zeros((6, 13), dtype=torch.int64, device=DEV)
    sc = torch.zeros(3, dtype=torch.float64, device=DEV)
    score = torch.zeros(6, device=DEV)

    def do_pack(b=2, n=3, mode=0, r=out, g=None, h=hist, tk=tok, a=adv, q=sc):
        return L.lib.fpnmt_scst_pack(b, n, mode, L.ptr(r), L.ptr(g), L.ptr(h), 13, L.ptr(slen), L.ptr(fin),
                                     L.ptr(score), START, END, 12, L.ptr(tk), 13, L.ptr(a), L.ptr(q), s)

    assert do_pack() == 0
    for kw in (dict(r=None), dict(h=None), dict(tk=None), dict(a=None), dict(q=None), dict(n=0), dict(mode=2),
               dict(mode=1), dict(b=6, n=1)):  # greedy without greedy[b]; the mean baseline with n = 1
        assert do_pack(**kw) == L.E_ARG, kw
    torch.cuda.synchronize()


# ----------------------------------------------------------------- capture
def test_the_two_launches_replay_in_a_graph():
    dev, _ = dense()
    slots, cands, _ = dense_case(3)
    b, n, T = len(slots), 3, 31
    flat = [c for cs in cands for c in cs]
    first, second = sampler_rows(flat, T, 32), sampler_rows(flat[::-1], T, 32)
    score = -torch.arange(b * n, dtype=torch.float32, device=DEV)
    idx = _idx(slots)

    def eager(rows):
        r = launch(dev, rows, idx, n)
        return (r,) + pack(rows, r, score, b, n, 0, None, T, 32)

    want1, want2 = eager(first), eager(second)
    static = tuple(t.clone() for t in first)
    reward = torch.zeros(b * n, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.reward(static[0], static[1], static[2], idx, n, reward)
        out = pack(static, reward, score, b, n, 0, None, T, 32)
    for rows, want in ((first, want1), (second, want2), (first, want1)):
        for dst, src in zip(static, rows):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip((reward,) + out, want):
            assert torch.equal(got, w)
    assert not torch.equal(want1[0], want2[0])

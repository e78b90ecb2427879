"""The packed CIDEr-D reference tables of the device-side reward (no GPU):
fpnmt.cider_device.DeviceCiderD.from_corpus against what
utils.cider_reward.CiderDReward holds, and score_host — the numpy walk over
the PACKED tables, the kernel's rule — against CiderDReward.score.

Bound. The tables (tf * idf, idf, the Gaussian) are the host's values bit for
bit, so the two scores differ only in the order of their sums. With
u = 2^-53, L the larger of the candidate's length and the longest reference
length, R the image's number of references, every quantity non-negative:
  numerator of one order: at most L products min(w, r) * r (one rounding
    each) summed in some order: relative error <= L u on either side, 2 L u
    between the two;
  each of the two norms: the square root of such a sum: (L / 2 + 1) u on
    either side, (2 L + 4) u for both norms between the two sides;
  nh * nr, the division: 2 u a side; the Gaussian factor: 1 u a side: 6 u;
  the sum over the references, the mean of the four orders (3 additions, one
    division), / R and * 10: (R + 6) u a side, (2 R + 12) u.
A division or a square root that is faithfully instead of correctly rounded
(2 u instead of u; the device's, tests/test_gpu_cider_reward.py) adds at most
4 u. Together (4 L + 2 R + 26) u to first order; the second-order terms are
below 2^-40 of that and covered by rounding the constant up:
  |score_host - host| <= 4 (L + R / 2 + 7) u host.
A host score of exactly 0 (no common n-gram, an empty candidate, every idf 0)
has a numerator of exact zeros on both sides: 0 there, too.
"""
import numpy as np
import pytest

U = 2.0 ** -53

# the five-image corpus of tests/test_scst_cpu.py
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
    "c": [26, 27, 19, 20],
    "d": [50, 51],
    "e": [6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7],
}


def bound(cand_len, ref_lens, host):
    L = max([cand_len] + list(ref_lens))
    return 4.0 * (L + len(ref_lens) / 2.0 + 7.0) * U * host


def random_corpus(seed=0, images=40, vocab=12):
    rng = np.random.default_rng(seed)
    refs = [[rng.integers(0, vocab, size=int(rng.integers(1, 13))).tolist() for _ in range(int(rng.integers(1, 7)))]
            for _ in range(images)]
    cands = [[rng.integers(0, vocab, size=int(n)).tolist() for n in rng.integers(0, 32, size=3)]
             for _ in range(images)]
    cands[0][0], cands[1][0] = [], [3]  # lengths 0 and 1, whatever the draw
    return refs, cands


def _check_scores(dev, keys, refs_of, cands):
    got = dev.score_host(list(range(len(keys))), cands)
    want = dev.host.score(keys, cands)
    assert got.shape == want.shape and got.dtype == np.float64
    worst, at = 0.0, 0
    for i, k in enumerate(keys):
        for c in cands[i]:
            g, w = got[at], want[at]
            at += 1
            if w == 0.0:
                assert g == 0.0, (k, c, g)
                continue
            b = bound(len(c), [len(r) for r in refs_of[k]], w)
            worst = max(worst, abs(g - w) / b)
            assert abs(g - w) <= b, (k, c, g, w, b)
    return worst, want


def test_tables_hold_the_host_values_bit_for_bit():
    from fpnmt.cider_device import DeviceCiderD, unpack_key, key_order
    from utils.cider_reward import ngram_counts
    dev = DeviceCiderD.from_corpus(CORPUS)
    a, host = dev.np, dev.host
    assert dev.keys == list(CORPUS) and dev.n_images == 5
    dk = a["df_keys"]
    assert dk.dtype == np.uint64 and np.all(dk[1:] > dk[:-1])
    # unpacking returns the n-grams: exactly the host's document-frequency keys
    grams = [unpack_key(k) for k in dk]
    assert set(grams) == set(host._df) and len(grams) == len(host._df)
    assert [len(g) for g in grams] == key_order(dk).tolist()
    for g, idf in zip(grams, a["df_idf"]):
        assert idf == host._ref_len - np.log(max(1.0, host._df[g])), g
    assert dev.idf_absent == float(host._ref_len)
    assert a["img_off"].tolist() == [0, 3, 5, 8, 10, 12]
    j = 0
    for key, rs in CORPUS.items():
        for r, (vec, norm, length) in zip(rs, host._refs[key]):
            e0, e1 = int(a["ref_off"][j]), int(a["ref_off"][j + 1])
            rk = a["ref_keys"][e0:e1]
            assert np.all(rk[1:] > rk[:-1])
            want = {g: v for d in vec for g, v in d.items()}
            assert {unpack_key(k) for k in rk} == set(want)
            for k, w in zip(rk, a["ref_w"][e0:e1]):
                assert w == want[unpack_key(k)], (key, unpack_key(k))  # bitwise: == on float64
            np.testing.assert_allclose(a["ref_norm"][j], norm, rtol=(len(r) + 2) * U, atol=0)
            # the quirk: "length" is the sum of the bigram counts, len - 1
            assert int(a["ref_len"][j]) == length == sum(c for g, c in ngram_counts(r, 4).items() if len(g) == 2)
            assert int(a["ref_len"][j]) == len(r) - 1
            j += 1
    assert j == len(a["ref_len"]) == 12
    assert len(a["gauss"]) == dev.max_len + int(a["ref_len"].max()) + 1
    for d, g in enumerate(a["gauss"]):
        assert g == np.e ** (-(float(d) ** 2) / (2 * 6.0 ** 2)), d


def test_score_host_on_the_five_image_corpus():
    from fpnmt.cider_device import DeviceCiderD
    dev = DeviceCiderD.from_corpus(CORPUS)
    keys = list(CORPUS)
    cands = [[CANDS[k], [], CORPUS[k][0]] for k in keys]
    worst, want = _check_scores(dev, keys, CORPUS, cands)
    print(f"largest |score_host - host| / bound: {worst:.3f}")
    assert want[9] == 0.0 and want[6] > want[0] > 0  # nothing in common; a verbatim reference
    # a sequence of reference lists gets the keys 0, 1, ...
    dev2 = DeviceCiderD.from_corpus(list(CORPUS.values()))
    assert dev2.keys == [0, 1, 2, 3, 4]
    assert dev2.score_host([0], [[CANDS["a"]]])[0] == dev.score_host([0], [[CANDS["a"]]])[0]
    with pytest.raises(ValueError):
        dev.score_host([0, 1], [[CANDS["a"]]])


def test_score_host_on_a_dense_random_corpus():
    from fpnmt.cider_device import DeviceCiderD
    refs, cands = random_corpus()
    dev = DeviceCiderD.from_corpus(refs)
    worst, want = _check_scores(dev, list(range(len(refs))), dict(enumerate(refs)), cands)
    print(f"largest |score_host - host| / bound: {worst:.3f}; {int((want == 0).sum())} exact zeros of {len(want)}")
    assert (want > 0).sum() > 80 and want[0] == 0.0


def test_a_one_image_corpus_scores_zero():
    from fpnmt.cider_device import DeviceCiderD
    dev = DeviceCiderD.from_corpus([[[5, 6, 7], [5, 8]]])
    assert dev.idf_absent == 0.0 and not dev.np["df_idf"].any()
    assert dev.score_host([0], [[[5, 6, 7], [9], []]]).tolist() == [0.0, 0.0, 0.0]


def test_packing_limits_and_errors():
    from fpnmt.cider_device import DeviceCiderD, pack_keys, unpack_key
    top = 65533
    dev = DeviceCiderD.from_corpus([[[top, 0, top, top]], [[0, 1]]])
    k4 = pack_keys([top, 0, top, top], 4)
    assert k4.tolist() == [(top + 1) | (1 << 16) | ((top + 1) << 32) | ((top + 1) << 48)]
    assert unpack_key(k4[0]) == (top, 0, top, top) and k4[0] in dev.np["ref_keys"]
    assert unpack_key(pack_keys([0], 1)[0]) == (0,)  # token 0 is present, not "absent"
    got = dev.score_host([0], [[[top, 0, top, top]]])[0]
    assert abs(got - dev.host.score([0], [[[top, 0, top, top]]])[0]) <= bound(4, [4], got) and got > 0
    with pytest.raises(ValueError):
        DeviceCiderD.from_corpus([[[5, 65534]], [[1]]])
    with pytest.raises(ValueError):
        DeviceCiderD.from_corpus([[[5, -1]], [[1]]])
    with pytest.raises(ValueError):
        DeviceCiderD.from_corpus(CORPUS, n=3)
    with pytest.raises(ValueError):
        DeviceCiderD.from_corpus({"x": [[1, 2]], "y": []})
    with pytest.raises(ValueError):
        DeviceCiderD.from_corpus(CORPUS, max_len=129)
    dev = DeviceCiderD.from_corpus(CORPUS)
    assert dev.index_of(["c", "a", "c"]).tolist() == [2, 0, 2]
    assert str(dev.index_of(["e"]).dtype) == "torch.int32"
    with pytest.raises(ValueError):
        dev.index_of(["a", "zz"])

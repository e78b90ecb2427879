"""Consensus (minimum-Bayes-risk) caption selection under CIDEr-D, no GPU:
utils.cider_reward.CiderDReward.pairwise / consensus pinned to known answers,
fpnmt.cider_device.DeviceCiderD.consensus_host — the numpy walk over the
PACKED document table, the kernel's rule — against them, and the argument
validation of the decoders' consensus arguments (fpnmt.decode.
consensus_validated, what Pipeline.predict_batch calls before any device
work).

Bound of consensus_host against CiderDReward. The idf and the Gaussian table
are the host's values bit for bit (tests/test_cider_tables_cpu.py), so a pair
differs only in the order of its sums: tests/test_cider_tables_cpu.py's bound
with ONE reference, L the longer of the two captions, u = 2^-53:
  |pair_packed - pair_host| <= 4 (L + 7.5) u pair_host.
Both utilities then come from the same plain-Python sums over ascending j
(utils.cider_reward.consensus_of) of non-negative terms each within that
relative bound, so the utility is within it too, L the image's longest
candidate; the (2 n + 4) u of tests/test_gpu_consensus.py for sums in another
arithmetic is kept on top so that the two files state one bound.
"""
import numpy as np
import pytest

U = 2.0 ** -53

# the five-image corpus of tests/test_gpu_cider_reward.py
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
# computed with CiderDReward on the CPU
UTIL = {
    "consensus": [4.366748045731846, 3.209470084887868, 1.2054468407310146, 3.2335245937945585, 0.0,
                  3.1741410870028477],
    "dups": [4.758240613529228, 4.758240613529228, 2.8498145603917897, 0.0],
    "short": [0.4569935465660465, 1.3176891796014116, 2.1122198703462836, 0.0, 1.906426301241567],
    "disjoint": [0.0, 0.0, 0.0],
    "long_repeat": [0.4232238275703228, 2.0685004066802115, 1.8050758117926249, 2.364239248580698],
}
PICK = {"consensus": 0, "dups": 0, "short": 2, "disjoint": 0, "long_repeat": 3}
MARGIN = {"consensus": 1.13, "short": 0.21, "long_repeat": 0.30}  # the top two utilities, to two digits
WEIGHTS = [0.5, 0.1, 0.1, 0.1, 0.1, 0.1]
UTIL_WEIGHTED = [4.366748045731846, 4.451752225858656, 1.3202871183932576, 4.963272853271034, 0.0,
                 4.6550606249553255]


def pair_bound(len_s, len_j, host):
    return 4.0 * (max(len_s, len_j) + 7.5) * U * host


def util_bound(cands, host):
    return (4.0 * (max(len(c) for c in cands) + 7.5) + 2 * len(cands) + 4) * U * host


@pytest.fixture(scope="module")
def host():
    from utils.cider_reward import CiderDReward
    return CiderDReward.from_corpus(CORPUS)


@pytest.fixture(scope="module")
def packed():
    from fpnmt.cider_device import DeviceCiderD
    return DeviceCiderD.from_corpus(CORPUS, "cpu")


# ---------------------------------------------------------- known answers
def test_self_similarity_by_length(host):
    """A caption against itself: every order it has gives 1, the others 0."""
    for c, want in (([5, 6, 7, 8], 10.0), ([5, 6, 7, 8, 9, 6, 7], 10.0), ([6, 7] * 6, 10.0), ([5, 6, 7], 7.5),
                    ([50, 51], 5.0), ([5], 2.5), ([55], 2.5)):
        assert abs(host.pairwise([c])[0, 0] - want) <= 1e-12, c
    assert host.pairwise([[]])[0, 0] == 0.0


def test_similarity_is_not_symmetric(host):
    p = host.pairwise(SETS["long_repeat"])
    assert abs(p[0, 1] - 0.9658720808613306) <= 1e-12  # the long caption's counts are clipped by the short one's
    assert abs(p[1, 0] - 3.8537533888847126) <= 1e-12
    assert abs(p[0, 1] - 0.96587) <= 1e-5 and abs(p[1, 0] - 3.85375) <= 1e-5


def test_pairwise_is_score_one_against_a_single_reference(host):
    """[s][j] = score_one of c_s in a CiderDReward whose image holds c_j
    alone, with THIS corpus's document frequencies."""
    from utils.cider_reward import CiderDReward
    cs = SETS["consensus"]
    p = host.pairwise(cs)
    for j, r in enumerate(cs):
        single = CiderDReward(host._df, len(CORPUS), {0: [r]})
        for s, c in enumerate(cs):
            assert p[s, j] == single.score_one(0, c), (s, j)


@pytest.mark.parametrize("name", list(SETS))
def test_uniform_consensus_known_answers(host, name):
    util, pick = host.consensus(SETS[name])
    assert util.dtype == np.float64 and util.shape == (len(SETS[name]),)
    assert np.all(np.abs(util - np.array(UTIL[name])) <= 1e-12), util.tolist()
    assert pick == PICK[name]
    top = np.sort(util)[::-1]
    if name in MARGIN:
        assert abs((top[0] - top[1]) - MARGIN[name]) <= 0.005
    if name == "dups":
        assert util[0] == util[1]  # an exact tie: the lower index wins
    if name == "disjoint":
        p = host.pairwise(SETS[name])
        assert np.all(p[~np.eye(3, dtype=bool)] == 0.0) and np.all(util == 0.0)


def test_weights_move_the_pick(host):
    util, pick = host.consensus(SETS["consensus"], WEIGHTS)
    assert pick == 3 and host.consensus(SETS["consensus"])[1] == 0
    assert np.all(np.abs(util - np.array(UTIL_WEIGHTED)) <= 1e-12), util.tolist()


def test_edges_of_the_definition(host):
    util, pick = host.consensus([[5, 6, 7]])  # one candidate: nothing to agree with
    assert util.tolist() == [0.0] and pick == 0
    util, pick = host.consensus([[], []])
    assert util.tolist() == [0.0, 0.0] and pick == 0
    # self is excluded by index: the only weight on the candidate itself leaves it a zero denominator
    util, pick = host.consensus(SETS["consensus"], [0, 0, 1.0, 0, 0, 0])
    p = host.pairwise(SETS["consensus"])
    assert util[2] == 0.0 and all(util[s] == p[s, 2] for s in (0, 1, 3, 4, 5))
    with pytest.raises(ValueError):
        host.consensus(SETS["dups"], [1, 1, 1])
    with pytest.raises(ValueError):
        host.consensus(SETS["dups"], [1, -1, 1, 1])


# ------------------------------------------------ the packed tables' walk
@pytest.mark.parametrize("name", list(SETS))
def test_consensus_host_on_the_packed_tables(host, packed, name):
    cs = SETS[name]
    want_p = host.pairwise(cs)
    got_p = packed.pairwise_host(cs)
    for s in range(len(cs)):
        for j in range(len(cs)):
            if want_p[s, j] == 0.0:
                assert got_p[s, j] == 0.0, (s, j)
            else:
                assert abs(got_p[s, j] - want_p[s, j]) <= pair_bound(len(cs[s]), len(cs[j]), want_p[s, j]), (s, j)
    (util, pick), = packed.consensus_host([cs])
    assert np.all(np.abs(util - np.array(UTIL[name])) <= 1e-9)
    for s, w in enumerate(UTIL[name]):
        assert (util[s] == 0.0) if w == 0.0 else abs(util[s] - w) <= util_bound(cs, w) + 1e-15, s
    assert pick == PICK[name] or (name == "dups" and pick in (0, 1))


def test_consensus_host_weights_and_several_images(host, packed):
    names = ["consensus", "dups", "long_repeat"]
    ws = [WEIGHTS, [0.0, 2.0, 0.5, 1.0], None]
    with pytest.raises(ValueError):
        packed.consensus_host([SETS[n] for n in names], ws[:2])
    got = packed.consensus_host([SETS[n] for n in names], [w or [1.0] * len(SETS[n]) for n, w in zip(names, ws)])
    for n, w, (util, pick) in zip(names, ws, got):
        want_u, want_k = host.consensus(SETS[n], w)
        assert pick == want_k
        for s in range(len(util)):
            assert abs(util[s] - want_u[s]) <= util_bound(SETS[n], want_u[s]), (n, s)
    assert got[0][1] == 3


def test_consensus_host_on_a_dense_random_case(packed):
    """V = 12: overlaps, repeats and clipping are dense; lengths 0 .. 12."""
    from fpnmt.cider_device import DeviceCiderD
    rng = np.random.default_rng(0)
    refs = [[rng.integers(0, 12, size=int(rng.integers(1, 13))).tolist() for _ in range(int(rng.integers(1, 7)))]
            for _ in range(40)]
    dev = DeviceCiderD.from_corpus(refs, "cpu")
    nonzero = 0
    for n in (1, 2, 3, 16):
        cs = [rng.integers(0, 12, size=int(L)).tolist() for L in rng.integers(0, 13, size=n)]
        w = rng.random(n) * (rng.random(n) < 0.7)
        want_p = dev.host.pairwise(cs)
        got_p = dev.pairwise_host(cs)
        for s in range(n):
            for j in range(n):
                assert abs(got_p[s, j] - want_p[s, j]) <= pair_bound(len(cs[s]), len(cs[j]), want_p[s, j]), (s, j)
                assert got_p[s, j] == 0.0 or want_p[s, j] != 0.0
        want_u, _ = dev.host.consensus(cs, w)
        (util, _), = dev.consensus_host([cs], [w])
        assert np.all(np.abs(util - want_u) <= [util_bound(cs, x) for x in want_u])
        nonzero += int((want_p != 0).sum())
    assert nonzero > 100


def test_a_candidate_longer_than_max_len_is_refused():
    from fpnmt.cider_device import DeviceCiderD
    dev = DeviceCiderD.from_corpus(CORPUS, "cpu", max_len=6)
    with pytest.raises(ValueError, match="max_len"):
        dev.consensus_host([[[5, 6, 7, 8, 9, 6, 7]]])


# ------------------------------------------------------ argument validation
def test_lds_budget_formula():
    from fpnmt import _lib as L
    from fpnmt.cider_device import DeviceCiderD
    f = DeviceCiderD.consensus_lds_bytes
    assert f(64, 32) == 64 * 122 * 16 + 8 * 122 * 8 + 64 * 44  # the keys and weights, the waves' scratch, the rest
    assert f(64, 38) <= L.CONSENSUS_LDS_BYTES < f(64, 39)
    assert f(16, 128) <= L.CONSENSUS_LDS_BYTES < f(17, 128)
    assert f(3, 2) == 16 * 3 * 3 + 64 * 3 + 44 * 3 and f(5, 0) == 44 * 5


def stub_tables(max_len=64, device="cuda:0"):
    """Stands for DeviceCiderD tables on cuda:0 (no GPU here): only what
    consensus_check reads is filled in, and the check is the real one."""
    import torch
    from fpnmt.cider_device import DeviceCiderD
    t = DeviceCiderD.__new__(DeviceCiderD)
    t.max_len, t.device = max_len, torch.device(device)
    return t


def test_the_consensus_arguments_are_validated_before_any_device_work(packed):
    from fpnmt import _lib as L
    from fpnmt.decode import consensus_validated as ok
    t = stub_tables()
    assert ok("beam", None) is False and ok("sample", None) is False and ok("reference", None) is False
    assert ok("sample", t, "uniform", False, 8, 20, "cuda:0") is True
    assert ok("beam", t, "posterior", True, 16, 64, "cuda") is True
    assert ok("sample", t, n=L.CONSENSUS_MAX_CANDS, max_seq_len=38) is True
    bad = [
        dict(mode="reference", consensus=t),                      # the reference's own procedure has one candidate
        dict(mode="beam", consensus=t, n=8, n_best=2),
        dict(mode="beam", consensus=t, n=8, group_best=True),
        dict(mode="beam", consensus=None, consensus_weights="posterior"),
        dict(mode="sample", consensus=None, consensus_all=True),
        dict(mode="sample", consensus=t, consensus_weights="softmax"),
        dict(mode="sample", consensus=t, n=4, max_seq_len=20, device="cpu"),       # another device
        dict(mode="sample", consensus=t, n=4, max_seq_len=20, device="cuda:1"),
        dict(mode="sample", consensus=packed, n=4, max_seq_len=20, device="cuda:0"),  # host-only tables
        dict(mode="sample", consensus=t, n=4, max_seq_len=65),                       # T > max_len
        dict(mode="sample", consensus=t, n=L.CONSENSUS_MAX_CANDS + 1, max_seq_len=8),
        dict(mode="sample", consensus=t, n=0, max_seq_len=8),
        dict(mode="sample", consensus=t, n=64, max_seq_len=39),                      # above one work-group's LDS
        dict(mode="beam", consensus=object(), n=4, max_seq_len=8),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
        print("refused:", {k: v for k, v in kw.items() if k != "consensus"})

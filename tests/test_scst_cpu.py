"""The host side of self-critical training (no GPU): the CIDEr-D reward on
token ids against utils.coco_eval.Cider, the advantage arithmetic of both
baselines, and the packing of sampled captions into training rows."""
import numpy as np
import pytest

# five images, 2-3 references each, with shared and repeated n-grams
CORPUS = {
    "a": [[5, 6, 7, 8, 9, 6, 7], [5, 6, 7, 10, 11], [12, 6, 7, 8]],
    "b": [[5, 13, 14, 15, 16], [17, 13, 14, 15, 16, 18]],
    "c": [[5, 6, 19, 20, 21, 22, 23, 24], [5, 6, 19, 25, 21], [26, 27, 19, 20]],
    "d": [[30, 31, 32, 33], [30, 31, 34, 33, 35]],
    "e": [[5, 6, 7, 8, 40, 41], [42, 43, 44, 6, 7]],
}
CANDS = {
    "a": [5, 6, 7, 8, 9],
    "b": [5, 13, 14, 14, 14, 16, 99],   # repeats (the clipped counts) and an unseen word
    "c": [26, 27, 19, 20],              # one reference verbatim
    "d": [50, 51],                      # nothing in common
    "e": [6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7],  # much longer than the references
}


def _text(ids):
    return " ".join(f"w{t}" for t in ids)


def test_reward_equals_the_coco_cider_per_image():
    from utils.cider_reward import CiderDReward
    from utils.coco_eval import Cider
    gts = {k: [_text(r) for r in rs] for k, rs in CORPUS.items()}
    res = {k: [_text(CANDS[k])] for k in CORPUS}
    mean, per_image = Cider().compute_score(gts, res)
    rw = CiderDReward.from_corpus(CORPUS)
    keys = list(CORPUS)
    got = rw.score(keys, [[CANDS[k]] for k in keys])
    assert got.shape == (5,) and got.dtype == np.float64
    assert float(np.abs(got - per_image).max()) <= 1e-12, (got, per_image)
    assert abs(float(got.mean()) - mean) <= 1e-12
    assert got[2] > got[0] > 0 and got[3] == 0.0  # a verbatim reference scores high, no overlap scores 0


def test_reward_scores_any_number_of_candidates():
    from utils.cider_reward import CiderDReward
    rw = CiderDReward.from_corpus(CORPUS)
    many = rw.score(["a", "c", "d"], [[CANDS["a"], CANDS["b"], CANDS["e"]], [], [CANDS["c"], CANDS["a"]]])
    one = [rw.score(["a"], [[c]])[0] for c in (CANDS["a"], CANDS["b"], CANDS["e"])] + \
          [rw.score(["d"], [[c]])[0] for c in (CANDS["c"], CANDS["a"])]
    assert many.tolist() == one
    assert rw("a", CANDS["a"]) == one[0]  # the callable form train_step_scst takes
    # a sequence of reference lists gets the keys 0, 1, ...
    rw2 = CiderDReward.from_corpus(list(CORPUS.values()))
    assert rw2.score([0], [[CANDS["a"]]])[0] == one[0]
    with pytest.raises(ValueError):
        rw.score(["a"], [[CANDS["a"]], [CANDS["b"]]])
    with pytest.raises(ValueError):
        CiderDReward.from_corpus({"x": []})


def test_an_empty_candidate_scores_zero():
    from utils.cider_reward import CiderDReward
    rw = CiderDReward.from_corpus(CORPUS)
    assert rw.score(["a", "b"], [[[]], [[], CANDS["b"]]]).tolist()[:2] == [0.0, 0.0]


def test_advantages_of_both_baselines():
    from fpnmt.scst import advantages
    r = [[1.0, 2.0, 6.0], [0.5, 0.5, 0.5]]
    adv, base = advantages(r, "mean")
    # against the mean of the OTHER samples: (2 + 6) / 2, (1 + 6) / 2, (1 + 2) / 2
    assert base.tolist() == [[4.0, 3.5, 1.5], [0.5, 0.5, 0.5]]
    assert adv.tolist() == [[-3.0, -1.5, 4.5], [0.0, 0.0, 0.0]]
    adv, base = advantages(r, "greedy", greedy=[1.5, 2.0])
    assert base.tolist() == [[1.5, 1.5, 1.5], [2.0, 2.0, 2.0]]
    assert adv.tolist() == [[-0.5, 0.5, 4.5], [-1.5, -1.5, -1.5]]
    adv, _ = advantages([[3.0]], "greedy", greedy=[1.0])  # one sample is enough for the greedy baseline
    assert adv.tolist() == [[2.0]]
    with pytest.raises(ValueError):
        advantages([[3.0]], "mean")
    with pytest.raises(ValueError):
        advantages(r, "median")
    with pytest.raises(ValueError):
        advantages(r, "greedy", greedy=[1.0])
    with pytest.raises(ValueError):
        advantages([1.0, 2.0], "mean")


def test_token_packing():
    from fpnmt.scst import pack_tokens
    start, end, steps, width = 2, 3, 5, 6  # the sampler ran 5 positions; rows as wide as the captions
    rows = pack_tokens([[7, 8], [], [7, 8, 9, 10, 11], [7, 8, 9, 10]], width, start, end, steps)
    assert rows.dtype == np.int64 and rows.shape == (4, width)
    assert rows.tolist() == [
        [2, 7, 8, 3, 0, 0],     # ended: <end> follows, then pads
        [2, 3, 0, 0, 0, 0],     # an empty sample: <end> at once
        [2, 7, 8, 9, 10, 11],   # ran all 5 positions without <end>: none appended
        [2, 7, 8, 9, 10, 3],    # <end> drawn at the last position
    ]
    # a narrower table cuts the row
    assert pack_tokens([[7, 8, 9, 10]], 4, start, end, steps).tolist() == [[2, 7, 8, 9]]

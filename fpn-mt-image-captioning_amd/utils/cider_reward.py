"""CIDEr-D as a training reward on token ids (self-critical training).

The arithmetic is utils.coco_eval.Cider's (n = 4, sigma = 6, clipped counts,
x 10), restated so that what depends on the references alone is computed
once: the n-gram document frequencies and log(#images) of the given corpus,
and every image's reference vectors, norms and lengths. A candidate then costs
its own n-gram counts and one pass over its image's references. Captions are
lists of token ids — ids are the words, so no tokenizer is involved — and any
number of candidates per image can be scored (Cider.compute_score takes
exactly one, and recomputes the frequencies from the images it is given).
"""
from collections import defaultdict

import numpy as np


def ngram_counts(ids, n):
    """{n-gram tuple: count} for the 1..n-grams of ids, in the insertion
    order of utils.coco_eval._ngrams (the sums below run in dict order)."""
    counts = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(ids) - k + 1):
            counts[tuple(ids[i:i + k])] += 1
    return counts


def consensus_of(pair, weights=None):
    """The consensus utilities and the pick from an (n, n) similarity matrix
    (CiderDReward.consensus states the definition): plain float64 sums over
    ascending j."""
    n = len(pair)
    p = [1.0] * n if weights is None else [float(w) for w in weights]
    if len(p) != n:
        raise ValueError(f"{len(p)} weights for {n} candidates")
    if any(not w >= 0.0 for w in p):
        raise ValueError(f"consensus weights must be non-negative, got {p}")
    util = np.zeros(n, dtype=np.float64)
    for s in range(n):
        num = den = 0.0
        for j in range(n):
            if j != s:
                num += p[j] * float(pair[s][j])
                den += p[j]
        util[s] = num / den if den != 0.0 else 0.0
    pick = 0
    for s in range(1, n):
        if util[s] > util[pick]:
            pick = s
    return util, pick


class CiderDReward:
    def __init__(self, df, n_images, refs, n=4, sigma=6.0):
        self._n, self._sigma = n, sigma
        self._df = df
        self._ref_len = np.log(float(n_images))
        # image key -> [(vec, norm, length)] per reference
        self._refs = {k: [self._vec(ngram_counts(r, n)) for r in rs] for k, rs in refs.items()}

    @classmethod
    def from_corpus(cls, refs_per_image, n=4, sigma=6.0):
        """refs_per_image: {image key: [token-id list, ...]} or a sequence of
        such lists (the keys are then 0, 1, ...). The document frequency of
        an n-gram is the number of images one of whose references holds it."""
        if not isinstance(refs_per_image, dict):
            refs_per_image = dict(enumerate(refs_per_image))
        refs = {}
        for k, rs in refs_per_image.items():
            rs = [[int(t) for t in r] for r in rs]
            if not rs:
                raise ValueError(f"CiderDReward: image {k!r} has no reference caption")
            refs[k] = rs
        df = defaultdict(float)
        for rs in refs.values():
            for g in {g for r in rs for g in ngram_counts(r, n)}:
                df[g] += 1
        return cls(df, len(refs), refs, n, sigma)

    def _vec(self, cnts):
        n = self._n
        vec = [{} for _ in range(n)]
        norm = [0.0] * n
        length = 0
        for g, tf in cnts.items():
            d = np.log(max(1.0, self._df.get(g, 0.0)))
            k = len(g) - 1
            vec[k][g] = float(tf) * (self._ref_len - d)
            norm[k] += pow(vec[k][g], 2)
            if k == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def _sim(self, vh, vr, nh, nr, lh, lr):
        n = self._n
        delta = float(lh - lr)
        val = np.array([0.0] * n)
        for k in range(n):
            for g in vh[k]:
                r = vr[k].get(g, 0.0)
                val[k] += min(vh[k][g], r) * r
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * self._sigma ** 2))
        return val

    def score_one(self, image_key, candidate):
        refs = self._refs[image_key]
        vec, norm, length = self._vec(ngram_counts([int(t) for t in candidate], self._n))
        score = np.array([0.0] * self._n)
        for vr, nr, lr in refs:
            score += self._sim(vec, vr, norm, nr, length, lr)
        return float(np.mean(score) / len(refs) * 10.0)

    def score(self, image_keys, candidates):
        """candidates[i]: the candidate captions (token-id lists) of image
        image_keys[i], any number each -> their scores, flattened in order
        (float64)."""
        if len(image_keys) != len(candidates):
            raise ValueError(f"{len(image_keys)} image keys for {len(candidates)} candidate lists")
        return np.array([self.score_one(k, c) for k, cs in zip(image_keys, candidates) for c in cs], dtype=np.float64)

    # ---- consensus (minimum-Bayes-risk) selection among an image's candidates
    def pairwise(self, candidates):
        """(n, n) float64: [s][j] = sim(c_s, c_j), the CIDEr-D of candidate s
        with candidate j as its ONLY reference (score_one's arithmetic on the
        two _vec's; the corpus supplies the idf). Not symmetric; the diagonal
        is the self-similarity."""
        vecs = [self._vec(ngram_counts([int(t) for t in c], self._n)) for c in candidates]
        out = np.zeros((len(vecs), len(vecs)), dtype=np.float64)
        for s, (vh, nh, lh) in enumerate(vecs):
            for j, (vr, nr, lr) in enumerate(vecs):
                out[s, j] = float(np.mean(self._sim(vh, vr, nh, nr, lh, lr)) / 1 * 10.0)
        return out

    def consensus(self, candidates, weights=None):
        """(util, pick): util[s] = sum_{j != s} p_j sim(c_s, c_j) / sum_{j !=
        s} p_j over ascending j (0 where the denominator is 0; p = weights,
        non-negative, None: all 1); pick = the index of the greatest util,
        ties to the lowest. Self is excluded by INDEX: a duplicate at another
        index counts, so for samples util is a Monte Carlo estimate of the
        expected CIDEr-D. An empty caption has utility 0 and contributes 0;
        one candidate alone has utility 0."""
        return consensus_of(self.pairwise(candidates), weights)

    def __call__(self, image_key, candidate):
        return self.score_one(image_key, candidate)

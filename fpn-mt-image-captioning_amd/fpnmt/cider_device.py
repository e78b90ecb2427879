"""CIDEr-D reference tables for the device-side reward (fpnmt_ciderd_reward).

Everything utils.cider_reward.CiderDReward derives from the references alone
is packed once, on the host, into flat arrays the kernel binary-searches:

  key       a k-gram (k <= 4) as ONE uint64, sum_i (tok_i + 1) << (16 * i).
            Absent positions are 0 and present ones never are, so the order
            is recoverable from the key, keys of different orders never
            collide, and nothing is hashed: the packing is exact for
            0 <= tok <= 65 533.
  document  df_keys u64[G] ascending and unique, df_idf f64[G] with
            idf = log(N) - log(max(1, df)); an n-gram absent from the table
            has idf log(N) (idf_absent).
  refs      CSR: img_off[I + 1] -> the references of image i, ref_off[R + 1]
            -> the entries of reference j, sorted by key; ref_keys u64[E],
            ref_w f64[E] = tf * idf, ref_norm f64[R][4], ref_len int32[R]
            (CiderDReward's "length": the sum of the BIGRAM counts).
  gauss     gauss[d] = e ** (-(d ** 2) / (2 sigma ** 2)), d = 0 .. max_len +
            the longest reference length.

Every idf, tf * idf and Gaussian factor is evaluated with the scalar
expression CiderDReward uses, so the tables hold its values bit for bit and
the kernel evaluates no transcendental function. The tables are built with
numpy (sliding windows, np.unique / sorting on the packed keys): seconds for
a COCO-sized corpus. `host` is a CiderDReward of the same corpus (built on
first use: it is the pure-Python form); `score_host` walks the PACKED tables
with numpy, which lets them be checked without a GPU.

The intended use is ONE instance over the whole training set, with
image_keys naming each batch's images (SelfCriticalTrainer.step).

The same document table serves consensus (minimum-Bayes-risk) selection
among an image's candidate captions (fpnmt_ciderd_consensus): there the
"references" are the other candidates, so only df_keys / df_idf, idf_absent
and the Gaussian table are read. `consensus` is the launch, `consensus_host`
/ `pairwise_host` walk the packed arrays with numpy, `consensus_check` says
before any device work whether a shape is served.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CIDER_MAX_LEN  # the kernel's LDS key table

MAX_TOKEN = 65533


class CiderTables(C.Structure):
    """fpnmt_cider_tables (include/fpnmt.h)."""
    _fields_ = [
        ("df_keys", C.c_void_p), ("df_idf", C.c_void_p), ("n_df", C.c_longlong), ("idf_absent", C.c_double),
        ("img_off", C.c_void_p), ("n_images", C.c_int), ("max_len", C.c_int),
        ("ref_off", C.c_void_p), ("ref_keys", C.c_void_p), ("ref_w", C.c_void_p), ("ref_norm", C.c_void_p),
        ("ref_len", C.c_void_p), ("gauss", C.c_void_p), ("n_gauss", C.c_int),
    ]


def pack_keys(ids, k):
    """The uint64 keys of the k-grams of ids, in position order."""
    t = np.asarray(ids, dtype=np.int64).astype(np.uint64) + np.uint64(1)
    m = len(t) - k + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64)
    key = np.zeros(m, dtype=np.uint64)
    for i in range(k):
        key |= t[i:i + m] << np.uint64(16 * i)
    return key


def unpack_key(key):
    """The n-gram (a tuple of token ids) a key stands for."""
    key, out = int(key), []
    while key:
        out.append((key & 0xFFFF) - 1)
        key >>= 16
    return tuple(out)


def key_order(keys):
    """1 .. 4: the number of tokens packed in each (non-zero) key."""
    k = np.asarray(keys, dtype=np.uint64)
    return (1 + (k >= np.uint64(1 << 16)).astype(np.int64) + (k >= np.uint64(1 << 32)).astype(np.int64)
            + (k >= np.uint64(1 << 48)).astype(np.int64))


class DeviceCiderD:
    def __init__(self, arrays, keys, n_images, sigma, max_len, device, corpus):
        import torch
        self.n, self.sigma, self.max_len = 4, float(sigma), int(max_len)
        self.keys = list(keys)
        self._row = {k: i for i, k in enumerate(self.keys)}
        self.n_images = n_images
        self.idf_absent = float(arrays["idf_absent"])
        self.np = arrays  # the host copies (score_host, tests)
        self.device = torch.device(device)
        self._corpus, self._host = corpus, None
        self.dev = {}
        if self.device.type != "cpu":
            for name, a in arrays.items():
                if isinstance(a, np.ndarray):
                    if a.dtype == np.uint64:
                        a = a.view(np.int64)  # the same bits; the kernel reads them unsigned
                    # a one-element pad keeps empty tables addressable
                    self.dev[name] = torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.device)
            d = self.dev
            self.device = d["gauss"].device  # with its index ("cuda" -> "cuda:0")
            t = self.tables = CiderTables()
            t.df_keys, t.df_idf = d["df_keys"].data_ptr(), d["df_idf"].data_ptr()
            t.n_df, t.idf_absent = len(arrays["df_keys"]), self.idf_absent
            t.img_off, t.n_images, t.max_len = d["img_off"].data_ptr(), n_images, self.max_len
            t.ref_off, t.ref_keys, t.ref_w = d["ref_off"].data_ptr(), d["ref_keys"].data_ptr(), d["ref_w"].data_ptr()
            t.ref_norm, t.ref_len = d["ref_norm"].data_ptr(), d["ref_len"].data_ptr()
            t.gauss, t.n_gauss = d["gauss"].data_ptr(), len(arrays["gauss"])

    # ----------------------------------------------------------------- build
    @classmethod
    def from_corpus(cls, refs_per_image, device="cpu", n=4, sigma=6.0, max_len=64):
        """refs_per_image: what CiderDReward.from_corpus takes, {image key:
        [token-id list, ...]} or a sequence of such lists (keys 0, 1, ...).
        max_len: the longest candidate the tables serve (the Gaussian table
        and the kernel's key buffer), at most 128. device "cpu" builds the
        host arrays only (score_host)."""
        if n != 4:
            raise ValueError(f"DeviceCiderD packs 1..4-grams into 64 bits: n must be 4, got {n}")
        if not 1 <= max_len <= CIDER_MAX_LEN:
            raise ValueError(f"max_len must lie in 1..{CIDER_MAX_LEN}, got {max_len}")
        if not isinstance(refs_per_image, dict):
            refs_per_image = dict(enumerate(refs_per_image))
        keys, flat, img_off = [], [], [0]
        for k, rs in refs_per_image.items():
            rs = [np.asarray([int(t) for t in r], dtype=np.int64) for r in rs]
            if not rs:
                raise ValueError(f"DeviceCiderD: image {k!r} has no reference caption")
            keys.append(k)
            flat.extend(rs)
            img_off.append(len(flat))
        if not keys:
            raise ValueError("DeviceCiderD: an empty corpus")
        I, R = len(keys), len(flat)
        lens = np.array([len(r) for r in flat], dtype=np.int64)
        toks = np.concatenate(flat) if lens.sum() else np.zeros(0, dtype=np.int64)
        if toks.size and (int(toks.min()) < 0 or int(toks.max()) > MAX_TOKEN):
            raise ValueError(f"DeviceCiderD: token ids must lie in 0..{MAX_TOKEN} (16 bits per position, 0 kept for "
                             f"'absent'), got {int(toks.min())}..{int(toks.max())}")
        rid = np.repeat(np.arange(R, dtype=np.int64), lens)
        t1 = toks.astype(np.uint64) + np.uint64(1)
        all_keys, all_rid = [], []
        for k in range(1, 5):  # sliding windows that stay inside one reference
            m = len(t1) - k + 1
            if m <= 0:
                break
            inside = rid[:m] == rid[k - 1:]
            key = np.zeros(m, dtype=np.uint64)
            for i in range(k):
                key |= t1[i:i + m] << np.uint64(16 * i)
            all_keys.append(key[inside])
            all_rid.append(rid[:m][inside])
        gk = np.concatenate(all_keys) if all_keys else np.zeros(0, dtype=np.uint64)
        gr = np.concatenate(all_rid) if all_rid else np.zeros(0, dtype=np.int64)
        # entries: the distinct (reference, key) pairs with their counts, by reference, then key
        order = np.lexsort((gk, gr))
        gk, gr = gk[order], gr[order]
        new = np.ones(len(gk), dtype=bool)
        if len(gk) > 1:
            new[1:] = (gk[1:] != gk[:-1]) | (gr[1:] != gr[:-1])
        start = np.flatnonzero(new)
        e_key, e_rid = gk[start], gr[start]
        e_tf = np.diff(np.append(start, len(gk)))
        ref_off = np.zeros(R + 1, dtype=np.int64)
        np.cumsum(np.bincount(e_rid, minlength=R), out=ref_off[1:])
        # document frequency: the number of IMAGES one of whose references holds the key
        img_of_ref = np.repeat(np.arange(I, dtype=np.int64), np.diff(img_off))
        e_img = img_of_ref[e_rid]
        o2 = np.lexsort((e_img, e_key))
        k2, i2 = e_key[o2], e_img[o2]
        pair_new = np.ones(len(k2), dtype=bool)
        if len(k2) > 1:
            pair_new[1:] = (k2[1:] != k2[:-1]) | (i2[1:] != i2[:-1])
        df_keys, df = np.unique(k2[pair_new], return_counts=True)
        # one idf per DISTINCT df, by CiderDReward._vec's scalar expression
        log_n = np.log(float(I))
        idf_of = {int(v): log_n - np.log(max(1.0, float(v))) for v in np.unique(df)}
        df_idf = np.array([idf_of[int(v)] for v in df], dtype=np.float64)
        idf_absent = log_n - np.log(max(1.0, 0.0))
        e_w = e_tf.astype(np.float64) * df_idf[np.searchsorted(df_keys, e_key)] if len(e_key) else \
            np.zeros(0, dtype=np.float64)
        e_ord = key_order(e_key) - 1
        ref_norm = np.sqrt(np.bincount(e_rid * 4 + e_ord, weights=e_w * e_w, minlength=4 * R)).reshape(R, 4)
        ref_len = np.bincount(e_rid[e_ord == 1], weights=e_tf[e_ord == 1], minlength=R).astype(np.int32)
        max_ref = int(ref_len.max()) if R else 0
        gauss = np.array([np.e ** (-(float(d) ** 2) / (2 * sigma ** 2)) for d in range(max_len + max_ref + 1)],
                         dtype=np.float64)
        arrays = dict(df_keys=df_keys.astype(np.uint64), df_idf=df_idf, idf_absent=np.float64(idf_absent),
                      img_off=np.asarray(img_off, dtype=np.int32), ref_off=ref_off,
                      ref_keys=e_key.astype(np.uint64), ref_w=e_w, ref_norm=np.ascontiguousarray(ref_norm),
                      ref_len=ref_len, gauss=gauss)
        corpus = {k: [r.tolist() for r in flat[img_off[i]:img_off[i + 1]]] for i, k in enumerate(keys)}
        return cls(arrays, keys, I, sigma, max_len, device, corpus)

    @property
    def host(self):
        """The CiderDReward of the same corpus (the host reference and the
        fallback for callers without a device)."""
        if self._host is None:
            from utils.cider_reward import CiderDReward
            self._host = CiderDReward.from_corpus(self._corpus, n=4, sigma=self.sigma)
        return self._host

    # ---------------------------------------------------------------- lookup
    def rows_of(self, keys):
        """Image keys -> their table rows (a list); an unknown key is a
        ValueError."""
        try:
            return [self._row[k] for k in keys]
        except (KeyError, TypeError) as e:
            raise ValueError(f"DeviceCiderD: unknown image key {e.args[0]!r}") from None

    def index_of(self, keys):
        """rows_of as an int32 CPU tensor, the img_index the kernel takes
        (once copied to the device)."""
        import torch
        return torch.tensor(self.rows_of(keys), dtype=torch.int32)

    # --------------------------------------------------------- host restatement
    def _score_one(self, row, cand):
        a = self.np
        cand = [int(t) for t in cand]
        keys = np.concatenate([pack_keys(cand, k) for k in range(1, 5)]) if cand else np.zeros(0, dtype=np.uint64)
        ck, tf = np.unique(keys, return_counts=True)
        pos = np.searchsorted(a["df_keys"], ck)
        pos_c = np.minimum(pos, max(len(a["df_keys"]) - 1, 0))
        hit = (pos < len(a["df_keys"])) & (a["df_keys"][pos_c] == ck) if len(a["df_keys"]) else np.zeros(len(ck), bool)
        idf = np.where(hit, a["df_idf"][pos_c] if len(a["df_idf"]) else 0.0, self.idf_absent)
        w = tf.astype(np.float64) * idf
        od = key_order(ck) - 1
        nh = np.sqrt(np.bincount(od, weights=w * w, minlength=4))
        lh = int(tf[od == 1].sum())
        score = np.zeros(4)
        j0, j1 = int(a["img_off"][row]), int(a["img_off"][row + 1])
        for j in range(j0, j1):
            e0, e1 = int(a["ref_off"][j]), int(a["ref_off"][j + 1])
            rk, rw = a["ref_keys"][e0:e1], a["ref_w"][e0:e1]
            p = np.searchsorted(rk, ck)
            pc = np.minimum(p, max(e1 - e0 - 1, 0))
            r = np.where((p < e1 - e0) & (rk[pc] == ck), rw[pc], 0.0) if e1 > e0 else np.zeros(len(ck))
            val = np.bincount(od, weights=np.minimum(w, r) * r, minlength=4)
            nr = a["ref_norm"][j]
            for k in range(4):
                if nh[k] != 0 and nr[k] != 0:
                    val[k] /= nh[k] * nr[k]
                val[k] *= a["gauss"][abs(lh - int(a["ref_len"][j]))]
            score += val
        return float(np.mean(score) / (j1 - j0) * 10.0)

    def score_host(self, image_index, candidates):
        """CiderDReward.score restated on the packed tables: candidates[i]
        are the candidates of table row image_index[i]; their scores,
        flattened in order (float64). The same binary searches and clipping
        as the kernel."""
        if len(image_index) != len(candidates):
            raise ValueError(f"{len(image_index)} image rows for {len(candidates)} candidate lists")
        for cs in candidates:
            for c in cs:
                if len(c) > self.max_len:
                    raise ValueError(f"a candidate of {len(c)} tokens exceeds max_len {self.max_len}")
        return np.array([self._score_one(int(i), c) for i, cs in zip(image_index, candidates) for c in cs],
                        dtype=np.float64)

    def _cand_vec(self, cand):
        """A candidate's distinct packed keys (ascending), tf * idf, orders,
        four norms and length (the bigram count), from the document table."""
        a = self.np
        cand = [int(t) for t in cand]
        keys = np.concatenate([pack_keys(cand, k) for k in range(1, 5)]) if cand else np.zeros(0, dtype=np.uint64)
        ck, tf = np.unique(keys, return_counts=True)
        pos = np.searchsorted(a["df_keys"], ck)
        pos_c = np.minimum(pos, max(len(a["df_keys"]) - 1, 0))
        hit = (pos < len(a["df_keys"])) & (a["df_keys"][pos_c] == ck) if len(a["df_keys"]) else np.zeros(len(ck), bool)
        idf = np.where(hit, a["df_idf"][pos_c] if len(a["df_idf"]) else 0.0, self.idf_absent)
        w = tf.astype(np.float64) * idf
        od = key_order(ck) - 1
        return ck, w, od, np.sqrt(np.bincount(od, weights=w * w, minlength=4)), int(tf[od == 1].sum())

    def pairwise_host(self, candidates):
        """CiderDReward.pairwise restated on the packed document table: (n,
        n) float64, [s][j] = the CIDEr-D of candidate s with candidate j as
        its only reference. The same keys, searches and clipping as
        fpnmt_ciderd_consensus."""
        for c in candidates:
            if len(c) > self.max_len:
                raise ValueError(f"a candidate of {len(c)} tokens exceeds max_len {self.max_len}")
        vecs = [self._cand_vec(c) for c in candidates]
        gauss = self.np["gauss"]
        out = np.zeros((len(vecs), len(vecs)), dtype=np.float64)
        for s, (hk, hw, hod, nh, lh) in enumerate(vecs):
            for j, (rk, rw, _, nr, lr) in enumerate(vecs):
                if not len(hk) or not len(rk):
                    continue
                p = np.searchsorted(rk, hk)
                pc = np.minimum(p, len(rk) - 1)
                r = np.where((p < len(rk)) & (rk[pc] == hk), rw[pc], 0.0)
                val = np.bincount(hod, weights=np.minimum(hw, r) * r, minlength=4)
                for k in range(4):
                    if nh[k] != 0 and nr[k] != 0:
                        val[k] /= nh[k] * nr[k]
                    val[k] *= gauss[abs(lh - lr)]
                out[s, j] = float(np.mean(val) * 10.0)
        return out

    def consensus_host(self, candidates_per_image, weights=None):
        """CiderDReward.consensus restated on the packed tables, per image:
        candidates_per_image[i] are image i's candidate token-id lists,
        weights[i] (optional) their non-negative weights -> a list of (util
        float64[n_i], pick) pairs. Checks the packing without a GPU."""
        from utils.cider_reward import consensus_of
        if weights is not None and len(weights) != len(candidates_per_image):
            raise ValueError(f"{len(weights)} weight rows for {len(candidates_per_image)} images")
        return [consensus_of(self.pairwise_host(cs), None if weights is None else weights[i])
                for i, cs in enumerate(candidates_per_image)]

    # ---------------------------------------------------------------- launch
    @staticmethod
    def consensus_lds_bytes(n, max_tokens):
        """The LDS fpnmt_ciderd_consensus needs for n candidates of up to
        max_tokens tokens (include/fpnmt.h): at most CONSENSUS_LDS_BYTES."""
        e = sum(max(max_tokens - k, 0) for k in range(4))
        return 16 * n * e + 64 * e + 44 * n

    def consensus_check(self, n, max_tokens, device=None):
        """ValueError unless fpnmt_ciderd_consensus serves n candidates per
        image of up to max_tokens tokens from these tables (on `device`, when
        given). Raises before any device work."""
        import torch
        from ._lib import CONSENSUS_LDS_BYTES, CONSENSUS_MAX_CANDS
        if self.device.type == "cpu":
            raise ValueError("consensus needs DeviceCiderD tables built on the GPU (from_corpus(..., device=...))")
        if device is not None:
            device = torch.device(device)
            if device.type != self.device.type or (device.index is not None and device.index != self.device.index):
                raise ValueError(f"the consensus tables live on {self.device}, the decoder on {device}")
        if not 1 <= n <= CONSENSUS_MAX_CANDS:
            raise ValueError(f"consensus serves 1..{CONSENSUS_MAX_CANDS} candidates per image, got {n}")
        if max_tokens > self.max_len:
            raise ValueError(f"captions of up to {max_tokens} tokens exceed the consensus tables' max_len "
                             f"{self.max_len}")
        need = self.consensus_lds_bytes(n, max_tokens)
        if need > CONSENSUS_LDS_BYTES:
            raise ValueError(f"consensus over {n} candidates of up to {max_tokens} tokens needs {need} bytes of LDS, "
                             f"above the {CONSENSUS_LDS_BYTES} of a work-group: fewer candidates or a shorter "
                             "max_seq_len")

    def consensus(self, hist, len, fin, n, util, pick, weight=None, pair=None):
        """fpnmt_ciderd_consensus over pick.numel() images of n candidate
        rows each, laid out as the sampler and the beam search leave them
        (row r's caption is hist[r][1 : 1 + len[r] - fin[r]]): util (f64,
        rows) the consensus utilities, pick (int32, images) the index of the
        greatest per image; weight (f64, rows; None: uniform) the candidates'
        non-negative weights, pair (f64, images * n * n; None: not wanted)
        every sim(c_s, c_j). At most CONSENSUS_MAX_CANDS candidates whose keys
        fit one work-group's LDS (consensus_lds_bytes(n, hist.shape[1] - 1) <=
        CONSENSUS_LDS_BYTES). No allocation, no synchronisation, capturable."""
        from ._lib import call, ptr, stream_ptr
        call("fpnmt_ciderd_consensus", C.byref(self.tables), pick.numel(), n, ptr(hist), hist.stride(0), ptr(len),
             ptr(fin), ptr(weight), ptr(util), ptr(pick), ptr(pair), stream_ptr())
        return util, pick

    def reward(self, hist, slen, fin, img_index, n, out):
        """fpnmt_ciderd_reward over out.numel() caption rows (n per image):
        out[r] (f64) = the CIDEr-D of hist[r][1 : 1 + slen[r] - fin[r]]
        against the references of table row img_index[r // n]. No
        allocation, no synchronisation, capturable."""
        from ._lib import call, ptr, stream_ptr
        call("fpnmt_ciderd_reward", C.byref(self.tables), out.numel(), n, ptr(hist), hist.stride(0), ptr(slen),
             ptr(fin), ptr(img_index), ptr(out), stream_ptr())
        return out

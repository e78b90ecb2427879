"""fpnmt_logits_ensemble (csrc/ensemble.hip) against tests/ensemble_ref.py, the
fp64 restatement of include/fpnmt.h's row semantics, on the same fp32 inputs.

The error bound (bound() below), from the roundings of the kernel's fp32
arithmetic. u = 2^-24 is fp32's unit roundoff; e = 2^-23 is the relative error
of the device expf and logf (1 ulp, the figure HIP's math API documents for
both); V the vocabulary, M the models, Lmax the largest finite |logit| of the
case, Wl the largest |log w_m|. Results that underflow to denormals add less
than V * 2^-126 and are left out.

lse_m = max + logf(s), s = sum_j expf(l_j - max) by an online (max, sum): a
term reaches the final sum as expf(l_j - m_0) times a chain of rescales
expf(m_i - m_{i+1}), one per change of a thread's running maximum (at most one
per sweep step, ceil(V / 1024) + 2 of them), then 6 shuffle merges and 3 merges
across the waves. The arguments of that chain are all <= 0 and telescope to
d_j = l_j - max, so the rounding of the subtractions costs the term u * |d_j| in
all, and each of the at most K = ceil(V / 1024) + 12 factors costs e (the expf)
+ u (the product) and each of the as many additions u: a relative error of
K (e + 2 u) + u |d_j| per term. Weighted by the terms' share p_j of s, sum_j
p_j |d_j| = max - lse + H(p) <= ln V. So s is off by at most K (e + 2 u) + u ln V
relatively, which is the absolute error of log s; logf adds e * ln V (log s <=
ln V) and the final addition u * |lse|, |lse| <= B = Lmax + ln V:
  d_lse = K (e + 2 u) + (u + e) ln V + u B.
mode 1: fl(l - lse_m) adds u * A, A = Lmax + B >= |l - lse|; the product with
w_m u * A; the M additions at most M u A (sum w = 1 up to M u, carried by the
factor wsum): d_1 = wsum * (d_lse + (M + 2) u A).
mode 0: c_m = fl(fl32(log w_m) - lse_m) is off by d_lse + u Wl + u (B + Wl);
a_m = fl(l + c_m) by u (Lmax + B + Wl) more: d_a = d_lse + u (3 Wl + 2 B + Lmax).
logsumexp_m is 1-Lipschitz in the largest input error, d_a. Its own
arithmetic, as for lse with M terms: the sum is off by e + (M - 1) u + u ln M
relatively, logf by e ln M, the last addition by u (Lmax + B + Wl + ln M):
  d_0 = d_a + e (1 + ln M) + u (M - 1 + ln M) + u (Lmax + B + Wl + ln M).
-inf columns carry no error: they must match exactly."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ensemble_ref import ensemble_rows, normalise

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = np.float32(-np.inf)
SENT = np.float32(12345.0)  # padding columns, finished rows: never written
U, E = 2.0 ** -24, 2.0 ** -23
VOCABS = [5, 64, 65, 200, 1023, 10007]
N_MODELS = [1, 2, 3, 8]
MODES = ("prob", "logprob")


def bound(vocab, n_models, lmax, weights, mode):
    lnv, lnm = math.log(vocab), math.log(n_models)
    wl, wsum = max(abs(math.log(w)) for w in weights), sum(weights)
    k = math.ceil(vocab / 1024) + 12
    b = lmax + lnv
    d_lse = k * (E + 2 * U) + (U + E) * lnv + U * b
    if mode == "logprob":
        return wsum * (d_lse + (n_models + 2) * U * (lmax + b))
    d_a = d_lse + U * (3 * wl + 2 * b + lmax)
    return d_a + E * (1 + lnm) + U * (n_models - 1 + lnm) + U * (lmax + b + wl + lnm)


def _w32(weights, n_models):
    """The host's normalisation, then what the kernel is given: fp32 values."""
    return [float(np.float32(w)) for w in normalise(weights, n_models)]


def _launch(bufs, vocab, weights, mode, fin=None, out=None, ldo=None, rows=None, inplace=False, expect=0,
            n_models=None, ldl=None, null=()):
    """bufs: per model a (rows, ld_m) fp32 numpy array whose first `vocab`
    columns are the logits. Returns the whole out buffer (rows, ldo) back."""
    from fpnmt import _lib as L
    n = len(bufs) if n_models is None else n_models
    rows = bufs[0].shape[0] if rows is None else rows
    dev, ptrs = {}, []
    for b in bufs:  # the same numpy object twice: the same device buffer twice
        if id(b) not in dev:
            dev[id(b)] = torch.from_numpy(b).to(DEV)
        ptrs.append(dev[id(b)].data_ptr())
    if inplace:
        o, ldo = dev[id(bufs[0])], bufs[0].shape[1]
    else:
        ldo = vocab if ldo is None else ldo
        o = torch.full((bufs[0].shape[0], ldo), float(SENT), device=DEV) if out is None else torch.from_numpy(out).to(DEV)
    f = None if fin is None else torch.tensor(fin, dtype=torch.int32, device=DEV)
    ld = [b.shape[1] for b in bufs] if ldl is None else ldl
    m = len(ptrs)
    args = dict(logits=(C.c_void_p * m)(*ptrs), ldl=(C.c_longlong * m)(*ld), weight=(C.c_float * m)(*weights),
                out=o.data_ptr())
    for k in null:
        args[k] = None
    rc = L.lib.fpnmt_logits_ensemble(rows, vocab, n, args["logits"], args["ldl"], args["weight"],
                                     {"prob": 0, "logprob": 1}.get(mode, mode), None if f is None else f.data_ptr(),
                                     args["out"], ldo, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib.fpnmt_last_error())
    return o.cpu().numpy()


def _check(out, bufs, vocab, weights, mode, fin=None, lmax=None, what=""):
    """out (rows, ldo) against the reference; returns the worst error / bound."""
    ref = ensemble_rows([b[:, :vocab] for b in bufs], weights, mode, fin)
    if lmax is None:
        finite = np.concatenate([b[:, :vocab][np.isfinite(b[:, :vocab])].ravel() for b in bufs])
        lmax = float(np.max(np.abs(finite))) if finite.size else 0.0
    bd = bound(vocab, len(bufs), lmax, weights, mode)
    worst = 0.0
    assert (out[:, vocab:] == SENT).all(), f"{what}: a column past vocab was written"
    for r, want in enumerate(ref):
        got = out[r, :vocab]
        if want is None:
            assert (got == SENT).all(), f"{what}: finished row {r} was written"
            continue
        if np.isnan(want).all():
            assert np.isnan(got).all(), f"{what}: bad row {r} is not NaN throughout"
            continue
        neg = np.isneginf(want)
        assert (got[neg] == NEG).all(), f"{what}: row {r}: a -inf column is {got[neg]}"
        assert np.isfinite(got[~neg]).all(), f"{what}: row {r}: a finite column is not finite"
        err = float(np.max(np.abs(got[~neg].astype(np.float64) - want[~neg]))) if (~neg).any() else 0.0
        worst = max(worst, err)
        assert err <= bd, f"{what}: row {r}: error {err:.3e} above the bound {bd:.3e}"
    return worst, bd


def _bufs(n_models, rows, vocab, lds, seed, scale=4.0, uniform=False):
    g = np.random.default_rng(seed)
    out = []
    for m in range(n_models):
        b = np.full((rows, lds[m]), SENT, dtype=np.float32)
        x = g.uniform(-scale, scale, (rows, vocab)) if uniform else g.normal(0.0, scale, (rows, vocab))
        b[:, :vocab] = x.astype(np.float32)
        out.append(b)
    return out


def _unequal(n_models):
    return [1.0 + (3 * m) % 5 for m in range(n_models)]  # 1, 4, 2, 5, 3, 1, 4, 2


@pytest.mark.parametrize("n_models", N_MODELS)
@pytest.mark.parametrize("vocab", VOCABS)
def test_kernel_matches_reference(vocab, n_models):
    """Both modes, equal and unequal weights, rows 1 and 5, ld == vocab
    exactly (odd vocab: every row starts at another alignment) and ld > vocab
    differing per model, N(0, 4^2) logits."""
    seed = 0
    for rows in (1, 5):
        for tight in (True, False):
            lds = [vocab if tight else vocab + 1 + (3 * m) % 7 for m in range(n_models)]
            ldo = vocab if tight else vocab + 5
            bufs = _bufs(n_models, rows, vocab, lds, seed := seed + 1)
            for mode in MODES:
                for wts in (None, _unequal(n_models)):
                    w = _w32(wts, n_models)
                    out = _launch(bufs, vocab, w, mode, ldo=ldo)
                    what = f"V {vocab} M {n_models} rows {rows} {'ld==V' if tight else 'ld>V'} {mode} w {wts}"
                    worst, bd = _check(out, bufs, vocab, w, mode, what=what)
                    print(f"{what}: worst error {worst:.3e}, bound {bd:.3e}")


@pytest.mark.parametrize("mode", MODES)
def test_kernel_large_logits(mode):
    """Logits over +-80: a sum of exp of raw logits would overflow fp32."""
    vocab, n_models, rows = 1023, 3, 5
    bufs = _bufs(n_models, rows, vocab, [vocab + 2, vocab, vocab + 1], 50, scale=80.0, uniform=True)
    assert max(float(np.max(b[:, :vocab])) for b in bufs) > 79.0
    w = _w32(_unequal(n_models), n_models)
    out = _launch(bufs, vocab, w, mode, ldo=vocab + 3)
    worst, bd = _check(out, bufs, vocab, w, mode, what=f"+-80 {mode}")
    print(f"+-80 {mode}: worst error {worst:.3e}, bound {bd:.3e}")


@pytest.mark.parametrize("vocab", [65, 10007])
@pytest.mark.parametrize("n_models", [2, 4])
def test_logprob_of_one_buffer_is_exact(vocab, n_models):
    """mode 1 with every pointer the same buffer and equal weights (powers
    of two) == the n_models = 1 output, bit for bit."""
    buf = _bufs(1, 5, vocab, [vocab + 3], 60 + n_models)[0]
    one = _launch([buf], vocab, [1.0], "logprob", ldo=vocab + 1)
    many = _launch([buf] * n_models, vocab, [1.0 / n_models] * n_models, "logprob", ldo=vocab + 1)
    assert one.tobytes() == many.tobytes()
    _check(one, [buf], vocab, [1.0], "logprob", what="one model")


@pytest.mark.parametrize("mode", MODES)
def test_in_place_gives_the_same_bytes(mode):
    vocab, rows, n_models = 1023, 5, 3
    for ld0 in (vocab, vocab + 6):
        bufs = _bufs(n_models, rows, vocab, [ld0, vocab + 1, vocab], 70)
        w = _w32(_unequal(n_models), n_models)
        apart = _launch(bufs, vocab, w, mode, ldo=ld0)
        within = _launch(bufs, vocab, w, mode, inplace=True)
        assert apart[:, :vocab].tobytes() == within[:, :vocab].tobytes()
        assert (within[:, vocab:] == SENT).all()


@pytest.mark.parametrize("mode", MODES)
def test_finished_rows_and_padding_keep_the_sentinel(mode):
    """fin set: a finished row is neither read (its members' rows hold NaN)
    nor written, and the live rows are right."""
    vocab, rows, n_models = 200, 5, 2
    bufs = _bufs(n_models, rows, vocab, [vocab + 4, vocab], 80)
    fin = [0, 1, 0, 7, 0]
    for b in bufs:
        b[1, :vocab] = np.nan
        b[3, :vocab] = np.nan
    w = _w32(None, n_models)
    out = _launch(bufs, vocab, w, mode, fin=fin, ldo=vocab + 9)
    _check(out, bufs, vocab, w, mode, fin=fin, what=f"fin {mode}")
    assert np.isfinite(out[[0, 2, 4], :vocab]).all()


@pytest.mark.parametrize("mode", MODES)
def test_minus_inf_rules(mode):
    """A column -inf in one model only, one -inf in all models, and a row
    with vocab - 1 columns -inf in one model: exact -inf where the rule says
    so, finite elsewhere, never a NaN."""
    vocab, rows, n_models = 200, 3, 3
    bufs = _bufs(n_models, rows, vocab, [vocab, vocab + 2, vocab + 1], 90)
    bufs[1][0, 17] = NEG
    for b in bufs:
        b[0, 64] = NEG
    bufs[2][1, :vocab] = NEG
    bufs[2][1, 133] = 0.5
    w = _w32(_unequal(n_models), n_models)
    out = _launch(bufs, vocab, w, mode)
    _check(out, bufs, vocab, w, mode, what=f"-inf {mode}")
    assert not np.isnan(out).any()
    assert out[0, 64] == NEG
    assert (out[0, 17] == NEG) == (mode == "logprob")
    live = np.isfinite(out[1, :vocab])
    assert live.all() if mode == "prob" else np.flatnonzero(live).tolist() == [133]


@pytest.mark.parametrize("mode", MODES)
def test_bad_rows_are_nan_and_the_others_right(mode):
    vocab, rows, n_models = 1023, 5, 2
    bufs = _bufs(n_models, rows, vocab, [vocab, vocab + 3], 100)
    bufs[1][0, 1000] = np.nan
    bufs[0][2, 3] = np.inf
    bufs[1][4, :vocab] = NEG
    w = _w32(None, n_models)
    out = _launch(bufs, vocab, w, mode, ldo=vocab + 2)
    _check(out, bufs, vocab, w, mode, what=f"bad rows {mode}")
    assert np.isnan(out[[0, 2, 4], :vocab]).all() and np.isfinite(out[[1, 3], :vocab]).all()


def test_entry_rejects_bad_arguments():
    """Every FPNMT_E_ARG / FPNMT_E_UNSUPPORTED case of include/fpnmt.h; the
    output keeps its sentinel (nothing was launched)."""
    from fpnmt import _lib as L
    vocab, rows = 64, 2
    bufs = _bufs(2, rows, vocab, [vocab, vocab], 110)
    w = [0.5, 0.5]
    nine = [bufs[0]] * 9

    def bad(code, word, b=bufs, wts=w, mode="prob", **kw):
        out = _launch(b, kw.pop("vocab", vocab), wts, mode, expect=code, **kw)
        assert word in L.lib.fpnmt_last_error(), (word, L.lib.fpnmt_last_error())
        assert (out == SENT).all() or kw.get("inplace")

    for k in ("logits", "ldl", "weight", "out"):
        bad(L.E_ARG, b"null", null=(k,))
    bad(L.E_ARG, b"rows", rows=0)
    bad(L.E_ARG, b"vocab", vocab=0, ldo=vocab)
    bad(L.E_ARG, b"n_models", n_models=0)
    bad(L.E_ARG, b"ldl", ldl=[vocab, vocab - 1])
    bad(L.E_ARG, b"ldo", ldo=vocab - 1, out=np.full((rows, vocab), SENT, dtype=np.float32))
    for x in (0.0, -0.5, float("nan"), float("inf")):
        bad(L.E_ARG, b"weight", wts=[0.5, x])
    for m in (2, -1):
        bad(L.E_ARG, b"mode", mode=m)
    bad(L.E_UNSUPPORTED, b"more than 8", b=nine, wts=[1.0 / 9] * 9)
    # out may be logits[0] and nothing else: the second model's buffer as the first's too, then in place
    same = [bufs[0], bufs[0]]
    keep = bufs[0].copy()
    out = _launch(same, vocab, w, "prob", inplace=True, expect=L.E_ARG)
    assert b"overlaps" in L.lib.fpnmt_last_error() and out.tobytes() == keep.tobytes()
    # a null entry in the pointer table
    from fpnmt._lib import lib
    o = torch.full((rows, vocab), float(SENT), device=DEV)
    d0 = torch.from_numpy(bufs[0]).to(DEV)
    rc = lib.fpnmt_logits_ensemble(rows, vocab, 2, (C.c_void_p * 2)(d0.data_ptr(), None), (C.c_longlong * 2)(vocab, vocab),
                                   (C.c_float * 2)(*w), 0, None, o.data_ptr(), vocab, L.stream_ptr())
    assert rc == L.E_ARG and b"null" in lib.fpnmt_last_error()
    # out inside the second model's buffer
    d1 = torch.from_numpy(np.concatenate([bufs[1], bufs[1]])).to(DEV)
    rc = lib.fpnmt_logits_ensemble(rows, vocab, 2, (C.c_void_p * 2)(d0.data_ptr(), d1.data_ptr()),
                                   (C.c_longlong * 2)(vocab, vocab), (C.c_float * 2)(*w), 0, None,
                                   d1.data_ptr() + 4 * vocab, vocab, L.stream_ptr())
    assert rc == L.E_ARG and b"overlaps" in lib.fpnmt_last_error()
    # out shifted inside logits[0]: not "the same buffer"
    d2 = torch.from_numpy(np.concatenate([bufs[0], bufs[0]])).to(DEV)
    rc = lib.fpnmt_logits_ensemble(rows, vocab, 2, (C.c_void_p * 2)(d2.data_ptr(), d0.data_ptr()),
                                   (C.c_longlong * 2)(vocab, vocab), (C.c_float * 2)(*w), 0, None,
                                   d2.data_ptr() + 4 * vocab, vocab, L.stream_ptr())
    assert rc == L.E_ARG and b"overlaps" in lib.fpnmt_last_error()
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == SENT).all()
    # the largest supported ensemble runs
    eight = _bufs(8, 1, vocab, [vocab] * 8, 111)
    _check(_launch(eight, vocab, [0.125] * 8, "prob"), eight, vocab, [0.125] * 8, "prob", what="8 models")

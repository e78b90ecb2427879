"""Properties of tests/ensemble_ref.py, the fp64 restatement of
fpnmt_logits_ensemble's row semantics (include/fpnmt.h), so that the yardstick
of the kernel tests is pinned by itself and does not rest on the kernel."""
import math
import os
import re

import numpy as np
import pytest

from ensemble_ref import ensemble_row, logsumexp, normalise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -np.inf


def _rows(n_models, vocab, seed, scale=4.0):
    g = np.random.default_rng(seed)
    return [g.normal(0.0, scale, vocab) for _ in range(n_models)]


def _log_softmax(l):
    return np.asarray(l, dtype=np.float64) - logsumexp(l)


@pytest.mark.parametrize("n_models,weights", [(1, None), (2, None), (3, (3.0, 2.0, 1.0)), (8, None)])
def test_prob_rows_are_normalised(n_models, weights):
    """The mixture of distributions is a distribution: logsumexp == 0 to
    fp64 rounding, also at logits where a naive exp overflows."""
    for scale in (4.0, 300.0):
        out = ensemble_row(_rows(n_models, 257, 1, scale), normalise(weights, n_models), "prob")
        assert abs(logsumexp(out)) < 1e-12


@pytest.mark.parametrize("mode", ["prob", "logprob"])
@pytest.mark.parametrize("n_models", [1, 2, 5])
def test_identical_rows_give_log_softmax(mode, n_models):
    l = _rows(1, 100, 2)[0]
    w = normalise([1.0 + m for m in range(n_models)], n_models)
    out = ensemble_row([l] * n_models, w, mode)
    assert np.max(np.abs(out - _log_softmax(l))) < 1e-12


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_small_second_weight_tends_to_the_first_model(mode):
    a, b = _rows(2, 64, 3, scale=1.0)  # p_b / p_a stays below e^8, so eps = 1e-8 leaves at most ~3e-5
    errs = []
    for eps in (1e-2, 1e-5, 1e-8):
        out = ensemble_row([a, b], normalise([1.0, eps], 2), mode)
        errs.append(np.max(np.abs(out - _log_softmax(a))))
    assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-4, errs


def test_minus_inf_rules():
    a, b = _rows(2, 16, 4)
    a[3] = NEG           # one model only
    a[5] = b[5] = NEG    # every model
    w = normalise(None, 2)
    prob, logp = ensemble_row([a, b], w, "prob"), ensemble_row([a, b], w, "logprob")
    # "prob" leaves the model out of the column: log(w_b * softmax(b)[3])
    assert prob[3] == pytest.approx(math.log(0.5) + b[3] - logsumexp(b), abs=1e-12)
    assert prob[5] == NEG and logp[3] == NEG and logp[5] == NEG
    assert not np.isnan(prob).any() and not np.isnan(logp).any()
    keep = [j for j in range(16) if j not in (3, 5)]
    assert np.isfinite(prob[keep]).all() and np.isfinite(logp[keep]).all()
    assert abs(logsumexp(prob)) < 1e-12
    # one model with a single finite column: still a good row
    b = _rows(2, 16, 4)[1]
    c = np.full(16, NEG)
    c[7] = 1.5
    prob = ensemble_row([c, b], w, "prob")
    logp = ensemble_row([c, b], w, "logprob")
    assert np.isfinite(prob).all() and abs(logsumexp(prob)) < 1e-12
    assert [j for j in range(16) if logp[j] != NEG] == [7]
    assert logp[7] == pytest.approx(0.5 * 0.0 + 0.5 * (b[7] - logsumexp(b)), abs=1e-12)


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_bad_rows_are_nan_throughout(mode):
    a, b = _rows(2, 16, 5)
    w = normalise(None, 2)
    for bad in (np.nan, np.inf):
        x = a.copy()
        x[2] = bad
        assert np.isnan(ensemble_row([b, x], w, mode)).all()
    assert np.isnan(ensemble_row([b, np.full(16, NEG)], w, mode)).all()


def test_prob_of_two_one_hot_like_rows_is_their_mixture():
    """Two rows that put (almost) all mass on different tokens: the "prob"
    mixture puts w_0 on the one and w_1 on the other; the geometric mean
    does not."""
    vocab = 10
    a, b = np.full(vocab, -60.0), np.full(vocab, -60.0)
    a[2], b[7] = 0.0, 0.0
    w = normalise([3.0, 1.0], 2)
    p = np.exp(ensemble_row([a, b], w, "prob"))
    assert p[2] == pytest.approx(0.75, abs=1e-9) and p[7] == pytest.approx(0.25, abs=1e-9)
    assert p.sum() == pytest.approx(1.0, abs=1e-12)
    q = ensemble_row([a, b], w, "logprob")
    q = np.exp(q - logsumexp(q))
    assert q[2] == pytest.approx(1.0, abs=1e-6) and q[7] < 1e-12  # exp(-60 * 0.75) vs exp(-60 * 0.25)


def test_weights_are_used_as_given():
    """No renormalisation inside: doubling both weights adds log 2 to a
    "prob" row and doubles a "logprob" row."""
    rows = _rows(2, 32, 6)
    for mode, f in (("prob", lambda x: x + math.log(2.0)), ("logprob", lambda x: 2.0 * x)):
        base = ensemble_row(rows, [0.25, 0.75], mode)
        assert np.max(np.abs(ensemble_row(rows, [0.5, 1.5], mode) - f(base))) < 1e-12


def test_normalise():
    assert normalise(None, 4) == [0.25] * 4
    assert normalise([2, 1, 1], 3) == [0.5, 0.25, 0.25]


def test_header_and_binding_agree_on_the_entry():
    from fpnmt import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fpnmt.h")).read()
    assert int(re.search(r"#define FPNMT_ENSEMBLE_MAX\s+(\d+)", hdr).group(1)) == L.ENSEMBLE_MAX
    assert len(L.SIGNATURES["fpnmt_logits_ensemble"]) == 11
    assert L.lib.fpnmt_logits_ensemble is not None


def test_decoder_weight_normalisation_names_bad_values():
    from fpnmt.decode import ensemble_weights_normalised
    assert ensemble_weights_normalised(2, None) == (0.5, 0.5)
    assert ensemble_weights_normalised(3, [2, 1, 1]) == (0.5, 0.25, 0.25)
    for bad, word in (([1.0], "1 weights"), ([1.0, 0.0], "0.0"), ([1.0, -2.0], "-2.0"), ([1.0, float("nan")], "nan"),
                      ([1.0, float("inf")], "inf"), ("ab", "ab")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ensemble_weights_normalised(2, bad)

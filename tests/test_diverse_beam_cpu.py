"""Diverse beam search without a GPU: the torch restatement of the rule
(tests/diverse_beam_ref.py, the reference of the GPU tests) checked against
the properties the rule implies, and the decoder's argument validation."""
import math

import pytest
import torch

from diverse_beam_ref import NEG, groups_step_ref, plain_step_ref

END = 3


def _case(K, V, seed, shared=False):
    g = torch.Generator().manual_seed(seed)
    logits = (2 * torch.randn(1, V, generator=g)).repeat(K, 1) if shared else torch.randn(K, V, generator=g)
    score = torch.zeros(K) if shared else -0.1 * torch.rand(K, generator=g)
    return logits, score, torch.full((K,), 5, dtype=torch.int32), torch.zeros(K, dtype=torch.int32)


@pytest.mark.parametrize("lam", [0.0, 3.0])
def test_one_group_is_the_plain_step(lam):
    K, V, t = 6, 50, 5
    logits, score, blen, fin = _case(K, V, 1)
    fin[4], score[4], blen[4] = 1, 0.5, 2  # a finished row that leads
    a = groups_step_ref(logits, score, blen, fin, t, END, K, 1, lam)
    b = plain_step_ref(logits, score, blen, fin, t, END, K)
    for k in ("par", "tok", "score", "blen", "fin"):
        assert torch.equal(a[k], b[k]), k
    assert int(a["par"][0]) == 4 and int(a["fin"][0]) == 1 and int(a["blen"][0]) == 2


def test_zero_penalty_gives_identical_groups():
    """The same row and score in every group, lam = 0: every group makes the
    same choice, from its own rows."""
    K, G, V, t = 8, 4, 40, 5
    Kg = K // G
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(Kg, V, generator=g).repeat(G, 1)
    score = (-0.1 * torch.rand(Kg, generator=g)).repeat(G)
    o = groups_step_ref(logits, score, torch.full((K,), t, dtype=torch.int32), torch.zeros(K, dtype=torch.int32), t,
                        END, K, G, 0.0)
    for grp in range(1, G):
        rows = slice(grp * Kg, (grp + 1) * Kg)
        assert torch.equal(o["tok"][rows], o["tok"][:Kg])
        assert torch.equal(o["score"][rows], o["score"][:Kg])
        assert torch.equal(o["par"][rows] - grp * Kg, o["par"][:Kg])
    # and each group alone is a plain step over its rows
    p = plain_step_ref(logits[:Kg], score[:Kg], torch.full((Kg,), t, dtype=torch.int32),
                       torch.zeros(Kg, dtype=torch.int32), t, END, Kg)
    assert torch.equal(p["tok"], o["tok"][:Kg]) and torch.equal(p["score"], o["score"][:Kg])


def test_large_penalty_makes_single_beam_groups_differ():
    K, V, t = 8, 60, 5
    logits, score, blen, fin = _case(K, V, 3, shared=True)
    o = groups_step_ref(logits, score, blen, fin, t, END, K, K, 1e4)
    assert len(set(o["tok"].tolist())) == K
    # the tokens are the row's K best, in order; the scores carry no penalty
    best = torch.sort(logits[0], descending=True, stable=True).indices[:K]
    assert o["tok"].tolist() == best.tolist()
    assert torch.equal(o["score"], torch.log_softmax(logits[0], -1)[best])
    assert o["cnt"] == {int(j): 1 for j in best}
    # without the penalty every group takes the best token
    z = groups_step_ref(logits, score, blen, fin, t, END, K, K, 0.0)
    assert z["tok"].tolist() == [int(best[0])] * K


def test_finished_row_is_neither_penalised_nor_counted():
    """Group 0: one live row that takes <end>, one finished row that carries
    itself. Group 1: a finished row at the same score as group 0's, kept
    whatever lam is, and a live row whose <end> candidate is penalised once
    (the live child), not twice (the carry)."""
    K, G, V, t, lam = 4, 2, 30, 5, 2.0
    logits = torch.zeros(K, V)
    logits[0, END] = 20.0  # group 0's live row ends
    logits[3, END] = 1.0   # group 1's live row would end too
    logits[3, 9] = 0.5
    score = torch.tensor([-1.0, -0.5, -0.5, -1.0])
    blen = torch.tensor([5, 2, 2, 5], dtype=torch.int32)
    fin = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    o = groups_step_ref(logits, score, blen, fin, t, END, K, G, lam)
    assert o["par"].tolist()[:2] == [1, 0] and o["tok"].tolist()[:2] == [END, END]
    assert o["cnt"].get(END) == 1  # the live child only
    # group 1: the carry leads at its own score; the live row's <end> lost lam, so token 9 wins
    assert o["par"].tolist()[2:] == [2, 3] and o["tok"].tolist()[2:] == [END, 9]
    assert float(o["score"][2]) == -0.5 and int(o["blen"][2]) == 2 and int(o["fin"][2]) == 1
    lp = torch.log_softmax(logits[3], -1)
    assert float(o["score"][3]) == float(score[3] + lp[9])
    assert float(lp[END] - lam) < float(lp[9]) < float(lp[END])


def test_count_is_once_per_live_child():
    """Two live rows of group 0 take the same token: group 1 sees cnt 2."""
    K, G, V, t, lam = 4, 2, 30, 5, 0.15
    logits = torch.zeros(K, V)
    logits[:, 7] = 3.0
    logits[:, 8] = 2.8
    logits[:, 9] = 2.3
    score = torch.tensor([0.0, 0.0, 0.0, NEG])
    blen = torch.full((K,), t, dtype=torch.int32)
    fin = torch.zeros(K, dtype=torch.int32)
    o = groups_step_ref(logits, score, blen, fin, t, END, K, G, lam)
    assert o["tok"].tolist()[:2] == [7, 7] and o["par"].tolist()[:2] == [0, 1]
    assert o["cnt"] == {7: 3, 8: 1}  # after group 1 took 8 and 7 as well
    # token 7 at 3.0 - 2 * 0.15 = 2.7 falls behind 8 at 2.8; counted once it would lead at 2.85
    assert o["par"].tolist()[2:] == [2, 2] and o["tok"].tolist()[2:] == [8, 7]
    lp = torch.log_softmax(logits[2], -1)
    assert torch.equal(o["score"][2:], torch.stack([lp[8], lp[7]]))  # unpenalised
    # one live row in group 0: it takes 7 and 8 once each, and 7 at 2.85 leads 8 at 2.65 in group 1
    once = groups_step_ref(logits, torch.tensor([0.0, NEG, 0.0, NEG]), blen, fin, t, END, K, G, lam)
    assert once["cnt"] == {7: 2, 8: 2} and once["tok"].tolist() == [7, 8, 7, 8]


def test_validation():
    from fpnmt.decode import beam_groups_validated as v
    assert v("beam", 8) == (1, 0.0)
    assert v("reference", 8) == (1, 0.0)
    assert v("beam", 8, 4, 0.5) == (4, 0.5)
    assert v("beam", 8, 8, 0) == (8, 0.0)
    for groups in (0, 3, -2, 16, 2.0, True):
        with pytest.raises(ValueError):
            v("beam", 8, groups, 0.0)
    for lam in (-0.5, math.nan, math.inf, -math.inf, "x"):
        with pytest.raises(ValueError):
            v("beam", 8, 4, lam)
    with pytest.raises(ValueError):
        v("beam", 8, 1, 0.5)
    with pytest.raises(ValueError):
        v("reference", 8, 4, 0.0)
    with pytest.raises(ValueError):
        v("reference", 8, 4, 0.5)

"""The row semantics of fpnmt_logits_ensemble (include/fpnmt.h) in numpy fp64,
the reference the kernel and decoder tests compare against, and a literal CPU
ensemble beam search on the oracle's models. Nothing here is clever on
purpose; tests/test_ensemble_cpu.py pins it by its properties so that it does
not rest on the kernel."""
import math

import numpy as np

MODES = {"prob": 0, "logprob": 1}


def normalise(weights, n_models):
    """The host's part: None -> equal weights; else the weights over their
    fp64 sum."""
    if weights is None:
        return [1.0 / n_models] * n_models
    w = [float(x) for x in weights]
    assert len(w) == n_models
    total = math.fsum(w)
    return [x / total for x in w]


def logsumexp(x):
    """fp64 logsumexp of a 1-d array; -inf for an all -inf one."""
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x)
    if not np.isfinite(m):
        return m
    return m + np.log(np.sum(np.exp(x - m)))


def row_is_bad(rows):
    """A model's row with a NaN or +inf, or -inf in all columns."""
    for l in rows:
        l = np.asarray(l, dtype=np.float64)
        if np.isnan(l).any() or np.isposinf(l).any() or np.isneginf(l).all():
            return True
    return False


def ensemble_row(rows, weights, mode):
    """rows: the M models' logits rows (vocab,) each; weights: M positive
    numbers used AS GIVEN (no renormalisation, as in the kernel); mode "prob"
    or "logprob". Returns the combined row in fp64."""
    assert mode in MODES
    ls = [np.asarray(l, dtype=np.float64) for l in rows]
    vocab = ls[0].shape[0]
    if row_is_bad(ls):
        return np.full(vocab, np.nan)
    # a good row has no NaN / +inf and a finite logsumexp, so l - lse is finite or -inf
    a = np.stack([l - logsumexp(l) for l in ls])  # (M, vocab) log-probabilities
    w = np.asarray([float(x) for x in weights], dtype=np.float64)[:, None]
    if mode == "logprob":
        return np.sum(w * a, axis=0)  # w > 0: -inf where any model has -inf, never a NaN
    terms = a + np.log(w)  # a model with -inf weighs exp(-inf) = 0 in the column's logsumexp
    mx = np.max(terms, axis=0)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(mx), safe + np.log(np.sum(np.exp(terms - safe), axis=0)), -np.inf)


def ensemble_rows(logits, weights, mode, fin=None):
    """logits: M arrays (rows, vocab). Returns (rows, vocab) fp64; a row with
    fin[r] != 0 is NaN-free garbage the caller must not look at (None)."""
    n = logits[0].shape[0]
    out = [None] * n
    for r in range(n):
        if fin is not None and fin[r]:
            continue
        out[r] = ensemble_row([l[r] for l in logits], weights, mode)
    return out


# ------------------------------------------------------------- CPU searches
def combined_log_probs(members, image, seqs, weights, mode, constrain=None):
    """log_softmax of the combined row of every prefix in seqs. members: a
    list of dicts with the oracle's sd, cfg and encs (encoder output per
    image); weights normalised. constrain(row_f32, seq) -> row, applied to
    the combined row (the device constrains the fp32 row it combined)."""
    import torch
    from test_gpu_beam_search import _cpu_logits
    per_model = [_cpu_logits(m["sd"], m["cfg"], m["encs"][image], seqs).double().numpy() for m in members]
    rows = []
    for n in range(len(seqs)):
        row = ensemble_row([l[n] for l in per_model], weights, mode)
        if constrain is not None:
            row = constrain(row.astype(np.float32), seqs[n]).astype(np.float64)
        rows.append(row)
    return torch.log_softmax(torch.from_numpy(np.stack(rows)), -1).float()


def cpu_ensemble_beam_search(members, image, T, K, start, end, weights, mode, constrain=None):
    """cpu_beam_search of test_gpu_beam_search.py with its per-step
    log_softmax(_cpu_logits(...)) replaced by combined_log_probs; nothing
    else differs. constrain(row_f32, seq, t) -> row (None: unconstrained)."""
    import torch
    NEG = float("-inf")
    V = members[0]["sd"]["final_layer.kernel"].shape[1]
    seqs = [[start] for _ in range(K)]
    score = torch.full((K,), NEG)
    score[0] = 0.0
    blen = torch.zeros(K, dtype=torch.int64)
    fin = torch.zeros(K, dtype=torch.bool)
    margin = math.inf
    for t in range(T):
        if bool(fin.all()):
            break
        cand = torch.full((K, V), NEG)
        live = [b for b in range(K) if not fin[b] and score[b] > NEG]
        con = None if constrain is None else (lambda row, seq, t=t: constrain(row, seq, t))
        lp = combined_log_probs(members, image, [seqs[b] for b in live], weights, mode, con)
        for n, b in enumerate(live):
            cand[b] = score[b] + lp[n]
        for b in range(K):
            if fin[b]:
                cand[b, end] = score[b]
        vals, idx = torch.sort(cand.reshape(-1), descending=True, stable=True)
        margin = min(margin, float(vals[K - 1] - vals[K]))
        par, tok = (idx[:K] // V).tolist(), (idx[:K] % V).tolist()
        seqs = [seqs[p] + [k] for p, k in zip(par, tok)]
        nfin = torch.tensor([bool(fin[p]) or k == end for p, k in zip(par, tok)])
        blen = torch.tensor([int(blen[p]) if fin[p] else t + 1 for p in par])
        score, fin = vals[:K].clone(), nfin
    return seqs, score, blen, fin, margin


def cpu_ensemble_greedy(members, image, T, start, end, weights, mode):
    """Arg-max decode from the combined distribution (ties to the lower id)."""
    import torch
    seq = [start]
    for _ in range(T):
        seq.append(int(torch.argmax(combined_log_probs(members, image, [seq], weights, mode)[0])))
        if seq[-1] == end:
            return seq[1:-1]
    return seq[1:]


def cpu_sequence_logp(members, image, ids, ended, start, end, weights, mode):
    """Teacher-forced log-probability of ids (+ <end> when ended) under the
    combined distribution, and the number of tokens scored."""
    toks = list(ids) + ([end] if ended else [])
    seq, total = [start], 0.0
    for k in toks:
        total += float(combined_log_probs(members, image, [seq], weights, mode)[0][k])
        seq.append(k)
    return total, len(toks)

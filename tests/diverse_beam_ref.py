"""Diverse beam search restated in torch on the CPU, for the tests of
fpnmt_beam_step_groups and BeamDecoder(beam_groups=G): one step of the rule
(`groups_step_ref`), a plain top-K step to compare it with (`plain_step_ref`),
and a literal search on the oracle's model that recomputes every prefix with
no cache (`cpu_diverse_beam_search`).

The rule, per image and position: the K rows are G groups of Kg = K / G
contiguous rows, ranked in group order. A live row b offers token j at
(score[b] + log_softmax(logits[b])[j]) - lam * cnt[j]; a finished row offers
itself once at b*V + <end>, unpenalised; a row at -inf offers nothing. Only a
group's own rows compete for its Kg rows (larger value first, then the lower
flat index b*V + j). A live child that took j does cnt[j] += 1 for the groups
after it. The carried score is the unpenalised value."""
import math

import torch

NEG = float("-inf")
NONE = -1  # a slot that found no candidate


def _select(vals, flat, n):
    """The n best (value desc, lower flat index first) of the candidates that
    can be offered (NaN never is); `flat` ascends, so a stable sort does it."""
    ok = ~torch.isnan(vals)
    vals, flat = vals[ok], flat[ok]
    v, order = torch.sort(vals, descending=True, stable=True)
    return v, flat[order][:n]


def groups_step_ref(logits, score, blen, fin, t, end, K, G, lam):
    """One image, one position. Returns a dict: par / tok / score / blen / fin
    per new row (par NONE: the empty slot, which carries its own row as a
    finished beam at -inf), `sorted`: per group the penalised candidate
    values in rank order, `cnt`: {token: count} after the last group."""
    V = logits.shape[1]
    Kg = K // G
    lam32 = torch.tensor(lam, dtype=torch.float32)
    base = score[:, None] + torch.log_softmax(logits.float(), -1)  # unpenalised, fp32
    live = (fin == 0) & (score > NEG)
    cnt = torch.zeros(V, dtype=torch.float32)
    par, tok, nscore, nlen, nfin, ranked = [], [], [], [], [], []
    for g in range(G):
        vals, flat = [], []
        for b in range(g * Kg, (g + 1) * Kg):
            if live[b]:
                vals.append(base[b] - lam32 * cnt)  # fp32 product, then the subtraction
                flat.append(b * V + torch.arange(V))
            elif fin[b]:
                vals.append(score[b:b + 1].clone())
                flat.append(torch.tensor([b * V + end]))
        if vals:
            v, chosen = _select(torch.cat(vals), torch.cat(flat), Kg)
        else:
            v, chosen = torch.empty(0), torch.empty(0, dtype=torch.int64)
        ranked.append(v)
        for k in range(Kg):
            r = g * Kg + k
            if k >= len(chosen):
                par.append(NONE), tok.append(end), nscore.append(NEG), nlen.append(int(blen[r])), nfin.append(1)
                continue
            p, j = int(chosen[k]) // V, int(chosen[k]) % V
            par.append(p), tok.append(j)
            if fin[p]:
                nscore.append(float(score[p])), nlen.append(int(blen[p])), nfin.append(1)
            else:
                nscore.append(float(base[p, j])), nlen.append(t + 1), nfin.append(int(j == end))
                cnt[j] += 1
    return dict(par=torch.tensor(par), tok=torch.tensor(tok, dtype=torch.int32),
                score=torch.tensor(nscore, dtype=torch.float32), blen=torch.tensor(nlen, dtype=torch.int32),
                fin=torch.tensor(nfin, dtype=torch.int32), sorted=ranked,
                cnt={int(j): int(cnt[j]) for j in torch.nonzero(cnt).flatten()})


def plain_step_ref(logits, score, blen, fin, t, end, K):
    """The plain beam step (fpnmt_beam_step_log's rule): the K best of all
    rows' candidates. The same keys as groups_step_ref."""
    V = logits.shape[1]
    base = score[:, None] + torch.log_softmax(logits.float(), -1)
    live = (fin == 0) & (score > NEG)
    vals, flat = [], []
    for b in range(K):
        if live[b]:
            vals.append(base[b]), flat.append(b * V + torch.arange(V))
        elif fin[b]:
            vals.append(score[b:b + 1].clone()), flat.append(torch.tensor([b * V + end]))
    v, chosen = _select(torch.cat(vals), torch.cat(flat), K)
    par, tok = chosen // V, chosen % V
    pfin = fin[par].bool()
    return dict(par=par, tok=tok.to(torch.int32), score=v[:K].clone(),
                blen=torch.where(pfin, blen[par], torch.full_like(blen[par], t + 1)),
                fin=(pfin | (tok == end)).to(torch.int32), sorted=[v])


def cut_gaps(ranked, Kg):
    """Per group the differences of neighbours among its first Kg + 1
    candidates, concatenated (a tie is 0; -inf next to -inf is dropped)."""
    out = []
    for v in ranked:
        v = v[:Kg + 1].double()
        d = v[:-1] - v[1:]
        out.append(d[~torch.isnan(d)])
    return torch.cat(out) if out else torch.empty(0, dtype=torch.float64)


def assert_clear(ranked, Kg, gap):
    """Every neighbouring pair at a cut is exactly equal (a constructed tie,
    which the index decides) or more than `gap` apart."""
    d = cut_gaps(ranked, Kg)
    assert bool(((d == 0) | (d > gap)).all()), d


# ------------------------------------------------------------ whole search
def _cpu_logits(sd, cfg, enc, seqs):
    from oracle import ref_cpu as R
    tar = torch.tensor(seqs, dtype=torch.int64)
    logits, _ = R.transformer(sd, enc.repeat(len(seqs), 1, 1), tar, False, R.create_look_ahead_mask(tar.shape[1]), cfg)
    return logits[:, -1, :]


def cpu_diverse_beam_search(sd, cfg, enc, T, K, G, lam, start, end):
    """The rule, literally: every position re-runs the decoder on the live
    beams' whole prefixes. Returns (seqs, score, len, fin) per beam and the
    smallest gap between a group's Kg-th and (Kg+1)-th candidate met on the
    way."""
    V = sd["final_layer.kernel"].shape[1]
    Kg = K // G
    seqs = [[start] for _ in range(K)]
    score = torch.full((K,), NEG)
    score[::Kg] = 0.0
    blen = torch.zeros(K, dtype=torch.int32)
    fin = torch.zeros(K, dtype=torch.int32)
    margin = math.inf
    for t in range(T):
        if bool(fin.all()):
            break
        live = [b for b in range(K) if not fin[b] and score[b] > NEG]
        logits = torch.zeros(K, V)
        logits[live] = _cpu_logits(sd, cfg, enc, [seqs[b] for b in live]).float()
        o = groups_step_ref(logits, score, blen, fin, t, end, K, G, lam)
        for v in o["sorted"]:
            if len(v) > Kg:
                margin = min(margin, float(v[Kg - 1] - v[Kg]))
        seqs = [seqs[p if p != NONE else r] + [j] for r, (p, j) in enumerate(zip(o["par"].tolist(), o["tok"].tolist()))]
        score, blen, fin = o["score"], o["blen"], o["fin"]
    return seqs, score, blen, fin, margin


def cpu_rank(seqs, score, blen, fin, alpha, rows):
    """[(ids, key, len)] of the beams `rows`, best first by score /
    len^alpha (ties to the lower row), and the smallest gap between keys."""
    rows = list(rows)
    key = score[rows].double() / blen[rows].clamp(min=1).double() ** alpha
    vals, order = torch.sort(key, descending=True, stable=True)
    gap = float((vals[:-1] - vals[1:]).min()) if len(vals) > 1 else math.inf
    out = []
    for o in order.tolist():
        b = rows[o]
        n = int(blen[b]) - int(fin[b])
        out.append((seqs[b][1:1 + n], float(key[o]), int(blen[b])))
    return out, gap

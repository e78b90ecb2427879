"""Sampled decoding (fpnmt_sample_step / fpnmt_sample_uniform, SampleDecoder,
predict_batch(mode="sample")): the uniforms against a Python-integer
restatement of the counter hash, the step against the rule restated in fp64,
ties and edge rows, determinism and graph replay, the whole decoder against
the CPU oracle step by step, and the error codes of the two entry points."""
import math

import numpy as np
import pytest
import torch

from test_gpu_beam_search import C_CFG, _cpu_logits, _pipeline

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = float("-inf")
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


# ------------------------------------------------------------ restatements
def hash_u32(seed, i):
    """csrc/common.h hash_u32 with Python integers (64-bit wrap-around)."""
    z = (seed * GOLD + i * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 8) & 0xFFFFFFFF


def draw_key(seed, seed_dev=None):
    return (seed + (0 if seed_dev is None else (seed_dev & M64) * GOLD)) & M64


def uniform(key, r, t):
    return (hash_u32(key, (r << 16) | t) & 0xFFFFFF) * 2.0 ** -24


def rule_ref(row, temperature, top_k, top_p):
    """The rule for one live row in fp64: (weights, kept mask, and the
    cumulative masses / W_k of the top-k survivors in weight order)."""
    l = row.double()
    V = l.numel()
    w = torch.exp((l - l.max()) / temperature)
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        keep = l >= torch.sort(l, descending=True).values[top_k - 1]
    order = torch.argsort(torch.where(keep, l, torch.full_like(l, NEG)), descending=True, stable=True)[:int(keep.sum())]
    cum = torch.cumsum(w[order], 0)
    if top_p < 1.0:
        n = int(torch.nonzero(cum >= top_p * cum[-1])[0])
        keep = keep & (l >= l[order[n]])
    return w, keep, cum / cum[-1]


def pick_p(rows, temperature, top_k, near=0.9):
    """top_p for a case: the midpoint of a gap between two consecutive
    cumulative masses of rows[0] (the shared row) wider than 2e-4 of the
    total, the one nearest `near` at which every other row of the case is
    also more than 1e-4 from each of its cumulative masses, so no row's
    kept set is a matter of summation order."""
    cums = [rule_ref(r, temperature, top_k, 1.0)[2].numpy() for r in rows]
    c0 = np.concatenate([[0.0], cums[0]])
    gaps = np.nonzero(np.diff(c0) > 2e-4)[0]
    mids = sorted(((c0[g] + c0[g + 1]) / 2 for g in gaps), key=lambda m: abs(m - near))
    for m in mids:
        p = float(np.float32(m))
        if not 0.0 < p < 1.0:
            continue
        ok = True
        for c in cums:
            i = np.searchsorted(c, p)
            near_mass = min(abs(c[min(i, len(c) - 1)] - p), abs(c[max(i - 1, 0)] - p))
            ok = ok and near_mass > 1e-4
        if ok:
            return p
    raise AssertionError("no top_p clear of every row's cumulative masses")


def launch(logits, V, t, T, end, temperature, top_k, top_p, seed, state, seed_dev=None, ldl=None, want_kept=True):
    """fpnmt_sample_step on device copies of `state`; returns the outputs on the CPU."""
    from fpnmt import _lib as L
    R = logits.shape[0]
    d = {k: v.clone().to(DEV) for k, v in state.items()}
    lg = logits.to(DEV)
    tok = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    sd = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, device=DEV)
    L.call("fpnmt_sample_step", R, V, lg.data_ptr(), ldl or lg.stride(0), temperature, top_k, top_p, seed,
           L.ptr(sd), d["score"].data_ptr(), d["slen"].data_ptr(), d["fin"].data_ptr(), d["hist"].data_ptr(), T + 1, t,
           end, tok.data_ptr(), kept.data_ptr() if want_kept else None, L.stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    out["tok"], out["kept"] = tok.cpu(), kept.cpu()
    return out


def make_state(R, V, t, T, g):
    return dict(score=-torch.rand(R, generator=g), slen=torch.full((R,), t, dtype=torch.int32),
                fin=torch.zeros(R, dtype=torch.int32),
                hist=torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32))


# ---------------------------------------------------------------- uniforms
def test_sample_uniform_matches_python_hash():
    from fpnmt import _lib as L
    rows = 300
    for seed in (0, 0xDEADBEEFCAFEF00D):
        for seed_dev in (None, 5, -3):
            sd = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, device=DEV)
            for t in (0, 1, 31, 65535):
                u = torch.full((rows,), -1.0, device=DEV)
                L.call("fpnmt_sample_uniform", rows, t, seed, L.ptr(sd), u.data_ptr(), L.stream_ptr())
                torch.cuda.synchronize()
                key = draw_key(seed, seed_dev)
                ref = torch.tensor([uniform(key, r, t) for r in range(rows)], dtype=torch.float32)
                assert torch.equal(u.cpu(), ref), (seed, seed_dev, t)
                assert float(ref.min()) >= 0.0 and float(ref.max()) < 1.0


# ------------------------------------------------------ step against fp64
VOCABS = [37, 200, 1001, 10000, 16384]  # scalar < threads; ldl 208; unaligned; vector path; the LDS limit
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, "p"), (1.0, 5, "p"), (1.0, 1, 1.0), (1.0, "V+3", 1.0)]
_CASE = {}


def _case_logits(V):
    """96 rows: 64 copies of one row (many u over one distribution), 32 distinct; randn * 3."""
    if V not in _CASE:
        g = torch.Generator().manual_seed(1000 + V)
        ldl = 208 if V == 200 else V
        buf = torch.zeros(96, ldl)
        buf[:, :V] = torch.randn(96, V, generator=g) * 3
        buf[:64, :V] = buf[0, :V]
        buf[:, V:] = 99.0  # padding a correct kernel never reads
        _CASE[V] = (buf, ldl, make_state(96, V, 5, 12, g))
    return _CASE[V]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"T{s[0]}-k{s[1]}-p{s[2]}")
@pytest.mark.parametrize("V", VOCABS)
def test_sample_step_matches_fp64_rule(V, setting):
    temperature, top_k, top_p = setting
    top_k = V + 3 if top_k == "V+3" else top_k
    buf, ldl, state = _case_logits(V)
    R, t, T, end, seed = 96, 5, 12, 3, 77 + V
    distinct = [buf[r, :V] for r in [0] + list(range(64, 96))]
    if top_p == "p":
        top_p = pick_p(distinct, temperature, top_k)
    refs = {}
    for r in [0] + list(range(64, 96)):
        w, keep, cum = rule_ref(buf[r, :V], temperature, top_k, top_p)
        if top_p < 1.0:  # the kept set is not a matter of summation order
            assert float((cum - top_p).abs().min()) > 1e-4, (r, top_p)
        refs[r] = (w, keep)
    out = launch(buf, V, t, T, end, temperature, top_k, top_p, seed, state, ldl=ldl)
    tol = V * 2.0 ** -24
    key = draw_key(seed)
    exact = 0
    for r in range(R):
        w, keep = refs[0 if r < 64 else r]
        tok = int(out["tok"][r])
        assert int(out["kept"][r]) == int(keep.sum()), (r, int(out["kept"][r]), int(keep.sum()))
        assert 0 <= tok < V and bool(keep[tok]) and float(w[tok]) > 0, (r, tok)
        c = torch.cumsum(w * keep, 0)
        W = float(c[-1])
        u = uniform(key, r, t)
        lo, hi = float(c[tok] - w[tok]) / W, float(c[tok]) / W
        assert lo - tol <= u < hi + tol, (r, tok, u, lo, hi)
        exact += int(torch.nonzero(c > u * W)[0]) == tok
        lp = torch.log_softmax(buf[r, :V].double(), 0)[tok]
        want = float(state["score"][r].double() + lp)
        assert abs(float(out["score"][r]) - want) <= 1e-5 + 1e-5 * abs(want), (r, float(out["score"][r]), want)
    print(f"V {V} setting {setting} top_p {top_p}: {exact}/{R} tokens are the fp64-exact draw")
    assert torch.equal(out["hist"][:, t + 1], out["tok"])
    assert torch.equal(out["hist"][:, :t + 1], state["hist"][:, :t + 1])
    assert torch.equal(out["hist"][:, t + 2:], state["hist"][:, t + 2:])
    assert out["slen"].tolist() == [t + 1] * R
    assert torch.equal(out["fin"], (out["tok"] == end).to(torch.int32))


# ------------------------------------------------------------ ties, edges
def _tie_row(V):
    g = torch.Generator().manual_seed(5)
    row = torch.rand(V, generator=g) - 20.0  # negligible tail
    row[9] = 5.0
    for j in (2, 17, 30, 31, 60):
        row[j] = 3.0
    return row


@pytest.mark.parametrize("top_k,top_p", [(3, 1.0), (0, 0.7)], ids=["top_k", "top_p"])
def test_ties_across_the_boundary_are_all_kept(top_k, top_p):
    """1 + five bitwise-equal logits. top_k 3 cuts inside the five. top_p 0.7:
    the masses are 0.596, 0.677, 0.757, ... of the total, so the prefix ends
    at the second of the five. Either way all six are kept."""
    V, R, t, T = 64, 64, 0, 4
    row = _tie_row(V)
    w, keep, _ = rule_ref(row, 1.0, top_k, top_p)
    assert sorted(torch.nonzero(keep).flatten().tolist()) == [2, 9, 17, 30, 31, 60]
    state = make_state(R, V, t, T, torch.Generator().manual_seed(1))
    out = launch(row.repeat(R, 1), V, t, T, 3, 1.0, top_k, top_p, 11, state)
    assert out["kept"].tolist() == [6] * R
    assert set(out["tok"].tolist()) <= {2, 9, 17, 30, 31, 60}
    assert len(set(out["tok"].tolist())) > 1


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (0, 0.95), (98, 1.0)], ids=["plain", "top_p", "top_k"])
def test_minus_inf_logits_are_never_drawn(top_k, top_p):
    V, R, t, T = 100, 96, 2, 6
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(R, V, generator=g)
    dead = torch.rand(R, V, generator=g) < 0.5
    dead[:, 0] = False
    logits[dead] = NEG
    out = launch(logits, V, t, T, 3, 1.0, top_k, top_p, 4, make_state(R, V, t, T, g))
    tok = out["tok"].long()
    assert bool(torch.isfinite(logits[torch.arange(R), tok]).all())
    assert bool(torch.isfinite(out["score"]).all())
    for r in range(R):
        assert int(out["kept"][r]) == int(rule_ref(logits[r], 1.0, top_k, top_p)[1].sum()), r


@pytest.mark.parametrize("top_k", [0, 5])
def test_finished_and_undrawable_rows(top_k):
    """Row 0: finished, NaN logits -> nothing but the <end> padding. Rows 1,
    2, 3: live with all -inf, a NaN, a +inf -> the no-token path. Row 4: an
    ordinary live row beside them."""
    V, R, t, T, end = 50, 5, 3, 6, 7
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(R, V, generator=g)
    logits[0] = float("nan")
    logits[1] = NEG
    logits[2, 13] = float("nan")
    logits[3, 21] = float("inf")
    state = make_state(R, V, t, T, g)
    state["fin"][0] = 1
    state["slen"][0] = 2
    out = launch(logits, V, t, T, end, 1.0, top_k, 1.0, 9, state)
    assert float(out["score"][0]) == float(state["score"][0]) and int(out["slen"][0]) == 2 and int(out["fin"][0]) == 1
    assert out["tok"][:4].tolist() == [end] * 4 and out["hist"][:4, t + 1].tolist() == [end] * 4
    assert out["kept"][:4].tolist() == [0] * 4
    for r in (1, 2, 3):
        assert float(out["score"][r]) == NEG and int(out["fin"][r]) == 1 and int(out["slen"][r]) == t + 1
    assert math.isfinite(float(out["score"][4])) and int(out["kept"][4]) == (top_k or V)
    assert torch.equal(out["hist"][:, :t + 1], state["hist"][:, :t + 1])


def test_top_k_1_is_the_argmax():
    V, R, t, T = 1001, 96, 0, 4
    g = torch.Generator().manual_seed(12)
    logits = torch.randn(R, V, generator=g) * 3
    out = launch(logits, V, t, T, 3, 1.0, 1, 1.0, 5, make_state(R, V, t, T, g))
    assert torch.equal(out["tok"].long(), logits.argmax(1))
    assert out["kept"].tolist() == [1] * R


# ------------------------------------------------------------- determinism
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (40, 0.9)], ids=["plain", "filtered"])
def test_same_seed_same_draws(top_k, top_p):
    V, R, t, T = 1001, 96, 1, 4
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(R, V, generator=g) * 3
    state = make_state(R, V, t, T, g)
    a = launch(logits, V, t, T, 3, 0.8, top_k, top_p, 123, state)
    b = launch(logits, V, t, T, 3, 0.8, top_k, top_p, 123, state)
    c = launch(logits, V, t, T, 3, 0.8, top_k, top_p, 124, state)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k  # bitwise, the scores too
    assert not torch.equal(a["tok"], c["tok"])
    assert torch.equal(a["kept"], c["kept"])


def test_seed_word_changes_a_replayed_graph():
    """One captured launch; the host changes only the device seed word between replays."""
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    V, R, t, T, end = 1001, 96, 1, 4, 3
    g = torch.Generator().manual_seed(22)
    logits = (torch.randn(R, V, generator=g) * 3).to(DEV)
    state = {k: v.to(DEV) for k, v in make_state(R, V, t, T, g).items()}
    work = {k: v.clone() for k, v in state.items()}
    tok = torch.zeros(R, dtype=torch.int32, device=DEV)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step():
        L.call("fpnmt_sample_step", R, V, logits.data_ptr(), V, 1.0, 40, 0.9, 5, word.data_ptr(),
               work["score"].data_ptr(), work["slen"].data_ptr(), work["fin"].data_ptr(), work["hist"].data_ptr(),
               T + 1, t, end, tok.data_ptr(), None, L.stream_ptr())

    step()  # once outside the capture (one-time kernel attributes)
    torch.cuda.synchronize()
    graph, = capture_sequence([step])
    draws = []
    for w in (1, 2, 1):
        for k in work:
            work[k].copy_(state[k])
        word.fill_(w)
        graph.replay()
        torch.cuda.synchronize()
        draws.append((tok.cpu().clone(), work["score"].cpu().clone()))
        key = draw_key(5, w)
        us = torch.zeros(R, device=DEV)
        L.call("fpnmt_sample_uniform", R, t, 5, word.data_ptr(), us.data_ptr(), L.stream_ptr())
        assert us.cpu().tolist() == [np.float32(uniform(key, r, t)) for r in range(R)]
    assert not torch.equal(draws[0][0], draws[1][0])
    assert torch.equal(draws[0][0], draws[2][0]) and torch.equal(draws[0][1], draws[2][1])


def test_sample_decode_graph_matches_eager_bf16():
    """Graph == eager == a second replay on a small bf16 model, with rows
    that finish at different steps (a finished row pads with <end> while the
    graphs replay for the others)."""
    import fpnmt
    fpnmt.set_precision("bf16")
    try:
        T, vocab, image, n_img, n_s = 12, 300, 224, 3, 6
        pl = _pipeline(2, vocab, image, 17, T, end_bias=3.2)
        g = torch.Generator().manual_seed(6)
        imgs = (torch.rand(n_img, image, image, 3, generator=g) * 2 - 1).to(DEV)
        kw = dict(mode="sample", n_samples=n_s, temperature=0.9, top_k=40, top_p=0.95, seed=31)
        a = pl.predict_batch(imgs, T, use_graph=False, **kw)
        b = pl.predict_batch(imgs, T, use_graph=True, **kw)
        c = pl.predict_batch(imgs, T, use_graph=True, **kw)  # replay of the captured graphs
        assert a == b == c
        lens = [len(ids) for img in a for ids, _ in img]
        print("caption lengths", lens)
        assert len(set(lens)) > 1 and min(lens) < T, lens
        d = pl.predict_batch(imgs, T, use_graph=True, **dict(kw, seed=32))
        assert d != a
    finally:
        fpnmt.set_precision("fp32")


# ----------------------------------------------------------- whole decoder
@pytest.fixture(scope="module")
def small_model():
    """The 2-layer, V = 200, 256^2 model of the beam tests on the GPU, its
    weights for the CPU oracle, and the oracle's encoder output per image."""
    import fpnmt
    from oracle import ref_cpu as R
    c = C_CFG
    fpnmt.set_precision("fp32")
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=c["n_layers"], num_heads=8, backbone="resnet50")
    imgs = torch.rand(c["n_img"], c["image"], c["image"], 3, generator=torch.Generator().manual_seed(c["image_seed"])) * 2 - 1
    encs = [R.encoder(sd, imgs[i][None], cfg) for i in range(c["n_img"])]
    return dict(pl=pl, sd=sd, cfg=cfg, imgs=imgs, encs=encs)


def test_sample_top_k_1_is_the_reference_decode(small_model):
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    ref = pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="reference")
    got = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=c["K"], top_k=1)
    for i in range(c["n_img"]):
        assert [ids for ids, _ in got[i]] == [ref[i]] * c["K"], (i, got[i], ref[i])


def test_sampled_trajectories_follow_the_oracle_fp32(small_model):
    """temperature 0.9, top_p 0.9: every GPU-sampled prefix goes through the
    CPU oracle; each drawn token's u must lie in the oracle's fp64 CDF
    interval (widened by 4 eps / temperature, eps = 1e-3 the fp32 logit
    parity bound) and the returned log-probability must be the oracle's
    teacher-forced sum within 2 eps per token."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl = m["pl"]
    temperature, top_p, seed, eps, n_s, T = 0.9, 0.9, 41, 1e-3, c["K"], c["T"]
    got = pl.predict_batch(m["imgs"].to(DEV), T, use_graph=False, mode="sample", n_samples=n_s,
                           temperature=temperature, top_p=top_p, seed=seed)
    key = draw_key(0, seed)
    tol = 4 * eps / temperature
    for i in range(c["n_img"]):
        seqs = []
        for ids, _ in got[i]:
            full = list(ids) + ([pl.end_token] if len(ids) < T else [])
            seqs.append(full)
        lp = [0.0] * n_s
        for t in range(max(len(s) for s in seqs)):
            live = [k for k in range(n_s) if len(seqs[k]) > t]
            logits = _cpu_logits(m["sd"], m["cfg"], m["encs"][i], [[pl.start_token] + seqs[k][:t] for k in live])
            for n, k in enumerate(live):
                tok = seqs[k][t]
                w, keep, _ = rule_ref(logits[n], temperature, 0, top_p)
                cdf = torch.cumsum(w * keep, 0)
                W = float(cdf[-1])
                u = uniform(key, i * n_s + k, t)
                lo, hi = float(cdf[tok] - w[tok] * keep[tok]) / W, float(cdf[tok]) / W
                assert lo - tol <= u < hi + tol, (i, k, t, tok, u, lo, hi)
                lp[k] += float(torch.log_softmax(logits[n].double(), 0)[tok])
        for k in range(n_s):
            ids, score = got[i][k]
            assert ids == seqs[k][:len(ids)] and pl.end_token not in ids
            assert abs(score - lp[k]) <= eps * 2 * len(seqs[k]), (i, k, score, lp[k])


def test_sample_mode_format_and_errors(small_model):
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = small_model, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    got = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=c["K"], seed=3)
    assert len(got) == c["n_img"]
    for img in got:
        assert len(img) == c["K"]
        for ids, score in img:
            assert isinstance(ids, list) and all(isinstance(x, int) for x in ids) and len(ids) <= c["T"]
            assert isinstance(score, float) and score < 0.0 and math.isfinite(score)
        assert len({tuple(ids) for ids, _ in img}) > 1, img  # temperature 1: the samples of an image differ
    again = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=c["K"], seed=3)
    assert again == got
    nxt = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=c["K"])  # the decoder's counter
    nxt2 = pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=c["K"])
    assert nxt != nxt2
    for kw in (dict(n_samples=0), dict(temperature=0.0), dict(temperature=float("nan")), dict(top_p=0.0),
               dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(ValueError):
            pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", **dict(dict(n_samples=2), **kw))


# ------------------------------------------------------------- error paths
def test_sample_entry_points_reject_bad_arguments():
    from fpnmt import _lib as L
    R, V, T = 4, 200, 12
    f = torch.zeros(R * V, device=DEV)
    big = torch.zeros(2 * 20000, device=DEV)
    sc = torch.zeros(R, device=DEV)
    i1, i2, i3, i4 = (torch.zeros(R * (T + 1), dtype=torch.int32, device=DEV) for _ in range(4))

    def step(vocab=V, logits=f.data_ptr(), ldl=None, temperature=1.0, top_k=0, top_p=1.0, score=sc.data_ptr(), t=0,
             hist_ld=T + 1, end=3, rows=R):
        return L.lib.fpnmt_sample_step(rows, vocab, logits, vocab if ldl is None else ldl, temperature, top_k, top_p,
                                       1, None, score, i1.data_ptr(), i2.data_ptr(), i3.data_ptr(), hist_ld, t, end,
                                       i4.data_ptr(), None, L.stream_ptr())

    bad = [(dict(temperature=0.0), b"temperature"), (dict(temperature=-1.0), b"temperature"),
           (dict(temperature=float("inf")), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
           (dict(top_p=0.0), b"top_p"), (dict(top_p=1.01), b"top_p"), (dict(top_p=float("nan")), b"top_p"),
           (dict(top_k=-1), b"top_k"), (dict(end=V), b"end_token"), (dict(end=-1), b"end_token"),
           (dict(t=-1), b"position"), (dict(t=65536, hist_ld=70000), b"position"), (dict(t=T, hist_ld=T + 1), b"width"),
           (dict(ldl=V - 1), b"ldl"), (dict(score=None), b"null"), (dict(logits=None), b"null")]
    for kw, word in bad:
        rc = step(**kw)
        assert rc == L.E_ARG and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    for kw in (dict(top_k=5), dict(top_p=0.5)):
        rc = step(vocab=20000, logits=big.data_ptr(), rows=2, **kw)
        assert rc == L.E_UNSUPPORTED and b"16384" in L.lib.fpnmt_last_error(), (kw, rc)
    assert step(vocab=20000, logits=big.data_ptr(), rows=2) == 0  # unfiltered: no limit
    assert step(vocab=20000, logits=big.data_ptr(), rows=2, top_k=20000) == 0  # top_k >= vocab: off
    u = torch.zeros(R, device=DEV)
    for kw, word in ((dict(t=-1), b"position"), (dict(t=65536), b"position"), (dict(out=None), b"null")):
        a = dict(dict(t=0, out=u.data_ptr()), **kw)
        rc = L.lib.fpnmt_sample_uniform(R, a["t"], 1, None, a["out"], L.stream_ptr())
        assert rc == L.E_ARG and word in L.lib.fpnmt_last_error(), (kw, rc, L.lib.fpnmt_last_error())
    torch.cuda.synchronize()

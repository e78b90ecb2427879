"""TrainEngine.eval_step / Pipeline.eval_step, validate and score_captions:
the held-out loss against the CPU oracle in inference mode, the arg-max hits
against the model's own logits, that an evaluation moves nothing (parameters,
optimizer state, moving statistics, dropout numbering), graph replay, and the
teacher-forced caption scores against the beam search's and the sampler's."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import _build
from test_gpu_scst_step import STATE, _captions, _images

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.1


def _engine(m, lr, **kw):
    from fpnmt.train import TrainEngine
    assert hasattr(TrainEngine, "eval_step"), "TrainEngine has no eval_step"
    return TrainEngine(m, lr, **kw)


def _oracle_eval(sd, img, tok, cfg, eps, training=False):
    """(smoothed loss, per-caption log-probability, lengths) on the CPU oracle."""
    from oracle import ref_cpu as R
    tar_inp, tar_real = tok[:, :-1], tok[:, 1:]
    with torch.no_grad():
        enc = R.encoder(sd, img, cfg, training=training)
        dec, _ = R.decoder(sd, tar_inp, enc, R.create_masks(tar_inp), cfg)
        logits = dec @ sd["final_layer.kernel"] + sd["final_layer.bias"]
        flat, lab = logits.reshape(-1, logits.shape[-1]), tar_real.reshape(-1).long()
        live = (lab != 0).float()
        loss = (F.cross_entropy(flat, lab, reduction="none", label_smoothing=eps) * live).mean()
        logp = (-F.cross_entropy(flat, lab, reduction="none") * live).view(tar_real.shape).sum(1)
    return float(loss), logp, (tar_real != 0).sum(1)


def test_eval_step_against_the_oracle_in_inference_mode_fp32():
    B, T, vocab, image = 2, 12, 300, 128
    m, sd, cfg = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T)
    img, tok = _images(B, image, 3), _captions(B, T, vocab, 4, lens=[12, 5])
    want_loss, want_logp, want_len = _oracle_eval(sd, img, tok, cfg, EPS)
    eng = _engine(m, 0.0, use_graph=False, label_smoothing=EPS)
    out = eng.eval_step(img.to(DEV), tok.to(DEV))
    assert set(out) == {"loss", "caption_logp", "caption_len", "caption_hit", "totals"}
    assert all(v.is_cuda for v in out.values())
    assert out["caption_logp"].dtype == torch.float32 and out["caption_len"].dtype == torch.int32
    assert out["caption_hit"].dtype == torch.int32 and out["totals"].dtype == torch.float64
    loss, logp, ln = float(out["loss"]), out["caption_logp"].cpu(), out["caption_len"].cpu()
    print(f"loss gpu {loss:.7f} oracle {want_loss:.7f}; logp gpu {logp.tolist()} oracle {want_logp.tolist()}")
    assert abs(loss - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    assert ln.tolist() == want_len.tolist() == [11, 4]
    for r in range(B):
        assert abs(float(logp[r]) - float(want_logp[r])) <= 2 * 1e-3 * int(ln[r]), r
    tot = out["totals"].cpu()
    assert float(tot[1]) == 15.0 and float(tot[2]) == float(out["caption_hit"].sum())
    assert abs(float(tot[0]) - float(logp.double().sum())) <= 2.0 ** -23 * abs(float(tot[0]))
    # n_per_image: the encoder once per image equals the images repeated
    tok3 = _captions(B * 3, T, vocab, 5).to(DEV)
    a = eng.eval_step(img.to(DEV), tok3, n_per_image=3)
    b = eng.eval_step(img.repeat_interleave(3, 0).to(DEV), tok3)
    assert torch.equal(a["caption_len"], b["caption_len"])
    assert bool(((a["caption_logp"] - b["caption_logp"]).abs() <= 2 * 1e-3 * a["caption_len"]).all())
    with pytest.raises(ValueError):
        eng.eval_step(img.to(DEV), tok3, n_per_image=2)


def _own_hits(m, img, tok, n):
    """Hits counted with torch from the logits of the same inference-mode launches."""
    from fpnmt import ops
    with torch.no_grad():
        tar_inp, tar_real, mask = ops.decoder_targets(tok)
        dec, _ = m.decoder(tar_inp, ops.RepeatRowsFn.apply(m.encoder(img, False, None), n), False, mask, None)
        logits = m.final_layer(dec)
    cols = torch.arange(logits.shape[-1], device=logits.device)
    first = torch.where(logits == logits.max(-1, keepdim=True).values, cols, logits.shape[-1]).min(-1).values
    return ((first == tar_real) & (tar_real != 0)).sum(1).int(), logits


# ------------------------------------------------------------ nothing moves
def _snapshot(m, eng):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd.update({"arena." + n: getattr(eng.arena, n).detach().clone() for n in STATE})
    sd["arena.grad"] = eng.arena.grad.detach().clone()
    return sd


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _bits(out):
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("backbone,precision", [("resnet50", "fp32"), ("mobilenet224_1.0", "bf16")])
def test_eval_step_moves_nothing(backbone, precision):
    import fpnmt
    B, T, vocab, image = 2, 12, 300, 128
    batches = [(_images(B, image, 20 + i).to(DEV), _captions(B, T, vocab, 30 + i).to(DEV)) for i in range(3)]
    ev_img, ev_tok = _images(B, image, 40).to(DEV), _captions(B, T, vocab, 41).to(DEV)
    kw = dict(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=71, rate=0.1, backbone=backbone)
    if backbone != "resnet50":
        # batch statistics are off: the loss is the oracle's training=False one, not its training=True one
        m, sd, cfg = _build(**kw)
        got = float(_engine(m, 0.0, use_graph=False).eval_step(ev_img, ev_tok)["loss"])
        off = _oracle_eval(sd, ev_img.cpu(), ev_tok.cpu(), cfg, 0.0, training=False)[0]
        on = _oracle_eval(sd, ev_img.cpu(), ev_tok.cpu(), cfg, 0.0, training=True)[0]
        print(f"mobilenet eval loss gpu {got:.7f} oracle inference {off:.7f} oracle training {on:.7f}")
        assert abs(got - off) <= 1e-4 * max(1.0, abs(off))
        assert abs(got - on) > 1e-4 * max(1.0, abs(on))
        del m
    fpnmt.set_precision(precision)
    try:
        for use_graph in (False, True):
            final = []
            for with_eval in (True, False):
                # one engine alive at a time: the dropout keys read the newest engine's step counter
                m, _, _ = _build(**kw)
                fpnmt.set_precision(precision)  # _build sets fp32
                eng = _engine(m, 1e-4, use_graph=use_graph, label_smoothing=EPS)
                outs = []
                for img, tok in batches:
                    eng.step(img, tok)
                    if with_eval:
                        before = _snapshot(m, eng)
                        outs.append(_bits(eng.eval_step(ev_img, ev_tok)))
                        torch.cuda.synchronize()
                        _assert_same(before, _snapshot(m, eng), "eval_step wrote")
                        again = _bits(eng.eval_step(ev_img, ev_tok))  # no dropout: the same bits
                        _assert_same(outs[-1], again, "two eval_step calls differ")
                torch.cuda.synchronize()
                if with_eval:
                    assert use_graph == (eng.graphs is not None)
                    assert use_graph == any(e[1] is not None for e in eng._esteps.values())
                    # the parameters moved between the evaluations, and the evaluations saw it
                    assert not torch.equal(outs[0]["loss"], outs[-1]["loss"])
                final.append(_snapshot(m, eng))
                if with_eval:
                    # the compute copies an evaluation reads after (replayed) steps are the current
                    # ones: the same bits with every copy rebuilt from the masters, eagerly
                    last = _bits(eng.eval_step(ev_img, ev_tok))
                    eng.use_graph = False
                    _assert_same(last, _bits(eng.eval_step(ev_img, ev_tok)), "eval_step read stale weight copies")
                del eng, m
            _assert_same(final[0], final[1], f"train, eval, train != train, train (graphs {use_graph})")
    finally:
        fpnmt.set_precision("fp32")


def test_eval_graph_replay_equals_eager_bits_and_survives_another_shape():
    B, T, vocab, image = 2, 12, 300, 128
    m, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=72, rate=0.1)
    E = _engine(m, 0.0, use_graph=False, label_smoothing=EPS)
    G = _engine(m, 0.0, use_graph=True, label_smoothing=EPS)  # the model's parameters now live in G's arena
    data = [(_images(B, image, 50 + i).to(DEV), _captions(B, T, vocab, 60 + i).to(DEV)) for i in range(4)]
    other = (_images(1, image, 59).to(DEV), _captions(1, T - 3, vocab, 69).to(DEV))
    for i, (img, tok) in enumerate(data):
        if i == 3:  # a batch of another shape between two replays
            _assert_same(_bits(G.eval_step(*other)), _bits(E.eval_step(*other)), "other shape")
        g, e = _bits(G.eval_step(img, tok)), _bits(E.eval_step(img, tok))
        torch.cuda.synchronize()
        _assert_same(g, e, f"call {i}")
    key = [k for k in G._esteps if k[0] == tuple(data[0][0].shape)]
    assert len(key) == 1 and G._esteps[key[0]][1] is not None and G._esteps[key[0]][0] == 4
    # a checkpoint restore / hand edit of the parameters reaches the replay
    from fpnmt.layers import invalidate_weights
    with torch.no_grad():
        m.final_layer.kernel.mul_(1.5)  # read through a compute copy: the replay must see the refreshed one
    invalidate_weights()
    g, e = _bits(G.eval_step(*data[0])), _bits(E.eval_step(*data[0]))
    _assert_same(g, e, "after an edit")
    first = _bits(E.eval_step(*data[0]))
    assert not torch.equal(first["loss"], _bits(G.eval_step(*data[1]))["loss"])


# ------------------------------------------- scores of the decode paths
SC = dict(n_layers=1, vocab=300, image=128, T=10, B=2, n=3, end_bias=4.0)


@pytest.fixture(scope="module")
def pipeline():
    import fpnmt
    from test_gpu_beam_search import _pipeline
    from utils.pipeline import Pipeline
    assert hasattr(Pipeline, "score_captions"), "Pipeline has no score_captions"
    fpnmt.set_precision("fp32")
    c = SC
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], 23, c["T"], c["end_bias"])
    return pl, _images(c["B"], c["image"], 9).to(DEV)


def _check_scores(pl, img, per_image, n):
    """Every decoded caption's score against the teacher-forced one. A
    caption that ended carries its <end> in the decoder's score: that is
    score_captions' convention. One that filled all T - 1 positions has no
    <end> in its score: its teacher-forced counterpart is eval_step on the
    self-critical packing (pack_tokens at the decoder's positions), which
    leaves the <end> out in the same way."""
    from fpnmt.scst import pack_tokens
    c = SC
    ids = [s[0] for per in per_image for s in per]
    score = [s[1] for per in per_image for s in per]
    assert len(ids) == c["B"] * n
    ended = [len(x) < c["T"] - 1 for x in ids]
    assert any(ended), [len(x) for x in ids]
    got = pl.score_captions(img, ids, n_per_image=n)
    tok = torch.from_numpy(pack_tokens(ids, c["T"], pl.start_token, pl.end_token, c["T"] - 1)).to(DEV)
    cut = pl.engine.eval_step(img, tok, n_per_image=n)
    cut = list(zip(cut["caption_logp"].cpu().tolist(), cut["caption_len"].cpu().tolist()))
    print("lengths", [g[1] for g in got], "ended", ended, "max |teacher-forced - decoder|",
          max(abs((g if e else k)[0] - s) for g, k, e, s in zip(got, cut, ended, score)))
    for r, s in enumerate(score):
        assert got[r][1] == len(ids[r]) + 1  # the final <end> counted
        lp, ln = got[r] if ended[r] else cut[r]
        assert ln == len(ids[r]) + ended[r]
        assert abs(lp - s) <= 2 * 1e-3 * ln, (r, lp, s)
    return ids, got


def test_score_captions_against_the_beam_search_and_hits_against_own_logits(pipeline):
    pl, img = pipeline
    c = SC
    best = pl.predict_batch(img, c["T"] - 1, use_graph=False, mode="beam", n_best=3, length_alpha=0.0)
    ids, got = _check_scores(pl, img, best, 3)
    assert len({g[1] for g in got}) > 1
    # image-major: caption r belongs to image r // 3 (scored against the other image it differs)
    swapped = pl.score_captions(img.flip(0), ids, n_per_image=3)
    assert all(a[0] != b[0] for a, b in zip(got, swapped))
    hits, lens = _check_hits(pl, img, ids, 3)
    assert 0 < sum(hits)  # a beam's tokens are mostly the model's arg-max


def _check_hits(pl, img, ids, n):
    """caption_hit: exact against torch on the logits of the same launches."""
    from fpnmt.scst import pack_tokens
    c = SC
    tok = torch.from_numpy(pack_tokens(ids, c["T"] + 1, pl.start_token, pl.end_token, c["T"])).to(DEV)
    out = pl.engine.eval_step(img, tok, n_per_image=n)
    want, _ = _own_hits(pl.transformer, img, tok, n)
    hits, lens = out["caption_hit"].cpu().tolist(), out["caption_len"].cpu().tolist()
    print("hits", hits, "lengths", lens)
    assert hits == want.cpu().tolist()
    assert all(0 <= h <= ln for h, ln in zip(hits, lens))
    return hits, lens


def test_score_captions_against_the_sampler(pipeline):
    pl, img = pipeline
    c = SC
    drawn = pl.predict_batch(img, c["T"] - 1, use_graph=False, mode="sample", n_samples=c["n"], seed=5,
                             temperature=1.0)
    ids, _ = _check_scores(pl, img, drawn, c["n"])
    hits, lens = _check_hits(pl, img, ids, c["n"])
    assert sum(hits) < sum(lens)  # samples leave the arg-max path


def test_score_captions_errors(pipeline):
    pl, img = pipeline
    c = SC
    ok = [[5, 6, 7]] * c["B"]
    assert len(pl.score_captions(img, ok)) == c["B"]
    assert pl.score_captions(img, [[5] * (c["T"] - 1)] * c["B"])[0][1] == c["T"]  # the longest that fits
    with pytest.raises(ValueError):
        pl.score_captions(img, [[5] * c["T"]] + ok[1:])
    with pytest.raises(ValueError):
        pl.score_captions(img, ok[:1])
    with pytest.raises(ValueError):
        pl.score_captions(img, ok, n_per_image=2)


def test_validate_accumulates_on_the_device(pipeline):
    pl, img = pipeline
    c = SC
    full = (img, _captions(c["B"], c["T"], c["vocab"], 80).to(DEV))
    short = (img[:1], _captions(1, c["T"], c["vocab"], 81).to(DEV))
    parts = [pl.eval_step(*b)["totals"].cpu() for b in (full, short)]
    want = parts[0] + parts[1]
    res = pl.validate([full, short])
    assert set(res) == {"token_nll", "perplexity", "token_accuracy", "tokens", "captions", "totals"}
    assert res["captions"] == 3 and res["tokens"] == int(want[1])
    assert res["totals"][1] == float(want[1]) and res["totals"][2] == float(want[2])
    assert abs(res["totals"][0] - float(want[0])) <= 4 * 2.0 ** -53 * abs(float(want[0]))
    assert res["perplexity"] == math.exp(-res["totals"][0] / res["tokens"])
    assert res["token_accuracy"] == res["totals"][2] / res["tokens"]
    again = pl.validate(iter([full, short]))  # the running sums start from zero every time
    assert again["totals"] == res["totals"]
    with pytest.raises(ValueError):
        pl.validate([])

"""TrainEngine(label_smoothing=eps): the plain step's gradients against the
CPU oracle restated with torch's own label_smoothing (fp64 anchor, the fp32
oracle's error as the noise floor: the bars of tests/test_gpu_scst_step.py),
graph replay, the untouched default and self-critical steps, the interface."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import _build, _perturbed
from test_gpu_scst_step import STATE, _bars, _captions, _grads, _images, _sync_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.1


def _engine(m, lr, **kw):
    import inspect
    from fpnmt.train import TrainEngine
    assert "label_smoothing" in inspect.signature(TrainEngine.__init__).parameters, \
        "TrainEngine has no label_smoothing argument"
    return TrainEngine(m, lr, **kw)


def oracle_smoothed(sd, img, tok, cfg, trainable, eps, dtype=torch.float32):
    """The plain step's loss on the CPU oracle with F.cross_entropy's
    label_smoothing: masked, a mean over ALL rows. Returns (loss, grads)."""
    from oracle import ref_cpu as R
    params = {k: v.to(dtype).detach().clone().requires_grad_(k in trainable) if v.is_floating_point() else v
              for k, v in sd.items()}
    tar_inp, tar_real = tok[:, :-1], tok[:, 1:]
    enc = R.encoder(params, img.to(dtype), cfg, training=True, stats=cfg.get("bn_stats"))
    dec, _ = R.decoder(params, tar_inp, enc, R.create_masks(tar_inp), cfg)
    logits = dec @ params["final_layer.kernel"] + params["final_layer.bias"]
    ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), tar_real.reshape(-1).long(), reduction="none",
                         label_smoothing=eps)
    loss = (ce * (tar_real.reshape(-1) != 0).to(dtype)).mean()
    loss.backward()
    grads = {k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])) for k in trainable}
    return loss.detach(), grads


def test_smoothed_step_gradients_against_the_oracle_fp32(parity_record):
    B, T, vocab, image = 2, 12, 300, 128
    m, sd, cfg = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T)
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    img = _images(B, image, 3)
    tok = _captions(B, T, vocab, 4, lens=[12, 5])
    l64, g64 = oracle_smoothed(sd, img, tok, cfg, trainable, EPS, torch.float64)
    l32, g32 = oracle_smoothed(sd, img, tok, cfg, trainable, EPS)
    _, g32p = oracle_smoothed(sd, _perturbed(img, 77), tok, cfg, trainable, EPS)
    l32_plain, _ = oracle_smoothed(sd, img, tok, cfg, trainable, 0.0)
    eng = _engine(m, 0.0, use_graph=False, label_smoothing=EPS)
    loss = float(eng.step(img.to(DEV), tok.to(DEV)))
    torch.cuda.synchronize()
    rows, bulk = _bars(m, g64, _grads(m), [g32, g32p])
    loss0 = float(_engine(m, 0.0, use_graph=False).step(img.to(DEV), tok.to(DEV)))
    for r in sorted(rows, key=lambda r: -r[1])[:3]:
        print("grad max rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    for r in sorted(bulk, key=lambda r: -r[1])[:3]:
        print("grad p90 rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    print(f"loss gpu {loss:.7f} oracle32 {float(l32):.7f} oracle64 {float(l64):.7f}; eps 0: gpu {loss0:.7f} "
          f"oracle32 {float(l32_plain):.7f}")
    parity_record["label_smoothing_step_1L_V300_128_b2"] = {
        "loss_gpu": loss, "loss_oracle32": float(l32), "loss_oracle64": float(l64), "loss_gpu_eps0": loss0,
        "grad_max_rel_err_vs_fp64_worst": [{"param": r[3], "gpu": r[1], "cpu_fp32": r[2]}
                                           for r in sorted(rows, key=lambda r: -r[1])][:5]}
    bar = 1e-4 * max(1.0, abs(float(l32)))
    assert abs(loss - float(l32)) <= bar
    assert abs(loss - loss0) > bar and abs(loss0 - float(l32_plain)) <= bar  # the term is really on
    assert rows[0][0] <= 0.0, rows[0]
    assert bulk[0][0] <= 0.0, bulk[0]


def _batches(B, T, vocab, image, k):
    return [(_images(B, image, 20 + i).to(DEV), _captions(B, T, vocab, 30 + i).to(DEV)) for i in range(k)]


def test_graph_replay_is_bitwise_the_eager_step_bf16():
    """Eager and graph engines put in the same state before every step: the
    first call (eager in both), the capture, a replay; with dropout."""
    import fpnmt
    B, T, vocab, image = 2, 12, 300, 128
    m_e, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=51, rate=0.1)
    m_g, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=51, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = _engine(m_e, 1e-4, use_graph=False, label_smoothing=EPS)
        G = _engine(m_g, 1e-4, use_graph=True, label_smoothing=EPS)
        losses = []
        for i, (img, tok) in enumerate(_batches(B, T, vocab, image, 3)):
            _sync_state(G, E)
            le = E.step(img, tok).clone()
            lg = G.step(img, tok).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            for nme in STATE:
                assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (i, nme)
            losses.append(float(le))
        assert len(set(losses)) == 3 and int(E.arena.step) == 3 and G.graphs is not None
    finally:
        fpnmt.set_precision("fp32")


def test_label_smoothing_zero_is_the_default():
    """Two steps (the second a graph capture + replay): an engine built with
    label_smoothing=0.0 leaves the arena of one built without the argument."""
    B, T, vocab, image = 2, 12, 300, 128
    m_a, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=52)
    m_b, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=52)
    A = _engine(m_a, 1e-4, use_graph=True)
    Bn = _engine(m_b, 1e-4, use_graph=True, label_smoothing=0.0)
    assert A.label_smoothing == 0.0
    for img, tok in _batches(B, T, vocab, image, 2):
        la, lb = A.step(img, tok).clone(), Bn.step(img, tok).clone()
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    for nme in STATE:
        assert torch.equal(getattr(A.arena, nme), getattr(Bn.arena, nme)), nme


def test_step_weighted_is_not_smoothed():
    B, n, T, vocab, image = 2, 2, 12, 300, 128
    m_a, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=53)
    m_b, _, _ = _build(num_layers=1, vocab=vocab, image=image, max_seq_len=T, seed=53)
    A = _engine(m_a, 1e-4, use_graph=False, label_smoothing=0.0)
    Bs = _engine(m_b, 1e-4, use_graph=False, label_smoothing=EPS)
    img, tok = _images(B, image, 5).to(DEV), _captions(B * n, T, vocab, 6).to(DEV)
    w = torch.tensor([1.3, -0.8, 0.0, 0.6], device=DEV)
    la, lb = A.step_weighted(img, tok, w).clone(), Bs.step_weighted(img, tok, w).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for nme in STATE:
        assert torch.equal(getattr(A.arena, nme), getattr(Bs.arena, nme)), nme


def test_label_smoothing_interface():
    import inspect
    from fpnmt.layers import Init
    from utils.pipeline import Pipeline
    assert "label_smoothing" in inspect.signature(Pipeline.__init__).parameters, \
        "Pipeline has no label_smoothing argument"
    kw = dict(max_seq_len=12, target_vocab_size=300, image_size=128, n_layers=1, rate=0.0,
              init=Init(torch.Generator().manual_seed(1)), use_graph=False)
    pl = Pipeline(label_smoothing=EPS, **kw)
    assert pl.engine.label_smoothing == EPS
    assert Pipeline(**kw).engine.label_smoothing == 0.0
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            _engine(pl.transformer, 0.0, use_graph=False, label_smoothing=bad)
    with pytest.raises(ValueError):
        Pipeline(label_smoothing=1.0, **kw)
    assert math.isfinite(float(pl.train_step(_images(2, 128, 1).to(DEV), _captions(2, 12, 300, 2).to(DEV))))

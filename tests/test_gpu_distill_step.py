"""TrainEngine.set_distill / step_distill: the step's gradients against the
CPU oracle restated with the composite loss (fp64 anchor, the fp32 oracle's
error as the noise floor: the bars of tests/test_gpu_scst_step.py), real
teachers against the same step fed their hand-folded logits, graph replay,
annealing through the device descriptor without recapture, the untouched
default, the step together with a frozen backbone, the average and the step
guard, and the interface. Tiny model: the label-smoothing step test's."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_model import _build, _perturbed
from test_gpu_scst_step import STATE, _bars, _captions, _grads, _images, _sync_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, ALPHA, TEMP = 0.1, 0.5, 2.0
B, T, VOCAB, IMAGE = 2, 12, 300, 128


def _engine(m, lr, **kw):
    from fpnmt.train import TrainEngine
    assert hasattr(TrainEngine, "set_distill") and hasattr(TrainEngine, "step_distill"), \
        "TrainEngine has no set_distill / step_distill"
    return TrainEngine(m, lr, **kw)


def _model(seed, num_layers=1, rate=0.0):
    return _build(num_layers=num_layers, vocab=VOCAB, image=IMAGE, max_seq_len=T, seed=seed, rate=rate)


def _soft(seed, scale=2.0):
    return torch.randn(B, T - 1, VOCAB, generator=torch.Generator().manual_seed(seed)) * scale


def _batches(k):
    return [(_images(B, IMAGE, 20 + i).to(DEV), _captions(B, T, VOCAB, 30 + i).to(DEV), _soft(40 + i).to(DEV))
            for i in range(k)]


def oracle_distill(sd, img, tok, z, cfg, trainable, eps, alpha, temp, dtype=torch.float32):
    """The distillation step's loss on the CPU oracle: masked, a mean over ALL
    rows of (1 - a) CE(label_smoothing=eps) + a T^2 KL(softmax(z / T) ||
    softmax(logits / T)). Returns (loss, grads)."""
    from oracle import ref_cpu as R
    params = {k: v.to(dtype).detach().clone().requires_grad_(k in trainable) if v.is_floating_point() else v
              for k, v in sd.items()}
    tar_inp, tar_real = tok[:, :-1], tok[:, 1:]
    enc = R.encoder(params, img.to(dtype), cfg, training=True, stats=cfg.get("bn_stats"))
    dec, _ = R.decoder(params, tar_inp, enc, R.create_masks(tar_inp), cfg)
    logits = (dec @ params["final_layer.kernel"] + params["final_layer.bias"]).reshape(-1, VOCAB)
    ce = F.cross_entropy(logits, tar_real.reshape(-1).long(), reduction="none", label_smoothing=eps)
    lq = torch.log_softmax(z.to(dtype).reshape(-1, VOCAB) / temp, 1)
    kl = (lq.exp() * (lq - torch.log_softmax(logits / temp, 1))).sum(1)
    loss = (((1 - alpha) * ce + alpha * temp * temp * kl) * (tar_real.reshape(-1) != 0).to(dtype)).mean()
    loss.backward()
    grads = {k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])) for k in trainable}
    return loss.detach(), grads


def test_distill_step_gradients_against_the_oracle_fp32(parity_record):
    m, sd, cfg = _model(1234)
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    img = _images(B, IMAGE, 3)
    tok = _captions(B, T, VOCAB, 4, lens=[12, 5])
    z = _soft(5)
    l64, g64 = oracle_distill(sd, img, tok, z, cfg, trainable, EPS, ALPHA, TEMP, torch.float64)
    l32, g32 = oracle_distill(sd, img, tok, z, cfg, trainable, EPS, ALPHA, TEMP)
    _, g32p = oracle_distill(sd, _perturbed(img, 77), tok, z, cfg, trainable, EPS, ALPHA, TEMP)
    l32_hard, _ = oracle_distill(sd, img, tok, z, cfg, trainable, EPS, 0.0, TEMP)
    eng = _engine(m, 0.0, use_graph=False, label_smoothing=EPS)
    eng.set_distill([], alpha=ALPHA, temperature=TEMP)
    loss = float(eng.step_distill(img.to(DEV), tok.to(DEV), teacher_logits=z.to(DEV)))
    torch.cuda.synchronize()
    stats = eng.distill_stats.tolist()
    rows, bulk = _bars(m, g64, _grads(m), [g32, g32p])
    eng.set_distill_alpha(0.0)
    loss0 = float(eng.step_distill(img.to(DEV), tok.to(DEV), teacher_logits=z.to(DEV)))
    for r in sorted(rows, key=lambda r: -r[1])[:3]:
        print("grad max rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    for r in sorted(bulk, key=lambda r: -r[1])[:3]:
        print("grad p90 rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    print(f"loss gpu {loss:.7f} oracle32 {float(l32):.7f} oracle64 {float(l64):.7f}; alpha 0: gpu {loss0:.7f} "
          f"oracle32 {float(l32_hard):.7f}; stats {stats}")
    parity_record["distill_step_1L_V300_128_b2"] = {
        "loss_gpu": loss, "loss_oracle32": float(l32), "loss_oracle64": float(l64), "loss_gpu_alpha0": loss0,
        "stats": stats,
        "grad_max_rel_err_vs_fp64_worst": [{"param": r[3], "gpu": r[1], "cpu_fp32": r[2]}
                                           for r in sorted(rows, key=lambda r: -r[1])][:5]}
    bar = 1e-4 * max(1.0, abs(float(l32)))
    assert abs(loss - float(l32)) <= bar
    assert abs(loss - loss0) > bar and abs(loss0 - float(l32_hard)) <= bar  # the term is really on
    # the parts: loss = (1 - a) hard + a T^2 kl, hard = the alpha-0 loss
    assert stats[0] == loss and abs(stats[1] - loss0) <= bar
    assert abs((1 - ALPHA) * stats[1] + ALPHA * TEMP * TEMP * stats[2] - loss) <= bar
    assert rows[0][0] <= 0.0, rows[0]
    assert bulk[0][0] <= 0.0, bulk[0]


def _hand_logits(teachers, weights, mode, img, tok):
    """The teachers' folded teacher-forced logits, by hand: the inference
    forward of TrainEngine._eval_forward per teacher, then one
    fpnmt_logits_ensemble over all rows."""
    import fpnmt
    from fpnmt import _lib as L
    from fpnmt import layers as flayers
    from fpnmt import ops
    outs = []
    with torch.no_grad():
        tar_inp, _, mask = ops.decoder_targets(tok)
        for t in teachers:
            flayers.prepare_all(t, fpnmt.compute_dtype())
            dec, _ = t.decoder(tar_inp, t.encoder(img, False, None), False, mask, None)
            outs.append(t.final_layer(dec).contiguous())
    n = len(outs)
    w = [x / sum(weights) for x in weights]
    L.call("fpnmt_logits_ensemble", B * (T - 1), VOCAB, n, (C.c_void_p * n)(*[x.data_ptr() for x in outs]),
           (C.c_longlong * n)(*[VOCAB] * n), (C.c_float * n)(*w), {"prob": 0, "logprob": 1}[mode], None,
           outs[0].data_ptr(), VOCAB, L.stream_ptr())
    return outs[0]


def test_real_teachers_are_the_hand_folded_logits():
    t1, _, _ = _model(61)
    t2, _, _ = _model(62, num_layers=2)
    before = [{k: v.detach().clone() for k, v in t.state_dict().items()} for t in (t1, t2)]
    m_a, _, _ = _model(60)
    m_b, _, _ = _model(60)
    A = _engine(m_a, 1e-4, use_graph=False, label_smoothing=EPS)
    Bn = _engine(m_b, 1e-4, use_graph=False, label_smoothing=EPS)
    A.set_distill([t1, t2], alpha=ALPHA, temperature=TEMP, ensemble_mode="prob", ensemble_weights=(1, 3))
    Bn.set_distill([], alpha=ALPHA, temperature=TEMP)
    img, tok, _ = _batches(1)[0]
    la = A.step_distill(img, tok).clone()
    z = _hand_logits([t1, t2], (1.0, 3.0), "prob", img, tok).reshape(B, T - 1, VOCAB)
    lb = Bn.step_distill(img, tok, teacher_logits=z).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb), (float(la), float(lb))
    assert torch.equal(A.distill_stats, Bn.distill_stats) and float(A.distill_stats[2]) > 0
    for nme in STATE:
        assert torch.equal(getattr(A.arena, nme), getattr(Bn.arena, nme)), nme
    assert int(A.arena.step) == 1
    # the fold matters: one teacher alone gives another loss
    m_c, _, _ = _model(60)
    Cn = _engine(m_c, 1e-4, use_graph=False, label_smoothing=EPS)
    Cn.set_distill([t1], alpha=ALPHA, temperature=TEMP)
    assert float(Cn.step_distill(img, tok)) != float(la)
    # nothing of the teachers was written
    for t, sd0 in zip((t1, t2), before):
        for k, v in t.state_dict().items():
            assert torch.equal(v, sd0[k]), k


def test_graph_replay_is_bitwise_the_eager_step_bf16():
    """Eager and graph engines put in the same state before every step: the
    first call (eager in both), the capture, a replay; with dropout in the
    student and the teacher's forward inside the captured graph."""
    import fpnmt
    teacher, _, _ = _model(71, rate=0.1)
    m_e, _, _ = _model(70, rate=0.1)
    m_g, _, _ = _model(70, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = _engine(m_e, 1e-4, use_graph=False, label_smoothing=EPS)
        G = _engine(m_g, 1e-4, use_graph=True, label_smoothing=EPS)
        for eng in (E, G):
            eng.set_distill([teacher], alpha=ALPHA, temperature=TEMP)
        losses = []
        for i, (img, tok, z) in enumerate(_batches(3)):
            _sync_state(G, E)
            le, lg = E.step_distill(img, tok).clone(), G.step_distill(img, tok).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            assert torch.equal(E.distill_stats, G.distill_stats), i
            for nme in STATE:
                assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (i, nme)
            losses.append(float(le))
        assert len(set(losses)) == 3 and int(E.arena.step) == 3
        (ent,) = G._dsteps.values()
        assert ent[0] == 3 and ent[1] is not None and G.graphs is None  # its own graphs, not the plain step's
        # precomputed soft targets go through a static buffer of their own
        for i, (img, tok, z) in enumerate(_batches(3)):
            _sync_state(G, E)
            le = E.step_distill(img, tok, teacher_logits=z).clone()
            lg = G.step_distill(img, tok, teacher_logits=z).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            for nme in STATE:
                assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (i, nme)
        assert len(G._dsteps) == 2
    finally:
        fpnmt.set_precision("fp32")


def test_annealing_alpha_and_temperature_without_recapture():
    m_g, _, _ = _model(72)
    G = _engine(m_g, 1e-4, use_graph=True, label_smoothing=EPS)
    G.set_distill([], alpha=ALPHA, temperature=TEMP)
    batches = _batches(4)
    for img, tok, z in batches[:2]:  # eager, then capture + replay
        G.step_distill(img, tok, teacher_logits=z)
    (ent,) = G._dsteps.values()
    graphs = ent[1]
    assert graphs is not None
    for (img, tok, z), (alpha, temp) in zip(batches[2:], ((0.9, TEMP), (0.9, 3.0))):
        G.set_distill_alpha(alpha)
        G.set_distill_temperature(temp)
        m_e, _, _ = _model(72)
        E = _engine(m_e, 1e-4, use_graph=False, label_smoothing=EPS)
        E.set_distill([], alpha=alpha, temperature=temp)
        _sync_state(E, G)
        le = E.step_distill(img, tok, teacher_logits=z).clone()
        lg = G.step_distill(img, tok, teacher_logits=z).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg), (alpha, temp, float(le), float(lg))
        assert torch.equal(E.distill_stats, G.distill_stats)
        for nme in STATE:
            assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (alpha, temp, nme)
        assert G._dsteps[next(iter(G._dsteps))][1] is graphs  # no recapture
    # and the new values did change the step: the old mix gives another loss from the same state
    m_o, _, _ = _model(72)
    O = _engine(m_o, 1e-4, use_graph=False, label_smoothing=EPS)
    O.set_distill([], alpha=ALPHA, temperature=TEMP)
    img, tok, z = batches[3]
    assert float(O.step_distill(img, tok, teacher_logits=z)) != float(lg)


def test_set_frozen_drops_the_distillation_graphs():
    """set_frozen("backbone", True) then False between captured step_distill
    calls: the distillation graphs are dropped with the others (they recorded
    the old autograd graph) and rebuilt, the backbone stands still while
    frozen and moves again afterwards, and the whole trajectory is bitwise an
    eager engine's (bf16, dropout, the teacher inside the graph)."""
    import fpnmt
    from test_gpu_param_groups_step import BB, _group, _segs
    teacher, _, _ = _model(81, rate=0.1)
    m_e, _, _ = _model(80, rate=0.1)
    m_g, _, _ = _model(80, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = _engine(m_e, 1e-4, use_graph=False, label_smoothing=EPS, param_groups=[_group(m_e, "backbone")])
        G = _engine(m_g, 1e-4, use_graph=True, label_smoothing=EPS, param_groups=[_group(m_g, "backbone")])
        for eng in (E, G):
            eng.set_distill([teacher], alpha=ALPHA, temperature=TEMP)
        lo = G.arena.offsets[_segs(G, BB)[0]]
        batches = _batches(9)
        seen = []
        for phase, frozen in enumerate((False, True, False)):
            if phase:
                assert G._dsteps and G.distill_stats is not None
                for eng in (E, G):
                    eng.set_frozen("backbone", frozen)
                assert G._dsteps == {} and G.distill_stats is None and G._wsteps == {} and G.graphs is None
                assert all(p.requires_grad != frozen for n, p in m_g.named_parameters() if n.startswith(BB))
            for k in range(3):
                i = 3 * phase + k
                img, tok, _ = batches[i]
                _sync_state(G, E)
                p0 = G.arena.flat.clone()
                le, lg = E.step_distill(img, tok).clone(), G.step_distill(img, tok).clone()
                torch.cuda.synchronize()
                assert torch.equal(le, lg), i
                assert torch.equal(E.distill_stats, G.distill_stats), i
                for nme in STATE:
                    assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), (i, nme)
                assert torch.equal(G.arena.flat[lo:], p0[lo:]) == frozen, (i, frozen)
                assert not torch.equal(G.arena.flat[:lo], p0[:lo])
                (ent,) = G._dsteps.values()
                assert (ent[1] is not None) == (k >= 1), (i, k)  # eager, then capture, then replay
            seen.append(ent[1])
        assert seen[0] is not seen[1] and seen[1] is not seen[2]
        assert int(G.arena.step) == 9
    finally:
        fpnmt.set_precision("fp32")


def test_new_teacher_weights_reach_a_captured_step():
    """Weights loaded into a teacher after the step was captured
    (layers.invalidate_weights()): the next replay reads the teacher's
    refreshed compute copies, bitwise the eager engine's step, without a
    recapture."""
    import fpnmt
    from fpnmt import layers as flayers
    teacher, _, _ = _model(83)
    m_e, _, _ = _model(82)
    m_g, _, _ = _model(82)
    fpnmt.set_precision("bf16")
    try:
        E = _engine(m_e, 1e-4, use_graph=False, label_smoothing=EPS)
        G = _engine(m_g, 1e-4, use_graph=True, label_smoothing=EPS)
        for eng in (E, G):
            eng.set_distill([teacher], alpha=ALPHA, temperature=TEMP)
        batches = _batches(3)
        for img, tok, _ in batches[:2]:  # eager, then capture + replay
            G.step_distill(img, tok)
        (ent,) = G._dsteps.values()
        graphs = ent[1]
        img, tok, _ = batches[2]
        _sync_state(E, G)
        state = {nme: getattr(G.arena, nme).clone() for nme in STATE}
        old = G.step_distill(img, tok).clone()  # the step with the teacher as it was
        with torch.no_grad():
            for nme, v in state.items():
                getattr(G.arena, nme).copy_(v)
            teacher.final_layer.kernel.mul_(-0.5)
            teacher.encoder.enc_layers[0].ffn1.kernel.mul_(1.5)
        flayers.invalidate_weights()
        flayers.prepare_all(G.model)
        flayers.prepare_all(E.model)
        lg = G.step_distill(img, tok).clone()
        le = E.step_distill(img, tok).clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg) and not torch.equal(lg, old), (float(le), float(lg), float(old))
        for nme in STATE:
            assert torch.equal(getattr(E.arena, nme), getattr(G.arena, nme)), nme
        assert G._dsteps[next(iter(G._dsteps))][1] is graphs  # no recapture
    finally:
        fpnmt.set_precision("fp32")


def test_default_steps_are_untouched():
    """An engine on which set_distill was called and cleared again, against
    one that never saw it: step() (eager, capture, replay) and
    step_weighted() leave the same bits."""
    teacher, _, _ = _model(74)
    m_a, _, _ = _model(73)
    m_b, _, _ = _model(73)
    A = _engine(m_a, 1e-4, use_graph=True, label_smoothing=EPS)
    Bn = _engine(m_b, 1e-4, use_graph=True, label_smoothing=EPS)
    Bn.set_distill([teacher], alpha=ALPHA, temperature=TEMP)
    Bn.set_distill(None)
    with pytest.raises(ValueError, match="set_distill"):
        Bn.step_distill(*_batches(1)[0][:2])
    for img, tok, _ in _batches(2):
        la, lb = A.step(img, tok).clone(), Bn.step(img, tok).clone()
        assert torch.equal(la, lb)
    n = 2
    tok_w = _captions(B * n, T, VOCAB, 6).to(DEV)
    w = torch.tensor([1.3, -0.8, 0.0, 0.6], device=DEV)
    img = _images(B, IMAGE, 5).to(DEV)
    la, lb = A.step_weighted(img, tok_w, w).clone(), Bn.step_weighted(img, tok_w, w).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for nme in STATE:
        assert torch.equal(getattr(A.arena, nme), getattr(Bn.arena, nme)), nme
    assert A.distill_stats is None and Bn.distill_stats is None


def _pipeline(**kw):
    from fpnmt.layers import Init
    from utils.pipeline import Pipeline
    assert hasattr(Pipeline, "set_teachers") and hasattr(Pipeline, "train_step_distill"), \
        "Pipeline has no set_teachers / train_step_distill"
    base = dict(max_seq_len=T, target_vocab_size=VOCAB, image_size=IMAGE, n_layers=1, rate=0.0,
                init=Init(torch.Generator().manual_seed(1)), use_graph=False)
    base.update(kw)
    return Pipeline(**base)


def test_distill_with_frozen_backbone_average_and_guard():
    pl = _pipeline(freeze=("backbone",), ema_decay=0.99, skip_nonfinite=True, label_smoothing=EPS, use_graph=True)
    teacher = _pipeline()
    pl.set_teachers([teacher], alpha=ALPHA, temperature=TEMP)
    assert pl.engine._distill.teachers[0] is teacher.transformer
    batches = _batches(3)
    ar = pl.engine.arena
    flat0, ema0 = ar.flat.clone(), ar.ema.clone()
    for img, tok, z in batches[:2]:
        assert math.isfinite(float(pl.train_step_distill(img, tok, teacher_logits=z)))
    # the schedule's first rate is 0: over the two steps the trained parameters and their average moved
    assert not torch.equal(ar.flat, flat0) and not torch.equal(ar.ema, ema0)
    st = pl.distill_stats()
    assert set(st) == {"loss", "hard", "kl", "alpha", "temperature"} and st["alpha"] == ALPHA and st["kl"] > 0
    assert abs((1 - ALPHA) * st["hard"] + ALPHA * TEMP * TEMP * st["kl"] - st["loss"]) <= 1e-4 * max(1.0, st["loss"])
    assert pl.guard_stats()["n_applied"] == 2 and pl.guard_stats()["n_skipped"] == 0
    mean_before = float(pl.train_loss.result())
    # a NaN in the soft targets: the guard skips the step, bit for bit
    keep = {nme: getattr(ar, nme).clone() for nme in STATE + ("ema",)}
    img, tok, z = batches[2]
    z = z.clone()
    z[0, 1, 7] = float("nan")
    loss = pl.train_step_distill(img, tok, teacher_logits=z)
    torch.cuda.synchronize()
    assert math.isnan(float(loss))
    gs = pl.guard_stats()
    assert gs["skipped"] == 1 and gs["n_skipped"] == 1 and gs["n_applied"] == 2
    for nme, v in keep.items():
        assert torch.equal(getattr(ar, nme), v), nme
    assert float(pl.train_loss.result()) == mean_before  # the skipped step's loss stays out
    # the teachers run too (the graph path: eager, capture, replay)
    for img, tok, _ in batches:
        assert math.isfinite(float(pl.train_step_distill(img, tok)))
    assert pl.guard_stats()["n_applied"] == 5


def test_distill_interface_errors():
    m, _, _ = _model(75)
    eng = _engine(m, 1e-4, use_graph=False)
    img, tok, z = _batches(1)[0]
    with pytest.raises(ValueError, match="set_distill"):
        eng.step_distill(img, tok)
    with pytest.raises(ValueError, match="set_distill"):
        eng.set_distill_alpha(0.5)
    other, _, _ = _build(num_layers=1, vocab=VOCAB + 1, image=IMAGE, max_seq_len=T, seed=76)
    with pytest.raises(ValueError, match="vocabulary"):
        eng.set_distill([other])
    same, _, _ = _model(77)
    with pytest.raises(ValueError, match="at most 8"):
        eng.set_distill([same] * 9)
    eng.set_distill([same] * 8)
    with pytest.raises(ValueError, match="ensemble_weights"):
        eng.set_distill([same, same], ensemble_weights=(1.0,))
    with pytest.raises(ValueError, match="ensemble_mode"):
        eng.set_distill([same], ensemble_mode="mean")
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            eng.set_distill([same], alpha=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            eng.set_distill([same], temperature=bad)
    eng.set_distill([same], alpha=0.25, temperature=1.5)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match="alpha"):
            eng.set_distill_alpha(bad)
    with pytest.raises(ValueError, match="temperature"):
        eng.set_distill_temperature(0.0)
    assert eng._distill.desc.table.tolist() == [0.25, 1.5, 0.0, 0.0]  # a refused value writes nothing
    for bad in (z[:, :-1], z[..., :-1], z.double(), z.cpu(), z[0]):
        with pytest.raises(ValueError, match="teacher_logits"):
            eng.step_distill(img, tok, teacher_logits=bad)
    with pytest.raises(ValueError, match="captions"):
        eng.step_distill(img, tok[:1])
    short, _, _ = _build(num_layers=1, vocab=VOCAB, image=IMAGE, max_seq_len=T - 4, seed=78)
    eng.set_distill([short])
    with pytest.raises(ValueError, match="positional table"):
        eng.step_distill(img, tok)
    eng.set_distill([])
    with pytest.raises(ValueError, match="no teachers"):
        eng.step_distill(img, tok)
    assert int(eng.arena.step) == 0  # nothing above took a step
    assert math.isfinite(float(eng.step_distill(img, tok, teacher_logits=z)))

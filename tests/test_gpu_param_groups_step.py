"""Parameter groups in the training step (TrainEngine(param_groups=...)): a
frozen backbone / feature extractor is pruned from the backward and skipped by
the optimizer, a group's rate scale and weight decay change between replays
without a recapture, freezing and unfreezing at run time, the split and
data-parallel forms, MobileNetV2's BatchNorm under a frozen backbone, and
checkpoints across groupings.

Model: test_gpu_model._build(num_layers=1, vocab=300, image=128,
max_seq_len=12), B = 2, captions of lengths 12 and 5."""
import inspect
import os
import types

import pytest
import torch

from test_gpu_model import _build, _perturbed
from test_gpu_scst_step import _bars, _captions, _images, oracle_weighted

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("flat", "m", "v", "vhat", "step")
B, T, VOCAB, IMAGE = 2, 12, 300, 128
BB = "encoder.feature_extractor.retinanet_model.backbone."
FE = "encoder.feature_extractor."


def _require_feature():
    from fpnmt.train import TrainEngine
    assert "param_groups" in inspect.signature(TrainEngine.__init__).parameters, \
        "TrainEngine has no param_groups argument"


def _model(seed=31, rate=0.0, backbone="resnet50"):
    return _build(num_layers=1, vocab=VOCAB, image=IMAGE, max_seq_len=T, seed=seed, rate=rate, backbone=backbone)


def _batch(i=0, n=1):
    lens = [12, 5] * n
    return _images(B, IMAGE, 40 + i).to(DEV), _captions(B * n, T, VOCAB, 50 + i, lens=lens).to(DEV)


def _sync_state(dst, src):
    from fpnmt import layers as flayers
    with torch.no_grad():
        for nme in STATE:
            getattr(dst.arena, nme).copy_(getattr(src.arena, nme))
    flayers.prepare_all(dst.model)


def _same_state(a, b, what):
    for nme in STATE:
        assert torch.equal(getattr(a.arena, nme), getattr(b.arena, nme)), (what, nme)


def _seg(eng, buf, i):
    a = eng.arena
    return buf[a.offsets[i]:a.offsets[i] + a.params[i].numel()]


def _segs(eng, prefix):
    return [i for i, n in enumerate(eng.arena.names) if n.startswith(prefix)]


def _frozen_copies(eng):
    """Clones of the compute copies of every weight layer with a frozen kernel."""
    from fpnmt import layers as flayers
    out = {}
    for j, lyr in enumerate(flayers.weight_layers(eng.model)):
        if not lyr.kernel.requires_grad:
            for dt, (wf, wb) in lyr._copies.items():
                out[(j, str(dt))] = (wf.clone(), wb.clone())
    return out


def _group(m, which, **kw):
    from fpnmt import param_groups as G
    return (G.backbone_group if which == "backbone" else G.feature_extractor_group)(m, **kw)


# ------------------------------------------------------------ gradients
def test_frozen_backbone_gradients_against_the_oracle_fp32():
    """Frozen backbone, fp32, eager, rate 0: the gradient of every non-frozen
    parameter against the CPU oracle with only those tensors trainable, under
    the bars of tests/test_gpu_scst_step.py (the fp64 anchor, the fp32 oracle
    at two inputs as the noise floor); arena.grad over the frozen segments is
    exactly zero after the backward, because nothing wrote there."""
    from fpnmt.train import TrainEngine
    _require_feature()
    m, sd, cfg = _model()
    img, tok = _images(B, IMAGE, 3), _captions(B, T, VOCAB, 4, lens=[12, 5])
    eng = TrainEngine(m, 0.0, use_graph=False, param_groups=[_group(m, "backbone", frozen=True)])
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    frozen = {k for k, p in m.named_parameters() if not p.requires_grad}
    assert frozen and frozen == {k for k, _ in m.named_parameters() if k.startswith(BB)}
    w = torch.ones(B)
    l64, g64, _, _ = oracle_weighted(sd, img, tok, w, 1, cfg, trainable, torch.float64)
    l32, g32, _, _ = oracle_weighted(sd, img, tok, w, 1, cfg, trainable)
    _, g32p, _, _ = oracle_weighted(sd, _perturbed(img, 77), tok, w, 1, cfg, trainable)
    loss = float(eng.step(img.to(DEV), tok.to(DEV)))
    torch.cuda.synchronize()
    gpu = {n: p.grad.detach().cpu().double().clone() for n, p in m.named_parameters() if n in trainable}
    view = types.SimpleNamespace(named_parameters=lambda: [(n, p) for n, p in m.named_parameters()
                                                           if n in trainable])
    rows, bulk = _bars(view, g64, gpu, [g32, g32p])
    for r in sorted(rows, key=lambda r: -r[1])[:3]:
        print("grad max rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    for r in sorted(bulk, key=lambda r: -r[1])[:3]:
        print("grad p90 rel err vs fp64: gpu %.2e  cpu32 %.2e  %s" % r[1:])
    print(f"loss gpu {loss:.7f} oracle32 {float(l32):.7f} oracle64 {float(l64):.7f}")
    assert abs(loss - float(l32)) <= 1e-4 * max(1.0, abs(float(l32)))
    assert rows[0][0] <= 0.0, rows[0]
    assert bulk[0][0] <= 0.0, bulk[0]
    a = eng.arena
    idx = _segs(eng, BB)
    assert idx and idx[-1] == len(a.names) - 1  # the backbone is the arena's tail
    lo = a.offsets[idx[0]]
    assert idx == list(range(idx[0], len(a.names)))
    assert not bool(a.grad[lo:].any())
    assert float(a.grad[:lo].abs().max()) > 0


# ------------------------------------------------- eager / capture / replay
@pytest.mark.parametrize("which", ["backbone", "feature_extractor"])
def test_frozen_group_is_untouched_and_graph_is_bitwise_eager_bf16(which):
    """bf16, rate 1e-4, dropout 0.1; three steps (eager, capture, replay): the
    frozen masters and their compute copies are bitwise unchanged, every
    other segment has changed, and the result is bitwise that of an eager
    engine put through the same steps.

    "Every other segment": every one that has a gradient. At 128^2 the P7
    level is 1x1 and its head's 2x2 'valid' pool leaves nothing, so P7_conv
    and the encoder's attention over that empty view get a gradient of
    exactly zero, as do the Q / K projections of attention over a single key
    (the softmax of one score is 1 whatever the score). AMSGrad with
    m = v = 0 leaves such a tensor where it is, with or without groups: the
    set must be exactly the one of an engine without groups (pruning may
    not cost a trainable tensor its gradient), and it is listed."""
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    m_e, _, _ = _model(seed=51, rate=0.1)
    m_g, _, _ = _model(seed=51, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False, param_groups=[_group(m_e, which, frozen=True)])
        G = TrainEngine(m_g, 1e-4, use_graph=True, param_groups=[_group(m_g, which, frozen=True)])
        init = G.arena.flat.clone()
        copies = None
        has_grad = set()
        for i in range(3):
            img, tok = _batch(i)
            _sync_state(G, E)
            le, lg = E.step(img, tok).clone(), G.step(img, tok).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            _same_state(E, G, i)
            if i == 0:
                copies = _frozen_copies(G)  # built by the first step
            has_grad |= {j for j in range(len(G.arena.names)) if bool(_seg(G, G.arena.grad, j).any())}
        assert G.graphs is not None and int(G.arena.step) == 3
        pre = BB if which == "backbone" else FE
        frozen = set(_segs(G, pre))
        assert frozen and all(not G.arena.params[i].requires_grad for i in frozen)
        assert not (frozen & has_grad)  # nothing wrote a frozen segment's gradient
        unchanged = []
        for i, n in enumerate(G.arena.names):
            same = torch.equal(_seg(G, G.arena.flat, i), _seg(G, init, i))
            if i in frozen:
                assert same, n
                for buf in (G.arena.m, G.arena.v, G.arena.vhat):
                    assert not bool(_seg(G, buf, i).any()), n
            else:
                assert same == (i not in has_grad), (n, same)
                if same:
                    unchanged.append(n)
        print("trainable segments without a gradient, which did not move:", unchanged)
        m_n, _, _ = _model(seed=51, rate=0.1)
        fpnmt.set_precision("bf16")
        N = TrainEngine(m_n, 1e-4, use_graph=False)
        assert N.arena.names == G.arena.names
        N.step(*_batch(0))
        torch.cuda.synchronize()
        plain = [n for j, n in enumerate(N.arena.names) if j not in frozen and not bool(_seg(N, N.arena.grad, j).any())]
        assert unchanged == plain, (unchanged, plain)
        after = _frozen_copies(G)
        assert copies and copies.keys() == after.keys()
        for k in copies:
            assert torch.equal(copies[k][0], after[k][0]) and torch.equal(copies[k][1], after[k][1]), k
    finally:
        fpnmt.set_precision("fp32")


def test_group_values_change_between_replays_without_recapture():
    """Backbone lr_scale = 0.1 and weight_decay = 0.01 on matrices, set between
    two replays: the graph objects are the same ones, and the arena is
    bitwise that of an eager engine given the same values at the same step."""
    import fpnmt
    from fpnmt import param_groups as PG
    from fpnmt.train import TrainEngine
    _require_feature()
    m_e, _, _ = _model(seed=52, rate=0.1)
    m_g, _, _ = _model(seed=52, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False, param_groups=[_group(m_e, "backbone")])
        G = TrainEngine(m_g, 1e-4, use_graph=True, param_groups=[_group(m_g, "backbone")])
        graphs = None
        moved = {}
        for i in range(5):
            if i == 3:
                assert G.graphs is not None
                graphs = G.graphs
                for eng in (E, G):
                    eng.set_lr_scale("backbone", 0.1)
                    eng.set_weight_decay("backbone", PG.decay_matrices(0.01))
            img, tok = _batch(i)
            _sync_state(G, E)
            p0 = G.arena.flat.clone()
            le, lg = E.step(img, tok).clone(), G.step(img, tok).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), i
            _same_state(E, G, i)
            bb = _segs(G, BB)
            lo = G.arena.offsets[bb[0]]
            moved[i] = float((G.arena.flat[lo:] - p0[lo:]).abs().mean())
        assert G.graphs is graphs and all(a is b for a, b in zip(G.graphs, graphs))  # no recapture
        print("backbone mean |update| per step:", moved)
        # AMSGrad's first steps move every element by ~lr: a tenth of the rate shows
        assert moved[3] < 0.5 * moved[2]
        tab = G.seg_groups.table.cpu()
        for i in _segs(G, BB):
            assert float(tab.view(torch.float32)[i, 0]) == pytest.approx(0.1)
            want = 0.01 if G.arena.params[i].ndim >= 2 else 0.0
            assert float(tab.view(torch.float32)[i, 1]) == pytest.approx(want)
    finally:
        fpnmt.set_precision("fp32")


def test_freeze_and_unfreeze_at_run_time():
    """set_frozen("backbone", True) then False: the step graphs are dropped
    and rebuilt each time, the backbone stands still while frozen and moves
    again afterwards, the whole trajectory is bitwise an eager engine's, and
    the eval graphs are not rebuilt."""
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    m_e, _, _ = _model(seed=53, rate=0.1)
    m_g, _, _ = _model(seed=53, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False, param_groups=[_group(m_e, "backbone")])
        G = TrainEngine(m_g, 1e-4, use_graph=True, param_groups=[_group(m_g, "backbone")])
        img, tok = _batch(9)
        for _ in range(3):
            G.eval_step(img, tok)
        (ekey, eent), = G._esteps.items()
        egraph = eent[1]
        assert egraph is not None
        lo = G.arena.offsets[_segs(G, BB)[0]]
        seen = []
        for phase, frozen in enumerate((False, True, False)):
            if phase:
                for eng in (E, G):
                    eng.set_frozen("backbone", frozen)
                assert G.graphs is None and G._wsteps == {}
                assert all(p.requires_grad != frozen for n, p in m_g.named_parameters() if n.startswith(BB))
            for k in range(3):
                i = 3 * phase + k
                img, tok = _batch(i)
                _sync_state(G, E)
                p0 = G.arena.flat.clone()
                le, lg = E.step(img, tok).clone(), G.step(img, tok).clone()
                torch.cuda.synchronize()
                assert torch.equal(le, lg), i
                _same_state(E, G, i)
                moved = not torch.equal(G.arena.flat[lo:], p0[lo:])
                assert moved != frozen, (i, frozen)
                assert not torch.equal(G.arena.flat[:lo], p0[:lo])
                assert (G.graphs is not None) == (k >= 1), (i, k)  # eager, then capture, then replay
            seen.append(G.graphs)
        assert seen[0] is not seen[1] and seen[1] is not seen[2]
        assert int(G.arena.step) == 9
        out = G.eval_step(img, tok)
        assert G._esteps[ekey][1] is egraph and len(G._esteps) == 1
        assert torch.isfinite(out["loss"])
    finally:
        fpnmt.set_precision("fp32")


def test_three_ways_of_saying_no_groups_are_bitwise_equal():
    """param_groups=None, [] and one explicit all-default group end three
    steps (eager, capture, replay) bitwise equal."""
    import fpnmt
    from fpnmt import param_groups as PG
    from fpnmt.train import TrainEngine
    _require_feature()
    fpnmt.set_precision("bf16")
    try:
        ends = []
        for make in (lambda m: None, lambda m: [], lambda m: [PG.ParamGroup("all", lambda n, p: True)]):
            m, _, _ = _model(seed=54, rate=0.1)
            fpnmt.set_precision("bf16")
            eng = TrainEngine(m, 1e-4, use_graph=True, param_groups=make(m))
            losses = [eng.step(*_batch(i)).clone() for i in range(3)]
            torch.cuda.synchronize()
            ends.append((losses, {nme: getattr(eng.arena, nme).clone() for nme in STATE}))
        assert ends[0][1]["flat"].abs().sum() > 0
        for other in ends[1:]:
            for a, b in zip(ends[0][0], other[0]):
                assert torch.equal(a, b)
            for nme in STATE:
                assert torch.equal(ends[0][1][nme], other[1][nme]), nme
    finally:
        fpnmt.set_precision("fp32")


def test_early_update_and_overlapped_zeroing_with_groups_are_bitwise_the_plain_update():
    """config.early_update (the transformer's part of the optimizer from
    inside the backward, the rest at the end) and config.zero_grad_overlap_grid
    with groups: the same table in every part, the one-launch update's losses,
    weights and state bit for bit over eager, captured and replayed steps. The
    groups give the early part work of its own (scale and decay on the
    transformer) and trim the late part (backbone frozen)."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt import param_groups as PG
    from fpnmt.train import TrainEngine
    _require_feature()
    fpnmt.set_precision("bf16")
    res, fired = {}, {}
    try:
        for mode in ("plain", "early", "zero"):
            fpnmt.config.early_update = mode == "early"
            fpnmt.config.zero_grad_overlap_grid = 7 if mode == "zero" else 0
            m, _, _ = _model(seed=59, rate=0.1)
            fpnmt.set_precision("bf16")
            groups = [PG.backbone_group(m, frozen=True),
                      PG.ParamGroup("decoder", ("decoder.",), lr_scale=3.0, weight_decay=PG.decay_matrices(0.01))]
            eng = TrainEngine(m, 1e-4, use_graph=True, param_groups=groups)
            assert 0 < eng.early_blocks < eng.arena.nblocks
            calls = []
            orig = eng._early_update
            eng._early_update = lambda: (calls.append(1), orig())
            losses = [eng.step(*_batch(i)).clone() for i in range(3)]
            torch.cuda.synchronize()
            fired[mode] = len(calls)
            res[mode] = (torch.stack(losses), {nme: getattr(eng.arena, nme).clone() for nme in STATE})
            del eng, m
            flayers.invalidate_weights()
    finally:
        fpnmt.config.early_update = False
        fpnmt.config.zero_grad_overlap_grid = 0
        fpnmt.set_precision("fp32")
    assert fired == {"plain": 0, "early": 2, "zero": 0}, fired  # the eager step and the capture run the callback
    for mode in ("early", "zero"):
        assert torch.equal(res["plain"][0], res[mode][0]), mode
        for nme in STATE:
            assert torch.equal(res["plain"][1][nme], res[mode][1][nme]), (mode, nme)


def test_step_weighted_with_frozen_backbone_graph_is_bitwise_eager():
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    n = 2
    m_e, _, _ = _model(seed=55, rate=0.1)
    m_g, _, _ = _model(seed=55, rate=0.1)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False, param_groups=[_group(m_e, "backbone", frozen=True)])
        G = TrainEngine(m_g, 1e-4, use_graph=True, param_groups=[_group(m_g, "backbone", frozen=True)])
        init = G.arena.flat.clone()
        g = torch.Generator().manual_seed(90)
        for i in range(3):
            img, tok = _batch(i, n=n)
            w = (torch.randn(B * n, generator=g) * 1.5).to(DEV)
            _sync_state(G, E)
            le, lg = E.step_weighted(img, tok, w).clone(), G.step_weighted(img, tok, w).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), i
            _same_state(E, G, i)
        assert next(iter(G._wsteps.values()))[1] is not None  # captured, then replayed
        lo = G.arena.offsets[_segs(G, BB)[0]]
        assert torch.equal(G.arena.flat[lo:], init[lo:])
        assert not torch.equal(G.arena.flat[:lo], init[:lo])
    finally:
        fpnmt.set_precision("fp32")


def test_split_backward_with_frozen_backbone_matches_single_graph():
    """split_backward=True with the backbone frozen against the single-graph
    step, one step at a time from identical state, bitwise; the frozen
    stages have no graph."""
    from fpnmt.train import TrainEngine
    _require_feature()
    m_a, _, _ = _model(seed=12)
    m_b, _, _ = _model(seed=12)
    A = TrainEngine(m_a, 1e-6, use_graph=True, param_groups=[_group(m_a, "backbone", frozen=True)])
    S = TrainEngine(m_b, 1e-6, use_graph=True, split_backward=True,
                    param_groups=[_group(m_b, "backbone", frozen=True)])
    assert S.split and not A.split and A.arena.names == S.arena.names
    img, tok = _batch(0)
    fails = []
    for i in range(4):
        if i:
            _sync_state(S, A)
        p0 = A.arena.flat.detach().clone()
        la, lb = A.step(img, tok).clone(), S.step(img, tok).clone()
        torch.cuda.synchronize()
        da, db = A.arena.flat - p0, S.arena.flat - p0
        upd, err = float(da.abs().mean()), float((da - db).abs().mean())
        print(f"step {i}: loss {float(la):.7f} / {float(lb):.7f}; mean |update| {upd:.3e}, "
              f"mean |d update| {err:.3e}, elements that differ {int((da != db).sum())}")
        assert upd > 0
        if not (torch.equal(la, lb) and all(torch.equal(getattr(A.arena, k), getattr(S.arena, k)) for k in STATE)):
            fails.append(i)
    g1, g2, *stages, g3 = S.graphs
    assert len(stages) == 5
    assert all(g is not None for g in stages[:2])  # heads, FPN
    assert all(g is None for g in stages[2:])  # the backbone's three stages: no graph
    assert not fails, fails


# ------------------------------------------------------------ MobileNetV2
def test_mobilenet_frozen_backbone_runs_batchnorm_in_inference_mode():
    """A frozen MobileNetV2 backbone: moving_mean and moving_variance are
    bitwise unchanged after a step, and the train-step forward of the feature
    extractor equals the inference-mode forward."""
    from fpnmt.layers import BatchNormalization
    from fpnmt.train import TrainEngine
    _require_feature()
    m, _, _ = _model(seed=56, backbone="mobilenet224_1.0")
    bns = [mod for mod in m.modules() if isinstance(mod, BatchNormalization)]
    assert bns
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # statistics unlike a fresh layer's, so the two modes differ
        for bn in bns:
            bn.moving_mean.copy_((torch.randn(bn.moving_mean.shape, generator=g) * 0.1).to(DEV))
            bn.moving_variance.copy_((torch.rand(bn.moving_variance.shape, generator=g) + 0.5).to(DEV))
    stats = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in bns]
    eng = TrainEngine(m, 1e-4, use_graph=False, param_groups=[_group(m, "backbone", frozen=True)])
    fe = m.encoder.feature_extractor
    assert fe.freeze_backbone_bn
    img, tok = _batch(0)
    init = eng.arena.flat.clone()
    eng.step(img, tok)
    torch.cuda.synchronize()
    for bn, (mean, var) in zip(bns, stats):
        assert torch.equal(bn.moving_mean, mean) and torch.equal(bn.moving_variance, var)
    lo = eng.arena.offsets[_segs(eng, BB)[0]]
    assert torch.equal(eng.arena.flat[lo:], init[lo:]) and not torch.equal(eng.arena.flat[:lo], init[:lo])
    with torch.no_grad():
        train = fe(img, training=True)
        infer = fe(img, training=False)
        eng.set_frozen("backbone", False)
        batch_stats = fe(img, training=True)
    for a, b in zip(train, infer):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(batch_stats, infer))  # the modes do differ
    for bn, (mean, var) in zip(bns, stats):
        assert not torch.equal(bn.moving_mean, mean)  # unfrozen: the averages move again


# ----------------------------------------------------------------- world 2
def _dp_worker(rank, world, port, out_dir):
    import test_gpu_dp_step as D
    D._paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        import fpnmt
        from fpnmt import dist as fd
        from fpnmt import param_groups as PG
        from fpnmt.train import TrainEngine
        import test_gpu_model as TM
        m, _, _ = TM._build(num_layers=1, vocab=VOCAB, image=IMAGE, max_seq_len=T, seed=17)
        fpnmt.set_precision("fp32")
        eng = TrainEngine(m, 1e-5, use_graph=True, param_groups=[PG.backbone_group(m, frozen=True)])
        calls = []
        real = fd.allreduce_flat

        def counted(flat, *a, **k):
            calls.append((int(flat.data_ptr() - eng.arena.grad.data_ptr()) // 4, int(flat.numel())))
            return real(flat, *a, **k)
        fd.allreduce_flat = counted
        init = eng.arena.flat.detach().cpu().clone()
        img = _images(2 * B, IMAGE, 23)[rank * B:(rank + 1) * B].cuda()
        tok = _captions(2 * B, T, VOCAB, 24, lens=[12, 5, 9, 12])[rank * B:(rank + 1) * B].cuda()
        per_step = []
        for _ in range(3):
            calls.clear()
            eng.step(img, tok)
            torch.cuda.synchronize()
            per_step.append(list(calls))
        a = eng.arena
        bb = [i for i, n in enumerate(a.names) if n.startswith(BB)]
        torch.save({"flat": a.flat.detach().cpu(), "init": init, "calls": per_step, "ranges": eng.ranges,
                    "split": eng.split, "world": eng.world, "bb_lo": a.offsets[bb[0]],
                    "graphs": [g is not None for g in eng.graphs]}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp_world2_frozen_backbone(tmp_path):
    """Two gloo ranks (as tests/test_gpu_dp_step.py sets them up), backbone
    frozen: both ranks end with identical arenas, the frozen ranges are
    unchanged, and no all-reduce is issued for a wholly frozen range."""
    import torch.multiprocessing as mp
    import test_gpu_dp_step as D
    _require_feature()
    ctx = mp.get_context("spawn")
    port = D._free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=500)
        assert p.exitcode == 0, p.exitcode
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(2)]
    assert res[0]["split"] and res[0]["world"] == 2
    assert torch.equal(res[0]["flat"], res[1]["flat"])
    lo = res[0]["bb_lo"]
    assert torch.equal(res[0]["flat"][lo:], res[0]["init"][lo:])
    assert not torch.equal(res[0]["flat"][:lo], res[0]["init"][:lo])
    ranges = res[0]["ranges"]
    live = [(a, b - a) for a, b in ranges[:4]]  # decoder side, encoder layers, heads, FPN
    frozen = [(a, b - a) for a, b in ranges[4:] if b > a]  # the backbone's stages
    assert len(frozen) == 3 and all(a >= lo for a, _ in frozen)
    for r in res:
        for step_calls in r["calls"]:
            assert sorted(step_calls) == sorted(live), (step_calls, live)
        assert r["graphs"] == [True, True, True, True, False, False, False, True]


# -------------------------------------------------------------- checkpoint
def test_checkpoint_saved_frozen_restores_into_an_engine_without_groups(tmp_path):
    from fpnmt.checkpoint import Checkpoint
    from fpnmt.train import TrainEngine
    _require_feature()
    m_a, _, _ = _model(seed=57)
    m_b, _, _ = _model(seed=58)
    A = TrainEngine(m_a, 1e-4, use_graph=False, param_groups=[_group(m_a, "backbone", frozen=True)])
    for i in range(2):
        A.step(*_batch(i))
    path = str(tmp_path / "ckpt.safetensors")
    Checkpoint(transformer=m_a, optimizer=A).write(path)
    Bn = TrainEngine(m_b, 1e-4, use_graph=False)
    assert Bn.arena.names == A.arena.names  # one arena layout across groupings
    assert not torch.equal(Bn.arena.flat, A.arena.flat)
    Checkpoint(transformer=m_b, optimizer=Bn).restore(path)
    torch.cuda.synchronize()
    _same_state(A, Bn, "restore")
    assert int(Bn.arena.step) == 2
    # and the restored engine trains on, backbone included
    p0 = Bn.arena.flat.clone()
    Bn.step(*_batch(2))
    torch.cuda.synchronize()
    lo = Bn.arena.offsets[_segs(Bn, BB)[0]]
    assert not torch.equal(Bn.arena.flat[lo:], p0[lo:])


# ---------------------------------------------------------------- Pipeline
def test_pipeline_keywords_build_the_groups():
    """Pipeline(freeze=, backbone_lr_scale=, weight_decay=): the groups of
    param_groups.recipe_groups; train_step, eval_step and the engine's
    setters work under them."""
    from fpnmt import param_groups as PG
    from utils.pipeline import Pipeline
    _require_feature()
    assert "freeze" in inspect.signature(Pipeline.__init__).parameters
    kw = dict(max_seq_len=T, target_vocab_size=VOCAB, image_size=IMAGE, n_layers=1, backbone="resnet50", rate=0.0)
    with pytest.raises(ValueError, match="not both"):
        Pipeline(param_groups=[], freeze=("backbone",), **kw)
    with pytest.raises(ValueError, match="freeze"):
        Pipeline(freeze=("decoder",), **kw)
    pl = Pipeline(freeze=("backbone",), backbone_lr_scale=0.1, weight_decay=0.01, **kw)
    eng = pl.engine
    assert [g.name for g in eng.param_groups] == ["backbone", "feature_extractor", "transformer"]
    bb = _segs(eng, BB)
    sg = eng.seg_groups
    assert all(sg.frozen[i] for i in bb) and not any(sg.frozen[i] for i in range(bb[0]))
    assert all(sg.lr_scale[i] == 0.1 for i in bb) and all(sg.lr_scale[i] == 1.0 for i in range(bb[0]))
    assert all(sg.weight_decay[i] == (0.01 if p.ndim >= 2 else 0.0) for i, p in enumerate(eng.arena.params))
    init = eng.arena.flat.clone()
    lo = eng.arena.offsets[bb[0]]
    img, tok = _batch(0)
    for _ in range(3):
        loss = pl.train_step(img, tok)
    out = pl.eval_step(img, tok)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(out["loss"])
    assert torch.equal(eng.arena.flat[lo:], init[lo:]) and not torch.equal(eng.arena.flat[:lo], init[:lo])
    eng.set_frozen("backbone", False)
    eng.set_weight_decay("backbone", PG.decay_matrices(0.0))
    pl.train_step(img, tok)
    torch.cuda.synchronize()
    assert not torch.equal(eng.arena.flat[lo:], init[lo:])
    with pytest.raises(ValueError, match="no parameter group"):
        eng.set_lr_scale("cnn", 0.5)
    with pytest.raises(ValueError):
        eng.set_lr_scale("backbone", -1.0)

"""Weight averaging in the training step (TrainEngine(ema_decay=...)): the
average kept by the optimizer kernel changes nothing else, is the same eager,
captured and replayed, through the early update, with a frozen group and in
step_weighted; ema_weights() puts it under the model exactly and takes it out
again; decoding, checkpoints, the live setters and the data-parallel form.

Model: tests/test_gpu_param_groups_step.py's (_model: one layer, ResNet-50,
vocab 300, 128 x 128 images, max_seq_len 12, dropout 0), B = 2."""
import inspect
import os

import pytest
import torch

from test_gpu_param_groups_step import BB, B, IMAGE, T, VOCAB, _batch, _group, _model, _seg, _segs

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("flat", "m", "v", "vhat", "step")
DECAY = 0.99


def _require_feature():
    from fpnmt.train import TrainEngine
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert "ema_decay" in sig and "ema_debias" in sig, "TrainEngine has no ema_decay argument"
    assert hasattr(TrainEngine, "ema_weights") and hasattr(TrainEngine, "set_ema_decay")


def _snapshot(eng, losses):
    a = eng.arena
    out = {k: getattr(a, k).clone() for k in STATE}
    out["ema"] = a.ema.clone() if a.ema is not None else None
    out["loss"] = torch.stack([x.reshape(()) for x in losses]) if losses else torch.empty(0, device=DEV)
    return out


def _run(seed, ema, graph, steps=3, weighted=False, groups=None, lr=1e-4, **kw):
    """A fresh model and engine, `steps` steps in bf16; the final state."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    m, _, _ = _model(seed=seed)
    fpnmt.set_precision("bf16")
    pg = [_group(m, groups, frozen=True)] if groups else None
    eng = TrainEngine(m, lr, use_graph=graph, param_groups=pg, ema_decay=DECAY if ema else None, **kw)
    init = eng.arena.flat.clone()
    losses = []
    g = torch.Generator().manual_seed(90)
    for i in range(steps):
        if weighted:
            img, tok = _batch(i, n=2)
            w = (torch.randn(B * 2, generator=g) * 1.5).to(DEV)
            losses.append(eng.step_weighted(img, tok, w).clone())
        else:
            losses.append(eng.step(*_batch(i)).clone())
    torch.cuda.synchronize()
    if graph:
        captured = next(iter(eng._wsteps.values()))[1] if weighted else eng.graphs
        assert captured is not None
    out = _snapshot(eng, losses)
    out["init"], out["eng"] = init, eng
    flayers.invalidate_weights()
    return out


def _same(a, b, what, ema=True):
    for k in STATE + ("loss",) + (("ema",) if ema else ()):
        assert torch.equal(a[k], b[k]), (what, k)


def _three(seed, **kw):
    """The same three steps by a graph engine without the average, an eager
    one with it and a graph one with it."""
    import fpnmt
    try:
        return (_run(seed, False, True, **kw), _run(seed, True, False, **kw), _run(seed, True, True, **kw))
    finally:
        fpnmt.set_precision("fp32")


def _check_three(P, E, G):
    _same(P, G, "the average changes nothing else", ema=False)
    _same(E, G, "graph replay against eager")
    assert int(G["step"]) == 3
    assert P["ema"] is None and not torch.equal(G["ema"], G["flat"]) and not torch.equal(G["ema"], G["init"])
    assert not torch.isnan(G["ema"]).any()


@pytest.fixture(scope="module")
def base():
    _require_feature()
    return _three(61)


def test_average_changes_nothing_else_and_graph_equals_eager(base):
    """Three steps (eager, capture, replay), bf16 with the fused compute-copy
    refresh: flat, m, v, vhat, the step counter and the losses of the engine
    with ema_decay=0.99 are bitwise those of the engine without; the average
    after graph replay is bitwise the eager run's."""
    P, E, G = base
    _check_three(P, E, G)


def test_early_update_and_overlapped_zeroing_keep_the_average_bitwise(base):
    """config.early_update (the transformer's segments from inside the
    backward on a persistent grid, the rest at the end: two launches of
    fpnmt_amsgrad_step_ema per step) and zero_grad_overlap_grid > 0: state,
    losses and the average are bitwise the one-launch step's."""
    import fpnmt
    _require_feature()
    fpnmt.config.early_update = True
    fpnmt.config.zero_grad_overlap_grid = 7
    calls = []
    try:
        import fpnmt.train as FT
        orig = FT.TrainEngine._early_update

        def counted(self):
            calls.append(1)
            return orig(self)
        FT.TrainEngine._early_update = counted
        try:
            R = _run(61, True, True)
        finally:
            FT.TrainEngine._early_update = orig
    finally:
        fpnmt.config.early_update = False
        fpnmt.config.zero_grad_overlap_grid = 0
        fpnmt.set_precision("fp32")
    assert len(calls) == 2, calls  # the eager step and the capture run the callback
    assert 0 < R["eng"].early_blocks < R["eng"].arena.nblocks
    _same(base[2], R, "early update")


def test_frozen_backbone_group_keeps_its_average():
    """With a frozen backbone group: the same three equalities, and the
    frozen segments' average is bitwise the initial parameters."""
    _require_feature()
    P, E, G = _three(62, groups="backbone")
    _check_three(P, E, G)
    eng = G["eng"]
    idx = _segs(eng, BB)
    assert idx and all(eng.seg_groups.frozen[i] for i in idx)
    for i in idx:
        assert torch.equal(_seg(eng, G["ema"], i), _seg(eng, G["init"], i)), eng.arena.names[i]
    lo = eng.arena.offsets[idx[0]]
    assert not torch.equal(G["ema"][:lo], G["init"][:lo])


def test_step_weighted_keeps_the_average():
    _require_feature()
    _check_three(*_three(63, weighted=True))


# ------------------------------------------------------- the context manager
def _second_engine(seed, src, tensors):
    """A second model (same seed: same buffers) whose parameters are set by
    hand to `tensors` (an arena of src's layout), with a plain eager engine."""
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    m2, _, _ = _model(seed=seed)
    e2 = TrainEngine(m2, 1e-4, use_graph=False)
    assert e2.arena.names == src.arena.names and e2.arena.ema is None
    with torch.no_grad():
        for p, o in zip(e2.arena.params, e2.arena.offsets):
            p.copy_(tensors[o:o + p.numel()].view(p.shape))
    flayers.invalidate_weights()
    return e2


def test_ema_weights_context_is_exact():
    """bf16, graphs. Inside ema_weights() the replayed eval graph gives,
    bitwise, the outputs of a second model holding the averaged tensors; step
    and step_weighted raise; after exit the arena and eval_step are bitwise
    what they were, on the same eval graph, and training goes on as in an
    engine that never opened the context."""
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    keys = ("loss", "caption_logp", "caption_len", "caption_hit", "totals")
    m, _, _ = _model(seed=64)
    m_n, _, _ = _model(seed=64)
    fpnmt.set_precision("bf16")
    try:
        G = TrainEngine(m, 1e-3, use_graph=True, ema_decay=0.5, ema_debias=False)
        N = TrainEngine(m_n, 1e-3, use_graph=True, ema_decay=0.5, ema_debias=False)  # never opens the context
        for i in range(3):
            G.step(*_batch(i))
            N.step(*_batch(i))
        img, tok = _batch(7)
        for _ in range(3):  # eager, capture, replay
            out_model = {k: v.clone() for k, v in G.eval_step(img, tok).items()}
        (ekey, eent), = G._esteps.items()
        egraph = eent[1]
        assert egraph is not None
        before = _snapshot(G, [])
        where = [p.data_ptr() for p in G.arena.params]
        with G.ema_weights() as inside:
            assert inside is G
            assert torch.equal(G.arena.flat, before["ema"]) and torch.equal(G.arena.ema, before["flat"])
            out_ema = {k: v.clone() for k, v in G.eval_step(img, tok).items()}
            assert G._esteps[ekey][1] is egraph and len(G._esteps) == 1
            with pytest.raises(RuntimeError, match="ema_weights"):
                G.step(*_batch(3))
            with pytest.raises(RuntimeError, match="ema_weights"):
                G.step_weighted(img, tok, torch.ones(B, device=DEV))
            with pytest.raises(RuntimeError):
                with G.ema_weights():
                    pass
            with pytest.raises(RuntimeError):
                G.reset_ema()
        torch.cuda.synchronize()
        after = _snapshot(G, [])
        for k in STATE + ("ema",):
            assert torch.equal(before[k], after[k]), k
        assert where == [p.data_ptr() for p in G.arena.params]
        out_back = G.eval_step(img, tok)
        assert G._esteps[ekey][1] is egraph
        for k in keys:
            assert torch.equal(out_back[k], out_model[k]), k
        assert not torch.equal(out_ema["caption_logp"], out_model["caption_logp"])  # the two sets of weights differ
        # an exception inside still puts the weights back
        with pytest.raises(KeyError):
            with G.ema_weights():
                raise KeyError("x")
        assert torch.equal(G.arena.flat, before["flat"]) and not G._ema_open
        # the second model, by hand
        e2 = _second_engine(64, G, before["ema"])
        fpnmt.set_precision("bf16")  # building a model resets it to fp32
        out2 = e2.eval_step(img, tok)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out_ema[k], out2[k]), k
        # training goes on from the same state
        lg, ln = G.step(*_batch(3)).clone(), N.step(*_batch(3)).clone()
        torch.cuda.synchronize()
        assert torch.equal(lg, ln)
        for k in STATE + ("ema",):
            assert torch.equal(getattr(G.arena, k), getattr(N.arena, k)), k
    finally:
        fpnmt.set_precision("fp32")


def test_engine_without_ema_refuses_the_ema_calls():
    from fpnmt.train import TrainEngine
    _require_feature()
    m, _, _ = _model(seed=65)
    eng = TrainEngine(m, 1e-4, use_graph=False)
    assert eng.arena.ema is None and eng.ema_decay is None
    for call in (lambda: eng.set_ema_decay(0.5), eng.reset_ema, lambda: eng.ema_weights().__enter__()):
        with pytest.raises(ValueError, match="ema_decay"):
            call()


# ------------------------------------------------ decoding and checkpoints
def _pipe(seed, **kw):
    from fpnmt.layers import Init, invalidate_weights
    from utils.pipeline import Pipeline
    pl = Pipeline(max_seq_len=T, target_vocab_size=VOCAB, image_size=IMAGE, n_layers=1, rate=0.0,
                  init=Init(torch.Generator().manual_seed(seed)), **kw)
    with torch.no_grad():
        pl.transformer.final_layer.bias[pl.end_token] += 3.0  # random weights would never end a caption
    invalidate_weights()
    return pl


def test_predict_batch_and_export_on_the_averaged_weights(tmp_path):
    """fp32. predict_batch(weights="ema") gives the ids of a second pipeline
    whose parameters were set to the averaged tensors by hand, in mode="beam"
    and in the reference mode, through decode graphs captured on the model's
    own weights; weights="model" is unchanged before and after. The average
    is then edited by hand so that the two sets of weights caption
    differently. export_ema's file, restored by a plain Pipeline, reproduces
    the ids; eval_step / score_captions / validate follow the same switch."""
    import fpnmt
    from fpnmt.layers import invalidate_weights
    _require_feature()
    fpnmt.set_precision("fp32")
    pl = _pipe(66, ema_decay=DECAY)
    eng = pl.engine
    for i in range(2):
        pl.train_step(*_batch(i))
    a = eng.arena
    with torch.no_grad():  # an average that captions differently: noise, and token 7 favoured
        g = torch.Generator().manual_seed(5)
        a.ema.mul_(1.0 + 0.05 * torch.randn(a.total, generator=g).to(DEV))
        i = a.names.index("final_layer.bias")
        a.ema[a.offsets[i] + 7] += 4.0
    imgs = _batch(11)[0]
    modes = (dict(mode="beam", beam_n=3), dict(mode="reference", beam_n=3))
    ids_model = [pl.predict_batch(imgs, T, **kw) for kw in modes]  # captures the decode graphs
    ids_ema = [pl.predict_batch(imgs, T, weights="ema", **kw) for kw in modes]
    assert [pl.predict_batch(imgs, T, **kw) for kw in modes] == ids_model
    assert not eng._ema_open
    assert ids_ema != ids_model, (ids_ema, ids_model)
    # the second model, by hand
    pl2 = _pipe(66)
    assert pl2.engine.arena.names == a.names
    with torch.no_grad():
        for p, o in zip(pl2.engine.arena.params, a.offsets):
            p.copy_(a.ema[o:o + p.numel()].view(p.shape))
    invalidate_weights()
    assert [pl2.predict_batch(imgs, T, **kw) for kw in modes] == ids_ema
    img, tok = _batch(12)
    want = {k: v.clone() for k, v in pl2.eval_step(img, tok).items()}
    got = pl.eval_step(img, tok, weights="ema")
    for k in ("loss", "caption_logp", "caption_len", "caption_hit"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(pl.eval_step(img, tok)["caption_logp"], want["caption_logp"])
    caps = [[5, 6, 7], [8, 9]]
    assert pl.score_captions(imgs, caps, weights="ema") == pl2.score_captions(imgs, caps)
    assert pl.validate([(img, tok)], weights="ema")["token_nll"] == pl2.validate([(img, tok)])["token_nll"]
    # export_ema: a model-only file any Pipeline loads
    path = str(tmp_path / "ema.safetensors")
    pl.ckpt.export_ema(path)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        assert not [k for k in f.keys() if not k.startswith("model/")]
    pl3 = _pipe(67)
    pl3.ckpt.restore(path)
    assert [pl3.predict_batch(imgs, T, **kw) for kw in modes] == ids_ema
    with pytest.raises(ValueError, match="ema_decay"):
        pl3.predict_batch(imgs, T, weights="ema")
    with pytest.raises(ValueError, match="ema_decay"):
        pl3.eval_step(img, tok, weights="ema")
    with pytest.raises(ValueError, match="weights"):
        pl.predict_batch(imgs, T, weights="average")
    with pytest.raises(ValueError):
        pl3.ckpt.export_ema(path)


def test_checkpoint_round_trip_continues_bitwise(tmp_path):
    """Save after two steps, restore into a fresh averaging engine (another
    seed), two more steps: bitwise the uninterrupted run, average included
    (the debias term follows the restored step counter)."""
    from fpnmt.checkpoint import Checkpoint
    from fpnmt.train import TrainEngine
    _require_feature()
    m_a, _, _ = _model(seed=68)
    m_b, _, _ = _model(seed=69)
    A = TrainEngine(m_a, 1e-4, use_graph=False, ema_decay=DECAY)
    for i in range(2):
        A.step(*_batch(i))
    path = str(tmp_path / "ckpt.safetensors")
    Checkpoint(transformer=m_a, optimizer=A).write(path)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        keys = set(f.keys())
        assert (f.metadata() or {}).get("format") == "fpnmt-ckpt-v1"
    assert {f"optimizer/ema/{n}" for n in A.arena.names} <= keys
    Bn = TrainEngine(m_b, 1e-4, use_graph=False, ema_decay=DECAY)
    assert not torch.equal(Bn.arena.flat, A.arena.flat)
    Checkpoint(transformer=m_b, optimizer=Bn).restore(path)
    torch.cuda.synchronize()
    for k in STATE + ("ema",):
        assert torch.equal(getattr(A.arena, k), getattr(Bn.arena, k)), k
    assert not torch.equal(A.arena.ema, A.arena.flat)
    for i in range(2, 4):
        la, lb = A.step(*_batch(i)).clone(), Bn.step(*_batch(i)).clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), i
    for k in STATE + ("ema",):
        assert torch.equal(getattr(A.arena, k), getattr(Bn.arena, k)), k
    assert int(Bn.arena.step) == 4


def test_checkpoint_compatibility_both_ways(tmp_path):
    """A checkpoint without ema keys into an averaging engine: the average
    starts at the restored parameters. One with them into a plain engine:
    they are ignored."""
    from fpnmt.checkpoint import Checkpoint
    from fpnmt.train import TrainEngine
    _require_feature()
    m_p, _, _ = _model(seed=70)
    m_e, _, _ = _model(seed=71)
    Pn = TrainEngine(m_p, 1e-4, use_graph=False)
    E = TrainEngine(m_e, 1e-4, use_graph=False, ema_decay=DECAY)
    for i in range(2):
        Pn.step(*_batch(i))
        E.step(*_batch(i))
    torch.cuda.synchronize()
    plain, with_ema = str(tmp_path / "plain.safetensors"), str(tmp_path / "ema.safetensors")
    Checkpoint(transformer=m_p, optimizer=Pn).write(plain)
    Checkpoint(transformer=m_e, optimizer=E).write(with_ema)
    want_p = {k: getattr(Pn.arena, k).clone() for k in STATE}
    want_e = {k: getattr(E.arena, k).clone() for k in STATE}
    assert not torch.equal(want_p["flat"], want_e["flat"]) and not torch.equal(E.arena.ema, E.arena.flat)
    Checkpoint(transformer=m_e, optimizer=E).restore(plain)  # no ema keys -> average = restored parameters
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(E.arena, k), want_p[k]), k
    assert torch.equal(E.arena.ema, E.arena.flat)
    Checkpoint(transformer=m_p, optimizer=Pn).restore(with_ema)  # ema keys ignored
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(Pn.arena, k), want_e[k]), k
    assert Pn.arena.ema is None
    loss = Pn.step(*_batch(2))
    assert torch.isfinite(loss)


# ------------------------------------------------------------- live setters
def test_set_ema_decay_and_reset_ema_between_replays():
    """After capture: set_ema_decay and reset_ema keep engine.graphs the same
    object, and the next replay shows the effect, bitwise that of an eager
    engine given the same calls. debias off, so the decay is the weight."""
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    m_e, _, _ = _model(seed=72)
    m_g, _, _ = _model(seed=72)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-3, use_graph=False, ema_decay=DECAY, ema_debias=False)
        G = TrainEngine(m_g, 1e-3, use_graph=True, ema_decay=DECAY, ema_debias=False)
        desc = G.arena.ema_desc.table.data_ptr()
        graphs = None
        for i in range(6):
            if i == 3:
                graphs = G.graphs
                assert graphs is not None
                for eng in (E, G):
                    eng.set_ema_decay(0.5)
                assert G.ema_decay == 0.5
            if i == 4:
                for eng in (E, G):
                    eng.reset_ema()
                assert torch.equal(G.arena.ema, G.arena.flat)
            old = G.arena.ema.clone()
            le, lg = E.step(*_batch(i)).clone(), G.step(*_batch(i)).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), i
            for k in STATE + ("ema",):
                assert torch.equal(getattr(E.arena, k), getattr(G.arena, k)), (i, k)
            w = 0.01 if i < 3 else 0.5
            want = old.double() + w * (G.arena.flat.double() - old.double())
            err = float((G.arena.ema.double() - want).abs().max())
            moved = float((G.arena.flat - old).abs().max())
            print(f"step {i}: weight {w}, max |ema - (old + w (p - old))| = {err:.3e}, max |p - old| = {moved:.3e}")
            # fp32(1 - 0.99) is within 2^-24 of 0.01; one fma rounding of values below 8
            assert err <= 2.0 ** -24 * moved + 2.0 ** -22, (i, err)
            if i >= 3:
                assert moved > 0 and float((G.arena.ema - old).abs().max()) > 0.4 * moved
        assert G.graphs is graphs and all(x is y for x, y in zip(G.graphs, graphs))
        assert G.arena.ema_desc.table.data_ptr() == desc
    finally:
        fpnmt.set_precision("fp32")


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
        from fpnmt.train import TrainEngine
        import test_gpu_model as TM
        from test_gpu_scst_step import _captions, _images
        # different initial weights per rank: the engine broadcasts rank 0's,
        # and the average must start from those
        m, _, _ = TM._build(num_layers=1, vocab=VOCAB, image=IMAGE, max_seq_len=T, seed=17 + rank)
        fpnmt.set_precision("fp32")
        eng = TrainEngine(m, 1e-5, use_graph=True, ema_decay=DECAY)
        start_equal = bool(torch.equal(eng.arena.ema, eng.arena.flat))
        img = _images(2 * B, IMAGE, 23)[rank * B:(rank + 1) * B].cuda()
        tok = _captions(2 * B, T, VOCAB, 24, lens=[12, 5, 9, 12])[rank * B:(rank + 1) * B].cuda()
        for _ in range(3):
            eng.step(img, tok)
        torch.cuda.synchronize()
        a = eng.arena
        torch.save({"flat": a.flat.detach().cpu(), "ema": a.ema.detach().cpu(), "start_equal": start_equal,
                    "split": eng.split, "world": eng.world, "step": int(a.step)},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp_world2_ranks_keep_equal_averages(tmp_path):
    """Two gloo ranks (as tests/test_gpu_dp_step.py sets them up), each on its
    own half of the batch: the parameters and the averages are bitwise equal
    across the ranks after three steps, with no exchange of the average."""
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
    assert res[0]["split"] and res[0]["world"] == 2 and res[0]["step"] == 3
    assert res[0]["start_equal"] and res[1]["start_equal"]
    assert torch.equal(res[0]["flat"], res[1]["flat"])
    assert torch.equal(res[0]["ema"], res[1]["ema"])
    assert not torch.equal(res[0]["ema"], res[0]["flat"])

"""Global-norm clipping and the non-finite step guard in the training step
(TrainEngine(global_clipnorm=..., skip_nonfinite=...)): with finite gradients
the guard changes no bit, eager, captured and replayed; a global clip scales by
the norm the arena's gradients have; a step with a non-finite gradient leaves
no trace and the steps after it are those of an engine that never saw it; the
live setter, Pipeline.train_loss, checkpoints and the data-parallel form.

Model: tests/test_gpu_param_groups_step.py's (_model: one layer, ResNet-50,
vocab 300, 128 x 128 images, max_seq_len 12, dropout 0), B = 2, bf16 unless a
test says otherwise.

BatchNorm moving statistics are not compared anywhere: a skipped step's forward
pass has already moved them, they are buffers outside the arena and are not
rolled back (documented in TrainEngine). This model's ResNet-50 runs frozen
BatchNorm, so it has none that move."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_param_groups_step import B, IMAGE, T, VOCAB, _batch, _group, _model
from test_gpu_step_guard_kernel import factor_rtol, norm_rtol

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("flat", "m", "v", "vhat", "step")
DECAY = 0.99


def _require_feature():
    from fpnmt.train import TrainEngine
    from utils.pipeline import Pipeline
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert "global_clipnorm" in sig and "skip_nonfinite" in sig, "TrainEngine has no step guard"
    assert hasattr(TrainEngine, "guard_stats") and hasattr(TrainEngine, "set_global_clipnorm")
    assert hasattr(Pipeline, "guard_stats")


def _snapshot(eng, losses=()):
    a = eng.arena
    out = {k: getattr(a, k).clone() for k in STATE}
    out["ema"] = a.ema.clone() if a.ema is not None else None
    out["loss"] = torch.stack([x.reshape(()) for x in losses]) if losses else torch.empty(0, device=DEV)
    return out


def _same(a, b, what, keys=STATE + ("ema", "loss")):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


def _run(seed, graph, steps=3, groups=None, lr=1e-4, **kw):
    """A fresh model and engine (bf16, with the average), `steps` steps."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    m, _, _ = _model(seed=seed)
    fpnmt.set_precision("bf16")
    pg = [_group(m, groups, frozen=True)] if groups else None
    eng = TrainEngine(m, lr, use_graph=graph, param_groups=pg, ema_decay=DECAY, **kw)
    losses = [eng.step(*_batch(i)).clone() for i in range(steps)]
    torch.cuda.synchronize()
    assert (eng.graphs is not None) == bool(graph)
    out = _snapshot(eng, losses)
    out["eng"] = eng
    flayers.invalidate_weights()
    return out


@pytest.mark.parametrize("groups", [None, "backbone"])
def test_guard_with_finite_gradients_changes_no_bit(groups):
    """Three steps (eager, capture, replay): state, average and losses of the
    guarded engine, run eagerly and through graphs, are bitwise those of the
    engine without the guard (per-tensor clipnorm 1.0 in all three)."""
    import fpnmt
    _require_feature()
    try:
        P = _run(81, True, groups=groups)
        E = _run(81, False, groups=groups, skip_nonfinite=True)
        G = _run(81, True, groups=groups, skip_nonfinite=True)
    finally:
        fpnmt.set_precision("fp32")
    assert P["eng"].arena.guard is None and P["eng"].guard_on is False
    _same(P, G, "the guard changes nothing")
    _same(E, G, "graph replay against eager")
    for R in (E, G):
        st = R["eng"].guard_stats()
        assert (st["skipped"], st["consecutive"], st["n_skipped"], st["n_applied"]) == (0, 0, 0, 3), st
        assert st["clip_factor"] == 1.0 and math.isfinite(st["grad_norm"]) and st["grad_norm"] > 0
    assert E["eng"].guard_stats()["grad_norm"] == G["eng"].guard_stats()["grad_norm"]
    assert int(G["step"]) == 3


def test_huge_global_clip_is_bitwise_no_clip():
    """global_clipnorm 1e30 with clipnorm 0: the factor is 1.0 exactly, and
    everything is bitwise the plain clipnorm = 0 engine."""
    import fpnmt
    _require_feature()
    try:
        P = _run(82, True, clipnorm=0.0)
        G = _run(82, True, clipnorm=0.0, global_clipnorm=1e30)
    finally:
        fpnmt.set_precision("fp32")
    _same(P, G, "global_clipnorm 1e30")
    assert G["eng"].guard_stats()["clip_factor"] == 1.0 and G["eng"].global_clipnorm == 1e30


def test_small_global_clip_scales_by_the_arena_gradients_norm():
    """One eager step. The gradient arena still holds the step's gradients:
    their fp64 norm (the embedding's segment through its supplied
    IndexedSlices norm, which is what every clip of that tensor uses) against
    guard_stats()["grad_norm"] within the kernel test's derived bound at this
    arena's block count; clip_factor is the fp32 clip / max(norm, clip) of the
    kernel's own total; the parameters differ from the unclipped run's."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    _require_feature()
    clip = 1e-2
    try:
        res = {}
        for name, kw in (("plain", {}), ("clipped", dict(global_clipnorm=clip))):
            m, _, _ = _model(seed=83)
            fpnmt.set_precision("bf16")
            eng = TrainEngine(m, 1e-4, use_graph=False, clipnorm=0.0, **kw)
            eng.step(*_batch(0))
            torch.cuda.synchronize()
            res[name] = eng
            flayers.invalidate_weights()
    finally:
        fpnmt.set_precision("fp32")
    eng = res["clipped"]
    a = eng.arena
    g = a.grad.double()
    i = eng.emb_seg
    lo, hi = a.offsets[i], a.offsets[i] + a.params[i].numel()
    total = float((g[:lo] ** 2).sum() + (g[hi:] ** 2).sum()) + float(a.sumsq[i].double())
    want = math.sqrt(total)
    st = eng.guard_stats()
    bound = norm_rtol(a.nblocks)
    print(f"nblocks {a.nblocks}: ||g|| {st['grad_norm']:.9g} (fp64 {want:.9g}, rel "
          f"{abs(st['grad_norm'] / want - 1):.3e}, bound {bound:.3e}); factor {st['clip_factor']:.9g}")
    assert want > clip and st["skipped"] == 0 and st["n_applied"] == 1
    assert abs(st["grad_norm"] - want) <= bound * want
    ss32 = np.float32(st["grad_norm"] ** 2)  # the state's fp32 total (its sqrt in double, squared, rounds back)
    want_f = np.float32(clip) / max(np.sqrt(ss32), np.float32(clip))
    assert st["clip_factor"] == float(want_f), (st["clip_factor"], float(want_f))
    assert abs(st["clip_factor"] - clip / want) <= factor_rtol(a.nblocks) * clip / want
    assert torch.equal(res["plain"].arena.grad, a.grad)  # the same gradients ...
    assert not torch.equal(res["plain"].arena.flat, a.flat)  # ... another update


def _wbatch(i, bad=False):
    img, tok = _batch(i, n=2)
    w = (torch.randn(B * 2, generator=torch.Generator().manual_seed(300 + i)) * 1.5).to(DEV)
    if bad:
        w[1] = float("inf")
    return img, tok, w


def test_skipped_step_weighted_leaves_no_trace():
    """step_weighted, graphs (eager, capture, then replays). The third call's
    weights hold one inf: the forward stays clean, the loss and the gradient
    are not finite. State, average and `iterations` are byte-equal across
    that step; the clean steps after it are bitwise, in state, average and
    losses, those of a twin engine that never saw the bad batch (dropout is
    off; with it on, `iterations` staying put makes the next step draw the
    skipped one's masks, which is what makes the twin exact). That also shows
    the bf16 compute copies were left consistent with the masters."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    _require_feature()
    try:
        out = {}
        for name, plan in (("A", [0, 1, "bad", 2, 3]), ("T", [0, 1, 2, 3])):
            m, _, _ = _model(seed=84)
            fpnmt.set_precision("bf16")
            eng = TrainEngine(m, 1e-4, use_graph=True, ema_decay=DECAY, skip_nonfinite=True)
            losses = []
            for k in plan:
                if k == "bad":
                    before = _snapshot(eng)
                    loss = eng.step_weighted(*_wbatch(7, bad=True)).clone()
                    torch.cuda.synchronize()
                    assert not bool(torch.isfinite(loss))
                    _same(before, _snapshot(eng), "across the skipped step", keys=STATE + ("ema",))
                    st = eng.guard_stats()
                    assert (st["skipped"], st["consecutive"], st["n_skipped"], st["n_applied"]) == (1, 1, 1, 2), st
                    assert not math.isfinite(st["grad_norm"])
                    assert int(eng.step_skipped) == 1
                else:
                    losses.append(eng.step_weighted(*_wbatch(k)).clone())
            torch.cuda.synchronize()
            assert next(iter(eng._wsteps.values()))[1] is not None  # captured
            out[name] = _snapshot(eng, losses)
            out[name]["stats"] = eng.guard_stats()
            flayers.invalidate_weights()
    finally:
        fpnmt.set_precision("fp32")
    _same(out["A"], out["T"], "after the skipped step")
    assert int(out["A"]["step"]) == 4 and bool(torch.isfinite(out["A"]["loss"]).all())
    sa, stw = out["A"]["stats"], out["T"]["stats"]
    assert (sa["skipped"], sa["consecutive"], sa["n_skipped"], sa["n_applied"]) == (0, 0, 1, 4), sa
    assert (stw["n_skipped"], stw["n_applied"]) == (0, 4) and sa["grad_norm"] == stw["grad_norm"]


def test_set_global_clipnorm_between_replays():
    """After capture: set_global_clipnorm keeps the captured graph object and
    the next replay clips; an eager engine given the same calls agrees bit for
    bit. A per-tensor-clipping engine refuses a global clip > 0."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.train import TrainEngine
    _require_feature()
    m_e, _, _ = _model(seed=85)
    m_g, _, _ = _model(seed=85)
    fpnmt.set_precision("bf16")
    try:
        E = TrainEngine(m_e, 1e-4, use_graph=False, clipnorm=0.0, global_clipnorm=1e30)
        G = TrainEngine(m_g, 1e-4, use_graph=True, clipnorm=0.0, global_clipnorm=1e30)
        desc = G.arena.guard.desc.data_ptr()
        graphs = None
        for i in range(5):
            if i == 3:
                graphs = G.graphs
                assert graphs is not None
                for eng in (E, G):
                    eng.set_global_clipnorm(1e-3)
                assert G.global_clipnorm == 1e-3
            if i == 4:
                for eng in (E, G):
                    eng.set_global_clipnorm(0)  # the clip off, the guard stays
            le, lg = E.step(*_batch(i)).clone(), G.step(*_batch(i)).clone()
            torch.cuda.synchronize()
            assert torch.equal(le, lg), i
            for k in STATE:
                assert torch.equal(getattr(E.arena, k), getattr(G.arena, k)), (i, k)
            st = G.guard_stats()
            assert st == E.guard_stats(), i
            if i == 3:
                assert 0.0 < st["clip_factor"] < 1.0 and st["clip_factor"] == float(
                    np.float32(1e-3) / np.sqrt(np.float32(st["grad_norm"] ** 2))), st
            else:
                assert st["clip_factor"] == 1.0, (i, st)
        assert G.graphs is graphs and all(x is y for x, y in zip(G.graphs, graphs))
        assert G.arena.guard.desc.data_ptr() == desc and G.guard_stats()["n_applied"] == 5
        flayers.invalidate_weights()
        P = TrainEngine(_model(seed=85)[0], 1e-4, use_graph=False, skip_nonfinite=True)  # clipnorm 1.0
        with pytest.raises(ValueError, match="exclusive"):
            P.set_global_clipnorm(1.0)
        P.set_global_clipnorm(0.0)
        N = TrainEngine(_model(seed=85)[0], 1e-4, use_graph=False)
        for call in (lambda: N.set_global_clipnorm(1.0), N.guard_stats):
            with pytest.raises(ValueError, match="global_clipnorm"):
                call()
    finally:
        fpnmt.set_precision("fp32")
        flayers.invalidate_weights()


def _pipe(seed, **kw):
    from fpnmt.layers import Init, invalidate_weights
    from utils.pipeline import Pipeline
    pl = Pipeline(max_seq_len=T, target_vocab_size=VOCAB, image_size=IMAGE, n_layers=1, rate=0.0,
                  init=Init(torch.Generator().manual_seed(seed)), **kw)
    invalidate_weights()
    return pl


def test_pipeline_train_loss_leaves_the_skipped_step_out():
    """fp32, eager. Two clean steps, one whose vocabulary bias holds an inf
    (set by hand, taken out again afterwards: the logits, the loss and the
    gradient are not finite; every index the kernels use comes from clean
    data), one more clean step. train_loss is finite and is the mean of the
    three applied steps' losses; guard_stats counts 3 and 1."""
    import fpnmt
    from fpnmt.layers import invalidate_weights
    _require_feature()
    fpnmt.set_precision("fp32")
    pl = _pipe(86, use_graph=False, clipnorm_mode="none", global_clipnorm=1.0)
    assert pl.engine.guard_on and pl.engine.adam["clipnorm"] == 0.0
    bias = pl.transformer.final_layer.bias
    kept = []
    for k in (0, 1, "bad", 2):
        if k == "bad":
            before = pl.engine.arena.flat.clone()
            with torch.no_grad():
                old = bias[5].clone()
                bias[5] = float("inf")
            invalidate_weights()
            poisoned = pl.engine.arena.flat.clone()
            loss = pl.train_step(*_batch(9)).clone()
            torch.cuda.synchronize()
            assert not bool(torch.isfinite(loss))
            assert torch.equal(pl.engine.arena.flat, poisoned)  # nothing moved
            with torch.no_grad():
                bias[5] = old
            invalidate_weights()
            assert torch.equal(pl.engine.arena.flat, before)
            assert pl.guard_stats()["skipped"] == 1
        else:
            kept.append(pl.train_step(*_batch(k)).clone())
    torch.cuda.synchronize()
    got = pl.train_loss.result()
    want = torch.stack(kept).to(torch.float32).cpu()
    want = ((want[0] + want[1]) + want[2]) / 3.0  # the metric's own fp32 order
    print(f"train_loss {float(got):.7f}, mean of the applied steps {float(want):.7f}")
    assert bool(torch.isfinite(got)) and float(got) == float(want)
    st = pl.guard_stats()
    assert (st["n_skipped"], st["n_applied"], st["consecutive"]) == (1, 3, 0), st
    assert not bool(torch.isnan(pl.engine.arena.flat).any())
    invalidate_weights()


def test_checkpoint_carries_the_counters(tmp_path):
    """fp32, eager. A guarded engine after one applied and one skipped step
    writes optimizer/guard/n_skipped and n_applied; a fresh guarded engine
    restores them; a checkpoint written without the guard has exactly the keys
    it had before, loads into the guarded engine, and the counts start at 0."""
    import fpnmt
    from fpnmt import layers as flayers
    from fpnmt.checkpoint import Checkpoint
    from fpnmt.train import TrainEngine
    from safetensors import safe_open
    _require_feature()
    fpnmt.set_precision("fp32")
    m_a, m_b, m_p = _model(seed=87)[0], _model(seed=88)[0], _model(seed=87)[0]
    A = TrainEngine(m_a, 1e-4, use_graph=False, skip_nonfinite=True)
    Pn = TrainEngine(m_p, 1e-4, use_graph=False)
    A.step_weighted(*_wbatch(0))
    A.step_weighted(*_wbatch(1, bad=True))
    Pn.step_weighted(*_wbatch(0))
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(A.arena, k), getattr(Pn.arena, k)), k
    guarded, plain = str(tmp_path / "guarded.safetensors"), str(tmp_path / "plain.safetensors")
    Checkpoint(transformer=m_a, optimizer=A).write(guarded)
    Checkpoint(transformer=m_p, optimizer=Pn).write(plain)
    with safe_open(guarded, framework="pt") as f:
        kg = set(f.keys())
        assert int(f.get_tensor("optimizer/guard/n_skipped")) == 1
        assert int(f.get_tensor("optimizer/guard/n_applied")) == 1
    with safe_open(plain, framework="pt") as f:
        kp = set(f.keys())
    assert kg - kp == {"optimizer/guard/n_skipped", "optimizer/guard/n_applied"} and kp <= kg
    Bn = TrainEngine(m_b, 1e-4, use_graph=False, global_clipnorm=0.0)
    Checkpoint(transformer=m_b, optimizer=Bn).restore(guarded)
    torch.cuda.synchronize()
    st = Bn.guard_stats()
    assert (st["n_skipped"], st["n_applied"]) == (1, 1), st
    for k in STATE:
        assert torch.equal(getattr(A.arena, k), getattr(Bn.arena, k)), k
    Bn.step_weighted(*_wbatch(2))
    assert Bn.guard_stats()["n_applied"] == 2
    Checkpoint(transformer=m_b, optimizer=Bn).restore(plain)  # written without the counters
    st = Bn.guard_stats()
    assert (st["n_skipped"], st["n_applied"]) == (0, 0), st
    Checkpoint(transformer=m_p, optimizer=Pn).restore(guarded)  # the guard keys are ignored
    assert Pn.arena.guard is None and int(Pn.arena.step) == 1
    flayers.invalidate_weights()


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
        m, _, _ = TM._build(num_layers=1, vocab=VOCAB, image=IMAGE, max_seq_len=T, seed=17 + rank)
        fpnmt.set_precision("fp32")
        eng = TrainEngine(m, 1e-5, use_graph=True, ema_decay=DECAY, skip_nonfinite=True)
        img = _images(2 * B, IMAGE, 23)[rank * B:(rank + 1) * B].cuda()
        tok = _captions(2 * B, T, VOCAB, 24, lens=[12, 5, 9, 12])[rank * B:(rank + 1) * B].cuda()
        good = torch.tensor([0.75, -1.25], device="cuda")
        bad = good.clone()
        if rank == 0:
            bad[1] = float("inf")  # only this rank's gradient is poisoned before the all-reduce
        skipped, snaps = [], []
        for w in (good, good, bad, good):  # eager, capture, replay, replay
            eng.step_weighted(img, tok, w)
            torch.cuda.synchronize()
            skipped.append(eng.guard_stats()["skipped"])
            snaps.append(eng.arena.flat.detach().cpu().clone())
        a = eng.arena
        torch.save({"flat": a.flat.detach().cpu(), "ema": a.ema.detach().cpu(), "m": a.m.detach().cpu(),
                    "vhat": a.vhat.detach().cpu(), "skipped": skipped, "stats": eng.guard_stats(),
                    "kept": bool(torch.equal(snaps[1], snaps[2])), "moved": not torch.equal(snaps[2], snaps[3]),
                    "split": eng.split, "world": eng.world, "step": int(a.step)},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp_world2_both_ranks_skip_the_same_step(tmp_path):
    """Two gloo ranks (as tests/test_gpu_ema_step.py sets them up), fresh
    child processes. Only rank 0 gets the inf weight in the third call; after
    the SUM all-reduce both ranks see the non-finite gradient, both skip that
    step and no other, and both end with byte-equal arenas."""
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
    for r in res:
        assert r["split"] and r["world"] == 2 and r["step"] == 3
        assert r["skipped"] == [0, 0, 1, 0] and r["kept"] and r["moved"]
        assert (r["stats"]["n_skipped"], r["stats"]["n_applied"], r["stats"]["consecutive"]) == (1, 3, 0)
    for k in ("flat", "ema", "m", "vhat"):
        assert torch.equal(res[0][k].view(torch.int32), res[1][k].view(torch.int32)), k
    assert not torch.isnan(res[0]["flat"]).any() and not torch.equal(res[0]["ema"], res[0]["flat"])

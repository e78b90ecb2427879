"""fpnmt_amsgrad_step_ema and fpnmt_swap_f32 at the arena level (no model):
the shadow update kept inside the optimizer kernel against the fp64 reference
tests/ema_ref.py, on the segment table of tests/test_gpu_param_groups_kernel.py
(2*16384 + 5 elements: three blocks, float4 body and a scalar tail; 7
elements: tail only; the sparse (50, 16) embedding; frozen segments first, in
the middle (two blocks) and last).

The bar for the average is the project's existing one for this kernel, atol
1e-6 and rtol 1e-5 (test_amsgrad_matches_keras): e_new = e + w (p - e) with
0 <= w <= 1 is a convex combination, so it carries at most the error of p,
which that bar already covers, plus one fp32 rounding of values below 8
(5e-7)."""
import inspect

import numpy as np
import pytest
import torch

from ema_ref import EmaAMSGradRef
from test_gpu_param_groups_kernel import ROWS, SEGS, _arena, _grads, _rows, _seg

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("flat", "m", "v", "vhat")
PLAIN = {n: (1.0, 0.0, False) for n, _, _ in SEGS}


def _require_feature():
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    assert "fpnmt_amsgrad_step_ema" in L.ALL_SYMBOLS and "fpnmt_swap_f32" in L.ALL_SYMBOLS
    assert hasattr(ParamArena, "enable_ema")
    assert "ema" in inspect.signature(ParamArena.amsgrad_step).parameters


def _gap_mask(ar):
    """True on the alignment gaps of the arena's layout."""
    mask = torch.ones(ar.total, dtype=torch.bool, device=DEV)
    for o, p in zip(ar.offsets, ar.params):
        mask[o:o + p.numel()] = False
    assert bool(mask.any())
    return mask


def _load(ar, ps, grads, rows, fill):
    """Gradients into the arena; the frozen segments' gradients and every
    alignment gap hold `fill` (NaN: anything that reads them shows)."""
    ar.zero_grad()
    ar.grad.fill_(fill)
    for n, p in ps:
        if not rows[n][2]:
            p.grad.copy_(grads[n].to(DEV))
    emb_ss = float((grads["emb"].double() ** 2).sum()) * 1.7  # caller-supplied IndexedSlices norm
    ar.sumsq_slot(dict(ps)["emb"]).fill_(emb_ss)
    return emb_ss


def _make(rows, grouped, decay, debias, seed=0):
    ar, ps, init = _arena(seed)
    groups = ar.make_groups(_rows(ar, rows)) if grouped else None
    if decay is not None:
        ar.enable_ema(decay, debias)
        ar.ema[_gap_mask(ar)] = float("nan")
    return ar, ps, init, groups


@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("clipnorm", [1.0, 0.0])
def test_ema_step_against_the_reference_and_the_step_without(clipnorm, grouped, debias):
    """Three steps at decay 0.9 (with debias the weight is 9 / (10 + t), without
    it 0.1). flat, m, v and vhat are bitwise those of the same run without the
    average. NaN sits in the frozen segments' gradients, in every alignment
    gap of grad and of ema: none reaches a trainable output, the gaps still
    hold it, and the frozen segments' shadow is bitwise what it was. The
    shadow of the trainable segments meets the reference at atol 1e-6, rtol
    1e-5."""
    from utils.utils import CustomSchedule
    _require_feature()
    rows = ROWS if grouped else PLAIN
    sched = CustomSchedule(2048, 4000)
    ar, ps, init, groups = _make(rows, grouped, 0.9, debias)
    ar0, ps0, _, groups0 = _make(rows, grouped, None, debias)
    mask = _gap_mask(ar)
    ref = EmaAMSGradRef({n: s for n, s, _ in SEGS}, 0.9, debias=debias, clipnorm=clipnorm, sparse=["emb"])
    assert ref.omd == ar.ema_desc.one_minus_decay  # the fp32 value the kernel is handed
    params = {n: v.double().numpy().copy() for n, v in init.items()}
    frozen = [n for n in rows if rows[n][2]]
    train = [n for n in rows if not rows[n][2]]
    assert bool(frozen) == grouped
    ema0 = ar.ema.clone()
    for step in range(3):
        grads = _grads(step)
        emb_ss = _load(ar, ps, grads, rows, float("nan"))
        _load(ar0, ps0, grads, rows, float("nan"))
        ar.amsgrad_step(sched, clipnorm=clipnorm, groups=groups, ema=True)
        ar0.amsgrad_step(sched, clipnorm=clipnorm, groups=groups0)
        ref.apply(params, {n: g.double().numpy() for n, g in grads.items()}, sched, rows, norms={"emb": emb_ss})
        torch.cuda.synchronize()
        for k in STATE:  # the average only reads
            assert torch.equal(getattr(ar, k), getattr(ar0, k)), (step, k)
            assert not torch.isnan(getattr(ar, k)).any(), (step, k)
        assert bool(torch.isnan(ar.ema[mask]).all()), step  # the gaps were not written
        assert not torch.isnan(ar.ema[~mask]).any(), step  # ... and nothing read them, or a frozen gradient
        for n in frozen:
            assert torch.equal(_seg(ar, ar.ema, n), _seg(ar, ema0, n)), (step, n)
    assert int(ar.step.item()) == 3
    for n in train:
        got = _seg(ar, ar.ema, n).cpu().double().numpy().reshape(ref.ema[n].shape)
        print(f"{n}: max |ema - ref| = {np.abs(got - ref.ema[n]).max():.3e}")
        assert np.allclose(got, ref.ema[n], atol=1e-6, rtol=1e-5), n
        p = _seg(ar, ar.flat, n).cpu().double().numpy().reshape(got.shape)
        if rows[n][0] != 0.0:  # lr_scale 0 stops the tensor (the decay term is scaled too), and its average
            assert not np.array_equal(got, init[n].double().numpy()), n  # it moved
            assert not np.array_equal(got, p), n  # and it is not the parameter
        else:
            assert np.array_equal(got, init[n].double().numpy()) and np.array_equal(got, p), n


@pytest.mark.parametrize("grouped", [True, False])
def test_one_launch_equals_the_early_update_parts(grouped):
    """One launch over all blocks against blocks=(0, k) on a persistent grid of
    3 workgroups without the step increment, then blocks=(k, n): the shape of
    the early update. Everything bitwise, the average included."""
    from utils.utils import CustomSchedule
    _require_feature()
    rows = ROWS if grouped else PLAIN
    sched = CustomSchedule(2048, 4000)
    res = []
    for parts in (False, True):
        ar, ps, _, groups = _make(rows, grouped, 0.99, True, seed=3)
        cut = ar.block_of(ar.offsets[ar.names.index("tiny")])
        assert 0 < cut < ar.nblocks
        for step in range(2):
            _load(ar, ps, _grads(step, seed=200), rows, float("nan"))
            if parts:
                ar.amsgrad_step(sched, blocks=(0, cut), inc_step=False, max_grid=3, groups=groups, ema=True)
                ar.amsgrad_step(sched, blocks=(cut, ar.nblocks), groups=groups, ema=True)
            else:
                ar.amsgrad_step(sched, groups=groups, ema=True)
        torch.cuda.synchronize()
        assert int(ar.step.item()) == 2
        res.append({k: getattr(ar, k).clone() for k in STATE + ("ema",)})
    mask = _gap_mask(ar)
    for k in STATE:
        assert torch.equal(res[0][k], res[1][k]), k
    assert torch.equal(res[0]["ema"][~mask], res[1]["ema"][~mask])
    assert not torch.equal(res[0]["ema"][~mask], res[0]["flat"][~mask])


def test_decay_zero_without_debias_follows_the_parameters():
    """decay 0, debias off: e + 1 * (p - e) is p up to one rounding, so the
    shadow equals the parameters within the kernel's bar after every step."""
    _require_feature()
    ar, ps, _, _ = _make(PLAIN, False, 0.0, False)
    mask = _gap_mask(ar)
    assert ar.ema_desc.host() == (1.0, 0)
    for step in range(3):
        _load(ar, ps, _grads(step), PLAIN, float("nan"))
        ar.amsgrad_step(1e-2, ema=True)
        torch.cuda.synchronize()
        e, p = ar.ema[~mask].cpu().double().numpy(), ar.flat[~mask].cpu().double().numpy()
        print(f"step {step}: max |ema - p| = {np.abs(e - p).max():.3e}")
        assert np.allclose(e, p, atol=1e-6, rtol=1e-5), step


def test_set_ema_decay_changes_the_next_step_only():
    """Two steps; arena A changes its decay from 0.9 to 0.5 between them, B
    keeps 0.9 (debias off, so the decay is the weight). After step one the
    two shadows are bitwise equal; after step two they differ, A's meets the
    reference that changed its decay at the same point, and the descriptor is
    the same device word. The parameters never differ."""
    _require_feature()
    A, psA, init, _ = _make(PLAIN, False, 0.9, False)
    Bm, psB, _, _ = _make(PLAIN, False, 0.9, False)
    mask = _gap_mask(A)
    ref = EmaAMSGradRef({n: s for n, s, _ in SEGS}, 0.9, debias=False, sparse=["emb"])
    params = {n: v.double().numpy().copy() for n, v in init.items()}
    where = A.ema_desc.table.data_ptr()
    for step in range(2):
        grads = _grads(step)
        emb_ss = _load(A, psA, grads, PLAIN, float("nan"))
        _load(Bm, psB, grads, PLAIN, float("nan"))
        A.amsgrad_step(1e-2, ema=True)
        Bm.amsgrad_step(1e-2, ema=True)
        ref.apply(params, {n: g.double().numpy() for n, g in grads.items()}, lambda it: 1e-2, PLAIN,
                  norms={"emb": emb_ss})
        torch.cuda.synchronize()
        assert torch.equal(A.flat, Bm.flat), step
        same = torch.equal(A.ema[~mask], Bm.ema[~mask])
        assert same == (step == 0), step
        if step == 0:
            A.set_ema_decay(0.5)
            ref.set_decay(0.5)
            assert A.ema_desc.table.data_ptr() == where and A.ema_desc.host() == (0.5, 0)
    for n in PLAIN:
        got = _seg(A, A.ema, n).cpu().double().numpy().reshape(ref.ema[n].shape)
        assert np.allclose(got, ref.ema[n], atol=1e-6, rtol=1e-5), n


def test_entry_point_refuses_missing_or_aliased_ema():
    from fpnmt import _lib as L
    _require_feature()
    ar, ps, _, _ = _make(PLAIN, False, 0.9, True)
    good = ar.ema
    try:
        ar.ema = ar.flat  # the average may not alias another array of the step
        with pytest.raises(RuntimeError, match="alias"):
            ar.amsgrad_step(1e-2, ema=True)
    finally:
        ar.ema = good
    assert int(ar.step.item()) == 0


# ------------------------------------------------------------------- swap
_ARENA_TOTAL = -1  # stands for the arena's total below
# 0, 3 (tail only), 4 (one vector), 4*256*7 + 3 (seven blocks and a tail), the
# arena's total, and one length past a single pass of the grid-stride loop
# (4096 workgroups of 256 threads, four elements each)
SWAP_LENGTHS = [0, 3, 4, 4 * 256 * 7 + 3, _ARENA_TOTAL, 4 * 4096 * 256 + 4 * 300 + 1]


@pytest.mark.parametrize("guard", [4, 1])
@pytest.mark.parametrize("n", SWAP_LENGTHS)
def test_swap_f32(n, guard):
    """One swap exchanges the contents exactly, two are the identity bitwise,
    and `guard` elements on both sides of each buffer are unchanged. guard 4
    keeps the buffers 16-byte aligned (the float4 body), guard 1 does not (the
    scalar form)."""
    from fpnmt import _lib as L
    _require_feature()
    if n == _ARENA_TOTAL:
        n = _arena()[0].total
        assert n > 0 and n % 4 == 0
    g = torch.Generator().manual_seed(n % 1000 + guard)
    # bit patterns of every kind, NaNs and infinities included
    a_full = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 2 * guard,), generator=g, dtype=torch.int64).to(torch.int32)
    b_full = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 2 * guard,), generator=g, dtype=torch.int64).to(torch.int32)
    a_full, b_full = a_full.to(DEV), b_full.to(DEV)
    a0, b0 = a_full.clone(), b_full.clone()
    a, b = a_full[guard:guard + n], b_full[guard:guard + n]
    if n:  # an empty slice has no address
        assert (a.data_ptr() % 16 == 0) == (guard == 4)

    def swap():
        L.call("fpnmt_swap_f32", a.data_ptr(), b.data_ptr(), n, L.stream_ptr())
        torch.cuda.synchronize()
    swap()
    assert torch.equal(a, b0[guard:guard + n]) and torch.equal(b, a0[guard:guard + n])
    for full, orig in ((a_full, a0), (b_full, b0)):
        assert torch.equal(full[:guard], orig[:guard]) and torch.equal(full[guard + n:], orig[guard + n:])
    swap()
    assert torch.equal(a_full, a0) and torch.equal(b_full, b0)


def test_arena_swap_ema_is_exact():
    _require_feature()
    ar, ps, _, _ = _make(PLAIN, False, 0.9, True)
    _load(ar, ps, _grads(0), PLAIN, float("nan"))
    ar.amsgrad_step(1e-2, ema=True)
    flat, ema = ar.flat.clone().view(torch.int32), ar.ema.clone().view(torch.int32)
    where = ar.flat.data_ptr()
    ar.swap_ema()
    torch.cuda.synchronize()
    assert torch.equal(ar.flat.view(torch.int32), ema) and torch.equal(ar.ema.view(torch.int32), flat)
    assert ar.flat.data_ptr() == where and ps[0][1].data_ptr() == where  # no pointer moved
    ar.swap_ema()
    torch.cuda.synchronize()
    assert torch.equal(ar.flat.view(torch.int32), flat) and torch.equal(ar.ema.view(torch.int32), ema)

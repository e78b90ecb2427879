"""fpnmt_grad_norm_total and fpnmt_amsgrad_step_guard at the arena level (no
model): the global-norm clip and the non-finite step guard against the fp64
reference tests/step_guard_ref.py, on the segment table of
tests/test_gpu_param_groups_kernel.py (2*16384 + 5 elements: three blocks,
float4 body and a scalar tail; 7 elements: tail only; the sparse (50, 16)
embedding with a caller-supplied norm; frozen segments first, in the middle
(two blocks) and last). NaN sits in the frozen segments' gradients, in every
alignment gap and, before each step, in every per-block partial, so that a
read of any of them shows.

The bar for flat, m, v, vhat and the average is the project's existing one for
this kernel, atol 1e-6 and rtol 1e-5 (test_amsgrad_matches_keras).

The bar for the norm is derived from the kernel's summation, not measured.
Every term is non-negative, so each fp32 rounding a term passes through adds
at most u = 2^-24 relative to the sum (first order). A term's path:
  2   the element times grad_scale, rounded once, enters the square twice
  1   the square
  3   the adds inside a float4's a*a + b*b + c*c + e*e
  17  the thread's running sum: a full block is 4096 float4 over 256 threads,
      16 per thread, plus one scalar-tail element
  6   wave_sum's tree
  2   (red[0] + red[1]) + (red[2] + red[3])
  ceil(nblocks / 256)   grad_norm_total's running sum per thread
  6   its wave_sum
  2   its four waves
(a bit0 segment's supplied norm passes through fewer: its fp32 storage, two
products with grad_scale, and the total's part.) With D their sum, ||g||^2 is
within D u and ||g|| = sqrt within D u / 2; one more u covers the second-order
terms: NORM_RTOL = (D / 2 + 1) u. clip_factor adds sqrtf's and the division's
rounding: FACTOR_RTOL = (D / 2 + 3) u. Here nblocks = 10, D = 40: 21 u = 1.25e-6
and 23 u = 1.37e-6."""
import inspect
import math

import numpy as np
import pytest
import torch

from step_guard_ref import GuardedAMSGradRef
from test_gpu_param_groups_kernel import BLOCK, ROWS, SEGS, _arena, _grads, _rows, _seg

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("flat", "m", "v", "vhat")
PLAIN = {n: (1.0, 0.0, False) for n, _, _ in SEGS}
U = 2.0 ** -24


def norm_rtol(nblocks):
    """(D / 2 + 1) u of the module docstring."""
    return ((2 + 1 + 3 + 17 + 6 + 2 + math.ceil(nblocks / 256) + 6 + 2) / 2 + 1) * U


def factor_rtol(nblocks):
    return norm_rtol(nblocks) + 2 * U


def _require_feature():
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    assert "fpnmt_grad_norm_total" in L.ALL_SYMBOLS and "fpnmt_amsgrad_step_guard" in L.ALL_SYMBOLS
    assert hasattr(ParamArena, "enable_guard")
    assert "guard" in inspect.signature(ParamArena.amsgrad_step).parameters


def _gap_mask(ar):
    mask = torch.ones(ar.total, dtype=torch.bool, device=DEV)
    for o, p in zip(ar.offsets, ar.params):
        mask[o:o + p.numel()] = False
    assert bool(mask.any())
    return mask


def _make(rows, grouped, ema, gcn, seed=0):
    """An arena; gcn None: no guard."""
    ar, ps, init = _arena(seed)
    groups = ar.make_groups(_rows(ar, rows)) if grouped else None
    if ema:
        ar.enable_ema(0.9, True)
        ar.ema[_gap_mask(ar)] = float("nan")
    if gcn is not None:
        ar.enable_guard(gcn)
    return ar, ps, init, groups


def _load(ar, ps, grads, rows, emb_norm=None):
    """Gradients into the arena. NaN in the frozen segments' gradients, in
    every alignment gap and in every per-block partial."""
    ar.zero_grad()
    ar.grad.fill_(float("nan"))
    ar.blk_part.fill_(float("nan"))
    for n, p in ps:
        if not rows[n][2]:
            p.grad.copy_(grads[n].to(DEV))
    emb_ss = float((grads["emb"].double() ** 2).sum()) * 1.7 if emb_norm is None else emb_norm
    ar.sumsq_slot(dict(ps)["emb"]).fill_(emb_ss)
    return float(np.float32(emb_ss))  # as the slot holds it


def _bits(ar, ema):
    out = {k: getattr(ar, k).clone().view(torch.int32) for k in STATE}
    out["step"] = ar.step.clone()
    if ema:
        out["ema"] = ar.ema.clone().view(torch.int32)
    return out


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


CASES = [(g, e, 1.0) for g in (True, False) for e in (True, False)] + [(True, True, 0.5)]


@pytest.mark.parametrize("grouped,ema,grad_scale", CASES)
def test_global_clip_against_the_reference(grouped, ema, grad_scale):
    """Three steps at global_clipnorm 1.0 (big's gradients are scaled by 5:
    ||g|| is near 900 and the clip bites). State and average at atol 1e-6,
    rtol 1e-5; sqrt(sumsq_total) and clip_factor after every step within the
    derived NORM_RTOL / FACTOR_RTOL of the fp64 values. With NaN in the frozen
    gradients, the gaps and the stale partials nothing is skipped and no NaN
    reaches an output."""
    from utils.utils import CustomSchedule
    _require_feature()
    rows = ROWS if grouped else PLAIN
    sched = CustomSchedule(2048, 4000)
    ar, ps, init, groups = _make(rows, grouped, ema, 1.0)
    assert ar.nblocks == 10
    mask = _gap_mask(ar)
    ref = GuardedAMSGradRef({n: s for n, s, _ in SEGS}, 0.9, debias=True, clipnorm=0.0, global_clipnorm=1.0,
                            sparse=["emb"])
    params = {n: v.double().numpy().copy() for n, v in init.items()}
    train = [n for n in rows if not rows[n][2]]
    for step in range(3):
        grads = _grads(step)
        emb_ss = _load(ar, ps, grads, rows)
        ar.amsgrad_step(sched, clipnorm=0.0, grad_scale=grad_scale, groups=groups, ema=ema, guard=True)
        ref.apply(params, {n: g.double().numpy() for n, g in grads.items()}, sched, rows, norms={"emb": emb_ss},
                  grad_scale=grad_scale)
        torch.cuda.synchronize()
        h = ar.guard.host()
        want_norm = math.sqrt(ref.sumsq_total)
        got_norm = math.sqrt(h["sumsq_total"])
        print(f"step {step}: ||g|| {got_norm:.9g} (fp64 {want_norm:.9g}, rel {abs(got_norm / want_norm - 1):.3e}, "
              f"bound {norm_rtol(ar.nblocks):.3e}); factor {h['clip_factor']:.9g} (fp64 {ref.clip_factor:.9g}, "
              f"rel {abs(h['clip_factor'] / ref.clip_factor - 1):.3e}, bound {factor_rtol(ar.nblocks):.3e})")
        assert want_norm > 100.0 and ref.clip_factor < 0.01  # the clip bites
        assert abs(got_norm - want_norm) <= norm_rtol(ar.nblocks) * want_norm, step
        assert abs(h["clip_factor"] - ref.clip_factor) <= factor_rtol(ar.nblocks) * ref.clip_factor, step
        assert (h["skipped"], h["consecutive"], h["n_skipped"], h["n_applied"]) == (0, 0, 0, step + 1)
        assert ar.guard.stats()["grad_norm"] == got_norm
        for k in STATE:
            assert not torch.isnan(getattr(ar, k)).any(), (step, k)
        if ema:
            assert bool(torch.isnan(ar.ema[mask]).all()) and not torch.isnan(ar.ema[~mask]).any(), step
    assert int(ar.step.item()) == 3 and ref.iterations == 3
    for n, p in ps:
        got = p.detach().cpu().double().numpy()
        print(f"{n}: max |p - ref| = {np.abs(got - params[n]).max():.3e}")
        assert np.allclose(got, params[n], atol=1e-6, rtol=1e-5), n
        if rows[n][2]:
            assert np.array_equal(got, init[n].double().numpy()), n
        for k, rk in (("m", ref.m), ("v", ref.v), ("vhat", ref.vhat)) + ((("ema", ref.ema),) if ema else ()):
            s = _seg(ar, getattr(ar, k), n).cpu().double().numpy().reshape(rk[n].shape)
            assert np.allclose(s, rk[n], atol=1e-6, rtol=1e-5), (n, k)
    for n in train:
        if rows[n][0] != 0.0:
            assert not np.array_equal(dict(ps)[n].detach().cpu().numpy(), init[n].numpy()), n


def _run(rows, grouped, ema, gcn, clipnorm, steps=2, seed=3, max_grid=0, grad_scale=1.0):
    from utils.utils import CustomSchedule
    sched = CustomSchedule(2048, 4000)
    ar, ps, _, groups = _make(rows, grouped, ema, gcn, seed=seed)
    for step in range(steps):
        _load(ar, ps, _grads(step, seed=200), rows)
        ar.amsgrad_step(sched, clipnorm=clipnorm, grad_scale=grad_scale, groups=groups, ema=ema,
                        guard=gcn is not None, max_grid=max_grid)
    torch.cuda.synchronize()
    assert int(ar.step.item()) == steps
    if gcn is not None:
        h = ar.guard.host()
        assert (h["skipped"], h["n_skipped"], h["n_applied"]) == (0, 0, steps), h
    return _bits(ar, ema), ar


@pytest.mark.parametrize("ema", [True, False])
@pytest.mark.parametrize("grouped", [True, False])
def test_bitwise_identities_with_the_unguarded_step(grouped, ema):
    """global_clipnorm 1e30 gives the factor 1.0 exactly and equals the
    unguarded clipnorm = 0 run; the guard alone (global_clipnorm 0) with the
    per-tensor clipnorm 1.0 equals the unguarded clipnorm = 1 run; a
    persistent grid of 3 workgroups equals one workgroup per block. All bit
    for bit, two steps, grad_scale 0.5 in the first pair."""
    _require_feature()
    rows = ROWS if grouped else PLAIN
    plain0, _ = _run(rows, grouped, ema, None, 0.0, grad_scale=0.5)
    huge, ar = _run(rows, grouped, ema, 1e30, 0.0, grad_scale=0.5)
    assert ar.guard.host()["clip_factor"] == 1.0
    _same_bits(plain0, huge, "global_clipnorm 1e30 against clipnorm 0")
    plain1, _ = _run(rows, grouped, ema, None, 1.0)
    only, ar = _run(rows, grouped, ema, 0.0, 1.0)
    assert ar.guard.host()["clip_factor"] == 1.0
    _same_bits(plain1, only, "guard alone against the per-tensor clip")
    assert not torch.equal(plain0["flat"], plain1["flat"])
    one, _ = _run(rows, grouped, ema, 1.0, 0.0)
    grid3, _ = _run(rows, grouped, ema, 1.0, 0.0, max_grid=3)
    _same_bits(one, grid3, "max_grid 3")
    assert not torch.equal(one["flat"], plain0["flat"])  # the global clip did something


def _poison(kind, ar, ps, grads):
    """-> (the gradients to load, the embedding's supplied norm or None)."""
    g = {n: v.clone() for n, v in grads.items()}
    emb_norm = None
    if kind == "inf_tail":  # the last scalar-tail element of big
        assert g["big"].numel() % 4 == 1
        g["big"][-1] = float("inf")
    elif kind == "nan_body":  # the float4 body of big's middle block
        g["big"][BLOCK + 4 * 100 + 1] = float("nan")
    elif kind == "neg_inf_tiny":
        g["tiny"][3] = float("-inf")
    elif kind == "inf_supplied_norm":
        emb_norm = float("inf")
    elif kind == "overflow":  # finite squares (2.25e38) in two blocks; their sum is not finite
        g["big"][5] = 1.5e19
        g["s0"][7] = 1.5e19
    else:
        raise AssertionError(kind)
    return g, emb_norm


@pytest.mark.parametrize("mode", ["global", "per_tensor"])
@pytest.mark.parametrize("kind", ["inf_tail", "nan_body", "neg_inf_tiny", "inf_supplied_norm", "overflow"])
def test_a_non_finite_step_is_skipped_and_leaves_no_trace(kind, mode):
    """Grouped, with the average. One clean step on arena A and its twin T,
    then the poisoned step on A alone: flat, m, v, vhat, ema and the step
    counter keep their bytes, skipped is 1, n_skipped and consecutive go up
    by one. Then the clean step on both: every array of A is bit for bit T's,
    which only ever took the clean steps; consecutive is 0 and n_applied 2 on
    both. mode: the global clip at 1.0, or the guard alone beside the
    per-tensor clip."""
    from utils.utils import CustomSchedule
    _require_feature()
    sched = CustomSchedule(2048, 4000)
    gcn, clipnorm = (1.0, 0.0) if mode == "global" else (0.0, 1.0)
    A, psA, _, groupsA = _make(ROWS, True, True, gcn)
    T, psT, _, groupsT = _make(ROWS, True, True, gcn)

    def step(ar, ps, groups, grads, emb_norm=None):
        _load(ar, ps, grads, ROWS, emb_norm)
        ar.amsgrad_step(sched, clipnorm=clipnorm, groups=groups, ema=True, guard=True)
        torch.cuda.synchronize()
        return ar.guard.host()
    step(A, psA, groupsA, _grads(0))
    step(T, psT, groupsT, _grads(0))
    before = _bits(A, True)
    _same_bits(before, _bits(T, True), "the first clean step")
    bad, emb_norm = _poison(kind, A, psA, _grads(1))
    h = step(A, psA, groupsA, bad, emb_norm)
    print(kind, mode, h)
    assert (h["skipped"], h["consecutive"], h["n_skipped"], h["n_applied"]) == (1, 1, 1, 1), h
    assert not math.isfinite(h["sumsq_total"]) and h["clip_factor"] == 0.0
    _same_bits(before, _bits(A, True), "across the skipped step")
    assert int(A.step.item()) == 1
    ha = step(A, psA, groupsA, _grads(1))
    ht = step(T, psT, groupsT, _grads(1))
    _same_bits(_bits(A, True), _bits(T, True), "the clean step after the skipped one")
    assert not torch.equal(before["flat"], A.flat.view(torch.int32))
    assert (ha["skipped"], ha["consecutive"], ha["n_skipped"], ha["n_applied"]) == (0, 0, 1, 2), ha
    assert (ht["skipped"], ht["consecutive"], ht["n_skipped"], ht["n_applied"]) == (0, 0, 0, 2), ht
    assert ha["sumsq_total"] == ht["sumsq_total"] and ha["clip_factor"] == ht["clip_factor"]
    assert int(A.step.item()) == int(T.step.item()) == 2


def _raw_call(ar, clipnorm, desc, state):
    """fpnmt_amsgrad_step_guard called directly; the status."""
    from fpnmt import _lib as L
    from fpnmt.arena import BLOCK_ELEMS
    d = L.AdamDesc()
    d.beta1, d.beta2, d.eps, d.clipnorm, d.grad_scale = 0.9, 0.98, 1e-9, clipnorm, 1.0
    d.sched_d_model, d.const_lr = 0.0, 1e-2
    return L.lib.fpnmt_amsgrad_step_guard(
        d, 0, ar.nblocks, 1, 0, L.ptr(ar.blk_seg), L.ptr(ar.blk_start), BLOCK_ELEMS, L.ptr(ar.seg_bounds),
        L.ptr(ar.seg_flags), L.ptr(ar.flat), L.ptr(ar.grad), L.ptr(ar.m), L.ptr(ar.v), L.ptr(ar.vhat),
        L.ptr(ar.sumsq), L.ptr(ar.blk_part), L.ptr(ar.seg_blk0), L.ptr(ar.step), None, None, None, None, desc, state,
        L.stream_ptr())


def test_entry_points_refuse_both_clips_and_null_records():
    from fpnmt import _lib as L
    _require_feature()
    ar, ps, _, _ = _make(PLAIN, False, False, 1.0)
    _load(ar, ps, _grads(0), PLAIN)
    before = _bits(ar, False)
    desc, state = L.ptr(ar.guard.desc), L.ptr(ar.guard.state)
    assert _raw_call(ar, 1.0, desc, state) == L.E_ARG  # per-tensor 1.0 and global 1.0
    assert b"exclusive" in L.lib.fpnmt_last_error()
    assert _raw_call(ar, 0.0, None, state) == L.E_ARG
    assert _raw_call(ar, 0.0, desc, None) == L.E_ARG
    assert L.lib.fpnmt_grad_norm_total(ar.nblocks, L.ptr(ar.blk_seg), L.ptr(ar.seg_flags), None, L.ptr(ar.sumsq),
                                       L.ptr(ar.blk_part), L.ptr(ar.seg_blk0), 1.0, None, state,
                                       L.stream_ptr()) == L.E_ARG
    assert L.lib.fpnmt_grad_norm_total(ar.nblocks, L.ptr(ar.blk_seg), L.ptr(ar.seg_flags), None, L.ptr(ar.sumsq),
                                       L.ptr(ar.blk_part), L.ptr(ar.seg_blk0), 1.0, desc, None,
                                       L.stream_ptr()) == L.E_ARG
    torch.cuda.synchronize()
    _same_bits(before, _bits(ar, False), "a refused call")
    assert ar.guard.host()["n_applied"] == 0
    with pytest.raises(ValueError, match="exclusive"):
        ar.amsgrad_step(1e-2, clipnorm=1.0, guard=True)
    ar.set_global_clipnorm(0.0)  # the guard alone beside the per-tensor clip: accepted
    ar.amsgrad_step(1e-2, clipnorm=1.0, guard=True)
    torch.cuda.synchronize()
    assert not torch.isnan(ar.flat).any()
    assert int(ar.step.item()) == 1

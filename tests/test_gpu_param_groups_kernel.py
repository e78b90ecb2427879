"""fpnmt_amsgrad_step_groups / fpnmt_grad_sumsq_groups at the arena level (no
model): per-segment rate scale, decoupled weight decay and frozen segments,
against the fp64 reference tests/param_groups_ref.py.

Segments sit at the kernel's edges (BLOCK_ELEMS = 16384): 2*16384 + 5 elements
(three blocks: float4 body and a scalar tail), 7 elements (tail only), the
sparse (50, 16) embedding, and frozen segments first in the arena, between two
trainable ones (two blocks) and last. The bars are test_amsgrad_matches_keras's
atol 1e-6, rtol 1e-5, the project's existing bar for this kernel."""
import inspect

import numpy as np
import pytest
import torch

from param_groups_ref import GroupedAMSGradRef

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK = 16384

# name, shape, (lr_scale, weight_decay, frozen); scales from {0, 0.1, 1, 3}, decays from {0, 0.01}
SEGS = [
    ("fz_first", (70,), (3.0, 0.01, True)),
    ("big", (2 * BLOCK + 5,), (0.1, 0.01, False)),
    ("fz_mid", (BLOCK + 9,), (1.0, 0.01, True)),
    ("tiny", (7,), (3.0, 0.0, False)),
    ("emb", (50, 16), (1.0, 0.01, False)),
    ("s0", (130,), (0.0, 0.01, False)),
    ("fz_last", (33,), (0.1, 0.0, True)),
]
ROWS = {n: r for n, _, r in SEGS}


def _require_feature():
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    assert "fpnmt_amsgrad_step_groups" in L.ALL_SYMBOLS and "fpnmt_grad_sumsq_groups" in L.ALL_SYMBOLS
    assert "groups" in inspect.signature(ParamArena.amsgrad_step).parameters


def _arena(seed=0):
    from fpnmt.arena import ParamArena
    g = torch.Generator().manual_seed(seed)
    ps = [(n, torch.nn.Parameter(torch.randn(*s, generator=g))) for n, s, _ in SEGS]
    init = {n: p.detach().clone() for n, p in ps}
    ar = ParamArena(ps, DEV, sparse_names=["emb"])
    return ar, ps, init


def _rows(ar, rows=ROWS):
    return [(0,) + tuple(rows[n]) for n in ar.names]


def _grads(step, seed=100):
    g = torch.Generator().manual_seed(seed + step)
    return {n: torch.randn(*s, generator=g) * (5 if n == "big" else 0.1) for n, s, _ in SEGS}


def _load_grads(ar, ps, grads, frozen_fill):
    """Gradients into the arena; the frozen segments' gradients and every
    alignment gap hold frozen_fill (NaN: anything that reads them shows)."""
    ar.zero_grad()
    ar.grad.fill_(frozen_fill)
    for n, p in ps:
        if not ROWS[n][2]:
            p.grad.copy_(grads[n].to(DEV))
    emb_ss = float((grads["emb"].double() ** 2).sum()) * 1.7  # caller-supplied IndexedSlices norm
    ar.sumsq_slot(dict(ps)["emb"]).fill_(emb_ss)
    return emb_ss


def _seg(ar, buf, name):
    i = ar.names.index(name)
    return buf[ar.offsets[i]:ar.offsets[i] + ar.params[i].numel()]


@pytest.mark.parametrize("clipnorm", [1.0, 0.0])
@pytest.mark.parametrize("const_lr", [None, 1e-2])
def test_grouped_step_matches_fp64_reference(const_lr, clipnorm):
    from utils.utils import CustomSchedule
    _require_feature()
    sched = CustomSchedule(2048, 4000) if const_lr is None else const_lr
    lr_fn = sched if const_lr is None else (lambda it: const_lr)
    ar, ps, init = _arena()
    groups = ar.make_groups(_rows(ar))
    ar0, ps0, _ = _arena()  # the same run with zeros where the first holds NaN
    groups0 = ar0.make_groups(_rows(ar0))
    ref = GroupedAMSGradRef({n: s for n, s, _ in SEGS}, clipnorm=clipnorm, sparse=["emb"])
    params = {n: v.double().numpy().copy() for n, v in init.items()}
    frozen_names = [n for n, _, r in SEGS if r[2]]
    train_names = [n for n, _, r in SEGS if not r[2]]
    for step in range(3):
        grads = _grads(step)
        before = {k: getattr(ar, k).clone() for k in ("flat", "m", "v", "vhat")}
        emb_ss = _load_grads(ar, ps, grads, float("nan"))
        _load_grads(ar0, ps0, grads, 0.0)
        ar.amsgrad_step(sched, clipnorm=clipnorm, groups=groups)
        ar0.amsgrad_step(sched, clipnorm=clipnorm, groups=groups0)
        ref.apply(params, {n: g.double().numpy() for n, g in grads.items()}, lr_fn,
                  {n: r for n, _, r in SEGS}, norms={"emb": emb_ss})
        torch.cuda.synchronize()
        for k in ("flat", "m", "v", "vhat"):
            buf = getattr(ar, k)
            for n in frozen_names:  # bitwise what they were
                assert torch.equal(_seg(ar, buf, n), _seg(ar, before[k], n)), (step, k, n)
            assert not torch.isnan(buf).any(), (step, k)  # nothing read a frozen gradient or a gap
            for n in train_names:  # bitwise the run whose frozen gradients were zero
                assert torch.equal(_seg(ar, buf, n), _seg(ar0, getattr(ar0, k), n)), (step, k, n)
    assert int(ar.step.item()) == 3
    for n, p in ps:
        got = p.detach().cpu().double().numpy()
        d = np.abs(got - params[n]).max()
        print(f"{n}: max |p - ref| = {d:.3e}")
        assert np.allclose(got, params[n], atol=1e-6, rtol=1e-5), n
        if ROWS[n][2]:
            assert np.array_equal(got, init[n].double().numpy()), n
        for k, rk in (("m", ref.m), ("v", ref.v), ("vhat", ref.vhat)):
            s = _seg(ar, getattr(ar, k), n).cpu().double().numpy().reshape(rk[n].shape)
            assert np.allclose(s, rk[n], atol=1e-6, rtol=1e-5), (n, k)
    # lr_scale 0 without frozen: the moments advanced
    assert float(_seg(ar, ar.vhat, "s0").abs().max()) > 0


@pytest.mark.parametrize("parts", [False, True])
def test_default_table_is_bitwise_the_plain_entry_point(parts):
    """(1, 0, not frozen) everywhere: flat, m, v, vhat bitwise those of
    fpnmt_amsgrad_step_part on the same inputs, over the full range and over a
    blocks= sub-range on a persistent grid of 3 workgroups."""
    from utils.utils import CustomSchedule
    _require_feature()
    sched = CustomSchedule(2048, 4000)
    res = []
    for grouped in (False, True):
        ar, ps, _ = _arena(seed=3)
        groups = ar.make_groups([(-1, 1.0, 0.0, False)] * len(ar.params)) if grouped else None
        cut = ar.block_of(ar.offsets[ar.names.index("tiny")])
        assert 0 < cut < ar.nblocks
        for step in range(2):
            grads = _grads(step, seed=200)
            ar.zero_grad()
            for n, p in ps:
                p.grad.copy_(grads[n].to(DEV))
            ar.sumsq_slot(dict(ps)["emb"]).fill_(float((grads["emb"].double() ** 2).sum()) * 1.3)
            if parts:
                ar.amsgrad_step(sched, blocks=(0, cut), inc_step=False, max_grid=3, groups=groups)
                ar.amsgrad_step(sched, blocks=(cut, ar.nblocks), max_grid=3, groups=groups)
            else:
                ar.amsgrad_step(sched, groups=groups)
        torch.cuda.synchronize()
        assert int(ar.step.item()) == 2
        res.append({k: getattr(ar, k).clone() for k in ("flat", "m", "v", "vhat")})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert float(res[0]["vhat"].abs().max()) > 0


def test_trim_skips_frozen_head_and_tail():
    """The host does not launch the frozen head / tail blocks of a range."""
    _require_feature()
    ar, _, _ = _arena()
    groups = ar.make_groups(_rows(ar))
    first_live = ar.block_of(ar.offsets[ar.names.index("big")])
    last_live = ar.block_of(ar.offsets[ar.names.index("fz_last")])
    assert groups.trim(0, ar.nblocks) == (first_live, last_live)
    mid = ar.block_of(ar.offsets[ar.names.index("fz_mid")])
    assert groups.trim(mid, mid + 2) == (mid + 2, mid + 2)  # a wholly frozen range is empty
    # an all-frozen launch still advances the step counter
    ar.amsgrad_step(1e-2, blocks=(mid, mid + 2), groups=groups)
    torch.cuda.synchronize()
    assert int(ar.step.item()) == 1


def test_fused_refresh_follows_groups():
    """PREP with groups: a trainable conv-kernel segment with scale and decay
    gets bf16 OHWI and flipped copies equal to fpnmt_weight_prep's conversion
    of its new master (k = 16 and k = 64); a frozen segment's copies,
    pre-filled with a pattern, are untouched."""
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    from fpnmt.layers import _fastdiv
    _require_feature()
    g = torch.Generator().manual_seed(9)
    shapes = [("t16", (3, 3, 8, 16), (0.1, 0.01, False)), ("f64", (1, 1, 32, 64), (1.0, 0.0, True)),
              ("t64", (3, 3, 300, 64), (3.0, 0.01, False)), ("f16", (3, 3, 24, 16), (3.0, 0.01, True)),
              ("bias", (64,), (1.0, 0.0, False))]
    ps = [(n, torch.nn.Parameter(torch.randn(*s, generator=g) * 0.1)) for n, s, _ in shapes]
    ar = ParamArena(ps, DEV)
    rows = {n: r for n, _, r in shapes}
    groups = ar.make_groups([(0,) + rows[n] for n in ar.names])
    assert ps[2][1].numel() > 2 * BLOCK  # more than one block with a fused refresh
    tab = (L.SegPrep * len(ps))()
    copies = {}
    for i, (n, p) in enumerate(ps):
        if p.dim() != 4:
            continue
        r, s, c, k = p.shape
        ohwi = torch.full((p.numel(),), 1.25, dtype=torch.bfloat16, device=DEV)
        flip = torch.full((p.numel(),), -2.5, dtype=torch.bfloat16, device=DEV)
        copies[n] = (ohwi, flip)
        e = tab[i]
        e.ohwi, e.flip, e.scale = ohwi.data_ptr(), flip.data_ptr(), None
        e.r, e.s, e.c, e.k = r, s, c, k
        e.ld_flip = 0
        e.c_magic, e.c_shift = _fastdiv(c)
    preps = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    before = ar.flat.clone()
    for step in range(2):
        ar.zero_grad()
        ar.grad.fill_(float("nan"))
        for n, p in ps:
            if not rows[n][2]:
                p.grad.copy_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))
        ar.amsgrad_step(1e-2, preps=preps, groups=groups)
    torch.cuda.synchronize()
    for n, p in ps:
        if p.dim() != 4:
            continue
        ohwi, flip = copies[n]
        if rows[n][2]:
            assert torch.equal(p.detach(), _seg(ar, before, n).view(p.shape)), n
            assert bool((ohwi == 1.25).all()) and bool((flip == -2.5).all()), n
            continue
        assert not torch.equal(p.detach(), _seg(ar, before, n).view(p.shape)), n
        r, s, c, k = p.shape
        want_o, want_f = torch.empty_like(ohwi), torch.empty_like(flip)
        L.call("fpnmt_weight_prep", L.ptr(p), r, s, c, k, None, L.BF16, L.ptr(want_o), L.ptr(want_f), 0,
               L.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(ohwi, want_o), ("ohwi", n)
        assert torch.equal(flip, want_f), ("flip", n)
        # and the layouts themselves, from the new master
        m = p.detach().to(torch.bfloat16)
        assert torch.equal(ohwi.view(k, r, s, c), m.permute(3, 0, 1, 2).contiguous())
        assert torch.equal(flip.view(c, r, s, k), m.flip(0, 1).permute(2, 0, 1, 3).contiguous())
    assert not torch.isnan(ar.flat).any()

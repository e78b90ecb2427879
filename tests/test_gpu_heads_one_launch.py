"""The 144-row M step of the wide conv class (tile class 12 of
csrc/gemm_dispatch.h: a 160x256 LDS image, rows 144-159 fed the zero chunk)
and the planner's level partition (csrc/wide_plan.h), through the grouped
conv entry points the heads' shared 3x3 convs use.

Class 12 is forced with fpnmt_set_wide_cfg(12), which also lets small shapes
reach it. Every tile class keeps the K order per output element and the
epilogue, so the results must be bitwise those of the same call with
fpnmt_set_wide_cfg(6) (the 128-row rule: at these sizes the 64x64 loader
tiles). The levels: exactly one full 144-row tile, two full tiles and a
50-row tail, one partial tile, and a 2-row level whose tile is almost all
zero-chunk rows with every tap but the centre padded."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_IN = 64  # K = 9 * 64 = 576: 9 K-tiles, more than the ring's 3 stages
LEVELS = [(1, 12, 12), (2, 13, 13), (2, 5, 5), (2, 1, 1)]  # rows 144, 338, 50, 2


def _desc(c, k, act):
    from fpnmt import _lib as L
    d = L.ConvDesc()
    d.c, d.k, d.r, d.s = c, k, 3, 3
    d.stride_h = d.stride_w = 1
    d.pad_t = d.pad_b = d.pad_l = d.pad_r = 1
    d.dtype, d.act, d.act_alpha = L.BF16, act, 0.0
    return d


def _levels(shapes, x=None, y=None, residual=None):
    from fpnmt import _lib as L
    lv = (L.ConvLevel * len(shapes))()
    for i, (n, h, w) in enumerate(shapes):
        lv[i].n, lv[i].h, lv[i].w = n, h, w
        lv[i].x = x[i].data_ptr() if x is not None else None
        lv[i].y = y[i].data_ptr() if y is not None else None
        lv[i].residual = residual[i].data_ptr() if residual is not None and residual[i] is not None else None
    return lv


def _rand(shape, gen, scale=1.0):
    return ((torch.rand(shape, generator=gen) * 2 - 1) * scale).to(torch.bfloat16).to(DEV)


def _forced(cfg, fn):
    """fn() under fpnmt_set_wide_cfg(cfg); the hook is restored whatever happens."""
    from fpnmt import _lib as L
    try:
        L.call("fpnmt_set_wide_cfg", cfg)
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.call("fpnmt_set_wide_cfg", 0)
    return out


def _fwd(shapes, xs, w_ohwi, bias, k, act, residual=None):
    from fpnmt import _lib as L
    ys = [torch.full((n, h, w, k), 7.0, dtype=torch.bfloat16, device=DEV) for n, h, w in shapes]
    d = _desc(w_ohwi.shape[3], k, act)
    L.call("fpnmt_conv2d_fwd_grouped", d, len(shapes), _levels(shapes, xs, ys, residual), w_ohwi.data_ptr(), None,
           L.ptr(bias), L.stream_ptr())
    return ys


@pytest.mark.parametrize("k", [256, 320])  # one N tile; a ragged second N tile
def test_forward_cfg12_bitwise_and_vs_fp32(k):
    """Forward with bias + ReLU, and with a residual on every level: cfg 12
    equals cfg 6 bit for bit; the bias + ReLU form is also bounded against a
    torch CPU fp32 conv on the same bf16 operands (the output's bf16 rounding +
    1e-2 absolute, as test_conv_wide_tiles_bitwise)."""
    from fpnmt import _lib as L
    g = torch.Generator().manual_seed(12 + k)
    xs = [_rand((n, h, w, C_IN), g) for n, h, w in LEVELS]
    w_hwio = (torch.randn(3, 3, C_IN, k, generator=g) * 0.05).to(torch.bfloat16)
    w_ohwi = w_hwio.permute(3, 0, 1, 2).contiguous().to(DEV)
    bias = (torch.randn(k, generator=g) * 0.1).to(DEV)
    res = [_rand((n, h, w, k), g) for n, h, w in LEVELS]
    outs = {}
    for cfg in (6, 12):
        outs[cfg] = _forced(cfg, lambda: (_fwd(LEVELS, xs, w_ohwi, bias, k, L.ACT_RELU),
                                          _fwd(LEVELS, xs, w_ohwi, bias, k, L.ACT_RELU, res)))
    for form in (0, 1):
        for a, b in zip(outs[6][form], outs[12][form]):
            assert torch.equal(a, b)
    assert not any(torch.equal(a, b) for a, b in zip(outs[12][0], outs[12][1]))  # the residual was read
    wr = w_hwio.float().permute(3, 2, 0, 1)
    for x, y in zip(xs, outs[12][0]):
        yr = F.relu(F.conv2d(x.float().cpu().permute(0, 3, 1, 2), wr, bias.cpu(), padding=1)).permute(0, 2, 3, 1)
        err = (y.float().cpu() - yr).abs()
        print(f"k={k} level {tuple(x.shape)}: max|d| {float(err.max()):.3e} of max|ref| {float(yr.abs().max()):.3e}")
        assert float(err.max()) <= 2.0 ** -7 * float(yr.abs().max()) + 1e-2


@pytest.mark.parametrize("k", [256, 320])
def test_bwd_data_forms_cfg12_bitwise(k):
    """Every grouped bwd-data form over the same levels (dx has k channels
    here: the GEMM's N; dz has C_IN): plain, accumulating into a non-zero dx,
    with the producer's act' fused (_act), and masked (_mask, overwriting and
    accumulating): cfg 12 equals cfg 6 bit for bit."""
    from fpnmt import _lib as L
    g = torch.Generator().manual_seed(21 + k)
    # the conv being differentiated maps k -> C_IN channels, so its bwd-data is a GEMM with N = k, K = 9 * C_IN
    dzs = [_rand((n, h, w, C_IN), g, 0.5) for n, h, w in LEVELS]
    w_flip = (torch.randn(k, 3, 3, C_IN, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    y_in = [_rand((n, h, w, k), g) for n, h, w in LEVELS]  # about half of it negative: act' masks
    old = [_rand((n, h, w, k), g) for n, h, w in LEVELS]
    d = _desc(k, C_IN, L.ACT_NONE)
    s = L.stream_ptr()

    def run():
        res = {}
        for form in ("plain", "acc", "act", "mask", "mask_acc"):
            dx = [o.clone() if form in ("acc", "mask_acc") else torch.full_like(o, 7.0) for o in old]
            lv = _levels(LEVELS, dzs, dx, y_in if form in ("act", "mask", "mask_acc") else None)
            if form in ("plain", "acc"):
                L.call("fpnmt_conv2d_bwd_data_grouped", d, len(LEVELS), lv, w_flip.data_ptr(), int(form == "acc"), s)
            elif form == "act":
                L.call("fpnmt_conv2d_bwd_data_grouped_act", d, len(LEVELS), lv, w_flip.data_ptr(), L.ACT_RELU, s)
            else:
                L.call("fpnmt_conv2d_bwd_data_grouped_mask", d, len(LEVELS), lv, w_flip.data_ptr(),
                       int(form == "mask_acc"), L.ACT_RELU, s)
            res[form] = dx
        return res

    outs = {cfg: _forced(cfg, run) for cfg in (6, 12)}
    for form, dxs in outs[12].items():
        for a, b in zip(outs[6][form], dxs):
            assert torch.equal(a, b), form
    # the forms differ from each other (each operand was used), and nothing kept the fill value
    for i in range(len(LEVELS)):
        assert not torch.equal(outs[12]["plain"][i], outs[12]["acc"][i])
        assert not torch.equal(outs[12]["plain"][i], outs[12]["act"][i])
        assert not bool((outs[12]["plain"][i] == 7.0).all())
    # the fused act' is the plain dx times (y_in > 0)
    for p, a, y in zip(outs[12]["plain"], outs[12]["act"], y_in):
        assert torch.equal(a, p * (y > 0).to(p.dtype))


@pytest.mark.parametrize("n,c", [(2, 64), (32, 256)])
def test_planned_levels_delivered_once(n, c):
    """Un-forced, the five C2 level shapes (P3..P7 of a 224^2 image) in one
    grouped call: the planner's break points deliver every level exactly once,
    forward and bwd-data.
    n = 2 (64 channels: 9 K-tiles, too few for any launch to split K, so every
    partition sums in the same order): equal to one call per level.
    n = 32, 256 channels: the training step's launch, which the planner puts on
    one launch of 233 tiles of 144 rows where the 128-row rule (forced with
    cfg 6) makes P3 + P4 and a split-K launch of P5..P7; the merged launch runs
    the tail's K chains into the same slabs, so both are equal bit for bit.
    (One call per level is no reference there: P6 alone splits K four ways.)"""
    from fpnmt import _lib as L
    g = torch.Generator().manual_seed(3)
    shapes = [(n, 28, 28), (n, 14, 14), (n, 7, 7), (n, 3, 3), (n, 1, 1)]
    k = 256
    xs = [_rand((b, h, w, c), g) for b, h, w in shapes]
    w_ohwi = (torch.randn(k, 3, 3, c, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    # bwd-data of a k -> c channel conv: dz has c channels (xs serves), dx has k: a GEMM with N = k, K = 9 c
    w_flip = (torch.randn(k, 3, 3, c, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(k, generator=g) * 0.1).to(DEV)
    d = _desc(k, c, L.ACT_NONE)
    s = L.stream_ptr()
    dzs = xs

    def bwd(shp, dz):
        dx = [torch.full((b, h, w, k), 7.0, dtype=torch.bfloat16, device=DEV) for b, h, w in shp]
        L.call("fpnmt_conv2d_bwd_data_grouped", d, len(shp), _levels(shp, dz, dx), w_flip.data_ptr(), 0, s)
        return dx

    ys = _fwd(shapes, xs, w_ohwi, bias, k, L.ACT_RELU)
    dxs = bwd(shapes, dzs)
    torch.cuda.synchronize()
    if n == 2:
        for i, shp in enumerate(shapes):
            y1 = _fwd([shp], [xs[i]], w_ohwi, bias, k, L.ACT_RELU)[0]
            dx1 = bwd([shp], [dzs[i]])[0]
            torch.cuda.synchronize()
            assert torch.equal(ys[i], y1), i
            assert torch.equal(dxs[i], dx1), i
    else:
        y_in = [_rand((b, h, w, k), g) for b, h, w in shapes]

        def bwd_act():  # the producer's act' fused: the tail's reduce applies it
            dx = [torch.full_like(y, 7.0) for y in y_in]
            L.call("fpnmt_conv2d_bwd_data_grouped_act", d, len(shapes), _levels(shapes, dzs, dx, y_in),
                   w_flip.data_ptr(), L.ACT_RELU, s)
            return dx

        dxa = bwd_act()
        torch.cuda.synchronize()
        y6, dx6, dxa6 = _forced(6, lambda: (_fwd(shapes, xs, w_ohwi, bias, k, L.ACT_RELU), bwd(shapes, dzs), bwd_act()))
        for i, (a, b) in enumerate(zip(ys + dxs + dxa, y6 + dx6 + dxa6)):
            assert torch.equal(a, b), i
        for a, p_, y in zip(dxa, dxs, y_in):
            assert torch.equal(a, p_ * (y > 0).to(p_.dtype))
    for t in ys + dxs:
        assert not bool((t == 7.0).all())

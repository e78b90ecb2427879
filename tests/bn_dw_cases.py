"""Case table of the MobileNetV2 kernels (csrc/mobilenet.hip): training-mode
BatchNorm, its cross-replica entry points and the depthwise convolution.

Helper module, not collected, importable without a GPU:
tests/test_bn_dw_bars.py (no GPU) proves on an fp32 emulation of each kernel
and on planted mutations that the bounds below can fail, and checks the
`col_grid` restatement against the geometry every case records;
tests/test_gpu_bn_dw_kernels.py runs every case through the C entry points.

Reference: float64, from the exact stored inputs widened to double (the
tensors after the cast to the case dtype; for the backward also the stored y,
mean and var handed to the kernel). Every entry point gets its own inputs
exact, so the error of one stage never reaches the next; the ReLU6 mask is
taken from the stored y (0 < y < 6) and cannot flip between reference and
kernel. All functions run on the device their tensors live on (the two
grid-stride cases are computed in torch float64 on the GPU).

Bounds: per element, first order, from the arithmetic the kernel performs.
U = 2^-24 is one fp32 rounding relative to the magnitude it acts on (a fused
multiply-add only removes roundings), U64 = 2^-53 one fp64 rounding, and the
store costs 2^-8 |ref| (bf16: an 8-bit significand, so round-to-nearest is
within half an ulp = 2^-8 of the value; 2^-9 would reject the correctly rounded
reference itself, see test_bn_dw_bars) or 2^-24 |ref| (fp32). RSQ = 2^-23 is the
allowance for `rsqrtf`: HIP documents its device rsqrtf with a maximum error
of 1 ulp (it compiles to v_rsq_f32, which the CDNA ISA manual specifies at
1 ulp), and one ulp is at most 2^-23 of the value. The rounding of
`var + eps` (U on the argument, U / 2 on the root) is counted as one U.

  mean, var        U |ref| + (n + 4) U64 (sum |x - K| / n + |K|)  resp.
                   U |ref| + (n + 4) U64 2 sum (x - K)^2 / n, K the shift
                   (row 0; 0 on the sync path, whose sums are unshifted)
  moving stats     (1 - m) (bound of the statistic [+ U |unbiased var|])
                   + 2 U |moving m| + 3 U |stat (1 - m)|   (1 - m is rounded)
  sync sums        (n + 8) U64 of the sum of absolute terms (fp64 outputs)
  bn_apply         (6 U + RSQ) (|xhat gamma| + |beta| + |residual|) + store:
                   x - mean, var + eps, two products, + beta, + residual
  bn_bwd dx        |gamma rstd| ((12 U + 2 RSQ) T + (3 U + RSQ) T2) + store,
                   T = |g| + |sum g| / n + |xhat| |sum g xhat| / n,
                   T2 = |xhat| sum |g xhat| / n. Per term at most: xhat
                   3 U + RSQ, the fp32 sum U, 1 / n U, two products 2 U; two
                   subtractions 2 U; gamma rstd and the outer product
                   3 U + RSQ. T2 carries the fp32 xhat inside sum g xhat.
                   (Not |dx|: dx is a cancellation.)
  dgamma           (3 U + RSQ) sum |g xhat| + U |sum| + U |old + sum| + fp64 term
  dbeta            U |sum| + U |old + sum| + fp64 term
  depthwise fwd,   taps U sum |x w| over the taps that land inside (taps - 1
  bwd_data         additions and the product) + store
  depthwise        depth U sum |x dy| + U |old + sum|: depth = per-lane adds
  bwd_filter       ceil(ppc / RL) + RL + chunks + 1 (the product), from the
                   restated col_grid
"""
from __future__ import annotations

import dataclasses
import math

import torch
import torch.nn.functional as F

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U, U64, RSQ = 2.0 ** -24, 2.0 ** -53, 2.0 ** -23
EPS = float(torch.tensor(1e-3, dtype=F32))  # the float the entry points receive
SENTINEL = -12352.0  # exact in bf16; no output of these cases comes near it
GUARD = 64  # sentinel elements after every output
GRID_CAP = 8192  # grid_n: blocks of 256 threads, 8 channels per thread
MOMENTA = (0.9, 0.999)


def cdiv(a, b):
    return -(-a // b)


def col_grid(rows, c):
    """(gx, gy, rpc, GT, RL) of csrc/mobilenet.hip's col_grid."""
    groups = c // 8
    GT = min(groups, 256)
    RL = 256 // GT
    gx = cdiv(groups, GT)
    chunks = max(1, min(512 // gx, cdiv(rows, 4 * RL)))
    rpc = cdiv(rows, chunks)
    return gx, cdiv(rows, rpc), rpc, GT, RL


def store_u(dtype):
    return 2.0 ** -8 if dtype == BF16 else U


def f32(v):
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------ BatchNorm
@dataclasses.dataclass(frozen=True)
class BnCase:
    name: str
    rows: int
    c: int
    geom: tuple  # (gx, gy, rpc, GT, RL) the case is meant to hit
    dtypes: tuple = (F32, BF16)
    data: str = "normal"
    wrap: bool = False  # rows * c / 8 > 8192 * 256: bn_apply / bn_bwd_dx loop
    small_rows: int = 0  # the CPU emulation's row count (wrap cases)
    note: str = ""


BN_CASES = [
    BnCase("one_row", 1, 8, (1, 1, 1, 1, 256), note="rows == 1: variance 0, no Bessel factor"),
    BnCase("rows_lt_rl", 7, 48, (1, 1, 7, 6, 42), note="rows < RL = 42, one chunk"),
    BnCase("six_chunks", 1000, 48, (1, 6, 167, 6, 42),
           note="6 chunks of 167, short last chunk (165), k += 4 loop iterates, idle lanes 252-255"),
    BnCase("one_group", 3001, 8, (1, 3, 1001, 1, 256), note="groups == 1, RL = 256"),
    BnCase("rl1", 515, 1280, (1, 129, 4, 160, 1), note="RL = 1, 129 chunks of 4 (last: 3)"),
    BnCase("gx2", 70, 2056, (2, 18, 4, 256, 1),
           note="gx = 2, one live group in the second column block, c % 64 = 8"),
    BnCase("wrap", 16391, 1024, (1, 497, 33, 128, 2), dtypes=(BF16,), wrap=True, small_rows=19,
           note="n8 = 2 098 048 > 8192 * 256: the grid-stride loops of bn_apply / bn_bwd_dx"),
    # data variants at (1000, 48)
    BnCase("large_mean_f32", 1000, 48, (1, 6, 167, 6, 42), dtypes=(F32,), data="large_mean",
           note="x = 1000 + 0.01 N(0, 1): mean large against the spread"),
    BnCase("large_mean_bf16", 1000, 48, (1, 6, 167, 6, 42), dtypes=(BF16,), data="large_mean",
           note="x = 64 + N(0, 1), quantised"),
    BnCase("outlier_shift", 1000, 48, (1, 6, 167, 6, 42), data="outlier", note="row 0 (the shift) = 1e4"),
    BnCase("const_channel", 1000, 48, (1, 6, 167, 6, 42), data="const", note="channel 5 constant: variance exactly 0"),
    BnCase("saturated", 1000, 48, (1, 6, 167, 6, 42), data="saturated",
           note="stored y at exactly 0 and exactly 6 (relu6)"),
]
BN_BY_NAME = {c.name: c for c in BN_CASES}
SYNC_CASES = ["six_chunks", "rl1", "gx2"]  # run as three ranks: uneven split + one rank with zero rows
ACTS = (None, "relu6")


def sync_split(rows):
    """Row ranges of the three ranks: uneven, the third empty."""
    a = (2 * rows) // 3 + 1
    return [(0, a), (a, rows), (rows, rows)]


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) * 7919


def bn_inputs(case, dtype, rows=None):
    """Seeded CPU inputs, activations already cast to the case dtype."""
    rows = rows or case.rows
    c = case.c
    g = torch.Generator().manual_seed(_seed(case.name))
    z = torch.randn(rows, c, generator=g)
    if case.data == "large_mean":
        x = 1000 + 0.01 * z if dtype == F32 else 64 + z
    elif case.data == "outlier":
        x = z.clone()
        x[0] = 1e4
    else:
        x = 3 * z + 2
    if case.data == "const":
        x[:, 5] = 1.5
    gamma = torch.rand(c, generator=g) + 0.5
    if case.data == "saturated":
        gamma = gamma * 4
    return {
        "x": x.to(dtype), "gamma": gamma, "beta": torch.randn(c, generator=g),
        "res": torch.randn(rows, c, generator=g).to(dtype), "dy": torch.randn(rows, c, generator=g).to(dtype),
        "mm": torch.randn(c, generator=g), "mv": torch.rand(c, generator=g) + 0.5,
        "dgamma0": torch.randn(c, generator=g) * 3, "dbeta0": torch.randn(c, generator=g) * 3,
    }


def bn_stats_ref(x):
    xd = x.double()
    mean = xd.mean(0)
    return mean, ((xd - mean) ** 2).mean(0)


def bn_stats_bound(x, mean, var, shift):
    """(mean bound, var bound); shift: the K of the sums, [c] in fp64."""
    n = x.shape[0]
    d = x.double() - shift
    acc = (n + 4) * U64
    return (U * mean.abs() + acc * (d.abs().sum(0) / n + shift.abs()),
            U * var.abs() + acc * 2 * (d * d).sum(0) / n)


def bn_moving_ref(mm, mv, mean, var, n, momentum):
    """Keras moving averages in fp64 from the stored moving values: the variance
    moves toward the Bessel-corrected batch variance. Returns (mm, mv, unbiased)."""
    m = f32(momentum)
    unb = var * (n / (n - 1)) if n > 1 else var
    return mm.double() * m + mean * (1 - m), mv.double() * m + unb * (1 - m), unb


def bn_moving_bound(mm, mv, mean, unb, bmean, bvar, n, momentum):
    m = f32(momentum)
    bess = n / (n - 1) if n > 1 else 1.0
    bm = (1 - m) * bmean + 2 * U * (mm.double() * m).abs() + 3 * U * (mean * (1 - m)).abs()
    bv = (1 - m) * (bvar * bess + U * unb.abs()) + 2 * U * (mv.double() * m).abs() + 3 * U * (unb * (1 - m)).abs()
    return bm, bv


def bn_sums_ref(x, shift):
    """Unshifted fp64 sums of one rank and their bounds: (sum x, sum x^2, b1, b2)."""
    n = x.shape[0]
    xd = x.double()
    d = xd - shift
    acc = (n + 8) * U64
    k = shift.abs()
    return (xd.sum(0), (xd * xd).sum(0), acc * (d.abs().sum(0) + n * k),
            acc * ((d * d).sum(0) + 2 * k * d.abs().sum(0) + n * k * k))


def stored_stats(x):
    """The fp32 mean / var handed to bn_apply and the backward."""
    mean, var = bn_stats_ref(x)
    return mean.float(), var.float()


def bn_apply_ref(x, mean, var, gamma, beta, act, res):
    """(y, magnitude) in fp64 from the stored x / mean / var."""
    rs = (var.double() + EPS).rsqrt()
    t = (x.double() - mean.double()) * rs * gamma.double()
    o = t + beta.double()
    if act == "relu6":
        o = o.clamp(0.0, 6.0)
    mag = t.abs() + beta.double().abs()
    if res is not None:
        o = o + res.double()
        mag = mag + res.double().abs()
    return o, mag


def bn_apply_bound(y, mag, dtype):
    return (6 * U + RSQ) * mag + store_u(dtype) * y.abs()


def bn_bwd_terms(x, mean, var, act, y, dy):
    """(g, xhat, rstd) in fp64; the ReLU6 mask from the stored y."""
    rs = (var.double() + EPS).rsqrt()
    xh = (x.double() - mean.double()) * rs
    g = dy.double()
    if act == "relu6":
        g = g * ((y > 0) & (y < 6)).double()
    return g, xh, rs


def bn_bwd_sums(g, xh):
    """sum g, sum g xhat and the sums of their absolute terms, per channel."""
    gx = g * xh
    return g.sum(0), gx.sum(0), g.abs().sum(0), gx.abs().sum(0)


def bn_bwd_dx_ref(gamma, rs, g, xh, sb, sg, ag, n, dtype):
    """(dx, bound) of rows g / xh given the batch's channel sums and row count."""
    dx = gamma.double() * rs * (g - sb / n - xh * sg / n)
    T = g.abs() + sb.abs() / n + xh.abs() * sg.abs() / n
    T2 = xh.abs() * ag / n
    bnd = (gamma.double() * rs).abs() * ((12 * U + 2 * RSQ) * T + (3 * U + RSQ) * T2) + store_u(dtype) * dx.abs()
    return dx, bnd


def bn_grad_bounds(n, sb, sg, ab, ag, old_b, old_g):
    """(dbeta bound, dgamma bound) of old + sum."""
    acc = (n + 4) * U64
    return (U * sb.abs() + U * (old_b.double() + sb).abs() + acc * ab,
            (3 * U + RSQ) * ag + U * sg.abs() + U * (old_g.double() + sg).abs() + acc * ag)


def bn_bwd_sums_bounds(n, ab, ag):
    """Bounds of the sync path's fp64 (sum g, sum g xhat)."""
    acc = (n + 8) * U64
    return acc * ab, (3 * U + RSQ + acc) * ag


# ------------------------------------------------------------------ depthwise
@dataclasses.dataclass(frozen=True)
class DwCase:
    name: str
    shape: tuple  # n, h, w, c
    k: tuple  # kh, kw
    stride: int
    pads: tuple  # t, b, l, r
    geom: tuple  # col_grid(n ho wo, c) of bwd_filter
    dtypes: tuple = (F32, BF16)
    wrap: bool = False  # fwd / bwd_data only (the kernels with a grid-stride loop)
    small: tuple = ()  # the CPU emulation's shape (wrap case)
    note: str = ""

    def out_hw(self, shape=None):
        n, h, w, c = shape or self.shape
        (kh, kw), st, (pt, pb, pl, pr) = self.k, self.stride, self.pads
        return (h + pt + pb - kh) // st + 1, (w + pl + pr - kw) // st + 1


_S = (1, 1, 1, 1)
DW_CASES = [
    DwCase("mn_14x14x96", (2, 14, 14, 96), (3, 3), 1, _S, (1, 5, 79, 12, 21)),
    DwCase("mn_s2_14x12x32", (3, 14, 12, 32), (3, 3), 2, (0, 1, 0, 1), (1, 1, 126, 4, 64)),
    DwCase("mn_s2_7x7x16", (2, 7, 7, 16), (3, 3), 2, (0, 1, 0, 1), (1, 1, 18, 2, 128)),
    DwCase("mn_5x6x8", (1, 5, 6, 8), (3, 3), 1, _S, (1, 1, 30, 1, 256)),
    DwCase("one_pixel", (1, 1, 1, 8), (3, 3), 1, _S, (1, 1, 1, 1, 256), note="1x1 image: one tap inside"),
    DwCase("s2_odd", (2, 5, 7, 8), (3, 3), 2, (0, 1, 0, 1), (1, 1, 12, 1, 256)),
    DwCase("s2_floor_drop", (2, 6, 8, 16), (3, 3), 2, _S, (1, 1, 24, 2, 128),
           note="floor division drops the bottom / right padding row"),
    DwCase("s2_drop_row", (2, 7, 9, 16), (3, 3), 2, (1, 0, 1, 0), (1, 1, 24, 2, 128),
           note="the last input row / column lies beyond every tap: dx exactly zero there"),
    DwCase("stride3", (1, 10, 10, 8), (3, 3), 3, (0, 0, 0, 0), (1, 1, 9, 1, 256)),
    DwCase("k2x2", (2, 6, 7, 24), (2, 2), 1, (0, 1, 0, 1), (1, 1, 84, 3, 85),
           note="kw = 2: accumulator index r * 3 + s against output index r * kw + s"),
    DwCase("k1x3", (1, 4, 9, 24), (1, 3), 1, (0, 0, 1, 1), (1, 1, 36, 3, 85)),
    DwCase("k3x1", (1, 9, 4, 24), (3, 1), 1, (1, 1, 0, 0), (1, 1, 36, 3, 85)),
    DwCase("c2056", (1, 6, 6, 2056), (3, 3), 1, _S, (2, 9, 4, 256, 1), note="c > 2048: gx = 2"),
    DwCase("seven_chunks", (4, 40, 40, 8), (3, 3), 1, _S, (1, 7, 915, 1, 256), note="6400 pixels, RL 256, 7 chunks"),
    DwCase("wrap", (2, 129, 128, 512), (3, 3), 1, _S, (1, 509, 65, 64, 4), dtypes=(BF16,), wrap=True,
           small=(1, 5, 7, 512), note="2 113 536 work items: the grid-stride loops of dw_fwd / dw_bwd_data"),
]
DW_BY_NAME = {c.name: c for c in DW_CASES}


def dw_inputs(case, dtype, shape=None):
    shape = shape or case.shape
    n, h, w, c = shape
    ho, wo = case.out_hw(shape)
    g = torch.Generator().manual_seed(_seed("dw_" + case.name))
    return {"x": torch.randn(n, h, w, c, generator=g).to(dtype), "w": torch.randn(*case.k, c, generator=g) * 0.5,
            "dy": torch.randn(n, ho, wo, c, generator=g).to(dtype), "dw0": torch.randn(*case.k, c, generator=g) * 3}


def _pad(t, pads):
    pt, pb, pl, pr = pads
    return F.pad(t, (0, 0, pl, pr, pt, pb))


def _tap(tp, r, s, ho, wo, st):
    return tp[:, r:r + (ho - 1) * st + 1:st, s:s + (wo - 1) * st + 1:st, :]


def dw_fwd_ref(case, x, w):
    """(y, sum |x w|, taps inside) in fp64."""
    n, h, wd, c = x.shape
    ho, wo = case.out_hw(tuple(x.shape))
    xp, op = _pad(x.double(), case.pads), _pad(torch.ones(1, h, wd, 1, dtype=F64, device=x.device), case.pads)
    y = torch.zeros(n, ho, wo, c, dtype=F64, device=x.device)
    S, cnt = torch.zeros_like(y), torch.zeros(1, ho, wo, 1, dtype=F64, device=x.device)
    for r in range(case.k[0]):
        for s in range(case.k[1]):
            t = _tap(xp, r, s, ho, wo, case.stride) * w[r, s].double()
            y += t
            S += t.abs()
            cnt += _tap(op, r, s, ho, wo, case.stride)
    return y, S, cnt


def dw_bwd_data_ref(case, dy, w, shape):
    """(dx, sum |dy w|, taps reaching the pixel) in fp64; shape: the input's."""
    n, h, wd, c = shape
    ho, wo = case.out_hw(shape)
    pt, pb, pl, pr = case.pads
    hp, wp = max(h + pt + pb, (ho - 1) * case.stride + case.k[0]), max(wd + pl + pr, (wo - 1) * case.stride + case.k[1])
    dx = torch.zeros(n, hp, wp, c, dtype=F64, device=dy.device)
    S, cnt = torch.zeros_like(dx), torch.zeros(1, hp, wp, 1, dtype=F64, device=dy.device)
    for r in range(case.k[0]):
        for s in range(case.k[1]):
            t = dy.double() * w[r, s].double()
            _tap(dx, r, s, ho, wo, case.stride).add_(t)
            _tap(S, r, s, ho, wo, case.stride).add_(t.abs())
            _tap(cnt, r, s, ho, wo, case.stride).add_(1.0)
    crop = lambda t: t[:, pt:pt + h, pl:pl + wd, :].contiguous()
    return crop(dx), crop(S), crop(cnt)


def dw_data_bound(ref, S, cnt, dtype):
    return cnt * U * S + store_u(dtype) * ref.abs()


def dw_bwd_filter_ref(case, x, dy):
    """(dw, sum |x dy|) in fp64, (kh, kw, c)."""
    ho, wo = case.out_hw(tuple(x.shape))
    xp, d = _pad(x.double(), case.pads), dy.double()
    out = torch.zeros(*case.k, x.shape[3], dtype=F64, device=x.device)
    S = torch.zeros_like(out)
    for r in range(case.k[0]):
        for s in range(case.k[1]):
            t = _tap(xp, r, s, ho, wo, case.stride) * d
            out[r, s] = t.sum((0, 1, 2))
            S[r, s] = t.abs().sum((0, 1, 2))
    return out, S


def dw_filter_depth(npix, c):
    gx, gy, ppc, GT, RL = col_grid(npix, c)
    return cdiv(ppc, RL) + RL + gy + 1


def dw_filter_bound(case, shape, dwsum, S, old):
    n, h, w, c = shape
    ho, wo = case.out_hw(shape)
    return dw_filter_depth(n * ho * wo, c) * U * S + U * (old.double() + dwsum).abs()


# ------------------------------------------------------------------ comparing
def compare(out, ref, bnd):
    """(all elements inside the bound, worst err / bound)."""
    err = (out.double() - ref).abs()
    bad = ~(err <= bnd)  # a NaN is outside
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return not bool(bad.any()), float(ratio.max()) if ratio.numel() else 0.0


# --------------------------------------------------------------------- suites
# One walk over a case's entry points, shared by the CPU emulation
# (tests/test_bn_dw_bars.py) and the GPU (tests/test_gpu_bn_dw_kernels.py):
# `impl` supplies the entry points, the walk supplies stored inputs, fp64
# references and bounds and returns (label, output, reference, bound) rows.
def bn_sync_stats_bound(n, mean, var, b1, b2, sx2):
    """mean = S1 / n, var = S2 / n - mean^2 in fp64 from all-reduced sums that
    carry the errors b1, b2; one fp32 rounding of each result."""
    return (U * mean.abs() + b1 / n + 4 * U64 * mean.abs(),
            U * var.abs() + b2 / n + 2 * mean.abs() * b1 / n + 4 * U64 * (sx2 / n + mean * mean))


def _moving_rows(tag, inp, got, mean64, var64, bm, bv, n, mom):
    mean, var, mm, mv = got
    rmm, rmv, unb = bn_moving_ref(inp["mm"], inp["mv"], mean64, var64, n, mom)
    bmm, bmv = bn_moving_bound(inp["mm"], inp["mv"], mean64, unb, bm, bv, n, mom)
    return [(f"{tag}.mean[{mom}]", mean, mean64, bm), (f"{tag}.var[{mom}]", var, var64, bv),
            (f"{tag}.moving_mean[{mom}]", mm, rmm, bmm), (f"{tag}.moving_var[{mom}]", mv, rmv, bmv)]


def bn_suite(case, dtype, impl, dev="cpu", rows=None):
    inp = {k: v.to(dev) for k, v in bn_inputs(case, dtype, rows).items()}
    x, gamma, beta, dy = inp["x"], inp["gamma"], inp["beta"], inp["dy"]
    n = x.shape[0]
    mean64, var64 = bn_stats_ref(x)
    out = []
    if not case.wrap:  # the wrap case: only the entry points with a grid-stride loop
        bm, bv = bn_stats_bound(x, mean64, var64, x[0].double())
        for mom in MOMENTA:
            out += _moving_rows("stats", inp, impl.stats(x, inp["mm"], inp["mv"], mom), mean64, var64, bm, bv, n, mom)
        mean, var, _, _ = impl.stats(x, None, None, MOMENTA[0])  # both moving pointers null
        out += [("stats.mean[null]", mean, mean64, bm), ("stats.var[null]", var, var64, bv)]
    smean, svar = mean64.float(), var64.float()
    for act in ACTS:
        for res in (None, inp["res"]):
            ref, mag = bn_apply_ref(x, smean, svar, gamma, beta, act, res)
            y = impl.apply(x, smean, svar, gamma, beta, act, res)
            out.append((f"apply[{act},{'res' if res is not None else '-'}]", y, ref, bn_apply_bound(ref, mag, dtype)))
    for act in ACTS:
        ys = bn_apply_ref(x, smean, svar, gamma, beta, act, None)[0].to(dtype) if act else None  # the stored y
        g, xh, rs = bn_bwd_terms(x, smean, svar, act, ys, dy)
        sb, sg, ab, ag = bn_bwd_sums(g, xh)
        dxr, dxb = bn_bwd_dx_ref(gamma, rs, g, xh, sb, sg, ag, n, dtype)
        bb, bg = bn_grad_bounds(n, sb, sg, ab, ag, inp["dbeta0"], inp["dgamma0"])
        dx, dg, db = impl.bwd(x, smean, svar, gamma, act, ys, dy, inp["dgamma0"], inp["dbeta0"])
        out += [(f"bwd.dx[{act}]", dx, dxr, dxb), (f"bwd.dgamma[{act}]", dg, inp["dgamma0"].double() + sg, bg),
                (f"bwd.dbeta[{act}]", db, inp["dbeta0"].double() + sb, bb)]
        if act is None:  # null gradient accumulators
            dx, _, _ = impl.bwd(x, smean, svar, gamma, act, ys, dy, None, None)
            out.append(("bwd.dx[None,null grads]", dx, dxr, dxb))
    return out


def bn_sync_suite(case, dtype, impl, dev="cpu"):
    """The sync entry points as three ranks in one process (no process group)."""
    inp = {k: v.to(dev) for k, v in bn_inputs(case, dtype).items()}
    x, gamma, beta, dy = inp["x"], inp["gamma"], inp["beta"], inp["dy"]
    n, c = x.shape
    ranks = sync_split(n)
    z = lambda k=c: torch.zeros(k, dtype=F64, device=dev)
    mean64, var64 = bn_stats_ref(x)
    out = []
    tot, b1, b2 = z(2 * c + 1), z(), z()
    for i, (a, b) in enumerate(ranks):
        sums = impl.stats_sums(x[a:b])
        tot = tot + sums.double()
        if b > a:
            s1, s2, e1, e2 = bn_sums_ref(x[a:b], x[a].double())
            b1, b2 = b1 + e1, b2 + e2
            out.append((f"sync.sums[rank {i}]", sums[:2 * c], torch.cat([s1, s2]), torch.cat([e1, e2])))
        else:
            out.append((f"sync.sums[rank {i}, no rows]", sums[:2 * c], z(2 * c), z(2 * c)))
        out.append((f"sync.count[rank {i}]", sums[2 * c:], torch.full((1,), float(b - a), dtype=F64, device=dev), z(1)))
    out.append(("sync.count[total]", tot[2 * c:], torch.full((1,), float(n), dtype=F64, device=dev), z(1)))
    xd = x.double()
    sx2 = (xd * xd).sum(0)
    b1, b2 = b1 + 3 * U64 * xd.sum(0).abs(), b2 + 3 * U64 * sx2  # the adds over the ranks
    bm, bv = bn_sync_stats_bound(n, mean64, var64, b1, b2, sx2)
    for mom in MOMENTA:
        out += _moving_rows("sync.finalize", inp, impl.finalize(tot, inp["mm"], inp["mv"], mom), mean64, var64, bm,
                            bv, n, mom)
    smean, svar = mean64.float(), var64.float()
    for act in ACTS:
        ys = bn_apply_ref(x, smean, svar, gamma, beta, act, None)[0].to(dtype) if act else None
        g, xh, rs = bn_bwd_terms(x, smean, svar, act, ys, dy)
        sb, sg, ab, ag = bn_bwd_sums(g, xh)
        dxr, dxb = bn_bwd_dx_ref(gamma, rs, g, xh, sb, sg, ag, n, dtype)
        tot, cg, cb, bgs, bbs = z(2 * c + 1), z(), z(), z(), z()
        for i, (a, b) in enumerate(ranks):
            sums, dg, db = impl.bwd_sums(x[a:b], smean, svar, act, None if ys is None else ys[a:b], dy[a:b],
                                         inp["dgamma0"], inp["dbeta0"])
            tot = tot + sums.double()
            rb, rg, rab, rag = bn_bwd_sums(g[a:b], xh[a:b])
            eb, eg = bn_bwd_sums_bounds(b - a, rab, rag)
            bb, bg = bn_grad_bounds(b - a, rb, rg, rab, rag, inp["dbeta0"], inp["dgamma0"])
            if b == a:  # zero rows: zero sums, the gradients untouched
                eb, eg, bb, bg = z(), z(), z(), z()
            out += [(f"sync.bwd_sums[{act},rank {i}]", sums[:2 * c], torch.cat([rb, rg]), torch.cat([eb, eg])),
                    (f"sync.bwd_count[{act},rank {i}]", sums[2 * c:],
                     torch.full((1,), float(b - a), dtype=F64, device=dev), z(1)),
                    (f"sync.dgamma[{act},rank {i}]", dg, inp["dgamma0"].double() + rg, bg),
                    (f"sync.dbeta[{act},rank {i}]", db, inp["dbeta0"].double() + rb, bb)]
            cg, cb = cg + (dg.double() - inp["dgamma0"].double()), cb + (db.double() - inp["dbeta0"].double())
            bgs, bbs = bgs + bg, bbs + bb
        # the ranks' contributions add to the whole batch's gradient
        out += [(f"sync.dgamma[{act},ranks added]", cg, sg, bgs), (f"sync.dbeta[{act},ranks added]", cb, sb, bbs)]
        for i, (a, b) in enumerate(ranks[:2]):
            dx = impl.bwd_dx(x[a:b], smean, svar, gamma, act, None if ys is None else ys[a:b], dy[a:b], tot, i)
            out.append((f"sync.dx[{act},rank {i}]", dx, dxr[a:b], dxb[a:b]))
    return out


def dw_suite(case, dtype, impl, dev="cpu", shape=None):
    inp = {k: v.to(dev) for k, v in dw_inputs(case, dtype, shape).items()}
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    shape = tuple(x.shape)
    ref, S, cnt = dw_fwd_ref(case, x, w)
    out = [("dw.fwd", impl.dw_fwd(case, x, w), ref, dw_data_bound(ref, S, cnt, dtype))]
    ref, S, cnt = dw_bwd_data_ref(case, dy, w, shape)
    out.append(("dw.bwd_data", impl.dw_bwd_data(case, dy, w, shape), ref, dw_data_bound(ref, S, cnt, dtype)))
    if not case.wrap:  # no grid-stride loop in the filter gradient
        ref, S = dw_bwd_filter_ref(case, x, dy)
        out.append(("dw.bwd_filter", impl.dw_bwd_filter(case, x, dy, inp["dw0"]), inp["dw0"].double() + ref,
                    dw_filter_bound(case, shape, ref, S, inp["dw0"])))
    return out


def worst(rows):
    """({label: worst err / bound}, labels outside their bound)."""
    ratios, bad = {}, []
    for label, got, ref, bnd in rows:
        assert got.shape == ref.shape == bnd.shape, (label, got.shape, ref.shape, bnd.shape)
        ok, r = compare(got, ref, bnd)
        ratios[label] = r
        if not ok:
            bad.append(label)
    return ratios, bad

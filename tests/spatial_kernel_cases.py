"""Case table of the spatial kernels of csrc/elementwise.hip, the image
branch's pooling, FPN top-down pathway and co-attention spatial softmax:
maxpool_fwd_kernel<T, 8 | 1>, maxpool_bwd_kernel<T, 8 | 1> (the gather form,
with a stored argmax or recomputing it from x), maxpool3s2_bwd_kernel (the
2x2-block form of the ResNet stem pool), the fused activation-derivative
variant fpnmt_maxpool2d_bwd_act, fpn_fwd_kernel / fpn_bwd_kernel (with the
"upsample" form h3 = w3 = 0 and accumulate_lat5) and ssm_fwd_kernel /
ssm_bwd1_kernel / ssm_bwd2_kernel.

Helper module, not collected, importable without a GPU:
tests/test_spatial_kernel_bars.py (no GPU) proves on an fp32 / bf16 emulation
of each kernel and on planted mutations that the bounds below can fail and
checks the restated host geometry against what every case records;
tests/test_gpu_spatial_kernels.py runs every case through the C entry points.
The constants, `compare` and `worst` are those of tests/row_kernel_cases.py.

Reference: float64, from the exact stored inputs of each entry point widened
to double. Where a second stage consumes a value the first stage rounds to the
storage dtype, the second stage is judged from the value the entry point
stored: P3m from the stored P4m, d_lat5 from the stored d_lat4 (the rounded
d_p4m total), d_hs / d_score from the stored fp32 a, d_score from the stored
fp64 da. NaN inputs are out of scope: today the first valid tap of a pooling
window wins if it is NaN and later NaNs are ignored.

The nearest-resize index map is the fp32 formula the kernel (nn_src) and
oracle/ref_cpu.py::nearest_index evaluate, TensorFlow's
floorf((d + 0.5f) * ((float)in / (float)out)) clamped to in - 1, restated by
`nn_src_f32` in numpy.float32; never the exact rational
floor((2 d + 1) in / (2 out)) (`nn_src_exact`). The two differ: the fp32
quotient in / out is rounded, which moves (d + 0.5) * (in / out) across an
integer the rational sits on. Among all (in, out) up to 96 they differ for 132
pairs (`differing_pairs`), e.g. 14 -> 23 (d = 11: 11.5 * 14 / 23 = 7 exactly, fp32 gives 6: its quotient
rounds down), 8 -> 41,
4 -> 41, 6 -> 37; the case fpn `fp32_index` resizes 14 -> 23. An integer
rewrite of nn_src would silently leave TensorFlow's behaviour.

Bounds: per element, first order, counted from the arithmetic. U = 2^-24 one
fp32 rounding, EXPU = 2^-23 for expf, the store 2^-8 |ref| (bf16) or
2^-24 |ref| (fp32). A sum whose chain has `depth` additions is within
depth U sum |terms| of the exact sum.

  pool y, argmax   exact: y bitwise the maximum of the window's valid taps,
                   argmax the first maximum in (r, q) order; no valid tap:
                   y = -inf, argmax 255 (bound zero: no rounding)
  pool dx          k terms of dy in window order (oh, then ow, ascending):
                   (k - 1) U sum |terms| + store; k <= 1: exact (zero
                   roundings); no contributing window: exactly +0. The 0 / 1
                   masks of relu / relu6 keep the bound; leaky adds U |ref|
                   (one product) where the factor is the slope
  fpn p4m, p3m     (U + store) |ref|: the fp32 sum, the store; fp32: the store
                   term alone (a single rounding). p3m from the stored p4m
  fpn d_lat4       depth U sum |terms| + store, depth = the children of the P4
                   pixel (one addition each onto d_p4m); no child: exact
  fpn d_lat5       depth U sum |terms| + store over the stored d_lat4 of the
                   children, depth = children + 1 under accumulate_lat5 (the
                   old value is a term); a chain without an addition (one
                   child, no child, old alone) is exact
  ssm a            e_j = exp(x_j - m), s = sum e_j, eps_s = sum e_j (U |x_j - m|
                   + EXPU) / s + (ceil(hw / 256) + 6 + 3) U (thread adds,
                   butterfly, the four waves); a (U |x - m| + EXPU + eps_s + U):
                   the subtraction moves the exponent, expf, the sum, the
                   division
  ssm ctx          (U + store) |ref| from the stored a: the kernel recomputes
                   a with the same three fp32 operations it stored, so the
                   tighter form holds (the looser one, the bound of a times
                   |hs| plus this, is not needed); the product, the store
  ssm d_hs         (U + store) |ref| from the stored a
  ssm da           (ceil(c / 64) + 6) 2^-53 sum |terms|: products of two fp32
                   values are exact in fp64; lane adds, butterfly
  ssm d_score      (U + store) |ref| + a (ceil(hw / 256) + 6 + 3 + 1) 2^-53
                   sum |a da| from the stored a and da: the fp64 weighted sum
                   (products 1, thread adds, butterfly, waves), then one fp32
                   rounding and the store. Never relative to |d_score| alone
                   in the sum term: d_score is a cancellation.
  The fp32 softmax outputs (a, ctx, d_hs, d_score) carry TINY = 2^-126
  (absolute) as the cross-entropy's dlogits do: the peaked cases reach
  exp(-300), where results underflow to subnormals or zero.

The grid-stride loops of maxpool_fwd_kernel and maxpool_bwd_kernel are reached
on the scalar route (`loop_840`) and with VN = 8 (`loop_840_c24`). The loop of
the tile form is left out: its work items are pooled windows x 8 channels, so
passing 8192 x 256 of them takes a 1680 x 1680 x 24 input (68 M elements),
whose seeded inputs and fp64 reference alone take longer than a test may; the
loop statement is the one the other two kernels share.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from row_kernel_cases import (BF16, EXPU, F32, F64, GUARD, SENTINEL, TINY, U, _seed, cdiv, compare, grid_for,  # noqa: F401
                              short, store_u, worst)

D53 = 2.0 ** -53
AM_SENTINEL = 0xA5  # no tap index (<= 8) and not 255
POOL_CAP, SSM_BWD_CAP, FLAT_CAP = 8192, 8192, 4096
LEAKY = 0.2
ACT_CODE = {"relu": 1, "leaky": 2, "relu6": 3}  # FPNMT_ACT_*


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------ geometry
def nn_src_f32(out, inp):
    """nn_src for d = 0 .. out - 1 in numpy.float32: TensorFlow's formula."""
    d = np.arange(out, dtype=np.float32)
    s = np.floor((d + np.float32(0.5)) * (np.float32(inp) / np.float32(out))).astype(np.int64)
    return np.minimum(s, inp - 1)


def nn_src_exact(out, inp):
    d = np.arange(out, dtype=np.int64)
    return np.minimum(((2 * d + 1) * inp) // (2 * out), inp - 1)


def differing_pairs(limit=96):
    return {(i, o) for i in range(1, limit + 1) for o in range(1, limit + 1)
            if not np.array_equal(nn_src_f32(o, i), nn_src_exact(o, i))}


def nn_children(s, inp, out, src=None):
    """[lo, hi) as the kernel's nn_children finds it: from the starting guess
    s * out / in - 2, the first d with src == s up to the first with src > s."""
    src = nn_src_f32(out, inp) if src is None and out > 0 else src
    d0 = max((s * out) // inp - 2, 0)
    lo = hi = -1
    for d in range(d0, out):
        if src[d] == s and lo < 0:
            lo = d
        if src[d] > s:
            hi = d
            break
    if lo < 0:
        return 0, 0
    return lo, out if hi < 0 else hi


def children_table(inp, out):
    """[in, 2] int64 (lo, hi) of every source pixel."""
    src = nn_src_f32(out, inp) if out > 0 else None
    return torch.tensor([nn_children(s, inp, out, src) for s in range(inp)], dtype=torch.int64).view(inp, 2)


def children_brute(s, inp, out):
    d = np.nonzero(nn_src_f32(out, inp) == s)[0]
    return (int(d[0]), int(d[-1]) + 1) if len(d) else (0, 0)


def pool_vec(c, aligned=True):
    return c % 8 == 0 and aligned


def pool_bwd_route(case, aligned=True, argmax=True):
    """maxpool_launch's backward route: zero_fill, tile (maxpool3s2_bwd_kernel),
    gather8 or gather1."""
    k = case
    if k.ho <= 0 or k.wo <= 0:
        return "zero_fill"
    vec = pool_vec(k.c, aligned)
    if vec and argmax and (k.kh, k.kw, k.sh, k.sw) == (3, 3, 2, 2) and 0 <= k.pt < 2 and 0 <= k.pl < 2 \
            and 2 * k.ho - k.pt >= k.h and 2 * k.wo - k.pl >= k.w:
        return "tile"
    return "gather8" if vec else "gather1"


def pool_loops(case, aligned=True):
    """(forward, gather backward) grid-stride loops taken."""
    k = case
    vn = 8 if pool_vec(k.c, aligned) else 1
    tf, tb = k.n * k.ho * k.wo * (k.c // vn), k.n * k.h * k.w * (k.c // vn)
    return tf > grid_for(tf, 256, POOL_CAP) * 256, tb > grid_for(tb, 256, POOL_CAP) * 256


def fpn_loop(n, cg, *sizes):
    """Work items of an fpn launch over the two grids given as (h, w, h, w) exceed the grid."""
    tot = n * cg * (sizes[0] * sizes[1] + sizes[2] * sizes[3])
    return tot > grid_for(tot, 256, FLAT_CAP) * 256


def ssm_chunks(hw, c):
    """(chunks, chunk) of fpnmt_spatial_softmax_fwd."""
    chunks = max(1, min(hw, hw * c // 8192))
    chunk = cdiv(hw, chunks)
    return cdiv(hw, chunk), chunk


def ssm_bwd_loop(n, hw):
    return n * hw > 4 * grid_for(n * hw, 4, SSM_BWD_CAP)


# ------------------------------------------------------------------- max pool
@dataclasses.dataclass(frozen=True)
class PoolCase:
    name: str
    n: int
    h: int
    w: int
    c: int
    kh: int
    kw: int
    sh: int
    sw: int
    pt: int
    pl: int
    ho: int
    wo: int
    routes: tuple  # backward launches: (route expected, argmax given, pointer offset in elements)
    acts: tuple = ()  # fused activation derivatives, on the first route
    datas: tuple = ("ties", "inf", "randn")
    loops: tuple = (False, False)
    small: tuple = ()  # (h, w, ho, wo) the emulation runs at
    note: str = ""

    @property
    def geo(self):
        return (self.n, self.h, self.w, self.c, self.kh, self.kw, self.sh, self.sw, self.pt, self.pl, self.ho, self.wo)


_T3 = (("tile", True, 0), ("gather8", False, 0), ("gather1", True, 1))
_G2 = (("gather8", True, 0), ("gather8", False, 0))
POOL_CASES = [
    PoolCase("same_8x10", 2, 8, 10, 16, 3, 3, 2, 2, 0, 0, 4, 5, _T3, acts=("relu", "relu6"),
             note="'same' 3x3/2, pt = pl = 0: tile form = gather with recompute = scalar gather by alignment"),
    PoolCase("same_9x7", 2, 9, 7, 8, 3, 3, 2, 2, 1, 1, 5, 4, _T3, note="'same' 3x3/2, pt = pl = 1; all three routes"),
    PoolCase("same_5x6", 1, 5, 6, 24, 3, 3, 2, 2, 1, 0, 3, 3, (("tile", True, 0),), note="pt = 1, pl = 0; c = 24"),
    PoolCase("same_1x1", 1, 1, 1, 8, 3, 3, 2, 2, 1, 1, 1, 1, (("tile", True, 0),), note="one pixel, one window"),
    PoolCase("c6", 2, 9, 11, 6, 3, 3, 2, 2, 1, 1, 5, 6, (("gather1", True, 0), ("gather1", False, 0)),
             acts=("relu", "relu6"), note="c = 6: the scalar route by channel count"),
    PoolCase("valid_7x7", 2, 7, 7, 16, 2, 2, 2, 2, 0, 0, 3, 3, _G2, acts=("leaky", "relu"),
             note="'valid' 2x2/2: the last row and column belong to no window"),
    PoolCase("valid_6x8", 2, 6, 8, 8, 2, 2, 2, 2, 0, 0, 3, 4, _G2, acts=("leaky",), note="'valid' 2x2/2, all covered"),
    PoolCase("valid_1x1", 1, 1, 1, 8, 2, 2, 2, 2, 0, 0, 0, 0, (("zero_fill", True, 0),),
             note="ho = wo = 0: the zero_fill path"),
    PoolCase("k3s1_6x5", 1, 6, 5, 8, 3, 3, 1, 1, 1, 1, 6, 5, _G2, acts=("relu6",),
             note="3x3/1 pad 1: up to nine windows per input"),
    PoolCase("k2x3_s3x2", 1, 8, 9, 8, 2, 3, 3, 2, 0, 0, 3, 4, _G2, note="stride 3 over kernel 2: uncovered input rows"),
    PoolCase("oversize_k2", 1, 4, 5, 8, 2, 2, 2, 2, 0, 0, 4, 4, _G2,
             note="ho / wo beyond the input: windows with no valid tap (argmax 255, y = -inf)"),
    PoolCase("oversize_tile", 1, 4, 4, 8, 3, 3, 2, 2, 0, 0, 3, 3, _T3,
             note="the same on the tile route: 255 must route nowhere"),
    PoolCase("loop_840", 1, 840, 840, 3, 3, 3, 1, 1, 1, 1, 840, 840, (("gather1", True, 0),), datas=("ties",),
             loops=(True, True), small=(12, 13, 12, 13), note="grid-stride loops, forward and backward, scalar route"),
    PoolCase("loop_840_c24", 1, 840, 840, 24, 3, 3, 1, 1, 1, 1, 840, 840, (("gather8", True, 0),), datas=("ties",),
             loops=(True, True), small=(12, 13, 12, 13), note="the same loops with VN = 8"),
]
POOL_BY_NAME = {c.name: c for c in POOL_CASES}
POOL_DTYPES = (F32, BF16)
# error returns of fpnmt_maxpool2d_bwd_act: (case, act code, why)
POOL_ACT_ERRORS = (("same_8x10", ACT_CODE["leaky"], "leaky with overlapping windows"), ("valid_7x7", 0, "act none"),
                   ("valid_7x7", 7, "unknown act"))


def pool_small(case):
    if not case.small:
        return case
    h, w, ho, wo = case.small
    return dataclasses.replace(case, h=h, w=w, ho=ho, wo=wo, small=(), loops=(False, False))


def pool_inputs(case, dtype, data):
    g = torch.Generator().manual_seed(_seed(f"pool_{case.name}_{data}"))
    n, h, w, c = case.n, case.h, case.w, case.c
    if data == "randn":
        x = torch.randn(n, h, w, c, generator=g)
    else:
        x = torch.randint(0, 3, (n, h, w, c), generator=g).float()  # ties everywhere
    if data == "inf":
        x[:, :min(h, 3), :min(w, 3)] = -np.inf  # whole windows
        x[torch.rand(n, h, w, c, generator=g) < 0.1] = -np.inf  # single taps
    dy = torch.randn(n, max(case.ho, 0), max(case.wo, 0), c, generator=g)
    out = {"x": x.to(dtype), "dy": dy.to(dtype)}
    if case.acts or case.name in {e[0] for e in POOL_ACT_ERRORS}:
        # the producer's output under the pool: straddles 0 and 6, exact 0.0 and 6.0 entries
        xa = (4 * torch.randn(n, h, w, c, generator=g) + 3).clamp(-2.0, 8.0)
        u = torch.rand(n, h, w, c, generator=g)
        out["xact"] = torch.where(u < 0.1, torch.zeros(()), torch.where(u > 0.9, torch.full((), 6.0), xa)).to(dtype)
    return out


def _taps(case, dev):
    k = case
    oh, ow = torch.arange(k.ho, device=dev), torch.arange(k.wo, device=dev)
    for r in range(k.kh):
        for q in range(k.kw):
            ih, iw = oh * k.sh - k.pt + r, ow * k.sw - k.pl + q
            valid = ((ih >= 0) & (ih < k.h))[:, None] & ((iw >= 0) & (iw < k.w))[None, :]
            yield r * k.kw + q, ih.clamp(0, k.h - 1), iw.clamp(0, k.w - 1), valid[None, :, :, None]


def pool_fwd_ref(case, x):
    """(y fp64, argmax uint8): the maximum of the valid taps, its first tap."""
    xd = x.double()
    n, c, dev = case.n, case.c, x.device
    m = torch.full((n, case.ho, case.wo, c), -np.inf, dtype=F64, device=dev)
    for _, ih, iw, valid in _taps(case, dev):
        m = torch.where(valid, torch.maximum(m, xd[:, ih][:, :, iw]), m)
    am = torch.full((n, case.ho, case.wo, c), 255, dtype=torch.int64, device=dev)
    for tap, ih, iw, valid in _taps(case, dev):
        am = torch.where(valid & (am == 255) & (xd[:, ih][:, :, iw] == m), tap, am)
    return m, am.to(torch.uint8)


def _win_slices(case, r, q):
    """Windows (oh, ow) whose tap (r, q) is inside the input, and the input slices they hit."""
    k = case
    oh0 = max(0, cdiv(k.pt - r, k.sh))
    oh1 = min(k.ho, (k.h - 1 + k.pt - r) // k.sh + 1)
    ow0 = max(0, cdiv(k.pl - q, k.sw))
    ow1 = min(k.wo, (k.w - 1 + k.pl - q) // k.sw + 1)
    if oh1 <= oh0 or ow1 <= ow0:
        return None
    ih0, iw0 = oh0 * k.sh - k.pt + r, ow0 * k.sw - k.pl + q
    return (slice(oh0, oh1), slice(ow0, ow1),
            slice(ih0, ih0 + (oh1 - oh0 - 1) * k.sh + 1, k.sh), slice(iw0, iw0 + (ow1 - ow0 - 1) * k.sw + 1, k.sw))


def pool_bwd_ref(case, am, dy, dtype):
    """(dx fp64, bound, k = contributing windows per input element)."""
    n, c, dev = case.n, case.c, dy.device
    z = lambda: torch.zeros((n, case.h, case.w, c), dtype=F64, device=dev)
    s, a, k = z(), z(), z()
    dyd, aml = dy.double(), am.long()
    for r in range(case.kh):
        for q in range(case.kw):
            sl = _win_slices(case, r, q)
            if sl is None:
                continue
            so, sw_, si, sj = sl
            hit = (aml[:, so, sw_] == r * case.kw + q).double()
            t = dyd[:, so, sw_] * hit
            s[:, si, sj] += t
            a[:, si, sj] += t.abs()
            k[:, si, sj] += hit
    bnd = torch.where(k > 1, (k - 1) * U * a + store_u(dtype) * s.abs(), torch.zeros_like(s))
    return s, bnd, k


def act_mask(xact, act):
    xd = xact.double()
    if act == "relu":
        return (xd > 0).double()
    if act == "relu6":
        return ((xd > 0) & (xd < 6)).double()
    return torch.where(xd > 0, 1.0, f32(LEAKY)).double()


def pool_suite(case, dtype, impl, dev="cpu", emulate=False):
    """(rows, pairs): rows (label, output, reference, bound); pairs of outputs that must agree bit for bit."""
    if emulate:
        case = pool_small(case)
    rows, pairs = [], []
    for data in case.datas:
        inp = {k: v.to(dev) for k, v in pool_inputs(case, dtype, data).items()}
        x, dy, xact = inp["x"], inp["dy"], inp.get("xact")
        if case.ho > 0 and case.wo > 0:
            yr, amr = pool_fwd_ref(case, x)
            zero = torch.zeros_like(yr)
            fin = lambda t: torch.nan_to_num(t.double(), nan=1e30, posinf=2e30, neginf=-1e30)  # -inf compares equal
            for off in sorted({o for _, _, o in case.routes}):
                y, am = impl.pool_fwd(case, x, True, off)
                rows += [(f"pool.y[{data},off{off}]", fin(y), fin(yr), zero),
                         (f"pool.argmax[{data},off{off}]", am, amr.double(), zero)]
                pairs.append((f"pool.y[{data},off{off}] is bitwise the maximum", y, yr.to(dtype)))
            y, _ = impl.pool_fwd(case, x, False, 0)
            rows.append((f"pool.y[{data},no argmax]", fin(y), fin(yr), zero))
        else:
            amr = torch.zeros((case.n, 0, 0, case.c), dtype=torch.uint8, device=dev)
        ref, bnd, k = pool_bwd_ref(case, amr, dy, dtype)
        first = None
        for route, with_am, off in case.routes:
            dx = impl.pool_bwd(case, dtype, None if with_am else x, amr if with_am else None, dy, off)
            tag = f"{data},{route},{'argmax' if with_am else 'recompute'}"
            rows.append((f"pool.dx[{tag}]", dx, ref, bnd))
            pairs.append((f"pool.dx[{tag}] has +0 where no window contributes", dx[k == 0], torch.zeros_like(dx[k == 0])))
            if first is not None:
                pairs.append((f"pool.dx[{tag}] = {first[0]}", dx, first[1]))
            else:
                first = (tag, dx)
        for act in case.acts:
            mk = act_mask(xact, act)
            slope = (mk != 1) & (mk != 0)
            ra = ref * mk
            ba = bnd * mk.abs() + torch.where(slope, U * ra.abs() + torch.where(k > 1, 0.0, store_u(dtype)) * ra.abs(), 0.0)
            route, _, off = case.routes[0]
            dxa = impl.pool_bwd_act(case, amr, dy, xact, act, LEAKY, off)
            rows.append((f"pool.dx_act[{data},{route},{act}]", dxa, ra, ba))
            if act != "leaky":  # fused = plain times the 0 / 1 mask, bit for bit (a zero may differ in sign)
                plain = (first[1].float() * mk.float()).to(dtype)
                pairs.append((f"pool.dx_act[{data},{route},{act}] = dx * mask", dxa + 0.0, plain + 0.0))
    return rows, pairs


# ------------------------------------------------------------------------ FPN
@dataclasses.dataclass(frozen=True)
class FpnCase:
    name: str
    n: int
    sizes: tuple  # (h5, w5, h4, w4, h3, w3); h3 = w3 = 0: the upsample form, null P3 pointers
    datas: tuple = ("randn", "ints")
    cs: tuple = ()  # channel counts; empty: FPN_CS of the dtype
    dtypes: tuple = (F32, BF16)
    loops: tuple = (False, False)  # (forward, backward) grid-stride loop
    run: tuple = ("fwd", "bwd")
    small: tuple = ()
    note: str = ""


FPN_CS = {BF16: (8, 24), F32: (4, 24)}
FPN_VN = {BF16: 8, F32: 4}
FPN_CASES = [
    FpnCase("square_7_14_28", 2, (7, 7, 14, 14, 28, 28), datas=("randn", "ints", "cancel"), note="exact 2x, four children each"),
    FpnCase("ragged_4x5", 2, (4, 5, 7, 9, 13, 18), note="non-square, ragged ratios: 1 to 3 children"),
    FpnCase("one_pixel", 1, (1, 1, 1, 1, 2, 2), note="one source pixel per level"),
    FpnCase("fp32_index", 1, (7, 14, 14, 23, 28, 46), note="14 -> 23: fp32 and the exact rational map differ at d = 11"),
    FpnCase("upsample_up", 2, (5, 7, 9, 16, 0, 0), note="upsample form, null P3 pointers"),
    FpnCase("upsample_down", 1, (7, 9, 4, 4, 0, 0), note="downsampling: sources without children"),
    FpnCase("loop_fwd", 1, (230, 230, 460, 460, 920, 920), datas=("ints",), cs=("vn",), loops=(True, False),
            run=("fwd",), small=(23, 23, 46, 46, 92, 92), note="forward grid-stride loop"),
    FpnCase("loop_bwd", 1, (250, 250, 1000, 1000, 0, 0), datas=("randn",), cs=("vn",), loops=(False, True),
            run=("bwd",), small=(25, 25, 100, 100, 0, 0), note="backward grid-stride loop, upsample form"),
]
FPN_BY_NAME = {c.name: c for c in FPN_CASES}


def fpn_cs(case, dtype):
    return tuple(FPN_VN[dtype] if c == "vn" else c for c in case.cs) or FPN_CS[dtype]


def fpn_small(case):
    return dataclasses.replace(case, sizes=case.small, small=(), loops=(False, False)) if case.small else case


def fpn_inputs(case, dtype, c, data):
    g = torch.Generator().manual_seed(_seed(f"fpn_{case.name}_{data}_{c}"))
    n = case.n
    h5, w5, h4, w4, h3, w3 = case.sizes
    shapes = {"l5": (n, h5, w5, c), "l4": (n, h4, w4, c), "l3": (n, h3, w3, c), "dp4": (n, h4, w4, c),
              "dp3": (n, h3, w3, c), "dl5_0": (n, h5, w5, c)}
    if data == "ints":  # small integers: every sum exact in both dtypes
        t = {k: torch.randint(-8, 9, s, generator=g).float() for k, s in shapes.items()}
    else:
        t = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    if data == "cancel":
        # forward: l3 = -(the rounded P4m) (1 + small): P3m is a cancellation, so the intermediate
        # rounding of P4m (half an ulp of P4m) shows against a bound relative to |P3m|
        iy, ix = up_idx(h4, h5), up_idx(w4, w5)
        p4 = (t["l4"].to(dtype).double() + t["l5"].to(dtype).double()[:, iy][:, :, ix]).to(dtype)
        jy, jx = up_idx(h3, h4), up_idx(w3, w4)
        t["l3"] = -(p4.float()[:, jy][:, :, jx]) * (1 + 0.01 * torch.rand(shapes["l3"], generator=g))
        # backward: the children of a P5 pixel alternate in sign, d_lat5 is a cancellation of rounded totals
        sgn = 1 - 2 * ((torch.arange(h4)[:, None] + torch.arange(w4)[None, :]) % 2).float()
        t["dp4"] = sgn[None, :, :, None] * (1 + 0.3 * torch.rand(shapes["dp4"], generator=g))
        t["dp3"] = 0.1 * t["dp3"]
    return {k: v.to(dtype) for k, v in t.items()}


def up_idx(out, inp, dev="cpu"):
    if out == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    return torch.from_numpy(nn_src_f32(out, inp)).to(dev)


def _down(t, iy, ix, h, w):
    n, _, w_in, c = t.shape
    rows = torch.zeros((n, h, w_in, c), dtype=F64, device=t.device).index_add_(1, iy, t)
    return torch.zeros((n, h, w, c), dtype=F64, device=t.device).index_add_(2, ix, rows)


def fpn_fwd_rows(case, dtype, l5, l4, l3, p4m, p3m, tag):
    h5, w5, h4, w4, h3, w3 = case.sizes
    dev = l5.device
    rel = store_u(dtype) + (U if dtype == BF16 else 0.0)
    r4 = l4.double() + l5.double()[:, up_idx(h4, h5, dev)][:, :, up_idx(w4, w5, dev)]
    rows = [(f"fpn.p4m[{tag}]", p4m, r4, rel * r4.abs())]
    if h3 > 0:
        r3 = l3.double() + p4m.double()[:, up_idx(h3, h4, dev)][:, :, up_idx(w3, w4, dev)]
        rows.append((f"fpn.p3m[{tag}]", p3m, r3, rel * r3.abs()))
    return rows


def fpn_bwd_rows(case, dtype, dp4, dp3, dl5_0, acc, dl4, dl5, tag):
    h5, w5, h4, w4, h3, w3 = case.sizes
    dev = dp4.device
    d4 = dp4.double()
    if h3 > 0:
        jy, jx = up_idx(h3, h4, dev), up_idx(w3, w4, dev)
        d3 = dp3.double()
        r4, a4 = d4 + _down(d3, jy, jx, h4, w4), d4.abs() + _down(d3.abs(), jy, jx, h4, w4)
        k4 = _down(torch.ones_like(d3), jy, jx, h4, w4)
    else:
        r4, a4, k4 = d4, d4.abs(), torch.zeros_like(d4)
    b4 = torch.where(k4 > 0, k4 * U * a4 + store_u(dtype) * r4.abs(), torch.zeros_like(r4))
    iy, ix = up_idx(h4, h5, dev), up_idx(w4, w5, dev)
    s4 = dl4.double()  # the stored, rounded totals
    old = dl5_0.double() if acc else torch.zeros((), dtype=F64, device=dev)
    r5 = _down(s4, iy, ix, h5, w5) + old
    a5 = _down(s4.abs(), iy, ix, h5, w5) + old.abs()
    k5 = _down(torch.ones_like(s4), iy, ix, h5, w5)
    b5 = torch.where(k5 - 1 + acc >= 1, (k5 + acc) * U * a5 + store_u(dtype) * r5.abs(), torch.zeros_like(r5))
    return [(f"fpn.d_lat4[{tag}]", dl4, r4, b4), (f"fpn.d_lat5[{tag}]", dl5, r5, b5)]


def fpn_suite(case, dtype, impl, dev="cpu", emulate=False):
    if emulate:
        case = fpn_small(case)
    rows, pairs = [], []
    up = case.sizes[4] == 0
    for c in fpn_cs(case, dtype):
        for data in case.datas:
            if data == "cancel" and dtype != BF16:
                continue
            inp = {k: v.to(dev) for k, v in fpn_inputs(case, dtype, c, data).items()}
            tag = f"c{c},{data}"
            if "fwd" in case.run:
                p4m, p3m = impl.fpn_fwd(case, inp["l5"], inp["l4"], None if up else inp["l3"])
                fr = fpn_fwd_rows(case, dtype, inp["l5"], inp["l4"], inp["l3"], p4m, p3m, tag)
                rows += fr
                if data == "ints":  # every sum exact: the in-register P4m of the P3m path = the stored P4m
                    pairs += [(f"{r[0]} is exact", r[1], r[2].to(dtype)) for r in fr]
            if "bwd" in case.run:
                for acc in (0, 1):
                    dl4, dl5 = impl.fpn_bwd(case, inp["dp4"], None if up else inp["dp3"], inp["dl5_0"], acc)
                    br = fpn_bwd_rows(case, dtype, inp["dp4"], inp["dp3"], inp["dl5_0"], acc, dl4, dl5, f"{tag},acc{acc}")
                    rows += br
                    if data == "ints":
                        pairs += [(f"{r[0]} is exact", r[1], r[2].to(dtype)) for r in br]
    return rows, pairs


def fpn_adjoint(case, impl, dev="cpu", c=4):
    """<fwd(l5, 0, 0), g> and <l5, bwd(g)> on integer-valued fp32 data: equal exactly."""
    inp = {k: v.to(dev) for k, v in fpn_inputs(case, F32, c, "ints").items()}
    up = case.sizes[4] == 0
    p4m, p3m = impl.fpn_fwd(case, inp["l5"], torch.zeros_like(inp["l4"]), None if up else torch.zeros_like(inp["l3"]))
    _, dl5 = impl.fpn_bwd(case, inp["dp4"], None if up else inp["dp3"], inp["dl5_0"], 0)
    lhs = (p4m.double() * inp["dp4"].double()).sum()
    if not up:
        lhs = lhs + (p3m.double() * inp["dp3"].double()).sum()
    return float(lhs), float((inp["l5"].double() * dl5.double()).sum())


# ------------------------------------------------------------ spatial softmax
@dataclasses.dataclass(frozen=True)
class SsmCase:
    name: str
    n: int
    hw: int
    c: int
    geom: tuple  # (chunks, chunk, ssm_bwd1 row loop)
    data: str = "normal"
    gap: float = 0.0
    small: tuple = ()
    note: str = ""


SSM_CASES = [
    SsmCase("hw784_c32", 2, 784, 32, (3, 262, False), note="3 chunks of 262, the last one short (260)"),
    SsmCase("hw1", 3, 1, 256, (1, 1, False), note="hw = 1: a = 1 and d_score = 0 exactly"),
    SsmCase("hw15_c5", 2, 15, 5, (1, 15, False), note="hw < 256, c < 64: idle threads and lanes"),
    SsmCase("hw300_c3", 2, 300, 3, (1, 300, False), note="a second, ragged thread stride"),
    SsmCase("chunks_clamped", 1, 2, 16384, (2, 1, False), note="hw c / 8192 = 4 chunks clamped to hw = 2"),
    SsmCase("peaked_gap4", 2, 196, 256, (6, 33, False), data="peaked", gap=4.0, note="scores x 100, nearly one-hot"),
    SsmCase("peaked_gap9", 2, 196, 256, (6, 33, False), data="peaked", gap=9.0),
    SsmCase("peaked_gap14", 2, 196, 256, (6, 33, False), data="peaked", gap=14.0),
    SsmCase("all_equal", 2, 49, 64, (1, 49, False), data="equal", note="a = 1 / 49"),
    SsmCase("neg_inf", 2, 49, 64, (1, 49, False), data="neg_inf", note="-inf at a few positions: a = 0 there"),
    SsmCase("pm80", 2, 49, 64, (1, 49, False), data="pm80", note="scores of magnitude 80 to 92: exp overflows unless the max is subtracted"),
    SsmCase("bwd_row_loop", 3, 11000, 4, (5, 2200, True), small=(3, 700, 4), note="33000 positions > 4 x 8192 waves"),
]
SSM_BY_NAME = {c.name: c for c in SSM_CASES}
SSM_DTYPES = (F32, BF16)


def ssm_small(case):
    if not case.small:
        return case
    n, hw, c = case.small
    return dataclasses.replace(case, n=n, hw=hw, c=c, small=(), geom=(*ssm_chunks(hw, c), False))


def ssm_inputs(case, dtype):
    g = torch.Generator().manual_seed(_seed("ssm_" + case.name))
    n, hw, c = case.n, case.hw, case.c
    score = 3 * torch.randn(n, hw, generator=g)
    hs, dctx = torch.randn(n, hw, c, generator=g), torch.randn(n, hw, c, generator=g)
    if case.data == "peaked":  # the existing peaked test's magnitudes
        score = (torch.randn(n, hw, generator=g) * 100.0).to(dtype).float()
        for b in range(n):
            score[b, (37 * (b + 1)) % hw] = score[b].max() + case.gap
        hs, dctx = hs * 400.0, dctx * 1e-4
    elif case.data == "equal":
        score = torch.full((n, hw), 1.25)
    elif case.data == "neg_inf":
        score[:, ::7] = -np.inf
    elif case.data == "pm80":
        u = torch.rand(n, hw, generator=g)
        mag = 80 + 4 * torch.randn(n, hw, generator=g).abs()  # the largest beyond 88.8: expf alone overflows
        score = torch.where(u < 0.5, mag, -mag)
        score[:, 1], score[:, 2] = 90.0, -92.0
    return {"score": score.to(dtype), "hs": hs.to(dtype), "dctx": dctx.to(dtype)}


def ssm_a_ref(score, hw):
    xd = score.double()
    m = xd.max(1, keepdim=True).values
    z = xd - m
    e = z.exp()
    s = e.sum(1, keepdim=True)
    zz = torch.where(e > 0, z.abs(), torch.zeros_like(z))  # exp(-inf) is exactly 0
    arg = U * zz + EXPU
    eps_s = (e * arg).sum(1, keepdim=True) / s + (cdiv(hw, 256) + 9) * U
    a = e / s
    return a, a * (arg + eps_s + U) + TINY


def ssm_suite(case, dtype, impl, dev="cpu", emulate=False):
    if emulate:
        case = ssm_small(case)
    inp = {k: v.to(dev) for k, v in ssm_inputs(case, dtype).items()}
    score, hs, dctx = inp["score"], inp["hs"], inp["dctx"]
    hw, c = case.hw, case.c
    rel = U + store_u(dtype)
    ctx, a = impl.ssm_fwd(case, score, hs)
    ar, ab = ssm_a_ref(score, hw)
    cr = a.double()[:, :, None] * hs.double()  # from the stored a
    rows = [("ssm.a", a, ar, ab), ("ssm.ctx", ctx, cr, rel * cr.abs() + TINY)]
    a_in = ar.float()  # the backward's input: the reference softmax as stored in fp32
    d_score, d_hs, da = impl.ssm_bwd(case, a_in, hs, dctx)
    ad = a_in.double()
    hr = ad[:, :, None] * dctx.double()
    t = dctx.double() * hs.double()
    dr = t.sum(2)
    rows += [("ssm.d_hs", d_hs, hr, rel * hr.abs() + TINY), ("ssm.da", da, dr, (cdiv(c, 64) + 6) * D53 * t.abs().sum(2))]
    dad = da.double()  # from the stored da
    w = ad * dad
    sr = ad * (dad - w.sum(1, keepdim=True))
    sb = rel * sr.abs() + ad * (cdiv(hw, 256) + 10) * D53 * w.abs().sum(1, keepdim=True) + TINY
    rows.append(("ssm.d_score", d_score, sr, sb))
    return rows, []

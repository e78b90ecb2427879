"""Case table of the row kernels of csrc/elementwise.hip that every
Transformer sublayer of the captioner runs: LayerNorm (plain, with the fused
dropout backward, the one-key broadcast form and the encoder's five views),
embedding + positional encoding, the masked cross-entropy, activation backward
with its bias gradient, dropout, cast and add.

Helper module, not collected, importable without a GPU:
tests/test_row_kernel_bars.py (no GPU) proves on an fp32 / bf16 emulation of
each kernel and on planted mutations that the bounds below can fail, and
checks the grid restatements against the geometry every case records;
tests/test_gpu_row_kernels.py runs every case through the C entry points.

Reference: float64, from the exact stored inputs of each entry point widened
to double, so the error of one stage never reaches the next. The backward
takes stored fp32 mean / rstd (the reference's statistics rounded to fp32,
what a correct forward stores to within its bound, the same on the emulation
and on the device); dz is judged from the dx the entry point
stored, db from the dz it stored, bcast_fwd's y from the x_out it stored. The
residual sum is rounded to the storage dtype as the kernel rounds it; the
inputs are chosen so that the fp32 sum is exact (asserted by `ln_inputs`), so
the two roundings cannot differ. Values that a kernel first rounds to the
storage dtype with a single IEEE operation (dy under the output dropout, the
synthesised x of the broadcast form when x_out is null) are restated with the
same single fp32 operation and are then inputs. Activation masks come from
the stored y.

Dropout mask: `hash_u32` / `uniform01` / `drop_key` restate csrc/common.h and
drop_key_of in numpy uint64 with wrap-around; an element is kept iff
(hash & 0xFFFFFF) * 2^-24 >= float32(p), element index row * d + col, key
seed + seed_dev * 0x9E3779B97F4A7C15. The mask is exact, so a dropped element
is exactly zero (bound zero) and a kept one is to_T(to_T(v) * sc), sc =
1 / (1 - p) formed in fp32: at most two roundings.

Bounds: per element, first order, counted from the arithmetic the kernel
performs. U = 2^-24 is one fp32 rounding relative to the magnitude it acts on,
RSQ = 2^-23 the allowance for rsqrtf and the store costs 2^-8 |ref| (bf16) or
2^-24 |ref| (fp32): the constants of tests/bn_dw_cases.py, justified in its
docstring. EXPU = LOGU = 2^-23: HIP's math API reference lists expf and logf
(as rsqrtf) with a maximum error of 1 ulp, and one ulp is at most 2^-23 of
the value. A sum whose longest chain of additions has `depth` links is within
depth U sum |terms| of the exact sum. L = `ln_lane_depth(d, vec)`, the columns
one lane adds in sequence (restated from ln_col); 6 is the wave butterfly.

  ln mean          bm = (L + 6 + 1) U sum |v| / d: lane adds, butterfly, the
                   division (v = x, or the rounded x + res)
  ln rstd          rstd (bvar / (2 (var + eps)) + U + RSQ), bvar =
                   (L + 6 + 4) U var + bm^2: t = v - mu (1, squared: 2), the
                   fused accumulation L + 6, the division 1; a mean off by
                   delta adds exactly delta^2 to the variance; var + eps 1
  ln y             |gamma| (rstd bm + |xhat| (2 U + brstd / rstd))
                   + U (|xhat gamma| + |beta|)            the fused multiply-add
                   + U (|xhat gamma| + |beta| + |pe|)     + pe
                   + store. The first term, |rstd gamma| depth U sum |x| / d,
                   governs the large-mean case; the variance error enters as
                   |xhat gamma| / 2 times its relative error (inside brstd).
  dropout of an    sc (bound of the value) + (U + store) |ref|; zero where
  output           dropped
  ln dx            rstd (4 U T + 2 U |xhat| |s2| + (L + 8) U A1
                   + (L + 11) U |xhat| A2) + store, T = |g| + |s1| + |xhat| |s2|,
                   A1 = sum |g| / d, A2 = sum |g xhat| / d. g = dy gamma 1; s1:
                   g 1, adds L + 6, division 1; s2: g 1, xhat 2, product 1,
                   adds L + 6, division 1; g - s1 1, the fused step 1, times
                   rstd 1 (3 on T); xhat inside the fused step 2. Never |dx|:
                   dx is a cancellation.
  ln dz            (U + store) |ref|, ref = stored dx under the mask times sc
  ln dgamma,       (depth [+ 3]) U sum |terms| + U |old + sum|, depth = rows per
  dbeta            wave ceil(rows / (4 grid)) + 3 (the four waves) +
                   ceil(grid / KL) + 2 (a lane's chunks, its four accumulators)
                   + KL - 1 (the lanes in order), KL = 1024 / CB, CB from
                   `colsum_cb(2 d)`; dgamma's terms dy xhat carry 3 more (xhat 2,
                   product 1). The views add one such sum per view, in view
                   order: U |running sum| each.
  bcast x_out      sc U (|c| + |cbias|) + (U + store) |ref|: one add, one scale,
                   the store
  embed fwd        U (|emb| + |pe|) + store (then the dropout rule)
  embed d_emb      (P + C + 1) U sum |dy| + U |old + sum| over the id's
                   positions, P its most positions in one 64-chunk, C its
                   chunks; rows of absent ids: bound zero
  embed sumsq      (ceil(d / 64) + 1 + 6 + ceil(rows / 256) + 6 + 2) U sum dy^2
                   + U |old + sum|: product, lane adds, butterfly; the ordered
                   sum's thread adds, butterfly and three block adds
  xent             e_j = exp(x_j - m), s = sum e_j. eps_s = sum e_j (U |x_j - m|
                   + EXPU) / s + (ceil(v / 256) + 6 + 3) U: the subtraction's
                   rounding moves the exponent, expf, thread adds, butterfly,
                   the four waves.
    row loss       eps_s + LOGU |log s| + U |m + log s| + U |row loss|
    loss           mean of the row bounds + (ceil(rows / 256) + 6 + 2 + 2) U
                   sum |row loss| / rows (ordered sum; 1 / rows and the product)
    dlogits        |coef| (p_j (U |x_j - m| + EXPU + eps_s + U) + [j = label]
                   U |p_j - 1|) + 2 U |ref| + store + TINY: the division, the
                   cancellation p - 1 on its terms, coef = gscale / rows 1, the
                   product 1; TINY = 2^-126 (absolute) covers underflow and the
                   subnormal stores. Rows with label 0: exactly zero.
  act_bwd dz       (n U + store) |ref|, n = [dropout] + [leaky]; zero (exact) for
                   n = 0: the 0/1 masks of none / relu / relu6 pass dy through
  act_bwd db,      depth U sum |dz| + U |old + sum| from the stored dz, depth =
  bias_grad        ceil(rpc / RL) + log2 RL + (gy > 1: ceil(gy / KL) + 2 + KL - 1)
                   + 1 from the restated `act_bwd_grid`
  dropout, cast,   exact: equality with the host restatement (bound zero)
  add
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U, RSQ, EXPU, LOGU, TINY = 2.0 ** -24, 2.0 ** -23, 2.0 ** -23, 2.0 ** -23, 2.0 ** -126
EPS = float(torch.tensor(1e-6, dtype=F32))  # the float the entry points receive
SENTINEL = -12352.0  # exact in bf16; no output of these cases comes near it
GUARD = 64  # sentinel elements after every output
LN_MAXE = 16
FWD_CAP, BWD_CAP = 8192, 1024  # blocks of four waves, a row per wave
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def cdiv(a, b):
    return -(-a // b)


def store_u(dtype):
    return 2.0 ** -8 if dtype == BF16 else U


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def short(dtype):
    return str(dtype).replace("torch.", "")


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) * 7919


# ------------------------------------------------------------- dropout mask
def hash_u32(key, idx):
    """csrc/common.h hash_u32 on a numpy uint64 index array."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = u((key * GOLDEN + 0x632BE59BD9B4E019) & M64) + idx.astype(u) * u(0xD1B54A32D192ED03)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(8)) & u(0xFFFFFFFF)


def uniform01(key, idx):
    return (hash_u32(key, idx) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)


def drop_key(seed, seed_dev=None):
    return (seed + (0 if seed_dev is None else (seed_dev & M64) * GOLDEN)) & M64


def keep_mask(key, n, p, first=0, shift=0, strict=False):
    """[n] bool on the CPU: elements first .. first + n of the tensor kept."""
    u = uniform01(key, np.arange(first + shift, first + shift + n, dtype=np.uint64))
    return torch.from_numpy(u > np.float32(p) if strict else u >= np.float32(p))


def drop_scale(p, inverse_of_p=False):
    """1 / (1 - p) formed in fp32, as a Python float."""
    one, pp = np.float32(1.0), np.float32(p)
    return float(one / pp) if inverse_of_p else float(one / (one - pp))


def drop_round(v, keep, p, dtype):
    """The kernels' dropout of a stored value: to_T(keep ? v * sc : 0), one fp32 product."""
    sc = torch.tensor(drop_scale(p), dtype=F32, device=v.device)
    return torch.where(keep, v.float() * sc, torch.zeros((), device=v.device)).to(dtype)


def drop_ref(ref, bnd, keep, p, dtype):
    """(ref, bound) of the dropout of a value with the given (ref, bound)."""
    sc = drop_scale(p)
    out = torch.where(keep, ref * sc, torch.zeros((), dtype=F64, device=ref.device))
    b = torch.where(keep, sc * bnd + (U + store_u(dtype)) * out.abs(), torch.zeros((), dtype=F64, device=ref.device))
    return out, b


# ------------------------------------------------------------------ geometry
def grid_for(work, block, cap=4096):
    return max(1, min(cap, cdiv(work, block)))


def pow2_floor(v):
    r = 1
    while r * 2 <= v:
        r *= 2
    return r


def colsum_cb(c):
    return 64 if c >= 64 * 64 else 32 if c >= 32 * 32 else 16


def ln_col(vec, lane, k):
    return (lane + 64 * (k >> 3)) * 8 + (k & 7) if vec else lane + 64 * k


def ln_lane_depth(d, vec):
    return max(sum(1 for k in range(LN_MAXE) if ln_col(vec, lane, k) < d) for lane in range(64))


def ln_is_vec(d, dtype, offset=0):
    return dtype == BF16 and d % 8 == 0 and offset % 8 == 0


def ln_geom(rows, d):
    """(fwd grid, rows per wave fwd, bwd grid, rows per wave bwd, CB, chunks in the four-wide loop)."""
    gf, gb = grid_for(rows, 4, FWD_CAP), grid_for(rows, 4, BWD_CAP)
    cb = colsum_cb(2 * d)
    return gf, cdiv(rows, 4 * gf), gb, cdiv(rows, 4 * gb), cb, gb > 3 * (1024 // cb)


def colsum_depth(chunks, c):
    kl = 1024 // colsum_cb(c)
    return cdiv(chunks, kl) + 2 + kl - 1


def ln_grad_depth(rows, d):
    gb = grid_for(rows, 4, BWD_CAP)
    return cdiv(rows, 4 * gb) + 3 + colsum_depth(gb, 2 * d)


def act_bwd_grid(rows, c, dtype, aligned=True, colsum=True):
    """(vec, gx, gy, rpc, GT, RL) of csrc/elementwise.hip's act_bwd_grid."""
    vn = 8 if dtype == BF16 else 4
    vec = c % vn == 0 and aligned
    groups = c // vn if vec else c
    if colsum:
        gt = max(1, min(256, groups // 64))
        rl = pow2_floor(256 // gt)
        if cdiv(rows, rl) <= 8:
            return vec, cdiv(groups, gt), 1, rows, gt, rl
    GT = min(groups, 256)
    RL = pow2_floor(256 // GT)
    gx = cdiv(groups, GT)
    chunks = max(1, min(max(1, 1024 // gx), cdiv(rows, 4 * RL)))
    rpc = cdiv(rows, chunks)
    return vec, gx, cdiv(rows, rpc), rpc, GT, RL


def act_db_depth(rows, c, dtype, aligned=True):
    vec, gx, gy, rpc, GT, RL = act_bwd_grid(rows, c, dtype, aligned)
    return cdiv(rpc, RL) + int(math.log2(RL)) + (colsum_depth(gy, c) if gy > 1 else 0) + 1


# ---------------------------------------------------------------- LayerNorm
@dataclasses.dataclass(frozen=True)
class LnCase:
    name: str
    rows: int
    d: int
    geom: tuple  # (bf16 vectorised, *ln_geom(rows, d)) the case is meant to hit
    dtypes: tuple = (F32, BF16)
    data: str = "normal"
    offset: int = 0  # elements every activation pointer is shifted by (bf16: 2 bytes each)
    fwd_only: bool = False
    pe_rows: int = 5
    drop: tuple = ()  # layernorm_bwd_drop at these p
    note: str = ""


LN_CASES = [
    LnCase("one_lane", 1, 8, (True, 1, 1, 1, 1, 16, False), note="(1, 8): one live lane, variance 0 per lane group"),
    LnCase("scalar_300", 7, 300, (False, 2, 1, 2, 1, 16, False), drop=(0.1, 0.5),
           note="scalar bf16 route, d % 8 = 4"),
    LnCase("vec_1000", 37, 1000, (True, 10, 1, 10, 1, 32, False), drop=(0.1, 0.5),
           note="vectorised, second lane group partly live (61 of 64 lanes)"),
    LnCase("maxe_full", 5, 1024, (True, 2, 1, 2, 1, 32, False), note="LN_MAXE full: d = 1024"),
    LnCase("vec_520", 33, 520, (True, 9, 1, 9, 1, 32, False), note="vectorised, one live lane in the second group"),
    LnCase("misaligned", 9, 512, (False, 3, 1, 3, 1, 32, False), dtypes=(BF16,), offset=1,
           note="every bf16 tensor offset by one element: the misaligned scalar route"),
    LnCase("bwd_row_loop", 4099, 8, (True, 1025, 1, 1024, 2, 16, True), drop=(0.1, 0.5), pe_rows=7,
           note="backward row loop (r += nw), 1024 partial rows, four-wide act_colsum loop"),
    LnCase("bwd_row_loop_512", 4101, 512, (True, 1026, 1, 1024, 2, 32, True), dtypes=(BF16,), pe_rows=7,
           note="backward row loop with CB = 32, four-wide act_colsum loop"),
    LnCase("fwd_row_loop", 32771, 8, (True, 8192, 2, 1024, 9, 16, True), fwd_only=True, pe_rows=7,
           note="forward row loop above 32768 rows"),
    LnCase("large_mean_f32", 37, 512, (True, 10, 1, 10, 1, 32, False), dtypes=(F32,), data="large_mean",
           note="x = 1000 + 0.01 N(0, 1): the unshifted row sum governs"),
    LnCase("large_mean_bf16", 37, 512, (True, 10, 1, 10, 1, 32, False), dtypes=(BF16,), data="large_mean",
           note="x = 64 + N(0, 1), quantised"),
    LnCase("const_row", 37, 512, (True, 10, 1, 10, 1, 32, False), data="const",
           note="row 3 constant: variance exactly 0, rstd = eps^-1/2"),
    LnCase("outlier", 37, 512, (True, 10, 1, 10, 1, 32, False), data="outlier", note="row 5 holds one 1e4 outlier"),
]
LN_BY_NAME = {c.name: c for c in LN_CASES}
QUANT = 256.0  # bf16 activations lie on a 2^-8 grid: the fp32 residual sum is exact


def _q(t, dtype):
    return (torch.round(t * QUANT) / QUANT).to(dtype) if dtype == BF16 else t.to(dtype)


def ln_inputs(case, dtype, rows=None, d=None, tag=""):
    rows, d = rows if rows is not None else case.rows, d or case.d
    g = torch.Generator().manual_seed(_seed("ln_" + case.name + tag))
    z = torch.randn(rows, d, generator=g)
    if case.data == "large_mean":
        x = 1000 + 0.01 * z if dtype == F32 else 64 + z
    else:
        x = 3 * z + 1
    if case.data == "const":
        x[3] = 1.5
    if case.data == "outlier":
        x[5, 77] = 1e4
    res = torch.randn(rows, d, generator=g)
    if case.data == "const":
        res[3] = -0.25
    inp = {"x": _q(x, dtype), "res": _q(res, dtype), "dy": torch.randn(rows, d, generator=g).to(dtype),
           "gamma": torch.rand(d, generator=g) + 0.5, "beta": torch.randn(d, generator=g),
           "pe": torch.randn(case.pe_rows, d, generator=g),
           "dgamma0": torch.randn(d, generator=g) * 3, "dbeta0": torch.randn(d, generator=g) * 3}
    assert_sum_exact(inp["x"], inp["res"], dtype)
    return inp


def assert_sum_exact(x, res, dtype):
    """bf16: the fp32 sum of the two stored values is exact, so rounding the
    fp64 sum to bf16 is the kernel's rounding. fp32: the fp64 sum rounds to
    the fp32 sum."""
    s64 = x.double() + res.double()
    if dtype == BF16:
        assert torch.equal((x.float() + res.float()).double(), s64), "the fp32 residual sum must be exact"
    else:
        assert torch.equal(x + res, s64.float()), "the fp64 residual sum must round to the fp32 sum"


def ln_v(x, res, dtype):
    """The row the kernel normalises, in fp64: x, or the rounded x + res."""
    return x.double() if res is None else (x.double() + res.double()).to(dtype).double()


def ln_fwd_ref(v, gamma, beta, pe, pe_rows, eps, dtype, vec):
    """{label: (ref, bound)} of y, mean, rstd from the row v (fp64)."""
    rows, d = v.shape
    L = ln_lane_depth(d, vec)
    mean = v.mean(1)
    var = ((v - mean[:, None]) ** 2).mean(1)
    rs = (var + eps).rsqrt()
    bm = (L + 7) * U * v.abs().sum(1) / d
    bvar = (L + 10) * U * var + bm * bm
    brs = rs * (bvar / (2 * (var + eps)) + U + RSQ)
    xh = (v - mean[:, None]) * rs[:, None]
    t = xh * gamma.double()
    mag = t.abs() + beta.double().abs()
    y = t + beta.double()
    by = gamma.double().abs() * ((rs * bm)[:, None] + xh.abs() * (2 * U + brs / rs)[:, None]) + U * mag
    if pe is not None:
        p = pe.double()[torch.arange(rows, device=v.device) % pe_rows]
        y = y + p
        by = by + U * (mag + p.abs())
    by = by + store_u(dtype) * y.abs()
    return {"y": (y, by), "mean": (mean, bm), "rstd": (rs, brs)}


def ln_dy_in(dy, keep, ip, dtype):
    """dy as the backward uses it: under the output dropout (ip > 0) rounded to T."""
    return dy if not ip else drop_round(dy, keep, ip, dtype)


def ln_bwd_ref(v, gamma, mean, rstd, dyf, dtype, vec):
    """dx (ref, bound) and the per-column sums (sg, sb, abs sg, abs sb) from
    the row v, the stored fp32 mean / rstd and the dy the kernel uses."""
    rows, d = v.shape
    L = ln_lane_depth(d, vec)
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (v - mu) * rs
    dyd = dyf.double()
    g = dyd * gamma.double()
    s1, s2 = g.sum(1, keepdim=True) / d, (g * xh).sum(1, keepdim=True) / d
    A1, A2 = g.abs().sum(1, keepdim=True) / d, (g * xh).abs().sum(1, keepdim=True) / d
    dx = rs * (g - s1 - xh * s2)
    T = g.abs() + s1.abs() + xh.abs() * s2.abs()
    b = rs.abs() * (4 * U * T + 2 * U * xh.abs() * s2.abs() + (L + 8) * U * A1 + (L + 11) * U * xh.abs() * A2) \
        + store_u(dtype) * dx.abs()
    t = dyd * xh
    return (dx, b), (t.sum(0), dyd.sum(0), t.abs().sum(0), dyd.abs().sum(0))


def grad_bound(depth, extra, s, a, old):
    """Bound of old + s for a sum s of terms with absolute sum a."""
    return (depth + extra) * U * a + U * (old.double() + s).abs()


def dz_ref(dx_stored, keep, p, dtype):
    sc = drop_scale(p)
    ref = torch.where(keep, dx_stored.double() * sc, torch.zeros((), dtype=F64, device=dx_stored.device))
    return ref, (U + store_u(dtype)) * ref.abs()


def _mask2d(key, rows, d, p, dev, **kw):
    return keep_mask(key, rows * d, p, **kw).view(rows, d).to(dev)


LN_SEED, LN_SEED_DEV = 0x1234567, 77


def ln_suite(case, dtype, impl, dev="cpu"):
    """(label, output, reference, bound) rows of fpnmt_layernorm_fwd / _bwd / _bwd_drop."""
    inp = {k: v.to(dev) for k, v in ln_inputs(case, dtype).items()}
    x, gamma, beta, dy = inp["x"], inp["gamma"], inp["beta"], inp["dy"]
    rows, d = x.shape
    vec = ln_is_vec(d, dtype, case.offset)
    out = []
    for res in (None, inp["res"]):
        rt = "res" if res is not None else "-"
        v = ln_v(x, res, dtype)
        for pe in (None, inp["pe"]):
            tag = f"[{rt},{'pe' if pe is not None else '-'}]"
            ref = ln_fwd_ref(v, gamma, beta, pe, case.pe_rows, EPS, dtype, vec)
            y, mean, rstd = impl.ln_fwd(case, x, res, gamma, beta, pe, case.pe_rows, EPS)
            out += [(f"ln.y{tag}", y, *ref["y"]), (f"ln.mean{tag}", mean, *ref["mean"]),
                    (f"ln.rstd{tag}", rstd, *ref["rstd"])]
        if case.fwd_only:
            continue
        smean, srstd = ref["mean"][0].float(), ref["rstd"][0].float()  # the stored statistics
        (dxr, dxb), (sg, sb, ag, ab) = ln_bwd_ref(v, gamma, smean, srstd, dy, dtype, vec)
        depth = ln_grad_depth(rows, d)
        rg, rb = inp["dgamma0"].double() + sg, inp["dbeta0"].double() + sb
        bg, bb = grad_bound(depth, 3, sg, ag, inp["dgamma0"]), grad_bound(depth, 0, sb, ab, inp["dbeta0"])
        dx, dg, db, _ = impl.ln_bwd(case, x, res, gamma, smean, srstd, dy, inp["dgamma0"], inp["dbeta0"], 0.0, 0, None)
        out += [(f"ln.dx[{rt}]", dx, dxr, dxb), (f"ln.dgamma[{rt}]", dg, rg, bg), (f"ln.dbeta[{rt}]", db, rb, bb)]
        if res is None:  # null gradient accumulators
            dx, _, _, _ = impl.ln_bwd(case, x, res, gamma, smean, srstd, dy, None, None, 0.0, 0, None)
            out.append(("ln.dx[-,null grads]", dx, dxr, dxb))
        for p in case.drop:
            for sd in (None, LN_SEED_DEV):
                keep = _mask2d(drop_key(LN_SEED, sd), rows, d, p, dev)
                dx, dg, db, dz = impl.ln_bwd(case, x, res, gamma, smean, srstd, dy, inp["dgamma0"], inp["dbeta0"], p,
                                             LN_SEED, sd)
                t = f"[{rt},p={p},{'dev' if sd else 'null'}]"
                out += [(f"lndrop.dx{t}", dx, dxr, dxb), (f"lndrop.dz{t}", dz, *dz_ref(dx, keep, p, dtype)),
                        (f"lndrop.dgamma{t}", dg, rg, bg), (f"lndrop.dbeta{t}", db, rb, bb)]
    return out


# ------------------------------------------------- the one-key broadcast form
@dataclasses.dataclass(frozen=True)
class BcastCase:
    name: str
    b: int
    t: int
    d: int
    dtypes: tuple = (F32, BF16)
    note: str = ""


BCAST_CASES = [
    BcastCase("b3_t5_512", 3, 5, 512, note="vectorised in bf16, rows = 15"),
    BcastCase("b2_t7_300", 2, 7, 300, note="scalar bf16 route"),
    BcastCase("b4_t1_8", 4, 1, 8, note="t = 1: every row its own image"),
]
BCAST_BY_NAME = {c.name: c for c in BCAST_CASES}
BCAST_P = (0.0, 0.1)


def bcast_inputs(case, dtype):
    base = LnCase(case.name, case.b * case.t, case.d, ())
    inp = ln_inputs(base, dtype, tag="bcast")
    g = torch.Generator().manual_seed(_seed("bc_" + case.name))
    inp["c"] = torch.randn(case.b, case.d, generator=g) * 2
    inp["cbias"] = torch.randn(case.d, generator=g)
    if dtype == BF16:  # the synthesised x on the 2^-8 grid where kept unscaled (p = 0): exact residual sums
        inp["c"], inp["cbias"] = torch.round(inp["c"] * QUANT) / QUANT, torch.round(inp["cbias"] * QUANT) / QUANT
    return inp


def bcast_synth(c, cbias, t, keep, p, dtype):
    """(x as the kernel synthesises it: one fp32 add, one fp32 scale, the
    rounding; its fp64 reference; the bound)."""
    rows = c.shape[0] * t
    cr = c.repeat_interleave(t, 0)
    a32 = cr if cbias is None else cr + cbias
    a64 = cr.double() if cbias is None else cr.double() + cbias.double()
    mag = cr.double().abs() + (0 if cbias is None else cbias.double().abs())
    if p > 0:
        sc = drop_scale(p)
        x = drop_round(a32, keep, p, dtype)
        ref = torch.where(keep, a64 * sc, torch.zeros((), dtype=F64, device=c.device))
        bnd = torch.where(keep, sc * U * mag + (U + store_u(dtype)) * ref.abs(), torch.zeros_like(ref))
    else:
        x, ref = a32.to(dtype), a64
        bnd = U * mag + store_u(dtype) * ref.abs()
    return x, ref, bnd


BC_SEED, BC_SEED_DEV = 0xABCDEF01, -5


def bcast_suite(case, dtype, impl, dev="cpu"):
    inp = {k: v.to(dev) for k, v in bcast_inputs(case, dtype).items()}
    rows, d, t = case.b * case.t, case.d, case.t
    res, gamma, beta, dy = inp["res"], inp["gamma"], inp["beta"], inp["dy"]
    vec = ln_is_vec(d, dtype)
    out = []
    for p in BCAST_P:
        for cbias in (None, inp["cbias"]):
            for want_x in (False, True):
                sd = BC_SEED_DEV if want_x else None
                keep = _mask2d(drop_key(BC_SEED, sd), rows, d, p, dev) if p > 0 else None
                tag = f"[p={p},{'cbias' if cbias is not None else '-'},{'x_out' if want_x else '-'}]"
                xs, xr, xb = bcast_synth(inp["c"], cbias, t, keep, p, dtype)
                assert_sum_exact(xs, res, dtype)
                y, mean, rstd, x_out = impl.bcast_fwd(case, inp["c"], cbias, p, BC_SEED, sd, res, gamma, beta, EPS,
                                                     want_x)
                if want_x:
                    out.append((f"bcast.x_out{tag}", x_out, xr, xb))
                    xs = x_out  # y is judged against the LayerNorm of the x the entry point stored
                v = ln_v(xs, res, dtype)
                ref = ln_fwd_ref(v, gamma, beta, None, 1, EPS, dtype, vec)
                out += [(f"bcast.y{tag}", y, *ref["y"]), (f"bcast.mean{tag}", mean, *ref["mean"]),
                        (f"bcast.rstd{tag}", rstd, *ref["rstd"])]
                smean, srstd = ref["mean"][0].float(), ref["rstd"][0].float()
                (dxr, dxb), (sg, sb, ag, ab) = ln_bwd_ref(v, gamma, smean, srstd, dy, dtype, vec)
                depth = ln_grad_depth(rows, d)
                dx, dg, db, dz = impl.bcast_bwd(case, inp["c"], cbias, p, BC_SEED, sd, res, gamma, smean, srstd, dy,
                                                inp["dgamma0"], inp["dbeta0"])
                out += [(f"bcast.dx{tag}", dx, dxr, dxb),
                        (f"bcast.dgamma{tag}", dg, inp["dgamma0"].double() + sg, grad_bound(depth, 3, sg, ag, inp["dgamma0"])),
                        (f"bcast.dbeta{tag}", db, inp["dbeta0"].double() + sb, grad_bound(depth, 0, sb, ab, inp["dbeta0"]))]
                if p > 0:
                    out.append((f"bcast.dz{tag}", dz, *dz_ref(dx, keep, p, dtype)))
    return out


# -------------------------------------------------------- the encoder's views
@dataclasses.dataclass(frozen=True)
class ViewsCase:
    name: str
    rows: tuple
    d: int
    dtype: torch.dtype
    misaligned: int = -1  # index of the view whose pointers are offset by one element
    geom: tuple = ()  # per view (fwd blocks, bwd blocks): a zero-row view has none
    note: str = ""


VIEW_ROWS = (4099, 37, 0, 1, 260)
_VG = ((1025, 1024), (10, 10), (0, 0), (1, 1), (65, 65))
VIEWS_CASES = [
    ViewsCase("views_512_bf16", VIEW_ROWS, 512, BF16, geom=_VG,
              note="vectorised; view 0 walks two rows per wave in the backward; the zero-row view is skipped"),
    ViewsCase("views_8_f32", VIEW_ROWS, 8, F32, geom=_VG, note="fp32, d = 8"),
    ViewsCase("views_512_bf16_misaligned", VIEW_ROWS, 512, BF16, misaligned=1, geom=_VG,
              note="the second view misaligned: the whole launch takes the scalar route"),
]
VIEWS_BY_NAME = {c.name: c for c in VIEWS_CASES}
VIEWS_P = (0.0, 0.1)
VIEW_SEEDS = (11, 0xFFFFFFFFFFFFFFF1, 5, 0x9E3779B9, 1 << 40)
VIEW_PE_ROWS = (49, 37, 3, 1, 13)
VIEWS_SEED_DEV = 123456789


def views_geom(rows):
    return tuple((grid_for(r, 4, FWD_CAP), grid_for(r, 4, BWD_CAP)) if r > 0 else (0, 0) for r in rows)


def views_inputs(case):
    g = torch.Generator().manual_seed(_seed("views_" + case.name))
    d = case.d
    inp = {"gamma": torch.rand(d, generator=g) + 0.5, "beta": torch.randn(d, generator=g),
           "pe": torch.randn(max(VIEW_PE_ROWS), d, generator=g),
           "dgamma0": torch.randn(d, generator=g) * 3, "dbeta0": torch.randn(d, generator=g) * 3}
    inp["x"] = [_q(3 * torch.randn(r, d, generator=g) + 1, case.dtype) for r in case.rows]
    inp["dy"] = [torch.randn(r, d, generator=g).to(case.dtype) for r in case.rows]
    return inp


def views_suite(case, impl, dev="cpu"):
    inp = views_inputs(case)
    mv = lambda t: [e.to(dev) for e in t] if isinstance(t, list) else t.to(dev)
    inp = {k: mv(v) for k, v in inp.items()}
    d, dtype = case.d, case.dtype
    gamma, beta, pe = inp["gamma"], inp["beta"], inp["pe"]
    vec = ln_is_vec(d, dtype) and case.misaligned < 0
    out = []
    for p in VIEWS_P:
        sd = VIEWS_SEED_DEV if p > 0 else None
        keeps = [(_mask2d(drop_key(s, sd), r, d, p, dev) if p > 0 else None) for s, r in zip(VIEW_SEEDS, case.rows)]
        got = impl.views_fwd(case, inp["x"], gamma, beta, pe, VIEW_PE_ROWS, VIEW_SEEDS, p, sd, EPS)
        stats = []
        for i, (x, (y, mean, rstd)) in enumerate(zip(inp["x"], got)):
            ref = ln_fwd_ref(x.double(), gamma, beta, pe, VIEW_PE_ROWS[i], EPS, dtype, vec)
            yr, yb = ref["y"] if p == 0 else drop_ref(*ref["y"], keeps[i], p, dtype)
            out += [(f"views.y[p={p},view {i}]", y, yr, yb), (f"views.mean[p={p},view {i}]", mean, *ref["mean"]),
                    (f"views.rstd[p={p},view {i}]", rstd, *ref["rstd"])]
            stats.append((ref["mean"][0].float(), ref["rstd"][0].float()))
        dyf = [ln_dy_in(dy, k, p, dtype) for dy, k in zip(inp["dy"], keeps)]
        dxs, dg, db = impl.views_bwd(case, inp["x"], gamma, stats, inp["dy"], VIEW_SEEDS, p, sd, inp["dgamma0"],
                                     inp["dbeta0"])
        rg, rb = inp["dgamma0"].double(), inp["dbeta0"].double()
        bg, bb = torch.zeros_like(rg), torch.zeros_like(rb)
        for i, x in enumerate(inp["x"]):
            if case.rows[i] == 0:
                continue
            (dxr, dxb), (sg, sb, ag, ab) = ln_bwd_ref(x.double(), gamma, *stats[i], dyf[i], dtype, vec)
            out.append((f"views.dx[p={p},view {i}]", dxs[i], dxr, dxb))
            depth = ln_grad_depth(case.rows[i], d)
            rg, rb = rg + sg, rb + sb  # the views add in view order
            bg, bb = bg + (depth + 3) * U * ag + U * rg.abs(), bb + depth * U * ab + U * rb.abs()
        out += [(f"views.dgamma[p={p}]", dg, rg, bg), (f"views.dbeta[p={p}]", db, rb, bb)]
    return out


# ------------------------------------------------------------------ embedding
@dataclasses.dataclass(frozen=True)
class EmbCase:
    name: str
    b: int
    t: int
    d: int
    geom: tuple  # (chunks, second cb pass, tokens from HBM, EMB_COLS passes, leader c0 passes)
    dtypes: tuple = (F32, BF16)
    note: str = ""


EMB_CHUNK, EMB_COLS, VOCAB, EMB_P = 64, 512, 48, 0.1
EMB_CASES = [
    EmbCase("b4_t31_512", 4, 31, 512, (2, False, False, 1, 1), note="124 positions, two chunks"),
    EmbCase("one_position", 1, 1, 8, (1, False, False, 1, 1), note="one position, one live lane group"),
    EmbCase("d300", 3, 21, 300, (1, False, False, 1, 1), note="d = 300: ragged columns"),
    EmbCase("d1024", 2, 33, 1024, (2, False, False, 2, 2), note="EMB_COLS and the leader's c0 loop run twice"),
    EmbCase("second_cb_pass", 3, 1400, 8, (66, True, False, 1, 1),
            note="4200 positions: 66 chunks, the leader's cb += EMB_CHUNK loop runs a second pass"),
    EmbCase("tokens_from_hbm", 2, 4101, 8, (129, True, True, 1, 1), note="8202 positions > 8192: lds == 0"),
]
EMB_BY_NAME = {c.name: c for c in EMB_CASES}
EMB_SEED, EMB_SEED_DEV = 99, 3


def emb_geom(rows, d):
    nch = cdiv(rows, EMB_CHUNK)
    return nch, nch > EMB_CHUNK, rows > 8192, cdiv(d, EMB_COLS), cdiv(d, 512)


def emb_inputs(case, dtype):
    g = torch.Generator().manual_seed(_seed("emb_" + case.name))
    rows, d = case.b * case.t, case.d
    tok = torch.randint(1, VOCAB - 2, (rows,), generator=g)  # id VOCAB - 2 never occurs
    tok[torch.rand(rows, generator=g) < 0.4] = 0  # ~40 % padding
    tok[rows // 2] = VOCAB - 1  # occurs once
    return {"tok": tok.to(torch.int32), "emb": torch.randn(VOCAB, d, generator=g),
            "pe": torch.randn(case.t, d, generator=g), "dy": torch.randn(rows, d, generator=g).to(dtype),
            "d_emb0": torch.randn(VOCAB, d, generator=g) * 3, "sumsq0": torch.tensor([2.5])}


def emb_suite(case, dtype, impl, dev="cpu"):
    inp = {k: v.to(dev) for k, v in emb_inputs(case, dtype).items()}
    tok, emb, pe, dy = inp["tok"].long(), inp["emb"], inp["pe"], inp["dy"]
    rows, d = case.b * case.t, case.d
    pos = torch.arange(rows, device=dev) % case.t
    e, q = emb.double()[tok], pe.double()[pos]
    yr, yb = e + q, U * (e.abs() + q.abs())
    yb = yb + store_u(dtype) * yr.abs()
    # per id: positions, most positions in one chunk, chunks
    onehot = torch.zeros(rows, VOCAB, dtype=F64, device=dev)
    onehot[torch.arange(rows, device=dev), tok] = 1.0
    pad = cdiv(rows, EMB_CHUNK) * EMB_CHUNK - rows
    per_chunk = torch.cat([onehot, onehot.new_zeros(pad, VOCAB)]).view(-1, EMB_CHUNK, VOCAB).sum(1)
    depth = (per_chunk.max(0).values + (per_chunk > 0).double().sum(0) + 1)[:, None]
    sq_depth = cdiv(d, 64) + 1 + 6 + cdiv(rows, 256) + 6 + 2
    out = []
    for p, sd in ((0.0, None), (EMB_P, None), (EMB_P, EMB_SEED_DEV)):
        tag = f"[p={p},{'dev' if sd else 'null'}]"
        keep = _mask2d(drop_key(EMB_SEED, sd), rows, d, p, dev) if p > 0 else None
        y = impl.embed_fwd(case, dtype, inp["tok"], emb, pe, p, EMB_SEED, sd)
        out.append((f"embed.y{tag}", y, *((yr, yb) if p == 0 else drop_ref(yr, yb, keep, p, dtype))))
        g = ln_dy_in(dy, keep, p, dtype).double()
        s, a = onehot.t() @ g, onehot.t() @ g.abs()
        ss = (g * g).sum().view(1)
        de, sumsq = impl.embed_bwd(case, inp["tok"], dy, inp["d_emb0"], inp["sumsq0"], p, EMB_SEED, sd)
        dr = inp["d_emb0"].double() + s
        sr = inp["sumsq0"].double() + ss
        out += [(f"embed.d_emb{tag}", de, dr, depth * U * a + U * dr.abs() * (a > 0).double()),
                (f"embed.sumsq{tag}", sumsq, sr, sq_depth * U * ss + U * sr.abs())]
        if p == 0:  # null sumsq
            de, _ = impl.embed_bwd(case, inp["tok"], dy, inp["d_emb0"], None, p, EMB_SEED, sd)
            out.append(("embed.d_emb[null sumsq]", de, dr, depth * U * a + U * dr.abs() * (a > 0).double()))
    return out


# -------------------------------------------------------------- cross-entropy
@dataclasses.dataclass(frozen=True)
class XentCase:
    name: str
    rows: int
    v: int
    data: str = "normal"
    note: str = ""


XENT_CASES = [
    XentCase("v7", 5, 7, note="v < 256: 249 lanes start at -inf"),
    XentCase("v256", 3, 256, note="v == 256: every lane one element"),
    XentCase("v1000", 37, 1000, note="ragged last stride"),
    XentCase("v10003", 4, 10003, note="40 strides, ragged"),
    XentCase("pm80_v7", 5, 7, data="pm80", note="logits near +-80"),
    XentCase("pm80_v1000", 37, 1000, data="pm80", note="logits near +-80"),
    XentCase("pm80_v10003", 4, 10003, data="pm80", note="logits near +-80: exp overflows unless the max is subtracted"),
    XentCase("all_pad", 5, 1000, data="all_pad", note="every label 0: loss exactly 0, dlogits all zero"),
]
XENT_BY_NAME = {c.name: c for c in XENT_CASES}
XENT_LD, XENT_LDD = 5, 3  # ld = v + 5, ldd = v + 3
XENT_SCALES = (1.0, 0.125)
XENT_DTYPES = (F32, BF16)


def xent_inputs(case):
    g = torch.Generator().manual_seed(_seed("xent_" + case.name))
    rows, v = case.rows, case.v
    x = 3 * torch.randn(rows, v, generator=g)
    if case.data == "pm80":
        u = torch.rand(rows, v, generator=g)
        n = 0.5 * torch.randn(rows, v, generator=g)
        x = torch.where(u < 0.8, 80 + n, torch.where(u < 0.9, -80 + n, x))
    lab = torch.randint(1, v, (rows,), generator=g)
    lab[0] = v - 1  # the last column
    if rows > 2:
        lab[1] = 0  # a masked row
    if case.data == "all_pad":
        lab[:] = 0
    return {"logits": x, "labels": lab.to(torch.int32)}


def xent_ref(x, lab, gscale, dtype):
    """{label: (ref, bound)} of loss and dlogits."""
    rows, v = x.shape
    xd = x.double()
    m = xd.max(1, keepdim=True).values
    z = xd - m
    e = z.exp()
    s = e.sum(1, keepdim=True)
    arg = U * z.abs() + EXPU
    eps_s = (e * arg).sum(1, keepdim=True) / s + (cdiv(v, 256) + 9) * U
    mask = (lab != 0).double()[:, None]
    ls = s.log()
    rl = ((m + ls) - xd.gather(1, lab.long()[:, None])) * mask
    brl = (eps_s + LOGU * ls.abs() + U * (m + ls).abs() + U * rl.abs()) * mask
    loss = rl.sum().view(1) / rows
    bl = brl.sum().view(1) / rows + (cdiv(rows, 256) + 10) * U * rl.abs().sum().view(1) / rows
    p = e / s
    onehot = torch.zeros_like(p).scatter_(1, lab.long()[:, None], 1.0)
    coef = mask * f32(gscale) / rows
    dl = (p - onehot) * coef
    bd = coef.abs() * (p * (arg + eps_s + U) + onehot * U * (p - 1).abs()) + (2 * U + store_u(dtype)) * dl.abs() \
        + TINY * (coef != 0).double()
    return {"loss": (loss, bl), "dlogits": (dl, bd)}


def xent_suite(case, impl, dev="cpu"):
    inp = {k: v.to(dev) for k, v in xent_inputs(case).items()}
    x, lab = inp["logits"], inp["labels"]
    out = []
    for dtype in XENT_DTYPES:
        for gs in XENT_SCALES:
            ref = xent_ref(x, lab, gs, dtype)
            loss, dl = impl.xent(case, x, lab, dtype, gs, True)
            tag = f"[{short(dtype)},scale={gs}]"
            out += [(f"xent.loss{tag}", loss, *ref["loss"]), (f"xent.dlogits{tag}", dl, *ref["dlogits"])]
    loss, _ = impl.xent(case, x, lab, F32, 1.0, False)
    out.append(("xent.loss[null dlogits]", loss, *xent_ref(x, lab, 1.0, F32)["loss"]))
    return out


# ------------------------------------------------------ activation backward
@dataclasses.dataclass(frozen=True)
class ActCase:
    name: str
    rows: int
    c: int
    geom: dict  # dtype -> act_bwd_grid(rows, c, dtype, aligned) the case is meant to hit
    dtypes: tuple = (F32, BF16)
    offset: int = 0
    data: str = "normal"
    acts: tuple = ("none", "relu", "relu6", "leaky")
    note: str = ""


ACT_P = (0.0, 0.25)
LEAKY = 0.2
ACT_CASES = [
    ActCase("scalar_5x3", 5, 3, {F32: (False, 3, 1, 5, 1, 256), BF16: (False, 3, 1, 5, 1, 256)}, note="scalar, c = 3"),
    ActCase("r37_c12", 37, 12, {F32: (True, 3, 1, 37, 1, 256), BF16: (False, 12, 1, 37, 1, 256)},
            note="fp32 vectorised (3 groups), bf16 scalar (12 % 8)"),
    ActCase("one_launch_gt3", 200, 1536, {BF16: (True, 64, 1, 200, 3, 64)}, dtypes=(BF16,),
            note="one-launch column sums, GT = 3: lanes tr >= 64 idle"),
    ActCase("one_launch_gt5", 100, 2560, {BF16: (True, 64, 1, 100, 5, 32)}, dtypes=(BF16,),
            note="one-launch column sums, GT = 5"),
    ActCase("cb64", 300, 4096, {BF16: (True, 2, 75, 4, 256, 1)}, dtypes=(BF16,),
            note="c >= 4096: act_colsum_kernel<64>, gy = 75 > 1"),
    ActCase("many_chunks", 3000, 64, {F32: (True, 1, 47, 64, 16, 16), BF16: (True, 1, 24, 125, 8, 32)},
            note="many row chunks through act_colsum_kernel<16>"),
    ActCase("misaligned", 9, 512, {F32: (False, 64, 1, 9, 8, 32), BF16: (False, 64, 1, 9, 8, 32)}, offset=1,
            note="pointers offset by one element: the scalar route"),
    ActCase("relu6_edges", 37, 64, {F32: (True, 16, 1, 37, 1, 256), BF16: (True, 8, 1, 37, 1, 256)}, data="edges",
            acts=("relu6",), note="stored y at exactly 0 and exactly 6"),
]
ACT_BY_NAME = {c.name: c for c in ACT_CASES}
ACT_SEED, ACT_SEED_DEV = 4242, 9


def act_inputs(case, dtype):
    g = torch.Generator().manual_seed(_seed("act_" + case.name))
    rows, c = case.rows, case.c
    y = 3 * torch.randn(rows, c, generator=g) + 1.5
    if case.data == "edges":
        y = y.clamp(0.0, 6.0)
    return {"dy": torch.randn(rows, c, generator=g).to(dtype), "y": y.to(dtype), "db0": torch.randn(c, generator=g) * 3}


def act_grad(y, act):
    yd = y.double()
    if act == "relu":
        return (yd > 0).double()
    if act == "relu6":
        return ((yd > 0) & (yd < 6)).double()
    if act == "leaky":
        return torch.where(yd > 0, 1.0, f32(LEAKY)).double()
    return torch.ones_like(yd)


def act_suite(case, dtype, impl, dev="cpu"):
    inp = {k: v.to(dev) for k, v in act_inputs(case, dtype).items()}
    dy, y, db0 = inp["dy"], inp["y"], inp["db0"]
    rows, c = dy.shape
    depth = act_db_depth(rows, c, dtype, case.offset == 0)
    out = []
    for act in case.acts:
        for p, sd in ((0.0, None), (ACT_P[1], None), (ACT_P[1], ACT_SEED_DEV)):
            tag = f"[{act},p={p},{'dev' if sd else 'null'}]"
            ref = dy.double() * act_grad(y, act)
            n = int(act == "leaky")
            if p > 0:
                keep = _mask2d(drop_key(ACT_SEED, sd), rows, c, p, dev)
                ref = torch.where(keep, ref * drop_scale(p), torch.zeros((), dtype=F64, device=dev))
                n += 1
            dz, db = impl.act_bwd(case, dtype, act, dy, y if act != "none" else None, db0, p, ACT_SEED, sd)
            s, a = dz.double().sum(0), dz.double().abs().sum(0)  # from the stored dz
            out += [(f"act.dz{tag}", dz, ref, (n * U + store_u(dtype)) * ref.abs() if n else torch.zeros_like(ref)),
                    (f"act.db{tag}", db, db0.double() + s, grad_bound(depth, 0, s, a, db0))]
    s, a = dy.double().sum(0), dy.double().abs().sum(0)
    out.append(("bias_grad", impl.bias_grad(case, dtype, dy, db0), db0.double() + s, grad_bound(depth, 0, s, a, db0)))
    dz, _ = impl.act_bwd(case, dtype, "leaky", dy, y, None, 0.0, 0, None)  # null db
    ref = dy.double() * act_grad(y, "leaky")
    out.append(("act.dz[leaky,null db]", dz, ref, (U + store_u(dtype)) * ref.abs()))
    return out


# --------------------------------------------------------- dropout, cast, add
FLAT_SIZES = (1, 4096 * 256 + 3)  # one element; past the grid cap: the grid-stride loop
FLAT_P = 0.5
# under seed 253 an element of the large size has u == p exactly, with the device
# seed null (137345 under seed_dev 31): a `>` for `>=` flips it (test_row_kernel_bars)
FLAT_SEED = {1: 7, 4096 * 256 + 3: 253}
FLAT_SEED_DEV = 31


def bf16_rne(x):
    """fp32 -> bf16 by integer arithmetic, round to nearest even (finite inputs)."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(BF16)


def flat_inputs(n):
    g = torch.Generator().manual_seed(_seed(f"flat_{n}"))
    a, b = 3 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n >= 8:
        a[1], a[2], a[3] = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.998  # two ties, a round-up into the next binade
        a[4], a[5] = -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20
    return a, b


def flat_suite(n, impl, dev="cpu"):
    a, b = (t.to(dev) for t in flat_inputs(n))
    z = lambda t: torch.zeros(t.shape, dtype=F64, device=dev)
    out = []
    rne = bf16_rne(a)
    assert n < 8 or [float(v) for v in rne[1:6]] == [1.0, 1.015625, 2.0, -1.0, 1.0078125]
    out.append(("cast[f32->bf16]", impl.cast(a, BF16), rne.double(), z(a)))
    out.append(("cast[bf16->f32]", impl.cast(rne, F32), rne.double(), z(a)))
    out.append(("cast[f32->f32]", impl.cast(a, F32), a.double(), z(a)))
    out.append(("cast[bf16->bf16]", impl.cast(rne, BF16), rne.double(), z(a)))
    for dtype in (F32, BF16):
        at, bt = a.to(dtype), b.to(dtype)
        ref = (at.float() + bt.float()).to(dtype)
        out.append((f"add[{short(dtype)}]", impl.add(at, bt), ref.double(), z(a)))
        for sd in (None, FLAT_SEED_DEV):
            keep = keep_mask(drop_key(FLAT_SEED[n], sd), n, FLAT_P).to(dev)
            out.append((f"dropout[{short(dtype)},{'dev' if sd else 'null'}]", impl.dropout(at, FLAT_P, FLAT_SEED[n], sd),
                        drop_round(at, keep, FLAT_P, dtype).double(), z(a)))
    return out


# ------------------------------------------------------------------ comparing
def compare(out, ref, bnd):
    """(all elements inside the bound, worst err / bound)."""
    err = (out.double() - ref).abs()
    bad = ~(err <= bnd)  # a NaN is outside
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    ratio = torch.where(bad & ~(ratio > 1), torch.full_like(ratio, math.inf), ratio)  # NaN / inf outputs
    return not bool(bad.any()), float(ratio.max()) if ratio.numel() else 0.0


def worst(rows):
    """({label: worst err / bound}, labels outside their bound)."""
    ratios, bad = {}, []
    for label, got, ref, bnd in rows:
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        ok, r = compare(got, ref, bnd.expand_as(ref))
        ratios[label] = r
        if not ok:
            bad.append(label)
    return ratios, bad

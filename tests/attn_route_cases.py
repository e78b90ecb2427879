"""Case table of the attention kernel routes (csrc/decode.hip, csrc/api.hip).

One entry per reachable (entry point, kernel, dtype): fpnmt_attention_fwd /
_bwd, fpnmt_attention_*_views and fpnmt_decode_attention each write one
`attn op= kernel= dtype= b= h= lq= lk= d= [n=]` line to FPNMT_GEMM_LOG per
launcher. Helper module, not collected: tests/test_attn_route_bars.py (no GPU)
proves on planted errors that the bound below can fail,
tests/test_gpu_attn_routes.py runs every case on the GPU in one child process
and checks route, numerics, padding and repeatability.

Every case is the reference's scaled_dot_product_attention
(models/transformer.py:70-104) on its own operands, through the C entry
points, so leading dimensions and base pointers are the case's to choose:

  * inputs: magnitudes in [0.5, 1] with random signs, rounded to the case's
    dtype, seeded on the CPU. A flat softmax hides a dropped key (one of Lk
    nearly uniform keys carries 1 / Lk of the weight), so a handful of edge
    keys are made hot: key 0, the last key and the keys on both sides of every
    stride a kernel uses (8, 16, 32, 64, 128, 256, 1024 where Lk reaches
    them). Hot key number t at j gets k_j = sign(q_i) of a designated query i
    with the channels c = t (mod 16) negated (its score is at least 3/4 of
    scale * sum |q_i|; identical hot keys would cancel in dq, see _hot_k) and
    v_j = +-sign(dO_i) with alternating sign, so each hot key holds a few to
    some tens of per cent of its row's weight and dP - sum P dP is large at
    each of them. Under a mask one hot key is
    masked; the others and the last key are kept, so every row keeps a key.
  * reference: fp64 on the CPU from the dtype-rounded operands,
        s = scale q k^T + mask * -1e9,  p = softmax(s),  out = p v,
        dp = dO v^T,  ds = p (dp - sum_l p dp),
        dq = scale ds k,  dk = scale ds^T q,  dv = p^T dO.
    The backward is fed the GPU forward's own weights buffer, as in the product.
  * bound (derived, not measured), u = 2^-8 (bf16 storage) or 2^-24 (fp32),
    f = 2^-23:
        sigma_i = D f scale max_j sum_c |q_ic| |k_jc|   (products of two bf16
                  values are exact in fp32; any fp32 summation order is within it)
        e_i     = u + 2 sigma_i + (Lk + 8) f            (relative error of a
                  stored weight: rounding to dtype, the score error through exp
                  and its sum, a few ulp for expf and the division)
        a_ij    = sum_c |dO_ic| |v_jc|
        weights  e_i p_ij + the dtype's smallest subnormal
        out      (e_i + Lk f) sum_j p_ij |v_j| + u |out|
        dv       sum_i (e_i + Lq f) p_ij |dO_i| + u |dv|
        E_ij   = (e_i + u) |ds_ij| + p_ij (e_i + Lk f) sum_l p_il |dp_il|
                 + p_ij D f (a_ij + sum_l p_il a_il)
        dq       scale (sum_j E_ij |k_j| + Lk f sum_j |ds_ij| |k_j|) + u |dq|
        dk       scale (sum_i E_ij |q_i| + Lq f sum_i |ds_ij| |q_i|) + u |dk|
    Decode attention (online softmax, weights never stored) bounds `out` only,
    with e_i without its u term.

Layout edges every case carries: B = 2 and H = 3 (a wrong batch or head stride
lands on other data; one H = 8 and some B = 1 cases), ld = H D + 8 on the 16-B
routes (+ 4, a base offset by one element, or D = 20 for the scalar bf16
routes, ldw = 40 for the scalar short-sequence kernel), padding columns of the
operands filled with a sentinel, outputs pre-filled with it and followed by two
guard rows. Masked weights and the weight columns from Lk to ldw must be
bitwise zero, the padding and guard rows untouched, two runs bitwise equal
(every reduction in these kernels is ordered).
"""
from __future__ import annotations

import dataclasses
import math
import os
import sys

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = -12352.0  # exact in bf16; no output of these cases comes near it
GUARD_ROWS = 2
SLACK = 8  # elements in front of every buffer, so its base can be moved by one element
STRIDES = (8, 16, 32, 64, 128, 256, 1024)  # key strides of the kernels' loops
FP = 2.0 ** -23


@dataclasses.dataclass(frozen=True)
class View:
    """One table entry of a fpnmt_attention_*_views case."""
    lk: int
    pads: tuple = (8, 8, 8, 8)
    mis: tuple = ()
    b: int | None = None  # 0: a view without images


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    op: str  # attn | views | decode
    fwd: str  # kernel= of the forward's attn line (views: of the views line)
    bwd: str = ""  # kernel= of the backward's (decode: none)
    dtype: torch.dtype = BF16
    B: int = 2  # decode: rows
    H: int = 3
    Lq: int = 1
    Lk: int = 1
    D: int = 64
    pads: tuple = (8, 8, 8, 8)  # ld - H D of q, k, v, out (dq / dk / dv / dO share them)
    ldw: int = 0  # 0: Lk rounded up to 8 (at least 8), the product's choice
    mask: str = ""  # "" | pad (key padding, strides 0 over heads and queries) | head (m_sh != 0) | causal (m_si != 0)
    mis: tuple = ()  # buffers whose base is moved by one element: q k v o w g dq dk dv
    views: tuple = ()
    per_view: tuple = ()  # views fallback: (fwd, bwd) kernel of each view's own line
    status: int = 0  # expected status of the entry point
    # decode
    src: bool = False  # cache rows through a src table (repeated and permuted rows), else row / row_div
    row_div: int = 1
    seed: int = 0
    note: str = ""

    @property
    def u(self):
        return 2.0 ** -8 if self.dtype == BF16 else 2.0 ** -24

    @property
    def tiny(self):
        return 2.0 ** -133 if self.dtype == BF16 else 2.0 ** -149

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.D)

    @property
    def ldw_(self):
        return self.ldw or max(8, (self.Lk + 7) // 8 * 8)

    @property
    def lds(self):
        return tuple(self.H * self.D + p for p in self.pads)

    @property
    def has_bwd(self):
        return self.op != "decode"

    @property
    def dname(self):
        return "bf16" if self.dtype == BF16 else "f32"


def _a(name, fwd, bwd, Lq, Lk, **kw):
    return Case(name, "attn", fwd, bwd, Lq=Lq, Lk=Lk, **kw)


def _d(name, fwd, Lk, **kw):
    kw.setdefault("B", 5)
    return Case(name, "decode", fwd, Lk=Lk, **kw)


_P4 = dict(pads=(4, 4, 4, 4))  # ld = H D + 4: no 16-B rows
_F = dict(dtype=F32, pads=(4, 4, 4, 4))
_SMALL = [(2, 1, ""), (32, 1, ""), (13, 17, "pad"), (17, 13, "head"), (31, 31, "causal"), (32, 32, "causal")]


def _small_cases():
    out = []
    for lq, lk, m in _SMALL:
        s = f"{lq}x{lk}"
        out.append(_a(f"small_mfma_{s}", "small_mfma", "small_mfma", lq, lk, mask=m))
        out.append(_a(f"small_vec_{s}", "small_vec", "small_vec", lq, lk, mask=m, D=32 if lq != 17 else 8))
        # the scalar bf16 kernel: ldw = 40 where Lk <= 32 allows a wider row, else no 16-B rows / D = 20
        how = dict(ldw=40) if lq in (13, 17, 31) else dict(ldw=40, D=48) if lq == 32 and lk == 32 else \
            _P4 if lq == 2 else dict(D=20)
        out.append(_a(f"small_scalar_{s}", "small_scalar", "small_scalar", lq, lk, mask=m, **how))
        out.append(_a(f"small_f32_{s}", "small_scalar", "small_scalar", lq, lk, mask=m, D=64 if lq % 2 else 24, **_F))
    return out


_DEC_LK = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)

CASES = [
    # ---- one query, bf16, 16-B rows, D = 64, Lk < 128: attn_q1_*_kernel<bf16, true>, D == 64 branch
    _a("q1_vec64_lk1", "q1_vec64", "q1_vec64", 1, 1),
    _a("q1_vec64_lk9", "q1_vec64", "q1_vec64", 1, 9, mask="pad"),
    _a("q1_vec64_lk63", "q1_vec64", "q1_vec64", 1, 63, mask="head"),
    _a("q1_vec64_lk65", "q1_vec64", "q1_vec64", 1, 65, H=8, note="H = 8"),
    _a("q1_vec64_lk127", "q1_vec64", "q1_vec64", 1, 127, mask="pad", B=1),
    _a("q1_vec64_fwd_scalar_bwd", "q1_vec64", "q1_scalar", 1, 65, mis=("dq",),
       note="the backward's predicate also looks at dq / dk / dv: dq off by one element"),
    # ---- the generic branch of the same instantiation (D % 8 == 0, D != 64)
    _a("q1_vec_d32_lk1", "q1_vec", "q1_vec", 1, 1, D=32),
    _a("q1_vec_d32_lk67", "q1_vec", "q1_vec", 1, 67, D=32, mask="head"),
    _a("q1_vec_d32_lk257", "q1_vec", "q1_vec", 1, 257, D=32, mask="pad"),
    _a("q1_vec_d8_lk1", "q1_vec", "q1_vec", 1, 1, D=8),
    _a("q1_vec_d8_lk67", "q1_vec", "q1_vec", 1, 67, D=8, mask="pad"),
    _a("q1_vec_d8_lk257", "q1_vec", "q1_vec", 1, 257, D=8),
    # ---- attn_q1_*_kernel<bf16, false>: no 16-B rows
    _a("q1_scalar_lk1", "q1_scalar", "q1_scalar", 1, 1, **_P4),
    _a("q1_scalar_lk2", "q1_scalar", "q1_scalar", 1, 2, mis=("k",), note="k off by one element"),
    _a("q1_scalar_lk67", "q1_scalar", "q1_scalar", 1, 67, D=20, mask="head"),
    _a("q1_scalar_lk130", "q1_scalar", "q1_scalar", 1, 130, mask="pad", **_P4,
       note="Lk >= 128 without the 16-B layout"),
    # ---- attn_q1_*_kernel<float, false>
    _a("q1_f32_lk1", "q1_scalar", "q1_scalar", 1, 1, **_F),
    _a("q1_f32_lk2", "q1_scalar", "q1_scalar", 1, 2, D=32, **_F),
    _a("q1_f32_lk9", "q1_scalar", "q1_scalar", 1, 9, mask="pad", **_F),
    _a("q1_f32_lk67", "q1_scalar", "q1_scalar", 1, 67, D=20, mask="head", **_F),
    # ---- attn_q1_*_mw_kernel: bf16, D = 64, Lk >= 128, 16-B rows
    _a("q1_mw_lk128", "q1_mw", "q1_mw", 1, 128),
    _a("q1_mw_lk130", "q1_mw", "q1_mw", 1, 130, mask="pad", H=8, note="H = 8"),
    _a("q1_mw_lk257", "q1_mw", "q1_mw", 1, 257, mask="head"),
    _a("q1_mw_lk1025", "q1_mw", "q1_mw", 1, 1025, B=1),
    _a("q1_mw_lk4096", "q1_mw", "q1_mw", 1, 4096, mask="pad"),
    _a("q1_mw_fwd_scalar_bwd", "q1_mw", "q1_scalar", 1, 130, mis=("dv",), note="dv off by one element"),
    # ---- the fused short-sequence kernels (Lq, Lk <= 32, ldw <= 64)
    *_small_cases(),
    _a("small_mfma_fwd_scalar_bwd", "small_mfma", "small_scalar", 13, 17, mis=("dk",), mask="pad",
       note="dk off by one element"),
    # ---- the general path: three launches forward, five backward
    _a("general_33x32", "general", "general", 33, 32),
    _a("general_32x33", "general", "general", 32, 33, mask="pad"),
    _a("general_40x40", "general", "general", 40, 40, mask="causal"),
    _a("general_d72_3x5", "general", "general", 3, 5, D=72, mask="head"),
    _a("general_lk0", "general", "zero_fill", 3, 0, note="no keys: out, weights and dq exactly zero"),
    _a("general_q1_lk4097", "general", "general", 1, 4097, B=1, H=1, note="one query past Q1_MAX_LK"),
    _a("general_f32_33x32", "general", "general", 33, 32, mask="head", **_F),
    _a("general_f32_40x40", "general", "general", 40, 40, mask="causal", **_F),
    _a("general_f32_d72_3x5", "general", "general", 3, 5, D=72, **_F),
    _a("general_f32_lk0", "general", "zero_fill", 3, 0, **_F),
    # ---- the views entry points (one query, bf16, D = 64; every view its own leading dimensions)
    Case("views_pyramid", "views", "views_grouped", "views_grouped",
         views=(View(784), View(196, (16, 8, 24, 8)), View(49, (8, 24, 16, 16)), View(9, (24, 16, 8, 24)))),
    Case("views_keyless", "views", "views_grouped", "views_grouped",
         views=(View(130, (8, 16, 8, 8)), View(1, (16, 8, 8, 24)), View(0, (8, 8, 16, 8)), View(64, (24, 8, 8, 16))),
         note="a view without keys: zero out / weights / dq from the grouped launch"),
    Case("views_b0", "views", "views_grouped", "views_grouped",
         views=(View(130), View(9, (16, 8, 8, 8), b=0), View(64, (8, 16, 16, 8)), View(1, (8, 8, 24, 8))),
         note="a view with b = 0 is left out of the grouped launch (n = 3 in the log)"),
    Case("views_n5_b0", "views", "", "", status=-1,
         views=(View(130), View(9, b=0), View(64), View(1), View(17)),
         note="n = 5 > FPNMT_MAX_VIEWS = 4 is refused (FPNMT_E_ARG) even when one of the five views is empty: "
              "the limit is on the table, not on the views that launch; nothing is logged or written"),
    Case("views_fallback", "views", "per_view", "per_view",
         views=(View(130, (8, 16, 8, 8)), View(9, (4, 4, 4, 4)), View(64, (16, 8, 8, 24))),
         per_view=(("q1_mw", "q1_mw"), ("q1_scalar", "q1_scalar"), ("q1_vec64", "q1_vec64")),
         note="view 1 has no 16-B rows: the calls one by one, each with its own line"),
    # ---- decode attention: R = 5 rows, one query each
    *[_d(f"dec_v_lk{lk}", "dec_v2" if lk <= 16 else "dec_v4", lk, src=bool(i % 2), row_div=1 if i % 2 else 3)
      for i, lk in enumerate(_DEC_LK)],
    _d("dec_v4_h8_lk32", "dec_v4", 32, H=8, src=True, note="H = 8"),
    _d("dec_v2_h8_lk16", "dec_v2", 16, H=8, row_div=3),
    *[_d(f"dec_scalar_d32_lk{lk}", "dec_scalar", lk, D=32, H=8, src=bool(i % 2), row_div=1 if i % 2 else 3)
      for i, lk in enumerate((0, 1, 17, 64, 65, 129))],
    _d("dec_scalar_ldo_lk16", "dec_scalar", 16, pads=(8, 8, 8, 4), src=True, note="misaligned ldo"),
    _d("dec_scalar_ldo_lk33", "dec_scalar", 33, pads=(8, 8, 8, 4), row_div=3, note="misaligned ldo"),
    *[_d(f"dec_f32_lk{lk}", "dec_scalar", lk, dtype=F32, src=bool(i % 2), row_div=1 if i % 2 else 3)
      for i, lk in enumerate((0, 15, 65))],
    *[_d(f"dec_f32_d32_lk{lk}", "dec_scalar", lk, dtype=F32, D=32, H=8, src=not i % 2, row_div=3 if i % 2 else 1)
      for i, lk in enumerate((1, 63, 129))],
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_K10 = ("q1_mw", "q1_vec64", "q1_vec", "q1_scalar", "small_mfma", "small_vec", "small_scalar", "general")
# (op, kernel, dtype) triples the launchers can log
REACHABLE = (
    {("fwd", k, "bf16") for k in _K10} | {("bwd", k, "bf16") for k in _K10}
    | {(o, k, "f32") for o in ("fwd", "bwd") for k in ("q1_scalar", "small_scalar", "general")}
    | {("bwd", "zero_fill", "bf16"), ("bwd", "zero_fill", "f32")}
    | {(o, k, "bf16") for o in ("views_fwd", "views_bwd") for k in ("views_grouped", "per_view")}
    | {("decode", "dec_v2", "bf16"), ("decode", "dec_v4", "bf16"), ("decode", "dec_scalar", "bf16"),
       ("decode", "dec_scalar", "f32")}
)
# Triples the predicates exclude:
#   q1_mw / q1_vec64 / q1_vec / small_mfma / small_vec / views_grouped / dec_v2 / dec_v4 in f32:
#       every 16-B kernel is bf16 only (q1_vec, small_vec, attn_q1_view_ok and v16 ask for FPNMT_BF16)
#   (views_*, per_view, f32) is logged only with d[0].dtype == f32, which the table does not hold: the per-view
#       calls of such a table log the f32 lines of the single-view entry points, which the table covers
#   (fwd, zero_fill): the forward without keys goes through the general path's softmax and a K = 0 GEMM
# The bf16 scalar fallbacks (attn_q1_*<bf16, false>, attn_small_*<bf16>) are reachable: any operand without
# 16-B rows (ld % 8 != 0, a base moved by one element, D % 8 != 0) or, for the short-sequence kernel, ldw > 32.
UNREACHABLE = (
    {(o, k, "f32") for o in ("fwd", "bwd") for k in ("q1_mw", "q1_vec64", "q1_vec", "small_mfma", "small_vec")}
    | {(o, k, "f32") for o in ("views_fwd", "views_bwd") for k in ("views_grouped", "per_view")}
    | {("decode", "dec_v2", "f32"), ("decode", "dec_v4", "f32")}
    | {("fwd", "zero_fill", "bf16"), ("fwd", "zero_fill", "f32")}
)


# ------------------------------------------------------------------ inputs
def _rnd(g, *shape, dtype=BF16):
    mag = torch.rand(*shape, generator=g) * 0.5 + 0.5
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn).to(dtype)


def _seed_of(case):
    return sum((i + 1) * b for i, b in enumerate(case.name.encode())) * 7919 + case.seed


def subcases(case):
    """The single attention problems of a case: itself, or one per view."""
    if case.op != "views":
        return [case]
    return [dataclasses.replace(case, name=f"{case.name}.v{i}", op="attn", Lk=v.lk, pads=v.pads, mis=v.mis, views=(),
                                B=case.B if v.b is None else v.b) for i, v in enumerate(case.views)]


def hot_keys(case):
    """Sorted hot keys: key 0, the last key, both sides of every stride below Lk."""
    Lk = case.Lk
    if Lk == 0:
        return []
    return sorted({0, Lk - 1} | {j for s in STRIDES if s < Lk for j in (s - 1, s)})


def masked_hot(case):
    """The hot key a mask hides (pad / head: for every query; causal: for the queries before it)."""
    hot = hot_keys(case)[:-1]
    if not case.mask or not hot:
        return None
    if case.mask == "causal":
        return hot[-1] if hot[-1] > 0 else None
    return hot[len(hot) // 2]


def boundary_hot(case):
    """A hot key next to a stride boundary, kept by the mask and not the last one."""
    Lk, jm = case.Lk, masked_hot(case) if case.mask != "causal" else None
    cand = [j for s in STRIDES if s < Lk for j in (s - 1, s) if j != Lk - 1 and j != jm]
    return max(cand) if cand else None


def wave_block(case):
    """The keys of one wave's / one 64-key partial: from the last 64-key block
    (the upper half of a short row) to the end; where that holds an even
    number of hot keys, whose alternating dP cancel in the partial, from the
    next stride boundary below Lk that leaves an odd number (at worst the last key alone)."""
    Lk, hot = case.Lk, hot_keys(case)
    starts = [64 * ((Lk - 1) // 64) if Lk > 64 else Lk // 2] + [s for s in reversed(STRIDES) if s < Lk] + [Lk - 1]
    j0 = next(j for j in starts if sum(h >= j for h in hot) % 2)
    return slice(j0, Lk)


def _hot_k(qrow, t):
    """k of hot key number t for the query row(s) qrow [..., D]: sign(q), with
    the channels c = t (mod 16) negated. All hot keys of one query being the
    same vector would make their (large, opposite) ds terms cancel in dq
    (sum_j ds_j = 0), leaving dq below its own bound; the negated group keeps
    7/8 or more of the hot score and gives dq a term of the size of ds_j."""
    k = torch.sign(qrow).clone()
    k[..., t % 16::16] *= -1
    return k


def _designated(case, t, j):
    if case.mask == "causal":
        return j + t % (case.Lq - j)  # a query that sees key j
    return t % case.Lq


def _mask_of(case, g):
    """The mask operand as the kernel reads it: (tensor, (m_sb, m_sh, m_si, m_sj)), and its [B, H, Lq, Lk] view."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    if not case.mask:
        return None, (0, 0, 0, 0), torch.zeros(B, H, Lq, Lk, dtype=F64)
    if case.mask == "causal":
        m = torch.triu(torch.ones(Lq, Lk), diagonal=1)
        return m, (0, 0, Lk, 1), m.double().expand(B, H, Lq, Lk)
    shape = (B, Lk) if case.mask == "pad" else (B, H, Lk)
    m = (torch.rand(*shape, generator=g) < 0.25).float()
    m[..., hot_keys(case)] = 0.0
    if masked_hot(case) is not None:
        m[..., masked_hot(case)] = 1.0
    if case.mask == "pad":
        return m, (Lk, 0, 0, 1), m.double()[:, None, None, :].expand(B, H, Lq, Lk)
    return m, (H * Lk, Lk, 0, 1), m.double()[:, :, None, :].expand(B, H, Lq, Lk)


_CACHE = {}


def inputs(case):
    """Seeded CPU inputs of a single problem (op attn or decode), logical
    [B, H, L, D] tensors in the case's dtype: q, k, v, g (dO), the mask; decode
    cases add the cache they are gathered from."""
    assert case.op != "views"
    if case.name in _CACHE:
        return _CACHE[case.name]
    while len(_CACHE) >= 8:
        _CACHE.pop(next(iter(_CACHE)))
    g = torch.Generator().manual_seed(_seed_of(case))
    B, H, Lq, Lk, D, dt = case.B, case.H, case.Lq, case.Lk, case.D, case.dtype
    q, gg = _rnd(g, B, H, Lq, D, dtype=dt), _rnd(g, B, H, Lq, D, dtype=dt)
    inp = {"q": q, "g": gg}
    if case.op == "decode":
        rc = B  # cache rows
        kc, vc = _rnd(g, rc, max(Lk, 1), H, D, dtype=dt), _rnd(g, rc, max(Lk, 1), H, D, dtype=dt)
        hot = hot_keys(case)
        if case.src:
            src = torch.randint(0, rc, (B, Lk + 3), generator=g, dtype=torch.int32)
            perm = torch.randperm(rc, generator=g).to(torch.int32)
            for j in hot:
                src[:, j] = perm  # the rows' hot entries in distinct cache rows
            rows = src[:, :Lk].long()
            inp["src"] = src
        else:
            rows = (torch.arange(B) // case.row_div)[:, None].expand(B, Lk)
        for t, j in enumerate(hot):
            for r in reversed(range(B)):  # rows sharing a cache row: the lowest row's query is the designated one
                kc[rows[r, j], j] = _hot_k(q[r, :, 0], t)
                vc[rows[r, j], j] = torch.sign(q[r, :, 0]) * (1 - 2 * (t % 2))
        pos = torch.arange(Lk)[None, :].expand(B, Lk)
        inp.update(kc=kc, vc=vc, k=kc[rows, pos].permute(0, 2, 1, 3).contiguous(),
                   v=vc[rows, pos].permute(0, 2, 1, 3).contiguous())
    else:
        k, v = _rnd(g, B, H, Lk, D, dtype=dt), _rnd(g, B, H, Lk, D, dtype=dt)
        for t, j in enumerate(hot_keys(case)):
            i = _designated(case, t, j)
            k[:, :, j] = _hot_k(q[:, :, i], t)
            v[:, :, j] = torch.sign(gg[:, :, i]) * (1 - 2 * (t % 2))
        inp.update(k=k, v=v)
    inp["mask_t"], inp["mask_strides"], inp["mask"] = _mask_of(case, g)
    _CACHE[case.name] = inp
    return inp


# ------------------------------------------------- reference, plants, bound
FWD_PLANTS = ("pv_last", "sum_last", "hot_boundary", "head_v", "unnorm_wave", "mask_kept", "mask_row_shift")
BWD_PLANTS = ("dsum_partial", "dq_last", "dkv_last_query", "dq_scale_twice")
PLANT_DOC = {
    "pv_last": "the last key dropped from P V",
    "sum_last": "the last key dropped from the softmax sum",
    "hot_boundary": "a hot key at a stride boundary dropped from P V",
    "head_v": "head h reading head h - 1's V",
    "unnorm_wave": "weights left unnormalised by one wave's share of the sum",
    "mask_kept": "a masked hot key treated as kept",
    "mask_row_shift": "the mask row of query i - 1 used for query i (causal)",
    "dsum_partial": "one 64-key (or one wave's) partial missing from sum P dP",
    "dq_last": "the last key's term missing from dq",
    "dkv_last_query": "the last query's term missing from dk / dv",
    "dq_scale_twice": "scale applied once too often in dq",
}


def plant_names(case):
    """The plants that apply to a single problem, from its table entry alone."""
    Lq, Lk = case.Lq, case.Lk
    if Lk == 0 or case.B == 0:
        return []  # nothing is computed: the outputs are exact zeros (or untouched)
    out = ["pv_last", "sum_last"]
    if boundary_hot(case) is not None:
        out.append("hot_boundary")
    if case.H > 1:
        out.append("head_v")
    if Lk >= 2:
        out.append("unnorm_wave")
    if masked_hot(case) is not None:
        out.append("mask_kept")
    if case.mask == "causal":
        out.append("mask_row_shift")
    if case.has_bwd:
        if Lk >= 2:  # one key: p = 1, ds = 0, dq = dk = 0
            out += ["dsum_partial", "dq_last", "dq_scale_twice"]
        if Lq > 1:
            out.append("dkv_last_query")
    return out


def compute(case, inp, plant=None):
    """fp64 attention forward and backward of a single problem, with one planted
    kernel error if asked. [B, H, L, *] tensors: w, out, dq, dk, dv."""
    q, k, v, g, mask = (inp[n].double() for n in ("q", "k", "v", "g", "mask"))
    B, H, Lq, Lk, D, sc = case.B, case.H, case.Lq, case.Lk, case.D, case.scale
    if Lk == 0 or B == 0:
        z = torch.zeros(B, H, Lq, D, dtype=F64)
        return {"w": torch.zeros(B, H, Lq, 0, dtype=F64), "out": z, "dq": z.clone(),
                "dk": torch.zeros(B, H, 0, D, dtype=F64), "dv": torch.zeros(B, H, 0, D, dtype=F64)}
    blk = wave_block(case)

    def softmax(mk, pl):
        s = sc * q @ k.transpose(-1, -2) + mk * -1e9
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        tot = e.sum(-1, keepdim=True)
        if pl == "sum_last":
            tot = tot - e[..., -1:]
        if pl == "unnorm_wave":
            tot = tot - e[..., blk].sum(-1, keepdim=True)
        return e / tot

    mk = mask
    if plant == "mask_kept":
        mk = mask.clone()
        mk[..., masked_hot(case)] = 0.0
    if plant == "mask_row_shift":
        mk = mask.clone()
        mk[..., 1:, :] = mask[..., :-1, :]
    p = softmax(mask, None)
    w = softmax(mk, plant) if plant in ("sum_last", "unnorm_wave", "mask_kept", "mask_row_shift") else p
    vf = v
    if plant == "head_v":
        vf = v.clone()
        vf[:, 1:] = v[:, :-1]
    out = w @ vf
    if plant == "pv_last":
        out = out - w[..., -1:] * vf[..., -1:, :]
    if plant == "hot_boundary":
        j = boundary_hot(case)
        out = out - w[..., j:j + 1] * vf[..., j:j + 1, :]
    res = {"w": w, "out": out, "p": p}
    if not case.has_bwd:
        return res
    dp = g @ v.transpose(-1, -2)
    rs = (p * dp).sum(-1, keepdim=True)
    if plant == "dsum_partial":
        rs = rs - (p * dp)[..., blk].sum(-1, keepdim=True)
    ds = p * (dp - rs)
    dq = sc * ds @ k
    if plant == "dq_last":
        dq = dq - sc * ds[..., -1:] * k[..., -1:, :]
    if plant == "dq_scale_twice":
        dq = dq * sc
    dk, dv = sc * ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g
    if plant == "dkv_last_query":
        dk = dk - sc * ds[..., -1:, :].transpose(-1, -2) * q[..., -1:, :]
        dv = dv - p[..., -1:, :].transpose(-1, -2) * g[..., -1:, :]
    res.update(dq=dq, dk=dk, dv=dv, dp=dp, ds=ds)
    return res


def outputs_of(case):
    return ("out",) if case.op == "decode" else ("w", "out", "dq", "dk", "dv")


def bound(case, inp, ref):
    """The bounds of the module docstring, one tensor per output of the case."""
    q, k, v, g = (inp[n].double().abs() for n in ("q", "k", "v", "g"))
    B, H, Lq, Lk, D, sc, u = case.B, case.H, case.Lq, case.Lk, case.D, case.scale, case.u
    if Lk == 0 or B == 0:
        return {n: torch.zeros_like(ref[n]) for n in outputs_of(case)}
    p = ref["p"]
    sigma = D * FP * sc * (q @ k.transpose(-1, -2)).max(-1, keepdim=True).values  # [B, H, Lq, 1]
    e = (0.0 if case.op == "decode" else u) + 2 * sigma + (Lk + 8) * FP
    bnd = {"w": e * p + case.tiny, "out": (e + Lk * FP) * (p @ v) + u * ref["out"].abs()}
    if not case.has_bwd:
        return {"out": bnd["out"]}
    dp, ds = ref["dp"].abs(), ref["ds"].abs()
    a = g @ v.transpose(-1, -2)
    bnd["dv"] = ((e + Lq * FP) * p).transpose(-1, -2) @ g + u * ref["dv"].abs()
    E = (e + u) * ds + p * (e + Lk * FP) * (p * dp).sum(-1, keepdim=True) + p * D * FP * (a + (p * a).sum(-1, keepdim=True))
    bnd["dq"] = sc * (E @ k + Lk * FP * ds @ k) + u * ref["dq"].abs()
    bnd["dk"] = sc * (E.transpose(-1, -2) @ q + Lq * FP * ds.transpose(-1, -2) @ q) + u * ref["dk"].abs()
    return bnd


def compare(out, ref, bnd):
    """(all elements inside the bound, worst err / bound). A NaN is outside."""
    err = (out.double() - ref).abs()
    ok = bool((err <= bnd).all())
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    ratio = torch.where(torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
    return ok, float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------ routing
def parse_log(lines):
    """The attn records of a log (the general path's GEMM lines are skipped)."""
    return [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines if ln.split()[:1] == ["attn"]]


def _rec(op, kernel, c, n=None):
    r = dict(op=op, kernel=kernel, dtype=c.dname, b=str(c.B), h=str(c.H), lq=str(c.Lq), lk=str(c.Lk), d=str(c.D))
    if n is not None:
        r["n"] = str(n)
    return r


def expected_log(case):
    """The attn records one run of the case (forward, then backward) writes."""
    if case.status:
        return []
    if case.op == "decode":
        return [_rec("decode", case.fwd, case)]
    if case.op == "attn":
        return [_rec("fwd", case.fwd, case), _rec("bwd", case.bwd, case)]
    subs = subcases(case)
    live = [s for s in subs if s.B > 0]
    out = []
    for op, sub_op, which in (("views_fwd", "fwd", 0), ("views_bwd", "bwd", 1)):
        if case.fwd == "views_grouped":
            top = dataclasses.replace(live[0], Lk=max(s.Lk for s in live))
            out.append(_rec(op, "views_grouped", top, n=len(live)))
        else:
            out.append(_rec(op, "per_view", subs[0], n=len(subs)))
            out += [_rec(sub_op, case.per_view[i][which], s) for i, s in enumerate(subs) if s.B > 0]
    return out


def route_errors(case, lines):
    got, want = parse_log(lines), expected_log(case)
    return [] if got == want else [f"logged {got}, expected {want}"]


# ------------------------------------------------------------ GPU execution
def _rows(t):
    """[B, H, L, D] -> the kernel's [B L, H D] rows."""
    B, H, L, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * D)


def _unrows(t, B, H, L, D):
    return t.reshape(B, L, H, D).permute(0, 2, 1, 3)


def _flat(rows, cols, ld, dtype):
    """A flat buffer of SLACK + (rows + GUARD_ROWS) x ld sentinel elements."""
    assert ld >= cols
    return torch.full((SLACK + (rows + GUARD_ROWS) * ld,), SENTINEL, dtype=dtype)


def _put(buf, off, logical, ld):
    rows, cols = logical.shape
    buf[off:off + (rows + GUARD_ROWS) * ld].view(rows + GUARD_ROWS, ld)[:rows, :cols] = logical
    return buf


def unpack(buf, off, rows, cols, ld):
    """(the logical [rows, cols] block of a flat buffer, whether everything else still holds the sentinel)."""
    body = buf[off:off + (rows + GUARD_ROWS) * ld].view(rows + GUARD_ROWS, ld)
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    rest[off:off + (rows + GUARD_ROWS) * ld].view(rows + GUARD_ROWS, ld)[:rows, :cols] = False
    sent = torch.tensor(SENTINEL, dtype=buf.dtype)
    return body[:rows, :cols], bool((buf[rest] == sent).all())


def geometry(case):
    """name -> (rows, cols, ld, offset) of every buffer of a single problem."""
    B, H, Lq, Lk, D = max(case.B, 0), case.H, case.Lq, case.Lk, case.D
    ldq, ldk, ldv, ldo = case.lds
    off = lambda n: 1 if n in case.mis else 0  # noqa: E731
    geo = {"q": (B * Lq, H * D, ldq), "k": (B * Lk, H * D, ldk), "v": (B * Lk, H * D, ldv), "g": (B * Lq, H * D, ldo),
           "out": (B * Lq, H * D, ldo), "w": (B * H * Lq, case.ldw_, case.ldw_), "dq": (B * Lq, H * D, ldq),
           "dk": (B * Lk, H * D, ldk), "dv": (B * Lk, H * D, ldv)}
    return {n: (*t, off("o" if n == "out" else n)) for n, t in geo.items()}


def _desc(L, case, strides):
    d = L.AttnDesc()
    d.b, d.h, d.lq, d.lk, d.d = case.B, case.H, case.Lq, case.Lk, case.D
    d.dtype = L.BF16 if case.dtype == BF16 else L.F32
    d.ldq, d.ldk, d.ldv, d.ldo = case.lds
    d.ldw, d.scale = case.ldw_, case.scale
    d.m_sb, d.m_sh, d.m_si, d.m_sj = strides
    return d


class _Problem:
    """Device buffers of one single problem."""

    def __init__(self, L, case, dev):
        inp = inputs(case) if case.B > 0 else None
        self.case, self.geo = case, geometry(case)
        self.buf, esz = {}, torch.tensor([], dtype=case.dtype).element_size()
        for n, (rows, cols, ld, off) in self.geo.items():
            b = _flat(rows, cols, ld, case.dtype)
            if n in ("q", "k", "v", "g") and inp is not None:
                _put(b, off, _rows(inp[n]), ld)
            self.buf[n] = b.to(dev)
        self.ptr = {n: self.buf[n].data_ptr() + self.geo[n][3] * esz for n in self.buf}
        self.mask = inp["mask_t"].to(dev) if inp is not None and inp["mask_t"] is not None else None
        self.desc = _desc(L, case, inp["mask_strides"] if inp is not None else (0, 0, 0, 0))
        self.ws = torch.zeros(int(L.lib.fpnmt_attention_ws_bytes(self.desc)) + 256, dtype=torch.uint8, device=dev)

    def result(self):
        return {n: self.buf[n].cpu() for n in ("out", "w", "dq", "dk", "dv")}


def _table(ps, n):
    import ctypes
    return (ctypes.c_void_p * len(ps))(*[p.ptr[n] for p in ps])


def _run_decode(L, case, dev):
    inp = inputs(case)
    R, H, D, Lk, dt = case.B, case.H, case.D, case.Lk, case.dtype
    ldq, _, _, ldo = case.lds
    P = max(Lk, 1)
    pos_stride, k_off, v_off = 2 * H * D + 16, 8, 8 + H * D  # K and V interleaved in one position row
    row_stride = P * pos_stride + 8
    kv = torch.full((R * row_stride + SLACK,), SENTINEL, dtype=dt)
    body = kv[:R * row_stride].view(R, row_stride)[:, :P * pos_stride].view(R, P, pos_stride)
    body[:, :, k_off:k_off + H * D] = inp["kc"].reshape(R, P, H * D)
    body[:, :, v_off:v_off + H * D] = inp["vc"].reshape(R, P, H * D)
    qb = _put(_flat(R, H * D, ldq, dt), 0, _rows(inp["q"]), ldq).to(dev)
    ob = _flat(R, H * D, ldo, dt).to(dev)
    kv = kv.to(dev)
    src = inp["src"].to(dev) if case.src else None
    st = L.lib.fpnmt_decode_attention(L.BF16 if dt == BF16 else L.F32, R, H, D, Lk, case.scale, qb.data_ptr(), ldq,
                                      kv.data_ptr(), row_stride, pos_stride, k_off, v_off, L.ptr(src),
                                      Lk + 3 if case.src else 0, case.row_div, ob.data_ptr(), ldo, L.stream_ptr())
    L.check(st, "fpnmt_decode_attention")
    torch.cuda.synchronize()
    return {"status": st, "bufs": [{"out": ob.cpu()}]}


def run_gpu(case, dev="cuda"):
    """One forward and one backward of the case through the C entry points;
    returns the status and, per single problem, every output buffer whole
    (padding and guard rows included) on the host."""
    from fpnmt import _lib as L
    if case.op == "decode":
        return _run_decode(L, case, dev)
    s = L.stream_ptr()
    ps = [_Problem(L, c, dev) for c in subcases(case)]
    if case.op == "attn":
        p = ps[0]
        L.call("fpnmt_attention_fwd", p.desc, p.ptr["q"], p.ptr["k"], p.ptr["v"], L.ptr(p.mask), p.ptr["out"], p.ptr["w"],
               p.ws.data_ptr(), s)
        L.call("fpnmt_attention_bwd", p.desc, p.ptr["q"], p.ptr["k"], p.ptr["v"], p.ptr["w"], p.ptr["g"], p.ptr["dq"],
               p.ptr["dk"], p.ptr["dv"], p.ws.data_ptr(), s)
        st = 0
    else:
        import ctypes
        n = len(ps)
        descs = (L.AttnDesc * n)(*[p.desc for p in ps])
        wss = (ctypes.c_void_p * n)(*[p.ws.data_ptr() for p in ps])
        st = L.lib.fpnmt_attention_fwd_views(n, descs, _table(ps, "q"), _table(ps, "k"), _table(ps, "v"), None,
                                             _table(ps, "out"), _table(ps, "w"), wss, s)
        st2 = L.lib.fpnmt_attention_bwd_views(n, descs, _table(ps, "q"), _table(ps, "k"), _table(ps, "v"),
                                              _table(ps, "w"), _table(ps, "g"), _table(ps, "dq"), _table(ps, "dk"),
                                              _table(ps, "dv"), wss, s)
        if (st, st2) != (case.status, case.status):
            raise RuntimeError(f"{case.name}: views status {st} / {st2}, expected {case.status}: "
                               f"{L.lib.fpnmt_last_error().decode(errors='replace')}")
    torch.cuda.synchronize()
    return {"status": st, "bufs": [p.result() for p in ps]}


def check_problem(case, bufs):
    """One single problem's host buffers against reference, bound and the exact
    checks. Returns (list of failures, {output: worst err / bound})."""
    bad, ratios = [], {}
    geo = geometry(case)
    B, H, Lq, Lk, D = max(case.B, 0), case.H, case.Lq, case.Lk, case.D
    if case.op == "decode":
        geo = {"out": (B, H * D, case.lds[3], 0)}
    got = {}
    for n, buf in bufs.items():
        rows, cols, ld, off = geo[n]
        if buf.dtype != case.dtype or buf.numel() != SLACK + (rows + GUARD_ROWS) * ld:
            bad.append(f"{n}: buffer {buf.dtype} x {buf.numel()}")
            continue
        got[n], clean = unpack(buf, off, rows, cols, ld)
        if not clean:
            bad.append(f"{n}: padding columns or guard rows written")
    if bad or B == 0:
        return bad, ratios
    inp = inputs(case)
    ref = compute(case, inp)
    bnd = bound(case, inp, ref)
    for n in outputs_of(case):
        if n == "w":
            w = got["w"].reshape(B, H, Lq, case.ldw_)
            if not bool((w[..., Lk:].contiguous().view(torch.int16 if case.dtype == BF16 else torch.int32) == 0).all()):
                bad.append("w: columns from Lk to ldw are not bitwise zero")
            val = w[..., :Lk]
            masked = val[inp["mask"] > 0].contiguous()
            if masked.numel() and not bool((masked.view(torch.int16 if case.dtype == BF16 else torch.int32) == 0).all()):
                bad.append("w: masked weights are not bitwise zero")
        else:
            val = _unrows(got[n], B, H, Lk if n in ("dk", "dv") else Lq, D)
        ok, ratios[n] = compare(val, ref[n], bnd[n])
        if not ok:
            bad.append(f"{n}: elements outside the bound, worst err / bound {ratios[n]:.3f}")
    return bad, ratios


def check_case(case, res):
    """The numeric and exact checks of a whole case on a child's result."""
    bad, ratios = [], {}
    if res["status"] != case.status:
        bad.append(f"status {res['status']}, expected {case.status}")
    subs = subcases(case)
    if len(res["bufs"]) != len(subs):
        return bad + [f"{len(res['bufs'])} problems, expected {len(subs)}"], ratios
    for sub, bufs in zip(subs, res["bufs"]):
        if case.status:  # a refused call writes nothing at all
            sent = torch.tensor(SENTINEL, dtype=case.dtype)
            bad += [f"{sub.name}.{n}: written by a refused call" for n, b in bufs.items() if not bool((b == sent).all())]
            continue
        b, r = check_problem(sub, bufs)
        bad += [f"{sub.name}: {x}" for x in b]
        for n, v in r.items():
            ratios[n] = max(ratios.get(n, 0.0), v)
    if not res["same"]:
        bad.append("two runs differ bitwise")
    return bad, ratios


def child_main(outdir):
    """Run every case twice in this process (FPNMT_GEMM_LOG set by the parent);
    save the first run's buffers, whether the second equals it bit for bit, and
    the log lines of each run. Any error (a failed call, a HIP error at the
    synchronize) ends the process at once with a non-zero status."""
    log = os.environ["FPNMT_GEMM_LOG"]
    torch.cuda.set_device(0)
    res = {}

    def n_lines():
        try:
            with open(log) as f:
                return f.read().splitlines()
        except FileNotFoundError:
            return []

    for case in CASES:
        runs, lines = [], []
        for _ in range(2):
            before = len(n_lines())
            runs.append(run_gpu(case))
            lines.append(n_lines()[before:])
        same = all(torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8))
                   for a, b in zip(runs[0]["bufs"], runs[1]["bufs"]) for n in a)
        res[case.name] = {"bufs": runs[0]["bufs"], "status": runs[0]["status"], "same": same, "log": lines}
        print(case.name, [ln for ln in lines[0] if ln.startswith("attn")], flush=True)
    torch.save(res, os.path.join(outdir, "results.pt"))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "fpn-mt-image-captioning_amd"))
    child_main(sys.argv[1])

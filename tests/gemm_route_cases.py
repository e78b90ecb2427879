"""Case table of the bf16 GEMM / conv dispatch routes (csrc/gemm_dispatch.h).

One entry per route: the smallest ragged shape that reaches it, the code the
route writes into the `cfg=` field of FPNMT_GEMM_LOG, and (split and
weight-gradient routes) the split count / tile grid. Helper module, not
collected: tests/test_gemm_route_bars.py (no GPU) proves on planted errors that
the bound below can fail, tests/test_gpu_gemm_routes.py runs every case on the
GPU in one child process and checks route, numerics, padding, repeatability.

Every case is a GEMM  out[M, N] = epilogue(A[M, K] @ B[K, N])  in the kernel's
own K order (im2col: (r, s, c), c fastest; weight gradients: K = pixels):

  * inputs: magnitudes in [0.5, 1] with random signs, rounded to bf16, seeded;
  * reference: fp64 on the CPU from the bf16-rounded operands (matmul,
    F.conv2d / conv_transpose2d, autograd of F.conv2d for the weight gradient),
    the epilogue applied in fp64;
  * bound: products of two bf16 values are exact in fp32, so with
    S = sum_k |a_k b_k| (+ |bias|, |R|, |old C|, scaled like the sum) any fp32
    summation order over any split is within (K - 1) 2^-24 S; the bound is
    K 2^-23 S (twice that and the epilogue's few extra roundings: MFMA's
    internal add order and rounding are not documented) plus the output
    rounding, 2^-23 |ref| for fp32 C and 2^-8 |ref| for bf16 C (the term of
    test_conv3x3_same_bf16; it covers a bf16 read-modify-write too).

Edges every case carries unless its entry point forbids one (said in `note`):
ragged M (odd partial last tile), an N tail (N = 8 mod the tile width on the
LDS-DMA routes: one live 8-column group; odd N elsewhere), the fewest K-tiles
the route admits (split routes: a K-tile count the split count does not
divide; weight gradients: an odd K), lda = K + 8, ldc = N + 8 with C
pre-filled with a sentinel and two guard rows after row M - 1. The conv entry
points take dense NHWC tensors only (no leading dimensions): there the guard
rows follow the dense output, and the reroute of tall rows needs lda = K.
The LDS-DMA weight-gradient tiles need M % 8 == 0 (16-B chunks along m), so
their ragged last tile has 8 or 72 live rows instead of an odd count, and the
256x128 conv tile needs c % 256 == 0 at 3x3, which makes M = 9 c whole tiles.
"""
from __future__ import annotations

import dataclasses
import math
import os
import sys

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = -12352.0  # exact in bf16; no output of these cases comes near it
GUARD_ROWS = 2
LEAKY = 0.2

# FPNMT_GEMM_LOG's a= / c= fields
A_ROW, A_COL, A_IM2COL, A_IM2COL_T = 0, 1, 2, 3
C_ROW, C_SCATTER = 0, 1

# weight-gradient tile forms of launch_pipe_wg: name -> (BM, BN, a= field or None)
WG_TILES = {
    "128x64": (128, 64, None),
    "64x256": (64, 256, None),
    "128x256+8lw": (128, 256, A_IM2COL_T),
    "256x128": (256, 128, None),
    "128x128+4lw": (128, 128, A_COL),
    "128x128": (128, 128, A_IM2COL_T),
}


def cdiv(a, b):
    return -(-a // b)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str  # gemm | wgrad_job | fwd | bwd_data | bwd_filter
    cfg: int  # expected cfg= code of the case's one log line
    # gemm kinds: C[m, n] = A[m, k] B[k, n]; ta / tb as fpnmt_gemm_desc a_trans / b_trans
    m: int = 0
    n: int = 0
    k: int = 0
    ta: int = 0
    tb: int = 0
    pad_lda: bool = True  # lda = K + 8 (A_ROW) / M + 8 (A_COL)
    # conv kinds: input levels (n, h, w) (more than one: the grouped entry point),
    # c input channels, ko filters, r x r taps, 'same' padding, stride
    levels: tuple = ()
    c: int = 0
    ko: int = 0
    r: int = 1
    stride: int = 1
    # epilogue
    bias: bool = False
    res: bool = False
    leaky: bool = False
    alpha: float = 1.0
    col_scale: bool = False
    mask: bool = False  # the M2 operand: out *= relu'(y)
    acc: int = 0  # 1: C += into bf16 C, 2: the fp32 weight-gradient accumulation
    c_f32: bool = False
    wide: str = ""  # fpnmt_set_wide_cfg for the case ("" = 0, automatic)
    # expected route details
    cmode: int = C_ROW
    psplit: int | None = None  # log psplit= (pipe routes; 1 = unsplit)
    split: int | None = None  # log split=
    ksplit: int = 0  # K elements per split (the last split is shorter)
    tile: str = ""  # WG_TILES key (cfg 110)
    seed: int = 0
    data: str = ""  # cases with the same key share inputs and reference
    note: str = ""

    @property
    def conv(self):
        return self.kind in ("fwd", "bwd_data", "bwd_filter")

    @property
    def pad(self):
        return (self.r - 1) // 2

    def out_hw(self, h, w):
        p, r, s = self.pad, self.r, self.stride
        return (h + 2 * p - r) // s + 1, (w + 2 * p - r) // s + 1

    @property
    def dims(self):
        """(M, N, K) of the GEMM the dispatch sees."""
        if not self.conv:
            return self.m, self.n, self.k
        if self.kind == "fwd":
            return sum(n * math.prod(self.out_hw(h, w)) for n, h, w in self.levels), self.ko, self.r * self.r * self.c
        if self.kind == "bwd_data":
            if self.stride == 1:
                return sum(n * h * w for n, h, w in self.levels), self.c, self.r * self.r * self.ko
            return sum(n * math.prod(self.out_hw(h, w)) for n, h, w in self.levels), self.c, self.ko
        return self.r * self.r * self.c, self.ko, sum(n * math.prod(self.out_hw(h, w)) for n, h, w in self.levels)

    @property
    def out_dtype(self):
        return F32 if self.c_f32 else BF16

    @property
    def ldc(self):
        return self.dims[1] + (0 if self.conv else 8)

    @property
    def splits(self):
        s = self.psplit if (self.psplit or 1) > 1 else self.split
        return s if s and s > 1 and self.ksplit else 1


def _g(name, cfg, m, n, k, **kw):
    return Case(name, kw.pop("kind", "gemm"), cfg, m=m, n=n, k=k, **kw)


def _c(name, kind, cfg, levels, c, ko, r, **kw):
    if isinstance(levels[0], int):
        levels = (levels,)
    return Case(name, kind, cfg, levels=tuple(levels), c=c, ko=ko, r=r, **kw)


_WG = dict(ta=1, tb=1, acc=2, c_f32=True)
_WGC = dict(acc=2, c_f32=True)
_TALL = dict(pad_lda=False, note="rows_via_im2col needs lda == K")
_CONV = "dense NHWC operands: no padded leading dimensions"

# Final table (256 CUs; every route confirmed from the log on the GPU).
CASES = [
    # ---- row-major Dense on the LDS-DMA pipe (cfg 130 + c) ----------------
    _g("row_cfg9", 139, 257, 264, 256, seed=1, psplit=1),
    _g("row_cfg9_epi", 139, 257, 264, 256, psplit=1, bias=True, res=True, leaky=True,
       note="bias + residual + leaky-ReLU 0.2 on a direct epilogue"),
    _g("row_cfg9_alpha", 139, 257, 264, 256, psplit=1, alpha=0.5, note="alpha != 1 on a direct epilogue"),
    _g("row_cfg9_acc", 139, 257, 264, 256, psplit=1, acc=1, note="accumulate = 1 into bf16 C, direct epilogue"),
    _g("row_cfg9_psplit2", 139, 257, 264, 1088, psplit=2, ksplit=576, note="17 K-tiles over 2 slabs"),
    _g("row_cfg5", 135, 257, 1032, 256, psplit=1),
    _g("row_cfg8", 138, 257, 1544, 256, seed=1, psplit=1),
    _g("row_cfg8_vocab", 138, 992, 2008, 512, psplit=1, note="the C2 vocabulary projection, N scaled down"),
    _g("row_cfg3", 133, 4101, 776, 512, psplit=1),
    # ---- tall rows rerouted as a 1x1 implicit GEMM (cfg 170 + c) ----------
    _g("tall_cfg0_epi", 170, 4097, 264, 256, psplit=1, bias=True, res=True, leaky=True, **_TALL),
    _g("tall_cfg0_alpha", 170, 4097, 264, 256, psplit=1, res=True, alpha=0.5, **_TALL),
    _g("tall_cfg0_acc", 170, 4097, 264, 256, psplit=1, res=True, acc=1, **_TALL),
    _g("tall_cfg1", 171, 4097, 264, 256, psplit=1, **_TALL),
    _g("tall_cfg8", 178, 4097, 264, 512, psplit=1, **_TALL),
    _g("tall_cfg2", 172, 6529, 264, 512, psplit=1, **_TALL),
    _g("tall_cfg11", 181, 6529, 264, 2048, seed=1, psplit=1, data="tall_2048", **_TALL),
    _g("tall_cfg7", 177, 6529, 264, 2048, seed=1, psplit=1, wide="6", data="tall_2048", **_TALL),
    # ---- register-staged tiles, the small and the skinny kernel -----------
    _g("reg128x64k_split8", 0, 513, 257, 4168, split=8, ksplit=576, note="ws_split_for: 66 K-tiles over 8 slabs"),
    _g("reg128x32k", 3, 3073, 2049, 264, split=1),
    _g("reg64x32k_bkn", 1, 129, 72, 72, tb=1, split=1),
    _g("reg64x32k_bkn_odd_n", 1, 129, 65, 72, tb=1, split=1, note="odd N: the scalar loaders"),
    _g("reg64x64k", 2, 129, 65, 1032, tb=1, split=1),
    _g("reg64x64k_split3", 2, 129, 65, 1544, tb=1, split=3, ksplit=576, note="ws_split_for: 25 K-tiles over 3 slabs"),
    _g("reg32", 4, 31, 31, 40, split=1),
    _g("small", 5, 33, 65, 72, split=1),
    _g("small_split2", 5, 33, 65, 1032, split=2, ksplit=528),
    _g("skinny", 5, 31, 65, 72, split=1, note="M <= 32: gemm_skinny_kernel (logged as the small class)"),
    _g("wgrad_reg_slabs", 2, 40, 41, 1125, split=9, ksplit=128,
       note="register-staged slabs + wgrad_reduce_kernel<16>", **_WG),
    # ---- Dense weight gradients: the LDS-DMA tiles (cfg 110), the job queue
    _g("wg_col_128x128lw", 110, 136, 136, 2049, tile="128x128+4lw", split=9, ksplit=256,
       note="wgrad_reduce_kernel<16>", **_WG),
    _g("wg_col_128x64", 110, 136, 72, 1125, tile="128x64", split=5, ksplit=256, note="wgrad_reduce_kernel<4>", **_WG),
    _g("wg_col_64x256", 110, 72, 264, 1125, tile="64x256", split=5, ksplit=256, **_WG),
    _g("wg_col_256x128", 110, 4104, 136, 1125, seed=1, tile="256x128", split=5, ksplit=256,
       note="wgrad_reduce_kernel<1> (>= 65536 items)", **_WG),
    _g("wg_jobs", 150, 136, 136, 1125, kind="wgrad_job", note="fpnmt_gemm_wgrad inside a deferred region", **_WG),
    # ---- implicit-GEMM conv forward (cfg 130 + c) -------------------------
    _c("im2col_cfg1", "fwd", 131, (3, 9, 9), 64, 72, 1, psplit=1, note=_CONV),
    _c("im2col_cfg8", "fwd", 138, (3, 9, 9), 64, 72, 3, psplit=1, note=_CONV),
    _c("im2col_cfg8_psplit2", "fwd", 138, (3, 9, 9), 128, 72, 3, psplit=2, ksplit=576, note=_CONV),
    _c("im2col_cfg8_psplit8", "fwd", 138, (3, 9, 9), 576, 72, 3, psplit=8, ksplit=704,
       note="81 K-tiles over 8 slabs; " + _CONV),
    _c("im2col_cfg0", "fwd", 130, (3, 9, 9), 256, 72, 1, psplit=1, res=True, note=_CONV),
    _c("im2col_cfg0_epi", "fwd", 130, (3, 9, 9), 256, 72, 1, psplit=1, bias=True, res=True, leaky=True,
       note="bias + residual + leaky-ReLU 0.2 on the staged epilogue; " + _CONV),
    _c("im2col_cfg2", "fwd", 132, (3, 61, 61), 64, 136, 3, psplit=1, note=_CONV),
    _c("im2col_cfg11", "fwd", 141, (1, 83, 83), 256, 264, 3, seed=1, psplit=1, data="im2col_2304", note=_CONV),
    _c("im2col_cfg7", "fwd", 137, (1, 83, 83), 256, 264, 3, seed=1, psplit=1, wide="6", data="im2col_2304", note=_CONV),
    _c("im2col_cfg10", "fwd", 140, (5, 51, 49), 128, 264, 3, psplit=1, wide="10", data="im2col_1152", note=_CONV),
    _c("im2col_cfg6", "fwd", 136, (5, 51, 49), 128, 264, 3, psplit=1, wide="6", data="im2col_1152", note=_CONV),
    _c("im2col_grouped", "fwd", 138, ((3, 9, 9), (1, 5, 5), (1, 1, 1)), 64, 72, 3, psplit=1,
       note="grouped: one group under a tile, one with M = 1; " + _CONV),
    _c("im2col_grouped_bwd", "bwd_data", 138, ((3, 9, 9), (1, 5, 5), (1, 1, 1)), 72, 64, 3, psplit=1,
       note="grouped bwd-data; " + _CONV),
    _c("im2col_grouped_bwd_mask", "bwd_data", 138, ((3, 9, 9), (1, 5, 5), (1, 1, 1)), 72, 64, 3, seed=2, psplit=1,
       mask=True,
       note="grouped bwd-data with the per-level act mask (the R operand with r_mask); " + _CONV),
    # ---- the M2 mask (bwd-data): pipe epilogues and mask_rows_kernel -------
    _c("m2_direct", "bwd_data", 138, (3, 9, 9), 72, 64, 3, psplit=1, mask=True, note=_CONV),
    _c("m2_staged", "bwd_data", 130, (3, 9, 9), 72, 256, 1, seed=5, psplit=1, res=True, mask=True, note=_CONV),
    _c("m2_mask_rows", "bwd_data", 138, (3, 9, 9), 72, 128, 3, seed=2, psplit=2, ksplit=576, mask=True,
       note="pipe split: the mask by mask_rows_kernel; " + _CONV),
    # ---- strided 1x1 bwd-data rerouted to the pipe (cfg 160 + c) ----------
    _c("scatter_cfg1", "bwd_data", 161, (3, 17, 17), 72, 64, 1, stride=2, cmode=C_SCATTER, psplit=1, note=_CONV),
    _c("scatter_cfg1_m2", "bwd_data", 161, (3, 17, 17), 72, 64, 1, stride=2, cmode=C_SCATTER, seed=2, psplit=1,
       mask=True,
       note="M2 at the scattered rows; " + _CONV),
    _c("scatter_cfg8", "bwd_data", 168, (3, 17, 17), 72, 512, 1, stride=2, cmode=C_SCATTER, psplit=1, note=_CONV),
    _c("scatter_cfg2", "bwd_data", 162, (3, 121, 121), 136, 512, 1, stride=2, cmode=C_SCATTER, psplit=1, note=_CONV),
    _c("scatter_cfg10", "bwd_data", 170, (3, 129, 129), 264, 1024, 1, stride=2, cmode=C_SCATTER, psplit=1,
       wide="10", data="scatter_1024", note=_CONV),
    _c("scatter_cfg6", "bwd_data", 166, (3, 129, 129), 264, 1024, 1, stride=2, cmode=C_SCATTER, psplit=1,
       wide="6", data="scatter_1024", note=_CONV),
    _c("scatter_cfg11", "bwd_data", 171, (1, 165, 165), 264, 2048, 1, stride=2, cmode=C_SCATTER, psplit=1,
       data="scatter_2048", note=_CONV),
    _c("scatter_cfg7", "bwd_data", 167, (1, 165, 165), 264, 2048, 1, stride=2, cmode=C_SCATTER, psplit=1,
       wide="6", data="scatter_2048", note=_CONV),
    # ---- conv weight gradients: the LDS-DMA tiles (cfg 110) ---------------
    _c("wg_conv_128x256lw", "bwd_filter", 110, (5, 15, 15), 136, 520, 3, tile="128x256+8lw", split=5, ksplit=256,
       note="wgrad_reduce_kernel<1>; " + _CONV, **_WGC),
    _c("wg_conv_128x128", "bwd_filter", 110, (5, 15, 15), 136, 136, 3, tile="128x128", split=5, ksplit=256,
       note="wgrad_reduce_kernel<4>; " + _CONV, **_WGC),
    _c("wg_conv_256x128", "bwd_filter", 110, (5, 15, 15), 512, 136, 3, tile="256x128", split=5, ksplit=256,
       note="this tile needs c % 256 == 0 at 3x3, so M = 9 c is whole tiles; " + _CONV, **_WGC),
    _c("wg_conv_128x64", "bwd_filter", 110, (5, 15, 15), 136, 72, 3, tile="128x64", split=5, ksplit=256,
       note=_CONV, **_WGC),
    _c("wg_conv_64x256", "bwd_filter", 110, (5, 15, 15), 72, 264, 1, tile="64x256", split=5, ksplit=256,
       col_scale=True, note="M = 72 < 128; with col_scale; " + _CONV, **_WGC),
    _c("wg_conv_grouped", "bwd_filter", 110, ((5, 15, 15), (1, 5, 5), (1, 1, 1)), 136, 136, 3, tile="128x128",
       split=5, ksplit=256, note="k-grouped: the levels' K-tiles end to end; " + _CONV, **_WGC),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# (cfg code, c= field) pairs dispatch_gemm_impl<bf16> can log. 160 + 10 / 11
# (scatter reroute on cfg 10 / 11) print the same number as 170 + 0 / 1 (tall
# rows on cfg 0 / 1): the c= field tells them apart.
REACHABLE = (
    {(c, C_ROW) for c in (0, 1, 2, 3, 4, 5, 110, 150)}
    | {(130 + c, C_ROW) for c in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11)}
    | {(160 + c, C_SCATTER) for c in (1, 2, 6, 7, 8, 10, 11)}
    | {(170 + c, C_ROW) for c in (0, 1, 2, 7, 8, 11)}
)
# Codes the arithmetic of the dispatch rules excludes:
#   134       launch_pipe_cfg case 4: no dispatch rule returns 4 (pipe_cfg gives
#             0 1 2 6 7 8 10 11, row_short_cfg 5 8 9, tall A_ROW 3); the
#             library does not instantiate it (pipe_cfg_built: only the pairs
#             a rule returns are compiled, anything else is FPNMT_E_UNSUPPORTED);
#             tools/fwd_bench.hip builds it for its "split cfg4" variants
#   160       cfg 0 needs a residual operand, which scatter_reroute refuses
#   163-165, 169, 173-175, 179: cfg 3 / 5 / 9 are A_ROW-only, 4 as above
#   176, 180  the wide class needs >= 192 tiles of 128x256 at K >= 1024, and
#             the A_ROW pipe class (cfg 3) takes every such GEMM first
UNREACHABLE = {134, 160, 163, 164, 165, 169, 173, 174, 175, 176, 179, 180}


# ------------------------------------------------------------------ inputs
def _rnd(g, *shape, dtype=BF16):
    mag = torch.rand(*shape, generator=g) * 0.5 + 0.5
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn).to(dtype)


def _seed_of(case):
    key = case.data or case.name
    return sum((i + 1) * b for i, b in enumerate(key.encode())) * 7919 + case.seed


_CACHE = {}


def _cached(kind, case, make):
    """make(case) cached per data key; the few last keys only (the tests walk
    the table in order, cases of one key are neighbours)."""
    key = (kind, case.data or case.name, case.seed)
    if key not in _CACHE:
        while len(_CACHE) >= 6:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make(case)
    return _CACHE[key]


def _operands(case):
    """The two bf16 operands (shared by the cases of one data key)."""
    g = torch.Generator().manual_seed(_seed_of(case))
    M, N, K = case.dims
    if not case.conv:
        lda = (M if case.ta else K) + (8 if case.pad_lda else 0)
        ldb = (N if case.tb else K) + 8
        A = _rnd(g, K if case.ta else M, lda)
        B = _rnd(g, K if case.tb else N, ldb)
        return {"A": A, "B": B, "lda": lda, "ldb": ldb}
    w = _rnd(g, case.r, case.r, case.c, case.ko)  # HWIO
    xs, dzs = [], []
    for n, h, wd in case.levels:
        ho, wo = case.out_hw(h, wd)
        if case.kind != "bwd_data":
            xs.append(_rnd(g, n, h, wd, case.c))
        if case.kind != "fwd":
            dzs.append(_rnd(g, n, ho, wo, case.ko))
    return {"w": w, "xs": xs, "dzs": dzs}


def inputs(case):
    """Seeded CPU inputs: the operands and the epilogue tensors."""
    inp = dict(_cached("operands", case, _operands))
    g = torch.Generator().manual_seed(_seed_of(case) + 1)
    M, N, K = case.dims
    rows = out_rows(case)
    if case.bias:
        inp["bias"] = _rnd(g, N, dtype=F32)
    if case.col_scale:
        inp["col_scale"] = _rnd(g, N, dtype=F32)
    if case.res:
        inp["R"] = _rnd(g, rows, case.ldc)  # conv: ldc == N
    if case.mask:
        inp["y"] = _rnd(g, rows, N)
    if case.acc:
        inp["old"] = _rnd(g, rows, N, dtype=case.out_dtype)
    return inp


# ---------------------------------------------------- logical GEMM of a case
def out_rows(case):
    """Rows of the output buffer (without guard rows)."""
    if case.kind != "bwd_filter" and len(case.levels) > 1:  # levels back to back, guard rows after each
        return case.dims[0] + GUARD_ROWS * (len(case.levels) - 1)
    if case.kind == "bwd_data":
        return sum(n * h * w for n, h, w in case.levels)
    return case.dims[0]


def _level_rows(case):
    """Output rows of each level (fwd: n ho wo; grouped bwd-data, stride 1: n h w)."""
    return [n * (math.prod(case.out_hw(h, w)) if case.kind == "fwd" else h * w) for n, h, w in case.levels]


def row_map(case):
    """Output-buffer row of every logical row (None: the identity)."""
    if case.kind == "bwd_data" and case.stride > 1:
        (n, h, w), s = case.levels[0], case.stride
        ho, wo = case.out_hw(h, w)
        i = torch.arange(n)[:, None, None]
        y = torch.arange(ho)[None, :, None]
        x = torch.arange(wo)[None, None, :]
        return ((i * h + y * s) * w + x * s).reshape(-1)
    if case.kind != "bwd_filter" and len(case.levels) > 1:
        rows, base = [], 0
        for m in _level_rows(case):
            rows.append(torch.arange(m) + base)
            base += m + GUARD_ROWS
        return torch.cat(rows)
    return None


def b_matrix(case, inp):
    """B[K, N] in fp64, in the kernel's K order."""
    M, N, K = case.dims
    if not case.conv:
        B = inp["B"].double()
        return B[:, :N] if case.tb else B[:, :K].t()
    w = inp["w"].double()
    if case.kind == "fwd":
        return w.permute(3, 0, 1, 2).reshape(N, K).t()  # w_ohwi rows
    if case.kind == "bwd_data":
        return w.flip(0, 1).permute(2, 0, 1, 3).reshape(N, K).t()  # w_flip rows
    return torch.cat([dz.double().reshape(-1, N) for dz in inp["dzs"]])


def a_rows(case, inp, rows):
    """Rows `rows` of A[M, K] in fp64 (im2col gathered for the conv kinds)."""
    M, N, K = case.dims
    if not case.conv:
        A = inp["A"].double()
        return A[:K, rows].t() if case.ta else A[rows, :K]
    p, r, s = case.pad, case.r, case.stride
    out = []
    if case.kind == "bwd_filter":
        xps = [F.pad(x.double(), (0, 0, p, p, p, p)) for x in inp["xs"]]
        for m in rows:
            tap, ch = divmod(int(m), case.c)
            rr, ss = divmod(tap, r)
            cols = []
            for xp, (n, h, w) in zip(xps, case.levels):
                ho, wo = case.out_hw(h, w)
                cols.append(xp[:, rr:rr + (ho - 1) * s + 1:s, ss:ss + (wo - 1) * s + 1:s, ch].reshape(-1))
            out.append(torch.cat(cols))
        return torch.stack(out)
    src = inp["xs"] if case.kind == "fwd" else inp["dzs"]
    if case.kind == "bwd_data" and s > 1:
        return src[0].double().reshape(M, K)[rows]
    q = p if case.kind == "fwd" else r - 1 - p
    bounds, base = [], 0
    for n, h, w in case.levels:
        ho, wo = case.out_hw(h, w) if case.kind == "fwd" else (h, w)
        bounds.append((base, n, ho, wo))
        base += n * ho * wo
    for m in rows:
        lv = max(i for i, b in enumerate(bounds) if b[0] <= int(m))
        b0, n, ho, wo = bounds[lv]
        img, rem = divmod(int(m) - b0, ho * wo)
        y, x = divmod(rem, wo)
        sp = F.pad(src[lv][img].double(), (0, 0, q, q, q, q))
        out.append(sp[y * s:y * s + r, x * s:x * s + r, :].reshape(-1))
    return torch.stack(out)


def _conv_lin(case, inp, absval):
    """A @ B of a conv kind in fp64 through torch's own convolution."""
    f = (lambda t: t.double().abs()) if absval else (lambda t: t.double())
    M, N, K = case.dims
    p, s = case.pad, case.stride
    w = f(inp["w"]).permute(3, 2, 0, 1).contiguous()  # OIHW
    if case.kind == "fwd":
        ys = [F.conv2d(f(x).permute(0, 3, 1, 2), w, stride=s, padding=p).permute(0, 2, 3, 1).reshape(-1, N)
              for x in inp["xs"]]
        return torch.cat(ys)
    if case.kind == "bwd_data" and len(case.levels) > 1:
        assert s == 1
        dxs = [F.conv_transpose2d(f(dz).permute(0, 3, 1, 2), w, padding=p).permute(0, 2, 3, 1).reshape(-1, N)
               for dz in inp["dzs"]]
        return torch.cat(dxs)
    if case.kind == "bwd_data":
        (n, h, wd), dz = case.levels[0], inp["dzs"][0]
        ho, wo = case.out_hw(h, wd)
        opad = (h - ((ho - 1) * s - 2 * p + case.r), wd - ((wo - 1) * s - 2 * p + case.r))
        dx = F.conv_transpose2d(f(dz).permute(0, 3, 1, 2), w, stride=s, padding=p, output_padding=opad)
        dx = dx.permute(0, 2, 3, 1).reshape(-1, N)
        rm = row_map(case)
        if rm is None:
            return dx
        rest = torch.ones(dx.shape[0], dtype=torch.bool)
        rest[rm] = False
        assert not dx[rest].any()  # rows the stride skips get nothing
        return dx[rm]
    tot = torch.zeros(M, N, dtype=F64)
    for x, dz in zip(inp["xs"], inp["dzs"]):
        w0 = torch.zeros(N, case.c, case.r, case.r, dtype=F64, requires_grad=True)
        y = F.conv2d(f(x).permute(0, 3, 1, 2), w0, stride=s, padding=p)
        (gw,) = torch.autograd.grad(y, w0, f(dz).permute(0, 3, 1, 2))
        tot += gw.permute(2, 3, 1, 0).reshape(M, N)  # HWIO rows (r, s, c)
    return tot


def linear_terms(case, inp):
    """(A @ B, |A| @ |B|) in fp64, both [M, N]."""
    if case.conv:
        return _conv_lin(case, inp, False), _conv_lin(case, inp, True)
    M = case.dims[0]
    A, B = a_rows(case, inp, slice(0, M)), b_matrix(case, inp)
    return A @ B, A.abs() @ B.abs()


def _logical(case, t):
    """A [rows, ld] epilogue tensor at the logical rows, N columns."""
    rm, N = row_map(case), case.dims[1]
    t = t.double()[:, :N]
    return t if rm is None else t[rm]


def epilogue(case, inp, lin, S):
    """fp64 epilogue of the logical product; returns (value, S with the addends)."""
    v, s = lin * case.alpha, S * abs(case.alpha)
    if case.col_scale:
        v, s = v * inp["col_scale"].double(), s * inp["col_scale"].double().abs()
    if case.bias:
        v, s = v + inp["bias"].double(), s + inp["bias"].double().abs()
    if case.res:
        v, s = v + _logical(case, inp["R"]), s + _logical(case, inp["R"]).abs()
    if case.leaky:
        v = torch.where(v > 0, v, LEAKY * v)
    if case.mask:
        mk = (_logical(case, inp["y"]) > 0).double()
        v, s = v * mk, s * mk
    if case.acc:
        v, s = v + _logical(case, inp["old"]), s + _logical(case, inp["old"]).abs()
    return v, s


def to_output(case, logical, gaps=None):
    """Logical [M, N] values at their rows of the [out_rows, N] output. The
    other rows: zero where a strided bwd-data skips them (the entry point
    zero-fills dx), the sentinel in the guard rows between grouped levels."""
    rm = row_map(case)
    if rm is None:
        return logical
    if gaps is None:
        gaps = SENTINEL if len(case.levels) > 1 else 0.0
    out = torch.full((out_rows(case), logical.shape[1]), gaps, dtype=logical.dtype)
    out[rm] = logical
    return out


def terms(case):
    """(A @ B, |A| @ |B|) of the case, shared by the cases of one data key."""
    return _cached("terms", case, lambda c: linear_terms(c, inputs(c)))


def reference(case, inp=None, lin=None, S=None):
    """(ref, S_total) in fp64 over the [out_rows, N] output (rows a strided
    bwd-data skips: exactly zero, bound zero; guard rows between grouped
    levels: the sentinel, bound zero)."""
    inp = inp or inputs(case)
    if lin is None:
        lin, S = terms(case)
    v, s = epilogue(case, inp, lin, S)
    return to_output(case, v), to_output(case, s, gaps=0.0)


def bound(case, ref, S):
    """K 2^-23 S + the output rounding (2^-23 |ref| fp32 C, 2^-8 |ref| bf16 C)."""
    K = case.dims[2]
    return K * 2.0 ** -23 * S + (2.0 ** -23 if case.c_f32 else 2.0 ** -8) * ref.abs()


def compare(case, out, ref, bnd):
    """(all elements inside the bound, worst err / bound). out: [rows, N]."""
    err = (out.double() - ref).abs()
    bad = err > bnd
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return not bool(bad.any()), float(ratio.max())


# ------------------------------------------------------------ planted errors
def plants(case, inp, lin):
    """(name, corrupted A @ B) pairs: the errors the bound must reject."""
    M, N, K = case.dims
    B = b_matrix(case, inp)
    last = a_rows(case, inp, [M - 1])[0]
    col = N - 1
    out = []
    k0 = 8 * (K // 16)
    p = lin.clone()
    p[M - 1, col] -= last[k0:k0 + 8] @ B[k0:k0 + 8, col]
    out.append(("k_chunk8", p))
    if K >= 128:
        k0 = 64 * (K // 128)
        p = lin.clone()
        p[M - 1, col] -= last[k0:k0 + 64] @ B[k0:k0 + 64, col]
        out.append(("k_tile64", p))
    if case.kind in ("fwd", "bwd_data"):
        # the centre tap (in range at every border) of the last pixel, a corner of the last image
        cc = K // (case.r * case.r)
        t0 = (case.r * case.r // 2) * cc
        p = lin.clone()
        p[M - 1] -= last[t0:t0 + cc] @ B[t0:t0 + cc]
        out.append(("tap", p))
    elif case.kind == "bwd_filter":
        # the centre tap x the last pixel of the first level (a corner): a rank-1
        # term of the tap's c rows (stride 1: the tap reads the pixel itself)
        assert case.stride == 1
        n, h, w = case.levels[0]
        pix = n * h * w - 1
        t0 = (case.r * case.r // 2) * case.c
        p = lin.clone()
        p[t0:t0 + case.c] -= torch.outer(inp["xs"][0].double().reshape(-1, case.c)[pix], B[pix])
        out.append(("tap", p))
    if M >= 2:
        p = lin.clone()
        p[M - 1] = p[M - 2]
        out.append(("row_swap", p))
    p = lin.clone()
    p[:, 8 * ((N - 1) // 8):] = 0
    out.append(("n_tail", p))
    if case.splits > 1:
        k0 = (case.splits - 1) * case.ksplit
        assert 0 < K - k0 <= case.ksplit, (case.name, K, k0)  # the last split (shorter wherever K allows)
        rows = list(range(max(0, M - 16), M))
        p = lin.clone()
        p[rows] -= a_rows(case, inp, rows)[:, k0:] @ B[k0:]
        out.append(("last_split", p))
    return out


# ------------------------------------------------------------------ routing
def parse_log(lines):
    """The GEMM launch lines (first word: the dtype); `conv` / `attn` lines are other launchers'."""
    return [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines if ln.strip() and ln.split()[0] in ("bf16", "f32")]


def route_errors(case, lines):
    """Mismatches between the log lines a case produced and its table entry."""
    M, N, K = case.dims
    recs = parse_log(lines)
    if len(recs) != 1:
        return [f"{len(recs)} log lines, expected 1: {lines}"]
    r, bad = recs[0], []

    def want(key, val, default=None):
        got = r.get(key, default)
        if got is None or int(got) != val:
            bad.append(f"{key}={got}, expected {val}")

    want("cfg", case.cfg)
    want("c", case.cmode)
    want("M", M), want("N", N), want("K", K)
    if case.psplit is not None:
        want("psplit", case.psplit)
    if case.split is not None:
        want("split", case.split)
    if case.tile:
        bm, bn, amode = WG_TILES[case.tile]
        want("tm", cdiv(M, bm)), want("tn", cdiv(N, bn))
        if amode is not None:
            want("a", amode)
        # no other tile form gives this shape the same grid
        same = [t for t, (m2, n2, _) in WG_TILES.items() if (m2, n2) != (bm, bn) and
                (cdiv(M, m2), cdiv(N, n2)) == (cdiv(M, bm), cdiv(N, bn))]
        if same:
            bad.append(f"tile grid does not tell {case.tile} from {same}")
    return bad


# ------------------------------------------------------------ GPU execution
def _buffer(case, inp, dev):
    rows, N, ldc = out_rows(case), case.dims[1], case.ldc
    buf = torch.full((rows + GUARD_ROWS, ldc), SENTINEL, dtype=case.out_dtype)
    if case.acc:
        buf[:rows, :N] = inp["old"]
    return buf.to(dev)


def run_gpu(case, inp, dev="cuda"):
    """One launch of the case through the C entry points; returns the whole
    output buffer (padding and guard rows included) on the device."""
    from fpnmt import _lib as L
    M, N, K = case.dims
    s = L.stream_ptr()
    C = _buffer(case, inp, dev)
    opt = {k: inp[k].to(dev) if k in inp else None for k in ("bias", "col_scale", "R", "y")}
    keep = [C, opt]
    if not case.conv:
        A, B = inp["A"].to(dev), inp["B"].to(dev)
        d = L.GemmDesc()
        d.m, d.n, d.k, d.batch, d.batch_inner, d.dtype = M, N, K, 1, 1, L.BF16
        d.a_trans, d.b_trans = case.ta, case.tb
        d.lda, d.ldb, d.ldc, d.ldr = inp["lda"], inp["ldb"], case.ldc, case.ldc
        d.alpha, d.act, d.act_alpha = case.alpha, L.ACT_LEAKY if case.leaky else L.ACT_NONE, LEAKY
        d.accumulate, d.c_f32, d.split_k = case.acc, int(case.c_f32), 0 if case.acc == 2 else 1
        if case.kind == "wgrad_job":
            with L.deferred_reductions(True):
                L.call("fpnmt_gemm_wgrad", d, A.data_ptr(), B.data_ptr(), C.data_ptr(), s)
        else:
            L.call("fpnmt_gemm", d, A.data_ptr(), B.data_ptr(), C.data_ptr(), L.ptr(opt["col_scale"]),
                   L.ptr(opt["bias"]), L.ptr(opt["R"]), s)
        torch.cuda.synchronize()
        return C
    d = L.ConvDesc()
    n, h, w = case.levels[0]
    d.n, d.h, d.w, d.c, d.k, d.r, d.s = n, h, w, case.c, case.ko, case.r, case.r
    d.stride_h = d.stride_w = case.stride
    d.pad_t = d.pad_b = d.pad_l = d.pad_r = case.pad
    d.dtype, d.act, d.act_alpha = L.BF16, L.ACT_LEAKY if case.leaky else L.ACT_NONE, LEAKY
    wt = inp["w"]
    xs, dzs = [x.to(dev) for x in inp["xs"]], [z.to(dev) for z in inp["dzs"]]
    keep += [xs, dzs]
    grouped = len(case.levels) > 1
    esz = C.element_size()
    lv = (L.ConvLevel * len(case.levels))()
    base = 0
    for i, ((n, h, w), m) in enumerate(zip(case.levels, _level_rows(case))):
        lv[i].n, lv[i].h, lv[i].w = n, h, w
        if case.kind != "bwd_filter":  # the level's rows of the output (and of the mask operand)
            lv[i].y = C.data_ptr() + base * N * esz
            if case.mask:
                lv[i].residual = opt["y"].data_ptr() + base * N * esz
            base += m + GUARD_ROWS
    if case.kind == "fwd":
        w_ohwi = wt.permute(3, 0, 1, 2).contiguous().to(dev)
        if grouped:
            for i, x in enumerate(xs):
                lv[i].x = x.data_ptr()
            L.call("fpnmt_conv2d_fwd_grouped", d, len(xs), lv, w_ohwi.data_ptr(), L.ptr(opt["col_scale"]),
                   L.ptr(opt["bias"]), s)
        else:
            L.call("fpnmt_conv2d_fwd", d, xs[0].data_ptr(), w_ohwi.data_ptr(), L.ptr(opt["col_scale"]),
                   L.ptr(opt["bias"]), L.ptr(opt["R"]), C.data_ptr(), s)
    elif case.kind == "bwd_data":
        w_flip = wt.flip(0, 1).permute(2, 0, 1, 3).contiguous().to(dev)
        dz = dzs[0].data_ptr()
        for i, z in enumerate(dzs):
            lv[i].x = z.data_ptr()
        if grouped and case.mask:
            L.call("fpnmt_conv2d_bwd_data_grouped_mask", d, len(dzs), lv, w_flip.data_ptr(), 0, L.ACT_RELU, s)
        elif grouped:
            L.call("fpnmt_conv2d_bwd_data_grouped", d, len(dzs), lv, w_flip.data_ptr(), 0, s)
        elif case.mask and case.res:
            L.call("fpnmt_conv2d_bwd_data_res_act", d, dz, w_flip.data_ptr(), C.data_ptr(), opt["R"].data_ptr(),
                   opt["y"].data_ptr(), L.ACT_RELU, s)
        elif case.mask:
            L.call("fpnmt_conv2d_bwd_data_mask", d, dz, w_flip.data_ptr(), C.data_ptr(), 0, opt["y"].data_ptr(),
                   L.ACT_RELU, s)
        else:
            L.call("fpnmt_conv2d_bwd_data", d, dz, w_flip.data_ptr(), C.data_ptr(), 0, s)
    else:
        if grouped:
            for i, (x, z) in enumerate(zip(xs, dzs)):
                lv[i].x, lv[i].dz = x.data_ptr(), z.data_ptr()
            L.call("fpnmt_conv2d_bwd_filter_grouped", d, len(xs), lv, L.ptr(opt["col_scale"]), C.data_ptr(), s)
        else:
            L.call("fpnmt_conv2d_bwd_filter", d, xs[0].data_ptr(), dzs[0].data_ptr(), L.ptr(opt["col_scale"]),
                   C.data_ptr(), s)
    torch.cuda.synchronize()
    del keep
    return C


def child_main(outdir):
    """Run every case twice in this process (FPNMT_GEMM_LOG set by the parent);
    save the first output, whether the second equals it bit for bit, and the
    log lines of each launch. Any error (a failed call, a HIP error at the
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

    from fpnmt import _lib as L
    for case in CASES:
        inp = inputs(case)
        outs, lines = [], []
        try:
            L.call("fpnmt_set_wide_cfg", int(case.wide or 0))
            for _ in range(2):
                before = len(n_lines())
                outs.append(run_gpu(case, inp))
                lines.append(n_lines()[before:])
        finally:
            L.call("fpnmt_set_wide_cfg", 0)
        res[case.name] = {"out": outs[0].cpu(), "same": bool(torch.equal(outs[0], outs[1])), "log": lines}
        print(case.name, lines[0], flush=True)
    torch.save(res, os.path.join(outdir, "results.pt"))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "fpn-mt-image-captioning_amd"))
    child_main(sys.argv[1])

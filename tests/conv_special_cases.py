"""Case table of the convolutions that bypass the GEMM dispatch, and of the
weight copies they read: the 7x7 / 2 stem forward and weight gradient
(csrc/conv_stem.hip), the single-filter kernels (csrc/conv_n1.hip), the fused
bottleneck (csrc/bottleneck.hip) and fpnmt_weight_prep / _batched
(csrc/optim.hip).

Helper module, not collected. tests/test_conv_special_bars.py (no GPU)
restates the kernels' index arithmetic and proves on planted errors that the
bounds below can fail; tests/test_gpu_conv_special.py runs every case on the
GPU in one child process (this file as a script) and checks route, numerics,
guards, repeatability and the bitwise agreements.

Every case names the entry point, shape, pads, dtype and epilogue, the
`kernel=` it must log in FPNMT_GEMM_LOG (or `fallback`: a GEMM line and no
`conv` line) with the expected grid, and in `note` the branch it is there for.
The expected route is NOT taken from a run: `route(case)` restates the host
predicates of the hooks and the table's literal `kernel` / `grid` fields are
asserted against it by the bars file.

Data
  * random cases: magnitudes in [0.5, 1] with random signs, rounded to the
    storage dtype, seeded (no denormals: v_dot2_f32_bf16's denormal behaviour
    is not documented);
  * reference: fp64 on the CPU from the exact stored operands, in plain
    slicing / einsum form (one term per tap);
  * exact cases (one per kernel): small-integer inputs and sparse {0, +-1}
    weights such that S = sum |a_k b_k| (+ |bias|, |old C|, the residual) is
    <= 256 at every output, which `reference` asserts: every partial sum of any
    summation order is then an integer of magnitude <= 256, exact in bf16 and
    fp32, and the GPU result must equal the reference bit for bit. Every tap
    (and so every halo row) carries a nonzero weight.

Bounds (as tests/gemm_route_cases.py): products of two bf16 values are exact
in fp32, so with S = sum_k |a_k b_k| (+ |bias| and the old C, scaled like the
sum) any fp32 summation order is within (K - 1) 2^-24 S; the bound is
K 2^-23 S plus the output rounding, 2^-23 |ref| for an fp32 output and
2^-8 |ref| for a bf16 one. For fp32 operands each product adds one rounding of
2^-24, inside the same K 2^-23 S. K is 147 for the stem forward, r s c for the
single-filter forward, r s for its bwd-data (the weights are widened exactly),
the number of pixels for both weight gradients. ReLU and leaky ReLU are
1-Lipschitz, so the pre-activation bound carries through them.

The bottleneck stores bf16 between its three stages. The reference is
computed UNROUNDED in fp64 and the error is propagated:
  d1 = K_a 2^-23 S_a + 2^-8 |m1|,                  K_a = c
  d2 = |W3| (*) d1 + K_b 2^-23 S_b + 2^-8 |m2|,    K_b = 9 cm
  d3 = |Wc| d2 + K_c 2^-23 S_c + 2^-8 |y|,         K_c = cm
with the absolute-weight convolutions in fp64 (ReLU is 1-Lipschitz; S_b and
S_c are taken at the reference intermediates plus their own d, so they bound
the kernel's rounded operands too). It is wide by construction; the exact
cases are what catch its seams.

Weight prep is one fp32 multiply and one rounding: the expected value is
(w * scale).to(dtype) permuted and the comparison is bitwise.

Left out: the single-filter bwd-data past its 8192-block cap. At the smallest
channel width that reaches it (bf16 c = 64) it needs > 524288 pixels, a 67 MB
output and a 270 MB fp64 reference per run: not a few seconds.
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
GUARD = 64           # sentinel elements after every output
OFF = 8              # and before it (16 B in bf16, 32 B in fp32: the alignment stays)
LEAKY = 0.2
E_ARG, E_UNSUPPORTED = -1, -2
U_OUT, U_STORE = 2.0 ** -23, 2.0 ** -8


def cdiv(a, b):
    return -(-a // b)


def eps_out(dtype):
    return U_STORE if dtype == BF16 else U_OUT


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) * 7919


def _gen(name, salt=0):
    return torch.Generator().manual_seed(_seed(name) + salt)


def rnd(g, shape, dtype=BF16):
    mag = torch.rand(*shape, generator=g) * 0.5 + 0.5
    sgn = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return (mag * sgn).to(dtype)


def ints(g, shape, lo, hi, dtype=BF16):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype)


def sparse_pm1(g, shape, keep, dtype=BF16):
    """{0, +-1} with about `keep` of the entries nonzero."""
    sgn = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    on = torch.rand(*shape, generator=g) < keep
    return (sgn * on).to(dtype)


def conv_out(i, pa, pb, k, st=1):
    return (i + pa + pb - k) // st + 1


# ============================================================== stem forward
@dataclasses.dataclass(frozen=True)
class StemFwd:
    name: str
    n: int
    h: int
    w: int
    k: int
    pads: tuple  # (t, b, l, r)
    kernel: str  # expected kernel= or "fallback"
    grid: int = 0
    act: str = "none"
    scale: bool = False
    bias: bool = False
    res: bool = False
    xshift: int = 0  # elements the x pointer is moved off its 16-B boundary
    mode: str = "rnd"  # rnd | exact | inf
    claims: tuple = ()
    note: str = ""
    family = "stem_fwd"
    dtype = BF16

    @property
    def out_hw(self):
        t, b, l, r = self.pads
        return conv_out(self.h, t, b, 7, 2), conv_out(self.w, l, r, 7, 2)


_S3, _S0, _SA = (3, 3, 3, 3), (0, 0, 0, 0), (2, 3, 2, 3)
STEM_FWD = [
    StemFwd("sf_misaligned_rows", 8, 9, 37, 64, _S3, "stem7x7s2", 8, claims=("row_d", "neg_E", "partial_tile"),
            note="3w%8=7 and image size %8=7: every row and image starts at another d; first tile E<0 (the "
                 "arithmetic-shift floor); partial tile rows (ho=5) and columns (wo=19)"),
    StemFwd("sf_nopad_two_col_tiles", 8, 21, 75, 64, _S0, "stem7x7s2", 16, claims=("col_tiles", "no_pad"),
            note="no padding, 3w%8=1, wo=35: two column tiles, the second with 3 live columns"),
    StemFwd("sf_asym_k128", 2, 18, 72, 128, _SA, "stem7x7s2", 8, claims=("asym_pads", "k_chunk2", "row_tiles"),
            note="TF 'same' asymmetric pads; k=128: blockIdx.y=1 and its weight offset; ho=9: second row "
                 "tile with one live row"),
    StemFwd("sf_persistent", 1000, 8, 8, 64, _S3, "stem7x7s2", 768, claims=("multi_tile",),
            note="1000 tiles on 768 blocks: some blocks run a second tile on prefetched input, others do "
                 "not; the staged row (69 px) is wider than the image"),
    StemFwd("sf_epi_none", 1, 16, 8, 64, _S3, "stem7x7s2", 1, claims=("epilogue",), note="one tile, no epilogue"),
    StemFwd("sf_epi_relu_bias", 1, 16, 8, 64, _S3, "stem7x7s2", 1, act="relu", bias=True, claims=("epilogue",),
            note="relu, bias set, scale null"),
    StemFwd("sf_epi_leaky_scale", 1, 16, 8, 64, _S3, "stem7x7s2", 1, act="leaky", scale=True,
            claims=("epilogue",), note="leaky, scale set, bias null"),
    StemFwd("sf_epi_relu_scale_bias", 1, 16, 8, 64, _S3, "stem7x7s2", 1, act="relu", scale=True, bias=True,
            claims=("epilogue",), note="relu, scale and bias set"),
    StemFwd("sf_pt_ne_pl", 1, 16, 8, 64, (1, 3, 3, 2), "stem7x7s2", 1, claims=("pt_ne_pl",),
            note="pad_t != pad_l (the 'same' pads above have pt == pl: swapping the two would pass them)"),
    StemFwd("sf_exact", 8, 9, 37, 128, (1, 3, 3, 2), "stem7x7s2", 8, mode="exact", bias=True,
            claims=("exact", "k_chunk2", "pt_ne_pl"),
            note="exact integers: every tap nonzero, four different pads, ragged rows, two channel chunks"),
    StemFwd("sf_inf", 8, 9, 37, 64, _S3, "stem7x7s2", 8, mode="inf", claims=("inf",),
            note="+Inf at element 0 of x (the chunk substituted for out-of-tensor loads) and at one interior "
                 "pixel: the register zeroing of tap 7, the pad channel and the out-of-image mask"),
    StemFwd("sf_fb_total", 3, 37, 37, 64, _S3, "fallback", claims=("fallback",),
            note="n h w 3 % 8 = 1: the implicit GEMM"),
    StemFwd("sf_fb_shift", 8, 9, 37, 64, _S3, "fallback", xshift=1, claims=("fallback",),
            note="x moved by 2 bytes: the implicit GEMM"),
    StemFwd("sf_fb_residual", 1, 16, 8, 64, _S3, "fallback", res=True, claims=("fallback",),
            note="residual set: the implicit GEMM"),
]


def stem_fwd_route(c):
    """stem_conv_fwd's predicate and grid (kernel, grid.x)."""
    total = c.n * c.h * c.w * 3
    if c.res or c.k % 64 or c.xshift or total % 8 or total >= 1 << 31:
        return "fallback", 0
    ho, wo = c.out_hw
    return "stem7x7s2", min(c.n * cdiv(ho, 8) * cdiv(wo, 32), 768)


def stem_fwd_inputs(c):
    g = _gen(c.name)
    shape = (c.n, c.h, c.w, 3)
    if c.mode == "exact":
        x = ints(g, shape, -2, 2)
        w = sparse_pm1(g, (c.k, 7, 7, 3), 0.45)
        w[:, :, :, 0] = torch.where(w.abs().sum(3) == 0, torch.ones(()), w[:, :, :, 0].float()).to(BF16)  # every tap
    else:
        x, w = rnd(g, shape), rnd(g, (c.k, 7, 7, 3))
    if c.mode == "inf":
        x.view(-1)[0] = math.inf
        x[c.n // 2, c.h // 2, c.w // 2, 1] = math.inf
    inp = {"x": x, "w": w}
    if c.scale:
        inp["scale"] = rnd(g, (c.k,), F32)
    if c.bias:
        inp["bias"] = ints(g, (c.k,), -3, 3, F32) if c.mode == "exact" else rnd(g, (c.k,), F32)
    if c.res:
        inp["res"] = rnd(g, (c.n, *c.out_hw, c.k))
    return inp


def _conv_nhwc(x, w_ohwi, pads, stride):
    """fp64 NHWC conv as one term per tap (r, s): sum_c x[..., c] w[k, r, s, c]."""
    t, b, l, r_ = pads
    n, h, w, c = x.shape
    k, R, S, _ = w_ohwi.shape
    ho, wo = conv_out(h, t, b, R, stride), conv_out(w, l, r_, S, stride)
    xp = F.pad(x, (0, 0, l, r_, t, b))
    out = torch.zeros(n, ho, wo, k, dtype=F64)
    for r in range(R):
        for s in range(S):
            xs = xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :]
            out += xs.reshape(-1, c) .matmul(w_ohwi[:, r, s, :].t()).view(n, ho, wo, k)
    return out


def _act(v, act):
    if act == "relu":
        return v.clamp_min(0)
    if act == "leaky":
        return torch.where(v > 0, v, v * LEAKY)
    return v


def stem_fwd_reference(c, inp):
    """{"y": (ref, bound)}; bound None: bitwise. The Inf case: non-finite ref
    elements carry bound inf (their set is compared separately)."""
    x, w = inp["x"].double(), inp["w"].double()
    xf = torch.where(torch.isfinite(x), x, torch.zeros((), dtype=F64))
    lin = _conv_nhwc(x, w, c.pads, 2) if c.mode == "inf" else _conv_nhwc(xf, w, c.pads, 2)
    S = _conv_nhwc(xf.abs(), w.abs(), c.pads, 2)
    if c.scale:
        lin, S = lin * inp["scale"].double(), S * inp["scale"].double().abs()
    if c.bias:
        lin, S = lin + inp["bias"].double(), S + inp["bias"].double().abs()
    if c.res:
        lin, S = lin + inp["res"].double(), S + inp["res"].double().abs()
    ref = _act(lin, c.act)
    if c.mode == "exact":
        assert float(S.max()) <= 256 and bool((ref == ref.round()).all()), (c.name, float(S.max()))
        return {"y": (ref, None)}
    bnd = 147 * U_OUT * S + U_STORE * ref.abs()
    bnd = torch.where(torch.isfinite(ref), bnd, torch.full((), math.inf, dtype=F64))
    return {"y": (ref, bnd)}


# ====================================================== stem weight gradient
@dataclasses.dataclass(frozen=True)
class StemWgrad:
    name: str
    n: int
    h: int
    w: int
    pads: tuple
    kernel: str
    grid: int = 0
    k: int = 64
    col_scale: bool = False
    mode: str = "rnd"
    claims: tuple = ()
    note: str = ""
    family = "stem_wgrad"
    dtype = BF16

    @property
    def out_hw(self):
        t, b, l, r = self.pads
        return conv_out(self.h, t, b, 7, 2), conv_out(self.w, l, r, 7, 2)


STEM_WGRAD = [
    StemWgrad("sw_two_rows", 65, 16, 16, _S3, "stem_wgrad112", 512, claims=("row_loop",),
              note="rows 520 > grid 512 (<112>): eight blocks walk two rows"),
    StemWgrad("sw_odd_wo", 67, 16, 16, _S0, "stem_wgrad112", 335, col_scale=True, claims=("odd_wo", "no_pad", "scale"),
              note="wo=5 is odd: the pixel pair's second half is zeroed; no padding; col_scale set"),
    StemWgrad("sw_256_two_rows", 33, 16, 232, _S3, "stem_wgrad256", 256, claims=("wp256", "row_loop"),
              note="wo=116 -> WP=128 -> <256>; rows 264 > grid 256"),
    StemWgrad("sw_256_asym", 35, 13, 232, _SA, "stem_wgrad256", 210, col_scale=True, claims=("wp256", "asym_pads"),
              note="<256>, asymmetric pads, one row per block"),
    StemWgrad("sw_last_112", 2, 16, 224, _S3, "stem_wgrad112", 16, claims=("wp112_edge",),
              note="wo=112: the last width on <112>"),
    StemWgrad("sw_widest", 1, 10, 512, _S3, "stem_wgrad256", 5, claims=("widest",),
              note="wo=256: the widest the kernel takes"),
    StemWgrad("sw_pad_cols", 3, 9, 40, _S0, "stem_wgrad112", 6, claims=("pad_cols",),
              note="wo=17 -> WP=32: 15 zero pad columns inside the MFMA k range"),
    StemWgrad("sw_exact", 65, 16, 16, _SA, "stem_wgrad112", 512, mode="exact", claims=("exact", "row_loop"),
              note="exact integers, two rows on eight blocks, asymmetric pads"),
    StemWgrad("sw_fb_w", 2, 16, 20, _S3, "fallback", claims=("fallback",), note="w % 8 != 0: the implicit GEMM"),
    StemWgrad("sw_fb_k128", 2, 16, 16, _S3, "fallback", k=128, claims=("fallback",), note="k = 128: the implicit GEMM"),
]


def stem_wgrad_route(c):
    """stem_conv_bwd_filter's predicate, kernel choice and grid."""
    ho, wo = c.out_hw
    if c.k != 64 or c.w % 8 or ho <= 0 or wo <= 0 or 2 * wo > 512 or c.w > 512:
        return "fallback", 0
    wp = cdiv(wo, 16) * 16
    if wp > 256 or c.w > 2 * wp:
        return "fallback", 0
    rows = c.n * ho
    return ("stem_wgrad112", min(rows, 512)) if wp <= 112 else ("stem_wgrad256", min(rows, 256))


def stem_wgrad_inputs(c):
    g = _gen(c.name)
    ho, wo = c.out_hw
    if c.mode == "exact":
        x = ints(g, (c.n, c.h, c.w, 3), -2, 2)
        dz = sparse_pm1(g, (c.n, ho, wo, c.k), 100.0 / (c.n * ho * wo))  # ~100 live pixels per channel
        old = ints(g, (7, 7, 3, c.k), -8, 8, F32)
    else:
        x, dz = rnd(g, (c.n, c.h, c.w, 3)), rnd(g, (c.n, ho, wo, c.k))
        old = rnd(g, (7, 7, 3, c.k), F32)
    inp = {"x": x, "dz": dz, "old": old}
    if c.col_scale:
        inp["col_scale"] = rnd(g, (c.k,), F32)
    return inp


def _wgrad_nhwc(x, dz, R, S, pads, stride):
    """fp64 dw[r, s, c, k] = sum_pixels x[n, st oh + r - pt, st ow + s - pl, c] dz[n, oh, ow, k]."""
    t, b, l, r_ = pads
    n, ho, wo, k = dz.shape
    c = x.shape[3]
    xp = F.pad(x, (0, 0, l, r_, t, b))
    dzf = dz.reshape(-1, k)
    out = torch.zeros(R, S, c, k, dtype=F64)
    for r in range(R):
        for s in range(S):
            xs = xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :]
            out[r, s] = xs.reshape(-1, c).t().matmul(dzf)
    return out


def stem_wgrad_reference(c, inp):
    x, dz, old = inp["x"].double(), inp["dz"].double(), inp["old"].double()
    lin = _wgrad_nhwc(x, dz, 7, 7, c.pads, 2)
    S = _wgrad_nhwc(x.abs(), dz.abs(), 7, 7, c.pads, 2)
    if c.col_scale:
        lin, S = lin * inp["col_scale"].double(), S * inp["col_scale"].double().abs()
    ref, S = old + lin, old.abs() + S
    if c.mode == "exact":
        assert float(S.max()) <= 256 and bool((ref == ref.round()).all()), (c.name, float(S.max()))
        return {"dw": (ref, None)}
    ho, wo = c.out_hw
    return {"dw": (ref, c.n * ho * wo * U_OUT * S + U_OUT * ref.abs())}


# ====================================================== single-filter kernels
@dataclasses.dataclass(frozen=True)
class N1:
    name: str
    op: str  # fwd | bwd_data | bwd_filter
    dtype: torch.dtype
    c: int
    r: int
    s: int
    pads: tuple
    levels: tuple  # ((n, h, w), ...); more than one, or grouped=True: the _grouped entry point
    kernel: str
    grid: int = 0
    grouped: bool = False
    act: str = "none"
    scale: bool = False
    bias: bool = False
    res: bool = False       # fwd: residual set -> fallback
    mask: bool = False      # bwd_data: the ReLU mask of y_in (also run plain: masked == plain * (y > 0) bitwise)
    col_scale: bool = False  # bwd_filter: col_scale set -> fallback
    mode: str = "rnd"
    claims: tuple = ()
    note: str = ""
    family = "n1"

    @property
    def is_grouped(self):
        return self.grouped or len(self.levels) > 1

    def out_hw(self, h, w):
        t, b, l, r = self.pads
        return conv_out(h, t, b, self.r), conv_out(w, l, r, self.s)


def _same(r, s):
    return ((r - 1) // 2, r // 2, (s - 1) // 2, s // 2)


def n1_live(c):
    """The levels n1_args keeps, with their output shapes."""
    out = []
    for n, h, w in c.levels:
        ho, wo = c.out_hw(h, w)
        if n > 0 and h > 0 and w > 0 and ho > 0 and wo > 0:
            out.append((n, h, w, ho, wo))
    return out


def n1_pixels(c):
    return sum(n * ho * wo if c.op == "fwd" else n * h * w for n, h, w, ho, wo in n1_live(c))


def n1_route(c):
    """conv_n1's predicates and the three launchers' grids."""
    vn = 8 if c.dtype == BF16 else 4
    kern = "n1_" + c.op
    if c.c % vn or c.r > 3 or c.s > 3:
        return "fallback", 0
    cv = c.c // vn
    if cv & (cv - 1) or cv < 8 or cv > 128:
        return "fallback", 0
    live = n1_live(c)
    if len(live) > 6 or not live or (c.op == "fwd" and c.res) or (c.op == "bwd_filter" and c.col_scale):
        return "fallback", 0
    if c.op == "bwd_data" and any(n * h * w > 0 and min(c.out_hw(h, w)) <= 0 for n, h, w in c.levels):
        return "fallback", 0  # a level without output pixels needs the entry point's zero fill
    P = n1_pixels(c)
    if P * c.c >= 1 << 31:
        return "fallback", 0
    if c.op == "fwd":
        lpp = min(cv, 64)
        return kern, min(1024, max(1, ((P * lpp + 63) // 64 + 7) // 8))
    if c.op == "bwd_data":
        return kern, min(8192, max(1, (P * cv + 511) // 512))
    nb = min(1024, max(1, P // 16))
    return kern, cdiv(P, cdiv(P, nb))


# (kernel, grid) per single-filter case: literals, checked against n1_route by the bars file
N1_EXPECT = {
    "n1_fwd_bf16_cv8": ("n1_fwd", 2),
    "n1_bwd_data_bf16_cv8": ("n1_bwd_data", 2),
    "n1_bwd_filter_bf16_cv8": ("n1_bwd_filter", 4),
    "n1_fwd_bf16_cv16": ("n1_fwd", 3),
    "n1_bwd_data_bf16_cv16": ("n1_bwd_data", 3),
    "n1_bwd_filter_bf16_cv16": ("n1_bwd_filter", 4),
    "n1_fwd_bf16_cv32": ("n1_fwd", 5),
    "n1_bwd_data_bf16_cv32": ("n1_bwd_data", 5),
    "n1_bwd_filter_bf16_cv32": ("n1_bwd_filter", 4),
    "n1_fwd_bf16_cv64": ("n1_fwd", 9),
    "n1_bwd_data_bf16_cv64": ("n1_bwd_data", 9),
    "n1_bwd_filter_bf16_cv64": ("n1_bwd_filter", 4),
    "n1_fwd_bf16_cv128": ("n1_fwd", 9),
    "n1_bwd_data_bf16_cv128": ("n1_bwd_data", 18),
    "n1_bwd_filter_bf16_cv128": ("n1_bwd_filter", 4),
    "n1_fwd_f32_cv8": ("n1_fwd", 2),
    "n1_bwd_data_f32_cv8": ("n1_bwd_data", 2),
    "n1_bwd_filter_f32_cv8": ("n1_bwd_filter", 4),
    "n1_fwd_f32_cv16": ("n1_fwd", 3),
    "n1_bwd_data_f32_cv16": ("n1_bwd_data", 3),
    "n1_bwd_filter_f32_cv16": ("n1_bwd_filter", 4),
    "n1_fwd_f32_cv32": ("n1_fwd", 5),
    "n1_bwd_data_f32_cv32": ("n1_bwd_data", 5),
    "n1_bwd_filter_f32_cv32": ("n1_bwd_filter", 4),
    "n1_fwd_f32_cv64": ("n1_fwd", 9),
    "n1_bwd_data_f32_cv64": ("n1_bwd_data", 9),
    "n1_bwd_filter_f32_cv64": ("n1_bwd_filter", 4),
    "n1_fwd_f32_cv128": ("n1_fwd", 9),
    "n1_bwd_data_f32_cv128": ("n1_bwd_data", 18),
    "n1_bwd_filter_f32_cv128": ("n1_bwd_filter", 4),
    "n1_fwd_fb_f32_c1024": ("fallback", 0),
    "n1_fwd_fb_bf16_c32": ("fallback", 0),
    "n1_bwd_data_fb_f32_c1024": ("fallback", 0),
    "n1_bwd_data_fb_bf16_c32": ("fallback", 0),
    "n1_bwd_filter_fb_f32_c1024": ("fallback", 0),
    "n1_bwd_filter_fb_bf16_c32": ("fallback", 0),
    "n1_fwd_valid3x3": ("n1_fwd", 1),
    "n1_bwd_data_valid3x3": ("n1_bwd_data", 3),
    "n1_bwd_filter_valid3x3": ("n1_bwd_filter", 5),
    "n1_fwd_1x1": ("n1_fwd", 3),
    "n1_bwd_data_1x1": ("n1_bwd_data", 3),
    "n1_bwd_filter_1x1": ("n1_bwd_filter", 5),
    "n1_fwd_1x3": ("n1_fwd", 3),
    "n1_bwd_data_1x3": ("n1_bwd_data", 3),
    "n1_bwd_filter_1x3": ("n1_bwd_filter", 5),
    "n1_fwd_3x1": ("n1_fwd", 3),
    "n1_bwd_data_3x1": ("n1_bwd_data", 3),
    "n1_bwd_filter_3x1": ("n1_bwd_filter", 5),
    "n1_fwd_2x2": ("n1_fwd", 3),
    "n1_bwd_data_2x2": ("n1_bwd_data", 3),
    "n1_bwd_filter_2x2": ("n1_bwd_filter", 5),
    "n1_fwd_levels_mix": ("n1_fwd", 2),
    "n1_fwd_levels_six": ("n1_fwd", 3),
    "n1_fwd_levels_seven": ("fallback", 0),
    "n1_bwd_data_levels_mix": ("n1_bwd_data", 2),
    "n1_bwd_data_levels_six": ("n1_bwd_data", 3),
    "n1_bwd_data_levels_seven": ("fallback", 0),
    "n1_bwd_filter_levels_mix": ("n1_bwd_filter", 5),
    "n1_bwd_filter_levels_six": ("n1_bwd_filter", 5),
    "n1_bwd_filter_levels_seven": ("fallback", 0),
    "n1_fwd_epi_relu_bias": ("n1_fwd", 5),
    "n1_fwd_epi_leaky_scale": ("n1_fwd", 5),
    "n1_fwd_epi_relu_scale_bias": ("n1_fwd", 5),
    "n1_fwd_fb_residual": ("fallback", 0),
    "n1_bwd_data_mask": ("n1_bwd_data", 5),
    "n1_bwd_data_mask_grouped": ("n1_bwd_data", 3),
    "n1_bwd_data_small_level_valid": ("fallback", 0),
    "n1_bwd_filter_fb_col_scale": ("fallback", 0),
    "n1_bwd_filter_one_block": ("n1_bwd_filter", 1),
    "n1_fwd_grid_cap": ("n1_fwd", 1024),
    "n1_bwd_filter_grid_cap": ("n1_bwd_filter", 995),
    "n1_fwd_grid_14": ("n1_fwd", 14),
    "n1_bwd_data_grid_13": ("n1_bwd_data", 13),
    "n1_fwd_exact": ("n1_fwd", 2),
    "n1_bwd_data_exact": ("n1_bwd_data", 2),
    "n1_bwd_filter_exact": ("n1_bwd_filter", 4),
}


def _n1_cases():
    out = []
    lv1 = ((2, 5, 7),)

    def add(name, op, dtype, c, r=3, s=3, pads=None, levels=lv1, **kw):
        kern, grid = N1_EXPECT[name]
        out.append(N1(name, op, dtype, c, r, s, pads if pads is not None else _same(r, s), tuple(levels), kern, grid, **kw))

    ops = ("fwd", "bwd_data", "bwd_filter")
    # channel widths: every cv in {8 .. 128}, both dtypes, every pass
    for dtype, tag, vn in ((BF16, "bf16", 8), (F32, "f32", 4)):
        for cv in (8, 16, 32, 64, 128):
            for op in ops:
                add(f"n1_{op}_{tag}_cv{cv}", op, dtype, cv * vn, claims=(f"cv{cv}_{tag}",),
                    note=f"{tag} cv={cv}: " + ("LPP=64 NCH=2" if cv == 128 else f"LPP={cv}" if op == "fwd" else "width"))
    for op in ops:
        add(f"n1_{op}_fb_f32_c1024", op, F32, 1024, claims=("fallback_width",), note="fp32 cv=256 > 128: the GEMM")
        add(f"n1_{op}_fb_bf16_c32", op, BF16, 32, claims=("fallback_width",), note="bf16 cv=4 < 8: the GEMM")
    # kernel shapes, bf16 c=128 and fp32 c=32 forward/backward
    shapes = (("valid3x3", 3, 3, (0, 0, 0, 0)), ("1x1", 1, 1, None), ("1x3", 1, 3, (0, 0, 1, 1)),
              ("3x1", 3, 1, None), ("2x2", 2, 2, (0, 1, 0, 1)))
    for tag, r, s, pads in shapes:
        for op in ops:
            add(f"n1_{op}_{tag}", op, BF16, 128, r, s, pads, levels=((2, 5, 7), (1, 4, 3)), claims=(f"shape_{tag}",),
                note=f"{tag}: tap index t / S, t % S with R != S or a one-sided pad")
    # levels
    mix = ((2, 5, 7), (1, 1, 1), (3, 1, 1), (0, 4, 4), (1, 3, 2), (2, 1, 1))
    six = ((2, 5, 7), (1, 1, 1), (3, 1, 1), (1, 3, 2), (2, 1, 1), (1, 2, 5))
    seven = six + ((1, 3, 3),)
    for op in ops:
        add(f"n1_{op}_levels_mix", op, BF16, 64, levels=mix, claims=("levels_1x1", "levels_empty"),
            note="1x1 levels: a level boundary inside a wave and inside a U pixel group; an empty level in the middle")
        add(f"n1_{op}_levels_six", op, F32, 64, levels=six, claims=("levels_six",), note="six live levels")
        add(f"n1_{op}_levels_seven", op, BF16, 64, levels=seven, claims=("levels_seven",),
            note="seven live levels: the GEMM")
    # forward epilogue
    for tag, kw in (("relu_bias", dict(act="relu", bias=True)), ("leaky_scale", dict(act="leaky", scale=True)),
                    ("relu_scale_bias", dict(act="relu", scale=True, bias=True))):
        add(f"n1_fwd_epi_{tag}", "fwd", BF16, 256, levels=((2, 5, 7), (1, 2, 2)), claims=("fwd_epilogue",), note=tag, **kw)
    add("n1_fwd_fb_residual", "fwd", BF16, 256, res=True, claims=("fwd_residual",), note="residual: the GEMM epilogue has it")
    # bwd-data
    add("n1_bwd_data_mask", "bwd_data", BF16, 256, mask=True, claims=("mask",), note="single entry, ReLU mask of y_in")
    add("n1_bwd_data_mask_grouped", "bwd_data", F32, 64, levels=mix, mask=True, claims=("mask",),
        note="grouped, ReLU mask per level")
    add("n1_bwd_data_small_level_valid", "bwd_data", BF16, 128, pads=(0, 0, 0, 0), levels=((2, 5, 5), (1, 2, 2)),
        claims=("small_level",), note="'valid' 3x3 over a 2x2 level: no dz, the zero fill; the GEMM route")
    # bwd-filter
    add("n1_bwd_filter_fb_col_scale", "bwd_filter", BF16, 256, col_scale=True, claims=("wgrad_scale",),
        note="col_scale set: the GEMM")
    add("n1_bwd_filter_one_block", "bwd_filter", BF16, 128, levels=((1, 3, 3),), claims=("one_block",), note="P = 9 < 16: one block")
    # grid caps and a grid that is no multiple of 8
    add("n1_fwd_grid_cap", "fwd", BF16, 64, levels=((4, 130, 130),), claims=("fwd_cap",),
        note="8450 waves > 1024 x 8: per = 2, the last active block partial")
    add("n1_bwd_filter_grid_cap", "bwd_filter", BF16, 64, levels=((4, 65, 65),), claims=("wgrad_cap", "grid_not_8"),
        note="P = 16900 > 16384: 17 pixels per block, 995 blocks (no multiple of 8)")
    add("n1_fwd_grid_14", "fwd", BF16, 64, levels=((2, 20, 21),), claims=("grid_not_8",), note="14 blocks: the XCD remap's r != 0")
    add("n1_bwd_data_grid_13", "bwd_data", BF16, 64, levels=((1, 27, 30),), claims=("grid_not_8",),
        note="13 blocks: the XCD remap's r != 0; the last round partial")
    # exact integers
    for op in ops:
        add(f"n1_{op}_exact", op, BF16, 64, levels=((2, 5, 7), (1, 1, 1), (1, 3, 2)), mode="exact", claims=("exact",),
            bias=op == "fwd", note="exact integers over three levels")
    return out


N1_CASES = _n1_cases()


def n1_inputs(c):
    g = _gen(c.name)
    exact = c.mode == "exact"
    inp = {"xs": [], "dzs": [], "ys": [], "res": []}
    for n, h, w in c.levels:
        ho, wo = c.out_hw(h, w)
        ho, wo = max(ho, 0), max(wo, 0)
        if exact:
            inp["xs"].append(ints(g, (n, h, w, c.c), -2, 2, c.dtype))
            inp["dzs"].append(ints(g, (n, ho, wo, 1), -2, 2, c.dtype) if c.op == "bwd_data"
                              else sparse_pm1(g, (n, ho, wo, 1), 0.5, c.dtype))
        else:
            inp["xs"].append(rnd(g, (n, h, w, c.c), c.dtype))
            inp["dzs"].append(rnd(g, (n, ho, wo, 1), c.dtype))
        inp["ys"].append(rnd(g, (n, h, w, c.c), c.dtype))        # y_in of the act' mask (x's layout)
        inp["res"].append(rnd(g, (n, ho, wo, 1), c.dtype))
    if exact and c.op == "fwd":
        w = sparse_pm1(g, (c.r, c.s, c.c), 8.0 / c.c, c.dtype)
        w[:, :, 0] = torch.where(w.float().abs().sum(2) == 0, torch.ones(()), w[:, :, 0].float()).to(c.dtype)
    elif exact:
        w = sparse_pm1(g, (c.r, c.s, c.c), 0.6, c.dtype)
        w[:, :, 0] = 1
    else:
        w = rnd(g, (c.r, c.s, c.c), c.dtype)
    inp["w"] = w  # [r][s][c]: OHWI of the one filter, HWIO with k = 1
    inp["old"] = ints(g, (c.r, c.s, c.c), -8, 8, F32) if exact else rnd(g, (c.r, c.s, c.c), F32)
    if c.scale:
        inp["scale"] = rnd(g, (1,), F32)
    if c.bias:
        inp["bias"] = ints(g, (1,), -3, 3, F32) if exact else rnd(g, (1,), F32)
    if c.col_scale:
        inp["col_scale"] = rnd(g, (1,), F32)
    return inp


def _n1_bwd_data(dz, w, h, w_in, pads):
    """fp64 dx[n, ih, iw, c] = sum_{r,s} dz[n, ih - r + pt, iw - s + pl] w[r, s, c]."""
    t, b, l, r_ = pads
    R, S, C = w.shape
    n, ho, wo = dz.shape[:3]
    dx = torch.zeros(n, h, w_in, C, dtype=F64)
    if ho <= 0 or wo <= 0:
        return dx
    # dz on the padded input grid: canvas[ih + R - 1 - r ...]; plain loops over taps
    for r in range(R):
        for s in range(S):
            # input pixel (ih, iw) = (oh + r - pt, ow + s - pl)
            ih0, iw0 = r - t, s - l
            oh_lo, oh_hi = max(0, -ih0), min(ho, h - ih0)
            ow_lo, ow_hi = max(0, -iw0), min(wo, w_in - iw0)
            if oh_lo >= oh_hi or ow_lo >= ow_hi:
                continue
            dx[:, oh_lo + ih0:oh_hi + ih0, ow_lo + iw0:ow_hi + iw0, :] += dz[:, oh_lo:oh_hi, ow_lo:ow_hi, :] * w[r, s]
    return dx


def n1_reference(c, inp):
    """{output name: (ref, bound or None)}: fwd y<i>, bwd_data dx<i> (every
    level of the table with pixels, zero where the level has no dz), bwd_filter dw."""
    w = inp["w"].double()
    eo = eps_out(c.dtype)
    exact = c.mode == "exact"
    out = {}

    def fin(name, ref, S, K, e):
        if exact:
            assert float(S.max()) <= 256 and bool((ref == ref.round()).all()), (c.name, name, float(S.max()))
            out[name] = (ref, None)
        else:
            out[name] = (ref, K * U_OUT * S + e * ref.abs())

    if c.op == "bwd_filter":
        lin = torch.zeros(c.r, c.s, c.c, dtype=F64)
        S = torch.zeros_like(lin)
        K = 0
        for i, (n, h, w_) in enumerate(c.levels):
            ho, wo = c.out_hw(h, w_)
            if n <= 0 or ho <= 0 or wo <= 0:
                continue
            x, dz = inp["xs"][i].double(), inp["dzs"][i].double()
            lin += _wgrad_nhwc(x, dz, c.r, c.s, c.pads, 1)[..., 0]
            S += _wgrad_nhwc(x.abs(), dz.abs(), c.r, c.s, c.pads, 1)[..., 0]
            K += n * h * w_  # the kernel walks input pixels
        if c.col_scale:
            lin, S = lin * inp["col_scale"].double(), S * inp["col_scale"].double().abs()
        old = inp["old"].double()
        fin("dw", old + lin, old.abs() + S, max(K, 1), U_OUT)
        return out
    for i, (n, h, w_) in enumerate(c.levels):
        ho, wo = c.out_hw(h, w_)
        if c.op == "fwd":
            if n <= 0 or ho <= 0 or wo <= 0:
                continue
            x = inp["xs"][i].double()
            lin = _conv_nhwc(x, w[None], c.pads, 1)
            S = _conv_nhwc(x.abs(), w.abs()[None], c.pads, 1)
            if c.scale:
                lin, S = lin * inp["scale"].double(), S * inp["scale"].double().abs()
            if c.bias:
                lin, S = lin + inp["bias"].double(), S + inp["bias"].double().abs()
            if c.res:
                lin, S = lin + inp["res"][i].double(), S + inp["res"][i].double().abs()
            fin(f"y{i}", _act(lin, c.act), S, c.r * c.s * c.c, eo)
        else:
            if n * h * w_ <= 0:
                continue
            dz = inp["dzs"][i].double()
            lin = _n1_bwd_data(dz, w, h, w_, c.pads)
            S = _n1_bwd_data(dz.abs(), w.abs(), h, w_, c.pads)
            if c.mask:
                m = (inp["ys"][i].double() > 0).double()
                lin, S = lin * m, S * m
            fin(f"dx{i}", lin, S, c.r * c.s, eo)
    return out


# ========================================================== fused bottleneck
@dataclasses.dataclass(frozen=True)
class Bneck:
    name: str
    n: int
    hw: int
    c: int
    cm: int
    grid: int
    uniq: int = 3  # distinct images (image i = base[i % uniq]: one reference per distinct image)
    mode: str = "rnd"
    claims: tuple = ()
    note: str = ""
    family = "bottleneck"
    dtype = BF16
    kernel = "bottleneck"

    @property
    def tr(self):
        return 2 if self.hw == 56 else 4


BNECK = [
    Bneck("bn_res2_n1", 1, 56, 256, 64, 28, uniq=1, claims=("few_tiles",), note="28 tiles: fewer than the 256 blocks"),
    Bneck("bn_res2_n10", 10, 56, 256, 64, 256, claims=("many_tiles",),
          note="280 tiles: exceeds and does not divide the 256 blocks"),
    Bneck("bn_res3_n1", 1, 28, 512, 128, 7, uniq=1, claims=("few_tiles",), note="7 tiles"),
    Bneck("bn_res3_n37", 37, 28, 512, 128, 256, claims=("many_tiles",),
          note="259 tiles: exceeds and does not divide the 256 blocks"),
    Bneck("bn_res2_exact", 10, 56, 256, 64, 256, mode="exact", claims=("exact",),
          note="exact integers, neighbouring images differ: a halo row read from the next image shows"),
    Bneck("bn_res3_exact", 37, 28, 512, 128, 256, mode="exact", claims=("exact",),
          note="exact integers, neighbouring images differ"),
]


def bneck_route(c):
    """fpnmt_bottleneck_fwd's shape test and launch_bottleneck's grid."""
    if (c.c, c.cm, c.hw) == (256, 64, 56):
        return "bottleneck", min(c.n * 28, 256)
    if (c.c, c.cm, c.hw) == (512, 128, 28):
        return "bottleneck", min(c.n * 7, 256)
    return "unsupported", 0


def bneck_inputs(c):
    g = _gen(c.name)
    u, h, C, CM = c.uniq, c.hw, c.c, c.cm
    if c.mode == "exact":
        base = ints(g, (u, h, h, C), -1, 2)

        def rows(k_out, k_in, per):  # `per` nonzeros (+-1) in every row
            w = torch.zeros(k_out, k_in)
            for o in range(k_out):
                idx = torch.randperm(k_in, generator=g)[:per]
                w[o, idx] = (torch.randint(0, 2, (per,), generator=g) * 2 - 1).float()
            return w
        wa = rows(CM, C, 4).to(BF16)
        w3 = torch.stack([rows(CM, CM, 1) for _ in range(9)], 1).view(CM, 3, 3, CM).to(BF16)  # every tap: one per row
        wc = rows(C, CM, 2).to(BF16)
        ba, b3, bc = (ints(g, (k,), 0, 2, F32) for k in (CM, CM, C))
    else:
        base = rnd(g, (u, h, h, C))
        # weights scaled so the three stages keep O(1) magnitudes (powers of two: the [0.5, 1] mantissas stay)
        wa = (rnd(g, (CM, C)).float() / 16).to(BF16)
        w3 = (rnd(g, (CM, 3, 3, CM)).float() / 16).to(BF16)
        wc = (rnd(g, (C, CM)).float() / 8).to(BF16)
        ba, b3, bc = rnd(g, (CM,), F32), rnd(g, (CM,), F32), rnd(g, (C,), F32)
    return {"base": base, "wa": wa, "w3": w3, "wc": wc, "ba": ba, "b3": b3, "bc": bc}


def bneck_x(c, inp):
    return inp["base"][torch.arange(c.n) % c.uniq].contiguous()


def bneck_stages(c, inp, mutate=None):
    """fp64, unrounded: (m1, m2, y, d3 or None) over the distinct images."""
    x = inp["base"].double()
    wa, w3, wc = inp["wa"].double(), inp["w3"].double(), inp["wc"].double()
    ba, b3, bc = inp["ba"].double(), inp["b3"].double(), inp["bc"].double()
    same = (1, 1, 1, 1)
    a1 = x.matmul(wa.t()) + ba
    m1 = a1.clamp_min(0)
    a2 = _conv_nhwc(m1, w3, same, 1) + b3
    m2 = a2.clamp_min(0)
    a3 = m2.matmul(wc.t()) + bc + x
    y = a3.clamp_min(0)
    Sa = x.abs().matmul(wa.abs().t()) + ba.abs()
    if c.mode == "exact":
        Sb = _conv_nhwc(m1, w3.abs(), same, 1) + b3.abs()
        Sc = m2.matmul(wc.abs().t()) + bc.abs() + x.abs()
        assert max(float(Sa.max()), float(Sb.max()), float(Sc.max())) <= 256, (c.name, float(Sa.max()),
                                                                              float(Sb.max()), float(Sc.max()))
        assert all(bool((t == t.round()).all()) for t in (m1, m2, y))
        return m1, m2, y, None
    C, CM = c.c, c.cm
    d1 = C * U_OUT * Sa + U_STORE * m1
    Sb = _conv_nhwc(m1 + d1, w3.abs(), same, 1) + b3.abs()
    d2 = _conv_nhwc(d1, w3.abs(), same, 1) + 9 * CM * U_OUT * Sb + U_STORE * m2
    Sc = (m2 + d2).matmul(wc.abs().t()) + bc.abs() + x.abs()
    d3 = d2.matmul(wc.abs().t()) + CM * U_OUT * Sc + U_STORE * y
    return m1, m2, y, d3


def bneck_reference(c, inp):
    _, _, y, d3 = bneck_stages(c, inp)
    idx = torch.arange(c.n) % c.uniq
    return {"y": (y[idx], None if d3 is None else d3[idx])}


# ================================================================ weight prep
@dataclasses.dataclass(frozen=True)
class WPrep:
    name: str
    dtype: torch.dtype
    shape: tuple  # (r, s, c, k)
    scale: bool = True
    ld_extra: int = 0  # 0: ld_flip = 0 (dense); else ld_flip = r s k + ld_extra
    ohwi: bool = True
    flip: bool = True
    claims: tuple = ()
    note: str = ""
    family = "wprep"
    kernel = "wprep"
    grid = 0


def _wprep_cases():
    out = []
    for dtype, tag in ((BF16, "bf16"), (F32, "f32")):
        for shape in ((3, 3, 33, 65), (7, 7, 3, 64), (1, 1, 5, 1), (1, 3, 40, 36)):
            nm = "x".join(map(str, shape))
            out.append(WPrep(f"wp_{tag}_{nm}", dtype, shape, claims=("ragged",), note="ragged c and k tiles"))
        out.append(WPrep(f"wp_{tag}_k_not4", dtype, (3, 3, 33, 65), ld_extra=7, claims=("ld_flip", "k_not4"),
                         note="k % 4 = 1; ld_flip = r s k + 7: odd rows of the flipped copy, the gap stays"))
        out.append(WPrep(f"wp_{tag}_noscale", dtype, (1, 3, 40, 36), scale=False, ld_extra=4, claims=("no_scale", "ld_flip"),
                         note="scale null; ld_flip = r s k + 4: 8-B aligned flipped rows"))
        out.append(WPrep(f"wp_{tag}_ohwi_only", dtype, (3, 3, 33, 65), flip=False, claims=("null_dst",), note="w_flip null"))
        out.append(WPrep(f"wp_{tag}_flip_only", dtype, (3, 3, 33, 65), ohwi=False, claims=("null_dst",), note="w_ohwi null"))
    return out


WPREP = _wprep_cases()


def wprep_ld(c):
    r, s, _, k = c.shape
    return r * s * k + c.ld_extra if c.ld_extra else 0


def wprep_inputs(c):
    g = _gen(c.name)
    inp = {"w": rnd(g, c.shape, F32)}
    if c.scale:
        inp["scale"] = rnd(g, (c.shape[3],), F32)
    return inp


def wprep_expected(c, inp, mutate=None):
    """(ohwi [k][r][s][c] flat, flip [c][ldf] with the gaps at the sentinel)
    in the case's dtype; `mutate`: a planted error (the bars file)."""
    r, s, ci, k = c.shape
    w = inp["w"]
    if mutate == "scale_by_c" and c.scale:
        v = w * inp["scale"][torch.arange(ci) % k][None, None, :, None]
    else:
        v = w * inp["scale"] if c.scale else w  # one fp32 multiply
    v = v.to(c.dtype)                            # one rounding
    ohwi = v.permute(3, 0, 1, 2).contiguous().view(-1)
    ldf = r * s * k if (c.ld_extra == 0 or mutate == "ld_ignored") else r * s * k + c.ld_extra
    fl = v if mutate == "no_flip" else v.flip(0, 1)
    body = fl.permute(2, 0, 1, 3).contiguous().view(ci, r * s * k)
    flip = torch.full((ci, ldf), SENTINEL, dtype=c.dtype)
    flip[:, :r * s * k] = body
    return ohwi, flip.view(-1)


# ======================================================================= all
FAMILIES = {
    "stem_fwd": (STEM_FWD, stem_fwd_route, stem_fwd_inputs, stem_fwd_reference),
    "stem_wgrad": (STEM_WGRAD, stem_wgrad_route, stem_wgrad_inputs, stem_wgrad_reference),
    "n1": (N1_CASES, n1_route, n1_inputs, n1_reference),
    "bottleneck": (BNECK, bneck_route, bneck_inputs, bneck_reference),
}
ROUTED = STEM_FWD + STEM_WGRAD + N1_CASES  # the cases whose launch writes (or must not write) a conv line
CASES = ROUTED + BNECK
BY_NAME = {c.name: c for c in CASES + WPREP}
assert len(BY_NAME) == len(CASES) + len(WPREP)

# every branch the issue names -> claimed by a case (test_conv_special_bars asserts the cover)
BRANCHES = {
    "stem_fwd": {"row_d", "neg_E", "partial_tile", "col_tiles", "no_pad", "asym_pads", "k_chunk2", "row_tiles",
                 "multi_tile", "epilogue", "exact", "inf", "fallback", "pt_ne_pl"},
    "stem_wgrad": {"row_loop", "odd_wo", "no_pad", "scale", "wp256", "asym_pads", "wp112_edge", "widest", "pad_cols",
                   "exact", "fallback"},
    "n1": {f"cv{cv}_{t}" for cv in (8, 16, 32, 64, 128) for t in ("bf16", "f32")} | {
        "fallback_width", "shape_valid3x3", "shape_1x1", "shape_1x3", "shape_3x1", "shape_2x2", "levels_1x1",
        "levels_empty", "levels_six", "levels_seven", "fwd_epilogue", "fwd_residual", "mask", "small_level",
        "wgrad_scale", "one_block", "fwd_cap", "wgrad_cap", "grid_not_8", "exact"},
    "bottleneck": {"few_tiles", "many_tiles", "exact"},
    "wprep": {"ragged", "ld_flip", "k_not4", "no_scale", "null_dst"},
}


def inputs(case):
    return wprep_inputs(case) if case.family == "wprep" else FAMILIES[case.family][2](case)


def reference(case, inp=None):
    return FAMILIES[case.family][3](case, inp if inp is not None else inputs(case))


def route(case):
    return FAMILIES[case.family][1](case)


def compare(out, ref, bnd):
    """(every element inside its bound, worst err / bound); bnd None: bitwise
    equality of the values (an exact case: integers, so -0 cannot arise but at
    a ReLU of a negative, where the kernel's fmaxf gives +0 as the reference)."""
    o = out.double()
    if bnd is None:
        return bool(torch.equal(o, ref)), 0.0 if torch.equal(o, ref) else math.inf
    fin = torch.isfinite(ref)
    if not bool((torch.isfinite(o) == fin).all()):
        return False, math.inf
    err = torch.where(fin, (o - ref).abs(), torch.zeros((), dtype=F64))
    b = torch.where(fin, bnd, torch.ones((), dtype=F64))
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return not bool((err > b).any()), float(ratio.max())


# ------------------------------------------------------------------ routing
def split_log(lines):
    """(conv records, number of GEMM launch lines) of a launch's log lines."""
    conv, gemm = [], 0
    for ln in lines:
        f = ln.split()
        if not f:
            continue
        if f[0] == "conv":
            conv.append(dict(kv.split("=") for kv in f[1:]))
        elif f[0] in ("bf16", "f32"):
            gemm += 1
    return conv, gemm


def expected_line(c):
    """The fields of the one conv line a case on its special route must log."""
    tag = "bf16" if c.dtype == BF16 else "f32"
    if c.family == "stem_fwd":
        return dict(op="fwd", kernel=c.kernel, dtype=tag, n=c.n, h=c.h, w=c.w, c=3, k=c.k, r=7, s=7, grid=c.grid)
    if c.family == "stem_wgrad":
        return dict(op="bwd_filter", kernel=c.kernel, dtype=tag, n=c.n, h=c.h, w=c.w, c=3, k=64, r=7, s=7, grid=c.grid)
    n, h, w = n1_live(c)[0][:3]
    e = dict(op=c.op, kernel=c.kernel, dtype=tag, n=n, h=h, w=w, c=c.c, k=1, r=c.r, s=c.s, grid=c.grid)
    if len(c.levels) > 1:
        e.update(levels=len(n1_live(c)), pixels=n1_pixels(c))
    return e


def route_errors(c, lines):
    """Mismatches between the log lines of one launch of a case and its entry."""
    conv, gemm = split_log(lines)
    if c.kernel == "fallback":
        bad = []
        if conv:
            bad.append(f"a fallback case logged {conv}")
        if gemm < 1:
            bad.append("a fallback case logged no GEMM line")
        return bad
    if len(conv) != 1 or gemm:
        return [f"{len(conv)} conv lines and {gemm} GEMM lines, expected 1 and 0: {lines}"]
    exp = expected_line(c)
    got = conv[0]
    bad = [f"{k}={got.get(k)}, expected {v}" for k, v in exp.items() if str(got.get(k)) != str(v)]
    bad += [f"unexpected field {k}" for k in got if k not in exp]
    return bad


# ------------------------------------------------------------ GPU execution
class Out:
    """A flat output with OFF sentinel elements before and GUARD after."""

    def __init__(self, shape, dtype, dev, init=None):
        self.shape = tuple(shape)
        self.n = math.prod(self.shape)
        buf = torch.full((OFF + self.n + GUARD,), SENTINEL, dtype=dtype)
        if init is not None:
            buf[OFF:OFF + self.n] = init.reshape(-1).to(dtype)
        self.buf = buf.to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + OFF * self.buf.element_size()


def live(buf, shape):
    n = math.prod(shape)
    return buf[OFF:OFF + n].view(shape)


def guards_ok(buf, shape):
    n = math.prod(shape)
    g = torch.cat([buf[:OFF], buf[OFF + n:]])
    return bool((g == torch.tensor(SENTINEL, dtype=buf.dtype)).all()) and g.numel() == OFF + GUARD


def _dev(t, dev, shift=0):
    if t is None:
        return None
    if not shift:
        return t.contiguous().to(dev)
    b = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    b[shift:shift + t.numel()] = t.reshape(-1).to(dev)
    return b[shift:shift + t.numel()].view(t.shape)


def _conv_desc(L, c, n, h, w, cin, k, r, s, stride, act="none"):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.r, d.s = n, h, w, cin, k, r, s
    d.stride_h = d.stride_w = stride
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = c.pads
    d.dtype = L.BF16 if c.dtype == BF16 else L.F32
    d.act = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "leaky": L.ACT_LEAKY}[act]
    d.act_alpha = LEAKY
    return d


def _flip_of(w_rsc):
    """[r][s][c] (k = 1) -> the flipped IHWO copy w_flip[c][R-1-r][S-1-s][0]."""
    return w_rsc.flip(0, 1).permute(2, 0, 1).contiguous()


def run_stem_fwd(L, c, inp, dev):
    s = L.stream_ptr()
    x = _dev(inp["x"], dev, c.xshift)
    w, sc, bi, rs = (_dev(inp.get(k), dev) for k in ("w", "scale", "bias", "res"))
    y = Out((c.n, *c.out_hw, c.k), BF16, dev)
    d = _conv_desc(L, c, c.n, c.h, c.w, 3, c.k, 7, 7, 2, c.act)
    L.call("fpnmt_conv2d_fwd", d, x.data_ptr(), w.data_ptr(), L.ptr(sc), L.ptr(bi), L.ptr(rs), y.ptr, s)
    torch.cuda.synchronize()
    return {"y": y.buf}


def run_stem_wgrad(L, c, inp, dev, deferred=False):
    s = L.stream_ptr()
    x, dz, cs = _dev(inp["x"], dev), _dev(inp["dz"], dev), _dev(inp.get("col_scale"), dev)
    dw = Out((7, 7, 3, c.k), F32, dev, init=inp["old"])
    d = _conv_desc(L, c, c.n, c.h, c.w, 3, c.k, 7, 7, 2)
    with L.deferred_reductions(deferred):
        L.call("fpnmt_conv2d_bwd_filter", d, x.data_ptr(), dz.data_ptr(), L.ptr(cs), dw.ptr, s)
    torch.cuda.synchronize()
    return {"dw": dw.buf}


def run_n1(L, c, inp, dev, mask=None):
    """One launch; bwd_data with mask=False runs the plain form of a masked case."""
    s = L.stream_ptr()
    mask = c.mask if mask is None else mask
    xs = [_dev(t, dev) for t in inp["xs"]]
    dzs = [_dev(t, dev) for t in inp["dzs"]]
    ys = [_dev(t, dev) for t in inp["ys"]]
    rss = [_dev(t, dev) for t in inp["res"]]
    w = inp["w"]
    n0, h0, w0 = c.levels[0]
    d = _conv_desc(L, c, n0, h0, w0, c.c, 1, c.r, c.s, 1, c.act)
    lv = (L.ConvLevel * len(c.levels))()
    outs = {}
    for i, (n, h, w_) in enumerate(c.levels):
        lv[i].n, lv[i].h, lv[i].w = n, h, w_
    if c.op == "fwd":
        wt, sc, bi = _dev(w.reshape(-1), dev), _dev(inp.get("scale"), dev), _dev(inp.get("bias"), dev)
        for i, (n, h, w_) in enumerate(c.levels):
            ho, wo = c.out_hw(h, w_)
            lv[i].x = xs[i].data_ptr()
            if n > 0 and ho > 0 and wo > 0:
                o = Out((n, ho, wo, 1), c.dtype, dev)
                outs[f"y{i}"] = o.buf
                lv[i].y = o.ptr
                if c.res:
                    lv[i].residual = rss[i].data_ptr()
        if c.is_grouped:
            L.call("fpnmt_conv2d_fwd_grouped", d, len(c.levels), lv, wt.data_ptr(), L.ptr(sc), L.ptr(bi), s)
        else:
            L.call("fpnmt_conv2d_fwd", d, lv[0].x, wt.data_ptr(), L.ptr(sc), L.ptr(bi), lv[0].residual, lv[0].y, s)
    elif c.op == "bwd_data":
        wf = _dev(_flip_of(w).reshape(-1), dev)
        for i, (n, h, w_) in enumerate(c.levels):
            lv[i].x = dzs[i].data_ptr()
            if n * h * w_ > 0:
                o = Out((n, h, w_, c.c), c.dtype, dev)
                outs[f"dx{i}"] = o.buf
                lv[i].y = o.ptr
                if mask:
                    lv[i].residual = ys[i].data_ptr()
        if c.is_grouped and mask:
            L.call("fpnmt_conv2d_bwd_data_grouped_act", d, len(c.levels), lv, wf.data_ptr(), L.ACT_RELU, s)
        elif c.is_grouped:
            L.call("fpnmt_conv2d_bwd_data_grouped", d, len(c.levels), lv, wf.data_ptr(), 0, s)
        elif mask:
            L.call("fpnmt_conv2d_bwd_data_act", d, lv[0].x, wf.data_ptr(), lv[0].y, lv[0].residual, L.ACT_RELU, s)
        else:
            L.call("fpnmt_conv2d_bwd_data", d, lv[0].x, wf.data_ptr(), lv[0].y, 0, s)
    else:
        cs = _dev(inp.get("col_scale"), dev)
        dw = Out((c.r, c.s, c.c), F32, dev, init=inp["old"])
        outs["dw"] = dw.buf
        for i in range(len(c.levels)):
            lv[i].x, lv[i].dz = xs[i].data_ptr(), dzs[i].data_ptr()
        if c.is_grouped:
            L.call("fpnmt_conv2d_bwd_filter_grouped", d, len(c.levels), lv, L.ptr(cs), dw.ptr, s)
        else:
            L.call("fpnmt_conv2d_bwd_filter", d, lv[0].x, lv[0].dz, L.ptr(cs), dw.ptr, s)
    torch.cuda.synchronize()
    del xs, dzs, ys, rss
    return outs


def run_bneck(L, c, inp, dev):
    s = L.stream_ptr()
    x = bneck_x(c, inp).to(dev)
    t = {k: inp[k].contiguous().to(dev) for k in ("wa", "w3", "wc", "ba", "b3", "bc")}
    y = Out((c.n, c.hw, c.hw, c.c), BF16, dev)
    L.call("fpnmt_bottleneck_fwd", c.n, c.hw, c.hw, c.c, c.cm, x.data_ptr(), t["wa"].data_ptr(), t["ba"].data_ptr(),
           t["w3"].data_ptr(), t["b3"].data_ptr(), t["wc"].data_ptr(), t["bc"].data_ptr(), y.ptr, s)
    torch.cuda.synchronize()
    return {"y": y.buf}


def bneck_errors(L, dev):
    """{name: (status, y untouched)} of the error returns (res2 shape, n = 1)."""
    s = L.stream_ptr()
    c = BNECK[0]
    inp = bneck_inputs(c)
    x = bneck_x(c, inp).to(dev)
    t = {k: inp[k].contiguous().to(dev) for k in ("wa", "w3", "wc", "ba", "b3", "bc")}
    res = {}

    def go(name, *, shape=(56, 56, 256, 64), xp=None, yp="out", wa=None):
        y = Out((1, 56, 56, 256), BF16, dev)
        yptr = {"out": y.ptr, "x": x.data_ptr(), "odd": y.ptr + 2, "null": None}[yp]
        st = L.lib.fpnmt_bottleneck_fwd(1, *shape, x.data_ptr() if xp is None else xp,
                                        t["wa"].data_ptr() if wa is None else wa, t["ba"].data_ptr(), t["w3"].data_ptr(),
                                        t["b3"].data_ptr(), t["wc"].data_ptr(), t["bc"].data_ptr(), yptr, s)
        torch.cuda.synchronize()
        res[name] = (int(st), bool((y.buf == torch.tensor(SENTINEL, dtype=BF16)).all().item()))

    go("null_y", yp="null")
    go("null_wa", wa=0)
    go("y_is_x", yp="x")
    go("y_off_16B", yp="odd")
    go("x_off_16B", xp=x.data_ptr() + 2)
    go("shape_28x28x256", shape=(28, 28, 256, 64))
    go("shape_56x56x512", shape=(56, 56, 512, 128))
    return res


def run_wprep(L, c, inp, dev, batched_with=None):
    """The unbatched call; returns the two whole buffers (guards included)."""
    s = L.stream_ptr()
    r, sx, ci, k = c.shape
    w, sc = _dev(inp["w"], dev), _dev(inp.get("scale"), dev)
    ldf = wprep_ld(c)
    ld = ldf or r * sx * k
    o = Out((k * r * sx * ci,), c.dtype, dev) if c.ohwi else None
    f = Out((ci * ld,), c.dtype, dev) if c.flip else None
    L.call("fpnmt_weight_prep", w.data_ptr(), r, sx, ci, k, L.ptr(sc), L.BF16 if c.dtype == BF16 else L.F32,
           o.ptr if o else None, f.ptr if f else None, ldf, s)
    torch.cuda.synchronize()
    return {"ohwi": o.buf if o else None, "flip": f.buf if f else None}


def run_wprep_batched(L, cases, inps, dev, dtype, flip_shift):
    """Every case of one dtype as ONE fpnmt_weight_prep_batched launch. The
    flipped destinations start `flip_shift` elements into their buffers'
    live region (bf16: 0 keeps them 8-B aligned, 1 does not: the scalar path)."""
    s = L.stream_ptr()
    items = (L.WPrepItem * len(cases))()
    keep, outs, tiles = [], {}, 0
    for i, (c, inp) in enumerate(zip(cases, inps)):
        r, sx, ci, k = c.shape
        w, sc = _dev(inp["w"], dev), _dev(inp.get("scale"), dev)
        ld = wprep_ld(c) or r * sx * k
        o = Out((k * r * sx * ci,), dtype, dev) if c.ohwi else None
        f = Out((ci * ld + flip_shift,), dtype, dev) if c.flip else None
        keep += [w, sc, o, f]
        it = items[i]
        it.w_hwio, it.scale = w.data_ptr(), L.ptr(sc)
        it.w_ohwi = o.ptr if o else None
        it.w_flip = f.ptr + flip_shift * f.buf.element_size() if f else None
        it.r, it.s, it.c, it.k = r, sx, ci, k
        it.tile_start, it.ld_flip = tiles, wprep_ld(c)
        tiles += r * sx * cdiv(ci, 32) * cdiv(k, 32)
        outs[c.name] = {"ohwi": o.buf if o else None, "flip": f.buf if f else None}
    import ctypes
    tab = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(items), ctypes.sizeof(items))), dtype=torch.uint8).to(dev)
    L.call("fpnmt_weight_prep_batched", tab.data_ptr(), len(cases), tiles, L.BF16 if dtype == BF16 else L.F32, s)
    torch.cuda.synchronize()
    del keep
    return {k: {n: (None if b is None else b.cpu()) for n, b in v.items()} for k, v in outs.items()}


def _bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a if a[k] is not None) and a.keys() == b.keys()


def child_main(outdir):
    """Every case twice in this process (FPNMT_GEMM_LOG set by the parent):
    the first run's whole buffers, whether the second equals it bit for bit,
    the log lines of each launch, and the bitwise agreements. Any failed call
    or HIP error ends the process at once with a non-zero status."""
    log = os.environ["FPNMT_GEMM_LOG"]
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from fpnmt import _lib as L

    def lines():
        try:
            with open(log) as f:
                return f.read().splitlines()
        except FileNotFoundError:
            return []

    res = {}
    for c in CASES:
        inp = inputs(c)
        run = {"stem_fwd": run_stem_fwd, "stem_wgrad": run_stem_wgrad, "n1": run_n1, "bottleneck": run_bneck}[c.family]
        outs, logs = [], []
        for _ in range(2):
            before = len(lines())
            outs.append({k: v.cpu() for k, v in run(L, c, inp, dev).items()})
            logs.append(lines()[before:])
        rec = {"out": outs[0], "same": _bits_equal(outs[0], outs[1]), "log": logs}
        if c.family == "stem_wgrad":
            before = len(lines())
            dfr = {k: v.cpu() for k, v in run_stem_wgrad(L, c, inp, dev, deferred=True).items()}
            rec["deferred_same"] = _bits_equal(outs[0], dfr)
            rec["deferred_log"] = lines()[before:]
        if c.family == "n1" and c.mask:
            rec["plain"] = {k: v.cpu() for k, v in run_n1(L, c, inp, dev, mask=False).items()}
        res[c.name] = rec
        print(c.name, logs[0], flush=True)
    res["bneck_errors"] = bneck_errors(L, dev)
    for c in WPREP:
        inp = inputs(c)
        a = {k: (None if v is None else v.cpu()) for k, v in run_wprep(L, c, inp, dev).items()}
        b = {k: (None if v is None else v.cpu()) for k, v in run_wprep(L, c, inp, dev).items()}
        res[c.name] = {"out": a, "same": _bits_equal(a, b)}
    for dtype, tag in ((BF16, "bf16"), (F32, "f32")):
        cs = [c for c in WPREP if c.dtype == dtype]
        for shift in (0, 1):
            res[f"wprep_batched_{tag}_shift{shift}"] = run_wprep_batched(L, cs, [inputs(c) for c in cs], dev, dtype, shift)
    print("wprep done", flush=True)
    torch.save(res, os.path.join(outdir, "results.pt"))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "fpn-mt-image-captioning_amd"))
    child_main(sys.argv[1])

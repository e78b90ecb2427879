"""The bounds of the spatial-kernel case table (tests/spatial_kernel_cases.py)
can fail.

No GPU. `Emu` restates the pooling, FPN top-down and spatial-softmax kernels
in torch on the CPU in the kernels' own arithmetic and order: the pool
forward's taps in (r, q) order, the gather backward's windows in ascending
(oh, ow) order, the tile form's four neighbour windows and 2x2 block, the FPN
children in (y, x) order from the restated nn_children with the intermediate
roundings to the storage dtype, the softmax's 256-thread strides, wave
butterfly and four-wave sums (fp32 forward, fp64 backward). The large cases
are emulated at a reduced shape (`small`). Checked:

  * the unmutated emulation is inside the bound of every case, dtype and label,
    and its outputs that must agree bit for bit do;
  * each mutation below puts at least one element of the named label outside
    its bound;
  * the restated route predicates, grids and chunk rule give the geometry every
    case records, every branch is named by a case, nn_children equals brute
    force for every (in, out) up to 96 and for the table's pairs, and the fp32
    index map differs from the exact rational on the `fp32_index` case's pair;
  * the correctly rounded fp64 reference passes every bound, and halving the
    bf16 store term rejects it.

Mutations: last_max (the last maximum on ties), pad_wins (a padded tap
competes as 0), am255_as_0 (the argmax starts at tap 0 and only `>` moves it),
gather_drop / gather_twice and tile_drop / tile_twice (a window missing from,
or twice in, the backward sum), tile_neighbour (the tile form reads the window
to the right for the one to the left), pt_pl_swapped, relu6_le, leaky_side,
exact_index (the rational map on 14 -> 23), children_lo / children_hi
(nn_children off by one), no_p4_round / no_dp4_round (no intermediate rounding
of P4m / of the d_p4m total, bf16), assign_lat5 (`=` for `+=`), no_max,
chunk_sum (the softmax sum over the chunk), a_other_image, da_fp32, sada_fp32,
no_s (d_score without - S).

Three mutations one might ask for cannot be observed through any entry point
and are therefore proved dead instead (`test_dead_branches_are_dead`): the
`in - 1` clamp of nn_src binds for no (in, out) up to 96 nor for the table's
larger sizes (the unclamped fp32 index stays below `in`), and a leaky slope applied per window equals the slope
applied once, because the entry point refuses leaky with overlapping windows
(at most one window per input; the refusal is asserted on the GPU). Likewise
an argmax of 255 never reaches a backward sum: a window without a valid tap
covers no input element.
"""
import dataclasses

import numpy as np
import pytest
import torch

import spatial_kernel_cases as S

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


@pytest.fixture(autouse=True, scope="module")
def _single_thread():
    """One thread starts no OpenMP pool (tests that fork later would hang in a child that inherits one)."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


def _butterfly(v):
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def block_sum(v):
    """Sum over the last dimension as a 256-thread block does it: threads
    striding by 256, the butterfly per wave, red[0] + red[1] + red[2] + red[3]."""
    n = v.shape[-1]
    pad = torch.zeros(*v.shape[:-1], S.cdiv(n, 256) * 256, dtype=v.dtype)
    pad[..., :n] = v
    pad = pad.view(*v.shape[:-1], -1, 256)
    s = torch.zeros(*v.shape[:-1], 256, dtype=v.dtype)
    for k in range(pad.shape[-2]):
        s = s + pad[..., k, :]
    w = _butterfly(s.view(*v.shape[:-1], 4, 64))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def wave_sum(v):
    """Sum over the last dimension as one wave does it: lanes striding by 64, the butterfly."""
    n = v.shape[-1]
    pad = torch.zeros(*v.shape[:-1], S.cdiv(n, 64) * 64, dtype=v.dtype)
    pad[..., :n] = v
    pad = pad.view(*v.shape[:-1], -1, 64)
    s = torch.zeros(*v.shape[:-1], 64, dtype=v.dtype)
    for k in range(pad.shape[-2]):
        s = s + pad[..., k, :]
    return _butterfly(s)


def _shift(t, dy, dx, fill):
    """t[:, oh + dy, ow + dx] with `fill` outside."""
    n, ho, wo, c = t.shape
    out = torch.full_like(t, fill)
    ys, xs = slice(max(0, -dy), ho - max(0, dy)), slice(max(0, -dx), wo - max(0, dx))
    yd, xd = slice(max(0, dy), ho - max(0, -dy)), slice(max(0, dx), wo - max(0, -dx))
    out[:, ys, xs] = t[:, yd, xd]
    return out


class Emu:
    def __init__(self, mut=None):
        self.mut = mut

    # ---- max pool
    def _pads(self, case):
        return dataclasses.replace(case, pt=case.pl, pl=case.pt) if self.mut == "pt_pl_swapped" else case

    def pool_fwd(self, case, x, want_am, off):
        k = self._pads(case)
        xf = x.float()
        m = torch.full((k.n, k.ho, k.wo, k.c), -np.inf)
        am = torch.full((k.n, k.ho, k.wo, k.c), 0 if self.mut == "am255_as_0" else 255, dtype=torch.int64)
        for tap, ih, iw, valid in S._taps(k, "cpu"):
            v = xf[:, ih][:, :, iw]
            if self.mut == "pad_wins":
                v, valid = torch.where(valid, v, torch.zeros(())), torch.ones_like(valid)
            better = v >= m if self.mut == "last_max" else v > m
            take = valid & (better if self.mut == "am255_as_0" else better | (am == 255))
            m, am = torch.where(take, v, m), torch.where(take, tap, am)
        return m.to(x.dtype), am.to(torch.uint8) if want_am else None

    def _mask(self, xact, act, alpha):
        v = xact.float()
        if act == "relu6":
            return ((v > 0) & ((v <= 6) if self.mut == "relu6_le" else (v < 6))).float()
        if act == "leaky":
            side = v < 0 if self.mut == "leaky_side" else v > 0
            return torch.where(side, 1.0, S.f32(alpha)).float()
        return (v > 0).float()

    def pool_bwd(self, case, dtype, x, am, dy, off, xact=None, act=None, alpha=0.0):
        k = self._pads(case)
        route = S.pool_bwd_route(case, off == 0, am is not None)
        if route == "zero_fill":
            return torch.zeros((k.n, k.h, k.w, k.c), dtype=dtype)
        if am is None:
            _, am = self.pool_fwd(case, x, True, off)
        aml, dyf = am.long(), dy.float()
        if route == "tile":
            dx = torch.full((k.n, k.h, k.w, k.c), float("nan"))
            for dr in (0, 1):
                for dc in (0, 1):
                    g = torch.zeros((k.n, k.ho, k.wo, k.c))
                    wins = [(a, b) for a in (-1, 0) for b in (-1, 0)]
                    if self.mut == "tile_drop":
                        wins = wins[1:]
                    if self.mut == "tile_twice":
                        wins = wins + [(0, 0)]
                    for dy_, dx_ in wins:
                        r, q = dr - 2 * dy_, dc - 2 * dx_
                        if not (0 <= r < 3 and 0 <= q < 3):
                            continue
                        sx = 1 if (self.mut == "tile_neighbour" and dx_ == -1) else dx_
                        hit = _shift(aml, dy_, sx, 255) == r * 3 + q
                        g = torch.where(hit, g + _shift(dyf, dy_, sx, 0.0), g)
                    ih, iw = 2 * torch.arange(k.ho) - k.pt + dr, 2 * torch.arange(k.wo) - k.pl + dc
                    vh, vw = (ih >= 0) & (ih < k.h), (iw >= 0) & (iw < k.w)
                    sub = g[:, vh][:, :, vw]
                    dx[:, ih[vh][:, None], iw[vw][None, :]] = sub
        else:
            dx = torch.zeros((k.n, k.h, k.w, k.c))
            # ascending (oh, ow) at a fixed input element is descending (r, q)
            taps = [(r, q) for r in reversed(range(k.kh)) for q in reversed(range(k.kw))]
            if self.mut == "gather_drop":
                taps = taps[:-1]
            if self.mut == "gather_twice":
                taps = taps + [taps[0]]
            for r, q in taps:
                sl = S._win_slices(k, r, q)
                if sl is None:
                    continue
                so, sw_, si, sj = sl
                hit = aml[:, so, sw_] == r * k.kw + q
                dx[:, si, sj] = torch.where(hit, dx[:, si, sj] + dyf[:, so, sw_], dx[:, si, sj])
        if act is not None:
            dx = dx * self._mask(xact, act, alpha)
        return dx.to(dtype)

    def pool_bwd_act(self, case, am, dy, xact, act, alpha, off):
        return self.pool_bwd(case, dy.dtype, None, am, dy, off, xact, act, alpha)

    # ---- FPN
    def _src(self, out, inp):
        fn = S.nn_src_exact if self.mut == "exact_index" else S.nn_src_f32
        return torch.from_numpy(fn(out, inp)) if out else torch.zeros(0, dtype=torch.int64)

    def fpn_fwd(self, case, l5, l4, l3):
        h5, w5, h4, w4, h3, w3 = case.sizes
        dt = l5.dtype
        iy, ix = self._src(h4, h5), self._src(w4, w5)
        s4 = l4.float() + l5.float()[:, iy][:, :, ix]
        p4m = s4.to(dt)
        if l3 is None:
            return p4m, None
        jy, jx = self._src(h3, h4), self._src(w3, w4)
        p4 = s4 if self.mut == "no_p4_round" else p4m.float()
        return p4m, (l3.float() + p4[:, jy][:, :, jx]).to(dt)

    def _children(self, inp, out):
        t = S.children_table(inp, out)
        if self.mut == "children_lo":
            t[:, 0] = torch.minimum(t[:, 0] + 1, t[:, 1])
        if self.mut == "children_hi":
            t[:, 1] = torch.where(t[:, 1] > t[:, 0], (t[:, 1] + 1).clamp_max(out), t[:, 1])
        return t

    @staticmethod
    def _gather_sum(acc, t, ty, tx):
        """acc[y, x] += t[yy, xx] over yy in ty[y], xx in tx[x], yy outer, in fp32."""
        ly, lx = int((ty[:, 1] - ty[:, 0]).max()), int((tx[:, 1] - tx[:, 0]).max())
        for oy in range(ly):
            for ox in range(lx):
                yy, xx = ty[:, 0] + oy, tx[:, 0] + ox
                valid = (yy < ty[:, 1])[:, None] & (xx < tx[:, 1])[None, :]
                v = t[:, yy.clamp_max(t.shape[1] - 1)][:, :, xx.clamp_max(t.shape[2] - 1)]
                acc = torch.where(valid[None, :, :, None], acc + v, acc)
        return acc

    def fpn_bwd(self, case, dp4, dp3, dl5_0, acc5):
        h5, w5, h4, w4, h3, w3 = case.sizes
        dt = dp4.dtype
        s4 = dp4.float()
        if dp3 is not None:
            s4 = self._gather_sum(s4, dp3.float(), self._children(h4, h3), self._children(w4, w3))
        dl4 = s4.to(dt)
        t = s4 if self.mut == "no_dp4_round" else dl4.float()
        acc = self._gather_sum(torch.zeros(dl5_0.shape), t, self._children(h5, h4), self._children(w5, w4))
        if acc5 and self.mut != "assign_lat5":
            acc = acc + dl5_0.float()
        return dl4, acc.to(dt)

    # ---- spatial softmax
    def ssm_fwd(self, case, score, hs):
        hw, c = case.hw, case.c
        x = score.float()
        m = torch.zeros(x.shape[0], 1) if self.mut == "no_max" else x.max(1, keepdim=True).values
        e = torch.exp(x - m)
        if self.mut == "chunk_sum":
            chunks, chunk = S.ssm_chunks(hw, c)
            pad = torch.zeros(x.shape[0], chunks * chunk)
            pad[:, :hw] = e
            s = block_sum(pad.view(-1, chunks, chunk)).repeat_interleave(chunk, 1)[:, :hw]
        else:
            s = block_sum(e)[:, None]
        a = e / s
        ac = a.roll(1, 0) if self.mut == "a_other_image" else a
        return (ac[:, :, None] * hs.float()).to(score.dtype), a

    def ssm_bwd(self, case, a, hs, dctx):
        dt = hs.dtype
        g = dctx.float()
        d_hs = (a[:, :, None] * g).to(dt)
        if self.mut == "da_fp32":
            da = wave_sum(g * hs.float()).double()
        else:
            da = wave_sum(g.double() * hs.double())
        if self.mut == "sada_fp32":
            s = block_sum(a * da.float()).double()[:, None]
        else:
            s = block_sum(a.double() * da)[:, None]
        if self.mut == "no_s":
            s = torch.zeros_like(s)
        return (a.double() * (da - s)).float().to(dt), d_hs, da


SUITES = {
    "pool": lambda name, dtype, impl: S.pool_suite(S.POOL_BY_NAME[name], dtype, impl, emulate=True),
    "fpn": lambda name, dtype, impl: S.fpn_suite(S.FPN_BY_NAME[name], dtype, impl, emulate=True),
    "ssm": lambda name, dtype, impl: S.ssm_suite(S.SSM_BY_NAME[name], dtype, impl, emulate=True),
}
ALL_CASES = ([("pool", c.name) for c in S.POOL_CASES] + [("fpn", c.name) for c in S.FPN_CASES]
             + [("ssm", c.name) for c in S.SSM_CASES])


def _dtypes(kind, name):
    return S.FPN_BY_NAME[name].dtypes if kind == "fpn" else (F32, BF16)


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------ clean emulation
@pytest.mark.parametrize("kind,name", ALL_CASES, ids=[f"{k}-{n}" for k, n in ALL_CASES])
def test_emulation_inside_bound(kind, name):
    for dtype in _dtypes(kind, name):
        rows, pairs = SUITES[kind](name, dtype, Emu())
        ratios, bad = S.worst(rows)
        top = max(ratios, key=ratios.get)
        print(kind, name, dtype, f"worst {ratios[top]:.3f} at {top}")
        assert not bad, (dtype, {k: ratios[k] for k in bad})
        for label, a, b in pairs:
            assert torch.equal(_bits(a), _bits(b)), (dtype, label)


def test_suites_carry_every_label():
    fam = lambda rows: {r[0].split("[")[0] for r in rows}
    assert fam(SUITES["pool"]("same_8x10", BF16, Emu())[0]) == {"pool.y", "pool.argmax", "pool.dx", "pool.dx_act"}
    assert fam(SUITES["fpn"]("square_7_14_28", BF16, Emu())[0]) == {"fpn.p4m", "fpn.p3m", "fpn.d_lat4", "fpn.d_lat5"}
    assert fam(SUITES["fpn"]("upsample_up", F32, Emu())[0]) == {"fpn.p4m", "fpn.d_lat4", "fpn.d_lat5"}
    assert fam(SUITES["ssm"]("hw15_c5", F32, Emu())[0]) == {"ssm.a", "ssm.ctx", "ssm.d_hs", "ssm.da", "ssm.d_score"}


def test_fpn_adjoint_identity_is_exact():
    for name in ("ragged_4x5", "fp32_index", "upsample_down"):
        lhs, rhs = S.fpn_adjoint(S.FPN_BY_NAME[name], Emu())
        assert lhs == rhs and lhs != 0.0, (name, lhs, rhs)


def test_exact_outputs_of_the_one_position_softmax():
    rows, _ = SUITES["ssm"]("hw1", BF16, Emu())
    got = {r[0]: r[1] for r in rows}
    assert bool((got["ssm.a"] == 1).all()) and bool((got["ssm.d_score"] == 0).all())


# ------------------------------------------------------------------ mutations
# (mutation, kind, case, dtypes, label families of which each must leave its bound)
BOTH = (F32, BF16)
MUTATIONS = [
    ("last_max", "pool", "same_8x10", BOTH, ("pool.argmax[ties", "pool.dx[ties")),
    ("last_max", "pool", "k3s1_6x5", BOTH, ("pool.argmax[ties", "pool.dx[ties,gather8,recompute")),
    ("pad_wins", "pool", "same_9x7", BOTH, ("pool.y[inf", "pool.argmax[randn")),
    ("am255_as_0", "pool", "oversize_k2", BOTH, ("pool.argmax",)),
    ("am255_as_0", "pool", "oversize_tile", BOTH, ("pool.argmax",)),
    ("am255_as_0", "pool", "same_9x7", BOTH, ("pool.argmax[inf",)),
    ("gather_drop", "pool", "k3s1_6x5", BOTH, ("pool.dx[ties,gather8,argmax", "pool.dx[randn,gather8,recompute")),
    ("gather_drop", "pool", "same_8x10", BOTH, ("pool.dx[ties,gather1",)),
    ("gather_twice", "pool", "k3s1_6x5", BOTH, ("pool.dx[ties,gather8,argmax",)),
    ("gather_twice", "pool", "c6", BOTH, ("pool.dx[ties,gather1,argmax", "pool.dx_act[ties,gather1,relu]")),
    ("tile_drop", "pool", "same_8x10", BOTH, ("pool.dx[ties,tile", "pool.dx_act[ties,tile,relu6")),
    ("tile_twice", "pool", "same_9x7", BOTH, ("pool.dx[ties,tile",)),
    ("tile_neighbour", "pool", "same_8x10", BOTH, ("pool.dx[ties,tile", "pool.dx[randn,tile")),
    ("tile_neighbour", "pool", "oversize_tile", BOTH, ("pool.dx[ties,tile",)),
    ("pt_pl_swapped", "pool", "same_5x6", BOTH, ("pool.y[randn", "pool.argmax[ties", "pool.dx[randn,tile")),
    ("relu6_le", "pool", "same_8x10", BOTH, ("pool.dx_act[ties,tile,relu6", "pool.dx_act[randn,tile,relu6")),
    ("relu6_le", "pool", "k3s1_6x5", BOTH, ("pool.dx_act[ties,gather8,relu6",)),
    ("leaky_side", "pool", "valid_7x7", BOTH, ("pool.dx_act[ties,gather8,leaky",)),
    ("exact_index", "fpn", "fp32_index", BOTH, ("fpn.p4m",)),  # p3m is judged from the stored p4m
    ("children_lo", "fpn", "ragged_4x5", BOTH, ("fpn.d_lat4", "fpn.d_lat5")),
    ("children_lo", "fpn", "fp32_index", BOTH, ("fpn.d_lat4", "fpn.d_lat5")),
    ("children_hi", "fpn", "ragged_4x5", BOTH, ("fpn.d_lat4", "fpn.d_lat5")),
    ("children_hi", "fpn", "upsample_down", BOTH, ("fpn.d_lat5",)),
    ("no_p4_round", "fpn", "square_7_14_28", (BF16,), ("fpn.p3m[c8,cancel", "fpn.p3m[c24,cancel")),
    ("no_dp4_round", "fpn", "square_7_14_28", (BF16,), ("fpn.d_lat5[c8,cancel,acc0", "fpn.d_lat5[c24,cancel,acc1")),
    ("assign_lat5", "fpn", "ragged_4x5", BOTH, ("fpn.d_lat5[c24,randn,acc1", "fpn.d_lat5[c24,ints,acc1")),
    ("assign_lat5", "fpn", "upsample_down", BOTH, ("fpn.d_lat5[c24,ints,acc1",)),
    ("no_max", "ssm", "pm80", BOTH, ("ssm.a", "ssm.ctx")),
    ("chunk_sum", "ssm", "hw784_c32", BOTH, ("ssm.a",)),
    ("chunk_sum", "ssm", "chunks_clamped", BOTH, ("ssm.a",)),
    ("a_other_image", "ssm", "hw15_c5", BOTH, ("ssm.ctx",)),
    ("da_fp32", "ssm", "peaked_gap14", BOTH, ("ssm.da",)),
    ("da_fp32", "ssm", "hw784_c32", BOTH, ("ssm.da",)),
    ("sada_fp32", "ssm", "peaked_gap14", BOTH, ("ssm.d_score",)),
    ("sada_fp32", "ssm", "peaked_gap9", (F32,), ("ssm.d_score",)),  # bf16: 2^-8 e^-9 covers an fp32 sum
    ("no_s", "ssm", "hw300_c3", BOTH, ("ssm.d_score",)),
]
ALL_MUTATIONS = {"last_max", "pad_wins", "am255_as_0", "gather_drop", "gather_twice", "tile_drop", "tile_twice",
                 "tile_neighbour", "pt_pl_swapped", "relu6_le", "leaky_side", "exact_index", "children_lo",
                 "children_hi", "no_p4_round", "no_dp4_round", "assign_lat5", "no_max", "chunk_sum", "a_other_image",
                 "da_fp32", "sada_fp32", "no_s"}


@pytest.mark.parametrize("mut,kind,name,dtypes,labels", MUTATIONS, ids=[f"{m[0]}-{m[2]}" for m in MUTATIONS])
def test_bound_rejects_mutation(mut, kind, name, dtypes, labels):
    for dtype in dtypes:
        ratios, bad = S.worst(SUITES[kind](name, dtype, Emu(mut))[0])
        for want in labels:
            hit = [b for b in bad if b.startswith(want)]
            near = {k: round(v, 3) for k, v in ratios.items() if k.startswith(want)}
            assert hit, f"{mut} passes the bound of {want} on {name} {dtype}: worst err / bound {near}"


def test_every_mutation_is_listed():
    assert {m[0] for m in MUTATIONS} == ALL_MUTATIONS


def test_dead_branches_are_dead():
    """The in - 1 clamp never binds; 255 never reaches a backward sum; leaky sees at most one window."""
    for i in list(range(1, 97)) + [230, 250, 460, 1000]:
        for o in list(range(1, 97)) + [460, 920, 1000]:
            d = np.arange(o, dtype=np.float32)
            s = np.floor((d + np.float32(0.5)) * (np.float32(i) / np.float32(o)))
            assert s.max() <= i - 1, (i, o)
    for case in S.POOL_CASES:
        case = S.pool_small(case)
        if case.ho <= 0:
            continue
        for data in case.datas:
            inp = S.pool_inputs(case, F32, data)
            _, am = S.pool_fwd_ref(case, inp["x"])
            _, _, k = S.pool_bwd_ref(case, am, inp["dy"], F32)
            none_valid = am == 255
            if case.name.startswith("oversize"):
                assert bool(none_valid.any())
            # windows routed in the backward = windows with a valid tap
            assert int(k.sum()) == int((~none_valid).sum()), case.name
            if "leaky" in case.acts:
                assert float(k.max()) <= 1 and case.kh <= case.sh and case.kw <= case.sw


# ------------------------------------------------------------------- geometry
def test_restatements_match_the_recorded_geometry():
    for c in S.POOL_CASES:
        for route, with_am, off in c.routes:
            assert S.pool_bwd_route(c, off == 0, with_am) == route, (c.name, route)
        assert S.pool_loops(c) == c.loops, c.name
        assert c.ho <= 0 or (c.n * c.h * c.w * c.c) < 2 ** 31
    for c in S.FPN_CASES:
        h5, w5, h4, w4, h3, w3 = c.sizes
        for dt in c.dtypes:
            for ch in S.fpn_cs(c, dt):
                cg = ch // S.FPN_VN[dt]
                assert (S.fpn_loop(c.n, cg, h3, w3, h4, w4), S.fpn_loop(c.n, cg, h4, w4, h5, w5)) == c.loops, c.name
    for c in S.SSM_CASES:
        assert (*S.ssm_chunks(c.hw, c.c), S.ssm_bwd_loop(c.n, c.hw)) == c.geom, c.name


def test_table_names_every_branch():
    P, Fp, M = S.POOL_BY_NAME, S.FPN_BY_NAME, S.SSM_BY_NAME
    routes = {(r, am, off > 0) for c in S.POOL_CASES for r, am, off in c.routes}
    # 1. every backward route: tile, gather8 with argmax and with recompute, gather1 by alignment and by
    #    channel count (with recompute too), zero_fill
    assert {("tile", True, False), ("gather8", True, False), ("gather8", False, False), ("gather1", True, True),
            ("gather1", True, False), ("gather1", False, False), ("zero_fill", True, False)} <= routes
    assert P["c6"].c % 8 and P["same_8x10"].c % 8 == 0 and ("gather1", True, 1) in P["same_8x10"].routes
    # 2. the three routes on the same data, with both pad parities
    for n in ("same_8x10", "same_9x7", "oversize_tile"):
        assert [r for r, _, _ in P[n].routes] == ["tile", "gather8", "gather1"]
    assert {(P[n].pt, P[n].pl) for n in ("same_8x10", "same_9x7", "same_5x6")} == {(0, 0), (1, 1), (1, 0)}
    # 3. windows without a valid tap, uncovered inputs (stride > kernel, 'valid' remainder), nine windows per input
    assert 2 * (P["oversize_k2"].ho - 1) >= P["oversize_k2"].h and 2 * (P["oversize_tile"].ho - 1) >= P["oversize_tile"].h
    assert P["k2x3_s3x2"].sh > P["k2x3_s3x2"].kh and P["valid_7x7"].h % 2 == 1
    for n in ("k2x3_s3x2", "valid_7x7"):
        inp = S.pool_inputs(P[n], F32, "ties")
        k = S.pool_bwd_ref(P[n], S.pool_fwd_ref(P[n], inp["x"])[1], inp["dy"], F32)[2]
        assert bool((k.sum(3) == 0).any()), n  # whole pixels no window covers
    assert (P["k3s1_6x5"].kh, P["k3s1_6x5"].sh) == (3, 1)
    # 4. the data: ties, -inf over whole windows and single taps, exact 0.0 and 6.0 under the activations
    inp = S.pool_inputs(P["same_8x10"], BF16, "inf")
    y, am = S.pool_fwd_ref(P["same_8x10"], inp["x"])
    assert bool(torch.isinf(y).any()) and bool((torch.isinf(inp["x"]).float().mean() < 0.5))
    assert not bool((am == 255).any())  # an all -inf window still names its first valid tap
    xa = inp["xact"]
    assert int((xa == 0).sum()) > 20 and int((xa == 6).sum()) > 20 and bool((xa < 0).any()) and bool((xa > 6).any())
    assert {a for c in S.POOL_CASES for a in c.acts} == {"relu", "relu6", "leaky"}
    assert {P[c].acts and S.pool_bwd_route(P[c]) for c in ("same_8x10", "c6", "k3s1_6x5")} == {"tile", "gather1", "gather8"}
    # 5. the grid-stride loops of the pool (scalar route and VN = 8), forward and backward
    assert P["loop_840"].loops == (True, True) and P["loop_840"].c % 8
    assert P["loop_840_c24"].loops == (True, True) and S.pool_bwd_route(P["loop_840_c24"]) == "gather8"
    # 6. FPN: non-square, the fp32 pair, the upsample form up and down, childless sources, both loops, cancel data
    assert Fp["ragged_4x5"].sizes[0] != Fp["ragged_4x5"].sizes[1]
    assert (14, 23) in S.differing_pairs(32) and Fp["fp32_index"].sizes[1:4:2] == (14, 23)
    assert Fp["upsample_up"].sizes[4:] == (0, 0) and Fp["upsample_down"].sizes[4:] == (0, 0)
    t = S.children_table(7, 4)
    assert bool((t[:, 0] == t[:, 1]).any())  # childless sources in upsample_down
    assert Fp["loop_fwd"].loops == (True, False) and Fp["loop_bwd"].loops == (False, True)
    assert "cancel" in Fp["square_7_14_28"].datas
    assert S.FPN_CS == {BF16: (8, 24), F32: (4, 24)}
    # 7. softmax: a short last chunk, the clamp, hw < 256, c % 64, hw = 1, -inf, +-80, peaked, the row loop
    chunks, chunk = S.ssm_chunks(784, 32)
    assert chunks == 3 and 784 - 2 * chunk == 260 < chunk
    assert M["chunks_clamped"].hw * M["chunks_clamped"].c // 8192 > M["chunks_clamped"].hw == M["chunks_clamped"].geom[0]
    assert M["hw15_c5"].hw < 256 and M["hw15_c5"].c % 64 and M["hw300_c3"].hw % 256 and M["hw1"].hw == 1
    assert M["bwd_row_loop"].geom[2] and M["bwd_row_loop"].n * M["bwd_row_loop"].hw > 32768
    sc = S.ssm_inputs(M["neg_inf"], F32)["score"]
    assert bool(torch.isinf(sc).any()) and bool(torch.isfinite(sc).any(1).all())
    sc = S.ssm_inputs(M["pm80"], F32)["score"]
    assert float(sc.max(1).values.min()) > 88.8 and float(sc.min()) < -80 and float(sc.abs().min()) >= 80
    for gap in (4, 9, 14):
        for dt in (F32, BF16):
            sc = S.ssm_inputs(M[f"peaked_gap{gap}"], dt)["score"].double()
            top = sc.topk(2, 1).values
            assert bool(((top[:, 0] - top[:, 1]) >= gap - 1).all())
    assert len(set(S.ssm_inputs(M["all_equal"], BF16)["score"].flatten().tolist())) == 1


def test_nn_children_equals_brute_force():
    pairs = [(i, o) for i in range(1, 97) for o in range(1, 97)]
    pairs += [(a, b) for c in S.FPN_CASES for s in (c.sizes, c.small) if s
              for a, b in ((s[0], s[2]), (s[1], s[3]), (s[2], s[4]), (s[3], s[5])) if b]
    for i, o in pairs:
        src = S.nn_src_f32(o, i)
        for s in range(i):
            assert S.nn_children(s, i, o, src) == S.children_brute(s, i, o), (s, i, o)


def test_fp32_index_map_differs_from_the_exact_rational():
    diff = S.differing_pairs(96)
    assert len(diff) == 132 and {(14, 23), (8, 41), (4, 41), (6, 37)} <= diff
    a, b = S.nn_src_f32(23, 14), S.nn_src_exact(23, 14)
    assert (int(a[11]), int(b[11])) == (6, 7) and int((a != b).sum()) == 1


# -------------------------------------------------- the reference and the store
STORE_CASES = [("pool", "k3s1_6x5"), ("pool", "valid_7x7"), ("fpn", "ragged_4x5"), ("fpn", "upsample_up"),
               ("ssm", "hw784_c32"), ("ssm", "hw15_c5")]


@pytest.mark.parametrize("kind,name", STORE_CASES, ids=[f"{k}-{n}" for k, n in STORE_CASES])
def test_rounded_reference_passes_and_half_the_store_term_rejects_it(kind, name, monkeypatch):
    """Every output replaced by its fp64 reference rounded to the output's
    dtype is inside every bound; with the bf16 store term halved (2^-9) the
    correctly rounded reference itself is rejected: the store term is not
    slack."""
    ideal = lambda rows: [(label, ref.to(got.dtype), ref, bnd) for label, got, ref, bnd in rows]
    for dtype in _dtypes(kind, name):
        ratios, bad = S.worst(ideal(SUITES[kind](name, dtype, Emu())[0]))
        assert not bad, (dtype, bad)
    monkeypatch.setattr(S, "store_u", lambda dt: 2.0 ** -9 if dt == BF16 else S.U)
    rows = [r for r in ideal(SUITES[kind](name, BF16, Emu())[0]) if r[1].dtype == BF16]
    ratios, bad = S.worst(rows)
    assert rows and bad, "the rounded reference passes with half the store term"

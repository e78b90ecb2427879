"""The bounds of the BatchNorm / depthwise case table (tests/bn_dw_cases.py)
can fail.

No GPU. `Emu` restates every kernel of csrc/mobilenet.hip in torch on the
CPU in the kernel's own arithmetic: fp32 element math (torch.rsqrt for
rsqrtf), the col_grid partition into row lanes and chunks, fp64 (BatchNorm)
or fp32 (depthwise filter gradient) partial sums, the four-lane fixed-order
final sum, `+=` into the gradients, the grid-stride loop. Checked:

  * the unmutated emulation is inside the bound of every case, dtype,
    activation and residual form (the two grid-stride cases at a reduced row
    count under a reduced grid cap, so that their loop still wraps);
  * each mutation below puts at least one element outside the bound on the
    case meant to catch it;
  * the col_grid restatement gives the geometry every case records, and each
    geometry branch the kernels have is named by a case.

Mutations: drop_chunk, drop_row_lane, drop_last_chunk (the short one),
drop_group (an 8-channel group; on gx2 the lone group of the second column
block), first_four_chunks (the final kernel's k += 4 loop run once),
naive_f32 (statistics as fp32 E[x^2] - E[x]^2), bessel_batch (Bessel's factor
on the batch variance), no_bessel_moving, drop_sgx (dx without the
sum g xhat term), inv_n_one_rank (sync: 1 / n of one rank's rows),
assign_grads (= instead of +=), drop_tap, swap_pads (pad_t and pad_l
swapped), no_phase (dw_bwd_data without the stride-phase test), acc_index
(the filter gradient's accumulator read at r * kw + s), loop_once (the
grid-stride loop body run once: the rest stays at the sentinel).
"""
import pytest
import torch

import bn_dw_cases as C

F32, F64 = torch.float32, torch.float64
SMALL_CAP = 8  # grid cap of the reduced wrap cases: 8 * 256 work items


@pytest.fixture(autouse=True, scope="module")
def _single_thread():
    """The tensors here are large enough for torch to start its OpenMP pool;
    tests that fork afterwards (tests/test_dist_gloo.py) would hang in a child
    that inherits a started pool. One thread starts none."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


def _partials(vals, c, mut, group=1):
    """part[chunk][c]: per-lane sums (index_add in the dtype of vals), then the
    block's lanes in order."""
    rows = vals.shape[0]
    gx, gy, rpc, GT, RL = C.col_grid(rows, c)
    r = torch.arange(rows)
    chunk, lane = r // rpc, (r % rpc) % RL
    if mut == "drop_row_lane":
        vals = vals * (lane != min(RL, rpc) - 1).to(vals.dtype)[:, None]
    lanes = torch.zeros(gy * RL, c, dtype=vals.dtype).index_add_(0, chunk * RL + lane, vals).view(gy, RL, c)
    part = lanes[:, 0].clone()
    for q in range(1, RL):
        part += lanes[:, q]
    if mut == "drop_chunk":
        part[gy // 2] = 0
    if mut == "drop_last_chunk":
        part[gy - 1] = 0
    if mut == "drop_group":
        part[:, group * 8:group * 8 + 8] = 0
    return part


def _final4(part, mut):
    """The *_final_kernels: lane kl sums chunks kl, kl + 4, ...; then ((0 + 1) + 2) + 3."""
    acc = []
    for kl in range(4):
        a = torch.zeros(part.shape[1], dtype=part.dtype)
        for k in range(kl, part.shape[0], 4):
            a = a + part[k]
            if mut == "first_four_chunks":
                break
        acc.append(a)
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def _mask(y, act):
    return ((y.float() > 0) & (y.float() < 6)).float() if act == "relu6" else 1.0


def _loop_once(out, cap):
    flat = out.reshape(-1)
    flat[cap * 256 * 8:] = C.SENTINEL
    return out


class Emu:
    def __init__(self, mut=None, group=1, cap=C.GRID_CAP):
        self.mut, self.group, self.cap = mut, group, cap
        self.eps = torch.tensor(C.EPS, dtype=F32)

    # ---- BatchNorm
    def _shifted(self, x):
        K = x[0].double()
        d = x.double() - K
        c = x.shape[1]
        return K, _final4(_partials(d, c, self.mut, self.group), self.mut), \
            _final4(_partials(d * d, c, self.mut, self.group), self.mut)

    def _moving(self, m, v64, n, mm, mv, momentum):
        if mm is None:
            return None, None
        unb = (v64 * (n / (n - 1.0)) if n > 1 and self.mut != "no_bessel_moving" else v64).float()
        mom = torch.tensor(momentum, dtype=F32)
        return mm * mom + m * (1 - mom), mv * mom + unb * (1 - mom)

    def stats(self, x, mm, mv, momentum):
        n = x.shape[0]
        if self.mut == "naive_f32":
            xf = x.float()
            m = xf.sum(0) / n
            v64 = ((xf * xf).sum(0) / n - m * m).clamp_min(0).double()
        else:
            K, s1, s2 = self._shifted(x)
            d = s1 / n
            v64 = (s2 / n - d * d).clamp_min(0)
            if self.mut == "bessel_batch" and n > 1:
                v64 = v64 * (n / (n - 1.0))
            m = (K + d).float()
        return (m, v64.float()) + self._moving(m, v64, n, mm, mv, momentum)

    def stats_sums(self, x):
        n, c = x.shape
        if n == 0:
            return torch.zeros(2 * c + 1, dtype=F64)
        K, s1, s2 = self._shifted(x)
        return torch.cat([s1 + n * K, s2 + 2.0 * K * s1 + n * K * K, torch.tensor([float(n)], dtype=F64)])

    def finalize(self, sums, mm, mv, momentum):
        c = (sums.numel() - 1) // 2
        n = float(sums[2 * c])
        m64 = sums[:c] / n
        v64 = (sums[c:2 * c] / n - m64 * m64).clamp_min(0)
        return (m64.float(), v64.float()) + self._moving(m64.float(), v64, n, mm, mv, momentum)

    def apply(self, x, mean, var, gamma, beta, act, res):
        o = (x.float() - mean) * torch.rsqrt(var + self.eps) * gamma + beta
        if act == "relu6":
            o = o.clamp(0.0, 6.0)
        if res is not None:
            o = o + res.float()
        y = o.to(x.dtype)
        return _loop_once(y, self.cap) if self.mut == "loop_once" else y

    def _bwd_parts(self, x, mean, var, act, y, dy):
        rs = torch.rsqrt(var + self.eps)
        gr = dy.float() * _mask(y, act)
        xh = (x.float() - mean) * rs
        c = x.shape[1]
        sb = _final4(_partials(gr.double(), c, self.mut, self.group), self.mut)
        sg = _final4(_partials(gr.double() * xh.double(), c, self.mut, self.group), self.mut)
        return rs, gr, xh, sb, sg

    def _acc(self, old, s):
        if old is None:
            return None
        return s.float() if self.mut == "assign_grads" else old + s.float()

    def _dx(self, x, gamma, rs, gr, xh, sb, sg, inv_n):
        t = gr - sb * inv_n
        if self.mut != "drop_sgx":
            t = t - xh * sg * inv_n
        dx = (gamma * rs * t).to(x.dtype)
        return _loop_once(dx, self.cap) if self.mut == "loop_once" else dx

    def bwd(self, x, mean, var, gamma, act, y, dy, dg0, db0):
        rs, gr, xh, sb, sg = self._bwd_parts(x, mean, var, act, y, dy)
        inv_n = 1.0 / torch.tensor(float(x.shape[0]), dtype=F32)
        return self._dx(x, gamma, rs, gr, xh, sb.float(), sg.float(), inv_n), self._acc(dg0, sg), self._acc(db0, sb)

    def bwd_sums(self, x, mean, var, act, y, dy, dg0, db0):
        n, c = x.shape
        if n == 0:
            return torch.zeros(2 * c + 1, dtype=F64), dg0.clone(), db0.clone()
        rs, gr, xh, sb, sg = self._bwd_parts(x, mean, var, act, y, dy)
        return torch.cat([sb, sg, torch.tensor([float(n)], dtype=F64)]), self._acc(dg0, sg), self._acc(db0, sb)

    def bwd_dx(self, x, mean, var, gamma, act, y, dy, sums, rank):
        c = x.shape[1]
        n = float(x.shape[0]) if self.mut == "inv_n_one_rank" else max(float(sums[2 * c]), 1.0)
        inv_n = torch.tensor(1.0 / n, dtype=F64).float()
        rs = torch.rsqrt(var + self.eps)
        gr = dy.float() * _mask(y, act)
        xh = (x.float() - mean) * rs
        return self._dx(x, gamma, rs, gr, xh, sums[:c].float(), sums[c:2 * c].float(), inv_n)

    # ---- depthwise
    def _pads(self, case):
        pt, pb, pl, pr = case.pads
        return (pl, pt) if self.mut == "swap_pads" else (pt, pl)

    def _gather_taps(self, case, x, shape_out):
        """{(r, s): x at the tap of every output pixel (zero outside)}, fp32."""
        n, h, w, c = x.shape
        ho, wo = shape_out
        pt, pl = self._pads(case)
        xf, st = x.float(), case.stride
        taps = {}
        for r in range(case.k[0]):
            ih = torch.arange(ho) * st - pt + r
            vr = (ih >= 0) & (ih < h)
            for s in range(case.k[1]):
                iw = torch.arange(wo) * st - pl + s
                vs = (iw >= 0) & (iw < w)
                v = xf[:, ih.clamp(0, h - 1)][:, :, iw.clamp(0, w - 1)]
                taps[(r, s)] = v * (vr[:, None] & vs[None, :]).float()[None, :, :, None]
        return taps

    def dw_fwd(self, case, x, w):
        ho, wo = case.out_hw(tuple(x.shape))
        acc = torch.zeros(x.shape[0], ho, wo, x.shape[3], dtype=F32)
        for (r, s), v in self._gather_taps(case, x, (ho, wo)).items():
            if self.mut == "drop_tap" and (r, s) == (case.k[0] - 1, case.k[1] - 1):
                continue
            acc = acc + v * w[r, s]
        y = acc.to(x.dtype)
        return _loop_once(y, self.cap) if self.mut == "loop_once" else y

    def dw_bwd_data(self, case, dy, w, shape):
        n, h, wd, c = shape
        ho, wo = case.out_hw(shape)
        pt, pl = self._pads(case)
        df, st = dy.float(), case.stride
        acc = torch.zeros(n, h, wd, c, dtype=F32)
        for r in range(case.k[0]):
            a = torch.arange(h) + pt - r
            vr = a >= 0
            if self.mut != "no_phase":
                vr = vr & (a % st == 0)
            oh = torch.div(a.clamp_min(0), st, rounding_mode="floor")
            vr = vr & (oh < ho)
            for s in range(case.k[1]):
                if self.mut == "drop_tap" and (r, s) == (case.k[0] - 1, case.k[1] - 1):
                    continue
                b = torch.arange(wd) + pl - s
                vs = b >= 0
                if self.mut != "no_phase":
                    vs = vs & (b % st == 0)
                ow = torch.div(b.clamp_min(0), st, rounding_mode="floor")
                vs = vs & (ow < wo)
                v = df[:, oh.clamp(0, ho - 1)][:, :, ow.clamp(0, wo - 1)]
                acc = acc + v * (vr[:, None] & vs[None, :]).float()[None, :, :, None] * w[r, s]
        dx = acc.to(dy.dtype)
        return _loop_once(dx, self.cap) if self.mut == "loop_once" else dx

    def dw_bwd_filter(self, case, x, dy, dw0):
        c = x.shape[3]
        kh, kw = case.k
        d = dy.float().reshape(-1, c)
        acc = {}  # the kernel's accumulators, indexed r * 3 + s
        for (r, s), v in self._gather_taps(case, x, tuple(dy.shape[1:3])).items():
            if self.mut == "drop_tap" and (r, s) == (kh - 1, kw - 1):
                continue
            part = _partials(v.reshape(-1, c) * d, c, self.mut, self.group)
            tot = torch.zeros(c, dtype=F32)
            for k in range(part.shape[0]):
                tot = tot + part[k]
            acc[r * 3 + s] = tot
        out = torch.empty(kh, kw, c, dtype=F32)
        for r in range(kh):
            for s in range(kw):
                q = r * kw + s if self.mut == "acc_index" else r * 3 + s
                tot = acc.get(q, torch.zeros(c, dtype=F32))
                out[r, s] = tot if self.mut == "assign_grads" else dw0[r, s] + tot
        return out


def _bn_rows(name, dtype, emu, sync=False):
    case = C.BN_BY_NAME[name]
    if sync:
        return C.bn_sync_suite(case, dtype, emu)
    return C.bn_suite(case, dtype, emu, rows=case.small_rows or None)


def _dw_rows(name, dtype, emu):
    case = C.DW_BY_NAME[name]
    return C.dw_suite(case, dtype, emu, shape=case.small or None)


def _cap(case):
    return SMALL_CAP if case.wrap else C.GRID_CAP


# ------------------------------------------------------------ clean emulation
@pytest.mark.parametrize("name", [c.name for c in C.BN_CASES])
def test_bn_emulation_inside_bound(name):
    case = C.BN_BY_NAME[name]
    for dtype in case.dtypes:
        rows = _bn_rows(name, dtype, Emu(cap=_cap(case)))
        ratios, bad = C.worst(rows)
        print(name, dtype, {k: round(v, 3) for k, v in ratios.items()})
        assert not bad, (dtype, {k: ratios[k] for k in bad})
        labels = {r[0].split("[")[0] for r in rows}
        assert {"apply", "bwd.dx", "bwd.dgamma", "bwd.dbeta"} <= labels
        assert case.wrap or {"stats.mean", "stats.var", "stats.moving_mean", "stats.moving_var"} <= labels


@pytest.mark.parametrize("name", C.SYNC_CASES)
def test_sync_emulation_inside_bound(name):
    case = C.BN_BY_NAME[name]
    for dtype in case.dtypes:
        ratios, bad = C.worst(_bn_rows(name, dtype, Emu(), sync=True))
        assert not bad, (dtype, {k: ratios[k] for k in bad})


@pytest.mark.parametrize("name", [c.name for c in C.DW_CASES])
def test_dw_emulation_inside_bound(name):
    case = C.DW_BY_NAME[name]
    for dtype in case.dtypes:
        rows = _dw_rows(name, dtype, Emu(cap=_cap(case)))
        ratios, bad = C.worst(rows)
        print(name, dtype, {k: round(v, 3) for k, v in ratios.items()})
        assert not bad, (dtype, {k: ratios[k] for k in bad})
        assert len(rows) == (2 if case.wrap else 3)


# ------------------------------------------------------------------ mutations
# (mutation, kind, case, labels of which at least one must leave the bound, Emu arguments)
MUTATIONS = [
    ("drop_chunk", "bn", "six_chunks", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta", "bwd.dx"), {}),
    ("drop_chunk", "sync", "rl1", ("sync.sums", "sync.bwd_sums", "sync.finalize.mean", "sync.dx"), {}),
    ("drop_chunk", "dw", "seven_chunks", ("dw.bwd_filter",), {}),
    ("drop_row_lane", "bn", "six_chunks", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {}),
    ("drop_row_lane", "dw", "seven_chunks", ("dw.bwd_filter",), {}),
    ("drop_last_chunk", "bn", "six_chunks", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {}),
    ("drop_last_chunk", "bn", "rl1", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {}),
    ("drop_group", "bn", "six_chunks", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {"group": 1}),
    ("drop_group", "bn", "gx2", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {"group": 256}),
    ("drop_group", "sync", "gx2", ("sync.sums", "sync.bwd_sums"), {"group": 256}),
    ("drop_group", "dw", "c2056", ("dw.bwd_filter",), {"group": 256}),
    ("first_four_chunks", "bn", "six_chunks", ("stats.mean", "stats.var", "bwd.dgamma", "bwd.dbeta"), {}),
    ("first_four_chunks", "sync", "rl1", ("sync.sums", "sync.bwd_sums"), {}),
    ("naive_f32", "bn", "large_mean_f32", ("stats.var",), {}),
    ("bessel_batch", "bn", "rows_lt_rl", ("stats.var",), {}),
    ("no_bessel_moving", "bn", "rows_lt_rl", ("stats.moving_var[0.9]", "stats.moving_var[0.999]"), {}),
    ("no_bessel_moving", "sync", "six_chunks", ("sync.finalize.moving_var[0.9]",), {}),
    ("drop_sgx", "bn", "six_chunks", ("bwd.dx",), {}),
    ("drop_sgx", "sync", "six_chunks", ("sync.dx",), {}),
    ("inv_n_one_rank", "sync", "six_chunks", ("sync.dx",), {}),
    ("assign_grads", "bn", "six_chunks", ("bwd.dgamma", "bwd.dbeta"), {}),
    ("assign_grads", "sync", "six_chunks", ("sync.dgamma", "sync.dbeta"), {}),
    ("assign_grads", "dw", "mn_5x6x8", ("dw.bwd_filter",), {}),
    ("drop_tap", "dw", "mn_5x6x8", ("dw.fwd", "dw.bwd_data", "dw.bwd_filter"), {}),
    ("swap_pads", "dw", "k1x3", ("dw.fwd", "dw.bwd_data", "dw.bwd_filter"), {}),
    ("swap_pads", "dw", "k3x1", ("dw.fwd", "dw.bwd_data", "dw.bwd_filter"), {}),
    ("no_phase", "dw", "s2_odd", ("dw.bwd_data",), {}),
    ("no_phase", "dw", "stride3", ("dw.bwd_data",), {}),
    ("acc_index", "dw", "k2x2", ("dw.bwd_filter",), {}),
    ("loop_once", "bn", "wrap", ("apply", "bwd.dx"), {"cap": SMALL_CAP}),
    ("loop_once", "dw", "wrap", ("dw.fwd", "dw.bwd_data"), {"cap": SMALL_CAP}),
]
ALL_MUTATIONS = {"drop_chunk", "drop_row_lane", "drop_last_chunk", "drop_group", "first_four_chunks", "naive_f32",
                 "bessel_batch", "no_bessel_moving", "drop_sgx", "inv_n_one_rank", "assign_grads", "drop_tap",
                 "swap_pads", "no_phase", "acc_index", "loop_once"}


@pytest.mark.parametrize("mut,kind,name,labels,kw", MUTATIONS, ids=[f"{m[0]}-{m[1]}-{m[2]}" for m in MUTATIONS])
def test_bound_rejects_mutation(mut, kind, name, labels, kw):
    """Every listed label family leaves its bound, in every dtype of the case."""
    case = (C.DW_BY_NAME if kind == "dw" else C.BN_BY_NAME)[name]
    for dtype in case.dtypes:
        emu = Emu(mut, **kw)
        rows = _dw_rows(name, dtype, emu) if kind == "dw" else _bn_rows(name, dtype, emu, sync=kind == "sync")
        ratios, bad = C.worst(rows)
        for want in labels:
            hit = [b for b in bad if b.startswith(want)]
            near = {k: round(v, 3) for k, v in ratios.items() if k.startswith(want)}
            assert hit, f"{mut} passes the bound of {want} on {name} {dtype}: worst err / bound {near}"


def test_every_mutation_is_listed():
    assert {m[0] for m in MUTATIONS} == ALL_MUTATIONS


# ------------------------------------------------------------------- geometry
def test_col_grid_restatement_matches_the_recorded_geometry():
    for case in C.BN_CASES:
        assert C.col_grid(case.rows, case.c) == case.geom, case.name
    for case in C.DW_CASES:
        n, h, w, c = case.shape
        ho, wo = case.out_hw()
        assert C.col_grid(n * ho * wo, c) == case.geom, case.name


def test_table_names_every_branch():
    bn = {c.name: c for c in C.BN_CASES}
    gx, gy, rpc, GT, RL = bn["rl1"].geom
    assert RL == 1 and bn["rl1"].c >= 1032 - 8 and gy > 4 and bn["rl1"].rows % rpc  # RL == 1, many chunks, short last
    gx, gy, rpc, GT, RL = bn["gx2"].geom
    assert gx == 2 and bn["gx2"].c // 8 - GT == 1 and bn["gx2"].c % 64 == 8  # one live group in block 1
    assert bn["one_group"].geom[3:] == (1, 256)
    assert bn["rows_lt_rl"].rows < bn["rows_lt_rl"].geom[4] and bn["rows_lt_rl"].geom[1] == 1
    gx, gy, rpc, GT, RL = bn["six_chunks"].geom
    assert gy > 4 and bn["six_chunks"].rows - (gy - 1) * rpc == 165 and GT * RL == 252  # idle lanes 252-255
    assert bn["one_row"].rows == 1
    for case in C.BN_CASES:
        if case.wrap:
            assert case.rows * case.c // 8 > C.GRID_CAP * 256
            assert case.small_rows * case.c // 8 > SMALL_CAP * 256
    dw = {c.name: c for c in C.DW_CASES}
    assert {c.k for c in C.DW_CASES} >= {(3, 3), (2, 2), (1, 3), (3, 1)}
    assert {c.stride for c in C.DW_CASES} == {1, 2, 3}
    assert dw["c2056"].geom[0] == 2 and dw["seven_chunks"].geom[1] == 7 and dw["one_pixel"].shape[1:3] == (1, 1)
    w = dw["wrap"]
    assert w.wrap and w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3] // 8 > C.GRID_CAP * 256
    assert w.small[0] * w.small[1] * w.small[2] * w.small[3] // 8 > SMALL_CAP * 256
    # input pixels no tap reaches: dx exactly zero (bound zero) there
    for name in ("stride3", "s2_drop_row"):
        case = dw[name]
        inp = C.dw_inputs(case, F32)
        ref, S, cnt = C.dw_bwd_data_ref(case, inp["dy"], inp["w"], case.shape)
        assert bool((cnt == 0).any()) and float(ref[(cnt == 0).expand_as(ref)].abs().max()) == 0.0


def test_saturated_case_stores_exact_bounds():
    case = C.BN_BY_NAME["saturated"]
    for dtype in case.dtypes:
        inp = C.bn_inputs(case, dtype)
        mean, var = C.stored_stats(inp["x"])
        y = C.bn_apply_ref(inp["x"], mean, var, inp["gamma"], inp["beta"], "relu6", None)[0].to(dtype)
        assert int((y == 0).sum()) > 100 and int((y == 6).sum()) > 100


def test_constant_channel_has_zero_variance_and_zero_bound():
    case = C.BN_BY_NAME["const_channel"]
    inp = C.bn_inputs(case, F32)
    mean, var = C.bn_stats_ref(inp["x"])
    bm, bv = C.bn_stats_bound(inp["x"], mean, var, inp["x"][0].double())
    assert float(var[5]) == 0.0 and float(bv[5]) == 0.0 and float(mean[5]) == 1.5

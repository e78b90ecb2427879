"""The bounds of the row-kernel case table (tests/row_kernel_cases.py) can
fail.

No GPU. `Emu` restates every kernel of the table in torch on the CPU in the
kernel's own arithmetic and order: fp32 element math with the storage dtype's
roundings, lane-strided column partials (ln_col), the wave butterfly, rows
strided over the waves of the restated grid, the four-wave block partial, the
act_colsum lanes with their four accumulators and the lanes in order, the
embedding's chunk leaders, the 256-thread strides of the cross-entropy. It is
honest about order, not bit-exact (fused steps are rounded once from fp64).
Checked:

  * the unmutated emulation is inside the bound of every case, dtype and label;
  * each mutation below puts at least one element of the named label outside
    the bound, in every dtype of its case;
  * the grid restatements give the geometry every case records, and every
    branch the kernels have is named by a case;
  * the correctly rounded fp64 reference itself passes every bound, and
    halving the bf16 store term rejects it.

Mutations: mean_skip_col (one column missing from the row mean), var_dm1
(variance / (d - 1)), eps_1e3, tail_098 (the last 8 columns' xhat * gamma term
scaled by 0.98), pe_row_r (pe row r in place of r % pe_rows), res_unrounded
(the residual sum kept in fp32), drop_s2 (dx without the s2 term),
s1_no_gamma, pg_reset (pg / pb reset on every row of a wave's walk),
drop_wave (one of the four waves missing from the block partial),
swap_grads (dbeta written where dgamma belongs), drop_index (mask index
row * d + col + 1), drop_scale (1 / p), drop_gt (`>` for `>=`: the large flat
case holds an element with u == p), emb_second_chunk (a repeated id's second
chunk not added), emb_skip_pad, emb_sumsq_once (sumsq counting each id once),
xent_no_max, xent_mean_unmasked, xent_onehot_shift (p - 1 at label + 1),
relu6_le6 (mask y <= 6), leaky_side, drop_row_chunk (one row chunk missing
from db).
"""
import numpy as np
import pytest
import torch

import row_kernel_cases as C

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


@pytest.fixture(autouse=True, scope="module")
def _single_thread():
    """The tensors here are large enough for torch to start its OpenMP pool;
    tests that fork afterwards (tests/test_dist_gloo.py) would hang in a child
    that inherits a started pool. One thread starts none."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


def _add(s, t):
    """One accumulation step rounded once to fp32 (t may be an exact fp64 product: a fused step)."""
    return (s.double() + t.double()).float()


def _butterfly(v):
    """wave_sum over the last dimension (64 lanes); every lane ends equal."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def lane_sum(terms, vec):
    """Row sums of terms [rows, d] (fp32, or fp64 exact products) in the
    LayerNorm kernels' order: each lane its columns in k order, then the
    butterfly."""
    rows, d = terms.shape
    tz = torch.cat([terms, torch.zeros(rows, 1, dtype=terms.dtype)], 1)  # column d: the dead lanes' zero
    lane = torch.arange(64)
    s = torch.zeros(rows, 64)
    for k in range(C.LN_MAXE):
        col = (lane + 64 * (k >> 3)) * 8 + (k & 7) if vec else lane + 64 * k
        if int(col.min()) < d:
            s = _add(s, tz[:, col.clamp_max(d)])
    return _butterfly(s)


def colsum(ws, mut=None):
    """act_colsum_kernel on ws [chunks, c]."""
    chunks, c = ws.shape
    KL = 1024 // C.colsum_cb(c)
    ws = torch.cat([ws, torch.zeros(4 * KL, c)])
    s = [torch.zeros(KL, c) for _ in range(4)]
    k = torch.arange(KL)
    while bool((k + 3 * KL < chunks).any()):
        m = (k + 3 * KL < chunks)
        for u in range(4):
            s[u] = s[u] + ws[torch.where(m, k + u * KL, chunks)]  # row `chunks` is zero
        k = torch.where(m, k + 4 * KL, k)
    while bool((k < chunks).any()):
        m = k < chunks
        s[0] = s[0] + ws[torch.where(m, k, chunks)]
        k = torch.where(m, k + KL, k)
    red = (s[0] + s[1]) + (s[2] + s[3])
    out = red[0]
    for q in range(1, KL):
        out = out + red[q]
    return out


def thread_sum(v, scale=None):
    """ordered_sum_kernel / the cross-entropy's block sums over the last
    dimension: 256 threads striding, the butterfly per wave, then the waves."""
    n = v.shape[-1]
    pad = torch.zeros(*v.shape[:-1], C.cdiv(n, 256) * 256)
    pad[..., :n] = v
    pad = pad.view(*v.shape[:-1], -1, 256)
    s = torch.zeros(*v.shape[:-1], 256)
    for k in range(pad.shape[-2]):
        s = s + pad[..., k, :]
    w = _butterfly(s.view(*v.shape[:-1], 4, 64))
    if scale is None:  # xent: red[0] + red[1] + red[2] + red[3]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])) * scale


class Emu:
    def __init__(self, mut=None):
        self.mut = mut

    # ---- dropout
    def _keep(self, seed, sd, rows, d, p):
        return C.keep_mask(C.drop_key(seed, sd), rows * d, p, shift=int(self.mut == "drop_index"),
                           strict=self.mut == "drop_gt").view(rows, d)

    def _drop(self, v, keep, p, dtype):
        sc = torch.tensor(C.drop_scale(p, self.mut == "drop_scale"), dtype=F32)
        return torch.where(keep, v.float() * sc, torch.zeros(())).to(dtype)

    # ---- LayerNorm
    def _v(self, x, res, dtype):
        if res is None:
            return x.float()
        s = x.float() + res.float()
        return s if self.mut == "res_unrounded" else s.to(dtype).float()

    def _ln_fwd(self, v, gamma, beta, pe, pe_rows, eps, dtype, vec):
        rows, d = v.shape
        eps = torch.tensor(1e-3 if self.mut == "eps_1e3" else eps, dtype=F32)
        vm = v.clone()
        if self.mut == "mean_skip_col":
            vm[:, d - 1] = 0
        mu = lane_sum(vm, vec) / torch.tensor(float(d))
        t = v - mu[:, None]
        var = lane_sum(t.double() * t.double(), vec) / torch.tensor(float(d - 1 if self.mut == "var_dm1" and d > 1 else d))
        rs = torch.rsqrt(var + eps)
        xh = t * rs[:, None]
        if self.mut == "tail_098":
            xg = xh.double() * gamma.double()
            xg[:, d - 8:] *= 0.98
            o = (xg + beta.double()).float()
        else:
            o = (xh.double() * gamma.double() + beta.double()).float()
        if pe is not None:
            r = torch.arange(rows)
            o = o + pe[r.clamp_max(pe.shape[0] - 1) if self.mut == "pe_row_r" else r % pe_rows]
        return o.to(dtype), mu, rs

    def ln_fwd(self, case, x, res, gamma, beta, pe, pe_rows, eps):
        dtype = x.dtype
        return self._ln_fwd(self._v(x, res, dtype), gamma, beta, pe, pe_rows, eps, dtype,
                            C.ln_is_vec(x.shape[1], dtype, case.offset))

    def _ln_bwd(self, v, gamma, mean, rstd, dyf, dtype, vec):
        """(dx, partial rows [grid, 2 d])."""
        rows, d = v.shape
        df = torch.tensor(float(d))
        xh = (v - mean[:, None]) * rstd[:, None]
        dyf = dyf.float()
        g = dyf * gamma
        s1 = lane_sum(dyf if self.mut == "s1_no_gamma" else g, vec) / df
        s2 = lane_sum(g * xh, vec) / df
        if self.mut == "drop_s2":
            s2 = s2 * 0
        dx = (rstd[:, None] * ((g - s1[:, None]).double() - xh.double() * s2[:, None].double()).float()).to(dtype)
        grid = C.grid_for(rows, 4, C.BWD_CAP)
        nw = 4 * grid
        pg, pb = torch.zeros(nw, d), torch.zeros(nw, d)
        tg = dyf * xh
        for r0 in range(0, rows, nw):  # a wave's rows in order
            n = min(nw, rows - r0)
            if self.mut == "pg_reset":
                pg, pb = torch.zeros(nw, d), torch.zeros(nw, d)
            pg[:n] = pg[:n] + tg[r0:r0 + n]
            pb[:n] = pb[:n] + dyf[r0:r0 + n]
        w = torch.cat([pg, pb], 1).view(grid, 4, 2 * d)
        part = (w[:, 0] + w[:, 1]) + w[:, 2]
        if self.mut != "drop_wave":
            part = part + w[:, 3]
        return dx, part

    def _grads(self, part, d, dg0, db0):
        if dg0 is None:
            return None, None
        s = colsum(part)
        sg, sb = (s[d:], s[:d]) if self.mut == "swap_grads" else (s[:d], s[d:])
        return dg0 + sg, db0 + sb

    def ln_bwd(self, case, x, res, gamma, mean, rstd, dy, dg0, db0, p, seed, sd):
        dtype = x.dtype
        rows, d = x.shape
        dx, part = self._ln_bwd(self._v(x, res, dtype), gamma, mean, rstd, dy, dtype, C.ln_is_vec(d, dtype, case.offset))
        dz = self._drop(dx, self._keep(seed, sd, rows, d, p), p, dtype) if p > 0 else None
        return (dx, *self._grads(part, d, dg0, db0), dz)

    # ---- broadcast form
    def _synth(self, case, c, cbias, p, seed, sd, dtype):
        cr = c.repeat_interleave(case.t, 0)
        a = cr if cbias is None else cr + cbias
        rows, d = a.shape
        return self._drop(a, self._keep(seed, sd, rows, d, p), p, dtype) if p > 0 else a.to(dtype)

    def bcast_fwd(self, case, c, cbias, p, seed, sd, res, gamma, beta, eps, want_x):
        dtype = res.dtype
        x = self._synth(case, c, cbias, p, seed, sd, dtype)
        y, mu, rs = self._ln_fwd(self._v(x, res, dtype), gamma, beta, None, 1, eps, dtype, C.ln_is_vec(case.d, dtype))
        return y, mu, rs, (x if want_x else None)

    def bcast_bwd(self, case, c, cbias, p, seed, sd, res, gamma, mean, rstd, dy, dg0, db0):
        dtype = res.dtype
        x = self._synth(case, c, cbias, p, seed, sd, dtype)
        rows, d = x.shape
        dx, part = self._ln_bwd(self._v(x, res, dtype), gamma, mean, rstd, dy, dtype, C.ln_is_vec(d, dtype))
        dz = self._drop(dx, self._keep(seed, sd, rows, d, p), p, dtype) if p > 0 else None
        return (dx, *self._grads(part, d, dg0, db0), dz)

    # ---- views
    def views_fwd(self, case, xs, gamma, beta, pe, pe_rows, seeds, p, sd, eps):
        vec = C.ln_is_vec(case.d, case.dtype) and case.misaligned < 0
        out = []
        for x, pr, seed in zip(xs, pe_rows, seeds):
            y, mu, rs = self._ln_fwd(x.float(), gamma, beta, pe, pr, eps, case.dtype, vec)
            if p > 0:
                y = self._drop(y, self._keep(seed, sd, x.shape[0], case.d, p), p, case.dtype)
            out.append((y, mu, rs))
        return out

    def views_bwd(self, case, xs, gamma, stats, dys, seeds, p, sd, dg0, db0):
        vec = C.ln_is_vec(case.d, case.dtype) and case.misaligned < 0
        dxs, dg, db = [], dg0, db0
        for x, (mean, rstd), dy, seed in zip(xs, stats, dys, seeds):
            if x.shape[0] == 0:
                dxs.append(None)
                continue
            if p > 0:
                dy = self._drop(dy, self._keep(seed, sd, x.shape[0], case.d, p), p, case.dtype)
            dx, part = self._ln_bwd(x.float(), gamma, mean, rstd, dy, case.dtype, vec)
            dxs.append(dx)
            dg, db = self._grads(part, case.d, dg, db)
        return dxs, dg, db

    # ---- embedding
    def embed_fwd(self, case, dtype, tok, emb, pe, p, seed, sd):
        rows = tok.numel()
        y = (emb[tok.long()] + pe[torch.arange(rows) % case.t]).to(dtype)
        return self._drop(y, self._keep(seed, sd, rows, case.d, p), p, dtype) if p > 0 else y

    def embed_bwd(self, case, tok, dy, de0, sumsq0, p, seed, sd):
        rows, d = dy.shape
        tok = tok.long()
        g = (self._drop(dy, self._keep(seed, sd, rows, d, p), p, dy.dtype) if p > 0 else dy).float()
        nch = C.cdiv(rows, C.EMB_CHUNK)
        tk = torch.full((nch * 64,), -1, dtype=torch.long)
        tk[:rows] = tok
        tk = tk.view(nch, 64)
        gp = torch.zeros(nch * 64, d)
        gp[:rows] = g
        gp = gp.view(nch, 64, d)
        same = tk[:, :, None] == tk[:, None, :]  # [chunk, i, j]
        lead = same.float().argmax(2)  # the first j with the same id
        acc = torch.zeros(nch, 64, d)
        ch = torch.arange(nch)
        for i in range(64):  # positions of a chunk in order into their leader's row
            acc[ch, lead[:, i]] = acc[ch, lead[:, i]] + gp[:, i]
        de = de0.clone()
        seen = set()
        a = torch.zeros_like(de0)
        for k in range(nch):  # the chunks in order
            ids = [int(i) for i in tk[k].unique() if i >= 0]
            for i in ids:
                if self.mut == "emb_second_chunk" and i in seen:
                    continue
                seen.add(i)
                a[i] = a[i] + acc[k, int((tk[k] == i).float().argmax())]
        present = torch.zeros(de0.shape[0], dtype=torch.bool)
        present[tok] = True
        if self.mut == "emb_skip_pad":
            present[0] = False
        de[present] = de[present] + a[present]
        if sumsq0 is None:
            return de, None
        rowsq = lane_sum(g.double() * g.double(), False) if d <= 1024 else None
        if self.mut == "emb_sumsq_once":
            first = torch.zeros(rows, dtype=torch.bool)
            first[[int((tok == i).float().argmax()) for i in tok.unique()]] = True
            rowsq = rowsq * first
        return de, sumsq0 + thread_sum(rowsq, 1.0).view(1)

    # ---- cross-entropy
    def xent(self, case, x, lab, dtype, gscale, want_d):
        rows, v = x.shape
        lab = lab.long()
        m = x.max(1, keepdim=True).values if self.mut != "xent_no_max" else torch.zeros(rows, 1)
        e = torch.exp(x - m)
        s = thread_sum(e)[:, None]
        mask = (lab != 0).float()[:, None]
        rl = torch.where(mask != 0, (m + torch.log(s)) - x.gather(1, lab[:, None]), torch.zeros(()))
        n = float(mask.sum().clamp_min(1)) if self.mut == "xent_mean_unmasked" else float(rows)
        loss = thread_sum(rl[:, 0], 1.0 / torch.tensor(n)).view(1)
        if not want_d:
            return loss, None
        p = e / s
        hot = (lab + 1).clamp_max(v - 1) if self.mut == "xent_onehot_shift" else lab
        p = p - torch.zeros_like(p).scatter_(1, hot[:, None], 1.0)
        coef = mask * torch.tensor(gscale, dtype=F32) / torch.tensor(float(rows))
        return loss, (p * coef).to(dtype)

    # ---- activation backward
    def act_bwd(self, case, dtype, act, dy, y, db0, p, seed, sd, write=True):
        rows, c = dy.shape
        t = dy.float()
        if p > 0:
            t = self._drop(dy, self._keep(seed, sd, rows, c, p), p, F32)
        if act != "none":
            yf = y.float()
            if act == "relu":
                g = (yf > 0).float()
            elif act == "relu6":
                g = ((yf > 0) & ((yf <= 6) if self.mut == "relu6_le6" else (yf < 6))).float()
            else:
                a = torch.tensor(C.LEAKY, dtype=F32)
                g = torch.where((yf <= 0) if self.mut == "leaky_side" else (yf > 0), torch.ones(()), a)
            t = t * g
        dz = t.to(dtype)
        if db0 is None:
            return dz, None
        vec, gx, gy, rpc, GT, RL = C.act_bwd_grid(rows, c, dtype, case.offset == 0)
        r = torch.arange(rows)
        chunk, lane = r // rpc, (r % rpc) % RL
        lanes = torch.zeros(gy * RL, c).index_add_(0, chunk * RL + lane, dz.float()).view(gy, RL, c)
        off = RL // 2
        while off > 0:  # the tree over the row lanes
            lanes = lanes[:, :off] + lanes[:, off:2 * off]
            off //= 2
        part = lanes[:, 0]
        if self.mut == "drop_row_chunk":
            part[gy // 2] = 0
        return dz, db0 + (part[0] if gy == 1 else colsum(part))

    def bias_grad(self, case, dtype, dy, db0):
        return self.act_bwd(case, dtype, "none", dy, None, db0, 0.0, 0, None)[1]

    # ---- dropout, cast, add
    def cast(self, x, dtype):
        return x.float().to(dtype)

    def add(self, a, b):
        return (a.float() + b.float()).to(a.dtype)

    def dropout(self, x, p, seed, sd):
        return self._drop(x, self._keep(seed, sd, 1, x.numel(), p).view(-1), p, x.dtype)


SUITES = {
    "ln": lambda name, dtype, impl: C.ln_suite(C.LN_BY_NAME[name], dtype, impl),
    "bcast": lambda name, dtype, impl: C.bcast_suite(C.BCAST_BY_NAME[name], dtype, impl),
    "views": lambda name, dtype, impl: C.views_suite(C.VIEWS_BY_NAME[name], impl),
    "embed": lambda name, dtype, impl: C.emb_suite(C.EMB_BY_NAME[name], dtype, impl),
    "xent": lambda name, dtype, impl: C.xent_suite(C.XENT_BY_NAME[name], impl),
    "act": lambda name, dtype, impl: C.act_suite(C.ACT_BY_NAME[name], dtype, impl),
    "flat": lambda name, dtype, impl: C.flat_suite(int(name), impl),
}


def _dtypes(kind, name):
    if kind in ("ln", "bcast", "embed", "act"):
        table = {"ln": C.LN_BY_NAME, "bcast": C.BCAST_BY_NAME, "embed": C.EMB_BY_NAME, "act": C.ACT_BY_NAME}[kind]
        return table[name].dtypes
    return (None,)  # the suite walks its own dtypes


ALL_CASES = ([("ln", c.name) for c in C.LN_CASES] + [("bcast", c.name) for c in C.BCAST_CASES]
             + [("views", c.name) for c in C.VIEWS_CASES] + [("embed", c.name) for c in C.EMB_CASES]
             + [("xent", c.name) for c in C.XENT_CASES] + [("act", c.name) for c in C.ACT_CASES]
             + [("flat", str(n)) for n in C.FLAT_SIZES])


# ------------------------------------------------------------ clean emulation
@pytest.mark.parametrize("kind,name", ALL_CASES, ids=[f"{k}-{n}" for k, n in ALL_CASES])
def test_emulation_inside_bound(kind, name):
    for dtype in _dtypes(kind, name):
        rows = SUITES[kind](name, dtype, Emu())
        ratios, bad = C.worst(rows)
        top = max(ratios, key=ratios.get)
        print(kind, name, dtype, f"worst {ratios[top]:.3f} at {top}")
        assert not bad, (dtype, {k: ratios[k] for k in bad})


def test_suites_carry_every_label():
    fam = lambda rows: {r[0].split("[")[0] for r in rows}
    assert fam(SUITES["ln"]("scalar_300", BF16, Emu())) == {
        "ln.y", "ln.mean", "ln.rstd", "ln.dx", "ln.dgamma", "ln.dbeta", "lndrop.dx", "lndrop.dz", "lndrop.dgamma",
        "lndrop.dbeta"}
    assert fam(SUITES["ln"]("fwd_row_loop", F32, Emu())) == {"ln.y", "ln.mean", "ln.rstd"}
    assert fam(SUITES["bcast"]("b4_t1_8", F32, Emu())) == {
        "bcast.x_out", "bcast.y", "bcast.mean", "bcast.rstd", "bcast.dx", "bcast.dz", "bcast.dgamma", "bcast.dbeta"}
    assert fam(SUITES["views"]("views_8_f32", None, Emu())) == {
        "views.y", "views.mean", "views.rstd", "views.dx", "views.dgamma", "views.dbeta"}
    assert fam(SUITES["embed"]("one_position", F32, Emu())) == {"embed.y", "embed.d_emb", "embed.sumsq"}
    assert fam(SUITES["xent"]("v7", None, Emu())) == {"xent.loss", "xent.dlogits"}
    assert fam(SUITES["act"]("scalar_5x3", F32, Emu())) == {"act.dz", "act.db", "bias_grad"}
    assert fam(SUITES["flat"]("1", None, Emu())) == {"cast", "add", "dropout"}


# ------------------------------------------------------------------ mutations
# (mutation, kind, case, label families of which each must leave its bound)
MUTATIONS = [
    ("mean_skip_col", "ln", "scalar_300", ("ln.y", "ln.mean")),
    ("mean_skip_col", "ln", "vec_1000", ("ln.y", "ln.mean")),
    ("mean_skip_col", "views", "views_512_bf16", ("views.y", "views.mean")),
    ("var_dm1", "ln", "scalar_300", ("ln.y", "ln.rstd")),
    ("var_dm1", "ln", "vec_1000", ("ln.y", "ln.rstd")),
    ("var_dm1", "bcast", "b3_t5_512", ("bcast.y", "bcast.rstd")),
    ("eps_1e3", "ln", "vec_1000", ("ln.rstd",)),
    ("eps_1e3", "ln", "const_row", ("ln.rstd",)),
    ("eps_1e3", "ln", "large_mean_f32", ("ln.y", "ln.rstd")),
    ("tail_098", "ln", "scalar_300", ("ln.y",)),
    ("tail_098", "ln", "vec_1000", ("ln.y",)),
    ("tail_098", "ln", "misaligned", ("ln.y",)),
    ("pe_row_r", "ln", "vec_1000", ("ln.y[-,pe]", "ln.y[res,pe]")),
    ("pe_row_r", "views", "views_8_f32", ("views.y",)),
    ("res_unrounded", "ln", "misaligned", ("ln.y[res", "ln.dx[res")),
    ("drop_s2", "ln", "scalar_300", ("ln.dx",)),
    ("drop_s2", "ln", "vec_1000", ("ln.dx", "lndrop.dx")),
    ("s1_no_gamma", "ln", "scalar_300", ("ln.dx",)),
    ("s1_no_gamma", "bcast", "b2_t7_300", ("bcast.dx",)),
    ("pg_reset", "ln", "bwd_row_loop", ("ln.dgamma", "ln.dbeta", "lndrop.dgamma", "lndrop.dbeta")),
    ("pg_reset", "ln", "bwd_row_loop_512", ("ln.dgamma", "ln.dbeta")),
    ("pg_reset", "views", "views_512_bf16", ("views.dgamma", "views.dbeta")),
    ("drop_wave", "ln", "vec_1000", ("ln.dgamma", "ln.dbeta")),
    ("drop_wave", "ln", "bwd_row_loop", ("ln.dgamma", "ln.dbeta")),
    ("swap_grads", "ln", "scalar_300", ("ln.dgamma", "ln.dbeta")),
    ("swap_grads", "views", "views_8_f32", ("views.dgamma", "views.dbeta")),
    ("drop_index", "ln", "scalar_300", ("lndrop.dz",)),
    ("drop_index", "views", "views_8_f32", ("views.y[p=0.1", "views.dx[p=0.1")),
    ("drop_index", "bcast", "b3_t5_512", ("bcast.x_out[p=0.1", "bcast.dz")),
    ("drop_index", "embed", "d300", ("embed.y[p=0.1", "embed.d_emb[p=0.1")),
    ("drop_index", "act", "r37_c12", ("act.dz[none,p=0.25",)),
    ("drop_index", "flat", str(C.FLAT_SIZES[1]), ("dropout",)),
    ("drop_scale", "ln", "vec_1000", ("lndrop.dz[-,p=0.1", "lndrop.dz[res,p=0.1")),
    ("drop_scale", "embed", "b4_t31_512", ("embed.y[p=0.1", "embed.d_emb[p=0.1", "embed.sumsq[p=0.1")),
    ("drop_scale", "act", "r37_c12", ("act.dz[relu,p=0.25",)),
    ("drop_gt", "flat", str(C.FLAT_SIZES[1]), ("dropout[float32,null", "dropout[bfloat16,dev")),
    ("emb_second_chunk", "embed", "b4_t31_512", ("embed.d_emb",)),
    ("emb_second_chunk", "embed", "second_cb_pass", ("embed.d_emb",)),
    ("emb_skip_pad", "embed", "d300", ("embed.d_emb",)),
    ("emb_sumsq_once", "embed", "d1024", ("embed.sumsq",)),
    ("xent_no_max", "xent", "pm80_v10003", ("xent.loss",)),
    ("xent_mean_unmasked", "xent", "v1000", ("xent.loss",)),
    ("xent_onehot_shift", "xent", "v7", ("xent.dlogits",)),
    ("xent_onehot_shift", "xent", "v10003", ("xent.dlogits",)),
    ("relu6_le6", "act", "relu6_edges", ("act.dz",)),  # db is judged from the stored dz
    ("leaky_side", "act", "r37_c12", ("act.dz[leaky",)),
    ("drop_row_chunk", "act", "cb64", ("act.db", "bias_grad")),
    ("drop_row_chunk", "act", "many_chunks", ("act.db", "bias_grad")),
]
ALL_MUTATIONS = {"mean_skip_col", "var_dm1", "eps_1e3", "tail_098", "pe_row_r", "res_unrounded", "drop_s2",
                 "s1_no_gamma", "pg_reset", "drop_wave", "swap_grads", "drop_index", "drop_scale", "drop_gt",
                 "emb_second_chunk", "emb_skip_pad", "emb_sumsq_once", "xent_no_max", "xent_mean_unmasked",
                 "xent_onehot_shift", "relu6_le6", "leaky_side", "drop_row_chunk"}


@pytest.mark.parametrize("mut,kind,name,labels", MUTATIONS, ids=[f"{m[0]}-{m[1]}-{m[2]}" for m in MUTATIONS])
def test_bound_rejects_mutation(mut, kind, name, labels):
    """Every listed label family leaves its bound, in every dtype of the case."""
    for dtype in _dtypes(kind, name):
        ratios, bad = C.worst(SUITES[kind](name, dtype, Emu(mut)))
        for want in labels:
            hit = [b for b in bad if b.startswith(want)]
            near = {k: round(v, 3) for k, v in ratios.items() if k.startswith(want)}
            assert hit, f"{mut} passes the bound of {want} on {name} {dtype}: worst err / bound {near}"


def test_every_mutation_is_listed():
    assert {m[0] for m in MUTATIONS} == ALL_MUTATIONS


def test_greater_than_case_holds_an_element_at_exactly_p():
    n = C.FLAT_SIZES[1]
    for sd in (None, C.FLAT_SEED_DEV):
        u = C.uniform01(C.drop_key(C.FLAT_SEED[n], sd), np.arange(n, dtype=np.uint64))
        assert int((u == np.float32(C.FLAT_P)).sum()) >= 1


# ------------------------------------------------------------------- geometry
def test_grid_restatements_match_the_recorded_geometry():
    for c in C.LN_CASES:
        vec = C.ln_is_vec(c.d, BF16, c.offset)
        assert (vec, *C.ln_geom(c.rows, c.d)) == c.geom, c.name
    for c in C.VIEWS_CASES:
        assert C.views_geom(c.rows) == c.geom, c.name
    for c in C.EMB_CASES:
        assert C.emb_geom(c.b * c.t, c.d) == c.geom, c.name
    for c in C.ACT_CASES:
        for dt in c.dtypes:
            assert C.act_bwd_grid(c.rows, c.c, dt, c.offset == 0) == c.geom[dt], (c.name, dt)


def test_table_names_every_branch():
    ln = C.LN_BY_NAME
    # 1. the backward row loop: more than 4096 rows, pg / pb accumulate across rows
    for n in ("bwd_row_loop", "bwd_row_loop_512"):
        vec, gf, rf, gb, rb, cb, four = ln[n].geom
        assert ln[n].rows > 4096 and gb == 1024 and rb == 2 and four and not ln[n].fwd_only
    assert ln["bwd_row_loop"].geom[5] == 16 and ln["bwd_row_loop_512"].geom[5] == 32
    # 2. the forward row loop
    assert ln["fwd_row_loop"].rows > 32768 and ln["fwd_row_loop"].geom[1:3] == (8192, 2)
    # 3. the scalar bf16 route through d % 8 and through alignment; one misaligned view
    assert ln["scalar_300"].d % 8 == 4 and not ln["scalar_300"].geom[0]
    assert ln["misaligned"].d % 8 == 0 and ln["misaligned"].offset % 8 and not ln["misaligned"].geom[0]
    assert C.VIEWS_BY_NAME["views_512_bf16_misaligned"].misaligned == 1
    assert C.ln_lane_depth(1024, True) == C.LN_MAXE and C.ln_lane_depth(300, False) == 5
    assert sum(1 for lane in range(64) if C.ln_col(True, lane, 8) < 520) == 1  # one live lane in the second group
    assert sum(1 for lane in range(64) if C.ln_col(True, lane, 8) < 1000) == 61
    v = C.VIEWS_BY_NAME["views_512_bf16"]
    assert 0 in v.rows and v.geom[0][1] == 1024 and v.rows[0] > 4096
    # 4. the embedding leader's second cb pass, tokens from HBM, d != 512
    emb = C.EMB_BY_NAME
    assert emb["second_cb_pass"].geom[1] and not emb["second_cb_pass"].geom[2]
    assert emb["tokens_from_hbm"].geom[2] and emb["d1024"].geom[3:] == (2, 2) and emb["d300"].d % 64
    for c in C.EMB_CASES:
        tok = C.emb_inputs(c, F32)["tok"]
        assert int((tok == C.VOCAB - 1).sum()) == 1 and int((tok == C.VOCAB - 2).sum()) == 0
        if c.b * c.t > 64:  # ~40 % padding, ids repeated within and across chunks
            assert 0.3 < float((tok == 0).float().mean()) < 0.5
            first = tok[:64]
            assert len(set(first.tolist())) < 64 and set(first.tolist()) & set(tok[64:].tolist())
    # 5. the cross-entropy's shapes and data
    xe = C.XENT_BY_NAME
    assert xe["v7"].v < 256 and xe["v256"].v == 256 and xe["v10003"].v % 256 and C.XENT_LD > 0 and C.XENT_LDD > 0
    assert set(C.XENT_DTYPES) == {F32, BF16} and set(C.XENT_SCALES) == {1.0, 0.125}
    big = C.xent_inputs(xe["pm80_v10003"])
    assert float(big["logits"].max()) > 80 and float(big["logits"].min()) < -80
    assert int(C.xent_inputs(xe["all_pad"])["labels"].abs().sum()) == 0
    assert int(C.xent_inputs(xe["v1000"])["labels"][0]) == 999
    # 6. act_bwd: the one-launch grids with GT 3 and 5, CB = 64, many chunks, misaligned, every activation
    act = C.ACT_BY_NAME
    assert act["one_launch_gt3"].geom[BF16][2:] == (1, 200, 3, 64) and 3 * 64 < 256  # lanes tr >= RL idle
    assert act["one_launch_gt5"].geom[BF16][2:] == (1, 100, 5, 32)
    assert C.colsum_cb(act["cb64"].c) == 64 and act["cb64"].geom[BF16][2] > 1
    assert act["many_chunks"].geom[F32][2] == 47 and not act["misaligned"].geom[BF16][0]
    assert set(act["r37_c12"].acts) == {"none", "relu", "relu6", "leaky"}
    y = C.act_inputs(act["relu6_edges"], BF16)["y"]
    assert int((y == 0).sum()) > 50 and int((y == 6).sum()) > 50
    # the four-wide act_colsum loop and its tail
    assert C.grid_for(4099, 4, C.BWD_CAP) > 3 * (1024 // 16)


def test_constant_row_has_zero_variance():
    case = C.LN_BY_NAME["const_row"]
    for dtype in case.dtypes:
        inp = C.ln_inputs(case, dtype)
        ref = C.ln_fwd_ref(inp["x"].double(), inp["gamma"], inp["beta"], None, 1, C.EPS, dtype, True)
        assert float(ref["rstd"][0][3]) == pytest.approx(C.EPS ** -0.5, rel=1e-12)
        assert float(ref["mean"][0][3]) == 1.5


# -------------------------------------------------- the reference and the store
STORE_CASES = [("ln", "vec_1000"), ("ln", "scalar_300"), ("bcast", "b3_t5_512"), ("embed", "d300"),
               ("act", "r37_c12"), ("xent", "v1000")]


@pytest.mark.parametrize("kind,name", STORE_CASES, ids=[f"{k}-{n}" for k, n in STORE_CASES])
def test_rounded_reference_passes_and_half_the_store_term_rejects_it(kind, name, monkeypatch):
    """Every output replaced by its fp64 reference rounded to the output's
    dtype is inside every bound; with the bf16 store term halved (2^-9) the
    correctly rounded reference itself is rejected: the store term is not
    slack."""
    for dtype in _dtypes(kind, name):
        rows = SUITES[kind](name, dtype, Emu())
        ideal = [(label, ref.to(got.dtype), ref, bnd) for label, got, ref, bnd in rows
                 if not label.startswith(("lndrop.dz", "bcast.dz", "act.db"))]  # judged from a stored output
        ratios, bad = C.worst(ideal)
        assert not bad, (dtype, bad)
    monkeypatch.setattr(C, "store_u", lambda dt: 2.0 ** -9 if dt == BF16 else C.U)
    rows = SUITES[kind](name, BF16 if kind != "xent" else None, Emu())
    ideal = [(label, ref.to(got.dtype), ref, bnd) for label, got, ref, bnd in rows if got.dtype == BF16
             and not label.startswith(("lndrop.dz", "bcast.dz"))]
    ratios, bad = C.worst(ideal)
    assert ideal and bad, "the rounded reference passes with half the store term"

"""The row kernels of csrc/elementwise.hip (LayerNorm and its fused,
broadcast and view forms, embedding + posenc, the masked cross-entropy,
activation backward / bias gradient, dropout, cast, add) element by element
against fp64, on the case table of tests/row_kernel_cases.py (whose bounds
tests/test_row_kernel_bars.py proves able to fail).

The C entry points are called directly through fpnmt._lib with the workspace
the package installs. For every case, dtype and variant:

1. every output element is within its derived bound of the fp64 reference
   computed from the exact stored inputs (the worst err / bound ratio of each
   output is printed);
2. every output is allocated with guard elements holding a sentinel after it
   (and before it where the case shifts the pointers, and in the ld / ldd gaps
   of the cross-entropy), which come back bitwise untouched; pre-filled
   gradient accumulators come back as old + sum, so `=` for `+=` fails 1.;
3. a second run into fresh buffers is bitwise equal (fixed-order reductions,
   no atomics);
4. routes that must agree do so bit for bit: fpnmt_bias_grad against
   fpnmt_act_bwd's db (act none, p = 0), and fpnmt_layernorm_views_fwd / _bwd
   against the same views launched one by one through fpnmt_layernorm_fwd /
   _bwd and fpnmt_dropout.
"""
import pytest
import torch

import row_kernel_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _lib():
    from fpnmt import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


class Out:
    """numel outputs (the sentinel, or `init`) with `off` sentinel elements
    before and GUARD after."""

    def __init__(self, shape, dtype, init=None, off=0):
        self.shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.off = off
        self.buf = torch.full((off + self.n + C.GUARD,), C.SENTINEL, dtype=dtype, device=DEV)
        if init is not None:
            self.buf[off:off + self.n] = init.reshape(-1)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def live(self):
        return self.buf[self.off:self.off + self.n].view(self.shape)

    def guards_untouched(self):
        g = torch.cat([self.buf[:self.off], self.buf[self.off + self.n:]])
        return torch.equal(_bits(g), _bits(torch.full_like(g, C.SENTINEL)))


def _in(t, off=0):
    """t at a pointer shifted by `off` elements from an aligned allocation."""
    if t is None or off == 0:
        return None if t is None else t.contiguous()
    b = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    b[off:] = t.reshape(-1)
    return b[off:].view(t.shape)


def _p(t):
    return None if t is None else (t.ptr if isinstance(t, Out) else t.data_ptr())


def _sd(sd):
    return None if sd is None else torch.tensor([sd], dtype=torch.int64, device=DEV)


def _twice(launch):
    """launch() -> [Out or None]. Runs it twice into fresh buffers: bitwise
    equal, guards untouched; returns the first run's live views."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    views = []
    for oa, ob in zip(a, b):
        if oa is None:
            views.append(None)
            continue
        assert torch.equal(_bits(oa.buf), _bits(ob.buf)), "two runs differ"
        assert oa.guards_untouched(), "guard elements overwritten"
        views.append(oa.live())
    return views


_ACT = {"none": "ACT_NONE", "relu": "ACT_RELU", "relu6": "ACT_RELU6", "leaky": "ACT_LEAKY"}


class Gpu:
    """The entry points as the suites of row_kernel_cases call them."""

    # ---- LayerNorm
    def ln_fwd(self, case, x, res, gamma, beta, pe, pe_rows, eps):
        L = _lib()
        rows, d = x.shape
        off = case.offset
        xi, ri = _in(x, off), _in(res, off)

        def launch():
            y, mean, rstd = Out((rows, d), x.dtype, off=off), Out(rows, F32), Out(rows, F32)
            L.call("fpnmt_layernorm_fwd", L.dtype_code(x.dtype), rows, d, eps, _p(xi), _p(ri), _p(gamma), _p(beta),
                   _p(pe), pe_rows, _p(y), _p(mean), _p(rstd), L.stream_ptr())
            return [y, mean, rstd]
        return tuple(_twice(launch))

    def ln_bwd(self, case, x, res, gamma, mean, rstd, dy, dg0, db0, p, seed, sd):
        L = _lib()
        rows, d = x.shape
        off = case.offset
        xi, ri, dyi, sdt = _in(x, off), _in(res, off), _in(dy, off), _sd(sd)

        def launch():
            dx = Out((rows, d), x.dtype, off=off)
            dg, db = (Out(d, F32, dg0), Out(d, F32, db0)) if dg0 is not None else (None, None)
            head = (L.dtype_code(x.dtype), rows, d, _p(xi), _p(ri), _p(gamma), _p(mean), _p(rstd), _p(dyi), _p(dx),
                    _p(dg), _p(db))
            if p > 0:
                dz = Out((rows, d), x.dtype, off=off)
                L.call("fpnmt_layernorm_bwd_drop", *head, p, seed, _p(sdt), _p(dz), L.stream_ptr())
            else:
                dz = None
                L.call("fpnmt_layernorm_bwd", *head, L.stream_ptr())
            return [dx, dg, db, dz]
        return tuple(_twice(launch))

    # ---- broadcast form
    def bcast_fwd(self, case, c, cbias, p, seed, sd, res, gamma, beta, eps, want_x):
        L = _lib()
        rows, d = res.shape
        sdt = _sd(sd)

        def launch():
            y, mean, rstd = Out((rows, d), res.dtype), Out(rows, F32), Out(rows, F32)
            xo = Out((rows, d), res.dtype) if want_x else None
            L.call("fpnmt_layernorm_bcast_fwd", L.dtype_code(res.dtype), rows, d, case.t, eps, _p(c), _p(cbias), p,
                   seed, _p(sdt), _p(res), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(xo), L.stream_ptr())
            return [y, mean, rstd, xo]
        return tuple(_twice(launch))

    def bcast_bwd(self, case, c, cbias, p, seed, sd, res, gamma, mean, rstd, dy, dg0, db0):
        L = _lib()
        rows, d = res.shape
        sdt = _sd(sd)

        def launch():
            dx, dg, db = Out((rows, d), res.dtype), Out(d, F32, dg0), Out(d, F32, db0)
            dz = Out((rows, d), res.dtype) if p > 0 else None
            L.call("fpnmt_layernorm_bcast_bwd", L.dtype_code(res.dtype), rows, d, case.t, _p(c), _p(cbias), p, seed,
                   _p(sdt), _p(res), _p(gamma), _p(mean), _p(rstd), _p(dy), _p(dx), _p(dg), _p(db), _p(dz),
                   L.stream_ptr())
            return [dx, dg, db, dz]
        return tuple(_twice(launch))

    # ---- views
    @staticmethod
    def _offs(case):
        return [1 if i == case.misaligned else 0 for i in range(len(case.rows))]

    def views_fwd(self, case, xs, gamma, beta, pe, pe_rows, seeds, p, sd, eps):
        L = _lib()
        d, dt, n = case.d, case.dtype, len(xs)
        offs = self._offs(case)
        xi = [_in(x, o) for x, o in zip(xs, offs)]
        sdt = _sd(sd)

        def launch():
            tab = (L.LnView * n)()
            outs = []
            for i, x in enumerate(xi):
                r = x.shape[0]
                y, mean, rstd = Out((r, d), dt, off=offs[i]), Out(r, F32), Out(r, F32)
                tab[i].x, tab[i].y, tab[i].mean, tab[i].rstd = _p(x), _p(y), _p(mean), _p(rstd)
                tab[i].rows, tab[i].pe_rows, tab[i].seed = r, pe_rows[i], seeds[i]
                outs += [y, mean, rstd]
            L.call("fpnmt_layernorm_views_fwd", L.dtype_code(dt), n, d, eps, tab, _p(gamma), _p(beta), _p(pe), p,
                   _p(sdt), L.stream_ptr())
            return outs
        got = _twice(launch)
        res = [tuple(got[3 * i:3 * i + 3]) for i in range(n)]
        if case.misaligned < 0:  # bit for bit the views launched one by one
            for i, x in enumerate(xi):
                r = x.shape[0]
                if r == 0:
                    continue
                y, mean, rstd, y2 = Out((r, d), dt), Out(r, F32), Out(r, F32), Out((r, d), dt)
                L.call("fpnmt_layernorm_fwd", L.dtype_code(dt), r, d, eps, _p(x), None, _p(gamma), _p(beta), _p(pe),
                       pe_rows[i], _p(y), _p(mean), _p(rstd), L.stream_ptr())
                if p > 0:
                    L.call("fpnmt_dropout", L.dtype_code(dt), r * d, p, seeds[i], _p(sdt), _p(y), _p(y2), L.stream_ptr())
                torch.cuda.synchronize()
                one = ((y2 if p > 0 else y).live(), mean.live(), rstd.live())
                for a, b in zip(res[i], one):
                    assert torch.equal(_bits(a), _bits(b)), f"view {i}: fused and single launches differ"
        return res

    def views_bwd(self, case, xs, gamma, stats, dys, seeds, p, sd, dg0, db0):
        L = _lib()
        d, dt, n = case.d, case.dtype, len(xs)
        offs = self._offs(case)
        xi = [_in(x, o) for x, o in zip(xs, offs)]
        dyi = [_in(t, o) for t, o in zip(dys, offs)]
        sdt = _sd(sd)

        def launch():
            tab = (L.LnView * n)()
            outs = []
            for i, x in enumerate(xi):
                r = x.shape[0]
                dx = Out((r, d), dt, off=offs[i])
                tab[i].x, tab[i].y, tab[i].dy = _p(x), _p(dx), _p(dyi[i])
                tab[i].mean, tab[i].rstd = _p(stats[i][0]), _p(stats[i][1])
                tab[i].rows, tab[i].pe_rows, tab[i].seed = r, 1, seeds[i]
                outs.append(dx)
            dg, db = Out(d, F32, dg0), Out(d, F32, db0)
            L.call("fpnmt_layernorm_views_bwd", L.dtype_code(dt), n, d, tab, _p(gamma), p, _p(sdt), _p(dg), _p(db),
                   L.stream_ptr())
            return outs + [dg, db]
        got = _twice(launch)
        dxs, dg, db = got[:n], got[n], got[n + 1]
        if case.misaligned < 0:  # bit for bit the views launched one by one, the gradients adding in view order
            g1, b1 = Out(d, F32, dg0), Out(d, F32, db0)
            for i, x in enumerate(xi):
                r = x.shape[0]
                if r == 0:
                    continue
                dyp, dx = Out((r, d), dt), Out((r, d), dt)
                if p > 0:
                    L.call("fpnmt_dropout", L.dtype_code(dt), r * d, p, seeds[i], _p(sdt), _p(dyi[i]), _p(dyp),
                           L.stream_ptr())
                L.call("fpnmt_layernorm_bwd", L.dtype_code(dt), r, d, _p(x), None, _p(gamma), _p(stats[i][0]),
                       _p(stats[i][1]), _p(dyp) if p > 0 else _p(dyi[i]), _p(dx), _p(g1), _p(b1), L.stream_ptr())
                torch.cuda.synchronize()
                assert torch.equal(_bits(dx.live()), _bits(dxs[i])), f"view {i}: fused and single launches differ"
            assert torch.equal(_bits(g1.live()), _bits(dg)) and torch.equal(_bits(b1.live()), _bits(db))
        return dxs, dg, db

    # ---- embedding
    def embed_fwd(self, case, dtype, tok, emb, pe, p, seed, sd):
        L = _lib()
        sdt = _sd(sd)

        def launch():
            y = Out((case.b * case.t, case.d), dtype)
            head = (L.dtype_code(dtype), case.b, case.t, case.d, _p(tok), _p(emb), _p(pe), _p(y))
            if p > 0:
                L.call("fpnmt_embed_posenc_fwd_drop", *head, p, seed, _p(sdt), L.stream_ptr())
            else:
                L.call("fpnmt_embed_posenc_fwd", *head, L.stream_ptr())
            return [y]
        return _twice(launch)[0]

    def embed_bwd(self, case, tok, dy, de0, sumsq0, p, seed, sd):
        L = _lib()
        sdt = _sd(sd)

        def launch():
            de = Out(tuple(de0.shape), F32, de0)
            sq = Out(1, F32, sumsq0) if sumsq0 is not None else None
            head = (L.dtype_code(dy.dtype), case.b, case.t, case.d, _p(tok), _p(dy), _p(de), _p(sq))
            if p > 0:
                L.call("fpnmt_embed_posenc_bwd_drop", *head, p, seed, _p(sdt), L.stream_ptr())
            else:
                L.call("fpnmt_embed_posenc_bwd", *head, L.stream_ptr())
            return [de, sq]
        return tuple(_twice(launch))

    # ---- cross-entropy
    def xent(self, case, x, lab, dtype, gscale, want_d):
        L = _lib()
        rows, v = x.shape
        ld, ldd = v + C.XENT_LD, v + C.XENT_LDD
        xin = torch.full((rows, ld), float("nan"), device=DEV)  # a read of the gap poisons the row
        xin[:, :v] = x

        def launch():
            loss = Out(1, F32)
            dl = Out((rows, ldd), dtype) if want_d else None
            L.call("fpnmt_xent_fwd_bwd", L.dtype_code(dtype), rows, v, _p(xin), ld, _p(lab), _p(loss), _p(dl), ldd,
                   gscale, L.stream_ptr())
            return [loss, dl]
        loss, dl = _twice(launch)
        if dl is None:
            return loss, None
        gap = dl[:, v:]
        assert torch.equal(_bits(gap), _bits(torch.full_like(gap, C.SENTINEL))), "the ldd gap was written"
        return loss, dl[:, :v]

    # ---- activation backward
    def act_bwd(self, case, dtype, act, dy, y, db0, p, seed, sd):
        L = _lib()
        rows, c = dy.shape
        off = case.offset
        dyi, yi, sdt = _in(dy, off), _in(y, off), _sd(sd)

        def launch():
            dz = Out((rows, c), dtype, off=off)
            db = Out(c, F32, db0) if db0 is not None else None
            L.call("fpnmt_act_bwd", L.dtype_code(dtype), rows, c, getattr(L, _ACT[act]), C.LEAKY, _p(dyi), _p(yi),
                   _p(dz), _p(db), None, p, seed, _p(sdt), L.stream_ptr())
            return [dz, db]
        dz, db = _twice(launch)
        if act == "none" and p == 0 and db is not None:
            self.db_none = db  # bias_grad must reproduce these bits
        return dz, db

    def bias_grad(self, case, dtype, dy, db0):
        L = _lib()
        rows, c = dy.shape
        dyi = _in(dy, case.offset)

        def launch():
            db = Out(c, F32, db0)
            L.call("fpnmt_bias_grad", L.dtype_code(dtype), rows, c, _p(dyi), _p(db), L.stream_ptr())
            return [db]
        db = _twice(launch)[0]
        if "none" in case.acts:
            assert torch.equal(_bits(db), _bits(self.db_none)), "bias_grad and act_bwd's db differ"
        return db

    # ---- dropout, cast, add
    def cast(self, x, dtype):
        L = _lib()

        def launch():
            y = Out(x.numel(), dtype)
            L.call("fpnmt_cast", L.dtype_code(x.dtype), L.dtype_code(dtype), x.numel(), _p(x), _p(y), L.stream_ptr())
            return [y]
        return _twice(launch)[0]

    def add(self, a, b):
        L = _lib()

        def launch():
            y = Out(a.numel(), a.dtype)
            L.call("fpnmt_add", L.dtype_code(a.dtype), a.numel(), _p(a), _p(b), _p(y), L.stream_ptr())
            return [y]
        return _twice(launch)[0]

    def dropout(self, x, p, seed, sd):
        L = _lib()
        sdt = _sd(sd)

        def launch():
            y = Out(x.numel(), x.dtype)
            L.call("fpnmt_dropout", L.dtype_code(x.dtype), x.numel(), p, seed, _p(sdt), _p(x), _p(y), L.stream_ptr())
            return [y]
        return _twice(launch)[0]


def _report(tag, name, dtype, rows):
    ratios, bad = C.worst(rows)
    fam = {}
    for k, v in ratios.items():
        f = k.split("[")[0]
        fam[f] = max(fam.get(f, 0.0), v)
    top = max(ratios, key=ratios.get)
    print(f"\nratio {tag} {name} {C.short(dtype) if dtype else '-'}: worst {ratios[top]:.3f} at {top}; "
          + " ".join(f"{k}={v:.3f}" for k, v in fam.items()))
    assert not bad, {k: ratios[k] for k in bad}


def _params(cases):
    return [pytest.param(c.name, dt, id=f"{c.name}-{C.short(dt)}") for c in cases for dt in c.dtypes]


@pytest.mark.parametrize("name,dtype", _params(C.LN_CASES))
def test_layernorm_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("ln", name, dtype, C.ln_suite(C.LN_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name,dtype", _params(C.BCAST_CASES))
def test_layernorm_bcast_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("bcast", name, dtype, C.bcast_suite(C.BCAST_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name", [c.name for c in C.VIEWS_CASES])
def test_layernorm_views_entry_points(name):
    torch.cuda.set_device(0)
    case = C.VIEWS_BY_NAME[name]
    _report("views", name, case.dtype, C.views_suite(case, Gpu(), DEV))


@pytest.mark.parametrize("name,dtype", _params(C.EMB_CASES))
def test_embedding_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("embed", name, dtype, C.emb_suite(C.EMB_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name", [c.name for c in C.XENT_CASES])
def test_xent_entry_point(name):
    torch.cuda.set_device(0)
    rows = C.xent_suite(C.XENT_BY_NAME[name], Gpu(), DEV)
    _report("xent", name, None, rows)
    if name == "all_pad":  # exactly zero, not merely inside a bound
        for label, got, ref, bnd in rows:
            assert float(got.double().abs().max()) == 0.0, label


@pytest.mark.parametrize("name,dtype", _params(C.ACT_CASES))
def test_act_bwd_and_bias_grad_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("act", name, dtype, C.act_suite(C.ACT_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("n", C.FLAT_SIZES)
def test_dropout_cast_add_are_exact(n):
    torch.cuda.set_device(0)
    _report("flat", str(n), None, C.flat_suite(n, Gpu(), DEV))


def test_absent_embedding_rows_stay_bit_identical():
    torch.cuda.set_device(0)
    case = C.EMB_BY_NAME["d300"]
    inp = {k: v.to(DEV) for k, v in C.emb_inputs(case, BF16).items()}
    de, _ = Gpu().embed_bwd(case, inp["tok"], inp["dy"], inp["d_emb0"], inp["sumsq0"], 0.0, 0, None)
    absent = torch.ones(C.VOCAB, dtype=torch.bool, device=DEV)
    absent[inp["tok"].long()] = False
    assert int(absent.sum()) >= 1
    assert torch.equal(_bits(de[absent]), _bits(inp["d_emb0"][absent]))

"""The spatial kernels of csrc/elementwise.hip (max pooling forward, its three
backward routes and the fused activation derivative; the FPN top-down pathway
forward and backward; the co-attention spatial softmax forward and backward)
element by element against fp64, on the case table of
tests/spatial_kernel_cases.py (whose bounds tests/test_spatial_kernel_bars.py
proves able to fail).

The C entry points are called directly through fpnmt._lib. For every case and
dtype:

1. every output element is within its derived bound of the fp64 reference
   computed from the exact stored inputs (the worst err / bound ratio of each
   output is printed; exact outputs report 0);
2. every output, the uint8 argmax and the fp64 da workspace included, is
   allocated with guard elements holding a sentinel after it (and before it
   where the case shifts the pointers), which come back bitwise untouched;
   d_lat5 is pre-filled, so `=` for `+=` fails 1., and dx is pre-filled with the
   sentinel, so an input no window covers must be written with +0;
3. a second run into fresh buffers is bitwise equal;
4. routes that must agree do so bit for bit: the pool backward's tile form,
   the gather form recomputing the argmax and the scalar gather form; the
   fused activation backward and the plain backward times the 0 / 1 mask; the
   in-register P4m of the P3m path and the stored P4m (through the exact
   integer cases);
5. error returns raise and leave the outputs at the sentinel: leaky with
   overlapping windows, an unsupported act, channels no multiple of the vector
   width, an FPN pointer off a 16-byte boundary.
"""
import pytest
import torch

import spatial_kernel_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8
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
        self.shape = tuple(shape)
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.off = off
        self.fill = S.AM_SENTINEL if dtype == U8 else S.SENTINEL
        self.buf = torch.full((off + self.n + S.GUARD,), self.fill, dtype=dtype, device=DEV)
        if init is not None:
            self.buf[off:off + self.n] = init.reshape(-1)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def live(self):
        return self.buf[self.off:self.off + self.n].view(self.shape)

    def guards_untouched(self):
        g = torch.cat([self.buf[:self.off], self.buf[self.off + self.n:]])
        return torch.equal(_bits(g), _bits(torch.full_like(g, self.fill)))

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(torch.full_like(self.buf, self.fill)))


def _in(t, off=0):
    """t at a pointer shifted by `off` elements from an aligned allocation."""
    if t is None or off == 0:
        return None if t is None else t.contiguous()
    b = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    b[off:] = t.reshape(-1)
    return b[off:].view(t.shape)


def _p(t):
    return None if t is None else (t.ptr if isinstance(t, Out) else t.data_ptr())


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


class Gpu:
    """The entry points as the suites of spatial_kernel_cases call them."""

    # ---- max pool
    def pool_fwd(self, case, x, want_am, off):
        L = _lib()
        xi = _in(x, off)
        shape = (case.n, case.ho, case.wo, case.c)

        def launch():
            y = Out(shape, x.dtype, off=off)
            am = Out(shape, U8, off=off) if want_am else None
            L.call("fpnmt_maxpool2d_fwd", L.dtype_code(x.dtype), *case.geo, _p(xi), _p(y), _p(am), L.stream_ptr())
            return [y, am]
        return tuple(_twice(launch))

    def pool_bwd(self, case, dtype, x, am, dy, off):
        L = _lib()
        xi, ami, dyi = _in(x, off), _in(am, off), _in(dy, off)

        def launch():
            dx = Out((case.n, case.h, case.w, case.c), dtype, off=off)
            L.call("fpnmt_maxpool2d_bwd", L.dtype_code(dtype), *case.geo, _p(xi), _p(ami), _p(dyi), _p(dx), L.stream_ptr())
            return [dx]
        return _twice(launch)[0]

    def pool_bwd_act(self, case, am, dy, xact, act, alpha, off):
        L = _lib()
        ami, dyi, xi = _in(am, off), _in(dy, off), _in(xact, off)

        def launch():
            dx = Out((case.n, case.h, case.w, case.c), dy.dtype, off=off)
            L.call("fpnmt_maxpool2d_bwd_act", L.dtype_code(dy.dtype), *case.geo, _p(ami), _p(dyi), _p(xi),
                   S.ACT_CODE[act], alpha, _p(dx), L.stream_ptr())
            return [dx]
        return _twice(launch)[0]

    # ---- FPN
    def fpn_fwd(self, case, l5, l4, l3):
        L = _lib()
        n, c = l5.shape[0], l5.shape[3]
        h5, w5, h4, w4, h3, w3 = case.sizes

        def launch():
            p4m = Out((n, h4, w4, c), l5.dtype)
            p3m = Out((n, h3, w3, c), l5.dtype) if l3 is not None else None
            L.call("fpnmt_fpn_topdown_fwd", L.dtype_code(l5.dtype), n, c, *case.sizes, _p(l5), _p(l4), _p(l3), _p(p4m),
                   _p(p3m), L.stream_ptr())
            return [p4m, p3m]
        return tuple(_twice(launch))

    def fpn_bwd(self, case, dp4, dp3, dl5_0, acc):
        L = _lib()
        n, c = dp4.shape[0], dp4.shape[3]

        def launch():
            dl4, dl5 = Out(tuple(dp4.shape), dp4.dtype), Out(tuple(dl5_0.shape), dp4.dtype, dl5_0)
            L.call("fpnmt_fpn_topdown_bwd", L.dtype_code(dp4.dtype), n, c, *case.sizes, _p(dp4), _p(dp3), _p(dl4),
                   _p(dl5), acc, L.stream_ptr())
            return [dl4, dl5]
        return tuple(_twice(launch))

    # ---- spatial softmax
    def ssm_fwd(self, case, score, hs):
        L = _lib()
        n, hw, c = case.n, case.hw, case.c

        def launch():
            ctx, a = Out((n, hw, c), hs.dtype), Out((n, hw), F32)
            L.call("fpnmt_spatial_softmax_fwd", L.dtype_code(hs.dtype), n, hw, c, _p(score), _p(hs), _p(ctx), _p(a),
                   L.stream_ptr())
            return [ctx, a]
        return tuple(_twice(launch))

    def ssm_bwd(self, case, a, hs, dctx):
        L = _lib()
        n, hw, c = case.n, case.hw, case.c

        def launch():
            d_score, d_hs, da = Out((n, hw), hs.dtype), Out((n, hw, c), hs.dtype), Out((n, hw), F64)
            L.call("fpnmt_spatial_softmax_bwd", L.dtype_code(hs.dtype), n, hw, c, _p(a), _p(hs), _p(dctx), _p(d_score),
                   _p(d_hs), _p(da), L.stream_ptr())
            return [d_score, d_hs, da]
        return tuple(_twice(launch))


def _report(tag, name, dtype, rows, pairs):
    ratios, bad = S.worst(rows)
    fam = {}
    for k, v in ratios.items():
        f = k.split("[")[0]
        fam[f] = max(fam.get(f, 0.0), v)
    top = max(ratios, key=ratios.get)
    print(f"\nratio {tag} {name} {S.short(dtype)}: worst {ratios[top]:.3f} at {top}; "
          + " ".join(f"{k}={v:.3f}" for k, v in fam.items()))
    assert not bad, {k: ratios[k] for k in bad}
    for label, a, b in pairs:
        assert torch.equal(_bits(a), _bits(b)), label
    return fam


def _params(cases, dtypes=None):
    return [pytest.param(c.name, dt, id=f"{c.name}-{S.short(dt)}") for c in cases for dt in (dtypes or c.dtypes)]


@pytest.mark.parametrize("name,dtype", _params(S.POOL_CASES, S.POOL_DTYPES))
def test_maxpool_entry_points(name, dtype):
    torch.cuda.set_device(0)
    fam = _report("pool", name, dtype, *S.pool_suite(S.POOL_BY_NAME[name], dtype, Gpu(), DEV))
    assert fam.get("pool.y", 0.0) == 0.0 and fam.get("pool.argmax", 0.0) == 0.0


@pytest.mark.parametrize("name,dtype", _params(S.FPN_CASES))
def test_fpn_topdown_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("fpn", name, dtype, *S.fpn_suite(S.FPN_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name,dtype", _params(S.SSM_CASES, S.SSM_DTYPES))
def test_spatial_softmax_entry_points(name, dtype):
    torch.cuda.set_device(0)
    rows, pairs = S.ssm_suite(S.SSM_BY_NAME[name], dtype, Gpu(), DEV)
    _report("ssm", name, dtype, rows, pairs)
    if name == "hw1":  # exactly, not merely inside a bound
        got = {r[0]: r[1] for r in rows}
        assert bool((got["ssm.a"] == 1).all()) and bool((got["ssm.d_score"] == 0).all())


@pytest.mark.parametrize("name", ["ragged_4x5", "fp32_index", "upsample_down"])
def test_fpn_adjoint_identity_is_exact(name):
    torch.cuda.set_device(0)
    lhs, rhs = S.fpn_adjoint(S.FPN_BY_NAME[name], Gpu(), DEV)
    assert lhs == rhs and lhs != 0.0, (lhs, rhs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=S.short)
def test_maxpool_bwd_act_error_returns_leave_dx_untouched(dtype):
    torch.cuda.set_device(0)
    L = _lib()
    for name, act, why in S.POOL_ACT_ERRORS:
        case = S.POOL_BY_NAME[name]
        inp = {k: v.to(DEV) for k, v in S.pool_inputs(case, dtype, "ties").items()}
        am = S.pool_fwd_ref(case, inp["x"])[1]
        dx = Out((case.n, case.h, case.w, case.c), dtype)
        with pytest.raises(RuntimeError):
            L.call("fpnmt_maxpool2d_bwd_act", L.dtype_code(dtype), *case.geo, _p(am), _p(inp["dy"]), _p(inp["xact"]), act,
                   S.LEAKY, _p(dx), L.stream_ptr())
        torch.cuda.synchronize()
        assert dx.untouched(), why
    case = S.POOL_BY_NAME["valid_7x7"]
    dy = S.pool_inputs(case, dtype, "ties")["dy"].to(DEV)
    dx = Out((case.n, case.h, case.w, case.c), dtype)
    with pytest.raises(RuntimeError):  # neither x nor argmax
        L.call("fpnmt_maxpool2d_bwd", L.dtype_code(dtype), *case.geo, None, None, _p(dy), _p(dx), L.stream_ptr())
    torch.cuda.synchronize()
    assert dx.untouched()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=S.short)
def test_fpn_error_returns_leave_the_outputs_untouched(dtype):
    """c % vn != 0, and every pointer in turn shifted one element off its
    16-byte boundary: an error before any launch."""
    torch.cuda.set_device(0)
    L = _lib()
    case = S.FPN_BY_NAME["ragged_4x5"]
    n = case.n
    h5, w5, h4, w4, h3, w3 = case.sizes
    vn = S.FPN_VN[dtype]

    def run(c, shift):
        inp = {k: v.to(DEV) for k, v in S.fpn_inputs(case, dtype, c, "randn").items()}
        o = lambda i: 1 if shift == i else 0
        p4m, p3m = Out((n, h4, w4, c), dtype, off=o(3)), Out((n, h3, w3, c), dtype, off=o(4))
        with pytest.raises(RuntimeError):
            L.call("fpnmt_fpn_topdown_fwd", L.dtype_code(dtype), n, c, *case.sizes, _p(_in(inp["l5"], o(0))),
                   _p(_in(inp["l4"], o(1))), _p(_in(inp["l3"], o(2))), _p(p4m), _p(p3m), L.stream_ptr())
        dl4, dl5 = Out((n, h4, w4, c), dtype, off=o(2)), Out((n, h5, w5, c), dtype, off=o(3))
        if shift == 4:
            return p4m, p3m
        with pytest.raises(RuntimeError):
            L.call("fpnmt_fpn_topdown_bwd", L.dtype_code(dtype), n, c, *case.sizes, _p(_in(inp["dp4"], o(0))),
                   _p(_in(inp["dp3"], o(1))), _p(dl4), _p(dl5), 0, L.stream_ptr())
        return p4m, p3m, dl4, dl5

    outs = list(run(vn // 2 * 3, None))  # 12 (bf16) / 6 (fp32) channels
    for shift in range(5):
        outs += run(3 * vn, shift)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)

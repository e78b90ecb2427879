"""The fpnmt_bn_* / fpnmt_depthwise_* entry points (csrc/mobilenet.hip)
element by element against fp64, on the case table of tests/bn_dw_cases.py
(whose bounds tests/test_bn_dw_bars.py proves able to fail).

The C entry points are called directly through fpnmt._lib with the workspace
the package installs. For every case, dtype, activation and residual form:

1. every output element is within its derived bound of the fp64 reference
   computed from the exact stored inputs (the worst err / bound ratio of each
   output is printed);
2. every output is allocated with trailing guard elements holding a sentinel,
   which come back bitwise untouched (pre-filled gradient accumulators come
   back as old + sum, so `=` for `+=` fails 1.);
3. a second run into fresh buffers is bitwise equal (fixed-order reductions,
   no atomics);
4. contract: bad channel counts, kernels over 3x3 and a single null moving
   pointer are rejected; empty problems succeed and write nothing (the sync
   entry points write all-zero sums instead: rank 2 of the sync cases).

The sync entry points run as three ranks in one process (two uneven shards
and one without rows), their fp64 sums added on the device in place of the
all-reduce: no process group.
"""
import inspect

import pytest
import torch

import bn_dw_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _lib():
    from fpnmt import _lib as L
    return L


def _bits(t):
    return t.view(_INT[t.element_size()])


def _buf(numel, dtype, init=None):
    """numel outputs (the sentinel, or `init`) followed by GUARD sentinel elements."""
    b = torch.full((numel + C.GUARD,), C.SENTINEL, dtype=dtype, device=DEV)
    if init is not None:
        b[:numel] = init.reshape(-1)
    return b


def _twice(launch):
    """launch() -> [(buffer, live elements, shape)]. Runs it twice into fresh
    buffers: bitwise equal, guards untouched; returns the first run's views."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    views = []
    for (ba, n, shape), (bb, _, _) in zip(a, b):
        if ba is None:
            views.append(None)
            continue
        assert torch.equal(_bits(ba), _bits(bb)), "two runs differ"
        guard = torch.full((C.GUARD,), C.SENTINEL, dtype=ba.dtype, device=DEV)
        assert torch.equal(_bits(ba[n:]), _bits(guard)), "guard elements overwritten"
        views.append(ba[:n].view(shape))
    return views


def _act(act):
    L = _lib()
    return L.ACT_RELU6 if act == "relu6" else L.ACT_NONE


class Gpu:
    """The entry points as the suites of bn_dw_cases call them."""

    def stats(self, x, mm, mv, momentum):
        L = _lib()
        rows, c = x.shape

        def launch():
            mean, var = _buf(c, F32), _buf(c, F32)
            m2, v2 = (_buf(c, F32, mm), _buf(c, F32, mv)) if mm is not None else (None, None)
            L.call("fpnmt_bn_stats", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(mean), L.ptr(var), L.ptr(m2),
                   L.ptr(v2), momentum, L.stream_ptr())
            return [(mean, c, (c,)), (var, c, (c,)), (m2, c, (c,)), (v2, c, (c,))]
        return tuple(_twice(launch))

    def stats_sums(self, x):
        L = _lib()
        rows, c = x.shape

        def launch():
            sums = _buf(2 * c + 1, F64)
            L.call("fpnmt_bn_stats_sums", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(sums), L.stream_ptr())
            return [(sums, 2 * c + 1, (2 * c + 1,))]
        return _twice(launch)[0]

    def finalize(self, sums, mm, mv, momentum):
        L = _lib()
        c = (sums.numel() - 1) // 2
        sums = sums.contiguous()

        def launch():
            mean, var, m2, v2 = _buf(c, F32), _buf(c, F32), _buf(c, F32, mm), _buf(c, F32, mv)
            L.call("fpnmt_bn_stats_finalize", c, L.ptr(sums), L.ptr(mean), L.ptr(var), L.ptr(m2), L.ptr(v2), momentum,
                   L.stream_ptr())
            return [(mean, c, (c,)), (var, c, (c,)), (m2, c, (c,)), (v2, c, (c,))]
        return tuple(_twice(launch))

    def apply(self, x, mean, var, gamma, beta, act, res):
        L = _lib()
        rows, c = x.shape

        def launch():
            y = _buf(rows * c, x.dtype)
            L.call("fpnmt_bn_apply", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(mean), L.ptr(var), L.ptr(gamma),
                   L.ptr(beta), C.EPS, _act(act), L.ptr(res), L.ptr(y), L.stream_ptr())
            return [(y, rows * c, (rows, c))]
        return _twice(launch)[0]

    def bwd(self, x, mean, var, gamma, act, y, dy, dg0, db0):
        L = _lib()
        rows, c = x.shape

        def launch():
            dx = _buf(rows * c, x.dtype)
            dg, db = (_buf(c, F32, dg0), _buf(c, F32, db0)) if dg0 is not None else (None, None)
            L.call("fpnmt_bn_bwd", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(mean), L.ptr(var), L.ptr(gamma),
                   C.EPS, _act(act), L.ptr(y), L.ptr(dy), L.ptr(dx), L.ptr(dg), L.ptr(db), L.stream_ptr())
            return [(dx, rows * c, (rows, c)), (dg, c, (c,)), (db, c, (c,))]
        return tuple(_twice(launch))

    def bwd_sums(self, x, mean, var, act, y, dy, dg0, db0):
        L = _lib()
        rows, c = x.shape

        def launch():
            sums, dg, db = _buf(2 * c + 1, F64), _buf(c, F32, dg0), _buf(c, F32, db0)
            L.call("fpnmt_bn_bwd_sums", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(mean), L.ptr(var), C.EPS,
                   _act(act), L.ptr(y), L.ptr(dy), L.ptr(sums), L.ptr(dg), L.ptr(db), L.stream_ptr())
            return [(sums, 2 * c + 1, (2 * c + 1,)), (dg, c, (c,)), (db, c, (c,))]
        return tuple(_twice(launch))

    def bwd_dx(self, x, mean, var, gamma, act, y, dy, sums, rank):
        L = _lib()
        rows, c = x.shape
        sums = sums.contiguous()

        def launch():
            dx = _buf(rows * c, x.dtype)
            L.call("fpnmt_bn_bwd_dx", L.dtype_code(x.dtype), rows, c, L.ptr(x), L.ptr(mean), L.ptr(var), L.ptr(gamma),
                   C.EPS, _act(act), L.ptr(y), L.ptr(dy), L.ptr(sums), L.ptr(dx), L.stream_ptr())
            return [(dx, rows * c, (rows, c))]
        return _twice(launch)[0]

    @staticmethod
    def _geom(case, shape):
        return (*shape, *case.k, case.stride, *case.pads)

    def dw_fwd(self, case, x, w):
        L = _lib()
        n, h, wd, c = x.shape
        ho, wo = case.out_hw(tuple(x.shape))

        def launch():
            y = _buf(n * ho * wo * c, x.dtype)
            L.call("fpnmt_depthwise_fwd", L.dtype_code(x.dtype), *self._geom(case, x.shape), L.ptr(x), L.ptr(w),
                   L.ptr(y), L.stream_ptr())
            return [(y, n * ho * wo * c, (n, ho, wo, c))]
        return _twice(launch)[0]

    def dw_bwd_data(self, case, dy, w, shape):
        L = _lib()

        def launch():
            dx = _buf(shape[0] * shape[1] * shape[2] * shape[3], dy.dtype)
            L.call("fpnmt_depthwise_bwd_data", L.dtype_code(dy.dtype), *self._geom(case, shape), L.ptr(dy), L.ptr(w),
                   L.ptr(dx), L.stream_ptr())
            return [(dx, shape[0] * shape[1] * shape[2] * shape[3], tuple(shape))]
        return _twice(launch)[0]

    def dw_bwd_filter(self, case, x, dy, dw0):
        L = _lib()
        ne = dw0.numel()

        def launch():
            dw = _buf(ne, F32, dw0)  # the filter gradient accumulates: pre-filled non-zero
            L.call("fpnmt_depthwise_bwd_filter", L.dtype_code(x.dtype), *self._geom(case, x.shape), L.ptr(x),
                   L.ptr(dy), L.ptr(dw), L.stream_ptr())
            return [(dw, ne, tuple(dw0.shape))]
        return _twice(launch)[0]


ENTRY_POINTS = ["fpnmt_bn_stats", "fpnmt_bn_apply", "fpnmt_bn_bwd", "fpnmt_bn_stats_sums", "fpnmt_bn_stats_finalize",
                "fpnmt_bn_bwd_sums", "fpnmt_bn_bwd_dx", "fpnmt_depthwise_fwd", "fpnmt_depthwise_bwd_data",
                "fpnmt_depthwise_bwd_filter"]


def _report(tag, name, dtype, rows):
    ratios, bad = C.worst(rows)
    top = max(ratios, key=ratios.get)
    short = str(dtype).replace("torch.", "")
    print(f"\nratio {tag} {name} {short}: worst {ratios[top]:.3f} at {top}; "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert not bad, {k: ratios[k] for k in bad}


def _params(cases):
    return [pytest.param(c.name, dt, id=f"{c.name}-{str(dt).replace('torch.', '')}") for c in cases for dt in c.dtypes]


@pytest.mark.parametrize("name,dtype", _params(C.BN_CASES))
def test_batchnorm_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("bn", name, dtype, C.bn_suite(C.BN_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name,dtype", _params([C.BN_BY_NAME[n] for n in C.SYNC_CASES]))
def test_sync_entry_points_as_three_ranks(name, dtype):
    torch.cuda.set_device(0)
    _report("sync", name, dtype, C.bn_sync_suite(C.BN_BY_NAME[name], dtype, Gpu(), DEV))


@pytest.mark.parametrize("name,dtype", _params(C.DW_CASES))
def test_depthwise_entry_points(name, dtype):
    torch.cuda.set_device(0)
    _report("dw", name, dtype, C.dw_suite(C.DW_BY_NAME[name], dtype, Gpu(), DEV))


def test_every_entry_point_has_a_case():
    src = inspect.getsource(Gpu)
    for ep in ENTRY_POINTS:
        assert f'"{ep}"' in src, ep
    # and they are all the batch-norm / depthwise entry points the binding declares
    L = _lib()
    assert sorted(ENTRY_POINTS) == sorted(n for n in L.SIGNATURES if n.startswith(("fpnmt_bn_", "fpnmt_depthwise_")))


# ------------------------------------------------------------------- contract
def _sentinel(numel, dtype=F32):
    return torch.full((numel,), C.SENTINEL, dtype=dtype, device=DEV)


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(torch.equal(_bits(t), _bits(_sentinel(t.numel(), t.dtype))) for t in ts)


def test_bad_arguments_are_rejected():
    L = _lib()
    s = L.stream_ptr()
    x = torch.zeros(4, 16, device=DEV)
    v = [torch.zeros(16, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.call("fpnmt_bn_stats", L.F32, 4, 12, L.ptr(x), L.ptr(v[0]), L.ptr(v[1]), None, None, 0.9, s)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.call("fpnmt_bn_apply", L.F32, 4, 12, L.ptr(x), L.ptr(v[0]), L.ptr(v[1]), L.ptr(v[2]), L.ptr(v[3]), C.EPS, 0,
               None, L.ptr(x), s)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.call("fpnmt_depthwise_fwd", L.F32, 1, 2, 2, 12, 3, 3, 1, 1, 1, 1, 1, L.ptr(x), L.ptr(x), L.ptr(x), s)
    for fn in ("fpnmt_depthwise_fwd", "fpnmt_depthwise_bwd_data", "fpnmt_depthwise_bwd_filter"):
        with pytest.raises(RuntimeError, match="kernel <= 3x3"):
            L.call(fn, L.F32, 1, 2, 2, 8, 4, 3, 1, 1, 1, 1, 1, L.ptr(x), L.ptr(x), L.ptr(x), s)
    with pytest.raises(RuntimeError, match="null pointer"):  # one moving pointer without the other
        L.call("fpnmt_bn_stats", L.F32, 4, 16, L.ptr(x), L.ptr(v[0]), L.ptr(v[1]), L.ptr(v[2]), None, 0.9, s)
    sums = torch.ones(33, dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("fpnmt_bn_stats_finalize", 16, L.ptr(sums), L.ptr(v[0]), L.ptr(v[1]), None, L.ptr(v[3]), 0.9, s)
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in v) and float(x.abs().max()) == 0.0  # a rejected call wrote nothing


def test_empty_problems_succeed_and_write_nothing():
    L = _lib()
    s = L.stream_ptr()
    c = 16
    a, b, d = _sentinel(64), _sentinel(64), _sentinel(64)
    m, v, g = _sentinel(c), _sentinel(c), _sentinel(c)
    sums = _sentinel(2 * c + 1, F64)
    L.call("fpnmt_bn_stats", L.F32, 0, c, L.ptr(a), L.ptr(m), L.ptr(v), L.ptr(g), L.ptr(d), 0.9, s)
    L.call("fpnmt_bn_apply", L.F32, 0, c, L.ptr(a), L.ptr(m), L.ptr(v), L.ptr(g), L.ptr(g), C.EPS, 0, None, L.ptr(b), s)
    L.call("fpnmt_bn_bwd", L.F32, 0, c, L.ptr(a), L.ptr(m), L.ptr(v), L.ptr(g), C.EPS, 0, None, L.ptr(a), L.ptr(b),
           L.ptr(g), L.ptr(d), s)
    L.call("fpnmt_bn_bwd_dx", L.F32, 0, c, L.ptr(a), L.ptr(m), L.ptr(v), L.ptr(g), C.EPS, 0, None, L.ptr(a),
           L.ptr(sums), L.ptr(b), s)
    # n == 0, and a 1x1 image under an unpadded 3x3 kernel (ho <= 0)
    for shape in ((0, 2, 2, c), (1, 1, 1, c)):
        L.call("fpnmt_depthwise_fwd", L.F32, *shape, 3, 3, 1, 0, 0, 0, 0, L.ptr(a), L.ptr(d), L.ptr(b), s)
        L.call("fpnmt_depthwise_bwd_filter", L.F32, *shape, 3, 3, 1, 0, 0, 0, 0, L.ptr(a), L.ptr(d), L.ptr(b), s)
    L.call("fpnmt_depthwise_bwd_data", L.F32, 0, 2, 2, c, 3, 3, 1, 0, 0, 0, 0, L.ptr(a), L.ptr(d), L.ptr(b), s)
    assert _untouched(a, b, d, m, v, g, sums)
    # no output pixel but an input: its gradient is exactly zero, nothing past it is written
    L.call("fpnmt_depthwise_bwd_data", L.F32, 1, 1, 1, c, 3, 3, 1, 0, 0, 0, 0, L.ptr(a), L.ptr(d), L.ptr(b), s)
    torch.cuda.synchronize()
    assert float(b[:c].abs().max()) == 0.0 and _untouched(b[c:], a, d)
    # the sync entry points write all-zero sums for a rank without rows
    for fn, args in (("fpnmt_bn_stats_sums", ()), ("fpnmt_bn_bwd_sums", (L.ptr(m), L.ptr(v), C.EPS, 0, None, L.ptr(a)))):
        sums = _sentinel(2 * c + 1 + 8, F64)
        tail = (L.ptr(g), L.ptr(d)) if args else ()
        L.call(fn, L.F32, 0, c, L.ptr(a), *args, L.ptr(sums), *tail, s)
        torch.cuda.synchronize()
        assert float(sums[:2 * c + 1].abs().max()) == 0.0 and _untouched(sums[2 * c + 1:], g, d)

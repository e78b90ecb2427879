"""fpnmt_xent_smooth_fwd_bwd against an fp64 restatement on every load route
and width (the (V, ld) list of tests/test_gpu_scst_kernels.py), its exact
arg-max flag with planted ties, exact zeros, rounding, determinism, the
eps = 0 agreement with fpnmt_xent_weighted_fwd_bwd and its error codes; and
fpnmt_caption_stats.

The reference sees the eps the kernel sees: eps rounded to fp32 (the C ABI
takes a float). Error bounds, with u = 2^-24 (fp32 unit roundoff), X =
max |logit| of the case, V the row width, and the steps of
tests/test_gpu_scst_kernels.py for what the two kernels share:
  s = sum_j exp(x_j - m)                           -> (V + 2X + 2) u relative
  lse = m + log s: s's relative error as an absolute one, logf 2 u log V,
    the addition u (X + log V)              -> B_lse = u (V + 3X + 3 log V + 2)
  logp = x_lab - lse: the subtraction u (2X + log V)
                                       -> B_logp = u (V + 5X + 4 log V + 2)
  ce = (lse - a x_lab) - b S, a = fl(1 - eps), b = fl(eps / V), S = sum_j x_j:
    a x_lab: a's rounding u |x_lab| and the product's u |a x_lab| -> 2 u X
    the first subtraction, on a value <= 2X + log V   -> u (2X + log V)
    S in any order carries at most g A, A = sum_j |x_j|, g = (V - 1) u /
      (1 - (V - 1) u); b's rounding and the product's, u b |S| each
                                                      -> (eps / V) (g + 2u) A
    the second subtraction, on a value <= 3X + log V  -> u (3X + log V)
          -> B_ce = u (V + 10X + 5 log V + 2) + (eps / V) (g + 2u) A    per row
  (at eps = 0 the kernel computes lse - x_lab: B_logp, which is smaller)
  loss = (1 / rows) sum_r ce_r over the live rows, the ordered sum <= rows u
    per term             -> B_loss = (1 / rows) sum_r (B_ce,r + (rows + 2) u |ce_r|)
  grad_j = ((e_j / s - a [j = lab]) - b) coef: e_j / s <= 1 carries
    (V + 4X + 6) u; a's rounding u, that subtraction's u; b's rounding <= u,
    that subtraction's u; coef = dloss_scale / rows one rounding and the
    product's two, 3 u, all on a factor <= 1
                                       -> B_grad = |coef| u (V + 4X + 13)
row_hit compares the given floats and is exact.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
CASES = [(37, 37), (37, 40), (200, 208), (1001, 1001), (4100, 4100), (10000, 10000), (10300, 10304),
         (10243, 10243)]
EPS_CASES = [(v, ld, 0.1) for v, ld in CASES] + [(v, ld, e) for v, ld in ((37, 40), (10000, 10000)) for e in (0.0, 0.5)]
NAME = "fpnmt_xent_smooth_fwd_bwd"


def _lib():
    from fpnmt import _lib as L
    assert hasattr(L.lib, NAME) and hasattr(L.lib, "fpnmt_caption_stats"), f"libfpnmt has no {NAME} / fpnmt_caption_stats"
    return L


@functools.lru_cache(maxsize=None)
def case(v, ld, rows, eps):
    """Inputs and the fp64 reference of one case (built once, shared)."""
    g = torch.Generator().manual_seed(1000 * v + 10 * rows)
    buf = torch.randn(rows, ld, generator=g) * 3
    buf[:, v:] = float("nan")  # the row padding is never read
    lab = torch.randint(1, v, (rows,), generator=g, dtype=torch.int32)
    lab[0] = v - 1
    if rows > 1:
        # pads, the last column, a label in the last (partial) vector, column 1
        lab[1], lab[2], lab[3], lab[5], lab[9] = 0, v - 2, 1, 0, v - 1 - (v % 4) // 2
        lab[10], lab[11], lab[12] = v, v + 5, -3  # outside [0, v): pads, never dereferenced
        # the row maximum twice, at columns a < b: label a hits, label b misses;
        # far apart (other threads) and next to each other (one 16-B vector)
        for r, (a, b, l) in {6: (2, v - 1, 2), 7: (2, v - 1, v - 1), 13: (4, 5, 4), 14: (4, 5, 5)}.items():
            buf[r, a] = buf[r, b] = 20.0
            lab[r] = l
        buf[8, int(lab[8])] = 20.0  # a plain hit
    logits = buf[:, :v]
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    live = ((lab > 0) & (lab < v))
    labc = torch.where(live, lab, torch.zeros_like(lab)).long()
    x64 = logits.double()
    lsm = torch.log_softmax(x64, 1)
    lv = live.double()
    logp = lsm.gather(1, labc[:, None])[:, 0] * lv
    ce = (-(1 - e32) * logp - (e32 / v) * lsm.sum(1)) * lv  # = lse - (1 - eps) x_lab - (eps / v) sum_j x_j
    loss = float(ce.sum() / rows)
    onehot = torch.zeros(rows, v, dtype=torch.float64)
    onehot[torch.arange(rows), labc] = 1.0
    coef = lv / rows
    grad = (lsm.exp() - (1 - e32) * onehot - e32 / v) * coef[:, None]
    first = torch.tensor([int(torch.nonzero(logits[r] == logits[r].max())[0]) for r in range(rows)])
    hit = ((first == labc) & live).int()
    x = float(logits.abs().max())
    gam = (v - 1) * U / (1 - (v - 1) * U)
    b_logp = U * (v + 5 * x + 4 * math.log(v) + 2)
    b_ce = U * (v + 10 * x + 5 * math.log(v) + 2) + (e32 / v) * (gam + 2 * U) * x64.abs().sum(1)
    b_loss = float((lv * (b_ce + (rows + 2) * U * ce.abs())).sum() / rows)
    b_grad = coef * U * (v + 4 * x + 13)
    return dict(buf=buf, lab=lab, live=live, logp=logp, loss=loss, grad=grad, hit=hit, coef=coef, b_logp=b_logp,
                b_grad=b_grad, b_loss=b_loss)


def launch(c, v, ld, eps, dtype=torch.float32, scale=1.0, ldd=None, grad=True):
    L = _lib()
    rows = c["buf"].shape[0]
    ldd = ldd or ld
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    logp = torch.full((rows,), 7.0, device=DEV)
    hit = torch.full((rows,), 7, dtype=torch.int32, device=DEV)
    dlog = torch.full((rows, ldd), 7.0, dtype=dtype, device=DEV)
    L.call(NAME, L.dtype_code(dtype), rows, v, buf.data_ptr(), ld, lab.data_ptr(), eps, loss.data_ptr(),
           logp.data_ptr(), hit.data_ptr(), dlog.data_ptr() if grad else None, ldd, scale, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dlog[:, v if grad else 0:].float() == 7.0).all())  # nothing written past a row's v columns
    return loss.cpu(), logp.cpu(), hit.cpu(), dlog[:, :v].cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("rows", [1, 21])
@pytest.mark.parametrize("v,ld,eps", EPS_CASES, ids=lambda x: str(x))
def test_smoothed_xent_against_fp64(v, ld, eps, rows, parity_record):
    c = case(v, ld, rows, eps)
    loss, logp, hit, dlog = launch(c, v, ld, eps)
    e_loss = abs(float(loss) - c["loss"])
    e_logp = float((logp.double() - c["logp"]).abs().max())
    e_grad = (dlog.double() - c["grad"]).abs()
    worst = float((e_grad.max(1).values / c["b_grad"].clamp_min(1e-300))[c["live"]].max())
    print(f"V={v} ld={ld} rows={rows} eps={eps}: loss err {e_loss:.3e} (bound {c['b_loss']:.3e}), "
          f"logp err {e_logp:.3e} (bound {c['b_logp']:.3e}), grad err / bound {worst:.3e}, hits {int(hit.sum())}")
    parity_record[f"xent_smooth_v{v}_ld{ld}_r{rows}_e{eps}"] = dict(
        loss_err=e_loss, loss_bound=c["b_loss"], logp_err=e_logp, logp_bound=c["b_logp"],
        grad_err=float(e_grad.max()), grad_err_over_bound=worst)
    assert e_loss <= c["b_loss"]
    assert e_logp <= c["b_logp"]
    assert bool((e_grad <= c["b_grad"][:, None]).all())
    # the arg-max flag is exact: planted ties (label a hits, label b misses), pads, labels >= v
    assert torch.equal(hit, c["hit"]), (hit.tolist(), c["hit"].tolist())
    if rows > 1:
        assert [int(hit[r]) for r in (6, 7, 13, 14, 8, 1, 10, 11, 12)] == [1, 0, 1, 0, 1, 0, 0, 0, 0]
    # pad rows: exact zeros
    dead = ~c["live"]
    assert bool((dlog[dead] == 0).all()) and bool((logp[dead] == 0).all())
    # twice the same launch: the same bits
    loss2, logp2, hit2, dlog2 = launch(c, v, ld, eps)
    assert _same_bits(loss, loss2) and _same_bits(logp, logp2) and _same_bits(dlog, dlog2) and torch.equal(hit, hit2)
    # without a gradient: the same loss / row_logp / row_hit bits, nothing written
    loss3, logp3, hit3, _ = launch(c, v, ld, eps, grad=False)
    assert _same_bits(loss, loss3) and _same_bits(logp, logp3) and torch.equal(hit, hit3)


@pytest.mark.parametrize("v,ld", CASES, ids=lambda x: str(x))
def test_bf16_gradient_is_the_fp32_one_rounded_once(v, ld):
    c = case(v, ld, 21, 0.1)
    loss, logp, hit, dlog = launch(c, v, ld, 0.1, scale=3.0)
    for ldd in (ld, ld + 4 - ld % 4, v + 1 if v % 2 == 0 else v):  # the row stride; 8-B-aligned rows; odd rows
        loss_b, logp_b, hit_b, dlog_b = launch(c, v, ld, 0.1, dtype=torch.bfloat16, scale=3.0, ldd=ldd)
        assert torch.equal(dlog_b.view(torch.int16), dlog.to(torch.bfloat16).view(torch.int16)), ldd
        assert torch.equal(loss_b, loss) and torch.equal(logp_b, logp) and torch.equal(hit_b, hit)
    # dloss_scale scales the gradient only
    _, _, _, dlog1 = launch(c, v, ld, 0.1)
    assert bool(((dlog.double() - 3.0 * dlog1.double()).abs() <= 3 * 3.0 * U * dlog1.double().abs()).all())


@pytest.mark.parametrize("v,ld", CASES, ids=lambda x: str(x))
def test_eps_zero_agrees_with_the_weighted_kernel_at_unit_weights(v, ld):
    """Both kernels lie within their own bounds of the exact values, so they
    agree within the sum (the weighted kernel's: tests/test_gpu_scst_kernels.py)."""
    L = _lib()
    rows = 21
    c = case(v, ld, rows, 0.0)
    loss, logp, _, dlog = launch(c, v, ld, 0.0)
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    w = torch.ones(rows, device=DEV)
    loss0, logp0 = torch.zeros(1, device=DEV), torch.zeros(rows, device=DEV)
    dlog0 = torch.zeros(rows, ld, device=DEV)
    L.call("fpnmt_xent_weighted_fwd_bwd", L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), w.data_ptr(), 1,
           loss0.data_ptr(), logp0.data_ptr(), dlog0.data_ptr(), ld, 1.0, L.stream_ptr())
    x = float(c["buf"][:, :v].abs().max())
    lv = c["live"].double()
    bw_loss = float((lv * (c["b_logp"] + (rows + 2) * U * c["logp"].abs())).sum() / rows)
    bw_grad = c["coef"] * U * (v + 4 * x + 10)
    assert abs(float(loss) - float(loss0)) <= c["b_loss"] + bw_loss
    assert float((logp.double() - logp0.cpu().double()).abs().max()) <= 2 * c["b_logp"]
    assert bool(((dlog.double() - dlog0[:, :v].cpu().double()).abs() <= (c["b_grad"] + bw_grad)[:, None]).all())


def test_smoothed_xent_null_outputs_and_error_codes():
    L = _lib()
    v, ld, rows = 200, 208, 21
    c = case(v, ld, rows, 0.1)
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    loss = torch.zeros(1, device=DEV)
    dlog = torch.zeros(rows, ld, device=DEV)
    # row_logp, row_hit and dlogits may be NULL (ldd is then not looked at)
    L.call(NAME, L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), 0.1, loss.data_ptr(), None, None, None, 0, 1.0,
           L.stream_ptr())
    assert abs(float(loss) - c["loss"]) <= c["b_loss"]
    # rows == 0: the loss is overwritten with 0
    L.call(NAME, L.F32, 0, v, buf.data_ptr(), ld, lab.data_ptr(), 0.1, loss.data_ptr(), None, None, None, 0, 1.0,
           L.stream_ptr())
    assert float(loss) == 0.0
    f = getattr(L.lib, NAME)
    ok = [L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), 0.1, loss.data_ptr(), None, None, dlog.data_ptr(), ld,
          1.0, L.stream_ptr()]
    assert f(*ok) == 0
    for pos, bad, what in [(6, -0.1, b"eps"), (6, 1.0, b"eps"), (6, float("nan"), b"eps"), (7, None, b"null"),
                           (3, None, b"null"), (5, None, b"null"), (4, v - 1, b"ld"), (11, v - 1, b"ldd"),
                           (1, -1, b"rows"), (1, 1 << 31, b"rows"), (0, 5, b"dtype")]:
        args = list(ok)
        args[pos] = bad
        assert f(*args) == L.E_ARG, (pos, bad)
        assert what in L.lib.fpnmt_last_error(), (pos, bad, L.lib.fpnmt_last_error())
    # no workspace attached
    dev = torch.cuda.current_device()
    try:
        assert L.lib.fpnmt_set_workspace(None, 0) == 0
        assert f(*ok) == L.E_ARG and b"workspace" in L.lib.fpnmt_last_error()
    finally:
        ws = L._ws[dev]
        L.check(L.lib.fpnmt_set_workspace(ws.data_ptr(), ws.numel()), "fpnmt_set_workspace")
    assert f(*ok) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------ caption stats
def _stats_inputs(captions, t, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(1, 50, (captions, t), generator=g, dtype=torch.int32)
    for c in range(captions):
        n = int(torch.randint(0 if t > 1 else 1, t + 1, (1,), generator=g))
        lab[c, n:] = 0
    if captions > 1:
        lab[2] = 0  # an all-pad caption
    live = lab > 0
    logp = -torch.rand(captions, t, generator=g) * 9 * live
    hit = (torch.randint(0, 2, (captions, t), generator=g, dtype=torch.int32) * live).int()
    return lab, logp, hit


def _stats_launch(lab, logp, hit, totals, accumulate):
    L = _lib()
    n, t = lab.shape
    d = [x.contiguous().to(DEV) for x in (lab, logp, hit)]
    cl = torch.full((n,), 7.0, device=DEV)
    cn = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    ch = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    L.call("fpnmt_caption_stats", n, t, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), cl.data_ptr(),
           cn.data_ptr(), ch.data_ptr(), totals.data_ptr(), accumulate, L.stream_ptr())
    torch.cuda.synchronize()
    return cl.cpu(), cn.cpu(), ch.cpu()


@pytest.mark.parametrize("t", [1, 11])
@pytest.mark.parametrize("captions", [1, 5])
def test_caption_stats(captions, t):
    """Integers exact; cap_logp within one fp32 rounding (u relative) of the
    fp64 sum; the totals within the fp64 roundings of a sum of captions * t
    terms, 2^-53 per addition on the sum of magnitudes."""
    a = _stats_inputs(captions, t, 7 * captions + t)
    b = _stats_inputs(captions, t, 70 * captions + t)
    totals = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    want = torch.zeros(3, dtype=torch.float64)
    mag = 0.0
    for k, (lab, logp, hit) in enumerate((a, b)):
        cl, cn, ch = _stats_launch(lab, logp, hit, totals, k)  # overwrite, then accumulate
        live = lab > 0
        s64 = (logp.double() * live).sum(1)
        assert torch.equal(cn, live.sum(1).int()) and torch.equal(ch, hit.sum(1).int())
        assert bool(((cl.double() - s64).abs() <= U * s64.abs()).all())
        if captions > 1:
            assert int(cn[2]) == 0 and float(cl[2]) == 0.0 and int(ch[2]) == 0
        want += torch.stack([s64.sum(), live.sum().double(), hit.sum().double()])
        mag += float(logp.abs().sum())
        got = totals.cpu()
        assert got[1] == want[1] and got[2] == want[2]
        assert abs(float(got[0] - want[0])) <= 2 * captions * t * 2.0 ** -53 * mag
    assert float(want[1]) > 0
    L = _lib()
    f = L.lib.fpnmt_caption_stats
    p = totals.data_ptr()
    assert f(1, 1, None, p, p, None, None, None, p, 0, L.stream_ptr()) == L.E_ARG
    assert f(1, 0, p, p, p, None, None, None, p, 0, L.stream_ptr()) == L.E_ARG
    assert f(-1, 1, p, p, p, None, None, None, p, 0, L.stream_ptr()) == L.E_ARG
    assert f(1, 1, p, p, p, None, None, None, None, 0, L.stream_ptr()) == L.E_ARG
    # no captions: accumulate leaves the totals, overwrite zeroes them
    L.call("fpnmt_caption_stats", 0, 1, p, p, p, None, None, None, p, 1, L.stream_ptr())
    assert torch.equal(totals.cpu(), got)
    L.call("fpnmt_caption_stats", 0, 1, p, p, p, None, None, None, p, 0, L.stream_ptr())
    assert bool((totals.cpu() == 0).all())

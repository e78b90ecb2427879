"""The two kernels of self-critical training: fpnmt_xent_weighted_fwd_bwd
against an fp64 restatement (every route: 16-B and scalar loads, the
register-resident widths, the streaming form above the cap), its exact
zeros, rounding, determinism, convention and error codes; and
fpnmt_repeat_rows with its ordered backward (ops.RepeatRowsFn).

Error bounds, with u = 2^-24 (fp32 unit roundoff), X = max |logit| of the
case and V the row width:
  e_j = exp(x_j - m): the subtraction's rounding moves the argument by
    <= 2X u, expf adds <= 2 u relative            -> (2X + 2) u relative
  s = sum_j e_j (positive terms, any order): <= (V - 1) u relative on top
                                                   -> (V + 2X + 2) u relative
  logp = x_lab - (m + log s): log s inherits s's relative error as an
    absolute one, logf adds 2 u log V, the two additions u (X + log V) and
    u (2X + log V)                     -> B_logp = u (V + 5X + 4 log V + 2)
  grad_j = (e_j / s - [j = lab]) coef: e_j / s <= 1 carries (2X + 2) u +
    (V + 2X + 2) u + 2 u (division), the subtraction u, coef (two roundings)
    and the product 3 u more, all on a factor <= 1
                                       -> B_grad = |coef| u (V + 4X + 10)
  loss = (1 / rows) sum_r w_r ce_r over the live rows: each term carries
    |w_r| B_logp and its own rounding, the ordered sum <= rows u per term
                   -> B_loss = (1 / rows) sum_r |w_r| (B_logp + (rows + 2) u ce_r)
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
# (V, ld): 37 / 37 and 1001 / 1001 give odd row starts (scalar loads); 37 / 40
# a partial last vector on the 16-B route; 10 000 the 10-vector width; the
# last two lie above the register-resident cap (10 240): 16-B and scalar
CASES = [(37, 37), (37, 40), (200, 208), (1001, 1001), (4100, 4100), (10000, 10000), (10300, 10304),
         (10243, 10243)]
SHAPES = [(1, 1), (21, 1), (21, 7)]  # (rows, w_div)


@functools.lru_cache(maxsize=None)
def case(v, ld, rows, w_div):
    """Inputs and the fp64 reference of one case (built once, shared)."""
    g = torch.Generator().manual_seed(1000 * v + 10 * rows + w_div)
    buf = torch.randn(rows, ld, generator=g) * 3
    buf[:, v:] = float("nan")  # the row padding is never read
    logits = buf[:, :v]
    lab = torch.randint(1, v, (rows,), generator=g, dtype=torch.int32)
    lab[0] = v - 1
    if rows > 1:
        # pads, the last column, a label in the last (partial) vector, column 1
        lab[1], lab[2], lab[3], lab[5], lab[9] = 0, v - 2, 1, 0, v - 1 - (v % 4) // 2
    nw = rows // w_div
    w = torch.tensor([1.5, -0.7, 0.0, 0.3, -2.0, 0.0, 1.0][:nw] * (nw // 7 + 1))[:nw].contiguous() if nw > 1 \
        else torch.tensor([-0.7])
    wr = w.double().repeat_interleave(w_div)
    lsm = torch.log_softmax(logits.double(), 1)
    live = (lab != 0).double()
    logp = lsm.gather(1, lab.long()[:, None])[:, 0] * live
    loss = float((wr * -logp).sum() / rows)
    onehot = torch.zeros(rows, v, dtype=torch.float64)
    onehot[torch.arange(rows), lab.long()] = 1.0
    coef = wr * live / rows
    grad = (lsm.exp() - onehot) * coef[:, None]
    x = float(logits.abs().max())
    b_logp = U * (v + 5 * x + 4 * math.log(v) + 2)
    b_grad = coef.abs() * U * (v + 4 * x + 10)
    b_loss = float((wr.abs() * live * (b_logp + (rows + 2) * U * -logp)).sum() / rows)
    return dict(buf=buf, lab=lab, w=w, wr=wr, logp=logp, loss=loss, grad=grad, coef=coef, b_logp=b_logp,
                b_grad=b_grad, b_loss=b_loss)


def launch(c, v, ld, w_div, dtype=torch.float32, scale=1.0, ldd=None, w=None):
    from fpnmt import _lib as L
    rows = c["buf"].shape[0]
    ldd = ldd or ld
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    w = (c["w"] if w is None else w).to(DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    logp = torch.full((rows,), 7.0, device=DEV)
    dlog = torch.full((rows, ldd), 7.0, dtype=dtype, device=DEV)
    L.call("fpnmt_xent_weighted_fwd_bwd", L.dtype_code(dtype), rows, v, buf.data_ptr(), ld, lab.data_ptr(),
           w.data_ptr(), w_div, loss.data_ptr(), logp.data_ptr(), dlog.data_ptr(), ldd, scale, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dlog[:, v:].float() == 7.0).all())  # nothing written past a row's v columns
    return loss.cpu(), logp.cpu(), dlog[:, :v].cpu()


@pytest.mark.parametrize("rows,w_div", SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("v,ld", CASES, ids=lambda x: str(x))
def test_weighted_xent_against_fp64(v, ld, rows, w_div, parity_record):
    c = case(v, ld, rows, w_div)
    loss, logp, dlog = launch(c, v, ld, w_div)
    e_loss = abs(float(loss) - c["loss"])
    e_logp = float((logp.double() - c["logp"]).abs().max())
    e_grad = (dlog.double() - c["grad"]).abs()
    worst = float((e_grad.max(1).values / c["b_grad"].clamp_min(1e-300)).max())
    print(f"V={v} ld={ld} rows={rows} w_div={w_div}: loss err {e_loss:.3e} (bound {c['b_loss']:.3e}), "
          f"logp err {e_logp:.3e} (bound {c['b_logp']:.3e}), grad err / bound {worst:.3e}")
    parity_record[f"scst_xent_v{v}_ld{ld}_r{rows}_d{w_div}"] = dict(
        loss_err=e_loss, loss_bound=c["b_loss"], logp_err=e_logp, logp_bound=c["b_logp"],
        grad_err=float(e_grad.max()), grad_err_over_bound=worst)
    assert e_loss <= c["b_loss"]
    assert e_logp <= c["b_logp"]
    assert bool((e_grad <= c["b_grad"][:, None]).all())
    # pad rows and zero-weight rows: exactly zero gradient; a pad row's logp is 0
    dead = c["coef"] == 0
    assert bool((dlog[dead] == 0).all())
    assert bool((logp[c["lab"] == 0] == 0).all())
    if rows > 1:
        assert bool(dead.any()) and bool((c["lab"][dead] != 0).any())  # a live row with weight 0 among them
    # twice the same launch: the same bits
    loss2, logp2, dlog2 = launch(c, v, ld, w_div)
    for a, b in ((loss, loss2), (logp, logp2), (dlog, dlog2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("v,ld", CASES, ids=lambda x: str(x))
def test_bf16_gradient_is_the_fp32_one_rounded_once(v, ld):
    c = case(v, ld, 21, 7)
    loss, logp, dlog = launch(c, v, ld, 7, scale=3.0)
    for ldd in (ld, ld + 4 - ld % 4, v + 1 if v % 2 == 0 else v):  # the row stride; 8-B-aligned rows; odd rows
        loss_b, logp_b, dlog_b = launch(c, v, ld, 7, dtype=torch.bfloat16, scale=3.0, ldd=ldd)
        assert torch.equal(dlog_b.view(torch.int16), dlog.to(torch.bfloat16).view(torch.int16)), ldd
        assert torch.equal(loss_b, loss) and torch.equal(logp_b, logp)
    # dloss_scale scales the gradient only
    _, _, dlog1 = launch(c, v, ld, 7)
    assert bool(((dlog.double() - 3.0 * dlog1.double()).abs() <= 3 * 3.0 * U * dlog1.double().abs()).all())


@pytest.mark.parametrize("v,ld", CASES, ids=lambda x: str(x))
def test_unit_weights_agree_with_the_plain_kernel(v, ld):
    """w = 1, w_div = 1: the convention (mean over ALL rows) is fpnmt_xent_fwd_bwd's."""
    from fpnmt import _lib as L
    rows = 21
    c = case(v, ld, rows, 1)
    ones = torch.ones(rows)
    loss, _, dlog = launch(c, v, ld, 1, w=ones)
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    loss0 = torch.zeros(1, device=DEV)
    dlog0 = torch.zeros(rows, ld, device=DEV)
    L.call("fpnmt_xent_fwd_bwd", L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), loss0.data_ptr(),
           dlog0.data_ptr(), ld, 1.0, L.stream_ptr())
    live = (c["lab"] != 0).double()
    b_loss = float((live * (c["b_logp"] + (rows + 2) * U * -c["logp"])).sum() / rows)
    b_grad = live / rows * U * (v + 4 * float(c["buf"][:, :v].abs().max()) + 10)
    assert abs(float(loss) - float(loss0)) <= b_loss
    assert bool(((dlog.double() - dlog0[:, :v].cpu().double()).abs() <= b_grad[:, None]).all())


def test_weighted_xent_without_outputs_and_error_codes():
    from fpnmt import _lib as L
    v, ld, rows = 200, 208, 21
    c = case(v, ld, rows, 7)
    buf, lab, w = c["buf"].to(DEV), c["lab"].to(DEV), c["w"].to(DEV)
    loss = torch.zeros(1, device=DEV)
    # row_logp and dlogits may be NULL
    L.call("fpnmt_xent_weighted_fwd_bwd", L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), w.data_ptr(), 7,
           loss.data_ptr(), None, None, 0, 1.0, L.stream_ptr())
    assert abs(float(loss) - c["loss"]) <= c["b_loss"]
    # rows == 0: the loss is overwritten with 0
    L.call("fpnmt_xent_weighted_fwd_bwd", L.F32, 0, v, buf.data_ptr(), ld, lab.data_ptr(), w.data_ptr(), 7,
           loss.data_ptr(), None, None, 0, 1.0, L.stream_ptr())
    assert float(loss) == 0.0
    f = L.lib.fpnmt_xent_weighted_fwd_bwd
    ok = [L.F32, rows, v, buf.data_ptr(), ld, lab.data_ptr(), w.data_ptr(), 7, loss.data_ptr(), None, None, 0, 1.0,
          L.stream_ptr()]
    for pos, bad, what in [(7, 4, b"multiple of w_div"), (7, 0, b"w_div"), (7, -1, b"w_div"), (3, None, b"null"),
                           (5, None, b"null"), (6, None, b"null"), (8, None, b"null"), (4, v - 1, b"ld"),
                           (0, 5, b"dtype")]:
        args = list(ok)
        args[pos] = bad
        assert f(*args) == L.E_ARG, (pos, bad)
        assert what in L.lib.fpnmt_last_error(), (pos, bad, L.lib.fpnmt_last_error())
    torch.cuda.synchronize()


# ------------------------------------------------------------- repeat rows
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ln", [512, 16 * 512, 24, 7])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("b", [1, 3])
def test_repeat_rows_and_its_ordered_backward(b, n, ln, dtype):
    from fpnmt import ops
    g = torch.Generator().manual_seed(b * 100 + n * 10 + ln)
    x = torch.randn(b, ln // 8 if ln % 8 == 0 else 1, 8 if ln % 8 == 0 else ln, generator=g).to(dtype)
    dy = torch.randn(b * n, *x.shape[1:], generator=g).to(dtype)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.RepeatRowsFn.apply(xd, n)
    assert y.shape == (b * n,) + x.shape[1:] and y.dtype == dtype
    assert torch.equal(y.detach().cpu(), x.repeat_interleave(n, 0))
    y.backward(dy.to(DEV))
    acc = torch.zeros(x.shape, dtype=torch.float32)
    for s in range(n):  # fp32, ascending s, rounded once
        acc = acc + dy.view(b, n, *x.shape[1:])[:, s].float()
    assert xd.grad.dtype == dtype
    assert torch.equal(xd.grad.cpu(), acc.to(dtype))


def test_repeat_rows_unaligned_pointers_and_errors():
    """A source that is not 16-B aligned takes the per-element copy."""
    from fpnmt import _lib as L
    base = torch.arange(3 * 24 + 1, dtype=torch.float32, device=DEV)
    x = base[1:].view(3, 24)
    y = torch.zeros(6, 24, device=DEV)
    L.call("fpnmt_repeat_rows", L.F32, 3, 2, 24, x.data_ptr(), y.data_ptr(), L.stream_ptr())
    assert torch.equal(y, x.repeat_interleave(2, 0))
    f = L.lib.fpnmt_repeat_rows
    assert f(L.F32, 3, 2, 24, None, y.data_ptr(), L.stream_ptr()) == L.E_ARG
    assert f(L.F32, 70000, 2, 24, x.data_ptr(), y.data_ptr(), L.stream_ptr()) == L.E_ARG
    assert f(7, 3, 2, 24, x.data_ptr(), y.data_ptr(), L.stream_ptr()) == L.E_ARG
    assert f(L.F32, 3, -1, 24, x.data_ptr(), y.data_ptr(), L.stream_ptr()) == L.E_ARG
    torch.cuda.synchronize()

"""fpnmt_xent_distill_fwd_bwd against the fp64 restatement and the derived
bounds of tests/distill_ref.py, on every load route and width (the (V, ld)
list of tests/test_gpu_xent_smooth_kernels.py, the same student rows and
planted labels), under four (alpha, T) mixes, with teacher strides whose
alignment differs from the student's; the bf16 gradient, the agreement with
fpnmt_xent_smooth_fwd_bwd at alpha = 0, repeatability, the device descriptor
rewritten in place, non-finite teachers, exact zeros and the error codes.

Padding columns of both inputs hold NaN and a pad row's teacher row is NaN
throughout: they are never read. Worst err / bound per case goes to the
parity record."""
import math

import pytest
import torch

import distill_ref as D
from test_gpu_xent_smooth_kernels import launch as smooth_launch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAME = "fpnmt_xent_distill_fwd_bwd"
FILL = 7.0


def _lib():
    from fpnmt import _lib as L
    assert hasattr(L.lib, NAME), f"libfpnmt has no {NAME}"
    assert NAME in L.SIGNATURES and hasattr(L, "DistillDesc"), f"fpnmt._lib does not declare {NAME}"
    return L


def _desc(alpha, T):
    return torch.tensor([alpha, T, 0.0, 0.0], dtype=torch.float32, device=DEV)


def _teacher_buf(c, v, ldt, tea=None):
    """(rows, ldt) on the device: the teacher in the first v columns, NaN in
    the padding and in every pad row."""
    tea = c["tea"] if tea is None else tea
    rows = tea.shape[0]
    buf = torch.full((rows, ldt), float("nan"))
    buf[:, :v] = tea
    buf[~c["live"]] = float("nan")
    return buf.to(DEV)


def launch(c, v, ld, ldt, eps, desc, dtype=torch.float32, scale=1.0, ldd=None, grad=True, tea=None, logp=True):
    L = _lib()
    rows = c["buf"].shape[0]
    ldd = ldd or ld
    buf, lab = c["buf"].to(DEV), c["lab"].to(DEV)
    tb = _teacher_buf(c, v, ldt, tea)
    loss = torch.full((3,), FILL, device=DEV)
    lp = torch.full((rows,), FILL, device=DEV)
    dlog = torch.full((rows, ldd), FILL, dtype=dtype, device=DEV)
    L.call(NAME, L.dtype_code(dtype), rows, v, buf.data_ptr(), ld, tb.data_ptr(), ldt, lab.data_ptr(), eps,
           desc.data_ptr(), loss.data_ptr(), lp.data_ptr() if logp else None, dlog.data_ptr() if grad else None, ldd,
           scale, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dlog[:, v if grad else 0:].float() == FILL).all())  # nothing written past a row's v columns
    return loss.cpu(), lp.cpu(), dlog[:, :v].cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(c, loss, lp, dlog, tag, record=None, extra_grad=None):
    e_loss = (loss.double() - c["loss"]).abs()
    e_logp = float((lp.double() - c["logp"]).abs().max())
    e_grad = (dlog.double() - c["grad"]).abs()
    b_grad = c["b_grad"][:, None] if extra_grad is None else c["b_grad"][:, None] + extra_grad
    live = c["live"]
    worst = float((e_grad / b_grad.clamp_min(1e-300))[live].max()) if bool(live.any()) else 0.0
    ratios = [float(e_loss[i] / c["b_loss"][i]) if float(c["b_loss"][i]) > 0 else 0.0 for i in range(3)]
    print(f"{tag}: loss err / bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f} (bounds "
          f"{float(c['b_loss'][0]):.2e} {float(c['b_loss'][1]):.2e} {float(c['b_loss'][2]):.2e}), logp err {e_logp:.2e} "
          f"(bound {c['b_logp']:.2e}), grad err / bound {worst:.3f}")
    if record is not None:
        record[tag] = dict(loss_err_over_bound=ratios, logp_err=e_logp, logp_bound=c["b_logp"],
                           grad_err=float(e_grad.max()), grad_err_over_bound=worst)
    assert bool((e_loss <= c["b_loss"]).all()), (e_loss.tolist(), c["b_loss"].tolist())
    assert e_logp <= c["b_logp"]
    assert bool((e_grad <= b_grad).all()), worst
    dead = ~live
    assert bool((dlog[dead].float() == 0).all()) and bool((lp[dead] == 0).all())  # pad rows: exact zeros


@pytest.mark.parametrize("rows", D.ROWS)
@pytest.mark.parametrize("v,ld,eps,alpha,T", D.PARAMS, ids=lambda x: str(x))
def test_distill_against_fp64(v, ld, eps, alpha, T, rows, parity_record):
    c = D.case(v, ld, rows, eps, alpha, T)
    ldt = D.LDT[(v, ld)]
    desc = _desc(alpha, T)
    loss, lp, dlog = launch(c, v, ld, ldt, eps, desc)
    _check(c, loss, lp, dlog, f"xent_distill_v{v}_ld{ld}_ldt{ldt}_r{rows}_e{eps}_a{alpha}_T{T}", parity_record)
    if rows > 1:
        assert int((~c["live"]).sum()) >= 5 and float(c["loss"][2]) > 0
    # twice the same launch: the same bits
    loss2, lp2, dlog2 = launch(c, v, ld, ldt, eps, desc)
    assert _same_bits(loss, loss2) and _same_bits(lp, lp2) and _same_bits(dlog, dlog2)
    # without a gradient / without row_logp: the same loss bits, nothing written
    loss3, lp3, _ = launch(c, v, ld, ldt, eps, desc, grad=False)
    assert _same_bits(loss, loss3) and _same_bits(lp, lp3)
    loss4, lp4, dlog4 = launch(c, v, ld, ldt, eps, desc, logp=False)
    assert _same_bits(loss, loss4) and _same_bits(dlog, dlog4) and bool((lp4 == FILL).all())


@pytest.mark.parametrize("v,ld,ldt", [(10000, 10000, 10001), (10300, 10304, 10301), (4100, 4100, 4104), (200, 208, 201)])
def test_teacher_strides_of_another_alignment(v, ld, ldt):
    """The register form with 16-B student rows and scalar teacher rows at
    the widest width, the streaming form's scalar route, and back."""
    c = D.case(v, ld, 21, 0.1, 0.5, 2.0)
    loss, lp, dlog = launch(c, v, ld, ldt, 0.1, _desc(0.5, 2.0))
    _check(c, loss, lp, dlog, f"ldt v{v} ld{ld} ldt{ldt}")


@pytest.mark.parametrize("alpha,T", [(0.5, 2.0), (0.5, 1.0)])
@pytest.mark.parametrize("v,ld", [(200, 208), (10000, 10000), (10243, 10243)], ids=lambda x: str(x))
def test_diffuse_teacher(v, ld, alpha, T):
    """The cases above have a confident teacher on every row; here it is as
    spread out as the student (randn * 3), the regime early in training."""
    c = D.case(v, ld, 21, 0.1, alpha, T)
    tea = torch.randn(21, v, generator=torch.Generator().manual_seed(v + 5)) * 3
    ref = dict(c, **D.reference(c["buf"][:, :v], tea, c["lab"], 0.1, alpha, T))
    loss, lp, dlog = launch(c, v, ld, D.LDT[(v, ld)], 0.1, _desc(alpha, T), tea=tea)
    _check(ref, loss, lp, dlog, f"diffuse v{v} a{alpha} T{T}")
    assert float(ref["loss"][2]) > 0


@pytest.mark.parametrize("v,ld", D.CASES, ids=lambda x: str(x))
def test_bf16_gradient_within_its_rounding(v, ld):
    c = D.case(v, ld, 21, 0.1, 0.5, 2.0, 3.0)
    desc = _desc(0.5, 2.0)
    ldt = D.LDT[(v, ld)]
    loss, lp, dlog = launch(c, v, ld, ldt, 0.1, desc, scale=3.0)
    _check(c, loss, lp, dlog, f"scale 3 v{v}")
    for ldd in (ld, ld + 4 - ld % 4, v + 1 if v % 2 == 0 else v):  # the row stride; 8-B-aligned rows; odd rows
        loss_b, lp_b, dlog_b = launch(c, v, ld, ldt, 0.1, desc, dtype=torch.bfloat16, scale=3.0, ldd=ldd)
        # one more rounding of a value within b_grad of the reference
        extra = D.U_BF16 * (c["grad"].abs() + c["b_grad"][:, None])
        _check(c, loss_b, lp_b, dlog_b.float(), f"bf16 v{v} ldd{ldd}", extra_grad=extra)
        assert torch.equal(loss_b, loss) and torch.equal(lp_b, lp)
        # and it is the fp32 gradient rounded once
        assert torch.equal(dlog_b.view(torch.int16), dlog.to(torch.bfloat16).view(torch.int16)), ldd


@pytest.mark.parametrize("v,ld", D.CASES, ids=lambda x: str(x))
def test_alpha_zero_agrees_with_the_smoothed_kernel(v, ld):
    """Both kernels lie within their own bounds of the same exact values."""
    c = D.case(v, ld, 21, 0.1, 0.0, 2.0)
    s = c["smooth"]
    loss, lp, dlog = launch(c, v, ld, D.LDT[(v, ld)], 0.1, _desc(0.0, 2.0))
    loss0, lp0, _, dlog0 = smooth_launch(s, v, ld, 0.1)
    assert abs(float(loss[0]) - float(loss0)) <= float(c["b_loss"][0]) + s["b_loss"]
    assert abs(float(loss[1]) - float(loss0)) <= float(c["b_loss"][1]) + s["b_loss"]
    assert float((lp.double() - lp0.double()).abs().max()) <= c["b_logp"] + s["b_logp"]
    assert bool(((dlog.double() - dlog0.double()).abs() <= (c["b_grad"] + s["b_grad"])[:, None]).all())


@pytest.mark.parametrize("v,ld", [(200, 208), (10000, 10000), (10243, 10243)], ids=lambda x: str(x))
def test_descriptor_is_read_on_the_device_at_execution(v, ld):
    L = _lib()
    rows, eps, ldt = 21, 0.1, D.LDT[(v, ld)]
    c1, c2 = D.case(v, ld, rows, eps, 0.5, 2.0), D.case(v, ld, rows, eps, 1.0, 4.0)
    buf, lab, tb = c1["buf"].to(DEV), c1["lab"].to(DEV), _teacher_buf(c1, v, ldt)
    desc = _desc(0.5, 2.0)
    loss, lp = torch.zeros(3, device=DEV), torch.zeros(rows, device=DEV)
    dlog = torch.zeros(rows, ld, device=DEV)
    args = (NAME, L.F32, rows, v, buf.data_ptr(), ld, tb.data_ptr(), ldt, lab.data_ptr(), eps, desc.data_ptr(),
            loss.data_ptr(), lp.data_ptr(), dlog.data_ptr(), ld, 1.0, L.stream_ptr())
    L.call(*args)
    _check(c1, loss.cpu(), lp.cpu(), dlog[:, :v].cpu(), "desc (0.5, 2)")
    desc.copy_(torch.tensor([1.0, 4.0, 0.0, 0.0]))  # in place: the same pointer, the same arguments
    L.call(*args)
    torch.cuda.synchronize()
    _check(c2, loss.cpu(), lp.cpu(), dlog[:, :v].cpu(), "desc (1, 4)")
    assert abs(float(loss[0]) - float(c1["loss"][0])) > 100 * float(c1["b_loss"][0])


@pytest.mark.parametrize("v,ld", [(37, 40), (4100, 4100), (10000, 10000), (10243, 10243)], ids=lambda x: str(x))
def test_non_finite_teachers(v, ld):
    rows, eps, a, T = 21, 0.1, 0.5, 2.0
    c = D.case(v, ld, rows, eps, a, T)
    ldt, desc = D.LDT[(v, ld)], _desc(a, T)
    clean = launch(c, v, ld, ldt, eps, desc)
    # tokens of probability zero: -inf columns, the first and the last among them
    tea = c["tea"].clone()
    cols = [0, v // 2, v - 1]
    tea[:, cols] = float("-inf")
    ref = dict(c, **D.reference(c["buf"][:, :v], tea, c["lab"], eps, a, T))
    loss, lp, dlog = launch(c, v, ld, ldt, eps, desc, tea=tea)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dlog).all())
    _check(ref, loss, lp, dlog, f"-inf columns v{v}")
    # rows without a softmax: NaN kl, so loss[0] and loss[2]; the hard term and every other row as before
    live = [int(r) for r in torch.nonzero(c["live"])[:, 0]]
    for what, r in (("nan", live[1]), ("inf", live[2]), ("all -inf", live[3])):
        tea = c["tea"].clone()
        if what == "nan":
            tea[r, v - 1] = float("nan")
        elif what == "inf":
            tea[r, 0] = float("inf")
        else:
            tea[r] = float("-inf")
        loss, lp, dlog = launch(c, v, ld, ldt, eps, desc, tea=tea)
        assert math.isnan(float(loss[0])) and math.isnan(float(loss[2])), (what, loss.tolist())
        assert _same_bits(loss[1:2], clean[0][1:2]) and _same_bits(lp, clean[1])
        keep = torch.arange(rows) != r
        assert _same_bits(dlog[keep], clean[2][keep]), what


def test_distill_trivial_cases_and_error_codes():
    L = _lib()
    v, ld, ldt, rows, eps = 200, 208, 208, 21, 0.1
    c = D.case(v, ld, rows, eps, 0.5, 2.0)
    desc = _desc(0.5, 2.0)
    # dloss_scale == 0: exact zeros, the losses as before
    loss, lp, dlog = launch(c, v, ld, ldt, eps, desc, scale=0.0)
    assert bool((dlog == 0).all())
    assert bool(((loss.double() - c["loss"]).abs() <= c["b_loss"]).all())
    c_wide = D.case(10243, 10243, rows, eps, 0.5, 2.0)
    loss, lp, dlog = launch(c_wide, 10243, 10243, 10244, eps, desc, scale=0.0)
    assert bool((dlog == 0).all())
    assert bool(((loss.double() - c_wide["loss"]).abs() <= c_wide["b_loss"]).all())
    buf, lab, tb = c["buf"].to(DEV), c["lab"].to(DEV), _teacher_buf(c, v, ldt)
    loss = torch.full((3,), FILL, device=DEV)
    dlog = torch.zeros(rows, ld, device=DEV)
    # rows == 0: the three losses are overwritten with 0
    L.call(NAME, L.F32, 0, v, buf.data_ptr(), ld, tb.data_ptr(), ldt, lab.data_ptr(), eps, desc.data_ptr(),
           loss.data_ptr(), None, None, 0, 1.0, L.stream_ptr())
    assert loss.tolist() == [0.0, 0.0, 0.0]
    f = getattr(L.lib, NAME)
    ok = [L.F32, rows, v, buf.data_ptr(), ld, tb.data_ptr(), ldt, lab.data_ptr(), eps, desc.data_ptr(),
          loss.data_ptr(), None, dlog.data_ptr(), ld, 1.0, L.stream_ptr()]
    assert f(*ok) == 0
    for pos, bad, what in [(8, -0.1, b"eps"), (8, 1.0, b"eps"), (8, float("nan"), b"eps"), (3, None, b"null"),
                           (5, None, b"null"), (7, None, b"null"), (9, None, b"null"), (10, None, b"null"),
                           (4, v - 1, b"ld"), (6, v - 1, b"ldt"), (13, v - 1, b"ldd"), (1, -1, b"rows"),
                           (1, 1 << 31, b"rows"), (0, 5, b"dtype"), (2, 0, b"v < 1")]:
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

"""The fp64 restatement of fpnmt_xent_distill_fwd_bwd (tests/distill_ref.py)
checked against itself on the CPU: its closed-form gradient against autograd,
its limits (alpha = 0: the smoothed CE of tests/test_gpu_xent_smooth_kernels;
a one-hot teacher at alpha = 1, T = 1: the plain CE), the -inf rule, that the
derived bounds leave room to see the errors a kernel could plausibly make
(planted in the reference, at the GPU tests' cases), and the host-side
validation of alpha, temperature and the teachers' weights. No GPU."""
import math

import pytest
import torch

import distill_ref as D
from test_gpu_xent_smooth_kernels import case as smooth_case


def _feature():
    """The product side of what this file checks; asserted first in every test."""
    from fpnmt import _lib as L
    assert "fpnmt_xent_distill_fwd_bwd" in L.SIGNATURES, "fpnmt._lib does not declare fpnmt_xent_distill_fwd_bwd"
    assert hasattr(L.lib, "fpnmt_xent_distill_fwd_bwd"), "libfpnmt has no fpnmt_xent_distill_fwd_bwd"
    import importlib.util
    assert importlib.util.find_spec("fpnmt.distill") is not None, "there is no fpnmt.distill"
    from fpnmt import distill as FD
    return L, FD


def _rand(rows, v, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, v, generator=g) * 3
    t = torch.randn(rows, v, generator=g) * 2
    lab = torch.randint(1, v, (rows,), generator=g, dtype=torch.int32)
    lab[1], lab[4] = 0, v + 2  # pads
    return x, t, lab


@pytest.mark.parametrize("alpha,T,eps", [(0.5, 2.0, 0.1), (1.0, 4.0, 0.0), (0.3, 1.0, 0.1), (0.0, 2.0, 0.1)])
def test_reference_gradient_is_autograd_of_its_loss(alpha, T, eps):
    _feature()
    rows, v = 7, 53
    x, t, lab = _rand(rows, v, 5)
    t[2, 7] = t[3, 0] = float("-inf")  # the -inf rule is part of the loss autograd sees
    ref = D.reference(x, t, lab, eps, alpha, T, scale=1.7)
    x64 = x.double().requires_grad_(True)
    row, _, _, _ = D.losses(x64, t, lab, ref["eps"], ref["alpha"], ref["T"])
    (row.sum() * D.f32(1.7) / rows).backward()
    err = float((x64.grad - ref["grad"]).abs().max())
    assert err <= 1e-12 * float(ref["grad"].abs().max()), err
    assert bool((ref["grad"][~ref["live"]] == 0).all()) and float(ref["grad"].abs().max()) > 0


@pytest.mark.parametrize("v,ld", [(37, 40), (1001, 1001)])
def test_alpha_zero_is_the_smoothed_ce_reference(v, ld):
    _feature()
    c = smooth_case(v, ld, 21, 0.1)
    t = D.teacher(v, ld, 21)
    ref = D.reference(c["buf"][:, :v], t, c["lab"], 0.1, 0.0, 2.0)
    assert abs(float(ref["loss"][0]) - c["loss"]) <= 1e-12 * abs(c["loss"])
    assert abs(float(ref["loss"][1]) - c["loss"]) <= 1e-12 * abs(c["loss"])
    assert float((ref["grad"] - c["grad"]).abs().max()) <= 1e-15
    assert float((ref["logp"] - c["logp"]).abs().max()) <= 1e-12
    assert float(ref["loss"][2]) > 0  # the KL is still reported


def test_one_hot_teacher_at_unit_temperature_approaches_plain_ce():
    _feature()
    rows, v = 7, 53
    x, _, lab = _rand(rows, v, 6)
    live = (lab > 0) & (lab < v)
    t = torch.zeros(rows, v)
    t[torch.arange(rows), torch.where(live, lab, torch.ones_like(lab)).long()] = 40.0
    ref = D.reference(x, t, lab, 0.0, 1.0, 1.0)
    p = torch.softmax(x.double(), 1)
    onehot = torch.zeros(rows, v, dtype=torch.float64)
    onehot[torch.arange(rows), lab.clamp(0, v - 1).long()] = 1.0
    ce_grad = (p - onehot) * live.double()[:, None] / rows
    # q differs from the one-hot by (V - 1) e^-40 in all
    assert float((ref["grad"] - ce_grad).abs().max()) <= 2 * v * math.exp(-40.0) / rows
    logp = torch.log_softmax(x.double(), 1)[torch.arange(rows), lab.clamp(0, v - 1).long()] * live.double()
    assert float((ref["kl"] + logp).abs().max()) <= 50 * v * math.exp(-40.0)  # KL(onehot || p) = -log p_lab


def test_minus_inf_teacher_entries_have_probability_zero():
    _feature()
    rows, v = 7, 53
    x, t, lab = _rand(rows, v, 7)
    cols = [0, 9, 52]
    t_inf = t.clone()
    t_inf[:, cols] = float("-inf")
    ref = D.reference(x, t_inf, lab, 0.1, 0.5, 2.0)
    assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["grad"]).all())
    # the same KL with those tokens given a probability that underflows to an exact 0
    t_low = t.clone()
    t_low[:, cols] = -1e6
    low = D.reference(x, t_low, lab, 0.1, 0.5, 2.0)
    assert torch.equal(ref["kl"], low["kl"]) and torch.equal(ref["grad"], low["grad"])
    # the gradient there: coef ((1 - a) (p - smooth target) + a T pT), q = 0
    a, T, e = ref["alpha"], ref["T"], ref["eps"]
    p, pt = torch.softmax(x.double(), 1), torch.softmax(x.double() / T, 1)
    onehot = torch.zeros(rows, v, dtype=torch.float64)
    onehot[torch.arange(rows), lab.clamp(0, v - 1).long()] = 1.0
    want = ((1 - a) * (p - (1 - e) * onehot - e / v) + a * T * pt) * ref["coef"][:, None]
    assert float((ref["grad"][:, cols] - want[:, cols]).abs().max()) <= 1e-15
    # a row without a softmax: NaN in kl and the two losses that hold it, nothing else
    for fill in (float("nan"), float("inf")):
        t_bad = t.clone()
        t_bad[2, 5] = fill
        bad = D.reference(x, t_bad, lab, 0.1, 0.5, 2.0)
        assert math.isnan(float(bad["kl"][2])) and math.isnan(float(bad["loss"][0])) and math.isnan(float(bad["loss"][2]))
        assert math.isfinite(float(bad["loss"][1]))
        keep = torch.arange(rows) != 2
        assert torch.equal(bad["grad"][keep], D.reference(x, t, lab, 0.1, 0.5, 2.0)["grad"][keep])
    t_bad = t.clone()
    t_bad[2] = float("-inf")
    assert math.isnan(float(D.reference(x, t_bad, lab, 0.1, 0.5, 2.0)["kl"][2]))
    # a pad row's teacher is never looked at
    t_pad = t.clone()
    t_pad[1] = float("nan")
    assert torch.equal(D.reference(x, t_pad, lab, 0.1, 0.5, 2.0)["loss"], D.reference(x, t, lab, 0.1, 0.5, 2.0)["loss"])


TEETH = [p for p in D.PARAMS if p[4] != 1.0]


@pytest.mark.parametrize("rows", D.ROWS)
@pytest.mark.parametrize("v,ld,eps,alpha,T", TEETH, ids=lambda x: str(x))
def test_bounds_leave_room_to_see_planted_errors(v, ld, eps, alpha, T, rows):
    """Each planted error moves the value it touches by more than 100 x the
    derived bound, at every case of the GPU test with T != 1. The two errors
    in a factor of alpha (a T for a T^2 on the loss, a T^2 for a T on the
    gradient) are invisible at alpha = 0 and are checked where alpha > 0; the
    unmasked pad rows need pad rows (rows = 21)."""
    _feature()
    c = D.case(v, ld, rows, eps, alpha, T)
    x, t, lab = c["buf"][:, :v], c["tea"], c["lab"]
    moved = {}
    if alpha > 0:
        r = D.reference(x, t, lab, eps, alpha, T, plant="loss_aT")
        moved["loss_aT"] = (abs(float(r["loss"][0] - c["loss"][0])), float(c["b_loss"][0]))
        r = D.reference(x, t, lab, eps, alpha, T, plant="grad_aT2")
        d = (r["grad"] - c["grad"]).abs().max(1).values
        k = int((d / c["b_grad"].clamp_min(1e-300)).argmax())
        moved["grad_aT2"] = (float(d[k]), float(c["b_grad"][k]))
    r = D.reference(x, t, lab, eps, alpha, T, plant="kl_swapped")
    moved["kl_swapped"] = (abs(float(r["loss"][2] - c["loss"][2])), float(c["b_loss"][2]))
    if rows > 1:
        r = D.reference(x, t, lab, eps, alpha, T, plant="kl_unmasked")
        moved["kl_unmasked"] = (abs(float(r["loss"][2] - c["loss"][2])), float(c["b_loss"][2]))
    print({k: f"{d:.3e} / {b:.3e} = {d / b:.0f}" for k, (d, b) in moved.items()})
    for k, (d, b) in moved.items():
        assert d > 100 * b, (k, d, b)


def test_host_side_validation():
    L, FD = _feature()
    for a in (0, 0.0, 0.5, 1, 1.0):
        assert FD.check_alpha(a) == float(a)
    for a in (-1e-9, 1.0000001, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="alpha"):
            FD.check_alpha(a)
    for t in (1e-3, 1, 2.5):
        assert FD.check_temperature(t) == float(t)
    for t in (0, 0.0, -1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="temperature"):
            FD.check_temperature(t)
    # no teachers: allowed (teacher_logits only), but then no weights
    assert FD.check_teachers((), 10, torch.device("cpu")) == ((), ())
    with pytest.raises(ValueError, match="without teachers"):
        FD.check_teachers((), 10, torch.device("cpu"), weights=(1.0,))
    with pytest.raises(ValueError, match="ensemble_mode"):
        FD.check_teachers((), 10, torch.device("cpu"), mode="mean")

    class _Fake:  # what check_teachers looks at
        def __init__(self, vocab):
            self.final_layer = type("F", (), {"kernel": torch.zeros(4, vocab)})()
            self.decoder = type("Dd", (), {"pos_encoding": torch.zeros(12, 4)})()
    two = (_Fake(10), _Fake(10))
    assert FD.check_teachers(two, 10, torch.device("cpu"), weights=(1, 3))[1] == (0.25, 0.75)
    assert FD.check_teachers(two, 10, torch.device("cpu"))[1] == (0.5, 0.5)
    for w in ((1.0,), (1.0, 0.0), (1.0, float("nan")), (1.0, -2.0), "ab"):
        with pytest.raises(ValueError, match="ensemble_weights"):
            FD.check_teachers(two, 10, torch.device("cpu"), weights=w)
    with pytest.raises(ValueError, match="vocabulary"):
        FD.check_teachers((_Fake(10), _Fake(11)), 10, torch.device("cpu"))
    with pytest.raises(ValueError, match="not a Transformer"):
        FD.check_teachers((object(),), 10, torch.device("cpu"))
    with pytest.raises(ValueError, match="positional table"):
        FD.check_teachers(two, 10, torch.device("cpu"), seq_len=13)
    with pytest.raises(ValueError, match=f"at most {L.ENSEMBLE_MAX}"):
        FD.check_teachers((_Fake(10),) * (L.ENSEMBLE_MAX + 1), 10, torch.device("cpu"))
    assert len(FD.check_teachers((_Fake(10),) * L.ENSEMBLE_MAX, 10, torch.device("cpu"))[0]) == L.ENSEMBLE_MAX
    # the C ABI and the ctypes mirror
    assert len(L.SIGNATURES["fpnmt_xent_distill_fwd_bwd"]) == 16
    assert L.lib.fpnmt_xent_distill_fwd_bwd is not None
    import ctypes as C
    assert C.sizeof(L.DistillDesc) == 16

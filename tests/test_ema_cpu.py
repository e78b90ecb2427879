"""Host side of the weight averaging (TrainEngine(ema_decay=...),
ParamArena.enable_ema, fpnmt_amsgrad_step_ema) and the fp64 reference
tests/ema_ref.py. No GPU."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from ema_ref import EmaAMSGradRef, omd_t, one_minus_decay_f32

BAD = (float("nan"), -0.1, -1e-9, 1.0, 1.5, float("inf"), "x", None)


def _require_feature():
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    from fpnmt.train import TrainEngine
    assert "fpnmt_amsgrad_step_ema" in L.ALL_SYMBOLS and "fpnmt_swap_f32" in L.ALL_SYMBOLS
    assert hasattr(ParamArena, "enable_ema")
    assert "ema" in inspect.signature(ParamArena.amsgrad_step).parameters
    assert "ema_decay" in inspect.signature(TrainEngine.__init__).parameters


def _cpu_arena():
    from fpnmt.arena import ParamArena
    g = torch.Generator().manual_seed(0)
    ps = [("a", torch.nn.Parameter(torch.randn(70, generator=g))),
          ("b", torch.nn.Parameter(torch.randn(3, 5, generator=g)))]
    return ParamArena(ps, "cpu"), ps


# ------------------------------------------------------------------ refusal
@pytest.mark.parametrize("bad", BAD[:-1])
def test_engine_refuses_a_decay_outside_0_1(bad):
    """[0, 1) only: NaN, negative values and 1.0 are refused the way
    label_smoothing is, before the model is touched."""
    from fpnmt.train import TrainEngine
    _require_feature()
    with pytest.raises(ValueError, match="ema_decay"):
        TrainEngine(None, 0.0, ema_decay=bad)


def test_arena_and_setters_refuse_a_bad_decay():
    from fpnmt.arena import check_ema_decay
    _require_feature()
    for bad in BAD:
        with pytest.raises(ValueError):
            check_ema_decay(bad)
    for ok in (0, 0.0, 0.5, 0.9999, np.float32(0.99), 1.0 - 2.0 ** -53):
        assert check_ema_decay(ok) == float(ok)
    ar, _ = _cpu_arena()
    for bad in BAD:
        with pytest.raises(ValueError):
            ar.enable_ema(bad)
    assert ar.ema is None and ar.ema_desc is None  # a refused call allocates nothing
    with pytest.raises(ValueError):
        ar.set_ema_decay(0.5)  # not enabled
    with pytest.raises(ValueError):
        ar.reset_ema()
    with pytest.raises(ValueError):
        ar.amsgrad_step(1e-3, ema=True)
    ar.enable_ema(0.9)
    for bad in BAD:
        with pytest.raises(ValueError):
            ar.set_ema_decay(bad)
    assert ar.ema_desc.decay == 0.9  # a refused value changes nothing


# ------------------------------------------------------------------ formula
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_omd_t_is_tf_min_decay_formula(decay):
    """1 - omd_t against tf.train.ExponentialMovingAverage's
    min(decay, (1 + t) / (10 + t)) in fp64 for t = 1..50, for the host
    restatement and the reference. omd is fp32(1 - decay): the decay the
    kernel applies differs from the one asked for by at most that rounding,
    2^-24 relative to 1 - decay <= 1."""
    from fpnmt.arena import ema_omd_t, ema_one_minus_decay
    _require_feature()
    omd = ema_one_minus_decay(decay)
    assert omd == one_minus_decay_f32(decay) == float(np.float32(1.0 - decay))
    assert abs(omd - (1.0 - decay)) <= 2.0 ** -24
    for t in range(1, 51):
        tf = min(decay, (1.0 + t) / (10.0 + t))
        for fn in (ema_omd_t, omd_t):
            got = fn(omd, True, float(t))
            assert abs((1.0 - got) - tf) <= 2.0 ** -24 + 4 * np.finfo(np.float64).eps, (t, fn)
            assert fn(omd, False, float(t)) == omd
    # debias off at decay 0: the average is the parameter itself
    assert ema_omd_t(ema_one_minus_decay(0.0), False, 1.0) == 1.0


# ---------------------------------------------------------------- reference
def _run(ref, p_of_step, steps):
    """Drive the reference with lr 0 (the optimizer leaves p alone) and set p
    by hand before every step: the shadow then follows a known sequence."""
    params = {"p": np.array(p_of_step(0), np.float64)}
    ref.reset(params)
    out = []
    for k in range(1, steps + 1):
        params["p"] = np.array(p_of_step(k), np.float64)
        ref.apply(params, {"p": np.zeros_like(params["p"])}, lambda it: 0.0)
        out.append(ref.ema["p"].copy())
    return out


def test_reference_closed_forms():
    """A constant parameter keeps its shadow exactly. A linear ramp p_k = a +
    b k without debias has the closed form e_k = p_k - b d (1 - d^k) / (1 - d)
    (from e_k = d e_{k-1} + (1 - d) p_k, e_0 = p_0)."""
    _require_feature()
    c = np.array([1.25, -3.0, 0.0])
    for debias in (True, False):
        ref = EmaAMSGradRef({"p": (3,)}, 0.9, debias=debias, clipnorm=0.0)
        for e in _run(ref, lambda k: c, 6):
            assert np.array_equal(e, c)
    a, b = np.array([0.5, -1.0]), np.array([0.25, 2.0])
    ref = EmaAMSGradRef({"p": (2,)}, 0.9, debias=False, clipnorm=0.0)
    d = 1.0 - ref.omd
    for k, e in enumerate(_run(ref, lambda k: a + b * k, 12), start=1):
        want = (a + b * k) - b * d * (1.0 - d ** k) / (1.0 - d)
        assert np.allclose(e, want, rtol=1e-13, atol=1e-13), k
    # with debias the first steps weigh the new value by 9 / (10 + t)
    ref = EmaAMSGradRef({"p": (2,)}, 0.9999, debias=True, clipnorm=0.0)
    es = _run(ref, lambda k: a + b * k, 2)
    e1 = a + (9.0 / 11.0) * ((a + b) - a)
    e2 = e1 + (9.0 / 12.0) * ((a + 2 * b) - e1)
    assert np.allclose(es[0], e1, rtol=1e-15) and np.allclose(es[1], e2, rtol=1e-15)


def test_reference_skips_frozen_and_leaves_the_step_alone():
    """The EMA reference's parameters and moments are GroupedAMSGradRef's."""
    from param_groups_ref import GroupedAMSGradRef
    _require_feature()
    rng = np.random.default_rng(0)
    shapes = {"a": (5,), "f": (4,)}
    rows = {"a": (1.0, 0.01, False), "f": (1.0, 0.0, True)}
    base = GroupedAMSGradRef(shapes)
    ref = EmaAMSGradRef(shapes, 0.5, debias=False)
    p0 = {n: rng.standard_normal(s) for n, s in shapes.items()}
    pa, pb = {n: v.copy() for n, v in p0.items()}, {n: v.copy() for n, v in p0.items()}
    for _ in range(3):
        g = {n: rng.standard_normal(s) for n, s in shapes.items()}
        base.apply(pa, g, lambda it: 1e-2, rows)
        ref.apply(pb, g, lambda it: 1e-2, rows)
    for n in shapes:
        assert np.array_equal(pa[n], pb[n]) and np.array_equal(base.vhat[n], ref.vhat[n])
    assert np.array_equal(ref.ema["f"], p0["f"])
    assert not np.array_equal(ref.ema["a"], p0["a"]) and not np.array_equal(ref.ema["a"], pb["a"])


# --------------------------------------------------------------- descriptor
def test_descriptor_host_mirror():
    """ParamArena.enable_ema on a CPU arena: the shadow starts as a copy of
    flat, the 16-byte descriptor holds fp32(1 - decay) and the debias flag,
    and set_ema_decay rewrites it in the same storage."""
    from fpnmt import _lib as L
    _require_feature()
    assert ctypes.sizeof(L.EmaDesc) == 16
    assert [f[0] for f in L.EmaDesc._fields_] == ["one_minus_decay", "debias", "reserved"]
    ar, ps = _cpu_arena()
    ema = ar.enable_ema(0.999, debias=True)
    assert ema is ar.ema and ema.dtype == torch.float32 and ema.shape == ar.flat.shape
    assert torch.equal(ema, ar.flat) and ema.data_ptr() != ar.flat.data_ptr()
    d = ar.ema_desc
    assert d.table.numel() * d.table.element_size() == 16
    assert d.host() == (one_minus_decay_f32(0.999), 1)
    assert (d.decay, d.one_minus_decay, d.debias) == (0.999, one_minus_decay_f32(0.999), True)
    where = d.table.data_ptr()
    ar.set_ema_decay(0.5)
    assert d.table.data_ptr() == where and ar.ema_desc is d
    assert d.host() == (0.5, 1) and d.decay == 0.5
    ar.enable_ema(0.25, debias=False)  # again: new values in place, the average is kept
    assert ar.ema is ema and ar.ema_desc is d and d.host() == (0.75, 0)
    with torch.no_grad():
        ar.flat.add_(1.0)
    assert not torch.equal(ar.ema, ar.flat)
    ar.reset_ema()
    assert torch.equal(ar.ema, ar.flat)


# ------------------------------------------------------------------ symbols
def test_symbols_in_header_library_and_binding():
    from fpnmt import _lib as L
    _require_feature()
    with open(L.HEADER_PATH) as f:
        header = f.read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("fpnmt_amsgrad_step_ema", "fpnmt_swap_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert "typedef struct fpnmt_ema_desc" in header
    assert len(L.SIGNATURES["fpnmt_amsgrad_step_ema"]) == len(L.SIGNATURES["fpnmt_amsgrad_step_groups"]) + 2
    assert ctypes.sizeof(L.AdamDesc) == 10 * 4  # fpnmt_adam_desc keeps its layout
    # argument validation happens before any HIP call
    nul = [None] * 23
    args = [None, 0, 0, 0, 0, None, None, 16384] + [None] * 16
    assert len(args) == len(L.SIGNATURES["fpnmt_amsgrad_step_ema"]) == 24 and len(nul) == 23
    assert L.lib.fpnmt_amsgrad_step_ema(*args) == L.E_ARG
    assert b"ema" in L.lib.fpnmt_last_error()
    assert L.lib.fpnmt_swap_f32(None, None, 0, None) == 0  # nothing to do
    assert L.lib.fpnmt_swap_f32(None, None, -1, None) == L.E_ARG
    assert L.lib.fpnmt_swap_f32(None, None, 4, None) == L.E_ARG
    buf = (ctypes.c_float * 8)()
    base = ctypes.addressof(buf)
    assert L.lib.fpnmt_swap_f32(base, base + 8, 4, None) == L.E_ARG  # [0, 4) and [2, 6) overlap
    assert b"overlap" in L.lib.fpnmt_last_error()


def test_pipeline_and_checkpoint_surface():
    from fpnmt.checkpoint import Checkpoint
    from fpnmt.train import TrainEngine
    from utils.pipeline import Pipeline
    _require_feature()
    sig = inspect.signature(Pipeline.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_debias"].default is True
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_debias"].default is True
    for fn in ("eval_step", "validate", "score_captions", "predict_batch", "evaluate"):
        assert inspect.signature(getattr(Pipeline, fn)).parameters["weights"].default == "model", fn
    for fn in ("set_ema_decay", "reset_ema", "ema_weights"):
        assert callable(getattr(TrainEngine, fn)), fn
    assert callable(Checkpoint.export_ema)
    assert math.isclose(one_minus_decay_f32(0.9), 0.1, rel_tol=1e-7)
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "ema_ref.py"))

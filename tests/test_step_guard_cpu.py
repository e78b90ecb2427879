"""Host side of global-norm clipping and the non-finite step guard
(TrainEngine(global_clipnorm=..., skip_nonfinite=...), ParamArena.enable_guard,
fpnmt_grad_norm_total, fpnmt_amsgrad_step_guard) and the fp64 reference
tests/step_guard_ref.py. No GPU."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from step_guard_ref import F32_MAX, GuardedAMSGradRef

NEW = ("fpnmt_grad_norm_total", "fpnmt_amsgrad_step_guard")


def _require_feature():
    from fpnmt import _lib as L
    from fpnmt.arena import ParamArena
    from fpnmt.train import TrainEngine
    from utils.pipeline import Pipeline
    assert all(n in L.ALL_SYMBOLS for n in NEW)
    assert hasattr(ParamArena, "enable_guard")
    assert "guard" in inspect.signature(ParamArena.amsgrad_step).parameters
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert "global_clipnorm" in sig and "skip_nonfinite" in sig
    assert hasattr(Pipeline, "guard_stats")


def _cpu_arena():
    from fpnmt.arena import ParamArena
    g = torch.Generator().manual_seed(0)
    ps = [("a", torch.nn.Parameter(torch.randn(70, generator=g))),
          ("b", torch.nn.Parameter(torch.randn(3, 5, generator=g)))]
    return ParamArena(ps, "cpu"), ps


# ---------------------------------------------------------------- reference
def test_reference_against_a_hand_computed_two_segment_case():
    """a = (3, 4), b = (12): ||g||^2 = 9 + 16 + 144 = 169, ||g|| = 13, so a
    global clip of 1 scales by 1/13. First step of AMSGrad at a constant rate
    lr (beta1 0.9, beta2 0.98): m = 0.1 g, v = vhat = 0.02 g^2,
    alpha = lr sqrt(0.02) / 0.1, p' = p - alpha m / (sqrt(vhat) + eps)."""
    _require_feature()
    lr, eps = 1e-2, 1e-9
    ref = GuardedAMSGradRef({"a": (2,), "b": (1,)}, global_clipnorm=1.0, clipnorm=0.0)
    p = {"a": np.array([1.0, -2.0]), "b": np.array([0.5])}
    g = {"a": np.array([3.0, -4.0]), "b": np.array([12.0])}
    ref.apply(p, g, lambda it: lr)
    assert ref.sumsq_total == 169.0 and ref.clip_factor == 1.0 / 13.0
    assert (ref.skipped, ref.n_applied, ref.n_skipped, ref.consecutive, ref.iterations) == (0, 1, 0, 0, 1)
    alpha = lr * math.sqrt(0.02) / 0.1
    for n, p0, g0 in (("a", [1.0, -2.0], [3.0, -4.0]), ("b", [0.5], [12.0])):
        for i, (pi, gi) in enumerate(zip(p0, g0)):
            gc = gi / 13.0
            m, v = 0.1 * gc, 0.02 * gc * gc
            want = pi - alpha * m / (math.sqrt(v) + eps)
            assert math.isclose(ref.m[n][i], m, rel_tol=1e-14) and math.isclose(ref.v[n][i], v, rel_tol=1e-14)
            assert math.isclose(p[n][i], want, rel_tol=1e-14), (n, i)
            assert math.isclose(p[n][i], pi - lr * math.copysign(1.0, gi), rel_tol=1e-6)  # Adam's first step
    # a clip above the norm leaves the gradient alone
    big = GuardedAMSGradRef({"a": (2,), "b": (1,)}, global_clipnorm=20.0, clipnorm=0.0)
    none = GuardedAMSGradRef({"a": (2,), "b": (1,)}, global_clipnorm=0.0, clipnorm=0.0)
    pa = {"a": np.array([1.0, -2.0]), "b": np.array([0.5])}
    pb = {k: v.copy() for k, v in pa.items()}
    big.apply(pa, g, lambda it: lr)
    none.apply(pb, g, lambda it: lr)
    assert big.clip_factor == 1.0 and none.clip_factor == 1.0
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    # a frozen tensor and a supplied norm: b frozen, a's norm given as 100 -> factor 1/10
    fz = GuardedAMSGradRef({"a": (2,), "b": (1,)}, global_clipnorm=1.0, clipnorm=0.0)
    pc = {"a": np.array([1.0, -2.0]), "b": np.array([0.5])}
    fz.apply(pc, {"a": g["a"], "b": np.array([float("nan")])}, lambda it: lr,
             rows={"b": (1.0, 0.0, True)}, norms={"a": 100.0})
    assert fz.sumsq_total == 100.0 and fz.clip_factor == 0.1 and fz.skipped == 0 and pc["b"][0] == 0.5
    with pytest.raises(ValueError):
        GuardedAMSGradRef({"a": (2,)}, global_clipnorm=1.0, clipnorm=1.0)


@pytest.mark.parametrize("bad", ["inf", "nan", "overflow"])
def test_reference_skip_rule(bad):
    """Inf, NaN, and two finite 1.5e19 whose squares (2.25e38) are finite in
    fp32 and whose sum (4.5e38) is not: the step is skipped, nothing moves,
    and a clean step afterwards equals a twin that only took the clean one."""
    _require_feature()
    shapes = {"a": (3,), "b": (2,)}
    rng = np.random.default_rng(1)
    p0 = {n: rng.standard_normal(s) for n, s in shapes.items()}
    clean = {n: rng.standard_normal(s) for n, s in shapes.items()}
    poison = {n: v.copy() for n, v in clean.items()}
    if bad == "overflow":
        poison["a"][0] = poison["b"][1] = 1.5e19
        assert 2 * 1.5e19 ** 2 > F32_MAX > 1.5e19 ** 2
    else:
        poison["b"][1] = float(bad)
    A = GuardedAMSGradRef(shapes, 0.9, global_clipnorm=0.5, clipnorm=0.0)
    T = GuardedAMSGradRef(shapes, 0.9, global_clipnorm=0.5, clipnorm=0.0)
    pa, pt = ({n: v.copy() for n, v in p0.items()} for _ in range(2))
    for k in range(2):
        A.apply(pa, poison, lambda it: 1e-2)
        assert (A.skipped, A.n_skipped, A.consecutive, A.n_applied, A.iterations) == (1, k + 1, k + 1, 0, 0)
        assert all(np.array_equal(pa[n], p0[n]) and not A.m[n].any() and not A.vhat[n].any() for n in shapes)
        assert all(np.array_equal(A.ema[n], p0[n]) for n in shapes)
    A.apply(pa, clean, lambda it: 1e-2)
    T.apply(pt, clean, lambda it: 1e-2)
    assert (A.skipped, A.n_skipped, A.consecutive, A.n_applied, A.iterations) == (0, 2, 0, 1, 1)
    for n in shapes:
        assert np.array_equal(pa[n], pt[n]) and np.array_equal(A.ema[n], T.ema[n]) and np.array_equal(A.v[n], T.v[n])
        assert not np.array_equal(pa[n], p0[n])


# ------------------------------------------------------------------ records
def test_record_layouts():
    from fpnmt import _lib as L
    _require_feature()
    assert ctypes.sizeof(L.GuardDesc) == 16 and ctypes.sizeof(L.GuardState) == 32
    assert ctypes.sizeof(L.AdamDesc) == 40  # fpnmt_adam_desc keeps its layout
    assert ctypes.sizeof(L.EmaDesc) == 16
    assert [f[0] for f in L.GuardDesc._fields_] == ["global_clipnorm", "reserved"]
    off = {f[0]: getattr(L.GuardState, f[0]).offset for f in L.GuardState._fields_}
    assert off == {"sumsq_total": 0, "clip_factor": 4, "skipped": 8, "consecutive": 12, "n_skipped": 16,
                   "n_applied": 24}


def test_symbols_in_header_library_and_binding():
    from fpnmt import _lib as L
    _require_feature()
    with open(L.HEADER_PATH) as f:
        header = f.read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    for rec in ("fpnmt_guard_desc", "fpnmt_guard_state"):
        assert "typedef struct " + rec in header, rec
    # the argument counts of the header's prototypes and of the binding agree
    for name in NEW + ("fpnmt_amsgrad_step_ema",):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(proto.split(",")) == len(L.SIGNATURES[name]), name
    assert len(L.SIGNATURES["fpnmt_amsgrad_step_guard"]) == len(L.SIGNATURES["fpnmt_amsgrad_step_ema"]) + 2
    # argument validation happens before any HIP call: null records
    args = [None, 0, 0, 1, 0, None, None, 16384] + [None] * 18
    assert len(args) == len(L.SIGNATURES["fpnmt_amsgrad_step_guard"]) == 26
    assert L.lib.fpnmt_amsgrad_step_guard(*args) == L.E_ARG
    assert b"guard" in L.lib.fpnmt_last_error()
    assert L.lib.fpnmt_grad_norm_total(0, None, None, None, None, None, None, 1.0, None, None, None) == L.E_ARG
    assert b"guard" in L.lib.fpnmt_last_error()


def test_guard_records_host_mirror():
    from fpnmt import _lib as L
    from fpnmt.arena import check_global_clipnorm
    _require_feature()
    ar, _ = _cpu_arena()
    assert ar.guard is None
    with pytest.raises(ValueError):
        ar.set_global_clipnorm(1.0)  # not enabled
    for bad in (float("nan"), float("inf"), -1.0, "x", None):
        with pytest.raises(ValueError):
            check_global_clipnorm(bad)
        with pytest.raises(ValueError):
            ar.enable_guard(bad)
    assert ar.guard is None  # a refused call allocates nothing
    g = ar.enable_guard(0.25)
    assert g is ar.guard and g.global_clipnorm == 0.25
    assert g.desc.numel() * g.desc.element_size() == ctypes.sizeof(L.GuardDesc)
    assert g.state.numel() * g.state.element_size() == ctypes.sizeof(L.GuardState)
    assert float(g.desc.view(torch.float32)[0]) == 0.25 and not g.desc[1:].any()
    assert g.host() == {"sumsq_total": 0.0, "clip_factor": 0.0, "skipped": 0, "consecutive": 0, "n_skipped": 0,
                        "n_applied": 0}
    where = g.desc.data_ptr(), g.state.data_ptr()
    ar.set_global_clipnorm(0)
    assert ar.enable_guard(2.0) is g and (g.desc.data_ptr(), g.state.data_ptr()) == where
    assert float(g.desc.view(torch.float32)[0]) == 2.0
    g.set_counts(2 ** 33 + 5, 7)
    raw = L.GuardState.from_buffer_copy(g.state.numpy().tobytes())
    assert (raw.n_skipped, raw.n_applied) == (2 ** 33 + 5, 7)
    raw.sumsq_total, raw.clip_factor, raw.skipped, raw.consecutive = 169.0, 0.5, 1, 3
    g.state.copy_(torch.frombuffer(bytearray(bytes(raw)), dtype=torch.int32))
    assert g.stats() == {"grad_norm": 13.0, "clip_factor": 0.5, "skipped": 1, "consecutive": 3,
                         "n_skipped": 2 ** 33 + 5, "n_applied": 7}
    assert int(g.skipped) == 1 and g.skipped.data_ptr() == g.state.data_ptr() + 8


# ------------------------------------------------------------------ refusals
def test_arena_refuses_a_step_it_could_not_skip_as_a_whole():
    _require_feature()
    ar, _ = _cpu_arena()
    assert ar.nblocks == 2
    with pytest.raises(ValueError, match="enable_guard"):
        ar.amsgrad_step(1e-3, clipnorm=0.0, guard=True)
    ar.enable_guard(0.0)
    with pytest.raises(ValueError, match="inc_step"):
        ar.amsgrad_step(1e-3, clipnorm=0.0, guard=True, inc_step=False)
    for blocks in ((0, 1), (1, 2), (1, 1)):
        with pytest.raises(ValueError, match="not frozen"):
            ar.amsgrad_step(1e-3, clipnorm=0.0, guard=True, blocks=blocks)
    groups = ar.make_groups([(0, 1.0, 0.0, True), (0, 1.0, 0.0, False)])  # a frozen, b trainable
    with pytest.raises(ValueError, match="not frozen"):
        ar.amsgrad_step(1e-3, clipnorm=0.0, guard=True, blocks=(0, 1), groups=groups)
    ar.set_global_clipnorm(1.0)
    with pytest.raises(ValueError, match="exclusive"):
        ar.amsgrad_step(1e-3, clipnorm=1.0, guard=True)
    assert int(ar.step) == 0


def test_engine_refuses_both_clips_and_the_early_update():
    """Before the model is touched, like ema_decay's check."""
    import fpnmt
    from fpnmt.train import TrainEngine
    _require_feature()
    with pytest.raises(ValueError, match="exclusive"):
        TrainEngine(None, 0.0, clipnorm=1.0, global_clipnorm=1.0)
    with pytest.raises(ValueError, match="exclusive"):
        TrainEngine(None, 0.0, global_clipnorm=0.5)  # the default clipnorm is the reference's 1.0
    for bad in (float("nan"), float("inf"), -1.0, "x"):
        with pytest.raises(ValueError, match="global_clipnorm"):
            TrainEngine(None, 0.0, clipnorm=0.0, global_clipnorm=bad)
    assert fpnmt.config.early_update is False
    fpnmt.config.early_update = True
    try:
        for kw in (dict(skip_nonfinite=True), dict(clipnorm=0.0, global_clipnorm=1.0), dict(global_clipnorm=0.0)):
            with pytest.raises(ValueError, match="early_update"):
                TrainEngine(None, 0.0, **kw)
    finally:
        fpnmt.config.early_update = False


def test_pipeline_surface_and_clipnorm_for():
    from fpnmt.train import TrainEngine
    from utils.pipeline import Pipeline, clipnorm_for
    _require_feature()
    with pytest.raises(ValueError):
        clipnorm_for("global")  # the mode switch stays the reference's two
    assert clipnorm_for("per_tensor") == 1.0 and clipnorm_for("none") == 0.0
    sig = inspect.signature(Pipeline.__init__).parameters
    assert sig["global_clipnorm"].default is None and sig["skip_nonfinite"].default is False
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert sig["global_clipnorm"].default is None and sig["skip_nonfinite"].default is False
    with pytest.raises(ValueError, match="clipnorm_mode='none'"):
        Pipeline(target_vocab_size=50, device="cpu", global_clipnorm=1.0)  # the default mode is per_tensor
    for fn in ("set_global_clipnorm", "guard_stats"):
        assert callable(getattr(TrainEngine, fn)), fn


def test_mean_keep_selects_and_does_not_multiply():
    """Mean(value, keep=0) leaves a NaN out altogether (NaN * 0 would not)."""
    from utils.utils import Mean
    _require_feature()
    m = Mean()
    one, zero = torch.ones((), dtype=torch.int32), torch.zeros((), dtype=torch.int32)
    m(torch.tensor(2.0), keep=one)
    m(torch.tensor(float("nan")), keep=zero)
    m(torch.tensor(float("inf")), keep=zero)
    m(torch.tensor(4.0), keep=one)
    assert float(m.result()) == 3.0
    m(torch.tensor(6.0))  # without keep: as before
    assert float(m.result()) == 4.0

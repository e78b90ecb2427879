"""Host model of the parameter groups (fpnmt/param_groups.py) and the fp64
reference of the grouped optimizer step (tests/param_groups_ref.py). No GPU."""
import math

import numpy as np
import pytest
import torch

from param_groups_ref import GroupedAMSGradRef


@pytest.mark.parametrize("const_lr", [None, 1e-2])
def test_reference_with_default_groups_is_keras_amsgrad(const_lr):
    """Every group at (1, 0, False): the reference is oracle.ref_cpu.
    KerasAMSGrad on the tensors of test_amsgrad_matches_keras, to that test's
    atol 1e-6, rtol 1e-5."""
    from oracle import ref_cpu as R
    from utils.utils import CustomSchedule
    torch.manual_seed(0)
    ps = [("a", torch.randn(300, 7)), ("emb", torch.randn(50, 16)), ("c", torch.randn(5))]
    opt = R.KerasAMSGrad([n for n, _ in ps], [p.shape for _, p in ps], sparse=["emb"])
    ref = GroupedAMSGradRef({n: tuple(p.shape) for n, p in ps}, sparse=["emb"])
    sched = CustomSchedule(2048, 4000)
    lr_fn = sched if const_lr is None else (lambda it: const_lr)
    params = {n: p.clone() for n, p in ps}
    params64 = {n: p.double().numpy().copy() for n, p in ps}
    rows = {n: (1.0, 0.0, False) for n, _ in ps}
    for _ in range(3):
        grads = {n: torch.randn(p.shape) * (5 if n == "a" else 0.1) for n, p in ps}
        emb_ss = float((grads["emb"].double() ** 2).sum()) * 1.7
        opt.apply(params, grads, lr_fn, norms={"emb": emb_ss})
        ref.apply(params64, {n: g.double().numpy() for n, g in grads.items()}, lr_fn, rows, norms={"emb": emb_ss})
    assert ref.iterations == 3
    for n, _ in ps:
        assert np.allclose(params64[n], params[n].double().numpy(), atol=1e-6, rtol=1e-5), n


def test_reference_scale_decay_frozen():
    """One step by hand: scale multiplies the Adam term, decay is decoupled
    and uses the old parameter, lr_scale 0 only decays, frozen skips."""
    ref = GroupedAMSGradRef({k: (2,) for k in "abcd"}, clipnorm=0.0)
    p0 = np.array([1.0, -2.0])
    params = {k: p0.copy() for k in "abcd"}
    grads = {k: np.array([0.5, 0.25]) for k in "abcd"}
    rows = {"a": (1.0, 0.0, False), "b": (3.0, 0.01, False), "c": (0.0, 0.01, False), "d": (3.0, 0.01, True)}
    lr = 0.1
    ref.apply(params, grads, lambda it: lr, rows)
    adam = p0 - params["a"]  # the unscaled Adam term
    assert np.all(np.abs(adam) > 0)
    assert np.allclose(params["b"], p0 - 3.0 * adam - lr * 3.0 * 0.01 * p0, rtol=1e-14, atol=0)
    assert np.array_equal(params["c"], p0)  # lr * 0 * w = 0: nothing moves ...
    assert np.all(ref.m["c"] != 0) and np.all(ref.vhat["c"] != 0)  # ... but the moments advance
    assert np.array_equal(params["d"], p0)
    assert not ref.m["d"].any() and not ref.v["d"].any() and not ref.vhat["d"].any()


class _P:
    def __init__(self, *shape):
        self.shape = shape
        self.ndim = len(shape)


def test_assign_first_match_wins_and_default_group():
    from fpnmt.param_groups import DEFAULT_ROW, ParamGroup, assign, decay_matrices
    names = ["enc.a.kernel", "enc.a.bias", "enc.b.kernel", "dec.kernel", "dec.bias"]
    params = [_P(3, 4), _P(4), _P(4, 4), _P(4, 2), _P(2)]
    groups = [ParamGroup("a", ("enc.a.",), lr_scale=0.1, frozen=True),
              ParamGroup("enc", ("enc.",), lr_scale=0.5, weight_decay=decay_matrices(0.01)),
              ParamGroup("bias", lambda n, p: n.endswith("bias"), lr_scale=2.0)]
    rows = assign(names, params, groups)
    assert rows[0] == (0, 0.1, 0.0, True) and rows[1] == (0, 0.1, 0.0, True)  # "a" before "enc"
    assert rows[2] == (1, 0.5, 0.01, False)
    assert rows[3] == DEFAULT_ROW == (-1, 1.0, 0.0, False)  # unmatched: the implicit default group
    assert rows[4] == (2, 2.0, 0.0, False)  # a callable match
    assert assign(names, params, []) == [DEFAULT_ROW] * 5
    assert assign(names, params, None) == [DEFAULT_ROW] * 5


def test_assign_rejects_bad_groups():
    from fpnmt.param_groups import ParamGroup, assign, decay_matrices
    names, params = ["x.kernel", "y.kernel"], [_P(2, 2), _P(2, 2)]
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lr_scale"):
            assign(names, params, [ParamGroup("g", ("x.",), lr_scale=bad)])
        with pytest.raises(ValueError, match="weight_decay"):
            assign(names, params, [ParamGroup("g", ("x.",), weight_decay=bad)])
        with pytest.raises(ValueError, match="weight_decay"):  # a callable's value is checked too
            assign(names, params, [ParamGroup("g", ("x.",), weight_decay=lambda n, p, b=bad: b)])
    with pytest.raises(ValueError):
        decay_matrices(-0.1)
    with pytest.raises(ValueError, match="duplicate"):
        assign(names, params, [ParamGroup("g", ("x.",)), ParamGroup("g", ("y.",))])
    with pytest.raises(ValueError, match="match no parameter"):
        assign(names, params, [ParamGroup("g", ("x.",)), ParamGroup("h", ("z.",))])
    with pytest.raises(ValueError, match="match no parameter"):  # everything it matches is already owned
        assign(names, params, [ParamGroup("g", ("x.", "y.")), ParamGroup("h", ("y.",))])
    # the legal edge: lr_scale 0 without frozen
    assert assign(names, params, [ParamGroup("g", ("x.",), lr_scale=0.0)])[0] == (0, 0.0, 0.0, False)


@pytest.fixture(scope="module")
def model(request):
    """test_gpu_model._build's model, on the CPU."""
    import test_gpu_model as T
    dev = T.DEV
    T.DEV = "cpu"
    try:
        m, _, _ = T._build(num_layers=1, vocab=300, image=128, max_seq_len=12)
    finally:
        T.DEV = dev
    return m


def test_helper_prefixes_cover_backbone_and_feature_extractor(model):
    from fpnmt import param_groups as G
    named = list(model.named_parameters())
    names, params = [n for n, _ in named], [p for _, p in named]
    bb = "encoder.feature_extractor.retinanet_model.backbone."
    fe = "encoder.feature_extractor."
    rows = G.assign(names, params, [G.backbone_group(model, lr_scale=0.1)])
    got = {n for n, r in zip(names, rows) if r[0] == 0}
    assert got == {n for n in names if n.startswith(bb)} and got
    rows = G.assign(names, params, [G.feature_extractor_group(model, frozen=True)])
    got = {n for n, r in zip(names, rows) if r[0] == 0}
    assert got == {n for n in names if n.startswith(fe)} and len(got) > len([n for n in names if n.startswith(bb)])
    assert all(r[3] for n, r in zip(names, rows) if n.startswith(fe))
    assert all(r == G.DEFAULT_ROW for n, r in zip(names, rows) if not n.startswith(fe))
    # the prefixes are the staged backward's, not typed in again
    stage = model.encoder.feature_extractor.stage_prefixes()
    assert set(G.feature_extractor_prefixes(model)) == {fe + p for ps in stage for p in ps}
    assert set(G.backbone_prefixes(model)) == {fe + p for ps in stage[2:] for p in ps}


def test_decay_matrices_leaves_vectors_alone(model):
    from fpnmt import param_groups as G
    named = list(model.named_parameters())
    names, params = [n for n, _ in named], [p for _, p in named]
    rows = G.assign(names, params, [G.ParamGroup("all", lambda n, p: True, weight_decay=G.decay_matrices(0.01))])
    vec = [r for p, r in zip(params, rows) if p.ndim < 2]
    mat = [r for p, r in zip(params, rows) if p.ndim >= 2]
    assert vec and mat
    assert all(r[2] == 0.0 for r in vec)
    assert all(r[2] == 0.01 for r in mat)


def test_recipe_groups(model):
    from fpnmt import param_groups as G
    assert G.recipe_groups(model) is None  # the defaults: the plain step
    named = list(model.named_parameters())
    names, params = [n for n, _ in named], [p for _, p in named]
    bb = "encoder.feature_extractor.retinanet_model.backbone."
    fe = "encoder.feature_extractor."
    rows = G.assign(names, params, G.recipe_groups(model, backbone_lr_scale=0.1, weight_decay=0.01))
    for n, p, r in zip(names, params, rows):
        assert r[1] == (0.1 if n.startswith(bb) else 1.0), n
        assert r[2] == (0.01 if p.ndim >= 2 else 0.0), n
        assert not r[3]
    rows = G.assign(names, params, G.recipe_groups(model, freeze=("backbone",)))
    assert all(r[3] == n.startswith(bb) for n, r in zip(names, rows))
    rows = G.assign(names, params, G.recipe_groups(model, freeze=("feature_extractor",)))
    assert all(r[3] == n.startswith(fe) for n, r in zip(names, rows))
    with pytest.raises(ValueError, match="freeze"):
        G.recipe_groups(model, freeze=("decoder",))
    with pytest.raises(ValueError):
        G.recipe_groups(model, backbone_lr_scale=math.nan)


def test_seg_group_struct_matches_header():
    """The ctypes mirror of fpnmt_seg_group has the header's 16-B layout, and
    the new entry points are exported."""
    import ctypes
    from fpnmt import _lib as L
    assert ctypes.sizeof(L.SegGroup) == 16
    assert [f[0] for f in L.SegGroup._fields_] == ["lr_scale", "weight_decay", "frozen", "reserved"]
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "fpnmt_amsgrad_step_groups") and hasattr(lib, "fpnmt_grad_sumsq_groups")
    # argument validation happens before any HIP call
    assert L.lib.fpnmt_amsgrad_step_groups(None, 0, 0, 0, 0, None, None, 16384, None, None, None, None, None, None,
                                           None, None, None, None, None, None, None, None) == L.E_ARG
    assert b"group table" in L.lib.fpnmt_last_error()

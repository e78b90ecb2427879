"""The convolutions outside the GEMM dispatch on the GPU: the 7x7 / 2 stem
forward and weight gradient, the single-filter kernels, the fused bottleneck
and the weight-prep kernels, element by element against fp64 on the case
table of tests/conv_special_cases.py (whose bounds and route restatements
tests/test_conv_special_bars.py proves able to fail).

The C entry points are called directly through fpnmt._lib, in ONE fresh child
process with FPNMT_GEMM_LOG set (the log is opened once per process); it stops
at the first failed call or HIP error, and then every test here fails without
anything else being started. For every case:

1. the logged `conv` line (kernel=, grid=, shape, levels) is the table's, or,
   for a fallback, a GEMM line was logged and no `conv` line;
2. every element is within its bound of the fp64 reference (the worst
   err / bound per output is printed); exact cases are bitwise equal; the Inf
   case's non-finite set is the reference's;
3. every output sits between sentinel guards that come back untouched, and
   every live element was written (weight gradients are pre-filled, so `=`
   for `+=` fails 2.);
4. a second run into fresh buffers is bitwise equal;
5. the agreements that must be bitwise hold: the stem weight gradient inside
   and outside a deferred-reduction region, the masked bwd-data and
   plain x (y > 0), the batched and the single weight prep;
6. the bottleneck's error returns and FPNMT_E_UNSUPPORTED leave y at the
   sentinel.
"""
import os
import subprocess
import sys

import pytest
import torch

import conv_special_cases as T

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 600  # the table runs in about a minute: imports, the 3 GiB deferred arena, ~130 cases x 2


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("conv_special")
    env = dict(os.environ, FPNMT_GEMM_LOG=str(out / "gemm.log"))
    r = subprocess.run([sys.executable, os.path.abspath(T.__file__), str(out)], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        return {"error": f"child exited {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"}
    return torch.load(out / "results.pt")


def _result(child, name):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    return child[name]


@pytest.mark.parametrize("name", [c.name for c in T.ROUTED])
def test_route(child, name):
    """Both runs logged exactly the table's line (or took the fallback)."""
    case, res = T.BY_NAME[name], _result(child, name)
    for lines in res["log"]:
        bad = T.route_errors(case, lines)
        assert not bad, (bad, lines)
    if case.family == "stem_wgrad":
        bad = T.route_errors(case, res["deferred_log"])
        # a fallback's GEMM may sit in the deferred queue (its line comes at the flush, inside the region)
        assert not bad, (bad, res["deferred_log"])


def _check_outputs(case, res):
    ref = T.reference(case)
    assert set(ref) == set(res["out"]), (sorted(ref), sorted(res["out"]))
    for key, (r, bnd) in ref.items():
        buf = res["out"][key]
        shape = tuple(r.shape)
        assert T.guards_ok(buf, shape), f"{key}: guard elements overwritten"
        out = T.live(buf, shape)
        ok, ratio = T.compare(out, r, bnd)
        print(f"{case.name} {key}: shape {shape} worst err/bound {ratio:.3e}" + (" (exact)" if bnd is None else ""))
        assert ok, f"{key}: outside the bound, worst err / bound {ratio:.3f}"
        if key != "dw":  # weight gradients are pre-filled; everything else starts at the sentinel
            assert bool((out != torch.tensor(T.SENTINEL, dtype=out.dtype)).all()), f"{key}: live elements left unwritten"
    assert res["same"], "two runs differ bitwise"


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_numerics(child, name):
    case, res = T.BY_NAME[name], _result(child, name)
    _check_outputs(case, res)
    if case.family == "stem_wgrad" and case.kernel != "fallback":
        assert res["deferred_same"], "deferred and immediate reductions differ bitwise"
    if case.family == "n1" and case.mask:
        for i in range(len(case.levels)):
            key = f"dx{i}"
            if key not in res["out"]:
                continue
            n, h, w = case.levels[i]
            shape = (n, h, w, case.c)
            y = T.inputs(case)["ys"][i]
            plain = T.live(res["plain"][key], shape)
            want = plain * (y > 0).to(plain.dtype)
            got = T.live(res["out"][key], shape)
            assert torch.equal(got, want), f"{key}: masked != plain x (y > 0)"


def test_bottleneck_error_returns(child):
    res = _result(child, "bneck_errors")
    want = {"null_y": T.E_ARG, "null_wa": T.E_ARG, "y_is_x": T.E_ARG, "y_off_16B": T.E_ARG, "x_off_16B": T.E_ARG,
            "shape_28x28x256": T.E_UNSUPPORTED, "shape_56x56x512": T.E_UNSUPPORTED}
    assert set(res) == set(want)
    for name, (status, untouched) in res.items():
        assert status == want[name], (name, status)
        assert untouched, f"{name}: y written"


def _wprep_check(case, out, shift=0):
    inp = T.inputs(case)
    ohwi, flip = T.wprep_expected(case, inp)
    for key, exp, on, sh in (("ohwi", ohwi, case.ohwi, 0), ("flip", flip, case.flip, shift)):
        buf = out[key]
        if not on:
            assert buf is None
            continue
        n = exp.numel() + sh
        assert T.guards_ok(buf, (n,)), f"{key}: guard elements overwritten"
        got = T.live(buf, (n,))
        sent = torch.tensor(T.SENTINEL, dtype=got.dtype)
        assert bool((got[:sh] == sent).all()), f"{key}: elements before the shifted destination written"
        # bitwise: the gaps of a padded ld_flip hold the sentinel in `exp` too
        assert torch.equal(got[sh:].view(torch.uint8), exp.contiguous().view(torch.uint8)), f"{key}: not bitwise (w * scale).to(dtype)"


@pytest.mark.parametrize("name", [c.name for c in T.WPREP])
def test_weight_prep(child, name):
    case, res = T.BY_NAME[name], _result(child, name)
    _wprep_check(case, res["out"])
    assert res["same"], "two runs differ bitwise"


@pytest.mark.parametrize("tag", ["bf16", "f32"])
@pytest.mark.parametrize("shift", [0, 1])
def test_weight_prep_batched(child, tag, shift):
    """All cases of a dtype as one launch (tile_start per item); shift 1 moves
    every flipped destination off its 8-B boundary (bf16: the scalar stores).
    Equal to the expected bits, hence to the unbatched results."""
    res = _result(child, f"wprep_batched_{tag}_shift{shift}")
    dtype = T.BF16 if tag == "bf16" else T.F32
    cases = [c for c in T.WPREP if c.dtype == dtype]
    assert set(res) == {c.name for c in cases}
    for c in cases:
        _wprep_check(c, res[c.name], shift)
        single = _result(child, c.name)["out"]
        if c.ohwi:
            assert torch.equal(res[c.name]["ohwi"].view(torch.uint8), single["ohwi"].view(torch.uint8))

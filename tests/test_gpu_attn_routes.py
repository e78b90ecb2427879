"""Every attention kernel route on the GPU: the route it took (the `attn`
lines of FPNMT_GEMM_LOG), every element of out / weights / dq / dk / dv
against the fp64 reference inside the derived bound, masked weights and the
weight columns from Lk to ldw bitwise zero, padding columns and guard rows
untouched, two runs bitwise equal.

The case table, the reference and the bound are tests/attn_route_cases.py;
tests/test_attn_route_bars.py proves without a GPU that the bound rejects a
dropped key, a dropped partial of the softmax sum or of sum P dP, a kept
masked key, a shifted mask row, a wrong head and a doubled scale.

The log file is opened once per process, so one fresh child process (as
test_gpu_gemm_routes.py does) runs the whole table twice with the log set; it
stops at the first failed call or HIP error, and then every case here fails
without anything else being started.
"""
import os
import subprocess
import sys

import pytest
import torch

import attn_route_cases as A

pytestmark = pytest.mark.gpu

# the table itself is seconds of GPU time (the largest launch is one (b, h) pair at Lk 4097);
# the child's time is imports, the first launch's code-object load and ~190 small host copies
CHILD_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("attn_routes")
    env = dict(os.environ, FPNMT_GEMM_LOG=str(out / "gemm.log"))
    r = subprocess.run([sys.executable, os.path.abspath(A.__file__), str(out)], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        return {"error": f"child exited {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"}
    return torch.load(out / "results.pt")


def _result(child, name):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    return child[name]


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_route(child, name):
    """The case logged exactly its table entry's attn lines, both runs."""
    res = _result(child, name)
    for lines in res["log"]:
        assert not A.route_errors(A.BY_NAME[name], lines), (A.route_errors(A.BY_NAME[name], lines), lines)


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_numerics(child, name):
    """|result - reference| <= bound on every element of every output; the
    exact checks (zero weights, untouched padding, repeatability)."""
    case = A.BY_NAME[name]
    bad, ratios = A.check_case(case, _result(child, name))
    print(f"route {name}: {case.fwd}/{case.bwd} {case.dname} worst err/bound "
          + " ".join(f"{n} {v:.2e}" for n, v in ratios.items()))
    assert not bad, bad


def test_all_attn_routes_logged(child):
    """The (op, kernel, dtype) triples seen in the log are exactly REACHABLE;
    the worst err / bound of each route."""
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    seen, worst = set(), {}
    for name in child:
        recs = A.parse_log(child[name]["log"][0])
        seen |= {(r["op"], r["kernel"], r["dtype"]) for r in recs}
        _, ratios = A.check_case(A.BY_NAME[name], child[name])
        c = A.BY_NAME[name]
        ops = {"attn": ("fwd", "bwd"), "views": ("views_fwd", "views_bwd"), "decode": ("decode", "")}[c.op]
        for key, outs in (((ops[0], c.fwd, c.dname), ("w", "out")), ((ops[1], c.bwd, c.dname), ("dq", "dk", "dv"))):
            vals = [ratios[n] for n in outs if n in ratios]
            if vals:
                worst[key] = max(worst.get(key, 0.0), max(vals))
    for key in sorted(worst):
        print("worst err/bound", *key, f"{worst[key]:.3f}")
    assert seen == A.REACHABLE, (sorted(A.REACHABLE - seen), sorted(seen - A.REACHABLE))

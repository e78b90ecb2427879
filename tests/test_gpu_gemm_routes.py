"""Every bf16 GEMM / conv dispatch route on the GPU: the route it took (from
FPNMT_GEMM_LOG), every output element against the fp64 reference inside the
derived bound, the padding untouched, two runs bitwise equal.

The case table, the reference and the bound are tests/gemm_route_cases.py;
tests/test_gemm_route_bars.py proves without a GPU that the bound rejects a
dropped K chunk / K-tile / tap / split, a swapped row and a zeroed N tail.

The log file is opened once per process, at the first GEMM, so one fresh child
process (as test_gemm_log_env does) runs the whole table twice with the log
set; it stops at the first failed call or HIP error, and then every case here
fails without anything else being started.

Bitwise repeatability is asserted for every case: all split forms in the table
are the ordered ones (workspace slabs + gemm_splitk_reduce_kernel /
gemm_small_reduce_kernel / wgrad_reduce_kernel, the deferred job queue's
whole-K tiles). The fp32-atomics fallback of a weight gradient whose slabs fit
neither the workspace nor the deferred arena is not in the table (it needs
slabs beyond the 256 MiB workspace) and is the one route left out of that check.
"""
import os
import subprocess
import sys

import pytest
import torch

import gemm_route_cases as G

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 420  # the table runs in ~1 min: imports, 3 GiB arena, ~60 cases x 2, host copies


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("gemm_routes")
    env = dict(os.environ, FPNMT_GEMM_LOG=str(out / "gemm.log"))
    r = subprocess.run([sys.executable, os.path.abspath(G.__file__), str(out)], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        return {"error": f"child exited {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"}
    return torch.load(out / "results.pt")


def _result(child, name):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    return child[name]


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_route(child, name):
    """The case produced exactly its table entry's log line, both runs."""
    res = _result(child, name)
    for lines in res["log"]:
        assert not G.route_errors(G.BY_NAME[name], lines), (G.route_errors(G.BY_NAME[name], lines), lines)


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_numerics(child, name):
    """|out - reference| <= bound on every element; sentinel padding columns
    and guard rows bitwise untouched; the second run bitwise equal."""
    case = G.BY_NAME[name]
    res = _result(child, name)
    buf = res["out"]
    rows, N = G.out_rows(case), case.dims[1]
    assert buf.shape == (rows + G.GUARD_ROWS, case.ldc) and buf.dtype == case.out_dtype
    ref, s_tot = G.reference(case)
    ok, ratio = G.compare(case, buf[:rows, :N], ref, G.bound(case, ref, s_tot))
    print(f"route {name}: dims {case.dims} worst err/bound {ratio:.2e}")
    assert ok, f"elements outside the bound, worst err / bound {ratio:.3f}"
    sent = torch.tensor(G.SENTINEL, dtype=buf.dtype)
    assert bool((buf[rows:] == sent).all()), "guard rows written"
    assert bool((buf[:, N:] == sent).all()), "padding columns written"
    rm = G.row_map(case)
    if rm is not None and len(case.levels) > 1:  # the guard rows between the grouped levels
        gap = torch.ones(rows, dtype=torch.bool)
        gap[rm] = False
        assert bool((buf[:rows][gap] == sent).all()), "guard rows between levels written"
    assert res["same"], "two runs differ bitwise"


def test_all_routes_logged(child):
    """Every reachable (cfg code, c mode) pair was logged by some case."""
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    seen = set()
    for name in child:
        for rec in G.parse_log(child[name]["log"][0]):
            seen.add((int(rec["cfg"]), int(rec["c"])))
    assert seen == G.REACHABLE, (sorted(G.REACHABLE - seen), sorted(seen - G.REACHABLE))

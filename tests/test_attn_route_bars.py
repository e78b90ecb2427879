"""The bound of the attention route table (tests/attn_route_cases.py) can fail.

No GPU: for every case the fp64 reference rounded to the case's dtype passes
the comparator (so the chosen inputs keep the reference itself inside the
bound), and each planted kernel error that applies to the case is outside the
bound on at least one output:

  pv_last         the last key dropped from P V
  sum_last        the last key dropped from the softmax sum
  hot_boundary    a hot key at a stride boundary dropped from P V
  head_v          head h reading head h - 1's V
  unnorm_wave     weights left unnormalised by one wave's share of the sum
  mask_kept       a masked hot key treated as kept
  mask_row_shift  the mask row of query i - 1 used for query i (causal)
  dsum_partial    one 64-key (or one wave's) partial missing from sum P dP
  dq_last         the last key's term missing from dq
  dkv_last_query  the last query's term missing from dk / dv (Lq > 1)
  dq_scale_twice  scale applied once too often in dq

Which plants apply is decided from the table entry (A.plant_names), not by a
skip at run time: a problem without keys or without images computes nothing
and says so; every other problem has at least three. A planted error is made
in fp64 where a kernel would make it and the result rounded to the dtype.
"""
import pytest
import torch

import attn_route_cases as A


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """The fp64 references run on one thread: this module is collected before
    tests/test_dist_gloo.py, whose ranks are forked from the test process and
    run autograd there; a child forked after the parent has started torch's
    intra-op thread pool waits for threads it does not have."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _checked(case, res, ref, bnd):
    """{output: (inside the bound, worst err / bound)} of rounded results."""
    return {n: A.compare(res[n].to(case.dtype), ref[n], bnd[n]) for n in A.outputs_of(case)}


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_bound_rejects_planted_errors(name):
    top = A.BY_NAME[name]
    for case in A.subcases(top):
        kinds = A.plant_names(case)
        if case.Lk == 0 or case.B == 0:
            assert not kinds  # nothing computed: exact zeros (or untouched buffers) on the GPU side
        else:
            assert len(kinds) >= 3, (case.name, kinds)
        if case.B == 0:
            continue
        inp = A.inputs(case)
        ref = A.compute(case, inp)
        bnd = A.bound(case, inp, ref)
        for n, (ok, ratio) in _checked(case, ref, ref, bnd).items():
            assert ok and ratio < 1, f"{case.name}: the rounded reference misses its own bound on {n}: {ratio:.3f}"
        if case.Lk:
            # every row keeps a key, and the hot keys carry visible weight somewhere
            assert bool((ref["p"].sum(-1) - 1).abs().max() < 1e-12)
            assert float(ref["p"][..., A.hot_keys(case)].max()) > 0.02, case.name
        if A.masked_hot(case) is not None:
            assert bool((ref["p"][inp["mask"] > 0] == 0).all())
        for kind in kinds:
            got = _checked(case, A.compute(case, inp, kind), ref, bnd)
            assert not all(ok for ok, _ in got.values()), \
                f"{case.name}: planted {kind} ({A.PLANT_DOC[kind]}) passes the bound: {got}"


def _routes(case):
    """(op, kernel, dtype) of every attn line the case writes."""
    return {(r["op"], r["kernel"], r["dtype"]) for r in A.expected_log(case)}


def test_table_covers_the_routes():
    """Every (op, kernel, dtype) the launchers can log has a case; the triples
    nobody can reach are listed with the reason."""
    have = set().union(*[_routes(c) for c in A.CASES])
    assert have == A.REACHABLE, (sorted(A.REACHABLE - have), sorted(have - A.REACHABLE))
    assert not have & A.UNREACHABLE
    # the shapes each route's loops can go wrong at
    lks = lambda k, dt="bf16": {c.Lk for c in A.CASES if c.op == "attn" and c.fwd == k and c.dname == dt}  # noqa: E731
    assert {1, 9, 63, 65, 127} <= lks("q1_vec64")
    assert {1, 67, 257} <= {c.Lk for c in A.CASES if c.fwd == "q1_vec" and c.D == 32}
    assert {1, 67, 257} <= {c.Lk for c in A.CASES if c.fwd == "q1_vec" and c.D == 8}
    assert {1, 2, 67} <= lks("q1_scalar") and {1, 2, 67} <= lks("q1_scalar", "f32")
    assert {128, 130, 257, 1025, 4096} <= lks("q1_mw")
    small = {(2, 1), (32, 1), (13, 17), (17, 13), (31, 31), (32, 32)}
    for k, dt in (("small_mfma", "bf16"), ("small_vec", "bf16"), ("small_scalar", "bf16"), ("small_scalar", "f32")):
        assert small <= {(c.Lq, c.Lk) for c in A.CASES if c.fwd == k and c.dname == dt}, (k, dt)
    for dt in ("bf16", "f32"):
        gen = {(c.Lq, c.Lk, c.D) for c in A.CASES if c.fwd == "general" and c.dname == dt}
        assert {(33, 32, 64), (40, 40, 64), (3, 5, 72), (3, 0, 64)} <= gen, dt
    assert A.BY_NAME["general_q1_lk4097"].fwd == "general" and A.BY_NAME["general_32x33"].fwd == "general"
    # forward on a 16-B route, backward on the scalar one
    assert any(c.fwd in ("q1_vec64", "q1_mw", "small_mfma") and c.bwd.endswith("scalar") for c in A.CASES)
    assert any(c.H == 8 for c in A.CASES if c.op == "attn") and any(c.B == 1 for c in A.CASES if c.op == "attn")
    assert {c.mask for c in A.CASES if c.op == "attn"} == {"", "pad", "head", "causal"}
    dec = [c for c in A.CASES if c.op == "decode"]
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129} <= {c.Lk for c in dec}
    assert {(c.D, c.H) for c in dec} >= {(64, 3), (32, 8), (64, 8)} and all(c.B == 5 for c in dec)
    assert {c.src for c in dec} == {True, False} and any(c.row_div == 3 and not c.src for c in dec)
    assert any(c.pads[3] % 8 for c in dec if c.fwd == "dec_scalar")
    views = [tuple(v.lk for v in c.views) for c in A.CASES if c.op == "views"]
    assert (784, 196, 49, 9) in views and (130, 1, 0, 64) in views
    assert any(len(c.views) == 5 and any(v.b == 0 for v in c.views) for c in A.CASES)
    assert all(len({v.pads for v in c.views}) > 1 for c in A.CASES if c.op == "views" and not c.status)


def test_every_plant_reaches_every_route_it_can_touch():
    """Per logged route, the plants that some case of the route carries."""
    seen = {}
    for c in A.CASES:
        for s in A.subcases(c):
            if s.B == 0 or c.status:
                continue
            kinds = set(A.plant_names(s))
            fwd, bwd = kinds & set(A.FWD_PLANTS), kinds & set(A.BWD_PLANTS)
            if c.op == "decode":
                seen.setdefault(("decode", c.fwd, c.dname), set()).update(fwd)
            elif c.op == "attn":
                seen.setdefault(("fwd", c.fwd, c.dname), set()).update(fwd)
                seen.setdefault(("bwd", c.bwd, c.dname), set()).update(bwd)
            else:
                seen.setdefault(("views_fwd", c.fwd, c.dname), set()).update(fwd)
                seen.setdefault(("views_bwd", c.bwd, c.dname), set()).update(bwd)
    one_query = {"pv_last", "sum_last", "hot_boundary", "head_v", "unnorm_wave"}
    bwd_q1 = {"dsum_partial", "dq_last", "dq_scale_twice"}
    for (op, kernel, dt), kinds in seen.items():
        if kernel == "zero_fill":
            assert not kinds
        elif op == "decode" or op == "views_fwd":  # no mask operand
            assert kinds == one_query, (op, kernel, dt, kinds)
        elif op == "views_bwd":
            assert kinds == bwd_q1, (op, kernel, dt, kinds)
        elif op == "fwd" and kernel.startswith("q1"):  # one query: no mask row to shift
            assert kinds == one_query | {"mask_kept"}, (op, kernel, dt, kinds)
        elif op == "fwd":
            assert kinds == set(A.FWD_PLANTS), (op, kernel, dt, kinds)
        elif kernel.startswith("q1"):
            assert kinds == bwd_q1, (op, kernel, dt, kinds)
        else:
            assert kinds == set(A.BWD_PLANTS), (op, kernel, dt, kinds)


def test_log_line_parser():
    lines = ["attn op=fwd kernel=general dtype=bf16 b=2 h=3 lq=33 lk=32 d=64",
             "bf16 a=0 b=0 c=0 M=33 N=32 K=64 batch=6 acc=0 split=1 cfg=4",
             "attn op=views_bwd kernel=views_grouped dtype=bf16 b=2 h=3 lq=1 lk=784 d=64 n=4"]
    recs = A.parse_log(lines)
    assert [r["kernel"] for r in recs] == ["general", "views_grouped"] and recs[1]["n"] == "4"
    case = A.BY_NAME["general_33x32"]
    ok = [lines[0], lines[1], lines[0].replace("op=fwd", "op=bwd")]
    assert not A.route_errors(case, ok)
    assert A.route_errors(case, ok[:2])
    assert A.route_errors(case, [ln.replace("lk=32", "lk=33") for ln in ok])
    assert A.route_errors(A.BY_NAME["q1_vec64_fwd_scalar_bwd"],
                          ["attn op=fwd kernel=q1_vec64 dtype=bf16 b=2 h=3 lq=1 lk=65 d=64",
                           "attn op=bwd kernel=q1_vec64 dtype=bf16 b=2 h=3 lq=1 lk=65 d=64"])

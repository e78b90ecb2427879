"""The bound of the GEMM route table (tests/gemm_route_cases.py) can fail.

No GPU: for every case the fp64 reference rounded to the output type passes
the comparator (so the chosen inputs keep the reference itself inside the
bound), and each planted kernel error is rejected:

  k_chunk8    one 8-element K chunk dropped from one element of the last row
              (the ragged M tile)
  k_tile64    one 64-wide K-tile dropped from that element (what the wide
              weight-gradient bar of test_conv_fwd_bwd lets through)
  tap         one filter tap dropped for one border pixel (conv cases)
  row_swap    the last live row replaced by its neighbour
  n_tail      the last N-tail 8-column group zeroed
  last_split  the last (shorter) split's slab left out (split cases)

A planted error is applied to A @ B before the case's epilogue, as a kernel
would make it. Where a seed put a planted error under the bound (the dropped
terms cancel, or the element is masked), the case's seed was changed, never
the bound.
"""
import pytest
import torch

import gemm_route_cases as G


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_bound_rejects_planted_errors(name):
    case = G.BY_NAME[name]
    inp = G.inputs(case)
    lin, S = G.terms(case)
    ref, s_tot = G.reference(case, inp, lin, S)
    bnd = G.bound(case, ref, s_tot)
    assert ref.shape == (G.out_rows(case), case.dims[1])
    rm = G.row_map(case)
    live = slice(None) if rm is None else rm
    assert bool((s_tot[live] >= ref[live].abs() * (1 - 1e-12)).all())  # S bounds the sum it belongs to
    ok, ratio = G.compare(case, ref.to(case.out_dtype), ref, bnd)
    assert ok, f"the rounded reference misses its own bound: worst err / bound {ratio:.3f}"
    kinds = []
    for kind, planted in G.plants(case, inp, lin):
        v, _ = G.epilogue(case, inp, planted, S)
        ok, ratio = G.compare(case, G.to_output(case, v).to(case.out_dtype), ref, bnd)
        assert not ok, f"planted {kind} passes the bound (worst err / bound {ratio:.3f})"
        kinds.append(kind)
    want = {"k_chunk8", "row_swap", "n_tail"}
    if case.dims[2] >= 128:
        want.add("k_tile64")
    if case.conv:
        want.add("tap")
    if case.splits > 1:
        want.add("last_split")
    assert set(kinds) == want


def test_table_covers_the_routes():
    """Every log code the bf16 dispatch can write, every launch_pipe_cfg case a
    dispatch rule returns and every launch_pipe_wg tile form has a named case;
    the codes nobody can reach are listed with the reason."""
    have = {(c.cfg, c.cmode) for c in G.CASES}
    assert have == G.REACHABLE, (sorted(G.REACHABLE - have), sorted(have - G.REACHABLE))
    assert not {c for c, _ in have} & G.UNREACHABLE
    # launch_pipe_cfg: all but 4 (tools/fwd_bench.hip only); the two im2col
    # instantiation sets (A_IM2COL: conv, scatter and tall-row reroutes; A_ROW)
    base = {c.name: 160 if c.cmode == G.C_SCATTER else 170 if c.cfg >= 170 else 130 for c in G.CASES if c.cfg >= 130}
    im2col = {c.cfg - base[c.name] for c in G.CASES if c.cfg >= 130 and c.cfg != 150 and (c.conv or c.cfg >= 160)}
    row = {c.cfg - 130 for c in G.CASES if 130 <= c.cfg < 142 and not c.conv}
    assert im2col == {0, 1, 2, 6, 7, 8, 10, 11} and row == {3, 5, 8, 9}
    for amode in (G.A_COL, G.A_IM2COL_T):
        tiles = {c.tile for c in G.CASES if c.tile and (c.ta == 1) == (amode == G.A_COL)}
        own = {"128x128+4lw"} if amode == G.A_COL else {"128x128", "128x256+8lw"}
        assert tiles == {"128x64", "64x256", "256x128"} | own, (amode, tiles)
    assert {c.tile for c in G.CASES if c.tile} == set(G.WG_TILES)
    # the ordered reduces: wgrad_reduce_kernel<1 | 4 | 16> by launch_wgrad_reduce's rule
    groups = set()
    for c in G.CASES:
        if c.acc == 2 and (c.split or 1) > 1:
            M, N, _ = c.dims
            items = M * G.cdiv(N, 4)
            groups.add(1 if items >= 65536 else 16 if c.split >= 8 else 4 if c.split >= 4 else 1)
    assert groups == {1, 4, 16}
    # split cases whose K-tiles the split count does not divide, per split form
    ragged = {c.name for c in G.CASES if c.splits > 1 and c.dims[2] % c.ksplit}
    assert {"row_cfg9_psplit2", "im2col_cfg8_psplit8", "reg128x64k_split8", "small_split2", "wg_col_128x64",
            "wg_conv_128x128"} <= ragged


def test_log_line_parser_accepts_appended_fields():
    rec = G.parse_log(["bf16 a=3 b=1 c=0 M=1224 N=136 K=1125 batch=1 acc=2 split=5 cfg=110 tm=10 tn=2\n"])[0]
    assert (rec["cfg"], rec["tm"], rec["tn"]) == ("110", "10", "2")
    assert not G.route_errors(G.BY_NAME["wg_conv_128x128"],
                              ["bf16 a=3 b=1 c=0 M=1224 N=136 K=1125 batch=1 acc=2 split=5 cfg=110 tm=10 tn=2"])
    assert G.route_errors(G.BY_NAME["wg_conv_128x128"],
                          ["bf16 a=3 b=1 c=0 M=1224 N=136 K=1125 batch=1 acc=2 split=5 cfg=110 tm=5 tn=2"])
    assert G.route_errors(G.BY_NAME["row_cfg9"], ["bf16 a=0 b=0 c=0 M=257 N=264 K=256 batch=1 acc=0 split=0 cfg=135"])

"""The wide conv class's launch planner (csrc/wide_plan.h, exported as
fpnmt_plan_wide_levels): where a grouped head conv's level list is broken into
launches and the M step of each. Pure host arithmetic: no GPU, the CU count
is an argument (256: MI355X)."""
import ctypes as C

CUS = 256
# output rows per level P3..P7 at 224^2: 28^2, 14^2, 7^2, 3^2, 1 pixels per image
C2_B32 = [25088, 6272, 1568, 288, 32]
C4_B64 = [50176, 12544, 3136, 576, 64]


def plan(rows, n_out=256, k_red=2304, cus=CUS):
    from fpnmt import _lib as L
    n = len(rows)
    lv, ms, tiles = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), (C.c_longlong * max(n, 1))()
    nl = L.lib.fpnmt_plan_wide_levels(n, (C.c_longlong * max(n, 1))(*rows), n_out, k_red, cus, lv, ms, tiles)
    assert nl >= 0, L.lib.fpnmt_last_error()
    return [(lv[i], ms[i], tiles[i]) for i in range(nl)]


def cdiv(a, b):
    return -(-a // b)


def test_five_levels_batch32_one_launch_at_144():
    """P3..P7 of the batch-32 step: 262 tiles at 128 rows (one launch of 245 +
    a tail launch before), 233 at 144: one launch, one wave of blocks."""
    assert sum(cdiv(r, 128) for r in C2_B32) == 262
    assert plan(C2_B32) == [(5, 144, 175 + 44 + 11 + 2 + 1)]
    assert plan(C2_B32)[0][2] == 233 <= CUS


def test_five_levels_batch64_one_launch():
    """C4's per-GPU batch: 521 tiles at 128 rows would need a third wave of
    blocks, 464 at 144 fit two."""
    assert sum(cdiv(r, 128) for r in C4_B64) == 521
    assert plan(C4_B64) == [(5, 144, 349 + 88 + 22 + 4 + 1)]
    assert plan(C4_B64)[0][2] == 464 <= 2 * CUS


def test_p3_only_keeps_the_112_row_step():
    """A single-level launch is never re-planned: P3 alone stays on 224 tiles
    of 112 rows (tile class 10, the kernel bench.py's roofline names)."""
    assert plan(C2_B32[:1]) == [(1, 112, 224)]
    assert plan(C4_B64[:1]) == [(1, 112, 448)]  # 392 at 128: two waves either way, 112 rows each


def test_two_levels_in_one_wave_keep_the_128_row_step():
    """P3 + P4 at batch 32 are 245 tiles of 128 rows, one wave of blocks (280 at
    112 rows would be two): no break, no taller tile."""
    assert plan(C2_B32[:2]) == [(2, 128, 196 + 49)]


def test_short_reduction_keeps_the_tail_break():
    """K < 1024 never reaches the wide class, so the 144-row step is not
    available: the earlier break after P4 stays."""
    got = plan(C2_B32, k_red=576)
    assert [g[0] for g in got] == [2, 3]
    assert got[0][1:] == (128, 245)


def test_every_level_lands_in_exactly_one_launch():
    for rows in (C2_B32, C4_B64, C2_B32[:3], C2_B32[1:], [r * 4 for r in C2_B32], [100] * 6, [33000, 200, 33000, 200]):
        for k_red in (576, 2304):
            got = plan(rows, k_red=k_red)
            assert sum(g[0] for g in got) == len(rows)
            i = 0
            for lv, ms, tiles in got:
                assert lv >= 1 and ms in (112, 128, 144)
                assert tiles == sum(cdiv(r, ms) for r in rows[i:i + lv])
                i += lv


def test_144_only_across_a_break():
    """A launch the 128-row rule does not break keeps its class, even where
    144-row tiles would save a wave of blocks (330 tiles -> 294: two either
    way; 280 -> 249 on one level: no break to merge across)."""
    for rows in ([330 * 128], [280 * 128], [165 * 128, 165 * 128]):
        got = plan(rows)
        assert len(got) == 1 and got[0][1] in (112, 128)
    # two launches below the wide class (140 tiles each) cost less than one wave of 144-row tiles
    assert [g[0] for g in plan([140 * 128, 140 * 128])] == [1, 1]


def test_arguments_are_checked():
    from fpnmt import _lib as L
    rows = (C.c_longlong * 7)(*([128] * 7))
    assert L.lib.fpnmt_plan_wide_levels(7, rows, 256, 2304, CUS, None, None, None) == L.E_ARG
    assert L.lib.fpnmt_plan_wide_levels(2, rows, 256, 2304, 0, None, None, None) == L.E_ARG
    assert L.lib.fpnmt_plan_wide_levels(2, None, 256, 2304, CUS, None, None, None) == L.E_ARG
    assert b"plan_wide_levels" in L.lib.fpnmt_last_error()
    assert L.lib.fpnmt_plan_wide_levels(2, rows, 256, 2304, CUS, None, None, None) == 1
    assert L.lib.fpnmt_plan_wide_levels(0, None, 256, 2304, CUS, None, None, None) == 0

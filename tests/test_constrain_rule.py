"""constrain_ref (tests/constrain_ref.py), the numpy statement of the rule of
fpnmt_logits_constrain, against answers worked out by hand, so that the
reference of the GPU tests does not rest on the kernel; and the binding's
constants and argument validation, which need no GPU."""
import numpy as np

from constrain_ref import banned_set, constrain_ref

S, A, B, C, END = 1, 5, 6, 7, 2
V = 12
NEG = np.float32(-np.inf)


def _row():
    """Distinct finite logits, positive at even columns and negative at odd ones."""
    return np.array([(j + 1) * (1.0 if j % 2 == 0 else -1.0) for j in range(V)], dtype=np.float32)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _banned(h, g, t=None, min_len=0, banned=()):
    t = len(h) - 1 if t is None else t
    return banned_set(h, t, V, g, min_len, END, banned)


def test_bigram_bans_the_continuation():
    # S a b a: the last token a opened "a b" before, so b is banned
    assert _banned([S, A, B, A], 2) == {B}


def test_bigram_overlapping_match_at_the_last_i():
    # S a a a: i = 2 is the last admissible start (h[2..3] = "a a"); it and i = 1 ban a
    assert _banned([S, A, A, A], 2) == {A}
    # only the last admissible i matches here: S b a a -> h[2] == h[3] = a, h[3] = a banned
    assert _banned([S, B, A, A], 2) == {A}


def test_trigram():
    # S a b c a b: "a b" was followed by c
    assert _banned([S, A, B, C, A, B], 3) == {C}
    assert _banned([S, A, B, C, B, A], 3) == set()


def test_unigram_bans_the_whole_history():
    assert _banned([S, A, B, A], 1) == {S, A, B}


def test_ngram_longer_than_the_history_bans_nothing():
    h = [A, A, A, A]
    t = 3
    assert _banned(h, t + 2) == set()  # no complete 5-gram in four tokens
    assert _banned(h, t + 40) == set()


def test_ngram_equal_to_the_history_length():
    # g = t + 1: one complete g-gram, i = 0; its first g - 1 tokens against the last g - 1
    assert _banned([S, A, A, A], 4) == set()  # S a a != a a a
    assert _banned([A, A, A, A], 4) == {A}  # a a a == a a a -> h[3] = a


def test_only_positions_up_to_t_count():
    h = [S, A, B, A, C, C, C]
    assert _banned(h, 2, t=3) == {B}


def test_out_of_range_ids_match_nothing():
    big = V + 1
    assert _banned([S, big, B, big], 2) == set()  # the prefix "big" equals itself only by value
    assert _banned([S, A, big, A], 2) == set()  # the continuation is no column
    assert _banned([S, A, -2, A], 1) == {S, A}
    assert _banned([S], 0, banned=[3, V, -1, 4]) == {3, 4}


def test_penalty_once_for_a_token_seen_three_times():
    row = _row()
    h = [S, 4, 4, 4]  # column 4 holds +5
    out = constrain_ref(row, h, 3, 0, 0, 2.0, 0, END, ())
    assert out[4] == np.float32(2.5)  # 5 / 2 once, not 5 / 8
    assert out[S] == np.float32(-4.0)  # column 1 holds -2: multiplied
    keep = [j for j in range(V) if j not in (4, S)]
    assert _bits(out[keep]) == _bits(row[keep])


def test_penalty_sign_rule_and_special_values():
    row = _row()
    row[3], row[4], row[5], row[6], row[7], row[8] = 3.0, -3.0, 0.0, -0.0, -np.inf, np.nan
    h = [3, 4, 5, 6, 7, 8]
    out = constrain_ref(row, h, 5, 0, 0, 1.5, 0, END, ())
    assert out[3] == np.float32(2.0) and out[4] == np.float32(-4.5)
    assert _bits(out[5:9]) == _bits(np.array([0.0, -0.0, -np.inf, np.nan], dtype=np.float32))
    # one IEEE fp32 divide, not a reciprocal multiply: 3 / 1.3 differs from 3 * (1 / 1.3) in fp32
    p = np.float32(1.3)
    out = constrain_ref(row, [3], 0, 0, 0, 1.3, 0, END, ())
    assert _bits(out[3]) == _bits(np.float32(3.0) / p)


def test_ban_beats_penalty():
    row = _row()
    h = [S, 4, B, 4]  # 4 is in the history (penalised) and listed (banned); +5 > 0
    out = constrain_ref(row, h, 3, 0, 2, 1.3, 0, END, (4,))
    assert out[4] == NEG and out[B] == NEG
    assert out[S] == np.float32(-2.0) * np.float32(1.3)


def test_min_len_boundary():
    row = _row()
    h = [S, A, B, C]
    for t, banned in ((2, True), (3, False)):  # min_len 3: t = min_len - 1 bans <end>, t = min_len does not
        out = constrain_ref(row, h, t, 0, 0, 1.0, 3, END, ())
        assert (out[END] == NEG) == banned
        keep = [j for j in range(V) if j != END]
        assert _bits(out[keep]) == _bits(row[keep])


def test_finished_row_is_untouched():
    row = _row()
    row[3] = np.nan
    out = constrain_ref(row, [S, A, B, A], 3, 1, 1, 1.3, 9, END, (0, 3))
    assert _bits(out) == _bits(row)


def test_binding_constants_and_validation_without_a_gpu():
    """The entry validates before any HIP call, and launches nothing with every rule off."""
    import re
    from fpnmt import _lib as L
    hdr = open(L.HEADER_PATH).read()
    assert int(re.search(r"#define FPNMT_CONSTRAIN_MAX_LEN\s+(\d+)", hdr).group(1)) == L.CONSTRAIN_MAX_LEN
    assert int(re.search(r"#define FPNMT_CONSTRAIN_MAX_BANNED\s+(\d+)", hdr).group(1)) == L.CONSTRAIN_MAX_BANNED
    f = L.lib.fpnmt_logits_constrain
    # (rows, vocab, logits, ldl, hist, hist_ld, t, fin, g, p, min_len, end, banned, n_banned, stream)
    assert f(4, 200, None, 200, 64, 8, 0, None, 2, 1.0, 0, 3, None, 0, None) == L.E_ARG
    assert b"null" in L.lib.fpnmt_last_error()
    assert f(4, 200, 64, 200, 64, 2000, 1024, None, 2, 1.0, 0, 3, None, 0, None) == L.E_UNSUPPORTED
    assert b"1024" in L.lib.fpnmt_last_error()
    assert f(4, 200, 64, 200, 64, 8, 3, None, 0, 1.0, 3, 3, None, 0, None) == 0  # min_len <= t: every rule off

"""The rule of fpnmt_logits_constrain (include/fpnmt.h) for one row, in numpy
fp32, element by element: the reference the kernel tests compare against
bitwise. Nothing here is clever on purpose; tests/test_constrain_rule.py pins
it with hand-written answers so it does not rest on the kernel."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def _in_range(tok, vocab):
    return 0 <= tok < vocab


def banned_set(h, t, vocab, g, min_len, end, banned):
    """The columns j in [0, vocab) whose final value is -inf."""
    out = set()
    if g > 0:
        for i in range(0, t - g + 2):  # i in [0, t - g + 1]: h[i .. i+g-1] is a complete g-gram
            same = True
            for k in range(g - 1):
                a, b = int(h[i + k]), int(h[t - g + 2 + k])
                # an id outside the vocabulary matches nothing, not even itself
                if not (_in_range(a, vocab) and _in_range(b, vocab) and a == b):
                    same = False
            j = int(h[i + g - 1])
            if same and _in_range(j, vocab):
                out.add(j)
    for b in banned:
        if _in_range(int(b), vocab):
            out.add(int(b))
    if t < min_len:
        out.add(int(end))
    return out


def constrain_ref(logits_row_f32, h, t, fin, g, p, min_len, end, banned):
    """logits_row_f32: the row's vocab logits (fp32); h: its history, h[0..t]
    used; fin: the row's finished flag. Returns the constrained row (a new
    fp32 array)."""
    row = np.array(logits_row_f32, dtype=np.float32, copy=True)
    if fin:
        return row
    vocab = row.shape[0]
    ban = banned_set(h, t, vocab, g, min_len, end, banned)
    seen = {int(h[i]) for i in range(t + 1) if _in_range(int(h[i]), vocab)}
    p32 = np.float32(p)
    for j in range(vocab):
        if j in ban:
            row[j] = NEG_INF
        elif p32 != np.float32(1.0) and j in seen:  # once, however often j occurs
            v = row[j]
            if np.isnan(v):
                continue  # a NaN keeps its bits
            with np.errstate(all="ignore"):
                row[j] = v / p32 if v > np.float32(0.0) else v * p32
    return row

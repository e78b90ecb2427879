"""fpnmt_xent_distill_fwd_bwd (include/fpnmt.h) restated in fp64, with the
error bounds the GPU tests hold the kernel to. No test lives here.

Per live row (0 < label < V), a = alpha, p = softmax(x), pT = softmax(x / T),
q = softmax(t / T):
  ce   = lse(x) - (1 - eps) x_lab - (eps / V) sum_j x_j
  kl   = sum_j q_j (log q_j - log pT_j); a column with q_j = 0 (a -inf teacher
         entry) adds exactly 0; a teacher row with a NaN or +inf, or -inf
         throughout, has no softmax: kl = NaN
  row  = (1 - a) ce + a T^2 kl
  grad = coef ((1 - a) (p - (1 - eps) onehot - eps / V) + a T (pT - q)),
         coef = dloss_scale / rows
  loss = (mean row, mean ce, mean kl) over ALL rows; a pad row adds zeros and
         has a zero gradient whatever its student and teacher rows hold.
The reference sees eps, alpha and T rounded to fp32, as the kernel does (eps
through the C ABI's float, alpha and T through the 16-byte device record).

Error bounds. u = 2^-24 (fp32 unit roundoff), V the row width, X = max |x| and
Z = max |t| over the finite entries of the case, first order in u as in
tests/test_gpu_xent_smooth_kernels.py, whose steps are reused for what the two
kernels share (B_lse, B_logp, B_ce, B_loss of the hard term: see there).
  dx = x_j - m, dt = t_j - mt: one rounding each on values <= 2X, 2Z.
  Exponents at temperature T: dx * fl(1 / T) carries dx's rounding, the
    reciprocal's and the product's: 3 u (2X / T) = 6 u X / T absolute (at
    T = 1: 2 u X, smaller). expf within 2 u relative.
  Sums over a row. The contract is one block of 256 threads per row: a
    thread adds at most n = 4 ceil(V / 1024) + 1 terms one after the other
    (whole 16-B vectors, or a scalar stride of 256, and one column of a
    ragged tail; a column past V adds an exact 0), then the 256 partial sums
    meet in a tree of 6 + 3 additions. No path holds more than D = n + 9
    additions: D u relative on positive terms, where a sum in an unknown
    order would carry V u.
    Rows wider than 10 240 columns are summed online: the running sum is
    rescaled by an exponential whenever the running maximum moves, at most n
    times, and once more against the block's maximum; each rescaling rounds
    an exponent of size Y (Y u), takes expf (2 u) and a product (u):
      resc(Y) = (n + 1) (Y + 3) u for V > 10 240, 0 otherwise.
    s0 = sum exp(dx)          -> E0 = (D + 2X + 2) u + resc(2X)       relative
    sT = sum exp(dx / T)      -> E1 = (D + 6X / T + 2) u + resc(6X / T)
    sq = sum exp(dt / T)      -> E2 = (D + 6Z / T + 2) u + resc(6Z / T)
  kl = (A / T) / sq + (log sT - log sq), A = sum_j eq_j w_j, eq_j =
    exp(dt_j / T), w_j = dt_j - dx_j (A is a plain sum at every width):
    eq_j: (6Z / T + 2) u relative; w_j: the two roundings and the
      subtraction's, 2 u relative to W_j = |dt_j| + |dx_j|; the product u;
      the sum D u   -> A within (D + 6Z / T + 5) u * sum_j eq_j W_j
    times fl(1 / T) 2 u; over sq: E2 and the division's u. With
      M = (1 / T) sum_j q_j W_j (computed per row below)
                    -> the first term within M ((2D + 12Z / T + 10) u + resc(6Z / T))
    log sT: E1 as an absolute error, logf 2 u log V; log sq likewise with E2
      (both sums lie in [1, V]); their difference u log V; the last
      addition u (M + log V)
      -> B_kl = u (M (2D + 12Z / T + 11) + 2D + 6 (X + Z) / T + 4 + 6 log V)
                + (M + 1) resc(6Z / T) + resc(6X / T)
  row = c1 ce + c3 kl, c1 = fl(1 - a) (u), c3 = fl(fl(a T) T) (2 u), the
    products u each, the sum u
      -> B_row = (1 - a) B_ce + a T^2 B_kl + u (3 (1 - a) |ce| + 4 a T^2 |kl|)
  loss[i] = (1 / rows) * ordered sum: rows u per term, as for the hard loss
      -> B_loss[i] = (1 / rows) sum_r (B_r + (rows + 2) u |value_r|)
  grad: p = exp(dx) * fl(1 / s0): the exponent 2 u X, expf 2 u, the
    reciprocal E0 + u, the product u -> (D + 4X + 6) u + resc(2X) on p <= 1;
    pT likewise (D + 12X / T + 6) u + resc(6X / T); q (D + 12Z / T + 6) u +
    resc(6Z / T) (a -inf entry: an exact 0).
    (p - a' [j = lab]) - b: a' = fl(1 - eps) u, b = fl(eps / V) <= u, two
      subtractions                                  -> (D + 4X + 10) u
    c1 * that: c1's rounding and the product's, on (1 - a) * (<= 1)
                                                    -> (1 - a) (D + 4X + 12) u
    pT - q: both errors and the subtraction's       -> (2D + 12 (X + Z) / T + 13) u
    c2 * that, c2 = fl(a T): rounding and product   -> a T (2D + 12 (X + Z) / T + 15) u
    the sum of the two (<= (1 - a) + a T): u; coef = dloss_scale / rows one
      rounding and the product's two: 3 u
      -> B_grad = |coef| (u ((1 - a) (D + 4X + 16) + a T (2D + 12 (X + Z) / T + 19))
                          + (1 - a) resc(2X) + a T (resc(6X / T) + resc(6Z / T)))
  A bf16 dlogits rounds that once more: 2^-8 relative (8 significant bits) on top.
No constant here is fitted to the kernel's output.
"""
import functools
import math

import torch

U = 2.0 ** -24
U_BF16 = 2.0 ** -8  # 8 significant bits, round to nearest
PLANTS = ("loss_aT", "grad_aT2", "kl_swapped", "kl_unmasked")


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def losses(x, t, lab, eps, alpha, T, plant=None):
    """(row, ce, kl, logp) per row in the dtype of x (fp64 for the reference;
    differentiable in x). eps, alpha, T are used as given."""
    rows, v = x.shape
    live = (lab > 0) & (lab < v)
    labc = torch.where(live, lab, torch.zeros_like(lab)).long()
    zero = torch.zeros((), dtype=x.dtype)
    xs = torch.where(live[:, None], x, zero)  # a pad row's contents are never looked at
    ts = torch.where(live[:, None], t.to(x.dtype), zero)
    lsm = torch.log_softmax(xs, 1)
    logp = lsm.gather(1, labc[:, None])[:, 0]
    ce = -(1 - eps) * logp - (eps / v) * lsm.sum(1)  # = lse - (1 - eps) x_lab - (eps / v) sum_j x_j
    lpt = torch.log_softmax(xs / T, 1)
    lq = torch.log_softmax(ts / T, 1)
    q = lq.exp()
    bad = ~torch.isfinite(q).all(1)
    if plant == "kl_swapped":
        pt = lpt.exp()
        kl = (pt * (lpt - torch.where(q > 0, lq, zero))).sum(1)
    else:
        kl = torch.where(q > 0, q * (torch.where(q > 0, lq, zero) - lpt), zero).sum(1)
    kl = torch.where(bad, torch.full_like(kl, float("nan")), kl)
    c3 = alpha * T if plant == "loss_aT" else alpha * T * T
    row = (1 - alpha) * ce + c3 * kl
    if plant == "kl_unmasked":
        # the pad rows' kl is kept: on the rows as given (a pad row with a finite teacher row)
        lq_u, lpt_u = torch.log_softmax(t.to(x.dtype) / T, 1), torch.log_softmax(x / T, 1)
        kl_u = (lq_u.exp() * (lq_u - lpt_u)).sum(1)
        kl = torch.where(live, kl, kl_u)
        row = torch.where(live, row, c3 * kl_u)
        return row, torch.where(live, ce, zero), kl, torch.where(live, logp, zero)
    return tuple(torch.where(live, a, zero) for a in (row, ce, kl, logp))


def reference(x, t, lab, eps, alpha, T, scale=1.0, plant=None):
    """x, t (rows, V) fp32 (t may hold -inf / NaN / +inf), lab (rows,) int.
    Returns fp64 values and the bounds of the module docstring."""
    rows, v = x.shape
    e, a, T = f32(eps), f32(alpha), f32(T)
    x64 = x.double()
    live = (lab > 0) & (lab < v)
    labc = torch.where(live, lab, torch.zeros_like(lab)).long()
    row, ce, kl, logp = losses(x64, t, lab, e, a, T, plant)
    loss = torch.stack([row.sum(), ce.sum(), kl.sum()]) / rows
    zero = torch.zeros((), dtype=torch.float64)
    xs = torch.where(live[:, None], x64, zero)
    ts = torch.where(live[:, None], t.double(), zero)
    p, pt, q = torch.softmax(xs, 1), torch.softmax(xs / T, 1), torch.softmax(ts / T, 1)
    onehot = torch.zeros(rows, v, dtype=torch.float64)
    onehot[torch.arange(rows), labc] = 1.0
    coef = live.double() * f32(scale) / rows
    c2 = a * T * T if plant == "grad_aT2" else a * T
    grad = ((1 - a) * (p - (1 - e) * onehot - e / v) + c2 * (pt - q)) * coef[:, None]
    grad = torch.where(live[:, None], grad, zero)
    # ---- bounds
    fin = torch.isfinite(ts)
    X = float(xs.abs().max())
    Z = float(torch.where(fin, ts.abs(), zero).max())
    lv = live.double()
    logv = math.log(v)
    gam = (v - 1) * U / (1 - (v - 1) * U)
    b_logp = U * (v + 5 * X + 4 * logv + 2)
    b_ce = U * (v + 10 * X + 5 * logv + 2) + (e / v) * (gam + 2 * U) * xs.abs().sum(1)
    n_t = 4 * math.ceil(v / 1024) + 1
    Dd = n_t + 9
    resc = (lambda y: (n_t + 1) * (y + 3) * U) if v > 10240 else (lambda y: 0.0)
    dx = xs.max(1, keepdim=True).values - xs
    tmax = torch.where(fin, ts, torch.full_like(ts, -1e300)).max(1, keepdim=True).values
    dt = torch.where(fin, tmax - ts, zero)
    qs = torch.where(torch.isfinite(q), q, zero)
    M = (qs * (dx + dt)).sum(1) / T
    b_kl = (U * (M * (2 * Dd + 12 * Z / T + 11) + 2 * Dd + 6 * (X + Z) / T + 4 + 6 * logv)
            + (M + 1) * resc(6 * Z / T) + resc(6 * X / T))
    ok = torch.isfinite(kl)
    kls, rws = torch.where(ok, kl, zero), torch.where(torch.isfinite(row), row, zero)
    b_row = (1 - a) * b_ce + a * T * T * b_kl + U * (3 * (1 - a) * ce.abs() + 4 * a * T * T * kls.abs())
    b_loss = torch.stack([(lv * (b_row + (rows + 2) * U * rws.abs())).sum(),
                          (lv * (b_ce + (rows + 2) * U * ce.abs())).sum(),
                          (lv * (b_kl + (rows + 2) * U * kls.abs())).sum()]) / rows
    b_grad = coef.abs() * (U * ((1 - a) * (Dd + 4 * X + 16) + a * T * (2 * Dd + 12 * (X + Z) / T + 19))
                           + (1 - a) * resc(2 * X) + a * T * (resc(6 * X / T) + resc(6 * Z / T)))
    return dict(loss=loss, row=row, ce=ce, kl=kl, logp=logp, grad=grad, live=live, coef=coef, b_loss=b_loss,
                b_logp=b_logp, b_grad=b_grad, b_kl=b_kl, eps=e, alpha=a, T=T)


# ------------------------------------------------------------------- cases
CASES = [(37, 37), (37, 40), (200, 208), (1001, 1001), (4100, 4100), (10000, 10000), (10300, 10304),
         (10243, 10243)]
# the teacher's row stride per student (V, ld): equal, padded otherwise, and
# rows whose 16-B alignment differs from the student's in both directions
LDT = {(37, 37): 40, (37, 40): 37, (200, 208): 208, (1001, 1001): 1004, (4100, 4100): 4101, (10000, 10000): 10000,
       (10300, 10304): 10304, (10243, 10243): 10244}
MIXES = [(0.5, 2.0), (0.5, 1.0), (1.0, 4.0), (0.0, 2.0)]
# (V, ld, eps, alpha, T): every width at eps = 0.1 under every mix; eps = 0 on two widths
PARAMS = [(v, ld, 0.1, a, t) for v, ld in CASES for a, t in MIXES] + \
         [(v, ld, 0.0, a, t) for v, ld in ((37, 40), (10000, 10000)) for a, t in MIXES[:2]]
ROWS = (1, 21)


@functools.lru_cache(maxsize=None)
def teacher(v, ld, rows):
    """A finite teacher (rows, V) fp32 for the student of
    test_gpu_xent_smooth_kernels.case(v, ld, rows, .): randn * 2 with +30 on
    the label's logit (on column 1 where the label is a pad), as a trained
    teacher's rows are: confident. That keeps KL(q || pT) and KL(pT || q)
    apart on every row, so a kernel that swaps them shows in the mean."""
    from test_gpu_xent_smooth_kernels import case as smooth_case
    lab = smooth_case(v, ld, rows, 0.1)["lab"]
    g = torch.Generator().manual_seed(77 * v + rows)
    t = torch.randn(rows, v, generator=g) * 2
    for r in range(rows):
        l = int(lab[r]) if 0 < int(lab[r]) < v else 1
        t[r, l] += 30.0
    return t


@functools.lru_cache(maxsize=None)
def case(v, ld, rows, eps, alpha, T, scale=1.0, plant=None):
    """Inputs (shared with the smooth-kernel tests: the same student buffer and
    labels) and the fp64 reference of one case, built once."""
    from test_gpu_xent_smooth_kernels import case as smooth_case
    c = smooth_case(v, ld, rows, eps)
    tea = teacher(v, ld, rows)
    ref = reference(c["buf"][:, :v], tea, c["lab"], eps, alpha, T, scale, plant)
    return dict(ref, buf=c["buf"], lab=c["lab"], tea=tea, smooth=c)

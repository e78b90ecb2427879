// Token-level knowledge distillation (not in the reference): the label-smoothed
// masked cross-entropy of xent.hip mixed with the KL divergence from a dense
// teacher row at temperature T, loss and gradient in one launch.
//
// fpnmt_xent_distill_fwd_bwd: block per row, 256 threads. With a = alpha,
// p = softmax(x), pT = softmax(x / T), q = softmax(t / T) per live row:
//   ce   = lse(x) - (1 - eps) x_lab - (eps / v) sum_j x_j
//   kl   = sum_j q_j (log q_j - log pT_j)
//        = (1 / (sq T)) sum_j eq_j ((t_j - mt) - (x_j - m)) + log sT - log sq
//          with m = max x, mt = max t, eq_j = exp((t_j - mt) / T), sq = sum eq,
//          sT = sum_j exp((x_j - m) / T); a column with eq_j = 0 (a -inf
//          teacher entry) is left out of the sum: 0, never 0 * inf
//   row  = (1 - a) ce + a T^2 kl
//   g_j  = ((1 - a) (p_j - (1 - eps) [j = lab] - eps / v) + a T (pT_j - q_j)) * dloss_scale / rows
// alpha and T come from a 16-byte record in device memory, read at execution
// (a captured step anneals either without recapture).
//
// Forms, as xent_smooth_kernel's: up to XD_REG_CAP columns both rows are read
// from memory once and held in registers, NV float4 each per thread (NV in
// {1, 4, 10}); the student's index map (16-B vectors or scalars) is the
// teacher's too, and a teacher row that is not 16-B aligned is fetched with
// scalar loads at the same columns. The first sweep leaves x_j - m (at T = 1:
// exp(x_j - m)) and eq_j in the registers, the second turns them into the
// gradient: five exponentials per column, two at T = 1 where pT = p. Wider
// rows take an online (max, sums) pass over both rows and a second read for
// the kl sum and the gradient.
//
// A pad row (label <= 0 or >= v) reads nothing: zeros everywhere. A teacher
// row with a NaN or +inf, or -inf throughout, gives a NaN kl (fmaxf skips a
// NaN, the exponential of that entry does not). The per-row row / ce / kl go
// to the workspace and each is summed by one block in row order.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int XD_REG_CAP = 10 * 4 * XS_THREADS;  // 10 240 columns

// the smoothed target: a on the label, b everywhere
struct XdTarget {
  float eps, a, b, coef;
};
// the mix, from the device record
struct XdMix {
  float c1, c2, c3, inv_t;  // 1 - alpha, alpha T, alpha T^2, 1 / T
  bool unit;                // T == 1: pT = p
};
__device__ __forceinline__ XdMix xd_mix(const fpnmt_distill_desc* __restrict__ d) {
  const float a = d->alpha, t = d->temperature;
  XdMix w;
  w.c1 = 1.f - a, w.c2 = a * t, w.c3 = (a * t) * t, w.inv_t = 1.f / t, w.unit = t == 1.f;
  return w;
}

struct XdRed {
  XsRed one;
  float f[4][4];
};
// four sums at once (wave order, then the four waves' in a fixed order)
__device__ __forceinline__ void xd_block_sum4(float (&s)[4], XdRed& red) {
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red.f[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = red.f[k][0] + red.f[k][1] + red.f[k][2] + red.f[k][3];
  __syncthreads();
}

template <typename T, bool VEC_ST>
__device__ __forceinline__ bool xd_pad_row(long long r, long long rows, int lab, int v, float* row_out,
                                           float* row_logp, T* dr) {
  if (lab > 0 && lab < v) return false;
  if (threadIdx.x == 0) {
    row_out[r] = 0.f, row_out[rows + r] = 0.f, row_out[2 * rows + r] = 0.f;
    if (row_logp) row_logp[r] = 0.f;
  }
  if (dr) xs_zero_row<T, VEC_ST>(dr, v);
  return true;
}

// thread 0: the row's three losses and its log-probability. s[] = {sum exp(x - m),
// sum exp((x - m) / T), sum eq, sum eq ((t - mt) - (x - m))}
__device__ __forceinline__ void xd_finish(long long r, long long rows, int lab, const XdTarget& q, const XdMix& w,
                                          float m, float sx, const float (&s)[4], const float* x, float* row_out,
                                          float* row_logp) {
  if (threadIdx.x == 0) {
    const float xl = x[lab], lse = m + logf(s[0]);
    // eps = 0: the plain -logp, whatever sum_j x_j is (0 * inf)
    const float ce = q.eps > 0.f ? (lse - q.a * xl) - q.b * sx : lse - xl;
    const float kl = (s[3] * w.inv_t) / s[2] + (logf(s[1]) - logf(s[2]));
    row_out[r] = w.c1 * ce + w.c3 * kl;
    row_out[rows + r] = ce;
    row_out[2 * rows + r] = kl;
    if (row_logp) row_logp[r] = xl - lse;
  }
}

// register-resident rows: NV float4 (VEC) or 4 * NV scalars per thread, twice.
// NV = 10: 80 registers of rows; held to two waves per SIMD (256 VGPRs), where
// the compiler keeps everything in registers (at 128 it spills to scratch).
// The second launch-bounds argument is the minimum number of waves per SIMD;
// 1 for the narrow forms is the default and constrains nothing
template <typename T, int NV, bool VEC, bool VEC_T, bool VEC_ST>
__global__ __launch_bounds__(XS_THREADS, NV == 10 ? 2 : 1) void xent_distill_kernel(
    int v, long long rows, const float* __restrict__ logits, long long ld, const float* __restrict__ teacher,
    long long ldt, const int32_t* __restrict__ labels, const fpnmt_distill_desc* __restrict__ desc, XdTarget q,
    float* __restrict__ row_out, float* __restrict__ row_logp, T* __restrict__ dlog, long long ldd) {
  __shared__ XdRed red;
  const long long r = blockIdx.x;
  const int lab = labels[r];
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (xd_pad_row<T, VEC_ST>(r, rows, lab, v, row_out, row_logp, dr)) return;
  const XdMix w = xd_mix(desc);
  const float* x = logits + r * ld;
  const float* tr = teacher + r * ldt;
  const int t = threadIdx.x;
  float e[4 * NV], u[4 * NV];
  // element index of register i (ascending in i for every thread), of both rows
  auto col = [&](int i) { return VEC ? ((i >> 2) * XS_THREADS + t) * 4 + (i & 3) : i * XS_THREADS + t; };
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c0 = col(4 * k);
    const bool whole = VEC && c0 + 4 <= v;
    if (whole) {
      const float4 f = *reinterpret_cast<const float4*>(x + c0);
      e[4 * k] = f.x, e[4 * k + 1] = f.y, e[4 * k + 2] = f.z, e[4 * k + 3] = f.w;
    }
    if (whole && VEC_T) {
      const float4 f = *reinterpret_cast<const float4*>(tr + c0);
      u[4 * k] = f.x, u[4 * k + 1] = f.y, u[4 * k + 2] = f.z, u[4 * k + 3] = f.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = col(4 * k + c);
      if (!whole) e[4 * k + c] = j < v ? x[j] : -INFINITY;
      if (!(whole && VEC_T)) u[4 * k + c] = j < v ? tr[j] : -INFINITY;
    }
  }
  float m = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4 * NV; ++i) m = fmaxf(m, e[i]), mt = fmaxf(mt, u[i]);
  m = xs_block_max(m, red.one);
  mt = xs_block_max(mt, red.one);
  float sx = 0.f;
  if (q.eps > 0.f) {
#pragma unroll
    for (int i = 0; i < 4 * NV; ++i) sx += col(i) < v ? e[i] : 0.f;
    sx = xs_block_sum(sx, red.one);
  }
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (w.unit) {
#pragma unroll
    for (int i = 0; i < 4 * NV; ++i) {
      const float dx = e[i] - m, dt = u[i] - mt;
      const float eq = expf(dt);  // a column past v: exp(-inf) = 0
      if (eq > 0.f) s[3] += eq * (dt - dx);
      s[2] += eq;
      u[i] = eq;
      e[i] = expf(dx);
      s[0] += e[i];
      if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // one vector at a time: keeps the temporaries few
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * NV; ++i) {
      const float dx = e[i] - m, dt = u[i] - mt;
      const float eq = expf(dt * w.inv_t);
      if (eq > 0.f) s[3] += eq * (dt - dx);
      s[2] += eq;
      u[i] = eq;
      e[i] = dx;
      s[0] += expf(dx);
      s[1] += expf(dx * w.inv_t);
      if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  xd_block_sum4(s, red);
  if (w.unit) s[1] = s[0];
  xd_finish(r, rows, lab, q, w, m, sx, s, x, row_out, row_logp);
  if (!dr) return;
  if (q.coef == 0.f) {  // a zero scale: exact zeros, whatever the softmax
    xs_zero_row<T, VEC_ST>(dr, v);
    return;
  }
  const float r0 = 1.f / s[0], r1 = 1.f / s[1], r2 = 1.f / s[2];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = 4 * k + c;
      float p, pt;
      if (w.unit) {
        p = e[i] * r0, pt = p;
      } else {
        p = expf(e[i]) * r0, pt = expf(e[i] * w.inv_t) * r1;
      }
      float h = p;
      if (col(i) == lab) h -= q.a;
      g[c] = (w.c1 * (h - q.b) + w.c2 * (pt - u[i] * r2)) * q.coef;
    }
    const int c0 = col(4 * k);
    if (VEC && VEC_ST && c0 + 4 <= v) {
      xs_store4(dr + c0, g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = col(4 * k + c);
        if (j < v) dr[j] = from_f32<T>(g[c]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// rows wider than XD_REG_CAP: an online (max, sums) pass over both rows, then
// a second read for the kl sum and (with a gradient) the gradient. VEC: both
// rows start 16-B aligned.
template <typename T, bool VEC, bool VEC_ST>
__global__ __launch_bounds__(XS_THREADS) void xent_distill_stream_kernel(
    int v, long long rows, const float* __restrict__ logits, long long ld, const float* __restrict__ teacher,
    long long ldt, const int32_t* __restrict__ labels, const fpnmt_distill_desc* __restrict__ desc, XdTarget q,
    float* __restrict__ row_out, float* __restrict__ row_logp, T* __restrict__ dlog, long long ldd) {
  __shared__ XdRed red;
  const long long r = blockIdx.x;
  const int lab = labels[r];
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (xd_pad_row<T, VEC_ST>(r, rows, lab, v, row_out, row_logp, dr)) return;
  const XdMix w = xd_mix(desc);
  const float* x = logits + r * ld;
  const float* tr = teacher + r * ldt;
  const int nv = VEC ? v >> 2 : 0;  // whole float4s; the rest as scalars
  float mx = -INFINITY, s0 = 0.f, s1 = 0.f, sxt = 0.f, mq = -INFINITY, sq = 0.f;
  auto take = [&](float a, float b) {
    sxt += a;
    if (a > mx) {
      const float d = mx - a;  // mx = -inf: the sums are 0 and stay finite
      s0 = s0 * expf(d) + 1.f;
      s1 = s1 * expf(d * w.inv_t) + 1.f;
      mx = a;
    } else if (mx > -INFINITY) {  // both -inf: the column weighs 0
      const float d = a - mx;
      s0 += expf(d);
      s1 += expf(d * w.inv_t);
    }
    if (b > mq) {
      sq = sq * expf((mq - b) * w.inv_t) + 1.f;
      mq = b;
    } else if (!(b == -INFINITY && mq == -INFINITY)) {  // a NaN poisons the sum, -inf on -inf weighs 0
      sq += expf((b - mq) * w.inv_t);
    }
  };
  for (int k = threadIdx.x; k < nv; k += XS_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    const float4 h = *reinterpret_cast<const float4*>(tr + 4 * k);
    take(f.x, h.x), take(f.y, h.y), take(f.z, h.z), take(f.w, h.w);
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XS_THREADS) take(x[j], tr[j]);
  const float m = xs_block_max(mx, red.one);
  const float mt = xs_block_max(mq, red.one);
  float s[4];
  s[0] = s0 > 0.f ? s0 * expf(mx - m) : 0.f;
  s[1] = s1 > 0.f ? s1 * expf((mx - m) * w.inv_t) : 0.f;
  s[2] = sq == 0.f ? 0.f : sq * expf((mq - mt) * w.inv_t);  // a NaN sum stays NaN
  s[3] = q.eps > 0.f ? sxt : 0.f;
  xd_block_sum4(s, red);
  const float sx = s[3];
  const bool store = dr && q.coef != 0.f;
  const float r0 = 1.f / s[0], r1 = 1.f / s[1], r2 = 1.f / s[2];
  float acc = 0.f;
  auto grad = [&](float a, float b, int j) {
    const float dx = a - m, dt = b - mt;
    const float eq = expf(dt * w.inv_t);
    if (eq > 0.f) acc += eq * (dt - dx);
    float p = expf(dx) * r0;
    const float pt = w.unit ? p : expf(dx * w.inv_t) * r1;
    if (j == lab) p -= q.a;
    return (w.c1 * (p - q.b) + w.c2 * (pt - eq * r2)) * q.coef;
  };
  for (int k = threadIdx.x; k < nv; k += XS_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    const float4 h = *reinterpret_cast<const float4*>(tr + 4 * k);
    const int j = 4 * k;
    const float g0 = grad(f.x, h.x, j), g1 = grad(f.y, h.y, j + 1), g2 = grad(f.z, h.z, j + 2),
                g3 = grad(f.w, h.w, j + 3);
    if (!store) continue;
    if (VEC_ST) {
      xs_store4(dr + j, g0, g1, g2, g3);
    } else {
      dr[j] = from_f32<T>(g0), dr[j + 1] = from_f32<T>(g1);
      dr[j + 2] = from_f32<T>(g2), dr[j + 3] = from_f32<T>(g3);
    }
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XS_THREADS) {
    const float g = grad(x[j], tr[j], j);
    if (store) dr[j] = from_f32<T>(g);
  }
  s[3] = xs_block_sum(acc, red.one);
  xd_finish(r, rows, lab, q, w, m, sx, s, x, row_out, row_logp);
  if (dr && !store) xs_zero_row<T, VEC_ST>(dr, v);
}

// loss[b] = scale * sum_r part[b * n + r], block b of three, fixed order
__global__ __launch_bounds__(256) void xd_ordered_sum3_kernel(long long n, const float* __restrict__ part, float scale,
                                                              float* __restrict__ out) {
  __shared__ float red[4];
  const float* p = part + (long long)blockIdx.x * n;
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) s += p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

struct XdCall {
  long long rows;
  int v;
  const float* logits;
  long long ld;
  const float* teacher;
  long long ldt;
  const int32_t* labels;
  const fpnmt_distill_desc* desc;
  XdTarget q;
  float* row_out;
  float* row_logp;
  long long ldd;
  hipStream_t s;
};

template <typename T, bool VEC, bool VEC_T, bool VEC_ST>
void xd_launch(const XdCall& c, T* dlog) {
  const dim3 grid((unsigned)c.rows), block(XS_THREADS);
#define XD_GO(K)                                                                                               \
  hipLaunchKernelGGL(K, grid, block, 0, c.s, c.v, c.rows, c.logits, c.ld, c.teacher, c.ldt, c.labels, c.desc, \
                     c.q, c.row_out, c.row_logp, dlog, c.ldd)
  if (c.v <= 1 * 4 * XS_THREADS) XD_GO((xent_distill_kernel<T, 1, VEC, VEC_T, VEC_ST>));
  else if (c.v <= 4 * 4 * XS_THREADS) XD_GO((xent_distill_kernel<T, 4, VEC, VEC_T, VEC_ST>));
  else if (c.v <= XD_REG_CAP) XD_GO((xent_distill_kernel<T, 10, VEC, VEC_T, VEC_ST>));
  else XD_GO((xent_distill_stream_kernel<T, VEC && VEC_T, VEC && VEC_T && VEC_ST>));
#undef XD_GO
}

template <typename T>
void xd_dispatch(const XdCall& c, T* dlog) {
  // every row start 16-B aligned (logits, teacher) / aligned for a 4-element store (dlogits)
  const bool vec = ((uintptr_t)c.logits & 15) == 0 && (c.rows == 1 || (c.ld & 3) == 0);
  const bool vet = ((uintptr_t)c.teacher & 15) == 0 && (c.rows == 1 || (c.ldt & 3) == 0);
  const bool vst = dlog && ((uintptr_t)dlog & (4 * sizeof(T) - 1)) == 0 && (c.rows == 1 || (c.ldd & 3) == 0);
  if (vec && vet && vst) xd_launch<T, true, true, true>(c, dlog);
  else if (vec && vet) xd_launch<T, true, true, false>(c, dlog);
  else if (vec && vst) xd_launch<T, true, false, true>(c, dlog);
  else if (vec) xd_launch<T, true, false, false>(c, dlog);
  else xd_launch<T, false, false, false>(c, dlog);
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_xent_distill_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                               const float* teacher, long long ldt, const int32_t* labels, float eps,
                               const fpnmt_distill_desc* desc, float* loss, float* row_logp, void* dlogits,
                               long long ldd, float dloss_scale, fpnmt_stream_t stream) {
  if (!loss || !logits || !teacher || !labels || !desc) return fail(FPNMT_E_ARG, "xent_distill: null pointer");
  if (!(eps >= 0.f && eps < 1.f)) return fail(FPNMT_E_ARG, "xent_distill: eps outside [0, 1)");
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32) return fail(FPNMT_E_ARG, "xent_distill: bad dtype");
  if (rows < 0 || rows > 0x7fffffffll || v < 1 || ld < v || ldt < v || (dlogits && ldd < v))
    return fail(FPNMT_E_ARG, "xent_distill: rows outside [0, 2^31) / v < 1 / ld < v / ldt < v / ldd < v");
  if (rows == 0) return zero_fill(loss, 3 * sizeof(float), S(stream));
  float* row_out = scratch_f32(3 * rows);
  if (!row_out) return fail(FPNMT_E_ARG, "xent_distill: needs the fpnmt workspace");
  XdCall c;
  c.rows = rows, c.v = v, c.logits = logits, c.ld = ld, c.teacher = teacher, c.ldt = ldt, c.labels = labels;
  c.desc = desc, c.row_out = row_out, c.row_logp = row_logp, c.ldd = ldd, c.s = S(stream);
  c.q.eps = eps, c.q.a = 1.f - eps, c.q.b = eps / (float)v, c.q.coef = dloss_scale / (float)rows;
  if (dtype == FPNMT_BF16) xd_dispatch<bf16>(c, (bf16*)dlogits);
  else xd_dispatch<float>(c, (float*)dlogits);
  // means over ALL rows, each summed in row order by one block
  hipLaunchKernelGGL(xd_ordered_sum3_kernel, dim3(3), dim3(256), 0, S(stream), rows, (const float*)row_out,
                     1.f / (float)rows, loss);
  return check_launch("xent_distill");
}

}  // extern "C"

// Label-smoothed cross-entropy and the held-out statistics of a caption batch
// (not in the reference).
//
// fpnmt_xent_smooth_fwd_bwd: masked sparse CE against the smoothed target
// (1 - eps) * onehot + eps / v, forward and (optional) gradient in one launch,
// block per row, the row read ONCE. The forms are fpnmt_xent_weighted_fwd_bwd's
// (scst.hip): a register-resident row of NV float4 per thread (NV in {1, 4,
// 10}; 16-B or scalar index map) up to XS_REG_CAP columns, a streaming form
// above. Beside the max and the exp sum the row gives two more block
// reductions while its logits still sit in the registers: sum_j x_j (the
// smoothing term) and the lowest column that holds the row maximum (row_hit:
// the label is the arg-max, ties to the lowest index; float comparisons only,
// so it carries no rounding). expf then overwrites the logits in place.
// Per live row, lse = m + log s:
//   ce   = lse - (1 - eps) x_lab - (eps / v) sum_j x_j
//   logp = x_lab - lse                                   (unsmoothed)
//   g_j  = (e_j / s - (1 - eps) [j = lab] - eps / v) * dloss_scale / rows
// A pad row (label <= 0 or >= v) reads nothing: zeros everywhere.
//
// The per-row ce go to the workspace and are summed by one block in row order,
// so the loss is bitwise repeatable.
//
// fpnmt_caption_stats: per caption the fp64 sum of its live rows' logp, its
// length and its hits; the three totals in caption order by one block, either
// written or added to what is there (a validation loop's running sums).
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

// XS_THREADS, XsRed, xs_block_max / _sum / _min, xs_store4, xs_zero_row: common.h
constexpr int XS_REG_CAP = 10 * 4 * XS_THREADS;  // 10 240 columns
constexpr int XS_NONE = 0x7fffffff;

// the smoothed target: a on the label, b everywhere
struct XsTarget {
  float eps, a, b, coef;
};

template <typename T, bool VEC_ST>
__device__ __forceinline__ bool xs_pad_row(long long r, int lab, int v, float* row_loss, float* row_logp,
                                           int32_t* row_hit, T* dr) {
  if (lab > 0 && lab < v) return false;
  if (threadIdx.x == 0) {
    row_loss[r] = 0.f;
    if (row_logp) row_logp[r] = 0.f;
    if (row_hit) row_hit[r] = 0;
  }
  if (dr) xs_zero_row<T, VEC_ST>(dr, v);
  return true;
}

__device__ __forceinline__ void xs_finish(long long r, int lab, const XsTarget& q, float m, float s, float sx,
                                          int first, const float* x, float* row_loss, float* row_logp,
                                          int32_t* row_hit) {
  if (threadIdx.x == 0) {
    const float xl = x[lab], lse = m + logf(s);
    // eps = 0: the plain -logp, whatever sum_j x_j is (0 * inf)
    row_loss[r] = q.eps > 0.f ? (lse - q.a * xl) - q.b * sx : lse - xl;
    if (row_logp) row_logp[r] = xl - lse;
    if (row_hit) row_hit[r] = first == lab ? 1 : 0;
  }
}

// register-resident row: NV float4 (VEC) or 4 * NV scalars per thread
template <typename T, int NV, bool VEC, bool VEC_ST>
__global__ __launch_bounds__(XS_THREADS) void xent_smooth_kernel(int v, const float* __restrict__ logits,
                                                                 long long ld, const int32_t* __restrict__ labels,
                                                                 XsTarget q, float* __restrict__ row_loss,
                                                                 float* __restrict__ row_logp,
                                                                 int32_t* __restrict__ row_hit,
                                                                 T* __restrict__ dlog, long long ldd) {
  __shared__ XsRed red;
  const long long r = blockIdx.x;
  const int lab = labels[r];
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (xs_pad_row<T, VEC_ST>(r, lab, v, row_loss, row_logp, row_hit, dr)) return;
  const float* x = logits + r * ld;
  const int t = threadIdx.x;
  float e[4 * NV];
  // element index of register i (ascending in i for every thread)
  auto col = [&](int i) { return VEC ? ((i >> 2) * XS_THREADS + t) * 4 + (i & 3) : i * XS_THREADS + t; };
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c0 = col(4 * k);
    if (VEC && c0 + 4 <= v) {
      const float4 f = *reinterpret_cast<const float4*>(x + c0);
      e[4 * k] = f.x, e[4 * k + 1] = f.y, e[4 * k + 2] = f.z, e[4 * k + 3] = f.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = col(4 * k + c);
        e[4 * k + c] = j < v ? x[j] : -INFINITY;
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4 * NV; ++i) m = fmaxf(m, e[i]);
  m = xs_block_max(m, red);
  float sx = 0.f;
  if (q.eps > 0.f) {
#pragma unroll
    for (int i = 0; i < 4 * NV; ++i) sx += col(i) < v ? e[i] : 0.f;
    sx = xs_block_sum(sx, red);
  }
  int first = XS_NONE;
  if (row_hit) {  // the lowest column equal to the row maximum
#pragma unroll
    for (int i = 4 * NV - 1; i >= 0; --i)
      if (e[i] == m && col(i) < v) first = col(i);
    first = xs_block_min(first, red);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4 * NV; ++i) {
    e[i] = expf(e[i] - m);  // a column past v: exp(-inf) = 0
    s += e[i];
  }
  s = xs_block_sum(s, red);
  xs_finish(r, lab, q, m, s, sx, first, x, row_loss, row_logp, row_hit);
  if (!dr) return;
  if (q.coef == 0.f) {  // a zero scale: exact zeros, whatever the softmax
    xs_zero_row<T, VEC_ST>(dr, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float p = e[4 * k + c] / s;
      if (col(4 * k + c) == lab) p -= q.a;
      g[c] = (p - q.b) * q.coef;
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
  }
}

// rows wider than XS_REG_CAP: an online (max, sum) pass that also carries
// sum_j x_j and the first column of the thread's maximum, then (with a
// gradient) a second read
template <typename T, bool VEC, bool VEC_ST>
__global__ __launch_bounds__(XS_THREADS) void xent_smooth_stream_kernel(int v, const float* __restrict__ logits,
                                                                        long long ld,
                                                                        const int32_t* __restrict__ labels,
                                                                        XsTarget q, float* __restrict__ row_loss,
                                                                        float* __restrict__ row_logp,
                                                                        int32_t* __restrict__ row_hit,
                                                                        T* __restrict__ dlog, long long ldd) {
  __shared__ XsRed red;
  const long long r = blockIdx.x;
  const int lab = labels[r];
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (xs_pad_row<T, VEC_ST>(r, lab, v, row_loss, row_logp, row_hit, dr)) return;
  const float* x = logits + r * ld;
  const int nv = VEC ? v >> 2 : 0;  // whole float4s; the rest as scalars
  float mt = -INFINITY, st = 0.f, sxt = 0.f;
  int it = XS_NONE;  // the columns come in ascending order: a strict > keeps the first
  auto take = [&](float a, int j) {
    sxt += a;
    if (a > mt) {
      st = st * expf(mt - a) + 1.f;  // mt = -inf: st is 0 and stays finite
      mt = a;
      it = j;
    } else if (mt > -INFINITY) {  // both -inf: the column weighs 0
      st += expf(a - mt);
    }
  };
  for (int k = threadIdx.x; k < nv; k += XS_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    take(f.x, 4 * k), take(f.y, 4 * k + 1), take(f.z, 4 * k + 2), take(f.w, 4 * k + 3);
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XS_THREADS) take(x[j], j);
  const float m = xs_block_max(mt, red);
  const float s = xs_block_sum(st > 0.f ? st * expf(mt - m) : 0.f, red);
  const float sx = q.eps > 0.f ? xs_block_sum(sxt, red) : 0.f;
  const int first = row_hit ? xs_block_min(mt == m ? it : XS_NONE, red) : XS_NONE;
  xs_finish(r, lab, q, m, s, sx, first, x, row_loss, row_logp, row_hit);
  if (!dr) return;
  if (q.coef == 0.f) {
    xs_zero_row<T, VEC_ST>(dr, v);
    return;
  }
  auto grad = [&](float a, int j) {
    float p = expf(a - m) / s;
    if (j == lab) p -= q.a;
    return (p - q.b) * q.coef;
  };
  for (int k = threadIdx.x; k < nv; k += XS_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    const int j = 4 * k;
    if (VEC_ST) {
      xs_store4(dr + j, grad(f.x, j), grad(f.y, j + 1), grad(f.z, j + 2), grad(f.w, j + 3));
    } else {
      dr[j] = from_f32<T>(grad(f.x, j)), dr[j + 1] = from_f32<T>(grad(f.y, j + 1));
      dr[j + 2] = from_f32<T>(grad(f.z, j + 2)), dr[j + 3] = from_f32<T>(grad(f.w, j + 3));
    }
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XS_THREADS) dr[j] = from_f32<T>(grad(x[j], j));
}

// loss = scale * sum_r v[r], one block, fixed order
__global__ __launch_bounds__(256) void xs_ordered_sum_kernel(long long n, const float* __restrict__ v, float scale,
                                                             float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) s += v[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

template <typename T, bool VEC, bool VEC_ST>
void xs_launch(long long rows, int v, const float* logits, long long ld, const int32_t* labels, const XsTarget& q,
               float* row_loss, float* row_logp, int32_t* row_hit, T* dlog, long long ldd, hipStream_t s) {
  const dim3 grid((unsigned)rows), block(XS_THREADS);
#define XS_GO(K) hipLaunchKernelGGL(K, grid, block, 0, s, v, logits, ld, labels, q, row_loss, row_logp, row_hit, dlog, ldd)
  if (v <= 1 * 4 * XS_THREADS) XS_GO((xent_smooth_kernel<T, 1, VEC, VEC_ST>));
  else if (v <= 4 * 4 * XS_THREADS) XS_GO((xent_smooth_kernel<T, 4, VEC, VEC_ST>));
  else if (v <= XS_REG_CAP) XS_GO((xent_smooth_kernel<T, 10, VEC, VEC_ST>));
  else XS_GO((xent_smooth_stream_kernel<T, VEC, VEC_ST>));
#undef XS_GO
}

template <typename T>
void xs_dispatch(long long rows, int v, const float* logits, long long ld, const int32_t* labels, const XsTarget& q,
                 float* row_loss, float* row_logp, int32_t* row_hit, T* dlog, long long ldd, hipStream_t s) {
  // every row start 16-B aligned (logits) / aligned for a 4-element store (dlogits)
  const bool vec = ((uintptr_t)logits & 15) == 0 && (rows == 1 || (ld & 3) == 0);
  const bool vst = dlog && ((uintptr_t)dlog & (4 * sizeof(T) - 1)) == 0 && (rows == 1 || (ldd & 3) == 0);
#define XS_D(A, B) xs_launch<T, A, B>(rows, v, logits, ld, labels, q, row_loss, row_logp, row_hit, dlog, ldd, s)
  if (vec && vst) XS_D(true, true);
  else if (vec) XS_D(true, false);
  else XS_D(false, false);
#undef XS_D
}

// one block: 256 captions at a time, one thread each (its live positions in
// ascending order, fp64), then thread 0 adds the 256 in caption order
__global__ __launch_bounds__(256) void caption_stats_kernel(long long captions, int t,
                                                            const int32_t* __restrict__ labels,
                                                            const float* __restrict__ row_logp,
                                                            const int32_t* __restrict__ row_hit,
                                                            float* __restrict__ cap_logp, int32_t* __restrict__ cap_len,
                                                            int32_t* __restrict__ cap_hit, double* __restrict__ totals,
                                                            int accumulate) {
  __shared__ double sl[256];
  __shared__ int sn[256], sh[256];
  double tl = 0.0, tn = 0.0, th = 0.0;
  for (long long base = 0; base < captions; base += 256) {
    const long long c = base + threadIdx.x;
    double lp = 0.0;
    int n = 0, h = 0;
    if (c < captions) {
      for (int p = 0; p < t; ++p) {
        const long long r = c * t + p;
        if (labels[r] > 0) {  // live: not a pad (a label >= v counts, with the 0s the loss kernel left)
          lp += (double)row_logp[r];
          n += 1;
          h += row_hit[r];
        }
      }
      if (cap_logp) cap_logp[c] = (float)lp;
      if (cap_len) cap_len[c] = n;
      if (cap_hit) cap_hit[c] = h;
    }
    sl[threadIdx.x] = lp, sn[threadIdx.x] = n, sh[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int lim = (int)min(256ll, captions - base);
      for (int i = 0; i < lim; ++i) tl += sl[i], tn += (double)sn[i], th += (double)sh[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[0] = (accumulate ? totals[0] : 0.0) + tl;
    totals[1] = (accumulate ? totals[1] : 0.0) + tn;
    totals[2] = (accumulate ? totals[2] : 0.0) + th;
  }
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_xent_smooth_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                              const int32_t* labels, float eps, float* loss, float* row_logp, int32_t* row_hit,
                              void* dlogits, long long ldd, float dloss_scale, fpnmt_stream_t stream) {
  if (!loss || !logits || !labels) return fail(FPNMT_E_ARG, "xent_smooth: null pointer");
  if (!(eps >= 0.f && eps < 1.f)) return fail(FPNMT_E_ARG, "xent_smooth: eps outside [0, 1)");
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32) return fail(FPNMT_E_ARG, "xent_smooth: bad dtype");
  if (rows < 0 || rows > 0x7fffffffll || v < 1 || ld < v || (dlogits && ldd < v))
    return fail(FPNMT_E_ARG, "xent_smooth: rows outside [0, 2^31) / v < 1 / ld < v / ldd < v");
  if (rows == 0) return zero_fill(loss, sizeof(float), S(stream));
  float* row_loss = scratch_f32(rows);
  if (!row_loss) return fail(FPNMT_E_ARG, "xent_smooth: needs the fpnmt workspace");
  XsTarget q;
  q.eps = eps, q.a = 1.f - eps, q.b = eps / (float)v, q.coef = dloss_scale / (float)rows;
  if (dtype == FPNMT_BF16)
    xs_dispatch<bf16>(rows, v, logits, ld, labels, q, row_loss, row_logp, row_hit, (bf16*)dlogits, ldd, S(stream));
  else
    xs_dispatch<float>(rows, v, logits, ld, labels, q, row_loss, row_logp, row_hit, (float*)dlogits, ldd, S(stream));
  // mean over ALL rows, summed in row order
  hipLaunchKernelGGL(xs_ordered_sum_kernel, dim3(1), dim3(256), 0, S(stream), rows, (const float*)row_loss,
                     1.f / (float)rows, loss);
  return check_launch("xent_smooth");
}

int fpnmt_caption_stats(long long captions, int t, const int32_t* labels, const float* row_logp,
                        const int32_t* row_hit, float* cap_logp, int32_t* cap_len, int32_t* cap_hit, double* totals,
                        int accumulate, fpnmt_stream_t stream) {
  if (!labels || !row_logp || !row_hit || !totals) return fail(FPNMT_E_ARG, "caption_stats: null pointer");
  if (captions < 0 || captions > 0x7fffffffll || t < 1 || captions * t > 0x7fffffffll)
    return fail(FPNMT_E_ARG, "caption_stats: captions outside [0, 2^31) / t < 1 / captions * t >= 2^31");
  hipLaunchKernelGGL(caption_stats_kernel, dim3(1), dim3(256), 0, S(stream), captions, t, labels, row_logp, row_hit,
                     cap_logp, cap_len, cap_hit, totals, accumulate);
  return check_launch("caption_stats");
}

}  // extern "C"

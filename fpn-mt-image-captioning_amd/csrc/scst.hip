// Self-critical caption training (not in the reference): the loss of a step
// whose caption rows are model samples weighted by their advantage, and the
// row repeat that lets n sampled captions share one encoder pass.
//
// fpnmt_xent_weighted_fwd_bwd: masked sparse CE times a per-caption weight,
// forward and gradient in one launch, block per row. Unlike xent_kernel
// (elementwise.hip: three scalar passes over the row, expf twice per element)
// the row is read ONCE: every thread keeps its share in registers across the
// max pass, the exp / sum pass (the exponentials replace the logits in place:
// one expf per element) and the store. Rows whose start is 16-B aligned move
// as float4 (thread t owns the vectors k * 256 + t), others as scalars (thread
// t owns the elements i * 256 + t): the same registers, another index map.
// Up to XW_REG_CAP columns stay register-resident (4 * NV floats per thread,
// NV in {1, 4, 10}: V = 10 000 is 10 float4 at 256 threads); wider rows take a
// streaming form, an online max / sum pass and a second read for the store.
// A pad row (label 0) reads nothing: its gradient row is a zero fill.
//
// The per-row terms w * ce go to the workspace and are summed by one block in
// row order (as fpnmt_xent_fwd_bwd does), so the loss is bitwise repeatable.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int XW_THREADS = 256;
constexpr int XW_REG_CAP = 10 * 4 * XW_THREADS;  // 10 240 columns

__device__ __forceinline__ float block_max(float m, float* red) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return m;
}
__device__ __forceinline__ float block_sum(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// four gradient elements as one 16-B (fp32) / 8-B (bf16) store
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void store4(bf16* p, float a, float b, float c, float d) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  bf16x4 o = {(bf16)a, (bf16)b, (bf16)c, (bf16)d};
  *reinterpret_cast<bf16x4*>(p) = o;
}

// what a row needs besides its logits; pad (also a label outside [0, v), which
// is never dereferenced) means: no loss, no gradient
struct XwRow {
  int lab;
  bool pad;
  float w, coef;
};
__device__ __forceinline__ XwRow xw_row(long long r, long long rows, int v, const int32_t* labels, const float* w,
                                        int w_div, float gscale) {
  XwRow q;
  q.lab = labels[r];
  q.pad = q.lab <= 0 || q.lab >= v;
  q.w = w[r / w_div];
  q.coef = gscale * q.w / (float)rows;
  return q;
}

template <typename T, bool VEC>
__device__ __forceinline__ void xw_zero_row(T* dr, int v) {
  if (VEC) {
    const int nv = v >> 2;
    for (int k = threadIdx.x; k < nv; k += XW_THREADS) store4(dr + 4 * k, 0.f, 0.f, 0.f, 0.f);
    for (int j = (nv << 2) + threadIdx.x; j < v; j += XW_THREADS) dr[j] = from_f32<T>(0.f);
  } else {
    for (int j = threadIdx.x; j < v; j += XW_THREADS) dr[j] = from_f32<T>(0.f);
  }
}

__device__ __forceinline__ void xw_finish(long long r, const XwRow& q, float m, float s, const float* x,
                                          float* row_loss, float* row_logp) {
  if (threadIdx.x == 0) {
    const float logp = x[q.lab] - (m + logf(s));
    row_loss[r] = q.w * -logp;
    if (row_logp) row_logp[r] = logp;
  }
}

// register-resident row: NV float4 (VEC) or 4 * NV scalars per thread
template <typename T, int NV, bool VEC, bool VEC_ST>
__global__ __launch_bounds__(XW_THREADS) void xent_weighted_kernel(long long rows, int v,
                                                                   const float* __restrict__ logits, long long ld,
                                                                   const int32_t* __restrict__ labels,
                                                                   const float* __restrict__ w, int w_div,
                                                                   float* __restrict__ row_loss,
                                                                   float* __restrict__ row_logp,
                                                                   T* __restrict__ dlog, long long ldd,
                                                                   float gscale) {
  __shared__ float red[4];
  const long long r = blockIdx.x;
  const XwRow q = xw_row(r, rows, v, labels, w, w_div, gscale);
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (q.pad) {
    if (threadIdx.x == 0) {
      row_loss[r] = 0.f;
      if (row_logp) row_logp[r] = 0.f;
    }
    if (dr) xw_zero_row<T, VEC_ST>(dr, v);
    return;
  }
  const float* x = logits + r * ld;
  const int t = threadIdx.x;
  float e[4 * NV];
  // element index of register i
  auto col = [&](int i) { return VEC ? ((i >> 2) * XW_THREADS + t) * 4 + (i & 3) : i * XW_THREADS + t; };
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
  m = block_max(m, red);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4 * NV; ++i) {
    e[i] = expf(e[i] - m);  // a column past v: exp(-inf) = 0
    s += e[i];
  }
  s = block_sum(s, red);
  xw_finish(r, q, m, s, x, row_loss, row_logp);
  if (!dr) return;
  if (q.coef == 0.f) {  // a zero weight: exact zeros, whatever the softmax
    xw_zero_row<T, VEC_ST>(dr, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float p = e[4 * k + c] / s;
      if (col(4 * k + c) == q.lab) p -= 1.f;
      g[c] = p * q.coef;
    }
    const int c0 = col(4 * k);
    if (VEC && VEC_ST && c0 + 4 <= v) {
      store4(dr + c0, g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = col(4 * k + c);
        if (j < v) dr[j] = from_f32<T>(g[c]);
      }
    }
  }
}

// rows wider than XW_REG_CAP: an online (max, sum) pass, then a second read
template <typename T, bool VEC, bool VEC_ST>
__global__ __launch_bounds__(XW_THREADS) void xent_weighted_stream_kernel(long long rows, int v,
                                                                          const float* __restrict__ logits,
                                                                          long long ld,
                                                                          const int32_t* __restrict__ labels,
                                                                          const float* __restrict__ w, int w_div,
                                                                          float* __restrict__ row_loss,
                                                                          float* __restrict__ row_logp,
                                                                          T* __restrict__ dlog, long long ldd,
                                                                          float gscale) {
  __shared__ float red[4];
  const long long r = blockIdx.x;
  const XwRow q = xw_row(r, rows, v, labels, w, w_div, gscale);
  T* dr = dlog ? dlog + r * ldd : nullptr;
  if (q.pad) {
    if (threadIdx.x == 0) {
      row_loss[r] = 0.f;
      if (row_logp) row_logp[r] = 0.f;
    }
    if (dr) xw_zero_row<T, VEC_ST>(dr, v);
    return;
  }
  const float* x = logits + r * ld;
  const int nv = VEC ? v >> 2 : 0;  // whole float4s; the rest as scalars
  float mt = -INFINITY, st = 0.f;
  auto take = [&](float a) {
    if (a > mt) {
      st = st * expf(mt - a) + 1.f;  // mt = -inf: st is 0 and stays finite
      mt = a;
    } else if (mt > -INFINITY) {  // both -inf: the column weighs 0
      st += expf(a - mt);
    }
  };
  for (int k = threadIdx.x; k < nv; k += XW_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    take(f.x), take(f.y), take(f.z), take(f.w);
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XW_THREADS) take(x[j]);
  const float m = block_max(mt, red);
  const float s = block_sum(st > 0.f ? st * expf(mt - m) : 0.f, red);
  xw_finish(r, q, m, s, x, row_loss, row_logp);
  if (!dr) return;
  if (q.coef == 0.f) {
    xw_zero_row<T, VEC_ST>(dr, v);
    return;
  }
  auto grad = [&](float a, int j) {
    float p = expf(a - m) / s;
    if (j == q.lab) p -= 1.f;
    return p * q.coef;
  };
  for (int k = threadIdx.x; k < nv; k += XW_THREADS) {
    const float4 f = *reinterpret_cast<const float4*>(x + 4 * k);
    const int j = 4 * k;
    if (VEC_ST) {
      store4(dr + j, grad(f.x, j), grad(f.y, j + 1), grad(f.z, j + 2), grad(f.w, j + 3));
    } else {
      dr[j] = from_f32<T>(grad(f.x, j)), dr[j + 1] = from_f32<T>(grad(f.y, j + 1));
      dr[j + 2] = from_f32<T>(grad(f.z, j + 2)), dr[j + 3] = from_f32<T>(grad(f.w, j + 3));
    }
  }
  for (int j = (nv << 2) + threadIdx.x; j < v; j += XW_THREADS) dr[j] = from_f32<T>(grad(x[j], j));
}

// loss = scale * sum_r v[r], one block, fixed order (ordered_sum_kernel's)
__global__ __launch_bounds__(256) void xw_ordered_sum_kernel(long long n, const float* __restrict__ v, float scale,
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
void xw_launch(long long rows, int v, const float* logits, long long ld, const int32_t* labels, const float* w,
               int w_div, float* row_loss, float* row_logp, T* dlog, long long ldd, float gscale, hipStream_t s) {
  const dim3 grid((unsigned)rows), block(XW_THREADS);
#define XW_GO(K) \
  hipLaunchKernelGGL(K, grid, block, 0, s, rows, v, logits, ld, labels, w, w_div, row_loss, row_logp, dlog, ldd, gscale)
  if (v <= 1 * 4 * XW_THREADS) XW_GO((xent_weighted_kernel<T, 1, VEC, VEC_ST>));
  else if (v <= 4 * 4 * XW_THREADS) XW_GO((xent_weighted_kernel<T, 4, VEC, VEC_ST>));
  else if (v <= XW_REG_CAP) XW_GO((xent_weighted_kernel<T, 10, VEC, VEC_ST>));
  else XW_GO((xent_weighted_stream_kernel<T, VEC, VEC_ST>));
#undef XW_GO
}

template <typename T>
void xw_dispatch(long long rows, int v, const float* logits, long long ld, const int32_t* labels, const float* w,
                 int w_div, float* row_loss, float* row_logp, T* dlog, long long ldd, float gscale, hipStream_t s) {
  // every row start 16-B aligned (logits) / aligned for a 4-element store (dlogits)
  const bool vec = ((uintptr_t)logits & 15) == 0 && (rows == 1 || (ld & 3) == 0);
  const bool vst = dlog && ((uintptr_t)dlog & (4 * sizeof(T) - 1)) == 0 && (rows == 1 || (ldd & 3) == 0);
#define XW_D(A, B) \
  xw_launch<T, A, B>(rows, v, logits, ld, labels, w, w_div, row_loss, row_logp, dlog, ldd, gscale, s)
  if (vec && vst) XW_D(true, true);
  else if (vec) XW_D(true, false);
  else XW_D(false, false);
#undef XW_D
}

// y[i * n + s] = x[i] for s < n, in units of U (16 B, or one element)
template <typename U>
__global__ __launch_bounds__(256) void repeat_rows_kernel(int n, long long units, const U* __restrict__ x,
                                                          U* __restrict__ y) {
  const long long i = blockIdx.y;
  const U* src = x + i * units;
  U* dst = y + i * n * units;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < units; e += (long long)gridDim.x * 256) {
    const U val = src[e];
    for (int s = 0; s < n; ++s) dst[s * units + e] = val;
  }
}

template <typename U>
void repeat_rows_launch(int b, int n, long long units, const void* x, void* y, hipStream_t s) {
  const unsigned gx = (unsigned)std::min<long long>((units + 255) / 256, 4096);
  hipLaunchKernelGGL(repeat_rows_kernel<U>, dim3(gx, (unsigned)b), dim3(256), 0, s, n, units, (const U*)x, (U*)y);
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_xent_weighted_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                                const int32_t* labels, const float* w, int w_div, float* loss, float* row_logp,
                                void* dlogits, long long ldd, float dloss_scale, fpnmt_stream_t stream) {
  if (!loss || !logits || !labels || !w) return fail(FPNMT_E_ARG, "xent_weighted: null pointer");
  if (w_div < 1) return fail(FPNMT_E_ARG, "xent_weighted: w_div < 1");
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32) return fail(FPNMT_E_ARG, "xent_weighted: bad dtype");
  if (rows < 0 || rows > 0x7fffffffll || v < 1 || ld < v || (dlogits && ldd < v))
    return fail(FPNMT_E_ARG, "xent_weighted: rows outside [0, 2^31) / v < 1 / ld < v / ldd < v");
  if (rows % w_div != 0) return fail(FPNMT_E_ARG, "xent_weighted: rows is not a multiple of w_div");
  if (rows == 0) return zero_fill(loss, sizeof(float), S(stream));
  float* row_loss = scratch_f32(rows);
  if (!row_loss) return fail(FPNMT_E_ARG, "xent_weighted: needs the fpnmt workspace");
  if (dtype == FPNMT_BF16)
    xw_dispatch<bf16>(rows, v, logits, ld, labels, w, w_div, row_loss, row_logp, (bf16*)dlogits, ldd, dloss_scale,
                      S(stream));
  else
    xw_dispatch<float>(rows, v, logits, ld, labels, w, w_div, row_loss, row_logp, (float*)dlogits, ldd, dloss_scale,
                       S(stream));
  // mean over ALL rows, summed in row order
  hipLaunchKernelGGL(xw_ordered_sum_kernel, dim3(1), dim3(256), 0, S(stream), rows, (const float*)row_loss,
                     1.f / (float)rows, loss);
  return check_launch("xent_weighted");
}

int fpnmt_repeat_rows(int dtype, int b, int n, long long len, const void* x, void* y, fpnmt_stream_t stream) {
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32) return fail(FPNMT_E_ARG, "repeat_rows: bad dtype");
  if (b < 0 || n < 0 || len < 0 || b > 65535) return fail(FPNMT_E_ARG, "repeat_rows: negative size / b > 65535");
  if (b == 0 || n == 0 || len == 0) return 0;
  if (!x || !y) return fail(FPNMT_E_ARG, "repeat_rows: null pointer");
  const long long esize = dtype == FPNMT_BF16 ? 2 : 4, bytes = len * esize;
  if ((bytes & 15) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0)
    repeat_rows_launch<uint4>(b, n, bytes >> 4, x, y, S(stream));
  else if (esize == 2)
    repeat_rows_launch<uint16_t>(b, n, len, x, y, S(stream));
  else
    repeat_rows_launch<uint32_t>(b, n, len, x, y, S(stream));
  return check_launch("repeat_rows");
}

}  // extern "C"

// Ensemble decoding: one launch that folds the fp32 logits rows of M models
// into one row per decode row, between the models' last GEMMs and the step
// kernels (fpnmt_logits_constrain, fpnmt_beam_step_log, fpnmt_beam_step,
// fpnmt_sample_step), which all normalise the row they are given themselves.
//   mode 0 "prob":    out[j] = log sum_m w_m softmax(l_m)[j]
//                            = logsumexp_m(l_m[j] + (log w_m - lse_m))
//   mode 1 "logprob": out[j] = sum_m w_m (l_m[j] - lse_m)      (unnormalised)
// The pointers, leading dimensions and weights travel by value in the launch
// arguments (EnsArgs), so a captured graph holds them.
//
// One block of EN_THREADS per row, two sweeps over every model's row:
//   1. per model an online (max, sum exp) per thread, merged across the wave
//      by shuffles and across the waves through LDS: lse_m = max + log(sum).
//      A NaN or +inf anywhere, or a row that is -inf throughout, marks the
//      row bad (every output column NaN);
//   2. the combine, every thread on its own columns of all models: the reads
//      are the second touch of a row of <= 40 KB per model that the same
//      block streamed a moment ago, so they are served from L2.
// Loads and stores are 16 bytes per lane where the row's address allows it:
// each row is split into a scalar head up to the next 16-byte boundary, a
// float4 body and a scalar tail, all inside [0, vocab) — nothing is read or
// written past vocab (ldl may equal vocab: the next row starts there). Sweep
// 2 partitions the columns by the OUTPUT row's alignment; a model whose row
// is aligned differently is read with four scalar loads there.
// out == logits[0] is safe: sweep 1 of every model ends (block barrier)
// before the first store, and in sweep 2 a column is read and written by the
// same thread only.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int EN_THREADS = 256, EN_WAVES = EN_THREADS / 64, EN_MAX = FPNMT_ENSEMBLE_MAX;

struct EnsArgs {
  const float* l[EN_MAX];
  long long ld[EN_MAX];
  float w[EN_MAX];
  float logw[EN_MAX];
};

// running (max, sum of exp(x - max)); m == -inf means "nothing finite yet", s == 0
__device__ __forceinline__ void ms_add4(float& m, float& s, int& bad, float a, float b, float c, float d) {
  bad |= !(a < INFINITY) | !(b < INFINITY) | !(c < INFINITY) | !(d < INFINITY);  // NaN or +inf
  const float mx = fmaxf(fmaxf(a, b), fmaxf(c, d));
  if (mx > m) {
    s *= expf(m - mx);  // m == -inf: s is 0 and stays 0
    m = mx;
  }
  if (m > -INFINITY) s += (expf(a - m) + expf(b - m)) + (expf(c - m) + expf(d - m));
}
__device__ __forceinline__ void ms_add1(float& m, float& s, int& bad, float a) {
  bad |= !(a < INFINITY);
  if (a > m) {
    s *= expf(m - a);
    m = a;
  }
  if (m > -INFINITY) s += expf(a - m);
}
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx > -INFINITY) s = s * expf(m - mx) + s2 * expf(m2 - mx);  // symmetric: both partners get the same bits
  m = mx;
}

// elements from p up to the next 16-byte boundary (p is 4-byte aligned), at most n
__device__ __forceinline__ int head_of(const float* p, int n) {
  const int h = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);
  return h < n ? h : n;
}
__device__ __forceinline__ float4 load4(const float* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

template <int MODE>
__device__ __forceinline__ float combine(const float (&x)[EN_MAX], const float (&c)[EN_MAX], const EnsArgs& A, int M) {
  if (MODE == 0) {
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m)
      if (m < M) mx = fmaxf(mx, x[m] + c[m]);
    if (!(mx > -INFINITY)) return -INFINITY;  // -inf in every model
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m)
      if (m < M) s += expf((x[m] + c[m]) - mx);  // a -inf term adds exp(-inf) = 0
    return mx + logf(s);
  }
  float acc = 0.f;
#pragma unroll
  for (int m = 0; m < EN_MAX; ++m)
    if (m < M) acc += A.w[m] * (x[m] - c[m]);  // -inf in any model: -inf (w > 0, no +inf in a good row)
  return acc;
}

template <int MODE>
__global__ __launch_bounds__(EN_THREADS) void logits_ensemble_kernel(int rows, int vocab, int M, EnsArgs A,
                                                                     const int32_t* __restrict__ fin, float* out,
                                                                     long long ldo) {
  __shared__ float sm[EN_MAX][EN_WAVES], ss[EN_MAX][EN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r = blockIdx.x;
  if (fin && fin[r] != 0) return;  // block-uniform, before any barrier: neither read nor written
  int bad = 0;
  for (int m = 0; m < M; ++m) {
    const float* p = A.l[m] + r * A.ld[m];
    const int head = head_of(p, vocab), nv = (vocab - head) >> 2;
    float mx = -INFINITY, s = 0.f;
    if (tid < head) ms_add1(mx, s, bad, p[tid]);
    const float4* pv = reinterpret_cast<const float4*>(p + head);
    for (int i = tid; i < nv; i += EN_THREADS) {
      const float4 v = pv[i];
      ms_add4(mx, s, bad, v.x, v.y, v.z, v.w);
    }
    const int j = head + 4 * nv + tid;
    if (j < vocab) ms_add1(mx, s, bad, p[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ms_merge(mx, s, __shfl_xor(mx, o, 64), __shfl_xor(s, o, 64));
    if (lane == 0) {
      sm[m][wave] = mx;
      ss[m][wave] = s;
    }
  }
  bad = __syncthreads_or(bad);  // also: the partials are visible, and every read of sweep 1 is done
  float c[EN_MAX];
#pragma unroll
  for (int m = 0; m < EN_MAX; ++m) {
    c[m] = 0.f;
    if (m < M) {
      float mx = sm[m][0], s = ss[m][0];
#pragma unroll
      for (int w = 1; w < EN_WAVES; ++w) ms_merge(mx, s, sm[m][w], ss[m][w]);
      bad |= !(mx > -INFINITY);  // -inf in all columns (every thread sees the same partials)
      const float lse = mx + logf(s);
      c[m] = MODE == 0 ? A.logw[m] - lse : lse;
    }
  }
  float* o = out + r * ldo;
  const int head = head_of(o, vocab), nv = (vocab - head) >> 2;
  const int jt = head + 4 * nv + tid;
  if (bad) {
    const float q = __builtin_nanf("");
    if (tid < head) o[tid] = q;
    for (int i = tid; i < nv; i += EN_THREADS) *reinterpret_cast<float4*>(o + head + 4 * i) = make_float4(q, q, q, q);
    if (jt < vocab) o[jt] = q;
    return;
  }
  const float* p[EN_MAX];
  bool al[EN_MAX];
#pragma unroll
  for (int m = 0; m < EN_MAX; ++m) {
    p[m] = m < M ? A.l[m] + r * A.ld[m] : nullptr;
    al[m] = (((uintptr_t)(p[m] + head)) & 15) == 0;
  }
  float x[EN_MAX];
  if (tid < head) {
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? p[m][tid] : 0.f;
    o[tid] = combine<MODE>(x, c, A, M);
  }
  for (int i = tid; i < nv; i += EN_THREADS) {
    const int j = head + 4 * i;
    float4 v[EN_MAX];
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m)
      if (m < M) v[m] = load4(p[m] + j, al[m]);
    float4 y;
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? v[m].x : 0.f;
    y.x = combine<MODE>(x, c, A, M);
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? v[m].y : 0.f;
    y.y = combine<MODE>(x, c, A, M);
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? v[m].z : 0.f;
    y.z = combine<MODE>(x, c, A, M);
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? v[m].w : 0.f;
    y.w = combine<MODE>(x, c, A, M);
    *reinterpret_cast<float4*>(o + j) = y;
  }
  if (jt < vocab) {
#pragma unroll
    for (int m = 0; m < EN_MAX; ++m) x[m] = m < M ? p[m][jt] : 0.f;
    o[jt] = combine<MODE>(x, c, A, M);
  }
}

// [p, p + ((rows - 1) * ld + vocab) floats) of two row sets share a byte
bool overlaps(const float* a, long long lda, const float* b, long long ldb, int rows, int vocab) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((uintptr_t)(rows - 1) * lda + vocab) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((uintptr_t)(rows - 1) * ldb + vocab) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_logits_ensemble(int rows, int vocab, int n_models, const float* const* logits, const long long* ldl,
                          const float* weight, int mode, const int32_t* fin, float* out, long long ldo,
                          fpnmt_stream_t stream) {
  if (!logits || !ldl || !weight || !out) return fail(FPNMT_E_ARG, "logits_ensemble: null pointer");
  if (rows <= 0) return fail(FPNMT_E_ARG, "logits_ensemble: rows <= 0");
  if (vocab <= 0 || ldo < vocab) return fail(FPNMT_E_ARG, "logits_ensemble: bad vocab, or ldo < vocab");
  if (n_models < 1) return fail(FPNMT_E_ARG, "logits_ensemble: n_models < 1");
  if (n_models > FPNMT_ENSEMBLE_MAX) return fail(FPNMT_E_UNSUPPORTED, "logits_ensemble: more than 8 models");
  if (mode != 0 && mode != 1) return fail(FPNMT_E_ARG, "logits_ensemble: mode must be 0 (prob) or 1 (logprob)");
  EnsArgs A = {};
  for (int m = 0; m < n_models; ++m) {
    if (!logits[m]) return fail(FPNMT_E_ARG, "logits_ensemble: null pointer (a model's logits)");
    if (ldl[m] < vocab) return fail(FPNMT_E_ARG, "logits_ensemble: ldl < vocab");
    if (!(weight[m] > 0.f) || !isfinite(weight[m]))
      return fail(FPNMT_E_ARG, "logits_ensemble: weight must be a finite positive number");
    const bool same = m == 0 && logits[0] == out && ldl[0] == ldo;  // in place on the first model
    if (!same && overlaps(logits[m], ldl[m], out, ldo, rows, vocab))
      return fail(FPNMT_E_ARG, "logits_ensemble: out overlaps an input (only out == logits[0], same ld, may)");
    A.l[m] = logits[m];
    A.ld[m] = ldl[m];
    A.w[m] = weight[m];
    A.logw[m] = (float)log((double)weight[m]);
  }
  const dim3 grid(rows), block(EN_THREADS);
  if (mode == 0)
    hipLaunchKernelGGL(logits_ensemble_kernel<0>, grid, block, 0, S(stream), rows, vocab, n_models, A, fin, out, ldo);
  else
    hipLaunchKernelGGL(logits_ensemble_kernel<1>, grid, block, 0, S(stream), rows, vocab, n_models, A, fin, out, ldo);
  return check_launch("logits_ensemble");
}

}  // extern "C"

// Sampled caption decoding: the last launch of a decode step that DRAWS the
// next token of every row from its fp32 logits (temperature, top-k, nucleus)
// instead of ranking candidates. One block per row (256 threads, 512 on the
// filtered path), rows independent, no host round trip: the uniform comes
// from the counter hash of common.h keyed like dropout (seed + device word),
// so a replayed hipGraph draws new numbers when the host changes the word.
//
// Weights are summed as 40-bit fixed point: w = exp((l - max) / T) lies in
// [0, 1], q = trunc(w * 2^40) is an integer, and integer sums are exact in
// any order. That makes the two thresholds, the kept set and the drawn token
// a function of the logits and u alone (no dependence on the order in which
// 256 threads add), at an absolute error below V * 2^-40 of the maximum
// weight — four orders under an fp32 sum's. A weight below 2^-40 of the
// maximum counts as 0 and is never drawn.
//
//  * unfiltered (top_k off, top_p == 1): nothing staged; one max pass, one
//    sums pass (the temperature-1 sum for the score and the tempered sum for
//    the draw; at T == 1 they are one), and the CDF walk, which only the wave
//    whose quarter of the row holds the target repeats over that quarter.
//  * filtered: the row is staged in LDS (vocab <= FPNMT_SAMPLE_FILTER_MAX_VOCAB)
//    and the thresholds are found exactly by a radix select over the
//    order-preserving integer keys of the logits, 8 bits per round: top-k on a
//    count histogram, top-p on a weight histogram (larger logit = larger
//    weight, so "the shortest prefix by weight" is a key threshold too). A
//    threshold is a key value, so every token bitwise equal to the boundary
//    is inside: the kept set does not depend on scan order. Nothing is sorted.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

typedef unsigned long long u64;
// threads per row: 256, and 512 on the filtered path, where the staged row
// bounds the blocks per CU (measured: top_p 137 -> 131 us at 2048 x 10 000)
constexpr int sm_threads(bool filt) { return filt ? 512 : 256; }
constexpr int sm_waves(bool filt) { return sm_threads(filt) / 64; }
constexpr int SM_BINS = 256;
constexpr int FIX_BITS = 40;
constexpr u64 FIX_ONE = 1ull << FIX_BITS;

__device__ __forceinline__ u64 sample_key(u64 seed, const long long* seed_dev) {  // drop_key_of (elementwise.hip)
  return seed + (seed_dev ? (u64)(*seed_dev) * 0x9E3779B97F4A7C15ull : 0ull);
}
__device__ __forceinline__ uint32_t sample_bits(u64 key, int r, int t) {  // 24 bits: u = bits * 2^-24
  return hash_u32(key, ((uint64_t)r << 16) | (uint64_t)t) & 0xFFFFFF;
}

// order-preserving key of a non-NaN float (-0 counts as +0): a < b <=> key(a) < key(b)
__device__ __forceinline__ uint32_t key_of(float l) {
  uint32_t b = __float_as_uint(l);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// fixed-point weight of a logit (finite or -inf) under a finite row maximum
__device__ __forceinline__ u64 fix_w(float l, float mx, float inv_t) {
  const float d = l - mx;
  if (d == 0.f) return FIX_ONE;       // the maximum itself, whatever inv_t
  if (d == -INFINITY) return 0ull;    // a -inf logit weighs nothing
  return (u64)(expf(d * inv_t) * (float)FIX_ONE);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// f(logit, index) over the wave's share [ub, ue) of the row's units (a unit
// is 4 logits when VEC, else 1), in index order per lane and iteration
template <bool VEC, class F>
__device__ __forceinline__ void seg_for(const float* src, int ub, int ue, int lane, F f) {
  if (VEC) {
    const f32x4* s4 = (const f32x4*)src;
#pragma unroll 4
    for (int u = ub + lane; u < ue; u += 64) {
      const f32x4 a = s4[u];
#pragma unroll
      for (int q = 0; q < 4; ++q) f(a[q], u * 4 + q);
    }
  } else {
#pragma unroll 4
    for (int u = ub + lane; u < ue; u += 64) f(src[u], u);
  }
}

// inclusive suffix sum over the block's values in thread order (thread tid
// holds bin tid; threads past the bins hold 0)
template <int NW>
__device__ __forceinline__ u64 block_suffix_incl(u64 v, u64* wtot, int lane, int wave) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 n = __shfl_down(v, o, 64);
    if (lane + o < 64) v += n;
  }
  if (lane == 0) wtot[wave] = v;
  __syncthreads();
  for (int w = wave + 1; w < NW; ++w) v += wtot[w];
  __syncthreads();
  return v;
}

// The largest key K among the tokens with key >= theta_min such that the
// amounts (1 per token, or its fixed-point weight) of the tokens with
// key >= K sum to at least the target: top_k itself for counts,
// ceil(top_p * total) for weights. Four rounds of 8 bits, most significant
// first; `prefix` holds the digits fixed so far.
template <bool VEC, bool WEIGHT, int NW>
__device__ __forceinline__ uint32_t radix_select(const float* src, int ub, int ue, int tid, float mx, float inv_t,
                                                 uint32_t theta_min, u64 target, float top_p, u64* bins, u64* wtot,
                                                 u64* sel) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0;
  for (int round = 0; round < 4; ++round) {
    const int shift = 24 - 8 * round;
    const uint32_t himask = round ? (0xFFFFFFFFu << (shift + 8)) : 0u;
    uint32_t* cbins = (uint32_t*)bins;  // counts fit 32 bits
    if (tid < SM_BINS) {
      if (WEIGHT) bins[tid] = 0ull;
      else cbins[tid] = 0u;
    }
    if (tid == 0) sel[0] = 0ull, sel[1] = 0ull;
    __syncthreads();
    seg_for<VEC>(src, ub, ue, lane, [&](float l, int) {
      const uint32_t k = key_of(l);
      if (k >= theta_min && (k & himask) == prefix) {
        if (WEIGHT) {
          const u64 a = fix_w(l, mx, inv_t);
          if (a) atomicAdd(&bins[(k >> shift) & 255u], a);
        } else {
          atomicAdd(&cbins[(k >> shift) & 255u], 1u);
        }
      }
    });
    __syncthreads();
    const u64 mine = tid < SM_BINS ? (WEIGHT ? bins[tid] : (u64)cbins[tid]) : 0ull;
    const u64 incl = block_suffix_incl<NW>(mine, wtot, lane, wave);
    if (WEIGHT && round == 0) {  // the survivors' total weight sets the target
      if (tid == 0) sel[2] = incl;
      __syncthreads();
      const u64 total = sel[2];
      target = (u64)ceil((double)top_p * (double)total);
      target = target < 1ull ? 1ull : (target > total ? total : target);
    }
    const u64 above = incl - mine;
    if (tid < SM_BINS && above < target && target <= incl) sel[0] = (u64)tid, sel[1] = above;
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    target -= sel[1];
    __syncthreads();
  }
  return prefix;
}

// the block's scratch (one per kernel, shared by the instantiations of sample_row)
template <bool FILT>
struct SampleShared {
  u64 bins[FILT ? SM_BINS : 1], red_c[sm_waves(FILT)], red_w[sm_waves(FILT)], red_s[sm_waves(FILT)],
      wtot[sm_waves(FILT)], sel[3];
  float red_f[sm_waves(FILT)];
  int red_i[sm_waves(FILT)];
  int tok;
};

template <bool FILT, bool VEC>
__device__ __forceinline__ void sample_row(SampleShared<FILT>& sh, int r, int vocab, const float* src, float inv_t,
                                           int top_k, float top_p, uint32_t ubits, float* score, int32_t* slen,
                                           int32_t* fin, int32_t* hist, int hist_ld, int t, int end_token,
                                           int32_t* tok_out, int32_t* kept_out) {
  float* red_f = sh.red_f;
  int* red_i = sh.red_i;
  u64 *red_c = sh.red_c, *red_w = sh.red_w, *red_s = sh.red_s, *wtot = sh.wtot, *sel = sh.sel, *bins = sh.bins;
  int& s_tok = sh.tok;
  constexpr int NW = sm_waves(FILT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nu = VEC ? vocab >> 2 : vocab;
  const int ub = (int)((long long)nu * wave / NW), ue = (int)((long long)nu * (wave + 1) / NW);
  // 1. the maximum; a NaN or +inf logit, or nothing above -inf: no drawable token
  float mx = -INFINITY;
  int bad = 0;
  seg_for<VEC>(src, ub, ue, lane, [&](float l, int) {
    mx = fmaxf(mx, l);
    bad |= l != l;
  });
  mx = wave_max(mx);
  bad = __ballot(bad) != 0ull;
  if (lane == 0) red_f[wave] = mx, red_i[wave] = bad;
  if (tid == 0) s_tok = -1;
  __syncthreads();
  mx = red_f[0], bad = red_i[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red_f[i]), bad |= red_i[i];
  if (bad || mx == INFINITY || mx == -INFINITY) {  // block-uniform
    if (tid == 0) {
      hist[(long long)r * hist_ld + t + 1] = end_token;
      tok_out[r] = end_token;
      score[r] = -INFINITY;
      slen[r] = t + 1;
      fin[r] = 1;
      if (kept_out) kept_out[r] = 0;
    }
    return;
  }
  // 2. the thresholds (keys): top-k on counts, then top-p on the survivors' weights
  uint32_t theta = 0u;
  if (FILT) {
    if (top_k > 0 && top_k < vocab)
      theta = radix_select<VEC, false, NW>(src, ub, ue, tid, mx, inv_t, 0u, (u64)top_k, 1.f, bins, wtot, sel);
    if (top_p < 1.f)
      theta = radix_select<VEC, true, NW>(src, ub, ue, tid, mx, inv_t, theta, 0ull, top_p, bins, wtot, sel);
  }
  // 3. per wave share: kept count, kept weight, and the temperature-1 sum of the whole row
  u64 c = 0ull, w = 0ull, s = 0ull;
  const bool t1 = inv_t == 1.f;
  seg_for<VEC>(src, ub, ue, lane, [&](float l, int) {
    const u64 a = fix_w(l, mx, 1.f);
    s += a;
    if (!FILT || key_of(l) >= theta) {
      c += 1ull;
      w += t1 ? a : fix_w(l, mx, inv_t);
    }
  });
  c = wave_sum_u64(c), w = wave_sum_u64(w), s = wave_sum_u64(s);
  if (lane == 0) red_c[wave] = c, red_w[wave] = w, red_s[wave] = s;
  __syncthreads();
  u64 W = 0ull, S1 = 0ull, kept64 = 0ull;  // W >= FIX_ONE: the maximum is always kept
#pragma unroll
  for (int i = 0; i < NW; ++i) W += red_w[i], S1 += red_s[i], kept64 += red_c[i];
  const int kept = (int)kept64;
  // 4. the draw: the smallest index whose prefix sum of kept weights, in
  //    index order, exceeds floor(u * W) (u = ubits * 2^-24 < 1, so one exists)
  const u64 tgt = __umul64hi(W, (u64)ubits << 40);
  u64 before = 0ull;  // kept weight of the waves below this one
  for (int i = 0; i < wave; ++i) before += red_w[i];
  if (before <= tgt && tgt < before + red_w[wave]) {  // wave-uniform: this wave's share holds the target
    u64 run = before;
    for (int u0 = ub; u0 < ue; u0 += 64) {  // wave-uniform bounds
      const int u = u0 + lane;
      u64 q[VEC ? 4 : 1];
      u64 ls = 0ull;
#pragma unroll
      for (int e = 0; e < (VEC ? 4 : 1); ++e) q[e] = 0ull;
      if (u < ue) {
        if (VEC) {
          const f32x4 a = ((const f32x4*)src)[u];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (!FILT || key_of(a[e]) >= theta) q[e] = fix_w(a[e], mx, inv_t);
        } else {
          const float a = src[u];
          if (!FILT || key_of(a) >= theta) q[0] = fix_w(a, mx, inv_t);
        }
      }
#pragma unroll
      for (int e = 0; e < (VEC ? 4 : 1); ++e) ls += q[e];
      u64 incl = ls;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 n = __shfl_up(incl, o, 64);
        if (lane >= o) incl += n;
      }
      const u64 hit = __ballot(run + incl > tgt);
      if (hit) {
        if (lane == __ffsll((long long)hit) - 1) {
          u64 p = run + incl - ls;
          int e = 0;
#pragma unroll
          for (; e < (VEC ? 4 : 1) - 1; ++e) {
            p += q[e];
            if (p > tgt) break;
          }
          s_tok = u * (VEC ? 4 : 1) + e;
        }
        break;
      }
      run += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int tok = s_tok;
    if (tok < 0 || tok >= vocab) {  // not reachable with exact prefix sums; never index from the sentinel
      hist[(long long)r * hist_ld + t + 1] = end_token;
      tok_out[r] = end_token;
      score[r] = -INFINITY;
      slen[r] = t + 1;
      fin[r] = 1;
      if (kept_out) kept_out[r] = 0;
      return;
    }
    hist[(long long)r * hist_ld + t + 1] = tok;
    tok_out[r] = tok;
    score[r] += src[tok] - (mx + logf((float)((double)S1 * (1.0 / (double)FIX_ONE))));
    slen[r] = t + 1;
    fin[r] = tok == end_token;
    if (kept_out) kept_out[r] = kept;
  }
}

template <bool FILT>
__global__ __launch_bounds__(sm_threads(FILT)) void sample_step_kernel(
    int vocab, const float* __restrict__ logits, long long ldl, float inv_t, int top_k, float top_p, u64 seed,
    const long long* __restrict__ seed_dev, float* __restrict__ score, int32_t* __restrict__ slen,
    int32_t* __restrict__ fin, int32_t* __restrict__ hist, int hist_ld, int t, int end_token,
    int32_t* __restrict__ tok_out, int32_t* __restrict__ kept_out) {
  extern __shared__ __attribute__((aligned(16))) float srow[];  // FILT: the row, vocab floats
  __shared__ SampleShared<FILT> sh;
  const int r = blockIdx.x, tid = threadIdx.x;
  if (fin[r] != 0) {  // block-uniform: a finished row pads with <end>; its logits are not read
    if (tid == 0) {
      hist[(long long)r * hist_ld + t + 1] = end_token;
      tok_out[r] = end_token;
      if (kept_out) kept_out[r] = 0;
    }
    return;
  }
  const uint32_t ubits = sample_bits(sample_key(seed, seed_dev), r, t);
  const float* lr = logits + (long long)r * ldl;
  const bool gvec = (vocab & 3) == 0 && (ldl & 3) == 0 && ((uintptr_t)logits & 15) == 0;
  if constexpr (FILT) {
    if (gvec) {
      for (int u = tid; u < (vocab >> 2); u += sm_threads(FILT)) ((f32x4*)srow)[u] = ((const f32x4*)lr)[u];
    } else {
      for (int j = tid; j < vocab; j += sm_threads(FILT)) srow[j] = lr[j];
    }
    __syncthreads();
    if ((vocab & 3) == 0)
      sample_row<true, true>(sh, r, vocab, srow, inv_t, top_k, top_p, ubits, score, slen, fin, hist, hist_ld, t,
                             end_token, tok_out, kept_out);
    else
      sample_row<true, false>(sh, r, vocab, srow, inv_t, top_k, top_p, ubits, score, slen, fin, hist, hist_ld, t,
                              end_token, tok_out, kept_out);
  } else {
    if (gvec)
      sample_row<false, true>(sh, r, vocab, lr, inv_t, top_k, top_p, ubits, score, slen, fin, hist, hist_ld, t,
                              end_token, tok_out, kept_out);
    else
      sample_row<false, false>(sh, r, vocab, lr, inv_t, top_k, top_p, ubits, score, slen, fin, hist, hist_ld, t,
                               end_token, tok_out, kept_out);
  }
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(int rows, int t, u64 seed,
                                                             const long long* __restrict__ seed_dev,
                                                             float* __restrict__ u_out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows) u_out[r] = (float)sample_bits(sample_key(seed, seed_dev), r, t) * (1.0f / 16777216.0f);
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_sample_step(int rows, int vocab, const float* logits, long long ldl, float temperature, int top_k,
                      float top_p, unsigned long long seed, const long long* seed_dev, float* score, int32_t* slen,
                      int32_t* fin, int32_t* hist, int hist_ld, int t, int end_token, int32_t* tok_out,
                      int32_t* kept_out, fpnmt_stream_t stream) {
  if (rows <= 0) return 0;
  if (!(temperature > 0.f) || !isfinite(temperature))
    return fail(FPNMT_E_ARG, "sample_step: temperature must be a finite positive number");
  if (!(top_p > 0.f && top_p <= 1.f)) return fail(FPNMT_E_ARG, "sample_step: top_p outside (0, 1]");
  if (top_k < 0) return fail(FPNMT_E_ARG, "sample_step: top_k < 0");
  if (vocab <= 0 || ldl < vocab) return fail(FPNMT_E_ARG, "sample_step: bad vocab, or ldl < vocab");
  if (end_token < 0 || end_token >= vocab) return fail(FPNMT_E_ARG, "sample_step: end_token outside the vocabulary");
  if (t < 0 || t >= 65536 || hist_ld < t + 2)
    return fail(FPNMT_E_ARG, "sample_step: bad position / table widths (0 <= t < 65536, hist_ld >= t + 2)");
  if (!logits || !score || !slen || !fin || !hist || !tok_out) return fail(FPNMT_E_ARG, "sample_step: null pointer");
  const bool filt = (top_k > 0 && top_k < vocab) || top_p < 1.f;
  if (filt && vocab > FPNMT_SAMPLE_FILTER_MAX_VOCAB)
    return fail(FPNMT_E_UNSUPPORTED, "sample_step: top_k / top_p need vocab <= 16384 (the row is staged in LDS)");
  if (vocab > (1 << 22)) return fail(FPNMT_E_UNSUPPORTED, "sample_step: vocab above 2^22 (fixed-point weight sums)");
  float inv_t = 1.0f / temperature;
  if (!isfinite(inv_t)) inv_t = 3.0e38f;
  if (filt) {
    static bool lds_ok = false;  // rows above ~60 KB exceed the default dynamic LDS bound beside the histograms
    if (!lds_ok) {
      if (hipFuncSetAttribute((const void*)sample_step_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              FPNMT_SAMPLE_FILTER_MAX_VOCAB * (int)sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FPNMT_E_HIP, "sample_step: cannot reserve LDS for the staged row");
      }
      lds_ok = true;
    }
    hipLaunchKernelGGL(sample_step_kernel<true>, dim3(rows), dim3(sm_threads(true)), (size_t)vocab * sizeof(float),
                       S(stream), vocab, logits, ldl, inv_t, top_k, top_p, seed, seed_dev, score, slen, fin, hist,
                       hist_ld, t, end_token, tok_out, kept_out);
  } else {
    hipLaunchKernelGGL(sample_step_kernel<false>, dim3(rows), dim3(sm_threads(false)), 0, S(stream), vocab, logits, ldl,
                       inv_t, top_k, top_p, seed, seed_dev, score, slen, fin, hist, hist_ld, t, end_token, tok_out,
                       kept_out);
  }
  return check_launch("sample_step");
}

int fpnmt_sample_uniform(int rows, int t, unsigned long long seed, const long long* seed_dev, float* u_out,
                         fpnmt_stream_t stream) {
  if (rows <= 0) return 0;
  if (t < 0 || t >= 65536) return fail(FPNMT_E_ARG, "sample_uniform: bad position (0 <= t < 65536)");
  if (!u_out) return fail(FPNMT_E_ARG, "sample_uniform: null pointer");
  hipLaunchKernelGGL(sample_uniform_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, S(stream), rows, t, seed, seed_dev,
                     u_out);
  return check_launch("sample_uniform");
}

}  // extern "C"

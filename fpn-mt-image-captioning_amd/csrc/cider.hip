// Device-side CIDEr-D reward for self-critical training (not in the
// reference): the sampled captions are scored where the sampler left them, so
// a self-critical step has no host round trip.
//
// fpnmt_ciderd_reward: one wave (one 64-thread block) per caption row. The
// wave packs the row's 1..4-grams into uint64 keys in LDS (exact, not a hash:
// sum_i (tok_i + 1) << 16 i), finds every key's term frequency and
// first-occurrence flag by comparison within its order (a caption has a few
// dozen tokens: an O(L^2) pass beats a sort), looks the idf up by binary
// search in the document table, and for every reference of the row's image
// binary-searches the reference's sorted entries. fp64 throughout, plain C++:
// the work is tiny and latency-bound. Every sum is lane-strided partials
// joined by a fixed shuffle tree, no atomics: a launch is bitwise repeatable
// and a row's result does not depend on the rows launched with it. The tables
// hold tf * idf, the norms and the Gaussian factor as the host computes them
// (fpnmt/cider_device.py), so no transcendental function is evaluated here;
// the final arithmetic is utils/cider_reward.py's _sim / score_one literally.
//
// fpnmt_scst_pack: one block per image turns the rewards into fp32
// advantages and the sampler's state into padded training rows; block 0 also
// sums the three reported means (one wave, fp64, a fixed order).
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int CD_MAX_LEN = FPNMT_CIDER_MAX_LEN;
constexpr int CD_MAX_KEYS = 4 * CD_MAX_LEN;  // 4 L - 6 for L >= 3

// index of key in the ascending keys[lo, hi), or -1
__device__ __forceinline__ long long cd_find(const unsigned long long* __restrict__ keys, long long lo, long long hi,
                                             unsigned long long key) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    const unsigned long long v = keys[mid];
    if (v == key) return mid;
    if (v < key) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

__global__ __launch_bounds__(64) void ciderd_reward_kernel(fpnmt_cider_tables t, int n,
                                                           const int32_t* __restrict__ hist, int hist_ld,
                                                           const int32_t* __restrict__ slen,
                                                           const int32_t* __restrict__ fin,
                                                           const int32_t* __restrict__ img_index,
                                                           double* __restrict__ reward) {
  __shared__ unsigned long long keys[CD_MAX_KEYS];
  __shared__ double wgt[CD_MAX_KEYS];  // tf * idf at a first occurrence, -1 at a repeat
  const int row = blockIdx.x, lane = threadIdx.x;
  const int img = img_index[row / n];
  int L = slen[row] - fin[row];
  L = min(max(L, 0), min(hist_ld - 1, t.max_len));
  if (img < 0 || img >= t.n_images || L == 0) {  // block-uniform
    if (lane == 0) reward[row] = 0.0;
    return;
  }
  const int32_t* h = hist + (long long)row * hist_ld + 1;
  // keys of order k + 1 at [off[k], off[k + 1])
  int off[5];
  off[0] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + max(L - k, 0);
  const int total = off[4];
  for (int e = lane; e < total; e += 64) {
    const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
    const int p = e - off[k];
    unsigned long long key = 0;
    for (int i = 0; i <= k; ++i) key |= (unsigned long long)(uint32_t)(h[p + i] + 1) << (16 * i);
    keys[e] = key;
  }
  __syncthreads();
  double nh2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = lane; e < total; e += 64) {
    const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
    const unsigned long long key = keys[e];
    int tf = 0;
    bool first = true;
    for (int j = off[k]; j < off[k + 1]; ++j) {
      const bool eq = keys[j] == key;
      tf += eq;
      first = first && !(eq && j < e);
    }
    double w = -1.0;
    if (first) {
      const long long at = cd_find(t.df_keys, 0, t.n_df, key);
      w = (double)tf * (at >= 0 ? t.df_idf[at] : t.idf_absent);
      const double w2 = w * w;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == k) nh2[q] += w2;
    }
    wgt[e] = w;
  }
  __syncthreads();
  double nh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) nh[k] = sqrt(wave_sum(nh2[k]));
  const int len_h = max(L - 1, 0);  // the host's "length": the sum of the bigram counts
  const int j0 = t.img_off[img], j1 = t.img_off[img + 1];
  double score[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = j0; j < j1; ++j) {
    const long long e0 = t.ref_off[j], e1 = t.ref_off[j + 1];
    double val[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = lane; e < total; e += 64) {
      const double w = wgt[e];
      if (w < 0.0) continue;
      const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
      const long long at = cd_find(t.ref_keys, e0, e1, keys[e]);
      const double r = at >= 0 ? t.ref_w[at] : 0.0;
      const double term = fmin(w, r) * r;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == k) val[q] += term;
    }
    const int d = abs(len_h - t.ref_len[j]);
    const double g = t.gauss[min(d, t.n_gauss - 1)];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double v = wave_sum(val[k]);
      const double nr = t.ref_norm[4ll * j + k];
      if (nh[k] != 0.0 && nr != 0.0) v /= nh[k] * nr;
      v *= g;
      score[k] += v;
    }
  }
  if (lane == 0) {
    const double mean = (((score[0] + score[1]) + score[2]) + score[3]) / 4.0;
    reward[row] = j1 > j0 ? mean / (double)(j1 - j0) * 10.0 : 0.0;
  }
}

// baseline of sample s of an image whose n rewards are r[0 .. n)
__device__ __forceinline__ double sp_base(int mode, const double* __restrict__ r, int n, int s, double g) {
  if (mode == FPNMT_SCST_GREEDY) return g;
  double sum = 0.0;
  for (int q = 0; q < n; ++q)
    if (q != s) sum += r[q];
  return sum / (double)(n - 1);
}

__global__ __launch_bounds__(64) void scst_pack_kernel(int b, int n, int mode, const double* __restrict__ reward,
                                                       const double* __restrict__ greedy,
                                                       const int32_t* __restrict__ hist, int hist_ld,
                                                       const int32_t* __restrict__ slen,
                                                       const int32_t* __restrict__ fin,
                                                       const float* __restrict__ score, int start_token,
                                                       int end_token, int max_tokens, long long* __restrict__ tok,
                                                       int width, float* __restrict__ adv,
                                                       double* __restrict__ scalars) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const double* r = reward + (long long)i * n;
  const double g = mode == FPNMT_SCST_GREEDY ? greedy[i] : 0.0;
  for (int s = lane; s < n; s += 64) adv[(long long)i * n + s] = (float)(r[s] - sp_base(mode, r, n, s, g));
  for (int s = 0; s < n; ++s) {
    const long long row = (long long)i * n + s;
    const int L = min(max(slen[row] - fin[row], 0), hist_ld - 1);
    const int32_t* h = hist + row * hist_ld;
    long long* out = tok + row * width;
    for (int c = lane; c < width; c += 64) {
      long long v = 0;
      if (c == 0) v = start_token;
      else if (c <= L) v = h[c];
      else if (c == L + 1 && L < max_tokens) v = end_token;
      out[c] = v;
    }
  }
  if (i == 0) {  // the reported means: lane-strided partials in row order, joined by the fixed shuffle tree
    double sr = 0.0, sb = 0.0, sl = 0.0;
    const long long rows = (long long)b * n;
    for (long long q = lane; q < rows; q += 64) {
      const int ii = (int)(q / n), s = (int)(q % n);
      const double* ri = reward + (long long)ii * n;
      sr += ri[s];
      sb += sp_base(mode, ri, n, s, mode == FPNMT_SCST_GREEDY ? greedy[ii] : 0.0);
      sl += (double)score[q];
    }
    sr = wave_sum(sr), sb = wave_sum(sb), sl = wave_sum(sl);
    if (lane == 0) {
      const double cnt = (double)b * (double)n;
      scalars[0] = sr / cnt;
      scalars[1] = sb / cnt;
      scalars[2] = sl / cnt;
    }
  }
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_ciderd_reward(const fpnmt_cider_tables* t, int rows, int n, const int32_t* hist, int hist_ld,
                        const int32_t* slen, const int32_t* fin, const int32_t* img_index, double* reward,
                        fpnmt_stream_t stream) {
  if (!t || !hist || !slen || !fin || !img_index || !reward) return fail(FPNMT_E_ARG, "ciderd_reward: null pointer");
  if (!t->df_keys || !t->df_idf || !t->img_off || !t->ref_off || !t->ref_keys || !t->ref_w || !t->ref_norm ||
      !t->ref_len || !t->gauss)
    return fail(FPNMT_E_ARG, "ciderd_reward: null table pointer");
  if (n < 1 || rows < 0 || rows % n != 0) return fail(FPNMT_E_ARG, "ciderd_reward: n < 1 / rows < 0 / rows % n != 0");
  if (hist_ld < 1 || t->n_df < 0 || t->n_images < 0 || t->n_gauss < 1 || t->max_len < 1)
    return fail(FPNMT_E_ARG, "ciderd_reward: hist_ld < 1 / negative table size / n_gauss < 1 / max_len < 1");
  if (t->max_len > CD_MAX_LEN || hist_ld - 1 > t->max_len)
    return fail(FPNMT_E_UNSUPPORTED, "ciderd_reward: captions of up to hist_ld - 1 = " + std::to_string(hist_ld - 1) +
                                         " tokens exceed the tables' max_len " + std::to_string(t->max_len) +
                                         " (at most " + std::to_string(CD_MAX_LEN) + ")");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ciderd_reward_kernel, dim3((unsigned)rows), dim3(64), 0, S(stream), *t, n, hist, hist_ld, slen,
                     fin, img_index, reward);
  return check_launch("ciderd_reward");
}

int fpnmt_scst_pack(int b, int n, int mode, const double* reward, const double* greedy, const int32_t* hist,
                    int hist_ld, const int32_t* slen, const int32_t* fin, const float* score, int start_token,
                    int end_token, int max_tokens, long long* tok, int width, float* adv, double* scalars,
                    fpnmt_stream_t stream) {
  if (!reward || !hist || !slen || !fin || !score || !tok || !adv || !scalars)
    return fail(FPNMT_E_ARG, "scst_pack: null pointer");
  if (mode != FPNMT_SCST_MEAN && mode != FPNMT_SCST_GREEDY) return fail(FPNMT_E_ARG, "scst_pack: bad mode");
  if (mode == FPNMT_SCST_GREEDY && !greedy) return fail(FPNMT_E_ARG, "scst_pack: the greedy baseline needs greedy[b]");
  if (b < 0 || n < 1 || hist_ld < 1 || width < 1 || max_tokens < 0)
    return fail(FPNMT_E_ARG, "scst_pack: b < 0 / n < 1 / hist_ld < 1 / width < 1 / max_tokens < 0");
  if (mode == FPNMT_SCST_MEAN && n < 2) return fail(FPNMT_E_ARG, "scst_pack: the mean baseline needs n >= 2");
  if (b == 0) return 0;
  hipLaunchKernelGGL(scst_pack_kernel, dim3((unsigned)b), dim3(64), 0, S(stream), b, n, mode, reward, greedy, hist,
                     hist_ld, slen, fin, score, start_token, end_token, max_tokens, tok, width, adv, scalars);
  return check_launch("scst_pack");
}

}  // extern "C"

// Consensus (minimum-Bayes-risk) caption selection under CIDEr-D (not in the
// reference): among an image's n candidate captions, left on the device by
// the sampler or the beam search, the one that agrees most with the others.
//
// fpnmt_ciderd_consensus: one block of eight waves per image.
//   Phase 1, a wave per candidate: the wave packs the caption's 1..4-grams
//     into the exact uint64 keys of cider.hip, and by one O(L^2) comparison
//     within each order finds every key's term frequency and its place in the
//     ascending order of that order's keys (the count of smaller keys plus the
//     count of equal keys before it: a counting sort, duplicates adjacent). It
//     looks the idf up by binary search in the document table and leaves
//     keys / tf * idf sorted per order in LDS, with the four norms and the
//     length. The references of a pair are other candidates, so nothing but
//     the document table and the Gaussian table is read from memory.
//   Phase 2, a wave per hypothesis s: for j = 0 .. n - 1 the lanes stride over
//     the distinct keys of c_s and binary-search c_j's keys of the same order
//     in LDS; the four orders are joined by the fixed shuffle tree and the
//     similarity is utils/cider_reward.py's _sim / score_one with c_j as the
//     only reference. The weighted sums run over ascending j in one lane's
//     registers, so no n x n matrix is kept.
//   Phase 3: the arg-max of the n utilities, ties to the lowest index.
// fp64 throughout, plain C++, no transcendental function (the tables hold
// those values), no atomics: a launch is bitwise repeatable and an image's
// outputs do not depend on the other images of the launch.
//
// LDS: per candidate E = L + (L - 1) + (L - 2) + (L - 3) entries (those above
// zero) of 16 bytes at the caption limit L = min(hist_ld - 1, max_len), plus
// one wave's unsorted keys per wave and 44 bytes per candidate: n = 64 at
// L = 32 is 64 * 122 * 16 B = 122 KB + 10 KB of gfx950's 160 KB per
// work-group. What does not fit is refused at the call.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int CS_WAVES = 8;
constexpr int CS_THREADS = 64 * CS_WAVES;
constexpr long long CS_LDS_BYTES = 160 * 1024;  // gfx950: LDS per work-group

// entries of a caption of L tokens: its 1..4-grams
__host__ __device__ __forceinline__ int cs_entries(int L) {
  return max(L, 0) + max(L - 1, 0) + max(L - 2, 0) + max(L - 3, 0);
}

__host__ __device__ __forceinline__ long long cs_lds_bytes(int n, int E) {
  // keys + weights, the waves' unsorted keys, norms + utilities, lengths
  return (long long)n * E * 16 + (long long)CS_WAVES * E * 8 + (long long)n * 40 + (long long)n * 4;
}

// index of key in the ascending keys[lo, hi) (any of its duplicates), or -1
template <typename P>
__device__ __forceinline__ long long cs_find(P keys, long long lo, long long hi, unsigned long long key) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    const unsigned long long v = keys[mid];
    if (v == key) return mid;
    if (v < key) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

__global__ __launch_bounds__(CS_THREADS) void ciderd_consensus_kernel(
    fpnmt_cider_tables t, int n, int E, const int32_t* __restrict__ hist, int hist_ld,
    const int32_t* __restrict__ len, const int32_t* __restrict__ fin, const double* __restrict__ weight,
    double* __restrict__ util, int32_t* __restrict__ pick, double* __restrict__ pair) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long cs_lds[];
  unsigned long long* keys = cs_lds;                          // [n][E], ascending within each order
  double* wgt = (double*)(keys + (long long)n * E);           // [n][E] tf * idf (the same at every duplicate)
  unsigned long long* raw = (unsigned long long*)(wgt + (long long)n * E);  // [CS_WAVES][E] in position order
  double* norm = (double*)(raw + (long long)CS_WAVES * E);    // [n][4]
  double* ut = norm + 4 * n;                                  // [n]
  int* clen = (int*)(ut + n);                                 // [n] tokens
  const int img = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row0 = (long long)img * n;
  const int cap = min(hist_ld - 1, t.max_len);

  // ---- phase 1: every candidate's sorted keys, weights, norms, length
  for (int c0 = 0; c0 < n; c0 += CS_WAVES) {  // block-uniform trip count: the barriers below are reached by all
    const int c = c0 + wave;
    int L = 0;
    int off[5] = {0, 0, 0, 0, 0};
    unsigned long long* rk = raw + wave * E;
    if (c < n) {
      L = min(max(len[row0 + c] - fin[row0 + c], 0), cap);
#pragma unroll
      for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + max(L - k, 0);
      const int32_t* h = hist + (row0 + c) * hist_ld + 1;
      for (int e = lane; e < off[4]; e += 64) {
        const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
        const int p = e - off[k];
        unsigned long long key = 0;
        for (int i = 0; i <= k; ++i) key |= (unsigned long long)(uint32_t)(h[p + i] + 1) << (16 * i);
        rk[e] = key;
      }
    }
    __syncthreads();
    if (c < n) {
      unsigned long long* ck = keys + (long long)c * E;
      double* cw = wgt + (long long)c * E;
      double nh2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int e = lane; e < off[4]; e += 64) {
        const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
        const unsigned long long key = rk[e];
        int tf = 0, less = 0, before = 0;
        for (int j = off[k]; j < off[k + 1]; ++j) {
          const unsigned long long v = rk[j];
          const bool eq = v == key;
          tf += eq;
          less += v < key;
          before += eq && j < e;
        }
        const long long at = cs_find(t.df_keys, 0, t.n_df, key);
        const double w = (double)tf * (at >= 0 ? t.df_idf[at] : t.idf_absent);
        const int slot = off[k] + less + before;  // < off[k + 1]: less + tf <= the order's count
        ck[slot] = key;
        cw[slot] = w;
        if (before == 0) {
          const double w2 = w * w;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == k) nh2[q] += w2;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double s = sqrt(wave_sum(nh2[k]));
        if (lane == 0) norm[4 * c + k] = s;
      }
      if (lane == 0) clen[c] = L;
    }
    __syncthreads();
  }

  // ---- phase 2: a wave per hypothesis, the references in ascending order
  for (int s = wave; s < n; s += CS_WAVES) {
    const int Ls = clen[s];
    int off[5];
    off[0] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + max(Ls - k, 0);
    const unsigned long long* sk = keys + (long long)s * E;
    const double* sw = wgt + (long long)s * E;
    double nh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) nh[k] = norm[4 * s + k];
    double num = 0.0, den = 0.0;
    for (int j = 0; j < n; ++j) {
      const int Lj = clen[j];
      double sim = 0.0;
      if (Ls > 0 && Lj > 0) {  // wave-uniform
        int offj[5];
        offj[0] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) offj[k + 1] = offj[k] + max(Lj - k, 0);
        const unsigned long long* jk = keys + (long long)j * E;
        const double* jw = wgt + (long long)j * E;
        double val[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = lane; e < off[4]; e += 64) {
          const int k = (e >= off[1]) + (e >= off[2]) + (e >= off[3]);
          const unsigned long long key = sk[e];
          if (e > off[k] && sk[e - 1] == key) continue;  // a duplicate: counted at its first slot
          const long long at = cs_find(jk, offj[k], offj[k + 1], key);
          const double r = at >= 0 ? jw[at] : 0.0;
          const double term = fmin(sw[e], r) * r;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == k) val[q] += term;
        }
        const int d = abs(max(Ls - 1, 0) - max(Lj - 1, 0));  // the host's "length": the bigram count
        const double g = t.gauss[min(d, t.n_gauss - 1)];
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k] = wave_sum(val[k]);
          const double nr = norm[4 * j + k];
          if (nh[k] != 0.0 && nr != 0.0) v[k] /= nh[k] * nr;
          v[k] *= g;
        }
        sim = (((v[0] + v[1]) + v[2]) + v[3]) / 4.0 * 10.0;
      }
      if (pair && lane == 0) pair[(row0 + s) * n + j] = sim;
      if (j != s) {
        const double p = weight ? weight[row0 + j] : 1.0;
        num += p * sim;
        den += p;
      }
    }
    if (lane == 0) {
      const double u = den != 0.0 ? num / den : 0.0;
      ut[s] = u;
      util[row0 + s] = u;
    }
  }
  __syncthreads();

  // ---- phase 3: the greatest utility, ties to the lowest index
  if (threadIdx.x == 0) {
    int best = 0;
    for (int s = 1; s < n; ++s)
      if (ut[s] > ut[best]) best = s;
    pick[img] = best;
  }
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_ciderd_consensus(const fpnmt_cider_tables* t, int images, int n, const int32_t* hist, int hist_ld,
                           const int32_t* len, const int32_t* fin, const double* weight, double* util, int32_t* pick,
                           double* pair, fpnmt_stream_t stream) {
  if (!t || !hist || !len || !fin || !util || !pick) return fail(FPNMT_E_ARG, "ciderd_consensus: null pointer");
  if (!t->df_keys || !t->df_idf || !t->gauss) return fail(FPNMT_E_ARG, "ciderd_consensus: null table pointer");
  if (images < 0 || n < 1) return fail(FPNMT_E_ARG, "ciderd_consensus: images < 0 / n < 1");
  if (hist_ld < 1 || t->n_df < 0 || t->n_gauss < 1 || t->max_len < 1)
    return fail(FPNMT_E_ARG, "ciderd_consensus: hist_ld < 1 / negative table size / n_gauss < 1 / max_len < 1");
  if (n > FPNMT_CONSENSUS_MAX_CANDS)
    return fail(FPNMT_E_UNSUPPORTED, "ciderd_consensus: n = " + std::to_string(n) + " candidates per image, at most " +
                                         std::to_string(FPNMT_CONSENSUS_MAX_CANDS));
  if (t->max_len > FPNMT_CIDER_MAX_LEN || hist_ld - 1 > t->max_len)
    return fail(FPNMT_E_UNSUPPORTED, "ciderd_consensus: captions of up to hist_ld - 1 = " +
                                         std::to_string(hist_ld - 1) + " tokens exceed the tables' max_len " +
                                         std::to_string(t->max_len) + " (at most " +
                                         std::to_string(FPNMT_CIDER_MAX_LEN) + ")");
  if ((long long)images * n > 0x7fffffffll) return fail(FPNMT_E_UNSUPPORTED, "ciderd_consensus: images * n >= 2^31");
  const int E = cs_entries(min(hist_ld - 1, t->max_len));
  const long long bytes = cs_lds_bytes(n, E);
  if (bytes > CS_LDS_BYTES)
    return fail(FPNMT_E_UNSUPPORTED,
                "ciderd_consensus: n = " + std::to_string(n) + " candidates of up to " +
                    std::to_string(min(hist_ld - 1, t->max_len)) + " tokens need " + std::to_string(bytes) +
                    " bytes of LDS (16 n E + 64 E + 44 n at E = " + std::to_string(E) +
                    " n-gram entries per candidate), above the " +
                    std::to_string(CS_LDS_BYTES) + " of a work-group");
  if (images == 0) return 0;
  static long long granted = 32 * 1024;  // larger launches raise the kernel's dynamic LDS bound first
  if (bytes > granted) {
    if (hipFuncSetAttribute((const void*)ciderd_consensus_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FPNMT_E_HIP, "ciderd_consensus: cannot reserve LDS for the candidates' keys");
    }
    granted = bytes;
  }
  hipLaunchKernelGGL(ciderd_consensus_kernel, dim3((unsigned)images), dim3(CS_THREADS), (size_t)bytes, S(stream), *t,
                     n, E, hist, hist_ld, len, fin, weight, util, pick, pair);
  return check_launch("ciderd_consensus");
}

}  // extern "C"

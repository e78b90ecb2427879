// Constrained caption decoding: one launch that rewrites the fp32 logits of a
// decode position in place, between the decoder's last GEMM and the step
// kernel (fpnmt_beam_step_log / fpnmt_sample_step), from the rows' token
// history on the device: no-repeat n-gram blocking, a repetition penalty, a
// minimum length and a banned list. Both step kernels already give a -inf
// logit its meaning (weight 0 / exp(-inf - max) = 0 and a -inf candidate), so
// a ban is a store of -inf and nothing else in the step changes.
//
// One wave per row, CN_ROWS rows per block; the row's history h[0..t] is
// staged in LDS with every id outside [0, vocab) replaced by -1, which the
// phases below skip: such an id matches nothing and no address is formed from
// it. The kernel touches at most t + 1 + n_banned + 1 logits of a row, never
// the vocabulary. Phases, separated by block barriers (their trip counts are
// functions of the kernel arguments, so every wave reaches every barrier):
//   1. stage: lane i % 64 loads h[i];
//   2. penalty: the lane that holds position i scans h[0..i) and applies the
//      penalty only when h[i] does not occur there — the FIRST occurrence
//      owns the token, so a token that occurs several times is penalised
//      exactly once and no two lanes write the same logit;
//   3. bans, after the penalty: n-gram (lane i compares the g - 1 tokens from
//      h[i] with the last g - 1 and bans h[i + g - 1]), the list, <end> below
//      the minimum length. A ban overwrites a penalised value, so a token
//      that is both ends at -inf; several lanes may store the same -inf.
// All stores are plain vector stores by the row's own wave.
#include "common.h"
#include <math.h>

namespace fpnmt {
namespace {

constexpr int CN_ROWS = 4;  // waves (rows) per block

__global__ __launch_bounds__(CN_ROWS * 64) void logits_constrain_kernel(
    int rows, int vocab, float* __restrict__ logits, long long ldl, const int32_t* __restrict__ hist, int hist_ld,
    int t, const int32_t* __restrict__ fin, int g, float p, int min_len, int end_token,
    const int32_t* __restrict__ banned, int n_banned) {
  __shared__ int32_t sh[CN_ROWS][FPNMT_CONSTRAIN_MAX_LEN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * CN_ROWS + wave;
  // wave-uniform; a finished row is neither read nor written (its wave only keeps the barriers)
  const bool on = r < rows && !(fin && fin[r] != 0);
  int32_t* h = sh[wave];
  float* l = logits + (long long)(on ? r : 0) * ldl;
  if (on) {
    const int32_t* hr = hist + (long long)r * hist_ld;
    for (int i = lane; i <= t; i += 64) {
      const int32_t v = hr[i];
      h[i] = (v >= 0 && v < vocab) ? v : -1;
    }
  }
  __syncthreads();
  if (on && p != 1.f) {
    for (int i = lane; i <= t; i += 64) {
      const int32_t j = h[i];
      if (j < 0) continue;
      bool first = true;
      for (int k = 0; k < i; ++k) first = first && h[k] != j;  // k is the same across the lanes: LDS broadcast
      if (!first) continue;
      const float v = l[j];
      if (v == v) l[j] = v > 0.f ? v / p : v * p;  // a NaN keeps its bits
    }
  }
  __syncthreads();  // the bans follow the penalty
  if (!on) return;
  if (g > 0 && g <= t + 1) {
    const int tail = t - g + 2;  // h[tail .. t]: the g - 1 tokens before the one being chosen
    for (int i = lane; i <= t - g + 1; i += 64) {
      bool match = true;
      for (int k = 0; k < g - 1; ++k) {
        const int32_t a = h[i + k];
        match = match && a >= 0 && a == h[tail + k];
      }
      const int32_t j = h[i + g - 1];
      if (match && j >= 0) l[j] = -INFINITY;
    }
  }
  for (int k = lane; k < n_banned; k += 64) {
    const int32_t j = banned[k];
    if (j >= 0 && j < vocab) l[j] = -INFINITY;
  }
  if (lane == 0 && t < min_len) l[end_token] = -INFINITY;
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_logits_constrain(int rows, int vocab, float* logits, long long ldl, const int32_t* hist, int hist_ld, int t,
                           const int32_t* fin, int no_repeat_ngram, float repetition_penalty, int min_len,
                           int end_token, const int32_t* banned, int n_banned, fpnmt_stream_t stream) {
  if (!logits || !hist) return fail(FPNMT_E_ARG, "logits_constrain: null pointer");
  if (rows <= 0) return fail(FPNMT_E_ARG, "logits_constrain: rows <= 0");
  if (vocab <= 0 || ldl < vocab) return fail(FPNMT_E_ARG, "logits_constrain: bad vocab, or ldl < vocab");
  if (t < 0 || hist_ld < t + 1) return fail(FPNMT_E_ARG, "logits_constrain: bad position / table width (hist_ld >= t + 1)");
  if (no_repeat_ngram < 0) return fail(FPNMT_E_ARG, "logits_constrain: no_repeat_ngram < 0");
  if (min_len < 0) return fail(FPNMT_E_ARG, "logits_constrain: min_len < 0");
  if (!(repetition_penalty > 0.f) || !isfinite(repetition_penalty))
    return fail(FPNMT_E_ARG, "logits_constrain: repetition_penalty must be a finite positive number");
  if (end_token < 0 || end_token >= vocab)
    return fail(FPNMT_E_ARG, "logits_constrain: end_token outside the vocabulary");
  if (n_banned < 0 || (n_banned > 0 && !banned))
    return fail(FPNMT_E_ARG, "logits_constrain: n_banned < 0, or a null banned list");
  if (t + 1 > FPNMT_CONSTRAIN_MAX_LEN)
    return fail(FPNMT_E_UNSUPPORTED, "logits_constrain: more than 1024 positions (the history row is staged in LDS)");
  if (n_banned > FPNMT_CONSTRAIN_MAX_BANNED) return fail(FPNMT_E_UNSUPPORTED, "logits_constrain: more than 4096 banned ids");
  if (no_repeat_ngram == 0 && repetition_penalty == 1.f && min_len <= t && n_banned == 0) return 0;  // every rule off
  hipLaunchKernelGGL(logits_constrain_kernel, dim3(cdiv(rows, CN_ROWS)), dim3(CN_ROWS * 64), 0, S(stream), rows, vocab,
                     logits, ldl, hist, hist_ld, t, fin, no_repeat_ngram, repetition_penalty, min_len, end_token,
                     banned, n_banned);
  return check_launch("logits_constrain");
}

}  // extern "C"

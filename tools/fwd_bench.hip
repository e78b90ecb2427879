// Forward-conv kernel variants on the ResNet-50-FPN forward shapes at batch
// 64 (the north_star headline), each checked against a naive fp32 reference
// GEMM and timed with HIP events (20 launches after 3 warm-ups). Prints one
// line per (shape, variant): us, TFLOP/s, HBM-floor GB/s (algorithmic bytes:
// x + w + y (+ residual) once), max relative error.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/fwd_bench.hip -o gpurun_out/fwd_bench
//   FB_FILTER=<substring of shape name>  FB_VAR=<substring of variant name>
// Not part of the library.
#define FPNMT_PIPE_ALL_CFGS  // every pipe tile class on the conv operand (psplit: cfg 3 / 4), not only the dispatched ones
#include "../fpn-mt-image-captioning_amd/csrc/gemm_dispatch.h"
#include "gemm_stream.h"
#include "gemm_sk.h"
#include "gemm_wide.h"
#include "gemm_pp.h"
#include "gemm_stream_lw.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <functional>

namespace fpnmt {
SplitWs g_split_ws;
void set_error(const std::string&) {}
int fail(int code, const std::string&) { return code; }
int check_launch(const char*) { return hipGetLastError() == hipSuccess ? 0 : -3; }
int forced_wide_cfg() { return 0; }
bool defer_active() { return false; }
bool wgrad_queue_ok() { return false; }
long long defer_room() { return 0; }
float* defer_alloc(long long) { return nullptr; }
bool defer_owns(const void*) { return false; }
int defer_touch(const void*, const void*, hipStream_t) { return 0; }
int defer_wgrad(const GemmParams&, const float*, int, int, hipStream_t) { return 0; }
void colsum_launch(int, int, const float*, float*, hipStream_t, int, float*) {}
}  // namespace fpnmt
using namespace fpnmt;

struct Shape { const char* name; int n, h, w, c, k, r, stride, res, relu; };

static const void* g_zero = nullptr;
static const void* g_res = nullptr;
static const void* g_m2 = nullptr;

static void setup(GemmParams& p, const Shape& s, const void* x, const void* w, void* y) {
  memset(&p, 0, sizeof(p));
  const int pad = s.r / 2;
  const int ho = s.stride == 1 ? s.h : (s.h + s.stride - 1) / s.stride;
  const int wo = s.stride == 1 ? s.w : (s.w + s.stride - 1) / s.stride;
  p.M = s.n * ho * wo; p.N = s.k; p.K = s.r * s.r * s.c;
  p.A = x; p.B = w; p.C = y; p.ldb = p.K; p.ldc = s.k; p.ldr = s.k;
  p.batch_inner = 1; p.alpha = 1.f;
  p.H = s.h; p.W = s.w; p.Cc = s.c; p.Ho = ho; p.Wo = wo; p.Rk = s.r; p.Sk = s.r; p.sh = p.sw = s.stride;
  p.pt = p.pl = s.stride == 1 ? pad : 0;
  p.fd_HoWo = make_fastdiv(ho * wo); p.fd_Wo = make_fastdiv(wo); p.fd_C = make_fastdiv(s.c); p.fd_S = make_fastdiv(s.r);
  p.fd_sHoWo = p.fd_sWo = make_fastdiv(1);
  p.act = s.relu ? FPNMT_ACT_RELU : FPNMT_ACT_NONE; p.split_k = 1; p.k_per_split = p.K;
  if (s.res) p.R = g_res;
  if (s.res == 2) { p.M2 = g_m2; p.m2_act = FPNMT_ACT_RELU; }  // the identity 2a bwd-data: residual grad + ReLU' mask
  p.zero16 = g_zero;
}

// naive reference: one thread per output element, fp32 accumulation
__global__ void ref_kernel(GemmParams p, float* out) {
  const long long e = blockIdx.x * 256LL + threadIdx.x;
  if (e >= (long long)p.M * p.N) return;
  const int m = (int)(e / p.N), n = (int)(e % p.N);
  const int hw = p.Ho * p.Wo;
  const int img = m / hw, rem = m % hw, ho = rem / p.Wo, wo = rem % p.Wo;
  const bf16* x = (const bf16*)p.A;
  const bf16* w = (const bf16*)p.B + (long long)n * p.K;
  float acc = 0.f;
  for (int r = 0; r < p.Rk; ++r)
    for (int s = 0; s < p.Sk; ++s) {
      const int hi = ho * p.sh - p.pt + r, wi = wo * p.sw - p.pl + s;
      if (hi < 0 || hi >= p.H || wi < 0 || wi >= p.W) continue;
      const bf16* xr = x + (((long long)img * p.H + hi) * p.W + wi) * p.Cc;
      const bf16* wr = w + (r * p.Sk + s) * p.Cc;
      for (int c = 0; c < p.Cc; ++c) acc += (float)xr[c] * (float)wr[c];
    }
  if (p.R) acc += (float)((const bf16*)p.R)[(long long)m * p.ldr + n];
  if (p.act == FPNMT_ACT_RELU) acc = fmaxf(acc, 0.f);
  if (p.M2 && !((float)((const bf16*)p.M2)[(long long)m * p.ldr + n] > 0.f)) acc = 0.f;
  out[e] = acc;
}

__global__ void diff_kernel(const bf16* y, const float* ref, long long n, float* out2) {
  __shared__ float smax[256], sref[256];
  float md = 0.f, mr = 0.f;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += 256LL * gridDim.x) {
    md = fmaxf(md, fabsf((float)y[i] - ref[i]));
    mr = fmaxf(mr, fabsf(ref[i]));
  }
  smax[threadIdx.x] = md; sref[threadIdx.x] = mr;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256; ++i) { md = fmaxf(md, smax[i]); mr = fmaxf(mr, sref[i]); }
    atomicMax((int*)&out2[0], __float_as_int(md));
    atomicMax((int*)&out2[1], __float_as_int(mr));
  }
}

template <int BM, int BN, int WM, int WN, int NT, int STAGES, int EPI = 1, int BK = 64, int SPREAD = 0, int MF = 32>
static void pipe(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + BM - 1) / BM; p.tiles_n = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_pipe_kernel<BM, BN, WM, WN, A_IM2COL, NT, STAGES, EPI, BK, SPREAD, MF>),
                     dim3(p.tiles_m * p.tiles_n, 1, 1), dim3(NT), 0, st, p);
}
template <int BM, int BN, int WM, int WN, int ST>
static void wide(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + BM - 1) / BM; p.tiles_n = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_wide_kernel<BM, BN, WM, WN, A_IM2COL, ST>), dim3(p.tiles_m * p.tiles_n, 1, 1),
                     dim3(64 * WM * WN), 0, st, p);
}
template <int BM, int BN, int WM, int WN, int BK>
static void reg(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + BM - 1) / BM; p.tiles_n = (p.N + BN - 1) / BN;
  p.k_per_split = ((p.K + BK - 1) / BK) * BK;
  hipLaunchKernelGGL((gemm_kernel<bf16, BM, BN, WM, WN, A_IM2COL, B_NK, true, BK>), dim3(p.tiles_m * p.tiles_n, 1, 1),
                     dim3(64 * WM * WN), 0, st, p);
}

template <int BM, int BN, int WM, int WN, int MF = 32>
static void pp(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + BM - 1) / BM; p.tiles_n = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_pp_kernel<BM, BN, WM, WN, A_IM2COL, MF>), dim3(p.tiles_m * p.tiles_n, 1, 1), dim3(512), 0,
                     st, p);
}

// the loader-wave kernel (csrc/gemm_pipe.h gemm_pipe_lw_kernel; PRIO: the
// round-6 probe's s_setprio placements, measured equal and dropped)
template <int BM, int BN, int WM, int WN, int NLW, int ST, int PRIO>
static void lw(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + BM - 1) / BM; p.tiles_n = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_pipe_lw_kernel<BM, BN, WM, WN, A_IM2COL, NLW, ST>), dim3(p.tiles_m * p.tiles_n, 1, 1),
                     dim3(64 * (WM * WN + NLW)), 0, st, p);
}

static bool g_skip = false;
// the library's streaming loader-wave kernel for the short-K 1x1 convs
static void stream_lib(GemmParams p, hipStream_t st) {
  if (!stream_eligible(p, 1, A_IM2COL)) { g_skip = true; return; }
  launch_stream(p, A_IM2COL, st);
}
template <int ST, int NLW, int BM>
static void stream_v(GemmParams p, hipStream_t st) {
  if (!stream_eligible(p, 1, A_IM2COL) || p.K != 64) { g_skip = true; return; }
  p.lda = p.Cc; p.zero16 = g_zero;
  if (p.M2) launch_stream_k<64, true, true, ST, NLW, BM>(p, st);
  else launch_stream_k<64, true, false, ST, NLW, BM>(p, st);
}
#if defined(FB_SPREAD)
// the dispatch's stream-K launcher (skips shapes it would not take)
static void sk(GemmParams p, hipStream_t st) {
  int rc = 0;
  if (!launch_pipe_sk<A_IM2COL>(p, 1, 1, st, &rc)) g_skip = true;
}
// the stream-K kernel with one block per tile (no split tiles: its loop and
// epilogue without the slab hand-off)
static void sk_whole(GemmParams p, hipStream_t st) {
  p.tiles_m = (p.M + 127) / 128; p.tiles_n = (p.N + 255) / 256;
  p.split_k = 1; p.k_per_split = p.K; p.ws_part = g_split_ws.part; p.ws_cnt = g_split_ws.cnt;
  hipLaunchKernelGGL((gemm_pipe_sk_kernel<128, 256, 2, 4, A_IM2COL, 512, 3>), dim3(p.tiles_m * p.tiles_n), dim3(512), 0,
                     st, p);
}
#endif
// weight-stationary streaming kernel (1x1 stride-1 convs with N, K fixed by
// the template): BPC blocks per CU, persistent
template <int BM, int N, int K, int WM, int WN, int BPC>
static void stream(GemmParams p, hipStream_t st) {
  if (p.Rk != 1 || p.Sk != 1 || p.sh != 1 || p.sw != 1 || p.N != N || p.K != K) { g_skip = true; return; }
  p.lda = p.Cc;
  const int tiles = (p.M + BM - 1) / BM;
  const int grid = tiles < 256 * BPC ? tiles : 256 * BPC;
  hipLaunchKernelGGL((gemm_stream_kernel<BM, N, K, WM, WN>), dim3(grid), dim3(64 * WM * WN), 0, st, p);
}
#if !defined(FB_LIGHT) && !defined(FB_SPREAD) && !defined(FB_LW) && (!defined(FB_TILE) || defined(FB_STREAM))
static void lib(GemmParams p, hipStream_t st) { dispatch_gemm_impl<bf16>(p, 1, A_IM2COL, B_NK, true, st); }
template <int CFG, int S>
static void psplit(GemmParams p, hipStream_t st) {
  launch_pipe_plan<A_IM2COL>(pipe_plan_split(CFG, S, p), p, 1, st);
}
#endif

struct Var { const char* name; int bn; std::function<void(GemmParams, hipStream_t)> fn; };

int main() {
  std::vector<Shape> shapes = {
      {"r2_a0 1x1 64->64", 64, 56, 56, 64, 64, 1, 1, 0, 1},
      {"r2_a 1x1 256->64", 64, 56, 56, 256, 64, 1, 1, 0, 1},
      {"r2_b 3x3 64->64", 64, 56, 56, 64, 64, 3, 1, 0, 1},
      {"r2_c 1x1 64->256 +R", 64, 56, 56, 64, 256, 1, 1, 1, 1},
      {"r2_sc 1x1 64->256", 64, 56, 56, 64, 256, 1, 1, 0, 0},
      {"r3_a0 1x1/2 256->128", 64, 56, 56, 256, 128, 1, 2, 0, 1},
      {"r3_sc 1x1/2 256->512", 64, 56, 56, 256, 512, 1, 2, 0, 0},
      {"r3_a 1x1 512->128", 64, 28, 28, 512, 128, 1, 1, 0, 1},
      {"r3_b 3x3 128->128", 64, 28, 28, 128, 128, 3, 1, 0, 1},
      {"r3_c 1x1 128->512 +R", 64, 28, 28, 128, 512, 1, 1, 1, 1},
      {"r4_a0 1x1/2 512->256", 64, 28, 28, 512, 256, 1, 2, 0, 1},
      {"r4_sc 1x1/2 512->1024", 64, 28, 28, 512, 1024, 1, 2, 0, 0},
      {"r4_a 1x1 1024->256", 64, 14, 14, 1024, 256, 1, 1, 0, 1},
      {"r4_b 3x3 256->256", 64, 14, 14, 256, 256, 3, 1, 0, 1},
      {"r4_c 1x1 256->1024 +R", 64, 14, 14, 256, 1024, 1, 1, 1, 1},
      {"r5_a0 1x1/2 1024->512", 64, 14, 14, 1024, 512, 1, 2, 0, 1},
      {"r5_sc 1x1/2 1024->2048", 64, 14, 14, 1024, 2048, 1, 2, 0, 0},
      {"r5_a 1x1 2048->512", 64, 7, 7, 2048, 512, 1, 1, 0, 1},
      {"r5_b 3x3 512->512", 64, 7, 7, 512, 512, 3, 1, 0, 1},
      {"r5_c 1x1 512->2048 +R", 64, 7, 7, 512, 2048, 1, 1, 1, 1},
      {"lat3 1x1 512->256", 64, 28, 28, 512, 256, 1, 1, 0, 0},
      {"lat4 1x1 1024->256", 64, 14, 14, 1024, 256, 1, 1, 0, 0},
      {"lat5 1x1 2048->256", 64, 7, 7, 2048, 256, 1, 1, 0, 0},
      {"P3 3x3 256->256", 64, 28, 28, 256, 256, 3, 1, 0, 1},
      {"P4 3x3 256->256", 64, 14, 14, 256, 256, 3, 1, 0, 1},
      {"P5 3x3 256->256", 64, 7, 7, 256, 256, 3, 1, 0, 1},
      {"C2 P3 3x3 256->256 b32", 32, 28, 28, 256, 256, 3, 1, 0, 1},
      {"b32 r2 3x3 64->64", 32, 56, 56, 64, 64, 3, 1, 0, 1},
      {"b32 r3 3x3 128->128", 32, 28, 28, 128, 128, 3, 1, 0, 1},
      {"b32 r4/P4 3x3 256->256", 32, 14, 14, 256, 256, 3, 1, 0, 1},
      {"b32 r5 3x3 512->512", 32, 7, 7, 512, 512, 3, 1, 0, 1},
      {"b32 FEout 3x3 256->512", 32, 14, 14, 256, 512, 3, 1, 0, 1},
      {"b32 r4c 1x1 256->1024 +R", 32, 14, 14, 256, 1024, 1, 1, 1, 1},
      {"b32 r3c 1x1 128->512 +R", 32, 28, 28, 128, 512, 1, 1, 1, 1},
      {"b32 r2c 1x1 64->256 +R", 32, 56, 56, 64, 256, 1, 1, 1, 1},
      // C3: R101-FPN at 512^2, batch 64 (res4 stage: 23 blocks at 32^2)
      {"c3 r4_a 1x1 1024->256 @32", 64, 32, 32, 1024, 256, 1, 1, 0, 1},
      {"c3 r4_b 3x3 256->256 @32", 64, 32, 32, 256, 256, 3, 1, 0, 1},
      {"c3 r4_c 1x1 256->1024 +R @32", 64, 32, 32, 256, 1024, 1, 1, 1, 1},
      {"c3 r3_a 1x1 512->128 @64", 64, 64, 64, 512, 128, 1, 1, 0, 1},
      {"c3 r5_a 1x1 2048->512 @16", 64, 16, 16, 2048, 512, 1, 1, 0, 1},
      {"c3 r5_b 3x3 512->512 @16", 64, 16, 16, 512, 512, 3, 1, 0, 1},
      {"c3 P3 3x3 256->256 @64", 64, 64, 64, 256, 256, 3, 1, 0, 1},
      {"b32 r2 dx 1x1 64->256 +R+M2", 32, 56, 56, 64, 256, 1, 1, 2, 0},
      {"b32 r3 dx 1x1 128->512 +R+M2", 32, 28, 28, 128, 512, 1, 1, 2, 0},
      {"b32 r4 dx 1x1 256->1024 +R+M2", 32, 14, 14, 256, 1024, 1, 1, 2, 0},
  };
  std::vector<Var> vars = {
#if defined(FB_LW2)
      // round 6: wave-tile size on the loader-wave wide tiles (LDS fragment
      // reads per MFMA FLOP scale with 1/WTM + 1/WTN: 64x64 wave tiles read
      // as many LDS bytes per K-tile as the MFMAs take cycles)
      {"lw4 128x256 w2x4 s3 (ship)", 256, lw<128, 256, 2, 4, 4, 3, 0>},
      {"lw4 128x256 w2x2 s3", 256, lw<128, 256, 2, 2, 4, 3, 0>},
      {"lw8 128x256 w2x2 s3", 256, lw<128, 256, 2, 2, 8, 3, 0>},
      {"lw4 128x256 w1x4 s3", 256, lw<128, 256, 1, 4, 4, 3, 0>},
      {"lw4 256x128 w2x2 s3", 128, lw<256, 128, 2, 2, 4, 3, 0>},
      {"lw4 256x256 w2x4 s2", 256, lw<256, 256, 2, 4, 4, 2, 0>},
      {"lw8 256x256 w2x4 s2", 256, lw<256, 256, 2, 4, 8, 2, 0>},
      {"lw4 128x128 w1x2 s4", 128, lw<128, 128, 1, 2, 4, 4, 0>},
#elif defined(FB_LW)
      // round 6: loader waves own the LDS-DMA of the ring (tools/gemm_lw.h);
      // the shipped tiles of each shape class for reference
      {"ship mf16 spread+prio 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 2, 16>},
      {"ship mf16 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1, 64, 0, 16>},
      {"ship 64x64 s4 spread", 64, pipe<64, 64, 2, 2, 256, 4, 1, 64, 1>},
      {"ship 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1>},
      {"ship 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0>},
      {"lw4 128x256 s3", 256, lw<128, 256, 2, 4, 4, 3, 0>},
      {"lw8 128x256 s3", 256, lw<128, 256, 2, 4, 8, 3, 0>},
      {"lw4 256x128 s3", 128, lw<256, 128, 4, 2, 4, 3, 0>},
      {"lw4 128x128 s3", 128, lw<128, 128, 2, 2, 4, 3, 0>},
      {"lw4 128x128 s4", 128, lw<128, 128, 2, 2, 4, 4, 0>},
      {"lw4 128x128 s5", 128, lw<128, 128, 2, 2, 4, 5, 0>},
      {"lw2 128x128 s4", 128, lw<128, 128, 2, 2, 2, 4, 0>},
      {"lw2 128x64 s4", 64, lw<128, 64, 2, 2, 2, 4, 0>},
      {"lw2 64x128 s4", 128, lw<64, 128, 2, 2, 2, 4, 0>},
      {"lw2 64x64 s4", 64, lw<64, 64, 2, 2, 2, 4, 0>},
      {"lw4 64x64 s4", 64, lw<64, 64, 2, 2, 4, 4, 0>},
      {"lw1 64x64 s3", 64, lw<64, 64, 2, 2, 1, 3, 0>},
      {"stream lw", 64, stream_lib},
      {"stream k64 bm16 s6 l2", 64, stream_v<6, 2, 16>},
      {"stream k64 bm16 s4 l2", 64, stream_v<4, 2, 16>},
      {"stream k64 bm32 s3 l4", 64, stream_v<3, 4, 32>},
#elif defined(FB_SPREAD)
      // round 4: the next K-tile's DMA issued between the k-steps' MFMAs
      {"big 128x256 w2x4 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1>},
      {"big 128x256 w2x4 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1>},
      {"spread 128x256 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1, 64, 1>},
      {"spread 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 1>},
      {"spread+prio 128x256 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1, 64, 2>},
      {"spread+prio 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 2>},
      {"stream-K 128x256 s3", 256, sk},
      {"stream-K 1 tile/block", 256, sk_whole},
      {"pipe 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1>},
      {"pipe 64x64 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1>},
      {"spread 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1, 64, 1>},
      {"spread 64x64 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1, 64, 1>},
      {"pipe 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1>},
      {"prio 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1, 64, 3>},
      {"prio 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1, 64, 3>},
      {"prio+spread 64x64 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1, 64, 2>},
      {"pipe 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0>},
      {"prio 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0, 64, 3>},
#elif defined(FB_PP)
      // round 5: the 16x16x32 MFMA form of the shipped pipe tiles (MF 16),
      // the widened 16-B epilogue stores (both forms), the ping-pong schedule;
      // FB_SPLIT: the dispatch against split-K of the big tiles (slabs +
      // ordered reduce) on the under-filled K-heavy convs
#if defined(FB_SPLIT)
      {"lib", 64, lib},
      {"split2 cfg3 128x256", 256, psplit<3, 2>},
      {"split3 cfg3 128x256", 256, psplit<3, 3>},
      {"split2 cfg2 64x64s2", 64, psplit<2, 2>},
      {"split2 cfg4 64x64s4", 64, psplit<4, 2>},
      {"split4 cfg4 64x64s4", 64, psplit<4, 4>},
#else
      {"spread+prio 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 2>},
      {"mf16 spread+prio 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 2, 16>},
      {"mf16 spread 128x256 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1, 64, 1, 16>},
      {"mf16 spread+prio 128x256 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1, 64, 2, 16>},
      {"mf16 spread+prio 256x128 s3", 128, pipe<256, 128, 4, 2, 512, 3, 1, 64, 2, 16>},
      {"pp16 128x256 w2x4", 256, pp<128, 256, 2, 4, 16>},
      {"pipe 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1>},
      {"mf16 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1, 64, 0, 16>},
      {"pipe 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1>},
      {"mf16 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1, 64, 0, 16>},
      {"pipe 64x64 s4 spread", 64, pipe<64, 64, 2, 2, 256, 4, 1, 64, 1>},
      {"mf16 64x64 s4 spread", 64, pipe<64, 64, 2, 2, 256, 4, 1, 64, 1, 16>},
      {"pipe 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0>},
      {"mf16 128x64 s1", 64, pipe<128, 64, 4, 1, 256, 1, 1, 64, 0, 16>},
      {"mf16 64x128 s2", 128, pipe<64, 128, 2, 2, 256, 2, 1, 64, 0, 16>},
#endif
#elif defined(FB_STREAM)
      {"lib", 64, lib},
      {"stream 128x256 k64 w2x2 b3", 64, stream<128, 256, 64, 2, 2, 3>},
      {"stream 128x256 k64 w2x2 b2", 64, stream<128, 256, 64, 2, 2, 2>},
      {"stream 64x256 k64 w1x4 b4", 64, stream<64, 256, 64, 1, 4, 4>},
      {"stream 128x64 k64 w4x1 b6", 64, stream<128, 64, 64, 4, 1, 6>},
      {"stream 128x64 k64 w4x1 b3", 64, stream<128, 64, 64, 4, 1, 3>},
      {"stream 64x64 k256 w2x2 b2", 64, stream<64, 64, 256, 2, 2, 2>},
      {"stream 128x64 k256 w4x1 b1", 64, stream<128, 64, 256, 4, 1, 1>},
#elif defined(FB_TILE)
      // round 4: K-tile depth 32 with deeper rings on 256-wide tiles
      {"big 128x256 w2x4 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1>},
      {"big 128x256 w2x4 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1>},
      {"bk32 128x256 w2x4 s4", 256, pipe<128, 256, 2, 4, 512, 4, 1, 32>},
      {"bk32 128x256 w2x4 s6", 256, pipe<128, 256, 2, 4, 512, 6, 1, 32>},
      {"bk32 256x256 w2x4 s3", 256, pipe<256, 256, 2, 4, 512, 3, 1, 32>},
      {"bk32 256x256 w2x4 s4", 256, pipe<256, 256, 2, 4, 512, 4, 1, 32>},
      {"bk32 256x128 w4x2 s4", 128, pipe<256, 128, 4, 2, 512, 4, 1, 32>},
      {"bk32 256x128 w4x2 s6", 128, pipe<256, 128, 4, 2, 512, 6, 1, 32>},
      {"bk32 128x128 w2x2 s4", 128, pipe<128, 128, 2, 2, 256, 4, 1, 32>},
      {"bk32 64x64 w2x2 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1, 32>},
      {"pipe 64x64 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1>},
      {"pipe 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1>},
#elif !defined(FB_LIGHT)
      {"lib", 64, lib},
      {"pipe 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0>},
      {"pipe 128x64 s1 E2", 64, pipe<128, 64, 4, 1, 256, 1, 2>},
      {"pipe 128x64 s2 E2", 64, pipe<128, 64, 4, 1, 256, 2, 2>},
      {"pipe 64x64 s1 E2", 64, pipe<64, 64, 2, 2, 256, 1, 2>},
      {"pipe 64x64 s2 E2", 64, pipe<64, 64, 2, 2, 256, 2, 2>},
      {"pipe 64x64 s4 E2", 64, pipe<64, 64, 2, 2, 256, 4, 2>},
      {"pipe 128x128 s1 E2", 128, pipe<128, 128, 2, 2, 256, 1, 2>},
      {"pipe 64x128 s1 E2", 128, pipe<64, 128, 2, 2, 256, 1, 2>},
      {"big 128x256 w2x4 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1>},
      {"big 128x256 w2x4 s3", 256, pipe<128, 256, 2, 4, 512, 3, 1>},
      {"big 128x256 w2x2 s2", 256, pipe<128, 256, 2, 2, 256, 2, 1>},
      {"big 128x256 w2x2 s3", 256, pipe<128, 256, 2, 2, 256, 3, 1>},
      {"big 128x128 w2x2 s2", 128, pipe<128, 128, 2, 2, 256, 2, 1>},
      {"big 128x128 w2x2 s3", 128, pipe<128, 128, 2, 2, 256, 3, 1>},
      {"big 128x128 w2x2 s4", 128, pipe<128, 128, 2, 2, 256, 4, 1>},
      {"big 128x128 w1x2 s3", 128, pipe<128, 128, 1, 2, 128, 3, 1>},
      {"big 256x128 w2x2 s2", 128, pipe<256, 128, 2, 2, 256, 2, 1>},
      {"big 256x128 w4x2 s2", 128, pipe<256, 128, 4, 2, 512, 2, 1>},
      {"big 256x256 w2x4 s2", 256, pipe<256, 256, 2, 4, 512, 2, 1>},

#else
      {"big 128x256 w2x4 s2", 256, pipe<128, 256, 2, 4, 512, 2, 1>},
      {"pipe 64x64 s1", 64, pipe<64, 64, 2, 2, 256, 1, 1>},
      {"pipe 64x64 s2", 64, pipe<64, 64, 2, 2, 256, 2, 1>},
      {"pipe 64x64 s4", 64, pipe<64, 64, 2, 2, 256, 4, 1>},
      {"pipe 128x64 s1 E0", 64, pipe<128, 64, 4, 1, 256, 1, 0>},
      {"pipe 64x128 s1 E2", 128, pipe<64, 128, 2, 2, 256, 1, 2>},
      {"pipe 128x128 s1 E2", 128, pipe<128, 128, 2, 2, 256, 1, 2>},
      {"pipe 64x64 s2 E2", 64, pipe<64, 64, 2, 2, 256, 2, 2>},
#endif
#if !defined(FB_TILE) && !defined(FB_STREAM) && !defined(FB_SPREAD) && !defined(FB_PP) && !defined(FB_LW)
      {"wide 128x256 w2x2 s3", 256, wide<128, 256, 2, 2, 3>},
      {"wide 128x256 w1x4 s3", 256, wide<128, 256, 1, 4, 3>},
      {"wide 128x128 w2x2 s3", 128, wide<128, 128, 2, 2, 3>},
      {"wide 256x128 w2x2 s3", 128, wide<256, 128, 2, 2, 3>},
#endif
  };





  const size_t maxe = 64ull * 64 * 64 * 512;
  bf16 *x, *w, *y, *res;
  float *ref, *d2;
  hipMalloc(&x, maxe * 2); hipMalloc(&w, 9ull * 2048 * 512 * 2); hipMalloc(&y, maxe * 2); hipMalloc(&res, maxe * 2);
  hipMalloc(&ref, maxe * 4); hipMalloc(&d2, 8);
  std::vector<bf16> hx(maxe);
  for (size_t i = 0; i < maxe; ++i) hx[i] = (bf16)(((i * 2654435761u) % 2001) / 1000.f - 1.f);
  hipMemcpy(x, hx.data(), maxe * 2, hipMemcpyHostToDevice);
  for (size_t i = 0; i < maxe; ++i) hx[i] = (bf16)((((i + 77) * 40503u) % 2001) / 1000.f - 1.f);
  hipMemcpy(res, hx.data(), maxe * 2, hipMemcpyHostToDevice);
  std::vector<bf16> hw(9ull * 2048 * 512);
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = (bf16)(((((i * 97) % 1009) / 1009.f) - 0.5f) * 0.08f);
  hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
  g_res = res;
  {
    bf16* m2;
    hipMalloc(&m2, maxe * 2);
    for (size_t i = 0; i < maxe; ++i) hx[i] = (bf16)((((i + 13) * 2246822519u) % 2001) / 1000.f - 1.f);
    hipMemcpy(m2, hx.data(), maxe * 2, hipMemcpyHostToDevice);
    g_m2 = m2;
  }
  void* zp;
  hipMalloc(&zp, 256);
  hipMemset(zp, 0, 256);
  g_zero = zp;
  {
    void* ws;
    const size_t wsb = 256ull << 20;
    hipMalloc(&ws, wsb);
    hipMemset(ws, 0, wsb);
    g_split_ws.zero = ws;
    g_split_ws.cnt = (unsigned*)((char*)ws + 256);
    g_split_ws.cnt_n = (65536 - 256) / 4;
    g_split_ws.part = (float*)((char*)ws + 65536);
    g_split_ws.part_floats = (wsb - 65536) / 4;
  }
  hipStream_t st; hipStreamCreate(&st);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const char* filt = getenv("FB_FILTER");
  const char* vf = getenv("FB_VAR");
  const int iters = getenv("FB_ITERS") ? atoi(getenv("FB_ITERS")) : 20;
  const bool cold = !getenv("FB_WARM");
  const size_t flush_bytes = 512ull << 20;
  void* flush;
  hipMalloc(&flush, flush_bytes);
  for (auto& s : shapes) {
    if (filt && !strstr(s.name, filt)) continue;
    GemmParams p;
    setup(p, s, x, w, y);
    const long long outs = (long long)p.M * p.N;
    hipLaunchKernelGGL(ref_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p, ref);
    hipStreamSynchronize(st);
    const double flop = 2.0 * p.M * p.N * (double)p.K;
    const double bytes = 2.0 * ((double)s.n * s.h * s.w * s.c + (double)p.N * p.K + (double)outs * (1 + s.res));
    for (auto& v : vars) {
      if (vf && !strstr(v.name, vf)) continue;
      if (v.bn > 64 && v.bn > s.k) continue;  // tile wider than N
      if (p.K % 64 || p.Cc % 64) continue;
      hipMemset(y, 0, outs * 2);
      g_skip = false;
      v.fn(p, st);
      if (g_skip) continue;
      hipMemsetAsync(d2, 0, 8, st);
      hipLaunchKernelGGL(diff_kernel, dim3(1024), dim3(256), 0, st, y, ref, outs, d2);
      float hd[2];
      hipMemcpy(hd, d2, 8, hipMemcpyDeviceToHost);
      for (int i = 0; i < 3; ++i) v.fn(p, st);
      hipStreamSynchronize(st);
      float ms = 0.f;
      for (int i = 0; i < iters; ++i) {
        if (cold) {  // evict L2 / MALL (512 MB written), then re-touch the input as its producer would
          hipMemsetAsync(flush, i & 0xff, flush_bytes, st);
          hipMemcpyAsync(y, x, (size_t)s.n * s.h * s.w * s.c * 2, hipMemcpyDeviceToDevice, st);
        }
        hipEventRecord(e0, st);
        v.fn(p, st);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float t; hipEventElapsedTime(&t, e0, e1);
        ms += t;
      }
      ms /= iters;
      if (hipGetLastError() != hipSuccess) { printf("launch error\n"); return 1; }
      {  // the last timed launch's output against the reference too (replays)
        hipMemsetAsync(d2, 0, 8, st);
        hipLaunchKernelGGL(diff_kernel, dim3(1024), dim3(256), 0, st, y, ref, outs, d2);
        float h2[2];
        hipMemcpy(h2, d2, 8, hipMemcpyDeviceToHost);
        if (h2[0] / h2[1] > hd[0] / hd[1]) hd[0] = h2[0], hd[1] = h2[1];
      }
      printf("%-26s %-26s %8.1f us %7.1f TF %7.0f GB/s  err %.2e%s\n", s.name, v.name, ms * 1e3,
             flop / (ms * 1e-3) / 1e12, bytes / (ms * 1e-3) / 1e9, hd[0] / hd[1], hd[0] / hd[1] > 2e-2 ? "  BAD" : "");
      fflush(stdout);
    }
  }
  return 0;
}

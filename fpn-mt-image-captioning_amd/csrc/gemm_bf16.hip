// bf16 instantiation set of the MFMA GEMM family (see gemm_impl.h).
#include <algorithm>
#include <cstring>
#include <vector>
#include "gemm_dispatch.h"
namespace fpnmt {
int gemm_bf16(GemmParams& p, int batch, int amode, int bmode, bool vec, hipStream_t s) {
  return dispatch_gemm_impl<bf16>(p, batch, amode, bmode, vec, s);
}

static GemmParams slab_view(float* C, int M, int N, int ldc, int splits, const float* col_scale) {
  GemmParams p;
  std::memset(&p, 0, sizeof(p));
  p.M = M;
  p.N = N;
  p.C = C;
  p.ldc = ldc;
  p.batch_inner = 1;
  p.alpha = 1.f;
  p.col_scale = col_scale;
  p.accumulate = 2;
  p.c_f32 = 1;
  p.split_k = splits;
  return p;
}

float* wgrad_slabs(int M, int N, int splits) {
  const GemmParams p = slab_view(nullptr, M, N, N, splits, nullptr);
  return slab_fits(p, 1, splits) ? slab_alloc(p, 1, splits) : nullptr;
}

int wgrad_slabs_reduce(float* C, int M, int N, int ldc, int splits, const float* col_scale, const float* slabs,
                       hipStream_t s) {
  return launch_wgrad_reduce(slab_view(C, M, N, ldc, splits, col_scale), 1, slabs, s);
}

// the flush of the deferred weight-gradient GEMMs (deferred.hip): jobs laid
// out block by block, GEMM_JOBS_PER_LAUNCH per launch
#ifndef FPNMT_JOBS_STAGES
#define FPNMT_JOBS_STAGES 2  // two blocks per CU (64 KB of LDS each): measured 0.23 ms per C2 step faster than 4 stages at one block
#endif
int launch_gemm_jobs(const DefGemmJob* jobs_in, int n, hipStream_t s) {
  // longest reductions first (their tiles dispatch first and the short ones
  // fill in behind them); the jobs of one flush share no destination, so
  // their order is free
  std::vector<DefGemmJob> jobs(jobs_in, jobs_in + n);
  std::stable_sort(jobs.begin(), jobs.end(), [](const DefGemmJob& a, const DefGemmJob& b) { return a.K > b.K; });
  int i = 0;
  while (i < n) {
    GemmJobs J{};
    J.zero = g_split_ws.zero;
    int blocks = 0;
    while (i < n && J.n < GEMM_JOBS_PER_LAUNCH) {
      DefGemmJob q = jobs[i++];
      q.tiles_n = cdiv(q.N, 128);
      q.blk0 = blocks;
      blocks += cdiv(q.M, 128) * q.tiles_n;
      J.j[J.n++] = q;
    }
    hipLaunchKernelGGL((gemm_wg_jobs_kernel<128, 128, 2, 4, FPNMT_JOBS_STAGES>), dim3(blocks), dim3(512), 0, s, J);
    const int st = check_launch("gemm_wg_jobs_kernel");
    if (st) return st;
  }
  return 0;
}

// the flush of the deferred conv weight-gradient GEMMs (deferred.hip): per
// kernel instantiation, longest reduction per block first, WG_JOBS_PER_LAUNCH
// per launch, each job's blocks from a multiple of 8 (the XCD remap of a
// block's index within its job, gemm_pipe_wg_jobs_kernel).
// Ring depths: 128x128 two stages (64 KB, two blocks per CU, as the Dense
// jobs); 128x64 three (72 KB, two blocks); 64x256 two (80 KB, two blocks);
// the 128x256 loader-wave tile (1024 threads, registers at the limit) and
// 256x128 keep their 3-stage ring and one block per CU.
template <int BM, int BN, int WM, int WN, int NLW, int STAGES, int BPC>
static int launch_wg_jobs_t(const WgJobs& J, int blocks, hipStream_t s) {
  hipLaunchKernelGGL((gemm_pipe_wg_jobs_kernel<BM, BN, WM, WN, A_IM2COL_T, NLW, STAGES, BPC>), dim3(blocks),
                     dim3(64 * (WM * WN + NLW)), 0, s, J);
  return check_launch("gemm_pipe_wg_jobs_kernel");
}

int launch_wg_jobs(const DefConvWg* jobs_in, int n, hipStream_t s) {
  static const int tile[WGJ_CLASSES][2] = {{128, 128}, {128, 64}, {64, 256}, {128, 256}, {256, 128}};
  for (int cls = 0; cls < WGJ_CLASSES; ++cls) {
    std::vector<WgJob> jobs;
    for (int i = 0; i < n; ++i)
      if (jobs_in[i].cls == cls) jobs.push_back(jobs_in[i].job);
    std::stable_sort(jobs.begin(), jobs.end(),
                     [](const WgJob& a, const WgJob& b) { return a.k_per_split > b.k_per_split; });
    size_t i = 0;
    while (i < jobs.size()) {
      WgJobs J{};
      J.zero = g_split_ws.zero;
      long long blocks = 0;
      while (i < jobs.size() && J.n < WG_JOBS_PER_LAUNCH) {
        WgJob q = jobs[i];
        const long long nb = (long long)q.tiles_m * q.tiles_n * q.split_k;
        if (J.n > 0 && blocks + nb > (1LL << 30)) break;
        q.blk0 = (int)blocks;
        blocks = (blocks + nb + 7) & ~7LL;
        J.j[J.n++] = q;
        ++i;
      }
      if (FILE* f = gemm_log()) {
        std::fprintf(f, "bf16 a=%d b=%d c=0 M=0 N=0 K=0 batch=1 acc=2 split=0 cfg=%d jobs=%d blocks=%lld tile=%dx%d\n",
                     A_IM2COL_T, B_KN, ROUTE_WG_JOBS, J.n, blocks, tile[cls][0], tile[cls][1]);
        std::fflush(f);
      }
      int st = 0;
      switch (cls) {
        case WGJ_128_128: st = launch_wg_jobs_t<128, 128, 2, 4, 0, 2, 2>(J, (int)blocks, s); break;
        case WGJ_128_64: st = launch_wg_jobs_t<128, 64, 2, 2, 0, 3, 2>(J, (int)blocks, s); break;
        case WGJ_64_256: st = launch_wg_jobs_t<64, 256, 1, 4, 0, 2, 2>(J, (int)blocks, s); break;
        case WGJ_128_256_LW: st = launch_wg_jobs_t<128, 256, 2, 4, 8, 3, 1>(J, (int)blocks, s); break;
        default: st = launch_wg_jobs_t<256, 128, 4, 2, 0, 3, 1>(J, (int)blocks, s); break;
      }
      if (st) return st;
    }
  }
  return 0;
}
}  // namespace fpnmt

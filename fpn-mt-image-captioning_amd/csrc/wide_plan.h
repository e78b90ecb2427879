// The one planner of the wide conv class's grouped launches (host only, no
// device call): where a level list is broken into launches and the M step
// (112 / 128 / 144 rows: tile classes 10 / 6 / 12 of gemm_dispatch.h) of each.
// fpnmt_conv2d_fwd_grouped / _bwd_data_grouped* (api.hip) break their level
// lists by it, wide_cfg (gemm_dispatch.h) picks a launch's tile class by it,
// fpnmt_plan_wide_levels exports it.
//
// Cost model: a wide launch puts one block on each CU (144-156 KB of LDS), so
// its time is the time of one tile times its waves of blocks, and a tile's
// time goes with its rows: cost = MS x ceil(tiles / CUs) "output rows per CU"
// (x a per-class factor), plus WIDE_EXTRA_LAUNCH_ROWS for every launch after
// the first. A launch below the wide class (fewer than 192 tiles of 128x256: a
// tail of small levels on 64x64 tiles) counts as that per-launch term alone.
//
// The break rule without the 144-row step is the earlier one: a level whose
// 128-row tiles would spill at most a quarter of a wave of blocks past a
// multiple of the CU count starts a launch of its own (P3 + P4 of the batch-32
// step fill 245 of 256 CUs; P5..P7 make 262, a second full tile time for 6
// tiles). Such a break is now weighed against ONE launch of both sides at the
// best of the three M steps: at 144 rows the five levels are 233 tiles at
// batch 32 (one wave) and 464 at batch 64 (two waves, against three at 128).
// A launch that the earlier rule does not break keeps its class: the 144-row
// step is only ever taken by a launch merged across such a break.
//
// What a merged launch computes is bitwise what the broken ones computed
// (launch_wide_chained, gemm_dispatch.h: a part that split K on its own keeps
// its chains, its slabs and its ordered reduce), so the plan only moves time.
#pragma once
#include <algorithm>

namespace fpnmt {

constexpr int WIDE_MAX_LEVELS = 6;  // = MAX_GROUPS (gemm_impl.h)

// The constants, from profiles/heads_one_launch/tiles.txt (MI355X, 256 CUs,
// the heads' 3x3 256->256 conv, us per launch).
// The 144-row tile's time per output row against the 128-row tile's, one
// launch of P3 + P4 each (219 tiles of 144 against 245 of 128; batch 64: 437
// against 490, two waves): graph replay 46.88 / 144 against 42.09 / 128 =
// 0.990, batch 64 92.08 / 288 against 81.60 / 256 = 1.003; in the training step
// (cold operands, rocprofv3) 54.5 / 144 against 50.1 / 128 = 0.968 with the
// tail's rows on board. Rows cost the same in both tiles:
constexpr double WIDE_MS144_FACTOR = 1.0;
// A launch more, in output rows per CU of the wide tile: the tail launch that
// a merge removes (P5..P7 on 64x64 loader tiles; its split-K reduce stays
// either way) is 14.4 us in the step against 50.1 / 128 = 0.391 us per row =
// 36.8 rows; at batch 64 (unsplit, graph replay) 15.07 us against 81.60 / 256 =
// 0.319 = 47 rows. The smaller one, so that a merge has to pay for itself:
// batch 32 merges at 144 < 128 + 37, batch 64 at 288 < 256 + 37 (measured:
// 64.4 -> 58.0 us and 99.8 -> 92.8 us per grouped call, forward).
constexpr double WIDE_EXTRA_LAUNCH_ROWS = 37.0;

struct WidePlan {
  int n_launch;
  int levels[WIDE_MAX_LEVELS];       // levels per launch, in order
  int ms[WIDE_MAX_LEVELS];           // its M step, were it a wide-class launch
  long long tiles[WIDE_MAX_LEVELS];  // its tiles at that step (M tiles x N tiles)
};

static inline long long wide_m_tiles(const long long* rows, int n, int ms) {
  long long t = 0;
  for (int i = 0; i < n; ++i) t += (rows[i] + ms - 1) / ms;
  return t;
}

// the wide class's own gate on a launch (pipe_cfg): >= 192 tiles of 128x256
static inline bool wide_class_launch(const long long* rows, int n, long long tn) {
  return wide_m_tiles(rows, n, 128) * tn >= 192;
}

// The M step of one launch over rows[0..n) and its cost in rows per CU. With
// with144 false this is the earlier rule: 112 where it leaves fewer rows per
// CU over the launch's waves of blocks than 128 (ties: 128).
static inline int wide_launch_ms(const long long* rows, int n, long long tn, long long cus, bool with144,
                                 double* cost = nullptr) {
  auto waves = [&](int ms) { return (wide_m_tiles(rows, n, ms) * tn + cus - 1) / cus; };
  int ms = 128;
  double c = 128.0 * waves(128);
  if (112.0 * waves(112) < c) { ms = 112; c = 112.0 * waves(112); }
  if (with144 && 144.0 * WIDE_MS144_FACTOR * waves(144) < c) { ms = 144; c = 144.0 * WIDE_MS144_FACTOR * waves(144); }
  if (cost) *cost = wide_class_launch(rows, n, tn) ? c : 0.0;
  return ms;
}

// the earlier tail rule: the launch that starts at level i ends before the
// first level whose 128-row tiles spill a little past a wave of blocks
static inline int wide_tail_end(const long long* rows, int i, int n, long long tn, long long cus) {
  long long now = 0;
  int e = i;
  for (; e < n && e - i < WIDE_MAX_LEVELS; ++e) {
    const long long after = now + (rows[e] + 127) / 128 * tn;
    if (now > 0 && (after + cus - 1) / cus > (now + cus - 1) / cus && after % cus != 0 && after % cus <= cus / 4) break;
    now = after;
  }
  return e;
}

// rows[0..n): the output rows of each level (n <= WIDE_MAX_LEVELS; the caller
// cuts longer lists), tn: tiles along N (cdiv(N, 256)) x batch, wide_k: the
// reduction is long enough for the wide class (K >= 1024, or class 12 forced),
// forced: fpnmt_set_wide_cfg's value (12: every tail break merged at 144 rows;
// 6 / 10: no merge, the launch's step is the forced one's).
static inline WidePlan wide_plan_levels(const long long* rows, int n, long long tn, bool wide_k, long long cus,
                                        int forced = 0) {
  WidePlan P{};
  n = std::min(n, WIDE_MAX_LEVELS);
  tn = std::max<long long>(tn, 1);
  cus = std::max<long long>(cus, 1);
  const bool may_merge = wide_k && (forced == 0 || forced == 12);
  int i = 0;
  while (i < n) {
    int e = wide_tail_end(rows, i, n, tn, cus);
    bool merged = false;
    double cost;
    wide_launch_ms(rows + i, e - i, tn, cus, false, &cost);
    while (may_merge && e < n) {
      const int e2 = wide_tail_end(rows, e, n, tn, cus);
      if (e2 - i > WIDE_MAX_LEVELS) break;
      double tail, both;
      wide_launch_ms(rows + e, e2 - e, tn, cus, false, &tail);
      const int ms = wide_launch_ms(rows + i, e2 - i, tn, cus, true, &both);
      if (forced != 12 && !(ms == 144 && both < cost + tail + WIDE_EXTRA_LAUNCH_ROWS)) break;
      e = e2;
      cost = both;
      merged = true;
    }
    int ms = wide_launch_ms(rows + i, e - i, tn, cus, merged);
    if (forced == 12) ms = 144;
    else if (forced == 6) ms = 128;
    else if (forced == 10) ms = 112;
    P.levels[P.n_launch] = e - i;
    P.ms[P.n_launch] = ms;
    P.tiles[P.n_launch] = wide_m_tiles(rows + i, e - i, ms) * tn;
    ++P.n_launch;
    i = e;
  }
  return P;
}

}  // namespace fpnmt

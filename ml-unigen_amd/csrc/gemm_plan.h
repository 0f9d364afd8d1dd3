// Which bf16 GEMM kernel a problem runs, as pure functions: plain C++17, no HIP, no globals, no environment, no pointer is
// dereferenced.  gemm_bf16.hip fills a GemmProblem, asks plan_gemm / plan_fused, and launches what the plan says (run_plan /
// launch_p10 there); tests/gemm_plan_dump.cpp compiles this header alone for the host and tests/test_gemm_plan_cpu.py holds its
// answers against tests/golden/gemm_plan.json.  Every threshold below is a measurement: an edit that changes a row of that table
// changes which kernel a projection of the training step runs.
#pragma once
#include <cstdint>

namespace ug_plan {

enum Epi { EPI_BF16 = 0, EPI_F32 = 1, EPI_RESID = 2, EPI_ROPE = 3, EPI_SWIGLU = 4, EPI_SWIGLU_BWD = 5 };    // EPI_ROPE: EPI_BF16 + rotate-half RoPE on the first rope_cols columns (128...320-row kernel only)

constexpr int BM = 128, BN = 128, BK = 64;       // gemm_kernel
constexpr int PBM = 256, PBN = 256, PBK = 32;    // gemm_kernel_p8; gemm_kernel_p10 shares PBN and PBK
constexpr int QBM = 320;                         // tallest gemm_kernel_p10 tile
constexpr int WS_PRIVATE_SLOTS = 768;            // 256 KiB slots of k-slice partials in a ug_handle's scratch (UG_HANDLE_WS_SLOTS)

constexpr int imin(int a, int b) { return a < b ? a : b; }
constexpr int imax(int a, int b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------- policy word of ug_gemm_bf16
constexpr int POLICY_NARROW_EPILOGUE = 0x100, POLICY_ONE_BARRIER = 0x200, POLICY_TWO_BARRIERS = 0x400, POLICY_AUTO_BITS = 0xff;

struct GemmPolicy {
  int policy;              // -1 automatic, else the pinned kernel (include/unigen_hip.h: ug_gemm_bf16)
  bool one_barrier;        // 256x256 kernel: one barrier per k-tile
  bool wide_epilogue;      // 256x256 kernel: LDS-transposed 16-byte stores
};

inline GemmPolicy decode_policy(int policy, bool a_kmajor, bool b_kmajor) {
  GemmPolicy d;
  d.wide_epilogue = !(policy >= 0 && (policy & POLICY_NARROW_EPILOGUE));
  // main loop of the 256x256 kernel: one barrier per k-tile for the weight gradients (both operands through the transposing
  // fragment reads make L half again as long as M: +10..13 %), two for forward and dgrad (short L: one barrier is -2..-3 %)
  d.one_barrier = a_kmajor && b_kmajor;
  if (policy >= 0 && (policy & POLICY_ONE_BARRIER)) d.one_barrier = true;
  if (policy >= 0 && (policy & POLICY_TWO_BARRIERS)) d.one_barrier = false;
  if (policy >= 0) policy &= ~(POLICY_NARROW_EPILOGUE | POLICY_ONE_BARRIER | POLICY_TWO_BARRIERS);
  if (policy == POLICY_AUTO_BITS) policy = -1;
  d.policy = policy;
  return d;
}

// ---------------------------------------------------------------------------------------------- gemm_kernel_p10 tile heights
// The one table of the 128 ... 320 x 256 kernel: a tile of `h` rows is gemm_kernel_p10<EPI, BKM, p10_f0(h), p10_f1(h)> (the two
// wave groups' 16-row blocks per wave), and each epilogue instantiates exactly the heights of its list.
constexpr int p10_f0(int h) { return (h / 16 + 1) / 2; }
constexpr int p10_f1(int h) { return (h / 16) / 2; }

template <int... H>
struct HeightList {
  static constexpr int count = sizeof...(H);
  static constexpr int values[sizeof...(H)] = {H...};
};
template <int EPI> struct P10Heights { using type = HeightList<128, 144, 160, 176, 192, 208, 224, 240, 256, 272, 288, 304, 320>; };   // bf16 / residual
template <> struct P10Heights<EPI_ROPE> { using type = HeightList<128, 160, 192, 208, 224, 256, 288, 320>; };
template <> struct P10Heights<EPI_SWIGLU> { using type = HeightList<128, 160, 192, 208, 224, 256, 288, 320>; };
template <> struct P10Heights<EPI_SWIGLU_BWD> { using type = HeightList<128, 160, 192, 208, 224, 256, 272, 288, 320>; };

// ---------------------------------------------------------------------------------------------- ug_gemm_bf16
struct GemmProblem {
  int M, N, K;
  int epilogue;            // EPI_BF16 / EPI_F32 / EPI_RESID
  bool a_kmajor, b_kmajor;
  int beta;
  int64_t ldc, ldr;
  bool bias_aligned8;      // no bias, or one at an address that is a multiple of 8
  bool has_workspace;      // the caller's ug_handle carries scratch for k-slice partials
  int policy;              // decode_policy().policy
  bool heights_on;         // UNIGEN_GEMM_HEIGHTS != 0 (A/B switch)
};

enum GemmKind { KIND_128 = 0, KIND_256 = 1, KIND_256_SLICED = 2, KIND_P10 = 3 };   // gemm_kernel, gemm_kernel_p8, the same with every tile k-sliced, gemm_kernel_p10

struct GemmPlan {
  GemmKind kind = KIND_128;
  bool dbuf = false;                 // KIND_128: two LDS stages
  int height = 0;                    // KIND_P10: tile rows
  int grid_x = 0, grid_y = 1;
  int tiles_m = 0, tiles_n = 0;      // GemmArgs fields of the same names
  int full_tiles = 0, tail_split = 1, tail_private = 1;
  bool uses_workspace = false;       // GemmArgs::tail_ws is the handle's scratch (else null)
  int finish_tiles = 0;              // tiles of the tail_finish launch that follows, or 0 for none
};

inline GemmPlan plan_gemm(const GemmProblem& a) {
  GemmPlan pl;
  const bool ws = a.has_workspace;                                     // k-sliced forms need a handle's scratch
  const int g_tile_policy = a.policy;                                  // per call: -1 auto, see ug_gemm_bf16 in the header
  const int EPI = a.epilogue;
  const bool AK = a.a_kmajor, BKM = a.b_kmajor;
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
  const int tiles = tiles_m * tiles_n;
  int splits = 1;
  if (EPI == EPI_F32 && a.beta == 1 && tiles < 384) {            // wgrad of a small weight: fill the chip along K
    const int nk = (a.K + BK - 1) / BK;
    splits = imin(32, imax(1, 768 / tiles));                       // skinny decode GEMMs (M = 16) get up to 32 slices
    splits = imax(1, imin(splits, nk / 2));
  }
  // Staggered 256x256 kernel when its one-workgroup-per-CU grid quantises well (measured, tools/gemm_bench.py:
  // +8..17 % on the wide shapes; the 294-tile N=1536 shapes lose a half-empty second round and stay on 128x128).
  const int tiles_p8 = ((a.M + PBM - 1) / PBM) * ((a.N + PBN - 1) / PBN);
  const int rounds = (tiles_p8 + 255) / 256;
  const bool p8_fits = (tiles_p8 <= 256) ? (tiles_p8 >= 200) : (4 * tiles_p8 >= 3 * rounds * 256);
  // token-count x 1536 outputs (o / down forward, qkv / o / gate_up dgrad): one round of 320 x 256 tiles instead of 1.15 rounds
  // of 256 x 256 -- also ahead of the k-sliced tail where the contraction is long (down forward 954 -> 1065, gate_up dgrad
  // 1188 -> 1354 TF/s)
  if (!AK && EPI != EPI_F32) {
    const int tiles_q = ((a.M + QBM - 1) / QBM) * (a.N / PBN);
    const bool aligned = a.N % PBN == 0 && a.K % PBK == 0 &&
                         (EPI == EPI_BF16 ? (a.ldc % 8 == 0 && a.bias_aligned8)
                                          : (a.ldc % 4 == 0 && a.ldr % 4 == 0));
    // many rounds: a 320-row tile costs 1.25 x a 256-row one and runs ~7 % more efficiently (fewer LDS and DMA bytes per MFMA);
    // taken when whole rounds come out at least 3 % cheaper (gate_up forward: 14 rounds -> 11 x 1.16 = 12.8: 1240 -> 1322 TF/s)
    const bool fewer_rounds = tiles_p8 >= 1024 && 1.1625f * (float)((tiles_q + 255) / 256) < 0.97f * (float)((tiles_p8 + 255) / 256);
    // Round 4: the same comparison over every tile height -- rounds(h) x t(h), t(h) = 0.35 + 0.00254 h in units of a 256-row tile
    // (from the two measured points t(256) = 1, t(320) = 1.1625).  down dgrad (12 336 x 8 960): 288 rows = 6 rounds x 1.08 against 7
    // rounds of 256 (286 -> 255 us); 9 288 rows: 272; gate_up forward keeps 320 at 12 336 rows and takes 304 at 9 288
    // (tools/gemm_shape_sweep.py agrees with the model's ranking on every shape it changes).
    int hb_multi = 0;
    // One-round launches (round 4): a round takes as long as one tile, so the SMALLEST tile height whose row tiles x column tiles
    // still fit the 256 CUs wins -- 12 336 x 1 536 outputs: 304 rows (246 workgroups) instead of 320 (234); 9 288 rows: 224.
    int hb = 0;
    const bool heights_on = a.heights_on;
    if (aligned && g_tile_policy < 0 && a.N / PBN >= 1 && a.N / PBN <= 64) {
      for (int h_ : P10Heights<EPI_BF16>::type::values) {
        if (!heights_on && h_ != QBM) continue;                  // (round 3's choice: 320 rows or nothing)
        const int64_t wgs = (int64_t)((a.M + h_ - 1) / h_) * (a.N / PBN);
        // (measured down to 78 workgroups: tools/gemm_shape_sweep.py at M = 1 542.)  Few workgroups AND a very long contraction
        // (an lm-head dgrad whose vocabulary is a multiple of 32: >= 2048 k-tiles on < 200 CUs) stay with the k-sliced form
        // below, which cuts every tile along K over the whole chip (measured 632 -> 1 094 TF/s at 174 tiles, K = 159 867)
        if (wgs <= 256) { if (wgs >= 64 && !(a.K / PBK >= 2048 && wgs < 200)) hb = h_; break; }
      }
      if (hb == 256 && p8_fits) hb = 0;                          // (the 256 x 256 kernel's own one-round case)
    }
    if (aligned && g_tile_policy < 0 && heights_on && hb == 0 && tiles_p8 >= 768) {
      constexpr int mheights[] = {176, 192, 208, 224, 240, 272, 288, 304, 320};
      float best = 0.97f * (float)((tiles_p8 + 255) / 256);
      for (int h_ : mheights) {
        const int64_t wgs = (int64_t)((a.M + h_ - 1) / h_) * (a.N / PBN);
        const float cost = (float)((wgs + 255) / 256) * (0.35f + 0.00254f * (float)h_);
        if (cost < best) { best = cost; hb_multi = h_; }
      }
    }
    if (aligned && g_tile_policy >= 40 && g_tile_policy <= 52 && g_tile_policy != 48) hb = 16 * (g_tile_policy - 32);   // forced height (tests, A/B)
    if (hb == 0 && hb_multi != 0) hb = hb_multi;
    if (hb == 0 && aligned && (g_tile_policy == 10 || (g_tile_policy < 0 && !heights_on && fewer_rounds))) hb = QBM;
    if (hb != 0) {
      pl.kind = KIND_P10; pl.height = hb;
      pl.tiles_m = (a.M + hb - 1) / hb; pl.tiles_n = a.N / PBN;
      pl.grid_x = pl.tiles_m * pl.tiles_n;
      return pl;
    }
  }
  // A partial last round of 256x256 tiles is cut along K instead: r = tiles mod 256 leftover tiles x s slices fill
  // the chip once more for 1/s of a tile time (fp32 atomics into a scratch, then tail_finish applies the epilogue).
  int tail_r = 0, tail_s = 1;
  if (!p8_fits && tiles_p8 > 256 && (tiles_p8 % 256) <= 128 && g_tile_policy != 5) {
    const int r = tiles_p8 % 256, nk32 = (a.K + PBK - 1) / PBK;
    int sp = 256 / r;
    // measured with private partials (tools/gemm_bench.py): slices of >= 40 k-tiles and >= 3 slices win (down fwd
    // 856 -> 1073, gate_up dgrad 748 -> ~1000 TF/s); the K = 1536 shapes (<= 24 k-tiles per slice) lose to 128x128
    while (sp > 1 && nk32 / sp < 40) --sp;
    if ((sp >= 3 || g_tile_policy == 6) && sp >= 2 && r * sp <= WS_PRIVATE_SLOTS && ws) { tail_r = r; tail_s = sp; }
  }
  // Small accumulating fp32 outputs (weight gradients of the attention projections: 48 / 36 tiles): cut EVERY tile
  // along K so one round fills the chip, each slice storing a private partial that a finishing pass sums into C.
  // (The same cut with fp32 atomics was 118-316 TF/s, the 128x128 kernel's 4 atomic slices 353: atomics cost more
  // than the GEMM itself at these sizes.)
  {
    const int nk32 = (a.K + PBK - 1) / PBK;
    int sp = 0;
    if (EPI == EPI_F32 && tiles_p8 >= 24 && tiles_p8 <= 128 && a.M >= 512 && a.N >= 512) {
      sp = 256 / tiles_p8;                               // one round
      while (sp > 1 && nk32 / sp < 32) --sp;
    } else if (tiles_p8 >= 24 && tiles_p8 < 200 && nk32 >= 2048) {
      // few output tiles, very long contraction (lm-head dgrad: 96 tiles, K = 159 867): up to three rounds of slices,
      // the count that fills whole rounds best (632 -> 1094 TF/s); up to 199 tiles since round 4 (the pt1 mixed batch's
      // 7 184 head rows = 174 tiles ran 2.7 rounds of 128 x 128 tiles at 817 TF/s)
      float best = (tiles_p8 > 128) ? (float)tiles_p8 / 256.f : 0.f;      // (must beat the unsliced single round)
      for (int c = 2; c <= 8 && tiles_p8 * c <= WS_PRIVATE_SLOTS; ++c) {
        const int items = tiles_p8 * c, r = (items + 255) / 256;
        const float eff = (float)items / (float)(r * 256);
        if (eff > best + 0.01f) { best = eff; sp = c; }
      }
    }
    if (sp >= 2 && tiles_p8 * sp <= WS_PRIVATE_SLOTS && (g_tile_policy < 0 || g_tile_policy == 8) && ws) {
      pl.kind = KIND_256_SLICED;
      pl.tiles_m = (a.M + PBM - 1) / PBM; pl.tiles_n = (a.N + PBN - 1) / PBN;
      pl.full_tiles = 0; pl.tail_split = sp; pl.tail_private = 1;
      pl.uses_workspace = true;
      pl.grid_x = tiles_p8 * sp;
      pl.finish_tiles = tiles_p8;
      return pl;
    }
  }
  if (g_tile_policy == 3 || g_tile_policy == 6 || (g_tile_policy < 0 && (p8_fits || tail_s > 1))) {
    pl.kind = KIND_256;
    pl.tiles_m = (a.M + PBM - 1) / PBM; pl.tiles_n = (a.N + PBN - 1) / PBN;
    pl.full_tiles = tiles_p8 - tail_r; pl.tail_split = tail_s;
    pl.tail_private = 1;                         // private partials beat atomics here too (gate_up dgrad 886 -> see DESIGN)
    pl.uses_workspace = ws;
    pl.grid_x = pl.full_tiles + tail_r * tail_s;
    pl.finish_tiles = tail_s > 1 ? tail_r : 0;
    return pl;
  }
  bool dbuf = (!AK && !BKM && a.K >= 4096);
  if (g_tile_policy == 0) dbuf = true;
  if (g_tile_policy == 2) dbuf = false;
  pl.kind = KIND_128; pl.dbuf = dbuf;
  pl.tiles_m = tiles_m; pl.tiles_n = tiles_n;
  pl.grid_x = tiles; pl.grid_y = splits;
  return pl;
}

// ---------------------------------------------------------------------------------------------- fused-epilogue entries
// Tile height of the fused-epilogue launches (ug_gemm_bf16_swiglu / _qkv_rope / _swiglu_bwd): rounds(h) x t(h) over the heights the
// epilogue instantiates -- or the height ug_gemm_set_fused_tile_height() forces (tests and A/B runs reach every instantiation
// that way; 0 = automatic).  A forced height the epilogue does not instantiate is refused: -1.
template <int... H>
inline int plan_fused_over(HeightList<H...>, int64_t M, int64_t col_tiles, int forced) {
  constexpr int heights[] = {H...};
  if (forced) {
    for (int h_ : heights)
      if (h_ == forced) return forced;
    return -1;
  }
  int hb = heights[sizeof...(H) - 1]; float best = 1e30f;
  for (int h_ : heights) {
    const int64_t wgs = ((M + h_ - 1) / h_) * col_tiles;
    const float cost = (float)((wgs + 255) / 256) * (0.35f + 0.00254f * (float)h_);
    if (cost < best) { best = cost; hb = h_; }
  }
  return hb;
}
inline int plan_fused(int epilogue, int64_t M, int64_t col_tiles, int forced_height) {
  switch (epilogue) {
    case EPI_ROPE: return plan_fused_over(P10Heights<EPI_ROPE>::type{}, M, col_tiles, forced_height);
    case EPI_SWIGLU: return plan_fused_over(P10Heights<EPI_SWIGLU>::type{}, M, col_tiles, forced_height);
    case EPI_SWIGLU_BWD: return plan_fused_over(P10Heights<EPI_SWIGLU_BWD>::type{}, M, col_tiles, forced_height);
    default: return -1;
  }
}

}  // namespace ug_plan

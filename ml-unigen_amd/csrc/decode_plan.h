// Which kernel, workgroup shape and grid a decode launch runs, as pure functions: plain C++17, no HIP, no globals, no environment, no
// pointer is dereferenced and nothing is read but the arguments.  decode.hip and decode_sw.hip check their arguments, ask a plan here
// and launch what it says; tests/decode_plan_dump.cpp compiles this header alone for the host and tests/test_decode_plan_cpu.py holds its
// answers against tests/golden/decode_plan.json, the launches recorded from the host code this was moved out of.  Every threshold below
// is a measurement on MI355X: an edit that changes a row of that table changes what a decode step launches.
#pragma once
#include <cstdint>

namespace ug_plan {

constexpr int DEC_KSLAB = 256;              // contraction columns per k-slab (one weight tile: 16 rows x 256 k)
constexpr int DEC_WGROUP = 16;              // weight rows per group (the MFMA's B columns)
// measured on MI355X (tools/gemv_bench.py): two row groups per wave once there are >= 3000 tiles, else one
constexpr int DEC_RING_KW2_TILES = 3000;
// short contractions: direct loads, deepest per-wave unroll that still leaves >= 2048 waves
constexpr int DEC_GEMV_MIN_WAVES = 2048;
constexpr int DEC_GEMV_MAX_UNROLL = 8;
// workgroup shape (waves, tiles per wave) by the tile count the busiest CU ends up with: one 9-wave x 3-tile workgroup
// per CU for gate_up (27 tile slots for 26.25 tiles per CU), 7 x 2 for down (14 for 13.1), 4 x 1|2 otherwise.  The cost counts 256 CUs
// whatever the device has (a constant of the measurement, not the device's count).  (4, 2) never wins: it costs at least what (4, 1)
// costs and a tie goes to the earlier candidate (tests/test_exact_products_cpu.py) -- it stays in the table as the loop had it.
struct RingCand { int nw, kw; };
constexpr RingCand DEC_RING_CANDS[4] = {{4, 1}, {4, 2}, {7, 2}, {9, 3}};
constexpr int DEC_RING_COST_CUS = 256;
// many k-slabs (down projection: 35): the workgroups of a slab on one XCD -- 8 waves x 2 tiles, chunks x ceil(slabs / 8)
// workgroups per XCD must fit its 32 CUs
// (dealing the nslabs % 8 left-over slabs' workgroups over all XCDs for equal bytes per XCD measured no better: 10.50 vs 10.33 us)
constexpr int DEC_XCD_MIN_SLABS = 16, DEC_XCDS = 8, DEC_XCD_CUS = 32, DEC_XCD_NW = 8, DEC_XCD_KW = 2;
constexpr int DEC_RING_MAX_ROWS1 = 16;      // rows of one row block; two row blocks (17 ... 32 rows): the operand image needs the LDS
// single-writer launches (decode_sw.hip): six waves x one k-slab (a 1536-wide contraction), k-blocks of seven slabs
constexpr int DEC_SW_WAVES = 6, DEC_SW_HIDDEN = DEC_SW_WAVES * DEC_KSLAB, DEC_SW_HEAD_DIM = 128;
constexpr int DEC_KBLOCK_SLABS = 7;
// units per workgroup: one workgroup per CU when the tile budget allows, else as many units as MAXT tiles hold
constexpr int DEC_SW_CAP_GATE_UP = 40;      // five tiles x eight hidden units
constexpr int DEC_SW_CAP_RESID = 8;         // eight weight rows of its one tile
constexpr int DEC_SW_CAP_HEAD = 32;         // two tiles x 16 weight rows
constexpr int DEC_SW_KBLOCK_UNITS = 32;     // two 16-row tiles per workgroup
constexpr int DEC_FINISH_COLS8 = 2048, DEC_FINISH_MAX_COLS = 4096;     // eight | sixteen float4 per lane
// the ordered (deterministic) forms are built for the 1.5B model's slot counts: q/k/v partials of 1536 / 256 k-slabs, down k-blocks
constexpr int DEC_ORD_QKV_SLABS = 6, DEC_ORD_DOWN_KBLOCKS = 5;
constexpr int DEC_XIN_BF16 = 0;             // XIN_BF16 of decode.hip: a finished bf16 operand, the one-wave ring kernel

struct Grid3 { unsigned x = 1, y = 1, z = 1; };
inline int64_t dec_groups(int64_t N) { return (N + DEC_WGROUP - 1) / DEC_WGROUP; }
inline int64_t dec_slabs(int64_t K) { return (K + DEC_KSLAB - 1) / DEC_KSLAB; }

// ---------------------------------------------------------------------------------------------- the clears a launch carries
// every workgroup's share (float4 units; the kernels only multiply)
struct ClearShares { int n0_4, per0, n1_4, per1; };
inline ClearShares clear_shares(int64_t n0, int64_t n1, unsigned nblocks) {
  ClearShares c;
  c.n0_4 = (int)(n0 >> 2); c.n1_4 = (int)(n1 >> 2);
  c.per0 = (int)((c.n0_4 + nblocks - 1) / nblocks); c.per1 = (int)((c.n1_4 + nblocks - 1) / nblocks);
  return c;
}

// ---------------------------------------------------------------------------------------------- ug_decode_gemv*, ug_gemv_bf16 (K >= 256)
// gemv_ring_kernel<RB, KW> (xin == DEC_XIN_BF16: NW = 1, CLR unused) or gemv_ring4_kernel<RB, KW, xin, NW, CLR>
struct RingPlan {
  int RB = 1, KW = 1, NW = 1;
  int xcd_chunks = 0;                  // > 0: the XCD-major grid (8, chunks, ceil(slabs / 8))
  Grid3 grid;
  int block = 64;
  bool CLR = false;
  unsigned nblocks() const { return grid.x * grid.y * grid.z; }
};

inline RingPlan plan_ring4(int xin, int R, int64_t N, int64_t K, bool has_clears) {
  RingPlan pl;
  const int64_t groups = dec_groups(N);
  const int nslabs = (int)dec_slabs(K);
  pl.RB = R <= DEC_RING_MAX_ROWS1 ? 1 : 2;
  if (xin == DEC_XIN_BF16) {
    pl.KW = groups * nslabs >= DEC_RING_KW2_TILES ? 2 : 1;
    pl.grid.x = (unsigned)nslabs; pl.grid.y = (unsigned)((groups + pl.KW - 1) / pl.KW);
    return pl;
  }
  int best = 0;
  int64_t best_cost = INT64_MAX;
  for (int c = 0; c < 4; ++c) {
    const int tiles = DEC_RING_CANDS[c].nw * DEC_RING_CANDS[c].kw;
    if (pl.RB == 2 && DEC_RING_CANDS[c].nw != 4) continue;
    const int64_t blocks = ((groups + tiles - 1) / tiles) * nslabs;
    const int64_t cost = ((blocks + DEC_RING_COST_CUS - 1) / DEC_RING_COST_CUS) * tiles;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  pl.NW = DEC_RING_CANDS[best].nw; pl.KW = DEC_RING_CANDS[best].kw;
  const int slabs_per_xcd = (nslabs + DEC_XCDS - 1) / DEC_XCDS;
  if (pl.RB == 1 && nslabs >= DEC_XCD_MIN_SLABS) {
    const int64_t chunks = (groups + DEC_XCD_NW * DEC_XCD_KW - 1) / (DEC_XCD_NW * DEC_XCD_KW);
    if (chunks * slabs_per_xcd <= DEC_XCD_CUS) { pl.NW = DEC_XCD_NW; pl.KW = DEC_XCD_KW; pl.xcd_chunks = (int)chunks; }
  }
  if (pl.xcd_chunks) { pl.grid.x = DEC_XCDS; pl.grid.y = (unsigned)pl.xcd_chunks; pl.grid.z = (unsigned)slabs_per_xcd; }
  else { pl.grid.x = (unsigned)nslabs; pl.grid.y = (unsigned)((groups + pl.NW * pl.KW - 1) / (pl.NW * pl.KW)); }
  pl.block = 64 * pl.NW;
  pl.CLR = has_clears;
  return pl;
}

// ---------------------------------------------------------------------------------------------- ug_gemv_bf16
// ring (K >= 256): plan_ring4(DEC_XIN_BF16) without clears.  Direct: gemv_kernel<RB, U>, four k-slices of 32 U columns per workgroup.
struct GemvPlan {
  bool ring = false;
  int RB = 1, U = 0, KW = 0;
  Grid3 grid;
  int block = 256;
};

inline GemvPlan plan_gemv(int R, int64_t N, int64_t K) {
  GemvPlan pl;
  if (K >= DEC_KSLAB) {
    const RingPlan r = plan_ring4(DEC_XIN_BF16, R, N, K, false);
    pl.ring = true; pl.RB = r.RB; pl.KW = r.KW; pl.grid = r.grid; pl.block = r.block;
    return pl;
  }
  const int64_t groups = dec_groups(N);
  int U = DEC_GEMV_MAX_UNROLL;
  while (U > 1 && groups * ((K + 32 * U - 1) / (32 * U)) < DEC_GEMV_MIN_WAVES) U >>= 1;
  const int64_t nslices = (K + 32 * U - 1) / (32 * U);
  pl.RB = R <= DEC_RING_MAX_ROWS1 ? 1 : 2; pl.U = U;
  pl.grid.x = (unsigned)groups; pl.grid.y = (unsigned)((nslices + 3) / 4);
  return pl;
}

// ug_gemv_bf16_ord: one wave per (k-slab, 16 weight rows), slot = k-slab.  ug_decode_gemv_resid_norm_ord: four waves x one group.
inline Grid3 gemv_ord_grid(int64_t N, int64_t K) {
  Grid3 g;
  g.x = (unsigned)dec_slabs(K); g.y = (unsigned)dec_groups(N);
  return g;
}
inline RingPlan plan_resid_norm_ord(int64_t N, int64_t K) {
  RingPlan pl;
  pl.NW = 4; pl.block = 64 * pl.NW;
  pl.grid.x = (unsigned)dec_slabs(K); pl.grid.y = (unsigned)((dec_groups(N) + pl.NW - 1) / pl.NW);
  return pl;
}

// ---------------------------------------------------------------------------------------------- finishers, fused cache attention
inline int finish_vectors(int64_t cols) { return cols <= DEC_FINISH_COLS8 ? 8 : 16; }     // float4 per lane (cols <= DEC_FINISH_MAX_COLS)

// (XCD-aware placement: see attn_decode_fused_kernel)
inline Grid3 attn_decode_fused_grid(int64_t rows, int H, int HKV) {
  Grid3 g;
  g.x = 8u; g.y = (unsigned)(H / HKV); g.z = (unsigned)((rows * HKV + 7) / 8);
  return g;
}

// ---------------------------------------------------------------------------------------------- decode_sw.hip
inline bool decode_sw_supported(int64_t hidden, int64_t inter, int64_t q_dim, int head_dim) {
  return hidden == DEC_SW_HIDDEN && q_dim == DEC_SW_HIDDEN && inter > 0 && head_dim == DEC_SW_HEAD_DIM;
}

enum SwKind { SW_GATE_UP = 0, SW_RESID = 1, SW_HEAD = 2, SW_KBLOCK = 3, SW_KBLOCK_ORD = 4 };

struct SwPlan {
  int upw = 1;                         // units per workgroup (hidden units for SW_GATE_UP, weight rows otherwise)
  Grid3 grid;                          // x: workgroups over the units, y: k-blocks
  int waves = DEC_SW_WAVES;
};

inline SwPlan plan_sw(SwKind kind, int nunits, int64_t K, int ncu) {
  SwPlan pl;
  if (kind == SW_KBLOCK || kind == SW_KBLOCK_ORD) {
    pl.upw = DEC_SW_KBLOCK_UNITS; pl.waves = DEC_KBLOCK_SLABS;
    pl.grid.y = (unsigned)(K / (DEC_KSLAB * DEC_KBLOCK_SLABS));
  } else {
    const int cap = kind == SW_GATE_UP ? DEC_SW_CAP_GATE_UP : kind == SW_RESID ? DEC_SW_CAP_RESID : DEC_SW_CAP_HEAD;
    pl.upw = (nunits + ncu - 1) / ncu;
    if (pl.upw < 1) pl.upw = 1;
    if (pl.upw > cap) pl.upw = cap;
  }
  pl.grid.x = (unsigned)((nunits + pl.upw - 1) / pl.upw);
  return pl;
}

}  // namespace ug_plan

// Launch geometry of ug_head_score (head_score.hip) as pure functions: plain C++17, no HIP, no globals, no environment, no pointer
// is dereferenced.  head_score.hip asks plan_head_score and launches what it says; tests/head_score_plan_dump.cpp compiles this
// header alone for the host and tests/test_head_score_cpu.py checks the cover, the workspace bytes and that the column tiles do
// not move with R.
//
// The grid is row tiles x column tiles, the row tile running fastest: the workgroups that share one 256-entry slice of the table
// are dispatched together, so the slice is read from HBM once and from L2 by the others.  Only the row-tile HEIGHT follows R
// (fewer idle MFMA columns for a handful of rows); the column tile, the k step and the contraction instruction are constants, and
// a workgroup reduces every row on its own, so a row's bits do not depend on R (include/unigen_hip.h: ug_head_score).
#pragma once
#include <cstdint>

namespace ug_plan {

constexpr int HS_BV = 256;          // table entries (columns of the logit matrix) per workgroup: 4 waves x 2 MFMA tiles of 32
constexpr int HS_BK = 32;           // k per staged piece: two mfma_f32_32x32x16_bf16 steps; K % HS_BK == 0 is the entry point's rule
constexpr int HS_BLOCK = 256;
constexpr int HS_PART_BYTES = 16;   // per (column tile, row): fp32 maximum, fp32 sum rescaled to it, int32 first index of it, one spare word
constexpr int HS_FINISH_ROWS = 4;   // rows per workgroup of the finishing launch (64 threads walk one row's tiles, in tile order)

struct HeadScorePlan {
  int br = 0;                       // row-tile height: 32 or 64 (head_score_kernel<1 | 2>)
  int64_t row_tiles = 0, col_tiles = 0;
  int64_t grid = 0;                 // row_tiles * col_tiles workgroups of HS_BLOCK threads; workgroup b: row tile b % row_tiles, column tile b / row_tiles
  int64_t finish_grid = 0;          // workgroups of the finishing launch
  int64_t label_off = 0;            // byte offset of the fp32 [R] label logits behind the partials [col_tiles][R]
  int64_t ws_bytes = 0;
};

// 64 rows from 33 rows on: two workgroups per CU (111 VGPRs + 64 accumulator AGPRs) cover each other's staging latency.  A 128-row
// tile halves the table's L2 reads per MFMA but runs one wave per SIMD with nothing to cover its loads: 4.08 ms against 3.3 .. 3.4 ms at
// R = 4096, V = 159 867 (profiles/head_score.md).
inline int head_score_row_tile(int64_t R) { return R <= 32 ? 32 : 64; }

// workgroup b of the grid -> its row tile and its column tile (constexpr: the kernel calls them too)
constexpr int64_t head_score_wg_row_tile(int64_t b, int64_t row_tiles) { return b % row_tiles; }
constexpr int64_t head_score_wg_col_tile(int64_t b, int64_t row_tiles) { return b / row_tiles; }

inline HeadScorePlan plan_head_score(int64_t R, int64_t V) {
  HeadScorePlan pl;
  if (R < 1 || V < 1) return pl;
  pl.br = head_score_row_tile(R);
  pl.row_tiles = (R + pl.br - 1) / pl.br;
  pl.col_tiles = (V + HS_BV - 1) / HS_BV;
  pl.grid = pl.row_tiles * pl.col_tiles;
  pl.finish_grid = (R + HS_FINISH_ROWS - 1) / HS_FINISH_ROWS;
  pl.label_off = pl.col_tiles * R * HS_PART_BYTES;
  pl.ws_bytes = pl.label_off + R * 4;
  return pl;
}

}  // namespace ug_plan

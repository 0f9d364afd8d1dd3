// Launch geometry and workspace layout of ug_beam_candidates and ug_beam_kv_reorder (beam.hip) as pure functions: plain C++17, no
// HIP, no globals, no environment, no pointer is dereferenced.  beam.hip asks the plan and launches what it says;
// tests/beam_plan_dump.cpp compiles this header alone for the host and tests/test_beam_search_cpu.py checks the limits, the grids
// and that the workspace covers everything the kernels index.
//
// ug_beam_candidates is four launches behind one clear of the zeroed part of the workspace:
//   count    grid (segments, rows): the row's histogram over the 65536 bf16 patterns (integer atomics: counts have no order)
//   select   one workgroup per row on its histogram: lse, the threshold total, how many candidates tie with it
//   collect  grid (segments, rows): every entry above the threshold (and the ties, when they all fit) into the row's list
//   merge    one workgroup per group: ties by index when they do not all fit, then the B lists ranked by (total, flat index)
// A row is read twice (count, collect); the lists hold at most K entries per row.
#pragma once
#include <cstdint>

namespace ug_plan {

constexpr int BEAM_MAX_B = 8;             // beams per group
constexpr int BEAM_MAX_ROWS = 32;         // G * B
constexpr int BEAM_MAX_K = 64;            // candidates per group; also the capacity of a row's list
constexpr int BEAM_MAX_V = 262144;
constexpr int BEAM_BINS = 65536;          // one histogram bin per bf16 pattern
constexpr int BEAM_SEG = 8192;            // entries per workgroup of the count and collect launches
constexpr int BEAM_SEG_THREADS = 256;
constexpr int BEAM_SELECT_THREADS = 512;  // 128 bins per thread
constexpr int BEAM_MERGE_THREADS = BEAM_MAX_B * BEAM_MAX_K;   // one thread per list slot of a group
constexpr int BEAM_META_INTS = 8;         // per row: lse bits, threshold total bits, flags (bit 0: ties are picked by index), ties
                                          // wanted, entries above the threshold, three spare

struct BeamCandPlan {
  int64_t rows = 0;                       // G * B; 0: outside the limits, no plan
  int64_t segs = 0;                       // count / collect grid: (segs, rows) workgroups of BEAM_SEG_THREADS
  int64_t select_grid = 0;                // rows workgroups of BEAM_SELECT_THREADS
  int64_t merge_grid = 0;                 // G workgroups of BEAM_MERGE_THREADS
  // workspace, byte offsets; [0, zero_bytes) is cleared at the start of every call, the rest is written before it is read
  int64_t hist_off = 0;                   // int32 [rows][BEAM_BINS]
  int64_t count_off = 0;                  // int32 [BEAM_MAX_ROWS]: entries pushed to a row's list
  int64_t zero_bytes = 0;
  int64_t meta_off = 0;                   // int32 [rows][BEAM_META_INTS]
  int64_t list_total_off = 0;             // fp32 [rows][BEAM_MAX_K]
  int64_t list_token_off = 0;             // int32 [rows][BEAM_MAX_K]
  int64_t ws_bytes = 0;
};

constexpr bool beam_cand_in_limits(int64_t G, int64_t B, int64_t V, int64_t K) {
  return G >= 1 && B >= 1 && B <= BEAM_MAX_B && G * B <= BEAM_MAX_ROWS && G <= BEAM_MAX_ROWS && K >= 1 && K <= BEAM_MAX_K && V >= 1 &&
         V <= BEAM_MAX_V;
}

inline BeamCandPlan plan_beam_candidates(int64_t G, int64_t B, int64_t V, int64_t K) {
  BeamCandPlan pl;
  if (!beam_cand_in_limits(G, B, V, K)) return pl;
  pl.rows = G * B;
  pl.segs = (V + BEAM_SEG - 1) / BEAM_SEG;
  pl.select_grid = pl.rows;
  pl.merge_grid = G;
  pl.hist_off = 0;
  pl.count_off = pl.hist_off + pl.rows * BEAM_BINS * 4;
  pl.zero_bytes = pl.count_off + BEAM_MAX_ROWS * 4;
  pl.meta_off = pl.zero_bytes;
  pl.list_total_off = pl.meta_off + pl.rows * BEAM_META_INTS * 4;
  pl.list_token_off = pl.list_total_off + pl.rows * BEAM_MAX_K * 4;
  pl.ws_bytes = pl.list_token_off + pl.rows * BEAM_MAX_K * 4;
  return pl;
}

// ---- ug_beam_kv_reorder: two launches of the same grid.  A lane moves one 16-byte piece of one (layer, cache, row, head, position):
// piece i of grid.x * BEAM_KV_THREADS is head i / (span * 16), position first + (i / 16) % span, 16-byte piece i % 16 of the 256-byte
// head vector; grid.y = rows, grid.z = 2 * n_layers (cache z: layer z >> 1, keys for even z, values for odd z).
constexpr int BEAM_KV_HD = 128;
constexpr int BEAM_KV_PIECES = BEAM_KV_HD * 2 / 16;
constexpr int BEAM_KV_THREADS = 256;
constexpr int BEAM_KV_MAX_LAYERS = 1024;
constexpr int64_t BEAM_KV_MAX_GRID_X = 1 << 20;

struct BeamKvPlan {
  int64_t grid_x = 0, grid_y = 0, grid_z = 0;     // 0: outside the limits
  int64_t pieces = 0;                             // HKV * span * 16: lanes with i >= pieces do nothing
  int64_t spare_bytes = 0;                        // bf16 [2 * n_layers][R][HKV][span][hd]
};

inline BeamKvPlan plan_beam_kv(int64_t n_layers, int64_t R, int64_t HKV, int64_t Tmax, int64_t hd, int64_t first, int64_t span) {
  BeamKvPlan pl;
  if (n_layers < 1 || n_layers > BEAM_KV_MAX_LAYERS || R < 1 || R > BEAM_MAX_ROWS || HKV < 1 || HKV > 1024 || hd != BEAM_KV_HD || first < 0 ||
      span < 1 || Tmax < 1 || Tmax > (1ll << 24) || first > Tmax || span > Tmax || first + span > Tmax)
    return pl;
  pl.pieces = HKV * span * BEAM_KV_PIECES;
  const int64_t gx = (pl.pieces + BEAM_KV_THREADS - 1) / BEAM_KV_THREADS;
  if (gx > BEAM_KV_MAX_GRID_X) return BeamKvPlan();
  pl.grid_x = gx;
  pl.grid_y = R;
  pl.grid_z = 2 * n_layers;
  pl.spare_bytes = 2 * n_layers * R * HKV * span * hd * 2;
  return pl;
}

}  // namespace ug_plan

// Stand-alone host program for tests/test_beam_search_cpu.py: problem rows on stdin, the plans of csrc/beam_plan.h on stdout.
//   cand G B V K
//     -> rows segs select_grid merge_grid hist_off count_off zero_bytes meta_off list_total_off list_token_off ws_bytes
//        BEAM_SEG BEAM_SEG_THREADS BEAM_SELECT_THREADS BEAM_MERGE_THREADS BEAM_BINS BEAM_MAX_K BEAM_MAX_ROWS BEAM_META_INTS
//   kv n_layers R HKV Tmax hd first span
//     -> grid_x grid_y grid_z pieces spare_bytes BEAM_KV_THREADS BEAM_KV_PIECES
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "beam_plan.h"

int main() {
  using namespace ug_plan;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "cand") {
      long long G, B, V, K;
      if (!(in >> G >> B >> V >> K)) return 2;
      const BeamCandPlan pl = plan_beam_candidates(G, B, V, K);
      std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %d\n", (long long)pl.rows, (long long)pl.segs,
                  (long long)pl.select_grid, (long long)pl.merge_grid, (long long)pl.hist_off, (long long)pl.count_off, (long long)pl.zero_bytes,
                  (long long)pl.meta_off, (long long)pl.list_total_off, (long long)pl.list_token_off, (long long)pl.ws_bytes, BEAM_SEG,
                  BEAM_SEG_THREADS, BEAM_SELECT_THREADS, BEAM_MERGE_THREADS, BEAM_BINS, BEAM_MAX_K, BEAM_MAX_ROWS, BEAM_META_INTS);
    } else if (what == "kv") {
      long long n, R, HKV, Tmax, hd, first, span;
      if (!(in >> n >> R >> HKV >> Tmax >> hd >> first >> span)) return 2;
      const BeamKvPlan pl = plan_beam_kv(n, R, HKV, Tmax, hd, first, span);
      std::printf("%lld %lld %lld %lld %lld %d %d\n", (long long)pl.grid_x, (long long)pl.grid_y, (long long)pl.grid_z, (long long)pl.pieces,
                  (long long)pl.spare_bytes, BEAM_KV_THREADS, BEAM_KV_PIECES);
    } else {
      return 2;
    }
  }
  return 0;
}

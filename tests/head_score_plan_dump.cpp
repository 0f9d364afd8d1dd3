// Stand-alone host program for tests/test_head_score_cpu.py: problem rows on stdin, the plans of csrc/head_score_plan.h on stdout.
//   plan R V
//     -> br row_tiles col_tiles grid finish_grid label_off ws_bytes column_tile_width finish_rows part_bytes
//   wgs R V
//     -> for every workgroup of the grid, in order: row_tile col_tile (one line)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "head_score_plan.h"

int main() {
  using namespace ug_plan;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    long long R, V;
    if (!(in >> what)) continue;
    if (!(in >> R >> V)) return 2;
    const HeadScorePlan pl = plan_head_score(R, V);
    if (what == "plan") {
      std::printf("%d %lld %lld %lld %lld %lld %lld %d %d %d\n", pl.br, (long long)pl.row_tiles, (long long)pl.col_tiles, (long long)pl.grid,
                  (long long)pl.finish_grid, (long long)pl.label_off, (long long)pl.ws_bytes, HS_BV, HS_FINISH_ROWS, HS_PART_BYTES);
    } else if (what == "wgs") {
      for (long long b = 0; b < (long long)pl.grid; ++b)
        std::printf("%lld %lld ", (long long)head_score_wg_row_tile(b, pl.row_tiles), (long long)head_score_wg_col_tile(b, pl.row_tiles));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}

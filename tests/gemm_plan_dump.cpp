// Stand-alone host program for tests/test_gemm_plan_cpu.py: problem rows on stdin, the plans of csrc/gemm_plan.h on stdout.
//   gemm M N K epilogue a_kmajor b_kmajor beta has_workspace heights_on policy ldc ldr bias_aligned8
//     -> kind dbuf height f0 f1 grid_x grid_y tiles_m tiles_n full_tiles tail_split tail_private uses_workspace finish_tiles
//        one_barrier wide_epilogue
//   fused epilogue M col_tiles forced_height
//     -> height f0 f1 tiles_m grid_x          (height -1: refused)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gemm_plan.h"

int main() {
  using namespace ug_plan;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "gemm") {
      GemmProblem p{};
      int ak, bk, ws, heights, policy, bias_ok;
      if (!(in >> p.M >> p.N >> p.K >> p.epilogue >> ak >> bk >> p.beta >> ws >> heights >> policy >> p.ldc >> p.ldr >> bias_ok)) return 2;
      p.a_kmajor = ak; p.b_kmajor = bk; p.has_workspace = ws; p.heights_on = heights; p.bias_aligned8 = bias_ok;
      const GemmPolicy d = decode_policy(policy, p.a_kmajor, p.b_kmajor);
      p.policy = d.policy;
      const GemmPlan pl = plan_gemm(p);
      std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)pl.kind, (int)pl.dbuf, pl.height, p10_f0(pl.height), p10_f1(pl.height),
                  pl.grid_x, pl.grid_y, pl.tiles_m, pl.tiles_n, pl.full_tiles, pl.tail_split, pl.tail_private, (int)pl.uses_workspace,
                  pl.finish_tiles, (int)d.one_barrier, (int)d.wide_epilogue);
    } else if (what == "fused") {
      int epi, forced;
      long long M, col_tiles;
      if (!(in >> epi >> M >> col_tiles >> forced)) return 2;
      const int h = plan_fused(epi, M, col_tiles, forced);
      if (h < 0) { std::printf("-1 0 0 0 0\n"); continue; }
      const long long tiles_m = (M + h - 1) / h;
      std::printf("%d %d %d %lld %lld\n", h, p10_f0(h), p10_f1(h), tiles_m, tiles_m * col_tiles);
    } else {
      return 2;
    }
  }
  return 0;
}

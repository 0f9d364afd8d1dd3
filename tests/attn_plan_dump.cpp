// Stand-alone host program for tests/test_attn_plan_cpu.py: problem rows on stdin, the plans of csrc/attn_plan.h on stdout.
//   fwd B L H HKV
//     -> kernel grid block order
//   bwd B L H HKV has_dkv_ws has_rope has_dbias
//     -> dq dq_grid dq_order dq_fused dkv dkv_heads dkv_grid dkv_order finish rpb finish_grid rope_dq colsum_dq rope_dk colsum_dk colsum_dv
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "attn_plan.h"

int main() {
  using namespace ug_plan;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    long long B, L;
    int H, HKV;
    if (!(in >> what)) continue;
    if (!(in >> B >> L >> H >> HKV)) return 2;
    if (what == "fwd") {
      const AttnFwdPlan pl = plan_attn_fwd(B, L, H, HKV);
      std::printf("%d %u %d %d\n", (int)pl.kernel, pl.grid, pl.block, pl.order);
    } else if (what == "bwd") {
      int ws, rope, dbias;
      if (!(in >> ws >> rope >> dbias)) return 2;
      const AttnBwdPlan pl = plan_attn_bwd(B, L, H, HKV, ws != 0, rope != 0, dbias != 0);
      std::printf("%d %u %d %d %d %d %u %d %d %d %u %d %d %d %d %d\n", (int)pl.dq, pl.dq_grid, pl.dq_order, (int)pl.dq_fused, (int)pl.dkv,
                  pl.dkv_heads, pl.dkv_grid, pl.dkv_order, (int)pl.finish, pl.rpb, pl.finish_grid, (int)pl.rope_dq, (int)pl.colsum_dq,
                  (int)pl.rope_dk, (int)pl.colsum_dk, (int)pl.colsum_dv);
    } else {
      return 2;
    }
  }
  return 0;
}

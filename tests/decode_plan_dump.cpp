// Stand-alone host program for tests/test_decode_plan_cpu.py: questions on stdin, the answers of csrc/decode_plan.h on stdout.
//   gemv R N K              -> ring RB U KW grid_x grid_y grid_z block
//   ring xin R N K clears   -> RB KW NW xcd_chunks grid_x grid_y grid_z block CLR
//   gemv_ord N K            -> grid_x grid_y grid_z
//   rn_ord N K              -> RB KW NW xcd_chunks grid_x grid_y grid_z block CLR
//   clear n0 n1 nblocks     -> n0_4 per0 n1_4 per1
//   sw kind nunits K ncu    -> upw grid_x grid_y grid_z waves
//   finish cols             -> float4 per lane
//   attn rows H HKV         -> grid_x grid_y grid_z
//   supported hidden inter q_dim head_dim -> 0 | 1
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "decode_plan.h"

static void put(const ug_plan::RingPlan& p) {
  std::printf("%d %d %d %d %u %u %u %d %d\n", p.RB, p.KW, p.NW, p.xcd_chunks, p.grid.x, p.grid.y, p.grid.z, p.block, (int)p.CLR);
}

int main() {
  using namespace ug_plan;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    long long a[5] = {0, 0, 0, 0, 0};
    if (!(in >> what)) continue;
    int n = 0;
    while (n < 5 && (in >> a[n])) ++n;
    auto need = [&](int k) { return n == k; };
    if (what == "gemv" && need(3)) {
      const GemvPlan p = plan_gemv((int)a[0], a[1], a[2]);
      std::printf("%d %d %d %d %u %u %u %d\n", (int)p.ring, p.RB, p.U, p.KW, p.grid.x, p.grid.y, p.grid.z, p.block);
    } else if (what == "ring" && need(5)) {
      put(plan_ring4((int)a[0], (int)a[1], a[2], a[3], a[4] != 0));
    } else if (what == "gemv_ord" && need(2)) {
      const Grid3 g = gemv_ord_grid(a[0], a[1]);
      std::printf("%u %u %u\n", g.x, g.y, g.z);
    } else if (what == "rn_ord" && need(2)) {
      put(plan_resid_norm_ord(a[0], a[1]));
    } else if (what == "clear" && need(3)) {
      const ClearShares c = clear_shares(a[0], a[1], (unsigned)a[2]);
      std::printf("%d %d %d %d\n", c.n0_4, c.per0, c.n1_4, c.per1);
    } else if (what == "sw" && need(4)) {
      const SwPlan p = plan_sw((SwKind)a[0], (int)a[1], a[2], (int)a[3]);
      std::printf("%d %u %u %u %d\n", p.upw, p.grid.x, p.grid.y, p.grid.z, p.waves);
    } else if (what == "finish" && need(1)) {
      std::printf("%d\n", finish_vectors(a[0]));
    } else if (what == "attn" && need(3)) {
      const Grid3 g = attn_decode_fused_grid(a[0], (int)a[1], (int)a[2]);
      std::printf("%u %u %u\n", g.x, g.y, g.z);
    } else if (what == "supported" && need(4)) {
      std::printf("%d\n", (int)decode_sw_supported(a[0], a[1], a[2], (int)a[3]));
    } else {
      return 2;
    }
  }
  return 0;
}

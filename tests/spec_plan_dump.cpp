// Host program over csrc/spec_plan.h (the rules ug_spec_verify applies on the device), for tests/test_spec_ref_cpu.py.  One case per
// input line, one output line each:
//   A n_draft g[0 .. n_draft] tok[0 .. n_draft]            ->  a
//   E a n_stop stop[0 .. n_stop) emitted width g[0 .. a]    ->  n done
//   D G K n h[0 .. n)                                       ->  ngram start len
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "spec_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char kind = 0;
    in >> kind;
    if (kind == 'A') {
      int nd = 0;
      in >> nd;
      std::vector<int> g(nd + 1);
      std::vector<int64_t> tok(nd + 1);
      for (int& v : g) in >> v;
      for (int64_t& v : tok) in >> v;
      std::printf("%d\n", ug_plan::spec_accept(g.data(), tok.data(), nd));
    } else if (kind == 'E') {
      int a = 0, n_stop = 0, emitted = 0, width = 0;
      in >> a >> n_stop;
      std::vector<int64_t> stop(n_stop + 1);
      for (int i = 0; i < n_stop; ++i) in >> stop[i];
      in >> emitted >> width;
      std::vector<int> g(a + 1);
      for (int& v : g) in >> v;
      const ug_plan::SpecEmit e = ug_plan::spec_emit(g.data(), a, stop.data(), n_stop, emitted, width);
      std::printf("%d %d\n", e.n, e.done);
    } else if (kind == 'D') {
      int G = 0, K = 0, n = 0;
      in >> G >> K >> n;
      std::vector<int> h(n + 1);
      for (int i = 0; i < n; ++i) in >> h[i];
      const ug_plan::SpecDraft d = ug_plan::spec_draft(h.data(), n, G, K);
      std::printf("%d %d %d\n", d.ngram, d.start, d.len);
    } else {
      std::fprintf(stderr, "spec_plan_dump: bad line: %s\n", line.c_str());
      return 1;
    }
    if (!in) {
      std::fprintf(stderr, "spec_plan_dump: short line: %s\n", line.c_str());
      return 1;
    }
  }
  return 0;
}

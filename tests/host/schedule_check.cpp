// schedule_check.cpp — the per-round functions of csrc/ilqg_schedule.hpp on the host alone (plain g++, no HIP):
// tests/test_schedule.py replays the recorded probing rounds of tests/golden/schedule_cases.json through it.
// stdin, one request per line:
//   R probe_max probe_budget deep_rule pairs lane_width pool_entries instances probe_first probe_lanes tail_rounds
//     tail_first deep_in                                         -> "R probe_k deep_out"   (round_probe_candidates)
//   F num_cus pairs lane_width lanes_auto has_lanes has_single probe_lanes instances probe_k -> "F form"  (probe_form)
#include <cstdio>
#include <cstring>

#include "ilqg_schedule.hpp"

int main() {
  char line[512];
  while (std::fgets(line, sizeof(line), stdin)) {
    ilqg::SolveSchedule s{};
    ilqg_solve_options opt;
    std::memset(&opt, 0, sizeof(opt));
    int v[12];
    if (line[0] == 'R') {
      if (std::sscanf(line + 1, "%d %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8,
                      v + 9, v + 10, v + 11) != 12)
        return 2;
      s.probe_max = v[0]; s.probe_budget = v[1]; s.deep_tails = v[2]; s.pairs = v[3]; s.lane_width = v[4];
      opt.probe_first = v[7]; opt.probe_lanes = v[8];
      bool deep = v[11] != 0;
      const int k = ilqg::round_probe_candidates(s, opt, v[5], v[6], v[9], v[10], &deep);
      std::printf("R %d %d\n", k, int(deep));
    } else if (line[0] == 'F') {
      if (std::sscanf(line + 1, "%d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) != 9) return 2;
      s.num_cus = v[0]; s.pairs = v[1]; s.lane_width = v[2]; s.lanes_auto = v[3]; s.proll_lanes = v[4]; s.proll_single = v[5];
      opt.probe_lanes = v[6];
      std::printf("F %d\n", int(ilqg::probe_form(s, opt, v[7], v[8])));
    } else {
      return 2;
    }
  }
  return 0;
}

// expr_check — the expression costs' validator and evaluators (ilqgames_amd/csrc/ilqg_expr.hpp) on the host alone: a plain
// g++ program, no device and no library.  tests/test_expression_cost.py feeds it programs and points and compares what
// it prints with a numpy restatement of the table in include/ilqg.h; the same program is built once with
// -fsanitize=address,undefined (every block sits in a heap allocation of exactly its size, so a validator that read past
// a malformed block would be caught).
//
// stdin, one case per line:   <f32|f64> <two_inputs 0|1> <weight> <value> <nwords> <block words...> <npoints> <x y>...
// stdout per case:            check <fault> <op> <depth>
//   and, for a valid program, per point:   jet f fx fy fxx fyy fxy | grad f fx fy | value f     (hexadecimal floats)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "ilqg_expr.hpp"

template <typename T>
static void run_case(const float* blk, bool /*two*/, double w, double v, const std::vector<double>& pts) {
  for (size_t q = 0; q + 1 < pts.size(); q += 2) {
    const T x = T(pts[q]), y = T(pts[q + 1]);
    T stack[ilqg::kExprStackScalars];
    ilqg::ExprJet<T> full, grad;
    ilqg::expr_eval_jet<T>(blk, T(w), T(v), x, y, true, ilqg::ExprStack<T>{stack, 1}, &full);
    ilqg::expr_eval_jet<T>(blk, T(w), T(v), x, y, false, ilqg::ExprStack<T>{stack, 1}, &grad);
    const T value = ilqg::expr_eval_value<T>(blk, T(w), T(v), x, y);
    std::printf("jet %a %a %a %a %a %a | grad %a %a %a | value %a\n", double(full.f), double(full.fx), double(full.fy),
                double(full.fxx), double(full.fyy), double(full.fxy), double(grad.f), double(grad.fx), double(grad.fy),
                double(value));
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string dtype;
    int two = 0, nwords = 0, npoints = 0;
    double w = 0.0, v = 0.0;
    in >> dtype >> two >> w >> v >> nwords;
    if (!in || nwords < 0) return 2;
    std::unique_ptr<float[]> blk(new float[nwords > 0 ? nwords : 1]);  // exactly the block (one word for an empty one)
    for (int e = 0; e < nwords; e++) {
      std::string tok;
      in >> tok;
      blk[e] = std::strtof(tok.c_str(), nullptr);  // (strtof: "nan" and "inf" are words a malformed block may hold)
    }
    in >> npoints;
    std::vector<double> pts(size_t(npoints > 0 ? npoints : 0) * 2);
    for (double& p : pts) in >> p;
    if (!in) return 2;
    const ilqg::ExprCheck chk = ilqg::expr_validate(nwords > 0 ? blk.get() : nullptr, nwords, two != 0);
    std::printf("check %d %d %d\n", chk.fault, chk.op, chk.depth);
    if (chk.fault != ilqg::EXPR_OK) continue;
    if (dtype == "f32") run_case<float>(blk.get(), two != 0, w, v, pts); else run_case<double>(blk.get(), two != 0, w, v, pts);
  }
  return 0;
}

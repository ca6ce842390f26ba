// expr_dyn_check — the rules of an ILQG_DYN_EXPRESSION subsystem (include/ilqg.h) on the host alone, over the validator and
// the evaluators the kernels run (ilqgames_amd/csrc/ilqg_expr.hpp): a plain g++ program, no device and no library.
// tests/test_expression_dynamics.py feeds it models and points and compares the rates, the linearisation and the RK4 step
// it prints with analytic Jacobians, central differences and a numpy integrator; the same program is built once with
// -fsanitize=address,undefined (every block sits in a heap allocation of exactly its size).
//
// stdin, one model per paragraph:
//   model <xdim> <udim> <param0> <dt>
//   row <X> <Y or -1> <weight> <nwords> <block words...>          (xdim lines, row 0 first)
//   points <npoints>
//   <x (xdim) | u (udim)>                                          (npoints lines)
// stdout per model:   check <row> <fault> <op> <depth>   per row; then, when every row is valid, per point
//   rate <xdim>  |  A <xdim x xdim, row-major>  |  B <xdim x udim, row-major>  |  step <xdim>        (hexadecimal floats)
// Rate: the program's value (expr_eval_value).  A = I + dt J_x, B = dt J_u: the jet without second derivatives, each
// derivative d as double(d) * dt, a diagonal entry 1 + that; a row whose whole program is one PUSH_X is the constant dt.
// Step: MultiPlayerDynamicalSystem::Integrate's RK4 with two half-steps, every operation rounded on its own.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "ilqg_expr.hpp"

namespace {

struct Row {
  int x, y;
  double weight;
  int nwords;
  std::unique_ptr<float[]> blk;  // exactly the block
};

struct Model {
  int xdim = 0, udim = 0;
  double param = 0.0, dt = 0.0;
  std::vector<Row> rows;
};

void rates(const Model& m, const std::vector<double>& xu, std::vector<double>* f) {
  f->assign(size_t(m.xdim), 0.0);
  for (int r = 0; r < m.xdim; r++) {
    const Row& row = m.rows[size_t(r)];
    (*f)[size_t(r)] = ilqg::expr_eval_value<double>(row.blk.get(), row.weight, m.param, xu[size_t(row.x)],
                                                    row.y >= 0 ? xu[size_t(row.y)] : 0.0);
  }
}

void step(const Model& m, std::vector<double> xu, std::vector<double>* out) {
  const int n = m.xdim;
  const double h = m.dt / 2.0;
  std::vector<double> x(xu.begin(), xu.begin() + n), k1, k2, k3, k4;
  for (int s = 0; s < 2; s++) {
    auto at = [&](const std::vector<double>& k, double c, std::vector<double>* f) {
      for (int i = 0; i < n; i++) xu[size_t(i)] = k.empty() ? x[size_t(i)] : x[size_t(i)] + c * k[size_t(i)];
      rates(m, xu, f);
      for (double& v : *f) v = h * v;
    };
    at({}, 0.0, &k1);
    at(k1, 0.5, &k2);
    at(k2, 0.5, &k3);
    at(k3, 1.0, &k4);
    for (int i = 0; i < n; i++) {
      const size_t e = size_t(i);
      x[e] += (k1[e] + 2.0 * (k2[e] + k3[e]) + k4[e]) / 6.0;
    }
  }
  *out = x;
}

void print(const char* tag, const std::vector<double>& v, const char* end) {
  std::printf("%s", tag);
  for (double e : v) std::printf(" %a", e);
  std::printf("%s", end);
}

void run_point(const Model& m, const std::vector<double>& xu) {
  const int n = m.xdim, mu = m.udim;
  std::vector<double> f, A(size_t(n) * n, 0.0), B(size_t(n) * mu, 0.0), next;
  rates(m, xu, &f);
  for (int i = 0; i < n; i++) A[size_t(i) * n + i] = 1.0;
  for (int r = 0; r < n; r++) {
    const Row& row = m.rows[size_t(r)];
    auto entry = [&](int in) -> double& { return in < n ? A[size_t(r) * n + in] : B[size_t(r) * mu + (in - n)]; };
    const bool identity = int(row.blk[0]) == 1 && int(row.blk[1]) == ILQG_EXPR_PUSH_X;
    if (identity && row.x != r) {
      entry(row.x) = m.dt;
      continue;
    }
    double stack[ilqg::kExprStackScalars];
    ilqg::ExprJet<double> j;
    ilqg::expr_eval_jet<double>(row.blk.get(), row.weight, m.param, xu[size_t(row.x)], row.y >= 0 ? xu[size_t(row.y)] : 0.0,
                                false, ilqg::ExprStack<double>{stack, 1}, &j);
    const double dx = double(j.fx) * m.dt, dy = double(j.fy) * m.dt;
    entry(row.x) = row.x == r ? 1.0 + dx : dx;
    if (row.y >= 0) entry(row.y) = row.y == r ? 1.0 + dy : dy;
  }
  step(m, xu, &next);
  print("rate", f, " | ");
  print("A", A, " | ");
  print("B", B, " | ");
  print("step", next, "\n");
}

}  // namespace

int main() {
  std::string line;
  Model m;
  bool valid = true;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string tag;
    in >> tag;
    if (tag == "model") {
      m = Model();
      valid = true;
      in >> m.xdim >> m.udim >> m.param >> m.dt;
      if (!in || m.xdim < 1 || m.xdim > 8 || m.udim < 1 || m.udim > 2) return 2;
    } else if (tag == "row") {
      Row row;
      in >> row.x >> row.y >> row.weight >> row.nwords;
      if (!in || row.nwords < 0 || int(m.rows.size()) >= m.xdim) return 2;
      row.blk.reset(new float[row.nwords > 0 ? row.nwords : 1]);
      for (int e = 0; e < row.nwords; e++) {
        std::string tok;
        in >> tok;
        row.blk[e] = std::strtof(tok.c_str(), nullptr);
      }
      if (!in) return 2;
      const bool inputs = row.x >= 0 && row.x < m.xdim + m.udim && row.y >= -1 && row.y < m.xdim + m.udim && row.x != row.y;
      const ilqg::ExprCheck chk = ilqg::expr_validate(row.nwords > 0 ? row.blk.get() : nullptr, row.nwords, row.y >= 0);
      std::printf("check %d %d %d %d\n", int(m.rows.size()), inputs ? chk.fault : -1, chk.op, chk.depth);
      valid = valid && inputs && chk.fault == ilqg::EXPR_OK;
      m.rows.push_back(std::move(row));
    } else if (tag == "points") {
      int npoints = 0;
      in >> npoints;
      if (!in || int(m.rows.size()) != m.xdim) return 2;
      for (int q = 0; q < npoints; q++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream pin(line);
        std::vector<double> xu(size_t(m.xdim + m.udim));
        for (double& v : xu) pin >> v;
        if (!pin) return 2;
        if (valid) run_point(m, xu);
      }
    } else {
      return 2;
    }
  }
  return 0;
}

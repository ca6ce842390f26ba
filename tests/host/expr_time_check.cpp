// expr_time_check — ILQG_EXPR_PUSH_TIME (include/ilqg.h) on the host alone, over the validator and the evaluators the
// kernels run (ilqgames_amd/csrc/ilqg_expr.hpp): a plain g++ program, no device and no library.
// tests/test_expression_time.py feeds it programs, steps and points and compares what it prints with a numpy restatement
// in which the time leaf is the constant t_k, with central differences, with analytic Jacobians and with a numpy RK4 that
// evaluates its stages at the stage times.
//
// stdin, one paragraph per case.  The time of step k is T(double(k) * dt), of an RK4 stage T(double) of the stage time.
//   jet <f32|f64> <two_inputs 0|1> <weight> <value> <k> <dt> <nwords> <block words...> <npoints> <x y>...
//     -> check <fault> <op> <depth>, and for a valid program per point
//        jet f fx fy fxx fyy fxy | grad f fx fy | value f                                        (hexadecimal floats)
//   model <xdim> <udim> <param0> <dt> <k>
//   row <X> <Y or -1> <weight> <nwords> <block words...>          (xdim lines, row 0 first)
//   points <npoints>
//   <x (xdim) | u (udim)>                                          (npoints lines)
//     -> check <row> <fault> <op> <depth> per row; then, when every row is valid, per point
//        rate <xdim> | A <xdim x xdim, row-major> | B <xdim x udim, row-major> | step <xdim> | euler <xdim>
// Rate, A = I + dt J_x and B = dt J_u are at t_k.  Step: MultiPlayerDynamicalSystem::Integrate's RK4 with two half-steps of
// h = dt / 2, the stages of half-step s at t0, t0 + h/2, t0 + h/2, t0 + h with t0 = k dt + s h.  Euler: x + dt f(t_k, x, u).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "ilqg_expr.hpp"

namespace {

template <typename T>
void run_jet(const float* blk, double w, double v, int k, double dt, const std::vector<double>& pts) {
  const T time = T(double(k) * dt);
  for (size_t q = 0; q + 1 < pts.size(); q += 2) {
    const T x = T(pts[q]), y = T(pts[q + 1]);
    T stack[ilqg::kExprStackScalars];
    ilqg::ExprJet<T> full, grad;
    ilqg::expr_eval_jet<T>(blk, T(w), T(v), x, y, true, ilqg::ExprStack<T>{stack, 1}, &full, time);
    ilqg::expr_eval_jet<T>(blk, T(w), T(v), x, y, false, ilqg::ExprStack<T>{stack, 1}, &grad, time);
    const T value = ilqg::expr_eval_value<T>(blk, T(w), T(v), x, y, time);
    std::printf("jet %a %a %a %a %a %a | grad %a %a %a | value %a\n", double(full.f), double(full.fx), double(full.fy),
                double(full.fxx), double(full.fyy), double(full.fxy), double(grad.f), double(grad.fx), double(grad.fy),
                double(value));
  }
}

bool read_block(std::istream& in, int nwords, std::unique_ptr<float[]>* blk) {
  blk->reset(new float[nwords > 0 ? nwords : 1]);  // exactly the block (one word for an empty one)
  for (int e = 0; e < nwords; e++) {
    std::string tok;
    in >> tok;
    (*blk)[e] = std::strtof(tok.c_str(), nullptr);
  }
  return bool(in);
}

struct Row {
  int x, y;
  double weight;
  int nwords;
  std::unique_ptr<float[]> blk;
};

struct Model {
  int xdim = 0, udim = 0, k = 0;
  double param = 0.0, dt = 0.0;
  std::vector<Row> rows;
};

void rates(const Model& m, const std::vector<double>& xu, double time, std::vector<double>* f) {
  f->assign(size_t(m.xdim), 0.0);
  for (int r = 0; r < m.xdim; r++) {
    const Row& row = m.rows[size_t(r)];
    (*f)[size_t(r)] = ilqg::expr_eval_value<double>(row.blk.get(), row.weight, m.param, xu[size_t(row.x)],
                                                    row.y >= 0 ? xu[size_t(row.y)] : 0.0, time);
  }
}

void step(const Model& m, std::vector<double> xu, std::vector<double>* out) {
  const int n = m.xdim;
  const double h = m.dt / 2.0;
  std::vector<double> x(xu.begin(), xu.begin() + n), k1, k2, k3, k4;
  for (int s = 0; s < 2; s++) {
    const double t0 = double(m.k) * m.dt + double(s) * h;
    auto at = [&](const std::vector<double>& k, double c, double time, std::vector<double>* f) {
      for (int i = 0; i < n; i++) xu[size_t(i)] = k.empty() ? x[size_t(i)] : x[size_t(i)] + c * k[size_t(i)];
      rates(m, xu, time, f);
      for (double& v : *f) v = h * v;
    };
    at({}, 0.0, t0, &k1);
    at(k1, 0.5, t0 + 0.5 * h, &k2);
    at(k2, 0.5, t0 + 0.5 * h, &k3);
    at(k3, 1.0, t0 + h, &k4);
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
  const double tk = double(m.k) * m.dt;
  std::vector<double> f, A(size_t(n) * n, 0.0), B(size_t(n) * mu, 0.0), next, euler(xu.begin(), xu.begin() + n);
  rates(m, xu, tk, &f);
  for (int i = 0; i < n; i++) A[size_t(i) * n + i] = 1.0;
  for (int r = 0; r < n; r++) {
    const Row& row = m.rows[size_t(r)];
    auto entry = [&](int in) -> double& { return in < n ? A[size_t(r) * n + in] : B[size_t(r) * mu + (in - n)]; };
    double stack[ilqg::kExprStackScalars];
    ilqg::ExprJet<double> j;
    ilqg::expr_eval_jet<double>(row.blk.get(), row.weight, m.param, xu[size_t(row.x)], row.y >= 0 ? xu[size_t(row.y)] : 0.0,
                                false, ilqg::ExprStack<double>{stack, 1}, &j, tk);
    const double dx = double(j.fx) * m.dt, dy = double(j.fy) * m.dt;
    entry(row.x) = row.x == r ? 1.0 + dx : dx;
    if (row.y >= 0) entry(row.y) = row.y == r ? 1.0 + dy : dy;
  }
  step(m, xu, &next);
  for (int i = 0; i < n; i++) euler[size_t(i)] += m.dt * f[size_t(i)];
  print("rate", f, " | ");
  print("A", A, " | ");
  print("B", B, " | ");
  print("step", next, " | ");
  print("euler", euler, "\n");
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
    if (tag == "jet") {
      std::string dtype;
      int two = 0, nwords = 0, npoints = 0, k = 0;
      double w = 0.0, v = 0.0, dt = 0.0;
      in >> dtype >> two >> w >> v >> k >> dt >> nwords;
      if (!in || nwords < 0) return 2;
      std::unique_ptr<float[]> blk;
      if (!read_block(in, nwords, &blk)) return 2;
      in >> npoints;
      std::vector<double> pts(size_t(npoints > 0 ? npoints : 0) * 2);
      for (double& p : pts) in >> p;
      if (!in) return 2;
      const ilqg::ExprCheck chk = ilqg::expr_validate(nwords > 0 ? blk.get() : nullptr, nwords, two != 0);
      std::printf("check %d %d %d\n", chk.fault, chk.op, chk.depth);
      if (chk.fault != ilqg::EXPR_OK) continue;
      if (dtype == "f32") run_jet<float>(blk.get(), w, v, k, dt, pts); else run_jet<double>(blk.get(), w, v, k, dt, pts);
    } else if (tag == "model") {
      m = Model();
      valid = true;
      in >> m.xdim >> m.udim >> m.param >> m.dt >> m.k;
      if (!in || m.xdim < 1 || m.xdim > 8 || m.udim < 1 || m.udim > 2 || m.k < 0) return 2;
    } else if (tag == "row") {
      Row row;
      in >> row.x >> row.y >> row.weight >> row.nwords;
      if (!in || row.nwords < 0 || int(m.rows.size()) >= m.xdim) return 2;
      if (!read_block(in, row.nwords, &row.blk)) return 2;
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

// What the per-instance demos of the host-side C++ mirror share (tests/host/instance_*_demo.cpp): the scene of
// ilqgames_amd/examples.py::modified_three_player_intersection written term for term with the mirrored classes, the
// generator of a batch's inputs, the solver parameters, and the solve half of a demo's main — solve the batch with its
// per-instance tables, write [x0 | the inputs a test replays | final xs | final us] as raw doubles, solve once more
// without the tables.
#pragma once

#include <ilqgames/host/api.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

namespace ilqgames {
namespace {

class HeadlineScene : public TopDownRenderableProblem {
 public:
  using Car = SinglePlayerCar5D;
  using Walker = SinglePlayerUnicycle4D;
  static constexpr Dimension kP1 = 0, kP2 = 5, kP3 = 10;
  // the objects a test declares as per-instance parameters
  std::shared_ptr<QuadraticCost> p1_nominal_speed;
  std::shared_ptr<QuadraticPolyline2Cost> p2_lane;
  std::shared_ptr<ProximityCost> p1_proximity_p2;
  // player 2's turn lane as the costs were built from it (they keep copies): what a test names as a per-instance route
  Polyline2 lane2;

  void ConstructDynamics() override {
    dynamics_.reset(new ConcatenatedDynamicalSystem(
        {std::make_shared<Car>(4.0f), std::make_shared<Car>(4.0f), std::make_shared<Walker>()}));
  }
  void ConstructInitialState() override {
    x0_ = VectorXf::Zero(dynamics_->XDim());
    x0_(kP1 + Car::kPxIdx) = -2.0f;
    x0_(kP1 + Car::kPyIdx) = -30.0f;
    x0_(kP1 + Car::kThetaIdx) = static_cast<float>(M_PI / 2);
    x0_(kP1 + Car::kVIdx) = 4.0f;
    x0_(kP2 + Car::kPxIdx) = -10.0f;
    x0_(kP2 + Car::kPyIdx) = 45.0f;
    x0_(kP2 + Car::kThetaIdx) = static_cast<float>(-M_PI / 2);
    x0_(kP2 + Car::kVIdx) = 3.0f;
    x0_(kP3 + Walker::kPxIdx) = -11.0f;
    x0_(kP3 + Walker::kPyIdx) = 16.0f;
    x0_(kP3 + Walker::kVIdx) = 1.25f;
  }
  void ConstructPlayerCosts() override {
    for (const char* name : {"P1", "P2", "P3"}) player_costs_.emplace_back(name, 10.0f, 10.0f);
    const Polyline2 lane1({Point2(-2.0f, -1000.0f), Point2(-2.0f, 1000.0f)});
    lane2 = Polyline2({Point2(-10.0f, 1000.0f), Point2(-10.0f, 28.0f), Point2(-9.5f, 25.0f), Point2(-9.0f, 24.0f),
                           Point2(-7.0f, 22.5f), Point2(-4.0f, 22.0f), Point2(1000.0f, 22.0f)});
    const Polyline2 lane3({Point2(-1000.0f, 16.0f), Point2(1000.0f, 16.0f)});
    const Polyline2* lanes[3] = {&lane1, &lane2, &lane3};
    const Dimension base[3] = {kP1, kP2, kP3};
    const Dimension vidx[3] = {kP1 + Car::kVIdx, kP2 + Car::kVIdx, kP3 + Walker::kVIdx};
    const float vmax[3] = {12.0f, 12.0f, 2.0f}, vnom[3] = {8.0f, 6.0f, 1.5f};
    const auto xy = [&](PlayerIndex ii) { return std::make_pair(base[ii], Dimension(base[ii] + 1)); };
    for (PlayerIndex ii = 0; ii < 3; ii++) {
      auto lane = std::make_shared<QuadraticPolyline2Cost>(25.0f, *lanes[ii], xy(ii), "lane");
      if (ii == 1) p2_lane = lane;
      player_costs_[ii].AddStateCost(lane);
      player_costs_[ii].AddStateCost(std::make_shared<SemiquadraticPolyline2Cost>(100.0f, *lanes[ii], xy(ii), 2.5f, true, "right"));
      player_costs_[ii].AddStateCost(std::make_shared<SemiquadraticPolyline2Cost>(100.0f, *lanes[ii], xy(ii), -2.5f, false, "left"));
    }
    for (PlayerIndex ii = 0; ii < 3; ii++) {
      player_costs_[ii].AddStateCost(std::make_shared<SemiquadraticCost>(100.0f, vidx[ii], 1.0f, false, "min v"));
      player_costs_[ii].AddStateCost(std::make_shared<SemiquadraticCost>(100.0f, vidx[ii], vmax[ii], true, "max v"));
      auto nominal = std::make_shared<QuadraticCost>(10.0f, vidx[ii], vnom[ii], "nominal v");
      if (ii == 0) p1_nominal_speed = nominal;
      player_costs_[ii].AddStateCost(nominal);
    }
    for (PlayerIndex ii = 0; ii < 3; ii++) {
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(0.1f, 0, 0.0f, "u0"));
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(0.1f, 1, 0.0f, "u1"));
    }
    for (PlayerIndex ii = 0; ii < 3; ii++)
      for (PlayerIndex jj = 0; jj < 3; jj++) {
        if (jj == ii) continue;
        auto gap = std::make_shared<ProximityCost>(0.0f, xy(ii), xy(jj), 6.0f, "proximity");
        if (ii == 0 && jj == 1) p1_proximity_p2 = gap;
        player_costs_[ii].AddStateCost(gap);
      }
  }
  std::vector<float> Xs(const VectorXf& x) const override { return {x(kP1), x(kP2), x(kP3)}; }
  std::vector<float> Ys(const VectorXf& x) const override { return {x(kP1 + 1), x(kP2 + 1), x(kP3 + 1)}; }
  std::vector<float> Thetas(const VectorXf& x) const override { return {x(kP1 + 2), x(kP2 + 2), x(kP3 + 2)}; }
};

struct Lcg {  // [-1, 1), reproducible
  uint32_t state;
  float next() {
    state = state * 1664525u + 1013904223u;
    return static_cast<float>(static_cast<int32_t>(state >> 8) % 20001 - 10000) * 1e-4f;
  }
};

SolverParams Params(float convergence_tolerance = 1.0f, int max_solver_iters = 25) {
  SolverParams params;
  params.max_backtracking_steps = 100;
  params.initial_alpha_scaling = 0.1f;
  params.convergence_tolerance = convergence_tolerance;
  params.expected_decrease_fraction = 0.001f;
  params.max_solver_iters = max_solver_iters;
  return params;
}

// B initial states: the scene's own, each player's position (the state entries at `bases`) moved by up to 1 m in x and
// `y_scale` m in y
std::vector<VectorXf> JitteredStates(const Problem& scene, std::initializer_list<Dimension> bases, float y_scale, size_t B,
                                     Lcg* rng) {
  std::vector<VectorXf> x0s;
  for (size_t b = 0; b < B; b++) {
    VectorXf x = scene.InitialState();
    for (Dimension base : bases) {
      x(base) += rng->next();
      x(base + 1) += y_scale * rng->next();
    }
    x0s.push_back(x);
  }
  return x0s;
}

// `solve f64|f32 B out.bin` once x0s and the tables of `ip` are made; `inputs`: what goes between x0 and the results
int SolveAndWrite(const std::shared_ptr<Problem>& scene, const SolverParams& params, const std::vector<VectorXf>& x0s,
                  const host::InstanceParams& ip, const std::vector<double>& inputs, const char* path) {
  const size_t B = x0s.size();
  ILQSolver solver(scene, params);
  const host::BatchResult result = solver.SolveBatch(x0s, ip);
  CHECK_EQ(result.logs.size(), B);
  std::vector<double> out;
  for (const auto& x : x0s)
    for (Dimension e = 0; e < x.size(); e++) out.push_back(x(e));
  out.insert(out.end(), inputs.begin(), inputs.end());
  for (size_t b = 0; b < B; b++)
    for (const auto& x : result.logs[b]->FinalOperatingPoint().xs)
      for (Dimension e = 0; e < x.size(); e++) out.push_back(x(e));
  for (size_t b = 0; b < B; b++)
    for (const auto& us : result.logs[b]->FinalOperatingPoint().us)
      for (const auto& u : us)
        for (Dimension e = 0; e < u.size(); e++) out.push_back(u(e));
  FILE* f = std::fopen(path, "wb");
  CHECK(f != nullptr);
  CHECK_EQ(std::fwrite(out.data(), sizeof(double), out.size(), f), out.size());
  std::fclose(f);
  // the solve unbinds what it bound: the plain call still runs, as before
  const host::BatchResult plain = solver.SolveBatch(x0s);
  CHECK_EQ(plain.logs.size(), B);
  return 0;
}

}  // namespace
}  // namespace ilqgames

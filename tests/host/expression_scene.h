// ilqgames_amd/examples.py::expression_scene written against the mirrored API (include/ilqgames/host/api.hpp), term for
// term and in the same order: tests/test_expression_cost.py checks that ExpressionCost and host::Expr flatten to the
// descriptor — program blocks included — that the Python builder produces.  Not a reference example.
#pragma once
#include <ilqgames/cost/expression_cost.h>
#include <ilqgames/host/api.hpp>

#include <cmath>
#include <memory>
#include <utility>
#include <vector>

namespace ilqgames {

class ExpressionScene : public TopDownRenderableProblem {
 public:
  using Car = SinglePlayerCar5D;
  void ConstructDynamics() override {
    dynamics_.reset(new ConcatenatedDynamicalSystem({std::make_shared<Car>(4.0f), std::make_shared<Car>(4.0f)}));
  }
  void ConstructInitialState() override {
    x0_ = VectorXf::Zero(dynamics_->XDim());
    x0_(Car::kPyIdx) = -30.0f;
    x0_(Car::kThetaIdx) = static_cast<float>(M_PI_2);
    x0_(Car::kVIdx) = 4.0f;
    x0_(5 + Car::kPxIdx) = -5.0f;
    x0_(5 + Car::kPyIdx) = 30.0f;
    x0_(5 + Car::kThetaIdx) = static_cast<float>(-M_PI_2);
    x0_(5 + Car::kVIdx) = 3.0f;
  }
  void ConstructPlayerCosts() override {
    using host::Expr;
    player_costs_.emplace_back("car1");
    player_costs_.emplace_back("car2");
    const auto xy = [](PlayerIndex ii) { return std::make_pair(Dimension(5 * ii + Car::kPxIdx), Dimension(5 * ii + Car::kPyIdx)); };
    for (PlayerIndex ii = 0; ii < 2; ii++) {
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(25.0f, Car::kOmegaIdx, 0.0f, "steer"));
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(15.0f, Car::kAIdx, 0.0f, "accelerate"));
    }
    player_costs_[0].AddStateCost(std::make_shared<QuadraticCost>(10.0f, Car::kVIdx, 8.0f, "cruise"));
    player_costs_[1].AddStateCost(std::make_shared<QuadraticCost>(10.0f, 5 + Car::kVIdx, 8.0f, "cruise"));
    const Polyline2 lane1({Point2(0.0, -1000.0), Point2(0.0, 1000.0)});
    const Polyline2 lane2({Point2(-5.0, 1000.0), Point2(-5.0, 5.0), Point2(0.0, 0.0), Point2(995.0, 0.0)});
    player_costs_[0].AddStateCost(std::make_shared<QuadraticPolyline2Cost>(25.0f, lane1, xy(0), "lane"));
    player_costs_[1].AddStateCost(std::make_shared<QuadraticPolyline2Cost>(25.0f, lane2, xy(1), "lane"));
    const Expr bump = host::Exp((host::Square(Expr::X() - 0.5) + host::Square(Expr::Y() - -27.0)) * -0.5 / host::Square(Expr::Value())) *
                      Expr::Weight();
    player_costs_[0].AddStateCost(std::make_shared<ExpressionCost>(bump, xy(0).first, xy(0).second, 30.0f, 2.0f, "bump"));
    player_costs_[0].AddStateCost(std::make_shared<ProximityCost>(50.0f, xy(0), xy(1), 6.0f, "gap"));
    const Expr barrier = -(Expr::Weight() * host::Log(Expr::Value() - Expr::X()));
    player_costs_[1].AddStateCost(std::make_shared<ExpressionCost>(barrier, 5 + Car::kVIdx, -1, 2.0f, 15.0f, "speed barrier"));
    player_costs_[1].AddStateCost(std::make_shared<ProximityCost>(50.0f, xy(1), xy(0), 6.0f, "gap"));
    const Expr cap = Expr::Weight() * host::Square(host::Hinge(Expr::X() - Expr::Value()));
    player_costs_[1].AddControlCost(1, std::make_shared<ExpressionCost>(cap, Car::kAIdx, -1, 20.0f, 0.5f, "acceleration cap"));
  }
  std::vector<float> Xs(const VectorXf& x) const override { return {x(0), x(5)}; }
  std::vector<float> Ys(const VectorXf& x) const override { return {x(1), x(6)}; }
  std::vector<float> Thetas(const VectorXf& x) const override { return {x(2), x(7)}; }
};

}  // namespace ilqgames

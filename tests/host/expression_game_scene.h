// ilqgames_amd/examples.py::expression_game_scene written against the mirrored API (include/ilqgames/host/api.hpp), term
// for term and in the same order: tests/test_expression_roles.py checks that the relative ExpressionCost forms and
// ExpressionConstraint flatten to the descriptor — idx[2..3], kind 25 and program blocks included — that the Python
// builder produces.  Not a reference example.
#pragma once
#include <ilqgames/constraint/expression_constraint.h>
#include <ilqgames/cost/expression_cost.h>
#include <ilqgames/host/api.hpp>

#include <cmath>
#include <memory>
#include <utility>
#include <vector>

namespace ilqgames {

class ExpressionGameScene : public TopDownRenderableProblem {
 public:
  using Car = SinglePlayerCar5D;
  void ConstructDynamics() override {
    dynamics_.reset(new ConcatenatedDynamicalSystem({std::make_shared<Car>(4.0f), std::make_shared<Car>(4.0f)}));
  }
  void ConstructInitialState() override {
    x0_ = VectorXf::Zero(dynamics_->XDim());
    x0_(Car::kPyIdx) = -12.0f;
    x0_(Car::kThetaIdx) = static_cast<float>(M_PI_2);
    x0_(Car::kVIdx) = 5.0f;
    x0_(5 + Car::kPxIdx) = -5.0f;
    x0_(5 + Car::kPyIdx) = 10.0f;
    x0_(5 + Car::kThetaIdx) = static_cast<float>(-M_PI_2);
    x0_(5 + Car::kVIdx) = 4.0f;
  }
  void ConstructPlayerCosts() override {
    using host::Expr;
    player_costs_.emplace_back("car1", 10.0f, 10.0f);
    player_costs_.emplace_back("car2", 10.0f, 10.0f);
    const auto xy = [](PlayerIndex ii) { return std::make_pair(Dimension(5 * ii + Car::kPxIdx), Dimension(5 * ii + Car::kPyIdx)); };
    for (PlayerIndex ii = 0; ii < 2; ii++) {
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(25.0f, Car::kOmegaIdx, 0.0f, "steer"));
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(15.0f, Car::kAIdx, 0.0f, "accelerate"));
      player_costs_[ii].AddStateCost(std::make_shared<QuadraticCost>(10.0f, 5 * ii + Car::kVIdx, 6.0f, "cruise"));
    }
    const Polyline2 lane1({Point2(0.0, -1000.0), Point2(0.0, 1000.0)});
    const Polyline2 lane2({Point2(-5.0, 1000.0), Point2(-5.0, 5.0), Point2(0.0, 0.0), Point2(995.0, 0.0)});
    player_costs_[0].AddStateCost(std::make_shared<QuadraticPolyline2Cost>(25.0f, lane1, xy(0), "lane"));
    player_costs_[1].AddStateCost(std::make_shared<QuadraticPolyline2Cost>(25.0f, lane2, xy(1), "lane"));
    const Expr dsq = host::Square(Expr::X()) + host::Square(Expr::Y());
    const Expr repulsion = host::Exp(dsq * -0.5 / host::Square(Expr::Value())) * Expr::Weight();
    player_costs_[0].AddStateCost(std::make_shared<ExpressionCost>(repulsion, xy(0), xy(1), 40.0f, 5.0f, "repulsion"));
    player_costs_[1].AddStateCost(std::make_shared<ExpressionCost>(repulsion, xy(1), xy(0), 40.0f, 5.0f, "repulsion"));
    const Expr match = Expr(0.5) * Expr::Weight() * host::Square(Expr::X() - Expr::Value());
    player_costs_[1].AddStateCost(std::make_shared<ExpressionCost>(match, 5 + Car::kVIdx, ExpressionCost::RelativeTo{Car::kVIdx},
                                                                   2.0f, -1.0f, "speed match"));
    const Expr disc = host::Square(Expr::Value()) - host::Square(Expr::X() - 2.5) - host::Square(Expr::Y() - -2.0);
    player_costs_[0].AddStateConstraint(std::make_shared<FinalTimeConstraint>(
        std::make_shared<ExpressionConstraint>(disc, xy(0), std::make_pair(Dimension(-1), Dimension(-1)), 1.0f, 2.0f, false, "keep out"),
        0.25f));
    const Expr clearance = Expr::Value() - host::Sqrt(dsq);
    player_costs_[1].AddStateConstraint(std::make_shared<ExpressionConstraint>(clearance, xy(1), xy(0), 1.0f, 3.0f, false, "clearance"));
    player_costs_[0].AddControlConstraint(0, std::make_shared<ExpressionConstraint>(
        Expr::X() - Expr::Value(), std::make_pair(Dimension(Car::kAIdx), Dimension(-1)), std::make_pair(Dimension(-1), Dimension(-1)),
        1.0f, 1.5f, false, "acceleration bound"));
  }
  std::vector<float> Xs(const VectorXf& x) const override { return {x(0), x(5)}; }
  std::vector<float> Ys(const VectorXf& x) const override { return {x(1), x(6)}; }
  std::vector<float> Thetas(const VectorXf& x) const override { return {x(2), x(7)}; }
};

}  // namespace ilqgames

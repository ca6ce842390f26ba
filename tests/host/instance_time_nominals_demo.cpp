// Test driver for the per-instance TIME NOMINALS of the host-side C++ mirror (host::InstanceParams::AddReference,
// host::FillInstanceTimeNominals, GameSolver::SolveBatch(x0s, instance_params)): two Car5D on a lane with a corner, a
// RouteProgressCost per player and a NominalPathLengthCost on player 2's x position, written with the mirrored classes.
//   instance_time_nominals_demo resolve                  host only: the tables AddReference(route of player 2) and
//                                                        AddReference(route of player 1) resolve to, a refusal, then
//                                                        "dump" and the flattened description
//   instance_time_nominals_demo solve f64|f32 B out.bin  a batch of B games, each with its own (nominal speed, initial
//                                                        route position) for the two named costs; writes
//                                                        [x0 | speed_pos | time nominals | final xs | final us] as raw
//                                                        doubles
// tests/test_gpu_instance_time_nominals.py replays both through the Python harness.
#include "instance_demo.h"

namespace ilqgames {
namespace {

class TwoCarScene : public TopDownRenderableProblem {
 public:
  using Car = SinglePlayerCar5D;
  static constexpr Dimension kP1 = 0, kP2 = 5;
  // the objects a test names as per-instance references, and one it leaves alone
  std::shared_ptr<RouteProgressCost> p1_route, p2_route;
  std::shared_ptr<NominalPathLengthCost> p2_path_length;
  std::shared_ptr<QuadraticCost> p1_nominal_speed;

  void ConstructDynamics() override {
    dynamics_.reset(new ConcatenatedDynamicalSystem({std::make_shared<Car>(4.0f), std::make_shared<Car>(4.0f)}));
  }
  void ConstructInitialState() override {
    x0_ = VectorXf::Zero(dynamics_->XDim());
    x0_(kP1 + Car::kPxIdx) = -10.0f;
    x0_(kP1 + Car::kPyIdx) = 0.3f;
    x0_(kP1 + Car::kVIdx) = 4.0f;
    x0_(kP2 + Car::kPxIdx) = -18.0f;
    x0_(kP2 + Car::kPyIdx) = -0.4f;
    x0_(kP2 + Car::kVIdx) = 3.0f;
  }
  void ConstructPlayerCosts() override {
    for (const char* name : {"P1", "P2"}) player_costs_.emplace_back(name);
    const Polyline2 lane({Point2(-20.0f, 0.0f), Point2(0.0f, 0.0f), Point2(6.0f, 2.5f), Point2(60.0f, 2.5f)});
    const Dimension base[2] = {kP1, kP2};
    const auto xy = [&](PlayerIndex ii) { return std::make_pair(base[ii], Dimension(base[ii] + 1)); };
    for (PlayerIndex ii = 0; ii < 2; ii++) {
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(25.0f, 0, 0.0f, "u0"));
      player_costs_[ii].AddControlCost(ii, std::make_shared<QuadraticCost>(15.0f, 1, 0.0f, "u1"));
      auto nominal = std::make_shared<QuadraticCost>(4.0f, base[ii] + Car::kVIdx, 5.0f, "nominal v");
      if (ii == 0) p1_nominal_speed = nominal;
      player_costs_[ii].AddStateCost(nominal);
      player_costs_[ii].AddStateCost(std::make_shared<SemiquadraticCost>(50.0f, base[ii] + Car::kPhiIdx, 0.4f, true, "phi"));
    }
    p1_route = std::make_shared<RouteProgressCost>(3.0f, 5.0f, lane, xy(0), "route 1", 10.0f);
    player_costs_[0].AddStateCost(p1_route);
    p2_path_length = std::make_shared<NominalPathLengthCost>(1.5f, kP2 + Car::kPxIdx, 4.0f, "path length");
    player_costs_[1].AddStateCost(p2_path_length);
    p2_route = std::make_shared<RouteProgressCost>(2.0f, 4.0f, lane, xy(1), "route 2", 2.0f);
    player_costs_[1].AddStateCost(p2_route);
    player_costs_[0].AddStateCost(std::make_shared<ProximityCost>(50.0f, xy(0), xy(1), 3.0f, "proximity"));
    player_costs_[1].AddStateCost(std::make_shared<ProximityCost>(50.0f, xy(1), xy(0), 3.0f, "proximity"));
  }
  std::vector<float> Xs(const VectorXf& x) const override { return {x(kP1), x(kP2)}; }
  std::vector<float> Ys(const VectorXf& x) const override { return {x(kP1 + 1), x(kP2 + 1)}; }
  std::vector<float> Thetas(const VectorXf& x) const override { return {x(kP1 + 2), x(kP2 + 2)}; }
};

// player 2's route first, then player 1's: not the tables' order
host::InstanceParams Declared(const TwoCarScene& scene) {
  host::InstanceParams ip;
  ip.AddReference(scene.p2_route);
  ip.AddReference(scene.p1_route.get());
  return ip;
}

}  // namespace
}  // namespace ilqgames

int main(int argc, char** argv) {
  using namespace ilqgames;
  if (argc < 2) {
    std::cerr << "usage: instance_time_nominals_demo resolve | solve f64|f32 B out.bin\n";
    return 2;
  }
  auto scene = std::make_shared<TwoCarScene>();
  scene->Initialize();
  const SolverParams params = Params(0.1f, 15);
  host::InstanceParams ip = Declared(*scene);
  const ilqg_dtype dtype = (argc > 2 && std::strcmp(argv[2], "f32") == 0) ? ILQG_F32 : ILQG_F64;
  host::ProblemDescription description;
  std::string why;
  CHECK(host::DescribeProblem(*scene, params, dtype, &description, &why)) << why;
  if (std::strcmp(argv[1], "resolve") == 0) {
    std::vector<int32_t> tables;
    int32_t count = 0;
    CHECK(host::ResolveTimeNominalReferences(description, ip, &tables, &why, &count)) << why;
    CHECK_EQ(tables.size(), 2u);
    std::cout << "tables " << count << "\n";
    std::cout << "references " << tables[0] << " " << tables[1] << "\n";
    // a cost of the problem that is not time-dependent, and a cost of no problem, are refused with a reason
    const NominalPathLengthCost foreign(1.0f, 0, 1.0f, "foreign");
    for (const Cost* other : {static_cast<const Cost*>(scene->p1_nominal_speed.get()), static_cast<const Cost*>(&foreign)}) {
      host::InstanceParams bad;
      bad.AddReference(other);
      why.clear();
      const bool ok = host::ResolveTimeNominalReferences(description, bad, &tables, &why);
      std::cout << "refused " << (ok ? 1 : 0) << " " << why << "\n";
    }
    // a row the library refuses (the route position turns negative) is reported, not tabulated
    why.clear();
    const bool ok_row = host::FillInstanceTimeNominals(description, 1, {-50.0f, 1.0f, 5.0f, 2.0f}, &ip, &why);
    std::cout << "negative " << (ok_row ? 1 : 0) << " " << why << "\n";
    std::cout << "dump\n" << host::DumpDescription(description);
    return 0;
  }
  if (std::strcmp(argv[1], "solve") != 0 || argc < 5) return 2;
  host::Options().dtype = dtype;
  const size_t B = static_cast<size_t>(std::atoi(argv[3]));
  Lcg rng{2025u};
  const std::vector<VectorXf> x0s = JitteredStates(*scene, {TwoCarScene::kP1, TwoCarScene::kP2}, 0.5f, B, &rng);
  std::vector<float> speed_pos;  // [B][2 references][2]: player 2's route, then player 1's
  for (size_t b = 0; b < B; b++) {
    speed_pos.push_back(4.0f + 2.0f * rng.next());
    speed_pos.push_back(6.0f + 5.0f * rng.next());
    speed_pos.push_back(5.0f + 2.0f * rng.next());
    speed_pos.push_back(14.0f + 5.0f * rng.next());  // some pass the corner at route position 20
  }
  CHECK(host::FillInstanceTimeNominals(description, B, speed_pos, &ip, &why)) << why;
  std::vector<double> inputs(speed_pos.begin(), speed_pos.end());
  inputs.insert(inputs.end(), ip.time_nominals.begin(), ip.time_nominals.end());
  return SolveAndWrite(scene, params, x0s, ip, inputs, argv[4]);
}

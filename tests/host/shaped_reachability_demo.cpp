// GPU test driver: tests/host/shaped_reachability_scene.h — a reach-avoid game whose two ExtremeValueCosts have only
// ExpressionCost children — built through Problem / PlayerCost and solved through the host-side C++ mirror.
//   shaped_reachability_demo dump                    host only: the flattened description (host::DumpDescription)
//   shaped_reachability_demo solve f64|f32 B out.bin GameSolver::SolveBatch on B jittered initial states; writes
//                                                    [x0 | final xs | final us] as raw doubles
// The solver parameters are examples.py::shaped_reachability_scene's.
#include "shaped_reachability_scene.h"
#include "instance_demo.h"

int main(int argc, char** argv) {
  using namespace ilqgames;
  if (argc < 2) {
    std::cerr << "usage: shaped_reachability_demo dump | solve f64|f32 B out.bin\n";
    return 2;
  }
  auto scene = std::make_shared<ShapedReachabilityScene>();
  scene->Initialize();
  SolverParams params = Params(0.01f, 40);
  params.expected_decrease_fraction = 0.1f;
  if (std::strcmp(argv[1], "dump") == 0) {
    host::ProblemDescription description;
    std::string why;
    CHECK(host::DescribeProblem(*scene, params, ILQG_F64, &description, &why)) << why;
    std::cout << host::DumpDescription(description);
    return 0;
  }
  if (std::strcmp(argv[1], "solve") != 0 || argc < 5) return 2;
  host::Options().dtype = std::strcmp(argv[2], "f32") == 0 ? ILQG_F32 : ILQG_F64;
  const size_t B = static_cast<size_t>(std::atoi(argv[3]));
  Lcg rng{2025u};
  const std::vector<VectorXf> x0s = JitteredStates(*scene, {0, 5}, 1.0f, B, &rng);
  return SolveAndWrite(scene, params, x0s, host::InstanceParams(), {}, argv[4]);
}

// GPU test driver: tests/host/gusting_car_scene.h — a model whose heading rate reads the time (host::Expr::Time()) —
// solved through the host-side C++ mirror.
//   gusting_car_demo dump                    host only: the flattened description (host::DumpDescription)
//   gusting_car_demo solve f64|f32 B out.bin GameSolver::SolveBatch on B jittered initial states; writes
//                                            [x0 | final xs | final us] as raw doubles
// tests/test_gpu_expression_time.py solves the dumped description from the same initial states through the Python harness
// and compares.
#include "gusting_car_scene.h"
#include "instance_demo.h"

int main(int argc, char** argv) {
  using namespace ilqgames;
  if (argc < 2) {
    std::cerr << "usage: gusting_car_demo dump | solve f64|f32 B out.bin\n";
    return 2;
  }
  auto scene = std::make_shared<GustingCarScene>();
  scene->Initialize();
  const SolverParams params = Params();
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
  Lcg rng{2024u};
  const std::vector<VectorXf> x0s = JitteredStates(*scene, {0, 4}, 1.0f, B, &rng);
  ILQSolver solver(scene, params);
  const host::BatchResult result = solver.SolveBatch(x0s);
  CHECK_EQ(result.logs.size(), B);
  std::vector<double> out;
  for (const auto& x : x0s)
    for (Dimension e = 0; e < x.size(); e++) out.push_back(x(e));
  for (size_t b = 0; b < B; b++)
    for (const auto& x : result.logs[b]->FinalOperatingPoint().xs)
      for (Dimension e = 0; e < x.size(); e++) out.push_back(x(e));
  for (size_t b = 0; b < B; b++)
    for (const auto& us : result.logs[b]->FinalOperatingPoint().us)
      for (const auto& u : us)
        for (Dimension e = 0; e < u.size(); e++) out.push_back(u(e));
  FILE* f = std::fopen(argv[4], "wb");
  CHECK(f != nullptr);
  CHECK_EQ(std::fwrite(out.data(), sizeof(double), out.size(), f), out.size());
  std::fclose(f);
  return 0;
}

// Test driver for the per-instance ROUTES of the host-side C++ mirror (host::InstanceParams::AddRoute,
// GameSolver::SolveBatch(x0s, instance_params)): the scene of ilqgames_amd/examples.py::modified_three_player_intersection
// written term for term with the mirrored classes, as tests/host/instance_params_demo.cpp has it.
//   instance_routes_demo resolve                  host only: the polyline AddRoute(&lane2) and AddRoute(1) resolve to, the
//                                                 refusals, then "dump" and the flattened description
//   instance_routes_demo solve f64|f32 B out.bin  a batch of B games with the bend of player 2's turn lane displaced per
//                                                 instance; writes [x0 | points | final xs | final us] as raw doubles
// tests/test_instance_routes.py and tests/test_gpu_instance_routes.py replay both through the Python harness.
#include "instance_demo.h"

namespace ilqgames {
namespace {

// player 2's turn lane, named by address
host::InstanceParams Declared(const HeadlineScene& scene) {
  host::InstanceParams ip;
  ip.AddRoute(&scene.lane2);
  return ip;
}

}  // namespace
}  // namespace ilqgames

int main(int argc, char** argv) {
  using namespace ilqgames;
  if (argc < 2) {
    std::cerr << "usage: instance_routes_demo resolve | solve f64|f32 B out.bin\n";
    return 2;
  }
  auto scene = std::make_shared<HeadlineScene>();
  scene->Initialize();
  const SolverParams params = Params();
  host::InstanceParams ip = Declared(*scene);
  if (std::strcmp(argv[1], "resolve") == 0) {
    host::ProblemDescription description;
    std::string why;
    CHECK(host::DescribeProblem(*scene, params, ILQG_F64, &description, &why)) << why;
    std::vector<ilqg_instance_param> declared;
    std::vector<int32_t> rows, by_address, by_index;
    CHECK(host::ResolveInstanceParams(description, ip, &declared, &why, &rows, &by_address)) << why;
    CHECK_EQ(by_address.size(), 1u);
    CHECK_EQ(ilqg_instance_routes_check(&description.desc, 1, by_address.data()), ILQG_OK) << ilqg_last_error();
    std::cout << "address " << by_address[0] << "\n";
    host::InstanceParams indexed;
    indexed.AddRoute(by_address[0]);
    CHECK(host::ResolveInstanceParams(description, indexed, &declared, &why, &rows, &by_index)) << why;
    std::cout << "index " << by_index[0] << "\n";
    // a polyline no cost of the problem was built from is refused, with a reason; so is an index the problem lacks
    const Polyline2 foreign({Point2(0.0f, 0.0f), Point2(1.0f, 1.0f)});
    host::InstanceParams bad;
    bad.AddRoute(&foreign);
    why.clear();
    const bool ok = host::ResolveInstanceParams(description, bad, &declared, &why, &rows, &by_index);
    std::cout << "foreign " << (ok ? 1 : 0) << " " << why << "\n";
    host::InstanceParams bad_index;
    bad_index.AddRoute(3);
    why.clear();
    const bool ok_index = host::ResolveInstanceParams(description, bad_index, &declared, &why, &rows, &by_index);
    std::cout << "polyline3 " << (ok_index ? 1 : 0) << " " << why << "\n";
    // the same polyline twice resolves, and the library refuses it
    host::InstanceParams twice = ip;
    twice.AddRoute(by_address[0]);
    CHECK(host::ResolveInstanceParams(description, twice, &declared, &why, &rows, &by_index)) << why;
    const ilqg_status st = ilqg_instance_routes_check(&description.desc, 2, by_index.data());
    std::cout << "twice " << st << " " << ilqg_last_error() << "\n";
    // routes named where the caller takes none are not dropped
    why.clear();
    const bool ok_none = host::ResolveInstanceParams(description, ip, &declared, &why, &rows);
    std::cout << "noroutes " << (ok_none ? 1 : 0) << " " << why << "\n";
    std::cout << "dump\n" << host::DumpDescription(description);
    return 0;
  }
  if (std::strcmp(argv[1], "solve") != 0 || argc < 5) return 2;
  host::Options().dtype = std::strcmp(argv[2], "f32") == 0 ? ILQG_F32 : ILQG_F64;
  const size_t B = static_cast<size_t>(std::atoi(argv[3]));
  Lcg rng{2024u};
  const std::vector<VectorXf> x0s = JitteredStates(*scene, {HeadlineScene::kP1, HeadlineScene::kP2, HeadlineScene::kP3}, 1.0f, B, &rng);
  const PointList2 lane = scene->lane2.Points();
  for (size_t b = 0; b < B; b++)
    for (size_t k = 0; k < lane.size(); k++) {  // the end of the straight and the bend move by up to 1.5 m
      const bool moves = k >= 1 && k + 1 < lane.size();
      ip.routes.push_back(lane[k].x() + (moves ? 1.5f * rng.next() : 0.0f));
      ip.routes.push_back(lane[k].y() + (moves ? 1.5f * rng.next() : 0.0f));
    }
  return SolveAndWrite(scene, params, x0s, ip, std::vector<double>(ip.routes.begin(), ip.routes.end()), argv[4]);
}

// Test tool (no GPU needed): plan integration of a model whose rows read the time (host::Expr::Time()) is refused by the
// mirror with a CHECK that names the subsystem, before any device call — the C ABI's plan entry points refuse the same
// problem with ILQG_ERR_UNSUPPORTED (include/ilqg.h: ILQG_EXPR_PUSH_TIME).  tests/test_expression_time.py runs it and
// reads the message; reaching the last line would mean the refusal is gone.
#include "gusting_car_scene.h"

#include <iostream>

int main() {
  auto problem = std::make_shared<ilqgames::GustingCarScene>();
  problem->Initialize();
  std::cout << "initialized" << std::endl;
  (void)problem->Dynamics()->Integrate(0.0, 0.05, problem->InitialState(), problem->CurrentOperatingPoint(),
                                       problem->CurrentStrategies());
  std::cout << "integrated" << std::endl;
  return 0;
}

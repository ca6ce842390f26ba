// Host-side check of the spelled-out polynomial steps of csrc/ilqg_trig.hpp (trig_poly_chains, the CHAINS = true form of
// the double kernels): on the host they are __builtin_fma calls, the operations the default form makes, so sine, cosine
// and tangent must come out bit for bit the same in both forms.  Exits non-zero at the first argument where they do not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../ilqgames_amd/csrc/ilqg_trig.hpp"

namespace {

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

long differing = 0;

void one(double x) {
  double s0, c0, s1, c1;
  ilqg::fast_sincos_core<double, false>(x, &s0, &c0);
  ilqg::fast_sincos_core<double, true>(x, &s1, &c1);
  const double t0 = ilqg::fast_tan_core<double, false>(x), t1 = ilqg::fast_tan_core<double, true>(x);
  if (!same_bits(s0, s1) || !same_bits(c0, c1) || !same_bits(t0, t1)) {
    if (differing++ < 5) std::printf("forms differ at %.17g: sin %a %a cos %a %a tan %a %a\n", x, s0, s1, c0, c1, t0, t1);
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(2024);
  const double limit = ilqg::kTrigFastLimit;
  std::uniform_real_distribution<double> wide(-limit, limit), small(-10.0, 10.0), tiny(-1e-3, 1e-3);
  const double half_pi = 1.5707963267948966;
  long count = 0;
  for (int i = 0; i < 1000000; i++, count += 4) {
    one(wide(rng));
    one(small(rng));
    one(tiny(rng));
    one((int(rng() % 2001) - 1000) * half_pi + tiny(rng));  // next to a multiple of pi/2
  }
  for (double x : {0.0, -0.0, half_pi / 2, -half_pi / 2, limit, -limit}) one(x), count++;
  std::printf("chains: %ld arguments, %ld differ\n", count, differing);
  return differing ? EXIT_FAILURE : EXIT_SUCCESS;
}

// ilqg_dims.hip — the per-shape unit of libilqg_hip.so: compiled once per entry of ILQG_FOR_DIMS (ilqg_shapes.hpp) with
// -DILQG_PART_NX / NP / MU, it holds DimsLaunch<T, n, N, m_i> of that shape in both precisions, and with it the kernels
// the shape's launchers bind.  Nothing else reads the three macros.
#include "ilqg_launch.hpp"

template struct DimsLaunch<float, ILQG_PART_NX, ILQG_PART_NP, ILQG_PART_MU>;
template struct DimsLaunch<double, ILQG_PART_NX, ILQG_PART_NP, ILQG_PART_MU>;

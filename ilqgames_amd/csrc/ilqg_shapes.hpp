// ilqg_shapes.hpp — the (n, N, m_i) instantiations of the library: one definition, read by the main unit (the shape
// table kShapes, ilqg_api.hip), by the build recipe (a unit of ilqg_dims.hip per entry) and by the test that wants
// sweep tests for every one of them.
// n=14/16/15/24: BASELINE configs 2-5; (4,2,2): config 1 (TwoPlayerUnicycle4D); (2,2,1): test_lq_solver's point mass;
// (6,3,2): synthetic parity cases.
#pragma once

#if defined(ILQG_DIMS_HEADER)
#include ILQG_DIMS_HEADER  // experiment builds: a generated subset of the list below (__graft_entry__.build_hip_library)
#else
#define ILQG_FOR_DIMS(X) X(14, 3, 2) X(16, 3, 2) X(15, 3, 2) X(24, 4, 2) X(18, 3, 2) X(12, 2, 2) X(10, 2, 2) X(4, 2, 2) X(6, 2, 1) X(3, 2, 1) X(3, 1, 1) X(2, 2, 1) X(6, 3, 2) X(2, 1, 2) X(8, 2, 2) X(17, 3, 2) X(8, 2, 1)
#endif

namespace {
// The list as a table, one entry per shape with DimsLaunch's members in both precisions (kShapes, ilqg_api.hip):
// the entry of (n, N, m_i), or nullptr where the shape has no instantiation.
struct ShapeEntry;
const ShapeEntry* find_shape(int n, int N, int mu);
}  // namespace

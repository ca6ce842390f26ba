// ilqg_problem.hpp — the problem object behind the C ABI's `ilqg_problem` handle (include/ilqg.h):
//   ProblemTables          what creation computes on the host: the DevProblem with its scalar fields filled and every table
//                          a kernel reads.  build_problem_tables() touches no device, so a refusal has nothing to release;
//                          the host-only entry point (ilqg_row_program_build) is a ProblemTables and nothing else.
//   DeviceBuffer / upload  a table on the device, freed by whoever holds it (the two deleters: no other hipFree here).
//   ilqg_problem           the handle: the device tables, the DevProblem that points at them and what the solves keep
//                          between calls.  ilqg_problem_destroy is `delete`.
// (What per-instance declarations and bindings do with the handle: ilqg_instances.hpp.)
// Every translation unit of the library sees the handle and the buffers (the per-shape units reach into the handle);
// only the main unit the builder and the upload (ilqg_problem_build.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "ilqg_lq_generic.hpp"      // GenDims

#include "ilqg_rowprog.hpp"         // RowProgramHost, build_row_program
#include "ilqg_rowprog_static.hpp"  // the registered structures
#include "ilqg_segment.hpp"         // line_segment2: the segment table's arithmetic
#include "ilqg_stages.hpp"          // DevProblem, the models, dims_use_plain_rk4
#include "ilqg_time_nominal.hpp"    // time_nominal: the per-step nominals' arithmetic

namespace ilqg {

// build_time_nominals and time_nominals_kernel step to a polyline's first segment by kSegStride; the shared function then
// strides by its own constant (ilqg_time_nominal.hpp includes no device header): one layout
static_assert(kTimeNominalSegStride == kSegStride, "ilqg_time_nominal.hpp and ilqg_common.hpp disagree on a segment's scalars");
// the kernels take the DevProblem by value: its layout is part of every launch
static_assert(sizeof(DevProblem) == 872, "DevProblem's size changed");  // (840 + dyn_rows)

// LoopTimer (include/ilqgames/utils/loop_timer.h:60-98, src/loop_timer.cpp:55-92): the last ten iteration times
struct LoopTimer {
  double times[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int count = 0, next = 0;
  void add(double seconds) {
    times[next] = seconds;
    next = (next + 1) % 10;
    if (count < 10) count++;
  }
  double upper_bound() const {  // mean + 3 sigma (unbiased), 0.02 s until two samples exist
    if (count < 2) return 0.02;
    double mean = 0.0, var = 0.0;
    for (int i = 0; i < count; i++) mean += times[i];
    mean /= count;
    for (int i = 0; i < count; i++) var += (times[i] - mean) * (times[i] - mean);
    return mean + 3.0 * std::sqrt(var / (count - 1));
  }
};

struct HipFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HipHostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
template <class X> using DeviceBuffer = std::unique_ptr<X[], HipFree>;
using PinnedInts = std::unique_ptr<int[], HipHostFree>;

// A table that exists once per precision of the geometry: on the host, and on the device
template <class F, class D> struct BothPrecisions { std::vector<F> f; std::vector<D> d; };
template <class F, class D> struct DeviceBothPrecisions { DeviceBuffer<F> f; DeviceBuffer<D> d; };

inline GenDims gen_dims_of(int n, int N, const int32_t* udim, int T) {
  GenDims g{};
  g.n = n; g.N = N; g.T = T;
  g.uoff[0] = 0;
  for (int i = 0; i < N; i++) {
    g.udim[i] = udim[i];
    g.uoff[i + 1] = g.uoff[i] + udim[i];
  }
  g.m = g.uoff[N];
  return g;
}

// Per-instance tables bound on a handle (ilqg.h; the checks over the record: ilqg_instances.hpp).  Invariant: every
// table bound on a handle is bound for the same batch, `batch` (which means nothing while none is bound): a bind of
// another table for another batch is refused, so is a call that would read a bound table on another number of instances.
// The kernels read the same state from the DevProblem: inst_values, seg_inst_stride, tnom_inst_stride, null / 0 unless bound.
enum InstanceBinding { kBindValues, kBindRoutes, kBindNominals, kNumBindings };
struct InstanceBindings {
  bool bound[kNumBindings] = {false, false, false};
  int batch = 0;
  void bind(int table, int instances) { bound[table] = true; batch = instances; }
  // Does a solve run the kernels that read per-instance tables (the bound twins, ilqg_solve.hpp)?  DimsLaunch::solve asks
  // twice, the second time for a problem that matches a registered static structure: none of those holds a time-dependent
  // term, so binding nominals to such a problem is refused and whether they count there cannot be observed.
  bool any() const { return bound[kBindValues] || bound[kBindRoutes] || bound[kBindNominals]; }
};

}  // namespace ilqg

struct ilqg_problem {
  ilqg::DevProblem dev;    // what the kernels get: its pointers are the buffers below
  ilqg_problem_desc desc;  // the description's scalars (its pointers are null: the caller's arrays are not kept)
  std::vector<ilqg_cost_term> terms_host;
  ilqg::DeviceBuffer<ilqg::DevTerm> d_terms;
  ilqg::DeviceBuffer<int> d_poly_off;
  ilqg::DeviceBuffer<float> d_poly_pts;
  ilqg::DeviceBothPrecisions<float, double> d_segs, d_dense;
  ilqg::DeviceBothPrecisions<double, double> d_time_nominal;
  ilqg::DeviceBuffer<int> d_cost_order;
  // the row program as built (ilqg_problem_row_program), with the term each op carries, and its device image
  ilqg::RowProgramHost row_prog;
  ilqg::DeviceBuffer<int> d_row_prog;
  // Per-instance parameters (ilqg.h): the declared (term, field) list, the declared subsystems (their columns follow the
  // cost columns), the declared ilqg_solver_fields (theirs come last) and their device table (DevProblem::inst_terms);
  // dev.inst_values / inst_count / inst_solver are set while a table is bound
  std::vector<ilqg_instance_param> inst_params;
  std::vector<int> inst_subs;
  std::vector<int> inst_solver;
  ilqg::DeviceBuffer<int> d_inst_terms;
  // Per-instance routes (ilqg.h): the declared polylines, per polyline of the descriptor its first point in a row of the
  // caller's points or -1 (device copy: route_segments_kernel), the points of a row, and while a table is bound the table
  // (in the handle's precision; dev.segs_f / segs_d points at it, dev.seg_inst_stride is set)
  std::vector<int> route_polys;
  ilqg::DeviceBuffer<int> d_route_cols;
  int route_points = 0;
  ilqg::DeviceBothPrecisions<float, double> d_route_segs;
  // Per-instance time nominals (ilqg.h): per table of the time-dependent costs (its term, 1: a route, its polyline's first
  // segment, segments), the device copy time_nominals_kernel reads, and while a table is bound (dev.time_nominal_f / _d
  // points at the caller's, dev.tnom_inst_stride is set)
  std::vector<int> tnom_tables;
  ilqg::DeviceBuffer<int> d_tnom_tables;
  ilqg::InstanceBindings bindings;  // which of the three tables are bound, and for which batch
  int static_prog = 0;                // id of the registered structure it matches (ilqg_rowprog_static.hpp), 0: none
  bool b_constant = false;            // the feedback sweep may take B's entries from registers (ProblemTables::b_constant)
  ilqg::DeviceBuffer<int> d_unfinished;  // instances still running after an LQ-kernel launch
  ilqg::PinnedInts h_unfinished;  // pinned host mirror: [0..3] the counters, [8] the sequence number of read_round_counters
  int* h_unfinished_dev = nullptr;  // ... as the device addresses it
  int publish_seq = 0;
  bool counters_clean = false;  // d_unfinished was cleared by the last thing that touched it (read_round_counters)
  int mu_uniform = 0;
  bool has_route_progress = false;  // a RouteProgressCost term: its tables are a first solve's (initial time 0)
  bool has_expression = false;  // an expression cost: the row kernels with its evaluator in them run (kExprProg, ilqg_solve.hpp)
  bool has_expression_dynamics = false;  // an ILQG_DYN_EXPRESSION subsystem: the kernels with its integrator and its
                                         // linearisation in them run (kExprDynProg, ilqg_solve.hpp)
  int time_reading_subsystem = -1;  // the first expression subsystem with a row that pushes the time (ILQG_EXPR_PUSH_TIME), -1:
                                    // none.  The receding-horizon plan kernels refuse such a problem (ilqg.h).
  int last_schedule = 0;  // ILQG_SCHEDULE_* of the last solve (ilqg_problem_last_schedule)
  bool generic = false;  // no specialised instantiation holds this problem: every entry point runs the run-time-dimensioned kernels
  // The solver object's LoopTimer over its iterations, kept across solves as the reference's member is (only solves with a
  // max_runtime feed and read it), and AugmentedLagrangianSolver's own (`timer_`) over its outer iterations
  ilqg::LoopTimer loop_timer, al_loop_timer;
};


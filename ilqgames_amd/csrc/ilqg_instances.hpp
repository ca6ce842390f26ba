// ilqg_instances.hpp — the host side of what makes the games of one batch differ (ilqg.h: per-instance cost parameters,
// subsystem parameters, routes, time nominals): the declaration checks, declare_instance_columns, the checks over the
// binding record (ilqg_problem::bindings: every "bound for a batch of N" refusal, the tables from a chunk's first
// instance) and the two table-builder kernels.  Included by the main unit alone (ilqg_api.hip);
// the extern "C" entry points stay there.
#pragma once

#include <string>
#include <vector>

#include "ilqg_problem.hpp"
#include "ilqg_problem_build.hpp"  // upload
#include "ilqg_shared.hpp"         // fail, HIP_TRY

namespace {
using namespace ilqg;

// ---- per-instance cost parameters (ilqg.h) ----
const char* cost_kind_name(int kind) {  // ilqg_cost_kind without its prefix
  static const char* const names[] = {
      "QUADRATIC", "QUADRATIC_POLYLINE2", "SEMIQUADRATIC", "SEMIQUADRATIC_POLYLINE2", "PROXIMITY", "SIGNED_DISTANCE",
      "EXTREME_VALUE", "CONSTRAINT_PROXIMITY", "CONSTRAINT_SINGLE_DIMENSION", "POLYLINE2_SIGNED_DISTANCE",
      "QUADRATIC_DIFFERENCE", "ORIENTATION", "QUADRATIC_NORM", "SEMIQUADRATIC_NORM", "RELATIVE_DISTANCE",
      "LOCALLY_CONVEX_PROXIMITY", "CURVATURE", "CONSTRAINT_POLYLINE2_SIGNED_DISTANCE", "NOMINAL_PATH_LENGTH",
      "ROUTE_PROGRESS", "WEIGHTED_CONVEX_PROXIMITY", "CONSTRAINT_AFFINE_SCALAR", "CONSTRAINT_AFFINE_VECTOR", "EXPRESSION",
      "CONSTRAINT_EXPRESSION", "DYN_ROW_EXPRESSION"};
  static_assert(ILQG_COST_QUADRATIC == 1 && ILQG_DYN_ROW_EXPRESSION == sizeof(names) / sizeof(names[0]), "one name per kind");
  return kind >= 1 && kind <= ILQG_DYN_ROW_EXPRESSION ? names[kind - 1] : "unknown kind";
}
// Does a term of this kind read the field (the table of ilqg.h; ilqg_models.hpp: term_compute_leaf, and the affine and expression evaluators beside it)?
// Null: yes; else why not.
const char* instance_param_refusal(int kind, int field) {
  const bool weight = field == ILQG_PARAM_WEIGHT;
  switch (kind) {
    case ILQG_COST_EXTREME_VALUE: return "an EXTREME_VALUE term has no parameters of its own: declare its children";
    case ILQG_CONSTRAINT_AFFINE_SCALAR:
    case ILQG_CONSTRAINT_AFFINE_VECTOR: return "the affine constraints keep their coefficients in dense blocks";
    case ILQG_COST_NOMINAL_PATH_LENGTH:
    case ILQG_COST_ROUTE_PROGRESS:
      return weight ? nullptr : "its nominal speed is tabulated per time step when the problem is created";
    case ILQG_COST_SIGNED_DISTANCE:
    case ILQG_COST_POLYLINE2_SIGNED_DISTANCE: return weight ? "this kind does not read its weight" : nullptr;
    case ILQG_CONSTRAINT_PROXIMITY:
    case ILQG_CONSTRAINT_SINGLE_DIMENSION:
    case ILQG_CONSTRAINT_POLYLINE2_SIGNED_DISTANCE: return weight ? "a constraint has no weight" : nullptr;
    case ILQG_COST_QUADRATIC_POLYLINE2:
    case ILQG_COST_QUADRATIC_DIFFERENCE:
    case ILQG_COST_RELATIVE_DISTANCE:
    case ILQG_COST_CURVATURE: return weight ? nullptr : "this kind has no nominal or threshold";
    case ILQG_COST_QUADRATIC:
    case ILQG_COST_SEMIQUADRATIC:
    case ILQG_COST_SEMIQUADRATIC_POLYLINE2:
    case ILQG_COST_PROXIMITY:
    case ILQG_COST_ORIENTATION:
    case ILQG_COST_QUADRATIC_NORM:
    case ILQG_COST_SEMIQUADRATIC_NORM:
    case ILQG_COST_LOCALLY_CONVEX_PROXIMITY:
    case ILQG_COST_WEIGHTED_CONVEX_PROXIMITY:
    case ILQG_COST_EXPRESSION:
    case ILQG_CONSTRAINT_EXPRESSION: return nullptr;  // (what its program pushes: PUSH_WEIGHT, PUSH_VALUE)
    case ILQG_DYN_ROW_EXPRESSION:
      return "a dynamics row is no cost term: its VALUE is the subsystem's param0 (declare the subsystem), its weight is baked";
  }
  return "unknown cost kind";
}
ilqg_status instance_params_check_terms(int num_terms, const ilqg_cost_term* terms, int32_t count,
                                        const ilqg_instance_param* params) {
  if (count < 0 || count > ILQG_MAX_INSTANCE_PARAMS)
    return fail(ILQG_ERR_INVALID, "instance parameters: count must be 0 .. ILQG_MAX_INSTANCE_PARAMS");
  if (count > 0 && (!params || !terms)) return fail(ILQG_ERR_INVALID, "null argument");
  for (int c = 0; c < count; c++) {
    const int term = params[c].term, field = params[c].field;
    const std::string where = "instance parameter " + std::to_string(c) + " (term " + std::to_string(term) + ", " +
                              (field == ILQG_PARAM_WEIGHT ? "weight" : field == ILQG_PARAM_VALUE ? "value" : "field " + std::to_string(field)) + "): ";
    if (term < 0 || term >= num_terms)
      return fail(ILQG_ERR_UNSUPPORTED, where + "term index out of range (the problem has " + std::to_string(num_terms) + " terms)");
    if (field != ILQG_PARAM_WEIGHT && field != ILQG_PARAM_VALUE)
      return fail(ILQG_ERR_UNSUPPORTED, where + "not an ilqg_param_field");
    for (int q = 0; q < c; q++)
      if (params[q].term == term && params[q].field == field)
        return fail(ILQG_ERR_UNSUPPORTED, where + "declared twice (also parameter " + std::to_string(q) + ")");
    if (const char* why = instance_param_refusal(terms[term].kind, field))
      return fail(ILQG_ERR_UNSUPPORTED, where + cost_kind_name(terms[term].kind) + ": " + why);
  }
  return ILQG_OK;
}
// Per-instance subsystem parameters (ilqg.h): does a subsystem of this kind read its param0?
const char* dyn_kind_name(int kind) {  // ilqg_dyn_kind without its prefix
  static const char* const names[] = {"UNICYCLE_4D", "CAR_5D", "CAR_6D", "UNICYCLE_4D_DISTURBED", "PLANAR_DISTURBANCE",
                                      "DUBINS_CAR", "AIR_3D_EVADER", "AIR_3D_PURSUER", "POINT_MASS_2D", "UNICYCLE_5D",
                                      "CAR_7D", "DELAYED_DUBINS_CAR", "EXPRESSION"};
  static_assert(ILQG_DYN_UNICYCLE_4D == 1 && ILQG_DYN_EXPRESSION == sizeof(names) / sizeof(names[0]), "one name per kind");
  return kind >= 1 && kind <= ILQG_DYN_EXPRESSION ? names[kind - 1] : "unknown kind";
}
bool subsystem_reads_param0(int kind) {
  switch (kind) {
    case ILQG_DYN_CAR_5D:
    case ILQG_DYN_CAR_6D:
    case ILQG_DYN_CAR_7D:              // inter-axle distance
    case ILQG_DYN_DUBINS_CAR:
    case ILQG_DYN_DELAYED_DUBINS_CAR:  // speed
    case ILQG_DYN_AIR_3D_EVADER:
    case ILQG_DYN_AIR_3D_PURSUER: return true;  // their speeds
    case ILQG_DYN_EXPRESSION: return true;      // what its rows' programs push as VALUE
  }
  return false;
}
ilqg_status instance_subsystems_check(int num_subsystems, const int* kinds, int32_t count, const int32_t* subsystems) {
  if (count < 0 || count > ILQG_MAX_INSTANCE_PARAMS)
    return fail(ILQG_ERR_INVALID, "instance subsystem parameters: count must be 0 .. ILQG_MAX_INSTANCE_PARAMS");
  if (count > 0 && (!subsystems || !kinds)) return fail(ILQG_ERR_INVALID, "null argument");
  for (int c = 0; c < count; c++) {
    const int s = subsystems[c];
    const std::string where = "instance parameter " + std::to_string(c) + " (subsystem " + std::to_string(s) + "): ";
    if (s < 0 || s >= num_subsystems)
      return fail(ILQG_ERR_UNSUPPORTED, where + "row out of range (the problem has " + std::to_string(num_subsystems) + " subsystems)");
    for (int q = 0; q < c; q++)
      if (subsystems[q] == s) return fail(ILQG_ERR_UNSUPPORTED, where + "declared twice (also parameter " + std::to_string(q) + ")");
    if (!subsystem_reads_param0(kinds[s]))
      return fail(ILQG_ERR_UNSUPPORTED, where + dyn_kind_name(kinds[s]) + ": this kind reads no param0");
  }
  return ILQG_OK;
}
// Per-instance solver parameters (ilqg.h): the members of ilqg_solver_params by ilqg_solver_field
const char* solver_field_name(int field) {
  static const char* const names[] = {"convergence_tolerance", "max_solver_iters", "linesearch", "initial_alpha_scaling",
                                      "geometric_alpha_scaling", "max_backtracking_steps", "expected_decrease_fraction",
                                      "open_loop", "unconstrained_solver_max_iters", "geometric_mu_scaling",
                                      "geometric_mu_downscaling", "geometric_lambda_downscaling", "constraint_error_tolerance"};
  static_assert(ILQG_NUM_SOLVER_FIELDS == sizeof(names) / sizeof(names[0]) &&
                    ILQG_SOLVER_CONSTRAINT_ERROR_TOLERANCE + 1 == ILQG_NUM_SOLVER_FIELDS, "one name per member");
  return field >= 0 && field < ILQG_NUM_SOLVER_FIELDS ? names[field] : "unknown field";
}
ilqg_status instance_solver_check(int32_t count, const int32_t* fields) {
  if (count < 0 || count > ILQG_MAX_INSTANCE_PARAMS)
    return fail(ILQG_ERR_INVALID, "instance solver parameters: count must be 0 .. ILQG_MAX_INSTANCE_PARAMS");
  if (count > 0 && !fields) return fail(ILQG_ERR_INVALID, "null argument");
  for (int c = 0; c < count; c++) {
    const int f = fields[c];
    if (f < 0 || f >= ILQG_NUM_SOLVER_FIELDS)
      return fail(ILQG_ERR_UNSUPPORTED, "instance parameter " + std::to_string(c) + " (solver field " + std::to_string(f) +
                                            "): not an ilqg_solver_field");
    const std::string where = "instance parameter " + std::to_string(c) + " (solver field " + solver_field_name(f) + "): ";
    if (f == ILQG_SOLVER_LINESEARCH || f == ILQG_SOLVER_OPEN_LOOP)
      return fail(ILQG_ERR_UNSUPPORTED, where + "it selects kernels and the host's schedule and cannot vary per instance");
    for (int q = 0; q < c; q++)
      if (fields[q] == f) return fail(ILQG_ERR_UNSUPPORTED, where + "declared twice (also parameter " + std::to_string(q) + ")");
  }
  return ILQG_OK;
}
// One value table holds the cost columns, the subsystem columns and the solver columns
ilqg_status instance_total_check(size_t cost_count, size_t subsystem_count, size_t solver_count) {
  if (cost_count + subsystem_count + solver_count > size_t(ILQG_MAX_INSTANCE_PARAMS))
    return fail(ILQG_ERR_INVALID, "instance parameters: " + std::to_string(cost_count) + " cost columns + " +
                                      std::to_string(subsystem_count) + " subsystem columns + " + std::to_string(solver_count) +
                                      " solver columns exceed ILQG_MAX_INSTANCE_PARAMS");
  return ILQG_OK;
}

// ---- per-instance routes (ilqg.h) ----
// May these polylines of the descriptor vary per instance?  A ROUTE_PROGRESS term's per-step nominals are tabulated from
// the baked polyline at creation (build_time_nominals).
ilqg_status instance_routes_check_terms(int num_polylines, int num_terms, const ilqg_cost_term* terms, int32_t count,
                                        const int32_t* polylines) {
  if (count < 0) return fail(ILQG_ERR_INVALID, "instance routes: count must not be negative");
  if (count > 0 && !polylines) return fail(ILQG_ERR_INVALID, "null argument");
  for (int c = 0; c < count; c++) {
    const int q = polylines[c];
    const std::string where = "instance route " + std::to_string(c) + " (polyline " + std::to_string(q) + "): ";
    if (q < 0 || q >= num_polylines)
      return fail(ILQG_ERR_UNSUPPORTED, where + "index out of range (the problem has " + std::to_string(num_polylines) + " polylines)");
    for (int e = 0; e < c; e++)
      if (polylines[e] == q) return fail(ILQG_ERR_UNSUPPORTED, where + "declared twice (also route " + std::to_string(e) + ")");
    for (int ti = 0; ti < num_terms; ti++)
      if (terms[ti].kind == ILQG_COST_ROUTE_PROGRESS && terms[ti].polyline == q)
        return fail(ILQG_ERR_UNSUPPORTED, where + "term " + std::to_string(ti) + " (" + cost_kind_name(terms[ti].kind) +
                                              ") tabulates its per-step nominals from it when the problem is created");
  }
  return ILQG_OK;
}

// ilqg_problem_declare_instance_params / _declare_instance_subsystem_params / _declare_instance_solver_params: the
// checked lists into the handle, and onto the device the column table ((term, field) per cost column, then subsystem ->
// column, then ilqg_solver_field -> column: DevProblem::inst_terms; the solver columns come last) and the
// row stage's side table (per op of the row program the column of its weight / value; the program is not touched).
// Subsystem s's column goes to the weight word of its Jacobian op and, for the Air3D pursuer, to the value word of the
// evader's, where build_row_program put the baked param0.
ilqg_status declare_instance_columns(ilqg_problem* p, const std::vector<ilqg_instance_param>& params,
                                     const std::vector<int>& subs, const std::vector<int>& solver) {
  const std::vector<int>&op_term = p->row_prog.op_term, &op_sub = p->row_prog.op_sub;
  const size_t count = params.size() + subs.size() + solver.size();
  std::vector<int> cols(op_term.size() * 2 + 2, -1), terms(count * 2 + kMaxPlayers + ILQG_NUM_SOLVER_FIELDS, -1);
  for (size_t c = 0; c < params.size(); c++) {
    terms[2 * c] = params[c].term;
    terms[2 * c + 1] = params[c].field;
    for (size_t op = 0; op < op_term.size(); op++)
      if (op_term[op] == params[c].term) cols[2 * op + (params[c].field == ILQG_PARAM_WEIGHT ? 0 : 1)] = int(c);
  }
  for (size_t q = 0; q < subs.size(); q++) {
    const int c = int(params.size() + q), s = subs[q];
    terms[2 * c] = -1;
    terms[2 * c + 1] = s;
    terms[2 * count + s] = c;
    for (size_t op = 0; op < op_sub.size(); op++) {
      if (op_sub[op] == s) cols[2 * op] = c;
      if (op_sub[op] == s - 1 && op_sub[op] >= 0 && p->dev.sub_kind[s] == ILQG_DYN_AIR_3D_PURSUER) cols[2 * op + 1] = c;
    }
  }
  for (size_t q = 0; q < solver.size(); q++) {
    const int c = int(params.size() + subs.size() + q);
    terms[2 * c] = -1;
    terms[2 * c + 1] = -1 - solver[q];
    terms[2 * count + kMaxPlayers + solver[q]] = c;
  }
  const char* what = "instance parameter tables";
  // kernels of earlier calls on any stream may still read the old tables (unbound: they look at neither)
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_failed(what, e);
  DeviceBuffer<int> d_terms;
  const ilqg_status s = upload(terms, 0, what, &d_terms);
  if (s != ILQG_OK) return s;
  e = copy_to_device(p->d_row_prog.get() + p->row_prog.words.size(), cols);
  if (e != hipSuccess) return hip_failed(what, e);
  p->d_inst_terms = std::move(d_terms);  // the old table goes only now that the new one is up
  p->inst_params = params;
  p->inst_subs = subs;
  p->inst_solver = solver;
  return ILQG_OK;
}

// ---- the binding record (ilqg_problem::bindings) ----
// A table in the refusals' words: in front of a bind call's message, as a table that is bound, the rows a bind brings
struct BindingWords { const char *prefix, *bound_name, *noun; };
constexpr BindingWords kBindingWords[kNumBindings] = {
    {"instance parameter values", "per-instance parameter values", "values"},
    {"instance routes", "per-instance routes", "routes"},
    {"instance time nominals", "per-instance time nominals", "nominals"}};

// Every "bound for a batch of N" refusal: table `y` is bound, and not for `batch` instances.  `x`: the table a bind call
// brings `batch` rows of; kNumBindings: an entry point called on `batch` instances.
ilqg_status bound_batch_refusal(const ilqg_problem* p, int y, int32_t batch, int x = kNumBindings) {
  const InstanceBindings& b = p->bindings;
  if (!b.bound[y] || batch == b.batch) return ILQG_OK;
  const std::string bound = std::string(kBindingWords[y].bound_name) + " are bound for a batch of " + std::to_string(b.batch);
  if (x == kNumBindings) return fail(ILQG_ERR_INVALID, bound + ", this call has " + std::to_string(batch) + " instances");
  return fail(ILQG_ERR_INVALID, std::string(kBindingWords[x].prefix) + ": " + bound + ", these " + kBindingWords[x].noun +
                                    " are for " + std::to_string(batch));
}

// What keeps the record's invariant, asked by a bind once its table is known to be declared: a positive batch that is
// the batch of every other table bound (in the enum's order); InstanceBindings::bind follows when nothing can fail any more
ilqg_status bind_batch_check(const ilqg_problem* p, int x, int32_t batch) {
  if (batch <= 0) return fail(ILQG_ERR_INVALID, std::string(kBindingWords[x].prefix) + ": batch must be positive");
  for (int y = 0; y < kNumBindings; y++)
    if (y != x)
      if (ilqg_status s = bound_batch_refusal(p, y, batch, x)) return s;
  return ILQG_OK;
}

// A call that reads a bound table on `batch` instances while it is bound for another batch would read past it: every
// call that evaluates costs (only those read a segment or a nominal), and — `costs` false — with a subsystem column
// declared the ones that integrate or linearise
ilqg_status instance_batch_check(const ilqg_problem* p, int32_t batch, bool costs = true) {
  if (costs)
    for (int y : {kBindRoutes, kBindNominals})
      if (ilqg_status s = bound_batch_refusal(p, y, batch)) return s;
  return costs || !p->inst_subs.empty() ? bound_batch_refusal(p, kBindValues, batch) : ILQG_OK;
}

// Of a segment table kept once per geometry precision (the baked one, a route binding's), the buffer of precision S
template <class S, class Table>
auto& segs_of(Table& table) {
  if constexpr (sizeof(S) == sizeof(float)) return table.f; else return table.d;
}

// p->dev with its bound tables starting at instance b0 (a call that works through a batch in chunks).  The routes' table
// moves in both pointers, the nominals' in the one of the handle's precision, the only one a bind set.
DevProblem dev_from_instance(const ilqg_problem* p, int b0) {
  DevProblem d = p->dev;
  if (p->bindings.bound[kBindValues]) d.inst_values += size_t(b0) * d.inst_count;
  if (p->bindings.bound[kBindRoutes]) {
    d.segs_f += size_t(b0) * d.seg_inst_stride;
    d.segs_d += size_t(b0) * d.seg_inst_stride;
  }
  if (p->bindings.bound[kBindNominals])
    (p->desc.dtype == ILQG_F32 ? d.time_nominal_f : d.time_nominal_d) += size_t(b0) * d.tnom_inst_stride;
  return d;
}

}  // namespace

// ---- the table builders ----
// Per-instance routes (ilqg_problem_bind_instance_routes): the segment table of every instance, [batch][total_segs]
// [kSegStride] in the layout of DevProblem::segs_f / segs_d.  One lane per (instance, segment).  A segment of a declared
// polyline (cols[q] >= 0: its first point in the instance's row of `points`, float [batch][row_points][2]) is built from
// the instance's points by the host builder's own function (ilqg_segment.hpp: the same roundings); a segment of any other
// polyline is copied from the baked table, so that one base pointer serves every op of the row program.
template <typename T>
__global__ void __launch_bounds__(256) route_segments_kernel(const int* poly_off, int num_polylines, const int* cols,
                                                             const float* points, int row_points, const T* baked,
                                                             int total_segs, int batch, T* out) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(batch) * size_t(total_segs)) return;
  const size_t b = gid / size_t(total_segs);
  const int s = int(gid - b * size_t(total_segs));
  T* const o = out + gid * kSegStride;
  for (int q = 0; q < num_polylines; q++) {
    const int first = poly_off[q] - q, nseg = poly_off[q + 1] - poly_off[q] - 1;  // (segment s of polyline q: DevProblem)
    if (s < first || s >= first + nseg) continue;
    if (cols[q] >= 0) {
      segment_and_shortcuts(points + 2 * (b * size_t(row_points) + size_t(cols[q])), nseg, s - first, o);
      return;
    }
    break;
  }
  for (int e = 0; e < kSegStride; e++) o[e] = baked[size_t(s) * kSegStride + e];
}

// Per-instance time nominals (ilqg_instance_time_nominals_build): [batch][tables][T][2] doubles in the layout of
// DevProblem::time_nominal_f / _d per instance.  One lane per (instance, table, step): what build_time_nominals tabulates
// for a descriptor whose term has the instance's (nominal speed, initial route position) — the host builder's own
// function (ilqg_time_nominal.hpp: the same roundings) on the baked segment table of precision S.  `tables`: per table
// (term, 1: a route, the polyline's first segment, its segments).
template <typename S>
__global__ void __launch_bounds__(256) time_nominals_kernel(const int* tables, int num_tables, int T, double dt,
                                                            const float* speed_pos, const S* segs, int batch, double* out) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(batch) * size_t(num_tables) * size_t(T)) return;
  const size_t bq = gid / size_t(T);  // (instance, table): a row of speed_pos
  const int k = int(gid - bq * size_t(T));
  const int* tab = tables + 4 * (bq % size_t(num_tables));
  time_nominal<S>(tab[1] != 0, speed_pos[2 * bq], speed_pos[2 * bq + 1], k, dt, segs + size_t(tab[2]) * kSegStride, tab[3],
                  out + 2 * gid);
}

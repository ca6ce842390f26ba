// ilqg_problem_build.hpp — how an ilqg_problem comes to be (ilqg_problem.hpp has the handle): check_problem_sizes,
// build_problem_tables (the host half: no device is touched) and upload_problem.  Included by the main unit alone.
#pragma once

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ilqg_problem.hpp"
#include "ilqg_shapes.hpp"  // find_shape: has the problem's (n, N, m_i) an instantiation?
#include "ilqg_shared.hpp"  // fail, HIP_TRY

namespace {
using namespace ilqg;

bool build_pairs(const ilqg_pair* pairs, int npairs, const int* udim, int N, PairTable* pt, std::string* err) {
  if (npairs > kMaxPairs) {
    *err = "too many control blocks";
    return false;
  }
  std::memset(pt, 0, sizeof(*pt));
  pt->npairs = npairs;
  for (int i = 0; i < kMaxPlayers; i++) pt->pii[i] = -1;
  int Rsz = 0, rsz = 0;
  for (int q = 0; q < npairs; q++) {
    const int i = pairs[q].i, j = pairs[q].j;
    if (i < 0 || i >= N || j < 0 || j >= N) {
      *err = "control block index out of range";
      return false;
    }
    pt->pi[q] = i;
    pt->pj[q] = j;
    pt->roff[q] = Rsz;
    pt->rgoff[q] = rsz;
    pt->from_cost[q] = 1;
    Rsz += udim[j] * udim[j];
    rsz += udim[j];
    if (i == j) pt->pii[i] = q;
  }
  pt->Rsz = Rsz;
  pt->rsz = rsz;
  for (int i = 0; i < N; i++)
    if (pt->pii[i] < 0) {
      *err = "player " + std::to_string(i) + " is missing a control Hessian";  // lq_feedback_solver.cpp:139-140
      return false;
    }
  return true;
}

bool uniform_udim(const int32_t* udim, int N, int* mu) {
  for (int i = 1; i < N; i++)
    if (udim[i] != udim[0]) return false;
  *mu = udim[0];
  return true;
}

// ---- the host half: a description's tables ----
struct ProblemTables {
  DevProblem dev;              // scalar fields filled, pointers null
  std::vector<DevTerm> terms;  // at least one entry
  std::vector<int> poly_off;   // [num_polylines + 1] (none: empty)
  std::vector<float> poly_pts;
  BothPrecisions<float, double> segs;           // DevProblem::segs_f / segs_d
  BothPrecisions<float, double> dense;          // DevProblem::dense_f / dense_d
  BothPrecisions<double, double> time_nominal;  // DevProblem::time_nominal_f / time_nominal_d
  std::vector<int> tnom_tables;  // per table of time_nominal: (its term, 1: a route, its polyline's first segment, segments)
  std::vector<int> cost_order;
  RowProgramHost row_prog;
  int static_prog = 0;  // id of the registered structure the program matches (ilqg_rowprog_static.hpp), 0: none
  int mu_uniform = 0;   // the players' common control dimension, 0: they differ
  bool b_constant = false;  // B is constant entries, at most one per row and column, and the solves read compact rows
                            // (RowProgramHost::b_constant on a specialised instantiation): ilqg_sweep_b_structure_build
  bool has_route_progress = false;
  bool has_expression = false;  // an expression cost (build_expression_blocks)
  bool has_expression_dynamics = false;  // an expression subsystem (flatten_subsystems)
  int time_reading_subsystem = -1;  // the first expression subsystem with a row that pushes the time (build_dynamics_rows)
  bool generic = false;  // no specialised instantiation holds the problem
};

ilqg_status check_problem_sizes(const ilqg_problem_desc& desc, ProblemTables*) {
  if (desc.num_players < 1 || desc.num_players > ILQG_MAX_PLAYERS) return fail(ILQG_ERR_INVALID, "bad player count");
  if (desc.T < 2 || desc.T > kMaxT) return fail(ILQG_ERR_INVALID, "bad horizon");
  return ILQG_OK;
}

// The concatenated system: each subsystem's place in the state and the controls, and which kernels hold its shape
ilqg_status flatten_subsystems(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  std::memset(&d, 0, sizeof(d));
  d.N = desc.num_players;
  d.T = desc.T;
  d.dt = desc.dt;
  const int kind0 = desc.subsystems[0].kind, kind1 = desc.subsystems[1].kind;
  // TwoPlayerUnicycle4D is exactly the pair (disturbed unicycle, disturbance) and nothing else; Air3D likewise
  const bool is_pair = desc.num_players == 2 && ((kind0 == ILQG_DYN_UNICYCLE_4D_DISTURBED && kind1 == ILQG_DYN_PLANAR_DISTURBANCE) ||
                                                 (kind0 == ILQG_DYN_AIR_3D_EVADER && kind1 == ILQG_DYN_AIR_3D_PURSUER));
  for (int i = 0; i < d.N; i++)  // an expression subsystem stands beside single-player models only
    if (desc.subsystems[i].kind == ILQG_DYN_EXPRESSION)
      for (int q = 0; q < d.N; q++)
        if (subsystem_shape(desc.subsystems[q].kind).paired || desc.subsystems[q].kind == ILQG_DYN_POINT_MASS_2D)
          return fail(ILQG_ERR_UNSUPPORTED, "subsystem " + std::to_string(i) + ": an expression subsystem (kind 13) does not occur "
                                            "beside the shared-state kinds (4, 5, 7, 8) or in a point-mass game (subsystem " +
                                                std::to_string(q) + ")");
  for (int i = 0; i < d.N; i++) {
    const ilqg_subsystem& sub = desc.subsystems[i];
    const SubsystemShape want = subsystem_shape(sub.kind);
    if (sub.kind == ILQG_DYN_EXPRESSION) {
      if (sub.xdim < 1 || sub.xdim > kSubStatesMax || sub.udim < 1 || sub.udim > 2)
        return fail(ILQG_ERR_UNSUPPORTED, "subsystem " + std::to_string(i) + ": an expression subsystem has 1 .. " +
                                              std::to_string(kSubStatesMax) + " states and 1 or 2 controls (xdim = " +
                                              std::to_string(sub.xdim) + ", udim = " + std::to_string(sub.udim) + ")");
      t->has_expression_dynamics = true;
    } else if (want.paired && !is_pair) {
      return fail(ILQG_ERR_UNSUPPORTED, "the shared-state kinds only occur as the pairs (4, 5) and (7, 8)");
    }
    if ((sub.kind == ILQG_DYN_POINT_MASS_2D) != (kind0 == ILQG_DYN_POINT_MASS_2D))
      return fail(ILQG_ERR_UNSUPPORTED, "point masses (kind 9) only occur in games made of point masses");
    if (sub.kind != ILQG_DYN_EXPRESSION && (want.xdim < 0 || sub.xdim != want.xdim || sub.udim != want.udim))
      return fail(ILQG_ERR_UNSUPPORTED, "unknown subsystem kind / dimension");
    d.sub_kind[i] = sub.kind;
    d.sub_param[i] = sub.param0;
    d.udim[i] = sub.udim;
    d.xoff[i + 1] = d.xoff[i] + sub.xdim;
    d.uoff[i + 1] = d.uoff[i] + sub.udim;
    d.state_reg[i] = desc.player_costs[i].state_regularization;
    d.control_reg[i] = desc.player_costs[i].control_regularization;
    d.structure[i] = desc.player_costs[i].structure;
  }
  d.n = d.xoff[d.N];
  d.m = d.uoff[d.N];
  if (d.n > ILQG_MAX_XDIM || d.m > ILQG_MAX_UDIM_TOTAL)  // before any table is sized by them
    return fail(ILQG_ERR_UNSUPPORTED, "more than ILQG_MAX_XDIM states or ILQG_MAX_UDIM_TOTAL controls");
  // DistanceBetween of the first subsystem: (px, py) where the model overrides it (two_player_unicycle_4d.h:141-147
  // too), the whole block where it does not (the two Dubins cars: single_player_dynamical_system.h:69-71)
  d.sync_dist_dims = d.sub_kind[0] == ILQG_DYN_DUBINS_CAR ? 3 : (d.sub_kind[0] == ILQG_DYN_DELAYED_DUBINS_CAR ? 4 : 2);
  if (d.sub_kind[0] == ILQG_DYN_EXPRESSION) d.sync_dist_dims = d.xoff[1];  // the default DistanceBetween: the whole block
  if (!uniform_udim(d.udim, d.N, &t->mu_uniform)) t->mu_uniform = 0;
  bool plain = false;
  for (int i = 0; i < d.N; i++) plain = plain || is_plain_rk4_kind(d.sub_kind[i]);
  const bool instantiated = find_shape(d.n, d.N, t->mu_uniform) != nullptr;
  // Unicycle5D / Car7D / DelayedDubinsCar rows need an instantiation that carries the plain RK4 (dims_use_plain_rk4,
  // ilqg_stages.hpp); in any other shape they run on the run-time-dimensioned path, which picks its integrator by model
  t->generic = !instantiated || (plain && !dims_use_plain_rk4(d.n, d.N, d.udim[0]));
  return ILQG_OK;
}

// The control blocks (i, j) in PlayerCost's first-touch order: control costs, then control constraints
ilqg_status build_pair_table(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  std::vector<ilqg_pair> pairs;
  std::vector<int> from_cost;
  for (int i = 0; i < d.N; i++)
    for (int pass = 0; pass < 2; pass++)
      for (int ti = 0; ti < desc.num_terms; ti++) {
        const ilqg_cost_term& c = desc.terms[ti];
        if (c.player != i) continue;
        if (pass == 0 && c.role != ILQG_ROLE_CONTROL_COST) continue;
        if (pass == 1 && c.role != ILQG_ROLE_CONTROL_CONSTRAINT) continue;
        bool found = false;
        for (auto& pr : pairs) found = found || (pr.i == i && pr.j == c.arg);
        if (!found) {
          pairs.push_back({i, c.arg});
          from_cost.push_back(pass == 0 ? 1 : 0);
        }
      }
  std::string err;
  if (!build_pairs(pairs.data(), (int)pairs.size(), d.udim, d.N, &d.pairs, &err)) return fail(ILQG_ERR_INVALID, err);
  for (size_t q = 0; q < pairs.size(); q++) d.pairs.from_cost[q] = from_cost[q];
  return ILQG_OK;
}

// The description's terms as the kernels read them, and where each one's argument vector sits inside a row's [x | u]
ilqg_status build_term_table(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  d.num_terms = desc.num_terms;
  d.num_polylines = desc.num_polylines;
  t->terms.assign(desc.num_terms > 0 ? desc.num_terms : 1, DevTerm());
  int nc = 0;
  for (int ti = 0; ti < desc.num_terms; ti++) {
    const ilqg_cost_term& c = desc.terms[ti];
    DevTerm& o = t->terms[ti];
    o.kind = c.kind; o.role = c.role; o.player = c.player; o.arg = c.arg;
    for (int q = 0; q < 4; q++) o.idx[q] = c.idx[q];
    o.weight = c.weight; o.value = c.value; o.flags = c.flags; o.polyline = c.polyline;
    o.child_begin = c.child_begin; o.child_count = c.child_count; o.slot = c.constraint_slot;
    o.k_start = c.first_step;
    if (c.kind == ILQG_COST_WEIGHTED_CONVEX_PROXIMITY) {  // its two speed indices ride in `polyline` (wcp_indices)
      if (c.role != ILQG_ROLE_STATE_COST || c.idx_extra[0] < 0 || c.idx_extra[0] >= d.n || c.idx_extra[1] < 0 ||
          c.idx_extra[1] >= d.n)
        return fail(ILQG_ERR_INVALID, "WeightedConvexProximityCost must be a top-level state cost with speed indices "
                                      "inside the state");
      o.polyline = c.idx_extra[0] | (c.idx_extra[1] << 16);
    }
    // Constraint::is_equality_ is only carried for the affine constraints (ilqg.h): on any other kind the multiplier
    // update would drop its clip at zero while the mu gate stayed an inequality's
    // (... and for the expression constraint, whose row op takes the same equality-aware gate)
    if ((c.flags & ILQG_FLAG_EQUALITY) && c.kind != ILQG_CONSTRAINT_AFFINE_SCALAR && c.kind != ILQG_CONSTRAINT_AFFINE_VECTOR &&
        c.kind != ILQG_CONSTRAINT_EXPRESSION)
      return fail(ILQG_ERR_INVALID, "ILQG_FLAG_EQUALITY is only defined for the affine constraints");
    if (c.constraint_slot >= 0 && c.constraint_slot + 1 > nc) nc = c.constraint_slot + 1;
    if (c.role == ILQG_ROLE_DYNAMICS_ROW || c.kind == ILQG_DYN_ROW_EXPRESSION) {  // not a cost: build_dynamics_rows checks it
      o.arg_off = 0;
      o.arg_dim = 0;
      continue;
    }
    const bool on_state = o.role == ILQG_ROLE_STATE_COST || o.role == ILQG_ROLE_STATE_CONSTRAINT || o.role == ILQG_ROLE_CHILD;
    o.arg_off = on_state ? 0 : d.n + d.uoff[o.arg];
    o.arg_dim = on_state ? d.n : d.udim[o.arg];
  }
  d.num_constraints = nc;
  return ILQG_OK;
}

// Coefficient blocks of the affine constraints (DevProblem::dense_f / dense_d), each precision from the description's
// floats in its own arithmetic; DevTerm::polyline of such a term becomes its block's offset
ilqg_status build_affine_blocks(const ilqg_problem_desc& desc, ProblemTables* t) {
  for (int ti = 0; ti < desc.num_terms; ti++) {
    DevTerm& o = t->terms[ti];
    if (!term_is_affine(o.kind)) continue;
    const int dim = o.arg_dim;
    const bool vec = o.kind == ILQG_CONSTRAINT_AFFINE_VECTOR;
    const long long count = vec ? (long long)dim * dim + dim : dim + 1;
    const bool constraint_role = o.role == ILQG_ROLE_STATE_CONSTRAINT || o.role == ILQG_ROLE_CONTROL_CONSTRAINT;
    if (!constraint_role || o.slot < 0 || desc.dense_params == nullptr || desc.terms[ti].polyline < 0 ||
        (long long)desc.terms[ti].polyline + count > desc.num_dense_params)
      return fail(ILQG_ERR_INVALID, "an affine constraint must be a state / control constraint with a multiplier slot "
                                    "and a coefficient block inside ilqg_problem_desc::dense_params");
    const float* src = desc.dense_params + desc.terms[ti].polyline;
    o.polyline = int(t->dense.f.size());
    auto emit = [&](auto& out) {
      using S = typename std::decay<decltype(out)>::type::value_type;
      for (long long e = 0; e < count; e++) out.push_back(S(src[e]));
      if (vec)  // ATA_ = A^T A, AAT_ = A A^T as the constructor forms them (affine_vector_constraint.h:60-61)
        for (int which = 0; which < 2; which++)
          for (int j = 0; j < dim; j++)
            for (int i = 0; i < dim; i++) {
              S acc = S(0);
              for (int q = 0; q < dim; q++)
                acc += which == 0 ? S(src[q + dim * i]) * S(src[q + dim * j]) : S(src[i + dim * q]) * S(src[j + dim * q]);
              out.push_back(acc);
            }
    };
    emit(t->dense.f);
    emit(t->dense.d);
  }
  return ILQG_OK;
}

// What creation checks about one ILQG_COST_EXPRESSION / ILQG_CONSTRAINT_EXPRESSION term (ilqg.h; the program's own
// rules: expr_validate, ilqg_expr.hpp).  arg_dim: the length of the term's argument vector.
ilqg_status check_expression_term(const ilqg_problem_desc& desc, int ti, int arg_dim) {
  const ilqg_cost_term& c = desc.terms[ti];
  const std::string where = "expression term " + std::to_string(ti) + ": ";
  const bool constraint_role = c.role == ILQG_ROLE_STATE_CONSTRAINT || c.role == ILQG_ROLE_CONTROL_CONSTRAINT;
  if (c.kind == ILQG_CONSTRAINT_EXPRESSION) {
    bool child = c.role == ILQG_ROLE_CHILD;
    for (int q = 0; q < desc.num_terms; q++)
      if (desc.terms[q].kind == ILQG_COST_EXTREME_VALUE && ti >= desc.terms[q].child_begin &&
          ti < desc.terms[q].child_begin + desc.terms[q].child_count)
        child = true;
    if (child) return fail(ILQG_ERR_INVALID, where + "an expression constraint cannot be an EXTREME_VALUE child");
    if (!constraint_role)
      return fail(ILQG_ERR_INVALID, where + "an expression constraint's role must be a state or control constraint");
    if (c.constraint_slot < 0)
      return fail(ILQG_ERR_INVALID, where + "constraint_slot = " + std::to_string(c.constraint_slot) + ": an expression "
                                        "constraint needs a multiplier slot of its own");
    for (int q = 0; q < desc.num_terms; q++)
      if (q != ti && desc.terms[q].constraint_slot == c.constraint_slot)
        return fail(ILQG_ERR_INVALID, where + "constraint_slot = " + std::to_string(c.constraint_slot) + " is also term " +
                                          std::to_string(q) + "'s");
  } else {
    if (constraint_role)
      return fail(ILQG_ERR_UNSUPPORTED, where + "an expression is a cost: a constraint role is not supported");
    // A child (ilqg.h): role ILQG_ROLE_CHILD and inside the child range of exactly one ExtremeValueCost — both or neither
    int parents = 0, parent = -1;
    for (int q = 0; q < desc.num_terms; q++)
      if (desc.terms[q].kind == ILQG_COST_EXTREME_VALUE && ti >= desc.terms[q].child_begin &&
          ti < desc.terms[q].child_begin + desc.terms[q].child_count) {
        parents++;
        parent = q;
      }
    if (c.role == ILQG_ROLE_CHILD && parents == 0)
      return fail(ILQG_ERR_UNSUPPORTED, where + "a term with ILQG_ROLE_CHILD that no ILQG_COST_EXTREME_VALUE term lists cannot be "
                                            "an EXTREME_VALUE child: put it inside one parent's [child_begin, child_begin + child_count)");
    if (c.role != ILQG_ROLE_CHILD && parents > 0)
      return fail(ILQG_ERR_UNSUPPORTED, where + "a term with a top-level role cannot be an EXTREME_VALUE child (term " +
                                            std::to_string(parent) + " lists it): give it ILQG_ROLE_CHILD");
    if (parents > 1)
      return fail(ILQG_ERR_INVALID, where + std::to_string(parents) + " ILQG_COST_EXTREME_VALUE terms list it (the last: term " +
                                        std::to_string(parent) + "): a term cannot be an EXTREME_VALUE child of more than one parent");
    if (c.role != ILQG_ROLE_STATE_COST && c.role != ILQG_ROLE_CONTROL_COST && c.role != ILQG_ROLE_CHILD)
      return fail(ILQG_ERR_INVALID, where + "its role must be a top-level state or control cost, or ILQG_ROLE_CHILD under an "
                                        "ExtremeValueCost");
  }
  if (c.idx[0] < 0 || c.idx[0] >= arg_dim)
    return fail(ILQG_ERR_INVALID, where + "idx[0] = " + std::to_string(c.idx[0]) + " is outside its argument vector (dimension " +
                                      std::to_string(arg_dim) + ")");
  if (c.idx[1] != -1 && (c.idx[1] < 0 || c.idx[1] >= arg_dim))
    return fail(ILQG_ERR_INVALID, where + "idx[1] = " + std::to_string(c.idx[1]) + " is neither -1 nor inside its argument "
                                      "vector (dimension " + std::to_string(arg_dim) + ")");
  if (c.idx[1] == c.idx[0]) return fail(ILQG_ERR_INVALID, where + "idx[0] and idx[1] name the same entry");
  // relative inputs: X = v[idx[0]] - v[idx[2]], Y = v[idx[1]] - v[idx[3]]
  for (int k = 2; k < 4; k++)
    if (c.idx[k] != -1 && (c.idx[k] < 0 || c.idx[k] >= arg_dim))
      return fail(ILQG_ERR_INVALID, where + "idx[" + std::to_string(k) + "] = " + std::to_string(c.idx[k]) + " is neither -1 nor "
                                        "inside its argument vector (dimension " + std::to_string(arg_dim) + ")");
  if (c.idx[3] >= 0 && c.idx[2] < 0)
    return fail(ILQG_ERR_INVALID, where + "idx[3] = " + std::to_string(c.idx[3]) + " without idx[2]: a relative term names the "
                                      "partner of its first input");
  if (c.idx[3] >= 0 && c.idx[1] < 0)
    return fail(ILQG_ERR_INVALID, where + "idx[3] = " + std::to_string(c.idx[3]) + " on a one-input term (idx[1] = -1)");
  if (c.idx[2] >= 0 && c.idx[1] >= 0 && c.idx[3] < 0)
    return fail(ILQG_ERR_INVALID, where + "idx[3] = -1 on a two-input term whose idx[2] names a partner: both inputs are "
                                      "relative or neither");
  for (int k = 2; k < 4; k++)
    for (int q = 0; q < k; q++)
      if (c.idx[k] >= 0 && c.idx[k] == c.idx[q])
        return fail(ILQG_ERR_INVALID, where + "idx[" + std::to_string(q) + "] and idx[" + std::to_string(k) + "] name the same entry");
  if (desc.dense_params == nullptr || c.polyline < 0 || c.polyline >= desc.num_dense_params)
    return fail(ILQG_ERR_INVALID, where + "its program block is out of range of ilqg_problem_desc::dense_params");
  const ExprCheck chk = expr_validate(desc.dense_params + c.polyline, (long long)desc.num_dense_params - c.polyline, c.idx[1] >= 0);
  const std::string at = where + "op " + std::to_string(chk.op) + ": ";
  switch (chk.fault) {
    case EXPR_OK: return ILQG_OK;
    case EXPR_BAD_LENGTH:
      return fail(ILQG_ERR_INVALID, where + "program length L must be a whole number in 1 .. " + std::to_string(ILQG_EXPR_MAX_OPS));
    case EXPR_OUT_OF_RANGE:
      return fail(ILQG_ERR_INVALID, where + "its program block is out of range of ilqg_problem_desc::dense_params");
    case EXPR_BAD_OPCODE: return fail(ILQG_ERR_UNSUPPORTED, at + "unknown opcode");
    case EXPR_UNDERFLOW: return fail(ILQG_ERR_INVALID, at + "stack underflow");
    case EXPR_OVERFLOW:
      return fail(ILQG_ERR_UNSUPPORTED, at + "stack overflow (more than " + std::to_string(ILQG_EXPR_MAX_DEPTH) + " entries)");
    case EXPR_NO_SECOND_INPUT: return fail(ILQG_ERR_INVALID, at + "PUSH_Y in a program without a second input (idx[1] = -1)");
  }
  return fail(ILQG_ERR_INVALID, where + "the program ends with " + std::to_string(chk.depth) + " entries on the stack: exactly "
                                    "one, the term's value, must be left");
}

// Programs of the expression costs and constraints, behind the affine blocks in the same table (DevProblem::dense_f / dense_d): the
// block's floats as they are, and as doubles; DevTerm::polyline of such a term becomes its block's offset
ilqg_status build_expression_blocks(const ilqg_problem_desc& desc, ProblemTables* t) {
  for (int ti = 0; ti < desc.num_terms; ti++) {
    DevTerm& o = t->terms[ti];
    if (!term_is_expression(o.kind)) continue;
    if (const ilqg_status s = check_expression_term(desc, ti, o.arg_dim)) return s;
    t->has_expression = true;
    const float* src = desc.dense_params + desc.terms[ti].polyline;
    const int count = 1 + 2 * int(src[0]);
    o.polyline = int(t->dense.f.size());
    t->dense.f.insert(t->dense.f.end(), src, src + count);
    t->dense.d.insert(t->dense.d.end(), src, src + count);
  }
  return ILQG_OK;
}

// What creation checks about one ILQG_DYN_ROW_EXPRESSION term (ilqg.h): its subsystem, its row, its inputs and its
// program.  `d`: the flattened subsystems.
ilqg_status check_dynamics_row_term(const ilqg_problem_desc& desc, const DevProblem& d, int ti) {
  const ilqg_cost_term& c = desc.terms[ti];
  const std::string term = "dynamics-row term " + std::to_string(ti);
  if (c.kind != ILQG_DYN_ROW_EXPRESSION || c.role != ILQG_ROLE_DYNAMICS_ROW)
    return fail(ILQG_ERR_INVALID, term + ": kind ILQG_DYN_ROW_EXPRESSION (26) and role ILQG_ROLE_DYNAMICS_ROW (5) only occur together");
  if (c.player < 0 || c.player >= d.N)
    return fail(ILQG_ERR_INVALID, term + ": player = " + std::to_string(c.player) + " names no subsystem");
  const std::string where = term + " (subsystem " + std::to_string(c.player) + ", row " + std::to_string(c.idx[0]) + "): ";
  if (d.sub_kind[c.player] != ILQG_DYN_EXPRESSION)
    return fail(ILQG_ERR_INVALID, where + "the subsystem is not an expression subsystem (kind 13)");
  const int xdim = d.xoff[c.player + 1] - d.xoff[c.player], udim = d.udim[c.player];
  if (c.idx[0] < 0 || c.idx[0] >= xdim)
    return fail(ILQG_ERR_INVALID, where + "the row lies outside the subsystem's " + std::to_string(xdim) + " states");
  for (int q = 0; q < ti; q++)
    if (desc.terms[q].kind == ILQG_DYN_ROW_EXPRESSION && desc.terms[q].player == c.player && desc.terms[q].idx[0] == c.idx[0])
      return fail(ILQG_ERR_INVALID, where + "the row is defined twice (also by term " + std::to_string(q) + ")");
  if (c.idx[1] < 0 || c.idx[1] >= xdim + udim)
    return fail(ILQG_ERR_INVALID, where + "input X = " + std::to_string(c.idx[1]) + " is outside the subsystem's [x | u] (dimension " +
                                      std::to_string(xdim + udim) + ")");
  if (c.idx[2] != -1 && (c.idx[2] < 0 || c.idx[2] >= xdim + udim))
    return fail(ILQG_ERR_INVALID, where + "input Y = " + std::to_string(c.idx[2]) + " is neither -1 nor inside the subsystem's [x | u] "
                                      "(dimension " + std::to_string(xdim + udim) + ")");
  if (c.idx[2] == c.idx[1]) return fail(ILQG_ERR_INVALID, where + "inputs X and Y name the same entry");
  if (c.idx[3] != -1) return fail(ILQG_ERR_INVALID, where + "idx[3] must be -1");
  if (c.arg != -1 || c.constraint_slot != -1)
    return fail(ILQG_ERR_INVALID, where + "arg and constraint_slot must be -1: a dynamics row is no cost and no constraint");
  if (c.first_step != 0)
    return fail(ILQG_ERR_UNSUPPORTED, where + "first_step = " + std::to_string(c.first_step) + ": a dynamics row cannot be gated");
  for (int q = 0; q < desc.num_terms; q++)
    if (desc.terms[q].kind == ILQG_COST_EXTREME_VALUE && ti >= desc.terms[q].child_begin &&
        ti < desc.terms[q].child_begin + desc.terms[q].child_count)
      return fail(ILQG_ERR_INVALID, where + "a dynamics row cannot be an EXTREME_VALUE child");
  if (desc.dense_params == nullptr || c.polyline < 0 || c.polyline >= desc.num_dense_params)
    return fail(ILQG_ERR_INVALID, where + "its program block is out of range of ilqg_problem_desc::dense_params");
  const ExprCheck chk = expr_validate(desc.dense_params + c.polyline, (long long)desc.num_dense_params - c.polyline, c.idx[2] >= 0);
  const std::string at = where + "op " + std::to_string(chk.op) + ": ";
  switch (chk.fault) {
    case EXPR_OK: return ILQG_OK;
    case EXPR_BAD_LENGTH:
      return fail(ILQG_ERR_INVALID, where + "program length L must be a whole number in 1 .. " + std::to_string(ILQG_EXPR_MAX_OPS));
    case EXPR_OUT_OF_RANGE:
      return fail(ILQG_ERR_INVALID, where + "its program block is out of range of ilqg_problem_desc::dense_params");
    case EXPR_BAD_OPCODE: return fail(ILQG_ERR_UNSUPPORTED, at + "unknown opcode");
    case EXPR_UNDERFLOW: return fail(ILQG_ERR_INVALID, at + "stack underflow");
    case EXPR_OVERFLOW:
      return fail(ILQG_ERR_UNSUPPORTED, at + "stack overflow (more than " + std::to_string(ILQG_EXPR_MAX_DEPTH) + " entries)");
    case EXPR_NO_SECOND_INPUT: return fail(ILQG_ERR_INVALID, at + "PUSH_Y in a program without a second input (Y = -1)");
  }
  return fail(ILQG_ERR_INVALID, where + "the program ends with " + std::to_string(chk.depth) + " entries on the stack: exactly "
                                    "one, the row's rate, must be left");
}

// The rows of the expression subsystems: every dynamics-row term checked, every row of every expression subsystem
// defined once; the programs go behind the other blocks of the dense table (DevTerm::polyline becomes the block's offset,
// DevTerm::child_count 1 where the whole program is one PUSH_X: build_row_program makes that entry the constant dt), and
// behind them each subsystem's row directory (DevProblem::dyn_rows)
ilqg_status build_dynamics_rows(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  for (int ti = 0; ti < desc.num_terms; ti++) {
    const ilqg_cost_term& c = desc.terms[ti];
    if (c.kind != ILQG_DYN_ROW_EXPRESSION && c.role != ILQG_ROLE_DYNAMICS_ROW) continue;
    if (const ilqg_status s = check_dynamics_row_term(desc, d, ti)) return s;
    DevTerm& o = t->terms[ti];
    const float* src = desc.dense_params + c.polyline;
    const int count = 1 + 2 * int(src[0]);
    o.polyline = int(t->dense.f.size());
    o.child_begin = 0;
    o.child_count = (int(src[0]) == 1 && int(src[1]) == ILQG_EXPR_PUSH_X) ? 1 : 0;
    for (int i = 0; i < int(src[0]); i++)
      if (int(src[1 + 2 * i]) == ILQG_EXPR_PUSH_TIME && (t->time_reading_subsystem < 0 || c.player < t->time_reading_subsystem))
        t->time_reading_subsystem = c.player;
    t->dense.f.insert(t->dense.f.end(), src, src + count);
    t->dense.d.insert(t->dense.d.end(), src, src + count);
  }
  for (int s = 0; s < d.N; s++) {
    if (d.sub_kind[s] != ILQG_DYN_EXPRESSION) continue;
    const int xdim = d.xoff[s + 1] - d.xoff[s];
    d.dyn_rows[s] = int(t->dense.f.size());
    for (int r = 0; r < xdim; r++) {
      const DevTerm* row = nullptr;
      for (int ti = 0; ti < desc.num_terms; ti++)
        if (t->terms[ti].kind == ILQG_DYN_ROW_EXPRESSION && t->terms[ti].player == s && t->terms[ti].idx[0] == r) row = &t->terms[ti];
      if (!row)
        return fail(ILQG_ERR_INVALID, "subsystem " + std::to_string(s) + ", row " + std::to_string(r) + ": an expression subsystem's "
                                      "row has no ILQG_DYN_ROW_EXPRESSION term");
      for (float v : {float(row->polyline), float(row->idx[1]), float(row->idx[2]), row->weight}) {
        t->dense.f.push_back(v);
        t->dense.d.push_back(double(v));
      }
    }
  }
  return ILQG_OK;
}

// The polylines, and the LineSegment2 objects of each (line_segment2.h:55-62) with its two shortcuts
// (DevProblem::segs_f / segs_d), each precision from the points' floats in its own arithmetic
ilqg_status build_segments(const ilqg_problem_desc& desc, ProblemTables* t) {
  if (desc.num_polylines) {
    t->poly_off.assign(desc.polyline_offsets, desc.polyline_offsets + desc.num_polylines + 1);
    t->poly_pts.assign(desc.polyline_points, desc.polyline_points + 2 * size_t(t->poly_off.back()));
  }
  for (int q = 0; q < desc.num_polylines; q++) {
    const float* pts = desc.polyline_points + 2 * desc.polyline_offsets[q];
    const int nseg = desc.polyline_offsets[q + 1] - desc.polyline_offsets[q] - 1;
    for (int c = 0; c < nseg; c++) {
      auto emit = [&](auto& out) {  // the arithmetic is ilqg_segment.hpp's, shared with route_segments_kernel
        typename std::decay<decltype(out)>::type::value_type sg[kSegStride];
        segment_and_shortcuts(pts, nseg, c, sg);
        out.insert(out.end(), sg, sg + kSegStride);
      };
      emit(t->segs.f);
      emit(t->segs.d);
    }
  }
  t->dev.total_segs = int(t->segs.f.size() / kSegStride);
  return ILQG_OK;
}

// Per-step nominals of the time-dependent costs, one table per such term and geometry precision (doubles: the
// path-length nominal is a double product in the reference, nominal_path_length_cost.cpp:53; the route point is a
// pair of the geometry's scalars, exact in double).  t = RelativeTime(k) = double(k) * dt (relative_time_tracker.h:
// 63-65); the route position is a scalar of the geometry made from a double expression (route_progress_cost.cpp:57-59).
// DevTerm::polyline of such a term becomes its table.
ilqg_status build_time_nominals(const ilqg_problem_desc& desc, ProblemTables* t) {
  const DevProblem& d = t->dev;
  int ntab = 0;
  for (int ti = 0; ti < desc.num_terms; ti++) {
    DevTerm& o = t->terms[ti];
    if (!term_is_time_dependent(o.kind)) continue;
    const bool route = o.kind == ILQG_COST_ROUTE_PROGRESS;
    if (o.role != ILQG_ROLE_STATE_COST || (route && (o.polyline < 0 || o.polyline >= desc.num_polylines)))
      return fail(ILQG_ERR_INVALID, "a time-dependent cost must be a top-level state cost (with a polyline, for "
                                    "RouteProgressCost)");
    const int src_poly = o.polyline;
    if (route) {
      // Polyline2::PointAt CHECKs its argument (src/polyline2.cpp:68-103): a route position that is negative at any
      // step, or a polyline without a segment, is a programmer error there and ILQG_ERR_INVALID here
      const int nseg_r = desc.polyline_offsets[src_poly + 1] - desc.polyline_offsets[src_poly] - 1;
      const double pos_first = double(desc.terms[ti].value2);
      const double pos_last = pos_first + double(d.T - 1) * d.dt * double(o.value);
      if (nseg_r < 1 || !(pos_first >= 0.0) || !(pos_last >= 0.0))
        return fail(ILQG_ERR_INVALID, "RouteProgressCost: the route needs a segment and a route position that stays "
                                      "non-negative over the horizon (initial_route_pos, nominal_speed)");
      t->has_route_progress = true;
    }
    const int first_seg = route ? desc.polyline_offsets[src_poly] - src_poly : 0;
    const int nseg = route ? desc.polyline_offsets[src_poly + 1] - desc.polyline_offsets[src_poly] - 1 : 0;
    for (int k = 0; k < d.T; k++) {
      auto nominal = [&](const auto& segs, std::vector<double>& out) {  // the arithmetic is ilqg_time_nominal.hpp's
        double pair[2];
        time_nominal(route, o.value, desc.terms[ti].value2, k, d.dt, segs.data() + size_t(first_seg) * kSegStride, nseg, pair);
        out.insert(out.end(), pair, pair + 2);
      };
      nominal(t->segs.f, t->time_nominal.f);
      nominal(t->segs.d, t->time_nominal.d);
    }
    t->tnom_tables.insert(t->tnom_tables.end(), {ti, route ? 1 : 0, first_seg, nseg});
    o.polyline = ntab++;
  }
  return ILQG_OK;
}

// TotalCosts summation order per player: [count, state costs then control costs in table order]
ilqg_status build_cost_order(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  const std::vector<DevTerm>& dt = t->terms;
  int maxc = 0;
  for (int i = 0; i < d.N; i++) {
    int cnt = 0;
    for (int ti = 0; ti < desc.num_terms; ti++)
      if (dt[ti].player == i && (dt[ti].role == ILQG_ROLE_STATE_COST || dt[ti].role == ILQG_ROLE_CONTROL_COST)) cnt++;
    if (cnt > maxc) maxc = cnt;
  }
  d.cost_order_stride = maxc + 1;
  t->cost_order.assign(size_t(d.N) * d.cost_order_stride, 0);
  for (int i = 0; i < d.N; i++) {
    int* o = t->cost_order.data() + size_t(i) * d.cost_order_stride;
    for (int role = 0; role < 2; role++)
      for (int ti = 0; ti < desc.num_terms; ti++)
        if (dt[ti].player == i && dt[ti].role == role) o[1 + o[0]++] = ti;
  }
  return ILQG_OK;
}

// The row program (ilqg_rowprog.hpp), and the registered structure it is, if any (ilqg_rowprog_static.hpp): word for
// word, parameters masked
ilqg_status build_row_program_and_match(const ilqg_problem_desc& desc, ProblemTables* t) {
  DevProblem& d = t->dev;
  RowProgramHost& rph = t->row_prog;
  std::string err;
  if (!build_row_program(d, t->terms, desc.polyline_offsets, &rph, &err)) return fail(ILQG_ERR_UNSUPPORTED, err);
  d.row_prog_words = int(rph.words.size());
  d.rp_pslots = rph.num_pslots;
  d.rp_lslots = rph.max_lslots;
  d.rp_gslots = rph.max_gslots;
  d.rp_maps_off = rph.maps_off;
  d.rp_maps_words = rph.maps_words;
  d.rp_compact_off = rph.compact_off;
  d.rp_compact_w = rph.compact_w;
  t->b_constant = rph.b_constant && rph.compact_w > 0 && !t->generic;
  std::vector<int> masked = rph.words;
  row_program_mask_parameters(&masked);
#define X(ID_, NX_, NP_, MU_)                                                                                   \
  if (t->static_prog == 0 && d.n == NX_ && d.N == NP_ && int(masked.size()) == StaticRowProg<ID_>::kWords &&    \
      std::memcmp(masked.data(), StaticRowProg<ID_>::w, sizeof(int) * masked.size()) == 0)                      \
    t->static_prog = ID_;
  ILQG_STATIC_PROGS(X)
#undef X
  return ILQG_OK;
}

// Everything creation does before it touches a device: the first check a description fails is the one reported
ilqg_status build_problem_tables(const ilqg_problem_desc& desc, ProblemTables* t) {
  *t = ProblemTables();
  using Step = ilqg_status (*)(const ilqg_problem_desc&, ProblemTables*);
  for (Step step : {check_problem_sizes, flatten_subsystems, build_pair_table, build_term_table, build_affine_blocks,
                    build_expression_blocks, build_dynamics_rows, build_segments, build_time_nominals, build_cost_order, build_row_program_and_match})
    if (ilqg_status s = step(desc, t)) return s;
  return ILQG_OK;
}

// ---- the device half: upload into the handle that owns what was uploaded ----
ilqg_status hip_failed(const char* what, hipError_t e) {
  return fail(ILQG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

template <class X>
hipError_t copy_to_device(X* dst, const std::vector<X>& host) {
  return host.empty() ? hipSuccess : hipMemcpy(dst, host.data(), sizeof(X) * host.size(), hipMemcpyHostToDevice);
}

// A device buffer of host.size() + pad_elems elements whose head is `host` (the pad is not written)
template <class X>
ilqg_status upload(const std::vector<X>& host, size_t pad_elems, const char* what, DeviceBuffer<X>* out) {
  X* raw = nullptr;
  hipError_t e = hipMalloc((void**)&raw, sizeof(X) * (host.size() + pad_elems));
  out->reset(raw);
  if (e == hipSuccess) e = copy_to_device(raw, host);
  return e == hipSuccess ? ILQG_OK : hip_failed(what, e);
}
template <class F, class D>
ilqg_status upload(const BothPrecisions<F, D>& host, size_t pad_elems, const char* what, DeviceBothPrecisions<F, D>* out) {
  const ilqg_status s = upload(host.f, pad_elems, what, &out->f);
  return s != ILQG_OK ? s : upload(host.d, pad_elems, what, &out->d);
}

// The round counters' pinned host mirror (read_round_counters), zeroed, and its device address (null: it has none)
ilqg_status alloc_counter_mirror(const char* what, PinnedInts* out, int** device_address) {
  int* raw = nullptr;
  const hipError_t e = hipHostMalloc((void**)&raw, 16 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return hip_failed(what, e);
  out->reset(raw);
  for (int i = 0; i < 16; i++) raw[i] = 0;
  if (hipHostGetDevicePointer((void**)device_address, raw, 0) != hipSuccess) *device_address = nullptr;
  return ILQG_OK;
}

ilqg_status upload_problem(const ilqg_problem_desc& desc, const ProblemTables& t, std::unique_ptr<ilqg_problem>* out) {
  auto p = std::make_unique<ilqg_problem>();
  p->desc = desc;
  p->desc.terms = nullptr;
  p->desc.polyline_offsets = nullptr;
  p->desc.polyline_points = nullptr;
  p->desc.dense_params = nullptr;
  p->terms_host.assign(desc.terms, desc.terms + desc.num_terms);
  p->row_prog = t.row_prog;
  p->static_prog = t.static_prog;
  p->b_constant = t.b_constant;
  p->mu_uniform = t.mu_uniform;
  p->has_route_progress = t.has_route_progress;
  p->time_reading_subsystem = t.time_reading_subsystem;
  p->has_expression = t.has_expression;
  p->has_expression_dynamics = t.has_expression_dynamics;
  p->generic = t.generic;
  p->tnom_tables = t.tnom_tables;
  // the row program's device image: the program, then per op the per-instance column of its weight / value (none: -1)
  std::vector<int> image = t.row_prog.words;
  image.resize(image.size() + 2 * t.row_prog.op_term.size() + 2, -1);
  const char* what = "problem tables";
  ilqg_status s = ILQG_OK;
  auto up = [&](const auto& host, size_t pad_elems, auto* buffer) {
    if (s == ILQG_OK) s = upload(host, pad_elems, what, buffer);
  };
  up(t.terms, 0, &p->d_terms);
  up(t.poly_off, t.poly_off.empty() ? 1 : 0, &p->d_poly_off);
  up(t.poly_pts, t.poly_pts.empty() ? 2 : 0, &p->d_poly_pts);
  up(t.segs, 1, &p->d_segs);
  up(t.time_nominal, 2, &p->d_time_nominal);
  if (!t.tnom_tables.empty()) up(t.tnom_tables, 0, &p->d_tnom_tables);
  up(t.dense, 1, &p->d_dense);
  up(t.cost_order, 0, &p->d_cost_order);
  up(std::vector<int>(), 4, &p->d_unfinished);  // the four round counters: cleared by whoever counts
  if (s == ILQG_OK) s = alloc_counter_mirror(what, &p->h_unfinished, &p->h_unfinished_dev);
  up(image, 0, &p->d_row_prog);
  if (s != ILQG_OK) return s;
  DevProblem& d = p->dev;
  d = t.dev;
  d.terms = p->d_terms.get();
  d.poly_off = p->d_poly_off.get();
  d.poly_pts = p->d_poly_pts.get();
  d.segs_f = p->d_segs.f.get();
  d.segs_d = p->d_segs.d.get();
  d.time_nominal_f = p->d_time_nominal.f.get();
  d.time_nominal_d = p->d_time_nominal.d.get();
  d.dense_f = p->d_dense.f.get();
  d.dense_d = p->d_dense.d.get();
  d.cost_order = p->d_cost_order.get();
  d.row_prog = p->d_row_prog.get();
  *out = std::move(p);
  return ILQG_OK;
}

// ilqg_problem_row_program / ilqg_row_program_build
ilqg_status copy_row_program(const RowProgramHost& prog, int static_prog, int32_t* words_out, int32_t capacity,
                             int32_t* num_words, int32_t* static_id) {
  *num_words = int32_t(prog.words.size());
  if (static_id) *static_id = static_prog;
  if (words_out) {
    if (capacity < *num_words) return fail(ILQG_ERR_INVALID, "ilqg_problem_row_program: buffer too small");
    std::memcpy(words_out, prog.words.data(), sizeof(int32_t) * prog.words.size());
  }
  return ILQG_OK;
}

}  // namespace

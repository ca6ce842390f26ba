/*
 * ilqg.h — C ABI of the MI355X-native iLQGames inner solver (libilqg_hip.so).
 *
 * This is the drop-in boundary for the hot path of HJReachability/ilqgames:
 * forward rollout + linearisation, per-player cost quadraticisation, the
 * coupled backward LQ Nash sweep, and the iterative-LQ loop around them,
 * batched over independent game instances.
 *
 * The reference has no FFI of its own; each entry point below replaces the
 * body of one reference C++ method (cited per function, paths relative to the
 * reference repo root).  The host-side C++ mirror of the reference classes
 * (include/ilqgames/...) packs its objects into the POD descriptors declared
 * here and calls these functions.  INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch / STL / Eigen types.
 *  - All array arguments are DEVICE pointers (HBM resident) unless the
 *    parameter name ends in `_host`.
 *  - Every small matrix is stored column-major (Eigen's default), so buffers
 *    can be handed back through `Strategy::Ps` etc. without reordering.
 *  - Arrays are trajectory-major per instance: [batch][T][...].
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - Return value: ilqg_status; no exceptions cross the boundary; programmer
 *    errors that glog CHECKs abort on in the reference (dimension mismatch,
 *    missing R_ii — src/lq_feedback_solver.cpp:77-78,139-140) are reported as
 *    ILQG_ERR_INVALID.  Algorithmic failure (line-search exhausted,
 *    src/ilq_solver.cpp:146-155) is reported per instance in `status[]`.
 */
#ifndef ILQG_H_
#define ILQG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQG_MAX_PLAYERS 8
#define ILQG_MAX_XDIM 32
#define ILQG_MAX_UDIM_TOTAL 16
#define ILQG_MAX_PAIRS 64

typedef enum {
  ILQG_OK = 0,
  ILQG_ERR_INVALID = 1,     /* bad argument / dimension mismatch / missing R_ii */
  ILQG_ERR_UNSUPPORTED = 2, /* dims or model kind have no device kernel */
  ILQG_ERR_HIP = 3,         /* HIP runtime error (see ilqg_last_error) */
  ILQG_ERR_NO_DEVICE = 4    /* no gfx950 device visible */
} ilqg_status;

typedef enum { ILQG_F32 = 0, ILQG_F64 = 1 } ilqg_dtype;

/* (i, j): player i's cost carries a control block (R_ij, r_ij) on player j's
 * input — the keys of QuadraticCostApproximation::control
 * (include/ilqgames/utils/quadratic_cost_approximation.h:61-86). */
typedef struct {
  int32_t i;
  int32_t j;
} ilqg_pair;

/* Dimensions of one batched LQ game. */
typedef struct {
  int32_t n;                      /* state dimension                      */
  int32_t num_players;            /* N                                    */
  int32_t udim[ILQG_MAX_PLAYERS]; /* m_i                                  */
  int32_t T;                      /* number of time steps                 */
  int32_t batch;                  /* B independent instances              */
  int32_t dtype;                  /* ilqg_dtype                           */
  int32_t adaptive_regularization;/* Gershgorin step of lq_feedback_solver.cpp:163-176 */
  int32_t sweep_formulation;      /* ilqg_choice: ILQG_CHOICE_OFF selects the VALU / LDS formulation of the feedback sweep
                                     where the matrix-core one is the default (n <= 16); ILQG_SWEEP_GENERIC the
                                     run-time-dimensioned kernels every shape without a specialised instantiation runs
                                     on anyway; same results (A/B runs) */
} ilqg_dims;
#define ILQG_SWEEP_GENERIC 3

/* A scheduling choice that does not change results: let the library decide, or force it off / on. */
typedef enum { ILQG_CHOICE_AUTO = 0, ILQG_CHOICE_OFF = 1, ILQG_CHOICE_ON = 2 } ilqg_choice;

/* ------------------------------------------------------------------------ *
 *  LQ Nash sweeps                                                          *
 * ------------------------------------------------------------------------ */

/* Replaces LQFeedbackSolver::Solve (src/lq_feedback_solver.cpp:71-244).
 *
 *  A      [B][T][n*n]            lin.A
 *  Bm     [B][T][n*m]            [lin.Bs[0] | lin.Bs[1] | ...], m = sum m_i
 *  Q      [B][T][N][n*n]         quad[k][i].state.hess
 *  l      [B][T][N][n]           quad[k][i].state.grad
 *  R      [B][T][sum_p m_j^2]    quad[k][i].control[j].hess, pair order
 *  r      [B][T][sum_p m_j]      quad[k][i].control[j].grad, pair order
 *  pairs_host / npairs           which (i,j) blocks exist; (i,i) is mandatory
 *  x0     [B][n] or NULL (=0)    initial delta-x for the forward pass
 *  P      [B][T][m*n]            stacked gains, rows of player i at sum_{p<i} m_p
 *  alpha  [B][T][m]
 *  dx     [B][T][n] or NULL      delta_xs (forward pass, lq_feedback_solver.cpp:217-241)
 *  costates [B][T][N][n] or NULL  -Z_i[k+1] dx_k - zeta_i[k+1], zero at T-1 (lq_feedback_solver.cpp:223-227);
 *                                needs dx (the reference CHECKs the pair, :77-78): ILQG_ERR_INVALID otherwise
 *  Entry T-1 of P/alpha is written as zero (strategy.h:64-70; loop starts at T-2).
 *  Any dimensions within ILQG_MAX_XDIM / ILQG_MAX_PLAYERS / ILQG_MAX_UDIM_TOTAL run, players with different control
 *  dimensions included (src/lq_feedback_solver.cpp:118-160 walks cumulative dimensions): the shapes of the reference's
 *  examples have specialised kernels (matrix cores, LDS-DMA staging), everything else the run-time-dimensioned ones.
 */
ilqg_status ilqg_lq_feedback_batch(const ilqg_dims* d, const void* A,
                                   const void* Bm, const void* Q, const void* l,
                                   const void* R, const void* r,
                                   const ilqg_pair* pairs_host, int32_t npairs,
                                   const void* x0, void* P, void* alpha,
                                   void* dx, void* costates, void* stream);

/* Replaces LQOpenLoopSolver::Solve (src/lq_open_loop_solver.cpp:73-195).
 * Same inputs; P is written as zero, alpha/dx as the reference; costates [B][T][N][n] or NULL:
 * A_k^T (M_i[k+1] x_{k+1} + m_i[k+1]), zero at T-1 (:171-176, :191), dx required with it (:83-84). */
ilqg_status ilqg_lq_openloop_batch(const ilqg_dims* d, const void* A,
                                   const void* Bm, const void* Q, const void* l,
                                   const void* R, const void* r,
                                   const ilqg_pair* pairs_host, int32_t npairs,
                                   const void* x0, void* P, void* alpha,
                                   void* dx, void* costates, void* stream);

/* ------------------------------------------------------------------------ *
 *  Problem descriptor (what Problem::Initialize builds, flattened to PODs)  *
 * ------------------------------------------------------------------------ */

typedef enum {
  ILQG_DYN_UNICYCLE_4D = 1, /* include/ilqgames/dynamics/single_player_unicycle_4d.h:90-116 */
  ILQG_DYN_CAR_5D = 2,      /* include/ilqgames/dynamics/single_player_car_5d.h:100-133     */
  ILQG_DYN_CAR_6D = 3,      /* include/ilqgames/dynamics/single_player_car_6d.h:102-138     */
  /* TwoPlayerUnicycle4D (include/ilqgames/dynamics/two_player_unicycle_4d.h:57-139): ONE 4-state
   * unicycle driven by two players.  Player 0's row is the unicycle with u = (omega, a)
   * (xdim 4, udim 2); player 1's row is a planar disturbance u = (dx, dy) added to the position
   * rates of the row before it (xdim 0, udim 2).  The two kinds only occur as this pair. */
  ILQG_DYN_UNICYCLE_4D_DISTURBED = 4,
  ILQG_DYN_PLANAR_DISTURBANCE = 5,
  ILQG_DYN_DUBINS_CAR = 6, /* include/ilqgames/dynamics/single_player_dubins_car.h:57-120: x = (px, py, theta),
                             u = (omega), constant speed param0; xdim 3, udim 1 */
  /* Air3D (include/ilqgames/dynamics/air_3d.h:64-157): the pursuer's pose relative to the evader, x = (rx, ry,
   * rtheta), driven by the evader's turn rate (player 0) and the pursuer's (player 1).  Row pair like kinds 4/5:
   * the evader row carries the state (xdim 3, udim 1, param0 = evader speed), the pursuer row none (xdim 0,
   * udim 1, param0 = pursuer speed). */
  ILQG_DYN_AIR_3D_EVADER = 7,
  ILQG_DYN_AIR_3D_PURSUER = 8,
  /* include/ilqgames/dynamics/single_player_point_mass_2d.h:55-110: x = (px, py, vx, vy), u = (ax, ay);
   * xdim 4, udim 2.  Point masses only occur in games made of point masses. */
  ILQG_DYN_POINT_MASS_2D = 9,
  /* The rest of the reference's single-player models.  They run on the plain RK4 (one lane walks the four stages of
   * a block) instead of the stage-per-lane integrator of kinds 1-3 and 6, in the instantiations that list them
   * (dims_use_plain_rk4 in csrc/ilqg_stages.hpp). */
  ILQG_DYN_UNICYCLE_5D = 10, /* include/ilqgames/dynamics/single_player_unicycle_5d.h:55-135: x = (px, py, theta, v, s),
                                u = (omega, a); s = path length; xdim 5, udim 2 */
  ILQG_DYN_CAR_7D = 11,      /* include/ilqgames/dynamics/single_player_car_7d.h:61-170: x = (px, py, theta, phi, v,
                                kappa, s), u = (omega, a), param0 = inter-axle distance; xdim 7, udim 2 */
  ILQG_DYN_DELAYED_DUBINS_CAR = 12, /* include/ilqgames/dynamics/single_player_delayed_dubins_car.h:57-129: x = (px, py,
                                theta, omega), u = (alpha), constant speed param0; xdim 4, udim 1 */
  /* A user-defined single-player model (the reference's way is a SinglePlayerDynamicalSystem subclass): 1 <= xdim <= 8,
   * 1 <= udim <= 2, param0 = the model's one free parameter.  Every state row r has exactly one term of kind
   * ILQG_DYN_ROW_EXPRESSION (role ILQG_ROLE_DYNAMICS_ROW) in the description's term table, whose program is the rate
   * xdot_r (see that kind).  A plain-RK4 kind like 10-12; never beside the paired kinds (4/5, 7/8) or in a point-mass game.
   *   Rate.  xdot_r is the program's value (the value-only evaluator: every product and sum rounded on its own).
   *   Integration.  MultiPlayerDynamicalSystem::Integrate's RK4 with two half-steps of dt / 2: per half-step
   *     k1 = h f(x), k2 = h f(x + 0.5 k1), k3 = h f(x + 0.5 k2), k4 = h f(x + k3), x += (k1 + 2 (k2 + k3) + k4) / 6,
   *     each operation rounded on its own, on every path alike.
   *   Linearisation.  A = I + dt J_x, B = dt J_u: the program's jet is evaluated without second derivatives, each
   *     derivative d becomes the entry T(double(d) * dt), a diagonal entry T(1) + that.  A row whose whole program is one
   *     PUSH_X is the constant entry dt.
   *   Distance.  DistanceBetween of an expression first subsystem is over its whole block (the reference's default, as
   *     for the two Dubins cars). */
  ILQG_DYN_EXPRESSION = 13
} ilqg_dyn_kind;

/* One block of a ConcatenatedDynamicalSystem
 * (src/concatenated_dynamical_system.cpp:52-107); player i owns subsystem i.
 * (TwoPlayerUnicycle4D is written as two rows, see ilqg_dyn_kind.) */
typedef struct {
  int32_t kind; /* ilqg_dyn_kind */
  int32_t xdim;
  int32_t udim;
  float param0; /* inter-axle distance for the car models; the speed of the Dubins car */
} ilqg_subsystem;

typedef enum {
  ILQG_COST_QUADRATIC = 1,           /* src/quadratic_cost.cpp:51-94             */
  ILQG_COST_QUADRATIC_POLYLINE2 = 2, /* src/quadratic_polyline2_cost.cpp:52-126  */
  ILQG_COST_SEMIQUADRATIC = 3,       /* src/semiquadratic_cost.cpp:51-85         */
  ILQG_COST_SEMIQUADRATIC_POLYLINE2 = 4, /* src/semiquadratic_polyline2_cost.cpp:52-142 */
  ILQG_COST_PROXIMITY = 5,           /* src/proximity_cost.cpp:52-122            */
  ILQG_COST_SIGNED_DISTANCE = 6,     /* src/signed_distance_cost.cpp:51-113      */
  ILQG_COST_EXTREME_VALUE = 7,       /* src/extreme_value_cost.cpp:51-85         */
  ILQG_CONSTRAINT_PROXIMITY = 8,     /* src/proximity_constraint.cpp:56-116      */
  ILQG_CONSTRAINT_SINGLE_DIMENSION = 9, /* include/ilqgames/constraint/single_dimension_constraint.h:57-103 */
  ILQG_COST_POLYLINE2_SIGNED_DISTANCE = 10, /* src/polyline2_signed_distance_cost.cpp:52-126: idx = (xidx, yidx),
                                              value = nominal, ORIENTED = oriented_same_as_polyline, weight unused */
  ILQG_COST_QUADRATIC_DIFFERENCE = 11, /* src/quadratic_difference_cost.cpp:51-91 with two dimension pairs:
                                         idx = (dims1[0], dims1[1], dims2[0], dims2[1]) */
  ILQG_COST_ORIENTATION = 12,        /* src/orientation_cost.cpp:50-80: idx[0] = heading dimension, value = nominal;
                                        0.5 w wrap(x - nominal)^2 with the difference wrapped into [-pi, pi) */
  ILQG_COST_QUADRATIC_NORM = 13,     /* src/quadratic_norm_cost.cpp:50-94: idx = (dim1, dim2), value = nominal;
                                        0.5 w (|(x[dim1], x[dim2])| - nominal)^2 */
  ILQG_COST_SEMIQUADRATIC_NORM = 14, /* src/semiquadratic_norm_cost.cpp:50-99: the one-sided form; value = threshold,
                                        ORIENTED = oriented_right */
  ILQG_COST_RELATIVE_DISTANCE = 15,  /* src/relative_distance_cost.cpp:50-104: idx = (x1, y1, x2, y2); w |p1 - p2| */
  ILQG_COST_LOCALLY_CONVEX_PROXIMITY = 16, /* src/locally_convex_proximity_cost.cpp:50-108: idx = (x1, y1, x2, y2),
                                        value = threshold; 0.5 w min((thr - |dx|)^2, (thr - |dy|)^2) inside the box */
  ILQG_COST_CURVATURE = 17,          /* src/curvature_cost.cpp:50-86: idx = (omega index, v index); 0.5 w (omega / v)^2 */
  ILQG_CONSTRAINT_POLYLINE2_SIGNED_DISTANCE = 18, /* src/polyline2_signed_distance_constraint.cpp:52-144: idx = (x, y),
                                        polyline, value = threshold, ORIENTED = keep_left */
  /* The two costs that depend on time.  ILQSolver hands them the time RELATIVE to the start of the window
   * (src/ilq_solver.cpp:186,236: RelativeTime(kk) = kk * dt), so each is a quadratic about a per-step nominal that
   * ilqg_problem_create tabulates.  RouteProgressCost subtracts RelativeTimeTracker's initial time from that
   * relative time (src/route_progress_cost.cpp:58), which is 0 until a receding-horizon step resets it: the tables
   * are those of a first solve. */
  ILQG_COST_NOMINAL_PATH_LENGTH = 19, /* src/nominal_path_length_cost.cpp:50-78: idx[0] = dimension, value =
                                        nominal speed; 0.5 w (x[dim] - t * speed)^2 */
  ILQG_COST_ROUTE_PROGRESS = 20,     /* src/route_progress_cost.cpp:52-110: idx = (x, y), polyline, value = nominal
                                        speed, value2 = initial route position; 0.5 w |p - PointAt(pos0 + t speed)|^2 */
  ILQG_COST_WEIGHTED_CONVEX_PROXIMITY = 21, /* src/weighted_convex_proximity_cost.cpp:50-158: idx = (x1, y1, x2, y2),
                                        idx_extra = (v1, v2), value = threshold; LOCALLY_CONVEX_PROXIMITY scaled by
                                        v1^2 + v2^2, derivatives as written there.  Top-level state cost only. */
  /* The two constraints on the WHOLE argument vector (the state, or the control vector of player `arg`; d = its
   * dimension): dense d x d Hessian blocks.  Their coefficients sit in ilqg_problem_desc::dense_params, the term's
   * `polyline` field is the offset of its block there. */
  ILQG_CONSTRAINT_AFFINE_SCALAR = 22, /* include/ilqgames/constraint/affine_scalar_constraint.h:54-100: g = a^T v - b;
                                        block [a (d) | b] */
  ILQG_CONSTRAINT_AFFINE_VECTOR = 23, /* include/ilqgames/constraint/affine_vector_constraint.h:52-112: g = |A v - b| with
                                        a square A; block [A (d x d, column-major) | b (d)]; derivatives as written
                                        there (its Hessian mixes A A^T and A^T A) */
  /* A user-defined cost (the reference's way is a Cost subclass): a small postfix program over one or two entries of
   * its argument vector, evaluated and differentiated to second order on the device (forward mode, ilqg_expr_op below).
   * idx[0] = input x, idx[1] = input y or -1; `polyline` = offset of the program's block in
   * ilqg_problem_desc::dense_params: [L, (opcode_0, imm_0), ..., (opcode_{L-1}, imm_{L-1})] as floats.  The program's
   * result is the term's value: `weight` and `value` enter only where it pushes them.  Top-level state / control cost, or
   * a child of an ExtremeValueCost.
   *
   * As a child.  The term is a well-formed child exactly when its role is ILQG_ROLE_CHILD AND it lies inside the
   * [child_begin, child_begin + child_count) range of exactly one ILQG_COST_EXTREME_VALUE term; either without the other
   * is refused (ILQG_ERR_UNSUPPORTED: "... cannot be an EXTREME_VALUE child"), two parents are ILQG_ERR_INVALID.  A child
   * takes everything a top-level expression cost takes — one or two inputs, the relative forms, PUSH_WEIGHT / PUSH_VALUE
   * (per instance where declared), PUSH_TIME — over the state (arg = -1), as every child; role, player, `first_step` gate
   * and cost structure are the parent's.  Max / min over such children is the union / intersection of the sets whose
   * signed distances the programs are.  The parent's value and active child at a step come from the children's values at
   * that step, first strict improvement in table order (src/extreme_value_cost.cpp:66-85); only the active child's jet
   * is scattered.  An ILQG_CONSTRAINT_EXPRESSION or dynamics-row term is never a child, nor is an ExtremeValueCost.
   *
   * Relative inputs (both expression kinds).  idx[2] = idx[3] = -1: the inputs are the entries themselves, as above.
   * idx[2] >= 0: the inputs are differences, rounded once in the solve's scalar type as the built-in kinds round theirs,
   *   X = v[idx[0]] - v[idx[2]],  Y = v[idx[1]] - v[idx[3]] (a two-input term);
   * idx[3] >= 0 exactly when idx[1] >= 0 and idx[2] >= 0; every named index lies inside the argument vector and all of
   * them are distinct.  What the jet (f, fx, fy, fxx, fyy, fxy) adds to the tile:
   *   inputs                 pattern                        gx   gy    hxx  hyy  hxy
   *   x                      SINGLE (idx0)                  fx         fxx
   *   x, y                   PAIR2  (idx0, idx1)            fx   fy    fxx  fyy  fxy
   *   x - x'                 PAIR2  (idx0, idx2)            fx   -fx   fxx  fxx  -fxx
   *   x - x', y - y'         PAIR4  (idx0, idx1, idx2, idx3) fx  fy    fxx  fyy  fxy   (the pattern carries the signs,
   *                                                                                    as for ProximityCost) */
  ILQG_COST_EXPRESSION = 24,
  /* A user-defined constraint g(X, Y) <= 0 (g = 0 with ILQG_FLAG_EQUALITY): the same program block, validator, idx rules
   * and relative inputs as ILQG_COST_EXPRESSION; `weight` and `value` enter only where the program pushes them.  Roles
   * ILQG_ROLE_STATE_CONSTRAINT / ILQG_ROLE_CONTROL_CONSTRAINT only, with a multiplier slot of its own; `first_step` gates
   * it as FinalTimeConstraint does (g = 0 before it).  The row stage applies Constraint::ModifyDerivatives to the jet
   * (with the equality-aware Mu) before the scatter of the table above; the term adds nothing to a player's cost. */
  ILQG_CONSTRAINT_EXPRESSION = 25,
  /* One state row of an ILQG_DYN_EXPRESSION subsystem: the same program block, ilqg_expr_op set and limits.  `player` =
   * the subsystem; idx[0] = the row r it defines (0 <= r < xdim); idx[1] = input X, idx[2] = input Y or -1, both indices
   * into the subsystem's own [x (xdim) | u (udim)] and distinct; idx[3] = -1; `polyline` = offset of the program's block
   * in dense_params; arg = -1, constraint_slot = -1, first_step = 0.  PUSH_VALUE pushes the subsystem's param0 (the
   * instance's, where the subsystem is declared per instance), PUSH_WEIGHT the term's `weight`, a second constant.
   * Role ILQG_ROLE_DYNAMICS_ROW only: the term takes no part in any cost walk (it is in no cost order, is no child and no
   * constraint, has no multiplier slot), and cannot carry a per-instance cost parameter.  Every row of an expression
   * subsystem has exactly one such term; a subsystem of any other kind has none. */
  ILQG_DYN_ROW_EXPRESSION = 26
} ilqg_cost_kind;

/* The program of an ILQG_COST_EXPRESSION term: 1 <= L <= ILQG_EXPR_MAX_OPS ops on a stack that never holds more than
 * ILQG_EXPR_MAX_DEPTH entries and exactly one at the end.  An entry is the jet (f, fx, fy, fxx, fyy, fxy) in the solve's
 * scalar type.  Pushes: X (x,1,0,0,0,0), Y (y,0,1,0,0,0), CONST (imm), WEIGHT, VALUE (the term's, or the instance's),
 * TIME (t,0,0,0,0,0) — see below.
 * Binary ops take a (below) and b (top): ADD, SUB, MUL, DIV.  Unary ops replace the top: NEG, SQUARE, SQRT, EXP, LOG, SIN,
 * COS, and HINGE — the entry itself where its f > 0 strictly, else all zeros (src/semiquadratic_cost.cpp's one-sided
 * rule).  Every product and sum rounds on its own (no contraction); a NaN or Inf is the program's own.
 *
 *   opcode  name         kind    what it does
 *   1       PUSH_X       push    the first input, (x, 1, 0, 0, 0, 0)
 *   2       PUSH_Y       push    the second input, (y, 0, 1, 0, 0, 0); a two-input term only
 *   3       PUSH_CONST   push    the op's immediate
 *   4       PUSH_WEIGHT  push    the term's `weight` (the instance's where it is bound per instance)
 *   5       PUSH_VALUE   push    the term's `value` (a dynamics row: the subsystem's param0)
 *   6-9     ADD SUB MUL DIV      binary, a (below) op b (top)
 *   10-17   NEG SQUARE SQRT EXP LOG SIN COS HINGE   unary, on the top entry
 *   18      PUSH_TIME    push    the time, (t, 0, 0, 0, 0, 0): a leaf whose derivatives are all zero
 *
 * PUSH_TIME.  t is the time the reference's ILQSolver hands the object at that step, RelativeTimeTracker::RelativeTime(k):
 * double(k) * dt, rounded once to the solve's scalar type.  It is relative to the start of the window: in a
 * receding-horizon loop a time-reading cost or constraint sees what NominalPathLengthCost sees there.  In the value-only
 * walks of the open-loop form the step is the one the term is evaluated at there (the "next step" index).  An expression
 * child of an ExtremeValueCost reads the time of the step its parent is evaluated at, as the reference's parent hands its
 * own t to its children — in the row stage and in the value-only walks alike (the built-in time-dependent kinds, as
 * children, are still evaluated at step 0 there).
 *   In an ILQG_DYN_ROW_EXPRESSION program t is the time of the stage being evaluated: the linearisation is at t_k = k dt,
 *   the Euler form integrates at t_k, and the two RK4 half-steps of h = dt / 2 evaluate their stages at t0, t0 + h/2,
 *   t0 + h/2, t0 + h with t0 = k dt and then k dt + h (MultiPlayerDynamicalSystem::Integrate), each time formed in double
 *   and rounded once.  The receding-horizon plan kernels integrate partial steps at absolute plan times, where the
 *   reference gives no consistent time: a problem with a dynamics row that reads the time is refused there
 *   (ILQG_ERR_UNSUPPORTED; ilqg_receding_horizon_shift_batch, _sync_batch, plan integration).  Time-reading costs and
 *   constraints are not. */
typedef enum {
  ILQG_EXPR_PUSH_X = 1, ILQG_EXPR_PUSH_Y = 2, ILQG_EXPR_PUSH_CONST = 3, ILQG_EXPR_PUSH_WEIGHT = 4, ILQG_EXPR_PUSH_VALUE = 5,
  ILQG_EXPR_ADD = 6, ILQG_EXPR_SUB = 7, ILQG_EXPR_MUL = 8, ILQG_EXPR_DIV = 9,
  ILQG_EXPR_NEG = 10, ILQG_EXPR_SQUARE = 11, ILQG_EXPR_SQRT = 12, ILQG_EXPR_EXP = 13, ILQG_EXPR_LOG = 14,
  ILQG_EXPR_SIN = 15, ILQG_EXPR_COS = 16, ILQG_EXPR_HINGE = 17,
  ILQG_EXPR_PUSH_TIME = 18
} ilqg_expr_op;
#define ILQG_EXPR_MAX_OPS 64
#define ILQG_EXPR_MAX_DEPTH 4

/* Where a term sits inside PlayerCost::Quadraticize (src/player_cost.cpp:194-215):
 * state costs, control costs, state constraints, control constraints — in that
 * order; CHILD terms are only reached through an EXTREME_VALUE parent. */
typedef enum {
  ILQG_ROLE_STATE_COST = 0,
  ILQG_ROLE_CONTROL_COST = 1,
  ILQG_ROLE_STATE_CONSTRAINT = 2,
  ILQG_ROLE_CONTROL_CONSTRAINT = 3,
  ILQG_ROLE_CHILD = 4,
  ILQG_ROLE_DYNAMICS_ROW = 5 /* an ILQG_DYN_ROW_EXPRESSION term: a state row of an expression subsystem, not a cost */
} ilqg_cost_role;

#define ILQG_FLAG_ORIENTED 1 /* oriented_right / keep_within / keep_below / less_is_positive */
#define ILQG_FLAG_IS_MIN 2   /* ExtremeValueCost::is_min_ */
#define ILQG_FLAG_EQUALITY 4 /* Constraint::is_equality_ (constraint.h:74-76,98-117): no inactive-constraint gate on mu, the
                                multiplier is not clipped at zero.  The affine constraints take it; the reference's other
                                constraints are inequalities by construction. */

typedef struct {
  int32_t kind;        /* ilqg_cost_kind                                       */
  int32_t role;        /* ilqg_cost_role                                       */
  int32_t player;      /* owning PlayerCost                                    */
  int32_t arg;         /* control costs/constraints: which player's u; else -1 */
  int32_t idx[4];      /* QUADRATIC/SEMIQUADRATIC/SINGLE_DIM: idx[0]=dimension (-1 = all dims);
                          *_POLYLINE2: (xidx, yidx); PROXIMITY/SIGNED_DISTANCE/
                          CONSTRAINT_PROXIMITY: (x1, y1, x2, y2)                */
  int32_t idx_extra[2]; /* WEIGHTED_CONVEX_PROXIMITY: (v1, v2); else 0          */
  float weight;        /* Cost::weight_                                        */
  float value;         /* nominal_ or threshold_                               */
  float value2;        /* ROUTE_PROGRESS: initial_route_pos_; else 0            */
  int32_t flags;       /* ILQG_FLAG_*                                          */
  int32_t polyline;    /* index into the polyline table or -1                  */
  int32_t child_begin; /* EXTREME_VALUE: first child term index                */
  int32_t child_count; /* EXTREME_VALUE: number of children                    */
  int32_t constraint_slot; /* constraints: index into the per-instance lambda table, else -1 */
  int32_t first_step;  /* FinalTimeCost (include/ilqgames/cost/final_time_cost.h:55-88): the term is zero (value
                          and derivatives) before this time step — the smallest k with k * dt >= threshold_time,
                          times taken relative to the start of the window.  0 = always active. */
} ilqg_cost_term;

typedef enum { ILQG_SUM = 0, ILQG_MAX = 1, ILQG_MIN = 2 } ilqg_cost_structure;

/* PlayerCost ctor arguments + cost structure (include/ilqgames/cost/player_cost.h:63-109). */
typedef struct {
  float state_regularization;
  float control_regularization;
  int32_t structure; /* ilqg_cost_structure */
} ilqg_player_cost;

/* SolverParams (include/ilqgames/solver/solver_params.h:50-84). */
typedef struct {
  float convergence_tolerance;
  int32_t max_solver_iters;
  int32_t linesearch;
  float initial_alpha_scaling;
  float geometric_alpha_scaling;
  int32_t max_backtracking_steps;
  float expected_decrease_fraction;
  int32_t open_loop;
  int32_t unconstrained_solver_max_iters;
  float geometric_mu_scaling;
  float geometric_mu_downscaling;
  float geometric_lambda_downscaling;
  float constraint_error_tolerance;
} ilqg_solver_params;

typedef struct {
  int32_t num_players;
  ilqg_subsystem subsystems[ILQG_MAX_PLAYERS];
  ilqg_player_cost player_costs[ILQG_MAX_PLAYERS];
  int32_t num_terms;
  const ilqg_cost_term* terms;     /* host array                             */
  int32_t num_polylines;
  const int32_t* polyline_offsets; /* host, num_polylines+1, in points       */
  const float* polyline_points;    /* host, 2 floats per point               */
  int32_t T;                       /* time::kNumTimeSteps (types.h:141-142)  */
  double dt;                       /* time::kTimeStep     (types.h:135)      */
  int32_t dtype;                   /* ilqg_dtype of state/gain arithmetic    */
  ilqg_solver_params params;
  int32_t num_dense_params;        /* coefficients of the affine constraints  */
  const float* dense_params;       /* host array (may be NULL when there are none) */
} ilqg_problem_desc;

void ilqg_default_solver_params(ilqg_solver_params* p);

typedef struct ilqg_problem ilqg_problem;

/* Builds the device-side tables of one Problem (what Problem::Initialize +
 * ILQSolver::ILQSolver set up, include/ilqgames/solver/problem.h:66-73,
 * include/ilqgames/solver/ilq_solver.h:69-95).
 * A handle also owns the four round counters its solves report through (device + pinned host copy, allocated
 * here): like the reference's solver objects it serves one solve at a time — concurrent solves need one handle
 * each (the read-only entry points, e.g. rollout / linearize / quadraticize / strategy costs, may share one). */
ilqg_status ilqg_problem_create(const ilqg_problem_desc* desc, ilqg_problem** out);
void ilqg_problem_destroy(ilqg_problem* p);

/* ---- Per-instance parameters -------------------------------------------------------------------------------------
 * A batch is thousands of games in one launch; by default they differ in x0 (and warm start) alone.  With a value table
 * bound to the handle, instance b of every later call evaluates the declared terms with row b of the table in place of
 * ilqg_cost_term::weight / value — different goals, nominal speeds, weights and thresholds in one batch.  The reference
 * has no counterpart: one Problem there is one game.
 *
 * The table is bound to the PROBLEM because ilqg_solve_again_batch, ilqg_quadraticize_batch, ilqg_total_costs_batch and
 * the Nash checks take no options struct and must all see the same game.  Every entry point that evaluates a cost
 * honours it: ilqg_solve_batch_ex and the three calls that are it (every mode), ilqg_quadraticize_batch,
 * ilqg_total_costs_batch, ilqg_strategy_costs_batch, ilqg_check_local_nash_batch, ilqg_check_sufficient_nash_batch; each
 * of them returns ILQG_ERR_INVALID, before anything is launched, when its `batch` is not the bound one.  Entry points
 * that evaluate no cost (rollout, linearize, the LQ sweeps, receding-horizon shift / sync / splice, plan integrate) are
 * unaffected by cost columns (for subsystem columns see below).  No scheduling choice depends on a binding; the row program (ilqg_problem_row_program) and the static
 * structure it matched are those of the descriptor.
 *
 * Values are float, like the descriptor's, and are converted to the problem's arithmetic where the baked value is: an
 * overridden instance computes, bit for bit, what a problem created with that float in its descriptor computes.
 *
 * What may be declared — `term` indexes ilqg_problem_desc::terms (top-level terms and the children of an EXTREME_VALUE):
 *   kind                                   weight   value
 *   QUADRATIC, SEMIQUADRATIC               yes      yes (nominal / threshold)
 *   SEMIQUADRATIC_POLYLINE2                yes      yes
 *   QUADRATIC_POLYLINE2                    yes      no  (has none)
 *   PROXIMITY, LOCALLY_CONVEX_PROXIMITY,
 *   WEIGHTED_CONVEX_PROXIMITY              yes      yes (threshold)
 *   ORIENTATION, QUADRATIC_NORM,
 *   SEMIQUADRATIC_NORM                     yes      yes
 *   EXPRESSION, CONSTRAINT_EXPRESSION      yes      yes (what its program's PUSH_WEIGHT / PUSH_VALUE push)
 *   QUADRATIC_DIFFERENCE, CURVATURE,
 *   RELATIVE_DISTANCE                      yes      no  (has none)
 *   NOMINAL_PATH_LENGTH, ROUTE_PROGRESS    yes      no  (tabulated per step by ilqg_problem_create; per instance:
 *                                                       "Per-instance TIME NOMINALS" below)
 *   SIGNED_DISTANCE,
 *   POLYLINE2_SIGNED_DISTANCE              no       yes (the weight is not read)
 *   CONSTRAINT_PROXIMITY, _SINGLE_DIMENSION,
 *   _POLYLINE2_SIGNED_DISTANCE             no       yes (threshold; a constraint has no weight)
 *   EXTREME_VALUE                          no       no  (declare its children)
 *   CONSTRAINT_AFFINE_SCALAR / _VECTOR     no       no  (dense coefficient blocks)
 * Anything else — a "no" above, a term index out of range, a field that is not an ilqg_param_field, the same (term,
 * field) twice — is ILQG_ERR_UNSUPPORTED with the term named in ilqg_last_error(); nothing is ever silently ignored.
 * Out of scope: value2, regularisation, ilqg_solver_params::linesearch and ::open_loop (polyline geometry: "Per-instance
 * ROUTES" below; the other solver parameters: "Per-instance SOLVER parameters" below).
 *
 * Per-instance SUBSYSTEM parameters (ilqg_problem_declare_instance_subsystem_params): ilqg_subsystem::param0 of the
 * declared rows of ilqg_problem_desc::subsystems varies per instance too — fleets of cars with different wheelbases,
 * the robustness of a plan to a Dubins or Air3D speed.  One value table serves both declarations: it is
 * float [batch][cost_count + subsystem_count], the cost columns first in their declared order, and column
 * cost_count + c replaces param0 of subsystems[c] for that instance.  Either declaration may be made first; together
 * they hold at most ILQG_MAX_INSTANCE_PARAMS columns.
 *   kind                                   param0
 *   CAR_5D, CAR_6D, CAR_7D                 yes (inter-axle distance)
 *   DUBINS_CAR, DELAYED_DUBINS_CAR         yes (speed)
 *   AIR_3D_EVADER, AIR_3D_PURSUER          yes (their speeds)
 *   UNICYCLE_4D, UNICYCLE_4D_DISTURBED,
 *   PLANAR_DISTURBANCE, POINT_MASS_2D,
 *   UNICYCLE_5D                            no  (the kind reads no param0)
 * A "no", a row out of range or the same row twice is ILQG_ERR_UNSUPPORTED with "subsystem <row>" and the kind named in
 * ilqg_last_error().  With a subsystem column declared and a table bound, the entry points that integrate or linearise
 * read the table as well — ilqg_rollout_batch, ilqg_linearize_batch, ilqg_receding_horizon_shift_batch / _sync_batch,
 * ilqg_plan_integrate_batch — and return ILQG_ERR_INVALID before any launch when their `batch` is not the bound one;
 * the cost-evaluating entry points above honour both kinds of column.  The LQ sweeps and the splice read no parameter.
 * The same bit-for-bit rule holds: an instance computes what a problem created with that float as param0 computes.
 * VALUES ARE NOT VALIDATED: the table lives on the device and may be rewritten between calls, so a zero wheelbase gives
 * what a descriptor with a zero wheelbase gives (a division by zero in the car models).
 *
 * Per-instance SOLVER parameters (ilqg_problem_declare_instance_solver_params): the declared members of
 * ilqg_problem_desc::params vary per instance — a sweep over (initial step, geometric scaling, Armijo fraction,
 * back-tracking depth), over the stopping rule, or over the augmented-Lagrangian schedule in ONE batch, with success,
 * iteration and back-tracking statistics per vector from one solve.  The solver columns are a third group of the same
 * value table: it is float [batch][cost_count + subsystem_count + solver_count], the solver columns last in their
 * declared order.  The three declarations may be made in any order; together they hold at most
 * ILQG_MAX_INSTANCE_PARAMS columns.  Every member may be declared but `linesearch` and `open_loop`, which select kernels
 * and the host's schedule: they, a number that is no ilqg_solver_field and the same field twice are
 * ILQG_ERR_UNSUPPORTED with the field named in ilqg_last_error().
 * The same bit-for-bit rule holds: an instance computes what a problem created with that float in
 * ilqg_problem_desc::params computes; a float member is converted to the handle's arithmetic where the baked one is.
 * The table is READ AT EVERY LATER SOLVE on the handle — ilqg_solve_batch_ex and the three calls that are it, in every
 * mode, and ilqg_solve_again_batch — and may be rewritten between calls in stream order.  ONLY THE SOLVES read solver
 * columns: every other entry point ignores them.  The "bound for a batch of N" refusals are what they are without
 * solver columns: a cost-evaluating call on another batch is refused while a value table is bound, whatever columns it
 * holds.  No scheduling choice depends on a binding — the host cannot see the device table — so the round plans, the
 * probing heuristics and the capacity of the iterate log keep using the descriptor's values, and therefore:
 * THE DESCRIPTOR'S VALUE OF AN INTEGER MEMBER IS A CEILING.  max_solver_iters, max_backtracking_steps and
 * unconstrained_solver_max_iters travel as floats; an instance's value is the float truncated to an integer and limited
 * on the device to [0, the descriptor's value] whatever the float holds (a NaN or anything at or above the descriptor's
 * value gives the descriptor's value, anything negative 0).  A caller sets the ceiling in the descriptor and sweeps
 * below it.  Everything else follows VALUES ARE NOT VALIDATED above. */
typedef enum {
  ILQG_SOLVER_CONVERGENCE_TOLERANCE = 0,
  ILQG_SOLVER_MAX_SOLVER_ITERS = 1,
  ILQG_SOLVER_LINESEARCH = 2, /* not declarable: named so that it is refused by name */
  ILQG_SOLVER_INITIAL_ALPHA_SCALING = 3,
  ILQG_SOLVER_GEOMETRIC_ALPHA_SCALING = 4,
  ILQG_SOLVER_MAX_BACKTRACKING_STEPS = 5,
  ILQG_SOLVER_EXPECTED_DECREASE_FRACTION = 6,
  ILQG_SOLVER_OPEN_LOOP = 7, /* not declarable: named so that it is refused by name */
  ILQG_SOLVER_UNCONSTRAINED_SOLVER_MAX_ITERS = 8,
  ILQG_SOLVER_GEOMETRIC_MU_SCALING = 9,
  ILQG_SOLVER_GEOMETRIC_MU_DOWNSCALING = 10,
  ILQG_SOLVER_GEOMETRIC_LAMBDA_DOWNSCALING = 11,
  ILQG_SOLVER_CONSTRAINT_ERROR_TOLERANCE = 12
} ilqg_solver_field; /* the members of ilqg_solver_params, in their order */
#define ILQG_NUM_SOLVER_FIELDS 13
typedef enum { ILQG_PARAM_WEIGHT = 0, ILQG_PARAM_VALUE = 1 } ilqg_param_field;
typedef struct {
  int32_t term;  /* index into ilqg_problem_desc::terms */
  int32_t field; /* ilqg_param_field */
} ilqg_instance_param;
#define ILQG_MAX_INSTANCE_PARAMS 256

/* Which (term, field) pairs vary per instance: column c of the value table overrides params[c].  count = 0 clears the
 * declaration.  ILQG_ERR_INVALID while a table is bound (unbind first). */
ilqg_status ilqg_problem_declare_instance_params(ilqg_problem* p, int32_t count, const ilqg_instance_param* params);
/* values: device float [batch][cost_count + subsystem_count + solver_count], or NULL to unbind.  The table is READ AT EVERY LATER CALL on this handle, not
 * copied: the caller may rewrite it between calls (in stream order with them) and keeps it alive while it is bound.
 * ILQG_ERR_INVALID without a declaration, or with batch <= 0. */
ilqg_status ilqg_problem_bind_instance_values(ilqg_problem* p, int32_t batch, const float* values);
/* Host only, no device needed: the checks of the declare call against a descriptor. */
ilqg_status ilqg_instance_params_check(const ilqg_problem_desc* desc, int32_t count, const ilqg_instance_param* params);
/* Which subsystems' param0 vary per instance: subsystems[c] is a row of ilqg_problem_desc::subsystems, and column
 * cost_count + c of the value table overrides its param0.  count = 0 clears the subsystem declaration.  ILQG_ERR_INVALID
 * while a table is bound (unbind first), or when cost and subsystem columns together exceed ILQG_MAX_INSTANCE_PARAMS. */
ilqg_status ilqg_problem_declare_instance_subsystem_params(ilqg_problem* p, int32_t count, const int32_t* subsystems);
/* Host only, no device needed: the checks of the declare call against a descriptor (the total with the cost columns is
 * the handle's to check). */
ilqg_status ilqg_instance_subsystem_params_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* subsystems);
/* Which members of ilqg_problem_desc::params vary per instance: fields[c] is an ilqg_solver_field, and column
 * cost_count + subsystem_count + c of the value table overrides it.  count = 0 clears the solver declaration.
 * ILQG_ERR_INVALID while a table is bound (unbind first), or when the three groups together exceed
 * ILQG_MAX_INSTANCE_PARAMS. */
ilqg_status ilqg_problem_declare_instance_solver_params(ilqg_problem* p, int32_t count, const int32_t* fields);
/* Host only, no device needed: the checks of the declare call (the total with the other columns is the handle's). */
ilqg_status ilqg_instance_solver_params_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* fields);

/* Per-instance ROUTES: the points of the declared polylines of the descriptor — lanes, boundaries, the polygon of a
 * signed-distance term — vary per instance — the same intersection with the turn lane bent differently in every game of
 * a batch.  Only the coordinates vary: instance b's polyline q has the descriptor's number of points.  The row program,
 * the static structure it matched and every scheduling choice are those of the descriptor.
 *   declare   polylines[c] indexes the descriptor's polylines.  An index out of range, the same polyline twice, or a
 *             polyline a ROUTE_PROGRESS term refers to (its per-step nominals are tabulated from the baked polyline by
 *             ilqg_problem_create) is ILQG_ERR_UNSUPPORTED with the polyline (and the term) named in ilqg_last_error().
 *             count = 0 clears the declaration.  ILQG_ERR_INVALID while a route table is bound (unbind first).
 *   bind      points: device float [batch][P][2], P the sum of the declared polylines' point counts in declaration order;
 *             row b holds instance b's points.  NULL unbinds.  ILQG_ERR_INVALID without a declaration or with batch <= 0.
 * THE POINTS ARE CONSUMED BY THE BIND CALL, unlike the value table, which is read at every call: the call builds, on
 * `stream`, a table the handle owns — every instance's segments with their derived scalars, batch * total segments * 21
 * elements in the problem's precision, allocated here and freed at unbind or ilqg_problem_destroy — and later calls read
 * that table, not `points`.  A caller who rewrites the points binds again (a table of the same batch is rewritten in
 * place); later calls on the handle must run in stream order after the bind.  `points` may be released once the bind has
 * run on its stream.
 * Independent of ilqg_problem_bind_instance_values: either, both or neither may be bound, in any order; when both are
 * bound their batches must agree (ILQG_ERR_INVALID from the second bind).  The calls that evaluate costs (the list
 * above: the solves, quadraticize, total_costs, strategy costs, both Nash checks) read the table and return
 * ILQG_ERR_INVALID before any launch when their `batch` is not the bound one; the others ignore a route binding.
 * An instance computes, bit for bit, what a problem created with its points in the descriptor computes.  COORDINATES ARE
 * NOT VALIDATED: a zero-length segment gives what a descriptor with one gives. */
ilqg_status ilqg_problem_declare_instance_routes(ilqg_problem* p, int32_t count, const int32_t* polylines);
ilqg_status ilqg_problem_bind_instance_routes(ilqg_problem* p, int32_t batch, const float* points, void* stream);
/* Host only, no device needed: the checks of the declare call against a descriptor. */
ilqg_status ilqg_instance_routes_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* polylines);

/* Per-instance TIME NOMINALS: a reference trajectory for each game.  The two time-dependent kinds track a per-step
 * nominal — NOMINAL_PATH_LENGTH a scalar t_k * speed on one state dimension, ROUTE_PROGRESS the point of its polyline at
 * pos0 + t_k * speed on a position pair — which ilqg_problem_create tabulates into [tables][T][2] doubles (the second
 * entry of a NOMINAL_PATH_LENGTH pair is 0 and is not read).  `tables` is the number of time-dependent terms of the
 * descriptor, and table q belongs to the q-th such term in ilqg_problem_desc::terms order
 * (ilqg_problem_time_nominal_terms).  A bound table replaces the tabulated one per instance: K candidate ego
 * trajectories against the same other agents, a speed profile per vehicle, a moving way-point per scene, the shifted
 * reference of every replan.
 *   bind      nominals: device double [batch][tables][T][2], or NULL to unbind; instance b tracks block b.  There is no
 *             declaration step: the table covers every time-dependent term, and a caller who varies only some fills the
 *             rest from the baked table (ilqg_time_nominal_table_build).  The table is READ AT EVERY LATER CALL on this
 *             handle and never copied, like the value table: the caller keeps it alive while it is bound and may rewrite
 *             it in place between calls, in stream order with them (a receding-horizon caller shifts its reference
 *             between replans).  ILQG_ERR_INVALID when the problem has no time-dependent term, with batch <= 0, or when
 *             a value table or a route table is bound with another batch (and likewise from those binds while this
 *             table is bound): any of the three may be bound, in any order, with one batch.
 *   build     ilqg_instance_time_nominals_build fills such a table on `stream` from speed_pos: device
 *             float [batch][tables][2] = (nominal speed, initial route position); the second entry is ignored for a
 *             NOMINAL_PATH_LENGTH term.  Block b is, bit for bit, what a problem created with those two floats as the
 *             term's value / value2 tabulates, on the handle's baked polylines in the handle's precision; the caller
 *             then binds `nominals` (it is not bound by this call).  Any other reference is the caller's to write.
 * The calls that evaluate costs read the bound table — ilqg_solve_batch_ex and the three calls that are it (every mode),
 * ilqg_solve_again_batch, ilqg_quadraticize_batch, ilqg_total_costs_batch, ilqg_strategy_costs_batch,
 * ilqg_check_local_nash_batch, ilqg_check_sufficient_nash_batch — and return ILQG_ERR_INVALID before any launch when
 * their `batch` is not the bound one.  Rollout, linearize, the LQ sweeps and the receding-horizon integration calls
 * ignore the binding.  No scheduling choice looks at it; the row program and the static match stay the descriptor's.
 * VALUES ARE NOT VALIDATED, on the device: where ilqg_problem_create returns ILQG_ERR_INVALID for a route position that
 * turns negative over the horizon (and the host-only builder below does too), the device builder lets a negative or NaN
 * route position take segment 0 — it extrapolates backwards along the first segment — and a position past the last
 * segment extrapolates along the last, as the descriptor path does.
 * Unchanged: a per-instance `value` column for these two kinds is still ILQG_ERR_UNSUPPORTED, and so is a per-instance
 * route for a polyline that a ROUTE_PROGRESS term refers to (the device builder reads the baked polylines). */
ilqg_status ilqg_problem_bind_instance_time_nominals(ilqg_problem* p, int32_t batch, const double* nominals);
ilqg_status ilqg_instance_time_nominals_build(const ilqg_problem* p, int32_t batch, const float* speed_pos, double* nominals,
                                              void* stream);
/* Which term owns table q: terms_out[q] indexes ilqg_problem_desc::terms.  *tables is the table count (0: the problem
 * has no time-dependent term); terms_out may be NULL to query it. */
ilqg_status ilqg_problem_time_nominal_terms(const ilqg_problem* p, int32_t* terms_out, int32_t capacity, int32_t* tables);

/* Bytes of device workspace a solve of `batch` instances needs: the per-instance iterates, linearisations and
 * loop states, the lists of back-tracking instances and the pool of the speculative line search.  A solve
 * allocates nothing. */
ilqg_status ilqg_workspace_bytes(const ilqg_problem* p, int32_t batch, uint64_t* bytes);

/* ------------------------------------------------------------------------ *
 *  Hot-path stages (each also usable on its own; all batched)               *
 * ------------------------------------------------------------------------ */

/* Replaces ILQSolver::CurrentOperatingPoint (src/ilq_solver.cpp:174-206):
 * closed-loop rollout from x0 under u_i = u_ref_i - P_i (x - x_ref) - alpha_i
 * with the RK4(2 sub-steps) integrator of
 * src/multi_player_dynamical_system.cpp:52-77.
 *  x0 [B][n]; xs_ref [B][T][n]; us_ref [B][T][m]; P [B][T][m*n]; alpha [B][T][m]
 *  alpha_scale [B] or NULL (=1): step size applied to alpha on the fly (the
 *  reference scales alphas destructively, ilq_solver.cpp:66-72,314,339)
 *  xs [B][T][n], us [B][T][m] outputs.  active [B] int32 mask or NULL. */
ilqg_status ilqg_rollout_batch(const ilqg_problem* p, int32_t batch,
                               const void* x0, const void* xs_ref,
                               const void* us_ref, const void* P,
                               const void* alpha, const void* alpha_scale,
                               void* xs, void* us, const int32_t* active,
                               void* stream);

/* Replaces ILQSolver::ComputeLinearization (src/ilq_solver.cpp:437-455) ->
 * ConcatenatedDynamicalSystem::Linearize (src/concatenated_dynamical_system.cpp:86-107).
 *  A [B][T][n*n], Bm [B][T][n*m].
 * The stage entry points (this one, ilqg_quadraticize_batch, ilqg_total_costs_batch, ilqg_rollout_batch) run the same
 * compile-time-dimensioned kernels as the solves: a problem whose (n, N, m_i) is not among the library's
 * instantiations, or whose players' control dimensions differ, gets ILQG_ERR_UNSUPPORTED here too. */
ilqg_status ilqg_linearize_batch(const ilqg_problem* p, int32_t batch,
                                 const void* xs, const void* us, void* A,
                                 void* Bm, const int32_t* active, void* stream);

/* Replaces ILQSolver::ComputeCostQuadraticization (src/ilq_solver.cpp:471-490)
 * -> PlayerCost::Quadraticize (src/player_cost.cpp:194-225).
 *  lambdas [B][num_constraints][T] or NULL; mu [B] or NULL (constraint.h:98-117)
 *  t_extreme [B][N] int32 or NULL: time of extreme cost for MAX/MIN players.
 *  Q,l,R,r: layouts of ilqg_lq_feedback_batch, pair order = ilqg_problem_pairs. */
ilqg_status ilqg_quadraticize_batch(const ilqg_problem* p, int32_t batch,
                                    const void* xs, const void* us,
                                    const void* lambdas, const void* mu,
                                    const int32_t* t_extreme, void* Q, void* l,
                                    void* R, void* r, const int32_t* active,
                                    void* stream);

/* The (i,j) control blocks PlayerCost::Quadraticize creates for this problem. */
ilqg_status ilqg_problem_pairs(const ilqg_problem* p, ilqg_pair* pairs_host,
                               int32_t* npairs);

/* Replaces ILQSolver::TotalCosts (src/ilq_solver.cpp:220-257).
 *  costs [B][N]; t_extreme [B][N] int32 (written for MAX/MIN players). */
ilqg_status ilqg_total_costs_batch(const ilqg_problem* p, int32_t batch,
                                   const void* xs, const void* us, void* costs,
                                   int32_t* t_extreme, const int32_t* active,
                                   void* stream);

/* ------------------------------------------------------------------------ *
 *  Whole iterative-LQ solve                                                 *
 * ------------------------------------------------------------------------ */

/* Replaces ILQSolver::Solve (src/ilq_solver.cpp:76-172) for `batch`
 * independent instances that share one Problem definition and differ in x0
 * (and warm start).
 *  x0        [B][n]        Problem::InitialState per instance
 *  xs, us    [B][T][n|m]   in: warm-start operating point; out: final one
 *  P, alpha  [B][T][..]    in: warm-start strategies; out: final strategies
 *                          (alpha carries the accepted step scaling, as the
 *                          strategies the reference logs do)
 *  total_costs [B][N]      ILQSolver::TotalCosts of the final iterate
 *  iters     [B] int32     outer iterations performed
 *  status    [B] int32     1 = success flag true (src/ilq_solver.cpp:169),
 *                          0 = line-search failure (:146-155)
 *  converged [B] int32     has_converged at exit
 *  workspace               device scratch of ilqg_workspace_bytes() bytes
 *  fixed_iters > 0 runs exactly that many outer iterations per instance
 *  ignoring convergence (throughput benchmarking); 0 = reference semantics. */
ilqg_status ilqg_ilq_solve_batch(ilqg_problem* p, int32_t batch, const void* x0,
                                 void* xs, void* us, void* P, void* alpha,
                                 void* total_costs, int32_t* iters,
                                 int32_t* status, int32_t* converged,
                                 void* workspace, int32_t fixed_iters,
                                 void* stream);

/* Everything a solve call can be told beyond its buffers (ilqg_solve_batch_ex).  The scheduling choices select among
 * device schedules of the SAME arithmetic: split_trial / handoff / probe / counted / compact_rows / round_bursts are
 * bit-identical with each other; single_wave_sweep and adjoint_expected_decrease run the same recursion as a different
 * instruction stream (sums in another order), i.e. the same results to rounding — and ILQG_CHOICE_AUTO picks them from
 * the batch size (five or more instances per CU), so an instance's last bits, and with them a line-search decision that
 * sits on a rounding threshold, can depend on the size of the batch it is solved in.  Set `deterministic` (or pin the two
 * choices ON / OFF) for results that must not; ilqg_problem_last_schedule says what the last solve ran.
 * single_wave_sweep = ON is a request: shapes the single-wave form is not built for (players with one control, n >= 16,
 * compact rows wider than its staging row) run the player-parallel sweep, and ilqg_problem_last_schedule reports it.
 * ilqg_default_solve_options fills the defaults: reference semantics, every choice ILQG_CHOICE_AUTO. */
typedef struct {
  int32_t fixed_iters;          /* > 0: exactly that many outer iterations per instance, convergence not tested   */
  int32_t augmented_lagrangian; /* 1: AugmentedLagrangianSolver::Solve around the inner solves                     */
  int32_t resume;               /* 1: GameSolver::Solve called again on the same solver object: the workspace
                                      holds the previous call's state (last_merit_function_value_)               */
  int32_t deterministic;        /* 1: every ILQG_CHOICE_AUTO below resolves to a schedule that does not depend on the
                                      batch size (the player-parallel sweep and its forward-pass expected decrease at
                                      every batch): an instance's result is the same bits whatever batch it is solved in
                                      (tests/test_gpu_single_wave.py).  Costs the large-batch throughput form.  (This
                                      field was reserved0 = 0 up to ABI 6: same layout.)                              */
  const int32_t* active;        /* [B] device int32 or NULL: instances with 0 are skipped, their buffers untouched.
                                     A free-running solve (which waits for the device every round anyway) counts the
                                     mask first and lets every ILQG_CHOICE_AUTO below go by the instances taking part,
                                     not by B; fixed_iters > 0 without the augmented Lagrangian stays asynchronous and
                                     goes by B.                                                                        */
  const void* forced_steps;     /* [B][fixed_iters] device (problem dtype) or NULL.  Test mode: iteration q of
                                      instance b scales its strategies by forced_steps[b][q], integrates and
                                      quadraticises once and ACCEPTS, whatever CheckArmijoCondition says — the
                                      loop's only data-dependent branch is gone, so iterates can be compared one
                                      by one with a CPU run given the same steps.  Needs fixed_iters > 0, no AL.   */
  int32_t split_trial;          /* ilqg_choice: the trial pass as three launches (integrate / rows / decide)        */
  int32_t handoff;              /* ilqg_choice: back-tracking instances leave the fused kernel for split passes     */
  int32_t probe;                /* ilqg_choice: speculative line search over the next step sizes of listed instances */
  int32_t counted;              /* ilqg_choice: host counts the rounds of a fixed-iteration solve as well           */
  int32_t compact_rows;         /* ilqg_choice: the row stage hands the sweep only the touched words of [Q|l|R|r]   */
  int32_t round_bursts;         /* ilqg_choice: free-running solves read their counters back once per burst of rounds */
  int32_t generic_kernels;      /* ilqg_choice: ILQG_CHOICE_ON runs the run-time-dimensioned kernels (what every shape
                                     without a specialised instantiation runs on) for this problem too */
  int32_t probe_first;          /* speculative line search: step sizes probed per listed instance in the first round of
                                     a tail (doubling every round up to 128, as many as the pool holds); 0 = the library's
                                     choice.  Same decisions whatever the value.                                       */
  int32_t single_wave_sweep;    /* ilqg_choice: the one-tile feedback sweep with one wave per instance (twice the instances
                                     per CU; the library picks it for batches of five or more instances per CU)           */
  int32_t adjoint_expected_decrease; /* ilqg_choice: the single-wave sweep forms ILQSolver::ExpectedDecrease itself, by an
                                     adjoint recursion inside the sweep, instead of leaving scratch rows for a forward pass
                                     in the next trial pass (AUTO: where the trial pass is split and has no wave to spare
                                     for one).  Same value up to the order of summation.                                */
  int32_t static_rows;          /* ilqg_choice: a problem whose row program matches a registered structure
                                     (ilqg_problem_row_program) runs the linearise / quadraticise stage of the fused trial
                                     kernel as straight-line code compiled for that structure instead of interpreting the
                                     program (AUTO: on).  Bit-identical.                                                */
  int32_t padded_sweep;         /* ilqg_choice: a solve on the run-time-dimensioned kernels runs its Riccati sweep on the
                                     specialised sweep of the smallest instantiated shape the game embeds in (same player
                                     count, at least its states and its widest control; added states are inert, added
                                     controls have a zero column of B and a unit entry of R_ii and solve to exact zeros).
                                     AUTO: on for problems without an instantiation of their own; ON where no shape holds
                                     the game is ILQG_ERR_UNSUPPORTED.  The same recursion on another elimination order:
                                     results to rounding.  (This field was reserved1 = 0 up to ABI 7: same layout.)        */
  int32_t probe_lanes;          /* ilqg_choice: the probing rollouts of the speculative line search with a lane per
                                     (candidate, subsystem) — 64 / N candidates of an instance per wavefront, the RK4 stages
                                     of a step one after the other in the lane — instead of two candidates per wavefront
                                     with a lane per stage: an eighth of the instructions per rollout, a longer chain per
                                     step (AUTO: rounds with more rollouts than the chip holds at once, eight or more
                                     candidates per instance).  Bit-identical trajectories.  (ABI 8)                      */
  int32_t sweep_forms;          /* ilqg_choice: the one-tile feedback sweeps (player-parallel and single-wave) run the
                                     m x m Nash solve of a step with DPP row broadcasts — the pivot columns replicated in
                                     every 16-lane row, values stay in vector registers — instead of read-lane broadcasts
                                     over the scalar unit (AUTO: on wherever the columns fit the rows: m < 16 and
                                     n + 1 <= 4 (16 - m)).  The same operations in the same order: bit-identical.
                                     With the forms on, the player-parallel sweep of a shape with n < 16 and two controls
                                     per player also takes B's entries from registers instead of a tile wherever B is
                                     constant entries with at most one per row and per column (dt x a selection matrix:
                                     ilqg_sweep_b_structure_build says whether; ILQG_SCHEDULE_CONSTANT_B reports it): G, S
                                     and F = A - B P are then one multiply or multiply-add per entry.  Every replaced
                                     sum had a single term that is not an exact zero, so the results are the same bits
                                     for finite operands, up to the sign of a zero; an infinite Z or P no longer turns
                                     into NaN through 0 x Inf.  OFF keeps the read-lane, dense-B instantiation selectable
                                     for A/B runs and the bit-for-bit tests (tests/test_gpu_sweep_forms.py,
                                     tests/test_gpu_sweep_b_structure.py).  (This field was reserved2 = 0 up to ABI 9's
                                     first release: same layout, same ABI version.)                                      */
  const struct ilqg_iterate_log* iterate_log; /* NULL, or where every logged iterate of the solve goes (below)          */
  double max_runtime;           /* > 0: the anytime exit of ILQSolver::Solve (src/ilq_solver.cpp:123-124) on the host's
                                     clock, seconds — once it has passed, instances leave the loop at their next
                                     iteration boundary with success = 1 and the iterate they hold (a line search in
                                     flight is finished first, as there).  <= 0: run to the iteration bounds.  Needs a
                                     free-running solve (fixed_iters = 0, no forced steps).  With the augmented-Lagrangian
                                     loop (src/augmented_lagrangian_solver.cpp:85-110,193) every inner solve of a constrained
                                     problem gets max_runtime / max_solver_iters, and the outer loop has its own clock: it
                                     starts at that allowance, adds the wall time of every outer iteration (its own
                                     LoopTimer, kept in the problem handle) and starts no further inner solve once
                                     elapsed >= max_runtime - RuntimeUpperBound() — a batch shares the clock. */
} ilqg_solve_options;

/* What SolverLog::AddSolverIterate receives per iterate (include/ilqgames/utils/solver_log.h:65-74: the reference deep-
 * copies operating point, strategies and total costs at src/ilq_solver.cpp:111 and :164).  On the device the copies are
 * optional: a solve given a log writes iterate q of instance b — q = 0 is the initial rollout, then one per accepted
 * step; with the augmented-Lagrangian loop the iterates of successive inner solves follow one another as in
 * src/augmented_lagrangian_solver.cpp:94,185 — to slot q of that instance while q < capacity, and counts them.
 * All arrays are device memory in the problem's dtype. */
typedef struct ilqg_iterate_log {
  void* xs;       /* [B][capacity][T][n]                                                         */
  void* us;       /* [B][capacity][T][m]                                                         */
  void* costs;    /* [B][capacity][N]     ILQSolver::TotalCosts of the iterate                    */
  void* P;        /* [B][capacity][T][m*n] or NULL: the strategies the iterate was played with    */
  void* alpha;    /* [B][capacity][T][m] or NULL (alpha carries the accepted step, as logged)     */
  int32_t* count; /* [B] out: iterates the solve produced (may exceed capacity: those were dropped) */
  int32_t capacity;
} ilqg_iterate_log;
void ilqg_default_solve_options(ilqg_solve_options* o);

/* ilqg_ilq_solve_batch / ilqg_al_solve_batch / ilqg_solve_again_batch are this call with the matching options. */
ilqg_status ilqg_solve_batch_ex(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                void* alpha, void* total_costs, int32_t* iters, int32_t* status, int32_t* converged,
                                void* workspace, const ilqg_solve_options* options, void* stream);

/* The loop state a solve left in its workspace, per instance (what ILQSolver keeps in members / locals):
 * last_merit_function_value_ (ilq_solver.h:189), the last expected decrease (:303), the step size of the last
 * accepted trial and the number of steps the solve's line searches rejected in total.  Outputs are device arrays [B] (problem dtype; int32
 * for backtracks), any may be NULL.  `augmented_lagrangian` must be what the solve was called with. */
ilqg_status ilqg_solve_state_batch(const ilqg_problem* p, int32_t batch, const void* workspace,
                                   int32_t augmented_lagrangian, void* last_merit, void* expected_decrease,
                                   void* step, int32_t* backtracks, void* stream);

/* Which device schedule the problem's last solve ran (bits below), so that a caller can tell two runs apart whose results
 * differ in the last bits because ILQG_CHOICE_AUTO chose differently for their batch sizes. */
#define ILQG_SCHEDULE_SINGLE_WAVE_SWEEP 1   /* one wave per instance (else: one wave per player)                  */
#define ILQG_SCHEDULE_ADJOINT_DECREASE 2    /* ExpectedDecrease by the sweep's adjoint recursion                  */
#define ILQG_SCHEDULE_SPLIT_TRIAL 4         /* trial pass as rollout / rows / decision kernels                    */
#define ILQG_SCHEDULE_COMPACT_ROWS 8        /* compact rows between the row stage and the sweep                   */
#define ILQG_SCHEDULE_COUNTED 16            /* host-counted rounds (hand-off, speculative line search)            */
#define ILQG_SCHEDULE_GENERIC 32            /* the run-time-dimensioned kernels                                   */
#define ILQG_SCHEDULE_OPEN_LOOP 64          /* LQOpenLoopSolver's sweep                                           */
#define ILQG_SCHEDULE_STATIC_ROWS 128       /* the row stage ran as straight-line code for a registered structure */
#define ILQG_SCHEDULE_PADDED_SWEEP 256      /* run-time-dimensioned solve, its sweep on a specialised kernel (padded_sweep) */
#define ILQG_SCHEDULE_CONSTANT_B 512        /* player-parallel sweep with B's constant entries in registers (sweep_forms)   */
ilqg_status ilqg_problem_last_schedule(const ilqg_problem* p, int32_t* schedule_out);

/* Host only, no device needed: the schedule a solve of this description would run — every decision the library makes
 * about how a solve runs, from the description, the options and what `query` says about the call and the device.  It runs
 * the function the solve itself runs (csrc/ilqg_schedule.hpp), so `word` is what ilqg_problem_last_schedule reports after
 * that solve; the other members name what the word has no bit for.  Flags are 0 / 1; a problem on the run-time-dimensioned
 * kernels reports its word and zeros. */
typedef struct {
  int32_t batch;         /* instances in the call's buffers                                                       */
  int32_t active;        /* instances its mask (ilqg_solve_options::active) lets take part; -1: no mask            */
  int32_t num_cus;       /* compute units of the device (ilqg_device_info)                                        */
  int32_t tables_bound;  /* per-instance tables are bound to the problem (values, routes or time nominals)        */
  int32_t solver_bound;  /* ... among them per-instance solver columns                                            */
} ilqg_schedule_query;
typedef struct {
  int32_t word;                     /* ILQG_SCHEDULE_* */
  int32_t sched_batch, num_cus;     /* the instances the schedule was chosen for (the mask's count where the solve counts it) */
  int32_t split, counted, handoff, lists, bursts, probe, timed;  /* the rounds: split trial pass, host-counted, hand-off
                                       to split passes, instance lists, bursts of rounds, speculative line search, anytime exit */
  int32_t pairs, lanes_auto, deep_tails, read_restarts, proll_single, proll_lanes;  /* probing rollout forms, AL read-back */
  int32_t probe_max, probe_budget;  /* most candidates per instance and round; rollouts of a tail's first probing round */
  int32_t compact, defer_forward, single_wave, adjoint, b_const, packed;
  int32_t sweep_kind, sweep_forms, sweep_threads;  /* the sweep kernel: its kind (csrc/ilqg_solve.hpp LQ_*), FORMS, threads */
  int32_t prog_kind, bound;         /* row program: 0 plain, 1 expression costs, 2 expression dynamics; the bound twins */
  int32_t static_id, static_prog, static_in_regs;  /* registered structure of the split row kernels / of the fused kernel */
  int32_t decide_solver;            /* the decision kernel's twin that reads per-instance solver columns */
  int32_t rows_cw, row_chunks, lane_width, prio_div, nt_exit, lds_part;
  int32_t lds_trial, lds_roll, lds_rows, lds_decide, lds_proll, lds_proll_single, lds_proll_lanes, lds_prows, lds_sweep,
      lds_exit;                     /* dynamic LDS bytes of each launch (0: the solve has no such launch) */
  int64_t cap;                      /* the iteration bound in rounds */
} ilqg_schedule_info;
ilqg_status ilqg_schedule_build(const ilqg_problem_desc* desc, const ilqg_solve_options* options,
                                const ilqg_schedule_query* query, ilqg_schedule_info* out);

/* The row program ilqg_problem_create compiled the problem's dynamics and cost list into (csrc/ilqg_rowprog.hpp: passes,
 * ops, slot ids, word maps; host memory, int32 words) and the id of the registered structure it matches (0: none — the
 * row stage interprets it).  words_out may be NULL to ask for the size only. */
ilqg_status ilqg_problem_row_program(const ilqg_problem* p, int32_t* words_out, int32_t capacity, int32_t* num_words,
                                     int32_t* static_id);
/* The same straight from a description, on the host alone: everything ilqg_problem_create validates and builds before
 * it uploads tables, without a device (the one entry point that works without one). */
ilqg_status ilqg_row_program_build(const ilqg_problem_desc* desc, int32_t* words_out, int32_t capacity, int32_t* num_words,
                                   int32_t* static_id);
/* Host only, no device needed: everything ilqg_problem_create checks about the ILQG_COST_EXPRESSION or
 * ILQG_CONSTRAINT_EXPRESSION term `term` of a description — its role and placement, its inputs, its block inside dense_params and the program in it (length, opcodes,
 * stack depth).  A refusal names the term, and the op where one is at fault, in ilqg_last_error().  An
 * ILQG_DYN_ROW_EXPRESSION term is checked too — its subsystem, its row, its inputs and its program — and a refusal names
 * the subsystem and the row. */
ilqg_status ilqg_expression_check(const ilqg_problem_desc* desc, int32_t term);
/* Host only, no device needed: what the feedback sweep may assume about B (sweep_forms).  *constant_out is 1 when the
 * problem's solves run on compact rows, every non-zero of B is a constant of the row program (no computed entry) and
 * every row and every column of B holds at most one of them.  entries_out (capacity int32 words; may be NULL to query
 * the count) receives B's constant entries, four words each: row, column, kind (ILQG_B_ENTRY_*), the bits of the float
 * value of a literal; *num_entries is their number. */
#define ILQG_B_ENTRY_LITERAL 0
#define ILQG_B_ENTRY_DT 1      /* the time step */
#define ILQG_B_ENTRY_NEG_DT 2  /* its negative  */
ilqg_status ilqg_sweep_b_structure_build(const ilqg_problem_desc* desc, int32_t* constant_out, int32_t* entries_out,
                                         int32_t capacity, int32_t* num_entries);
/* Host only, no device needed: the segment table ilqg_problem_create builds from the descriptor's polylines — per segment,
 * in polyline order, 21 scalars [p1x p1y p2x p2y length ux uy | the shortcut prev.p1 -> p2 | the shortcut p1 -> next.p2] in
 * the arithmetic of `dtype` (ILQG_F32 / ILQG_F64).  This is also the layout of one instance's block of a per-instance
 * route table.  *num_elems is the element count; out may be NULL to query it. */
ilqg_status ilqg_segment_table_build(const ilqg_problem_desc* desc, int32_t dtype, void* out, int32_t capacity,
                                     int32_t* num_elems);
/* Host only, no device needed: the per-step nominals ilqg_problem_create tabulates for the descriptor's time-dependent
 * terms, double [tables][T][2] in the geometry arithmetic of `dtype` (ILQG_F32 / ILQG_F64) — one instance's block of a
 * per-instance table of time nominals.  *num_elems is the element count (0 without such a term); out may be NULL to
 * query it. */
ilqg_status ilqg_time_nominal_table_build(const ilqg_problem_desc* desc, int32_t dtype, double* out, int32_t capacity,
                                          int32_t* num_elems);

/* Replaces AugmentedLagrangianSolver::Solve (src/augmented_lagrangian_solver.cpp:72-210) with
 * max_runtime = infinity: inner ilqg_ilq_solve_batch calls capped at
 * params.unconstrained_solver_max_iters, multiplier update lambda <- max(0, lambda + mu g) at the
 * final operating point (with the reference's TimeIndex aliasing), mu *= geometric_mu_scaling,
 * warm restart from the last successful inner solve, down-scaling of lambda and mu after a failed
 * one, until the SolverLog would hold max_solver_iters iterates or max g <= constraint_error_tolerance.
 * One (lambda, mu) state per instance replaces the reference's process-global Constraint::mu_.
 *  iters [B]  = number of SolverLog iterates;  status [B] = overall success flag.
 * Same buffers as ilqg_ilq_solve_batch; workspace from ilqg_workspace_bytes. */
ilqg_status ilqg_al_solve_batch(ilqg_problem* p, int32_t batch, const void* x0,
                                void* xs, void* us, void* P, void* alpha,
                                void* total_costs, int32_t* iters,
                                int32_t* status, int32_t* converged,
                                void* workspace, void* stream);

/* Replaces Problem::SetUpNextRecedingHorizon (src/problem.cpp:127-186) with Problem::SyncToExistingProblem
 * (:64-125) and the integrators of src/multi_player_integrable_system.cpp:76-130, for `batch` plans that share
 * one time base: the measured state is integrated forward under the stored strategies by ~planner_runtime, the
 * nearest plan state is found (first subsystem's position distance), the plan is shifted to start there, the
 * tail gets zero strategies / controls and is re-propagated.
 *  x0          [B][n]   measured state at absolute time t0
 *  t0, planner_runtime  the reference's arguments;  plan_t0 = OperatingPoint::t0 of the stored plan
 *  xs, us, P, alpha     in: stored plan (previous solution);  out: warm start of the next solve
 *  x0_next     [B][n]   out: Problem::x0_ of the next solve (Stitch of the nearest plan state and the integrated one)
 *  first_step  [B] int32 out: first_timestep_in_new_problem
 *  new_plan_t0_host     out (host): OperatingPoint::t0 of the shifted plan
 * Invalid times (t0 before the plan, t0 + planner_runtime past its horizon: the reference's CHECKs) return
 * ILQG_ERR_INVALID. */
ilqg_status ilqg_receding_horizon_shift_batch(const ilqg_problem* p, int32_t batch, const void* x0, double t0,
                                              double planner_runtime, double plan_t0, void* xs, void* us,
                                              void* P, void* alpha, void* x0_next, int32_t* first_step,
                                              double* new_plan_t0_host, void* stream);

/* ------------------------------------------------------------------------ *
 *  Receding-horizon harness (examples/receding_horizon_simulator.h:58-60)   *
 * ------------------------------------------------------------------------ *
 * The pieces RecedingHorizonSimulator (src/receding_horizon_simulator.cpp:64-137) strings together, for
 * `batch` instances that share the simulator's clock but each keep their own stored plan.  A stored plan is
 * what SolutionSplicer holds (solver/solution_splicer.h:57-86): T .. T+5 rows, its own start time:
 *  plan_xs/us/P/alpha [B][plan_rows][n | m | m*n | m]   plan_rows >= T + 5
 *  plan_len [B] int32 (device)    rows in use (0 = not constructed yet)
 *  plan_t0  [B] double (device)   OperatingPoint::t0 of the stored plan
 *  active   [B] int32 (device)    1 = instance still running.  Where the reference would leave the loop
 *                                 (ContainsTime false) or CHECK-abort on the times, the instance is
 *                                 cleared instead and left untouched; the batch never aborts. */

/* Replaces MultiPlayerIntegrableSystem::Integrate(t0, t, x0, operating_point, strategies)
 * (src/multi_player_integrable_system.cpp:54-74 with :76-155): x [B][n] is advanced from t_from to t_to under
 * the stored plan's strategies.  Instances whose plan does not satisfy SolutionSplicer::ContainsTime(must_contain)
 * (solution_splicer.h:66-71) are deactivated first — the simulator's loop exits (:89-91, :126). */
ilqg_status ilqg_plan_integrate_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows, const void* plan_xs,
                                      const void* plan_us, const void* plan_P, const void* plan_alpha,
                                      const int32_t* plan_len, const double* plan_t0, double t_from, double t_to,
                                      double must_contain, void* x, int32_t* active, void* stream);

/* Replaces Problem::OverwriteSolution(stored plan) + Problem::SetUpNextRecedingHorizon(x, t, planner_runtime)
 * (src/problem.cpp:127-193, receding_horizon_simulator.cpp:98-103) per instance: like
 * ilqg_receding_horizon_shift_batch, but every instance has its own plan length / start time and the result goes
 * to the next solve's buffers.
 *  x          [B][n]       measured state at time t
 *  xs, us, P, alpha [B][T][..]  out: warm start of the next solve (must not alias the plan)
 *  x0_next    [B][n]       out: Problem::InitialState of the next solve
 *  solve_t0   [B] double   out (device): OperatingPoint::t0 of the next solve
 *  first_step [B] int32    out: first_timestep_in_new_problem, -1 where the times were invalid */
ilqg_status ilqg_receding_horizon_sync_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows,
                                             const void* plan_xs, const void* plan_us, const void* plan_P,
                                             const void* plan_alpha, const int32_t* plan_len, const double* plan_t0,
                                             const void* x, double t, double planner_runtime, void* xs, void* us,
                                             void* P, void* alpha, void* x0_next, double* solve_t0,
                                             int32_t* first_step, int32_t* active, void* stream);

/* Replaces SolutionSplicer::SolutionSplicer(log) (src/solution_splicer.cpp:56-58; instances with plan_len == 0)
 * and SolutionSplicer::Splice(log) (:60-129; instances with converged != 0, receding_horizon_simulator.cpp:133):
 * up to five rows of the old plan in front of the solution's start are kept, the solution follows.
 *  xs, us, P, alpha [B][T][..] the solve's final operating point / strategies, solve_t0 [B] its start time
 *  converged, active [B] int32 (device), either may be NULL (= all ones) */
ilqg_status ilqg_solution_splice_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows, void* plan_xs,
                                       void* plan_us, void* plan_P, void* plan_alpha, int32_t* plan_len,
                                       double* plan_t0, const void* xs, const void* us, const void* P,
                                       const void* alpha, const double* solve_t0, const int32_t* converged,
                                       const int32_t* active, void* stream);

/* GameSolver::Solve called AGAIN on the same solver object (the simulator reuses one, :75,108): like
 * ilqg_ilq_solve_batch / ilqg_al_solve_batch (augmented_lagrangian != 0), except that
 * ILQSolver::last_merit_function_value_ (solver/ilq_solver.h:189) starts from what the previous call on this
 * `workspace` left instead of infinity.  The workspace must come from a previous solve of the same kind and
 * batch.  Constraint multipliers are indexed relative to the start of each window, as in a first solve.
 * active [B] int32 (device, nullable): instances with 0 are skipped, their buffers and outputs left as they are. */
ilqg_status ilqg_solve_again_batch(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                   void* alpha, void* total_costs, int32_t* iters, int32_t* status,
                                   int32_t* converged, void* workspace, int32_t augmented_lagrangian,
                                   const int32_t* active, void* stream);

/* ------------------------------------------------------------------------ *
 *  Equilibrium checks                                                       *
 * ------------------------------------------------------------------------ */

/* Replaces ComputeStrategyCosts (src/compute_strategy_costs.cpp:61-106): the cost every player accumulates when
 * the strategies (P, alpha) are played from x0 against the operating point (xs, us) — closed loop, or with
 * open_loop != 0 as u = u_ref - alpha with state costs taken at the next state (PlayerCost::EvaluateOffset,
 * src/player_cost.cpp:175-190).  euler != 0: one-step Euler integration
 * (MultiPlayerIntegrableSystem::IntegrateUsingEuler), else the default RK4.  costs [B][N]. */
ilqg_status ilqg_strategy_costs_batch(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                      const void* us, const void* P, const void* alpha, int32_t open_loop,
                                      int32_t euler, void* costs, void* stream);

/* Replaces NumericalCheckLocalNashEquilibrium (src/check_local_nash_equilibrium.cpp:60-133): every entry of every
 * alpha_i[k], k < T-1, is moved by -/+ max_perturbation in turn (Euler integration, as there) and the mover's cost
 * compared with the nominal one — 2 m (T-1) rollouts per instance, all in one launch.
 *  is_nash [B] int32   1 = no unilateral move lowered its mover's cost
 *  margin  [B]         out (nullable): min over moves of (moved cost - nominal cost) of the mover */
ilqg_status ilqg_check_local_nash_batch(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                        const void* us, const void* P, const void* alpha, double max_perturbation,
                                        int32_t open_loop, int32_t* is_nash, void* margin, void* stream);

/* Replaces CheckSufficientLocalNashEquilibrium (src/check_local_nash_equilibrium.cpp:144-201): every player's full
 * PlayerCost::Quadraticize at every step of the operating point (xs, us) has Q_i and all its R_ij without an
 * eigenvalue below -1e-4 (decided by a Cholesky factorisation of the matrix shifted by 1e-4, not by a spectrum).
 *  is_psd [B] int32 (device) */
ilqg_status ilqg_check_sufficient_nash_batch(const ilqg_problem* p, int32_t batch, const void* xs, const void* us,
                                             int32_t* is_psd, void* stream);

/* Diagnostics: out = X^T Y + C for 16x16 column-major device matrices, computed through the
 * MFMA accumulator-layout path the LQ sweep is built on (pins the gfx950 register layouts). */
ilqg_status ilqg_selftest_mfma(int32_t dtype, const void* X, const void* Y, const void* C, void* out, void* stream);

/* Diagnostics: a streaming 16-byte-per-lane copy of `bytes` (a multiple of 16; both buffers 16-byte aligned, device
 * memory) on `stream` — the copy kernel SURVEY.md 8(d) asks the roofline's measured-bandwidth denominator to come from
 * (bench.py times it with HIP events: 2 x bytes per launch / time). */
ilqg_status ilqg_copy_bandwidth(void* dst, const void* src, size_t bytes, void* stream);

/* Last HIP / validation error text of the calling thread. */
const char* ilqg_last_error(void);

/* Scratch of the stand-alone stage entry points that take no workspace argument (ilqg_lq_feedback_batch /
 * ilqg_lq_openloop_batch when delta_x or costates are asked for, ilqg_total_costs_batch, ilqg_check_*_nash_batch):
 * by default the library keeps one grow-only device allocation per calling thread for them.  A caller that owns all
 * device memory hands a buffer of its own here (per calling thread; NULL returns to the default): nothing is
 * allocated afterwards, and a call that needs more than `bytes` fails with ILQG_ERR_INVALID and the size it needs in
 * ilqg_last_error().  The solves (ilqg_*_solve_batch*) keep their memory in the workspace, with one exception: a solve
 * on the run-time-dimensioned kernels whose sweep runs on the padded specialised kernel (ilqg_solve_options::padded_sweep)
 * stages the padded rows of every instance in this scratch (batch x T x ~(N + 3) n'^2 elements). */
ilqg_status ilqg_set_scratch(void* device_buffer, size_t bytes);

/* Library / device introspection (used by the loader to fail loudly). */
#define ILQG_ABI_VERSION 9 /* 9: per-instance cost parameters (ilqg_instance_param, ilqg_problem_declare_instance_params,
                                 ilqg_problem_bind_instance_values, ilqg_instance_params_check); still 9:
                                 per-instance subsystem parameters (ilqg_problem_declare_instance_subsystem_params,
                                 ilqg_instance_subsystem_params_check: two new calls, the table gains columns); still 9:
                                 ilqg_solve_options::sweep_forms (was reserved2 = 0 = AUTO: no layout or behaviour change); still 9:
                                 per-instance routes (ilqg_problem_declare_instance_routes, ilqg_problem_bind_instance_routes,
                                 ilqg_instance_routes_check, and the host-only ilqg_segment_table_build: four new calls); still 9:
                                 per-instance time nominals (ilqg_problem_bind_instance_time_nominals,
                                 ilqg_instance_time_nominals_build, ilqg_problem_time_nominal_terms, and the host-only
                                 ilqg_time_nominal_table_build: four new calls); still 9:
                                 ILQG_SCHEDULE_CONSTANT_B and the host-only ilqg_sweep_b_structure_build (one new call); still 9:
                                 per-instance solver parameters (ilqg_solver_field, ilqg_problem_declare_instance_solver_params,
                                 ilqg_instance_solver_params_check: two new calls, the table gains columns); still 9:
                                 ILQG_COST_EXPRESSION (cost kind 24, ilqg_expr_op) and the host-only ilqg_expression_check
                                 (one new call, no layout change); still 9: relative inputs of the expression kinds
                                 (idx[2], idx[3]) and ILQG_CONSTRAINT_EXPRESSION (kind 25; no new call, no layout change); still 9:
                                 ILQG_DYN_EXPRESSION (subsystem kind 13), ILQG_ROLE_DYNAMICS_ROW (role 5) and
                                 ILQG_DYN_ROW_EXPRESSION (term kind 26): three enumerators, no new call, no layout change; still 9:
                                 the host-only ilqg_schedule_build (ilqg_schedule_query, ilqg_schedule_info: one new call); still 9:
                                 ILQG_EXPR_PUSH_TIME (expression opcode 18: one enumerator, no new call, no layout change);
                              8: ilqg_solve_options::padded_sweep (was reserved1) / probe_lanes (new, with reserved2: the struct grew by
                                 eight bytes), ILQG_SCHEDULE_PADDED_SWEEP;
                              7: ilqg_solve_options::deterministic (was reserved0) / static_rows, ilqg_copy_bandwidth, ilqg_problem_row_program, ilqg_row_program_build;
                              6: ilqg_problem_last_schedule;
                              5: ilqg_solve_options::iterate_log / max_runtime, run-time-dimensioned kernels behind every entry
                              point (any n <= 32, N <= 8, m_i), the affine constraints (ilqg_problem_desc::dense_params);
                              4: ilqg_cost_term::idx_extra / value2, cost kinds 12-21, dynamics kinds 10-12;
                              3: ilqg_solve_options / ilqg_solve_batch_ex / ilqg_solve_state_batch, ilqg_dims::sweep_formulation;
                              the workspace holds every device buffer a solve uses */
int32_t ilqg_abi_version(void);
ilqg_status ilqg_device_info(char* name_out, int32_t name_len, int32_t* num_cus);

#ifdef __cplusplus
}
#endif
#endif /* ILQG_H_ */

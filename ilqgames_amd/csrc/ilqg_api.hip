// ilqg_api.hip — the main unit of libilqg_hip.so (gfx950 only): the state the units share, the table of instantiated
// shapes, the run-time-dimensioned solve and the C ABI.  The per-shape unit is ilqg_dims.hip; DESIGN.md 3.18 has the layout.
// Entry points and the reference methods they replace: include/ilqg.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ilqg_costates.hpp"
#include "ilqg_decide_schedule.hpp"  // decide_schedule's definition
#include "ilqg_instances.hpp"        // per-instance declarations and bindings on the problem object
#include "ilqg_kernels.hpp"
#include "ilqg_launch.hpp"
#include "ilqg_nash.hpp"
#include "ilqg_problem_build.hpp"  // the problem object's host tables and its upload
#include "ilqg_receding.hpp"
#include "ilqg_round_loop.hpp"  // run_rounds' definition
#include "ilqg_shapes.hpp"
#include "ilqg_shared.hpp"

using namespace ilqg;

// ---- the state the units share (ilqg_shared.hpp), defined here ----
namespace ilqg_shared __attribute__((visibility("hidden"))) {

thread_local std::string g_err;
#if ILQG_DIAGNOSTIC_BUILD
long long* g_prof = nullptr;
#endif

ilqg_status fail(ilqg_status s, const std::string& msg) {
  g_err = msg;
  return s;
}

ScratchState& scratch_state() {
  static thread_local ScratchState st;
  return st;
}

ilqg_status Scratch::reserve(size_t need) {
  ScratchState& st = scratch_state();
  if (need <= st.bytes) return ILQG_OK;
  if (st.caller_owned)
    return fail(ILQG_ERR_INVALID, "the scratch buffer given to ilqg_set_scratch is too small: this call needs " +
                                      std::to_string(need) + " bytes");
  if (st.ptr) (void)hipFree(st.ptr);
  st.ptr = nullptr;
  st.bytes = 0;
  HIP_TRY(hipMalloc(&st.ptr, need));
  st.bytes = need;
  return ILQG_OK;
}

void raise_lds_limit(const void* kern, size_t lds) {
  if (lds <= 48 * 1024) return;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
}

ilqg_status check_device() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(ILQG_ERR_NO_DEVICE, "no HIP device visible: libilqg_hip.so has no CPU fallback");
  return ILQG_OK;
}

template ilqg_status run_rounds<float>(ilqg_problem*, SolveArgs<float>&, const SolveTail<float>&, const RoundPlan<float>&,
                                       const ilqg_solve_options&, hipStream_t);
template ilqg_status run_rounds<double>(ilqg_problem*, SolveArgs<double>&, const SolveTail<double>&, const RoundPlan<double>&,
                                        const ilqg_solve_options&, hipStream_t);

}  // namespace ilqg_shared

// The list's one expansion besides the table: without these declarations the table's addresses would instantiate every
// shape's launchers, and the kernels behind them, in this unit as well.
#define X(NX_, NP_, MU_)                                   \
  extern template struct DimsLaunch<float, NX_, NP_, MU_>; \
  extern template struct DimsLaunch<double, NX_, NP_, MU_>;
ILQG_FOR_DIMS(X)
#undef X

namespace {

// The measured-bandwidth denominator of bench.py's roofline ("measure achievable BW on the box with a copy
// kernel"): every workgroup copies one contiguous 16 KB piece, four 16-byte loads per lane in flight before the first
// store.  scripts/ubench/copy_bw.hip compares shapes on the box: this one 5.65-5.98 TB/s, a grid-stride loop over the
// same pieces 4.3-5.6, hipMemcpyDtoD 5.5.
typedef float copy_v4f __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) copy_bandwidth_kernel(copy_v4f* __restrict__ dst, const copy_v4f* __restrict__ src, size_t n16) {
  const size_t b0 = size_t(blockIdx.x) * 1024, b1 = b0 + 1024 < n16 ? b0 + 1024 : n16;
  const size_t i = b0 + threadIdx.x;
  if (b1 - b0 == 1024) {
    const copy_v4f a = src[i], b = src[i + 256], c = src[i + 512], e = src[i + 768];
    dst[i] = a;
    dst[i + 256] = b;
    dst[i + 512] = c;
    dst[i + 768] = e;
  } else {
    for (size_t k = i; k < b1; k += 256) dst[k] = src[k];
  }
}

// Index of a precision in a ShapeEntry's pairs
inline int dtype_index(int32_t dtype) { return dtype == ILQG_F32 ? 0 : 1; }

struct ShapeEntry {
  int nx, np, mu;
  // DimsLaunch<float, nx, np, mu>'s member at [0], DimsLaunch<double, nx, np, mu>'s at [1]
  decltype(&DimsLaunch<float, 0, 0, 0>::lq) lq[2];
  decltype(&DimsLaunch<float, 0, 0, 0>::lq_openloop) lq_openloop[2];
  decltype(&DimsLaunch<float, 0, 0, 0>::solve) solve[2];
  decltype(&DimsLaunch<float, 0, 0, 0>::rows) rows[2];
  PaddedSweep lq_padded[2];
  decltype(&DimsLaunch<float, 0, 0, 0>::lq_padded_batch) lq_padded_batch[2];
  ShapeTraits traits[2];  // what decide_schedule reads of the shape (needs no kernel: ilqg_schedule_build)
};
template <int NX, int NP, int MU>
constexpr ShapeEntry shape_entry() {
  using F = DimsLaunch<float, NX, NP, MU>;
  using D = DimsLaunch<double, NX, NP, MU>;
  return {NX, NP, MU, {F::lq, D::lq}, {F::lq_openloop, D::lq_openloop}, {F::solve, D::solve}, {F::rows, D::rows},
          {F::lq_padded, D::lq_padded}, {F::lq_padded_batch, D::lq_padded_batch},
          {shape_traits<float, NX, NP, MU>(), shape_traits<double, NX, NP, MU>()}};
}
#define X(NX_, NP_, MU_) shape_entry<NX_, NP_, MU_>(),
const ShapeEntry kShapes[] = {ILQG_FOR_DIMS(X)};
#undef X

const ShapeEntry* find_shape(int n, int N, int mu) {
  for (const ShapeEntry& e : kShapes)
    if (e.nx == n && e.np == N && e.mu == mu) return &e;
  return nullptr;
}

}  // namespace

// `d`: the problem as the kernels get it, p->dev or a variant of it
static ilqg_status launch_linquad(const ilqg_problem* p, const DevProblem& d, int32_t batch, const void* xs, const void* us,
                                  const void* lambdas, const void* mu, const int32_t* t_extreme, void* A, void* Bm,
                                  void* Q, void* l, void* R, void* r, void* merit_part, void* cost_part,
                                  const int32_t* active, void* stream) {
  const void* const ptrs[14] = {xs, us, lambdas, mu, t_extreme, A, Bm, Q, l, R, r, merit_part, cost_part, active};
  if (p->generic)  // the row stage with run-time dimensions (rows_chunk<T, 0, 0, 0>)
    return p->desc.dtype == ILQG_F32 ? DimsLaunch<float, 0, 0, 0>::rows(d, batch, ptrs, p->has_expression, (hipStream_t)stream)
                                     : DimsLaunch<double, 0, 0, 0>::rows(d, batch, ptrs, p->has_expression, (hipStream_t)stream);
  if (const ShapeEntry* e = find_shape(d.n, d.N, p->mu_uniform))
    return e->rows[dtype_index(p->desc.dtype)](d, batch, ptrs, p->has_expression, (hipStream_t)stream);
  return fail(ILQG_ERR_UNSUPPORTED, "no device kernel instantiated for this problem's dimensions");
}

// The smallest instantiated shape a game embeds in (same player count, at least its states and its widest control), for
// the padded sweeps (padded_lq_kernel / padded_lq_batch_kernel); nullptr: none.
static const ShapeEntry* pick_padded_shape(int n, int N, const int32_t* udim) {
  int mumax = 0;
  for (int i = 0; i < N; i++) mumax = udim[i] > mumax ? udim[i] : mumax;
  const ShapeEntry* best = nullptr;
  for (const ShapeEntry& e : kShapes)
    if (e.np == N && e.nx >= n && e.mu >= mumax && (!best || e.nx < best->nx || (e.nx == best->nx && e.mu < best->mu)))
      best = &e;
  return best;
}

// The game's control blocks at mu x mu each (the padded shape's PairTable)
static bool padded_pairs(const PairTable& pt, int N, int mu, PairTable* ptp, std::string* err) {
  std::vector<ilqg_pair> pairs(pt.npairs);
  std::vector<int> udim_p(kMaxPlayers, mu);
  for (int q = 0; q < pt.npairs; q++) pairs[q] = {pt.pi[q], pt.pj[q]};
  if (!build_pairs(pairs.data(), pt.npairs, udim_p.data(), N, ptp, err)) return false;
  for (int q = 0; q < pt.npairs; q++) ptp->from_cost[q] = pt.from_cost[q];
  return true;
}

// Threads of a workgroup of the run-time-dimensioned sweeps (ilqg_lq_generic.hpp: every phase strides its entries over
// the workgroup and ends with a barrier; lq_generic_kernel's launch bound).
static constexpr int kGenSweepThreads = 256;

// The whole solve on the run-time-dimensioned kernels: the split trial pass (integrate / rows / decide, ilqg_solve.hpp)
// over the whole batch in a round without back-tracking instances, the host counting rounds; the sweeps of
// ilqg_lq_generic.hpp on dense rows.  Instances whose step is rejected are listed and their next step sizes probed side
// by side (round 5: the speculative line search of DimsLaunch::solve, bit-identical with probe = OFF).  No fused trial
// kernel, no compact rows: the path of every shape without a specialised instantiation.
template <typename T>
static ilqg_status generic_solve(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P, void* alpha,
                                 void* total_costs, int32_t* iters, int32_t* status, int32_t* converged, void* workspace,
                                 const ilqg_solve_options& opt, hipStream_t stream) {
  const DevProblem& d = p->dev;
  SolveTail<T> tail;
  SolveArgs<T> sa = solve_args_of<T>(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, opt, &tail);
  const bool open_loop = p->desc.params.open_loop != 0;
  p->last_schedule = generic_schedule_word(open_loop, false);
  sa.rows_cw = rows_chunk_width(d.n, d.m, d.rp_pslots, d.rp_lslots, sizeof(T), size_t(48) * 1024);
  const size_t lds_roll = trial_phase_lds_bytes<T>(d, TRIAL_ROLL, sa.rows_cw);
  const size_t lds_rows = rows_maps_bytes(d) + trial_rows_elems(d, sa.rows_cw) * sizeof(T);
  const size_t lds_lq = ((open_loop ? gen_openloop_lds_elems(d.n, d.N, d.m) : gen_feedback_lds_elems(d.n, d.N, d.m)) + 4) * sizeof(T);
  if (lds_lq > kLdsPerCu || lds_rows > kLdsPerCu)
    return fail(ILQG_ERR_UNSUPPORTED, "the game does not fit a CU's LDS");
  // Back-tracking instances are listed and their next step sizes probed side by side, as in the specialised solve
  // (DimsLaunch::solve): without it a single failing line search of 100 steps costs the whole batch 100 serial passes
  // (round 5: mixed_dubins_car_scene, B = 1024: 76 passes per iteration, 42 k it/s).  One rollout per wavefront and
  // candidate: the probing rollout has a single form, so "fat" is the same kernel.
  RoundPlan<T> plan;
  const bool xdyn = p->has_expression_dynamics;  // (kExprDynProg: kernels of their own, ilqg_solve.hpp)
  const int prog_kind = xdyn ? PROG_EXPR_DYN : p->has_expression ? PROG_EXPR : PROG_PLAIN;
  plan.roll = {xdyn ? ilq_roll_kernel<T, 0, 0, 0, true> : ilq_roll_kernel<T, 0, 0, 0>, 64, lds_roll};
  plan.rows = {rows_kernel_of<T, 0, 0, 0>(prog_kind, 0, false), 64, lds_rows};
  plan.decide = {ilq_decide_kernel<T, 0, 0, 0>, 64, trial_phase_lds_bytes<T>(d, TRIAL_DECIDE, sa.rows_cw)};
  plan.proll = plan.proll_fat = {xdyn ? ilq_probe_roll_kernel<T, 0, 0, 0, false, false, true> : ilq_probe_roll_kernel<T, 0, 0, 0>, 64, lds_roll};
  plan.prows = {probe_rows_kernel_of<T, 0, 0, 0>(prog_kind, 0, false), 64, rows_maps_bytes(d) + probe_rows_elems(d, 0, sa.rows_cw) * sizeof(T)};
  plan.sweep = {gen_lq_kernel<T>, kGenSweepThreads, lds_lq};
  plan.exit = {ilq_exit_kernel<T, 0, 0, 0>, 64, quad_tables_bytes(d, sizeof(T)) + 64 * sizeof(T)};
  plan.exit_fill_first = true;
  SolveSchedule& sc = plan.s;  // the fixed schedule of this path
  sc.read_restarts = sa.al_mode != 0;
  sc.cap = sa.al_mode ? (long long)(sa.prm.max_solver_iters + 1) * (sa.prm.unconstrained_solver_max_iters + 2)
                      : (long long)(opt.fixed_iters > 0 ? opt.fixed_iters : sa.prm.max_solver_iters) + 2;
  sc.cap = (sc.cap + 2) * ((long long)sa.prm.max_backtracking_steps + 3);
  sc.row_chunks = (d.T + sa.rows_cw - 1) / sa.rows_cw;
  sc.split = sc.counted = sc.lists = 1;
  sc.probe = !opt.forced_steps && sa.prm.linesearch && opt.probe != ILQG_CHOICE_OFF;
  sc.timed = opt.max_runtime > 0.0;
  sc.lane_width = 1;
  sc.num_cus = 256;
  sc.probe_max = kProbeCandidates;
  sc.probe_budget = kProbeRoundBudget;
  // The sweep on a specialised kernel: the smallest instantiated shape the game embeds in (padded_lq_kernel).  AUTO: for
  // problems that have no instantiation of their own (ilqg_problem::generic); a problem sent here by
  // ilqg_solve_options::generic_kernels keeps the run-time-dimensioned sweeps unless padded_sweep = ON.
  PairTable ptp;
  if (opt.padded_sweep == ILQG_CHOICE_ON || (opt.padded_sweep == ILQG_CHOICE_AUTO && p->generic)) {
    const ShapeEntry* const shape = pick_padded_shape(d.n, d.N, d.udim);
    if (!shape && opt.padded_sweep == ILQG_CHOICE_ON)
      return fail(ILQG_ERR_UNSUPPORTED, "padded_sweep = ON: no instantiated shape holds this game (same player count, at "
                                        "least its states and its widest control)");
    if (shape) {
      plan.padded = shape->lq_padded[dtype_index(p->desc.dtype)];
      std::string err;
      if (!padded_pairs(d.pairs, d.N, shape->mu, &ptp, &err)) return fail(ILQG_ERR_INVALID, err);
      size_t elems = 0;
      ilqg_status s = plan.padded(d, &sa, ptp, nullptr, &elems, open_loop, stream);
      if (s != ILQG_OK) return s;
      s = Scratch().reserve(size_t(batch) * elems * sizeof(T));
      if (s != ILQG_OK) return s;
      plan.pad_pairs = &ptp;
      plan.pad = ilqg_shared::scratch_state().ptr;
      p->last_schedule = generic_schedule_word(open_loop, true);
    }
  }
  return run_rounds(p, sa, tail, plan, opt, stream);
}

// ilqg_lq_feedback_batch / ilqg_lq_openloop_batch of a shape without an instantiation on the padded sweep of `shape`
static ilqg_status launch_lq_padded(const ilqg_dims* d, const PairTable& pt, const ShapeEntry& shape, bool open_loop,
                                    const void* A, const void* Bm, const void* Q, const void* l, const void* R,
                                    const void* r, const void* x0, void* P, void* alpha, void* dx, hipStream_t stream) {
  PairTable ptp;
  std::string err;
  if (!padded_pairs(pt, d->num_players, shape.mu, &ptp, &err)) return fail(ILQG_ERR_INVALID, err);
  return shape.lq_padded_batch[dtype_index(d->dtype)](d, pt, ptp, open_loop, A, Bm, Q, l, R, r, x0, P, alpha, dx, stream);
}

// ilqg_lq_feedback_batch / ilqg_lq_openloop_batch for a shape without a specialised instantiation (or when the caller
// asks for these kernels: ilqg_dims::sweep_formulation = ILQG_SWEEP_GENERIC).
template <typename T>
static ilqg_status launch_lq_generic(const ilqg_dims* d, const PairTable& pt, bool open_loop, const void* A, const void* Bm,
                                     const void* Q, const void* l, const void* R, const void* r, const void* x0, void* P,
                                     void* alpha, void* dx, void* costates, hipStream_t stream) {
  const GenDims gd = gen_dims_of(d->n, d->num_players, d->udim, d->T);
  if (gd.m > ILQG_MAX_UDIM_TOTAL) return fail(ILQG_ERR_UNSUPPORTED, "more than ILQG_MAX_UDIM_TOTAL controls in total");
  const size_t lds = (open_loop ? gen_openloop_lds_elems(gd.n, gd.N, gd.m) : gen_feedback_lds_elems(gd.n, gd.N, gd.m)) * sizeof(T);
  if (lds > kLdsPerCu) return fail(ILQG_ERR_UNSUPPORTED, "the game's value functions do not fit a CU's LDS");
  LQBatchArgs<T> g(d, A, Bm, Q, l, R, r, x0, P, alpha, dx);
  const int row = open_loop ? gen_ol_row_elems(gd.n, gd.m, gd.N, costates != nullptr) : 0;
  if (open_loop) {
    const ilqg_status s = Scratch().reserve(size_t(d->batch) * d->T * size_t(row) * sizeof(T));
    if (s != ILQG_OK) return s;
    g.scratch = (T*)ilqg_shared::scratch_state().ptr;
    g.costates = (T*)costates;
    g.adaptive = 0;
  }
  auto kern = lq_generic_kernel<T>;
  raise_lds_limit((const void*)kern, lds);
  return launch(kern, dim3(d->batch), dim3(kGenSweepThreads), lds, stream, g, gd, pt, open_loop ? 1 : 0, row);
}

// The sweep of ilqg_lq_feedback_batch / ilqg_lq_openloop_batch on the first route that takes the game: its shape's own
// instantiation (`uniform`: one m_i, `mu`, for all players), the smallest instantiated shape that holds it, the
// run-time-dimensioned sweep (also when the caller asks for it: ilqg_dims::sweep_formulation = ILQG_SWEEP_GENERIC).
// `costates`: the open-loop sweeps carry them out themselves, the padded one excepted: with them it is passed over.
// (The feedback sweeps carry none: ilqg_lq_feedback_batch runs a kernel of its own behind whichever ran.)
static ilqg_status launch_lq_route(const ilqg_dims* d, const PairTable& pt, bool uniform, int mu, bool open_loop,
                                   const void* A, const void* Bm, const void* Q, const void* l, const void* R,
                                   const void* r, const void* x0, void* P, void* alpha, void* dx, void* costates,
                                   hipStream_t st) {
  const int ty = dtype_index(d->dtype);
  const bool specialised = d->sweep_formulation != ILQG_SWEEP_GENERIC;
  if (!open_loop) costates = nullptr;
  if (const ShapeEntry* own = uniform && specialised ? find_shape(d->n, d->num_players, mu) : nullptr)
    return open_loop ? own->lq_openloop[ty](d, pt, A, Bm, Q, l, R, r, x0, P, alpha, dx, costates, st)
                     : own->lq[ty](d, pt, A, Bm, Q, l, R, r, x0, P, alpha, dx, st);
  if (const ShapeEntry* holds = specialised && !costates ? pick_padded_shape(d->n, d->num_players, d->udim) : nullptr)
    return launch_lq_padded(d, pt, *holds, open_loop, A, Bm, Q, l, R, r, x0, P, alpha, dx, st);
  return ty ? launch_lq_generic<double>(d, pt, open_loop, A, Bm, Q, l, R, r, x0, P, alpha, dx, costates, st)
            : launch_lq_generic<float>(d, pt, open_loop, A, Bm, Q, l, R, r, x0, P, alpha, dx, costates, st);
}

// The costates of a feedback sweep's results, behind it on the stream; `zs`: costates_scratch_elems per instance
template <typename T>
static ilqg_status launch_feedback_costates(const ilqg_dims* d, const PairTable& pt, const void* A, const void* Bm,
                                            const void* Q, const void* l, const void* R, const void* r, const void* P,
                                            const void* alpha, const void* dx, void* zs, void* costates, hipStream_t st) {
  CostateDims cd;
  cd.n = d->n; cd.N = d->num_players; cd.T = d->T;
  cd.uoff[0] = 0;
  for (int i = 0; i < cd.N; i++) cd.uoff[i + 1] = cd.uoff[i] + d->udim[i];
  cd.m = cd.uoff[cd.N];
  const size_t lds = costates_lds_elems(cd.n, cd.N) * sizeof(T);
  auto kern = lq_feedback_costates_kernel<T>;
  raise_lds_limit((const void*)kern, lds);
  return launch(kern, dim3(d->batch), dim3(256), lds, st, cd, pt, (const T*)A, (const T*)Bm, (const T*)Q, (const T*)l,
                (const T*)R, (const T*)r, (const T*)P, (const T*)alpha, (const T*)dx, (T*)zs, (T*)costates);
}

// The argument checks of ilqg_lq_feedback_batch / ilqg_lq_openloop_batch and their control blocks; `uniform`: one m_i
// (`mu`) for all players, what the specialised sweeps take.  They differ in the shortest horizon and in the reference
// line that ties costates to delta_xs.
static ilqg_status lq_batch_setup(const ilqg_dims* d, const void* A, const void* Bm, const void* Q, const void* l,
                                  const void* R, const void* r, const ilqg_pair* pairs_host, int32_t npairs,
                                  const void* P, const void* alpha, const void* dx, const void* costates, int min_T,
                                  const char* costates_ref, PairTable* pt, bool* uniform, int* mu) {
  if (!d || !A || !Bm || !Q || !l || !R || !r || !pairs_host || !P || !alpha)
    return fail(ILQG_ERR_INVALID, "null argument");
  if (d->num_players < 1 || d->n < 1 || d->T < min_T || d->T > kMaxT || d->batch < 0)
    return fail(ILQG_ERR_INVALID, "bad dimensions");
  if (d->num_players > ILQG_MAX_PLAYERS || d->n > ILQG_MAX_XDIM)
    return fail(ILQG_ERR_UNSUPPORTED, "more than ILQG_MAX_XDIM states or ILQG_MAX_PLAYERS players");
  if (costates && !dx) return fail(ILQG_ERR_INVALID, std::string("costates come with delta_xs (") + costates_ref + ")");
  for (const void* ptr : {A, Bm, Q, l, R, r})
    if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return fail(ILQG_ERR_INVALID, "array bases must be 16-byte aligned");
  std::string err;
  if (!build_pairs(pairs_host, npairs, d->udim, d->num_players, pt, &err)) return fail(ILQG_ERR_INVALID, err);
  *uniform = uniform_udim(d->udim, d->num_players, mu);
  return check_device();
}

// RouteProgressCost subtracts RelativeTimeTracker::initial_time_ from the time it is handed (src/route_progress_cost.cpp:
// 58), which Problem::SetUpNextRecedingHorizon resets to the window's start (src/problem.cpp:120); the device tables
// are tabulated once with initial time 0 (ilqg_problem_create).  Re-anchoring such a problem would silently diverge
// from the reference after the first re-plan, so the receding-horizon entry points refuse it.
static const char* const kRouteProgressReceding =
    "receding horizon: the problem holds a RouteProgressCost, whose per-step nominals are tabulated for a first solve "
    "(initial time 0) only";

// An expression subsystem whose rows push the time (ILQG_EXPR_PUSH_TIME): the plan kernels integrate partial steps at
// absolute plan times (IntegrateToNextTimeStep, IntegrateFromPriorTimeStep), where the reference hands a model no
// consistent time.  The entry points that run them refuse such a problem; time-reading costs and constraints pass.
static ilqg_status refuse_time_reading_dynamics(const ilqg_problem* p, const char* entry) {
  if (p->time_reading_subsystem < 0) return ILQG_OK;
  return fail(ILQG_ERR_UNSUPPORTED, std::string(entry) + ": subsystem " + std::to_string(p->time_reading_subsystem) +
                                        " is an expression subsystem whose rows read the time (ILQG_EXPR_PUSH_TIME); the plan "
                                        "kernels integrate partial steps at absolute plan times and give a model no time");
}

extern "C" {

const char* ilqg_last_error(void) { return g_err.c_str(); }

ilqg_status ilqg_set_scratch(void* device_buffer, size_t bytes) {
  ilqg_shared::ScratchState& st = ilqg_shared::scratch_state();
  if (st.ptr && !st.caller_owned) (void)hipFree(st.ptr);
  st.ptr = device_buffer;
  st.bytes = device_buffer ? bytes : 0;
  st.caller_owned = device_buffer != nullptr;
  return ILQG_OK;
}

// Diagnostics: device buffer [B][8] of int64 receiving per-stage shader-clock cycles of the next solves.
#if ILQG_DIAGNOSTIC_BUILD
void ilqg_debug_set_profile_buffer(void* buf) { g_prof = (long long*)buf; }
#endif

// out = X^T Y + C for 16x16 column-major device matrices, through the MFMA accumulator-layout
// path the LQ sweep uses (tests pin the register layouts with asymmetric inputs).
ilqg_status ilqg_selftest_mfma(int32_t dtype, const void* X, const void* Y, const void* C, void* out, void* stream) {
  ilqg_status s = check_device();
  if (s != ILQG_OK) return s;
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch(mfma_selftest_kernel<T>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const T*)X, (const T*)Y, (const T*)C, (T*)out);
  });
}
int32_t ilqg_abi_version(void) { return ILQG_ABI_VERSION; }

ilqg_status ilqg_copy_bandwidth(void* dst, const void* src, size_t bytes, void* stream) {
  ilqg_status s = check_device();
  if (s != ILQG_OK) return s;
  if (!dst || !src || bytes < 16 || (bytes & 15) || (reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 15))
    return fail(ILQG_ERR_INVALID, "ilqg_copy_bandwidth: 16-byte aligned buffers and a multiple of 16 bytes");
  const size_t n16 = bytes / 16;
  const size_t blocks = (n16 + 1023) / 1024;  // 16 KB per workgroup
  return launch(copy_bandwidth_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<copy_v4f*>(dst), reinterpret_cast<const copy_v4f*>(src), n16);
}

ilqg_status ilqg_problem_row_program(const ilqg_problem* p, int32_t* words_out, int32_t capacity, int32_t* num_words,
                                     int32_t* static_id) {
  if (!p || !num_words) return fail(ILQG_ERR_INVALID, "null argument");
  return copy_row_program(p->row_prog, p->static_prog, words_out, capacity, num_words, static_id);
}

ilqg_status ilqg_problem_last_schedule(const ilqg_problem* p, int32_t* schedule_out) {
  if (!p || !schedule_out) return fail(ILQG_ERR_INVALID, "null argument");
  *schedule_out = p->last_schedule;
  return ILQG_OK;
}

ilqg_status ilqg_device_info(char* name_out, int32_t name_len, int32_t* num_cus) {
  ilqg_status s = check_device();
  if (s != ILQG_OK) return s;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (name_out && name_len > 0) {
    std::snprintf(name_out, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (num_cus) *num_cus = prop.multiProcessorCount;
  return ILQG_OK;
}

void ilqg_default_solver_params(ilqg_solver_params* p) {  // solver_params.h:50-84
  p->convergence_tolerance = 1e-1f;
  p->max_solver_iters = 1000;
  p->linesearch = 1;
  p->initial_alpha_scaling = 0.5f;
  p->geometric_alpha_scaling = 0.5f;
  p->max_backtracking_steps = 10;
  p->expected_decrease_fraction = 0.1f;
  p->open_loop = 0;
  p->unconstrained_solver_max_iters = 10;
  p->geometric_mu_scaling = 1.1f;
  p->geometric_mu_downscaling = 0.5f;
  p->geometric_lambda_downscaling = 0.5f;
  p->constraint_error_tolerance = 1e-1f;
}

ilqg_status ilqg_lq_feedback_batch(const ilqg_dims* d, const void* A, const void* Bm, const void* Q, const void* l,
                                   const void* R, const void* r, const ilqg_pair* pairs_host, int32_t npairs,
                                   const void* x0, void* P, void* alpha, void* dx, void* costates, void* stream) {
  PairTable pt;
  bool uniform = false;
  int mu = 0;
  ilqg_status s = lq_batch_setup(d, A, Bm, Q, l, R, r, pairs_host, npairs, P, alpha, dx, costates, 1,
                                 "lq_feedback_solver.cpp:77-78", &pt, &uniform, &mu);
  if (s != ILQG_OK) return s;
  if (d->batch == 0) return ILQG_OK;
  hipStream_t st = (hipStream_t)stream;
  // costates: Z_i, zeta_i of every step (this translation unit's scratch; the sweep's launcher has its own)
  if (costates) {
    const size_t elem = d->dtype == ILQG_F32 ? 4 : 8;
    s = Scratch().reserve(size_t(d->batch) * costates_scratch_elems(d->n, d->num_players, d->T) * elem);
    if (s != ILQG_OK) return s;
  }
  s = launch_lq_route(d, pt, uniform, mu, false, A, Bm, Q, l, R, r, x0, P, alpha, dx, costates, st);
  if (s != ILQG_OK || !costates) return s;
  void* zs = ilqg_shared::scratch_state().ptr;
  return dtype_index(d->dtype) ? launch_feedback_costates<double>(d, pt, A, Bm, Q, l, R, r, P, alpha, dx, zs, costates, st)
                               : launch_feedback_costates<float>(d, pt, A, Bm, Q, l, R, r, P, alpha, dx, zs, costates, st);
}

ilqg_status ilqg_lq_openloop_batch(const ilqg_dims* d, const void* A, const void* Bm, const void* Q, const void* l,
                                   const void* R, const void* r, const ilqg_pair* pairs_host, int32_t npairs,
                                   const void* x0, void* P, void* alpha, void* dx, void* costates, void* stream) {
  PairTable pt;
  bool uniform = false;
  int mu = 0;
  const ilqg_status s = lq_batch_setup(d, A, Bm, Q, l, R, r, pairs_host, npairs, P, alpha, dx, costates, 2,
                                       "lq_open_loop_solver.cpp:83-84", &pt, &uniform, &mu);
  if (s != ILQG_OK) return s;
  if (d->batch == 0) return ILQG_OK;
  return launch_lq_route(d, pt, uniform, mu, true, A, Bm, Q, l, R, r, x0, P, alpha, dx, costates, (hipStream_t)stream);
}

// ---- the problem object (ilqg_problem.hpp) ----
ilqg_status ilqg_problem_create(const ilqg_problem_desc* desc, ilqg_problem** out) {
  if (!desc || !out) return fail(ILQG_ERR_INVALID, "null argument");
  ProblemTables tables;
  std::unique_ptr<ilqg_problem> p;
  // (the sizes in front of the device: a bad player count or horizon is reported on a machine without one too)
  ilqg_status s = check_problem_sizes(*desc, &tables);
  if (s == ILQG_OK) s = check_device();
  if (s == ILQG_OK) s = build_problem_tables(*desc, &tables);
  if (s == ILQG_OK) s = upload_problem(*desc, tables, &p);
  if (s == ILQG_OK) *out = p.release();
  return s;
}

// The host half of creation alone (validation, flattening, the row program and its match against the registered
// structures): no device is touched and no handle made.
ilqg_status ilqg_row_program_build(const ilqg_problem_desc* desc, int32_t* words_out, int32_t capacity, int32_t* num_words,
                                   int32_t* static_id) {
  if (!num_words || !desc) return fail(ILQG_ERR_INVALID, "null argument");
  ProblemTables tables;
  const ilqg_status s = build_problem_tables(*desc, &tables);
  return s != ILQG_OK ? s : copy_row_program(tables.row_prog, tables.static_prog, words_out, capacity, num_words, static_id);
}

// The host half of creation up to the term table, then the checks of one expression cost or constraint
// (check_expression_term)
ilqg_status ilqg_expression_check(const ilqg_problem_desc* desc, int32_t term) {
  if (!desc) return fail(ILQG_ERR_INVALID, "null argument");
  if (term < 0 || term >= desc->num_terms || !desc->terms)
    return fail(ILQG_ERR_INVALID, "ilqg_expression_check: term index out of range (the problem has " + std::to_string(desc->num_terms) + " terms)");
  if (desc->terms[term].kind == ILQG_DYN_ROW_EXPRESSION) {  // a state row of an expression subsystem (check_dynamics_row_term)
    ProblemTables tables;
    using Step = ilqg_status (*)(const ilqg_problem_desc&, ProblemTables*);
    for (Step step : {check_problem_sizes, flatten_subsystems})
      if (ilqg_status s = step(*desc, &tables)) return s;
    return check_dynamics_row_term(*desc, tables.dev, term);
  }
  if (!term_is_expression(desc->terms[term].kind))  // (either kind; the message is the one the first kind came with)
    return fail(ILQG_ERR_INVALID, "ilqg_expression_check: term " + std::to_string(term) + " is not an ILQG_COST_EXPRESSION term");
  ProblemTables tables;
  using Step = ilqg_status (*)(const ilqg_problem_desc&, ProblemTables*);
  for (Step step : {check_problem_sizes, flatten_subsystems, build_term_table})
    if (ilqg_status s = step(*desc, &tables)) return s;
  return check_expression_term(*desc, term, tables.terms[term].arg_dim);
}

// The host half of creation alone, for what the feedback sweep may assume about B (ProblemTables::b_constant)
ilqg_status ilqg_sweep_b_structure_build(const ilqg_problem_desc* desc, int32_t* constant_out, int32_t* entries_out,
                                         int32_t capacity, int32_t* num_entries) {
  static_assert(ILQG_B_ENTRY_LITERAL == RC_LITERAL && ILQG_B_ENTRY_DT == RC_DT && ILQG_B_ENTRY_NEG_DT == RC_NEG_DT, "ilqg.h");
  if (!desc || !constant_out || !num_entries) return fail(ILQG_ERR_INVALID, "null argument");
  ProblemTables tables;
  const ilqg_status s = build_problem_tables(*desc, &tables);
  if (s != ILQG_OK) return s;
  const std::vector<int>& e = tables.row_prog.b_entries;
  *constant_out = tables.b_constant ? 1 : 0;
  *num_entries = int32_t(e.size() / 4);
  if (entries_out) {
    if (size_t(capacity) < e.size()) return fail(ILQG_ERR_INVALID, "ilqg_sweep_b_structure_build: buffer too small");
    std::memcpy(entries_out, e.data(), sizeof(int32_t) * e.size());
  }
  return ILQG_OK;
}

// The host half of creation alone, then the schedule a solve of it would run: decide_schedule as DimsLaunch::solve calls
// it, on what the query says the call and the device are
ilqg_status ilqg_schedule_build(const ilqg_problem_desc* desc, const ilqg_solve_options* options, const ilqg_schedule_query* query,
                                ilqg_schedule_info* out) {
  if (!desc || !options || !query || !out) return fail(ILQG_ERR_INVALID, "null argument");
  if (query->batch < 1 || query->num_cus < 1) return fail(ILQG_ERR_INVALID, "ilqg_schedule_build: batch and num_cus are positive");
  ProblemTables tables;
  const ilqg_status s = build_problem_tables(*desc, &tables);
  if (s != ILQG_OK) return s;
  const DevProblem& d = tables.dev;
  *out = ilqg_schedule_info{};
  if (tables.generic || options->generic_kernels == ILQG_CHOICE_ON) {
    const bool padded = (options->padded_sweep == ILQG_CHOICE_ON || (options->padded_sweep == ILQG_CHOICE_AUTO && tables.generic)) &&
                        pick_padded_shape(d.n, d.N, d.udim) != nullptr;
    out->word = generic_schedule_word(desc->params.open_loop != 0, padded);
    return ILQG_OK;
  }
  const ShapeEntry* e = find_shape(d.n, d.N, tables.mu_uniform);
  if (!e) return fail(ILQG_ERR_UNSUPPORTED, "no device kernel instantiated for this problem's dimensions");
  const ProblemFacts f{desc->params, tables.static_prog, tables.b_constant, tables.has_expression, tables.has_expression_dynamics,
                       query->tables_bound != 0 || query->solver_bound != 0, query->solver_bound != 0};
  const int sched_batch = (schedule_counts_mask(*options) && query->active >= 0) ? std::max(query->active, 1) : query->batch;
  *out = decide_schedule(e->traits[dtype_index(desc->dtype)], d, f, *options, query->batch, sched_batch, query->num_cus, kProfile);
  return ILQG_OK;
}

// The host half of creation alone, for the segment table (DevProblem::segs_f / segs_d: 21 scalars per segment)
ilqg_status ilqg_segment_table_build(const ilqg_problem_desc* desc, int32_t dtype, void* out, int32_t capacity,
                                     int32_t* num_elems) {
  if (!num_elems || !desc) return fail(ILQG_ERR_INVALID, "null argument");
  if (dtype != ILQG_F32 && dtype != ILQG_F64) return fail(ILQG_ERR_INVALID, "ilqg_segment_table_build: dtype");
  ProblemTables tables;
  const ilqg_status s = build_problem_tables(*desc, &tables);
  if (s != ILQG_OK) return s;
  *num_elems = int32_t(tables.segs.f.size());
  if (out) {
    if (capacity < *num_elems) return fail(ILQG_ERR_INVALID, "ilqg_segment_table_build: buffer too small");
    if (dtype == ILQG_F32) std::memcpy(out, tables.segs.f.data(), sizeof(float) * tables.segs.f.size());
    else std::memcpy(out, tables.segs.d.data(), sizeof(double) * tables.segs.d.size());
  }
  return ILQG_OK;
}

// The host half of creation alone, for the per-step nominals of the time-dependent costs (DevProblem::time_nominal_f /
// time_nominal_d: [tables][T][2] doubles in the geometry precision of `dtype`)
ilqg_status ilqg_time_nominal_table_build(const ilqg_problem_desc* desc, int32_t dtype, double* out, int32_t capacity,
                                          int32_t* num_elems) {
  if (!num_elems || !desc) return fail(ILQG_ERR_INVALID, "null argument");
  if (dtype != ILQG_F32 && dtype != ILQG_F64) return fail(ILQG_ERR_INVALID, "ilqg_time_nominal_table_build: dtype");
  ProblemTables tables;
  const ilqg_status s = build_problem_tables(*desc, &tables);
  if (s != ILQG_OK) return s;
  const std::vector<double>& table = dtype == ILQG_F32 ? tables.time_nominal.f : tables.time_nominal.d;
  *num_elems = int32_t(table.size());
  if (out) {
    if (capacity < *num_elems) return fail(ILQG_ERR_INVALID, "ilqg_time_nominal_table_build: buffer too small");
    if (!table.empty()) std::memcpy(out, table.data(), sizeof(double) * table.size());
  }
  return ILQG_OK;
}

void ilqg_problem_destroy(ilqg_problem* p) { delete p; }

// ---- per-instance cost parameters (ilqg.h) ----
ilqg_status ilqg_instance_params_check(const ilqg_problem_desc* desc, int32_t count, const ilqg_instance_param* params) {
  if (!desc) return fail(ILQG_ERR_INVALID, "null argument");
  return instance_params_check_terms(desc->num_terms, desc->terms, count, params);
}

ilqg_status ilqg_problem_declare_instance_params(ilqg_problem* p, int32_t count, const ilqg_instance_param* params) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->bindings.bound[kBindValues])
    return fail(ILQG_ERR_INVALID, "instance parameters cannot be declared while values are bound: unbind first");
  ilqg_status s = instance_params_check_terms(int(p->terms_host.size()), p->terms_host.data(), count, params);
  if (s == ILQG_OK) s = instance_total_check(size_t(count), p->inst_subs.size(), p->inst_solver.size());
  return s != ILQG_OK ? s : declare_instance_columns(p, std::vector<ilqg_instance_param>(params, params + count), p->inst_subs,
                                                     p->inst_solver);
}

// ---- per-instance subsystem parameters (ilqg.h) ----
ilqg_status ilqg_instance_subsystem_params_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* subsystems) {
  if (!desc) return fail(ILQG_ERR_INVALID, "null argument");
  if (desc->num_players < 0 || desc->num_players > kMaxPlayers)
    return fail(ILQG_ERR_INVALID, "instance subsystem parameters: num_players out of range");
  int kinds[kMaxPlayers];
  for (int i = 0; i < desc->num_players; i++) kinds[i] = desc->subsystems[i].kind;
  return instance_subsystems_check(desc->num_players, kinds, count, subsystems);
}

ilqg_status ilqg_problem_declare_instance_subsystem_params(ilqg_problem* p, int32_t count, const int32_t* subsystems) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->bindings.bound[kBindValues])
    return fail(ILQG_ERR_INVALID, "instance parameters cannot be declared while values are bound: unbind first");
  ilqg_status s = instance_subsystems_check(p->dev.N, p->dev.sub_kind, count, subsystems);
  if (s == ILQG_OK) s = instance_total_check(p->inst_params.size(), size_t(count), p->inst_solver.size());
  return s != ILQG_OK ? s : declare_instance_columns(p, p->inst_params, std::vector<int>(subsystems, subsystems + count),
                                                     p->inst_solver);
}

// ---- per-instance solver parameters (ilqg.h) ----
ilqg_status ilqg_instance_solver_params_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* fields) {
  if (!desc) return fail(ILQG_ERR_INVALID, "null argument");
  return instance_solver_check(count, fields);
}

ilqg_status ilqg_problem_declare_instance_solver_params(ilqg_problem* p, int32_t count, const int32_t* fields) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->bindings.bound[kBindValues])
    return fail(ILQG_ERR_INVALID, "instance parameters cannot be declared while values are bound: unbind first");
  ilqg_status s = instance_solver_check(count, fields);
  if (s == ILQG_OK) s = instance_total_check(p->inst_params.size(), p->inst_subs.size(), size_t(count));
  return s != ILQG_OK ? s : declare_instance_columns(p, p->inst_params, p->inst_subs, std::vector<int>(fields, fields + count));
}

ilqg_status ilqg_problem_bind_instance_values(ilqg_problem* p, int32_t batch, const float* values) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  DevProblem& d = p->dev;
  if (!values) {
    d.inst_values = nullptr;
    d.inst_terms = nullptr;
    d.inst_count = 0;
    d.inst_solver = 0;
    p->bindings.bound[kBindValues] = false;
    return ILQG_OK;
  }
  if (p->inst_params.empty() && p->inst_subs.empty() && p->inst_solver.empty())
    return fail(ILQG_ERR_INVALID, "no instance parameters are declared (ilqg_problem_declare_instance_params)");
  if (ilqg_status s = bind_batch_check(p, kBindValues, batch)) return s;
  d.inst_values = values;
  d.inst_terms = p->d_inst_terms.get();
  d.inst_count = int(p->inst_params.size() + p->inst_subs.size() + p->inst_solver.size());
  d.inst_solver = int(p->inst_solver.size());
  p->bindings.bind(kBindValues, batch);
  return ILQG_OK;
}

// ---- per-instance routes (ilqg.h) ----
ilqg_status ilqg_instance_routes_check(const ilqg_problem_desc* desc, int32_t count, const int32_t* polylines) {
  if (!desc) return fail(ILQG_ERR_INVALID, "null argument");
  return instance_routes_check_terms(desc->num_polylines, desc->num_terms, desc->terms, count, polylines);
}

ilqg_status ilqg_problem_declare_instance_routes(ilqg_problem* p, int32_t count, const int32_t* polylines) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->bindings.bound[kBindRoutes])
    return fail(ILQG_ERR_INVALID, "instance routes cannot be declared while a route table is bound: unbind first");
  ilqg_status s = instance_routes_check_terms(p->dev.num_polylines, int(p->terms_host.size()), p->terms_host.data(), count, polylines);
  if (s != ILQG_OK) return s;
  // polyline -> its first point in a row of the caller's points (declaration order), -1: not declared
  std::vector<int> cols(size_t(p->dev.num_polylines) + 1, -1), off(size_t(p->dev.num_polylines) + 1, 0);
  if (count > 0) HIP_TRY(hipMemcpy(off.data(), p->d_poly_off.get(), sizeof(int) * off.size(), hipMemcpyDeviceToHost));
  int points = 0;
  for (int c = 0; c < count; c++) {
    cols[polylines[c]] = points;
    points += off[polylines[c] + 1] - off[polylines[c]];
  }
  DeviceBuffer<int> d_cols;
  s = upload(cols, 0, "instance route tables", &d_cols);
  if (s != ILQG_OK) return s;
  p->d_route_cols = std::move(d_cols);
  p->route_polys.assign(polylines, polylines + count);
  p->route_points = points;
  return ILQG_OK;
}

ilqg_status ilqg_problem_bind_instance_routes(ilqg_problem* p, int32_t batch, const float* points, void* stream) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  DevProblem& d = p->dev;
  if (!points) {  // (hipFree waits for the kernels that may still read the table)
    d.segs_f = p->d_segs.f.get();
    d.segs_d = p->d_segs.d.get();
    d.seg_inst_stride = 0;
    p->d_route_segs.f.reset();
    p->d_route_segs.d.reset();
    p->bindings.bound[kBindRoutes] = false;
    return ILQG_OK;
  }
  if (p->route_polys.empty())
    return fail(ILQG_ERR_INVALID, "no instance routes are declared (ilqg_problem_declare_instance_routes)");
  if (ilqg_status s = bind_batch_check(p, kBindRoutes, batch)) return s;
  const size_t count = size_t(batch) * size_t(d.total_segs);
  // a new table; one of the same size is rewritten in place, in stream order
  if (!p->bindings.bound[kBindRoutes] || batch != p->bindings.batch) {
    const ilqg_status s = with_dtype(p->desc.dtype, [&](auto tag) {
      using T = decltype(tag);
      return upload(std::vector<T>(), count * kSegStride + 1, "instance route table", &segs_of<T>(p->d_route_segs));
    });
    if (s != ILQG_OK) {
      (void)ilqg_problem_bind_instance_routes(p, 0, nullptr, stream);
      return s;
    }
  }
  if (count > 0) {
    const dim3 grid((unsigned)((count + 255) / 256));
    if (ilqg_status s = with_dtype(p->desc.dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch(route_segments_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, d.poly_off, d.num_polylines,
                    p->d_route_cols.get(), points, p->route_points, segs_of<T>(p->d_segs).get(), d.total_segs, batch,
                    segs_of<T>(p->d_route_segs).get());
    })) return s;
  }
  if (p->desc.dtype == ILQG_F32) d.segs_f = p->d_route_segs.f.get(); else d.segs_d = p->d_route_segs.d.get();
  d.seg_inst_stride = d.total_segs * kSegStride;
  p->bindings.bind(kBindRoutes, batch);
  return ILQG_OK;
}

// ---- per-instance time nominals (ilqg.h) ----
ilqg_status ilqg_problem_time_nominal_terms(const ilqg_problem* p, int32_t* terms_out, int32_t capacity, int32_t* tables) {
  if (!p || !tables) return fail(ILQG_ERR_INVALID, "null argument");
  *tables = int32_t(p->tnom_tables.size() / 4);
  if (terms_out) {
    if (capacity < *tables) return fail(ILQG_ERR_INVALID, "ilqg_problem_time_nominal_terms: buffer too small");
    for (int q = 0; q < *tables; q++) terms_out[q] = p->tnom_tables[size_t(4) * q];
  }
  return ILQG_OK;
}

ilqg_status ilqg_problem_bind_instance_time_nominals(ilqg_problem* p, int32_t batch, const double* nominals) {
  if (!p) return fail(ILQG_ERR_INVALID, "null argument");
  DevProblem& d = p->dev;
  if (!nominals) {
    d.time_nominal_f = p->d_time_nominal.f.get();
    d.time_nominal_d = p->d_time_nominal.d.get();
    d.tnom_inst_stride = 0;
    p->bindings.bound[kBindNominals] = false;
    return ILQG_OK;
  }
  if (p->tnom_tables.empty())
    return fail(ILQG_ERR_INVALID, "instance time nominals: the problem has no time-dependent term (NOMINAL_PATH_LENGTH, "
                                  "ROUTE_PROGRESS)");
  if (ilqg_status s = bind_batch_check(p, kBindNominals, batch)) return s;
  // (the handle's precision: the other pointer is not read)
  if (p->desc.dtype == ILQG_F32) d.time_nominal_f = nominals; else d.time_nominal_d = nominals;
  d.tnom_inst_stride = int(p->tnom_tables.size() / 4) * d.T * 2;
  p->bindings.bind(kBindNominals, batch);
  return ILQG_OK;
}

ilqg_status ilqg_instance_time_nominals_build(const ilqg_problem* p, int32_t batch, const float* speed_pos, double* nominals,
                                              void* stream) {
  if (!p || !speed_pos || !nominals) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->tnom_tables.empty())
    return fail(ILQG_ERR_INVALID, "instance time nominals: the problem has no time-dependent term (NOMINAL_PATH_LENGTH, "
                                  "ROUTE_PROGRESS)");
  if (batch <= 0) return fail(ILQG_ERR_INVALID, "instance time nominals: batch must be positive");
  const DevProblem& d = p->dev;
  const int num_tables = int(p->tnom_tables.size() / 4);
  const size_t count = size_t(batch) * size_t(num_tables) * size_t(d.T);
  const dim3 grid((unsigned)((count + 255) / 256));
  // the BAKED segment table (a ROUTE_PROGRESS term's polyline never varies per instance), in the handle's precision
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch(time_nominals_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, p->d_tnom_tables.get(),
                  num_tables, d.T, d.dt, speed_pos, segs_of<T>(p->d_segs).get(), batch, nominals);
  });
}

ilqg_status ilqg_problem_pairs(const ilqg_problem* p, ilqg_pair* pairs_host, int32_t* npairs) {
  if (!p || !pairs_host || !npairs) return fail(ILQG_ERR_INVALID, "null argument");
  *npairs = p->dev.pairs.npairs;
  for (int q = 0; q < *npairs; q++) pairs_host[q] = {p->dev.pairs.pi[q], p->dev.pairs.pj[q]};
  return ILQG_OK;
}

ilqg_status ilqg_workspace_bytes(const ilqg_problem* p, int32_t batch, uint64_t* bytes) {
  if (!p || !bytes) return fail(ILQG_ERR_INVALID, "null argument");
  const DevProblem& d = p->dev;
  const size_t elem = p->desc.dtype == ILQG_F32 ? 4 : 8;
  *bytes = ws_tail(d, batch > 0 ? batch : 0, elem, p->desc.params.open_loop ? ol_row_elems(d.n, d.m, d.N) : 0).total;
  return ILQG_OK;
}


ilqg_status ilqg_rollout_batch(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs_ref,
                               const void* us_ref, const void* P, const void* alpha, const void* alpha_scale,
                               void* xs, void* us, const int32_t* active, void* stream) {
  if (!p || !x0 || !xs_ref || !us_ref || !P || !alpha || !xs || !us) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch, false)) return sb;
  const DevProblem& d = p->dev;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    RolloutBatchArgs<T> g{(const T*)x0, (const T*)xs_ref, (const T*)us_ref, (const T*)P, (const T*)alpha,
                          (const T*)alpha_scale, (T*)xs, (T*)us, active};
    auto kern = p->has_expression_dynamics ? rollout_kernel<T, true> : rollout_kernel<T, false>;
    return launch(kern, dim3(batch), dim3(64), rollout_lds_elems(d.n, d.m) * sizeof(T),
                  (hipStream_t)stream, d, g);
  });
}

ilqg_status ilqg_linearize_batch(const ilqg_problem* p, int32_t batch, const void* xs, const void* us, void* A,
                                 void* Bm, const int32_t* active, void* stream) {
  if (!p || !xs || !us || !A || !Bm) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch, false)) return sb;
  return launch_linquad(p, p->dev, batch, xs, us, nullptr, nullptr, nullptr, A, Bm, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, active, stream);
}

ilqg_status ilqg_quadraticize_batch(const ilqg_problem* p, int32_t batch, const void* xs, const void* us,
                                    const void* lambdas, const void* mu, const int32_t* t_extreme, void* Q, void* l,
                                    void* R, void* r, const int32_t* active, void* stream) {
  if (!p || !xs || !us || !Q || !l || !R || !r) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  return launch_linquad(p, p->dev, batch, xs, us, lambdas, mu, t_extreme, nullptr, nullptr, Q, l, R, r, nullptr, nullptr,
                        active, stream);
}

ilqg_status ilqg_total_costs_batch(const ilqg_problem* p, int32_t batch, const void* xs, const void* us, void* costs,
                                   int32_t* t_extreme, const int32_t* active, void* stream) {
  if (!p || !xs || !us || !costs) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  const DevProblem& d = p->dev;
  const size_t esz = p->desc.dtype == ILQG_F32 ? 4 : 8;
  ilqg_status s = Scratch().reserve(size_t(batch) * d.T * d.N * esz);
  if (s != ILQG_OK) return s;
  s = launch_linquad(p, p->dev, batch, xs, us, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, ilqg_shared::scratch_state().ptr, active, stream);
  if (s != ILQG_OK) return s;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch(costs_reduce_kernel<T>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d,
                  (const T*)ilqg_shared::scratch_state().ptr, (T*)costs, t_extreme, active);
  });
}

void ilqg_default_solve_options(ilqg_solve_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));  // reference semantics, every scheduling choice ILQG_CHOICE_AUTO
}

ilqg_status ilqg_solve_batch_ex(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                void* alpha, void* total_costs, int32_t* iters, int32_t* status, int32_t* converged,
                                void* workspace, const ilqg_solve_options* options, void* stream) {
  if (!p || !x0 || !xs || !us || !P || !alpha || !total_costs || !iters || !status || !converged || !workspace || !options)
    return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  const ilqg_solve_options& o = *options;
  if (o.fixed_iters < 0) return fail(ILQG_ERR_INVALID, "fixed_iters must not be negative");
  if (o.forced_steps && (o.fixed_iters <= 0 || o.augmented_lagrangian))
    return fail(ILQG_ERR_INVALID, "forced_steps needs fixed_iters > 0 and no augmented-Lagrangian loop");
  if (o.max_runtime > 0.0 && (o.fixed_iters > 0 || o.forced_steps))
    return fail(ILQG_ERR_INVALID, "max_runtime needs a free-running solve (fixed_iters = 0, no forced steps)");
  for (int32_t c : {o.single_wave_sweep, o.adjoint_expected_decrease, o.split_trial, o.handoff, o.probe, o.counted,
                    o.generic_kernels, o.padded_sweep, o.probe_lanes, o.sweep_forms})
    if (c < ILQG_CHOICE_AUTO || c > ILQG_CHOICE_ON) return fail(ILQG_ERR_INVALID, "scheduling choices are ilqg_choice values");
  if (o.probe_first < 0 || o.probe_first > 1024) return fail(ILQG_ERR_INVALID, "probe_first: 0 (the library's choice) or a count");
  const DevProblem& d = p->dev;
  hipStream_t st = (hipStream_t)stream;
  if (p->generic || o.generic_kernels == ILQG_CHOICE_ON)
    return p->desc.dtype == ILQG_F32
               ? generic_solve<float>(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, o, st)
               : generic_solve<double>(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, o, st);
  if (const ShapeEntry* e = find_shape(d.n, d.N, p->mu_uniform))
    return e->solve[dtype_index(p->desc.dtype)](p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged,
                                                workspace, o, st);
  return fail(ILQG_ERR_UNSUPPORTED, "no device kernel instantiated for this problem's dimensions");
}

ilqg_status ilqg_ilq_solve_batch(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                 void* alpha, void* total_costs, int32_t* iters, int32_t* status, int32_t* converged,
                                 void* workspace, int32_t fixed_iters, void* stream) {
  ilqg_solve_options o;
  ilqg_default_solve_options(&o);
  o.fixed_iters = fixed_iters;
  return ilqg_solve_batch_ex(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, &o, stream);
}

ilqg_status ilqg_al_solve_batch(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                void* alpha, void* total_costs, int32_t* iters, int32_t* status, int32_t* converged,
                                void* workspace, void* stream) {
  ilqg_solve_options o;
  ilqg_default_solve_options(&o);
  o.augmented_lagrangian = 1;
  return ilqg_solve_batch_ex(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, &o, stream);
}

ilqg_status ilqg_solve_again_batch(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                                   void* alpha, void* total_costs, int32_t* iters, int32_t* status,
                                   int32_t* converged, void* workspace, int32_t augmented_lagrangian,
                                   const int32_t* active, void* stream) {
  ilqg_solve_options o;
  ilqg_default_solve_options(&o);
  o.augmented_lagrangian = augmented_lagrangian ? 1 : 0;
  o.resume = 1;
  o.active = active;
  return ilqg_solve_batch_ex(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, &o, stream);
}

ilqg_status ilqg_solve_state_batch(const ilqg_problem* p, int32_t batch, const void* workspace,
                                   int32_t augmented_lagrangian, void* last_merit, void* expected_decrease,
                                   void* step, int32_t* backtracks, void* stream) {
  if (!p || !workspace) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  const DevProblem& d = p->dev;
  const int ol_row = p->desc.params.open_loop ? ol_row_elems(d.n, d.m, d.N) : 0;
  const WsLayout L = ws_layout_of(d, ol_row, augmented_lagrangian ? 1 : 0);
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch(solve_state_kernel<T>, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                  (const T*)workspace, L.total, L.state, batch, (T*)last_merit, (T*)expected_decrease,
                  (T*)step, backtracks);
  });
}

ilqg_status ilqg_receding_horizon_shift_batch(const ilqg_problem* p, int32_t batch, const void* x0, double t0,
                                              double planner_runtime, double plan_t0, void* xs, void* us, void* P,
                                              void* alpha, void* x0_next, int32_t* first_step,
                                              double* new_plan_t0_host, void* stream) {
  if (!p || !x0 || !xs || !us || !P || !alpha || !x0_next || !first_step) return fail(ILQG_ERR_INVALID, "null argument");
  if (p->has_route_progress) return fail(ILQG_ERR_UNSUPPORTED, kRouteProgressReceding);
  if (ilqg_status st = refuse_time_reading_dynamics(p, "receding horizon")) return st;
  const DevProblem& d = p->dev;
  const double dt = d.dt, horizon = dt * d.T;
  // the reference's CHECKs (src/problem.cpp:68-70)
  if (planner_runtime < 0.0 || planner_runtime + t0 > plan_t0 + horizon || t0 < plan_t0)
    return fail(ILQG_ERR_INVALID, "receding horizon: t0 / planner_runtime outside the stored plan");
  // SyncToExistingProblem's time bookkeeping (:75-102) is identical for every instance of this batch; the
  // kernel repeats it per instance, here it validates the call and reports the new plan's start time
  const float kRoundingError = 0.9f;
  const double relative_t0 = t0 - plan_t0;
  size_t current_timestep = static_cast<size_t>(relative_t0 / dt);
  double remaining = (current_timestep + 1) * dt - relative_t0;
  if (remaining < kRoundingError * dt) {
    current_timestep += 1;
    remaining = dt - remaining;
  }
  const size_t itn_step = static_cast<size_t>((relative_t0 + kSmallNumberF) / dt);  // IntegrateToNextTimeStep's own (:104-113)
  if (itn_step >= size_t(d.T)) return fail(ILQG_ERR_INVALID, "receding horizon: t0 past the last plan step");
  double new_t0 = t0 + remaining;
  int int_begin = int(current_timestep) + 1, int_end = int_begin;
  if (remaining <= planner_runtime) {
    const size_t num_steps = static_cast<size_t>(kSmallNumberF + (planner_runtime - remaining) / dt);
    int_end = int(current_timestep + num_steps);
    if (int_end < int_begin) int_end = int_begin;
    new_t0 += dt * double(num_steps);
  }
  if (int_end > d.T) return fail(ILQG_ERR_INVALID, "receding horizon: integration runs past the plan");
  if (new_plan_t0_host) *new_plan_t0_host = new_t0;
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch, false)) return sb;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    RecedingArgs<T> g{};
    g.plan = PlanBuffers<T>{(T*)xs, (T*)us, (T*)P, (T*)alpha, nullptr, nullptr, plan_t0, d.T};
    g.x = (const T*)x0; g.t = t0; g.planner_runtime = planner_runtime;
    g.xs = (T*)xs; g.us = (T*)us; g.P = (T*)P; g.alpha = (T*)alpha; g.x0_next = (T*)x0_next;
    g.first_step = first_step;
    auto kern = p->has_expression_dynamics ? receding_sync_kernel<T, true> : receding_sync_kernel<T, false>;
    return launch(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(T),
                  (hipStream_t)stream, d, g);
  });
}

static ilqg_status launch_strategy_costs(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                         const void* us, const void* P, const void* alpha, double eps, int open_loop,
                                         int euler, int moves, void* costs, void* stream) {
  const DevProblem& d = p->dev;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    StrategyCostArgs<T> g{(const T*)x0, (const T*)xs, (const T*)us, (const T*)P, (const T*)alpha,
                            (T*)costs, T(eps), open_loop, euler, batch};
    const size_t lds = quad_tables_bytes(d, sizeof(T)) + strategy_cost_lds_elems(d.n, d.m, d.num_terms) * sizeof(T);
    auto kern = p->has_expression_dynamics ? strategy_costs_kernel<T, true> : strategy_costs_kernel<T, false>;
    return launch(kern, dim3(batch, moves), dim3(64), lds, (hipStream_t)stream, d, g);
  });
}

ilqg_status ilqg_strategy_costs_batch(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                      const void* us, const void* P, const void* alpha, int32_t open_loop,
                                      int32_t euler, void* costs, void* stream) {
  if (!p || !x0 || !xs || !us || !P || !alpha || !costs) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  return launch_strategy_costs(p, batch, x0, xs, us, P, alpha, 0.0, open_loop ? 1 : 0, euler ? 1 : 0, 1, costs, stream);
}

ilqg_status ilqg_check_local_nash_batch(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                        const void* us, const void* P, const void* alpha, double max_perturbation,
                                        int32_t open_loop, int32_t* is_nash, void* margin, void* stream) {
  if (!p || !x0 || !xs || !us || !P || !alpha || !is_nash) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  const DevProblem& d = p->dev;
  const int moves = 1 + 2 * d.m * (d.T - 1);
  if (moves > 65535) return fail(ILQG_ERR_UNSUPPORTED, "too many perturbations for one launch");
  const size_t esz = p->desc.dtype == ILQG_F32 ? 4 : 8;
  ilqg_status s = Scratch().reserve(size_t(moves) * batch * d.N * esz);
  if (s != ILQG_OK) return s;
  // the reference switches the integrator to one-step Euler for this check (check_local_nash_equilibrium.cpp:75-79)
  s = launch_strategy_costs(p, batch, x0, xs, us, P, alpha, max_perturbation, open_loop ? 1 : 0, 1, moves, ilqg_shared::scratch_state().ptr,
                            stream);
  if (s != ILQG_OK) return s;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch(nash_verdict_kernel<T>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d,
                  (const T*)ilqg_shared::scratch_state().ptr, moves, batch, is_nash, (T*)margin);
  });
}

ilqg_status ilqg_check_sufficient_nash_batch(const ilqg_problem* p, int32_t batch, const void* xs, const void* us,
                                             int32_t* is_psd, void* stream) {
  if (!p || !xs || !us || !is_psd) return fail(ILQG_ERR_INVALID, "null argument");
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch)) return sb;
  // PlayerCost::Quadraticize of every player at every step (:168-172), whatever the player's time structure: the
  // quadraticisation kernel is launched on a copy of the problem whose players are all time-additive (the copy carries
  // the declared per-instance parameters and the bound tables; each chunk below starts at its own rows of them)
  const DevProblem& d = p->dev;
  const size_t esz = p->desc.dtype == ILQG_F32 ? 4 : 8;
  const size_t per_inst = size_t(d.T) * (size_t(d.N) * d.n * d.n + size_t(d.N) * d.n + d.pairs.Rsz + d.pairs.rsz) * esz;
  int chunk = int((size_t(256) << 20) / per_inst);
  if (chunk < 1) chunk = 1;
  if (chunk > batch) chunk = batch;
  ilqg_status s = Scratch().reserve(per_inst * chunk);
  if (s != ILQG_OK) return s;
  s = launch(fill_int_kernel<int>, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, is_psd, 1, batch);
  if (s != ILQG_OK) return s;
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    const int nb = (batch - b0 < chunk) ? batch - b0 : chunk;
    char* base = (char*)ilqg_shared::scratch_state().ptr;
    char* Q = base;
    char* l = Q + size_t(nb) * d.T * d.N * d.n * d.n * esz;
    char* R = l + size_t(nb) * d.T * d.N * d.n * esz;
    char* r = R + size_t(nb) * d.T * d.pairs.Rsz * esz;
    const char* xs_c = (const char*)xs + size_t(b0) * d.T * d.n * esz;
    const char* us_c = (const char*)us + size_t(b0) * d.T * d.m * esz;
    DevProblem full = dev_from_instance(p, b0);
    for (int i = 0; i < full.N; i++) full.structure[i] = ILQG_SUM;
    s = launch_linquad(p, full, nb, xs_c, us_c, nullptr, nullptr, nullptr, nullptr, nullptr, Q, l, R, r, nullptr, nullptr,
                       nullptr, stream);
    if (s != ILQG_OK) break;
    s = with_dtype(p->desc.dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch(psd_check_kernel<T>, dim3(d.T, nb), dim3(64), 0, (hipStream_t)stream, full, (T*)Q, (T*)R,
                    is_psd + b0);
    });
    if (s != ILQG_OK) break;
  }
  return s;
}

static ilqg_status check_plan(const ilqg_problem* p, int32_t plan_rows, const void* a, const void* b, const void* c,
                              const void* d, const void* e, const void* f) {
  if (!p || !a || !b || !c || !d || !e || !f) return fail(ILQG_ERR_INVALID, "null argument");
  if (plan_rows < p->dev.T) return fail(ILQG_ERR_INVALID, "plan_rows must be at least the problem's T");
  return ILQG_OK;
}

ilqg_status ilqg_plan_integrate_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows, const void* plan_xs,
                                      const void* plan_us, const void* plan_P, const void* plan_alpha,
                                      const int32_t* plan_len, const double* plan_t0, double t_from, double t_to,
                                      double must_contain, void* x, int32_t* active, void* stream) {
  ilqg_status s = check_plan(p, plan_rows, plan_xs, plan_us, plan_P, plan_alpha, plan_len, plan_t0);
  if (s != ILQG_OK) return s;
  if (!x || !active) return fail(ILQG_ERR_INVALID, "null argument");
  if (ilqg_status st = refuse_time_reading_dynamics(p, "plan integration")) return st;
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch, false)) return sb;
  const DevProblem& d = p->dev;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    PlanIntegrateArgs<T> g{};
    g.plan = PlanBuffers<T>{(T*)plan_xs, (T*)plan_us, (T*)plan_P, (T*)plan_alpha, (int*)plan_len,
                              (double*)plan_t0, 0.0, plan_rows};
    g.t_from = t_from; g.t_to = t_to; g.must_contain = must_contain; g.x = (T*)x; g.active = active;
    auto kern = p->has_expression_dynamics ? plan_integrate_kernel<T, true> : plan_integrate_kernel<T, false>;
    return launch(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(T),
                  (hipStream_t)stream, d, g);
  });
}

ilqg_status ilqg_receding_horizon_sync_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows,
                                             const void* plan_xs, const void* plan_us, const void* plan_P,
                                             const void* plan_alpha, const int32_t* plan_len, const double* plan_t0,
                                             const void* x, double t, double planner_runtime, void* xs, void* us,
                                             void* P, void* alpha, void* x0_next, double* solve_t0,
                                             int32_t* first_step, int32_t* active, void* stream) {
  ilqg_status s = check_plan(p, plan_rows, plan_xs, plan_us, plan_P, plan_alpha, plan_len, plan_t0);
  if (s != ILQG_OK) return s;
  if (!x || !xs || !us || !P || !alpha || !x0_next || !solve_t0 || !first_step || !active)
    return fail(ILQG_ERR_INVALID, "null argument");
  if (xs == plan_xs || us == plan_us || P == plan_P || alpha == plan_alpha)
    return fail(ILQG_ERR_INVALID, "the next solve's buffers must not alias the stored plan");
  if (p->has_route_progress) return fail(ILQG_ERR_UNSUPPORTED, kRouteProgressReceding);
  if (ilqg_status st = refuse_time_reading_dynamics(p, "receding horizon")) return st;
  if (batch <= 0) return ILQG_OK;
  if (ilqg_status sb = instance_batch_check(p, batch, false)) return sb;
  const DevProblem& d = p->dev;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    RecedingArgs<T> g{};
    g.plan = PlanBuffers<T>{(T*)plan_xs, (T*)plan_us, (T*)plan_P, (T*)plan_alpha, (int*)plan_len,
                              (double*)plan_t0, 0.0, plan_rows};
    g.x = (const T*)x; g.t = t; g.planner_runtime = planner_runtime;
    g.xs = (T*)xs; g.us = (T*)us; g.P = (T*)P; g.alpha = (T*)alpha; g.x0_next = (T*)x0_next;
    g.solve_t0 = solve_t0; g.first_step = first_step; g.active = active;
    auto kern = p->has_expression_dynamics ? receding_sync_kernel<T, true> : receding_sync_kernel<T, false>;
    return launch(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(T),
                  (hipStream_t)stream, d, g);
  });
}

ilqg_status ilqg_solution_splice_batch(const ilqg_problem* p, int32_t batch, int32_t plan_rows, void* plan_xs,
                                       void* plan_us, void* plan_P, void* plan_alpha, int32_t* plan_len,
                                       double* plan_t0, const void* xs, const void* us, const void* P,
                                       const void* alpha, const double* solve_t0, const int32_t* converged,
                                       const int32_t* active, void* stream) {
  ilqg_status s = check_plan(p, plan_rows, plan_xs, plan_us, plan_P, plan_alpha, plan_len, plan_t0);
  if (s != ILQG_OK) return s;
  if (!xs || !us || !P || !alpha || !solve_t0) return fail(ILQG_ERR_INVALID, "null argument");
  if (plan_rows < p->dev.T + 5)
    return fail(ILQG_ERR_INVALID, "plan_rows must leave room for five saved rows (T + 5)");
  if (batch <= 0) return ILQG_OK;
  const DevProblem& d = p->dev;
  return with_dtype(p->desc.dtype, [&](auto tag) {
    using T = decltype(tag);
    SpliceArgs<T> g{};
    g.plan = PlanBuffers<T>{(T*)plan_xs, (T*)plan_us, (T*)plan_P, (T*)plan_alpha, plan_len, plan_t0,
                              0.0, plan_rows};
    g.xs = (const T*)xs; g.us = (const T*)us; g.P = (const T*)P; g.alpha = (const T*)alpha;
    g.solve_t0 = solve_t0; g.converged = converged; g.active = active;
    return launch(splice_kernel<T>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d, g);
  });
}

}  // extern "C"

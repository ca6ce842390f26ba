// ilqg_launch.hpp — DimsLaunch<T, n, N, m_i>: the host side of one instantiated shape.  Its launchers of the stand-alone
// sweeps, the row stage and the padded sweeps, and its solve: the compile-time facts of the shape (shape_traits), the
// schedule's decisions as kernel addresses (for_row_program, the *_kernel_of pickers, bind_plan), the rounds.
// ilqg_dims.hip instantiates it for one shape; the main unit (ilqg_api.hip) for the run-time-dimensioned kernels (n = 0).
#pragma once

#include <type_traits>

#include "ilqg_kernels.hpp"
#include "ilqg_lq_padded.hpp"
#include "ilqg_problem.hpp"
#include "ilqg_rounds.hpp"
#include "ilqg_rowprog_static.hpp"  // ILQG_STATIC_PROGS
#include "ilqg_schedule.hpp"
#include "ilqg_shared.hpp"

using namespace ilqg;

// Launchers of the kernels that are instantiated per (n, N, m_i).  Members are defined out of class (not inline),
// so `extern template struct DimsLaunch<...>` in the main unit leaves their code — and the kernels behind them — to the
// unit that instantiates them explicitly (ilqg_dims.hip).
template <typename T, int NX, int NP, int MU>
struct __attribute__((visibility("hidden"))) DimsLaunch {
  static ilqg_status lq(const ilqg_dims* d, const PairTable& pt, const void* A, const void* Bm, const void* Q,
                        const void* l, const void* R, const void* r, const void* x0, void* P, void* alpha, void* dx,
                        hipStream_t stream);
  static ilqg_status lq_openloop(const ilqg_dims* d, const PairTable& pt, const void* A, const void* Bm,
                                 const void* Q, const void* l, const void* R, const void* r, const void* x0, void* P,
                                 void* alpha, void* dx, void* costates, hipStream_t stream);
  static ilqg_status solve(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P, void* alpha,
                           void* total_costs, int32_t* iters, int32_t* status, int32_t* converged, void* workspace,
                           const ilqg_solve_options& opt, hipStream_t stream);
  // pointers in QuadBatchArgs' order: xs us lambdas mu t_extreme A Bm Q l R r merit_part cost_part active
  // expr: the problem holds an expression cost (ilqg_problem::has_expression)
  static ilqg_status rows(const DevProblem& d, int32_t batch, const void* const* ptrs, bool expr, hipStream_t stream);
  // the sweep of a run-time-dimensioned solve whose game is embedded in this shape (padded_lq_kernel);
  // pad_elems_out != nullptr: only report the scratch elements one instance needs
  static ilqg_status lq_padded(const DevProblem& d, const void* solve_args, const PairTable& ptp, void* pad,
                               size_t* pad_elems_out, bool open_loop, hipStream_t stream);
  // ilqg_lq_feedback_batch / ilqg_lq_openloop_batch of a game embedded in this shape (padded_lq_batch_kernel): `d`, `pt`
  // are the game's own dimensions and control blocks, `ptp` its blocks at MU x MU
  static ilqg_status lq_padded_batch(const ilqg_dims* d, const PairTable& pt, const PairTable& ptp, bool open_loop,
                                     const void* A, const void* Bm, const void* Q, const void* l, const void* R,
                                     const void* r, const void* x0, void* P, void* alpha, void* dx, hipStream_t stream);
};

template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::rows(const DevProblem& d, int32_t batch, const void* const* q, bool expr,
                                            hipStream_t stream) {
  const QuadBatchArgs<T> g{(const T*)q[0], (const T*)q[1], (const T*)q[2], (const T*)q[3], (const int*)q[4], (T*)q[5],
                           (T*)q[6], (T*)q[7], (T*)q[8], (T*)q[9], (T*)q[10], (T*)q[11], (T*)q[12], (const int*)q[13]};
  // the widest chunk that leaves a CU three workgroups of this kernel
  const int cw = rows_chunk_width(d.n, d.m, d.rp_pslots, d.rp_lslots, sizeof(T), size_t(48) * 1024);
  const size_t lds = rows_maps_bytes(d) + rows_lds_elems(d.n, d.m, d.rp_pslots, d.rp_lslots, cw) * sizeof(T);
  auto kern = expr ? rows_kernel<T, NX, NP, MU, true> : rows_kernel<T, NX, NP, MU>;
  // (a problem that holds an expression subsystem: the interpreter that linearises it; such a problem sits in a
  // plain-RK4 shape or on the run-time-dimensioned path)
  if constexpr (NX == 0 || dims_use_plain_rk4(NX, NP, MU)) {
    bool xdyn = false;
    for (int i = 0; i < d.N; i++) xdyn = xdyn || d.sub_kind[i] == ILQG_DYN_EXPRESSION;
    if (xdyn) kern = rows_kernel<T, NX, NP, MU, true, true>;
  }
  raise_lds_limit((const void*)kern, lds);
  return launch(kern, dim3((d.T + cw - 1) / cw, batch), dim3(64), lds, stream, d, g, cw);
}

template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::lq(const ilqg_dims* d, const PairTable& pt, const void* A, const void* Bm,
                                          const void* Q, const void* l, const void* R, const void* r, const void* x0,
                                          void* P, void* alpha, void* dx, hipStream_t stream) {
  using C = LQCfg<T, NX, NP, MU>;
  LQBatchArgs<T> g(d, A, Bm, Q, l, R, r, x0, P, alpha, dx);
  if (dx) {
    const size_t need = size_t(d->batch) * d->T * (NP * (NX + 1) + NX) * sizeof(T);
    ilqg_status s = Scratch().reserve(need);
    if (s != ILQG_OK) return s;
    g.scratch = (T*)ilqg_shared::scratch_state().ptr;
  }
  // ilqg_dims::sweep_formulation = ILQG_CHOICE_OFF selects the VALU/LDS formulation where the MFMA one is the default
  const bool valu = C::USE_MFMA && d->sweep_formulation == ILQG_CHOICE_OFF;
  const bool use_pw = C::USE_MFMA && !valu;
  const size_t lds = size_t(use_pw ? MfmaSweepLds<T, NX, NP, MU>::ELEMS : C::LDS_ELEMS) * sizeof(T);
  auto kern = valu ? lq_feedback_kernel<T, NX, NP, MU, true> : lq_feedback_kernel<T, NX, NP, MU, false>;
  const int nt = valu ? LQFeedbackThreads<T, NX, NP, MU, true>::NT : LQFeedbackThreads<T, NX, NP, MU, false>::NT;
  raise_lds_limit((const void*)kern, lds);
  return launch(kern, dim3(d->batch), dim3(nt), lds, stream, g, pt);
}

template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::lq_openloop(const ilqg_dims* d, const PairTable& pt, const void* A,
                                                   const void* Bm, const void* Q, const void* l, const void* R,
                                                   const void* r, const void* x0, void* P, void* alpha, void* dx,
                                                   void* costates, hipStream_t stream) {
  using O = OLCfg<T, NX, NP, MU>;
  LQBatchArgs<T> g(d, A, Bm, Q, l, R, r, x0, P, alpha, dx);
  g.costates = (T*)costates;
  const size_t need = size_t(d->batch) * d->T * (costates ? O::ROW_FAT : O::ROW) * sizeof(T);
  ilqg_status s = Scratch().reserve(need);
  if (s != ILQG_OK) return s;
  g.scratch = (T*)ilqg_shared::scratch_state().ptr;
  g.adaptive = 0;
  const size_t lds = size_t(O::LDS_ELEMS) * sizeof(T);
  auto kern = lq_openloop_kernel<T, NX, NP, MU>;
  raise_lds_limit((const void*)kern, lds);
  return launch(kern, dim3(d->batch), dim3(O::NT), lds, stream, g, pt);
}

template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::lq_padded(const DevProblem& d, const void* solve_args, const PairTable& ptp,
                                                 void* pad, size_t* pad_elems_out, bool open_loop, hipStream_t stream) {
  if constexpr (NX == 0) {
    return fail(ILQG_ERR_UNSUPPORTED, "no shape to embed the game in");
  } else {
    auto go = [&](auto ol) -> ilqg_status {
      constexpr bool OL = decltype(ol)::value;
      const PadLayout<T, NX, NP, MU, OL> PL(d.T, ptp.Rsz, ptp.rsz);
      if (pad_elems_out) {
        *pad_elems_out = PL.total;
        return ILQG_OK;
      }
      const SolveArgs<T>& sa = *static_cast<const SolveArgs<T>*>(solve_args);
      PadArgs<T> pa{(T*)pad, PL.total, ptp};
      using PS = PadSweep<T, NX, NP, MU, OL>;
      auto kern = padded_lq_kernel<T, NX, NP, MU, OL>;
      const size_t lds = PS::LDS_ELEMS * sizeof(T);
      raise_lds_limit((const void*)kern, lds);
      return launch(kern, dim3(sa.batch), dim3(PS::NT), lds, stream, d, sa, pa);
    };
    return open_loop ? go(std::true_type{}) : go(std::false_type{});
  }
}

template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::lq_padded_batch(const ilqg_dims* d, const PairTable& pt, const PairTable& ptp,
                                                       bool open_loop, const void* A, const void* Bm, const void* Q,
                                                       const void* l, const void* R, const void* r, const void* x0,
                                                       void* P, void* alpha, void* dx, hipStream_t stream) {
  if constexpr (NX == 0) {
    return fail(ILQG_ERR_UNSUPPORTED, "no shape to embed the game in");
  } else {
    auto go = [&](auto ol) -> ilqg_status {
      constexpr bool OL = decltype(ol)::value;
      const PadLayout<T, NX, NP, MU, OL> PL(d->T, ptp.Rsz, ptp.rsz);
      const ilqg_status s = Scratch().reserve(size_t(d->batch) * PL.total * sizeof(T));
      if (s != ILQG_OK) return s;
      const GenDims gd = gen_dims_of(d->n, d->num_players, d->udim, d->T);
      const LQBatchArgs<T> g(d, A, Bm, Q, l, R, r, x0, P, alpha, dx);
      PadArgs<T> pa{(T*)ilqg_shared::scratch_state().ptr, PL.total, ptp};
      using PS = PadSweep<T, NX, NP, MU, OL>;
      auto kern = padded_lq_batch_kernel<T, NX, NP, MU, OL>;
      const size_t lds = PS::LDS_ELEMS * sizeof(T);
      raise_lds_limit((const void*)kern, lds);
      return launch(kern, dim3(d->batch), dim3(PS::NT), lds, stream, g, gd, pt, pa);
    };
    return open_loop ? go(std::true_type{}) : go(std::false_type{});
  }
}

// The compile-time facts of an instantiation the schedule's policy reads (ShapeTraits, ilqg_schedule.hpp)
template <typename T, int NX, int NP, int MU>
constexpr ShapeTraits shape_traits() {
  using C = LQCfg<T, NX, NP, MU>;
  using O = OLCfg<T, NX, NP, MU>;
  using W1 = W1Cfg<T, NX, NP, MU>;
  static_assert(O::ROW == ol_row_elems(NX, NP * MU, NP) && O::ROW_FAT == ol_row_elems(NX, NP * MU, NP, true), "ol_row_elems");
  ShapeTraits t{};
  t.nx = NX; t.np = NP; t.mu = MU; t.elem = int(sizeof(T));
  t.trial_waves = TrialWaves<T>::W;
  t.use_mfma = C::USE_MFMA;
  t.one_tile = C::MFMA_ONE_TILE;
  t.has_1w = W1::SUPPORTED && C::USE_MFMA && C::MFMA_ONE_TILE;
  t.has_packed = sizeof(T) == 4 && C::USE_MFMA && C::MFMA_ONE_TILE && NP == 3;
  if constexpr (C::USE_MFMA) {
    t.has_forms = C::MFMA_ONE_TILE && SolveRows<NP * MU, NX + 1>::FITS;
    t.has_bconst = t.has_forms && NX < 16 && MU == 2;
    t.pw_lds_elems = MfmaSweepLds<T, NX, NP, MU>::ELEMS + (C::MFMA_ONE_TILE ? 0 : 4);
  }
  if constexpr (W1::SUPPORTED && C::USE_MFMA && C::MFMA_ONE_TILE) t.w1_lds_elems = W1::ELEMS;
  t.w1_words = W1::kWords;
  t.ol_threads = O::NT; t.ol_lds_elems = O::LDS_ELEMS;
  t.valu_threads = C::NT; t.valu_lds_elems = C::LDS_ELEMS;
  t.fwd_elems = 4 * 2 * ((NX * NX + C::SCR + 3) & ~3) + 2 * NX + 8;
  t.pairs = rollout_pairs(NX, NP, MU);
  t.may_xdyn = dims_use_plain_rk4(NX, NP, MU);
  t.rows_in_regs = rows_state_in_registers(NX, NP * MU);
  t.partials_room = fused_partials_room(int(sizeof(T)), NX, NP, MU);
  t.lane_width = rollout_lanes_per_wave(NP > 0 ? NP : 1);
#define X(ID_, NX_, NP_, MU_)                                                             \
  if constexpr (NX_ == NX && NP_ == NP && MU_ == MU) {                                   \
    t.static_ids[t.num_static] = ID_;                                                     \
    t.static_in_regs[t.num_static++] = static_prog_in_registers<StaticRowProg<ID_>>();    \
  }
  ILQG_STATIC_PROGS(X)
#undef X
  return t;
}

inline ProblemFacts problem_facts(const ilqg_problem* p) {
  return {p->desc.params, p->static_prog, p->b_constant, p->has_expression, p->has_expression_dynamics, p->bindings.any(),
          p->dev.inst_solver != 0};
}

// The one place a row program's (kind, bound, static id) picks an instantiation: f(PROGID, BOUND) as integral constants,
// for the fused trial kernel, the split row kernel and the probing row kernel of a shape (NX = 0: the run-time-dimensioned
// kernels).  A registered structure goes before the expression kinds (it holds none); a problem with per-instance tables
// bound runs twins of its own where the kernel has one (ilqg_solve.hpp).
template <typename R, int NX, int NP, int MU, typename F>
R for_row_program(int prog_kind, int static_id, bool bound, F f) {
  using Bound = std::true_type;
  using Unbound = std::false_type;
#define X(ID_, NX_, NP_, MU_)                                  \
  if constexpr (NX_ == NX && NP_ == NP && MU_ == MU)           \
    if (static_id == ID_)                                      \
      return bound ? f(std::integral_constant<int, kBoundProg + ID_>{}, Bound{}) : f(std::integral_constant<int, ID_>{}, Unbound{});
  ILQG_STATIC_PROGS(X)
#undef X
  if constexpr (NX == 0 || dims_use_plain_rk4(NX, NP, MU))
    if (prog_kind == PROG_EXPR_DYN)
      return bound ? f(std::integral_constant<int, kExprDynProg>{}, Bound{}) : f(std::integral_constant<int, kExprDynProg>{}, Unbound{});
  if (prog_kind == PROG_EXPR)
    return bound ? f(std::integral_constant<int, kExprProg>{}, Bound{}) : f(std::integral_constant<int, kExprProg>{}, Unbound{});
  return bound ? f(std::integral_constant<int, 0>{}, Bound{}) : f(std::integral_constant<int, 0>{}, Unbound{});
}
template <typename T>
using SolveKernel = void (*)(DevProblem, SolveArgs<T>);
template <typename T, int NX, int NP, int MU>
SolveKernel<T> rows_kernel_of(int prog_kind, int static_id, bool bound) {
  return for_row_program<SolveKernel<T>, NX, NP, MU>(prog_kind, static_id, bound, [](auto id, auto) {
    return SolveKernel<T>(ilq_rows_kernel<T, NX, NP, MU, decltype(id)::value>);
  });
}
template <typename T, int NX, int NP, int MU>
SolveKernel<T> probe_rows_kernel_of(int prog_kind, int static_id, bool bound) {
  return for_row_program<SolveKernel<T>, NX, NP, MU>(prog_kind, static_id, bound, [](auto id, auto) {
    return SolveKernel<T>(ilq_probe_rows_kernel<T, NX, NP, MU, decltype(id)::value>);
  });
}

// The sweep instantiation of (sweep_kind, sweep_forms)
template <typename T, int NX, int NP, int MU>
SolveKernel<T> sweep_kernel_of(const SolveSchedule& s) {
  static constexpr ShapeTraits st = shape_traits<T, NX, NP, MU>();
  if (s.sweep_kind == LQ_OPEN_LOOP_COMPACT) return ilq_lq_kernel<T, NX, NP, MU, LQ_OPEN_LOOP_COMPACT>;
  if (s.sweep_kind == LQ_OPEN_LOOP) return ilq_lq_kernel<T, NX, NP, MU, LQ_OPEN_LOOP>;
  if constexpr (!st.use_mfma) {
    return ilq_lq_kernel<T, NX, NP, MU, LQ_VALU_FEEDBACK>;
  } else {
    auto forms_of = [&](auto kind) -> SolveKernel<T> {
      constexpr int KIND = decltype(kind)::value;
      if constexpr (st.has_bconst && KIND != LQ_SINGLE_WAVE)
        if (s.sweep_forms == 2) return ilq_lq_kernel<T, NX, NP, MU, KIND, 2>;
      if constexpr (st.has_forms)
        if (s.sweep_forms == 0) return ilq_lq_kernel<T, NX, NP, MU, KIND, 0>;
      return ilq_lq_kernel<T, NX, NP, MU, KIND>;
    };
    if constexpr (st.has_1w)
      if (s.sweep_kind == LQ_SINGLE_WAVE) return forms_of(std::integral_constant<int, LQ_SINGLE_WAVE>{});
    if constexpr (st.has_packed)
      if (s.sweep_kind == LQ_PLAYER_WAVES_PACKED) return forms_of(std::integral_constant<int, LQ_PLAYER_WAVES_PACKED>{});
    return forms_of(std::integral_constant<int, LQ_PLAYER_WAVES>{});
  }
}

// A schedule's decisions as kernel addresses: nothing is decided here.
template <typename T, int NX, int NP, int MU>
RoundPlan<T> bind_plan(const SolveSchedule& s) {
  constexpr int W = TrialWaves<T>::W;
  constexpr bool kMayXdyn = dims_use_plain_rk4(NX, NP, MU);
  RoundPlan<T> plan;
  plan.s = s;
  plan.trial = {for_row_program<SolveKernel<T>, NX, NP, MU>(s.prog_kind, s.static_prog, s.bound != 0, [](auto id, auto bound) {
                  return SolveKernel<T>(ilq_trial_kernel<T, NX, NP, MU, W, decltype(id)::value, decltype(bound)::value>);
                }), 64 * W, size_t(s.lds_trial)};
  plan.sweep = {sweep_kernel_of<T, NX, NP, MU>(s), s.sweep_threads, size_t(s.lds_sweep)};
  plan.exit = {ilq_exit_kernel<T, NX, NP, MU>, s.nt_exit, size_t(s.lds_exit)};
  if (!s.lists) return plan;
  plan.roll = {ilq_roll_kernel<T, NX, NP, MU>, 64, size_t(s.lds_roll)};
  plan.rows = {rows_kernel_of<T, NX, NP, MU>(s.prog_kind, s.static_id, s.bound != 0), 64, size_t(s.lds_rows)};
  plan.decide = {s.decide_solver ? ilq_decide_kernel<T, NX, NP, MU, true> : ilq_decide_kernel<T, NX, NP, MU, false>, 64, size_t(s.lds_decide)};
  plan.prows = {probe_rows_kernel_of<T, NX, NP, MU>(s.prog_kind, s.static_id, s.bound != 0), 64, size_t(s.lds_prows)};
  plan.proll = {ilq_probe_roll_kernel<T, NX, NP, MU>, 64, size_t(s.lds_proll)};
  plan.proll_fat = {ilq_probe_roll_kernel<T, NX, NP, MU, sizeof(T) == 8>, 64, size_t(s.lds_proll)};  // (fp32: the same kernel)
  if (s.proll_single) plan.proll_single = {ilq_probe_roll_kernel<T, NX, NP, MU, sizeof(T) == 8, true>, 64, size_t(s.lds_proll_single)};
  if (s.proll_lanes) plan.proll_lanes = {ilq_probe_roll_lanes_kernel<T, NX, NP, MU>, 64, size_t(s.lds_proll_lanes)};
  if constexpr (kMayXdyn)  // (a plain-RK4 shape: one rollout per wavefront, no paired or lane-per-candidate form)
    if (s.prog_kind == PROG_EXPR_DYN) {
      plan.roll.kernel = ilq_roll_kernel<T, NX, NP, MU, true>;
      plan.proll.kernel = ilq_probe_roll_kernel<T, NX, NP, MU, false, false, true>;
      plan.proll_fat.kernel = ilq_probe_roll_kernel<T, NX, NP, MU, sizeof(T) == 8, false, true>;
    }
  return plan;
}

// The specialised solve: its arguments, the mask's count where the schedule wants it (the only device interaction before
// the rounds), the schedule (decide_schedule, ilqg_schedule.hpp), its kernels (bind_plan), the rounds.
template <typename T, int NX, int NP, int MU>
ilqg_status DimsLaunch<T, NX, NP, MU>::solve(ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us,
                                             void* P, void* alpha, void* total_costs, int32_t* iters, int32_t* status,
                                             int32_t* converged, void* workspace, const ilqg_solve_options& opt,
                                             hipStream_t stream) {
  const DevProblem& d = p->dev;
  SolveTail<T> tail;
  SolveArgs<T> sa = solve_args_of<T>(p, batch, x0, xs, us, P, alpha, total_costs, iters, status, converged, workspace, opt, &tail);
#if ILQG_DIAGNOSTIC_BUILD
  sa.prof = g_prof;
#endif
  // ws_tail places the lists behind the augmented-Lagrangian layout (the larger one): whatever al_mode this solve runs in
  if (ws_layout_of(d, sa.ol_row, 1).total < ws_layout_of(d, sa.ol_row, sa.al_mode).total)
    return fail(ILQG_ERR_INVALID, "workspace layout: the tail offset does not cover this solve's per-instance blocks");
  int sched_batch = batch;
  if (schedule_counts_mask(opt)) {
    int active = 0;
    if (const ilqg_status s = ilqg_shared::count_active_instances(p, opt.active, int(batch), stream, &active)) return s;
    sched_batch = active > 0 ? active : 1;
  }
  int num_cus = 256, dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) num_cus = prop.multiProcessorCount;
  static constexpr ShapeTraits traits = shape_traits<T, NX, NP, MU>();
  const SolveSchedule s = decide_schedule(traits, d, problem_facts(p), opt, batch, sched_batch, num_cus, kProfile);
  sa.rows_cw = s.rows_cw;
  sa.compact = s.compact;
  sa.defer_forward = s.defer_forward;
  sa.prio_div = s.prio_div;
  sa.lds_part = s.lds_part;
  sa.clear_counters = 1;
  p->last_schedule = s.word;
  return run_rounds(p, sa, tail, bind_plan<T, NX, NP, MU>(s), opt, stream);
}

// ilqg_decide_schedule.hpp — decide_schedule's definition (ilqg_schedule.hpp declares it and says what it decides),
// beside the host-side size functions of the solve and the sweeps that it calls.  Included by the main unit alone.
#pragma once

#include "ilqg_lq.hpp"
#include "ilqg_rows.hpp"
#include "ilqg_schedule.hpp"
#include "ilqg_solve.hpp"
#include "ilqg_stages.hpp"

namespace ilqg {

SolveSchedule decide_schedule(const ShapeTraits& st, const DevProblem& d, const ProblemFacts& f, const ilqg_solve_options& opt,
                              int batch, int sched_batch, int num_cus, bool profile_build) {
  (void)batch;
  SolveSchedule s{};
  const ilqg_solver_params& prm = f.prm;
  const bool open_loop = prm.open_loop != 0, al_mode = opt.augmented_lagrangian != 0;
  const bool fixed = opt.fixed_iters > 0 && !al_mode;
  const size_t elem = size_t(st.elem);
  const int W = st.trial_waves;
  const WsLayout L = ws_layout_of(d, open_loop ? ol_row_elems(d.n, d.m, d.N) : 0, al_mode ? 1 : 0);
  auto trial_lds = [&](int cw, bool xreg) { return elem == 4 ? trial_lds_bytes<float>(d, W, cw, xreg) : trial_lds_bytes<double>(d, W, cw, xreg); };
  auto phase_lds = [&](int phase, int cw) { return elem == 4 ? trial_phase_lds_bytes<float>(d, phase, cw) : trial_phase_lds_bytes<double>(d, phase, cw); };
  s.sched_batch = sched_batch;
  s.num_cus = num_cus;
  s.probe_max = kProbeCandidates;
  s.probe_budget = kProbeRoundBudget;
  s.bound = f.bound;
  // (a problem that holds an expression subsystem, in the two plain-RK4 shapes: kExprDynProg, the rollout with the
  // expression integrator and the interpreter that linearises it; one that holds an expression cost: kExprProg, the
  // interpreter with the evaluator in it — in the fused kernel, the split row kernel and the merit-only one)
  s.prog_kind = (st.may_xdyn && f.has_expression_dynamics) ? PROG_EXPR_DYN : f.has_expression ? PROG_EXPR : PROG_PLAIN;
  // Rows per chunk of the row stage as the interpreter runs it: the widest whose scratch lets a CU hold four instances
  // of the fused trial kernel (the headline batch is four instances per CU); the split row kernels get the same width.
  const size_t per_instance = kLdsPerCu / kTrialInstancesPerCu;
  const size_t fixed_lds = rows_maps_bytes(d) + ((rollout_lds_elems(d.n, d.m) + 3) & ~size_t(3)) * elem + 16;
  const int cw_interpreted = rows_chunk_width(d.n, d.m, d.rp_pslots, d.rp_lslots, elem,
                                              per_instance > fixed_lds ? (per_instance - fixed_lds) / trial_row_waves(W) : 0);
  const bool pw = st.use_mfma && !open_loop;  // one wave per player (MFMA feedback sweep)
  // Compact rows (ilqg_common.hpp) between the row stage and the sweep: the one-tile player-parallel sweep and the
  // open-loop sweep read them; the other sweeps take the dense arrays.  What the row stage writes and the sweep reads
  // per time step shrinks from N (n^2 + n) + ... words to the ones a cost term can touch.
  // ... and only when the [T][rp_compact_w] rows fit the space they are kept in: the dense Q, l, R, r arrays up to the
  // sweep's scratch rows (a small or densely coupled problem's row carries the A and B words too)
  const bool compact_on = d.rp_compact_w > 0 && size_t(d.T) * size_t(d.rp_compact_w) <= L.lqscr - L.Q && choice(opt.compact_rows, true);
  s.compact = (pw && st.one_tile && compact_on) || (open_loop && compact_on);
  // A registered row-program structure (ilqg_rowprog_static.hpp): the row stage as straight-line code for it — in the
  // fused kernel (state rows in registers, i.e. without the chunk's (x, u) image in LDS, so it takes the 64-row chunk
  // where the interpreter's scratch would not fit four instances on a CU: n = 16 in fp64), in the split row kernel and
  // in the merit-only row kernel of the speculative line search.  Same results, bit for bit.
  // (the static kernels exist for solves on compact rows: they write nothing dense)
  if (opt.static_rows != ILQG_CHOICE_OFF && s.compact)
    for (int q = 0; q < st.num_static; q++)
      if (f.static_prog == st.static_ids[q]) {
        s.static_id = st.static_ids[q];
        s.static_in_regs = st.static_in_regs[q];  // the slots of a chunk in registers (ilqg_rows.hpp: no row scratch in LDS)
      }
  // ... the fused kernel's: the one the trial launch is bound to, run unless the pass is split
  s.static_prog = (s.static_id && st.rows_in_regs && trial_lds(64, true) <= per_instance) ? s.static_id : 0;
  const int cw_fused = s.static_prog ? 64 : cw_interpreted;
  s.lds_trial = int32_t(trial_lds(cw_fused, s.static_prog != 0));
  // (the exit kernel copies an instance's final iterate, T m n words of strategies among them: four waves where the
  // instances are few and the kernel is a link of the round's chain, one where they share the chip's bandwidth anyway)
  s.nt_exit = sched_batch <= 2 * num_cus ? 256 : 64;
  // The throughput form of the one-tile feedback sweep — one wave per instance, twice the instances per CU
  // (ilqg_lq_feedback1w.hpp) — for batches of five or more instances per CU (measured, n = 14 fp64: B = 1024 1.47 M it/s
  // player-parallel vs 1.11 M single-wave; 1280: 1.09 vs 1.10; 1536: 1.17 vs 1.25; 2048: 1.20 vs 1.45; 8192: 1.45 vs
  // 1.68); it reads compact rows and leaves the forward pass to the trial kernel.
  // ilqg_solve_options::single_wave_sweep overrides the choice (same results to rounding).
  // `decrease`: its expected decrease has a source — its own adjoint recursion, or — only possible with the fused trial
  // kernel, whose row wave runs it — the deferred forward pass over the sweep's scratch rows.
  auto one_wave_sweep = [&](bool compact_rows, bool decrease) {
    return st.has_1w && pw && compact_rows && !profile_build && decrease && d.rp_compact_w <= st.w1_words &&
           choice(opt.single_wave_sweep, !opt.deterministic && size_t(sched_batch) >= size_t(5) * num_cus);
  };
  // Split passes: where the fused kernel cannot keep four instances on a CU (n = 24), and for batches that are several
  // times what it keeps resident when the split integration kernel (a quarter of the registers, 4 KB of LDS) gains from
  // the co-residency — measured: n = 24, B = 4096: 65 k vs 39 k it/s.  For n <= 16 the fused kernel stays
  // (round 3, with compact rows: n = 14 fp32, B = 8192: 1.97 M fused vs 1.79 M split; fp64: 1.34 M vs 1.27 M) ...
  // ... except wherever the single-wave sweep will run with its adjoint pass: it takes its expected decrease from there, so
  // nothing is left for the fused kernel's row wave to overlap with the rollout, and the three split kernels each keep
  // more instances on a CU than the fused one (measured, n = 14, B = 8192, LQ single-wave + adjoint: fp64 1.58 M it/s
  // fused vs 1.65 M split, fp32 2.61 M vs 2.77 M; B = 2048 fp64 1.40 M vs 1.50 M).  That sweep is foreseen here on what the
  // options allow (compact_on, an adjoint pass not refused); single_wave below is the one that runs.
  // The host then counts every round: an instance may ask for another pass (back-tracking) before its sweep.
  // ilqg_solve_options::split_trial overrides the choice; the phase profile reads the fused kernel's counters.
  const bool big_batch = size_t(sched_batch) >= size_t(8) * num_cus;
  s.split = !profile_build && !opt.forced_steps &&
            choice(opt.split_trial, kTrialInstancesPerCu * size_t(s.lds_trial) > kLdsPerCu || (big_batch && st.nx > 16) ||
                                        one_wave_sweep(compact_on, opt.adjoint_expected_decrease != ILQG_CHOICE_OFF));
  const bool fused_static = !s.split && s.static_prog;
  // The split row kernel interprets the program at the interpreter's width; it is one wave per chunk with the chunk's
  // scratch to itself, and its instances per CU are what the scratch leaves room for: chunks of equal width (T = 100:
  // 2 x 50 rows, 28 KB, five per CU — not 64 + 36 at 36 KB and four).
  const int split_chunks = (d.T + cw_interpreted - 1) / cw_interpreted;
  s.rows_cw = s.split ? (d.T + split_chunks - 1) / split_chunks : cw_fused;
  s.row_chunks = (d.T + s.rows_cw - 1) / s.rows_cw;
  s.counted = !opt.forced_steps && (s.split || !fixed || choice(opt.counted, false));
  // Hand-off: whenever the host counts rounds anyway, the fused kernel keeps an instance only until its line
  // search rejects a step; the back-tracking instances then go through split passes with the speculative line
  // search (ilqg_solve_options::handoff = OFF keeps every pass in the fused kernel).
  s.handoff = s.counted && !s.split && !profile_build && prm.linesearch && choice(opt.handoff, true);
  s.lists = s.split || s.handoff;
  // The sweep's forward pass runs in the fused trial kernel that follows it, beside the rollout, whenever that is the
  // kernel that follows (split passes and the open-loop sweep keep it in the sweep's kernel) and its scratch fits the
  // row wave's.
  const bool may_defer = !s.split && !open_loop && trial_rows_elems(d, s.rows_cw, fused_static) >= st.fwd_elems + 8;
  s.adjoint = choice(opt.adjoint_expected_decrease, !may_defer);
  s.single_wave = one_wave_sweep(s.compact, s.adjoint || may_defer);
  // (a single-wave sweep with the adjoint pass forms the expected decrease itself: no forward pass anywhere)
  s.defer_forward = may_defer && !(s.single_wave && s.adjoint);
  // the whole batch resident at once (four instances per CU): fair issue arbitration among the co-resident instances
  s.prio_div = (!s.single_wave && sched_batch > num_cus && sched_batch <= 4 * num_cus) ? num_cus : 0;
  // The sweep kernel.  The open-loop sweep's LDS is its own working set plus the slot the expected decrease is handed
  // over in (n = 24: 54 KB, three instances per CU; the feedback layout would take 85 KB).  fp32, one-tile sweep of
  // three player waves, many instances per CU: the 128-register build (see ilq_lq_kernel).
  s.sweep_forms = 1;
  if (open_loop) {
    s.sweep_kind = s.compact ? LQ_OPEN_LOOP_COMPACT : LQ_OPEN_LOOP;
    s.sweep_threads = st.ol_threads;
    s.lds_sweep = int32_t((st.ol_lds_elems + 4) * elem);
  } else if (!st.use_mfma) {
    s.sweep_kind = LQ_VALU_FEEDBACK;
    s.sweep_threads = st.valu_threads;
    s.lds_sweep = int32_t(st.valu_lds_elems * elem);
  } else {
    // ilqg_solve_options::sweep_forms = OFF: the read-lane instantiation of the same kind (only where the two differ)
    const bool forms = choice(opt.sweep_forms, true);
    // ... and with the forms on, a problem whose B is constant entries, at most one per row and column (ilqg_problem::
    // b_constant), takes them from registers instead of the B tile — the solver's instantiation of the one-tile sweep with
    // a spare tile column and two controls per player, i.e. compact rows and the forward pass in the trial kernel
    s.b_const = st.has_bconst && forms && f.b_constant && s.compact && s.defer_forward && !s.single_wave;
    s.packed = st.has_packed && !s.single_wave && size_t(sched_batch) >= size_t(5) * 256;
    s.sweep_forms = s.b_const ? 2 : (st.has_forms && !forms) ? 0 : 1;
    s.sweep_kind = s.single_wave ? LQ_SINGLE_WAVE : s.packed ? LQ_PLAYER_WAVES_PACKED : LQ_PLAYER_WAVES;
    s.sweep_threads = s.single_wave ? 64 : 64 * st.np;
    s.lds_sweep = int32_t((s.single_wave ? st.w1_lds_elems + 4 : st.pw_lds_elems) * elem);
  }
  // The fused kernel with a register-held static row stage keeps the per-row partials of a trial's reductions in LDS as
  // well (trial_part_instance's running reductions) — where four instances still fit a CU with that block behind theirs.
  const size_t partials = partials_lds_elems(d.T, d.N) * elem;
  s.lds_part = fused_static && s.static_in_regs && W == 2 && st.partials_room &&
               kTrialInstancesPerCu * (size_t(s.lds_trial) + partials) <= kLdsPerCu;
  if (s.lds_part) s.lds_trial += int32_t(partials);
  s.lds_exit = int32_t(quad_tables_bytes(d, elem) + 64 * elem);
  s.pairs = st.pairs;  // two rollouts per wavefront (ilqg_stages.hpp)
  s.decide_solver = f.solver_bound;
  if (s.lists) {
    const size_t maps = s.compact ? 0 : rows_maps_bytes(d);  // the split row kernels' copy of the word maps
    // (a static row kernel whose slots are registers needs no scratch beyond the (x, u) image of shapes past 16 states)
    const size_t static_regs_lds = (st.rows_in_regs ? 0 : size_t(d.n + d.m) * 64) * elem + 16;
    const int cw = s.static_id ? 64 : s.rows_cw;
    const bool regs = s.static_id && s.static_in_regs;
    const int32_t lds_one = int32_t(phase_lds(TRIAL_ROLL, s.rows_cw));  // one rollout per wavefront
    s.lds_roll = s.lds_proll = st.pairs ? int32_t(size_t(rollout_pair_lds_elems(d.n, d.m)) * elem + 16) : lds_one;
    s.lds_proll_single = st.pairs ? lds_one : 0;
    s.lds_rows = int32_t(regs ? static_regs_lds : maps + split_rows_elems(d, st.nx, cw) * elem);
    s.lds_prows = int32_t(regs ? static_regs_lds : maps + probe_rows_elems(d, st.nx, cw) * elem);
    s.lds_decide = int32_t(phase_lds(TRIAL_DECIDE, s.rows_cw));
    s.lds_proll_lanes = st.pairs ? int32_t(size_t(rollout_lanes_lds_elems(d.n, d.m, d.N)) * elem + 16) : 0;
    s.proll_single = s.proll_lanes = st.pairs;
  }
  s.cap = al_mode ? (long long)(prm.max_solver_iters + 1) * (prm.unconstrained_solver_max_iters + 2) : (long long)prm.max_solver_iters + 2;
  if (s.counted) s.cap = (s.cap + 2) * ((long long)prm.max_backtracking_steps + 3);
  s.lane_width = st.lane_width;
  s.read_restarts = s.counted && al_mode;
  s.timed = opt.max_runtime > 0.0 && s.counted;  // (InnerClock reads the clock in front of every iteration: no bursts)
  s.bursts = s.counted && !profile_build && !s.timed && choice(opt.round_bursts, true);
  s.probe = s.lists && prm.linesearch && choice(opt.probe, true);
  s.lanes_auto = st.nx <= 16;
  s.deep_tails = 1;
  s.word = schedule_word(s, open_loop);
  return s;
}

}  // namespace ilqg

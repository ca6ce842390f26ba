// ilqg_schedule.hpp — how a solve runs, decided once in plain host code.
// decide_schedule turns a problem's scalars, the solve options, the batch and the device's CU count into a SolveSchedule:
// every AUTO decision as a named field.  DimsLaunch::solve (ilqg_api.hip) binds kernels from it (bind_plan) and
// run_rounds launches them, asking the per-round functions below what a probing round looks like; the host-only
// ilqg_schedule_build reports the same schedule without a device.  Nothing here calls HIP; the per-round functions
// compile without it (tests/host/schedule_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ilqg.h"

namespace ilqg {

// The schedule is the struct ilqg_schedule_build reports (ilqg.h): flags are 0 / 1.
typedef ilqg_schedule_info SolveSchedule;

// The row program a solve's row stage runs besides a registered static structure (SolveSchedule::prog_kind)
enum { PROG_PLAIN = 0, PROG_EXPR = 1, PROG_EXPR_DYN = 2 };
// The probing rollouts of a round (probe_form)
enum ProbeForm { PROBE_LANES = 0, PROBE_SINGLE = 1, PROBE_FAT = 2, PROBE_PAIRS = 3 };

// The compile-time facts of an instantiation (n, N, m_i) in one precision that the policy reads (shape_traits,
// ilqg_api.hip); kept beside the launch pointers in ShapeEntry.
struct ShapeTraits {
  int nx, np, mu, elem;       // elem: sizeof(T)
  int trial_waves;            // TrialWaves<T>::W
  bool use_mfma, one_tile;    // LQCfg: the MFMA feedback sweep, on one tile
  bool has_1w, has_forms, has_bconst, has_packed;  // sweep instantiations the shape has
  bool pairs, may_xdyn, rows_in_regs, partials_room;  // rollout_pairs, dims_use_plain_rk4, rows_state_in_registers, fused_partials_room
  int w1_words;               // W1Cfg::kWords: the widest compact row the single-wave sweep scatters
  int ol_threads, valu_threads;
  size_t w1_lds_elems, ol_lds_elems, valu_lds_elems, pw_lds_elems;  // LDS elements of the sweep kinds
  size_t fwd_elems;           // scratch of the deferred forward pass in the fused kernel's row wave
  int lane_width;             // rollout_lanes_per_wave
  int num_static;             // registered structures of this shape (ILQG_STATIC_PROGS): ids, slots in registers
  int static_ids[4];
  bool static_in_regs[4];
};

// What decide_schedule reads of a problem besides DevProblem's scalars
struct ProblemFacts {
  ilqg_solver_params prm;
  int static_prog;  // the registered structure its row program matches, 0: none
  bool b_constant, has_expression, has_expression_dynamics;
  bool bound;         // per-instance tables are bound (InstanceBindings::any)
  bool solver_bound;  // ... among them solver columns (DevProblem::inst_solver)
};

// The LDS of a CU (gfx950: 160 KB): the most one workgroup can be given, and what the workgroups resident on a CU share
constexpr size_t kLdsPerCu = size_t(160) * 1024;
// ... among the four instances per CU of the headline batch, which the fused trial kernel's LDS is sized for
constexpr size_t kTrialInstancesPerCu = 4;

inline bool choice(int32_t c, bool automatic) { return c == ILQG_CHOICE_ON ? true : (c == ILQG_CHOICE_OFF ? false : automatic); }

// The schedules are chosen by how many instances the chip will hold at once.  Under a mask that is the number
// of instances taking part, not the length of the buffers: a receding-horizon loop replans the few dozen plans
// still running of a batch of 2048 (src/receding_horizon_simulator.cpp:77), and the throughput forms chosen for 2048
// — single-wave sweep, adjoint expected decrease, split trial pass — are latency forms three times slower for them
// (config 5 as written: 400 us per sweep launch instead of 190).  A free-running solve waits for the device every
// round anyway, so it counts its mask first (one more read-back per call); a fixed-iteration solve stays
// asynchronous and keeps the buffer length.
inline bool schedule_counts_mask(const ilqg_solve_options& opt) {
  return opt.active && !opt.forced_steps && !opt.deterministic && !(opt.fixed_iters > 0 && !opt.augmented_lagrangian);
}

// The fixed schedule of the run-time-dimensioned solve (generic_solve), as its ILQG_SCHEDULE_* word
inline int generic_schedule_word(bool open_loop, bool padded) {
  return ILQG_SCHEDULE_GENERIC | ILQG_SCHEDULE_SPLIT_TRIAL | ILQG_SCHEDULE_COUNTED | (open_loop ? ILQG_SCHEDULE_OPEN_LOOP : 0) |
         (padded ? ILQG_SCHEDULE_PADDED_SWEEP : 0);
}
inline int schedule_word(const SolveSchedule& s, bool open_loop) {
  const bool static_rows = s.split ? s.static_id != 0 : s.static_prog != 0;
  return (s.single_wave ? ILQG_SCHEDULE_SINGLE_WAVE_SWEEP : 0) | ((s.single_wave && s.adjoint) ? ILQG_SCHEDULE_ADJOINT_DECREASE : 0) |
         (s.split ? ILQG_SCHEDULE_SPLIT_TRIAL : 0) | (s.compact ? ILQG_SCHEDULE_COMPACT_ROWS : 0) |
         (s.counted ? ILQG_SCHEDULE_COUNTED : 0) | (open_loop ? ILQG_SCHEDULE_OPEN_LOOP : 0) |
         (static_rows ? ILQG_SCHEDULE_STATIC_ROWS : 0) | (s.b_const ? ILQG_SCHEDULE_CONSTANT_B : 0);
}

struct DevProblem;
// Defined once, in the library's main unit (below); the units of a split build see this declaration only.
__attribute__((visibility("hidden"))) SolveSchedule decide_schedule(const ShapeTraits& st, const DevProblem& d, const ProblemFacts& f, const ilqg_solve_options& opt,
                              int batch, int sched_batch, int num_cus, bool profile_build);

// ---------------------------------------------------------------------------------------------------------------
// Per round of a line-search tail (run_rounds)
// ---------------------------------------------------------------------------------------------------------------

// Step sizes probed per listed instance in a round of a line-search tail: as many as the pool holds for a list this long,
// ramping up from `probe_first` in a tail's first round (ilqg_solve_options::probe_first) and doubling per round (most
// line searches that back-track at all end within a step or two; the ones that do not are mostly on their way through
// all max_backtracking_steps of a failing search, and a round for the few instances left costs the latency of its
// launches whatever it probes: 2, 4, 8, 16, 32, ...).
// The library's `probe_first`: as many candidates per instance as keep the round's rollouts within one filling of the
// chip (probe_budget of them), between 2 and probe_max.  A short list is a few deep searches — the instances
// that back-track at all mostly go on for tens of steps (the n = 16 intersection: ~10 % of the batch, mean depth ~30) —
// and 32 at once ends them in a round or two (measured, B = 1024: 280 k -> 335 k it/s); a long list (config 4: ~40 % of
// 4096 instances, most done within a step or two) pays for every candidate it does not need (226 k it/s at 2, 193 k at
// 32).  Round 4, with two rollouts per wavefront and the gradient-only row pass: a budget of 8192 rollouts (config 5 /
// n = 16 constrained / config 4: 249 k / 483 k / 248 k it/s; 4096: 240 / 469 / 252; 16384: 261 / 483 / 236; 4096
// growing fourfold per round: 245 / 457 / 251).
inline int probe_candidates(const SolveSchedule& s, int pool_entries, int round_instances, int probe_first, int tail_rounds) {
  int probe_k = pool_entries / round_instances;
  if (probe_k > s.probe_max) probe_k = s.probe_max;
  int first = probe_first;
  if (first <= 0) {
    first = s.probe_budget / round_instances;
    first = first < 2 ? 2 : (first > s.probe_max ? s.probe_max : first);
  }
  long long ramp = (long long)first << (tail_rounds < 8 ? tail_rounds : 8);
  if (ramp < 2) ramp = 2;
  return probe_k > ramp ? int(ramp) : probe_k;
}

// The specialised driver's choices on top of probe_candidates, measured on the MI355X and kept as
// constants rather than scaled by the device's CU count:
// - deep tails probe whole lane wavefronts up to this many per round, where they fill the chip;
constexpr int kDeepTailWaves = 2400;
// - the cost of a probing round per time step, max(one wave's chain, waves / SIMDs x a wave's issue time), in cycles as
//   measured on the n = 15 scene: the paired form (two candidates per wave) and the lane form (64 / N candidates per
//   wave, thirteen trigonometric evaluations in sequence, ~1180 instructions).
constexpr double kPairChainCycles = 1500.0, kPairIssueCycles = 550.0;
constexpr double kLaneChainCycles = 3500.0, kLaneIssueCycles = 1530.0;

// Candidates per listed instance of this round.  *deep_tails: the solve's deep-search state, carried from round to round.
// Deep searches: once a tail of this solve has kept half of its list through three rounds (2 + 4 + 8 or more
// rejected candidates each: they are mostly on their way through all max_backtracking_steps), later tails skip the
// ramp.  A probing round costs one wave's chain per time step until its waves fill the chip, so every candidate up
// to that point is free: with the lane form (rollout_lanes: 64 / N candidates per wavefront) that is
// C floor(kDeepTailWaves / instances) candidates per instance — whole wavefronts —, as far as the pool holds them.
// (config 5's scene: rounds of 4, 10, 20, 21, 42 ... candidates -> 16 - 63 from a tail's first round on;
// config 4's ~1600 back-tracking instances are mostly done after a step or two: they keep the ramp.)
inline int round_probe_candidates(const SolveSchedule& s, const ilqg_solve_options& opt, int pool_entries, int instances,
                                  int tail_rounds, int tail_first_instances, bool* deep_tails) {
  int probe_k = probe_candidates(s, pool_entries, instances, opt.probe_first, tail_rounds);
  if (s.deep_tails && tail_rounds == 3 && 2 * instances >= tail_first_instances) *deep_tails = true;
  if (!*deep_tails || opt.probe_first > 0) return probe_k;
  int k_deep = std::min(pool_entries / instances, s.probe_max);  // what the pool holds
  if (s.pairs && opt.probe_lanes != ILQG_CHOICE_OFF) {
    const int C = s.lane_width, free_waves = kDeepTailWaves / instances;
    k_deep = std::min(k_deep, C * (free_waves > 1 ? free_waves : 1));
    if (k_deep >= C) k_deep = k_deep / C * C;
  }
  return std::max(probe_k, k_deep);
}

// Rollout launches of a probing round in the y direction of the paired forms
inline int probe_pair_rows(const SolveSchedule& s, int probe_k) { return s.pairs ? (probe_k + 1) / 2 : probe_k; }

// Which kernel integrates a probing round's candidates.
// PROBE_FAT: the register-rich build while every rollout of the round is resident at once at two waves per SIMD.
// PROBE_LANES: a lane per (candidate, subsystem) where that is the shorter round.  A round of W waves takes about
// max(one wave's chain, W / SIMDs x a wave's issue time) per time step (the k*Cycles model).  So the lane
// form wins once its own waves fill the chip (config 5's scene from 16 candidates per instance on), and loses a
// round of a few deep searches (n = 16: ~100 instances x 128 candidates are 700 lane waves, one chain long).
// (n > 16: the lane form's step carries a 2 n-term control product per lane and, for the six-state cars, spills
// inside the time loop — n = 24 on the feedback sweep: 2.2 ms per launch against 0.4-0.6 for the paired form,
// 99 k -> 83 k it/s; the model's constants are the n = 15 scene's, so AUTO leaves those shapes on pairs.)
// PROBE_SINGLE: a candidate per wavefront while every one of them finds a SIMD of its own.
inline ProbeForm probe_form(const SolveSchedule& s, const ilqg_solve_options& opt, int instances, int probe_k) {
  const int C = s.lane_width, proll_y = probe_pair_rows(s, probe_k);
  const int lanes_min = opt.probe_lanes == ILQG_CHOICE_OFF ? (1 << 30) : (opt.probe_lanes == ILQG_CHOICE_ON ? 2 : 8);
  const double simds = 4.0 * s.num_cus;
  const double w_pair = double(instances) * proll_y, w_lane = double(instances) * ((probe_k + C - 1) / C);
  const double t_pair = std::max(kPairChainCycles, w_pair / simds * kPairIssueCycles),
               t_lane = std::max(kLaneChainCycles, w_lane / simds * kLaneIssueCycles);
  if (s.proll_lanes && probe_k >= lanes_min && (opt.probe_lanes == ILQG_CHOICE_ON || (s.lanes_auto && t_lane < 0.9 * t_pair)))
    return PROBE_LANES;
  if (s.proll_single && (long long)instances * probe_k <= 4ll * s.num_cus && opt.probe_lanes != ILQG_CHOICE_ON) return PROBE_SINGLE;
  return (long long)instances * proll_y <= 8ll * s.num_cus ? PROBE_FAT : PROBE_PAIRS;
}

}  // namespace ilqg

#if defined(__HIPCC__) && !defined(ILQG_PART_NX)
// ---------------------------------------------------------------------------------------------------------------
// decide_schedule (the main unit; after ilqg_solve.hpp and the sweeps' headers, whose host-side size functions it calls)
// ---------------------------------------------------------------------------------------------------------------
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
#endif

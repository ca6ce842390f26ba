// ilqg_schedule.hpp — how a solve runs, decided once in plain host code.
// decide_schedule turns a problem's scalars, the solve options, the batch and the device's CU count into a SolveSchedule:
// every AUTO decision as a named field.  DimsLaunch::solve (ilqg_launch.hpp) binds kernels from it (bind_plan) and
// run_rounds (ilqg_round_loop.hpp) launches them, asking the per-round functions below what a probing round looks like; the host-only
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
// ilqg_launch.hpp); kept beside the launch pointers in ShapeEntry.
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
// Defined once, in the library's main unit (ilqg_decide_schedule.hpp); every other unit sees this declaration only.
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

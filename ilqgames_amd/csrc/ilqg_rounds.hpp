// ilqg_rounds.hpp — the round protocol both solve drivers share (DimsLaunch::solve on the specialised kernels,
// generic_solve on the run-time-dimensioned ones), as every unit of the library sees it.  Each driver fills a RoundPlan
// and run_rounds launches it; what differs between the two is a value of the plan, never a question of who is calling.
// The loop itself, its clocks and the kernels it launches by itself are compiled once, in the main unit
// (ilqg_round_loop.hpp): the per-shape units see the declarations below.
#pragma once

#include <algorithm>

#include "ilqg_problem.hpp"   // the handle
#include "ilqg_schedule.hpp"  // SolveSchedule
#include "ilqg_shared.hpp"
#include "ilqg_solve.hpp"     // SolveArgs, ws_layout_of, ProbeEntry

namespace ilqg_shared __attribute__((visibility("hidden"))) {
using namespace ilqg;

// What follows the per-instance blocks in a solve's workspace: two lists of instance ids (this round's back-tracking
// instances, the next round's) and the pool of the speculative line search.
struct WsTail {
  size_t ids_off, pool_off, total;
  int pool_entries;
};
inline WsTail ws_tail(const DevProblem& d, int batch, size_t elem, int ol_row) {
  auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
  const WsLayout L = ws_layout_of(d, ol_row, 1);  // the augmented-Lagrangian layout, the larger one: for either al_mode
  WsTail t;
  t.ids_off = up(size_t(L.total) * elem * size_t(batch));
  t.pool_off = up(t.ids_off + size_t(2) * batch * sizeof(int));
  // sixteen candidates per instance up to kProbeEntries; a small batch gets every candidate of every instance up to
  // one round's budget (a few dozen instances in failing line searches walk through all their step sizes, 128 a round
  // each: config 5's 47 surviving plans as a dense batch, 752 entries: 75 ms per replan; 6016: see DESIGN.md 3.13),
  // and never fewer than two full rounds' worth for a single instance
  const long long small = std::min<long long>((long long)batch * kProbeCandidates, kProbeRoundBudget);
  const long long want = std::max<long long>((long long)batch * 16, small);
  t.pool_entries = int(std::min<long long>(want, kProbeEntries));
  if (t.pool_entries < 2 * kProbeCandidates) t.pool_entries = 2 * kProbeCandidates;
  t.total = up(t.pool_off + size_t(t.pool_entries) * ProbeEntry(d.n, d.m, d.N, d.T).total * elem);
  return t;
}

// What follows the per-instance blocks of a solve's workspace (ws_tail), as pointers.
template <typename T>
struct SolveTail {
  int* pass_ids;    // [2][batch]: this round's back-tracking instances, the next round's
  T* probe_pool;    // the speculative line search's candidates
  int pool_entries;
};

// The SolveArgs fields every solve fills alike; the schedule's own ones (prof, rows_cw, compact, ...) are the driver's.
template <typename T>
SolveArgs<T> solve_args_of(const ilqg_problem* p, int32_t batch, const void* x0, void* xs, void* us, void* P,
                           void* alpha, void* total_costs, int32_t* iters, int32_t* status, int32_t* converged,
                           void* workspace, const ilqg_solve_options& opt, SolveTail<T>* tail) {
  const DevProblem& d = p->dev;
  SolveArgs<T> sa{};
  sa.ol_row = p->desc.params.open_loop ? ol_row_elems(d.n, d.m, d.N) : 0;
  sa.al_mode = opt.augmented_lagrangian ? 1 : 0;
  sa.x0 = (const T*)x0; sa.xs = (T*)xs; sa.us = (T*)us; sa.P = (T*)P; sa.alpha = (T*)alpha;
  sa.total_costs = (T*)total_costs; sa.iters = iters; sa.status = status; sa.converged = converged;
  sa.ws = (T*)workspace;
  sa.ws_stride = ws_layout_of(d, sa.ol_row, sa.al_mode).total;
  sa.fixed_iters = opt.fixed_iters;
  sa.batch = batch;
  sa.prm = p->desc.params;
  sa.active = opt.active;
  sa.forced_steps = (const T*)opt.forced_steps;
  sa.unfinished = p->d_unfinished.get();
  sa.first = opt.resume ? 2 : 1;
  const WsTail t = ws_tail(d, batch, sizeof(T), sa.ol_row);
  tail->pass_ids = reinterpret_cast<int*>(static_cast<char*>(workspace) + t.ids_off);
  tail->probe_pool = reinterpret_cast<T*>(static_cast<char*>(workspace) + t.pool_off);
  tail->pool_entries = t.pool_entries;
  return sa;
}

// One kernel of a round as a driver chose it; the grid is the round's.
template <typename T>
struct KernelLaunch {
  void (*kernel)(DevProblem, SolveArgs<T>) = nullptr;  // null: the solve has no such launch
  int threads = 64;
  size_t lds = 0;
};

// The sweep of a run-time-dimensioned solve on the padded kernels of an instantiated shape (DimsLaunch::lq_padded).
using PaddedSweep = ilqg_status (*)(const DevProblem&, const void*, const PairTable&, void*, size_t*, bool, hipStream_t);

// What a solve launches and how its rounds go, as its driver chose them: run_rounds reads nothing else about the
// schedule.  The split-pass launches (roll to prows) exist where `lists` holds.
template <typename T>
struct RoundPlan {
  KernelLaunch<T> trial;                // the fused pass
  KernelLaunch<T> roll, rows, decide;   // the split pass
  KernelLaunch<T> proll, proll_fat, proll_single, proll_lanes, prows;  // probing rollouts (null: no such form), their rows
  KernelLaunch<T> sweep, exit;          // (the sweep: unless `padded` runs it)
  PaddedSweep padded = nullptr;
  const PairTable* pad_pairs = nullptr; void* pad = nullptr;  // the padded sweep's control blocks and scratch
  SolveSchedule s{};                    // the rounds' flags, cap, row_chunks, lane_width, num_cus (ilqg_schedule.hpp)
  bool exit_fill_first = false;  // clear the round counters in front of the exit launch where they are not clean
};

// The rounds of a solve, on either driver's plan (ilqg_round_loop.hpp); instantiated for float and double in the main unit.
template <typename T>
ilqg_status run_rounds(ilqg_problem* p, SolveArgs<T>& sa, const SolveTail<T>& tail, const RoundPlan<T>& plan,
                       const ilqg_solve_options& opt, hipStream_t stream);

// The round counters' way back to the host: p->h_unfinished holds them when this returns.
ilqg_status read_round_counters(ilqg_problem* p, hipStream_t stream);

// How many instances of a masked batch take part (ilqg_solve_options::active): into *count, through the round counters.
ilqg_status count_active_instances(ilqg_problem* p, const int* active, int batch, hipStream_t stream, int* count);

}  // namespace ilqg_shared

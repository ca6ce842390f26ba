// ilqg_round_loop.hpp — the rounds of a solve (run_rounds), the round counters' read-back, the two clocks of a timed
// solve and the kernels the loop launches by itself.  Included by the main unit alone (ilqg_api.hip), which instantiates
// run_rounds for both precisions: what the other units see of it is ilqg_rounds.hpp.
#pragma once

#include <chrono>
#include <string>

#include "ilqg_kernels.hpp"  // ilq_probe_pick_kernel, ilq_log_kernel, ilq_deadline_kernel
#include "ilqg_rounds.hpp"

// The round counters' way back to the host.  A counted solve reads them once per round (twice with the augmented
// Lagrangian's restarts), and while it does the device idles: what a read-back costs is the gap between two rounds.
// A copy command plus a stream synchronisation is ~20 us of that; instead a one-wave kernel behind the round's last
// launch stores the four counters and then a sequence number into host memory (pinned, coherent, mapped), and the
// host spins on the sequence number; a device fault shows up in the periodic hipStreamQuery.  Where the pinned mirror
// has no device address (hipHostGetDevicePointer failed) the counters come back by the copy + synchronise form.
namespace {
using namespace ilqg;
using namespace ilqg_shared;

__global__ void ilq_publish_kernel(int* counts, int* host, int seq) {
  const int t = threadIdx.x;
  if (t < 4) {
    __hip_atomic_store(host + t, counts[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    counts[t] = 0;  // ... and the next round finds them cleared (ilqg_problem::counters_clean): one fill command less
  }
  __threadfence_system();
  if (t == 0) __hip_atomic_store(host + 8, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// How many instances of a masked batch take part (ilqg_solve_options::active): into the fourth round counter.
__global__ void ilq_count_active_kernel(const int* active, int batch, int* counts) {
  int mine = 0;
  for (int b = threadIdx.x; b < batch; b += blockDim.x) mine += active[b] != 0;
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counts + 3, mine);
}

}  // namespace

// The outer loop's clock of AugmentedLagrangianSolver::Solve under a max_runtime (src/augmented_lagrangian_solver.cpp:
// 104-110,193): `elapsed` starts at the first inner solve's ALLOWANCE (max_runtime / max_solver_iters, not the time it
// took), every outer iteration adds its wall time, and another one starts only while
// elapsed < max_runtime - timer_.RuntimeUpperBound().  A batch shares the clock.  It runs without a gap from the first
// exit launch that restarted an instance until the solve returns — whoever is restarted or not at the launches in
// between (round 5 re-armed it only when a launch restarted somebody: with staggered instances whole inner solves went
// uncounted).  The LoopTimer's samples are outer-iteration durations: every restart-bearing exit launch opens an
// interval, and each later exit launch (one exists only when some inner solve has ended) closes the oldest open one —
// exact for a batch in lockstep, the inner-solve length of the earliest group when instances are staggered; never the
// gap between two neighbouring rounds.  before_exit() is called in front of every exit launch and says whether instances
// whose inner solve has ended may still restart.
struct AlOuterClock {
  ilqg_problem* p;
  bool on;
  double max_runtime, elapsed, last = 0.0;
  bool running = false;
  static constexpr int kOpen = 32;
  double open_since[kOpen];
  int open_head = 0, open_count = 0;
  AlOuterClock(ilqg_problem* p_, bool on_, double max_runtime_, double first_allowance)
      : p(p_), on(on_), max_runtime(max_runtime_), elapsed(first_allowance) {}
  static double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  bool before_exit() {  // true: the outer loop is closed
    if (!on) return false;
    const double now = wall();
    if (running) {
      elapsed += now - last;
      last = now;
      if (open_count > 0) {
        p->al_loop_timer.add(now - open_since[open_head]);
        open_head = (open_head + 1) % kOpen;
        open_count--;
      }
    }
    return !(elapsed < max_runtime - p->al_loop_timer.upper_bound());
  }
  void after_exit(int restarted) {
    if (!on || !restarted) return;
    const double now = wall();
    if (!running) {
      running = true;
      last = now;
    }
    if (open_count < kOpen) {
      open_since[(open_head + open_count) % kOpen] = now;
      open_count++;
    }
  }
};

namespace {

// The anytime exit of one inner solve (ilqg_solve_options::max_runtime): the loop condition of src/ilq_solver.cpp:
// 123-124, read where the batch is about to start an iteration, so timed solves do not batch rounds into bursts.  The
// augmented-Lagrangian solver gives each inner solve of a constrained problem max_runtime / max_solver_iters
// (src/augmented_lagrangian_solver.cpp:85-88), which is also where its AlOuterClock starts.
struct InnerClock {
  ilqg_problem* p;
  bool on;
  double budget, elapsed = 0.0, tic = 0.0;
  bool iteration_open = false;
  InnerClock(ilqg_problem* p_, bool on_, double max_runtime, bool al_constrained)
      : p(p_), on(on_),
        budget(!on_ ? 0.0 : al_constrained ? max_runtime / double(p_->desc.params.max_solver_iters) : max_runtime) {}
  bool deadline_passed() {  // in front of an iteration: the one in flight ends here; true: the next may not start
    const double now = AlOuterClock::wall();
    if (iteration_open) {
      p->loop_timer.add(now - tic);
      elapsed += now - tic;
      iteration_open = false;
    }
    return !(elapsed < budget - p->loop_timer.upper_bound());
  }
  void open_iteration() {
    if (!on) return;
    tic = AlOuterClock::wall();
    iteration_open = true;
  }
  void restart() { elapsed = 0.0; }  // an augmented-Lagrangian restart: the next inner solve's own budget
};

ilqg_status iteration_bound(long long round, long long cap) {
  return round > cap ? fail(ILQG_ERR_HIP, "solve did not terminate within its iteration bound") : ILQG_OK;
}

// The iterate log (ilqg_solve_options::iterate_log): checked and its counts cleared where the solve begins ...
template <typename T>
ilqg_status iterate_log_open(const ilqg_solve_options& opt, int32_t batch, hipStream_t stream, IterLog<T>* lg) {
  *lg = IterLog<T>{};
  if (!opt.iterate_log) return ILQG_OK;
  const ilqg_iterate_log& il = *opt.iterate_log;
  if (!il.xs || !il.us || !il.costs || !il.count || il.capacity < 1)
    return fail(ILQG_ERR_INVALID, "iterate log: xs, us, costs, count and a capacity of at least one are required");
  *lg = IterLog<T>{(T*)il.xs, (T*)il.us, (T*)il.costs, (T*)il.P, (T*)il.alpha, il.count, il.capacity};
  HIP_TRY(hipMemsetAsync(il.count, 0, sizeof(int) * size_t(batch), stream));
  return ILQG_OK;
}

// ... and copied in front of every exit / sweep launch
template <typename T>
ilqg_status iterate_log_launch(const ilqg_problem* p, const SolveArgs<T>& sa, const IterLog<T>& lg, hipStream_t stream) {
  if (!lg.count) return ILQG_OK;
  return launch(ilq_log_kernel<T>, dim3(sa.batch), dim3(256), 0, stream, p->dev, sa, lg);
}

// Split passes: the decision kernel lists the instances that want another pass (the initial quadraticisation,
// back-tracking), and the next round covers those only — a tail of rounds that lasts until the last of them has made up
// its mind.  The sweeps and exits the batch asks for wait until then: the sweep is launched once per iteration, which
// keeps the batch in step (a sweep launch with a handful of instances costs a full sweep's latency).
template <typename T>
struct RoundLists {
  SolveArgs<T>& sa;             // sa.ids: the instances of this round (null: the whole batch)
  int* const pass_ids;          // the two lists (SolveTail)
  const long long cap;          // the driver's iteration bound in rounds
  int round_instances;          // how many instances this round covers
  int list = 0;                 // which list is free for the round to write
  int tail_rounds = 0;          // rounds since the whole batch was last in one
  int tail_first_instances = 0;  // instances in the current tail's first round
  bool probed_in_tail = false;  // the current tail has launched a probing pass
  int waiting_lq = 0, waiting_exit = 0;  // instances already through this iteration's line search
  RoundLists(SolveArgs<T>& sa_, int* pass_ids_, long long cap_)
      : sa(sa_), pass_ids(pass_ids_), cap(cap_), round_instances(sa_.batch) {}
  int* free_list() const { return pass_ids + size_t(list) * sa.batch; }
  // a round over listed instances that probes probe_k step sizes of each (fewer than two: no probing launch)
  ilqg_status tail_round(bool probe, int probe_k) {
    tail_rounds++;
    if (!probe) return ILQG_OK;
    // an instance every candidate of which was rejected waits in ST_PROBE and is skipped by the regular pass: it is
    // only picked up again by the next probing launch, so a tail that has probed must keep probing (the list only
    // shrinks and the ramp only grows, so this cannot trigger; if it ever does, fail instead of dropping instances)
    if (probed_in_tail && probe_k < 2) return fail(ILQG_ERR_HIP, "a probing line-search tail lost its probe launch");
    if (probe_k >= 2) probed_in_tail = true;
    return ILQG_OK;
  }
  // The round's counters are back.  *again: the instances it listed go round again, by themselves; otherwise the batch
  // is whole again and *want_lq / *want_exit are what its iteration asks for.
  ilqg_status after_round(const int* counters, long long round, bool* again, int* want_lq, int* want_exit) {
    waiting_lq += counters[0];
    waiting_exit += counters[1];
    *again = counters[3] != 0;
    if (*again) {
      const ilqg_status s = iteration_bound(round, cap);
      if (s != ILQG_OK) return s;
      if (!sa.ids) tail_first_instances = counters[3];
      sa.ids = sa.ids_next;
      round_instances = counters[3];
      list ^= 1;
      return ILQG_OK;
    }
    sa.ids = nullptr;
    round_instances = sa.batch;
    tail_rounds = 0;
    probed_in_tail = false;
    *want_lq = waiting_lq;
    *want_exit = waiting_exit;
    waiting_lq = waiting_exit = 0;
    return ILQG_OK;
  }
};

// LDS limits of every launch of a plan (raise_lds_limit; the padded sweep raises its own)
template <typename T>
void raise_lds_limits(const RoundPlan<T>& pl) {
  for (const KernelLaunch<T>* k : {&pl.trial, &pl.roll, &pl.rows, &pl.decide, &pl.proll, &pl.proll_fat, &pl.proll_single,
                                   &pl.proll_lanes, &pl.prows, &pl.sweep, &pl.exit})
    if (k->kernel) raise_lds_limit((const void*)k->kernel, k->lds);
}

}  // namespace

namespace ilqg_shared __attribute__((visibility("hidden"))) {

ilqg_status read_round_counters(ilqg_problem* p, hipStream_t stream) {
  p->counters_clean = false;
  if (!p->h_unfinished_dev) {
    HIP_TRY(hipMemcpyAsync(p->h_unfinished.get(), p->d_unfinished.get(), 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ILQG_OK;
  }
  const int seq = ++p->publish_seq;
  if (launch(ilq_publish_kernel, dim3(1), dim3(64), 0, stream, p->d_unfinished.get(), p->h_unfinished_dev, seq) != ILQG_OK) return ILQG_ERR_HIP;
  p->counters_clean = true;
  volatile int* const flag = p->h_unfinished.get() + 8;
  for (long long spins = 0;; spins++) {
    if (__atomic_load_n(const_cast<int*>(flag), __ATOMIC_ACQUIRE) == seq) return ILQG_OK;
    __builtin_ia32_pause();
    if ((spins & 0xffff) == 0xffff) {  // every ~65 k polls: has the stream died, or drained without our store?
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) {
        if (__atomic_load_n(const_cast<int*>(flag), __ATOMIC_ACQUIRE) == seq) return ILQG_OK;
        return fail(ILQG_ERR_HIP, "the round counters never reached the host");
      }
      if (q != hipErrorNotReady) return fail(ILQG_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
    }
  }
}

ilqg_status count_active_instances(ilqg_problem* p, const int* active, int batch, hipStream_t stream, int* count) {
  HIP_TRY(hipMemsetAsync(p->d_unfinished.get(), 0, 4 * sizeof(int), stream));  // (whatever an earlier solve left there)
  if (launch(ilq_count_active_kernel, dim3(1), dim3(256), 0, stream, active, batch, p->d_unfinished.get()) != ILQG_OK) return ILQG_ERR_HIP;
  if (read_round_counters(p, stream) != ILQG_OK) return ILQG_ERR_HIP;
  *count = p->h_unfinished[3];
  return ILQG_OK;
}

// The rounds of a solve, on either driver's plan.  One round = a pass (the fused trial kernel, or the split kernels over
// the whole batch or over the listed back-tracking instances with their probing launches), then, for the instances
// that asked, the exit kernel and the sweep.  The kernels count what their instances wait for; with fixed_iters = K
// (no AL) and no counting the sequence is known — trial, K x (sweep, trial), exit — otherwise the host reads the counts
// back each round, which makes a free-running solve synchronous with respect to `stream`.
template <typename T>
ilqg_status run_rounds(ilqg_problem* p, SolveArgs<T>& sa, const SolveTail<T>& tail, const RoundPlan<T>& plan,
                       const ilqg_solve_options& opt, hipStream_t stream) {
  const DevProblem& d = p->dev;
  const int batch = sa.batch;
  const SolveSchedule& sc = plan.s;
  raise_lds_limits(plan);
  IterLog<T> lg;
  ilqg_status s = iterate_log_open(opt, batch, stream, &lg);
  if (s != ILQG_OK) return s;
  const bool al_constrained = sa.al_mode && d.num_constraints > 0;
  InnerClock clock(p, sc.timed, opt.max_runtime, al_constrained);
  AlOuterClock outer(p, sc.timed && al_constrained, opt.max_runtime, clock.budget);
  p->counters_clean = false;  // whatever an earlier solve left in the round counters
  RoundLists<T> rl(sa, tail.pass_ids, sc.cap);
  auto launch = [&](const KernelLaunch<T>& k, dim3 grid) { return ilqg_shared::launch(k.kernel, grid, dim3(k.threads), k.lds, stream, d, sa); };
  auto sweep = [&]() -> ilqg_status {
    const ilqg_status s = plan.padded ? plan.padded(d, &sa, *plan.pad_pairs, plan.pad, nullptr, p->desc.params.open_loop != 0, stream)
                                      : launch(plan.sweep, dim3(batch));
    if (s == ILQG_OK && sa.clear_counters) p->counters_clean = true;  // (SolveArgs::clear_counters)
    return s;
  };
  bool deep_tails = false;  // a tail of this solve kept half of its list through three rounds (round_probe_candidates)
  // the listed instances' next step sizes side by side; their states move to the first acceptable one
  auto probe_round = [&](int instances, int probe_k) -> ilqg_status {
    sa.probe_pool = tail.probe_pool;
    sa.probe_k = probe_k;
    const int C = sc.lane_width, proll_y = probe_pair_rows(sc, probe_k);
    const ProbeForm form = probe_form(sc, opt, instances, probe_k);
    const ilqg_status s = form == PROBE_LANES    ? launch(plan.proll_lanes, dim3(instances, (probe_k + C - 1) / C))
                          : form == PROBE_SINGLE ? launch(plan.proll_single, dim3(instances, probe_k))
                                                 : launch(form == PROBE_FAT ? plan.proll_fat : plan.proll, dim3(instances, proll_y));
    if (s != ILQG_OK || launch(plan.prows, dim3(sc.row_chunks, instances * probe_k)) != ILQG_OK) return ILQG_ERR_HIP;
    return launch(KernelLaunch<T>{ilq_probe_pick_kernel<T>, kProbeCandidates, 0}, dim3(instances));
  };
  auto pass = [&]() -> ilqg_status {
    if (sc.counted && !p->counters_clean) HIP_TRY(hipMemsetAsync(p->d_unfinished.get(), 0, 4 * sizeof(int), stream));
    p->counters_clean = false;  // (the round's kernels count into them)
    if (!sc.split && !sa.ids) {
      sa.ids_next = sc.handoff ? rl.free_list() : nullptr;
      const ilqg_status s = launch(plan.trial, dim3(batch));
      sa.first = 0;
      return s;
    }
    sa.ids_next = rl.free_list();
    const int instances = rl.round_instances;
    if (sa.ids) {
      const int probe_k = round_probe_candidates(sc, opt, tail.pool_entries, instances, rl.tail_rounds, rl.tail_first_instances, &deep_tails);
      ilqg_status s = rl.tail_round(sc.probe, probe_k);
      if (s == ILQG_OK && sc.probe && probe_k >= 2) s = probe_round(instances, probe_k);
      if (s != ILQG_OK) return s;
    }
    sa.round_count = instances;
    if (launch(plan.roll, dim3(sc.pairs ? (instances + 1) / 2 : instances)) != ILQG_OK) return ILQG_ERR_HIP;
    sa.first = 0;
    if (launch(plan.rows, dim3(sc.row_chunks, instances)) != ILQG_OK) return ILQG_ERR_HIP;
    return launch(plan.decide, dim3(instances));
  };
  // Free-running solves: the kernels select their instances by the stage each one is in, so a round launched for
  // nobody is harmless — the host therefore enqueues BURSTS of whole rounds (trial, exit, sweep) and reads the
  // counters back once per burst instead of once per round (a read-back is a stream synchronisation: ~20-30 us against
  // a ~0.45 ms round of a single instance).  The burst doubles up to eight rounds while no instance is back-tracking
  // and falls back to one as soon as one is (those go through the probing passes, which need the lists every round).
  const bool fixed = opt.fixed_iters > 0 && !sa.al_mode;
  int burst = 1;
  bool exit_pending = false;  // a burst round went without its exit launch (see the burst loop)
  for (long long round = 0;; round++) {
    if (sc.bursts && !sa.ids) {
      // a fixed-iteration solve knows its last round: no burst runs past it
      const long long left = fixed ? (long long)opt.fixed_iters - round : (long long)burst;
      for (int q = 1; q < burst && q <= left; q++) {  // rounds without a read-back
        s = pass();
        if (s != ILQG_OK) return s;
        if (iterate_log_launch(p, sa, lg, stream) != ILQG_OK) return ILQG_ERR_HIP;
        // The exit path inside a burst only where it starts something (the augmented Lagrangian's next inner solve);
        // an ILQSolver::Solve that ends here waits for the burst's last round, whose exit launch is then unconditional
        // (a launch for nobody is ~5 us of every round of a lone instance).
        if (sa.al_mode) {
          if (launch(plan.exit, dim3(batch)) != ILQG_OK) return ILQG_ERR_HIP;
        } else {
          exit_pending = true;
        }
        s = sweep();
        if (s != ILQG_OK) return s;
        round++;
      }
    }
    s = pass();
    if (s != ILQG_OK) return s;
    int want_lq = 1, want_exit = 0;
    if (sc.counted) {
      if (read_round_counters(p, stream) != ILQG_OK) return ILQG_ERR_HIP;
      want_lq = p->h_unfinished[0];
      want_exit = p->h_unfinished[1];
      if (sc.lists) {
        bool again = false;
        s = rl.after_round(p->h_unfinished.get(), round, &again, &want_lq, &want_exit);
        if (s != ILQG_OK) return s;
        if (again) {
          burst = 1;
          continue;
        }
      }
      if (sc.bursts) burst = p->h_unfinished[3] ? 1 : (burst < 8 ? burst * 2 : 8);
    } else if (round == opt.fixed_iters) {
      want_lq = 0;
      want_exit = 1;
    }
    if (exit_pending) {  // instances that ended in a burst round without an exit launch
      want_exit = 1;
      exit_pending = false;
    }
    // The end of an iteration of the batch: want_lq instances wait for a sweep and want_exit for the exit path.  The
    // anytime exit's deadline (which turns the sweep into an exit), the iterate log, the exit launch and the restarts it
    // made, the sweep.
    if (clock.on && want_lq && clock.deadline_passed()) {
      if (launch(KernelLaunch<T>{ilq_deadline_kernel<T>, 64, 0}, dim3(batch)) != ILQG_OK) return ILQG_ERR_HIP;
      want_exit = 1;
      want_lq = 0;
    }
    if ((want_exit || want_lq) && iterate_log_launch(p, sa, lg, stream) != ILQG_OK) return ILQG_ERR_HIP;
    int restarted = 0;
    if (want_exit) {
      if (plan.exit_fill_first && !p->counters_clean) HIP_TRY(hipMemsetAsync(p->d_unfinished.get(), 0, 4 * sizeof(int), stream));
      if (outer.before_exit()) sa.outer_closed = 1;  // out of time: inner solves that end now are the last ones
      if (launch(plan.exit, dim3(batch)) != ILQG_OK) return ILQG_ERR_HIP;
      p->counters_clean = false;
      if (sc.read_restarts) {
        if (read_round_counters(p, stream) != ILQG_OK) return ILQG_ERR_HIP;
        restarted = p->h_unfinished[2];
        if (restarted) clock.restart();
        outer.after_exit(restarted);
      }
    }
    if (want_lq) {
      clock.open_iteration();
      s = sweep();
      if (s != ILQG_OK) return s;
    }
    if (!want_lq && !restarted) return ILQG_OK;  // the solve has ended
    if (iteration_bound(round, sc.cap) != ILQG_OK) return ILQG_ERR_HIP;
  }
}

}  // namespace ilqg_shared

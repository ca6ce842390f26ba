// ilqg_kernels.hpp — the __global__ entry points of libilqg_hip.so and their argument structs: one workgroup (or one
// wavefront) per game instance, each a thin shell around the device code of the header named beside it.  Templates only:
// a translation unit emits the kernels it launches, so the per-shape units (ilqg_dims.hip) hold the kernels of their
// (n, N, m_i) and the main unit (ilqg_api.hip) the ones that depend on the precision alone.  The kernels keep the
// anonymous namespace: their names are what profiles/, DESIGN.md and scripts/summarize_profile.py know them by.
#pragma once

#include <type_traits>

#include "ilqg_lq.hpp"
#include "ilqg_lq_generic.hpp"
#include "ilqg_lq_openloop.hpp"
#include "ilqg_rows.hpp"
#include "ilqg_solve.hpp"
#include "ilqg_stages.hpp"

namespace {
using namespace ilqg;

// ------------------------------------------------------------------------------------
// Kernels — one workgroup per game instance
// ------------------------------------------------------------------------------------
template <typename T>
struct LQBatchArgs {
  const T *A, *Bm, *Q, *l, *R, *r, *x0;
  T *P, *alpha, *dx, *scratch;
  int T_steps, adaptive, batch, force_valu;
  T* costates = nullptr;
  // the arrays of an ilqg_lq_*_batch call; no scratch, no costates, the caller's regularisation
  LQBatchArgs(const ilqg_dims* d, const void* A_, const void* Bm_, const void* Q_, const void* l_, const void* R_,
              const void* r_, const void* x0_, void* P_, void* alpha_, void* dx_)
      : A((const T*)A_), Bm((const T*)Bm_), Q((const T*)Q_), l((const T*)l_), R((const T*)R_), r((const T*)r_),
        x0((const T*)x0_), P((T*)P_), alpha((T*)alpha_), dx((T*)dx_), scratch(nullptr), T_steps(d->T),
        adaptive(d->adaptive_regularization), batch(d->batch), force_valu(0) {}
};

template <typename T, int NX, int NP, int MU, bool FORCE_VALU>
__global__ void __launch_bounds__((LQFeedbackThreads<T, NX, NP, MU, FORCE_VALU>::NT),
                                  (LQFeedbackThreads<T, NX, NP, MU, FORCE_VALU>::PLAYER_WAVES ? (NX <= 16 ? NP : 2) : 1))
lq_feedback_kernel(LQBatchArgs<T> g, PairTable pt) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const int b = blockIdx.x;
  constexpr int M = NP * MU;
  const size_t Tn = g.T_steps;
  LQArgs<T> a;
  a.A = g.A + b * Tn * NX * NX;
  a.Bm = g.Bm + b * Tn * NX * M;
  a.Q = g.Q + b * Tn * NP * NX * NX;
  a.l = g.l + b * Tn * NP * NX;
  a.R = g.R + b * Tn * pt.Rsz;
  a.r = g.r + b * Tn * pt.rsz;
  a.x0 = g.x0 ? g.x0 + size_t(b) * NX : nullptr;
  a.P = g.P + b * Tn * M * NX;
  a.alpha = g.alpha + b * Tn * M;
  a.dx = g.dx ? g.dx + b * Tn * NX : nullptr;
  a.scratch = g.scratch ? g.scratch + b * Tn * (NP * (NX + 1) + NX) : nullptr;
  a.ed_out = nullptr;
  a.T_steps = g.T_steps;
  a.adaptive = g.adaptive;
  lq_feedback_dispatch<T, NX, NP, MU, FORCE_VALU>(a, pt, sm);
}

template <typename T, int NX, int NP, int MU>
__global__ void __launch_bounds__((OLCfg<T, NX, NP, MU>::NT), 3)  // three instances per CU (see ilqg_lq_openloop.hpp)
lq_openloop_kernel(LQBatchArgs<T> g, PairTable pt) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const int b = blockIdx.x;
  constexpr int M = NP * MU;
  const size_t Tn = g.T_steps;
  LQArgs<T> a;
  a.A = g.A + b * Tn * NX * NX;
  a.Bm = g.Bm + b * Tn * NX * M;
  a.Q = g.Q + b * Tn * NP * NX * NX;
  a.l = g.l + b * Tn * NP * NX;
  a.R = g.R + b * Tn * pt.Rsz;
  a.r = g.r + b * Tn * pt.rsz;
  a.x0 = g.x0 ? g.x0 + size_t(b) * NX : nullptr;
  a.P = g.P + b * Tn * M * NX;
  a.alpha = g.alpha + b * Tn * M;
  a.dx = g.dx ? g.dx + b * Tn * NX : nullptr;
  a.scratch = g.scratch + b * Tn * (g.costates ? OLCfg<T, NX, NP, MU>::ROW_FAT : OLCfg<T, NX, NP, MU>::ROW);
  a.costates = g.costates ? g.costates + b * Tn * NP * NX : nullptr;
  a.ed_out = nullptr;
  a.T_steps = g.T_steps;
  a.adaptive = 0;
  lq_openloop_instance<T, NX, NP, MU>(a, pt, sm);
}

// The sweeps with run-time dimensions (ilqg_lq_generic.hpp): whatever has no specialised instantiation above.
template <typename T>
__global__ void __launch_bounds__(256) lq_generic_kernel(LQBatchArgs<T> g, GenDims d, PairTable pt, int open_loop,
                                                         int scratch_row) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const size_t b = blockIdx.x, Tn = d.T, n = d.n, m = d.m, N = d.N;
  GenLQArgs<T> a;
  a.A = g.A + b * Tn * n * n;
  a.Bm = g.Bm + b * Tn * n * m;
  a.Q = g.Q + b * Tn * N * n * n;
  a.l = g.l + b * Tn * N * n;
  a.R = g.R + b * Tn * pt.Rsz;
  a.r = g.r + b * Tn * pt.rsz;
  a.x0 = g.x0 ? g.x0 + b * n : nullptr;
  a.P = g.P + b * Tn * m * n;
  a.alpha = g.alpha + b * Tn * m;
  a.dx = g.dx ? g.dx + b * Tn * n : nullptr;
  a.costates = (open_loop && g.costates) ? g.costates + b * Tn * N * n : nullptr;
  a.scratch = g.scratch ? g.scratch + b * Tn * size_t(scratch_row) : nullptr;
  a.ed_out = nullptr;
  a.adaptive = g.adaptive;
  const ParDevice par;
  if (open_loop)
    lq_openloop_generic<T>(d, a, pt, sm, par);
  else
    lq_feedback_generic<T>(d, a, pt, sm, par);
}

template <typename T>
struct RolloutBatchArgs {
  const T *x0, *xs_ref, *us_ref, *P, *alpha, *alpha_scale;
  T *xs, *us;
  const int* active;
};

// XDYN: the problem holds an expression subsystem (rollout_instance's XDYN, ilqg_stages.hpp): a kernel of its own
// (launched with one wavefront; the expression integrator wants the whole register file: 1024 is the bound a kernel
// without the attribute gets)
template <typename T, bool XDYN = false>
__global__ void __launch_bounds__(XDYN ? 64 : 1024) rollout_kernel(DevProblem p, RolloutBatchArgs<T> g) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const size_t b = blockIdx.x;
  if (g.active && !g.active[b]) return;
  const size_t Tn = p.T, n = p.n, m = p.m;
  RolloutArgs<T> a{g.x0 + b * n,          g.xs_ref + b * Tn * n, g.us_ref + b * Tn * m, g.P + b * Tn * m * n,
                   g.alpha + b * Tn * m,  g.alpha_scale ? g.alpha_scale[b] : T(1),
                   g.xs + b * Tn * n,     g.us + b * Tn * m,     instance_values(p, int(b))};
  rollout_instance_rt<T, XDYN>(p, a, sm, threadIdx.x);
}

template <typename T>
struct QuadBatchArgs {
  const T *xs, *us, *lambdas, *mu;
  const int* t_extreme;
  T *A, *Bm, *Q, *l, *R, *r, *merit_part, *cost_part;
  const int* active;
};

template <typename T>
__device__ __forceinline__ QuadArgs<T> quad_args_of(const DevProblem& p, const QuadBatchArgs<T>& g, size_t b) {
  const size_t Tn = p.T, n = p.n, m = p.m, N = p.N;
  QuadArgs<T> a;
  a.xs = g.xs + b * Tn * n;
  a.us = g.us + b * Tn * m;
  a.lambdas = g.lambdas ? g.lambdas + b * p.num_constraints * Tn : nullptr;
  a.mu = g.mu ? g.mu[b] : T(10);
  a.t_extreme = g.t_extreme ? g.t_extreme + b * N : nullptr;
  a.t_init = 0.0;
  a.A = g.A ? g.A + b * Tn * n * n : nullptr;
  a.Bm = g.Bm ? g.Bm + b * Tn * n * m : nullptr;
  a.Q = g.Q ? g.Q + b * Tn * N * n * n : nullptr;
  a.l = g.l ? g.l + b * Tn * N * n : nullptr;
  a.R = g.R ? g.R + b * Tn * p.pairs.Rsz : nullptr;
  a.r = g.r ? g.r + b * Tn * p.pairs.rsz : nullptr;
  a.merit_part = g.merit_part ? g.merit_part + b * Tn * N * 2 : nullptr;
  a.cost_part = g.cost_part ? g.cost_part + b * Tn * N : nullptr;
  a.iv = instance_values(p, int(b));
  a.seg_off = instance_segs_offset(p, int(b));
  a.tnom_off = instance_tnom_offset(p, int(b));
  return a;
}

// Linearise / quadraticise / cost stage on its own (ilqg_rows.hpp): grid = (ceil(T / cw), B), one wavefront takes cw
// consecutive rows of one instance.
// EXPR: the interpreter that also evaluates expression costs (ProgDynamicExpr, ilqg_rows.hpp), for the problems that hold one
// XDYN: ... and linearises expression subsystems (ProgDynamicExprDyn)
template <typename T, int NX, int NP, int MU, bool EXPR = false, bool XDYN = false>
__global__ void __launch_bounds__(64) rows_kernel(DevProblem p, QuadBatchArgs<T> g, int cw) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const size_t b = blockIdx.y;
  if (g.active && !g.active[b]) return;
  const short* maps = rows_maps_load(p, smem_raw);
  T* sm = reinterpret_cast<T*>(smem_raw + rows_maps_bytes(p));
  const QuadArgs<T> a = quad_args_of<T>(p, g, b);
  const int k0 = int(blockIdx.x) * cw;
  const int nrows = p.T - k0 < cw ? p.T - k0 : cw;
  typedef typename std::conditional<XDYN, ProgDynamicExprDyn, typename std::conditional<EXPR, ProgDynamicExpr, ProgDynamic>::type>::type Prog;
  rows_chunk<T, NX, NP * MU, NP, false, false, Prog>(p, maps, a, k0, nrows, cw, sm, int(threadIdx.x));
}

// ilqg_solve_state_batch: the loop state of every instance out of the workspace
template <typename T>
__global__ void solve_state_kernel(const T* ws, size_t ws_stride, size_t state_off, int batch, T* last_merit,
                                   T* expected_decrease, T* step, int* backtracks) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const SolveState<T>* s = reinterpret_cast<const SolveState<T>*>(ws + size_t(b) * ws_stride + state_off);
  if (last_merit) last_merit[b] = s->last_merit;
  if (expected_decrease) expected_decrease[b] = s->expected_decrease;
  if (step) step[b] = s->acc_scale;
  if (backtracks) backtracks[b] = s->rejected;
}

template <typename T>
__global__ void costs_reduce_kernel(DevProblem p, const T* cost_part, T* costs, int* t_extreme, const int* active) {
  const size_t b = blockIdx.x;
  if (active && !active[b]) return;
  costs_reduce<T>(p, cost_part + b * p.T * p.N, costs + b * p.N, t_extreme ? t_extreme + b * p.N : nullptr);
}

// Wavefronts per instance in the trial kernel: wave 0 integrates, the others take the chunks of rows it has
// produced (ilqg_solve.hpp).  One row wave keeps up with the integration; each more costs a row scratch of LDS.
#ifndef ILQG_TRIAL_WAVES_F32
#define ILQG_TRIAL_WAVES_F32 2
#endif
#ifndef ILQG_TRIAL_WAVES_F64
#define ILQG_TRIAL_WAVES_F64 2
#endif
template <typename T>
struct TrialWaves {
  static constexpr int W = sizeof(T) == 4 ? ILQG_TRIAL_WAVES_F32 : ILQG_TRIAL_WAVES_F64;
};

// Trial kernel: rollout + linearise/quadraticise + line-search decision (ilqg_solve.hpp).  The second
// launch-bound argument is the number of waves per SIMD the register allocation must allow.  fp32 was compiled for
// three (168 registers: six instances per CU) until round 5; since the large batches of the one-tile shapes run the
// split pass, the fused kernel serves four instances per CU at most there, and the full register file is worth 1.6 %
// at the headline batch in fp32 (2.105 -> 2.140 M it/s).  -DILQG_TRIAL_OCCUPANCY_F32=3 restores the old build.
#ifndef ILQG_TRIAL_OCCUPANCY_F32
#define ILQG_TRIAL_OCCUPANCY_F32 2
#endif
template <typename T, int NX, int NP, int MU, int W, int PROGID = 0, bool BOUND = (PROGID >= kBoundProg)>
__global__ void __launch_bounds__(64 * W, (sizeof(T) == 4 && W == 2) ? ILQG_TRIAL_OCCUPANCY_F32 : W) ilq_trial_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x;
  if (!sa.first) {  // instances that are done (or waiting for the LQ kernel) leave without touching LDS
    const int stage = instance_stage<T>(p, sa, b);
    if (stage != ST_ROLLOUT && stage != ST_QUAD) return;
  } else if (sa.active && !sa.active[b]) {  // skipped instance
    instance_mark_done<T>(p, sa, b);
    return;
  }
  const short* maps = rows_maps_load(p, smem_raw);
  T* sm = reinterpret_cast<T*>(smem_raw + rows_maps_bytes(p));
  // (its own type: the fused form reads the two arguments again from the argument segment, trial_args_again)
  trial_part_instance<T, NX, NP, MU, W, TRIAL_FUSED, PROGID, BOUND, true, decltype(&ilq_trial_kernel<T, NX, NP, MU, W, PROGID, BOUND>)>(p, maps, sa, b, sm);
}

// The same pass cut into three launches (ilqg_solve.hpp, TRIAL_ROLL / rows_part_instance / TRIAL_DECIDE), for
// problems whose fused trial kernel fits fewer than three instances on a CU.
#ifndef ILQG_ROLL_WAVES
#define ILQG_ROLL_WAVES 4
#endif
// XDYN: the problem holds an expression subsystem (kExprDynProg: the rollout with the expression integrator in it)
template <typename T, int NX, int NP, int MU, bool XDYN = false>
__global__ void __launch_bounds__(64, sizeof(T) == 8 ? (XDYN ? 2 : ILQG_ROLL_WAVES) : 1) ilq_roll_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  if constexpr (rollout_pairs(NX, NP, MU)) {  // two instances per wavefront: entries 2 x and 2 x + 1 of the round
    const int i0 = 2 * int(blockIdx.x), i1 = i0 + 1;
    const int b0 = sa.ids ? sa.ids[i0] : i0;
    const int b1 = i1 < sa.round_count ? (sa.ids ? sa.ids[i1] : i1) : -1;
    roll_pair_instances<T, NX, NP, MU>(p, sa, b0, b1, reinterpret_cast<T*>(smem_raw));
    return;
  }
  const int b = sa.ids ? sa.ids[blockIdx.x] : int(blockIdx.x);
  if (!sa.first) {
    if (instance_stage<T>(p, sa, b) != ST_ROLLOUT) return;
  } else if (sa.active && !sa.active[b]) {
    instance_mark_done<T>(p, sa, b);
    return;
  }
  trial_part_instance<T, NX, NP, MU, 1, TRIAL_ROLL, (XDYN ? kExprDynProg : 0)>(p, nullptr, sa, b, reinterpret_cast<T*>(smem_raw));
}

template <typename T, int NX, int NP, int MU, int PROGID = 0>
__global__ void __launch_bounds__(64) ilq_rows_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = sa.ids ? sa.ids[blockIdx.y] : int(blockIdx.y);
  if (const int stage = instance_stage<T>(p, sa, b); stage != ST_ROLLOUT && stage != ST_QUAD) return;
  // compact rows: nothing dense is written, so the word maps of the dense images are not needed (nor their LDS)
  const short* maps = sa.compact ? nullptr : rows_maps_load(p, smem_raw);
  T* sm = reinterpret_cast<T*>(smem_raw + (sa.compact ? 0 : rows_maps_bytes(p)));
  rows_part_instance<T, NX, NP, MU, PROGID>(p, maps, sa, b, int(blockIdx.x), sm);
}

// SOLVER: the kernel of a problem with per-instance solver columns bound (solver_params_of).  A twin, as the fused trial
// kernel has one for bound problems: this kernel is a chain of dependent loads per instance, and the test of
// DevProblem::inst_solver with its wait cost the unbound fp32 batch of 8192 0.4-0.55 % — the unbound
// twin is the code it was.
template <typename T, int NX, int NP, int MU, bool SOLVER = true>
__global__ void __launch_bounds__(64) ilq_decide_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = sa.ids ? sa.ids[blockIdx.x] : int(blockIdx.x);
  if (const int stage = instance_stage<T>(p, sa, b); stage != ST_ROLLOUT && stage != ST_QUAD) return;
  trial_part_instance<T, NX, NP, MU, 1, TRIAL_DECIDE, 0, false, SOLVER>(p, nullptr, sa, b, reinterpret_cast<T*>(smem_raw));
}

// Speculative line search of the listed instances (ilqg_solve.hpp): candidate j of list entry `slot`.
// FAT (fp64): compiled for two waves per SIMD instead of ILQG_ROLL_WAVES — 256 registers, none spilled.  At four waves per
// SIMD the paired fp64 rollout keeps 42 registers in scratch memory, reloaded inside the time-step chain: a round of a few
// candidates, which costs the latency of one rollout however empty the chip is, runs a third faster without them (n = 16,
// 6 instances x 128 candidates: 248 -> 166 us; the n = 16 constrained workload at B = 1024: 517 -> 533 k it/s); a round
// that fills the chip wants the occupancy back (config 5's scene: 255 k it/s lean, 244 k fat).  The launcher picks.
// SINGLE: one candidate per wavefront (rollout_instance) also where the shape has the paired form — for a round whose
// candidates all find a SIMD of their own, where a launch costs one rollout's chain and the paired chain is the longer
// one (n = 15, a few instances x 128 candidates: 176 us paired).
template <typename T, int NX, int NP, int MU, bool FAT = false, bool SINGLE = false, bool XDYN = false>
__global__ void __launch_bounds__(64, sizeof(T) == 8 ? ((FAT || XDYN) ? 2 : ILQG_ROLL_WAVES) : 1) ilq_probe_roll_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  if constexpr (rollout_pairs(NX, NP, MU) && !SINGLE)  // candidates 2 y and 2 y + 1 in the two halves of the wave
    probe_roll_pair<T, NX, NP, MU>(p, sa, sa.ids[blockIdx.x], blockIdx.x, 2 * int(blockIdx.y), reinterpret_cast<T*>(smem_raw));
  else
    probe_roll_instance<T, NX, NP, MU, XDYN>(p, sa, sa.ids[blockIdx.x], blockIdx.x, blockIdx.y, reinterpret_cast<T*>(smem_raw));
}

// The probing rollouts of a round that fills the chip: 64 / NP candidates of one instance per wavefront, a lane per
// (candidate, subsystem), the RK4 stages in sequence (rollout_lanes, ilqg_stages.hpp) — an eighth of the instructions
// per trajectory of the paired form above, a longer chain per step: the launcher takes it where the round has more
// rollouts than the chip holds at once.
template <typename T, int NX, int NP, int MU>
__global__ void __launch_bounds__(64, 4) ilq_probe_roll_lanes_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  if constexpr (rollout_pairs(NX, NP, MU))
    probe_roll_lanes<T, NX, NP, MU>(p, sa, sa.ids[blockIdx.x], blockIdx.x, rollout_lanes_per_wave(NP) * int(blockIdx.y),
                                    reinterpret_cast<T*>(smem_raw));
}

template <typename T, int NX, int NP, int MU, int PROGID = 0>
__global__ void __launch_bounds__(64, sizeof(T) == 8 ? 4 : 1) ilq_probe_rows_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int slot = blockIdx.y / sa.probe_k, j = blockIdx.y % sa.probe_k;
  const int b = sa.ids[slot];
  {  // leave before the table load if this candidate is not wanted
    const SolveState<T> s = state_load<T>(sa.ws + size_t(b) * sa.ws_stride, ws_layout_of(p, sa));
    if (!probe_wanted(sa, solver_params_of(p, sa.prm, b), s, j)) return;
  }
  const short* maps = sa.compact ? nullptr : rows_maps_load(p, smem_raw);  // merit only: no dense image either way
  T* sm = reinterpret_cast<T*>(smem_raw + (sa.compact ? 0 : rows_maps_bytes(p)));
  probe_rows_instance<T, NX, NP, MU, PROGID>(p, maps, sa, b, slot, j, int(blockIdx.x), sm);
}

template <typename T>
__global__ void __launch_bounds__(kProbeCandidates) ilq_probe_pick_kernel(DevProblem p, SolveArgs<T> sa) {
  __shared__ T merits[kProbeCandidates];  // the candidates' merit values, reduced here one lane per candidate
  probe_pick_instance<T>(p, sa, sa.ids[blockIdx.x], blockIdx.x, merits);
}

// Iterate log and anytime exit (ilqg_solve.hpp): only launched by solves that ask for them.
template <typename T>
__global__ void __launch_bounds__(256) ilq_log_kernel(DevProblem p, SolveArgs<T> sa, IterLog<T> lg) {
  log_part_instance<T>(p, sa, lg, int(blockIdx.x));
}
template <typename T>
__global__ void __launch_bounds__(64) ilq_deadline_kernel(DevProblem p, SolveArgs<T> sa) {
  deadline_part_instance<T>(p, sa, int(blockIdx.x));
}

// Exit kernel: return path of ILQSolver::Solve / AugmentedLagrangianSolver bookkeeping for the instances
// whose inner solve has ended (converged, out of iterations, or line search exhausted).
template <typename T, int NX, int NP, int MU>
__global__ void __launch_bounds__(256) ilq_exit_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x;
  if (instance_stage<T>(p, sa, b) != ST_INNER_DONE) return;
  const QuadTables<T> tb = quad_tables_load<T>(p, smem_raw, b);
  T* sm = reinterpret_cast<T*>(smem_raw + quad_tables_bytes(p, sizeof(T)));
  exit_part_instance<T, NX, NP, MU>(p, tb, sa, b, sm);
}

// LQ kernel: the Riccati sweep at the accepted operating point of every instance that asked for one.
// KIND LQ_PLAYER_WAVES_PACKED is LQ_PLAYER_WAVES compiled for four waves per SIMD (128 registers): the fp32 one-tile
// sweep is three registers over that by itself, and at batches of many instances per CU a fifth resident instance is
// worth more than the two spilled registers cost (n = 14 fp32, B = 8192: 2.15 M vs 2.04 M it/s; B = 1024, where only
// four instances per CU exist: 1.81 M vs 1.85 M — so the launcher picks it for large batches only).
#ifndef ILQG_1W_WAVES_F64
#define ILQG_1W_WAVES_F64 2
#endif
// KIND LQ_SINGLE_WAVE: one wave per instance (ilqg_lq_feedback1w.hpp), compiled for as many waves per SIMD as its LDS
// lets a CU hold instances (fp64: 20 KB -> eight per CU, two per SIMD; fp32: 10 KB -> sixteen, four per SIMD).
// FORMS = false: the same sweep with the m x m solve's broadcasts through read-lanes (ilqg_solve_options::sweep_forms =
// OFF), a second instantiation of the kinds that have the row-broadcast form: each step loop carries one of the two.
// FORMS = 2: the player-parallel sweep with B's constant entries in registers as well (lq_part_instance).
template <typename T, int NX, int NP, int MU, int KIND, int FORMS = 1>
__global__ void __launch_bounds__((KIND == LQ_SINGLE_WAVE ? 64 : KIND == LQ_VALU_FEEDBACK ? LQCfg<T, NX, NP, MU>::NT : ((KIND == LQ_OPEN_LOOP || KIND == LQ_OPEN_LOOP_COMPACT) ? OLCfg<T, NX, NP, MU>::NT : 64 * NP)),
                                  (KIND == LQ_SINGLE_WAVE ? (sizeof(T) == 4 ? 4 : ILQG_1W_WAVES_F64) : KIND == LQ_PLAYER_WAVES_PACKED ? 4 : KIND == LQ_PLAYER_WAVES ? (NX <= 16 ? NP : 2) : ((KIND == LQ_OPEN_LOOP || KIND == LQ_OPEN_LOOP_COMPACT) ? 3 : 1)))
ilq_lq_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x;
  if (sa.clear_counters && b == 0 && threadIdx.x < 4) sa.unfinished[threadIdx.x] = 0;  // (SolveArgs::clear_counters)
  {  // instance_stage, written out: through the helper the compiler schedules this kernel's whole sweep differently
    const WsLayout L = ws_layout_of(p, sa);
    const int stage = reinterpret_cast<const SolveState<T>*>(sa.ws + size_t(b) * sa.ws_stride + L.state)->stage;
    if (stage != ST_LQ) return;
  }
  lq_part_instance<T, NX, NP, MU, (KIND == LQ_PLAYER_WAVES_PACKED ? LQ_PLAYER_WAVES : KIND), FORMS>(p, sa, b, reinterpret_cast<T*>(smem_raw));
}

// The sweep of the run-time-dimensioned solve path (lq_part_generic, ilqg_solve.hpp).
template <typename T>
__global__ void __launch_bounds__(256) gen_lq_kernel(DevProblem p, SolveArgs<T> sa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x;
  if (instance_stage<T>(p, sa, b) != ST_LQ) return;
  lq_part_generic<T>(p, sa, b, reinterpret_cast<T*>(smem_raw));
}

template <typename T>
__global__ void mfma_selftest_kernel(const T* X, const T* Y, const T* C, T* out) {
  mfma_selftest<T>(X, Y, C, out);
}

}  // namespace

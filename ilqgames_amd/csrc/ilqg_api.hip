// ilqg_api.hip — kernels and the C ABI of libilqg_hip.so (gfx950 only).
// Entry points and the reference methods they replace: include/ilqg.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "ilqg_common.hpp"
#include "ilqg_lq.hpp"
#include "ilqg_lq_openloop.hpp"
#include "ilqg_lq_feedback2.hpp"
#include "ilqg_lq_generic.hpp"
#include "ilqg_costates.hpp"
#include "ilqg_models.hpp"
#include "ilqg_nash.hpp"
#include "ilqg_receding.hpp"
#include "ilqg_rowprog.hpp"
#include "ilqg_rowprog_static.hpp"
#include "ilqg_solve.hpp"
#include "ilqg_stages.hpp"

using namespace ilqg;

// The library is built from several translation units of this one file (__graft_entry__.build): one "main" unit
// with the C ABI and every kernel that does not depend on the (n, N, m_i) instantiation, and one unit per entry of
// ILQG_FOR_DIMS (compiled with -DILQG_PART_NX/NP/MU) that holds DimsLaunch<T, n, N, m_i> and the kernels it
// launches — they compile in parallel.  Without those macros the file is a single self-contained unit.
// This is the state the units share.
namespace ilqg_shared __attribute__((visibility("hidden"))) {
// g_prof: the diagnostic builds' buffer (-DILQG_PROFILE=1 / -DILQG_TIMELINE=1: ilqg_debug_set_profile_buffer exists only
// there); the product library has neither the symbol nor the global.
#define ILQG_DIAGNOSTIC_BUILD (ILQG_PROFILE || ILQG_TIMELINE)
#if defined(ILQG_PART_NX)
extern thread_local std::string g_err;
#if ILQG_DIAGNOSTIC_BUILD
extern long long* g_prof;
#endif
#else
thread_local std::string g_err;
#if ILQG_DIAGNOSTIC_BUILD
long long* g_prof = nullptr;  // set through ilqg_debug_set_profile_buffer
#endif
#endif
}  // namespace ilqg_shared
using ilqg_shared::g_err;
#if ILQG_DIAGNOSTIC_BUILD
using ilqg_shared::g_prof;
#endif

namespace {

ilqg_status fail(ilqg_status s, const std::string& msg) {
  g_err = msg;
  return s;
}
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(ILQG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

}  // namespace

// Device scratch of the stand-alone entry points that take no workspace argument (ilqg_lq_*_batch with delta_x /
// costates, ilqg_total_costs_batch, the equilibrium checks).  The caller may hand the library a buffer of its own
// (ilqg_set_scratch): then nothing is allocated here and a call that needs more fails with the size it needs.  Without
// one the library keeps a grow-only allocation per calling thread.  (The solves never use it: ilqg_workspace_bytes.)
namespace ilqg_shared __attribute__((visibility("hidden"))) {
struct ScratchState {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool caller_owned = false;
};
// One per calling thread, shared by the library's translation units — through an accessor: an `extern thread_local` of a
// constant-initialised class type makes the other units call a TLS init function that the defining unit never emits.
ScratchState& scratch_state();
#if !defined(ILQG_PART_NX)
ScratchState& scratch_state() {
  static thread_local ScratchState st;
  return st;
}
#endif
}  // namespace ilqg_shared

namespace {
struct Scratch {  // this unit's view of the shared state
  ilqg_status reserve(size_t need) {
    ilqg_shared::ScratchState& st = ilqg_shared::scratch_state();
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
};
}  // namespace

namespace {


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
  trial_part_instance<T, NX, NP, MU, W, TRIAL_FUSED, PROGID, BOUND>(p, maps, sa, b, sm);
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

// ---------------------------------------------------------------------------------------------------------------
// The sweep of a run-time-dimensioned solve on a SPECIALISED sweep: a game whose (n, N, m_i) has no instantiation is
// embedded in the smallest instantiated shape (NX >= n, NP == N, MU >= max m_i) —
//   states n .. NX - 1:   A = 1 on the diagonal, no column of any B, no row of any Q_i or l_i;
//   controls m_i .. MU - 1 of player i:  a zero column of B_i, a unit diagonal entry of R_ii, zeros in every other block —
// which solves to exact zeros in the added rows of [P | alpha] and leaves every other entry the recursion of
// src/lq_feedback_solver.cpp:110-213 (src/lq_open_loop_solver.cpp:73-195) produces for the game itself: the added
// column of S = R + B^T Z B is the unit vector (the Gershgorin step of :163-176 reads a column at a time and leaves it
// alone: radius 0, diagonal 1), the added rows and columns of every Z_i stay zero.  One workgroup per instance whose
// stage is LQ: (1) the instance's dense rows, written by the run-time-dimensioned row stage, are copied into the padded
// layout (a region of the library's scratch buffer), (2) the specialised sweep of the padded shape runs on them —
// strategies, delta_x and ILQSolver::ExpectedDecrease as in lq_part_instance —, (3) the rows of [P | alpha] that belong
// to the game are copied to where the solve keeps its strategies.  The copies are ~2 x the sweep's own traffic; the sweep
// is the register-tiled one instead of the all-LDS form with a barrier per phase (ilqg_lq_generic.hpp): n = 8,
// m_i = (1, 2), B = 1024: 1.7 ms -> see DESIGN.md 3.8.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int NX, int NP, int MU, bool OL>
struct PadLayout {
  static constexpr int M = NP * MU;
  size_t A, B, Q, l, R, r, P, al, dx, scr, x0, total;
  __host__ __device__ PadLayout(int T_steps, int Rsz, int rsz) {
    size_t o = 0;
    auto take = [&](size_t cnt) {
      const size_t at = o;
      o += (cnt + 3) & ~size_t(3);
      return at;
    };
    const size_t Tn = size_t(T_steps);
    A = take(Tn * NX * NX);
    B = take(Tn * NX * M);
    Q = take(Tn * NP * NX * NX);
    l = take(Tn * NP * NX);
    R = take(Tn * Rsz);
    r = take(Tn * rsz);
    P = take(Tn * M * NX);
    al = take(Tn * M);
    dx = take(Tn * NX);
    scr = take(Tn * size_t(OL ? OLCfg<T, NX, NP, MU>::ROW : NP * (NX + 1) + NX));
    x0 = take(NX);
    total = o;
  }
};

template <typename T>
struct PadArgs {
  T* pad;             // [batch][PadLayout::total]
  size_t pad_stride;  // elements
  PairTable ptp;      // the game's control blocks at MU x MU each
};

template <typename T, int NX, int NP, int MU, bool OL>
struct PadSweep {
  using C = LQCfg<T, NX, NP, MU>;
  static constexpr bool PW = !OL && C::USE_MFMA;
  static constexpr int NT = OL ? OLCfg<T, NX, NP, MU>::NT : LQFeedbackThreads<T, NX, NP, MU, false>::NT;
  static constexpr int WG_PER_CU = OL ? 3 : (PW ? (NX <= 16 ? NP : 2) : 1);
  // the slot the sweep leaves ILQSolver::ExpectedDecrease in (lq_part_instance), and the LDS the launch asks for
  static constexpr int ED_SLOT = OL ? OLCfg<T, NX, NP, MU>::LDS_ELEMS
                                 : (PW && !C::MFMA_ONE_TILE) ? FB2Cfg<T, NX, NP, MU>::LDS_ELEMS : C::oX;
  static constexpr size_t LDS_ELEMS = OL ? OLCfg<T, NX, NP, MU>::LDS_ELEMS + 4
                                      : PW ? MfmaSweepLds<T, NX, NP, MU>::ELEMS + (C::MFMA_ONE_TILE ? 0 : 4) : C::LDS_ELEMS;
};

// The game as the copies see it: its own dimensions and control blocks, and where its rows are.
template <typename T>
struct PadGame {
  int n, m, N, T_steps;
  const int *udim, *uoff;            // [N], [N + 1]
  const PairTable* pt;               // the game's blocks at their own sizes
  const T *A, *Bm, *Q, *l, *R, *r;   // instance bases, the game's dense rows
  const T* x0;                       // [n] or nullptr
  T *P, *alpha, *dx;                 // instance bases of the results; dx may be nullptr
  int want_ed;                       // ILQSolver::ExpectedDecrease into sm[PadSweep::ED_SLOT]
  int adaptive, symmetric;
  const int* xoff;                   // open loop: [N + 1] state offsets of a block-diagonal A, or nullptr (dense)
};

// Steps (1) - (3) above for one instance, by the whole workgroup; `q`: the instance's region of the padded buffer.
template <typename T, int NX, int NP, int MU, bool OL>
__device__ __forceinline__ void padded_sweep_instance(const PadGame<T>& g, const PairTable& ptp, T* q, T* sm) {
  using PS = PadSweep<T, NX, NP, MU, OL>;
  constexpr int M = NP * MU, NT = PS::NT;
  const int tid = threadIdx.x;
  const int n = g.n, m = g.m, Tn = g.T_steps;
  const PadLayout<T, NX, NP, MU, OL> PL(Tn, ptp.Rsz, ptp.rsz);
  // (eight loads in flight per lane: the workgroup is two to four waves, and a load-store pair per trip leaves the
  // copy bound by one memory latency per element)
  auto copy = [&](T* dst, int count, auto src_of) {
    constexpr int U = 8;
    for (int e0 = tid; e0 < count; e0 += NT * U) {
      T v[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int e = e0 + u * NT;
        v[u] = e < count ? src_of(e) : T(0);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int e = e0 + u * NT;
        if (e < count) dst[e] = v[u];
      }
    }
  };
  // ---- (1) dense rows of the game -> rows of the padded shape ----
  {
    const T *A = g.A, *Bm = g.Bm, *Q = g.Q, *l = g.l, *R = g.R, *r = g.r;
    const PairTable& pt = *g.pt;
    copy(q + PL.A, Tn * NX * NX, [&](int e) {
      const int k = e / (NX * NX), f = e - k * (NX * NX), c = f / NX, row = f - c * NX;
      return (row < n && c < n) ? A[size_t(k) * n * n + row + n * c] : (row == c ? T(1) : T(0));
    });
    copy(q + PL.B, Tn * NX * M, [&](int e) {
      const int k = e / (NX * M), f = e - k * (NX * M), c = f / NX, row = f - c * NX, i = c / MU, ce = c - i * MU;
      return (row < n && ce < g.udim[i]) ? Bm[size_t(k) * n * m + row + n * (g.uoff[i] + ce)] : T(0);
    });
    copy(q + PL.Q, Tn * NP * NX * NX, [&](int e) {
      const int ki = e / (NX * NX), f = e - ki * (NX * NX), c = f / NX, row = f - c * NX;  // ki = k * NP + i
      return (row < n && c < n) ? Q[size_t(ki) * n * n + row + n * c] : T(0);
    });
    copy(q + PL.l, Tn * NP * NX, [&](int e) {
      const int ki = e / NX, row = e - ki * NX;
      return row < n ? l[size_t(ki) * n + row] : T(0);
    });
    const int Rsz_p = ptp.Rsz, rsz_p = ptp.rsz;  // npairs * MU * MU, npairs * MU
    copy(q + PL.R, Tn * Rsz_p, [&](int e) {
      const int k = e / Rsz_p, f = e - k * Rsz_p, pq = f / (MU * MU), h = f - pq * (MU * MU), cb = h / MU, ca = h - cb * MU;
      const int mj = g.udim[pt.pj[pq]];
      return (ca < mj && cb < mj) ? R[size_t(k) * pt.Rsz + pt.roff[pq] + ca + mj * cb]
                                  : ((pt.pi[pq] == pt.pj[pq] && ca == cb) ? T(1) : T(0));
    });
    copy(q + PL.r, Tn * rsz_p, [&](int e) {
      const int k = e / rsz_p, f = e - k * rsz_p, pq = f / MU, ca = f - pq * MU;
      const int mj = g.udim[pt.pj[pq]];
      return ca < mj ? r[size_t(k) * pt.rsz + pt.rgoff[pq] + ca] : T(0);
    });
    if (g.x0 && tid < NX) q[PL.x0 + tid] = tid < n ? g.x0[tid] : T(0);
  }
  __threadfence_block();
  __syncthreads();
  // ---- (2) the specialised sweep (dense rows, its own forward pass) ----
  LQArgs<T> la;
  la.A = q + PL.A; la.Bm = q + PL.B; la.Q = q + PL.Q; la.l = q + PL.l; la.R = q + PL.R; la.r = q + PL.r;
  la.x0 = g.x0 ? q + PL.x0 : nullptr;
  la.P = q + PL.P; la.alpha = q + PL.al;
  const bool forward = g.dx != nullptr || g.want_ed;
  la.dx = forward ? q + PL.dx : nullptr;
  la.scratch = (forward || OL) ? q + PL.scr : nullptr;
  la.ed_out = g.want_ed ? sm + PS::ED_SLOT : nullptr;
  la.T_steps = Tn;
  la.adaptive = g.adaptive;
  la.symmetric = g.symmetric;
  if constexpr (OL) {
    if (g.xoff) {  // the added states extend the last player's block (their A entries are its diagonal's)
      la.nsub = NP;
#pragma unroll
      for (int i = 0; i < NP; i++) la.xoff[i] = g.xoff[i];
      la.xoff[NP] = NX;
    }
    lq_openloop_instance<T, NX, NP, MU>(la, ptp, sm);
  } else {
    lq_feedback_dispatch<T, NX, NP, MU, false>(la, ptp, sm);
  }
  __threadfence_block();
  __syncthreads();
  // ---- (3) the game's rows of [P | alpha] (and of delta_x) ----
  copy(g.P, Tn * m * n, [&](int e) {
    const int k = e / (m * n), f = e - k * (m * n), c = f / m, row = f - c * m;
    int i = 0;
    while (i + 1 < g.N && row >= g.uoff[i + 1]) i++;
    return q[PL.P + size_t(k) * M * NX + (i * MU + row - g.uoff[i]) + M * c];
  });
  copy(g.alpha, Tn * m, [&](int e) {
    const int k = e / m, row = e - k * m;
    int i = 0;
    while (i + 1 < g.N && row >= g.uoff[i + 1]) i++;
    return q[PL.al + size_t(k) * M + i * MU + row - g.uoff[i]];
  });
  if (g.dx)
    copy(g.dx, Tn * n, [&](int e) {
      const int k = e / n, row = e - k * n;
      return q[PL.dx + size_t(k) * NX + row];
    });
}

template <typename T, int NX, int NP, int MU, bool OL>
__global__ void __launch_bounds__((PadSweep<T, NX, NP, MU, OL>::NT), (PadSweep<T, NX, NP, MU, OL>::WG_PER_CU))
padded_lq_kernel(DevProblem p, SolveArgs<T> sa, PadArgs<T> pa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  using PS = PadSweep<T, NX, NP, MU, OL>;
  const int b = blockIdx.x;
  const int Tn = p.T;
  if (instance_stage<T>(p, sa, b) != ST_LQ) return;
  const WsLayout L = ws_layout_of(p, sa);
  T* const w = sa.ws + size_t(b) * sa.ws_stride;
  SolveState<T>* const st = reinterpret_cast<SolveState<T>*>(w + L.state);
  const int sacc = __builtin_amdgcn_readfirstlane(st->sacc);
  PadGame<T> g;
  g.n = p.n; g.m = p.m; g.N = p.N; g.T_steps = Tn;
  g.udim = p.udim; g.uoff = p.uoff; g.pt = &p.pairs;
  g.A = w + L.A; g.Bm = w + L.B; g.Q = w + L.Q; g.l = w + L.l; g.R = w + L.R; g.r = w + L.r;
  g.x0 = nullptr;
  g.P = sacc ? sa.P + size_t(b) * Tn * p.m * p.n : w + L.P1;  // strategy buffer 1 - sacc
  g.alpha = sacc ? sa.alpha + size_t(b) * Tn * p.m : w + L.al1;
  g.dx = nullptr;
  g.want_ed = 1;
  g.adaptive = 1;
  g.symmetric = 1;  // what the quadraticisation stage writes
  bool blocks = OL;
  for (int i = 0; i < p.N; i++) blocks = blocks && p.xoff[i + 1] > p.xoff[i];
  g.xoff = blocks ? p.xoff : nullptr;
  padded_sweep_instance<T, NX, NP, MU, OL>(g, pa.ptp, pa.pad + size_t(b) * pa.pad_stride, sm);
  if (threadIdx.x == 0) {
    st->expected_decrease = sm[PS::ED_SLOT];
    st->num_iterations += 1;
    st->step = sa.forced_steps ? sa.forced_steps[size_t(b) * sa.fixed_iters + (st->num_iterations - 1)]
                               : T(solver_real_of(p, b, ILQG_SOLVER_INITIAL_ALPHA_SCALING, sa.prm.initial_alpha_scaling));
    st->bt = 0;
    st->stage = ST_ROLLOUT;
  }
}

// ilqg_lq_feedback_batch / ilqg_lq_openloop_batch for a shape without an instantiation of its own, on the padded sweep.
template <typename T, int NX, int NP, int MU, bool OL>
__global__ void __launch_bounds__((PadSweep<T, NX, NP, MU, OL>::NT), (PadSweep<T, NX, NP, MU, OL>::WG_PER_CU))
padded_lq_batch_kernel(LQBatchArgs<T> a, GenDims d, PairTable pt, PadArgs<T> pa) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const size_t b = blockIdx.x, Tn = d.T, n = d.n, m = d.m, N = d.N;
  PadGame<T> g;
  g.n = d.n; g.m = d.m; g.N = d.N; g.T_steps = d.T;
  g.udim = d.udim; g.uoff = d.uoff; g.pt = &pt;
  g.A = a.A + b * Tn * n * n;
  g.Bm = a.Bm + b * Tn * n * m;
  g.Q = a.Q + b * Tn * N * n * n;
  g.l = a.l + b * Tn * N * n;
  g.R = a.R + b * Tn * pt.Rsz;
  g.r = a.r + b * Tn * pt.rsz;
  g.x0 = a.x0 ? a.x0 + b * n : nullptr;
  g.P = a.P + b * Tn * m * n;
  g.alpha = a.alpha + b * Tn * m;
  g.dx = a.dx ? a.dx + b * Tn * n : nullptr;
  g.want_ed = 0;
  g.adaptive = OL ? 0 : a.adaptive;
  g.symmetric = 0;
  g.xoff = nullptr;
  padded_sweep_instance<T, NX, NP, MU, OL>(g, pa.ptp, pa.pad + b * pa.pad_stride, sm);
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

// ------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------

// Large dynamic-LDS launches: ask for the opt-in limit; a refusal is not fatal by itself (the launch
// reports the real error if the size is unusable), so it must not poison the sticky error state.
void raise_lds_limit(const void* kern, size_t lds) {
  if (lds <= 48 * 1024) return;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
}

// Supported (n, N, m_i) instantiations.  n=14/16/15/24: BASELINE configs 2-5;
// (4,2,2): config 1 (TwoPlayerUnicycle4D); (2,2,1): test_lq_solver's point mass;
// (6,3,2): synthetic parity cases.
#if defined(ILQG_DIMS_HEADER)
#include ILQG_DIMS_HEADER  // experiment builds: a generated subset of the list below (__graft_entry__.build_hip_library)
#else
#define ILQG_FOR_DIMS(X) X(14, 3, 2) X(16, 3, 2) X(15, 3, 2) X(24, 4, 2) X(18, 3, 2) X(12, 2, 2) X(10, 2, 2) X(4, 2, 2) X(6, 2, 1) X(3, 2, 1) X(3, 1, 1) X(2, 2, 1) X(6, 3, 2) X(2, 1, 2) X(8, 2, 2) X(17, 3, 2) X(8, 2, 1)
#endif

#if !defined(ILQG_PART_NX)
// The list as a table, one entry per shape with DimsLaunch's members in both precisions (kShapes, below DimsLaunch):
// the entry of (n, N, m_i), or nullptr where the shape has no instantiation.
struct ShapeEntry;
const ShapeEntry* find_shape(int n, int N, int mu);
#endif

}  // namespace

#include "ilqg_problem.hpp"  // the problem object: its host tables, its device buffers, the handle
#include "ilqg_instances.hpp"  // per-instance declarations and bindings on it
#include "ilqg_schedule.hpp"  // how a solve runs: decide_schedule and the per-round choices

// Launchers of the kernels that are instantiated per (n, N, m_i).  Members are defined out of class (not inline),
// so `extern template struct DimsLaunch<...>` in the main unit of a split build leaves their code — and the
// kernels behind them — to the unit that instantiates them explicitly.
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
  hipLaunchKernelGGL(kern, dim3((d.T + cw - 1) / cw, batch), dim3(64), lds, stream, d, g, cw);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
  hipLaunchKernelGGL(kern, dim3(d->batch), dim3(nt), lds, stream, g, pt);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
  hipLaunchKernelGGL(kern, dim3(d->batch), dim3(O::NT), lds, stream, g, pt);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
      hipLaunchKernelGGL(kern, dim3(sa.batch), dim3(PS::NT), lds, stream, d, sa, pa);
      HIP_TRY(hipGetLastError());
      return ILQG_OK;
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
      hipLaunchKernelGGL(kern, dim3(d->batch), dim3(PS::NT), lds, stream, g, gd, pt, pa);
      HIP_TRY(hipGetLastError());
      return ILQG_OK;
    };
    return open_loop ? go(std::true_type{}) : go(std::false_type{});
  }
}

namespace {

ilqg_status check_device() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(ILQG_ERR_NO_DEVICE, "no HIP device visible: libilqg_hip.so has no CPU fallback");
  return ILQG_OK;
}

}  // namespace

// The round counters' way back to the host.  A counted solve reads them once per round (twice with the augmented
// Lagrangian's restarts), and while it does the device idles: what a read-back costs is the gap between two rounds.
// A copy command plus a stream synchronisation is ~20 us of that; instead a one-wave kernel behind the round's last
// launch stores the four counters and then a sequence number into host memory (pinned, coherent, mapped), and the
// host spins on the sequence number; a device fault shows up in the periodic hipStreamQuery.  Where the pinned mirror
// has no device address (hipHostGetDevicePointer failed) the counters come back by the copy + synchronise form.
namespace {
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

inline ilqg_status read_round_counters(ilqg_problem* p, hipStream_t stream) {
  p->counters_clean = false;
  if (!p->h_unfinished_dev) {
    HIP_TRY(hipMemcpyAsync(p->h_unfinished.get(), p->d_unfinished.get(), 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ILQG_OK;
  }
  const int seq = ++p->publish_seq;
  hipLaunchKernelGGL(ilq_publish_kernel, dim3(1), dim3(64), 0, stream, p->d_unfinished.get(), p->h_unfinished_dev, seq);
  HIP_TRY(hipGetLastError());
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

// ---------------------------------------------------------------------------------------------------------------
// The round protocol both solve drivers share (DimsLaunch::solve on the specialised kernels, generic_solve on the
// run-time-dimensioned ones).  Each driver fills a RoundPlan and run_rounds launches it; what differs between the two
// is a value of the plan, never a question of who is calling.
// ---------------------------------------------------------------------------------------------------------------
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
  hipLaunchKernelGGL(ilq_log_kernel<T>, dim3(sa.batch), dim3(256), 0, stream, p->dev, sa, lg);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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

// LDS limits of every launch of a plan (raise_lds_limit; the padded sweep raises its own)
template <typename T>
void raise_lds_limits(const RoundPlan<T>& pl) {
  for (const KernelLaunch<T>* k : {&pl.trial, &pl.roll, &pl.rows, &pl.decide, &pl.proll, &pl.proll_fat, &pl.proll_single,
                                   &pl.proll_lanes, &pl.prows, &pl.sweep, &pl.exit})
    if (k->kernel) raise_lds_limit((const void*)k->kernel, k->lds);
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
  auto launch = [&](const KernelLaunch<T>& k, dim3 grid) -> ilqg_status {
    hipLaunchKernelGGL(k.kernel, grid, dim3(k.threads), k.lds, stream, d, sa);
    HIP_TRY(hipGetLastError());
    return ILQG_OK;
  };
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
      hipLaunchKernelGGL(ilq_deadline_kernel<T>, dim3(batch), dim3(64), 0, stream, d, sa);
      HIP_TRY(hipGetLastError());
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

}  // namespace

#define DT_DISPATCH(p, CALL) ((p)->desc.dtype == ILQG_F32 ? CALL(float) : CALL(double))

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
    HIP_TRY(hipMemsetAsync(p->d_unfinished.get(), 0, 4 * sizeof(int), stream));  // (whatever an earlier solve left there)
    hipLaunchKernelGGL(ilq_count_active_kernel, dim3(1), dim3(256), 0, stream, opt.active, int(batch), p->d_unfinished.get());
    HIP_TRY(hipGetLastError());
    if (read_round_counters(p, stream) != ILQG_OK) return ILQG_ERR_HIP;
    sched_batch = p->h_unfinished[3] > 0 ? p->h_unfinished[3] : 1;
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

#if defined(ILQG_PART_NX)
// instantiation unit of a split build: this (n, N, m_i) in both precisions, nothing else
template struct DimsLaunch<float, ILQG_PART_NX, ILQG_PART_NP, ILQG_PART_MU>;
template struct DimsLaunch<double, ILQG_PART_NX, ILQG_PART_NP, ILQG_PART_MU>;
#else
#if defined(ILQG_SPLIT_BUILD)
// The list's one expansion besides the table: without these declarations the table's addresses would instantiate every
// shape's launchers, and the kernels behind them, in this unit as well.
#define X(NX_, NP_, MU_)                                   \
  extern template struct DimsLaunch<float, NX_, NP_, MU_>; \
  extern template struct DimsLaunch<double, NX_, NP_, MU_>;
ILQG_FOR_DIMS(X)
#undef X
#endif

namespace {

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
  hipLaunchKernelGGL(kern, dim3(d->batch), dim3(kGenSweepThreads), lds, stream, g, gd, pt, open_loop ? 1 : 0, row);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
  hipLaunchKernelGGL(kern, dim3(d->batch), dim3(256), lds, st, cd, pt, (const T*)A, (const T*)Bm, (const T*)Q, (const T*)l,
                     (const T*)R, (const T*)r, (const T*)P, (const T*)alpha, (const T*)dx, (T*)zs, (T*)costates);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
  if (dtype == ILQG_F32)
    hipLaunchKernelGGL(mfma_selftest_kernel<float>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)X,
                       (const float*)Y, (const float*)C, (float*)out);
  else
    hipLaunchKernelGGL(mfma_selftest_kernel<double>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)X,
                       (const double*)Y, (const double*)C, (double*)out);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
}
int32_t ilqg_abi_version(void) { return ILQG_ABI_VERSION; }

ilqg_status ilqg_copy_bandwidth(void* dst, const void* src, size_t bytes, void* stream) {
  ilqg_status s = check_device();
  if (s != ILQG_OK) return s;
  if (!dst || !src || bytes < 16 || (bytes & 15) || (reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 15))
    return fail(ILQG_ERR_INVALID, "ilqg_copy_bandwidth: 16-byte aligned buffers and a multiple of 16 bytes");
  const size_t n16 = bytes / 16;
  const size_t blocks = (n16 + 1023) / 1024;  // 16 KB per workgroup
  hipLaunchKernelGGL(copy_bandwidth_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<copy_v4f*>(dst), reinterpret_cast<const copy_v4f*>(src), n16);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
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
#define CALL(TY_) upload(std::vector<TY_>(), count * kSegStride + 1, "instance route table", &segs_of<TY_>(p->d_route_segs))
    const ilqg_status s = DT_DISPATCH(p, CALL);
#undef CALL
    if (s != ILQG_OK) {
      (void)ilqg_problem_bind_instance_routes(p, 0, nullptr, stream);
      return s;
    }
  }
  if (count > 0) {
    const dim3 grid((unsigned)((count + 255) / 256));
#define CALL(TY_)                                                                                                           \
  [&]() -> ilqg_status {                                                                                                    \
    hipLaunchKernelGGL(route_segments_kernel<TY_>, grid, dim3(256), 0, (hipStream_t)stream, d.poly_off, d.num_polylines,    \
                       p->d_route_cols.get(), points, p->route_points, segs_of<TY_>(p->d_segs).get(), d.total_segs, batch,  \
                       segs_of<TY_>(p->d_route_segs).get());                                                                \
    HIP_TRY(hipGetLastError());                                                                                             \
    return ILQG_OK;                                                                                                         \
  }()
    if (ilqg_status s = DT_DISPATCH(p, CALL)) return s;
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                           \
    hipLaunchKernelGGL(time_nominals_kernel<TY_>, grid, dim3(256), 0, (hipStream_t)stream, p->d_tnom_tables.get(), \
                       num_tables, d.T, d.dt, speed_pos, segs_of<TY_>(p->d_segs).get(), batch, nominals);          \
    HIP_TRY(hipGetLastError());                                                                                    \
    return ILQG_OK;                                                                                                \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                              \
  [&]() -> ilqg_status {                                                                                     \
    RolloutBatchArgs<TY_> g{(const TY_*)x0, (const TY_*)xs_ref, (const TY_*)us_ref, (const TY_*)P, (const TY_*)alpha,    \
                          (const TY_*)alpha_scale, (TY_*)xs, (TY_*)us, active};                                    \
    auto kern = p->has_expression_dynamics ? rollout_kernel<TY_, true> : rollout_kernel<TY_, false>;             \
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64), rollout_lds_elems(d.n, d.m) * sizeof(TY_),                  \
                       (hipStream_t)stream, d, g);                                                           \
    HIP_TRY(hipGetLastError());                                                                              \
    return ILQG_OK;                                                                                          \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                             \
  [&]() -> ilqg_status {                                                                                    \
    hipLaunchKernelGGL(costs_reduce_kernel<TY_>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d,            \
                       (const TY_*)ilqg_shared::scratch_state().ptr, (TY_*)costs, t_extreme, active);                              \
    HIP_TRY(hipGetLastError());                                                                             \
    return ILQG_OK;                                                                                         \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    hipLaunchKernelGGL(solve_state_kernel<TY_>, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream,        \
                       (const TY_*)workspace, L.total, L.state, batch, (TY_*)last_merit, (TY_*)expected_decrease,   \
                       (TY_*)step, backtracks);                                                                    \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    RecedingArgs<TY_> g{};                                                                                         \
    g.plan = PlanBuffers<TY_>{(TY_*)xs, (TY_*)us, (TY_*)P, (TY_*)alpha, nullptr, nullptr, plan_t0, d.T};          \
    g.x = (const TY_*)x0; g.t = t0; g.planner_runtime = planner_runtime;                                           \
    g.xs = (TY_*)xs; g.us = (TY_*)us; g.P = (TY_*)P; g.alpha = (TY_*)alpha; g.x0_next = (TY_*)x0_next;             \
    g.first_step = first_step;                                                                                     \
    auto kern = p->has_expression_dynamics ? receding_sync_kernel<TY_, true> : receding_sync_kernel<TY_, false>;     \
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(TY_),                                 \
                       (hipStream_t)stream, d, g);                                                                 \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
}

static ilqg_status launch_strategy_costs(const ilqg_problem* p, int32_t batch, const void* x0, const void* xs,
                                         const void* us, const void* P, const void* alpha, double eps, int open_loop,
                                         int euler, int moves, void* costs, void* stream) {
  const DevProblem& d = p->dev;
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    StrategyCostArgs<TY_> g{(const TY_*)x0, (const TY_*)xs, (const TY_*)us, (const TY_*)P, (const TY_*)alpha,      \
                            (TY_*)costs, TY_(eps), open_loop, euler, batch};                                       \
    const size_t lds = quad_tables_bytes(d, sizeof(TY_)) + strategy_cost_lds_elems(d.n, d.m, d.num_terms) * sizeof(TY_); \
    auto kern = p->has_expression_dynamics ? strategy_costs_kernel<TY_, true> : strategy_costs_kernel<TY_, false>; \
    hipLaunchKernelGGL(kern, dim3(batch, moves), dim3(64), lds, (hipStream_t)stream, d, g);                       \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    hipLaunchKernelGGL(nash_verdict_kernel<TY_>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d,                 \
                       (const TY_*)ilqg_shared::scratch_state().ptr, moves, batch, is_nash, (TY_*)margin);                            \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
  hipLaunchKernelGGL(fill_int_kernel<int>, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, is_psd, 1, batch);
  HIP_TRY(hipGetLastError());
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    hipLaunchKernelGGL(psd_check_kernel<TY_>, dim3(d.T, nb), dim3(64), 0, (hipStream_t)stream, full, (TY_*)Q, (TY_*)R, \
                       is_psd + b0);                                                                               \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
    s = DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    PlanIntegrateArgs<TY_> g{};                                                                                    \
    g.plan = PlanBuffers<TY_>{(TY_*)plan_xs, (TY_*)plan_us, (TY_*)plan_P, (TY_*)plan_alpha, (int*)plan_len,       \
                              (double*)plan_t0, 0.0, plan_rows};                                                   \
    g.t_from = t_from; g.t_to = t_to; g.must_contain = must_contain; g.x = (TY_*)x; g.active = active;             \
    auto kern = p->has_expression_dynamics ? plan_integrate_kernel<TY_, true> : plan_integrate_kernel<TY_, false>;   \
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(TY_),                                 \
                       (hipStream_t)stream, d, g);                                                                 \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    RecedingArgs<TY_> g{};                                                                                         \
    g.plan = PlanBuffers<TY_>{(TY_*)plan_xs, (TY_*)plan_us, (TY_*)plan_P, (TY_*)plan_alpha, (int*)plan_len,       \
                              (double*)plan_t0, 0.0, plan_rows};                                                   \
    g.x = (const TY_*)x; g.t = t; g.planner_runtime = planner_runtime;                                             \
    g.xs = (TY_*)xs; g.us = (TY_*)us; g.P = (TY_*)P; g.alpha = (TY_*)alpha; g.x0_next = (TY_*)x0_next;             \
    g.solve_t0 = solve_t0; g.first_step = first_step; g.active = active;                                           \
    auto kern = p->has_expression_dynamics ? receding_sync_kernel<TY_, true> : receding_sync_kernel<TY_, false>;     \
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64), (d.n + d.m + 2) * sizeof(TY_),                                 \
                       (hipStream_t)stream, d, g);                                                                 \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
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
#define CALL(TY_)                                                                                                  \
  [&]() -> ilqg_status {                                                                                         \
    SpliceArgs<TY_> g{};                                                                                           \
    g.plan = PlanBuffers<TY_>{(TY_*)plan_xs, (TY_*)plan_us, (TY_*)plan_P, (TY_*)plan_alpha, plan_len, plan_t0,    \
                              0.0, plan_rows};                                                                     \
    g.xs = (const TY_*)xs; g.us = (const TY_*)us; g.P = (const TY_*)P; g.alpha = (const TY_*)alpha;               \
    g.solve_t0 = solve_t0; g.converged = converged; g.active = active;                                             \
    hipLaunchKernelGGL(splice_kernel<TY_>, dim3(batch), dim3(64), 0, (hipStream_t)stream, d, g);                   \
    HIP_TRY(hipGetLastError());                                                                                  \
    return ILQG_OK;                                                                                              \
  }()
  return DT_DISPATCH(p, CALL);
#undef CALL
}

}  // extern "C"
#endif  // !ILQG_PART_NX

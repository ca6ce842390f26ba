// ilqg_lq_padded.hpp — a game without an instantiation of its own on the specialised sweep of a larger shape.
#pragma once

#include "ilqg_kernels.hpp"  // LQBatchArgs
#include "ilqg_lq_feedback2.hpp"
#include "ilqg_lq_generic.hpp"  // GenDims
#include "ilqg_lq_openloop.hpp"
#include "ilqg_solve.hpp"

namespace {
using namespace ilqg;

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

}  // namespace

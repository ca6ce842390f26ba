// ilqg_expr.hpp — the program of an ILQG_COST_EXPRESSION term (include/ilqg.h: ilqg_expr_op): its validator and its two
// evaluators, in the one form the host (ilqg_problem_create, ilqg_expression_check, tests/host/expr_check.cpp) and the
// kernels (rows_chunk, term_evaluate_leaf_of) both call.  A program is a block [L, (opcode, imm) x L] of floats or of the
// solve's scalars (opcodes and L are small integers, exact in either); it runs on a stack of jets
// (f, fx, fy, fxx, fyy, fxy): second-order forward differentiation over the term's one or two inputs.  Plain C++ apart
// from the two function attributes: a host-only program includes it as it is.
//
// Where the stack lives.  The TOP entry is six scalars of the caller's (registers in a kernel); the entries below it
// are in memory the caller hands in (ExprStack: element e of entry q at base[(6 q + e) * stride]) — in the row stage
// that is LDS, this lane's own column behind the pass's slots, as an affine constraint's temporaries are (ilqg_rows.hpp).
// A unary op never touches memory, a push stores the old top, a binary op loads its lower operand: at most
// ILQG_EXPR_MAX_DEPTH - 1 entries are ever stored (kExprStackScalars).  A gradient-only evaluation (want_h false) neither
// forms nor moves the three second derivatives.
//
// Arithmetic: the table of include/ilqg.h, every product and sum rounded on its own, left to right as written there (no
// contraction, as in ilqg_segment.hpp and ilqg_time_nominal.hpp).  SIN / COS go through ILQG_EXPR_SINCOS, which the
// kernels define as ilqg_trig.hpp's pair before they include this header; anywhere else it is the C library's.
#pragma once

#include <cmath>

#include "ilqg.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ILQG_EXPR_FN __host__ __device__ inline
#else
#define ILQG_EXPR_FN inline
#endif

namespace ilqg {

ILQG_EXPR_FN float expr_sqrt(float v) { return __builtin_sqrtf(v); }
ILQG_EXPR_FN double expr_sqrt(double v) { return __builtin_sqrt(v); }
ILQG_EXPR_FN float expr_exp(float v) { return ::expf(v); }
ILQG_EXPR_FN double expr_exp(double v) { return ::exp(v); }
ILQG_EXPR_FN float expr_log(float v) { return ::logf(v); }
ILQG_EXPR_FN double expr_log(double v) { return ::log(v); }
#ifndef ILQG_EXPR_SINCOS
ILQG_EXPR_FN void expr_sincos(float v, float* s, float* c) { *s = ::sinf(v); *c = ::cosf(v); }
ILQG_EXPR_FN void expr_sincos(double v, double* s, double* c) { *s = ::sin(v); *c = ::cos(v); }
#define ILQG_EXPR_SINCOS(x, s, c) ::ilqg::expr_sincos(x, s, c)
#endif

// PUSH_TIME (18) joined the pushes after the operators were numbered: a push is 1 .. PUSH_VALUE, or it — every valid
// opcode outside the operators' range ADD .. HINGE.  One unsigned compare, as the range test `op <= PUSH_VALUE` was: the
// interpreter's step is a chain of scalar compares and branches, and a second test per op showed in the rollout of an
// expression model.
ILQG_EXPR_FN bool expr_is_push(int op) {
  return unsigned(op - ILQG_EXPR_ADD) > unsigned(ILQG_EXPR_HINGE - ILQG_EXPR_ADD);
}

constexpr int kExprJetScalars = 6;
constexpr int kExprStackScalars = (ILQG_EXPR_MAX_DEPTH - 1) * kExprJetScalars;  // what an evaluation keeps in memory

// ---- the validator ----
enum ExprFault {
  EXPR_OK = 0, EXPR_BAD_LENGTH, EXPR_OUT_OF_RANGE, EXPR_BAD_OPCODE, EXPR_UNDERFLOW, EXPR_OVERFLOW, EXPR_BAD_FINAL_DEPTH,
  EXPR_NO_SECOND_INPUT
};
struct ExprCheck {
  int fault;  // ExprFault
  int op;     // the op at fault (BAD_OPCODE, UNDERFLOW, OVERFLOW, NO_SECOND_INPUT), else -1
  int depth;  // the final depth (BAD_FINAL_DEPTH)
};
// `avail`: the floats from blk to the end of the table it lies in; two_inputs: the term names an input y.
inline ExprCheck expr_validate(const float* blk, long long avail, bool two_inputs) {
  if (blk == nullptr || avail < 1) return {EXPR_OUT_OF_RANGE, -1, 0};
  const float lf = blk[0];
  if (!(lf >= 1.0f && lf <= float(ILQG_EXPR_MAX_OPS)) || lf != float(int(lf))) return {EXPR_BAD_LENGTH, -1, 0};
  const int L = int(lf);
  if (1 + 2 * (long long)L > avail) return {EXPR_OUT_OF_RANGE, -1, 0};
  int depth = 0;
  for (int i = 0; i < L; i++) {
    const float of = blk[1 + 2 * i];
    const int op = (of >= 1.0f && of <= 64.0f && of == float(int(of))) ? int(of) : 0;
    if (op < ILQG_EXPR_PUSH_X || op > ILQG_EXPR_PUSH_TIME) return {EXPR_BAD_OPCODE, i, depth};
    if (expr_is_push(op)) {
      if (op == ILQG_EXPR_PUSH_Y && !two_inputs) return {EXPR_NO_SECOND_INPUT, i, depth};
      if (depth == ILQG_EXPR_MAX_DEPTH) return {EXPR_OVERFLOW, i, depth};
      depth++;
    } else if (op <= ILQG_EXPR_DIV) {
      if (depth < 2) return {EXPR_UNDERFLOW, i, depth};
      depth--;
    } else if (depth < 1) {
      return {EXPR_UNDERFLOW, i, depth};
    }
  }
  if (depth != 1) return {EXPR_BAD_FINAL_DEPTH, -1, depth};
  return {EXPR_OK, -1, 1};
}

// ---- the evaluators (of a program the validator has passed) ----
template <typename T>
struct ExprJet { T f, fx, fy, fxx, fyy, fxy; };

template <typename T>
struct ExprStack {
  T* base;
  int stride;
};

// g, g' and g'' of a unary op at a.f, chained through a's derivatives
template <typename T>
ILQG_EXPR_FN ExprJet<T> expr_chain(const ExprJet<T>& a, T g, T g1, T g2, bool want_h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ExprJet<T> o;
  o.f = g;
  o.fx = g1 * a.fx;
  o.fy = g1 * a.fy;
  o.fxx = o.fyy = o.fxy = T(0);
  if (want_h) {
    o.fxx = g2 * (a.fx * a.fx) + g1 * a.fxx;
    o.fyy = g2 * (a.fy * a.fy) + g1 * a.fyy;
    o.fxy = g2 * (a.fx * a.fy) + g1 * a.fxy;
  }
  return o;
}

// P: anything indexable that yields the block's words (floats, or the solve's scalars made from them).
// `time`: what PUSH_TIME pushes (include/ilqg.h); a program without that op never reads it.
template <typename T, typename P>
ILQG_EXPR_FN void expr_eval_jet(P program, T weight, T value, T x, T y, bool want_h, ExprStack<T> stack, ExprJet<T>* out,
                                T time = T(0)) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int L = int(program[0]);
  ExprJet<T> t{T(0), T(0), T(0), T(0), T(0), T(0)};
  int n = 0;  // entries on the stack, t the top one
  for (int i = 0; i < L; i++) {
    const int op = int(program[1 + 2 * i]);
    if (expr_is_push(op)) {
      if (n > 0) {
        T* const s = stack.base + (n - 1) * kExprJetScalars * stack.stride;
        s[0] = t.f; s[stack.stride] = t.fx; s[2 * stack.stride] = t.fy;
        if (want_h) { s[3 * stack.stride] = t.fxx; s[4 * stack.stride] = t.fyy; s[5 * stack.stride] = t.fxy; }
      }
      n++;
      t.fx = t.fy = t.fxx = t.fyy = t.fxy = T(0);
      if (op == ILQG_EXPR_PUSH_X) { t.f = x; t.fx = T(1); }
      else if (op == ILQG_EXPR_PUSH_Y) { t.f = y; t.fy = T(1); }
      else if (op == ILQG_EXPR_PUSH_CONST) t.f = T(program[2 + 2 * i]);
      else if (op == ILQG_EXPR_PUSH_WEIGHT) t.f = weight;
      else if (op == ILQG_EXPR_PUSH_VALUE) t.f = value;
      else t.f = time;
    } else if (op <= ILQG_EXPR_DIV) {
      n--;
      const T* const s = stack.base + (n - 1) * kExprJetScalars * stack.stride;
      ExprJet<T> a;
      a.f = s[0]; a.fx = s[stack.stride]; a.fy = s[2 * stack.stride];
      a.fxx = a.fyy = a.fxy = T(0);
      if (want_h) { a.fxx = s[3 * stack.stride]; a.fyy = s[4 * stack.stride]; a.fxy = s[5 * stack.stride]; }
      const ExprJet<T> b = t;
      if (op == ILQG_EXPR_ADD) {
        t.f = a.f + b.f; t.fx = a.fx + b.fx; t.fy = a.fy + b.fy;
        t.fxx = a.fxx + b.fxx; t.fyy = a.fyy + b.fyy; t.fxy = a.fxy + b.fxy;
      } else if (op == ILQG_EXPR_SUB) {
        t.f = a.f - b.f; t.fx = a.fx - b.fx; t.fy = a.fy - b.fy;
        t.fxx = a.fxx - b.fxx; t.fyy = a.fyy - b.fyy; t.fxy = a.fxy - b.fxy;
      } else if (op == ILQG_EXPR_MUL) {
        t.f = a.f * b.f;
        t.fx = a.fx * b.f + a.f * b.fx;
        t.fy = a.fy * b.f + a.f * b.fy;
        if (want_h) {
          t.fxx = (a.fxx * b.f + a.f * b.fxx) + T(2) * (a.fx * b.fx);
          t.fyy = (a.fyy * b.f + a.f * b.fyy) + T(2) * (a.fy * b.fy);
          t.fxy = (a.fxy * b.f + a.f * b.fxy) + (a.fx * b.fy + a.fy * b.fx);
        }
      } else {
        const T q = a.f / b.f;
        const T qx = (a.fx - q * b.fx) / b.f;
        const T qy = (a.fy - q * b.fy) / b.f;
        t.f = q; t.fx = qx; t.fy = qy;
        if (want_h) {
          t.fxx = (a.fxx - T(2) * (qx * b.fx) - q * b.fxx) / b.f;
          t.fyy = (a.fyy - T(2) * (qy * b.fy) - q * b.fyy) / b.f;
          t.fxy = (a.fxy - qx * b.fy - qy * b.fx - q * b.fxy) / b.f;
        }
      }
    } else if (op == ILQG_EXPR_HINGE) {
      if (!(t.f > T(0))) t.f = t.fx = t.fy = t.fxx = t.fyy = t.fxy = T(0);
    } else {
      const T a = t.f;
      T g, g1, g2;
      if (op == ILQG_EXPR_NEG) { g = -a; g1 = T(-1); g2 = T(0); }
      else if (op == ILQG_EXPR_SQUARE) { g = a * a; g1 = T(2) * a; g2 = T(2); }
      else if (op == ILQG_EXPR_SQRT) { g = expr_sqrt(a); g1 = T(0.5) / g; g2 = T(-0.5) * g1 / a; }
      else if (op == ILQG_EXPR_EXP) { g = expr_exp(a); g1 = g; g2 = g; }
      else if (op == ILQG_EXPR_LOG) { g = expr_log(a); g1 = T(1) / a; g2 = -(g1 * g1); }
      else {
        T sn, cs;
        ILQG_EXPR_SINCOS(a, &sn, &cs);
        if (op == ILQG_EXPR_SIN) { g = sn; g1 = cs; g2 = -sn; } else { g = cs; g1 = -sn; g2 = -cs; }
      }
      t = expr_chain<T>(t, g, g1, g2, want_h);
    }
  }
  *out = t;
}

// The value alone (Cost::Evaluate): the same f of every op, four scalars and no memory.
template <typename T, typename P>
ILQG_EXPR_FN T expr_eval_value(P program, T weight, T value, T x, T y, T time = T(0)) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(ILQG_EXPR_MAX_DEPTH == 4, "the value stack is four named scalars");
  const int L = int(program[0]);
  T t = T(0), s1 = T(0), s2 = T(0), s3 = T(0);  // the top and the entries below it, nearest first
  for (int i = 0; i < L; i++) {
    const int op = int(program[1 + 2 * i]);
    if (expr_is_push(op)) {
      s3 = s2; s2 = s1; s1 = t;
      if (op == ILQG_EXPR_PUSH_X) t = x;
      else if (op == ILQG_EXPR_PUSH_Y) t = y;
      else if (op == ILQG_EXPR_PUSH_CONST) t = T(program[2 + 2 * i]);
      else if (op == ILQG_EXPR_PUSH_WEIGHT) t = weight;
      else if (op == ILQG_EXPR_PUSH_VALUE) t = value;
      else t = time;
    } else if (op <= ILQG_EXPR_DIV) {
      const T a = s1, b = t;
      s1 = s2; s2 = s3;
      if (op == ILQG_EXPR_ADD) t = a + b;
      else if (op == ILQG_EXPR_SUB) t = a - b;
      else if (op == ILQG_EXPR_MUL) t = a * b;
      else t = a / b;
    } else if (op == ILQG_EXPR_HINGE) {
      if (!(t > T(0))) t = T(0);
    } else if (op == ILQG_EXPR_NEG) t = -t;
    else if (op == ILQG_EXPR_SQUARE) t = t * t;
    else if (op == ILQG_EXPR_SQRT) t = expr_sqrt(t);
    else if (op == ILQG_EXPR_EXP) t = expr_exp(t);
    else if (op == ILQG_EXPR_LOG) t = expr_log(t);
    else {
      T sn, cs;
      ILQG_EXPR_SINCOS(t, &sn, &cs);
      t = op == ILQG_EXPR_SIN ? sn : cs;
    }
  }
  return t;
}

}  // namespace ilqg

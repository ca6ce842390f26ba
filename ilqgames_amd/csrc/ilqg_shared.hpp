// ilqg_shared.hpp — what every translation unit of libilqg_hip.so sees of the state the units share, as declarations.
// The library is one main unit (ilqg_api.hip: the C ABI and every kernel that does not depend on the (n, N, m_i)
// instantiation) and one unit per shape (ilqg_dims.hip: DimsLaunch<T, n, N, m_i> and the kernels it launches).  Each
// name below is defined once, in the main unit, with hidden visibility.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "ilqg_common.hpp"

// g_prof: the diagnostic builds' buffer (-DILQG_PROFILE=1 / -DILQG_TIMELINE=1: ilqg_debug_set_profile_buffer exists only
// there); the product library has neither the symbol nor the global.
#define ILQG_DIAGNOSTIC_BUILD (ILQG_PROFILE || ILQG_TIMELINE)

namespace ilqg_shared __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;  // ilqg_last_error, per calling thread
#if ILQG_DIAGNOSTIC_BUILD
extern long long* g_prof;  // set through ilqg_debug_set_profile_buffer
#endif

ilqg_status fail(ilqg_status s, const std::string& msg);
#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return ilqg_shared::fail(ILQG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// Device scratch of the stand-alone entry points that take no workspace argument (ilqg_lq_*_batch with delta_x /
// costates, ilqg_total_costs_batch, the equilibrium checks).  The caller may hand the library a buffer of its own
// (ilqg_set_scratch): then nothing is allocated here and a call that needs more fails with the size it needs.  Without
// one the library keeps a grow-only allocation per calling thread.  (The solves never use it: ilqg_workspace_bytes.)
struct ScratchState {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool caller_owned = false;
};
// One per calling thread, shared by the library's translation units — through an accessor: an `extern thread_local` of a
// constant-initialised class type makes the other units call a TLS init function that the defining unit never emits.
ScratchState& scratch_state();
struct Scratch {
  ilqg_status reserve(size_t need);  // scratch_state().ptr holds at least `need` bytes, or why not
};

// Large dynamic-LDS launches: ask for the opt-in limit; a refusal is not fatal by itself (the launch
// reports the real error if the size is unusable), so it must not poison the sticky error state.
void raise_lds_limit(const void* kern, size_t lds);

ilqg_status check_device();

// A kernel launch and its error check.  A kernel is launched through its host stub's address, which is valid in every
// unit of the library: the main unit's round loop launches what a shape unit bound.
template <typename... Params, typename... Args>
ilqg_status launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<Args>(args)...);
  HIP_TRY(hipGetLastError());
  return ILQG_OK;
}

// f(T{}) for the precision `dtype` names: with_dtype(dtype, [&](auto tag) { using T = decltype(tag); ... })
template <typename F>
auto with_dtype(int32_t dtype, F f) {
  return dtype == ILQG_F32 ? f(float{}) : f(double{});
}

}  // namespace ilqg_shared

using namespace ilqg_shared;

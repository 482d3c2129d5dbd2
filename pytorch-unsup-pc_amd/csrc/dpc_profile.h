// Opt-in per-kernel timing of the fused path (off by default; bench.py switches it on for a short eager pass).
// When on, every fused-path launch is bracketed by two hipEvents recorded on the launch stream; the caller
// synchronises the stream and then reads (name, milliseconds) pairs, and the template instantiation each launch ran
// (dpc_profile_get_id).  Not usable during graph capture.
#pragma once
#include <hip/hip_runtime.h>

// The instantiation a launch runs, as the launcher knows it: the kernel's name and its integer template arguments
// (printed as the demangled symbol's template, "k_gather_hw<64, 8, 3>"; no arguments: the name alone).  Built from
// compile-time constants at every DPC_LAUNCH site, read only while the record is on.
struct DpcKernelId {
  const char* kernel;
  int nargs;
  int args[3];
};
template <class... A>
constexpr DpcKernelId dpc_kid(const char* kernel, A... args) {
  static_assert(sizeof...(A) <= 3, "DpcKernelId holds up to 3 template arguments");
  return DpcKernelId{kernel, (int)sizeof...(A), {(int)args...}};
}

void dpc_prof_before(const char* name, const DpcKernelId& id, hipStream_t st);
void dpc_prof_after(hipStream_t st);

#ifdef DPC_LAUNCH_TWICE
// timing experiment: every kernel is launched twice back to back (idempotent kernels only); the second launch finds its
// code in the instruction cache, its record carries the suffix "#2"
#define DPC_LAUNCH(name, id, kernel, grid, block, lds, st, ...)      \
  do {                                                               \
    dpc_prof_before(name, id, st);                                   \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);   \
    dpc_prof_after(st);                                              \
    dpc_prof_before(name "#2", id, st);                              \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);   \
    dpc_prof_after(st);                                              \
  } while (0)
#else
#define DPC_LAUNCH(name, id, kernel, grid, block, lds, st, ...)      \
  do {                                                               \
    dpc_prof_before(name, id, st);                                   \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);   \
    dpc_prof_after(st);                                              \
  } while (0)
#endif

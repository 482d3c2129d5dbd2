// Host-side launch plumbing of every kernel file: DPC_LAUNCH and the launch record (dpc_profile.h), the return code of a
// launch (launch_ok) and the one way to raise a kernel's dynamic-LDS limit (LdsLimit, set_lds).  No kernel file calls
// hipFuncSetAttribute or spells out the hipGetLastError test itself.
#pragma once
#include <atomic>
#include <cstddef>

#include "../../include/dpc_render.h"
#include "dpc_profile.h"

// Raise a kernel's dynamic-LDS limit.  hipFuncSetAttribute is a driver call, so it is made once per kernel, device and
// size instead of on every launch: every launcher keeps, per device, the largest size it has set (relaxed atomics: two
// threads racing on the first launch both make the call, which is idempotent).  `slot` is a static of the launcher's
// template instantiation = one per kernel.
struct LdsLimit {
  std::atomic<size_t> set[16];
};
template <class K>
int set_lds(K kernel, size_t bytes, LdsLimit& slot) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return DPC_ERR_LAUNCH;
  const bool tracked = dev >= 0 && dev < 16;
  if (tracked && slot.set[dev].load(std::memory_order_relaxed) >= bytes) return DPC_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return DPC_ERR_LAUNCH;
  if (tracked) slot.set[dev].store(bytes, std::memory_order_relaxed);
  return DPC_OK;
}

inline int launch_ok() { return hipGetLastError() == hipSuccess ? DPC_OK : DPC_ERR_LAUNCH; }

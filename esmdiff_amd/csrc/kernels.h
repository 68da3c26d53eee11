// kernels.h — internal launch functions of libesmdiff_hip.so (gfx950 only).
// Every launch function enqueues on `stream` and returns the hipError_t of the launch; finish_entry below is the one that waits.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/esmdiff_hip.h"
#include "../../include/esmdiff_hip_test.h"

#include <map>
#include <mutex>
#include <utility>

typedef uint16_t bf16_t;  // raw bfloat16 bits

// Types shared by the two operand-type builds of the kernels (namespace ed = bf16, ed16 = f16, see ed_half.h).
struct EdGemmWorkspace {
  float* partial;
  size_t partial_floats;
};
struct EdGemmPartials {
  const float* p;
  int S;
  int64_t stride;
};

// The tail of a C entry that returns when its work is done: the last launch's error, then the stream's -> 0 / ESMDIFF_E_HIP.
inline int finish_entry(hipStream_t st) {
  if (hipGetLastError() != hipSuccess) return ESMDIFF_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? 0 : ESMDIFF_E_HIP;
}

#include "kernels_ns.inc"

// HIP status -> ClipErr(CLIPGPU_ERR_DEVICE) for the host code of the engine, the index and the test hooks.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/clipgpu.h"
#include "host/api_util.hpp"

// A failed runtime call also stays behind as the thread's last error: it is reported here, so it is
// cleared and the next call's launch check (the launchers return hipGetLastError()) does not see it again.
#define HIP_CHECK(expr)                                                                                    \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) {                                                                                \
      (void)hipGetLastError();                                                                             \
      throw ::clipgpu::ClipErr(CLIPGPU_ERR_DEVICE,                                                         \
                               std::string("HIP error: ") + hipGetErrorString(_e) + " (" #expr ")");       \
    }                                                                                                      \
  } while (0)

namespace clipgpu {

// The status of a kernel launcher (kernels/kernels.hpp), named by what was launched.
__attribute__((visibility("hidden"))) inline void check(hipError_t err, const char* what) {
  if (err != hipSuccess) {
    (void)hipGetLastError();  // reported here; do not let the next call's launch check see it again
    throw ClipErr(CLIPGPU_ERR_DEVICE, std::string("HIP error in ") + what + ": " + hipGetErrorString(err));
  }
}

}  // namespace clipgpu

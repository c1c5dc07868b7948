// rmsf_host.h -- host helpers shared by the library's translation units (not
// installed: include/rmsf_hip.h is the public header).  The thread-local
// error message lives in rmsf_kernels.hip, behind rmsf_internal_set_error.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "rmsf_hip.h"

#define RMSF_EXPORT __attribute__((visibility("default")))

extern "C" int rmsf_internal_set_error(int code, const char *msg);

namespace {

// Records the message for rmsf_last_error() and returns the code.
inline int fail(int code, const std::string &m) { return rmsf_internal_set_error(code, m.c_str()); }

inline int after_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RMSF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return RMSF_OK;
}

inline hipStream_t S(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

}  // namespace

// cairo_amd/csrc/hip_status.h -- host plumbing shared by every .hip file's
// entry points: the library's status values, the HIP error report, the colour
// description check, and the owning device buffer of the known-answer tests.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>

#include "../../include/cairo_amd.h"

namespace cairo {

// evx_status (base.h:150-172), the values used inside the library.
constexpr int kSuccess = 0, kInvalidArg = 1, kOutOfMemory = 3, kHardwareFail = 5, kInvalidResource = 8;

static inline int fail(hipError_t e, const char* what) {
  if (e == hipSuccess) return kSuccess;
  fprintf(stderr, "[cairo_amd] %s: %s\n", what, hipGetErrorString(e));
  return kHardwareFail;
}

static inline bool color_known(int range, int matrix) {
  return (range == CAIRO_RANGE_FULL || range == CAIRO_RANGE_LIMITED) &&
         (matrix == CAIRO_MATRIX_BT601 || matrix == CAIRO_MATRIX_BT709);
}

// A device allocation of a known-answer entry point, freed when it leaves
// scope; every step returns the library's status.  mis: the buffer starts that
// many bytes in, so that a device copy keeps its host address modulo 4 or 16.
class KatBuffer {
 public:
  KatBuffer() = default;
  KatBuffer(const KatBuffer&) = delete;
  KatBuffer& operator=(const KatBuffer&) = delete;
  ~KatBuffer() { (void)hipFree(base_); }
  int alloc(size_t bytes, size_t mis = 0) {
    const int r = fail(hipMalloc(&base_, bytes + mis), "malloc");
    if (r == kSuccess) p_ = (uint8_t*)base_ + mis;
    return r;
  }
  int upload(const void* src, size_t bytes, size_t at = 0) {
    return fail(hipMemcpy(p_ + at, src, bytes, hipMemcpyHostToDevice), "h2d");
  }
  int download(void* dst, size_t bytes, size_t at = 0) const {
    return fail(hipMemcpy(dst, p_ + at, bytes, hipMemcpyDeviceToHost), "d2h");
  }
  template <class T>
  T* as() const { return (T*)p_; }

 private:
  void* base_ = nullptr;
  uint8_t* p_ = nullptr;
};

// A launch's status, then the device's once everything queued has run.
static inline int kat_run(hipError_t launched, const char* what) {
  const int r = fail(launched, what);
  return r ? r : fail(hipDeviceSynchronize(), "sync");
}

}  // namespace cairo

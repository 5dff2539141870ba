// cairo_amd/csrc/tensor.h -- launch interface of the tensor frame kernels
// (tensor.hip): strided uint8 / float16 / bfloat16 / float32 device tensors to
// and from the tight RGB24 frame of a staging slot (include/cairo_amd.h,
// cairo_tensor).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cairo_amd.h"

namespace cairo {

// One tensor frame of a launch.
struct TensorFrame {
  uint8_t* tensor;  // element (0, 0, 0), device memory, read (pack) or written (unpack) in place
  uint8_t* rgb;     // the tight RGB24 frame (the frame's staging slot)
  cairo_tensor d;
};

// Every tensor frame of one launch (grid.z = frame); all are w x h, the
// context's size.  A launch with more frames takes several kernels.
constexpr int kTensorFrames = 48;
struct TensorArgs {
  int w, h, nframes, reserved;
  TensorFrame f[kTensorFrames];
};
static_assert(sizeof(TensorArgs) <= 4096, "passed as kernel arguments");

// cairo_tensor_check's verdict (evx_status) and the span in bytes.
int tensor_check(const cairo_tensor* d, const void* base, uint32_t w, uint32_t h, uint64_t* span_bytes);
hipError_t launch_tensor_pack_batch(const TensorArgs& a, hipStream_t s);
hipError_t launch_tensor_unpack(const TensorArgs& a, hipStream_t s);

}  // namespace cairo

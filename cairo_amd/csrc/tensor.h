// cairo_amd/csrc/tensor.h -- launch interface of the tensor frame kernels
// (tensor.hip): strided uint8 / float16 / bfloat16 / float32 device tensors to
// and from the tight RGB24 frame of a staging slot (include/cairo_amd.h,
// cairo_tensor), and of the scaled tensor submit's pre-pass
// (DESIGN.md §4.18).
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

// One scaled tensor frame of a launch: the tensor has the
// source's size, of which the crop is mapped to samples and area-averaged into
// the slot.  lx .. recip are ScaleFrame's (scale.h), for RGB24.
struct TensorScaleFrame {
  const uint8_t* tensor;  // element (0, 0, 0) of the source, device memory, read in place
  uint8_t* rgb;           // the tight RGB24 frame of the context's size (the frame's staging slot)
  cairo_tensor d;
  uint32_t cx, cy;        // crop origin (pixels, even)
  uint32_t cw;            // crop width: no element of a column beyond it is read
  uint32_t lx, px, ly, py;
  uint32_t recip;         // min(floor(2^32 / (lx * ly)), 2^32 - 1)
};

// Every scaled tensor frame of one launch (grid.z = frame); all have the
// output size w x h, the context's.  A launch with more frames takes several
// kernels.
constexpr int kTensorScaleFrames = 36;
struct TensorScaleArgs {
  int w, h, nframes, reserved;
  TensorScaleFrame f[kTensorScaleFrames];
};
static_assert(sizeof(TensorScaleArgs) <= 4096, "passed as kernel arguments");
static_assert(sizeof(TensorScaleArgs) + sizeof(TensorScaleFrame) > 4096, "the capacity is what the block holds");

// cairo_tensor_check's verdict (evx_status) and the span in bytes.
int tensor_check(const cairo_tensor* d, const void* base, uint32_t w, uint32_t h, uint64_t* span_bytes);
// cairo_tensor_scale_check's verdict, the span of the source tensor in bytes
// and the argument block of the frame (either may be nullptr).
int tensor_scale_plan(const cairo_tensor* d, const void* base, const cairo_source* src, uint32_t dw, uint32_t dh,
                      uint8_t* slot, uint64_t* span_bytes, TensorScaleFrame* out);
hipError_t launch_tensor_pack_batch(const TensorArgs& a, hipStream_t s);
hipError_t launch_tensor_unpack(const TensorArgs& a, hipStream_t s);
hipError_t launch_tensor_scale_batch(const TensorScaleArgs& a, hipStream_t s);

}  // namespace cairo

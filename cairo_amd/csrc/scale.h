// cairo_amd/csrc/scale.h -- launch interface of the downscaler (scale.hip):
// an exact-integer area average of a device frame of any CAIRO_FMT_* into a
// tight frame of the same format (include/cairo_amd.h, cairo_source).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cairo_amd.h"
#include "kernels.h"

namespace cairo {

// One scaled frame of a launch.  Per axis, with S source and D output samples
// of the crop, g = gcd(S, D): L = S / g units per output sample, P = D / g
// units per source sample.  The chroma planes (S / 2, D / 2) have the same L
// and P, so one divisor L_x * L_y serves every plane of the frame.
struct ScaleFrame {
  const uint8_t* src;  // the source frame, device memory, read in place
  uint8_t* dst;        // the tight scaled frame (the frame's staging slot)
  uint32_t pitch;      // source row pitch in bytes
  uint32_t sw, sh;     // source frame size
  uint32_t cx, cy;     // crop origin (luma samples / pixels, even)
  uint32_t lx, px, ly, py;
  uint32_t recip;      // min(floor(2^32 / (lx * ly)), 2^32 - 1)
  uint32_t fmt;        // CAIRO_FMT_*
  uint32_t reserved;
};

// Every scaled frame of one launch (grid.z = frame); all have the output size
// dw x dh, the context's.  A launch with more frames takes several kernels.
constexpr int kScaleFrames = 48;
struct ScaleArgs {
  int dw, dh, nframes, reserved;
  ScaleFrame f[kScaleFrames];
};
static_assert(sizeof(ScaleArgs) <= 4096, "passed as kernel arguments");

// The argument block of one frame; cairo_scale_check's verdict (evx_status).
int scale_plan(int fmt, uint32_t pitch, const cairo_source* src, uint32_t dw, uint32_t dh, const uint8_t* frame,
               uint8_t* dst, ScaleFrame* out);
hipError_t launch_scale_batch(const ScaleArgs& a, hipStream_t s);

}  // namespace cairo

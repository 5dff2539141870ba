// cairo_amd/csrc/ctx_internal.h -- hooks of the device context used by the
// frame pipeline (pipeline.cpp) and the drop-in encoder and decoder; not part
// of the C ABI.
#pragma once
#include <atomic>
#include <cstdint>

#include "../../include/cairo_amd.h"

namespace cairo {

// Like cairo_ctx_wait, but never launches the pending batch itself: blocks
// until another thread's submit (a full batch) or flush launched the frame,
// or until *stop becomes true (then kInvalidResource; wake the waiter with
// ctx_wake after setting it).
int ctx_wait_launched(cairo_ctx* c, int ticket, const std::atomic<bool>* stop,
                      cairo_frame_result* out);
// Launch the pending (partial) batch; with ticket >= 0 only if that frame is
// part of it (not yet launched).
int ctx_flush(cairo_ctx* c, int ticket = -1);
void ctx_wake(cairo_ctx* c);
// Macroblock grid, ring size and the ticket the next submit will get.
int ctx_geometry(cairo_ctx* c, uint32_t* wmb, uint32_t* hmb, uint32_t* ring, int* next_ticket);

// Where a frame to encode comes from: what every cairo_ctx_submit* and
// cairo_stream_submit* call describes.
struct FrameSource {
  const uint8_t* base;  // the frame; element (0, 0, 0) of a tensor
  int on_device;        // device memory read in place (scaled and tensor sources always are)
  int fmt;              // CAIRO_FMT_*
  uint32_t pitch;       // row pitch in bytes (0: tight); a scaled source's own
  // Whether a device frame must lie, with all its bytes, inside one allocation.
  // The plain tight-RGB24 calls do not ask (no address-range query per frame on
  // the timed path); every other call does.
  bool check_range;
  const cairo_source* scaled;  // the frame is scaled to the context's size first (or nullptr)
  const cairo_tensor* tensor;  // the frame is a tensor read through this (or nullptr)
};
// Where a decoded frame goes (cairo_ctx_decode_frame*).
struct FrameSink {
  uint8_t* base;   // host frame; element (0, 0, 0) of a device tensor
  int fmt;         // CAIRO_FMT_* through k_planes_to_fmt; kSinkRgb888: RGB888 through k_yuv_to_rgb
  uint32_t pitch;  // row pitch in bytes (0: tight)
  const cairo_tensor* tensor;  // RGB888 is unpacked into this device tensor (or nullptr)
};
constexpr int kSinkRgb888 = -1;
int submit_frame(cairo_ctx* c, const FrameSource& src, uint32_t index, uint32_t type, uint32_t quality, int* ticket);
int decode_frame(cairo_ctx* c, const uint8_t* table, const int16_t* coef, uint32_t index, const FrameSink& out);

}  // namespace cairo

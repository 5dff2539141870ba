// cairo_amd/csrc/frame_io.h -- the frame description the drop-in encoder keeps
// for its input and the drop-in decoder for its output (encoder.cpp,
// decoder.cpp), with the checks their setters share.
#pragma once
#include "../../include/cairo_amd.h"
#include "ctx_internal.h"

namespace cairo {

struct FrameIo {
  int fmt = CAIRO_FMT_RGB24;  // layout of the image (set_format)
  uint32_t pitch = 0;
  bool tensor = false;  // set_tensor: the image is a device tensor through tens
  cairo_tensor tens{};
  int range = CAIRO_RANGE_FULL, matrix = CAIRO_MATRIX_BT601;  // set_color

  // The setters hold between frames too and say whether they took the value.
  // w x h: the frame size of an initialised encoder / decoder, else 0 x 0 (before
  // the first frame, after clear()): any even size stands in and the pitch waits
  // for check().
  bool set_format(int f, uint32_t p, uint32_t w, uint32_t h) {
    if (cairo_frame_layout(f, w ? w : 2, h ? h : 2, w ? p : 0, nullptr, nullptr)) return false;
    fmt = f, pitch = p;
    return true;
  }
  // nullptr: back to the pixel formats.  The strides are checked against the
  // frame size by check().
  bool set_tensor(const cairo_tensor* d) {
    if (d && cairo_tensor_check(d, nullptr, 1, 1, nullptr)) return false;
    tensor = d != nullptr;
    if (d) tens = *d;
    return true;
  }
  // The colour description of I420 / NV12 images (RGB images ignore it);
  // output: 1 for the decoder's.  ctx: the context of an initialised encoder /
  // decoder, else nullptr.
  bool set_color(int output, int r, int m, cairo_ctx* ctx) {
    int32_t k[9], oy;
    if (cairo_color_coefs(output, r, m, k, &oy)) return false;
    if (ctx && (output ? cairo_ctx_set_output_color : cairo_ctx_set_input_color)(ctx, r, m)) return false;
    range = r, matrix = m;
    return true;
  }
  // At each frame: the description against the frame size (0: it fits).
  int check(const void* image, uint32_t w, uint32_t h) const {
    return tensor ? cairo_tensor_check(&tens, image, w, h, nullptr)
                  : cairo_frame_layout(fmt, w, h, pitch, nullptr, nullptr);
  }
  // Tight RGB24 stays on the plain calls' paths: cairo_ctx_submit's, and
  // cairo_ctx_decode_frame's RGB888 through k_yuv_to_rgb.
  bool plain() const { return fmt == CAIRO_FMT_RGB24 && !pitch; }
  FrameSource source(const void* image) const {  // a host image, or a device tensor
    if (tensor) return {(const uint8_t*)image, 1, CAIRO_FMT_RGB24, 0, true, nullptr, &tens};
    return {(const uint8_t*)image, 0, fmt, pitch, !plain(), nullptr, nullptr};
  }
  FrameSink sink(void* image) const {
    if (tensor) return {(uint8_t*)image, kSinkRgb888, 0, &tens};
    return {(uint8_t*)image, plain() ? kSinkRgb888 : fmt, pitch, nullptr};
  }
};

}  // namespace cairo

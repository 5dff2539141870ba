// cairo_amd/csrc/rgb_pixel.h -- the codec's own colour rule between 8-bit RGB
// and its full-range BT.601 YUV 4:2:0 samples, as __host__ __device__
// functions: k_convert_batch, k_yuv_to_rgb and the RGB24 / BGR24 strips of
// pixfmt.hip, and evx1_encoder::peek (encoder.cpp) compile this one text.
// (cairo_amd/__init__.py yuv_to_rgb restates the output rule for the tests.)
// It needs nothing but <stdint.h> and pixel_common.h.  Everything is integer.
#pragma once

#include <stdint.h>

#include "pixel_common.h"

namespace cairo {

// EVX_CONVERT_PIXEL_RGB_TO_YUV (convert.cpp:11-14) as convert_image applies it
// (convert.cpp:30-73): a luma sample per pixel; a chroma sample is the rounded
// mean of the four chroma terms of a 2 x 2 quad.  `/ 256` truncates towards
// zero, `>> 8` floors: the reference's own mix.
//
// A chroma term lies in 1..256 for 8-bit inputs (256: pure blue for U, pure
// red for V), a sum of four in 4..1024: it fits int16_t, so k_convert_batch,
// which carries it through int16_t casts as the reference does, and
// convert_strip, which adds in int, give the same bits; each keeps its form
// because that is what leaves its code as measured.
CAIRO_HD int rgb_luma(int r, int g, int b) { return ((77 * r + 150 * g + 29 * b + 128) >> 8) + 16; }
CAIRO_HD int rgb_chroma_u(int r, int g, int b) { return ((-43 * r - 85 * g + 128 * b + 128) / 256) + 128; }
CAIRO_HD int rgb_chroma_v(int r, int g, int b) { return ((128 * r - 107 * g - 21 * b + 128) / 256) + 128; }
CAIRO_HD int chroma_mean4(int sum) { return (sum + 2) >> 2; }

// saturate narrows to int16 before it clips (math.h:218-221).  Not pinned: a
// caller that packs the byte into a dword pins it (pin8).
CAIRO_HD uint32_t sat8(int32_t v) { return clamp8((int)(int16_t)v); }

// EVX_CONVERT_PIXEL_YUV_TO_RGB (convert.cpp:16-19, 162-223) of y = Y - 16,
// u = U - 128, v = V - 128: the three values, saturated.  One function, not the
// unsaturated values and sat8 apart: with the narrowing in another function
// than the sums, the compiler folds the rounding constant differently and
// k_yuv_to_rgb's code is no longer what was measured.  PIN: each
// value is pinned (pin8) as it is made, for a caller that packs them.
struct Rgb8 {
  uint32_t r, g, b;  // 0..255 each
};
template <bool PIN = false>
CAIRO_HD Rgb8 yuv_to_rgb8(int y, int u, int v) {
  Rgb8 c;
  c.r = sat8((256 * y + 358 * v + 128) >> 8);
  if (PIN) c.r = pin8(c.r);
  c.g = sat8((256 * y - 88 * u - 182 * v + 128) >> 8);
  if (PIN) c.g = pin8(c.g);
  c.b = sat8((256 * y + 452 * u + 128) >> 8);
  if (PIN) c.b = pin8(c.b);
  return c;
}

}  // namespace cairo

// cairo_amd/csrc/capfmt_pixel.h -- the sample rules of the capture and 10-bit
// layouts (include/cairo_amd.h, CAIRO_FMT_YUY2 / UYVY / P010; DESIGN.md
// §4.16), as __host__ __device__ functions: the strips of pixfmt.hip and
// cairo_frame_fold compile this one text.  It needs nothing but <stdint.h>
// and pixel_common.h (the host + device macro and the register pin, pin8).
//
// fold takes a frame of one of the three layouts to the NV12 frame the codec
// takes in its place, unfold takes an NV12 frame back.  Everything is integer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pixel_common.h"

namespace cairo {

constexpr int kFmtYuy2 = 8, kFmtUyvy = 9, kFmtP010 = 10;  // CAIRO_FMT_YUY2 / UYVY / P010

// Every folded or unfolded sample is pinned (pin8) before anything packs it
// into a dword or a pair of half-words.

// Packed 4:2:2 fold: the 4:2:0 chroma sample between rows 2cy and 2cy + 1 is
// the mean of their two 4:2:2 samples, halves rounded up.
CAIRO_HD uint32_t cap_fold_chroma(uint32_t row0, uint32_t row1) { return pin8((row0 + row1 + 1u) >> 1); }

// P010 fold: the ten significant bits are the word's high ten, the low six are
// ignored; to 8 bits by round to nearest, halves up, clamped to 255.
CAIRO_HD uint32_t cap_fold_p010(uint32_t word) {
  const uint32_t s = (((word & 0xFFFFu) >> 6) + 2u) >> 2;
  return pin8(s > 255u ? 255u : s);
}

// P010 unfold: the 8-bit sample in the word's high byte, the low byte zero.
CAIRO_HD uint32_t cap_unfold_p010(uint32_t s8) { return pin8((s8 & 255u) << 8); }

// Byte offsets inside the 4 bytes of a pixel pair: YUY2 is Y0 U Y1 V, UYVY is
// U Y0 V Y1.
CAIRO_HD int cap_y_at(int fmt, int k) { return 2 * k + (fmt == kFmtUyvy ? 1 : 0); }  // luma column k
CAIRO_HD int cap_u_at(int fmt, int j) { return 4 * j + (fmt == kFmtUyvy ? 0 : 1); }  // pair j
CAIRO_HD int cap_v_at(int fmt, int j) { return 4 * j + (fmt == kFmtUyvy ? 2 : 3); }

// The two maps as plain loops on buffers this code can address: what
// cairo_frame_fold runs.  dir 0 reads the frame and writes the NV12 image
// bytes, dir 1 the reverse; only image bytes are written, never pitch padding.
inline void frame_fold_loops(int dir, int fmt, uint32_t w, uint32_t h, size_t pitch, uint8_t* frame, size_t np,
                             uint8_t* nv12) {
  uint8_t* nuv = nv12 + np * h;
  if (fmt == kFmtP010) {
    auto word = [](const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); };  // little endian
    for (uint32_t y = 0; y < h + h / 2; y++)  // the Y rows, then the UV rows: one rule for every sample
      for (uint32_t x = 0; x < w; x++) {
        uint8_t* p = frame + pitch * y + 2 * (size_t)x;
        uint8_t* s = (y < h ? nv12 + np * y : nuv + np * (y - h)) + x;
        if (dir == 0) {
          *s = (uint8_t)cap_fold_p010(word(p));
        } else {
          const uint32_t v = cap_unfold_p010(*s);
          p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8);
        }
      }
    return;
  }
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      uint8_t* p = frame + pitch * y + cap_y_at(fmt, (int)x);
      uint8_t* s = nv12 + np * y + x;
      if (dir == 0)
        *s = *p;
      else
        *p = *s;
    }
  for (uint32_t cy = 0; cy < h / 2; cy++)
    for (uint32_t cx = 0; cx < w / 2; cx++) {
      uint8_t *r0 = frame + pitch * (2 * (size_t)cy), *r1 = r0 + pitch;
      uint8_t* s = nuv + np * cy + 2 * (size_t)cx;
      const int iu = cap_u_at(fmt, (int)cx), iv = cap_v_at(fmt, (int)cx);
      if (dir == 0) {
        s[0] = (uint8_t)cap_fold_chroma(r0[iu], r1[iu]);
        s[1] = (uint8_t)cap_fold_chroma(r0[iv], r1[iv]);
      } else {
        r0[iu] = r1[iu] = s[0];
        r0[iv] = r1[iv] = s[1];
      }
    }
}

}  // namespace cairo

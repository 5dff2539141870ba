// cairo_amd/csrc/tensor_pixel.h -- the sample map of tensor frames
// (include/cairo_amd.h, cairo_tensor), as __host__ __device__
// functions: the kernels of tensor.hip, cairo_tensor_host and the stand-alone
// sanitizer program (tests/sanitize/tensor_host_main.cpp) all compile this one
// text.  It needs nothing but <math.h>, <stdint.h>, <string.h> and
// pixel_common.h (the host + device macro and the register pin, pin8).
//
// Everything is IEEE binary32 with one stated rounding per step: the element
// to float conversions are exact, fmaf rounds once, rintf rounds to nearest
// even, and the narrowing stores round to nearest even in integer arithmetic
// on the bits.  No expression here may be contracted or reassociated: the only
// floating-point operations are the explicit fmaf, rintf and two compares.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pixel_common.h"

namespace cairo {

constexpr uint32_t kDtU8 = 0, kDtF16 = 1, kDtBf16 = 2, kDtF32 = 3;  // CAIRO_DT_*

CAIRO_HD uint32_t tensor_elem_size(uint32_t dtype) { return dtype == kDtU8 ? 1u : (dtype == kDtF32 ? 4u : 2u); }

CAIRO_HD float bits_to_f32(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
CAIRO_HD uint32_t f32_to_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// binary16 bits to float, exact (subnormals, infinities and NaN payloads kept).
CAIRO_HD float f16_bits_to_f32(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 31u) return bits_to_f32(sign | 0x7F800000u | (m << 13));
  if (e) return bits_to_f32(sign | ((e + 112u) << 23) | (m << 13));
  // zero or subnormal: m * 2^-24, an integer below 2^10 times a power of two
  const float v = (float)(int)m * 5.9604644775390625e-08f;
  return sign ? -v : v;
}

// float to binary16 bits: nearest even, overflow to infinity, subnormals kept.
CAIRO_HD uint32_t f32_to_f16_bits(float f) {
  const uint32_t x = f32_to_bits(f), sign = (x >> 16) & 0x8000u, ax = x & 0x7FFFFFFFu;
  if (ax > 0x7F800000u) return sign | 0x7E00u;   // NaN (the map never makes one)
  if (ax >= 0x477FF000u) return sign | 0x7C00u;  // 65520 and above, infinity
  if (ax >= 0x38800000u) {                       // 2^-14 and above: a normal half
    const uint32_t v = ax - 0x38000000u;
    return sign | ((v + 0xFFFu + ((v >> 13) & 1u)) >> 13);  // (a carry moves into the exponent)
  }
  const uint32_t e = ax >> 23;
  if (e < 102u) return sign;  // below 2^-25: zero
  // a multiple of 2^-24: the 24-bit significand shifted down by 126 - e (14..24)
  const uint32_t m = (ax & 0x7FFFFFu) | 0x800000u, sh = 126u - e;
  uint32_t q = m >> sh;
  const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  if (rem > half || (rem == half && (q & 1u))) q++;
  return sign | q;
}

// float to bfloat16 bits: nearest even, overflow to infinity, subnormals kept.
CAIRO_HD uint32_t f32_to_bf16_bits(float f) {
  const uint32_t x = f32_to_bits(f);
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (x >> 16) | 0x40u;  // NaN (the map never makes one)
  return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
}

// Steps 2 and 3 of the input map, and the U8 store of the output map:
// NaN -> 0, else rintf (nearest even), clamped to 0..255; infinities clamp.
// The sample is pinned before anything packs it (pin8).
CAIRO_HD uint32_t tensor_sat8(float t) {
  if (t != t) return 0u;
  float r = rintf(t);
  r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
  return pin8((uint32_t)(int)r);
}

// Element bits (zero-extended, as stored) -> step 1's float.
CAIRO_HD float tensor_elem_to_f32(uint32_t dtype, uint32_t bits) {
  switch (dtype) {
    case kDtU8: return (float)(int)(bits & 255u);
    case kDtF16: return f16_bits_to_f32(bits & 0xFFFFu);
    case kDtBf16: return bits_to_f32(bits << 16);
    default: return bits_to_f32(bits);
  }
}

// dir 0: element bits of channel c -> 8-bit sample.
CAIRO_HD uint32_t tensor_pack_sample(uint32_t dtype, uint32_t bits, float mul, float add) {
  return tensor_sat8(fmaf(tensor_elem_to_f32(dtype, bits), mul, add));
}

// dir 1: 8-bit sample -> element bits of the dtype.
CAIRO_HD uint32_t tensor_unpack_sample(uint32_t dtype, uint32_t s, float mul, float add) {
  const float t = fmaf((float)(int)s, mul, add);
  switch (dtype) {
    case kDtU8: return tensor_sat8(t);
    case kDtF16: return f32_to_f16_bits(t);
    case kDtBf16: return f32_to_bf16_bits(t);
    default: return f32_to_bits(t);
  }
}

// The whole map as plain loops on buffers this code can address: what
// cairo_tensor_host runs.  tensor is the address of element (0, 0, 0); strides
// are in elements.  dir 0 reads the tensor and writes the tight RGB24 frame,
// dir 1 the reverse; only covered elements are written.
inline void tensor_host_loops(int dir, uint32_t dtype, const int64_t stride[3], const float mul[3], const float add[3],
                              uint32_t w, uint32_t h, uint8_t* tensor, uint8_t* rgb24) {
  const uint32_t es = tensor_elem_size(dtype);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++)
      for (uint32_t c = 0; c < 3; c++) {
        uint8_t* e = tensor + (size_t)((int64_t)c * stride[0] + (int64_t)y * stride[1] + (int64_t)x * stride[2]) * es;
        uint8_t* s = rgb24 + ((size_t)y * w + x) * 3 + c;
        if (dir == 0) {
          uint32_t bits = 0;
          memcpy(&bits, e, es);  // (little endian)
          *s = (uint8_t)tensor_pack_sample(dtype, bits, mul[c], add[c]);
        } else {
          const uint32_t bits = tensor_unpack_sample(dtype, *s, mul[c], add[c]);
          memcpy(e, &bits, es);
        }
      }
}

}  // namespace cairo

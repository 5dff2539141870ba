// cairo_amd/csrc/pixel_common.h -- what every 8-bit sample rule at the codec's
// edges shares (rgb_pixel.h, capfmt_pixel.h, tensor_pixel.h and their kernels):
// the host + device macro, the clamp and the register pin.  Needs <stdint.h> only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CAIRO_HD __host__ __device__ __forceinline__
#else
#define CAIRO_HD inline
#endif

namespace cairo {

CAIRO_HD uint32_t clamp8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// A clamped, folded or shifted sample in a 32-bit register of its own before
// anything packs it into a dword or a pair of half-words: left
// to itself the compiler fuses shift, clamp and byte packing into
// v_ashr_pk_u8_i32 and 16-bit ops, and bytes 2 and 3 of a packed dword then
// carried bits of an unclamped neighbour on the device (the same source is
// right on a CPU; the KAT's output side caught it).  Every new clamped byte
// that is packed goes through this.  Empty on the host.
CAIRO_HD uint32_t pin8(uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(r));
#endif
  return r;
}

}  // namespace cairo

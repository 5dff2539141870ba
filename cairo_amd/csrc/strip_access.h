// cairo_amd/csrc/strip_access.h -- how an edge kernel's thread reads or writes
// its strip of a row: the first n of N elements, as one vector access when all
// N are wanted and the address is aligned to it, else element by element with
// nothing past the n-th touched.  Device code: pixfmt.hip, metrics.hip, and
// scale.hip's output dword.  (tensor.hip's element accessors and scale.hip's
// load_column differ in kind and stay with their kernels.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cairo {

// Byte k / half-word k of a little-endian dword array.
template <int W>
__device__ __forceinline__ int byte_of(const uint32_t (&w)[W], int k) {
  return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
}
template <int W>
__device__ __forceinline__ uint32_t half_of(const uint32_t (&w)[W], int k) {
  return (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}

// The unsigned integer of UNIT bytes: the narrow access of load_bytes and
// store_bytes.
template <int UNIT>
struct Narrow {
  typedef uint8_t type;
};
template <>
struct Narrow<2> {
  typedef uint16_t type;
};

// The first n of N bytes at p (N a multiple of 4) into dwords: dword loads
// when all N are wanted and p is 4-byte aligned, else loads of UNIT bytes of
// the n valid ones (the rest read as 0).  UNIT 2: p is 2-byte aligned and n
// even (16-bit samples).
template <int N, int UNIT = 1>
__device__ __forceinline__ void load_bytes(const uint8_t* p, int n, uint32_t (&w)[N / 4]) {
  static_assert(UNIT == 1 || UNIT == 2, "byte or half-word accesses");
  if (n == N && ((uintptr_t)p & 3) == 0) {
    const uint32_t* q = (const uint32_t*)p;
#pragma unroll
    for (int k = 0; k < N / 4; k++) w[k] = q[k];
  } else {
    const typename Narrow<UNIT>::type* q = (const typename Narrow<UNIT>::type*)p;
#pragma unroll
    for (int k = 0; k < N / 4; k++) w[k] = 0;
#pragma unroll
    for (int k = 0; k < N; k += UNIT)
      if (k < n) w[k >> 2] |= (uint32_t)q[k / UNIT] << (8 * (k & 3));
  }
}

// The first n of N bytes held in dwords to p; bytes from n on are not written.
template <int N, int UNIT = 1>
__device__ __forceinline__ void store_bytes(uint8_t* p, int n, const uint32_t (&w)[N / 4]) {
  static_assert(UNIT == 1 || UNIT == 2, "byte or half-word accesses");
  if (n == N && ((uintptr_t)p & 3) == 0) {
    uint32_t* q = (uint32_t*)p;
#pragma unroll
    for (int k = 0; k < N / 4; k++) q[k] = w[k];
  } else {
    typename Narrow<UNIT>::type* q = (typename Narrow<UNIT>::type*)p;
#pragma unroll
    for (int k = 0; k < N; k += UNIT)
      if (k < n) q[k / UNIT] = (typename Narrow<UNIT>::type)(w[k >> 2] >> (8 * (k & 3)));
  }
}

// The first n of N int16 plane elements (N = 8: 16 bytes, N = 4: 8 bytes) at p
// as one vector access when all are wanted and p is aligned to it; elements
// from n on are not written / read as 0.
template <int N>
__device__ __forceinline__ void store_i16(int16_t* p, int n, const int (&v)[N]) {
  static_assert(N == 8 || N == 4, "a 16-byte or an 8-byte plane access");
  if (n == N && ((uintptr_t)p & (2 * N - 1)) == 0) {
    uint32_t w[N / 2];
#pragma unroll
    for (int k = 0; k < N / 2; k++) w[k] = ((uint32_t)v[2 * k] & 0xFFFFu) | ((uint32_t)v[2 * k + 1] << 16);
    if constexpr (N == 8)
      *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
    else
      *(uint2*)p = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int k = 0; k < N; k++)
      if (k < n) p[k] = (int16_t)v[k];
  }
}

template <int N>
__device__ __forceinline__ void load_i16(const int16_t* p, int n, int (&v)[N]) {
  static_assert(N == 8 || N == 4, "a 16-byte or an 8-byte plane access");
  if (n == N && ((uintptr_t)p & (2 * N - 1)) == 0) {
    uint32_t w[N / 2];
    if constexpr (N == 8) {
      const uint4 q = *(const uint4*)p;
      w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
      const uint2 q = *(const uint2*)p;
      w[0] = q.x, w[1] = q.y;
    }
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = (int)(int16_t)(w[k >> 1] >> (16 * (k & 1)));
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = k < n ? (int)p[k] : 0;
  }
}

}  // namespace cairo

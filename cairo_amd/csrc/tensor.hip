// cairo_amd/csrc/tensor.hip -- tensor frames: a strided uint8 / float16 /
// bfloat16 / float32 tensor in device memory to the tight RGB24 frame of a
// staging slot (k_tensor_pack_batch, the tensor submit's pre-pass) and back
// (k_tensor_unpack: a decoded frame or a kept reconstruction written straight
// into the caller's tensor).  include/cairo_amd.h, cairo_tensor; DESIGN.md
// §4.15.  The sample map itself is tensor_pixel.h, shared with the host.
// k_tensor_scale_batch, further down, is the scaled tensor submit's pre-pass
// (DESIGN.md §4.18): a tensor of a larger source's size, mapped to samples and
// area-averaged into the slot in one pass; its work split is described there.
//
// Like the scaled submit's pre-pass, the pack kernel runs before the launch's
// convert kernel and writes the frame's staging slot, which k_convert_batch
// then reads as it reads an uploaded host frame: the convert kernels and the
// engine are untouched.
//
// Work split: a thread owns 4 consecutive pixels of one row (the last strip of
// a row may hold fewer), 128 threads per workgroup, grid = (ceil(W / 512), H,
// frames).  On the tensor side each channel's 4 elements are one 4 / 8 / 16
// byte access where the column stride is 1, the strip is whole and its address
// is aligned to the access; otherwise they are element accesses.  On the RGB24
// side the strip's 12 bytes are three dword accesses where the strip is whole
// and its address is a multiple of 4, else byte accesses.  Nothing outside the
// W x H elements of the three channels is read or written on the tensor side,
// nothing outside the tight frame on the RGB24 side.  No LDS, no scratch.
// The status values, fail() and the KAT's device buffers are hip_status.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <utility>

#include "../../include/cairo_amd.h"
#include "hip_status.h"
#include "scale.h"
#include "tensor.h"
#include "tensor_pixel.h"

namespace cairo {

namespace {

constexpr int kTensorThreads = 128;  // a workgroup spans 512 pixels of one row
constexpr uint64_t kMaxSpanElems = 1ull << 40;

template <uint32_t DT>
struct ElemSize {
  static constexpr int v = DT == kDtU8 ? 1 : (DT == kDtF32 ? 4 : 2);
};

// The element bits of columns lo..n-1 of a strip (zero outside).  p: column 0;
// (Not strip_access.h's accessors: the elements are 1, 2 or 4 bytes wide and a
// column step apart, and the wide access is 4, 8 or 16 bytes accordingly.)
// step: bytes from one column to the next; vec: the 4 elements are contiguous,
// all inside the row, and p is aligned to the 4-element access.
template <uint32_t DT>
__device__ __forceinline__ void load_elems(const uint8_t* p, int64_t step, bool vec, int n, uint32_t bits[4],
                                           int lo = 0) {
  constexpr int ES = ElemSize<DT>::v;
  if (vec) {
    if (ES == 1) {
      const uint32_t v = *(const uint32_t*)p;
#pragma unroll
      for (int k = 0; k < 4; k++) bits[k] = (v >> (8 * k)) & 255u;
    } else if (ES == 2) {
      const uint2 v = *(const uint2*)p;
      bits[0] = v.x & 0xFFFFu, bits[1] = v.x >> 16, bits[2] = v.y & 0xFFFFu, bits[3] = v.y >> 16;
    } else {
      const uint4 v = *(const uint4*)p;
      bits[0] = v.x, bits[1] = v.y, bits[2] = v.z, bits[3] = v.w;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    bits[k] = 0;
    if (k >= lo && k < n) {
      const uint8_t* e = p + k * step;
      bits[k] = ES == 1 ? (uint32_t)*e : (ES == 2 ? (uint32_t) * (const uint16_t*)e : *(const uint32_t*)e);
    }
  }
}

template <uint32_t DT>
__device__ __forceinline__ void store_elems(uint8_t* p, int64_t step, bool vec, int n, const uint32_t bits[4]) {
  constexpr int ES = ElemSize<DT>::v;
  if (vec) {
    if (ES == 1) {
      *(uint32_t*)p = bits[0] | (bits[1] << 8) | (bits[2] << 16) | (bits[3] << 24);
    } else if (ES == 2) {
      *(uint2*)p = make_uint2(bits[0] | (bits[1] << 16), bits[2] | (bits[3] << 16));
    } else {
      *(uint4*)p = make_uint4(bits[0], bits[1], bits[2], bits[3]);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k < n) {
      uint8_t* e = p + k * step;
      if (ES == 1)
        *e = (uint8_t)bits[k];
      else if (ES == 2)
        *(uint16_t*)e = (uint16_t)bits[k];
      else
        *(uint32_t*)e = bits[k];
    }
  }
}

// A strip of the frame: row y, pixels px0 .. px0 + n - 1.
struct Strip {
  int y, px0, n;
  uint8_t* rgb;  // the strip's first RGB24 byte
  bool rgb_vec;  // whole and dword-aligned: three dword accesses (decided once per strip, for both
                 // directions, so not strip_access.h's load_bytes / store_bytes, which decide per access)
};

__device__ __forceinline__ bool make_strip(const TensorArgs& a, const TensorFrame& f, Strip* s) {
  s->y = (int)blockIdx.y;
  s->px0 = 4 * (int)(blockIdx.x * kTensorThreads + threadIdx.x);
  if (s->y >= a.h || s->px0 >= a.w) return false;
  s->n = min(4, a.w - s->px0);
  s->rgb = f.rgb + ((size_t)s->y * (size_t)a.w + (size_t)s->px0) * 3;
  s->rgb_vec = s->n == 4 && ((uintptr_t)s->rgb & 3) == 0;
  return true;
}

// Channel c's column 0 of the strip, the column step in bytes, and whether the
// 4 elements are one aligned access.
template <uint32_t DT>
__device__ __forceinline__ uint8_t* channel_at(const TensorFrame& f, const Strip& s, int c, int64_t* step, bool* vec) {
  constexpr int ES = ElemSize<DT>::v;
  const int64_t e = (int64_t)c * f.d.stride[0] + (int64_t)s.y * f.d.stride[1] + (int64_t)s.px0 * f.d.stride[2];
  uint8_t* p = f.tensor + e * ES;
  *step = f.d.stride[2] * ES;
  *vec = f.d.stride[2] == 1 && s.n == 4 && ((uintptr_t)p & (uintptr_t)(4 * ES - 1)) == 0;
  return p;
}

template <uint32_t DT>
__device__ __forceinline__ void pack_strip(const TensorFrame& f, const Strip& s) {
  uint32_t smp[3][4];  // [channel][pixel], each pinned by tensor_sat8
#pragma unroll
  for (int c = 0; c < 3; c++) {
    int64_t step;
    bool vec;
    const uint8_t* p = channel_at<DT>(f, s, c, &step, &vec);
    uint32_t bits[4];
    load_elems<DT>(p, step, vec, s.n, bits);
#pragma unroll
    for (int k = 0; k < 4; k++) smp[c][k] = tensor_pack_sample(DT, bits[k], f.d.mul[c], f.d.add[c]);
  }
  if (s.rgb_vec) {
    uint32_t d[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int b = 3 * k + c;
        d[b >> 2] |= smp[c][k] << (8 * (b & 3));
      }
    uint32_t* o = (uint32_t*)s.rgb;
    o[0] = d[0], o[1] = d[1], o[2] = d[2];
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < s.n) {
#pragma unroll
        for (int c = 0; c < 3; c++) s.rgb[3 * k + c] = (uint8_t)smp[c][k];
      }
  }
}

template <uint32_t DT>
__device__ __forceinline__ void unpack_strip(const TensorFrame& f, const Strip& s) {
  uint32_t smp[3][4];
  if (s.rgb_vec) {
    const uint32_t* i = (const uint32_t*)s.rgb;
    const uint32_t d[3] = {i[0], i[1], i[2]};
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int b = 3 * k + c;
        smp[c][k] = (d[b >> 2] >> (8 * (b & 3))) & 255u;
      }
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) smp[c][k] = k < s.n ? (uint32_t)s.rgb[3 * k + c] : 0u;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    int64_t step;
    bool vec;
    uint8_t* p = channel_at<DT>(f, s, c, &step, &vec);
    uint32_t bits[4];
#pragma unroll
    for (int k = 0; k < 4; k++) bits[k] = tensor_unpack_sample(DT, smp[c][k], f.d.mul[c], f.d.add[c]);
    store_elems<DT>(p, step, vec, s.n, bits);
  }
}

// grid: x strips of a row, y row, z tensor frame of the launch.  The dtype is
// uniform over the workgroup.
__global__ __launch_bounds__(kTensorThreads) void k_tensor_pack_batch(TensorArgs a) {
  const TensorFrame& f = a.f[blockIdx.z];
  Strip s;
  if (!make_strip(a, f, &s)) return;
  switch (f.d.dtype) {
    case kDtU8: pack_strip<kDtU8>(f, s); break;
    case kDtF16: pack_strip<kDtF16>(f, s); break;
    case kDtBf16: pack_strip<kDtBf16>(f, s); break;
    default: pack_strip<kDtF32>(f, s); break;
  }
}

__global__ __launch_bounds__(kTensorThreads) void k_tensor_unpack(TensorArgs a) {
  const TensorFrame& f = a.f[blockIdx.z];
  Strip s;
  if (!make_strip(a, f, &s)) return;
  switch (f.d.dtype) {
    case kDtU8: unpack_strip<kDtU8>(f, s); break;
    case kDtF16: unpack_strip<kDtF16>(f, s); break;
    case kDtBf16: unpack_strip<kDtBf16>(f, s); break;
    default: unpack_strip<kDtF32>(f, s); break;
  }
}

// The scaled tensor submit's pre-pass: scale(pack(tensor)).
// Every source element of the crop is mapped to its 8-bit sample by
// tensor_pack_sample, and the samples are area-averaged in exact integers by
// the rule of scale.hip (the weights and the rounded division are restated
// here from scale_strip; the frame record carries the same L, P and
// reciprocal):  out = (sum wy * wx * s + (Lx Ly >> 1)) / (Lx Ly), floor.
//
// Work split: a thread owns 4 consecutive output pixels of one row (the last
// strip of a row may hold fewer), 128 threads per workgroup, grid =
// (ceil(W / 512), H, frames) of the output.  Their taps are the crop's columns
// [sa, sb) of rows [ya, yb).  The thread walks them in groups of 4 columns:
// a group's 4 x 4 horizontal weights are computed once and serve every row and
// all three channels.  A channel's 4 elements of a row are one 4 / 8 / 16 byte
// access where the column stride is 1, the group lies inside the crop's
// columns and its address is aligned to the access (the groups start where
// channel 0's first row is), else element accesses of the columns in [sa, sb).
// No element outside the crop is read, the tensor is not written, and nothing
// outside the tight output frame is written.  No LDS, no scratch.
template <uint32_t DT>
__device__ __forceinline__ void scale_tensor_strip(const TensorScaleArgs& a, const TensorScaleFrame& f) {
  constexpr int ES = ElemSize<DT>::v;
  const int row = (int)blockIdx.y;
  const int o0 = 4 * (int)(blockIdx.x * kTensorThreads + threadIdx.x);
  if (row >= a.h || o0 >= a.w) return;
  const int n = min(4, a.w - o0);
  const int lx = (int)f.lx, px = (int)f.px, ly = (int)f.ly, py = (int)f.py, cw = (int)f.cw;
  // the 4 output pixels' unit ranges (pixels past the row's end repeat the last one and are not stored)
  int us[4];
#pragma unroll
  for (int k = 0; k < 4; k++) us[k] = (o0 + min(k, n - 1)) * lx;
  // columns [sa, sb) and rows [ya, yb) of the crop
  const int sa = us[0] / px, sb = (us[3] + lx + px - 1) / px;
  const int uy = row * ly;
  const int ya = uy / py, yb = (uy + ly + py - 1) / py;
  const int64_t s0 = f.d.stride[0], s1 = f.d.stride[1], s2 = f.d.stride[2];
  const bool unit = s2 == 1;
  // element offset of (channel 0, crop row ya, crop column 0)
  const int64_t e0 = (int64_t)(f.cy + (uint32_t)ya) * s1 + (int64_t)f.cx * s2;
  int g0 = sa;
  if (unit) g0 -= (int)(((uint64_t)((uintptr_t)f.tensor / ES) + (uint64_t)(e0 + sa)) & 3);
  uint32_t acc[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int g = g0; g < sb; g += 4) {
    int w[4][4];  // w[i][k]: weight of the group's column i in output pixel k (0 outside [sa, sb))
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int ss = (g + i) * px, se = ss + px;
#pragma unroll
      for (int k = 0; k < 4; k++) w[i][k] = max(min(se, us[k] + lx) - max(ss, us[k]), 0);
    }
    const int lo = max(sa - g, 0), hi = min(sb - g, 4);
    const bool inside = unit && g >= 0 && g + 4 <= cw;
    for (int y = ya; y < yb; y++) {
      const int wy = min((y + 1) * py, uy + ly) - max(y * py, uy);
      const int64_t er = e0 + (int64_t)(y - ya) * s1 + (int64_t)g * s2;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint8_t* p = f.tensor + (er + (int64_t)c * s0) * ES;
        const bool vec = inside && ((uintptr_t)p & (uintptr_t)(4 * ES - 1)) == 0;
        uint32_t bits[4], smp[4];
        load_elems<DT>(p, s2 * ES, vec, hi, bits, lo);
#pragma unroll
        for (int i = 0; i < 4; i++) smp[i] = tensor_pack_sample(DT, bits[i], f.d.mul[c], f.d.add[c]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint32_t h = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) h += (uint32_t)w[i][k] * smp[i];
          acc[c][k] += (uint32_t)wy * h;
        }
      }
    }
  }
  // (acc + (N >> 1)) / N, N = lx * ly: the host's floor(2^32 / N) gives the
  // quotient or one less (the numerator is below 2^31)
  const uint32_t nn = f.lx * f.ly;
  uint8_t* rgb = f.rgb + ((size_t)row * (size_t)a.w + (size_t)o0) * 3;
  uint32_t d[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const uint32_t num = acc[c][k] + (nn >> 1);
      uint32_t q = __umulhi(num, f.recip);
      uint32_t r = num - q * nn;
      if (r >= nn) q++, r -= nn;
      if (r >= nn) q++;
      const int b = 3 * k + c;
      d[b >> 2] |= (q & 255u) << (8 * (b & 3));
    }
  if (n == 4 && ((uintptr_t)rgb & 3) == 0) {
    uint32_t* o = (uint32_t*)rgb;
    o[0] = d[0], o[1] = d[1], o[2] = d[2];
  } else {
#pragma unroll
    for (int b = 0; b < 12; b++)
      if (b < 3 * n) rgb[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
  }
}

// grid: x strips of an output row, y output row, z scaled tensor frame of the
// launch.  The dtype is uniform over the workgroup.
__global__ __launch_bounds__(kTensorThreads) void k_tensor_scale_batch(TensorScaleArgs a) {
  const TensorScaleFrame& f = a.f[blockIdx.z];
  switch (f.d.dtype) {
    case kDtU8: scale_tensor_strip<kDtU8>(a, f); break;
    case kDtF16: scale_tensor_strip<kDtF16>(a, f); break;
    case kDtBf16: scale_tensor_strip<kDtBf16>(a, f); break;
    default: scale_tensor_strip<kDtF32>(a, f); break;
  }
}

bool launch_ok(const TensorArgs& a) {
  return a.nframes >= 1 && a.nframes <= kTensorFrames && a.w >= 1 && a.h >= 1 && a.h <= 65535;
}
dim3 tensor_grid(const TensorArgs& a) {
  return dim3((unsigned)((a.w + 4 * kTensorThreads - 1) / (4 * kTensorThreads)), (unsigned)a.h, (unsigned)a.nframes);
}

}  // namespace

int tensor_check(const cairo_tensor* d, const void* base, uint32_t w, uint32_t h, uint64_t* span_bytes) {
  if (!d || !w || !h || h > 65535) return kInvalidArg;
  if (d->dtype > kDtF32 || d->reserved0 || d->reserved[0] || d->reserved[1]) return kInvalidArg;
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(d->mul[c]) || !std::isfinite(d->add[c])) return kInvalidArg;
  const uint32_t es = tensor_elem_size(d->dtype);
  if ((uintptr_t)base % es) return kInvalidArg;
  // (stride, extent) sorted by stride, ties by extent: each dimension must
  // step over everything the smaller ones cover
  std::pair<int64_t, uint64_t> p[3] = {{d->stride[0], 3}, {d->stride[1], h}, {d->stride[2], w}};
  std::sort(p, p + 3);
  if (p[0].first < 1) return kInvalidArg;
  unsigned __int128 span = 1;
  for (int i = 0; i < 3; i++) {
    if (i && (unsigned __int128)p[i].first < (unsigned __int128)p[i - 1].first * p[i - 1].second) return kInvalidArg;
    span += (unsigned __int128)(p[i].second - 1) * (uint64_t)p[i].first;
    if (span > kMaxSpanElems) return kInvalidArg;
  }
  if (span_bytes) *span_bytes = (uint64_t)span * es;
  return kSuccess;
}

hipError_t launch_tensor_pack_batch(const TensorArgs& a, hipStream_t s) {
  if (!launch_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tensor_pack_batch, tensor_grid(a), dim3(kTensorThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tensor_unpack(const TensorArgs& a, hipStream_t s) {
  if (!launch_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tensor_unpack, tensor_grid(a), dim3(kTensorThreads), 0, s, a);
  return hipGetLastError();
}

int tensor_scale_plan(const cairo_tensor* d, const void* base, const cairo_source* src, uint32_t dw, uint32_t dh,
                      uint8_t* slot, uint64_t* span_bytes, TensorScaleFrame* out) {
  ScaleFrame p;
  if (!src || tensor_check(d, base, src->width, src->height, span_bytes) != kSuccess ||
      scale_plan(CAIRO_FMT_RGB24, 0, src, dw, dh, nullptr, nullptr, &p) != kSuccess)
    return kInvalidArg;
  if (out) {
    out->tensor = (const uint8_t*)base, out->rgb = slot, out->d = *d;
    out->cx = p.cx, out->cy = p.cy;
    out->cw = p.lx * (dw / p.px);
    out->lx = p.lx, out->px = p.px, out->ly = p.ly, out->py = p.py, out->recip = p.recip;
  }
  return kSuccess;
}

hipError_t launch_tensor_scale_batch(const TensorScaleArgs& a, hipStream_t s) {
  if (a.nframes < 1 || a.nframes > kTensorScaleFrames || a.w < 2 || a.h < 2 || a.h > 65535) return hipErrorInvalidValue;
  const int strips = (a.w + 3) / 4;
  hipLaunchKernelGGL(k_tensor_scale_batch, dim3((strips + kTensorThreads - 1) / kTensorThreads, a.h, a.nframes),
                     dim3(kTensorThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace cairo

using namespace cairo;

extern "C" {

int cairo_tensor_size(void) { return (int)sizeof(cairo_tensor); }

int cairo_tensor_check(const cairo_tensor* desc, const void* base, uint32_t width, uint32_t height,
                       uint64_t* span_bytes) {
  return tensor_check(desc, base, width, height, span_bytes);
}

int cairo_tensor_host(int dir, const cairo_tensor* desc, uint32_t w, uint32_t h, void* tensor, uint8_t* rgb24) {
  if ((dir != 0 && dir != 1) || !tensor || !rgb24 || tensor_check(desc, tensor, w, h, nullptr) != kSuccess)
    return kInvalidArg;
  tensor_host_loops(dir, desc->dtype, desc->stride, desc->mul, desc->add, w, h, (uint8_t*)tensor, rgb24);
  return kSuccess;
}

int cairo_kat_tensor(int dir, const cairo_tensor* desc, uint32_t w, uint32_t h, void* tensor, uint64_t tensor_bytes,
                     uint8_t* rgb24, int device) {
  uint64_t span = 0;
  if ((dir != 0 && dir != 1) || !tensor || !rgb24 || tensor_check(desc, tensor, w, h, &span) != kSuccess ||
      span > tensor_bytes)
    return kInvalidArg;
  int r = fail(hipSetDevice(device), "hipSetDevice");
  if (r) return r;
  const size_t rbytes = (size_t)w * h * 3 + CAIRO_KAT_TENSOR_GUARD;
  const size_t mis = (uintptr_t)tensor & 15;  // the device copy keeps the tensor's address modulo 16 (tensor_bytes + 16 allocated)
  KatBuffer dt, dr;
  if ((r = dt.alloc(tensor_bytes + 16 - mis, mis)) || (r = dr.alloc(rbytes))) return r;
  std::unique_ptr<TensorArgs> a(new TensorArgs());
  a->w = (int)w, a->h = (int)h, a->nframes = 1;
  a->f[0].tensor = dt.as<uint8_t>(), a->f[0].rgb = dr.as<uint8_t>(), a->f[0].d = *desc;
  if ((r = dt.upload(tensor, tensor_bytes)) || (r = dr.upload(rgb24, rbytes)) ||
      (r = kat_run(dir ? launch_tensor_unpack(*a, nullptr) : launch_tensor_pack_batch(*a, nullptr), "k_tensor")) ||
      (r = dt.download(tensor, tensor_bytes)) || (r = dr.download(rgb24, rbytes)))
    return r;
  return kSuccess;
}

int cairo_tensor_scale_check(const cairo_tensor* desc, const void* base, const cairo_source* src, uint32_t dst_w,
                             uint32_t dst_h, uint64_t* span_bytes) {
  return tensor_scale_plan(desc, base, src, dst_w, dst_h, nullptr, span_bytes, nullptr);
}

int cairo_kat_tensor_scale(const cairo_tensor* desc, const cairo_source* src, void* tensor, uint64_t tensor_bytes,
                           uint32_t dst_w, uint32_t dst_h, uint8_t* rgb24, int device) {
  uint64_t span = 0;
  if (!tensor || !rgb24 || tensor_scale_plan(desc, tensor, src, dst_w, dst_h, nullptr, &span, nullptr) != kSuccess ||
      span > tensor_bytes)
    return kInvalidArg;
  int r = fail(hipSetDevice(device), "hipSetDevice");
  if (r) return r;
  const size_t rbytes = (size_t)dst_w * dst_h * 3 + CAIRO_KAT_TENSOR_GUARD;
  const size_t mis = (uintptr_t)tensor & 15;  // as cairo_kat_tensor: the device copy keeps the address modulo 16
  KatBuffer dt, dr;
  if ((r = dt.alloc(tensor_bytes + 16 - mis, mis)) || (r = dr.alloc(rbytes))) return r;
  std::unique_ptr<TensorScaleArgs> a(new TensorScaleArgs());
  a->w = (int)dst_w, a->h = (int)dst_h, a->nframes = 1;
  (void)tensor_scale_plan(desc, dt.as<uint8_t>(), src, dst_w, dst_h, dr.as<uint8_t>(), nullptr, &a->f[0]);
  if ((r = dt.upload(tensor, tensor_bytes)) || (r = dr.upload(rgb24, rbytes)) ||
      (r = kat_run(launch_tensor_scale_batch(*a, nullptr), "k_tensor_scale_batch")) ||
      (r = dt.download(tensor, tensor_bytes)) || (r = dr.download(rgb24, rbytes)))
    return r;
  return kSuccess;
}

}  // extern "C"

// cairo_amd/csrc/pixfmt.hip -- every conversion kernel at the codec's edges:
// frames into the int16 4:2:0 source planes, and ring-slot planes out into
// frames.  The sample rules are headers shared with the host (rgb_pixel.h: the
// codec's own RGB <-> YUV; capfmt_pixel.h; pixel_common.h), the strip accesses
// are strip_access.h.
//
// The default launch (every frame tight RGB24) runs k_convert_batch, and
// cairo_ctx_decode_frame runs k_yuv_to_rgb: both are measured beside a running
// engine launch and keep their work split and their
// code (§4.17).  The strip kernels run whenever a launch holds any other
// layout: BGR24, I420, NV12, YUY2, UYVY, P010, and RGB24 with a row pitch.
//
// Work split of both strip kernels: one thread owns a strip of 8 luma columns
// by 2 rows (4 chroma samples per plane): a strip's Y rows are one 16-byte
// plane access each and its 8-bit side is whole dwords.  A strip falls back to
// byte accesses where its row start is not aligned or where it is cut by the
// right edge; nothing outside width x height is read or written on either
// side, so the pitch padding of a destination keeps its bytes.
//
// YUY2, UYVY and P010 frames are the NV12 frame they fold to
// or unfold from (capfmt_pixel.h): 16 bytes of each row of a strip for the
// packed 4:2:2 layouts, 16 of each Y row and 16 of the UV row for P010.
//
// The YUV frames carry a colour description (cairo_amd.h CAIRO_RANGE_*,
// CAIRO_MATRIX_*; YUY2, UYVY and P010: of their NV12).  Both
// strip functions take its mode as a template parameter, chosen once per
// workgroup like the format: identity (the codec's own space: the code as it
// was), diagonal (LIMITED with BT601: no chroma term in the luma) and full.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cairo_amd.h"
#include "capfmt_pixel.h"
#include "hip_status.h"
#include "kernels.h"
#include "rgb_pixel.h"
#include "strip_access.h"

namespace cairo {

namespace {

constexpr int kStrip = 8;         // luma columns per thread
constexpr int kFmtThreads = 128;  // a workgroup spans 1024 luma columns of one row pair

// Modes of a colour description index (kernels.h color_index).
constexpr int kColorIdentity = 0, kColorDiagonal = 1, kColorFull = 2;
constexpr int kColorShift = 14, kColorHalf = 1 << (kColorShift - 1);

// A sample of a colour map: one rounding, clamped to 0..255 and pinned before
// anything packs it.
__device__ __forceinline__ uint32_t color8(int32_t acc) { return pin8(clamp8(acc >> kColorShift)); }

// The map of one strip on its 8-bit samples, in place: y8[dy][k] with the
// chroma sample k >> 1, then the chroma samples themselves (which never depend
// on luma).  IN: the input direction (oy leaves Y before the product), else
// the output direction (oy joins it after).
template <int MODE, bool IN>
__device__ __forceinline__ void color_strip(const ColorMap& m, int (&y8)[2][kStrip], int (&u8)[kStrip / 2],
                                            int (&v8)[kStrip / 2]) {
  static_assert(MODE == kColorDiagonal || MODE == kColorFull, "the identity has no map");
  const int ybias = (IN ? -m.k00 * m.oy : (m.oy << kColorShift)) + kColorHalf;
  constexpr int cbias = (128 << kColorShift) + kColorHalf;
#pragma unroll
  for (int k = 0; k < kStrip / 2; k++) {
    const int d1 = u8[k] - 128, d2 = v8[k] - 128;
    int cy = ybias;
    if constexpr (MODE == kColorFull) cy += m.k01 * d1 + m.k02 * d2;
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
      y8[dy][2 * k] = (int)color8(m.k00 * y8[dy][2 * k] + cy);
      y8[dy][2 * k + 1] = (int)color8(m.k00 * y8[dy][2 * k + 1] + cy);
    }
    if constexpr (MODE == kColorFull) {
      u8[k] = (int)color8(m.k11 * d1 + m.k12 * d2 + cbias);
      v8[k] = (int)color8(m.k21 * d1 + m.k22 * d2 + cbias);
    } else {
      u8[k] = (int)color8(m.k11 * d1 + cbias);
      v8[k] = (int)color8(m.k22 * d2 + cbias);
    }
  }
}

static_assert(kFmtYuy2 == CAIRO_FMT_YUY2 && kFmtUyvy == CAIRO_FMT_UYVY && kFmtP010 == CAIRO_FMT_P010,
              "capfmt_pixel.h names the header's values");

// The formats whose samples are 8-bit YUV once read (for YUY2, UYVY and P010:
// once folded), which a colour description applies to.
constexpr bool fmt_is_yuv(int fmt) {
  return fmt == CAIRO_FMT_I420 || fmt == CAIRO_FMT_NV12 || fmt == CAIRO_FMT_YUY2 || fmt == CAIRO_FMT_UYVY ||
         fmt == CAIRO_FMT_P010;
}

// Slice z == nframes of a convert launch, nthreads threads a workgroup: the
// launch's frame views (mapped host memory -> device) and the zeroed sync area,
// spread over the slice's blocks.
__device__ __forceinline__ void launch_prologue(const ConvertArgs& e, int nthreads) {
  const int nb = gridDim.x * gridDim.y, t = (blockIdx.y * gridDim.x + blockIdx.x) * nthreads + threadIdx.x;
  for (int k = t; k < e.fa_chunks; k += nb * nthreads) e.fa_dev[k] = e.fa_host[k];
  for (int k = t; k < e.sync_words; k += nb * nthreads) e.sync[k] = 0;
}

// ---------------------------------------------------------------------------
// Input side: strip sx of row pair qy of one frame -> its source planes.
// RGB24 / BGR24: the rule of k_convert_batch (rgb_pixel.h).
// I420 / NV12: the codec's own full-range BT.601 samples, Y + 16, U, V; under
// a colour description, the same rule on the mapped samples.
// YUY2 / UYVY / P010: the NV12 rule on the folded samples (capfmt_pixel.h).
// ---------------------------------------------------------------------------
template <int FMT, int MODE = kColorIdentity>
__device__ __forceinline__ void convert_strip(const uint8_t* frame, uint32_t pitch, const PlaneSet& in, int w, int h,
                                              int wa, int sx, int qy, const ColorMap& m) {
  static_assert(MODE == kColorIdentity || fmt_is_yuv(FMT), "a colour description applies to the YUV formats");
  const int x0 = sx * kStrip;
  const int n = min(kStrip, w - x0);  // luma columns of this strip inside the image: 2, 4, 6 or 8
  const int nc = n >> 1;
  int yv[2][kStrip], uv[kStrip / 2], vv[kStrip / 2];
  if constexpr (FMT == CAIRO_FMT_RGB24 || FMT == CAIRO_FMT_BGR24) {
    int su[kStrip / 2] = {}, sv[kStrip / 2] = {};
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
      uint32_t px[6];
      load_bytes<24>(frame + (size_t)(2 * qy + dy) * pitch + 3 * x0, 3 * n, px);
#pragma unroll
      for (int k = 0; k < kStrip; k++) {
        const int c0 = byte_of(px, 3 * k), g = byte_of(px, 3 * k + 1), c2 = byte_of(px, 3 * k + 2);
        const int r = FMT == CAIRO_FMT_RGB24 ? c0 : c2, b = FMT == CAIRO_FMT_RGB24 ? c2 : c0;
        // rgb_luma(r, g, b) written out: the call changed this kernel's code and its BGR24 leg
        yv[dy][k] = ((77 * r + 150 * g + 29 * b + 128) >> 8) + 16;
        su[k >> 1] += rgb_chroma_u(r, g, b);
        sv[k >> 1] += rgb_chroma_v(r, g, b);
      }
    }
#pragma unroll
    for (int k = 0; k < kStrip / 2; k++) uv[k] = chroma_mean4(su[k]), vv[k] = chroma_mean4(sv[k]);
  } else {
    constexpr int ybase = MODE == kColorIdentity ? 16 : 0;
    if constexpr (FMT == CAIRO_FMT_YUY2 || FMT == CAIRO_FMT_UYVY) {
      uint32_t px[2][4];  // 16 bytes of each row: 4 pixel pairs
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        load_bytes<16>(frame + (size_t)(2 * qy + dy) * pitch + 2 * x0, 2 * n, px[dy]);
#pragma unroll
        for (int k = 0; k < kStrip; k++) yv[dy][k] = byte_of(px[dy], cap_y_at(FMT, k)) + ybase;
      }
#pragma unroll
      for (int k = 0; k < kStrip / 2; k++) {
        uv[k] = (int)cap_fold_chroma(byte_of(px[0], cap_u_at(FMT, k)), byte_of(px[1], cap_u_at(FMT, k)));
        vv[k] = (int)cap_fold_chroma(byte_of(px[0], cap_v_at(FMT, k)), byte_of(px[1], cap_v_at(FMT, k)));
      }
    } else if constexpr (FMT == CAIRO_FMT_P010) {
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint32_t py[4];  // 8 words
        load_bytes<16, 2>(frame + (size_t)(2 * qy + dy) * pitch + 2 * x0, 2 * n, py);
#pragma unroll
        for (int k = 0; k < kStrip; k++) yv[dy][k] = (int)cap_fold_p010(half_of(py, k)) + ybase;
      }
      uint32_t puv[4];  // 4 U, V word pairs
      load_bytes<16, 2>(frame + (size_t)pitch * h + (size_t)qy * pitch + 2 * x0, 2 * n, puv);
#pragma unroll
      for (int k = 0; k < kStrip / 2; k++)
        uv[k] = (int)cap_fold_p010(half_of(puv, 2 * k)), vv[k] = (int)cap_fold_p010(half_of(puv, 2 * k + 1));
    } else {
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint32_t py[2];
        load_bytes<8>(frame + (size_t)(2 * qy + dy) * pitch + x0, n, py);
#pragma unroll
        for (int k = 0; k < kStrip; k++) yv[dy][k] = byte_of(py, k) + ybase;
      }
      const uint8_t* chroma = frame + (size_t)pitch * h;
      if constexpr (FMT == CAIRO_FMT_I420) {
        const size_t cp = pitch >> 1;
        const uint8_t* up = chroma + (size_t)qy * cp + (x0 >> 1);
        uint32_t pu[1], pv[1];
        load_bytes<4>(up, nc, pu);
        load_bytes<4>(up + cp * (size_t)(h >> 1), nc, pv);
#pragma unroll
        for (int k = 0; k < kStrip / 2; k++) uv[k] = byte_of(pu, k), vv[k] = byte_of(pv, k);
      } else {
        uint32_t puv[2];
        load_bytes<8>(chroma + (size_t)qy * pitch + x0, n, puv);
#pragma unroll
        for (int k = 0; k < kStrip / 2; k++) uv[k] = byte_of(puv, 2 * k), vv[k] = byte_of(puv, 2 * k + 1);
      }
    }
    if constexpr (MODE != kColorIdentity) {
      color_strip<MODE, true>(m, yv, uv, vv);
#pragma unroll
      for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int k = 0; k < kStrip; k++) yv[dy][k] += 16;
    }
  }
#pragma unroll
  for (int dy = 0; dy < 2; dy++) store_i16<kStrip>(in.y + (size_t)(2 * qy + dy) * wa + x0, n, yv[dy]);
  const size_t co = (size_t)qy * (wa >> 1) + (x0 >> 1);
  store_i16<kStrip / 2>(in.u + co, nc, uv);
  store_i16<kStrip / 2>(in.v + co, nc, vv);
}

// The strip of a YUV format under colour description index col: the identity,
// the diagonal map (LIMITED, BT601) or a full one.
template <int FMT>
__device__ __forceinline__ void convert_strip_col(int col, const uint8_t* frame, uint32_t pitch, const PlaneSet& in,
                                                  int w, int h, int wa, int sx, int qy, const ColorMap& m) {
  if (col == 0)
    convert_strip<FMT>(frame, pitch, in, w, h, wa, sx, qy, m);
  else if (col == 1)
    convert_strip<FMT, kColorDiagonal>(frame, pitch, in, w, h, wa, sx, qy, m);
  else
    convert_strip<FMT, kColorFull>(frame, pitch, in, w, h, wa, sx, qy, m);
}

// Grid convention of both convert kernels: slice z < nframes converts frame z
// (a null source: a decoded frame, nothing to convert), slice z == nframes
// copies the launch's frame views to the device and zeroes its sync area.
__global__ __launch_bounds__(kFmtThreads) void k_convert_fmt_batch(ConvertFmtArgs e) {
  if ((int)blockIdx.z == e.c.nframes) {
    launch_prologue(e.c, kFmtThreads);
    return;
  }
  const uint8_t* frame = e.c.rgb[blockIdx.z];
  const int sx = blockIdx.x * kFmtThreads + threadIdx.x, qy = blockIdx.y;
  if (!frame || sx * kStrip >= e.c.w) return;
  const PlaneSet in = e.c.in[blockIdx.z];
  const uint32_t pitch = e.pitch[blockIdx.z];
  const int col = e.col[blockIdx.z] & (kColorMaps - 1);
  const ColorMap m = e.map[col];
  switch (e.fmt[blockIdx.z]) {  // uniform over the workgroup, as is col
    case CAIRO_FMT_RGB24: convert_strip<CAIRO_FMT_RGB24>(frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    case CAIRO_FMT_BGR24: convert_strip<CAIRO_FMT_BGR24>(frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    case CAIRO_FMT_I420: convert_strip_col<CAIRO_FMT_I420>(col, frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    case CAIRO_FMT_YUY2: convert_strip_col<CAIRO_FMT_YUY2>(col, frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    case CAIRO_FMT_UYVY: convert_strip_col<CAIRO_FMT_UYVY>(col, frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    case CAIRO_FMT_P010: convert_strip_col<CAIRO_FMT_P010>(col, frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
    default: convert_strip_col<CAIRO_FMT_NV12>(col, frame, pitch, in, e.c.w, e.c.h, e.c.wa, sx, qy, m); break;
  }
}

// ---------------------------------------------------------------------------
// Output side: strip sx of row pair qy of a plane set -> the pitched frame.
// RGB24 / BGR24: the rule of k_yuv_to_rgb (rgb_pixel.h), each byte pinned.
// I420 / NV12: clamp(Y - 16), clamp(U), clamp(V) of the int16 samples; under a
// colour description those 8-bit samples are then mapped.
// YUY2 / UYVY / P010: the unfold of those NV12 samples (capfmt_pixel.h).
// ---------------------------------------------------------------------------
template <int FMT, int MODE = kColorIdentity>
__device__ __forceinline__ void planes_strip(const PlaneSet& src, int sp, int w, int h, uint32_t pitch, uint8_t* dst,
                                             int sx, int qy, const ColorMap& m) {
  static_assert(MODE == kColorIdentity || fmt_is_yuv(FMT), "a colour description applies to the YUV formats");
  const int x0 = sx * kStrip;
  const int n = min(kStrip, w - x0);
  const int nc = n >> 1;
  int yv[2][kStrip], uv[kStrip / 2], vv[kStrip / 2];
#pragma unroll
  for (int dy = 0; dy < 2; dy++) load_i16<kStrip>(src.y + (size_t)(2 * qy + dy) * sp + x0, n, yv[dy]);
  const size_t co = (size_t)qy * (sp >> 1) + (x0 >> 1);
  load_i16<kStrip / 2>(src.u + co, nc, uv);
  load_i16<kStrip / 2>(src.v + co, nc, vv);
  if constexpr (FMT == CAIRO_FMT_RGB24 || FMT == CAIRO_FMT_BGR24) {
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
      uint32_t px[6] = {};
#pragma unroll
      for (int k = 0; k < kStrip; k++) {
        const Rgb8 c = yuv_to_rgb8<true>(yv[dy][k] - 16, uv[k >> 1] - 128, vv[k >> 1] - 128);
        const uint32_t g = c.g, c0 = FMT == CAIRO_FMT_RGB24 ? c.r : c.b, c2 = FMT == CAIRO_FMT_RGB24 ? c.b : c.r;
        px[(3 * k) >> 2] |= c0 << (8 * ((3 * k) & 3));
        px[(3 * k + 1) >> 2] |= g << (8 * ((3 * k + 1) & 3));
        px[(3 * k + 2) >> 2] |= c2 << (8 * ((3 * k + 2) & 3));
      }
      store_bytes<24>(dst + (size_t)(2 * qy + dy) * pitch + 3 * x0, 3 * n, px);
    }
  } else {
    if constexpr (MODE != kColorIdentity) {  // clamp to 8 bits as the identity does, then map
#pragma unroll
      for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int k = 0; k < kStrip; k++) yv[dy][k] = (int)clamp8(yv[dy][k] - 16);
#pragma unroll
      for (int k = 0; k < kStrip / 2; k++) uv[k] = (int)clamp8(uv[k]), vv[k] = (int)clamp8(vv[k]);
      color_strip<MODE, false>(m, yv, uv, vv);
    }
    // the bytes to pack: clamped here, or the map's clamped and pinned samples
    auto yb = [&](int dy, int k) { return MODE == kColorIdentity ? clamp8(yv[dy][k] - 16) : (uint32_t)yv[dy][k]; };
    auto ub = [&](int k) { return MODE == kColorIdentity ? clamp8(uv[k]) : (uint32_t)uv[k]; };
    auto vb = [&](int k) { return MODE == kColorIdentity ? clamp8(vv[k]) : (uint32_t)vv[k]; };
    if constexpr (FMT == CAIRO_FMT_YUY2 || FMT == CAIRO_FMT_UYVY) {
      uint32_t cu[kStrip / 2], cv[kStrip / 2];  // both rows of the pair carry the same chroma bytes
#pragma unroll
      for (int k = 0; k < kStrip / 2; k++) cu[k] = pin8(ub(k)), cv[k] = pin8(vb(k));
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint32_t px[4] = {};  // 4 pixel pairs
#pragma unroll
        for (int k = 0; k < kStrip; k++) px[k >> 1] |= pin8(yb(dy, k)) << (8 * (cap_y_at(FMT, k) & 3));
#pragma unroll
        for (int k = 0; k < kStrip / 2; k++)
          px[k] |= (cu[k] << (8 * (cap_u_at(FMT, k) & 3))) | (cv[k] << (8 * (cap_v_at(FMT, k) & 3)));
        store_bytes<16>(dst + (size_t)(2 * qy + dy) * pitch + 2 * x0, 2 * n, px);
      }
    } else if constexpr (FMT == CAIRO_FMT_P010) {
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint32_t py[4] = {};  // 8 words
#pragma unroll
        for (int k = 0; k < kStrip; k++) py[k >> 1] |= cap_unfold_p010(pin8(yb(dy, k))) << (16 * (k & 1));
        store_bytes<16, 2>(dst + (size_t)(2 * qy + dy) * pitch + 2 * x0, 2 * n, py);
      }
      uint32_t puv[4] = {};  // 4 U, V word pairs
#pragma unroll
      for (int k = 0; k < kStrip / 2; k++)
        puv[k] = cap_unfold_p010(pin8(ub(k))) | (cap_unfold_p010(pin8(vb(k))) << 16);
      store_bytes<16, 2>(dst + (size_t)pitch * h + (size_t)qy * pitch + 2 * x0, 2 * n, puv);
    } else {
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        uint32_t py[2] = {};
#pragma unroll
        for (int k = 0; k < kStrip; k++) py[k >> 2] |= yb(dy, k) << (8 * (k & 3));
        store_bytes<8>(dst + (size_t)(2 * qy + dy) * pitch + x0, n, py);
      }
      uint8_t* chroma = dst + (size_t)pitch * h;
      if constexpr (FMT == CAIRO_FMT_I420) {
        const size_t cp = pitch >> 1;
        uint8_t* up = chroma + (size_t)qy * cp + (x0 >> 1);
        uint32_t pu[1] = {}, pv[1] = {};
#pragma unroll
        for (int k = 0; k < kStrip / 2; k++) pu[0] |= ub(k) << (8 * k), pv[0] |= vb(k) << (8 * k);
        store_bytes<4>(up, nc, pu);
        store_bytes<4>(up + cp * (size_t)(h >> 1), nc, pv);
      } else {
        uint32_t puv[2] = {};
#pragma unroll
        for (int k = 0; k < kStrip / 2; k++)
          puv[k >> 1] |= (ub(k) | (vb(k) << 8)) << (16 * (k & 1));
        store_bytes<8>(chroma + (size_t)qy * pitch + x0, n, puv);
      }
    }
  }
}

template <int FMT>
__device__ __forceinline__ void planes_strip_col(int col, const PlaneSet& src, int sp, int w, int h, uint32_t pitch,
                                                 uint8_t* dst, int sx, int qy, const ColorMap& m) {
  if (col == 0)
    planes_strip<FMT>(src, sp, w, h, pitch, dst, sx, qy, m);
  else if (col == 1)
    planes_strip<FMT, kColorDiagonal>(src, sp, w, h, pitch, dst, sx, qy, m);
  else
    planes_strip<FMT, kColorFull>(src, sp, w, h, pitch, dst, sx, qy, m);
}

// col / m: the colour description index of the frame written and its output
// map (used for the YUV formats only).
__global__ __launch_bounds__(kFmtThreads) void k_planes_to_fmt(PlaneSet src, int sp, int w, int h, int fmt,
                                                               uint32_t pitch, uint8_t* dst, int col, ColorMap m) {
  const int sx = blockIdx.x * kFmtThreads + threadIdx.x, qy = blockIdx.y;
  if (sx * kStrip >= w) return;
  switch (fmt) {
    case CAIRO_FMT_RGB24: planes_strip<CAIRO_FMT_RGB24>(src, sp, w, h, pitch, dst, sx, qy, m); break;
    case CAIRO_FMT_BGR24: planes_strip<CAIRO_FMT_BGR24>(src, sp, w, h, pitch, dst, sx, qy, m); break;
    case CAIRO_FMT_I420: planes_strip_col<CAIRO_FMT_I420>(col, src, sp, w, h, pitch, dst, sx, qy, m); break;
    case CAIRO_FMT_YUY2: planes_strip_col<CAIRO_FMT_YUY2>(col, src, sp, w, h, pitch, dst, sx, qy, m); break;
    case CAIRO_FMT_UYVY: planes_strip_col<CAIRO_FMT_UYVY>(col, src, sp, w, h, pitch, dst, sx, qy, m); break;
    case CAIRO_FMT_P010: planes_strip_col<CAIRO_FMT_P010>(col, src, sp, w, h, pitch, dst, sx, qy, m); break;
    default: planes_strip_col<CAIRO_FMT_NV12>(col, src, sp, w, h, pitch, dst, sx, qy, m); break;
  }
}

// The integer maps by direction and description index (kernels.h color_index):
// k_ij = floor(2^14 c_ij + 1/2) of the real matrices of cairo_amd.h, derived in
// exact rationals (tests/color_ref.py re-derives them from Kr and Kb, and
// tests/test_color.py pins this table to that derivation).
constexpr ColorMap kColorTable[2][kColorMaps] = {
    {{16384, 0, 0, 16384, 0, 0, 16384, 0},                // in: FULL, BT601 (the identity)
     {19077, 0, 0, 18651, 0, 0, 18651, 16},               //     LIMITED, BT601
     {16384, 1664, 3213, 16218, -1813, -1187, 16112, 0},  //     FULL, BT709
     {19077, 1895, 3657, 18462, -2064, -1351, 18342, 16}},  //   LIMITED, BT709
    {{16384, 0, 0, 16384, 0, 0, 16384, 0},                  // out
     {14071, 0, 0, 14392, 0, 0, 14392, 16},
     {16384, -1936, -3485, 16689, 1878, 1230, 16799, 0},
     {14071, -1663, -2993, 14660, 1650, 1080, 14757, 16}}};

dim3 strip_grid(int w, int h, int slices) {
  const int strips = (w + kStrip - 1) / kStrip;
  return dim3((strips + kFmtThreads - 1) / kFmtThreads, h / 2, slices);
}

}  // namespace

// ---------------------------------------------------------------------------
// The default input path, tight RGB888 -> YUV 4:2:0 int16 (convert.cpp:11-14,
// 30-73, 95-160): one thread per 2 x 2 quad, 256 quad columns a workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_convert_batch(ConvertArgs e) {
  if ((int)blockIdx.z == e.nframes) {
    launch_prologue(e, 256);
    return;
  }
  const uint8_t* rgb = e.rgb[blockIdx.z];
  const int qx = blockIdx.x * 256 + threadIdx.x;  // quad column
  const int qy = blockIdx.y;                      // quad row
  if (qx >= (e.w >> 1) || !rgb) return;
  const PlaneSet in = e.in[blockIdx.z];
  int su = 0, sv = 0;  // (through int16_t as the reference adds them: rgb_pixel.h)
#pragma unroll
  for (int dy = 0; dy < 2; dy++) {
    const uint8_t* p = rgb + ((size_t)(2 * qy + dy) * e.w + 2 * qx) * 3;
    int16_t* y = in.y + (size_t)(2 * qy + dy) * e.wa + 2 * qx;
#pragma unroll
    for (int dx = 0; dx < 2; dx++) {
      int r = p[3 * dx], g = p[3 * dx + 1], b = p[3 * dx + 2];
      y[dx] = (int16_t)rgb_luma(r, g, b);
      su = (int16_t)(su + rgb_chroma_u(r, g, b));
      sv = (int16_t)(sv + rgb_chroma_v(r, g, b));
    }
  }
  in.u[(size_t)qy * (e.wa >> 1) + qx] = (int16_t)chroma_mean4(su);
  in.v[(size_t)qy * (e.wa >> 1) + qx] = (int16_t)chroma_mean4(sv);
}

hipError_t launch_convert_batch(const ConvertArgs& e, hipStream_t s) {
  dim3 grid((e.w / 2 + 255) / 256, e.h / 2, e.nframes + 1);
  hipLaunchKernelGGL(k_convert_batch, grid, dim3(256), 0, s, e);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The default output path, convert_image YUV -> RGB (convert.cpp:16-19, 75-93,
// 162-223): one thread per horizontal pixel pair.  The crop is
// min(W, Wa) x min(H, Ha) = W x H.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_yuv_to_rgb(PlaneSet src, int wa, int w, int h, uint8_t* rgb) {
  const int x2 = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (2 * x2 >= w) return;
  const int u = src.u[(size_t)(y >> 1) * (wa >> 1) + x2] - 128;
  const int v = src.v[(size_t)(y >> 1) * (wa >> 1) + x2] - 128;
  uint8_t* o = rgb + ((size_t)y * w + 2 * x2) * 3;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const Rgb8 c = yuv_to_rgb8(src.y[(size_t)y * wa + 2 * x2 + k] - 16, u, v);
    o[3 * k] = (uint8_t)c.r, o[3 * k + 1] = (uint8_t)c.g, o[3 * k + 2] = (uint8_t)c.b;
  }
}

hipError_t launch_yuv_to_rgb(PlaneSet src, int wa, int w, int h, uint8_t* rgb, hipStream_t s) {
  hipLaunchKernelGGL(k_yuv_to_rgb, dim3((w / 2 + 255) / 256, h), dim3(256), 0, s, src, wa, w, h, rgb);
  return hipGetLastError();
}

hipError_t launch_convert_fmt_batch(const ConvertFmtArgs& e, hipStream_t s) {
  ConvertFmtArgs a = e;
  for (int k = 0; k < kColorMaps; k++) a.map[k] = kColorTable[0][k];
  hipLaunchKernelGGL(k_convert_fmt_batch, strip_grid(e.c.w, e.c.h, e.c.nframes + 1), dim3(kFmtThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_planes_to_fmt(PlaneSet src, int plane_pitch, int w, int h, int fmt, uint32_t pitch, uint8_t* dst,
                                int col, hipStream_t s) {
  if (col < 0 || col >= kColorMaps) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_planes_to_fmt, strip_grid(w, h, 1), dim3(kFmtThreads), 0, s, src, plane_pitch, w, h, fmt, pitch,
                     dst, col, kColorTable[1][col]);
  return hipGetLastError();
}

}  // namespace cairo

using namespace cairo;

extern "C" {

int cairo_frame_layout(int fmt, uint32_t width, uint32_t height, uint32_t pitch, uint64_t* bytes,
                       uint32_t* tight_pitch) {
  const bool cap = fmt >= CAIRO_FMT_YUY2 && fmt <= CAIRO_FMT_P010;  // (4..7 are unassigned)
  if (fmt < CAIRO_FMT_RGB24 || (fmt > CAIRO_FMT_NV12 && !cap) || !width || !height || (width & 1) || (height & 1))
    return kInvalidArg;
  const bool rgb = fmt == CAIRO_FMT_RGB24 || fmt == CAIRO_FMT_BGR24;
  const bool one_plane = rgb || fmt == CAIRO_FMT_YUY2 || fmt == CAIRO_FMT_UYVY;
  const uint64_t tight = rgb ? (uint64_t)3 * width : cap ? (uint64_t)2 * width : width;
  if (tight > 0xFFFFFFFFull) return kInvalidArg;
  const uint64_t p = pitch ? pitch : tight;
  if (p < tight || ((fmt == CAIRO_FMT_I420 || fmt == CAIRO_FMT_P010) && (p & 1))) return kInvalidArg;
  // 4:2:0: chroma rows hold pitch bytes in all
  if (bytes) *bytes = one_plane ? p * height : p * height + p * (height / 2);
  if (tight_pitch) *tight_pitch = (uint32_t)tight;
  return kSuccess;
}

int cairo_frame_fold(int dir, int fmt, uint32_t w, uint32_t h, uint32_t pitch, uint8_t* frame, uint32_t nv12_pitch,
                     uint8_t* nv12) {
  uint32_t tight = 0, ntight = 0;
  if (dir < 0 || dir > 1 || !frame || !nv12 || fmt < CAIRO_FMT_YUY2 || fmt > CAIRO_FMT_P010 ||
      cairo_frame_layout(fmt, w, h, pitch, nullptr, &tight) != kSuccess ||
      cairo_frame_layout(CAIRO_FMT_NV12, w, h, nv12_pitch, nullptr, &ntight) != kSuccess)
    return kInvalidArg;
  frame_fold_loops(dir, fmt, w, h, pitch ? pitch : tight, frame, nv12_pitch ? nv12_pitch : ntight, nv12);
  return kSuccess;
}

int cairo_color_coefs(int dir, int range, int matrix, int32_t k[9], int32_t* offset) {
  if (dir < 0 || dir > 1 || !color_known(range, matrix) || !k || !offset) return kInvalidArg;
  const ColorMap& m = kColorTable[dir][color_index(range, matrix)];
  const int32_t rows[9] = {m.k00, m.k01, m.k02, 0, m.k11, m.k12, 0, m.k21, m.k22};
  for (int i = 0; i < 9; i++) k[i] = rows[i];
  *offset = m.oy;
  return kSuccess;
}

int cairo_kat_convert(int dir, int fmt, uint32_t w, uint32_t h, uint32_t pitch, uint8_t* frame, int16_t* y, int16_t* u,
                      int16_t* v, int device) {
  return cairo_kat_convert_color(dir, fmt, CAIRO_RANGE_FULL, CAIRO_MATRIX_BT601, w, h, pitch, frame, y, u, v, device);
}

int cairo_kat_convert_color(int dir, int fmt, int range, int matrix, uint32_t w, uint32_t h, uint32_t pitch,
                            uint8_t* frame, int16_t* y, int16_t* u, int16_t* v, int device) {
  uint64_t bytes = 0;
  uint32_t tight = 0;
  // (a grid's y extent is at most 65535 row pairs; column offsets are ints)
  if (dir < 0 || dir > 1 || !frame || !y || !u || !v || w > (1u << 20) || h > 2 * 65535u || !color_known(range, matrix) ||
      cairo_frame_layout(fmt, w, h, pitch, &bytes, &tight) != kSuccess)
    return kInvalidArg;
  const int col = fmt_is_yuv(fmt) ? color_index(range, matrix) : 0;  // an RGB frame has no description
  if (!pitch) pitch = tight;
  int r = fail(hipSetDevice(device), "hipSetDevice");
  if (r) return r;
  const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2);
  KatBuffer df, dp;  // the frame; y | u | v, tight: w and w / 2 elements per row
  if ((r = df.alloc(bytes)) || (r = dp.alloc((ny + 2 * nc) * 2)) || (r = df.upload(frame, bytes))) return r;
  PlaneSet p;
  p.y = dp.as<int16_t>(), p.u = p.y + ny, p.v = p.u + nc;
  if (dir == 0) {
    ConvertFmtArgs a{};
    a.c.w = (int)w, a.c.h = (int)h, a.c.wa = (int)w, a.c.nframes = 1;
    a.c.rgb[0] = df.as<uint8_t>();
    a.c.in[0] = p;
    a.fmt[0] = (uint8_t)fmt;
    a.pitch[0] = pitch;
    a.col[0] = (uint8_t)col;
    if ((r = kat_run(launch_convert_fmt_batch(a, nullptr), "k_convert_fmt_batch")) || (r = dp.download(y, ny * 2)) ||
        (r = dp.download(u, nc * 2, ny * 2)) || (r = dp.download(v, nc * 2, (ny + nc) * 2)))
      return r;
  } else {
    if ((r = dp.upload(y, ny * 2)) || (r = dp.upload(u, nc * 2, ny * 2)) || (r = dp.upload(v, nc * 2, (ny + nc) * 2)) ||
        (r = kat_run(launch_planes_to_fmt(p, (int)w, (int)w, (int)h, fmt, pitch, df.as<uint8_t>(), col, nullptr),
                     "k_planes_to_fmt")) ||
        (r = df.download(frame, bytes)))
      return r;
  }
  return kSuccess;
}

}  // extern "C"

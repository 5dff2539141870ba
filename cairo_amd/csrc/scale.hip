// cairo_amd/csrc/scale.hip -- the scaled submit's pre-pass: downscale a device
// frame of any CAIRO_FMT_* into a tight frame of the same format at the
// context's size (include/cairo_amd.h, cairo_source).
//
// The rule is an area average in exact integers.  Per axis, S source samples
// map onto D output samples; with g = gcd(S, D), L = S / g and P = D / g,
// output sample o covers the units [o L, (o + 1) L) and source sample s the
// units [s P, (s + 1) P); the weight of s in o is the length of their overlap.
//   out = (sum_sy sum_sx wy * wx * src + (Lx Ly >> 1)) / (Lx Ly)      (floor)
// with no intermediate rounding; 255 Lx Ly < 2^31 keeps the sum in 32 bits.
//
// The kernel runs before the launch's convert kernel and writes the frame's
// staging slot, which the convert kernels then read as they read an uploaded
// host frame: they are untouched.
//
// Work split: every 8-bit plane of a frame is a set of rows of C interleaved
// channels (RGB24 / BGR24: one plane, C = 3; Y, U, V of I420: C = 1; NV12's
// chroma: C = 2).  A thread owns 4 consecutive output bytes of one plane row,
// one dword.  Their taps are a contiguous byte span of at most 9 source rows;
// the thread walks that span in 4-byte columns: the 4 x 4 horizontal weights
// of a column are computed once, from o L and s P, and every source row then
// adds its column with its vertical weight.  A column is one dword load where
// its address is 4-byte aligned and it lies inside the row, else byte loads
// of the bytes inside the row: nothing outside the source's rows is read, and
// nothing outside the tight output frame is written.  No LDS, no scratch.
// The output dword goes through strip_access.h's store_bytes<4>; the status
// values, fail() and the KAT's device buffers are hip_status.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "../../include/cairo_amd.h"
#include "hip_status.h"
#include "scale.h"
#include "strip_access.h"

namespace cairo {

namespace {

constexpr int kScaleThreads = 128;  // a workgroup spans 512 output bytes of one plane row
// Sizes are bounded so that o * L and s * P (at most lcm(S, D)) stay in 31 bits.
constexpr uint32_t kMaxSourceSide = 32768;

// Bytes j4 .. j4 + 3 of a row of `bytes` bytes as a little-endian dword; bytes
// outside the row read as 0 and are not touched.  (Not strip_access.h's
// load_bytes: a column can be cut at the row's start as well as at its end.)
__device__ __forceinline__ uint32_t load_column(const uint8_t* row, int j4, int bytes) {
  const uint8_t* p = row + j4;
  if (j4 >= 0 && j4 + 4 <= bytes && ((uintptr_t)p & 3) == 0) return *(const uint32_t*)p;
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (j4 + i >= 0 && j4 + i < bytes) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

// One plane of a frame as the kernel walks it.
struct Plane {
  const uint8_t* src;  // row 0 of the source plane
  uint8_t* dst;        // row 0 of the output plane
  uint32_t spitch, dpitch;  // bytes
  int sbytes, dbytes;  // image bytes of a source / output row
  int cx, cy;          // crop origin in samples of this plane
  int row;             // output row of this plane
};

// Strip `strip` (output bytes 4 strip .. 4 strip + 3) of row p.row of a plane
// of C interleaved channels.
template <int C>
__device__ __forceinline__ void scale_strip(const Plane& p, const ScaleFrame& f, int strip) {
  const int b0 = 4 * strip;
  if (b0 >= p.dbytes) return;
  const int n = min(4, p.dbytes - b0);
  const int lx = (int)f.lx, px = (int)f.px, ly = (int)f.ly, py = (int)f.py;
  // the 4 output bytes: sample, channel, unit range (bytes past the row's end
  // repeat the last one and are not stored)
  int ch[4], us[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int b = b0 + min(k, n - 1);
    const int o = b / C;
    ch[k] = b - o * C;
    us[k] = o * lx;
  }
  // source samples [sa, sb) of the crop, as row bytes [ja, jb)
  const int sa = us[0] / px, sb = (us[3] + lx + px - 1) / px;
  const int ja = (p.cx + sa) * C, jb = (p.cx + sb) * C;
  // source rows [ya, yb) of the crop
  const int uy = p.row * ly;
  const int ya = uy / py, yb = (uy + ly + py - 1) / py;
  const uint8_t* row0 = p.src + (size_t)(p.cy + ya) * p.spitch;
  uint32_t acc[4] = {0, 0, 0, 0};
  // columns start where row ya's address is a multiple of 4 (every row's, when the pitch is one)
  for (int j4 = ja - (int)((uintptr_t)(row0 + ja) & 3); j4 < jb; j4 += 4) {
    int w[4][4];  // w[i][k]: weight of the column's byte i in output byte k
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = max(j4 + i, 0);  // (a byte before the row is not read)
      const int s = j / C;
      const int c = j - s * C;
      const int ss = (s - p.cx) * px, se = ss + px;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int o = max(min(se, us[k] + lx) - max(ss, us[k]), 0);
        w[i][k] = (C == 1 || c == ch[k]) ? o : 0;
      }
    }
    const uint8_t* row = row0;
    for (int y = ya; y < yb; y++, row += p.spitch) {
      const int wy = min((y + 1) * py, uy + ly) - max(y * py, uy);
      const uint32_t v = load_column(row, j4, p.sbytes);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t h = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) h += (uint32_t)w[i][k] * ((v >> (8 * i)) & 255u);
        acc[k] += (uint32_t)wy * h;
      }
    }
  }
  // (acc + (N >> 1)) / N, N = lx * ly: the host's floor(2^32 / N) gives the
  // quotient or one less (the numerator is below 2^31)
  const uint32_t nn = f.lx * f.ly;
  uint32_t out[1] = {0};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t num = acc[k] + (nn >> 1);
    uint32_t q = __umulhi(num, f.recip);
    uint32_t r = num - q * nn;
    if (r >= nn) q++, r -= nn;
    if (r >= nn) q++;
    out[0] |= (q & 255u) << (8 * k);
  }
  store_bytes<4>(p.dst + (size_t)p.row * p.dpitch + b0, n, out);
}

// grid: x strips of a row, y rows of the frame's planes one after the other
// (at most 2 dh: I420's Y, U and V), z scaled frame of the launch.
__global__ __launch_bounds__(kScaleThreads) void k_scale_batch(ScaleArgs a) {
  const ScaleFrame& f = a.f[blockIdx.z];
  const int strip = blockIdx.x * kScaleThreads + threadIdx.x;
  const int dw = a.dw, dh = a.dh;
  int row = blockIdx.y;  // uniform over the workgroup, as is the format
  Plane p;
  p.cx = (int)f.cx, p.cy = (int)f.cy;
  if (f.fmt == CAIRO_FMT_RGB24 || f.fmt == CAIRO_FMT_BGR24) {
    if (row >= dh) return;
    p.src = f.src, p.dst = f.dst, p.spitch = f.pitch, p.dpitch = 3 * dw;
    p.sbytes = 3 * (int)f.sw, p.dbytes = 3 * dw, p.row = row;
    scale_strip<3>(p, f, strip);
    return;
  }
  if (row < dh) {  // Y
    p.src = f.src, p.dst = f.dst, p.spitch = f.pitch, p.dpitch = dw;
    p.sbytes = (int)f.sw, p.dbytes = dw, p.row = row;
    scale_strip<1>(p, f, strip);
    return;
  }
  row -= dh;
  const uint8_t* schroma = f.src + (size_t)f.pitch * f.sh;
  uint8_t* dchroma = f.dst + (size_t)dw * dh;
  p.cx >>= 1, p.cy >>= 1;
  if (f.fmt == CAIRO_FMT_NV12) {  // U and V interleaved: two planes with sample stride 2
    if (row >= dh / 2) return;
    p.src = schroma, p.dst = dchroma, p.spitch = f.pitch, p.dpitch = dw;
    p.sbytes = (int)f.sw, p.dbytes = dw, p.row = row;
    scale_strip<2>(p, f, strip);
    return;
  }
  if (row >= dh) return;
  const int v = row >= dh / 2;  // I420: U, then V
  p.spitch = f.pitch >> 1, p.dpitch = dw >> 1;
  p.src = schroma + (v ? (size_t)p.spitch * (f.sh >> 1) : 0);
  p.dst = dchroma + (v ? (size_t)(dw >> 1) * (dh >> 1) : 0);
  p.sbytes = (int)f.sw >> 1, p.dbytes = dw >> 1, p.row = row - (v ? dh / 2 : 0);
  scale_strip<1>(p, f, strip);
}

uint32_t gcd32(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t t = a % b;
    a = b, b = t;
  }
  return a;
}

}  // namespace

int scale_plan(int fmt, uint32_t pitch, const cairo_source* src, uint32_t dw, uint32_t dh, const uint8_t* frame,
               uint8_t* dst, ScaleFrame* out) {
  if (!src || src->reserved[0] || src->reserved[1]) return kInvalidArg;
  uint32_t tight = 0;
  // The kernel walks planes of equally interleaved bytes: packed 4:2:2 (YUY2,
  // UYVY) and 16-bit samples (P010) are not scaled.
  if (fmt > CAIRO_FMT_NV12) return kInvalidArg;
  // format, even non-zero sizes, pitch against the source's width
  if (cairo_frame_layout(fmt, src->width, src->height, pitch, nullptr, &tight) != kSuccess ||
      cairo_frame_layout(fmt, dw, dh, 0, nullptr, nullptr) != kSuccess)
    return kInvalidArg;
  if (src->width > kMaxSourceSide || src->height > kMaxSourceSide) return kInvalidArg;
  uint32_t cx = src->crop_x, cy = src->crop_y, cw = src->crop_w, chh = src->crop_h;
  if (!cw) {  // the whole frame
    if (cx || cy || chh) return kInvalidArg;
    cw = src->width, chh = src->height;
  }
  if (!chh || ((cx | cy | cw | chh) & 1)) return kInvalidArg;
  if ((uint64_t)cx + cw > src->width || (uint64_t)cy + chh > src->height) return kInvalidArg;
  if (dw > cw || dh > chh || (uint64_t)cw > 8ull * dw || (uint64_t)chh > 8ull * dh) return kInvalidArg;
  const uint32_t gx = gcd32(cw, dw), gy = gcd32(chh, dh);
  const uint64_t n = (uint64_t)(cw / gx) * (chh / gy);
  if (255ull * n >= (1ull << 31)) return kInvalidArg;
  if (out) {
    out->src = frame, out->dst = dst;
    out->pitch = pitch ? pitch : tight;
    out->sw = src->width, out->sh = src->height;
    out->cx = cx, out->cy = cy;
    out->lx = cw / gx, out->px = dw / gx, out->ly = chh / gy, out->py = dh / gy;
    const uint64_t m = (1ull << 32) / n;
    out->recip = m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
    out->fmt = (uint32_t)fmt;
    out->reserved = 0;
  }
  return kSuccess;
}

hipError_t launch_scale_batch(const ScaleArgs& a, hipStream_t s) {
  if (a.nframes < 1 || a.nframes > kScaleFrames || a.dw < 2 || a.dh < 2 || 2 * a.dh > 65535) return hipErrorInvalidValue;
  const int strips = (3 * a.dw + 3) / 4;  // of the widest plane row (RGB)
  hipLaunchKernelGGL(k_scale_batch, dim3((strips + kScaleThreads - 1) / kScaleThreads, 2 * a.dh, a.nframes),
                     dim3(kScaleThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace cairo

using namespace cairo;

extern "C" {

int cairo_source_size(void) { return (int)sizeof(cairo_source); }

int cairo_scale_check(int fmt, uint32_t pitch, const cairo_source* src, uint32_t dst_w, uint32_t dst_h) {
  return scale_plan(fmt, pitch, src, dst_w, dst_h, nullptr, nullptr, nullptr);
}

int cairo_kat_scale(int fmt, uint32_t pitch, const cairo_source* src, const uint8_t* frame, uint32_t dst_w,
                    uint32_t dst_h, uint8_t* out, int device) {
  uint64_t sbytes = 0, dbytes = 0;
  if (!frame || !out || 2ull * dst_h > 65535 || cairo_scale_check(fmt, pitch, src, dst_w, dst_h) != kSuccess ||
      cairo_frame_layout(fmt, src->width, src->height, pitch, &sbytes, nullptr) != kSuccess ||
      cairo_frame_layout(fmt, dst_w, dst_h, 0, &dbytes, nullptr) != kSuccess)
    return kInvalidArg;
  int r = fail(hipSetDevice(device), "hipSetDevice");
  if (r) return r;
  const size_t mis = (uintptr_t)frame & 3;  // the device copy keeps the source's address modulo 4
  dbytes += CAIRO_KAT_SCALE_GUARD;
  KatBuffer ds, dd;
  if ((r = ds.alloc(sbytes, mis)) || (r = dd.alloc(dbytes))) return r;
  std::unique_ptr<ScaleArgs> a(new ScaleArgs());
  a->dw = (int)dst_w, a->dh = (int)dst_h, a->nframes = 1;
  (void)scale_plan(fmt, pitch, src, dst_w, dst_h, ds.as<uint8_t>(), dd.as<uint8_t>(), &a->f[0]);
  if ((r = ds.upload(frame, sbytes)) || (r = dd.upload(out, dbytes)) ||
      (r = kat_run(launch_scale_batch(*a, nullptr), "k_scale_batch")) || (r = dd.download(out, dbytes)))
    return r;
  return kSuccess;
}

}  // extern "C"

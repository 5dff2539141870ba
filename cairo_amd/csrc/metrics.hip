// cairo_amd/csrc/metrics.hip -- per-frame distortion of the encode path: SSE
// and SSIM of a frame's source planes against its kept deblocked
// reconstruction (include/cairo_amd.h cairo_frame_metrics has the
// definitions).
//
// Two kernels per launch of the engine, however many frames it holds:
//   k_metrics_tiles   grid = tiles of all three planes x frames.  A workgroup
//     reduces one tile of 128 x 64 samples: a thread reads 8 columns x 4 rows
//     of both sides (one 16-byte plane load per row and side where the row is
//     aligned), clamps them to the 8-bit samples, adds the squared errors and
//     leaves the sums of its two 4x4 blocks in LDS; then a thread per window
//     adds four blocks' sums and divides.  Wave reductions (shuffles), then
//     wave 0..3 in order: one MetricsPartial per tile.
//   k_metrics_finish  one workgroup per frame, one wave per plane: lane l adds
//     a contiguous run of the plane's partials in index order, the lanes are
//     combined by a butterfly, and lane 0 writes the plane's totals into the
//     frame's result (mapped pinned host memory inside a context).
// No floating-point atomics and no order that depends on timing: the same
// input gives the same bits.  No fast-math flag: the fp64 division is IEEE.
// The plane loads are strip_access.h's load_i16<8>, the clamp pixel_common.h's;
// the status values, fail() and the KAT's device buffers are hip_status.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_status.h"
#include "metrics.h"
#include "pixel_common.h"
#include "strip_access.h"

namespace cairo {

namespace {

constexpr int kMetThreads = 256;
constexpr int kBlocksX = kMetTileW / 4, kBlocksY = kMetTileH / 4;  // 32 x 16 blocks a tile owns
constexpr int kUnitsX = kBlocksX / 2 + 1;  // units of 2 blocks per row, the last one holds the halo column
constexpr int kUnitsY = kBlocksY + 1;      // block rows, the last one is the halo row
constexpr int kSsimC1 = 416, kSsimC2 = 235963;

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += (uint64_t)__shfl_xor((long long)v, m, 64);
  return v;
}
// a + b == b + a bit for bit, so every lane of the butterfly holds the same sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ const int16_t* pick_plane(const PlaneSet& s, int p) {
  return p == 0 ? s.y : (p == 1 ? s.u : s.v);
}

template <bool SSIM>
__global__ __launch_bounds__(kMetThreads) void k_metrics_tiles(MetricsArgs m) {
  // {s1, s2, ss, s12} of every 4x4 block of the tile and its halo (the odd
  // block of the last unit is never read)
  __shared__ uint4 blk[SSIM ? kUnitsY : 1][SSIM ? 2 * kUnitsX : 1];
  __shared__ uint64_t w_sse[kMetThreads / 64];
  __shared__ double w_ssim[kMetThreads / 64];
  __shared__ uint32_t w_cnt[kMetThreads / 64];

  const int f = blockIdx.y, tid = threadIdx.x;
  const int nl = metrics_tiles(m.w, m.h), nc = metrics_tiles(m.w >> 1, m.h >> 1);
  int t = blockIdx.x, plane = 0;
  if (t >= nl) {
    t -= nl, plane = 1;
    if (t >= nc) t -= nc, plane = 2;
  }
  const int pw = plane ? m.w >> 1 : m.w, ph = plane ? m.h >> 1 : m.h;
  const int pitch = plane ? m.pitch >> 1 : m.pitch, off = plane ? 0 : 16;
  const int tx = metrics_tiles_x(pw);
  const int x0 = (t % tx) * kMetTileW, y0 = (t / tx) * kMetTileH;
  const int16_t* pa = pick_plane(m.a[f], plane);
  const int16_t* pb = pick_plane(m.b[f], plane);

  uint32_t sse = 0;  // at most 2 units x 32 samples x 255^2 per thread
  constexpr int kUx = SSIM ? kUnitsX : kUnitsX - 1, kUy = SSIM ? kUnitsY : kUnitsY - 1;
  for (int i = tid; i < kUx * kUy; i += kMetThreads) {
    const int ux = i % kUx, uy = i / kUx;
    const int x = x0 + 8 * ux, y = y0 + 4 * uy;
    const bool own = ux < kBlocksX / 2 && uy < kBlocksY;  // not the halo
    const int n = min(8, pw - x);
    uint32_t s1[2] = {}, s2[2] = {}, ss[2] = {}, s12[2] = {};
    if (n > 0) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (y + r >= ph) break;
        const size_t o = (size_t)(y + r) * pitch + x;
        int va[8], vb[8];
        load_i16<8>(pa + o, n, va);
        load_i16<8>(pb + o, n, vb);
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int a = k < n ? clamp8(va[k] - off) : 0, b = k < n ? clamp8(vb[k] - off) : 0;
          const int d = a - b;
          if (own) sse += (uint32_t)(d * d);
          if constexpr (SSIM) {
            s1[k >> 2] += a, s2[k >> 2] += b;
            ss[k >> 2] += a * a + b * b;
            s12[k >> 2] += a * b;
          }
        }
      }
    }
    if constexpr (SSIM) {
      blk[uy][2 * ux] = make_uint4(s1[0], s2[0], ss[0], s12[0]);
      blk[uy][2 * ux + 1] = make_uint4(s1[1], s2[1], ss[1], s12[1]);
    }
  }
  double ssim = 0;
  uint32_t cnt = 0;
  if constexpr (SSIM) {
    __syncthreads();
    // windows of complete blocks only: a block cut by the plane's edge holds
    // partial sums, and no window below reaches it
    const int bw = pw >> 2, bh = ph >> 2, bx0 = x0 >> 2, by0 = y0 >> 2;
    for (int i = tid; i < kBlocksX * kBlocksY; i += kMetThreads) {
      const int lx = i % kBlocksX, ly = i / kBlocksX;
      if (bx0 + lx >= bw - 1 || by0 + ly >= bh - 1) continue;
      const uint4 q0 = blk[ly][lx], q1 = blk[ly][lx + 1], q2 = blk[ly + 1][lx], q3 = blk[ly + 1][lx + 1];
      const int64_t a1 = q0.x + q1.x + q2.x + q3.x, a2 = q0.y + q1.y + q2.y + q3.y;
      const int64_t qs = q0.z + q1.z + q2.z + q3.z, q12 = q0.w + q1.w + q2.w + q3.w;
      const int64_t vars = 64 * qs - a1 * a1 - a2 * a2, covar = 64 * q12 - a1 * a2;
      const int64_t num = (2 * a1 * a2 + kSsimC1) * (2 * covar + kSsimC2);
      const int64_t den = (a1 * a1 + a2 * a2 + kSsimC1) * (vars + kSsimC2);
      ssim += (double)num / (double)den;
      cnt++;
    }
  }
  const uint64_t t_sse = wave_sum((uint64_t)sse);
  const double t_ssim = SSIM ? wave_sum(ssim) : 0.0;
  const uint32_t t_cnt = SSIM ? (uint32_t)wave_sum((uint64_t)cnt) : 0u;
  if ((tid & 63) == 0) w_sse[tid >> 6] = t_sse, w_ssim[tid >> 6] = t_ssim, w_cnt[tid >> 6] = t_cnt;
  __syncthreads();
  if (tid == 0) {
    MetricsPartial p;
    p.sse = 0, p.ssim = 0, p.windows = 0;
    for (int k = 0; k < kMetThreads / 64; k++) p.sse += w_sse[k], p.ssim += w_ssim[k], p.windows += w_cnt[k];
    m.part[((size_t)m.slot[f] * 3 + plane) * nl + t] = p;
  }
}

__global__ __launch_bounds__(192) void k_metrics_finish(MetricsArgs m) {
  const int f = blockIdx.x, plane = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nl = metrics_tiles(m.w, m.h);
  const int pw = plane ? m.w >> 1 : m.w, ph = plane ? m.h >> 1 : m.h;
  const int n = metrics_tiles(pw, ph), run = (n + 63) / 64;
  const MetricsPartial* p = m.part + ((size_t)m.slot[f] * 3 + plane) * nl;
  uint64_t sse = 0, windows = 0;
  double ssim = 0;
  for (int k = lane * run; k < min(n, (lane + 1) * run); k++) sse += p[k].sse, ssim += p[k].ssim, windows += p[k].windows;
  sse = wave_sum(sse), ssim = wave_sum(ssim), windows = wave_sum(windows);
  cairo_frame_metrics* o = m.out + m.slot[f];
  if (lane == 0) {
    o->sse[plane] = (m.flags & CAIRO_METRIC_SSE) ? sse : 0;
    o->ssim_sum[plane] = ssim;
    o->ssim_windows[plane] = windows;
    o->samples[plane] = (uint64_t)pw * ph;
  }
  if (threadIdx.x == 0) {
    o->flags = (uint32_t)(m.flags & (CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM));
    o->width = (uint32_t)m.w, o->height = (uint32_t)m.h;
    o->reserved = 0;
  }
}

}  // namespace

hipError_t launch_metrics(const MetricsArgs& m, hipStream_t s) {
  if (m.nframes < 1 || !(m.flags & (CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM))) return hipSuccess;
  const dim3 grid(metrics_tiles(m.w, m.h) + 2 * metrics_tiles(m.w >> 1, m.h >> 1), m.nframes);
  if (m.flags & CAIRO_METRIC_SSIM)
    hipLaunchKernelGGL(k_metrics_tiles<true>, grid, dim3(kMetThreads), 0, s, m);
  else
    hipLaunchKernelGGL(k_metrics_tiles<false>, grid, dim3(kMetThreads), 0, s, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_metrics_finish, dim3(m.nframes), dim3(192), 0, s, m);
  return hipGetLastError();
}

}  // namespace cairo

using namespace cairo;

extern "C" {

int cairo_frame_metrics_size(void) { return (int)sizeof(cairo_frame_metrics); }

int cairo_kat_metrics(uint32_t w, uint32_t h, uint32_t pitch_elems, const int16_t* a_y, const int16_t* a_u,
                      const int16_t* a_v, const int16_t* b_y, const int16_t* b_u, const int16_t* b_v,
                      cairo_frame_metrics* out, int device) {
  if (!a_y || !a_u || !a_v || !b_y || !b_u || !b_v || !out || !w || !h || (w & 1) || (h & 1) || w > (1u << 15) ||
      h > (1u << 15) || pitch_elems < w || (pitch_elems & 1) || pitch_elems > (1u << 16))
    return kInvalidArg;
  int r = fail(hipSetDevice(device), "hipSetDevice");
  if (r) return r;
  const size_t ny = (size_t)pitch_elems * h, nc = (size_t)(pitch_elems / 2) * (h / 2), ne = ny + 2 * nc;
  KatBuffer dp, part, dout;  // dp: a's y | u | v, then b's
  if ((r = dp.alloc(2 * ne * 2)) || (r = part.alloc((size_t)3 * metrics_tiles((int)w, (int)h) * sizeof(MetricsPartial))) ||
      (r = dout.alloc(sizeof(*out))))
    return r;
  MetricsArgs m{};
  m.w = (int)w, m.h = (int)h, m.pitch = (int)pitch_elems, m.nframes = 1;
  m.flags = CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM;
  m.a[0].y = dp.as<int16_t>(), m.a[0].u = m.a[0].y + ny, m.a[0].v = m.a[0].u + nc;
  m.b[0].y = m.a[0].y + ne, m.b[0].u = m.b[0].y + ny, m.b[0].v = m.b[0].u + nc;
  m.slot[0] = 0;
  m.part = part.as<MetricsPartial>();
  m.out = dout.as<cairo_frame_metrics>();
  if ((r = dp.upload(a_y, ny * 2)) || (r = dp.upload(a_u, nc * 2, ny * 2)) || (r = dp.upload(a_v, nc * 2, (ny + nc) * 2)) ||
      (r = dp.upload(b_y, ny * 2, ne * 2)) || (r = dp.upload(b_u, nc * 2, (ne + ny) * 2)) ||
      (r = dp.upload(b_v, nc * 2, (ne + ny + nc) * 2)) || (r = kat_run(launch_metrics(m, nullptr), "k_metrics")) ||
      (r = dout.download(out, sizeof(*out))))
    return r;
  return kSuccess;
}

}  // extern "C"

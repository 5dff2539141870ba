// cairo_amd/csrc/metrics.h -- launch interface of the per-frame distortion
// kernels (metrics.hip): SSE and SSIM of a frame's source planes against its
// kept deblocked reconstruction (include/cairo_amd.h, cairo_frame_metrics).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cairo_amd.h"
#include "kernels.h"

namespace cairo {

// A tile is what one workgroup reduces: 128 x 64 samples of one plane, i.e.
// 32 x 16 blocks of 4 x 4, plus one block column and one block row of halo
// for the windows that start in its last column / row.
constexpr int kMetTileW = 128, kMetTileH = 64;

// One workgroup's partial sums of one tile.
struct MetricsPartial {
  uint64_t sse;
  double ssim;       // sum of the window values of the tile, in a fixed order
  uint64_t windows;  // windows the tile owns
};

// Tiles of the luma plane of a w x h frame: the stride of a frame's partials
// per plane (the chroma planes use fewer).
__host__ __device__ inline int metrics_tiles_x(int w) { return (w + kMetTileW - 1) / kMetTileW; }
__host__ __device__ inline int metrics_tiles(int w, int h) {
  return metrics_tiles_x(w) * ((h + kMetTileH - 1) / kMetTileH);
}

// One launch: every frame of a batch that has metrics on.
struct MetricsArgs {
  int w, h;       // nominal frame size: the luma plane compared; chroma is (w/2) x (h/2)
  int pitch;      // luma plane pitch in elements (chroma: pitch / 2)
  int nframes;
  int flags;      // CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM
  PlaneSet a[kMaxBatch];  // source planes
  PlaneSet b[kMaxBatch];  // reconstruction
  int slot[kMaxBatch];    // the frame's staging slot: its partials and its result
  MetricsPartial* part;   // [slot][3][metrics_tiles(w, h)]
  cairo_frame_metrics* out;  // [slot], device-visible (mapped pinned host memory, or device memory)
};

// k_metrics_tiles over tiles x planes x frames, then k_metrics_finish, which
// adds each plane's partials in index order and writes the frame's result.
hipError_t launch_metrics(const MetricsArgs& m, hipStream_t s);

}  // namespace cairo

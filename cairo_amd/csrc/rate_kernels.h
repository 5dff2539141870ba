// cairo_amd/csrc/rate_kernels.h -- launch interface of the target-bitrate
// kernels (rate.hip; the rules they run are rate.h's).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "rate.h"

namespace cairo {

// Workgroups a frame's feed words are split over (k_rate_observe), and the
// partial counts per staging slot.
constexpr int kRateBlocks = 32;

// A staging slot's record, in device memory and in mapped pinned host memory:
// what k_rate_finish saw of the slot's frame, and what k_rate_decide chose for
// its launch.
struct RateSlot {
  uint64_t nbits, ones;
  uint32_t overflow, quality;
  int64_t aim, debt;
};

struct RateObserveArgs {
  int nframes;
  int slot[kMaxBatch];       // staging slot of frame j
  const uint32_t* feed;      // per slot: feed words (device)
  size_t feed_stride;        // words per slot; a frame's words never exceed it
  const uint32_t* hdr;       // per slot: kFeedHdrWords (bits lo, hi, overflow, ...)
  uint32_t* part;            // per slot: kRateBlocks partial counts
  RateSlot* dev;             // per slot
  RateSlot* host;            // per slot, mapped pinned host memory (nullptr: none)
};

struct RateDecideArgs {
  cairo_rate cfg;
  cairo_rate_state* state;   // device
  const RateSlot* obs;       // per slot (device): the records k_rate_finish wrote
  RateSlot* host;            // per slot, mapped pinned host memory
  FrameArgs* fa;             // this launch's frame views (device)
  int n_obs, n_new;
  int oslot[kMaxBatch];      // slots of the launch before the last (n_obs of them)
  int nslot[kMaxBatch];      // slots of this launch (n_new)
};

// k_rate_observe over (kRateBlocks, frames), then k_rate_finish per frame.
hipError_t launch_rate_observe(const RateObserveArgs& a, hipStream_t s);
// k_rate_decide: one wave.
hipError_t launch_rate_decide(const RateDecideArgs& a, hipStream_t s);

}  // namespace cairo

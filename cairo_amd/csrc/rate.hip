// cairo_amd/csrc/rate.hip -- the target-bitrate kernels and the
// host entry points of the same rules (rate.h).
//
//   k_rate_observe  counts the set bits of each frame's device feed over bits
//                   [0, N): a frame's words are split over kRateBlocks
//                   workgroups, 16-byte loads, a wave reduction, one partial
//                   count per workgroup (no atomics: nothing to zero, and the
//                   same counts in the same order every time)
//   k_rate_finish   adds a frame's partials and writes {N, ones, overflow} to
//                   its slot's record, on the device and in mapped host memory
//   k_rate_decide   one wave: sums the observed launch's frames, runs the
//                   control law on the device-resident state, and stores the
//                   quality into the views of the launch about to run
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/cairo_amd.h"
#include "hip_status.h"
#include "precode.h"
#include "rate_kernels.h"

namespace cairo {

namespace {

constexpr int kRateThreads = 256;
static_assert(kMaxBatch <= 64 && kRateBlocks <= 64, "k_rate_decide and k_rate_finish are one wave");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0
}
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// The frame's feed as the observer may read it: its bit count, 0 for a frame
// whose feed is not valid (overflow, or a count no feed slot can hold).
__device__ __forceinline__ uint64_t observed_bits(const RateObserveArgs& a, int slot, uint32_t* overflow) {
  const uint32_t* h = a.hdr + (size_t)slot * kFeedHdrWords;
  const uint64_t nbits = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
  *overflow = h[2] != 0 || nbits > (uint64_t)a.feed_stride * 32 || nbits >= ((uint64_t)1 << 32);
  return *overflow ? 0 : nbits;
}

__global__ __launch_bounds__(kRateThreads) void k_rate_observe(const RateObserveArgs a) {
  const int slot = a.slot[blockIdx.y];
  uint32_t overflow;
  const uint64_t nbits = observed_bits(a, slot, &overflow);
  const uint32_t* p = a.feed + (size_t)slot * a.feed_stride;
  // whole words [0, full): `head` words up to the first 16-byte boundary, then
  // nvec 16-byte loads shared by the frame's workgroups, then fewer than four
  // words; the bits of word `full` below N are counted under a mask
  const size_t full = (size_t)(nbits >> 5);
  size_t head = ((16 - ((uintptr_t)p & 15)) & 15) / 4;
  if (head > full) head = full;
  const size_t nvec = (full - head) / 4, tail = head + nvec * 4;
  const uint4* v = (const uint4*)(p + head);
  uint32_t cnt = 0;
  for (size_t i = (size_t)blockIdx.x * kRateThreads + threadIdx.x; i < nvec; i += (size_t)gridDim.x * kRateThreads) {
    const uint4 w = v[i];
    cnt += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
  }
  if (blockIdx.x == 0) {
    const size_t t = threadIdx.x;
    if (t < head)
      cnt += __popc(p[t]);
    else if (t - head < full - tail)
      cnt += __popc(p[tail + (t - head)]);
    if (t == kRateThreads - 1 && (nbits & 31)) cnt += __popc(p[full] & ((1u << (nbits & 31)) - 1u));
  }
  __shared__ uint32_t wsum[kRateThreads / 64];
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int k = 0; k < kRateThreads / 64; k++) s += wsum[k];
    a.part[(size_t)slot * kRateBlocks + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void k_rate_finish(const RateObserveArgs a) {
  const int slot = a.slot[blockIdx.x];
  const int lane = threadIdx.x;
  const uint32_t ones = wave_sum(lane < kRateBlocks ? a.part[(size_t)slot * kRateBlocks + lane] : 0u);
  if (lane == 0) {
    uint32_t overflow;
    const uint64_t nbits = observed_bits(a, slot, &overflow);
    RateSlot* d = a.dev + slot;
    d->nbits = nbits, d->ones = ones, d->overflow = overflow;
    if (a.host) {
      RateSlot* h = a.host + slot;
      h->nbits = nbits, h->ones = ones, h->overflow = overflow;
    }
  }
}

__global__ __launch_bounds__(64) void k_rate_decide(const RateDecideArgs a) {
  const int lane = threadIdx.x;
  long long bits = 0;
  if (lane < a.n_obs) {
    const RateSlot* o = a.obs + a.oslot[lane];
    bits = rate_frame_bits(o->nbits, o->ones, o->overflow, a.cfg.target_bits);
  }
  bits = wave_sum(bits);
  unsigned q = 0;
  long long aim = 0, debt = 0;
  if (lane == 0) {
    cairo_rate_state s = *a.state;
    q = rate_step(&s, &a.cfg, a.n_new, bits);
    *a.state = s;
    aim = s.p_aim, debt = s.debt;
  }
  q = __shfl(q, 0, 64);
  aim = __shfl(aim, 0, 64);
  debt = __shfl(debt, 0, 64);
  if (lane < a.n_new) {  // one lane per frame of the launch
    a.fa[lane].quality = (int)q;
    RateSlot* h = a.host + a.nslot[lane];
    h->quality = q, h->aim = aim, h->debt = debt;
  }
}

}  // namespace

hipError_t launch_rate_observe(const RateObserveArgs& a, hipStream_t s) {
  if (a.nframes < 1) return hipSuccess;
  hipLaunchKernelGGL(k_rate_observe, dim3(kRateBlocks, a.nframes), dim3(kRateThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rate_finish, dim3(a.nframes), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rate_decide(const RateDecideArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rate_decide, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cairo

using namespace cairo;

extern "C" {

int cairo_rate_size(void) { return (int)sizeof(cairo_rate); }
int cairo_rate_state_size(void) { return (int)sizeof(cairo_rate_state); }
int cairo_rate_info_size(void) { return (int)sizeof(cairo_rate_info); }

int64_t cairo_rate_estimate(uint64_t nbits, uint64_t zeros) {
  if (nbits >= ((uint64_t)1 << 32) || zeros > nbits) return -1;
  return rate_estimate(nbits, zeros);
}

int cairo_rate_init(cairo_rate_state* state, const cairo_rate* cfg) {
  if (!state || !cfg || !rate_cfg_ok(cfg)) return kInvalidArg;
  rate_init(state);
  return kSuccess;
}

int cairo_rate_step(cairo_rate_state* state, const cairo_rate* cfg, int n_new, int64_t obs_sum, uint32_t* q) {
  if (!state || !cfg || !q || !rate_cfg_ok(cfg) || n_new < 1 || n_new > 65535 || obs_sum < 0 || obs_sum > kRateMaxObs)
    return kInvalidArg;
  *q = rate_step(state, cfg, n_new, obs_sum);
  return kSuccess;
}

int cairo_kat_rate_observe(const uint32_t* words, uint64_t total_words, uint64_t base_words, uint64_t stride_words,
                           const uint64_t* nbits, int count, cairo_rate_info* out, int device) {
  if (!words || !total_words || !nbits || !out || count < 1 || count > kMaxBatch || base_words > total_words)
    return kInvalidArg;
  for (int j = 0; j < count; j++) {
    const uint64_t w = (nbits[j] + 31) / 32;
    if (nbits[j] >= ((uint64_t)1 << 32) || w > stride_words || stride_words > total_words ||
        base_words + (uint64_t)j * stride_words + w > total_words)
      return kInvalidArg;
  }
  if (fail(hipSetDevice(device), "hipSetDevice")) return kHardwareFail;
  KatBuffer dw, dh, dp, ds;
  std::vector<uint32_t> hdr((size_t)count * kFeedHdrWords, 0);
  for (int j = 0; j < count; j++) {
    hdr[(size_t)j * kFeedHdrWords] = (uint32_t)nbits[j];
    hdr[(size_t)j * kFeedHdrWords + 1] = (uint32_t)(nbits[j] >> 32);
  }
  RateObserveArgs a;
  memset(&a, 0, sizeof(a));
  int r;
  if ((r = dw.alloc(total_words * 4)) || (r = dh.alloc(hdr.size() * 4)) ||
      (r = dp.alloc((size_t)count * kRateBlocks * 4)) || (r = ds.alloc((size_t)count * sizeof(RateSlot))) ||
      (r = dw.upload(words, total_words * 4)) || (r = dh.upload(hdr.data(), hdr.size() * 4)))
    return r;
  a.nframes = count;
  for (int j = 0; j < count; j++) a.slot[j] = j;
  a.feed = dw.as<uint32_t>() + base_words;
  a.feed_stride = (size_t)stride_words;
  a.hdr = dh.as<uint32_t>();
  a.part = dp.as<uint32_t>();
  a.dev = ds.as<RateSlot>();
  a.host = nullptr;
  std::vector<RateSlot> got((size_t)count);
  if ((r = kat_run(launch_rate_observe(a, nullptr), "k_rate_observe")) ||
      (r = ds.download(got.data(), got.size() * sizeof(RateSlot))))
    return r;
  for (int j = 0; j < count; j++) {
    memset(&out[j], 0, sizeof(out[j]));
    out[j].overflow = got[(size_t)j].overflow;
    out[j].feed_bits = got[(size_t)j].nbits;
    out[j].ones = got[(size_t)j].ones;
    out[j].est_bits = got[(size_t)j].overflow ? 0 : rate_frame_bits(got[(size_t)j].nbits, got[(size_t)j].ones, 0, 1);
  }
  return kSuccess;
}

}  // extern "C"

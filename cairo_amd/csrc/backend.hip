// cairo_amd/csrc/backend.hip -- device context and frame orchestration.
//
// One context = one encoder's device state in HBM (DESIGN.md "Data layout"):
//   ring          R contiguous plane sets (reconstruction slots, frame n -> n % R)
//   staging slots (64 for pipelined callers, 2 for the synchronous drop-in
//     encoder/decoder), one per frame in flight, each with its own
//     source planes (convert output), output_cache planes (coefficients),
//     block table, inter-search records, granules, RGB staging and pinned
//     host buffers for the table + coefficients; with cairo_ctx_set_metrics
//     also a plane set that keeps the frame's deblocked reconstruction
//   sync          batch flags (zeroed per launch)
// Frames are submitted into a batch (up to batch_max, cairo_default_batch)
// that is launched when full or when a caller waits on one of its frames:
//   memset(sync) -> convert (all frames) -> engine (inter search, row coding,
//   deblock, pipelined across the frames)
// and on the copy stream, after the engine: D2H of each frame's table and
// coefficients into its pinned staging (the host entropy stage reads those
// while the GPU runs the next batch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/cairo_amd.h"
#include "ctx_internal.h"
#include "hip_status.h"
#include "kernels.h"
#include "metrics.h"
#include "precode.h"
#include "rate_kernels.h"
#include "scale.h"
#include "tensor.h"

using namespace cairo;

namespace {

// staging slots (frames in flight): three 32-frame batches, so that the host
// entropy of one batch overlaps the GPU work of the next two
constexpr int kDefaultStages = 96;
constexpr int kMaxStages = 256;
constexpr int kLaunchSlots = 64;    // per-launch host records (frame views, timing events), reused round-robin
constexpr int kTimed = 3;        // timed kernels: convert, (inter: fused), engine
// Frames per launch by default, from measured sweeps (DESIGN.md §4.2,
// tools/sweep_bench.sh).  With the pools shared between consecutive launches
// (k_engine next_task) a batch's tail no longer idles half the workers, so
// larger batches pay: 32 up to about 1080p (1080p: 2981 at 12, 3460 at 24,
// 3551 at 32 Mpix/s); at 4K 28 was best in round 3 (4443-4454 vs 4235 at
// 32); on the round-4 engine larger launches pay there: 32 over 28 (5838 vs
// 5808 Mpix/s, three alternating rounds, profiles/r04/batch_ab_4k.txt), and
// with the cap raised to 48: 32 / 36 / 40 / 44 -> 5820 / 5828 / 5856 / 5868
// (two rounds, profiles/r04/batch_cap_4k.txt).  But two 40-frame launches
// in flight leave only 16 of the default 96 staging slots to the host entropy
// pipeline: end to end fell to 82 % of the hot path (profiles/r04/
// bench_4k_batch40.json), so the default stays at 32 everywhere.
inline int default_batch(size_t mbs) {
  (void)mbs;
  return 32;
}
constexpr int kSyncAreas = 3;    // launch b uses area b % 3; launch b+1 reads it too
// The output_cache slots are allocated in chunks of at most this size, each
// exported with its own IPC handle (cairo_peer): an IPC import of one
// fine-grained allocation of 2 GiB or more never returned.
constexpr size_t kCoefChunkBytes = size_t(1) << 30;
// Reconstruction slots of a member of a group over several devices or
// processes: every member keeps the same layout, N * S slots (S = ceil(R / N)),
// frame m in slot (m % N) * S + (m / N) % S -- its producer's own block, a
// mirror block on every other member -- for any N <= kMaxGroup.
constexpr int kMirrorSlots = kMaxGroup > kMaxRing ? kMaxGroup : kMaxRing;

struct Stage {
  uint8_t* table = nullptr;  // pinned, mapped (k_feed_copy writes it in feed mode)
  int16_t* coef = nullptr;   // pinned, 1.5 * wa * ha
  int32_t* err = nullptr;    // pinned, mapped: the context's TimeoutInfo words after the frame
  uint8_t* table_dev = nullptr;  // device addresses of table / err
  int32_t* err_dev = nullptr;
  hipEvent_t d2h_done = nullptr;
  // The launch that converts this slot's staged host RGB: a later frame's
  // upload into the same staging buffer waits for it (rgb_read).
  hipEvent_t rgb_read = nullptr;
  bool rgb_pending = false;
  int ticket = -1;
  bool busy = false;      // submitted, not yet released
  bool launched = false;  // its batch has been launched
  bool waited = false;    // its outputs were handed to a caller (cairo_ctx_wait)
  int mflags = 0;         // cairo_ctx_set_metrics flags in force at its submit (0 for a decoded frame)
  bool rated = false;     // cairo_ctx_set_rate was on at its submit: its launch's quality is the controller's
  uint32_t index = 0, type = 0, quality = 0;
};

// Ticket t takes the stage (submit, decode_frame).
void take_stage(Stage& s, int t, uint32_t index, uint32_t type, uint32_t quality, int mflags) {
  s.busy = true, s.launched = false, s.waited = false;
  s.mflags = mflags;
  s.rated = false;
  s.ticket = t;
  s.index = index, s.type = type, s.quality = quality;
}

struct TimedBatch {
  hipEvent_t ev[kTimed + 1] = {};
  int frames = 0;
  bool pending = false;
};

// Length of the union of [start, end) intervals (ms): the time the engine
// was running at all, with the two in-flight launches overlapping.
double union_length(std::vector<std::pair<double, double>>& iv) {
  std::sort(iv.begin(), iv.end());
  double total = 0, s = 0, e = -1e300;
  for (const auto& p : iv) {
    if (p.first > e) {
      if (e > s) total += e - s;
      s = p.first;
      e = p.second;
    } else if (p.second > e) {
      e = p.second;
    }
  }
  if (e > s) total += e - s;
  return total;
}

}  // namespace

struct cairo_ctx {
  int device = 0;
  uint32_t w = 0, h = 0, wa = 0, ha = 0, wmb = 0, hmb = 0, ring = 0;
  size_t plane_elems = 0, mbs = 0, nref = 1;
  hipStream_t ks = nullptr, cs = nullptr;
  hipStream_t ks2 = nullptr;         // launches alternate between ks and ks2 (consecutive batches overlap)
  // Host RGB uploads (rgb_on_device = 0), issued at submit on a stream of
  // their own so that they overlap the launches in flight; a launch waits for
  // the last one (the stream is in order).  Made on first use; a group member
  // keeps uploading on its launch stream (its queue budget, join_group).
  hipStream_t us = nullptr;
  hipEvent_t up_last = nullptr;
  bool up_pending = false;  // an upload the next launch has not waited for
  hipEvent_t engine_done = nullptr;  // last launched batch finished (copy stream waits on it)
  hipEvent_t batch_end[kSyncAreas] = {};  // end of the launch that used sync area k (every task done)
  hipEvent_t batch_ready[kSyncAreas] = {};  // its frames converted, views and sync area set up
  hipEvent_t pre_done[kSyncAreas] = {};  // its precode's feeds written (the host copy follows on cs)
  bool host_uploads = false;  // host-RGB frames were submitted (the copy stream carries their uploads)
  // the last launch, whose remaining tasks the next launch's workers take first
  const FrameArgs* prev_fa = nullptr;
  const int32_t* prev_order[2] = {};
  const int32_t* prev_seg[2] = {};
  int32_t* prev_sync = nullptr;
  int prev_total = 0, prev_area = 0, prev_decode = 0;
  bool prev_sys = false;   // some frame of the last launch had FrameDesc::sys
  int engine_variant = 0;  // the last launch's engine: 0 plain, 1 general (cairo_ctx_engine_variant)
  int order_slope = kOrderSlope;  // of the task order tables (3N + 2 in an N-member group)
  long long batches = 0;             // launches so far
  // per-slot device buffers
  int16_t* src = nullptr;
  int16_t* coef[CAIRO_MAX_COEF_CHUNKS] = {};  // output_cache: slot s in chunk s / coef_per, at s % coef_per
  int coef_chunks = 0, coef_per = 0;
  BlockDesc *table = nullptr, *idesc = nullptr;
  uint64_t* gran = nullptr;
  uint8_t* rgb = nullptr;
  int16_t* ring_buf = nullptr;
  int ring_slots = 0;  // R; kMirrorSlots once allocated for a group over devices / processes
  uint64_t* progress = nullptr;  // [stages][hmb] tagged deblock progress of each slot's frame
  bool fresh = true;             // no frame since create / reset: the next has no predecessor
  long since_fresh = 0;          // frames since create / reset (frame_links)
  // Frame-interleaved group (cairo_ctx_join_group): member grank of gsize
  // encodes the stream's frames n = grank (mod gsize), reading the others'
  // reconstructions, output_cache and progress words in place.
  struct Peer {
    int16_t* ring = nullptr;
    int16_t* coef[CAIRO_MAX_COEF_CHUNKS] = {};
    int coef_chunks = 0, coef_per = 1;
    uint64_t* progress = nullptr;
    int stages = 0;
    bool imported = false;  // opened from another process's IPC handles
  };
  int gsize = 1, grank = 0, gbase = 0;  // gbase: ticket of the group's frame grank
  Peer gp[kMaxGroup];
  int16_t* zero = nullptr;  // a zero plane set: references before the stream start
  bool fine_grained = false;  // ring / coef / progress allocated fine-grained (cross-device sharing)
  // Outputs for the host entropy stage (cairo_ctx_set_outputs): the
  // coefficient planes (D2H per frame) and/or the GPU precode's feed bits
  // (precode.hip), written straight into mapped pinned host memory.
  int outputs = CAIRO_OUT_COEF;
  size_t feed_words = 0;          // per staging slot
  uint32_t* feed_dev = nullptr;   // [stages][feed_words]
  uint32_t* feed_hdr = nullptr;   // [stages][kFeedHdrWords]
  uint32_t* feed_scratch = nullptr;  // [stages][feed_scratch_words(mbs)]
  uint32_t* feed_host = nullptr;  // mapped pinned [stages][kFeedHdrWords + feed_words]
  hipStream_t fs = nullptr;       // synchronous coefficient fetches (a frame whose feed overflowed)
  // (The precode runs on the launch's stream, between its kernel and the
  // launch two ahead: on a stream of its own its kernels took the slots the
  // next launch's workers need, -2 to -5 % at 4K)
  bool sys = false;           // a member is another process or device: system-scope hand-offs
  int32_t *sync = nullptr;
  int32_t* sticky = nullptr;  // TimeoutInfo words (kernels.h), cleared only by zero_state
  int inject = 0;             // test hook (cairo_ctx_set_debug 16): EngineArgs::inject
  int32_t* order = nullptr;  // [kMaxBatch][kMaxBatch * hmb]: pool task order per batch size
  FrameArgs* fdesc_host = nullptr;  // pinned [kLaunchSlots][kMaxBatch]: per-frame views per launch
  FrameArgs* fdesc_host_dev = nullptr;  // its device-visible address (read by the convert kernel)
  FrameArgs* fdesc = nullptr;       // device copy
  int fdesc_next = 0;
  // the H2D copy of each fdesc_host slot: a slot is rewritten only after its
  // previous copy ran (more than kLaunchSlots launches may be queued, e.g.
  // batch 1 with 96 staging slots, and the copy waits behind earlier launches)
  hipEvent_t fdesc_done[kLaunchSlots] = {};
  bool fdesc_used[kLaunchSlots] = {};
  int32_t* trace_host = nullptr;  // diagnostic live trace (mapped), opt-in via set_debug(4)
  int32_t* trace_dev = nullptr;
  size_t sync_words = 0;
  int stages = kDefaultStages;
  std::vector<Stage> st;  // [stages]
  int next_ticket = 0;
  uint32_t epoch = 0;
  int batch_max = 16;
  // A pending frame: its FrameDesc and how the launch reads its pixels, all of
  // it written at submit (decode_frame: its one frame); flush() only reads it.
  struct Pending {
    // kStaged: a host frame, staged tight in its slot (uploaded at submit; in a
    // group at launch).  kDevice: a device frame read in place.  kScaled
    // (cairo_ctx_submit_scaled), kTensor (cairo_ctx_submit_tensor, DESIGN
    // §4.15): f.rgb is the staging slot, tight, which the launch's k_scale_batch
    // / k_tensor_pack_batch fills from `scale` / `tens` before the convert.
    // kTensorScaled (cairo_ctx_submit_tensor_scaled): the same,
    // filled by k_tensor_scale_batch from `tscale`.
    enum Kind : uint8_t { kStaged, kDevice, kScaled, kTensor, kTensorScaled };
    FrameDesc f;
    Kind kind;
    // Layout as the convert kernel reads it (CAIRO_FMT_*, row pitch in bytes):
    // a device frame's own, a staged frame's tight one.  hpitch: the pitch of a
    // host source still to upload (flush).  col: the input colour description
    // in force at submit (kernels.h color_index; 0 for an RGB frame).
    uint8_t fmt, col;
    uint32_t pitch, hpitch;
    union {
      ScaleFrame scale;
      TensorFrame tens;
      TensorScaleFrame tscale;
    };
  };
  Pending pend[kMaxBatch];
  // Colour descriptions (cairo_ctx_set_input_color / _output_color, DESIGN
  // §4.13) as kernels.h color_index values: in_col is recorded per frame at
  // submit (Pending::col), out_col is read when a frame is written as I420 /
  // NV12.  Neither is touched by cairo_ctx_reset.
  int in_col = 0, out_col = 0;
  int npend = 0;
  int last_slot = -1;  // slot of the last launched frame
  uint32_t last_epoch = 0;  // and its epoch (the tag of its inter records)
  int wg_rows = 0;
  int wg_helpers = 0;  // helpers of the launch's 2 * wg_rows workgroups (0: half)
  int max_rows = 0;  // row coders (= helpers) per launch that stay co-resident with the other in-flight launch
  bool profiling = false;
  TimedBatch tb[kLaunchSlots];
  int tb_next = 0;
  double acc_ms[kTimed] = {0, 0, 0};
  int acc_frames = 0;
  hipEvent_t t_base = nullptr;  // profiling epoch: engine intervals are measured from it
  std::vector<std::pair<double, double>> busy;  // engine [start, end) per launch, ms after t_base
  int16_t* predeblock = nullptr;  // debug: pre-deblock reconstruction of the last frame (opt-in)
  uint64_t* stamps = nullptr;     // diagnostic phase stamps (opt-in)
  uint64_t* acct = nullptr;       // diagnostic time accounting (opt-in; CAIRO_ACCT builds fill it)
  // Kept reconstructions and per-frame metrics (cairo_ctx_set_metrics, DESIGN
  // §4.8): a plane set per staging slot that the frame's deblock pushes its
  // output to (FrameArgs::push), the tile partials of metrics.hip, and each
  // slot's result in mapped pinned host memory, written by k_metrics_finish.
  int metrics = 0;
  int16_t* keep = nullptr;             // [stages] plane sets
  MetricsPartial* met_part = nullptr;  // [stages][3][metrics_tiles(w, h)]
  cairo_frame_metrics* met_host = nullptr;  // [stages]
  cairo_frame_metrics* met_dev = nullptr;   // its device-visible address
  // Target bitrate (cairo_ctx_set_rate): the controller's state
  // lives on the device; launch L's k_rate_decide reads what launch L-2's
  // k_rate_observe wrote, by stream order (the launches alternate between two
  // streams).  The host only keeps which slots the last two launches used.
  bool rate_on = false;
  cairo_rate rate_cfg = {};
  cairo_rate_state* rate_state = nullptr;  // device
  RateSlot* rate_dev = nullptr;            // [stages]
  uint32_t* rate_part = nullptr;           // [stages][kRateBlocks]
  RateSlot* rate_host = nullptr;           // mapped pinned [stages]
  RateSlot* rate_host_dev = nullptr;       // its device-visible address
  int rate_launches = 0;                   // launches since the controller (re)started, up to 2
  int rate_n[2] = {};                      // frames of the last launch [0] and of the one before [1]
  int rate_slot[2][kMaxBatch] = {};        // and their staging slots
  // Thread safety (the frame pipeline of pipeline.cpp calls in from its
  // completion and entropy threads): every public entry point holds mu;
  // HIP event waits on a frame's outputs run outside it.  launched_cv is
  // signalled when a batch launches.
  std::mutex mu;
  std::condition_variable launched_cv;
  std::mutex tmu;                             // guards timeout (written by threads waiting outside mu)
  int32_t timeout[TimeoutInfo::kWords] = {};  // the last reported TimeoutInfo words
};

namespace {

using Pending = cairo_ctx::Pending;

#define CK(x)                                   \
  do {                                          \
    int _r = fail((x), #x);                     \
    if (_r != kSuccess) return _r;              \
  } while (0)

PlaneSet planes_at(int16_t* base, const cairo_ctx* c) {
  return ring_slot(base, 0, (int)c->wa, (int)c->ha, 0);
}
PlaneSet slot_planes(int16_t* base, const cairo_ctx* c, int slot) {
  return ring_slot(base, c->plane_elems, (int)c->wa, (int)c->ha, slot);
}
// Staging slot s's output_cache (chunked allocation).
int16_t* coef_base(const cairo_ctx* c, int slot) {
  return c->coef[slot / c->coef_per] + (size_t)(slot % c->coef_per) * c->plane_elems;
}
PlaneSet coef_planes(const cairo_ctx* c, int slot) { return planes_at(coef_base(c, slot), c); }
PlaneSet peer_coef_planes(const cairo_ctx::Peer& p, const cairo_ctx* c, int slot) {
  return planes_at(p.coef[slot / p.coef_per] + (size_t)(slot % p.coef_per) * c->plane_elems, c);
}
// Allocate the output_cache: one allocation for a context nobody imports;
// fine-grained chunks of at most kCoefChunkBytes, each exported with its own
// IPC handle, for cross-device sharing (cairo_ctx_peer_info).  On failure
// nothing stays allocated.
hipError_t alloc_coef(const cairo_ctx* c, bool fine, int16_t* out[CAIRO_MAX_COEF_CHUNKS], int* chunks, int* per) {
  const size_t slot_bytes = c->plane_elems * 2;
  if (fine && slot_bytes > kCoefChunkBytes) {
    fprintf(stderr, "[cairo_amd] peer_info: one output_cache slot (%zu bytes) exceeds the %zu-byte IPC export limit\n",
            slot_bytes, kCoefChunkBytes);
    return hipErrorInvalidValue;
  }
  const int p = fine ? (int)std::min<size_t>((size_t)c->stages, kCoefChunkBytes / slot_bytes) : c->stages;
  const int n = (c->stages + p - 1) / p;
  if (n > CAIRO_MAX_COEF_CHUNKS) {
    fprintf(stderr, "[cairo_amd] peer_info: %d output_cache chunks needed, at most %d\n", n, CAIRO_MAX_COEF_CHUNKS);
    return hipErrorInvalidValue;
  }
  for (int k = 0; k < CAIRO_MAX_COEF_CHUNKS; k++) out[k] = nullptr;
  for (int k = 0; k < n; k++) {
    const size_t bytes = slot_bytes * (size_t)std::min(p, c->stages - k * p);
    const hipError_t e = fine ? hipExtMallocWithFlags((void**)&out[k], bytes, hipDeviceMallocFinegrained)
                              : hipMalloc((void**)&out[k], bytes);
    if (e != hipSuccess) {
      for (int j = 0; j <= k; j++)
        if (out[j]) (void)hipFree(out[j]);
      for (int j = 0; j < CAIRO_MAX_COEF_CHUNKS; j++) out[j] = nullptr;
      return e;
    }
  }
  *chunks = n;
  *per = p;
  return hipSuccess;
}

size_t stamp_words(const cairo_ctx* c) {
  // frames, engine entry/exit, then 3 stamps per inter task
  return kMaxBatch * stamp_frame_words((int)c->wmb, (int)c->hmb) + 2 +
         (size_t)kMaxBatch * c->hmb * ((c->wmb + 3) / 4) * kIStamps;
}

EngineArgs engine_args(const cairo_ctx* c) {
  EngineArgs e;
  memset(&e, 0, sizeof(e));
  e.wa = (int)c->wa, e.ha = (int)c->ha, e.w = (int)c->w, e.h = (int)c->h;
  e.wmb = (int)c->wmb, e.hmb = (int)c->hmb, e.ring = (int)c->ring;
  e.src_base = c->src;
  e.plane_elems = c->plane_elems;
  e.table_base = c->table;
  e.idesc_base = c->idesc;
  e.gran_base = c->gran;
  e.sync = c->sync;
  e.sticky = c->sticky;
  e.inject = c->inject;
  e.stamps = c->stamps;
  e.acct = c->acct;
  e.trace = c->trace_dev;
  return e;
}

// Close the group's imported peer mappings and forget the group.
void leave_group(cairo_ctx* c) {
  for (int i = 0; i < c->gsize; i++) {
    cairo_ctx::Peer& p = c->gp[i];
    if (p.imported) {
      for (void* q : {(void*)p.ring, (void*)p.progress})
        if (q) (void)hipIpcCloseMemHandle(q);
      for (int k = 0; k < p.coef_chunks; k++)
        if (p.coef[k]) (void)hipIpcCloseMemHandle(p.coef[k]);
    }
    p = cairo_ctx::Peer();
  }
  if (c->zero) (void)hipFree(c->zero);
  c->zero = nullptr;
  c->gsize = 1;
  c->grank = 0;
  c->sys = false;
}

// (frame, row) task order of the engine pools for every batch size, by
// row + slope * frame (kOrderSlope for one context; a group of N members
// needs 3N + 2: kernels.h kOrderSlope).
std::vector<int32_t> task_order(int hmb, int slope) {
  const int per = kMaxBatch * hmb;
  std::vector<int32_t> ord((size_t)kMaxBatch * per, 0);
  for (int nf = 1; nf <= kMaxBatch; nf++) {
    int32_t* o = &ord[(size_t)(nf - 1) * per];
    int n = 0;
    for (int d = 0; d < hmb + slope * nf; d++)
      for (int f = 0; f < nf; f++) {
        const int r = d - slope * f;
        if (r >= 0 && r < hmb) o[n++] = (f << 16) | r;
      }
  }
  return ord;
}

// The device block of task orders (OrderBlock): for every batch size the
// plain order (one queue per pool) and the labelled one (task_order stably
// partitioned by task_label: one queue per label and pool), then each one's
// label segments.
struct OrderBlock {
  static size_t order_at(int hmb, int banded, int nf) { return ((size_t)banded * kMaxBatch + nf - 1) * kMaxBatch * hmb; }
  static size_t seg_at(int hmb, int banded, int nf) {
    return (size_t)2 * kMaxBatch * kMaxBatch * hmb + ((size_t)banded * kMaxBatch + nf - 1) * (kLabels + 1);
  }
  static size_t words(int hmb) { return seg_at(hmb, 2, 1); }
};

std::vector<int32_t> order_block(int hmb, int slope) {
  const std::vector<int32_t> ord = task_order(hmb, slope);
  std::vector<int32_t> blk(OrderBlock::words(hmb), 0);
  for (int nf = 1; nf <= kMaxBatch; nf++) {
    const int32_t* o = &ord[(size_t)(nf - 1) * kMaxBatch * hmb];
    const int total = nf * hmb;
    std::copy(o, o + total, &blk[OrderBlock::order_at(hmb, 0, nf)]);
    int32_t* seg = &blk[OrderBlock::seg_at(hmb, 0, nf)];
    for (int l = 1; l <= kLabels; l++) seg[l] = total;
    int32_t* ob = &blk[OrderBlock::order_at(hmb, 1, nf)];
    int32_t* sb = &blk[OrderBlock::seg_at(hmb, 1, nf)];
    int n = 0;
    for (int l = 0; l < kLabels; l++) {
      sb[l] = n;
      for (int i = 0; i < total; i++)
        if (task_label(o[i] >> 16, o[i] & 0xFFFF, hmb) == l) ob[n++] = o[i];
    }
    sb[kLabels] = n;
  }
  return blk;
}

// Whether a launch's pool uses per-label (XCD-banded) queues: frames of at
// least kBandMinRows macroblock rows, both pools splitting evenly over the
// labels, and the pool enabled in kBandPools.  flush() and cairo_task_queues
// share it, so the tests check the layout the engine runs.
bool banded_pool(int hmb, int n_helpers, int n_rows, int pool) {
  return hmb >= kBandMinRows && n_helpers % kLabels == 0 && n_rows % kLabels == 0 && ((kBandPools >> pool) & 1);
}

int upload_orders(cairo_ctx* c, int slope) {
  c->order_slope = slope;
  const std::vector<int32_t> blk = order_block((int)c->hmb, slope);
  CK(hipMemcpy(c->order, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->prev_total = 0;  // the previous launch's queue used the other order
  return kSuccess;
}

void free_ctx(cairo_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->ks) (void)hipStreamSynchronize(c->ks);
  if (c->ks2) (void)hipStreamSynchronize(c->ks2);
  if (c->cs) (void)hipStreamSynchronize(c->cs);
  for (auto& s : c->st) {
    if (s.table) (void)hipHostFree(s.table);
    if (s.coef) (void)hipHostFree(s.coef);
    if (s.err) (void)hipHostFree(s.err);
    if (s.d2h_done) (void)hipEventDestroy(s.d2h_done);
    if (s.rgb_read) (void)hipEventDestroy(s.rgb_read);
  }
  for (auto& t : c->tb)
    for (auto& e : t.ev)
      if (e) (void)hipEventDestroy(e);
  if (c->engine_done) (void)hipEventDestroy(c->engine_done);
  if (c->t_base) (void)hipEventDestroy(c->t_base);
  for (auto& ev : c->batch_end)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->batch_ready)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->pre_done)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->fdesc_done)
    if (ev) (void)hipEventDestroy(ev);
  if (c->fdesc_host) (void)hipHostFree(c->fdesc_host);
  if (c->feed_host) (void)hipHostFree(c->feed_host);
  if (c->fs) (void)hipStreamDestroy(c->fs);
  if (c->trace_host) (void)hipHostFree(c->trace_host);
  if (c->met_host) (void)hipHostFree(c->met_host);
  if (c->rate_host) (void)hipHostFree(c->rate_host);
  leave_group(c);
  for (int16_t* q : c->coef)
    if (q) (void)hipFree(q);
  for (void* p : {(void*)c->fdesc, (void*)c->order, (void*)c->src, (void*)c->table, (void*)c->idesc, (void*)c->progress, (void*)c->feed_dev, (void*)c->feed_hdr, (void*)c->feed_scratch,
                  (void*)c->gran, (void*)c->rgb, (void*)c->ring_buf, (void*)c->sync, (void*)c->sticky,
                  (void*)c->predeblock, (void*)c->stamps, (void*)c->acct, (void*)c->keep, (void*)c->met_part,
                  (void*)c->rate_state, (void*)c->rate_dev, (void*)c->rate_part})
    (void)hipFree(p);
  if (c->us) (void)hipStreamSynchronize(c->us);
  if (c->up_last) (void)hipEventDestroy(c->up_last);
  if (c->us) (void)hipStreamDestroy(c->us);
  if (c->ks) (void)hipStreamDestroy(c->ks);
  if (c->ks2) (void)hipStreamDestroy(c->ks2);
  if (c->cs) (void)hipStreamDestroy(c->cs);
  delete c;
}

// Fresh-encoder state (every stream idle): zero planes, tables and granules,
// the launch sync areas and the sticky timeout word, so a context that once
// reported a timed-out wait is usable again after cairo_ctx_reset.
int zero_state(cairo_ctx* c) {
  const size_t S = (size_t)c->stages;
  CK(hipMemsetAsync(c->src, 0, c->plane_elems * 2 * S, c->ks));
  for (int k = 0; k < c->coef_chunks; k++)
    CK(hipMemsetAsync(c->coef[k], 0, c->plane_elems * 2 * (size_t)std::min(c->coef_per, c->stages - k * c->coef_per),
                      c->ks));
  CK(hipMemsetAsync(c->ring_buf, 0, c->plane_elems * 2 * c->ring_slots, c->ks));
  CK(hipMemsetAsync(c->table, 0, c->mbs * sizeof(BlockDesc) * S, c->ks));
  // inter records: a frame whose search was cut short by a timed-out wait
  // still reads in-frame motion vectors
  CK(hipMemsetAsync(c->idesc, 0, c->nref * c->mbs * sizeof(BlockDesc) * S, c->ks));
  // granule tags start at 0; the n-th submission after a reset publishes tag n
  CK(hipMemsetAsync(c->gran, 0, c->mbs * kGranuleStride * sizeof(uint64_t) * S, c->ks));
  CK(hipMemsetAsync(c->sync, 0, c->sync_words * sizeof(int32_t) * kSyncAreas, c->ks));
  CK(hipMemsetAsync(c->progress, 0, (size_t)c->hmb * sizeof(uint64_t) * S, c->ks));
  CK(hipMemsetAsync(c->sticky, 0, TimeoutInfo::kWords * sizeof(int32_t), c->ks));
  CK(hipStreamSynchronize(c->ks));
  {
    std::lock_guard<std::mutex> lk(c->tmu);
    memset(c->timeout, 0, sizeof(c->timeout));
  }
  c->epoch = 0;
  c->last_slot = -1;
  c->batches = 0;
  c->prev_total = 0;  // its sync areas are zero now
  c->fresh = true;  // the first frame after a reset depends on no earlier frame
  c->since_fresh = 0;
  // tickets restart at 0 (every stage is idle here): a group member's k-th
  // frame after a (re)join is its ticket k, which its peers assume when they
  // locate its output_cache and progress words (frame_links)
  c->next_ticket = 0;
  for (auto& s : c->st) {
    memset(s.err, 0, TimeoutInfo::kWords * sizeof(int32_t));
    s.ticket = -1;
  }
  return kSuccess;
}

int collect_times(cairo_ctx* c, TimedBatch& t) {
  if (!t.pending) return kSuccess;
  CK(hipEventSynchronize(t.ev[kTimed]));
  for (int k = 0; k < kTimed; k++) {
    float ms = 0;
    CK(hipEventElapsedTime(&ms, t.ev[k], t.ev[k + 1]));
    c->acc_ms[k] += ms;
  }
  float s0 = 0, s1 = 0;  // the engine's interval on the common clock
  CK(hipEventElapsedTime(&s0, c->t_base, t.ev[2]));
  CK(hipEventElapsedTime(&s1, c->t_base, t.ev[3]));
  c->busy.emplace_back((double)s0, (double)s1);
  c->acc_frames += t.frames;
  t.pending = false;
  return kSuccess;
}

// Copy a frame of format fmt (fmt < 0: RGB888) between a staging slot, where it
// lies tight (every tight format fits the slot's 3 * w * h bytes), and a host
// frame of the given pitch (0: tight): one copy when that is tight too, else a
// 2D copy per plane, so a host frame's pitch padding keeps its bytes.
// Asynchronous on st.
int copy_frame(const cairo_ctx* c, uint8_t* staged, uint8_t* host, bool upload, int fmt, uint32_t pitch,
               hipStream_t st) {
  uint64_t bytes = (uint64_t)c->w * c->h * 3;
  uint32_t tight = 3 * c->w;
  if (fmt >= 0 && cairo_frame_layout(fmt, c->w, c->h, 0, &bytes, &tight) != kSuccess) return kInvalidArg;
  const hipMemcpyKind kind = upload ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  if (fmt < 0 || !pitch || pitch == tight) {
    CK(hipMemcpyAsync(upload ? staged : host, upload ? host : staged, (size_t)bytes, kind, st));
    return kSuccess;
  }
  // one plane: `rows` rows of `row` bytes, at soff (pitch sp) in the slot and hoff (pitch hp) in the host frame
  auto plane = [&](size_t soff, size_t sp, size_t hoff, size_t hp, size_t row, size_t rows) {
    return upload ? hipMemcpy2DAsync(staged + soff, sp, host + hoff, hp, row, rows, kind, st)
                  : hipMemcpy2DAsync(host + hoff, hp, staged + soff, sp, row, rows, kind, st);
  };
  const size_t w = c->w, h = c->h;
  CK(plane(0, tight, 0, pitch, tight, h));  // RGB rows, packed 4:2:2 rows, or the Y plane
  if (fmt == CAIRO_FMT_P010) {              // the UV rows: w 16-bit words each, like the Y rows
    CK(plane((size_t)tight * h, tight, (size_t)pitch * h, pitch, tight, h / 2));
  } else if (fmt == CAIRO_FMT_I420) {
    const size_t cw = w / 2, ch = h / 2, cp = pitch / 2;
    CK(plane(w * h, cw, (size_t)pitch * h, cp, cw, ch));
    CK(plane(w * h + cw * ch, cw, (size_t)pitch * h + cp * ch, cp, cw, ch));
  } else if (fmt == CAIRO_FMT_NV12) {
    CK(plane(w * h, w, (size_t)pitch * h, pitch, w, h / 2));
  }
  return kSuccess;
}

// A staging slot's frame buffer: 3 * w * h bytes, which every tight format fits.
uint8_t* slot_rgb(const cairo_ctx* c, int slot) { return c->rgb + (size_t)slot * c->w * c->h * 3; }

// One launch of the pending batch, handed from step to step of flush(): the
// plan, the inputs, the engine, the outputs.
struct Launch {
  EngineArgs e;
  hipStream_t st = nullptr, ost = nullptr;  // the launch's stream; the stream its outputs complete on
  int fslot = 0, area = 0, rows = 0;
  FrameArgs *fh = nullptr, *fd = nullptr;  // its frame views: pinned host slot, device copy
  TimedBatch* tb = nullptr;                // profiling events (nullptr: off)
};

// Plan: the launch's stream, sync area, frame views, pool split and task
// queues.
int plan_launch(cairo_ctx* c, Launch& l) {
  EngineArgs& e = l.e;
  e = engine_args(c);
  e.nframes = c->npend;
  // frame descriptors -> device (a ring of pinned slots: the copy of an earlier
  // launch may still be pending when this one is written)
  const int fslot = l.fslot = c->fdesc_next;
  c->fdesc_next = (c->fdesc_next + 1) % kLaunchSlots;
  if (c->fdesc_used[fslot]) CK(hipEventSynchronize(c->fdesc_done[fslot]));
  FrameArgs* fh = l.fh = c->fdesc_host + (size_t)fslot * kMaxBatch;
  FrameArgs* fd = l.fd = c->fdesc + (size_t)fslot * kMaxBatch;
  e.fa = fd;
  e.decode = c->pend[0].f.decode;  // a launch never mixes (decode_frame flushes first)
  const int rows = l.rows = e.nframes * e.hmb;
  // Launch b alternates streams and sync areas; it follows launch b-1, which
  // may still be running: its frame 0 waits on the deblock progress of b-1's
  // last frame (tagged words in that frame's staging slot).  Residency: a
  // launch takes at most half of the engine's resident
  // workgroup slots (CUs x occupancy, measured at create: 256 x 3 = 768 on a
  // full MI355X), so two launches are always co-resident.  Every row has a
  // coder task and a helper (inter search + deblock) task: two pools.  The
  // pools are shared: launch b's workers take b-1's
  // remaining tasks first (all of them are older), so b-1's tail is not left
  // to b-1's own workers; a batch is complete when its finished-task count
  // says so (k_batch_wait), not when its launch ends.
  const long long b = c->batches++;
  l.st = l.ost = (b & 1) ? c->ks2 : c->ks;
  const int area = l.area = (int)(b % kSyncAreas);
  e.sync = c->sync + (size_t)area * c->sync_words;
  e.pfa = c->prev_fa;
  for (int k = 0; k < 2; k++) e.porder[k] = c->prev_order[k], e.pseg[k] = c->prev_seg[k];
  e.psync = c->prev_sync;
  e.ptotal = c->prev_decode == e.decode ? c->prev_total : 0;  // a worker runs one kind of task
  e.slope = c->order_slope;
  for (int i = 0; i < c->npend; i++) fh[i] = make_frame_view(e, c->pend[i].f, i);
  // The plain engine (EngineArgs::general) has no diagnostics
  // and only agent-scope hand-offs: for a launch without stamps, trace or
  // inject none of whose frames -- its own, or those of the previous launch
  // whose queues its workers serve -- is shared across devices.  A decode
  // launch always takes the general engine.
  bool sys = e.ptotal && c->prev_sys;
  for (int i = 0; i < c->npend; i++) sys |= c->pend[i].f.sys != 0;
  e.general = e.decode || e.stamps || e.trace || e.inject || sys;
  {  // half of the resident slots per launch, split between the pools
    const int total = 2 * (c->wg_rows > 0 ? std::min(c->wg_rows, (c->stamps ? 2 : 1) * c->max_rows) : c->max_rows);
    // default split: even, and 25/48 helpers (200 of 384) on large frames
    // (kernels.h kPrioFrameMBs); multiples of kLabels keep both pools banded
    const bool large = (int)c->wmb * (int)c->hmb > kPrioFrameMBs;
    int nh = c->wg_helpers > 0 ? std::min(c->wg_helpers, total - 1)
                               : (large ? std::max(1, (total * 25 / 48) & ~(kLabels - 1)) : total / 2);
    int nr = total - nh;
    e.n_helpers = std::max(1, std::min(nh, rows));
    e.n_rows = std::max(1, std::min(nr, rows));
  }
  // XCD-banded queues (kernels.h kLabels) on large frames, when both pools
  // split evenly over the labels
  for (int k = 0; k < 2; k++) {
    const int bk = banded_pool((int)c->hmb, e.n_helpers, e.n_rows, k);
    e.nlab[k] = bk ? kLabels : 1;
    e.order[k] = c->order + OrderBlock::order_at((int)c->hmb, bk, e.nframes);
    e.seg[k] = c->order + OrderBlock::seg_at((int)c->hmb, bk, e.nframes);
  }
  // this sync area was last used by launch b-3 (only a launch reads its own
  // area); launch b-2 precedes this one on the same stream
  if (b >= 3) CK(hipStreamWaitEvent(l.st, c->batch_end[(b - 3) % kSyncAreas], 0));
  return kSuccess;
}

// Inputs: the uploads issued at submit, host sources still to upload, the
// decoder's table and coefficients.
int enqueue_uploads(cairo_ctx* c, Launch& l) {
  const hipStream_t st = l.st;
  if (c->profiling) {
    l.tb = &c->tb[c->tb_next];
    c->tb_next = (c->tb_next + 1) % kLaunchSlots;
    int r = collect_times(c, *l.tb);  // its events are about to be reused
    if (r) return r;
  }
  if (c->up_pending) {  // the frames' uploads, issued at submit on the upload stream
    CK(hipStreamWaitEvent(st, c->up_last, 0));
    c->up_pending = false;
  }
  for (int i = 0; i < l.e.nframes; i++) {  // host RGB sources; the decoder's table and coefficients
    const FrameDesc& f = c->pend[i].f;
    if (f.host_rgb) {
      const int r = copy_frame(c, slot_rgb(c, f.slot), const_cast<uint8_t*>(f.host_rgb), true, c->pend[i].fmt,
                               c->pend[i].hpitch, st);
      if (r) return r;
    }
    if (f.decode) {
      CK(hipMemcpyAsync(c->table + (size_t)f.slot * c->mbs, f.host_table, c->mbs * sizeof(BlockDesc),
                        hipMemcpyHostToDevice, st));
      CK(hipMemcpyAsync(coef_base(c, f.slot), f.host_coef, c->plane_elems * 2, hipMemcpyHostToDevice, st));
    }
  }
  if (c->stamps) {  // engine entry (min) / exit (max) words
    static const uint64_t init[2] = {~0ull, 0};
    CK(hipMemcpyAsync(c->stamps + kMaxBatch * stamp_frame_words((int)c->wmb, (int)c->hmb), init, sizeof(init),
                      hipMemcpyHostToDevice, st));
  }
  if (l.tb) CK(hipEventRecord(l.tb->ev[0], st));
  return kSuccess;
}

// Inputs: the pre-pass of one kind of frame (scaled: k_scale_batch, tensor:
// k_tensor_pack_batch, scaled tensor: k_tensor_scale_batch) fills those
// frames' staging slots before the convert
// reads them: one kernel, and another whenever its argument block is full.
// A launch without such a frame enqueues nothing here.  A slot's previous
// frame may have been converted on the other launch stream (a ticket may be
// released unwaited): wait for that convert (rgb_read).
template <class Args, class Frame>
int enqueue_prepass(cairo_ctx* c, const Launch& l, Pending::Kind kind, Frame Pending::*frame,
                    hipError_t (*launch)(const Args&, hipStream_t)) {
  Args a;  // only the header is written here: every block is {frame width, height, nframes, reserved, f[]}
  auto& [aw, ah, an, ares, af] = a;
  aw = (int)c->w, ah = (int)c->h, an = 0, ares = 0;
  constexpr int cap = (int)(sizeof(af) / sizeof(af[0]));
  for (int i = 0; i < l.e.nframes; i++) {
    if (c->pend[i].kind != kind) continue;
    Stage& s = c->st[c->pend[i].f.slot];
    if (s.rgb_pending) {
      CK(hipStreamWaitEvent(l.st, s.rgb_read, 0));
      s.rgb_pending = false;
    }
    af[an++] = c->pend[i].*frame;
    if (an == cap) {
      CK(launch(a, l.st));
      an = 0;
    }
  }
  if (an) CK(launch(a, l.st));
  return kSuccess;
}

// Inputs: the convert, which also writes the frame views and zeroes the sync
// area, then the records that say so (rgb_read, fdesc_done, batch_ready).
int enqueue_convert(cairo_ctx* c, Launch& l) {
  const EngineArgs& e = l.e;
  const hipStream_t st = l.st;
  // the frame views and the zeroed sync area are written by the convert
  // kernel below (ConvertArgs), not by runtime copy / fill kernels
  ConvertArgs ca{};
  ca.w = e.w, ca.h = e.h, ca.wa = e.wa, ca.nframes = e.nframes;
  for (int i = 0; i < e.nframes; i++) {
    ca.rgb[i] = l.fh[i].decode ? nullptr : l.fh[i].rgb;
    ca.in[i] = l.fh[i].in;
  }
  static_assert(sizeof(FrameArgs) % sizeof(uint4) == 0, "frame views copied in 16-byte chunks");
  ca.fa_host = (const uint4*)(c->fdesc_host_dev + (size_t)l.fslot * kMaxBatch);
  ca.fa_dev = (uint4*)l.fd;
  ca.fa_chunks = (int)(sizeof(FrameArgs) * e.nframes / sizeof(uint4));
  ca.sync = e.sync;
  ca.sync_words = (int)c->sync_words;
  // A launch of tight RGB24 frames keeps k_convert_batch, whose behaviour
  // beside the running launch is measured; any other
  // layout in the launch takes all of its frames through k_convert_fmt_batch
  // (a colour description belongs to a YUV frame, which is never tight RGB24).
  bool tight_rgb = true;
  for (int i = 0; i < e.nframes; i++)
    tight_rgb &= !ca.rgb[i] || (c->pend[i].fmt == CAIRO_FMT_RGB24 && c->pend[i].pitch == 3 * c->w);
  if (tight_rgb) {
    CK(launch_convert_batch(ca, st));
  } else {
    ConvertFmtArgs cf{};
    cf.c = ca;
    for (int i = 0; i < e.nframes; i++)
      cf.fmt[i] = c->pend[i].fmt, cf.pitch[i] = c->pend[i].pitch, cf.col[i] = c->pend[i].col;
    CK(launch_convert_fmt_batch(cf, st));
  }
  CK(hipEventRecord(c->fdesc_done[l.fslot], st));  // fh has been read
  c->fdesc_used[l.fslot] = true;
  // (a staged frame of any format starts at its slot's address)
  for (int i = 0; i < e.nframes; i++) {  // staged host RGB converted: the buffer may be refilled
    const FrameDesc& f = c->pend[i].f;
    Stage& s = c->st[f.slot];
    if (!f.decode && f.rgb == slot_rgb(c, f.slot)) {
      CK(hipEventRecord(s.rgb_read, st));
      s.rgb_pending = true;
    }
  }
  // Target bitrate: the launch's quality goes into its views here, after the
  // convert kernel that writes them and before batch_ready is recorded -- the
  // next launch's workers may run this launch's tasks from these views as soon
  // as that event fires.  It reads the records of launch b-2, which precedes
  // this one on the same stream, k_rate_observe included.
  if (c->rate_on) {
    RateDecideArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.cfg = c->rate_cfg;
    ra.state = c->rate_state;
    ra.obs = c->rate_dev;
    ra.host = c->rate_host_dev;
    ra.fa = l.fd;
    ra.n_new = e.nframes;
    ra.n_obs = c->rate_launches >= 2 ? c->rate_n[1] : 0;
    for (int i = 0; i < ra.n_obs; i++) ra.oslot[i] = c->rate_slot[1][i];
    for (int i = 0; i < e.nframes; i++) ra.nslot[i] = c->pend[i].f.slot;
    CK(launch_rate_decide(ra, st));
  }
  CK(hipEventRecord(c->batch_ready[l.area], st));
  // the previous batch's tasks, which this launch's workers may run, need its
  // frames converted and its views and sync area in place
  if (e.ptotal) CK(hipStreamWaitEvent(st, c->batch_ready[c->prev_area], 0));
  return kSuccess;
}

// Engine: k_engine, and the kernel that waits for the batch.
int enqueue_engine(cairo_ctx* c, Launch& l) {
  const EngineArgs& e = l.e;
  const hipStream_t st = l.st;
  TimedBatch* tb = l.tb;
  if (tb) CK(hipEventRecord(tb->ev[1], st));
  if (tb) CK(hipEventRecord(tb->ev[2], st));
  CK(launch_engine(e, st));
  // the launch ends when its workers find no task left; its batch is done
  // when every task has finished (the next launch's workers may run the last)
  CK(launch_batch_wait(e.sync, 2 * l.rows, c->sticky, st));
  c->prev_fa = l.fd;
  for (int k = 0; k < 2; k++) c->prev_order[k] = e.order[k], c->prev_seg[k] = e.seg[k];
  c->prev_sync = e.sync;
  c->prev_total = l.rows;
  c->prev_area = l.area;
  c->prev_decode = e.decode;
  c->prev_sys = false;
  for (int i = 0; i < e.nframes; i++) c->prev_sys |= l.fh[i].sys != 0;
  c->engine_variant = e.general;
  if (tb) {
    CK(hipEventRecord(tb->ev[3], st));
    tb->frames = e.nframes;
    tb->pending = true;
  }
  return kSuccess;
}

// Outputs: the debug pre-deblock unpack, the per-frame metrics, the precode and
// its feed copy (l.ost becomes the stream that copy runs on).
int enqueue_results(cairo_ctx* c, Launch& l) {
  const EngineArgs& e = l.e;
  const hipStream_t st = l.st;
  if (c->predeblock) CK(launch_unpack_granules(e, e.nframes - 1, planes_at(c->predeblock, c), st));
  // Per-frame metrics: one launch for the batch, after k_batch_wait on the
  // launch's stream (every push store of the batch has been drained by then,
  // DESIGN §4.8) and before the precode, so that every path to a frame's
  // d2h_done below already follows it.
  if (c->metrics & (CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM)) {
    MetricsArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.w = e.w, ma.h = e.h, ma.pitch = e.wa;
    ma.flags = c->metrics;
    for (int i = 0; i < e.nframes; i++) {
      if (c->pend[i].f.decode) continue;
      const int slot = c->pend[i].f.slot;
      ma.a[ma.nframes] = l.fh[i].in;
      ma.b[ma.nframes] = slot_planes(c->keep, c, slot);
      ma.slot[ma.nframes++] = slot;
    }
    ma.part = c->met_part;
    ma.out = c->met_dev;
    CK(launch_metrics(ma, st));
  }
  if (!(c->outputs & CAIRO_OUT_FEED)) return kSuccess;
  FeedArgs fa;  // the entropy precode, straight into mapped host memory
  memset(&fa, 0, sizeof(fa));
  fa.nframes = e.nframes;
  fa.fa = l.fd;
  for (int i = 0; i < e.nframes; i++) {
    fa.slot[i] = c->pend[i].f.slot;
    fa.host[i] = c->feed_host + (size_t)fa.slot[i] * (kFeedHdrWords + c->feed_words);
  }
  fa.scratch = c->feed_scratch;
  fa.scratch_stride = feed_scratch_words(c->mbs);
  fa.feed = c->feed_dev;
  fa.feed_stride = c->feed_words;
  fa.hdr = c->feed_hdr;
  // each frame's block table and the timeout words go to its mapped pinned
  // stage in the same kernel as the feed: no D2H copy per frame, whose
  // shader blit waits for a workgroup slot of the persistent engine
  for (int i = 0; i < e.nframes; i++) {
    const Stage& s = c->st[fa.slot[i]];
    fa.table_host[i] = c->pend[i].f.decode ? nullptr : (uint4*)s.table_dev;
    fa.err_host[i] = c->pend[i].f.decode ? nullptr : s.err_dev;
  }
  fa.table_words = (int)(c->mbs * sizeof(BlockDesc) / sizeof(uint4));
  CK(launch_precode(fa, (int)c->mbs, st));
  // Target bitrate: the frames' set bits are counted right behind the precode
  // on the launch's stream, before pre_done is recorded: ahead of every
  // frame's d2h_done (the host reads the slot's record after it) and of the
  // launch two ahead on this stream, whose k_rate_decide reads it.
  if (c->rate_on) {
    RateObserveArgs ro;
    memset(&ro, 0, sizeof(ro));
    ro.nframes = e.nframes;
    for (int i = 0; i < e.nframes; i++) ro.slot[i] = fa.slot[i];
    ro.feed = c->feed_dev;
    ro.feed_stride = c->feed_words;
    ro.hdr = c->feed_hdr;
    ro.part = c->rate_part;
    ro.dev = c->rate_dev;
    ro.host = c->rate_host_dev;
    CK(launch_rate_observe(ro, st));
  }
  // The copy into the mapped host stages is PCIe-bound and no engine
  // launch needs it: on the copy stream, so that the launch two ahead on
  // this stream starts without it (+0.2 %, profiles/r06/ab_4k_feed_copy_aside.txt).
  // Not when the copy stream carries host-RGB uploads (submit): those must
  // not queue behind a feed copy that waits for its launch.
  if (!c->host_uploads) {
    CK(hipEventRecord(c->pre_done[l.area], st));
    CK(hipStreamWaitEvent(c->cs, c->pre_done[l.area], 0));
    CK(launch_feed_copy(fa, c->cs));
    l.ost = c->cs;
  } else {
    CK(launch_feed_copy(fa, st));
  }
  return kSuccess;
}

// Outputs: the end of the batch, then each frame's copies to the host and its
// d2h_done.
int enqueue_copies(cairo_ctx* c, const Launch& l) {
  const hipStream_t ost = l.ost;
  CK(hipEventRecord(c->batch_end[l.area], ost));
  // the copy stream carries the outputs' copies to the host: the feed copies
  // (k_feed_copy, above) or the host-RGB uploads (submit), and with the
  // coefficient planes their D2H copies (the uploads then go on a stream of
  // their own)
  if ((c->outputs & CAIRO_OUT_COEF) && ost != c->cs) {
    CK(hipStreamWaitEvent(c->cs, c->batch_end[l.area], 0));
  }
  // outputs for the host entropy stage: with the feed, the precode's last
  // kernel (k_feed_copy) has written each frame's feed, block table and
  // timeout words into its mapped pinned stage; the coefficient planes (and,
  // without the feed, the table and timeout words) go D2H on the copy stream
  for (int i = 0; i < l.e.nframes; i++) {
    const int slot = c->pend[i].f.slot;
    Stage& s = c->st[slot];
    if (c->pend[i].f.decode) {  // the decoder's output is the slot (decode_frame converts it)
      s.launched = true;
      continue;
    }
    if (c->outputs & CAIRO_OUT_COEF) {
      if (!(c->outputs & CAIRO_OUT_FEED)) {
        CK(hipMemcpyAsync(s.table, c->table + (size_t)slot * c->mbs, c->mbs * sizeof(BlockDesc),
                          hipMemcpyDeviceToHost, c->cs));
        CK(hipMemcpyAsync(s.err, c->sticky, TimeoutInfo::kWords * sizeof(int32_t), hipMemcpyDeviceToHost, c->cs));
      }
      CK(hipMemcpyAsync(s.coef, coef_base(c, slot), c->plane_elems * 2, hipMemcpyDeviceToHost, c->cs));
      CK(hipEventRecord(s.d2h_done, c->cs));
    } else {
      CK(hipEventRecord(s.d2h_done, ost));
    }
    s.launched = true;
  }
  return kSuccess;
}

// Launch the pending batch: the steps above, in the order their comments give
// reasons for.
int flush(cairo_ctx* c) {
  if (c->npend == 0) return kSuccess;
  CK(hipSetDevice(c->device));
  Launch l;
  int r = plan_launch(c, l);  // pool split and queue choice
  // inputs
  if (!r) r = enqueue_uploads(c, l);
  if (!r) r = enqueue_prepass(c, l, Pending::kScaled, &Pending::scale, launch_scale_batch);
  if (!r) r = enqueue_prepass(c, l, Pending::kTensor, &Pending::tens, launch_tensor_pack_batch);
  if (!r) r = enqueue_prepass(c, l, Pending::kTensorScaled, &Pending::tscale, launch_tensor_scale_batch);
  if (!r) r = enqueue_convert(c, l);
  // engine and batch wait
  if (!r) r = enqueue_engine(c, l);
  // outputs
  if (!r) r = enqueue_results(c, l);
  if (!r) r = enqueue_copies(c, l);
  if (r) return r;
  if (c->rate_on) {  // the launch before the last is the one the next launch observes
    c->rate_n[1] = c->rate_n[0];
    memcpy(c->rate_slot[1], c->rate_slot[0], sizeof(c->rate_slot[0]));
    c->rate_n[0] = c->npend;
    for (int i = 0; i < c->npend; i++) c->rate_slot[0][i] = c->pend[i].f.slot;
    if (c->rate_launches < 2) c->rate_launches++;
  }
  c->last_slot = c->pend[c->npend - 1].f.slot;
  c->last_epoch = c->pend[c->npend - 1].f.epoch;
  c->npend = 0;
  c->launched_cv.notify_all();
  return kSuccess;
}

// The cross-frame views of the frame submitted as ticket t (FrameDesc):
// ring slots by index (common.cpp:192-195), the previous ticket's staging
// slot for the output_cache chain and its deblock progress.
void frame_links(cairo_ctx* c, FrameDesc& f, int t) {
  const int R = (int)c->ring;
  f.sys = c->sys;
  if (c->gsize > 1) {
    // Group member: frame m lives with member m % N as its ticket m / N
    // (staging slot (m / N) % stages, reconstruction slot (m / N) % S with
    // S = ceil(R / N) slots per member, so that a slot is reused only by a
    // frame at least R later; when N * S == R that is frame m + R itself,
    // in place, as in the reference's ring).
    const int N = c->gsize, S = (R + N - 1) / N;
    const long n = f.index;
    const PlaneSet zero = planes_at(c->zero, c);
    // Members on other devices or processes (sys) keep mirrors: every frame
    // read here is local (slot (m % N) * S + (m / N) % S of this member's
    // ring), and this frame's deblock pushes it into the same slot of each
    // member that reads it.  Members on one device read each other's rings.
    const bool mirror = c->sys && c->fine_grained && c->ring_slots >= N * S;
    auto slot_of = [&](long m) { return mirror ? (int)((m % N) * S + (m / N) % S) : (int)((m / N) % S); };
    auto recon_of = [&](long m) {
      if (m < 0) return zero;
      return slot_planes(mirror ? c->ring_buf : c->gp[m % N].ring, c, slot_of(m));
    };
    for (int k = 0; k < kMaxRing; k++) f.recon[k] = k < R ? recon_of(n - k) : zero;
    f.stale = recon_of(n - R);
    f.npush = 0;
    if (mirror) {
      bool seen[kMaxGroup] = {};
      seen[c->grank] = true;
      for (int d = 1; d <= R; d++) {  // the frames n+1..n+R-1 reference it, n+R reads its stale rows
        const int j = (int)((n + d) % N);
        if (seen[j]) continue;
        seen[j] = true;
        f.push[f.npush++] = slot_planes(c->gp[j].ring, c, slot_of(n));
      }
    }
    f.progress = c->progress + (size_t)f.slot * c->hmb;
    f.coef = coef_planes(c, f.slot);
    if (n >= 1) {
      const cairo_ctx::Peer& p = c->gp[(n - 1) % N];
      const int ps = (int)(((n - 1) / N) % p.stages);
      f.coef_prev = peer_coef_planes(p, c, ps);
      f.prev_progress = p.progress + (size_t)ps * c->hmb;
    } else {
      f.coef_prev = zero;
      f.prev_progress = nullptr;
    }
    if (n >= 2) {
      const cairo_ctx::Peer& p = c->gp[(n - 2) % N];
      f.prev2_progress = p.progress + (size_t)(((n - 2) / N) % p.stages) * c->hmb;
    } else {
      f.prev2_progress = nullptr;
    }
    c->fresh = false;
    c->since_fresh++;
    return;
  }
  for (int k = 0; k < kMaxRing; k++)
    f.recon[k] = slot_planes(c->ring_buf, c, k < R ? (int)(((uint32_t)f.index + R - k) % R) : 0);
  f.npush = 0;
  if (c->metrics && !f.decode) {  // the deblock stores the frame into its slot's keep as well
    f.npush = 1;
    f.push[0] = slot_planes(c->keep, c, f.slot);
  }
  f.stale = f.recon[0];
  const int ps = (t + c->stages - 1) % c->stages;
  f.coef = coef_planes(c, f.slot);
  f.coef_prev = coef_planes(c, ps);
  f.progress = c->progress + (size_t)f.slot * c->hmb;
  f.prev_progress = c->fresh ? nullptr : c->progress + (size_t)ps * c->hmb;
  f.prev2_progress = c->since_fresh < 2 ? nullptr : c->progress + (size_t)((t + 2 * c->stages - 2) % c->stages) * c->hmb;
  c->fresh = false;
  c->since_fresh++;
}

int sync_all(cairo_ctx* c) {
  int r = flush(c);
  if (r) return r;
  CK(hipStreamSynchronize(c->ks));
  CK(hipStreamSynchronize(c->ks2));
  CK(hipStreamSynchronize(c->cs));
  if (c->us) CK(hipStreamSynchronize(c->us));
  return kSuccess;
}

// Whether [p, p + bytes) is device memory of the context's GPU, inside one
// allocation (bytes 0: only where p points is asked): a wrong pitch or stride is
// refused here, not found as an access past the buffer.  Says why not, for `who`.
bool device_span(const cairo_ctx* c, const void* p, uint64_t bytes, const char* who) {
  hipPointerAttribute_t pa;
  if (hipPointerGetAttributes(&pa, p) != hipSuccess || pa.type != hipMemoryTypeDevice || pa.device != c->device) {
    (void)hipGetLastError();
    fprintf(stderr, "[cairo_amd] %s: %p is not device memory of device %d (host memory is not taken here)\n", who, p,
            c->device);
    return false;
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (bytes && (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess ||
                (uint64_t)((const uint8_t*)p - (const uint8_t*)base) + bytes > (uint64_t)size)) {
    (void)hipGetLastError();
    fprintf(stderr, "[cairo_amd] %s: the span of %llu bytes at %p does not fit its allocation on device %d\n", who,
            (unsigned long long)bytes, p, c->device);
    return false;
  }
  return true;
}

// A host frame into its staging slot (mu held).  One context uploads it now,
// beside the launches in flight; a group member at its launch, on the launch
// stream (its queue budget, join_group): the caller keeps it valid until wait.
int stage_host_frame(cairo_ctx* c, Stage& s, Pending& p, const uint8_t* rgb) {
  p.f.host_rgb = rgb;
  if (c->gsize > 1) return kSuccess;
  // The staging buffer's previous frame may still wait for its conversion (a
  // caller may release a ticket without waiting for it): the upload waits for
  // the launch that converts it (rgb_read).  With feed outputs only, the copy
  // stream carries nothing else once a context uploads (flush then keeps the
  // feed copies on the launch stream), so the uploads use it: on a stream of
  // their own they ran at 12.3 GB/s instead of 19.1 (bench.py host_rgb, 4K;
  // GPU_MAX_HW_QUEUES is 4 by default: a fifth stream shares a hardware queue
  // with one of the others).  With the coefficient planes' D2H copies queued
  // on the copy stream, they get a stream of their own.
  c->host_uploads = true;
  hipStream_t up = c->cs;
  if (c->outputs & CAIRO_OUT_COEF) {
    if (!c->us) CK(hipStreamCreateWithFlags(&c->us, hipStreamNonBlocking));
    up = c->us;
  }
  if (!c->up_last) CK(hipEventCreateWithFlags(&c->up_last, hipEventDisableTiming));
  if (s.rgb_pending) {
    CK(hipStreamWaitEvent(up, s.rgb_read, 0));
    s.rgb_pending = false;
  }
  // packed tight into the slot (3 * w * h bytes for RGB24)
  const int r = copy_frame(c, const_cast<uint8_t*>(p.f.rgb), const_cast<uint8_t*>(rgb), true, p.fmt, p.hpitch, up);
  if (r) return r;
  CK(hipEventRecord(c->up_last, up));
  c->up_pending = true;
  p.f.host_rgb = nullptr;
  return kSuccess;
}

// A plane set into a staging slot's frame buffer, tight: RGB888 through
// k_yuv_to_rgb (kSinkRgb888, as cairo_ctx_decode_frame ever did), or any
// CAIRO_FMT_* through k_planes_to_fmt.  Asynchronous on st.
int stage_planes(const cairo_ctx* c, const PlaneSet& p, int slot, int fmt, hipStream_t st) {
  if (fmt == kSinkRgb888)
    return fail(launch_yuv_to_rgb(p, (int)c->wa, (int)c->w, (int)c->h, slot_rgb(c, slot), st), "launch_yuv_to_rgb");
  uint32_t tight = 0;
  if (cairo_frame_layout(fmt, c->w, c->h, 0, nullptr, &tight) != kSuccess) return kInvalidArg;
  return fail(launch_planes_to_fmt(p, (int)c->wa, (int)c->w, (int)c->h, fmt, tight, slot_rgb(c, slot), c->out_col, st),
              "launch_planes_to_fmt");
}

// The frame staged tight in a slot, out to its sink: through the output map
// into the sink's device tensor (the slot holds RGB888; the caller checked the
// span), or to the caller's host frame (copy_frame).  Asynchronous on st.
int write_staged(const cairo_ctx* c, int slot, const FrameSink& out, hipStream_t st) {
  uint8_t* staged = slot_rgb(c, slot);
  if (out.tensor) {
    TensorArgs ta;
    ta.w = (int)c->w, ta.h = (int)c->h, ta.nframes = 1, ta.reserved = 0;
    ta.f[0] = TensorFrame{out.base, staged, *out.tensor};
    return fail(launch_tensor_unpack(ta, st), "launch_tensor_unpack");
  }
  return copy_frame(c, staged, out.base, false, out.fmt, out.pitch, st);
}

// A fresh controller state on the device (nothing is in flight), and no launch
// to observe yet.
int restart_rate(cairo_ctx* c) {
  cairo_rate_state s;
  rate_init(&s);
  CK(hipMemcpy(c->rate_state, &s, sizeof(s), hipMemcpyHostToDevice));
  c->rate_launches = 0;
  c->rate_n[0] = c->rate_n[1] = 0;
  return kSuccess;
}

}  // namespace

extern "C" {

// cairo_ctx_create_ex: the streams and every device buffer of a context whose
// geometry is set.
static int alloc_device(cairo_ctx* c) {
  CK(hipSetDevice(c->device));
  {  // engine pools per launch: half of the resident workgroup slots, split
     // between helpers and row coders at submit
    int cus = 0, per_cu = 0;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    CK(engine_blocks_per_cu(&per_cu));
    c->max_rows = std::max(1, cus * per_cu / 4);
  }
  CK(hipStreamCreateWithFlags(&c->ks, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&c->ks2, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking));
  const size_t S = (size_t)c->stages;
  CK(hipMalloc(&c->src, c->plane_elems * 2 * S));
  CK(alloc_coef(c, false, c->coef, &c->coef_chunks, &c->coef_per));
  CK(hipMalloc(&c->ring_buf, c->plane_elems * 2 * c->ring));
  c->ring_slots = (int)c->ring;
  CK(hipMalloc(&c->table, c->mbs * sizeof(BlockDesc) * S));
  CK(hipMalloc(&c->idesc, c->nref * c->mbs * sizeof(BlockDesc) * S));
  CK(hipMalloc(&c->gran, c->mbs * kGranuleStride * sizeof(uint64_t) * S));
  CK(hipMalloc(&c->rgb, (size_t)c->w * c->h * 3 * S));
  CK(hipMalloc(&c->sync, c->sync_words * sizeof(int32_t) * kSyncAreas));
  CK(hipMalloc(&c->progress, (size_t)c->hmb * sizeof(uint64_t) * S));
  CK(hipMalloc(&c->sticky, TimeoutInfo::kWords * sizeof(int32_t)));
  CK(hipMemset(c->sticky, 0, TimeoutInfo::kWords * sizeof(int32_t)));
  CK(hipHostMalloc(&c->fdesc_host, sizeof(FrameArgs) * kLaunchSlots * kMaxBatch, hipHostMallocMapped));
  CK(hipHostGetDevicePointer((void**)&c->fdesc_host_dev, c->fdesc_host, 0));
  CK(hipMalloc(&c->fdesc, sizeof(FrameArgs) * kLaunchSlots * kMaxBatch));
  // (frame, row) task order of the engine pools, for every batch size
  CK(hipMalloc(&c->order, OrderBlock::words((int)c->hmb) * sizeof(int32_t)));
  return upload_orders(c, kOrderSlope);
}

// cairo_ctx_create_ex: the stages' pinned host buffers, and the events.
static int alloc_records(cairo_ctx* c) {
  for (auto& s : c->st) {
    CK(hipHostMalloc(&s.table, c->mbs * sizeof(BlockDesc), hipHostMallocMapped));
    CK(hipHostMalloc(&s.coef, c->plane_elems * 2, hipHostMallocDefault));
    CK(hipHostMalloc(&s.err, TimeoutInfo::kWords * sizeof(int32_t), hipHostMallocMapped));
    memset(s.err, 0, TimeoutInfo::kWords * sizeof(int32_t));
    CK(hipHostGetDevicePointer((void**)&s.table_dev, s.table, 0));
    CK(hipHostGetDevicePointer((void**)&s.err_dev, s.err, 0));
    CK(hipEventCreateWithFlags(&s.d2h_done, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&s.rgb_read, hipEventDisableTiming));
  }
  for (auto& t : c->tb)
    for (auto& e : t.ev) CK(hipEventCreate(&e));
  CK(hipEventCreateWithFlags(&c->engine_done, hipEventDisableTiming));
  CK(hipEventCreate(&c->t_base));
  for (auto& ev : c->batch_end) CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  for (auto& ev : c->batch_ready) CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  for (auto& ev : c->pre_done) CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  for (auto& ev : c->fdesc_done) CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return kSuccess;
}

int cairo_ctx_create(uint32_t width, uint32_t height, uint32_t ring, int device, cairo_ctx** out) {
  return cairo_ctx_create_ex(width, height, ring, device, kDefaultStages, out);
}

int cairo_ctx_create_ex(uint32_t width, uint32_t height, uint32_t ring, int device, int stages,
                        cairo_ctx** out) {
  // The reference indexes blocks with uint16 (deblock.cpp, serialize.cpp): at
  // most 65535 macroblocks per frame.
  if (!out || width == 0 || height == 0 || (width & 1) || (height & 1) || ring < 1 ||
      ring > (uint32_t)kMaxRing || ((width + 15) / 16) * ((height + 15) / 16) > 65535u || stages < 2 ||
      stages > kMaxStages)
    return kInvalidArg;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) {
    fprintf(stderr, "[cairo_amd] no HIP device %d available (count %d)\n", device, n);
    return kHardwareFail;
  }
  cairo_ctx* c = new (std::nothrow) cairo_ctx;
  if (!c) return kOutOfMemory;
  c->device = device;
  c->w = width;
  c->h = height;
  c->wa = (width + 15) & ~15u;
  c->ha = (height + 15) & ~15u;
  c->wmb = c->wa / 16;
  c->hmb = c->ha / 16;
  c->ring = ring;
  c->plane_elems = (size_t)c->wa * c->ha * 3 / 2;
  c->mbs = (size_t)c->wmb * c->hmb;
  c->stages = stages;
  c->st.resize((size_t)stages);
  c->batch_max = std::min(default_batch(c->mbs), stages / 2);
  c->nref = ring > 1 ? ring - 1 : 1;
  c->sync_words = (size_t)SyncLayout::words((int)c->hmb, (int)(c->wmb + 3) / 4);
  int r = alloc_device(c);
  if (r == kSuccess) r = alloc_records(c);
  if (r == kSuccess) r = zero_state(c);
  if (r != kSuccess) {
    free_ctx(c);
    return r;
  }
  *out = c;
  return kSuccess;
}

int cairo_ctx_destroy(cairo_ctx* c) {
  if (!c) return kInvalidArg;
  free_ctx(c);
  return kSuccess;
}

int cairo_ctx_reset(cairo_ctx* c) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  for (auto& s : c->st) s.busy = false;
  if (c->gsize > 1) {  // a reset leaves the group (its members reset and rejoin together)
    leave_group(c);
    r = upload_orders(c, kOrderSlope);
    if (r) return r;
  }
  r = zero_state(c);
  if (r == kSuccess && c->rate_on) r = restart_rate(c);  // the controller starts over at q0
  return r;
}

int cairo_ctx_stages(const cairo_ctx* c) { return c ? c->stages : 0; }

int cairo_default_batch(uint32_t width, uint32_t height) {
  if (!width || !height) return 0;
  return default_batch((size_t)((width + 15) / 16) * ((height + 15) / 16));
}

int cairo_task_order(int hmb, int frames, int32_t* out, int* slope) {
  if (hmb < 1 || hmb > 0xFFFF || frames < 1 || frames > kMaxBatch || !out) return kInvalidArg;
  const std::vector<int32_t> ord = task_order(hmb, kOrderSlope);
  memcpy(out, &ord[(size_t)(frames - 1) * kMaxBatch * hmb], (size_t)frames * hmb * sizeof(int32_t));
  if (slope) *slope = kOrderSlope;
  return kSuccess;
}

int cairo_task_queues(int hmb, int frames, int n_helpers, int n_rows, int pool, int32_t* order, int32_t* seg,
                      int* nlab) {
  if (hmb < 1 || hmb > 0xFFFF || frames < 1 || frames > kMaxBatch || !order || !seg || n_helpers < 1 || n_rows < 1 ||
      pool < 0 || pool > 1)
    return kInvalidArg;
  const std::vector<int32_t> blk = order_block(hmb, kOrderSlope);
  const int banded = banded_pool(hmb, n_helpers, n_rows, pool);
  memcpy(order, &blk[OrderBlock::order_at(hmb, banded, frames)], (size_t)frames * hmb * sizeof(int32_t));
  memcpy(seg, &blk[OrderBlock::seg_at(hmb, banded, frames)], (kLabels + 1) * sizeof(int32_t));
  if (nlab) *nlab = banded ? kLabels : 1;
  return kSuccess;
}

int cairo_ctx_set_batch(cairo_ctx* c, int frames) {
  if (!c || frames < 1 || frames > kMaxBatch || frames > c->stages / 2) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  int r = flush(c);
  if (r) return r;
  c->batch_max = frames;
  return kSuccess;
}

int cairo_ctx_set_workgroups(cairo_ctx* c, int rows) {
  // more row coders than stay co-resident with the other in-flight launch
  // would leave tasks to workgroups that never get a slot.  With the stamp
  // diagnostics on (set_debug(2), whose caller waits for each batch) one
  // launch may take every slot.
  if (!c || rows < 0 || rows > (c->stamps ? 2 : 1) * c->max_rows) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  c->wg_rows = rows;
  return kSuccess;
}

int cairo_ctx_set_helpers(cairo_ctx* c, int helpers) {
  if (!c || helpers < 0 || helpers >= 2 * (c->stamps ? 2 : 1) * c->max_rows) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  c->wg_helpers = helpers;
  return kSuccess;
}

int cairo_ctx_set_profiling(cairo_ctx* c, int enable) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  if (enable && !c->profiling) {
    int r = flush(c);
    if (r) return r;
    CK(hipEventRecord(c->t_base, c->ks));
  }
  c->profiling = enable != 0;
  return kSuccess;
}

int cairo_ctx_take_timings(cairo_ctx* c, double ms[4], int* frames) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = flush(c);
  if (r) return r;
  for (auto& t : c->tb) {
    r = collect_times(c, t);
    if (r) return r;
  }
  for (int k = 0; k < kTimed; k++) {
    if (ms) ms[k] = c->acc_ms[k];
    c->acc_ms[k] = 0;
  }
  if (ms) ms[kTimed] = union_length(c->busy);
  c->busy.clear();
  if (frames) *frames = c->acc_frames;
  c->acc_frames = 0;
  return kSuccess;
}

int cairo_ctx_busy_intervals(cairo_ctx* c, double* out, int cap, int* n) {
  if (!c || !n || cap < 0 || (cap && !out)) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  // read-only: the launches made so far (a pending partial batch stays pending)
  for (auto& t : c->tb) {
    const int r = collect_times(c, t);
    if (r) return r;
  }
  std::vector<std::pair<double, double>> iv = c->busy;
  std::sort(iv.begin(), iv.end());
  *n = (int)iv.size();
  for (int i = 0; i < cap && i < (int)iv.size(); i++) {
    out[2 * i] = iv[i].first;
    out[2 * i + 1] = iv[i].second;
  }
  return kSuccess;
}

int cairo_ctx_submit(cairo_ctx* c, const uint8_t* rgb, int rgb_on_device, uint32_t index,
                     uint32_t type, uint32_t quality, int* ticket) {
  return submit_frame(c, {rgb, rgb_on_device, CAIRO_FMT_RGB24, 0, false, nullptr, nullptr}, index, type, quality,
                      ticket);
}

int cairo_ctx_submit_fmt(cairo_ctx* c, const uint8_t* frame, int on_device, int fmt, uint32_t pitch, uint32_t index,
                         uint32_t type, uint32_t quality, int* ticket) {
  return submit_frame(c, {frame, on_device, fmt, pitch, true, nullptr, nullptr}, index, type, quality, ticket);
}

int cairo_ctx_submit_scaled(cairo_ctx* c, const uint8_t* frame, int fmt, uint32_t pitch, const cairo_source* src,
                            uint32_t index, uint32_t type, uint32_t quality, int* ticket) {
  if (!src) return kInvalidArg;
  return submit_frame(c, {frame, 1, fmt, pitch, true, src, nullptr}, index, type, quality, ticket);
}

int cairo_ctx_submit_tensor(cairo_ctx* c, const void* base, const cairo_tensor* desc, uint32_t index, uint32_t type,
                            uint32_t quality, int* ticket) {
  if (!desc) return kInvalidArg;
  return submit_frame(c, {(const uint8_t*)base, 1, CAIRO_FMT_RGB24, 0, true, nullptr, desc}, index, type, quality,
                      ticket);
}

int cairo_ctx_submit_tensor_scaled(cairo_ctx* c, const void* base, const cairo_tensor* desc, const cairo_source* src,
                                   uint32_t index, uint32_t type, uint32_t quality, int* ticket) {
  if (!desc || !src) return kInvalidArg;
  return submit_frame(c, {(const uint8_t*)base, 1, CAIRO_FMT_RGB24, 0, true, src, desc}, index, type, quality, ticket);
}

static const char* timeout_kind_name(int k) {
  switch (k) {
    case kWaitRecords: return "inter records (row coder)";
    case kWaitGranule: return "granule";
    case kWaitPrevProgress: return "previous frame's deblock progress (row helper)";
    case kWaitRowAbove: return "row above's deblock progress (deblock)";
    case kWaitBatch: return "batch completion";
    case kWaitInjected: return "injected (test hook)";
    case kWaitHostMark: return "marked by the host (test hook)";
    default: return "unknown";
  }
}

// A frame found the context's timeout words set: say on stderr which wait
// gave up first, and keep the words for cairo_ctx_timeout_info.
// w is a copy the host took without ordering between the words (a D2H copy,
// or k_feed_copy's relaxed reads in the mapped stage) while a launch may still
// have been writing the record.  The record's kind is stored last, with a
// system-scope release (report_timeout in kernels.hip), so once a read has
// seen the kind, every word of the record was visible before it: a second
// read of the device words, started now, returns the whole record.
// fs: a stream for that read (nullptr: the context's fetch stream, made under
// mu, which the caller must not hold).
static void report_timeout_host(cairo_ctx* c, const int32_t* seen, uint32_t index, hipStream_t fs = nullptr) {
  int32_t w[TimeoutInfo::kWords];
  memcpy(w, seen, sizeof(w));
  {
    if (!fs) {
      std::lock_guard<std::mutex> lk(c->mu);
      if (!c->fs) (void)hipStreamCreateWithFlags(&c->fs, hipStreamNonBlocking);
      fs = c->fs;
    }
    if (fs && hipMemcpyAsync(w, c->sticky, sizeof(w), hipMemcpyDeviceToHost, fs) == hipSuccess)
      (void)hipStreamSynchronize(fs);
    if (!w[TimeoutInfo::kKind]) memcpy(w, seen, sizeof(w));  // (a reset in between: keep what was seen)
  }
  {
    std::lock_guard<std::mutex> lk(c->tmu);
    memcpy(c->timeout, w, sizeof(c->timeout));
  }
  using T = TimeoutInfo;
  fprintf(stderr,
          "[cairo_amd] an in-kernel wait timed out (reported at frame %u): %s; member %d, frame index %d (epoch %u), "
          "MB row %d, waiting on %d (0x%x) for %d, last seen 0x%08x%08x\n",
          index, timeout_kind_name(w[T::kKind]), w[T::kMember], w[T::kIndex], (uint32_t)w[T::kEpoch], w[T::kRow],
          w[T::kOn], (uint32_t)w[T::kOn], w[T::kNeed], (uint32_t)w[T::kSeenHi], (uint32_t)w[T::kSeenLo]);
}

// Frame outputs once its D2H finished (called without mu held).  poll: wait
// with hipEventQuery + short sleeps instead of hipEventSynchronize -- a
// thread blocked in hipEventSynchronize on the copy stream's event stalls
// another thread enqueueing on that stream (the frame pipeline's completion
// thread vs. the submitting thread: measured 0.43 -> 0.8 ms per 720p frame).
static int frame_result(cairo_ctx* c, Stage& s, cairo_frame_result* out, bool poll = false) {
  CK(hipSetDevice(c->device));
  if (poll) {
    for (;;) {
      const hipError_t q = hipEventQuery(s.d2h_done);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) CK(q);
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  } else {
    CK(hipEventSynchronize(s.d2h_done));
  }
  if (s.err[TimeoutInfo::kKind]) {
    report_timeout_host(c, s.err, s.index);
    return kHardwareFail;
  }
  out->block_table = s.table;
  if (c->outputs & CAIRO_OUT_COEF) {
    out->coef_y = s.coef;
    out->coef_u = s.coef + (size_t)c->wa * c->ha;
    out->coef_v = out->coef_u + (size_t)(c->wa / 2) * (c->ha / 2);
  } else {
    out->coef_y = out->coef_u = out->coef_v = nullptr;
  }
  out->feed = nullptr;
  out->feed_bits = 0;
  out->feed_status = CAIRO_FEED_NONE;
  if (c->outputs & CAIRO_OUT_FEED) {
    const int slot = (int)(&s - c->st.data());
    const volatile uint32_t* h = c->feed_host + (size_t)slot * (kFeedHdrWords + c->feed_words);
    out->feed = (const uint32_t*)h + kFeedHdrWords;
    out->feed_bits = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    out->feed_status = h[2] ? CAIRO_FEED_OVERFLOW : CAIRO_FEED_VALID;
    if (!h[2] && h[3]) {  // k_feed_write's bounds guard dropped writes: the feed is not the frame's
      fprintf(stderr, "[cairo_amd] frame %u: the precode writer found %u writes outside the frame's feed\n",
              s.index, (uint32_t)h[3]);
      return kHardwareFail;
    }
  }
  out->wa = c->wa;
  out->ha = c->ha;
  out->wmb = c->wmb;
  out->hmb = c->hmb;
  out->index = s.index;
  out->type = s.type;
  // the controller's choice: k_rate_decide wrote it before the frame's d2h_done
  if (s.rated) s.quality = ((const volatile RateSlot*)c->rate_host)[&s - c->st.data()].quality;
  out->quality = s.quality;
  if (s.mflags || s.rated) {  // (set at its submit, under mu, before this frame could be waited on)
    std::lock_guard<std::mutex> lk(c->mu);
    s.waited = true;  // cairo_ctx_frame_metrics / fetch_recon / frame_rate may be used now
  }
  return kSuccess;
}

int cairo_ctx_wait(cairo_ctx* c, int ticket, cairo_frame_result* out) {
  if (!c || !out || ticket < 0) return kInvalidArg;
  Stage& s = c->st[ticket % c->stages];
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!s.busy || s.ticket != ticket) return kInvalidResource;
    CK(hipSetDevice(c->device));
    if (!s.launched) {
      int r = flush(c);
      if (r) return r;
    }
  }
  return frame_result(c, s, out);
}

int cairo_ctx_decode_frame(cairo_ctx* c, const uint8_t* table, const int16_t* coef, uint32_t index,
                           uint8_t* rgb) {
  return decode_frame(c, table, coef, index, {rgb, kSinkRgb888, 0, nullptr});
}

int cairo_ctx_decode_frame_fmt(cairo_ctx* c, const uint8_t* table, const int16_t* coef, uint32_t index, int fmt,
                               uint32_t pitch, uint8_t* out) {
  if (fmt < 0) return kInvalidArg;
  return decode_frame(c, table, coef, index, {out, fmt, pitch, nullptr});
}

int cairo_ctx_decode_frame_tensor(cairo_ctx* c, const uint8_t* table, const int16_t* coef, uint32_t index, void* base,
                                  const cairo_tensor* desc) {
  if (!desc) return kInvalidArg;
  return decode_frame(c, table, coef, index, {(uint8_t*)base, kSinkRgb888, 0, desc});
}

static int set_color(cairo_ctx* c, int cairo_ctx::*col, int range, int matrix) {
  if (!c || !color_known(range, matrix)) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  c->*col = color_index(range, matrix);  // frames already submitted keep theirs (Pending::col)
  return kSuccess;
}
int cairo_ctx_set_input_color(cairo_ctx* c, int r, int m) { return set_color(c, &cairo_ctx::in_col, r, m); }
int cairo_ctx_set_output_color(cairo_ctx* c, int r, int m) { return set_color(c, &cairo_ctx::out_col, r, m); }

int cairo_ctx_max_workgroups(const cairo_ctx* c) { return c ? c->max_rows : 0; }

int cairo_ctx_timeout_info(cairo_ctx* c, int32_t* out, int n) {
  if (!c || !out || n < 0 || n > TimeoutInfo::kWords) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->tmu);
  memcpy(out, c->timeout, (size_t)n * sizeof(int32_t));
  return kSuccess;
}

int cairo_ctx_set_outputs(cairo_ctx* c, int outputs) {
  if (!c || outputs < 1 || outputs > (CAIRO_OUT_COEF | CAIRO_OUT_FEED)) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->rate_on && !(outputs & CAIRO_OUT_FEED)) return kInvalidArg;  // the controller observes the feed
  CK(hipSetDevice(c->device));
  int r = sync_all(c);  // frames in flight keep the outputs they were launched with
  if (r) return r;
  for (const Stage& s : c->st)
    if (s.busy) return kInvalidResource;
  if ((outputs & CAIRO_OUT_FEED) && !c->feed_host) {
    // all or nothing: a partial allocation would leave feed_dev set with no
    // host buffer for the precode to write into
    const size_t S = (size_t)c->stages;
    const size_t words = feed_words_per_slot(c->mbs);
    uint32_t *dev = nullptr, *hdr = nullptr, *scratch = nullptr, *host = nullptr;
    hipError_t e = hipMalloc(&dev, words * 4 * S);
    if (e == hipSuccess) e = hipMalloc(&hdr, kFeedHdrWords * 4 * S);
    if (e == hipSuccess) e = hipMalloc(&scratch, feed_scratch_words(c->mbs) * 4 * S);
    if (e == hipSuccess) e = hipHostMalloc(&host, (kFeedHdrWords + words) * 4 * S, hipHostMallocMapped);
    if (e != hipSuccess) {
      for (void* q : {(void*)dev, (void*)hdr, (void*)scratch}) (void)hipFree(q);
      if (host) (void)hipHostFree(host);
      return fail(e, "set_outputs: feed buffers");
    }
    c->feed_words = words;
    c->feed_dev = dev, c->feed_hdr = hdr, c->feed_scratch = scratch, c->feed_host = host;
  }
  c->outputs = outputs;
  return kSuccess;
}

int cairo_ctx_fetch_coef(cairo_ctx* c, int ticket, cairo_frame_result* out) {
  if (!c || !out || ticket < 0) return kInvalidArg;
  Stage& s = c->st[ticket % c->stages];
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!s.busy || s.ticket != ticket || !s.launched) return kInvalidResource;
  }
  CK(hipSetDevice(c->device));
  CK(hipEventSynchronize(s.d2h_done));  // the frame's engine launch has finished
  const int slot = ticket % c->stages;
  if (!(c->outputs & CAIRO_OUT_COEF)) {  // still in the staging slot until its release
    {
      std::lock_guard<std::mutex> lk(c->mu);
      if (!c->fs) CK(hipStreamCreateWithFlags(&c->fs, hipStreamNonBlocking));  // rare: made on first use
    }
    CK(hipMemcpyAsync(s.coef, coef_base(c, slot), c->plane_elems * 2, hipMemcpyDeviceToHost, c->fs));
    CK(hipStreamSynchronize(c->fs));
  }
  out->coef_y = s.coef;
  out->coef_u = s.coef + (size_t)c->wa * c->ha;
  out->coef_v = out->coef_u + (size_t)(c->wa / 2) * (c->ha / 2);
  return kSuccess;
}

int cairo_ctx_set_metrics(cairo_ctx* c, int flags) {
  constexpr int kAll = CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM | CAIRO_KEEP_RECON;
  if (!c || flags < 0 || (flags & ~kAll)) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->gsize > 1) return kInvalidArg;  // a mirrored group may use every push target itself
  CK(hipSetDevice(c->device));
  int r = sync_all(c);  // frames in flight keep the setting they were submitted with
  if (r) return r;
  for (const Stage& s : c->st)
    if (s.busy) return kInvalidResource;
  if (flags) flags |= CAIRO_KEEP_RECON;
  if (flags && !c->keep) {  // all or nothing
    const size_t S = (size_t)c->stages;
    int16_t* keep = nullptr;
    MetricsPartial* part = nullptr;
    cairo_frame_metrics* host = nullptr;
    hipError_t e = hipMalloc(&keep, c->plane_elems * 2 * S);
    if (e == hipSuccess) e = hipMalloc(&part, sizeof(MetricsPartial) * 3 * metrics_tiles((int)c->w, (int)c->h) * S);
    if (e == hipSuccess) e = hipHostMalloc(&host, sizeof(cairo_frame_metrics) * S, hipHostMallocMapped);
    cairo_frame_metrics* dev = nullptr;
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dev, host, 0);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(keep);
      (void)hipFree(part);
      if (host) (void)hipHostFree(host);
      fprintf(stderr, "[cairo_amd] set_metrics: %s (%zu bytes of kept reconstructions)\n", hipGetErrorString(e),
              c->plane_elems * 2 * S);
      return e == hipErrorOutOfMemory ? kOutOfMemory : kHardwareFail;
    }
    memset(host, 0, sizeof(cairo_frame_metrics) * S);
    c->keep = keep, c->met_part = part, c->met_host = host, c->met_dev = dev;
  } else if (!flags && c->keep) {  // nothing is in flight: back to the path without a keep
    (void)hipFree(c->keep);
    (void)hipFree(c->met_part);
    (void)hipHostFree(c->met_host);
    c->keep = nullptr, c->met_part = nullptr, c->met_host = nullptr, c->met_dev = nullptr;
  }
  c->metrics = flags;
  return kSuccess;
}

// The stage of a waited, unreleased, encoded frame that was submitted with a
// keep (mu held); nullptr otherwise.
static Stage* kept_stage(cairo_ctx* c, int ticket) {
  if (ticket < 0) return nullptr;
  Stage& s = c->st[ticket % c->stages];
  if (s.ticket != ticket || !s.busy || !s.waited || !s.mflags || !c->keep) return nullptr;
  return &s;
}

int cairo_ctx_frame_metrics(cairo_ctx* c, int ticket, cairo_frame_metrics* out) {
  if (!c || !out) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  const Stage* s = kept_stage(c, ticket);
  if (!s || !(s->mflags & (CAIRO_METRIC_SSE | CAIRO_METRIC_SSIM))) return kInvalidArg;
  // written by k_metrics_finish before the frame's d2h_done, which its wait saw
  memcpy(out, (const void*)(c->met_host + ticket % c->stages), sizeof(*out));
  return kSuccess;
}

int cairo_ctx_set_rate(cairo_ctx* c, const cairo_rate* cfg) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  // a refused call changes nothing: no flush before the checks (a pending
  // frame's stage is busy, so nothing is pending once they pass)
  if (cfg && (!rate_cfg_ok(cfg) || !(c->outputs & CAIRO_OUT_FEED) || c->gsize > 1)) return kInvalidArg;
  for (const Stage& s : c->st)
    if (s.busy) return kInvalidResource;
  CK(hipSetDevice(c->device));
  int r = sync_all(c);  // released, unwaited frames may still run
  if (r) return r;
  if (!cfg) {
    c->rate_on = false;  // the buffers stay until the context goes
    return kSuccess;
  }
  if (!c->rate_host) {  // all or nothing
    const size_t S = (size_t)c->stages;
    cairo_rate_state* state = nullptr;
    RateSlot *dev = nullptr, *host = nullptr, *host_dev = nullptr;
    uint32_t* part = nullptr;
    hipError_t e = hipMalloc(&state, sizeof(cairo_rate_state));
    if (e == hipSuccess) e = hipMalloc(&dev, sizeof(RateSlot) * S);
    if (e == hipSuccess) e = hipMalloc(&part, sizeof(uint32_t) * kRateBlocks * S);
    if (e == hipSuccess) e = hipHostMalloc(&host, sizeof(RateSlot) * S, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&host_dev, host, 0);
    if (e == hipSuccess) e = hipMemset(dev, 0, sizeof(RateSlot) * S);
    if (e != hipSuccess) {
      for (void* q : {(void*)state, (void*)dev, (void*)part}) (void)hipFree(q);
      if (host) (void)hipHostFree(host);
      return fail(e, "set_rate: controller buffers");
    }
    memset(host, 0, sizeof(RateSlot) * S);
    c->rate_state = state, c->rate_dev = dev, c->rate_part = part, c->rate_host = host, c->rate_host_dev = host_dev;
  }
  r = restart_rate(c);
  if (r) return r;
  c->rate_cfg = *cfg;
  c->rate_on = true;
  return kSuccess;
}

int cairo_ctx_frame_rate(cairo_ctx* c, int ticket, cairo_rate_info* info) {
  if (!c || !info || ticket < 0) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  const Stage& s = c->st[ticket % c->stages];
  if (s.ticket != ticket || !s.busy || !s.waited || !s.rated || !c->rate_host) return kInvalidArg;
  // written by k_rate_decide and k_rate_finish before the frame's d2h_done, which its wait saw
  RateSlot r;
  memcpy(&r, (const void*)(c->rate_host + ticket % c->stages), sizeof(r));
  info->quality = r.quality;
  info->overflow = r.overflow;
  info->feed_bits = r.nbits;
  info->ones = r.ones;
  info->est_bits = rate_frame_bits(r.nbits, r.ones, r.overflow, c->rate_cfg.target_bits);
  info->aim = r.aim;
  info->debt = r.debt;
  return kSuccess;
}

int cairo_ctx_fetch_recon_planes(cairo_ctx* c, int ticket, int16_t* y, int16_t* u, int16_t* v) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!kept_stage(c, ticket)) return kInvalidArg;
  CK(hipSetDevice(c->device));
  if (!c->fs) CK(hipStreamCreateWithFlags(&c->fs, hipStreamNonBlocking));
  const PlaneSet p = slot_planes(c->keep, c, ticket % c->stages);
  const size_t ly = (size_t)c->wa * c->ha, lc = ly / 4;
  if (y) CK(hipMemcpyAsync(y, p.y, ly * 2, hipMemcpyDeviceToHost, c->fs));
  if (u) CK(hipMemcpyAsync(u, p.u, lc * 2, hipMemcpyDeviceToHost, c->fs));
  if (v) CK(hipMemcpyAsync(v, p.v, lc * 2, hipMemcpyDeviceToHost, c->fs));
  CK(hipStreamSynchronize(c->fs));
  return kSuccess;
}

// cairo_ctx_fetch_recon and _fetch_recon_tensor (mu held, the sink checked):
// the ticket's kept planes as out.fmt into the slot's frame buffer -- its own frame
// was converted before the wait, and the next upload into it follows the
// ticket's release -- and from there to the sink.
static int fetch_kept(cairo_ctx* c, int ticket, const FrameSink& out) {
  if (!c->fs) CK(hipStreamCreateWithFlags(&c->fs, hipStreamNonBlocking));
  const int slot = ticket % c->stages;
  int r = stage_planes(c, slot_planes(c->keep, c, slot), slot, out.fmt, c->fs);
  if (!r) r = write_staged(c, slot, out, c->fs);
  if (r) return r;
  CK(hipStreamSynchronize(c->fs));
  return kSuccess;
}

int cairo_ctx_fetch_recon(cairo_ctx* c, int ticket, int fmt, uint32_t pitch, uint8_t* out) {
  if (!c || !out || cairo_frame_layout(fmt, c->w, c->h, pitch, nullptr, nullptr) != kSuccess) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!kept_stage(c, ticket)) return kInvalidArg;
  CK(hipSetDevice(c->device));
  return fetch_kept(c, ticket, {out, fmt, pitch, nullptr});
}

int cairo_ctx_fetch_recon_tensor(cairo_ctx* c, int ticket, void* base, const cairo_tensor* desc) {
  if (!c || !base || !desc) return kInvalidArg;
  uint64_t span = 0;
  if (tensor_check(desc, base, c->w, c->h, &span) != kSuccess) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!kept_stage(c, ticket)) return kInvalidArg;
  CK(hipSetDevice(c->device));
  if (!device_span(c, base, span, "fetch_recon_tensor")) return kInvalidArg;
  // tight RGB24 through k_planes_to_fmt, as cairo_ctx_fetch_recon stages it
  return fetch_kept(c, ticket, {(uint8_t*)base, CAIRO_FMT_RGB24, 0, desc});
}

int cairo_ctx_flush(cairo_ctx* c) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  return flush(c);
}

int cairo_ctx_peer_info(cairo_ctx* c, int cross_device, cairo_peer* out) {
  if (!c || !out) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!c->fresh || c->npend || c->gsize > 1) return kInvalidResource;  // before any frame, outside a group
  CK(hipSetDevice(c->device));
  if (cross_device && !c->fine_grained) {
    // Memory another device reads while this one writes it: fine-grained, so
    // that system-scope releases and acquires order it across devices.
    const size_t S = (size_t)c->stages;
    int16_t* ring = nullptr;
    int16_t* coef[CAIRO_MAX_COEF_CHUNKS] = {};
    int chunks = 0, per = 0;
    uint64_t* prog = nullptr;
    hipError_t e = hipExtMallocWithFlags((void**)&ring, c->plane_elems * 2 * kMirrorSlots, hipDeviceMallocFinegrained);
    if (e == hipSuccess) e = alloc_coef(c, true, coef, &chunks, &per);
    if (e == hipSuccess)
      e = hipExtMallocWithFlags((void**)&prog, (size_t)c->hmb * sizeof(uint64_t) * S, hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
      for (void* q : {(void*)ring, (void*)prog}) (void)hipFree(q);
      for (int16_t* q : coef)
        if (q) (void)hipFree(q);
      return fail(e, "hipExtMallocWithFlags(fine-grained)");
    }
    int r0 = sync_all(c);  // nothing is in flight (fresh), but the zeroing memsets may be
    if (r0) return r0;
    (void)hipFree(c->ring_buf);
    for (int16_t*& q : c->coef) {
      if (q) (void)hipFree(q);
      q = nullptr;
    }
    (void)hipFree(c->progress);
    c->ring_buf = ring, c->progress = prog;
    c->ring_slots = kMirrorSlots;
    for (int k = 0; k < CAIRO_MAX_COEF_CHUNKS; k++) c->coef[k] = coef[k];
    c->coef_chunks = chunks, c->coef_per = per;
    c->fine_grained = true;
    int r = zero_state(c);
    if (r) return r;
  }
  memset(out, 0, sizeof(*out));
  out->width = c->w, out->height = c->h, out->ring = c->ring;
  out->device = c->device;
  out->pid = (int32_t)getpid();
  out->stages = c->stages;
  out->fine_grained = c->fine_grained;
  out->coef_chunks = c->coef_chunks;
  out->coef_chunk_slots = c->coef_per;
  out->ring_addr = (uint64_t)(uintptr_t)c->ring_buf;
  out->progress_addr = (uint64_t)(uintptr_t)c->progress;
  hipIpcMemHandle_t h;
  static_assert(sizeof(h) == sizeof(out->ipc_ring), "IPC handle size");
  CK(hipIpcGetMemHandle(&h, c->ring_buf));
  memcpy(out->ipc_ring, &h, sizeof(h));
  CK(hipIpcGetMemHandle(&h, c->progress));
  memcpy(out->ipc_progress, &h, sizeof(h));
  for (int k = 0; k < c->coef_chunks; k++) {
    out->coef_addr[k] = (uint64_t)(uintptr_t)c->coef[k];
    CK(hipIpcGetMemHandle(&h, c->coef[k]));
    memcpy(out->ipc_coef[k], &h, sizeof(h));
  }
  return kSuccess;
}

int cairo_peer_size(void) { return (int)sizeof(cairo_peer); }

// GPU_MAX_HW_QUEUES as the HIP runtime reads it: once, when it starts.  Read
// here when the library is loaded (before any HIP call of ours); setting it
// later in the process (os.environ after torch started HIP) changes nothing.
static const int g_hw_queues = [] {
  const char* env = getenv("GPU_MAX_HW_QUEUES");
  return env && *env ? atoi(env) : 4;
}();

int cairo_group_check_queues(int local_members, int hw_queues) {
  // Members in one process on one device share that process's hardware
  // queues (GPU_MAX_HW_QUEUES, HIP's default 4).  Each member keeps two launch
  // streams and a copy stream busy; when two members' persistent launches
  // land in one in-order queue, the later cannot start until the earlier
  // ends, which waits on it: a deadlock the bounded in-kernel waits would
  // only report as EVX_ERROR_HARDWAREFAIL after 2 s.  Refuse up front.
  if (local_members < 2) return kSuccess;
  const int have = hw_queues >= 0 ? hw_queues : g_hw_queues;
  const int need = 3 * local_members + 2;
  if (need > 32 || have < need) {
    fprintf(stderr,
            "[cairo_amd] join_group: %d members share this process and device; they need GPU_MAX_HW_QUEUES >= %d "
            "(have %d, at most 32); run one process per member, or set GPU_MAX_HW_QUEUES before the first HIP call\n",
            local_members, need, have);
    return kInvalidArg;
  }
  return kSuccess;
}

// cairo_ctx_join_group: another member's buffers as this member addresses them.
static int map_peer(cairo_ctx* c, cairo_ctx::Peer& q, const cairo_peer& p, bool same_process) {
  if (p.coef_chunks < 1 || p.coef_chunks > CAIRO_MAX_COEF_CHUNKS || p.coef_chunk_slots < 1 ||
      (long)p.coef_chunks * p.coef_chunk_slots < p.stages)
    return kInvalidArg;
  q.coef_chunks = p.coef_chunks, q.coef_per = p.coef_chunk_slots;
  if (same_process) {  // the addresses are valid here
    if (p.device != c->device) {
      const hipError_t e = hipDeviceEnablePeerAccess(p.device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(e, "hipDeviceEnablePeerAccess");
    }
    q.ring = (int16_t*)(uintptr_t)p.ring_addr;
    q.progress = (uint64_t*)(uintptr_t)p.progress_addr;
    for (int k = 0; k < p.coef_chunks; k++) q.coef[k] = (int16_t*)(uintptr_t)p.coef_addr[k];
    return kSuccess;
  }
  // another process: open its IPC handles (peer access over xGMI), each allocation < 1 GiB
  q.imported = true;
  auto open = [&](const uint8_t* bytes, void** dst) {
    hipIpcMemHandle_t h;
    memcpy(&h, bytes, sizeof(h));
    return hipIpcOpenMemHandle(dst, h, hipIpcMemLazyEnablePeerAccess);
  };
  hipError_t e = open(p.ipc_ring, (void**)&q.ring);
  if (e == hipSuccess) e = open(p.ipc_progress, (void**)&q.progress);
  for (int k = 0; e == hipSuccess && k < p.coef_chunks; k++) e = open(p.ipc_coef[k], (void**)&q.coef[k]);
  return fail(e, "hipIpcOpenMemHandle");
}

int cairo_ctx_join_group(cairo_ctx* c, int size, int rank, const cairo_peer* peers) {
  if (!c || !peers || size < 1 || size > kMaxGroup || rank < 0 || rank >= size) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!c->fresh || c->npend || c->gsize > 1) return kInvalidResource;
  if (c->metrics) return kInvalidArg;  // a member's deblock pushes to its mirrors, not to a keep
  if (c->rate_on) return kInvalidArg;  // the controller sees one context's launches, not the stream's
  CK(hipSetDevice(c->device));
  if (size == 1) return kSuccess;
  const pid_t me = getpid();
  bool sys = false;
  int local = 0;  // members in this process on this device, this one included
  for (int i = 0; i < size; i++) {
    const cairo_peer& p = peers[i];
    if (p.width != c->w || p.height != c->h || p.ring != c->ring || p.stages < 2) return kInvalidArg;
    if (i == rank || (p.pid == me && p.device == c->device)) local++;
    if (i == rank) continue;
    if (p.pid != me || p.device != c->device) sys = true;
    if (p.device != c->device || p.pid != me) {
      if (!p.fine_grained || !c->fine_grained) {
        fprintf(stderr, "[cairo_amd] group members on other devices or processes need cairo_ctx_peer_info(..., 1)\n");
        return kInvalidArg;
      }
    }
  }
  if (cairo_group_check_queues(local, -1) != kSuccess) return kInvalidArg;
  for (int i = 0; i < size; i++) {
    cairo_ctx::Peer& q = c->gp[i];
    const cairo_peer& p = peers[i];
    q.stages = p.stages;
    if (i == rank) {
      q.ring = c->ring_buf, q.progress = c->progress;
      for (int k = 0; k < CAIRO_MAX_COEF_CHUNKS; k++) q.coef[k] = c->coef[k];
      q.coef_chunks = c->coef_chunks, q.coef_per = c->coef_per;
      continue;
    }
    const int r = map_peer(c, q, p, p.pid == me);
    if (r) {  // leave_group closes whatever is open: the members before this one, and its own imports
      c->gsize = q.imported ? i + 1 : i;
      leave_group(c);
      return r;
    }
  }
  c->gsize = size;
  c->grank = rank;
  c->gbase = c->next_ticket;
  // (CAIRO_GROUP_FORCE_SYS: system-scope hand-offs in one process too, to
  // time their cost on one device)
  c->sys = sys || getenv("CAIRO_GROUP_FORCE_SYS") != nullptr;
  CK(hipMalloc(&c->zero, c->plane_elems * 2));
  CK(hipMemset(c->zero, 0, c->plane_elems * 2));
  // a member's consecutive frames are N stream frames apart
  return upload_orders(c, 3 * size + 2);
}

int cairo_ctx_release(cairo_ctx* c, int ticket) {
  if (!c || ticket < 0) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  Stage& s = c->st[ticket % c->stages];
  if (s.ticket != ticket) return kInvalidResource;
  s.busy = false;
  return kSuccess;
}

int cairo_ctx_sync(cairo_ctx* c) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  return sync_all(c);
}

int cairo_ctx_read_planes(cairo_ctx* c, int which, int16_t* y, int16_t* u, int16_t* v) {
  if (!c || which < 0 || which >= 2 + c->ring_slots) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  if (which < 2 && c->last_slot < 0) return kInvalidResource;
  PlaneSet p = which == 0 ? slot_planes(c->src, c, c->last_slot)
               : which == 1 ? coef_planes(c, c->last_slot)
                            : slot_planes(c->ring_buf, c, which - 2);
  const size_t ly = (size_t)c->wa * c->ha, lc = ly / 4;
  if (y) CK(hipMemcpy(y, p.y, ly * 2, hipMemcpyDeviceToHost));
  if (u) CK(hipMemcpy(u, p.u, lc * 2, hipMemcpyDeviceToHost));
  if (v) CK(hipMemcpy(v, p.v, lc * 2, hipMemcpyDeviceToHost));
  return kSuccess;
}

int cairo_ctx_read_inter(cairo_ctx* c, uint8_t* descs, int32_t* sads) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  if (c->last_slot < 0) return kInvalidResource;
  const size_t n = c->mbs * (c->ring > 1 ? c->ring - 1 : 0);
  if (!n) return kSuccess;
  const size_t o = (size_t)c->last_slot * c->nref * c->mbs;
  // two tagged granules per record (kernels.h pack_inter_desc); a record
  // whose tag is not the last frame's epoch is stale (an intra or decoded
  // frame has none): refused, not returned as current
  std::vector<uint64_t> g(2 * n);
  CK(hipMemcpy(g.data(), c->idesc + o, n * sizeof(BlockDesc), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < 2 * n; i++)
    if ((uint32_t)(g[i] >> 32) != c->last_epoch) return kInvalidResource;
  for (size_t i = 0; i < n; i++) {
    if (descs) {
      const BlockDesc d = unpack_inter_desc((uint32_t)g[2 * i]);
      memcpy(descs + i * sizeof(BlockDesc), &d, sizeof(d));
    }
    if (sads) sads[i] = (int32_t)(uint32_t)g[2 * i + 1];
  }
  return kSuccess;
}

int cairo_ctx_set_debug(cairo_ctx* c, int flags) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = flush(c);
  if (r) return r;
  if ((flags & 1) && !c->predeblock) CK(hipMalloc(&c->predeblock, c->plane_elems * 2));
  if ((flags & 2) && !c->stamps) CK(hipMalloc(&c->stamps, stamp_words(c) * sizeof(uint64_t)));
  if ((flags & 4) && !c->trace_host) {
    CK(hipHostMalloc(&c->trace_host, 4096 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->trace_host, 0xFF, 4096 * sizeof(int32_t));
    CK(hipHostGetDevicePointer((void**)&c->trace_dev, c->trace_host, 0));
  }
  if (flags & 8) {
    int32_t mark[TimeoutInfo::kWords] = {};  // a complete, claimed record
    mark[TimeoutInfo::kKind] = kWaitHostMark;
    mark[TimeoutInfo::kClaim] = 1;
    CK(hipMemcpy(c->sticky, mark, sizeof(mark), hipMemcpyHostToDevice));
  }
  c->inject = (flags & 16) ? 1 : 0;
  if ((flags & 32) && !c->acct) {
    CK(hipMalloc(&c->acct, kAcctShards * kAcctWords * sizeof(uint64_t)));
    CK(hipMemset(c->acct, 0, kAcctShards * kAcctWords * sizeof(uint64_t)));
  }
  return kSuccess;
}

int cairo_ctx_read_acct(cairo_ctx* c, uint64_t* out, int n, int reset) {
  if (!c || !out || n < 0 || n > kAcctWords) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  memset(out, 0, (size_t)n * sizeof(uint64_t));
  if (!c->acct) return kSuccess;
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  std::vector<uint64_t> v((size_t)kAcctShards * kAcctWords);
  CK(hipMemcpy(v.data(), c->acct, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < kAcctShards; s++)
    for (int k = 0; k < n; k++) out[k] += v[(size_t)s * kAcctWords + k];
  if (reset) CK(hipMemset(c->acct, 0, v.size() * sizeof(uint64_t)));
  return kSuccess;
}

// Diagnostic: the live trace words (no synchronization; readable while the engine runs).
int cairo_ctx_read_trace(cairo_ctx* c, int32_t* out, int n) {
  if (!c || !c->trace_host || !out || n < 0 || n > 4096) return kInvalidArg;
  memcpy(out, (const void*)c->trace_host, n * sizeof(int32_t));
  return kSuccess;
}

int cairo_ctx_read_stamps(cairo_ctx* c, uint64_t* out) {
  if (!c || !c->stamps || !out) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  CK(hipMemcpy(out, c->stamps, stamp_words(c) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return kSuccess;
}

int cairo_ctx_engine_variant(cairo_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  return c->engine_variant;
}

int cairo_ctx_read_predeblock(cairo_ctx* c, int16_t* y, int16_t* u, int16_t* v) {
  if (!c || !c->predeblock) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  PlaneSet p = planes_at(c->predeblock, c);
  const size_t ly = (size_t)c->wa * c->ha, lc = ly / 4;
  if (y) CK(hipMemcpy(y, p.y, ly * 2, hipMemcpyDeviceToHost));
  if (u) CK(hipMemcpy(u, p.u, lc * 2, hipMemcpyDeviceToHost));
  if (v) CK(hipMemcpy(v, p.v, lc * 2, hipMemcpyDeviceToHost));
  return kSuccess;
}

int cairo_ctx_read_table(cairo_ctx* c, uint8_t* table) {
  if (!c || !table) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  int r = sync_all(c);
  if (r) return r;
  if (c->last_slot < 0) return kInvalidResource;
  CK(hipMemcpy(table, c->table + (size_t)c->last_slot * c->mbs, c->mbs * sizeof(BlockDesc),
               hipMemcpyDeviceToHost));
  return kSuccess;
}

int cairo_kat_transform(const int16_t* src, const int16_t* pred, const uint8_t* qtype, int count,
                        int16_t* coef, int16_t* recon, int32_t* qvar, int device) {
  if (!src || !pred || !qtype || !coef || !recon || !qvar || count <= 0) return kInvalidArg;
  CK(hipSetDevice(device));
  const size_t n = (size_t)count * 384;
  KatBuffer ds, dp, dc, dr, dq, dv;
  int r;
  if ((r = ds.alloc(n * 2)) || (r = dp.alloc(n * 2)) || (r = dc.alloc(n * 2)) || (r = dr.alloc(n * 2)) ||
      (r = dq.alloc((size_t)count * 2)) || (r = dv.alloc((size_t)count * 8)) || (r = ds.upload(src, n * 2)) ||
      (r = dp.upload(pred, n * 2)) || (r = dq.upload(qtype, (size_t)count * 2)) ||
      (r = kat_run(launch_kat_transform(ds.as<int16_t>(), dp.as<int16_t>(), dc.as<int16_t>(), dr.as<int16_t>(),
                                        dq.as<uint8_t>(), dv.as<int32_t>(), count, nullptr),
                   "kat")) ||
      (r = dc.download(coef, n * 2)) || (r = dr.download(recon, n * 2)) || (r = dv.download(qvar, (size_t)count * 8)))
    return r;
  return kSuccess;
}

int cairo_kat_quant(const int16_t* coef, const uint8_t* tq, int count, int16_t* quant, int16_t* dequant,
                    int device) {
  if (!coef || !tq || !quant || !dequant || count < 1) return kInvalidArg;
  for (int m = 0; m < count; m++)
    if ((tq[2 * m] & kCopy) || tq[2 * m + 1] < 1 || tq[2 * m + 1] > 31) return kInvalidArg;
  CK(hipSetDevice(device));
  const size_t n = (size_t)count * 384;
  KatBuffer dc, dt, dq, dd;
  int r;
  if ((r = dc.alloc(n * 2)) || (r = dt.alloc((size_t)count * 2)) || (r = dq.alloc(n * 2)) || (r = dd.alloc(n * 2)) ||
      (r = dc.upload(coef, n * 2)) || (r = dt.upload(tq, (size_t)count * 2)) ||
      (r = kat_run(launch_kat_quant(dc.as<int16_t>(), dt.as<uint8_t>(), dq.as<int16_t>(), dd.as<int16_t>(), count,
                                    nullptr),
                   "kat_quant")) ||
      (r = dq.download(quant, n * 2)) || (r = dd.download(dequant, n * 2)))
    return r;
  return kSuccess;
}

int cairo_kat_precode(uint32_t wmb, uint32_t hmb, uint32_t ring, int count, int nslots, const int32_t* slot,
                      const uint8_t* tables, const int16_t* coef_y, const int16_t* coef_u, const int16_t* coef_v,
                      uint32_t prefill, uint32_t* hdr, uint32_t* feed, uint64_t feed_words, uint32_t* guard,
                      uint32_t guard_words, int device) {
  if (!slot || !tables || !coef_y || !coef_u || !coef_v || !hdr || (!feed && feed_words) || (!guard && guard_words) ||
      count < 1 || count > kMaxBatch || nslots < count || nslots > kMaxBatch || !wmb || !hmb ||
      (uint64_t)wmb * hmb > 65535u || ring < 1 || ring > (uint32_t)kMaxRing)
    return kInvalidArg;
  for (int j = 0; j < count; j++) {
    if (slot[j] < 0 || slot[j] >= nslots) return kInvalidArg;
    for (int i = 0; i < j; i++)
      if (slot[i] == slot[j]) return kInvalidArg;
  }
  CK(hipSetDevice(device));
  const size_t mbs = (size_t)wmb * hmb, ny = mbs * 256, nc = mbs * 64, ne = ny + 2 * nc;
  const size_t stride = feed_words_per_slot(mbs), sw = feed_scratch_words(mbs), hw = kFeedHdrWords + stride;
  const size_t take = feed_words < stride ? (size_t)feed_words : stride;
  KatBuffer dt, dc, dfa, dfeed, dhdr, dscr, dhost;  // dhost stands for the frames' mapped pinned host buffers
  int r;
  if ((r = dt.alloc(count * mbs * sizeof(BlockDesc))) || (r = dc.alloc(count * ne * 2)) ||
      (r = dfa.alloc(count * sizeof(FrameArgs))) || (r = dfeed.alloc(nslots * stride * 4)) ||
      (r = dhdr.alloc((size_t)nslots * kFeedHdrWords * 4)) || (r = dscr.alloc(nslots * sw * 4)) ||
      (r = dhost.alloc(count * hw * 4)) || (r = dt.upload(tables, count * mbs * sizeof(BlockDesc))))
    return r;
  // the views: only what the precode reads of them
  std::vector<FrameArgs> views((size_t)count);
  FeedArgs fa;
  memset(&fa, 0, sizeof(fa));
  for (int j = 0; j < count; j++) {
    int16_t* base = dc.as<int16_t>() + (size_t)j * ne;
    if ((r = dc.upload(coef_y + (size_t)j * ny, ny * 2, (size_t)j * ne * 2)) ||
        (r = dc.upload(coef_u + (size_t)j * nc, nc * 2, ((size_t)j * ne + ny) * 2)) ||
        (r = dc.upload(coef_v + (size_t)j * nc, nc * 2, ((size_t)j * ne + ny + nc) * 2)))
      return r;
    FrameArgs& a = views[(size_t)j];
    memset((void*)&a, 0, sizeof(a));
    a.wa = (int)wmb * 16, a.ha = (int)hmb * 16, a.wmb = (int)wmb, a.hmb = (int)hmb, a.ring = (int)ring;
    a.table = dt.as<BlockDesc>() + (size_t)j * mbs;
    a.coef = PlaneSet{base, base + ny, base + ny + nc};
    fa.slot[j] = slot[j];
    fa.host[j] = dhost.as<uint32_t>() + (size_t)j * hw;
  }
  if ((r = dfa.upload(views.data(), count * sizeof(FrameArgs)))) return r;
  // what the slots held before: every feed word, header, scratch word and host word
  CK(hipMemsetD32(dfeed.as<void>(), (int)prefill, nslots * stride));
  CK(hipMemsetD32(dhdr.as<void>(), (int)prefill, (size_t)nslots * kFeedHdrWords));
  CK(hipMemsetD32(dscr.as<void>(), (int)prefill, nslots * sw));
  CK(hipMemsetD32(dhost.as<void>(), (int)prefill, count * hw));
  // the launch as enqueue_results makes it (no table or timeout hand-over)
  fa.nframes = count;
  fa.fa = dfa.as<FrameArgs>();
  fa.scratch = dscr.as<uint32_t>();
  fa.scratch_stride = sw;
  fa.feed = dfeed.as<uint32_t>();
  fa.feed_stride = stride;
  fa.hdr = dhdr.as<uint32_t>();
  if ((r = fail(launch_precode(fa, (int)mbs, nullptr), "precode")) ||
      (r = kat_run(launch_feed_copy(fa, nullptr), "k_feed_copy")))
    return r;
  for (int j = 0; j < count; j++) {
    uint32_t* h = hdr + (size_t)j * kFeedHdrWords;
    if ((r = dhost.download(h, kFeedHdrWords * 4, (size_t)j * hw * 4)) ||
        (take && (r = dhost.download(feed + (size_t)j * feed_words, take * 4, ((size_t)j * hw + kFeedHdrWords) * 4))))
      return r;
    for (size_t i = take; i < feed_words; i++) feed[(size_t)j * feed_words + i] = prefill;
    // the slot's device words from the frame's end on (from word 0 where nothing was written)
    const uint64_t bits = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    const uint64_t end = h[2] ? 0 : (bits + 31) / 32;
    const size_t n = end >= stride ? 0 : (stride - end < guard_words ? (size_t)(stride - end) : guard_words);
    uint32_t* g = guard + (size_t)j * guard_words;
    if (n && (r = dfeed.download(g, n * 4, ((size_t)slot[j] * stride + end) * 4))) return r;
    for (size_t i = n; i < guard_words; i++) g[i] = prefill;
  }
  return kSuccess;
}

int cairo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* cairo_version(void) { return "cairo_amd 0.1 (gfx950)"; }
int cairo_api_version(void) { return CAIRO_AMD_API_VERSION; }

}  // extern "C"

namespace cairo {

// Every cairo_ctx_submit* and cairo_stream_submit* call.  A scaled frame
// (src.base: a device frame of the source's size and pitch) and a tensor frame
// (src.base: element (0, 0, 0) of a device tensor) are recorded as frames whose
// f.rgb is their staging slot, tight, which the launch's pre-pass fills from
// the source (flush: k_scale_batch, k_tensor_pack_batch); a source that is both
// (a tensor of the source's size) by k_tensor_scale_batch.
int submit_frame(cairo_ctx* c, const FrameSource& src, uint32_t index, uint32_t type, uint32_t quality,
                 int* ticket) {
  const uint8_t* rgb = src.base;
  if (!c || !rgb || !ticket || quality < 1 || quality > 31 || type > 1) return kInvalidArg;
  const Pending::Kind kind = src.tensor ? (src.scaled ? Pending::kTensorScaled : Pending::kTensor)
                             : src.scaled ? Pending::kScaled
                             : src.on_device ? Pending::kDevice : Pending::kStaged;
  const char* who = src.tensor ? (src.scaled ? "submit_tensor_scaled" : "submit_tensor")
                    : src.scaled ? "submit_scaled" : "submit";
  uint64_t frame_bytes = 0;  // of the source as it lies in memory (a tensor's span)
  uint32_t tight = 3 * c->w;
  ScaleFrame plan{};
  TensorScaleFrame tplan{};
  if (kind == Pending::kTensorScaled) {
    // the tensor has the source's size; the slot gets the tight RGB24 frame of the context's
    if (tensor_scale_plan(src.tensor, rgb, src.scaled, c->w, c->h, nullptr, &frame_bytes, &tplan) != kSuccess)
      return kInvalidArg;
  } else if (kind == Pending::kTensor) {
    if (tensor_check(src.tensor, rgb, c->w, c->h, &frame_bytes) != kSuccess) return kInvalidArg;
  } else if (kind == Pending::kScaled) {
    // (the scaler's grid has a row per plane row: at most 65535)
    const cairo_source& sc = *src.scaled;
    if (2ull * c->h > 65535 || scale_plan(src.fmt, src.pitch, &sc, c->w, c->h, rgb, nullptr, &plan) != kSuccess ||
        cairo_frame_layout(src.fmt, sc.width, sc.height, src.pitch, &frame_bytes, nullptr) != kSuccess ||
        cairo_frame_layout(src.fmt, c->w, c->h, 0, nullptr, &tight) != kSuccess)
      return kInvalidArg;
  } else if (cairo_frame_layout(src.fmt, c->w, c->h, src.pitch, &frame_bytes, &tight) != kSuccess) {
    return kInvalidArg;
  } else if (kind == Pending::kDevice && src.fmt == CAIRO_FMT_P010 && ((uintptr_t)rgb & 1)) {
    return kInvalidArg;  // 16-bit samples are read as such
  }
  std::lock_guard<std::mutex> lk(c->mu);
  CK(hipSetDevice(c->device));
  const int t = c->next_ticket, slot = t % c->stages;
  Stage& s = c->st[slot];
  if (s.busy) {
    fprintf(stderr, "[cairo_amd] staging slot of ticket %d not released\n", s.ticket);
    return kInvalidResource;
  }
  if (kind != Pending::kStaged && !device_span(c, rgb, src.check_range ? frame_bytes : 0, who)) return kInvalidArg;
  if (c->gsize > 1 && (long)index != (long)(t - c->gbase) * c->gsize + c->grank) {
    fprintf(stderr, "[cairo_amd] group member %d of %d: frame %u out of turn\n", c->grank, c->gsize, index);
    return kInvalidArg;
  }
  Pending& p = c->pend[c->npend];
  memset(&p, 0, sizeof(p));  // the whole record: nothing is left of the index's previous frame
  FrameDesc& f = p.f;
  p.kind = kind;
  p.fmt = (uint8_t)src.fmt;
  p.pitch = kind == Pending::kDevice && src.pitch ? src.pitch : tight;  // whatever is staged is staged tight
  p.hpitch = src.pitch;
  // (the YUV formats: YUY2, UYVY and P010 are described as the NV12 frame they fold to)
  p.col = src.fmt != CAIRO_FMT_RGB24 && src.fmt != CAIRO_FMT_BGR24 ? (uint8_t)c->in_col : 0;
  f.rgb = kind == Pending::kDevice ? rgb : slot_rgb(c, slot);
  if (kind == Pending::kScaled) {
    plan.dst = slot_rgb(c, slot);
    p.scale = plan;
  } else if (kind == Pending::kTensorScaled) {
    tplan.rgb = slot_rgb(c, slot);
    p.tscale = tplan;
  } else if (kind == Pending::kTensor) {
    p.tens = TensorFrame{const_cast<uint8_t*>(rgb), slot_rgb(c, slot), *src.tensor};
  } else if (kind == Pending::kStaged) {
    const int r = stage_host_frame(c, s, p, rgb);
    if (r) return r;
  }
  f.index = (int)index;
  f.inter = type == 1 ? 1 : 0;
  f.quality = (int)quality;
  // granule tag; frames of a stream have consecutive epochs (a group numbers
  // them by stream index)
  f.epoch = c->gsize > 1 ? index + 1 : ++c->epoch;
  f.slot = slot;
  f.member = c->grank;
  frame_links(c, f, t);
  c->npend++;
  take_stage(s, t, index, type, quality, c->metrics);
  s.rated = c->rate_on;
  c->next_ticket++;
  *ticket = t;
  if (c->npend >= c->batch_max) return flush(c);
  return kSuccess;
}

// Every cairo_ctx_decode_frame* call: the decode-mode engine reconstructs the
// frame into its ring slot, stage_planes writes it into the staging slot in
// the sink's format, write_staged takes it to the caller.
int decode_frame(cairo_ctx* c, const uint8_t* table, const int16_t* coef, uint32_t index, const FrameSink& out) {
  if (!c || !table || !coef || !out.base) return kInvalidArg;
  uint64_t span = 0;
  if (out.tensor && tensor_check(out.tensor, out.base, c->w, c->h, &span) != kSuccess) return kInvalidArg;
  if (out.fmt >= 0 && cairo_frame_layout(out.fmt, c->w, c->h, out.pitch, nullptr, nullptr) != kSuccess)
    return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->gsize > 1) return kInvalidResource;
  if (c->rate_on) return kInvalidResource;  // a decode launch between two encode launches has no feed to observe
  CK(hipSetDevice(c->device));
  if (out.tensor && !device_span(c, out.base, span, "decode_frame_tensor")) return kInvalidArg;
  int r = flush(c);  // encode frames still pending go first, in their own launch
  if (r) return r;
  const int t = c->next_ticket, slot = t % c->stages;
  Stage& s = c->st[slot];
  if (s.busy) {
    fprintf(stderr, "[cairo_amd] staging slot of ticket %d not released\n", s.ticket);
    return kInvalidResource;
  }
  Pending& p = c->pend[0];
  memset(&p, 0, sizeof(p));  // the whole record: a decode frame has no pixel source (kind kStaged, nothing to upload)
  FrameDesc& f = p.f;
  f.index = (int)index;
  f.inter = 1;
  f.quality = 1;
  f.epoch = ++c->epoch;
  f.slot = slot;
  f.decode = 1;
  frame_links(c, f, t);
  f.host_table = reinterpret_cast<const BlockDesc*>(table);
  f.host_coef = coef;
  c->npend = 1;
  take_stage(s, t, index, 1, 0, 0);
  c->next_ticket++;
  const long long b = c->batches;  // the launch flush() is about to make
  r = flush(c);
  if (r == kSuccess) {
    hipStream_t st = (b & 1) ? c->ks2 : c->ks;
    r = stage_planes(c, slot_planes(c->ring_buf, c, (int)(index % c->ring)), slot, out.fmt, st);
    if (r == kSuccess)
      r = fail(hipMemcpyAsync(s.err, c->sticky, TimeoutInfo::kWords * sizeof(int32_t), hipMemcpyDeviceToHost, st),
               "hipMemcpyAsync");
    if (r == kSuccess) r = write_staged(c, slot, out, st);
    if (r == kSuccess) r = fail(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (r == kSuccess && s.err[TimeoutInfo::kKind]) {
      report_timeout_host(c, s.err, index, st);  // (mu held: the launch stream, idle now)
      r = kHardwareFail;
    }
  }
  s.busy = false;
  return r;
}

int ctx_wait_launched(cairo_ctx* c, int ticket, const std::atomic<bool>* stop,
                      cairo_frame_result* out) {
  if (!c || !out || ticket < 0) return kInvalidArg;
  Stage& s = c->st[ticket % c->stages];
  {
    std::unique_lock<std::mutex> lk(c->mu);
    if (!s.busy || s.ticket != ticket) return kInvalidResource;
    c->launched_cv.wait(lk, [&] { return s.launched || (stop && stop->load()); });
    if (!s.launched) return kInvalidResource;
  }
  return frame_result(c, s, out, true);
}

int ctx_flush(cairo_ctx* c, int ticket) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  if (ticket >= 0) {  // only if that frame is still in the pending batch
    const Stage& s = c->st[ticket % c->stages];
    if (!s.busy || s.ticket != ticket || s.launched) return kSuccess;
  }
  CK(hipSetDevice(c->device));
  return flush(c);
}

void ctx_wake(cairo_ctx* c) {
  std::lock_guard<std::mutex> lk(c->mu);
  c->launched_cv.notify_all();
}

int ctx_geometry(cairo_ctx* c, uint32_t* wmb, uint32_t* hmb, uint32_t* ring, int* next_ticket) {
  if (!c) return kInvalidArg;
  std::lock_guard<std::mutex> lk(c->mu);
  *next_ticket = c->next_ticket;
  *wmb = c->wmb;
  *hmb = c->hmb;
  *ring = c->ring;
  return kSuccess;
}

}  // namespace cairo

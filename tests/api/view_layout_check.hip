// A host-built frame view, read back field by field at the offsets the
// kernels' block reads use (tests/test_view_layout.py).
// Compiled for the host and for gfx950, so kernels.h's static_asserts on the
// layout are evaluated in both passes; runs without a GPU (make_frame_view is
// host code of libcairo_amd.so).
#include <cstdio>
#include <cstring>

#include "kernels.h"

using namespace cairo;

static int failures = 0, fields = 0;

template <class T>
static void expect_at(const FrameArgs& a, size_t off, T want, const char* name) {
  T got;
  std::memcpy(&got, reinterpret_cast<const char*>(&a) + off, sizeof(T));
  fields++;
  if (std::memcmp(&got, &want, sizeof(T)) != 0) {
    std::printf("MISMATCH %s at offset %zu\n", name, off);
    failures++;
  }
}
static void expect_planes(const FrameArgs& a, size_t off, const PlaneSet& p, const char* name) {
  expect_at(a, off, p.y, name);
  expect_at(a, off + 8, p.u, name);
  expect_at(a, off + 16, p.v, name);
}
template <class T>
static T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }
static PlaneSet fake_planes(uintptr_t v) { return PlaneSet{fake<int16_t>(v), fake<int16_t>(v + 0x100), fake<int16_t>(v + 0x200)}; }

int main() {
  // 200 x 120, R = 4: wmb = 13, hmb = 8, a distinct value in every field
  EngineArgs e{};
  e.wa = 208, e.ha = 128, e.w = 200, e.h = 120, e.wmb = 13, e.hmb = 8, e.ring = 4, e.nframes = 6;
  e.src_base = fake<int16_t>(0x10000000);
  e.plane_elems = 0x12340;
  e.table_base = fake<BlockDesc>(0x20000000);
  e.idesc_base = fake<BlockDesc>(0x30000000);
  e.gran_base = fake<uint64_t>(0x40000000);
  e.sync = fake<int32_t>(0x50000000);
  e.sticky = fake<int32_t>(0x60000000);
  e.inject = 1;
  e.stamps = fake<uint64_t>(0x70000000);
  e.acct = fake<uint64_t>(0x78000000);
  FrameDesc f{};
  f.rgb = fake<const uint8_t>(0x80000000);
  f.index = 41, f.inter = 1, f.quality = 23, f.epoch = 0xABCD1234u, f.slot = 3, f.decode = 0;
  for (int k = 0; k < kMaxRing; k++) f.recon[k] = fake_planes(0x90000000 + 0x1000 * k);
  f.stale = fake_planes(0xA0000000);
  f.coef = fake_planes(0xB0000000);
  f.coef_prev = fake_planes(0xB8000000);
  for (int k = 0; k < kMaxPush; k++) f.push[k] = fake_planes(0xC0000000 + 0x1000 * k);
  f.npush = 2;
  f.progress = fake<uint64_t>(0xD0000000);
  f.prev_progress = fake<const uint64_t>(0xD1000000);
  f.prev2_progress = fake<const uint64_t>(0xD2000000);
  f.sys = 1, f.member = 5;
  const int j = 2;
  const FrameArgs a = make_frame_view(e, f, j);

  const size_t mbs = 13 * 8;
  const int ng = 4;
  // block 0: the row coder's macroblock start
  expect_at(a, 0, 208, "wa");
  expect_at(a, 4, 128, "ha");
  expect_at(a, 8, 13, "wmb");
  expect_at(a, 12, 8, "hmb");
  expect_at(a, 16, 0xABCD1234u, "epoch");
  expect_at(a, 20, 3, "nrec");
  expect_at(a, 24, e.idesc_base + 3 * 3 * mbs, "inter_desc");
  expect_planes(a, 32, ring_slot(e.src_base, e.plane_elems, 208, 128, 3), "in");
  expect_at(a, 56, e.gran_base + 3 * mbs * kGranuleStride, "granules");
  // block 1: window prefetch; group start
  expect_planes(a, 64, f.stale, "stale");
  expect_at(a, 88, 4, "ring");
  expect_at(a, 96, e.sync + SyncLayout::inter_done(8, ng, j), "inter_done");
  expect_at(a, 104, ng, "ng");
  expect_at(a, 108, 1, "sys");
  expect_at(a, 112, 3, "nref");
  expect_at(a, 116, 1, "inter");
  expect_at(a, 120, e.acct, "acct");
  // block 2: classification and prediction
  for (int k = 0; k < kMaxRing; k++) expect_planes(a, 128 + 24 * k, f.recon[k], "recon");
  expect_at(a, 224, e.table_base + 3 * mbs, "table");
  expect_at(a, 232, 23, "quality");
  expect_at(a, 236, 0, "decode");
  expect_at(a, 240, 41, "index");
  expect_at(a, 244, 5, "member");
  expect_at(a, 248, e.sync + SyncLayout::kErr, "err");
  // block 3: stores and publish, deblock chunk
  expect_planes(a, 256, f.coef, "coef");
  expect_planes(a, 280, f.coef_prev, "coef_prev");
  expect_at(a, 304, f.progress, "progress");
  expect_at(a, 312, 4, "db_shift");  // wmb < 100: chunks of one macroblock
  expect_at(a, 316, 2, "npush");
  // block 4: helper group start and carry
  expect_at(a, 320, f.prev_progress, "prev_progress");
  expect_at(a, 328, f.prev2_progress, "prev2_progress");
  expect_at(a, 336, e.sticky, "sticky");
  expect_at(a, 344, e.stamps + kMaxBatch * stamp_frame_words(13, 8) + 2 + (size_t)j * 8 * ng * kIStamps, "istamps");
  expect_at(a, 352, f.rgb, "rgb");
  expect_at(a, 360, 1, "inject");
  expect_at(a, 364, 200, "w");
  expect_at(a, 368, 120, "h");
  expect_at(a, 376, e.stamps + (size_t)j * stamp_frame_words(13, 8), "stamps");
  // block 5: the deblock's mirrors
  for (int k = 0; k < kMaxPush; k++) expect_planes(a, 384 + 24 * k, f.push[k], "push");

  // an intra frame and a decoded one: the derived counts
  FrameDesc fi = f;
  fi.inter = 0;
  const FrameArgs ai = make_frame_view(e, fi, 0);
  expect_at(ai, 20, 0, "nrec (intra)");
  expect_at(ai, 112, 1, "nref (intra)");
  expect_at(ai, 116, 0, "inter (intra)");
  FrameDesc fd = f;
  fd.decode = 1;
  const FrameArgs ad = make_frame_view(e, fd, 0);
  expect_at(ad, 20, 0, "nrec (decode)");
  expect_at(ad, 116, 0, "inter (decode)");
  expect_at(ad, 236, 1, "decode (decode)");

  std::printf("%s: %d fields of %zu bytes checked, %d mismatches\n", failures ? "FAILED" : "ok", fields,
              sizeof(FrameArgs), failures);
  return failures ? 1 : 0;
}

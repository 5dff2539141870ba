// Host check of cairo_amd/csrc/search_geometry.h (tests/test_search_geometry.py).
//
// 1. Geometry: for every stage 0..4, both halves, every group 0..15 and every
//    replay lane 0..31, over states (bx0, by0) around and inside a 160x64
//    frame and every macroblock of it, the header's candidate, its validity and
//    what the replay reads back equal the closed form of the search restated
//    here (k9 = stage == 0 || c < 4 ? c : c + 1, % 3, / 3, jlo, step, step/2).
// 2. Source sum: for every int16 value v, the distance of the biased
//    b = v + 0x8000 from the bias, as an unsigned 16-bit absolute difference
//    (what v_sad_u16 adds up), equals |v|.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "search_geometry.h"

namespace {

constexpr int kRadius = 16, kMB = 16, kW = 160, kH = 64;

bool ref_valid(int cx, int cy, int px, int py, int wa, int ha) {
  if (cy > py - kMB && cx > px - kMB) return false;
  return cx >= 0 && cx <= wa - kMB && cy >= 0 && cy <= ha - kMB;
}

struct Cand {
  bool active;
  int cx, cy;
};

// The evaluation's closed form: group grp in the pass of `stage`.
Cand ref_group(int grp, int stage, int bx0, int by0) {
  const int step = stage == 0 ? kRadius : (kRadius >> stage);
  const int jlo = stage == 0 ? -2 * kRadius : -step;
  const int n0 = stage == 0 ? 9 : 8;
  const bool spec = stage >= 1 && stage < 4;
  const bool second = stage >= 1 && grp >= 8;
  const int c = second ? grp - 8 : grp;
  const int k9 = stage == 0 || c < 4 ? c : c + 1;
  const int st = second ? step >> 1 : step;
  Cand r;
  r.active = second ? spec : grp < n0;
  r.cx = bx0 - st + (k9 % 3) * st;
  r.cy = by0 + (second ? -st : jlo) + (k9 / 3) * st;
  return r;
}

// The replay's closed form: lane 0..31 in the pass of `stage`.
Cand ref_lane(int lane, int stage, int bx0, int by0, int& entry) {
  const int step = stage == 0 ? kRadius : (kRadius >> stage);
  const int jlo = stage == 0 ? -2 * kRadius : -step;
  const int n0 = stage == 0 ? 9 : 8;
  const int c = lane & 15;
  const bool row1 = (lane & 16) != 0;
  entry = row1 ? 8 + (c & 7) : c;
  const int k9 = stage == 0 || c < 4 ? c : c + 1;
  const int st = row1 ? step >> 1 : step;
  Cand r;
  r.active = c < (row1 ? 8 : n0);
  r.cx = bx0 - st + (k9 % 3) * st;
  r.cy = by0 + (row1 ? -st : jlo) + (k9 / 3) * st;
  return r;
}

long checked = 0, bad = 0;
// which sides of the frame, and the not-yet-coded region, the sweep reached
long left = 0, above = 0, right = 0, below = 0, uncoded = 0, valid = 0;

void fail(const char* what, int stage, int who, int bx0, int by0, int px, int py) {
  if (bad++ < 10)
    std::printf("mismatch: %s stage %d group/lane %d state (%d, %d) macroblock (%d, %d)\n", what, stage, who, bx0,
                by0, px, py);
}

void check_state(int stage, int bx0, int by0, int px, int py) {
  for (int grp = 0; grp < 16; grp++) {
    const Cand r = ref_group(grp, stage, bx0, by0);
    checked++;
    if (sg::group_active(grp, stage) != r.active) fail("group_active", stage, grp, bx0, by0, px, py);
    if (!r.active) continue;
    int cx, cy;
    sg::candidate(sg::group_units(grp), stage, sg::group_shift(grp, stage), bx0, by0, cx, cy);
    if (cx != r.cx || cy != r.cy) fail("candidate", stage, grp, bx0, by0, px, py);
    const bool ok = ref_valid(r.cx, r.cy, px, py, kW, kH);
    if (sg::intra_valid(cx, cy, px, py, kW, kH) != ok) fail("intra_valid", stage, grp, bx0, by0, px, py);
    left += r.cx < 0, above += r.cy < 0, right += r.cx > kW - kMB, below += r.cy > kH - kMB;
    uncoded += r.cy > py - kMB && r.cx > px - kMB && r.cx >= 0 && r.cx <= kW - kMB && r.cy >= 0 && r.cy <= kH - kMB;
    valid += ok;
  }
  const bool spec = stage >= 1 && stage < 4;
  for (int lane = 0; lane < 32; lane++) {
    int e;
    const Cand r = ref_lane(lane, stage, bx0, by0, e);
    checked++;
    if (sg::replay_entry(lane) != e) fail("replay_entry", stage, lane, bx0, by0, px, py);
    if (sg::replay_slot(lane, stage) != r.active) fail("replay_slot", stage, lane, bx0, by0, px, py);
    if (!r.active || (lane >= 16 && !spec)) continue;  // row 1 counts only with a speculated stage
    // the lane reads what the evaluating group of its entry stored
    if (!sg::group_active(e, stage)) fail("replay reads an idle group", stage, lane, bx0, by0, px, py);
    int cx, cy;
    sg::candidate(sg::group_units(e), stage, sg::group_shift(e, stage), bx0, by0, cx, cy);
    const uint32_t xy = sg::pack_xy(cx, cy);
    if (sg::unpack_x(xy) != r.cx || sg::unpack_y(xy) != r.cy) fail("replay coordinates", stage, lane, bx0, by0, px, py);
  }
}

void check_subpel() {
  bool seen[16] = {};
  for (int grp = 0; grp < 16; grp++) {
    const int q = (grp >> 2) & 1, nn = (grp & 3) | ((grp >> 3) << 2), c = 2 * nn + q;
    const int k9 = nn < 4 ? nn : nn + 1;
    checked++;
    if (sg::subpel_q(grp) != q || sg::subpel_neighbour(grp) != nn) fail("subpel slot", -1, grp, 0, 0, 0, 0);
    if (sg::unit_x(sg::skip_centre(nn)) != k9 % 3 - 1 || sg::unit_y(sg::skip_centre(nn)) != k9 / 3 - 1)
      fail("subpel neighbour", -1, grp, 0, 0, 0, 0);
    seen[c] = true;
  }
  for (int c = 0; c < 16; c++)
    if (!seen[c]) fail("subpel candidate not covered", -1, c, 0, 0, 0, 0);
}

long check_source_sum() {
  long wrong = 0;
  for (int v = -32768; v <= 32767; v++) {
    const uint16_t b = (uint16_t)(v + 0x8000), bias = 0x8000;
    const uint32_t d = b > bias ? (uint32_t)(b - bias) : (uint32_t)(bias - b);  // one half of v_sad_u16
    if (d != (uint32_t)std::abs(v)) wrong++;
  }
  return wrong;
}

}  // namespace

int main() {
  // states: every position the search can reach from a macroblock of the
  // frame (the state starts at the macroblock and moves at most 2 * radius - 1
  // left, right and down, 3 * radius up), on a grid fine enough for the
  // smallest steps near the edges
  for (int py = 0; py < kH; py += kMB)
    for (int px = 0; px < kW; px += kMB)
      for (int stage = 0; stage < 5; stage++)
        for (int dy = -3 * kRadius; dy <= 2 * kRadius; dy += (dy > -4 && dy < 4) ? 1 : 5)
          for (int dx = -2 * kRadius; dx <= 2 * kRadius; dx += (dx > -4 && dx < 4) ? 1 : 5)
            check_state(stage, px + dx, py + dy, px, py);
  check_subpel();
  const long wrong = check_source_sum();
  std::printf("geometry: %ld checks, %ld mismatches; candidates left %ld above %ld right %ld below %ld of the frame, "
              "%ld not yet coded, %ld valid\n", checked, bad, left, above, right, below, uncoded, valid);
  std::printf("source sum: 65536 values, %ld mismatches\n", wrong);
  const bool covered = left && above && right && below && uncoded && valid;
  if (!covered) std::printf("the sweep missed a region\n");
  if (bad || wrong || !covered) return 1;
  std::printf("ok\n");
  return 0;
}

// Candidate geometry of the row coder's intra search.
//
// A pass of the search evaluates one candidate per 16-lane group.  Which slot
// of the 3x3 pattern a group holds never changes during a row, only the step
// and the state (bx0, by0) do, so a lane keeps its slot's unit offsets
// (ux, uy) as signed bytes of one register and a pass derives its candidate
// with two bit-field extracts, two shifts and two adds.  The replay's lanes read
// the coordinates the evaluating group stored beside (sad, mad), packed into
// one word.
//
// Host and device: tests/api/search_geometry_check.hip checks every function
// here against the closed form of the search (motion.cpp:354-419).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SG_HD inline
#endif

namespace sg {

constexpr int kMB = 16;      // macroblock edge
constexpr int kGroups = 16;  // 16-lane groups of the coder's workgroup

// Unit offsets of slot k9 (0..8, row-major) of a 3x3 pattern: k9 % 3 - 1 and
// k9 / 3 - 1 as 2-bit fields of a constant (k9 up to 15 gives -1, unused).
SG_HD int unit_x(int k9) { return (int)((0x24924u >> (2 * k9)) & 3u) - 1; }
SG_HD int unit_y(int k9) { return (int)((0x2A540u >> (2 * k9)) & 3u) - 1; }
// Slot of candidate c (0..7) of a pattern without its centre.
SG_HD int skip_centre(int c) { return c < 4 ? c : c + 1; }

// A group's unit offsets for the whole row.  Bytes 0, 1: (ux, uy) at stage 0,
// where groups 0..8 hold the 9 slots and the pattern's rows are -2, -1, 0
// steps from the state.  Bytes 2, 3: (ux, uy) at stages >= 1, where groups
// 0..7 hold the stage's 8 slots and groups 8..15 the next stage's.
SG_HD uint32_t group_units(int grp) {
  const int k1 = skip_centre(grp & 7);
  const uint32_t x0 = (uint32_t)unit_x(grp) & 0xFFu, y0 = (uint32_t)(unit_y(grp) - 1) & 0xFFu;
  const uint32_t x1 = (uint32_t)unit_x(k1) & 0xFFu, y1 = (uint32_t)unit_y(k1) & 0xFFu;
  return x0 | (y0 << 8) | (x1 << 16) | (y1 << 24);
}

SG_HD int sext8(uint32_t v, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sbfe((int)v, off, 8);
#else
  return (int)(int8_t)(v >> off);
#endif
}

// Step of stage 0..4: 16, 8, 4, 2, 1 (EVX_MOTION_SEARCH_RADIUS = 16), as a shift.
constexpr int kRadiusLog2 = 4;
SG_HD int stage_shift(int stage) { return kRadiusLog2 - stage; }
// Does group grp evaluate a candidate in the pass of `stage`?  The second
// half speculates stage + 1, which exists for stages 1..3.
SG_HD bool group_active(int grp, int stage) {
  return stage == 0 ? grp < 9 : (grp < 8 || stage < 4);
}
// The step a group's candidate is scaled by, as a shift: the speculated half
// uses step / 2 (at stage 4 it has none and is not active).
SG_HD int group_shift(int grp, int stage) {
  const int sh = stage_shift(stage) - (stage >= 1 && grp >= 8 ? 1 : 0);
  return sh < 0 ? 0 : sh;
}
// Candidate of a group: `units` from group_units, `sh` from group_shift
// (wave-uniform), (bx0, by0) the state.
SG_HD void candidate(uint32_t units, int stage, int sh, int bx0, int by0, int& cx, int& cy) {
  const int off = stage == 0 ? 0 : 16;
  cx = (int)(((uint32_t)sext8(units, off) << sh) + (uint32_t)bx0);  // one shift-and-add each
  cy = (int)(((uint32_t)sext8(units, off + 8) << sh) + (uint32_t)by0);
}

// May (cx, cy) predict the macroblock at (px, py)?  Inside the frame and not
// in the region that is not yet coded (motion.cpp:239-243).
SG_HD bool intra_valid(int cx, int cy, int px, int py, int wa, int ha) {
  if (cy > py - kMB && cx > px - kMB) return false;
  return cx >= 0 && cx <= wa - kMB && cy >= 0 && cy <= ha - kMB;
}

// The coordinates as one word beside a candidate's (sad, mad): int16 halves
// (frames are at most 32767 wide and high, candidates at least -3 * radius).
SG_HD uint32_t pack_xy(int cx, int cy) { return ((uint32_t)cx & 0xFFFFu) | ((uint32_t)cy << 16); }
SG_HD int unpack_x(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
SG_HD int unpack_y(uint32_t w) { return (int)w >> 16; }

// The replay: lanes 0..15 (row 0) fold the stage's entries, lanes 16..31
// (row 1) entries 8..15, the speculated stage.  The entry a lane reads, and
// whether it holds a candidate of this pass at all.
SG_HD int replay_entry(int lane) { return (lane & 16) ? 8 + (lane & 7) : lane & 15; }
SG_HD bool replay_slot(int lane, int stage) {
  const int c = lane & 15;
  return (lane & 16) ? c < 8 : c < (stage == 0 ? 9 : 8);
}

// Sub-pel step: group grp evaluates candidate 2 nn + q toward neighbour slot
// skip_centre(nn); q (0 half, 1 quarter) is wave-uniform.
SG_HD int subpel_q(int grp) { return (grp >> 2) & 1; }
SG_HD int subpel_neighbour(int grp) { return (grp & 3) | ((grp >> 3) << 2); }

}  // namespace sg

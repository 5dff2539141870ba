// cairo_amd/csrc/table_check.cpp -- the legality predicate of a decoded block
// table (cairo_table_check): what the decode-mode engine can reconstruct as
// the reference decoder would.  Host only, no device.
//
// The engine trusts the table; a stream may carry anything.  Every table the
// reference encoder writes passes:
//   * types: decode_block's switch (decode.cpp:14-142) knows 0-4, 6 and 7.
//   * q_index of a block with coefficients: 1..31, the quantizer's range
//     (quantize.cpp:65-68 clips to it; with qp 0 the forward quantizer would
//     divide by zero, quantize.cpp:89-91, so no encoder can have produced it).
//     A copy block's q_index is not in the stream and never read
//     (deblock.cpp:49-79 skips it).
//   * motion: the block at the vector, and at the sub-pel neighbour when
//     sp_pred, lies inside the frame (motion.cpp:225-275, 277-352).
//   * intra motion: both also lie inside the row coder's window (at most 32 px
//     sideways, 48 px up, 16 px down) and outside the region the raster order
//     has not coded yet, y > py-16 && x > px-16 (motion.cpp:238-241, 303-306).
//     A block there would overlap its own destination in the reference and is
//     overwritten by the window prefetch in the engine.
//   * inter types: 1 <= prediction_target <= ring-1 (encode.cpp:17-67 searches
//     offsets 1..R-1).  Target 0 is the slot being written; targets of R and
//     more do not exist.
#include <cstddef>
#include <cstdint>

#include "../../include/cairo_amd.h"
#include "evx_defs.h"

namespace cairo {

// One desc at macroblock (bx, by).
static bool desc_ok(const BlockDesc& d, uint32_t bx, uint32_t by, uint32_t wmb, uint32_t hmb, uint32_t ring) {
  // frac_index -> direction (motion.cpp:61-109); sp_index 0..7.
  static const int8_t kDx[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
  static const int8_t kDy[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
  const int32_t xmax = (int32_t)wmb * 16 - 16, ymax = (int32_t)hmb * 16 - 16;
  const uint32_t t = d.block_type;
  if (t > 7 || t == 5) return false;
  if (!(t & kCopy) && (d.q_index < 1 || d.q_index > 31)) return false;
  if (!(t & kIntra) && (d.prediction_target < 1 || d.prediction_target + 1u > ring)) return false;
  if (!(t & kMotion)) return true;
  if (d.sp_pred > 1 || (d.sp_pred && (d.sp_index > 7 || d.sp_amount > 1))) return false;
  const int32_t px = (int32_t)bx * 16, py = (int32_t)by * 16;
  for (int k = 0; k <= (int)d.sp_pred; k++) {
    const int32_t x = px + d.motion_x + (k ? kDx[d.sp_index] : 0);
    const int32_t y = py + d.motion_y + (k ? kDy[d.sp_index] : 0);
    if (x < 0 || x > xmax || y < 0 || y > ymax) return false;
    if (!(t & kIntra)) continue;
    if (x < px - 32 || x > px + 32 || y < py - 48 || y > py + 16) return false;
    if (y > py - 16 && x > px - 16) return false;
  }
  return true;
}

int table_check(const BlockDesc* table, uint32_t wmb, uint32_t hmb, uint32_t ring) {
  for (uint32_t by = 0; by < hmb; by++)
    for (uint32_t bx = 0; bx < wmb; bx++)
      if (!desc_ok(table[(size_t)by * wmb + bx], bx, by, wmb, hmb, ring)) return 0;
  return 1;
}

}  // namespace cairo

extern "C" int cairo_table_check(const uint8_t* block_table, uint32_t wmb, uint32_t hmb, uint32_t ring) {
  if (!block_table || !wmb || !hmb || ring < 1 || ring > (uint32_t)cairo::kMaxRing) return 0;
  return cairo::table_check(reinterpret_cast<const cairo::BlockDesc*>(block_table), wmb, hmb, ring);
}

extern "C" int cairo_desc_check(const uint8_t* descs, const uint32_t* mb_index, uint32_t n, uint32_t wmb,
                                uint32_t hmb, uint32_t ring, uint8_t* ok) {
  if (!descs || !mb_index || !ok || !wmb || !hmb || ring < 1 || ring > (uint32_t)cairo::kMaxRing) return 1;
  const cairo::BlockDesc* d = reinterpret_cast<const cairo::BlockDesc*>(descs);
  for (uint32_t k = 0; k < n; k++)
    ok[k] = mb_index[k] < wmb * hmb && cairo::desc_ok(d[k], mb_index[k] % wmb, mb_index[k] / wmb, wmb, hmb, ring);
  return 0;
}

// cairo_amd/csrc/rate.h -- the rules of the target-bitrate controller (DESIGN
// §4.20), stated once: the host entry points (cairo_rate_estimate, _init,
// _step) and the kernels of rate.hip run this code.  Integers only, so the
// device chooses what the host model chooses.  Needs <stdint.h> and the
// public header only.
#pragma once

#include <stdint.h>

#include "../../include/cairo_amd.h"
#include "pixel_common.h"

namespace cairo {

// Bits a frame's record adds to its payload (stream_format.h: 10 bytes).
constexpr int64_t kRateFrameRecordBits = 80;
// |debt| is kept below this, so that every sum of the law fits int64 for any
// sequence of observations the entry points accept (obs_sum <= kRateMaxObs).
constexpr int64_t kRateDebtLimit = (int64_t)1 << 60;
constexpr int64_t kRateMaxObs = (int64_t)1 << 48;

// Number of significant bits of x (0 for 0).
CAIRO_HD int rate_bitlen(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 64 - __clzll((long long)x);
#else
  return x ? 64 - __builtin_clzll(x) : 0;
#endif
}

// log2(x) in Q16 for 1 <= x < 2^32, by sixteen squarings of the normalised
// mantissa: the algorithm is the definition (cairo_amd.h, cairo_rate_estimate).
CAIRO_HD uint32_t rate_log2_q16(uint32_t x) {
  const int e = rate_bitlen(x) - 1;
  uint64_t y = (uint64_t)x << (31 - e);  // in [2^31, 2^32)
  uint32_t frac = 0;
  for (int i = 0; i < 16; i++) {
    y = (y * y) >> 31;
    const uint32_t bit = y >= ((uint64_t)1 << 32);
    frac = (frac << 1) | bit;
    if (bit) y >>= 1;
  }
  return ((uint32_t)e << 16) | frac;
}

CAIRO_HD int64_t rate_xlog(uint64_t x) { return x ? (int64_t)(x * rate_log2_q16((uint32_t)x)) : 0; }

// E(N, z): the arithmetic coder's output for a feed of N bits of which z are
// zero, N < 2^32, z <= N.
CAIRO_HD int64_t rate_estimate(uint64_t n, uint64_t z) {
  return (rate_xlog(n) - rate_xlog(z) - rate_xlog(n - z)) >> 16;
}

// A frame as the controller observes it: its estimate plus the frame record;
// 4 T for a frame whose feed overflowed (its feed is not valid).
CAIRO_HD int64_t rate_frame_bits(uint64_t nbits, uint64_t ones, uint32_t overflow, uint32_t target) {
  return overflow ? 4 * (int64_t)target : rate_estimate(nbits, nbits - ones) + kRateFrameRecordBits;
}

CAIRO_HD bool rate_cfg_ok(const cairo_rate* c) {
  return c->target_bits >= 1 && c->target_bits <= (1u << 28) && c->qmin >= 1 && c->qmax <= 31 && c->qmin <= c->qmax &&
         c->q0 >= 1 && c->q0 <= 31 && c->window >= 1 && !c->reserved[0] && !c->reserved[1] && !c->reserved[2];
}

CAIRO_HD int64_t rate_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

CAIRO_HD void rate_init(cairo_rate_state* s) {
  s->debt = 0;
  s->p_aim = s->o_aim = 0;
  s->p_n = s->p_q = s->o_n = s->o_q = 0;
  s->launches = 0;
  s->reserved = 0;
}

// The quality of all n_new frames of the next launch.  obs_sum: the summed
// bits (rate_frame_bits) of the frames of the launch before the last, read
// only once two launches exist.  P is the last launch, O the one before.
CAIRO_HD uint32_t rate_step(cairo_rate_state* s, const cairo_rate* c, int n_new, int64_t obs_sum) {
  const int64_t T = c->target_bits;
  int64_t q = c->q0, aim = T;
  if (s->launches >= 2) {
    s->debt = rate_clamp(s->debt + obs_sum - s->o_n * T, -kRateDebtLimit, kRateDebtLimit);
    // the last launch is taken to hit what it aimed at: without this term the
    // two-launch lag corrects the same debt twice
    const int64_t dp = s->debt + s->p_n * (s->p_aim - T);
    aim = rate_clamp(T - dp / (int64_t)c->window, T / 4 > 1 ? T / 4 : 1, 4 * T);
    const uint64_t M = obs_sum > 0 ? (uint64_t)obs_sum / (uint64_t)s->o_n : 0;
    const int len = rate_bitlen(M > (uint64_t)aim ? M : (uint64_t)aim);
    const int sh = len > 24 ? len - 24 : 0;
    const uint64_t m = M >> sh;
    uint64_t t = (uint64_t)aim >> sh;
    if (t < 1) t = 1;
    // bits fall more slowly than 1 / q^(1/2), so squaring the
    // ratio moves q by less than the whole miss
    const uint64_t qm = ((uint64_t)s->o_q * m * m + t * t / 2) / (t * t);
    const int64_t st = 1 + s->p_q / 4;
    q = rate_clamp((int64_t)(qm < 64 ? qm : 64), s->p_q - st, s->p_q + st);
  }
  q = rate_clamp(q, c->qmin, c->qmax);
  s->o_n = s->p_n, s->o_q = s->p_q, s->o_aim = s->p_aim;
  s->p_n = n_new, s->p_q = (int32_t)q, s->p_aim = aim;
  if (s->launches < 0xFFFFFFFFu) s->launches++;
  return (uint32_t)q;
}

}  // namespace cairo

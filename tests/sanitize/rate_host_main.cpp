// tests/sanitize/rate_host_main.cpp -- rate.h (the target-bitrate rules) in a
// stand-alone host program, built by tests/test_rate.py with the address and
// undefined-behaviour sanitizers: the law at the ends of every range the entry
// points accept (T = 1 and 2^28, launches of 65535 frames, observations of 0 and
// 2^48 for thousands of steps, windows of 1 and 2^32 - 1) and the estimate up to
// N = 2^32 - 1 must stay inside int64 and inside [qmin, qmax].
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../cairo_amd/csrc/rate.h"

using namespace cairo;

int main() {
  std::mt19937_64 g(1);
  long steps = 0;
  for (int trial = 0; trial < 4000; trial++) {
    cairo_rate c{};
    const uint32_t targets[] = {1, 2, 1000, 55000, 1u << 28};
    const uint32_t windows[] = {1, 2, 32, 0xFFFFFFFFu};
    c.target_bits = targets[g() % 5];
    c.qmin = 1 + g() % 31;
    c.qmax = c.qmin + g() % (32 - c.qmin);
    c.q0 = 1 + g() % 31;
    c.window = windows[g() % 4];
    if (!rate_cfg_ok(&c)) return 2;
    cairo_rate_state s;
    rate_init(&s);
    const int mode = g() % 3;  // every observation the largest, the smallest, or random
    const int len = trial < 30 ? 3000 : 40;
    for (int k = 0; k < len; k++, steps++) {
      const int n = (g() % 2) ? 65535 : 1 + (int)(g() % 48);
      const int64_t obs = mode == 0 ? kRateMaxObs : mode == 1 ? 0 : (int64_t)(g() % ((uint64_t)kRateMaxObs + 1));
      const uint32_t q = rate_step(&s, &c, n, obs);
      if (q < c.qmin || q > c.qmax || s.debt > kRateDebtLimit || s.debt < -kRateDebtLimit) return 3;
    }
  }
  for (int i = 0; i < 100000; i++) {
    const uint64_t n = g() >> 32, z = n ? g() % (n + 1) : 0;
    // within the truncation of L (2^-16 bit per feed bit and term) of [0, N]
    const int64_t e = rate_estimate(n, z), slack = (int64_t)(n >> 14) + 1;
    if (e < -slack || e > (int64_t)n + slack) return 4;
  }
  if (rate_estimate(0, 0) != 0 || rate_estimate(0xFFFFFFFFull, 0) != 0 || rate_estimate(2, 1) != 2) return 5;
  printf("steps %ld\n", steps);
  return 0;
}

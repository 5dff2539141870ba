// tests/sanitize/unserialize_driver.cpp -- arbitrary byte streams through the
// host entropy decode (cairo_unserialize_slice) and the legality predicate
// (cairo_table_check), built with -fsanitize=address,undefined together with
// unserialize.cpp and table_check.cpp by tests/test_tables.py.
//
// Streams: random, all-zero, all-one and sparse bytes, in heap buffers of
// exactly their size (a read past the end is an error), decoded from random
// read offsets into a block table and coefficient planes that persist across
// three frames.  Whatever the stream holds, the decode must stay inside its
// buffers, leave read_index <= write_index, and the predicate must answer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/cairo_amd.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main(int argc, char** argv) {
  const int iterations = argc > 1 ? atoi(argv[1]) : 3000;
  long decoded = 0, refused = 0, legal = 0;
  for (int it = 0; it < iterations; it++) {
    const uint32_t wmb = 1 + rnd() % 6, hmb = 1 + rnd() % 5, ring = 2 + rnd() % 3;
    const size_t ny = (size_t)wmb * hmb * 256, nc = ny / 4;
    std::vector<uint8_t> table((size_t)wmb * hmb * 16, 0);
    std::vector<int16_t> cy(ny, 0), cu(nc, 0), cv(nc, 0);
    for (int frame = 0; frame < 3; frame++) {
      const uint32_t size = rnd() % 513;
      uint8_t* data = (uint8_t*)malloc(size ? size : 1);
      const int kind = rnd() % 4;
      for (uint32_t k = 0; k < size; k++)
        data[k] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? 0 : kind == 2 ? 0xFF : (rnd() % 16 ? 0 : (uint8_t)rnd());
      const uint32_t wr = size * 8 - (size ? rnd() % 8 : 0);
      uint32_t rd = wr ? rnd() % (wr + 1) : 0;
      const uint32_t rd0 = rd;
      const int r = cairo_unserialize_slice(data, &rd, wr, wmb, hmb, ring, table.data(), cy.data(), cu.data(),
                                            cv.data());
      free(data);
      if (rd > wr || rd < rd0) {
        fprintf(stderr, "iteration %d frame %d: read_index %u outside [%u, %u]\n", it, frame, rd, rd0, wr);
        return 2;
      }
      if (r) {
        refused++;
        continue;
      }
      decoded++;
      legal += cairo_table_check(table.data(), wmb, hmb, ring);
    }
  }
  printf("decoded %ld refused %ld legal %ld\n", decoded, refused, legal);
  return 0;
}

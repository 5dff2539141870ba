// tests/sanitize/tensor_host_main.cpp -- the tensor frame map's per-sample code
// (cairo_amd/csrc/tensor_pixel.h, the text the kernels compile) as a
// stand-alone program, built with -fsanitize=address,undefined by
// tests/test_tensor.py.  It reads a file of cases, runs each on heap buffers
// of exactly the tensor's span and exactly 3 * w * h bytes, and writes both
// buffers of every case to the output file, for the test to compare with the
// exact reference.
//
// Case file, little endian: uint32 count, then per case
//   int32 dir, uint32 dtype, uint32 w, uint32 h, int64 stride[3],
//   float mul[3], float add[3], uint64 tensor_bytes,
//   tensor_bytes bytes (the tensor from element (0, 0, 0)), 3 * w * h bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../cairo_amd/csrc/tensor_pixel.h"

namespace {

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Header {
  int32_t dir;
  uint32_t dtype, w, h;
  int64_t stride[3];
  float mul[3], add[3];
  uint64_t tensor_bytes;
};
static_assert(sizeof(Header) == 72, "packed as the test writes it");

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t count = 0;
  if (!rd(in, &count, 4)) return 2;
  for (uint32_t i = 0; i < count; i++) {
    Header hd;
    if (!rd(in, &hd, sizeof(hd))) return 2;
    const size_t rgb_bytes = (size_t)hd.w * hd.h * 3;
    uint8_t* tensor = (uint8_t*)malloc(hd.tensor_bytes);
    uint8_t* rgb = (uint8_t*)malloc(rgb_bytes);
    if (!tensor || !rgb || !rd(in, tensor, hd.tensor_bytes) || !rd(in, rgb, rgb_bytes)) return 2;
    cairo::tensor_host_loops(hd.dir, hd.dtype, hd.stride, hd.mul, hd.add, hd.w, hd.h, tensor, rgb);
    if (fwrite(tensor, 1, hd.tensor_bytes, out) != hd.tensor_bytes || fwrite(rgb, 1, rgb_bytes, out) != rgb_bytes)
      return 2;
    free(tensor);
    free(rgb);
  }
  fclose(in);
  if (fclose(out)) return 2;
  printf("cases %u\n", count);
  return 0;
}

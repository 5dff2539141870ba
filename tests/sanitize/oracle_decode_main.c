/* tests/sanitize/oracle_decode_main.c -- the oracle decoder (orc_decode_frame)
 * as a stand-alone program, built with -fsanitize=address,undefined together
 * with oracle/evx_oracle.c by tests/test_tables.py.
 *
 * Reads a sequence file: int32 width, height, ring, frames, then per frame the
 * block table (16 B per macroblock) and the y, u, v coefficient planes
 * (int16).  Decodes the frames in order and prints the FNV-1a hash over every
 * frame's planes before the deblock and its ring slot after it, which the test
 * compares with the same hash from the shared library. */
#include <stdio.h>
#include <stdlib.h>

#include "../../oracle/evx_oracle.h"

static int read_all(void *p, size_t n, FILE *f) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[4];
    if (!f || !read_all(hd, sizeof(hd), f)) return 2;
    const int w = hd[0], h = hd[1], ring = hd[2], frames = hd[3];
    const int wa = (w + 15) & ~15, ha = (h + 15) & ~15;
    const size_t nt = (size_t)(wa / 16) * (ha / 16) * 16, ny = (size_t)wa * ha, nc = ny / 4;
    uint8_t *table = (uint8_t *)malloc(nt);
    int16_t *y = (int16_t *)malloc(ny * 2), *u = (int16_t *)malloc(nc * 2), *v = (int16_t *)malloc(nc * 2);
    orc_encoder *e = orc_create(ring);
    if (!table || !y || !u || !v || !e) return 2;
    uint64_t hash = 0xCBF29CE484222325ull;
    for (int t = 0; t < frames; t++) {
        if (!read_all(table, nt, f) || !read_all(y, ny * 2, f) || !read_all(u, nc * 2, f) || !read_all(v, nc * 2, f))
            return 2;
        if (orc_decode_frame(e, w, h, table, y, u, v)) return 3;
        for (int p = 0; p < 3; p++)
            hash = orc_fnv1a64(hash, (const uint8_t *)orc_predeblock_plane(e, p), (p ? nc : ny) * 2);
        for (int p = 0; p < 3; p++)
            hash = orc_fnv1a64(hash, (const uint8_t *)orc_plane(e, 2 + t % ring, p), (p ? nc : ny) * 2);
    }
    printf("%016llx\n", (unsigned long long)hash);
    orc_destroy(e);
    free(table);
    free(y);
    free(u);
    free(v);
    fclose(f);
    return 0;
}

// upsample_wide.cpp -- stand-alone driver for lj_pixels8 and lj_luma8 (mjx_kernels.h, the routines k_upsample_color and
// k_upsample_luma run) with upsampling ratios of 4 (tests/test_wide_sampling.py builds it under -fsanitize=address,undefined and runs
// it on the CPU).  For every ratio pair from {1, 2, 4}^2 with a 4 in it and plane sizes 1, 2, 3, 8, 9 and 17, a component plane lives
// in a heap block of exactly stride x ch bytes -- stride = cw rounded up to 8, what LjPlane promises and no more --, and every strip
// of every row the plane covers goes through both routines: a read outside the block is the sanitizer's to report.  The samples
// are checked against plain replication, s[X / rh] of row Y / rv.  Prints what it did; exits non-zero on a wrong sample.
#include "mjx_kernels.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mjx;

static uint8_t *plane_of(uint32_t cw, uint32_t ch, uint32_t stride, uint32_t seed)
{
    uint8_t *p = static_cast<uint8_t *>(std::malloc(size_t(stride) * ch));      // exactly the plane: no slack behind it
    if (!p) std::exit(2);
    std::memset(p, 0xa5, size_t(stride) * ch);
    uint32_t s = seed * 2654435761u + 12345u;
    for (uint32_t y = 0; y < ch; y++)
        for (uint32_t x = 0; x < cw; x++) { s = s * 1664525u + 1013904223u; p[size_t(y) * stride + x] = uint8_t(s >> 24); }
    return p;
}

int main()
{
    const uint32_t dims[6] = {1, 2, 3, 8, 9, 17}, ratios[3] = {1, 2, 4};
    unsigned long strips = 0;
    for (uint32_t rh : ratios)
        for (uint32_t rv : ratios) {
            if (rh != 4 && rv != 4) continue;
            for (uint32_t cw : dims)
                for (uint32_t ch : dims) {
                    const uint32_t stride = (cw + 7u) & ~7u, W = cw * rh, H = ch * rv;
                    uint8_t *c = plane_of(cw, ch, stride, cw * 31u + ch), *y = plane_of(W, H, (W + 7u) & ~7u, 7u);
                    const LjPlane pc{c, stride, cw, ch, rh, rv}, py{y, (W + 7u) & ~7u, W, H, 1u, 1u};
                    const LjPlane pl[3] = {py, pc, pc};
                    for (uint32_t Y = 0; Y < H; Y++)
                        for (uint32_t X0 = 0; X0 < W; X0 += kLjStrip, strips++) {
                            uint32_t w2[2], w6[6];
                            lj_luma8(pc, X0, Y, w2);
                            lj_pixels8(pl, 3u, X0, Y, w6);
                            for (uint32_t k = 0; k < kLjStrip && X0 + k < W; k++) {
                                const uint32_t want = c[size_t(Y / rv) * stride + (X0 + k) / rh];
                                const uint32_t got = (w2[k >> 2] >> ((k & 3u) * 8u)) & 0xffu;
                                if (got != want) {
                                    std::fprintf(stderr, "ratio %ux%u plane %ux%u pixel (%u, %u): %u, expected %u\n", rh, rv, cw, ch, X0 + k, Y, got, want);
                                    return 1;
                                }
                                // the colour step on (Y, c, c): checked against lj_color itself, so only the upsampling is at stake
                                float r, g, b;
                                lj_color(float(y[size_t(Y) * py.stride + X0 + k]), float(want), float(want), r, g, b);
                                const float ch3[3] = {r, g, b};
                                for (uint32_t q = 0; q < 3; q++) {
                                    const uint32_t at = 3 * k + q, byte = (w6[at >> 2] >> ((at & 3u) * 8u)) & 0xffu;
                                    if (byte != lj_put_u8(ch3[q], 0, 0)) { std::fprintf(stderr, "colour byte %u of pixel (%u, %u)\n", q, X0 + k, Y); return 1; }
                                }
                            }
                        }
                    std::free(c);
                    std::free(y);
                }
        }
    std::printf("strips %lu\n", strips);
    return 0;
}

// islow_host.cpp -- stand-alone driver for idct_islow_inplace (mjx_kernels.h, the lane routine stage B's integer sink runs)
// (tests/test_islow_idct.py builds it under -fsanitize=address,undefined and runs it on the CPU).  Every block lives in a heap block
// of exactly 64 words, what a lane owns and no more: a read or write outside it is the sanitizer's to report, and so is signed
// overflow -- the routine works on uint32_t, the contract's wrap-around is defined behaviour.  The blocks: every single coefficient at
// +-1, +-1023 and +-32767 with table entries of 1, 255 and 65535; dense blocks in range, at the 16-bit limits and of pseudo-random
// 32-bit words (whatever a wrapped product can be); all-zero AC rows and columns.  A flat block is checked against its closed form;
// a checksum of every sample is printed so that a run says what it did.  Exits non-zero on a wrong sample.
#include "mjx_kernels.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mjx;

static unsigned long blocks_run = 0, checksum = 0;

// coef x q in a heap block of exactly 64 words -> the 64 samples
static void run(const int32_t coef[64], const uint32_t q[64], uint8_t out[64])
{
    uint32_t *blk = static_cast<uint32_t *>(std::malloc(64 * sizeof(uint32_t)));
    if (!blk) std::exit(2);
    for (int k = 0; k < 64; k++) blk[k] = uint32_t(coef[k]) * q[k];
    idct_islow_inplace(blk);
    for (int k = 0; k < 64; k++) {
        const uint32_t s = islow_sample(blk[k]);
        if (s > 255u) { std::fprintf(stderr, "sample %u out of range\n", s); std::exit(1); }
        out[k] = uint8_t(s);
        checksum = checksum * 31u + s;
    }
    std::free(blk);
    blocks_run++;
}

int main()
{
    const int32_t values[6] = {1, -1, 1023, -1023, 32767, -32767};
    const uint32_t tables[3] = {1u, 255u, 65535u};
    int32_t coef[64];
    uint32_t q[64];
    uint8_t out[64];
    // every single coefficient
    for (int pos = 0; pos < 64; pos++)
        for (int32_t v : values)
            for (uint32_t t : tables) {
                std::memset(coef, 0, sizeof coef);
                for (int k = 0; k < 64; k++) q[k] = t;
                coef[pos] = v;
                run(coef, q, out);
                if (pos == 0) {                // a flat block: DC d gives clamp(((d + 4) >> 3) + 128) everywhere while d 2^13 does not wrap
                    const int64_t d = int64_t(v) * t;
                    if (d > -(1 << 16) + 4 && d < (1 << 16) - 4) {      // ((d 2^15 + 2^17) stays inside 32 bits)
                        int64_t s = ((d + 4) >> 3) + 128;
                        s = s < 0 ? 0 : s > 255 ? 255 : s;
                        for (int k = 0; k < 64; k++)
                            if (out[k] != s) { std::fprintf(stderr, "flat block dc %ld: sample %d is %u, expected %ld\n", long(d), k, out[k], long(s)); return 1; }
                    }
                }
            }
    // dense blocks: in range, at the limits of 16 bits, and any 32-bit word
    uint32_t s = 12345u;
    auto next = [&s]() { s = s * 1664525u + 1013904223u; return s; };
    for (int round = 0; round < 300; round++) {
        for (int k = 0; k < 64; k++) {
            const uint32_t r = next();
            if (round < 100) { coef[k] = int32_t(r >> 20) % 64 - 32; q[k] = 1u + (next() >> 28); }
            else if (round < 200) { coef[k] = (r & 1u) ? 32767 : -32768; q[k] = (next() & 1u) ? 65535u : 255u; }
            else { coef[k] = int32_t(r); q[k] = next(); }
        }
        run(coef, q, out);
    }
    // all-zero AC rows and columns: only row 0, only column 0, only the DC term and one far corner
    for (int kind = 0; kind < 3; kind++) {
        std::memset(coef, 0, sizeof coef);
        for (int k = 0; k < 64; k++) q[k] = 16u;
        for (int k = 0; k < 8; k++) {
            if (kind == 0) coef[k] = 100 - 30 * k;
            if (kind == 1) coef[8 * k] = 100 - 30 * k;
        }
        if (kind == 2) { coef[0] = 64; coef[63] = -500; }
        run(coef, q, out);
    }
    std::printf("blocks %lu checksum %lu\n", blocks_run, checksum);
    return 0;
}

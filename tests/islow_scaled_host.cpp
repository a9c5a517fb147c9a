// islow_scaled_host.cpp -- stand-alone driver for idct_red4_inplace, idct_red2_inplace and idct_red1 (mjx_kernels.h, the lane routines
// stage B runs for MJX_IDCT_ISLOW at scale 2, 4 and 8)
// (tests/test_islow_scaled.py builds it under -fsanitize=address,undefined and runs it on the CPU).  Every block lives in a heap block
// of exactly 64 words, what a lane owns and no more: a read or write outside it is the sanitizer's to report, and so is signed
// overflow -- the routines work on uint32_t, the contract's wrap-around is defined behaviour.  The blocks are islow_host.cpp's: every
// single coefficient at +-1, +-1023 and +-32767 with table entries of 1, 255 and 65535; dense blocks in range, at the 16-bit limits and
// of pseudo-random 32-bit words.  Checked here: a flat block against its closed form (every size gives clamp(((d + 4) >> 3) + 128)),
// and that the positions the contract says are never read do not matter -- row and column 4 for N = 4, the even rows and columns from
// 2 on for N = 2, everything but the DC term for N = 1.  A checksum of every sample is printed.  Exits non-zero on a wrong sample.
#include "mjx_kernels.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mjx;

static unsigned long blocks_run = 0, checksum = 0;

// coef x q in a heap block of exactly 64 words -> the N x N samples (rows of N)
static void run(const int32_t coef[64], const uint32_t q[64], uint32_t N, uint8_t *out)
{
    uint32_t *blk = static_cast<uint32_t *>(std::aligned_alloc(16, 64 * sizeof(uint32_t)));
    if (!blk) std::exit(2);
    for (int k = 0; k < 64; k++) blk[k] = uint32_t(coef[k]) * q[k];
    if (N == 4u) idct_red4_inplace(blk);
    else if (N == 2u) idct_red2_inplace(blk);
    else idct_red1(blk);
    for (uint32_t y = 0; y < N; y++)
        for (uint32_t x = 0; x < N; x++) {
            const uint32_t s = islow_sample(blk[y * 8u + x]);
            if (s > 255u) { std::fprintf(stderr, "sample %u out of range\n", s); std::exit(1); }
            out[y * N + x] = uint8_t(s);
            checksum = checksum * 31u + s;
        }
    std::free(blk);
    blocks_run++;
}

static bool unread(uint32_t N, int pos)
{
    const int v = pos >> 3, u = pos & 7;
    if (N == 4u) return v == 4 || u == 4;
    if (N == 2u) return (v != 0 && !(v & 1)) || (u != 0 && !(u & 1));
    return pos != 0;
}

// the block with every position the size never reads overwritten must give the same samples
static int check_unread(const int32_t coef[64], const uint32_t q[64], uint32_t N, const uint8_t *want)
{
    int32_t c2[64];
    uint8_t out[64];
    for (int k = 0; k < 64; k++) c2[k] = unread(N, k) ? coef[k] * 7 + 12345 : coef[k];
    run(c2, q, N, out);
    if (std::memcmp(out, want, N * N) != 0) { std::fprintf(stderr, "N = %u: a position outside the contract's reads changed the output\n", N); return 1; }
    return 0;
}

int main()
{
    const int32_t values[6] = {1, -1, 1023, -1023, 32767, -32767};
    const uint32_t tables[3] = {1u, 255u, 65535u};
    const uint32_t sizes[3] = {4u, 2u, 1u};
    int32_t coef[64];
    uint32_t q[64];
    uint8_t out[64];
    for (uint32_t N : sizes) {
        for (int pos = 0; pos < 64; pos++)
            for (int32_t v : values)
                for (uint32_t t : tables) {
                    std::memset(coef, 0, sizeof coef);
                    for (int k = 0; k < 64; k++) q[k] = t;
                    coef[pos] = v;
                    run(coef, q, N, out);
                    const int64_t d = int64_t(v) * t;
                    // (a flat block; |d| < 2^15: the DC term shifted left by at most 15 plus the rounding constant, below 2^30 + 2^19, does not wrap)
                    if (pos == 0 && d > -(1 << 15) + 4 && d < (1 << 15) - 4) {
                        int64_t s = ((d + 4) >> 3) + 128;
                        s = s < 0 ? 0 : s > 255 ? 255 : s;
                        for (uint32_t k = 0; k < N * N; k++)
                            if (out[k] != s) { std::fprintf(stderr, "N = %u flat block dc %ld: sample %u is %u, expected %ld\n", N, long(d), k, out[k], long(s)); return 1; }
                    }
                    if (pos != 0 && unread(N, pos)) {                                // a coefficient the size never reads: the all-zero block's picture
                        for (uint32_t k = 0; k < N * N; k++)
                            if (out[k] != 128) { std::fprintf(stderr, "N = %u: position %d was read\n", N, pos); return 1; }
                    }
                }
        uint32_t s = 12345u;
        auto next = [&s]() { s = s * 1664525u + 1013904223u; return s; };
        for (int round = 0; round < 300; round++) {
            for (int k = 0; k < 64; k++) {
                const uint32_t r = next();
                if (round < 100) { coef[k] = int32_t(r >> 20) % 64 - 32; q[k] = 1u + (next() >> 28); }
                else if (round < 200) { coef[k] = (r & 1u) ? 32767 : -32768; q[k] = (next() & 1u) ? 65535u : 255u; }
                else { coef[k] = int32_t(r >> 1); q[k] = next(); }
            }
            run(coef, q, N, out);
            if (round < 200 && check_unread(coef, q, N, out)) return 1;
        }
    }
    std::printf("blocks %lu checksum %lu\n", blocks_run, checksum);
    return 0;
}

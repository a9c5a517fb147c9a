// exif_fuzz.cpp -- stand-alone driver for mjx_exif_orientation (tests/test_orientation.py builds it with mjx_parse.cpp under
// -fsanitize=address,undefined and runs it on the CPU).  Input: a file of cases, each a little-endian u32 length, one byte with the
// code the reader must find, and the bytes.  Every case, and then seeded mutations of the first one -- byte flips, and truncations
// at every length --, is handed to the reader in a heap block of exactly its size, so a read outside [jpeg, jpeg + len) is
// the sanitizer's to report.  Prints what it did; exits non-zero on a wrong code or status.
#include "mjx.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int run_one(const uint8_t *p, size_t n, int want)
{
    uint8_t *blk = static_cast<uint8_t *>(std::malloc(n ? n : 1));      // exactly n bytes: no slack behind them
    if (!blk) return 2;
    if (n) std::memcpy(blk, p, n);
    uint8_t code = 0xee;
    const int rc = mjx_exif_orientation(blk, n, &code);
    std::free(blk);
    if (rc != MJX_OK || code < 1 || code > 8) { std::fprintf(stderr, "status %d code %u on %zu bytes\n", rc, unsigned(code), n); return 1; }
    if (want && code != want) { std::fprintf(stderr, "code %u, expected %d, on %zu bytes\n", unsigned(code), want, n); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const unsigned long mutations = std::strtoul(argv[2], nullptr, 10);
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<std::vector<uint8_t>> cases;
    std::vector<int> want;
    for (;;) {
        uint8_t h[5];
        if (std::fread(h, 1, 5, f) != 5) break;
        const size_t n = size_t(h[0]) | size_t(h[1]) << 8 | size_t(h[2]) << 16 | size_t(h[3]) << 24;
        std::vector<uint8_t> v(n);
        if (n && std::fread(v.data(), 1, n, f) != n) { std::fclose(f); return 2; }
        cases.push_back(v);
        want.push_back(h[4]);
    }
    std::fclose(f);
    if (cases.empty()) return 2;
    for (size_t k = 0; k < cases.size(); k++)
        if (int rc = run_one(cases[k].data(), cases[k].size(), want[k])) { std::fprintf(stderr, "case %zu\n", k); return rc; }
    uint8_t code;
    if (mjx_exif_orientation(nullptr, 4, &code) != MJX_ERR_INVALID_ARG || mjx_exif_orientation(cases[0].data(), cases[0].size(), nullptr) != MJX_ERR_INVALID_ARG) return 1;
    // truncations of the first case at every length, then seeded byte flips (one to four bytes, sometimes truncated as well)
    const std::vector<uint8_t> &base = cases[0];
    unsigned long done = 0;
    for (size_t n = 0; n <= base.size(); n++, done++)
        if (int rc = run_one(base.data(), n, 0)) return rc;
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (; done < mutations; done++) {
        std::vector<uint8_t> v = base;
        const unsigned flips = 1 + unsigned(next() % 4);
        for (unsigned k = 0; k < flips; k++) v[next() % v.size()] = (next() & 1) ? uint8_t(next()) : uint8_t(v[next() % v.size()] ^ (1u << (next() % 8)));
        const size_t n = (next() % 4 == 0) ? next() % (v.size() + 1) : v.size();
        if (int rc = run_one(v.data(), n, 0)) return rc;
    }
    std::printf("cases %zu mutations %lu\n", cases.size(), done);
    return 0;
}

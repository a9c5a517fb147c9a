// adobe_fuzz.cpp -- stand-alone driver for the parser's APP0 / APP14 / SOF paths under MJX_COLOR_FILE (tests/test_color_models.py builds
// it with mjx_parse.cpp under -fsanitize=address,undefined and runs it on the CPU).  Input: a file of cases, each a little-endian u32
// length, one byte with the model mjx_color_model must find (0xff: it must refuse the file), and the bytes.  Every case, and then
// seeded mutations of every case's head -- byte flips, and truncations at every length --, is handed to mjx_color_model and to
// mjx_parse (color = MJX_COLOR_FILE) in a heap block of exactly its size, so a read outside [jpeg, jpeg + len) is the sanitizer's to
// report.  Where both accept a file they must agree on its model.  Prints what it did; exits non-zero on a wrong model or status.
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
    mjx_color_info ci;
    std::memset(&ci, 0xee, sizeof ci);
    const int rc = mjx_color_model(blk, n, &ci);
    int bad = 0;
    if (rc != MJX_OK && rc != MJX_ERR_UNSUPPORTED_FORMAT) { std::fprintf(stderr, "mjx_color_model: status %d on %zu bytes\n", rc, n); bad = 1; }
    if (rc == MJX_OK && (ci.model > MJX_MODEL_YCCK || (ci.ncomp != 1 && ci.ncomp != 3 && ci.ncomp != 4))) { std::fprintf(stderr, "model %u of %u components\n", unsigned(ci.model), unsigned(ci.ncomp)); bad = 1; }
    if (rc != MJX_OK && (ci.model || ci.ncomp || ci.jfif || ci.adobe)) { std::fprintf(stderr, "a refused file leaves a filled struct\n"); bad = 1; }
    if (want >= 0 && want != 0xff && (rc != MJX_OK || ci.model != want)) { std::fprintf(stderr, "model %u (status %d), expected %d, on %zu bytes\n", unsigned(ci.model), rc, want, n); bad = 1; }
    if (want == 0xff && rc == MJX_OK) { std::fprintf(stderr, "accepted a file it must refuse (%zu bytes)\n", n); bad = 1; }
    mjx_opts o;
    std::memset(&o, 0, sizeof o);
    MJX_OPTS_COLOR(&o) = MJX_COLOR_FILE;
    mjx_scan_desc d;
    const int rp = mjx_parse(blk, n, &o, &d);
    if (rp == MJX_OK) {
        // (mjx_color_model reads the first frame header, mjx_parse keeps the last one: they agree where there is one)
        if (rc == MJX_OK && want >= 0 && want != 0xff && d.ncomp == ci.ncomp && d.model != ci.model) { std::fprintf(stderr, "mjx_parse says model %u, mjx_color_model %u\n", unsigned(d.model), unsigned(ci.model)); bad = 1; }
        if (d.model > MJX_MODEL_YCCK || d.ncomp > 4) { std::fprintf(stderr, "mjx_parse: model %u of %u components\n", unsigned(d.model), unsigned(d.ncomp)); bad = 1; }
        mjx_free_scan(&d);
    }
    std::free(blk);
    return bad;
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
    mjx_color_info ci;
    if (mjx_color_model(nullptr, 4, &ci) != MJX_ERR_INVALID_ARG || mjx_color_model(cases[0].data(), cases[0].size(), nullptr) != MJX_ERR_INVALID_ARG) return 1;
    // truncations of every case at every length of its head (up to the scan's first bytes), then seeded byte flips in the heads
    // (one to four bytes, sometimes truncated as well)
    unsigned long done = 0;
    std::vector<size_t> head(cases.size());
    for (size_t k = 0; k < cases.size(); k++) {
        const std::vector<uint8_t> &v = cases[k];
        size_t sos = v.size();
        for (size_t i = 0; i + 1 < v.size(); i++) if (v[i] == 0xff && v[i + 1] == 0xda) { sos = i; break; }
        head[k] = sos + 16 < v.size() ? sos + 16 : v.size();
        for (size_t n = 0; n <= head[k]; n++, done++)
            if (int rc = run_one(v.data(), n, -1)) return rc;
    }
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (; done < mutations; done++) {
        const size_t k = next() % cases.size();
        std::vector<uint8_t> v = cases[k];
        const unsigned flips = 1 + unsigned(next() % 4);
        for (unsigned q = 0; q < flips; q++) {
            const size_t at = next() % head[k];
            v[at] = (next() & 1) ? uint8_t(next()) : uint8_t(v[at] ^ (1u << (next() % 8)));
        }
        const size_t n = (next() % 3 == 0) ? next() % (v.size() + 1) : v.size();
        if (int rc = run_one(v.data(), n, -1)) return rc;
    }
    std::printf("cases %zu mutations %lu\n", cases.size(), done);
    return 0;
}

// prog_fuzz.cpp -- a stand-alone fuzz driver for the progressive path's host side (test infrastructure only).
//
// Built with -fsanitize=address,undefined together with mjx_parse.cpp, mjx_plan.cpp, mjx_lut.cpp and tests/emul/prog_emul.cpp and run
// directly (tests/test_progressive_host.py): for every file named on the command line it drives mjx_parse, the planner and the lane
// routine of mjx_prog.h (through prog_emul_decode, which runs every lane and the count / copy rule) over every truncation of the
// file and over seeded mutations of it -- single bytes, runs of bytes, and bytes of the marker segments.  Nothing here judges the
// answers: the sanitizers do, and the program's exit status is theirs.  Usage: prog_fuzz MUTATIONS FILE...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int prog_emul_decode(const uint8_t *jpeg, size_t len, int16_t *coefs, size_t cap_blocks, uint32_t *info, int *status);

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return uint32_t(rng_state >> 32);
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: prog_fuzz MUTATIONS FILE...\n"); return 2; }
    const long mutations = std::atol(argv[1]);
    const size_t cap = 4096;
    std::vector<int16_t> coefs(cap * 64);
    uint32_t info[6];
    long runs = 0, counts[16] = {0};
    for (int a = 2; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> file;
        for (int c; (c = std::fgetc(f)) != EOF;) file.push_back(uint8_t(c));
        std::fclose(f);
        auto run = [&](const std::vector<uint8_t> &d) {
            int status = 0;
            // (an exact-size heap copy: a read one byte past the input is the sanitizer's to find)
            std::vector<uint8_t> exact(d.begin(), d.end());
            if (prog_emul_decode(exact.data(), exact.size(), coefs.data(), cap, info, &status) != 0) status = 15;
            counts[status >= 0 && status < 16 ? status : 15]++;
            runs++;
        };
        for (size_t n = 0; n <= file.size(); n++) run(std::vector<uint8_t>(file.begin(), file.begin() + long(n)));
        for (long m = 0; m < mutations; m++) {
            std::vector<uint8_t> d = file;
            const uint32_t kind = rnd() % 4;
            const size_t at = rnd() % d.size();
            if (kind == 0) d[at] = uint8_t(rnd());
            else if (kind == 1) for (size_t k = at; k < d.size() && k < at + 1 + rnd() % 8; k++) d[k] = uint8_t(rnd());
            else if (kind == 2) d[at] ^= uint8_t(1u << (rnd() % 8));
            else { const size_t head = d.size() < 700 ? d.size() : 700; d[rnd() % head] = uint8_t(rnd()); }      // the segments in front of the scans
            run(d);
        }
    }
    std::printf("runs %ld:", runs);
    for (int k = 0; k < 16; k++) if (counts[k]) std::printf(" status%d=%ld", k, counts[k]);
    std::printf("\n");
    return 0;
}

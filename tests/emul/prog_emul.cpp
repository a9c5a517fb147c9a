// prog_emul.cpp -- CPU emulation of the progressive path (test infrastructure only).
//
// Runs what the device runs, serially: mjx_parse and the planner as they are, the layout routine the batch uses (prog_layout), the
// per-lane routine of k_prog_scan (prog_lane, mjx_prog.h) lane by lane and level by level into a dense store, and the count / copy
// rule of k_prog_count / k_prog_copy (prog_slot, prog_block_count, prog_block_emit) tile by tile into the linear stream, tile
// offsets and DC values that stage B reads -- which are then expanded into blocks the way mjx_batch_copy_coefs expands them.
#include "mjx.h"
#include "mjx_kernels.h"
#include "mjx_plan.h"
#include "mjx_prog.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mjx;

namespace {
struct Store {                                   // 16-byte aligned, as the device's
    int16_t *p = nullptr;
    explicit Store(size_t n) { p = static_cast<int16_t *>(std::aligned_alloc(64, (n * 2 + 63) / 64 * 64 + 64)); if (p) std::memset(p, 0, (n * 2 + 63) / 64 * 64 + 64); }
    ~Store() { std::free(p); }
};
}

// Decodes one file.  status: what the library would report for it (a planner's refusal, or MJX_OK / MJX_ERR_TRUNCATED /
// MJX_ERR_BAD_HUFFMAN from the lanes' flags).  coefs: nblocks x 64 in MCU order, zig-zag order inside a block, written when the
// status is MJX_OK.  info: width, height, blocks per MCU, MCUs, levels, lanes.  Returns 0, or -1 when coefs is too small.
extern "C" int prog_emul_decode(const uint8_t *jpeg, size_t len, int16_t *coefs, size_t cap_blocks, uint32_t *info, int *status)
{
    mjx_opts o;
    std::memset(&o, 0, sizeof o);
    MJX_OPTS_PROGRESSIVE(&o) = 1;
    mjx_scan_desc d;
    *status = mjx_parse(jpeg, len, &o, &d);
    if (*status != MJX_OK) return 0;
    std::vector<ImagePlan> plans;
    plan_input(d, o, plans);
    const ImagePlan &p = plans.back();
    *status = p.status;
    if (p.status != MJX_OK || !p.prog) { if (p.status == MJX_OK) *status = -1; mjx_free_scan(&d); return 0; }
    if (cap_blocks < size_t(p.nmcu) * p.bpm) { mjx_free_scan(&d); return -1; }       // (before anything is sized by the picture)
    ProgPic pic;
    std::vector<std::vector<ProgLane>> levels;
    std::vector<uint8_t> bytes;
    const uint64_t elems = prog_layout(p, 0, 0, 0, pic, levels, bytes);
    bytes.resize(bytes.size() + 16, 0);
    Store store(elems);
    uint32_t flags = 0, nlanes = 0;
    for (const std::vector<ProgLane> &lv : levels)
        for (const ProgLane &ln : lv) { flags |= prog_lane(ln, pic, bytes.data(), p.lut.data(), store.p); nlanes++; }
    const size_t nblocks = size_t(p.nmcu) * p.bpm;
    info[0] = p.width; info[1] = p.height; info[2] = p.bpm; info[3] = p.nmcu; info[4] = uint32_t(levels.size()); info[5] = nlanes;
    mjx_free_scan(&d);
    if (flags) { *status = (flags & kProgShort) ? MJX_ERR_TRUNCATED : MJX_ERR_BAD_HUFFMAN; return 0; }
    // the count / copy rule, a tile at a time
    const uint32_t T = tile_mcus(p.bpm, p.hmax), tile_blocks = T * p.bpm, ntiles = (p.nmcu + T - 1) / T;
    std::vector<uint32_t> eoff(ntiles + 1, 0), entries;
    std::vector<int32_t> dc(nblocks, 0);
    for (uint32_t t = 0; t < ntiles; t++) {
        uint32_t total = 0;
        for (uint32_t tid = 0; tid < tile_blocks; tid++) {
            const uint32_t m = t * T + tid / p.bpm, k = tid % p.bpm;
            if (m >= p.nmcu) continue;
            const ProgSlot s = prog_slot(pic, m, p.blk_comp[k], p.blk_bx[k], p.blk_by[k]);
            dc[size_t(t) * tile_blocks + tid] = s.real ? store.p[s.at] : 0;
            if (!s.real) continue;
            const uint32_t cnt = prog_block_count(store.p + s.at);
            entries.resize(entries.size() + cnt);
            const uint32_t wrote = prog_block_emit(store.p + s.at, (t * tile_blocks + tid) & 0xffu, entries.data() + entries.size() - cnt);
            if (wrote != cnt) { *status = MJX_ERR_DEVICE; return 0; }
            total += cnt;
        }
        eoff[t + 1] = eoff[t] + total;
    }
    std::memset(coefs, 0, nblocks * 128);
    for (uint32_t t = 0; t < ntiles; t++) {                      // (mjx_batch_copy_coefs' expansion of a linear stream)
        const uint32_t first = t * tile_blocks;
        for (uint32_t j = eoff[t]; j < eoff[t + 1]; j++) {
            const uint32_t e = entries[j];
            const uint64_t blk = first + (((e >> 22) - first) & 0xffu);
            if (blk < nblocks) coefs[blk * 64 + ((e >> 16) & 63)] = int16_t(e & 0xffff);
        }
    }
    for (size_t k = 0; k < nblocks; k++) coefs[k * 64] = int16_t(dc[k]);
    return 0;
}

// Host-only: the level of every scan of a progressive file, as the planner numbers them (0 entries on a refusal).
extern "C" int prog_emul_levels(const uint8_t *jpeg, size_t len, uint32_t *levels, size_t cap)
{
    mjx_opts o;
    std::memset(&o, 0, sizeof o);
    MJX_OPTS_PROGRESSIVE(&o) = 1;
    mjx_scan_desc d;
    if (mjx_parse(jpeg, len, &o, &d) != MJX_OK) return 0;
    std::vector<ImagePlan> plans;
    plan_input(d, o, plans);
    int n = 0;
    if (plans.back().status == MJX_OK)
        for (const ProgScanPlan &s : plans.back().pscans) if (size_t(n) < cap) levels[n++] = s.level;
    mjx_free_scan(&d);
    return n;
}

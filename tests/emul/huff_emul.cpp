// huff_emul.cpp -- CPU emulation of the GPU entropy-decode *algorithm* (test infrastructure only).
//
// Runs the same per-lane routine the HIP kernels run (jpeg-rust_amd/csrc/mjx_huff.h) over every
// subsequence sequentially, in the kernels' phase order: speculative pass, intra-workgroup
// synchronisation, inter-workgroup fix passes, block-count scan, write pass, DC prefix sum.
// It lets the CPU test-suite check the decode tables, the symbol step and the convergence of the
// self-synchronising scheme against the oracle without a GPU.  It is never linked into libmjx.so.
#include "mjx.h"
#include "mjx_huff.h"
#include "mjx_kernels.h"
#include "mjx_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mjx;

namespace {
struct HostBits {
    const uint8_t *p;
    size_t n;
    uint32_t be32(uint32_t byte_off) const
    {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++) {
            const size_t idx = size_t(byte_off) + k;
            w = (w << 8) | (idx < n ? p[idx] : 0xaau);
        }
        return w;
    }
    uint32_t ahead(uint32_t byte_off) const { return be32(byte_off); }
    void advance() const {}
};
// Mirrors the device sink of k_huff_write: AC entries appended to the compact stream, DC differences per block,
// the stream offset of every tile's first block.
struct StreamSink {
    uint32_t *entries;
    int16_t *dcbuf;
    uint32_t *tile_eoff;
    uint32_t tile_blocks, total_blocks;
    uint32_t off;
    int *bad;
    void dc(uint32_t b, int v)
    {
        dcbuf[b] = int16_t(v);
        if (b % tile_blocks == 0) tile_eoff[b / tile_blocks] = off;
    }
    void ac(uint32_t b, uint32_t r_scaled, int v) { entries[off++] = coef_entry(v, 63u - (r_scaled >> kRShift), b); }
    void block_done(uint32_t next_blk)
    {
        if (next_blk == total_blocks) tile_eoff[(total_blocks + tile_blocks - 1) / tile_blocks] = off;
    }
    void bad_code(uint32_t, uint32_t) const { *bad = 1; }
    void tick() const {}
};
// The same for the quad-interleaved stream (pictures of one scan on the device, mjx_kernels.h: stream_phys): the lane's entries go
// to its own column, a tile offset is the virtual index subsequence * column capacity + entry.
struct QuadSink {
    uint32_t *col;          // the columns (behind the run-length head of the region)
    int16_t *dcbuf;
    uint32_t *tile_eoff;
    uint32_t tile_blocks, total_blocks;
    uint32_t s, rows, off;
    int *bad;
    void dc(uint32_t b, int v)
    {
        dcbuf[b] = int16_t(v);
        if (b % tile_blocks == 0) tile_eoff[b / tile_blocks] = s * (rows * 8u) + off;
    }
    void ac(uint32_t b, uint32_t r_scaled, int v)
    {
        if (off >= rows * 8u) { *bad = 6; return; }                 // (a column holds any run: an entry takes two bits of scan at least)
        col[stream_phys(s, off++, rows)] = coef_entry(v, 63u - (r_scaled >> kRShift), b);
    }
    void block_done(uint32_t next_blk)
    {
        if (next_blk == total_blocks) tile_eoff[(total_blocks + tile_blocks - 1) / tile_blocks] = s * (rows * 8u) + off;
    }
    void bad_code(uint32_t, uint32_t) const { *bad = 1; }
    void tick() const {}
};
struct TickSink {
    mutable long ticks = 0;
    void dc(uint32_t, int) const {}
    void ac(uint32_t, uint32_t, int) const {}
    void block_done(uint32_t) const {}
    void bad_code(uint32_t, uint32_t) const {}
    void tick() const { ticks++; }
};
struct HostCps {
    uint32_t *w;     // 2 words per checkpoint
    uint32_t get(uint32_t k) const { return w[2 * k]; }
    uint32_t get_m(uint32_t k) const { return w[2 * k + 1]; }
    CpPair get_pair(uint32_t k) const { return CpPair{w[2 * k], w[2 * k + 1]}; }
    void set(uint32_t k, uint32_t v, uint32_t m) const { w[2 * k] = v; w[2 * k + 1] = m; }
};
}   // namespace

// Emulates the kernel sequence  k_huff_spec -> k_huff_merge rounds -> k_huff_scan -> k_huff_write -> DC prediction.
// `mode`: 0 = rounds see a snapshot of the previous round's exits (what fully concurrent lanes see in the worst case),
//         1 = rounds update in place in subsequence order (what a single lane walking the items would see).
// `sub_base_bits`: 0 = the subsequence length plan_image chooses; otherwise the scan is re-cut into subsequences of about
// that many bits (replan_subsequences: what build_batch does for batches too small to fill the device).
extern "C" int emul_decode_coefs_sub(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, int16_t *out,
                                     size_t cap_blocks, size_t *nblocks, int *stats /* [8] */);
extern "C" int emul_decode_coefs(const uint8_t *jpeg, size_t len, int layout, int mode, int16_t *out,
                                 size_t cap_blocks, size_t *nblocks, int *stats /* [8] */)
{
    return emul_decode_coefs_sub(jpeg, len, layout, mode, 0, out, cap_blocks, nblocks, stats);
}
// (..._color: the same with mjx_opts.color = `color` (MJX_COLOR_*): MJX_COLOR_FILE admits four-component files)
extern "C" int emul_decode_coefs_sub_color(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, int16_t *out,
                                           size_t cap_blocks, size_t *nblocks, int *stats /* [8] */, int color)
{
    mjx_opts opts{};
    opts.layout = uint8_t(layout);
    MJX_OPTS_COLOR(&opts) = uint8_t(color);
    mjx_scan_desc d;
    int rc = mjx_parse(jpeg, len, &opts, &d);
    if (rc) return rc;
    ImagePlan plan;
    rc = plan_image(d, opts, plan);
    if (rc) { mjx_free_scan(&d); return rc; }
    if (sub_base_bits) replan_subsequences(plan, sub_base_bits);
    if (plan.restart_mcus) { mjx_free_scan(&d); return MJX_ERR_DRI_UNSUPPORTED; }   // (restart intervals: GPU tests only)
    const HuffImage &img = plan.himg;
    // the counting passes (k_huff_spec, the merge rounds) use the image's second table set: AC tables with a pair part, two
    // symbols per step where they can (mjx_huff.h); the write pass the plain one
    HuffImage img2 = img;
    for (uint32_t k = 0; k < uint32_t(kMaxBlocksPerMcu); k++) img2.btab[k].tabs = img.tabs_pair[k];
    const LutEntry *lut2 = plan.lut.data() + plan.lut_plain_n;
    const HostBits bits{plan.scan, plan.scan_len};
    const uint32_t nsub = img.nsub;
    std::vector<SubseqState> g_entry(nsub), g_exit(nsub);
    std::vector<uint32_t> g_cps(size_t(nsub) * kMaxCp * 2, 0xdeadbeefu);  // uninitialised on the device
    TickSink ns;
    NoCheckpoints nocp;
    std::vector<std::vector<long>> iter_ticks;
    const char *dump = std::getenv("MJX_EMUL_DUMP");
    auto end_of = [&](uint32_t s) { uint64_t e = uint64_t(s + 1) * img.sub_bits; return uint32_t(e < img.total_bits ? e : img.total_bits); };
    long redecodes = 0, rounds = 0;

    iter_ticks.emplace_back();
    for (uint32_t s = 0; s < nsub; s++) {                                  // k_huff_spec
        const SubseqState e = make_state(s * img.sub_bits, 0, 0);
        HostCps hc{g_cps.data() + size_t(s) * kMaxCp * 2};
        const long t0 = ns.ticks;
        g_exit[s] = decode_subseq<false, 1, true>(bits, lut2, img2, e, end_of(s), 0, ns, hc, s * img.sub_bits, e);
        g_entry[s] = e;
        iter_ticks[0].push_back(ns.ticks - t0);
    }
    // Two generations per subsequence (Gen2, mjx_kernels.hip; MJX_MERGE_MEMO=0 or mode 1: one, the loop below): the decode before the
    // last is kept -- entry, exit, checkpoints -- in a second set, gen[s] bit 0 = the current set, bit 1 = the other one holds a
    // decode.  A round: every workgroup's worth of lanes first takes remembered decodes back in a sweep (round_begin), then the lanes
    // that still do not start where their predecessor ended decode again, recording in a scratch set and comparing with both
    // recorded paths (merge_slice), and settle as merge_finish does.  Rounds see the previous round's exits (mode 0).
    const char *memo_env = std::getenv("MJX_MERGE_MEMO");
    const bool two = mode == 0 && !(memo_env && std::atoi(memo_env) == 0);
    if (two) {
        std::vector<SubseqState> ent[3], ext[2];
        std::vector<uint32_t> cp[3];
        std::vector<uint8_t> gen(nsub, 0);
        ent[0] = g_entry; ent[1].assign(nsub, make_state(0, 0, 0)); ent[2] = ent[1];
        ext[0] = g_exit; ext[1].assign(nsub, make_state(0, 0, 0));
        cp[0] = g_cps; cp[1].assign(g_cps.size(), 0xdeadbeefu); cp[2] = cp[1];
        auto cps_of = [&](int k, uint32_t s) { return HostCps{cp[k].data() + size_t(s) * kMaxCp * 2}; };
        for (;;) {
            long changed = 0;
            iter_ticks.emplace_back();
            std::vector<SubseqState> snap_exit(nsub);
            for (uint32_t s = 0; s < nsub; s++) snap_exit[s] = ext[gen[s] & 1][s];
            std::vector<char> active(nsub, 0);
            std::vector<SubseqState> start(nsub);
            for (uint32_t w0 = 1; w0 < nsub; w0 += uint32_t(kMergeWg)) {      // a merge workgroup: lanes w0 .. w0 + kMergeWg - 1
                const uint32_t w1 = std::min<uint32_t>(nsub, w0 + uint32_t(kMergeWg));
                std::vector<SubseqState> cur_exit(w1 - w0);
                std::vector<char> flipped(w1 - w0, 0);
                for (uint32_t s = w0; s < w1; s++) cur_exit[s - w0] = ext[gen[s] & 1][s];
                for (uint32_t iter = 0; iter < uint32_t(kMergeWg); iter++) {
                    std::vector<char> flip(w1 - w0, 0);
                    bool any = false;
                    for (uint32_t s = w0; s < w1; s++) {
                        const SubseqState prev = s == w0 ? snap_exit[s - 1] : cur_exit[s - 1 - w0];
                        const uint32_t c = gen[s] & 1;
                        if ((gen[s] & 2) && !same_entry(prev, ent[c][s]) && same_entry(prev, ent[c ^ 1][s])) { flip[s - w0] = 1; any = true; }
                    }
                    if (!any) break;
                    for (uint32_t s = w0; s < w1; s++)
                        if (flip[s - w0]) { gen[s] = uint8_t((gen[s] & 1) ^ 1) | 2; cur_exit[s - w0] = ext[gen[s] & 1][s]; flipped[s - w0] = 1; }
                }
                for (uint32_t s = w0; s < w1; s++) {
                    const SubseqState prev = s == w0 ? snap_exit[s - 1] : cur_exit[s - 1 - w0];
                    active[s] = !same_entry(prev, ent[gen[s] & 1][s]);
                    start[s] = make_state(prev.p, prev.z, prev.c);
                    if (active[s] || flipped[s - w0]) changed++;
                }
            }
            for (uint32_t s = 1; s < nsub; s++) {
                if (!active[s]) continue;
                const uint32_t cset = gen[s] & 1, oset = cset ^ 1;
                const bool other_valid = (gen[s] & 2) != 0;
                const SubseqState e = start[s];
                ent[2][s] = e;
                const HostCps cc = cps_of(int(cset), s), co = cps_of(int(oset), s), cw = cps_of(2, s);
                uint32_t met = 0, nrec = 0;
                SubseqState x = make_state(e.p, e.z, e.c);
                const long t0 = ns.ticks;
                if (e.p <= s * img.sub_bits + band_end(end_of(s) - s * img.sub_bits)) {
                    LaneState st; LaneEvents ev;
                    lane_begin(st, bits, img2, e);
                    events_begin<2>(ev, s * img.sub_bits, end_of(s), img2.cp_bits);
                    uint32_t blk = 0;
                    for (;;) {
                        const bool crossed = symbol_step<false, true>(st, bits, lut2, img2, blk, ns);
                        if (!crossed || st.wn < ev.next_wn) continue;
                        if (st.wn >= ev.end_wn) break;
                        const uint32_t state = cp_state_word(st);
                        const uint32_t w_c = cc.get(ev.k), w_o = other_valid ? co.get(ev.k) : 0u;
                        if ((w_c & kCpStateMask) == state) {
                            met = 1;
                            x = make_state(ext[cset][s].p, ext[cset][s].z, ext[cset][s].c, st.n + ((w_c >> 16) & 0x7fffu), lane_m(st) + cc.get_m(ev.k));
                            break;
                        }
                        if (other_valid && (w_o & kCpStateMask) == state) {
                            met = 2;
                            x = make_state(ext[oset][s].p, ext[oset][s].z, ext[oset][s].c, st.n + ((w_o >> 16) & 0x7fffu), lane_m(st) + co.get_m(ev.k));
                            break;
                        }
                        cw.set(ev.k, state | (st.n << 16), lane_m(st));
                        ev.k++;
                        ev.next_wn += ev.cp_bytes;
                        if (ev.next_wn > ev.end_wn) ev.next_wn = ev.end_wn;
                    }
                    nrec = ev.k;
                    if (!met) x = make_state(lane_pos(st), lane_z(st), lane_c(st, img2), st.n, lane_m(st));
                }
                iter_ticks.back().push_back(ns.ticks - t0);
                const uint32_t dset = met == 1 ? cset : oset;
                const HostCps dst = cps_of(int(dset), s);
                for (uint32_t j = 0; j < nrec; j++) {
                    const CpPair v = cw.get_pair(j);
                    dst.set(j, (v.w & kCpStateMask) | ((x.n - ((v.w >> 16) & 0x7fffu)) << 16), x.m - v.m);
                }
                ent[dset][s] = ent[2][s];
                ext[dset][s] = x;
                if (met != 1) gen[s] = uint8_t(oset | 2);
                redecodes++;
            }
            rounds++;
            if (changed == 0) break;
            if (rounds > 100000) return MJX_ERR_INVALID_ARG;
        }
        for (uint32_t s = 0; s < nsub; s++) { g_entry[s] = ent[gen[s] & 1][s]; g_exit[s] = ext[gen[s] & 1][s]; }      // (k_huff_scan folds the sets)
    }
    for (; !two;) {                                                        // k_huff_merge rounds, one recorded decode per subsequence
        long redone = 0;
        iter_ticks.emplace_back();
        std::vector<SubseqState> snap;
        if (mode == 0) snap = g_exit;
        for (uint32_t s = 1; s < nsub; s++) {
            const SubseqState prev = mode == 0 ? snap[s - 1] : g_exit[s - 1];
            if (same_entry(prev, g_entry[s])) continue;
            const SubseqState e = make_state(prev.p, prev.z, prev.c);
            g_entry[s] = e;
            HostCps hc{g_cps.data() + size_t(s) * kMaxCp * 2};
            const long t0 = ns.ticks;
            g_exit[s] = decode_subseq<false, 2, true>(bits, lut2, img2, e, end_of(s), 0, ns, hc, s * img.sub_bits, g_exit[s]);
            iter_ticks.back().push_back(ns.ticks - t0);
            redone++;
        }
        rounds++;
        redecodes += redone;
        if (redone == 0) break;
    }
    if (dump) {
        for (size_t it = 0; it < iter_ticks.size(); it++) {
            auto &v = iter_ticks[it];
            if (v.empty()) continue;
            std::sort(v.begin(), v.end());
            long sum = 0; for (long x : v) sum += x;
            std::fprintf(stderr, "pass %zu: items %zu mean %.1f p50 %ld p90 %ld p99 %ld max %ld\n", it, v.size(), double(sum) / v.size(), v[v.size() / 2], v[v.size() * 9 / 10], v[v.size() * 99 / 100], v.back());
        }
    }
    // k_huff_scan + k_huff_write + DC prediction + expansion of the compact stream
    std::vector<uint32_t> blkbase(nsub), ebase(nsub);
    uint32_t acc = 0, eacc = 0;
    for (uint32_t s = 0; s < nsub; s++) { blkbase[s] = acc; ebase[s] = eacc; acc += g_exit[s].n; eacc += g_exit[s].m; }
    const size_t nb = img.total_blocks;
    *nblocks = nb;
    int bad = 0;
    const bool truncated = acc < nb;          // k_huff_scan: the picture is flagged and every later kernel skips it
    if (truncated) bad = 3;
    if (nb <= cap_blocks && !truncated) {
        const uint32_t tile_blocks = tile_mcus(plan.bpm, plan.hmax) * plan.bpm;
        const uint32_t ntiles = uint32_t((nb + tile_blocks - 1) / tile_blocks);
        std::vector<uint32_t> entries(size_t(eacc) + 1, 0xffffffffu), tile_eoff(ntiles + 1, 0xffffffffu);
        std::vector<int16_t> dcb(nb, 0);
        for (uint32_t s = 0; s < nsub; s++) {
            StreamSink sink{entries.data(), dcb.data(), tile_eoff.data(), tile_blocks, uint32_t(nb), ebase[s], &bad};
            decode_subseq<true, 0>(bits, plan.lut.data(), img, g_entry[s], end_of(s), blkbase[s], sink, nocp, 0, g_exit[s]);
            // the entry count of the synchronisation passes must be exact for every subsequence that lies inside the image
            if (blkbase[s] + g_exit[s].n < nb && sink.off - ebase[s] != g_exit[s].m) { if (dump && !bad) std::fprintf(stderr, "m mismatch s=%u got %u want %u n=%u\n", s, sink.off - ebase[s], g_exit[s].m, g_exit[s].n); bad = 2; }
        }
        std::memset(out, 0, nb * 64 * sizeof(int16_t));
        for (uint32_t t = 0; t < ntiles; t++) {
            if (tile_eoff[t] == 0xffffffffu || tile_eoff[t + 1] == 0xffffffffu) { bad = 3; break; }
            for (uint32_t j = tile_eoff[t]; j < tile_eoff[t + 1]; j++) {
                const uint32_t e = entries[j];
                const uint32_t blk = t * tile_blocks + (((e >> 22) - t * tile_blocks) & 0xffu);
                if (blk >= nb) { bad = 4; break; }
                out[size_t(blk) * 64 + ((e >> 16) & 63)] = int16_t(e & 0xffff);
            }
        }
        // The write pass once more into the quad-interleaved layout, expanded the way stage B reads it (quad_prepare + quad_cell,
        // the functions the kernel runs): every group of every tile, masked at the tile's ends -- must give the same blocks.
        if (!bad) {
            const uint32_t rows = stream_rows_for(img.sub_bits), cap = rows * 8u, hdr = stream_hdr_entries(nsub);
            std::vector<uint32_t> region(size_t(hdr) + size_t(stream_quad_entries(nsub, rows)), 0xdeadbeefu), eoff2(ntiles + 1, 0xffffffffu);
            std::vector<int16_t> dcb2(nb, 0), out2(nb * 64, 0);
            uint32_t *runs = region.data();                                        // one run word per subsequence (mjx_kernels.h: run_word)
            for (uint32_t s = 0; s < nsub; s++) {
                QuadSink sink{region.data() + hdr, dcb2.data(), eoff2.data(), tile_blocks, uint32_t(nb), s, rows, 0u, &bad};
                decode_subseq<true, 0>(bits, plan.lut.data(), img, g_entry[s], end_of(s), blkbase[s], sink, nocp, 0, g_exit[s]);
                while (sink.off & 7u) region[hdr + stream_phys(s, sink.off++, rows)] = 0u;       // null entries up to the group boundary
                runs[s] = run_word(0u, sink.off >> 3, 0u);
            }
            for (uint32_t t = 0; t < ntiles && !bad; t++) {
                if (eoff2[t] == 0xffffffffu || eoff2[t + 1] == 0xffffffffu) { bad = 7; break; }
                const uint32_t sub[2] = {eoff2[t] / cap, eoff2[t + 1] / cap};
                const uint16_t at[2] = {uint16_t(eoff2[t] % cap), uint16_t(eoff2[t + 1] % cap)};
                QuadCum cum;
                QuadView q{sub, at, &cum, runs, rows, nsub};
                cum = quad_prepare(q, 0);
                QuadCell cell;
                const uint32_t total = quad_cell(q, 0, 0, cell);
                for (uint32_t o = 0; o < total; o++) {
                    if (quad_cell(q, 0, o, cell) != total || cell.phys == 0xffffffffu) { bad = 8; break; }
                    for (uint32_t k = cell.k_lo; k < cell.k_hi; k++) {
                        const uint32_t e = region[hdr + cell.phys + k];
                        if (((e >> 16) & 63) == 0) continue;                                   // null entry
                        const uint32_t blk = t * tile_blocks + (((e >> 22) + cell.label - t * tile_blocks) & 0xffu);
                        if (blk >= nb || blk / tile_blocks != t) { bad = 9; break; }
                        out2[size_t(blk) * 64 + ((e >> 16) & 63)] = int16_t(e & 0xffff);
                    }
                }
            }
            if (!bad && (std::memcmp(out2.data(), out, nb * 64 * sizeof(int16_t)) != 0 || dcb2 != dcb)) bad = 10;
        }
        int32_t pred[4] = {0, 0, 0, 0};            // (a fourth component with MJX_COLOR_FILE)
        for (size_t b = 0; b < nb; b++) {
            const int c = plan.blk_comp[b % plan.bpm];
            pred[c] += dcb[b];
            out[b * 64] = int16_t(pred[c]);
        }
    }
    if (stats) {
        stats[0] = int(nsub); stats[1] = int(rounds); stats[2] = int(redecodes); stats[3] = int(rounds);
        stats[4] = int(plan.bpm); stats[5] = int(plan.lut.size()); stats[6] = bad; stats[7] = 0;
    }
    mjx_free_scan(&d);
    if (nb > cap_blocks) return MJX_ERR_NOMEM;
    return truncated ? MJX_ERR_TRUNCATED : bad ? MJX_ERR_BAD_HUFFMAN : MJX_OK;      // (as mjx_batch_wait: truncated wins)
}
extern "C" int emul_decode_coefs_sub(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, int16_t *out,
                                     size_t cap_blocks, size_t *nblocks, int *stats /* [8] */)
{
    return emul_decode_coefs_sub_color(jpeg, len, layout, mode, sub_base_bits, out, cap_blocks, nblocks, stats, MJX_COLOR_POSITIONAL);
}

// ---- single decode (round 5): the counting pass emits ------------------------------------------------------------------
// Emulates  k_huff_emit -> k_huff_merge rounds (count only, with the merge depth kept) -> k_huff_scan -> k_huff_prefix -> k_block_gather
// and the expansion stage B performs, on the CPU:
//   * every lane warms up over the last `warm_bits` bits of the subsequence before its own (count only, from the guess "a block
//     starts here") and then decodes its own subsequence ONCE, emitting -- entries into its column from index H on, labelled with
//     the number of blocks it has completed (not the block's index in the picture, which it cannot know), one word {DC difference,
//     column index where the block's entries start} per block into its block column from index Hb on -- and recording checkpoints;
//   * the merge rounds find the true entries as before; per subsequence the deepest merge point of its re-decodes is kept (kfix);
//   * lanes whose entry was wrong re-decode from the true entry up to that checkpoint and write the prefix RIGHT-ALIGNED against
//     the first entry / block word of the first decode that is valid, with labels continuing into that decode's;
//   * block bases (scan) give every subsequence's label -> block offset; the gather turns block columns into dcdiff[] and tile offsets.
// out/nblocks as emul_decode_coefs_sub.  stats: [0] nsub [1] rounds [2] lanes re-decoded by the prefix pass [3] symbols of the prefix pass
// [4] symbols of the merge rounds [5] max(m_prefix - j0K) [6] bad [7] max(n_prefix - n0K)
namespace {
struct EmitSink {                  // first decode and prefix pass: the column of one subsequence (entries upwards, block words from the top downwards)
    uint32_t *col;
    uint32_t s, rows, eoff, boff;             // next entry index in the column; block word index = boff + label
    uint32_t label_add;                       // what is added to the decode's own block count to give the label
    uint32_t e_lo, e_hi;                      // bounds the entry indices must stay inside (a violation = fall back to the two-pass path)
    uint32_t bad_label; int *overflow;
    uint32_t bad_pos = 0;
    uint32_t bad_last = 0xffffffffu, bad_tail = 0xffffffffu, nbad = 0;   // EmitSub::bad_last, bad_tail: position inside the subsequence | label << 16
    uint32_t bad_tail2 = 0xffffffffu;                    // EmitSub::bad_tail2
    uint32_t sub_start = 0, tail_start = 0, tail_cp = 0; // the subsequence's first bit; emit_tail_start, emit_tail_cp
    uint32_t lowest_bword = 0xffffffffu;      // lowest column index a block word went to (entries must stay below it)
    long ticks = 0;
    void dc(uint32_t b, int v)
    {
        const uint32_t j = block_word_index(boff + b, rows);
        if (j >= rows * 8u || j < eoff) { *overflow = 1; return; }
        lowest_bword = std::min(lowest_bword, j);
        col[stream_phys(s, j, rows)] = (uint32_t(v) & 0xffffu) | (eoff << 16);
    }
    void ac(uint32_t b, uint32_t r_scaled, int v)
    {
        if (eoff < e_lo || eoff >= e_hi || eoff >= lowest_bword) { *overflow = 1; return; }
        col[stream_phys(s, eoff++, rows)] = coef_entry(v, 63u - (r_scaled >> kRShift), b + label_add);
    }
    void block_done(uint32_t) const {}
    void bad_code(uint32_t b, uint32_t pos)
    {
        if (bad_label == 0xffffffffu) { bad_label = b; bad_pos = pos; }
        nbad++;
        if (pos - sub_start < tail_start) bad_last = ((pos - sub_start) & 0xffffu) | (b << 16);
        else {
            if (bad_tail == 0xffffffffu) bad_tail = ((pos - sub_start) & 0xffffu) | (b << 16);
            if (pos - sub_start > tail_cp && bad_tail2 == 0xffffffffu) bad_tail2 = ((pos - sub_start) & 0xffffu) | (b << 16);
        }
    }
    void tick() { ticks++; }
};
}   // namespace

extern "C" int emul_single_decode_cp(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                     unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */);
extern "C" int emul_single_decode_lanes(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                        unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */,
                                        uint32_t *lanes /* [lanes_cap][4] */, size_t lanes_cap);
extern "C" int emul_single_decode(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                  unsigned headroom_groups, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */)
{
    return emul_single_decode_cp(jpeg, len, layout, mode, sub_base_bits, warm_bits, headroom_groups, 0, out, cap_blocks, nblocks, stats);
}
// cp_bits: bits between the checkpoints the emitting decode records (0: kCpBits; a multiple of kCpBits)
extern "C" int emul_single_decode_cp(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                     unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */)
{
    return emul_single_decode_lanes(jpeg, len, layout, mode, sub_base_bits, warm_bits, headroom_groups, cp_bits, out, cap_blocks, nblocks, stats, nullptr, 0);
}
// lanes: per subsequence (the first lanes_cap of them) what the first decode knows of the bit patterns no code matched --
//   [0] position of the first one inside the subsequence (0xffffffff: none)   [1] the merge point pK inside the subsequence (0: the
//   lane's entry was right, everything it decoded stays; 0xffffffff: nothing stays)   [2] position of a later one the sink keeps   [3] how many
// and behind the last subsequence's a row {bits per subsequence, subsequences, bits between checkpoints, warm-up bits}.
// A lane with [0] < [1] has spent "the first one" on a code that does not count: what k_huff_prefix decides on is the last one.
// (..._color: the same with mjx_opts.color = `color`, as emul_decode_coefs_sub_color)
extern "C" int emul_single_decode_lanes_color(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                              unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */,
                                              uint32_t *lanes, size_t lanes_cap, int color)
{
    mjx_opts opts{};
    opts.layout = uint8_t(layout);
    MJX_OPTS_COLOR(&opts) = uint8_t(color);
    mjx_scan_desc d;
    int rc = mjx_parse(jpeg, len, &opts, &d);
    if (rc) return rc;
    ImagePlan plan;
    rc = plan_image(d, opts, plan);
    if (rc) { mjx_free_scan(&d); return rc; }
    if (sub_base_bits) replan_subsequences(plan, sub_base_bits);
    if (plan.restart_mcus) { mjx_free_scan(&d); return MJX_ERR_DRI_UNSUPPORTED; }
    const uint32_t CPB = cp_bits ? std::max<uint32_t>(uint32_t(kCpBits), cp_bits / uint32_t(kCpBits) * uint32_t(kCpBits)) : uint32_t(kCpBits);
    plan.himg.cp_bits = CPB;
    const HuffImage &img = plan.himg;
    HuffImage img2 = img;                                                     // counting passes: the table set with pair parts
    for (uint32_t k = 0; k < uint32_t(kMaxBlocksPerMcu); k++) img2.btab[k].tabs = img.tabs_pair[k];
    const LutEntry *lut2 = plan.lut.data() + plan.lut_plain_n;
    HuffImage imgw = img;                                                     // emitting passes: no "last block" to stop at
    imgw.total_blocks = 0xffffffffu;
    const HostBits bits{plan.scan, plan.scan_len};
    const uint32_t nsub = img.nsub, L = img.sub_bits;
    const uint32_t W = std::min<uint32_t>(warm_bits / 32u * 32u, L);
    headroom_groups = std::min<unsigned>(headroom_groups, kEmitHeadGroups);
    const uint32_t H = headroom_groups * 8u, Hb = headroom_groups * 4u;       // head room in front of the first decode's entries / block words (DevImage::emit_head)
    const uint32_t rows = stream_rows_for(L), cap = rows * 8u;
    auto end_of = [&](uint32_t s) { uint64_t e = uint64_t(s + 1) * L; return uint32_t(e < img.total_bits ? e : img.total_bits); };
    const uint32_t hdr = stream_hdr_entries(nsub);
    std::vector<uint32_t> whole(size_t(hdr) + size_t(stream_quad_entries(nsub, rows)), 0xdeadbeefu);
    uint32_t *runs = whole.data(), *region = whole.data() + hdr;
    std::vector<SubseqState> g_entry(nsub), g_exit(nsub);
    std::vector<uint32_t> g_cps(size_t(nsub) * kMaxCp * 2, 0xdeadbeefu), d0n(nsub), d0m(nsub), kfix(nsub, 0), badl(nsub, 0xffffffffu), badp(nsub, 0), badq(nsub, 0xffffffffu), badql(nsub, 0), badq2(nsub, 0xffffffffu);
    constexpr uint32_t kAll = kEmitAll;
    NoCheckpoints nocp;
    TickSink ns;
    int overflow = 0, bad = 0, give_up = 0, huff_bad = 0;      // (huff_bad: an invalid code in a block of the picture -- the decode goes on, as on the device)
    long merge_ticks = 0, prefix_ticks = 0, prefix_lanes = 0, rounds = 0;
    // ---- k_huff_emit
    for (uint32_t s = 0; s < nsub; s++) {
        SubseqState e = make_state(0, 0, 0);
        if (s > 0) {
            const uint32_t from = s * L - W;
            e = W ? decode_subseq<false, 0>(bits, plan.lut.data(), img, make_state(from, 0, 0), s * L, 0, ns, nocp, from, make_state(0, 0, 0))
                  : make_state(s * L, 0, 0);
            e.n = e.m = 0;
        }
        EmitSink sink{region, s, rows, H, Hb, 0u, H, cap, 0xffffffffu, &overflow};
        sink.sub_start = s * L;
        sink.tail_start = emit_tail_start(img.total_bits, s * L);
        sink.tail_cp = emit_tail_cp(sink.tail_start, CPB);
        HostCps hc{g_cps.data() + size_t(s) * kMaxCp * 2};
        const SubseqState x = decode_subseq<true, 1>(bits, plan.lut.data(), imgw, e, end_of(s), 0, sink, hc, s * L, e);
        while (sink.eoff & 7u) {                                                   // null entries up to the group boundary
            if (sink.eoff >= sink.lowest_bword) { overflow = 1; break; }            // (they would land on block words: ImagePlan::emit_fits keeps such pictures off this path)
            region[stream_phys(s, sink.eoff++, rows)] = 0u;
        }
        g_entry[s] = make_state(e.p, e.z, e.c);
        g_exit[s] = x;
        d0n[s] = x.n; d0m[s] = x.m;
        badl[s] = sink.bad_label;
        badp[s] = sink.bad_pos - s * L;
        badq[s] = sink.bad_last;
        badql[s] = sink.bad_tail;
        badq2[s] = sink.bad_tail2;
        if (lanes && s < lanes_cap) {
            lanes[4 * s] = sink.bad_label == 0xffffffffu ? 0xffffffffu : badp[s];
            lanes[4 * s + 1] = 0;
            lanes[4 * s + 2] = sink.bad_tail != 0xffffffffu && sink.nbad ? (sink.bad_tail & 0xffffu) : sink.bad_last == 0xffffffffu ? 0xffffffffu : (sink.bad_last & 0xffffu);
            lanes[4 * s + 3] = sink.nbad;
        }
    }
    if (lanes && nsub < lanes_cap) { lanes[4 * nsub] = L; lanes[4 * nsub + 1] = nsub; lanes[4 * nsub + 2] = CPB; lanes[4 * nsub + 3] = W; }      // (a trailer: the cut)
    // ---- merge rounds (count only); the deepest merge point of a subsequence's re-decodes is kept
    for (;;) {
        long redone = 0;
        std::vector<SubseqState> snap;
        if (mode == 0) snap = g_exit;
        for (uint32_t s = 1; s < nsub; s++) {
            const SubseqState prev = mode == 0 ? snap[s - 1] : g_exit[s - 1];
            if (same_entry(prev, g_entry[s])) continue;
            const SubseqState e = make_state(prev.p, prev.z, prev.c);
            g_entry[s] = e;
            HostCps hc{g_cps.data() + size_t(s) * kMaxCp * 2};
            uint32_t depth = kAll;
            if (e.p > s * L + band_end(end_of(s) - s * L)) { g_exit[s] = make_state(e.p, e.z, e.c); }
            else {
                LaneState st; LaneEvents ev;
                lane_begin(st, bits, img2, e);
                events_begin<2>(ev, s * L, end_of(s), CPB);
                uint32_t blk = 0;
                const long t0 = ns.ticks;
                for (;;) {
                    const bool crossed = symbol_step<false, true>(st, bits, lut2, img2, blk, ns);
                    if (crossed && lane_event<2>(st, ev, img2, hc)) break;
                }
                merge_ticks += ns.ticks - t0;
                checkpoint_fixup(hc, ev.k, st.n, lane_m(st));
                if (ev.merged) depth = ev.k + 1;
                g_exit[s] = lane_exit(st, ev, img2, g_exit[s]);
            }
            kfix[s] = std::max(kfix[s], depth);
            redone++;
        }
        rounds++;
        if (redone == 0) break;
        if (rounds > long(nsub) + 1) { bad = 11; break; }          // (a round puts at least one more subsequence right: the device keeps repairing, mjx_batch_wait)
    }
    // ---- k_huff_scan: blocks completed before every subsequence
    std::vector<uint32_t> B(nsub + 1, 0);
    for (uint32_t s = 0; s < nsub; s++) B[s + 1] = B[s] + g_exit[s].n;
    const size_t nb = img.total_blocks;
    *nblocks = nb;
    // ---- k_huff_prefix: re-decode from the true entry up to the merge point, right-aligned against the first decode's valid part
    std::vector<uint32_t> gs(nsub, H / 8u), ge(nsub);
    std::vector<int32_t> lbl(nsub, 0);
    int64_t worst_e = 0, worst_b = 0;
    for (uint32_t s = 0; s < nsub; s++) {
        ge[s] = (H + d0m[s] + 7u) / 8u;
        if (!kfix[s]) continue;
        prefix_lanes++;
        uint32_t n0r = 0, m0r = 0, stop_bit = end_of(s);
        if (kfix[s] != kAll) {
            const uint32_t k = kfix[s] - 1;
            n0r = (g_cps[(size_t(s) * kMaxCp + k) * 2] >> 16) & 0x7fffu;
            m0r = g_cps[(size_t(s) * kMaxCp + k) * 2 + 1];
            stop_bit = s * L + (k + 1) * CPB;
        }
        const uint32_t n0K = d0n[s] - n0r, j0K = d0m[s] - m0r, n_p = g_exit[s].n - n0r, m_p = g_exit[s].m - m0r;
        worst_e = std::max<int64_t>(worst_e, int64_t(m_p) - int64_t(j0K));
        worst_b = std::max<int64_t>(worst_b, int64_t(n_p) - int64_t(n0K));
        if (int64_t(H) + j0K < int64_t(m_p) || int64_t(Hb) + n0K < int64_t(n_p)) { overflow = 1; continue; }
        const uint32_t off_e = H + j0K - m_p;
        lbl[s] = int32_t(n0K) - int32_t(n_p);
        EmitSink sink{region, s, rows, off_e, uint32_t(int32_t(Hb) + lbl[s]), uint32_t(lbl[s]), off_e, H + j0K, 0xffffffffu, &overflow};
        for (uint32_t i = off_e & ~7u; i < off_e; i++) region[stream_phys(s, i, rows)] = 0u;      // null entries in front of the run's first entry
        gs[s] = off_e >> 3;
        const SubseqState e = g_entry[s];
        if (e.p <= s * L + band_end(end_of(s) - s * L)) {
            LaneState st;
            lane_begin(st, bits, imgw, e);
            uint32_t blk = 0;
            const uint32_t stop_wn = wn_after(stop_bit);
            while (st.wn < stop_wn) (void)symbol_step<true, false>(st, bits, plan.lut.data(), imgw, blk, sink);
            prefix_ticks += sink.ticks;
            if (sink.eoff != H + j0K || st.n != n_p) bad = 12;                   // the counts of the merge rounds must be exact
            if (kfix[s] != kAll) {
                const uint32_t rec = g_cps[(size_t(s) * kMaxCp + kfix[s] - 1) * 2];
                if ((rec & kCpStateMask) != cp_state_word(st)) bad = 13;        // ... and the prefix must meet the first decode's path there
            }
            if (sink.bad_label != 0xffffffffu && B[s] + sink.bad_label < nb) huff_bad = 1;
        }
        if (lanes && s < lanes_cap) lanes[4 * s + 1] = 0xffffffffu;
        if (badl[s] != 0xffffffffu) {       // the first decode's invalid codes count if they lie at or behind the merge point (k_huff_prefix)
            if (kfix[s] == kAll) badl[s] = 0xffffffffu;
            else {
                const uint32_t rec = g_cps[(size_t(s) * kMaxCp + kfix[s] - 1) * 2];
                const uint32_t pK = 8u * (wn_after(kfix[s] * CPB) - 8u) - (rec & 31u);
                if (lanes && s < lanes_cap) lanes[4 * s + 1] = pK;
                if (badp[s] < pK) {
                    // the first one lies on the discarded part: the last one in front of the scan's tail, then the first one inside it (k_huff_prefix)
                    auto inside = [&](uint32_t w) { return int64_t(B[s]) + int64_t(w >> 16) - lbl[s] < int64_t(nb); };
                    const bool first_inside = int64_t(B[s]) + int64_t(badl[s]) - lbl[s] < int64_t(nb);
                    badl[s] = 0xffffffffu;
                    if (!first_inside) {
                        // (the first one's block is already behind the picture's last: so is every later one's)
                    } else if (badq[s] != 0xffffffffu && (badq[s] & 0xffffu) >= pK) {
                        if (inside(badq[s])) badl[s] = badq[s] >> 16;
                        else give_up = 16;                 // (the device hands the picture to the two-pass kernels: reason bit 256)
                    } else {
                        const uint32_t tw = pK > emit_tail_cp(emit_tail_start(img.total_bits, s * L), CPB) ? badq2[s] : badql[s];
                        if (tw != 0xffffffffu && (tw & 0xffffu) >= pK && inside(tw)) badl[s] = tw >> 16;
                    }
                }
            }
        }
    }
    for (uint32_t s = 0; s < nsub; s++) runs[s] = run_word(gs[s], ge[s], uint32_t(int32_t(B[s]) - lbl[s]) & 0xffu);
    if (overflow) bad = 14;                        // (the device hands the picture to the two-pass kernels: nothing else counts)
    else if (give_up && !bad) bad = give_up;       // (the same, for an invalid code k_huff_prefix cannot place: 16 -- the last one in front of the
                                                   // scan's tail lies behind the picture's last block, and the first one was discarded)
    for (uint32_t s = 0; s < nsub; s++)
        if (badl[s] != 0xffffffffu && int64_t(B[s]) + int64_t(badl[s]) - lbl[s] < int64_t(nb)) huff_bad = 1;
    // ---- k_block_gather + stage B's expansion (quad_prepare / quad_cell: the functions the kernel runs)
    const bool truncated = B[nsub] < nb;            // k_huff_scan: the picture is flagged and every later kernel skips it
    if (truncated && !bad) bad = 15;
    if (!bad && nb <= cap_blocks && B[nsub] >= nb) {
        const uint32_t tile_blocks = tile_mcus(plan.bpm, plan.hmax) * plan.bpm;
        const uint32_t ntiles = uint32_t((nb + tile_blocks - 1) / tile_blocks);
        std::vector<uint32_t> eoff(ntiles + 1, 0xffffffffu);
        std::vector<int16_t> dcb(nb, 0);
        for (uint32_t s = 0; s < nsub; s++) {
            const uint32_t fs = g_entry[s].z ? 1u : 0u, fs1 = s + 1 < nsub ? (g_entry[s + 1].z ? 1u : 0u) : (g_exit[s].z ? 1u : 0u);
            for (uint64_t a = uint64_t(B[s]) + fs; a < uint64_t(B[s + 1]) + fs1 && a <= nb; a++) {
                const uint32_t w = region[stream_phys(s, block_word_index(uint32_t(int64_t(Hb) + int64_t(a - B[s]) + lbl[s]), rows), rows)];
                if (a < nb) dcb[a] = int16_t(w & 0xffffu);
                if (a == nb) eoff[ntiles] = s * cap + (w >> 16);
                else if (a % tile_blocks == 0) eoff[a / tile_blocks] = s * cap + (w >> 16);
            }
            if (s == nsub - 1 && uint64_t(B[s + 1]) + fs1 <= nb) eoff[ntiles] = s * cap + H + d0m[s];
        }
        std::memset(out, 0, nb * 64 * sizeof(int16_t));
        for (uint32_t t = 0; t < ntiles && !bad; t++) {
            if (eoff[t] == 0xffffffffu || eoff[t + 1] == 0xffffffffu) { bad = 7; break; }
            const uint32_t sub[2] = {eoff[t] / cap, eoff[t + 1] / cap};
            const uint16_t at[2] = {uint16_t(eoff[t] % cap), uint16_t(eoff[t + 1] % cap)};
            QuadCum cum;
            QuadView q{sub, at, &cum, runs, rows, nsub};
            cum = quad_prepare(q, 0);
            QuadCell cell;
            const uint32_t total = quad_cell(q, 0, 0, cell);
            const uint32_t first_lo = (t * tile_blocks) & 0xffu;
            for (uint32_t o = 0; o < total && !bad; o++) {
                if (quad_cell(q, 0, o, cell) != total || cell.phys == 0xffffffffu) { bad = 8; break; }
                for (uint32_t k = cell.k_lo; k < cell.k_hi; k++) {
                    const uint32_t e = region[cell.phys + k];
                    if (((e >> 16) & 63) == 0) continue;                        // null entry
                    const uint32_t bi = ((e >> 22) - (first_lo - cell.label)) & 0xffu;      // (as scatter_batch)
                    const uint32_t blk = t * tile_blocks + bi;
                    if (bi >= tile_blocks || blk >= nb) { bad = 9; break; }
                    out[size_t(blk) * 64 + ((e >> 16) & 63)] = int16_t(e & 0xffff);
                }
            }
        }
        int32_t pred[4] = {0, 0, 0, 0};            // (a fourth component with MJX_COLOR_FILE)
        for (size_t b = 0; b < nb; b++) {
            const int c = plan.blk_comp[b % plan.bpm];
            pred[c] += dcb[b];
            out[b * 64] = int16_t(pred[c]);
        }
    }
    if (stats) {
        stats[0] = int(nsub); stats[1] = int(rounds); stats[2] = int(prefix_lanes); stats[3] = int(prefix_ticks);
        stats[4] = int(merge_ticks); stats[5] = int(worst_e); stats[6] = bad ? bad : huff_bad; stats[7] = int(worst_b);
    }
    mjx_free_scan(&d);
    if (nb > cap_blocks) return MJX_ERR_NOMEM;
    return truncated ? MJX_ERR_TRUNCATED : (bad || huff_bad) ? MJX_ERR_BAD_HUFFMAN : MJX_OK;      // (as mjx_batch_wait: truncated wins)
}
extern "C" int emul_single_decode_lanes(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                        unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */,
                                        uint32_t *lanes, size_t lanes_cap)
{
    return emul_single_decode_lanes_color(jpeg, len, layout, mode, sub_base_bits, warm_bits, headroom_groups, cp_bits, out, cap_blocks, nblocks, stats,
                                          lanes, lanes_cap, MJX_COLOR_POSITIONAL);
}
extern "C" int emul_single_decode_cp_color(const uint8_t *jpeg, size_t len, int layout, int mode, unsigned sub_base_bits, unsigned warm_bits,
                                           unsigned headroom_groups, unsigned cp_bits, int16_t *out, size_t cap_blocks, size_t *nblocks, int *stats /* [8] */,
                                           int color)
{
    return emul_single_decode_lanes_color(jpeg, len, layout, mode, sub_base_bits, warm_bits, headroom_groups, cp_bits, out, cap_blocks, nblocks, stats,
                                          nullptr, 0, color);
}

// ---- round 5: multi-scan pictures read without the gather, and what the planner decides per scan ------------------------------------
// The cuts of a scan's stream as k_huff_write records them (StreamSink::next_cut): the first cut at or after block 0, then always
// the first one behind the last.  Returns the number of cuts (mcu_out / slot_out hold the first `cap`).
extern "C" int emul_planar_cuts(unsigned scan_mcux, unsigned scan_mcuy, unsigned T, unsigned pic_mcux, unsigned hs, unsigned vs,
                                unsigned *mcu_out, unsigned *slot_out, int cap)
{
    const uint32_t S = planar_row_slots(pic_mcux, T), nmcu = scan_mcux * scan_mcuy;
    int n = 0;
    for (uint32_t q = 0; q < nmcu;) {
        const PlanarCut c = planar_cut(q, scan_mcux, S, T, pic_mcux, hs, vs);
        if (c.mcu >= nmcu) break;
        if (n < cap) { mcu_out[n] = c.mcu; slot_out[n] = c.slot; }
        n++;
        q = c.mcu + 1;
    }
    return n;
}
// plan_input on a file: per plan {role, part_idx, ncomp, bpm, himg.bpm (the decoder's block-in-MCU period), sub_bits, nsub, status}
extern "C" int emul_plan_parts_color(const uint8_t *jpeg, size_t len, int *out /* [cap][8] */, int cap, int color)
{
    mjx_opts opts{};
    MJX_OPTS_COLOR(&opts) = uint8_t(color);
    mjx_scan_desc d;
    const int rc = mjx_parse(jpeg, len, &opts, &d);
    if (rc) return -rc;
    std::vector<ImagePlan> plans;
    plan_input(d, opts, plans);
    int n = 0;
    for (const ImagePlan &p : plans) {
        if (n < cap) {
            int *o = out + 8 * n;
            o[0] = int(p.role); o[1] = int(p.part_idx); o[2] = int(p.ncomp); o[3] = int(p.bpm); o[4] = int(p.himg.bpm);
            o[5] = int(p.himg.sub_bits); o[6] = int(p.himg.nsub); o[7] = p.status;
        }
        n++;
    }
    mjx_free_scan(&d);
    return n;
}
extern "C" int emul_plan_parts(const uint8_t *jpeg, size_t len, int *out /* [cap][8] */, int cap)
{
    return emul_plan_parts_color(jpeg, len, out, cap, MJX_COLOR_POSITIONAL);
}
// stage_b_choice on n plans that hold nothing but its inputs: rows of {lj, ycc_on, out_on, rs_on, out_channels, cropped, scale, layout,
// sampling is 4:2:0, role, orient, or_copy} -> rows of {mode, rs_on, or_on, out_ch, lj_on, lj_luma, lj_out, tile_420}
extern "C" void emul_stage_b_choice(const uint32_t *in /* [n][12] */, int n, uint8_t *out /* [n][8] */)
{
    for (int i = 0; i < n; i++, in += 12, out += 8) {
        ImagePlan p;
        p.lj = in[0] != 0; p.ycc_on = in[1] != 0; p.out_on = in[2] != 0; p.rs_on = in[3] != 0; p.out_channels = in[4];
        p.cropped = in[5] != 0; p.scale = in[6]; p.layout = in[7]; p.role = in[9]; p.orient = in[10]; p.or_copy = in[11] != 0;
        p.ncomp = 3;
        if (in[8]) p.h[0] = p.v[0] = p.hmax = p.vmax = 2;
        const StageBChoice c = stage_b_choice(p);
        const uint32_t o[8] = {c.mode, c.rs_on, c.or_on, c.out_ch, c.lj_on, c.lj_luma, c.lj_out, c.tile_420 ? 1u : 0u};
        for (int k = 0; k < 8; k++) out[k] = uint8_t(o[k]);
    }
}
// the modes of the entries of MJX_STAGE_B_KERNELS (mjx_kernels.h), in the list's order; returns their count
extern "C" int emul_stage_b_kernel_modes(uint32_t *out, int cap)
{
    int n = 0;
#define EMUL_MODE(F, S, PF, SRC, LAYOUT, DENSITY) if (n < cap) out[n] = stage_b_mode(F, S); n++;
    MJX_STAGE_B_KERNELS(EMUL_MODE)
#undef EMUL_MODE
    return n;
}

// ---- decode tables as the host builds them (tests/test_huffman_tables.py walks them over every 16-bit window) ------------------------
// build_decode_table on one DHT table (vals: 256 bytes) -> entries written, or the negative status
extern "C" int emul_build_table(const uint8_t *bits, const uint8_t *vals, int is_dc, int pair, uint32_t *out, int cap)
{
    return build_decode_table(bits, vals, is_dc != 0, out, cap, pair != 0);
}
// plan_image on a file: out = {entries of the plain table set, entries of the set with pair parts, blocks per MCU, BlockTab::tabs per
// block of the MCU [12], ImagePlan::emit_fits}; returns the plan's status
// (with mjx_opts.color = `color`; the status of a file the parser or the planner refuses comes back as it is)
extern "C" int emul_table_set_color(const uint8_t *jpeg, size_t len, uint32_t *out /* [16] */, int color)
{
    mjx_opts opts{};
    MJX_OPTS_COLOR(&opts) = uint8_t(color);
    mjx_scan_desc d;
    int rc = mjx_parse(jpeg, len, &opts, &d);
    if (rc) return rc;
    ImagePlan plan;
    rc = plan_image(d, opts, plan);
    if (rc == 0) {
        out[0] = plan.lut_plain_n;
        out[1] = uint32_t(plan.lut.size()) - plan.lut_plain_n;
        out[2] = plan.bpm;
        for (uint32_t b = 0; b < uint32_t(kMaxBlocksPerMcu); b++) out[3 + b] = b < plan.bpm ? plan.himg.btab[b].tabs : 0u;
        out[15] = plan.emit_fits ? 1u : 0u;
    }
    mjx_free_scan(&d);
    return rc;
}
extern "C" int emul_table_set(const uint8_t *jpeg, size_t len, uint32_t *out /* [16] */)
{
    return emul_table_set_color(jpeg, len, out, MJX_COLOR_POSITIONAL);
}

// ---- device-side de-stuffing and marker scan (tests/test_destuff_boundaries.py) ------------------------------------------------------
// What k_destuff_count, k_destuff_prefix and k_destuff_scatter do, serially, with the kernels' own rule per 64-byte piece
// (destuff_keep_mask, mjx_kernels.h): per 16 KiB workgroup the bytes kept and the markers found -> seg_counts[2 g], [2 g + 1];
// exclusive sums of both; then every piece's kept bytes at workgroup base + offset inside the workgroup, and the offsets of its
// markers into the list.  The input is copied into a buffer laid out as build_batch lays out the raw staging buffer -- 64-byte
// aligned, 64 bytes of padding behind the length rounded up to 64, here filled with `pad` -- and not one byte longer, so that a
// read the rule should not make is one AddressSanitizer sees.  Returns the de-stuffed length (-1: out_cap or rst_cap too small);
// *n_rst: markers found.
namespace {
struct Word4 { uint32_t x, y, z, w; };          // the piece loads of the kernels are uint4
}
extern "C" long emul_destuff(const uint8_t *raw, size_t len, int restarts, int pad, uint8_t *out, size_t out_cap,
                             uint32_t *rst_off, size_t rst_cap, uint32_t *seg_counts, uint32_t *n_rst)
{
    const size_t room = ((len + 63) & ~size_t(63)) + 64;
    std::vector<Word4> store(room / sizeof(Word4));
    uint8_t *buf = reinterpret_cast<uint8_t *>(store.data());
    std::memset(buf, pad, room);
    if (len) std::memcpy(buf, raw, len);
    const uint32_t nseg = uint32_t((len + kDestuffSeg - 1) / kDestuffSeg), lanes = uint32_t(kDestuffSeg / 64);
    std::vector<uint32_t> cnt(size_t(nseg) * 2), base(size_t(nseg) * 2);
    for (uint32_t g = 0; g < nseg; g++)                                      // k_destuff_count
        for (uint32_t t = 0; t < lanes; t++) {
            uint64_t mask, rst;
            Word4 q[4];
            cnt[2 * g] += destuff_keep_mask(buf, uint64_t(g) * kDestuffSeg + t * 64ull, len, q, &mask, restarts != 0, &rst);
            cnt[2 * g + 1] += mjx_popcount64(rst);
        }
    uint32_t run = 0, run_rst = 0;
    for (uint32_t g = 0; g < nseg; g++) {                                    // k_destuff_prefix
        base[2 * g] = run;
        base[2 * g + 1] = run_rst;
        run += cnt[2 * g];
        run_rst += cnt[2 * g + 1];
        if (seg_counts) { seg_counts[2 * g] = cnt[2 * g]; seg_counts[2 * g + 1] = cnt[2 * g + 1]; }
    }
    if (n_rst) *n_rst = run_rst;
    if (run > out_cap || run_rst > rst_cap) return -1;
    for (uint32_t g = 0; g < nseg; g++) {                                    // k_destuff_scatter
        uint32_t o = 0, r = base[2 * g + 1];
        for (uint32_t t = 0; t < lanes; t++) {
            uint64_t mask, rst;
            Word4 q[4];
            (void)destuff_keep_mask(buf, uint64_t(g) * kDestuffSeg + t * 64ull, len, q, &mask, restarts != 0, &rst);
            for (uint64_t m = rst; m; m &= m - 1) {
                const uint32_t j = uint32_t(__builtin_ctzll(m));
                rst_off[r++] = base[2 * g] + o + mjx_popcount64(mask & ((1ull << j) - 1ull));
            }
            for (int k = 0; k < 4; k++) {
                const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
                for (int j = 0; j < 16; j++)
                    if ((mask >> (k * 16 + j)) & 1) out[base[2 * g] + o++] = uint8_t(w[j >> 2] >> ((j & 3) * 8));
            }
        }
        if (o != cnt[2 * g] || r != base[2 * g + 1] + cnt[2 * g + 1]) return -2;          // (the two kernels must count alike)
    }
    return long(run);
}

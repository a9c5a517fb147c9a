// mjx_prog.h -- progressive JPEG (SOF2, T.81 Annex G): the per-lane scan decode and the rule that turns the dense coefficient
// store into the stream stage B reads.  Shared by the HIP kernels (k_prog_scan, k_prog_count / _copy) and the host
// (tests/emul/prog_emul.cpp, tests/prog_fuzz.cpp): the host runs the identical code.
//
// One lane decodes one restart interval of one scan, serially, with the semantics of T.81 G.2 / libjpeg's jdphuff.c:
//   DC first   running prediction per interval, value << Al, stored absolute
//   DC refine  one bit per block
//   AC first   EOBn runs up to 32767, ZRL
//   AC refine  correction bits for every already non-zero coefficient passed over, +-(1 << Al) for new ones; runs count only
//              zero-history coefficients; correction bits are also consumed inside EOB runs
// into a dense store: per picture one plane of 64-coefficient blocks (int16, zig-zag order) per component, each in the component's own
// raster over the MCU-padded block grid.  A non-interleaved scan visits the component's unpadded grid, an interleaved DC scan MCU
// order, padding blocks included.
// Safety: every load is bounded by the interval's end (bits behind it read as zero and set kProgShort, and the lane stops there);
// every store is index-checked against the component's plane; an end-of-band run longer than the blocks left is cut and flagged;
// every loop runs over the lane's blocks or over the 64 coefficients of one, so the work is bounded whatever the bytes say.
#ifndef MJX_PROG_H
#define MJX_PROG_H

#include "mjx_huff.h"

namespace mjx {

// flags a lane ORs into its picture's word of img_flags
constexpr uint32_t kProgShort = 1u;     // out of bits before the interval's blocks were complete: MJX_ERR_TRUNCATED (wins)
constexpr uint32_t kProgBad = 4u;       // no matching code, a coefficient index past Se, an over-long end-of-band run: MJX_ERR_BAD_HUFFMAN

// T.81 G.1.1.1 and libjpeg's coef_bits rule for one scan of `n` components (indices into the frame's `ncomp`) against what the scans
// in front of it sent: bits[c][k] is the Al of the last scan that carried coefficient k of component c, -1 when none has (the caller
// starts from all -1).  true: the scan is allowed, and bits is updated.  mjx_parse and the planner (mjx_validate) both ask here.
inline bool prog_scan_ok(int8_t bits[3][64], uint32_t ncomp, uint32_t n, const uint8_t *comp, uint32_t ss, uint32_t se, uint32_t ah, uint32_t al)
{
    if (n < 1 || n > 3 || n > ncomp || ss > se || se > 63 || al > 13 || ah > 14) return false;
    if (ss == 0 ? se != 0 : n != 1) return false;            // a DC scan is DC alone and may interleave; an AC scan has one component
    for (uint32_t q = 0; q < n; q++) {
        if (comp[q] >= ncomp) return false;
        for (uint32_t e = 0; e < q; e++) if (comp[e] == comp[q]) return false;
        if (ss != 0 && bits[comp[q]][0] < 0) return false;   // an AC scan needs the component's first DC scan in front of it
        for (uint32_t k = ss; k <= se; k++) {
            const int prev = bits[comp[q]][k];
            if (prev < 0 ? ah != 0 : (ah != uint32_t(prev) || al + 1 != ah)) return false;
        }
    }
    for (uint32_t q = 0; q < n; q++)
        for (uint32_t k = ss; k <= se; k++) bits[comp[q]][k] = int8_t(al);
    return true;
}

// A progressive picture as its lanes and the compaction see it
struct ProgPic {
    uint64_t plane[3];          // first coefficient of component c's plane in the chunk's store (int16 elements)
    uint32_t pbw[3], pbh[3];    // the padded block grid: mcux * h, mcuy * v
    uint32_t cbw[3], cbh[3];    // the component's own grid: ceil(W h / (8 hmax)) x ceil(H v / (8 vmax))
    uint32_t h[3], v[3];
    uint32_t mcux, mcuy, ncomp, pad_;
};

// One lane: a restart interval of a scan
struct ProgLane {
    uint64_t byte_off;          // the interval's first byte in the pool of progressive scans
    uint32_t nbytes;            // its length
    uint32_t first, count;      // units of the interval: MCUs of an interleaved scan, else blocks of the component's own raster
    uint32_t img;               // the picture: index inside the chunk
    uint32_t pic;               // its ProgPic
    uint32_t tab[3];            // decode tables, entries from the picture's first table: DC tables per scan component, or the AC table in [0]
    uint8_t ss, se, ah, al;
    uint8_t ncomp, comp[3];
};

struct ProgBits {
    const uint8_t *p;
    uint32_t nbytes, pos;       // pos: next byte to load
    uint32_t have;              // valid bits at the top of acc
    uint64_t acc;
    uint64_t used;              // bits consumed
};
MJX_HD void prog_bits_begin(ProgBits &b, const uint8_t *p, uint32_t nbytes)
{
    b.p = p; b.nbytes = nbytes; b.pos = 0; b.have = 0; b.acc = 0; b.used = 0;
}
MJX_HD void prog_fill(ProgBits &b)                         // at least 57 bits in acc; bytes behind the interval's end read as zero
{
    while (b.have <= 56u) {
        const uint32_t v = b.pos < b.nbytes ? b.p[b.pos] : 0u;
        b.pos++;
        b.acc |= uint64_t(v) << (56u - b.have);
        b.have += 8u;
    }
}
MJX_HD void prog_skip(ProgBits &b, uint32_t n) { b.acc <<= n; b.have -= n; b.used += n; }
MJX_HD uint32_t prog_receive(ProgBits &b, uint32_t n)      // n <= 16
{
    if (!n) return 0u;
    prog_fill(b);
    const uint32_t v = uint32_t(b.acc >> (64u - n));
    prog_skip(b, n);
    return v;
}
MJX_HD bool prog_short(const ProgBits &b) { return b.used > uint64_t(b.nbytes) * 8u; }
MJX_HD int32_t prog_extend(uint32_t v, uint32_t s) { return s && v < (1u << (s - 1u)) ? int32_t(v) - int32_t((1u << s) - 1u) : int32_t(v); }

// One Huffman symbol from a table of build_decode_table's (mjx_lut.cpp), read where it lies.  Returns the direct entry: size = (e >> 11)
// & 15, zinc = (e >> 16) & 127 (run + 1; 64: symbol 0x00).  A pattern no code matches takes one bit, sets kProgBad and returns kLutBad.
MJX_HD LutEntry prog_symbol(ProgBits &b, const LutEntry *tab, uint32_t &flags)
{
    prog_fill(b);
    const uint32_t w = uint32_t(b.acc >> 32);
    LutEntry e = tab[w >> (32 - kLutPrimaryBits)];
    if (lut_is_link(e)) {
        const uint32_t nb = e & 15u;
        const uint32_t idx = nb ? (w << kLutPrimaryBits) >> (32u - nb) : 0u;
        e = tab[lut_link_offset(e) + idx];
    }
    if (e & kLutBad) {
        flags |= kProgBad;
        prog_skip(b, 1u);
        return kLutBad;
    }
    prog_skip(b, (e & 31u) - ((e >> 11) & 15u));
    return e;
}

// correction bit of an already non-zero coefficient (jdphuff.c decode_mcu_AC_refine)
MJX_HD void prog_correct(ProgBits &b, int16_t *c, int32_t p1)
{
    const int32_t v = *c;
    if (prog_receive(b, 1u) && (v & p1) == 0) *c = int16_t(v >= 0 ? v + p1 : v - p1);
}

// One block of an AC scan.  `blk`: its 64 coefficients, or null when the block's index lies outside the plane (nothing is stored,
// the bits are consumed as if every coefficient were zero).
MJX_HD void prog_ac_block(ProgBits &b, const ProgLane &ln, const LutEntry *tab, int16_t *blk, uint32_t &eobrun, uint32_t &flags)
{
    const uint32_t ss = ln.ss, se = ln.se, al = ln.al;
    uint32_t k = ss;
    if (ln.ah == 0) {                                       // first pass (decode_mcu_AC_first)
        if (eobrun) { eobrun--; return; }
        while (k <= se) {
            const LutEntry e = prog_symbol(b, tab, flags);
            if (e == kLutBad) { k++; continue; }            // (one bit taken; stands for run 0, size 0 -- the next coefficient)
            const uint32_t zinc = (e >> 16) & 127u, s = (e >> 11) & 15u, r = zinc == 64u ? 0u : zinc - 1u;
            if (s) {
                k += r;
                const int32_t v = prog_extend(prog_receive(b, s), s);
                if (k > se) { flags |= kProgBad; return; }
                if (blk) blk[k] = int16_t(uint32_t(v) << al);
                k++;
            } else if (r == 15u) {
                k += 16u;
            } else {                                        // EOBr: this block and 2^r + extra - 1 more
                eobrun = (1u << r) + prog_receive(b, r) - 1u;
                return;
            }
        }
        return;
    }
    const int32_t p1 = int32_t(1u << al);                   // refinement (decode_mcu_AC_refine)
    if (!eobrun) {
        while (k <= se) {
            const LutEntry e = prog_symbol(b, tab, flags);
            if (e == kLutBad) { k++; continue; }
            const uint32_t zinc = (e >> 16) & 127u, size = (e >> 11) & 15u;
            int32_t r = zinc == 64u ? 0 : int32_t(zinc) - 1;
            int32_t s = 0;
            if (size) {
                if (size != 1u) flags |= kProgBad;          // (libjpeg warns and goes on as if the size were 1)
                s = prog_receive(b, 1u) ? p1 : -p1;
            } else if (r != 15) {
                eobrun = (1u << r) + prog_receive(b, uint32_t(r));
                break;
            }
            // over the coefficients that already have a history (a correction bit each) and r of those that do not
            while (k <= se) {
                if (blk && blk[k] != 0) prog_correct(b, blk + k, p1);
                else if (--r < 0) break;
                k++;
            }
            if (s) {
                if (k > se) { flags |= kProgBad; return; }
                if (blk) blk[k] = int16_t(s);
            }
            k++;
        }
    }
    if (eobrun) {                                           // inside an end-of-band run: correction bits only
        for (; k <= se; k++)
            if (blk && blk[k] != 0) prog_correct(b, blk + k, p1);
        eobrun--;
    }
}

// The lane.  `pic`: the lane's picture; `store`: the chunk's dense store; `lut`: the picture's first decode table.  Returns the flags.
MJX_HD uint32_t prog_lane(const ProgLane &ln, const ProgPic &pic, const uint8_t *bytes, const LutEntry *lut, int16_t *store)
{
    ProgBits b;
    prog_bits_begin(b, bytes + ln.byte_off, ln.nbytes);
    uint32_t flags = 0, eobrun = 0;
    if (ln.ncomp < 1u || ln.ncomp > 3u || ln.se > 63u || ln.ss > ln.se || ln.al > 13u) return kProgBad;
    if (ln.ss == 0u) {                                      // DC scan: interleaved (MCU order, padding included) or one component's own raster
        uint32_t pred0 = 0, pred1 = 0, pred2 = 0;
        for (uint32_t u = 0; u < ln.count; u++) {
            const uint32_t unit = ln.first + u;
            for (uint32_t q = 0; q < ln.ncomp; q++) {
                const uint32_t c = ln.comp[q];
                if (c >= pic.ncomp) return flags | kProgBad;
                const uint32_t hh = ln.ncomp == 1u ? 1u : pic.h[c], vv = ln.ncomp == 1u ? 1u : pic.v[c];
                const uint32_t gw = ln.ncomp == 1u ? pic.cbw[c] : pic.mcux;
                const uint32_t ux = unit % gw, uy = unit / gw;
                for (uint32_t j = 0; j < hh * vv; j++) {
                    const uint32_t bx = ux * hh + j % hh, by = uy * vv + j / hh;
                    const bool inside = bx < pic.pbw[c] && by < pic.pbh[c];
                    int16_t *blk = inside ? store + pic.plane[c] + (uint64_t(by) * pic.pbw[c] + bx) * 64u : nullptr;
                    if (ln.ah == 0) {
                        const LutEntry e = prog_symbol(b, lut + ln.tab[q], flags);
                        const uint32_t s = e == kLutBad ? 0u : (e >> 11) & 15u;
                        const uint32_t diff = uint32_t(prog_extend(prog_receive(b, s), s));
                        uint32_t pred = q == 0 ? pred0 : q == 1 ? pred1 : pred2;
                        pred += diff;
                        if (q == 0) pred0 = pred; else if (q == 1) pred1 = pred; else pred2 = pred;
                        if (blk) blk[0] = int16_t(pred << ln.al);
                    } else if (prog_receive(b, 1u) && blk) {
                        blk[0] = int16_t(blk[0] | int16_t(1u << ln.al));
                    }
                    if (prog_short(b)) return flags | kProgShort;
                }
            }
        }
        return flags;
    }
    const uint32_t c = ln.comp[0];
    if (ln.ncomp != 1u || c >= pic.ncomp) return kProgBad;
    for (uint32_t u = 0; u < ln.count; u++) {
        const uint32_t unit = ln.first + u, bx = unit % pic.cbw[c], by = unit / pic.cbw[c];
        const bool inside = bx < pic.pbw[c] && by < pic.pbh[c];
        int16_t *blk = inside ? store + pic.plane[c] + (uint64_t(by) * pic.pbw[c] + bx) * 64u : nullptr;
        prog_ac_block(b, ln, lut + ln.tab[0], blk, eobrun, flags);
        if (prog_short(b)) return flags | kProgShort;
    }
    if (eobrun) flags |= kProgBad;                          // the run reaches past the interval's last block: cut here
    return flags;
}

// ---- dense store -> the stream stage B reads ----------------------------------------------------------------------------
// Block slot `slot` of MCU m of the picture (blk_comp / blk_bx / blk_by of the slot given): where its block lies in the store, and
// whether it is a real block of the component's own grid (a padding slot gives zeros).
struct ProgSlot { uint64_t at; bool real; };
MJX_HD ProgSlot prog_slot(const ProgPic &pic, uint32_t m, uint32_t c, uint32_t sbx, uint32_t sby)
{
    const uint32_t bx = (m % pic.mcux) * pic.h[c] + sbx, by = (m / pic.mcux) * pic.v[c] + sby;
    ProgSlot s;
    s.real = bx < pic.cbw[c] && by < pic.cbh[c];
    s.at = pic.plane[c] + (uint64_t(by) * pic.pbw[c] + bx) * 64u;
    return s;
}
// non-zero AC coefficients of a block, eight coefficients (16 bytes) at a time
struct alignas(16) ProgOct { uint32_t w0, w1, w2, w3; };   // (two coefficients per word, the even one in the low half)
MJX_HD uint32_t prog_pair_count(uint32_t w, bool low) { return ((w >> 16) ? 1u : 0u) + (low && (w & 0xffffu) ? 1u : 0u); }
MJX_HD uint32_t prog_block_count(const int16_t *blk)
{
    uint32_t n = 0;
    for (uint32_t g = 0; g < 8u; g++) {
        const ProgOct o = *reinterpret_cast<const ProgOct *>(blk + 8u * g);
        n += prog_pair_count(o.w0, g != 0u) + prog_pair_count(o.w1, true) + prog_pair_count(o.w2, true) + prog_pair_count(o.w3, true);
    }
    return n;
}
// ... and its entries, ascending position, label `slot` (coef_entry).  Returns the number written.
MJX_HD uint32_t prog_pair_emit(uint32_t w, uint32_t pos, bool low, uint32_t slot, uint32_t *dst, uint32_t n)
{
    if (low && (w & 0xffffu)) dst[n++] = coef_entry(int(int16_t(w & 0xffffu)), pos, slot);
    if (w >> 16) dst[n++] = coef_entry(int(int16_t(w >> 16)), pos + 1u, slot);
    return n;
}
MJX_HD uint32_t prog_block_emit(const int16_t *blk, uint32_t slot, uint32_t *dst)
{
    uint32_t n = 0;
    for (uint32_t g = 0; g < 8u; g++) {
        const ProgOct o = *reinterpret_cast<const ProgOct *>(blk + 8u * g);
        n = prog_pair_emit(o.w0, 8u * g, g != 0u, slot, dst, n);
        n = prog_pair_emit(o.w1, 8u * g + 2u, true, slot, dst, n);
        n = prog_pair_emit(o.w2, 8u * g + 4u, true, slot, dst, n);
        n = prog_pair_emit(o.w3, 8u * g + 6u, true, slot, dst, n);
    }
    return n;
}

}   // namespace mjx
#endif

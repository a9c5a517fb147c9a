// mjx_plan.cpp -- see mjx_plan.h.
#include "mjx_plan.h"
#include "mjx_prog.h"
#include "mjx_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mjx {

const uint8_t kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

bool ref_get_indices(long x, long y, long max_x, long x_factor, long y_factor, long max_x_factor, long max_y_factor,
                     long *ox, long *oy)
{
    if (max_y_factor > 1 && y_factor == 1) {
        if (max_x_factor > 1 && x_factor == 1) {                 // decoder.rs:262-278, fitted to nbx = 94
            if ((y & 1) == 0) {
                if (((x / 2) & 1) == 1) { *ox = x / 2 - 1 + (x & 1); *oy = y + 1; }
                else { *ox = x / 2 + (x & 1); *oy = y; }
                return true;
            }
            if (y > 0 && ((x / 2) & 1) == 0) {
                if (max_x / 2 + x / 2 < 1) return false;
                *ox = max_x / 2 + x / 2 - 1 + (x & 1); *oy = y;
                return true;
            }
            if (y < 1) return false;
            *ox = max_x / 2 + x / 2 + (x & 1); *oy = y - 1;
            return true;
        }
        if ((y & 1) == 0) { *ox = x / 2; *oy = y + (x & 1); return true; }      // decoder.rs:279-285
        if (y < (x & 1)) return false;
        *ox = x / 2 + max_x / 2; *oy = y - (x & 1);
        return true;
    }
    *ox = x; *oy = y;                                            // decoder.rs:287
    return true;
}

// REF_COMPAT: geometry of decoder.rs:239-312 and the inputs on which that code panics: a block index
// past the component's blocks (:303), usize underflow in get_indices, or a store index past the plane where the
// guard `i + j*stride < len` (:370) disagrees with the index `i + j*stride*8` (:371).
static int plan_ref_layout(ImagePlan &p)
{
    const size_t W = p.width, H = p.height, len = W * H;
    p.nbx = (p.width + 7) / 8;
    p.nby = (p.height + 7) / 8;
    for (uint32_t c = 0; c < p.ncomp; c++) {
        const float x_i = std::ceil(float(p.width) * (float(p.h[c]) / float(p.hmax)));      // decoder.rs:239-246
        const float y_i = std::ceil(float(p.height) * (float(p.v[c]) / float(p.vmax)));
        const float xf = std::ceil(float(p.width) / x_i), yf = std::ceil(float(p.height) / y_i);
        if (!(xf >= 1.0f) || !(yf >= 1.0f)) return MJX_ERR_REF_PANIC;                       // division by zero at :290
        const size_t xs = size_t(xf), ys = size_t(yf);
        p.ref_xf[c] = uint32_t(xs);
        p.ref_yf[c] = uint32_t(ys);
        const size_t cols = p.nbx / xs, rows = p.nby / ys;
        const size_t nblk = size_t(p.nmcu) * p.h[c] * p.v[c];
        if (cols * rows > nblk) return MJX_ERR_REF_PANIC;                                   // component_blocks[block_i]
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < cols; x++) {
                long bx, by;
                if (!ref_get_indices(long(x), long(y), long(p.nbx), long(xs), long(ys), long(p.hmax), long(p.vmax), &bx, &by))
                    return MJX_ERR_REF_PANIC;
                const size_t start_x = size_t(bx) * 8 * xs;
                if (W < start_x) continue;                                                  // :360 skips the line
                for (size_t line = 0; line < 8; line++) {
                    const size_t a = size_t(by) * 8 * ys * W + line * W + start_x, b = a + 8 * xs - 1;   // i range
                    for (size_t j = 1; j < ys; j++) {
                        // guard passes (i < len - jW) while the index i + 8jW is out of range (i >= len - 8jW)
                        const size_t lo = len > 8 * j * W ? len - 8 * j * W : 0, hi = len > j * W ? len - j * W : 0;
                        if (hi == 0) continue;
                        if (std::max(a, lo) <= std::min(b, hi - 1)) return MJX_ERR_REF_PANIC;
                    }
                }
            }
    }
    return MJX_OK;
}

// Cuts the scan of a planned picture into subsequences of about `base_bits` bits: p.seg holds the first bit of every
// segment (one segment without restart intervals); sets himg.sub_bits, himg.nsub and the first subsequence of every segment.
// (MJX_LONG_FIT=0: scans below kLongScanBits never take the long subsequences, as before round 6 -- for the A/B)
static bool long_fit_enabled()
{
    static const bool on = [] { const char *e = std::getenv("MJX_LONG_FIT"); return !e || std::atoi(e) != 0; }();
    return on;
}

void replan_subsequences(ImagePlan &p, uint32_t base_bits, bool allow_long)
{
    p.wg_lanes = uint32_t(kHuffWg);
    if (p.role == 2 || p.seg.size() < 2 * (size_t(p.nseg) + 1)) return;        // (role 2: no scan of its own)
    // long scans without restart intervals: long subsequences (mjx_huff.h: kLongSubseqBits), unless the caller asks for short ones
    uint32_t long_lanes = 0, long_bits = 0;
    if (allow_long && base_bits == uint32_t(kSubseqBits) && p.nseg == 1 && p.restart_mcus == 0 && (long long)p.himg.total_bits >= kLongScanBits)
        base_bits = uint32_t(kLongSubseqBits);
    else if (allow_long && base_bits == uint32_t(kSubseqBits) && p.role == 0 && p.nseg == 1 && p.restart_mcus == 0 && !p.stuffed && long_fit_enabled()) {
        // Round 6 (BASELINE config 4): a shorter scan whose long subsequences fill ONE workgroup of 256 lanes to seven
        // eighths takes them as well -- a 1080p scan of 0.24 MB is 238 of them in a 256-lane workgroup -- and with them the single decode (k_huff_emit runs at the chunk's workgroup size since this round; at
        // 512 lanes a 1080p picture held half an idle workgroup's LDS, which is why the long cut used to lose 13 % there).
        // (the length may stretch to 5/4 of the long one, as choose_subseq_bits stretches it to save a workgroup)
        // (256 lanes and up: what smaller scans do was settled on batches of small pictures in round 5 and is left alone)
        // ... and 256 lanes only: measured (tools/ab.sh -e MJX_LONG_FIT=0 -e MJX_LONG_FIT=1, same box) 4096 x 1080p 14.36 / 14.32 -> 13.84 / 14.08 ms per
        // step (592 -> 608 Gpixels/s); a 4K scan at quality 50 in ONE 512-lane workgroup of 500 long subsequences loses to its two passes
        // over 1000 short ones (21.5 -> 23.5 ms per 2048 pictures: k_huff_emit 10.5 ms against 2.0 + 5.6), so 512 lanes keep the old rule
        for (uint32_t lanes = 256u; lanes <= 256u && !long_lanes; lanes *= 2u) {
            const uint32_t fit = std::max<uint32_t>(uint32_t(kLongSubseqBits), ((p.himg.total_bits + lanes - 1) / lanes + uint32_t(kCpBits) - 1) / uint32_t(kCpBits) * uint32_t(kCpBits));
            if (fit <= uint32_t(kMaxSubseqBits) && uint64_t(p.himg.total_bits) * 8u >= uint64_t(lanes) * uint32_t(kLongSubseqBits) * 7u) { long_lanes = lanes; long_bits = fit; }
        }
        if (long_lanes) base_bits = uint32_t(kLongSubseqBits);
    }
    if (p.stuffed) {
        // the exact length and the restart offsets are only known on the device: an upper bound of the subsequence count
        // (every segment adds less than one to total / sub_bits) for the host's sizing, the subsequence length itself is final
        base_bits = std::max<uint32_t>(uint32_t(kCpBits), std::min<uint32_t>(base_bits, uint32_t(kLongSubseqBits)) / uint32_t(kCpBits) * uint32_t(kCpBits));
        p.himg.sub_bits = p.nseg == 1 ? choose_subseq_bits(p.himg.total_bits, base_bits) : base_bits;
        p.himg.nsub = (p.himg.total_bits + p.himg.sub_bits - 1) / p.himg.sub_bits + (p.nseg > 1 ? p.nseg : 0u);
        for (uint32_t g = 0; g <= p.nseg; g++) { p.seg[2 * size_t(g)] = g == p.nseg ? p.himg.nsub : 0u; p.seg[2 * size_t(g) + 1] = g == p.nseg ? p.himg.total_bits : 0u; }
        return;
    }
    base_bits = std::max<uint32_t>(uint32_t(kCpBits), std::min<uint32_t>(base_bits, uint32_t(kLongSubseqBits)) / uint32_t(kCpBits) * uint32_t(kCpBits));
    // A scan that does not fill one workgroup at the default length is cut shorter, so that it does: the workgroup holds its LDS for
    // as long as its longest lane decodes, whatever the number of lanes at work (the chroma scans of a three-scan 4K file: 272 and 219
    // subsequences of 4096 bits -- half a workgroup idle for the whole pass; round 5).
    // (MJX_FIT_SHORT=0: off, for the A/B; a value above 1: the shortest cut in bits instead of 1024)
    static const uint32_t fit_floor = [] { const char *e = std::getenv("MJX_FIT_SHORT"); const long v = e ? std::atol(e) : 1; return uint32_t(v <= 1 ? v * 4 * kCpBits : std::max<long>(v, kCpBits)); }();
    const bool fit_short = fit_floor != 0;
    p.wg_lanes = long_lanes ? long_lanes : uint32_t(kHuffWg);
    if (fit_short && base_bits == uint32_t(kSubseqBits) && p.nseg == 1 && p.restart_mcus == 0 && p.himg.total_bits < uint32_t(kSubseqBits) * uint32_t(kHuffWg) / 4u * 3u) {       // (under three quarters of a workgroup)
        // ... of 512 lanes, or -- the LDS of the counting and the write pass is sized per lane -- of 256 / 128, the fewest that
        // hold the scan at the default length: four times the workgroups per CU for the same scan (32768 x 256x256: 130 -> 176
        // Gpixels/s, 16384 x 500x375: 235 -> 284; `-DMJX_HUFF_WG=128` had measured it for the whole library)
        uint32_t lanes = uint32_t(kHuffWg);
        while (lanes > 128u && uint64_t(p.himg.total_bits) <= uint64_t(lanes / 2u) * uint32_t(kSubseqBits)) lanes /= 2u;
        p.wg_lanes = lanes;
        const uint32_t fit = ((p.himg.total_bits + lanes - 1) / lanes + uint32_t(kCpBits) - 1) / uint32_t(kCpBits) * uint32_t(kCpBits);
        base_bits = std::max<uint32_t>(fit_floor / uint32_t(kCpBits) * uint32_t(kCpBits), std::min(base_bits, fit));
    }
    const uint32_t top = base_bits * 5 / 4;
    auto bit0 = [&](uint32_t g) { return p.seg[2 * size_t(g) + 1]; };
    p.himg.sub_bits = long_bits ? long_bits : choose_subseq_bits(p.himg.total_bits, base_bits);
    if (p.nseg == 1 && p.restart_mcus == 0) {
        p.himg.nsub = (p.himg.total_bits + p.himg.sub_bits - 1) / p.himg.sub_bits;
        p.seg[0] = 0;
        p.seg[2] = p.himg.nsub;
        return;
    }
    auto count = [&](uint32_t bits) {
        uint32_t n = 0;
        for (uint32_t g = 0; g < p.nseg; g++) {
            const uint32_t len = bit0(g + 1) - bit0(g);
            n += len ? (len + bits - 1) / bits : 1u;
        }
        return n;
    };
    // the same workgroup-filling rule as choose_subseq_bits, on the segmented count
    uint32_t sub = count(p.himg.sub_bits);
    const uint32_t nwg = sub / uint32_t(kHuffWg);
    if (nwg > 0 && sub % uint32_t(kHuffWg) != 0)
        for (uint32_t bits = p.himg.sub_bits + kCpBits; bits <= top; bits += kCpBits)
            if (count(bits) <= nwg * uint32_t(kHuffWg)) { p.himg.sub_bits = bits; break; }
    sub = 0;
    for (uint32_t g = 0; g <= p.nseg; g++) {
        if (g > 0) {
            const uint32_t len = bit0(g) - bit0(g - 1);
            sub += len ? (len + p.himg.sub_bits - 1) / p.himg.sub_bits : 1u;
        }
        p.seg[2 * size_t(g)] = sub;
    }
    p.himg.nsub = sub;
}

// The scans of a progressive picture (geometry already planned): the script's rule (prog_scan_ok), the distinct decode tables, the
// restart intervals of every scan and the levels.
static int plan_progressive(const mjx_scan_desc &d, ImagePlan &p)
{
    int8_t bits[3][64];
    std::memset(bits, -1, sizeof bits);
    p.prog = true;
    p.lut.clear();
    std::vector<std::pair<const mjx_hufftab *, uint32_t>> built[2];      // [is_dc]: table -> its first entry in p.lut
    static thread_local LutEntry tmp[2 * kLutPrimarySize + 4096];
    auto table = [&](const mjx_hufftab &t, bool is_dc, uint32_t *at) -> int {
        size_t n = 0;
        for (int i = 0; i < 16; i++) n += t.bits[i];
        for (const auto &b : built[is_dc])
            if (std::memcmp(b.first->bits, t.bits, 16) == 0 && std::memcmp(b.first->vals, t.vals, std::min(n, sizeof t.vals)) == 0) { *at = b.second; return 0; }
        const int k = build_decode_table(t.bits, t.vals, is_dc, tmp, int(sizeof tmp / sizeof tmp[0]), false);
        if (k < 0) return -k;
        *at = uint32_t(p.lut.size());
        built[is_dc].emplace_back(&t, *at);
        p.lut.insert(p.lut.end(), tmp, tmp + k);
        while (p.lut.size() % 4) p.lut.push_back(0);
        return 0;
    };
    std::vector<uint32_t> lvl[3];                  // per component: the level of the last scan that touched coefficient k
    for (uint32_t c = 0; c < 3; c++) lvl[c].assign(64, 0);
    uint32_t dc_level[3] = {0, 0, 0};              // ... and of its first DC scan
    for (uint32_t k = 0; k < d.n_parts; k++) {
        const mjx_scan_part &part = d.parts[k];
        const mjx_scan_prog &pr = d.prog[k];
        if (!prog_scan_ok(bits, p.ncomp, part.ncomp, part.comp, pr.ss, pr.se, pr.ah, pr.al)) return MJX_ERR_UNSUPPORTED_FORMAT;
        if (!part.scan && part.scan_len) return MJX_ERR_INVALID_ARG;
        if (part.scan_len >= (size_t(1) << 28)) return MJX_ERR_UNSUPPORTED_FORMAT;
        ProgScanPlan s;
        s.ss = pr.ss; s.se = pr.se; s.ah = pr.ah; s.al = pr.al;
        s.ncomp = part.ncomp;
        s.scan = part.scan;
        for (uint32_t q = 0; q < part.ncomp; q++) {
            s.comp[q] = part.comp[q];
            if (pr.ss == 0 && pr.ah == 0) { const int rc = table(part.dc[q], true, &s.tab[q]); if (rc) return rc; }
            if (pr.ss != 0 && q == 0) { const int rc = table(part.ac[0], false, &s.tab[0]); if (rc) return rc; }
            for (uint32_t z = pr.ss; z <= pr.se; z++) s.level = std::max(s.level, lvl[part.comp[q]][z] + 1);
            // (an AC scan stands behind its component's first DC scan, G.1.1.1: it counts as touching it)
            if (pr.ss != 0) s.level = std::max(s.level, dc_level[part.comp[q]] + 1);
        }
        for (uint32_t q = 0; q < part.ncomp; q++)
            if (pr.ss == 0 && pr.ah == 0) dc_level[part.comp[q]] = s.level;
        for (uint32_t q = 0; q < part.ncomp; q++)
            for (uint32_t z = pr.ss; z <= pr.se; z++) lvl[part.comp[q]][z] = s.level;
        p.prog_levels = std::max(p.prog_levels, s.level);
        s.units = part.ncomp == 1 ? p.cbw[part.comp[0]] * p.cbh[part.comp[0]] : p.nmcu;
        s.per_interval = part.restart_interval ? part.restart_interval : s.units;
        const uint32_t nint = (s.units + s.per_interval - 1) / s.per_interval;
        if (part.restart_interval && part.n_restart + 1 < nint) return MJX_ERR_TRUNCATED;       // fewer RSTn markers than intervals
        if (part.n_restart && !part.restart_offsets) return MJX_ERR_INVALID_ARG;
        s.cuts.push_back(0);
        for (uint32_t g = 1; g < nint; g++) {
            const uint32_t at = part.restart_offsets[g - 1];
            if (at > part.scan_len || at < s.cuts.back()) return MJX_ERR_INVALID_ARG;
            s.cuts.push_back(at);
        }
        // (markers beyond the last interval's: whatever lies behind the first of them is never looked at)
        const size_t end = part.restart_interval && part.n_restart >= nint ? part.restart_offsets[nint - 1] : part.scan_len;
        if (end > part.scan_len || end < s.cuts.back()) return MJX_ERR_INVALID_ARG;
        s.cuts.push_back(uint32_t(end));
        p.prog_bytes += part.scan_len;
        if (pr.ss != 0) p.prog_ac_bytes += part.scan_len;
        p.pscans.push_back(std::move(s));
    }
    for (uint32_t c = 0; c < p.ncomp; c++) if (bits[c][0] < 0) return MJX_ERR_UNSUPPORTED_FORMAT;      // a component without a first DC scan
    p.lut_plain_n = uint32_t(p.lut.size());
    return MJX_OK;
}

uint64_t prog_layout(const ImagePlan &p, uint64_t store0, uint32_t img, uint32_t pic_index, ProgPic &pic,
                     std::vector<std::vector<ProgLane>> &levels, std::vector<uint8_t> &bytes, uint64_t *bytes_at)
{
    const bool append = !bytes_at || *bytes_at == kProgAppend;
    uint64_t next = append ? bytes.size() : *bytes_at;
    if (bytes_at) *bytes_at = next;
    std::memset(&pic, 0, sizeof pic);
    pic.ncomp = p.ncomp; pic.mcux = p.mcux; pic.mcuy = p.mcuy;
    for (uint32_t q = 0; q < p.ncomp && q < 3; q++) {
        pic.h[q] = p.h[q]; pic.v[q] = p.v[q];
        pic.pbw[q] = p.mcux * p.h[q]; pic.pbh[q] = p.mcuy * p.v[q];
        pic.cbw[q] = p.cbw[q]; pic.cbh[q] = p.cbh[q];
        pic.plane[q] = store0;
        store0 += uint64_t(pic.pbw[q]) * pic.pbh[q] * 64u;
    }
    for (const ProgScanPlan &sc : p.pscans) {
        const uint64_t at = next;
        next += sc.cuts.back();
        if (append && sc.cuts.back()) bytes.insert(bytes.end(), sc.scan, sc.scan + sc.cuts.back());
        if (levels.size() < sc.level) levels.resize(sc.level);
        for (size_t g = 0; g + 1 < sc.cuts.size(); g++) {
            ProgLane ln;
            std::memset(&ln, 0, sizeof ln);
            ln.byte_off = at + sc.cuts[g];
            ln.nbytes = sc.cuts[g + 1] - sc.cuts[g];
            ln.first = uint32_t(g) * sc.per_interval;
            ln.count = std::min(sc.per_interval, sc.units - ln.first);
            ln.img = img;
            ln.pic = pic_index;
            for (uint32_t q = 0; q < 3; q++) { ln.tab[q] = sc.tab[q]; ln.comp[q] = sc.comp[q]; }
            ln.ss = sc.ss; ln.se = sc.se; ln.ah = sc.ah; ln.al = sc.al; ln.ncomp = sc.ncomp;
            levels[sc.level - 1].push_back(ln);
        }
    }
    return store0;
}

int plan_image(const mjx_scan_desc &d, const mjx_opts &opts, ImagePlan &p, bool scan_part)
{
    p = ImagePlan{};
    auto fail = [&](int code) { p.status = code; return code; };
    const uint32_t scale = opts.scale_denom <= 1 ? 1u : opts.scale_denom;
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return fail(MJX_ERR_INVALID_ARG);
    if (scale != 1 && opts.layout == MJX_LAYOUT_REF_COMPAT) return fail(MJX_ERR_INVALID_ARG);    // (the reference has no scaled decode)
    p.scale = scale;
    // libjpeg's pixels: STANDARD layout, at full size unless the inverse DCT is libjpeg's too and the call opts into its reduced transforms
    // (MJX_OPTS_EXACT_SCALE: without that byte a scale stays refused, as before the byte existed; a scan of a multi-scan file has no
    // pixels: its picture's plan carries the option)
    if (opts.pixels > MJX_PIXELS_LIBJPEG) return fail(MJX_ERR_INVALID_ARG);
    const bool lj = opts.pixels == MJX_PIXELS_LIBJPEG && !scan_part;
    if (MJX_OPTS_EXACT_SCALE(&opts) > 1) return fail(MJX_ERR_INVALID_ARG);
    const bool exact_scale = MJX_OPTS_EXACT_SCALE(&opts) == 1;
    if (exact_scale && (opts.pixels != MJX_PIXELS_LIBJPEG || MJX_OPTS_IDCT(&opts) != MJX_IDCT_ISLOW)) return fail(MJX_ERR_INVALID_ARG);
    if (lj && ((scale != 1 && !exact_scale) || opts.layout == MJX_LAYOUT_REF_COMPAT || opts.strict_ref)) return fail(MJX_ERR_INVALID_ARG);
    // libjpeg's integer inverse DCT: with its pixels only
    if (MJX_OPTS_IDCT(&opts) > MJX_IDCT_ISLOW) return fail(MJX_ERR_INVALID_ARG);
    if (MJX_OPTS_IDCT(&opts) == MJX_IDCT_ISLOW && opts.pixels != MJX_PIXELS_LIBJPEG) return fail(MJX_ERR_INVALID_ARG);
    const bool islow = lj && MJX_OPTS_IDCT(&opts) == MJX_IDCT_ISLOW;
    // the file's own colour model: STANDARD layout without strict_ref only (the reference has one rule)
    if (MJX_OPTS_COLOR(&opts) > MJX_COLOR_FILE) return fail(MJX_ERR_INVALID_ARG);
    const bool color_file = MJX_OPTS_COLOR(&opts) == MJX_COLOR_FILE;
    if (color_file && (opts.layout == MJX_LAYOUT_REF_COMPAT || opts.strict_ref)) return fail(MJX_ERR_INVALID_ARG);
    const bool four = color_file && !scan_part && d.ncomp == 4;
    if (MJX_OPTS_PROGRESSIVE(&opts) > 1) return fail(MJX_ERR_INVALID_ARG);
    const bool prog = d.prog != nullptr && !scan_part;      // a progressive file: the opt-in, STANDARD layout without strict_ref
    if (prog && (opts.layout == MJX_LAYOUT_REF_COMPAT || opts.strict_ref)) return fail(MJX_ERR_INVALID_ARG);
    if (prog && MJX_OPTS_PROGRESSIVE(&opts) != 1) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
    const bool gather = d.n_parts != 0 || prog;    // the picture of a multi-scan file: geometry only, no scan of its own
    if (prog) {
        if (!d.parts || d.n_parts < 1 || (d.ncomp != 1 && d.ncomp != 3)) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
    } else if (gather) {
        if (!d.parts || d.n_parts < 2 || d.n_parts > 3 || d.ncomp != 3) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
        if (opts.layout == MJX_LAYOUT_REF_COMPAT || opts.strict_ref) return fail(MJX_ERR_UNSUPPORTED_FORMAT);   // the reference stops after scan 1
    } else if (!d.scan) {
        return fail(MJX_ERR_INVALID_ARG);
    }
    if (d.ncomp != 1 && d.ncomp != 3 && !(scan_part && d.ncomp == 2) && !(four && !gather)) return fail(MJX_ERR_UNSUPPORTED_FORMAT);     // decoder.rs:328-330
    // what the components are: by position unless the call takes the file's word for it
    p.model = d.ncomp == 1 ? MJX_MODEL_GREY : MJX_MODEL_YCBCR;
    if (color_file && !scan_part && d.ncomp == 3 && d.model == MJX_MODEL_RGB) p.model = MJX_MODEL_RGB;
    else if (color_file && !scan_part && d.ncomp == 3 && d.model > MJX_MODEL_RGB) return fail(MJX_ERR_INVALID_ARG);
    if (four) {
        if (d.model != MJX_MODEL_CMYK && d.model != MJX_MODEL_YCCK) return fail(MJX_ERR_INVALID_ARG);
        p.model = d.model;
    }
    const bool other_model = p.model >= MJX_MODEL_RGB;
    if (other_model && lj) return fail(MJX_ERR_UNSUPPORTED_FORMAT);        // (libjpeg's pixels of these models: not built)
    if (d.width == 0 || d.height == 0) return fail(MJX_ERR_REF_PANIC);             // x_factor division by zero
    // huffman.rs:127-128 preloads data[0..4] and panics on a shorter scan; the bug-compatible modes keep that.  Otherwise a
    // short scan (a flat 8x8 grey picture has one byte of entropy data) is decoded: past its end the lanes read the 0xAA
    // padding the reference itself reads there (huffman.rs:236-246).
    if (!gather && d.scan_len < ((opts.strict_ref || opts.layout == MJX_LAYOUT_REF_COMPAT) ? 4u : 1u)) return fail(MJX_ERR_TRUNCATED);
    if (d.scan_len >= (size_t(1) << 28)) return fail(MJX_ERR_UNSUPPORTED_FORMAT);  // bit positions are 32 bit
    p.width = d.width;
    p.height = d.height;
    p.out_w = (p.width + scale - 1) / scale;
    p.out_h = (p.height + scale - 1) / scale;
    p.ncomp = d.ncomp;
    p.layout = opts.layout;
    p.scan = d.scan;
    p.scan_len = d.scan_len;
    p.stuffed = d.scan_is_stuffed != 0 && !gather;
    auto comp_of = [&d](uint32_t c) -> const mjx_comp & { return c < 3 ? d.comp[c] : d.comp_fourth; };
    for (uint32_t c = 0; c < p.ncomp; c++) {
        const mjx_comp &k = comp_of(c);
        // factors of 1, 2 and 4 (a 3 or anything above 4: not a power of two, or beyond the 32 x 32 MCU the pixel forms hold); the
        // reference asserts 1 or 2 (mod.rs:275-277), so its own modes answer a 4 as it does
        if (!sampling_factor_ok(k.h) || !sampling_factor_ok(k.v)) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
        if ((k.h > 2 || k.v > 2) && (opts.layout == MJX_LAYOUT_REF_COMPAT || opts.strict_ref)) return fail(MJX_ERR_REF_PANIC);
        if (k.tq > 3 || !(d.qt_present & (1u << k.tq))) return fail(MJX_ERR_MISSING_TABLE);      // decoder.rs:222-225
        if (!gather && (k.td > 3 || !(d.dc_present & (1u << k.td)))) return fail(MJX_ERR_MISSING_TABLE);      // decoder.rs:158-160
        if (!gather && (k.ta > 3 || !(d.ac_present & (1u << k.ta)))) return fail(MJX_ERR_MISSING_TABLE);      // decoder.rs:154-156
        p.h[c] = k.h;
        p.v[c] = k.v;
        p.tq[c] = k.tq;
    }
    // A single-component scan is non-interleaved in the standard: one block per MCU whatever SOF0 says.
    // The reference keeps h*v blocks per "MCU" (decoder.rs:200-201), which REF_COMPAT reproduces.
    if (p.ncomp == 1 && p.layout == MJX_LAYOUT_STANDARD) p.h[0] = p.v[0] = 1;
    p.hmax = p.vmax = 1;
    for (uint32_t c = 0; c < p.ncomp; c++) {
        if (p.h[c] > p.hmax) p.hmax = p.h[c];
        if (p.v[c] > p.vmax) p.vmax = p.v[c];
    }
    for (uint32_t c = 0; c < p.ncomp; c++)
        if (p.hmax % p.h[c] || p.vmax % p.v[c]) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
    p.bpm = 0;
    {                      // T.81 B.2.3: an interleaved MCU holds at most 10 blocks; three components may fill the per-MCU tables (12)
        uint32_t blocks = 0;
        for (uint32_t c = 0; c < p.ncomp; c++) blocks += p.h[c] * p.v[c];
        if (blocks > (four ? 10u : uint32_t(kMaxBlocksPerMcu))) return fail(MJX_ERR_UNSUPPORTED_FORMAT);
    }
    for (uint32_t c = 0; c < p.ncomp; c++)
        for (uint32_t by = 0; by < p.v[c]; by++)
            for (uint32_t bx = 0; bx < p.h[c]; bx++) {
                p.blk_comp[p.bpm] = uint8_t(c);
                p.blk_bx[p.bpm] = uint8_t(bx);
                p.blk_by[p.bpm] = uint8_t(by);
                p.bpm++;
            }
    p.mcux = (p.width + 8 * p.hmax - 1) / (8 * p.hmax);
    p.mcuy = (p.height + 8 * p.vmax - 1) / (8 * p.vmax);
    // region-of-interest decode: the rectangle must lie inside the picture the call would otherwise write
    p.roi_w = p.out_w;
    p.roi_h = p.out_h;
    if (!scan_part && opts.rois && opts.n_rois && (opts.rois[0].w || opts.rois[0].h)) {
        const mjx_rect &r = opts.rois[0];
        if (p.layout == MJX_LAYOUT_REF_COMPAT) return fail(MJX_ERR_INVALID_ARG);            // (as with a scale)
        if (!r.w || !r.h || r.x >= p.out_w || r.y >= p.out_h || r.w > p.out_w - r.x || r.h > p.out_h - r.y) return fail(MJX_ERR_INVALID_ARG);
        p.cropped = true;
        p.roi_x = r.x; p.roi_y = r.y; p.roi_w = r.w; p.roi_h = r.h;
    }
    {
        const uint32_t pw = 8 / scale * p.hmax, ph = 8 / scale * p.vmax;      // an MCU's patch of the output picture
        p.lj = lj;
        p.islow = islow;
        // (jdsample.c takes its triangle filters for downsampled_width > 2 only: a narrower plane of ratios (2, 1) or (2, 2) is replicated)
        for (uint32_t c = 0; islow && scale == 1 && c < p.ncomp; c++) {
            const uint32_t cw = (p.width * p.h[c] + p.hmax - 1) / p.hmax, rh = p.hmax / p.h[c], rv = p.vmax / p.v[c];
            if (cw <= 2 && rh == 2 && (rv == 1 || rv == 2)) p.lj_rep |= 1u << c;
        }
        // (... at a reduced scale: libjpeg's transform size per component, the same rule on the scaled plane and the scaled ratios, and
        // at 1/8 no filter at all -- jdsample.c turns fancy upsampling off when min_DCT_scaled_size is 1)
        uint32_t red_gx = 0, red_gy = 0;
        for (uint32_t c = 0; islow && scale != 1 && c < p.ncomp; c++) {
            const uint32_t m = 8 / scale, nc = red_size(m, p.h[c], p.v[c], p.hmax, p.vmax);
            const RedPlane g = red_plane(p.width, p.height, p.h[c], p.v[c], p.hmax, p.vmax, m, nc);
            const uint32_t cw = g.cw, rh = g.rh, rv = g.rv;
            p.red_n[c] = uint8_t(nc);
            if (scale == 8 || (cw <= 2 && rh == 2 && (rv == 1 || rv == 2))) p.lj_rep |= 1u << c;
            else { red_gx = std::max(red_gx, rh > 1 ? rh : 0u); red_gy = std::max(red_gy, rv > 1 ? rv : 0u); }
        }
        // (libjpeg's pixels: the rectangle grown by the filter's reach -- a pixel's chroma neighbours lie up to hmax x vmax pixels away;
        // at a reduced scale one sample of the filtered component with the largest scaled ratio)
        const uint32_t gx = islow && scale != 1 ? red_gx : lj && p.hmax > 1 ? p.hmax : 0u, gy = islow && scale != 1 ? red_gy : lj && p.vmax > 1 ? p.vmax : 0u;
        const uint32_t x0 = p.roi_x > gx ? p.roi_x - gx : 0u, x1 = std::min(p.out_w - 1, p.roi_x + p.roi_w - 1 + gx);
        const uint32_t y0 = p.roi_y > gy ? p.roi_y - gy : 0u, y1 = std::min(p.out_h - 1, p.roi_y + p.roi_h - 1 + gy);
        p.roi_mc0 = x0 / pw; p.roi_mc1 = x1 / pw;
        p.roi_mr0 = y0 / ph; p.roi_mr1 = y1 / ph;
    }
    if (p.layout == MJX_LAYOUT_REF_COMPAT) {
        const uint64_t nb = uint64_t((p.width + 7) / 8) * ((p.height + 7) / 8);    // decoder.rs:164-166
        const uint64_t f = uint64_t(p.hmax) * p.vmax;
        p.nmcu = uint32_t((nb + f - 1) / f);                                       // decoder.rs:191-192 (Q2)
    } else {
        p.nmcu = p.mcux * p.mcuy;
    }
    if (p.layout == MJX_LAYOUT_REF_COMPAT) {
        const int rc = plan_ref_layout(p);
        if (rc != MJX_OK) return fail(rc);
    }

    if (gather) {
        // no scan of its own: the kernels of the entropy stage find no subsequences here; stage B needs the geometry above,
        // the dequantisation multipliers below and the components' own block grids (what the scans actually carry)
        p.role = 2;
        std::memset(&p.himg, 0, sizeof p.himg);
        p.himg.bpm = p.bpm;
        p.himg.total_blocks = p.nmcu * p.bpm;
        p.himg.sub_bits = kSubseqBits;
        p.himg.cp_bits = uint32_t(kCpBits);
        p.nseg = 1;
        p.seg = {0u, 0u, 0u, 0u};
        for (uint32_t c = 0; c < p.ncomp; c++) {
            p.cbw[c] = ((p.width * p.h[c] + p.hmax - 1) / p.hmax + 7) / 8;
            p.cbh[c] = ((p.height * p.v[c] + p.vmax - 1) / p.vmax + 7) / 8;
        }
    }
    if (prog) {
        const int rc = plan_progressive(d, p);
        if (rc != MJX_OK) return fail(rc);
    }
    int dc_base[4] = {-1, -1, -1, -1}, ac_base[4] = {-1, -1, -1, -1};
    if (!gather) {
    // decode tables: each distinct (class, slot) used by the scan is built once.  Layout: the primary tables first, each
    // on a multiple of its size (lut_slot ORs the index into the base) -- an AC table of the second set with its pair part
    // right behind it --, then the sub-tables; a table's links are relative to its own primary table.
    // Two sets: the plain one for the write pass, and one whose AC tables have a pair part for the passes that only count
    // (mjx_huff.h); p.lut holds the first, then (from lut_plain_n on) the second.
    p.lut.clear();
    static thread_local LutEntry tmp[2 * kLutPrimarySize + 4096];
    int dc_base2[4] = {-1, -1, -1, -1}, ac_base2[4] = {-1, -1, -1, -1};
    auto build_set = [&](bool pair, std::vector<LutEntry> &out, int *dcb, int *acb) -> int {
        std::vector<std::vector<LutEntry>> built;
        std::vector<int> units;                              // primary-sized slots the table takes in front (1, or 2 with a pair part)
        int next_unit = 0;
        auto add_table = [&](const mjx_hufftab &t, bool is_dc) -> int {
            const bool with_pair = pair && !is_dc;
            const int n = build_decode_table(t.bits, t.vals, is_dc, tmp, int(sizeof tmp / sizeof tmp[0]), with_pair);
            if (n < 0) return n;
            built.emplace_back(tmp, tmp + n);
            units.push_back(with_pair ? 2 : 1);
            const int base = next_unit * kLutPrimarySize;
            next_unit += units.back();
            return base;
        };
        // (a slot that holds the same table as one built already shares it: the scans of a multi-scan file arrive with a slot per
        // component, and components that decode alike are what shortens the decoder's block-in-MCU state below)
        auto same_table = [](const mjx_hufftab &x, const mjx_hufftab &y) {
            size_t n = 0;
            for (int i = 0; i < 16; i++) n += x.bits[i];
            return std::memcmp(x.bits, y.bits, sizeof x.bits) == 0 && std::memcmp(x.vals, y.vals, std::min(n, sizeof x.vals)) == 0;
        };
        for (uint32_t c = 0; c < p.ncomp; c++) {
            const mjx_comp &k = comp_of(c);
            for (uint32_t e = 0; e < c && dcb[k.td] < 0; e++)
                if (same_table(d.dc[comp_of(e).td], d.dc[k.td])) dcb[k.td] = dcb[comp_of(e).td];
            if (dcb[k.td] < 0) {
                const int b = add_table(d.dc[k.td], true);
                if (b < 0) return b;
                dcb[k.td] = b;
            }
            for (uint32_t e = 0; e < c && acb[k.ta] < 0; e++)
                if (same_table(d.ac[comp_of(e).ta], d.ac[k.ta])) acb[k.ta] = acb[comp_of(e).ta];
            if (acb[k.ta] < 0) {
                const int b = add_table(d.ac[k.ta], false);
                if (b < 0) return b;
                acb[k.ta] = b;
            }
        }
        size_t subs = size_t(next_unit) * kLutPrimarySize;                            // where the next sub-table region goes
        out.assign(subs, 0);
        size_t own = 0;
        for (size_t k = 0; k < built.size(); k++) {
            const std::vector<LutEntry> &t = built[k];
            const size_t front = size_t(units[k]) * kLutPrimarySize;
            for (size_t i = 0; i < front; i++) {
                LutEntry e = t[i];
                if (i < size_t(kLutPrimarySize) && lut_is_link(e)) e = lut_link(unsigned(lut_link_offset(e) - front + subs - own), e & 15u);
                out[own + i] = e;
            }
            out.insert(out.end(), t.begin() + long(front), t.end());
            subs += t.size() - front;
            own += front;
        }
        // table offsets become 16-bit LDS addresses on the device; four tables of a baseline scan need < 24 KB
        if (out.size() * sizeof(LutEntry) > 0x7fff) return -MJX_ERR_BAD_HUFFMAN;
        while (out.size() % 4) out.push_back(0);                                      // 16-byte granules for staging
        return 0;
    };
    {
        std::vector<LutEntry> second;
        int rc1 = build_set(false, p.lut, dc_base, ac_base);
        if (rc1 == 0) rc1 = build_set(true, second, dc_base2, ac_base2);
        if (rc1 < 0) return fail(-rc1);
        p.lut_plain_n = uint32_t(p.lut.size());
        p.lut.insert(p.lut.end(), second.begin(), second.end());
    }
    // (see ImagePlan::emit_fits: a 1-bit DC code and a 2-bit entry -- a 1-bit code for an AC symbol of size 1 --, per component)
    p.emit_fits = true;
    for (uint32_t c = 0; c < p.ncomp; c++) {
        const mjx_hufftab &dc = d.dc[comp_of(c).td], &ac = d.ac[comp_of(c).ta];
        uint32_t dc_min = 0, entry_min = 0xffffu, v = 0;
        for (uint32_t l = 1; l <= 16 && !dc_min; l++) if (dc.bits[l - 1]) dc_min = l;
        for (uint32_t l = 1; l <= 16; l++)
            for (uint32_t k = 0; k < ac.bits[l - 1]; k++, v++)
                if (ac.vals[v] & 15u) entry_min = std::min(entry_min, l + (ac.vals[v] & 15u));
        if (dc_min == 1u && entry_min == 2u) p.emit_fits = false;
    }
    std::memset(&p.himg, 0, sizeof p.himg);
    for (uint32_t b = 0; b < p.bpm; b++) {
        const mjx_comp &k = comp_of(p.blk_comp[b]);
        p.himg.btab[b].tabs = uint32_t(dc_base[k.td]) * uint32_t(sizeof(LutEntry)) | (uint32_t(ac_base[k.ta]) * uint32_t(sizeof(LutEntry)) << 16);
        p.himg.btab[b].next = b + 1 == p.bpm ? 0 : b + 1;
        p.himg.tabs_pair[b] = uint32_t(dc_base2[k.td]) * uint32_t(sizeof(LutEntry)) | (uint32_t(ac_base2[k.ta]) * uint32_t(sizeof(LutEntry)) << 16);
    }
    p.himg.bpm = p.bpm;
    {
        // The decoder's "block in MCU" state only selects tables.  Where the MCU's table sequence repeats with a shorter period --
        // Cb and Cr in a scan of their own share both tables: period 1 -- the state counts inside that period: two decodes that
        // agree on the bit position and the zig-zag index but disagree on which of the two chroma blocks they are in would
        // otherwise never be seen to coincide, and every subsequence of such a scan was re-decoded in one serial chain
        // (1024 copies of a 4K luma + chroma file: 41.7 ms of merge rounds; block indices come from counts, not from this state).
        uint32_t per = 1;
        for (; per < p.bpm; per++) {
            if (p.bpm % per) continue;
            bool rep = true;
            for (uint32_t b = per; b < p.bpm && rep; b++)
                rep = p.himg.btab[b].tabs == p.himg.btab[b - per].tabs && p.himg.tabs_pair[b] == p.himg.tabs_pair[b - per];
            if (rep) break;
        }
        for (uint32_t b = 0; b < per; b++) p.himg.btab[b].next = b + 1 == per ? 0 : b + 1;
        p.himg.bpm = per;
    }
    p.himg.cp_bits = uint32_t(kCpBits);            // (build_batch widens it for the pictures whose first decode emits)
    p.himg.warm_bits = 0;
    p.himg.total_bits = uint32_t(p.scan_len * 8);
    p.himg.total_blocks = p.nmcu * p.bpm;
    p.restart_mcus = d.restart_interval;
    p.seg.clear();
    if (p.restart_mcus == 0) {
        p.nseg = 1;
        p.seg = {0u, 0u, 0u, p.himg.total_bits};
    } else {
        // Each restart interval is decoded on its own: its first subsequence starts in a known state, subsequences do
        // not straddle intervals, and the DC predictors start again (T.81 E.2.4).  REF_COMPAT has no meaning here: the
        // reference panics on DRI (jpeg/mod.rs:424-428).
        if (p.layout == MJX_LAYOUT_REF_COMPAT) return fail(MJX_ERR_DRI_UNSUPPORTED);
        p.nseg = (p.nmcu + p.restart_mcus - 1) / p.restart_mcus;
        if (!p.stuffed && d.n_restart + 1 < p.nseg) return fail(MJX_ERR_TRUNCATED);     // fewer RSTn markers than intervals (a stuffed scan: the device counts them)
        for (uint32_t g = 0; g <= p.nseg && p.stuffed; g++) { p.seg.push_back(0u); p.seg.push_back(0u); }      // placeholder, see replan_subsequences
        for (uint32_t g = 0; g <= p.nseg && !p.stuffed; g++) {
            const uint64_t byte0 = g == 0 ? 0 : (g - 1 < d.n_restart ? d.restart_offsets[g - 1] : p.scan_len);
            if (byte0 > p.scan_len) return fail(MJX_ERR_INVALID_ARG);
            const uint32_t bit0 = g == p.nseg ? p.himg.total_bits : uint32_t(byte0 * 8);
            if (g > 0 && bit0 < p.seg[2 * g - 1]) return fail(MJX_ERR_INVALID_ARG);
            p.seg.push_back(0u);
            p.seg.push_back(bit0);
        }
    }
    replan_subsequences(p, uint32_t(kSubseqBits));

    }   // !gather

    // dequantisation x IDCT prescale, zig-zag order (reference: decoder.rs:230-232 multiplies by the raw table;
    // the AAN row/column factors and the 1/8 are folded in here so the kernel does one multiply per coefficient)
    double aan[8];
    for (int k = 0; k < 8; k++) aan[k] = k == 0 ? 1.0 : std::cos(k * 3.14159265358979323846 / 16.0) * std::sqrt(2.0);
    for (uint32_t c = 0; c < p.ncomp; c++)
        for (int k = 0; k < 64; k++) {
            const int nat = kZigZag[k];
            p.qmult[c][k] = float(double(d.qt[p.tq[c]][k]) * aan[nat >> 3] * aan[nat & 7] / 8.0);
            p.qint[c][k] = uint32_t(d.qt[p.tq[c]][k]);
        }
    // scaled decode: the N-point transforms of the kernels are plain cosine sums, C(u) C(v) / 4 goes here (N = 8 / scale)
    const uint32_t n = 8 / scale;
    std::memset(p.qmult_scaled, 0, sizeof p.qmult_scaled);
    for (uint32_t c = 0; c < p.ncomp; c++)
        for (int k = 0; k < 64; k++) {
            const uint32_t nat = kZigZag[k], v = nat >> 3, u = nat & 7;
            if (u >= n || v >= n) continue;
            const double cu = u == 0 ? std::sqrt(0.5) : 1.0, cv = v == 0 ? std::sqrt(0.5) : 1.0;
            p.qmult_scaled[c][k] = float(double(d.qt[p.tq[c]][k]) * cu * cv / 4.0);
        }
    return p.status;
}

StageBChoice stage_b_choice(const ImagePlan &p)
{
    const bool luma = p.out_on && p.out_channels == 1;
    // The form, first match: libjpeg's pixels have the generic form alone, whatever else the plan says; REF_COMPAT placement; a
    // scale; Y 2x2 + Cb 1x1 + Cr 1x1 on the 4:2:0 kernel, unless the picture leaves as component planes (no 4:2:0 plane form).
    const bool s420 = p.ncomp == 3 && p.model < MJX_MODEL_RGB && p.h[0] == 2 && p.v[0] == 2 && p.h[1] == 1 && p.v[1] == 1 && p.h[2] == 1 && p.v[2] == 1;
    const StageBForm form = p.lj ? kFormGeneric
                          : p.layout == MJX_LAYOUT_REF_COMPAT ? kFormRefCompat
                          : p.scale > 1 ? (p.scale == 2 ? kFormHalf : p.scale == 4 ? kFormQuarter : kFormEighth)
                          : s420 && !p.ycc_on ? kForm420 : kFormGeneric;
    // The sink, by precedence: (1) libjpeg's planes -- k_upsample_color then writes whatever the picture leaves as; (2) the
    // component planes as the picture; (3) luminance, also as the one-byte intermediate of a resize or an orientation; (4) an output
    // description with no resize behind it -- a resized picture's description is the resize's, stage B writes the packed
    // intermediate; (5) a rectangle; (6) the packed whole picture.  (This is the order in which the features' overwrites of the
    // mode used to follow one another, last writer first; tests/golden/stage_b_choice.npz holds what those gave.)
    const bool red = p.lj && p.islow && p.scale > 1;     // (the integer inverse DCT at a reduced scale: a sink, a pass and a descriptor word of its own)
    const StageBSink sink = p.lj ? (red ? kSinkPlanesRed : p.islow ? kSinkPlanesInt : kSinkPlanes) : p.ycc_on ? kSinkYcc : luma ? kSinkLuma : p.out_on && !p.rs_on ? kSinkOut
                          : p.cropped ? kSinkCropped : kSinkPacked;
    StageBChoice c;
    // (0) ahead of them all: a scan of a multi-scan file has no stage B.  Its tile geometry is still that of `form`.
    c.mode = p.role == 1 ? stage_b_mode(kFormScan, kSinkPacked) : stage_b_mode(form, sink);
    c.tile_420 = form == kForm420;
    // the passes behind stage B: a colour picture is k_resize_out's (rs_on) without an orientation, else k_orient_out's or
    // k_resize_orient's; a luminance picture is always one of the one-channel passes', orientation code 1 included
    const bool pass = p.out_on && p.rs_on;
    c.rs_on = pass && !luma && p.orient == 1 ? 1u : 0u;
    c.or_on = !pass ? kOrNone : luma ? (p.or_copy ? kOrCopyLuma : kOrResizeLuma)
            : p.orient == 1 ? kOrNone : p.or_copy ? kOrCopy : kOrResize;
    c.out_ch = luma ? 1u : 0u;
    // (the integer inverse DCT's pictures with a replicated component are k_upsample_rep's, luminance or not.  A luminance picture
    // reads component 0 alone: only its own bit counts)
    const uint32_t rep = !p.lj || red ? 0u : luma ? p.lj_rep & 1u : p.lj_rep;
    c.lj_rep = rep ? kLjRepOn | rep | (luma ? kLjRepLuma : 0u) : 0u;
    c.lj_luma = p.lj && luma && !rep && !red ? 1u : 0u;      // (a luminance picture is k_upsample_luma's: component 0's plane alone)
    c.lj_on = p.lj && !luma && !rep && !red ? 1u : 0u;
    // (... at a reduced scale k_upsample_red's, luminance or not: every component's transform size and replicate bit, DevImage::lj_red)
    c.lj_red = 0u;
    for (uint32_t k = 0; red && k < 3u; k++) {
        const uint32_t n = k < p.ncomp ? p.red_n[k] : 8u;
        c.lj_red |= ((n >= 8u ? 3u : n >= 4u ? 2u : n >= 2u ? 1u : 0u) | (p.lj_rep >> k & 1u) << 2) << (4u * k);
    }
    if (red) c.lj_red |= kLjRedOn | (luma ? kLjRedLuma : 0u);
    c.lj_out = p.lj && p.out_on && !p.rs_on ? 1u : 0u;
    return c;
}

bool rois_fit(const mjx_opts &opts, size_t n)
{
    if (!opts.rois) return opts.n_rois == 0;
    return opts.n_rois <= 1 || opts.n_rois == n;
}

mjx_opts opts_for_input(const mjx_opts &opts, size_t n, size_t i)
{
    mjx_opts o = opts;
    if (!o.rois || o.n_rois == 0) { o.rois = nullptr; o.n_rois = 0; return o; }
    if (o.n_rois == n && n > 1) o.rois += i;
    o.n_rois = 1;
    return o;
}

bool output_fits(const mjx_output *out, size_t n)
{
    if (!out) return true;
    if (!out->dst) return out->n_dst == 0;
    return out->n_dst == n;
}

int plan_output(ImagePlan &p, const mjx_output *out, size_t i)
{
    p.out_on = false;
    p.out_dev = 0;
    p.out_channels = 3;
    p.out_bytes = uint64_t(p.roi_w) * p.roi_h * 3;
    if (!out || p.status != MJX_OK) return p.status;
    auto fail = [&]() { p.status = MJX_ERR_INVALID_ARG; return p.status; };
    if (out->dtype > MJX_DTYPE_F32 || p.layout == MJX_LAYOUT_REF_COMPAT) return fail();
    const uint8_t channels = reinterpret_cast<const uint8_t *>(out)[MJX_OUTPUT_CHANNELS_OFFSET];       // (the byte behind bgr, mjx.h)
    if (channels != 0 && channels != 1 && channels != 3) return fail();
    const bool luma = channels == 1;                                  // luminance: H x W elements, one plane whatever `planar` says
    if (luma && p.model >= MJX_MODEL_RGB) { p.status = MJX_ERR_UNSUPPORTED_FORMAT; return p.status; }      // (component 0 of such a file is no luminance: not built)
    const uint64_t esz = out->dtype == MJX_DTYPE_U8 ? 1u : out->dtype == MJX_DTYPE_F16 ? 2u : 4u;
    const bool planar = out->planar != 0 && !luma;
    for (int c = 0; c < (luma ? 1 : 3); c++) {
        if (out->dtype != MJX_DTYPE_U8 && !(std::isfinite(out->scale[c]) && std::isfinite(out->bias[c]))) return fail();
        p.out_scale[c] = out->dtype == MJX_DTYPE_U8 ? 1.f : out->scale[c];
        p.out_bias[c] = out->dtype == MJX_DTYPE_U8 ? 0.f : out->bias[c];
    }
    const uint64_t w = p.rs_on ? p.fit_w : p.roi_w, h = p.rs_on ? p.fit_h : p.roi_h, row_min = planar || luma ? w : 3 * w;      // (a resized picture: the target)
    for (int c = 0; c < 3; c++)                                          // (the pad colour: the three bytes in front of dst, mjx.h; MJX_FIT_CONTAIN only)
        p.pad[c] = p.rs_on && p.fit_mode == kFitContain ? reinterpret_cast<const uint8_t *>(out)[MJX_OUTPUT_PAD_OFFSET + c] : uint8_t(0);
    p.out_row_pitch = row_min;
    p.out_plane_pitch = planar ? h * w : 0;
    if (out->dst) {
        const mjx_dst &d = out->dst[i];
        if (d.width != w || d.height != h || d.row_pitch < row_min) return fail();
        if (d.row_pitch > (uint64_t(1) << 40) || d.plane_pitch > (uint64_t(1) << 56)) return fail();      // (no overflow below)
        if (planar && d.plane_pitch < h * d.row_pitch) return fail();
        if (!d.dev || (uint64_t(uintptr_t(d.dev)) & (esz - 1))) return fail();
        p.out_dev = uint64_t(uintptr_t(d.dev));
        p.out_row_pitch = d.row_pitch;
        p.out_plane_pitch = planar ? d.plane_pitch : 0;
    }
    // the last element: channel 2's last row's last pixel (planar) or the last row's last channel (interleaved)
    p.out_bytes = ((planar ? 2 * p.out_plane_pitch : 0) + (h - 1) * p.out_row_pitch + row_min) * esz;
    p.out_on = true;
    p.out_dtype = out->dtype;
    p.out_planar = out->planar ? 1u : 0u;             // (luminance: no planes -- kept for mjx_batch_output_info, nothing reads it)
    p.out_bgr = out->bgr && !luma ? 1u : 0u;
    p.out_channels = luma ? 1u : 3u;
    return p.status;
}

int plan_output_of_input(std::vector<ImagePlan> &plans, const mjx_output *out, size_t i)
{
    ImagePlan &p = plans.back();
    const bool was_ok = p.status == MJX_OK;
    const size_t nparts = p.role == 2 ? p.nparts : 0;
    const int rc = plan_output(p, out, i);
    if (was_ok && rc != MJX_OK && nparts && plans.size() > nparts) {       // one status for the whole picture, as plan_input: its scans go
        ImagePlan pic;
        pic.status = rc;
        plans.resize(plans.size() - 1 - nparts);
        plans.push_back(pic);
    }
    return rc;
}

bool planes_fit(const mjx_planes *pl, size_t n)
{
    if (!pl) return false;
    if (!pl->dst) return pl->n_dst == 0;
    return pl->n_dst == n;
}

int plan_planes(ImagePlan &p, const mjx_planes *pl, size_t i)
{
    p.ycc_on = false;
    if (!pl || p.status != MJX_OK) return p.status;
    auto fail = [&]() { p.status = MJX_ERR_INVALID_ARG; return p.status; };
    if (pl->dtype > MJX_DTYPE_F32 || p.layout == MJX_LAYOUT_REF_COMPAT) return fail();
    if (p.model >= MJX_MODEL_RGB) { p.status = MJX_ERR_UNSUPPORTED_FORMAT; return p.status; }      // (the planes of an RGB, CMYK or YCCK file: not built)
    if (p.islow) { p.status = MJX_ERR_UNSUPPORTED_FORMAT; return p.status; }      // (the integer inverse DCT's planes as the picture: not built)
    const uint32_t nc = p.ncomp;
    const bool il = pl->interleave_chroma != 0 && nc == 3;           // (a one-component file has one plane: the flag has no meaning)
    if (il && (p.h[1] != p.h[2] || p.v[1] != p.v[2])) return fail();
    const uint64_t esz = pl->dtype == MJX_DTYPE_U8 ? 1u : pl->dtype == MJX_DTYPE_F16 ? 2u : 4u;
    for (uint32_t c = 0; c < nc; c++) {
        if (pl->dtype != MJX_DTYPE_U8 && !(std::isfinite(pl->scale[c]) && std::isfinite(pl->bias[c]))) return fail();
        p.out_scale[c] = pl->dtype == MJX_DTYPE_U8 ? 1.f : pl->scale[c];
        p.out_bias[c] = pl->dtype == MJX_DTYPE_U8 ? 0.f : pl->bias[c];
    }
    // libjpeg's pixels: the planes in front of that option's upsampling -- no filter, so no reach: the rectangle's own tiles, and the
    // generic plane form with the rounding half on the DC term instead of k_upsample_color's pass
    if (p.lj) {
        const uint32_t pw = 8 * p.hmax, ph = 8 * p.vmax;
        p.roi_mc0 = p.roi_x / pw; p.roi_mc1 = (p.roi_x + p.roi_w - 1) / pw;
        p.roi_mr0 = p.roi_y / ph; p.roi_mr1 = (p.roi_y + p.roi_h - 1) / ph;
        p.lj = false;
        p.ycc_round = 1;
    }
    uint64_t off = 0, first = 0, last = 0;
    p.ycc_written = 0;
    const uint32_t nplanes = il ? 2u : nc;
    for (uint32_t c = 0; c < nc; c++) {
        const PlaneSpan s = plane_span(p.roi_x, p.roi_y, p.roi_w, p.roi_h, p.h[c], p.v[c], p.hmax, p.vmax);
        p.ycc_x0[c] = s.x0; p.ycc_y0[c] = s.y0; p.ycc_w[c] = s.w; p.ycc_h[c] = s.h;
        p.ycc_written += uint64_t(s.w) * s.h * esz;
        p.ycc_dev[c] = 0; p.ycc_off[c] = 0; p.ycc_pitch[c] = 0;
        if (c >= nplanes) continue;                                    // (Cr rides in plane 1)
        const uint64_t row_min = uint64_t(s.w) * (il && c == 1 ? 2u : 1u);
        uint64_t pitch = row_min;
        if (pl->dst) {
            const mjx_plane_layout &d = pl->dst[i];
            if (d.width[c] != s.w || d.height[c] != s.h || d.row_pitch[c] < row_min || d.row_pitch[c] > (uint64_t(1) << 40)) return fail();
            if (!d.dev[c] || (uint64_t(uintptr_t(d.dev[c])) & (esz - 1))) return fail();
            pitch = d.row_pitch[c];
            p.ycc_dev[c] = uint64_t(uintptr_t(d.dev[c]));
        } else {
            p.ycc_off[c] = off;
        }
        p.ycc_pitch[c] = pitch;
        const uint64_t span = ((uint64_t(s.h) - 1) * pitch + row_min) * esz;
        const uint64_t at = pl->dst ? p.ycc_dev[c] : off;
        if (c == 0) first = at;
        last = std::max(last, at + span);
        off += span;
    }
    p.ycc_on = true;
    p.ycc_il = il ? 1u : 0u;
    p.out_on = true;
    p.out_channels = 3;
    p.out_dtype = pl->dtype;
    p.out_planar = 1; p.out_bgr = 0;
    p.out_dev = p.ycc_dev[0];
    p.out_row_pitch = p.ycc_pitch[0]; p.out_plane_pitch = 0;
    p.out_bytes = last > first ? last - first : ((uint64_t(p.ycc_h[0]) - 1) * p.ycc_pitch[0] + p.ycc_w[0]) * esz;
    return p.status;
}

int plan_planes_of_input(std::vector<ImagePlan> &plans, const mjx_planes *pl, size_t i)
{
    ImagePlan &p = plans.back();
    const bool was_ok = p.status == MJX_OK;
    const size_t nparts = p.role == 2 ? p.nparts : 0;
    const int rc = plan_planes(p, pl, i);
    if (was_ok && rc != MJX_OK && nparts && plans.size() > nparts) {       // one status for the whole picture, as plan_output_of_input
        ImagePlan pic;
        pic.status = rc;
        plans.resize(plans.size() - 1 - nparts);
        plans.push_back(pic);
    }
    return rc;
}

// one status for the whole input: a multi-scan picture that is refused takes its scans' plans with it
static void fail_input(std::vector<ImagePlan> &plans, size_t first, int rc)
{
    plans.resize(first);
    ImagePlan pic;
    pic.status = rc;
    plans.push_back(pic);
}

int resize_opts(uint32_t width, uint32_t height, const mjx_opts &opts_i, const mjx_resize &rs, mjx_opts &eff, mjx_rect &rect)
{
    std::memcpy(&eff, &opts_i, sizeof eff);                                // (byte for byte, as above)
    if (!rs.width || !rs.height || rs.width > kResizeMaxDim || rs.height > kResizeMaxDim) return MJX_ERR_INVALID_ARG;
    if (opts_i.layout == MJX_LAYOUT_REF_COMPAT) return MJX_ERR_INVALID_ARG;
    if (!rs.auto_scale) return MJX_OK;
    if (opts_i.scale_denom > 1) return MJX_ERR_INVALID_ARG;
    if (opts_i.pixels == MJX_PIXELS_LIBJPEG) return MJX_OK;               // (libjpeg's pixels exist at full size only: scale 1 for every picture, the rectangle as given)
    if (!width || !height) return MJX_OK;                                  // (plan_image says what is wrong with the picture)
    uint32_t x = 0, y = 0, w = width, h = height;
    if (opts_i.rois && opts_i.n_rois && (opts_i.rois[0].w || opts_i.rois[0].h)) {
        const mjx_rect &r = opts_i.rois[0];
        if (!r.w || !r.h || r.x >= width || r.y >= height || r.w > width - r.x || r.h > height - r.y) return MJX_ERR_INVALID_ARG;
        x = r.x; y = r.y; w = r.w; h = r.h;
    }
    uint32_t s = 8;
    for (;; s /= 2) {
        rect.x = x / s; rect.y = y / s;
        rect.w = (x + w + s - 1) / s - rect.x; rect.h = (y + h + s - 1) / s - rect.y;
        if (s == 1 || (rect.w >= rs.width && rect.h >= rs.height)) break;
    }
    eff.scale_denom = uint8_t(s);
    const uint32_t ow = (width + s - 1) / s, oh = (height + s - 1) / s;
    if (rect.x == 0 && rect.y == 0 && rect.w == ow && rect.h == oh) { eff.rois = nullptr; eff.n_rois = 0; }   // the whole picture: the plain forms
    else { eff.rois = &rect; eff.n_rois = 1; }
    return MJX_OK;
}

// YCbCr planes with an orientation and / or a resize: the input (planned at the stored rectangle and scale, plans.back()) becomes the
// plain plane decode -- uint8, dense, not interleaved, library-owned: the intermediate -- and the planes that leave are laid out by
// `pl`'s rules.  Without a resize plane k is orient_c(P_k): its sides swap for codes 5 .. 8.  With one, component k's factors in D are
// (h_k, v_k) or, codes 5 .. 8, (v_k, h_k), the maxima likewise, and the plane's target is the whole-picture formula of a W x H
// picture: ceil(W h'_k / hmax') x ceil(H v'_k / vmax').
static void plan_planes_pass(std::vector<ImagePlan> &plans, size_t first, const mjx_planes *pl, const mjx_resize *rs, uint32_t code, size_t i)
{
    static const mjx_planes mid = {MJX_DTYPE_U8, 0, {1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, nullptr, 0};
    plan_output_of_input(plans, nullptr, i);
    if (plan_planes_of_input(plans, &mid, i) != MJX_OK) return;
    ImagePlan &p = plans.back();
    const uint32_t nc = p.ncomp;
    const bool il = pl->interleave_chroma != 0 && nc == 3;
    bool bad = pl->dtype > MJX_DTYPE_F32 || (il && (p.h[1] != p.h[2] || p.v[1] != p.v[2]));
    for (uint32_t c = 0; c < nc && !bad; c++)
        bad = pl->dtype != MJX_DTYPE_U8 && !(std::isfinite(pl->scale[c]) && std::isfinite(pl->bias[c]));
    const uint64_t esz = pl->dtype == MJX_DTYPE_U8 ? 1u : pl->dtype == MJX_DTYPE_F16 ? 2u : 4u;
    const bool sw = orient_swaps(code);
    const uint32_t nplanes = il ? 2u : nc;
    uint64_t off = 0, first_at = 0, last = 0;
    p.yp_written = 0;
    for (uint32_t c = 0; c < nc && !bad; c++) {
        uint32_t w = sw ? p.ycc_h[c] : p.ycc_w[c], h = sw ? p.ycc_w[c] : p.ycc_h[c];
        if (rs) {
            const uint64_t hc = sw ? p.v[c] : p.h[c], vc = sw ? p.h[c] : p.v[c], hm = sw ? p.vmax : p.hmax, vm = sw ? p.hmax : p.vmax;
            w = uint32_t((uint64_t(rs->width) * hc + hm - 1) / hm);
            h = uint32_t((uint64_t(rs->height) * vc + vm - 1) / vm);
        }
        p.yp_w[c] = w; p.yp_h[c] = h;
        p.yp_scale[c] = pl->dtype == MJX_DTYPE_U8 ? 1.f : pl->scale[c];
        p.yp_bias[c] = pl->dtype == MJX_DTYPE_U8 ? 0.f : pl->bias[c];
        p.yp_written += uint64_t(w) * h * esz;
        p.yp_dev[c] = 0; p.yp_off[c] = 0; p.yp_pitch[c] = 0;
        if (c >= nplanes) continue;                                    // (Cr rides in plane 1)
        const uint64_t row_min = uint64_t(w) * (il && c == 1 ? 2u : 1u);
        uint64_t pitch = row_min;
        if (pl->dst) {
            const mjx_plane_layout &dl = pl->dst[i];
            if (dl.width[c] != w || dl.height[c] != h || dl.row_pitch[c] < row_min || dl.row_pitch[c] > (uint64_t(1) << 40)) { bad = true; break; }
            if (!dl.dev[c] || (uint64_t(uintptr_t(dl.dev[c])) & (esz - 1))) { bad = true; break; }
            pitch = dl.row_pitch[c];
            p.yp_dev[c] = uint64_t(uintptr_t(dl.dev[c]));
        } else {
            p.yp_off[c] = off;
        }
        p.yp_pitch[c] = pitch;
        const uint64_t span = ((uint64_t(h) - 1) * pitch + row_min) * esz;
        const uint64_t at = pl->dst ? p.yp_dev[c] : off;
        if (c == 0) first_at = at;
        last = std::max(last, at + span);
        off += span;
    }
    if (bad) { fail_input(plans, first, MJX_ERR_INVALID_ARG); return; }
    p.yp_kind = rs ? kPlaneResize : kPlaneCopy;
    p.yp_code = code;
    p.yp_il = il ? 1u : 0u;
    p.yp_dtype = pl->dtype;
    p.yp_filter = rs ? MJX_RESIZE_FILTER(rs) : 0u;
    p.yp_aa = rs && rs->antialias ? 1u : 0u;
    p.yp_out_w = rs ? rs->width : sw ? p.roi_h : p.roi_w;
    p.yp_out_h = rs ? rs->height : sw ? p.roi_w : p.roi_h;
    p.yp_bytes = last > first_at ? last - first_at : ((uint64_t(p.yp_h[0]) - 1) * p.yp_pitch[0] + p.yp_w[0]) * esz;
}

void plan_input_for(const mjx_scan_desc &d, const mjx_opts &opts_i, const mjx_output *out, const mjx_resize *rs, size_t i,
                    std::vector<ImagePlan> &plans, uint32_t code, const mjx_planes *pl)
{
    if (!rs && code == 1) {
        plan_input(d, opts_i, plans);
        plan_output_of_input(plans, pl ? nullptr : out, i);
        if (pl) plan_planes_of_input(plans, pl, i);
        return;
    }
    const size_t first = plans.size();
    mjx_rect rect{0, 0, 0, 0}, stored{0, 0, 0, 0}, cover{0, 0, 0, 0};
    int rc = MJX_OK;
    mjx_resize rs_s{};                                                     // the resize in S's axes
    if (rs) rs_s = *rs;
    // fit modes (the byte is read from the caller's object, as the filter byte below).  A: the rectangle asked for, in D's coordinates at
    // the scale it is given in.  MJX_FIT_COVER: the picture is the stretch call's with rois[0] = A' -- everything below sees that
    // rectangle; MJX_FIT_CONTAIN: the stretch call's with the target iw x ih, moved to (ox, oy) of the target once it is planned.  A
    // rectangle or a target the checks below refuse is left to them.
    const uint32_t fit = rs ? MJX_RESIZE_FIT(rs) : kFitStretch;
    FitPlan fp{};
    bool fit_known = false;
    mjx_opts opts_f;                                                       // (byte for byte: the colour option lives outside the declared members)
    std::memcpy(&opts_f, &opts_i, sizeof opts_f);
    if (rs && fit < kFitCount && rs->width && rs->height && rs->width <= kResizeMaxDim && rs->height <= kResizeMaxDim) {
        const uint32_t s = rs->auto_scale ? 1u : opts_i.scale_denom > 1 ? opts_i.scale_denom : 1u;
        const uint32_t w = (d.width + s - 1) / s, h = (d.height + s - 1) / s;
        const bool sw = orient_valid(code) && orient_swaps(code);
        const uint32_t dw = sw ? h : w, dh = sw ? w : h;
        mjx_rect a{0, 0, dw, dh};
        const bool given = opts_i.rois && opts_i.n_rois && (opts_i.rois[0].w || opts_i.rois[0].h);
        if (given) a = opts_i.rois[0];
        if ((s == 1 || s == 2 || s == 4 || s == 8) && a.w && a.h && a.x < dw && a.y < dh && a.w <= dw - a.x && a.h <= dh - a.y) {
            fp = fit_rule(fit, a.x, a.y, a.w, a.h, rs->width, rs->height);
            fit_known = true;
            if (fit == kFitCover && (fp.a.w != a.w || fp.a.h != a.h)) {
                cover = mjx_rect{fp.a.x, fp.a.y, fp.a.w, fp.a.h};
                opts_f.rois = &cover; opts_f.n_rois = 1;
            }
            if (fit == kFitContain) { rs_s.width = fp.inner.w; rs_s.height = fp.inner.h; }
        }
    }
    mjx_opts eff;
    std::memcpy(&eff, &opts_f, sizeof eff);
    if (code != 1) {
        // orientation: the rectangle is D's; back to S at the scale it is given in (full size with auto_scale)
        const uint32_t s = rs && rs->auto_scale ? 1u : opts_f.scale_denom > 1 ? opts_f.scale_denom : 1u;
        const uint32_t w = (d.width + s - 1) / s, h = (d.height + s - 1) / s;
        if (!orient_valid(code) || opts_f.layout == MJX_LAYOUT_REF_COMPAT) rc = MJX_ERR_INVALID_ARG;
        else if (w && h && (s == 1 || s == 2 || s == 4 || s == 8) && opts_f.rois && opts_f.n_rois && (opts_f.rois[0].w || opts_f.rois[0].h)) {
            const mjx_rect &r = opts_f.rois[0];
            const OrientMap m = orient_map(code, w, h);
            if (!r.w || !r.h || r.x >= m.dw || r.y >= m.dh || r.w > m.dw - r.x || r.h > m.dh - r.y) rc = MJX_ERR_INVALID_ARG;
            else {
                orient_rect_to_stored(code, w, h, r.x, r.y, r.w, r.h, &stored.x, &stored.y, &stored.w, &stored.h);
                eff.rois = &stored; eff.n_rois = 1;
            }
        }
        if (orient_swaps(code)) std::swap(rs_s.width, rs_s.height);
    }
    // (the filter byte is read from the caller's object: rs_s is a member-wise copy and need not carry it)
    if (rs && (MJX_RESIZE_FILTER(rs) >= kFilterCount || fit >= kFitCount)) rc = MJX_ERR_INVALID_ARG;
    if (pl && fit == kFitContain) rc = MJX_ERR_INVALID_ARG;               // (a pad per component plane: not built)
    if (rs && rc == MJX_OK) {
        mjx_opts in;
        std::memcpy(&in, &eff, sizeof in);
        rc = resize_opts(d.width, d.height, in, rs_s, eff, rect);
    }
    if (rc != MJX_OK && code != 1) { eff.rois = nullptr; eff.n_rois = 0; }  // (the rectangle is D's: the picture's own fault, which comes first, is found on the whole picture)
    plan_input(d, eff, plans);
    if (plans.back().status != MJX_OK) return;
    if (rc != MJX_OK) { fail_input(plans, first, rc); return; }
    if (pl) { plan_planes_pass(plans, first, pl, rs, code, i); return; }
    ImagePlan &p = plans.back();
    p.rs_on = true;
    p.orient = code;
    if (rs) { p.rs_w = rs->width; p.rs_h = rs->height; p.rs_aa = rs->antialias ? 1u : 0u; p.rs_filter = MJX_RESIZE_FILTER(rs); }
    else {
        p.or_copy = true;
        p.rs_w = orient_swaps(code) ? p.roi_h : p.roi_w; p.rs_h = orient_swaps(code) ? p.roi_w : p.roi_h; p.rs_aa = 0; p.rs_filter = 0;
    }
    p.fit_mode = fit;
    p.fit_w = p.rs_w; p.fit_h = p.rs_h;                                    // the picture that leaves: what plan_output lays out
    if (fit_known) {
        p.fit_ax = fp.a.x; p.fit_ay = fp.a.y; p.fit_aw = fp.a.w; p.fit_ah = fp.a.h;
        if (fit == kFitContain) { p.rs_w = fp.inner.w; p.rs_h = fp.inner.h; p.fit_ox = fp.inner.x; p.fit_oy = fp.inner.y; }
    }
    static const mjx_output packed = {MJX_DTYPE_U8, 0, 0, {1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, nullptr, 0};
    plan_output_of_input(plans, out ? out : &packed, i);
}

void plan_input(const mjx_scan_desc &d, const mjx_opts &opts, std::vector<ImagePlan> &out)
{
    if (d.n_parts == 0 || d.prog) {           // (a progressive picture is one plan: its scans are no pictures of their own)
        out.emplace_back();
        plan_image(d, opts, out.back());
        return;
    }
    ImagePlan pic;
    plan_image(d, opts, pic);
    const size_t first = out.size();
    int bad = pic.status;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < d.n_parts && bad == MJX_OK; k++) {
        const mjx_scan_part &part = d.parts[k];
        if (part.ncomp < 1 || part.ncomp > 2) { bad = MJX_ERR_UNSUPPORTED_FORMAT; break; }
        // the scan as a picture of its own: one component over the component's own block grid (non-interleaved order), or
        // two interleaved components on the MCU grid their sampling factors give
        mjx_scan_desc sub;
        std::memset(&sub, 0, sizeof sub);
        sub.scan = part.scan;
        sub.scan_len = part.scan_len;
        sub.ncomp = part.ncomp;
        uint32_t hm = 1, vm = 1;
        for (uint32_t q = 0; q < part.ncomp; q++) {
            const uint32_t c = part.comp[q];
            if (c > 2 || ((seen >> c) & 1)) { bad = MJX_ERR_UNSUPPORTED_FORMAT; break; }
            seen |= 1u << c;
            pic.src_part[c] = k;
            pic.src_comp[c] = q;
            hm = std::max(hm, pic.h[c]);
            vm = std::max(vm, pic.v[c]);
            sub.comp[q] = mjx_comp{d.comp[c].id, uint8_t(part.ncomp == 1 ? 1 : pic.h[c]), uint8_t(part.ncomp == 1 ? 1 : pic.v[c]),
                                   d.comp[c].tq, uint8_t(q), uint8_t(q)};
            sub.dc[q] = part.dc[q];
            sub.ac[q] = part.ac[q];
        }
        if (bad != MJX_OK) break;
        sub.width = uint16_t((uint32_t(d.width) * hm + pic.hmax - 1) / pic.hmax);
        sub.height = uint16_t((uint32_t(d.height) * vm + pic.vmax - 1) / pic.vmax);
        std::memcpy(sub.qt, d.qt, sizeof sub.qt);
        sub.qt_present = d.qt_present;
        sub.dc_present = sub.ac_present = uint8_t((1u << part.ncomp) - 1);
        sub.restart_interval = part.restart_interval;
        sub.n_restart = part.n_restart;
        sub.restart_offsets = part.restart_offsets;
        out.emplace_back();
        ImagePlan &pp = out.back();
        plan_image(sub, opts, pp, true);
        pp.role = 1;
        pp.part_idx = k;
        pp.nparts = d.n_parts;
        if (pp.status != MJX_OK) bad = pp.status;
    }
    if (bad == MJX_OK && seen != 7u) bad = MJX_ERR_UNSUPPORTED_FORMAT;
    pic.nparts = d.n_parts;
    if (bad != MJX_OK) {                       // one status for the whole picture
        out.resize(first);
        pic = ImagePlan{};
        pic.status = bad;
    }
    out.push_back(pic);
}

}   // namespace mjx

// mjx_plan.h -- host-side per-image decode plan: geometry (reference src/jpeg/decoder.rs:164-192,
// 239-250), decode tables, dequantisation multipliers.  Shared by the device API (mjx_device.hip) and the
// CPU emulation harness (tests/emul).
#ifndef MJX_PLAN_H
#define MJX_PLAN_H

#include "mjx.h"
#include "mjx_huff.h"

#include <vector>

namespace mjx {

// One scan of a progressive picture as the planner hands it to the batch (MJX_OPTS_PROGRESSIVE, mjx_prog.h)
struct ProgScanPlan {
    uint8_t ss = 0, se = 0, ah = 0, al = 0;
    uint8_t ncomp = 0, comp[3] = {0, 0, 0};
    uint32_t level = 1;                            // 1 + the largest level of an earlier scan that touches a common (component, coefficient);
                                                   // an AC scan counts its component's first DC scan among them
    uint32_t tab[3] = {0, 0, 0};                   // entries into ImagePlan::lut: the DC table per scan component, or the AC table in [0]
    const uint8_t *scan = nullptr;                 // de-stuffed, restart markers taken out
    uint32_t units = 0, per_interval = 0;          // MCUs (interleaved) or blocks of the component's own grid; units per restart interval
    std::vector<uint32_t> cuts;                    // byte offsets of the intervals' starts, and the scan's length behind them
};

struct ImagePlan {
    int status = MJX_OK;
    uint32_t width = 0, height = 0;
    uint32_t ncomp = 0;
    uint32_t h[4] = {1, 1, 1, 1}, v[4] = {1, 1, 1, 1};   // effective sampling factors (scan order)
    uint32_t tq[4] = {0, 0, 0, 0};
    // colour model (mjx_opts.color): MJX_MODEL_* -- grey for one component and YCbCr for three unless the call asks for the file's own
    // model (MJX_COLOR_FILE) and the description carries RGB, CMYK or YCCK.  A fourth component exists for the last two only.
    uint32_t model = MJX_MODEL_GREY;
    uint32_t hmax = 1, vmax = 1;
    uint32_t bpm = 0;                              // blocks per MCU
    uint32_t mcux = 0, mcuy = 0;                   // MCU grid of the standard layout
    uint32_t nmcu = 0;                             // MCUs to decode (Q2 count in REF_COMPAT)
    uint32_t layout = MJX_LAYOUT_STANDARD;
    uint8_t blk_comp[kMaxBlocksPerMcu] = {0};      // block position in MCU -> component
    uint8_t blk_bx[kMaxBlocksPerMcu] = {0};        //                       -> block column inside the MCU
    uint8_t blk_by[kMaxBlocksPerMcu] = {0};        //                       -> block row inside the MCU
    HuffImage himg{};
    std::vector<LutEntry> lut;                     // all decode tables of the image, concatenated: the plain set (what the write pass
    uint32_t lut_plain_n = 0;                      // uses), then from lut_plain_n on the set with pair parts (the counting passes)
    // Single decode (k_huff_emit): a column holds a subsequence's entries AND a word per block, sized for sub_bits / 2 + 2 words --
    // every entry takes two bits at least and every block two more (a DC code and an end-of-block).  A block can end without an
    // end-of-block: after 63 coded coefficients, or -- in a stream that is corrupt, or decoded from a wrong state, where runs are
    // clamped -- after four symbols of run 15.  With a 1-bit DC code and 2-bit entries (a 1-bit code for an AC symbol of size 1)
    // that is 64 words in 127 bits, or 5 words in 9 bits, and the entries would run into the block words; with any longer DC code
    // or entry a block of j entries takes 2 j + 2 bits at least.  false: the tables are of that kind; the picture takes the
    // two-pass kernels, in this batch and in every batch tiled from it.
    bool emit_fits = true;
    float qmult[4][64];                            // per component, zig-zag order: q[k] * idct prescale
    // scaled decode (mjx_opts.scale_denom): 1, 2, 4 or 8, the output size ceil(width / scale) x ceil(height / scale), and the
    // multipliers of the reduced transforms (zig-zag order: q[k] * C(u) C(v) / 4 inside the low N x N corner, 0 outside)
    uint32_t scale = 1, out_w = 0, out_h = 0;
    float qmult_scaled[4][64];
    // region-of-interest decode (mjx_opts.rois): the rectangle in the coordinates of the out_w x out_h picture -- the whole of it
    // without one -- and the MCU rows and columns that touch it.  The picture written is roi_w x roi_h.  A multi-scan file's
    // rectangle belongs to its role-2 plan, not to its scans.
    bool cropped = false;
    uint32_t roi_x = 0, roi_y = 0, roi_w = 0, roi_h = 0;
    uint32_t roi_mr0 = 0, roi_mr1 = 0, roi_mc0 = 0, roi_mc1 = 0;
    // output formats (mjx_output, plan_output): what the picture leaves as -- roi_w x roi_h elements per channel at these pitches (in
    // elements), in caller-owned memory at out_dev or, out_dev == 0, in the batch's pool; out_bytes: the span from the first element's
    // first byte to the last element's last.  Without a description (out_on false): packed R,G,B bytes, out_bytes = roi_w roi_h 3.
    bool out_on = false;
    uint32_t out_dtype = 0, out_planar = 0, out_bgr = 0;
    uint32_t out_channels = 3;                     // 1: luminance -- one element per pixel, rows of out_row_pitch, no planes (scale[0], bias[0])
    float out_scale[3] = {1.f, 1.f, 1.f}, out_bias[3] = {0.f, 0.f, 0.f};
    uint64_t out_dev = 0, out_row_pitch = 0, out_plane_pitch = 0, out_bytes = 0;
    // YCbCr output (mjx_planes, plan_planes): the picture leaves as its component planes.  out_on, out_dtype, out_scale / out_bias (by
    // COMPONENT), out_dev (plane 0's, 0: library-owned) and out_bytes (the span from plane 0's first byte to the last plane's end)
    // above are set as for any output description; plane c is ycc_w[c] x ycc_h[c] samples from (ycc_x0[c], ycc_y0[c]) of the
    // component's plane (plane_span of the rectangle), rows of ycc_pitch[c] elements at ycc_dev[c] or, library-owned, ycc_off[c]
    // bytes behind plane 0's first.  ycc_il: Cb and Cr share plane 1 as pairs.  ycc_round: libjpeg's pixels (rounded samples).
    // ycc_written: the bytes stage B writes (the pitches' padding not counted).
    bool ycc_on = false;
    uint32_t ycc_il = 0, ycc_round = 0;
    uint32_t ycc_x0[3] = {0, 0, 0}, ycc_y0[3] = {0, 0, 0}, ycc_w[3] = {0, 0, 0}, ycc_h[3] = {0, 0, 0};
    uint64_t ycc_dev[3] = {0, 0, 0}, ycc_off[3] = {0, 0, 0}, ycc_pitch[3] = {0, 0, 0}, ycc_written = 0;
    // YCbCr planes with an orientation and / or a resize (plan_input_for with a plane description; PlanePass, mjx_kernels.h).  yp_kind
    // != 0 (kPlaneCopy, kPlaneResize): ycc_* above, out_dtype (uint8) and out_bytes describe the INTERMEDIATE -- the plain plane decode
    // of the stored rectangle, library-owned, dense, not interleaved -- and the fields here the planes that LEAVE: plane k is yp_w[k] x
    // yp_h[k] samples of yp_dtype, rows of yp_pitch[k] elements at yp_dev[k] (caller-owned) or, yp_dev[k] == 0, yp_off[k] bytes behind
    // the first leaving plane; yp_il: Cb and Cr share plane 1.  yp_bytes: the span from the first leaving plane's first byte to the
    // last one's end; yp_written: the bytes written; yp_out_w x yp_out_h: the picture that leaves (D's rectangle, or the target).
    uint32_t yp_kind = 0, yp_code = 1, yp_il = 0, yp_dtype = 0, yp_filter = 0, yp_aa = 0;
    uint32_t yp_w[3] = {0, 0, 0}, yp_h[3] = {0, 0, 0}, yp_out_w = 0, yp_out_h = 0;
    uint64_t yp_dev[3] = {0, 0, 0}, yp_off[3] = {0, 0, 0}, yp_pitch[3] = {0, 0, 0}, yp_bytes = 0, yp_written = 0;
    float yp_scale[3] = {1.f, 1.f, 1.f}, yp_bias[3] = {0.f, 0.f, 0.f};
    // resize on the device (mjx_resize, plan_resize): the picture is planned as the packed (cropped) picture roi_w x roi_h at `scale`
    // -- the intermediate -- and leaves as rs_w x rs_h elements per channel: out_* above then describe the TARGET picture, and
    // stage B keeps its packed forms (fill_dev_image).
    bool rs_on = false;
    uint32_t rs_w = 0, rs_h = 0, rs_aa = 0;
    uint32_t rs_filter = 0;                // MJX_RESIZE_FILTER of the description: 0 triangle, 1 bicubic, 2 nearest
    // fit modes (MJX_RESIZE_FIT of the description, fit_rule): fit_w x fit_h is the picture that leaves -- rs_w x rs_h unless the mode
    // is MJX_FIT_CONTAIN, where rs_w x rs_h is the inner rectangle at (fit_ox, fit_oy) of the fit_w x fit_h target and out_* describe
    // the target.  pad: the three pad bytes of the output description, by OUTPUT channel (read for MJX_FIT_CONTAIN only).  MJX_FIT_COVER
    // only rewrites the rectangle the picture is planned with.  fit_ax .. fit_ah: the rectangle asked for (A' for MJX_FIT_COVER) in the
    // coordinates of the picture that leaves, as mjx_resize_fit_plan reports it.
    uint32_t fit_mode = 0, fit_w = 0, fit_h = 0, fit_ox = 0, fit_oy = 0;
    uint32_t fit_ax = 0, fit_ay = 0, fit_aw = 0, fit_ah = 0;
    uint8_t pad[3] = {0, 0, 0};
    // orientation on the device (mjx_orient, plan_input_for): orient = the EXIF code 2 .. 8 of a picture that leaves as orient_c(S), S
    // the packed intermediate as above (rs_on is set either way: the pool, the output's rules and the accessors are the resize's).
    // or_copy: there is no resize, rs_w x rs_h is the oriented size of roi_w x roi_h and k_orient_out copies.  Code 1 leaves no trace.
    uint32_t orient = 1;
    bool or_copy = false;
    // libjpeg's pixels (mjx_opts.pixels = MJX_PIXELS_LIBJPEG): stage B writes component planes and k_upsample_color makes the picture.
    // roi_m* above are then those of the rectangle grown by the upsampling filter's reach -- one sample of the most subsampled
    // component, hmax x vmax pixels, on each side, clipped to the picture: the tiles stage B must fill for the rectangle's pixels.
    bool lj = false;
    // ... with libjpeg's integer slow inverse DCT (MJX_OPTS_IDCT = MJX_IDCT_ISLOW; kSinkPlanesInt): qint holds the components' raw DQT
    // entries, zig-zag order, the table stage B multiplies by in place of qmult.  lj_rep: bit c -- component c's plane has at most two
    // columns and ratios (2, 1) or (2, 2), so jdsample.c replicates it (its downsampled_width > 2 condition); such a picture is
    // k_upsample_rep's.  Without the option both stay 0.
    // ... and a scale of 2, 4 or 8 (kSinkPlanesRed): red_n[c] is the size N_c of the transform libjpeg picks for component c (red_size,
    // mjx_kernels.h; 8 without a scale), its plane holds N_c samples per block side, and lj_rep is the same rule on the scaled plane and
    // the scaled ratios -- every component at 1/8.  Such a picture is k_upsample_red's.
    bool islow = false;
    uint32_t lj_rep = 0;
    uint8_t red_n[4] = {8, 8, 8, 8};
    uint32_t qint[4][64] = {};
    const uint8_t *scan = nullptr;
    size_t scan_len = 0;
    // The scan still holds FF00 pairs (and RSTn markers): it is de-stuffed on the device at upload (k_destuff_*), scan_len is
    // the stuffed length -- an upper bound; himg.total_bits, himg.nsub and the segment table are bounds and placeholders here,
    // the device writes the exact values into the DevImage (k_destuff_prefix, k_restart_geometry).
    bool stuffed = false;
    uint32_t wg_lanes = uint32_t(kHuffWg);         // lanes of the entropy workgroups the scan is cut for: 512, or 256 / 128 for a scan that fills no more
                                                   // (replan_subsequences; k_huff_spec / k_huff_write run a chunk at its pictures' largest)
    uint32_t nsub_layout = 0;                      // subsequences the scan pool region is laid out for (0: himg.nsub; a batch tiled from
                                                   // one that was de-stuffed on the device keeps the region of the bound)
    // REF_COMPAT placement (decoder.rs:239-250): replication factors per component, block grid of the image
    uint32_t ref_xf[3] = {1, 1, 1}, ref_yf[3] = {1, 1, 1};
    uint32_t nbx = 0, nby = 0;
    // Restart intervals: the scan is a sequence of independent segments of restart_mcus MCUs each.
    // seg[g] = (first subsequence, first bit) of segment g, plus a sentinel (nsub, total_bits).  One segment when the
    // image has no restart interval.
    uint32_t restart_mcus = 0;
    std::vector<uint32_t> seg;                     // 2 * (nseg + 1) words
    uint32_t nseg = 1;
    // Multi-scan files (one component per scan): every scan is planned as a one-component picture of
    // its own (role 1: entropy decode and DC prediction only, blocks in the component's raster order), the picture
    // itself as role 2 (no scan: its coefficient stream is gathered from the role-1 streams, then stage B as usual).
    uint32_t role = 0;
    uint32_t cbw[3] = {0, 0, 0}, cbh[3] = {0, 0, 0};   // role 2: the components' own block grids (T.81 A.2.2)
    uint32_t nparts = 0;                               // role 2: scans in front of the picture; role 1: scans of its file
    uint32_t part_idx = 0;                             // role 1: which of them this is (the picture's plan lies nparts - part_idx plans behind)
    uint32_t src_part[3] = {0, 0, 0}, src_comp[3] = {0, 0, 0};   // ... which of them carries component c, as its n-th component
    // Progressive pictures (MJX_OPTS_PROGRESSIVE): a role-2 picture with no plans in front of it (nparts = 0).  Its scans are decoded
    // serially, a lane per restart interval, level by level into a dense store and compacted into the stream stage B reads.  `lut`
    // holds the scans' distinct tables one behind the other, each as build_decode_table left it.
    bool prog = false;
    std::vector<ProgScanPlan> pscans;
    uint32_t prog_levels = 0;
    uint64_t prog_bytes = 0, prog_ac_bytes = 0;    // bytes of all scans / of the AC scans (a non-zero AC costs two bits of one at least)
};

// What stage B and the passes behind it do with a planned picture: DevImage's fields of the same names (mjx_kernels.h), decided
// here and nowhere else.  tile_420: the picture's tile is the 4:2:0 kernel's (tile_mcus_420) and not the generic power of two.
struct StageBChoice {
    uint32_t mode, rs_on, or_on, out_ch, lj_on, lj_luma, lj_out, lj_rep, lj_red;
    bool tile_420;
};
StageBChoice stage_b_choice(const ImagePlan &p);

// decoder.rs:259-288 get_indices: raster counter (x, y) of a component's blocks -> block position (bug-for-bug, Q3).
// Returns false where the reference's usize arithmetic underflows (panic).
bool ref_get_indices(long x, long y, long max_x, long x_factor, long y_factor, long max_x_factor, long max_y_factor,
                     long *ox, long *oy);

// Validates `d` and fills `plan`.  Returns plan.status.  `scan_part`: d is one scan of a multi-scan file (two interleaved
// components are then allowed; opts.rois is not looked at).  Otherwise the picture's rectangle is opts.rois[0] (n_rois <= 1).
int plan_image(const mjx_scan_desc &d, const mjx_opts &opts, ImagePlan &plan, bool scan_part = false);

// Re-cuts a planned picture's scan into subsequences of about `base_bits` bits (at most kSubseqBits; plan_image uses
// kSubseqBits).  Batches too small to fill the device are re-planned with shorter subsequences (mjx_api.hip).
void replan_subsequences(ImagePlan &plan, uint32_t base_bits, bool allow_long = true);     // allow_long: kLongSubseqBits for long scans (base_bits == kSubseqBits only)

// The plans of one input: `plan_image` for an ordinary file; for a multi-scan file one role-1 plan per scan (in file
// order) followed by the role-2 plan of the picture.  The last plan appended is the picture's.
void plan_input(const mjx_scan_desc &d, const mjx_opts &opts, std::vector<ImagePlan> &out);

// The options input i of a call of n inputs is planned with: opts with its own rectangle as rois[0] (n_rois 0 or 1).
// false: opts.rois / opts.n_rois do not fit a call of n inputs (MJX_ERR_INVALID_ARG for the call).
bool rois_fit(const mjx_opts &opts, size_t n);
mjx_opts opts_for_input(const mjx_opts &opts, size_t n, size_t i);

// Output formats: does out->dst / n_dst fit a call of n inputs (false: MJX_ERR_INVALID_ARG for the call)?  And the one place that
// knows the rules of a picture's output: plan_output gives the planned picture `p` (the last plan of input i) its format and
// destination -- the pitches of a dense library-owned picture, or dst[i]'s after checking them -- or fails it with
// MJX_ERR_INVALID_ARG.  out == nullptr: the packed picture.  mjx_output_layout reports what it finds here.
bool output_fits(const mjx_output *out, size_t n);
int plan_output(ImagePlan &p, const mjx_output *out, size_t i);
// ... applied to the plans of one input as plan_input left them (the last is the picture's): a multi-scan picture that is refused
// takes its scans' plans with it, so that nothing of the file is uploaded or decoded.
int plan_output_of_input(std::vector<ImagePlan> &plans, const mjx_output *out, size_t i);

// YCbCr output: does pl->dst / n_dst fit a call of n inputs, and the one place that knows the rules of a picture's planes -- sizes
// (plane_span, mjx_kernels.h), offsets of dense library-owned planes or dst[i]'s pointers and pitches after checking them -- or fails
// the picture with MJX_ERR_INVALID_ARG.  mjx_planes_layout reports what it finds here.  plan_planes_of_input: as plan_output_of_input.
bool planes_fit(const mjx_planes *pl, size_t n);
int plan_planes(ImagePlan &p, const mjx_planes *pl, size_t i);
int plan_planes_of_input(std::vector<ImagePlan> &plans, const mjx_planes *pl, size_t i);

// Resize on the device.  resize_opts: the options input i is planned with under `rs` -- the call's own (auto_scale 0), or the scale
// and the rectangle at that scale the auto-scale rule picks for a picture of width x height (`rect` is the storage the options
// returned point at).  MJX_ERR_INVALID_ARG: a target of 0 (or above kResizeMaxDim), auto_scale with scale_denom > 1, REF_COMPAT, a
// full-size rectangle outside the picture.  plan_resize marks the planned picture (the last plan of the input).
// plan_input_for: plan_input + plan_resize + plan_output_of_input in the one order every entry point uses; rs == nullptr: as before.
// A resize without an output description leaves interleaved u8 R,G,B, library-owned.
// code: the picture's resolved orientation (mjx_orient), an EXIF code.  1: as before.  2 .. 8: rois[0] is in the coordinates of the
// oriented picture D (full-size D with auto_scale), is mapped back to the stored picture S (orient_rect_to_stored) and the picture
// is planned as the cropped packed picture there; with auto_scale the target's axes are swapped into S's for codes 5 .. 8 before the
// scale is picked.  Anything else, a rectangle outside D, or REF_COMPAT: MJX_ERR_INVALID_ARG for the picture.
// pl: the call's plane description (`out` is then not looked at).  Without a resize and with code 1 the picture is planned exactly as
// mjx_batch_create_planes plans it (plan_input + plan_planes_of_input).  Otherwise the rectangle, the orientation mapping, the fit
// rule and the scale are the ones above, the picture is planned as the plain uint8 plane decode at (s, R_S) -- the intermediate --
// and the leaving planes (ImagePlan::yp_*) are laid out by pl's rules; MJX_FIT_CONTAIN is MJX_ERR_INVALID_ARG for the picture.
int resize_opts(uint32_t width, uint32_t height, const mjx_opts &opts_i, const mjx_resize &rs, mjx_opts &eff, mjx_rect &rect);
void plan_input_for(const mjx_scan_desc &d, const mjx_opts &opts_i, const mjx_output *out, const mjx_resize *rs, size_t i,
                    std::vector<ImagePlan> &plans, uint32_t code = 1, const mjx_planes *pl = nullptr);

// A planned progressive picture as the device sees it (mjx_prog.h): its ProgPic, planes laid out from element `store0` of the chunk's
// dense store on; its scans' bytes appended to `bytes`; one lane per (scan, restart interval) appended to levels[level - 1], for image
// `img` of the chunk and entry `pic_index` of the picture array.  Returns the first store element behind the picture.  The batch
// (mjx_api.hip) and the host emulation (tests/emul/prog_emul.cpp) both lay a picture out here.
struct ProgPic;
struct ProgLane;
// bytes_at: null, or where the scans' bytes lie -- *bytes_at == kProgAppend appends them and notes the place, any other value says
// that they are at that offset of `bytes` already (the copies of one picture in a tiled batch share one copy of its scans).
constexpr uint64_t kProgAppend = ~uint64_t(0);
uint64_t prog_layout(const ImagePlan &p, uint64_t store0, uint32_t img, uint32_t pic_index, ProgPic &pic,
                     std::vector<std::vector<ProgLane>> &levels, std::vector<uint8_t> &bytes, uint64_t *bytes_at = nullptr);

// mjx_parse.cpp: mjx_parse with caller-lent storage for the de-stuffed scan (see there)
int parse_into(const uint8_t *jpeg, size_t len, const mjx_opts *opts, mjx_scan_desc *out, uint8_t *storage, size_t cap);

extern const uint8_t kZigZag[64];                  // decoder.rs:404-407 ZIGZAG_INDICES

}   // namespace mjx
#endif

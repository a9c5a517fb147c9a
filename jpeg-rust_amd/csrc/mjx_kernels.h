// mjx_kernels.h -- device-side data layout shared by the kernel file and the host API.
#ifndef MJX_KERNELS_H
#define MJX_KERNELS_H

#include "mjx_huff.h"

#include <stddef.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define MJX_UNROLL _Pragma("unroll")
#else
#define MJX_UNROLL
#endif

namespace mjx {

constexpr int kWgLanes = 256;                                   // lanes of the scan / prefix-sum workgroups
constexpr int kDcSegMcus = 2048;                                // MCUs per DC-prediction segment (k_dc_sums / k_dc_apply)
constexpr uint32_t kPlanarKinds = 4, kPlanarSegs = 8;           // multi-scan pictures read without the gather: segment kinds per piece, segments per tile

// One image of a chunk, as the kernels see it (HBM, read-only during decode).
struct DevImage {
    HuffImage himg;
    uint64_t scan_off;      // bytes into the scan pool (256-byte aligned): the image's lane-interleaved region, see LaneBits
    uint64_t coef_off;      // blocks into the per-block arrays (dcbuf)
    uint64_t ent_off;       // entries into the compact coefficient stream pool (start of the image's region)
    uint64_t rgb_off;       // bytes into the RGB pool
    uint32_t scan_cols;     // columns of the region = subsequences rounded up to 8 (a row = scan_cols 16-byte pieces);
                            // rows = sub_bits / 128 + kLookPieces
    uint32_t lut_off;       // entries into the decode-table pool (multiple of 4): the plain table set (write pass)
    uint32_t lut_n;         // entries (multiple of 4)
    uint32_t lut2_off, lut2_n;   // the set with pair parts (counting passes: k_huff_spec, merge rounds), HuffImage::tabs_pair
    uint32_t sub_off;       // index of subsequence 0 in the per-subsequence arrays
    uint32_t qm_off;        // floats into the dequant-multiplier pool (3 x 64 per image; a fourth component's: qm3_off)
    uint32_t width, height, mcux, mcuy, nmcu;
    uint32_t ncomp, bpm, hmax, vmax;
    uint32_t valid;         // 0: skip (error at plan time)
    uint32_t status_idx;    // index into the batch-wide device status array
    uint32_t log2_tile;     // stage-B tile = 1 << log2_tile MCUs (kForm420: floor(log2(tile_mcus)), unused)
    uint32_t tile_mcus;     // MCUs per stage-B tile (kForm420: tile_mcus_420(), which need not be a power of two)
    uint32_t mode;          // stage-B specialisation: stage_b_mode(form, sink) = form | sink << 3 (StageBForm, StageBSink below) -- what
                            // stage B computes and how the picture leaves it.  Every kernel form compares the whole number, so the
                            // forms of one sink leave the pictures of every other alone.
    uint32_t tile_off;      // index of the image's first tile offset in the tile_eoff array
    uint32_t tile_blocks;   // blocks per stage-B tile = tile_mcus * bpm  (<= 256)
    uint8_t blk_comp[kMaxBlocksPerMcu], blk_bx[kMaxBlocksPerMcu], blk_by[kMaxBlocksPerMcu];
    uint8_t ch[4], cv[4];   // sampling factors per component
    uint8_t cfirst[4];      // first block position of each component inside the MCU
    // REF_COMPAT layout only (kFormRefCompat): decoder.rs:239-250 replication factors, block grid, f32 plane scratch
    uint8_t ref_xf[4], ref_yf[4];
    uint32_t nbx, nby;
    uint64_t plane_off;     // 64-bit words into the plane scratch (ncomp planes of width*height words)
    // restart intervals: nseg segments of restart_mcus MCUs; (first subsequence, first bit) pairs + sentinel at seg_off
    uint32_t seg_off;       // index (in pairs) into the segment pool
    uint32_t nseg;          // 1 = no restart interval
    uint32_t restart_mcus;
    uint32_t ent_cap;       // entries the image's stream region holds
    uint32_t ent_rows;      // 0: the stream is linear, the lanes' runs packed behind one another (multi-scan pictures and their scans).
                            // > 0: quad-interleaved columns (see stream_phys): rows of 32 bytes every lane's column holds
    uint32_t ent_hdr;       // quad-interleaved: entries (4-byte words) at the head of the region that hold the subsequences' run
                            // lengths in groups, 16 bits each (stream_hdr_entries); the columns follow
    uint32_t n_rst_found;   // scans de-stuffed on the device: RSTn markers found (k_destuff_prefix)
    uint32_t upload_short;  // ... and their diagnosis at upload (a scan of nothing but stuffing, fewer RSTn markers than intervals): the
                            // picture is truncated whatever the block counts of a later decode say (k_huff_scan ORs it in)
    // multi-scan files: role 1 = one scan as a picture of its own (one component in raster order, or two
    // interleaved; entropy stage only; tile = one block, so tile_eoff holds an offset per block -- or, seg_S != 0, where the picture's
    // tile segments begin, see below), role 2 = the picture
    // (no scan; the k_planar_* kernels build its stream from the role-1 images: component c comes from the image
    // src_back[c] places before it in the image array, as that image's src_comp[c]-th component)
    uint32_t role;
    uint32_t src_back[3], src_comp[3];
    uint32_t wg_lanes;          // lanes of the entropy workgroups this scan was cut for (ImagePlan::wg_lanes; the chunk runs at its pictures' largest)
    uint32_t nparts;            // (role 1 as well: the scans of its file, of which it is the part_idx-th)
    uint32_t part_idx;
    uint32_t cbw[3], cbh[3];    // role 2: block grid of each component's own scan
    // Multi-scan pictures WITHOUT the gather (round 5, `planar`): stage B reads a tile's entries straight out of the scans' streams.
    // A tile of the picture is, in every scan, a few runs of consecutive blocks -- per MCU row the tile touches ("piece") and per
    // block row of the component inside the MCU row: a SEGMENT.  The write pass of a scan (role 1, seg_S != 0) records where every
    // segment's entries begin instead of an offset per block: a cut lies at every scan-MCU-row start and wherever a tile of the
    // picture begins (planar_cut); the table has seg_S slots per scan-MCU row (slot k = the k-th tile boundary inside the row).
    //   role 1: seg_S, seg_T (the picture's MCUs per tile), seg_mcux (the picture's MCUs per row), seg_hs / seg_vs (scan MCUs per
    //           picture MCU: the component's sampling factors for a one-component scan, 1 for an interleaved subset)
    //   role 2: planar = 1; pk_n kinds of segments per piece, per kind: the scan (pk_back images before the picture), its block
    //           row inside the MCU row (pk_v of pk_vs), scan MCUs per picture MCU (pk_hs), blocks of the segment per picture MCU
    //           (pk_u) and where these land in the picture's MCU (pk_map)
    uint32_t planar;
    uint32_t seg_S, seg_T, seg_mcux, seg_hs, seg_vs;
    uint8_t pk_n, pk_back[kPlanarKinds], pk_v[kPlanarKinds], pk_vs[kPlanarKinds], pk_hs[kPlanarKinds], pk_u[kPlanarKinds];
    uint8_t pk_map[kPlanarKinds][kMaxBlocksPerMcu];
    // single decode (round 5): 1 = the picture's first decode emits (k_huff_emit, then k_huff_prefix + k_block_gather instead of
    // k_huff_spec ... k_huff_write): pictures of one scan without restart intervals, quad-interleaved stream
    uint32_t emit;
    uint32_t emit_head;         // groups of head room in front of the first decode's entries (kEmitHeadGroups; tests shrink it)
    // scaled decode (mjx_opts.scale_denom): 1, 2, 4 or 8; the picture written is out_w x out_h = ceil(width / scale) x
    // ceil(height / scale).  kFormHalf and kFormQuarter run k_idct_color with a 4- or 2-point inverse DCT on the low corner of
    // each block, kFormEighth runs k_dc_color on the DC values alone; qm_off then points at the reduced multipliers.
    uint32_t scale, out_w, out_h;
    // region-of-interest decode (mjx_opts.rois; kSinkCropped and every sink above it): the rectangle in the coordinates of the out_w x out_h picture
    // -- the picture written is roi_w x roi_h, rgb_off its first byte --, the MCU rows and columns that touch it, and the tiles
    // that can: roi_ntiles tiles from roi_tile0 on hold the MCU rows roi_mr0 .. roi_mr1 (roi_tile_wanted says which of them also
    // hold one of the columns).  Without a rectangle: 0, 0, out_w, out_h and all the picture's tiles.
    uint32_t roi_x, roi_y, roi_w, roi_h;
    uint32_t roi_mr0, roi_mr1, roi_mc0, roi_mc1;
    uint32_t roi_tile0, roi_ntiles;
    // output formats (mjx_output; kSinkOut): the picture leaves as 3 x H x W or H x W x 3 elements of u8 / f16 / f32 in the
    // channel order asked for, a float element as fmaf(float(u8), out_scale[c], out_bias[c]) with c the OUTPUT channel.  The first
    // element lies at out_dev (caller-owned memory) or, out_dev == 0, at byte rgb_off of the batch's picture pool; pitches count
    // elements.  Such a picture is its own whole rectangle unless it has one (roi_* above say which either way).
    uint64_t out_dev;
    uint64_t out_row_pitch, out_plane_pitch;
    uint32_t out_dtype, out_planar, out_bgr;
    float out_scale[3], out_bias[3];
    // resize on the device (mjx_resize; rs_on): stage B writes the picture as a packed (cropped) one -- roi_w x roi_h x 3 bytes at
    // rgb_off, kSinkPacked or kSinkCropped -- and k_resize_out resamples that to rs_w x rs_h elements per channel in the format out_* above
    // describe, at out_dev or, out_dev == 0, at byte rs_off of the batch's picture pool.
    // rs_filter: the filter kind (MJX_RESIZE_FILTER: 0 triangle, 1 bicubic, 2 nearest), also of k_resize_orient's and k_resize_luma's pictures
    uint32_t rs_on, rs_w, rs_h, rs_aa;
    uint64_t rs_off;
    uint32_t rs_filter;
    // orientation on the device (mjx_orient; or_on): the picture that leaves is orient_c(S), S the packed intermediate above, c =
    // orient (an EXIF code 2 .. 8; a picture whose code is 1 has or_on = kOrNone and is planned as if there were no orientation).
    // kOrCopy: k_orient_out copies S to rs_w x rs_h = the oriented size, element by element through the formats' table, to out_dev
    // or byte rs_off of the pool; kOrResize: k_resize_orient resamples orient_c(S) to rs_w x rs_h (rs_on stays 0: k_resize_out
    // passes over the picture).
    uint32_t orient, or_on;
    // libjpeg's pixels (mjx_opts.pixels = MJX_PIXELS_LIBJPEG; lj_on, kSinkPlanes): stage B stores the rounded samples of component c
    // as a uint8 plane over the whole MCU grid -- rows of lj_stride[c] = mcux * 8 * ch[c] bytes, mcuy * 8 * cv[c] of them -- at byte
    // plane_off * 8 + lj_off[c] of the chunk's plane scratch, and k_upsample_color makes the picture of them: the packed picture at
    // rgb_off (what a resize or an orientation then works on) or, lj_out = 1, the output format out_* describe.  roi_m* and
    // roi_tile* are those of the rectangle grown by the filter's reach.
    uint32_t lj_on, lj_out;
    uint32_t lj_stride[3];
    uint64_t lj_off[3];
    // luminance output (MJX_OUTPUT_CHANNELS == 1; out_ch = 1, kSinkLuma): the picture leaves as roi_w x roi_h elements, one per
    // pixel, rows of out_row_pitch elements at out_dev or byte rgb_off of the pool, a float element as fmaf(float(L), out_scale[0],
    // out_bias[0]).  Stage B transforms the luminance blocks only.  A resized or oriented luminance picture has rs_on = 0 and or_on = kOrCopyLuma
    // (k_orient_luma copies) or kOrResizeLuma (k_resize_luma resamples orient_c(S), c = 1 included): stage B then writes S as roi_w x roi_h BYTES at
    // rgb_off, and the three-channel passes leave the picture alone.  With libjpeg's pixels lj_on stays 0 and lj_luma = 1: stage B's
    // plane form as it is, k_upsample_luma reads component 0's plane.
    uint32_t out_ch, lj_luma;
    // YCbCr output (mjx_planes; ycc_on, kSinkYcc): the picture leaves as its component planes at their own sampling.  Plane c
    // is the ycc_w[c] x ycc_h[c] samples from (ycc_x0[c], ycc_y0[c]) of component c's plane at the picture's scale (plane_span of the
    // rectangle roi_*), rows of ycc_pitch[c] elements of out_dtype at ycc_dev[c] (caller-owned memory) or, ycc_dev[c] == 0, at byte
    // rgb_off + ycc_off[c] of the batch's pool; a float element is fmaf(float(u8), out_scale[c], out_bias[c]), c the COMPONENT.
    // ycc_il = 1: Cb and Cr share plane 1, element (X, Y) as the pair Cb, Cr at Y ycc_pitch[1] + 2 X (ycc_dev[2] / ycc_off[2] are
    // not used).  ycc_round = 1 (libjpeg's pixels): the sample is rounded, not truncated.
    uint32_t ycc_on, ycc_il, ycc_round;
    uint32_t ycc_x0[3], ycc_y0[3], ycc_w[3], ycc_h[3];
    uint64_t ycc_dev[3], ycc_off[3], ycc_pitch[3];
    // colour models (mjx_opts.color = MJX_COLOR_FILE; ColorModel below).  model: what the pixel phase does with the components' samples;
    // 0 (kModelPositional) is the decode of every picture planned without the option: one component grey, three Y, Cb, Cr.
    // qm3_off: floats into the dequant-multiplier pool of the FOURTH component's 64 multipliers (components 0 .. 2 stay at qm_off).
    // dc_shape: what the DC-prediction kernels choose by -- bpm for a picture of up to three components, kDcShape4 + bpm for one of
    // four, which so never takes a kernel that carries three running sums.
    uint32_t model, qm3_off, dc_shape;
    // fit modes (mjx_resize's fit byte).  MJX_FIT_COVER leaves no trace: its rectangle is the planner's.  MJX_FIT_CONTAIN: the picture
    // that leaves is fit_w x fit_h elements per channel at the pitches above; the resize pass writes its rs_w x rs_h into the inner
    // rectangle at (fit_ox, fit_oy) -- out_dev and rs_off above are already moved there by fit_oy rows and fit_ox pixels -- and,
    // fit_on = 1 (there is a border), k_fit_pad writes every other element: the format's table applied to fit_pad's byte c
    // (bits 8 c .. 8 c + 7, c the OUTPUT channel).  Without the mode fit_w x fit_h = rs_w x rs_h, the origin is 0 and fit_on = 0.
    uint32_t fit_on, fit_w, fit_h, fit_ox, fit_oy, fit_pad;
    // progressive pictures (MJX_OPTS_PROGRESSIVE; prog = 1): a role-2 picture with no scans in front of it.  k_prog_scan's lanes fill
    // the chunk's dense store, k_prog_count / _offsets / _copy build the stream from it (the k_planar_* kernels pass over the picture);
    // prog_pic: its ProgPic (mjx_prog.h) in the batch's array.
    uint32_t prog, prog_pic;
    // libjpeg's integer inverse DCT (MJX_OPTS_IDCT = MJX_IDCT_ISLOW; kSinkPlanesInt): stage B's planes hold clamp(x + 128, 0, 255) of the
    // integer transform, and qm_off points at the components' raw DQT entries (uint32, zig-zag order, 64 each) in the multiplier pool.
    // lj_rep != 0: a picture with a component of at most two columns and ratios (2, 1) or (2, 2), which jdsample.c replicates --
    // kLjRepOn | bit c per replicated component | kLjRepLuma for a luminance picture.  Such a picture has lj_on = lj_luma = 0 and is
    // k_upsample_rep's; lj_out says where it leaves as for k_upsample_color.
    uint32_t lj_rep;
    // ... at a reduced scale (scale 2, 4 or 8 with MJX_IDCT_ISLOW; kSinkPlanesRed): libjpeg picks a transform size N_c per component
    // (jdmaster.c; red_size below), so component c's plane holds N_c samples per block side -- rows of lj_stride[c] bytes (mcux * N_c * ch[c]
    // rounded up to 8), mcuy * N_c * cv[c] of them -- and is upsampled by (hmax m / (ch N_c), vmax m / (cv N_c)), m = 8 / scale.  lj_red != 0:
    // kLjRedOn | kLjRedLuma for a luminance picture | per component c, from bit 4 c on: log2 N_c in two bits and the replicate bit (a
    // narrow plane as lj_rep; every component at 1/8).  Such a picture has lj_on = lj_luma = lj_rep = 0 and is k_upsample_red's.
    uint32_t lj_red;
};
constexpr uint32_t kLjRepOn = 16u, kLjRepLuma = 32u;
constexpr uint32_t kLjRedOn = 1u << 31, kLjRedLuma = 1u << 30;
MJX_HD constexpr uint32_t lj_red_n(uint32_t word, uint32_t c) { return 1u << (word >> (4u * c) & 3u); }
MJX_HD constexpr uint32_t lj_red_rep(uint32_t word, uint32_t c) { return word >> (4u * c + 2u) & 1u; }
// Component (hc, vc) of maxima (hmax, vmax) in a W x H picture at scale 8 / m with a transform of size n: its plane's samples and its
// upsampling ratios.  The planner and mjx_plan_reduced run this routine; k_upsample_red states the same arithmetic on the descriptor.
struct RedPlane { uint32_t cw, ch, rh, rv; };
MJX_HD constexpr RedPlane red_plane(uint32_t W, uint32_t H, uint32_t hc, uint32_t vc, uint32_t hmax, uint32_t vmax, uint32_t m, uint32_t n)
{
    return RedPlane{(W * hc * n + hmax * 8u - 1u) / (hmax * 8u), (H * vc * n + vmax * 8u - 1u) / (vmax * 8u), hmax * m / (hc * n), vmax * m / (vc * n)};
}
// jdmaster.c's rule for the transform size of a component with factors (hc, vc) of maxima (hmax, vmax) at scale 8 / m: from m, doubled
// while it stays below 8 and the doubled size still divides the MCU's scaled extent in BOTH directions -- one size for both.
MJX_HD constexpr uint32_t red_size(uint32_t m, uint32_t hc, uint32_t vc, uint32_t hmax, uint32_t vmax)
{
    uint32_t n = m;
    while (n < 8u && (hmax * m) % (hc * n * 2u) == 0u && (vmax * m) % (vc * n * 2u) == 0u) n *= 2u;
    return n;
}
// DevImage::model
enum ColorModel : uint32_t {
    kModelPositional = 0,   // grey, or Y, Cb, Cr by position: the pixel phase as it has always been
    kModelRgb = 2,          // three components stored as R, G, B: no arithmetic
    kModelCmyk = 3,         // four components, Adobe's convention: R,G,B = ink_mul(s_c, s_3)
    kModelYcck = 4,         // the colour step on components 0 .. 2, its bytes complemented (C = 255 - R), then ink_mul with s_3
};
constexpr uint32_t kDcShape4 = 16;       // DevImage::dc_shape of a four-component picture = kDcShape4 + bpm (bpm <= 10)
// mul(a, k) of mjx_opts.color: (a k + 127) / 255 in integers -- the host (mjx_ink_mul) and the pixel phase run this routine; the
// division by a constant is a multiplication and a shift, exact for every a, k < 256.
MJX_HD uint32_t ink_mul(uint32_t a, uint32_t k) { return (a * k + 127u) / 255u; }
// DevImage::mode.  The form: what stage B computes per tile.
enum StageBForm : uint32_t {
    kFormGeneric = 0,       // any sampling layout
    kForm420 = 1,           // Y 2x2, Cb 1x1, Cr 1x1 on the 4:2:0 kernel's own tile (tile_mcus_420)
    kFormRefCompat = 2,     // any sampling layout, REF_COMPAT placement into the plane scratch (k_ref_color finishes the picture)
    kFormHalf = 3,          // scaled decode at 1/2: the 4-point transform on each block's low corner
    kFormQuarter = 4,       // ... at 1/4: the 2-point transform
    kFormEighth = 5,        // ... at 1/8: the DC values alone (the k_dc_color* kernels, not k_idct_color)
    kFormScan = 7,          // a scan of a multi-scan file (role 1): no stage B
};
// The sink: how the picture leaves stage B.  Every sink but kSinkPacked walks the tiles of the picture's rectangle only.
enum StageBSink : uint32_t {
    kSinkPacked = 0,        // the whole picture, packed R,G,B bytes
    kSinkCropped = 1,       // the rectangle's pixels, packed R,G,B bytes (also the intermediate of a resize or an orientation)
    kSinkOut = 2,           // the picture's output description (DevImage::out_*)
    kSinkPlanes = 3,        // libjpeg's pixels: rounded component planes in the chunk's scratch, kFormGeneric only (k_upsample_color follows)
    kSinkLuma = 4,          // luminance: component 0 alone, one element per pixel
    kSinkYcc = 5,           // YCbCr output: the component planes as the picture (4:2:0 takes kFormGeneric)
    kSinkPlanesInt = 6,     // libjpeg's pixels with its integer inverse DCT (MJX_IDCT_ISLOW): kSinkPlanes on an int32 tile, kFormGeneric only
    kSinkPlanesRed = 7,     // ... at scale 2, 4 or 8: libjpeg's reduced integer transforms, a size per component (k_upsample_red follows), kFormGeneric only
};
constexpr uint32_t kStageBSinks = 8;
MJX_HD constexpr uint32_t stage_b_mode(uint32_t form, uint32_t sink) { return form | sink << 3; }
MJX_HD constexpr StageBForm form_of(uint32_t mode) { return StageBForm(mode & 7u); }
MJX_HD constexpr StageBSink sink_of(uint32_t mode) { return StageBSink(mode >> 3); }

// Every instantiation of k_idct_color, in the order launch_idct_color launches them: X(form, sink, PF, SRC, layout bit, density).
// PF / SRC: the kernel's prefetch depth and stream source (0 linear, 1 quad-interleaved, 2 the scans of a multi-scan picture); layout
// bit: the bit of a chunk's layout_mask that holds pictures of that source; density: which of a chunk's two kinds of linear stream
// the instantiation is for (kAnyDensity: both).  configure_kernels and launch_idct_color are generated from this list and nothing
// else names an instantiation: a mode that is not here has no kernel.
enum StageBDensity : uint32_t { kAnyDensity = 0, kSparse = 1, kDense = 2 };
#define MJX_STAGE_B_SOURCES(X, F, S) X(F, S, kPrefetch, 0, 1u, kAnyDensity) X(F, S, 8, 1, 2u, kAnyDensity) X(F, S, 8, 2, 4u, kAnyDensity)
#define MJX_STAGE_B_KERNELS(X)                                                                                                       \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkPacked)                                                                                \
    X(kForm420, kSinkPacked, kPrefetchDense, 0, 1u, kDense) X(kForm420, kSinkPacked, kPrefetch, 0, 1u, kSparse)                      \
    X(kForm420, kSinkPacked, 16, 1, 2u, kDense) X(kForm420, kSinkPacked, 8, 1, 2u, kSparse) X(kForm420, kSinkPacked, 8, 2, 4u, kAnyDensity) \
    X(kFormRefCompat, kSinkPacked, kPrefetch, 0, 1u, kAnyDensity) X(kFormRefCompat, kSinkPacked, 8, 1, 2u, kAnyDensity)              \
    MJX_STAGE_B_SOURCES(X, kFormHalf, kSinkPacked) MJX_STAGE_B_SOURCES(X, kFormQuarter, kSinkPacked)                                 \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkCropped) MJX_STAGE_B_SOURCES(X, kForm420, kSinkCropped)                                \
    MJX_STAGE_B_SOURCES(X, kFormHalf, kSinkCropped) MJX_STAGE_B_SOURCES(X, kFormQuarter, kSinkCropped)                               \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkOut) MJX_STAGE_B_SOURCES(X, kForm420, kSinkOut)                                        \
    MJX_STAGE_B_SOURCES(X, kFormHalf, kSinkOut) MJX_STAGE_B_SOURCES(X, kFormQuarter, kSinkOut)                                       \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkPlanes)                                                                                \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkLuma) MJX_STAGE_B_SOURCES(X, kForm420, kSinkLuma)                                      \
    MJX_STAGE_B_SOURCES(X, kFormHalf, kSinkLuma) MJX_STAGE_B_SOURCES(X, kFormQuarter, kSinkLuma)                                     \
    MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkYcc) MJX_STAGE_B_SOURCES(X, kFormHalf, kSinkYcc) MJX_STAGE_B_SOURCES(X, kFormQuarter, kSinkYcc)
// The forms of the integer inverse DCT (MJX_IDCT_ISLOW): a list of their own behind the one above, which stays what it was -- the
// modes stage_b_choice gave before the option existed.  MJX_STAGE_B_ALL is what configure_kernels and launch_idct_color are generated from.
#define MJX_STAGE_B_KERNELS_ISLOW(X) MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkPlanesInt)
// ... and of its reduced transforms (MJX_IDCT_ISLOW with a scale): again a list of their own, so that neither count above moves.
#define MJX_STAGE_B_KERNELS_ISLOW_RED(X) MJX_STAGE_B_SOURCES(X, kFormGeneric, kSinkPlanesRed)
#define MJX_STAGE_B_ALL(X) MJX_STAGE_B_KERNELS(X) MJX_STAGE_B_KERNELS_ISLOW(X) MJX_STAGE_B_KERNELS_ISLOW_RED(X)
#define MJX_STAGE_B_COUNT(F, S, PF, SRC, LAYOUT, DENSITY) +1
static_assert(0 MJX_STAGE_B_KERNELS(MJX_STAGE_B_COUNT) == 64, "16 packed kernels + 48 of the other sinks (DESIGN.md s3.2)");
static_assert(0 MJX_STAGE_B_KERNELS_ISLOW(MJX_STAGE_B_COUNT) == 3, "the integer inverse DCT: the generic form on the three stream sources");
static_assert(0 MJX_STAGE_B_KERNELS_ISLOW_RED(MJX_STAGE_B_COUNT) == 3, "the reduced integer transforms: one form for 1/2, 1/4 and 1/8 on the three stream sources");
#undef MJX_STAGE_B_COUNT

// DevImage::or_on: the pass behind stage B that brings an oriented (or resized, one-channel) picture to the form it leaves in
enum OrientPass : uint32_t {
    kOrNone = 0,
    kOrCopy = 1,            // k_orient_out copies the packed intermediate
    kOrResize = 2,          // k_resize_orient resamples it
    kOrCopyLuma = 3,        // k_orient_luma: the one-byte intermediate of a luminance picture
    kOrResizeLuma = 4,      // k_resize_luma (any orientation code, 1 included)
};

// Sampling factors: 1, 2 or 4 in each direction (include/mjx.h).  Strips per MCU row, lane -> (MCU, strip) and the replication of a
// subsampled component are all shifts, so a factor -- and with it every ratio hmax / h_c -- is a power of two; ratio_shift is its
// log2, 0, 1 or 2 (hmax a multiple of hc: the planner checks).
MJX_HD constexpr bool sampling_factor_ok(uint32_t f) { return f == 1u || f == 2u || f == 4u; }
MJX_HD constexpr uint32_t ratio_shift(uint32_t fmax, uint32_t fc) { return fmax >= 4u * fc ? 2u : fmax >= 2u * fc ? 1u : 0u; }

// YCbCr output: the samples of component c -- factors (hc, vc) of maxima (hmax, vmax) -- that the rectangle (x, y, w, h) of the
// out_w x out_h picture covers: columns floor(x hc / hmax) .. ceil((x + w) hc / hmax), rows likewise.  These are the samples the
// packed decode of the rectangle reads from the component (box replication: pixel X takes sample floor(X hc / hmax)); the whole
// picture's plane is ceil(out_w hc / hmax) x ceil(out_h vc / vmax).  The planner (plan_planes) and k_dc_color_ycc run this routine;
// stage B's plane forms clip to what the planner put into DevImage::ycc_* with it.
struct PlaneSpan { uint32_t x0, y0, w, h; };
MJX_HD PlaneSpan plane_span(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t hc, uint32_t vc, uint32_t hmax, uint32_t vmax)
{
    PlaneSpan s;
    s.x0 = x * hc / hmax;
    s.y0 = y * vc / vmax;
    s.w = ((x + w) * hc + hmax - 1u) / hmax - s.x0;
    s.h = ((y + h) * vc + vmax - 1u) / vmax - s.y0;
    return s;
}

// Region-of-interest decode: does tile t -- T consecutive MCUs in raster order, so it may wrap into the next MCU row -- hold an MCU
// of the MCU rows r0 .. r1 and the MCU columns c0 .. c1?  Arithmetic on uniform values only: stage B decides per tile without a
// memory access, and the host counts with the same rule (mjx_plan_tiles).
MJX_HD bool roi_tile_wanted(uint32_t t, uint32_t T, uint32_t nmcu, uint32_t mcux, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1)
{
    const uint32_t m_lo = t * T, m_end = m_lo + T < nmcu ? m_lo + T : nmcu, m_hi = m_end - 1u;
    const uint32_t ra = m_lo / mcux, ca = m_lo - ra * mcux, rb = m_hi / mcux, cb = m_hi - rb * mcux;
    const uint32_t rs = ra > r0 ? ra : r0, re = rb < r1 ? rb : r1;
    if (rs > re) return false;
    if (re > rs + 1u) return true;                                 // (a row strictly between the tile's first and last: all its columns)
    const bool first = (rs == ra ? ca : 0u) <= c1 && (rs == rb ? cb : mcux - 1u) >= c0;
    const bool last = (re == ra ? ca : 0u) <= c1 && (re == rb ? cb : mcux - 1u) >= c0;
    return first || last;
}

// ---- orientation (mjx_orient): the eight EXIF codes ------------------------------------------------------------------------------
// S is the stored picture, h rows of w; D = orient_c(S) is the picture that leaves.  Every code is "swap the axes or not, then mirror
// S's columns and / or rows":  D(x, y) = S[v][u],  u = (T ? y : x) mirrored in w when FU,  v = (T ? x : y) mirrored in h when FV
//   code  1      2      3      4      5      6      7      8
//   T     .      .      .      .      x      x      x      x
//   FU    .      x      x      .      .      .      x      x
//   FV    .      .      x      x      .      x      x      .
// The host (plan, mjx_orient_plan), k_orient_out and k_resize_orient run these routines.
MJX_HD bool orient_valid(uint32_t c) { return c >= 1u && c <= 8u; }
MJX_HD bool orient_swaps(uint32_t c) { return c >= 5u; }
MJX_HD bool orient_flips_u(uint32_t c) { return c == 2u || c == 3u || c == 7u || c == 8u; }
MJX_HD bool orient_flips_v(uint32_t c) { return c == 3u || c == 4u || c == 6u || c == 7u; }
// D's size and, in pixels of the row-major w x h picture, the base and the two signed strides:  D(x, y) = S[base + x sx + y sy]
struct OrientMap { uint32_t dw, dh; int64_t base, sx, sy; };
MJX_HD OrientMap orient_map(uint32_t c, uint32_t w, uint32_t h)
{
    OrientMap m;
    const bool T = orient_swaps(c), fu = orient_flips_u(c), fv = orient_flips_v(c);
    m.dw = T ? h : w; m.dh = T ? w : h;
    const int64_t du = fu ? -1 : 1, dv = fv ? -int64_t(w) : int64_t(w);         // one step along S's columns / rows
    m.base = (fu ? int64_t(w) - 1 : 0) + (fv ? (int64_t(h) - 1) * int64_t(w) : 0);
    m.sx = T ? dv : du;
    m.sy = T ? du : dv;
    return m;
}
// The rectangle of S that holds exactly the pixels of the rectangle (x, y, rw, rh) of D (rw, rh > 0, inside D): its two opposite
// corners through the map.
MJX_HD void orient_rect_to_stored(uint32_t c, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                                  uint32_t *sx0, uint32_t *sy0, uint32_t *sw, uint32_t *sh)
{
    const OrientMap m = orient_map(c, w, h);
    const int64_t i0 = m.base + int64_t(x) * m.sx + int64_t(y) * m.sy;
    const int64_t i1 = m.base + int64_t(x + rw - 1u) * m.sx + int64_t(y + rh - 1u) * m.sy;
    const uint32_t r0 = uint32_t(i0 / int64_t(w)), c0 = uint32_t(i0 - int64_t(r0) * int64_t(w));
    const uint32_t r1 = uint32_t(i1 / int64_t(w)), c1 = uint32_t(i1 - int64_t(r1) * int64_t(w));
    *sx0 = c0 < c1 ? c0 : c1; *sy0 = r0 < r1 ? r0 : r1;
    *sw = (c0 < c1 ? c1 - c0 : c0 - c1) + 1u; *sh = (r0 < r1 ? r1 - r0 : r0 - r1) + 1u;
}
// orient_compose(first, then): the one code that does what `first` followed by `then` does (0: a code outside 1 .. 8)
MJX_HD uint32_t orient_compose(uint32_t first, uint32_t then)
{
    const uint8_t t[8][8] = {{1, 2, 3, 4, 5, 6, 7, 8}, {2, 1, 4, 3, 8, 7, 6, 5}, {3, 4, 1, 2, 7, 8, 5, 6}, {4, 3, 2, 1, 6, 5, 8, 7},
                             {5, 6, 7, 8, 1, 2, 3, 4}, {6, 5, 8, 7, 4, 3, 2, 1}, {7, 8, 5, 6, 3, 4, 1, 2}, {8, 7, 6, 5, 2, 1, 4, 3}};
    return orient_valid(first) && orient_valid(then) ? t[first - 1u][then - 1u] : 0u;
}
constexpr uint32_t kOrientTile = 64;                        // k_orient_out: a workgroup owns kOrientTile x kOrientTile pixels of D
MJX_HD uint32_t orient_tiles(uint32_t w, uint32_t h) { return ((w + kOrientTile - 1) / kOrientTile) * ((h + kOrientTile - 1) / kOrientTile); }

// ---- YCbCr planes with an orientation and / or a resize (mjx_batch_create_planes_orient) -----------------------------------------
// Stage B writes such a picture as the plain plane decode does -- dense uint8 planes P_0 .. P_2, not interleaved, in the batch's pool
// (DevImage::ycc_*, kSinkYcc): the intermediate.  A pass behind it brings every plane to the form it leaves in: k_orient_planes
// copies orient_c(P_k) through the dtype's table (kPlaneCopy), k_resize_planes resamples orient_c(P_k) to the plane's own target
// (kPlaneResize; any code, 1 included).  What the pass needs of a picture is this descriptor, an array of its own beside the chunk's
// DevImages (same index): no DevImage field, and with it no existing kernel, changes.  A job is one plane -- plane 0, plane 1 (with
// il: Cb and Cr as pairs into the one plane), plane 2 (skipped with il) -- and rides in the grid's z dimension, so that every field a
// workgroup reads is uniform and indexed by a uniform.
enum PlanePassKind : uint32_t { kPlaneNone = 0, kPlaneCopy = 1, kPlaneResize = 2 };
struct PlanePass {
    uint32_t kind;              // PlanePassKind
    uint32_t code;              // the orientation, an EXIF code 1 .. 8
    uint32_t ncomp, il;         // planes of the intermediate (1 or 3); Cb and Cr leave interleaved in plane 1
    uint32_t dtype;             // MJX_DTYPE_* of the leaving planes
    uint32_t filter, aa;        // kPlaneResize: the filter kind and `antialias`
    uint32_t pad_;
    uint32_t sw[3], sh[3];      // the intermediate: plane k is sh[k] dense rows of sw[k] bytes at byte src_off[k] of the pool
    uint32_t dw[3], dh[3];      // the leaving planes' sizes in samples (the interleaved plane 1 has 2 dw[1] elements per row)
    uint64_t src_off[3];
    uint64_t dst_dev[3];        // caller-owned memory, or 0: byte dst_off[k] of the pool
    uint64_t dst_off[3];
    uint64_t pitch[3];          // elements between rows of leaving plane k
    float scale[3], bias[3];    // by COMPONENT: fmaf(value, scale[k], bias[k]) for the float dtypes
};
MJX_HD uint32_t plane_pass_jobs(uint32_t ncomp, uint32_t il) { return ncomp == 1u ? 1u : il ? 2u : 3u; }

// ---- libjpeg's pixels (mjx_opts.pixels = MJX_PIXELS_LIBJPEG): fancy upsampling and jdcolor.c's integer colour step ---------------
// A component plane: cw x ch samples in rows of `stride` bytes; s and stride are multiples of 8 and stride >= cw rounded up to 8, so
// that the aligned 4- and 8-byte reads below stay inside a row (what they bring in from behind cw is never used: indices clamp to
// the plane's edge).  rh, rv: the upsampling ratios, 1, 2 or 4.  k_upsample_color and the host (mjx_upsample_color_host) run these
// routines; a lane makes 8 adjacent pixels of one output row.  rep: the component is replicated whatever its ratios (MJX_IDCT_ISLOW's
// planes of at most two columns; k_upsample_rep and the host set it, the other kernels leave it 0).
struct LjPlane { const uint8_t *s; uint32_t stride, cw, ch, rh, rv; uint32_t rep = 0; };
constexpr uint32_t kLjStrip = 8;                               // pixels a lane makes
constexpr uint32_t kLjTileW = 64 * kLjStrip, kLjTileH = 16;    // the tile of a workgroup of k_upsample_color: a wave per row, four rows each
MJX_HD uint32_t lj_tiles(uint32_t x, uint32_t w, uint32_t h)   // strips start on multiples of kLjStrip of the PICTURE (aligned plane reads)
{
    const uint32_t span = x % kLjStrip + w;
    return ((span + kLjTileW - 1) / kLjTileW) * ((h + kLjTileH - 1) / kLjTileH);
}
MJX_HD uint32_t lj_ld32(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
#endif
}
// the samples X0 .. X0 + 7 (X0 a multiple of 8) of one row
MJX_HD void lj_row8(const uint8_t *row, uint32_t X0, int32_t v[8])
{
    const uint32_t a = lj_ld32(row + X0), b = lj_ld32(row + X0 + 4);
MJX_UNROLL
    for (uint32_t k = 0; k < 4; k++) { v[k] = int32_t((a >> (8 * k)) & 0xffu); v[4 + k] = int32_t((b >> (8 * k)) & 0xffu); }
}
// the samples i0 - 1 .. i0 + 4 (i0 a multiple of 4, i0 < cw) of one row, indices clamped to [0, cw)
MJX_HD void lj_row6(const uint8_t *row, uint32_t i0, uint32_t cw, int32_t v[6])
{
    const uint32_t a = lj_ld32(row + i0);
MJX_UNROLL
    for (uint32_t k = 0; k < 4; k++) v[1 + k] = int32_t((a >> (8 * k)) & 0xffu);
    v[0] = i0 ? int32_t(row[i0 - 1]) : v[1];
    v[5] = int32_t(row[i0 + 4 < cw ? i0 + 4 : i0]);               // (clamped below when it lies outside; the read stays inside the row)
MJX_UNROLL
    for (uint32_t k = 2; k < 6; k++) v[k] = i0 + k - 1 < cw ? v[k] : v[k - 1];
}
// Component p at the 8 pixels (X0 .. X0 + 7, Y) of the picture, X0 a multiple of 8 with X0 / rh < cw and Y / rv < ch:
//   (1, 1) the sample; (2, 1) out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2; (1, 2) the same down the
//   columns, bias 1 for the upper output row and 2 for the lower; (2, 2) t[i] = 3 near[i] + far[i], out[2i] = (3 t[i] + t[i-1] + 8) >> 4,
//   out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4 -- jdsample.c's h2v1 / h2v2 fancy upsampling with edge replication.
// A component with a ratio of 4 in EITHER direction is replicated in both -- out[k] = s[(X0 + k) / rh] of row Y / rv, jdsample.c's
// int_upsample, which libjpeg picks for every ratio pair that is not one of the four above; there is no triangle filter at ratio 4.
// So is a component with p.rep set (MJX_IDCT_ISLOW: jdsample.c takes its triangle filters only for planes of more than two columns).
MJX_HD void lj_strip8(const LjPlane &p, uint32_t X0, uint32_t Y, int32_t out[8])
{
    if (p.rh == 4u || p.rv == 4u || p.rep) {
        const uint8_t *row = p.s + size_t(Y >> ratio_shift(p.rv, 1u)) * p.stride;
        if (p.rh == 1u) {
            lj_row8(row, X0, out);
        } else if (p.rh == 2u) {
            const uint32_t a = lj_ld32(row + (X0 >> 1));                   // (X0 / 2 is a multiple of 4: inside the row)
MJX_UNROLL
            for (uint32_t k = 0; k < 8; k++) out[k] = int32_t((a >> (8 * (k >> 1))) & 0xffu);
        } else {
            const uint32_t i = X0 >> 2;                                    // (a multiple of 2, below cw; the row holds a multiple of 8)
            const int32_t s0 = int32_t(row[i]), s1 = int32_t(row[i + 1u]);
MJX_UNROLL
            for (uint32_t k = 0; k < 8; k++) out[k] = k < 4 ? s0 : s1;
        }
        return;
    }
    const uint32_t j = p.rv == 2u ? Y >> 1 : Y;
    uint32_t jf = j;                                               // the far row: above for even output rows, below for odd, clamped
    if (p.rv == 2u) jf = (Y & 1u) ? (j + 1u < p.ch ? j + 1u : j) : (j ? j - 1u : 0u);
    const uint8_t *rn = p.s + size_t(j) * p.stride, *rf = p.s + size_t(jf) * p.stride;     // the near and the far row
    if (p.rh == 1u) {
        int32_t a[8];
        lj_row8(rn, X0, a);
        if (p.rv == 2u) {
            int32_t b[8];
            lj_row8(rf, X0, b);
            const int32_t bias = (Y & 1u) ? 2 : 1;
MJX_UNROLL
            for (uint32_t k = 0; k < 8; k++) a[k] = (3 * a[k] + b[k] + bias) >> 2;
        }
MJX_UNROLL
        for (uint32_t k = 0; k < 8; k++) out[k] = a[k];
    } else {
        int32_t t[6];
        lj_row6(rn, X0 >> 1, p.cw, t);
        if (p.rv == 2u) {
            int32_t b[6];
            lj_row6(rf, X0 >> 1, p.cw, b);
MJX_UNROLL
            for (uint32_t k = 0; k < 6; k++) t[k] = 3 * t[k] + b[k];
        }
        const int32_t be = p.rv == 2u ? 8 : 1, bo = p.rv == 2u ? 7 : 2, sh = p.rv == 2u ? 4 : 2;
MJX_UNROLL
        for (uint32_t k = 0; k < 4; k++) {
            out[2 * k] = (3 * t[k + 1] + t[k] + be) >> sh;
            out[2 * k + 1] = (3 * t[k + 1] + t[k + 2] + bo) >> sh;
        }
    }
}
// jdcolor.c: FIX(x) = int(x 65536 + 0.5), R = Y + ((FIX(1.402) cr + 32768) >> 16) and so on, the shifts arithmetic.  Computed in
// float32, where it is EXACT: every product and sum is a whole number below 2^24 in magnitude (116130 * 128 + 32768 = 14.9 M), the
// scaling by 2^-16 is exact and floor is the arithmetic shift -- fused or not, rounding never happens.  On the device that is five
// full-rate instructions per channel where v_mul_lo_u32 alone costs four, and the clamp and the byte's place are one
// v_cvt_pk_u8_f32 (it saturates to [0, 255]; the value is a whole number, so its rounding mode does not matter).
MJX_HD void lj_color(float y, float cb, float cr, float &r, float &g, float &b)      // whole numbers in, whole numbers out, not clamped
{
    cb -= 128.0f; cr -= 128.0f;
    r = y + __builtin_floorf((91881.0f * cr + 32768.0f) * (1.0f / 65536.0f));
    b = y + __builtin_floorf((116130.0f * cb + 32768.0f) * (1.0f / 65536.0f));
    g = y + __builtin_floorf(((-22554.0f * cb + 32768.0f) - 46802.0f * cr) * (1.0f / 65536.0f));
}
// clamp(v, 0, 255) of a whole number, placed as byte `byte` of `word`
MJX_HD uint32_t lj_put_u8(float v, uint32_t byte, uint32_t word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_cvt_pk_u8_f32(v, byte, word);
#else
    const uint32_t u = v < 0.0f ? 0u : v > 255.0f ? 255u : uint32_t(v);
    return (word & ~(0xffu << (8u * byte))) | (u << (8u * byte));
#endif
}
// The 8 pixels (X0 .. X0 + 7, Y) as 24 bytes R,G,B,R,G,B ... in six little-endian words; one component: R = G = B = the sample.
MJX_HD void lj_pixels8(const LjPlane pl[3], uint32_t ncomp, uint32_t X0, uint32_t Y, uint32_t w[6])
{
    int32_t y[8], cb[8], cr[8];
    lj_strip8(pl[0], X0, Y, y);
    if (ncomp == 3u) { lj_strip8(pl[1], X0, Y, cb); lj_strip8(pl[2], X0, Y, cr); }
MJX_UNROLL
    for (uint32_t k = 0; k < 6; k++) w[k] = 0;
MJX_UNROLL
    for (uint32_t k = 0; k < 8; k++) {
        float c[3];
        c[0] = c[1] = c[2] = float(y[k]);
        if (ncomp == 3u) lj_color(float(y[k]), float(cb[k]), float(cr[k]), c[0], c[1], c[2]);
MJX_UNROLL
        for (uint32_t q = 0; q < 3; q++) w[(3 * k + q) >> 2] = lj_put_u8(c[q], (3 * k + q) & 3u, w[(3 * k + q) >> 2]);
    }
}
// Component p alone at the 8 pixels (X0 .. X0 + 7, Y), as 8 bytes in two little-endian words: a luminance picture (no colour step).
// k_upsample_luma and the host (mjx_upsample_luma_host) run this routine.
MJX_HD void lj_luma8(const LjPlane &p, uint32_t X0, uint32_t Y, uint32_t w[2])
{
    int32_t y[8];
    lj_strip8(p, X0, Y, y);
    w[0] = w[1] = 0;
MJX_UNROLL
    for (uint32_t k = 0; k < 8; k++) w[k >> 2] = lj_put_u8(float(y[k]), k & 3u, w[k >> 2]);
}

// ---- libjpeg's integer slow inverse DCT (MJX_OPTS_IDCT = MJX_IDCT_ISLOW; include/mjx.h states the contract) ---------------------
// jidctint.c's jpeg_idct_islow on uint32_t, so that the wrap-around the contract asks for is defined behaviour on the host too; only
// the descaling shift works on the value cast back to int32_t (arithmetic).  FIX(x) = int(x 8192 + 0.5).
constexpr uint32_t kIslowBits = 13, kIslowPass1 = 2;       // CONST_BITS, PASS1_BITS: pass 1 descales by 11, pass 2 by 18
MJX_HD uint32_t islow_descale(uint32_t x, uint32_t n) { return uint32_t(int32_t(x + (1u << (n - 1u))) >> n); }
// P of the contract on d[0 .. 7], in place, descaled by n
MJX_HD void islow_pass(uint32_t d[8], uint32_t n)
{
    constexpr uint32_t F0_298 = 2446u, F0_390 = 3196u, F0_541 = 4433u, F0_765 = 6270u, F0_899 = 7373u, F1_175 = 9633u, F1_501 = 12299u,
                       F1_847 = 15137u, F1_961 = 16069u, F2_053 = 16819u, F2_562 = 20995u, F3_072 = 25172u;
    uint32_t z1 = (d[2] + d[6]) * F0_541;
    const uint32_t t2 = z1 - d[6] * F1_847, t3 = z1 + d[2] * F0_765;
    const uint32_t t0 = (d[0] + d[4]) << kIslowBits, t1 = (d[0] - d[4]) << kIslowBits;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = d[7], b = d[5], c = d[3], e = d[1];
    z1 = a + e;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + e;
    const uint32_t z5 = (z3 + z4) * F1_175;
    a *= F0_298; b *= F2_053; c *= F3_072; e *= F1_501;
    z1 *= 0u - F0_899; z2 *= 0u - F2_562;
    z3 = z3 * (0u - F1_961) + z5;
    z4 = z4 * (0u - F0_390) + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; e += z1 + z4;
    d[0] = islow_descale(t10 + e, n); d[7] = islow_descale(t10 - e, n);
    d[1] = islow_descale(t11 + c, n); d[6] = islow_descale(t11 - c, n);
    d[2] = islow_descale(t12 + b, n); d[5] = islow_descale(t12 - b, n);
    d[3] = islow_descale(t13 + a, n); d[4] = islow_descale(t13 - a, n);
}
// four adjacent words of a block: one 16-byte access on the device (blk is 16-byte aligned there: a tile row of kPixStride words)
struct IslowQuad { uint32_t x, y, z, w; };
MJX_HD IslowQuad islow_ld4(const uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    return IslowQuad{v.x, v.y, v.z, v.w};
#else
    return IslowQuad{p[0], p[1], p[2], p[3]};
#endif
}
MJX_HD void islow_st4(uint32_t *p, uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(p) = make_uint4(x, y, z, w);
#else
    p[0] = x; p[1] = y; p[2] = z; p[3] = w;
#endif
}
// One lane = one block: blk[v * 8 + u] = coef[v][u] q[v][u] on entry, pass 2's output x on exit (the sample is islow_sample(x)).  In
// place, 16 bytes per access: a lane's blocks lie kPixStride = 17 x 16 bytes apart in the tile, an odd number of 16-byte units, so a
// wave's quads fall on different banks.  The column pass takes four columns at a time (eight quads in, 32 values in registers, eight
// quads out), the row pass one row (two quads).  libjpeg's shortcuts for all-zero AC columns give the same numbers and are left out.
MJX_HD void idct_islow_inplace(uint32_t *blk)
{
MJX_UNROLL
    for (uint32_t h = 0; h < 2u; h++) {                        // pass 1: columns 4 h .. 4 h + 3
        uint32_t c[4][8];
MJX_UNROLL
        for (uint32_t v = 0; v < 8u; v++) {
            const IslowQuad t = islow_ld4(blk + v * 8u + h * 4u);
            c[0][v] = t.x; c[1][v] = t.y; c[2][v] = t.z; c[3][v] = t.w;
        }
MJX_UNROLL
        for (uint32_t k = 0; k < 4u; k++) islow_pass(c[k], kIslowBits - kIslowPass1);
MJX_UNROLL
        for (uint32_t v = 0; v < 8u; v++) islow_st4(blk + v * 8u + h * 4u, c[0][v], c[1][v], c[2][v], c[3][v]);
    }
MJX_UNROLL
    for (uint32_t v = 0; v < 8u; v++) {                        // pass 2: row v
        const IslowQuad lo = islow_ld4(blk + v * 8u), hi = islow_ld4(blk + v * 8u + 4u);
        uint32_t r[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        islow_pass(r, kIslowBits + kIslowPass1 + 3u);
        islow_st4(blk + v * 8u, r[0], r[1], r[2], r[3]);
        islow_st4(blk + v * 8u + 4u, r[4], r[5], r[6], r[7]);
    }
}
// ---- ... at reduced scales: jidctred.c's 4x4, 2x2 and 1x1 transforms (include/mjx.h states the contract) ------------------------
// R4 of the contract: d[0 .. 7] of one column or row (d[4] is never read) -> four outputs in d[0 .. 3], descaled by n
MJX_HD void islow_red4_pass(uint32_t d[8], uint32_t n)
{
    constexpr uint32_t F0_211 = 1730u, F0_509 = 4176u, F0_601 = 4926u, F0_765 = 6270u, F0_899 = 7373u, F1_061 = 8697u, F1_451 = 11893u,
                       F1_847 = 15137u, F2_172 = 17799u, F2_562 = 20995u;
    const uint32_t t0 = d[0] << (kIslowBits + 1u);
    const uint32_t t2 = d[2] * F1_847 - d[6] * F0_765;
    const uint32_t t10 = t0 + t2, t12 = t0 - t2;
    const uint32_t z1 = d[7], z2 = d[5], z3 = d[3], z4 = d[1];
    const uint32_t a = z2 * F1_451 - z1 * F0_211 - z3 * F2_172 + z4 * F1_061;
    const uint32_t b = z3 * F0_899 - z1 * F0_509 - z2 * F0_601 + z4 * F2_562;
    d[0] = islow_descale(t10 + b, n); d[3] = islow_descale(t10 - b, n);
    d[1] = islow_descale(t12 + a, n); d[2] = islow_descale(t12 - a, n);
}
// R2: d[0], d[1], d[3], d[5], d[7] -> two outputs in d[0 .. 1]
MJX_HD void islow_red2_pass(uint32_t d[8], uint32_t n)
{
    constexpr uint32_t F0_720 = 5906u, F0_850 = 6967u, F1_272 = 10426u, F3_624 = 29692u;
    const uint32_t t10 = d[0] << (kIslowBits + 2u);
    const uint32_t t0 = d[5] * F0_850 - d[7] * F0_720 - d[3] * F1_272 + d[1] * F3_624;
    d[0] = islow_descale(t10 + t0, n); d[1] = islow_descale(t10 - t0, n);
}
// One lane = one block, in place as idct_islow_inplace: blk[v * 8 + u] = coef[v][u] q[v][u] on entry; on exit output (y, x), x, y < N,
// lies at blk[y * 8 + x] (the sample is islow_sample of it) and the rest of the block holds leftovers.  16 bytes per access.
// N = 4: pass 1 on every column but 4 over rows 0 .. 3, 5 .. 7 (four columns at a time; row 4 is not loaded), pass 2 on rows 0 .. 3.
MJX_HD void idct_red4_inplace(uint32_t *blk)
{
MJX_UNROLL
    for (uint32_t h = 0; h < 2u; h++) {
        uint32_t c[4][8];
MJX_UNROLL
        for (uint32_t v = 0; v < 8u; v++) {
            if (v == 4u) { c[0][v] = c[1][v] = c[2][v] = c[3][v] = 0u; continue; }
            const IslowQuad t = islow_ld4(blk + v * 8u + h * 4u);
            c[0][v] = t.x; c[1][v] = t.y; c[2][v] = t.z; c[3][v] = t.w;
        }
MJX_UNROLL
        for (uint32_t k = 0; k < 4u; k++)
            if (h * 4u + k != 4u) islow_red4_pass(c[k], kIslowBits - kIslowPass1 + 1u);        // (column 4: pass 2 never reads it)
MJX_UNROLL
        for (uint32_t v = 0; v < 4u; v++) islow_st4(blk + v * 8u + h * 4u, c[0][v], c[1][v], c[2][v], c[3][v]);
    }
MJX_UNROLL
    for (uint32_t v = 0; v < 4u; v++) {
        const IslowQuad lo = islow_ld4(blk + v * 8u), hi = islow_ld4(blk + v * 8u + 4u);
        uint32_t r[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        islow_red4_pass(r, kIslowBits + kIslowPass1 + 3u + 1u);
        islow_st4(blk + v * 8u, r[0], r[1], r[2], r[3]);
    }
}
// N = 2: pass 1 on columns 0, 1, 3, 5, 7 over rows 0, 1, 3, 5, 7, pass 2 on rows 0 and 1.
MJX_HD void idct_red2_inplace(uint32_t *blk)
{
MJX_UNROLL
    for (uint32_t h = 0; h < 2u; h++) {
        uint32_t c[4][8];
MJX_UNROLL
        for (uint32_t v = 0; v < 8u; v++) {
            if (v != 0u && !(v & 1u)) { c[0][v] = c[1][v] = c[2][v] = c[3][v] = 0u; continue; }
            const IslowQuad t = islow_ld4(blk + v * 8u + h * 4u);
            c[0][v] = t.x; c[1][v] = t.y; c[2][v] = t.z; c[3][v] = t.w;
        }
MJX_UNROLL
        for (uint32_t k = 0; k < 4u; k++)
            if (h * 4u + k == 0u || ((h * 4u + k) & 1u)) islow_red2_pass(c[k], kIslowBits - kIslowPass1 + 2u);
MJX_UNROLL
        for (uint32_t v = 0; v < 2u; v++) islow_st4(blk + v * 8u + h * 4u, c[0][v], c[1][v], c[2][v], c[3][v]);
    }
MJX_UNROLL
    for (uint32_t v = 0; v < 2u; v++) {
        const IslowQuad lo = islow_ld4(blk + v * 8u), hi = islow_ld4(blk + v * 8u + 4u);
        uint32_t r[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        islow_red2_pass(r, kIslowBits + kIslowPass1 + 3u + 2u);
        islow_st4(blk + v * 8u, r[0], r[1], r[2], r[3]);
    }
}
// N = 1: the DC term alone, descaled by 3
MJX_HD void idct_red1(uint32_t *blk) { blk[0] = islow_descale(blk[0], 3u); }
// the block's transform by its component's size N (8: the full one)
MJX_HD void idct_reduced_inplace(uint32_t *blk, uint32_t N)
{
    if (N == 8u) idct_islow_inplace(blk);
    else if (N == 4u) idct_red4_inplace(blk);
    else if (N == 2u) idct_red2_inplace(blk);
    else idct_red1(blk);
}
// the sample of pass 2's output x: clamp(x + 128, 0, 255) -- it saturates (|x| < 2^14 after the shift by 18: the sum cannot wrap)
MJX_HD uint32_t islow_sample(uint32_t x)
{
    const int32_t s = int32_t(x) + 128;
    return uint32_t(s < 0 ? 0 : s > 255 ? 255 : s);
}

// ---- resize on the device (mjx_resize): the separable triangle filter, one axis -----------------------------------------------
// Output coordinate X of an axis n_in -> n_out samples the input at c = (2X + 1) n_in / (2 n_out) with a triangle of half width
// fs = F / n_out, F = n_in when shrinking with antialias, n_out otherwise (fs = 1).  Everything stays in integers (n_in and n_out
// below stand for the two sizes divided by their greatest common divisor, which leaves c and fs as they are): with
// c = q + rem / (2 n_out), tap j lies at  j + 1/2 - c = t_j / (2 n_out),  t_j = (2 (j - q) + 1) n_out - rem,  and its weight is
// max(0, 2F - |t_j|) / 2F -- the numerators are whole numbers, so the weight of a tap is ONE rounding (the division by their sum,
// which is also a whole number) whatever the sizes; a float32 product (X + 0.5) r near 4000 would be 2e-4 pixels off.
// lo = max(0, floor(c - fs + 1/2)), hi = min(n_in, floor(c + fs + 1/2)); outside [lo, hi) the numerator is <= 0.
// The kernel (k_resize_out) and the host (mjx_resize_weights, mjx_resize_plan) run this one routine.  n_in, n_out <= kResizeMaxDim.
constexpr uint32_t kResizeMaxDim = 1u << 24;
constexpr uint32_t kResizeTileW = 64, kResizeTileH = 16;     // the target tile of a workgroup of k_resize_out
MJX_HD uint32_t resize_tiles(uint32_t w, uint32_t h) { return ((w + kResizeTileW - 1) / kResizeTileW) * ((h + kResizeTileH - 1) / kResizeTileH); }
struct ResizeAxis {
    uint32_t lo, hi;        // taps [lo, hi)
    int32_t t_lo;           // t_j at j = lo; t_(j+1) = t_j + step
    int32_t step;           // 2 n_out
    int32_t full;           // 2 F
    float sum;              // sum of the numerators over [lo, hi), added up as a whole number and rounded once (> 0)
};
MJX_HD uint32_t resize_num(const ResizeAxis &a, uint32_t j)       // numerator of tap j's weight (any j: 0 outside the triangle)
{
    const int32_t t = a.t_lo + int32_t(j - a.lo) * a.step, m = t < 0 ? -t : t;
    return m < a.full ? uint32_t(a.full - m) : 0u;
}
// the window and the first tap's offset, without the sum (uniform values a workgroup only needs the window of)
MJX_HD ResizeAxis resize_window(uint32_t n_in, uint32_t n_out, bool antialias, uint32_t X)
{
    ResizeAxis a;
    // in lowest terms (uniform over the picture): the ratio, so c, is the same, and the numerators are as small as they get -- an
    // integer ratio keeps them, the sums and their products with a byte exact in float32 (equal sizes: 2 and 0; 2:1: 1, 3, 3, 1)
    uint32_t g = n_in, g2 = n_out;
    while (g2) { const uint32_t r = g % g2; g = g2; g2 = r; }
    const uint64_t ni = n_in / g, no = n_out / g;
    const uint64_t num = (2ull * X + 1ull) * ni, den = 2ull * no;
    const uint64_t q = num / den, rem = num - q * den;
    const uint64_t F = antialias && ni > no ? ni : no;
    const int64_t lo_num = int64_t(num) + int64_t(no) - int64_t(2 * F);
    const uint64_t hi_q = (num + no + 2 * F) / den;
    a.lo = lo_num > 0 ? uint32_t(uint64_t(lo_num) / den) : 0u;
    a.hi = hi_q < n_in ? uint32_t(hi_q) : n_in;
    a.step = int32_t(den);
    a.full = int32_t(2 * F);
    a.t_lo = int32_t((2 * (int64_t(a.lo) - int64_t(q)) + 1) * int64_t(no) - int64_t(rem));
    a.sum = 0.f;
    return a;
}
MJX_HD ResizeAxis resize_axis(uint32_t n_in, uint32_t n_out, bool antialias, uint32_t X)
{
    ResizeAxis a = resize_window(n_in, n_out, antialias, X);
    uint64_t sum = 0;       // (a whole number; 65535 -> 1 passes 2^32)
    for (uint32_t j = a.lo; j < a.hi; j++) sum += resize_num(a, j);
    a.sum = float(sum);
    return a;
}

// ---- fit modes (mjx_resize's fit byte: MJX_FIT_COVER, MJX_FIT_CONTAIN; the rule of mjx.h) ------------------------------------------
// A = (x, y, w, h): the rectangle asked for, in the coordinates of the picture that leaves; W x H: the target.  COVER rewrites A to its
// largest centred part with the target's aspect (a: A', inner: the whole target); CONTAIN keeps A and gives the inner rectangle of the
// target the picture fills.  64-bit products, round(a / b) = (2a + b) / (2b).  w, h, W, H >= 1, all <= kResizeMaxDim.
// The planner (plan_input_for), mjx_resize_fit_plan and the tests' ctypes call run this one routine.
constexpr uint32_t kFitStretch = 0, kFitCover = 1, kFitContain = 2, kFitCount = 3;
struct FitRect { uint32_t x, y, w, h; };
struct FitPlan { FitRect a, inner; };
MJX_HD uint32_t fit_round_clamp(uint64_t num, uint64_t den, uint32_t hi)      // clamp(round(num / den), 1, hi)
{
    const uint64_t q = (2 * num + den) / (2 * den);
    return q < 1 ? 1u : q > hi ? hi : uint32_t(q);
}
MJX_HD FitPlan fit_rule(uint32_t mode, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t W, uint32_t H)
{
    FitPlan f;
    f.a = FitRect{x, y, w, h};
    f.inner = FitRect{0, 0, W, H};
    const uint64_t wH = uint64_t(w) * H, hW = uint64_t(h) * W;
    if (mode == kFitCover) {
        if (wH > hW) { f.a.w = fit_round_clamp(hW, H, w); f.a.x = x + (w - f.a.w) / 2; }
        else if (wH < hW) { f.a.h = fit_round_clamp(wH, W, h); f.a.y = y + (h - f.a.h) / 2; }
    } else if (mode == kFitContain) {
        if (wH > hW) f.inner.h = fit_round_clamp(hW, w, H);
        else if (wH < hW) f.inner.w = fit_round_clamp(wH, h, W);
        f.inner.x = (W - f.inner.w) / 2;
        f.inner.y = (H - f.inner.h) / 2;
    }
    return f;
}
// k_fit_pad: a workgroup owns kFitPadRows rows of the target (of every plane behind one another), a wave every fourth of them
constexpr uint32_t kFitPadRows = 16;
MJX_HD uint32_t fit_pad_wgs(uint32_t planes, uint32_t H) { return uint32_t((uint64_t(planes) * H + kFitPadRows - 1) / kFitPadRows); }

// ---- the filter kinds beside the triangle (mjx_resize's filter byte: MJX_FILTER_BICUBIC, MJX_FILTER_NEAREST) ----------------------
// The positions are the triangle's: c = q + rem / (2 n_out) in lowest terms, tap j at t_j / (2 n_out), its distance in units of the
// filter's scale x = |t_j| / 2F (F as above; F = n_out whenever the filter does not widen).  What differs is the support and the weight:
//   bicubic, antialias:  a = -0.5,  taps with x < 2: [floor(c - 2 fs + 1/2), floor(c + 2 fs + 1/2)), clipped to [0, n_in) and divided
//                        by their sum
//   bicubic, no antialias: a = -0.75, F = n_out, the four taps floor(c - 1/2) - 1 ... + 2 (the same window formula at fs = 1);
//                        a tap outside [0, n_in) reads the edge sample, so its weight is ADDED to tap 0's (fold_lo) or tap
//                        n_in - 1's (fold_hi) and the divisor is 1: nothing is renormalised
//   nearest:             the one tap q, weight 1
// The weight is evaluated in float32 from the quotient x = float(|t_j|) / float(2F) by the Horner forms of resize_cubic: x = 0, 1
// and 2 give exactly 1, 0 and 0, so equal sizes (t_j = 2 (j - X), 2F = 2) leave the tap j = X alone with weight 1 and sum 1.
// Explicit fmaf everywhere: host and device round alike whatever the compiler would contract.
// The kernels (resize_body), mjx_resize_filter_weights and mjx_resize_plan run these routines.
constexpr uint32_t kFilterTriangle = 0, kFilterBicubic = 1, kFilterNearest = 2, kFilterCount = 3;
MJX_HD float resize_cubic(float x, float a)      // k_a(x), x >= 0
{
    if (x < 1.0f) return __builtin_fmaf(__builtin_fmaf(a + 2.0f, x, -(a + 3.0f)), x * x, 1.0f);
    if (x < 2.0f) return a * __builtin_fmaf(__builtin_fmaf(x - 5.0f, x, 8.0f), x, -4.0f);
    return 0.0f;
}
struct ResizeTaps {
    uint32_t lo, hi;        // taps [lo, hi), inside [0, n_in)
    uint32_t last;          // n_in - 1
    int32_t t_lo;           // t_j at j = lo; t_(j+1) = t_j + step
    int32_t step;           // 2 n_out
    int32_t full;           // 2 F
    float a;                // the cubic's parameter
    float fold_lo, fold_hi; // no antialias: the weights of the taps below 0 / at and above n_in (else 0)
    float sum;              // the divisor: the float32 sum of the window's weights in ascending order, or 1 where nothing is renormalised
};
// the unfolded weight of a tap from its t (any tap: 0 outside the support)
template <uint32_t FILTER>
MJX_HD float resize_tap(int32_t t, int32_t step, int32_t full, float a)
{
    if constexpr (FILTER == kFilterNearest) return 2 * int64_t(t) > -int64_t(step) && 2 * int64_t(t) <= int64_t(step) ? 1.0f : 0.0f;   // (t_q = n_out - rem, rem in [0, 2 n_out))
    else { const int32_t m = t < 0 ? -t : t; return resize_cubic(float(m) / float(full), a); }
}
// the weight tap j of the window has in the sum: its own and what folds onto it
template <uint32_t FILTER>
MJX_HD float resize_tap_at(const ResizeTaps &a, uint32_t j, int32_t t)
{
    float w = resize_tap<FILTER>(t, a.step, a.full, a.a);
    if constexpr (FILTER == kFilterBicubic) {
        if (j == 0u) w += a.fold_lo;
        if (j == a.last) w += a.fold_hi;
    }
    return w;
}
// the window, the first tap's offset and the folded weights, without the sum
template <uint32_t FILTER>
MJX_HD ResizeTaps resize_taps_window(uint32_t n_in, uint32_t n_out, bool antialias, uint32_t X)
{
    static_assert(FILTER == kFilterBicubic || FILTER == kFilterNearest, "the triangle is resize_window's");
    ResizeTaps a;
    uint32_t g = n_in, g2 = n_out;
    while (g2) { const uint32_t r = g % g2; g = g2; g2 = r; }
    const uint64_t ni = n_in / g, no = n_out / g;
    const uint64_t num = (2ull * X + 1ull) * ni, den = 2ull * no;
    const uint64_t q = num / den, rem = num - q * den;
    const uint64_t F = FILTER == kFilterBicubic && antialias && ni > no ? ni : no;
    a.last = n_in - 1u;
    a.step = int32_t(den);
    a.full = int32_t(2 * F);
    a.a = antialias ? -0.5f : -0.75f;
    a.fold_lo = a.fold_hi = 0.0f;
    a.sum = 1.0f;
    if constexpr (FILTER == kFilterNearest) {
        a.lo = uint32_t(q); a.hi = a.lo + 1u;            // (q <= n_in - 1: (2X + 1) n_in < 2 n_out n_in)
        a.t_lo = int32_t(int64_t(no) - int64_t(rem));
        return a;
    }
    // floor((num + no -+ 4F) / den): the first tap and one past the last, before clipping
    const int64_t lo_num = int64_t(num) + int64_t(no) - int64_t(4 * F);
    const int64_t lo_raw = lo_num >= 0 ? lo_num / int64_t(den) : -((-lo_num + int64_t(den) - 1) / int64_t(den));
    const int64_t hi_raw = int64_t((num + no + 4 * F) / den);
    a.lo = lo_raw > 0 ? uint32_t(lo_raw) : 0u;
    a.hi = hi_raw < int64_t(n_in) ? uint32_t(hi_raw) : n_in;
    a.t_lo = int32_t((2 * (int64_t(a.lo) - int64_t(q)) + 1) * int64_t(no) - int64_t(rem));
    if (!antialias) {                                    // (four taps: at most two on either side)
        for (int64_t j = lo_raw; j < 0; j++)
            a.fold_lo += resize_tap<FILTER>(int32_t((2 * (j - int64_t(q)) + 1) * int64_t(no) - int64_t(rem)), a.step, a.full, a.a);
        for (int64_t j = int64_t(n_in); j < hi_raw; j++)
            a.fold_hi += resize_tap<FILTER>(int32_t((2 * (j - int64_t(q)) + 1) * int64_t(no) - int64_t(rem)), a.step, a.full, a.a);
    }
    return a;
}
template <uint32_t FILTER>
MJX_HD ResizeTaps resize_taps(uint32_t n_in, uint32_t n_out, bool antialias, uint32_t X)
{
    ResizeTaps a = resize_taps_window<FILTER>(n_in, n_out, antialias, X);
    if (FILTER == kFilterBicubic && antialias) {
        float sum = 0.0f;
        int32_t t = a.t_lo;
        for (uint32_t j = a.lo; j < a.hi; j++, t += a.step) sum += resize_tap<FILTER>(t, a.step, a.full, a.a);
        a.sum = sum;
    }
    return a;
}

// Where the segments of a scan begin (DevImage::seg_S): the first cut at or after scan MCU q0, as the scan MCU it lies at and its
// slot in the scan's table.  A cut lies at the start of every scan-MCU row and wherever a tile of the picture (seg_T picture MCUs
// in raster order) begins; a cut past the component's last real column is the next row's start (T.81 A.2.2: a one-component scan
// has no MCU padding blocks).  q0 at or past the scan's last MCU gives the sentinel slot, mcuy * seg_S.
struct PlanarCut { uint32_t mcu, slot; };
MJX_HD PlanarCut planar_cut(uint32_t q0, uint32_t scan_mcux, uint32_t S, uint32_t T, uint32_t pic_mcux, uint32_t hs, uint32_t vs)
{
    const uint32_t Rs = q0 / scan_mcux, Cs = q0 - Rs * scan_mcux;
    if (Cs == 0) return PlanarCut{q0, Rs * S};
    const uint32_t base = (Rs / vs) * pic_mcux;                  // the picture's first MCU in this MCU row
    const uint32_t t = (base + (Cs + hs - 1) / hs + T - 1) / T;  // the tile that begins at or after this column
    const uint32_t Cs2 = (t * T - base) * hs;
    if (Cs2 >= scan_mcux) return PlanarCut{(Rs + 1) * scan_mcux, (Rs + 1) * S};
    return PlanarCut{Rs * scan_mcux + Cs2, Rs * S + (t - base / T)};
}
// slots per scan-MCU row: the row's start + the tile boundaries inside a row of the picture
MJX_HD uint32_t planar_row_slots(uint32_t pic_mcux, uint32_t T) { return (pic_mcux + T - 1) / T + 1; }

// ---- compact coefficient stream, quad-interleaved (round 4) -----------------------------------------------------------
// A write-pass lane appends 32-byte groups (8 entries) to a stream of its own.  Packed one lane's run behind the other (the linear
// layout), every lane keeps a 128-byte line open over four flushes and a wave's flush touches 64 lines 3 KB apart: three fifths
// of the write pass went into these stores.  Here every subsequence owns a **column** of fixed capacity -- an
// entry takes at least 2 bits of scan, so sub_bits / 2 + 1 entries at most -- and four neighbouring columns are interleaved
// group by group: row r of quad q is one 128-byte line holding group r of subsequences 4q .. 4q + 3.  The four lanes flush
// within a step or two of each other, so the line is whole before it leaves L2 (k_huff_write 9.6 -> 8.05 ms per 2048 4K pictures
// for the stores alone), and a stage-B tile -- two or three lanes' worth of entries -- still reads consecutive lines.
//   entry j of subsequence s lies at  stream_phys(s, j, rows) = ((s >> 2) * rows + (j >> 3)) * 32 + (s & 3) * 8 + (j & 7)
//   a tile's start is recorded as the virtual index  s * (rows * 8) + j  (tile_eoff stays one 32-bit word per tile)
#ifndef MJX_STREAM_QUAD
#define MJX_STREAM_QUAD 4
#endif
constexpr uint32_t kStreamQuad = MJX_STREAM_QUAD;      // columns interleaved per row (a power of two; 4: a row is one 128-byte line)
// Single decode (round 5, k_huff_emit): a column also holds one word per block -- {DC difference, column index where the block's
// entries begin} -- filled from its top downwards (block word i at column index cap - 4 - 4 * (i >> 2) + (i & 3): 16-byte groups).
// A block takes at least two bits of scan and every entry two more, so entries and block words together are at most
// sub_bits / 2 + 2 words and never meet -- for tables that allow no denser block: ImagePlan::emit_fits keeps the others off this
// path.  kEmitHeadGroups rows of head room on top of that: the first decode of a subsequence starts
// its entries at index kEmitHeadGroups * 8 (its block words at kEmitHeadWords), so that a prefix that is decoded again
// from the true entry state can be written RIGHT-ALIGNED against the part of the first decode that stays valid, whatever the
// difference between the two prefixes' counts (photographic content: <= 24 entries, <= 33 blocks; flat content, whose blocks take
// a handful of bits, reaches a hundred and more blocks per 1024 bits of prefix; more than the head room = the picture falls back
// to the two-pass kernels).
constexpr uint32_t kEmitHeadGroups = 64;                       // entries: 512 of head room
constexpr uint32_t kEmitHeadWords = kEmitHeadGroups * 4u;      // block words of head room: 256 (DevImage::emit_head scales both)
constexpr uint32_t kEmitExtraRows = kEmitHeadGroups + kEmitHeadWords / 8u + 2u;
// (rows of a column: what the entries of a subsequence can need, and -- only for pictures whose first decode emits -- the head room and
// the block words on top; a picture that cannot take the single-decode path does not pay for them: at 1024-bit subsequences the
// column would be 164 rows instead of 66.  Round-5 advisor.)
MJX_HD uint32_t stream_rows_base(uint32_t sub_bits) { return (sub_bits / 2u + 1u + 7u) / 8u + 1u; }
MJX_HD uint32_t stream_rows_for(uint32_t sub_bits, bool emit = true) { return stream_rows_base(sub_bits) + (emit ? kEmitExtraRows : 0u); }
MJX_HD uint64_t stream_quad_entries(uint32_t nsub, uint32_t rows) { return uint64_t((nsub + kStreamQuad - 1) / kStreamQuad) * rows * 8u * kStreamQuad; }
// Head of a picture's stream region: one 32-bit word per subsequence -- the run of its entries in the column, in store groups,
// and what is added to its entries' block labels:   first group [11:0] | end group [23:12] | label offset [31:24]
// (k_huff_write: first group 0, offset 0 -- its entries carry the block's index in the picture; k_huff_emit / k_huff_prefix: the
// labels count the blocks the lane has completed, and the offset is the low byte of what turns that into the block's index).
MJX_HD uint32_t stream_hdr_entries(uint32_t nsub) { return (nsub * 4u + 127u) / 128u * 32u; }      // whole 128-byte lines
MJX_HD constexpr uint32_t run_word(uint32_t g0, uint32_t g1, uint32_t label_off) { return (g0 & 0xfffu) | ((g1 & 0xfffu) << 12) | (label_off << 24); }
MJX_HD constexpr uint32_t run_first(uint32_t w) { return w & 0xfffu; }
MJX_HD constexpr uint32_t run_end(uint32_t w) { return (w >> 12) & 0xfffu; }
MJX_HD constexpr uint32_t run_label(uint32_t w) { return w >> 24; }
// column index of block word i (see above)
MJX_HD uint32_t block_word_index(uint32_t i, uint32_t rows) { return rows * 8u - 4u - 4u * (i >> 2) + (i & 3u); }
// per-subsequence record of the emitting decode (chunk array, index sub_off + s)
struct alignas(16) EmitSub {
    uint32_t d0n, d0m;      // blocks completed / entries produced by the first decode (k_huff_emit)
    uint32_t kfix;          // 0: its entry state was right; k + 1: the true path meets it at checkpoint k; kEmitAll: nowhere inside
    uint32_t bad;           // the first symbol of the first decode that no code matches: bit position inside the subsequence [15:0] | label of its block [31:16], or 0xffffffff
    uint32_t bad_tail2;     // ... the first one inside the scan's tail behind the checkpoint boundary that lies in the tail (emit_tail_cp), same form
    int32_t lbl;            // label of the first decode's block at the merge point minus the true path's (k_huff_prefix)
    // The first one may lie in front of the merge point, on the part k_huff_prefix replaces; what it decides on then
    // (position inside the subsequence [15:0] | label [31:16], or 0xffffffff):
    uint32_t bad_last;      // the last such symbol in front of the scan's tail (emit_tail_start)
    uint32_t bad_tail;      // the first one inside the tail
};
// The tail of a scan: the bits a valid file has behind its last block at the least -- up to 7 padding bits and the end-of-image marker,
// which the scan keeps -- and what is read behind them.  Invalid codes of a valid file's true path lie there and nowhere else.
// (the tail and what is read behind it is shorter than the distance of two checkpoints: at most one boundary lies in it, this one)
MJX_HD uint32_t emit_tail_cp(uint32_t tail_start, uint32_t cp_bits) { return (tail_start + cp_bits - 1u) / cp_bits * cp_bits; }
MJX_HD uint32_t emit_tail_start(uint32_t total_bits, uint32_t sub_start) { return total_bits > sub_start + 23u ? total_bits - 23u - sub_start : 0u; }
constexpr uint32_t kEmitAll = 0xffffu;
MJX_HD uint64_t stream_phys(uint32_t s, uint32_t j, uint32_t rows) { return (uint64_t(s / kStreamQuad) * rows + (j >> 3)) * (8u * kStreamQuad) + (s % kStreamQuad) * 8u + (j & 7u); }

// ---- reading a tile out of the quad-interleaved stream (stage B; also the host-side expansion and the CPU emulation of the tests) ----
// A tile's entries are store groups in the columns of a few neighbouring subsequences: from the tile's own start (subsequence
// s0, entry j0 -- its tile offset, split by the caller) to the end of s0's run, the whole runs of the subsequences between, and
// the head of s1's column up to the next tile's start.  The groups are numbered in that order; quad_cell() finds group o.  So
// that a lane of stage B finds its group without a loop over memory, quad_prepare() packs, once per tile, the cumulative group
// counts of the tile's first kQuadSegs subsequences into 16 bytes; tiles that span more (beyond quality ~97) take the loop over
// the run lengths at the head of the stream region.  (With a dependent LDS read per subsequence in the fetch -- which sits
// between the scatter phase and the barrier in front of the inverse DCT -- stage B took 0.3 ms more per 2048 pictures.)
constexpr uint32_t kQuadSegs = 8;
// What the workgroup prepares per tile (32 bytes of LDS, two 16-byte reads): one word per subsequence of the tile, in order --
//   cumulative groups of the tile after this subsequence [13:0] | first group of the subsequence's run [23:14] | label offset [31:24]
// (the cumulative count of the last slot = the tile's groups; all ones there: more than kQuadSegs subsequences, the loop over the
// run words).  Round 5: the first group and the label offset are new -- a run no longer starts at row 0 of its column and its
// entries no longer carry the block's index in the picture (see run_word); packed here, once per tile, a lane still finds its
// group without a dependent read.
struct alignas(16) QuadCum { uint32_t w[kQuadSegs]; };
constexpr uint32_t kQuadCumMask = 0x3fffu, kQuadMany = 0x3fffu;
static_assert((kMaxSubseqBits / 2 + 8) / 8 + 1 + kEmitExtraRows < 1024, "a run's first group must fit ten bits (stream_rows_for(kMaxSubseqBits) < 1024)");
struct QuadView {
    const uint32_t *s_sub;               // LDS: subsequence of the workgroup's tile starts ...
    const uint16_t *s_at;                // ... and entry index in its column
    const QuadCum *s_cum;                 // LDS, per tile: see QuadCum
    const uint32_t *runs;                // the runs of all the picture's subsequences (run_word): the head of its stream region
    uint32_t rows, nsub;
};
struct QuadCell { uint32_t phys, k_lo, k_hi, label; };     // phys = 0xffffffff: no group for this lane; label: run_label of the group's subsequence
// What lane t of the workgroup prepares for tile t.
MJX_HD QuadCum quad_prepare(const QuadView &q, uint32_t k)
{
    const uint32_t s0 = q.s_sub[k], s1 = q.s_sub[k + 1], j0 = q.s_at[k], j1 = q.s_at[k + 1];
    QuadCum out;
MJX_UNROLL
    for (uint32_t i = 0; i < kQuadSegs; i++) out.w[i] = 0;
    if (s1 < s0 || s1 >= q.nsub) return out;                      // (offsets of a picture that did not decode: no entries, no reads)
    if (s1 - s0 >= kQuadSegs) { out.w[kQuadSegs - 1] = kQuadMany; return out; }
    uint32_t c = 0, run[kQuadSegs];
MJX_UNROLL
    for (uint32_t i = 0; i < kQuadSegs; i++) run[i] = q.runs[s0 + i < s1 ? s0 + i : s1];       // (all in flight together)
MJX_UNROLL
    for (uint32_t i = 0; i < kQuadSegs; i++) {
        const uint32_t s = s0 + i;
        if (s <= s1) {
            const uint32_t gs = i == 0 ? j0 >> 3 : run_first(run[i]);
            const uint32_t ge = s == s1 ? (j1 + 7u) >> 3 : run_end(run[i]);
            c += ge > gs ? ge - gs : 0u;
        }
        out.w[i] = (c < kQuadCumMask - 1u ? c : kQuadCumMask - 1u) | ((run_first(run[i]) & 0x3ffu) << 14) | (run_label(run[i]) << 24);
    }
    return out;
}
// Group o of tile k (of the workgroup): where it lies and which of its entries are the tile's.  Returns the tile's groups.
MJX_HD uint32_t quad_cell(const QuadView &q, uint32_t k, uint32_t o, QuadCell &cell)
{
    const uint32_t s0 = q.s_sub[k], s1 = q.s_sub[k + 1], j0 = q.s_at[k], j1 = q.s_at[k + 1];
    const QuadCum cw = q.s_cum[k];
    cell.phys = 0xffffffffu;
    cell.k_lo = 0;
    cell.k_hi = 8;
    cell.label = 0;
    uint32_t total, s = s0, first = j0 >> 3, before = 0;              // the group's subsequence, that one's first group, groups before it
    if ((cw.w[kQuadSegs - 1] & kQuadCumMask) != kQuadMany) {
        total = cw.w[kQuadSegs - 1] & kQuadCumMask;
        uint32_t sel = cw.w[0];
        bool own = true;                                                   // the group lies in the tile's first subsequence: it starts at j0
MJX_UNROLL
        for (uint32_t i = 0; i + 1 < kQuadSegs; i++) {
            const uint32_t ci = cw.w[i] & kQuadCumMask;
            const bool behind = o >= ci;                                   // (the counts stay at the total behind the tile's last subsequence)
            s += behind ? 1u : 0u;
            before = behind ? ci : before;
            sel = behind ? cw.w[i + 1] : sel;
            own = own && !behind;
        }
        first = own ? first : (sel >> 14) & 0x3ffu;
        cell.label = sel >> 24;
    } else {
        total = 0;
        bool found = false;
        for (uint32_t t = s0; t <= s1; t++) {
            const uint32_t rw = q.runs[t];
            const uint32_t gs = t == s0 ? j0 >> 3 : run_first(rw);
            const uint32_t ge = t == s1 ? (j1 + 7u) >> 3 : run_end(rw);
            const uint32_t cnt = ge > gs ? ge - gs : 0u;
            if (!found && o < total + cnt) { s = t; first = gs; before = total; found = true; cell.label = run_label(rw); }
            total += cnt;
        }
    }
    if (o < total) {
        const uint32_t at = (first + o - before) * 8u;
        cell.phys = uint32_t(stream_phys(s, at, q.rows));
        cell.k_lo = (o == 0u) ? j0 & 7u : 0u;
        cell.k_hi = (o == total - 1u && (j1 & 7u) != 0u) ? j1 & 7u : 8u;
    }
    return total;
}


// Lane-interleaved scan pool: pieces of 16 bytes, kLookPieces of look-ahead behind every subsequence (see LaneBits).
constexpr uint32_t kLookPieces = 4;
MJX_HD uint32_t scan_region_cols(uint32_t nsub) { return nsub ? (nsub + 7u) & ~7u : 0u; }
MJX_HD uint32_t scan_region_rows(uint32_t sub_bits) { return sub_bits / 128u + kLookPieces; }
MJX_HD uint64_t scan_region_bytes(uint32_t nsub, uint32_t sub_bits) { return uint64_t(scan_region_cols(nsub)) * scan_region_rows(sub_bits) * 16u; }
// One image of an upload for k_scan_interleave: where its linear de-stuffed scan lies in the staging buffer.
struct InterleaveImg {
    uint64_t lin_off;       // bytes into the linear staging buffer
    uint32_t lin_len;       // de-stuffed scan bytes
    uint32_t image;         // index into the DevImage array
};

// Device-side de-stuffing and marker scan (jpeg/mod.rs:371-385 on the GPU): one scan of an upload.
constexpr int kDestuffSeg = 16384;       // raw bytes per workgroup
struct DestuffImg {
    uint64_t raw_off, raw_len;           // stuffed bytes in the raw staging buffer (64-byte aligned, 64 bytes of padding behind)
    uint64_t out_off;                    // where the de-stuffed scan goes in the linear staging buffer
    uint32_t seg0, nseg;                 // this scan's slots in the per-segment count / base arrays (pairs: bytes kept, markers)
    uint32_t image;                      // its DevImage
    uint32_t ii_index;                   // its InterleaveImg (receives the de-stuffed length)
    uint32_t restarts;                   // 1: the picture has restart intervals -- RSTn markers leave the stream and are listed
    uint32_t rst0, rst_cap;              // the scan's slots in the marker list
    uint32_t direct;                     // 1: k_destuff_scatter writes the lane-interleaved region itself (scans without restart intervals,
                                         // round 5: no linear copy, no k_scan_interleave; the region was filled with 0xAA before); ii_index unused
    uint32_t pad_;
};

MJX_HD uint32_t mjx_popcount64(uint64_t v) { return uint32_t(__builtin_popcountll(v)); }

// The rule of one 64-byte piece, shared by k_destuff_count, k_destuff_scatter and the CPU emulation (tests/emul: emul_destuff).
// keep flags of the 64 bytes [i0, i0+64) of `raw` as a bit mask (+ the bytes themselves in q[0..3]); returns the
// number of kept bytes.  *rst_out: bit j set = a marker FF Dn begins at byte j (restarts only).  The raw staging buffer is
// 64-byte aligned per image and padded by 64 bytes (build_batch), so the four 16-byte loads of a piece and the byte behind
// it stay inside the image's own region.  V4: four 32-bit words x, y, z, w that are loaded as one (uint4 on the device).
template <class V4>
MJX_HD uint32_t destuff_keep_mask(const uint8_t *raw, uint64_t i0, uint64_t raw_len, V4 q[4], uint64_t *mask_out, bool restarts,
                                  uint64_t *rst_out)
{
    uint64_t mask = 0, rst = 0;
    if (i0 < raw_len) {
        const V4 *src = reinterpret_cast<const V4 *>(raw + i0);
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = src[k];
        uint32_t prev = i0 > 0 ? raw[i0 - 1] : 0u;
        const uint32_t n = uint32_t(raw_len - i0 < uint64_t(64) ? raw_len - i0 : uint64_t(64));
        const uint32_t behind = i0 + 64 < raw_len ? raw[i0 + 64] : 0u;       // (a marker may straddle two pieces)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t b = (w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
                const uint32_t jj = uint32_t(k * 16 + j);
                const uint32_t next = j < 15 ? (w[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xffu
                                             : (k < 3 ? (k == 0 ? q[1].x : k == 1 ? q[2].x : q[3].x) & 0xffu : behind);
                bool keep = !(b == 0x00u && prev == 0xffu);
                if (restarts) {
                    const bool marker = b == 0xffu && (next & 0xf8u) == 0xd0u && jj + 1 < n + (i0 + 64 < raw_len ? 1u : 0u);
                    if (marker) { keep = false; if (jj < n) rst |= 1ull << jj; }
                    if ((b & 0xf8u) == 0xd0u && prev == 0xffu) keep = false;
                }
                if (keep && jj < n) mask |= 1ull << jj;
                prev = b;
            }
        }
    }
    *mask_out = mask;
    *rst_out = rst;
    return mjx_popcount64(mask);
}

// mjx_batch_compare_rgb: one pair of pictures (device pointers: the pictures may live in different pools)
struct RgbPair { const uint8_t *a, *b; uint64_t bytes; };

// MCUs per stage-B tile: a power of two so that lane -> (MCU, strip) is a shift, and at most 256 strips per row.  At most
// MJX_GENERIC_TILE_BLOCKS blocks: the 4:2:0 kernel's 192, so that three workgroups fit a CU (round 5: a tile of 256 blocks -- 4:2:2,
// 64 MCUs -- held 69.6 KB of LDS, two workgroups per CU, and every picture of its batch was launched with that).
#ifndef MJX_GENERIC_TILE_BLOCKS
#define MJX_GENERIC_TILE_BLOCKS 192
#endif
inline uint32_t tile_mcus(uint32_t bpm, uint32_t hmax)
{
    uint32_t t = 1;
    while (t * 2 * bpm <= MJX_GENERIC_TILE_BLOCKS) t *= 2;
    const uint32_t cap = 256 / (2 * hmax);
    return t < cap ? t : cap;
}


uint32_t tile_mcus_420();       // MCUs per stage-B tile of the 4:2:0 kernel (kForm420)

// ---- launchers (mjx_kernels.hip); all asynchronous on `st` ---------------------------------------------
#if defined(__HIPCC__) || defined(MJX_WITH_HIP_RUNTIME)
size_t huff_lds_bytes(uint32_t lut_cap_entries);
size_t idct_lds_bytes(uint32_t max_tile_blocks);
int configure_kernels(size_t huff_lds, size_t idct_lds);
size_t huff_window_bytes();     // LDS the windowed entropy kernels need on top of huff_lds_bytes()
size_t huff_stage_bytes();      // ... and the write pass's entry rings
size_t huff_merge_bytes();      // LDS the merge kernels (rounds, straggler kernel, loop kernel) need on top of huff_lds_bytes()
uint32_t stream_group_entries();    // entries per store group of the write pass: a subsequence's run in the stream is rounded up to whole groups
// count -> prefix (+ geometry into `images`) -> scatter (+ marker list) -> segment tables of the pictures with restart intervals;
// segcount / segbase: two words per 16 KiB segment of every scan
void launch_destuff(hipStream_t st, uint32_t max_seg, uint32_t nimg, bool any_restarts, const DestuffImg *imgs, const uint8_t *raw,
                    uint32_t *segcount, uint32_t *segbase, uint8_t *pool, uint32_t *rst_off, DevImage *images, InterleaveImg *ii,
                    uint32_t *segs, uint32_t *img_flags, uint8_t *scan_pool /* the lane-interleaved pool: DestuffImg::direct scans go straight there */);
void launch_scan_interleave(hipStream_t st, uint32_t max_pieces, uint32_t nimg, const InterleaveImg *imgs, const DevImage *images,
                            const uint8_t *linear, uint8_t *pool, const uint32_t *segs);
void launch_huff_spec(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, size_t pad_lds, const DevImage *images,
                      const uint8_t *scan_pool, const LutEntry *lut_pool, SubseqState *entry, SubseqState *exit_,
                      uint32_t *cps, const uint32_t *segs, uint32_t lanes /* per workgroup: kHuffWg, or 256 / 128 for a chunk of short scans */,
                      uint8_t *gen /* [chunk subsequences] cleared per subsequence (Gen2), or null */);
void launch_huff_merge(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, size_t pad_lds, const DevImage *images,
                       const uint8_t *scan_pool, const LutEntry *lut_pool, SubseqState *entry, SubseqState *exit_,
                       uint32_t *cps, uint32_t *mismatches, uint32_t *items, uint32_t *item_count, const uint32_t *segs,
                       const uint32_t *prev_mismatches /* count of the round before, or null for the first */,
                       bool first_round /* most subsequences re-decode: the workgroups run their first slices in place */,
                       EmitSub *esub /* pictures whose first decode emits: the merge depth is kept here */,
                       uint32_t max_items /* subsequences of the chunk's longest scan - 1 (an upper bound will do) */,
                       uint8_t *gen /* [chunk subsequences]: which of the two sets of entry / exit / checkpoints is current (Gen2, mjx_kernels.hip) */,
                       uint32_t gen_stride /* subsequences between the two sets (a multiple of 256); 0: one set */);
// The merge rounds of a small chunk in one launch (device-wide barrier between rounds); `participants` = the workgroups (x, image)
// with x * merge_wg_lanes() + 1 < nsub(image): all of them must be resident at once (the caller checks against merge_loop_capacity()).
void launch_huff_merge_loop(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, size_t pad_lds, const DevImage *images,
                            const uint8_t *scan_pool, const LutEntry *lut_pool, SubseqState *entry, SubseqState *exit_,
                            uint32_t *cps, uint32_t *verdict, const uint32_t *segs, uint32_t *ctl, uint32_t participants, uint32_t max_rounds,
                            uint32_t spin_limit,       // spin_limit: polls of a barrier (~1.5 us each) before a workgroup gives up
                            EmitSub *esub,
                            uint8_t *gen, uint32_t gen_stride /* as launch_huff_merge */);
// single decode (round 5): the first decode of a picture emits (k_huff_emit); after the merge rounds and the scan, k_huff_prefix
// re-decodes what lay in front of the merge point for the lanes whose entry was wrong and k_block_gather makes dcdiff / tile offsets
size_t huff_prefix_bytes();
void launch_emit_off(hipStream_t st, DevImage *images, uint32_t nimg, const uint32_t *img_flags);     // fall-back: the flagged pictures leave the single-decode path (device copies patched in place)
void launch_huff_emit(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, size_t pad_lds, const DevImage *images,
                      const uint8_t *scan_pool, const LutEntry *lut_pool, SubseqState *entry, SubseqState *exit_, uint32_t *cps,
                      EmitSub *esub, uint32_t *entries, uint32_t lanes /* as launch_huff_spec */);
void launch_huff_prefix(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, const DevImage *images,
                        const uint8_t *scan_pool, const LutEntry *lut_pool, const SubseqState *entry, const SubseqState *exit_,
                        const uint32_t *cps, EmitSub *esub, const uint32_t *blkbase, uint32_t *entries, int *status, uint32_t *img_flags,
                        uint32_t *fallback /* device word: a picture had no head room for its prefix */, int16_t *dcdiff, uint32_t *tile_eoff,
                        const uint32_t *items, const uint32_t *item_count /* as written by k_huff_scan */,
                        uint32_t *unconverged /* device word, counted up by the first picture of the run that falls back */,
                        uint32_t lanes /* of the chunk's entropy workgroups (max_wg counts those) */);
void launch_huff_scan(hipStream_t st, uint32_t nimg, const DevImage *images, SubseqState *exit_, uint32_t *blkbase,
                      uint32_t *ebase, uint32_t *img_entries, uint32_t *img_flags, const uint32_t *segs,
                      const uint32_t *verdict /* device word: re-decodes of the last synchronisation round, or null */,
                      const EmitSub *esub, uint32_t *items /* [chunk subsequences][6]: per picture the (subsequence, checkpoint interval) pieces k_huff_prefix decodes again */,
                      uint32_t *item_count /* [chunk images] */, uint32_t *fallback /* device word: a picture goes to the two-pass kernels */,
                      uint32_t *unconverged /* device word, counted up when `verdict` is not zero */,
                      SubseqState *entry, uint8_t *gen, uint32_t gen_stride /* the rounds' second set is folded back into the first here */);
void launch_huff_write(hipStream_t st, uint32_t max_wg, uint32_t nimg, size_t tables_lds, size_t pad_lds, const DevImage *images,
                       const uint8_t *scan_pool, const LutEntry *lut_pool, const SubseqState *entry,
                       const uint32_t *blkbase, const uint32_t *ebase, uint32_t *entries, uint32_t *tile_eoff,
                       int16_t *dcdiff, int *status, const uint32_t *img_flags, const uint32_t *segs, const SubseqState *exit_,
                       uint32_t *cps /* measurement builds only */, uint32_t lanes /* as launch_huff_spec */);
void launch_dc_scan(hipStream_t st, uint32_t max_segs, uint32_t nimg, const DevImage *images, const int16_t *dcdiff, int32_t *dcbuf,
                    int32_t *segsum, const uint32_t *img_flags, uint32_t bpm_mask, uint32_t max_restart_segs,
                    uint32_t *segflag = nullptr, uint32_t gen = 0,
                    uint32_t *fail = nullptr /* device word, set when the one-pass kernel gave up waiting */, uint32_t spin_limit = 1u << 20,
                    bool fault = false /* test knob: a workgroup never publishes */);
// (max_tiles: the chunk's largest count of tiles a picture's workgroups walk -- DevImage::roi_ntiles; mode_mask bit m: the chunk holds
// a picture of DevImage::mode m; each entry of MJX_STAGE_B_KERNELS whose mode, layout bit and density are present is launched)
void launch_idct_color(hipStream_t st, uint32_t max_tiles, uint32_t nimg, size_t lds, const DevImage *images,
                       const uint32_t *entries, const uint32_t *tile_eoff, const int32_t *dcbuf, const float *qmult,
                       uint8_t *rgb, uint64_t mode_mask, unsigned long long *planes, const uint32_t *img_flags,
                       bool dense /* the chunk's linear streams are dense (many entries per tile): deeper prefetch in the 4:2:0 kernel */,
                       uint32_t layout_mask /* bit 0: pictures with a linear stream, bit 1: with a quad-interleaved one */);
// multi-scan pictures: component streams (raster order) -> the picture's stream in MCU order, tile offsets, DC values
void launch_planar_gather(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, uint32_t *entries,
                          uint32_t *tile_eoff, int32_t *dcbuf, uint32_t *img_flags, bool copy);
// progressive pictures: one lane per (scan, restart interval) of one level -- lanes [lane0, lane0 + nlanes) of the batch's array --
// into the dense store; then the store -> the picture's stream in MCU order, tile offsets, DC values (k_prog_count / _offsets / _copy)
struct ProgLane;
struct ProgPic;
void launch_prog_scan(hipStream_t st, uint32_t nlanes, const ProgLane *lanes, const ProgPic *pics, const DevImage *images,
                      const uint8_t *bytes, const LutEntry *lut_pool, int16_t *store, uint32_t *img_flags);
void launch_prog_compact(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const ProgPic *pics, const int16_t *store,
                         uint32_t *entries, uint32_t *tile_eoff, int32_t *dcbuf, uint32_t *img_flags, int *status);
void launch_rgb_compare(hipStream_t st, uint32_t npairs, uint64_t max_bytes, const RgbPair *pairs, uint32_t *maxdiff,
                        unsigned long long *ndiff);
void launch_ref_color(hipStream_t st, uint32_t max_pixel_wgs, uint32_t nimg, const DevImage *images,
                      const unsigned long long *planes, uint8_t *rgb, const uint32_t *img_flags);
// scaled decode at 1/8 (kFormEighth): one lane per output pixel from the blocks' DC values; max_pixel_wgs = the chunk's largest
// ceil(out_w * out_h / 256)
void launch_dc_color(hipStream_t st, uint32_t max_pixel_wgs, uint32_t nimg, const DevImage *images, const int32_t *dcbuf,
                     const float *qmult, uint8_t *rgb, const uint32_t *img_flags, bool roi = false /* the form for pictures with a rectangle */,
                     bool out = false /* the form for pictures with an output description (kFormEighth, kSinkOut) */);
// ... luminance pictures (kFormEighth, kSinkLuma): one lane per pixel of the rectangle, component 0's DC value alone
void launch_dc_color_luma(hipStream_t st, uint32_t max_pixel_wgs, uint32_t nimg, const DevImage *images, const int32_t *dcbuf,
                          const float *qmult, uint8_t *rgb, const uint32_t *img_flags);
// ... YCbCr output (kFormEighth, kSinkYcc): one lane per sample of each plane, the components' DC values alone
void launch_dc_color_ycc(hipStream_t st, uint32_t max_sample_wgs, uint32_t nimg, const DevImage *images, const int32_t *dcbuf,
                         const float *qmult, uint8_t *rgb, const uint32_t *img_flags);
// resize on the device: one workgroup per tile of the target (resize_tiles) and picture with DevImage::rs_on, behind stage B
// (filter: the kind of the pictures the launch is for -- kFilterTriangle, kFilterBicubic, kFilterNearest; the others are passed over)
void launch_resize_out(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, uint8_t *rgb, const uint32_t *img_flags,
                       uint32_t filter = 0);
// orientation on the device, behind stage B like the resize: one workgroup per tile of D (orient_tiles) and picture with or_on == kOrCopy
// (k_orient_out), or per tile of the target (resize_tiles) and picture with or_on == kOrResize (k_resize_orient)
// luma: the one-channel forms for luminance pictures -- kOrCopyLuma (k_orient_luma), kOrResizeLuma (k_resize_luma, any code, 1 included)
void launch_orient_out(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, uint8_t *rgb, const uint32_t *img_flags, bool luma = false);
void launch_resize_orient(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, uint8_t *rgb, const uint32_t *img_flags, bool luma = false,
                          uint32_t filter = 0);
// fit modes: the border of every picture with DevImage::fit_on (MJX_FIT_CONTAIN), behind stage B on the resize's stream; max_wgs = the
// chunk's largest fit_pad_wgs
void launch_fit_pad(hipStream_t st, uint32_t max_wgs, uint32_t nimg, const DevImage *images, uint8_t *rgb, const uint32_t *img_flags);
// YCbCr planes with an orientation and / or a resize, behind stage B: one workgroup per tile (orient_tiles / resize_tiles of the
// chunk's largest leaving plane), plane job (grid z: 3) and picture whose PlanePass::kind is kPlaneCopy (k_orient_planes) or
// kPlaneResize with this filter kind (k_resize_planes, _cubic, _nearest); `passes` is the chunk's array, one entry per DevImage
void launch_orient_planes(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const PlanePass *passes, uint8_t *rgb,
                          const uint32_t *img_flags);
void launch_resize_planes(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const PlanePass *passes, uint8_t *rgb,
                          const uint32_t *img_flags, uint32_t filter);
// libjpeg's pixels, behind stage B: one workgroup per tile of the rectangle (lj_tiles) and picture with DevImage::lj_on
void launch_upsample_color(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const uint8_t *planes, uint8_t *rgb,
                           const uint32_t *img_flags, bool luma = false /* k_upsample_luma: pictures with DevImage::lj_luma */);
// ... k_upsample_rep: pictures with DevImage::lj_rep (the integer inverse DCT's planes of at most two columns, replicated)
void launch_upsample_rep(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const uint8_t *planes, uint8_t *rgb,
                         const uint32_t *img_flags);
// ... k_upsample_red: pictures with DevImage::lj_red (the integer inverse DCT at a reduced scale)
void launch_upsample_red(hipStream_t st, uint32_t max_tiles, uint32_t nimg, const DevImage *images, const uint8_t *planes, uint8_t *rgb,
                         const uint32_t *img_flags);
#endif

}   // namespace mjx
#endif

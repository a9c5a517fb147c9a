/*
 * mjx.h -- C ABI of the MI355X-native baseline-JPEG decode path.
 *
 * Drop-in boundary for martinhath/jpeg-rust's decode(&[u8]) -> RGB surface
 * (SURVEY.md s8(b)).  Every entry point cites the reference interface it replaces
 * (paths relative to /root/reference/src).  Plain pointers and sizes only: this is what a
 * Rust `extern "C"` block binds (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Nothing here ever panics/aborts across the ABI: the reference's panics (jpeg/mod.rs Q12)
 * become status codes.  The GPU entry points fail with MJX_ERR_DEVICE when no HIP device or
 * kernel image is available -- there is no CPU fallback.
 */
#ifndef MJX_H
#define MJX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The binary layout of the structs below.  1: up to scaled decode, rectangles, output formats, resize and orientation.  2: mjx_opts
 * gained `pixels` at byte 8 and its scale_denom moved from byte 8 to byte 9 (size and every other offset unchanged): a caller built
 * against layout 1 that sets scale_denom is refused with MJX_ERR_INVALID_ARG, never served another picture.  mjx_version() prints the
 * layout the library was built with as "abi=<n>". */
#define MJX_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------------------------ */
enum {
    MJX_OK = 0,
    MJX_ERR_TRUNCATED = 1,          /* ran off the end of the file while parsing (ref: slice-index panic); or, from the device:
                                     * the scan ends early.  The device's rule (the band rule): the scan is the
                                     * de-stuffed bytes behind the SOS header up to the end of the file, the end-of-image marker
                                     * included, 0xAA behind them; a symbol is decoded when it STARTS at or before the scan's last
                                     * bit rounded up to a multiple of 32 (with restart intervals: the interval's last bit, counted
                                     * from the interval's first, and the bits behind it are the next interval's); the picture is
                                     * truncated when the symbols so decoded do not complete every block it needs (every block of
                                     * every interval), or when it has fewer RSTn markers than intervals less one.  A scan that
                                     * ends a few bytes early can therefore come out MJX_OK with wrong last blocks; whatever lies
                                     * behind the last block needed is never looked at.  Wins over MJX_ERR_BAD_HUFFMAN. */
    MJX_ERR_UNSUPPORTED_MARKER = 2, /* strict_ref: marker outside jpeg/mod.rs:166-179 (incl. APP12/APP14, :445-450) */
    MJX_ERR_DRI_UNSUPPORTED = 3,    /* jpeg/mod.rs:424-428 panics on DRI */
    MJX_ERR_BAD_HUFFMAN = 4,        /* invalid DHT, or no code matched during decode (huffman.rs:156,162): inside a block the
                                     * picture needs, the next 16 bits begin with no code of the block's table (or the DC symbol
                                     * is above 15).  The decode goes on -- such a pattern takes one bit and stands for a symbol of
                                     * run 0, size 0 -- but the picture's coefficients and pixels are not handed out.  Patterns
                                     * behind the last block needed do not count.  MJX_ERR_TRUNCATED wins where both hold.
                                     * Also the status of a picture whose decode tables do not fit: the tables of a scan's distinct
                                     * DC and AC slots -- 2 KiB per DC table, 4 KiB per AC table, and their second-level tables -- are
                                     * addressed with 15 bits, so a set above 32 767 bytes is refused by the planner, the other
                                     * pictures of the call unaffected.  Three pairs of any shape fit (largest seen 23 696 bytes), and
                                     * so do four Annex K-style or optimised pairs (under 28 KiB; the largest set of the test shapes
                                     * is 31 584 bytes); four pairs that each spread codes of 10 to 16 bits over every prefix they
                                     * can (34 880 bytes) do not, valid though the file is. */
    MJX_ERR_REF_PANIC = 5,          /* other input on which the reference panics (asserts, bad DQT precision ...) */
    MJX_ERR_DEVICE = 6,             /* HIP error / no device / kernels missing */
    MJX_ERR_UNSUPPORTED_FORMAT = 7, /* non-baseline SOF, ncomp not in {1,3} (decoder.rs:328-330; {1,3,4} with MJX_COLOR_FILE), a sampling factor other than 1, 2 or 4,
                                       more than 12 blocks per MCU (10 with four components) */
    MJX_ERR_NO_SCAN = 8,            /* EOF without SOS: the reference returns image_data() == None */
    MJX_ERR_INVALID_ARG = 9,
    MJX_ERR_NOMEM = 10,
    MJX_ERR_MISSING_TABLE = 11      /* scan references a DQT/DHT slot that was never defined (decoder.rs:154-160,222) */
};

enum {
    MJX_LAYOUT_STANDARD = 0,  /* standard MCU count, block placement, box chroma replication, edge clipping */
    MJX_LAYOUT_REF_COMPAT = 1 /* bug-for-bug placement of decoder.rs:239-312 */
};

enum {
    MJX_PIXELS_REFERENCE = 0, /* box chroma replication, float colour conversion, truncating store (the reference's pixels) */
    MJX_PIXELS_LIBJPEG = 1    /* rounded samples, fancy (triangle) chroma upsampling, libjpeg's integer colour tables */
};

enum {
    MJX_COLOR_POSITIONAL = 0, /* one component, or three that are Y, Cb, Cr by position (the reference's rule); four are refused */
    MJX_COLOR_FILE = 1        /* the file says what its components are: MJX_OPTS_COLOR */
};

/* What the components of a file are (mjx_color_model, mjx_batch_image_color, mjx_scan_desc.model). */
enum {
    MJX_MODEL_GREY = 0,   /* one component */
    MJX_MODEL_YCBCR = 1,  /* Y, Cb, Cr */
    MJX_MODEL_RGB = 2,    /* R, G, B stored as they are */
    MJX_MODEL_CMYK = 3,   /* C, M, Y, K in Adobe's convention: the stored value is the amount of light */
    MJX_MODEL_YCCK = 4    /* CMYK whose first three components went through the YCbCr transform */
};

enum mjx_destuff {
    MJX_DESTUFF_AUTO = 0,
    MJX_DESTUFF_DEVICE = 1,
    MJX_DESTUFF_HOST = 2
};

/* A rectangle in the coordinates of the picture a call would otherwise produce (STANDARD layout at the call's scale_denom:
 * out_w x out_h = ceil(W/s) x ceil(H/s)).  No alignment is asked of x, y, w or h; w == 0 && h == 0 means the whole picture. */
typedef struct mjx_rect { uint32_t x, y, w, h; } mjx_rect;

typedef struct mjx_opts {
    uint8_t strict_ref;   /* 1: unknown / APP12 / APP14 markers are errors like the reference; 0: skip them */
    uint8_t layout;       /* MJX_LAYOUT_* */
    uint8_t keep_coefs;   /* 1: keep the whole batch's coefficient stream resident (T0 checks, stage-B-only sweeps) */
    uint8_t device_destuff;/* MJX_DESTUFF_*: who removes the FF00 stuffing of jpeg/mod.rs:371-385.
                             MJX_DESTUFF_DEVICE (1): the host does not touch the entropy-coded bytes -- mjx_parse copies them as
                             they are (desc.scan_is_stuffed = 1), and the FF00 -> FF compaction, the search for RSTn markers
                             and the scan's length are the GPU's at upload (mjx_batch_create, mjx_decode_batch, the pool).
                             MJX_DESTUFF_HOST (2): the byte pass on the host.  MJX_DESTUFF_AUTO (0): the host pass in
                             mjx_parse and mjx_decode; in mjx_decode_batch and the pool the GPU for lists of 64 MB and more
                             (MJX_AUTO_DESTUFF_MB; it is the faster of the two there), the host below.  The picture is the
                             same.  Never on the GPU with strict_ref (the byte pass stays, for the reference's unguarded read
                             behind a last FF) nor for multi-scan files (their scans are cut apart on the host). */
    uint32_t chunk_images;/* images per kernel chunk; 0 = library default */
    uint8_t pixels;       /* MJX_PIXELS_*.  MJX_PIXELS_LIBJPEG: the picture libjpeg's pipeline gives behind its inverse DCT.  Component c
                             with factors (h, v) is a plane of ceil(W h / hmax) x ceil(H v / vmax) samples s = clamp(floor(f + 128 + 0.5),
                             0, 255), f the float sample of the default pixels.  Each plane is upsampled by (rh, rv) = (hmax / h,
                             vmax / v) in integers, indices outside the plane clamped to its edge:
                               (2, 1) out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2;
                               (1, 2) the same down the columns, bias 1 for the upper output row and 2 for the lower;
                               (2, 2) t[i] = 3 near[i] + far[i] (near: the chroma row under the output row, far: the one above it for
                                      even output rows, below for odd), out[2i] = (3 t[i] + t[i-1] + 8) >> 4,
                                      out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4;
                             a component with a ratio of 4 in EITHER direction is replicated in both, out[X][Y] = s[X / rh][Y / rv]
                             (jdsample.c's int_upsample: libjpeg has no triangle filter at ratio 4, and picks replication for the
                             whole component even where its other ratio is 2);
                             (no fall-back to replication for planes of one or two columns).  Colour is jdcolor.c's, FIX(x) =
                             int(x 65536 + 0.5), cb = Cb - 128, cr = Cr - 128: R = clamp(Y + ((FIX(1.40200) cr + 32768) >> 16)),
                             B = clamp(Y + ((FIX(1.77200) cb + 32768) >> 16)), G = clamp(Y + ((-FIX(0.34414) cb + 32768
                             - FIX(0.71414) cr) >> 16)); one component: R = G = B = s.  STANDARD layout at full size only:
                             MJX_LAYOUT_REF_COMPAT, strict_ref or scale_denom > 1 give the picture MJX_ERR_INVALID_ARG (a resize with
                             auto_scale picks scale 1) -- a scale is accepted together with MJX_IDCT_ISLOW and MJX_OPTS_EXACT_SCALE
                             only, see there.  Rectangles, output formats, resize and orientation compose as with the
                             default pixels: a rectangle is byte for byte the crop of the whole picture.  Anything but 0 and 1:
                             MJX_ERR_INVALID_ARG.  (The field stands in front of scale_denom, not at the struct's end: the struct's
                             size and the other fields' offsets are as before, scale_denom's moved by one byte -- callers are
                             rebuilt against this header.  A zero-filled struct keeps the default pixels.) */
    uint8_t scale_denom;  /* scaled decode in the DCT domain: 0 or 1 = full size; 2, 4, 8 = 1/2, 1/4, 1/8 (anything else:
                             MJX_ERR_INVALID_ARG).  The picture is ceil(W/s) x ceil(H/s) (libjpeg's jdiv_round_up).  Per block the
                             low N x N corner (N = 8/s) of the dequantised coefficients F(u,v), natural order, goes through the
                             N-point inverse DCT with the 8-point normalisation:
                               f(x,y) = 1/4 sum_{u,v<N} C(u) C(v) F(u,v) cos((2x+1)u pi/2N) cos((2y+1)v pi/2N),
                               C(0) = 1/sqrt(2), C(k>0) = 1  (N = 1: F(0,0)/8),
                             so a flat block gives the same level at every scale.  Level shift, colour formula and truncating
                             store are the STANDARD layout's; chroma is box-replicated at the output resolution (output pixel
                             (X,Y) takes the sample at (X h/Hmax, Y v/Vmax) of the component's scaled plane).  STANDARD layout
                             only: MJX_LAYOUT_REF_COMPAT with a scale above 1 is MJX_ERR_INVALID_ARG.  For a scaled batch
                             mjx_batch_image_info, mjx_batch_copy_rgb, mjx_batch_rgb_device and mjx_batch_bytes speak of the
                             output picture. */
    const mjx_rect *rois; /* region-of-interest decode: NULL = whole pictures.  A picture with a rectangle is w x h x 3 bytes, R,G,B,
                             row-major, unpadded: the pixels [y, y+h) x [x, x+w) of the picture the call would otherwise write, byte
                             for byte.  Stage B fetches and transforms only the tiles that touch the rectangle (mjx_plan_tiles), and
                             the picture's RGB region is the rectangle's.  A rectangle that does not lie inside out_w x out_h, or has
                             exactly one of w and h zero, gives that picture MJX_ERR_INVALID_ARG (the others are unaffected);
                             MJX_LAYOUT_REF_COMPAT with a rectangle is MJX_ERR_INVALID_ARG.  mjx_batch_image_info, _copy_rgb,
                             _rgb_device, _bytes and _compare_rgb speak of the cropped picture (mjx_batch_image_roi: where it
                             lies); mjx_batch_copy_coefs is unchanged.  The array is only borrowed for the duration of the call. */
    uint32_t n_rois;      /* 0 with rois == NULL; 1: the one rectangle applies to every input of the call (mjx_validate,
                             mjx_plan_tiles: rois[0]); n, the call's number of inputs: rois[i] belongs to input i.  Anything else,
                             or rois == NULL with n_rois != 0, fails the call with MJX_ERR_INVALID_ARG. */
} mjx_opts;

/* The colour option of a call: byte 10 of mjx_opts, one of the padding bytes behind `scale_denom` that the declared members leave unused
 * (the struct's members, size and offsets are as they were; a zero-filled struct means what it meant).  An lvalue:
 * MJX_OPTS_COLOR(&opts) = MJX_COLOR_FILE.  Fill the struct with zeros first (memset, = {0} on a static, value-initialisation in C++)
 * and set the byte on the object the call is given: a member-wise copy of the struct need not carry it.
 * MJX_COLOR_*: where the meaning of a file's components comes from.  MJX_COLOR_POSITIONAL (0): one component is grey, three are Y, Cb,
 * Cr whatever the file says, four are MJX_ERR_UNSUPPORTED_FORMAT -- bit for bit the decode of every earlier version.  MJX_COLOR_FILE
 * (1): libjpeg's default_decompress_parms, decided on the host (mjx_color_model).  One component: grey.  Three: a JFIF APP0 segment
 * seen: YCbCr; else an Adobe APP14 segment seen: transform 0 RGB, anything else YCbCr; else the component ids 'R','G','B': RGB; else
 * YCbCr.  Four: an Adobe segment with a transform other than 0: YCCK; transform 0 or no Adobe segment: CMYK.  An APP14 segment counts
 * when its payload is at least 12 bytes and begins with "Adobe"; the transform is payload byte 11; JFIF is an APP0 whose payload
 * begins "JFIF\0"; the last such segment in front of the first SOS counts.  The pixels: s_c is the byte of component c at a pixel --
 * box-replicated, level-shifted, truncated and saturated exactly as the packed decode of a one-component file that carries c's blocks
 * stores it.  RGB: R,G,B = s_0, s_1, s_2.  CMYK: R = mul(s_0, s_3), G = mul(s_1, s_3), B = mul(s_2, s_3), mul(a, k) = (a k + 127) /
 * 255 in integers (mjx_ink_mul): samples are taken in Adobe's convention, stored value = amount of light, with or without an APP14
 * segment, as Pillow takes them. YCCK: (r, g, b) = the default colour step on components 0 .. 2, truncated to bytes; the
 * writer took that transform of the complemented samples, so s_0 = 255 - r (libjpeg's ycck_cmyk_convert: C = MAXJSAMPLE - R), and
 * R = mul(255 - r, s_3), likewise G, B -- the picture libjpeg and Pillow give for an Adobe transform 2 file.  YCbCr and grey pictures are byte for byte those of MJX_COLOR_POSITIONAL.  A frame of four components must
 * be one interleaved scan of at most 10 blocks per MCU (T.81's limit), else MJX_ERR_UNSUPPORTED_FORMAT; restart intervals are fine.
 * Scales, rectangles, output formats, caller memory, resize, orientation and the pipelined calls compose: a picture leaves stage B as
 * R,G,B.  Refused per picture with MJX_ERR_UNSUPPORTED_FORMAT, the others of the call unaffected -- the follow-ups: an RGB, CMYK or
 * YCCK picture with luminance output (MJX_OUTPUT_CHANNELS == 1: component 0 of such a file is not a luminance), with a plane
 * description, or with MJX_PIXELS_LIBJPEG.  strict_ref or MJX_LAYOUT_REF_COMPAT together with MJX_COLOR_FILE: MJX_ERR_INVALID_ARG for
 * the picture (the reference has one rule). Anything but 0 and 1: MJX_ERR_INVALID_ARG. */
#define MJX_OPTS_COLOR_OFFSET 10
#define MJX_OPTS_COLOR(opts) (((uint8_t *)(opts))[MJX_OPTS_COLOR_OFFSET])

/* The progressive option of a call: byte 11 of mjx_opts, the next padding byte behind MJX_OPTS_COLOR (the struct's members, size and
 * offsets are as they were; a zero-filled struct means what it meant).  An lvalue: MJX_OPTS_PROGRESSIVE(&opts) = 1.  Fill the struct
 * with zeros first and set the byte on the object the call is given: a member-wise copy of the struct need not carry it.
 * 0: everything as in every earlier version, bit for bit -- a progressive frame (SOF2) is MJX_ERR_UNSUPPORTED_FORMAT.  1: SOF2 frames of
 * 8-bit precision with one or three components are accepted (four: MJX_ERR_UNSUPPORTED_FORMAT), in every sampling layout the baseline
 * path takes, with the colour model as for baseline files (MJX_COLOR_FILE included); baseline files decode as they always did.
 * Anything but 0 and 1: MJX_ERR_INVALID_ARG.  Together with strict_ref or MJX_LAYOUT_REF_COMPAT: MJX_ERR_INVALID_ARG for the picture.
 * The scans (at most 255, else MJX_ERR_UNSUPPORTED_FORMAT) follow T.81 G.1.1.1 and libjpeg's coef_bits rule, any violation is
 * MJX_ERR_UNSUPPORTED_FORMAT: a DC scan has Ss = Se = 0 and may interleave components; an AC scan has one component and 1 <= Ss <= Se
 * <= 63; Al <= 13; the first scan of a (component, coefficient) has Ah = 0, every later one Ah = the previous Al and Al = Ah - 1; an AC
 * scan needs the component's first DC scan in front of it; a component without a first DC scan is refused.  A progression that stops
 * early (low bits or bands never sent) is valid and decodes to what was sent, as libjpeg does.  DHT and DRI are those in force at
 * each SOS, a component's DQT the one in force at the first scan that carries it; a slot defined only later is MJX_ERR_MISSING_TABLE.
 * The host de-stuffs the scans and cuts them at their restart markers (device_destuff does not apply, as for multi-scan files).
 * On the device one lane decodes one restart interval of one scan serially (T.81 G.2) into a dense coefficient store; scans that
 * touch no common (component, coefficient) run side by side (levels).  The store is then compacted into the coefficient stream stage
 * B reads, so scales, rectangles, output formats, caller memory, luminance, planes, resize, orientation, MJX_PIXELS_LIBJPEG,
 * keep_coefs and mjx_batch_tile compose as for a gathered multi-scan picture.  Statuses: a lane that runs out of bits before its
 * interval's blocks are complete gives MJX_ERR_TRUNCATED, which wins; a bit pattern that matches no code, or an end-of-band run longer
 * than the blocks left, MJX_ERR_BAD_HUFFMAN; such a picture hands out neither pixels nor coefficients, the others are unaffected. */
#define MJX_OPTS_PROGRESSIVE_OFFSET 11
#define MJX_OPTS_PROGRESSIVE(opts) (((uint8_t *)(opts))[MJX_OPTS_PROGRESSIVE_OFFSET])

/* The inverse DCT of a call: byte 12 of mjx_opts, the next padding byte behind MJX_OPTS_PROGRESSIVE (the struct's members, size and
 * offsets are as they were; a zero-filled struct means what it meant).  An lvalue: MJX_OPTS_IDCT(&opts) = MJX_IDCT_ISLOW.  Fill the
 * struct with zeros first and set the byte on the object the call is given: a member-wise copy of the struct need not carry it.
 * MJX_IDCT_FLOAT (0): stage B's float transform, everything as in every earlier version, bit for bit.  MJX_IDCT_ISLOW (1), with
 * pixels == MJX_PIXELS_LIBJPEG only (without it: MJX_ERR_INVALID_ARG for the picture): libjpeg's integer slow inverse DCT
 * (jidctint.c), so that the picture is byte for byte the one libjpeg and libjpeg-turbo give (Pillow, OpenCV, torchvision's CPU path),
 * not the one up to 3 levels from it.  Anything but 0 and 1: MJX_ERR_INVALID_ARG.  Everything MJX_PIXELS_LIBJPEG refuses stays
 * refused with the same status (MJX_LAYOUT_REF_COMPAT, strict_ref: MJX_ERR_INVALID_ARG; RGB, CMYK and YCCK pictures:
 * MJX_ERR_UNSUPPORTED_FORMAT), scale_denom > 1 included (MJX_ERR_INVALID_ARG) unless the call also sets MJX_OPTS_EXACT_SCALE, which
 * makes scale_denom 2, 4 and 8 libjpeg's own reduced decode (below); a plane description (mjx_planes) together with MJX_IDCT_ISLOW
 * gives the picture MJX_ERR_UNSUPPORTED_FORMAT.
 * The arithmetic, for one 8 x 8 block of one component.  All of it is in 32-bit two's-complement integers that wrap.
 *   d[v][u] = coef[v][u] q[v][u], q the raw DQT entry (8 or 16 bits).
 *   Pass 1 runs P with n = 11 on every column (over v), pass 2 the same P with n = 18 on every row of pass 1's output.
 *   P takes d0 .. d7, FIX(x) = int(x 8192 + 0.5).  Even part:
 *     z1 = (d2 + d6) FIX(0.541196100),  t2 = z1 - d6 FIX(1.847759065),  t3 = z1 + d2 FIX(0.765366865),
 *     t0 = (d0 + d4) 8192,  t1 = (d0 - d4) 8192,  t10 = t0 + t3,  t13 = t0 - t3,  t11 = t1 + t2,  t12 = t1 - t2.
 *   Odd part: a = d7, b = d5, c = d3, e = d1;  z1 = a + e,  z2 = b + c,  z3 = a + c,  z4 = b + e,  z5 = (z3 + z4) FIX(1.175875602);
 *     a *= FIX(0.298631336),  b *= FIX(2.053119869),  c *= FIX(3.072711026),  e *= FIX(1.501321110);
 *     z1 *= -FIX(0.899976223),  z2 *= -FIX(2.562915447),  z3 = z3 (-FIX(1.961570560)) + z5,  z4 = z4 (-FIX(0.390180644)) + z5;
 *     a += z1 + z3,  b += z2 + z4,  c += z2 + z3,  e += z1 + z4.
 *   Outputs: o0 = t10 + e, o7 = t10 - e, o1 = t11 + c, o6 = t11 - c, o2 = t12 + b, o5 = t12 - b, o3 = t13 + a, o4 = t13 - a, each
 *   finished as (o + (1 << (n - 1))) >> n with an arithmetic shift.
 *   The sample is s = clamp(x + 128, 0, 255), x pass 2's output: it saturates (libjpeg's C table wraps modulo 1024; the two agree
 *   for every x in [-512, 511], and libjpeg-turbo's SIMD code saturates).  mjx_idct_islow_host runs exactly this on the CPU.
 * Behind the transform the pipeline is MJX_PIXELS_LIBJPEG's with two changes: there is no rounding constant (the samples are
 * integers already), and a component whose plane has at most two columns (ceil(W h / hmax) <= 2) and whose ratios (rh, rv) are
 * (2, 1) or (2, 2) is replicated in both directions, out[X][Y] = s[X / rh][Y / rv] -- jdsample.c picks its triangle filters only for
 * downsampled_width > 2; (1, 2) keeps its filter at every width.  Without MJX_IDCT_ISLOW MJX_PIXELS_LIBJPEG's own rule stands.
 * Rectangles, output formats, caller memory, luminance, resize, orientation, mjx_batch_tile, the pool, mjx_decode, multi-scan,
 * restart and progressive inputs compose as with MJX_PIXELS_LIBJPEG.
 *
 * At a reduced scale: MJX_PIXELS_LIBJPEG, MJX_IDCT_ISLOW, MJX_OPTS_EXACT_SCALE(&opts) = 1 (byte 13 of mjx_opts, the next padding byte:
 * 0 keeps every earlier behaviour, the refusal of a scale with these pixels included; 1 without MJX_PIXELS_LIBJPEG and MJX_IDCT_ISLOW,
 * or any other value: MJX_ERR_INVALID_ARG; with scale_denom 0 or 1 it changes nothing) and scale_denom = s in {2, 4, 8} give byte for
 * byte the picture libjpeg gives with scale_denom = s (Pillow's draft() / thumbnail(), OpenCV's IMREAD_REDUCED_COLOR_*, torchvision's and DALI's libjpeg back ends).
 * Let m = 8 / s.
 *   1. The picture is ceil(W / s) x ceil(H / s), as for every scaled decode.
 *   2. Component c takes a transform of size N_c (jdmaster.c; one size for both directions): N_c = m, doubled while N_c < 8,
 *      (hmax m) mod (h_c N_c 2) == 0 and (vmax m) mod (v_c N_c 2) == 0; a one-component file has h = v = 1.  Its plane holds
 *      ceil(W h_c N_c / (8 hmax)) x ceil(H v_c N_c / (8 vmax)) samples and is upsampled by rh = hmax m / (h_c N_c),
 *      rv = vmax m / (v_c N_c).  (4:2:0 at 1/2: Y through the 4 x 4 transform, Cb and Cr through the full 8 x 8 one, nothing upsampled.)
 *   3. d[v][u] = coef[v][u] q[v][u] as above, wrapping.
 *   4. The transform (jidctred.c).  D(x, n) = (x + (1 << (n - 1))) >> n, arithmetic; FIX as above; everything wraps.
 *      N = 8: the transform above.
 *      N = 4: R4(d0 .. d7, n): t0 = d0 << 14, t2 = d2 FIX(1.847759065) - d6 FIX(0.765366865), t10 = t0 + t2, t12 = t0 - t2;
 *        with z1 = d7, z2 = d5, z3 = d3, z4 = d1:
 *        a = -z1 FIX(0.211164243) + z2 FIX(1.451774981) - z3 FIX(2.172734803) + z4 FIX(1.061594337),
 *        b = -z1 FIX(0.509795579) - z2 FIX(0.601344887) + z3 FIX(0.899976223) + z4 FIX(2.562915447);
 *        outputs D(t10 + b, n), D(t12 + a, n), D(t12 - a, n), D(t10 - b, n); d4 is never read.  Pass 1 runs R4(., 12) down every
 *        column u != 4 over v, pass 2 R4(., 19) along each of the four rows over u.
 *      N = 2: R2(d, n): t10 = d0 << 15, t0 = -d7 FIX(0.720959822) + d5 FIX(0.850430095) - d3 FIX(1.272758580) + d1 FIX(3.624509785);
 *        outputs D(t10 + t0, n), D(t10 - t0, n).  Pass 1 runs R2(., 13) on columns 0, 1, 3, 5, 7, pass 2 R2(., 20) on the two rows.
 *      N = 1: D(d[0][0], 3).
 *      The sample is clamp(x + 128, 0, 255) as above.  mjx_idct_reduced_host runs exactly this on the CPU.
 *   5. Upsampling.  At s = 2 and 4 the rules above on the scaled planes and the scaled ratios: the triangle filters for (2, 1), (1, 2)
 *      and (2, 2), replication for a ratio of 4, and the narrow-plane rule on the SCALED plane's width.  At s = 8 every component is
 *      replicated whatever its ratios (jdsample.c turns fancy upsampling off when min_DCT_scaled_size is 1).  Then jdcolor.c's colour
 *      step; a one-component picture is its plane.
 * Rectangles are in the coordinates of the scaled picture and are byte for byte its crop; output formats, caller memory, luminance,
 * orientation, an explicit scale with a resize, mjx_batch_tile, mjx_decode and every input path compose.  A resize with auto_scale
 * still picks scale 1 with MJX_PIXELS_LIBJPEG; scale_denom with MJX_PIXELS_LIBJPEG and the float transform, or without
 * MJX_OPTS_EXACT_SCALE, stays MJX_ERR_INVALID_ARG. */
#define MJX_OPTS_EXACT_SCALE_OFFSET 13
#define MJX_OPTS_EXACT_SCALE(opts) (((uint8_t *)(opts))[MJX_OPTS_EXACT_SCALE_OFFSET])
#define MJX_OPTS_IDCT_OFFSET 12
#define MJX_OPTS_IDCT(opts) (((uint8_t *)(opts))[MJX_OPTS_IDCT_OFFSET])
enum {
    MJX_IDCT_FLOAT = 0,       /* stage B's float inverse DCT (every earlier version) */
    MJX_IDCT_ISLOW = 1        /* libjpeg's integer slow inverse DCT: byte-exact libjpeg pixels, with MJX_PIXELS_LIBJPEG only */
};

/* ---- output formats: what a picture leaves as, and where -------------------------------------------------------------
 * Without an output description a picture is packed R,G,B uint8 in the batch's own memory.  With one (mjx_batch_create_out,
 * mjx_decode_batch_out) stage B writes, in its one pass over the pixels, H x W x 3 or 3 x H x W elements of uint8, float16 or
 * float32, channels R,G,B or B,G,R, into the batch's memory or into device memory of the caller's.
 * Values: the u8 value of a sample is exactly the byte the packed decode of the same build writes for that pixel and channel
 * (same scale, same rectangle, STANDARD layout).  U8 outputs are a permutation of those bytes.  F32 is the single-rounded
 * fmaf((float)u8, scale[c], bias[c]), round to nearest even; F16 is that float rounded to nearest even to half.  c is the
 * OUTPUT channel (with bgr, c = 0 is blue).  An element so takes one of 256 values per channel.
 * Ordering: the library writes on streams of its own.  A caller-owned destination must be idle when mjx_batch_decode (or
 * mjx_decode_batch_out) is called and is complete when mjx_batch_wait (mjx_decode_batch_out) returns; nothing is written outside
 * height rows x width elements (3 width interleaved) x 3 channels at the given pitches.
 * Luminance (MJX_OUTPUT_CHANNELS(out) == 1, below): the picture leaves as H x W elements of dtype, one per pixel; chroma is never transformed.  Element
 * (X, Y) of the rectangle (x, y, w, h) lies at dst + (Y - y) row_pitch + (X - x), row_pitch >= width; plane_pitch, planar and bgr have
 * no meaning and are ignored (H x W x 1 and 1 x H x W are the same memory); dense library-owned output has row_pitch = width.  The u8
 * value L is the byte the packed decode of the same build writes into all three channels when the picture's chroma is zero -- the
 * truncating, saturating store applied to the luminance sample stage B computes, + 128 included -- at the call's scale and
 * rectangle; for a one-component file the R byte of the packed decode.  With MJX_PIXELS_LIBJPEG L is component 0's rounded sample,
 * upsampled by its own (rh, rv) with that option's filters where Y is not the most finely sampled component, and there is no
 * colour step.  A float element is fmaf((float)L, scale[0], bias[0]), F16 rounded from that.  Nothing is written outside height rows
 * x width elements. */
enum { MJX_DTYPE_U8 = 0, MJX_DTYPE_F16 = 1, MJX_DTYPE_F32 = 2 };
typedef struct mjx_dst {      /* caller-owned device memory for one picture; pitches in elements */
    void *dev;                /* first element of channel 0, row 0 */
    uint32_t width, height;   /* the picture the caller expects (after scale and rectangle) */
    uint64_t row_pitch;       /* elements between rows: >= width (planar) or >= 3*width (interleaved) */
    uint64_t plane_pitch;     /* planar only: elements between channel planes, >= height*row_pitch */
} mjx_dst;
typedef struct mjx_output {
    uint8_t dtype;            /* MJX_DTYPE_* */
    uint8_t planar;           /* 0: H x W x 3 interleaved, 1: 3 x H x W */
    uint8_t bgr;              /* 0: channel order R,G,B; 1: B,G,R */
    float scale[3], bias[3];  /* F16/F32 only, indexed by OUTPUT channel: value = fmaf((float)u8, scale[c], bias[c]) */
    const mjx_dst *dst;       /* NULL: library-owned, dense (row_pitch = width or 3*width, plane_pitch = height*width) */
    uint32_t n_dst;           /* 0 with dst == NULL, else the call's number of inputs; dst[i] belongs to input i */
} mjx_output;
/* The channel count of an output description: byte 3 of mjx_output, the byte behind `bgr` that the declared members leave unused (the
 * struct's members, size and offsets are as they were; a zero-filled struct means what it meant).  0 or 3: three colour channels;
 * 1: luminance (above); anything else: MJX_ERR_INVALID_ARG for the picture.  An lvalue: MJX_OUTPUT_CHANNELS(&out) = 1.  Fill the
 * struct with zeros first (memset, = {0} on a static, value-initialisation in C++) and set the count on the object the call is given:
 * a member-wise copy of the struct need not carry the byte. */
#define MJX_OUTPUT_CHANNELS_OFFSET 3
#define MJX_OUTPUT_CHANNELS(out) (((uint8_t *)(out))[MJX_OUTPUT_CHANNELS_OFFSET])
/* Per picture, MJX_ERR_INVALID_ARG (nothing is written for it, the others are unaffected): an unknown dtype or channel count;
 * MJX_LAYOUT_REF_COMPAT;
 * dst[i].width / height other than the picture's output size; a pitch too small; dev NULL or not aligned to the element size; a
 * non-finite scale / bias with a float dtype.  n_dst other than 0 or the call's number of inputs, or dst == NULL with n_dst != 0,
 * fails the call.  The description and dst[] are only borrowed for the duration of the call.
 * A batch that carries an output description: mjx_batch_copy_rgb returns MJX_ERR_INVALID_ARG (mjx_batch_copy_output is its
 * counterpart), mjx_batch_compare_rgb reports 0xffffffff for its pictures, mjx_batch_rgb_device gives the output's first byte and
 * the span from there to the end of its last element, mjx_batch_bytes' rgb_bytes counts the bytes written.  mjx_batch_tile keeps
 * a library-owned format and refuses a batch with caller-owned destinations (the copies would share them).  With caller-owned
 * destinations the batch's device block holds no picture pool at all; with library-owned output the pool is sized by the format.
 * YCbCr output is the plane description's (mjx_planes, below).  Not built: mjx_decode and the pool (mjx_pool_decode_batch: the slot -- so the device -- of a file is not known to the
 * caller before the deal) keep packed RGB; the CLI writes packed RGB or, with --luma, the luminance picture. */

/* ---- YCbCr output: the component planes at their own sampling (I420, NV12) ---------------------------------------------
 * With a plane description (mjx_batch_create_planes, mjx_decode_batch_planes) a picture leaves as the planes a JPEG holds -- Y, Cb
 * and Cr, chroma at its own resolution -- not as RGB: no upsampling, no colour arithmetic, 1.5 bytes per pixel for 4:2:0.
 * Geometry.  A picture has ncomp components (1 or 3) with factors (h_c, v_c) and maxima hmax, vmax; its size at the call's
 * scale_denom s is out_w x out_h = ceil(W/s) x ceil(H/s).  Plane c of the whole picture is ceil(out_w h_c / hmax) x
 * ceil(out_h v_c / vmax) samples.  For a rectangle (x, y, w, h) of the out_w x out_h picture (mjx_opts.rois, same rules) plane c
 * covers the columns floor(x h_c / hmax) .. ceil((x + w) h_c / hmax) and the rows floor(y v_c / vmax) .. ceil((y + h) v_c / vmax)
 * of the whole picture's plane: exactly the samples the packed decode of that picture or rectangle reads from component c.  Stage
 * B reads only the tiles that touch the rectangle, as for any cropped picture.  A one-component file has one plane (its factors
 * count as 1 x 1).
 * Values, MJX_PIXELS_REFERENCE: the u8 value of a sample is stage B's truncating, saturating store of the component's float sample
 * + 128, for every component, at every scale.  Said without this code: build the one-component file that carries component c's
 * coefficient blocks and quantisation table; its packed decode at the same scale has the sample in its R byte.  Component 0's plane
 * equals the luminance output (MJX_OUTPUT_CHANNELS == 1) byte for byte wherever Y has the largest factors.
 * Values, MJX_PIXELS_LIBJPEG (full size only, as that option is): the rounded sample clamp(floor(f + 128 + 0.5), 0, 255) -- the
 * planes mjx_opts.pixels describes, in front of its upsampling.
 * Dtypes: U8 as above; F32 is fmaf((float)u8, scale[c], bias[c]), c the COMPONENT; F16 is that float rounded to nearest even.
 * Layout.  Library-owned output is dense, the planes directly behind one another in component order: a u8 4:2:0 picture is an I420
 * frame as it stands.  interleave_chroma = 1 writes Cb and Cr into one plane, element (X, Y) as the pair Cb, Cr at dev[1] +
 * Y row_pitch[1] + 2 X -- NV12's second plane; it needs equal chroma factors and has no meaning for a one-component file.
 * Caller-owned output (dst) takes a pointer and a row pitch, in elements, per plane: a pitch is at least the plane's width (twice
 * the width for the interleaved plane), a pointer is aligned to the element size; dev[2] is ignored with interleave_chroma, dev[1]
 * and dev[2] for a one-component file.  Nothing is written outside each plane's height rows x width elements.  Ordering is
 * mjx_output's: a caller-owned destination is idle at the call and complete when mjx_batch_wait / the pipelined call returns. */
typedef struct mjx_plane_layout {  /* the planes of one picture; pitches in elements */
    void *dev[3];             /* first element of plane c (device memory) */
    uint64_t row_pitch[3];    /* elements between rows of plane c */
    uint32_t width[3], height[3];  /* samples of component c; the interleaved plane 1 has 2 * width[1] elements per row */
} mjx_plane_layout;
typedef struct mjx_planes {
    uint8_t dtype;            /* MJX_DTYPE_* */
    uint8_t interleave_chroma;/* 0: three planes (I420 order); 1: Y, then Cb and Cr interleaved (NV12) */
    float scale[3], bias[3];  /* F16/F32 only, indexed by COMPONENT: value = fmaf((float)u8, scale[c], bias[c]) */
    const mjx_plane_layout *dst;  /* NULL: library-owned, dense, planes back to back */
    uint32_t n_dst;           /* 0 with dst == NULL, else the call's number of inputs; dst[i] belongs to input i */
} mjx_planes;
/* Per picture, MJX_ERR_INVALID_ARG (nothing is written for it, the others are unaffected): an unknown dtype; MJX_LAYOUT_REF_COMPAT;
 * interleave_chroma with unequal chroma factors; dst[i].width / height other than the planes' sizes, or a pitch too small; a
 * pointer NULL or not aligned to the element size; a non-finite scale / bias with a float dtype; MJX_PIXELS_LIBJPEG with
 * scale_denom > 1; the rectangle's own rules.  n_dst other than 0 or the call's number of inputs, dst == NULL with n_dst != 0 or a
 * NULL description fails the call.  The description and dst[] are only borrowed for the duration of the call.
 * A batch that carries a plane description: mjx_batch_copy_rgb returns MJX_ERR_INVALID_ARG (mjx_batch_copy_planes is its
 * counterpart), mjx_batch_compare_rgb reports 0xffffffff, mjx_batch_rgb_device gives the first plane's first byte and the span
 * from there to the last plane's end, mjx_batch_bytes' rgb_bytes counts the bytes written, mjx_batch_image_info, _image_roi and
 * _image_scale are as for a packed picture, mjx_batch_output_channels answers 3, mjx_batch_tile carries the description along
 * (library-owned output only), mjx_batch_copy_coefs is unchanged.
 * Not built: mjx_decode and the pool with planes; a dedicated 4:2:0 plane form (4:2:0 takes the generic form); skipping anything in
 * the entropy stage.
 *
 * Planes with a resize and / or an orientation (mjx_batch_create_planes_orient, mjx_decode_batch_planes_orient; mjx_resize and
 * mjx_orient are described below).  For picture i, c is the resolved orientation code (the file's tag with from_exif, then
 * extra[i]), S the stored picture at the call's scale s, D = orient_c(S) the picture that leaves; rois[i] is in D's coordinates
 * (full-size D with auto_scale), as for every oriented call.
 * The intermediate.  The rectangle is mapped to S (orient_rect_to_stored); with auto_scale s is picked by the resize's rule on the
 * picture-level rectangle and target, the target's axes swapped for codes 5 .. 8, exactly as for an oriented resized picture.  The
 * picture is then planned as the library-owned, dense, uint8, non-interleaved plane decode at (s, R_S): stage B reads only the tiles
 * that touch the rectangle, and its planes P_0 .. P_2 -- plane_span of R_S, as above -- lie in the batch's own memory.
 * Without a resize plane k of the output is orient_c(P_k), the table of mjx_orient applied to the plane as a one-channel picture: for
 * codes 5 .. 8 a plane's width and height swap, so a 4:2:2 file leaves with 4:4:0 planes.  Elements go through the dtype rule above,
 * fmaf((float)u8, scale[k], bias[k]) by COMPONENT; a uint8 output is a permutation of the intermediate's bytes.  With
 * interleave_chroma the pair at (X, Y) of plane 1 is (orient_c(P_1)[Y][X], orient_c(P_2)[Y][X]).
 * With a resize to W x H (D's axes) component k's factors in D are (h_k, v_k) for codes 1 .. 4 and (v_k, h_k) for 5 .. 8, the maxima
 * likewise, and the plane's target is W_k x H_k = ceil(W h'_k / hmax') x ceil(H v'_k / vmax') -- the whole-picture formula above for a
 * W x H picture; a one-component file has one plane, W x H.  Output plane k is mjx_resize's rule applied to orient_c(P_k) as a
 * one-channel picture, n_in -> n_out per axis being the oriented plane's size -> (W_k, H_k): the chosen filter and antialias, float32
 * sums with whole-number numerators and one division, U8 rint clamped, F32 fmaf(v, scale[k], bias[k]) on the unrounded v, F16 that
 * value rounded -- bit for bit what the luminance resize of the one-component file that carries component k's blocks gives for that
 * rectangle and target.  A plane target equal to the oriented plane's own size is bit for bit the un-resized output, in every dtype.
 * Siting: each plane is resampled over its OWN span.  Where the rectangle's edges are not multiples of hmax / h_k (vmax / v_k) the
 * chroma span is the outward-rounded one of plane_span, a little wider than the luma span it belongs to: chroma then registers to
 * luma within less than one chroma sample.  A rectangle aligned to the MCU's chroma grid has no such shift.
 * Fit modes: MJX_FIT_COVER rewrites the rectangle before anything else, so the output is byte for byte the stretch call's on the
 * rewritten rectangle; MJX_FIT_CONTAIN gives the picture MJX_ERR_INVALID_ARG (a pad per component plane is not built).
 * MJX_PIXELS_LIBJPEG composes as it does with planes: full size only, rounded samples; with auto_scale every picture takes scale 1
 * and its rectangle as given, as in any resize call with that option.
 * rs == NULL and orient == NULL: the call plans, launches and writes exactly what mjx_batch_create_planes does; c == 1 without a
 * resize is planned exactly as the planes call (no intermediate, no further launch).
 * Per picture, MJX_ERR_INVALID_ARG (the others unaffected, nothing written): every refusal listed for mjx_planes, mjx_resize and
 * mjx_orient; dst[i].width / height other than the LEAVING planes'; interleave_chroma with unequal chroma factors; MJX_FIT_CONTAIN.
 * Whole-call failures are mjx_orient's and mjx_planes's own.
 * Such a batch: mjx_batch_plane_info and mjx_batch_copy_planes speak of the leaving planes, mjx_batch_image_info of the leaving
 * picture (D's rectangle, or W x H), mjx_batch_image_roi, mjx_batch_resize_rect and mjx_batch_image_scale of the intermediate in S's
 * coordinates, mjx_batch_image_orientation gives c, mjx_batch_bytes' rgb_bytes counts the bytes written, mjx_batch_tile carries
 * everything along (library-owned only).  Not built: MJX_FIT_CONTAIN on planes, per-picture targets, fusing the resize into stage B. */

/* ---- resize on the device: every picture of a call leaves at one target size -------------------------------------------
 * With a resize description (mjx_batch_create_resize, mjx_decode_batch_resize) picture i is decoded as a packed picture at a
 * scale s and a rectangle R (the intermediate: byte for byte what a plain call with scale_denom = s, rois[i] = R writes; it
 * lives in the batch's own memory) and a further kernel resamples it to height x width with the separable triangle filter of
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...): "crop, then resize", taps never reach
 * outside R.  Per axis (n_in -> n_out, r = n_in / n_out, fs = antialias ? max(1, r) : 1), for output coordinate X:
 *   c = (X + 0.5) r,  lo = max(0, floor(c - fs + 0.5)),  hi = min(n_in, floor(c + fs + 0.5)),
 *   w_j = max(0, 1 - |j + 0.5 - c| / fs) for j in [lo, hi), divided by their sum
 * (coordinates in exact integer arithmetic: (2X+1) n_in divided by 2 n_out, quotient and remainder).  The resized sample
 * v = sum_y sum_x wy wx I[y][x][ch] is computed in float32 and is not rounded between the two passes.  The element written:
 * U8 rint (half to even) of v clamped to [0, 255]; F32 fmaf(v, scale[c], bias[c]) on the unrounded v; F16 that float rounded to
 * nearest even; c the OUTPUT channel.  bgr, planar, pitches and caller-owned dst are mjx_output's, at the target size; nothing is
 * written outside height rows x width elements x 3 channels.
 * Scale and rectangle.  auto_scale = 0: s = opts->scale_denom and R = rois[i] (or the whole picture), as in any call.
 * auto_scale = 1: opts->scale_denom must be 0 or 1 and rois[i] = (x, y, w, h) is in FULL-SIZE coordinates; the library picks the
 * largest s in {1, 2, 4, 8} for which R_s = (floor(x/s), floor(y/s), ceil((x+w)/s) - floor(x/s), ceil((y+h)/s) - floor(y/s)) is at
 * least width wide and height high (s = 1 when even that is smaller: the DCT scale never forces an upsample) and R = R_s: a
 * rectangle that is not aligned to s is rounded OUTWARD, by less than s full-size pixels per side.
 * Per picture, MJX_ERR_INVALID_ARG (nothing is written for it, the others are unaffected): width or height 0 (or above 2^24);
 * MJX_LAYOUT_REF_COMPAT; auto_scale with scale_denom > 1; dst[i].width / height other than the target; and mjx_output's and the
 * rectangle's own rules.
 * A resized batch: mjx_batch_image_info and mjx_batch_output_info speak of the target picture, mjx_batch_image_roi gives R's
 * origin and the picture's size at the chosen scale (mjx_batch_resize_rect: all of R), mjx_batch_image_scale the scale,
 * mjx_batch_bytes' rgb_bytes counts the bytes written; mjx_batch_copy_output serves library-owned output; mjx_batch_copy_rgb and
 * mjx_batch_compare_rgb behave as for any batch with an output description; mjx_batch_tile carries the resize along
 * (library-owned output only).  Not built: mjx_decode, the pool and the CLI keep packed RGB. */
typedef struct mjx_resize {
    uint32_t width, height;   /* the target size of every picture of the call */
    uint8_t antialias;        /* 1: the filter widens with the ratio when shrinking (fs = max(1, r)); 0: two taps */
    uint8_t auto_scale;       /* 1: the library picks the DCT-domain scale per picture; rois are in full-size coordinates */
} mjx_resize;
/* The filter kind of a resize description: byte 10 of mjx_resize, one of the two bytes behind `auto_scale` that the declared members
 * leave unused (the struct's members, size and offsets are as they were; a zero-filled struct means what it meant).  An lvalue:
 * MJX_RESIZE_FILTER(&rs) = MJX_FILTER_BICUBIC.  Fill the struct with zeros first (memset, = {0} on a static, value-initialisation
 * in C++) and set the kind on the object the call is given: a member-wise copy of the struct need not carry the byte.  A value
 * above MJX_FILTER_NEAREST gives the picture MJX_ERR_INVALID_ARG (mjx_resize_plan reports it). */
#define MJX_RESIZE_FILTER_OFFSET 10
#define MJX_RESIZE_FILTER(rs) (((uint8_t *)(rs))[MJX_RESIZE_FILTER_OFFSET])
#define MJX_FILTER_TRIANGLE 0   /* the rule above, bit for bit */
#define MJX_FILTER_BICUBIC  1   /* torch's two bicubic rules, picked by `antialias` */
#define MJX_FILTER_NEAREST  2   /* torch's nearest-exact / Pillow's NEAREST; `antialias` is ignored */
/* The other two kinds keep the notation of the rule above -- per axis n_in -> n_out, r = n_in / n_out, c = (X + 0.5) r, coordinates
 * in exact integer arithmetic -- and everything around it: crop, then resize; auto_scale, rectangles, output formats, caller-owned
 * memory, orientation, luminance, MJX_PIXELS_LIBJPEG, mjx_batch_tile and the pipelined calls.  The cubic kernel with parameter a:
 *   k_a(x) = ((a + 2)|x| - (a + 3)) x^2 + 1 for |x| < 1,  a (((|x| - 5)|x| + 8)|x| - 4) for 1 <= |x| < 2,  else 0.
 * Bicubic, antialias = 1 (torch mode="bicubic", antialias=True; Pillow's BICUBIC): a = -0.5, fs = max(1, r),
 *   lo = max(0, floor(c - 2 fs + 0.5)),  hi = min(n_in, floor(c + 2 fs + 0.5)),
 *   w_j = k_a((j + 0.5 - c) / fs) for j in [lo, hi), divided by their sum
 * (the window is clipped at the rectangle's edge and renormalised, as the triangle is).
 * Bicubic, antialias = 0 (torch mode="bicubic", antialias=False, align_corners=False): a = -0.75, s = c - 0.5, q = floor(s) (may
 * be -1), t = s - q; the four taps q - 1 .. q + 2 with the weights k_a(1 + t), k_a(t), k_a(1 - t), k_a(2 - t).  A tap outside
 * [0, n_in) reads the edge sample: its weight is added to the edge sample's, and nothing is renormalised.  This filter does NOT
 * widen when shrinking -- it is torch's behaviour: a picture shrunk by more than about two aliases; ask for antialias = 1 then.
 * Nearest: the one tap j = floor((2X + 1) n_in / (2 n_out)) with weight 1.
 * The weights are evaluated in float32 from the whole-number distance of a tap (the Horner forms above: distances 0, 1 and 2 give
 * exactly 1, 0 and 0).  The sample v = sum_y sum_x wy wx I[y][x][ch] and the element are as above: U8 rint of v clamped to
 * [0, 255] -- bicubic weights are signed, v over- and undershoots, and the clamp acts on both sides --, F32 fmaf(v, scale[c],
 * bias[c]) on the unrounded and UNCLAMPED v (as torch's float path), F16 that float rounded to nearest even.  With nearest every
 * element is mjx_output's table applied to the byte picked, bit for bit; with any kind a target of the rectangle's own size is
 * that table applied to the packed decode, bit for bit.  Not built: Lanczos (its weights need sin(pi x) from one host-and-device
 * routine that gives exact zeros at whole distances: an argument-reduced form of its own). */

/* The fit mode of a resize description: byte 11 of mjx_resize, the last byte the declared members leave unused (the struct's members,
 * size and offsets are as they were; a zero-filled struct means what it meant).  An lvalue: MJX_RESIZE_FIT(&rs) = MJX_FIT_CONTAIN.
 * Fill the struct with zeros first and set the mode on the object the call is given, as for the filter byte: a member-wise copy need
 * not carry it.  A value above MJX_FIT_CONTAIN gives the picture MJX_ERR_INVALID_ARG (the plan functions report it).  Every entry
 * point that takes a resize description carries the mode: mjx_batch_create_resize, mjx_decode_batch_resize, mjx_batch_create_orient,
 * mjx_decode_batch_orient, mjx_resize_plan, mjx_orient_plan. */
#define MJX_RESIZE_FIT_OFFSET 11
#define MJX_RESIZE_FIT(rs) (((uint8_t *)(rs))[MJX_RESIZE_FIT_OFFSET])
#define MJX_FIT_STRETCH 0       /* the rectangle is stretched to the target: the rule above, bit for bit */
#define MJX_FIT_COVER   1       /* centre-crop: the largest centred part of the rectangle with the target's aspect fills the target */
#define MJX_FIT_CONTAIN 2       /* letterbox: the rectangle fits inside the target, the rest is the pad colour */
/* The pad colour of MJX_FIT_CONTAIN: bytes 28, 29 and 30 of mjx_output, the alignment gap between `bias` and `dst` (size, members and
 * offsets as they were; a zero-filled struct pads with black).  MJX_OUTPUT_PAD(&out)[c] = value, c the OUTPUT channel as for scale
 * and bias -- bgr does not reorder the three bytes; luminance output uses byte 0 only.  A padded element is the format's table
 * applied to that byte, exactly what a decoded pixel of that value would become: U8 the byte, F32 fmaf((float)byte, scale[c],
 * bias[c]), F16 that value rounded to nearest even.  out == NULL pads with black; with mean / std black is what Pad(fill=0) before
 * Normalize gives, and the mean colour's bytes give about 0 after normalisation.  The bytes are ignored unless the mode is
 * MJX_FIT_CONTAIN.  Set them on the object the call is given. */
#define MJX_OUTPUT_PAD_OFFSET 28
#define MJX_OUTPUT_PAD(out) ((uint8_t *)(out) + MJX_OUTPUT_PAD_OFFSET)
/* The rule (fit_rule, mjx_kernels.h: the planner and mjx_resize_fit_plan run this one routine).  Per picture
 * A = (x, y, w, h) is the rectangle the call asks for -- rois[i] or the whole picture -- in the coordinates of the picture that
 * leaves (D, after orientation): full size with auto_scale, else at the call's scale.  The target is W x H in D's axes.  Products are
 * 64-bit, round(a / b) = (2a + b) / (2b) in integers, the other divisions floor.
 * MJX_FIT_COVER takes the largest centred part A' of A with the target's aspect:
 *   w H > h W:  w' = clamp(round(h W / H), 1, w),  x' = x + (w - w') / 2,  h and y unchanged;
 *   w H < h W:  h' = clamp(round(w H / W), 1, h),  y' = y + (h - h') / 2,  w and x unchanged;   else A' = A.
 * The picture is then planned exactly as the stretch call with rois[i] = A': orientation mapping, auto_scale with its outward
 * rounding, tiles read and filter taps are that call's, and the output is byte for byte that call's.
 * MJX_FIT_CONTAIN computes the inner size and origin:
 *   w H > h W:  iw = W,  ih = clamp(round(h W / w), 1, H);   w H < h W:  ih = H,  iw = clamp(round(w H / h), 1, W);   else iw = W, ih = H;
 *   ox = (W - iw) / 2,  oy = (H - ih) / 2.
 * The inner rectangle (ox, oy, iw, ih) of the target is exactly what the stretch call with target iw x ih and rois[i] = A writes --
 * with auto_scale the scale is chosen against iw x ih -- bit for bit in every format; every other element of the target is the pad
 * element (k_fit_pad writes the border, behind stage B like the resize).  Only one axis is ever padded.
 * Everything else is the resize's: dst[i].width / height are the target's, mjx_batch_image_info and mjx_batch_output_info speak of
 * the W x H picture, mjx_batch_resize_rect, mjx_batch_image_roi and mjx_batch_image_scale of what was decoded, rgb_bytes counts the
 * whole target, mjx_orient_plan's out_w x out_h are the target (its rectangle and scale, and all of mjx_resize_plan, are the rewritten
 * stretch call's), mjx_batch_tile carries mode and pad along; a picture whose status is not MJX_OK has nothing written, border
 * included; the refusals (MJX_LAYOUT_REF_COMPAT, auto_scale with a scale, planes) are unchanged.
 * Mapping a source coordinate to the output (boxes, key points): with (asked, inner) from mjx_resize_fit_plan, a point (px, py) of D
 * in asked's coordinates lies at  inner.x + (px - asked.x) inner.w / asked.w,  inner.y + (py - asked.y) inner.h / asked.h  of the
 * target (pixel centres: add 0.5 before and take it off after).
 * Not built: per-picture target sizes, a fractional crop ratio, pad modes other than a constant colour, contain for planes. */

/* ---- orientation on the device: EXIF orientation, with per-picture flips on top -----------------------------------------
 * A camera file stores its pixels as the sensor saw them and names, in EXIF tag 0x0112, one of eight ways to turn them upright.
 * S is the stored picture (h rows of w) at the call's scale, D = orient_c(S) the picture that leaves:
 *   code  D[y][x]               size      |  code  D[y][x]               size
 *    1    S[y][x]               w x h     |   5    S[x][y]               h x w
 *    2    S[y][w-1-x]           w x h     |   6    S[h-1-x][y]           h x w
 *    3    S[h-1-y][w-1-x]       w x h     |   7    S[h-1-x][w-1-y]       h x w
 *    4    S[h-1-y][x]           w x h     |   8    S[x][w-1-y]           h x w
 * With an orientation description (mjx_batch_create_orient, mjx_decode_batch_orient) picture i has the resolved code c: the file's
 * own tag (from_exif; mjx_exif_orientation) followed by extra[i] (mjx_orient_compose) -- a horizontal flip as augmentation is
 * extra[i] = 2.  rois[i] is in D's coordinates (full-size D with auto_scale); the planner maps it back to S (full-size S with
 * auto_scale, after which the outward rounding above applies unchanged) and plans the picture as the cropped packed picture at
 * (s, R_S): stage B still reads only the tiles that touch the rectangle, and that packed picture is the intermediate I.
 * Without a resize an element of the output is mjx_output's table applied to the byte of I at the mapped pixel, bit for bit, in
 * every format (U8 outputs are a permutation of I's bytes).  With a resize the output is the resize rule above applied to
 * orient_c(I): axis sizes, taps and mjx_resize_plan's taps_x / taps_y are in D's axes.
 * c == 1 without a resize: the picture is planned exactly as mjx_batch_create_out plans it (no intermediate, no further launch);
 * c == 1 with a resize: exactly as mjx_batch_create_resize.  A batch built through these entry points always carries an output
 * description: out == NULL is interleaved u8 R,G,B, library-owned.
 * Per picture, MJX_ERR_INVALID_ARG (the others are unaffected): a code outside 1 .. 8 in extra; a rectangle outside D;
 * MJX_LAYOUT_REF_COMPAT with c != 1; dst[i] of another size than D's rectangle or the target; and the rules above.  n_extra other
 * than 0 or the call's number of inputs, or extra == NULL with n_extra != 0, fails the call.
 * An oriented batch: mjx_batch_image_info and mjx_batch_output_info speak of the picture that leaves, mjx_batch_image_roi and
 * mjx_batch_resize_rect stay in S's coordinates (they describe the intermediate), mjx_batch_image_orientation gives c;
 * mjx_batch_tile carries the code along (library-owned output only).  Not built: mjx_decode, the pool and the CLI do not turn. */
typedef struct mjx_orient {
    uint8_t from_exif;        /* 1: picture i starts from the code mjx_exif_orientation finds in file i */
    const uint8_t *extra;     /* NULL, or one code 1..8 per input, applied AFTER the EXIF one (mjx_orient_compose) */
    uint32_t n_extra;         /* 0 with extra == NULL, else the call's number of inputs */
} mjx_orient;

/* ---- inner seam: what jpeg/mod.rs:388-415 hands to JPEGDecoder -------------------------- */
/* Sampling factors: h and v are each 1, 2 or 4 -- 4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1 (Y 4x1), 4:1:0 (Y 4x2), their vertical forms and
 * every mixed layout.  Three components: at most 12 blocks per MCU (sum of h v; T.81 B.2.3 says 10, files with 11 and 12 exist);
 * four components (MJX_COLOR_FILE): at most 10; one component: any of the factors, the scan is non-interleaved and decodes as
 * h = v = 1 in the STANDARD layout.  An MCU covers 8 hmax x 8 vmax pixels, up to 32 x 32; pixel (X, Y) takes sample
 * (floor(X h / hmax), floor(Y v / vmax)) of each component (box replication).  A factor of 3, or above 4, is
 * MJX_ERR_UNSUPPORTED_FORMAT: strips per MCU row and replication by shifts need powers of two, and the pixel forms hold 32 x 32.
 * The reference asserts 1 or 2 (mod.rs:275-277): strict_ref and MJX_LAYOUT_REF_COMPAT answer a 4 with MJX_ERR_REF_PANIC. */
typedef struct mjx_comp {          /* decoder.rs:39-52 JPEGDecoderComponentFields */
    uint8_t id, h, v, tq, td, ta;
} mjx_comp;

typedef struct mjx_hufftab {       /* the two slices given to HuffmanTable::from_size_data_tables, huffman.rs:37 */
    uint8_t bits[16];
    uint8_t vals[256];
} mjx_hufftab;

/* One scan of a multi-scan baseline file: a single component (non-interleaved order, T.81 A.2.2) or an interleaved
 * subset of the frame's components ("0; 1 2;", the separate-luma-and-chroma script of libjpeg's wizard.txt) -- beyond the
 * reference, which stops after the first SOS (jpeg/mod.rs:415-417).  SURVEY s8(f)-4. */
typedef struct mjx_scan_part {
    const uint8_t *scan;           /* this scan's entropy-coded segment, de-stuffed, RSTn taken out */
    size_t scan_len;
    uint8_t ncomp;                 /* components in this scan: 1 or 2 */
    uint8_t comp[3];               /* their indices into mjx_scan_desc.comp, scan order */
    uint16_t restart_interval;     /* MCUs (single component: blocks) per restart interval as defined when the SOS was read */
    uint32_t n_restart;
    const uint32_t *restart_offsets;
    mjx_hufftab dc[3], ac[3];      /* per component of the scan: the tables it selects, as defined when the SOS was read */
} mjx_scan_part;

/* One scan of a progressive file (mjx_scan_desc.prog): spectral selection Ss .. Se, successive approximation Ah, Al (T.81 G.1.1.1) */
typedef struct mjx_scan_prog { uint8_t ss, se, ah, al; } mjx_scan_prog;

typedef struct mjx_scan_desc {
    const uint8_t *scan;           /* bytes after the SOS header to end of file, de-stuffed (jpeg/mod.rs:371-385) unless
                                      scan_is_stuffed */
    size_t scan_len;
    uint16_t width, height;        /* .dimensions() decoder.rs:66 */
    uint8_t ncomp;                 /* 1 or 3; 4 with MJX_COLOR_FILE (the fourth component is comp_fourth, at the struct's end) */
    mjx_comp comp[3];              /* scan order (decoder.rs:141-150) */
    uint16_t qt[4][64];            /* zig-zag (file) order as in DQT, jpeg/mod.rs:236-256; .quantization_table() */
    uint8_t qt_present;            /* bit i = slot i defined */
    mjx_hufftab dc[4], ac[4];      /* .huffman_dc_tables() / .huffman_ac_tables() decoder.rs:71-77 */
    uint8_t dc_present, ac_present;
    uint8_t scan_is_stuffed;       /* 1: `scan` still holds FF00 pairs and RSTn markers, scan_len is the stuffed length and
                                      restart_offsets is empty: the device de-stuffs, finds the markers and the length */
    /* Restart intervals (T.81 B.2.4.4) -- beyond the reference, which panics on DRI (jpeg/mod.rs:424-428; strict_ref keeps
       that).  mjx_parse removes the RSTn markers from `scan` and lists where each further interval begins. */
    uint16_t restart_interval;     /* MCUs per interval, 0 = none */
    uint32_t n_restart;            /* entries of restart_offsets */
    const uint32_t *restart_offsets; /* byte offset in `scan` of the first byte of interval 1, 2, ... (interval 0 starts at 0) */
    /* Multi-scan files: n_parts > 0 means `scan` is NULL, `comp` lists the frame's components in frame order and every
       component is carried by exactly one of `parts`; the dc / ac slots above are not used.  DQT, DHT and DRI segments may
       stand between the scans (T.81 B.2.4): a part keeps the Huffman tables and the restart interval in force at its SOS, and a
       component keeps the quantisation table its slot holds when the scan that carries it starts (libjpeg's rule; a DQT
       further on does not change it, a slot not defined by then is MJX_ERR_MISSING_TABLE).  mjx_parse puts component c's
       table in qt[c] and sets comp[c].tq = c (qt_present = 7, qt[3] zero). */
    uint8_t n_parts;
    const mjx_scan_part *parts;
    void *owner_;                  /* internal: storage behind `scan` / `parts` when filled by mjx_parse */
    /* MJX_COLOR_FILE (appended: every offset above is as before).  comp_fourth: the fourth component of a four-component scan, scan
       order, behind comp[0 .. 2].  model: MJX_MODEL_* as mjx_parse decided it with MJX_COLOR_FILE; with MJX_COLOR_POSITIONAL -- and
       in a zero-filled struct a caller fills by hand -- MJX_MODEL_GREY (0), which for three components means Y, Cb, Cr by
       position.  A four-component description needs MJX_MODEL_CMYK or MJX_MODEL_YCCK. */
    mjx_comp comp_fourth;
    uint8_t model;
    /* MJX_OPTS_PROGRESSIVE (appended: every offset above is as before).  NULL: a baseline file -- every hand-filled or zero-filled
       description means what it meant.  Else the file is progressive (SOF2): prog[k] holds Ss, Se, Ah, Al of parts[k], n_parts is 1 ..
       255, ncomp 1 or 3, a part's ncomp is 1 .. 3 (an interleaved DC scan), its dc[q] counts for a first DC scan and its ac[0] for an
       AC scan, its restart interval counts MCUs (interleaved) or blocks of the component's own grid.  mjx_validate applies the rules of
       MJX_OPTS_PROGRESSIVE to a hand-filled description. */
    const mjx_scan_prog *prog;
} mjx_scan_desc;

/* ---- outer surface ------------------------------------------------------------------------ */
typedef struct mjx_image {         /* JPEGImage: width() mod.rs:467, height() :471, image_data() :475 */
    uint32_t width, height;
    uint8_t *rgb;                  /* width*height*3 bytes, R,G,B, row-major, unpadded; NULL on error */
} mjx_image;

/* JPEGImage::parse, jpeg/mod.rs:202 -- host-side marker walk only (no GPU): fills the POD the decoder needs
 * exactly as mod.rs:228-362 does, de-stuffs the scan (mod.rs:371-385).  Release with mjx_free_scan. */
int mjx_parse(const uint8_t *jpeg, size_t len, const mjx_opts *opts, mjx_scan_desc *out);
void mjx_free_scan(mjx_scan_desc *desc);

/* Host-only: the EXIF orientation of a file.  Walks the markers up to the first SOS, takes the first APP1 whose payload starts
 * "Exif\0\0", reads the TIFF header (either byte order) and IFD0 and looks for tag 0x0112 of type SHORT, count 1.  Everything else --
 * no such segment, no tag, another type or count, a value outside 1 .. 8, an offset or an entry count that points outside the
 * segment, a file that ends inside it -- gives *code = 1 and MJX_OK; nothing outside [jpeg, jpeg + len) is read.  Only NULL arguments
 * are an error.  mjx_parse is not involved (it skips APP1; with strict_ref it still refuses it). */
int mjx_exif_orientation(const uint8_t *jpeg, size_t len, uint8_t *code);
/* Host-only: what the components of a file are under MJX_COLOR_FILE (MJX_OPTS_COLOR has the rule).  Walks the markers up to the first
 * SOS, notes JFIF APP0 and Adobe APP14 segments and the first SOF's component ids.  A file without a frame of 1, 3 or 4 components in
 * front of its first SOS, or one that ends inside a segment, gives MJX_ERR_UNSUPPORTED_FORMAT (out is zero-filled); nothing outside
 * [jpeg, jpeg + len) is read.  mjx_parse with MJX_COLOR_FILE decides with the same routine. */
typedef struct mjx_color_info {
    uint8_t model;            /* MJX_MODEL_* */
    uint8_t ncomp;            /* components of the frame */
    uint8_t jfif;             /* 1: a JFIF APP0 segment was seen */
    uint8_t adobe;            /* 1: an Adobe APP14 segment was seen */
    uint8_t adobe_transform;  /* its transform byte (0 without one) */
    uint8_t ids[4];           /* the frame's component ids, frame order */
} mjx_color_info;
int mjx_color_model(const uint8_t *jpeg, size_t len, mjx_color_info *out);
/* mul(a, k) = (a k + 127) / 255 of MJX_OPTS_COLOR: the routine the kernels run (ink_mul, mjx_kernels.h).  Equal to Pillow's
 * CMYK -> RGB conversion on all 65 536 pairs. */
uint8_t mjx_ink_mul(uint8_t a, uint8_t k);
/* The one code that does what `first` followed by `then` does; 0 when either lies outside 1 .. 8. */
uint8_t mjx_orient_compose(uint8_t first, uint8_t then);

/* Host-only check of a parsed scan: tables present and valid, geometry supported and, for MJX_LAYOUT_REF_COMPAT, not
 * one of the inputs on which the reference's placement code panics (decoder.rs:300-303, 370-371; SURVEY Q5 ->
 * MJX_ERR_REF_PANIC).  The same check mjx_batch_create applies per image. */
int mjx_validate(const mjx_scan_desc *desc, const mjx_opts *opts);

/* Host-only: the stage-B tiles a decode of this picture with these options reads.  A tile is *tile_mcus consecutive MCUs in raster
 * order; with a rectangle (opts->rois[0]) stage B fetches and transforms only the tiles that hold an MCU of the rectangle's MCU
 * rows and columns -- *tiles_read of the picture's *tiles_total.  Multi-scan pictures that are read straight from their scans'
 * streams skip by MCU rows only: every tile from the first to the last one that touches the rectangle's MCU rows is read.
 * The numbers come from the planner and the tile rule of the kernels themselves.  Returns the picture's plan status. */
int mjx_plan_tiles(const mjx_scan_desc *desc, const mjx_opts *opts, uint64_t *tiles_read, uint64_t *tiles_total,
                   uint32_t *tile_mcus);

/* JPEGImage::parse + image_data() in one call on device `0` (main.rs:31-36 usage): parse, upload, decode on the
 * GPU, copy the RGB back.  Release with mjx_free_image. */
int mjx_decode(const uint8_t *jpeg, size_t len, const mjx_opts *opts, mjx_image *out);
void mjx_free_image(mjx_image *img);

/* ---- batch / device-resident API (one context per process per GPU) ------------------------ */
typedef struct mjx_ctx mjx_ctx;
typedef struct mjx_batch mjx_batch;

int mjx_ctx_create(int device, mjx_ctx **out);
void mjx_ctx_destroy(mjx_ctx *ctx);
/* 1: record HIP events around every kernel class of mjx_batch_decode (read with mjx_batch_kernel_ms) */
int mjx_ctx_set_profiling(mjx_ctx *ctx, int enable);
/* 1: batches of this context are always cut for throughput (512-byte subsequences).  By default a batch too small to fill the
 * device is cut into shorter subsequences, which shortens its latency; a caller that builds a small batch only to replicate
 * it on the device (mjx_batch_tile keeps the base's cut) switches that off, so that the large batch is cut like one that
 * was created at its size.  Also the first mjx_decode_batch / mjx_batch_create on a fresh context allocates its device
 * block and pinned buffers: expect that call to take several times as long as the ones after it (0.5 s against 50 ms for
 * 2048 4K files). */
int mjx_ctx_set_throughput_plan(mjx_ctx *ctx, int enable);
/* NUMA node of the context's GPU (from the PCI device's numa_node in sysfs), -1 when the platform does not say. */
int mjx_ctx_numa_node(const mjx_ctx *ctx);
/* Processors this process may use: the affinity mask, capped by the cgroup CPU quota. */
unsigned mjx_host_processors(void);

/* JPEGDecoder::new(..).frame_header(..).scan_header(..).dimensions(..) + table setters for n images
 * (decoder.rs:55-152): validates, builds decode tables, packs and uploads the scans; device buffers for the
 * outputs are allocated here.  status[i] (optional) receives the per-image code; images with an error are
 * skipped by decode and produce no output.  Inputs are only borrowed for the duration of the call. */
int mjx_batch_create(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts,
                     mjx_batch **out, int *status);
void mjx_batch_free(mjx_batch *b);
/* mjx_batch_create with an output description (above); out == NULL: mjx_batch_create itself. */
int mjx_batch_create_out(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts, const mjx_output *out,
                         mjx_batch **b, int *status);
/* Host-only, in the spirit of mjx_plan_tiles: what a decode of this picture as input i of a call with these options and this
 * description would write -- size, pitches, for a caller-owned destination dst[i]'s own -- and *bytes, the span from the first
 * element's first byte to the last element's last.  layout->dev stays NULL for library-owned output.  out == NULL: the packed
 * picture (interleaved u8, width * height * 3 bytes).  The numbers come from the planner itself.  Returns the picture's status. */
int mjx_output_layout(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_output *out, size_t i, mjx_dst *layout,
                      size_t *bytes);
/* The output of picture i of a batch: where it lies (layout->dev: device pointer), its pitches and its format.  A batch without
 * an output description answers with the packed picture's (u8, interleaved, R,G,B). */
int mjx_batch_output_info(const mjx_batch *b, size_t i, mjx_dst *layout, uint8_t *dtype, uint8_t *planar, uint8_t *bgr);
/* The channels picture i leaves with: 1 for a luminance picture (MJX_OUTPUT_CHANNELS == 1), 3 for every other batch. */
int mjx_batch_output_channels(mjx_batch *b, size_t i, uint8_t *channels);
/* Copy picture i's library-owned output to host memory, dense, as mjx_output_layout sizes it; cap_bytes smaller than that, a
 * caller-owned destination or a batch without an output description: MJX_ERR_INVALID_ARG. */
int mjx_batch_copy_output(mjx_batch *b, size_t i, void *host, size_t cap_bytes);

/* mjx_batch_create with a plane description (YCbCr output, above): the pictures leave as their component planes.  planes == NULL:
 * MJX_ERR_INVALID_ARG. */
int mjx_batch_create_planes(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts, const mjx_planes *planes,
                            mjx_batch **b, int *status);
/* Host-only, from the planner itself, like mjx_output_layout: the planes a decode of this picture as input i of a call with these
 * options and this description would write -- *nplanes of them (1 for a one-component file, 3, or 2 with interleave_chroma), per
 * component width and height in samples, per plane its pitch in elements (a caller-owned plane: dst[i]'s own pitch and pointer;
 * layout->dev stays NULL for library-owned output) -- and *bytes, the planes' spans added up (dense library-owned output: the
 * whole of it, what mjx_batch_copy_planes copies).  Returns the picture's status. */
int mjx_planes_layout(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_planes *planes, size_t i, mjx_plane_layout *layout,
                      uint32_t *nplanes, size_t *bytes);
/* The planes of picture i of a batch with a plane description: their number, device pointers, pitches, sizes, dtype and whether
 * chroma is interleaved.  A batch without a plane description: MJX_ERR_INVALID_ARG. */
int mjx_batch_plane_info(const mjx_batch *b, size_t i, uint32_t *nplanes, mjx_plane_layout *layout, uint8_t *dtype, uint8_t *interleave);
/* Copy picture i's library-owned planes to host memory, dense, planes back to back, as mjx_planes_layout sizes them; cap_bytes
 * smaller than that, caller-owned planes or a batch without a plane description: MJX_ERR_INVALID_ARG. */
int mjx_batch_copy_planes(mjx_batch *b, size_t i, void *host, size_t cap_bytes);
/* mjx_batch_create_planes with a resize and / or an orientation description (planes with a resize and / or an orientation, above);
 * rs == NULL and orient == NULL: mjx_batch_create_planes itself.  from_exif = 1 is MJX_ERR_INVALID_ARG for the call, as in
 * mjx_batch_create_orient: descriptors carry no file bytes. */
int mjx_batch_create_planes_orient(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts, const mjx_planes *planes,
                                   const mjx_resize *rs, const mjx_orient *orient, mjx_batch **b, int *status);
/* Host-only, from the planner itself (the routine the two calls above plan with): picture `desc` as input i of a call with these
 * options (rois[i], or rois[0] when n_rois <= 1), this plane description, this resize (or NULL) and the resolved code `code` -- the
 * LEAVING planes' sizes and pitches (library-owned planes are dense and back to back in plane order: the pitch is the row and
 * layout->dev stays NULL; caller-owned: dst[i]'s own pitches and pointers), the scale the picture is decoded at and the rectangle of
 * the stored picture its intermediate covers at that scale.  With rs == NULL and code == 1 the layout is mjx_planes_layout's member
 * for member.  Returns the picture's status. */
int mjx_planes_orient_layout(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_planes *planes, const mjx_resize *rs, uint8_t code,
                             size_t i, mjx_plane_layout *layout, uint8_t *scale_denom, mjx_rect *rect);

/* mjx_batch_create_out with a resize description (above); rs == NULL: mjx_batch_create_out itself.  out == NULL with a resize:
 * interleaved u8 R,G,B, library-owned. */
int mjx_batch_create_resize(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts, const mjx_output *out,
                            const mjx_resize *rs, mjx_batch **b, int *status);
/* Host-only, from the planner itself, in the spirit of mjx_plan_tiles: the scale and the rectangle (at that scale) picture `desc`
 * is decoded at as input i of a call with these options (rois[i], or rois[0] when n_rois <= 1) and this resize, and the largest
 * number of taps of an output column / row (what the resize kernel's loops run to).  Returns the picture's status. */
int mjx_resize_plan(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_resize *rs, size_t i, uint8_t *scale_denom,
                    mjx_rect *rect, uint32_t *taps_x, uint32_t *taps_y);
/* Host-only, the planner's own rule (fit_rule): picture `desc` as input i of a call with these options, this output description (its
 * pad bytes are not looked at; NULL is fine), this resize and the resolved orientation code -- *inner: the inner rectangle in the
 * target (the whole target for MJX_FIT_STRETCH and MJX_FIT_COVER); *asked: A' for MJX_FIT_COVER and A otherwise, in D's coordinates at
 * full size (auto_scale) or at the call's scale; *scale_denom: the scale the picture is decoded at.  Returns the picture's status. */
int mjx_resize_fit_plan(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_output *out, const mjx_resize *rs, uint8_t orient_code,
                        size_t i, mjx_rect *inner, mjx_rect *asked, uint8_t *scale_denom);
/* Host-only: the filter of one output coordinate X of an axis n_in -> n_out -- the routine the resize kernel itself runs
 * (resize_axis / resize_weight, mjx_kernels.h).  *first: the first tap's input index, weights[0 .. *count): the normalised weights
 * (at most cap are written; *count is the window's length either way).  n_in, n_out in 1 .. 2^24, X < n_out. */
int mjx_resize_weights(uint32_t n_in, uint32_t n_out, int antialias, uint32_t X, uint32_t *first, float *weights, size_t cap,
                       size_t *count);
/* mjx_resize_weights with the filter kind (MJX_FILTER_*; the routines the bicubic and nearest kernels run: resize_taps,
 * mjx_kernels.h); filter 0 is mjx_resize_weights itself.  Bicubic with antialias = 0 returns the folded weights over the clipped
 * window -- a tap outside [0, n_in) added to the edge sample's --, so *first + *count <= n_in as for every kind.  An unknown filter:
 * MJX_ERR_INVALID_ARG. */
int mjx_resize_filter_weights(uint32_t n_in, uint32_t n_out, int filter, int antialias, uint32_t X, uint32_t *first, float *weights,
                              size_t cap, size_t *count);
/* Host-only: MJX_PIXELS_LIBJPEG's upsampling and colour step on the CPU -- the routines k_upsample_color itself runs (lj_strip8 /
 * lj_color, mjx_kernels.h).  ncomp (1 or 3) dense planes of cw[c] x ch[c] samples, upsampled by rh[c], rv[c] (each 1, 2 or 4); rgb receives
 * the rectangle's rect->w x rect->h pixels, packed R,G,B.  The rectangle must lie inside every upsampled plane (cw[c] rh[c] x
 * ch[c] rv[c]); the plane of an odd picture is one sample short of the picture's size, which the rule allows.
 * MJX_UPSAMPLE_REPLICATE or-ed into rh[c] (the planner's flag for MJX_IDCT_ISLOW's planes of at most two columns): component c is
 * replicated in both directions, out[X][Y] = s[X / rh][Y / rv], whatever its ratios. */
#define MJX_UPSAMPLE_REPLICATE 0x80
int mjx_upsample_color_host(const uint8_t *const *planes, const uint32_t *cw, const uint32_t *ch, const uint8_t *rh, const uint8_t *rv,
                            uint32_t ncomp, const mjx_rect *rect, uint8_t *rgb);
/* Host-only: MJX_PIXELS_LIBJPEG's luminance picture (MJX_OUTPUT_CHANNELS == 1) on the CPU -- the routine k_upsample_luma itself runs
 * (lj_luma8, mjx_kernels.h).  One dense plane of cw x ch samples, upsampled by rh, rv (each 1, 2 or 4; 1, 1: the plane itself); out receives
 * the rectangle's rect->w x rect->h bytes.  The rectangle must lie inside the upsampled plane.  MJX_UPSAMPLE_REPLICATE in rh: as above. */
int mjx_upsample_luma_host(const uint8_t *plane, uint32_t cw, uint32_t ch, uint8_t rh, uint8_t rv, const mjx_rect *rect, uint8_t *out);
/* Host-only: MJX_IDCT_ISLOW's transform of one block on the CPU -- the lane routine stage B's integer sink itself runs
 * (idct_islow_inplace, mjx_kernels.h).  coef: the 64 coefficients, q: the 64 raw DQT entries, out: the 64 samples
 * clamp(x + 128, 0, 255), all three in natural (row-major, [v][u]) order. */
int mjx_idct_islow_host(const int16_t coef[64], const uint16_t q[64], uint8_t out[64]);
/* Host-only, from the planner itself: the geometry of MJX_IDCT_ISLOW's planes for this picture and these options -- per component the
 * transform's size N_c (8 without MJX_OPTS_EXACT_SCALE and a scale), the plane's samples, the upsampling ratios, the row stride of the
 * plane in the library's scratch and whether the component is replicated (the narrow-plane rule; every component at 1/8).  Any
 * pointer may be NULL.  A picture without MJX_PIXELS_LIBJPEG and MJX_IDCT_ISLOW: MJX_ERR_INVALID_ARG; else the picture's status. */
int mjx_plan_reduced(const mjx_scan_desc *desc, const mjx_opts *opts, uint32_t *ncomp, uint32_t size[3], uint32_t plane_w[3],
                     uint32_t plane_h[3], uint32_t rh[3], uint32_t rv[3], uint32_t stride[3], uint32_t replicated[3]);
/* ... and of its reduced siblings at scale_denom 2, 4, 8 (the lane routines stage B runs there): N = 8, 4, 2 or 1, the size of the
 * component's transform; out holds the N x N samples, rows of N.  Any other N: MJX_ERR_INVALID_ARG. */
int mjx_idct_reduced_host(const int16_t coef[64], const uint16_t q[64], uint32_t N, uint8_t *out);

/* mjx_batch_create_resize with an orientation description (above); orient == NULL: mjx_batch_create_resize itself.  Descriptors
 * carry no file bytes: from_exif = 1 is MJX_ERR_INVALID_ARG for the call -- read the tag with mjx_exif_orientation and pass it in
 * extra. */
int mjx_batch_create_orient(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts, const mjx_output *out,
                            const mjx_resize *rs, const mjx_orient *orient, mjx_batch **b, int *status);
/* Host-only, from the planner itself, in the spirit of mjx_plan_tiles: picture `desc` as input i of a call with these options, this
 * resize (or NULL) and the resolved code `code` -- the size of the picture that leaves, the rectangle of the stored picture its
 * intermediate covers (at the scale it is decoded at) and that scale.  Returns the picture's status. */
int mjx_orient_plan(const mjx_scan_desc *desc, const mjx_opts *opts, const mjx_resize *rs, uint8_t code, size_t i, uint32_t *out_w,
                    uint32_t *out_h, mjx_rect *stored_rect, uint8_t *scale_denom);

/* Replicate the uploaded images `times`x on the device (image i*n+k is a byte copy of image k): builds the
 * large synthetic batches of BASELINE.json configs 4/5 from n unique images without re-uploading.  The copies keep their
 * source's scale and rectangle. */
int mjx_batch_tile(mjx_ctx *ctx, const mjx_batch *src, size_t times, mjx_batch **out);

/* JPEGDecoder::decode, decoder.rs:162 -- the hot path.  Enqueues every kernel for the whole batch on the
 * context's stream and returns; inputs and outputs stay in HBM.  stages: MJX_STAGE_* mask (0 = all). */
enum { MJX_STAGE_ENTROPY = 1, MJX_STAGE_PIXELS = 2, MJX_STAGE_ALL = 3 };
int mjx_batch_decode(mjx_batch *b, unsigned stages);
/* Block until the stream is idle; fold device-side error flags into the per-image status. */
int mjx_batch_wait(mjx_batch *b);

size_t mjx_batch_size(const mjx_batch *b);
int mjx_batch_status(const mjx_batch *b, size_t i);
/* geometry of image i: width, height, number of blocks per MCU, MCUs decoded */
int mjx_batch_image_info(const mjx_batch *b, size_t i, uint32_t *width, uint32_t *height, uint32_t *blocks_per_mcu,
                         uint32_t *mcus);
/* region-of-interest decode: the origin of image i's rectangle and the size of the uncropped picture (out_w x out_h at the
 * batch's scale); without a rectangle 0, 0 and the picture's own size */
int mjx_batch_image_roi(const mjx_batch *b, size_t i, uint32_t *x, uint32_t *y, uint32_t *full_width, uint32_t *full_height);
/* the DCT-domain scale picture i was decoded at (1, 2, 4 or 8): the call's, or the one auto_scale picked */
int mjx_batch_image_scale(const mjx_batch *b, size_t i, uint8_t *scale_denom);
/* the colour model of picture i (MJX_MODEL_*; with MJX_COLOR_POSITIONAL grey for one component, YCbCr for three) */
int mjx_batch_image_color(const mjx_batch *b, size_t i, uint8_t *model);
/* the orientation code picture i left with (1 .. 8: the file's tag followed by extra[i]; 1 for any batch without an orientation) */
int mjx_batch_image_orientation(const mjx_batch *b, size_t i, uint8_t *code);
/* a resized batch: the rectangle R picture i's intermediate covers, in the coordinates of the picture at its scale
 * (mjx_batch_image_roi: that picture's size); any other batch: the picture's own rectangle */
int mjx_batch_resize_rect(const mjx_batch *b, size_t i, mjx_rect *rect);
/* a resized batch: the inner rectangle of picture i in its target -- the part the picture fills; (0, 0, W, H) for MJX_FIT_STRETCH and
 * MJX_FIT_COVER, the letterboxed part for MJX_FIT_CONTAIN; (0, 0, 0, 0) for a batch without a resize */
int mjx_batch_fit_rect(const mjx_batch *b, size_t i, mjx_rect *inner);
/* device pointer + byte size of image i's packed RGB (valid until mjx_batch_free) */
int mjx_batch_rgb_device(const mjx_batch *b, size_t i, void **dev_ptr, size_t *bytes);
/* copy image i's RGB to host memory (width*height*3 bytes) */
int mjx_batch_copy_rgb(mjx_batch *b, size_t i, uint8_t *host_rgb);
/* T0 stream of image i (needs keep_coefs, or i inside the last decoded chunk): blocks in decode (MCU-interleaved)
 * order, 64 x i16 zig-zag, DC prediction applied, before dequantisation.  `cap_blocks` = capacity of host buffer.
 * A multi-scan picture needs keep_coefs: without it its coefficients only exist scan by scan (stage B reads them from the
 * scans' streams) and the call returns MJX_ERR_INVALID_ARG. */
int mjx_batch_copy_coefs(mjx_batch *b, size_t i, int16_t *host_coefs, size_t cap_blocks, size_t *nblocks);

/* Verification helper (bench.py's parity gate, batch-scale tests): compares the decoded RGB of n pairs of pictures on the
 * device -- picture ia[k] of batch a with picture ib[k] of batch b (same device; a == b is fine) -- without copying them
 * to the host.  Per pair: the largest absolute difference of a byte and the number of differing bytes; a pair whose
 * pictures differ in size, or either of which failed to decode, reports max_abs_diff = 0xffffffff. */
int mjx_batch_compare_rgb(mjx_batch *a, const size_t *ia, mjx_batch *b, const size_t *ib, size_t n,
                          uint32_t *max_abs_diff, uint64_t *n_diff);

/* bytes used to compute roofline figures: sum of de-stuffed entropy bytes and of RGB bytes over valid images */
int mjx_batch_bytes(const mjx_batch *b, uint64_t *scan_bytes, uint64_t *rgb_bytes, uint64_t *coef_bytes,
                    uint64_t *pixels);

/* work units of the batch (valid images): subsequences the entropy stage decodes in parallel (512..640 bytes of scan each,
 * chosen per image), coefficient blocks, and the kernel chunks the batch is processed in (one launch per kernel class and chunk) */
int mjx_batch_geometry(const mjx_batch *b, uint64_t *subsequences, uint64_t *blocks, uint64_t *chunks);

/* Runs of a chunk, since the batch was created, whose synchronisation rounds had not converged when the rest of the entropy stage
 * was enqueued behind them: the chunk's pictures were skipped in that run -- and runs in which a picture left the single-decode
 * path on the device (it is skipped by the rest of that run too).  mjx_batch_wait examines and repairs the LAST decode
 * only, so a caller that enqueues several mjx_batch_decode calls before one wait (a throughput measurement) reads here whether
 * every one of them did the whole work.  Synchronises the batch's streams. */
int mjx_batch_unconverged_runs(const mjx_batch *b, uint64_t *runs);

/* accumulated kernel time (ms) and launch count per kernel class since the last reset (profiling enabled) */
enum {
    MJX_K_GATHER = 0,     /* multi-scan pictures only: component streams -> the picture's stream (k_planar_*) */
    MJX_K_HUFF_SYNC = 1,  /* speculative decode + intra-workgroup synchronisation */
    MJX_K_HUFF_FIX = 2,   /* inter-workgroup synchronisation passes */
    MJX_K_HUFF_SCAN = 3,  /* block-count prefix sums */
    MJX_K_HUFF_WRITE = 4, /* final decode writing coefficients */
    MJX_K_DC_SCAN = 5,    /* DC prediction prefix sums */
    MJX_K_IDCT_COLOR = 6, /* dequant + IDCT + upsample + colour + RGB store */
    MJX_K_UPLOAD = 7,     /* upload time, once per batch, not part of a decode: de-stuffing on the device (opts.device_destuff)
                             and the pass that lays the scans out lane-interleaved (k_scan_interleave) */
    MJX_K_HUFF_EMIT = 8,  /* single decode (pictures of one scan without restart intervals): the first decode, which emits -- instead of
                             MJX_K_HUFF_SYNC and the decode of MJX_K_HUFF_WRITE */
    MJX_K_HUFF_PREFIX = 9,/* ... the prefixes of the subsequences whose entry state was wrong, and block words -> DC differences + tile offsets */
    MJX_K_RESIZE = 10,    /* the pass behind stage B that brings a picture to the form it leaves in: resize on the device (k_resize_out),
                             orientation (k_orient_out, k_resize_orient), the same on planes (k_orient_planes, k_resize_planes), MJX_PIXELS_LIBJPEG's upsampling and colour step (k_upsample_color).  No launches
                             for a batch without a resized or oriented picture or that option */
    MJX_K_COUNT = 11
};
int mjx_batch_kernel_ms(mjx_batch *b, double ms[MJX_K_COUNT], uint64_t launches[MJX_K_COUNT], int reset);

/* SURVEY s8(b) convenience form: create + decode + wait; rgb_dev[i] receives device pointers owned by *out. */
int mjx_decode_scans(mjx_ctx *ctx, const mjx_scan_desc *descs, size_t n, const mjx_opts *opts,
                     uint8_t **rgb_dev, int *status, mjx_batch **out);

/* The outer surface for a batch of files: JPEGImage::parse of jpeg/mod.rs:202 for n files at once,
 * pipelined -- the list is cut into groups of compressed data (12 MB first, doubling up to 96 MB, 192 MB for long lists);
 * `threads` host threads (0 = half the processors the process may use -- affinity mask and cgroup quota counted --,
 * between 4 and 32) walk the markers and de-stuff group after group into pinned memory, every
 * group goes up in one DMA transfer on an upload stream of its own, and its kernels start behind that transfer's event,
 * so parsing, transfer and decode of successive groups overlap.  status[i] receives the parse / plan / decode status of
 * file i, rgb_dev[i] a device pointer owned by *out (NULL on failure); mjx_batch_image_info(*out, i, ...) gives the
 * dimensions.  *out is a directory of the groups' batches: every per-picture accessor, mjx_batch_decode / _wait / _bytes /
 * _geometry / _kernel_ms / _compare_rgb work on it, mjx_batch_tile does not.  Calls on one context are serialised (the
 * pinned arena belongs to the context).  Release with mjx_batch_free. */
int mjx_decode_batch(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                     unsigned threads, uint8_t **rgb_dev, int *status, mjx_batch **out);

/* mjx_decode_batch with an output description; dst[i] follows file i through the groups of the pipelined call, as rois[i] does.
 * out == NULL: mjx_decode_batch (without its rgb_dev array: mjx_batch_output_info says where picture i lies).  ctx == NULL -- what a
 * failed mjx_ctx_create leaves -- is MJX_ERR_DEVICE: there is no device to write the output, and no CPU path. */
int mjx_decode_batch_out(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                         unsigned threads, const mjx_output *out, int *status, mjx_batch **b);

/* mjx_decode_batch_out with a resize description; rs follows file i through the groups of the pipelined call, as rois[i] and
 * dst[i] do.  rs == NULL: mjx_decode_batch_out.  out == NULL with a resize: interleaved u8 R,G,B, library-owned. */
int mjx_decode_batch_resize(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                            unsigned threads, const mjx_output *out, const mjx_resize *rs, int *status, mjx_batch **b);

/* mjx_decode_batch_resize with an orientation description; the code goes with file i through the groups of the pipelined call, as
 * rois[i], dst[i] and rs do, and the worker that plans file i reads its tag.  orient == NULL: mjx_decode_batch_resize. */
int mjx_decode_batch_orient(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                            unsigned threads, const mjx_output *out, const mjx_resize *rs, const mjx_orient *orient, int *status,
                            mjx_batch **b);

/* mjx_decode_batch with a plane description (YCbCr output); dst[i] follows file i through the groups of the pipelined call, as in
 * mjx_decode_batch_out; mjx_batch_plane_info says where picture i's planes lie.  ctx == NULL is MJX_ERR_DEVICE, planes == NULL
 * MJX_ERR_INVALID_ARG. */
int mjx_decode_batch_planes(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                            unsigned threads, const mjx_planes *planes, int *status, mjx_batch **b);
/* mjx_decode_batch_planes with a resize and / or an orientation description: dst[i], rois[i], the file's tag (from_exif: the worker
 * that plans file i reads it) and extra[i] follow file i through the groups.  Both NULL: mjx_decode_batch_planes. */
int mjx_decode_batch_planes_orient(mjx_ctx *ctx, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                                   unsigned threads, const mjx_planes *planes, const mjx_resize *rs, const mjx_orient *orient, int *status,
                                   mjx_batch **b);

/* ---- multi-GPU front: one context + one host thread + one work queue per device, no collective ----------
 * Pictures are independent (decoder.rs:162-343 touches only `self`), so a list of files shards over the GPUs of a node
 * without any exchange: every slot decodes its share with the pipelined mjx_decode_batch on its own device, outputs stay
 * where they were produced.  Files are dealt to the slots by compressed bytes (largest file first, each to the slot with the
 * fewest bytes so far, the lowest slot on a tie: i mod N for a list of equal files, level queues for a skewed one) or round
 * robin (mjx_pool_set_deal).  `devices` may name a device more than once (two slots on one GPU).  One mjx_pool_decode_batch
 * call at a time per pool.  A slot whose device fails fails its own files (their status is the slot's error, the call
 * returns it); the other slots' results stay valid.
 * Host side: the slots share the host.  With threads_per_device == 0 every slot takes max(2, P / (2 N)) parse threads, P =
 * mjx_host_processors(), so that N slots together stay within the processors the process may use (mjx_decode_batch alone
 * takes P / 2); and a slot's host thread -- with it the parse threads it starts and the pinned arena it allocates -- is bound
 * to the processors of its GPU's NUMA node when the platform names one and the process may run there (MJX_POOL_NUMA=0: no). */
typedef struct mjx_pool mjx_pool;
typedef struct mjx_pool_result mjx_pool_result;
int mjx_pool_create(const int *devices, size_t n_devices, mjx_pool **out);
void mjx_pool_destroy(mjx_pool *pool);
size_t mjx_pool_devices(const mjx_pool *pool);
int mjx_pool_device(const mjx_pool *pool, size_t slot);          /* HIP device of a slot, -1 if out of range */
enum { MJX_POOL_DEAL_BY_BYTES = 0, MJX_POOL_DEAL_ROUND_ROBIN = 1 };
int mjx_pool_set_deal(mjx_pool *pool, int deal);
/* slot_of[i] / rgb_dev[i] / status[i] (each optional, n entries): the slot that decoded file i, its device pointer (owned
 * by *out, NULL on failure) and status.  Release with mjx_pool_result_free. */
int mjx_pool_decode_batch(mjx_pool *pool, const uint8_t *const *jpegs, const size_t *lens, size_t n, const mjx_opts *opts,
                          unsigned threads_per_device, int *slot_of, uint8_t **rgb_dev, int *status, mjx_pool_result **out);
/* file i of the call -> its slot, the slot's batch and the picture's index inside it (for mjx_batch_image_info,
 * mjx_batch_copy_rgb, ...) */
int mjx_pool_result_locate(const mjx_pool_result *r, size_t i, size_t *slot, mjx_batch **batch, size_t *index);
/* host side of the call, per slot: parse threads the slot's mjx_decode_batch ran with (0: the slot had no file) and the NUMA
 * node its host thread was bound to (-1: not bound) */
int mjx_pool_result_host(const mjx_pool_result *r, size_t slot, unsigned *threads, int *numa_node);
/* ... and the wall clock of the slot's own mjx_decode_batch (host parse + uploads + kernels, in milliseconds; 0: no file): which
 * queue the call waited for */
int mjx_pool_result_slot_ms(const mjx_pool_result *r, size_t slot, double *ms);
void mjx_pool_result_free(mjx_pool_result *r);

const char *mjx_strerror(int code);
/* library build info: "mjx <version> gfx950 subseq=<bits> ..." */
const char *mjx_version(void);

#ifdef __cplusplus
}
#endif
#endif

// mjx_cli.cpp -- counterpart of the reference's CLI (src/main.rs:24-40):  mjx_cli <in.jpeg> <out.ppm> [--p6] [--strict]
// [--scale N] [--crop X,Y,W,H] [--libjpeg-pixels]  (N = 2, 4, 8: the picture decoded at 1/N in the DCT domain, mjx_opts.scale_denom;
// --crop: only that rectangle of the -- scaled -- picture is decoded and written, mjx_opts.rois; --libjpeg-pixels: rounded samples,
// fancy chroma upsampling and libjpeg's integer colour tables, mjx_opts.pixels = MJX_PIXELS_LIBJPEG; --color-from-file: the file says
// what its components are, MJX_OPTS_COLOR = MJX_COLOR_FILE -- RGB, CMYK and YCCK files are written as R,G,B; --progressive: progressive
// files (SOF2) are accepted, MJX_OPTS_PROGRESSIVE = 1; --islow: --libjpeg-pixels with libjpeg's integer inverse DCT, MJX_OPTS_IDCT =
// MJX_IDCT_ISLOW -- byte for byte the picture libjpeg gives, with --scale 2, 4 or 8 libjpeg's own reduced decode, MJX_OPTS_EXACT_SCALE = 1)
// Writes the same ASCII P3 file ("P3\n{w} {h}\n255\n" then "r g b\n" per pixel, main.rs:35-39), buffered; --p6 writes
// binary PPM instead.  --luma: the luminance picture (MJX_OUTPUT_CHANNELS = 1) through the batch API, written as binary PGM (P5); chroma
// is never transformed.  --ycc: the component planes at their own sampling (mjx_planes), written back to back as one raw file -- Y,
// Cb, Cr: I420 order for a 4:2:0 file --; --nv12: Y, then Cb and Cr interleaved.  Both print the planes' sizes.  Exit code = MJX_* status.
#include "jpeg.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// --luma: mjx_decode keeps packed RGB, so the one file goes through mjx_decode_batch_out with a luminance description
static int write_luma(const std::vector<uint8_t> &bytes, const mjx_opts &opts, const char *path)
{
    mjx_ctx *ctx = nullptr;
    int rc = mjx_ctx_create(0, &ctx);
    if (rc != MJX_OK) { std::fprintf(stderr, "decode failed: %s (%d)\n", mjx_strerror(rc), rc); return rc; }
    mjx_output fmt{};
    fmt.dtype = MJX_DTYPE_U8;
    MJX_OUTPUT_CHANNELS(&fmt) = 1;
    const uint8_t *ptr = bytes.data();
    const size_t len = bytes.size();
    int status = MJX_OK;
    mjx_batch *b = nullptr;
    rc = mjx_decode_batch_out(ctx, &ptr, &len, 1, &opts, 1, &fmt, &status, &b);
    if (rc == MJX_OK) rc = status;
    uint32_t w = 0, h = 0;
    std::vector<uint8_t> pix;
    if (rc == MJX_OK) rc = mjx_batch_image_info(b, 0, &w, &h, nullptr, nullptr);
    if (rc == MJX_OK) {
        pix.resize(size_t(w) * h);
        rc = mjx_batch_copy_output(b, 0, pix.data(), pix.size());
    }
    if (b) mjx_batch_free(b);
    mjx_ctx_destroy(ctx);
    if (rc != MJX_OK) { std::fprintf(stderr, "decode failed: %s (%d)\n", mjx_strerror(rc), rc); return rc; }
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return MJX_ERR_INVALID_ARG; }
    std::fprintf(o, "P5\n%u %u\n255\n", w, h);
    std::fwrite(pix.data(), 1, pix.size(), o);
    std::fclose(o);
    return MJX_OK;
}

// --ycc / --nv12: the one file through mjx_decode_batch_planes, library-owned uint8 planes, copied out dense
static int write_planes(const std::vector<uint8_t> &bytes, const mjx_opts &opts, const char *path, bool nv12)
{
    mjx_ctx *ctx = nullptr;
    int rc = mjx_ctx_create(0, &ctx);
    if (rc != MJX_OK) { std::fprintf(stderr, "decode failed: %s (%d)\n", mjx_strerror(rc), rc); return rc; }
    mjx_planes fmt{};
    fmt.dtype = MJX_DTYPE_U8;
    fmt.interleave_chroma = nv12 ? 1 : 0;
    const uint8_t *ptr = bytes.data();
    const size_t len = bytes.size();
    int status = MJX_OK;
    mjx_batch *b = nullptr;
    rc = mjx_decode_batch_planes(ctx, &ptr, &len, 1, &opts, 1, &fmt, &status, &b);
    if (rc == MJX_OK) rc = status;
    uint32_t nplanes = 0;
    uint8_t il = 0;
    mjx_plane_layout lay{};
    std::vector<uint8_t> pix;
    if (rc == MJX_OK) rc = mjx_batch_plane_info(b, 0, &nplanes, &lay, nullptr, &il);
    if (rc == MJX_OK) {
        size_t total = 0;
        for (uint32_t c = 0; c < nplanes; c++) total += size_t(lay.width[c]) * lay.height[c] * (il && c == 1 ? 2u : 1u);
        pix.resize(total);
        rc = mjx_batch_copy_planes(b, 0, pix.data(), pix.size());
    }
    if (b) mjx_batch_free(b);
    mjx_ctx_destroy(ctx);
    if (rc != MJX_OK) { std::fprintf(stderr, "decode failed: %s (%d)\n", mjx_strerror(rc), rc); return rc; }
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return MJX_ERR_INVALID_ARG; }
    std::fwrite(pix.data(), 1, pix.size(), o);
    std::fclose(o);
    for (uint32_t c = 0; c < nplanes; c++)
        std::printf("plane %u: %ux%u%s\n", c, lay.width[c], lay.height[c], il && c == 1 ? " pairs Cb,Cr" : "");
    return MJX_OK;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <input.jpeg> <output.ppm> [--p6] [--strict] [--ref-compat] [--scale N] [--crop X,Y,W,H] [--libjpeg-pixels] [--islow] [--color-from-file] [--progressive] [--luma] [--ycc] [--nv12]\n", argv[0]);   // main.rs:26-28 expect()
        return MJX_ERR_INVALID_ARG;
    }
    bool p6 = false, luma = false, ycc = false, nv12 = false;
    mjx_opts opts{};
    mjx_rect crop{0, 0, 0, 0};
    for (int i = 3; i < argc; i++) {
        if (!std::strcmp(argv[i], "--p6")) p6 = true;
        else if (!std::strcmp(argv[i], "--luma")) luma = true;
        else if (!std::strcmp(argv[i], "--ycc")) ycc = true;
        else if (!std::strcmp(argv[i], "--nv12")) nv12 = true;
        else if (!std::strcmp(argv[i], "--strict")) opts.strict_ref = 1;
        else if (!std::strcmp(argv[i], "--ref-compat")) opts.layout = MJX_LAYOUT_REF_COMPAT;
        else if (!std::strcmp(argv[i], "--libjpeg-pixels")) opts.pixels = MJX_PIXELS_LIBJPEG;
        else if (!std::strcmp(argv[i], "--islow")) { opts.pixels = MJX_PIXELS_LIBJPEG; MJX_OPTS_IDCT(&opts) = MJX_IDCT_ISLOW; MJX_OPTS_EXACT_SCALE(&opts) = 1; }      // (implies --libjpeg-pixels)
        else if (!std::strcmp(argv[i], "--color-from-file")) MJX_OPTS_COLOR(&opts) = MJX_COLOR_FILE;
        else if (!std::strcmp(argv[i], "--progressive")) MJX_OPTS_PROGRESSIVE(&opts) = 1;
        else if (!std::strcmp(argv[i], "--scale")) {
            const long v = i + 1 < argc ? std::strtol(argv[++i], nullptr, 10) : -1;
            if (v < 0 || v > 255) { std::fprintf(stderr, "--scale takes 1, 2, 4 or 8\n"); return MJX_ERR_INVALID_ARG; }
            opts.scale_denom = uint8_t(v);           // (other values: mjx_decode says MJX_ERR_INVALID_ARG)
        } else if (!std::strcmp(argv[i], "--crop")) {
            unsigned x, y, w, h;
            char tail;
            if (i + 1 >= argc || std::sscanf(argv[++i], "%u,%u,%u,%u%c", &x, &y, &w, &h, &tail) != 4) { std::fprintf(stderr, "--crop takes X,Y,W,H\n"); return MJX_ERR_INVALID_ARG; }
            crop = mjx_rect{x, y, w, h};             // (a rectangle outside the picture: mjx_decode says MJX_ERR_INVALID_ARG)
            opts.rois = &crop;
            opts.n_rois = 1;
        }
    }
    std::FILE *f = std::fopen(argv[1], "rb");                                   // file_to_bytes, main.rs:16-22
    if (!f) { std::perror(argv[1]); return MJX_ERR_INVALID_ARG; }
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    if (luma) return write_luma(bytes, opts, argv[2]);
    if (ycc || nv12) return write_planes(bytes, opts, argv[2], nv12);
    jpeg::JPEGImage image;
    const jpeg::JPEGImage::Result r = jpeg::JPEGImage::parse(bytes, image, &opts);   // main.rs:31
    if (!r.ok()) { std::fprintf(stderr, "decode failed: %s (%d)\n", r.message.c_str(), r.code); return r.code; }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return MJX_ERR_INVALID_ARG; }
    std::fprintf(o, "%s\n%zu %zu\n255\n", p6 ? "P6" : "P3", image.width(), image.height());   // main.rs:35
    std::string out;
    for (const jpeg::Pixel &px : *image.image_data()) {                          // main.rs:36-39
        if (p6) { out.push_back(char(std::get<0>(px))); out.push_back(char(std::get<1>(px))); out.push_back(char(std::get<2>(px))); }
        else { char line[24]; out.append(line, size_t(std::snprintf(line, sizeof line, "%u %u %u\n", std::get<0>(px), std::get<1>(px), std::get<2>(px)))); }
        if (out.size() > (1u << 20)) { std::fwrite(out.data(), 1, out.size(), o); out.clear(); }
    }
    std::fwrite(out.data(), 1, out.size(), o);
    std::fclose(o);
    return MJX_OK;
}

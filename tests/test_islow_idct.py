"""libjpeg's integer slow inverse DCT in stage B (MJX_OPTS_IDCT = MJX_IDCT_ISLOW with MJX_PIXELS_LIBJPEG, include/mjx.h): exact pixels.

The reference is tests/islow_ref.py, a numpy restatement of the contract in int32 with wrap-around.
  CPU  the reference equals Pillow (libjpeg-turbo) byte for byte on every file set below, and differs from it without the narrow-plane
       rule; the lane routine the kernel and the host share (mjx_idct_islow_host) is the reference bit for bit, wrap-around and
       saturation included, and runs clean under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program; the option
       byte, its mirrors and its refusals.
  GPU  the decoded picture equals the reference AND Pillow byte for byte; every stream source and both entropy paths give the same
       bytes; constructed extreme blocks equal the reference; rectangles, formats, luminance, resize, orientation, mixed calls, tile,
       the pool and mjx_decode compose; a call without the byte launches what it launched before and gives the parent's bytes.
"""
import ctypes
import glob
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import islow_ref as isl
import jpegwriter as jw
import libjpeg_ref as lj
import scaled_ref
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_sampling_layouts as tsl
import wide_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_DIR = os.path.join(ROOT, "tests", "golden", "pil")
DATA_DIR = os.path.join(ROOT, "tests", "data")
PIL_NAMES = [n for n in tsl.NAMES if n != "Y22_Cb22_Cr22"]             # (Pillow refuses the 12-block MCU)
LAYOUT_SIZES = [(61, 45), (40, 24), (5, 3), (3, 17)]
WIDE_SIZES = [(61, 45), (9, 70)]
Y420, Y422, Y440, LUMA_SUB = "Y22_Cb11_Cr11", "Y21_Cb11_Cr11", "Y12_Cb11_Cr11", "Y11_Cb22_Cr21"
EXACT = dict(pixels="libjpeg", idct="islow")


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def q85(n, w, h):
    return tsl.data_of(n, w, h, quality=85)


def baseline_files():
    """all of tests/data/*.jp*g and the baseline files of tests/golden/pil/*.jpg"""
    out = []
    for p in sorted(glob.glob(os.path.join(DATA_DIR, "*.jp*g")) + glob.glob(os.path.join(PIL_DIR, "*.jpg"))):
        try:
            scaled_ref.jpeg_tables(_read(p))
        except ValueError:                       # (no baseline frame: progressive.jpg)
            continue
        out.append(p)
    return out


def differing(a, b):
    return "shape %s / %s" % (a.shape, b.shape) if a.shape != b.shape else int((a != b).sum())


# ---- CPU: the reference is Pillow's, exactly ----------------------------------------------------------------------------------------
def test_the_reference_is_pillow_exactly_on_files(orc):
    files = baseline_files()
    assert len(files) == 34, len(files)
    bad = []
    for p in files:
        data = _read(p)
        got, want = isl.pixels(data), pillow(data)
        if not np.array_equal(got, want):
            bad.append((os.path.basename(p), differing(got, want)))
    assert bad == [], bad


@pytest.mark.parametrize("size", LAYOUT_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_reference_is_pillow_exactly_on_every_layout(orc, size):
    w, h = size
    bad = []
    for n in PIL_NAMES:
        data = q85(n, w, h)
        got, want = isl.pixels(data, tsl.oracle_std(data)), pillow(data)
        if not np.array_equal(got, want):
            bad.append((n, differing(got, want)))
    assert len(PIL_NAMES) == 63 and bad == [], bad[:8]


@pytest.mark.parametrize("size", WIDE_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_reference_is_pillow_exactly_with_factors_of_4(size):
    w, h = size
    bad = []
    for n in wide_ref.PILLOW_NAMES:
        data, blocks = wide_ref.layout_file(n, w, h)
        got, want = isl.pixels(data, wide_ref.dec_of(n, w, h, blocks)), pillow(data)
        if not np.array_equal(got, want):
            bad.append((n, differing(got, want)))
    assert len(wide_ref.PILLOW_NAMES) == 132 and bad == [], bad[:8]


def pillow_written(w, h, subsampling, quality, noise):
    """a w x h file written by Pillow: a crop of lena.jpeg, or noise"""
    from PIL import Image
    if noise:
        src = np.random.default_rng(w * 100 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        src = pillow(_read(os.path.join(DATA_DIR, "lena.jpeg")))[40:40 + h, 60:60 + w]
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(src)).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


TINY = [(w, h, s, q, n) for w in (1, 2, 3, 4) for h in (1, 2, 3, 5, 9, 17) for s in (1, 2) for q in (50, 95, 100) for n in (False, True)]


def test_the_reference_is_pillow_exactly_on_tiny_pillow_written_files(orc):
    """Widths 1 .. 4 (planes of one and two columns: the narrow-plane rule), 4:2:2 and 4:2:0."""
    bad = []
    for case in TINY:
        data = pillow_written(*case)
        got, want = isl.pixels(data), pillow(data)
        if not np.array_equal(got, want):
            bad.append((case, differing(got, want)))
    assert len(TINY) == 288 and bad == [], bad[:8]


def test_without_the_narrow_plane_rule_the_reference_is_not_pillows(orc):
    """The planted error: a 3-wide 4:2:0 file has chroma planes of two columns, which libjpeg replicates and the filter does not."""
    caught = 0
    for h in (5, 9, 17):
        data = pillow_written(3, h, 2, 95, True)
        want = pillow(data)
        assert np.array_equal(isl.pixels(data), want)
        caught += not np.array_equal(isl.pixels(data, narrow=False), want)
    assert caught == 3, caught


# ---- CPU: the lane routine is the reference, bit for bit ------------------------------------------------------------------------------
def extreme_blocks():
    """[(coef [64] int16, q [64] uint16)] in natural order: every single coefficient at +-1, +-1023 and +-32767 with tables of 1, 255 and
    65535; dense random blocks in range, at the limits of 16 bits and anywhere in them; all-zero AC rows and columns"""
    out = []
    for pos in range(64):
        for v in (1, -1, 1023, -1023, 32767, -32767):
            for t in (1, 255, 65535):
                c = np.zeros(64, np.int16)
                c[pos] = v
                out.append((c, np.full(64, t, np.uint16)))
    rng = np.random.default_rng(11)
    for k in range(300):
        if k < 100:                                          # what a picture holds
            c, q = rng.integers(-64, 64, 64), rng.integers(1, 32, 64)
        elif k < 200:                                        # the limits: the products wrap in the passes, the samples saturate
            c, q = rng.choice([32767, -32768], 64), rng.choice([255, 65535], 64)
        else:
            c, q = rng.integers(-32768, 32768, 64), rng.integers(1, 65536, 64)
        out.append((c.astype(np.int16), q.astype(np.uint16)))
    for kind in range(3):
        c = np.zeros((8, 8), np.int16)
        if kind == 0:
            c[0, :] = 100 - 30 * np.arange(8)                # only row 0: every column's AC terms are zero
        elif kind == 1:
            c[:, 0] = 100 - 30 * np.arange(8)                # only column 0
        else:
            c[0, 0], c[7, 7] = 64, -500
        out.append((c.reshape(64), np.full(64, 16, np.uint16)))
    return out


def test_the_lane_routine_is_the_reference_bit_for_bit(mjx):
    blocks = extreme_blocks()
    want = [isl.idct_blocks(c.reshape(1, 8, 8), q.reshape(8, 8).astype(np.int64))[0] for c, q in blocks]
    bad = [k for k, ((c, q), w) in enumerate(zip(blocks, want)) if not np.array_equal(mjx.idct_islow_host(c, q), w)]
    assert bad == [], (len(bad), bad[:8])
    # the cases do exercise saturation at both ends and wrap-around: int64 arithmetic gives other samples on some of them
    flat = np.concatenate([w.reshape(-1) for w in want])
    assert (flat == 0).any() and (flat == 255).any()
    c, q = blocks[64 * 18 + 150]
    d = c.astype(np.int64) * q.astype(np.int64)
    assert np.abs(d).max() * 8192 * 4 > 2 ** 31                                # (pass 1 alone leaves 32 bits)
    # a flat block: DC d gives ((d + 4) >> 3) + 128 everywhere
    for dc, t in ((100, 16), (-100, 16), (1, 1), (-1, 1), (-3, 1), (4, 1)):
        c = np.zeros(64, np.int16)
        c[0] = dc
        s = min(max(((dc * t + 4) >> 3) + 128, 0), 255)
        assert np.array_equal(mjx.idct_islow_host(c, np.full(64, t, np.uint16)), np.full((8, 8), s, np.uint8)), (dc, t)


def test_the_lane_routine_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program (tests/islow_host.cpp, its own main) under -fsanitize=address,undefined: idct_islow_inplace on heap blocks of
    exactly 64 words, the extreme blocks above among them."""
    exe = tmp_path / "islow_host"
    csrc = os.path.join(ROOT, "jpeg-rust_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", str(exe), os.path.join(ROOT, "tests", "islow_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = r.stdout.split()
    assert out[0] == "blocks" and int(out[1]) == 64 * 18 + 300 + 3, r.stdout


def test_the_shared_upsampling_takes_the_replicate_flag(mjx):
    """mjx_upsample_color_host / _luma_host with MJX_UPSAMPLE_REPLICATE on a component: islow_ref's narrow-plane rule, bit for bit"""
    rng = np.random.default_rng(3)
    rep = mjx.UPSAMPLE_REPLICATE
    for hv, W, H in (([(2, 2), (1, 1), (1, 1)], 3, 17), ([(2, 1), (1, 1), (1, 1)], 4, 9), ([(2, 2), (1, 1), (1, 1)], 1, 1), ([(1, 1), (2, 2), (2, 1)], 2, 5)):
        hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
        ratios = [(hmax // h, vmax // v) for h, v in hv]
        planes = [rng.integers(0, 256, (-(-H * v // vmax), -(-W * h // hmax)), dtype=np.uint8) for h, v in hv]
        flags = [rep if p.shape[1] <= 2 and r == 2 else 0 for p, (r, _) in zip(planes, ratios)]
        assert any(flags)
        want = isl.pixels_from_planes(planes, ratios, W, H)
        got = mjx.upsample_color_host(planes, [r | f for (r, _), f in zip(ratios, flags)], [v for _, v in ratios], (0, 0, W, H))
        assert np.array_equal(got, want), (hv, W, H)
        if flags[0]:
            got = mjx.upsample_luma_host(planes[0], ratios[0][0] | rep, ratios[0][1], (0, 0, W, H))
            assert np.array_equal(got, isl.upsample(planes[0], *ratios[0])[:H, :W]), (hv, W, H)
    # without the flag the existing rule stands
    p = rng.integers(0, 256, (4, 2), dtype=np.uint8)
    assert np.array_equal(mjx.upsample_luma_host(p, 2, 2, (0, 0, 4, 8)), lj.upsample(p, 2, 2))


# ---- CPU: the option byte ---------------------------------------------------------------------------------------------------------------
def test_the_option_byte_its_mirrors_and_its_refusals(mjx):
    hdr = _read(os.path.join(ROOT, "include", "mjx.h")).decode()
    assert re.search(r"#define MJX_OPTS_IDCT_OFFSET 12\b", hdr) and re.search(r"MJX_IDCT_FLOAT = 0", hdr) and re.search(r"MJX_IDCT_ISLOW = 1", hdr)
    assert re.search(r"#define MJX_ABI_VERSION 2\b", hdr) and b"abi=2 " in mjx.lib().mjx_version() and b"islow" in mjx.lib().mjx_version()
    assert mjx.Opts.IDCT_OFFSET == 12 and (mjx.IDCT_FLOAT, mjx.IDCT_ISLOW) == (0, 1)
    assert ctypes.sizeof(mjx.Opts) == 32 and mjx.Opts.rois.offset == 16 and mjx.Opts.scale_denom.offset == 9
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    assert "pub const MJX_OPTS_IDCT_OFFSET: usize = 12;" in rs and "pub const MJX_IDCT_ISLOW: u8 = 1;" in rs and "pub fn mjx_idct_islow_host(" in rs
    assert "--islow" in _read(os.path.join(ROOT, "jpeg-rust_amd", "csrc", "mjx_cli.cpp")).decode()
    raw = lambda o: bytes((ctypes.c_uint8 * 32).from_address(ctypes.addressof(o)))
    o = mjx._opts()
    assert o.idct == 0 and raw(o)[8] == 0 and raw(o)[10:16] == bytes(6)          # (the default call is untouched: pixels and the option bytes)
    o = mjx._opts(pixels="libjpeg")
    assert (o.pixels, o.idct) == (1, 0) and raw(o)[12] == 0
    o = mjx._opts(pixels="libjpeg", idct="islow")
    assert (o.pixels, o.idct) == (1, 1) and raw(o)[12] == 1 and raw(o)[8] == 1
    o = mjx._opts(pixels="libjpeg-exact")
    assert (o.pixels, o.idct) == (1, 1)                                          # (the shorthand sets both bytes)
    assert mjx._opts(pixels="libjpeg-exact", idct="float").idct == 0 and mjx._opts(pixels="libjpeg", idct="float").idct == 0
    with pytest.raises(mjx.MjxError):
        mjx._opts(idct="ifast")
    data = tsl.data_of(Y420, 61, 45)
    scan = mjx.ParsedScan(data)
    try:
        assert scan.validate(pixels="libjpeg", idct="islow") == mjx.OK
        assert scan.validate(pixels="libjpeg-exact", roi=(3, 5, 20, 10)) == mjx.OK
        assert scan.validate(idct="islow") == mjx.ERR_INVALID_ARG                # (without pixels = libjpeg)
        assert scan.validate(pixels="reference", idct=mjx.IDCT_ISLOW) == mjx.ERR_INVALID_ARG
        assert scan.validate(pixels="libjpeg", idct=2) == mjx.ERR_INVALID_ARG
        assert scan.validate(idct=2) == mjx.ERR_INVALID_ARG
        for s in (2, 4, 8):
            assert scan.validate(scale=s, **EXACT) == mjx.ERR_INVALID_ARG, s
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT, **EXACT) == mjx.ERR_INVALID_ARG
        assert scan.validate(strict_ref=True, **EXACT) == mjx.ERR_INVALID_ARG
        assert scan.validate(pixels=2) == mjx.ERR_INVALID_ARG and scan.validate() == mjx.OK and scan.validate(pixels="libjpeg") == mjx.OK
        # a plane description with the option: not built
        with pytest.raises(mjx.MjxError) as e:
            scan.planes_layout(mjx.Planes("uint8"), **EXACT)
        assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT
        assert scan.planes_layout(mjx.Planes("uint8"), pixels="libjpeg") is not None
        # the tiles are those of pixels = libjpeg, and auto_scale picks scale 1
        for roi in (None, (20, 10, 9, 7), (0, 16, 61, 16)):
            assert scan.plan_tiles(roi=roi, **EXACT) == scan.plan_tiles(roi=roi, pixels="libjpeg"), roi
        plan = scan.resize_plan(mjx.Resize(8, 6, auto_scale=True), **EXACT)
        assert plan["scale"] == 1 and plan["rect"] == (0, 0, 61, 45), plan
    finally:
        scan.close()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
def exact_decode(mjx, ctx, datas, **kw):
    """-> [picture or ('status', code)] of an exact-pixels Batch of parsed scans"""
    kw = dict(EXACT, **kw)
    scans = [mjx.ParsedScan(d, progressive=kw.get("progressive", False)) for d in datas]
    b = mjx.Batch(ctx, scans, **kw)
    try:
        b.decode()
        b.wait()
        return [b.rgb(i) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


def problems(cases, got, want_ref, want_pil):
    bad = []
    for c, g, r, p in zip(cases, got, want_ref, want_pil):
        if not isinstance(g, np.ndarray):
            bad.append((c, g))
        elif r is not None and not tsl.same(g, r):
            bad.append((c, "reference", differing(g, r)))
        elif p is not None and not tsl.same(g, p):
            bad.append((c, "Pillow", differing(g, p)))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(61, 45), (40, 24)], ids=lambda s: "%dx%d" % s)
def test_every_layout_equals_the_reference_and_pillow(mjx, gpu_ctx, size):
    w, h = size
    datas = [q85(n, w, h) for n in tsl.NAMES]
    got = exact_decode(mjx, gpu_ctx, datas)
    ref = [isl.pixels(d, tsl.oracle_std(d)) for d in datas]
    pil = [pillow(d) if n != "Y22_Cb22_Cr22" else None for n, d in zip(tsl.NAMES, datas)]
    bad = problems(tsl.NAMES, got, ref, pil)
    alone = exact_decode(mjx, gpu_ctx, datas[:1])                      # (a batch of one: the latency plan's cut of the scan)
    if not tsl.same(alone[0], got[0]):
        bad.append((tsl.NAMES[0], "alone"))
    assert bad == [], bad[:6]


NARROW = [(n, w, h) for n in (Y420, Y422, Y440) for w, h in ((3, 17), (2, 2), (1, 1))]


@pytest.mark.gpu
def test_narrow_planes_are_replicated_as_libjpeg_does(mjx, gpu_ctx):
    datas = [q85(n, w, h) for n, w, h in NARROW] + [pillow_written(3, 9, 2, 95, True), pillow_written(4, 5, 1, 95, True)]
    cases = NARROW + ["pillow 3x9 4:2:0", "pillow 4x5 4:2:2"]
    got = exact_decode(mjx, gpu_ctx, datas)
    bad = problems(cases, got, [isl.pixels(d) for d in datas], [pillow(d) for d in datas])
    # the luminance picture and an output format of such a picture leave through the same pass
    fmt = mjx.Output("uint8", bgr=True)
    for out, want in ((mjx.Output("uint8", channels=1), lambda d: isl.luma(d)), (fmt, lambda d: tof.expected(isl.pixels(d), fmt))):
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, output=out, **EXACT)
        try:
            b.decode()
            b.wait()
            for i, d in enumerate(datas):
                if b.status(i) != mjx.OK or not np.array_equal(np.squeeze(b.output(i)), np.squeeze(want(d))):
                    bad.append((cases[i], "output", b.status(i)))
        finally:
            tsl.close_all(b, scans)
    # without the option the filter stands at every width: pixels = libjpeg alone is not Pillow's picture there
    plain = exact_decode(mjx, gpu_ctx, datas[-2:-1], idct="float")[0]
    assert not tsl.same(plain, pillow(datas[-2]))
    assert bad == [], bad[:6]


@pytest.mark.gpu
def test_factors_of_4_and_files_equal_the_reference_and_pillow(mjx, gpu_ctx):
    wide = [wide_ref.layout_file(n, 61, 45) for n in wide_ref.NAMED]
    files = [os.path.join(DATA_DIR, "lena.jpeg"), os.path.join(DATA_DIR, "2x2-chroma.jpeg"), os.path.join(DATA_DIR, "lena-bw.jpeg"),
             os.path.join(PIL_DIR, "std_420_big.jpg")]
    big = q85(Y420, 1035, 490)                                           # (63 tiles that wrap MCU rows, an odd width)
    datas = [d for d, _ in wide] + [_read(p) for p in files] + [big]
    cases = wide_ref.NAMED + [os.path.basename(p) for p in files] + ["420 1035x490"]
    ref = [isl.pixels(d, wide_ref.dec_of(n, 61, 45, blocks)) for n, (d, blocks) in zip(wide_ref.NAMED, wide)]
    ref += [isl.pixels(_read(p)) for p in files] + [isl.pixels(big, tsl.oracle_std(big))]
    pil = [pillow(d) if sum(a * b for a, b in wide_ref.parse_name(n)) <= 10 else None for n, (d, _) in zip(wide_ref.NAMED, wide)]
    pil += [pillow(d) for d in datas[len(wide):]]
    got = exact_decode(mjx, gpu_ctx, datas)
    assert problems(cases, got, ref, pil) == []


def stream_files():
    """[(name, bytes, progressive)]: a multi-scan file, the 4:2:0 layout and its restart twin, a progressive file"""
    return [("ms_420_odd.jpg", _read(os.path.join(PIL_DIR, "ms_420_odd.jpg")), False), ("420 333x217", q85(Y420, 333, 217), False),
            ("420 333x217 dri3", tsl.data_of(Y420, 333, 217, quality=85, restart=3), False),
            ("progressive.jpg", _read(os.path.join(PIL_DIR, "progressive.jpg")), True)]


def child_streams(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = stream_files()
    out, status = {}, {}
    for dd in (False, True):
        b, st = mjx.decode_batch(ctx, [d for _, d, _ in files], device_destuff=dd, progressive=True, **EXACT)
        for i in range(len(files)):
            status["%d_%d" % (i, dd)] = st[i] or b.status(i)
            if not status["%d_%d" % (i, dd)]:
                out["%d_%d" % (i, dd)] = b.rgb(i)
        b.close()
        # alone: a multi-scan picture that fits is read straight from its scans' streams, unless MJX_PLANAR_DIRECT=0 gathers it
        b, st = mjx.decode_batch(ctx, [files[0][1]], device_destuff=dd, **EXACT)
        status["alone_%d" % dd] = st[0] or b.status(0)
        if not status["alone_%d" % dd]:
            out["alone_%d" % dd] = b.rgb(0)
        b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=status)))


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_islow_idct as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_stream_source_and_entropy_path_gives_the_same_bytes(mjx, gpu_ctx, tmp_path):
    files = stream_files()
    want = [pillow(d) for _, d, _ in files]                            # (Pillow reads all four; the reference needs baseline coefficients)
    assert np.array_equal(want[1], want[2]) and np.array_equal(want[1], isl.pixels(files[1][1], tsl.oracle_std(files[1][1])))
    assert np.array_equal(want[0], isl.pixels(files[0][1]))
    got = exact_decode(mjx, gpu_ctx, [d for _, d, _ in files], progressive=True)
    bad = problems([n for n, _, _ in files], got, [None] * len(files), want)
    for k, env in enumerate(({}, {"MJX_SINGLE_DECODE": "0"}, {"MJX_STREAM_LINEAR": "1"}, {"MJX_PLANAR_DIRECT": "0"})):
        npz = tmp_path / ("streams%d.npz" % k)
        res = run_child(tmp_path, "child_streams(%r)" % str(npz), env)
        with np.load(str(npz)) as z:
            for dd in (0, 1):
                for i, (n, _, _) in enumerate(files):
                    key = "%d_%d" % (i, dd)
                    if res["status"][key] != 0 or not tsl.same(z[key], want[i]):
                        bad.append((n, sorted(env.items()), "device de-stuffing" if dd else "host de-stuffing", res["status"][key]))
                key = "alone_%d" % dd
                if res["status"][key] != 0 or not tsl.same(z[key], want[0]):
                    bad.append(("ms_420_odd.jpg alone", sorted(env.items()), dd, res["status"][key]))
    assert bad == [], bad[:8]


def constructed(hv, mcux, mcuy, qt16, seed):
    """-> (file, reference picture): blocks of extreme coefficients through jpegwriter.jpeg_from_blocks, 8- or 16-bit tables"""
    rng = np.random.default_rng(seed)
    per = sum(h * v for h, v in hv) if len(hv) == 3 else 1
    n = mcux * mcuy * per
    blocks = np.zeros((n, 64), np.int64)
    ext = extreme_blocks()
    for b in range(n):
        kind = b % 4
        if kind == 0:                                                  # one extreme coefficient (DC differences stay within the codes' 11 bits)
            c = ext[int(rng.integers(0, 64 * 18))][0].astype(np.int64)
            c[0] = np.clip(c[0], -1000, 1000)
            blocks[b] = c[scaled_ref.ZIGZAG]
        elif kind == 1:                                                # dense, far out of range: wrap-around and saturation
            blocks[b] = rng.choice([32767, -32767, 1023, -1023], 64)
            blocks[b, 0] = rng.integers(-1000, 1000)
        elif kind == 2:                                                # what a picture holds
            blocks[b] = rng.integers(-40, 40, 64) * (rng.random(64) < 0.3)
            blocks[b, 0] = rng.integers(-500, 500)
        else:                                                          # one row of AC terms only
            blocks[b, [0, 1, 5, 6, 14, 15, 27, 28]] = rng.integers(-300, 300, 8)
    top = 65535 if qt16 else 255
    qts = [np.concatenate([[1, 2, top], rng.integers(1, top + 1, 61)]) for _ in hv]
    tables = {(0, 0): jw.small_dc_table(11), (1, 0): jw.full_ac_table()}     # (every run / size symbol: sizes up to 15 bits)
    data = jw.jpeg_from_blocks(blocks, hv, mcux, mcuy, qts, tables, qt16=qt16)
    # per-component blocks in decode order for the reference
    mcu = blocks.reshape(mcux * mcuy, per, 64)
    counts, at, coefs = ([h * v for h, v in hv] if len(hv) == 3 else [1]), 0, []
    for k in counts:
        coefs.append(mcu[:, at:at + k].reshape(-1, 64).astype(np.int16))
        at += k
    import types
    dec = types.SimpleNamespace(coefs=coefs)
    return data, isl.pixels(data, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("qt16", [False, True], ids=["dqt8", "dqt16"])
def test_constructed_extreme_blocks_equal_the_reference(mjx, gpu_ctx, qt16):
    """Wrap-around and saturation on the device.  Pillow is not asked: its SIMD code works in 16 bits on such blocks."""
    grey, grey_ref = constructed([(1, 1)], 8, 8, qt16, 1)
    col, col_ref = constructed([(2, 2), (1, 1), (1, 1)], 5, 3, qt16, 2)
    got = exact_decode(mjx, gpu_ctx, [grey, col])
    assert grey_ref.shape == (64, 64, 3) and problems(["grey 64x64", "4:2:0"], got, [grey_ref, col_ref], [None, None]) == []


def rectangles(W, H, mw, mh):
    r = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H),
         (mw + 1, mh + 1, mw - 2, mh - 2), (mw, mh, mw, mh), (3, 5, W - 7, H - 11), (mw - 1, mh - 1, 2, 2), (7, 2 * mh, 9, 1), (W // 2, H // 2, 41, 37)]
    return [q for q in r if q[0] + q[2] <= W and q[1] + q[3] <= H and q[2] > 0 and q[3] > 0]


@pytest.mark.gpu
def test_rectangles_formats_and_luminance_compose(mjx, gpu_ctx):
    bad = []
    # a rectangle is the crop of the whole picture
    for lname, W, H in ((Y420, 333, 217), (LUMA_SUB, 61, 45)):
        data = q85(lname, W, H)
        full = isl.pixels(data, tsl.oracle_std(data))
        hv = tsl.parse_name(lname)
        rects = rectangles(W, H, 8 * max(h for h, _ in hv), 8 * max(v for _, v in hv))
        got = exact_decode(mjx, gpu_ctx, [data] * len(rects), rois=rects)
        bad += [(lname, r) for r, g in zip(rects, got) if not tsl.same(g, full[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])]
    # two output formats: the formats' table applied to the exact picture
    cases = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 61, 45)]
    datas = [q85(*c) for c in cases]
    rois = [None, (3, 5, 40, 30), None, (11, 7, 48, 36)]
    exact = [isl.pixels(d, tsl.oracle_std(d)) for d in datas]
    crop = [e if r is None else np.ascontiguousarray(e[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for e, r in zip(exact, rois)]
    for fmt in (mjx.Output("float16", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD), mjx.Output("uint8", bgr=True)):
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, **EXACT)
        try:
            b.decode()
            b.wait()
            bad += [("format", fmt.dtype, cases[i], b.status(i)) for i in range(len(datas))
                    if b.status(i) != mjx.OK or not tof.same_bits(b.output(i), tof.expected(crop[i], fmt))]
        finally:
            tsl.close_all(b, scans)
    # luminance: component 0's exact plane, upsampled where Y is not the most finely sampled component
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(gpu_ctx, scans, rois=rois, output=mjx.Output("uint8", channels=1), **EXACT)
    try:
        b.decode()
        b.wait()
        for i, d in enumerate(datas):
            L, r = isl.luma(d, tsl.oracle_std(d)), rois[i]
            L = L if r is None else L[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]
            if b.status(i) != mjx.OK or not np.array_equal(np.squeeze(b.output(i)), L):
                bad.append(("luma", cases[i], b.status(i)))
    finally:
        tsl.close_all(b, scans)
    assert bad == [], bad[:8]


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    cases = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 333, 217)]
    datas = [q85(*c) for c in cases]
    rois = [(11, 7, 48, 36), (3, 5, 48, 36), (0, 9, 48, 36), (101, 50, 48, 36)]
    packed = [np.ascontiguousarray(isl.pixels(d, tsl.oracle_std(d))[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for d, r in zip(datas, rois)]
    dev, n = torch.device("cuda", 0), len(datas)
    big = torch.full((n, 3, 36, 56), float("nan"), dtype=torch.float16, device=dev)
    st = mjx.decode_into(ctx, datas, big[:, :, :, 4:52], rois=rois, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD, **EXACT)
    torch.cuda.synchronize()
    fmt = mjx.Output("float16", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD)
    got = big.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, :, 4:52]), tof.expected(packed[i], fmt)):
            bad.append(("f16 planar", i, st[i]))
    if not (np.isnan(got[:, :, :, :4]).all() and np.isnan(got[:, :, :, 52:]).all()):
        bad.append("the padding of the f16 rows was written")
    big8 = torch.full((n, 36, 54, 3), 7, dtype=torch.uint8, device=dev)
    st = mjx.decode_into(ctx, datas, big8[:, :, 3:51, :], rois=rois, bgr=True, pixels="libjpeg-exact")
    torch.cuda.synchronize()
    fmt = mjx.Output("uint8", bgr=True)
    got = big8.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, 3:51, :]), tof.expected(packed[i], fmt)):
            bad.append(("u8 interleaved", i, st[i]))
    if not (np.all(got[:, :, :3, :] == 7) and np.all(got[:, :, 51:, :] == 7)):
        bad.append("the padding of the u8 rows was written")
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad)}))


@pytest.mark.gpu
def test_decode_into_a_torch_tensor_with_padded_pitches(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0, res


def run_out(mjx, ctx, datas, fmt, roi, **kw):
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, rois=roi, output=fmt, **dict(EXACT, **kw))
    try:
        b.decode()
        b.wait()
        assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas)
        return [b.output(i) for i in range(len(datas))], [b.scale(i) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


@pytest.mark.gpu
def test_resize_and_orientation_work_on_the_exact_intermediate(mjx, gpu_ctx):
    """The parent's rules (test_resize's reference and tolerance, test_orientation's map) applied to the exact intermediate."""
    datas = [q85(Y420, 333, 217), q85(Y422, 333, 217)]
    roi = (10, 20, 300, 190)
    S = [isl.pixels(d, tsl.oracle_std(d)) for d in datas]
    packed = [np.ascontiguousarray(s[20:210, 10:310]) for s in S]
    bad = []
    fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
    for aa in (True, False):
        got, scales = run_out(mjx, gpu_ctx, datas, fmt, roi, resize=mjx.Resize(70, 37, antialias=aa, auto_scale=True))
        assert scales == [1, 1], scales
        for i, g in enumerate(got):
            tx, ty = trs.max_taps(300, 70, aa), trs.max_taps(190, 37, aa)
            p, _, _ = trs.check_against(g, trs.resize_ref(packed[i], 70, 37, aa), fmt, trs.tolerance(tx, ty))
            if p:
                bad.append(("resize", aa, i, p))
    fmt8, r = mjx.Output("uint8"), (5, 9, 120, 100)
    for code in (2, 6, 7):
        got, _ = run_out(mjx, gpu_ctx, datas, fmt8, r, orient=mjx.Orient(exif=False, extra=code))
        for i, g in enumerate(got):
            D = tor.orient_np(code, S[i])
            if not tof.same_bits(g, tof.expected(np.ascontiguousarray(D[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), fmt8)):
                bad.append(("orient", code, i))
    code, aa = 6, True
    D = [np.ascontiguousarray(tor.orient_np(code, s)[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for s in S]
    got, _ = run_out(mjx, gpu_ctx, datas, fmt, r, orient=mjx.Orient(exif=False, extra=code), resize=mjx.Resize(33, 40, antialias=aa, auto_scale=True))
    for i, g in enumerate(got):
        tx, ty = trs.max_taps(120, 33, aa), trs.max_taps(100, 40, aa)
        p, _, _ = trs.check_against(g, trs.resize_ref(D[i], 33, 40, aa), fmt, trs.tolerance(tx, ty))
        if p:
            bad.append(("resize + orient", i, p))
    assert bad == [], bad[:8]


@pytest.mark.gpu
def test_mixed_calls_tiles_the_pool_and_mjx_decode(mjx, gpu_ctx):
    ms = _read(os.path.join(PIL_DIR, "ms_420_odd.jpg"))
    good = [q85(Y420, 333, 217), q85(Y422, 61, 45), q85(LUMA_SUB, 61, 45), q85("gray22", 61, 45), q85(Y420, 3, 17), ms,
            tsl.data_of(Y420, 333, 217, quality=85, restart=3)]
    want = [isl.pixels(d, tsl.oracle_std(d)) for d in good[:5]] + [isl.pixels(ms), isl.pixels(good[0], tsl.oracle_std(good[0]))]
    # one call: several layouts, a grey file, a narrow picture, one picture per stream source, a refused file and a refused rectangle
    datas = good + [_read(os.path.join(PIL_DIR, "progressive.jpg"))]
    b, st = mjx.decode_batch(gpu_ctx, datas + [good[1]], rois=[None] * len(datas) + [(60, 0, 2, 2)], **EXACT)
    try:
        assert st == [mjx.OK] * len(good) + [mjx.ERR_UNSUPPORTED_FORMAT, mjx.ERR_INVALID_ARG], st
        for i in range(len(good)):
            assert tsl.same(b.rgb(i), want[i]), i
    finally:
        b.close()
    b, st = mjx.decode_batch(gpu_ctx, good[:2], layout=mjx.LAYOUT_REF_COMPAT, **EXACT)
    b.close()
    assert st == [mjx.ERR_INVALID_ARG] * 2, st
    b, st = mjx.decode_batch(gpu_ctx, good[:2], idct="islow")                    # (without pixels = libjpeg)
    b.close()
    assert st == [mjx.ERR_INVALID_ARG] * 2, st
    # mjx_decode and the reference's front door
    assert tsl.same(mjx.decode(good[0], pixels="libjpeg-exact"), want[0])
    assert tsl.same(mjx.decode(good[4], **EXACT), want[4])
    assert tsl.same(mjx.JPEGImage.parse(good[1], ctx=gpu_ctx, **EXACT).image_data(), want[1])
    with pytest.raises(mjx.MjxError):
        mjx.decode(good[0], scale=2, **EXACT)
    # tile(3) keeps the option, the narrow picture's pass included
    scans = [mjx.ParsedScan(d) for d in good]
    src = mjx.Batch(gpu_ctx, scans, **EXACT)
    try:
        t = src.tile(3)
        try:
            t.decode()
            t.wait()
            n = len(good)
            assert [t.status(i) for i in range(3 * n)] == [mjx.OK] * (3 * n)
            for i in range(3 * n):
                assert tsl.same(t.rgb(i), want[i % n]), i
        finally:
            t.close()
    finally:
        tsl.close_all(src, scans)
    # a two-slot pool
    pool = mjx.Pool([0, 0])
    try:
        res = pool.decode_batch(datas, **EXACT)
        try:
            assert res.status == [mjx.OK] * len(good) + [mjx.ERR_UNSUPPORTED_FORMAT], res.status
            assert sorted(set(res.slot_of[:len(good)])) == [0, 1]
            for i in range(len(good)):
                assert tsl.same(res.rgb(i), want[i]), i
        finally:
            res.close()
    finally:
        pool.close()


@pytest.mark.gpu
def test_a_call_without_the_byte_is_untouched(mjx, gpu_ctx):
    """pixels = None and pixels = "libjpeg" give the bytes they gave -- idct = "float" said aloud changes nothing, and the float
    libjpeg picture lies within the 3 levels of the exact one that DESIGN.md s19 measured --, and launch the kernels they launched."""
    datas = [_read(os.path.join(DATA_DIR, "lena.jpeg")), q85(Y420, 333, 217), q85(LUMA_SUB, 61, 45), q85(Y420, 3, 17)]
    for px in (None, "libjpeg"):
        a, st_a = mjx.decode_batch(gpu_ctx, datas, pixels=px)
        b, st_b = mjx.decode_batch(gpu_ctx, datas, pixels=px, idct="float")
        try:
            assert st_a == st_b == [mjx.OK] * len(datas)
            for i in range(len(datas)):
                assert tsl.same(a.rgb(i), b.rgb(i)), (px, i)
                if px:
                    lo, hi = lj.interval(datas[i], 64, tsl.oracle_std(datas[i]) if i else None)
                    assert ((a.rgb(i) >= lo) & (a.rgb(i) <= hi)).all(), i          # (the parent's own test of these bytes)
        finally:
            a.close(); b.close()
    ctx = mjx.Context(0, profiling=True)
    try:
        for kw, want in ((dict(pixels=None), 0), (dict(pixels="libjpeg"), 1), (EXACT, 1)):
            bt, _ = mjx.decode_batch(ctx, datas[:3], **kw)
            try:
                bt.kernel_ms(reset=True)
                bt.decode()
                bt.wait()
                k = bt.kernel_ms()
                assert (k["resize"][1] > 0) == bool(want), (kw, k["resize"])
                assert k["idct_color"][1] > 0
            finally:
                bt.close()
    finally:
        ctx.close()

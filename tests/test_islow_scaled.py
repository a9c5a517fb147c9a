"""Exact libjpeg pixels at 1/2, 1/4 and 1/8 (MJX_IDCT_ISLOW with scale_denom 2, 4, 8; include/mjx.h): libjpeg's reduced
integer inverse DCTs, a transform size per component, and its upsampling rule at each scale.

The reference is tests/islow_scaled_ref.py, a numpy int32 restatement of the contract built on islow_ref and libjpeg_ref.
  CPU  the reference equals Pillow's scaled decode (libjpeg-turbo) byte for byte on every file set below, and differs from it with
       fancy upsampling kept on at 1/8 or with one transform size for every component; the lane routines the kernel and the host share
       (mjx_idct_reduced_host) are the reference bit for bit, ignore what the contract says they never read, and run clean under
       AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program; the planner's sizes, tiles and refusals.
  GPU  the decoded picture equals the reference AND Pillow byte for byte; every stream source and both entropy paths give the same
       bytes; constructed extreme blocks equal the reference; rectangles, formats, luminance, resize, orientation, mixed calls, tile
       and mjx_decode compose; a call without the option gives the parent's bytes.
"""
import ctypes
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import islow_ref as isl
import islow_scaled_ref as isr
import scaled_ref
import test_islow_idct as tii
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_sampling_layouts as tsl
import wide_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_DIR, DATA_DIR = tii.PIL_DIR, tii.DATA_DIR
SCALES = (2, 4, 8)
Y420, Y422, Y440, LUMA_SUB = tii.Y420, tii.Y422, tii.Y440, tii.LUMA_SUB
EXACT = dict(pixels="libjpeg-exact")       # (the spelling that opts into the reduced decode; tii.EXACT's, pixels="libjpeg", idct="islow", keeps refusing a scale)
q85, differing, _read = tii.q85, tii.differing, tii._read


# ---- CPU: the reference is Pillow's scaled decode, exactly ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tii.LAYOUT_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_reference_is_pillow_exactly_on_every_layout(orc, size):
    w, h = size
    bad, n = [], 0
    for name in tii.PIL_NAMES:
        data = q85(name, w, h)
        dec = tsl.oracle_std(data)
        for s in SCALES:
            got, want = isr.pixels(data, s, dec), isr.pillow(data, s)
            n += 1
            if not np.array_equal(got, want):
                bad.append((name, s, differing(got, want)))
    assert n == 63 * 3 and bad == [], bad[:8]                                    # (four sizes: 756 cases)


@pytest.mark.parametrize("size", tii.WIDE_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_reference_is_pillow_exactly_with_factors_of_4(size):
    w, h = size
    bad, n = [], 0
    for name in wide_ref.PILLOW_NAMES:
        data, blocks = wide_ref.layout_file(name, w, h)
        dec = wide_ref.dec_of(name, w, h, blocks)
        for s in SCALES:
            got, want = isr.pixels(data, s, dec), isr.pillow(data, s)
            n += 1
            if not np.array_equal(got, want):
                bad.append((name, s, differing(got, want)))
    assert n == 132 * 3 and bad == [], bad[:8]                                   # (two sizes: 792 cases)


WRITTEN = [(w, h, sub) for w, h in ((1, 1), (2, 3), (3, 17), (8, 8), (17, 9), (33, 31), (64, 48), (131, 77)) for sub in (0, 1, 2, "grey")]


def written(w, h, sub):
    from PIL import Image
    src = tii.pillow(_read(os.path.join(DATA_DIR, "lena.jpeg")))[40:40 + h, 60:60 + w]
    im = Image.fromarray(np.ascontiguousarray(src))
    buf = io.BytesIO()
    if sub == "grey":
        im.convert("L").save(buf, "JPEG", quality=90)
    else:
        im.save(buf, "JPEG", quality=90, subsampling=sub)
    return buf.getvalue()


def test_the_reference_is_pillow_exactly_on_pillow_written_files_and_baseline_files(orc):
    """4:4:4, 4:2:2, 4:2:0 and grey at eight sizes down to 1 x 1, s = 1, 2, 4, 8 (128 cases); tests/data and tests/golden/pil at s = 2, 4, 8."""
    bad, n = [], 0
    for case in WRITTEN:
        data = written(*case)
        for s in (1,) + SCALES:
            got, want = isr.pixels(data, s), isr.pillow(data, s)
            n += 1
            if not np.array_equal(got, want):
                bad.append((case, s, differing(got, want)))
    assert n == 128
    files = tii.baseline_files()
    assert len(files) == 34
    for p in files:
        data = _read(p)
        for s in SCALES:
            got, want = isr.pixels(data, s), isr.pillow(data, s)
            if not np.array_equal(got, want):
                bad.append((os.path.basename(p), s, differing(got, want)))
    assert bad == [], bad[:8]


def test_planted_errors_are_not_pillows(orc):
    """Fancy upsampling kept on at 1/8 (4:2:2, 61 x 45), and one transform size N_c = m for every component (4:2:0 at 1/2, where libjpeg
    gives chroma the full 8 x 8 transform and upsamples nothing)."""
    data = q85(Y422, 61, 45)
    dec = tsl.oracle_std(data)
    want = isr.pillow(data, 8)
    assert np.array_equal(isr.pixels(data, 8, dec), want) and not np.array_equal(isr.pixels(data, 8, dec, fancy_at_8=True), want)
    data = q85(Y420, 61, 45)
    dec = tsl.oracle_std(data)
    want = isr.pillow(data, 2)
    assert np.array_equal(isr.pixels(data, 2, dec), want) and not np.array_equal(isr.pixels(data, 2, dec, same_size=True), want)
    assert [g[0] for g in isr.geometry(61, 45, [(2, 2), (1, 1), (1, 1)], 2)] == [4, 8, 8]
    assert [g[3:] for g in isr.geometry(61, 45, [(2, 2), (1, 1), (1, 1)], 2)] == [(1, 1)] * 3


# ---- CPU: the lane routines are the reference, bit for bit -----------------------------------------------------------------------------
def unread(n):
    """[8, 8] bool: the positions the transform of size n never reads"""
    m = np.zeros((8, 8), bool)
    if n == 4:
        m[4, :] = m[:, 4] = True
    elif n == 2:
        m[[2, 4, 6], :] = True
        m[:, [2, 4, 6]] = True
    elif n == 1:
        m[:] = True
        m[0, 0] = False
    return m


@pytest.mark.parametrize("n", [4, 2, 1])
def test_the_lane_routines_are_the_reference_bit_for_bit(mjx, n):
    blocks = tii.extreme_blocks()                                             # (single coefficients, 300 dense blocks, anywhere in 16 bits)
    want = [isr.idct_blocks(c.reshape(1, 8, 8), q.reshape(8, 8).astype(np.int64), n)[0] for c, q in blocks]
    bad = [k for k, ((c, q), w) in enumerate(zip(blocks, want)) if not np.array_equal(mjx.idct_reduced_host(c, q, n), w)]
    assert bad == [], (len(bad), bad[:8])
    flat = np.concatenate([w.reshape(-1) for w in want])
    assert (flat == 0).any() and (flat == 255).any()                             # (saturation at both ends)
    # what the contract says is never read does not matter
    rng = np.random.default_rng(5)
    skip = unread(n).reshape(64)
    for c, q in blocks[64 * 18:64 * 18 + 120]:
        c2 = np.where(skip, rng.integers(-32768, 32768, 64), c).astype(np.int16)
        assert np.array_equal(mjx.idct_reduced_host(c2, q, n), mjx.idct_reduced_host(c, q, n))
    # ... and everything else does: every other position moves some sample of some block
    for pos in np.nonzero(~skip)[0]:
        c = np.zeros(64, np.int16)
        c[pos] = 64
        assert not np.array_equal(mjx.idct_reduced_host(c, np.full(64, 16, np.uint16), n), np.full((n, n), 128, np.uint8)), pos
    # a flat block: DC d gives ((d + 4) >> 3) + 128 in every size; size 8 is the full transform
    for dc, t in ((100, 16), (-100, 16), (1, 1), (-3, 1), (4, 1)):
        c = np.zeros(64, np.int16)
        c[0] = dc
        s = min(max(((dc * t + 4) >> 3) + 128, 0), 255)
        assert np.array_equal(mjx.idct_reduced_host(c, np.full(64, t, np.uint16), n), np.full((n, n), s, np.uint8)), (dc, t)
    c, q = blocks[64 * 18 + 7]
    assert np.array_equal(mjx.idct_reduced_host(c, q, 8), mjx.idct_islow_host(c, q))
    with pytest.raises(mjx.MjxError):
        mjx.idct_reduced_host(c, q, 3)


def test_the_lane_routines_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program (tests/islow_scaled_host.cpp, its own main) under -fsanitize=address,undefined: the three routines on heap
    blocks of exactly 64 words."""
    exe = tmp_path / "islow_scaled_host"
    csrc = os.path.join(ROOT, "jpeg-rust_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", str(exe), os.path.join(ROOT, "tests", "islow_scaled_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = r.stdout.split()
    assert out[0] == "blocks" and int(out[1]) == 3 * (64 * 18 + 300 + 200), r.stdout


# ---- CPU: the planner ----------------------------------------------------------------------------------------------------------------------
def tiles_of(T, hmax, vmax, s, roi, reach_x, reach_y, W=333, H=217):
    """tiles of T MCUs (raster order) that hold an MCU of the rectangle grown by the filter's reach, in scaled coordinates"""
    pw, ph, mcux = 8 * hmax // s, 8 * vmax // s, -(-W // (8 * hmax))
    ow, oh = -(-W // s), -(-H // s)
    x0, y0 = max(roi[0] - reach_x, 0) // pw, max(roi[1] - reach_y, 0) // ph
    x1, y1 = min(roi[0] + roi[2] - 1 + reach_x, ow - 1) // pw, min(roi[1] + roi[3] - 1 + reach_y, oh - 1) // ph
    return len({(my * mcux + mx) // T for my in range(y0, y1 + 1) for mx in range(x0, x1 + 1)})


def test_the_planner_sizes_tiles_and_refusals(mjx):
    hdr = _read(os.path.join(ROOT, "include", "mjx.h")).decode()
    assert "#define MJX_ABI_VERSION 2" in hdr and b"abi=2 " in mjx.lib().mjx_version() and b"islow-scaled" in mjx.lib().mjx_version()
    assert ctypes.sizeof(mjx.Opts) == 32
    # the transform size, the plane sizes and the ratios: libjpeg's own numbers for the layouts everybody uses, the rule for all
    assert [isr.transform_size(4, *f) for f in ((2, 2, 2, 2), (1, 1, 2, 2), (2, 1, 2, 1), (1, 1, 2, 1), (1, 1, 1, 1))] == [4, 8, 4, 4, 4]
    assert [isr.transform_size(1, *f) for f in ((2, 2, 2, 2), (1, 1, 2, 2), (1, 1, 4, 1), (1, 1, 4, 4), (1, 2, 4, 2))] == [1, 2, 1, 4, 1]
    # ... and the PLANNER's numbers (mjx_plan_reduced: red_size, red_plane, the stride and the replicate bits as the device gets them)
    # against the reference's, for every layout -- the 64 of tsl.NAMES and the factor-of-4 ones -- at two sizes and three scales
    def planned_against_the_reference(name, hv, data, w, h):
        bad = []
        if len(hv) == 1:
            hv = [(1, 1)]                                                    # (a one-component file is h = v = 1 whatever its frame says)
        hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
        mcux = -(-w // (8 * hmax))
        scan = mjx.ParsedScan(data)
        try:
            for s in (1,) + SCALES:
                if scan.validate(scale=s, **EXACT) != mjx.OK:
                    bad.append((name, w, h, s, "status"))
                    continue
                got = scan.plan_reduced(scale=s)
                if s == 1:
                    want = [(8, -(-w * a // hmax), -(-h * b // vmax), hmax // a, vmax // b) for a, b in hv]
                else:
                    want = isr.geometry(w, h, hv, s)
                for c, (g, (n, pw, ph, rh, rv)) in enumerate(zip(got, want)):
                    rep = int(s == 8 or (pw <= 2 and rh == 2 and rv in (1, 2)))
                    stride = -(-(mcux * hv[c][0] * n) // 8) * 8
                    if (g["size"], g["plane_w"], g["plane_h"], g["rh"], g["rv"], g["stride"], g["replicated"]) != (n, pw, ph, rh, rv, stride, rep):
                        bad.append((name, w, h, s, c, g, (n, pw, ph, rh, rv, stride, rep)))
                if len(got) != len(hv):
                    bad.append((name, w, h, s, "components", len(got)))
        finally:
            scan.close()
        return bad
    bad, seen = [], set()
    for w, h in ((61, 45), (3, 17)):
        for name in tsl.NAMES:
            bad += planned_against_the_reference(name, tsl.parse_name(name), q85(name, w, h), w, h)
            seen.add(tuple(tsl.parse_name(name)))
        for name in wide_ref.PILLOW_NAMES:
            bad += planned_against_the_reference(name, wide_ref.parse_name(name), wide_ref.layout_file(name, w, h)[0], w, h)
            seen.add(tuple(wide_ref.parse_name(name)))
    assert bad == [], (len(bad), bad[:6])
    assert len(tsl.NAMES) == 64 and len(wide_ref.PILLOW_NAMES) == 132 and len(seen) >= 150
    sizes = {isr.transform_size(8 // s, a, b, max(x for x, _ in hv), max(y for _, y in hv)) for hv in seen for a, b in hv for s in SCALES}
    assert sizes == {1, 2, 4, 8}                                             # (the layouts do reach every transform)
    with pytest.raises(mjx.MjxError):                                        # (the planes of the float transform: not this entry's)
        mjx.ParsedScan(q85(Y420, 61, 45)).plan_reduced(pixels="libjpeg")
    data = q85(Y420, 333, 217)
    scan = mjx.ParsedScan(data)
    try:
        # every refusal keeps its status
        for s in SCALES:
            assert scan.validate(scale=s, pixels="libjpeg") == mjx.ERR_INVALID_ARG                       # (the float transform at a scale)
            assert scan.validate(scale=s, idct="islow") == mjx.ERR_INVALID_ARG                           # (without pixels = libjpeg)
            assert scan.validate(scale=s, layout=mjx.LAYOUT_REF_COMPAT, **EXACT) == mjx.ERR_INVALID_ARG
            assert scan.validate(scale=s, strict_ref=True, **EXACT) == mjx.ERR_INVALID_ARG
            with pytest.raises(mjx.MjxError) as e:
                scan.planes_layout(mjx.Planes("uint8"), scale=s, **EXACT)
            assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT
            ow, oh = -(-333 // s), -(-217 // s)
            assert scan.validate(scale=s, roi=(ow - 1, oh - 1, 1, 1), **EXACT) == mjx.OK
            assert scan.validate(scale=s, roi=(ow - 1, oh - 1, 2, 1), **EXACT) == mjx.ERR_INVALID_ARG
        assert scan.validate(scale=3, **EXACT) == mjx.ERR_INVALID_ARG
        # other colour models: an RGB, CMYK or YCCK picture with the exact pixels stays unsupported, at a scale as at full size
        import colorwriter as cw
        for head, hv in (([cw.app14(0)], [(1, 1)] * 3), ([cw.app14(0)], [(1, 1)] * 4), ([cw.app14(2)], [(2, 2), (1, 1), (1, 1), (2, 2)])):
            other = mjx.ParsedScan(cw.color_jpeg(40, 24, hv, head=head).data, color="file")
            try:
                for s in (1,) + SCALES:
                    assert other.validate(scale=s, color="file", **EXACT) == mjx.ERR_UNSUPPORTED_FORMAT, (len(hv), s)
                    assert other.validate(scale=s, color="file") == mjx.OK
            finally:
                other.close()
        # the opt-in (MJX_OPTS_EXACT_SCALE, byte 13): without it a scale with the exact pixels is refused as it always was
        raw = lambda o: bytes((ctypes.c_uint8 * 32).from_address(ctypes.addressof(o)))
        assert "#define MJX_OPTS_EXACT_SCALE_OFFSET 13" in hdr and mjx.Opts.EXACT_SCALE_OFFSET == 13
        assert "pub const MJX_OPTS_EXACT_SCALE_OFFSET: usize = 13;" in _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
        assert raw(mjx._opts())[13] == 0 and raw(mjx._opts(pixels="libjpeg"))[13] == 0 and raw(mjx._opts(**tii.EXACT))[13] == 0
        assert raw(mjx._opts(pixels="libjpeg-exact"))[12:14] == b"\x01\x01" and raw(mjx._opts(pixels="libjpeg", idct="islow-scaled"))[12:14] == b"\x01\x01"
        assert raw(mjx._opts(pixels="libjpeg-exact", idct="float"))[12:14] == b"\x00\x00"
        assert raw(mjx._opts(pixels="libjpeg-exact", idct="islow"))[12:14] == raw(mjx._opts(pixels="libjpeg-exact", idct=mjx.IDCT_ISLOW))[12:14] == b"\x01\x01"
        assert raw(mjx._opts(pixels="libjpeg", idct=mjx.IDCT_ISLOW))[12:14] == b"\x01\x00"
        for s in SCALES:
            assert scan.validate(scale=s, **tii.EXACT) == mjx.ERR_INVALID_ARG
            assert scan.validate(scale=s, pixels="libjpeg", idct="islow-scaled") == mjx.OK
            assert scan.validate(scale=s, pixels="libjpeg-exact", idct="float") == mjx.ERR_INVALID_ARG
        assert scan.validate(idct="islow-scaled") == mjx.ERR_INVALID_ARG and scan.validate(**EXACT) == mjx.OK
        # the tiles of a rectangle, in scaled coordinates: an MCU is a 16 / s patch.  4:2:0 upsamples nothing at any reduced scale -- Y
        # takes N = m, chroma N = 2 m, the planes are equally large --, so the rectangle's own tiles are read
        full = scan.plan_tiles(scale=2, **EXACT)
        assert full["tiles_read"] == full["tiles_total"] == scan.plan_tiles(**EXACT)["tiles_total"]
        assert [[g[3:] for g in isr.geometry(333, 217, [(2, 2), (1, 1), (1, 1)], s)] for s in SCALES] == [[(1, 1)] * 3] * 3
        for s in SCALES:
            for roi in ((0, 0, 1, 1), (16 // s, 16 // s, 16 // s, 16 // s), (5, 3, 20, 9), (-(-333 // s) - 3, -(-217 // s) - 2, 3, 2)):
                assert scan.plan_tiles(scale=s, roi=roi, **EXACT)["tiles_read"] == tiles_of(full["tile_mcus"], 2, 2, s, roi, 0, 0), (s, roi)
    finally:
        scan.close()
    # 4:2:2: chroma keeps a ratio of (2, 1) at 1/2 and 1/4 -- the (2, 1) filter reaches one sample, 2 pixels, to the left and right and
    # nowhere up or down -- and at 1/8 everything is replicated: no reach
    scan = mjx.ParsedScan(q85(Y422, 333, 217))
    try:
        assert [[g[3:] for g in isr.geometry(333, 217, [(2, 1), (1, 1), (1, 1)], s)] for s in SCALES] == [[(1, 1), (2, 1), (2, 1)]] * 3
        T = scan.plan_tiles(scale=2, **EXACT)["tile_mcus"]
        for s, reach in ((2, 2), (4, 2), (8, 0)):
            for roi in ((0, 0, 1, 1), (16 // s, 8 // s, 16 // s, 8 // s), (16 // s, 0, 1, 1), (32 // s - 1, 3, 1, 9), (5, 3, 20, 9)):
                assert scan.plan_tiles(scale=s, roi=roi, **EXACT)["tiles_read"] == tiles_of(T, 2, 1, s, roi, reach, 0), (s, roi)
    finally:
        scan.close()
    scan = mjx.ParsedScan(data)
    try:
        # a call with the option and no scale plans exactly as before; auto_scale still picks scale 1 with these pixels
        for roi in (None, (20, 10, 9, 7), (0, 16, 61, 16)):
            assert scan.plan_tiles(roi=roi, **EXACT) == scan.plan_tiles(roi=roi, pixels="libjpeg"), roi
        plan = scan.resize_plan(mjx.Resize(8, 6, auto_scale=True), **EXACT)
        assert plan["scale"] == 1 and plan["rect"] == (0, 0, 333, 217), plan
        with pytest.raises(mjx.MjxError):
            scan.resize_plan(mjx.Resize(8, 6, auto_scale=True), scale=4, **EXACT)                        # (auto_scale with a scale: as for any pixels)
        plan = scan.resize_plan(mjx.Resize(8, 6, auto_scale=False), scale=4, **EXACT)
        assert plan["scale"] == 4 and plan["rect"] == (0, 0, 84, 55), plan
    finally:
        scan.close()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
def exact_decode(mjx, ctx, datas, **kw):
    return tii.exact_decode(mjx, ctx, datas, **dict(EXACT, **kw))


def run_out(mjx, ctx, datas, fmt, roi, **kw):
    return tii.run_out(mjx, ctx, datas, fmt, roi, **dict(EXACT, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(61, 45), (40, 24)], ids=lambda s: "%dx%d" % s)
def test_every_layout_equals_the_reference_and_pillow(mjx, gpu_ctx, size):
    w, h = size
    datas = [q85(n, w, h) for n in tii.PIL_NAMES]
    decs = [tsl.oracle_std(d) for d in datas]
    bad = []
    for s in SCALES:
        got = exact_decode(mjx, gpu_ctx, datas, scale=s)
        ref = [isr.pixels(d, s, dec) for d, dec in zip(datas, decs)]
        pil = [isr.pillow(d, s) for d in datas]
        bad += tii.problems([(n, s) for n in tii.PIL_NAMES], got, ref, pil)
    assert len(datas) == 63 and bad == [], bad[:6]


@pytest.mark.gpu
def test_small_wide_and_large_files_equal_the_reference_and_pillow(mjx, gpu_ctx):
    small = [(n, w, h) for n in (Y420, Y422, Y440, "gray22") for w, h in ((3, 17), (2, 2), (1, 1))]
    wide_names = [n for n in wide_ref.NAMED if sum(a * b for a, b in wide_ref.parse_name(n)) <= 10][:8]
    wide = [wide_ref.layout_file(n, 61, 45) for n in wide_names]
    files = [os.path.join(DATA_DIR, "lena.jpeg")]
    big = q85(Y420, 1035, 490)                                           # (many tiles that wrap MCU rows, a partial last MCU row and column)
    datas = [q85(*c) for c in small] + [d for d, _ in wide] + [_read(p) for p in files] + [big]
    cases = small + wide_names + ["lena.jpeg", "420 1035x490"]
    decs = [None] * len(small) + [wide_ref.dec_of(n, 61, 45, blocks) for n, (_, blocks) in zip(wide_names, wide)] + [None, tsl.oracle_std(big)]
    bad = []
    for s in SCALES:
        got = exact_decode(mjx, gpu_ctx, datas, scale=s)
        ref = [isr.pixels(d, s, dec) for d, dec in zip(datas, decs)]
        pil = [isr.pillow(d, s) for d in datas]
        bad += tii.problems([(c, s) for c in cases], got, ref, pil)
    alone = exact_decode(mjx, gpu_ctx, [big], scale=4)                       # (a batch of one: the latency plan's cut of the scan)
    if not tsl.same(alone[0], isr.pillow(big, 4)):
        bad.append("alone")
    assert bad == [], bad[:6]


def child_streams(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = tii.stream_files()
    out, status = {}, {}
    for s in SCALES:
        for dd in (False, True):
            b, st = mjx.decode_batch(ctx, [d for _, d, _ in files], device_destuff=dd, progressive=True, scale=s, **EXACT)
            for i in range(len(files)):
                key = "%d_%d_%d" % (i, dd, s)
                status[key] = st[i] or b.status(i)
                if not status[key]:
                    out[key] = b.rgb(i)
            b.close()
            # alone: a multi-scan picture that fits is read straight from its scans' streams, unless MJX_PLANAR_DIRECT=0 gathers it
            b, st = mjx.decode_batch(ctx, [files[0][1]], device_destuff=dd, scale=s, **EXACT)
            key = "alone_%d_%d" % (dd, s)
            status[key] = st[0] or b.status(0)
            if not status[key]:
                out[key] = b.rgb(0)
            b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=status)))


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_islow_scaled as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_stream_source_and_entropy_path_gives_the_same_bytes(mjx, gpu_ctx, tmp_path):
    files = tii.stream_files()
    want = {s: [isr.pillow(d, s) for _, d, _ in files] for s in SCALES}      # (Pillow reads all four; the reference needs baseline coefficients)
    for s in SCALES:
        assert np.array_equal(want[s][1], want[s][2]) and np.array_equal(want[s][1], isr.pixels(files[1][1], s, tsl.oracle_std(files[1][1])))
        assert np.array_equal(want[s][0], isr.pixels(files[0][1], s))
    bad = []
    for k, env in enumerate(({}, {"MJX_SINGLE_DECODE": "0"}, {"MJX_STREAM_LINEAR": "1"}, {"MJX_PLANAR_DIRECT": "0"})):
        npz = tmp_path / ("streams%d.npz" % k)
        res = run_child(tmp_path, "child_streams(%r)" % str(npz), env)
        with np.load(str(npz)) as z:
            for s in SCALES:
                for dd in (0, 1):
                    for i, (n, _, _) in enumerate(files):
                        key = "%d_%d_%d" % (i, dd, s)
                        if res["status"][key] != 0 or not tsl.same(z[key], want[s][i]):
                            bad.append((n, s, sorted(env.items()), "device de-stuffing" if dd else "host de-stuffing", res["status"][key]))
                    key = "alone_%d_%d" % (dd, s)
                    if res["status"][key] != 0 or not tsl.same(z[key], want[s][0]):
                        bad.append(("ms_420_odd.jpg alone", s, sorted(env.items()), dd, res["status"][key]))
    assert bad == [], bad[:8]


def constructed(hv, mcux, mcuy, qt16, seed):
    """-> (file, its blocks per component in decode order): tii.constructed's file, for the scaled reference"""
    data, _ = tii.constructed(hv, mcux, mcuy, qt16, seed)
    # (the same generator state gives the same blocks: rebuild them for the reference's decode)
    rng = np.random.default_rng(seed)
    per = sum(h * v for h, v in hv) if len(hv) == 3 else 1
    n = mcux * mcuy * per
    blocks = np.zeros((n, 64), np.int64)
    ext = tii.extreme_blocks()
    for b in range(n):
        kind = b % 4
        if kind == 0:
            c = ext[int(rng.integers(0, 64 * 18))][0].astype(np.int64)
            c[0] = np.clip(c[0], -1000, 1000)
            blocks[b] = c[scaled_ref.ZIGZAG]
        elif kind == 1:
            blocks[b] = rng.choice([32767, -32767, 1023, -1023], 64)
            blocks[b, 0] = rng.integers(-1000, 1000)
        elif kind == 2:
            blocks[b] = rng.integers(-40, 40, 64) * (rng.random(64) < 0.3)
            blocks[b, 0] = rng.integers(-500, 500)
        else:
            blocks[b, [0, 1, 5, 6, 14, 15, 27, 28]] = rng.integers(-300, 300, 8)
    mcu = blocks.reshape(mcux * mcuy, per, 64)
    counts, at, coefs = ([h * v for h, v in hv] if len(hv) == 3 else [1]), 0, []
    for k in counts:
        coefs.append(mcu[:, at:at + k].reshape(-1, 64).astype(np.int16))
        at += k
    dec = types.SimpleNamespace(coefs=coefs)
    assert np.array_equal(isl.pixels(data, dec), tii.constructed(hv, mcux, mcuy, qt16, seed)[1])      # (the blocks are the file's)
    return data, dec


@pytest.mark.gpu
@pytest.mark.parametrize("qt16", [False, True], ids=["dqt8", "dqt16"])
def test_constructed_extreme_blocks_equal_the_reference(mjx, gpu_ctx, qt16):
    """Wrap-around and saturation on the device.  Pillow is not asked: its SIMD code works in 16 bits on such blocks."""
    grey, grey_dec = constructed([(1, 1)], 8, 8, qt16, 1)
    col, col_dec = constructed([(2, 2), (1, 1), (1, 1)], 5, 3, qt16, 2)
    bad = []
    for s in SCALES:
        got = exact_decode(mjx, gpu_ctx, [grey, col], scale=s)
        bad += tii.problems([("grey 64x64", s), ("4:2:0", s)], got, [isr.pixels(grey, s, grey_dec), isr.pixels(col, s, col_dec)], [None, None])
    assert bad == [], bad


@pytest.mark.gpu
def test_rectangles_formats_and_luminance_compose(mjx, gpu_ctx):
    bad = []
    # a rectangle in scaled coordinates is the crop of the whole scaled picture
    for lname, W, H in ((Y420, 333, 217), (LUMA_SUB, 61, 45), (Y422, 333, 217)):
        data = q85(lname, W, H)
        dec = tsl.oracle_std(data)
        hv = tsl.parse_name(lname)
        for s in SCALES:
            full = isr.pixels(data, s, dec)
            oh, ow = full.shape[:2]
            rects = tii.rectangles(ow, oh, max(8 * max(h for h, _ in hv) // s, 1), max(8 * max(v for _, v in hv) // s, 1))
            got = exact_decode(mjx, gpu_ctx, [data] * len(rects), rois=rects, scale=s)
            bad += [(lname, s, r) for r, g in zip(rects, got) if not tsl.same(g, full[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])]
    # two output formats and luminance
    cases = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 61, 45)]
    datas = [q85(*c) for c in cases]
    decs = [tsl.oracle_std(d) for d in datas]
    for s, rois in ((2, [None, (3, 5, 20, 15), None, (5, 3, 24, 18)]), (4, [None, (1, 2, 10, 7), None, (2, 1, 12, 9)]), (8, [None, (1, 1, 5, 4), None, None])):
        exact = [isr.pixels(d, s, dec) for d, dec in zip(datas, decs)]
        crop = [e if r is None else np.ascontiguousarray(e[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for e, r in zip(exact, rois)]
        for fmt in (mjx.Output("float16", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD), mjx.Output("uint8", bgr=True)):
            scans = [mjx.ParsedScan(d) for d in datas]
            b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, scale=s, **EXACT)
            try:
                b.decode()
                b.wait()
                bad += [("format", s, fmt.dtype, cases[i], b.status(i)) for i in range(len(datas))
                        if b.status(i) != mjx.OK or not tof.same_bits(b.output(i), tof.expected(crop[i], fmt))]
            finally:
                tsl.close_all(b, scans)
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, rois=rois, output=mjx.Output("uint8", channels=1), scale=s, **EXACT)
        try:
            b.decode()
            b.wait()
            for i, d in enumerate(datas):
                L, r = isr.luma(d, s, decs[i]), rois[i]
                L = L if r is None else L[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]
                if b.status(i) != mjx.OK or not np.array_equal(np.squeeze(b.output(i)), L):
                    bad.append(("luma", s, cases[i], b.status(i)))
        finally:
            tsl.close_all(b, scans)
    assert bad == [], bad[:8]


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    cases = [(Y420, 333, 217), (Y422, 333, 217), ("gray22", 333, 217), (LUMA_SUB, 333, 217)]
    datas = [q85(*c) for c in cases]
    rois = [(11, 7, 48, 36), (3, 5, 48, 36), (0, 9, 48, 36), (101, 50, 48, 36)]
    packed = [np.ascontiguousarray(isr.pixels(d, 2, tsl.oracle_std(d))[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for d, r in zip(datas, rois)]
    dev, n = torch.device("cuda", 0), len(datas)
    big = torch.full((n, 3, 36, 56), float("nan"), dtype=torch.float16, device=dev)
    st = mjx.decode_into(ctx, datas, big[:, :, :, 4:52], rois=rois, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD, scale=2, **EXACT)
    torch.cuda.synchronize()
    fmt = mjx.Output("float16", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD)
    got = big.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, :, 4:52]), tof.expected(packed[i], fmt)):
            bad.append(("f16 planar", i, st[i]))
    if not (np.isnan(got[:, :, :, :4]).all() and np.isnan(got[:, :, :, 52:]).all()):
        bad.append("the padding of the f16 rows was written")
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad)}))


@pytest.mark.gpu
def test_decode_into_a_torch_tensor_with_padded_pitches(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0, res


@pytest.mark.gpu
def test_resize_and_orientation_work_on_the_exact_scaled_intermediate(mjx, gpu_ctx):
    """An explicit scale with a resize, an orientation or both: the parent's rules (test_resize's reference and tolerance,
    test_orientation's map) applied to the reference's scaled picture."""
    datas = [q85(Y420, 333, 217), q85(Y422, 333, 217)]
    s, roi = 2, (5, 10, 150, 95)
    S = [isr.pixels(d, s, tsl.oracle_std(d)) for d in datas]
    packed = [np.ascontiguousarray(p[10:105, 5:155]) for p in S]
    bad = []
    fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
    for aa in (True, False):
        got, scales = run_out(mjx, gpu_ctx, datas, fmt, roi, resize=mjx.Resize(70, 37, antialias=aa, auto_scale=False), scale=s)
        assert scales == [s, s], scales
        for i, g in enumerate(got):
            tx, ty = trs.max_taps(150, 70, aa), trs.max_taps(95, 37, aa)
            p, _, _ = trs.check_against(g, trs.resize_ref(packed[i], 70, 37, aa), fmt, trs.tolerance(tx, ty))
            if p:
                bad.append(("resize", aa, i, p))
    fmt8, r = mjx.Output("uint8"), (5, 9, 60, 50)
    for code in (2, 6, 7):
        got, _ = run_out(mjx, gpu_ctx, datas, fmt8, r, orient=mjx.Orient(exif=False, extra=code), scale=s)
        for i, g in enumerate(got):
            D = tor.orient_np(code, S[i])
            if not tof.same_bits(g, tof.expected(np.ascontiguousarray(D[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), fmt8)):
                bad.append(("orient", code, i))
    code, aa = 6, True
    D = [np.ascontiguousarray(tor.orient_np(code, p)[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for p in S]
    got, _ = run_out(mjx, gpu_ctx, datas, fmt, r, orient=mjx.Orient(exif=False, extra=code), resize=mjx.Resize(33, 40, antialias=aa, auto_scale=False), scale=s)
    for i, g in enumerate(got):
        tx, ty = trs.max_taps(60, 33, aa), trs.max_taps(50, 40, aa)
        p, _, _ = trs.check_against(g, trs.resize_ref(D[i], 33, 40, aa), fmt, trs.tolerance(tx, ty))
        if p:
            bad.append(("resize + orient", i, p))
    assert bad == [], bad[:8]


@pytest.mark.gpu
def test_mixed_calls_tiles_and_mjx_decode(mjx, gpu_ctx):
    """Scales 1 and 4, exact and default pixels side by side.  The options belong to a call, not to a picture, so "mixed" is one batch
    per option set on the same context, back to back -- no single batch can hold two scales or two kinds of pixels."""
    ms = _read(os.path.join(PIL_DIR, "ms_420_odd.jpg"))
    good = [q85(Y420, 333, 217), q85(Y422, 61, 45), q85(LUMA_SUB, 61, 45), q85("gray22", 61, 45), q85(Y420, 3, 17), ms,
            tsl.data_of(Y420, 333, 217, quality=85, restart=3)]
    decs = [tsl.oracle_std(d) for d in good[:5]] + [None, tsl.oracle_std(good[0])]
    want4 = [isr.pixels(d, 4, dec) for d, dec in zip(good, decs)]
    # one batch per option set, the same context, back to back: scales 1 and 4, exact and default pixels
    for kw, want in ((dict(EXACT), [isr.pixels(d, 1, dec) for d, dec in zip(good, decs)]), (dict(EXACT, scale=4), want4)):
        b, st = mjx.decode_batch(gpu_ctx, good, **kw)
        try:
            assert st == [mjx.OK] * len(good), st
            for i in range(len(good)):
                assert tsl.same(b.rgb(i), want[i]), (kw, i)
        finally:
            b.close()
    plain, st = mjx.decode_batch(gpu_ctx, good, scale=4)
    try:
        assert st == [mjx.OK] * len(good) and plain.rgb(0).shape == want4[0].shape and not tsl.same(plain.rgb(0), want4[0])
    finally:
        plain.close()
    # a refused file and a refused rectangle beside good pictures
    b, st = mjx.decode_batch(gpu_ctx, [good[1], _read(os.path.join(PIL_DIR, "progressive.jpg")), good[1]], rois=[None, None, (15, 0, 2, 2)], scale=4, **EXACT)
    try:
        assert st == [mjx.OK, mjx.ERR_UNSUPPORTED_FORMAT, mjx.ERR_INVALID_ARG], st
        assert tsl.same(b.rgb(0), want4[1])
    finally:
        b.close()
    # mjx_decode and the reference's front door
    assert tsl.same(mjx.decode(good[0], pixels="libjpeg-exact", scale=4), want4[0])
    assert tsl.same(mjx.decode(good[4], scale=2, **EXACT), isr.pixels(good[4], 2, decs[4]))
    assert tsl.same(mjx.JPEGImage.parse(good[1], ctx=gpu_ctx, scale=4, **EXACT).image_data(), want4[1])
    # tile(3) keeps the option and the scale
    scans = [mjx.ParsedScan(d) for d in good]
    src = mjx.Batch(gpu_ctx, scans, scale=4, **EXACT)
    try:
        t = src.tile(3)
        try:
            t.decode()
            t.wait()
            n = len(good)
            assert [t.status(i) for i in range(3 * n)] == [mjx.OK] * (3 * n)
            for i in range(3 * n):
                assert tsl.same(t.rgb(i), want4[i % n]), i
        finally:
            t.close()
    finally:
        tsl.close_all(src, scans)


@pytest.mark.gpu
def test_a_call_without_the_option_is_untouched(mjx, gpu_ctx):
    """A scale without the exact pixels is s14's decode, the exact pixels without a scale are s28's: the bytes they gave."""
    datas = [_read(os.path.join(DATA_DIR, "lena.jpeg")), q85(Y420, 333, 217), q85(LUMA_SUB, 61, 45)]
    for s in SCALES:
        b, st = mjx.decode_batch(gpu_ctx, datas, scale=s)
        try:
            assert st == [mjx.OK] * len(datas)
            for i, d in enumerate(datas):
                lo, hi = scaled_ref.rgb_interval(d, s, 64, tsl.oracle_std(d) if i else None)         # (the parent's own test of these bytes)
                assert ((b.rgb(i) >= lo) & (b.rgb(i) <= hi)).all(), (s, i)
        finally:
            b.close()
    b, st = mjx.decode_batch(gpu_ctx, datas, scale=2, **tii.EXACT)              # (the exact pixels without the opt-in: a scale is refused, as it was)
    b.close()
    assert st == [mjx.ERR_INVALID_ARG] * len(datas), st
    b, st = mjx.decode_batch(gpu_ctx, datas, **tii.EXACT)
    try:
        assert st == [mjx.OK] * len(datas)
        for i, d in enumerate(datas):
            assert tsl.same(b.rgb(i), tii.pillow(d)), i
    finally:
        b.close()
    ctx = mjx.Context(0, profiling=True)
    try:
        for kw, want in ((dict(scale=2), 0), (dict(tii.EXACT), 1), (dict(EXACT, scale=2), 1)):
            bt, _ = mjx.decode_batch(ctx, datas, **kw)
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

"""Orientation on the device (mjx_orient, include/mjx.h): EXIF orientation, with per-picture codes on top.

The contract: picture i has a resolved code c -- the file's EXIF tag followed by extra[i] -- and leaves as D = orient_c(S), S the
picture at the call's scale; rectangles are D's.  Without a resize an element is the formats' table (tests/test_output_formats.py)
applied to the byte of the plain packed decode at the mapped pixel, bit for bit; with one it is the resize rule of
tests/test_resize.py applied to orient_c of the packed decode at the (s, R) the batch reports, within that file's derived tolerance
(the arithmetic is the same, the operands are reached through other addresses: no new number).

The reference for the eight codes is the numpy column of the header's table (orient_np), pinned against Pillow's
ImageOps.exif_transpose as an independent reading of the standard.

Not checked without a device: the whole-call failures (a wrong n_extra, from_exif with descriptors) and dst[i] of another size --
the entry points that apply them need a context; they are in the GPU part (test_argument_rules_of_the_entry_points).
"""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import scaled_ref
import test_output_formats as of
import test_resize as trs
import test_roi_decode as roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = range(1, 9)


def orient_np(c, S):
    """The header's table: S [h, w, ...] -> D"""
    S = np.asarray(S)
    t = (1, 0) + tuple(range(2, S.ndim))
    return {1: S, 2: S[:, ::-1], 3: S[::-1, ::-1], 4: S[::-1], 5: S.transpose(t), 6: np.rot90(S, -1),
            7: np.rot90(S, 2).transpose(t), 8: np.rot90(S, 1)}[c]


def swaps(c):
    return c >= 5


# ---- EXIF segments by hand ------------------------------------------------------------------------------------------------------------
def tiff(entries, order="<", ifd_offset=8, count=None):
    """entries: [(tag, type, count, value bytes (4))] -> a TIFF header + IFD0"""
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", 42, ifd_offset)
    body = b"\0" * (ifd_offset - 8)
    ifd = struct.pack(order + "H", len(entries) if count is None else count)
    for tag, typ, cnt, val in entries:
        ifd += struct.pack(order + "HHI", tag, typ, cnt) + val
    return head + body + ifd + struct.pack(order + "I", 0)


def short(order, v):
    return struct.pack(order + "HH", v, 0)


def orientation_entry(order, v, typ=3, cnt=1):
    return (0x0112, typ, cnt, struct.pack(order + "I", v) if typ == 4 else short(order, v))


def exif_segment(t):
    return jw._segment(0xe1, b"Exif\0\0" + t)


def with_segments(data, *segs):
    """the segments go in right behind SOI"""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segs) + data[2:]


def tagged(data, c, order="<"):
    return with_segments(data, exif_segment(tiff([orientation_entry(order, c)], order)))


OTHER = lambda o: [(0x010f, 2, 4, b"abc\0"), (0x0131, 2, 3, b"xy\0\0")]          # Make, Software: entries around the tag


def reader_cases(base):
    """-> [(name, bytes, the code the reader must find)]; base: a small baseline JPEG.  The first case is the fuzzer's seed."""
    cases = [("seed_le_6_among_others", with_segments(base, exif_segment(tiff([OTHER("<")[0], orientation_entry("<", 6), OTHER("<")[1]], "<"))), 6)]
    for o in "<>":
        for v in range(1, 9):
            cases.append(("value_%d_%s" % (v, o), tagged(base, v, o), v))
        for v in (0, 9, 0xffff):
            cases.append(("value_%d_%s" % (v, o), tagged(base, v, o), 1))
        cases.append(("first_%s" % o, with_segments(base, exif_segment(tiff([orientation_entry(o, 5)] + OTHER(o), o))), 5))
        cases.append(("last_%s" % o, with_segments(base, exif_segment(tiff(OTHER(o) + [orientation_entry(o, 7)], o))), 7))
        cases.append(("absent_%s" % o, with_segments(base, exif_segment(tiff(OTHER(o), o))), 1))
        cases.append(("type_long_%s" % o, with_segments(base, exif_segment(tiff([orientation_entry(o, 6, typ=4)], o))), 1))
        cases.append(("count_2_%s" % o, with_segments(base, exif_segment(tiff([orientation_entry(o, 6, cnt=2)], o))), 1))
        cases.append(("ifd_further_on_%s" % o, with_segments(base, exif_segment(tiff([orientation_entry(o, 8)], o, ifd_offset=26))), 8))
    xmp = jw._segment(0xe1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>")
    cases.append(("xmp_in_front", with_segments(base, xmp, exif_segment(tiff([orientation_entry("<", 3)]))), 3))
    cases.append(("two_exif_first_wins", with_segments(base, exif_segment(tiff([orientation_entry("<", 4)])), exif_segment(tiff([orientation_entry(">", 6)], ">"))), 4))
    cases.append(("first_exif_without_tag_wins", with_segments(base, exif_segment(tiff(OTHER("<"))), exif_segment(tiff([orientation_entry("<", 6)]))), 1))
    cases.append(("no_app1", base, 1))
    sos = base.index(b"\xff\xda")
    seglen = struct.unpack(">H", base[sos + 2:sos + 4])[0]
    behind = base[:sos + 2 + seglen] + exif_segment(tiff([orientation_entry("<", 6)])) + base[sos + 2 + seglen:]
    cases.append(("exif_behind_the_sos", behind, 1))
    # malformed: all of them "no tag"
    good = tiff([orientation_entry("<", 6)])
    cases.append(("ifd_offset_beyond_the_segment", with_segments(base, exif_segment(good[:4] + struct.pack("<I", 4000) + good[8:])), 1))
    cases.append(("ifd_offset_at_the_last_byte", with_segments(base, exif_segment(good[:4] + struct.pack("<I", len(good) - 1) + good[8:])), 1))
    cases.append(("entry_count_runs_past", with_segments(base, exif_segment(tiff([orientation_entry("<", 6)], count=200))), 1))
    cases.append(("entry_count_runs_past_by_one", with_segments(base, exif_segment(tiff([orientation_entry("<", 6)])[:-4][:8 + 2 + 11])), 1))
    for cut in (6, 7, 10, 13):                                         # the segment's length cuts the header
        cases.append(("segment_length_cuts_at_%d" % cut, with_segments(base, jw._segment(0xe1, (b"Exif\0\0" + good)[:cut])), 1))
    whole = exif_segment(good)
    for cut in (3, 4, 9, 12, 20, len(whole) - 1):                      # the file ends inside the segment
        cases.append(("file_ends_inside_at_%d" % cut, base[:2] + whole[:cut], 1))
    cases.append(("bad_magic", with_segments(base, exif_segment(good[:2] + b"\x2b\0" + good[4:])), 1))
    cases.append(("bad_byte_order", with_segments(base, exif_segment(b"IM" + good[2:])), 1))
    cases.append(("empty", b"", 1))
    cases.append(("soi_only", b"\xff\xd8", 1))
    return cases


@pytest.fixture(scope="module")
def small_jpeg(mjx):
    return mjx.synth_jpeg(24, 16, "420", 75, seed=2)


# ---- CPU 1: the algebra ------------------------------------------------------------------------------------------------------------------
def test_base_and_strides_equal_the_numpy_column(mjx):
    """A 5 x 3 x 3 array of distinct values (h = 5, w = 3): for every pixel of D the planner's map -- orient_map's base and strides, reached
    through mjx_orient_plan with a 1 x 1 rectangle -- names the pixel of S numpy's column puts there; and D's size."""
    S = np.arange(5 * 3 * 3).reshape(5, 3, 3)
    scan = mjx.ParsedScan(mjx.synth_jpeg(3, 5, "444", 75, seed=1))
    try:
        for c in CODES:
            D = orient_np(c, S)
            whole = scan.orient_plan(c)
            assert (whole["width"], whole["height"]) == (D.shape[1], D.shape[0]) and whole["stored_rect"] == (0, 0, 3, 5)
            for y in range(D.shape[0]):
                for x in range(D.shape[1]):
                    p = scan.orient_plan(c, roi=(x, y, 1, 1))
                    sx, sy, sw, sh = p["stored_rect"]
                    assert (sw, sh, p["width"], p["height"]) == (1, 1, 1, 1)
                    assert np.array_equal(S[sy, sx], D[y, x]), (c, x, y)
    finally:
        scan.close()


def test_compose_is_first_then(mjx):
    S = np.arange(5 * 3 * 3).reshape(5, 3, 3)
    for a in CODES:
        for b in CODES:
            c = mjx.orient_compose(a, b)
            want = orient_np(b, orient_np(a, S))
            got = orient_np(c, S)
            assert got.shape == want.shape and np.array_equal(got, want), (a, b, c)
    for bad in ((0, 1), (1, 0), (9, 2), (2, 255)):
        assert mjx.lib().mjx_orient_compose(*bad) == 0


def test_every_rectangle_maps_back_to_exactly_its_pixels(mjx):
    S = np.arange(4 * 7).reshape(4, 7)                                # a 7 x 4 picture
    scan = mjx.ParsedScan(mjx.synth_jpeg(7, 4, "444", 75, seed=1))
    n = 0
    try:
        for c in CODES:
            D = orient_np(c, S)
            dh, dw = D.shape
            for y in range(dh):
                for h in range(1, dh - y + 1):
                    for x in range(dw):
                        for w in range(1, dw - x + 1):
                            p = scan.orient_plan(c, roi=(x, y, w, h))
                            assert (p["width"], p["height"]) == (w, h)
                            assert np.array_equal(orient_np(c, roi.crop(S, p["stored_rect"])), D[y:y + h, x:x + w]), (c, x, y, w, h)
                            n += 1
    finally:
        scan.close()
    assert n == 8 * (7 * 8 // 2) * (4 * 5 // 2)


def test_pillow_reads_the_standard_the_same_way(mjx):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    import io
    rng = np.random.RandomState(3)
    arr = (rng.randint(0, 256, (5, 9, 3)) // 8 * 8).astype(np.uint8)
    arr[0, 0] = (255, 0, 0); arr[0, -1] = (0, 255, 0); arr[-1, 0] = (0, 0, 255)          # asymmetric whatever the noise
    for c in CODES:
        exif = Image.Exif()
        exif[0x0112] = c
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "JPEG", quality=95, exif=exif)
        data = buf.getvalue()
        im = Image.open(io.BytesIO(data))
        stored = np.asarray(im).copy()
        upright = np.asarray(ImageOps.exif_transpose(im))
        assert np.array_equal(upright, orient_np(c, stored)), c
        assert mjx.exif_orientation(data) == c                       # a segment written by Pillow, read by the library


# ---- CPU 2: the tag reader ------------------------------------------------------------------------------------------------------------------
def test_tag_reader_cases(mjx, small_jpeg):
    cases = reader_cases(small_jpeg)
    assert len(cases) == 58
    for name, data, want in cases:
        assert mjx.exif_orientation(data) == want, name
    lib = mjx.lib()
    c = ctypes.c_uint8()
    assert lib.mjx_exif_orientation(None, 0, ctypes.byref(c)) == mjx.ERR_INVALID_ARG
    assert lib.mjx_exif_orientation(small_jpeg, len(small_jpeg), None) == mjx.ERR_INVALID_ARG
    # mjx_parse is as it was: it skips the segment, and strict_ref still refuses it
    t = tagged(small_jpeg, 6)
    s = mjx.ParsedScan(t)
    assert (s.desc.width, s.desc.height) == (24, 16)
    s.close()
    with pytest.raises(mjx.MjxError) as e:
        mjx.ParsedScan(t, strict_ref=True)
    assert e.value.code == mjx.ERR_UNSUPPORTED_MARKER


def test_tag_reader_under_address_and_undefined_sanitizers(mjx, small_jpeg, tmp_path):
    """A stand-alone program (tests/exif_fuzz.cpp, its own main) with mjx_parse.cpp under -fsanitize=address,undefined: the cases above
    and 20 000 seeded mutations of a valid segment (truncations at every length, byte flips), each in a heap block of exactly its size."""
    cases = reader_cases(small_jpeg)
    blob = tmp_path / "cases.bin"
    with open(blob, "wb") as f:
        for _, data, want in cases:
            f.write(struct.pack("<IB", len(data), want) + data)
    exe = tmp_path / "exif_fuzz"
    csrc = os.path.join(ROOT, "jpeg-rust_amd", "csrc")
    # (the sanitizers' runtimes are linked statically: the program needs nothing from its environment and leaves it alone)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-o", str(exe), os.path.join(ROOT, "tests", "exif_fuzz.cpp"), os.path.join(csrc, "mjx_parse.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(blob), "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.split() == ["cases", str(len(cases)), "mutations", "20000"], r.stdout


# ---- CPU 3: argument rules, per picture (mjx_orient_plan is the planner itself) -------------------------------------------------------------
def test_argument_rules_per_picture(mjx):
    scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))

    def code(c, **kw):
        try:
            scan.orient_plan(c, **kw)
            return mjx.OK
        except mjx.MjxError as e:
            return e.code
    try:
        for c in CODES:
            assert code(c) == mjx.OK
        for c in (0, 9, 255):
            assert code(c) == mjx.ERR_INVALID_ARG
        # a rectangle outside D: D of code 6 is 48 x 64
        assert code(6, roi=(40, 0, 8, 10)) == mjx.OK and code(6, roi=(40, 0, 9, 10)) == mjx.ERR_INVALID_ARG
        assert code(6, roi=(0, 54, 10, 10)) == mjx.OK and code(1, roi=(0, 54, 10, 10)) == mjx.ERR_INVALID_ARG
        assert code(2, roi=(56, 40, 8, 8)) == mjx.OK and code(2, roi=(57, 40, 8, 8)) == mjx.ERR_INVALID_ARG
        assert code(6, roi=(0, 0, 8, 0)) == mjx.ERR_INVALID_ARG
        # ... at the call's scale: 32 x 24 at 1/2, so 24 x 32 for code 8
        assert code(8, roi=(16, 24, 8, 8), scale=2) == mjx.OK and code(8, roi=(17, 24, 8, 8), scale=2) == mjx.ERR_INVALID_ARG
        # REF_COMPAT with an orientation
        assert code(6, layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG and code(2, layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        # with a resize: the resize's own rules, and full-size D coordinates with auto_scale
        rs = mjx.Resize(24, 16)
        assert code(6, resize=rs, roi=(40, 0, 8, 10)) == mjx.OK and code(6, resize=rs, roi=(40, 0, 9, 10)) == mjx.ERR_INVALID_ARG
        assert code(6, resize=rs, scale=2) == mjx.ERR_INVALID_ARG and code(6, resize=mjx.Resize(0, 16)) == mjx.ERR_INVALID_ARG
    finally:
        scan.close()


def test_no_orientation_is_the_resize_entry_points_plan(mjx):
    """orient == NULL is mjx_decode_batch_resize; code 1 is planned as without an orientation: the same scale and rectangle as
    mjx_resize_plan for seeded rectangles and targets, and the same size."""
    rng = np.random.RandomState(4)
    scan = mjx.ParsedScan(mjx.synth_jpeg(333, 217, "420", 75, seed=3))
    try:
        for _ in range(40):
            w, h = int(rng.randint(1, 334)), int(rng.randint(1, 218))
            r = (int(rng.randint(0, 333 - w + 1)), int(rng.randint(0, 217 - h + 1)), w, h)
            rs = mjx.Resize(int(rng.choice([7, 24, 224])), int(rng.choice([7, 16, 224])), antialias=bool(rng.randint(2)))
            a, b = scan.orient_plan(1, resize=rs, roi=r), scan.resize_plan(rs, roi=r)
            assert (a["scale"], a["stored_rect"], a["width"], a["height"]) == (b["scale"], b["rect"], rs.width, rs.height)
            assert scan.orient_plan(1, roi=r)["stored_rect"] == r
            # a transposing code picks its scale with the target's axes swapped into S's
            c = scan.orient_plan(6, resize=rs, roi=(r[1], r[0], r[3], r[2]))
            d = scan.resize_plan(mjx.Resize(rs.height, rs.width, antialias=rs.antialias), roi=(r[0], 217 - r[1] - r[3], r[2], r[3]))
            assert (c["scale"], c["stored_rect"]) == (d["scale"], d["rect"]) and (c["width"], c["height"]) == (rs.width, rs.height)
    finally:
        scan.close()


# ---- CPU 4: mirrors, no device ----------------------------------------------------------------------------------------------------------------
def test_mirrors_of_the_orient_struct_and_entry_points(mjx):
    import re
    hdr = re.sub(r"/\*.*?\*/", "", trs._read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    rs = trs._read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    body = re.search(r"typedef struct mjx_orient\s*\{(.*?)\}\s*mjx_orient;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\**", "", decl)
            fields += [re.sub(r"[\[\]0-9\s\*]", "", x) for x in names.split(",")]
    want = ["from_exif", "extra", "n_extra"]
    assert fields == want and [f[0] for f in mjx.OrientDesc._fields_] == want
    rbody = re.search(r"pub struct mjx_orient\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+): ([^,\n]+),", rbody) == list(zip(want, ["u8", "*const u8", "u32"]))
    assert re.search(r"#\[repr\(C\)\]\s*(#\[[^\]]*\]\s*)*pub struct mjx_orient", rs)
    assert ctypes.sizeof(mjx.OrientDesc) == 24 and mjx.OrientDesc.extra.offset == 8 and mjx.OrientDesc.n_extra.offset == 16
    for fn, n in (("mjx_batch_create_orient", 9), ("mjx_decode_batch_orient", 11), ("mjx_orient_plan", 9), ("mjx_exif_orientation", 3),
                  ("mjx_batch_image_orientation", 3), ("mjx_orient_compose", 2)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*(c_int|u8);", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)
        assert fn in mjx.SYMBOLS and len(mjx.SYMBOLS[fn][1]) == n, fn
    # no new kernel class, and the structs the earlier tests pin are as they were
    assert re.search(r"MJX_K_RESIZE = 10,", hdr) and re.search(r"MJX_K_COUNT = 11", hdr) and len(mjx.KERNEL_NAMES) == 11
    assert ctypes.sizeof(mjx.OutputDesc) == 48 and ctypes.sizeof(mjx.ResizeDesc) == 12
    assert [f[0] for f in mjx.Opts._fields_][-3:] == ["scale_denom", "rois", "n_rois"]


def test_decode_batch_orient_without_a_device_is_a_device_error(tmp_path):
    script = tmp_path / "nodev.py"
    script.write_text(
        "import ctypes, os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "data = open(os.path.join(%r, 'tests', 'data', 'lena.jpeg'), 'rb').read()\n"
        "h = ctypes.c_void_p()\n"
        "print('ctx', mjx.lib().mjx_ctx_create(0, ctypes.byref(h)), bool(h))\n"
        "class C: pass\n"
        "c = C(); c.h = h; c.device = 0\n"
        "try:\n"
        "    mjx.decode_batch(c, [data], orient=mjx.Orient(exif=True, extra=6))\n"
        "    print('decoded')\n"
        "except mjx.MjxError as e:\n"
        "    print('rc', e.code)\n" % (ROOT, ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    dev = str(ge.load_package().ERR_DEVICE)
    assert out.stdout.split() == ["ctx", dev, "False", "rc", dev], out.stdout


# ---- the resized sweep's cases (the band share on the CPU and the GPU sweep walk the same list) -----------------------------------------------
RS_CODES = (1, 2, 3, 6, 7, 8)
RS_TARGETS = ((24, 16), (9, 7), (40, 24))              # the last one an upscale from a 19 x 13 rectangle of D
RS_UP_RECT = (19, 13)
RS_GROUPS = [(aa, auto, t) for aa in (False, True) for auto in (False, True) for t in range(3)]
RS_SCALE = 2                                           # the call's scale where auto_scale is off


def rs_inputs(mjx):
    return [("lena", trs._read(os.path.join(ROOT, "tests", "data", "lena.jpeg"))), ("synth_160x96_420", mjx.synth_jpeg(160, 96, "420")),
            ("synth_75x50_444", mjx.synth_jpeg(75, 50, "444"))]


def rs_cases(mjx, inputs, scans):
    """-> list of dict(g, k, code, aa, auto, target, roi, s, R, taps, fmt2): every group (filter, auto_scale, target) x input x code.  roi is
    D's (full-size D with auto_scale, D at 1 / RS_SCALE otherwise); s, R from mjx_orient_plan; taps from mjx_resize_plan on R with the
    target's axes swapped into S's for the transposing codes (their sum is what the tolerance takes).  fmt2: the group's second format
    next to planar F32, or None where it is a U8 format and the case is not u8_eligible."""
    cases = []
    others = [f for f in range(12) if f != trs.F32_PLANAR]
    for g, (aa, auto, t) in enumerate(RS_GROUPS):
        target = RS_TARGETS[t]
        for k, (name, data) in enumerate(inputs):
            W, H = roi.frame_of(data)[:2]
            pw, ph = (W, H) if auto else (-(-W // RS_SCALE), -(-H // RS_SCALE))
            for c in RS_CODES:
                dw, dh = (ph, pw) if swaps(c) else (pw, ph)
                rng = np.random.RandomState(1000 * g + 10 * k + c)
                if t == 2:
                    r = (int(rng.randint(0, dw - RS_UP_RECT[0] + 1)), int(rng.randint(0, dh - RS_UP_RECT[1] + 1))) + RS_UP_RECT
                else:
                    r = trs._seeded_rect(rng, dw, dh, 9, 9)
                rs = mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto)
                plan = scans[k].orient_plan(c, resize=rs, roi=r, scale=1 if auto else RS_SCALE)
                st = (target[1], target[0]) if swaps(c) else target
                taps = scans[k].resize_plan(mjx.Resize(st[0], st[1], antialias=aa, auto_scale=False), roi=plan["stored_rect"], scale=plan["scale"])
                R = plan["stored_rect"]
                d_wh = (R[3], R[2]) if swaps(c) else R[2:]
                f2 = others[g % 11]
                if of.FORMATS[f2][0] == "uint8" and not trs.u8_eligible(d_wh, target, aa):
                    f2 = None
                cases.append(dict(g=g, k=k, code=c, aa=aa, auto=auto, target=target, roi=r, s=plan["scale"], R=R,
                                  taps=(taps["taps_x"], taps["taps_y"]), fmt2=f2))
    return cases


def test_band_share_of_the_reference_alone_on_oriented_pictures(mjx, orc):
    inputs = rs_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        cases = rs_cases(mjx, inputs, scans)
    finally:
        for s in scans:
            s.close()
    assert len(cases) == 12 * 3 * 6
    decs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True) for _, d in inputs]
    fulls = {}
    band = total = 0
    for c in cases:
        if c["fmt2"] is None or of.FORMATS[c["fmt2"]][0] != "uint8":
            continue
        key = (c["k"], c["s"])
        if key not in fulls:
            fulls[key] = decs[c["k"]].rgb if c["s"] == 1 else scaled_ref.scaled_rgb(inputs[c["k"]][1], c["s"], decs[c["k"]])
        ref = trs.resize_ref(orient_np(c["code"], roi.crop(fulls[key], c["R"])), c["target"][0], c["target"][1], c["aa"])
        tol = trs.tolerance(*c["taps"])
        band += int((np.rint(np.clip(ref - tol, 0, 255)) != np.rint(np.clip(ref + tol, 0, 255))).sum())
        total += ref.size
    print("U8 elements of the oriented sweep: %d, in the band: %d (%.3f %%)" % (total, band, 100.0 * band / max(total, 1)))
    assert total > 20000 and band <= trs.BAND_CAP * total


# ---- GPU: helpers -------------------------------------------------------------------------------------------------------------------------
def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_orientation as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


def packed_decodes(mjx, ctx, scans, scale=1, rois=None):
    b = mjx.Batch(ctx, scans, scale=scale, rois=rois)
    try:
        b.decode(); b.wait()
        assert [b.status(i) for i in range(len(scans))] == [mjx.OK] * len(scans)
        return [b.rgb(i) for i in range(len(scans))]
    finally:
        b.close()


# ---- GPU 1: bit for bit, no resize ------------------------------------------------------------------------------------------------------------
BITS_SIZES = ((1, 1), (3, 5), (17, 65), (31, 33), (64, 64), (65, 63), (257, 129))          # stored w x h
BITS_LAYOUTS = (("420", [(2, 2), (1, 1), (1, 1)], None), ("444", [(1, 1), (1, 1), (1, 1)], None), ("grey", None, (1, 1)))
BITS_FORMATS = (0, 3, 6, 8)
assert [of.FORMATS[f] for f in BITS_FORMATS] == [("uint8", False, False), ("uint8", True, True), ("float16", True, False), ("float32", False, False)]


def child_bits():
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, profiling=True)
    files = []
    for name, hv, gray in BITS_LAYOUTS:
        for (w, h) in BITS_SIZES:
            files.append(("%s_%dx%d" % (name, w, h), jw.layout_jpeg(w, h, hv, seed=w * 131 + h, gray_hv=gray)[0]))
    scans = [mjx.ParsedScan(d) for _, d in files]
    bad, n, launches = [], 0, 0
    for s in (1, 2, 8):
        packed = packed_decodes(mjx, ctx, scans, scale=s)
        many = [sc for sc in scans for _ in CODES]
        codes = [c for _ in scans for c in CODES]
        for f in BITS_FORMATS:
            fmt = of.make_format(mjx, f)
            b = mjx.Batch(ctx, many, scale=s, output=fmt, orient=mjx.Orient(exif=False, extra=codes))
            b.decode(); b.wait()
            launches += b.kernel_ms()["resize"][1]
            for i, c in enumerate(codes):
                k = i // 8
                S = packed[k]
                what = (files[k][0], s, c, of.FORMATS[f])
                n += 1
                if b.status(i) != mjx.OK or b.orientation(i) != c:
                    bad.append(what + ("status / code", b.status(i), b.orientation(i))); continue
                D = np.ascontiguousarray(orient_np(c, S))
                inf = b.info(i)
                if (inf["width"], inf["height"]) != (D.shape[1], D.shape[0]) or b.rect(i) != (0, 0, S.shape[1], S.shape[0]) or b.scale(i) != s:
                    bad.append(what + ("size / rectangle / scale", inf, b.rect(i))); continue
                if not of.same_bits(b.output(i), of.expected(D, fmt)):
                    bad.append(what + ("bits",))
            b.close()
    for sc in scans:
        sc.close()
    ctx.close()
    print(json.dumps({"bad": bad[:30], "nbad": len(bad), "n": n, "launches": int(launches)}))


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
def test_every_code_is_the_table_on_the_mapped_byte_bit_for_bit(mjx, tmp_path, single_decode):
    res = run_child(tmp_path, "child_bits()", {} if single_decode is None else {"MJX_SINGLE_DECODE": single_decode})
    assert res["nbad"] == 0, res
    assert res["n"] == 3 * 7 * 8 * 4 * 3 and res["launches"] >= 12, res


# ---- GPU 2: rectangles ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rectangles_are_the_crop_of_the_oriented_picture_and_read_fewer_tiles(mjx, gpu_ctx):
    W, H = 333, 217
    scan = mjx.ParsedScan(mjx.synth_jpeg(W, H, "420", 75, seed=11))
    try:
        whole = packed_decodes(mjx, gpu_ctx, [scan])[0]
        total = scan.plan_tiles()["tiles_total"]
        assert total >= 6
        rects, codes = [], []
        for c in CODES:
            dw, dh = (H, W) if swaps(c) else (W, H)
            rng = np.random.RandomState(50 + c)
            rs = [(0, 0, dw, dh), (int(rng.randint(dw)) | 1, int(rng.randint(dh)) | 1, 1, 1)]
            while len(rs) < 6:
                w, h = int(rng.randint(1, dw // 3)) | 1, int(rng.randint(1, dh // 3)) | 1
                rs.append((int(rng.randint(0, dw - w)) | 1, int(rng.randint(0, dh - h)) | 1, w, h))
            rs[1] = (min(rs[1][0], dw - 1), min(rs[1][1], dh - 1), 1, 1)
            rects += rs
            codes += [c] * 6
        b = mjx.Batch(gpu_ctx, [scan] * len(rects), rois=rects, orient=mjx.Orient(exif=False, extra=codes))        # out == NULL: interleaved u8
        try:
            b.decode(); b.wait()
            for i, (r, c) in enumerate(zip(rects, codes)):
                assert b.status(i) == mjx.OK and b.orientation(i) == c, (i, r, c)
                D = orient_np(c, whole)
                assert np.array_equal(b.output(i), roi.crop(D, r)), (r, c)
                plan = scan.orient_plan(c, roi=r)
                assert b.rect(i) == plan["stored_rect"] and (b.info(i)["width"], b.info(i)["height"]) == r[2:]
                rr = b.roi(i)
                assert (rr["x"], rr["y"], rr["full_width"], rr["full_height"]) == plan["stored_rect"][:2] + (W, H)      # S's coordinates
                tiles = scan.plan_tiles(roi=plan["stored_rect"])
                if r[2:] == ((H, W) if swaps(c) else (W, H)):
                    assert tiles["tiles_read"] == total
                else:
                    assert tiles["tiles_read"] < total, (r, c, tiles)
        finally:
            b.close()
    finally:
        scan.close()


# ---- GPU 3: caller-owned memory ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_k,pitched", [(6, True), (0, False)], ids=["f16_planar_pitched", "u8_interleaved_dense"])
def test_caller_owned_memory_and_nothing_written_outside(mjx, gpu_ctx, fmt_k, pitched):
    files = [jw.layout_jpeg(w, h, [(2, 2), (1, 1), (1, 1)], seed=7 + w)[0] for (w, h) in ((65, 63), (31, 33), (130, 17))]
    codes = [2, 6, 7]
    scans = [mjx.ParsedScan(d) for d in files]
    hip = of._hip(mjx)
    fmt0 = of.make_format(mjx, fmt_k)
    esz = np.dtype(fmt0.numpy_dtype()).itemsize
    planar = fmt0.planar
    try:
        packed = packed_decodes(mjx, gpu_ctx, scans)
        Ds = [np.ascontiguousarray(orient_np(c, p)) for c, p in zip(codes, packed)]
        guard = 4096
        lay, off = [], guard
        for D in Ds:
            h, w = D.shape[:2]
            rp = (w if planar else 3 * w) + (5 if pitched else 0)
            pp = (h * rp + (11 if pitched else 0)) if planar else 0
            per = ((3 * pp if planar else h * rp) + (13 if pitched else 0)) * esz
            lay.append((off, w, h, rp, pp))
            off += (per + 7) // 8 * 8
        total = off + guard
        base = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(base), total) == 0
        try:
            assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
            dst = [(base.value + o, w, h, rp, pp) for (o, w, h, rp, pp) in lay]
            fmt = of.make_format(mjx, fmt_k, dst=dst)
            b = mjx.Batch(gpu_ctx, scans, output=fmt, orient=mjx.Orient(exif=False, extra=codes))
            try:
                assert b.create_status == [mjx.OK] * 3
                b.decode(); b.wait()
                mem = np.empty(total, np.uint8)
                assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
                covered = np.zeros(total, bool)
                for i, D in enumerate(Ds):
                    o, w, h, rp, pp = lay[i]
                    if planar:
                        el = (np.arange(3)[:, None, None] * pp + np.arange(h)[None, :, None] * rp + np.arange(w)[None, None, :])
                    else:
                        el = (np.arange(h)[:, None, None] * rp + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :])
                    slot = mem[o:].view(fmt.numpy_dtype()) if (total - o) % esz == 0 else mem[o:o + (total - o) // esz * esz].view(fmt.numpy_dtype())
                    assert of.same_bits(np.ascontiguousarray(slot[el]), of.expected(D, fmt)), i
                    covered[(o + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)] = True
                    inf = b.output_info(i)
                    assert (inf["dev"], inf["width"], inf["height"], inf["row_pitch"], inf["plane_pitch"]) == dst[i]
                assert np.all(mem[~covered] == SENTINEL), np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist()
            finally:
                b.close()
            # dst[i] of the stored size instead of D's fails that picture, and only it
            o, w, h, rp, pp = lay[1]
            wrong = list(dst)
            wrong[1] = (dst[1][0], h, w, (h if planar else 3 * h) + 8, (w * (h + 8)) if planar else 0)
            b = mjx.Batch(gpu_ctx, scans, output=of.make_format(mjx, fmt_k, dst=wrong), orient=mjx.Orient(exif=False, extra=codes))
            assert b.create_status == [mjx.OK, mjx.ERR_INVALID_ARG, mjx.OK]
            with pytest.raises(mjx.MjxError):
                b.tile(2)
            b.close()
        finally:
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipFree(base) == 0
    finally:
        for s in scans:
            s.close()


# ---- GPU 4: resized -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resized_sweep_is_the_rule_applied_to_the_oriented_packed_decode(mjx, gpu_ctx):
    inputs = rs_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        cases = rs_cases(mjx, inputs, scans)
        assert len(cases) == 12 * 3 * 6 and set(c["s"] for c in cases if c["auto"]) >= {1, 2, 4}
        packed = trs._packed(mjx, gpu_ctx, scans, set((c["k"], c["s"], c["R"]) for c in cases))
        bad, band, total = [], 0, 0
        for g, (aa, auto, t) in enumerate(RS_GROUPS):
            target = RS_TARGETS[t]
            for second in (False, True):
                cs = [c for c in cases if c["g"] == g and (not second or c["fmt2"] is not None)]
                if not cs:
                    continue
                f = cs[0]["fmt2"] if second else trs.F32_PLANAR
                fmt = of.make_format(mjx, f)
                b = mjx.Batch(gpu_ctx, [scans[c["k"]] for c in cs], scale=1 if auto else RS_SCALE, rois=[c["roi"] for c in cs], output=fmt,
                              resize=mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto),
                              orient=mjx.Orient(exif=False, extra=[c["code"] for c in cs]))
                try:
                    b.decode(); b.wait()
                    for i, c in enumerate(cs):
                        what = (inputs[c["k"]][0], c["code"], aa, auto, target, c["roi"], of.FORMATS[f])
                        inf = b.info(i)
                        if b.status(i) != mjx.OK or (b.scale(i), b.rect(i), b.orientation(i)) != (c["s"], c["R"], c["code"]) or (inf["width"], inf["height"]) != target:
                            bad.append(what + ("status / scale / rectangle / code / size", b.status(i), b.scale(i), b.rect(i), inf)); continue
                        ref = trs.resize_ref(orient_np(c["code"], packed[(c["k"], c["s"], c["R"])]), target[0], target[1], aa)
                        fail, nb, nt = trs.check_against(b.output(i), ref, fmt, trs.tolerance(*c["taps"]))
                        band, total = band + nb, total + nt
                        if fail:
                            bad.append(what + (fail,))
                finally:
                    b.close()
        print("U8 elements %d, in the band %d" % (total, band))
        assert not bad, (len(bad), bad[:10])
        assert total > 20000 and band <= trs.BAND_CAP * total
    finally:
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_a_target_of_the_oriented_rectangles_size_is_the_table_bit_for_bit(mjx, gpu_ctx):
    inputs = rs_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        w, h = 37, 29                                                  # D's rectangle
        for c in (2, 6):
            rois, stored = [], []
            for i, (_, d) in enumerate(inputs):
                W, H = roi.frame_of(d)[:2]
                dw, dh = (H, W) if swaps(c) else (W, H)
                rois.append((min(3 + 5 * i, dw - w), min(2 + 3 * i, dh - h), w, h))
                stored.append(scans[i].orient_plan(c, roi=rois[-1])["stored_rect"])
            packed = packed_decodes(mjx, gpu_ctx, scans, rois=stored)
            for f in range(12):
                fmt = of.make_format(mjx, f)
                for auto in (False, True):
                    b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, resize=mjx.Resize(w, h, antialias=bool(f & 1), auto_scale=auto),
                                  orient=mjx.Orient(exif=False, extra=c))
                    try:
                        b.decode(); b.wait()
                        for i in range(len(scans)):
                            assert b.status(i) == mjx.OK and b.scale(i) == 1 and b.rect(i) == stored[i]
                            want = of.expected(np.ascontiguousarray(orient_np(c, packed[i])), fmt)
                            assert of.same_bits(b.output(i), want), (c, of.FORMATS[f], auto, inputs[i][0])
                    finally:
                        b.close()
    finally:
        for s in scans:
            s.close()


# ---- GPU 5: from file bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_from_file_bytes_tags_extra_flips_and_chunks(mjx, gpu_ctx):
    base = [jw.layout_jpeg(w, h, [(2, 2), (1, 1), (1, 1)], seed=20 + k)[0] for k, (w, h) in enumerate(((70, 45), (33, 64), (129, 31)))]
    files, tags = [], []
    for c in CODES:
        files.append(tagged(base[c % 3], c, "<>"[c & 1])); tags.append(c)
    files.append(base[0]); tags.append(1)                                                         # no tag
    files.append(with_segments(base[1], exif_segment(tiff([orientation_entry("<", 6)], count=200)))); tags.append(1)      # malformed
    n = len(files)
    extra = [2 if i % 2 else 1 for i in range(n)]
    scans = [mjx.ParsedScan(d) for d in files]
    gpu_ctx.set_profiling(True)
    try:
        packed = packed_decodes(mjx, gpu_ctx, scans)
        for f in (None, 6):
            fmt = None if f is None else of.make_format(mjx, f)
            for ex in (None, extra):
                b, st = mjx.decode_batch(gpu_ctx, files, chunk_images=2, output=fmt, orient=mjx.Orient(exif=True, extra=ex))
                try:
                    assert st == [mjx.OK] * n and b.geometry()["chunks"] >= 5
                    for i in range(n):
                        c = mjx.orient_compose(tags[i], 1 if ex is None else ex[i])
                        assert b.orientation(i) == c, (i, c)
                        want = of.expected(np.ascontiguousarray(orient_np(c, packed[i])), fmt or mjx.Output())
                        assert of.same_bits(b.output(i), want), (f, i, c)
                    assert b.kernel_ms()["resize"][1] >= 1
                finally:
                    b.close()
            # Batch from parsed scans reads the tags from the files' bytes itself
            b = mjx.Batch(gpu_ctx, scans, output=fmt, orient=mjx.Orient(exif=True, extra=extra), datas=files)
            try:
                b.decode(); b.wait()
                for i in range(n):
                    c = mjx.orient_compose(tags[i], extra[i])
                    assert b.orientation(i) == c and of.same_bits(b.output(i), of.expected(np.ascontiguousarray(orient_np(c, packed[i])), fmt or mjx.Output()))
            finally:
                b.close()
        # all codes 1: no launch behind stage B, and byte for byte mjx_batch_create_out's pictures
        fmt = of.make_format(mjx, 6)
        plain = mjx.Batch(gpu_ctx, scans[8:], output=fmt)
        plain.decode(); plain.wait()
        b, st = mjx.decode_batch(gpu_ctx, files[8:], output=fmt, orient=mjx.Orient(exif=True))
        try:
            assert st == [mjx.OK] * 2 and b.kernel_ms()["resize"][1] == 0
            for i in range(2):
                assert b.orientation(i) == 1 and of.same_bits(b.output(i), plain.output(i))
        finally:
            b.close(); plain.close()
    finally:
        gpu_ctx.set_profiling(False)
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_argument_rules_of_the_entry_points(mjx, gpu_ctx):
    files = [jw.layout_jpeg(w, h, [(1, 1), (1, 1), (1, 1)], seed=30 + w)[0] for (w, h) in ((40, 24), (24, 40), (33, 17))]
    scans = [mjx.ParsedScan(d) for d in files]
    try:
        # per picture, the neighbours unaffected: a code outside 1 .. 8, a rectangle outside D
        b = mjx.Batch(gpu_ctx, scans, orient=mjx.Orient(exif=False, extra=[6, 9, 2]))
        assert b.create_status == [mjx.OK, mjx.ERR_INVALID_ARG, mjx.OK]
        b.close()
        b = mjx.Batch(gpu_ctx, scans, rois=[(0, 30, 24, 10), (30, 0, 10, 24), (0, 0, 0, 0)], orient=mjx.Orient(exif=False, extra=[6, 6, 0]))
        assert b.create_status == [mjx.OK, mjx.OK, mjx.ERR_INVALID_ARG]
        b.close()
        b = mjx.Batch(gpu_ctx, scans, rois=[(0, 30, 24, 10), (0, 30, 24, 10), (0, 0, 0, 0)], orient=mjx.Orient(exif=False, extra=[6, 6, 3]))
        assert b.create_status == [mjx.OK, mjx.ERR_INVALID_ARG, mjx.OK]                      # (D of picture 1 is 40 x 24)
        b.close()
        b, st = mjx.decode_batch(gpu_ctx, files, layout=mjx.LAYOUT_REF_COMPAT, orient=mjx.Orient(exif=False, extra=[6, 2, 3]))
        assert st == [mjx.ERR_INVALID_ARG] * 3
        b.close()
        # the call: n_extra other than the number of inputs; from_exif with descriptors
        for call in (lambda: mjx.Batch(gpu_ctx, scans, orient=mjx.Orient(exif=False, extra=[6, 2])),
                     lambda: mjx.decode_batch(gpu_ctx, files, orient=mjx.Orient(exif=True, extra=[6, 2, 3, 4]))):
            with pytest.raises(mjx.MjxError) as e:
                call()
            assert e.value.code == mjx.ERR_INVALID_ARG
        arr = (mjx.ScanDesc * 3)()
        for i, s in enumerate(scans):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(s.desc), ctypes.sizeof(mjx.ScanDesc))
        h, od = ctypes.c_void_p(), mjx.OrientDesc(1, None, 0)
        assert mjx.lib().mjx_batch_create_orient(gpu_ctx.h, arr, 3, None, None, None, ctypes.byref(od), ctypes.byref(h), None) == mjx.ERR_INVALID_ARG
        # a tiled batch carries the code along
        b = mjx.Batch(gpu_ctx, scans, orient=mjx.Orient(exif=False, extra=[6, 1, 3]))
        t = b.tile(2)
        t.decode(); t.wait()
        packed = packed_decodes(mjx, gpu_ctx, scans)
        for i in range(6):
            c = [6, 1, 3][i % 3]
            assert t.orientation(i) == c and np.array_equal(t.output(i), orient_np(c, packed[i % 3]))
        t.close(); b.close()
    finally:
        for s in scans:
            s.close()


# ---- GPU 6: torch -----------------------------------------------------------------------------------------------------------------------------------
def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    sizes = [(320, 200, "420", 6), (200, 320, "444", 1), (301, 263, "422", 8), (320, 200, "420", 2), (263, 301, "gray", 3)]
    datas = [tagged(mjx.synth_jpeg(w, h, sub, 75, seed=70 + k), c) for k, (w, h, sub, c) in enumerate(sizes)]
    n = len(datas)
    extra = [1, 2, 1, 5, 1]
    codes = [mjx.orient_compose(s[3], e) for s, e in zip(sizes, extra)]
    dev = torch.device("cuda", 0)
    H, W = 96, 64
    out = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, resize=True, orient=mjx.Orient(exif=True, extra=extra))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    rs = mjx.Resize(W, H)
    portrait = 0
    for i in range(n):
        if st[i] != mjx.OK:
            bad.append(("status", i, st[i])); continue
        scan = mjx.ParsedScan(datas[i])
        plan = scan.orient_plan(codes[i], resize=rs)
        sw, sh = (H, W) if swaps(codes[i]) else (W, H)
        taps = scan.resize_plan(mjx.Resize(sw, sh, auto_scale=False), roi=plan["stored_rect"], scale=plan["scale"])
        scan.close()
        ref, _ = mjx.decode_batch(ctx, [datas[i]], scale=plan["scale"], rois=[plan["stored_rect"]])
        D = orient_np(codes[i], ref.rgb(0))
        ref.close()
        portrait += D.shape[0] > D.shape[1]
        fail, _, _ = trs.check_against(np.ascontiguousarray(got[i]), trs.resize_ref(D, W, H, True), fmt, trs.tolerance(taps["taps_x"], taps["taps_y"]))
        if fail:
            bad.append((i, codes[i], fail))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad), "portrait": int(portrait), "codes": codes}))


@pytest.mark.gpu
def test_decode_into_one_tensor_with_mixed_codes_and_resize(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0 and res["portrait"] >= 2 and len(set(res["codes"])) >= 4, res

"""The colour model of a file (mjx_opts.color = MJX_COLOR_FILE), host side: the decision table against Pillow, mjx_ink_mul against
Pillow's CMYK -> RGB conversion on every pair, the default left as it was, the planner on four-component layouts, and the APP14 / SOF
paths of the parser under the sanitizers (tests/adobe_fuzz.cpp, a stand-alone program).  Nothing here needs a GPU; the decode of these
files is tests/test_color_decode.py."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import colorwriter as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 16
S444 = [(1, 1)] * 3
S4 = [(1, 1)] * 4
LAYOUTS4 = {"1x1x4": [(1, 1)] * 4, "h2_k2": [(2, 1), (1, 1), (1, 1), (2, 1)], "v2_k2": [(1, 2), (1, 1), (1, 1), (1, 2)],
            "y22_k11": [(2, 2), (1, 1), (1, 1), (1, 1)], "y22_k22": [(2, 2), (1, 1), (1, 1), (2, 2)]}

# (name, components, component ids, head segments, the model the rule gives)
TABLE = [
    ("3 jfif", 3, None, [cw.app0()], "ycbcr"),
    ("3 jfif adobe0", 3, None, [cw.app0(), cw.app14(0)], "ycbcr"),
    ("3 jfif ids RGB", 3, b"RGB", [cw.app0()], "ycbcr"),
    ("3 adobe0", 3, None, [cw.app14(0)], "rgb"),
    ("3 adobe1", 3, None, [cw.app14(1)], "ycbcr"),
    ("3 adobe2", 3, None, [cw.app14(2)], "ycbcr"),
    ("3 adobe7", 3, None, [cw.app14(7)], "ycbcr"),
    ("3 adobe1 ids RGB", 3, b"RGB", [cw.app14(1)], "ycbcr"),
    ("3 short adobe0", 3, None, [cw.app14(0, length=11)], "ycbcr"),
    ("3 wrong tag adobe0", 3, None, [cw.app14(0, tag=b"Adobf")], "ycbcr"),
    ("3 ids RGB", 3, b"RGB", [], "rgb"),
    ("3 ids RGB short adobe1", 3, b"RGB", [cw.app14(1, length=11)], "rgb"),
    ("3 ids 123", 3, None, [], "ycbcr"),
    ("4 ids CMYK", 4, b"CMYK", [], "cmyk"),
    ("4 ids 1234", 4, None, [], "cmyk"),
    ("4 adobe0", 4, None, [cw.app14(0)], "cmyk"),
    ("4 adobe1", 4, None, [cw.app14(1)], "ycck"),
    ("4 adobe2", 4, None, [cw.app14(2)], "ycck"),
    ("4 adobe7", 4, None, [cw.app14(7)], "ycck"),
    ("4 jfif adobe2", 4, None, [cw.app0(), cw.app14(2)], "ycck"),
    ("4 jfif", 4, None, [cw.app0()], "cmyk"),
    ("4 short adobe2", 4, None, [cw.app14(2, length=11)], "cmyk"),
    ("4 wrong tag adobe2", 4, None, [cw.app14(2, tag=b"adobe")], "cmyk"),
]


def table_file(ncomp, ids, head):
    return cw.color_jpeg(W, H, S444 if ncomp == 3 else S4, ids=ids, head=head, quality=90, seed=3, noise=2.0).data


def pil(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.fixture(scope="module")
def pil_refs():
    """Pillow's pixels of the table's two scans under heads that leave no doubt: JFIF (YCbCr) and Adobe transform 0 (RGB) for three
    components, Adobe transform 0 (CMYK) and 2 (YCCK) for four."""
    r = {"ycbcr": np.asarray(pil(table_file(3, None, [cw.app0()]))), "rgb": np.asarray(pil(table_file(3, None, [cw.app14(0)]))),
         "cmyk": np.asarray(pil(table_file(4, None, [cw.app14(0)]))), "ycck": np.asarray(pil(table_file(4, None, [cw.app14(2)])))}
    assert not np.array_equal(r["ycbcr"], r["rgb"]) and not np.array_equal(r["cmyk"], r["ycck"])
    return r


@pytest.mark.parametrize("name,ncomp,ids,head,want", TABLE, ids=[t[0] for t in TABLE])
def test_decision_table_agrees_with_pillow(mjx, pil_refs, name, ncomp, ids, head, want):
    data = table_file(ncomp, ids, head)
    got = mjx.color_model(data)
    assert got["name"] == want and got["ncomp"] == ncomp, got
    im = pil(data)
    assert im.mode == ("RGB" if ncomp == 3 else "CMYK")
    # Pillow notes the transform of every APP14 that begins "Adobe" and has a byte 11; libjpeg, which decides, wants 12 bytes
    seen = [s for s in head if s[1] == 0xee and s[4:9] == b"Adobe" and len(s) >= 4 + 12]
    assert got["adobe"] == bool(seen) and (not seen or im.info["adobe_transform"] == got["adobe_transform"] == seen[-1][4 + 11])
    assert got["jfif"] == any(s[1] == 0xe0 for s in head)
    # which of the two readings of the same scan Pillow's pixels are
    a = np.asarray(im)
    other = {"ycbcr": "rgb", "rgb": "ycbcr", "cmyk": "ycck", "ycck": "cmyk"}[want]
    assert np.array_equal(a, pil_refs[want]) and not np.array_equal(a, pil_refs[other])
    # mjx_parse decides with the same routine
    scan = mjx.ParsedScan(data, color="file")
    assert scan.desc.ncomp == ncomp and scan.desc.model == got["model"] == mjx.MODEL_NAMES.index(want)
    scan.close()


def test_grey_and_the_repositorys_own_files(mjx, data_dir):
    g = mjx.synth_jpeg(16, 16, "gray", 75, seed=1)
    assert mjx.color_model(g)["name"] == "grey" and pil(g).mode == "L"
    with open(os.path.join(data_dir, "huff_simple0.jpg"), "rb") as f:
        d = f.read()
    got = mjx.color_model(d)
    assert got["name"] == "ycbcr" and got["jfif"] and got["adobe"] and got["adobe_transform"] == 1 == pil(d).info["adobe_transform"]
    for bad in (b"", b"\xff\xd8", b"\xff\xd8\xff\xd9", d[:40]):
        with pytest.raises(mjx.MjxError) as e:
            mjx.color_model(bad)
        assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT


def test_ink_mul_is_pillows_cmyk_to_rgb_on_every_pair(mjx):
    """Stored value = amount of light: a sample a and K's sample k are the inks 255 - a and 255 - k of Pillow's CMYK mode."""
    a, k = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    cmyk = np.stack([255 - a, 255 - a, 255 - a, 255 - k], axis=-1)
    rgb = np.asarray(Image.frombytes("CMYK", (256, 256), cmyk.tobytes()).convert("RGB"))
    mine = np.array([[mjx.ink_mul(x, y) for y in range(256)] for x in range(256)], np.uint8)
    assert np.array_equal(mine, rgb[..., 0]) and np.array_equal(mine, rgb[..., 1]) and np.array_equal(mine, rgb[..., 2])
    assert np.array_equal(mine, cw.ink_mul(a, k))


def code_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
        return 0
    except Exception as e:          # (MjxError of the loaded package)
        return e.code


def test_default_is_unchanged(mjx):
    four = table_file(4, None, [cw.app14(2)])
    assert code_of(mjx.ParsedScan, four) == mjx.ERR_UNSUPPORTED_FORMAT
    assert code_of(mjx.ParsedScan, four, color="positional") == mjx.ERR_UNSUPPORTED_FORMAT
    # an Adobe transform 0 file of three components: parsed, validated and planned exactly as its copy without the segment
    rgb = cw.color_jpeg(40, 24, [(2, 2), (1, 1), (1, 1)], head=[cw.app14(0)], quality=85, seed=5).data
    a, b = mjx.ParsedScan(rgb), mjx.ParsedScan(cw.strip_app14(rgb))
    assert cw.strip_app14(rgb) != rgb and a.desc.model == b.desc.model == 0 and a.scan_bytes() == b.scan_bytes()
    assert (a.desc.width, a.desc.height, a.desc.ncomp) == (b.desc.width, b.desc.height, b.desc.ncomp) == (40, 24, 3)
    for kw in ({}, {"scale": 2}, {"roi": (3, 2, 20, 11)}, {"pixels": "libjpeg"}):
        assert a.validate(**kw) == b.validate(**kw) == mjx.OK
        assert a.plan_tiles(**kw) == b.plan_tiles(**kw)
    # ... and a description parsed for its own model is Y, Cb, Cr by position again when the call does not ask
    c = mjx.ParsedScan(rgb, color="file")
    assert c.desc.model == mjx.MODEL_RGB and c.validate() == mjx.OK and c.plan_tiles() == a.plan_tiles()
    # 4:2:0 RGB leaves the 4:2:0 kernel's tile for the generic form's
    assert c.validate(color="file") == mjx.OK
    # the option's own rules
    assert code_of(mjx.ParsedScan, rgb, color=2) == mjx.ERR_INVALID_ARG
    assert a.validate(color=2) == mjx.ERR_INVALID_ARG and a.validate(color=255) == mjx.ERR_INVALID_ARG
    assert a.validate(color="file", strict_ref=True) == mjx.ERR_INVALID_ARG
    assert a.validate(color="file", layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
    assert a.validate(color="file") == mjx.OK
    with pytest.raises(mjx.MjxError):
        mjx.ParsedScan(rgb, color="adobe")
    # the refusals that are part of the feature, host side: libjpeg's pixels, luminance and planes of an RGB file
    assert c.validate(color="file", pixels="libjpeg") == mjx.ERR_UNSUPPORTED_FORMAT
    assert code_of(c.output_layout, mjx.Output(channels=1), color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    assert code_of(c.output_layout, mjx.Output(channels=3), color="file") == 0
    assert code_of(c.planes_layout, mjx.Planes(), color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    assert code_of(c.planes_layout, mjx.Planes()) == 0
    for s in (a, b, c):
        s.close()


def test_struct_layouts_kept(mjx):
    """mjx_opts.color sits in the padding behind scale_denom, and the scan description grew at its end only."""
    import ctypes
    assert mjx.Opts.COLOR_OFFSET == 10 and mjx.Opts.scale_denom.offset == 9 and mjx.Opts.rois.offset == 16 and ctypes.sizeof(mjx.Opts) == 32
    o = mjx._opts(color="file", scale=2)
    assert o.color == 1 and bytes(o)[10] == 1 and o.scale_denom == 2 and mjx._opts().color == 0
    assert mjx.ScanDesc.comp_fourth.offset == mjx.ScanDesc.owner_.offset + 8 and mjx.ScanDesc.model.offset == mjx.ScanDesc.comp_fourth.offset + 6
    with open(os.path.join(ROOT, "include", "mjx.h")) as f:
        hdr = f.read()
    assert "#define MJX_OPTS_COLOR_OFFSET 10" in hdr and "mjx_comp comp_fourth;" in hdr and hdr.index("void *owner_;") < hdr.index("mjx_comp comp_fourth;")
    assert "#define MJX_ABI_VERSION 2" in hdr
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as f:
        rs = f.read()
    assert "pub const MJX_OPTS_COLOR_OFFSET: usize = 10;" in rs and "pub comp_fourth: mjx_comp" in rs and "pub fn mjx_color_model" in rs


@pytest.mark.parametrize("name", list(LAYOUTS4))
def test_four_component_layouts_validate_and_plan(mjx, name):
    hv = LAYOUTS4[name]
    bpm = sum(h * v for h, v in hv)
    for head, model in (([cw.app14(0)], mjx.MODEL_CMYK), ([cw.app14(2)], mjx.MODEL_YCCK), ([], mjx.MODEL_CMYK)):
        f = cw.color_jpeg(37, 29, hv, head=head, quality=80, seed=2)
        s = mjx.ParsedScan(f.data, color="file")
        assert s.desc.ncomp == 4 and s.desc.model == model
        assert [(s.desc.comp[c].h, s.desc.comp[c].v) for c in range(3)] + [(s.desc.comp_fourth.h, s.desc.comp_fourth.v)] == hv
        assert s.validate(color="file") == mjx.OK
        assert s.validate() == mjx.ERR_UNSUPPORTED_FORMAT            # (the call must ask as well)
        t = s.plan_tiles(color="file")
        assert t["tiles_total"] == -(-(f.mcux * f.mcuy) // t["tile_mcus"]) and t["tile_mcus"] * bpm <= 256
        for sc in (2, 4, 8):
            assert s.validate(color="file", scale=sc) == mjx.OK
        assert s.validate(color="file", roi=(5, 3, 9, 9)) == mjx.OK
        assert s.validate(color="file", pixels="libjpeg") == mjx.ERR_UNSUPPORTED_FORMAT
        s.close()


def test_frames_the_planner_refuses(mjx):
    # more than ten blocks per MCU: four 2 x 2 components
    big = cw.color_jpeg(32, 32, [(2, 2)] * 4, head=[cw.app14(0)], seed=1)
    s = mjx.ParsedScan(big.data, color="file")
    assert s.validate(color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    assert code_of(s.plan_tiles, color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    s.close()
    eleven = cw.color_jpeg(32, 32, [(2, 2), (2, 1), (1, 1), (2, 2)], head=[cw.app14(0)], seed=1)
    s = mjx.ParsedScan(eleven.data, color="file")
    assert s.validate(color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    s.close()
    # a four-component frame whose first scan carries one component: a multi-scan file
    d = bytearray(cw.color_jpeg(16, 16, S4, head=[cw.app14(0)], seed=1).data)
    i = d.index(b"\xff\xda")
    assert d[i + 4] == 4
    multi = bytes(d[:i]) + b"\xff\xda" + struct.pack(">HB", 8, 1) + bytes(d[i + 5:i + 7]) + bytes(d[i + 13:])
    assert code_of(mjx.ParsedScan, multi, color="file") == mjx.ERR_UNSUPPORTED_FORMAT
    assert mjx.color_model(multi)["name"] == "cmyk"
    # a description of four components that names no four-component model
    s = mjx.ParsedScan(cw.color_jpeg(16, 16, S4, seed=1).data, color="file")
    s.desc.model = mjx.MODEL_RGB
    assert s.validate(color="file") == mjx.ERR_INVALID_ARG
    s.close()


def fuzz_cases(mjx):
    cases = [(table_file(n, ids, head), mjx.MODEL_NAMES.index(want)) for _, n, ids, head, want in TABLE]
    cases.append((mjx.synth_jpeg(16, 16, "gray", 75, seed=1), mjx.MODEL_GREY))
    cases.append((b"\xff\xd8\xff\xd9", 0xff))
    cases.append((cases[0][0][:30], 0xff))
    return cases


def test_app14_and_sof_paths_under_address_and_undefined_sanitizers(mjx, tmp_path):
    """A stand-alone program (tests/adobe_fuzz.cpp, its own main) with mjx_parse.cpp under -fsanitize=address,undefined: the table's
    files and seeded mutations of their heads (truncations at every length, byte flips) through mjx_color_model and mjx_parse with
    MJX_COLOR_FILE, each in a heap block of exactly its size."""
    cases = fuzz_cases(mjx)
    blob = tmp_path / "cases.bin"
    with open(blob, "wb") as f:
        for data, want in cases:
            f.write(struct.pack("<IB", len(data), want) + data)
    exe = tmp_path / "adobe_fuzz"
    csrc = os.path.join(ROOT, "jpeg-rust_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"),
           "-I" + csrc, "-o", str(exe), os.path.join(ROOT, "tests", "adobe_fuzz.cpp"), os.path.join(csrc, "mjx_parse.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(blob), "30000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = r.stdout.split()
    assert out[:3] == ["cases", str(len(cases)), "mutations"] and int(out[3]) >= 30000, r.stdout

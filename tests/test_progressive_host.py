"""Progressive JPEG (SOF2), the host side: the opt-in byte, the accept / refuse table of include/mjx.h (MJX_OPTS_PROGRESSIVE), the levels,
and the three references of the GPU tests held against one another -- no GPU needed.

  (a) Pillow's baseline twin: prog_cases.twins_of asserts that Pillow decodes the two files of a pair to equal arrays;
  (b) tests/prog_ref.py: its coefficients on the progressive twin must equal the oracle's T0 coefficients on the baseline twin;
  (c) tests/progwriter.py: Pillow must decode the writer's file to the pixels of jpegwriter.jpeg_from_blocks' file of the same blocks;
  tests/emul/prog_emul.cpp runs mjx_prog.h's lane routine and its count / copy rule serially: its coefficients must equal (b)'s on all
  twins and writer scripts, its statuses (b)'s on the damaged set; tests/prog_fuzz.cpp drives mjx_parse and the lane routine under
  AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program.
"""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpegwriter
import prog_cases as pc
import prog_ref
import progwriter

ROOT = pc.ROOT
CSRC = os.path.join(ROOT, "jpeg-rust_amd", "csrc")


def _code(mjx, data, progressive, strict=False):
    try:
        scan = mjx.ParsedScan(data, strict_ref=strict, progressive=progressive)
    except mjx.MjxError as e:
        return e.code
    return scan.validate(progressive=progressive)


def _sos_offsets(data):
    """offset of the Ss byte of every SOS header"""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xff:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xd9:
            break
        if m == 0xda:
            out.append(i + 2 + ln - 3)
            i = next(b for a, b in pc.scan_spans(data) if a == i + 2 + ln)
        else:
            i += 2 + ln
    return out


def _patch_scan(data, k, ss=None, se=None, ah=None, al=None, table=None):
    """scan k's header with other spectral selection, successive approximation or table selectors"""
    at = _sos_offsets(data)[k]
    d = bytearray(data)
    if ss is not None:
        d[at] = ss
    if se is not None:
        d[at + 1] = se
    if ah is not None:
        d[at + 2] = (ah << 4) | (d[at + 2] & 15)
    if al is not None:
        d[at + 2] = (d[at + 2] & 0xf0) | al
    if table is not None:
        d[at - 1] = table
    return bytes(d)


def _written(shape, script):
    s = pc.WRITER_SHAPES[shape]
    return progwriter.progressive_from_blocks(pc.constructed_blocks(shape), script, s["hv"], s["mcux"], s["mcuy"], pc.QTS[len(s["hv"])], s["width"], s["height"])


def _many_scans(n):
    """a valid grey script of n scans: the DC from Al = 13 down, then every AC coefficient at Al = 3 and three refinements"""
    sc = [([0], 0, 0, 0, 13)] + [([0], 0, 0, a, a - 1) for a in range(13, 0, -1)]
    for k in range(1, 64):
        sc += [([0], k, k, 0, 3)] + [([0], k, k, a, a - 1) for a in (3, 2, 1)]
    assert len(sc) >= n
    return sc[:n]


def _refusals():
    """name -> (file, status with the opt-in): one file per rule"""
    grey_succ = pc.writer_case("grey_17x9", "successive")[0]           # DC(Al 2), AC(Al 2), DC 2->1, AC 2->1, DC 1->0, AC 1->0
    grey_spec = pc.writer_case("grey_17x9", "spectral")[0]             # DC, 1-5, 6-20, 21-63
    col = pc.writer_case("420_24x24", "spectral")[0]
    U, M = 7, 11                                                       # MJX_ERR_UNSUPPORTED_FORMAT, MJX_ERR_MISSING_TABLE
    sof = grey_spec.index(b"\xff\xc2")
    sof_col = col.index(b"\xff\xc2") + 2 + struct.unpack(">H", col[col.index(b"\xff\xc2") + 2:col.index(b"\xff\xc2") + 4])[0]      # behind the SOF2 segment
    four = b"\xff\xd8" + b"\xff\xc2" + struct.pack(">HBHHB", 8 + 12, 8, 16, 16, 4) + b"".join(bytes([c + 1, 0x11, 0]) for c in range(4)) + b"\xff\xd9"
    return {
        "dc_scan_with_se": (_patch_scan(grey_spec, 0, se=3), U),
        "ac_scan_se_above_63": (_patch_scan(grey_spec, 3, se=64), U),
        "ac_scan_ss_above_se": (_patch_scan(grey_spec, 2, ss=30), U),
        "ac_scan_of_two_components": (_written("420_24x24", [([0, 1, 2], 0, 0, 0, 0), ([0, 1], 1, 63, 0, 0)]), U),
        "al_above_13": (_patch_scan(grey_spec, 0, al=14), U),
        "first_scan_with_ah": (_patch_scan(grey_spec, 1, ah=1), U),
        "ah_is_not_the_previous_al": (_patch_scan(grey_succ, 3, ah=3), U),
        "al_is_not_ah_less_one": (_patch_scan(grey_succ, 3, al=2), U),
        "dc_refinement_out_of_step": (_patch_scan(grey_succ, 2, ah=1, al=0), U),
        "ac_scan_in_front_of_the_dc": (_written("grey_17x9", [([0], 1, 63, 0, 0), ([0], 0, 0, 0, 0)]), U),
        "component_without_a_dc_scan": (_written("420_24x24", [([0, 1], 0, 0, 0, 0), ([0], 1, 63, 0, 0)]), U),
        "scans_256": (_written("grey_17x9", _many_scans(256)), U),
        "four_components": (four, U),
        "baseline_frame_behind_the_scans": (col[:-2] + b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3, 8, 24, 24, 1) + bytes([1, 0x11, 0]) + b"\xff\xd9", U),
        "baseline_frame_behind_the_frame": (col[:sof_col] + b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3, 8, 24, 24, 1) + bytes([1, 0x11, 0]) + col[sof_col:], U),
        "precision_12": (grey_spec[:sof + 4] + b"\x0c" + grey_spec[sof + 5:], U),
        "ac_table_never_defined": (_patch_scan(grey_spec, 1, table=0x03), M),
        "dc_table_never_defined": (_patch_scan(col, 0, table=0x30), M),
    }


def _accepted():
    out = {"pillow_" + x[0]: pc.layout_pair(x[0])[1] for x in pc.LAYOUTS + pc.SIZES[:2]}
    for shape in pc.WRITER_SHAPES:
        for name in pc.writer_scripts(shape):
            out["%s_%s" % (shape, name)] = pc.writer_case(shape, name)[0]
    out["scans_255"] = _written("grey_17x9", _many_scans(255))
    out["dc_only"] = _written("420_24x24", [([0, 1, 2], 0, 0, 0, 0)])             # a progression that stops after its first scan
    return out


def test_accept_and_refuse_table_with_the_opt_in_off_and_on(mjx):
    for name, (data, want) in _refusals().items():
        assert _code(mjx, data, False) == mjx.ERR_UNSUPPORTED_FORMAT, name          # off: every SOF2 frame, as before
        assert _code(mjx, data, True) == want, name
        assert prog_ref.decode(data).status == want or name in ("four_components", "precision_12"), name
    for name, data in _accepted().items():
        assert _code(mjx, data, False) == mjx.ERR_UNSUPPORTED_FORMAT, name
        assert _code(mjx, data, True) == mjx.OK, name
        assert _code(mjx, data, False, strict=True) == mjx.ERR_UNSUPPORTED_MARKER and _code(mjx, data, True, strict=True) == mjx.ERR_UNSUPPORTED_MARKER, name
    # baseline and multi-scan files do not notice the option
    for name in ("opt_420_q85.jpg", "ms_420_odd.jpg", "restart.jpg"):
        data = open(os.path.join(ROOT, "tests", "golden", "pil", name), "rb").read()
        assert _code(mjx, data, True) == _code(mjx, data, False) == mjx.OK, name


def test_option_byte_and_the_reference_modes(mjx):
    prog = pc.layout_pair("420_70x52")[1]
    base = pc.layout_pair("420_70x52")[0]
    for v in (2, 3, 128, 255):
        for data in (prog, base):
            assert _code(mjx, data, v) == mjx.ERR_INVALID_ARG, v
            scan = mjx.ParsedScan(data, progressive=True)
            assert scan.validate(progressive=v) == mjx.ERR_INVALID_ARG, v
    o = mjx._opts(progressive=True)
    assert bytes(o)[11] == 1 and bytes(mjx._opts())[11] == 0 and mjx.ctypes.sizeof(mjx.Opts) == 32
    scan = mjx.ParsedScan(prog, progressive=True)
    assert scan.desc.n_parts == 10 and bool(scan.desc.prog) and scan.desc.ncomp == 3
    assert [(scan.desc.prog[k].ss, scan.desc.prog[k].se, scan.desc.prog[k].ah, scan.desc.prog[k].al) for k in range(3)] == [(0, 0, 0, 1), (1, 5, 0, 2), (1, 63, 0, 1)]
    assert scan.desc.parts[0].ncomp == 3 and list(scan.desc.parts[0].comp) == [0, 1, 2]
    assert scan.validate(progressive=True) == mjx.OK
    assert scan.validate() == mjx.ERR_UNSUPPORTED_FORMAT                            # a progressive description without the opt-in
    assert scan.validate(progressive=True, strict_ref=True) == mjx.ERR_INVALID_ARG
    assert scan.validate(progressive=True, layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
    assert not bool(mjx.ParsedScan(base, progressive=True).desc.prog)              # NULL: a baseline file
    # a hand-changed description answers to the same rules
    scan.desc.prog[1].ah = 1
    assert scan.validate(progressive=True) == mjx.ERR_UNSUPPORTED_FORMAT
    scan.desc.prog[1].ah = 0
    scan.desc.prog[4].se = 64
    assert scan.validate(progressive=True) == mjx.ERR_UNSUPPORTED_FORMAT
    scan.desc.prog[4].se = 63
    assert scan.validate(progressive=True) == mjx.OK


def test_levels(mjx):
    """A scan's level is 1 + the largest level of an earlier scan that touches a common (component, coefficient), an AC scan counting
    its component's first DC scan among them: Pillow's ten scans are four levels, 64 single-coefficient scans two."""
    assert pc.emul_levels(pc.layout_pair("420_70x52")[1]) == [1, 2, 2, 2, 2, 3, 2, 3, 3, 4]
    assert pc.emul_levels(pc.writer_case("grey_17x9", "single_coefficients")[0]) == [1] + [2] * 63
    assert max(pc.emul_levels(pc.writer_case("420_24x24", "al13")[0])) == 14
    assert pc.emul_levels(pc.writer_case("420_24x24", "dc_apart")[0]) == [1, 1, 1, 2, 2, 2]


def _t0(orc, base):
    return orc.interleave(orc.decode(base, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True))


@pytest.mark.parametrize("name", [x[0] for x in pc.LAYOUTS + pc.SIZES])
def test_reference_and_emulation_on_pillow_twins(mjx, orc, name):
    base, prog = pc.layout_pair(name)
    ref = prog_ref.decode(prog)
    assert ref.status == prog_ref.OK
    g = ref.geometry
    real = pc.real_blocks(g["width"], g["height"], pc.hv_of(prog))
    t0 = _t0(orc, base)
    assert t0.shape == ref.coefs.shape and np.array_equal(ref.coefs[real], t0[real])          # (b) against the oracle on the baseline twin
    assert not ref.coefs[~real].any()
    st, co, inf = pc.emul_decode(prog)
    assert st == 0 and np.array_equal(co, ref.coefs) and inf["levels"] == 4


@pytest.mark.parametrize("shape", list(pc.WRITER_SHAPES))
def test_writer_reference_and_emulation_on_constructed_blocks(mjx, orc, shape):
    for name in pc.writer_scripts(shape):
        prog, base, held, real = pc.writer_case(shape, name)
        if name != "stops_early":
            # (c): Pillow on the writer's file and on the baseline file of the same blocks.  (Not for a progression that stops early:
            # libjpeg smooths the blocks of an incomplete progression for display, jdcoefct.c -- the coefficients are not in question.)
            a, b = (np.asarray(Image.open(io.BytesIO(x)).convert("RGB")) for x in (prog, base))
            assert np.array_equal(a, b), name
        ref = prog_ref.decode(prog)
        assert ref.status == prog_ref.OK and np.array_equal(ref.coefs[real], held[real]) and not ref.coefs[~real].any(), name
        assert np.array_equal(_t0(orc, base)[real], held[real]), name
        st, co, _ = pc.emul_decode(prog)
        assert st == 0 and np.array_equal(co, ref.coefs), name
    assert prog_ref.decode(pc.writer_case(shape, "successive")[0]).stats["max_eob_category"] >= 1


def test_constructed_blocks_meet_the_situations_they_are_built_for(mjx):
    """Not the fixture alone: decoding the writer's successive-approximation and libjpeg scripts, the reference must actually run into
    a refinement ZRL whose run passes over coefficients sent earlier, into correction bits inside end-of-band runs, and into runs of
    more than one block; and the emulation -- the kernels' routine -- decodes those very files to the blocks."""
    b = pc.constructed_blocks("420_24x24")
    assert b[:, 1:].max() == 1023 and b[:, 1:].min() == -1023 and b[:, 0].min() == -1024 and b[:, 0].max() == 1016
    assert set(range(-7, 8)) - {0} <= set(np.unique(b[:, 1:]).tolist())
    for shape in pc.WRITER_SHAPES:
        for name in ("successive", "libjpeg"):
            prog, _, held, real = pc.writer_case(shape, name)
            st = prog_ref.decode(prog).stats
            assert st["zrl_over_history"] > 0 and st["eob_run_corrections"] > 0 and st["max_eob_category"] >= 1, (shape, name, st)
            code, co, _ = pc.emul_decode(prog)
            assert code == 0 and np.array_equal(co[real], held[real]), (shape, name)
        last = pc.writer_scripts(shape)["successive"][-1]
        born = (np.abs(pc.constructed_blocks(shape)[:, 1:]) == 1).sum()
        assert last[3:] == (1, 0) and born > 20                     # coefficients born only in the last refinement (+-1)


def test_emulation_statuses_on_the_damaged_set(mjx):
    seen = set()
    for i, data in enumerate(pc.damaged_set()):
        ref = prog_ref.decode(data)
        st, co, _ = pc.emul_decode(data)
        assert st == ref.status, i
        if st == 0:
            assert np.array_equal(co, ref.coefs), i
        seen.add(st)
    assert {prog_ref.OK, prog_ref.TRUNCATED, prog_ref.BAD_HUFFMAN} <= seen


def test_fuzz_program_under_address_and_undefined_behaviour_sanitizers(mjx, tmp_path):
    """tests/prog_fuzz.cpp, a program of its own: every truncation of three small files and seeded mutations of them through
    mjx_parse, the planner and the lane routine.  It must exit clean."""
    files = {"a.jpg": pc.layout_pair("444_17x9")[1], "b.jpg": pc.writer_case("grey_17x9", "successive")[0],
             "c.jpg": pc.pillow_pair(56, 40, "RGB", 2, 75, 3)[1]}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    exe = str(tmp_path / "prog_fuzz")
    srcs = [os.path.join(ROOT, "tests", "prog_fuzz.cpp"), os.path.join(ROOT, "tests", "emul", "prog_emul.cpp")] + [os.path.join(CSRC, s) for s in ("mjx_parse.cpp", "mjx_plan.cpp", "mjx_lut.cpp")]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + srcs, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "2000"] + [str(tmp_path / n) for n in files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runs" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
    assert "status0=" in r.stdout and "status1=" in r.stdout and "status4=" in r.stdout, r.stdout


def test_headers_and_bindings_carry_the_option(mjx):
    hdr = open(os.path.join(ROOT, "include", "mjx.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "#define MJX_OPTS_PROGRESSIVE_OFFSET 11" in hdr and "#define MJX_ABI_VERSION 2" in hdr
    assert "pub const MJX_OPTS_PROGRESSIVE_OFFSET: usize = 11;" in rs and "pub struct mjx_scan_prog" in rs
    assert mjx.Opts.PROGRESSIVE_OFFSET == 11
    assert [f[0] for f in mjx.ScanDesc._fields_][-1] == "prog" and [f[0] for f in mjx.ScanProg._fields_] == ["ss", "se", "ah", "al"]

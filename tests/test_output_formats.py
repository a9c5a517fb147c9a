"""Output formats (mjx_output, include/mjx.h): pictures leave stage B as 3 x H x W or H x W x 3 elements of u8 / f16 / f32, R,G,B or
B,G,R, normalised, in the batch's memory or in device memory of the caller's.

The contract: the u8 value of a sample is exactly the byte the packed decode of the same build writes for that pixel and channel;
F32 is the single-rounded fmaf(float(u8), scale[c], bias[c]) with c the OUTPUT channel, F16 that float rounded to nearest even.
So an element takes one of 256 values per channel, and every GPU comparison here is bit for bit: the reference is the packed RGB of
the same build pushed through a 3 x 256 table that this file builds with exact rational arithmetic (fractions), rounded once to
float32 and once more to half.  The +-1 gate against the oracle is carried by the packed path's own tests; it is repeated here
once, for U8 planar, over the sweep (TOL = 1 per byte, under 1 % of bytes pooled per picture, as tests/test_roi_decode.py).

GPU checks run in a child process per sweep (this module is the child's library), one process building batches at a time.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import scaled_ref
import test_roi_decode as roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1
SCALES = (1, 2, 4, 8)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("uint8", "float16", "float32")
FORMATS = [(d, p, b) for d in DTYPES for p in (False, True) for b in (False, True)]           # the twelve
ESZ = {"uint8": 1, "float16": 2, "float32": 4}


def _read(p):
    with open(p, "rb") as f:
        return f.read()


# ---- the test's own reference -----------------------------------------------------------------------------------------------------
def _round_f32(q):
    """An exact rational -> the nearest float32, ties to even, by integer arithmetic (no float64 on the way)."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)                                             # (subnormals share the smallest exponent)
    scaled = q / Fraction(2) ** (e - 23)                         # the significand in units of the last place
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))         # (n < 2^25 and the power of two: exact in float64 and in float32)


def exact_table(scale, bias):
    """scale, bias: three float32 each -> float32 [3, 256]: fma(v, scale[c], bias[c]) rounded once, from exact rationals."""
    t = np.empty((3, 256), np.float32)
    for c in range(3):
        s, b = Fraction(float(np.float32(scale[c]))), Fraction(float(np.float32(bias[c])))
        for v in range(256):
            t[c, v] = _round_f32(v * s + b)
    return t


def tables_for(fmt):
    """fmt: mjx.Output -> the [3, 256] table of its dtype, by OUTPUT channel (u8: the identity)"""
    if fmt.numpy_dtype() == np.uint8:
        return np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    t = exact_table(fmt.scale, fmt.bias)
    return t if fmt.numpy_dtype() == np.float32 else t.astype(np.float16)         # (numpy rounds float32 -> float16 to nearest even)


def expected(rgb, fmt):
    """The packed picture [H, W, 3] u8 pushed through the format: channel order, table, planarity."""
    t = tables_for(fmt)
    src = rgb[:, :, ::-1] if fmt.bgr else rgb
    out = np.stack([t[c][src[:, :, c]] for c in range(3)], axis=0 if fmt.planar else 2)
    return np.ascontiguousarray(out)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_format(mjx, k, **kw):
    """Format k of the twelve; float formats take the ImageNet constants (in OUTPUT channel order)."""
    d, p, b = FORMATS[k % 12]
    if d == "uint8":
        return mjx.Output(d, planar=p, bgr=b, **kw)
    mean, std = (IMAGENET_MEAN[::-1], IMAGENET_STD[::-1]) if b else (IMAGENET_MEAN, IMAGENET_STD)
    return mjx.Output(d, planar=p, bgr=b, mean=mean, std=std, **kw)


def test_the_reference_table_is_the_fused_single_rounding(mjx):
    fmt = mjx.Output("float32", planar=True, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    sc64 = 1.0 / (255.0 * np.array(IMAGENET_STD, np.float64))
    bi64 = -np.array(IMAGENET_MEAN, np.float64) / np.array(IMAGENET_STD, np.float64)
    assert fmt.scale.dtype == np.float32 and np.array_equal(fmt.scale, sc64.astype(np.float32)) and np.array_equal(fmt.bias, bi64.astype(np.float32))
    t = exact_table(fmt.scale, fmt.bias)
    v = np.arange(256, dtype=np.float64)
    # the float64 route: a byte times a float32 is exact in float64 (8 + 24 bits), the sum is rounded once to 53 bits and once more to
    # 24 -- double rounding could differ from the exact result only on a tie of the second rounding; the assertion says it does not here
    f64 = np.stack([(v * np.float64(fmt.scale[c]) + np.float64(fmt.bias[c])).astype(np.float32) for c in range(3)])
    assert np.array_equal(t.view(np.uint32), f64.view(np.uint32))
    unfused = np.stack([(np.arange(256, dtype=np.float32) * fmt.scale[c]).astype(np.float32) + fmt.bias[c] for c in range(3)]).astype(np.float32)
    differ = int((unfused.view(np.uint32) != t.view(np.uint32)).sum())
    print("entries where the unfused float32(v*s)+b differs from the fused result:", differ, "of 768")
    assert differ >= 1
    h = t.astype(np.float16)
    mag = np.abs(h.astype(np.float64))
    print("smallest |f16| of the table:", float(mag[mag > 0].min()))
    assert np.all((mag == 0) | (mag >= 2.0 ** -14)), "a half value of the table is subnormal"
    assert np.all(np.isfinite(h))
    # _round_f32 itself: exactly representable values, a tie to even, a tie to odd's neighbour
    assert _round_f32(Fraction(1, 3)) == np.float32(1.0 / 3.0) and _round_f32(Fraction(-5, 2)) == np.float32(-2.5)
    assert _round_f32(Fraction(2 ** 24 + 1)) == np.float32(2 ** 24) and _round_f32(Fraction(2 ** 24 + 3)) == np.float32(2 ** 24 + 4)


# ---- CPU: mjx_output_layout ----------------------------------------------------------------------------------------------------------
def _formula(w, h, dtype, planar, row_pitch=None, plane_pitch=None):
    """restated: pitches of a dense picture and the span of bytes from its first element to its last"""
    rmin = w if planar else 3 * w
    rp = rmin if row_pitch is None else row_pitch
    pp = (h * w if plane_pitch is None else plane_pitch) if planar else 0
    last = (2 * pp if planar else 0) + (h - 1) * rp + rmin
    return rp, pp, last * ESZ[dtype]


def test_output_layout_sizes_and_pitches(mjx):
    n = 0
    for (W, H, sub) in ((1001, 37, "420"), (61, 45, "gray"), (333, 217, "422")):
        scan = mjx.ParsedScan(mjx.synth_jpeg(W, H, sub, 75, seed=3))
        try:
            for s in SCALES:
                ow, oh = -(-W // s), -(-H // s)
                for r in (None, (ow // 3, oh // 4, max(1, ow // 2), max(1, oh // 3)), (ow - 1, oh - 1, 1, 1)):
                    w, h = (ow, oh) if r is None else r[2:]
                    got = scan.output_layout(None, roi=r, scale=s)                                 # out == NULL: today's picture
                    assert (got["width"], got["height"], got["bytes"], got["dev"]) == (w, h, w * h * 3, 0), (s, r, got)
                    for k, (d, p, b) in enumerate(FORMATS):
                        got = scan.output_layout(make_format(mjx, k), roi=r, scale=s)
                        rp, pp, nb = _formula(w, h, d, p)
                        assert (got["width"], got["height"], got["row_pitch"], got["plane_pitch"], got["bytes"], got["dev"]) == (w, h, rp, pp, nb, 0), (s, r, d, p, got)
                        assert nb == w * h * 3 * ESZ[d]
                        # pitched, caller-owned: as input 1 of a call of three
                        rp2 = rp + 5
                        pp2 = h * rp2 + 7 if p else 0
                        dev = 0x10000 + 4 * k
                        dst = [(0, 0, 0, 0, 0), (dev, w, h, rp2, pp2), (0, 0, 0, 0, 0)]
                        got = scan.output_layout(make_format(mjx, k, dst=dst), i=1, roi=r, scale=s)
                        _, _, nb2 = _formula(w, h, d, p, rp2, pp2 if p else None)
                        assert (got["row_pitch"], got["plane_pitch"], got["bytes"], got["dev"]) == (rp2, pp2, nb2, dev), (s, r, d, p, got)
                        n += 1
        finally:
            scan.close()
    assert n == 3 * 4 * 3 * 12


def test_output_layout_argument_rules(mjx):
    scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))

    def code(fmt, i=0, **kw):
        try:
            scan.output_layout(fmt, i=i, **kw)
            return mjx.OK
        except mjx.MjxError as e:
            return e.code
    try:
        ok = (0x1000, 64, 48, 64, 64 * 48)
        assert code(mjx.Output("float32", planar=True, dst=[ok])) == mjx.OK
        assert code(mjx.Output(3)) == mjx.ERR_INVALID_ARG and code(mjx.Output(255, planar=True)) == mjx.ERR_INVALID_ARG       # unknown dtype
        assert code(mjx.Output("uint8"), layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        assert code(None, layout=mjx.LAYOUT_REF_COMPAT) == mjx.OK
        for bad in ((0x1000, 63, 48, 64, 64 * 48), (0x1000, 64, 47, 64, 64 * 48),          # not the picture's size
                    (0x1000, 64, 48, 63, 64 * 48), (0x1000, 64, 48, 64, 64 * 48 - 1),      # pitches too small
                    (0x1000, 64, 48, 65, 65 * 48 - 1),
                    (0, 64, 48, 64, 64 * 48), (0x1002, 64, 48, 64, 64 * 48)):              # dev NULL / not aligned to 4
            assert code(mjx.Output("float32", planar=True, dst=[bad])) == mjx.ERR_INVALID_ARG, bad
        assert code(mjx.Output("float16", planar=True, dst=[(0x1002, 64, 48, 64, 64 * 48)])) == mjx.OK
        assert code(mjx.Output("float16", planar=True, dst=[(0x1001, 64, 48, 64, 64 * 48)])) == mjx.ERR_INVALID_ARG
        assert code(mjx.Output("uint8", planar=True, dst=[(0x1001, 64, 48, 64, 64 * 48)])) == mjx.OK
        assert code(mjx.Output("uint8", dst=[(0x1001, 64, 48, 191, 0)])) == mjx.ERR_INVALID_ARG                                 # interleaved: >= 3 * width
        assert code(mjx.Output("uint8", dst=[(0x1001, 64, 48, 192, 0)])) == mjx.OK
        assert code(mjx.Output("uint8", dst=[(0x1001, 16, 8, 48, 0)]), roi=(3, 5, 16, 8)) == mjx.OK                            # the rectangle's size
        assert code(mjx.Output("uint8", dst=[(0x1001, 64, 48, 192, 0)]), roi=(3, 5, 16, 8)) == mjx.ERR_INVALID_ARG
        assert code(mjx.Output("uint8", dst=[(0x1001, 32, 24, 96, 0)]), scale=2) == mjx.OK                                      # the scaled size
        for nf in (float("nan"), float("inf"), -float("inf")):
            assert code(mjx.Output("float32", scale=(1.0, nf, 1.0))) == mjx.ERR_INVALID_ARG
            assert code(mjx.Output("float16", bias=(0.0, 0.0, nf))) == mjx.ERR_INVALID_ARG
            assert code(mjx.Output("uint8", scale=(1.0, nf, 1.0))) == mjx.OK                                                    # (u8 does not look at them)
        # n_dst / dst: the index must lie inside dst[]; a count without an array is refused
        assert code(mjx.Output("uint8", dst=[(0x1001, 64, 48, 192, 0)]), i=1) == mjx.ERR_INVALID_ARG
        d = mjx.Output("uint8").desc()
        d.n_dst = 1
        lay, nb = mjx.Dst(), ctypes.c_size_t()
        o = mjx._opts()
        assert mjx.lib().mjx_output_layout(ctypes.byref(scan.desc), ctypes.byref(o), ctypes.byref(d), 0, ctypes.byref(lay), ctypes.byref(nb)) == mjx.ERR_INVALID_ARG
        assert code(mjx.Output("uint8"), roi=(60, 0, 8, 8)) == mjx.ERR_INVALID_ARG                                              # the picture's own status
    finally:
        scan.close()
    with pytest.raises(mjx.MjxError):
        mjx.Output("float32", mean=IMAGENET_MEAN, scale=(1, 1, 1))


def test_mirrors_of_the_output_structs_and_entry_points(mjx):
    hdr = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()

    def c_fields(struct):
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", hdr, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names = re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\**", "", decl)
                out += [re.sub(r"[\[\]0-9\s\*]", "", x) for x in names.split(",")]
        return out
    want = {"mjx_dst": ["dev", "width", "height", "row_pitch", "plane_pitch"],
            "mjx_output": ["dtype", "planar", "bgr", "scale", "bias", "dst", "n_dst"]}
    rust_types = {"mjx_dst": ["*mut c_void", "u32", "u32", "u64", "u64"], "mjx_output": ["u8", "u8", "u8", "[f32; 3]", "[f32; 3]", "*const mjx_dst", "u32"]}
    for struct, py in (("mjx_dst", mjx.Dst), ("mjx_output", mjx.OutputDesc)):
        assert c_fields(struct) == want[struct]
        assert [f[0] for f in py._fields_] == want[struct]
        body = re.search(r"pub struct " + struct + r"\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
        assert re.findall(r"pub ([a-z_0-9]+): ([^,\n]+),", body) == list(zip(want[struct], rust_types[struct])), struct
        assert re.search(r"#\[repr\(C\)\]\s*(#\[[^\]]*\]\s*)*pub struct " + struct, rs)
    assert ctypes.sizeof(mjx.Dst) == 32 and ctypes.sizeof(mjx.OutputDesc) == 48
    assert mjx.OutputDesc.scale.offset == 4 and mjx.OutputDesc.bias.offset == 16 and mjx.OutputDesc.dst.offset == 32 and mjx.OutputDesc.n_dst.offset == 40
    assert (mjx.DTYPE_U8, mjx.DTYPE_F16, mjx.DTYPE_F32) == (0, 1, 2)
    assert re.search(r"MJX_DTYPE_U8 = 0, MJX_DTYPE_F16 = 1, MJX_DTYPE_F32 = 2", hdr)
    for fn, n in (("mjx_batch_create_out", 7), ("mjx_decode_batch_out", 9), ("mjx_output_layout", 6), ("mjx_batch_output_info", 6), ("mjx_batch_copy_output", 4)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)
        assert fn in mjx.SYMBOLS and len(mjx.SYMBOLS[fn][1]) == n, fn
    # mjx_opts is as it was
    assert [f[0] for f in mjx.Opts._fields_][-3:] == ["scale_denom", "rois", "n_rois"]


def test_decode_batch_out_without_a_device_is_a_device_error(tmp_path):
    """No fallback: with the devices hidden mjx_ctx_create fails, and mjx_decode_batch_out on what it leaves says MJX_ERR_DEVICE."""
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
        "    mjx.decode_batch(c, [data], output=mjx.Output('float16', planar=True))\n"
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


# ---- GPU: the child's library ----------------------------------------------------------------------------------------------------------
def _mode_of(data, scale):
    _, _, comps, _ = scaled_ref.jpeg_tables(data)
    if scale > 1:
        return {2: "3", 4: "4", 8: "1/8"}[scale]
    return "1" if [tuple(c[:2]) for c in comps] == [(2, 2), (1, 1), (1, 1)] else "0"


def _source_of(mjx, ctx, scan, scale):
    """Where stage B reads a picture's entries from: its quad-interleaved stream (a picture of one scan), or for a multi-scan file
    the scans' streams (planar) or a gathered linear stream.  The library says which through mjx_batch_copy_coefs, which has
    nothing to expand for a picture read from its scans (include/mjx.h)."""
    if scan.desc.n_parts == 0:
        return "quad"
    b = mjx.Batch(ctx, [scan], scale=scale)
    try:
        b.decode(); b.wait()
        assert b.status(0) == mjx.OK
        try:
            b.coefs(0)
            return "linear"
        except mjx.MjxError as e:
            assert e.code == mjx.ERR_INVALID_ARG
            return "planar"
    finally:
        b.close()


def child_sweep(group):
    """Every input of the group at every scale, the whole picture and seeded rectangles; picture j of case c takes format
    (c + j) mod 12.  Per scale: one packed batch (the reference) and one batch per format.  Bit for bit against the table; U8
    planar also against the oracle's crop.  Prints failures, the cells hit and the largest figures as JSON."""
    import __graft_entry__ as ge
    import oracle_binding as orc
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad, cells, pairs, worst, npic = [], set(), set(), {"max_diff": 0, "share": 0.0}, 0
    inputs = roi.group_inputs(mjx, orc, group)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    decs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True) for _, d in inputs]
    for s in SCALES:
        pics = []                                                   # (input, rectangle, format)
        for k, (name, data) in enumerate(inputs):
            w, h, hmax, vmax, _ = roi.frame_of(data)
            rects = roi.rectangles(-(-w // s), -(-h // s), 8 // s * hmax, 8 // s * vmax, seed=1000 * k + s)
            pics += [(k, r, (k + s + j) % 12) for j, r in enumerate(rects)]
        npic += len(pics)
        ref = mjx.Batch(ctx, [scans[k] for k, _, _ in pics], scale=s, rois=[r for _, r, _ in pics])
        ref.decode(); ref.wait()
        src = {}
        gate = {}                                                   # input -> [differing bytes, bytes] against the oracle, U8 planar
        for f in range(12):
            mine = [i for i, p in enumerate(pics) if p[2] == f]
            if not mine:
                continue
            fmt = make_format(mjx, f)
            b = mjx.Batch(ctx, [scans[pics[i][0]] for i in mine], scale=s, rois=[pics[i][1] for i in mine], output=fmt)
            b.decode(); b.wait()
            for q, i in enumerate(mine):
                k, r, _ = pics[i]
                name = inputs[k][0]
                if ref.status(i) != mjx.OK or b.status(q) != mjx.OK:
                    bad.append((name, s, r, f, "status", ref.status(i), b.status(q))); continue
                packed = ref.rgb(i)
                got = b.output(q)
                if not same_bits(got, expected(packed, fmt)):
                    bad.append((name, s, r, FORMATS[f], "differs from the table applied to the packed decode")); continue
                if k not in src:
                    src[k] = _source_of(mjx, ctx, scans[k], s)
                pairs.add((_mode_of(inputs[k][1], s), src[k]))
                cells.add((_mode_of(inputs[k][1], s), src[k], f))
                if FORMATS[f][0] == "uint8" and FORMATS[f][1]:
                    full = decs[k].rgb if s == 1 else scaled_ref.scaled_rgb(inputs[k][1], s, decs[k])
                    want = roi.crop(full, r)
                    back = np.transpose(got, (1, 2, 0))
                    back = back[:, :, ::-1] if FORMATS[f][2] else back
                    d = np.abs(back.astype(np.int32) - want.astype(np.int32))
                    worst["max_diff"] = max(worst["max_diff"], int(d.max()))
                    if d.max() > TOL:
                        bad.append((name, s, r, "oracle", int(d.max())))
                    g = gate.setdefault(k, [0, 0])
                    g[0] += int((d > 0).sum()); g[1] += d.size
            b.close()
        ref.close()
        for k, (nd, nb) in gate.items():
            worst["share"] = max(worst["share"], nd / max(nb, 1))
            if nd >= 0.01 * nb:
                bad.append((inputs[k][0], s, "share of differing bytes over the picture's U8 planar rectangles", nd, nb))
    missing = sorted((m, so, f) for (m, so) in pairs for f in range(12) if (m, so, f) not in cells)
    for sc in scans:
        sc.close()
    ctx.close()
    print(json.dumps({"bad": bad[:40], "nbad": len(bad), "pictures": npic, "pairs": sorted(pairs), "cells": len(cells), "missing": missing[:40],
                      "worst": worst}))


def run_child(tmp_path, call, env_set=None, timeout=1500):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_output_formats as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


MODES = ("0", "1", "3", "4", "1/8")


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
@pytest.mark.parametrize("group", roi.GROUPS)
def test_sweep_every_format_is_the_table_applied_to_the_packed_decode(mjx, tmp_path, group, single_decode):
    res = run_child(tmp_path, "child_sweep(%r)" % group, {} if single_decode is None else {"MJX_SINGLE_DECODE": single_decode})
    assert res["nbad"] == 0, res
    assert res["missing"] == [] and res["cells"] == 12 * len(res["pairs"]), res           # every (mode, stream source, format) cell that exists
    pairs = set(tuple(p) for p in res["pairs"])
    sources = ("linear", "planar") if group == "scripts" else ("quad",)                  # (all three stream sources over the five groups)
    assert pairs >= set((m, so) for m in MODES for so in sources), res
    assert res["pictures"] > 100 and res["worst"]["max_diff"] <= TOL and res["worst"]["share"] < 0.01, res


# ---- GPU: caller-owned memory -------------------------------------------------------------------------------------------------------------
def _hip(mjx):
    h = roi._hip(mjx)
    h.hipMalloc.restype = h.hipFree.restype = ctypes.c_int
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_images", [0, 2])
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("fmt_k", [3, 6, 10, 1], ids=["u8_planar_bgr", "f16_planar", "f32_planar", "u8_interleaved_bgr"])
def test_caller_owned_memory_and_nothing_written_outside(mjx, orc, gpu_ctx, fmt_k, pitched, chunk_images):
    """One hipMalloc holds N x 3 x h x w (or N x h x w x 3) for equal-size rectangles of pictures of different sizes and samplings;
    guards in front and behind, everything sentinel-filled; an undecodable file and a picture with a wrong dst.width keep their
    slots untouched."""
    datas = roi._mixed_inputs(mjx, orc)
    undecodable, wrong, wrong_ms = 6, 2, 4            # (wrong_ms: a multi-scan file -- its scans' plans go with the refused picture)
    w, h = 29, 23
    scale = 1
    rois = []
    for i, d in enumerate(datas):
        W, H = (64, 64) if i == undecodable else roi.frame_of(d)[:2]
        rois.append((min(3 + 5 * i, W - w), min(2 + 3 * i, H - h), w, h))
    n = len(datas)
    fmt0 = make_format(mjx, fmt_k)
    esz = np.dtype(fmt0.numpy_dtype()).itemsize
    planar = fmt0.planar
    rp = (w if planar else 3 * w) + (5 if pitched else 0)
    pp = (h * rp + (11 if pitched else 0)) if planar else 0
    per = (3 * pp if planar else h * rp) + (13 if pitched else 0)                         # elements per picture slot
    guard = 4096
    total = guard + n * per * esz + guard
    hip = _hip(mjx)
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [(base.value + guard + i * per * esz, w + (1 if i in (wrong, wrong_ms) else 0), h, rp + (3 if i in (wrong, wrong_ms) and not planar else 0), pp) for i in range(n)]
        fmt = make_format(mjx, fmt_k, dst=dst)
        good = [i for i in range(n) if i not in (undecodable, wrong, wrong_ms)]
        b, st = mjx.decode_batch(gpu_ctx, datas, scale=scale, rois=rois, chunk_images=chunk_images, output=fmt)
        try:
            assert st[wrong] == mjx.ERR_INVALID_ARG and st[wrong_ms] == mjx.ERR_INVALID_ARG and st[undecodable] == mjx.ERR_UNSUPPORTED_FORMAT, st          # each its own code
            assert [st[i] for i in good] == [mjx.OK] * len(good), st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            covered = np.zeros(total, bool)
            for i in good:
                assert b.status(i) == mjx.OK
                want = expected(roi.crop(roi._full(mjx, gpu_ctx, datas[i], scale), rois[i]), fmt)
                slot = mem[guard + i * per * esz: guard + (i + 1) * per * esz].view(fmt.numpy_dtype())
                if planar:
                    el = (np.arange(3)[:, None, None] * pp + np.arange(h)[None, :, None] * rp + np.arange(w)[None, None, :])
                else:
                    el = (np.arange(h)[:, None, None] * rp + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :])
                assert same_bits(np.ascontiguousarray(slot[el]), want), ("picture", i)
                bytes_at = (guard + i * per * esz + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)
                covered[bytes_at] = True
                inf = b.output_info(i)
                assert (inf["dev"], inf["width"], inf["height"], inf["row_pitch"], inf["plane_pitch"]) == dst[i], (i, inf)
                assert (inf["dtype"], inf["planar"], inf["bgr"]) == (fmt.dtype, fmt.planar, fmt.bgr)
                with pytest.raises(mjx.MjxError):
                    b.output(i)                                      # mjx_batch_copy_output serves library-owned output only
            assert np.all(mem[~covered] == SENTINEL), ("bytes outside the pictures' elements were written", np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist())
            assert b.status(wrong) == mjx.ERR_INVALID_ARG and b.status(wrong_ms) == mjx.ERR_INVALID_ARG and b.status(undecodable) != mjx.OK
            assert b.bytes()["rgb"] == len(good) * w * h * 3 * esz
            if chunk_images:
                assert b.geometry()["chunks"] >= 3
        finally:
            b.close()
        # mjx_batch_tile refuses caller-owned destinations: the copies would share them
        scans = [mjx.ParsedScan(datas[i]) for i in good[:2]]
        two = mjx.Batch(gpu_ctx, scans, scale=scale, rois=[rois[i] for i in good[:2]], output=make_format(mjx, fmt_k, dst=[dst[i] for i in good[:2]]))
        try:
            assert two.create_status == [mjx.OK, mjx.OK]
            with pytest.raises(mjx.MjxError) as e:
                two.tile(2)
            assert e.value.code == mjx.ERR_INVALID_ARG
        finally:
            two.close()
            for s in scans:
                s.close()
    finally:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipFree(base) == 0


# ---- GPU: front doors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_front_doors(mjx, orc, gpu_ctx):
    paths = [os.path.join(ROOT, "tests", "data", "lena.jpeg"), os.path.join(ROOT, "tests", "golden", "pil", "dri_422_rows.jpg"),
             os.path.join(ROOT, "tests", "golden", "pil", "ms_420_odd.jpg"), os.path.join(ROOT, "tests", "data", "lena-bw.jpeg")]
    datas = [_read(p) for p in paths] + [mjx.synth_jpeg(1920, 1080, "420", 75, seed=9)]
    n = len(datas)
    for s in SCALES:
        fulls = [roi._full(mjx, gpu_ctx, d, s) for d in datas]
        rois = []
        for i, (d, f) in enumerate(zip(datas, fulls)):
            _, _, hmax, vmax, _ = roi.frame_of(d)
            rs = roi.rectangles(f.shape[1], f.shape[0], 8 // s * hmax, 8 // s * vmax, seed=5 + i)
            rois.append(rs[0] if i == 1 else rs[7 + (i + s) % 3])
        packed = [roi.crop(f, r) for f, r in zip(fulls, rois)]
        scans = [mjx.ParsedScan(d) for d in datas]
        try:
            for k in (s % 12, (s + 5) % 12, (s + 10) % 12):
                fmt = make_format(mjx, k)
                want = [expected(p, fmt) for p in packed]
                b = mjx.Batch(gpu_ctx, scans, scale=s, rois=rois, output=fmt)                 # mjx_batch_create_out
                try:
                    b.decode(); b.wait()
                    created = [b.output(i) for i in range(n)]
                    for i in range(n):
                        assert b.status(i) == mjx.OK and same_bits(created[i], want[i]), (s, k, i)
                        p, nb = b.rgb_device(i)
                        assert nb == want[i].nbytes and p == b.output_info(i)["dev"]
                        with pytest.raises(mjx.MjxError) as e:
                            b.rgb(i)                                                           # copy_rgb: not packed RGB
                        assert e.value.code == mjx.ERR_INVALID_ARG
                    assert b.bytes()["rgb"] == sum(x.nbytes for x in want)
                    mx, cnt = b.compare_rgb(list(range(n)), b, list(range(n)))
                    assert [int(v) for v in mx] == [0xffffffff] * n
                    t = b.tile(3)                                                              # a library-owned format is replicated
                    try:
                        t.decode(); t.wait()
                        for i in range(3 * n):
                            assert same_bits(t.output(i), want[i % n]), (s, k, i)
                            inf = t.output_info(i)
                            assert (inf["dtype"], inf["planar"], inf["bgr"]) == (fmt.dtype, fmt.planar, fmt.bgr)
                        assert t.bytes()["rgb"] == 3 * b.bytes()["rgb"]
                    finally:
                        t.close()
                finally:
                    b.close()
                for dd in (True, False):                                                       # mjx_decode_batch_out, both de-stuffings
                    fb, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd, scale=s, rois=rois, output=fmt)
                    try:
                        assert st == [mjx.OK] * n
                        for i in range(n):
                            assert same_bits(fb.output(i), created[i]), (dd, s, k, i)
                    finally:
                        fb.close()
            # out == NULL and the all-default description: the packed path's bytes
            o = mjx._opts(scale=s, rois=rois)
            arr = (mjx.ScanDesc * n)()
            for i, sc in enumerate(scans):
                ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(sc.desc), ctypes.sizeof(mjx.ScanDesc))
            h, st = ctypes.c_void_p(), (ctypes.c_int * n)()
            assert mjx.lib().mjx_batch_create_out(gpu_ctx.h, arr, n, ctypes.byref(o), None, ctypes.byref(h), st) == mjx.OK
            b0 = mjx.Batch(gpu_ctx, _handle=h)
            b1 = mjx.Batch(gpu_ctx, scans, scale=s, rois=rois, output=mjx.Output())
            try:
                for b in (b0, b1):
                    b.decode(); b.wait()
                for i in range(n):
                    assert np.array_equal(b0.rgb(i), packed[i]), (s, i)
                    assert same_bits(b1.output(i), packed[i]), (s, i)
                    inf = b0.output_info(i)
                    assert (inf["dtype"], inf["planar"], inf["bgr"], inf["row_pitch"]) == (0, False, False, 3 * packed[i].shape[1])
                mx, _ = b0.compare_rgb(list(range(n)), b0, list(range(n)))
                assert int(mx.max()) == 0
            finally:
                b0.close()
                b1.close()
        finally:
            for sc in scans:
                sc.close()
    # n_dst other than 0 or n fails the call
    scans = [mjx.ParsedScan(d) for d in datas[:2]]
    try:
        for dst in ([(0x1000, 8, 8, 24, 0)], [(0x1000, 8, 8, 24, 0)] * 3):
            with pytest.raises(mjx.MjxError) as e:
                mjx.Batch(gpu_ctx, scans, output=mjx.Output("uint8", dst=dst))
            assert e.value.code == mjx.ERR_INVALID_ARG
            with pytest.raises(mjx.MjxError) as e:
                mjx.decode_batch(gpu_ctx, datas[:2], output=mjx.Output("uint8", dst=dst))
            assert e.value.code == mjx.ERR_INVALID_ARG
    finally:
        for sc in scans:
            sc.close()


# ---- GPU: torch ---------------------------------------------------------------------------------------------------------------------------
def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    rng = np.random.RandomState(7)
    sizes = [(750, 595, "420"), (640, 480, "422"), (333, 317, "444"), (512, 512, "gray"), (1920, 1080, "420"), (301, 263, "440")]
    datas = [mjx.synth_jpeg(w, h, sub, 75, seed=60 + k) for k, (w, h, sub) in enumerate(sizes)]
    n = len(datas)
    rois = [(int(rng.randint(0, w - 224 + 1)), int(rng.randint(0, h - 224 + 1)), 224, 224) for (w, h, _) in sizes]
    ref, st = mjx.decode_batch(ctx, datas, rois=rois)
    packed = [ref.rgb(i) for i in range(n)]
    ref.close()
    dev = torch.device("cuda", 0)
    # float16 N x 3 x 224 x 224, ImageNet constants
    out = torch.full((n, 3, 224, 224), float("nan"), dtype=torch.float16, device=dev)
    st = mjx.decode_into(ctx, datas, out, rois=rois, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    torch.cuda.synchronize()
    fmt = mjx.Output("float16", planar=True, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    got = out.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not same_bits(np.ascontiguousarray(got[i]), expected(packed[i], fmt)):
            bad.append(("f16 planar", i, st[i]))
    # uint8 N x H x W x 3, B,G,R, as a view with padded rows of a larger tensor (strides the interleaved form can express)
    big = torch.full((n, 224, 230, 3), 7, dtype=torch.uint8, device=dev)
    view = big[:, :, 3:227, :]
    st = mjx.decode_into(ctx, datas, view, rois=rois, bgr=True)
    torch.cuda.synchronize()
    fmt = mjx.Output("uint8", bgr=True)
    got = big.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not same_bits(np.ascontiguousarray(got[i][:, 3:227, :]), expected(packed[i], fmt)):
            bad.append(("u8 interleaved", i, st[i]))
    if not (np.all(got[:, :, :3, :] == 7) and np.all(got[:, :, 227:, :] == 7)):
        bad.append("the padding of the rows was written")
    # float32 at 1/2 scale, whole pictures of one size
    same = [mjx.synth_jpeg(320, 200, sub, 75, seed=80 + k) for k, sub in enumerate(("420", "444", "gray"))]
    ref, _ = mjx.decode_batch(ctx, same, scale=2)
    out32 = torch.zeros((3, 3, 100, 160), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, same, out32, scale=2, mean=0.5, std=0.25)
    torch.cuda.synchronize()
    fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
    for i in range(3):
        if st[i] != mjx.OK or not same_bits(np.ascontiguousarray(out32[i].cpu().numpy()), expected(ref.rgb(i), fmt)):
            bad.append(("f32 planar scale 2", i, st[i]))
    ref.close()
    # refused before anything is enqueued: unsupported strides, the CPU, a wrong count, a wrong dtype; a wrong size fails its pictures
    refused = 0
    probe = torch.full((n, 3, 224, 224), 3, dtype=torch.uint8, device=dev)
    for t in (probe.permute(0, 1, 3, 2), probe[:, :, :, ::2], torch.zeros((n, 3, 224, 224), dtype=torch.uint8), probe[:2],
              torch.zeros((n, 3, 224, 224), dtype=torch.float64, device=dev), torch.zeros((n, 224, 224, 3), dtype=torch.uint8, device=dev).permute(0, 3, 1, 2),
              probe[:1].expand(n, 3, 224, 224),                                       # every picture the same destination
              torch.zeros((n + 1, 3, 224, 224), dtype=torch.uint8, device=dev).as_strided((n, 3, 224, 224), (224 * 224, 224 * 224, 224, 1)),   # overlapping
              torch.zeros((n, 3, 224, 3), dtype=torch.uint8, device=dev)):             # reads both ways, no keyword
        try:
            mjx.decode_into(ctx, datas, t, rois=rois)
            bad.append(("not refused", tuple(t.shape), tuple(t.stride()), str(t.device)))
        except mjx.MjxError as e:
            refused += e.code == mjx.ERR_INVALID_ARG
    torch.cuda.synchronize()
    if not bool((probe == 3).all()):
        bad.append("a refused call wrote")
    st = mjx.decode_into(ctx, datas, torch.zeros((n, 3, 200, 224), dtype=torch.uint8, device=dev), rois=rois)
    if st != [mjx.ERR_INVALID_ARG] * n:
        bad.append(("wrong height", st))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad), "refused": int(refused)}))


@pytest.mark.gpu
def test_decode_into_a_torch_tensor(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()", timeout=900)
    assert res["nbad"] == 0 and res["refused"] == 9, res


# ---- GPU: a larger batch ---------------------------------------------------------------------------------------------------------------------
def child_larger():
    """64 unique 1080p pictures tiled x 8, planar f16 at 1/2 scale; a seeded sample of 32 pictures compared on the host"""
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, throughput_plan=True)
    datas = mjx.synth_batch(64, 1920, 1080, "420", 75, seed0=300)
    scans = [mjx.ParsedScan(d) for d in datas]
    fmt = mjx.Output("float16", planar=True, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    base, ref = mjx.Batch(ctx, scans, scale=2, output=fmt), mjx.Batch(ctx, scans, scale=2)
    t = base.tile(8)
    ref.decode(); ref.wait()
    t.decode(); t.wait()
    bad = []
    sample = sorted(int(x) for x in np.random.RandomState(11).choice(len(t), 32, replace=False))
    for i in sample:
        if t.status(i) != mjx.OK or not same_bits(t.output(i), expected(ref.rgb(i % 64), fmt)):
            bad.append(i)
    res = {"bad": bad, "nbad": len(bad), "n": len(t), "unconverged": t.unconverged_runs(), "bytes": t.bytes()["rgb"], "sample": len(sample)}
    for x in (t, base, ref):
        x.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(res))


@pytest.mark.gpu
def test_larger_tiled_batch_planar_f16_at_half_scale(mjx, tmp_path):
    res = run_child(tmp_path, "child_larger()", timeout=900)
    assert res["nbad"] == 0 and res["n"] == 512 and res["sample"] == 32 and res["unconverged"] == 0, res
    assert res["bytes"] == 512 * 960 * 540 * 3 * 2, res

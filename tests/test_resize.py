"""Resize on the device (mjx_resize, include/mjx.h): every picture of a call leaves at one target size.

The contract: picture i is decoded as a packed picture at a scale s and a rectangle R -- byte for byte what a plain call with
scale_denom = s, rois[i] = R writes -- and that intermediate is resampled with the separable triangle filter of
torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...), in float32, without rounding between the two
passes; the element written is rint (half to even) of the clamped sample (U8), fmaf(v, scale[c], bias[c]) (F32) or that float rounded
to half (F16).

The reference here is the rule restated in float64 numpy (axis_matrix / resize_ref), pinned against torch on the CPU, applied to the
packed decode of the same build.  The tolerance is derived, not measured: a weight is good to a few float32 roundings (2^-22), a
sample sums Tx + Ty weighted terms of at most 255 (Tx, Ty: the longest tap loops, from mjx_resize_plan), so
tol = 255 (Tx + Ty + 8) 2^-21 per case -- about three times the bound.  F32: |got - (ref scale + bias)| <= tol |scale| + 2^-23 |value|;
F16: 2^-11 |value| on top; U8: rint(ref), and +-1 only where ref lies within tol of k + 0.5 -- over all U8 elements of the sweep at most
2 % may lie in that band (the reference alone: test_band_share_of_the_reference_alone).

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
import test_output_formats as of
import test_roi_decode as roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_CAP = 0.02
F32_PLANAR = 10                                   # of.FORMATS[10] = ("float32", True, False)
assert of.FORMATS[F32_PLANAR] == ("float32", True, False)


def _read(p):
    with open(p, "rb") as f:
        return f.read()


# ---- the rule, in float64 -----------------------------------------------------------------------------------------------------------
def axis_matrix(n_in, n_out, antialias):
    """[n_out, n_in] float64: row X holds the normalised weights of output coordinate X."""
    r = n_in / n_out
    fs = max(1.0, r) if antialias else 1.0
    m = np.zeros((n_out, n_in), np.float64)
    for X in range(n_out):
        c = (X + 0.5) * r
        lo, hi = max(0, int(np.floor(c - fs + 0.5))), min(n_in, int(np.floor(c + fs + 0.5)))
        j = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs(j + 0.5 - c) / fs)
        m[X, lo:hi] = w / w.sum()
    return m


def resize_ref(img, width, height, antialias):
    """img [h, w, C] (any dtype) -> float64 [height, width, C]: v = sum_y sum_x wy wx I[y][x][ch]"""
    a = np.asarray(img, np.float64)
    my, mx = axis_matrix(a.shape[0], height, antialias), axis_matrix(a.shape[1], width, antialias)
    return np.einsum("yi,ijc,xj->yxc", my, a, mx)


def tolerance(tx, ty):
    return 255.0 * (tx + ty + 8) * 2.0 ** -21


def check_against(got, ref, fmt, tol):
    """got: the library's array in the format's shape and dtype; ref: float64 [H, W, 3] in R,G,B.
    -> (failure text or None, U8 elements in the band, U8 elements)"""
    src = ref[:, :, ::-1] if fmt.bgr else ref
    want = np.ascontiguousarray(np.transpose(src, (2, 0, 1)) if fmt.planar else src)
    if got.shape != want.shape or got.dtype != fmt.numpy_dtype():
        return "shape %s dtype %s, expected %s %s" % (got.shape, got.dtype, want.shape, fmt.numpy_dtype()), 0, 0
    if fmt.numpy_dtype() == np.uint8:
        lo, hi = np.rint(np.clip(want - tol, 0, 255)), np.rint(np.clip(want + tol, 0, 255))
        band = int((lo != hi).sum())
        g = got.astype(np.float64)
        nbad = int(((g < lo) | (g > hi)).sum())
        return (None if nbad == 0 else "%d u8 elements are not rint(ref) (band of %d)" % (nbad, band)), band, got.size
    sc = np.asarray(fmt.scale, np.float64).reshape((3, 1, 1) if fmt.planar else (1, 1, 3))
    bi = np.asarray(fmt.bias, np.float64).reshape(sc.shape)
    value = want * sc + bi
    bound = tol * np.abs(sc) + 2.0 ** -23 * np.abs(value)
    if fmt.numpy_dtype() == np.float16:
        bound = bound + 2.0 ** -11 * np.abs(value)
    err = np.abs(got.astype(np.float64) - value)
    if not np.all(np.isfinite(got.astype(np.float64))) or np.any(err > bound):
        k = int(np.argmax(err - bound))
        return "error %.3g over a bound of %.3g" % (err.reshape(-1)[k], bound.reshape(-1)[k]), 0, 0
    return None, 0, 0


# ---- CPU 1: the rule is torch's ----------------------------------------------------------------------------------------------------------
def test_the_rule_equals_torch_interpolate_in_float64():
    import torch
    import torch.nn.functional as F
    rng = np.random.RandomState(5)
    worst = 0.0
    for (h, w), (oh, ow) in [((37, 53), (16, 24)), ((45, 61), (16, 24)), ((9, 7), (16, 24)), ((131, 200), (16, 24)), ((16, 24), (16, 24)),
                             ((1, 1), (5, 3)), ((100, 3), (7, 9))]:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1))))[None]
        for aa in (False, True):
            want = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False, antialias=aa)[0].numpy()
            got = np.transpose(resize_ref(img, ow, oh, aa), (2, 0, 1))
            worst = max(worst, float(np.abs(got - want).max()))
    print("largest difference between the numpy rule and torch (float64):", worst)
    assert worst <= 1e-9


# ---- CPU 2: the kernel's weights ---------------------------------------------------------------------------------------------------------
def _dense_weights(mjx, n_in, n_out, aa, xs=None):
    lib = mjx.lib()
    first, cnt = ctypes.c_uint32(), ctypes.c_size_t()
    buf = np.zeros(2 * n_in + 8, np.float32)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    xs = range(n_out) if xs is None else xs
    m = np.zeros((len(xs), n_in), np.float64)
    for r, X in enumerate(xs):
        assert lib.mjx_resize_weights(n_in, n_out, int(aa), X, ctypes.byref(first), ptr, buf.size, ctypes.byref(cnt)) == mjx.OK
        assert cnt.value >= 1 and first.value + cnt.value <= n_in, (n_in, n_out, aa, X, first.value, cnt.value)
        m[r, first.value:first.value + cnt.value] = buf[:cnt.value]
    return m


def test_weights_of_the_kernels_routine_against_float64(mjx):
    worst, worst_sum, n = 0.0, 0.0, 0
    for aa in (False, True):
        for n_out in (1, 7, 16, 24, 224):
            for n_in in range(1, 301):
                got = _dense_weights(mjx, n_in, n_out, aa)
                d = float(np.abs(got - axis_matrix(n_in, n_out, aa)).max())
                s = float(np.abs(got.sum(axis=1) - 1.0).max())
                assert d <= 2.0 ** -20 and s <= 2.0 ** -20, (n_in, n_out, aa, d, s)
                worst, worst_sum, n = max(worst, d), max(worst_sum, s), n + 1
    assert n == 3000
    # coordinates near 4000: (X + 0.5) r in float32 would be 2e-4 pixels off, a weight 2e-4 / fs = 1e-5
    for aa in (False, True):
        got = _dense_weights(mjx, 3840, 224, aa, xs=[223])
        want = axis_matrix(3840, 224, aa)[223:224]
        d = float(np.abs(got - want).max())
        assert d <= 2.0 ** -20 and abs(float(got.sum()) - 1.0) <= 2.0 ** -20, (aa, d)
        worst = max(worst, d)
    print("largest weight difference %.3g, largest |row sum - 1| %.3g" % (worst, worst_sum))
    lib = mjx.lib()
    for bad in ((0, 4, 0), (4, 0, 0), (4, 4, 4), ((1 << 24) + 1, 4, 0)):
        assert lib.mjx_resize_weights(bad[0], bad[1], 1, bad[2], None, None, 0, None) == mjx.ERR_INVALID_ARG


# ---- CPU 3: the plan -----------------------------------------------------------------------------------------------------------------------
def auto_scale_rule(W, H, rect, tw, th):
    """restated: the largest s of 1, 2, 4, 8 whose outward-rounded rectangle is at least the target; s = 1 if none"""
    x, y, w, h = (0, 0, W, H) if rect is None else rect
    for s in (8, 4, 2, 1):
        rs = (x // s, y // s, -(-(x + w) // s) - x // s, -(-(y + h) // s) - y // s)
        if s == 1 or (rs[2] >= tw and rs[3] >= th):
            return s, rs


def max_taps(n_in, n_out, aa):
    return int((axis_matrix(n_in, n_out, aa) > 0).sum(axis=1).max())


def test_resize_plan_is_the_auto_scale_rule(mjx):
    rng = np.random.RandomState(17)
    n, scales = 0, set()
    for (W, H, sub) in ((1001, 37, "420"), (61, 45, "gray"), (333, 217, "422"), (640, 480, "444"), (1920, 1080, "420")):
        scan = mjx.ParsedScan(mjx.synth_jpeg(W, H, sub, 75, seed=3))
        try:
            for _ in range(40):
                rect = None
                if rng.randint(4):
                    w, h = int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))
                    rect = (int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1)), w, h)
                tw, th = int(rng.choice([1, 7, 24, 70, 224, 300])), int(rng.choice([1, 7, 16, 37, 224, 300]))
                aa = bool(rng.randint(2))
                got = scan.resize_plan(mjx.Resize(tw, th, antialias=aa, auto_scale=True), roi=rect)
                s, rs = auto_scale_rule(W, H, rect, tw, th)
                assert (got["scale"], got["rect"]) == (s, rs), (W, H, rect, tw, th, got)
                # the rectangle covers the full-size one and is rounded outward by less than s pixels per side
                x, y, w, h = (0, 0, W, H) if rect is None else rect
                assert rs[0] * s <= x < (rs[0] + 1) * s and rs[1] * s <= y < (rs[1] + 1) * s
                assert (rs[0] + rs[2] - 1) * s < x + w <= (rs[0] + rs[2]) * s and (rs[1] + rs[3] - 1) * s < y + h <= (rs[1] + rs[3]) * s
                # the tap counts are the windows' of the routine: never fewer than the float64 rule's positive weights, at most two more
                tx, ty = max_taps(rs[2], tw, aa), max_taps(rs[3], th, aa)
                assert tx <= got["taps_x"] <= tx + 2 and ty <= got["taps_y"] <= ty + 2, (W, H, rect, tw, th, aa, got, tx, ty)
                scales.add(s)
                n += 1
            # auto_scale = 0: the call's own scale and rectangle
            for s in (1, 2, 4, 8):
                ow, oh = -(-W // s), -(-H // s)
                r = (ow // 3, oh // 4, max(1, ow // 2), max(1, oh // 3))
                got = scan.resize_plan(mjx.Resize(24, 16, auto_scale=False), roi=r, scale=s)
                assert (got["scale"], got["rect"]) == (s, r)
                got = scan.resize_plan(mjx.Resize(24, 16, auto_scale=False), scale=s)
                assert (got["scale"], got["rect"]) == (s, (0, 0, ow, oh))
        finally:
            scan.close()
    assert n == 200 and scales == {1, 2, 4, 8}


def test_resize_argument_rules(mjx):
    scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))

    def code(rs, **kw):
        try:
            scan.resize_plan(rs, **kw)
            return mjx.OK
        except mjx.MjxError as e:
            return e.code
    try:
        assert code(mjx.Resize(24, 16)) == mjx.OK and code(mjx.Resize(24, 16, auto_scale=False), scale=4) == mjx.OK
        assert code(mjx.Resize(0, 16)) == mjx.ERR_INVALID_ARG and code(mjx.Resize(24, 0)) == mjx.ERR_INVALID_ARG
        assert code(mjx.Resize(0, 16, auto_scale=False)) == mjx.ERR_INVALID_ARG
        assert code(mjx.Resize(24, 16), layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        assert code(mjx.Resize(24, 16, auto_scale=False), layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        assert code(mjx.Resize(24, 16), scale=2) == mjx.ERR_INVALID_ARG                        # auto_scale with a scale of the call's
        assert code(mjx.Resize(24, 16), scale=0) == mjx.OK
        assert code(mjx.Resize(24, 16), roi=(60, 0, 8, 8)) == mjx.ERR_INVALID_ARG              # the rectangle rules, full-size coordinates
        assert code(mjx.Resize(24, 16), roi=(56, 40, 8, 8)) == mjx.OK
        assert code(mjx.Resize(24, 16), roi=(0, 0, 8, 0)) == mjx.ERR_INVALID_ARG
        assert code(mjx.Resize(24, 16, auto_scale=False), roi=(28, 20, 8, 8), scale=2) == mjx.ERR_INVALID_ARG     # (the scaled picture is 32 x 24)
        assert code(mjx.Resize(24, 16, auto_scale=False), roi=(24, 16, 8, 8), scale=2) == mjx.OK
        assert code(mjx.Resize(5000, 3000)) == mjx.OK                                          # no limit on the ratio: upscaling
    finally:
        scan.close()


# ---- CPU 4: mirrors ----------------------------------------------------------------------------------------------------------------------------
def test_mirrors_of_the_resize_struct_and_entry_points(mjx):
    hdr = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    body = re.search(r"typedef struct mjx_resize\s*\{(.*?)\}\s*mjx_resize;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\**", "", decl)
            fields += [re.sub(r"[\[\]0-9\s\*]", "", x) for x in names.split(",")]
    want = ["width", "height", "antialias", "auto_scale"]
    assert fields == want and [f[0] for f in mjx.ResizeDesc._fields_] == want
    rbody = re.search(r"pub struct mjx_resize\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+): ([^,\n]+),", rbody) == list(zip(want, ["u32", "u32", "u8", "u8"]))
    assert re.search(r"#\[repr\(C\)\]\s*(#\[[^\]]*\]\s*)*pub struct mjx_resize", rs)
    assert ctypes.sizeof(mjx.ResizeDesc) == 12 and mjx.ResizeDesc.antialias.offset == 8 and mjx.ResizeDesc.auto_scale.offset == 9
    for fn, n in (("mjx_batch_create_resize", 8), ("mjx_decode_batch_resize", 10), ("mjx_resize_plan", 8), ("mjx_resize_weights", 8),
                  ("mjx_batch_image_scale", 3), ("mjx_batch_resize_rect", 3)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)
        assert fn in mjx.SYMBOLS and len(mjx.SYMBOLS[fn][1]) == n, fn
    assert re.search(r"MJX_K_RESIZE = 10,", hdr) and re.search(r"MJX_K_COUNT = 11", hdr)
    assert mjx.KERNEL_NAMES[10] == "resize" and len(mjx.KERNEL_NAMES) == 11
    # mjx_opts and mjx_output are as they were
    assert ctypes.sizeof(mjx.OutputDesc) == 48 and [f[0] for f in mjx.Opts._fields_][-3:] == ["scale_denom", "rois", "n_rois"]


def test_decode_batch_resize_without_a_device_is_a_device_error(tmp_path):
    """No fallback: with the devices hidden mjx_ctx_create fails, and mjx_decode_batch_resize on what it leaves says MJX_ERR_DEVICE."""
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
        "    mjx.decode_batch(c, [data], resize=mjx.Resize(24, 16))\n"
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


# ---- the sweep's cases (CPU 5 and GPU 1 walk the same list) --------------------------------------------------------------------------------
TARGETS = ((24, 16), (70, 37))
UPSCALE = ((40, 24), (19, 13))                     # target, the rectangle's size
MODES = ((False, 1), (False, 2), (True, 1))        # (auto_scale, the call's scale)


def sweep_inputs(mjx):
    pil = os.path.join(ROOT, "tests", "golden", "pil")
    return [("lena", _read(os.path.join(ROOT, "tests", "data", "lena.jpeg"))),
            ("synth_160x96_420", mjx.synth_jpeg(160, 96, "420")), ("synth_75x50_444", mjx.synth_jpeg(75, 50, "444")),
            ("synth_61x45_gray", mjx.synth_jpeg(61, 45, "gray")),
            ("ms_420_odd", _read(os.path.join(pil, "ms_420_odd.jpg"))), ("dri_420_r5", _read(os.path.join(pil, "dri_420_r5.jpg")))]


def _seeded_rect(rng, W, H, min_w, min_h):
    w, h = int(rng.randint(min(min_w, W), W + 1)), int(rng.randint(min(min_h, H), H + 1))
    return (int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1)), w, h)


def u8_eligible(rect_wh, target, aa):
    """The U8 sweep keeps away from integer and near-integer ratios (they put elements exactly on halves): neither axis ratio has a
    lowest-terms denominator below 5, and at most 30 taps per axis."""
    for n_in, n_out in zip(rect_wh, target):
        if Fraction(n_in, n_out).denominator < 5 or max_taps(n_in, n_out, aa) > 30:
            return False
    return True


def sweep_cases(mjx, inputs, scans):
    """-> list of dict(k, auto, scale, aa, target, roi, s, R, taps, fmt): every input x mode x antialias x (two targets x (whole picture, two
    seeded rectangles) + the upscale from a 19 x 13 rectangle).  roi is what the call is given (full-size coordinates with auto_scale,
    the scaled picture's otherwise); s, R and taps come from mjx_resize_plan.  fmt: one of the eleven formats other than planar F32, in
    rotation -- a U8 format only where the case is u8_eligible (the next float format otherwise)."""
    cases, rot = [], 0
    others = [f for f in range(12) if f != F32_PLANAR]
    for k, (name, data) in enumerate(inputs):
        W, H = roi.frame_of(data)[:2]
        for auto, scale in MODES:
            pw, ph = (W, H) if auto else (-(-W // scale), -(-H // scale))
            rng = np.random.RandomState(100 * k + 10 * scale + int(auto))
            rects = [None, _seeded_rect(rng, pw, ph, 9, 9), _seeded_rect(rng, pw, ph, 9, 9)]
            up = (int(rng.randint(0, pw - UPSCALE[1][0] + 1)), int(rng.randint(0, ph - UPSCALE[1][1] + 1))) + UPSCALE[1]
            for aa in (False, True):
                for target, r in [(t, r) for t in TARGETS for r in rects] + [(UPSCALE[0], up)]:
                    plan = scans[k].resize_plan(mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto), roi=r, scale=scale)
                    f = others[rot % 11]
                    while of.FORMATS[f][0] == "uint8" and not u8_eligible(plan["rect"][2:], target, aa):
                        rot += 1
                        f = others[rot % 11]
                    rot += 1
                    cases.append(dict(k=k, auto=auto, scale=scale, aa=aa, target=target, roi=r, s=plan["scale"], R=plan["rect"],
                                      taps=(plan["taps_x"], plan["taps_y"]), fmt=f))
    return cases


def test_band_share_of_the_reference_alone(mjx, orc):
    """The U8 exception (+-1 within tol of a half) must not hide a failure: on the oracle's pictures of the sweep's U8 cases the share of
    elements in the band stays under the cap."""
    inputs = sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        cases = sweep_cases(mjx, inputs, scans)
    finally:
        for s in scans:
            s.close()
    assert len(cases) == 6 * 3 * 2 * 7
    assert set(c["s"] for c in cases if c["auto"]) == {1, 2, 4, 8}
    decs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True) for _, d in inputs]
    fulls = {}
    band = total = 0
    for c in cases:
        if of.FORMATS[c["fmt"]][0] != "uint8":
            continue
        key = (c["k"], c["s"])
        if key not in fulls:
            fulls[key] = decs[c["k"]].rgb if c["s"] == 1 else scaled_ref.scaled_rgb(inputs[c["k"]][1], c["s"], decs[c["k"]])
        ref = resize_ref(roi.crop(fulls[key], c["R"]), c["target"][0], c["target"][1], c["aa"])
        tol = tolerance(*c["taps"])
        band += int((np.rint(np.clip(ref - tol, 0, 255)) != np.rint(np.clip(ref + tol, 0, 255))).sum())
        total += ref.size
    print("U8 elements of the sweep: %d, in the band: %d (%.3f %%)" % (total, band, 100.0 * band / max(total, 1)))
    assert total > 20000 and band <= BAND_CAP * total


# ---- GPU: the child's library -------------------------------------------------------------------------------------------------------------
def _packed(mjx, ctx, scans, wanted):
    """wanted: set of (k, s, R) -> dict of the plain packed decodes, one batch per scale"""
    out = {}
    for s in sorted(set(w[1] for w in wanted)):
        keys = sorted(w for w in wanted if w[1] == s)
        b = mjx.Batch(ctx, [scans[k] for k, _, _ in keys], scale=s, rois=[R for _, _, R in keys])
        b.decode(); b.wait()
        for i, key in enumerate(keys):
            assert b.status(i) == mjx.OK, key
            out[key] = b.rgb(i)
        b.close()
    return out


def child_sweep():
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, profiling=True)
    inputs = sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    cases = sweep_cases(mjx, inputs, scans)
    packed = _packed(mjx, ctx, scans, set((c["k"], c["s"], c["R"]) for c in cases))
    bad, band, total, worst, launches = [], 0, 0, 0.0, 0
    groups = {}
    for c in cases:
        for f in (F32_PLANAR, c["fmt"]):
            groups.setdefault((c["auto"], c["scale"], c["aa"], c["target"], f), []).append(c)
    for (auto, scale, aa, target, f), cs in sorted(groups.items(), key=lambda g: g[0]):
        fmt = of.make_format(mjx, f)
        b = mjx.Batch(ctx, [scans[c["k"]] for c in cs], scale=scale, rois=[c["roi"] for c in cs], output=fmt,
                      resize=mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto))
        b.decode(); b.wait()
        launches += b.kernel_ms()["resize"][1]
        for i, c in enumerate(cs):
            what = (inputs[c["k"]][0], auto, scale, aa, target, c["roi"], of.FORMATS[f])
            if b.status(i) != mjx.OK:
                bad.append(what + ("status", b.status(i))); continue
            inf, r = b.info(i), b.roi(i)
            if (b.scale(i), b.rect(i)) != (c["s"], c["R"]) or (inf["width"], inf["height"]) != target or (r["x"], r["y"]) != c["R"][:2]:
                bad.append(what + ("scale / rectangle / size", b.scale(i), b.rect(i), inf)); continue
            ref = resize_ref(packed[(c["k"], c["s"], c["R"])], target[0], target[1], aa)
            fail, nb, nt = check_against(b.output(i), ref, fmt, tolerance(*c["taps"]))
            band, total = band + nb, total + nt
            if fail:
                bad.append(what + (fail,))
        b.close()
    # a batch without a resize never launches the kernel
    plain = mjx.Batch(ctx, scans[:2], output=of.make_format(mjx, 3))
    plain.decode(); plain.wait()
    idle = plain.kernel_ms()["resize"][1]
    plain.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps({"bad": bad[:30], "nbad": len(bad), "cases": len(cases), "batches": len(groups), "band": band, "u8": total,
                      "auto_scales": sorted(set(c["s"] for c in cases if c["auto"])), "launches": int(launches), "idle_launches": int(idle)}))


def run_child(tmp_path, call, env_set=None, timeout=900):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_resize as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
def test_sweep_every_case_is_the_rule_applied_to_the_packed_decode(mjx, tmp_path, single_decode):
    res = run_child(tmp_path, "child_sweep()", {} if single_decode is None else {"MJX_SINGLE_DECODE": single_decode})
    assert res["nbad"] == 0, res
    assert res["cases"] == 6 * 3 * 2 * 7 and res["auto_scales"] == [1, 2, 4, 8], res
    assert res["u8"] > 20000 and res["band"] <= BAND_CAP * res["u8"], res
    assert res["launches"] >= res["batches"] and res["idle_launches"] == 0, res


# ---- GPU 2: exactness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_target_of_the_rectangles_size_is_the_format_table_bit_for_bit(mjx, gpu_ctx):
    inputs = sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        w, h = 37, 29
        rois = []
        for i, (_, d) in enumerate(inputs):
            W, H = roi.frame_of(d)[:2]
            rois.append((min(3 + 5 * i, W - w), min(2 + 3 * i, H - h), w, h))
        ref = mjx.Batch(gpu_ctx, scans, rois=rois)
        ref.decode(); ref.wait()
        packed = [ref.rgb(i) for i in range(len(scans))]
        ref.close()
        for f in range(12):
            fmt = of.make_format(mjx, f)
            for auto in (False, True):
                b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, resize=mjx.Resize(w, h, antialias=bool(f & 1), auto_scale=auto))
                try:
                    b.decode(); b.wait()
                    for i in range(len(scans)):
                        assert b.status(i) == mjx.OK and b.scale(i) == 1 and b.rect(i) == rois[i]
                        assert of.same_bits(b.output(i), of.expected(packed[i], fmt)), (of.FORMATS[f], auto, inputs[i][0])
                finally:
                    b.close()
    finally:
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_halving_with_antialias_rounds_half_to_even_exactly(mjx, gpu_ctx):
    """48 x 32 -> 24 x 16 with antialias: the weights are 1, 3, 3, 1 of 8 (at the edges 3, 3, 1 of 7), so a float32 sample is the exact
    quotient rounded once and U8 is rint half-even of the reference, with no band."""
    inputs = sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        rois = []
        for i, (_, d) in enumerate(inputs):
            W, H = roi.frame_of(d)[:2]
            rois.append((min(5 + 7 * i, W - 48), min(1 + 2 * i, H - 32), 48, 32))
        ref = mjx.Batch(gpu_ctx, scans, rois=rois)
        ref.decode(); ref.wait()
        packed = [ref.rgb(i) for i in range(len(scans))]
        ref.close()
        halves = 0
        for f in (0, 3):                                            # u8 interleaved R,G,B; u8 planar B,G,R
            fmt = of.make_format(mjx, f)
            b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, resize=mjx.Resize(24, 16, antialias=True, auto_scale=False))
            try:
                b.decode(); b.wait()
                for i in range(len(scans)):
                    # the reference in exact arithmetic: numerators 1, 3, 3, 1 (clipped at the edges), integer sums, one division
                    a = packed[i].astype(np.int64)
                    def num(n_in, n_out):
                        m = np.zeros((n_out, n_in), np.int64)
                        for X in range(n_out):
                            for j, v in zip(range(2 * X - 1, 2 * X + 3), (1, 3, 3, 1)):
                                if 0 <= j < n_in:
                                    m[X, j] = v
                        return m
                    my, mx = num(32, 16), num(48, 24)
                    acc = np.einsum("yi,ijc,xj->yxc", my, a, mx)
                    den = my.sum(axis=1)[:, None, None] * mx.sum(axis=1)[None, :, None]
                    exact = acc / den                                # float64 of an exact quotient of integers below 2^24
                    assert float(np.abs(exact - resize_ref(packed[i], 24, 16, True)).max()) < 1e-9
                    halves += int((2 * acc % den == 0).sum() - (acc % den == 0).sum())
                    want = np.rint(exact).astype(np.uint8)
                    src = want[:, :, ::-1] if fmt.bgr else want
                    want = np.ascontiguousarray(np.transpose(src, (2, 0, 1)) if fmt.planar else src)
                    assert of.same_bits(b.output(i), want), (of.FORMATS[f], inputs[i][0])
            finally:
                b.close()
        print("elements exactly on a half:", halves)
        assert halves > 0                                           # (the rounding mode was exercised)
    finally:
        for s in scans:
            s.close()


# ---- GPU 3: a large ratio ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_ratios_many_slabs(mjx, gpu_ctx):
    data = _read(os.path.join(ROOT, "tests", "data", "lena.jpeg"))
    scan = mjx.ParsedScan(data)
    try:
        ref = mjx.Batch(gpu_ctx, [scan])
        ref.decode(); ref.wait()
        packed = ref.rgb(0)
        ref.close()
        fmt = of.make_format(mjx, F32_PLANAR)
        for target in ((9, 7), (1, 1)):
            plan = scan.resize_plan(mjx.Resize(target[0], target[1], auto_scale=False))
            assert plan["taps_x"] > 100 and plan["taps_y"] > 100
            b = mjx.Batch(gpu_ctx, [scan], output=fmt, resize=mjx.Resize(target[0], target[1], antialias=True, auto_scale=False))
            try:
                b.decode(); b.wait()
                assert b.status(0) == mjx.OK and b.scale(0) == 1
                fail, _, _ = check_against(b.output(0), resize_ref(packed, target[0], target[1], True), fmt, tolerance(plan["taps_x"], plan["taps_y"]))
                assert fail is None, (target, fail)
            finally:
                b.close()
    finally:
        scan.close()


# ---- GPU 4: caller-owned memory ------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_images", [0, 2])
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("fmt_k", [6, 0], ids=["f16_planar", "u8_interleaved"])
def test_caller_owned_memory_and_nothing_written_outside(mjx, gpu_ctx, fmt_k, pitched, chunk_images):
    """One hipMalloc holds N x 3 x 16 x 24 (or N x 16 x 24 x 3) for pictures of different sizes and samplings; guards in front and
    behind, everything sentinel-filled; a file that does not decode keeps its slot untouched and the others decode."""
    inputs = sweep_inputs(mjx)
    datas = [d for _, d in inputs]
    undecodable = 3
    datas.insert(undecodable, _read(os.path.join(ROOT, "tests", "golden", "pil", "progressive.jpg")))
    n = len(datas)
    w, h = 24, 16
    fmt0 = of.make_format(mjx, fmt_k)
    esz = np.dtype(fmt0.numpy_dtype()).itemsize
    planar = fmt0.planar
    rp = (w if planar else 3 * w) + (5 if pitched else 0)
    pp = (h * rp + (11 if pitched else 0)) if planar else 0
    per = (3 * pp if planar else h * rp) + (13 if pitched else 0)
    guard = 4096
    total = guard + n * per * esz + guard
    hip = of._hip(mjx)
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [(base.value + guard + i * per * esz, w, h, rp, pp) for i in range(n)]
        fmt = of.make_format(mjx, fmt_k, dst=dst)
        good = [i for i in range(n) if i != undecodable]
        rs = mjx.Resize(w, h, antialias=True, auto_scale=True)
        b, st = mjx.decode_batch(gpu_ctx, datas, chunk_images=chunk_images, output=fmt, resize=rs)
        try:
            assert st[undecodable] == mjx.ERR_UNSUPPORTED_FORMAT and [st[i] for i in good] == [mjx.OK] * len(good), st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            covered = np.zeros(total, bool)
            band = u8 = 0
            for i in good:
                s, R = b.scale(i), b.rect(i)
                scan = mjx.ParsedScan(datas[i])
                plan = scan.resize_plan(rs)
                scan.close()
                assert (plan["scale"], plan["rect"]) == (s, R)
                ref = resize_ref(roi.crop(roi._full(mjx, gpu_ctx, datas[i], s), R), w, h, True)
                slot = mem[guard + i * per * esz: guard + (i + 1) * per * esz].view(fmt.numpy_dtype())
                if planar:
                    el = (np.arange(3)[:, None, None] * pp + np.arange(h)[None, :, None] * rp + np.arange(w)[None, None, :])
                else:
                    el = (np.arange(h)[:, None, None] * rp + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :])
                fail, nb, nt = check_against(np.ascontiguousarray(slot[el]), ref, fmt, tolerance(plan["taps_x"], plan["taps_y"]))
                assert fail is None, ("picture", i, fail)
                band, u8 = band + nb, u8 + nt
                bytes_at = (guard + i * per * esz + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)
                covered[bytes_at] = True
                inf = b.output_info(i)
                assert (inf["dev"], inf["width"], inf["height"], inf["row_pitch"], inf["plane_pitch"]) == dst[i], (i, inf)
                with pytest.raises(mjx.MjxError):
                    b.output(i)                                      # mjx_batch_copy_output serves library-owned output only
            assert np.all(mem[~covered] == SENTINEL), ("bytes outside the pictures' elements were written", np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist())
            assert b.bytes()["rgb"] == len(good) * w * h * 3 * esz
            if chunk_images:
                assert b.geometry()["chunks"] >= 3
        finally:
            b.close()
        # a destination that is not the target's size fails its picture; tile refuses caller-owned destinations
        scans = [mjx.ParsedScan(datas[i]) for i in good[:2]]
        try:
            wrong = mjx.Batch(gpu_ctx, scans, output=of.make_format(mjx, fmt_k, dst=[dst[0], (dst[1][0], w + 1, h, rp + 3, pp)]), resize=rs)
            assert wrong.create_status == [mjx.OK, mjx.ERR_INVALID_ARG]
            wrong.close()
            two = mjx.Batch(gpu_ctx, scans, output=of.make_format(mjx, fmt_k, dst=dst[:2]), resize=rs)
            assert two.create_status == [mjx.OK, mjx.OK]
            with pytest.raises(mjx.MjxError) as e:
                two.tile(2)
            assert e.value.code == mjx.ERR_INVALID_ARG
            two.close()
        finally:
            for s in scans:
                s.close()
    finally:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipFree(base) == 0


# ---- GPU 5: front doors, torch, a tiled batch ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_front_door_from_file_bytes_with_per_file_rectangles(mjx, gpu_ctx):
    inputs = sweep_inputs(mjx)
    datas = [d for _, d in inputs]
    n = len(datas)
    rois = []
    for i, d in enumerate(datas):
        W, H = roi.frame_of(d)[:2]
        rois.append(None if i == 1 else (W // 7, H // 5, W - W // 3, H - H // 4))
    target = (31, 19)
    for auto in (True, False):
        for f in (None, 6, 1):                                       # out == NULL: interleaved u8 R,G,B
            rs = mjx.Resize(target[0], target[1], antialias=True, auto_scale=auto)
            fmt = None if f is None else of.make_format(mjx, f)
            for dd in (True, False):
                b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd, rois=rois, output=fmt, resize=rs)
                try:
                    assert st == [mjx.OK] * n
                    for i in range(n):
                        s, R = b.scale(i), b.rect(i)
                        scan = mjx.ParsedScan(datas[i])
                        plan = scan.resize_plan(rs, roi=rois[i])
                        scan.close()
                        assert (plan["scale"], plan["rect"]) == (s, R) and (auto or s == 1)
                        ref = resize_ref(roi.crop(roi._full(mjx, gpu_ctx, datas[i], s), R), target[0], target[1], True)
                        fail, _, _ = check_against(b.output(i), ref, fmt or mjx.Output(), tolerance(plan["taps_x"], plan["taps_y"]))
                        assert fail is None, (auto, f, dd, i, fail)
                        inf = b.output_info(i)
                        assert (inf["width"], inf["height"]) == target
                        with pytest.raises(mjx.MjxError) as e:
                            b.rgb(i)                                  # copy_rgb: as for any batch with a description
                        assert e.value.code == mjx.ERR_INVALID_ARG
                    mx, _ = b.compare_rgb(list(range(n)), b, list(range(n)))
                    assert [int(v) for v in mx] == [0xffffffff] * n
                    assert b.bytes()["rgb"] == n * target[0] * target[1] * 3 * (1 if fmt is None else of.ESZ[of.FORMATS[f][0]])
                finally:
                    b.close()
    # per picture: a zero target, auto_scale with a scale; the call goes through and says so for every picture
    for rs, kw in ((mjx.Resize(0, 16), {}), (mjx.Resize(24, 16), {"scale": 2})):
        b, st = mjx.decode_batch(gpu_ctx, datas[:2], resize=rs, **kw)
        assert st == [mjx.ERR_INVALID_ARG] * 2
        b.close()


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import torch.nn.functional as F
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    sizes = [(750, 595, "420"), (640, 480, "422"), (333, 317, "444"), (512, 512, "gray"), (301, 263, "440")]          # five different sizes
    datas = [mjx.synth_jpeg(w, h, sub, 75, seed=60 + k) for k, (w, h, sub) in enumerate(sizes)]
    n = len(datas)
    rng = np.random.RandomState(9)
    rois = []
    for (w, h, _) in sizes:
        cw, ch = int(rng.randint(w // 2, w + 1)), int(rng.randint(h // 2, h + 1))
        rois.append((int(rng.randint(0, w - cw + 1)), int(rng.randint(0, h - ch + 1)), cw, ch))
    dev = torch.device("cuda", 0)
    H, W = 96, 112
    for aa in (True, False):
        rs = mjx.Resize(0, 0, antialias=aa, auto_scale=True)
        out = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=dev)
        st = mjx.decode_into(ctx, datas, out, rois=rois, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, resize=True if aa else rs)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
        for i in range(n):
            if st[i] != mjx.OK:
                bad.append(("status", aa, i, st[i])); continue
            scan = mjx.ParsedScan(datas[i])
            plan = scan.resize_plan(mjx.Resize(W, H, antialias=aa), roi=rois[i])
            scan.close()
            ref, _ = mjx.decode_batch(ctx, [datas[i]], scale=plan["scale"], rois=[plan["rect"]])
            packed = ref.rgb(0)
            ref.close()
            t = torch.from_numpy(np.ascontiguousarray(np.transpose(packed, (2, 0, 1))).astype(np.float64))[None]
            want = F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False, antialias=aa)[0].numpy()        # torch on the CPU, double
            fail, _, _ = check_against(np.ascontiguousarray(got[i]), np.transpose(want, (1, 2, 0)), fmt, tolerance(plan["taps_x"], plan["taps_y"]))
            if fail:
                bad.append((aa, i, fail))
    # uint8 N x H x W x 3 as a view with padded rows of a larger tensor
    big = torch.full((n, H, W + 6, 3), 7, dtype=torch.uint8, device=dev)
    st = mjx.decode_into(ctx, datas, big[:, :, 3:W + 3, :], rois=rois, resize=True)
    torch.cuda.synchronize()
    g8 = big.cpu().numpy()
    if st != [mjx.OK] * n or not (np.all(g8[:, :, :3, :] == 7) and np.all(g8[:, :, W + 3:, :] == 7)) or np.all(g8[:, :, 3:W + 3, :] == 7):
        bad.append(("u8 view", st))
    # a Resize that names another size than the tensor's is refused; without resize= pictures of other sizes fail as before
    refused = 0
    try:
        mjx.decode_into(ctx, datas, torch.zeros((n, 3, H, W), dtype=torch.uint8, device=dev), resize=mjx.Resize(W + 1, H))
    except mjx.MjxError as e:
        refused += e.code == mjx.ERR_INVALID_ARG
    st = mjx.decode_into(ctx, datas, torch.zeros((n, 3, H, W), dtype=torch.uint8, device=dev), rois=rois)
    if st != [mjx.ERR_INVALID_ARG] * n:
        bad.append(("without resize", st))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad), "refused": int(refused)}))


@pytest.mark.gpu
def test_decode_into_one_tensor_from_files_of_five_sizes(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()", timeout=900)
    assert res["nbad"] == 0 and res["refused"] == 1, res


def child_tiled():
    """16 unique 320 x 240 pictures tiled x 8, target 64 x 64, several chunks; a seeded sample of 32 pictures compared on the host"""
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, throughput_plan=True, profiling=True)
    datas = mjx.synth_batch(16, 320, 240, "420", 75, seed0=500)
    scans = [mjx.ParsedScan(d) for d in datas]
    fmt = mjx.Output("float16", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    rs = mjx.Resize(64, 64, antialias=True, auto_scale=True)
    base = mjx.Batch(ctx, scans, output=fmt, resize=rs, chunk_images=24)
    plan = scans[0].resize_plan(rs)
    ref = mjx.Batch(ctx, scans, scale=plan["scale"])
    t = base.tile(8)
    ref.decode(); ref.wait()
    t.decode(); t.wait()
    bad = []
    sample = sorted(int(x) for x in np.random.RandomState(11).choice(len(t), 32, replace=False))
    for i in sample:
        if t.status(i) != mjx.OK or t.scale(i) != plan["scale"] or t.rect(i) != plan["rect"]:
            bad.append((i, "status / scale / rectangle")); continue
        fail, _, _ = check_against(t.output(i), resize_ref(ref.rgb(i % 16), 64, 64, True), fmt, tolerance(plan["taps_x"], plan["taps_y"]))
        if fail:
            bad.append((i, fail))
    res = {"bad": bad[:20], "nbad": len(bad), "n": len(t), "chunks": t.geometry()["chunks"], "unconverged": t.unconverged_runs(),
           "bytes": t.bytes()["rgb"], "sample": len(sample), "scale": plan["scale"], "launches": t.kernel_ms()["resize"][1]}
    for x in (t, base, ref):
        x.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(res))


@pytest.mark.gpu
def test_tiled_batch_in_several_chunks(mjx, tmp_path):
    res = run_child(tmp_path, "child_tiled()", timeout=900)
    assert res["nbad"] == 0 and res["n"] == 128 and res["sample"] == 32 and res["unconverged"] == 0, res
    assert res["chunks"] >= 3 and res["launches"] == res["chunks"] and res["scale"] == 2, res
    assert res["bytes"] == 128 * 64 * 64 * 3 * 2, res

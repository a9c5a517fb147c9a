"""Resize on the device with the bicubic and the nearest filter (MJX_RESIZE_FILTER, include/mjx.h) beside the triangle.

The contract is the triangle's (tests/test_resize.py) with another weight: the intermediate -- byte for byte the plain packed decode at
(s, R) -- is resampled with torch's bicubic rule (antialias: a = -0.5, the window widens with the ratio, clipped and renormalised;
no antialias: a = -0.75, four taps, out-of-range taps fold onto the edge sample, nothing renormalised) or with the nearest-exact
rule, in float32, not rounded between the passes; U8 is rint of the sample CLAMPED to [0, 255], F32 / F16 take the unclamped sample.

The reference is the rule restated in float64 numpy with exact whole-number coordinates, pinned against torch in double and Pillow.
The tolerance is test_resize's bound times the absolute weight sums -- a bicubic sample sums terms of up to 255 |w|:
tol = 255 Ax Ay (Tx + Ty + 8) 2^-21, T the tap counts of mjx_resize_plan, A the largest sum |w| of a row of the axis' float64 matrix
(1 for nearest, at most 1.25 for a = -0.5 and 1.375 for a = -0.75).  check_against is test_resize's, unchanged.  Nearest has no
tolerance: every element is the formats' table on the byte picked.
"""
import ctypes
import functools
import inspect
import json
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import jpegwriter as jw
import scaled_ref
import test_orientation as tor
import test_output_formats as of
import test_resize as trs
import test_roi_decode as roi

ROOT = trs.ROOT
BAND_CAP = trs.BAND_CAP
F32_PLANAR = trs.F32_PLANAR
KINDS = (("bicubic", True), ("bicubic", False), ("nearest", False))       # (filter, antialias): the three new forms
CODE = {"bilinear": 0, "bicubic": 1, "nearest": 2}
# |weight - float64| of mjx_resize_filter_weights.  A weight is k_a(x) / sum: x = |t| / 2F is one float32 rounding of an exact
# quotient, the Horner form three more on intermediates of at most 8 (|x - 5| x + 8), times |a| <= 0.75, and the division by a sum
# of up to a few hundred such terms -- about 8 * 4 * 2^-24 = 2^-19 at the worst.  Measured over the cases of the test below:
# weights 6.5e-7 = 2^-20.6 (antialias) and 5.7e-7 (no antialias), row sums 8.3e-7 = 2^-20.2 off 1: a margin of 2.3.
WEIGHT_BOUND = 2.0 ** -19


def _read(p):
    with open(p, "rb") as f:
        return f.read()


# ---- the rules, in float64 with exact coordinates ------------------------------------------------------------------------------------------
def cubic(x, a):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, a * (((x - 5) * x + 8) * x - 4), 0.0))


def _floor(q):
    return q.numerator // q.denominator


@functools.lru_cache(maxsize=256)
def axis_matrix(n_in, n_out, filt, aa):
    """[n_out, n_in] float64: row X holds the weights of output coordinate X (folded onto the edge samples where the rule folds).
    Computed once per axis and shared: nobody writes into it."""
    if filt == "bilinear":
        return trs.axis_matrix(n_in, n_out, aa)
    # exact coordinates: c = num / den, tap j lies (2 (2 j + 1) n_out - 2 num) / (2 den) from it; Python's whole numbers, one float64
    # division per tap (test_the_rules_equal_torch_in_float64_and_pillow pins the result)
    m = np.zeros((n_out, n_in), np.float64)
    den = 2 * n_out
    for X in range(n_out):
        num = (2 * X + 1) * n_in
        if filt == "nearest":
            m[X, num // den] = 1.0
        elif aa:
            F = max(n_in, n_out)                                     # fs = F / n_out
            lo, hi = max(0, (num + n_out - 4 * F) // den), min(n_in, (num + n_out + 4 * F) // den)
            j = np.arange(lo, hi, dtype=np.int64)
            w = cubic(((2 * j + 1) * n_out - num) / (2.0 * F), -0.5)
            m[X, lo:hi] = w / w.sum()
        else:
            q = (num - n_out) // den                                 # floor(c - 1/2), may be -1
            j = np.arange(q - 1, q + 3, dtype=np.int64)              # at distances 1 + t, t, 1 - t, 2 - t
            np.add.at(m[X], np.clip(j, 0, n_in - 1), cubic(((2 * j + 1) * n_out - num) / float(den), -0.75))
    return m


def windows(n_in, n_out, filt, aa):
    """the window lengths of the rule, clipped to [0, n_in): what mjx_resize_plan's tap counts are measured against"""
    out = []
    for X in range(n_out):
        c = Fraction((2 * X + 1) * n_in, 2 * n_out)
        if filt == "nearest":
            out.append(1); continue
        fs = max(Fraction(1), Fraction(n_in, n_out)) if aa else Fraction(1)
        out.append(min(n_in, _floor(c + 2 * fs + Fraction(1, 2))) - max(0, _floor(c - 2 * fs + Fraction(1, 2))))
    return out


def max_taps(n_in, n_out, filt, aa):
    return int((axis_matrix(n_in, n_out, filt, aa) != 0).sum(axis=1).max())


def abs_sum(n_in, n_out, filt, aa):
    return float(np.abs(axis_matrix(n_in, n_out, filt, aa)).sum(axis=1).max())


def resize_ref(img, width, height, filt, aa):
    a = np.asarray(img, np.float64)
    rows = np.einsum("yi,ijc->yjc", axis_matrix(a.shape[0], height, filt, aa), a)          # (one axis at a time: the same sums)
    return np.einsum("yjc,xj->yxc", rows, axis_matrix(a.shape[1], width, filt, aa))


def tolerance(taps, rect_wh, target, filt, aa):
    ax, ay = abs_sum(rect_wh[0], target[0], filt, aa), abs_sum(rect_wh[1], target[1], filt, aa)
    assert 1.0 - 1e-12 <= ax <= 1.375 + 1e-12 and 1.0 - 1e-12 <= ay <= 1.375 + 1e-12
    return 255.0 * ax * ay * (taps[0] + taps[1] + 8) * 2.0 ** -21


def nearest_pick(img, width, height):
    h, w = img.shape[:2]
    ys = [((2 * Y + 1) * h) // (2 * height) for Y in range(height)]
    xs = [((2 * X + 1) * w) // (2 * width) for X in range(width)]
    return np.ascontiguousarray(img[ys][:, xs])


def rs_of(mjx, target, filt, aa, auto):
    return mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto, filter=filt)


# ---- CPU 1: the rules are torch's and Pillow's ------------------------------------------------------------------------------------------------
SIZES = [((37, 53), (16, 24)), ((37, 53), (74, 80)), ((64, 48), (7, 9)), ((5, 3), (17, 11)), ((1, 9), (4, 3)), ((300, 200), (224, 224)),
         ((2, 2), (5, 5)), ((1, 1), (5, 3)), ((100, 3), (7, 9))]                      # (h, w) -> (oh, ow)


def test_the_rules_equal_torch_in_float64_and_pillow():
    import torch
    import torch.nn.functional as F
    from PIL import Image
    rng = np.random.RandomState(5)
    worst, worst_pil = 0.0, 0.0
    for (h, w), (oh, ow) in SIZES:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1))))[None]
        for aa in (False, True):
            want = F.interpolate(t, size=(oh, ow), mode="bicubic", align_corners=False, antialias=aa)[0].numpy()
            worst = max(worst, float(np.abs(np.transpose(resize_ref(img, ow, oh, "bicubic", aa), (2, 0, 1)) - want).max()))
        pil = np.asarray(Image.fromarray(img[:, :, 0].astype(np.float32), mode="F").resize((ow, oh), Image.BICUBIC), np.float64)
        worst_pil = max(worst_pil, float(np.abs(resize_ref(img[:, :, :1], ow, oh, "bicubic", True)[:, :, 0] - pil).max()))
    for (h, w), (oh, ow) in SIZES + [((23, 35), (24, 16)), ((23, 35), (50, 70)), ((23, 35), (5, 7)), ((23, 35), (23, 35))]:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1))))[None]
        want = np.transpose(F.interpolate(t, size=(oh, ow), mode="nearest-exact")[0].numpy(), (1, 2, 0))
        assert np.array_equal(resize_ref(img, ow, oh, "nearest", False), want) and np.array_equal(nearest_pick(img, ow, oh), want), (h, w, oh, ow)
    print("largest difference to torch (float64): %.3g, to Pillow (mode F): %.3g" % (worst, worst_pil))
    assert worst <= 1e-9 and worst_pil <= 1e-3


# ---- CPU 2: the kernels' weights ----------------------------------------------------------------------------------------------------------------
def _dense_weights(mjx, n_in, n_out, filt, aa, xs=None):
    lib = mjx.lib()
    first, cnt = ctypes.c_uint32(), ctypes.c_size_t()
    buf = np.zeros(4 * n_in + 16, np.float32)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    xs = range(n_out) if xs is None else xs
    m = np.zeros((len(xs), n_in), np.float64)
    for r, X in enumerate(xs):
        assert lib.mjx_resize_filter_weights(n_in, n_out, CODE[filt], int(aa), X, ctypes.byref(first), ptr, buf.size, ctypes.byref(cnt)) == mjx.OK
        assert cnt.value >= 1 and first.value + cnt.value <= n_in, (n_in, n_out, filt, aa, X, first.value, cnt.value)
        m[r, first.value:first.value + cnt.value] = buf[:cnt.value]
    return m


def test_weights_of_the_kernels_routine_against_float64(mjx):
    worst, worst_sum, n = {}, {}, 0
    for filt, aa in KINDS:
        for n_out in (1, 7, 16, 24, 224):
            for n_in in range(1, 301):
                got = _dense_weights(mjx, n_in, n_out, filt, aa)
                d = float(np.abs(got - axis_matrix(n_in, n_out, filt, aa)).max())
                s = float(np.abs(got.sum(axis=1) - 1.0).max())
                assert d <= WEIGHT_BOUND and s <= WEIGHT_BOUND, (n_in, n_out, filt, aa, d, s)
                if filt == "nearest":
                    assert d == 0.0 and s == 0.0
                worst[(filt, aa)], worst_sum[(filt, aa)], n = max(worst.get((filt, aa), 0.0), d), max(worst_sum.get((filt, aa), 0.0), s), n + 1
        got = _dense_weights(mjx, 3840, 224, filt, aa, xs=[223])      # (a float32 product (X + 0.5) r would be 2e-4 pixels off here)
        d = float(np.abs(got - axis_matrix(3840, 224, filt, aa)[223:224]).max())
        assert d <= WEIGHT_BOUND and abs(float(got.sum()) - 1.0) <= WEIGHT_BOUND, (filt, aa, d)
        worst[(filt, aa)] = max(worst[(filt, aa)], d)
    assert n == 4500
    print("largest weight difference", worst, "largest |row sum - 1|", worst_sum)
    # filter 0 is mjx_resize_weights, bit for bit
    lib = mjx.lib()
    for aa in (False, True):
        for n_in, n_out in ((37, 16), (16, 37), (300, 7), (5, 5), (3840, 224)):
            for X in range(n_out):
                f0, w0 = mjx.resize_weights(n_in, n_out, aa, X)
                f1, c1 = ctypes.c_uint32(), ctypes.c_size_t()
                w1 = np.zeros(len(w0) + 4, np.float32)
                assert lib.mjx_resize_filter_weights(n_in, n_out, 0, int(aa), X, ctypes.byref(f1), w1.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     w1.size, ctypes.byref(c1)) == mjx.OK
                assert (f1.value, c1.value) == (f0, len(w0)) and of.same_bits(w1[:c1.value], w0)
    # the Python front door, and the argument errors
    f, w = mjx.resize_weights(2, 5, False, 0, filter="bicubic")
    assert f == 0 and len(w) == 2 and abs(float(w.sum()) - 1.0) <= WEIGHT_BOUND
    assert mjx.resize_weights(9, 4, True, 2, filter="nearest") == (5, np.ones(1, np.float32))
    for flt in (1, 2):
        for bad in ((0, 4, 0), (4, 0, 0), (4, 4, 4), ((1 << 24) + 1, 4, 0)):
            assert lib.mjx_resize_filter_weights(bad[0], bad[1], flt, 1, bad[2], None, None, 0, None) == mjx.ERR_INVALID_ARG
    for flt in (3, -1, 255):
        assert lib.mjx_resize_filter_weights(8, 4, flt, 1, 0, None, None, 0, None) == mjx.ERR_INVALID_ARG
    with pytest.raises(mjx.MjxError):
        mjx.Resize(4, 4, filter="lanczos")


# ---- CPU 3: the plan ----------------------------------------------------------------------------------------------------------------------------
def test_resize_plan_taps_the_filter_byte_and_the_unchanged_auto_scale_rule(mjx):
    rng = np.random.RandomState(23)
    n, slack = 0, 0
    for (W, H, sub) in ((1001, 37, "420"), (61, 45, "gray"), (333, 217, "422")):
        scan = mjx.ParsedScan(mjx.synth_jpeg(W, H, sub, 75, seed=3))
        try:
            for _ in range(30):
                rect = None
                if rng.randint(4):
                    w, h = int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))
                    rect = (int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1)), w, h)
                tw, th = int(rng.choice([1, 7, 24, 70, 224, 300])), int(rng.choice([1, 7, 16, 37, 224, 300]))
                filt, aa = KINDS[int(rng.randint(3))]
                got = scan.resize_plan(rs_of(mjx, (tw, th), filt, aa, True), roi=rect)
                s, rs = trs.auto_scale_rule(W, H, rect, tw, th)
                assert (got["scale"], got["rect"]) == (s, rs), (W, H, rect, tw, th, filt, got)
                assert got == dict(scan.resize_plan(mjx.Resize(tw, th, antialias=aa), roi=rect), taps_x=got["taps_x"], taps_y=got["taps_y"])
                # the tap counts are the rule's windows exactly: positions are whole numbers on both sides (the triangle's test allows
                # 0 .. 2 more because it counts POSITIVE weights; measured here against the windows themselves the slack is 0)
                tx, ty = max(windows(rs[2], tw, filt, aa)), max(windows(rs[3], th, filt, aa))
                assert (got["taps_x"], got["taps_y"]) == (tx, ty), (W, H, rect, tw, th, filt, aa, got, tx, ty)
                sx, sy = tx - max_taps(rs[2], tw, filt, aa), ty - max_taps(rs[3], th, filt, aa)
                assert 0 <= sx <= 3 and 0 <= sy <= 3                # (over the NON-ZERO float64 weights: measured 0 .. 3 -- a window's end taps may weigh exactly 0)
                slack = max(slack, sx, sy)
                n += 1
            d = rs_of(mjx, (24, 16), "bicubic", True, True).desc()
            for v, want in ((0, mjx.OK), (1, mjx.OK), (2, mjx.OK), (3, mjx.ERR_INVALID_ARG), (255, mjx.ERR_INVALID_ARG)):
                d.filter = v
                try:
                    scan.resize_plan(d)
                    rc = mjx.OK
                except mjx.MjxError as e:
                    rc = e.code
                assert rc == want, (v, rc)
        finally:
            scan.close()
    print("largest surplus of the tap counts over the non-zero float64 weights:", slack)
    assert n == 90


# ---- CPU 4: mirrors -------------------------------------------------------------------------------------------------------------------------------
def test_mirrors_of_the_filter_byte_and_the_entry_point(mjx):
    hdr_all = _read(os.path.join(ROOT, "include", "mjx.h")).decode()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_all, flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    assert re.search(r"#define MJX_RESIZE_FILTER_OFFSET 10\b", hdr)
    assert re.search(r"#define MJX_RESIZE_FILTER\(rs\) \(\(\(uint8_t \*\)\(rs\)\)\[MJX_RESIZE_FILTER_OFFSET\]\)", hdr)
    for name, v in (("TRIANGLE", 0), ("BICUBIC", 1), ("NEAREST", 2)):
        assert re.search(r"#define MJX_FILTER_%s\s+%d\b" % (name, v), hdr) and re.search(r"pub const MJX_FILTER_%s: u8 = %d;" % (name, v), rs)
        assert getattr(mjx, "FILTER_" + name) == v
    assert re.search(r"pub const MJX_RESIZE_FILTER_OFFSET: usize = 10;", rs) and "pub fn set_filter(&mut self, filter: u8)" in rs
    c = re.search(r"\bmjx_resize_filter_weights\(([^;{]*?)\);", hdr).group(1)
    r = re.search(r"pub fn mjx_resize_filter_weights\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
    assert c.count(",") + 1 == 9 and r.count(",") + 1 == 9
    assert len(mjx.SYMBOLS["mjx_resize_filter_weights"][1]) == 9 and hasattr(mjx.lib(), "mjx_resize_filter_weights")
    assert re.search(r"#define MJX_ABI_VERSION 2\b", hdr) and re.search(r"MJX_K_COUNT = 11", hdr)
    # the byte: offset 10 of twelve, zero in every description built the old way
    assert ctypes.sizeof(mjx.ResizeDesc) == 12 and [f[0] for f in mjx.ResizeDesc._fields_] == ["width", "height", "antialias", "auto_scale"]
    d = mjx.ResizeDesc(24, 16, 1, 1)
    assert d.filter == 0 and bytes(d)[10] == 0
    d.filter = 2
    assert bytes(d)[10] == 2 and bytes(d)[11] == 0 and (d.width, d.height, d.antialias, d.auto_scale) == (24, 16, 1, 1)
    assert bytes(mjx.Resize(24, 16).desc())[10] == 0 and mjx.Resize(24, 16).filter == "bilinear"
    for name, v in (("bilinear", 0), ("bicubic", 1), ("nearest", 2)):
        assert mjx.Resize(24, 16, filter=name).desc().filter == v
    # decode_into rebuilds the description at the tensor's size: the filter goes along
    src = mjx.Resize(0, 0, antialias=False, auto_scale=False, filter="bicubic").sized(24, 16)
    assert (src.width, src.height, src.antialias, src.auto_scale, src.filter, src.desc().filter) == (24, 16, False, False, "bicubic", 1)
    assert "resize.sized(w, h)" in inspect.getsource(mjx.decode_into)


def test_bicubic_decode_batch_without_a_device_is_a_device_error(tmp_path):
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
        "    mjx.decode_batch(c, [data], resize=mjx.Resize(24, 16, filter='bicubic'))\n"
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


# ---- the sweep's cases (CPU 5 and GPU 1 walk the same list) -----------------------------------------------------------------------------------
TARGETS = ((70, 37), (24, 16))
MODES = ((True, 1), (False, 2))                     # (auto_scale, the call's scale)


def u8_eligible(rect_wh, target, filt, aa):
    """test_resize.u8_eligible's rule with the filter's own tap counts"""
    for n_in, n_out in zip(rect_wh, target):
        if Fraction(n_in, n_out).denominator < 5 or max_taps(n_in, n_out, filt, aa) > 30:
            return False
    return True


def sweep_cases(mjx, inputs, scans):
    """every input x mode x kind x (two targets x (whole picture, one seeded rectangle) + the upscale from a 19 x 13 rectangle); fmt: one
    of the eleven formats other than planar F32 in rotation -- a U8 format only where the case is u8_eligible (nearest: any)"""
    cases, rot = [], 0
    others = [f for f in range(12) if f != F32_PLANAR]
    for k, (name, data) in enumerate(inputs):
        W, H = roi.frame_of(data)[:2]
        for auto, scale in MODES:
            pw, ph = (W, H) if auto else (-(-W // scale), -(-H // scale))
            rng = np.random.RandomState(200 * k + 10 * scale + int(auto))
            rects = [None, trs._seeded_rect(rng, pw, ph, 9, 9)]
            up = (int(rng.randint(0, pw - trs.UPSCALE[1][0] + 1)), int(rng.randint(0, ph - trs.UPSCALE[1][1] + 1))) + trs.UPSCALE[1]
            for filt, aa in KINDS:
                for target, r in [(t, r) for t in TARGETS for r in rects] + [(trs.UPSCALE[0], up)]:
                    plan = scans[k].resize_plan(rs_of(mjx, target, filt, aa, auto), roi=r, scale=scale)
                    f = others[rot % 11]
                    while filt != "nearest" and of.FORMATS[f][0] == "uint8" and not u8_eligible(plan["rect"][2:], target, filt, aa):
                        rot += 1
                        f = others[rot % 11]
                    rot += 1
                    cases.append(dict(k=k, auto=auto, scale=scale, filt=filt, aa=aa, target=target, roi=r, s=plan["scale"], R=plan["rect"],
                                      taps=(plan["taps_x"], plan["taps_y"]), fmt=f))
    return cases


def test_band_share_of_the_reference_alone(mjx, orc):
    inputs = trs.sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        cases = sweep_cases(mjx, inputs, scans)
    finally:
        for s in scans:
            s.close()
    assert len(cases) == 6 * 2 * 3 * 5 and set(c["s"] for c in cases if c["auto"]) == {1, 2, 4, 8}
    decs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True) for _, d in inputs]
    fulls, share = {}, {}
    for c in cases:
        if of.FORMATS[c["fmt"]][0] != "uint8" or c["filt"] == "nearest":
            continue
        key = (c["k"], c["s"])
        if key not in fulls:
            fulls[key] = decs[c["k"]].rgb if c["s"] == 1 else scaled_ref.scaled_rgb(inputs[c["k"]][1], c["s"], decs[c["k"]])
        ref = resize_ref(roi.crop(fulls[key], c["R"]), c["target"][0], c["target"][1], c["filt"], c["aa"])
        tol = tolerance(c["taps"], c["R"][2:], c["target"], c["filt"], c["aa"])
        b, t = share.get(c["aa"], (0, 0))
        share[c["aa"]] = (b + int((np.rint(np.clip(ref - tol, 0, 255)) != np.rint(np.clip(ref + tol, 0, 255))).sum()), t + ref.size)
    print("U8 elements of the sweep in the band, by antialias:", {k: (v, "%.3f %%" % (100.0 * v[0] / max(v[1], 1))) for k, v in share.items()})
    for aa in (True, False):
        assert share[aa][1] > 5000 and share[aa][0] <= BAND_CAP * share[aa][1], share


# ---- GPU: shared pieces -----------------------------------------------------------------------------------------------------------------------------
def run(mjx, ctx, scans, fmt, rs, expect_ok=True, **kw):
    b = mjx.Batch(ctx, scans, output=fmt, resize=rs, **kw)
    try:
        b.decode(); b.wait()
        n = len(scans)
        if expect_ok:
            assert [b.status(i) for i in range(n)] == [mjx.OK] * n, [b.status(i) for i in range(n)]
        return [b.output(i) for i in range(n)], [(b.scale(i), b.rect(i)) for i in range(n)]
    finally:
        b.close()


def check(got, packed, target, filt, aa, fmt, taps=None, ref=None):
    """-> failure text or None (and band, u8 through check_against); ref: resize_ref of these arguments, where the caller shares it"""
    if filt == "nearest":
        return (None if of.same_bits(got, of.expected(nearest_pick(packed, *target), fmt)) else "not the table on the byte picked"), 0, 0
    h, w = packed.shape[:2]
    if taps is None:
        taps = (max(windows(w, target[0], filt, aa)), max(windows(h, target[1], filt, aa)))
    if ref is None:
        ref = resize_ref(packed, target[0], target[1], filt, aa)
    return trs.check_against(got, ref, fmt, tolerance(taps, (w, h), target, filt, aa))


def child_sweep():
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, profiling=True)
    inputs = trs.sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    cases = sweep_cases(mjx, inputs, scans)
    packed = trs._packed(mjx, ctx, scans, set((c["k"], c["s"], c["R"]) for c in cases))
    bad, band, total, launches = [], 0, 0, 0
    groups = {}
    for c in cases:
        for f in (F32_PLANAR, c["fmt"]):
            groups.setdefault((c["auto"], c["scale"], c["filt"], c["aa"], c["target"], f), []).append(c)
    refs = {}
    for (auto, scale, filt, aa, target, f), cs in sorted(groups.items(), key=lambda g: g[0]):
        fmt = of.make_format(mjx, f)
        b = mjx.Batch(ctx, [scans[c["k"]] for c in cs], scale=scale, rois=[c["roi"] for c in cs], output=fmt, resize=rs_of(mjx, target, filt, aa, auto))
        b.decode(); b.wait()
        launches += b.kernel_ms()["resize"][1]
        for i, c in enumerate(cs):
            what = (inputs[c["k"]][0], auto, scale, filt, aa, target, c["roi"], of.FORMATS[f])
            if b.status(i) != mjx.OK:
                bad.append(what + ("status", b.status(i))); continue
            inf = b.info(i)
            if (b.scale(i), b.rect(i)) != (c["s"], c["R"]) or (inf["width"], inf["height"]) != target:
                bad.append(what + ("scale / rectangle / size", b.scale(i), b.rect(i), inf)); continue
            src = packed[(c["k"], c["s"], c["R"])]
            if filt != "nearest" and id(c) not in refs:              # (computed once per case, shared by its two formats, not written to)
                refs[id(c)] = resize_ref(src, target[0], target[1], filt, aa)
            fail, nb, nt = check(b.output(i), src, target, filt, aa, fmt, c["taps"], refs.get(id(c)))
            band, total = band + nb, total + nt
            if fail:
                bad.append(what + (fail,))
        b.close()
    plain = mjx.Batch(ctx, scans[:2], output=of.make_format(mjx, 3))
    plain.decode(); plain.wait()
    idle = plain.kernel_ms()["resize"][1]
    plain.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps({"bad": bad[:30], "nbad": len(bad), "cases": len(cases), "batches": len(groups), "band": band, "u8": total,
                      "auto_scales": sorted(set(c["s"] for c in cases if c["auto"])), "launches": int(launches), "idle_launches": int(idle)}))


def run_child(tmp_path, call, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_resize_filters as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


# ---- GPU 1: the sweep ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_every_case_is_the_rule_applied_to_the_packed_decode(mjx, tmp_path):
    res = run_child(tmp_path, "child_sweep()")
    assert res["nbad"] == 0, res
    assert res["cases"] == 6 * 2 * 3 * 5 and res["auto_scales"] == [1, 2, 4, 8], res
    assert res["u8"] > 5000 and res["band"] <= BAND_CAP * res["u8"], res
    assert res["launches"] >= res["batches"] and res["idle_launches"] == 0, res


# ---- GPU 2: exactness -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_target_of_the_rectangles_size_is_the_format_table_bit_for_bit(mjx, gpu_ctx):
    inputs = trs.sweep_inputs(mjx)[:4]
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        w, h = 37, 29
        rois = []
        for i, (_, d) in enumerate(inputs):
            W, H = roi.frame_of(d)[:2]
            rois.append((min(3 + 5 * i, W - w), min(2 + 3 * i, H - h), w, h))
        packed = tor.packed_decodes(mjx, gpu_ctx, scans, rois=rois)
        for f in range(12):
            fmt = of.make_format(mjx, f)
            for filt, aa in KINDS:
                got, sr = run(mjx, gpu_ctx, scans, fmt, rs_of(mjx, (w, h), filt, aa, bool(f & 2)), rois=rois)
                for i in range(len(scans)):
                    assert sr[i] == (1, rois[i])
                    assert of.same_bits(got[i], of.expected(packed[i], fmt)), (of.FORMATS[f], filt, aa, inputs[i][0])
    finally:
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_nearest_is_the_byte_the_integer_rule_picks_in_every_format(mjx, gpu_ctx):
    scans = [mjx.ParsedScan(mjx.synth_jpeg(61, 45, "gray")), mjx.ParsedScan(mjx.synth_jpeg(61, 45, "420", 75, seed=4))]
    try:
        packed = tor.packed_decodes(mjx, gpu_ctx, scans)
        for target in ((24, 16), (150, 100)):
            for f in range(12):
                fmt = of.make_format(mjx, f)
                got, _ = run(mjx, gpu_ctx, scans, fmt, rs_of(mjx, target, "nearest", bool(f & 1), False))
                for i in range(len(scans)):
                    assert of.same_bits(got[i], of.expected(nearest_pick(packed[i], *target), fmt)), (target, of.FORMATS[f], i)
    finally:
        for s in scans:
            s.close()


# ---- GPU 3: the clamp -----------------------------------------------------------------------------------------------------------------------------------
def clamp_picture():
    """64 x 48, one component, DC only: a chequerboard of blocks whose levels are 128 - 140 and 128 + 140 -- the packed decode saturates
    them to 0 and 255, and a cubic across such a step leaves [0, 255] on both sides"""
    bx, by = 8, 6
    blocks = np.zeros((bx * by, 64), np.int64)
    for k in range(bx * by):
        blocks[k, 0] = 140 if ((k % bx) + (k // bx)) % 2 else -140
    return jw.jpeg_from_blocks(blocks, [(1, 1)], bx, by, [[8] + [1] * 63], jw._annex_k_tables())


@pytest.mark.gpu
def test_over_and_undershoot_is_clamped_in_u8_and_kept_in_f32(mjx, gpu_ctx):
    scan = mjx.ParsedScan(clamp_picture())
    try:
        packed = tor.packed_decodes(mjx, gpu_ctx, [scan])[0]
        assert packed.shape == (48, 64, 3) and packed.min() == 0 and packed.max() == 255
        target = (150, 110)
        for filt, aa in KINDS[:2]:
            ref = resize_ref(packed, target[0], target[1], filt, aa)
            assert ref.min() < -5.0 and ref.max() > 260.0, (ref.min(), ref.max())
            f32, u8 = of.make_format(mjx, F32_PLANAR), of.make_format(mjx, 0)
            g32, _ = run(mjx, gpu_ctx, [scan], f32, rs_of(mjx, target, filt, aa, False))
            g8, _ = run(mjx, gpu_ctx, [scan], u8, rs_of(mjx, target, filt, aa, False))
            fail, _, _ = check(g32[0], packed, target, filt, aa, f32)
            assert fail is None, (filt, aa, fail)
            sc, bi = np.asarray(f32.scale, np.float64), np.asarray(f32.bias, np.float64)
            v = (g32[0].astype(np.float64) - bi.reshape(3, 1, 1)) / sc.reshape(3, 1, 1)
            assert v.min() < -5.0 and v.max() > 260.0, (v.min(), v.max())                 # F32 shows the unclamped sample
            fail, band, n = check(g8[0], packed, target, filt, aa, u8)
            assert fail is None, (filt, aa, fail)
            over, under = ref > 255.5, ref < -0.5                     # (format 0 is H x W x 3 in R,G,B: the reference's own shape)
            assert over.sum() > 100 and under.sum() > 100
            assert np.all(g8[0][over] == 255) and np.all(g8[0][under] == 0)
    finally:
        scan.close()


# ---- GPU 4: narrow and extreme ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rectangles_narrower_than_the_window_and_large_ratios(mjx, gpu_ctx):
    lena = mjx.ParsedScan(_read(os.path.join(ROOT, "tests", "data", "lena.jpeg")))
    small = mjx.ParsedScan(mjx.synth_jpeg(75, 50, "444"))
    fmt = of.make_format(mjx, F32_PLANAR)
    bad = []
    try:
        rects = [(11, 7, 1, 9), (11, 7, 2, 9), (11, 7, 3, 9), (20, 5, 9, 1), (20, 5, 9, 2), (20, 5, 9, 3), (30, 30, 1, 1), (30, 30, 2, 2)]
        packed = tor.packed_decodes(mjx, gpu_ctx, [small] * len(rects), rois=rects)
        for filt, aa in KINDS:
            # (n_in = 2 without antialias: q - 1 < 0 and q + 2 >= n_in on one axis -- both folds in one window)
            got, sr = run(mjx, gpu_ctx, [small] * len(rects), fmt, rs_of(mjx, (17, 11), filt, aa, False), rois=rects)
            for i, r in enumerate(rects):
                assert sr[i] == (1, r)
                fail, _, _ = check(got[i], packed[i], (17, 11), filt, aa, fmt)
                if fail:
                    bad.append((filt, aa, r, fail))
        big = tor.packed_decodes(mjx, gpu_ctx, [lena])[0]
        assert big.shape[0] == 512 and big.shape[1] == 512
        for target in ((9, 7), (1, 1)):
            for filt, aa in KINDS:
                rs = rs_of(mjx, target, filt, aa, False)
                plan = lena.resize_plan(rs)
                assert (plan["taps_x"] > 200) == (filt == "bicubic" and aa)
                got, _ = run(mjx, gpu_ctx, [lena], fmt, rs)
                fail, _, _ = check(got[0], big, target, filt, aa, fmt, (plan["taps_x"], plan["taps_y"]))
                if fail:
                    bad.append((filt, aa, target, fail))
        assert bad == [], bad[:8]
    finally:
        lena.close(); small.close()


# ---- GPU 5: composition ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_orientation_luminance_and_libjpeg_pixels_compose_with_the_filter(mjx, gpu_ctx):
    datas = [mjx.synth_jpeg(160, 96, "420"), mjx.synth_jpeg(75, 50, "444")]
    scans = [mjx.ParsedScan(d) for d in datas]
    bad = []
    try:
        fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
        S = tor.packed_decodes(mjx, gpu_ctx, scans)
        # orientation: the rule on orient_c(I); codes 2 (mirror) and 6 (axes swapped); a rectangle of D
        for code in (2, 6):
            for filt, aa in (("bicubic", True), ("nearest", False)):
                r = (3, 4, 41, 30)
                got, _ = run(mjx, gpu_ctx, scans, fmt, rs_of(mjx, (23, 31), filt, aa, False), rois=r, orient=mjx.Orient(exif=False, extra=code))
                for i, g in enumerate(got):
                    D = np.ascontiguousarray(tor.orient_np(code, S[i])[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])
                    fail, _, _ = check(g, D, (23, 31), filt, aa, fmt)
                    if fail:
                        bad.append(("orient", code, filt, i, fail))
        # luminance: one channel, the one-byte intermediate; with and without a turn
        f1 = mjx.Output("float32", planar=True, channels=1, mean=0.5, std=0.25)
        f3 = mjx.Output("float32", planar=True, scale=[float(f1.scale[0])] * 3, bias=[float(f1.bias[0])] * 3)
        L = []
        b = mjx.Batch(gpu_ctx, scans, output=mjx.Output("uint8", channels=1))
        b.decode(); b.wait()
        L = [b.output(i).reshape(b.info(i)["height"], b.info(i)["width"]) for i in range(len(scans))]
        b.close()
        for code in (1, 6):
            for filt, aa in (("bicubic", True), ("bicubic", False), ("nearest", False)):
                got, _ = run(mjx, gpu_ctx, scans, f1, rs_of(mjx, (29, 21), filt, aa, False), orient=mjx.Orient(exif=False, extra=code))
                for i, g in enumerate(got):
                    D = np.repeat(np.ascontiguousarray(tor.orient_np(code, L[i][:, :, None])), 3, axis=2)
                    fail, _, _ = check(np.ascontiguousarray(np.repeat(g.reshape(1, 21, 29), 3, axis=0)), D, (29, 21), filt, aa, f3)
                    if fail:
                        bad.append(("luma", code, filt, aa, i, fail))
        # libjpeg's pixels: the intermediate is that option's packed picture
        P = []
        b = mjx.Batch(gpu_ctx, scans, pixels="libjpeg")
        b.decode(); b.wait()
        P = [b.rgb(i) for i in range(len(scans))]
        b.close()
        for filt, aa in KINDS[:2]:
            got, sr = run(mjx, gpu_ctx, scans, fmt, rs_of(mjx, (40, 27), filt, aa, True), pixels="libjpeg")
            for i, g in enumerate(got):
                assert sr[i][0] == 1
                fail, _, _ = check(g, P[i], (40, 27), filt, aa, fmt)
                if fail:
                    bad.append(("libjpeg", filt, aa, i, fail))
        assert bad == [], bad[:8]
    finally:
        for s in scans:
            s.close()


SENTINEL = 0xA5


@pytest.mark.gpu
def test_caller_owned_pitched_memory_from_file_bytes_with_per_file_rectangles(mjx, gpu_ctx):
    inputs = trs.sweep_inputs(mjx)
    datas = [d for _, d in inputs]
    n = len(datas)
    rois = []
    for i, d in enumerate(datas):
        W, H = roi.frame_of(d)[:2]
        rois.append(None if i == 1 else (W // 7, H // 5, W - W // 3, H - H // 4))
    w, h = 31, 19
    rs = mjx.Resize(w, h, antialias=True, auto_scale=True, filter="bicubic")
    fmt0 = of.make_format(mjx, 6)                                    # f16 planar
    esz = 2
    rp, pp = w + 5, h * (w + 5) + 11
    per = 3 * pp + 13
    guard = 4096
    total = guard + n * per * esz + guard
    hip = of._hip(mjx)
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [(base.value + guard + i * per * esz, w, h, rp, pp) for i in range(n)]
        fmt = of.make_format(mjx, 6, dst=dst)
        b, st = mjx.decode_batch(gpu_ctx, datas, chunk_images=2, rois=rois, output=fmt, resize=rs)
        try:
            assert st == [mjx.OK] * n, st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            covered = np.zeros(total, bool)
            el = (np.arange(3)[:, None, None] * pp + np.arange(h)[None, :, None] * rp + np.arange(w)[None, None, :])
            for i in range(n):
                s, R = b.scale(i), b.rect(i)
                scan = mjx.ParsedScan(datas[i])
                plan = scan.resize_plan(rs, roi=rois[i])
                scan.close()
                assert (plan["scale"], plan["rect"]) == (s, R)
                packed = roi.crop(roi._full(mjx, gpu_ctx, datas[i], s), R)
                slot = mem[guard + i * per * esz: guard + (i + 1) * per * esz].view(np.float16)
                fail, _, _ = check(np.ascontiguousarray(slot[el]), packed, (w, h), "bicubic", True, fmt0, (plan["taps_x"], plan["taps_y"]))
                assert fail is None, ("picture", i, fail)
                covered[(guard + i * per * esz + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)] = True
            assert np.all(mem[~covered] == SENTINEL), "bytes outside the pictures' elements were written"
            assert b.geometry()["chunks"] >= 3
        finally:
            b.close()
    finally:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipFree(base) == 0


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import torch.nn.functional as F
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    sizes = [(333, 317, "444"), (301, 263, "440"), (160, 96, "420")]
    datas = [mjx.synth_jpeg(w, h, sub, 75, seed=60 + k) for k, (w, h, sub) in enumerate(sizes)]
    n = len(datas)
    dev = torch.device("cuda", 0)
    H, W = 48, 56
    rs = mjx.Resize(0, 0, antialias=True, auto_scale=True, filter="bicubic")
    out = torch.full((n, 3, H, W), float("nan"), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, resize=rs)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    for i in range(n):
        if st[i] != mjx.OK:
            bad.append(("status", i, st[i])); continue
        scan = mjx.ParsedScan(datas[i])
        plan = scan.resize_plan(mjx.Resize(W, H, filter="bicubic"))
        scan.close()
        ref, _ = mjx.decode_batch(ctx, [datas[i]], scale=plan["scale"], rois=[plan["rect"]])
        packed = ref.rgb(0)
        ref.close()
        t = torch.from_numpy(np.ascontiguousarray(np.transpose(packed, (2, 0, 1))).astype(np.float32))[None].to(dev)
        want = F.interpolate(t, size=(H, W), mode="bicubic", align_corners=False, antialias=True)[0].cpu().numpy().astype(np.float64)
        tol = tolerance((plan["taps_x"], plan["taps_y"]), plan["rect"][2:], (W, H), "bicubic", True)
        fail, _, _ = trs.check_against(np.ascontiguousarray(got[i]), np.transpose(want, (1, 2, 0)), fmt, tol)
        if fail:
            bad.append((i, fail))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad), "n": n}))


@pytest.mark.gpu
def test_decode_into_a_tensor_with_the_bicubic_filter_is_torchs_interpolate(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0 and res["n"] == 3, res


@pytest.mark.gpu
def test_a_tiled_batch_in_several_chunks_carries_the_filter(mjx, gpu_ctx):
    datas = mjx.synth_batch(6, 96, 64, "420", 75, seed0=500)
    scans = [mjx.ParsedScan(d) for d in datas]
    fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    try:
        packed = tor.packed_decodes(mjx, gpu_ctx, scans)
        for filt, aa in (("bicubic", False), ("nearest", False)):
            base = mjx.Batch(gpu_ctx, scans, output=fmt, resize=rs_of(mjx, (40, 24), filt, aa, False), chunk_images=4)
            t = base.tile(3)
            try:
                t.decode(); t.wait()
                assert len(t) == 18 and t.geometry()["chunks"] >= 3
                for i in range(len(t)):
                    assert t.status(i) == mjx.OK
                    fail, _, _ = check(t.output(i), packed[i % 6], (40, 24), filt, aa, fmt)
                    assert fail is None, (filt, i, fail)
            finally:
                t.close(); base.close()
    finally:
        for s in scans:
            s.close()


# ---- GPU 6: the triangle is untouched -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_filter_bilinear_is_the_plain_resize_byte_for_byte(mjx, gpu_ctx):
    inputs = trs.sweep_inputs(mjx)
    scans = [mjx.ParsedScan(d) for _, d in inputs]
    try:
        for f in (0, F32_PLANAR, 5):
            fmt = of.make_format(mjx, f)
            for aa in (True, False):
                a, sa = run(mjx, gpu_ctx, scans, fmt, mjx.Resize(70, 37, antialias=aa, auto_scale=True, filter="bilinear"))
                b, sb = run(mjx, gpu_ctx, scans, fmt, mjx.Resize(70, 37, antialias=aa, auto_scale=True))
                assert sa == sb
                for i in range(len(scans)):
                    assert of.same_bits(a[i], b[i]), (of.FORMATS[f], aa, inputs[i][0])
    finally:
        for s in scans:
            s.close()

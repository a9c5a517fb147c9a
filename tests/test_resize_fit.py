"""Aspect-preserving resize: MJX_FIT_COVER (centre-crop) and MJX_FIT_CONTAIN (letterbox).

The rule of include/mjx.h is restated here in Python (fit_rule) and compared with mjx_resize_fit_plan, which runs the planner's own
routine.  On the GPU every comparison is bit for bit against the stretch path of the same build, taken in the same process through the
rewritten call: COVER is the stretch call with rois[i] = A', CONTAIN's inner rectangle is the stretch call with the target iw x ih, and
every other element of a letterboxed target is the format's table applied to the pad byte (test_output_formats.tables_for: exact
rationals rounded once).  One anchor does not pass through the library's resize: test_resize.resize_ref with test_resize's tolerance.

CPU (-m "not gpu"): the rule, its properties, the plan functions, argument rules, mirrors, the no-device error.
GPU (-m gpu): cover, contain, caller-owned memory, orientation, front doors, identities, the independent anchor."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_orientation as ori
import test_output_formats as of
import test_resize as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCH, COVER, CONTAIN = 0, 1, 2
FIT_NAMES = ("stretch", "cover", "contain")
PAD = (10, 200, 77)


def _read(p):
    with open(p, "rb") as f:
        return f.read()


# ---- the rule, restated from the header's text -------------------------------------------------------------------------------------
def rnd(a, b):
    return (2 * a + b) // (2 * b)


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def fit_rule(mode, A, W, H):
    """-> (A', inner): the rectangle the picture is planned with and the inner rectangle (ox, oy, iw, ih) of the W x H target"""
    x, y, w, h = A
    inner = (0, 0, W, H)
    if mode == COVER:
        if w * H > h * W:
            w2 = clamp(rnd(h * W, H), 1, w)
            x, w = x + (w - w2) // 2, w2
        elif w * H < h * W:
            h2 = clamp(rnd(w * H, W), 1, h)
            y, h = y + (h - h2) // 2, h2
    elif mode == CONTAIN:
        iw, ih = W, H
        if w * H > h * W:
            ih = clamp(rnd(h * W, w), 1, H)
        elif w * H < h * W:
            iw = clamp(rnd(w * H, h), 1, W)
        inner = ((W - iw) // 2, (H - ih) // 2, iw, ih)
    return (x, y, w, h), inner


def d_size(pw, ph, code, s):
    """the picture that leaves (D) at scale s: ceil(w / s) x ceil(h / s), axes swapped for codes 5 .. 8"""
    ow, oh = -(-pw // s), -(-ph // s)
    return (oh, ow) if code >= 5 else (ow, oh)


def asked(pw, ph, code, roi, auto, scale):
    dw, dh = d_size(pw, ph, code, 1 if auto else scale)
    return (0, 0, dw, dh) if roi is None else tuple(roi)


def check_properties(mode, A, W, H, A2, inner):
    x, y, w, h = A
    x2, y2, w2, h2 = A2
    ox, oy, iw, ih = inner
    assert x <= x2 and y <= y2 and x2 + w2 <= x + w and y2 + h2 <= y + h and w2 >= 1 and h2 >= 1           # A' inside A
    assert abs((x2 - x) - ((x + w) - (x2 + w2))) <= 1 and abs((y2 - y) - ((y + h) - (y2 + h2))) <= 1      # centred to within a pixel
    assert 0 <= ox and 0 <= oy and ox + iw <= W and oy + ih <= H and iw >= 1 and ih >= 1                  # inner inside the target
    assert abs(ox - (W - ox - iw)) <= 1 and abs(oy - (H - oy - ih)) <= 1
    assert iw == W or ih == H                                                                             # one axis is the target's
    assert w2 == w or h2 == h
    if mode != CONTAIN:
        assert inner == (0, 0, W, H)
    if mode != COVER:
        assert A2 == A
    if w * H == h * W:
        assert A2 == A and inner == (0, 0, W, H)                                                          # equal aspect: the stretch plan


class SizedScan:
    """One parsed 4:2:0 file whose description is given any frame size: the plan functions are host-only and look at the geometry."""
    def __init__(self, mjx):
        self.mjx = mjx
        self.scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))

    def sized(self, w, h):
        self.scan.desc.width, self.scan.desc.height = w, h
        return self.scan

    def close(self):
        self.scan.desc.width, self.scan.desc.height = 64, 48
        self.scan.close()


SIDES = (1, 7, 16, 37, 64, 65, 224, 300)


def test_the_rule_equals_mjx_resize_fit_plan_on_seeded_cases(mjx):
    rng = np.random.RandomState(23)
    ss = SizedScan(mjx)
    n = 0
    seen = set()
    try:
        for k in range(2000):
            big = k % 40 == 0
            pw, ph = (int(rng.choice([65535, 40000, 4097])), int(rng.randint(1, 301))) if big else (int(rng.randint(1, 301)), int(rng.randint(1, 301)))
            if big and rng.randint(2):
                pw, ph = ph, pw
            mode, code, auto = int(rng.randint(3)), int(rng.randint(1, 9)), bool(rng.randint(2))
            scale = 1 if auto else int(rng.choice([1, 2, 4, 8]))
            dw, dh = d_size(pw, ph, code, scale)
            roi = None
            if rng.randint(3):
                w, h = int(rng.randint(1, dw + 1)), int(rng.randint(1, dh + 1))
                roi = (int(rng.randint(0, dw - w + 1)), int(rng.randint(0, dh - h + 1)), w, h)
            W, H = int(rng.choice(SIDES)), int(rng.choice(SIDES))
            rs = mjx.Resize(W, H, antialias=bool(rng.randint(2)), auto_scale=auto, fit=FIT_NAMES[mode])
            got = ss.sized(pw, ph).fit_plan(rs, code=code, roi=roi, scale=scale)
            A = asked(pw, ph, code, roi, auto, scale)
            A2, inner = fit_rule(mode, A, W, H)
            assert (got["asked"], got["inner"]) == (A2, inner), (pw, ph, code, roi, auto, scale, W, H, mode, got)
            check_properties(mode, A, W, H, A2, inner)
            n += 1
            seen.add((mode, A2 != A, inner != (0, 0, W, H)))
    finally:
        ss.close()
    assert n == 2000 and seen == {(0, False, False), (1, False, False), (1, True, False), (2, False, False), (2, False, True)}


def test_the_rule_exhaustively_up_to_twelve(mjx):
    """all w, h, W, H <= 12: the rectangle (0, 0, w, h) of a 12 x 12 picture, both modes, against the library; the properties on all three"""
    ss = SizedScan(mjx)
    try:
        scan = ss.sized(12, 12)
        lib, desc = mjx.lib(), ctypes.byref(scan.desc)
        opts = mjx._opts(rois=(0, 0, 1, 1))
        rect_in = ctypes.cast(opts.rois, ctypes.POINTER(mjx.Rect))
        inner, ask, sc = mjx.Rect(), mjx.Rect(), ctypes.c_uint8()
        rs = mjx.Resize(1, 1, auto_scale=False).desc()
        n = 0
        for w in range(1, 13):
            for h in range(1, 13):
                rect_in[0].w, rect_in[0].h = w, h
                for W in range(1, 13):
                    for H in range(1, 13):
                        rs.width, rs.height = W, H
                        for mode in (STRETCH, COVER, CONTAIN):
                            A2, inn = fit_rule(mode, (0, 0, w, h), W, H)
                            check_properties(mode, (0, 0, w, h), W, H, A2, inn)
                            if mode == STRETCH:
                                continue
                            rs.fit = mode
                            rc = lib.mjx_resize_fit_plan(desc, ctypes.byref(opts), None, ctypes.byref(rs), 1, 0, ctypes.byref(inner), ctypes.byref(ask),
                                                         ctypes.byref(sc))
                            assert rc == mjx.OK
                            assert ((ask.x, ask.y, ask.w, ask.h), (inner.x, inner.y, inner.w, inner.h)) == (A2, inn), (w, h, W, H, mode)
                            n += 1
        assert n == 2 * 12 ** 4
    finally:
        ss.close()


def test_plans_with_the_fit_byte_are_the_stretch_plans_of_the_rewritten_call(mjx):
    """mjx_resize_plan and mjx_orient_plan: COVER is the stretch plan with roi = A', CONTAIN the stretch plan with the target iw x ih
    (mjx_orient_plan's width / height stay the picture that leaves: the whole target)."""
    rng = np.random.RandomState(5)
    n = 0
    for (pw, ph, sub) in ((200, 40, "420"), (61, 45, "gray"), (333, 217, "444"), (16, 160, "420")):
        scan = mjx.ParsedScan(mjx.synth_jpeg(pw, ph, sub, 75, seed=2))
        try:
            for _ in range(60):
                mode, code, auto = int(rng.randint(1, 3)), int(rng.randint(1, 9)), bool(rng.randint(2))
                scale = 1 if auto else int(rng.choice([1, 2, 4]))
                dw, dh = d_size(pw, ph, code, scale)
                roi = None
                if rng.randint(2):
                    w, h = int(rng.randint(1, dw + 1)), int(rng.randint(1, dh + 1))
                    roi = (int(rng.randint(0, dw - w + 1)), int(rng.randint(0, dh - h + 1)), w, h)
                W, H = int(rng.choice(SIDES)), int(rng.choice(SIDES))
                kw = dict(antialias=bool(rng.randint(2)), auto_scale=auto, filter=("bilinear", "bicubic", "nearest")[int(rng.randint(3))])
                A = asked(pw, ph, code, roi, auto, scale)
                A2, inner = fit_rule(mode, A, W, H)
                rewritten_roi = (A2 if A2 != A else roi) if mode == COVER else roi
                tw, th = (inner[2], inner[3]) if mode == CONTAIN else (W, H)
                got = scan.orient_plan(code, mjx.Resize(W, H, fit=FIT_NAMES[mode], **kw), roi=roi, scale=scale)
                want = scan.orient_plan(code, mjx.Resize(tw, th, **kw), roi=rewritten_roi, scale=scale)
                assert (got["stored_rect"], got["scale"]) == (want["stored_rect"], want["scale"]), (pw, ph, code, roi, W, H, mode)
                assert (got["width"], got["height"]) == (W, H) and (want["width"], want["height"]) == (tw, th)
                fp = scan.fit_plan(mjx.Resize(W, H, fit=FIT_NAMES[mode], **kw), code=code, roi=roi, scale=scale)
                assert fp["scale"] == want["scale"]
                if code == 1:
                    assert scan.resize_plan(mjx.Resize(W, H, fit=FIT_NAMES[mode], **kw), roi=roi, scale=scale) == \
                        scan.resize_plan(mjx.Resize(tw, th, **kw), roi=rewritten_roi, scale=scale)
                n += 1
        finally:
            scan.close()
    assert n == 240


def test_argument_rules(mjx):
    scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))

    def code(rs, fn="resize_plan", **kw):
        try:
            getattr(scan, fn)(rs, **kw)
            return mjx.OK
        except mjx.MjxError as e:
            return e.code
    try:
        for bad in (3, 255):
            d = mjx.Resize(24, 16).desc()
            d.fit = bad
            assert code(d) == mjx.ERR_INVALID_ARG and code(d, "fit_plan") == mjx.ERR_INVALID_ARG
            try:
                scan.orient_plan(1, d)
                assert False
            except mjx.MjxError as e:
                assert e.code == mjx.ERR_INVALID_ARG
        # fit 0 with pad bytes set is fine, and means what it meant
        out = mjx.Output("float32", planar=True, pad=(1, 2, 3))
        assert scan.fit_plan(mjx.Resize(24, 16), output=out) == dict(inner=(0, 0, 24, 16), asked=(0, 0, 64, 48), scale=2)
        # the resize's own refusals are unchanged under every mode
        for fit in FIT_NAMES:
            assert code(mjx.Resize(24, 16, fit=fit)) == mjx.OK and code(mjx.Resize(24, 16, auto_scale=False, fit=fit), scale=4) == mjx.OK
            assert code(mjx.Resize(0, 16, fit=fit)) == mjx.ERR_INVALID_ARG and code(mjx.Resize(24, 0, fit=fit)) == mjx.ERR_INVALID_ARG
            assert code(mjx.Resize(24, 16, fit=fit), layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
            assert code(mjx.Resize(24, 16, fit=fit), scale=2) == mjx.ERR_INVALID_ARG                   # auto_scale with a scale
            assert code(mjx.Resize(24, 16, fit=fit), roi=(60, 0, 8, 8)) == mjx.ERR_INVALID_ARG
            assert code(mjx.Resize(24, 16, fit=fit), roi=(0, 0, 8, 0)) == mjx.ERR_INVALID_ARG
            assert code(mjx.Resize(24, 16, fit=fit), roi=(56, 40, 8, 8)) == mjx.OK
            assert code(mjx.Resize(24, 16, fit=fit), "fit_plan", layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        with pytest.raises(mjx.MjxError):
            mjx.Resize(24, 16, fit="fill")
        with pytest.raises(mjx.MjxError):
            mjx.Output(pad=256)
        with pytest.raises(mjx.MjxError):
            mjx.Output(pad=(1, 2))
        assert mjx.Output(pad=7).pad == (7, 7, 7) and mjx.Resize(3, 4, fit="cover").sized(5, 6).desc().fit == COVER
    finally:
        scan.close()


def test_mirrors_of_the_fit_byte_the_pad_bytes_and_the_entry_points(mjx):
    hdr = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    assert re.search(r"#define MJX_RESIZE_FIT_OFFSET 11\b", hdr) and re.search(r"#define MJX_OUTPUT_PAD_OFFSET 28\b", hdr)
    assert re.search(r"#define MJX_RESIZE_FIT\(rs\) \(\(\(uint8_t \*\)\(rs\)\)\[MJX_RESIZE_FIT_OFFSET\]\)", hdr)
    assert re.search(r"#define MJX_OUTPUT_PAD\(out\) \(\(uint8_t \*\)\(out\) \+ MJX_OUTPUT_PAD_OFFSET\)", hdr)
    assert re.search(r"pub const MJX_RESIZE_FIT_OFFSET: usize = 11;", rs) and re.search(r"pub const MJX_OUTPUT_PAD_OFFSET: usize = 28;", rs)
    assert mjx.ResizeDesc.FIT_OFFSET == 11 and mjx.OutputDesc.PAD_OFFSET == 28
    for name, v in (("STRETCH", 0), ("COVER", 1), ("CONTAIN", 2)):
        assert re.search(r"#define MJX_FIT_%s\s+%d\b" % (name, v), hdr)
        assert re.search(r"pub const MJX_FIT_%s: u8 = %d;" % (name, v), rs)
        assert getattr(mjx, "FIT_" + name) == v
    assert re.search(r"pub fn set_fit\(&mut self", rs) and re.search(r"pub fn set_pad\(&mut self", rs)
    # sizes and declared members are as they were
    assert ctypes.sizeof(mjx.ResizeDesc) == 12 and [f[0] for f in mjx.ResizeDesc._fields_] == ["width", "height", "antialias", "auto_scale"]
    assert ctypes.sizeof(mjx.OutputDesc) == 48 and [f[0] for f in mjx.OutputDesc._fields_] == ["dtype", "planar", "bgr", "scale", "bias", "dst", "n_dst"]
    assert mjx.OutputDesc.bias.offset + 12 == 28 and mjx.OutputDesc.dst.offset == 32
    body = re.search(r"typedef struct mjx_resize\s*\{(.*?)\}\s*mjx_resize;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", body) == ["width", "height", "antialias", "auto_scale"]
    # a description built without the new keywords has zeros in the new bytes
    assert bytes(mjx.Resize(24, 16, filter="bicubic").desc())[11] == 0
    assert bytes(mjx.Output("float16", planar=True, bgr=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, channels=3).desc())[28:32] == b"\0\0\0\0"
    d = mjx.Output(pad=PAD).desc()
    assert bytes(d)[28:31] == bytes(PAD) and d.pad == PAD and bytes(mjx.Resize(1, 1, fit="contain").desc())[11] == 2
    for fn, n in (("mjx_resize_fit_plan", 9), ("mjx_batch_fit_rect", 3)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)
        assert fn in mjx.SYMBOLS and len(mjx.SYMBOLS[fn][1]) == n and hasattr(mjx.lib(), fn), fn
    assert re.search(r"#define MJX_ABI_VERSION 2\b", hdr) and re.search(r"MJX_K_COUNT = 11", hdr) and len(mjx.KERNEL_NAMES) == 11


def test_a_fit_call_without_a_device_is_a_device_error(tmp_path):
    """No fallback: with the devices hidden mjx_ctx_create fails, and a letterboxed mjx_decode_batch_resize on what it leaves says MJX_ERR_DEVICE."""
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
        "for fit in ('cover', 'contain'):\n"
        "    try:\n"
        "        mjx.decode_batch(c, [data], resize=mjx.Resize(24, 16, fit=fit), output=mjx.Output(pad=(1, 2, 3)))\n"
        "        print('decoded')\n"
        "    except mjx.MjxError as e:\n"
        "        print('rc', e.code)\n" % (ROOT, ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    dev = str(ge.load_package().ERR_DEVICE)
    assert out.stdout.split() == ["ctx", dev, "False", "rc", dev, "rc", dev], out.stdout


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
SIZES = ((64, 48), (48, 64), (37, 29), (200, 40), (16, 160))
SUBS = ("420", "444", "gray")
TARGETS = ((24, 16), (70, 37), (64, 64), (65, 17), (150, 40), (1, 7), (7, 1))
MODES = ((True, 1), (False, 1), (False, 2))           # (auto_scale, the call's scale)
KINDS = [(f, aa) for f in ("bilinear", "bicubic", "nearest") for aa in (False, True)]
FORMAT_IDS = ("u8_interleaved", "f32_planar_mean_std", "f16_bgr")


def make_fmt(mjx, name, **kw):
    if name == "u8_interleaved":
        return mjx.Output("uint8", **kw)
    if name == "f32_planar_mean_std":
        return mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, **kw)
    if name == "f16_bgr":
        return mjx.Output("float16", bgr=True, mean=of.IMAGENET_MEAN[::-1], std=of.IMAGENET_STD[::-1], **kw)
    assert name == "f32_luma"
    return mjx.Output("float32", channels=1, mean=0.45, std=0.225, **kw)


@pytest.fixture(scope="module")
def sources(mjx):
    """the fifteen synthetic pictures: (width, height, file bytes, parsed scan)"""
    out = []
    for k, (w, h) in enumerate(SIZES):
        for j, sub in enumerate(SUBS):
            d = mjx.synth_jpeg(w, h, sub, 80, seed=100 + 3 * k + j)
            out.append((w, h, d, mjx.ParsedScan(d)))
    yield out
    for s in out:
        s[3].close()


def caller_rect(dw, dh):
    """a rectangle on top, a function of the size alone: off centre, odd sides"""
    w, h = max(1, (2 * dw) // 3 | 1 if dw > 2 else dw), max(1, (3 * dh) // 4 | 1 if dh > 2 else dh)
    w, h = min(w, dw), min(h, dh)
    return ((dw - w) // 3, (dh - h) // 2, w, h)


def rois_for(sources, auto, scale, with_rects=True, code=1):
    """every second picture has a caller's rectangle, in D's coordinates at the scale the call gives them in"""
    rois = []
    for i, (w, h, _, _) in enumerate(sources):
        dw, dh = d_size(w, h, code, 1 if auto else scale)
        rois.append(caller_rect(dw, dh) if with_rects and i % 2 else None)
    return rois


def run(mjx, ctx, scans, **kw):
    b = mjx.Batch(ctx, scans, **kw)
    b.decode(); b.wait()
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FORMAT_IDS)
def test_cover_is_the_stretch_call_on_the_centred_rectangle(mjx, gpu_ctx, sources, fmt_name):
    fmt = make_fmt(mjx, fmt_name, pad=PAD)             # (the pad bytes are ignored by this mode)
    scans = [s[3] for s in sources]
    n = cropped = 0
    for W, H in TARGETS:
        for auto, scale in MODES:
            rois = rois_for(sources, auto, scale)
            As = [asked(s[0], s[1], 1, r, auto, scale) for s, r in zip(sources, rois)]
            rew = [fit_rule(COVER, A, W, H)[0] for A in As]
            ref_rois = [a2 if a2 != a else r for a2, a, r in zip(rew, As, rois)]
            for filt, aa in KINDS:
                kw = dict(antialias=aa, auto_scale=auto, filter=filt)
                got = run(mjx, gpu_ctx, scans, scale=scale, rois=rois, output=fmt, resize=mjx.Resize(W, H, fit="cover", **kw))
                ref = run(mjx, gpu_ctx, scans, scale=scale, rois=ref_rois, output=make_fmt(mjx, fmt_name), resize=mjx.Resize(W, H, **kw))
                try:
                    for i in range(len(scans)):
                        assert got.status(i) == mjx.OK and ref.status(i) == mjx.OK
                        assert (got.scale(i), got.rect(i)) == (ref.scale(i), ref.rect(i))
                        assert got.fit_rect(i) == (0, 0, W, H)
                        assert of.same_bits(got.output(i), ref.output(i)), (W, H, auto, scale, filt, aa, i)
                        n += 1
                        cropped += rew[i] != As[i]
                finally:
                    got.close(); ref.close()
    assert n == len(TARGETS) * len(MODES) * len(KINDS) * len(scans) and cropped > n // 2


def pad_elements(fmt):
    """the format's table applied to the pad bytes, by OUTPUT channel"""
    t = of.tables_for(fmt)
    return [t[c][fmt.pad[c]] for c in range(3)]


def letterboxed(fmt, W, H, inner, inner_out):
    """the whole target: the pad element everywhere, the stretch call's output in the inner rectangle"""
    ox, oy, iw, ih = inner
    pe = pad_elements(fmt)
    if fmt.channels == 1:                               # luminance: H x W x 1 and 1 x H x W are the same memory, pad byte 0 alone
        full = np.full((H, W), pe[0], fmt.numpy_dtype())
        full[oy:oy + ih, ox:ox + iw] = inner_out.reshape(ih, iw)
        return full.reshape((1, H, W) if fmt.planar else (H, W, 1))
    if fmt.planar:
        full = np.stack([np.full((H, W), pe[c], fmt.numpy_dtype()) for c in range(3)])
        full[:, oy:oy + ih, ox:ox + iw] = inner_out
    else:
        full = np.stack([np.full((H, W), pe[c], fmt.numpy_dtype()) for c in range(3)], axis=2)
        full[oy:oy + ih, ox:ox + iw, :] = inner_out
    return np.ascontiguousarray(full)


def contain_references(mjx, ctx, sources, inners, rois, fmt_ref, scale, pixels, code=1, **kw):
    """per picture the stretch call with Resize(iw, ih): one batch per distinct inner size"""
    out = [None] * len(sources)
    for size in sorted(set((i[2], i[3]) for i in inners)):
        idx = [k for k, i in enumerate(inners) if (i[2], i[3]) == size]
        extra = dict(orient=mjx.Orient(exif=False, extra=[code] * len(idx))) if code != 1 else {}
        b = run(mjx, ctx, [sources[k][3] for k in idx], scale=scale, rois=[rois[k] for k in idx], output=fmt_ref, pixels=pixels,
                resize=mjx.Resize(size[0], size[1], **kw), **extra)
        try:
            for j, k in enumerate(idx):
                assert b.status(j) == mjx.OK
                out[k] = (b.output(j), b.scale(j), b.rect(j))
        finally:
            b.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pixels", [None, "libjpeg"], ids=["reference_pixels", "libjpeg_pixels"])
@pytest.mark.parametrize("fmt_name", FORMAT_IDS + ("f32_luma",))
def test_contain_is_the_stretch_call_inside_and_the_pad_element_outside(mjx, gpu_ctx, sources, fmt_name, pixels):
    fmt = make_fmt(mjx, fmt_name, pad=PAD)
    scans = [s[3] for s in sources]
    n = borders = 0
    modes = MODES if pixels is None else MODES[:2]      # (libjpeg's pixels exist at full size only)
    for t, (W, H) in enumerate(TARGETS):
        for m, (auto, scale) in enumerate(modes):
            filt, aa = KINDS[(2 * t + m) % len(KINDS)]
            kw = dict(antialias=aa, auto_scale=auto, filter=filt)
            rois = rois_for(sources, auto, scale)
            inners = [fit_rule(CONTAIN, asked(s[0], s[1], 1, r, auto, scale), W, H)[1] for s, r in zip(sources, rois)]
            refs = contain_references(mjx, gpu_ctx, sources, inners, rois, make_fmt(mjx, fmt_name), scale, pixels, **kw)
            got = run(mjx, gpu_ctx, scans, scale=scale, rois=rois, output=fmt, pixels=pixels, resize=mjx.Resize(W, H, fit="contain", **kw))
            try:
                for i in range(len(scans)):
                    assert got.status(i) == mjx.OK
                    assert (got.scale(i), got.rect(i)) == refs[i][1:] and got.fit_rect(i) == inners[i]
                    inf = got.output_info(i)
                    assert (inf["width"], inf["height"]) == (W, H)
                    out = got.output(i)
                    want = letterboxed(fmt, W, H, inners[i], refs[i][0]).reshape(out.shape)
                    assert of.same_bits(out, want), (W, H, auto, scale, filt, aa, i, inners[i])
                    n += 1
                    borders += inners[i][2:] != (W, H)
                esz = np.dtype(fmt.numpy_dtype()).itemsize
                assert got.bytes()["rgb"] == len(scans) * W * H * (1 if fmt.channels == 1 else 3) * esz      # the whole target counts
            finally:
                got.close()
    assert n == len(TARGETS) * len(modes) * len(scans) and borders > n // 2


SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_images", [0, 1])
@pytest.mark.parametrize("fmt_name", ("u8_interleaved", "f32_planar_mean_std", "f16_bgr"))
def test_caller_owned_pitched_memory_nothing_outside_nothing_left(mjx, gpu_ctx, sources, fmt_name, chunk_images):
    """One allocation, pitched slots with guard elements, sentinel-filled.  Complete pictures fill their whole target -- no element
    keeps the sentinel -- and change nothing else; a truncated file and a progressive one between them keep their slots untouched,
    border included."""
    datas = [s[2] for s in sources[:6]]
    whole = sources[3][2]
    truncated = whole[:len(whole) // 2] + b"\xff\xd9"
    datas.insert(2, truncated)
    datas.insert(4, _read(os.path.join(ROOT, "tests", "golden", "pil", "progressive.jpg")))
    bad = {2: mjx.ERR_TRUNCATED, 4: mjx.ERR_UNSUPPORTED_FORMAT}
    n = len(datas)
    for (w, h) in ((70, 37), (65, 17), (24, 16)):
        fmt0 = make_fmt(mjx, fmt_name, pad=(10, 200, 77))
        esz = np.dtype(fmt0.numpy_dtype()).itemsize
        planar = fmt0.planar
        rp = (w if planar else 3 * w) + 5
        pp = (h * rp + 11) if planar else 0
        per = (3 * pp if planar else h * rp) + 13
        guard = 4096
        total = guard + n * per * esz + guard
        hip = of._hip(mjx)
        base = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(base), total) == 0
        try:
            assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
            dst = [(base.value + guard + i * per * esz, w, h, rp, pp) for i in range(n)]
            fmt = make_fmt(mjx, fmt_name, pad=(10, 200, 77), dst=dst)
            b, st = mjx.decode_batch(gpu_ctx, datas, chunk_images=chunk_images, output=fmt, resize=mjx.Resize(w, h, fit="contain"))
            try:
                assert st == [bad.get(i, mjx.OK) for i in range(n)], st
                mem = np.empty(total, np.uint8)
                assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
                covered = np.zeros(total, bool)
                if planar:
                    el = (np.arange(3)[:, None, None] * pp + np.arange(h)[None, :, None] * rp + np.arange(w)[None, None, :])
                else:
                    el = (np.arange(h)[:, None, None] * rp + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :])
                bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[esz]
                sent = np.frombuffer(bytes([SENTINEL]) * esz, bits)[0]
                for i in range(n):
                    if i in bad:
                        continue
                    slot = mem[guard + i * per * esz: guard + (i + 1) * per * esz].view(fmt0.numpy_dtype())
                    pic = np.ascontiguousarray(slot[el])
                    # (the pad bytes 10, 200, 77 and what the tables make of them are not the sentinel, nor is any float the tables give;
                    # a decoded u8 element may be 165 by right, so an element counts as left over where the reference says otherwise)
                    scan = mjx.ParsedScan(datas[i])
                    fp = scan.fit_plan(mjx.Resize(w, h, fit="contain"))
                    inner = fp["inner"]
                    ref = run(mjx, gpu_ctx, [scan], output=make_fmt(mjx, fmt_name), resize=mjx.Resize(inner[2], inner[3]))
                    want = letterboxed(fmt0, w, h, inner, ref.output(0))
                    ref.close(); scan.close()
                    assert of.same_bits(pic, want), (w, h, i)
                    assert all(np.array([e]).view(bits)[0] != sent for e in pad_elements(fmt0)) and not np.any((pic.view(sent.dtype) == sent) & (want.view(sent.dtype) != sent)), \
                        "an element of the target kept the sentinel"
                    assert b.fit_rect(i) == inner
                    covered[(guard + i * per * esz + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)] = True
                assert np.all(mem[~covered] == SENTINEL), ("bytes outside the complete pictures' elements were written",
                                                           np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist())
                if chunk_images:
                    assert b.geometry()["chunks"] >= n - len(bad)
            finally:
                b.close()
        finally:
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipFree(base) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (COVER, CONTAIN), ids=("cover", "contain"))
def test_orientation_codes_from_exif_with_an_extra_flip(mjx, gpu_ctx, mode):
    """64 x 48 with every EXIF code, an extra horizontal flip on every second picture; the references are the rewritten stretch calls
    through mjx_batch_create_orient."""
    base = [mjx.synth_jpeg(64, 48, sub, 80, seed=7 + k) for k, sub in enumerate(("420", "444"))]
    datas = [ori.tagged(base[c % 2], c) for c in range(1, 9)]
    extra = [2 if c % 2 else 1 for c in range(8)]
    codes = [mjx.orient_compose(c, e) for c, e in zip(range(1, 9), extra)]
    scans = [mjx.ParsedScan(d) for d in datas]
    fmt_name = "f32_planar_mean_std"
    try:
        for (W, H) in ((70, 37), (37, 70)):
            for auto, scale in MODES:
                for with_rects in (False, True):
                    kw = dict(antialias=True, auto_scale=auto)
                    rois, As = [], []
                    for c in codes:
                        dw, dh = d_size(64, 48, c, 1 if auto else scale)
                        rois.append(caller_rect(dw, dh) if with_rects else None)
                        As.append(rois[-1] or (0, 0, dw, dh))
                    plans = [fit_rule(mode, A, W, H) for A in As]
                    got = run(mjx, gpu_ctx, scans, datas=datas, scale=scale, rois=rois, output=make_fmt(mjx, fmt_name, pad=PAD),
                              orient=mjx.Orient(exif=True, extra=extra), resize=mjx.Resize(W, H, fit=FIT_NAMES[mode], **kw))
                    try:
                        for i, c in enumerate(codes):
                            A2, inner = plans[i]
                            assert got.status(i) == mjx.OK and got.orientation(i) == c
                            assert scans[i].fit_plan(mjx.Resize(W, H, fit=FIT_NAMES[mode], **kw), code=c, roi=rois[i], scale=scale)["inner"] == inner
                            r_roi = (A2 if A2 != As[i] else rois[i]) if mode == COVER else rois[i]
                            ref = run(mjx, gpu_ctx, [scans[i]], scale=scale, rois=[r_roi], output=make_fmt(mjx, fmt_name),
                                      orient=mjx.Orient(exif=False, extra=[c]), resize=mjx.Resize(inner[2], inner[3], **kw))
                            try:
                                assert ref.status(0) == mjx.OK and (got.scale(i), got.rect(i)) == (ref.scale(0), ref.rect(0))
                                want = letterboxed(make_fmt(mjx, fmt_name, pad=PAD), W, H, inner, ref.output(0))
                                assert of.same_bits(got.output(i), want), (W, H, auto, scale, with_rects, c)
                                assert got.fit_rect(i) == inner
                            finally:
                                ref.close()
                    finally:
                        got.close()
    finally:
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_front_doors_from_file_bytes_fit_rect_and_tile(mjx, gpu_ctx, sources):
    """mjx_decode_batch_resize and _orient from file bytes, five sizes in one call; Batch.fit_rect is the plan; tile(3) repeats it"""
    five = [sources[3 * k + (k % 3)] for k in range(5)]
    datas = [s[2] for s in five]
    W, H = 64, 64
    fmt_name = "f16_bgr"
    for code in (1, 6):
        orient = None if code == 1 else mjx.Orient(exif=False, extra=[code] * 5)
        rs = mjx.Resize(W, H, fit="contain")
        inners = [fit_rule(CONTAIN, asked(s[0], s[1], code, None, True, 1), W, H)[1] for s in five]
        refs = contain_references(mjx, gpu_ctx, five, inners, [None] * 5, make_fmt(mjx, fmt_name), 1, None, code=code)
        b, st = mjx.decode_batch(gpu_ctx, datas, output=make_fmt(mjx, fmt_name, pad=PAD), resize=rs, orient=orient)
        try:
            assert st == [mjx.OK] * 5
            for i in range(5):
                assert b.fit_rect(i) == inners[i] == five[i][3].fit_plan(rs, code=code)["inner"]
                want = letterboxed(make_fmt(mjx, fmt_name, pad=PAD), W, H, inners[i], refs[i][0])
                assert of.same_bits(b.output(i), want), (code, i)
        finally:
            b.close()
        # cover through the same doors
        rs = mjx.Resize(W, H, fit="cover")
        rew = [fit_rule(COVER, asked(s[0], s[1], code, None, True, 1), W, H)[0] for s in five]
        b, st = mjx.decode_batch(gpu_ctx, datas, output=make_fmt(mjx, fmt_name), resize=rs, orient=orient)
        r, st2 = mjx.decode_batch(gpu_ctx, datas, output=make_fmt(mjx, fmt_name), rois=rew, resize=mjx.Resize(W, H), orient=orient)
        try:
            assert st == st2 == [mjx.OK] * 5
            for i in range(5):
                assert of.same_bits(b.output(i), r.output(i)) and b.fit_rect(i) == (0, 0, W, H)
        finally:
            b.close(); r.close()
    # a batch without a resize has no inner rectangle; a tiled letterboxed batch repeats pictures, borders and rectangles
    scans = [s[3] for s in five]
    plain = run(mjx, gpu_ctx, scans)
    assert plain.fit_rect(0) == (0, 0, 0, 0)
    plain.close()
    fmt = make_fmt(mjx, "f32_planar_mean_std", pad=PAD)
    small = run(mjx, gpu_ctx, scans, output=fmt, resize=mjx.Resize(70, 37, fit="contain"))
    tiled = small.tile(3)
    tiled.decode(); tiled.wait()
    try:
        assert len(tiled) == 15
        for i in range(15):
            assert tiled.status(i) == mjx.OK and tiled.fit_rect(i) == small.fit_rect(i % 5)
            assert of.same_bits(tiled.output(i), small.output(i % 5)), i
        assert tiled.bytes()["rgb"] == 3 * small.bytes()["rgb"]
    finally:
        tiled.close(); small.close()


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    sizes = [(64, 48, "420"), (48, 64, "444"), (37, 29, "gray"), (200, 40, "420"), (16, 160, "444")]
    datas = [mjx.synth_jpeg(w, h, sub, 80, seed=40 + k) for k, (w, h, sub) in enumerate(sizes)]
    mean, std = of.IMAGENET_MEAN, of.IMAGENET_STD
    pad = tuple(int(round(255 * m)) for m in mean)
    dev = torch.device("cuda", 0)
    out = torch.full((5, 3, 64, 64), float("nan"), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out, mean=mean, std=std, pad=pad, resize=mjx.Resize(0, 0, fit="contain"))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    fmt = mjx.Output("float32", planar=True, mean=mean, std=std, pad=pad)
    bad = []
    near_zero = float(np.abs(np.array(pad_elements(fmt), np.float64)).max())
    for i, (w, h, _) in enumerate(sizes):
        _, inner = fit_rule(CONTAIN, (0, 0, w, h), 64, 64)
        scan = mjx.ParsedScan(datas[i])
        b = mjx.Batch(ctx, [scan], output=mjx.Output("float32", planar=True, mean=mean, std=std), resize=mjx.Resize(inner[2], inner[3]))
        b.decode(); b.wait()
        want = letterboxed(fmt, 64, 64, inner, b.output(0))
        b.close(); scan.close()
        if st[i] != mjx.OK or not of.same_bits(np.ascontiguousarray(got[i]), want):
            bad.append(i)
    ctx.close()
    print(json.dumps({"bad": bad, "st": st, "near_zero": near_zero}))


def run_child(tmp_path, call, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_resize_fit as t\nt.%s\n" % (ROOT, ROOT, call))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_decode_into_a_letterboxed_tensor_padded_with_the_mean(mjx, tmp_path):
    """5 x 3 x 64 x 64 float32, mean / std, pad = the mean's bytes: the tensor assembled from per-picture stretch calls, bit for bit;
    the padded elements are within half a byte's step of zero."""
    res = run_child(tmp_path, "child_torch()")
    assert res["bad"] == [] and res["st"] == [0] * 5, res
    assert res["near_zero"] <= 0.5 / (255 * min(of.IMAGENET_STD)) + 1e-6, res


@pytest.mark.gpu
def test_identities(mjx, gpu_ctx, sources):
    # a picture of the target's aspect: the stretch output in all three modes; fit 0 with pad bytes set: the same bytes
    scans = [s[3] for s in sources if (s[0], s[1]) == (64, 48)]
    for fmt_name in FORMAT_IDS:
        ref = run(mjx, gpu_ctx, scans, output=make_fmt(mjx, fmt_name), resize=mjx.Resize(32, 24))
        try:
            for fit in FIT_NAMES:
                b = run(mjx, gpu_ctx, scans, output=make_fmt(mjx, fmt_name, pad=PAD), resize=mjx.Resize(32, 24, fit=fit))
                try:
                    for i in range(len(scans)):
                        assert b.status(i) == mjx.OK and (b.scale(i), b.rect(i)) == (ref.scale(i), ref.rect(i)) and b.fit_rect(i) == (0, 0, 32, 24)
                        assert of.same_bits(b.output(i), ref.output(i)), (fmt_name, fit, i)
                finally:
                    b.close()
        finally:
            ref.close()


@pytest.mark.gpu
def test_a_picture_65535_wide_letterboxed_to_one_row(mjx, gpu_ctx):
    data = mjx.synth_jpeg(65535, 16, "420", 50, seed=3)
    scan = mjx.ParsedScan(data)
    try:
        assert (scan.desc.width, scan.desc.height) == (65535, 16)
        fmt = make_fmt(mjx, "f32_planar_mean_std", pad=PAD)
        rs = mjx.Resize(224, 224, fit="contain")
        assert scan.fit_plan(rs)["inner"] == (0, 111, 224, 1) == fit_rule(CONTAIN, (0, 0, 65535, 16), 224, 224)[1]
        b = run(mjx, gpu_ctx, [scan], output=fmt, resize=rs)
        ref = run(mjx, gpu_ctx, [scan], output=make_fmt(mjx, "f32_planar_mean_std"), resize=mjx.Resize(224, 1))
        try:
            assert b.status(0) == mjx.OK and ref.status(0) == mjx.OK and (b.scale(0), b.rect(0)) == (ref.scale(0), ref.rect(0))
            out = b.output(0)
            assert of.same_bits(out, letterboxed(fmt, 224, 224, (0, 111, 224, 1), ref.output(0)))
            pe = pad_elements(fmt)
            assert all(np.all(out[c, :111] == pe[c]) and np.all(out[c, 112:] == pe[c]) for c in range(3))       # 223 pad rows
        finally:
            b.close(); ref.close()
    finally:
        scan.close()


@pytest.mark.gpu
def test_independent_anchor_the_inner_rectangle_against_the_float64_rule(mjx, gpu_ctx, sources):
    """200 x 40 -> 150 x 40 letterboxed with the triangle: the inner rectangle (0, 5, 150, 30) against test_resize.resize_ref of the
    packed decode, within test_resize.tolerance -- a reference that does not pass through the library's resize."""
    src = [s for s in sources if (s[0], s[1]) == (200, 40)]
    scans = [s[3] for s in src]
    packed = run(mjx, gpu_ctx, scans)
    try:
        for aa in (True, False):
            rs = mjx.Resize(150, 40, antialias=aa, auto_scale=False, fit="contain")
            formats = [mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, pad=PAD)]
            if tr.u8_eligible((200, 40), (150, 30), aa):
                formats.append(mjx.Output("uint8", pad=PAD))
            for fmt in formats:
                b = run(mjx, gpu_ctx, scans, output=fmt, resize=rs)
                try:
                    for i, scan in enumerate(scans):
                        assert b.status(i) == mjx.OK and b.fit_rect(i) == (0, 5, 150, 30) and b.scale(i) == 1
                        plan = scan.resize_plan(mjx.Resize(150, 30, antialias=aa, auto_scale=False))
                        out = b.output(i)
                        inner = out[:, 5:35, :] if fmt.planar else out[5:35]
                        fail, _, _ = tr.check_against(np.ascontiguousarray(inner), tr.resize_ref(packed.rgb(i), 150, 30, aa), fmt,
                                                      tr.tolerance(plan["taps_x"], plan["taps_y"]))
                        assert fail is None, (aa, i, fail)
                        pe = pad_elements(fmt)
                        border = np.concatenate([out[:, :5], out[:, 35:]], axis=1) if fmt.planar else np.concatenate([out[:5], out[35:]], axis=0)
                        for c in range(3):
                            assert np.all((border[c] if fmt.planar else border[:, :, c]) == pe[c])
                finally:
                    b.close()
    finally:
        packed.close()

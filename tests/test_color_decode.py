"""Decode of RGB, CMYK and YCCK files (mjx_opts.color = MJX_COLOR_FILE) on the GPU, byte for byte against expectations built from
twins -- the rule tests/test_ycbcr_planes.py uses: the byte of component c is the packed decode of the one-component file that carries
c's blocks (colorwriter.component_twin); the (r, g, b) of a YCCK picture is the packed decode of the three-component file that carries
components 0 .. 2 (colorwriter.ycc_twin); box replication and mjx_ink_mul compose them on the host (colorwriter.compose).  Everything
behind stage B -- rectangles, scales, formats, resize, orientation -- is the existing rule applied to that packed picture.
The host side of the option is tests/test_color_models.py."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import colorwriter as cw
import test_orientation as tor
import test_output_formats as of
import test_resize_filters as trf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LAYOUTS4 = {"1x1x4": [(1, 1)] * 4, "h2_k2": [(2, 1), (1, 1), (1, 1), (2, 1)], "v2_k2": [(1, 2), (1, 1), (1, 1), (1, 2)],
            "y22_k11": [(2, 2), (1, 1), (1, 1), (1, 1)], "y22_k22": [(2, 2), (1, 1), (1, 1), (2, 2)]}
LAYOUTS3 = {"444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)]}
HEAD = {"rgb": [cw.app14(0)], "cmyk": [cw.app14(0)], "ycck": [cw.app14(2)]}
MODEL = {"rgb": 2, "cmyk": 3, "ycck": 4}


def make(model, hv, w, h, **kw):
    return cw.color_jpeg(w, h, hv, head=HEAD[model], **kw)


def decode_all(mjx, ctx, datas, ok=True, **kw):
    """Batch over parsed scans -> [packed picture or status]"""
    color = kw.get("color")
    scans = [mjx.ParsedScan(d, color=color) for d in datas]
    b = mjx.Batch(ctx, scans, **kw)
    try:
        b.decode(); b.wait()
        st = [b.status(i) for i in range(len(datas))]
        if ok:
            assert st == [mjx.OK] * len(datas), st
        return [b.rgb(i) if s == mjx.OK else s for i, s in enumerate(st)]
    finally:
        b.close()
        for s in scans:
            s.close()


def expectations(mjx, ctx, cases, scale=1):
    """cases: [(model, ColorFile)] -> the packed pictures at 1/scale, composed from the twins' decodes (one batch for all twins)."""
    twins, where = [], []
    for model, cf in cases:
        need = range(3) if model == "rgb" else (range(4) if model == "cmyk" else (3,))
        at = {}
        for c in need:
            at[c] = len(twins)
            twins.append(cw.component_twin(cf, c))
        if model == "ycck":
            at["ycc"] = len(twins)
            twins.append(cw.ycc_twin(cf))
        where.append(at)
    dec = decode_all(mjx, ctx, twins, scale=scale)
    out = []
    for (model, cf), at in zip(cases, where):
        ow, oh = -(-cf.width // scale), -(-cf.height // scale)
        comp = [dec[at[c]][..., 0] if c in at else None for c in range(len(cf.hv))]
        out.append(cw.compose(model, cf, comp, ow, oh, rgb3=dec[at["ycc"]] if "ycc" in at else None))
    return out


def check_equal(got, want, tags):
    bad = [(t, g.shape, w.shape, int((g != w).sum()) if g.shape == w.shape else -1) for g, w, t in zip(got, want, tags)
           if g.shape != w.shape or not np.array_equal(g, w)]
    assert not bad, bad


# ---- layouts and sizes -----------------------------------------------------------------------------------------------------------------
def layout_cases():
    cases, tags = [], []
    for name, hv in LAYOUTS4.items():
        hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
        for k, (w, h) in enumerate(((8 * hmax, 8 * vmax), (37, 29))):
            for model in ("cmyk", "ycck"):
                cases.append((model, make(model, hv, w, h, quality=85, seed=11 + k, noise=6.0)))
                tags.append((name, model, w, h))
    for name, hv in LAYOUTS3.items():
        hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
        for k, (w, h) in enumerate(((8 * hmax, 8 * vmax), (37, 29))):
            cases.append(("rgb", make("rgb", hv, w, h, quality=85, seed=21 + k, noise=6.0)))
            tags.append((name, "rgb", w, h))
    # ... and the other ways a file says RGB and CMYK: component ids, no segment at all
    cases.append(("rgb", cw.color_jpeg(37, 29, LAYOUTS3["420"], ids=b"RGB", seed=31)))
    tags.append(("420", "rgb by ids", 37, 29))
    cases.append(("cmyk", cw.color_jpeg(37, 29, LAYOUTS4["h2_k2"], seed=32)))
    tags.append(("h2_k2", "cmyk without a segment", 37, 29))
    return cases, tags


def test_every_layout_one_mcu_and_clipped_odd_sizes(mjx, gpu_ctx):
    """The five four-component layouts -- three of them share their blocks per MCU with 4:2:2 or 4:2:0, whose DC kernels carry three
    running sums -- as CMYK and as YCCK, and RGB at 4:4:4 and 4:2:0: one MCU, and 37 x 29 (clipped last MCUs, odd width)."""
    cases, tags = layout_cases()
    want = expectations(mjx, gpu_ctx, cases)
    datas = [cf.data for _, cf in cases]
    scans = [mjx.ParsedScan(d, color="file") for d in datas]
    b = mjx.Batch(gpu_ctx, scans, color="file")
    try:
        b.decode(); b.wait()
        assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas)
        assert [b.color_model(i) for i in range(len(datas))] == [MODEL[m] for m, _ in cases]
        check_equal([b.rgb(i) for i in range(len(datas))], want, tags)
    finally:
        b.close()
        for s in scans:
            s.close()
    # the same pictures one per chunk: no picture leans on what another of its chunk launched
    got = decode_all(mjx, gpu_ctx, datas, color="file", chunk_images=1)
    check_equal(got, want, tags)


def test_k_carry_across_dc_segments_and_both_entropy_paths(mjx):
    """1 x 1 x 4 at 520 x 264 = 65 x 33 MCUs, more than the 2048 of a DC segment, K swinging by +-90 from block to block so that its
    running sum crosses the segment with large differences of both signs; noisy at quality 95, so that the scan is longer than one
    entropy workgroup holds (512 lanes x 512 bytes) -- and short enough to fill one 256-lane workgroup with long subsequences, which
    is what takes a picture that is alone in its batch to the emitting pass (a context with the throughput plan).  Through that pass
    and, with MJX_SINGLE_DECODE=0, through the two-pass kernels; both byte for byte the twins' composition."""
    cf = make("cmyk", LAYOUTS4["1x1x4"], 520, 264, quality=95, seed=41, noise=12.0, k_swing=90.0)
    yk = make("ycck", LAYOUTS4["h2_k2"], 520, 264, quality=95, seed=42, noise=28.0, k_swing=90.0)
    for c in (cf, yk):
        assert c.mcux * c.mcuy > (2048 if c is cf else 1024) and 512 * 512 < len(c.entropy) <= 256 * 1280, len(c.entropy)
    cases = [("cmyk", cf), ("ycck", yk)]
    emits = []
    old = os.environ.get("MJX_SINGLE_DECODE")
    try:
        for env in (None, "0"):
            os.environ.pop("MJX_SINGLE_DECODE", None)
            if env is not None:
                os.environ["MJX_SINGLE_DECODE"] = env
            ctx = mjx.Context(0, profiling=True, throughput_plan=True)       # (the switch is read when the context is created)
            try:
                want = expectations(mjx, ctx, cases)
                for (model, c), w in zip(cases, want):
                    scan = mjx.ParsedScan(c.data, color="file")
                    b = mjx.Batch(ctx, [scan], color="file")                   # (alone: see above)
                    try:
                        b.decode(); b.wait()
                        assert b.status(0) == mjx.OK
                        emits.append(b.kernel_ms()["huff_emit"][1])
                        check_equal([b.rgb(0)], [w], ["%s single_decode %s" % (model, env)])
                    finally:
                        b.close()
                        scan.close()
            finally:
                ctx.close()
    finally:
        os.environ.pop("MJX_SINGLE_DECODE", None)
        if old is not None:
            os.environ["MJX_SINGLE_DECODE"] = old
    print("huff_emit launches:", emits)
    assert emits[0] > 0 and emits[1] > 0 and emits[2:] == [0, 0], emits


def test_restart_intervals_that_do_not_divide_the_mcu_row(mjx, gpu_ctx):
    cases = [("cmyk", make("cmyk", LAYOUTS4["h2_k2"], 37, 29, seed=51, restart=2)),          # 3 MCUs per row
             ("ycck", make("ycck", LAYOUTS4["1x1x4"], 37, 29, seed=52, restart=3)),          # 5 MCUs per row
             ("cmyk", make("cmyk", LAYOUTS4["y22_k22"], 100, 60, seed=53, restart=5)),       # 7 MCUs per row
             ("rgb", make("rgb", LAYOUTS3["420"], 37, 29, seed=54, restart=2))]
    assert all(cf.mcux % r for (_, cf), r in zip(cases, (2, 3, 5, 2)))
    want = expectations(mjx, gpu_ctx, cases)
    tags = ["h2_k2 dri 2", "1x1x4 dri 3", "y22_k22 dri 5", "rgb 420 dri 2"]
    for dd in (False, True):
        fb, st = mjx.decode_batch(gpu_ctx, [cf.data for _, cf in cases], device_destuff=dd, color="file")
        try:
            assert st == [mjx.OK] * len(cases), st
            check_equal([fb.rgb(i) for i in range(len(cases))], want, ["%s destuff %s" % (t, dd) for t in tags])
        finally:
            fb.close()


# ---- composition with everything behind stage B -----------------------------------------------------------------------------------------
W, H = 61, 45


@pytest.fixture(scope="module")
def trio(mjx, gpu_ctx):
    """One CMYK, one YCCK and one RGB picture of one size, and their packed pictures at every scale (computed once, left unchanged)."""
    cases = [("cmyk", make("cmyk", LAYOUTS4["y22_k22"], W, H, quality=90, seed=61, noise=8.0)),
             ("ycck", make("ycck", LAYOUTS4["h2_k2"], W, H, quality=90, seed=62, noise=8.0)),
             ("rgb", make("rgb", LAYOUTS3["420"], W, H, quality=90, seed=63, noise=8.0))]
    packed = {s: expectations(mjx, gpu_ctx, cases, scale=s) for s in (1, 2, 4, 8)}
    for v in packed.values():
        for a in v:
            a.setflags(write=False)
    return [cf.data for _, cf in cases], packed


def crop(a, r):
    x, y, w, h = r
    return a[y:y + h, x:x + w]


def test_rectangles_and_scales(mjx, gpu_ctx, trio):
    datas, packed = trio
    for s in (1, 2, 4, 8):
        ow, oh = -(-W // s), -(-H // s)
        rects = [None, (0, 0, 1, 1), (ow - 1, oh - 1, 1, 1), (ow - 1, 0, 1, 1), (0, oh - 1, 1, 1)]
        rects += [(5, 3, 17, 11), (13, 9, 30, 20), (15, 0, 3, oh)] if s == 1 else [(1, 1, ow - 2, oh - 3), (ow // 2, oh // 3, 3, 2)]
        for r in rects:
            got = decode_all(mjx, gpu_ctx, datas, color="file", scale=s, rois=r)
            want = [p if r is None else crop(p, r) for p in packed[s]]
            check_equal(got, want, [("scale", s, "rect", r, m) for m in ("cmyk", "ycck", "rgb")])
    # a rectangle per picture
    rois = [(3, 5, 20, 9), None, (40, 30, 21, 15)]
    got = decode_all(mjx, gpu_ctx, datas, color="file", rois=rois)
    check_equal(got, [p if r is None else crop(p, r) for p, r in zip(packed[1], rois)], ["cmyk", "ycck", "rgb"])


def run_out(mjx, ctx, datas, **kw):
    scans = [mjx.ParsedScan(d, color="file") for d in datas]
    b = mjx.Batch(ctx, scans, color="file", **kw)
    try:
        b.decode(); b.wait()
        assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas)
        return [b.output(i) for i in range(len(datas))]
    finally:
        b.close()
        for s in scans:
            s.close()


def test_output_formats_are_the_table_on_the_packed_bytes(mjx, gpu_ctx, trio):
    datas, packed = trio
    fmts = [mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD), mjx.Output("uint8", planar=False, bgr=True)]
    for fmt in fmts:
        for s, r in ((1, None), (1, (7, 5, 33, 21)), (2, None), (8, (1, 1, 5, 4))):
            got = run_out(mjx, gpu_ctx, datas, output=fmt, scale=s, rois=r)
            for g, p, m in zip(got, packed[s], ("cmyk", "ycck", "rgb")):
                assert of.same_bits(g, of.expected(np.ascontiguousarray(p if r is None else crop(p, r)), fmt)), (fmt.dtype, s, r, m)


def test_resize_and_orientation(mjx, gpu_ctx, trio):
    datas, packed = trio
    fmt = mjx.Output("uint8")
    for filt, aa, target in (("bilinear", True, (24, 20)), ("bicubic", True, (24, 20)), ("bicubic", False, (70, 50))):
        rs = mjx.Resize(target[0], target[1], antialias=aa, filter=filt, auto_scale=False)
        got = run_out(mjx, gpu_ctx, datas, resize=rs)
        for g, p, m in zip(got, packed[1], ("cmyk", "ycck", "rgb")):
            bad, _, _ = trf.check(g, p, target, filt, aa, fmt)
            assert bad is None, (filt, aa, m, bad)
    # the library picks the scale: 61 x 45 -> 24 x 20 is decoded at 1/2, and the rule runs on that picture
    got = run_out(mjx, gpu_ctx, datas, resize=mjx.Resize(24, 20, antialias=True, auto_scale=True))
    for g, p, m in zip(got, packed[2], ("cmyk", "ycck", "rgb")):
        bad, _, _ = trf.check(g, p, (24, 20), "bilinear", True, fmt)
        assert bad is None, ("auto scale", m, bad)
    # a rectangle, then the resize: the rule on the crop
    r = (9, 6, 40, 30)
    got = run_out(mjx, gpu_ctx, datas, resize=mjx.Resize(16, 12, antialias=True, auto_scale=False), rois=r)
    for g, p, m in zip(got, packed[1], ("cmyk", "ycck", "rgb")):
        bad, _, _ = trf.check(g, crop(p, r), (16, 12), "bilinear", True, fmt)
        assert bad is None, (m, bad)
    # orientation code 6, whole pictures and a rectangle of the turned picture, in two formats
    for f in (mjx.Output("uint8"), mjx.Output("float32", planar=True, mean=0.5, std=0.25)):
        got = run_out(mjx, gpu_ctx, datas, orient=mjx.Orient(exif=False, extra=6), output=f)
        for g, p, m in zip(got, packed[1], ("cmyk", "ycck", "rgb")):
            assert of.same_bits(g, of.expected(np.ascontiguousarray(tor.orient_np(6, p)), f)), ("orient 6", m)
    r = (4, 7, 30, 41)                                   # (the turned picture is 45 x 61)
    got = run_out(mjx, gpu_ctx, datas, orient=mjx.Orient(exif=False, extra=6), rois=r)
    for g, p, m in zip(got, packed[1], ("cmyk", "ycck", "rgb")):
        assert of.same_bits(g, np.ascontiguousarray(crop(tor.orient_np(6, p), r))), ("orient 6 rect", m)
    # ... and turned, then resized
    got = run_out(mjx, gpu_ctx, datas, orient=mjx.Orient(exif=False, extra=6), resize=mjx.Resize(20, 24, antialias=True, auto_scale=False))
    for g, p, m in zip(got, packed[1], ("cmyk", "ycck", "rgb")):
        bad, _, _ = trf.check(g, np.ascontiguousarray(tor.orient_np(6, p)), (20, 24), "bilinear", True, fmt)
        assert bad is None, ("orient 6 resize", m, bad)


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    cases = [("cmyk", make("cmyk", LAYOUTS4["y22_k22"], W, H, quality=90, seed=61, noise=8.0)),
             ("ycck", make("ycck", LAYOUTS4["h2_k2"], W, H, quality=90, seed=62, noise=8.0)),
             ("rgb", make("rgb", LAYOUTS3["420"], W, H, quality=90, seed=63, noise=8.0))]
    datas = [cf.data for _, cf in cases]
    packed = expectations(mjx, ctx, cases)
    bad = []
    dev = torch.device("cuda", 0)
    out = torch.full((3, 3, H, W), float("nan"), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD, color="file")
    torch.cuda.synchronize()
    fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    got = out.cpu().numpy()
    for i in range(3):
        if st[i] != mjx.OK or not of.same_bits(np.ascontiguousarray(got[i]), of.expected(packed[i], fmt)):
            bad.append(("f32 planar", i, st[i]))
    u8 = torch.full((3, 12, 16, 3), 9, dtype=torch.uint8, device=dev)
    st = mjx.decode_into(ctx, datas, u8, resize=mjx.Resize(16, 12, antialias=True, auto_scale=False), color="file")
    torch.cuda.synchronize()
    got = u8.cpu().numpy()
    for i in range(3):
        msg, _, _ = trf.check(np.ascontiguousarray(got[i]), packed[i], (16, 12), "bilinear", True, mjx.Output("uint8"))
        if st[i] != mjx.OK or msg is not None:
            bad.append(("u8 resized", i, st[i], msg))
    # without the option the four-component files are refused, the three-component one is decoded as Y, Cb, Cr
    st = mjx.decode_into(ctx, datas, torch.zeros((3, 3, H, W), dtype=torch.uint8, device=dev))
    if st != [mjx.ERR_UNSUPPORTED_FORMAT, mjx.ERR_UNSUPPORTED_FORMAT, mjx.OK]:
        bad.append(("default", st))
    ctx.close()
    print(json.dumps({"bad": bad, "nbad": len(bad)}))


def test_decode_into_a_torch_tensor(mjx, tmp_path):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_color_decode as t\nt.child_torch()\n" % (ROOT, ROOT))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["nbad"] == 0, res


# ---- front doors, a mixed call, refusals, a damaged file --------------------------------------------------------------------------------
def _read(*p):
    with open(os.path.join(ROOT, "tests", *p), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def mixed(mjx, gpu_ctx, trio):
    """grey, 4:2:0 YCbCr, CMYK, YCCK, RGB and a progressive file; what the last three models decode to."""
    datas, packed = trio
    files = [mjx.synth_jpeg(48, 40, "gray", 80, seed=3), mjx.synth_jpeg(70, 52, "420", 80, seed=4)] + list(datas) + [_read("golden", "pil", "progressive.jpg")]
    return files, list(packed[1])


def test_front_doors_and_a_mixed_call(mjx, gpu_ctx, mixed):
    files, packed = mixed
    n = len(files)
    plain, st0 = mjx.decode_batch(gpu_ctx, files)                               # color unset
    try:
        assert st0[:2] == [mjx.OK, mjx.OK] and st0[2:4] == [mjx.ERR_UNSUPPORTED_FORMAT] * 2 and st0[4] == mjx.OK and st0[5] != mjx.OK, st0
        grey, ycc, rgb_as_ycc = plain.rgb(0), plain.rgb(1), plain.rgb(4)
        assert [plain.color_model(i) for i in (0, 1, 4)] == [mjx.MODEL_GREY, mjx.MODEL_YCBCR, mjx.MODEL_YCBCR]
    finally:
        plain.close()
    assert not np.array_equal(rgb_as_ycc, packed[2])                           # (the wrong colours the default gives such a file)
    want = [grey, ycc] + packed
    for dd in (False, True, None):                                              # the pipelined call, host and device de-stuffing
        fb, st = mjx.decode_batch(gpu_ctx, files, device_destuff=dd, color="file", threads=2)
        try:
            assert st[:5] == [mjx.OK] * 5 and st[5] == st0[5], st
            assert [fb.color_model(i) for i in range(5)] == [mjx.MODEL_GREY, mjx.MODEL_YCBCR, mjx.MODEL_CMYK, mjx.MODEL_YCCK, mjx.MODEL_RGB]
            check_equal([fb.rgb(i) for i in range(5)], want, ["grey", "ycbcr", "cmyk", "ycck", "rgb"])
        finally:
            fb.close()
    # Batch over parsed scans (the progressive file does not parse), one picture per chunk as well
    for ci in (0, 1):
        got = decode_all(mjx, gpu_ctx, files[:5], color="file", chunk_images=ci)
        check_equal(got, want, ["grey", "ycbcr", "cmyk", "ycck", "rgb"])
    # JPEGImage.parse, one file at a time
    for d, w in zip(files[:5], want):
        img = mjx.JPEGImage.parse(d, ctx=gpu_ctx, color="file")
        assert (img.width(), img.height()) == (w.shape[1], w.shape[0]) and np.array_equal(np.asarray(img.image_data()).reshape(w.shape), w)
    with pytest.raises(mjx.MjxError) as e:
        mjx.JPEGImage.parse(files[2], ctx=gpu_ctx)
    assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT
    # the pool
    pool = mjx.Pool([0])
    try:
        res = pool.decode_batch(files, color="file")
        try:
            assert list(res.status)[:5] == [mjx.OK] * 5 and res.status[5] == st0[5]
            check_equal([res.rgb(i) for i in range(5)], want, ["grey", "ycbcr", "cmyk", "ycck", "rgb"])
        finally:
            res.close()
        res = pool.decode_batch(files)
        try:
            assert list(res.status) == st0
        finally:
            res.close()
    finally:
        pool.close()


def test_refusals_are_per_picture(mjx, gpu_ctx, mixed):
    """Luminance output, planes and libjpeg's pixels refuse the RGB, CMYK and YCCK pictures with MJX_ERR_UNSUPPORTED_FORMAT; the grey and
    the YCbCr picture of the same call decode to what the call gives them without the option."""
    files, _ = mixed
    files = files[:5]
    U = mjx.ERR_UNSUPPORTED_FORMAT
    for kw in (dict(output=mjx.Output("uint8", channels=1)), dict(planes=mjx.Planes()), dict(pixels="libjpeg")):
        ref, st_ref = mjx.decode_batch(gpu_ctx, files[:2], **kw)
        fb, st = mjx.decode_batch(gpu_ctx, files, color="file", **kw)
        try:
            assert st_ref == [mjx.OK] * 2 and st == [mjx.OK, mjx.OK, U, U, U], (list(kw), st)
            for i in range(2):
                if "planes" in kw:
                    a, b = fb.planes(i), ref.planes(i)
                    assert len(a) == len(b) and all(of.same_bits(x, y) for x, y in zip(a, b))
                elif "output" in kw:
                    assert of.same_bits(fb.output(i), ref.output(i))
                else:
                    assert np.array_equal(fb.rgb(i), ref.rgb(i))
        finally:
            fb.close()
            ref.close()
        scans = [mjx.ParsedScan(d, color="file") for d in files]
        b = mjx.Batch(gpu_ctx, scans, color="file", **kw)
        try:
            assert b.create_status == [mjx.OK, mjx.OK, U, U, U]
        finally:
            b.close()
            for s in scans:
                s.close()


def test_a_scan_cut_in_its_last_mcu_is_truncated(mjx, gpu_ctx):
    cf = make("cmyk", LAYOUTS4["h2_k2"], 64, 48, quality=95, seed=71, noise=25.0)
    ok = make("ycck", LAYOUTS4["1x1x4"], 37, 29, seed=72)
    want = expectations(mjx, gpu_ctx, [("cmyk", cf), ("ycck", ok)])
    cut = cw.cut_in_last_mcu(cf)
    for dd in (False, True):
        fb, st = mjx.decode_batch(gpu_ctx, [cut, ok.data, cf.data], device_destuff=dd, color="file")
        try:
            assert st == [mjx.ERR_TRUNCATED, mjx.OK, mjx.OK], st
            check_equal([fb.rgb(1), fb.rgb(2)], [want[1], want[0]], ["intact ycck", "intact cmyk"])
        finally:
            fb.close()


# ---- against Pillow (independent, not exact: libjpeg's integer IDCT differs from this float one) -------------------------------------------
def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_grey(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def pillow_cmyk(w, h, subsampling, seed):
    """A CMYK file written by Pillow (quality 90): smooth inks plus noise."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([128 + 90 * np.sin(0.07 * (k + 1) * xx + 0.05 * (4 - k) * yy + k) + rng.normal(0, 4, (h, w)) for k in range(4)], axis=-1)
    buf = io.BytesIO()
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), "CMYK").save(buf, "JPEG", quality=90, subsampling=subsampling)
    return buf.getvalue()


def test_against_pillow_within_the_twins_own_differences(mjx, gpu_ctx):
    """ink_mul is 1-Lipschitz in each argument up to its rounding, so a picture may differ from Pillow's by d3 + dK + 1, d3 and dK being
    the largest differences between this decoder's and Pillow's bytes of the components: measured on the twins -- for CMYK the
    one-component twins of components 0 .. 2 and of K, for YCCK the three-component twin and K's.  Two files are Pillow's own (quality
    90, subsampling 0 and 2; their coefficients are read back by colorwriter.read_baseline to build the twins), the YCCK file is
    constructed.
    Pillow's subsampling=2 writes C at full resolution and M, Y, K at half in both directions, and libjpeg brings those up with its
    triangle filter where this decoder replicates (mjx.h: box replication; libjpeg's pixels are refused for these models).  That is a
    difference of the two rules, not of the decoders, and it is known from Pillow's own planes: u_c = the largest difference between
    libjpeg's upsampling (mjx.upsample_luma_host, the routine of pixels="libjpeg", pinned against libjpeg by
    tests/test_libjpeg_pixels.py) and the replication of Pillow's decode of twin c.  A component's byte then differs by at most
    d_c + u_c, and the bound is max_c (d_c + u_c) + (d_K + u_K) + 1; without subsampling every u is 0 and it is d3 + dK + 1.
    Measured on an MI355X (d of C, M, Y, K; u; the picture's largest difference; the bound) -- see DESIGN.md s23."""
    files = [("cmyk", cw.read_baseline(pillow_cmyk(96, 64, 0, 1))), ("cmyk", cw.read_baseline(pillow_cmyk(90, 61, 2, 2))),
             ("ycck", make("ycck", LAYOUTS4["1x1x4"], 96, 64, quality=90, seed=83, noise=5.0))]
    assert mjx.color_model(files[0][1].data)["name"] == "cmyk" and len(files[1][1].hv) == 4 and files[1][1].hmax == 2
    got = decode_all(mjx, gpu_ctx, [cf.data for _, cf in files], color="file")
    for (model, cf), g in zip(files, got):
        twins = [cw.component_twin(cf, c) for c in range(4)]
        mine = decode_all(mjx, gpu_ctx, twins)
        theirs = [pil_grey(t) for t in twins]
        d = [int(np.abs(m[..., 0].astype(int) - t.astype(int)).max()) for m, t in zip(mine, theirs)]
        u = []
        for t, (h, v) in zip(theirs, cf.hv):
            rh, rv = cf.hmax // h, cf.vmax // v
            if rh == 1 and rv == 1:
                u.append(0)
                continue
            fancy = mjx.upsample_luma_host(t, rh, rv, (0, 0, cf.width, cf.height))
            u.append(int(np.abs(fancy.astype(int) - cw.replicate(t, h, v, cf.hmax, cf.vmax, cf.width, cf.height).astype(int)).max()))
        if model == "ycck":
            t3 = cw.ycc_twin(cf)
            d3 = int(np.abs(decode_all(mjx, gpu_ctx, [t3])[0].astype(int) - pil_rgb(cw.with_head(t3, cw.app0())).astype(int)).max())
            assert u == [0, 0, 0, 0]
        else:
            d3 = max(dc + uc for dc, uc in zip(d[:3], u[:3]))
        bound = d3 + d[3] + u[3] + 1
        diff = int(np.abs(g.astype(int) - pil_rgb(cf.data).astype(int)).max())
        print("against Pillow: %s %s d = %s, u = %s, d3 = %d, picture = %d (bound %d)" % (model, cf.hv, d, u, d3, diff, bound))
        assert diff <= bound, (model, cf.hv, diff, d, u, bound)

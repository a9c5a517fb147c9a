"""libjpeg's pixels (mjx_opts.pixels = MJX_PIXELS_LIBJPEG, include/mjx.h): rounded samples, fancy chroma upsampling, integer colour.

The reference is tests/libjpeg_ref.py, a numpy restatement of the contract on float64 samples from the oracle's coefficients.
  CPU  the reference is libjpeg's (Pillow, within the error of libjpeg's integer IDCT: max 3, 1 % of bytes more than 1 off, 5 % off
       at all -- measured for the reference alone: 3, 0.83 %, 4.0 %); the routine the kernel and the host share
       (mjx_upsample_color_host) is the reference's integer steps bit for bit; the refusals.
  GPU  every byte lies in the interval float64 allows (libjpeg_ref.interval, K = 64) and at most 2 % of a picture's bytes have an
       interval of more than one value (measured for the reference alone: <= 0.57 % over the layouts at 61 x 45, 1.3 % on
       2x2-chroma.jpeg); every stream source, rectangle, output format, resize, orientation and front door gives the bytes of the
       plain pixels = 1 decode; Pillow end to end; the default is untouched.
"""
import io
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import libjpeg_ref as lj
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_sampling_layouts as tsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_DIR = os.path.join(ROOT, "tests", "golden", "pil")
DATA_DIR = os.path.join(ROOT, "tests", "data")
NAMES = tsl.NAMES
PIL_NAMES = [n for n in NAMES if n != "Y22_Cb22_Cr22"]                  # (Pillow refuses the 12-block MCU)
CPU_SIZES = [(61, 45), (40, 24)]
CPU_FILES = [os.path.join(DATA_DIR, "lena.jpeg"), os.path.join(DATA_DIR, "2x2-chroma.jpeg"), os.path.join(PIL_DIR, "std_420_big.jpg"),
             os.path.join(PIL_DIR, "opt_422_q95.jpg"), os.path.join(PIL_DIR, "opt_444_q40.jpg"), os.path.join(PIL_DIR, "opt_gray_q70.jpg")]
PILLOW_GPU_FILES = CPU_FILES[:3]
Y420, Y422, Y440, LUMA_SUB = "Y22_Cb11_Cr11", "Y21_Cb11_Cr11", "Y12_Cb11_Cr11", "Y11_Cb22_Cr21"


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def q85(n, w, h):
    return tsl.data_of(n, w, h, quality=85)


def diff_figures(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int(d.max()), float((d > 1).mean()), float((d > 0).mean())


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", CPU_SIZES)
def test_the_reference_is_libjpegs_on_every_layout(orc, size):
    w, h = size
    bad, worst = [], [0, 0.0, 0.0]
    for n in PIL_NAMES:
        data = q85(n, w, h)
        mx, off1, off0 = diff_figures(lj.libjpeg_pixels(data, tsl.oracle_std(data)), pillow(data))
        worst = [max(worst[0], mx), max(worst[1], off1), max(worst[2], off0)]
        if mx > 3 or off1 > 0.01 or off0 > 0.05:
            bad.append((n, mx, off1, off0))
    print("worst over the layouts at %d x %d: max %d, more than 1 off %.4f, off at all %.4f" % (w, h, *worst))
    assert bad == [], bad
    with pytest.raises(OSError):
        pillow(q85("Y22_Cb22_Cr22", w, h))


@pytest.mark.parametrize("path", CPU_FILES, ids=os.path.basename)
def test_the_reference_is_libjpegs_on_files(orc, path):
    data = _read(path)
    mx, off1, off0 = diff_figures(lj.libjpeg_pixels(data), pillow(data))
    print("%s: max %d, more than 1 off %.4f, off at all %.4f" % (os.path.basename(path), mx, off1, off0))
    assert mx <= 3 and off1 <= 0.01 and off0 <= 0.05, (mx, off1, off0)


HV = [(1, 1), (2, 1), (1, 2), (2, 2)]
PLANE_DIMS = (1, 2, 3, 8, 9, 17)


def _host_case(mjx, planes, hv, rect=None):
    """planes of the components' true sizes for factors hv -> (host routine, numpy) on `rect` of the picture they cover"""
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    ratios = [(hmax // h, vmax // v) for h, v in hv]
    W = min(p.shape[1] * rh for p, (rh, _) in zip(planes, ratios))
    H = min(p.shape[0] * rv for p, (_, rv) in zip(planes, ratios))
    x, y, w, h = rect or (0, 0, W, H)
    want = lj.pixels_from_planes([p.astype(np.int32) for p in planes], ratios, W, H)[y:y + h, x:x + w]
    got = mjx.upsample_color_host(planes, [r[0] for r in ratios], [r[1] for r in ratios], (x, y, w, h))
    return got, want, (W, H)


def _planes_for(hv, W, H, fill):
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    return [fill((-(-H * v // vmax), -(-W * h // hmax))) for h, v in hv]


def test_the_shared_routine_is_the_reference_bit_for_bit(mjx):
    rng = np.random.default_rng(5)
    rand = lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)
    bad = []
    # all 64 factor combinations, random planes, picture sizes whose planes are 1, 2, 3, 8, 9 and 17 wide and high
    for hv in itertools.product(HV, repeat=3):
        hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
        for k, d in enumerate(PLANE_DIMS):
            W, H = d * hmax - (k % 2) * (hmax - 1), PLANE_DIMS[(k + 2) % 6] * vmax - ((k // 2) % 2) * (vmax - 1)
            planes = _planes_for(hv, W, H, rand)
            got, want, _ = _host_case(mjx, planes, hv)
            if not np.array_equal(got, want):
                bad.append(("random", hv, W, H))
    # plane widths and heights themselves, one component subsampled both ways against a full-size one
    for cw in PLANE_DIMS:
        for ch in PLANE_DIMS:
            for hv in ([(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (2, 1)], [(1, 2), (1, 2), (1, 1)], [(1, 1), (2, 2), (2, 2)]):
                planes = _planes_for(hv, cw * 2, ch * 2, rand)
                got, want, _ = _host_case(mjx, planes, hv)
                if not np.array_equal(got, want):
                    bad.append(("dims", hv, cw, ch))
    # both clamps of every channel: all 0, all 255, checkerboards of 0 and 255 per component
    yy, xx = np.mgrid[0:18, 0:34]
    board = lambda shape, ph: (((yy[:shape[0], :shape[1]] + xx[:shape[0], :shape[1]] + ph) & 1) * 255).astype(np.uint8)
    for hv in ([(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)], [(2, 1), (1, 2), (1, 1)]):
        fills = [lambda s: np.zeros(s, np.uint8), lambda s: np.full(s, 255, np.uint8), lambda s: board(s, 0), lambda s: board(s, 1)]
        for fy, fb, fr in itertools.product(fills, repeat=3):
            shapes = _planes_for(hv, 33, 17, lambda s: s)
            planes = [f(s) for f, s in zip((fy, fb, fr), shapes)]
            got, want, _ = _host_case(mjx, planes, hv)
            if not np.array_equal(got, want):
                bad.append(("clamps", hv))
    # (these fills reach both clamps of every channel: before clamping R and B of (255, 255, 255) lie above 255 and of (0, 0, 0) below 0,
    # G of (255, 0, 0) above and of (0, 255, 255) below)
    assert 255 + ((lj.fix(1.402) * 127 + 32768) >> 16) > 255 > 0 > ((lj.fix(1.772) * -128 + 32768) >> 16)
    assert 255 + ((lj.fix(0.34414) * 128 + 32768 + lj.fix(0.71414) * 128) >> 16) > 255 > 0 > ((-lj.fix(0.34414) * 127 + 32768 - lj.fix(0.71414) * 127) >> 16)
    # rectangles: 1 x 1 at every corner and at odd and even origins, strips, the whole
    for hv in ([(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(1, 1), (2, 2), (2, 1)]):
        W, H = 29, 19
        planes = _planes_for(hv, W, H, rand)
        rects = [(x, y, 1, 1) for x in (0, 1, 2, 7, 8, 9, 15, 16, W - 2, W - 1) for y in (0, 1, 2, 7, 8, H - 2, H - 1)]
        rects += [(0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H), (3, 5, 11, 7), (4, 6, 9, 8), (0, 0, W, H)]
        for r in rects:
            got, want, _ = _host_case(mjx, planes, hv, r)
            if not np.array_equal(got, want):
                bad.append(("rect", hv, r))
    # one component: R = G = B = the sample
    g = rand((9, 17))
    got = mjx.upsample_color_host([g], [1], [1], (0, 0, 17, 9))
    if not np.array_equal(got, np.repeat(g[:, :, None], 3, axis=2)):
        bad.append("grey")
    assert bad == [], bad[:10]
    # a rectangle outside the planes is refused
    with pytest.raises(mjx.MjxError):
        mjx.upsample_color_host([g], [1], [1], (10, 0, 8, 9))


def test_refusals_through_validate_and_the_auto_scale_rule(mjx):
    data = tsl.data_of(Y420, 333, 217)
    scan = mjx.ParsedScan(data)
    try:
        assert scan.validate(pixels="libjpeg") == mjx.OK
        assert scan.validate(pixels=mjx.PIXELS_LIBJPEG, roi=(3, 5, 100, 70)) == mjx.OK
        assert scan.validate(pixels="libjpeg", layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_INVALID_ARG
        assert scan.validate(pixels="libjpeg", strict_ref=True) == mjx.ERR_INVALID_ARG
        for s in (2, 4, 8):
            assert scan.validate(pixels="libjpeg", scale=s) == mjx.ERR_INVALID_ARG, s
            assert scan.validate(scale=s) == mjx.OK
        assert scan.validate(pixels=2) == mjx.ERR_INVALID_ARG
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT) in (mjx.OK, mjx.ERR_REF_PANIC)          # (the default's refusals are its own)
        # auto_scale picks scale 1 and keeps the rectangle; without the option the same call picks 1/8
        rs = mjx.Resize(40, 24, auto_scale=True)
        assert scan.resize_plan(rs)["scale"] == 8
        plan = scan.resize_plan(rs, pixels="libjpeg")
        assert plan["scale"] == 1 and plan["rect"] == (0, 0, 333, 217), plan
        plan = scan.resize_plan(rs, roi=(10, 20, 300, 190), pixels="libjpeg")
        assert plan["scale"] == 1 and plan["rect"] == (10, 20, 300, 190), plan
        # the tiles of an interior rectangle: fewer than the picture's, and never fewer than the default pixels read for it
        whole = scan.plan_tiles(pixels="libjpeg")
        assert whole["tiles_read"] == whole["tiles_total"] == scan.plan_tiles()["tiles_total"] and whole["tile_mcus"] == 32
        inner, plain = scan.plan_tiles(roi=(100, 80, 40, 30), pixels="libjpeg"), scan.plan_tiles(roi=(100, 80, 40, 30))
        assert plain["tiles_read"] <= inner["tiles_read"] < inner["tiles_total"], (inner, plain)
        # a rectangle whose first row is an MCU's first row reaches into the MCU row above it
        edge, edge_plain = scan.plan_tiles(roi=(0, 32, 333, 16), pixels="libjpeg"), scan.plan_tiles(roi=(0, 32, 333, 16))
        assert edge["tiles_read"] > edge_plain["tiles_read"], (edge, edge_plain)
    finally:
        scan.close()


def test_the_option_is_mirrored_everywhere(mjx):
    hdr = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    body = re.search(r"typedef struct mjx_opts\s*\{(.*?)\}\s*mjx_opts;", hdr, flags=re.S).group(1)
    c_fields = [re.sub(r".*[\s\*]", "", d.strip()) for d in body.split(";") if d.strip()]
    assert "pixels" in c_fields and c_fields == [f[0] for f in mjx.Opts._fields_], c_fields
    assert re.search(r"MJX_PIXELS_REFERENCE = 0", hdr) and re.search(r"MJX_PIXELS_LIBJPEG = 1", hdr)
    assert (mjx.PIXELS_REFERENCE, mjx.PIXELS_LIBJPEG) == (0, 1)
    # the layout change is marked: the header's number, its mirrors and what the built library says of itself
    abi = int(re.search(r"#define MJX_ABI_VERSION (\d+)", hdr).group(1))
    assert abi == 2 == mjx.ABI_VERSION and ("abi=%d " % abi).encode() in mjx.lib().mjx_version()
    import ctypes
    assert ctypes.sizeof(mjx.Opts) == 32 and mjx.Opts.rois.offset == 16 and mjx.Opts.pixels.size == 1     # (the struct's size is as it was)
    assert mjx._opts().pixels == 0 and mjx._opts(pixels="libjpeg").pixels == 1 and mjx._opts(pixels="reference").pixels == 0
    with pytest.raises(mjx.MjxError):
        mjx._opts(pixels="fancy")
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    rbody = re.search(r"pub struct mjx_opts\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", rbody) == c_fields
    assert "pub const MJX_ABI_VERSION: u32 = 2;" in rs
    assert "pub fn mjx_upsample_color_host(" in rs and "mjx_upsample_color_host" in mjx.SYMBOLS
    assert "--libjpeg-pixels" in _read(os.path.join(ROOT, "jpeg-rust_amd", "csrc", "mjx_cli.cpp")).decode()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def lj_decode(mjx, ctx, datas, **kw):
    """-> [picture or ('status', code)] of a pixels = libjpeg Batch of parsed scans"""
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, pixels="libjpeg", **kw)
    try:
        b.decode()
        b.wait()
        return [b.rgb(i) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


def interval_problem(got, data):
    """None when every byte of `got` lies in the interval float64 allows and at most 2 % of them have a choice, else what is wrong"""
    lo, hi = lj.interval(data, 64, tsl.oracle_std(data))
    if not isinstance(got, np.ndarray) or got.shape != lo.shape:
        return ("shape or status", got if not isinstance(got, np.ndarray) else got.shape, lo.shape)
    share = float((lo != hi).mean())
    out = (got < lo) | (got > hi)
    if out.any() or share > 0.02:
        return ("outside %d of %d, first at %s; undecided share %.4f" % (int(out.sum()), out.size, np.argwhere(out)[:2].tolist(), share))
    return None


F64_GROUPS = {
    "layouts_61x45": [(n, 61, 45) for n in NAMES],
    "layouts_333x217": [(n, 333, 217) for n in NAMES],
    # 4:2:0 at 1035 x 490: 63 tiles, so four workgroups, tiles that wrap MCU rows, an odd width; the smallest 4:2:0 pictures; grey
    "420_and_grey": [(Y420, 1035, 490), (Y420, 17, 9), (Y420, 16, 16), ("gray22", 61, 45), ("gray12", 333, 217)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(F64_GROUPS))
def test_every_byte_lies_in_the_interval_float64_allows(mjx, gpu_ctx, group):
    cases = F64_GROUPS[group]
    datas = [tsl.data_of(n, w, h) for n, w, h in cases]
    got = lj_decode(mjx, gpu_ctx, datas)
    bad = []
    for c, d, g in zip(cases, datas, got):
        p = interval_problem(g, d)
        if p:
            bad.append((c, p))
    alone = lj_decode(mjx, gpu_ctx, datas[:1])                        # (a batch of one: the latency plan's cut of the scan)
    if not tsl.same(alone[0], got[0]):
        bad.append((cases[0], "alone"))
    assert bad == [], bad[:6]


STREAM_CASES = [(Y420, 1000, 40), (Y420, 333, 217), (LUMA_SUB, 1000, 40), (Y422, 61, 45)]


def stream_files():
    """[(name, bytes, index of the interleaved file it must equal)]: per case the interleaved file, two multi-scan script twins and
    a restart-interval twin.  At 1000 x 40 stage B reads a twin straight from its scans' streams, at 333 x 217 through the gather."""
    out = []
    for n, w, h in STREAM_CASES:
        d = tsl.data_of(n, w, h)
        base = len(out)
        out.append(("%s_%dx%d" % (n, w, h), d, base))
        ref = tsl.oracle_std(d)
        out.append(("Y;Cb;Cr", jw.script_twin(d, ref, "Y;Cb;Cr"), base))
        out.append(("Y;Cb Cr", jw.script_twin(d, ref, "Y;Cb Cr"), base))
        out.append(("dri3", tsl.data_of(n, w, h, restart=3), base))
    return out


def child_streams(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = stream_files()
    out, status = {}, {}
    for dd in (False, True):
        b, st = mjx.decode_batch(ctx, [d for _, d, _ in files], device_destuff=dd, pixels="libjpeg")
        for i in range(len(files)):
            status["%d_%d" % (i, dd)] = st[i] or b.status(i)
            if not status["%d_%d" % (i, dd)]:
                out["%d_%d" % (i, dd)] = b.rgb(i)
        b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=status)))


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_libjpeg_pixels as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_stream_source_gives_the_interleaved_files_bytes(mjx, gpu_ctx, tmp_path):
    files = stream_files()
    want = lj_decode(mjx, gpu_ctx, [d for _, d, _ in files])
    bad = [(files[i][0], "status", w) for i, w in enumerate(want) if not isinstance(w, np.ndarray)]
    bad += [(files[b][0], n, "in process") for i, (n, _, b) in enumerate(files) if not tsl.same(want[i], want[b])]
    # which twins stage B read straight from their scans: those at 1000 x 40, none at 333 x 217 (a batch of one, its chunk resident)
    direct = {}
    for i, (n, d, b) in enumerate(files):
        if ";" in n:
            scans = [mjx.ParsedScan(d)]
            bt = mjx.Batch(gpu_ctx, scans, pixels="libjpeg")
            try:
                bt.decode()
                bt.wait()
                direct[i] = not tsl.coefs_expand(mjx, bt, 0)
                if not tsl.same(bt.rgb(0), want[b]):
                    bad.append((files[b][0], n, "alone"))
            finally:
                tsl.close_all(bt, scans)
    assert direct[1] and direct[2] and not direct[5] and not direct[6], direct
    for k, env in enumerate(({"MJX_SINGLE_DECODE": "0"}, {"MJX_STREAM_LINEAR": "1"}, {"MJX_PLANAR_DIRECT": "0"})):
        npz = tmp_path / ("streams%d.npz" % k)
        res = run_child(tmp_path, "child_streams(%r)" % str(npz), env)
        with np.load(str(npz)) as z:
            for i, (n, _, b) in enumerate(files):
                for dd in (0, 1):
                    key = "%d_%d" % (i, dd)
                    if res["status"][key] != 0 or not tsl.same(z[key], want[b]):
                        bad.append((files[b][0], n, sorted(env.items()), "device de-stuffing" if dd else "host de-stuffing", res["status"][key]))
    assert bad == [], bad[:8]


def rectangles(W, H, mw, mh):
    """unaligned rectangles with odd and even origins, 1 x 1 at the four corners, strips along each edge, one inside one MCU, one
    that ends on MCU borders, one interior"""
    r = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),
         (0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H), (0, 1, W, 2), (1, 0, 2, H),
         (mw + 1, mh + 1, mw - 2, mh - 2), (mw, mh, mw, mh), (2 * mw, mh, 3 * mw, 2 * mh),
         (3, 5, W - 7, H - 11), (4, 6, W - 9, H - 12), (mw - 1, mh - 1, 2, 2), (mw, mh - 1, 5, 3), (7, 2 * mh, 9, 1), (W // 2, H // 2, 41, 37)]
    return [q for q in r if q[0] + q[2] <= W and q[1] + q[3] <= H and q[2] > 0 and q[3] > 0]


@pytest.mark.gpu
@pytest.mark.parametrize("lname", [Y420, Y422, Y440, LUMA_SUB])
def test_rectangles_are_the_crop_of_the_uncropped_decode(mjx, gpu_ctx, lname):
    bad = []
    for W, H in ((333, 217), (61, 45)):
        data = tsl.data_of(lname, W, H)
        full = lj_decode(mjx, gpu_ctx, [data])[0]
        assert isinstance(full, np.ndarray) and full.shape == (H, W, 3)
        hv = tsl.parse_name(lname)
        rects = rectangles(W, H, 8 * max(h for h, _ in hv), 8 * max(v for _, v in hv))
        got = lj_decode(mjx, gpu_ctx, [data] * len(rects), rois=rects)
        for (x, y, w, h), g in zip(rects, got):
            if not tsl.same(g, full[y:y + h, x:x + w]):
                bad.append((W, H, (x, y, w, h), g if not isinstance(g, np.ndarray) else int((g != full[y:y + h, x:x + w]).sum())))
        one = lj_decode(mjx, gpu_ctx, [data], rois=[rects[-1]])[0]
        if not tsl.same(one, got[-1]):
            bad.append((W, H, "alone"))
    assert bad == [], bad[:8]
    tiles = mjx.plan_tiles(tsl.data_of(lname, 333, 217), roi=(120, 90, 40, 30), pixels="libjpeg")
    assert tiles["tiles_read"] < tiles["tiles_total"], tiles


FMT_FILES = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 333, 217)]


@pytest.mark.gpu
def test_output_formats_are_the_table_on_the_packed_decode(mjx, gpu_ctx):
    datas = [tsl.data_of(*c) for c in FMT_FILES]
    rois = [None, (3, 5, 40, 30), None, (101, 50, 99, 77)]
    packed = lj_decode(mjx, gpu_ctx, datas, rois=rois)
    assert all(isinstance(p, np.ndarray) for p in packed), packed
    bad = []
    for k in range(12):
        fmt = tof.make_format(mjx, k)
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, rois=rois, output=fmt, pixels="libjpeg")
        try:
            b.decode()
            b.wait()
            for i in range(len(datas)):
                if b.status(i) != mjx.OK or not tof.same_bits(b.output(i), tof.expected(packed[i], fmt)):
                    bad.append((tof.FORMATS[k], FMT_FILES[i], b.status(i)))
        finally:
            tsl.close_all(b, scans)
    assert bad == [], bad[:8]


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    datas = [tsl.data_of(*c) for c in FMT_FILES]
    rois = [(11, 7, 48, 36), (3, 5, 48, 36), (0, 9, 48, 36), (101, 50, 48, 36)]
    ref, _ = mjx.decode_batch(ctx, datas, rois=rois, pixels="libjpeg")
    packed = [ref.rgb(i) for i in range(len(datas))]
    ref.close()
    dev, n = torch.device("cuda", 0), len(datas)
    # float16 planar with mean and std, rows padded; uint8 interleaved B,G,R, rows padded; float32 planar
    big = torch.full((n, 3, 36, 56), float("nan"), dtype=torch.float16, device=dev)
    st = mjx.decode_into(ctx, datas, big[:, :, :, 4:52], rois=rois, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD, pixels="libjpeg")
    torch.cuda.synchronize()
    fmt = mjx.Output("float16", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD)
    got = big.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, :, 4:52]), tof.expected(packed[i], fmt)):
            bad.append(("f16 planar", i, st[i]))
    if not (np.isnan(got[:, :, :, :4]).all() and np.isnan(got[:, :, :, 52:]).all()):
        bad.append("the padding of the f16 rows was written")
    big8 = torch.full((n, 36, 54, 3), 7, dtype=torch.uint8, device=dev)
    st = mjx.decode_into(ctx, datas, big8[:, :, 3:51, :], rois=rois, bgr=True, pixels="libjpeg")
    torch.cuda.synchronize()
    fmt = mjx.Output("uint8", bgr=True)
    got = big8.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, 3:51, :]), tof.expected(packed[i], fmt)):
            bad.append(("u8 interleaved", i, st[i]))
    if not (np.all(got[:, :, :3, :] == 7) and np.all(got[:, :, 51:, :] == 7)):
        bad.append("the padding of the u8 rows was written")
    out32 = torch.zeros((n, 3, 36, 48), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out32, rois=rois, mean=0.5, std=0.25, pixels="libjpeg")
    torch.cuda.synchronize()
    fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(out32[i].cpu().numpy()), tof.expected(packed[i], fmt)):
            bad.append(("f32 planar", i, st[i]))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad)}))


@pytest.mark.gpu
def test_decode_into_a_torch_tensor_with_padded_pitches(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0, res


@pytest.mark.gpu
def test_resize_and_orientation_work_on_the_packed_intermediate(mjx, gpu_ctx):
    datas = [tsl.data_of(Y420, 333, 217), tsl.data_of(Y422, 333, 217)]
    roi = (10, 20, 300, 190)
    packed = lj_decode(mjx, gpu_ctx, datas, rois=roi)
    assert all(isinstance(p, np.ndarray) for p in packed)
    bad = []

    def run(fmt, **kw):
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, rois=roi, output=fmt, pixels="libjpeg", **kw)
        try:
            b.decode()
            b.wait()
            assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas)
            return [b.output(i) for i in range(len(datas))], [b.scale(i) for i in range(len(datas))]
        finally:
            tsl.close_all(b, scans)

    # resize (auto_scale on: scale 1 all the same): the existing rule on the intermediate, within the existing bound
    fmt = mjx.Output("float32", planar=True, mean=0.5, std=0.25)
    for aa in (True, False):
        rs = mjx.Resize(70, 37, antialias=aa, auto_scale=True)
        got, scales = run(fmt, resize=rs)
        assert scales == [1, 1], scales
        for i, g in enumerate(got):
            tx, ty = trs.max_taps(300, 70, aa), trs.max_taps(190, 37, aa)
            p, _, _ = trs.check_against(g, trs.resize_ref(packed[i], 70, 37, aa), fmt, trs.tolerance(tx, ty))
            if p:
                bad.append(("resize", aa, i, p))
    # orientation alone: the formats' table on the mapped byte, bit for bit (the rectangle is the turned picture's)
    fmt8, r = mjx.Output("uint8"), (5, 9, 120, 100)
    S = lj_decode(mjx, gpu_ctx, datas)
    for code in (2, 6, 7):
        got = run_orient(mjx, gpu_ctx, datas, fmt8, code, r)
        for i, g in enumerate(got):
            D = tor.orient_np(code, S[i])
            if not tof.same_bits(g, tof.expected(np.ascontiguousarray(D[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), fmt8)):
                bad.append(("orient", code, i))
    # combined: the rule on orient_c of the intermediate
    code, aa = 6, True
    D = [np.ascontiguousarray(tor.orient_np(code, s)[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]) for s in S]
    got = run_orient(mjx, gpu_ctx, datas, fmt, code, r, resize=mjx.Resize(33, 40, antialias=aa, auto_scale=True))
    for i, g in enumerate(got):
        tx, ty = trs.max_taps(120, 33, aa), trs.max_taps(100, 40, aa)
        p, _, _ = trs.check_against(g, trs.resize_ref(D[i], 33, 40, aa), fmt, trs.tolerance(tx, ty))
        if p:
            bad.append(("resize + orient", i, p))
    assert bad == [], bad[:8]


def run_orient(mjx, ctx, datas, fmt, code, roi, resize=None):
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, rois=roi, output=fmt, pixels="libjpeg", orient=mjx.Orient(exif=False, extra=code), resize=resize)
    try:
        b.decode()
        b.wait()
        assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas)
        return [b.output(i) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


@pytest.mark.gpu
def test_mixed_calls_tiles_and_the_pool(mjx, gpu_ctx):
    good = [tsl.data_of(n, w, h) for n, w, h in ((Y420, 333, 217), (Y422, 61, 45), (LUMA_SUB, 61, 45), ("Y11_Cb11_Cr11", 333, 217), ("gray22", 61, 45))]
    datas = good + [_read(os.path.join(PIL_DIR, "progressive.jpg"))]
    want = lj_decode(mjx, gpu_ctx, good)
    assert all(isinstance(w, np.ndarray) for w in want)
    # One call holds several layouts, a grey file, progressive.jpg and a per-picture refusal.  The layout is an option of the call,
    # not of a picture, so a REF_COMPAT refusal cannot stand beside good pictures: the refusal inside the mixed call is a rectangle
    # outside its picture (MJX_ERR_INVALID_ARG as well), and REF_COMPAT is checked in a call of its own below, where it refuses
    # every picture.
    b, st = mjx.decode_batch(gpu_ctx, datas + [good[1]], pixels="libjpeg", rois=[None] * len(datas) + [(60, 0, 2, 2)])
    try:
        assert st == [mjx.OK] * len(good) + [mjx.ERR_UNSUPPORTED_FORMAT, mjx.ERR_INVALID_ARG], st
        for i in range(len(good)):
            assert tsl.same(b.rgb(i), want[i]), i
    finally:
        b.close()
    # a REF_COMPAT call refuses every picture of its own and decodes nothing; mjx_decode gives the same bytes
    b, st = mjx.decode_batch(gpu_ctx, good, pixels="libjpeg", layout=mjx.LAYOUT_REF_COMPAT)
    b.close()
    assert st == [mjx.ERR_INVALID_ARG] * len(good), st
    assert tsl.same(mjx.decode(good[0], pixels="libjpeg"), want[0])
    assert tsl.same(mjx.JPEGImage.parse(good[1], ctx=gpu_ctx, pixels="libjpeg").image_data(), want[1])
    with pytest.raises(mjx.MjxError):
        mjx.decode(good[0], pixels="libjpeg", scale=2)
    # tile(3) keeps the option
    scans = [mjx.ParsedScan(d) for d in good]
    src = mjx.Batch(gpu_ctx, scans, pixels="libjpeg")
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
        res = pool.decode_batch(datas, pixels="libjpeg")
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
def test_pillow_end_to_end(mjx, gpu_ctx):
    """The reference alone is at 3; a sample that rounds the other way moves a channel by at most 2."""
    datas = [_read(p) for p in PILLOW_GPU_FILES]
    got = lj_decode(mjx, gpu_ctx, datas)
    for p, d, g in zip(PILLOW_GPU_FILES, datas, got):
        assert isinstance(g, np.ndarray), (p, g)
        mx, off1, off0 = diff_figures(g, pillow(d))
        print("%s: max %d, more than 1 off %.4f, off at all %.4f" % (os.path.basename(p), mx, off1, off0))
        assert mx <= 5 and off1 <= 0.02, (p, mx, off1)


@pytest.mark.gpu
def test_the_default_is_untouched(mjx, gpu_ctx):
    datas = [_read(p) for p in CPU_FILES] + [tsl.data_of(Y420, 333, 217), tsl.data_of(LUMA_SUB, 61, 45)]
    a, st_a = mjx.decode_batch(gpu_ctx, datas)
    b, st_b = mjx.decode_batch(gpu_ctx, datas, pixels=mjx.PIXELS_REFERENCE)
    c, st_c = mjx.decode_batch(gpu_ctx, datas, pixels="libjpeg")
    try:
        assert st_a == st_b == st_c == [mjx.OK] * len(datas)
        differ = 0
        for i in range(len(datas)):
            assert tsl.same(a.rgb(i), b.rgb(i)), i
            differ += not tsl.same(a.rgb(i), c.rgb(i))
        assert differ >= len(datas) - 2               # (the option is not a no-op: only flat or grey content can coincide)
        # a batch without the option launches exactly the kernels it launched before: none of the new pass's class
    finally:
        a.close(); b.close(); c.close()
    ctx = mjx.Context(0, profiling=True)
    try:
        for px, want in ((None, 0), ("libjpeg", 1)):
            bt, _ = mjx.decode_batch(ctx, datas[:3], pixels=px)
            try:
                bt.kernel_ms(reset=True)
                bt.decode()
                bt.wait()
                k = bt.kernel_ms()
                assert (k["resize"][1] > 0) == bool(want), (px, k["resize"])
                assert k["idct_color"][1] > 0
            finally:
                bt.close()
    finally:
        ctx.close()

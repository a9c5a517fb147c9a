"""Luminance output (MJX_OUTPUT_CHANNELS = 1, include/mjx.h): one element per pixel, chroma never transformed.

References, none of them the code under test:
  1  the chroma-neutral twin: the file's quantised blocks with every chroma block zeroed, written again with
     jpegwriter.jpeg_from_blocks (same layout, size, DQT and DHT).  The packed three-channel decode of the twin has R = G = B and
     that byte is L, bit for bit, at every scale (and for a one-component file L is the R byte of its own packed decode).
  2  float64: scaled_ref._samples(data, s)[0] = w with delta = 64 * 2^-24 * S_Y; the byte lies in [trunc_u8(w - delta),
     trunc_u8(w + delta)] and at most 2 % of a picture is undecided.  Scales 1 and 1/2 only: at 1/4 and 1/8 a quarter to all of the
     samples sit on whole numbers (q DC / 8), where no float decoder is decidable, and the twin is the check.
  3  libjpeg's pixels: libjpeg_ref.component_planes -> round_u8, upsampled with libjpeg_ref.upsample where Y is subsampled, its
     interval at K = 64 (2 % cap); Pillow's draft("L") -- libjpeg's own grey mode -- on the 24 layouts whose Y is the finest
     component, within test_libjpeg_pixels.py's bounds (max 3, more than 1 off 1 %, off at all 5 %).
The CPU tests prove the references against each other and check the planner, the mirrors and the shared host routine; the GPU
tests compare the device with them.
"""
import ctypes
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import libjpeg_ref as lj
import scaled_ref
import test_libjpeg_pixels as tlp
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_sampling_layouts as tsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA_DIR = os.path.join(ROOT, "tests", "data")
NAMES = tsl.NAMES
Y420, Y422, Y440, LUMA_SUB = tlp.Y420, tlp.Y422, tlp.Y440, tlp.LUMA_SUB
# the layouts whose Y is the finest component and that Pillow decodes (it refuses the 12-block MCU): libjpeg's grey mode gives their Y plane
Y_FINEST = [n for n in tlp.PIL_NAMES if tsl.parse_name(n)[0] == (max(h for h, _ in tsl.parse_name(n)), max(v for _, v in tsl.parse_name(n)))]
GENERIC5 = [Y422, Y440, LUMA_SUB, "Y11_Cb11_Cr11", "Y22_Cb22_Cr22"]
K = 64
CAP = 0.02


def _read(p):
    with open(p, "rb") as f:
        return f.read()


# ---- the references ------------------------------------------------------------------------------------------------------------------
def twin_of(lname, w, h, restart=None, quality=75, noise=4.0):
    """Reference 1: the chroma-neutral twin of tsl.layout_file(lname, w, h, ...) -- its own bytes for a one-component file."""
    data, per_comp = tsl.layout_file(lname, w, h, restart=restart, quality=quality, noise=noise)
    if lname.startswith("gray"):
        return data
    hv = tsl.parse_name(lname)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    rows = [a * b for a, b in hv]
    blocks = np.concatenate([(pc if c == 0 else np.zeros_like(pc)).reshape(mcux * mcuy, k, 64) for c, (pc, k) in enumerate(zip(per_comp, rows))],
                            axis=1).reshape(-1, 64)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    return jw.jpeg_from_blocks(blocks, hv, mcux, mcuy, [qt[tq] for _, _, tq in comps], jw.tables_from_jpeg(data), width=w, height=h,
                               restart=restart)


def y_f64(data, s):
    """Reference 2 -> (w, lo, hi): the float64 luminance sample under every output pixel and the bytes a float32 decoder may give"""
    dec = tsl.oracle_std(data)
    w = scaled_ref._samples(data, s, dec)[0]
    d = K * 2.0 ** -24 * scaled_ref._samples(data, s, dec, magnitude=True)[0]
    return w, scaled_ref.trunc_u8(w - d), scaled_ref.trunc_u8(w + d)


def interval_problem(got, data, s):
    _, lo, hi = y_f64(data, s)
    if not isinstance(got, np.ndarray) or got.shape != lo.shape:
        return ("shape or status", got if not isinstance(got, np.ndarray) else got.shape, lo.shape)
    share = float((lo != hi).mean())
    out = (got < lo) | (got > hi)
    if out.any() or share > CAP:
        return "outside %d of %d, first at %s; undecided share %.4f" % (int(out.sum()), out.size, np.argwhere(out)[:2].tolist(), share)
    return None


def lj_luma(data):
    """Reference 3 -> (L, lo, hi) uint8 [H, W]"""
    dec = tsl.oracle_std(data)
    w, h, pl, ratios = lj.component_planes(data, dec)
    _, _, mag, _ = lj.component_planes(data, dec, magnitude=True)
    rh, rv = ratios[0]
    up = lambda p: lj.upsample(lj.round_u8(p), rh, rv)[:h, :w].astype(np.uint8)
    d = K * 2.0 ** -24 * mag[0]
    return up(pl[0]), up(pl[0] - d), up(pl[0] + d)


def lj_problem(got, data):
    _, lo, hi = lj_luma(data)
    if not isinstance(got, np.ndarray) or got.shape != lo.shape:
        return ("shape or status", got if not isinstance(got, np.ndarray) else got.shape, lo.shape)
    share = float((lo != hi).mean())
    out = (got < lo) | (got > hi)
    if out.any() or share > CAP:
        return "outside %d of %d, first at %s; undecided share %.4f" % (int(out.sum()), out.size, np.argwhere(out)[:2].tolist(), share)
    return None


def pillow_l(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L", im.mode
    return np.asarray(im)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_output_layout_of_a_luminance_picture(mjx):
    for lname, W, H in ((Y420, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 333, 217)):
        scan = mjx.ParsedScan(tsl.data_of(lname, W, H))
        try:
            for dtype, esz in (("uint8", 1), ("float16", 2), ("float32", 4)):
                for planar in (False, True):
                    fmt = mjx.Output(dtype, planar=planar, bgr=planar, channels=1)
                    for s in (1, 2, 4, 8):
                        w, h = -(-W // s), -(-H // s)
                        lay = scan.output_layout(fmt, scale=s)
                        assert (lay["width"], lay["height"], lay["row_pitch"], lay["bytes"], lay["dev"]) == (w, h, w, w * h * esz, 0), (lname, dtype, s, lay)
                    lay = scan.output_layout(fmt, roi=(3, 5, 17, 9), scale=2)
                    assert (lay["width"], lay["height"], lay["row_pitch"], lay["bytes"]) == (17, 9, 17, 17 * 9 * esz), lay
                # caller-owned memory: padded rows are taken as they are, plane_pitch is ignored, a pitch below the width is refused
                base = 4096
                lay = scan.output_layout(mjx.Output(dtype, channels=1, dst=[(base, W, H, W + 5, 0)]))
                assert (lay["dev"], lay["row_pitch"], lay["bytes"]) == (base, W + 5, ((H - 1) * (W + 5) + W) * esz), lay
                lay = scan.output_layout(mjx.Output(dtype, planar=True, channels=1, dst=[(base, W, H, W, 1)]))
                assert (lay["row_pitch"], lay["bytes"]) == (W, W * H * esz), lay
                for dst in ((base, W, H, W - 1, 0), (base, W + 1, H, W + 1, 0), (0, W, H, W, 0)):
                    with pytest.raises(mjx.MjxError) as e:
                        scan.output_layout(mjx.Output(dtype, channels=1, dst=[dst]))
                    assert e.value.code == mjx.ERR_INVALID_ARG
            # channels: 0 and 3 are today's three channels, 1 is luminance, anything else is refused -- and refuses nothing else
            three = scan.output_layout(mjx.Output("uint8"))
            for ch in (2, 4, 255):
                with pytest.raises(mjx.MjxError) as e:
                    scan.output_layout(mjx.Output("uint8", channels=ch))
                assert e.value.code == mjx.ERR_INVALID_ARG
            assert scan.output_layout(mjx.Output("uint8", channels=0)) == three == scan.output_layout(mjx.Output("uint8", channels=3))
            assert three["row_pitch"] == 3 * W and three["bytes"] == 3 * W * H
        finally:
            scan.close()
    # REF_COMPAT is refused as for any output description (a file the reference's own layout accepts: the refusal is the description's)
    scan = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))
    try:
        assert scan.output_layout(None, layout=mjx.LAYOUT_REF_COMPAT)["bytes"] == 64 * 48 * 3
        with pytest.raises(mjx.MjxError) as e:
            scan.output_layout(mjx.Output("uint8", channels=1), layout=mjx.LAYOUT_REF_COMPAT)
        assert e.value.code == mjx.ERR_INVALID_ARG
    finally:
        scan.close()
    # one value per channel: a scalar or one element for luminance
    a, b = mjx.Output("float32", channels=1, mean=0.5, std=0.25), mjx.Output("float32", channels=1, mean=[0.5], std=(0.25,))
    assert np.array_equal(a.scale, b.scale) and np.array_equal(a.bias, b.bias) and a.desc().channels == 1


def test_the_channel_byte_and_the_accessor_are_mirrored_everywhere(mjx):
    """The channel count is byte 3 of mjx_output, the byte its declared members leave unused behind `bgr`: the member lists of the
    header, Python and Rust stay the parent's (tests/test_output_formats.py pins them), and each of the three names the byte."""
    raw = _read(os.path.join(ROOT, "include", "mjx.h")).decode()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    assert re.search(r"#define MJX_OUTPUT_CHANNELS_OFFSET 3\b", hdr) and re.search(r"#define MJX_OUTPUT_CHANNELS\(out\) \(\(\(uint8_t \*\)\(out\)\)\[MJX_OUTPUT_CHANNELS_OFFSET\]\)", hdr)
    assert re.search(r"pub const MJX_OUTPUT_CHANNELS_OFFSET: usize = 3;", rs) and "pub fn set_channels(&mut self, channels: u8)" in rs and "pub fn channels(&self) -> u8" in rs
    assert mjx.OutputDesc.CHANNELS_OFFSET == 3
    # the byte is free: no member covers it, and the size and every offset are the parent's (literals)
    assert ctypes.sizeof(mjx.OutputDesc) == 48
    members = ["dtype", "planar", "bgr", "scale", "bias", "dst", "n_dst"]
    assert [f[0] for f in mjx.OutputDesc._fields_] == members
    assert [getattr(mjx.OutputDesc, n).offset for n in members] == [0, 1, 2, 4, 16, 32, 40] and mjx.OutputDesc.bgr.size == 1
    d = mjx.Output("float32", planar=True, bgr=True, channels=1).desc()
    assert bytes(d)[:4] == bytes([mjx.DTYPE_F32, 1, 1, 1]) and d.channels == 1
    d.channels = 3
    assert bytes(d)[3] == 3 and (d.dtype, d.planar, d.bgr) == (mjx.DTYPE_F32, 1, 1)
    assert bytes(mjx.Output("uint8").desc())[3] == 3 and bytes(mjx.OutputDesc())[3] == 0         # (a zero-filled struct means what it meant)
    for fn, n in (("mjx_batch_output_channels", 3), ("mjx_upsample_luma_host", 7)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)
        assert fn in mjx.SYMBOLS and len(mjx.SYMBOLS[fn][1]) == n, fn
        assert hasattr(ctypes.CDLL(mjx.lib_path()), fn), fn
    assert re.search(r"#define MJX_ABI_VERSION 2\b", hdr) and b"abi=2" in mjx.lib().mjx_version()


def test_the_shared_luminance_routine_is_the_reference_bit_for_bit(mjx):
    rng = np.random.default_rng(11)
    bad = []
    for rh, rv in tlp.HV:
        for cw in tlp.PLANE_DIMS:
            for ch in tlp.PLANE_DIMS:
                for fill in ("random", "low", "high"):
                    plane = {"random": rng.integers(0, 256, (ch, cw), dtype=np.uint8), "low": np.zeros((ch, cw), np.uint8),
                             "high": np.full((ch, cw), 255, np.uint8)}[fill]
                    want = lj.upsample(plane.astype(np.int32), rh, rv).astype(np.uint8)
                    H, W = want.shape
                    rects = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (W // 2, H // 3, W - W // 2, H - H // 3)]
                    if W > 1:
                        rects += [(W - 1, 0, 1, H), (0, 0, W - 1, H)]     # (an odd picture: the plane's last sample is not used to its end)
                    for x, y, w, h in rects:
                        got = mjx.upsample_luma_host(plane, rh, rv, (x, y, w, h))
                        if not tsl.same(got, want[y:y + h, x:x + w]):
                            bad.append((rh, rv, cw, ch, fill, (x, y, w, h)))
    assert bad == [], bad[:8]
    for args in ((np.zeros((3, 3), np.uint8), 3, 1, (0, 0, 1, 1)), (np.zeros((3, 3), np.uint8), 1, 1, (0, 0, 4, 1)), (np.zeros((3, 3), np.uint8), 2, 2, (0, 6, 1, 1))):
        with pytest.raises(mjx.MjxError):
            mjx.upsample_luma_host(*args)


@pytest.mark.parametrize("part", range(4))
def test_the_references_agree_with_each_other(orc, part):
    """Reference 1 against the oracle and reference 2: under the oracle the twin keeps Y's T0 and has R = G = B, and that byte is
    to_u8 of the float64 luminance sample of the FILE at every scale in float64 arithmetic (the oracle's own float32 picture of the twin
    lies in reference 2's interval); reference 2 decides at least 98 % of a picture at scales 1, 2."""
    cases = [(n, 61, 45) for n in NAMES[part * 16:(part + 1) * 16]]
    if part == 0:
        cases += [(n, 333, 217) for n in GENERIC5] + [(Y420, 17, 9), (Y420, 16, 16), ("gray12", 333, 217)]
    bad, worst = [], 0.0
    for lname, w, h in cases:
        data, tw = tsl.data_of(lname, w, h), twin_of(lname, w, h)
        da, dt = tsl.oracle_std(data), tsl.oracle_std(tw)
        if not np.array_equal(da.coefs[0], dt.coefs[0]) or any(c.any() for c in dt.coefs[1:]):
            bad.append((lname, w, h, "the twin's coefficients"))
        if not (np.array_equal(dt.rgb[:, :, 0], dt.rgb[:, :, 1]) and np.array_equal(dt.rgb[:, :, 0], dt.rgb[:, :, 2])):
            bad.append((lname, w, h, "the oracle's twin is not grey"))
        for s in (1, 2, 4, 8):
            y = scaled_ref.to_u8(scaled_ref._samples(data, s, da)[0])
            t = scaled_ref.scaled_rgb(tw, s, dt)
            if not all(np.array_equal(t[:, :, c], y) for c in range(3)):
                bad.append((lname, w, h, s, "float64 twin"))
            if s <= 2:
                _, lo, hi = y_f64(data, s)
                # (the oracle computes in float32: its twin's byte is float64's wherever float64 decides, e.g. not at 142.9999994)
                if s == 1 and ((dt.rgb[:, :, 0] < lo) | (dt.rgb[:, :, 0] > hi)).any():
                    bad.append((lname, w, h, "oracle twin outside the float64 interval"))
                share = float((lo != hi).mean())
                worst = max(worst, share)
                if share > CAP or ((y < lo) | (y > hi)).any():
                    bad.append((lname, w, h, s, "undecided %.4f" % share))
    print("largest undecided share of the float64 interval: %.4f" % worst)
    assert bad == [], bad[:8]


def test_the_libjpeg_reference_is_libjpegs_grey_mode(orc):
    """Reference 3 against Pillow's draft("L") on the 24 layouts whose Y is the finest component (the others libjpeg upsamples
    only on the way to RGB), lena.jpeg and a grey file; its interval decides at least 98 % of every picture."""
    assert len(Y_FINEST) == 24
    files = [(n, tlp.q85(n, 61, 45)) for n in Y_FINEST] + [("lena.jpeg", _read(os.path.join(DATA_DIR, "lena.jpeg"))), ("gray22", tsl.data_of("gray22", 61, 45))]
    bad, worst = [], [0, 0.0, 0.0, 0.0]
    for n, data in files:
        L, lo, hi = lj_luma(data)
        mx, off1, off0 = tlp.diff_figures(L, pillow_l(data))
        share = float((lo != hi).mean())
        worst = [max(worst[0], mx), max(worst[1], off1), max(worst[2], off0), max(worst[3], share)]
        if mx > 3 or off1 > 0.01 or off0 > 0.05 or share > CAP or ((L < lo) | (L > hi)).any():
            bad.append((n, mx, off1, off0, share))
    for n in NAMES:
        data = tsl.data_of(n, 61, 45)
        _, lo, hi = lj_luma(data)
        worst[3] = max(worst[3], float((lo != hi).mean()))
    print("against Pillow: max %d, more than 1 off %.4f, off at all %.4f; largest undecided share %.4f" % tuple(worst))
    assert bad == [] and worst[3] <= CAP, (bad[:8], worst)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def luma_decode(mjx, ctx, datas, fmt=None, **kw):
    """-> [the luminance picture [H, W] (or the format's array when fmt is given) or ('status', code)] of a Batch of parsed scans"""
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, output=fmt or mjx.Output("uint8", channels=1), **kw)
    try:
        b.decode()
        b.wait()
        out = []
        for i in range(len(datas)):
            if b.status(i) != mjx.OK:
                out.append(("status", b.status(i)))
                continue
            a = b.output(i)
            assert b.output_info(i)["channels"] == 1
            out.append(a if fmt is not None else np.ascontiguousarray(a[:, :, 0]))
        return out
    finally:
        tsl.close_all(b, scans)


def packed_decode(mjx, ctx, datas, **kw):
    """the parent's path: no output description at all"""
    b, scans = tsl.decode_batch(mjx, ctx, datas, **kw)
    try:
        return [b.rgb(i) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


def twin_problems(mjx, ctx, cases, scales, **kw):
    """cases: [(lname, w, h, keywords of layout_file)] -> what differs between the luminance decode and the twins' packed decode"""
    datas = [tsl.data_of(n, w, h, **k) for n, w, h, k in cases]
    twins = [twin_of(n, w, h, **k) for n, w, h, k in cases]
    bad = []
    for s in scales:
        got = luma_decode(mjx, ctx, datas, scale=s, **kw)
        want = packed_decode(mjx, ctx, twins, scale=s)
        for c, g, t, d in zip(cases, got, want, datas):
            if not isinstance(t, np.ndarray) or not (np.array_equal(t[:, :, 0], t[:, :, 1]) and np.array_equal(t[:, :, 0], t[:, :, 2])):
                bad.append((c, s, "the twin's packed decode is not grey"))
            elif not tsl.same(g, t[:, :, 0]):
                bad.append((c, s, g if not isinstance(g, np.ndarray) else "%d bytes differ" % int((g != t[:, :, 0]).sum())))
            elif s <= 2:
                p = interval_problem(g, d, s)
                if p:
                    bad.append((c, s, p))
        alone = luma_decode(mjx, ctx, datas[:1], scale=s, **kw)          # (a batch of one: the latency plan's cut of the scan)
        if not tsl.same(alone[0], got[0]):
            bad.append((cases[0], s, "alone"))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("scale", (1, 2, 4, 8))
def test_every_layout_is_its_twins_byte(mjx, gpu_ctx, scale):
    bad = twin_problems(mjx, gpu_ctx, [(n, 61, 45, {}) for n in NAMES], [scale])
    assert bad == [], bad[:6]


@pytest.mark.gpu
def test_larger_pictures_the_dedicated_form_and_one_component(mjx, gpu_ctx):
    # five generic layouts at 333 x 217; 4:2:0 at 1035 x 490 -- 63 tiles of the dedicated form, several workgroups, tiles that wrap MCU
    # rows, an odd width --, once with a sparse stream and once with a dense one (tiles of more entries than a lane prefetches); the
    # smallest 4:2:0 pictures; one-component files against their own R channel (twin_of gives the file itself)
    cases = [(n, 333, 217, {}) for n in GENERIC5] + [(Y420, 1035, 490, {}), (Y420, 1035, 490, dict(quality=97, noise=12.0)),
                                                     (Y420, 17, 9, {}), (Y420, 16, 16, {}), ("gray22", 61, 45, {}), ("gray12", 333, 217, {})]
    bad = twin_problems(mjx, gpu_ctx, cases, (1, 2, 4, 8))
    assert bad == [], bad[:6]
    # the dense file alone in its call: the chunk then counts as dense
    bad = twin_problems(mjx, gpu_ctx, cases[6:7], (1,))
    assert bad == [], bad[:6]


STREAM_SCALES = (1, 2, 8)


def stream_files():
    """tlp.stream_files' cases: per case the interleaved file, two multi-scan twins (read directly at 1000 x 40, gathered at
    333 x 217) and a restart-interval twin -> [(name, bytes, index of the interleaved file whose luminance picture it must equal)]"""
    return tlp.stream_files()


def child_streams(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = stream_files()
    out, status = {}, {}
    for dd in (False, True):
        for s in STREAM_SCALES:
            b, st = mjx.decode_batch(ctx, [d for _, d, _ in files], device_destuff=dd, scale=s, output=mjx.Output("uint8", channels=1))
            for i in range(len(files)):
                key = "%d_%d_%d" % (i, dd, s)
                status[key] = st[i] or b.status(i)
                if not status[key]:
                    out[key] = b.output(i)[:, :, 0]
            b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=status)))


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_luma_output as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_stream_source_gives_the_interleaved_files_picture(mjx, gpu_ctx, tmp_path):
    files = stream_files()
    want = {s: luma_decode(mjx, gpu_ctx, [d for _, d, _ in files], scale=s) for s in STREAM_SCALES}
    bad = [(files[i][0], s, "status", w) for s in STREAM_SCALES for i, w in enumerate(want[s]) if not isinstance(w, np.ndarray)]
    bad += [(files[b][0], n, s, "in process") for s in STREAM_SCALES for i, (n, _, b) in enumerate(files) if not tsl.same(want[s][i], want[s][b])]
    for k, env in enumerate(({"MJX_SINGLE_DECODE": "0"}, {"MJX_STREAM_LINEAR": "1"}, {"MJX_PLANAR_DIRECT": "0"})):
        npz = tmp_path / ("streams%d.npz" % k)
        res = run_child(tmp_path, "child_streams(%r)" % str(npz), env)
        with np.load(str(npz)) as z:
            for i, (n, _, b) in enumerate(files):
                for dd in (0, 1):
                    for s in STREAM_SCALES:
                        key = "%d_%d_%d" % (i, dd, s)
                        if res["status"][key] != 0 or not tsl.same(z[key], want[s][b]):
                            bad.append((files[b][0], n, sorted(env.items()), "device de-stuffing" if dd else "host de-stuffing", s, res["status"][key]))
    assert bad == [], bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("lname", [Y420, Y422, LUMA_SUB, "gray22"])
def test_rectangles_are_the_crop_of_the_whole_luminance_picture(mjx, gpu_ctx, lname):
    bad = []
    hv = [(1, 1)] if lname.startswith("gray") else tsl.parse_name(lname)
    for W, H in ((333, 217), (61, 45)):
        data = tsl.data_of(lname, W, H)
        for s in (1, 2, 4, 8):
            w, h = -(-W // s), -(-H // s)
            full = luma_decode(mjx, gpu_ctx, [data], scale=s)[0]
            assert isinstance(full, np.ndarray) and full.shape == (h, w)
            n = 8 // s
            rects = tlp.rectangles(w, h, n * max(a for a, _ in hv), n * max(b for _, b in hv))
            assert len(rects) >= 8, rects
            got = luma_decode(mjx, gpu_ctx, [data] * len(rects), scale=s, rois=rects)
            for (x, y, rw, rh), g in zip(rects, got):
                if not tsl.same(g, full[y:y + rh, x:x + rw]):
                    bad.append((W, H, s, (x, y, rw, rh), g if not isinstance(g, np.ndarray) else int((g != full[y:y + rh, x:x + rw]).sum())))
    assert bad == [], bad[:8]
    tiles = mjx.plan_tiles(tsl.data_of(lname, 333, 217), roi=(120, 90, 40, 30))
    assert tiles["tiles_read"] < tiles["tiles_total"], tiles


FMT_FILES = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 333, 217)]
FMT_ROIS = [None, (3, 5, 40, 30), None, (101, 50, 99, 77)]


def luma_formats(mjx):
    """the dtypes, both shapes, a scalar and a one-element mean / std"""
    out = []
    for d in tof.DTYPES:
        for planar in (False, True):
            kw = {} if d == "uint8" else (dict(mean=0.449, std=0.226) if planar else dict(mean=[0.5], std=[0.25]))
            out.append(mjx.Output(d, planar=planar, bgr=planar, channels=1, **kw))
    return out


def expected_luma(L, fmt):
    """The luminance bytes [H, W] pushed through the format's 256-entry table (exact arithmetic, tof.exact_table) and its shape"""
    if fmt.numpy_dtype() == np.uint8:
        v = L
    else:
        t = tof.exact_table(fmt.scale, fmt.bias)[0]
        v = (t if fmt.numpy_dtype() == np.float32 else t.astype(np.float16))[L]
    return np.ascontiguousarray(v[None, :, :] if fmt.planar else v[:, :, None])


@pytest.mark.gpu
def test_formats_are_the_table_on_the_luminance_byte(mjx, gpu_ctx):
    datas = [tsl.data_of(*c) for c in FMT_FILES]
    bad = []
    for s in (1, 2, 8):
        rois = FMT_ROIS if s == 1 else [None if r is None else (r[0] // s, r[1] // s, max(1, r[2] // s), max(1, r[3] // s)) for r in FMT_ROIS]
        L = luma_decode(mjx, gpu_ctx, datas, scale=s, rois=rois)
        assert all(isinstance(p, np.ndarray) for p in L), L
        for fmt in luma_formats(mjx):
            got = luma_decode(mjx, gpu_ctx, datas, fmt=fmt, scale=s, rois=rois)
            for i, g in enumerate(got):
                if not isinstance(g, np.ndarray) or not tof.same_bits(g, expected_luma(L[i], fmt)):
                    bad.append((s, fmt.dtype, fmt.planar, FMT_FILES[i]))
    assert bad == [], bad[:8]


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    datas = [tsl.data_of(*c) for c in FMT_FILES]
    rois = [(11, 7, 47, 35), (3, 5, 47, 35), (0, 9, 47, 35), (101, 50, 47, 35)]
    ref, _ = mjx.decode_batch(ctx, datas, rois=rois, output=mjx.Output("uint8", channels=1))
    L = [ref.output(i)[:, :, 0] for i in range(len(datas))]
    ref.close()
    dev, n = torch.device("cuda", 0), len(datas)
    # N x 1 x H x W float16, rows padded on both sides (an odd offset: misaligned strips), guard rows above and below
    big = torch.full((n, 1, 39, 56), float("nan"), dtype=torch.float16, device=dev)
    st = mjx.decode_into(ctx, datas, big[:, :, 2:37, 5:52], rois=rois, mean=0.449, std=0.226)
    torch.cuda.synchronize()
    fmt = mjx.Output("float16", planar=True, channels=1, mean=0.449, std=0.226)
    got = big.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][:, 2:37, 5:52]), expected_luma(L[i], fmt)):
            bad.append(("f16 1xHxW", i, st[i]))
    inside = np.zeros(got.shape, bool)
    inside[:, :, 2:37, 5:52] = True
    if not np.isnan(got[~inside]).all():
        bad.append("the padding or the guards of the f16 rows were written")
    # N x H x W x 1 uint8 with a sentinel
    big8 = torch.full((n, 37, 53, 1), 7, dtype=torch.uint8, device=dev)
    st = mjx.decode_into(ctx, datas, big8[:, 1:36, 3:50, :], rois=rois)
    torch.cuda.synchronize()
    got = big8.cpu().numpy()
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(got[i][1:36, 3:50, :]), np.ascontiguousarray(L[i][:, :, None])):
            bad.append(("u8 HxWx1", i, st[i]))
    inside = np.zeros(got.shape, bool)
    inside[:, 1:36, 3:50, :] = True
    if not np.all(got[~inside] == 7):
        bad.append("the padding or the guards of the u8 rows were written")
    # float32 dense, a one-element mean / std; N x 1 x H x 1 needs the keyword
    out32 = torch.zeros((n, 35, 47, 1), dtype=torch.float32, device=dev)
    st = mjx.decode_into(ctx, datas, out32, rois=rois, mean=[0.5], std=[0.25])
    torch.cuda.synchronize()
    fmt = mjx.Output("float32", channels=1, mean=0.5, std=0.25)
    for i in range(n):
        if st[i] != mjx.OK or not tof.same_bits(np.ascontiguousarray(out32[i].cpu().numpy()), expected_luma(L[i], fmt)):
            bad.append(("f32 HxWx1", i, st[i]))
    col = torch.zeros((n, 1, 35, 1), dtype=torch.uint8, device=dev)
    try:
        mjx.decode_into(ctx, datas, col, rois=[(r[0], r[1], 1, 35) for r in rois])
        bad.append("N x 1 x H x 1 was taken without planar=")
    except mjx.MjxError:
        pass
    st = mjx.decode_into(ctx, datas, col, rois=[(r[0], r[1], 1, 35) for r in rois], planar=True)
    torch.cuda.synchronize()
    for i in range(n):
        if st[i] != mjx.OK or not np.array_equal(col[i, 0, :, 0].cpu().numpy(), L[i][:, 0]):
            bad.append(("u8 1xHx1", i, st[i]))
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad)}))


@pytest.mark.gpu
def test_decode_into_both_tensor_shapes_with_padded_rows_and_guards(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["nbad"] == 0, res


def _three(fmt1, mjx):
    """the three-channel format with the luminance format's one scale and bias: test_resize.check_against speaks of three channels"""
    names = {0: "uint8", 1: "float16", 2: "float32"}
    if fmt1.dtype == 0:
        return mjx.Output("uint8", planar=fmt1.planar)
    return mjx.Output(names[fmt1.dtype], planar=fmt1.planar, scale=[float(fmt1.scale[0])] * 3, bias=[float(fmt1.bias[0])] * 3)


def _rep3(a, planar):
    return np.ascontiguousarray(np.repeat(a, 3, axis=0 if planar else 2))


def run_luma(mjx, ctx, datas, fmt, **kw):
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, output=fmt, **kw)
    try:
        b.decode()
        b.wait()
        assert [b.status(i) for i in range(len(datas))] == [mjx.OK] * len(datas), [b.status(i) for i in range(len(datas))]
        return [b.output(i) for i in range(len(datas))], [b.scale(i) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


@pytest.mark.gpu
def test_resize_orientation_and_both_work_on_the_one_byte_intermediate(mjx, gpu_ctx):
    datas = [tsl.data_of(Y420, 333, 217), tsl.data_of(Y422, 333, 217), tsl.data_of("gray12", 333, 217)]
    roi = (10, 6, 50, 37)
    bad = []
    plain = {s: luma_decode(mjx, gpu_ctx, datas, scale=s) for s in (1, 2)}
    # resize without auto_scale at scales 1 and 2, the rectangle in the scaled picture: test_resize's rule on the plain luminance decode
    for s in (1, 2):
        for fmt in (mjx.Output("uint8", channels=1), mjx.Output("float32", planar=True, channels=1, mean=0.5, std=0.25), mjx.Output("float16", channels=1, mean=[0.4], std=[0.2])):
            for aa in (True, False):
                got, scales = run_luma(mjx, gpu_ctx, datas, fmt, scale=s, rois=roi, resize=mjx.Resize(23, 31, antialias=aa, auto_scale=False))
                assert scales == [s] * 3
                for i, g in enumerate(got):
                    I = plain[s][i][roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]
                    tx, ty = trs.max_taps(roi[2], 23, aa), trs.max_taps(roi[3], 31, aa)
                    p, _, _ = trs.check_against(_rep3(g, fmt.planar), trs.resize_ref(np.repeat(I[:, :, None], 3, axis=2), 23, 31, aa), _three(fmt, mjx), trs.tolerance(tx, ty))
                    if p:
                        bad.append(("resize", s, fmt.dtype, aa, i, p))
    # auto_scale picks the scale as for colour
    fmt = mjx.Output("float32", channels=1)
    got, scales = run_luma(mjx, gpu_ctx, datas[:2], fmt, resize=mjx.Resize(70, 37, antialias=True, auto_scale=True))
    want_scale = mjx.ParsedScan(datas[0]).resize_plan(mjx.Resize(70, 37, antialias=True, auto_scale=True))["scale"]
    assert scales == [want_scale] * 2 and want_scale > 1, (scales, want_scale)
    full = luma_decode(mjx, gpu_ctx, datas[:2], scale=want_scale)
    for i, g in enumerate(got):
        hh, ww = full[i].shape
        p, _, _ = trs.check_against(_rep3(g, False), trs.resize_ref(np.repeat(full[i][:, :, None], 3, axis=2), 70, 37, True), _three(fmt, mjx),
                                    trs.tolerance(trs.max_taps(ww, 70, True), trs.max_taps(hh, 37, True)))
        if p:
            bad.append(("auto_scale", i, p))
    # orientation alone, codes 1 .. 8: the formats' table on the mapped byte, bit for bit (the rectangle is the turned picture's)
    r = (5, 9, 41, 30)
    for code in range(1, 9):
        for fmt in (mjx.Output("uint8", channels=1), mjx.Output("float16", planar=True, channels=1, mean=0.449, std=0.226)):
            got, _ = run_luma(mjx, gpu_ctx, datas, fmt, rois=r, orient=mjx.Orient(exif=False, extra=code))
            for i, g in enumerate(got):
                D = np.ascontiguousarray(tor.orient_np(code, plain[1][i])[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])
                if not tof.same_bits(g, expected_luma(D, fmt)):
                    bad.append(("orient", code, fmt.dtype, i))
    # both: the rule on orient_c of the intermediate
    fmt = mjx.Output("float32", planar=True, channels=1, mean=0.5, std=0.25)
    for code in range(1, 9):
        got, _ = run_luma(mjx, gpu_ctx, datas, fmt, rois=r, orient=mjx.Orient(exif=False, extra=code), resize=mjx.Resize(19, 26, antialias=True, auto_scale=False))
        for i, g in enumerate(got):
            D = np.ascontiguousarray(tor.orient_np(code, plain[1][i])[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])
            p, _, _ = trs.check_against(_rep3(g, True), trs.resize_ref(np.repeat(D[:, :, None], 3, axis=2), 19, 26, True), _three(fmt, mjx),
                                        trs.tolerance(trs.max_taps(r[2], 19, True), trs.max_taps(r[3], 26, True)))
            if p:
                bad.append(("resize + orient", code, i, p))
    assert bad == [], bad[:8]


def lj_decode(mjx, ctx, datas, **kw):
    return luma_decode(mjx, ctx, datas, pixels="libjpeg", **kw)


@pytest.mark.gpu
def test_libjpeg_pixels_lie_in_the_interval_float64_allows(mjx, gpu_ctx):
    cases = [(n, 61, 45) for n in NAMES] + [(Y420, 1035, 490), ("gray22", 61, 45)]
    datas = [tsl.data_of(*c) for c in cases]
    got = lj_decode(mjx, gpu_ctx, datas)
    bad = [(c, p) for c, d, g in zip(cases, datas, got) for p in [lj_problem(g, d)] if p]
    # rectangles, the formats, a resize and an orientation on top: the crop / table / rule on the plain libjpeg luminance
    k = NAMES.index(LUMA_SUB)
    rects = tlp.rectangles(61, 45, 16, 16)
    crops = lj_decode(mjx, gpu_ctx, [datas[k]] * len(rects), rois=rects)
    bad += [(LUMA_SUB, r) for r, g in zip(rects, crops) if not tsl.same(g, got[k][r[1]:r[1] + r[3], r[0]:r[0] + r[2]])]
    fmt = mjx.Output("float32", planar=True, channels=1, mean=0.5, std=0.25)
    f = lj_decode(mjx, gpu_ctx, datas[:4], fmt=fmt)
    bad += [("format", i) for i in range(4) if not tof.same_bits(f[i], expected_luma(got[i], fmt))]
    o, _ = run_luma(mjx, gpu_ctx, [datas[k]], mjx.Output("uint8", channels=1), pixels="libjpeg", orient=mjx.Orient(exif=False, extra=6))
    if not tof.same_bits(o[0], np.ascontiguousarray(tor.orient_np(6, got[k])[:, :, None])):
        bad.append("orientation")
    rs, _ = run_luma(mjx, gpu_ctx, [datas[k]], fmt, pixels="libjpeg", resize=mjx.Resize(23, 31, antialias=True, auto_scale=True))
    p, _, _ = trs.check_against(_rep3(rs[0], True), trs.resize_ref(np.repeat(got[k][:, :, None], 3, axis=2), 23, 31, True), _three(fmt, mjx),
                                trs.tolerance(trs.max_taps(61, 23, True), trs.max_taps(45, 31, True)))
    if p:
        bad.append(("resize", p))
    # the refusals stay: a scale with libjpeg's pixels
    assert lj_decode(mjx, gpu_ctx, datas[:1], scale=2) == [("status", mjx.ERR_INVALID_ARG)]
    assert bad == [], bad[:6]


@pytest.mark.gpu
def test_libjpeg_pixels_against_pillows_grey_mode(mjx, gpu_ctx):
    files = [(n, tlp.q85(n, 61, 45)) for n in Y_FINEST] + [("lena.jpeg", _read(os.path.join(DATA_DIR, "lena.jpeg")))]
    got = lj_decode(mjx, gpu_ctx, [d for _, d in files])
    bad = []
    for (n, d), g in zip(files, got):
        assert isinstance(g, np.ndarray), (n, g)
        mx, off1, off0 = tlp.diff_figures(g, pillow_l(d))
        print("%s: max %d, more than 1 off %.4f, off at all %.4f" % (n, mx, off1, off0))
        if mx > 3 or off1 > 0.01 or off0 > 0.05:
            bad.append((n, mx, off1, off0))
    assert bad == [], bad


def child_groups(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    datas = group_files()
    b, st = mjx.decode_batch(ctx, datas, output=mjx.Output("uint8", channels=1))
    out = {"%d" % i: b.output(i)[:, :, 0] for i in range(len(datas)) if not st[i]}
    b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=list(st))))


def group_files():
    """3.8 MB of files: with groups of 1 MB the pipelined call cuts the list several times"""
    base = [tsl.data_of(Y420, 1035, 490, quality=97, noise=12.0), tsl.data_of(Y422, 333, 217), tsl.data_of("gray12", 333, 217), tsl.data_of(LUMA_SUB, 333, 217)]
    return base * 7


@pytest.mark.gpu
def test_mixed_calls_tiles_and_the_pipelined_groups(mjx, gpu_ctx, tmp_path):
    good = [tsl.data_of(n, w, h) for n, w, h in ((Y420, 333, 217), (Y422, 61, 45), (LUMA_SUB, 61, 45), ("Y11_Cb11_Cr11", 333, 217), ("gray22", 61, 45))]
    want = luma_decode(mjx, gpu_ctx, good)
    assert all(isinstance(w, np.ndarray) for w in want)
    for i, d in enumerate(good):                       # (each alone is the picture of the mixed batch; each its twin's byte was shown above)
        assert tsl.same(luma_decode(mjx, gpu_ctx, [d])[0], want[i]), i
    datas = good + [_read(os.path.join(tlp.PIL_DIR, "progressive.jpg"))]
    fmt = mjx.Output("uint8", channels=1)
    b, st = mjx.decode_batch(gpu_ctx, datas + [good[1]], output=fmt, rois=[None] * len(datas) + [(60, 0, 2, 2)])
    try:
        assert st == [mjx.OK] * len(good) + [mjx.ERR_UNSUPPORTED_FORMAT, mjx.ERR_INVALID_ARG], st
        for i in range(len(good)):
            assert tsl.same(b.output(i)[:, :, 0], want[i]), i
            inf = b.output_info(i)
            assert (inf["channels"], inf["row_pitch"], inf["width"]) == (1, want[i].shape[1], want[i].shape[1]), inf
        sb = b.bytes()
        assert sb["rgb"] == sum(w.size for w in want) and sb["pixels"] == sb["rgb"], sb
        with pytest.raises(mjx.MjxError):
            b.rgb(0)
    finally:
        b.close()
    # a REF_COMPAT call and a channel count of 2 refuse every picture; a colour batch answers 3
    # (REF_COMPAT: a picture on which the reference's own placement panics keeps that status, the picture's fault comes first)
    b, st0 = mjx.decode_batch(gpu_ctx, good, layout=mjx.LAYOUT_REF_COMPAT)
    b.close()
    assert mjx.OK in st0, st0
    for kw, want_st in ((dict(layout=mjx.LAYOUT_REF_COMPAT, output=fmt), [s or mjx.ERR_INVALID_ARG for s in st0]),
                        (dict(output=mjx.Output("uint8", channels=2)), [mjx.ERR_INVALID_ARG] * len(good))):
        b, st = mjx.decode_batch(gpu_ctx, good, **kw)
        b.close()
        assert st == want_st, (st, want_st)
    b, st = mjx.decode_batch(gpu_ctx, good[:2])
    try:
        assert b.output_info(0)["channels"] == 3
    finally:
        b.close()
    # tile(3) keeps the format
    scans = [mjx.ParsedScan(d) for d in good]
    src = mjx.Batch(gpu_ctx, scans, output=mjx.Output("float16", planar=True, channels=1, mean=0.449, std=0.226))
    try:
        t = src.tile(3)
        try:
            t.decode()
            t.wait()
            n = len(good)
            assert [t.status(i) for i in range(3 * n)] == [mjx.OK] * (3 * n)
            f16 = mjx.Output("float16", planar=True, channels=1, mean=0.449, std=0.226)
            for i in range(3 * n):
                assert tof.same_bits(t.output(i), expected_luma(want[i % n], f16)), i
        finally:
            t.close()
    finally:
        tsl.close_all(src, scans)
    # mjx_decode_batch_out over a list cut into groups, in a fresh process
    files = group_files()
    assert sum(len(d) for d in files) > 3 << 20
    one = luma_decode(mjx, gpu_ctx, files[:4])
    npz = tmp_path / "groups.npz"
    res = run_child(tmp_path, "child_groups(%r)" % str(npz), {"MJX_GROUP_MB": "1"})
    assert res["status"] == [0] * len(files), res
    with np.load(str(npz)) as z:
        for i in range(len(files)):
            assert tsl.same(z["%d" % i], one[i % 4]), i


@pytest.mark.gpu
def test_the_default_is_untouched(mjx, gpu_ctx):
    datas = [tsl.data_of(Y420, 333, 217), tsl.data_of(LUMA_SUB, 61, 45), tsl.data_of("gray22", 61, 45), _read(os.path.join(DATA_DIR, "lena.jpeg"))]
    for s in (1, 2, 8):
        packed = packed_decode(mjx, gpu_ctx, datas, scale=s)
        for k in (0, 3, 7, 10):
            for ch in (None, 0, 3):
                fmt = tof.make_format(mjx, k) if ch is None else tof.make_format(mjx, k, channels=ch)
                got, _ = run_luma(mjx, gpu_ctx, datas, fmt, scale=s)
                for i, g in enumerate(got):
                    assert tof.same_bits(g, tof.expected(packed[i], fmt)), (s, k, ch, i)
    # a call that does not ask for luminance launches what it launched before: no kernel of the passes behind stage B; a luminance
    # call at full size neither
    ctx = mjx.Context(0, profiling=True)
    try:
        for fmt in (None, mjx.Output("uint8"), mjx.Output("uint8", channels=1)):
            bt, _ = mjx.decode_batch(ctx, datas, output=fmt)
            try:
                bt.kernel_ms(reset=True)
                bt.decode()
                bt.wait()
                k = bt.kernel_ms()
                assert k["resize"][1] == 0 and k["idct_color"][1] > 0, k
            finally:
                bt.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_cli_writes_the_batchs_picture_as_p5(mjx, gpu_ctx, tmp_path):
    import __graft_entry__ as ge
    cli = os.path.join(ge.PKG_DIR, "mjx_cli")
    for lname, kw, args in ((Y420, {}, []), (LUMA_SUB, dict(scale=2), ["--scale", "2"]), (Y422, dict(rois=(3, 5, 40, 30)), ["--crop", "3,5,40,30"])):
        data = tsl.data_of(lname, 61, 45)
        src, dst = tmp_path / "in.jpg", tmp_path / "out.pgm"
        src.write_bytes(data)
        out = subprocess.run([cli, str(src), str(dst), "--luma"] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        want = luma_decode(mjx, gpu_ctx, [data], **kw)[0]
        raw = dst.read_bytes()
        head = b"P5\n%d %d\n255\n" % (want.shape[1], want.shape[0])
        assert raw[:len(head)] == head and raw[len(head):] == want.tobytes(), (lname, raw[:20])

"""YCbCr output (include/mjx.h: mjx_planes): a picture leaves as its component planes at their own sampling -- I420, NV12.

The references, none of which is the code under test:
  1  the component twin: the one-component file that carries component c's coefficient blocks and quantisation table (in the manner
     of test_luma_output.twin_of); the R byte of its PACKED decode at the same scale is the sample -- bit for bit;
  2  the float64 plane (scaled_ref.planes, + 128 on every component) with the project's K = 64 half-ulps of the block's magnitude:
     every sample lies in [lo, hi]; at scales 1 and 1/2 the interval decides at least 98 % of every plane (CAP).  At 1/4 and 1/8 a
     flat block's samples are exact multiples of 1/8 in float64 itself, so whole levels sit on the truncation's edge and the interval
     cannot decide them -- there the samples are still required inside it, and the share is printed, as test_luma_output does;
  3  libjpeg_ref.component_planes rounded, for pixels="libjpeg", and mjx_upsample_color_host on the decoded planes against the packed
     "libjpeg" decode of the same file;
  4  the plane geometry written out in plain Python from the header's formulas.
"""
import ctypes
import functools
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
import test_luma_output as tlo
import test_output_formats as tof
import test_sampling_layouts as tsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tsl.NAMES
Y420, Y422, Y440, LUMA_SUB = tlp.Y420, tlp.Y422, tlp.Y440, tlp.LUMA_SUB
K, CAP = tlo.K, tlo.CAP
SCALES = (1, 2, 4, 8)
LARGE = [Y420, Y422, Y440, LUMA_SUB]
ESZ = {"uint8": 1, "float16": 2, "float32": 4}


def cdiv(a, b):
    return -(-a // b)


def hv_of(lname):
    return [(1, 1)] if lname.startswith("gray") else tsl.parse_name(lname)


# ---- reference 4: the geometry, from the header's text ----------------------------------------------------------------------------
def geometry(hv, W, H, s, rect=None):
    """-> [(x0, y0, w, h) of plane c] for the rectangle (x, y, w, h) of the ceil(W/s) x ceil(H/s) picture (None: the whole picture)"""
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    ow, oh = cdiv(W, s), cdiv(H, s)
    x, y, w, h = rect if rect else (0, 0, ow, oh)
    out = []
    for hc, vc in hv:
        x0, x1 = x * hc // hmax, cdiv((x + w) * hc, hmax)
        y0, y1 = y * vc // vmax, cdiv((y + h) * vc, vmax)
        out.append((x0, y0, x1 - x0, y1 - y0))
    return out


# ---- reference 1: the component twin ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def comp_twin(lname, w, h, c, restart=None, quality=75, noise=4.0):
    """The one-component file that carries component c of tsl.layout_file(lname, w, h): its blocks over the component's own grid
    (T.81 A.2.2: ceil(wc / 8) x ceil(hc / 8)), its quantisation table, Huffman tables that hold every symbol."""
    data, per_comp = tsl.layout_file(lname, w, h, restart=restart, quality=quality, noise=noise)
    if lname.startswith("gray"):
        return data
    hv = tsl.parse_name(lname)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mcux, mcuy = cdiv(w, 8 * hmax), cdiv(h, 8 * vmax)
    hc, vc = hv[c]
    wc, hc_px = cdiv(w * hc, hmax), cdiv(h * vc, vmax)
    grid = np.asarray(per_comp[c]).reshape(mcuy, mcux, vc, hc, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy * vc, mcux * hc, 64)
    bx, by = cdiv(wc, 8), cdiv(hc_px, 8)
    blocks = grid[:by, :bx].reshape(-1, 64)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    tables = {(0, 0): jw.small_dc_table(11), (1, 0): jw.full_ac_table()}
    return jw.jpeg_from_blocks(blocks, [(1, 1)], bx, by, [qt[comps[c][2]]], tables, width=wc, height=hc_px)


# ---- reference 2: float64 -------------------------------------------------------------------------------------------------------------
def planes_f64(data, s):
    """-> [(w, lo, hi) per component]: the float64 plane of the component's true size at 1/s (+ 128 on every component) and the bytes
    a float32 decoder may give: K half-ulps of the block's magnitude (its own + 128 included) to either side, truncated."""
    dec = tsl.oracle_std(data)
    W, H, comps, pl, hmax, vmax = scaled_ref.planes(data, s, dec)
    mag = scaled_ref.planes(data, s, dec, magnitude=True)[3]
    ow, oh = cdiv(W, s), cdiv(H, s)
    out = []
    for c, ((hc, vc, _), p, m) in enumerate(zip(comps, pl, mag)):
        cw, ch = cdiv(ow * hc, hmax), cdiv(oh * vc, vmax)
        w = p[:ch, :cw] + (128.0 if c else 0.0)
        d = K * 2.0 ** -24 * (m[:ch, :cw] + (128.0 if c else 0.0))
        out.append((w, scaled_ref.trunc_u8(w - d), scaled_ref.trunc_u8(w + d)))
    return out


def interval_problem(got, data, s):
    for c, ((_, lo, hi), g) in enumerate(zip(planes_f64(data, s), got)):
        if not isinstance(g, np.ndarray) or g.shape != lo.shape:
            return (c, "shape", getattr(g, "shape", g), lo.shape)
        out = (g < lo) | (g > hi)
        share = float((lo != hi).mean())
        if out.any() or (s <= 2 and share > CAP):
            return (c, "outside %d of %d, first at %s; undecided share %.4f" % (int(out.sum()), out.size, np.argwhere(out)[:2].tolist(), share))
    return None


def lj_planes(data):
    """reference 3 -> [(rounded plane, lo, hi) per component] uint8, of the components' true sizes"""
    dec = tsl.oracle_std(data)
    _, _, pl, _ = lj.component_planes(data, dec)
    _, _, mag, _ = lj.component_planes(data, dec, magnitude=True)
    out = []
    for c, (p, m) in enumerate(zip(pl, mag)):
        d = K * 2.0 ** -24 * (m + (128.0 if c else 0.0))
        out.append(tuple(lj.round_u8(v).astype(np.uint8) for v in (p, p - d, p + d)))
    return out


GPU_FILES = [(n, 61, 45) for n in NAMES] + [(n, 333, 217) for n in LARGE]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
LAYOUT_SIZES = [(1, 1), (2, 7), (7, 8), (8, 9), (9, 15), (15, 16), (16, 17), (17, 31), (31, 33), (33, 61), (61, 333), (333, 2)]


def rects_of(ow, oh):
    r = [(0, 0, 1, 1), (ow - 1, oh - 1, 1, 1), (ow - 1, 0, 1, oh), (0, oh - 1, ow, 1), (1, 1, ow - 1, oh - 1), (3, 5, 9, 7), (5, 3, 2, 1), (ow // 2, oh // 3, 3, 3)]
    return [q for q in r if q[2] > 0 and q[3] > 0 and q[0] + q[2] <= ow and q[1] + q[3] <= oh]


@pytest.mark.parametrize("part", range(4))
def test_planes_layout_is_the_headers_formulas(mjx, part):
    checked = 0
    for k, lname in enumerate(NAMES[part * 16:(part + 1) * 16] + (["gray22"] if part == 0 else [])):
        hv = hv_of(lname)
        equal_chroma = len(hv) == 3 and hv[1] == hv[2]
        for W, H in LAYOUT_SIZES[k % 3::3] + [LAYOUT_SIZES[(k + part) % 12]]:
            scan = mjx.ParsedScan(tsl.data_of(lname, W, H))
            try:
                for s in SCALES:
                    ow, oh = cdiv(W, s), cdiv(H, s)
                    for rect in [None] + rects_of(ow, oh):
                        want = geometry(hv, W, H, s, rect)
                        for il in (False, True):
                            for dtype in (("uint8", "float32") if rect is None else ("float16",)):
                                pl = mjx.Planes(dtype, interleave=il)
                                if il and len(hv) == 3 and not equal_chroma:
                                    with pytest.raises(mjx.MjxError) as e:
                                        scan.planes_layout(pl, roi=rect, scale=s)
                                    assert e.value.code == mjx.ERR_INVALID_ARG
                                    continue
                                lay = scan.planes_layout(pl, roi=rect, scale=s)
                                pair = il and len(hv) == 3
                                assert lay["nplanes"] == (1 if len(hv) == 1 else 2 if pair else 3), (lname, lay)
                                for c, (_, _, w, h) in enumerate(want):
                                    assert (lay["width"][c], lay["height"][c]) == (w, h), (lname, W, H, s, rect, c, lay, want)
                                    if c < lay["nplanes"]:
                                        assert lay["row_pitch"][c] == (2 * w if pair and c == 1 else w) and lay["dev"][c] == 0, (lname, c, lay)
                                assert lay["bytes"] == sum(w * h for _, _, w, h in want) * ESZ[dtype], (lname, W, H, s, rect, lay, want)
                                checked += 1
                # caller-owned planes: pointers and pitches are echoed
                want = geometry(hv, W, H, 1)
                dst = [([(4096 * (c + 1), w + 3 + c) for c, (_, _, w, h) in enumerate(want)], [(w, h) for _, _, w, h in want])]
                lay = scan.planes_layout(mjx.Planes("float16", dst=dst))
                for c, (_, _, w, h) in enumerate(want):
                    assert (lay["dev"][c], lay["row_pitch"][c]) == (4096 * (c + 1), w + 3 + c), lay
                assert lay["bytes"] == sum(((h - 1) * (w + 3 + c) + w) * 2 for c, (_, _, w, h) in enumerate(want)), lay
            finally:
                scan.close()
    assert checked > 200


def _code(mjx, fn):
    try:
        fn()
    except mjx.MjxError as e:
        return e.code
    return mjx.OK


def test_every_refusal_is_the_pictures_own(mjx):
    W, H = 61, 45
    good, odd = tsl.data_of(Y420, W, H), tsl.data_of("Y22_Cb21_Cr11", W, H)
    sg = mjx.ParsedScan(good)
    so = mjx.ParsedScan(odd)
    try:
        geo = geometry(hv_of(Y420), W, H, 1)
        sizes = [(w, h) for _, _, w, h in geo]
        ok_dst = ([(4096, sizes[0][0]), (8192, sizes[1][0]), (12288, sizes[2][0])], sizes)
        INV = mjx.ERR_INVALID_ARG
        layout = lambda scan, pl, **kw: _code(mjx, lambda: scan.planes_layout(pl, **kw))
        assert layout(sg, mjx.Planes("uint8")) == mjx.OK and layout(so, mjx.Planes("uint8")) == mjx.OK
        assert layout(sg, mjx.Planes(7)) == INV                                                        # unknown dtype
        # REF_COMPAT (a file the reference's own layout accepts: the refusal is the description's, the picture's own fault comes first)
        sr = mjx.ParsedScan(mjx.synth_jpeg(64, 48, "420", 75, seed=1))
        try:
            assert sr.validate(layout=mjx.LAYOUT_REF_COMPAT) == mjx.OK and layout(sr, mjx.Planes("uint8")) == mjx.OK
            assert layout(sr, mjx.Planes("uint8"), layout=mjx.LAYOUT_REF_COMPAT) == INV
        finally:
            sr.close()
        assert layout(so, mjx.Planes("uint8", interleave=True)) == INV                                 # unequal chroma factors
        assert layout(sg, mjx.Planes("uint8", interleave=True)) == mjx.OK
        assert layout(sg, mjx.Planes("uint8", dst=[ok_dst])) == mjx.OK
        for c in range(3):
            bad_size = [list(sizes), list(sizes)]
            bad_size[0][c] = (sizes[c][0] + 1, sizes[c][1])
            bad_size[1][c] = (sizes[c][0], sizes[c][1] - 1)
            for bs in bad_size:
                assert layout(sg, mjx.Planes("uint8", dst=[(ok_dst[0], bs)])) == INV                  # a destination of another size
            short = list(ok_dst[0])
            short[c] = (short[c][0], sizes[c][0] - 1)
            assert layout(sg, mjx.Planes("uint8", dst=[(short, sizes)])) == INV                       # a pitch too small
            null = list(ok_dst[0])
            null[c] = (0, sizes[c][0])
            assert layout(sg, mjx.Planes("uint8", dst=[(null, sizes)])) == INV                        # a NULL pointer
            mis = list(ok_dst[0])
            mis[c] = (mis[c][0] + 2, sizes[c][0])
            assert layout(sg, mjx.Planes("float32", dst=[(mis, sizes)])) == INV                       # misaligned for the element size
            assert layout(sg, mjx.Planes("float16", dst=[(mis, sizes)])) == mjx.OK
            for what in ("scale", "bias"):
                v = [1.0, 1.0, 1.0]
                v[c] = float("inf") if what == "scale" else float("nan")
                assert layout(sg, mjx.Planes("float32", **{what: v})) == INV                          # non-finite, float dtype
                assert layout(sg, mjx.Planes("uint8", **{what: v})) == mjx.OK
        # the interleaved plane: dev[2] is ignored, the pitch counts both components
        nv = [(4096, sizes[0][0]), (8192, 2 * sizes[1][0]), (0, 0)]
        assert layout(sg, mjx.Planes("uint8", interleave=True, dst=[(nv, sizes)])) == mjx.OK
        nv[1] = (8192, 2 * sizes[1][0] - 1)
        assert layout(sg, mjx.Planes("uint8", interleave=True, dst=[(nv, sizes)])) == INV
        assert layout(sg, mjx.Planes("uint8"), pixels="libjpeg") == mjx.OK
        assert layout(sg, mjx.Planes("uint8"), pixels="libjpeg", scale=2) == INV                       # libjpeg's pixels: full size only
        for r in ((0, 0, W + 1, 1), (W, 0, 1, 1), (0, 0, 0, 5), (5, 5, W - 4, 1)):
            assert layout(sg, mjx.Planes("uint8"), roi=r) == INV                                       # the rectangle's own rules
        # dst[i] is input i's: a wrong neighbour in the same description does not touch the picture, and the other way round
        two = [ok_dst, (ok_dst[0], [(sizes[0][0] + 1, sizes[0][1]), sizes[1], sizes[2]])]
        assert layout(sg, mjx.Planes("uint8", dst=two), i=0) == mjx.OK and layout(sg, mjx.Planes("uint8", dst=two), i=1) == INV
        assert layout(sg, mjx.Planes("uint8", dst=two[::-1]), i=0) == INV and layout(sg, mjx.Planes("uint8", dst=two[::-1]), i=1) == mjx.OK
        # n_dst: as mjx_output's
        assert layout(sg, mjx.Planes("uint8", dst=[ok_dst]), i=1) == INV
        # a one-component file has one plane; dev[1..2] and interleave have no meaning
        s1 = mjx.ParsedScan(tsl.data_of("gray22", W, H))
        try:
            lay = s1.planes_layout(mjx.Planes("uint8", interleave=True, dst=[([(4096, W + 1), (0, 0), (0, 0)], [(W, H), (0, 0), (0, 0)])]))
            assert lay["nplanes"] == 1 and lay["width"][0] == W and lay["row_pitch"][0] == W + 1, lay
        finally:
            s1.close()
    finally:
        sg.close()
        so.close()


def _members(text, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first = True
        for part in decl.split(","):
            ident = re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part.split("[")[0])
            out.append(ident[-1])
            first = False
    return out


def test_the_structs_are_mirrored_member_for_member(mjx):
    with open(os.path.join(ROOT, "include", "mjx.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as f:
        rust = f.read()
    for name, cls in (("mjx_planes", mjx.PlanesDesc), ("mjx_plane_layout", mjx.PlaneLayout)):
        want = _members(header, name)
        assert [n for n, _ in cls._fields_] == want, (name, want)
        m = re.search(r"pub struct %s \{(.*?)\n\}" % name, rust, re.S)
        assert re.findall(r"pub ([a-z_]+):", m.group(1)) == want, (name, want)
    assert _members(header, "mjx_planes") == ["dtype", "interleave_chroma", "scale", "bias", "dst", "n_dst"]
    assert _members(header, "mjx_plane_layout") == ["dev", "row_pitch", "width", "height"]
    assert "#define MJX_ABI_VERSION 2" in header
    for fn in ("mjx_batch_create_planes", "mjx_decode_batch_planes", "mjx_planes_layout", "mjx_batch_plane_info", "mjx_batch_copy_planes"):
        assert fn in mjx.SYMBOLS and ("pub fn %s(" % fn) in rust and hasattr(mjx.lib(), fn), fn


@pytest.mark.parametrize("part", range(4))
def test_the_references_are_fit_for_their_job(orc, part):
    """The component twin keeps component c's coefficients under the oracle; float64 of the twin is float64 of the plane at every scale;
    the interval decides at least 98 % of every plane at scales 1 and 1/2 and contains float64's own byte at every scale."""
    cases = GPU_FILES[part * 17:(part + 1) * 17]
    bad, worst, worst48 = [], 0.0, 0.0
    for lname, w, h in cases:
        data = tsl.data_of(lname, w, h)
        hv = hv_of(lname)
        hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
        mcux, mcuy = cdiv(w, 8 * hmax), cdiv(h, 8 * vmax)
        da = tsl.oracle_std(data)
        for c, (hc, vc) in enumerate(hv):
            tw = comp_twin(lname, w, h, c)
            dt = tsl.oracle_std(tw)
            grid = da.coefs[c].reshape(mcuy, mcux, vc, hc, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy * vc, mcux * hc, 64)
            wc, hc_px = cdiv(w * hc, hmax), cdiv(h * vc, vmax)
            if not np.array_equal(dt.coefs[0].reshape(cdiv(hc_px, 8), cdiv(wc, 8), 64), grid[:cdiv(hc_px, 8), :cdiv(wc, 8)]):
                bad.append((lname, w, h, c, "the twin's coefficients"))
        for s in SCALES:
            for c, (wf, lo, hi) in enumerate(planes_f64(data, s)):
                y = scaled_ref.to_u8(wf)
                t = scaled_ref.scaled_rgb(comp_twin(lname, w, h, c), s)
                if t.shape[:2] != y.shape or not np.array_equal(t[:, :, 0], y):
                    bad.append((lname, w, h, s, c, "float64 twin"))
                share = float((lo != hi).mean())
                if s <= 2:
                    worst = max(worst, share)
                else:
                    worst48 = max(worst48, share)
                if ((y < lo) | (y > hi)).any() or (s <= 2 and share > CAP):
                    bad.append((lname, w, h, s, c, "undecided %.4f" % share))
    print("largest undecided share of a plane: %.4f at scales 1, 1/2; %.4f at 1/4, 1/8" % (worst, worst48))
    assert bad == [], bad[:8]


def test_the_libjpeg_planes_interval_decides(orc):
    worst = 0.0
    for lname, w, h in [(n, 61, 45) for n in NAMES[::5]] + [(n, 333, 217) for n in LARGE]:
        for p, lo, hi in lj_planes(tsl.data_of(lname, w, h)):
            worst = max(worst, float((lo != hi).mean()))
            assert not ((p < lo) | (p > hi)).any()
    print("largest undecided share of a rounded plane: %.4f" % worst)
    assert worst <= CAP, worst


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def planes_decode(mjx, ctx, datas, planes=None, **kw):
    """-> [the tuple of planes, or ('status', code)] of a Batch of parsed scans"""
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, planes=planes or mjx.Planes("uint8"), **kw)
    try:
        b.decode()
        b.wait()
        return [b.planes(i) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


def same_planes(a, b):
    return isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and all(tof.same_bits(np.ascontiguousarray(x), np.ascontiguousarray(y)) for x, y in zip(a, b))


def twin_problems(mjx, ctx, cases, scales):
    datas = [tsl.data_of(*c) for c in cases]
    twins, owner = [], []
    for k, (n, w, h) in enumerate(cases):
        for c in range(len(hv_of(n))):
            twins.append(comp_twin(n, w, h, c))
            owner.append((k, c))
    bad = []
    for s in scales:
        got = planes_decode(mjx, ctx, datas, scale=s)
        want = tlo.packed_decode(mjx, ctx, twins, scale=s)
        for (k, c), t in zip(owner, want):
            g = got[k]
            if not isinstance(g, tuple) or not isinstance(t, np.ndarray):
                bad.append((cases[k], s, c, g if not isinstance(g, tuple) else t))
            elif len(g) != len(hv_of(cases[k][0])) or not tof.same_bits(np.ascontiguousarray(g[c]), np.ascontiguousarray(t[:, :, 0])):
                bad.append((cases[k], s, c, g[c].shape, t.shape[:2], int((g[c] != t[:, :, 0]).sum()) if g[c].shape == t.shape[:2] else "shape"))
        for k, g in enumerate(got):
            if isinstance(g, tuple):
                p = interval_problem(g, datas[k], s)
                if p:
                    bad.append((cases[k], s, p))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_every_plane_is_its_component_twins_byte(mjx, gpu_ctx, scale):
    bad = twin_problems(mjx, gpu_ctx, GPU_FILES + [("gray22", 61, 45)], [scale])
    assert bad == [], bad[:6]


@pytest.mark.gpu
def test_plane_0_is_the_luminance_output(mjx, gpu_ctx):
    cases = [c for c in GPU_FILES if hv_of(c[0])[0] == (max(a for a, _ in hv_of(c[0])), max(b for _, b in hv_of(c[0])))] + [("gray22", 61, 45)]
    datas = [tsl.data_of(*c) for c in cases]
    bad = []
    for s in SCALES:
        got = planes_decode(mjx, gpu_ctx, datas, scale=s)
        L = tlo.luma_decode(mjx, gpu_ctx, datas, scale=s)
        bad += [(c, s) for c, g, l in zip(cases, got, L) if not isinstance(g, tuple) or not tsl.same(np.ascontiguousarray(g[0]), l)]
    rect = (3, 5, 40, 30)
    got = planes_decode(mjx, gpu_ctx, datas, rois=rect)
    L = tlo.luma_decode(mjx, gpu_ctx, datas, rois=rect)
    bad += [(c, rect) for c, g, l in zip(cases, got, L) if not isinstance(g, tuple) or not tsl.same(np.ascontiguousarray(g[0]), l)]
    assert len(cases) > 20 and bad == [], bad[:6]


@pytest.mark.gpu
def test_libjpeg_pixels_are_the_rounded_planes_and_close_the_loop(mjx, gpu_ctx):
    cases = [(n, 61, 45) for n in NAMES[::3]] + [(n, 333, 217) for n in LARGE] + [("gray22", 61, 45)]
    datas = [tsl.data_of(*c) for c in cases]
    got = planes_decode(mjx, gpu_ctx, datas, pixels="libjpeg")
    packed = tlo.packed_decode(mjx, gpu_ctx, datas, pixels="libjpeg")
    bad = []
    for c, d, g, p in zip(cases, datas, got, packed):
        if not isinstance(g, tuple):
            bad.append((c, g))
            continue
        for k, ((_, lo, hi), pl) in enumerate(zip(lj_planes(d), g)):
            if pl.shape != lo.shape or ((pl < lo) | (pl > hi)).any():
                bad.append((c, k, "outside the rounded interval"))
        hv = hv_of(c[0])
        hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
        rgb = mjx.upsample_color_host(list(g), [hmax // a for a, _ in hv], [vmax // b for _, b in hv], (0, 0, c[1], c[2]))
        if not tsl.same(rgb, p):
            bad.append((c, "upsampled planes != the packed libjpeg decode"))
    assert bad == [], bad[:6]
    # ... and a scale is refused, per picture
    st = planes_decode(mjx, gpu_ctx, datas[:2], pixels="libjpeg", scale=2)
    assert st == [("status", mjx.ERR_INVALID_ARG)] * 2, st


@pytest.mark.gpu
@pytest.mark.parametrize("lname", [Y420, Y422, Y440, LUMA_SUB, "Y22_Cb21_Cr12", "gray22"])
def test_rectangles_are_the_crop_of_the_whole_pictures_planes(mjx, gpu_ctx, lname):
    bad = []
    hv = hv_of(lname)
    for W, H in ((333, 217), (61, 45)):
        data = tsl.data_of(lname, W, H)
        for s in SCALES:
            w, h = cdiv(W, s), cdiv(H, s)
            full = planes_decode(mjx, gpu_ctx, [data], scale=s)[0]
            assert isinstance(full, tuple)
            n = 8 // s
            rects = tlp.rectangles(w, h, n * max(a for a, _ in hv), n * max(b for _, b in hv))     # (odd origins, 1 x 1 corners, edges: chroma bounds round outward)
            assert len(rects) >= 8, rects
            got = planes_decode(mjx, gpu_ctx, [data] * len(rects), scale=s, rois=rects)
            for r, g in zip(rects, got):
                want = tuple(np.ascontiguousarray(f[y0:y0 + ph, x0:x0 + pw]) for f, (x0, y0, pw, ph) in zip(full, geometry(hv, W, H, s, r)))
                if not same_planes(g, want):
                    bad.append((W, H, s, r, [getattr(p, "shape", p) for p in (g if isinstance(g, tuple) else [g])]))
    assert bad == [], bad[:8]
    tiles = mjx.plan_tiles(tsl.data_of(lname, 333, 217), roi=(120, 90, 40, 30))
    assert tiles["tiles_read"] < tiles["tiles_total"], tiles


@pytest.mark.gpu
def test_one_mcu_wide_one_mcu_tall_and_tiles_that_wrap(mjx, gpu_ctx):
    # one MCU wide and one MCU tall (a tile then spans many MCU rows / is one short run), a picture narrower than a tile so that a
    # tile wraps through several MCU rows (24 x 600 4:2:0: two MCUs per row), a one-component file: one plane
    cases = [(Y420, 16, 600), (Y420, 600, 16), (Y420, 24, 600), (Y422, 9, 333), (LUMA_SUB, 333, 9), ("Y22_Cb22_Cr22", 24, 200), ("gray22", 24, 600), ("gray12", 7, 5)]
    bad = twin_problems(mjx, gpu_ctx, cases, SCALES)
    assert bad == [], bad[:6]
    got = planes_decode(mjx, gpu_ctx, [tsl.data_of("gray22", 24, 600)])[0]
    assert len(got) == 1 and got[0].shape == (600, 24)


FMT_FILES = [(Y420, 333, 217), (Y422, 61, 45), ("gray22", 61, 45), (LUMA_SUB, 333, 217), ("Y11_Cb11_Cr11", 61, 45)]
FMT_ROIS = [None, (3, 5, 40, 30), None, (101, 50, 99, 77), (1, 1, 1, 1)]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def expected_planes(u8, fmt):
    """the u8 planes pushed through the dtype's table per COMPONENT (exact arithmetic, tof.exact_table); interleaved: Cb, Cr pairs"""
    if fmt.numpy_dtype() == np.uint8:
        out = [np.ascontiguousarray(p) for p in u8]
    else:
        t = tof.exact_table(fmt.scale, fmt.bias)
        out = [np.ascontiguousarray((t[c] if fmt.numpy_dtype() == np.float32 else t[c].astype(np.float16))[p]) for c, p in enumerate(u8)]
    if fmt.interleave and len(out) == 3:
        out = [out[0], np.ascontiguousarray(np.stack([out[1], out[2]], axis=2))]
    return tuple(out)


@pytest.mark.gpu
def test_formats_are_the_table_on_the_u8_planes_and_nv12_is_the_pairs(mjx, gpu_ctx):
    datas = [tsl.data_of(*c) for c in FMT_FILES]
    bad = []
    for s in (1, 2, 8):
        rois = FMT_ROIS if s == 1 else [None if r is None else (r[0] // s, r[1] // s, max(1, r[2] // s), max(1, r[3] // s)) for r in FMT_ROIS]
        u8 = planes_decode(mjx, gpu_ctx, datas, scale=s, rois=rois)
        assert all(isinstance(p, tuple) for p in u8), u8
        for d in tof.DTYPES:
            for il in (False, True):
                fmt = mjx.Planes(d, interleave=il) if d == "uint8" else mjx.Planes(d, interleave=il, mean=MEAN, std=STD)
                got = planes_decode(mjx, gpu_ctx, datas, planes=fmt, scale=s, rois=rois)
                for i, g in enumerate(got):
                    hv = hv_of(FMT_FILES[i][0])
                    if il and len(hv) == 3 and hv[1] != hv[2]:           # (unequal chroma factors: refused, the others unaffected)
                        if g != ("status", mjx.ERR_INVALID_ARG):
                            bad.append((s, d, il, FMT_FILES[i], "accepted"))
                    elif not same_planes(g, expected_planes(u8[i], fmt)):
                        bad.append((s, d, il, FMT_FILES[i]))
    assert bad == [], bad[:8]


SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", tof.DTYPES)
@pytest.mark.parametrize("il", [False, True], ids=["i420", "nv12"])
def test_caller_owned_planes_padded_rows_and_guards(mjx, gpu_ctx, dtype, il):
    """One allocation holds every picture's planes at padded pitches with gaps in front of, between and behind them, sentinel-filled;
    a damaged file and a picture with a wrong plane size leave their slots untouched; the pipelined call carries dst[i] with file i."""
    cases = [(Y420, 61, 45), (Y422, 61, 45), (Y420, 61, 45), ("gray22", 61, 45), (Y420, 333, 217), (Y420, 61, 45)]
    datas = [tsl.data_of(*c) for c in cases]
    damaged, wrong = 2, 5
    datas[damaged] = datas[damaged][:len(datas[damaged]) // 2]
    rois = [None, (3, 5, 40, 30), None, None, (101, 50, 99, 77), None]
    esz = ESZ[dtype]
    hip = tof._hip(mjx)
    geo, dst, spans, at = [], [], [], 4096
    for i, (n, W, H) in enumerate(cases):
        g = geometry(hv_of(n), W, H, 1, rois[i])
        pair = il and len(g) == 3
        planes, sizes = [], [(w + (1 if i == wrong and c == 0 else 0), h) for c, (_, _, w, h) in enumerate(g)]
        for c, (_, _, w, h) in enumerate(g[:2] if pair else g):
            row = 2 * w if pair and c == 1 else w
            pitch = row + 3 + c
            planes.append((at, pitch, row, h))
            at += ((h - 1) * pitch + row) * esz + 64                      # (a gap behind every plane, multiples of the element size)
            at = (at + 3) & ~3
        geo.append(g)
        spans.append(planes)
        dst.append(([(p, pitch) for p, pitch, _, _ in planes] + [(0, 0)] * (3 - len(planes)), sizes + [(0, 0)] * (3 - len(sizes))))
    total = at + 4096
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [([(base.value + p if p else 0, pitch) for p, pitch in pl], sz) for pl, sz in dst]
        fmt = mjx.Planes(dtype, interleave=il) if dtype == "uint8" else mjx.Planes(dtype, interleave=il, mean=MEAN, std=STD)
        u8 = planes_decode(mjx, gpu_ctx, [d for i, d in enumerate(datas) if i != damaged], rois=[r for i, r in enumerate(rois) if i != damaged])
        u8.insert(damaged, None)
        fmt_dst = mjx.Planes(dtype, interleave=il, scale=fmt.scale, bias=fmt.bias, dst=dst)
        b, st = mjx.decode_batch(gpu_ctx, datas, rois=rois, planes=fmt_dst, chunk_images=2)
        try:
            good = [i for i in range(len(cases)) if i not in (damaged, wrong)]
            assert st[wrong] == mjx.ERR_INVALID_ARG and st[damaged] not in (mjx.OK, mjx.ERR_INVALID_ARG) and [st[i] for i in good] == [mjx.OK] * len(good), st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            covered = np.zeros(total, bool)
            for i in good:
                want = expected_planes(u8[i], fmt)
                inf = b.plane_info(i)
                assert inf["nplanes"] == len(want) and inf["dtype"] == fmt.dtype and inf["interleave"] == (il and len(geo[i]) == 3), inf
                for c, ((p, pitch, row, h), w) in enumerate(zip(spans[i], want)):
                    assert (inf["dev"][c], inf["row_pitch"][c]) == (base.value + p, pitch), (i, c, inf)
                    el = np.arange(h)[:, None] * pitch + np.arange(row)[None, :]
                    slot = mem[p: p + ((h - 1) * pitch + row) * esz].view(fmt.numpy_dtype())
                    assert tof.same_bits(np.ascontiguousarray(slot[el]).reshape(w.shape), w), ("picture", i, "plane", c)
                    covered[(p + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)] = True
                with pytest.raises(mjx.MjxError):
                    b.planes(i)                                          # mjx_batch_copy_planes serves library-owned planes only
            assert np.all(mem[~covered] == SENTINEL), ("bytes outside the planes' elements were written", np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist())
            # (mjx_batch_bytes counts the pictures that were planned: the damaged one fails in the decode)
            assert b.bytes()["rgb"] == sum(sum(w * h for _, _, w, h in geo[i]) for i in good + [damaged]) * esz
            with pytest.raises(mjx.MjxError):
                b.tile(2)                                                # (the copies would share the destinations)
        finally:
            b.close()
    finally:
        assert hip.hipFree(base) == 0


def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    W, H = 61, 45
    datas = [tsl.data_of(Y420, W, H), tsl.data_of(Y420, W, H, quality=85), tsl.data_of(Y420, W, H, noise=12.0)]
    n = len(datas)
    ref, _ = mjx.decode_batch(ctx, datas, planes=mjx.Planes("uint8"))
    u8 = [ref.planes(i) for i in range(n)]
    ref.close()
    dev = torch.device("cuda", 0)
    (_, _, wy, hy), (_, _, wc, hc), _ = geometry(hv_of(Y420), W, H, 1)
    # three planes, float32, padded rows (a slice of a wider tensor), per-component mean / std
    y = torch.full((n, hy, wy + 5), 7.0, dtype=torch.float32, device=dev)
    cb = torch.full((n, hc, wc + 3), 7.0, dtype=torch.float32, device=dev)
    cr = torch.full((n, hc + 2, wc), 7.0, dtype=torch.float32, device=dev)
    st = mjx.decode_planes_into(ctx, datas, y[:, :, :wy], cb[:, :, :wc], cr[:, :hc, :], mean=MEAN, std=STD)
    torch.cuda.synchronize()
    fmt = mjx.Planes("float32", mean=MEAN, std=STD)
    for i in range(n):
        want = expected_planes(u8[i], fmt)
        for k, (t, w_) in enumerate(((y, wy), (cb, wc), (cr, wc))):
            g = t[i].cpu().numpy()
            hh = want[k].shape[0]
            if st[i] != 0 or not tof.same_bits(np.ascontiguousarray(g[:hh, :w_]), want[k]) or not (g[:hh, w_:] == 7.0).all() or not (g[hh:] == 7.0).all():
                bad.append(("three planes", i, k, st[i]))
    # NV12: uint8 Y and N x Hc x Wc x 2, padded rows
    y8 = torch.full((n, hy, wy + 4), 9, dtype=torch.uint8, device=dev)
    cc = torch.full((n, hc, wc + 2, 2), 9, dtype=torch.uint8, device=dev)
    st = mjx.decode_planes_into(ctx, datas, y8[:, :, :wy], cbcr=cc[:, :, :wc, :])
    torch.cuda.synchronize()
    for i in range(n):
        gy, gc = y8[i].cpu().numpy(), cc[i].cpu().numpy()
        ok = st[i] == 0 and np.array_equal(gy[:, :wy], u8[i][0]) and (gy[:, wy:] == 9).all()
        ok = ok and np.array_equal(gc[:, :wc, 0], u8[i][1]) and np.array_equal(gc[:, :wc, 1], u8[i][2]) and (gc[:, wc:] == 9).all()
        if not ok:
            bad.append(("nv12", i, st[i]))
    # what is refused before anything runs
    for args, kw in (((y[:, :, ::2], cb, cr), {}), ((y, cb), {}), ((y8, cb, cr), {}), ((y, cb.cpu(), cr), {}), ((y8,), dict(cbcr=cc[:, :, :, :1]))):
        try:
            mjx.decode_planes_into(ctx, datas, *args, **kw)
            bad.append(("accepted", [tuple(t.shape) for t in args]))
        except mjx.MjxError as e:
            if e.code != mjx.ERR_INVALID_ARG:
                bad.append(("code", e.code))
    # a tensor of another size: the pictures' own status
    st = mjx.decode_planes_into(ctx, datas, torch.zeros((n, hy, wy + 1), dtype=torch.uint8, device=dev), cbcr=cc[:, :, :wc, :])
    if st != [mjx.ERR_INVALID_ARG] * n:
        bad.append(("size", st))
    ctx.close()
    print(json.dumps(dict(bad=bad)))


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_ycbcr_planes as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_decode_planes_into_both_forms_with_padded_rows(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["bad"] == [], res


STREAM_SCALES = (1, 2, 8)


def child_streams(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = tlp.stream_files()
    out, status = {}, {}
    for dd in (False, True):
        for s in STREAM_SCALES:
            b, st = mjx.decode_batch(ctx, [d for _, d, _ in files], device_destuff=dd, scale=s, planes=mjx.Planes("uint8"))
            for i in range(len(files)):
                key = "%d_%d_%d" % (i, dd, s)
                status[key] = st[i] or b.status(i)
                if not status[key]:
                    for c, p in enumerate(b.planes(i)):
                        out["%s_%d" % (key, c)] = p
            b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=status)))


@pytest.mark.gpu
def test_every_stream_source_gives_the_interleaved_files_planes(mjx, gpu_ctx, tmp_path):
    files = tlp.stream_files()
    want = {s: planes_decode(mjx, gpu_ctx, [d for _, d, _ in files], scale=s) for s in STREAM_SCALES}
    bad = [(files[i][0], s, "status", w) for s in STREAM_SCALES for i, w in enumerate(want[s]) if not isinstance(w, tuple)]
    bad += [(files[b][0], n, s, "in process") for s in STREAM_SCALES for i, (n, _, b) in enumerate(files) if not same_planes(want[s][i], want[s][b])]
    for k, env in enumerate(({"MJX_SINGLE_DECODE": "0"}, {"MJX_STREAM_LINEAR": "1"}, {"MJX_PLANAR_DIRECT": "0"})):
        npz = tmp_path / ("streams%d.npz" % k)
        res = run_child(tmp_path, "child_streams(%r)" % str(npz), env)
        with np.load(str(npz)) as z:
            for i, (n, _, b) in enumerate(files):
                for dd in (0, 1):
                    for s in STREAM_SCALES:
                        key = "%d_%d_%d" % (i, dd, s)
                        ok = res["status"][key] == 0 and isinstance(want[s][b], tuple)
                        ok = ok and all(tsl.same(z["%s_%d" % (key, c)], np.ascontiguousarray(p)) for c, p in enumerate(want[s][b]))
                        if not ok:
                            bad.append((files[b][0], n, sorted(env.items()), "device de-stuffing" if dd else "host de-stuffing", s, res["status"][key]))
    assert bad == [], bad[:8]


def child_groups(out_path):
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    files = group_files()
    b, st = mjx.decode_batch(ctx, files, planes=mjx.Planes("float16", mean=MEAN, std=STD), rois=[(1, 3, 50, 40)] * len(files))
    out = {}
    for i in range(len(files)):
        if not (st[i] or b.status(i)):
            for c, p in enumerate(b.planes(i)):
                out["%d_%d" % (i, c)] = p
    b.close()
    ctx.close()
    np.savez(out_path, **out)
    print(json.dumps(dict(status=list(st))))


def group_files():
    """test_luma_output's list: 3.8 MB of files, four different ones seven times -- with groups of 1 MB the pipelined call cuts it several times"""
    return tlo.group_files()


@pytest.mark.gpu
def test_the_pipelined_groups_tiles_and_a_damaged_neighbour(mjx, gpu_ctx, tmp_path):
    files = group_files()
    assert sum(len(d) for d in files) > 3 << 20
    rois = [(1, 3, 50, 40)] * len(files)
    fmt = mjx.Planes("float16", mean=MEAN, std=STD)                 # (the list holds a layout with unequal chroma factors: three planes)
    want = planes_decode(mjx, gpu_ctx, files[:4], planes=fmt, rois=rois[:4])
    assert all(isinstance(w, tuple) and len(w) in (1, 3) for w in want), want
    # more than one group: the groups' size is an environment knob of the pipelined call, so the call runs in a fresh process
    npz = tmp_path / "groups.npz"
    res = run_child(tmp_path, "child_groups(%r)" % str(npz), {"MJX_GROUP_MB": "1"})
    assert res["status"] == [0] * len(files), res
    with np.load(str(npz)) as z:
        for i in range(len(files)):
            assert all(tsl.same(z["%d_%d" % (i, c)], np.ascontiguousarray(p)) for c, p in enumerate(want[i % 4])), ("group", i)
    # Batch.tile carries the description (library-owned planes)
    scans = [mjx.ParsedScan(d) for d in files[:4]]
    base = mjx.Batch(gpu_ctx, scans, planes=fmt, rois=rois[:4])
    big = base.tile(3)
    try:
        big.decode()
        big.wait()
        for i in range(12):
            assert big.status(i) == mjx.OK and same_planes(big.planes(i), want[i % 4]), ("tile", i)
            assert not big.plane_info(i)["interleave"] and big.plane_info(i)["dtype"] == mjx.DTYPE_F16 and big.info(i)["width"] == 50
        assert big.bytes()["rgb"] == 3 * base.bytes()["rgb"]
        # the accessors of a batch with a plane description
        with pytest.raises(mjx.MjxError) as e:
            big.rgb(0)
        assert e.value.code == mjx.ERR_INVALID_ARG
        assert big.compare_rgb([0], big, [4])[0][0] == 0xffffffff
        ptr, nbytes = big.rgb_device(0)
        inf = big.plane_info(0)
        assert ptr == inf["dev"][0] and nbytes == sum(p.nbytes for p in want[0]) and big.output_info(0)["channels"] == 3
        assert big.roi(1)["x"] == 1 and big.scale(1) == 1
    finally:
        big.close()
        tsl.close_all(base, scans)
    # a damaged file beside a good one: its own status, nothing written for it, the neighbour unaffected
    cut = files[1][:len(files[1]) // 2]
    b, st = mjx.decode_batch(gpu_ctx, [files[0], cut, files[2]], planes=fmt, rois=rois[:3])
    try:
        assert st[0] == mjx.OK and st[2] == mjx.OK and st[1] != mjx.OK, st
        assert same_planes(b.planes(0), want[0]) and same_planes(b.planes(2), want[2])
        with pytest.raises(mjx.MjxError):
            b.planes(1)
    finally:
        b.close()


@pytest.mark.gpu
def test_the_default_is_untouched(mjx, gpu_ctx):
    datas = [tsl.data_of(*c) for c in FMT_FILES]

    def others():
        out = tlo.packed_decode(mjx, gpu_ctx, datas, scale=2) + tlo.luma_decode(mjx, gpu_ctx, datas)
        b, scans = tsl.decode_batch(mjx, gpu_ctx, datas, output=mjx.Output("float16", planar=True, mean=MEAN, std=STD), rois=(3, 5, 40, 30))
        try:
            return out + [b.output(i) for i in range(len(datas))]
        finally:
            tsl.close_all(b, scans)

    before = others()
    for il in (False, True):
        got = planes_decode(mjx, gpu_ctx, datas[:2], planes=mjx.Planes("float32", interleave=il, mean=MEAN, std=STD))
        assert all(isinstance(g, tuple) for g in got)
    after = others()
    assert len(before) == len(after) and all(tof.same_bits(a, b) for a, b in zip(before, after))


@pytest.mark.gpu
def test_the_cli_writes_the_batchs_planes(mjx, gpu_ctx, tmp_path):
    cli = os.path.join(ROOT, "jpeg-rust_amd", "mjx_cli")
    for lname, W, H in ((Y420, 61, 45), (Y422, 333, 217), ("gray22", 61, 45)):
        data = tsl.data_of(lname, W, H)
        src = tmp_path / "in.jpg"
        src.write_bytes(data)
        for flag, il in (("--ycc", False), ("--nv12", True)):
            for extra, kw in (([], {}), (["--scale", "2", "--crop", "3,5,20,10"], dict(scale=2, rois=(3, 5, 20, 10)))):
                out = tmp_path / "out.yuv"
                r = subprocess.run([cli, str(src), str(out), flag] + extra, capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, r.stdout + r.stderr
                want = planes_decode(mjx, gpu_ctx, [data], planes=mjx.Planes("uint8", interleave=il), **kw)[0]
                assert out.read_bytes() == b"".join(np.ascontiguousarray(p).tobytes() for p in want), (lname, flag, extra)
                for p in want:
                    assert "%dx%d" % (p.shape[1], p.shape[0]) in r.stdout, (r.stdout, p.shape)

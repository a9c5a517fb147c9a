"""YCbCr planes with a resize and / or an orientation (include/mjx.h: mjx_batch_create_planes_orient).

The references, none of which is the code under test:
  1  the existing plane decode (planes= alone) of the stored rectangle, turned by numpy's eight permutations (test_orientation.orient_np);
  2  the component twin (test_ycbcr_planes.comp_twin, wide_ref.component_file) through the EXISTING luminance resize / orientation:
     every leaving plane equals it bit for bit;
  3  the float64 rules of test_resize / test_resize_filters applied per plane, with their derived tolerances and the U8 band rule;
  4  the geometry written out in plain Python from the header's formulas.
"""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import scaled_ref
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_resize_filters as trf
import test_sampling_layouts as tsl
import test_ycbcr_planes as typ
import wide_ref as wr

ROOT = typ.ROOT
Y444, Y420, Y422, Y440, Y411, LUMA_SUB, GREY = "Y11_Cb11_Cr11", typ.Y420, typ.Y422, typ.Y440, "Y41_Cb11_Cr11", typ.LUMA_SUB, "gray22"
ESZ = typ.ESZ
cdiv, hv_of, geometry = typ.cdiv, typ.hv_of, typ.geometry
FILTERS = ("bilinear", "bicubic", "nearest")
MEAN, STD = typ.MEAN, typ.STD


# ---- the files and their component twins -------------------------------------------------------------------------------------------------
def wide(lname):
    return lname in wr.NAMES


def file_of(lname, w, h, **kw):
    return wr.layout_file(lname, w, h)[0] if wide(lname) else tsl.data_of(lname, w, h, **kw)


def twin_of(lname, w, h, c):
    """the one-component file that carries component c: its luminance picture is the plane (over the component's block grid at least)"""
    return wr.component_file(lname, w, h, c) if wide(lname) else typ.comp_twin(lname, w, h, c)


# ---- reference 4: the geometry, from the header's text ---------------------------------------------------------------------------------------
def oriented_size(code, w, h):
    return (h, w) if code >= 5 else (w, h)


def rect_to_stored(code, sw, sh, rect):
    """the rectangle of S (sw x sh) that holds the pixels of `rect` of D = orient_c(S): numpy's permutation on the pixel indices"""
    idx = np.arange(sw * sh).reshape(sh, sw)
    x, y, w, h = rect
    sub = tor.orient_np(code, idx)[y:y + h, x:x + w]
    rows, cols = sub // sw, sub % sw
    return (int(cols.min()), int(rows.min()), int(cols.max() - cols.min() + 1), int(rows.max() - rows.min() + 1))


def rect_to_oriented(code, sw, sh, rect):
    """the other way round: where the rectangle `rect` of S lies in D"""
    mark = np.zeros((sh, sw), bool)
    x, y, w, h = rect
    mark[y:y + h, x:x + w] = True
    ys, xs = np.nonzero(tor.orient_np(code, mark))
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def plan_of(hv, W, H, code, rect=None, scale=1, target=None, auto=False):
    """-> (s, R_S, spans of the intermediate's planes, leaving plane sizes): the header's contract in plain Python.  rect is D's (full-size
    D with auto); target is in D's axes."""
    s0 = 1 if auto else scale
    sw, sh = cdiv(W, s0), cdiv(H, s0)
    dw, dh = oriented_size(code, sw, sh)
    r_s = rect_to_stored(code, sw, sh, rect if rect else (0, 0, dw, dh))
    s = s0
    if auto:
        tw, th = (target[1], target[0]) if code >= 5 else target
        s, r_s = trs.auto_scale_rule(W, H, r_s, tw, th)
    spans = geometry(hv, W, H, s, r_s)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    out = []
    for (hc, vc), (_, _, w, h) in zip(hv, spans):
        if target is None:
            out.append(oriented_size(code, w, h))
        else:
            hd, vd, hm, vm = (vc, hc, vmax, hmax) if code >= 5 else (hc, vc, hmax, vmax)
            out.append((cdiv(target[0] * hd, hm), cdiv(target[1] * vd, vm)))
    return s, r_s, spans, out


def d_rects(dw, dh):
    r = [None, (1, 1, dw - 1, dh - 1), (dw // 2, dh // 3, 1, 1), (0, dh - 1, dw, 1), (dw - 1, 0, 1, dh), (3, 1, 9, 2)]
    return [q for q in r if q is None or (q[2] > 0 and q[3] > 0 and q[0] + q[2] <= dw and q[1] + q[3] <= dh)]


LAYOUT_NAMES = (Y444, Y422, Y440, Y420, Y411, LUMA_SUB, GREY)
LAYOUT_SIZES = ((1, 1), (7, 4), (17, 9), (61, 45))
AUTO_TARGETS = ((40, 30), (30, 22), (15, 11), (7, 5))              # on 61 x 45 (codes 1 .. 4): scales 1, 2, 4, 8


# ---- CPU 1: mjx_planes_orient_layout is the header's formulas ------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(1, 9))
def test_orient_layout_is_the_headers_formulas(mjx, code):
    checked, scales = 0, set()
    for lname in LAYOUT_NAMES:
        hv = hv_of(lname)
        pair_ok = len(hv) == 3 and hv[1] == hv[2]
        for W, H in LAYOUT_SIZES:
            scan = mjx.ParsedScan(file_of(lname, W, H))
            try:
                cases = []
                for s in (1, 2):
                    dw, dh = oriented_size(code, cdiv(W, s), cdiv(H, s))
                    for rect in d_rects(dw, dh):
                        for target in (None, (24, 16), (5, 9)):
                            cases.append((rect, s, target, False))
                if (W, H) == (61, 45):
                    dw, dh = oriented_size(code, W, H)
                    for t in AUTO_TARGETS:
                        t = (t[1], t[0]) if code >= 5 else t
                        cases += [(None, 1, t, True), ((1, 3, dw - 2, dh - 5), 1, t, True)]
                for rect, s, target, auto in cases:
                    want_s, want_r, _, want = plan_of(hv, W, H, code, rect, s, target, auto)
                    rs = None if target is None else mjx.Resize(target[0], target[1], auto_scale=auto, filter=FILTERS[checked % 3])
                    for il in (False, True):
                        pl = mjx.Planes(("uint8", "float16", "float32")[checked % 3], interleave=il)
                        if il and len(hv) == 3 and not pair_ok:
                            with pytest.raises(mjx.MjxError) as e:
                                scan.planes_layout(pl, roi=rect, scale=s, resize=rs, code=code)
                            assert e.value.code == mjx.ERR_INVALID_ARG
                            continue
                        lay = scan.planes_layout(pl, roi=rect, scale=s, resize=rs, code=code)
                        what = (lname, W, H, code, rect, s, target, auto, il, lay, want)
                        pair = il and len(hv) == 3
                        assert lay["scale"] == want_s and lay["rect"] == want_r, what
                        assert lay["nplanes"] == (1 if len(hv) == 1 else 2 if pair else 3), what
                        for c, (w, h) in enumerate(want):
                            assert (lay["width"][c], lay["height"][c]) == (w, h), what
                            if c < lay["nplanes"]:
                                assert lay["row_pitch"][c] == (2 * w if pair and c == 1 else w) and lay["dev"][c] == 0, what
                        assert lay["bytes"] == sum(w * h for w, h in want) * ESZ[("uint8", "float16", "float32")[checked % 3]], what
                        if auto:
                            scales.add(lay["scale"])
                        checked += 1
                # caller-owned planes: pointers and pitches are echoed, at the LEAVING planes' sizes
                for target in (None, (24, 16)):
                    _, _, _, want = plan_of(hv, W, H, code, None, 1, target)
                    dst = [([(4096 * (c + 1), w + 3 + c) for c, (w, h) in enumerate(want)], list(want))]
                    rs = None if target is None else mjx.Resize(target[0], target[1], auto_scale=False)
                    lay = scan.planes_layout(mjx.Planes("float16", dst=dst), resize=rs, code=code)
                    for c, (w, h) in enumerate(want):
                        assert (lay["dev"][c], lay["row_pitch"][c]) == (4096 * (c + 1), w + 3 + c), lay
            finally:
                scan.close()
    assert checked > 1000 and scales == {1, 2, 4, 8}, (checked, scales)


# ---- CPU 2: both descriptions NULL: mjx_planes_layout member for member ------------------------------------------------------------------------
def test_without_resize_and_orientation_the_layout_is_mjx_planes_layout(mjx):
    lib = mjx.lib()
    n = 0
    for lname in LAYOUT_NAMES:
        for W, H in LAYOUT_SIZES:
            scan = mjx.ParsedScan(file_of(lname, W, H))
            try:
                for s in (1, 2, 8):
                    for rect in d_rects(cdiv(W, s), cdiv(H, s)):
                        for il in (False, True):
                            o = mjx._opts(scale=s, rois=rect)
                            keep, ref = mjx._planes_ref(mjx.Planes("float16", interleave=il))
                            a, b, np_, nb, sc, r = mjx.PlaneLayout(), mjx.PlaneLayout(), ctypes.c_uint32(), ctypes.c_size_t(), ctypes.c_uint8(), mjx.Rect()
                            ra = lib.mjx_planes_layout(ctypes.byref(scan.desc), ctypes.byref(o), ref, 0, ctypes.byref(a), ctypes.byref(np_), ctypes.byref(nb))
                            rb = lib.mjx_planes_orient_layout(ctypes.byref(scan.desc), ctypes.byref(o), ref, None, 1, 0, ctypes.byref(b), ctypes.byref(sc), ctypes.byref(r))
                            assert ra == rb, (lname, W, H, s, rect, il, ra, rb)
                            if ra != mjx.OK:
                                continue
                            for f, _ in mjx.PlaneLayout._fields_:
                                assert list(getattr(a, f)) == list(getattr(b, f)), (lname, W, H, s, rect, il, f)
                            assert sc.value == s and (r.x, r.y, r.w, r.h) == (rect or (0, 0, cdiv(W, s), cdiv(H, s)))
                            n += 1
            finally:
                scan.close()
    assert n > 300, n


# ---- CPU 3: every refusal, one case each, with an unaffected neighbour ---------------------------------------------------------------------
def test_every_refusal_is_the_pictures_own(mjx):
    W, H = 61, 45
    sg, so = mjx.ParsedScan(file_of(Y422, W, H)), mjx.ParsedScan(file_of("Y22_Cb21_Cr11", W, H))
    try:
        INV = mjx.ERR_INVALID_ARG
        layout = lambda scan, pl, **kw: typ._code(mjx, lambda: scan.planes_layout(pl, **kw))
        rs = mjx.Resize(24, 16, auto_scale=False)
        good = dict(resize=rs, code=6)
        assert layout(sg, mjx.Planes("uint8"), **good) == mjx.OK and layout(so, mjx.Planes("uint8"), **good) == mjx.OK      # the neighbours
        assert layout(sg, mjx.Planes(7), **good) == INV                                                    # mjx_planes: unknown dtype
        assert layout(sg, mjx.Planes("uint8"), layout=mjx.LAYOUT_REF_COMPAT, **good) == INV                # ... REF_COMPAT
        assert layout(so, mjx.Planes("uint8", interleave=True), **good) == INV                             # ... unequal chroma factors
        assert layout(sg, mjx.Planes("uint8", interleave=True), **good) == mjx.OK
        assert layout(sg, mjx.Planes("float32", scale=[1.0, float("inf"), 1.0]), **good) == INV            # ... non-finite
        assert layout(sg, mjx.Planes("uint8"), pixels="libjpeg", scale=2, **good) == INV                   # ... libjpeg's pixels at a scale
        assert layout(sg, mjx.Planes("uint8"), pixels="libjpeg", **good) == mjx.OK
        # dst[i]: the LEAVING planes' sizes (code 6 without a resize: a 4:2:2 file's planes leave as 4:4:0 planes), pitches, pointers
        _, _, spans, want = plan_of(hv_of(Y422), W, H, 6)
        stored = [(w, h) for _, _, w, h in spans]
        assert want == [(h, w) for w, h in stored] and want[1] == (45, 31)
        ptrs = lambda sizes, pad=0: [(4096 * (c + 1), w + pad) for c, (w, h) in enumerate(sizes)]
        two = [(ptrs(want), want), (ptrs(stored), stored)]
        assert layout(sg, mjx.Planes("uint8", dst=two), code=6, i=0) == mjx.OK and layout(sg, mjx.Planes("uint8", dst=two), code=6, i=1) == INV
        assert layout(sg, mjx.Planes("uint8", dst=two[::-1]), code=6, i=0) == INV and layout(sg, mjx.Planes("uint8", dst=two[::-1]), code=6, i=1) == mjx.OK
        assert layout(sg, mjx.Planes("uint8", dst=[(ptrs(want, -1), want)]), code=6) == INV                # a pitch too small
        assert layout(sg, mjx.Planes("uint8", dst=[([(0, want[0][0])] + ptrs(want)[1:], want)]), code=6) == INV      # a NULL pointer
        assert layout(sg, mjx.Planes("float32", dst=[([(4098, want[0][0])] + ptrs(want)[1:], want)]), code=6) == INV  # misaligned
        tw = plan_of(hv_of(Y422), W, H, 6, None, 1, (24, 16))[3]
        assert layout(sg, mjx.Planes("uint8", dst=[(ptrs(tw), tw)]), **good) == mjx.OK
        assert layout(sg, mjx.Planes("uint8", dst=[(ptrs(want), want)]), **good) == INV                    # not the target's planes
        # mjx_resize's
        assert layout(sg, mjx.Planes("uint8"), resize=mjx.Resize(0, 16, auto_scale=False), code=6) == INV
        assert layout(sg, mjx.Planes("uint8"), resize=mjx.Resize(24, 16, auto_scale=True), code=6, scale=2) == INV
        bad_filter = rs.desc()
        bad_filter.filter = 3
        assert layout(sg, mjx.Planes("uint8"), resize=bad_filter, code=6) == INV
        # mjx_orient's: a code outside 1 .. 8; a rectangle outside D (inside S)
        assert layout(sg, mjx.Planes("uint8"), code=0) == INV and layout(sg, mjx.Planes("uint8"), code=9) == INV
        assert layout(sg, mjx.Planes("uint8"), code=6, roi=(0, 0, 61, 45)) == INV and layout(sg, mjx.Planes("uint8"), code=6, roi=(0, 0, 45, 61)) == mjx.OK
        assert layout(sg, mjx.Planes("uint8"), code=6, roi=(0, 0, 0, 5)) == INV
        # fit modes: cover composes, contain is refused
        assert layout(sg, mjx.Planes("uint8"), resize=mjx.Resize(24, 16, auto_scale=False, fit="cover"), code=6) == mjx.OK
        assert layout(sg, mjx.Planes("uint8"), resize=mjx.Resize(24, 16, auto_scale=False, fit="contain"), code=6) == INV
        assert layout(sg, mjx.Planes("uint8"), resize=mjx.Resize(24, 16, auto_scale=False, fit="contain")) == INV
    finally:
        sg.close()
        so.close()


# ---- CPU 4: the mirrors ------------------------------------------------------------------------------------------------------------------------
def test_mirrors_of_the_entry_points_and_unchanged_structs(mjx):
    with open(os.path.join(ROOT, "include", "mjx.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")) as f:
        rust = f.read()
    for fn in ("mjx_batch_create_planes_orient", "mjx_decode_batch_planes_orient", "mjx_planes_orient_layout"):
        assert fn in mjx.SYMBOLS and ("pub fn %s(" % fn) in rust and hasattr(mjx.lib(), fn) and ("int %s(" % fn) in header, fn
    assert "#define MJX_ABI_VERSION 2" in header and "MJX_K_COUNT = 11" in header
    assert typ._members(header, "mjx_planes") == ["dtype", "interleave_chroma", "scale", "bias", "dst", "n_dst"]
    assert typ._members(header, "mjx_plane_layout") == ["dev", "row_pitch", "width", "height"]
    assert typ._members(header, "mjx_resize") == ["width", "height", "antialias", "auto_scale"]
    assert typ._members(header, "mjx_orient") == ["from_exif", "extra", "n_extra"]
    assert (ctypes.sizeof(mjx.PlanesDesc), ctypes.sizeof(mjx.PlaneLayout), ctypes.sizeof(mjx.ResizeDesc), ctypes.sizeof(mjx.OrientDesc)) == (48, 72, 12, 24)
    # the C prototypes and the ctypes / Rust mirrors take the same number of arguments
    for fn in ("mjx_batch_create_planes_orient", "mjx_decode_batch_planes_orient", "mjx_planes_orient_layout"):
        proto = re.search(r"int %s\((.*?)\);" % fn, header, re.S).group(1)
        rproto = re.search(r"pub fn %s\((.*?)\) -> c_int;" % fn, rust, re.S).group(1)
        assert len(proto.split(",")) == len(mjx.SYMBOLS[fn][1]) == len(rproto.split(",")), fn


# ---- the resize sweep's cases (CPU 5 and GPU 2, 3 walk the same list) ---------------------------------------------------------------------------
SWEEP_FILES = [(Y420, 61, 45), (Y422, 61, 45), (Y411, 61, 45), (GREY, 61, 45), (Y420, 333, 217), (Y422, 333, 217), (Y411, 333, 217)]
SWEEP_TARGETS = ((24, 16), (9, 7), (1, 1), (80, 60))               # the last one an upscale: the 61 x 45 files only
NOISE = dict(quality=85, noise=12.0)                                 # the noisy generator settings (the wide layouts' writer has one setting)


def sweep_data(k):
    n, w, h = SWEEP_FILES[k]
    return file_of(n, w, h) if wide(n) else file_of(n, w, h, **NOISE)


def sweep_twin(k, c):
    n, w, h = SWEEP_FILES[k]
    return wr.component_file(n, w, h, c) if wide(n) else typ.comp_twin(n, w, h, c, **NOISE)


@functools.lru_cache(maxsize=None)
def sweep_planes_f64(k, s):
    """the float64 planes of file k at 1/s, truncated to bytes (no device): typ.planes_f64 on the oracle's coefficients; the oracle keeps
    the reference's assertion on factors of 4, so a wide layout takes the writer's own blocks, which its serial decode reads back
    (test_wide_sampling), through the same scaled_ref.planes"""
    n, w, h = SWEEP_FILES[k]
    if not wide(n):
        return [scaled_ref.trunc_u8(p) for p, _, _ in typ.planes_f64(sweep_data(k), s)]
    data, blocks = wr.layout_file(n, w, h)
    W, H, comps, pl, hmax, vmax = scaled_ref.planes(data, s, wr.dec_of(n, w, h, blocks))
    ow, oh = cdiv(W, s), cdiv(H, s)
    return [scaled_ref.trunc_u8(p[:cdiv(oh * vc, vmax), :cdiv(ow * hc, hmax)] + (128.0 if c else 0.0)) for c, ((hc, vc, _), p) in enumerate(zip(comps, pl))]


def sweep_groups():
    """-> [(target, aa, auto, [file indices])]; the filter is the tests' parameter"""
    out = []
    for target in SWEEP_TARGETS:
        ks = [k for k, (_, w, h) in enumerate(SWEEP_FILES) if target != (80, 60) or (w, h) == (61, 45)]
        for aa in (False, True):
            for auto in (False, True):
                out.append((target, aa, auto, ks))
    return out


def rule_ref(plane, target, filt, aa):
    """the float64 rule on one plane -> [H, W]"""
    p = np.asarray(plane)[:, :, None]
    r = trs.resize_ref(p, target[0], target[1], aa) if filt == "bilinear" else trf.resize_ref(p, target[0], target[1], filt, aa)
    return r[:, :, 0]


def rule_tol(src_wh, target, filt, aa):
    if filt == "bilinear":
        return trs.tolerance(trs.max_taps(src_wh[0], target[0], aa), trs.max_taps(src_wh[1], target[1], aa))
    taps = (max(trf.windows(src_wh[0], target[0], filt, aa)), max(trf.windows(src_wh[1], target[1], filt, aa)))
    return trf.tolerance(taps, src_wh, target, filt, aa)


def plane_fmt(dtype, sc, bi):
    """one plane as a planar picture of three equal channels: what test_resize.check_against takes"""
    return types.SimpleNamespace(bgr=False, planar=True, numpy_dtype=lambda: np.dtype(dtype), scale=[sc] * 3, bias=[bi] * 3)


def check_plane(got, ref, dtype, sc, bi, tol):
    g3 = np.stack([np.asarray(got)] * 3)
    return trs.check_against(g3, np.stack([ref] * 3, axis=2), plane_fmt(dtype, sc, bi), tol)


@pytest.mark.parametrize("filt", ("bilinear", "bicubic"))
def test_band_share_of_the_reference_alone_on_the_sweeps_planes(mjx, orc, filt):
    """The U8 exception (+-1 within tol of a half) must not hide a failure: on the oracle's own planes (float64, truncated) of the GPU
    sweep's files the share of U8 elements in the band stays under test_resize's cap."""
    band = total = 0
    scans = [mjx.ParsedScan(sweep_data(k)) for k in range(len(SWEEP_FILES))]
    try:
        for target, aa, auto, ks in sweep_groups():
            for k in ks:
                n, W, H = SWEEP_FILES[k]
                hv = hv_of(n)
                lay = scans[k].planes_layout(mjx.Planes("uint8"), resize=mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto, filter=filt))
                s = lay["scale"]
                planes = sweep_planes_f64(k, s)
                for c, p in enumerate(planes):
                    t = (lay["width"][c], lay["height"][c])
                    ref = rule_ref(p, t, filt, aa)
                    tol = rule_tol(p.shape[::-1], t, filt, aa)
                    band += int((np.rint(np.clip(ref - tol, 0, 255)) != np.rint(np.clip(ref + tol, 0, 255))).sum())
                    total += ref.size
    finally:
        for s in scans:
            s.close()
    print("%s: U8 elements of the sweep: %d, in the band: %d (%.3f %%)" % (filt, total, band, 100.0 * band / max(total, 1)))
    assert total > 20000 and band <= trs.BAND_CAP * total, (band, total)


# ---- GPU: shared pieces ---------------------------------------------------------------------------------------------------------------------
def po_decode(mjx, ctx, datas, planes=None, resize=None, codes=None, **kw):
    """-> per picture dict(planes, scale, rect, size, code) or ('status', code): a Batch with a plane description, a resize and / or an
    orientation (codes: one resolved code per picture)"""
    scans = [mjx.ParsedScan(d) for d in datas]
    orient = None if codes is None else mjx.Orient(False, [int(c) for c in codes])
    b = mjx.Batch(ctx, scans, planes=planes or mjx.Planes("uint8"), resize=resize, orient=orient, **kw)
    try:
        b.decode()
        b.wait()
        out = []
        for i in range(len(datas)):
            if b.status(i) != mjx.OK:
                out.append(("status", b.status(i)))
                continue
            inf = b.info(i)
            out.append(dict(planes=b.planes(i), scale=b.scale(i), rect=b.rect(i), size=(inf["width"], inf["height"]), code=b.orientation(i)))
        return out
    finally:
        tsl.close_all(b, scans)


def luma_resized(mjx, ctx, datas, target, filt, aa, scale, rois, codes=None):
    """the EXISTING luminance call: Output(channels=1) + Resize(auto_scale=False) (+ Orient) -> [H, W] uint8 per file"""
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, output=mjx.Output("uint8", channels=1), scale=scale, rois=rois,
                  resize=mjx.Resize(target[0], target[1], antialias=aa, auto_scale=False, filter=filt),
                  orient=None if codes is None else mjx.Orient(False, [int(c) for c in codes]))
    try:
        b.decode()
        b.wait()
        return [np.ascontiguousarray(b.output(i)[:, :, 0]) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        tsl.close_all(b, scans)


def fmt_of(mjx, dtype, il):
    return mjx.Planes(dtype, interleave=il) if dtype == "uint8" else mjx.Planes(dtype, interleave=il, mean=MEAN, std=STD)


def split(planes):
    """(Y, CbCr[h, w, 2]) -> (Y, Cb, Cr)"""
    if len(planes) == 2 and planes[1].ndim == 3:
        return (planes[0], np.ascontiguousarray(planes[1][:, :, 0]), np.ascontiguousarray(planes[1][:, :, 1]))
    return tuple(planes)


def run_child(tmp_path, call, env_set=None, timeout=600):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_planes_resize_orient as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


# ---- GPU 1: orientation, bit for bit ------------------------------------------------------------------------------------------------------------
OR_LAYOUTS = (Y420, Y422, Y440, Y444, Y411, GREY)
OR_SIZES = ((1, 1), (17, 9), (61, 45), (130, 67))                    # stored
OR_SCALES = (1, 2, 8)


def expected_fast(u8, fmt, table):
    """typ.expected_planes with the dtype's exact table computed once (tof.exact_table is exact rational arithmetic per call)"""
    if table is None:
        out = [np.ascontiguousarray(p) for p in u8]
    else:
        out = [np.ascontiguousarray(table[c][p]) for c, p in enumerate(u8)]
    if fmt.interleave and len(out) == 3:
        out = [out[0], np.ascontiguousarray(np.stack([out[1], out[2]], axis=2))]
    return tuple(out)


def child_orient():
    """Every layout x stored size x code x scale x (I420, NV12) x (uint8, float32): the whole picture and one rectangle in rotation over
    the kinds (odd origin, 1 x 1, last row, last column), so that every kind meets every code, layout and scale."""
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0, profiling=True)
    bad, n, launches, kinds = [], 0, 0, set()
    scans = {(l, W, H): mjx.ParsedScan(file_of(l, W, H)) for l in OR_LAYOUTS for W, H in OR_SIZES}
    for s in OR_SCALES:
        cases = []
        for li, lname in enumerate(OR_LAYOUTS):
            for zi, (W, H) in enumerate(OR_SIZES):
                sw, sh = cdiv(W, s), cdiv(H, s)
                for code in range(1, 9):
                    dw, dh = oriented_size(code, sw, sh)
                    rects = d_rects(dw, dh)
                    pick = [None] + ([rects[1 + (code + li + zi + s) % (len(rects) - 1)]] if len(rects) > 1 else [])
                    for rect in pick:
                        if len(rects) == 6:                 # (every kind fits the picture: the index names the kind)
                            kinds.add(rects.index(rect))
                        cases.append((lname, W, H, code, rect, rect_to_stored(code, sw, sh, rect or (0, 0, dw, dh)), (dw, dh)))
        ss = [scans[c[:3]] for c in cases]
        pb = mjx.Batch(ctx, ss, planes=mjx.Planes("uint8"), scale=s, rois=[c[5] for c in cases])        # the existing call, no orientation
        pb.decode(); pb.wait()
        plain = [tuple(np.ascontiguousarray(tor.orient_np(c[3], p)) for p in pb.planes(i)) if pb.status(i) == mjx.OK else None for i, c in enumerate(cases)]
        pb.close()
        for dtype in ("uint8", "float32"):
            for il in (False, True):
                fmt = fmt_of(mjx, dtype, il)
                table = None if dtype == "uint8" else tof.exact_table(fmt.scale, fmt.bias)
                b = mjx.Batch(ctx, ss, planes=fmt, scale=s, rois=[c[4] for c in cases], orient=mjx.Orient(False, [c[3] for c in cases]))
                b.decode(); b.wait()
                launches += b.kernel_ms()["resize"][1]
                for i, c in enumerate(cases):
                    n += 1
                    if b.status(i) != mjx.OK or plain[i] is None:
                        bad.append((s, dtype, il) + c[:5] + ("status", b.status(i))); continue
                    inf = b.info(i)
                    rw, rh = (c[4][2], c[4][3]) if c[4] else c[6]
                    if (inf["width"], inf["height"]) != (rw, rh) or b.rect(i) != c[5] or b.orientation(i) != c[3] or b.scale(i) != s:
                        bad.append((s, dtype, il) + c[:5] + ("accessors", inf, b.rect(i), b.orientation(i), b.scale(i))); continue
                    if not typ.same_planes(b.planes(i), expected_fast(plain[i], fmt, table)):
                        bad.append((s, dtype, il) + c[:5] + ("planes differ",))
                b.close()
    for sc in scans.values():
        sc.close()
    ctx.close()
    print(json.dumps({"bad": bad[:20], "nbad": len(bad), "n": n, "launches": int(launches), "kinds": sorted(kinds)}))


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
def test_every_code_is_numpys_permutation_of_the_plain_plane_decode(mjx, tmp_path, single_decode):
    res = run_child(tmp_path, "child_orient()", {} if single_decode is None else {"MJX_SINGLE_DECODE": single_decode})
    assert res["nbad"] == 0, res
    assert res["n"] > 4000 and res["launches"] >= 12 and res["kinds"] == [0, 1, 2, 3, 4, 5], res


# ---- GPU 2 and 3: the resize sweep against the twin (bit for bit) and against the float64 rule -----------------------------------------------
_SWEEP = {}
EXTRA_FORMATS = (("float32", True), ("float16", False), ("uint8", True), ("float32", False))


def sweep_run(mjx, ctx, filt):
    """one pass per filter, shared by the two tests: per group the feature's uint8 I420 planes and one more format in rotation, the twins
    through the existing luminance resize, and the plain planes at the reported (s, R)"""
    if filt in _SWEEP:
        return _SWEEP[filt]
    recs, scales = [], set()
    for g, (target, aa, auto, ks) in enumerate(sweep_groups()):
        scale = 1 if auto or target in ((1, 1), (80, 60)) else 2
        datas = [sweep_data(k) for k in ks]
        rs = mjx.Resize(target[0], target[1], antialias=aa, auto_scale=auto, filter=filt)
        got = po_decode(mjx, ctx, datas, resize=rs, scale=scale)
        xd, xil = EXTRA_FORMATS[g % 4]
        xfmt = fmt_of(mjx, xd, xil)
        extra = po_decode(mjx, ctx, datas, planes=xfmt, resize=rs, scale=scale)
        assert all(isinstance(r, dict) for r in got + extra), (target, aa, auto, got)
        # the plain planes at the reported scale and rectangle, one batch per scale
        plain = {}
        for s in sorted(set(r["scale"] for r in got)):
            idx = [i for i, r in enumerate(got) if r["scale"] == s]
            for i, p in zip(idx, typ.planes_decode(mjx, ctx, [datas[i] for i in idx], scale=s, rois=[got[i]["rect"] for i in idx])):
                plain[i] = p
        # the twins, one batch per (plane target, scale)
        jobs = {}
        for i, k in enumerate(ks):
            n, W, H = SWEEP_FILES[k]
            s = got[i]["scale"]
            spans = geometry(hv_of(n), W, H, s, got[i]["rect"])
            for c, p in enumerate(got[i]["planes"]):
                jobs.setdefault((p.shape[1], p.shape[0], s), []).append((i, c, sweep_twin(k, c), spans[c]))
        twin = {}
        for (tw, th, s), js in sorted(jobs.items()):
            for (i, c, _, _), t in zip(js, luma_resized(mjx, ctx, [j[2] for j in js], (tw, th), filt, aa, s, [j[3] for j in js])):
                twin[(i, c)] = t
        for i, k in enumerate(ks):
            if auto:
                scales.add(got[i]["scale"])
            recs.append(dict(k=k, target=target, aa=aa, auto=auto, got=got[i], extra=extra[i], xfmt=xfmt, plain=plain[i],
                             twin=[twin[(i, c)] for c in range(len(got[i]["planes"]))]))
    _SWEEP[filt] = (recs, scales)
    return _SWEEP[filt]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILTERS)
def test_resized_planes_are_the_twins_luminance_resize_bit_for_bit(mjx, gpu_ctx, filt):
    recs, scales = sweep_run(mjx, gpu_ctx, filt)
    bad = []
    for r in recs:
        n, W, H = SWEEP_FILES[r["k"]]
        want_s, want_r, _, want = plan_of(hv_of(n), W, H, 1, None, r["got"]["scale"] if not r["auto"] else 1, r["target"], r["auto"])
        what = (n, W, H, r["target"], r["aa"], r["auto"])
        if (r["got"]["scale"], r["got"]["rect"], r["got"]["size"]) != (want_s, want_r, r["target"]) or [p.shape[::-1] for p in r["got"]["planes"]] != want:
            bad.append(what + ("plan", r["got"]["scale"], r["got"]["rect"], [p.shape for p in r["got"]["planes"]], want))
            continue
        for c, (p, t) in enumerate(zip(r["got"]["planes"], r["twin"])):
            if not tsl.same(np.ascontiguousarray(p), t):
                bad.append(what + (c, "differs from the twin", int((p != t).sum()) if isinstance(t, np.ndarray) and p.shape == t.shape else t))
    assert len(recs) == 16 * 7 - 4 * 3 and scales == {1, 2, 4, 8}, (len(recs), scales)
    assert bad == [], bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILTERS)
def test_resized_planes_lie_within_the_float64_rule(mjx, gpu_ctx, filt):
    recs, _ = sweep_run(mjx, gpu_ctx, filt)
    bad, band, total = [], 0, 0
    for r in recs:
        n, W, H = SWEEP_FILES[r["k"]]
        what = (n, W, H, r["target"], r["aa"], r["auto"])
        xf = r["xfmt"]
        xplanes = split(r["extra"]["planes"])
        if not isinstance(r["plain"], tuple) or len(xplanes) != len(r["plain"]):
            bad.append(what + ("planes", r["plain"]))
            continue
        for c, src in enumerate(r["plain"]):
            g = r["got"]["planes"][c]
            t = g.shape[::-1]
            if filt == "nearest":
                pick = trf.nearest_pick(src, t[0], t[1])
                ok = tsl.same(np.ascontiguousarray(g), pick) and tof.same_bits(np.ascontiguousarray(xplanes[c]), typ.expected_planes((pick,) * (c + 1), fmt_of(mjx, ("uint8", "float16", "float32")[xf.dtype], False))[c])
                if not ok:
                    bad.append(what + (c, "not the table on the byte picked"))
                continue
            ref, tol = rule_ref(src, t, filt, r["aa"]), rule_tol(src.shape[::-1], t, filt, r["aa"])
            fail, nb, nt = check_plane(g, ref, "uint8", 1.0, 0.0, tol)
            band, total = band + nb // 3, total + nt // 3
            if fail:
                bad.append(what + (c, "uint8", fail))
            dt = ("uint8", "float16", "float32")[xf.dtype]
            fail, _, _ = check_plane(xplanes[c], ref, dt, 1.0 if dt == "uint8" else xf.scale[c], 0.0 if dt == "uint8" else xf.bias[c], tol)
            if fail:
                bad.append(what + (c, dt, "interleaved" if xf.interleave else "planes", fail))
    print("U8 elements: %d, in the band: %d" % (total, band))
    assert bad == [], bad[:8]
    assert filt == "nearest" or (total > 20000 and band <= trs.BAND_CAP * total), (band, total)


# ---- GPU 4: exactness -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILTERS)
def test_a_target_of_the_oriented_planes_own_size_is_the_unresized_output(mjx, gpu_ctx, filt):
    files = [(Y420, 61, 45), (Y422, 61, 45), (Y411, 61, 45), (GREY, 61, 45)]
    datas = [file_of(*f) for f in files]
    bad = []
    for code in (1, 2, 6):
        tw, th = oriented_size(code, 61, 45)
        for dtype in tof.DTYPES:
            for il in (False, True):
                fmt = fmt_of(mjx, dtype, il)
                for aa in (False, True):
                    got = po_decode(mjx, gpu_ctx, datas, planes=fmt, codes=[code] * len(datas),
                                    resize=mjx.Resize(tw, th, antialias=aa, auto_scale=False, filter=filt))
                    want = typ.planes_decode(mjx, gpu_ctx, datas, planes=fmt) if code == 1 else \
                        [r["planes"] if isinstance(r, dict) else r for r in po_decode(mjx, gpu_ctx, datas, planes=fmt, codes=[code] * len(datas))]
                    for f, g, w in zip(files, got, want):
                        if not isinstance(g, dict) or not typ.same_planes(g["planes"], w):
                            bad.append((f, code, dtype, il, aa))
    assert bad == [], bad[:8]


# ---- GPU 5: orientation with a resize ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("filt", ("bilinear", "bicubic"))
def test_oriented_and_resized_planes_are_the_twin_through_the_existing_oriented_luminance_resize(mjx, gpu_ctx, filt):
    files = [(Y420, 61, 45), (Y422, 61, 45), (Y411, 61, 45), (Y420, 333, 217)]
    datas = [file_of(*f) for f in files]
    bad, n = [], 0
    for code in (2, 3, 6, 7):
        for target in ((24, 16), (9, 7)):
            for auto in (False, True):
                rs = mjx.Resize(target[0], target[1], antialias=True, auto_scale=auto, filter=filt)
                got = po_decode(mjx, gpu_ctx, datas, resize=rs, codes=[code] * len(files), scale=1 if auto else 2)
                jobs, plain = {}, {}
                for i, (lname, W, H) in enumerate(files):
                    what = (lname, W, H, code, target, auto)
                    if not isinstance(got[i], dict):
                        bad.append(what + got[i]); continue
                    want_s, want_r, spans, want = plan_of(hv_of(lname), W, H, code, None, 2, target, auto)
                    if (got[i]["scale"], got[i]["rect"], got[i]["size"], got[i]["code"]) != (want_s, want_r, target, code) or [p.shape[::-1] for p in got[i]["planes"]] != want:
                        bad.append(what + ("plan", got[i]["scale"], got[i]["rect"], want)); continue
                    plain[i] = typ.planes_decode(mjx, gpu_ctx, [datas[i]], scale=want_s, rois=want_r)[0]
                    for c, p in enumerate(got[i]["planes"]):
                        t = twin_of(lname, W, H, c)
                        fw, fh = trs.roi.frame_of(t)[:2]
                        d_rect = rect_to_oriented(code, cdiv(fw, want_s), cdiv(fh, want_s), spans[c])
                        jobs.setdefault((p.shape[1], p.shape[0], want_s), []).append((i, c, t, d_rect))
                for (tw, th, s), js in sorted(jobs.items()):
                    twins = luma_resized(mjx, gpu_ctx, [j[2] for j in js], (tw, th), filt, True, s, [j[3] for j in js], codes=[code] * len(js))
                    for (i, c, _, _), t in zip(js, twins):
                        n += 1
                        g = np.ascontiguousarray(got[i]["planes"][c])
                        if not tsl.same(g, t):
                            bad.append(files[i] + (code, target, auto, c, "differs from the twin")); continue
                        src = np.ascontiguousarray(tor.orient_np(code, plain[i][c]))
                        fail, _, _ = check_plane(g, rule_ref(src, (tw, th), filt, True), "uint8", 1.0, 0.0, rule_tol(src.shape[::-1], (tw, th), filt, True))
                        if fail:
                            bad.append(files[i] + (code, target, auto, c, fail))
    assert n == 4 * 2 * 2 * 12 and bad == [], (n, bad[:8])


# ---- GPU 6: fit modes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cover_is_the_stretch_call_on_the_rewritten_rectangle_and_contain_is_refused(mjx, gpu_ctx):
    files = [(Y420, 61, 45), (Y422, 61, 45), (GREY, 61, 45), (Y420, 333, 217)]
    datas = [file_of(*f) for f in files]
    for code, target, auto, roi in ((1, (16, 16), True, None), (6, (24, 9), True, (3, 5, 30, 40)), (2, (9, 20), False, None)):
        cover = mjx.Resize(target[0], target[1], auto_scale=auto, fit="cover")
        asked = []
        for d in datas:
            scan = mjx.ParsedScan(d)
            asked.append(scan.fit_plan(cover, code=code, roi=roi)["asked"])
            scan.close()
        fmt = mjx.Planes("uint8", interleave=True)
        a = po_decode(mjx, gpu_ctx, datas, planes=fmt, resize=cover, codes=[code] * 4, rois=roi)
        b = po_decode(mjx, gpu_ctx, datas, planes=fmt, resize=mjx.Resize(target[0], target[1], auto_scale=auto), codes=[code] * 4, rois=asked)
        for f, x, y, r in zip(files, a, b, asked):
            assert isinstance(x, dict) and isinstance(y, dict) and typ.same_planes(x["planes"], y["planes"]) and (x["scale"], x["rect"]) == (y["scale"], y["rect"]), (f, code, r)
        assert any(r[2:] != (oriented_size(code, f[1], f[2]) if roi is None else roi[2:]) for f, r in zip(files, asked))
    # contain: every picture of the call is refused, the call itself and the context are fine
    st = po_decode(mjx, gpu_ctx, datas, resize=mjx.Resize(24, 16, fit="contain"), codes=[1, 6, 1, 2])
    assert st == [("status", mjx.ERR_INVALID_ARG)] * 4, st
    ok = po_decode(mjx, gpu_ctx, datas, resize=mjx.Resize(24, 16), codes=[1, 6, 1, 2])
    assert all(isinstance(r, dict) for r in ok)


# ---- GPU 7: caller-owned planes ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("code", (2, 6))
@pytest.mark.parametrize("il", [False, True], ids=["i420", "nv12"])
def test_caller_owned_planes_padded_rows_and_guards(mjx, gpu_ctx, il, code):
    cases = [(Y420, 61, 45), (Y422, 61, 45), (Y420, 61, 45), (GREY, 61, 45), (Y420, 333, 217), (Y420, 61, 45)]
    datas = [file_of(*c) for c in cases]
    damaged, wrong = 2, 5
    datas[damaged] = datas[damaged][:len(datas[damaged]) // 2]
    target, dtype = (24, 16), "float16"
    esz = ESZ[dtype]
    rs = mjx.Resize(target[0], target[1], filter="bicubic")
    hip = tof._hip(mjx)
    dst, spans, sizes_of, at = [], [], [], 4096
    for i, (n, W, H) in enumerate(cases):
        want = plan_of(hv_of(n), W, H, code, None, 1, target, True)[3]
        pair = il and len(want) == 3
        planes, sizes = [], [(w + (1 if i == wrong and c == 0 else 0), h) for c, (w, h) in enumerate(want)]
        for c, (w, h) in enumerate(want[:2] if pair else want):
            row = 2 * w if pair and c == 1 else w
            pitch = row + 3 + c
            planes.append((at, pitch, row, h))
            at += ((h - 1) * pitch + row) * esz + 64
            at = (at + 3) & ~3
        spans.append(planes)
        sizes_of.append(want)
        dst.append(([(p, pitch) for p, pitch, _, _ in planes] + [(0, 0)] * (3 - len(planes)), sizes + [(0, 0)] * (3 - len(sizes))))
    total = at + 4096
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [([(base.value + p if p else 0, pitch) for p, pitch in pl], sz) for pl, sz in dst]
        fmt = fmt_of(mjx, dtype, il)
        good = [i for i in range(len(cases)) if i not in (damaged, wrong)]
        lib_owned = po_decode(mjx, gpu_ctx, [datas[i] for i in good], planes=fmt, resize=rs, codes=[code] * len(good))
        fmt_dst = mjx.Planes(dtype, interleave=il, scale=fmt.scale, bias=fmt.bias, dst=dst)
        b, st = mjx.decode_batch(gpu_ctx, datas, planes=fmt_dst, resize=rs, orient=mjx.Orient(False, code), chunk_images=2)
        try:
            assert st[wrong] == mjx.ERR_INVALID_ARG and st[damaged] not in (mjx.OK, mjx.ERR_INVALID_ARG) and [st[i] for i in good] == [mjx.OK] * len(good), st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            covered = np.zeros(total, bool)
            for i, ref in zip(good, lib_owned):
                want = ref["planes"]
                inf = b.plane_info(i)
                assert inf["nplanes"] == len(want) and inf["dtype"] == fmt.dtype and inf["interleave"] == (il and len(sizes_of[i]) == 3), inf
                for c, ((p, pitch, row, h), w) in enumerate(zip(spans[i], want)):
                    assert (inf["dev"][c], inf["row_pitch"][c]) == (base.value + p, pitch), (i, c, inf)
                    el = np.arange(h)[:, None] * pitch + np.arange(row)[None, :]
                    slot = mem[p: p + ((h - 1) * pitch + row) * esz].view(fmt.numpy_dtype())
                    assert tof.same_bits(np.ascontiguousarray(slot[el]).reshape(w.shape), np.ascontiguousarray(w)), ("picture", i, "plane", c)
                    covered[(p + el.reshape(-1)[:, None] * esz + np.arange(esz)[None, :]).reshape(-1)] = True
                with pytest.raises(mjx.MjxError):
                    b.planes(i)
            assert np.all(mem[~covered] == SENTINEL), ("bytes outside the planes' elements were written", np.argwhere((mem != SENTINEL) & ~covered)[:8].ravel().tolist())
            assert b.bytes()["rgb"] == sum(sum(w * h for w, h in sizes_of[i]) for i in good + [damaged]) * esz
            with pytest.raises(mjx.MjxError):
                b.tile(2)
        finally:
            b.close()
    finally:
        assert hip.hipFree(base) == 0


# ---- GPU 8: the front doors ---------------------------------------------------------------------------------------------------------------------
def child_torch():
    import torch                                     # first: the package then shares torch's HIP runtime
    import __graft_entry__ as ge
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad = []
    sizes = [(61, 45), (333, 217), (130, 67), (45, 61)]
    datas = [file_of(Y420, w, h) for w, h in sizes]
    datas[3] = tor.tagged(datas[3], 6)                                    # a portrait file that says so: it leaves 61 x 45 wide
    other = file_of(Y422, 61, 45)                                         # another sampling layout: refused, its slot untouched
    all_datas = datas + [other]
    n = len(all_datas)
    W, H = 48, 32
    rs = mjx.Resize(W, H, filter="bicubic")
    ref, st = mjx.decode_batch(ctx, datas, planes=mjx.Planes("uint8", interleave=True), resize=rs, orient=mjx.Orient(True))
    want = [ref.planes(i) for i in range(len(datas))]
    codes = [ref.orientation(i) for i in range(len(datas))]
    ref.close()
    if codes != [1, 1, 1, 6] or st != [mjx.OK] * 4:
        bad.append(("codes", codes, st))
    dev = torch.device("cuda", 0)
    y = torch.full((n, H, W + 5), 7, dtype=torch.uint8, device=dev)
    cbcr = torch.full((n, H // 2, W // 2 + 3, 2), 7, dtype=torch.uint8, device=dev)
    st = mjx.decode_planes_into(ctx, all_datas, y[:, :, :W], cbcr=cbcr[:, :, :W // 2], resize=rs, orient=mjx.Orient(True))
    if st != [mjx.OK] * 4 + [mjx.ERR_INVALID_ARG]:
        bad.append(("status", st))
    yh, ch = y.cpu().numpy(), cbcr.cpu().numpy()
    for i in range(4):
        if not np.array_equal(yh[i, :, :W], want[i][0]) or not np.array_equal(ch[i, :, :W // 2], want[i][1]):
            bad.append(("picture", i))
    if not (yh[:, :, W:] == 7).all() or not (ch[:, :, W // 2:] == 7).all() or not (yh[4] == 7).all() or not (ch[4] == 7).all():
        bad.append("written outside the planes, or into the refused picture's slot")
    ctx.close()
    print(json.dumps({"bad": bad}))


@pytest.mark.gpu
def test_decode_planes_into_one_pair_of_tensors_from_files_of_four_sizes(mjx, tmp_path):
    res = run_child(tmp_path, "child_torch()")
    assert res["bad"] == [], res


@pytest.mark.gpu
def test_front_door_from_file_bytes_in_groups_tiles_destuffings_and_progressive(mjx, gpu_ctx):
    import prog_cases as pc
    files = [(Y420, 333, 217), (Y422, 61, 45), (Y411, 130, 67), (GREY, 61, 45), (Y420, 61, 45), (Y440, 130, 67), (Y420, 333, 217)]
    datas = [file_of(*f) for f in files]
    extra = [1, 6, 3, 8, 2, 5, 7]
    datas[0] = tor.tagged(datas[0], 6)                                    # tag 6 then extra 1
    datas[4] = tor.tagged(datas[4], 3, ">")                               # tag 3 then extra 2: code 4
    codes = [6, 6, 3, 8, 4, 5, 7]
    rs = mjx.Resize(40, 24, filter="bilinear")
    fmt = mjx.Planes("uint8", interleave=True)
    plain = [file_of(*f) for f in files]
    want = po_decode(mjx, gpu_ctx, plain, planes=fmt, resize=rs, codes=codes)
    assert all(isinstance(w, dict) for w in want)
    old = os.environ.get("MJX_GROUP_MB")
    os.environ["MJX_GROUP_MB"] = "1"
    try:
        for dd in (False, True):
            b, st = mjx.decode_batch(gpu_ctx, datas * 3, planes=fmt, resize=rs, orient=mjx.Orient(True, extra * 3), chunk_images=2, device_destuff=dd)
            try:
                assert st == [mjx.OK] * 21, st
                for i in range(21):
                    w = want[i % 7]
                    assert typ.same_planes(b.planes(i), w["planes"]) and (b.orientation(i), b.scale(i), b.rect(i)) == (w["code"], w["scale"], w["rect"]), (dd, i)
            finally:
                b.close()
    finally:
        if old is None:
            del os.environ["MJX_GROUP_MB"]
        else:
            os.environ["MJX_GROUP_MB"] = old
    # tile(3): everything is carried along
    scans = [mjx.ParsedScan(d) for d in plain]
    base = mjx.Batch(gpu_ctx, scans, planes=fmt, resize=rs, orient=mjx.Orient(False, codes), chunk_images=3)
    tiled = base.tile(3)
    try:
        tiled.decode(); tiled.wait()
        for i in range(21):
            w = want[i % 7]
            assert tiled.status(i) == mjx.OK and typ.same_planes(tiled.planes(i), w["planes"]), i
            assert (tiled.orientation(i), tiled.scale(i), tiled.rect(i)) == (w["code"], w["scale"], w["rect"]), i
            inf = tiled.info(i)
            assert (inf["width"], inf["height"]) == (40, 24)
        assert tiled.bytes()["rgb"] == 3 * sum(sum(p.size for p in w["planes"]) for w in want)
    finally:
        tiled.close()
        tsl.close_all(base, scans)
    # a progressive file is its baseline twin through the same call
    pair = list(pc.layout_pair("420_70x52"))
    b, st = mjx.decode_batch(gpu_ctx, pair, planes=fmt, resize=mjx.Resize(24, 16, filter="bicubic"), orient=mjx.Orient(False, 6), progressive=True)
    try:
        assert st == [mjx.OK, mjx.OK] and typ.same_planes(b.planes(0), b.planes(1))
    finally:
        b.close()


# ---- GPU 9: untouched defaults ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_both_descriptions_null_is_the_planes_call_and_the_packed_decode_is_what_it_was(mjx, gpu_ctx):
    files = [(Y420, 333, 217), (Y422, 61, 45), (Y411, 61, 45), (GREY, 61, 45)]
    datas = [file_of(*f) for f in files]
    rois = [(3, 5, 99, 77), None, (1, 1, 1, 1), None]
    lib = mjx.lib()
    for dtype, il in (("uint8", False), ("float32", True)):
        fmt = fmt_of(mjx, dtype, il)
        want = typ.planes_decode(mjx, gpu_ctx, datas, planes=fmt, rois=rois)
        scans = [mjx.ParsedScan(d) for d in datas]
        arr = (mjx.ScanDesc * 4)()
        for i, s in enumerate(scans):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(s.desc), ctypes.sizeof(mjx.ScanDesc))
        o = mjx._opts(rois=rois)
        keep, ref = mjx._planes_ref(fmt)
        h, st = ctypes.c_void_p(), (ctypes.c_int * 4)()
        assert lib.mjx_batch_create_planes_orient(gpu_ctx.h, arr, 4, ctypes.byref(o), ref, None, None, ctypes.byref(h), st) == mjx.OK
        b = mjx.Batch(gpu_ctx, _handle=h)
        try:
            b.decode(); b.wait()
            assert b.kernel_ms()["resize"][1] == 0
            for i in range(4):
                assert b.status(i) == mjx.OK and typ.same_planes(b.planes(i), want[i]) and b.orientation(i) == 1, (dtype, il, i)
        finally:
            tsl.close_all(b, scans)
        # code 1 without a resize through the orientation description: planned as the planes call, no further launch
        got = po_decode(mjx, gpu_ctx, datas, planes=fmt, codes=[1] * 4, rois=rois)
        assert all(typ.same_planes(g["planes"], w) for g, w in zip(got, want))
    # the plain packed decode: the oracle's picture within its usual bound, and the same bytes before and after a feature batch on the context
    import test_luma_output as tlo
    before = tlo.packed_decode(mjx, gpu_ctx, datas[:2] + datas[3:])
    po_decode(mjx, gpu_ctx, datas, resize=mjx.Resize(24, 16), codes=[6] * 4)
    after = tlo.packed_decode(mjx, gpu_ctx, datas[:2] + datas[3:])
    assert all(tsl.same(x, y) for x, y in zip(before, after))
    for d, p in zip(datas[:2] + datas[3:], before):
        assert tsl.rgb_problem(p, tsl.oracle_std(d).rgb) is None

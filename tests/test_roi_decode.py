"""Region-of-interest decode (mjx_opts.rois, include/mjx.h): a rectangle per picture, at every scale.

The contract: a rectangle is given in the coordinates of the picture the call would otherwise produce (STANDARD layout at the
call's scale); the result is exactly w x h x 3 bytes and equals, byte for byte, the crop of what the same build writes without a
rectangle.  Stage B fetches and transforms only the tiles that touch the rectangle; mjx_plan_tiles says which, from the planner
and the kernels' own tile rule, so the saving is checked here without a GPU against a brute-force enumeration.

GPU checks run in a child process per group of inputs (this module is the child's library: `python -c "import test_roi_decode"`).
The independent yardstick is the project's gate (TOL = 1 per byte, under 1 % of bytes) against the crop of the
reference picture -- the oracle's STANDARD picture at scale 1, tests/scaled_ref.py above it --, the share pooled over all the
rectangles of a picture (one flipped byte is a third of a 1 x 1 crop).
"""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import scaled_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1
SCALES = (1, 2, 4, 8)
SYNTH_SIZES = [(1, 1), (7, 5), (17, 33), (61, 45), (750, 595), (1001, 37)]          # test_scaled_decode.py's
HV = [(1, 1), (2, 1), (1, 2), (2, 2)]
LAYOUTS = [[a, b, c] for a in HV for b in HV for c in HV]
GRAYS = [(1, 2), (2, 1), (2, 2)]
LAYOUT_SIZES = [(37, 29), (333, 217)]
SCRIPT_LAYOUTS = [[(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(2, 2), (2, 2), (1, 1)], [(2, 1), (1, 2), (1, 2)]]
SCRIPT_SIZES = [(333, 217), (1000, 40)]          # ((1000, 40): a tile touches at most two MCU rows, so stage B reads the scans directly)


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def fixture_paths():
    out = sorted(glob.glob(os.path.join(ROOT, "tests", "data", "*.jp*g")))
    out += [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pil", "*.jpg"))) if "progressive" not in p]
    return out


def lname(hv):
    return "Y%d%d_Cb%d%d_Cr%d%d" % tuple(f for c in hv for f in c)


def layout_data(hv, w, h, restart=None, gray=None):
    seed = (LAYOUTS.index(hv) if gray is None else 100 + GRAYS.index(gray)) * 1000 + w * 7 + h
    return jw.layout_jpeg(w, h, hv, quality=75, seed=seed, restart=restart, gray_hv=gray)[0]


def frame_of(data):
    """-> (width, height, hmax, vmax, bpm) of the STANDARD layout (a one-component frame: one block per MCU)"""
    w, h, comps, _ = scaled_ref.jpeg_tables(data)
    if len(comps) == 1:
        return w, h, 1, 1, 1
    return w, h, max(c[0] for c in comps), max(c[1] for c in comps), sum(c[0] * c[1] for c in comps)


# ---- the rectangle generator ----------------------------------------------------------------------------------------------------
def rectangles(ow, oh, mw, mh, seed):
    """Rectangles inside an ow x oh picture whose MCUs are mw x mh patches of it: the whole picture, the four 1 x 1 corners, a
    one-pixel column and row through the middle, one that starts and ends in the middle of an MCU, one that starts on an MCU
    boundary, one whose w * 3 is not a multiple of 4, three random ones.  Seeded; duplicates (tiny pictures) are dropped."""
    rng = np.random.RandomState(seed)
    out = [(0, 0, 0, 0), (0, 0, 1, 1), (ow - 1, 0, 1, 1), (0, oh - 1, 1, 1), (ow - 1, oh - 1, 1, 1), (ow // 2, 0, 1, oh), (0, oh // 2, ow, 1)]

    def mid(n, m):          # [a, b) with a and b in the middle of an MCU where the picture is large enough
        a = min(n - 1, (n // (3 * m)) * m + m // 2)
        b = min(n, a + m + 1 + (n // 2 // m) * m)
        if b % m == 0 and b > a + 1:
            b -= 1
        return a, b
    x0, x1 = mid(ow, mw)
    y0, y1 = mid(oh, mh)
    out.append((x0, y0, x1 - x0, y1 - y0))
    bx, by = (ow // 2 // mw) * mw, (oh // 2 // mh) * mh
    out.append((bx, by, min(ow - bx, mw + 3), min(oh - by, mh + 2)))
    ww = ow if ow % 4 else ow - 1
    if ww >= 1:
        out.append(((ow - ww) // 2, oh // 3, ww, max(1, min(oh - oh // 3, 3))))
    for _ in range(3):
        x, y = int(rng.randint(0, ow)), int(rng.randint(0, oh))
        out.append((x, y, int(rng.randint(1, ow - x + 1)), int(rng.randint(1, oh - y + 1))))
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


def crop(full, r):
    x, y, w, h = r
    return full if w == 0 and h == 0 else full[y:y + h, x:x + w]


# ---- CPU: argument rules --------------------------------------------------------------------------------------------------------
def test_argument_rules_through_validate(mjx):
    data = mjx.synth_jpeg(1001, 37, "420", 75, seed=3)
    scan = mjx.ParsedScan(data)
    try:
        assert scan.validate(roi=(10, 5, 100, 20)) == mjx.OK
        assert scan.validate(roi=(0, 0, 1001, 37)) == mjx.OK
        for r in [(1, 0, 1001, 37), (0, 1, 1001, 37), (0, 0, 1002, 37), (0, 0, 1001, 38), (1001, 0, 1, 1), (0, 37, 1, 1),
                  (2 ** 32 - 1, 0, 2, 1), (0, 2 ** 32 - 1, 1, 2)]:
            assert scan.validate(roi=r) == mjx.ERR_INVALID_ARG, r
        assert scan.validate(roi=(0, 0, 0, 5)) == mjx.ERR_INVALID_ARG           # exactly one of w and h zero
        assert scan.validate(roi=(0, 0, 5, 0)) == mjx.ERR_INVALID_ARG
        assert scan.validate(roi=(0, 0, 0, 0)) == mjx.OK                        # the whole picture
        assert scan.validate(roi=(7, 9, 0, 0)) == mjx.OK
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT, roi=(0, 0, 8, 8)) == mjx.ERR_INVALID_ARG
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT, roi=(0, 0, 0, 0)) == scan.validate(layout=mjx.LAYOUT_REF_COMPAT)
        for s in (2, 4, 8):                                                     # the bounds are those of ceil(W / s) x ceil(H / s)
            ow, oh = -(-1001 // s), -(-37 // s)
            assert scan.validate(scale=s, roi=(0, 0, ow, oh)) == mjx.OK, s
            assert scan.validate(scale=s, roi=(ow - 1, oh - 1, 1, 1)) == mjx.OK, s
            assert scan.validate(scale=s, roi=(0, 0, ow + 1, oh)) == mjx.ERR_INVALID_ARG, s
            assert scan.validate(scale=s, roi=(0, 0, ow, oh + 1)) == mjx.ERR_INVALID_ARG, s
            assert scan.validate(scale=s, roi=(ow, 0, 1, 1)) == mjx.ERR_INVALID_ARG, s
        assert (-(-1001 // 8), -(-37 // 8)) == (126, 5)
        assert scan.validate(scale=8, roi=(125, 4, 1, 1)) == mjx.OK
        assert scan.validate(scale=8, roi=(126, 4, 1, 1)) == mjx.ERR_INVALID_ARG
        assert scan.validate(scale=3, roi=(0, 0, 1, 1)) == mjx.ERR_INVALID_ARG
        # n_rois: 0 or 1 for the one-picture entry points; a null array with a count is refused
        two = mjx._opts(rois=[(0, 0, 1, 1), (0, 0, 1, 1)])
        assert mjx.lib().mjx_validate(ctypes.byref(scan.desc), ctypes.byref(two)) == mjx.ERR_INVALID_ARG
        null = mjx._opts()
        null.n_rois = 1
        assert mjx.lib().mjx_validate(ctypes.byref(scan.desc), ctypes.byref(null)) == mjx.ERR_INVALID_ARG
    finally:
        scan.close()
    scan = mjx.ParsedScan(_read(os.path.join(ROOT, "tests", "golden", "pil", "ms_420_odd.jpg")))      # a multi-scan file
    try:
        w, h = scan.desc.width, scan.desc.height
        assert scan.validate(roi=(1, 1, w - 1, h - 1)) == mjx.OK
        assert scan.validate(roi=(1, 1, w, h - 1)) == mjx.ERR_INVALID_ARG
        assert scan.validate(scale=4, roi=(0, 0, -(-w // 4), -(-h // 4))) == mjx.OK
        assert scan.validate(scale=4, roi=(0, 0, -(-w // 4) + 1, 1)) == mjx.ERR_INVALID_ARG
    finally:
        scan.close()


# ---- CPU: mjx_plan_tiles against a brute-force enumeration ----------------------------------------------------------------------
def enumerate_tiles(w, h, hmax, vmax, scale, T, r):
    """-> (the set of tiles holding an MCU of the rectangle's MCU rows and columns, the tiles of its row band, all tiles)"""
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    ntiles = -(-(mcux * mcuy) // T)
    x, y, rw, rh = r
    if rw == 0 and rh == 0:
        return set(range(ntiles)), ntiles, ntiles
    pw, ph = 8 // scale * hmax, 8 // scale * vmax
    rows = np.arange(y // ph, (y + rh - 1) // ph + 1)
    cols = np.arange(x // pw, (x + rw - 1) // pw + 1)
    mcus = (rows[:, None] * mcux + cols[None, :]).ravel()
    band = (rows[-1] * mcux + mcux - 1) // T - (rows[0] * mcux) // T + 1
    return set((mcus // T).tolist()), int(band), ntiles


def _plan_cases(mjx):
    for gray, hvs in ((None, LAYOUTS), (True, GRAYS)):
        for hv in hvs:
            for (w, h) in [(37, 29), (333, 217), (1000, 40), (641, 481)]:
                data = layout_data(None, w, h, gray=hv) if gray else layout_data(hv, w, h)
                yield ("gray%d%d" % hv if gray else lname(hv)) + "_%dx%d" % (w, h), data


def test_plan_tiles_matches_the_enumeration(mjx):
    bad, n = [], 0
    for cname, data in _plan_cases(mjx):
        w, h, hmax, vmax, _ = frame_of(data)
        scan = mjx.ParsedScan(data)
        try:
            for s in SCALES:
                ow, oh = -(-w // s), -(-h // s)
                for r in rectangles(ow, oh, 8 // s * hmax, 8 // s * vmax, seed=n):
                    got = scan.plan_tiles(roi=r, scale=s)
                    want, _, total = enumerate_tiles(w, h, hmax, vmax, s, got["tile_mcus"], r)
                    n += 1
                    if got["tiles_read"] != len(want) or got["tiles_total"] != total:
                        bad.append((cname, s, r, got, len(want), total))
        finally:
            scan.close()
    assert bad == [], bad[:10]
    assert n > 8000, n


def test_plan_tiles_of_multi_scan_pictures_lies_between_the_set_and_the_band(mjx, orc):
    bad, n, exact, wider = [], 0, 0, 0
    for hv in SCRIPT_LAYOUTS:
        for (w, h) in SCRIPT_SIZES:
            src = layout_data(hv, w, h)
            ref = orc.decode(src, layout=orc.LAYOUT_STD)
            for twin in jw.script_twins(src, ref, jw.SCRIPTS[::5]):
                scan = mjx.ParsedScan(twin)
                try:
                    _, _, hmax, vmax, _ = frame_of(src)
                    for s in SCALES:
                        ow, oh = -(-w // s), -(-h // s)
                        for r in rectangles(ow, oh, 8 // s * hmax, 8 // s * vmax, seed=n):
                            got = scan.plan_tiles(roi=r, scale=s)
                            want, band, total = enumerate_tiles(w, h, hmax, vmax, s, got["tile_mcus"], r)
                            n += 1
                            exact += got["tiles_read"] == len(want)
                            wider += got["tiles_read"] > len(want)
                            if not (len(want) <= got["tiles_read"] <= band) or got["tiles_total"] != total:
                                bad.append((lname(hv), w, h, s, r, got, len(want), band))
                finally:
                    scan.close()
    assert bad == [], bad[:10]
    assert n > 500 and exact > 0, (n, exact, wider)


def test_plan_tiles_fixed_points_of_a_4k_picture(mjx):
    scan = mjx.ParsedScan(mjx.synth_jpeg(3840, 2160, "420", 75, seed=1))
    try:
        whole = scan.plan_tiles()
        T = whole["tile_mcus"]
        for r, n32 in (((960, 540, 1920, 1080), 345), ((1808, 968, 224, 224), 15), ((0, 0, 0, 0), 1013)):
            got = scan.plan_tiles(roi=r)
            want, _, total = enumerate_tiles(3840, 2160, 2, 2, 1, T, r)
            assert got["tile_mcus"] == T and got["tiles_total"] == total and got["tiles_read"] == len(want), (r, got, len(want))
            if T == 32:                             # (the counts of the tile rule with the 4:2:0 kernel's 32 MCUs per tile)
                assert got["tiles_read"] == n32 and total == 1013, (r, got)
        assert whole["tiles_read"] == whole["tiles_total"]
    finally:
        scan.close()


# ---- CPU: the other surfaces -------------------------------------------------------------------------------------------------------
def test_rust_binding_mirrors_the_rectangle_and_the_new_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "mjx.h")).decode(), flags=re.S)
    rs = _read(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).decode()
    body = re.search(r"typedef struct mjx_rect\s*\{(.*?)\}\s*mjx_rect;", hdr, flags=re.S).group(1)
    assert [f.strip() for f in body.replace("uint32_t", "").strip(" ;\n").split(",")] == ["x", "y", "w", "h"]
    rbody = re.search(r"pub struct mjx_rect\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+): u32", rbody) == ["x", "y", "w", "h"]
    assert re.search(r"#\[repr\(C\)\]\s*(#\[[^\]]*\]\s*)*pub struct mjx_rect", rs)
    obody = re.search(r"pub struct mjx_opts\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    fields = re.findall(r"pub ([a-z_0-9]+): ([^,\n]+),", obody)
    assert fields[-2:] == [("rois", "*const mjx_rect"), ("n_rois", "u32")] and fields[-3][0] == "scale_denom", fields
    cbody = re.search(r"typedef struct mjx_opts\s*\{(.*?)\}\s*mjx_opts;", hdr, flags=re.S).group(1)
    assert re.search(r"scale_denom\s*;\s*const\s+mjx_rect\s*\*\s*rois\s*;\s*uint32_t\s+n_rois\s*;\s*$", cbody.strip() + "\n".strip())
    for fn, n in (("mjx_plan_tiles", 5), ("mjx_batch_image_roi", 6)):
        c = re.search(r"\b" + fn + r"\(([^;{]*?)\);", hdr).group(1)
        r = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        assert c.count(",") + 1 == n and r.count(",") + 1 == n, (fn, c, r)


def test_python_structures_mirror_the_header(mjx):
    assert [f[0] for f in mjx.Rect._fields_] == ["x", "y", "w", "h"] and ctypes.sizeof(mjx.Rect) == 16
    assert [f[0] for f in mjx.Opts._fields_][-3:] == ["scale_denom", "rois", "n_rois"]
    assert "mjx_plan_tiles" in mjx.SYMBOLS and "mjx_batch_image_roi" in mjx.SYMBOLS
    o = mjx._opts(rois=[(1, 2, 3, 4), None])
    assert o.n_rois == 2 and (o.rois[0].x, o.rois[0].y, o.rois[0].w, o.rois[0].h) == (1, 2, 3, 4) and o.rois[1].w == 0
    assert mjx._opts(rois=(1, 2, 3, 4)).n_rois == 1 and not mjx._opts().rois


def test_roi_decode_without_a_device_is_a_device_error(tmp_path):
    """No fallback: mjx_decode with a rectangle and no visible device says MJX_ERR_DEVICE (a child process with the devices hidden)."""
    script = tmp_path / "nodev.py"
    script.write_text(
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "data = open(os.path.join(%r, 'tests', 'data', 'lena.jpeg'), 'rb').read()\n"
        "try:\n"
        "    mjx.decode(data, roi=(10, 20, 30, 40))\n"
        "    print('decoded')\n"
        "except mjx.MjxError as e:\n"
        "    print('rc', e.code)\n" % (ROOT, ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    assert out.stdout.split() == ["rc", str(ge.load_package().ERR_DEVICE)], out.stdout


# ---- GPU: the child's library ----------------------------------------------------------------------------------------------------
def group_inputs(mjx, orc, group):
    """[(name, bytes)] of one group of inputs"""
    if group == "fixtures":
        return [(os.path.basename(p), _read(p)) for p in fixture_paths()]
    if group == "synthetic":
        return [("%s_%dx%d" % (sub, w, h), mjx.synth_jpeg(w, h, sub, 75, seed=31 + k))
                for sub in ("420", "422", "440", "444", "gray") for k, (w, h) in enumerate(SYNTH_SIZES)]
    if group == "layouts":
        out = [("%s_%dx%d" % (lname(hv), w, h), layout_data(hv, w, h)) for hv in LAYOUTS for (w, h) in LAYOUT_SIZES]
        return out + [("gray%d%d_%dx%d" % (g + (w, h)), layout_data(None, w, h, gray=g)) for g in GRAYS for (w, h) in LAYOUT_SIZES]
    if group == "scripts":
        out = []
        for hv in SCRIPT_LAYOUTS:
            for (w, h) in SCRIPT_SIZES:
                src = layout_data(hv, w, h)
                ref = orc.decode(src, layout=orc.LAYOUT_STD)
                out += [("%s_%dx%d_%s" % (lname(hv), w, h, sc), t) for sc, t in zip(jw.SCRIPTS, jw.script_twins(src, ref, jw.SCRIPTS))]
        return out
    if group == "restart_and_large":
        out = [("%s_%dx%d_rst%d" % (lname(hv), w, h, rst), layout_data(hv, w, h, restart=rst))
               for hv, rst in ((LAYOUTS[48], 5), (LAYOUTS[0], 3), (LAYOUTS[16], 40)) for (w, h) in LAYOUT_SIZES + [(1000, 40)]]
        return out + [("1080p_420", mjx.synth_jpeg(1920, 1080, "420", 75, seed=5)), ("4k_420", mjx.synth_jpeg(3840, 2160, "420", 75, seed=6)),
                      ("4k_420_q92", mjx.synth_jpeg(3840, 2160, "420", 92, seed=7))]
    raise ValueError(group)


GROUPS = ["fixtures", "synthetic", "layouts", "scripts", "restart_and_large"]


def child_equality(group):
    """Every rectangle of every input of the group, at every scale: equal to the crop of the device's uncropped picture (one Batch
    with a rectangle per copy of the picture, and mjx_decode_batch with the host's and the device's de-stuffing), and within the
    gate of the reference's crop.  Prints the failures and the largest figures as JSON."""
    import __graft_entry__ as ge
    import oracle_binding as orc
    mjx = ge.load_package()
    ctx = mjx.Context(0)
    bad, worst, nrect = [], {"max_diff": 0, "share": 0.0}, 0
    for k, (name, data) in enumerate(group_inputs(mjx, orc, group)):
        dec = orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)
        w, h, hmax, vmax, _ = frame_of(data)
        for s in SCALES:
            ref = dec.rgb if s == 1 else scaled_ref.scaled_rgb(data, s, dec)
            scan = mjx.ParsedScan(data)
            b = mjx.Batch(ctx, [scan], scale=s)
            b.decode(); b.wait()
            if b.status(0) != mjx.OK:
                bad.append((name, s, "uncropped status", b.status(0))); b.close(); scan.close(); continue
            full = b.rgb(0)
            b.close()
            if full.shape != ref.shape:
                bad.append((name, s, "shape", full.shape, ref.shape)); scan.close(); continue
            rects = rectangles(full.shape[1], full.shape[0], 8 // s * hmax, 8 // s * vmax, seed=1000 * k + s)
            nrect += len(rects)
            ndiff = nbytes = 0
            b = mjx.Batch(ctx, [scan] * len(rects), scale=s, rois=rects)
            b.decode(); b.wait()
            for i, r in enumerate(rects):
                if b.status(i) != mjx.OK:
                    bad.append((name, s, r, "status", b.status(i))); continue
                got, want = b.rgb(i), crop(full, r)
                if got.shape != want.shape or not np.array_equal(got, want):
                    bad.append((name, s, r, "differs from the crop of the uncropped decode", got.shape, want.shape))
                    continue
                d = np.abs(got.astype(np.int32) - crop(ref, r).astype(np.int32))
                worst["max_diff"] = max(worst["max_diff"], int(d.max()))
                if d.max() > TOL:
                    bad.append((name, s, r, "reference", int(d.max())))
                ndiff += int((d > 0).sum()); nbytes += d.size
            b.close()
            scan.close()
            worst["share"] = max(worst["share"], ndiff / max(nbytes, 1))
            if ndiff >= 0.01 * nbytes:
                bad.append((name, s, "share of differing bytes over the picture's rectangles", ndiff, nbytes))
            for dd in (True, False):
                fb, st = mjx.decode_batch(ctx, [data] * len(rects), device_destuff=dd, scale=s, rois=rects)
                for i, r in enumerate(rects):
                    if st[i] != mjx.OK or not np.array_equal(fb.rgb(i), crop(full, r)):
                        bad.append((name, s, r, "decode_batch device_destuff=%s" % dd, st[i]))
                fb.close()
    ctx.close()
    print(json.dumps({"bad": bad[:40], "nbad": len(bad), "rectangles": nrect, "worst": worst}))


def run_child(tmp_path, call, env_set=None, timeout=1500):
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_roi_decode as t\nt.%s\n" % (ROOT, ROOT, call))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    env.update(env_set or {})
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
@pytest.mark.parametrize("group", GROUPS)
def test_every_rectangle_equals_the_crop_of_the_uncropped_decode(mjx, tmp_path, group, single_decode):
    res = run_child(tmp_path, "child_equality(%r)" % group, {} if single_decode is None else {"MJX_SINGLE_DECODE": single_decode})
    assert res["nbad"] == 0, res
    assert res["rectangles"] > 100 and res["worst"]["max_diff"] <= TOL and res["worst"]["share"] < 0.01, res


# ---- GPU: in-process checks ---------------------------------------------------------------------------------------------------------
def _hip(mjx):
    """The HIP runtime the library itself is linked against, found through the library's own handle (a second copy of the runtime
    loaded by name -- another package may bundle one -- would not know the library's device pointers)."""
    h = mjx.lib()
    h.hipMemset.restype = h.hipMemcpy.restype = h.hipDeviceSynchronize.restype = ctypes.c_int
    h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipDeviceSynchronize.argtypes = []
    return h


def _full(mjx, ctx, data, scale):
    scan = mjx.ParsedScan(data)
    b = mjx.Batch(ctx, [scan], scale=scale)
    try:
        b.decode()
        b.wait()
        assert b.status(0) == mjx.OK, b.status(0)
        return b.rgb(0)
    finally:
        b.close()
        scan.close()


def _mixed_inputs(mjx, orc):
    """pictures of every stream kind and mode: 4:2:0 and generic single-scan (quad-interleaved), restart intervals (linear), a
    multi-scan twin read from its scans (planar) and one that is gathered, grey, and one undecodable file"""
    src = layout_data(LAYOUTS[48], 1000, 40)
    twins = jw.script_twins(src, orc.decode(src, layout=orc.LAYOUT_STD), ["Y;Cb;Cr"])
    src2 = layout_data(LAYOUTS[63], 333, 217)
    twins2 = jw.script_twins(src2, orc.decode(src2, layout=orc.LAYOUT_STD), ["Cb;Y;Cr"])
    return [mjx.synth_jpeg(750, 595, "420", 75, seed=1), mjx.synth_jpeg(333, 217, "422", 75, seed=2), layout_data(LAYOUTS[48], 333, 217, restart=5),
            twins[0], twins2[0], mjx.synth_jpeg(61, 45, "gray", 75, seed=3), _read(os.path.join(ROOT, "tests", "golden", "pil", "progressive.jpg")),
            mjx.synth_jpeg(1001, 37, "444", 75, seed=4), mjx.synth_jpeg(640, 480, "420", 92, seed=5)]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_images", [0, 2])
@pytest.mark.parametrize("scale", SCALES)
def test_mixed_batch_and_nothing_written_outside(mjx, orc, gpu_ctx, scale, chunk_images):
    datas = _mixed_inputs(mjx, orc)
    undecodable = 6
    sizes = []
    for i, d in enumerate(datas):
        w, h, hmax, vmax, _ = frame_of(d) if i != undecodable else (8, 8, 1, 1, 1)
        sizes.append((-(-w // scale), -(-h // scale), 8 // scale * hmax, 8 // scale * vmax))
    rois = []
    for i, (ow, oh, mw, mh) in enumerate(sizes):
        rs = rectangles(ow, oh, mw, mh, seed=77 + i)
        rois.append(rs[0] if i in (1, 7) else rs[7 + i % (len(rs) - 7)] if len(rs) > 7 else rs[-1])
    bad_rect = 4
    rois[bad_rect] = (0, 0, sizes[bad_rect][0] + 1, 1)
    scans = [mjx.ParsedScan(d) for d in datas if d is not datas[undecodable]]
    descs = scans[:undecodable] + [mjx.ScanDesc()] + scans[undecodable:]         # (an empty descriptor: refused at plan time)
    b = mjx.Batch(gpu_ctx, descs, scale=scale, rois=rois, chunk_images=chunk_images)
    hip = _hip(mjx)
    try:
        good = [i for i in range(len(datas)) if i not in (bad_rect, undecodable)]
        assert b.create_status[bad_rect] == mjx.ERR_INVALID_ARG and b.create_status[undecodable] != mjx.OK, b.create_status
        assert [b.create_status[i] for i in good] == [mjx.OK] * len(good), b.create_status
        # a pattern over the whole of the pictures' regions, then the decode: only the rectangles' bytes may change
        regions = {i: b.rgb_device(i) for i in good}
        lo = min(p for p, _ in regions.values())
        hi = max((p + n + 255) // 256 * 256 for p, n in regions.values())
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemset(lo, 0xA5, hi - lo) == 0
        assert hip.hipDeviceSynchronize() == 0
        b.decode()
        b.wait()
        pool = np.empty(hi - lo, np.uint8)
        assert hip.hipMemcpy(pool.ctypes.data, lo, hi - lo, 2) == 0
        covered = np.zeros(hi - lo, bool)
        total_bytes = total_pixels = 0
        for i in good:
            assert b.status(i) == mjx.OK, (i, b.status(i))
            full = _full(mjx, gpu_ctx, datas[i], scale)
            want = crop(full, rois[i])
            p, n = regions[i]
            assert n == want.nbytes and p % 256 == 0, (i, n, want.nbytes)
            assert np.array_equal(pool[p - lo:p - lo + n].reshape(want.shape), want), ("picture", i, rois[i])
            assert np.array_equal(b.rgb(i), want), i
            covered[p - lo:p - lo + n] = True
            inf, roi = b.info(i), b.roi(i)
            assert (inf["width"], inf["height"]) == (want.shape[1], want.shape[0]), (i, inf)
            x, y, w, h = rois[i]
            assert (roi["x"], roi["y"]) == ((x, y) if w else (0, 0)) and (roi["full_width"], roi["full_height"]) == (full.shape[1], full.shape[0]), (i, roi)
            assert (roi["w"], roi["h"]) == (want.shape[1], want.shape[0])
            total_bytes += want.nbytes
            total_pixels += want.shape[0] * want.shape[1]
            # the picture alone gives the same bytes
            one = mjx.Batch(gpu_ctx, [descs[i]], scale=scale, rois=rois[i])
            try:
                one.decode(); one.wait()
                assert one.status(0) == mjx.OK and np.array_equal(one.rgb(0), want), i
            finally:
                one.close()
        assert np.all(pool[~covered] == 0xA5), ("bytes outside the results were written", np.argwhere((pool != 0xA5) & ~covered)[:8].ravel().tolist())
        assert b.status(bad_rect) == mjx.ERR_INVALID_ARG and b.status(undecodable) != mjx.OK
        assert b.bytes()["rgb"] == total_bytes and b.bytes()["pixels"] == total_pixels
        if chunk_images:
            assert b.geometry()["chunks"] >= 3
    finally:
        b.close()
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_n_rois_mismatches_fail_the_call(mjx, gpu_ctx):
    datas = [mjx.synth_jpeg(64, 48, "420", 75, seed=k) for k in range(3)]
    scans = [mjx.ParsedScan(d) for d in datas]
    try:
        for rois in ([(0, 0, 8, 8)] * 2, [(0, 0, 8, 8)] * 4):
            with pytest.raises(mjx.MjxError) as e:
                mjx.Batch(gpu_ctx, scans, rois=rois)
            assert e.value.code == mjx.ERR_INVALID_ARG
            with pytest.raises(mjx.MjxError) as e:
                mjx.decode_batch(gpu_ctx, datas, rois=rois)
            assert e.value.code == mjx.ERR_INVALID_ARG
            pool = mjx.Pool([0])
            try:
                with pytest.raises(mjx.MjxError) as e:
                    pool.decode_batch(datas, rois=rois)
                assert e.value.code == mjx.ERR_INVALID_ARG
            finally:
                pool.close()
        arr = (mjx.ScanDesc * 3)()
        for i, s in enumerate(scans):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(s.desc), ctypes.sizeof(mjx.ScanDesc))
        o = mjx._opts()
        o.n_rois = 3                                                       # a count without an array
        h, st = ctypes.c_void_p(), (ctypes.c_int * 3)()
        assert mjx.lib().mjx_batch_create(gpu_ctx.h, arr, 3, ctypes.byref(o), ctypes.byref(h), st) == mjx.ERR_INVALID_ARG
        with pytest.raises(mjx.MjxError) as e:
            mjx.decode(datas[0], roi=[(0, 0, 8, 8)] * 2)
        assert e.value.code == mjx.ERR_INVALID_ARG
        b = mjx.Batch(gpu_ctx, scans, rois=[(0, 0, 8, 8)])                # one rectangle for every input
        try:
            assert [b.info(i)["width"] for i in range(3)] == [8, 8, 8]
        finally:
            b.close()
    finally:
        for s in scans:
            s.close()


@pytest.mark.gpu
def test_every_front_door_gives_the_batch_bytes(mjx, orc, gpu_ctx, tmp_path):
    paths = [os.path.join(ROOT, "tests", "data", "lena.jpeg"), os.path.join(ROOT, "tests", "golden", "pil", "dri_422_rows.jpg"),
             os.path.join(ROOT, "tests", "golden", "pil", "ms_420_odd.jpg"), os.path.join(ROOT, "tests", "data", "lena-bw.jpeg")]
    datas = [_read(p) for p in paths] + [mjx.synth_jpeg(1920, 1080, "420", 75, seed=9)]
    cli = os.path.join(os.path.dirname(mjx.lib_path()), "mjx_cli")
    for s in SCALES:
        fulls = [_full(mjx, gpu_ctx, d, s) for d in datas]
        rois = []
        for i, (d, f) in enumerate(zip(datas, fulls)):
            _, _, hmax, vmax, _ = frame_of(d)
            rois.append(rectangles(f.shape[1], f.shape[0], 8 // s * hmax, 8 // s * vmax, seed=5 + i)[7 + (i + s) % 3])
        want = [crop(f, r) for f, r in zip(fulls, rois)]
        for d, r, w in zip(datas, rois, want):
            assert np.array_equal(mjx.decode(d, scale=s, roi=r), w), (s, r)                          # mjx_decode
            img = mjx.JPEGImage.parse(d, ctx=gpu_ctx, scale=s, roi=r)
            assert (img.width(), img.height()) == (w.shape[1], w.shape[0]) and np.array_equal(img.image_data(), w)
        for dd in (True, False):                                                                     # mjx_decode_batch
            b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd, scale=s, rois=rois)
            try:
                assert st == [mjx.OK] * len(datas)
                for i, w in enumerate(want):
                    assert np.array_equal(b.rgb(i), w), (dd, s, i)
                    assert b.rgb_device(i)[1] == w.nbytes and b.roi(i)["x"] == rois[i][0]
                assert b.bytes()["rgb"] == sum(w.nbytes for w in want)
            finally:
                b.close()
        for devs in ([0], [0, 0]):                                                                   # mjx_pool: the deal reorders the files
            pool = mjx.Pool(devs)
            try:
                r = pool.decode_batch(datas, scale=s, rois=rois)
                try:
                    assert r.status == [mjx.OK] * len(datas)
                    if len(devs) == 2:
                        assert len(set(r.slot_of)) == 2 and r.slot_of != sorted(r.slot_of), r.slot_of
                    for i, w in enumerate(want):
                        assert np.array_equal(r.rgb(i), w), (devs, s, i)
                finally:
                    r.close()
            finally:
                pool.close()
        out = tmp_path / "o.ppm"                                                                     # the CLI
        args = [cli, paths[0], str(out), "--p6", "--crop", "%d,%d,%d,%d" % rois[0]] + (["--scale", str(s)] if s > 1 else [])
        subprocess.check_call(args)
        head = out.read_bytes().split(b"\n", 3)
        assert head[0] == b"P6" and head[1] == b"%d %d" % (want[0].shape[1], want[0].shape[0])
        assert np.array_equal(np.frombuffer(head[3], np.uint8).reshape(want[0].shape), want[0])
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, scale=s, rois=rois)                                            # tile() keeps the rectangles
        try:
            b.decode(); b.wait()
            t = b.tile(3)
            try:
                t.decode()
                t.wait()
                n = len(datas)
                for i in range(3 * n):
                    assert (t.info(i)["width"], t.info(i)["height"]) == (want[i % n].shape[1], want[i % n].shape[0])
                    assert t.roi(i) == b.roi(i % n)
                    assert np.array_equal(t.rgb(i), want[i % n]), (s, i)
                mx, cnt = t.compare_rgb(list(range(3 * n)), b, [i % n for i in range(3 * n)])
                assert int(mx.max()) == 0 and int(cnt.sum()) == 0
            finally:
                t.close()
        finally:
            b.close()
            for sc in scans:
                sc.close()
    assert subprocess.call([cli, paths[0], str(tmp_path / "x.ppm"), "--crop", "500,500,100,100"]) == mjx.ERR_INVALID_ARG
    assert subprocess.call([cli, paths[0], str(tmp_path / "x.ppm"), "--crop", "1,2,3"]) == mjx.ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2])
def test_larger_tiled_batch(mjx, gpu_ctx, scale):
    """3 unique 4K pictures tiled 22 times with the centre 1920 x 1080 rectangle (of the scaled picture: its centre quarter)"""
    datas = [mjx.synth_jpeg(3840, 2160, "420", 75, seed=40 + k) for k in range(3)]
    ow, oh = 3840 // scale, 2160 // scale
    roi = (ow // 4, oh // 4, ow // 2, oh // 2)
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(gpu_ctx, scans, scale=scale, rois=roi)
    whole = mjx.Batch(gpu_ctx, scans, scale=scale)
    try:
        t, tw = b.tile(22), whole.tile(22)                   # 66 pictures each
        try:
            for x in (t, tw):
                x.decode()
                x.wait()
                assert x.unconverged_runs() == 0
            for k in range(3):
                assert np.array_equal(t.rgb(k), crop(tw.rgb(k), roi)), (scale, k)
                assert np.array_equal(t.rgb(63 + k), crop(tw.rgb(63 + k), roi)), (scale, k)
            mine = list(range(3, len(t)))
            mx, cnt = t.compare_rgb(mine, t, [i % 3 for i in mine])
            assert int(mx.max()) == 0 and int(cnt.sum()) == 0
            assert t.bytes()["rgb"] == 66 * roi[2] * roi[3] * 3
        finally:
            t.close()
            tw.close()
    finally:
        b.close()
        whole.close()
        for s in scans:
            s.close()

"""Pictures one MCU wide, one MCU tall and 65535 on a side; MCU counts on both sides of every DC segment boundary.

Everything behind the entropy stage depends on how MCUs map to rows and columns: a stage-B tile is T consecutive MCUs in raster
order (mjx_plan_tiles reports T), phase 3 derives (mx, my) = (m % mcux, m / mcux) per lane, the multi-scan read is direct or
gathered by how many MCU rows a tile touches, rectangles skip tiles by row and by column, the row alignment of the store is
(width * 3) & 3, and DC prediction carries sums between segments of kDcSegMcus = 2048 MCUs.  The rest of the suite exercises one
regime of that mapping: rows much longer than a tile, a few thousand MCUs.  This module holds the other regimes.

The geometry family (family(); mw x mh: the MCU's pixel size), per layout:
  item 1  columns    mcux in {1, 2, 3, T - 1}, at least three tiles, nmcu no multiple of T; the last MCU column full, one pixel
                     short, and one pixel wide
  item 2  one tile per row   mcux in {T, T + 1, 2T - 1}, three MCU rows, the last one clipped to one pixel
  item 3  rows       mcuy in {1, 2}, W in {65535, 65528, 65521}: row bytes mod 4 = 1, 0, 3
  item 4  the header's limits   H = 65535 with W in {1, 8, 16, 17} and W = 65535 with H in {1, 8, 16, 17}; 65535 x 48 and 48 x 65535
                     in 4:2:0 (3.1 Mpixels, the largest pictures here; 65535 x 65535 is out of scope)
4:2:0 and 4:4:4 take all of it; 4:2:2, 4:4:0, grey, Y22_Cb21_Cr12 (12 blocks), Y21_Cb12_Cr11 (5 blocks) and gray22 take
mcux in {1, T - 1, T + 1} and one picture each of items 3 and 4.  test_coverage_table prints and asserts the (layout x item) cells.

The DC family (dc_file()): DC-only blocks with quantiser 1 written by jpegwriter.jpeg_from_blocks, nmcu = 2048 k + r for k in {1, 2}
and r in {-1, 0, 1, 8, 9}, one MCU wide wherever the frame header allows it, for 1, 2 (the pair scan of a multi-scan twin), 3, 4, 5, 6
and 12 blocks per MCU; every component's DC is drawn over the whole range -1024 .. 1023, so differences reach +-2047 and every
segment's per-component sum is large and distinct.  The same blocks with restart intervals of 1 and of 2049 MCUs.  The pictures
compared as bytes at scale 8 carry luminance levels -40 .. 300 (quantiser 8: the level is DC + 128) and no chroma.

Every comparison is one the suite already has, with its tolerance: T0 bit for bit, RGB within TOL = 1 and under 1 % of bytes
(test_sampling_layouts.rgb_problem), scaled pictures against scaled_ref, rectangles byte for byte the crop of the uncropped decode,
formats through test_output_formats.expected, luminance and libjpeg pixels inside the float64 interval, orientation as the mapped
bytes, resize through test_resize.check_against.  Pillow refuses sides above 65500, so these files have no Pillow twin.

The CPU tests run first and catch an out-of-range plan before anything is launched: tile counts against a brute-force count,
layouts and plans, REF_COMPAT panic detection against the oracle, the emulated entropy stage, the DC family through the oracle, and
three mutations of Python restatements (the tile-to-pixel map, the DC carry, the tile-wanted rule) that the family must catch.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import jpegwriter as jw
import oracle_binding as orc_mod
import scaled_ref
import test_libjpeg_pixels as tlp
import test_luma_output as tlo
import test_multiscan_scripts as tms
import test_orientation as tor
import test_output_formats as tof
import test_resize as trs
import test_roi_decode as roi
import test_sampling_layouts as tsl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = tsl.TOL
SCALES = (2, 4, 8)
SIDE = 65535
SYNTH = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "gray": [(1, 1)]}
WRITER = ["Y22_Cb21_Cr12", "Y21_Cb12_Cr11", "gray22"]
LAYOUTS = list(SYNTH) + WRITER
FULL = ("420", "444")                       # the layouts that take every case of items 1 to 4
ITEMS = (1, 2, 3, 4)
# the tile sizes the family is built for; test_tile_sizes_are_the_planners asserts them against mjx_plan_tiles
NAMED_T = {"420": 32, "422": 32, "440": 32, "444": 64, "gray": 128, "Y22_Cb21_Cr12": 16, "gray22": 128}
ORDINARY = (333, 217)
F16_BGR = tof.FORMATS.index(("float16", False, True))           # interleaved f16 B,G,R (planar f32: test_resize.F32_PLANAR)


def hv_of(layout):
    """the MCU's sampling factors (one component: a non-interleaved scan, one block per MCU whatever the frame header says)"""
    if layout in SYNTH:
        return SYNTH[layout]
    return [(1, 1)] if layout.startswith("gray") else tsl.parse_name(layout)


def mcu_px(layout):
    hv = hv_of(layout)
    return 8 * max(h for h, _ in hv), 8 * max(v for _, v in hv)


def tile_rule(layout, scale=1):
    """tile_mcus as test_sampling_layouts.planar_fits restates it: 32 for 4:2:0 at full size, else the largest power of two with
    T * bpm <= 192, at most 128 / hmax"""
    hv = hv_of(layout)
    bpm, hmax = sum(a * b for a, b in hv), max(a for a, _ in hv)
    if hv == SYNTH["420"] and scale == 1:
        return 32
    t = 1
    while t * 2 * bpm <= 192:
        t *= 2
    return min(t, 128 // hmax)


def name_for_rules(layout):
    """the layout's name in test_sampling_layouts' scheme (for planar_direct)"""
    return tsl.name(SYNTH[layout]) if layout in SYNTH and layout != "gray" else layout


@functools.lru_cache(maxsize=None)
def file_of(layout, w, h):
    """the bytes of one family picture: the project's generator for the five named schemes, jpegwriter.layout_jpeg for the rest"""
    if layout in SYNTH:
        import __graft_entry__ as ge
        return ge.load_package().synth_jpeg(w, h, layout, 75, seed=w * 7 + h)
    return tsl.data_of(layout, w, h)


def oracle(data):
    return tsl.oracle_std(data)


def rows_for(mcux, T):
    """the fewest MCU rows that give more than two tiles' worth of MCUs, their count no multiple of T"""
    mcuy = -(-(2 * T + 3) // mcux)
    while (mcux * mcuy) % T == 0:
        mcuy += 1
    return mcuy


def _widths(mcux, mw):
    return [mcux * mw, mcux * mw - 1, (mcux - 1) * mw + 1]


@functools.lru_cache(maxsize=None)
def family():
    """[case]: name, layout, item, w, h, mcux, mcuy, T -- built from tile_rule; the planner's own T is asserted in
    test_tile_sizes_are_the_planners before any other test relies on it"""
    out = []

    def add(layout, item, w, h, T):
        mw, mh = mcu_px(layout)
        assert 1 <= w <= SIDE and 1 <= h <= SIDE, (layout, item, w, h)
        out.append(types.SimpleNamespace(name="%s_%dx%d" % (layout, w, h), layout=layout, item=item, w=w, h=h, mcux=-(-w // mw),
                                         mcuy=-(-h // mh), T=T, mw=mw, mh=mh))
    for k, layout in enumerate(LAYOUTS):
        T = tile_rule(layout)
        mw, mh = mcu_px(layout)
        full = layout in FULL
        # item 1: columns
        for j, mcux in enumerate([1, 2, 3, T - 1] if full else [1, T - 1]):
            mcuy = rows_for(mcux, T)
            heights = [mcuy * mh, mcuy * mh - 1, (mcuy - 1) * mh + 1]
            ws = _widths(mcux, mw)
            for i, w in enumerate(ws if full else [ws[2 - j]]):
                add(layout, 1, w, heights[(i + j + k) % 3], T)
        # item 2: around one tile per row, the last of three MCU rows one pixel high
        for j, mcux in enumerate([T, T + 1, 2 * T - 1] if full else [T + 1]):
            add(layout, 2, _widths(mcux, mw)[(j + k) % 3], 2 * mh + 1, T)
        # item 3: rows
        for i, w in enumerate([SIDE, SIDE - 7, SIDE - 14] if full else [SIDE - 14]):
            if full:
                add(layout, 3, w, [mh - 1, mh - 3, 1][i], T)
            add(layout, 3, w, [mh + 2, mh + 1, 2 * mh][i] if full else mh + 1, T)
        # item 4: the header's limits
        if full:
            for v in (1, 8, 16, 17):
                add(layout, 4, v, SIDE, T)
                add(layout, 4, SIDE, v, T)
            if layout == "420":
                add(layout, 4, SIDE, 48, T)
                add(layout, 4, 48, SIDE, T)
        elif k % 2:
            add(layout, 4, SIDE, 17, T)
        else:
            add(layout, 4, 17, SIDE, T)
    assert len({c.name for c in out}) == len(out) and len(out) <= 150, len(out)
    return out


def data_of(case):
    return file_of(case.layout, case.w, case.h)


def cases_of(layout=None, items=ITEMS):
    return [c for c in family() if (layout is None or c.layout == layout) and c.item in items]


def one_per_item():
    """one file per item, of different layouts, the 12-block MCU and a grey frame among them"""
    picks = [("420", 1), ("Y22_Cb21_Cr12", 2), ("444", 3), ("gray22", 4)]
    return [[c for c in family() if c.layout == l and c.item == i][0] for l, i in picks]


def derived_cases(layout):
    """one narrow (item 1, one MCU wide), one wide (item 3) and one item-4 file of the layout"""
    fam = cases_of(layout)
    return [[c for c in fam if c.item == 1 and c.mcux == 1][0], [c for c in fam if c.item == 3][-1], [c for c in fam if c.item == 4][-1]]


# ---- CPU: the family itself ----------------------------------------------------------------------------------------------------------
def test_tile_sizes_are_the_planners(mjx):
    """T of every layout at every scale comes from mjx_plan_tiles; the family is built for exactly these values."""
    for layout in LAYOUTS:
        scan = mjx.ParsedScan(file_of(layout, *ORDINARY))
        try:
            for s in (1,) + SCALES:
                assert scan.plan_tiles(scale=s)["tile_mcus"] == tile_rule(layout, s), (layout, s)
        finally:
            scan.close()
        if layout in NAMED_T:
            assert tile_rule(layout) == NAMED_T[layout], layout
    assert tile_rule("Y21_Cb12_Cr11") == 32


def test_coverage_table():
    """(layout x item) cells: none that is required is empty, and each holds what the item is aimed at."""
    fam = family()
    table = {(l, i): [c for c in fam if c.layout == l and c.item == i] for l in LAYOUTS for i in ITEMS}
    print("%-16s %s" % ("layout", "  ".join("item %d" % i for i in ITEMS)))
    for l in LAYOUTS:
        print("%-16s %s" % (l, "  ".join("%6d" % len(table[(l, i)]) for i in ITEMS)))
    print("files: %d" % len(fam))
    for l in LAYOUTS:
        T, (mw, mh) = tile_rule(l), mcu_px(l)
        c1, c2, c3, c4 = (table[(l, i)] for i in ITEMS)
        assert all(c for c in (c1, c2, c3, c4)), l
        want1 = {1, 2, 3, T - 1} if l in FULL else {1, T - 1}
        assert {c.mcux for c in c1} == want1, (l, sorted({c.mcux for c in c1}))
        for c in c1:
            n = c.mcux * c.mcuy
            assert n > 2 * T and n % T, (c.name, n)
        ends = {(c.mcux, c.w - (c.mcux - 1) * mw) for c in c1}                   # how many pixels the last MCU column holds
        if l in FULL:
            assert ends == {(m, e) for m in want1 for e in (mw, mw - 1, 1)}, l
        else:
            assert {e for _, e in ends} <= {mw, mw - 1, 1} and len(ends) == 2, l
        want2 = {T, T + 1, 2 * T - 1} if l in FULL else {T + 1}
        assert {c.mcux for c in c2} == want2 and all(c.mcuy == 3 and c.h == 2 * mh + 1 for c in c2), l
        assert all(c.mcuy in (1, 2) and c.w in (SIDE, SIDE - 7, SIDE - 14) for c in c3), l
        if l in FULL:
            assert {(c.mcuy, (c.w * 3) & 3) for c in c3} == {(y, r) for y in (1, 2) for r in (1, 0, 3)}, l
            assert {(c.w, c.h) for c in c4} >= {(v, SIDE) for v in (1, 8, 16, 17)} | {(SIDE, v) for v in (1, 8, 16, 17)}, l
        else:
            assert (SIDE - 14) % 16 == 1 and c3[0].w == SIDE - 14
        assert all(SIDE in (c.w, c.h) for c in c4), l
    assert {(c.w, c.h) for c in table[("420", 4)]} >= {(SIDE, 48), (48, SIDE)}
    assert max(c.w * c.h for c in fam) == SIDE * 48
    assert len(fam) <= 150


# ---- the three restatements the mutation check runs against ------------------------------------------------------------------------
def tile_pixel_map(nmcu, mcux, T, mw, mh, mutate=False):
    """phase 3's map restated: lane i of tile t holds MCU m = t T + i and writes its patch at (mx mw, my mh), with
    (mx, my) = (m % mcux, m / mcux).  mutate: my = m / (mcux + 1).  -> int [nmcu, 2]: (x, y) of every MCU's patch"""
    out = np.empty((nmcu, 2), np.int64)
    for t in range(-(-nmcu // T)):
        for i in range(min(T, nmcu - t * T)):
            m = t * T + i
            out[m] = ((m % mcux) * mw, (m // (mcux + 1 if mutate else mcux)) * mh)
    return out


def raster_map(mcux, mcuy, mw, mh):
    yy, xx = np.mgrid[0:mcuy, 0:mcux]
    return np.stack([xx.ravel() * mw, yy.ravel() * mh], axis=1)


def tiles_wanted(case, scale, r, mutate=False):
    """the documented rule: a tile is wanted when one of its MCUs lies in the rectangle's MCU rows and columns.
    mutate: only the tile's first MCU is looked at."""
    if r[2] == 0 and r[3] == 0:
        return -(-(case.mcux * case.mcuy) // tile_rule(case.layout, scale))
    T = tile_rule(case.layout, scale)
    pw, ph = case.mw // scale, case.mh // scale
    x, y, rw, rh = r
    r0, r1, c0, c1 = y // ph, (y + rh - 1) // ph, x // pw, (x + rw - 1) // pw
    n = 0
    for t in range(-(-(case.mcux * case.mcuy) // T)):
        ms = range(t * T, min((t + 1) * T, case.mcux * case.mcuy))
        if mutate:
            ms = ms[:1]
        n += any(r0 <= m // case.mcux <= r1 and c0 <= m % case.mcux <= c1 for m in ms)
    return n


def limit_rects(ow, oh, mw, mh):
    """the four corners' single pixels, a one-pixel column at x in {0, W/2, W-1} over the full height, a one-pixel row likewise, the
    whole picture, and two unaligned interior rectangles (dropped where the picture has no interior)"""
    out = [(0, 0, 1, 1), (ow - 1, 0, 1, 1), (0, oh - 1, 1, 1), (ow - 1, oh - 1, 1, 1)]
    out += [(x, 0, 1, oh) for x in (0, ow // 2, ow - 1)] + [(0, y, ow, 1) for y in (0, oh // 2, oh - 1)] + [(0, 0, 0, 0)]
    x0, y0 = min(ow - 1, mw // 2 + 1), min(oh - 1, mh // 2 + 1)
    out.append((x0, y0, max(1, min(ow - x0, ow // 2 + 1)), max(1, min(oh - y0, oh // 2 + 1))))
    x1, y1 = ow // 3, oh // 3
    out.append((x1, y1, max(1, min(ow - x1, mw + 3)), max(1, min(oh - y1, mh + 2))))
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


def dc_scan_restated(diffs, restart=0, mutate=False, seg=2048, lane=8):
    """DC prediction as the kernels organise it: segments of `seg` MCUs, lanes of `lane` MCUs inside them (a shorter last run), the
    running sum carried from segment to segment, and set back to zero where a restart interval begins.
    diffs: int [nmcu, columns], one column per running sum.  mutate: the carry into a segment is dropped.
    -> the absolute DC values [nmcu, columns]"""
    d = np.asarray(diffs, np.int64)
    out = np.empty_like(d)
    carry = np.zeros(d.shape[1], np.int64)
    for s0 in range(0, len(d), seg):
        acc = np.zeros(d.shape[1], np.int64) if mutate else carry.copy()
        for l0 in range(s0, min(s0 + seg, len(d)), lane):
            for m in range(l0, min(l0 + lane, s0 + seg, len(d))):
                if restart and m % restart == 0:
                    acc[:] = 0
                acc = acc + d[m]
                out[m] = acc
        carry = acc
    return out


# ---- CPU: mutation check ---------------------------------------------------------------------------------------------------------------
def test_mutations_of_the_restatements_are_caught():
    """Each planted error in a restatement fails at least one case of the family: the map with my = m / (mcux + 1) against the raster
    enumeration of the MCU grid, the DC scan with a dropped carry against the blocks written, and the tile rule that looks at a tile's
    first MCU only against the brute-force count.  Prints which cases catch which."""
    fam = [c for c in family() if c.mcux * c.mcuy <= 20000]
    caught = []
    for c in fam:
        want = raster_map(c.mcux, c.mcuy, c.mw, c.mh)
        assert np.array_equal(tile_pixel_map(c.mcux * c.mcuy, c.mcux, c.T, c.mw, c.mh), want), c.name
        if not np.array_equal(tile_pixel_map(c.mcux * c.mcuy, c.mcux, c.T, c.mw, c.mh, mutate=True), want):
            caught.append(c.name)
    print("map mutation caught by %d of %d cases, e.g. %s" % (len(caught), len(fam), caught[:4]))
    missed = [c.name for c in fam if c.name not in caught]
    assert caught and all(c.mcuy == 1 for c in fam if c.name in missed), missed            # (one MCU row: my is 0 either way)
    assert any(c.mcux == 1 and c.name in caught for c in fam)
    dc_caught = []
    for k, r in DC_COUNTS:
        for rst in DC_RESTARTS:
            p = dc_picture(3, k, r)
            absolute = np.stack([p.per_comp[c][:, 0] for c in range(3)], axis=1)
            d = np.diff(absolute, axis=0, prepend=0)
            if rst:
                d[::rst] = absolute[::rst]
            assert np.array_equal(dc_scan_restated(d, rst), absolute), (k, r, rst)
            if not np.array_equal(dc_scan_restated(d, rst, mutate=True), absolute):
                dc_caught.append((2048 * k + r, rst))
    print("dropped carry caught at (nmcu, restart):", dc_caught)
    assert {n for n, rst in dc_caught if rst == 0} == {2048 * k + r for k, r in DC_COUNTS if 2048 * k + r > 2048}
    assert not [n for n, rst in dc_caught if rst == 1] and [n for n, rst in dc_caught if rst == 2049]
    roi_caught = []
    for c in cases_of(items=(1, 2)):
        for r in limit_rects(c.w, c.h, c.mw, c.mh):
            if tiles_wanted(c, 1, r, mutate=True) != tiles_wanted(c, 1, r):
                roi_caught.append((c.name, r))
    print("first-MCU-only rule caught by %d (case, rectangle) pairs, e.g. %s" % (len(roi_caught), roi_caught[:3]))
    assert roi_caught


# ---- CPU: plans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tile_counts(mjx, layout):
    """tiles_total = ceil(nmcu / T) at every scale; tiles_read equals the brute-force count over the MCU grid for the limit
    rectangles at scales 1 and 8 (test_roi_decode.enumerate_tiles, the restatement of the documented rule)."""
    bad, n = [], 0
    for c in cases_of(layout):
        scan = mjx.ParsedScan(data_of(c))
        try:
            hmax, vmax = c.mw // 8, c.mh // 8
            for s in (1,) + SCALES:
                whole = scan.plan_tiles(scale=s)
                T = whole["tile_mcus"]
                if whole["tiles_total"] != -(-(c.mcux * c.mcuy) // T) or whole["tiles_read"] != whole["tiles_total"] or T != tile_rule(layout, s):
                    bad.append((c.name, s, whole))
                if s not in (1, 8):
                    continue
                ow, oh = -(-c.w // s), -(-c.h // s)
                for r in limit_rects(ow, oh, c.mw // s, c.mh // s):
                    got = scan.plan_tiles(roi=r, scale=s)
                    want, _, total = roi.enumerate_tiles(c.w, c.h, hmax, vmax, s, T, r)
                    n += 1
                    if got["tiles_read"] != len(want) or got["tiles_total"] != total:
                        bad.append((c.name, s, r, got, len(want), total))
                    if c.mcux * c.mcuy <= 5000 and tiles_wanted(c, s, r) != len(want):
                        bad.append((c.name, s, r, "the two restatements differ"))
        finally:
            scan.close()
    assert bad == [], bad[:8]
    assert n >= 40


def twin_sources():
    """(layout, case) of the multi-scan sources: 16 wide, T + 1 MCUs wide and 65535 x 16, of 4:2:0 and the 12-block MCU"""
    out = []
    for layout in ("420", "Y22_Cb21_Cr12"):
        T = tile_rule(layout)
        for w, h in ((16, rows_for(1, T) * 16), ((T + 1) * 16, 33), (SIDE, 16)):
            out.append(types.SimpleNamespace(name="%s_%dx%d" % (layout, w, h), layout=layout, item=0, w=w, h=h, mcux=-(-w // 16),
                                             mcuy=-(-h // 16), T=T, mw=16, mh=16))
    return out


TWIN_SCRIPTS = ["Y;Cb;Cr", "Y;Cb Cr", "Cb Cr;Y"]                 # three single scans, luma then pair, pair first


@functools.lru_cache(maxsize=None)
def twins_of(layout, w, h):
    src = file_of(layout, w, h)
    return jw.script_twins(src, oracle(src), TWIN_SCRIPTS)


def test_plan_tiles_of_the_twins_counts_whole_tile_ranges(mjx):
    """The planar source counts whole tile ranges: between the set of wanted tiles and the band of the rectangle's MCU rows, and the
    oracle decodes every twin to its source's picture."""
    bad = []
    for c in twin_sources():
        src = data_of(c)
        for script, twin in zip(TWIN_SCRIPTS, twins_of(c.layout, c.w, c.h)):
            assert np.array_equal(oracle(twin).rgb, oracle(src).rgb), (c.name, script)
            scan = mjx.ParsedScan(twin)
            try:
                for s in (1, 8):
                    ow, oh = -(-c.w // s), -(-c.h // s)
                    for r in limit_rects(ow, oh, 16 // s, 16 // s):
                        got = scan.plan_tiles(roi=r, scale=s)
                        want, band, total = roi.enumerate_tiles(c.w, c.h, 2, 2, s, got["tile_mcus"], r)
                        if not (len(want) <= got["tiles_read"] <= band) or got["tiles_total"] != total:
                            bad.append((c.name, script, s, r, got, len(want), band))
            finally:
                scan.close()
    assert bad == [], bad[:8]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_and_plans(mjx, layout):
    """mjx_output_layout for packed u8, planar f32 and channels = 1; mjx_orient_plan for the transposing codes; mjx_resize_plan for a
    224 x 224 target: the auto-scale rule of test_resize and its tap counts."""
    for c in cases_of(layout):
        scan = mjx.ParsedScan(data_of(c))
        try:
            for s in (1, 8):
                ow, oh = -(-c.w // s), -(-c.h // s)
                got = scan.output_layout(mjx.Output("uint8"), scale=s)
                assert (got["width"], got["height"], got["row_pitch"], got["plane_pitch"], got["bytes"]) == (ow, oh, 3 * ow, 0, 3 * ow * oh), (c.name, s, got)
                got = scan.output_layout(mjx.Output("float32", planar=True), scale=s)
                assert (got["width"], got["height"], got["row_pitch"], got["plane_pitch"], got["bytes"]) == (ow, oh, ow, ow * oh, 12 * ow * oh), (c.name, s, got)
                got = scan.output_layout(mjx.Output("uint8", channels=1), scale=s)
                assert (got["width"], got["height"], got["row_pitch"], got["bytes"]) == (ow, oh, ow, ow * oh), (c.name, s, got)
            for code in (5, 6, 7, 8):
                p = scan.orient_plan(code)
                assert (p["width"], p["height"], p["stored_rect"], p["scale"]) == (c.h, c.w, (0, 0, c.w, c.h), 1), (c.name, code, p)
            p = scan.resize_plan(mjx.Resize(224, 224))
            s, rect = trs.auto_scale_rule(c.w, c.h, None, 224, 224)
            assert (p["scale"], p["rect"]) == (s, rect), (c.name, p, s, rect)
            assert (p["taps_x"], p["taps_y"]) == (max_taps(rect[2], 224), max_taps(rect[3], 224)), (c.name, p)
            if (c.w, c.h) == (SIDE, 16):
                assert (p["scale"], p["taps_x"], p["taps_y"]) == (1, 586, 2), p
        finally:
            scan.close()


def runs_past(layout, w, h):
    """test_sampling_layouts.ref_runs_past_the_scan; the generator's grey frames carry factors 1 x 1 and never do"""
    return layout in WRITER and tsl.ref_runs_past_the_scan(layout, w, h)


def ref_want(mjx, rc):
    """the status REF_COMPAT gives a family file, from the oracle's (test_sampling_layouts.test_validate's rule)"""
    return {orc_mod.OK: mjx.OK, orc_mod.ERR_REF_PANIC: mjx.ERR_REF_PANIC}[rc]


@functools.lru_cache(maxsize=None)
def oracle_ref(data):
    return tsl.oracle_ref(data)


def test_ref_compat_panic_detection_on_the_family(mjx):
    """The host's detection equals the oracle on every file: many of these geometries panic in the reference's placement code
    (fill_block_in_array: index out of bounds), the rest decode.  STANDARD accepts every file at every scale."""
    bad, npanic = [], 0
    for c in family():
        data = data_of(c)
        rc, _ = oracle_ref(data)
        scan = mjx.ParsedScan(data)
        try:
            for s in (1,) + SCALES:
                if scan.validate(scale=s) != mjx.OK:
                    bad.append((c.name, "STANDARD", s))
            got = scan.validate(layout=mjx.LAYOUT_REF_COMPAT)
        finally:
            scan.close()
        if runs_past(c.layout, c.w, c.h):
            # the reference panics while it reads past the scan (the oracle says so); the host cannot know that before decoding
            # and says OK (the decode finds it), unless the placement of such a frame panics as well, which it sees at once
            if rc != orc_mod.ERR_REF_PANIC or got not in (mjx.OK, mjx.ERR_REF_PANIC):
                bad.append((c.name, got, rc, "runs past the scan"))
            continue
        npanic += rc == orc_mod.ERR_REF_PANIC
        if got != ref_want(mjx, rc):
            bad.append((c.name, got, rc))
    assert bad == [], bad
    assert 10 < npanic < len(family()) - 10, npanic


# ---- CPU: the emulated entropy stage -------------------------------------------------------------------------------------------------
def _emul_lib(mjx):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libhuff_emul.so"))
    lib.emul_decode_coefs_sub.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    lib.emul_single_decode_cp.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                          ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    return lib


def test_emulated_entropy_stage_gives_the_oracles_t0(mjx):
    """emul_decode_coefs_sub and emul_single_decode_cp (tests/emul: the kernels' per-lane routine on the CPU) on one file per item:
    what the writers wrote is what the device is expected to read."""
    lib = _emul_lib(mjx)
    for c in one_per_item():
        data = data_of(c)
        want = orc_mod.interleave(oracle(data))
        cap = len(want) + 64
        for fn, args in ((lib.emul_decode_coefs_sub, (0, 0, 0)), (lib.emul_single_decode_cp, (0, 0, 0, 1024, 32, 1024))):
            out = np.zeros((cap, 64), np.int16)
            nb, st = ctypes.c_size_t(), (ctypes.c_int * 8)()
            rc = fn(data, len(data), *args, out.ctypes.data, cap, ctypes.byref(nb), st)
            assert rc == 0 and nb.value == len(want) and np.array_equal(out[:nb.value], want), (c.name, fn.__name__, rc, nb.value, list(st))


# ---- the DC family -------------------------------------------------------------------------------------------------------------------------
DC_COUNTS = [(k, r) for k in (1, 2) for r in (-1, 0, 1, 8, 9)]
DC_RESTARTS = (0, 1, 2049)
DC_LAYOUTS = {1: "gray", 3: "444", 4: "422", 6: "420", 5: "Y21_Cb12_Cr11", 12: "Y22_Cb21_Cr12"}          # by blocks per MCU
DC_FAST, DC_GENERIC = (1, 3, 4, 6), (5, 12, 2)           # k_dc_scan_t<1|3|4|6>; the generic kernels (2: the pair scan of a 4:4:4 twin)


def dc_grid(layout, nmcu):
    """one MCU wide where 65535 rows allow it, else the smallest divisor of nmcu above 1 that does"""
    _, mh = mcu_px(layout)
    mcux = 1
    while nmcu % mcux or (nmcu // mcux) * mh > SIDE:
        mcux += 1
    return mcux, nmcu // mcux


@functools.lru_cache(maxsize=None)
def dc_picture(bpm, k, r, levels=False):
    """-> .hv, .mcux, .mcuy, .per_comp (absolute DC per component's blocks), .blocks (int16 [nmcu bpm, 64], what T0 must be), .qts.
    The DC of each component: drawn over the whole range -1024 .. 1023 with both extremes side by side, so differences reach +-2047
    in both directions.  levels: luminance DC in -168 .. 172 with quantiser 8 (levels -40 .. 300) and no chroma."""
    layout = DC_LAYOUTS[3 if bpm == 2 else bpm]
    hv = hv_of(layout)
    nmcu = 2048 * k + r
    mcux, mcuy = dc_grid(layout, nmcu)
    rng = np.random.RandomState(1000 * bpm + 10 * nmcu + int(levels))
    per_comp = []
    for c, (h, v) in enumerate(hv):
        co = np.zeros((nmcu * h * v, 64), np.int64)
        if levels:
            if c == 0:
                co[:, 0] = rng.randint(-168, 173, len(co))
        else:
            co[:, 0] = rng.randint(-1024, 1024, len(co))
            at = 2048 * h * v - 4 + c                       # the extremes straddle the first segment boundary of the component
            if at + 4 <= len(co):
                co[at:at + 4, 0] = [-1024, 1023, -1024, 1023]
            co[:3, 0] = [1023, -1024, 1023]
        per_comp.append(co)
    per_mcu = [h * v for h, v in hv]
    blocks = np.concatenate([p.reshape(nmcu, n, 64) for p, n in zip(per_comp, per_mcu)], axis=1).reshape(-1, 64)
    q = 8 if levels else 1
    return types.SimpleNamespace(bpm=bpm, layout=layout, hv=hv, nmcu=nmcu, mcux=mcux, mcuy=mcuy, per_comp=per_comp, blocks=blocks.astype(np.int16),
                                 qts=[np.full(64, q)] * len(hv), w=mcux * mcu_px(layout)[0], h=mcuy * mcu_px(layout)[1],
                                 dec=types.SimpleNamespace(coefs=per_comp, mcus=nmcu))


@functools.lru_cache(maxsize=None)
def dc_file(bpm, k, r, restart=0, levels=False):
    """the file of dc_picture(bpm, k, r) with a restart interval of `restart` MCUs; bpm = 2: the 'Y Cb;Cr' twin of the 4:4:4 file,
    whose pair scan carries two blocks per MCU (its restart interval counts that scan's MCUs)"""
    p = dc_picture(bpm, k, r, levels)
    src = jw.jpeg_from_blocks(p.blocks, p.hv, p.mcux, p.mcuy, p.qts, jw._annex_k_tables(), restart=(restart or None) if bpm != 2 else None)
    if bpm != 2:
        return src
    return jw.script_twin(src, p.dec, "Y Cb;Cr", restart=restart or None)


def dc_cases(bpms, restarts=DC_RESTARTS):
    return [(b, k, r, rst) for b in bpms for k, r in DC_COUNTS for rst in restarts]


@pytest.mark.parametrize("bpm", DC_FAST + DC_GENERIC)
def test_dc_family_through_the_oracle(orc, bpm):
    """The oracle's T0 is exactly the blocks written, with and without restart intervals; differences reach +-2047."""
    for k, r in DC_COUNTS:
        p = dc_picture(bpm, k, r)
        d = np.diff(p.per_comp[0][:, 0])
        assert d.max() == 2047 and d.min() == -2047
        for rst in DC_RESTARTS:
            dec = orc.decode(dc_file(bpm, k, r, rst), layout=orc.LAYOUT_STD, ext_dri=True, ext_multiscan=True)
            assert dec.mcus == p.nmcu and np.array_equal(orc.interleave(dec), p.blocks), (bpm, k, r, rst)
    p = dc_picture(bpm, 1, 1, levels=True)
    want = np.clip(p.per_comp[0][:, 0] + 128, 0, 255)
    assert want.min() == 0 and want.max() == 255 and (p.per_comp[0][:, 0] + 128).min() == -40 and (p.per_comp[0][:, 0] + 128).max() == 300


def dc_level_picture(p):
    """the picture of a `levels` file at scale 8: one pixel per luminance block, its clamped level, R = G = B"""
    h, v = p.hv[0]
    hmax, vmax = max(a for a, _ in p.hv), max(b for _, b in p.hv)
    lv = np.clip(p.per_comp[0][:, 0] + 128, 0, 255).astype(np.uint8)
    plane = lv.reshape(p.mcuy, p.mcux, v, h).transpose(0, 2, 1, 3).reshape(p.mcuy * v, p.mcux * h)
    plane = np.repeat(np.repeat(plane, vmax // v, axis=0), hmax // h, axis=1)
    return np.repeat(plane[:, :, None], 3, axis=2)


def test_dc_level_picture_is_the_float64_reference(orc):
    for bpm in DC_FAST + DC_GENERIC[:2]:
        p = dc_picture(bpm, 1, 9, levels=True)
        assert np.array_equal(dc_level_picture(p), scaled_ref.scaled_rgb(dc_file(bpm, 1, 9, levels=True), 8, p.dec)), bpm


# ---- CPU: the resize reference on long rows ------------------------------------------------------------------------------------------------
def resize_ref_banded(img, width, height, antialias):
    """test_resize.resize_ref for pictures too long for its dense [n_out, n_in] matrices: the same weights (axis_matrix's formula per
    output coordinate), applied window by window, the vertical pass first."""
    a = np.asarray(img, np.float64)

    def along(a, n_out):
        n_in = a.shape[0]
        r = n_in / n_out
        fs = max(1.0, r) if antialias else 1.0
        out = np.empty((n_out,) + a.shape[1:], np.float64)
        for X in range(n_out):
            c = (X + 0.5) * r
            lo, hi = max(0, int(np.floor(c - fs + 0.5))), min(n_in, int(np.floor(c + fs + 0.5)))
            w = np.maximum(0.0, 1.0 - np.abs(np.arange(lo, hi) + 0.5 - c) / fs)
            out[X] = np.tensordot(w / w.sum(), a[lo:hi], axes=(0, 0))
        return out
    return along(along(a, height).transpose(1, 0, 2), width).transpose(1, 0, 2)


def max_taps(n_in, n_out):
    """test_resize.max_taps (antialias on) without the dense matrix: the most non-zero weights of any output coordinate, a weight
    being 1 - |j + 0.5 - c| / fs over the window axis_matrix gives coordinate X"""
    r = n_in / n_out
    fs = max(1.0, r)
    c = (np.arange(n_out) + 0.5) * r
    lo, hi = np.maximum(0, np.floor(c - fs + 0.5)), np.minimum(n_in, np.floor(c + fs + 0.5))
    first, last = np.floor(c - fs - 0.5) + 1, np.ceil(c + fs - 0.5) - 1              # the integers j with |j + 0.5 - c| < fs
    return int((np.minimum(hi - 1, last) - np.maximum(lo, first) + 1).max())


RESIZE_TARGETS = ((224, 224), "long")           # "long": 7 x 65535 for a tall picture, 65535 x 7 for a wide one


def resize_target(c, t):
    if t != "long":
        return t
    return (7, SIDE) if c.h >= c.w else (SIDE, 7)


@functools.lru_cache(maxsize=None)
def _u8_eligible(rect_wh, target):
    return all(trs.Fraction(n_in, n_out).denominator >= 5 and max_taps(n_in, n_out) <= 30 for n_in, n_out in zip(rect_wh, target))


def u8_eligible(mjx, c, t):
    """test_resize.u8_eligible for the planned rectangle (its max_taps builds dense matrices; this one does not)"""
    tw, th = resize_target(c, t)
    plan = mjx.resize_plan(data_of(c), mjx.Resize(tw, th))
    return _u8_eligible(tuple(plan["rect"][2:]), (tw, th))


def test_resize_reference_and_band_share(mjx):
    """resize_ref_banded is test_resize.resize_ref.  test_resize compares u8 output only where its u8_eligible holds -- no axis ratio
    with a lowest-terms denominator below 5 (they put elements exactly on halves) and at most 30 taps per axis -- because the share
    of elements inside the rounding band grows with the tolerance, which grows with the tap count, whatever the picture holds: at
    586 taps the band is a seventh of every unit interval.  The same rule here: the pictures it admits are compared as u8 as well,
    and on those the reference alone stays inside BAND_CAP; the others are compared in two float formats, which have no band."""
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (37, 53, 3))
    for tw, th in ((7, 5), (53, 37), (90, 11)):
        for aa in (True, False):
            assert np.allclose(resize_ref_banded(img, tw, th, aa), trs.resize_ref(img, tw, th, aa), rtol=0, atol=1e-9), (tw, th, aa)
        assert max_taps(53, tw) == trs.max_taps(53, tw, True) and max_taps(37, th) == trs.max_taps(37, th, True)
    for n_in, n_out in ((1072, 224), (16, 224), (535, 7), (1, 7), (17, 224), (4096, 224), (224, 4096), (9, 9)):
        assert max_taps(n_in, n_out) == trs.max_taps(n_in, n_out, True), (n_in, n_out)
    assert max_taps(SIDE, 224) == 586 and 2 * trs.tolerance(586, 2) > 0.14
    bad, n = [], 0
    for layout in LAYOUTS:
        for c in derived_cases(layout):
            for t in RESIZE_TARGETS:
                if not u8_eligible(mjx, c, t):
                    continue
                n += 1
                tw, th = resize_target(c, t)
                plan = mjx.resize_plan(data_of(c), mjx.Resize(tw, th))
                data = data_of(c)
                src = oracle(data).rgb if plan["scale"] == 1 else scaled_ref.scaled_rgb(data, plan["scale"], oracle(data))
                ref = resize_ref_banded(src, tw, th, True)
                tol = trs.tolerance(plan["taps_x"], plan["taps_y"])
                band = int((np.rint(np.clip(ref - tol, 0, 255)) != np.rint(np.clip(ref + tol, 0, 255))).sum())
                if band > trs.BAND_CAP * ref.size:
                    bad.append((c.name, (tw, th), band, ref.size))
    assert bad == [] and n >= 8, (bad, n)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def ordinary(layout):
    return file_of(layout, *ORDINARY)


N_BATCHES = 3


def mixed_batch(k):
    """[(name, bytes)]: every third file of the family, narrow, wide and tall pictures of every layout side by side, and an ordinary
    333 x 217 picture of three layouts among them"""
    cs = [(c.name, data_of(c)) for c in family()[k::N_BATCHES]]
    for j, layout in enumerate(LAYOUTS[k::N_BATCHES]):
        cs.insert(3 + 7 * j, ("%s_%dx%d" % ((layout,) + ORDINARY), ordinary(layout)))
    return cs


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(N_BATCHES))
def test_standard_mixed_batches(mjx, gpu_ctx, k):
    """Every file of the family in three heterogeneous batches: T0 equals the oracle's bit for bit, RGB within TOL, no run left
    unconverged; and tile(3) of the first batch gives the same bytes three times."""
    cases = mixed_batch(k)
    assert len(cases) <= 40
    b, scans = tsl.decode_batch(mjx, gpu_ctx, [d for _, d in cases], keep_coefs=True)
    try:
        bad = [(cn, p) for i, (cn, d) in enumerate(cases) for p in [tsl.check_std(mjx, b, i, d)] if p]
        assert b.unconverged_runs() == 0
    finally:
        tsl.close_all(b, scans)
    assert bad == [], bad


@pytest.mark.gpu
def test_tiled_mixed_batch(mjx, gpu_ctx):
    cases = mixed_batch(1)
    n = len(cases)
    scans = [mjx.ParsedScan(d) for _, d in cases]
    b = mjx.Batch(gpu_ctx, scans)
    try:
        t = b.tile(3)
        try:
            t.decode()
            t.wait()
            assert [t.status(i) for i in range(3 * n)] == [mjx.OK] * (3 * n)
            assert t.unconverged_runs() == 0
            mine = list(range(n, 3 * n))
            mx, cnt = t.compare_rgb(mine, t, [i % n for i in mine])
            assert int(mx.max()) == 0 and int(cnt.sum()) == 0, [cases[i % n][0] for i, m in zip(mine, mx) if m]
            bad = [(cn, p) for i, (cn, d) in enumerate(cases) for p in [tsl.rgb_problem(t.rgb(i), oracle(d).rgb)] if p]
            assert bad == [], bad
        finally:
            t.close()
    finally:
        tsl.close_all(b, scans)


@pytest.mark.gpu
def test_front_doors_with_device_destuff(mjx, gpu_ctx):
    """One file per item through mjx_decode and through mjx_decode_batch with the device's de-stuffing."""
    cases = one_per_item()
    datas = [data_of(c) for c in cases]
    b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=True, keep_coefs=True)
    try:
        assert st == [mjx.OK] * len(datas), st
        bad = [(c.name, p) for i, (c, d) in enumerate(zip(cases, datas)) for p in [tsl.check_std(mjx, b, i, d)] if p]
        assert b.unconverged_runs() == 0
        batch_rgb = [b.rgb(i) for i in range(len(datas))]
    finally:
        b.close()
    assert bad == [], bad
    for c, d, want in zip(cases, datas, batch_rgb):
        img = mjx.Image()
        o = mjx._opts(device_destuff=True)
        assert mjx.lib().mjx_decode(d, len(d), ctypes.byref(o), ctypes.byref(img)) == mjx.OK, c.name
        try:
            got = np.ctypeslib.as_array(img.rgb, (img.height, img.width, 3)).copy()
        finally:
            mjx.lib().mjx_free_image(ctypes.byref(img))
        assert tsl.same(got, want), c.name


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("k", range(N_BATCHES))
def test_scaled(mjx, gpu_ctx, k, scale):
    """Every file of items 1 to 4 at scales 2, 4 and 8 against scaled_ref, with test_scaled_decode's comparison."""
    cases = mixed_batch(k)
    b, scans = tsl.decode_batch(mjx, gpu_ctx, [d for _, d in cases], scale=scale)
    bad = []
    try:
        for i, (cn, d) in enumerate(cases):
            w, h, _, _ = scaled_ref.jpeg_tables(d)
            inf = b.info(i)
            if (inf["width"], inf["height"]) != (-(-w // scale), -(-h // scale)) or b.status(i) != mjx.OK:
                bad.append((cn, "info or status", inf, b.status(i)))
                continue
            p = tsl.rgb_problem(b.rgb(i), scaled_ref.scaled_rgb(d, scale, oracle(d)))
            if p:
                bad.append((cn, p))
        assert b.unconverged_runs() == 0
    finally:
        tsl.close_all(b, scans)
    assert bad == [], bad


def rect_cases(layout):
    """the files whose rectangles are decoded: of 4:2:0 and 4:4:4 one per mcux of items 1 and 2 and the 16- and 17-pixel limits,
    of the other layouts everything they have"""
    fam = cases_of(layout)
    if layout not in FULL:
        return fam
    keep, seen = [], set()
    for c in fam:
        key = (c.item, c.mcux if c.item <= 2 else (c.w, c.h) if min(c.w, c.h) in (1, 17) else None)
        if key[1] is not None and key not in seen:
            seen.add(key)
            keep.append(c)
    return keep + [c for c in fam if c.item == 3][:2]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rectangles(mjx, gpu_ctx, layout):
    """The limit rectangles at scales 1 and 8: each result is byte for byte the crop of the same process's uncropped decode.  From
    plan_tiles: some rectangle of the layout skipped tiles, and some full-height column of a picture narrower than a tile could not
    skip any, because every tile wraps through every column."""
    bad, skipped, stuck = [], 0, 0
    for s in (1, 8):
        for c in rect_cases(layout):
            data = data_of(c)
            scan = mjx.ParsedScan(data)
            try:
                full = roi._full(mjx, gpu_ctx, data, s)
                rects = limit_rects(full.shape[1], full.shape[0], c.mw // s, c.mh // s)
                b = mjx.Batch(gpu_ctx, [scan] * len(rects), scale=s, rois=rects)
                try:
                    b.decode()
                    b.wait()
                    for i, r in enumerate(rects):
                        plan = scan.plan_tiles(roi=r, scale=s)
                        skipped += plan["tiles_read"] < plan["tiles_total"]
                        stuck += c.mcux < plan["tile_mcus"] and r[3] == full.shape[0] and r[2] == 1 and plan["tiles_read"] == plan["tiles_total"] > 2
                        if b.status(i) != mjx.OK:
                            bad.append((c.name, s, r, "status", b.status(i)))
                        elif not tsl.same(b.rgb(i), roi.crop(full, r)):
                            bad.append((c.name, s, r, "differs from the crop"))
                finally:
                    b.close()
            finally:
                scan.close()
    assert bad == [], bad[:10]
    assert skipped > 0 and stuck > 0, (skipped, stuck)


# ---- GPU: the DC family ------------------------------------------------------------------------------------------------------------------
def child_dc(job_path):
    """Child process: decodes the files of the job (keep_coefs) in one batch and writes every T0 and status."""
    import __graft_entry__ as ge
    mjx = ge.load_package()
    job = json.load(open(job_path))
    datas = [open(p, "rb").read() for p in job["paths"]]
    ctx = mjx.Context(0)
    b, scans = tsl.decode_batch(mjx, ctx, datas, keep_coefs=True)
    out = {}
    status = [b.status(i) for i in range(len(datas))]
    for i in range(len(datas)):
        if status[i] == mjx.OK:
            out["c%d" % i] = b.coefs(i)
    unconverged = b.unconverged_runs()
    tsl.close_all(b, scans)
    ctx.close()
    np.savez(job["out"], **out)
    print(json.dumps(dict(status=status, unconverged=unconverged)))


def run_dc_child(tmp_path, datas, env_set):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("dc_%d.jpg" % i)
        p.write_bytes(d)
        paths.append(str(p))
    job, out = tmp_path / "job.json", tmp_path / "out.npz"
    job.write_text(json.dumps(dict(paths=paths, out=str(out))))
    script = tmp_path / "child.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
                      "import test_geometry_limits as t\nt.child_dc(%r)\n" % (ROOT, ROOT, str(job)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with np.load(str(out)) as z:
        return {k: z[k] for k in z.files}, res


def dc_t0_problems(cases, coefs_of, status):
    bad = []
    for i, (bpm, k, r, rst) in enumerate(cases):
        if status[i] != 0:
            bad.append((bpm, 2048 * k + r, rst, "status", status[i]))
        elif not np.array_equal(coefs_of(i), dc_picture(bpm, k, r).blocks):
            got, want = coefs_of(i)[:, 0].astype(np.int64), dc_picture(bpm, k, r).blocks[:, 0].astype(np.int64)
            first = int(np.argmax(got != want)) if got.shape == want.shape else -1
            bad.append((bpm, 2048 * k + r, rst, "T0 differs from block", first, "MCU", first // bpm))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("bpm", DC_FAST + DC_GENERIC)
def test_dc_segments_t0_is_the_blocks_written(mjx, gpu_ctx, bpm):
    """nmcu on both sides of a segment boundary, without and with restart intervals of 1 and of 2049 MCUs: T0 is what was written."""
    cases = dc_cases([bpm])
    b, scans = tsl.decode_batch(mjx, gpu_ctx, [dc_file(*c) for c in cases], keep_coefs=True)
    try:
        bad = dc_t0_problems(cases, b.coefs, [b.status(i) for i in range(len(cases))])
        assert b.unconverged_runs() == 0
    finally:
        tsl.close_all(b, scans)
    assert bad == [], bad


@pytest.mark.gpu
@pytest.mark.parametrize("restart", DC_RESTARTS)
@pytest.mark.parametrize("kernels", ["fast", "generic"])
def test_dc_segments_in_two_passes(mjx, tmp_path, kernels, restart):
    """The same under MJX_DC_ONE_PASS=0 (k_dc_sums / k_dc_apply and their _t forms), in a child process."""
    cases = dc_cases(DC_FAST if kernels == "fast" else DC_GENERIC, (restart,))
    out, res = run_dc_child(tmp_path, [dc_file(*c) for c in cases], {"MJX_DC_ONE_PASS": "0"})
    assert res["unconverged"] == 0
    bad = dc_t0_problems(cases, lambda i: out["c%d" % i], res["status"])
    assert bad == [], bad


@pytest.mark.gpu
def test_dc_level_pictures_at_scale_8(mjx, gpu_ctx):
    """Levels -40 .. 300 on luminance only: the picture at scale 8 is the clamped level exactly (DC-only levels are exact: class 4 of
    test_stageb_arithmetic), for every blocks-per-MCU count on both sides of both segment boundaries."""
    cases = [(bpm, k, r, rst) for bpm in DC_FAST + DC_GENERIC for k, r in ((1, -1), (1, 1), (2, 0), (2, 9)) for rst in (0,)]
    cases += [(bpm, 1, 9, 2049) for bpm in DC_FAST + DC_GENERIC]
    got = tsl.gpu_pictures(mjx, gpu_ctx, [dc_file(b, k, r, rst, levels=True) for b, k, r, rst in cases], 8)
    bad = [c for c, g in zip(cases, got) if not tsl.same(g, dc_level_picture(dc_picture(c[0], c[1], c[2], levels=True)))]
    assert bad == [], bad


# ---- GPU: multi-scan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multiscan_twins_narrow_and_wide(mjx, gpu_ctx, tmp_path):
    """Twins of a 16-wide, a (T + 1)-MCU-wide and a 65535 x 16 source, 4:2:0 and the 12-block MCU, three scripts: the device's bytes
    for the twin are its bytes for the source at scales 1, 2 and 8, by default and with MJX_PLANAR_DIRECT=0.  Alone, a twin is read
    straight from its scans exactly where planar_ok admits it (test_multiscan_scripts.planar_direct): never in the 16-wide
    pictures, whose tiles span T MCU rows, and in the wide ones wherever the scans give at most four block rows per MCU."""
    srcs = twin_sources()
    cases = [(c, script, tw) for c in srcs for script, tw in zip(TWIN_SCRIPTS, twins_of(c.layout, c.w, c.h))]
    scales = (1, 2, 8)
    bad, ndirect, ngather_narrow = [], {}, 0
    want = {s: dict(zip([c.name for c in srcs], tsl.gpu_pictures(mjx, gpu_ctx, [data_of(c) for c in srcs], s))) for s in scales}
    for s in scales:
        got = tsl.gpu_pictures(mjx, gpu_ctx, [tw for _, _, tw in cases], s)
        bad += [(c.name, script, s, "mixed") for (c, script, _), g in zip(cases, got) if not tsl.same(g, want[s][c.name])]
        for c, script, tw in cases:
            b, scans = tsl.decode_batch(mjx, gpu_ctx, [tw], scale=s)
            try:
                g = b.rgb(0) if b.status(0) == mjx.OK else None
                direct = g is not None and not tsl.coefs_expand(mjx, b, 0)
            finally:
                tsl.close_all(b, scans)
            if direct != tms.planar_direct(name_for_rules(c.layout), c.w, script, s):
                bad.append((c.name, script, s, "direct path taken" if direct else "gather taken"))
            if c.mcux == 1:
                ngather_narrow += not direct
                if direct:
                    bad.append((c.name, script, s, "a picture one MCU wide read directly"))
            elif direct:
                ndirect[c.layout] = ndirect.get(c.layout, 0) + 1
            if not tsl.same(g, want[s][c.name]):
                bad.append((c.name, script, s, "alone", "direct" if direct else "gather"))
    out, status, _, expands = tsl.run_child(tmp_path, "gather", [tw for _, _, tw in cases], scales, {"MJX_PLANAR_DIRECT": "0"}, single=True)
    for s in scales:
        for i, (c, script, _) in enumerate(cases):
            for tag in ("all", "one"):
                key = "%d_%d_%s" % (i, s, tag)
                if not tsl.same(out.get(key), want[s][c.name]):
                    bad.append((c.name, script, s, "MJX_PLANAR_DIRECT=0", tag, status[key]))
            if not expands.get("%d_%d_one" % (i, s)):
                bad.append((c.name, script, s, "not gathered with MJX_PLANAR_DIRECT=0"))
    assert bad == [], bad[:12]
    assert ngather_narrow == 2 * len(TWIN_SCRIPTS) * len(scales) and all(ndirect.get(l, 0) > 0 for l in ("420", "Y22_Cb21_Cr12")), (ngather_narrow, ndirect)


# ---- GPU: REF_COMPAT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(N_BATCHES))
def test_ref_compat(mjx, gpu_ctx, k):
    """Every file the oracle decodes in the reference's layout is within TOL of it (T0 equal); every file it panics on gives
    MJX_ERR_REF_PANIC, and the pictures around it in the batch are unaffected."""
    cases = mixed_batch(k)
    names = {c.name: c for c in family()}
    b, scans = tsl.decode_batch(mjx, gpu_ctx, [d for _, d in cases], keep_coefs=True, layout=mjx.LAYOUT_REF_COMPAT)
    bad, npanic, nok = [], 0, 0
    try:
        for i, (cn, d) in enumerate(cases):
            rc, ref = oracle_ref(d)
            want = {ref_want(mjx, rc)}
            c = names.get(cn)
            if runs_past(c.layout if c else cn[:cn.rindex("_")], *((c.w, c.h) if c else ORDINARY)):
                rc, want = -1, {mjx.ERR_BAD_HUFFMAN, mjx.ERR_TRUNCATED} if scans[i].validate(layout=mjx.LAYOUT_REF_COMPAT) == mjx.OK else {mjx.ERR_REF_PANIC}
            npanic += rc == orc_mod.ERR_REF_PANIC
            if b.status(i) not in want:
                bad.append((cn, "status", b.status(i), want))
                continue
            if rc != orc_mod.OK:
                continue
            nok += 1
            if not np.array_equal(b.coefs(i), orc_mod.interleave(ref)):
                bad.append((cn, "T0"))
                continue
            p = tsl.rgb_problem(b.rgb(i), ref.rgb)
            if p:
                bad.append((cn, p))
    finally:
        tsl.close_all(b, scans)
    assert bad == [], bad
    assert npanic > 3 and nok > 3, (npanic, nok)


# ---- GPU: derived paths --------------------------------------------------------------------------------------------------------------------
def packed(mjx, ctx, datas, **kw):
    return tlo.packed_decode(mjx, ctx, datas, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_formats(mjx, gpu_ctx, layout):
    """Planar f32 with mean and std and interleaved f16 BGR are test_output_formats.expected of the packed decode, bit for bit; u8
    into caller-owned pitched memory likewise, with the guard bytes around and between the rows untouched."""
    cases = derived_cases(layout)
    datas = [data_of(c) for c in cases]
    want = packed(mjx, gpu_ctx, datas)
    assert all(isinstance(w, np.ndarray) for w in want), want
    for fmt_k in (trs.F32_PLANAR, F16_BGR):
        fmt = tof.make_format(mjx, fmt_k)
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, output=fmt)
        try:
            b.decode()
            b.wait()
            for i, c in enumerate(cases):
                assert b.status(i) == mjx.OK, (c.name, b.status(i))
                assert tof.same_bits(b.output(i), tof.expected(want[i], fmt)), (c.name, fmt_k)
        finally:
            tsl.close_all(b, scans)
    hip = tof._hip(mjx)
    guard, pad = 4096, 5
    for c, d, w in zip(cases, datas, want):
        rp = 3 * c.w + pad
        total = guard + c.h * rp + guard
        base = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(base), total) == 0
        try:
            assert hip.hipMemset(base, tof.SENTINEL, total) == 0 and hip.hipDeviceSynchronize() == 0
            fmt = mjx.Output("uint8", dst=[(base.value + guard, c.w, c.h, rp, 0)])
            b, st = mjx.decode_batch(gpu_ctx, [d], output=fmt)
            try:
                assert st == [mjx.OK] and b.status(0) == mjx.OK, (c.name, st)
                mem = np.empty(total, np.uint8)
                assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
            finally:
                b.close()
            rows = mem[guard:guard + c.h * rp].reshape(c.h, rp)
            assert np.array_equal(rows[:, :3 * c.w].reshape(c.h, c.w, 3), w), c.name
            assert np.all(rows[:, 3 * c.w:] == tof.SENTINEL) and np.all(mem[:guard] == tof.SENTINEL) and np.all(mem[guard + c.h * rp:] == tof.SENTINEL), c.name
        finally:
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipFree(base) == 0


@functools.lru_cache(maxsize=None)
def neutral_twin(layout, w, h):
    """test_luma_output.twin_of for a family file: the same luminance blocks, every chroma coefficient zero; a one-component file is
    its own twin"""
    data = file_of(layout, w, h)
    hv = hv_of(layout)
    if len(hv) == 1:
        return data
    dec = oracle(data)
    mw, mh = mcu_px(layout)
    mcux, mcuy = -(-w // mw), -(-h // mh)
    blocks = np.concatenate([(pc if c == 0 else np.zeros_like(pc)).reshape(mcux * mcuy, a * b, 64) for c, (pc, (a, b)) in enumerate(zip(dec.coefs, hv))],
                            axis=1).reshape(-1, 64)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    return jw.jpeg_from_blocks(blocks, hv, mcux, mcuy, [qt[tq] for _, _, tq in comps], jw.tables_from_jpeg(data), width=w, height=h)


def test_neutral_twins_keep_the_luminance_blocks():
    """the oracle reads the narrow file's twin as the file's luminance blocks and no chroma at all"""
    for layout in LAYOUTS:
        c = derived_cases(layout)[0]
        a, b = oracle(neutral_twin(c.layout, c.w, c.h)), oracle(data_of(c))
        assert np.array_equal(a.coefs[0], b.coefs[0]) and not any(co.any() for co in a.coefs[1:]), c.name


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_luminance_and_libjpeg_pixels(mjx, gpu_ctx, layout):
    """channels = 1 as test_luma_output.twin_problems compares it, at scales 1 and 8: the byte of the chroma-neutral twin's packed
    decode, which is grey, and at full size inside the interval float64 allows (interval_problem).  pixels = "libjpeg" inside
    libjpeg_ref's interval (test_libjpeg_pixels.interval_problem)."""
    cases = derived_cases(layout)
    datas = [data_of(c) for c in cases]
    twins = [neutral_twin(c.layout, c.w, c.h) for c in cases]
    bad = []
    for s in (1, 8):
        got = tlo.luma_decode(mjx, gpu_ctx, datas, scale=s)
        want = tlo.packed_decode(mjx, gpu_ctx, twins, scale=s)
        for c, d, g, t in zip(cases, datas, got, want):
            if not isinstance(t, np.ndarray) or not (np.array_equal(t[:, :, 0], t[:, :, 1]) and np.array_equal(t[:, :, 0], t[:, :, 2])):
                bad.append((c.name, s, "the twin's packed decode is not grey"))
            elif not tsl.same(g, t[:, :, 0]):
                bad.append((c.name, s, g if not isinstance(g, np.ndarray) else "%d bytes differ from the twin" % int((g != t[:, :, 0]).sum())))
            elif s == 1:
                p = tlo.interval_problem(g, d, s)
                if p:
                    bad.append((c.name, "luma", s, p))
    got = tlp.lj_decode(mjx, gpu_ctx, datas)
    bad += [(c.name, "libjpeg", p) for c, d, g in zip(cases, datas, got) for p in [tlp.interval_problem(g, d)] if p]
    assert bad == [], bad


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_orientation(mjx, gpu_ctx, layout):
    """Codes 2, 3, 6 and 8: the mapped bytes of the unturned decode; 6 and 8 turn 65535 x 16 into 16 x 65535."""
    cases = derived_cases(layout)
    datas = [data_of(c) for c in cases]
    want = packed(mjx, gpu_ctx, datas)
    for code in (2, 3, 6, 8):
        scans = [mjx.ParsedScan(d) for d in datas]
        b = mjx.Batch(gpu_ctx, scans, output=mjx.Output("uint8"), orient=mjx.Orient(exif=False, extra=code))
        try:
            b.decode()
            b.wait()
            for i, c in enumerate(cases):
                assert b.status(i) == mjx.OK and b.orientation(i) == code, (c.name, code, b.status(i))
                assert tsl.same(b.output(i), np.ascontiguousarray(tor.orient_np(code, want[i]))), (c.name, code)
        finally:
            tsl.close_all(b, scans)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_resize(mjx, gpu_ctx, layout):
    """To 224 x 224 (586 taps on one axis and 2 on the other for 65535 x 16) and to 7 x 65535 / 65535 x 7, planar f32 and, where
    test_resize's u8 rule admits the picture, packed u8 (else interleaved f16 BGR): test_resize.check_against, with
    test_resize.tolerance, on the rule applied to the device's own packed decode at the plan's scale; the band share under BAND_CAP."""
    cases = derived_cases(layout)
    bad, band, total = [], 0, 0
    for c in cases:
        data = data_of(c)
        scan = mjx.ParsedScan(data)
        try:
            for t in RESIZE_TARGETS:
                tw, th = resize_target(c, t)
                rs = mjx.Resize(tw, th)
                plan = scan.resize_plan(rs)
                src = roi._full(mjx, gpu_ctx, data, plan["scale"])
                ref = resize_ref_banded(src, tw, th, True)
                second = mjx.Output("uint8") if u8_eligible(mjx, c, t) else tof.make_format(mjx, F16_BGR)
                for fmt in (tof.make_format(mjx, trs.F32_PLANAR), second):
                    b = mjx.Batch(gpu_ctx, [scan], output=fmt, resize=rs)
                    try:
                        b.decode()
                        b.wait()
                        if b.status(0) != mjx.OK or b.scale(0) != plan["scale"]:
                            bad.append((c.name, (tw, th), "status or scale", b.status(0), b.scale(0)))
                            continue
                        fail, nb, nt = trs.check_against(b.output(0), ref, fmt, trs.tolerance(plan["taps_x"], plan["taps_y"]))
                    finally:
                        b.close()
                    band, total = band + nb, total + nt
                    if fail:
                        bad.append((c.name, (tw, th), fmt.dtype, fail))
        finally:
            scan.close()
    assert bad == [], bad
    assert band <= trs.BAND_CAP * total, (band, total)

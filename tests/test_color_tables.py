"""Four-component decode on its own tables, sums and arithmetic (mjx_opts.color = MJX_COLOR_FILE).

tests/test_color_decode.py composes RGB, CMYK and YCCK pictures with everything behind stage B, with K on component 0's tables and
the device's own decode of twins as the expectation.  Here the fourth component has tables of its own -- four DQTs that differ at
every position (one of them 16-bit, K's a factor of two or more from component 0's), four Huffman pairs on crossed slots -- and the
expectation is independent of the device: the blocks written for T0, and for the pixels scaled_ref.model_interval, the float64
picture moved by K = 64 half-ulps per component (tests/test_stageb_arithmetic.py's K) and carried through mjx_ink_mul, which is
non-decreasing in both arguments.  The twins' composition is asserted beside it.

CPU tests: the writer pinned by Pillow and by the serial decode; the planner's table bases; the 0x7fff cap of a picture's decode-table
set with four pairs; planted errors in the reference; the share of bytes the interval leaves open; the K the float32 restatement of
stage B needs on the new classes.  GPU tests: four tables through every form; the arithmetic classes with a fourth component; the
four-sum DC kernels on both sides of every 2048-MCU segment boundary and over three workgroups of restart intervals; damaged
four-component scans against the serial decode.

Numbers the tests print (measured; DESIGN.md s23 "Checks" has the same):
  largest four-pair table set       31 584 bytes (sub7 on all four slots; 30 064 with the shape list rotated, from sub5); the cap is 32 767
  a set over the cap                34 880 bytes ("deep": codes of 10 .. 16 bits under as many 9-bit prefixes as a table of 256 symbols
                                    reaches) -- refused with MJX_ERR_BAD_HUFFMAN
  four Annex K-style pairs          25 792 bytes; four pairs optimised for the picture: 26 768 (1 x 1 x 4), 26 256 (y22_k22)
  K the float32 restatement needs   3.34 (sat_sparse_q65535, 1 x 1 x 4 CMYK, scale 1, component 2); 4 x 3.34 = 13.4 <= 64
  ambiguous share per picture       at most 0.0184 (class 5 at 1/2; the four-table files 0.0140); the table is in test_ambiguous_share_per_case
  planted errors                    each of the six leaves the interval on every pixel of its best case (share 1.000)
"""
import ctypes
import functools
import hashlib
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import colorwriter as cw
import damaged_ref as dr
import jpegwriter as jw
import scaled_ref
import test_color_decode as tcd
import test_geometry_limits as tgl
import test_huffman_tables as tht
import test_output_formats as of
import test_stageb_arithmetic as tsa
from test_stageb_arithmetic import K, AMBIGUOUS_CAP

ROOT = tcd.ROOT
LAYOUTS4, LAYOUTS3, HEAD, MODEL = tcd.LAYOUTS4, tcd.LAYOUTS3, tcd.HEAD, tcd.MODEL
F64 = np.float64
COLOR_FILE = 1                                        # MJX_COLOR_FILE (include/mjx.h)
ERR_BAD_HUFFMAN = 4                                   # MJX_ERR_BAD_HUFFMAN: the status of a picture whose decode-table set is over the cap
CAP = 0x7fff
CROSSED = [(3, 0), (1, 2), (2, 1), (0, 3)]            # (DC slot, AC slot) per component


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def dqts(i=0):
    """{slot: table} for picture number i of a batch: four tables that differ from one another at every position, slot 3 (K's) a
    factor of two or more above slot 0's, slot 2 with one 16-bit entry (so that it is written with 16-bit precision); the tables of
    two pictures differ at every position as well.  Every entry is odd, so that a block's DC alone can take its samples off the
    whole numbers (off_the_integers)."""
    k = np.arange(64)
    q0 = 3 + 10 * i + 2 * (k % 3)                     # 3, 5, 7; 13, 15, 17; ...; K's: 7, 11, 15; 27, 31, 35; ...
    q2 = 171 + 10 * i + 2 * (k % 4)
    q2[63] = 257 + 2 * i
    return {0: q0, 3: 2 * q0 + 1, 1: 111 + 10 * i + 2 * (k % 5), 2: q2}


@functools.lru_cache(maxsize=None)
def four_pairs():
    """{(class, slot): table}: four distinct DC and four distinct AC tables -- the Annex K pairs on slots 0 and 1, two shapes of
    jpegwriter.huffman_shapes on slots 2 and 3 (second-level tables of three index bits; a random length profile)"""
    ak = jw._annex_k_tables()
    dc, ac = jw.huffman_shapes(jw.DC_SYMBOLS, seed=40), jw.huffman_shapes(jw.AC_SYMBOLS, seed=41)
    t = {(cls, s): ak[(cls, s)] for s in (0, 1) for cls in (0, 1)}
    t.update({(0, 2): dc["sub3"], (1, 2): ac["sub3"], (0, 3): dc["random5"], (1, 3): ac["random5"]})
    assert len({repr(t[(0, s)]) for s in range(4)}) == 4 and len({repr(t[(1, s)]) for s in range(4)}) == 4
    return t


def make(model, hv, w, h, i=0, **kw):
    """color_jpeg's content on four tables and crossed slots, its blocks taken off the whole samples (off_the_integers) and written
    again by color_from_blocks: what the writer quantised is natural content, whose DC-only blocks are whole for one in eight"""
    nc = len(hv)
    cf = cw.color_jpeg(w, h, hv, head=HEAD[model], tq=list(range(nc)), huff=CROSSED[:nc], qts=dqts(i), tables=four_pairs(), **kw)
    blocks = off_the_integers(cf.blocks, cf.qts, 1023, None)
    return cw.color_from_blocks(blocks, cf.hv, cf.mcux, cf.mcuy, cf.qt_slots, cf.tq, cf.tables, cf.huff, head=cf.head, width=w, height=h,
                                restart=cf.restart or None)


def undecided(cf, model, scale):
    """the share of the picture's bytes with lo != hi, on the reference alone (model "grey": component 0 as a picture of its own)"""
    if model == "grey":
        lo, hi = scaled_ref.byte_interval(*scaled_ref.component_samples(grey_view(cf), 0, scale), K)
    else:
        lo, hi = scaled_ref.model_interval(cf, model, scale, K)
    return float((lo != hi).mean())


def make_decided(model, hv, w, h, seed, **kw):
    """make() with the first of seed, seed + 1000, ... whose picture meets the condition on the inputs at every scale: at most
    AMBIGUOUS_CAP of its bytes undecided between two levels.  A sample falls within K half-ulps of a whole number by chance for
    about one byte in 300, and a one-MCU picture at 1/2 has 48 to 192 bytes: the choice is made on float64 alone, as the
    amplitudes of the class pictures are."""
    for s in range(seed, seed + 8000, 1000):
        cf = make("cmyk" if model == "grey" else model, hv, w, h, seed=s, **kw)
        if all(undecided(cf, model, scale) <= AMBIGUOUS_CAP for scale in (1, 2, 4, 8)):
            return cf
    raise AssertionError(("no seed meets the cap", model, hv, w, h, seed))


@functools.lru_cache(maxsize=None)
def table_cases():
    """[(tag, model, ColorFile)]: the five four-component layouts as CMYK and as YCCK and RGB at 4:4:4 and 4:2:0, one MCU and 37 x 29,
    every component on a DQT and on Huffman slots of its own"""
    out = []
    for name, hv in list(LAYOUTS4.items()) + list(LAYOUTS3.items()):
        hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
        for k, (w, h) in enumerate(((8 * hmax, 8 * vmax), (37, 29))):
            for model in (("cmyk", "ycck") if len(hv) == 4 else ("rgb",)):
                out.append(("%s %s %dx%d" % (name, model, w, h), model, make_decided(model, hv, w, h, 111 + k, quality=85, noise=6.0)))
    return out


def grey_view(cf, c=0):
    """a stand-in ColorFile of the one-component picture that carries component c's blocks, for scaled_ref.component_samples"""
    h, v = cf.hv[c]
    raster = cf.blocks[c].reshape(cf.mcuy, cf.mcux, v, h, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
    g = types.SimpleNamespace(hv=[(1, 1)], blocks=[raster], qts=[cf.qts[c]], width=cf.mcux * h * 8, height=cf.mcuy * v * 8, mcux=cf.mcux * h,
                              mcuy=cf.mcuy * v, hmax=1, vmax=1)
    return g


def grey_of(cf, c=0):
    """(the one-component file of component c, its stand-in)"""
    return cw.component_twin(cf, c), grey_view(cf, c)


@functools.lru_cache(maxsize=None)
def mixed_cases():
    """three-component, four-component, grey, four-component, three-component -- every picture with tables of its own (dqts(i))"""
    a = make_decided("rgb", LAYOUTS3["420"], 37, 29, 121, i=0, quality=85, noise=6.0)
    b = make_decided("cmyk", LAYOUTS4["y22_k22"], 37, 29, 122, i=1, quality=85, noise=6.0)
    g = make_decided("grey", LAYOUTS4["1x1x4"], 40, 24, 123, i=2, quality=85, noise=6.0)
    d = make_decided("ycck", LAYOUTS4["h2_k2"], 37, 29, 124, i=3, quality=85, noise=6.0)
    e = make_decided("rgb", LAYOUTS3["444"], 37, 29, 125, i=4, quality=85, noise=6.0)
    return [("rgb", a), ("cmyk", b), ("grey", g), ("ycck", d), ("rgb", e)]


@functools.lru_cache(maxsize=None)
def interval_of(key, scale):
    """(lo, hi) of a picture named by key = (family, index): computed once, read-only"""
    fam, i = key
    if fam == "table":
        _, model, cf = table_cases()[i]
    elif fam == "mixed":
        model, cf = mixed_cases()[i]
        if model == "grey":
            lo, hi = scaled_ref.byte_interval(*scaled_ref.component_samples(grey_view(cf), 0, scale), K)
            lo, hi = np.repeat(lo[:, :, None], 3, 2), np.repeat(hi[:, :, None], 3, 2)
            lo.setflags(write=False); hi.setflags(write=False)
            return lo, hi
    else:
        model, cf = class_picture(*i).model, class_picture(*i)
    lo, hi = scaled_ref.model_interval(cf, model, scale, K)
    lo.setflags(write=False); hi.setflags(write=False)
    return lo, hi


def ambiguous(key, scale):
    lo, hi = interval_of(key, scale)
    return float((lo != hi).mean())


# ---- the arithmetic classes with a fourth component -----------------------------------------------------------------------------------
COMBOS = [("1x1x4", "cmyk"), ("y22_k22", "cmyk"), ("h2_k2", "ycck")]
CW, CH = 189, 131                                    # 24 x 17 MCUs of 8 x 8 (12 x 9 of 16 x 16), the last column and row clipped
GEN_VARIANTS = [v for v in tsa.VARIANTS if tsa.CLASS_OF[v] in (1, 2, 3, 6) or v.startswith("sat_sparse") or v.startswith("sat_dense")]
OWN_VARIANTS = ["exact4", "sat_k"]
CLASS4 = {**{v: tsa.CLASS_OF[v] for v in GEN_VARIANTS}, "exact4": 4, "sat_k": 5, "sat_chroma": 5}
VARIANTS4 = GEN_VARIANTS + OWN_VARIANTS


def variants_of(model):
    """sat_chroma -- mid luminance under a grid of far chroma, here under a mid K -- is a YCCK picture's business: as CMYK its
    components are three inks, which sat_k already takes out of range one by one"""
    return VARIANTS4 + (["sat_chroma"] if model == "ycck" else [])


def _level(n, stride, off):
    return tsa.EXACT_LEVELS[(stride * n + off) % len(tsa.EXACT_LEVELS)]


def _gen_exact4(per_mcu, mcus):
    """class 4: DC-only levels -40 .. 300 on component 0 and on K independently (strides 7 and 13 through the 341 levels), quantiser 8
    on both; components 1 and 2 are zero -- M = Y = 128 of a CMYK file, no chroma of a YCCK one"""
    out = [np.zeros((mcus * kc, 64), np.int64) for kc in per_mcu]
    out[0][:, 0] = _level(np.arange(mcus * per_mcu[0]), 7, 0) - 128
    out[3][:, 0] = _level(np.arange(mcus * per_mcu[3]), 13, 5) - 128
    return out, [np.full(64, 8), np.full(64, 3), np.full(64, 5), np.full(64, 8)]


def _gen_sat_k(per_mcu, mcus, rng):
    """class 5: in even MCUs K on a grid of 17 DC levels from far below 0 to far above 255 under mid inks, in odd MCUs the three other
    components on that grid (each at a stride of its own) under a mid K; sparse small AC on top"""
    grid = np.linspace(-1023, 1023, 17).astype(np.int64)
    out = []
    for c, kc in enumerate(per_mcu):
        n = np.arange(mcus * kc)
        even = (n // kc) % 2 == 0
        blk = np.where(rng.random((mcus * kc, 64)) < 0.05, rng.integers(-6, 7, (mcus * kc, 64)), 0)
        mid = rng.integers(-100, 101, mcus * kc)
        far = grid[((n // 2) * (1 + 2 * (c % 3)) + 5 * c) % 17]                    # (strides 1, 3, 5: the components walk the grid apart)
        blk[:, 0] = np.where(even, far, mid) if c == 3 else np.where(even, mid, far)
        out.append(blk)
    return out, [np.full(64, 7), np.full(64, 3), np.full(64, 5), np.full(64, 9)]        # (odd: off_the_integers needs no more than the DC)


def off_the_integers(per_comp, qts, top, max_diff):
    """What _in_range_amp does for one coefficient, for whole blocks: a component that leaves as a byte of its own has, at 1/8, the
    sample D / 8 (D = DC q) and, at 1/4, the four samples (D +- x +- y +- z) / 8 over the dequantised coefficients of the 2 x 2 corner
    -- rational numbers, whole for one block in eight, where trunc(w - delta) and trunc(w + delta) differ by construction.  The DC of
    such a block moves to the nearest value for which none of them is whole (a corner that is all zero is exactly 128 in any
    arithmetic and stays).  |DC| stays within `top` and, where max_diff is given, the differences between a component's successive
    blocks within it (the DC table's largest size): a block whose move would break that keeps its DC."""
    out = []
    for blk, q in zip(per_comp, qts):
        blk, q = np.array(blk, np.int64), np.asarray(q, np.int64)
        x, y, z, dc = blk[:, 1] * q[1], blk[:, 2] * q[2], blk[:, 4] * q[4], blk[:, 0].copy()       # zig-zag 1, 2, 4: (0,1), (1,0), (1,1)
        empty = (x == 0) & (y == 0) & (z == 0)
        done, new = np.zeros(len(blk), bool), dc.copy()
        for off in [0] + [s * k for k in range(1, 8) for s in (1, -1)]:
            cand = dc + off
            d = cand * q[0]
            ok = ((d % 8 != 0) | ((d == 0) & (off == 0))) & (np.abs(cand) <= top)
            corner = np.ones(len(blk), bool)
            for sx in (1, -1):
                for sy in (1, -1):
                    for sz in (1, -1):
                        corner &= (d + sx * x + sy * y + sz * z) % 8 != 0
            take = ok & (corner | (empty & (d == 0))) & ~done
            new[take] = cand[take]
            done |= take
        assert done.all()
        while max_diff is not None:
            bad = np.abs(np.diff(np.concatenate([[0], new]))) > max_diff
            if not bad.any():
                break
            bad[:-1] |= bad[1:]
            new[bad] = dc[bad]
        blk[:, 0] = new
        out.append(blk)
    return out


@functools.lru_cache(maxsize=None)
def class_picture(variant, lname, model):
    """a ColorFile of CW x CH with .model, .variant, .cls, .order16 (what b.coefs must return)"""
    hv = LAYOUTS4[lname]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-CW // (8 * hmax)), -(-CH // (8 * vmax))
    per_mcu = [h * v for h, v in hv]
    huff = "annex_k"
    if variant == "exact4":
        per_comp, qts = _gen_exact4(per_mcu, mcux * mcuy)
    elif variant == "sat_k":
        per_comp, qts = _gen_sat_k(per_mcu, mcux * mcuy, np.random.default_rng([5, mcux * mcuy, len(lname)]))
    elif variant == "sat_chroma":
        per_comp, qts, _, huff = tsa._generate(variant, per_mcu[:3], mcux * mcuy)
        rng = np.random.default_rng([6, mcux * mcuy, len(lname)])
        k = np.where(rng.random((mcux * mcuy * per_mcu[3], 64)) < 0.05, rng.integers(-6, 7, (mcux * mcuy * per_mcu[3], 64)), 0)
        k[:, 0] = rng.integers(-100, 101, len(k))                                    # a mid K: levels 15 .. 241 at q = 9
        per_comp, qts = list(per_comp) + [k], list(qts) + [np.full(64, 9)]
    else:
        per_comp, qts, _, huff = tsa._generate(variant, per_mcu, mcux * mcuy)
    assert len(qts) == 4
    if variant == "sat_chroma":                     # (Cb's quantiser is 4: chroma is no byte of its own in a YCCK picture, and stays)
        fixed = off_the_integers([per_comp[0], per_comp[3]], [qts[0], qts[3]], 1023, None)
        per_comp = [fixed[0], per_comp[1], per_comp[2], fixed[1]]
    elif variant != "exact4":
        over = variant.startswith("over")
        per_comp = off_the_integers(per_comp, qts, 2047 if variant == "over_q1" else 1023, 2047 if over else None)
    if huff == "annex_k":
        ak = jw._annex_k_tables()
        tables, slots = {(cls, s): ak[(cls, s)] for s in (0, 1) for cls in (0, 1)}, [(0, 0), (1, 1), (1, 1), (0, 0)]
    else:
        tables, slots = {(0, 0): jw.small_dc_table(11), (1, 0): jw.full_ac_table()}, [(0, 0)] * 4
    cf = cw.color_from_blocks(per_comp, hv, mcux, mcuy, {c: q for c, q in enumerate(qts)}, [0, 1, 2, 3], tables, slots, head=HEAD[model],
                              width=CW, height=CH)
    cf.model, cf.variant, cf.cls, cf.layout = model, variant, CLASS4[variant], lname
    cf.order16 = cf.order.astype(np.int16)
    assert np.array_equal(cf.order16, cf.order)
    return cf


def class_keys():
    return [("class", (v, l, m)) for l, m in COMBOS for v in variants_of(m)]


def exact4_want(cf, scale):
    """class 4 by integer arithmetic alone: mul(255 - clamp(l_Y) | clamp(l_C), clamp(l_K)) in the first channel, 128 in the ink's
    place of the others"""
    n = 8 // scale
    ow, oh = -(-cf.width // scale), -(-cf.height // scale)
    pl = []
    for c in (0, 3):
        h, v = cf.hv[c]
        lev = np.clip(cf.blocks[c][:, 0] + 128, 0, 255).reshape(cf.mcuy, cf.mcux, v, h).transpose(0, 2, 1, 3).reshape(cf.mcuy * v, cf.mcux * h)
        pl.append(cw.replicate(np.repeat(np.repeat(lev, n, 0), n, 1), h, v, cf.hmax, cf.vmax, ow, oh).astype(np.uint8))
    c0, k = pl
    if cf.model == "ycck":
        return np.stack([cw.ink_mul(255 - c0, k)] * 3, axis=2)
    mid = np.full_like(c0, 128)
    return np.stack([cw.ink_mul(c0, k), cw.ink_mul(mid, k), cw.ink_mul(mid, k)], axis=2)


# ---- CPU: the writer --------------------------------------------------------------------------------------------------------------------
def test_default_arguments_write_the_bytes_they_wrote():
    """color_jpeg without the new arguments writes what it wrote before they existed (hashes taken from the earlier writer), its
    ColorFile says slot = [0, 1, 1, 0] as before, and the new arguments spelt out as the defaults give the same file."""
    a = cw.color_jpeg(37, 29, LAYOUTS4["1x1x4"], seed=11, quality=85, noise=6.0)
    b = cw.color_jpeg(37, 29, LAYOUTS4["h2_k2"], seed=5, restart=3, k_swing=90.0, head=[cw.app14(2)])
    c = cw.color_jpeg(37, 29, LAYOUTS3["420"], seed=11, quality=85, noise=6.0)
    assert hashlib.sha256(a.data).hexdigest() == "af38d6414534bda743d5ea0aa7803f49e3082a4aaedd0ac65392f44f50489121"
    assert hashlib.sha256(b.data).hexdigest() == "3d14d6afee4882ee59c2ed640879af08c14074400056d23dc2e607bae82f7bc3"
    assert hashlib.sha256(c.data).hexdigest() == "22905680282d4ebf18b2f212c3241772ddfa73934ef6419a0dabc7f7c65187e3"
    assert a.slot == [0, 1, 1, 0] and c.slot == [0, 1, 1]
    ak = jw._annex_k_tables()
    same = cw.color_jpeg(37, 29, LAYOUTS4["1x1x4"], seed=11, quality=85, noise=6.0, tq=[0, 1, 1, 0], huff=[(0, 0), (1, 1), (1, 1), (0, 0)],
                         qts={0: jw.quality_table(jw.ANNEX_K_LUMA, 85), 1: jw.quality_table(jw.ANNEX_K_CHROMA, 85)},
                         tables={(cls, s): ak[(cls, s)] for s in (0, 1) for cls in (0, 1)})
    assert same.data == a.data
    again = cw.color_from_blocks(a.blocks, a.hv, a.mcux, a.mcuy, a.qt_slots, a.tq, a.tables, a.huff, width=37, height=29)
    assert again.data == a.data


def test_the_tables_are_what_the_tests_say():
    for i in range(5):
        q = dqts(i)
        assert all(np.all(q[a] != q[b]) for a in range(4) for b in range(a)) and np.all(q[3] >= 2 * q[0])
        assert max(q[2]) > 255 and all(max(q[s]) <= 255 for s in (0, 1, 3))
        for j in range(i):
            assert all(np.all(q[s] != dqts(j)[t]) for s in range(4) for t in range(4)), (i, j)
    for _, model, cf in table_cases():
        w, h, comps, qt = scaled_ref.jpeg_tables(cf.data)
        assert [c[2] for c in comps] == list(range(len(cf.hv))) and all(np.array_equal(qt[s], cf.qts[s]) for s in range(len(cf.hv)))
        pic = dr.Picture(cf.data)
        assert [(td, ta) for _, td, ta in dict.fromkeys(pic.blocks_of_mcu)] == CROSSED[:len(cf.hv)]
        assert cf.data.count(b"\xff\xdb\x00\x83\x12") == 1                       # one DQT with 16-bit entries, on slot 2


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_grey(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def test_pillow_decodes_the_four_table_files_within_the_twins_differences(mjx):
    """The rule of test_color_decode.test_against_pillow_within_the_twins_own_differences with the float64 reference in the device's
    place: d_c = the largest difference between Pillow's decode of component c's one-component twin and the reference's byte
    (model_bytes of an "rgb" stand-in: trunc(sample + 128)), u_c = what libjpeg's triangle upsampling adds where the component is
    subsampled (measured on Pillow's own planes), and the picture may differ from Pillow's by max_c (d_c + u_c) + d_K + u_K + 1; for
    YCCK d3 is measured on the three-component twin, which carries the chroma upsampling.  Pillow reads a 16-bit DQT, four DQTs and
    Huffman slots 2 and 3 in a baseline frame without complaint."""
    worst = []
    for tag, model, cf in table_cases():
        ncomp = len(cf.hv)
        d, u = [], []
        for c in range(ncomp):
            data, g = grey_of(cf, c)
            theirs = pil_grey(data)
            mine = scaled_ref.to_u8(scaled_ref.component_samples(g, 0, 1)[0] + 128.0)
            d.append(int(np.abs(mine.astype(int) - theirs.astype(int)).max()))
            h, v = cf.hv[c]
            rh, rv = cf.hmax // h, cf.vmax // v
            if rh == 1 and rv == 1:
                u.append(0)
            else:
                fancy = mjx.upsample_luma_host(theirs, rh, rv, (0, 0, cf.width, cf.height))
                u.append(int(np.abs(fancy.astype(int) - cw.replicate(theirs, h, v, cf.hmax, cf.vmax, cf.width, cf.height).astype(int)).max()))
        want = scaled_ref.model_bytes(cf, model, 1)
        if model == "ycck":
            data3, dec3 = scaled_ref.ycc_part(cf)
            d3 = int(np.abs(scaled_ref.to_u8(scaled_ref.rgb_f64(data3, 1, dec3)).astype(int) - pil_rgb(cw.with_head(data3, cw.app0())).astype(int)).max())
        else:
            d3 = max(dc + uc for dc, uc in zip(d[:3], u[:3]))
        bound = d3 + (d[3] + u[3] + 1 if ncomp == 4 else 0)
        diff = int(np.abs(want.astype(int) - pil_rgb(cf.data).astype(int)).max())
        worst.append((tag, d, u, d3, diff, bound))
        assert diff <= bound, (tag, d, u, d3, diff, bound)
        assert max(d) <= 2, (tag, d)                                           # (libjpeg's integer inverse DCT: a level or two)
    for row in worst:
        print("against Pillow: %s d = %s, u = %s, d3 = %d, picture = %d (bound %d)" % row)


def serial_problem(cf):
    r = dr.decode(dr.Picture(cf.data))
    if r.verdict != dr.OK or not r.complete:
        return r.verdict
    return None if np.array_equal(r.t0, cf.order.astype(np.int16)) else "T0"


def test_the_serial_decode_reads_the_new_files():
    """damaged_ref.decode -- one bit reader, none of the project's tables -- gives OK and the blocks written for the four-table files,
    the mixed batch's, every class picture on every layout and the damaged family's sources.  (The files of the table-set cap are
    decoded where they are built, test_table_set_cap_with_four_pairs; the DC family below.)"""
    files = [cf for _, _, cf in table_cases()] + [cf for _, cf in mixed_cases()]
    files += [class_picture(*key) for _, key in class_keys()] + [cf for _, cf in damaged_sources()]
    bad = [(getattr(cf, "variant", None), cf.hv, p) for cf in files for p in [serial_problem(cf)] if p]
    assert bad == [], bad


@pytest.mark.parametrize("lname", list(LAYOUTS4))
def test_the_serial_decode_reads_the_dc_family(lname):
    """... and for every member of the DC family -- every MCU count on both sides of the segment boundaries, every restart interval --
    and the two pictures of 600 and 700 restart intervals."""
    files = [dc4_file(lname, k, r, rst) for k, r in DC_COUNTS for rst in DC_RESTARTS]
    files += [f for f in (dc4_file("y22_k11", 0, 1800, 3), dc4_file("1x1x4", 0, 700, 1)) if f.hv == LAYOUTS4[lname]]
    bad = [(cf.mcux * cf.mcuy, cf.restart, p) for cf in files for p in [serial_problem(cf)] if p]
    assert bad == [], bad


# ---- CPU: the planner -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul_lib(mjx):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libhuff_emul.so"))
    lib.emul_table_set_color.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    lib.emul_table_set.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.emul_plan_parts_color.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.emul_decode_coefs_sub_color.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
                                                ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.emul_single_decode_cp_color.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                                ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def table_set(lib, data):
    """-> (status, bytes of the larger of the picture's two table sets, [(DC base, AC base)] per block of the MCU)"""
    out = np.zeros(16, np.uint32)
    rc = lib.emul_table_set_color(data, len(data), out.ctypes.data, COLOR_FILE)
    tabs = [int(x) for x in out[3:3 + int(out[2])]]
    return rc, 4 * int(max(out[0], out[1])), [(t & 0xffff, t >> 16) for t in tabs]


def plan_parts(lib, data):
    out = np.zeros((8, 8), np.int32)
    n = lib.emul_plan_parts_color(data, len(data), out.ctypes.data, 8, COLOR_FILE)
    return out[:max(n, 0)], n


def test_the_emulator_entry_points_keep_their_answers(emul_lib):
    """Without the colour option the entry points refuse a four-component file as before, and a three-component file gets the same
    table set from emul_table_set and from its twin with either option."""
    cf4, cf3 = table_cases()[2][2], make("rgb", LAYOUTS3["420"], 37, 29, quality=85, seed=1)
    out = np.zeros(16, np.uint32)
    assert emul_lib.emul_table_set(cf4.data, len(cf4.data), out.ctypes.data) == 7            # MJX_ERR_UNSUPPORTED_FORMAT
    a, b, c = np.zeros(16, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    plain = cw.strip_app14(cf3.data)
    assert emul_lib.emul_table_set(plain, len(plain), a.ctypes.data) == 0
    assert emul_lib.emul_table_set_color(plain, len(plain), b.ctypes.data, 0) == 0 and emul_lib.emul_table_set_color(plain, len(plain), c.ctypes.data, 1) == 0
    assert np.array_equal(a, b) and np.array_equal(a, c) and a[2] == 6


def test_planner_gives_every_pair_its_own_tables(emul_lib):
    """Four distinct pairs are four distinct DC and four distinct AC decode-table bases, K's entry differs from every other
    component's in both halves, and the block-in-MCU period is the whole MCU; slots that repeat a table share it (2 and 2 for the
    default [0, 1, 1, 0]), and a slot that holds a copy of another slot's table shares it too."""
    for tag, model, cf in table_cases():
        if len(cf.hv) != 4:
            continue
        rc, size, tabs = table_set(emul_lib, cf.data)
        assert rc == 0 and len(tabs) == cf.bpm, (tag, rc)
        comp_of_block = [c for c, (h, v) in enumerate(cf.hv) for _ in range(h * v)]
        per_comp = {}
        for c, t in zip(comp_of_block, tabs):
            assert per_comp.setdefault(c, t) == t, tag                              # a component's blocks share its entry
        assert len({t[0] for t in per_comp.values()}) == 4 and len({t[1] for t in per_comp.values()}) == 4, (tag, per_comp)
        assert all(per_comp[3][0] != per_comp[c][0] and per_comp[3][1] != per_comp[c][1] for c in range(3)), (tag, per_comp)
        parts, n = plan_parts(emul_lib, cf.data)
        assert n == 1 and parts[0][2] == 4 and parts[0][3] == cf.bpm and parts[0][4] == cf.bpm and parts[0][7] == 0, (tag, parts)
    for lname, hv in LAYOUTS4.items():
        cf = cw.color_jpeg(37, 29, hv, head=HEAD["cmyk"], seed=7)
        rc, _, tabs = table_set(emul_lib, cf.data)
        assert rc == 0 and len({t[0] for t in tabs}) == 2 and len({t[1] for t in tabs}) == 2, lname
        assert tabs[0] == tabs[-1] and tabs[0] != tabs[cf.hv[0][0] * cf.hv[0][1]], lname          # K on component 0's, not on component 1's
        parts, n = plan_parts(emul_lib, cf.data)
        # (1 x 1 x 4 on [0, 1, 1, 0]: the table sequence A B B A has no shorter period; it would with [0, 1, 0, 1])
        assert n == 1 and parts[0][4] == cf.bpm, (lname, parts)
    t = four_pairs()
    copy = {(0, 0): t[(0, 0)], (1, 0): t[(1, 0)], (0, 1): t[(0, 1)], (1, 1): t[(1, 1)], (0, 2): t[(0, 0)], (1, 2): t[(1, 1)]}
    cf = cw.color_jpeg(37, 29, LAYOUTS4["1x1x4"], head=HEAD["cmyk"], seed=7, huff=[(0, 0), (1, 1), (2, 2), (2, 0)], tables=copy)
    rc, _, tabs = table_set(emul_lib, cf.data)
    assert rc == 0 and tabs[2] == (tabs[0][0], tabs[1][1]) and tabs[3] == tabs[0], tabs
    ab = cw.color_jpeg(37, 29, LAYOUTS4["1x1x4"], head=HEAD["cmyk"], seed=7, huff=[(0, 0), (1, 1), (0, 0), (1, 1)])
    assert plan_parts(emul_lib, ab.data)[0][0][4] == 2                               # A B A B: the period is two blocks


# ---- CPU: the table-set cap with four pairs ----------------------------------------------------------------------------------------------
CAP_LAYOUTS = ["1x1x4", "y22_k22"]


@functools.lru_cache(maxsize=None)
def cap_source(lname):
    return cw.color_jpeg(120, 88, LAYOUTS4[lname], head=HEAD["cmyk"], quality=90, seed=3, noise=4.0)


def symbol_counts(cf):
    tally = [(jw._Tally(), jw._Tally()) for _ in cf.hv]
    jw.encode_scan_np(cf.order, cf.owner, {q: t[0] for q, t in enumerate(tally)}, {q: t[1] for q, t in enumerate(tally)}, 0)
    return [(t[0].n, t[1].n) for t in tally]


@functools.lru_cache(maxsize=None)
def cap_shapes(lname):
    """per component ({shape: DC table}, {shape: AC table}) over the component's own symbol counts, as test_huffman_tables.picture_shapes"""
    return [(jw.huffman_shapes(jw.DC_SYMBOLS, d, seed=2 * c), jw.huffman_shapes(jw.AC_SYMBOLS, a, seed=2 * c + 1))
            for c, (d, a) in enumerate(symbol_counts(cap_source(lname)))]


def deep_pair(lname, c):
    """A valid pair (codes of at most 16 bits, the all-ones code free) built to need the most table space: a code of every length
    from 10 to 16 bits in front of the 16-bit codes, so that every 9-bit prefix that holds long codes needs a second-level table of
    its full size, over all 256 AC symbols and 16 DC symbols; ranked by component c's own counts, so that the four pairs differ."""
    d, a = symbol_counts(cap_source(lname))[c]
    rd = sorted(range(16), key=lambda s: (-d.get(s, 0), s))
    ra = sorted(range(256), key=lambda s: (-a.get(s, 0), (s + 7 * c) % 256))
    al = [2, 3, 4, 5, 6, 7, 8, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15]
    return jw.table_of_lengths(rd, [2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 16, 16]), jw.table_of_lengths(ra, al + [16] * (256 - len(al)))


def with_pairs(lname, pairs):
    """cap_source(lname) coded again with pairs[c] = (DC table, AC table) on slot c of both classes"""
    src = cap_source(lname)
    tables = {(cls, c): pairs[c][cls] for c in range(4) for cls in (0, 1)}
    assert len({repr(tables[(0, c)]) for c in range(4)}) == 4 and len({repr(tables[(1, c)]) for c in range(4)}) == 4
    return cw.color_from_blocks(src.blocks, src.hv, src.mcux, src.mcuy, src.qt_slots, src.tq, tables, [(c, c) for c in range(4)], head=HEAD["cmyk"],
                                width=src.width, height=src.height)


def emul_problems4(lib, cf):
    """tests/test_huffman_tables.emul_problems through the twins that take the colour option"""
    want, bad = cf.order.astype(np.int16), []
    cap = len(want) + 64
    for sub in (0, 1024, 256):
        for mode in (0, 1):
            out, nb, st = np.zeros((cap, 64), np.int16), ctypes.c_size_t(), (ctypes.c_int * 8)()
            rc = lib.emul_decode_coefs_sub_color(cf.data, len(cf.data), 0, mode, sub, out.ctypes.data, cap, ctypes.byref(nb), st, COLOR_FILE)
            if rc != 0 or not np.array_equal(out[:min(nb.value, cap)], want):
                bad.append(("two-pass", sub, mode, rc, list(st)))
    for warm, cp in tht.SINGLE_SETTINGS:
        for mode in (0, 1):
            out, nb, st = np.zeros((cap, 64), np.int16), ctypes.c_size_t(), (ctypes.c_int * 8)()
            rc = lib.emul_single_decode_cp_color(cf.data, len(cf.data), 0, mode, 0, warm, 32, cp, out.ctypes.data, cap, ctypes.byref(nb), st, COLOR_FILE)
            if rc != 0 or not np.array_equal(out[:min(nb.value, cap)], want):
                bad.append(("single", warm, cp, mode, rc, list(st)))
    return bad


def test_table_set_cap_with_four_pairs(emul_lib):
    """Every shape of test_huffman_tables.SHAPES on slots 0 to 3, on 1 x 1 x 4 and on y22_k22: the shape list rotated, component c
    on shape number i + c, so that the four tables of a picture differ in kind; and the same shape on all four slots over each
    component's own symbol counts, where that gives four distinct pairs.  A set at or under 0x7fff bytes decodes in the emulator
    (both kernel sequences, every configuration of emul_problems) to the blocks written; a set over it is refused by the planner
    with MJX_ERR_BAD_HUFFMAN (include/mjx.h says so beside the status).  Measured: the largest set of the rotated lists is 30 064
    bytes (sub5, sub6, sub7, all256), of one shape on four slots 31 584 bytes (sub7); every shape fits.  Four Annex K-style pairs
    (the luminance and chrominance tables of T.81 K.3 and K.2-optimal tables of equal and of rising counts) need 25 792 bytes, four
    pairs optimised for the picture's own statistics (jpegwriter.optimal_table per component) 26 768 on 1 x 1 x 4 and 26 256 on
    y22_k22: both fit.  The one
    set over the cap is built for it (deep_pair): 34 880 bytes, a valid baseline file that Pillow reads and this decoder refuses;
    with three such pairs (26 160 bytes) it decodes."""
    largest, over = (0, None), []
    n = len(tht.SHAPES)
    for lname in CAP_LAYOUTS:
        sh = cap_shapes(lname)
        for i in range(n):
            for kind in ("rotated", "same"):
                names = [tht.SHAPES[(i + c) % n] if kind == "rotated" else tht.SHAPES[i] for c in range(4)]
                pairs = [(sh[c][0][names[c]], sh[c][1][names[c]]) for c in range(4)]
                if len({repr(p[0]) for p in pairs}) < 4 or len({repr(p[1]) for p in pairs}) < 4:
                    assert kind == "same"                                              # (a shape that does not depend on the counts)
                    continue
                cf = with_pairs(lname, pairs)
                rc, size, tabs = table_set(emul_lib, cf.data)
                assert serial_problem(cf) is None, (lname, names)                      # (the file is what the writer meant, whatever its tables)
                if rc == 0:
                    assert size <= CAP and len({t[0] for t in tabs}) == 4 and len({t[1] for t in tabs}) == 4, (lname, names, size)
                    largest = max(largest, (size, (lname, kind, names[0])))
                    assert emul_problems4(emul_lib, cf) == [], (lname, kind, names)
                else:
                    assert rc == ERR_BAD_HUFFMAN, (lname, names, rc)
                    over.append((lname, names))
    print("largest four-pair table set: %d bytes %s; sets over the cap among the shapes: %s" % (largest[0], largest[1], over))
    assert 24576 < largest[0] <= CAP and over == [], (largest, over)
    for lname in CAP_LAYOUTS:
        ak = jw._annex_k_tables()
        eq_dc, eq_ac = jw.optimal_table({s: 1 for s in jw.DC_SYMBOLS}), jw.optimal_table({s: 1 for s in jw.AC_SYMBOLS})
        eq2_dc, eq2_ac = jw.optimal_table({s: 1 + s for s in jw.DC_SYMBOLS}), jw.optimal_table({s: 1 + (s & 15) for s in jw.AC_SYMBOLS})
        annex = with_pairs(lname, [(ak[(0, 0)], ak[(1, 0)]), (ak[(0, 1)], ak[(1, 1)]), (eq_dc, eq_ac), (eq2_dc, eq2_ac)])
        own = with_pairs(lname, [(jw.optimal_table({s: d.get(s, 0) + 1 for s in jw.DC_SYMBOLS}), jw.optimal_table({s: a.get(s, 0) + 1 for s in jw.AC_SYMBOLS}))
                                 for d, a in symbol_counts(cap_source(lname))])
        for what, cf in (("Annex K-style", annex), ("optimised", own)):
            rc, size, tabs = table_set(emul_lib, cf.data)
            print("%s pairs on %s: %d bytes" % (what, lname, size))
            assert rc == 0 and size <= CAP and len(set(tabs)) == 4, (what, lname, rc, size)
            assert emul_problems4(emul_lib, cf) == [] and serial_problem(cf) is None, (what, lname)
        deep = with_pairs(lname, [deep_pair(lname, c) for c in range(4)])
        rc, _, _ = table_set(emul_lib, deep.data)
        assert rc == ERR_BAD_HUFFMAN, rc
        parts, n_parts = plan_parts(emul_lib, deep.data)
        assert n_parts == 1 and parts[0][7] == ERR_BAD_HUFFMAN
        assert serial_problem(deep) is None and pil_rgb(deep.data).shape == (88, 120, 3)     # a valid file all the same
        three = [deep_pair(lname, c) for c in range(3)]
        src = cap_source(lname)
        cf3 = cw.color_from_blocks(src.blocks, src.hv, src.mcux, src.mcuy, src.qt_slots, src.tq, {(cls, c): three[c][cls] for c in range(3) for cls in (0, 1)},
                                   [(0, 0), (1, 1), (2, 2), (0, 0)], head=HEAD["cmyk"], width=src.width, height=src.height)
        rc, size, _ = table_set(emul_lib, cf3.data)
        assert rc == 0 and 24576 < size <= CAP and emul_problems4(emul_lib, cf3) == [] and serial_problem(cf3) is None, (rc, size)


# ---- CPU: the reference ------------------------------------------------------------------------------------------------------------------
def test_ink_mul_is_monotone():
    """mul(a, k) = (a k + 127) // 255 over all 65 536 pairs: non-decreasing in both arguments -- what lets model_interval carry the
    ends of two intervals through the product -- with mul(a, 255) = a and mul(a, 0) = 0."""
    a = np.arange(256, dtype=np.uint8)
    t = scaled_ref.ink_mul(a[:, None], a[None, :])
    assert t.shape == (256, 256) and np.all(np.diff(t.astype(int), axis=0) >= 0) and np.all(np.diff(t.astype(int), axis=1) >= 0)
    assert np.array_equal(t[:, 255], a) and not t[:, 0].any() and np.array_equal(t, cw.ink_mul(a[:, None], a[None, :]))


def all_keys():
    return [("table", i) for i in range(len(table_cases()))] + [("mixed", i) for i in range(len(mixed_cases()))] + class_keys()


def model_of(key):
    fam, i = key
    if fam == "table":
        return table_cases()[i][1], table_cases()[i][2]
    if fam == "mixed":
        return mixed_cases()[i]
    return class_picture(*i).model, class_picture(*i)


def check_ambiguous(keys, scales=(1, 2, 4, 8)):
    """the condition on the inputs: per picture -- the four-table files, the mixed batch's, the class pictures -- and scale at most
    AMBIGUOUS_CAP of the bytes have lo != hi (class 4 is compared for equality and has no interval) -> {key: {scale: share}}"""
    out = {}
    for key in keys:
        if key[0] == "class" and CLASS4[key[1][0]] == 4:
            continue
        out[key] = {s: ambiguous(key, s) for s in scales}
        for s in scales:
            if (key[0], s) == ("class", 4) and key[1][0] == "sat_dense_q65535" and key[1][2] == "cmyk":
                continue                          # (the exception test_stageb_arithmetic states for this picture at 1/4; see test_ambiguous_share_per_case)
            assert out[key][s] <= AMBIGUOUS_CAP, (key, s, out[key][s])
    return out


def test_ambiguous_share_per_case():
    """At K = 64 the interval decides: per picture and scale at most 2 % of the bytes have lo != hi, on the reference alone.  The
    amplitudes of the in-range classes are test_stageb_arithmetic._in_range_amp's (off the exact integers), and off_the_integers
    does the same for whole blocks at 1/4 and 1/8.  Measured, the largest share of a picture per class at scales 1, 2, 4, 8:
    class 1: 0.0013, 0.0038, 0, 0; class 2: 0.0112, 0.0010, 0, 0; class 3: 0.0111, 0.0056, 0.0023, 0.0025; class 5: 0.0033, 0.0184,
    0.0048, 0.0065; class 6: 0.0031, 0.0017, 0.0017, 0.0016; class 4 is compared for equality.  The four-table files, whose blocks
    go through off_the_integers as well and whose seeds are chosen on the reference (make_decided): 0.0052, 0.0140, 0, 0; the mixed
    batch's: 0.0025, 0.0082, 0, 0.  One exception,
    the one tests/test_stageb_arithmetic.py states and for its reason: sat_dense_q65535 at 1/4 (four coefficients of one magnitude
    cancel to exactly 128 under a band of +-32 levels) -- asserted as what it is: 13 % on the two CMYK layouts, where components 1
    and 2 leave as bytes of their own (1023 x 65535 - 1023 x 65534 over 8 is 128 levels: 256, at the upper clamp); none on YCCK."""
    shares = check_ambiguous(all_keys())
    per = {}
    for key, row in shares.items():
        name = "class %d" % CLASS4[key[1][0]] if key[0] == "class" else key[0]
        for s, v in row.items():
            if not (key[0] == "class" and key[1][0] == "sat_dense_q65535" and s == 4 and key[1][2] == "cmyk"):
                per[(name, s)] = max(per.get((name, s), 0.0), v)
    print("largest ambiguous share per (family, scale):", {k: round(v, 5) for k, v in sorted(per.items())})
    exc = [ambiguous(("class", ("sat_dense_q65535", l, m)), 4) for l, m in COMBOS]
    print("sat_dense_q65535 at 1/4:", [round(v, 4) for v in exc])
    assert [v > AMBIGUOUS_CAP for v in exc] == [m == "cmyk" for _, m in COMBOS], exc


PLANTS = ["k_table0", "k_table0_scaled", "mul_no_127", "ycck_no_complement", "k_no_128", "swap_1_3"]


def test_planted_errors_in_the_reference_are_caught():
    """Each planted error (scaled_ref.model_bytes: K dequantised with component 0's table, the same at reduced scales only, mul
    without its + 127, YCCK without the complement, K without its + 128, components 1 and 3 swapped) recomputes the float64 picture
    of the GPU cases and must leave [lo, hi] on at least a tenth of the pixels of at least one case; without a plant no byte does.
    The K tables are a factor of two or more from component 0's at every position, which is what makes the first two hold.  The
    printed table has, per plant, the largest share of pixels outside and the case that gives it; measured: 1.000 for each of the six
    (a one-MCU four-table picture; k_table0_scaled at 1/4, ycck_no_complement on the YCCK file)."""
    keys = [k for k in all_keys() if model_of(k)[0] in ("cmyk", "ycck") and not (k[0] == "class" and CLASS4[k[1][0]] == 4)]
    for plant in [None] + PLANTS:
        best = (0.0, None)
        for key in keys:
            model, cf = model_of(key)
            if plant == "ycck_no_complement" and model != "ycck":
                continue
            if plant == "swap_1_3" and model == "ycck" and cf.hv[1] != cf.hv[3]:
                continue
            for s in ((2, 4, 8) if plant == "k_table0_scaled" else (1, 2) if key[0] == "class" else (1, 2, 4, 8)):
                lo, hi = interval_of(key, s)
                got = scaled_ref.model_bytes(cf, model, s, plant)
                out = ((got < lo) | (got > hi)).any(axis=2).mean()
                if plant is None:
                    assert out == 0.0, (key, s)
                best = max(best, (float(out), (key, s)), key=lambda t: t[0])
        if plant is not None:
            print("plant %-20s leaves the interval on %.3f of the pixels of %s" % (plant, best[0], best[1]))
            assert best[0] >= 0.1, (plant, best)
    # the scale-1 picture of the plant that is wrong at reduced scales only stays inside: it takes a reduced scale to see it
    model, cf = table_cases()[3][1:]
    assert np.array_equal(scaled_ref.model_bytes(cf, model, 1, "k_table0_scaled"), scaled_ref.model_bytes(cf, model, 1))


def f32_component(cf, c, scale):
    """component c's byte plane as the numpy float32 restatement of stage B gives it (test_stageb_arithmetic.stageb_f32 on the
    one-component picture that carries c's blocks), under every output pixel"""
    g = grey_view(cf, c)
    p = types.SimpleNamespace(hv=[(1, 1)], per_comp=[g.blocks[0]], per_mcu=[1], qts=[np.asarray(cf.qts[c], np.int64)], mcux=g.mcux, mcuy=g.mcuy,
                              hmax=1, vmax=1, w=g.width, h=g.height)
    plane = tsa.stageb_f32(p, scale)[:, :, 0]
    h, v = cf.hv[c]
    return cw.replicate(plane, h, v, cf.hmax, cf.vmax, -(-cf.width // scale), -(-cf.height // scale))


def test_K_of_the_float32_restatement_with_a_fourth_component():
    """The measurement behind K = 64 (test_stageb_arithmetic: 4 x the largest K a float32 CPU restatement needs) repeated on the new
    classes: per class picture, scale and component the smallest K under which the numpy float32 restatement of stage B (the
    reference's, not the kernel's) puts every byte of the component inside byte_interval -- for a YCCK picture's first three
    components inside rgb_interval.  Measured over scales 1, 2, 4, 8: the largest is K = 3.34 (sat_sparse_q65535 on 1 x 1 x 4 as
    CMYK, scale 1, component 2 -- a component that a YCbCr picture never stores as a byte of its own; test_stageb_arithmetic's K_b
    is 1.92); 4 x 3.34 = 13.4 <= 64.  And the composed restatement lies inside model_interval."""
    worst = (0.0, None)
    for _, (v, l, m) in class_keys():
        cf = class_picture(v, l, m)
        if cf.cls == 4:
            continue
        for scale in (1, 2, 4, 8):
            comp = []
            for c in (range(4) if m == "cmyk" else (3,)):
                got = f32_component(cf, c, scale)
                s, mag = scaled_ref.component_samples(cf, c, scale)
                k, _ = tsa.needed_k(got[:, :, None], (s + 128.0)[:, :, None], mag + 128.0)
                worst = max(worst, (k, (v, l, m, scale, c)), key=lambda t: t[0])
                comp.append(got)
            if m == "ycck":
                data3, dec3 = scaled_ref.ycc_part(cf)
                p3 = types.SimpleNamespace(hv=cf.hv[:3], per_comp=cf.blocks[:3], per_mcu=[h * w for h, w in cf.hv[:3]], qts=[np.asarray(q, np.int64) for q in cf.qts[:3]],
                                           mcux=cf.mcux, mcuy=cf.mcuy, hmax=cf.hmax, vmax=cf.vmax, w=cf.width, h=cf.height)
                rgb = tsa.stageb_f32(p3, scale)
                k, _ = tsa.needed_k(rgb, scaled_ref.rgb_f64(data3, scale, dec3), scaled_ref.magnitude(data3, scale, dec3))
                worst = max(worst, (k, (v, l, m, scale, "ycc")), key=lambda t: t[0])
                pic = cw.ink_mul(255 - rgb, comp[0][:, :, None])
            else:
                pic = np.stack([cw.ink_mul(comp[c], comp[3]) for c in range(3)], axis=2)
            lo, hi = interval_of(("class", (v, l, m)), scale)
            assert not ((pic < lo) | (pic > hi)).any(), (v, l, m, scale)
    print("K the float32 restatement needs with a fourth component: %.3f on %s" % worst)
    assert 4.0 * worst[0] <= K, worst


def test_class_conditions_with_a_fourth_component():
    """What the two new generators are for, on float64 alone.  Class 4: the levels run through -40 .. 300 on component 0 and on K,
    the float64 picture is the integer one at every scale, and so is the float32 restatement at scales 1 and 8.  Class 5: K leaves
    0..255 on both sides where all three inks are inside, and each ink does where K is inside."""
    for l, m in COMBOS:
        cf = class_picture("exact4", l, m)
        assert set(cf.blocks[0][:, 0] + 128) == set(range(-40, 301)) and set(cf.blocks[3][:, 0] + 128) == set(range(-40, 301))
        for scale in (1, 2, 4, 8):
            want = exact4_want(cf, scale)
            assert np.array_equal(scaled_ref.model_bytes(cf, m, scale), want), (l, m, scale)
            if scale in (1, 8):
                k = f32_component(cf, 3, scale)
                c0 = f32_component(cf, 0, scale)
                assert np.array_equal(cw.ink_mul(255 - c0 if m == "ycck" else c0, k), want[:, :, 0]), (l, m, scale)
        assert len(np.unique(want)) > 100
        cf = class_picture("sat_k", l, m)
        s = [scaled_ref.component_samples(cf, c, 1)[0] + (128.0 if (c == 0 or m == "cmyk" or c == 3) else 0.0) for c in range(4)]
        if m == "ycck":
            data3, dec3 = scaled_ref.ycc_part(cf)
            ink = 255.0 - scaled_ref.rgb_f64(data3, 1, dec3)
        else:
            ink = np.stack(s[:3], axis=2)
        k = s[3]
        ink_in = np.all((ink > 0) & (ink < 255), axis=2)
        assert (ink_in & (k < 0)).mean() > 0.02 and (ink_in & (k > 255)).mean() > 0.02, (l, m)
        for ch in range(3):
            assert (((k > 0) & (k < 255)) & (ink[:, :, ch] < 0)).any() and (((k > 0) & (k < 255)) & (ink[:, :, ch] > 255)).any(), (l, m, ch)


# ---- the DC family for four sums ---------------------------------------------------------------------------------------------------------
DC_LAYOUTS4 = ["1x1x4", "h2_k2", "v2_k2", "y22_k11", "y22_k22"]           # 4, 6, 6, 7 and 10 blocks per MCU
DC_COUNTS, DC_RESTARTS = tgl.DC_COUNTS, tgl.DC_RESTARTS
SIDE = 65535


@functools.lru_cache(maxsize=None)
def dc4_picture(lname, k, r):
    """test_geometry_limits.dc_picture with four components: every component's DC drawn over -1024 .. 1023; a run -1024, 1023, -1024,
    1023 (one value more for K) that holds the last block in front of the first segment boundary and the first behind it, starting
    3, 2, 1 and 4 blocks in front of the boundary for the four components, so that the difference across the boundary is +-2047 in
    each; 1023, -1024, 1023 at the picture's start.  One MCU wide where 65535 rows allow it."""
    hv = LAYOUTS4[lname]
    nmcu = 2048 * k + r
    mh = 8 * max(v for _, v in hv)
    mcux = 1
    while nmcu % mcux or (nmcu // mcux) * mh > SIDE:
        mcux += 1
    rng = np.random.RandomState(7000 + 10 * nmcu + DC_LAYOUTS4.index(lname))
    per_comp = []
    for c, (h, v) in enumerate(hv):
        co = np.zeros((nmcu * h * v, 64), np.int64)
        co[:, 0] = rng.randint(-1024, 1024, len(co))
        edge = 2048 * h * v                                  # the component's first block behind the first segment boundary
        at = edge + (-3, -2, -1, -4)[c]
        if edge < len(co):                                   # (the run is cut where the picture ends: it still holds edge - 1 and edge)
            run = np.array([-1024, 1023, -1024, 1023, -1024])[:min(5 if c == 3 else 4, len(co) - at)]
            co[at:at + len(run), 0] = run
        co[:3, 0] = [1023, -1024, 1023]
        per_comp.append(co)
    return types.SimpleNamespace(hv=hv, nmcu=nmcu, mcux=mcux, mcuy=nmcu // mcux, per_comp=per_comp)


@functools.lru_cache(maxsize=None)
def dc4_file(lname, k, r, restart=0):
    p = dc4_picture(lname, k, r)
    ak = jw._annex_k_tables()
    return cw.color_from_blocks(p.per_comp, p.hv, p.mcux, p.mcuy, {0: [1] * 64, 1: [1] * 64}, [0, 1, 1, 0], {(cls, s): ak[(cls, s)] for s in (0, 1) for cls in (0, 1)},
                                [(0, 0), (1, 1), (1, 1), (0, 0)], head=HEAD["cmyk"], restart=restart or None)


def test_dc_family_inputs_reach_every_difference():
    """on the input: differences of +2047 and -2047 in each of the four components, with and without the boundary run"""
    for lname in DC_LAYOUTS4:
        for k, r in DC_COUNTS:
            p = dc4_picture(lname, k, r)
            for c in range(4):
                d = np.diff(p.per_comp[c][:, 0])
                assert d.max() == 2047 and d.min() == -2047, (lname, k, r, c)
                edge = 2048 * p.hv[c][0] * p.hv[c][1]
                if edge < len(p.per_comp[c]):                # the difference that straddles the segment boundary itself
                    assert abs(d[edge - 1]) == 2047, (lname, k, r, c)
            assert p.mcux * p.mcuy == p.nmcu and p.mcuy * 8 * max(v for _, v in p.hv) <= SIDE
    assert dc4_picture("y22_k11", 0, 1800).nmcu == 600 * 3 and dc4_picture("1x1x4", 0, 700).nmcu == 700


# ---- damaged four-component scans ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damaged_sources():
    """[(model, ColorFile)]: h2_k2 CMYK and 1 x 1 x 4 YCCK, 64 x 48, restart interval 3, quality 95 with noise, four pairs on crossed
    slots"""
    return [("cmyk", make("cmyk", LAYOUTS4["h2_k2"], 64, 48, quality=95, seed=171, noise=25.0, restart=3)),
            ("ycck", make("ycck", LAYOUTS4["1x1x4"], 64, 48, quality=95, seed=172, noise=25.0, restart=3))]


def rebuild(head, scan, rst):
    """the file of a de-stuffed scan (without its end-of-image marker) and the offsets behind its RSTn markers: stuffed again, the markers numbered 0, 1, ... mod 8"""
    cuts = [0] + list(rst) + [len(scan)]
    raw = b"".join(dr.stuff(scan[a:b]) + (bytes([0xff, 0xd0 + g % 8]) if g + 2 < len(cuts) else b"") for g, (a, b) in enumerate(zip(cuts, cuts[1:])))
    return head + raw + b"\xff\xd9"


class Damaged:
    def __init__(self, name, src, data):
        self.name, self.source, self.data = name, src, data
        pic = dr.Picture(damaged_sources()[src][1].data)
        scan, rst = dr.destuff(dr.Picture(data).raw, True)
        self.ref = dr.decode(pic, scan, rst)


@functools.lru_cache(maxsize=None)
def damaged_family():
    out = []
    for si, (model, cf) in enumerate(damaged_sources()):
        pic = dr.Picture(cf.data)
        clean = dr.decode(pic)
        assert clean.verdict == dr.OK and np.array_equal(clean.t0, cf.order.astype(np.int16)) and pic.restart == 3
        raw = pic.raw[:-2]
        # cuts at every byte of the last two MCUs
        n = len(cf.order) - 2 * cf.bpm
        prefix = jw.encode_scan_np(cf.order[:n], cf.owner[:n], cf.codes[0], cf.codes[1], restart_blocks=3 * cf.bpm)
        assert raw.startswith(prefix[:-1]) and len(raw) - len(prefix) >= 16
        for keep in range(len(prefix) - 1, len(raw) + 1):
            b = raw[:keep]
            while b.endswith(b"\xff") or b.endswith(b"\xff\x00"):
                b = b[:-1] if b.endswith(b"\xff") else b[:-2]
            out.append(Damaged("%s cut to %d of %d" % (model, keep, len(raw)), si, pic.head + b + b"\xff\xd9"))
        # an invalid code planted in a block of each component: the table's own unmatched pattern at the block's first bit
        body = pic.scan[:-2]
        for c in range(4):
            blk = next(b for b in range(len(cf.order) // 3, len(cf.order)) if cf.owner[b] == c and b % (3 * cf.bpm) != 0)
            pat = dr.unmatched_patterns(pic.dht[(0, CROSSED[c][0])])
            assert pat, c
            e = int(clean.ends[blk - 1])
            hit = bytearray(body)
            for j, ch in enumerate(pat[0]):
                q = e + j
                hit[q >> 3] = (hit[q >> 3] & ~(0x80 >> (q & 7))) | ((0x80 >> (q & 7)) if ch == "1" else 0)
            d = Damaged("%s unmatched DC pattern in block %d of component %d" % (model, blk, c), si, rebuild(pic.head, bytes(hit), pic.rst))
            assert (blk, e) in d.ref.invalid, d.name
            out.append(d)
        # 64 single-byte substitutions (no byte of or next to a marker or a stuffed FF, and no new FF)
        rng = np.random.default_rng([len(raw), 64])
        free = [j for j in range(1, len(raw) - 1) if 0xff not in raw[j - 1:j + 2]]
        for q in rng.choice(free, 64, replace=False):
            v = int(rng.integers(0, 255))
            v = v ^ 1 if v == raw[q] else v
            out.append(Damaged("%s byte %d = %02x" % (model, q, v), si, pic.head + raw[:q] + bytes([v]) + raw[q + 1:] + b"\xff\xd9"))
        # one RSTn missing, one misnumbered
        marks = [j for j in range(len(raw) - 1) if raw[j] == 0xff and (raw[j + 1] & 0xf8) == 0xd0]
        assert len(marks) == cf.mcux * cf.mcuy // 3 - 1
        g = len(marks) // 2
        out.append(Damaged("%s marker %d missing" % (model, g), si, pic.head + raw[:marks[g]] + raw[marks[g] + 2:] + b"\xff\xd9"))
        wrong = bytes([0xff, 0xd0 + (raw[marks[g] + 1] + 3) % 8])
        out.append(Damaged("%s marker %d misnumbered" % (model, g), si, pic.head + raw[:marks[g]] + wrong + raw[marks[g] + 2:] + b"\xff\xd9"))
    return out


def test_damaged_family_has_every_verdict():
    fam = damaged_family()
    verdicts = {(d.source, d.ref.verdict) for d in fam}
    assert verdicts == {(s, v) for s in (0, 1) for v in (dr.OK, dr.TRUNCATED, dr.BAD_HUFFMAN)}, verdicts
    changed = sum(1 for d in fam if d.ref.verdict == dr.OK and not np.array_equal(d.ref.t0, damaged_sources()[d.source][1].order.astype(np.int16)))
    print("%d damaged files; %d decode as OK with other coefficients than the intact file's" % (len(fam), changed))
    assert changed > 0
    missing = [d for d in fam if "missing" in d.name]
    assert all(d.ref.verdict == dr.TRUNCATED for d in missing)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
def run_batch(mjx, ctx, datas, **kw):
    """a Batch over parsed scans with the colour option, decoded -> (batch, scans); close_batch closes both"""
    scans = [mjx.ParsedScan(d, color="file") for d in datas]
    b = mjx.Batch(ctx, scans, color="file", **kw)
    b.decode()
    b.wait()
    return b, scans


def close_batch(b, scans):
    b.close()
    for s in scans:
        s.close()


def outside(got, key, scale, rect=None):
    """None, or where and how a device picture leaves its interval"""
    lo, hi = interval_of(key, scale)
    if rect is not None:
        lo, hi = tcd.crop(lo, rect), tcd.crop(hi, rect)
    if got.shape != lo.shape:
        return ("shape", got.shape, lo.shape)
    bad = (got < lo) | (got > hi)
    if not bad.any():
        return None
    y, x, ch = (int(v) for v in np.argwhere(bad)[0])
    return ("%d of %d bytes outside" % (int(bad.sum()), bad.size), "first at (y %d, x %d, channel %d): got %d, interval [%d, %d]"
            % (y, x, ch, got[y, x, ch], lo[y, x, ch], hi[y, x, ch]))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_four_tables_through_every_form(mjx, gpu_ctx, scale):
    """The five four-component layouts as CMYK and as YCCK and RGB at 4:4:4 and 4:2:0 with three tables, one MCU and 37 x 29, every
    component on a DQT of its own (K's a factor of two or more above component 0's, one table 16-bit) and on crossed Huffman slots:
    status OK, the file's model, T0 the blocks written, every byte inside model_interval and equal to the twins' composition; the same
    pictures one per chunk; an unaligned rectangle (the crop, byte for byte); a normalised planar float32 Output (the format table
    on the packed bytes, bit for bit).  At 1/2 and below the fourth component's multipliers are the second 64 of its pool entry."""
    cases = table_cases()
    check_ambiguous([("table", i) for i in range(len(cases))], (scale,))          # the condition on the inputs, before any device byte
    datas = [cf.data for _, _, cf in cases]
    want = tcd.expectations(mjx, gpu_ctx, [(m, cf) for _, m, cf in cases], scale=scale)
    b, scans = run_batch(mjx, gpu_ctx, datas, keep_coefs=True, scale=scale)
    bad, whole = [], []
    try:
        for i, (tag, model, cf) in enumerate(cases):
            assert b.status(i) == mjx.OK and b.color_model(i) == MODEL[model], (tag, b.status(i))
            if not np.array_equal(b.coefs(i), cf.order.astype(np.int16)):
                bad.append((tag, "T0"))
            got = b.rgb(i)
            whole.append(got)
            out = outside(got, ("table", i), scale)
            if out:
                bad.append((tag, "interval") + out)
            if got.shape != want[i].shape or not np.array_equal(got, want[i]):
                bad.append((tag, "twins", int((got != want[i]).sum()) if got.shape == want[i].shape else -1))
    finally:
        close_batch(b, scans)
    assert bad == [], bad
    tags = [t for t, _, _ in cases]
    tcd.check_equal(tcd.decode_all(mjx, gpu_ctx, datas, color="file", chunk_images=1, scale=scale), whole, tags)
    big = [i for i, (_, _, cf) in enumerate(cases) if cf.width == 37]
    ow, oh = -(-37 // scale), -(-29 // scale)
    r = (5, 3, 17, 11) if scale == 1 else (1, 1, max(1, ow - 3), max(1, oh - 2))
    got = tcd.decode_all(mjx, gpu_ctx, [datas[i] for i in big], color="file", scale=scale, rois=r)
    tcd.check_equal(got, [tcd.crop(whole[i], r) for i in big], [tags[i] for i in big])
    fmt = mjx.Output("float32", planar=True, mean=of.IMAGENET_MEAN, std=of.IMAGENET_STD)
    for g, p, t in zip(tcd.run_out(mjx, gpu_ctx, datas, output=fmt, scale=scale), whole, tags):
        assert of.same_bits(g, of.expected(np.ascontiguousarray(p), fmt)), (t, "float32 planar")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_mixed_batch_with_tables_of_their_own(mjx, gpu_ctx, scale):
    """One batch ordered three-component, four-component, grey, four-component, three-component, every picture with DQTs no other has
    (at no position), so that a wrong offset into the multiplier pool -- its tail holds the fourth components' multipliers behind both
    halves -- lands on a neighbour's numbers; and behind them a valid file whose four table pairs exceed the decode-table cap: it gets
    MJX_ERR_BAD_HUFFMAN, the others their pictures, byte for byte what they are without it."""
    cases = mixed_cases()
    check_ambiguous([("mixed", i) for i in range(len(cases))], (scale,))          # the condition on the inputs, before any device byte
    datas = [grey_of(cf)[0] if m == "grey" else cf.data for m, cf in cases]
    t0 = [grey_view(cf).blocks[0] if m == "grey" else cf.order for m, cf in cases]
    twins = tcd.expectations(mjx, gpu_ctx, [(m, cf) for m, cf in cases if m != "grey"], scale=scale)
    twins.insert(2, None)
    deep = with_pairs("1x1x4", [deep_pair("1x1x4", c) for c in range(4)]).data
    pictures = []
    for files in (datas + [deep], datas):
        b, scans = run_batch(mjx, gpu_ctx, files, keep_coefs=True, scale=scale)
        try:
            st = [b.status(i) for i in range(len(files))]
            assert st == [mjx.OK] * 5 + [mjx.ERR_BAD_HUFFMAN] * (len(files) - 5), st
            got = [b.rgb(i) for i in range(5)]
            for i, (m, cf) in enumerate(cases):
                assert np.array_equal(b.coefs(i), t0[i].astype(np.int16)), (i, m, "T0")
                assert outside(got[i], ("mixed", i), scale) is None, (i, m, outside(got[i], ("mixed", i), scale))
                if twins[i] is not None:
                    assert np.array_equal(got[i], twins[i]), (i, m, "twins")
            pictures.append(got)
        finally:
            close_batch(b, scans)
    tcd.check_equal(pictures[0], pictures[1], [m for m, _ in cases])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("combo", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_arithmetic_classes_with_a_fourth_component(mjx, gpu_ctx, combo, scale):
    """The classes of tests/test_stageb_arithmetic.py with a fourth component (basis, pairs, dense, sat and over from its generators,
    class 4 and a saturating K from this module's), 189 x 131 with the last column and row clipped, on 1 x 1 x 4 and y22_k22 as CMYK
    and on h2_k2 as YCCK: T0 is the blocks written, so a pixel failure is stage B's; every byte inside model_interval; class 4 equal
    to mul(clamp(l_c), clamp(l_K)) at scales 1 and 8.  The condition on the inputs -- at most 2 % of a picture's bytes undecided --
    is asserted before any device byte is looked at."""
    l, m = combo
    pics = [class_picture(v, l, m) for v in variants_of(m)]
    keys = [("class", (v, l, m)) for v in variants_of(m)]
    check_ambiguous(keys, (scale,))
    b, scans = run_batch(mjx, gpu_ctx, [p.data for p in pics], keep_coefs=True, scale=scale)
    bad = []
    try:
        for i, p in enumerate(pics):
            assert b.status(i) == mjx.OK and b.color_model(i) == MODEL[m], (p.variant, b.status(i))
            if not np.array_equal(b.coefs(i), p.order16):
                bad.append((p.variant, "T0"))
            got = b.rgb(i)
            if p.cls == 4 and scale in (1, 8):
                if not np.array_equal(got, exact4_want(p, scale)):
                    bad.append((p.variant, "exact", int((got != exact4_want(p, scale)).sum())))
            else:
                out = outside(got, keys[i], scale)
                if out:
                    bad.append((p.variant,) + out)
    finally:
        close_batch(b, scans)
    assert bad == [], bad


def dc_problems(mjx, b, files):
    bad = []
    for i, cf in enumerate(files):
        want = cf.blocks if isinstance(cf.blocks, np.ndarray) and cf.blocks.ndim == 2 else cf.order
        if b.status(i) != mjx.OK:
            bad.append((i, "status", b.status(i)))
        elif not np.array_equal(b.coefs(i), np.asarray(want).astype(np.int16)):
            got = b.coefs(i)[:, 0].astype(np.int64)
            first = int(np.argmax(got != np.asarray(want)[:, 0])) if len(got) == len(want) else -1
            bad.append((i, "T0 differs from block", first))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("lname", DC_LAYOUTS4)
def test_dc_family_for_four_sums(mjx, gpu_ctx, lname):
    """k_dc_sums4 / k_dc_apply4 / k_dc_restart4 on 4, 6, 6, 7 and 10 blocks per MCU: MCU counts on both sides of every 2048-MCU
    segment boundary, runs of -1024 / 1023 across the boundary in each of the four components at block offsets of their own, no
    restart interval and intervals of 1 and 2049 MCUs: T0 is the blocks written and no run is left unconverged.
    MJX_DC_ONE_PASS does not change which kernels a four-component picture takes -- launch_dc_scan launches the three kernels above
    for the chunk's four-component pictures whatever `segflag` is; the switch selects between k_dc_scan_t and the two-pass kernels
    for the pictures of up to three components only -- so the family is not repeated in a child process."""
    cases = [(lname, k, r, rst) for k, r in DC_COUNTS for rst in DC_RESTARTS]
    files = [dc4_file(*c) for c in cases]
    b, scans = run_batch(mjx, gpu_ctx, [f.data for f in files], keep_coefs=True)
    try:
        bad = [(cases[p[0]],) + p[1:] for p in dc_problems(mjx, b, files)]
        assert b.unconverged_runs() == 0
    finally:
        close_batch(b, scans)
    assert bad == [], bad


@pytest.mark.gpu
def test_dc_restart_workgroups_and_neighbours_of_the_same_shape(mjx, gpu_ctx):
    """k_dc_restart4 takes an interval per lane, eight blocks at a time: 600 intervals of 3 MCUs of y22_k11 (21 blocks, not a multiple
    of eight) and 700 intervals of one 1 x 1 x 4 MCU fill a second and a third workgroup.  And in the same batch 1 x 1 x 4 stands beside
    a 4:2:2 picture and h2_k2 beside a 4:2:0 picture of the same MCU counts (2049, without restart intervals and with intervals of one
    MCU): four and six blocks per MCU with four running sums and with three, which DevImage::dc_shape keeps apart.  All exact."""
    files = [dc4_file("y22_k11", 0, 1800, 3), dc4_file("1x1x4", 0, 700, 1)]
    datas = [f.data for f in files]
    for rst in (0, 1):
        for lname, bpm in (("1x1x4", 4), ("h2_k2", 6)):
            files.append(dc4_file(lname, 1, 1, rst))
            datas.append(files[-1].data)
            files.append(tgl.dc_picture(bpm, 1, 1))
            datas.append(tgl.dc_file(bpm, 1, 1, rst))
    assert files[0].restart == 3 and files[0].mcux * files[0].mcuy == 1800 and files[1].mcux * files[1].mcuy == 700
    b, scans = run_batch(mjx, gpu_ctx, datas, keep_coefs=True)
    try:
        bad = dc_problems(mjx, b, files)
        assert b.unconverged_runs() == 0
        assert [b.color_model(i) for i in range(2, 6)] == [mjx.MODEL_CMYK, mjx.MODEL_YCBCR] * 2
    finally:
        close_batch(b, scans)
    assert bad == [], bad


# ---- GPU: damaged four-component scans -------------------------------------------------------------------------------------------------------
STATUS_OF = {dr.OK: 0, dr.TRUNCATED: 1, dr.BAD_HUFFMAN: 4}
GROUP = 250


@functools.lru_cache(maxsize=None)
def damaged_groups():
    """the family in groups of about GROUP pictures, the intact source in front of every 8 damaged ones: [[(data, status, T0 or None,
    name, index of the source for an intact picture or None)]]"""
    rows = []
    for k, d in enumerate(damaged_family()):
        if k % 8 == 0:
            cf = damaged_sources()[d.source][1]
            rows.append((cf.data, 0, cf.order.astype(np.int16), "intact %d" % d.source, d.source))
        rows.append((d.data, STATUS_OF[d.ref.verdict], d.ref.t0 if d.ref.verdict == dr.OK else None, d.name, None))
    return [rows[k:k + GROUP] for k in range(0, len(rows), GROUP)]


@pytest.fixture(scope="module")
def intact_pictures(mjx, gpu_ctx):
    """the packed pictures of the two intact sources, decoded alone; inside their intervals.  (The family and its serial decodes are
    built here as well: once per session and outside the GPU tests' own time, as test_damaged_streams.prepared does.)"""
    damaged_groups()
    srcs = damaged_sources()
    got = tcd.decode_all(mjx, gpu_ctx, [cf.data for _, cf in srcs], color="file")
    for (m, cf), g in zip(srcs, got):
        lo, hi = scaled_ref.model_interval(cf, m, 1, K)
        assert not ((g < lo) | (g > hi)).any(), m
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["batch", "decode_batch", "device_destuff"])
def test_damaged_four_component_scans(mjx, gpu_ctx, intact_pictures, door):
    """An h2_k2 CMYK and a 1 x 1 x 4 YCCK file with restart interval 3 and four table pairs, damaged: cut at every byte of the last
    two MCUs, a table's unmatched bit pattern planted at the first bit of a block of each component, 64 single-byte substitutions, one
    RSTn marker missing and one misnumbered.  Status and, where OK, coefficients are the serial decode's (damaged_ref.decode, the band
    rule) through the batch API on parsed scans and through mjx_decode_batch with host and with device de-stuffing; the intact
    pictures between them keep their coefficients and their bytes."""
    bad = []
    for rows in damaged_groups():
        datas = [r[0] for r in rows]
        if door == "batch":
            b, scans = run_batch(mjx, gpu_ctx, datas, keep_coefs=True)
            st = [b.status(i) for i in range(len(rows))]
        else:
            b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=door == "device_destuff", keep_coefs=True, color="file")
            scans = []
        try:
            for i, (data, want, t0, name, src) in enumerate(rows):
                if st[i] != want or b.status(i) != want:
                    bad.append((name, "status", st[i], b.status(i), want))
                elif t0 is not None and not np.array_equal(b.coefs(i), t0):
                    bad.append((name, "T0"))
                elif src is not None and not np.array_equal(b.rgb(i), intact_pictures[src]):
                    bad.append((name, "pixels"))
        finally:
            close_batch(b, scans)
    assert bad == [], (len(bad), bad[:12])


_CHILD = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import __graft_entry__ as ge
mjx = ge.load_package()
job = json.load(open(%(job)r))
ctx = mjx.Context(0, profiling=True, throughput_plan=True)
res = []
for paths in job['groups']:
    scans = [mjx.ParsedScan(open(p, 'rb').read(), color='file') for p in paths]
    b = mjx.Batch(ctx, scans, keep_coefs=True, color='file')
    b.kernel_ms(reset=True)
    b.decode(); b.wait()
    k = b.kernel_ms()
    st = [b.status(i) for i in range(len(paths))]
    sha = [hashlib.sha1(b.coefs(i).tobytes()).hexdigest() if s == 0 else None for i, s in enumerate(st)]
    pix = [hashlib.sha1(np.ascontiguousarray(b.rgb(i)).tobytes()).hexdigest() if s == 0 else None for i, s in enumerate(st)]
    res.append(dict(status=st, sha=sha, pix=pix, emit=k['huff_emit'][1], write=k['huff_write'][1], unconverged=b.unconverged_runs()))
    b.close()
    for s in scans:
        s.close()
ctx.close()
print(json.dumps(res))
"""


@pytest.mark.gpu
def test_damaged_four_component_scans_with_the_single_decode_off(mjx, intact_pictures, tmp_path):
    """The same family with MJX_SINGLE_DECODE=0 in a child process, as test_damaged_streams.test_family_with_the_single_decode_off: the
    two-pass kernels alone give the serial decode's statuses and coefficients, and the intact pictures their bytes."""
    groups = damaged_groups()
    job = dict(groups=[])
    for g, rows in enumerate(groups):
        paths = []
        for i, r in enumerate(rows):
            p = tmp_path / ("off_%d_%d.jpg" % (g, i))
            p.write_bytes(r[0])
            paths.append(str(p))
        job["groups"].append(paths)
    (tmp_path / "off.json").write_text(json.dumps(job))
    script = tmp_path / "off.py"
    script.write_text(_CHILD % dict(root=ROOT, job=str(tmp_path / "off.json")))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env["MJX_SINGLE_DECODE"] = "0"
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    bad = []
    for rows, out in zip(groups, res):
        for i, (data, want, t0, name, src) in enumerate(rows):
            if out["status"][i] != want:
                bad.append((name, "status", out["status"][i], want))
            elif t0 is not None and out["sha"][i] != hashlib.sha1(np.ascontiguousarray(t0).tobytes()).hexdigest():
                bad.append((name, "T0"))
            elif src is not None and out["pix"][i] != hashlib.sha1(np.ascontiguousarray(intact_pictures[src]).tobytes()).hexdigest():
                bad.append((name, "pixels"))
    assert sum(o["emit"] for o in res) == 0 and all(o["write"] > 0 for o in res), [(o["emit"], o["write"]) for o in res]
    assert bad == [], (len(bad), bad[:12])

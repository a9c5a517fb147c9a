"""Sampling factors of 4 (4:1:1, 4:1:0 and every other layout with a factor of 4): names, files and numpy references.

A layout is named as in test_sampling_layouts: Y41_Cb11_Cr11 is luma 4 blocks wide and 1 tall (4:1:1).  WIDE holds the 206
three-component layouts with h, v in {1, 2, 4}, at least one factor of 4 and at most 12 blocks per MCU; GRAYS the greyscale frames
whose SOF carries a 4.  The oracle restates the reference and panics on these files, so nothing here asks it: the writer's own
quantised blocks are T0, and scaled_ref / libjpeg_ref take them through a stand-in for the oracle's decode (`dec_of`).

libjpeg's pixels: a component whose ratio is 4 in either direction is replicated in both (jdsample.c int_upsample, the routine
libjpeg picks for every ratio pair that is not 1x1, 2x1, 1x2 or 2x2); every other component keeps libjpeg_ref's triangle filters.
`upsample` is that rule, `rule="filter2"` the planted alternative (filter the direction whose ratio is 2, replicate the other).
"""
import functools
import itertools
import types

import numpy as np

import jpegwriter as jw
import libjpeg_ref
import scaled_ref

F = (1, 2, 4)
HV = [(h, v) for h in F for v in F]
ALL = [list(x) for x in itertools.product(HV, repeat=3) if sum(h * v for h, v in x) <= 12]
WIDE = [x for x in ALL if max(f for c in x for f in c) == 4]
GRAYS = ["gray41", "gray14", "gray44"]
NAMED = ["Y41_Cb11_Cr11", "Y42_Cb11_Cr11", "Y14_Cb11_Cr11", "Y24_Cb11_Cr11", "Y41_Cb21_Cr11", "Y11_Cb41_Cr14", "Y22_Cb41_Cr12",
         "Y42_Cb21_Cr12"]


def name(hv):
    return "Y%d%d_Cb%d%d_Cr%d%d" % tuple(f for c in hv for f in c)


def parse_name(s):
    return [(int(p[-2]), int(p[-1])) for p in s.split("_")]


NAMES = [name(hv) for hv in WIDE]
PILLOW_NAMES = [n for n in NAMES if sum(h * v for h, v in parse_name(n)) <= 10]


def mcu_hv(lname):
    """the factors the MCU is made of: a greyscale frame is non-interleaved, one block per MCU whatever its SOF says"""
    return [(1, 1)] if lname.startswith("gray") else parse_name(lname)


def geometry(lname, w, h):
    """-> (hv of the MCU, hmax, vmax, mcux, mcuy, bpm)"""
    hv = mcu_hv(lname)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return hv, hmax, vmax, -(-w // (8 * hmax)), -(-h // (8 * vmax)), sum(a * b for a, b in hv)


def mcu_sizes(lname):
    """exactly one MCU, and one MCU plus one pixel each way"""
    _, hmax, vmax, _, _, _ = geometry(lname, 1, 1)
    return [(8 * hmax, 8 * vmax), (8 * hmax + 1, 8 * vmax + 1)]


@functools.lru_cache(maxsize=None)
def layout_file(lname, w, h, restart=None, seed=None, quality=75):
    """(bytes, per-component blocks) of layout `lname` at w x h; seed None: the layout's index x 1000 + 7 w + h (the file with and
    without restart intervals carries the same coefficients)"""
    if seed is None:
        seed = (NAMES + GRAYS).index(lname) * 1000 + w * 7 + h
    if lname.startswith("gray"):
        return jw.layout_jpeg(w, h, None, quality=quality, seed=seed, restart=restart, gray_hv=(int(lname[4]), int(lname[5])))
    return jw.layout_jpeg(w, h, parse_name(lname), quality=quality, seed=seed, restart=restart)


def dec_of(lname, w, h, blocks):
    """what scaled_ref, libjpeg_ref and jpegwriter.script_twins read of an oracle decode: coefs, mcus, hv (blocks per MCU)"""
    hv, _, _, mcux, mcuy, _ = geometry(lname, w, h)
    return types.SimpleNamespace(coefs=[np.asarray(b, np.int16) for b in blocks], mcus=mcux * mcuy, hv=[a * b for a, b in hv])


def interleave(dec):
    """per-component blocks -> MCU-interleaved decode order [mcus * bpm, 64] int16 (the device buffer's order)"""
    return np.concatenate([c.reshape(dec.mcus, k, 64) for c, k in zip(dec.coefs, dec.hv)], axis=1).reshape(-1, 64).astype(np.int16)


def blocks_file(lname, w, h, blocks, data, restart=None):
    """jpeg_from_blocks of per-component blocks with the tables and Huffman codes of `data` (a layout_file of the same geometry)"""
    hv, _, _, mcux, mcuy, _ = geometry(lname, w, h)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    frame_hv = [(c[0], c[1]) for c in comps]
    dec = dec_of(lname, w, h, blocks)
    return jw.jpeg_from_blocks(interleave(dec), frame_hv, mcux, mcuy, [qt[c[2]] for c in comps], jw.tables_from_jpeg(data), width=w, height=h,
                               restart=restart)


def chroma_zeroed(lname, w, h):
    """the file of the same luminance blocks with every chroma block zero: its packed picture is the luminance picture, R = G = B"""
    data, blocks = layout_file(lname, w, h)
    z = [blocks[0]] + [np.zeros_like(b) for b in blocks[1:]]
    return blocks_file(lname, w, h, z, data)


def component_file(lname, w, h, c):
    """The one-component file that carries component c's blocks and table over the component's whole block grid (mcux h x mcuy v
    blocks): its packed decode has component c's byte at sample (x, y) in every channel of pixel (x, y)."""
    data, blocks = layout_file(lname, w, h)
    hv, _, _, mcux, mcuy, _ = geometry(lname, w, h)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    hc, vc = hv[c]
    b = np.asarray(blocks[c]).reshape(mcuy, mcux, vc, hc, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)      # decode order -> raster
    t = jw.tables_from_jpeg(data)
    slot = 0 if c == 0 or (0, 1) not in t else 1
    return jw.jpeg_from_blocks(b, [(1, 1)], mcux * hc, mcuy * vc, [qt[comps[c][2]]], {(0, 0): t[(0, slot)], (1, 0): t[(1, slot)]})


# ---- libjpeg's pixels ----------------------------------------------------------------------------------------------------------------
def upsample(s, rh, rv, rule="replicate4"):
    """int plane [ch, cw] -> [ch rv, cw rh].  "replicate4": replication in both directions where either ratio is 4, libjpeg_ref's
    filters elsewhere.  Planted: "filter2" -- where a ratio is 4, the direction whose ratio is 2 is still filtered; "by2" -- ratio 4
    replicated by 2 only (half the size)."""
    s = np.asarray(s, np.int32)
    if rh != 4 and rv != 4:
        return libjpeg_ref.upsample(s, rh, rv)
    if rule == "filter2":
        if rh == 2:
            s, rh = libjpeg_ref.upsample(s, 2, 1), 1
        elif rv == 2:
            s, rv = libjpeg_ref.upsample(s, 1, 2), 1
    if rule == "by2":
        rh, rv = min(rh, 2), min(rv, 2)
    return np.repeat(np.repeat(s, rv, axis=0), rh, axis=1)


def pixels_from_planes(planes, ratios, w, h, rule="replicate4"):
    """libjpeg_ref.pixels_from_planes with the rule above"""
    up = [upsample(p, rh, rv, rule)[:h, :w] for p, (rh, rv) in zip(planes, ratios)]
    assert all(u.shape == (h, w) for u in up), [u.shape for u in up]
    if len(up) == 1:
        return np.repeat(up[0][:, :, None], 3, axis=2).astype(np.uint8)
    y, cb, cr = up
    return np.stack([libjpeg_ref.channel_r(y, cr), libjpeg_ref.channel_g(y, cb, cr), libjpeg_ref.channel_b(y, cb)], axis=2).astype(np.uint8)


def libjpeg_pixels(data, dec, rule="replicate4"):
    w, h, pl, ratios = libjpeg_ref.component_planes(data, dec)
    return pixels_from_planes([libjpeg_ref.round_u8(p) for p in pl], ratios, w, h, rule)


def interval(data, dec, K=64):
    """libjpeg_ref.interval's construction on the rule above: every step behind the rounding is monotone in every sample (replication
    is, as the triangle filters are), so lo is the pipeline on round(w - delta) and hi on round(w + delta), chroma swapped for G."""
    w, h, pl, ratios = libjpeg_ref.component_planes(data, dec)
    _, _, mag, _ = libjpeg_ref.component_planes(data, dec, magnitude=True)
    R = libjpeg_ref
    lo = [upsample(R.round_u8(p - K * 2.0 ** -24 * m), rh, rv)[:h, :w] for p, m, (rh, rv) in zip(pl, mag, ratios)]
    hi = [upsample(R.round_u8(p + K * 2.0 ** -24 * m), rh, rv)[:h, :w] for p, m, (rh, rv) in zip(pl, mag, ratios)]
    if len(pl) == 1:
        return (np.repeat(lo[0][:, :, None], 3, axis=2).astype(np.uint8), np.repeat(hi[0][:, :, None], 3, axis=2).astype(np.uint8))
    out_lo = np.stack([R.channel_r(lo[0], lo[2]), R.channel_g(lo[0], hi[1], hi[2]), R.channel_b(lo[0], lo[1])], axis=2).astype(np.uint8)
    out_hi = np.stack([R.channel_r(hi[0], hi[2]), R.channel_g(hi[0], lo[1], lo[2]), R.channel_b(hi[0], hi[1])], axis=2).astype(np.uint8)
    return out_lo, out_hi


# ---- the packed picture, restated with planted errors ----------------------------------------------------------------------------------
def box_rgb(data, dec, plant=None):
    """scaled_ref.scaled_rgb at scale 1 restated from scaled_ref.planes, so that an error can be planted: "by2" -- a ratio of 4
    replicated as if it were 2 (sample X h / hmax with the ratio capped at 2); "mcu16" -- an MCU taken to be 16 pixels wide where it
    is 32 (pixel X reads MCU X / 16)."""
    w, h, comps, pl, hmax, vmax = scaled_ref.planes(data, 1, dec)
    X, Y = np.arange(w), np.arange(h)
    smp = []
    for (hc, vc, _), p in zip(comps, pl):
        rh, rv = hmax // hc, vmax // vc
        if plant == "by2":
            rh, rv = min(rh, 2), min(rv, 2)
        xs, ys = X // rh, Y // rv
        if plant == "mcu16" and hmax == 4:
            xs = (X // 16) * 8 * hc + (X % 16) // rh
        smp.append(p[np.minimum(ys, p.shape[0] - 1)[:, None], np.minimum(xs, p.shape[1] - 1)[None, :]])
    if len(smp) == 1:
        return scaled_ref.to_u8(np.repeat(smp[0][:, :, None], 3, axis=2))
    y, cb, cr = smp
    r = cr * (2 - 2 * 0.299) + y
    b = cb * (2 - 2 * 0.114) + y
    g = (y - 0.114 * b - 0.299 * r) / 0.587
    return scaled_ref.to_u8(np.stack([r, g, b], axis=2))

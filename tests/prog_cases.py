"""Inputs shared by the progressive tests (tests/test_progressive_host.py on the CPU, tests/test_progressive.py on the GPU): Pillow's
baseline / progressive twins, the constructed blocks and scan scripts of the writer (tests/progwriter.py), the damaged set, and the
binding of the host emulation (tests/emul/prog_emul.cpp)."""
import ctypes
import functools
import io
import os

import numpy as np
from PIL import Image

import jpegwriter
import progwriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _picture(w, h, mode, seed):
    """texture over a ramp: every band of every scan carries something"""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0, 120, w)[None, :] + np.linspace(0, 60, h)[:, None]
    if mode == "RGB":
        a = rng.integers(0, 70, (h, w, 3)) + ramp[:, :, None] * np.array([1.0, 0.6, 0.3])
    else:
        a = rng.integers(0, 70, (h, w)) + ramp
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), mode)


def twins_of(im, quality=75, subsampling=0, **kw):
    """(baseline, progressive) of one array at the same quality and subsampling: libjpeg codes identical coefficients.  The equality
    of Pillow's decodes of the two is re-asserted here, before anybody uses the pair."""
    out = []
    for prog in (False, True):
        b = io.BytesIO()
        k = dict(quality=quality, progressive=prog, **kw)
        if im.mode != "L":
            k["subsampling"] = subsampling
        im.save(b, "JPEG", **k)
        out.append(b.getvalue())
    a0, a1 = (np.asarray(Image.open(io.BytesIO(x)).convert("RGB")) for x in out)
    assert np.array_equal(a0, a1), "Pillow decodes the twins differently"
    assert b"\xff\xc2" in out[1] and b"\xff\xc2" not in out[0]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pillow_pair(w, h, mode, subsampling, quality=75, restart_blocks=0, restart_rows=0, seed=5):
    kw = {}
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    return twins_of(_picture(w, h, mode, seed), quality, subsampling, **kw)


# the five layouts of the issue: (name, width, height, mode, Pillow's subsampling code, restart_marker_blocks)
LAYOUTS = [("grey_23x31", 23, 31, "L", 0, 0), ("444_17x9", 17, 9, "RGB", 0, 0), ("422_33x40", 33, 40, "RGB", 1, 0),
           ("420_70x52", 70, 52, "RGB", 2, 0), ("420_56x40_rst3", 56, 40, "RGB", 2, 3)]
SIZES = [("1x1", 1, 1, "RGB", 2, 0), ("420_16x16", 16, 16, "RGB", 2, 0), ("grey_8x2000", 8, 2000, "L", 0, 0)]


def layout_pair(name, quality=75):
    _, w, h, mode, sub, rst = next(x for x in LAYOUTS + SIZES if x[0] == name)
    return pillow_pair(w, h, mode, sub, quality, rst)


def real_blocks(width, height, hv):
    """bool [MCUs * bpm]: the blocks (MCU-interleaved order) that lie inside their component's own grid -- the others exist only as
    MCU padding: a progressive file carries nothing of them beyond what an interleaved DC scan sends"""
    hv = [(1, 1)] if len(hv) == 1 else [tuple(x) for x in hv]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = []
    for m in range(mcux * mcuy):
        for h, v in hv:
            cbw, cbh = -(-(width * h) // (8 * hmax)), -(-(height * v) // (8 * vmax))
            for j in range(h * v):
                out.append((m % mcux) * h + j % h < cbw and (m // mcux) * v + j // h < cbh)
    return np.array(out)


def hv_of(data):
    """sampling factors of a file's frame header"""
    i = data.index(b"\xff\xc2") if b"\xff\xc2" in data else data.index(b"\xff\xc0")
    n = data[i + 9]
    return [(data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15) for c in range(n)]


# ---- constructed blocks and the writer's scripts -------------------------------------------------------------------------
WRITER_SHAPES = {"420_24x24": dict(hv=[(2, 2), (1, 1), (1, 1)], mcux=2, mcuy=2, width=24, height=24),
                 "grey_17x9": dict(hv=[(1, 1)], mcux=3, mcuy=2, width=17, height=9)}


def constructed_blocks(shape, seed=11):
    """int [MCUs * bpm, 64], zig-zag: values at +-1, +-2, +-3 around each Al (1, 2, 4: 1 .. 7 and their negatives); extremes +-1023
    (AC) and -1024 / 1016 (DC); coefficients born only in the last refinement (+-1); ZRL across non-zero history (a run of more than
    15 zero-history coefficients that passes over coefficients sent earlier); correction bits pending inside an end-of-band run
    (consecutive blocks whose only coefficients were all sent earlier)."""
    s = WRITER_SHAPES[shape]
    bpm = 1 if len(s["hv"]) == 1 else sum(h * v for h, v in s["hv"])
    n = s["mcux"] * s["mcuy"] * bpm
    rng = np.random.default_rng(seed)
    blocks = np.zeros((n, 64), np.int64)
    around = [v for a in (1, 2, 4) for d in (-3, -2, -1, 0, 1, 2, 3) if a + d > 0 for v in (a + d, -(a + d))]
    for i in range(n):
        kind = (i + i // bpm) % 6
        blk = blocks[i]
        blk[0] = [-1024, 1016][i & 1] if kind == 1 else int(rng.integers(-1024, 1017))
        if kind == 0:
            for k in rng.choice(np.arange(1, 64), 20, replace=False):
                blk[k] = around[int(rng.integers(len(around)))]
        elif kind == 1:
            for k in rng.choice(np.arange(1, 64), 6, replace=False):
                blk[k] = [1023, -1023][int(rng.integers(2))]
        elif kind == 2:
            for k in rng.choice(np.arange(1, 64), 24, replace=False):
                blk[k] = [1, -1][int(rng.integers(2))]
            blk[3], blk[17] = 9, -12
        elif kind == 3:
            blk[5], blk[30], blk[63] = 37, -20, [1, -1][i & 1]
        else:
            for k in range(1, 4 + kind):
                blk[k] = int(rng.integers(8, 200)) * [1, -1][int(rng.integers(2))]
    return blocks


def comp_of_blocks(shape):
    s = WRITER_SHAPES[shape]
    per = [0] if len(s["hv"]) == 1 else [c for c, (h, v) in enumerate(s["hv"]) for _ in range(h * v)]
    return per * (s["mcux"] * s["mcuy"])


def writer_scripts(shape):
    n = len(WRITER_SHAPES[shape]["hv"])
    out = {"spectral": progwriter.script_spectral(n), "successive": progwriter.script_successive(n), "libjpeg": progwriter.script_libjpeg(n),
           "dc_apart": progwriter.script_dc_apart(n), "al13": progwriter.script_al13(n), "stops_early": progwriter.script_stops_early(n)}
    if n == 1:
        out["single_coefficients"] = progwriter.script_single_coefficients()
    return out


QTS = {1: [[2] * 64], 3: [[2] * 64, [3] * 64, [3] * 64]}


@functools.lru_cache(maxsize=None)
def writer_case(shape, script):
    """-> (progressive file, baseline twin, blocks the decoder must hold [MCUs * bpm, 64], real-block mask)"""
    s = WRITER_SHAPES[shape]
    blocks = constructed_blocks(shape)
    sc = writer_scripts(shape)[script]
    qts = QTS[len(s["hv"])]
    prog = progwriter.progressive_from_blocks(blocks, sc, s["hv"], s["mcux"], s["mcuy"], qts, s["width"], s["height"])
    held = progwriter.masked_blocks(blocks, sc, comp_of_blocks(shape)) if script == "stops_early" else blocks
    base = jpegwriter.jpeg_from_blocks(held, s["hv"], s["mcux"], s["mcuy"], qts, jpegwriter._annex_k_tables(), width=s["width"], height=s["height"])
    return prog, base, held.astype(np.int16), real_blocks(s["width"], s["height"], s["hv"])


# ---- the damaged set ---------------------------------------------------------------------------------------------------------
def scan_spans(data):
    """[(first byte, end)] of every entropy-coded segment of a file"""
    out, i = [], 2
    while i + 4 <= len(data):
        assert data[i] == 0xff
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xd9:
            break
        i += 2 + ln
        if m == 0xda:
            k = i
            while not (data[k] == 0xff and data[k + 1] != 0 and not 0xd0 <= data[k + 1] <= 0xd7):
                k += 1
            out.append((i, k))
            i = k
    return out


def damaged_set(seed=3):
    """The 33x40 4:2:2 progressive file cut at every byte of its last 64 and at one byte inside every scan, and 200 seeded one-byte
    substitutions inside the scans -- any byte, any value: a substitution may make or break a marker or a stuffed pair, and the file
    may then be the parser's to refuse."""
    data = layout_pair("422_33x40")[1]
    spans = scan_spans(data)
    rng = np.random.default_rng(seed)
    out = [data[:len(data) - k] for k in range(1, 65)]
    out += [data[:int(rng.integers(a + 1, b))] for a, b in spans if b - a > 1]
    inside = [p for a, b in spans for p in range(a, b)]
    for k in range(200):
        p = inside[int(rng.integers(len(inside)))]
        v = 0xff if k % 25 == 0 else int(rng.integers(0, 256))         # (eight of them write 0xFF)
        v = v if v != data[p] else v ^ 0x10
        out.append(data[:p] + bytes([v]) + data[p + 1:])
    return out


# ---- the host emulation ------------------------------------------------------------------------------------------------------
_emul = None


def emul():
    global _emul
    if _emul is None:
        import __graft_entry__ as ge
        ge.build()
        _emul = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libprog_emul.so"))
        _emul.prog_emul_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        _emul.prog_emul_levels.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    return _emul


def emul_decode(data, cap=1 << 15):
    """-> (status, coefs [blocks, 64] or None, dict(width, height, bpm, mcus, levels, lanes))"""
    co = np.zeros((cap, 64), np.int16)
    info = (ctypes.c_uint32 * 6)()
    st = ctypes.c_int(0)
    rc = emul().prog_emul_decode(bytes(data), len(data), co.ctypes.data, cap, info, ctypes.byref(st))
    assert rc == 0, "more blocks than the buffer holds"
    inf = dict(zip(("width", "height", "bpm", "mcus", "levels", "lanes"), info))
    return st.value, (co[:inf["bpm"] * inf["mcus"]].copy() if st.value == 0 else None), inf


def emul_levels(data):
    lv = (ctypes.c_uint32 * 256)()
    n = emul().prog_emul_levels(bytes(data), len(data), lv, 256)
    return list(lv)[:n]

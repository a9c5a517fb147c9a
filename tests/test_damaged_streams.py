"""Damaged scans: which status a damaged picture gets and, where the decode goes on, which coefficients.

The expected result of every file is the serial decode of tests/damaged_ref.py -- one bit reader, one loop over the blocks, the band
rule for a scan that ends early.  Files are built here from tests/data/lena.jpeg and lena-bw.jpeg, from small pictures of
test_sampling_layouts.layout_file (4:2:0, 4:4:4, grey, and a 12-block MCU), from two of them re-coded with tables of
jpegwriter.huffman_shapes (`flat`: unmatched patterns of 2 bits, so entries of the 9-bit primary table itself are invalid;
`random4`: unmatched patterns of 4 to 10 bits) and from the restart fixtures of tests/golden/pil.

Families (family() lists them; test_coverage counts them):
  ends        the scan cut at every byte of its last 48, of its first 16 and at every 97th between, the end-of-image marker put
              back and a trailing FF dropped -- on four small sources whose scan lengths have the four residues mod 4; the last 13
              cuts on every other source; three named cuts that come out OK with other last blocks (lena-bw.jpeg less 3 and 6 bytes,
              2x2-chroma.jpeg less 1); three tails on which the verdict used to depend on the subsequence length;
              1, 3, 10 and 59 trailing bytes and a stuffed run of FF behind the last MCU (must stay OK)
  invalid     FF FF FF over six bytes, and the table's own unmatched pattern spliced in at a block's first bit, in the first, a
              middle and the last subsequence, inside the last block, and two in one file; FF FF FF behind the last block (OK)
  discarded   for every lane the emulated single decode reports as "first invalid code in front of the merge point" on the
              clean lena.jpeg, FF FF FF at three places of the part of the first decode that is kept -- at 1024, 2048 and 4096 bits
              without warm-up, a checkpoint every 256 bits
  subst       200 seeded single-byte replacements per source
  corner      the one case k_huff_prefix cannot decide and hands to the two-pass kernels: a lane whose first invalid code was
              discarded, and bytes behind the last MCU, in front of the scan's tail, with an unmatched pattern in them
  restart     an interval short by one block and one long by one block (ignored: the lane stops at the interval's last block),
              damage inside one interval, a missing and a doubled marker, 200 seeded single-byte replacements

CPU tests: the reference equals the oracle on every intact source and on every damaged file the oracle decodes; both emulated kernel
sequences (tests/emul) equal the reference in verdict and coefficients at the planned cut and at 256, 1024 and 2048 bits; three
planted errors in the reference are caught.  GPU tests: the whole family in batches of about 200 with intact pictures between,
through the batch API, mjx_decode_batch with device de-stuffing, and child processes with the single decode off and forced on.
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import damaged_ref as dr
import jpegwriter as jw
import oracle_binding as orc_mod
import test_huffman_tables as th
import test_sampling_layouts as sl

ROOT = sl.ROOT
DATA = os.path.join(ROOT, "tests", "data")
PIL = os.path.join(ROOT, "tests", "golden", "pil")
CUTS = (0, 256, 1024, 2048)                       # subsequence lengths the emulations run at (0: the planned one)
DISCARD_SETTINGS = [(1024, 0, 256), (2048, 0, 256), (4096, 0, 256)]      # (sub_base_bits, warm-up, cp_bits)
FF3 = b"\xff\xff\xff"


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def sources():
    """{name: bytes}: the intact files.  The four `ends` sources have scan lengths of residue 1, 0, 3 and 2 mod 4."""
    s = {"lena": _read(os.path.join(DATA, "lena.jpeg")), "lena-bw": _read(os.path.join(DATA, "lena-bw.jpeg")),
         "420": sl.layout_file("Y22_Cb11_Cr11", 256, 128)[0], "444": sl.layout_file("Y11_Cb11_Cr11", 136, 88)[0],
         "grey": sl.layout_file("gray21", 99, 77)[0], "mcu12": sl.layout_file("Y22_Cb22_Cr22", 64, 48)[0],
         "flat": th.recoded("Y22_Cb11_Cr11", 160, 96, "flat"), "random4": th.recoded("Y22_Cb11_Cr11", 160, 96, "random4")}
    for n in ("dri_444_r1", "dri_gray_r7", "dri_420_r5"):
        s[n] = _read(os.path.join(PIL, n + ".jpg"))
    return s


ENDS_SOURCES = ["420", "444", "grey", "mcu12"]
PLAIN_SOURCES = ["lena", "lena-bw", "420", "444", "grey", "mcu12", "flat", "random4"]
RESTART_SOURCES = ["dri_444_r1", "dri_gray_r7", "dri_420_r5"]


@functools.lru_cache(maxsize=None)
def picture(name):
    pic = dr.Picture(sources()[name] if name in sources() else _read(os.path.join(DATA, name)))
    assert pic.raw[-2:] == b"\xff\xd9"
    return pic


@functools.lru_cache(maxsize=None)
def clean(name):
    r = dr.decode(picture(name))
    assert r.verdict == dr.OK and r.complete, name
    return r


class Case:
    """name, family, source; data: the file; scan, rst: what the decode sees of it; ref: the serial decode's Result; sites: [(block, bit)]
    where an invalid code was planted by construction"""

    def __init__(self, name, fam, src, data, scan, rst, ref, sites=()):
        self.name, self.family, self.source, self.data, self.scan, self.rst, self.ref, self.sites = name, fam, src, data, scan, rst, ref, sites


def file_of(pic, body):
    """the picture's head, the entropy-coded bytes `body` (de-stuffed: every FF gets its 00) and the end-of-image marker"""
    return pic.head + dr.stuff(body) + b"\xff\xd9"


def make(name, fam, src, body, lo=None, hi=None, sites=()):
    """a damaged file of a source without restart intervals.  lo: first bit that differs from the source's scan (the reference starts
    there), hi: from this bit on the scans are the same again (same length), or None"""
    pic = picture(src)
    scan = bytes(body) + b"\xff\xd9"
    resume = None if lo is None else (clean(src), lo, hi)
    return Case(name, fam, src, file_of(pic, body), scan, [], dr.decode(pic, scan, [], resume=resume), sites)


def set_bits(body, bit, pattern):
    """`pattern` (a string of 0 and 1) written over the bits from `bit` on"""
    b = bytearray(body)
    for k, ch in enumerate(pattern):
        q = bit + k
        if q >> 3 < len(b):
            b[q >> 3] = (b[q >> 3] & ~(0x80 >> (q & 7))) | ((0x80 >> (q & 7)) if ch == "1" else 0)
    return bytes(b)


def ends_cases(src, cuts=None):
    pic = picture(src)
    body = pic.scan[:-2]
    n = len(body)
    if cuts is None:
        cuts = sorted(set(range(max(0, n - 48), n + 1)) | set(range(0, 17)) | set(range(16, n - 48, 97)))
    out = []
    for keep in cuts:
        b = body[:keep]
        if b.endswith(b"\xff"):
            b = b[:-1]
        out.append(make("%s cut to %d of %d" % (src, keep, n), "ends", src, b, lo=8 * len(b)))
    return out


# Tails found by search: with them the scan of `grey` ends 1 to 3 bytes behind a multiple of 32 bytes, the last symbol
# that starts in front of that multiple ends behind the scan's last bit, and the blocks the picture still needs lie in the band behind
# it.  The parent commit's lanes decoded them or not depending on where the scan was cut: OK at the planned cut, at 1024 and at 2048
# bits, TRUNCATED at 256 and 512.
BAND_TAILS = [(954, "4fe82c084a21"), (953, "5685c8b764ac"), (954, "09601cd77729")]


def band_cases():
    body = picture("grey").scan[:-2]
    return [make("grey cut to %d + %s" % (keep, tail), "ends", "grey", body[:keep] + bytes.fromhex(tail), lo=8 * keep) for keep, tail in BAND_TAILS]


# Found by search with the emulation: bytes behind the last MCU of `444` with FF FF FF in them, for which, at the subsequence length
# given and without warm-up, the lane that holds the picture's end has a wrong entry guess and a discarded invalid code in a block of
# the picture, and the run lies on the kept part behind the picture's last block, in front of the scan's tail.
CORNER_TAILS = [(1024, "fb49cff34945850a4fb5d2e45091d8c545e7e69af60dadb611363823eff0fcb893a5002f0496fb554a409b9c9ce42ba9b37f398db2ffffff87889b65ccaefd98624a"),
                (512, "fbbfa1fac3590ae2b9e2697993db2ab115d5c2f28052b4bfbcffffff547f6e1d01e1fd779741e4eeee54d9141956d0be21c95f4d15bf3acc627a6f986dc93a66a3936197d41e33174bef6067d6928ea73dbc9b720801f80b02aefba546a24f07bc825673c9"),
                (1024, "fed3532e4d50589bbc3256aabf0b250042d672d87070e36b2748d9c4516d4a8f6254cc581508823c603d867a7f31dbb831ee53a1fd21073a85751194cdb155062b97c7d1977a5de9565d195152e7fd6e3ea84ba6ffffffdc70b1920cb1fe")]


def corner_cases():
    body = picture("444").scan[:-2]
    out = []
    for k, (sub, tail) in enumerate(CORNER_TAILS):
        c = make("444 + corner tail %d at %d bits" % (k, sub), "corner", "444", body + bytes.fromhex(tail), lo=8 * len(body))
        c.setting = (sub, 0, 256)
        out.append(c)
    return out


def trailing_cases(src):
    body = picture(src).scan[:-2]
    rng = np.random.default_rng(len(body))
    out = []
    for k in (1, 3, 10, 59):
        extra = bytes(int(x) for x in rng.integers(0, 255, k))            # (no FF)
        out.append(make("%s + %d trailing bytes" % (src, k), "ends", src, body + extra, lo=8 * len(body)))
    out.append(make("%s + a stuffed run" % src, "ends", src, body + b"\xff" * 7, lo=8 * len(body)))
    return out


def subsequence_bytes(src):
    """[(label, first byte, last byte)]: the first, a middle and the last subsequence of the source's scan at 2048 bits"""
    n = len(picture(src).scan) - 2
    nsub = -(-n // 256)
    return [("first", 8, min(n, 256) - 8), ("middle", (nsub // 2) * 256 + 8, min(n, (nsub // 2 + 1) * 256) - 8), ("last", max(8, (nsub - 1) * 256), n - 8)]


def invalid_cases(src):
    pic, ref = picture(src), clean(src)
    body = pic.scan[:-2]
    out = []
    # FF FF FF over six bytes
    for label, b0, b1 in subsequence_bytes(src):
        q = (b0 + b1) // 2 if b1 - b0 > 8 else max(0, b0 - 8)
        out.append(make("%s FF run in the %s subsequence" % (src, label), "invalid", src, body[:q] + FF3 + body[q + 6:], lo=8 * q))
    for num in (1, 3, 5, 7):                                              # ... and at odd eighths of the scan
        q = len(body) * num // 8
        out.append(make("%s FF FF FF over three bytes at %d/8 of the scan" % (src, num), "invalid", src, body[:q] + FF3 + body[q + 3:], lo=8 * q, hi=8 * q + 24))
    q = int(ref.ends[-2]) // 8 + 1                                        # inside the last block
    out.append(make("%s FF run in the last block" % src, "invalid", src, body[:q] + FF3 + body[q + 3:], lo=8 * q, hi=8 * (q + 3)))
    out.append(make("%s FF run behind the last block" % src, "invalid", src, body + FF3, lo=8 * len(body)))
    # the table's own unmatched pattern at the first bit of a block: an invalid DC code whatever follows
    def dc_pattern(b):
        c, td, ta = pic.blocks_of_mcu[b % pic.bpm]
        return dr.unmatched_patterns(pic.dht[(0, td)])[0]
    def ac_pattern(b):
        c, td, ta = pic.blocks_of_mcu[b % pic.bpm]
        return dr.unmatched_patterns(pic.dht[(1, ta)])[0]
    picks = []
    for label, b0, b1 in subsequence_bytes(src):
        inside = np.nonzero((ref.ends >= 8 * b0) & (ref.ends < 8 * b1))[0]
        if len(inside):
            picks.append((label, int(inside[len(inside) // 2]) + 1))     # the block that starts there
    picks.append(("last block", pic.nblocks - 1))
    for label, b in picks:
        if b >= pic.nblocks:
            continue
        e = int(ref.ends[b - 1])
        pat = dc_pattern(b)
        out.append(make("%s unmatched DC pattern (%d bits) at block %d, %s" % (src, len(pat), b, label), "invalid", src,
                        set_bits(body, e, pat), lo=e, hi=e + len(pat), sites=((b, e),)))
    # ... and behind a block's DC symbol: an invalid AC code (the DC symbol of the clean stream stays)
    for label, b in picks[1:2]:
        c, td, ta = pic.blocks_of_mcu[b % pic.bpm]
        sym_t, len_t = dr.code_lookup(pic.dht[(0, td)])
        e = int(ref.ends[b - 1])
        w = int.from_bytes((pic.scan + b"\xaa" * 4)[e >> 3:(e >> 3) + 4], "big") >> (16 - (e & 7)) & 0xffff
        e2 = e + len_t[w] + sym_t[w]
        pat = ac_pattern(b)
        out.append(make("%s unmatched AC pattern (%d bits) in block %d" % (src, len(pat), b), "invalid", src, set_bits(body, e2, pat),
                        lo=e2, hi=e2 + len(pat), sites=((b, e2),)))
    # two in one file, in blocks far apart
    if len(picks) >= 2 and picks[0][1] + 4 < picks[-1][1]:
        b1, b2 = picks[0][1], picks[-1][1]
        e1 = int(ref.ends[b1 - 1])
        first = make("", "invalid", src, set_bits(body, e1, dc_pattern(b1)), lo=e1, hi=e1 + len(dc_pattern(b1)))
        if first.ref.complete and first.ref.ends[b2 - 1] == ref.ends[b2 - 1]:       # (the decode is back on the clean path at the second one)
            e2 = int(ref.ends[b2 - 1])
            both = set_bits(set_bits(body, e1, dc_pattern(b1)), e2, dc_pattern(b2))
            out.append(make("%s unmatched DC patterns at blocks %d and %d" % (src, b1, b2), "invalid", src, both, lo=e1, sites=((b1, e1), (b2, e2))))
    return out


def subst_cases(src, n=200):
    body = picture(src).scan[:-2]
    rng = np.random.default_rng([len(body), 200])
    out = []
    for k in range(n):
        q = int(rng.integers(0, len(body)))
        v = int(rng.integers(0, 256))
        if v == body[q]:
            v ^= 1 << int(rng.integers(0, 8))
        out.append(make("%s byte %d = %02x" % (src, q, v), "subst", src, body[:q] + bytes([v]) + body[q + 1:], lo=8 * q, hi=8 * q + 8))
    return out


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emul():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libhuff_emul.so"))
    lib.emul_decode_coefs_sub.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    lib.emul_single_decode_lanes.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                             ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t]
    return lib


VERDICT_OF = {0: dr.OK, 1: dr.TRUNCATED, 4: dr.BAD_HUFFMAN}            # MJX_OK, MJX_ERR_TRUNCATED, MJX_ERR_BAD_HUFFMAN (include/mjx.h)
_BUF = np.zeros((11000, 64), np.int16)


def emul_two_pass(data, sub=0, mode=0):
    _BUF.fill(0x5a5a)                                                # (what a call does not write must not pass for coefficients)
    nb, st = ctypes.c_size_t(), (ctypes.c_int * 8)()
    rc = emul().emul_decode_coefs_sub(data, len(data), 0, mode, sub, _BUF.ctypes.data, len(_BUF), ctypes.byref(nb), st)
    return rc, _BUF[:nb.value], list(st)


def emul_single(data, sub=0, warm=1024, cp=1024, mode=0, lanes=False):
    """-> (status, coefficients, stats[, lanes [nsub, 4], (bits per subsequence, subsequences, cp_bits, warm-up)])"""
    nb, st = ctypes.c_size_t(), (ctypes.c_int * 8)()
    ln = np.zeros((4096, 4), np.uint32) if lanes else None
    _BUF.fill(0x5a5a)
    rc = emul().emul_single_decode_lanes(data, len(data), 0, mode, sub, min(warm, sub) if sub else warm, 32, cp, _BUF.ctypes.data, len(_BUF),
                                         ctypes.byref(nb), st, ln.ctypes.data if lanes else None, 4096 if lanes else 0)
    if lanes:
        return rc, _BUF[:nb.value], list(st), ln[:st[0]].astype(np.int64), tuple(int(x) for x in ln[st[0]])
    return rc, _BUF[:nb.value], list(st)


def discarded_lanes(data, sub, warm, cp):
    """[(subsequence, position of the discarded code, merge point)] of the clean file, and the bits per subsequence"""
    rc, _, st, ln, cut = emul_single(data, sub, warm, cp, lanes=True)
    assert rc == 0 and st[6] == 0, (rc, st)
    none = 0xffffffff
    return [(s, int(a), int(pk)) for s, (a, pk, _, _) in enumerate(ln) if a != none and pk not in (0, none) and a < pk], cut[0]


def discarded_cases(src, settings):
    """for every such lane, FF FF FF at three places of the kept part of its first decode (behind the merge point, 64 bits in front of
    the subsequence's end at the latest)"""
    pic = picture(src)
    body = pic.scan[:-2]
    out = []
    for sub, warm, cp in settings:
        lanes, L = discarded_lanes(sources()[src], sub, warm, cp)
        for s, a, pk in lanes:
            end = min(L, 8 * len(body) - s * L)
            for frac in (0.25, 0.5, 0.75):
                q = (s * L + pk + int((end - pk - 64) * frac)) // 8
                if 8 * q < s * L + pk + 16 or q + 6 > len(body):
                    continue
                c = make("%s lane %d of %d bits (discarded code at %d, merge point %d): FF run at byte %d" % (src, s, L, a, pk, q), "discarded", src,
                         body[:q] + FF3 + body[q + 6:], lo=8 * q)
                c.setting, c.lane = (sub, warm, cp), s
                out.append(c)
    return out


# ---- restart intervals -------------------------------------------------------------------------------------------------------------
def restart_case(name, src, raw):
    pic = picture(src)
    scan, rst = dr.destuff(raw, True)
    return Case(name, "restart", src, pic.head + raw, scan, rst, dr.decode(pic, scan, rst))


def restart_cases(src):
    """the entropy-coded bytes cut apart at their RSTn markers and put together again"""
    pic = picture(src)
    raw = pic.raw[:-2]
    marks = [k for k in range(len(raw) - 1) if raw[k] == 0xff and (raw[k + 1] & 0xf8) == 0xd0]
    segs = [raw[a:b] for a, b in zip([0] + [k + 2 for k in marks], marks + [len(raw)])]
    mk = [raw[k:k + 2] for k in marks]
    look = {key: jw.huff_codes(*t) for key, t in pic.dht.items()}

    def join(segs_, mk_):
        return b"".join(s + m for s, m in zip(segs_, list(mk_) + [b""])) + b"\xff\xd9"

    def coded_blocks(g, blocks):
        """interval g coded again with only `blocks` of its blocks (a list of indices into the interval's blocks, repeats allowed)"""
        ref = clean(src)
        per = pic.restart * pic.bpm
        t0 = ref.t0[g * per:(g + 1) * per].astype(np.int64)
        owner = [pic.blocks_of_mcu[k % pic.bpm] for k in range(len(t0))]
        w, pred = jw.BitWriter(), {}
        for k in blocks:
            c, td, ta = owner[k]
            pred_k = 0
            for j in range(k - 1, -1, -1):                          # the interval's own prediction of this block, as the source codes it
                if owner[j][0] == c:
                    pred_k = int(t0[j, 0])
                    break
            s, bits = jw.magnitude(int(t0[k, 0]) - pred_k)
            w.put(*look[(0, td)][s]); w.put(bits, s)
            run, last = 0, max([i for i in range(1, 64) if t0[k, i]], default=0)
            for i in range(1, last + 1):
                if t0[k, i] == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*look[(1, ta)][0xf0]); run -= 16
                s, bits = jw.magnitude(int(t0[k, i]))
                w.put(*look[(1, ta)][(run << 4) | s]); w.put(bits, s)
                run = 0
            if last < 63:
                w.put(*look[(1, ta)][0x00])
        return w.flush()
    g = len(segs) // 2
    per = min(pic.restart * pic.bpm, pic.nblocks - g * pic.restart * pic.bpm)
    out = []
    short = coded_blocks(g, list(range(per - 1)))
    out.append(restart_case("%s interval %d short by one block" % (src, g), src, join(segs[:g] + [short] + segs[g + 1:], mk)))
    long_ = coded_blocks(g, list(range(per)) + [per - 1])
    out.append(restart_case("%s interval %d long by one block" % (src, g), src, join(segs[:g] + [long_] + segs[g + 1:], mk)))
    for k, (label, fill) in enumerate((("FF run", dr.stuff(FF3)), ("zeros", b"\x00" * 4), ("a changed byte", None))):
        gg = max(1, g - 1 + k)
        s = bytearray(segs[gg])
        q = len(s) // 2
        if fill is None:
            s[q] = (s[q] ^ 0x5a) if s[q] ^ 0x5a != 0xff and s[q] != 0xff and s[q - 1] != 0xff else s[q]
        else:
            while s[q - 1] == 0xff or (q + 3 < len(s) and s[q + 3] == 0x00 and s[q + 2] == 0xff):
                q += 1
            s[q:q + 3] = fill
        out.append(restart_case("%s %s inside interval %d" % (src, label, gg), src, join(segs[:gg] + [bytes(s)] + segs[gg + 1:], mk)))
    for gg in sorted(set(len(segs) * num // 9 for num in range(1, 9))):         # an FF run in eight intervals, one at a time
        sg = segs[gg]
        q = len(sg) // 3
        while q + 3 <= len(sg) and (sg[q - 1:q] == b"\xff" or sg[q + 3:q + 4] == b"\x00"):
            q += 1
        out.append(restart_case("%s FF run at a third of interval %d" % (src, gg), src, join(segs[:gg] + [sg[:q] + dr.stuff(FF3) + sg[q + 3:]] + segs[gg + 1:], mk)))
        out.append(restart_case("%s FF FF in front of interval %d" % (src, gg), src, join(segs[:gg] + [dr.stuff(b"\xff\xff") + sg] + segs[gg + 1:], mk)))
        if gg % 2 == 0:
            half = sg[:len(sg) // 2]
            half = half[:-1] if half.endswith(b"\xff") else half
            out.append(restart_case("%s interval %d cut to half" % (src, gg), src, join(segs[:gg] + [half] + segs[gg + 1:], mk)))
        if gg % 2:                                                           # bytes behind an interval's last block are not looked at
            out.append(restart_case("%s garbage behind interval %d" % (src, gg), src, join(segs[:gg] + [sg + bytes([0x5a, gg & 0x7f, 0xfe, 0x01])] + segs[gg + 1:], mk)))
    out.append(restart_case("%s marker %d missing" % (src, g), src, join(segs[:g] + [segs[g] + segs[g + 1]] + segs[g + 2:], mk[:g] + mk[g + 1:])))
    out.append(restart_case("%s marker %d doubled" % (src, g), src, join(segs[:g + 1] + [b""] + segs[g + 1:], mk[:g + 1] + [mk[g]] + mk[g + 1:])))
    # the scan's end: the last interval cut short byte by byte, and bytes behind it
    last = segs[-1]
    for cut in range(0, 9):
        b = last[:len(last) - cut]
        while b.endswith(b"\xff") or b.endswith(b"\xff\x00"):
            b = b[:-1] if b.endswith(b"\xff") else b[:-2]
        out.append(restart_case("%s last interval less %d bytes" % (src, cut), src, join(segs[:-1] + [b], mk)))
    out.append(restart_case("%s + 10 trailing bytes" % src, src, join(segs[:-1] + [last + bytes(range(1, 11))], mk)))
    # 200 single-byte replacements inside the intervals (no byte of or next to a marker or a stuffed FF, and no new FF)
    rng = np.random.default_rng([len(raw), 200])
    free = [k for k in range(1, len(raw) - 1) if 0xff not in raw[k - 1:k + 2]]
    for q in rng.choice(free, 200, replace=False):
        v = int(rng.integers(0, 255))
        v = v ^ 1 if v == raw[q] else v
        out.append(restart_case("%s byte %d = %02x" % (src, q, v), src, raw[:q] + bytes([v]) + raw[q + 1:] + b"\xff\xd9"))
    return out


# ---- the family ----------------------------------------------------------------------------------------------------------------------
NAMED_CUTS = [("lena-bw", 3), ("lena-bw", 6), ("2x2-chroma.jpeg", 1)]        # cuts that decode as OK with other last blocks than the clean file's


@functools.lru_cache(maxsize=None)
def family():
    """[Case], every family, in a fixed order"""
    out = []
    for src in PLAIN_SOURCES:
        n = len(picture(src).scan) - 2
        out += ends_cases(src) if src in ENDS_SOURCES else ends_cases(src, list(range(n - 12, n + 1)))
        out += trailing_cases(src)
        out += invalid_cases(src)
        out += subst_cases(src)
    for src, k in NAMED_CUTS:
        n = len(picture(src).scan) - 2
        if src not in PLAIN_SOURCES:
            out += ends_cases(src, [n - k])
    out += band_cases()
    out += corner_cases()
    out += discarded_cases("lena", DISCARD_SETTINGS)
    for src in RESTART_SOURCES:
        out += restart_cases(src)
    return out


def tally(cases):
    t = {}
    for c in cases:
        k = t.setdefault((c.source, c.family), {dr.OK: 0, dr.TRUNCATED: 0, dr.BAD_HUFFMAN: 0})
        k[c.ref.verdict] += 1
    return t


def test_coverage():
    """The coverage table, from the reference alone.  Every verdict has 8 members or more per source; the four `ends` sources' scan
    lengths have the four residues mod 4; the discarded-code family has 5 BAD_HUFFMAN members or more from 2 lanes per setting (17 in
    all); trailing bytes and damage behind the last block stay OK; a missing marker and a
    doubled one are TRUNCATED, an interval long by one block is OK, one short by a block is TRUNCATED on two sources of three.  The named cuts: the band rule
    leaves them OK with other coefficients than the clean file's (their last blocks are read from the end-of-image marker's bits,
    which the scan keeps, and from the band behind them); the exact rule would call the two of lena-bw.jpeg TRUNCATED, and
    2x2-chroma.jpeg's OK as well: its last block ends inside the marker's 16 bits."""
    cases = family()
    t = tally(cases)
    for key in sorted(t):
        print("%-12s %-10s OK %4d  TRUNCATED %4d  BAD_HUFFMAN %4d" % (key + tuple(t[key][v] for v in (dr.OK, dr.TRUNCATED, dr.BAD_HUFFMAN))))
    per_source = {}
    for (src, fam), k in t.items():
        for v, n in k.items():
            per_source.setdefault(src, {}).setdefault(v, 0)
            per_source[src][v] += n
    for src in PLAIN_SOURCES + RESTART_SOURCES:
        assert all(per_source[src][v] >= 8 for v in (dr.OK, dr.TRUNCATED, dr.BAD_HUFFMAN)), (src, per_source[src])
    assert sorted(len(picture(s).scan) % 4 for s in ENDS_SOURCES) == [0, 1, 2, 3]
    disc = [c for c in cases if c.family == "discarded"]
    for setting in DISCARD_SETTINGS:
        mine = [c for c in disc if c.setting == setting and c.ref.verdict == dr.BAD_HUFFMAN]
        assert len(mine) >= 5 and len({c.lane for c in mine}) >= 2, (setting, len(mine))
    # (one of the 18 is OK: at 4096 bits one of the lanes is the scan's last, and its third place lies behind the picture's last block)
    assert sum(c.ref.verdict == dr.BAD_HUFFMAN for c in disc) >= 6 and all(c.ref.verdict in (dr.BAD_HUFFMAN, dr.OK) for c in disc)
    for c in cases:
        if "trailing bytes" in c.name or "stuffed run" in c.name or "behind the last block" in c.name or "long by one block" in c.name:
            assert c.ref.verdict == dr.OK and np.array_equal(c.ref.t0, clean(c.source).t0), c.name
        if "missing" in c.name or "doubled" in c.name:
            assert c.ref.verdict == dr.TRUNCATED, c.name
        if "short by one block" in c.name:
            # (the band rule: a last block of a few bits can be read from the first bits of the interval behind -- dri_444_r1, whose
            # intervals are one MCU of 15 bytes, comes out OK with a wrong last block in that interval; the two others are TRUNCATED)
            print(c.name, c.ref.verdict)
            if c.source == "dri_444_r1":
                pic, g = picture(c.source), int(c.name.split("interval ")[1].split()[0])
                last = (g + 1) * pic.restart * pic.bpm - 1
                assert c.ref.verdict == dr.OK and not np.array_equal(c.ref.t0[last], clean(c.source).t0[last]), c.name
                assert np.array_equal(c.ref.t0[:last], clean(c.source).t0[:last]), c.name
            else:
                assert c.ref.verdict == dr.TRUNCATED, c.name
    # a primary entry of the 9-bit table is invalid: `flat` has unmatched patterns of 2 bits, and cases that meet them
    assert min(len(p) for t in picture("flat").dht.values() for p in dr.unmatched_patterns(t)) < 9
    assert sum(1 for c in cases if c.source == "flat" and c.sites and c.ref.verdict == dr.BAD_HUFFMAN) >= 4
    assert sum(1 for c in cases if len(c.sites) == 2 and c.ref.verdict == dr.BAD_HUFFMAN) >= 4
    # substitutions: a valid stream with other coefficients, too few blocks, too many blocks (the picture's last block ends a byte or
    # more in front of where the clean file's does), an invalid code -- each occurs, without and with restart intervals
    for restart in (False, True):
        sub = [c for c in cases if ("byte " in c.name and " = " in c.name) and (c.source in RESTART_SOURCES) == restart]
        other = sum(c.ref.verdict == dr.OK and not np.array_equal(c.ref.t0, clean(c.source).t0) for c in sub)
        few = sum(c.ref.verdict == dr.TRUNCATED for c in sub)
        many = sum(c.ref.complete and c.ref.ends[-1] + 8 <= clean(c.source).ends[-1] for c in sub)
        inval = sum(c.ref.verdict == dr.BAD_HUFFMAN for c in sub)
        print("substitutions (restart intervals: %s): %d, other coefficients %d, too few blocks %d, too many %d, invalid code %d" % (restart, len(sub), other, few, many, inval))
        assert len(sub) == 200 * (len(RESTART_SOURCES) if restart else len(PLAIN_SOURCES)) and min(other, few, many, inval) >= 1
    assert not any(c.family == "corner" and c.ref.verdict != dr.OK for c in cases) and sum(c.family == "corner" for c in cases) == 3
    for c in cases:
        if c.source == "grey" and " + " in c.name and "cut to" in c.name:
            assert c.ref.verdict == dr.OK and c.ref.ends[-1] > 8 * len(c.scan) and (len(c.scan) % 32) in (1, 2, 3), c.name
    assert len(gpu_groups(cases)) == N_GROUPS
    for src, k in NAMED_CUTS:
        pic = picture(src)
        n = len(pic.scan) - 2
        c, = [c for c in cases if c.name == "%s cut to %d of %d" % (src, n - k, n)]
        exact = dr.decode(pic, c.scan, [], rule="exact")
        print(c.name, "band rule:", c.ref.verdict, "exact rule:", exact.verdict, "last block ends at bit", int(c.ref.ends[-1]), "of", 8 * len(c.scan))
        assert c.ref.verdict == dr.OK and not np.array_equal(c.ref.t0, clean(src).t0), c.name
        assert exact.verdict == (dr.OK if src == "2x2-chroma.jpeg" else dr.TRUNCATED), c.name


def test_the_files_are_what_the_reference_decoded(mjx):
    """Every case's file de-stuffs to the scan its reference result was computed over (damaged_ref.destuff), and the project's parser
    hands out the same bytes and restart offsets."""
    for c in family():
        pic = dr.Picture(c.data)
        assert pic.scan == c.scan and pic.rst == c.rst, c.name
        try:
            s = mjx.ParsedScan(c.data)
        except mjx.MjxError:
            assert False, c.name
        try:
            assert s.scan_bytes() == c.scan, c.name
            assert [s.desc.restart_offsets[k] for k in range(s.desc.n_restart)] == c.rst, c.name
        finally:
            s.close()


def test_reference_shortcuts_change_nothing():
    """damaged_ref.decode(resume=...) -- blocks in front of the damage taken from the clean decode, the rest taken from it once the two
    decodes are in the same state -- gives what the plain loop gives: every 7th case of the families that use it."""
    n = 0
    for c in family()[::7]:
        if c.family == "restart":
            continue
        full = dr.decode(picture(c.source), c.scan, c.rst)
        assert full.verdict == c.ref.verdict and full.complete == c.ref.complete and full.invalid == c.ref.invalid, c.name
        assert np.array_equal(full.t0, c.ref.t0) and np.array_equal(full.ends, c.ref.ends), c.name
        n += 1
    assert n > 100


def oracle_t0(data, restart):
    try:
        return orc_mod.interleave(orc_mod.decode(data, layout=orc_mod.LAYOUT_STD, ext_1bit=True, ext_dri=restart))
    except orc_mod.OracleError:
        return None


def test_reference_equals_the_oracle(orc):
    """On every intact source, and on every damaged file that the oracle decodes and whose needed blocks all end inside the scan
    (there the oracle reads the same bits): the same T0."""
    for src in PLAIN_SOURCES + RESTART_SOURCES + ["2x2-chroma.jpeg"]:
        data = sources().get(src) or _read(os.path.join(DATA, src))
        assert np.array_equal(clean(src).t0, oracle_t0(data, src in RESTART_SOURCES)), src
    n = 0
    for c in family():
        if not c.ref.complete or c.ref.invalid or c.ref.ends[-1] > 8 * len(c.scan) or c.family == "restart":
            continue
        want = oracle_t0(c.data, False)
        if want is not None:
            assert np.array_equal(c.ref.t0, want), c.name
            n += 1
    print("damaged files the oracle decodes:", n)
    assert n > 500


def emulation_problems(c, cuts=CUTS):
    """what the two emulated kernel sequences get wrong on a case: verdict, and T0 wherever the decode went to the end"""
    bad = []
    want = c.ref
    for sub in cuts:
        for kind in ("two-pass", "single"):
            if kind == "two-pass":
                rc, coefs, st = emul_two_pass(c.data, sub)
            else:
                setting = getattr(c, "setting", None)
                rc, coefs, st = emul_single(c.data, sub, 1024, 1024) if setting is None or sub else emul_single(c.data, *setting)
                if c.family == "corner" and not sub and st[6] != 16:
                    bad.append((c.name, kind, setting, "the corner is not reached", st[6]))
                if c.family == "corner" and st[6] == 16:
                    continue                                       # (the device hands the picture to the two-pass kernels: the corner, and only there)
            if st[6] not in (0, 1, 3, 15):                         # (14, 16: a fall-back no other file may take; the rest: an inconsistency)
                bad.append((c.name, kind, sub, "internal code", st[6]))
            elif VERDICT_OF.get(rc) != want.verdict:
                bad.append((c.name, kind, sub, "verdict", rc, st[6], want.verdict))
            elif rc != 1 and not np.array_equal(coefs, want.t0):
                bad.append((c.name, kind, sub, "T0", rc, st[6]))
    return bad


@pytest.mark.parametrize("fam", ["ends", "invalid", "discarded", "subst", "corner"])
def test_emulated_kernels_equal_the_reference(fam):
    """Both kernel sequences on the CPU, at the planned cut and at 256, 1024 and 2048 bits (the discarded-code cases also at the
    setting they were made for): the reference's verdict, and its coefficients wherever the decode goes to the last block --
    pictures with invalid codes included.  No emulated configuration reports an index out of range.
    A fall-back to the two-pass kernels (codes 14 and 16) counts as a failure on every file but the three of the corner family, which must
    report 16 at their setting; any other internal code is a failure too, and the output buffer is filled with a sentinel before each
    call, so coefficients a call did not write cannot pass.
    On the emulation of the parent commit the discarded-code family failed: the single decode said OK where the reference says
    BAD_HUFFMAN (17 of 17 cases); the three `grey cut to ... + ...` files were TRUNCATED at 256 bits and OK at the other cuts."""
    bad = []
    for c in family():
        if c.family == fam:
            bad += emulation_problems(c)
    assert bad == [], (len(bad), bad[:12])


PLANTS = [("first invalid code only", dict(first_invalid_only=True)), ("a block counts when it starts inside the scan", dict(rule="start")),
          ("an invalid code consumes the whole window", dict(invalid_takes_window=True))]


@pytest.mark.parametrize("what,kw", PLANTS)
def test_planted_errors_are_caught(what, kw):
    """Each planted error in the reference makes a case fail: its verdict, its coefficients or the invalid codes it must record differ
    from what the emulated kernels give / from the codes planted by construction."""
    caught = []
    for c in family():
        if c.family not in ("ends", "invalid") or c.source in ("lena", "lena-bw", "2x2-chroma.jpeg"):
            continue
        r = dr.decode(picture(c.source), c.scan, c.rst, **kw)
        rc, coefs, st = emul_two_pass(c.data)
        if VERDICT_OF.get(rc) != r.verdict or (rc != 1 and not np.array_equal(coefs, r.t0)) or not set(c.sites) <= set(r.invalid):
            caught.append(c.name)
    print(what, "fails", len(caught), "cases, e.g.", caught[:3])
    assert caught, what


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
STATUS_OF = {dr.OK: 0, dr.TRUNCATED: 1, dr.BAD_HUFFMAN: 4}
GROUP = 200
N_GROUPS = 17                                     # len(gpu_groups(family())): test_coverage checks it


def gpu_groups(cases):
    """the cases in groups of about GROUP pictures, an intact source in front of every 8 damaged ones: [[(data, status, T0 or None, name)]]"""
    rows = []
    for k, c in enumerate(cases):
        if k % 8 == 0:
            src = c.source if c.source in sources() else "lena-bw"
            rows.append((sources()[src], 0, clean(src).t0, "intact " + src))
        rows.append((c.data, STATUS_OF[c.ref.verdict], c.ref.t0 if c.ref.verdict == dr.OK else None, c.name))
    return [rows[k:k + GROUP] for k in range(0, len(rows), GROUP)]


_EMULATED = set()


def emulated_first(cases):
    """every file goes through the emulation at the planned cut before a GPU test sees it (restart files: the emulation has none)"""
    for c in cases:
        if c.family != "restart" and c.name not in _EMULATED:
            bad = emulation_problems(c, cuts=(0,))
            assert bad == [], bad
            _EMULATED.add(c.name)


@pytest.fixture(scope="module")
def prepared():
    """the family and its run through the emulation, once per session and outside the GPU tests' own time"""
    cases = family()
    emulated_first(cases)
    return cases


def group_problems(mjx, b, rows, status=None):
    bad, ncoefs = [], 0
    for i, (data, want, t0, name) in enumerate(rows):
        got = b.status(i) if status is None else status[i]
        if got != want:
            bad.append((name, "status", got, want))
        elif t0 is not None:
            ncoefs += 1
            if not np.array_equal(b.coefs(i), t0):
                bad.append((name, "T0"))
    print("%d statuses and %d coefficient streams compared" % (len(rows), ncoefs))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("g", range(N_GROUPS))
@pytest.mark.parametrize("door", ["batch", "decode_batch", "device_destuff"])
def test_family_on_the_device(mjx, gpu_ctx, prepared, door, g):
    """The whole family in heterogeneous batches of about 200, intact pictures between the damaged ones: every picture's status is the
    reference's verdict, coefs(i) the reference's T0 wherever the API hands coefficients out (status OK), the intact neighbours
    included -- through the batch API on parsed scans, through mjx_decode_batch, and through mjx_decode_batch with the scans
    de-stuffed on the device."""
    cases = prepared
    bad, unconverged = [], 0
    for rows in gpu_groups(cases)[g:g + 1]:
        datas = [r[0] for r in rows]
        if door == "batch":
            b, scans = sl.decode_batch(mjx, gpu_ctx, datas, keep_coefs=True)
            st = None
        else:
            b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=door == "device_destuff", keep_coefs=True)
            scans = []
        try:
            bad += group_problems(mjx, b, rows, st)
            if st is not None:
                bad += [(r[3], "status of the batch", b.status(i), st[i]) for i, r in enumerate(rows) if b.status(i) != st[i]]
            unconverged += b.unconverged_runs()
        finally:
            sl.close_all(b, scans)
    print("unconverged runs:", unconverged)
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
    scans = [mjx.ParsedScan(open(p, 'rb').read()) for p in paths]
    b = mjx.Batch(ctx, scans, keep_coefs=True)
    b.kernel_ms(reset=True)
    b.decode(); b.wait()
    k = b.kernel_ms()
    st = [b.status(i) for i in range(len(paths))]
    sha = [hashlib.sha1(b.coefs(i).tobytes()).hexdigest() if s == 0 else None for i, s in enumerate(st)]
    res.append(dict(status=st, sha=sha, emit=k['huff_emit'][1], write=k['huff_write'][1], prefix=k['huff_prefix'][1],
                    unconverged=b.unconverged_runs(), subsequences=b.geometry()['subsequences']))
    b.close()
    for s in scans:
        s.close()
print(json.dumps(res))
"""


def run_child(tmp_path, tag, groups, env_set):
    """groups of files, each one batch in a fresh process with `env_set` (a context with the throughput plan: 4096-bit subsequences
    whatever the batch's size) -> per group dict(status, sha of coefs, emit / write / prefix launches, unconverged, subsequences)"""
    job = dict(groups=[])
    for g, datas in enumerate(groups):
        paths = []
        for i, d in enumerate(datas):
            p = tmp_path / ("%s_%d_%d.jpg" % (tag, g, i))
            p.write_bytes(d)
            paths.append(str(p))
        job["groups"].append(paths)
    (tmp_path / (tag + ".json")).write_text(json.dumps(job))
    script = tmp_path / (tag + ".py")
    script.write_text(_CHILD % dict(root=ROOT, job=str(tmp_path / (tag + ".json"))))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def child_problems(rows, res):
    bad = []
    for i, (data, want, t0, name) in enumerate(rows):
        if res["status"][i] != want:
            bad.append((name, "status", res["status"][i], want))
        elif t0 is not None and res["sha"][i] != hashlib.sha1(np.ascontiguousarray(t0).tobytes()).hexdigest():
            bad.append((name, "T0"))
    return bad


EMIT_ENV = {"MJX_EMIT_MIN_SUB_BITS": "256", "MJX_EMIT_CP_BITS": "256", "MJX_EMIT_WARM_BITS": "0"}


@pytest.mark.gpu
def test_family_with_the_single_decode_off(mjx, prepared, tmp_path):
    """MJX_SINGLE_DECODE=0 in a child process: the two-pass kernels alone (k_huff_emit never runs, k_huff_write does) give the
    reference's statuses and coefficients."""
    cases = prepared
    groups = gpu_groups(cases)
    res = run_child(tmp_path, "off", [[r[0] for r in rows] for rows in groups], {"MJX_SINGLE_DECODE": "0"})
    bad = [p for rows, r in zip(groups, res) for p in child_problems(rows, r)]
    print("unconverged runs:", sum(r["unconverged"] for r in res))
    assert sum(r["emit"] for r in res) == 0 and all(r["write"] > 0 for r in res), [(r["emit"], r["write"]) for r in res]
    assert bad == [], (len(bad), bad[:12])


@pytest.mark.gpu
def test_family_with_the_single_decode_forced(mjx, prepared, tmp_path):
    """MJX_EMIT_MIN_SUB_BITS=256 MJX_EMIT_CP_BITS=256 MJX_EMIT_WARM_BITS=0 in a child process: every picture without restart
    intervals takes the emitting pass (k_huff_emit launches are counted) with no warm-up, so lanes start from wrong guesses and
    k_huff_prefix decides on their invalid codes.  The subsequence length the device planned is read back from a batch of the clean
    lena.jpeg, the emulation finds the discarded-code lanes of that cut, and the discarded-code cases are made again for it: the
    damage sits where the device's lanes have their merge points."""
    lena = sources()["lena"]
    probe, = run_child(tmp_path, "probe", [[lena]], EMIT_ENV)
    assert probe["status"] == [0] and probe["emit"] > 0, probe
    base = [b for b in (256, 512, 1024, 2048, 4096, 8192) if emul_single(lena, b, 0, 256)[2][0] == probe["subsequences"]]
    assert base, probe
    lanes, L = discarded_lanes(lena, base[0], 0, 256)
    print("the device cuts lena.jpeg into %d subsequences of %d bits; discarded-code lanes at that cut: %s" % (probe["subsequences"], L, lanes))
    mine = discarded_cases("lena", [(base[0], 0, 256)])
    # (a place behind the picture's last block, in a lane of the scan's end, stays OK)
    assert len(lanes) >= 1 and len(mine) >= 3 * len(lanes) and sum(c.ref.verdict == dr.BAD_HUFFMAN for c in mine) >= 3
    assert all(c.ref.verdict in (dr.BAD_HUFFMAN, dr.OK) for c in mine)
    emulated_first(mine)
    cases = mine + prepared
    groups = gpu_groups(cases)
    res = run_child(tmp_path, "emit", [[r[0] for r in rows] for rows in groups], EMIT_ENV)
    bad = [p for rows, r in zip(groups, res) for p in child_problems(rows, r)]
    print("unconverged runs:", sum(r["unconverged"] for r in res), "huff_emit launches:", sum(r["emit"] for r in res),
          "huff_prefix launches:", sum(r["prefix"] for r in res))
    assert bad == [], (len(bad), bad[:12])
    plain = [any(not r[3].startswith(("dri_", "intact dri_")) for r in rows) for rows in groups]      # (restart pictures take the two-pass kernels)
    assert all(r["emit"] > 0 for r, p in zip(res, plain) if p) and res[0]["prefix"] > 0, [(r["emit"], r["prefix"]) for r in res]


@pytest.mark.gpu
def test_a_truncated_picture_leaves_the_callers_memory_alone(mjx, gpu_ctx, prepared):
    """Pictures decoded into caller-owned memory filled with a guard byte: the slots of the truncated ones are untouched, their
    neighbours are complete (the intact file's pixels)."""
    import test_output_formats as tof
    pic = picture("420")
    cuts = [c for c in family() if c.source == "420" and c.family == "ends" and c.ref.verdict == dr.TRUNCATED][:6:2]
    assert len(cuts) == 3
    good = sources()["420"]
    datas = [good, cuts[0].data, good, cuts[1].data, cuts[2].data, good]
    per, guard = pic.height * pic.width * 3, 4096
    total = guard + len(datas) * per + guard
    hip = tof._hip(mjx)
    base = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(base), total) == 0
    try:
        assert hip.hipMemset(base, 0x5a, total) == 0 and hip.hipDeviceSynchronize() == 0
        dst = [(base.value + guard + i * per, pic.width, pic.height, 3 * pic.width, 0) for i in range(len(datas))]
        b, st = mjx.decode_batch(gpu_ctx, datas, output=mjx.Output("uint8", dst=dst))
        try:
            assert st == [0, 1, 0, 1, 1, 0], st
            mem = np.empty(total, np.uint8)
            assert hip.hipMemcpy(mem.ctypes.data, base, total, 2) == 0
        finally:
            b.close()
    finally:
        hip.hipFree(base)
    assert np.all(mem[:guard] == 0x5a) and np.all(mem[-guard:] == 0x5a)
    want = sl.oracle_std(good).rgb
    for i, code in enumerate(st):
        got = mem[guard + i * per:guard + (i + 1) * per].reshape(pic.height, pic.width, 3)
        if code:
            assert np.all(got == 0x5a), i
        else:
            assert sl.rgb_problem(got, want) is None, i

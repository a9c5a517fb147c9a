"""Device-side de-stuffing and the marker scan on constructed byte streams.

The upload-time kernels (k_destuff_count, k_destuff_prefix, k_destuff_scatter, k_restart_geometry, k_scan_interleave) are the only
ones whose correctness hangs on fixed byte boundaries of the raw input: 64-byte pieces (a lane), 4 KiB (a wave), 16 KiB (a
workgroup), 256 workgroups (a trip of the prefix kernel).  In natural pictures an FF 00 pair meets such a boundary by chance.  Here
every pattern is put on every boundary on purpose.

The reference is destuff_ref: the single-scan rule of mjx_parse.cpp::read_sos (jpeg/mod.rs:371-385 plus the restart extension)
restated in plain Python.  The per-piece rule the kernels run (destuff_keep_mask, mjx_kernels.h) runs on the CPU through
emul_destuff (tests/emul), which does serially what the three kernels do.

The byte-aligned alphabet.  With these two Huffman tables every symbol and every value is whole bytes, so the entropy-coded bytes
follow directly from the blocks handed to jpegwriter.jpeg_from_blocks:
  DC  twelve 8-bit codes: the code byte of size s is s; only sizes 0 (byte 00) and 8 (08 vv) are used
  AC  thirteen 4-bit codes that are never used, 47 8-bit codes D0..FE -- EOB = D0, (run 0, size 8) = D1 -- and one 16-bit code,
      FF00 = (run 2, size 8)
  values of size 8: +255 is the byte FF (stuffed to FF 00), -255 is 00, +128..+254 are 80..FE, -254..-128 are 01..7F
A block is (1 or 2) + 2 k + (1 if k < 63) bytes: every length from 2 to 127.  FF is a value byte only (or the first byte of the
16-bit code), so two stuffed pairs stand side by side, FF 00 FF 00, exactly where the value +255 is followed by the code FF00.

What a valid entropy-coded segment cannot hold: a run of FF 00 pairs that fills a 64-byte piece would be 256 one-bits in a row, and
every code has a zero bit and a symbol is at most 16 + 11 bits.  Such runs are therefore placed on every boundary in byte streams
that are not decodable (_byte_stream below: host parser, device rule and reference, on the CPU); the decodable files carry every
other pattern, and the long scan without restart intervals is as dense in FF 00 as a scan gets (about two kept bytes in three).

Families (all greyscale, q = 1; FAMILIES):
  place, place_rst   every (pattern, split) over a piece, a wave and a workgroup boundary, without / with restart intervals
  ends, ends_rst     raw lengths = 0, 1, 2, 63 (mod 64) and 0, 1 (mod 16384); a final FF 00 whose 00 is alone in the last workgroup;
                     a de-stuffed length that is a multiple of every subsequence length
  ladder             DRI 12, interval i exactly 24 + i bytes after de-stuffing, 1300 consecutive lengths; ladder_short: 64 of them
  long               two scans of more than 256 workgroups (k_destuff_prefix's second trip), with and without restart intervals
For every family the cases it hits are computed from the files' own bytes and asserted (coverage, test_constructed_files_cover_what_they_claim), not assumed.
"""
import concurrent.futures
import ctypes
import functools
import itertools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import jpegwriter as jw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE, WAVE, WG = 64, 4096, 16384


# ---- 1. the reference: a plain restatement ---------------------------------------------------------------------------------------------
def destuff_ref(body, restarts, dropped=None):
    """The single-scan rule, front to back -> (de-stuffed bytes, [output length at every restart marker]).  FF 00 -> FF; with
    restart intervals FF Dn -> nothing; any other FF x keeps the FF and looks at x again; a lone FF as the last byte stays.
    dropped: a list that receives the raw index of every byte that is not copied (counts_ref)."""
    out, offs, i, n = bytearray(), [], 0, len(body)
    dropped = [] if dropped is None else dropped
    while i < n:
        j = body.find(b"\xff", i)
        if j < 0:
            j = n
        out += body[i:j]                                   # bytes other than FF are copied
        if j >= n:
            break
        if j + 1 < n and body[j + 1] == 0x00:
            out.append(0xff)
            dropped.append(j + 1)
            i = j + 2
        elif restarts and j + 1 < n and 0xd0 <= body[j + 1] <= 0xd7:
            offs.append(len(out))
            dropped += (j, j + 1)
            i = j + 2
        else:
            out.append(0xff)
            i = j + 1
    return bytes(out), offs


def _local_masks(body, restarts, wrong=0, pad=0xd0):
    """(bytes, keep flags, marker flags) of the per-byte rule, see destuff_local"""
    b = np.frombuffer(bytes(body), np.uint8).astype(np.int16)
    n = len(b)
    i = np.arange(n)
    prev = np.concatenate([[0], b[:-1]])
    nxt = np.concatenate([b[1:], [pad if wrong == 3 else 0]])
    if wrong == 1:
        prev[i % PIECE == 0] = 0
    if wrong == 2:
        nxt[i % PIECE == PIECE - 1] = 0
    keep = ~((b == 0) & (prev == 0xff))
    marker = np.zeros(n, bool)
    if restarts:
        marker = (b == 0xff) & ((nxt & 0xf8) == 0xd0)
        keep &= ~marker & ~(((b & 0xf8) == 0xd0) & (prev == 0xff))
    return b, keep, marker


def destuff_local(body, restarts, wrong=0, pad=0xd0):
    """The same rule said per byte, as a piecewise implementation must say it: byte i goes if it is the 00 behind an FF, if it is an
    FF in front of Dn (a marker: the output length is recorded) or the Dn behind an FF -- the last two with restart intervals only,
    and no marker begins at the scan's last byte.  wrong = 0 is the rule (asserted equal to destuff_ref wherever it is used).
    Three deliberately wrong variants show that the constructed inputs tell them apart:
      1  the predecessor is forgotten at each piece start
      2  the byte behind the piece reads as 0
      3  a marker is accepted without the end-of-scan bound (the byte behind the scan, `pad`, is looked at)"""
    if len(body) == 0:
        return b"", []
    b, keep, marker = _local_masks(body, restarts, wrong, pad)
    return b[keep].astype(np.uint8).tobytes(), [int(v) for v in np.cumsum(keep)[marker]]


# ---- the device rule on the CPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(mjx):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libhuff_emul.so"))
    lib.emul_destuff.restype = ctypes.c_long
    lib.emul_destuff.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    return lib


def emul_destuff(lib, body, restarts, pad=0xd0):
    """-> (de-stuffed bytes, [marker offsets], [(bytes kept, markers)] per 16 KiB workgroup)"""
    body = bytes(body)
    n, nseg = len(body), (len(body) + WG - 1) // WG
    out, rst, seg, nr = np.empty(n + 64, np.uint8), np.empty(n // 2 + 8, np.uint32), np.empty(2 * nseg + 2, np.uint32), ctypes.c_uint32()
    got = lib.emul_destuff(body, n, int(restarts), int(pad), out.ctypes.data, len(out), rst.ctypes.data, len(rst), seg.ctypes.data, ctypes.byref(nr))
    assert got >= 0, got                                   # (-2: the counting and the scattering pass disagree)
    return out[:got].tobytes(), rst[:nr.value].tolist(), list(zip(seg[0:2 * nseg:2].tolist(), seg[1:2 * nseg:2].tolist()))


def counts_ref(body, dropped):
    """[(bytes kept, markers begun)] per 16 KiB of raw bytes, from the raw indices of the bytes the reference did not copy: a
    workgroup keeps its raw bytes less the dropped ones among them, and a dropped FF is the first byte of a marker"""
    d = np.asarray(dropped, np.int64)
    nseg = (len(body) + WG - 1) // WG
    size = np.minimum(WG, len(body) - WG * np.arange(nseg))
    ff = d[np.frombuffer(bytes(body), np.uint8)[d] == 0xff]
    return list(zip((size - np.bincount(d // WG, minlength=nseg)).tolist(), np.bincount(ff // WG, minlength=nseg).tolist()))


def check_rule(lib, body, restarts, pads=(0xd0,)):
    """emul_destuff == destuff_ref in bytes, marker offsets and per-workgroup counts; returns the reference's answer"""
    dropped = []
    want = destuff_ref(body, restarts, dropped)
    counts = counts_ref(body, dropped)
    assert sum(c[0] for c in counts) == len(want[0]) and sum(c[1] for c in counts) == len(want[1])
    for pad in pads:
        out, offs, seg = emul_destuff(lib, body, restarts, pad)
        assert out == want[0], ("bytes", len(body), restarts, pad, _first_difference(out, want[0]))
        assert offs == want[1], ("offsets", len(body), restarts, pad)
        assert seg == counts, ("counts", len(body), restarts, pad, [(g, a, b) for g, (a, b) in enumerate(zip(seg, counts)) if a != b][:4])
    return want


def _first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, len(a), len(b), bytes(a[max(0, k - 4):k + 4]).hex(), bytes(b[max(0, k - 4):k + 4]).hex()


# ---- the alphabet and the block-level writer -------------------------------------------------------------------------------------------
_AC4 = [0x11 * k for k in range(1, 14)]
_AC8 = [0x00, 0x08, 0x07, 0x18]
_AC8 += [s for s in jw.AC_SYMBOLS if s not in _AC4 and s not in _AC8 and s != 0x28][:47 - len(_AC8)]
DC_TAB = ([0] * 7 + [12] + [0] * 8, list(range(12)))
AC_TAB = ([0, 0, 0, 13, 0, 0, 0, 47, 0, 0, 0, 0, 0, 0, 0, 1], _AC4 + _AC8 + [0x28])
TABLES = {(0, 0): DC_TAB, (1, 0): AC_TAB}
EOB, AC8, WIDE = 0xd0, 0xd1, b"\xff\x00\x00"          # code bytes: end of block, (run 0, size 8), and FF00 = (run 2, size 8) as it stands stuffed


def _value(b):
    return b if b >= 128 else b - 255


def _stuffed(b):
    return b"\xff\x00" if b == 0xff else bytes([b])


class Scan:
    """Blocks in the byte-aligned alphabet, and the stuffed entropy-coded bytes they must become (the writer's output is compared
    with them).  dri: blocks per restart interval (greyscale: one block per MCU)."""

    def __init__(self, dri=0, seed=0):
        self.dri, self.rng = dri, np.random.default_rng(seed)
        self.blocks, self.raw, self.pred = [], bytearray(), 0

    @property
    def pos(self):
        return len(self.raw)

    def neutral(self, k=1):
        """k value bytes that are not FF"""
        return [int(v) for v in self.rng.integers(0, 255, k)]

    def block(self, dc=None, acs=()):
        """dc: None (difference 0: the byte 00) or the value byte of a size-8 difference (08 vv); acs: value bytes coded D1 vv, or
        (vv,) coded FF00 vv two places further on"""
        n = len(self.blocks)
        if self.dri and n and n % self.dri == 0:
            self.raw += bytes([0xff, 0xd0 + (n // self.dri - 1) % 8])
            self.pred = 0
        blk = [0] * 64
        if dc is None:
            self.raw.append(0x00)
        else:
            self.raw += b"\x08" + _stuffed(dc)
            self.pred += _value(dc)
        blk[0], at = self.pred, 1
        for t in acs:
            if isinstance(t, tuple):
                t, at = t[0], at + 2
                self.raw += WIDE + _stuffed(t)
            else:
                self.raw += bytes([AC8]) + _stuffed(t)
            blk[at] = _value(t)
            at += 1
        assert at <= 64
        if at < 64:
            self.raw.append(EOB)
        self.blocks.append(blk)

    def _plain(self, length):
        """a block of `length` raw bytes (2..127) without FF; the predictor is steered back towards 0"""
        assert 2 <= length <= 127, length
        odd = length & 1
        self.block((0x37 if self.pred > 0 else 0xc8) if odd else None, self.neutral((length - 2 - odd) // 2))

    def fill_exact(self, nbytes, nblocks):
        """nblocks blocks without FF that take exactly nbytes raw bytes, the markers between them included"""
        n0 = len(self.blocks)
        marks = sum(1 for j in range(n0, n0 + nblocks) if self.dri and j and j % self.dri == 0)
        room = nbytes - 2 * marks
        assert nblocks >= 0 and 2 * nblocks <= room <= 127 * nblocks, (nbytes, nblocks, marks)
        at = self.pos
        for k in range(nblocks):
            self._plain(room // nblocks + (1 if k < room % nblocks else 0))
        assert self.pos == at + nbytes

    def fill_to(self, target, residue=None, modulus=None):
        """blocks without FF up to raw offset `target` (where the next block, or the marker in front of it, begins); the number of
        blocks written so far then is `residue` modulo `modulus` (default: the restart interval)"""
        modulus = modulus or self.dri or 1
        residue = 0 if residue is None or modulus == 1 else residue % modulus
        nbytes, n0 = target - self.pos, len(self.blocks)
        assert nbytes >= 0, (target, self.pos)
        for nb in sorted(range((residue - n0) % modulus, nbytes // 2 + 1, modulus), key=lambda v: abs(v - nbytes / 90.0)):
            marks = sum(1 for j in range(n0, n0 + nb) if self.dri and j and j % self.dri == 0)
            if 2 * nb <= nbytes - 2 * marks <= 127 * nb:
                return self.fill_exact(nbytes, nb)
        raise AssertionError("no filling of %d bytes from block %d to residue %d mod %d" % (nbytes, n0, residue, modulus))

    def jpeg(self, blocks_x, eoi=True):
        """-> (file, blocks int16 [n, 64]); the writer's entropy-coded bytes are the ones predicted here"""
        blocks = np.asarray(self.blocks, np.int64)
        assert len(blocks) % blocks_x == 0 and np.abs(blocks).max() < 2048
        data = jw.jpeg_from_blocks(blocks, [(1, 1)], blocks_x, len(blocks) // blocks_x, [[1] * 64], TABLES, restart=self.dri or None)
        assert data.endswith(bytes(self.raw) + b"\xff\xd9"), "the writer's bytes are not the predicted ones"
        return (data if eoi else data[:-2]), blocks.astype(np.int16)


def raw_scan(data):
    """the bytes behind the SOS header to the end of the file: what the parser copies for the device"""
    sos = data.index(b"\xff\xda")
    return data[sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"):]


# ---- 3. patterns, placements, coverage ---------------------------------------------------------------------------------------------------
# name -> (bytes of the stuffed stream, n = any RSTn, restart files only)
PATTERNS = {"FF00": 2, "FF00FF00": 4, "FF00D0": 3, "FF0000": 3}
PATTERNS_RST = dict(PATTERNS, FFDn=2, FF00FFDn=4, FFDn08FF00=5, FF00D0FFDn=5)
RUNS = {"run64": 64, "run128": 128}                                      # FF 00 pairs that fill one / two whole pieces: byte streams only
_FIND = re.compile(rb"(?P<run128>(?:\xff\x00){64})|(?P<run64>(?:\xff\x00){32})|(?P<FF00D0FFDn>\xff\x00\xd0\xff[\xd0-\xd7])"
                   rb"|(?P<FFDn08FF00>\xff[\xd0-\xd7]\x08\xff\x00)|(?P<FF00FFDn>\xff\x00\xff[\xd0-\xd7])|(?P<FF00FF00>\xff\x00\xff\x00)"
                   rb"|(?P<FF00D0>\xff\x00\xd0)|(?P<FF0000>\xff\x00\x00)|(?P<FF00>\xff\x00)|(?P<FFDn>\xff[\xd0-\xd7])", re.S)
KINDS = ("piece", "wave", "workgroup")


def splits(name, length):
    """first byte at B - length + 1 .. B: `split` bytes of the pattern lie in front of the boundary (the long runs: first and last)"""
    return (0, length - 1) if name in RUNS else tuple(range(length))


def combos(patterns):
    return [(name, s) for name, length in patterns.items() for s in splits(name, length)]


def coverage(raws, restarts):
    """{(pattern, split, kind of boundary): occurrences} from the raw scans' own bytes.  Without restart intervals FF Dn is no
    pattern (both bytes are data)."""
    cov = {}
    for raw in raws:
        for m in _FIND.finditer(raw):
            name, (a, e) = m.lastgroup, m.span()
            if "Dn" in name and not restarts:
                continue
            for b in range(-(-a // PIECE) * PIECE, e, PIECE):
                if b == 0:
                    continue
                kind = "workgroup" if b % WG == 0 else "wave" if b % WAVE == 0 else "piece"
                cov[(name, b - a, kind)] = cov.get((name, b - a, kind), 0) + 1
    return cov


def required(patterns):
    return [(name, s, kind) for name, s in combos(patterns) for kind in KINDS]


def place(scan, name, at):
    """blocks that put pattern `name` with its first byte at raw offset `at` (filling up to it first)"""
    d = scan.dri
    if name == "FF00":                                       # 00 D1 [FF 00] D1 vv D0
        scan.fill_to(at - 2, 1)
        scan.block(None, [0xff] + scan.neutral())
    elif name == "FF00FF00":                                 # 00 D1 [FF 00 FF 00] 00 vv D0: the value +255, then the code FF00
        scan.fill_to(at - 2, 1)
        scan.block(None, [0xff, (scan.neutral()[0],)])
    elif name == "FF00D0":                                   # 00 D1 [FF 00 D0]: a value followed by the EOB code byte
        scan.fill_to(at - 2, 1)
        scan.block(None, [0xff])
    elif name == "FF0000":                                   # 63 coded coefficients ending in +255, then a block with DC difference 0
        scan.fill_to(at - 126, 1)
        scan.block(None, scan.neutral(62) + [0xff])
        scan.block(None, scan.neutral())
    elif name == "FFDn":
        scan.fill_to(at, 0)
        scan.block(None, scan.neutral())
    elif name == "FF00FFDn":                                 # an interval ending in a stuffed FF
        scan.fill_to(at - 126, d - 1)
        scan.block(None, scan.neutral(62) + [0xff])
        scan.block(None, scan.neutral())
    elif name == "FFDn08FF00":                               # an interval beginning with a stuffed value: DC difference +255
        scan.fill_to(at, 0)
        scan.block(0xff, scan.neutral())
    elif name == "FF00D0FFDn":
        scan.fill_to(at - 2, d - 1)
        scan.block(None, [0xff])
        scan.block(None, scan.neutral())
    else:
        raise KeyError(name)
    assert (scan.raw[at:at + 2] == b"\xff\x00") or (scan.raw[at] == 0xff and 0xd0 <= scan.raw[at + 1] <= 0xd7), name


BX = 4                                                        # blocks per row of the placement and end files (= their restart interval)


def _placement_file(patterns, dri, j):
    """File j of a placement family: every (pattern, split) at a piece boundary (320 + 256 c: never a multiple of 4096), and the
    combinations j, j + 1, ... at the workgroup boundaries 16384, 32768 and the wave boundaries 8192, 12288, 20480, 24576"""
    cs = combos(patterns)
    scan = Scan(dri, seed=1000 * bool(dri) + j)
    spots = [(320 + 256 * c, cs[c]) for c in range(len(cs))]
    assert spots[-1][0] + 200 < 2 * WAVE
    spots += [(b, cs[(j + 1 + k) % len(cs)]) for k, b in enumerate((2 * WAVE, 3 * WAVE, 5 * WAVE, 6 * WAVE))]
    spots += [(WG, cs[j]), (2 * WG, cs[(j + len(cs) // 2) % len(cs)])]
    for b, (name, s) in sorted(spots):
        place(scan, name, b - s)
    scan.fill_to(scan.pos + 300, 0, BX)
    return scan.jpeg(BX)


def _ends_file(total, dri, seed, final_ff=False, kept_multiple=0):
    """a file whose raw scan (the EOI's two bytes included) is `total` bytes long.  final_ff: no EOI, and the last two raw bytes are
    the FF 00 of the last block's 63rd coefficient.  kept_multiple: `total` is adjusted until the de-stuffed length is that
    multiple (the filling holds no FF, so a byte more of it is a byte more of both)"""
    for _ in range(8):
        scan = Scan(dri, seed=seed)
        end = total - (0 if final_ff else 2)
        if end > 1500:
            for k in range(4):
                place(scan, "FF00", 200 + 300 * k + k)
        if final_ff:
            scan.fill_to(end - 128, BX - 1, BX)
            scan.block(None, scan.neutral(62) + [0xff])
        else:
            scan.fill_to(end, 0, BX)
        data, blocks = scan.jpeg(BX, eoi=not final_ff)
        kept = len(destuff_ref(raw_scan(data), bool(dri))[0])
        if not kept_multiple or kept == kept_multiple:
            return data, blocks
        total += kept_multiple - kept
    raise AssertionError("no file of %d de-stuffed bytes" % kept_multiple)


LADDER_DRI, LADDER_L0 = 12, 24          # twelve blocks of two bytes (00 D0): the shortest interval there is
SUB_BYTES = (64, 128, 256, 512, 640)    # the subsequence lengths the planner uses at small and at default cuts


def _ladder_file(n_intervals, seed):
    """DRI 12; interval i is exactly 24 + i bytes after de-stuffing, i % 3 of them stuffed FFs where it is long enough"""
    scan = Scan(LADDER_DRI, seed=seed)
    for i in range(n_intervals):
        want, ff = LADDER_L0 + i, (i % 3 if i >= 16 else 0)
        at = scan.pos + (2 if i else 0)                      # (behind the marker the first block brings)
        if ff:
            scan.block(None, [0xff] * ff)                    # 00 (D1 FF 00) x ff D0: 2 + 2 ff bytes after de-stuffing, 2 + 3 ff raw
            scan.fill_exact(at + want + ff - scan.pos, LADDER_DRI - 1)
        else:
            scan.fill_exact(want + (2 if i else 0), LADDER_DRI)
    return scan.jpeg(LADDER_DRI)


LONG_BX, LONG_ROWS = 160, 150           # 24 000 blocks of about 184 raw bytes: just past 256 workgroups of 16 KiB


def _long_file(dri, seed):
    """63 coded coefficients in every block, nine value bytes in ten FF: about the densest stuffing a valid scan holds.  Even blocks have DC
    0 (so has every interval's first), odd ones +-128..255: every difference is of size 0 or 8."""
    rng = np.random.default_rng(seed)
    n = LONG_BX * LONG_ROWS
    vb = rng.integers(0, 256, (n, 63))
    vb[rng.random((n, 63)) < 0.9] = 0xff
    blocks = np.zeros((n, 64), np.int64)
    blocks[:, 1:] = np.where(vb >= 128, vb, vb - 255)
    blocks[1::2, 0] = rng.integers(128, 256, n // 2) * (rng.integers(0, 2, n // 2) * 2 - 1)
    data = jw.jpeg_from_blocks(blocks, [(1, 1)], LONG_BX, LONG_ROWS, [[1] * 64], TABLES, restart=dri or None)
    return data, blocks.astype(np.int16)


FAMILIES = ("place", "place_rst", "ends", "ends_rst", "ladder", "ladder_short", "long")


@functools.lru_cache(maxsize=None)
def family(name):
    """-> namespace(datas, blocks, restarts [per file])"""
    if name in ("place", "place_rst"):
        pats, dri = (PATTERNS_RST, BX) if name == "place_rst" else (PATTERNS, 0)
        files = [_placement_file(pats, dri, j) for j in range(len(combos(pats)))]
    elif name in ("ends", "ends_rst"):
        dri = BX if name == "ends_rst" else 0
        files = [_ends_file(t, dri, 50 + k) for k, t in enumerate((WG, WG + 1, 9 * PIECE + 2, 10 * PIECE - 1, 10 * PIECE, 10 * PIECE + 1))]
        files.append(_ends_file(WG + 1, dri, 60, final_ff=True))
        files.append(_ends_file(5200, dri, 61, kept_multiple=2 * 2560))
    elif name == "ladder":
        files = [_ladder_file(1300, 7)]
    elif name == "ladder_short":
        files = [_ladder_file(64, 8)]
    elif name == "long":
        files = [_long_file(0, 11), _long_file(LADDER_DRI, 12)]
    else:
        raise KeyError(name)
    restarts = [True, True] if name.startswith("ladder") else [False, True] if name == "long" else [name.endswith("_rst")] * len(files)
    return types.SimpleNamespace(name=name, datas=[f[0] for f in files], blocks=[f[1] for f in files], restarts=restarts[:len(files)])


def _byte_stream(restarts):
    """Every (pattern, split), the long runs included, at a piece, a wave and a workgroup boundary of one stream of
    neutral bytes -- not an entropy-coded segment, a byte stream for the parser and the rule.  With restarts it ends in a lone FF."""
    cs = combos(dict(PATTERNS_RST if restarts else PATTERNS, **RUNS))
    text = {"FF00": b"\xff\x00", "FF00FF00": b"\xff\x00\xff\x00", "FF00D0": b"\xff\x00\xd0", "FF0000": b"\xff\x00\x00",
            "run64": b"\xff\x00" * 32, "run128": b"\xff\x00" * 64, "FFDn": b"\xff\xd3", "FF00FFDn": b"\xff\x00\xff\xd5",
            "FFDn08FF00": b"\xff\xd0\x08\xff\x00", "FF00D0FFDn": b"\xff\x00\xd0\xff\xd7"}
    waves = [m * WAVE for m in range(3, 4 * len(cs) + 8) if m % 4][:len(cs)]
    spots = [(320 * (c + 1), cs[c]) for c in range(len(cs))] + [(waves[c], cs[c]) for c in range(len(cs))]
    spots += [(WG * (c + 1), cs[c]) for c in range(len(cs))]
    assert 320 * len(cs) + 200 < 3 * WAVE
    buf = bytearray(b"\x55" * (WG * len(cs) + 777))
    for b, (name, s) in spots:
        buf[b - s:b - s + len(text[name])] = text[name]
    if restarts:
        buf += b"\xff"
    return bytes(buf)


def _wrap(body, restarts):
    """a file around a byte stream that is no entropy-coded segment (the parser copies or de-stuffs it, nothing decodes it)"""
    return jw.write_jpeg(8, 8, [(1, 1, 1, 0, 0, 0)], {0: [1] * 64}, TABLES, body, restart_interval=4 if restarts else 0)[:-2]


# ---- 2. CPU tests --------------------------------------------------------------------------------------------------------------------------
ALPHABET = (0x00, 0xff, 0xd0, 0xd7, 0xd8, 0x55)
OFFSETS = range(-5, 2)                                       # a string starts 5 bytes before .. 1 byte after the boundary
TOTALS = {1, 2, 63, 64, 65, 16383, 16384, 16385, 32768}      # buffer lengths that must occur among the strings placed last
THREADS = 4                                                  # the exhaustive windows at 16 KiB boundaries are 5 GB through the rule


def _strings():
    return [bytes(s) for n in range(1, 6) for s in itertools.product(ALPHABET, repeat=n)]


def test_reference_and_local_rule_agree_and_the_alphabet_is_byte_aligned():
    codes = jw.huff_codes(*AC_TAB)
    assert codes[0x00] == (0xd0, 8) and codes[0x08] == (0xd1, 8) and codes[0x28] == (0xff00, 16)
    assert all(jw.huff_codes(*DC_TAB)[s] == (s, 8) for s in range(12))
    assert destuff_ref(b"\xff\x00\xff\xd0\xff\xff\xd9\xff", True) == (b"\xff\xff\xff\xd9\xff", [1])
    assert destuff_ref(b"\xff\x00\xff\xd0\xff\xff\xd9\xff", False) == (b"\xff\xff\xd0\xff\xff\xd9\xff", [])
    assert destuff_ref(b"\xff\xff\x00\xff\xff\xd1\x00", True) == (b"\xff\xff\xff\x00", [3])      # fill bytes are kept
    for s in _strings():
        for restarts in (False, True):
            assert destuff_local(s, restarts) == destuff_ref(s, restarts), (s.hex(), restarts)


def test_exhaustive_windows_inside_a_buffer(emul):
    """Every string of 1..5 bytes over {00, FF, D0, D7, D8, 55} starting 5 bytes before .. 1 byte after a piece boundary -- all of
    them in one buffer of neutral bytes, two pieces apart (the rule looks one byte back and one ahead) -- and around a 16 KiB
    boundary, 63 strings to a buffer.  The wrong variants 1 and 2 each give other bytes on the first buffer."""
    strings = _strings()
    assert len(strings) == 6 + 36 + 216 + 1296 + 7776
    cases = [(s, o) for s in strings for o in OFFSETS]
    buf = bytearray(b"\x55" * (2 * PIECE * (len(cases) + 1)))
    for k, (s, o) in enumerate(cases):
        at = 2 * PIECE * (k + 1) + o
        buf[at:at + len(s)] = s
    for restarts in (False, True):
        want = check_rule(emul, bytes(buf), restarts, pads=(0xd0, 0x00))
        assert destuff_local(buf, restarts) == want
        assert destuff_local(buf, restarts, wrong=1) != want
        assert not restarts or destuff_local(buf, restarts, wrong=2) != want       # (the byte behind a piece matters to markers only)
    def sixty_three(k0):
        part = cases[k0:k0 + 63]
        buf = bytearray(b"\x55" * (WG * (len(part) + 1)))
        for k, (s, o) in enumerate(part):
            at = WG * (k + 1) + o
            buf[at:at + len(s)] = s
        for restarts in (False, True):
            check_rule(emul, bytes(buf), restarts)

    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:     # (the rule takes a workgroup of neutral bytes per string)
        list(pool.map(sixty_three, range(0, len(cases), 63)))


def test_exhaustive_windows_as_the_last_bytes(emul):
    """The same strings at the same places with the buffer ending behind them: total length = boundary + offset + length, for the
    piece boundary 64 and the workgroup boundary 16384; and the strings of one and two bytes alone, and every string as the end of
    two whole workgroups.  The byte behind the buffer -- padding on the device -- is D0, then 00 (a lone FF in front of it must
    stay and must not be a marker; variant 3 makes it one)."""
    neutral = b"\x55" * (2 * WG)

    def placed_last(s):
        totals, caught = set(), 0
        heads = {b + o for b in (PIECE, WG) for o in OFFSETS} | {2 * WG - len(s)} | ({0} if len(s) <= 2 else set())
        for head in sorted(heads):
            body = neutral[:head] + s
            totals.add(len(body))
            for restarts in (False, True):
                want = check_rule(emul, body, restarts, pads=(0xd0, 0x00) if head <= PIECE + 1 else (0xd0,))
                if head == PIECE - 1:
                    assert destuff_local(body, restarts) == want
                    caught += destuff_local(body, restarts, wrong=3) != want
        return totals, caught

    done = [placed_last(s) for s in _strings()]           # (many short calls: threads would only wait for each other)
    totals = set().union(*(t for t, _ in done))
    assert TOTALS <= totals, sorted(TOTALS - totals)
    assert sum(c for _, c in done) > 0


def test_constructed_files_cover_what_they_claim():
    """The coverage tables, from the files' own bytes."""
    for name, pats in (("place", PATTERNS), ("place_rst", PATTERNS_RST)):
        fam = family(name)
        cov = coverage([raw_scan(d) for d in fam.datas], name == "place_rst")
        missing = [c for c in required(pats) if not cov.get(c)]
        assert not missing, (name, missing)
        assert len(required(pats)) == (36 if name == "place" else 84)
        # every file spans three workgroups, so seg0 / rst0 of the pictures of one launch differ
        assert all(2 * WG < len(raw_scan(d)) <= 3 * WG for d in fam.datas)
    for restarts in (False, True):
        pats = dict(PATTERNS_RST if restarts else PATTERNS, **RUNS)
        cov = coverage([_byte_stream(restarts)], restarts)
        missing = [c for c in required(pats) if not cov.get(c)]
        assert not missing, (restarts, missing)
    for name in ("ends", "ends_rst"):
        fam = family(name)
        lens = [len(raw_scan(d)) for d in fam.datas]
        assert {0, 1, 2, 63} <= {n % PIECE for n in lens} and {0, 1} <= {n % WG for n in lens}, lens
        last = raw_scan(fam.datas[6])
        assert len(last) == WG + 1 and last[-2:] == b"\xff\x00"                     # the 00 alone in the second workgroup
        kept = len(destuff_ref(raw_scan(fam.datas[7]), name == "ends_rst")[0])
        assert kept and all(kept % s == 0 for s in SUB_BYTES), kept
        assert all(r == (name == "ends_rst") for r in fam.restarts)
    for name, n in (("ladder", 1300), ("ladder_short", 64)):
        raw = raw_scan(family(name).datas[0])
        out, offs = destuff_ref(raw, True)
        lens = np.diff([0] + offs + [len(out) - 2])                                  # (the EOI's two bytes close the last interval)
        assert list(lens) == list(range(LADDER_L0, LADDER_L0 + n))
        assert {o % 16 for o in offs} == set(range(16))
        assert len(out) < len(raw) - 2 * len(offs)                                   # stuffed FFs inside the intervals
        for s in SUB_BYTES:
            for m in range(1, (LADDER_L0 + n - 2) // s + 1):
                assert {m * s - 1, m * s, m * s + 1} <= set(lens) or m * s - 1 < LADDER_L0, (s, m)
    assert 1300 > 256 and max(SUB_BYTES) * 2 + 1 < LADDER_L0 + 1300
    assert family("long").restarts == [False, True]
    for data in family("long").datas:
        assert len(raw_scan(data)) > 256 * WG == 4194304


def test_rule_on_every_constructed_file(mjx, emul):
    """emul_destuff == destuff_ref == the host parser (ParsedScan: scan_bytes, restart_offsets) on every constructed file and on
    the two byte streams; the stuffed copy the parser hands to the device is the file's raw scan.  The wrong variants 1 and 2 give
    other answers on files of both placement families, variant 3 on the byte stream that ends in a lone FF."""
    caught = {1: 0, 2: 0, 3: 0}
    items = [(d, r, fam) for fam in FAMILIES for d, r in zip(family(fam).datas, family(fam).restarts)]
    items += [(_wrap(_byte_stream(r), r), r, "bytes") for r in (False, True)]
    for data, restarts, fam in items:
        raw = raw_scan(data)
        want = check_rule(emul, raw, restarts, pads=(0xd0, 0xff) if fam != "long" else (0xd0,))
        host = mjx.ParsedScan(data)
        assert host.desc.scan_is_stuffed == 0 and host.scan_bytes() == want[0], (fam, len(raw))
        assert [host.desc.restart_offsets[k] for k in range(host.desc.n_restart)] == want[1], fam
        assert (host.desc.restart_interval != 0) == restarts
        host.close()
        dev = mjx.ParsedScan(data, device_destuff=True)
        assert dev.desc.scan_is_stuffed == 1 and dev.scan_bytes() == raw
        dev.close()
        if fam in ("place", "place_rst", "bytes"):
            assert destuff_local(raw, restarts) == want
            for v in caught:
                caught[v] += destuff_local(raw, restarts, wrong=v) != want
            if fam != "bytes":                                  # every decodable placement file tells 1 (and, with markers, 2) apart
                assert destuff_local(raw, restarts, wrong=1) != want
                assert not restarts or destuff_local(raw, restarts, wrong=2) != want
    assert all(caught.values()), caught
    # the long scans: about two bytes in three are kept where nothing but stuffing goes; every workgroup of the restart scan has markers
    seg = emul_destuff(emul, raw_scan(family("long").datas[0]), False)[2]
    assert len(seg) > 256 and all(0.6 * WG < s[0] < 0.75 * WG for s in seg[:-1])
    seg = emul_destuff(emul, raw_scan(family("long").datas[1]), True)[2]
    assert len(seg) > 256 and all(s[1] >= 1 for s in seg)
    # the end file whose last workgroup keeps nothing
    for name in ("ends", "ends_rst"):
        seg = emul_destuff(emul, raw_scan(family(name).datas[6]), name == "ends_rst")[2]
        assert len(seg) == 2 and seg[1][0] == 0, seg


def test_oracle_gives_back_the_blocks_written(orc):
    """one file per family through the CPU oracle: the blocks written, which is what the GPU tests hold the device to"""
    for fam in FAMILIES:
        f = family(fam)
        k = len(f.datas) - 1
        ref = orc.decode(f.datas[k], layout=orc.LAYOUT_STD, ext_dri=True)
        assert np.array_equal(orc.interleave(ref), f.blocks[k]), fam


# ---- 4. GPU tests ----------------------------------------------------------------------------------------------------------------------------
PATHS = ("batch", "decode_batch", "pool")


def _decoded(b, n):
    b.decode()
    b.wait()
    return [b.status(i) for i in range(n)]


def _batch(mjx, ctx, datas, device_destuff=False, **kw):
    """a Batch of the files; it copies the descriptors, so the parsed scans are closed here.  device_destuff: one flag, or one per file"""
    flags = device_destuff if isinstance(device_destuff, (list, tuple)) else [device_destuff] * len(datas)
    scans = [mjx.ParsedScan(d, device_destuff=f) for d, f in zip(datas, flags)]
    try:
        assert [s.desc.scan_is_stuffed for s in scans] == [int(f) for f in flags]
        return mjx.Batch(ctx, scans, **kw)
    finally:
        for s in scans:
            s.close()


def check_family(mjx, orc, ctx, name, paths=PATHS, groups=False):
    """Decodes the family's files in one batch per path with the device de-stuffing: status OK, T0 = the blocks written (exact),
    RGB = the bytes of the same file de-stuffed on the host in this process; one file also against the oracle's coefficients.
    The pool's interface hands out pictures, not coefficients, and a list decoded with kept coefficients is one group: there, and
    with groups=True (several pipelined groups), the pictures and the statuses are what is compared."""
    fam = family(name)
    if groups:                                             # (a list of eight files or fewer is never cut)
        reps = -(-9 // len(fam.datas))
        fam = types.SimpleNamespace(datas=fam.datas * reps, blocks=fam.blocks * reps)
    n = len(fam.datas)
    host = _batch(mjx, ctx, fam.datas, keep_coefs=True)
    assert _decoded(host, n) == [mjx.OK] * n, name
    for i in range(n):
        assert np.array_equal(host.coefs(i), fam.blocks[i]), (name, "host", i)
    ref = orc.decode(fam.datas[-1], layout=orc.LAYOUT_STD, ext_dri=True)
    done = []
    for path in paths:
        if path == "pool":
            pool = mjx.Pool([0, 0])
            res = pool.decode_batch(fam.datas, device_destuff=True)
            assert res.status == [mjx.OK] * n, (name, path, res.status)
            assert n == 1 or sorted(set(res.slot_of)) == [0, 1]
            for i in range(n):
                assert np.array_equal(res.rgb(i), host.rgb(i)), (name, path, i)
            res.close()
            pool.close()
            done.append(path)
            continue
        if path == "batch":
            dev = _batch(mjx, ctx, fam.datas, True, keep_coefs=True)
            assert _decoded(dev, n) == [mjx.OK] * n, (name, path, [dev.status(i) for i in range(n)])
        else:
            dev, st = mjx.decode_batch(ctx, fam.datas, device_destuff=True, keep_coefs=not groups, threads=4)
            assert st == [mjx.OK] * n, (name, path, st)
            assert not groups or dev.geometry()["chunks"] >= 2
        mx, cnt = dev.compare_rgb(list(range(n)), host, list(range(n)))
        assert int(mx.max()) == 0 and int(cnt.sum()) == 0, (name, path, [i for i in range(n) if mx[i]])
        if path == "batch" or not groups:
            for i in range(n):
                got = dev.coefs(i)
                assert got.shape == fam.blocks[i].shape and np.array_equal(got, fam.blocks[i]), \
                    (name, path, i, np.argwhere((got != fam.blocks[i]).any(axis=1))[:4].ravel().tolist())
            assert np.array_equal(dev.coefs(n - 1), orc.interleave(ref)), (name, path)
        dev.close()
        done.append(path)
    host.close()
    return done


def _child(name, env, paths, groups=False):
    """a decode under a changed environment: a fresh process, which makes the family's files again and runs check_family (the
    libraries are built: the tests that come here ask for the mjx fixture)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import __graft_entry__ as ge, oracle_binding as orc, test_destuff_boundaries as t\n"
            "mjx = ge.load_package()\n"
            "ctx = mjx.Context(0)\n"
            "print('done', t.check_family(mjx, orc, ctx, %r, %r, %r))\n"
            "ctx.close()\n" % (ROOT, os.path.join(ROOT, "tests"), name, tuple(paths), groups))
    keep = {k: v for k, v in os.environ.items() if k not in ("MJX_DESTUFF_DIRECT", "MJX_GROUP_MB", "MJX_GROUP_FIRST_MB", "MJX_LATENCY_SUB_BITS", "MJX_FIT_SHORT")}
    out = subprocess.run([sys.executable, "-c", code], env=dict(keep, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "done" in out.stdout, (name, env, out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_family_through_batch_api_decode_batch_and_pool(mjx, orc, gpu_ctx, name):
    assert check_family(mjx, orc, gpu_ctx, name) == list(PATHS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_family_through_the_linear_copy(mjx, name):
    """MJX_DESTUFF_DIRECT=0: scans without restart intervals too go through a linear copy and k_scan_interleave"""
    _child(name, {"MJX_DESTUFF_DIRECT": "0"}, ("batch", "decode_batch"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_family_in_pipelined_groups(mjx, name):
    """MJX_GROUP_MB=1 (and a first group of 20 KB): mjx_decode_batch cuts the list into several groups that are uploaded and
    decoded in overlap"""
    _child(name, {"MJX_GROUP_MB": "1", "MJX_GROUP_FIRST_MB": "0.02"}, ("decode_batch",), groups=True)


@pytest.mark.gpu
def test_short_ladder_under_the_shortest_cuts(mjx):
    """64 intervals of 24 .. 87 bytes with the shortest subsequences the planner can be asked for"""
    _child("ladder_short", {"MJX_LATENCY_SUB_BITS": "512", "MJX_FIT_SHORT": "256"}, ("batch", "decode_batch"))
    _child("ladder_short", {"MJX_LATENCY_SUB_BITS": "512", "MJX_FIT_SHORT": "256", "MJX_DESTUFF_DIRECT": "0"}, ("batch",))


@pytest.mark.gpu
def test_mixed_batch_and_its_tiling(mjx, orc, gpu_ctx):
    """Stuffed and host-de-stuffed scans, restart and non-restart, short and long in one Batch, then tile(3) of it: seg0, rst0,
    ii_index and out_off of the device-side compaction are all non-trivial."""
    picks = [("place", 3, True), ("place_rst", 5, False), ("ends", 2, True), ("long", 1, True), ("ladder_short", 0, True),
             ("ends_rst", 6, True), ("long", 0, False), ("place_rst", 20, True), ("ends_rst", 7, True), ("place", 7, True),
             ("ladder", 0, True), ("ends", 6, True)]
    datas = [family(f).datas[k] for f, k, _ in picks]
    blocks = [family(f).blocks[k] for f, k, _ in picks]
    n = len(picks)
    host = _batch(mjx, gpu_ctx, datas)
    assert _decoded(host, n) == [mjx.OK] * n
    kept = _batch(mjx, gpu_ctx, datas, [dd for _, _, dd in picks], keep_coefs=True)
    assert _decoded(kept, n) == [mjx.OK] * n
    for i in range(n):
        assert np.array_equal(kept.coefs(i), blocks[i]), picks[i]
    mx, _ = kept.compare_rgb(list(range(n)), host, list(range(n)))
    assert int(mx.max()) == 0, [picks[i] for i in range(n) if mx[i]]
    base = _batch(mjx, gpu_ctx, datas, [dd for _, _, dd in picks])
    big = base.tile(3)
    assert len(big) == 3 * n and _decoded(big, 3 * n) == [mjx.OK] * (3 * n)
    idx = list(range(3 * n))
    mx, _ = big.compare_rgb(idx, host, [i % n for i in idx])
    assert int(mx.max()) == 0, [(i, picks[i % n]) for i in idx if mx[i]]
    ref = orc.decode(datas[7], layout=orc.LAYOUT_STD, ext_dri=True)
    assert np.array_equal(kept.coefs(7), orc.interleave(ref))
    kept.close()
    big.close()
    base.close()
    host.close()

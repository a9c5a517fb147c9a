"""The entropy stage with Huffman tables of every shape (tests/jpegwriter.huffman_shapes): one-bit codes, codes at and just past
the 9-bit primary table, second-level tables of 1 to 7 index bits, symbols of 26 and 27 bits, all 256 AC symbols, T.81 K.2 tables
and 24 random length profiles -- three distinct table pairs per picture, on slots 0, 1 and 3.

The pictures are the files of tests/test_sampling_layouts.py with their entropy-coded segment coded again
(jpegwriter.recode_huffman), so the expected coefficients are the writer's, and four constructed greyscale pictures: two bits
per block, two bits per stream entry (the densest stream a column holds) with and without synchronisation points, and 27-bit
symbols.

CPU tests: the decode tables the host builds, walked over every 16-bit window against a canonical decode written here from T.81
C.2, pair part included; the tables the host refuses; the planner's table set; the kernels' per-lane routine on the CPU emulation
(tests/emul) in both its kernel sequences; Pillow's decode of every re-coded file, which pins the writer independently.  GPU
tests: T0 bit for bit the writer's and the oracle's, RGB within TOL of the oracle, status OK -- through the latency path, the
emitting pass and its switches, device de-stuffing, restart intervals, multi-scan scripts, REF_COMPAT and the front doors.  Every
file sent to the device is a valid file that the oracle decodes.
"""
import ctypes
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import oracle_binding as orc_mod
import test_sampling_layouts as sl

ROOT = sl.ROOT
SHAPES = jw.SHAPES
# 4:2:0, 4:4:4, a crossed layout with three different components, and a greyscale frame
LAYS = ["Y22_Cb11_Cr11", "Y11_Cb11_Cr11", "Y21_Cb12_Cr11", "gray21"]
SMALL, TRIAL, QUALITY = (333, 217), (640, 480), 90
TRIAL_SHAPES = ["ladder", "anti", "flat", "edge9_10"]
SLOTS = (0, 1, 3)


# ---- files ---------------------------------------------------------------------------------------------------------------------
def source(lname, w, h, quality=QUALITY, noise=4.0):
    """(bytes, the writer's blocks in decode order) of the Annex-K file the re-coded ones come from"""
    return sl.layout_file(lname, w, h, quality=quality, noise=noise)


def writer_t0(lname, w, h, quality=QUALITY, noise=4.0):
    """the writer's blocks MCU-interleaved: what T0 must be"""
    data, blocks = source(lname, w, h, quality, noise)
    ref = sl.oracle_std(data)
    for c, b in enumerate(blocks):
        assert np.array_equal(ref.coefs[c], b), (lname, w, h, c)
    return orc_mod.interleave(ref)


@functools.lru_cache(maxsize=None)
def picture_shapes(lname, w, h, quality=QUALITY, noise=4.0):
    """[({shape: DC table}, {shape: AC table})] per component, over the component's own symbol counts (so "frequent" differs from
    component to component, and with it the tables)"""
    ref = sl.oracle_std(source(lname, w, h, quality, noise)[0])
    return [(jw.huffman_shapes(jw.DC_SYMBOLS, dcn, seed=2 * c), jw.huffman_shapes(jw.AC_SYMBOLS, acn, seed=2 * c + 1))
            for c, (dcn, acn) in enumerate(jw.symbol_counts(ref))]


def tables_of(lname, w, h, shape, quality=QUALITY, noise=4.0):
    return [(dc[shape], ac[shape]) for dc, ac in picture_shapes(lname, w, h, quality, noise)]


@functools.lru_cache(maxsize=None)
def recoded(lname, w, h, shape, restart=None, quality=QUALITY, noise=4.0):
    data = source(lname, w, h, quality, noise)[0]
    return jw.recode_huffman(data, sl.oracle_std(data), tables_of(lname, w, h, shape, quality, noise), SLOTS, restart)


def one_bit(lname, w, h, shape):
    return any(jw.has_1bit_code(t) for pair in tables_of(lname, w, h, shape) for t in pair)


@functools.lru_cache(maxsize=None)
def constructed(which, blocks_x, blocks_y):
    """(bytes, blocks [n, 64] zig-zag with absolute DC) of a greyscale picture of blocks_x x blocks_y blocks:
      "bits2_block"  a 1-bit code for DC size 0 and a 1-bit end-of-block, every block flat: two bits per block
      "bits2_entry"  symbol 0x01 on the 1-bit code, every AC coefficient +-1: two bits per entry of the coefficient stream, the most a
                     stream can hold per bit (the column capacity of mjx_kernels.h), and nothing a decoder could synchronise on
      "bits2_dense"  the same with an end-of-block in every 16th block, which decoders synchronise on: 993 words -- stream entries
                     and one word per block -- in 1972 bits, more than one per two bits
      "bits27"       DC differences of size 11 and AC values of size 10 behind 16-bit codes: symbols of 27 and 26 bits"""
    n = blocks_x * blocks_y
    rng = np.random.default_rng([n, len(which)])
    blk = np.zeros((n, 64), np.int32)
    if which == "bits2_block":
        dc, ac = ([1] + [0] * 15, [0]), ([1] + [0] * 15, [0x00])
    elif which in ("bits2_entry", "bits2_dense"):
        dc, ac = ([1] + [0] * 15, [0]), ([1, 1] + [0] * 14, [0x01, 0x00])
        blk[:, 1:] = rng.integers(0, 2, (n, 63)) * 2 - 1
        if which == "bits2_dense":
            blk[::16, 33:] = 0
    else:
        dc = jw.table_of_lengths(list(range(12)), list(range(1, 8)) + [16] * 5)                # sizes 7 .. 11 on 16-bit codes
        ac = jw.huffman_shapes(jw.AC_SYMBOLS, {s: 1 + (s & 15 != 10) * 100 for s in jw.AC_SYMBOLS})["ladder"]      # size 10: 16 bits
        blk[:, 0] = np.where(np.arange(n) % 2 == 0, 1000, -1000) + rng.integers(-20, 21, n)     # differences of +-2000: size 11
        for k in range(n):
            pos = rng.choice(np.arange(1, 64), 6, replace=False)
            blk[k, pos] = rng.integers(512, 1024, 6) * (rng.integers(0, 2, 6) * 2 - 1)
        assert all(jw.huff_codes(*ac)[(r << 4) | 10][1] == 16 for r in range(16))
    ent = jw.encode_scan(blk, [0] * n, {0: jw.huff_codes(*dc)}, {0: jw.huff_codes(*ac)})
    data = jw.write_jpeg(blocks_x * 8, blocks_y * 8, [(1, 1, 1, 0, 0, 0)], {0: [1] * 64}, {(0, 0): dc, (1, 0): ac}, ent)
    return data, blk.astype(np.int16)


CONSTRUCTED = ["bits2_block", "bits2_entry", "bits2_dense", "bits27"]


# ---- the decode tables, walked over every 16-bit window ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul_lib(mjx):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "libhuff_emul.so"))
    lib.emul_build_table.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.emul_table_set.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.emul_decode_coefs_sub.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    lib.emul_single_decode_cp.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                          ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    return lib


def built_table(lib, table, is_dc, pair):
    bits, vals = table
    cap = 2 * 512 + 4096
    out = np.zeros(cap, np.uint32)
    n = lib.emul_build_table(bytes(bits), bytes(vals) + bytes(256 - len(vals)), int(is_dc), int(pair), out.ctypes.data, cap)
    assert n > 0, n
    return out[:n].copy()


def canonical(table):
    """T.81 C.2, bit by bit on all 65536 windows of 16 bits: (symbol or -1 where no code matches, code length)"""
    bits, vals = table
    w = np.arange(65536, dtype=np.int64)
    sym, ln = np.full(65536, -1, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        c = w >> (16 - l)
        hit = (sym < 0) & (c >= code) & (c < code + bits[l - 1])
        sym[hit] = np.asarray(vals + [0], np.int64)[k + (c[hit] - code)]
        ln[hit] = l
        code = (code + bits[l - 1]) << 1
        k += bits[l - 1]
    return sym, ln


def symbol_fields(sym, is_dc):
    """(zinc, size, cnt) of symbols as mjx_huff.h defines them; a DC symbol above 15 has none (bad)"""
    sym = np.asarray(sym, np.int64)
    if is_dc:
        return np.ones_like(sym), sym, np.zeros_like(sym)
    size = sym & 15
    return np.where(sym == 0, 64, (sym >> 4) + 1), size, (size != 0).astype(np.int64)


def walk(t, front=512):
    """primary entry, link, second-level entry for all 65536 windows, as symbol_step does it -> the final entries"""
    w = np.arange(65536, dtype=np.int64)
    e = t[w >> 7].astype(np.int64)
    link = (e >> 31) == 1
    nb = e & 15
    off = ((e >> 4) & 0xffff) // 4
    assert np.all(nb[link] <= 7) and np.all(off[link] >= front)
    idx = off + (((w & 0x7f) >> (7 - np.minimum(nb, 7))) & ((1 << nb) - 1))
    assert np.all(idx[link] < len(t)), "a link leaves the table"
    e2 = t[np.where(link, idx, 0)].astype(np.int64)
    return np.where(link, e2, e), link


def check_table(lib, table, is_dc, what):
    sym, ln = canonical(table)
    bad_want = (sym < 0) | ((sym > 15) if is_dc else False)
    zinc, size, cnt = symbol_fields(np.maximum(sym, 0), is_dc)
    npairs = 0
    for pair in ((False,) if is_dc else (False, True)):
        t = built_table(lib, table, is_dc, pair)
        e, link = walk(t, 1024 if pair else 512)
        assert np.all((e >> 31) == 0) and np.all(((e >> 15) & 1) == 0), what
        bad = ((e >> 30) & 1) == 1
        assert np.array_equal(bad, bad_want), (what, pair, int(np.argmax(bad != bad_want)))
        assert np.all(link[bad]), (what, "a bad entry that is not behind a link")
        ok = ~bad
        got = {"zinc": (e >> 16) & 0x7f, "size": (e >> 11) & 15, "cnt": (e >> 8) & 1, "adv": e & 31}
        want = {"zinc": zinc, "size": size, "cnt": cnt, "adv": ln + size}
        for k in got:
            assert np.array_equal(got[k][ok], want[k][ok]), (what, pair, k, int(np.argmax((got[k] != want[k]) & ok)))
        baseline = ok & (size <= (11 if is_dc else 10))                 # (T.81 Tables F.1, F.2: what a baseline stream uses)
        assert np.all((got["adv"][baseline] >= 1) & (got["adv"][baseline] <= 27)), what
        assert np.all(got["adv"][bad] == 1) and np.all(got["size"][bad] == 0), what
        if not pair:
            continue
        # the pair part, from the canonical decode alone: entry i = the symbol behind the one the 9 bits i begin with, if that one is
        # no end-of-block and both lie wholly inside the 9 bits
        want_pair = np.zeros(512, np.int64)
        for i in range(512):
            w16 = i << 7
            s1, l1 = int(sym[w16]), int(ln[w16])
            if s1 < 0 or l1 > 9 or s1 == 0:
                continue
            adv1 = l1 + (s1 & 15)
            if adv1 >= 9:
                continue
            rem = 9 - adv1
            w2 = ((i << adv1) & 511) << 7                              # the bits behind it, zeros behind them
            s2, l2 = int(sym[w2]), int(ln[w2])
            if s2 < 0 or l2 > rem:
                continue
            z2, sz2, c2 = symbol_fields([s2], False)
            want_pair[i] = (int(z2[0]) << 16) | (int(sz2[0]) << 11) | (int(c2[0]) << 8) | (l2 + int(sz2[0]))
        got_pair = t[512:1024].astype(np.int64)
        assert np.array_equal(got_pair, want_pair), (what, "pair part", int(np.argmax(got_pair != want_pair)))
        first = t[:512].astype(np.int64)
        behind = ((first >> 31) == 1) | (((first >> 16) & 0x7f) == 64)
        assert not np.any(got_pair[behind]), (what, "a pair entry behind a link, a bad entry or an end-of-block")
        npairs = int(np.count_nonzero(got_pair))
        assert npairs == int(np.count_nonzero(want_pair))
    return npairs


def profile_counts():
    """symbol counts of a photograph-like picture (the 640 x 480 4:2:0 trial picture's luma)"""
    ref = sl.oracle_std(source("Y22_Cb11_Cr11", *TRIAL)[0])
    return jw.symbol_counts(ref)[0]


def test_every_shape_is_a_valid_table():
    """Prefix codes of at most 16 bits with the all-ones code free, deterministic, and of the shape their name promises."""
    dcn, acn = profile_counts()
    for syms, freq, is_dc in ((jw.DC_SYMBOLS, dcn, True), (jw.AC_SYMBOLS, acn, False)):
        a, b = jw.huffman_shapes(syms, freq, seed=5), jw.huffman_shapes(syms, freq, seed=5)
        assert a == b and list(a) == SHAPES
        rank = sorted(syms, key=lambda s: (-freq.get(s, 0), s))
        for name, (bits, vals) in a.items():
            lengths = [l + 1 for l in range(16) for _ in range(bits[l])]
            assert len(vals) == len(lengths) == len(set(vals)) and jw.kraft(lengths) < 65536, name
            assert set(syms) <= set(vals) and (set(vals) == set(syms) or name == "all256"), name
            codes = jw.huff_codes(bits, vals)
            assert all(code != (1 << ln) - 1 for code, ln in codes.values()), name
        lens = {n: {s: jw.huff_codes(*t)[s][1] for s in syms} for n, t in a.items()}
        assert [lens["ladder"][s] for s in rank[:7]] == list(range(1, 8)) and all(lens["ladder"][s] == 16 for s in rank[7:])
        assert [lens["anti"][s] for s in rank[::-1][:7]] == list(range(1, 8)) and all(lens["anti"][s] == 16 for s in rank[:-7])
        assert len(set(lens["flat"].values())) == 1
        assert set(lens["edge9"].values()) == {9} and set(lens["edge10"].values()) == {10} and set(lens["edge9_10"].values()) == {9, 10}
        for k in range(1, 8):
            assert max(lens["sub%d" % k].values()) == 9 + k and min(lens["sub%d" % k].values()) == 2
        assert len(a["all256"][1]) == (16 if is_dc else 256) and a["all256"][0][15] > 0
        if all(freq.get(s) for s in syms):
            assert a["k2"] == jw.optimal_table({s: freq[s] for s in syms})
        rnd = [a["random%d" % r] for r in range(jw.N_RANDOM_SHAPES)]
        assert len({tuple(t[0]) for t in rnd}) >= 20
        full = [jw.kraft([l + 1 for l in range(16) for _ in range(t[0][l])]) for t in rnd]
        assert sum(f == 65536 - (1 << (16 - max(l + 1 for l in range(16) if t[0][l]))) for f, t in zip(full, rnd)) >= 6      # complete but for one
        assert sum(f < 65536 * 3 // 4 for f in full) >= (6 if not is_dc else 3)                      # many code points unused


def test_decode_tables_over_every_window(emul_lib):
    """build_decode_table for every shape, DC and AC, without and with the pair part: primary entry, link and second-level entry of
    every 16-bit window give the symbol, code length, zinc, size, cnt and adv of the canonical decode and `bad` exactly where no
    code matches; every link width 1..7 occurs; the pair part equals the rule of mjx_huff.h computed from the canonical decode
    (so it is non-zero wherever a pair is certain, and zero everywhere else), and it is not empty."""
    dcn, acn = profile_counts()
    widths, pairs = set(), {}
    for is_dc, syms, freq in ((True, jw.DC_SYMBOLS, dcn), (False, jw.AC_SYMBOLS, acn)):
        for seed in (0, 1):
            for name, table in jw.huffman_shapes(syms, freq, seed=seed).items():
                n = check_table(emul_lib, table, is_dc, (name, "dc" if is_dc else "ac", seed))
                t = built_table(emul_lib, table, is_dc, False)[:512].astype(np.int64)
                widths |= {(name[:3], int(x)) for x in (t[(t >> 31) == 1] & 15)}
                if not is_dc:
                    pairs[(name, seed)] = n
    assert {k for n3, k in widths if n3 == "sub"} >= set(range(1, 8)), sorted(widths)
    assert pairs[("ladder", 0)] > 100 and pairs[("k2", 0)] > 50 and pairs[("edge9", 0)] == 0, pairs
    assert sum(v > 0 for v in pairs.values()) >= len(pairs) // 2, pairs
    # the tables the suite had before: Annex K, and the two hand-made ones of the corrupt-stream tests
    ak = jw._annex_k_tables()
    for (cls, slot), table in ak.items():
        check_table(emul_lib, table, cls == 0, ("annex k", cls, slot))
    check_table(emul_lib, jw.full_ac_table(), False, "full_ac_table")
    check_table(emul_lib, jw.small_dc_table(), True, "small_dc_table")
    check_table(emul_lib, ([0] * 3 + [1] + [0] * 12, [16]), True, "a DC symbol above 15")
    for which in CONSTRUCTED:
        for key, table in jw.tables_from_jpeg(constructed(which, 8, 8)[0]).items():
            check_table(emul_lib, table, key[0] == 0, (which, key))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _grey_file(dc, ac, entropy=b"\x00" * 8):
    return jw.write_jpeg(8, 8, [(1, 1, 1, 0, 0, 0)], {0: [1] * 64}, {(0, 0): dc, (1, 0): ac}, entropy)


def test_tables_the_host_refuses(mjx, orc, emul_lib):
    """None of these reaches a device: a table with no code or more than 256 codes is MJX_ERR_BAD_HUFFMAN from mjx_parse, an
    over-subscribed one from mjx_validate (the planner builds the decode tables), and a DC symbol above 15 that the stream uses is
    MJX_ERR_BAD_HUFFMAN from the decode -- the entry is a bad one (huffman.rs:202) -- which the emulation shows; the oracle refuses
    the same file."""
    good_dc, good_ac = jw.small_dc_table(), jw.full_ac_table()
    assert mjx.ParsedScan(_grey_file(good_dc, good_ac)).validate() == mjx.OK
    for dc, ac in ((([0] * 16, []), good_ac), (good_dc, ([0] * 16, []))):
        with pytest.raises(mjx.MjxError) as e:
            mjx.ParsedScan(_grey_file(dc, ac))
        assert e.value.code == mjx.ERR_BAD_HUFFMAN
    many = ([0] * 14 + [2, 255], list(range(256)) + [0])
    with pytest.raises(mjx.MjxError) as e:
        mjx.ParsedScan(_grey_file(good_dc, many))
    assert e.value.code == mjx.ERR_BAD_HUFFMAN
    cases = [(([3] + [0] * 15, [0, 1, 2]), mjx.ERR_BAD_HUFFMAN), (([1, 3] + [0] * 14, [0, 1, 2, 3]), mjx.ERR_BAD_HUFFMAN),
             (([0] * 15 + [255], list(range(255))), mjx.OK), (([0] * 8 + [255] + [0] * 6 + [1], list(range(256))), mjx.OK)]
    for k, (t, want) in enumerate(cases):                              # (over-subscribed at 1 bit, at 2 bits; two full but valid ones)
        for cls in (0, 1):
            scan = mjx.ParsedScan(_grey_file(t if cls == 0 else good_dc, t if cls == 1 else good_ac))
            try:
                assert scan.validate() == want, (k, cls)
            finally:
                scan.close()
    # a DC table whose 1-bit code is symbol 16: parsed, planned, and no code of the stream is valid
    dc16 = ([1, 1] + [0] * 14, [16, 0])
    data = _grey_file(dc16, good_ac, b"\x00" * 8)
    scan = mjx.ParsedScan(data)
    assert scan.validate() == mjx.OK
    scan.close()
    rc, _, st = emul_two_pass(emul_lib, data)
    assert rc == mjx.ERR_BAD_HUFFMAN and st[6] == 1, (rc, st)
    with pytest.raises(orc.OracleError):
        orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True)
    # ... and is harmless where the stream does not use it
    data = _grey_file(dc16, good_ac, jw.encode_blocks(np.zeros((1, 64), np.int32), [0], {0: jw.huff_codes(*dc16)}, {0: jw.huff_codes(*good_ac)}))
    rc, coefs, st = emul_two_pass(emul_lib, data)
    assert rc == 0 and not coefs.any()


# ---- planning ----------------------------------------------------------------------------------------------------------------------
def table_set(lib, data):
    """-> (bytes of the larger of the picture's two table sets, distinct DC tables, distinct AC tables, ImagePlan::emit_fits)"""
    out = np.zeros(16, np.uint32)
    rc = lib.emul_table_set(data, len(data), out.ctypes.data)
    assert rc == 0, rc
    tabs = [int(x) for x in out[3:3 + int(out[2])]]
    return 4 * int(max(out[0], out[1])), len({t & 0xffff for t in tabs}), len({t >> 16 for t in tabs}), bool(out[15])


def test_three_table_pairs_are_planned_and_fit(emul_lib):
    """Three distinct pairs on slots 0, 1 and 3 are three decode tables per class; a slot that repeats a table shares it; the set
    -- three DC tables, three AC tables with their pair parts, every second-level table -- stays under the 0x7fff bytes a 16-bit
    LDS offset reaches, for every shape.  The largest is 23 696 bytes (sub7 on Y21_Cb12_Cr11)."""
    largest = (0, None)
    for lname in LAYS:
        for shape in SHAPES:
            size, ndc, nac, _ = table_set(emul_lib, recoded(lname, *SMALL, shape))
            largest = max(largest, (size, (shape, lname)))
            assert size <= 0x7fff, (shape, lname, size)
            if not lname.startswith("gray"):
                tabs = tables_of(lname, *SMALL, shape)
                assert ndc == len({repr(t[0]) for t in tabs}) and nac == len({repr(t[1]) for t in tabs}), (shape, lname, ndc, nac)
    print("largest table set: %d bytes (%s)" % largest)
    assert 20000 < largest[0] <= 0x7fff, largest
    data = source("Y22_Cb11_Cr11", *SMALL)[0]
    t = tables_of("Y22_Cb11_Cr11", *SMALL, "ladder")
    u, v = tables_of("Y22_Cb11_Cr11", *SMALL, "anti"), tables_of("Y22_Cb11_Cr11", *SMALL, "sub7")
    three = jw.recode_huffman(data, sl.oracle_std(data), [t[0], u[1], v[2]], SLOTS)          # three shapes in one picture
    assert table_set(emul_lib, three)[1:3] == (3, 3)
    assert emul_problems(emul_lib, three, writer_t0("Y22_Cb11_Cr11", *SMALL)) == []
    shared = jw.recode_huffman(data, sl.oracle_std(data), [t[0], t[1], t[1]], SLOTS)
    assert table_set(emul_lib, shared)[1:3] == (2, 2)
    mixed = jw.recode_huffman(data, sl.oracle_std(data), [t[0], (t[1][0], t[2][1]), (t[1][0], t[0][1])], SLOTS)
    assert table_set(emul_lib, mixed)[1:3] == (2, 2)
    ref = sl.oracle_std(mixed)
    assert np.array_equal(orc_mod.interleave(ref), writer_t0("Y22_Cb11_Cr11", *SMALL))


# ---- the writer, pinned by Pillow --------------------------------------------------------------------------------------------------
def test_pillow_decodes_every_recoded_file_like_its_source():
    """libjpeg (through Pillow) knows nothing of this project: its picture of a re-coded file equals its picture of the source,
    for every shape -- tables with 1-bit codes included -- on every layout, with restart intervals, and as multi-scan files."""
    Image = pytest.importorskip("PIL.Image")

    def pil(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    n = 0
    for lname in LAYS:
        want = pil(source(lname, *SMALL)[0])
        for shape in SHAPES:
            assert np.array_equal(pil(recoded(lname, *SMALL, shape)), want), (lname, shape)
            n += 1
        for shape, restart in (("ladder", 1), ("anti", 5), ("sub7", sl.mcux_of(lname, SMALL[0]))):
            assert np.array_equal(pil(recoded(lname, *SMALL, shape, restart)), want), (lname, shape, restart)
        if not lname.startswith("gray"):
            src = source(lname, *SMALL)[0]
            for shape in ("ladder", "anti", "sub7", "random0"):
                tabs = dict(enumerate(tables_of(lname, *SMALL, shape)))
                for twin in jw.script_twins(src, sl.oracle_std(src), ["Y;Cb;Cr", "Cb Cr;Y", "Y Cb;Cr"], tables=tabs):
                    assert np.array_equal(pil(twin), want), (lname, shape)
    assert n == len(LAYS) * len(SHAPES) and any(one_bit(l, *SMALL, s) for l in LAYS for s in SHAPES)
    for which in CONSTRUCTED:                                         # (no source to compare with: libjpeg reads them without a warning)
        assert pil(constructed(which, 16, 16)[0]).shape == (128, 128, 3)


# ---- the kernels' per-lane routine on the CPU ---------------------------------------------------------------------------------------
def emul_two_pass(lib, data, mode=0, sub_bits=0, cap=70000):
    out = np.zeros((cap, 64), np.int16)
    nb, st = ctypes.c_size_t(), (ctypes.c_int * 8)()
    rc = lib.emul_decode_coefs_sub(data, len(data), 0, mode, sub_bits, out.ctypes.data, cap, ctypes.byref(nb), st)
    return rc, out[: min(nb.value, cap)].copy(), list(st)


def emul_single(lib, data, mode=0, sub_bits=0, warm=1024, head=32, cp_bits=1024, cap=70000):
    out = np.zeros((cap, 64), np.int16)
    nb, st = ctypes.c_size_t(), (ctypes.c_int * 8)()
    rc = lib.emul_single_decode_cp(data, len(data), 0, mode, sub_bits, warm, head, cp_bits, out.ctypes.data, cap, ctypes.byref(nb), st)
    return rc, out[: min(nb.value, cap)].copy(), list(st)


SINGLE_SETTINGS = [(0, 256), (1024, 1024), (2048, 512), (512, 2048)]      # (warm-up, checkpoint distance), as tests/test_host.py


def emul_problems(lib, data, want, single=True):
    """every emulated configuration that does not give `want`: the two-pass sequence at the planned cut, 1024 and 256 bits in both
    modes, the single decode at the four settings in both modes"""
    bad = []
    for sub in (0, 1024, 256):
        for mode in (0, 1):
            rc, coefs, st = emul_two_pass(lib, data, mode, sub)
            if rc != 0 or not np.array_equal(coefs, want):
                bad.append(("two-pass", sub, mode, rc, st))
    for warm, cp in SINGLE_SETTINGS if single else ():
        for mode in (0, 1):
            rc, coefs, st = emul_single(lib, data, mode, 0, warm, 32, cp)
            if rc != 0 or not np.array_equal(coefs, want):
                bad.append(("single", warm, cp, mode, rc, st))
    return bad


@pytest.mark.parametrize("lname", LAYS)
def test_emulated_decode_of_every_shape(orc, emul_lib, lname):
    """Every shape on every layout: the oracle and every emulated configuration give the writer's coefficients."""
    want = writer_t0(lname, *SMALL)
    bad = []
    for shape in SHAPES:
        data = recoded(lname, *SMALL, shape)
        ref = orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=one_bit(lname, *SMALL, shape))
        if not np.array_equal(orc.interleave(ref), want):
            bad.append((shape, "oracle"))
        bad += [(shape,) + p for p in emul_problems(emul_lib, data, want)]
    assert bad == [], bad


def test_emulated_decode_of_the_trial_pictures(orc, emul_lib):
    """640 x 480 4:2:0 at quality 90, the four shapes of the first trial: three subsequences' worth of every configuration."""
    want = writer_t0("Y22_Cb11_Cr11", *TRIAL)
    bad = []
    for shape in TRIAL_SHAPES:
        data = recoded("Y22_Cb11_Cr11", *TRIAL, shape)
        if not np.array_equal(orc.interleave(sl.oracle_std(data)), want):
            bad.append((shape, "oracle"))
        bad += [(shape,) + p for p in emul_problems(emul_lib, data, want)]
    assert bad == [], bad


def emit_fits(tables):
    """ImagePlan::emit_fits restated: a column of the emitting pass is sized for one word -- stream entry or block word -- per two
    bits.  An entry takes two bits at least and a block two more, a DC code and an end-of-block, unless the block ends without
    one: after 63 coded coefficients (64 words in d + 63 e bits, d the shortest DC code, e the cheapest entry), or, where runs are
    clamped -- a corrupt stream, a decode from a wrong state -- after four symbols of run 15 (5 words in d + 4 e bits, the tighter
    case).  Either is more than a word per two bits exactly when d = 1 and e = 2: a 1-bit DC code and a 1-bit code for an AC
    symbol of size 1."""
    for dc, ac in tables:
        d = min(ln for _, ln in jw.huff_codes(*dc).values())
        e = min(ln + (s & 15) for s, (_, ln) in jw.huff_codes(*ac).items() if s & 15)
        assert (d + 63 * e < 128) == (2 * 5 > d + 4 * e) == (d == 1 and e == 2)
        if d == 1 and e == 2:
            return False
    return True


def test_pictures_too_dense_for_the_emitting_pass_are_planned_for_two_passes(emul_lib):
    """mjx_plan.cpp marks the pictures whose tables allow more than one word per two bits (emit_fits), and the planner's mark is the
    rule above for every shape and every constructed picture; both kinds of shape occur."""
    got = {}
    for lname in LAYS:
        for shape in SHAPES:
            want = emit_fits(tables_of(lname, *SMALL, shape))
            got[(lname, shape)] = want
            assert table_set(emul_lib, recoded(lname, *SMALL, shape))[3] == want, (lname, shape)
    assert not got[("Y22_Cb11_Cr11", "ladder")] and got[("Y22_Cb11_Cr11", "k2")] and got[("Y22_Cb11_Cr11", "anti")]
    assert sum(got.values()) >= len(got) * 3 // 4, sorted(k for k, v in got.items() if not v)
    for which, want in (("bits2_block", True), ("bits2_entry", False), ("bits2_dense", False), ("bits27", True)):
        assert table_set(emul_lib, constructed(which, 40, 30)[0])[3] == want, which
    assert table_set(emul_lib, source("Y22_Cb11_Cr11", *SMALL)[0])[3]                          # Annex K


def test_emulated_decode_of_the_constructed_pictures(orc, emul_lib):
    """Two bits per block (180 x 180 flat blocks), two bits per stream entry (60 x 60 blocks), the same with an end-of-block now
    and then, and 27-bit symbols: the oracle and every emulated configuration give the writer's blocks.

    The two-bits-per-entry picture never synchronises -- every bit string is a valid sequence of its two symbols from every
    state -- so the merge rounds put one subsequence right per round: 128 rounds for 128 subsequences at the planned cut, 441 for
    447 at 1024 bits.  The emulated single decode used to stop after 64 rounds and report MJX_ERR_BAD_HUFFMAN (status 4) for it, a
    limit the device does not have (mjx_batch_wait keeps repairing); it now allows a round per subsequence, and
    the picture is exact.  With no head room a prefix that grows cannot be written (st[6] == 14: the picture falls back to the
    two-pass kernels on the device); on this picture prefixes grow by up to 22 entries.

    At 232 x 232 blocks (8192-bit subsequences, the cut of the emitting pass) a column of these two pictures would take 4128 words
    where it holds 4124: the emulated single decode says so (st[6] == 14) -- before this check it wrote null entries over block words
    and returned garbage (st[6] == 9) for the picture that synchronises -- and the planner keeps such pictures off that path
    (emit_fits); the two-pass sequence is exact."""
    for which, bx, by in (("bits2_block", 180, 180), ("bits2_entry", 60, 60), ("bits2_dense", 60, 60), ("bits27", 48, 40)):
        data, blk = constructed(which, bx, by)
        ref = orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True)
        assert np.array_equal(ref.coefs[0], blk), which
        bad = emul_problems(emul_lib, data, blk)
        assert bad == [], (which, bad)
    data, blk = constructed("bits2_entry", 60, 60)
    for sub in (0, 1024):
        rc, _, st = emul_two_pass(emul_lib, data, 0, sub)
        print("two bits per entry: %d rounds for %d subsequences" % (st[1], st[0]))
        assert rc == 0 and st[0] > 64 and st[0] * 0.95 <= st[1] <= st[0] + 1, st
    rc, coefs, st = emul_single(emul_lib, data, 0, 0, 2048, 130, 1024)                  # (more head room than there is: clamped)
    assert rc == 0 and np.array_equal(coefs, blk) and st[0] * 0.95 <= st[1] <= st[0] + 1 and 0 < st[5] <= 32 * 8, st
    rc, _, st = emul_single(emul_lib, data, 0, 0, 2048, 0, 1024)
    assert rc == 4 and st[6] == 14, (rc, st)
    for which in ("bits2_dense", "bits2_entry"):
        data, blk = constructed(which, 232, 232)
        rc, coefs, st = emul_two_pass(emul_lib, data, 0, 0)
        assert rc == 0 and np.array_equal(coefs, blk), (which, st)
        rc, _, st = emul_single(emul_lib, data, 0, 0, 2048, 64, 1024)
        assert rc == 4 and st[6] == 14, (which, rc, st)


def test_entropy_routine_under_asan_ubsan_with_every_shape(tmp_path):
    """The shapes through the sanitizer build of the emulation (tools/sanitize/asan_emul_fuzz.cpp), both kernel sequences: each file
    as it is, then with mutated tables and scan bytes.  Every file as it is must decode clean (the driver counts those apart)."""
    import test_sanitizers as ts
    exe = ts.build(tmp_path, "asan_emul_fuzz", ["g++", "-std=c++17"] + ts.ASAN + ts.INC + [
        os.path.join(ts.SAN, "asan_emul_fuzz.cpp"), os.path.join(ROOT, "tests", "emul", "huff_emul.cpp"),
        os.path.join(ts.CSRC, "mjx_parse.cpp"), os.path.join(ts.CSRC, "mjx_plan.cpp"), os.path.join(ts.CSRC, "mjx_lut.cpp")])
    files = []
    for lname, (w, h) in (("Y22_Cb11_Cr11", (64, 48)), ("gray21", (37, 29))):
        for shape in SHAPES:
            p = tmp_path / ("%s_%s.jpg" % (lname, shape))
            p.write_bytes(recoded(lname, w, h, shape))
            files.append(str(p))
    for which in CONSTRUCTED:
        p = tmp_path / (which + ".jpg")
        p.write_bytes(constructed(which, 40, 30)[0])
        files.append(str(p))
    out = ts.run(exe, ["4"] + files)
    w = out.split()
    assert "asan emul fuzz:" in out and int(w[3]) == 4 * len(files) and int(w[7]) == len(files) and int(w[9]) == len(files), out


def test_numpy_entropy_coder_writes_the_same_bytes():
    """jpegwriter.encode_scan_np (what layout_jpeg and recode_huffman code with) against the loop it replaces, encode_scan: every
    shape, restart intervals, runs of more than 16 zeros, values of every size."""
    for lname, (w, h), rst in (("Y22_Cb11_Cr11", SMALL, None), ("Y21_Cb12_Cr11", SMALL, 5), ("gray21", (37, 29), 1), ("Y11_Cb11_Cr11", (64, 48), 1)):
        ref = sl.oracle_std(source(lname, w, h)[0])
        blocks, owner, bpm = jw.scan_blocks(ref)
        for shape in SHAPES:
            tabs = tables_of(lname, w, h, shape)
            dcc = {c: jw.huff_codes(*t[0]) for c, t in enumerate(tabs)}
            acc = {c: jw.huff_codes(*t[1]) for c, t in enumerate(tabs)}
            assert jw.encode_scan(blocks, owner, dcc, acc, (rst or 0) * bpm) == jw.encode_scan_np(blocks, owner, dcc, acc, (rst or 0) * bpm), (lname, shape)
    blk = np.zeros((6, 64), np.int64)
    blk[0, 63], blk[1, 40], blk[1, 17], blk[3, 0], blk[4, 1], blk[4, 62], blk[5, 0] = -3, 7, 1, -5, 1023, -1023, 2047
    ak = jw._annex_k_tables()
    d, a = {0: jw.huff_codes(*ak[(0, 0)])}, {0: jw.huff_codes(*ak[(1, 0)])}
    for rst in (0, 1, 2):
        assert jw.encode_scan(blk, [0] * 6, d, a, rst) == jw.encode_scan_np(blk, [0] * 6, d, a, rst), rst


def ff_share(mjx, data):
    scan = mjx.ParsedScan(data)
    try:
        a = np.frombuffer(scan.scan_bytes(), np.uint8)
    finally:
        scan.close()
    return float((a == 0xff).mean())


DESTUFF_SHAPES = ["anti", "random4", "ladder", "k2"]


def test_which_shapes_raise_the_share_of_ff_bytes(mjx):
    """What test_device_destuff relies on.  Share of 0xFF among the de-stuffed bytes of the 640 x 480 4:2:0 scan, measured: Annex K
    0.0098, k2 0.0023, ladder 0.023, anti 0.047, random4 0.065 (its frequent symbols sit on codes of many 1-bits) -- and none at all
    for edge9, edge10 and edge9_10: 162 codes of 9 or 10 bits all begin with a 0-bit, so eight 1-bits in a row need value bits alone.
    The `edge` shapes therefore say nothing about de-stuffing; `anti` and `random4` do."""
    share = {s: ff_share(mjx, recoded("Y22_Cb11_Cr11", *TRIAL, s)) for s in DESTUFF_SHAPES + ["edge9", "edge10", "edge9_10"]}
    base = ff_share(mjx, source("Y22_Cb11_Cr11", *TRIAL)[0])
    print(base, share)
    assert share["anti"] > 4 * base and share["random4"] > 4 * base and share["anti"] > 0.04, (base, share)
    assert max(share["edge9"], share["edge10"], share["edge9_10"]) < base / 10, share


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def check(mjx, b, i, data, want_t0):
    """None, or what is wrong with picture i of the batch: status OK, T0 the writer's and the oracle's bit for bit, RGB within TOL"""
    if b.status(i) != mjx.OK:
        return ("status", b.status(i))
    ref = sl.oracle_std(data)
    got = b.coefs(i)
    if not np.array_equal(got, want_t0):
        return ("T0 (writer)",)
    if not np.array_equal(got, orc_mod.interleave(ref)):
        return ("T0 (oracle)",)
    return sl.rgb_problem(b.rgb(i), ref.rgb)


def small_cases():
    """[(name, bytes, the writer's T0)]: every shape on every layout, and the four constructed pictures"""
    out = [("%s %s" % (lname, shape), recoded(lname, *SMALL, shape), writer_t0(lname, *SMALL)) for lname in LAYS for shape in SHAPES]
    out += [(which,) + constructed(which, 40, 30) for which in CONSTRUCTED]
    return out


@pytest.mark.gpu
def test_every_shape_one_picture_per_batch(mjx, gpu_ctx):
    """The latency path (short subsequences, k_huff_merge_loop) with one table set per batch."""
    bad = []
    for cname, data, want in small_cases():
        b, scans = sl.decode_batch(mjx, gpu_ctx, [data], keep_coefs=True)
        try:
            p = check(mjx, b, 0, data, want)
        finally:
            sl.close_all(b, scans)
        if p:
            bad.append((cname, p))
    assert bad == [], bad


@pytest.mark.gpu
def test_every_shape_in_one_mixed_batch(mjx, gpu_ctx):
    """All shapes and the constructed pictures in one batch cut into chunks of three: the table pool holds a different set per picture."""
    cases = small_cases()
    for keep in (True, False):
        b, scans = sl.decode_batch(mjx, gpu_ctx, [c[1] for c in cases], keep_coefs=keep, chunk_images=3)
        try:
            if keep:
                bad = [(cn, p) for i, (cn, d, want) in enumerate(cases) for p in [check(mjx, b, i, d, want)] if p]
            else:
                bad = [(cn, p) for i, (cn, d, _) in enumerate(cases) for p in [sl.check_std(mjx, b, i, d, coefs=False)] if p]
        finally:
            sl.close_all(b, scans)
        assert bad == [], (keep, bad)


# (a child process per environment: every picture alone, with its coefficients, in a profiled context; it compares with the oracle
# itself and reports per picture the status, what is wrong, how often the emitting kernels ran, the batch's unconverged runs and a
# digest of the picture and its coefficients)
_CHILD = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import __graft_entry__ as ge
import oracle_binding as orc_mod
import test_sampling_layouts as sl
mjx = ge.load_package()
job = json.load(open(%(job)r))
ctx = mjx.Context(0, profiling=True, throughput_plan=job['throughput'])
res = []
for p in job['paths']:
    data = open(p, 'rb').read()
    scan = mjx.ParsedScan(data)
    b = mjx.Batch(ctx, [scan], keep_coefs=True)
    b.kernel_ms(reset=True)
    b.decode(); b.wait()
    k = b.kernel_ms()
    r = dict(status=b.status(0), emit=k['huff_emit'][1], prefix=k['huff_prefix'][1], write=k['huff_write'][1], unconverged=b.unconverged_runs(),
             subsequences=b.geometry()['subsequences'], problem=None, sha=None)
    if r['status'] == 0:
        rgb, coefs = b.rgb(0), b.coefs(0)
        ref = sl.oracle_std(data)
        r['sha'] = hashlib.sha1(rgb.tobytes() + coefs.tobytes()).hexdigest()
        r['problem'] = ('T0',) if not np.array_equal(coefs, orc_mod.interleave(ref)) else sl.rgb_problem(rgb, ref.rgb)
    res.append(r)
    b.close(); scan.close()
print(json.dumps(res))
"""


def run_alone(tmp_path, tag, datas, env_set=None, throughput=True, timeout=600):
    """every file alone in a child process with `env_set`; -> [dict(status, problem, emit, prefix, write, unconverged, subsequences, sha)]"""
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s_%d.jpg" % (tag, i))
        if not p.exists():
            p.write_bytes(d)
        paths.append(str(p))
    job = tmp_path / ("%s.json" % tag)
    job.write_text(json.dumps(dict(paths=paths, throughput=throughput)))
    script = tmp_path / ("%s.py" % tag)
    script.write_text(_CHILD % dict(root=ROOT, job=str(job)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


BIG, BIG_NOISE = (1920, 1080), 12.0
SWITCHES = [{}, {"MJX_SINGLE_DECODE": "0"}, {"MJX_EMIT_MIN_SUB_BITS": "256", "MJX_EMIT_CP_BITS": "256", "MJX_EMIT_WARM_BITS": "0"},
            {"MJX_STREAMS": "1"}]


@pytest.mark.gpu
def test_every_shape_at_1080p_through_the_emitting_pass_and_its_switches(mjx, tmp_path):
    """1920 x 1080 4:2:0 at quality 90 with noise (scans of 1.2 MB with the K.2 tables to 4.3 MB with `anti`), and one 3840 x 2160
    picture with `anti` tables, each alone in a context with the throughput plan: by default every one takes the emitting pass
    (k_huff_emit runs, counted) -- except the shapes with a 1-bit DC code and a 1-bit code for an AC symbol of size 1 (`ladder`,
    some of the random ones), whose tables allow more words than a column of that pass holds (emit_fits): those must take the
    two-pass kernels --, with MJX_SINGLE_DECODE=0 none does, and the four environments give the same bytes -- T0 the
    writer's and the oracle's, RGB within TOL.  No run is left unconverged with a warm-up; without one (MJX_EMIT_WARM_BITS=0)
    every lane starts from the guess "a block begins here", the rounds may need more than the six that are enqueued and
    mjx_batch_wait then repairs the chunk: the count is printed, the bytes must be the same."""
    names = ["%s 1080p" % s for s in SHAPES] + ["anti 4K"]
    datas = [recoded("Y22_Cb11_Cr11", *BIG, s, None, QUALITY, BIG_NOISE) for s in SHAPES]
    datas.append(recoded("Y22_Cb11_Cr11", 3840, 2160, "anti", None, QUALITY, BIG_NOISE))
    fits = {"%s 1080p" % s: emit_fits(tables_of("Y22_Cb11_Cr11", *BIG, s, QUALITY, BIG_NOISE)) for s in SHAPES}
    fits["anti 4K"] = True
    assert sum(fits.values()) >= 30 and not all(fits.values()), fits
    bad = []
    for cn, d, (w, h) in zip(names, datas, [BIG] * len(SHAPES) + [(3840, 2160)]):
        if not np.array_equal(orc_mod.interleave(sl.oracle_std(d)), writer_t0("Y22_Cb11_Cr11", w, h, QUALITY, BIG_NOISE)):
            bad.append((cn, "the oracle's T0 is not the writer's"))
    runs = [run_alone(tmp_path, "big%d" % k, datas, e) for k, e in enumerate(SWITCHES)]
    for e, res in zip(SWITCHES, runs):
        for cn, r, r0 in zip(names, res, runs[0]):
            if r["status"] != 0 or r["problem"]:
                bad.append((cn, e, r["status"], r["problem"]))
            elif r["sha"] != r0["sha"]:
                bad.append((cn, e, "bytes differ from the default's"))
            if (r["emit"] > 0) != (e.get("MJX_SINGLE_DECODE") != "0" and fits[cn]):
                bad.append((cn, e, "huff_emit launches", r["emit"]))
            if not fits[cn] and r["write"] == 0:
                bad.append((cn, e, "huff_write launches", r["write"]))
            if r["unconverged"] and "MJX_EMIT_WARM_BITS" not in e:
                bad.append((cn, e, "unconverged runs", r["unconverged"]))
        print(e, "unconverged runs:", sum(r["unconverged"] for r in res), "huff_emit launches:", sum(r["emit"] for r in res))
    assert bad == [], bad


@pytest.mark.gpu
def test_device_destuff_and_the_front_doors(mjx, gpu_ctx):
    """mjx_decode_batch from bytes with the scans de-stuffed on the host and on the device, and the pool: `anti` and `random4` scans
    hold 5 % and 7 % of 0xFF bytes (test_which_shapes_raise_the_share_of_ff_bytes), every other shape rides along."""
    cases = [("%s %s" % (lname, shape), recoded(lname, *SMALL, shape), writer_t0(lname, *SMALL)) for lname in LAYS for shape in SHAPES]
    cases += [("trial %s" % s, recoded("Y22_Cb11_Cr11", *TRIAL, s), writer_t0("Y22_Cb11_Cr11", *TRIAL)) for s in DESTUFF_SHAPES]
    cases += [(which,) + constructed(which, 40, 30) for which in CONSTRUCTED]
    datas = [c[1] for c in cases]
    bad = []
    for dd in (False, True, None):
        b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd, keep_coefs=True)
        try:
            bad += [(cn, "mjx_decode_batch", dd, st[i], p) for i, (cn, d, want) in enumerate(cases)
                    for p in [check(mjx, b, i, d, want)] if p or st[i] != mjx.OK]
        finally:
            b.close()
    pool = mjx.Pool([0])
    try:
        for dd in (False, True):
            r = pool.decode_batch(datas, device_destuff=dd)
            try:
                bad += [(cn, "pool", dd, r.status[i]) for i, (cn, d, _) in enumerate(cases)
                        if r.status[i] != mjx.OK or sl.rgb_problem(r.rgb(i), sl.oracle_std(d).rgb)]
            finally:
                r.close()
    finally:
        pool.close()
    assert bad == [], bad


HARD_SHAPES = ["ladder", "anti", "sub7", "random0", "random4", "random11"]
SCRIPTS3 = ["Y;Cb;Cr", "Cb Cr;Y", "Y Cb;Cr"]


@pytest.mark.gpu
def test_restart_intervals_with_hard_tables(mjx, gpu_ctx):
    """DRI of 1, 5 and one MCU row: T0 and RGB as the oracle's, and the picture of the file without restart intervals bit for bit."""
    cases, plain = [], []
    for lname in LAYS:
        for shape in HARD_SHAPES:
            for r in (1, 5, sl.mcux_of(lname, SMALL[0])):
                cases.append(("%s %s dri%d" % (lname, shape, r), recoded(lname, *SMALL, shape, r), writer_t0(lname, *SMALL)))
                plain.append(recoded(lname, *SMALL, shape))
    bad = []
    b, scans = sl.decode_batch(mjx, gpu_ctx, [c[1] for c in cases], keep_coefs=True)
    try:
        got = []
        for i, (cn, d, want) in enumerate(cases):
            p = check(mjx, b, i, d, want)
            if p:
                bad.append((cn, p))
            got.append(b.rgb(i) if b.status(i) == mjx.OK else None)
    finally:
        sl.close_all(b, scans)
    want = sl.gpu_pictures(mjx, gpu_ctx, plain, 1)
    bad += [(cn, "vs plain") for (cn, _, _), g, wnt in zip(cases, got, want) if g is not None and not sl.same(g, wnt)]
    assert bad == [], bad


@pytest.mark.gpu
def test_multiscan_scripts_with_hard_tables(mjx, gpu_ctx):
    """The same tables through multi-scan files (script_twins tables=<dict>): one scan per component, Cb and Cr together in front of
    Y, Y and Cb together in front of Cr.  Status OK and the GPU picture of the interleaved Annex-K source bit for bit, alone and
    in one batch."""
    cases = []
    for lname in LAYS[:3]:
        src = source(lname, *SMALL)[0]
        for shape in HARD_SHAPES:
            tabs = dict(enumerate(tables_of(lname, *SMALL, shape)))
            for script, tw in zip(SCRIPTS3, jw.script_twins(src, sl.oracle_std(src), SCRIPTS3, tables=tabs)):
                cases.append(("%s %s %s" % (lname, shape, script), src, tw))
    srcs = list(dict.fromkeys(c[1] for c in cases))
    want = dict(zip(srcs, sl.gpu_pictures(mjx, gpu_ctx, srcs, 1)))
    bad = []
    got = sl.gpu_pictures(mjx, gpu_ctx, [c[2] for c in cases], 1)
    bad += [(cn, "mixed batch", g if not isinstance(g, np.ndarray) else "rgb") for (cn, src, _), g in zip(cases, got) if not sl.same(g, want[src])]
    for cn, src, tw in cases:
        (g,) = sl.gpu_pictures(mjx, gpu_ctx, [tw], 1)
        if not sl.same(g, want[src]):
            bad.append((cn, "alone", g if not isinstance(g, np.ndarray) else "rgb"))
    assert bad == [], bad


@pytest.mark.gpu
def test_ref_compat_with_every_shape_the_reference_can_read(mjx, gpu_ctx):
    """REF_COMPAT on 4:2:0 (640 x 480: whole MCUs, the reference panics in placing the blocks of partial ones) and 4:4:4 for the
    shapes without a 1-bit code (the reference cannot read one): the oracle's reference layout decodes them, and T0 and RGB equal it."""
    cases = [("%s %s" % (lname, shape), recoded(lname, w, h, shape)) for lname, (w, h) in (("Y22_Cb11_Cr11", TRIAL), ("Y11_Cb11_Cr11", SMALL))
             for shape in SHAPES if not one_bit(lname, w, h, shape)]
    assert len(cases) >= 2 * 20
    b, scans = sl.decode_batch(mjx, gpu_ctx, [c[1] for c in cases], keep_coefs=True, layout=mjx.LAYOUT_REF_COMPAT)
    bad = []
    try:
        for i, (cn, d) in enumerate(cases):
            rc, ref = sl.oracle_ref(d)
            if rc != orc_mod.OK:
                bad.append((cn, "the oracle's reference layout refuses it", rc))
            elif b.status(i) != mjx.OK:
                bad.append((cn, "status", b.status(i)))
            elif not np.array_equal(b.coefs(i), orc_mod.interleave(ref)):
                bad.append((cn, "T0"))
            elif sl.rgb_problem(b.rgb(i), ref.rgb):
                bad.append((cn, sl.rgb_problem(b.rgb(i), ref.rgb)))
    finally:
        sl.close_all(b, scans)
    assert bad == [], bad


@pytest.mark.gpu
def test_constructed_pictures_where_the_emitting_pass_is_eligible(mjx, tmp_path):
    """The constructed pictures with scans of 0.83 MB and more, each alone in a context with the throughput plan, in a child process
    with a time limit: status OK, T0 the writer's and the oracle's, RGB within TOL.
      * 27-bit symbols (192 x 192 blocks): the emitting pass runs, nothing falls back.
      * two bits per stream entry (232 x 232 blocks, 3.4 million symbols), and the same with an end-of-block in every 16th block:
        their tables allow more words than a column of the emitting pass holds, so they are planned for the two-pass kernels
        (emit_fits; k_huff_emit does not run, k_huff_write does).  The first never synchronises: its rounds put one subsequence right
        at a time, more than the six that are enqueued, mjx_batch_wait repairs the chunk and
        mjx_batch_unconverged_runs counts it; serial decode at 0.29 us per symbol (s11) is 1 s.  The second converges in time.
      * two bits per block would need 14 752 x 14 752 pixels for such a scan; it is decoded at 1440 x 1440 with
        MJX_EMIT_MIN_SUB_BITS=256, which makes its 8 KB scan eligible."""
    pics = [constructed("bits27", 192, 192), constructed("bits2_entry", 232, 232), constructed("bits2_dense", 232, 232),
            constructed("bits2_block", 180, 180)]
    for d, blk in pics:
        assert np.array_equal(orc_mod.interleave(sl.oracle_std(d)), blk)
    res = run_alone(tmp_path, "cons", [p[0] for p in pics[:3]], timeout=300)
    res += run_alone(tmp_path, "consb", [pics[3][0]], {"MJX_EMIT_MIN_SUB_BITS": "256"}, timeout=300)
    print(res)
    bad = [(k, r["status"], r["problem"]) for k, r in enumerate(res) if r["status"] != 0 or r["problem"]]
    assert bad == [], (bad, res)
    assert res[0]["emit"] > 0 and res[0]["write"] == 0 and res[0]["unconverged"] == 0, res[0]
    assert res[1]["emit"] == 0 and res[1]["write"] > 0 and res[1]["unconverged"] >= 1, res[1]
    assert res[2]["emit"] == 0 and res[2]["write"] > 0 and res[2]["unconverged"] == 0, res[2]
    assert res[3]["emit"] > 0 and res[3]["write"] == 0 and res[3]["unconverged"] == 0, res[3]


_CHILD_TILE = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import __graft_entry__ as ge
import oracle_binding as orc_mod
import test_sampling_layouts as sl
mjx = ge.load_package()
job = json.load(open(%(job)r))
ctx = mjx.Context(0, profiling=True, throughput_plan=True)
datas = [open(p, 'rb').read() for p in job['paths']]
res = []
for group, times in job['groups']:
    scans = [mjx.ParsedScan(datas[i]) for i in group]
    b = mjx.Batch(ctx, scans, keep_coefs=True)
    t = b.tile(times)
    t.kernel_ms(reset=True)
    t.decode(); t.wait()
    k = t.kernel_ms()
    r = dict(emit=k['huff_emit'][1], write=k['huff_write'][1], unconverged=t.unconverged_runs(), n=len(t), problems=[])
    for i in range(len(t)):
        d = datas[group[i %% len(group)]]
        ref = sl.oracle_std(d)
        if t.status(i) != 0:
            r['problems'].append((i, 'status', t.status(i)))
        elif not np.array_equal(t.coefs(i), orc_mod.interleave(ref)):
            r['problems'].append((i, 'T0'))
        elif sl.rgb_problem(t.rgb(i), ref.rgb):
            r['problems'].append((i, sl.rgb_problem(t.rgb(i), ref.rgb)))
    res.append(r)
    t.close(); b.close()
    for sc in scans:
        sc.close()
print(json.dumps(res))
"""


@pytest.mark.gpu
def test_tiled_batches_keep_dense_pictures_off_the_emitting_pass(mjx, tmp_path):
    """mjx_batch_tile rebuilds its plans from the source batch's device images, which hold no Huffman tables: the mark of a picture
    too dense for the emitting pass (emit_fits) must come along.  In a context with the throughput plan: the two-bits-per-entry
    picture with synchronisation points (232 x 232 blocks) tiled four times never runs k_huff_emit and every copy is exact; tiled
    twice together with two ordinary 1080p pictures (K.2 and `anti` tables), which do take the emitting pass, every copy of all
    three is exact -- status OK, T0 the writer's and the oracle's, RGB within TOL."""
    dense, blk = constructed("bits2_dense", 232, 232)
    assert np.array_equal(orc_mod.interleave(sl.oracle_std(dense)), blk)
    datas = [dense] + [recoded("Y22_Cb11_Cr11", *BIG, s, None, QUALITY, BIG_NOISE) for s in ("k2", "anti")]
    for d in datas[1:]:
        assert np.array_equal(orc_mod.interleave(sl.oracle_std(d)), writer_t0("Y22_Cb11_Cr11", *BIG, QUALITY, BIG_NOISE))
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("tile_%d.jpg" % i)
        p.write_bytes(d)
        paths.append(str(p))
    job = tmp_path / "tile.json"
    job.write_text(json.dumps(dict(paths=paths, groups=[([0], 4), ([0, 1, 2], 2), ([1, 2], 2)])))
    script = tmp_path / "tile.py"
    script.write_text(_CHILD_TILE % dict(root=ROOT, job=str(job)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    alone, mixed, ordinary = json.loads(r.stdout.strip().splitlines()[-1])
    print(alone, mixed, ordinary)
    assert alone["n"] == 4 and mixed["n"] == 6 and ordinary["n"] == 4
    assert alone["problems"] == [] and mixed["problems"] == [] and ordinary["problems"] == [], (alone, mixed, ordinary)
    assert alone["emit"] == 0 and alone["write"] > 0, alone
    assert ordinary["emit"] > 0 and ordinary["write"] == 0, ordinary              # (the control: tiled ordinary pictures do emit)
    assert mixed["emit"] > 0 and mixed["write"] > 0, mixed

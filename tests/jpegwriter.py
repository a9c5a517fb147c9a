"""Minimal baseline-JPEG *writer* for tests (test infrastructure, no reference counterpart: the reference only decodes).

Builds files the synthetic generator cannot: pictures from chosen coefficient blocks (the T1 per-block tier),
custom Huffman tables (every run/size symbol, including the degenerate `0x?0` ones of SURVEY Q9), and entropy-coded
segments that are syntactically valid symbol sequences but semantically corrupt (runs past the end of a block), on which
the reference does not panic but clamps (src/jpeg/huffman.rs:170-189), and pictures of every sampling layout (layout_jpeg).
Only markers the reference parses are written (src/jpeg/mod.rs:166-179): SOI, DQT, SOF0, DHT, SOS, EOI -- and DRI with RSTn
markers where a test asks for restart intervals.
"""
import os
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63]       # src/jpeg/decoder.rs:404-407


def huff_codes(bits, vals):
    """T.81 Fig. C.2 (src/jpeg/huffman.rs:80-98): symbol -> (code, length)."""
    codes, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            codes[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return codes


def tables_from_jpeg(data):
    """DHT tables of a file: {(class, slot): (bits[16], vals)}."""
    out, i = {}, 2
    while i + 4 <= len(data) and data[i] == 0xff:
        m = data[i + 1]
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        p = data[i + 4:i + 2 + ln]
        if m == 0xc4:
            j = 0
            while j < len(p):
                bits = list(p[j + 1:j + 17])
                nv = sum(bits)
                out[(p[j] >> 4, p[j] & 15)] = (bits, list(p[j + 17:j + 17 + nv]))
                j += 17 + nv
        if m == 0xda:
            break
        i += 2 + ln
    return out


class BitWriter:
    """MSB-first bit packer with FF -> FF00 byte stuffing (undone by src/jpeg/mod.rs:371-385)."""

    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, code, ln):
        if ln == 0:
            return
        self.acc = (self.acc << ln) | (code & ((1 << ln) - 1))
        self.n += ln
        self.bits += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xff
            self.out.append(b)
            if b == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)       # pad with ones (T.81 F.1.2.3)
        return bytes(self.out)


def magnitude(v):
    a = abs(int(v))
    s = a.bit_length()
    return s, (int(v) if v >= 0 else int(v) + (1 << s) - 1)


def encode_blocks(blocks, comp_of_block, dc_codes, ac_codes):
    """Valid entropy coding of `blocks` (int [n, 64], zig-zag order, absolute DC) in the given order; comp_of_block[k] selects
    the predictor and the code tables of block k."""
    w, pred = BitWriter(), {}
    for k, blk in enumerate(blocks):
        c = comp_of_block[k]
        s, bits = magnitude(int(blk[0]) - pred.get(c, 0))
        pred[c] = int(blk[0])
        w.put(*dc_codes[c][s])
        w.put(bits, s)
        run = 0
        last = max([i for i in range(1, 64) if blk[i]], default=0)
        for i in range(1, last + 1):
            if blk[i] == 0:
                run += 1
                continue
            while run > 15:
                w.put(*ac_codes[c][0xf0])
                run -= 16
            s, bits = magnitude(blk[i])
            w.put(*ac_codes[c][(run << 4) | s])
            w.put(bits, s)
            run = 0
        if last < 63:
            w.put(*ac_codes[c][0x00])
    return w.flush()


def write_jpeg(width, height, comps, qts, dhts, entropy, qt16=False, restart_interval=0):
    """comps: [(id, h, v, tq, td, ta)] in frame = scan order; qts: {slot: 64 values in zig-zag (file) order};
    dhts: {(class, slot): (bits, vals)}; entropy: the stuffed entropy-coded segment (with its RSTn markers);
    qt16: every table with 16-bit entries, or the set of slots whose tables have them; restart_interval: > 0 writes a DRI segment in
    front of the scan."""
    out = bytearray(b"\xff\xd8")
    for slot, q in sorted(qts.items()):
        if (slot in qt16) if isinstance(qt16, (set, frozenset)) else qt16:
            out += b"\xff\xdb" + struct.pack(">H", 2 + 129) + bytes([0x10 | slot]) + b"".join(struct.pack(">H", int(v)) for v in q)
        else:
            out += b"\xff\xdb" + struct.pack(">H", 2 + 65) + bytes([slot]) + bytes(int(v) for v in q)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * len(comps), 8, height, width, len(comps))
    for cid, h, v, tq, _, _ in comps:
        out += bytes([cid, (h << 4) | v, tq])
    for (tc, th), (bits, vals) in sorted(dhts.items()):
        out += b"\xff\xc4" + struct.pack(">H", 2 + 17 + len(vals)) + bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
    if restart_interval:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart_interval)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(comps), len(comps))
    for cid, _, _, _, td, ta in comps:
        out += bytes([cid, (td << 4) | ta])
    out += bytes([0, 63, 0]) + entropy + b"\xff\xd9"
    return bytes(out)


def grey_jpeg_from_blocks(blocks_zz, blocks_x, qt_zz, tables, qt16=False):
    """A greyscale picture whose 8x8 blocks (raster order, blocks_x per row) carry exactly the coefficients given
    (int [n, 64] zig-zag order, absolute DC, before dequantisation)."""
    n = len(blocks_zz)
    assert n % blocks_x == 0
    dc = {0: huff_codes(*tables[(0, 0)])}
    ac = {0: huff_codes(*tables[(1, 0)])}
    ent = encode_blocks(blocks_zz, [0] * n, dc, ac)
    return write_jpeg(blocks_x * 8, (n // blocks_x) * 8, [(1, 1, 1, 0, 0, 0)], {0: qt_zz},
                      {(0, 0): tables[(0, 0)], (1, 0): tables[(1, 0)]}, ent, qt16=qt16)


def jpeg_from_blocks(blocks, hv, mcux, mcuy, qts, tables, qt16=False, width=None, height=None, restart=None):
    """grey_jpeg_from_blocks for any sampling layout: an interleaved baseline file whose blocks carry exactly the coefficients
    given (tests/test_stageb_arithmetic.py).

    blocks: int [mcux * mcuy * bpm, 64] in MCU-interleaved decode order (per MCU each component's v x h blocks, components in frame
    order), zig-zag, absolute DC, before dequantisation.  hv: [(h, v)] per component, one or three of them (one component: a
    non-interleaved scan of one block per MCU, and (h, v) only goes into the frame header).  qts: one table of 64 zig-zag entries
    per component, component c on slot c.  tables: {(class, slot): (bits, vals)}; luminance codes with slot 0, chroma with slot 1
    where the dictionary has one.  width, height: the frame's; default the whole MCU grid, smaller values clip the last MCUs
    (they must still need all mcux x mcuy of them).  restart=n: DRI n and an RSTn marker every n MCUs."""
    blocks = np.asarray(blocks, np.int64)
    hv = [tuple(x) for x in hv]
    assert len(hv) in (1, 3) and len(qts) == len(hv)
    mcu_hv = [(1, 1)] if len(hv) == 1 else hv
    hmax, vmax = max(h for h, _ in mcu_hv), max(v for _, v in mcu_hv)
    per_mcu = [h * v for h, v in mcu_hv]
    bpm = sum(per_mcu)
    assert blocks.shape == (mcux * mcuy * bpm, 64), (blocks.shape, mcux, mcuy, bpm)
    width = mcux * 8 * hmax if width is None else width
    height = mcuy * 8 * vmax if height is None else height
    assert -(-width // (8 * hmax)) == mcux and -(-height // (8 * vmax)) == mcuy, (width, height, mcux, mcuy)
    slot = [0 if c == 0 or (0, 1) not in tables else 1 for c in range(len(hv))]
    dc = {c: huff_codes(*tables[(0, slot[c])]) for c in range(len(hv))}
    ac = {c: huff_codes(*tables[(1, slot[c])]) for c in range(len(hv))}
    owner = [c for c, k in enumerate(per_mcu) for _ in range(k)] * (mcux * mcuy)
    ent = encode_scan_np(blocks, owner, dc, ac, restart_blocks=(restart or 0) * bpm)
    comps = [(c + 1, h, v, c, slot[c], slot[c]) for c, (h, v) in enumerate(hv)]
    dhts = {(cls, s): tables[(cls, s)] for s in sorted(set(slot)) for cls in (0, 1)}
    return write_jpeg(width, height, comps, {c: [int(v) for v in q] for c, q in enumerate(qts)}, dhts, ent, qt16=qt16,
                      restart_interval=restart or 0)


# ---- syntactically valid, semantically corrupt streams ---------------------------------------------------
def full_ac_table():
    """An AC table that holds all 256 run/size symbols -- including the degenerate `0x?0` ones (r zeros then a 0,
    src/jpeg/huffman.rs:176-189) that the Annex-K tables lack: 128 codes of 8 bits, 128 of 9 bits (no 1-bit code).
    Symbol order: a fixed permutation, so that frequent and rare symbols mix over both lengths."""
    rng = np.random.default_rng(256)
    vals = [int(v) for v in rng.permutation(256)]
    bits = [0] * 16
    bits[7], bits[8] = 128, 128
    return bits, vals


def small_dc_table(max_size=8):
    """DC sizes 0..max_size with 4-bit codes (sums of differences stay far inside i16 on small pictures)."""
    bits = [0] * 16
    bits[3] = max_size + 1
    return bits, list(range(max_size + 1))


def random_symbol_stream(rng, nsymbols, dc_tab, ac_tab, p_dc=0.12, max_size=15):
    """Random *valid codes* with random value bits, written with no regard to block structure: DC-table codes are only
    valid where the decoder expects them, so the stream is produced by simulating the decoder's table choice --
    src/jpeg/huffman.rs:146-195 semantics: first symbol of a block from the DC table, then AC symbols until 64 coefficients
    are produced (EOB fills up; ZRL and runs are clamped, Q9).  Returns the stuffed bytes and the number of whole blocks."""
    dcc, acc = huff_codes(*dc_tab), huff_codes(*ac_tab)
    dc_syms, ac_syms = [s for s in dcc if s <= max_size], [s for s in acc if (s & 15) <= max_size]    # (small values: the
    w, blocks, z = BitWriter(), 0, 0                               # samples stay in range and the RGB comparison means something)
    for _ in range(nsymbols):
        if z == 0:
            s = dc_syms[int(rng.integers(len(dc_syms)))]
            w.put(*dcc[s])
            w.put(int(rng.integers(1 << s)) if s else 0, s)
            z = 1
            continue
        if rng.random() < p_dc:
            sym = 0x00                                   # EOB now and then, so that blocks also end regularly
        else:
            sym = ac_syms[int(rng.integers(len(ac_syms)))]
        w.put(*acc[sym])
        r, s = sym >> 4, sym & 15
        if sym == 0x00:
            z = 64
        elif sym == 0xf0:
            z = min(z + 16, 64)
        else:
            w.put(int(rng.integers(1 << s)) if s else 0, s)
            z = min(z + r, 63) + 1
        if z >= 64:
            z = 0
            blocks += 1
    return w.flush(), blocks


# ---- fast entropy coding, non-interleaved twins without Pillow (tests/golden/make_multiscan.py is the checked version) ---
def encode_scan(blocks, comp_of_block, dc_codes, ac_codes, restart_blocks=0):
    """encode_blocks touching only the non-zero coefficients (a 4K picture has 200 000 blocks).  restart_blocks > 0: after every
    restart_blocks blocks (one restart interval) but the last, pad with 1-bits to a byte, write RST0..RST7 in turn and reset the
    DC predictors (T.81 F.1.2.3, E.1.4)."""
    w, pred, rst = BitWriter(), {}, 0
    nzr, nzc = np.nonzero(blocks[:, 1:])
    starts = np.searchsorted(nzr, np.arange(blocks.shape[0] + 1))
    for k in range(blocks.shape[0]):
        if restart_blocks and k and k % restart_blocks == 0:
            w.flush()
            w.out += bytes([0xff, 0xd0 + rst % 8])
            rst += 1
            pred = {}
        c = comp_of_block[k]
        blk = blocks[k]
        s, bits = magnitude(int(blk[0]) - pred.get(c, 0))
        pred[c] = int(blk[0])
        w.put(*dc_codes[c][s])
        w.put(bits, s)
        prev = 0
        for i in nzc[starts[k]:starts[k + 1]] + 1:
            run = int(i) - prev - 1
            while run > 15:
                w.put(*ac_codes[c][0xf0])
                run -= 16
            s, bits = magnitude(int(blk[i]))
            w.put(*ac_codes[c][(run << 4) | s])
            w.put(bits, s)
            prev = int(i)
        if prev < 63:
            w.put(*ac_codes[c][0x00])
    return w.flush()


def noninterleaved_twin(data, ref):
    """One scan per component, blocks in raster order over the component's own block grid (T.81 A.2.2), from the quantised
    coefficients `ref` (oracle decode of `data`, STANDARD layout).  Same coefficients, same picture."""
    return script_twin(data, ref, "Y;Cb;Cr")


# ---- every multi-scan script of a three-component baseline frame (tests/test_multiscan_scripts.py) ---------------------------
# Scans in file order, ';' between scans, the components of a scan in frame order: each component alone in any order, or a
# pair interleaved and the third alone, either first.
SCRIPTS = ["Y;Cb;Cr", "Y;Cr;Cb", "Cb;Y;Cr", "Cb;Cr;Y", "Cr;Y;Cb", "Cr;Cb;Y",
           "Y Cb;Cr", "Cr;Y Cb", "Y Cr;Cb", "Cb;Y Cr", "Cb Cr;Y", "Y;Cb Cr"]
_COMP = {"Y": 0, "Cb": 1, "Cr": 2}


def parse_script(script):
    """'Cr;Y Cb' -> [[2], [0, 1]]: frame indices per scan"""
    return [sorted(_COMP[c] for c in scan.split()) for scan in script.split(";")]


def optimal_table(counts):
    """T.81 K.2 (Figures K.1 to K.3, the procedure of libjpeg's jpeg_gen_optimal_table): (bits[16], vals) of a Huffman table
    for the symbol counts {symbol: n}; codes of at most 16 bits, none of them all ones."""
    freq = [0] * 257
    for sym, n in counts.items():
        freq[sym] = n
    freq[256] = 1                                   # the reserved code point
    size, others = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if freq[i]]
        if len(live) < 2:
            break
        c1 = max(live, key=lambda i: (-freq[i], i))                 # the least frequent; on a tie the larger symbol
        c2 = max((i for i in live if i != c1), key=lambda i: (-freq[i], i))
        freq[c1] += freq[c2]
        freq[c2] = 0
        for c in (c1, c2):
            size[c] += 1
            while others[c] >= 0:
                c = others[c]
                size[c] += 1
        c = c1
        while others[c] >= 0:
            c = others[c]
        others[c] = c2
    bits = [0] * 33
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    for i in range(32, 16, -1):                     # Figure K.3: no code longer than 16 bits
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                    # drop the reserved code point
    vals = [s for ln in range(1, 33) for s in range(256) if size[s] == ln]
    return bits[1:17], vals


class _Tally(dict):
    """Stands in for a code table of encode_scan: counts the symbols it is asked for and codes nothing."""

    def __init__(self):
        super().__init__()
        self.n = {}

    def __getitem__(self, sym):
        self.n[sym] = self.n.get(sym, 0) + 1
        return (0, 0)


def _segment(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", 2 + len(payload)) + bytes(payload)


def _ones_dqt(slot):
    return bytes([slot]) + b"\x01" * 64


def script_twins(data, ref, scripts, tables="source", dqt=None, restart=None, markers=False):
    """The quantised coefficients `ref` (oracle decode of the interleaved baseline file `data`, STANDARD layout) re-encoded as
    multi-scan files, one per script of `scripts` (see SCRIPTS).  A single-component scan is non-interleaved: raster order over
    the component's own block grid (T.81 A.2.2).  A pair is interleaved on the frame's MCU grid with each component's h x v
    blocks per MCU (A.2.3), as in `data`.  A scan that several scripts share is encoded once.

    tables: "source" (the source's DHT segments in front of the frame; every scan selects the source's slots) or "per_scan"
    (no DHT up front; right before each SOS a DHT built from that scan's symbol counts (K.2), slot q for its q-th component),
    or {frame index of a component: ((bits, vals) DC, (bits, vals) AC)}: as "per_scan" with these tables (huffman_shapes).
    dqt: where quantisation tables are defined.  None: as in the source.  "after": behind each scan, every slot whose components
    have all been scanned is redefined as a table of ones.  "split": Cr takes Cb's slot number in the frame header, and that slot
    is defined right before each scan that carries Cb or Cr, with that component's own table (the source needs three slots,
    layout_jpeg tables="three"; the script must keep Cb and Cr apart).  "tail": a table of ones on every slot behind the last
    scan.  "late": the slot of the first scan's first component is left out in front and defined behind that scan (a file
    T.81 decoders refuse: a component's table is latched when its scan starts).
    restart: None, one interval for every scan, or one per scan of the script (0: none for that scan): a DRI segment in front of
    each scan whose interval differs from the one in force, and RSTn markers in its data.
    markers: a COM and an APP1 segment in front of every scan but the first, and a COM behind the last."""
    segs, i = [], 2
    while True:
        m = data[i + 1]
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        p = bytes(data[i + 4:i + 2 + ln])
        if m == 0xda:
            break
        segs.append((m, p))
        i += 2 + ln
    sel = [(p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
    sof = [q for mk, q in segs if mk == 0xc0][0]
    H, W = struct.unpack(">HH", sof[1:5])
    comps = [(sof[6 + 3 * c], sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15, sof[8 + 3 * c]) for c in range(sof[5])]
    assert len(comps) == 3 and [p[1 + 2 * c] for c in range(p[0])] == [c[0] for c in comps]
    qts = {}
    for mk, q in segs:
        j = 0
        while mk == 0xdb and j < len(q):
            nb = 129 if q[j] >> 4 else 65
            qts[q[j] & 15] = q[j:j + nb]
            j += nb
    dht = {key: huff_codes(*t) for key, t in tables_from_jpeg(data).items()}
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux = (W + 8 * hmax - 1) // (8 * hmax)
    slots = sorted({c[3] for c in comps})
    cb_slot = comps[1][3]
    if dqt == "split":
        assert len(slots) == 3, "dqt='split' needs three quantisation slots"
    encoded = {}

    def scan(cs, r):
        """-> (DHT payload in front of the scan or b'', SOS payload, entropy-coded segment)"""
        if (tuple(cs), r) in encoded:
            return encoded[(tuple(cs), r)]
        if len(cs) == 1:
            _, h, v, _ = comps[cs[0]]
            bw = ((W * h + hmax - 1) // hmax + 7) // 8
            bh = ((H * v + vmax - 1) // vmax + 7) // 8
            mc = ref.coefs[cs[0]].reshape(ref.mcus, v, h, 64)
            yy, xx = np.mgrid[0:bh, 0:bw]
            blocks = mc[(yy // v) * mcux + (xx // h), yy % v, xx % h].reshape(-1, 64)
            owner, unit = [0] * len(blocks), 1
        else:
            ks = [comps[c][1] * comps[c][2] for c in cs]
            blocks = np.concatenate([ref.coefs[c].reshape(ref.mcus, k, 64) for c, k in zip(cs, ks)], axis=1).reshape(-1, 64)
            owner, unit = [q for q, k in enumerate(ks) for _ in range(k)] * ref.mcus, sum(ks)
        if tables == "per_scan" or isinstance(tables, dict):
            if isinstance(tables, dict):
                tabs = [tables[c] for c in cs]
            else:
                tally = [(_Tally(), _Tally()) for _ in cs]
                encode_scan(blocks, owner, {q: t[0] for q, t in enumerate(tally)}, {q: t[1] for q, t in enumerate(tally)}, r * unit)
                tabs = [(optimal_table(t[0].n), optimal_table(t[1].n)) for t in tally]
            head = b"".join(bytes([(cls << 4) | q]) + bytes(t[cls][0]) + bytes(t[cls][1]) for q, t in enumerate(tabs) for cls in (0, 1))
            selq = [(q, q) for q in range(len(cs))]
            dcc = {q: huff_codes(*t[0]) for q, t in enumerate(tabs)}
            acc = {q: huff_codes(*t[1]) for q, t in enumerate(tabs)}
        else:
            head, selq = b"", [sel[c] for c in cs]
            dcc = {q: dht[(0, sel[c][0])] for q, c in enumerate(cs)}
            acc = {q: dht[(1, sel[c][1])] for q, c in enumerate(cs)}
        ent = encode_scan(blocks, owner, dcc, acc, restart_blocks=r * unit)
        sos = bytes([len(cs)]) + b"".join(bytes([comps[c][0], (td << 4) | ta]) for c, (td, ta) in zip(cs, selq)) + bytes([0, 63, 0])
        encoded[(tuple(cs), r)] = (head, sos, ent)
        return encoded[(tuple(cs), r)]

    out = []
    for script in scripts:
        plan = parse_script(script)
        rs = [0] * len(plan) if restart is None else [restart] * len(plan) if isinstance(restart, int) else list(restart)
        assert len(rs) == len(plan) and sorted(sum(plan, [])) == [0, 1, 2], script
        late = comps[plan[0][0]][3]
        f = bytearray(b"\xff\xd8")
        for mk, q in segs:
            if mk == 0xdd or (mk == 0xc4 and tables != "source") or (mk == 0xdb and dqt in ("split", "late")):
                continue
            if mk == 0xc0 and dqt in ("split", "late"):
                for s in slots:
                    if s not in ((cb_slot, comps[2][3]) if dqt == "split" else (late,)):
                        f += _segment(0xdb, qts[s])
                if dqt == "split":
                    q = q[:14] + bytes([cb_slot]) + q[15:]          # Cr's Tq
            f += _segment(mk, q)
        done, redone, in_force = set(), set(), 0
        for k, cs in enumerate(plan):
            if k and markers:
                f += _segment(0xfe, b"scan %d of %s" % (k, script.encode())) + _segment(0xe1, b"between scans")
            if dqt == "after":
                for s in slots:
                    if s not in redone and all(c in done for c in range(3) if comps[c][3] == s):
                        f += _segment(0xdb, _ones_dqt(s))
                        redone.add(s)
            if dqt == "split":
                chroma = [c for c in cs if c in (1, 2)]
                assert len(chroma) <= 1, "dqt='split' needs Cb and Cr in different scans"
                if chroma:
                    own = qts[comps[chroma[0]][3]]
                    f += _segment(0xdb, bytes([(own[0] & 0xf0) | cb_slot]) + own[1:])
            if dqt == "late" and k == 1:
                f += _segment(0xdb, qts[late])
            if rs[k] != in_force:
                f += _segment(0xdd, struct.pack(">H", rs[k]))
                in_force = rs[k]
            head, sos, ent = scan(cs, rs[k])
            if head:
                f += _segment(0xc4, head)
            f += _segment(0xda, sos) + ent
            done.update(cs)
        if dqt == "tail":
            for s in slots:
                f += _segment(0xdb, _ones_dqt(s))
        if markers:
            f += _segment(0xfe, b"behind the last scan")
        out.append(bytes(f + b"\xff\xd9"))
    return out


def script_twin(data, ref, script, **kw):
    """script_twins for one script"""
    return script_twins(data, ref, [script], **kw)[0]


# ---- any sampling layout: h, v in {1, 2} per component (tests/test_sampling_layouts.py) --------------------------------
ANNEX_K_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                101, 72, 92, 95, 98, 112, 100, 103, 99]            # T.81 Table K.1, natural order
ANNEX_K_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                  99, 99, 99, 99] + [99] * 32                       # T.81 Table K.2


def quality_table(base, quality):
    """A K.1/K.2 table scaled to `quality` (the usual 5000/q, 200-2q rule), zig-zag (file) order, entries 1..255."""
    q = max(1, min(100, int(quality)))
    s = 5000 // q if q < 50 else 200 - 2 * q
    nat = [max(1, min(255, (b * s + 50) // 100)) for b in base]
    return [nat[z] for z in ZIGZAG]


def _dct_matrix():
    m = np.empty((8, 8))
    for u in range(8):
        for x in range(8):
            m[u, x] = (np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return m


def fdct_quantise(plane, qt_zz):
    """float64 forward DCT of a plane (level-shifted samples; both sides multiples of 8) -> quantised blocks int [n, 64] in
    raster order over the plane's block grid, zig-zag order (AC clamped to the Annex-K tables' size 10)."""
    h, w = plane.shape
    m = _dct_matrix()
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    f = np.einsum("ux,bxy,vy->buv", m, b, m).reshape(-1, 64)[:, ZIGZAG]
    q = np.rint(f / np.asarray(qt_zz, np.float64)[None, :]).astype(np.int32)
    q[:, 1:] = np.clip(q[:, 1:], -1023, 1023)
    return q


def _annex_k_tables():
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil", "std_420_q100.jpg")     # Pillow writes Annex K
    with open(p, "rb") as f:
        return tables_from_jpeg(f.read())


def layout_jpeg(width, height, hv, quality=75, seed=0, tables="split", restart=None, gray_hv=None, noise=4.0):
    """A baseline file of any sampling layout, written from float64 DCT coefficients (not by the project's own generator).

    hv: [(h, v)] * 3 (Y, Cb, Cr), h, v in {1, 2}; or None with gray_hv = (h, v): one component whose SOF carries those factors
    (its scan is non-interleaved: one block per MCU over ceil(W/8) x ceil(H/8) blocks whatever they are).  Content: smooth
    plane waves plus gaussian noise per component at its own resolution over the whole MCU grid.  tables: "split" (Y on
    slot 0, Cb and Cr on slot 1), "shared" (all on slot 0) or "three" (Cr on slot 2, its DQT coarser than Cb's).
    restart=n: DRI n and an RSTn marker every n MCUs.
    -> (bytes, [quantised blocks per component: int [n, 64], zig-zag, absolute DC, in decode order -- the oracle's T0])"""
    rng = np.random.default_rng(seed)
    if hv is None:
        comps_hv, mcu_hv = [tuple(gray_hv)], [(1, 1)]
    else:
        comps_hv = mcu_hv = [tuple(x) for x in hv]
    hmax, vmax = max(h for h, _ in mcu_hv), max(v for _, v in mcu_hv)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    slot = {"split": [0, 1, 1], "shared": [0, 0, 0], "three": [0, 1, 2]}[tables]
    qts = {0: quality_table(ANNEX_K_LUMA, quality)}
    if len(comps_hv) == 3 and tables != "shared":
        qts[1] = quality_table(ANNEX_K_CHROMA, quality)
        if tables == "three":
            qts[2] = quality_table(ANNEX_K_CHROMA, max(1, quality // 2))
    ak = _annex_k_tables()
    dhts = {}
    for s in sorted(set(slot[:len(comps_hv)])):
        src = 0 if s == 0 else 1
        dhts[(0, s)], dhts[(1, s)] = ak[(0, src)], ak[(1, src)]
    per_comp, comp_rows = [], []
    for c, (h, v) in enumerate(mcu_hv):
        ph, pw = mcuy * v * 8, mcux * h * 8
        yy, xx = np.mgrid[0:ph, 0:pw].astype(np.float64)
        amp, base = (60.0, 0.0) if c == 0 else (35.0, 0.0)
        p = np.full((ph, pw), base)
        for _ in range(3):
            fx, fy, ph0 = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0, 2 * np.pi)
            p += amp / 3 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph0)
        p += rng.normal(0.0, noise, p.shape)
        p = np.clip(p, -128.0, 127.0)
        blocks = fdct_quantise(p, qts[slot[c]])
        # raster over the component's grid -> decode order (MCU-major, v x h inside the MCU)
        g = blocks.reshape(mcuy, v, mcux, h, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
        per_comp.append(g)
        comp_rows.append(h * v)
    bpm = sum(comp_rows)
    order = np.concatenate([pc.reshape(mcux * mcuy, k, 64) for pc, k in zip(per_comp, comp_rows)], axis=1).reshape(-1, 64)
    comp_of_block = [c for c, k in enumerate(comp_rows) for _ in range(k)] * (mcux * mcuy)
    dc = {c: huff_codes(*dhts[(0, slot[c])]) for c in range(len(comps_hv))}
    ac = {c: huff_codes(*dhts[(1, slot[c])]) for c in range(len(comps_hv))}
    ent = encode_scan_np(order, comp_of_block, dc, ac, restart_blocks=(restart or 0) * bpm)
    comps = [(c + 1, h, v, slot[c], slot[c], slot[c]) for c, (h, v) in enumerate(comps_hv)]
    return write_jpeg(width, height, comps, qts, dhts, ent, restart_interval=restart or 0), per_comp


# ---- Huffman tables of every shape, and files re-coded with them (tests/test_huffman_tables.py) --------------------------------
DC_SYMBOLS = list(range(12))                                                      # baseline difference sizes (T.81 Table F.1)
AC_SYMBOLS = [0x00, 0xf0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]   # the 162 symbols of Table F.2 ("the sane ones")
N_RANDOM_SHAPES = 24


def kraft(lengths):
    """sum of 2^(16 - l): a prefix code exists iff <= 65536; the all-ones code of the longest length stays free iff < 65536"""
    return sum(1 << (16 - l) for l in lengths)


def table_of_lengths(ranked, lengths):
    """(bits, vals): the k-th symbol of `ranked` gets the k-th shortest of `lengths` (canonical codes, T.81 C.2)"""
    lengths = sorted(lengths)
    assert len(ranked) == len(lengths) and 1 <= lengths[0] and lengths[-1] <= 16 and kraft(lengths) < 65536, lengths
    bits = [0] * 16
    for l in lengths:
        bits[l - 1] += 1
    return bits, [int(s) for s in ranked]


def _random_lengths(rng, n, style, slack):
    """n code lengths from a tree grown by splitting leaves: n + 1 leaves of depth <= 16, one of them the reserved code point
    (left out: the code is complete but for it).  style: which leaf is split -- "deep" the deepest, "wide" the shallowest, "any" a
    random one.  slack > 0: afterwards that many codes are made longer, which leaves code points no code reaches."""
    leaves = [1, 1]
    while len(leaves) < n + 1:
        open_ = [k for k, d in enumerate(leaves) if d < 16]
        if style == "deep" and rng.random() < 0.8:
            k = max(open_, key=lambda j: leaves[j])
        elif style == "wide" and rng.random() < 0.8:
            k = min(open_, key=lambda j: leaves[j])
        else:
            k = open_[int(rng.integers(len(open_)))]
        leaves[k] += 1
        leaves.append(leaves[k])
    leaves.remove(max(leaves))                                      # the reserved code point: one of the longest
    for _ in range(slack):
        k = int(rng.integers(n))
        leaves[k] = int(rng.integers(leaves[k], 17))
    return leaves


def huffman_shapes(symbols, freq=None, seed=0):
    """{name: (bits, vals)}: Huffman tables of every shape over `symbols` (at most 255 of them; DC size categories or AC run/size
    symbols).  freq: {symbol: count}, what "frequent" means (ties and missing symbols: symbol order).  Every table is a prefix
    code of at most 16 bits (T.81 C.2) in which the all-ones code is free, as Annex K.2 leaves it; deterministic in its
    arguments.
      ladder        lengths 1..7, every other symbol 16 bits; frequent symbols short
      anti          the same lengths, frequent symbols on the 16-bit codes
      flat          one length, the shortest that holds all symbols
      edge9 edge10 edge9_10   every code 9 bits / 10 bits / half and half: at and just past a 9-bit primary table
      sub1 .. sub7  a few short codes, then codes of 10 and of 9 + k bits: the longest code under some 9-bit prefix is 9 + k bits
                    and shorter ones share its second-level table
      all256        AC: all 256 run/size symbols, DC: 16 symbols, lengths 2 .. 16 (`symbols` first, by frequency)
      k2            T.81 K.2 (optimal_table) on freq, or on equal counts
      random0 .. random23   lengths of trees grown by random splits (_random_lengths): a third of them complete but for the reserved
                    code point, the others with many code points unused; symbols ranked by frequency, against it or at random"""
    symbols = [int(s) for s in symbols]
    n = len(symbols)
    assert 2 <= n <= 255 and len(set(symbols)) == n
    f = dict(freq or {})
    ranked = sorted(symbols, key=lambda s: (-f.get(s, 0), s))
    out = {}
    lad = list(range(1, 8))[:n - 1] + [16] * max(0, n - 7)
    lad = lad if len(lad) == n else list(range(1, n + 1))
    out["ladder"] = table_of_lengths(ranked, lad)
    out["anti"] = table_of_lengths(ranked[::-1], lad)
    out["flat"] = table_of_lengths(ranked, [n.bit_length()] * n)
    out["edge9"] = table_of_lengths(ranked, [9] * n)
    out["edge10"] = table_of_lengths(ranked, [10] * n)
    out["edge9_10"] = table_of_lengths(ranked, [9] * (n // 2) + [10] * (n - n // 2))
    nhead = min(9, n // 2)
    for k in range(1, 8):
        head = ([2, 3, 4, 5, 6, 7, 8, 9, 9])[:nhead]
        rest = n - nhead
        n10 = rest // 3 if k > 1 else 0
        out["sub%d" % k] = table_of_lengths(ranked, head + [10] * n10 + [9 + k] * (rest - n10))
    is_dc = max(symbols) <= 15 and n <= 16
    every = ranked + [s for s in range(16 if is_dc else 256) if s not in symbols]
    prof = [2, 3, 4, 5, 6, 7, 8] + [9] * 20 + [10] * 30 + [12] * 60 + [14] * 60 + [16] * 79
    if is_dc:
        prof = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16]
    out["all256"] = table_of_lengths(every, prof)
    counts = {s: f.get(s, 0) for s in symbols if f.get(s, 0) > 0}
    out["k2"] = optimal_table(counts if len(counts) >= 2 else {s: 1 for s in symbols})
    if set(out["k2"][1]) != set(symbols):                           # (a symbol the picture does not use gets a count of one)
        out["k2"] = optimal_table({s: f.get(s, 0) + 1 for s in symbols})
    for r in range(N_RANDOM_SHAPES):
        rng = np.random.default_rng([int(seed), r, n])
        style = ("deep", "wide", "any")[r % 3]
        slack = 0 if r % 3 == r // 3 % 3 else int(rng.integers(1, n))
        lengths = _random_lengths(rng, n, style, slack)
        order = (ranked, ranked[::-1], [ranked[int(k)] for k in rng.permutation(n)])[(r // 3) % 3]
        out["random%d" % r] = table_of_lengths(order, lengths)
    return out


SHAPES = (["ladder", "anti", "flat", "edge9", "edge10", "edge9_10"] + ["sub%d" % k for k in range(1, 8)] + ["all256", "k2"]
          + ["random%d" % r for r in range(N_RANDOM_SHAPES)])


def has_1bit_code(table):
    return table[0][0] != 0


def head_segments(data):
    """-> ([(marker, payload)] in front of the first SOS, that SOS's payload)"""
    segs, i = [], 2
    while True:
        m = data[i + 1]
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        p = bytes(data[i + 4:i + 2 + ln])
        if m == 0xda:
            return segs, p
        segs.append((m, p))
        i += 2 + ln


def scan_blocks(ref):
    """the blocks of an interleaved scan in coding order, and the component each belongs to, from an oracle decode (STANDARD layout;
    a greyscale frame: one block per MCU)"""
    ks = [len(c) // ref.mcus for c in ref.coefs]
    blocks = np.concatenate([c.reshape(ref.mcus, k, 64) for c, k in zip(ref.coefs, ks)], axis=1).reshape(-1, 64)
    return blocks, [q for q, k in enumerate(ks) for _ in range(k)] * ref.mcus, sum(ks)


def symbol_counts(ref, restart=None):
    """[({DC symbol: n}, {AC symbol: n})] per component: what coding the picture's interleaved scan asks of each table"""
    blocks, owner, bpm = scan_blocks(ref)
    tally = [(_Tally(), _Tally()) for _ in ref.coefs]
    encode_scan_np(blocks, owner, {q: t[0] for q, t in enumerate(tally)}, {q: t[1] for q, t in enumerate(tally)}, (restart or 0) * bpm)
    return [(t[0].n, t[1].n) for t in tally]


def recode_huffman(data, ref, tables, slots=(0, 1, 3), restart=None):
    """The interleaved baseline file `data` (any layout layout_jpeg writes, or greyscale) with its entropy-coded segment coded
    again: component c with the table pair tables[c] = ((bits, vals) DC, (bits, vals) AC) on slot slots[c] of both classes.
    ref: the oracle's decode of `data` (STANDARD layout).  restart=n: DRI n and an RSTn marker every n MCUs (the source's own
    restart interval is dropped).  Everything else -- frame, quantisation tables, other segments -- is the source's."""
    segs, sos = head_segments(data)
    ncomp = sos[0]
    assert ncomp == len(ref.coefs) and len(tables) >= ncomp and len(slots) >= ncomp
    blocks, owner, bpm = scan_blocks(ref)
    dcc = {c: huff_codes(*tables[c][0]) for c in range(ncomp)}
    acc = {c: huff_codes(*tables[c][1]) for c in range(ncomp)}
    ent = encode_scan_np(blocks, owner, dcc, acc, restart_blocks=(restart or 0) * bpm)
    f = bytearray(b"\xff\xd8")
    for mk, q in segs:
        if mk not in (0xc4, 0xdd):
            f += _segment(mk, q)
    written = {}
    for c in range(ncomp):
        for cls in (0, 1):
            t = (list(tables[c][cls][0]), list(tables[c][cls][1]))
            assert written.setdefault((cls, slots[c]), t) == t, "two tables on one slot"
    for (cls, s), (bits, vals) in sorted(written.items()):
        f += _segment(0xc4, bytes([(cls << 4) | s]) + bytes(bits) + bytes(vals))
    if restart:
        f += _segment(0xdd, struct.pack(">H", restart))
    f += _segment(0xda, bytes([ncomp]) + b"".join(bytes([sos[1 + 2 * c], (slots[c] << 4) | slots[c]]) for c in range(ncomp))
                  + bytes([0, 63, 0]))
    return bytes(f + ent + b"\xff\xd9")


def _code_arrays(codes):
    """{symbol: (code, length)} -> (code[256], length[256]); length 0: the table has no such symbol"""
    code, ln = np.zeros(256, np.int64), np.zeros(256, np.int64)
    if isinstance(codes, _Tally):
        return code, ln + 1                                     # (counting, not coding: see encode_scan_np)
    for s, (c, l) in codes.items():
        code[s], ln[s] = c, l
    return code, ln


def encode_scan_np(blocks, comp_of_block, dc_codes, ac_codes, restart_blocks=0):
    """encode_scan in numpy (a 1080p picture in a second instead of a minute); the same bytes, which tests/test_huffman_tables.py
    checks.  Every symbol becomes one token (code and value bits, at most 27 bits); the tokens are sorted into coding order and
    added into 32-bit words; stuffing and the RSTn markers go in at byte level."""
    blocks = np.asarray(blocks, np.int64)
    n = blocks.shape[0]
    owner = np.asarray(comp_of_block, np.int64)
    ncomp = int(owner.max()) + 1
    dcc = [_code_arrays(dc_codes[c]) for c in range(ncomp)]
    acc = [_code_arrays(ac_codes[c]) for c in range(ncomp)]
    interval = np.arange(n) // restart_blocks if restart_blocks else np.zeros(n, np.int64)

    def sized(v):                                              # magnitude() on an array
        a = np.abs(v)
        s = np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)
        return s, np.where(v >= 0, v, v + (1 << s) - 1)
    keys, vals, lens = [], [], []
    diff = np.zeros(n, np.int64)
    for c in range(ncomp):
        idx = np.nonzero(owner == c)[0]
        dc = blocks[idx, 0]
        prev = np.concatenate([[0], dc[:-1]])
        prev[np.concatenate([[True], interval[idx][1:] != interval[idx][:-1]])] = 0
        diff[idx] = dc - prev
    s, b = sized(diff)
    code = np.array([dcc[c][0] for c in range(ncomp)])[owner, s]
    ln = np.array([dcc[c][1] for c in range(ncomp)])[owner, s]
    assert np.all(ln > 0), "a DC size the table lacks"
    keys.append(np.arange(n) * 260 + 3)
    vals.append((code << s) | b)
    lens.append(ln + s)
    acode, alen = np.array([a[0] for a in acc]), np.array([a[1] for a in acc])
    nzr, nzc = np.nonzero(blocks[:, 1:])
    nzc = nzc + 1
    first = np.concatenate([[True], nzr[1:] != nzr[:-1]]) if len(nzr) else np.zeros(0, bool)
    run = nzc - np.where(first, 0, np.concatenate([[0], nzc[:-1]])) - 1
    o = owner[nzr]
    for j in range(3):                                         # up to three ZRL in front of a coefficient
        m = run >= 16 * (j + 1)
        assert np.all(alen[o[m], 0xf0] > 0), "the AC table lacks ZRL"
        keys.append(nzr[m] * 260 + nzc[m] * 4 + j)
        vals.append(acode[o[m], 0xf0])
        lens.append(alen[o[m], 0xf0])
    s, b = sized(blocks[nzr, nzc])
    sym = ((run & 15) << 4) | s
    assert np.all(s <= 15) and np.all(alen[o, sym] > 0), "an AC symbol the table lacks"
    keys.append(nzr * 260 + nzc * 4 + 3)
    vals.append((acode[o, sym] << s) | b)
    lens.append(alen[o, sym] + s)
    last = np.zeros(n, np.int64)
    last[nzr] = nzc                                            # (ascending inside a block: the last one stays)
    m = last < 63
    assert np.all(alen[owner[m], 0] > 0), "the AC table lacks EOB"
    keys.append(np.nonzero(m)[0] * 260 + 257)
    vals.append(acode[owner[m], 0])
    lens.append(alen[owner[m], 0])
    if isinstance(dc_codes[0], _Tally):                         # the symbols are counted, nothing is coded
        for c in range(ncomp):
            dsz = sized(diff[owner == c])[0]
            zrl = sum(int(np.count_nonzero((run >= 16 * (j + 1)) & (o == c))) for j in range(3))
            asym = np.bincount(sym[o == c], minlength=256)
            asym[0xf0] += zrl
            asym[0] += int(np.count_nonzero(m & (owner == c)))
            dc_codes[c].n.update({int(k): int(v) for k, v in enumerate(np.bincount(dsz, minlength=16)) if v})
            ac_codes[c].n.update({int(k): int(v) for k, v in enumerate(asym) if v})
        return b""
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    keys, vals, lens = keys[order], vals[order], lens[order]
    # pad every restart interval (and the scan) to a byte with 1-bits: a pad token behind the interval's last token
    tint = interval[keys // 260]
    ends = np.nonzero(np.concatenate([tint[1:] != tint[:-1], [True]]))[0]
    cum = np.cumsum(lens)
    pads, shift, byte_ends = np.zeros(len(ends), np.int64), 0, []
    for j, e in enumerate(ends):                               # (a loop over the intervals only)
        pads[j] = -(int(cum[e]) + shift) % 8
        shift += int(pads[j])
        byte_ends.append((int(cum[e]) + shift) // 8)
    vals = np.insert(vals, ends + 1, (1 << pads) - 1)
    lens = np.insert(lens, ends + 1, pads)
    start = np.cumsum(lens) - lens
    total = int(start[-1] + lens[-1])
    words = np.zeros(total // 32 + 2, np.uint64)
    w, off = start >> 5, start & 31
    v64 = vals.astype(np.uint64) << (np.uint64(64) - off.astype(np.uint64) - lens.astype(np.uint64))      # lens <= 27, off <= 31
    v64[lens == 0] = 0
    np.add.at(words, w, v64 >> np.uint64(32))
    np.add.at(words, w + 1, v64 & np.uint64(0xffffffff))
    raw = np.frombuffer(words.astype(">u4").tobytes(), np.uint8)[:total // 8]
    ff = np.nonzero(raw == 0xff)[0]
    out = np.insert(raw, ff + 1, 0)
    if restart_blocks and len(byte_ends) > 1:
        cuts = np.asarray(byte_ends[:-1], np.int64)
        at = cuts + np.searchsorted(ff, cuts)                  # stuffed position of every interval's end
        marks = np.stack([np.full(len(cuts), 0xff), 0xd0 + np.arange(len(cuts)) % 8], axis=1).reshape(-1)
        out = np.insert(out, np.repeat(at, 2), marks.astype(np.uint8))
    return out.astype(np.uint8).tobytes()

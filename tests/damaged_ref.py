"""A serial decode of damaged baseline scans: what status and which coefficients a damaged picture must get (test infrastructure).

One bit reader, one loop over the blocks, no subsequences, none of the project's tables.  It states the rule of DESIGN.md s2 and
include/mjx.h once:

  Bits      The scan is the de-stuffed bytes behind the SOS header up to the end of the file, markers other than RSTn kept as they
            are (the end-of-image marker's 16 bits included).  Bytes past the end read 0xAA.
  Symbols   Canonical Huffman (T.81 C.2), the shortest code that matches.  Where no code of 1 to 16 bits matches -- or the DC symbol
            is above 15 -- the decoder consumes ONE bit, produces a symbol of run 0 and size 0 and records "invalid code in block b"
            (mjx_huff.h: lut_invalid).  The decode goes on.
  Blocks    End-of-block, ZRL and the run clamps of huffman.rs:164-189: pos = min(z + run, 63), z = pos + 1.  DC prediction per
            component, never reset, or reset at each restart interval.
  End       The decode stops after the picture's last block; with restart intervals after each interval's last block -- what
            follows in the interval is ignored.  An interval starts at the byte behind its RSTn marker and ends in front of the next
            interval's first byte; while decoding it the reader sees the bytes that follow it in the de-stuffed scan.
  Verdict   TRUNCATED if a block the picture needs has a symbol that STARTS behind the band: the last bit of the scan (of the
            block's interval), counted from the scan's (the interval's) first bit, rounded up to a multiple of 32, inclusive.  This is
            the band rule: the kernels look at the end of a scan when a lane takes a new dword, so up to 31 bits of the padding may
            be read as symbols, and so may the bits of a symbol that starts inside the band and ends behind it.  A scan that ends up to
            58 bits early can therefore come out OK (DESIGN.md s2 says why the exact rule was not taken).  Also TRUNCATED: fewer RSTn
            markers than the picture has intervals less one.
            Else BAD_HUFFMAN if an invalid code was recorded in a block the picture needs.  Else OK.  TRUNCATED wins.
`rule="exact"` is the other rule (a block must END at or before the last bit), kept for the tests that show the two differ.
"""
import functools
import struct

import numpy as np

OK, TRUNCATED, BAD_HUFFMAN = "OK", "TRUNCATED", "BAD_HUFFMAN"


class Picture:
    """Frame and scan of a baseline file with one interleaved scan: what the decode needs, read from the file's own segments."""

    def __init__(self, data):
        data = bytes(data)
        assert data[:2] == b"\xff\xd8"
        self.dht, self.restart = {}, 0
        frame, i = None, 2
        while True:
            assert data[i] == 0xff, "marker expected at %d" % i
            m = data[i + 1]
            ln = struct.unpack(">H", data[i + 2:i + 4])[0]
            p = data[i + 4:i + 2 + ln]
            i += 2 + ln
            if m == 0xc0:
                self.height, self.width = struct.unpack(">HH", p[1:5])
                frame = [(p[6 + 3 * k], p[7 + 3 * k] >> 4, p[7 + 3 * k] & 15) for k in range(p[5])]
            elif m == 0xc4:
                j = 0
                while j < len(p):
                    bits = list(p[j + 1:j + 17])
                    self.dht[(p[j] >> 4, p[j] & 15)] = (bits, list(p[j + 17:j + 17 + sum(bits)]))
                    j += 17 + sum(bits)
            elif m == 0xdd:
                self.restart = struct.unpack(">H", p[:2])[0]
            elif m == 0xda:
                sel = [(p[1 + 2 * k], p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15) for k in range(p[0])]
                break
        self.raw = data[i:]                                    # the entropy-coded bytes, stuffed, to the end of the file
        self.head = data[:i]
        hv = {cid: (h, v) for cid, h, v in frame}
        if len(sel) == 1:                                      # one component: one block per MCU, the sampling factors say nothing
            self.mcux, self.mcuy = -(-self.width // 8), -(-self.height // 8)
            self.blocks_of_mcu = [(0, sel[0][1], sel[0][2])]
        else:
            hmax, vmax = max(h for h, _ in hv.values()), max(v for _, v in hv.values())
            self.mcux, self.mcuy = -(-self.width // (8 * hmax)), -(-self.height // (8 * vmax))
            self.blocks_of_mcu = [(c, td, ta) for c, (cid, td, ta) in enumerate(sel) for _ in range(hv[cid][0] * hv[cid][1])]
        self.ncomp = len(sel)
        self.bpm = len(self.blocks_of_mcu)
        self.nblocks = self.mcux * self.mcuy * self.bpm
        self.scan, self.rst = destuff(self.raw, self.restart != 0)


def destuff(raw, restarts):
    """The entropy-coded bytes as the decode sees them: FF 00 -> FF; with restart intervals FF D0..D7 taken out and the offset of the
    byte that follows recorded; any other FF xx kept as it is; a lone FF at the very end kept.  -> (bytes, [offsets])"""
    out, rst, k, n = bytearray(), [], 0, len(raw)
    while k < n:
        b = raw[k]
        out.append(b)
        k += 1
        if b != 0xff or k >= n:
            continue
        if raw[k] == 0x00:
            k += 1
        elif restarts and (raw[k] & 0xf8) == 0xd0:
            out.pop()
            k += 1
            rst.append(len(out))
    return bytes(out), rst


def stuff(scan):
    """bytes of a de-stuffed scan -> entropy-coded bytes that de-stuff to them (every FF followed by 00)"""
    return bytes(scan).replace(b"\xff", b"\xff\x00")


def code_lookup(table):
    """(bits, vals) -> two lists over all 65536 windows of 16 bits: symbol (-1: no code matches) and code length.  T.81 C.2."""
    return _code_lookup(tuple(table[0]), tuple(table[1]))


@functools.lru_cache(maxsize=64)
def _code_lookup(bits, vals):
    w = np.arange(65536, dtype=np.int64)
    sym, ln = np.full(65536, -1, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        c = w >> (16 - l)
        hit = (sym < 0) & (c >= code) & (c < code + bits[l - 1])
        sym[hit] = np.asarray(list(vals) + [0], np.int64)[k + (c[hit] - code)]
        ln[hit] = l
        code = (code + bits[l - 1]) << 1
        k += bits[l - 1]
    return sym.tolist(), ln.tolist()


def unmatched_patterns(table):
    """The bit patterns after which no code of the table can match whatever follows, shortest first: [bit string].  (A pattern of k
    bits qualifies when all 2^(16-k) windows that begin with it are unmatched and its first k - 1 bits do not qualify.)"""
    bad = np.asarray(code_lookup(table)[0]) < 0
    out = []
    for k in range(1, 17):
        mine = bad.reshape(1 << k, -1).all(axis=1)
        parent = bad.reshape(1 << (k - 1), -1).all(axis=1)
        out += [format(j, "0%db" % k) for j in np.nonzero(mine & ~np.repeat(parent, 2))[0]]
    return out


class Result:
    """verdict; t0 int16 [nblocks, 64] (MCU-interleaved decode order, zig-zag, DC predicted; a truncated picture's stop at the block that
    is short); ends [nblocks] bit position in the scan behind each block's last symbol (-1: not reached); last_start [nblocks] where
    that symbol starts; invalid: [(block, bit position)] of the invalid codes met; complete: every block was decoded"""


PAD = 512          # bytes of 0xAA behind the scan: a block's symbols start at or before the band, and one block is 64 symbols at most


def decode(pic, scan=None, rst=None, rule="band", first_invalid_only=False, invalid_takes_window=False, resume=None):
    """The serial decode of `pic` (a Picture) over `scan` / `rst` (default: the picture's own).
    rule: "band" (the rule above), "exact" (a block must end at or before the scan's last bit), or "start" (a block counts when it
    starts inside the scan -- a planted error).  first_invalid_only, invalid_takes_window: planted errors.
    resume = (Result of this picture over another scan, lo, hi), for pictures without restart intervals, saves work and changes
    nothing (tests/test_damaged_streams.py checks that): the two scans have the same first `lo` bits, so the blocks of the other
    decode that end 32 bits or more in front of bit lo are taken over -- no symbol of theirs looks at a bit that differs (16 bits of
    code window, value bits inside the block) -- and the decode starts behind them.  hi (or None): the scans are of one length and the
    same again from bit hi on; once a block of this decode ends at or behind hi where the same block of the other decode ends, the
    two decodes are in the same state but for the DC predictors, and the rest is the other's with the DC offsets added."""
    scan = pic.scan if scan is None else bytes(scan)
    rst = pic.rst if rst is None else list(rst)
    nb, bpm = pic.nblocks, pic.bpm
    look = {key: code_lookup(t) for key, t in pic.dht.items()}
    tabs = [(c, look[(0, td)], look[(1, ta)]) for c, td, ta in pic.blocks_of_mcu]
    res = Result()
    t0 = res.t0 = np.zeros((nb, 64), np.int16)
    res.ends = np.full(nb, -1, np.int64)
    res.last_start = np.full(nb, -1, np.int64)
    res.invalid, res.complete, res.verdict = [], False, TRUNCATED
    seg_blocks = pic.restart * bpm if pic.restart else nb
    nseg = -(-nb // seg_blocks)
    if len(rst) + 1 < nseg:
        return res                                             # fewer markers than intervals: nothing is decoded
    starts = [0] + rst[:nseg - 1]
    stops = starts[1:] + [len(scan)]
    padded = scan + b"\xaa" * PAD
    for g in range(nseg):
        base, seg_bits = 8 * starts[g], 8 * (stops[g] - starts[g])
        band, last_bit = base + (seg_bits + 31) // 32 * 32, base + seg_bits
        p = base
        pred = [0] * pic.ncomp
        b0, b1 = g * seg_blocks, min((g + 1) * seg_blocks, nb)
        if resume is not None:
            old, same_bits, same_again = resume
            assert nseg == 1 and old.complete
            keep = int(np.searchsorted(old.ends, same_bits - 32, side="right"))
            t0[:keep] = old.t0[:keep]
            res.ends[:keep], res.last_start[:keep] = old.ends[:keep], old.last_start[:keep]
            res.invalid = [x for x in old.invalid if x[0] < keep]
            seen = set()
            for k in range(keep - 1, max(keep - 1 - bpm, -1), -1):
                if tabs[k % bpm][0] not in seen:
                    seen.add(tabs[k % bpm][0])
                    pred[tabs[k % bpm][0]] = int(old.t0[k, 0])
            if keep:
                b0, p = keep, int(old.ends[keep - 1])
        for b in range(b0, b1):
            c, dct, act = tabs[b % bpm]
            z, first, row = 0, p, t0[b]
            while z < 64:
                start = p
                i = p >> 3
                w = ((padded[i] << 16 | padded[i + 1] << 8 | padded[i + 2]) >> (8 - (p & 7))) & 0xffff
                sym_t, len_t = dct if z == 0 else act
                sym = sym_t[w]
                if sym < 0 or (z == 0 and sym > 15):
                    if not (first_invalid_only and res.invalid):
                        res.invalid.append((b, p))
                    p += 16 if invalid_takes_window else 1
                    run, size = 0, 0
                else:
                    p += len_t[w]
                    if z == 0:
                        run, size = 0, sym
                    elif sym == 0x00:
                        run, size = 63, 0                      # end of block
                    elif sym == 0xf0:
                        run, size = 15, 0
                    else:
                        run, size = sym >> 4, sym & 15
                val = 0
                if size:
                    i = p >> 3
                    v = ((padded[i] << 16 | padded[i + 1] << 8 | padded[i + 2]) >> (8 - (p & 7))) & 0xffff
                    v >>= 16 - size
                    val = v if v >> (size - 1) else v - (1 << size) + 1
                    p += size
                pos = min(z + run, 63)
                if z == 0:
                    pred[c] += val
                    row[0] = ((pred[c] + 32768) & 0xffff) - 32768
                elif size:
                    row[pos] = ((val + 32768) & 0xffff) - 32768
                z = pos + 1
            res.ends[b], res.last_start[b] = p, start
            if (start > band) if rule == "band" else (p > last_bit) if rule == "exact" else (first > last_bit):
                return res                                     # a block the picture needs is short: nothing behind it is looked at
            if resume is not None and same_again is not None and p >= same_again and p == old.ends[b] and b + 1 < b1:
                k = np.arange(b + 1, b1)
                t0[b + 1:] = old.t0[b + 1:]
                comp = np.asarray([tabs[j % bpm][0] for j in range(bpm)])[k % bpm]
                for cc in range(pic.ncomp):
                    own = [j for j in range(b, max(b - bpm, -1), -1) if tabs[j % bpm][0] == cc]
                    delta = pred[cc] - (int(old.t0[own[0], 0]) if own else 0)
                    t0[k[comp == cc], 0] = (old.t0[k[comp == cc], 0].astype(np.int64) + delta).astype(np.int16)
                res.ends[b + 1:], res.last_start[b + 1:] = old.ends[b + 1:], old.last_start[b + 1:]
                res.invalid += [x for x in old.invalid if x[0] > b]
                break
    res.complete = True
    res.verdict = BAD_HUFFMAN if res.invalid else OK
    return res

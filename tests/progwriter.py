"""A progressive (SOF2) JPEG writer for tests: progressive_from_blocks beside jpegwriter.jpeg_from_blocks.

The file carries exactly the coefficient blocks given, sent by the scan script given, with the procedures of T.81 G.1.2 as libjpeg's
jcphuff.c codes them (DC first / refine, AC first with EOBn runs and ZRL, AC refine with buffered correction bits).  Every scan gets
its own optimal Huffman table (jpegwriter.optimal_table), written in front of its SOS.  No restart intervals: Pillow's files cover
those.  Pillow must decode a file from here to the pixels of jpeg_from_blocks' file of the same blocks (tests/test_progressive_host.py).
"""
import struct

import numpy as np

from jpegwriter import BitWriter, huff_codes, optimal_table

# scan scripts: [(components, Ss, Se, Ah, Al)]
def script_spectral(ncomp):
    """spectral selection only: DC, then three bands per component"""
    s = [(list(range(ncomp)), 0, 0, 0, 0)]
    for c in range(ncomp):
        s += [([c], 1, 5, 0, 0), ([c], 6, 20, 0, 0), ([c], 21, 63, 0, 0)]
    return s


def script_successive(ncomp):
    """successive approximation only over the full band, with two refinements"""
    s = [(list(range(ncomp)), 0, 0, 0, 2)]
    s += [([c], 1, 63, 0, 2) for c in range(ncomp)]
    for ah in (2, 1):
        s += [(list(range(ncomp)), 0, 0, ah, ah - 1)] + [([c], 1, 63, ah, ah - 1) for c in range(ncomp)]
    return s


def script_libjpeg(ncomp):
    """libjpeg's default (jpeg_simple_progression): ten scans for three components, six for one"""
    if ncomp == 1:
        return [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 1, 0)]
    return [([0, 1, 2], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([2], 1, 63, 0, 1), ([1], 1, 63, 0, 1), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1),
            ([0, 1, 2], 0, 0, 1, 0), ([2], 1, 63, 1, 0), ([1], 1, 63, 1, 0), ([0], 1, 63, 1, 0)]


def script_dc_apart(ncomp):
    """DC non-interleaved: a DC scan per component, then the whole AC band"""
    return [([c], 0, 0, 0, 0) for c in range(ncomp)] + [([c], 1, 63, 0, 0) for c in range(ncomp)]


def script_single_coefficients():
    """64 single-coefficient scans, grey"""
    return [([0], k, k, 0, 0) for k in range(64)]


def script_al13(ncomp):
    """Al = 13: the point transform's limit, refined down to 0 for the DC; the AC band is sent once at 0"""
    s = [(list(range(ncomp)), 0, 0, 0, 13)]
    s += [(list(range(ncomp)), 0, 0, ah, ah - 1) for ah in range(13, 0, -1)]
    return s + [([c], 1, 63, 0, 0) for c in range(ncomp)]


def script_stops_early(ncomp):
    """a progression that stops early: the low bit of every coefficient and the band 33 .. 63 are never sent"""
    return [(list(range(ncomp)), 0, 0, 0, 1)] + [([c], 1, 32, 0, 1) for c in range(ncomp)]


def masked_blocks(blocks, script, comp_of_block):
    """What a decoder holds after `script`: per (component, coefficient) the bits down to the last Al sent, zero where nothing was
    sent -- the blocks whose baseline file is the twin of a progression that stops early."""
    blocks = np.asarray(blocks, np.int64)
    ncomp = max(comp_of_block) + 1
    al = np.full((ncomp, 64), -1, np.int64)
    for comps, ss, se, _, a in script:
        for c in comps:
            al[c, ss:se + 1] = a
    out = np.zeros_like(blocks)
    for k, blk in enumerate(blocks):
        a = al[comp_of_block[k]]
        sent = a >= 0
        sh = np.where(sent, a, 0)
        dc = (int(blk[0]) >> int(sh[0])) << int(sh[0])               # (the DC is shifted arithmetically, the ACs by magnitude)
        mag = (np.abs(blk) >> sh) << sh
        out[k] = np.where(sent, np.sign(blk) * mag, 0)
        out[k, 0] = dc if sent[0] else 0
    return out


class _Scan:
    """Tokens of one scan: ("s", symbol) or ("b", value, nbits); coded once the symbol counts are known."""

    def __init__(self):
        self.tok, self.eobrun, self.be = [], 0, []

    def sym(self, s):
        self.tok.append(("s", s))

    def bits(self, v, n):
        if n:
            self.tok.append(("b", int(v) & ((1 << n) - 1), n))

    def flush_eobrun(self):
        if self.eobrun:
            n = self.eobrun.bit_length() - 1
            self.sym(n << 4)
            self.bits(self.eobrun, n)
            self.eobrun = 0
            for b in self.be:
                self.bits(b, 1)
            self.be = []


def _ac_first(sc, blk, ss, se, al):
    r = 0
    for k in range(ss, se + 1):
        v = int(blk[k])
        t = abs(v) >> al
        if t == 0:
            r += 1
            continue
        sc.flush_eobrun()
        while r > 15:
            sc.sym(0xf0)
            r -= 16
        n = t.bit_length()
        sc.sym((r << 4) | n)
        sc.bits(t if v >= 0 else ~t, n)
        r = 0
    if r > 0:
        sc.eobrun += 1
        if sc.eobrun == 0x7fff:
            sc.flush_eobrun()


def _ac_refine(sc, blk, ss, se, al):
    absv = [abs(int(blk[k])) >> al for k in range(64)]
    eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
    r, br = 0, []
    for k in range(ss, se + 1):
        t = absv[k]
        if t == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            sc.flush_eobrun()
            sc.sym(0xf0)
            r -= 16
            for b in br:
                sc.bits(b, 1)
            br = []
        if t > 1:
            br.append(t & 1)
            continue
        sc.flush_eobrun()
        sc.sym((r << 4) | 1)
        sc.bits(0 if int(blk[k]) < 0 else 1, 1)
        for b in br:
            sc.bits(b, 1)
        br, r = [], 0
    if r > 0 or br:
        sc.eobrun += 1
        sc.be += br
        if sc.eobrun == 0x7fff or len(sc.be) > 1000 - 64 + 1:
            sc.flush_eobrun()


def _segment(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", 2 + len(payload)) + payload


def progressive_from_blocks(blocks, script, hv, mcux, mcuy, qts, width=None, height=None):
    """blocks: int [mcux * mcuy * bpm, 64] in MCU-interleaved decode order, zig-zag, absolute DC (as jpeg_from_blocks takes them);
    script: [(components, Ss, Se, Ah, Al)]; hv: [(h, v)] per component, one or three; qts: one table of 64 zig-zag entries per
    component (slot c).  width, height default to the whole MCU grid."""
    blocks = np.asarray(blocks, np.int64)
    hv = [tuple(x) for x in hv]
    ncomp = len(hv)
    mcu_hv = [(1, 1)] if ncomp == 1 else hv
    hmax, vmax = max(h for h, _ in mcu_hv), max(v for _, v in mcu_hv)
    bpm = sum(h * v for h, v in mcu_hv)
    assert blocks.shape == (mcux * mcuy * bpm, 64)
    width = mcux * 8 * hmax if width is None else width
    height = mcuy * 8 * vmax if height is None else height
    assert -(-width // (8 * hmax)) == mcux and -(-height // (8 * vmax)) == mcuy
    first = np.cumsum([0] + [h * v for h, v in mcu_hv])

    def block(c, bx, by):                        # block (bx, by) of component c's padded grid
        h, v = mcu_hv[c]
        m = (by // v) * mcux + bx // h
        return blocks[m * bpm + first[c] + (by % v) * h + bx % h]

    out = bytearray(b"\xff\xd8")
    for c, q in enumerate(qts):
        out += _segment(0xdb, bytes([c]) + bytes(int(x) for x in q))
    sof = struct.pack(">BHHB", 8, height, width, ncomp)
    for c, (h, v) in enumerate(hv):
        sof += bytes([c + 1, (h << 4) | v, c])
    out += _segment(0xc2, sof)
    for comps, ss, se, ah, al in script:
        scans = {c: _Scan() for c in comps}      # one token list per table: DC scans code per component, an AC scan has one
        order = []                               # (component, block) in scan order
        if len(comps) > 1:
            for m in range(mcux * mcuy):
                for c in comps:
                    h, v = mcu_hv[c]
                    for j in range(h * v):
                        order.append((c, block(c, (m % mcux) * h + j % h, (m // mcux) * v + j // h)))
        else:
            c = comps[0]
            h, v = mcu_hv[c]
            cbw = -(-(width * h) // (8 * hmax)) if ncomp > 1 else -(-width // 8)
            cbh = -(-(height * v) // (8 * vmax)) if ncomp > 1 else -(-height // 8)
            order = [(c, block(c, bx, by)) for by in range(cbh) for bx in range(cbw)]
        stream = []                              # (scan object, token index) in coding order
        pred = {c: 0 for c in comps}
        for c, blk in order:
            sc = scans[c]
            n0 = len(sc.tok)
            if ss == 0 and ah == 0:
                v = int(blk[0]) >> al
                d = v - pred[c]
                pred[c] = v
                n = abs(d).bit_length()
                sc.sym(n)
                sc.bits(d if d >= 0 else d + (1 << n) - 1, n)
            elif ss == 0:
                sc.bits((int(blk[0]) >> al) & 1, 1)
            elif ah == 0:
                _ac_first(sc, blk, ss, se, al)
            else:
                _ac_refine(sc, blk, ss, se, al)
            stream += [(c, i) for i in range(n0, len(sc.tok))]
        for c in comps:
            n0 = len(scans[c].tok)
            scans[c].flush_eobrun()
            stream += [(c, i) for i in range(n0, len(scans[c].tok))]
        # tables: slot q for the scan's q-th component (a DC refinement scan codes no symbol and writes none)
        codes = {}
        for q, c in enumerate(comps):
            counts = {}
            for t in scans[c].tok:
                if t[0] == "s":
                    counts[t[1]] = counts.get(t[1], 0) + 1
            if counts:
                bits, vals = optimal_table(counts)
                out += _segment(0xc4, bytes([((1 if ss else 0) << 4) | q]) + bytes(bits) + bytes(vals))
                codes[c] = huff_codes(bits, vals)
        sos = bytes([len(comps)])
        for q, c in enumerate(comps):
            sos += bytes([c + 1, (q << 4) | q])
        out += _segment(0xda, sos + bytes([ss, se, (ah << 4) | al]))
        w = BitWriter()
        for c, i in stream:
            t = scans[c].tok[i]
            if t[0] == "s":
                w.put(*codes[c][t[1]])
            else:
                w.put(t[1], t[2])
        out += w.flush()
    return bytes(out + b"\xff\xd9")

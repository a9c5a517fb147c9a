"""A plain serial restatement of T.81 Annex G.2 (progressive Huffman decoding) in Python: the reference the progressive tests compare
the library with.  It is not the kernels' routine: its own marker walk, its own bit reader, Huffman decoding bit by bit from the
code list, dictionaries of blocks.

decode(data) -> Result with
    status  OK, or what the library is specified to answer (include/mjx.h, MJX_OPTS_PROGRESSIVE): UNSUPPORTED_FORMAT for a script the
            rules refuse, MISSING_TABLE, TRUNCATED when a restart interval runs out of bits before its blocks are complete (it
            wins), BAD_HUFFMAN for a bit pattern no code matches, a coefficient index past Se, a refinement symbol of a size other
            than 1 or an end-of-band run that reaches past the interval's last block.  A file that ends inside a marker segment is
            TRUNCATED; a lone 0xFF as the file's last byte belongs to the scan.
    coefs   int16 [MCUs * blocks per MCU, 64] in MCU-interleaved order, zig-zag inside a block, zeros in the padding blocks
            (None unless status is OK)
    stats   {"max_eob_category": the largest r of an EOBr symbol decoded, "scans": number of scans, "symbols": Huffman symbols,
             "zrl_over_history": coefficients with a history that a refinement ZRL's run passed over, "eob_run_corrections": correction
             bits read inside end-of-band runs}
The rules for damaged streams follow the specification in the header, step by step: a pattern no code matches takes one bit and
stands for "run 0, size 0" (the next coefficient); bits behind an interval's end read as zero and the interval stops at the end of the
block in which it first used one.
"""
import numpy as np

OK, TRUNCATED, BAD_HUFFMAN, UNSUPPORTED_FORMAT, MISSING_TABLE = 0, 1, 4, 7, 11


class Result:
    def __init__(self, status, coefs=None, stats=None, geometry=None):
        self.status, self.coefs, self.stats, self.geometry = status, coefs, stats or {}, geometry


class _Refused(Exception):
    def __init__(self, code):
        self.code = code


class _Bits:
    def __init__(self, data):
        self.d, self.pos, self.n = data, 0, len(data) * 8

    def bit(self):
        p = self.pos
        self.pos += 1
        return (self.d[p >> 3] >> (7 - (p & 7))) & 1 if p < self.n else 0

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def short(self):
        return self.pos > self.n


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def _symbol(b, table, st):
    """-> symbol, or None for a pattern no code matches (one bit taken)"""
    start, code = b.pos, 0
    for ln in range(1, 17):
        code = (code << 1) | b.bit()
        if (ln, code) in table:
            st["symbols"] += 1
            return table[(ln, code)]
    b.pos = start + 1
    st["bad"] = True
    return None


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _i16(v):
    v &= 0xffff
    return v - 0x10000 if v & 0x8000 else v


def _walk(data):
    """the marker walk: frame, and per scan (components, Ss, Se, Ah, Al, tables in force, restart interval, intervals' bytes)"""
    def at(i):
        if i >= len(data):
            raise _Refused(TRUNCATED)
        return data[i]
    i, frame, dc, ac, qt, dri, scans, size = 0, None, {}, {}, {}, 0, [], None
    bits_sent = {}
    latched = {}
    while i < len(data):
        if at(i) != 0xff:
            raise _Refused(UNSUPPORTED_FORMAT)
        m = at(i + 1)
        if m in (0xd8, 0x01) or 0xd0 <= m <= 0xd7:
            i += 2
            continue
        if m == 0xd9:
            break
        ln = (at(i + 2) << 8) | at(i + 3)
        if ln < 2:
            raise _Refused(TRUNCATED)
        p, end = i + 4, i + 2 + ln
        if m == 0xdb:
            while p < end:
                prec, slot = at(p) >> 4, at(p) & 15
                n = 128 if prec else 64
                at(p + n)
                qt[slot] = [((data[p + 1 + 2 * k] << 8) | data[p + 2 + 2 * k]) if prec else data[p + 1 + k] for k in range(64)]
                p += 1 + n
        elif m == 0xc4:
            while p < end:
                cls, slot = at(p) >> 4, at(p) & 15
                at(p + 16)
                bits = list(data[p + 1:p + 17])
                at(p + 16 + sum(bits)) if sum(bits) else None
                (ac if cls else dc)[slot] = _codes(bits, list(data[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xdd:
            dri = (at(p) << 8) | at(p + 1)
        elif m == 0xc2:
            if at(p) != 8 or at(p + 5) not in (1, 3):
                raise _Refused(UNSUPPORTED_FORMAT)
            size = ((at(p + 3) << 8) | at(p + 4), (at(p + 1) << 8) | at(p + 2))
            frame = [(at(p + 6 + 3 * c), at(p + 7 + 3 * c) >> 4, at(p + 7 + 3 * c) & 15, at(p + 8 + 3 * c)) for c in range(at(p + 5))]
        elif 0xc0 <= m <= 0xcf and m not in (0xc4, 0xc8, 0xcc):
            raise _Refused(UNSUPPORTED_FORMAT)
        elif m == 0xda:
            n = at(p)
            sel = [(at(p + 1 + 2 * q), at(p + 2 + 2 * q) >> 4, at(p + 2 + 2 * q) & 15) for q in range(n)]
            ss, se, ah, al = at(p + 1 + 2 * n), at(p + 2 + 2 * n), at(p + 3 + 2 * n) >> 4, at(p + 3 + 2 * n) & 15
            if frame is None or len(scans) >= 255 or not 1 <= n <= 3:
                raise _Refused(UNSUPPORTED_FORMAT)
            ids = [f[0] for f in frame]
            if any(s[0] not in ids for s in sel):
                raise _Refused(UNSUPPORTED_FORMAT)
            comps = [ids.index(s[0]) for s in sel]
            # T.81 G.1.1.1 and libjpeg's coef_bits rule
            ok = len(set(comps)) == n and ss <= se <= 63 and al <= 13 and ((se == 0) if ss == 0 else (n == 1))
            for c in comps:
                ok = ok and (ss == 0 or (c, 0) in bits_sent)
                for k in range(ss, se + 1):
                    prev = bits_sent.get((c, k))
                    ok = ok and (ah == 0 if prev is None else (ah == prev and al == ah - 1))
            if not ok:
                raise _Refused(UNSUPPORTED_FORMAT)
            for c in comps:
                for k in range(ss, se + 1):
                    bits_sent[(c, k)] = al
            tabs = []
            for (_, td, ta) in sel:
                if ss == 0 and ah == 0 and td not in dc:
                    raise _Refused(MISSING_TABLE)
                if ss != 0 and ta not in ac:
                    raise _Refused(MISSING_TABLE)
                tabs.append(ac.get(ta) if ss else dc.get(td))
            for c in comps:
                if c not in latched:
                    if frame[c][3] not in qt:
                        raise _Refused(MISSING_TABLE)
                    latched[c] = qt[frame[c][3]]
            # the entropy-coded segment: FF00 -> FF, fill bytes skipped, RSTn cut the intervals (with a restart interval defined)
            k, cur, parts = end, bytearray(), []
            while k < len(data):
                b = data[k]
                if b != 0xff:
                    cur.append(b)
                    k += 1
                elif k + 1 >= len(data):
                    cur.append(b)
                    k += 1
                elif data[k + 1] == 0:
                    cur.append(0xff)
                    k += 2
                elif data[k + 1] == 0xff:
                    k += 1
                elif dri and 0xd0 <= data[k + 1] <= 0xd7:
                    parts.append(bytes(cur))
                    cur = bytearray()
                    k += 2
                else:
                    break
            parts.append(bytes(cur))
            scans.append((comps, ss, se, ah, al, tabs, dri, parts))
            i = k
            continue
        else:
            at(end - 1)
        i = end
    if frame is None or not scans:
        raise _Refused(UNSUPPORTED_FORMAT)
    if any((c, 0) not in bits_sent for c in range(len(frame))):
        raise _Refused(UNSUPPORTED_FORMAT)
    return frame, size, scans


def decode(data):
    data = bytes(data)
    try:
        frame, (width, height), scans = _walk(data)
    except _Refused as e:
        return Result(e.code)
    ncomp = len(frame)
    hv = [(1, 1)] if ncomp == 1 else [(f[1], f[2]) for f in frame]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    grid = [(-(-(width * h) // (8 * hmax)), -(-(height * v) // (8 * vmax))) for h, v in hv]      # the components' own block grids
    store = [dict() for _ in range(ncomp)]                       # (bx, by) -> 64 coefficients

    def block(c, bx, by):
        return store[c].setdefault((bx, by), [0] * 64)

    st = {"symbols": 0, "bad": False, "short": False, "max_eob_category": -1, "zrl_over_history": 0, "eob_run_corrections": 0}
    for comps, ss, se, ah, al, tabs, dri, parts in scans:
        if len(comps) > 1:
            units = [[(q, c, (m % mcux) * hv[c][0] + j % hv[c][0], (m // mcux) * hv[c][1] + j // hv[c][0])
                      for q, c in enumerate(comps) for j in range(hv[c][0] * hv[c][1])] for m in range(mcux * mcuy)]
        else:
            c = comps[0]
            units = [[(0, c, bx, by)] for by in range(grid[c][1]) for bx in range(grid[c][0])]
        per = dri if dri else len(units)
        nint = -(-len(units) // per)
        if len(parts) < nint:
            return Result(TRUNCATED)
        for g in range(nint):
            b = _Bits(parts[g])
            pred, eobrun = [0, 0, 0], 0
            stop = False
            for unit in units[g * per:(g + 1) * per]:
                for q, c, bx, by in unit:
                    blk = block(c, bx, by)
                    if ss == 0:
                        if ah == 0:
                            s = _symbol(b, tabs[q], st)
                            s = 0 if s is None else s
                            pred[q] = (pred[q] + _extend(b.get(s), s)) & 0xffffffff
                            blk[0] = _i16(pred[q] << al)
                        elif b.bit():
                            blk[0] = _i16(blk[0] | (1 << al))
                    elif ah == 0:
                        eobrun = _ac_first(b, blk, ss, se, al, tabs[0], eobrun, st)
                    else:
                        eobrun = _ac_refine(b, blk, ss, se, al, tabs[0], eobrun, st)
                    if b.short():
                        st["short"] = stop = True
                        break
                if stop:
                    break
            if not stop and eobrun:
                st["bad"] = True
    if st["short"]:
        return Result(TRUNCATED, stats=st)
    if st["bad"]:
        return Result(BAD_HUFFMAN, stats=st)
    bpm = sum(h * v for h, v in hv)
    out = np.zeros((mcux * mcuy * bpm, 64), np.int16)
    k = 0
    for m in range(mcux * mcuy):
        for c, (h, v) in enumerate(hv):
            for j in range(h * v):
                bx, by = (m % mcux) * h + j % h, (m // mcux) * v + j // h
                if bx < grid[c][0] and by < grid[c][1] and (bx, by) in store[c]:
                    out[k] = store[c][(bx, by)]
                k += 1
    st["scans"] = len(scans)
    return Result(OK, out, st, dict(width=width, height=height, hv=hv, mcux=mcux, mcuy=mcuy, grid=grid))


def _ac_first(b, blk, ss, se, al, table, eobrun, st):
    if eobrun:
        return eobrun - 1
    k = ss
    while k <= se:
        sym = _symbol(b, table, st)
        if sym is None:
            k += 1
            continue
        r, s = sym >> 4, sym & 15
        if s:
            k += r
            v = _extend(b.get(s), s)
            if k > se:
                st["bad"] = True
                return 0
            blk[k] = _i16(v << al)
            k += 1
        elif r == 15:
            k += 16
        else:
            st["max_eob_category"] = max(st["max_eob_category"], r)
            return (1 << r) + b.get(r) - 1
    return 0


def _correct(b, blk, k, p1):
    v = blk[k]
    if b.bit() and (v & p1) == 0:
        blk[k] = _i16(v + p1 if v >= 0 else v - p1)


def _ac_refine(b, blk, ss, se, al, table, eobrun, st):
    p1, k = 1 << al, ss
    if not eobrun:
        while k <= se:
            sym = _symbol(b, table, st)
            if sym is None:
                k += 1
                continue
            r, size, s = sym >> 4, sym & 15, 0
            if size:
                if size != 1:
                    st["bad"] = True
                s = p1 if b.bit() else -p1
            elif r != 15:
                st["max_eob_category"] = max(st["max_eob_category"], r)
                eobrun = (1 << r) + b.get(r)
                break
            while k <= se:
                if blk[k] != 0:
                    _correct(b, blk, k, p1)
                    if not size and r >= 0:
                        st["zrl_over_history"] += 1            # a ZRL's run passes over a coefficient sent earlier
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if s:
                if k > se:
                    st["bad"] = True
                    return eobrun
                blk[k] = _i16(s)
            k += 1
    if eobrun:
        while k <= se:
            if blk[k] != 0:
                _correct(b, blk, k, p1)
                st["eob_run_corrections"] += 1                 # a correction bit inside an end-of-band run
            k += 1
        eobrun -= 1
    return eobrun

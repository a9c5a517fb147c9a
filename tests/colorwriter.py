"""Files whose colour model is not "Y, Cb, Cr by position", for the tests of mjx_opts.color (tests/test_color_models.py,
tests/test_color_decode.py): three components stored as R, G, B and four-component CMYK / YCCK files in any sampling layout, with
JFIF APP0 and Adobe APP14 segments and component ids of the test's choosing.  Built on tests/jpegwriter.py, whose write_jpeg and
encode_scan_np take any component list; this module adds the head segments, the fourth component, and the twins a test builds its
exact expectation from: the one-component file that carries a component's blocks, and the three-component file that carries the
first three."""
import struct

import numpy as np

import jpegwriter as jw

JFIF = b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def app0(payload=JFIF):
    return b"\xff\xe0" + struct.pack(">H", 2 + len(payload)) + payload


def app14(transform, tag=b"Adobe", length=12):
    """An Adobe APP14 segment: tag, version 100, flags0, flags1, transform -- 12 payload bytes; `length` cuts or pads the payload."""
    p = (tag + struct.pack(">HHHB", 100, 0, 0, transform))[:length]
    p += b"\x00" * (length - len(p))
    return b"\xff\xee" + struct.pack(">H", 2 + len(p)) + p


def with_head(data, *segments):
    """The file with the segments put in right behind SOI."""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"".join(segments) + data[2:]


def strip_app14(data):
    """The file without its APP14 segments (in front of the first SOS)."""
    out, i = bytearray(data[:2]), 2
    while i + 4 <= len(data) and data[i] == 0xff:
        m = data[i + 1]
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        if m == 0xda:
            break
        if m != 0xee:
            out += data[i:i + 2 + ln]
        i += 2 + ln
    return bytes(out) + data[i:]


class ColorFile:
    """data: the file; hv: [(h, v)] per component; blocks[c]: int [n, 64] component c's quantised blocks in decode order (MCU-major,
    v x h inside the MCU), zig-zag, absolute DC; qts[c]: its table (64 zig-zag entries); tables: {(class, slot): (bits, vals)};
    slot[c]: its Huffman slot; width, height, mcux, mcuy."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _slots(nc, tq, huff):
    """the DQT slot and the (DC slot, AC slot) pair of each component; default: Adobe's 0, 1, 1, 0 for all three"""
    slot = [0, 1, 1, 0][:nc]
    tq = list(slot) if tq is None else [int(t) for t in tq]
    huff = [(s, s) for s in slot] if huff is None else [(int(d), int(a)) for d, a in huff]
    assert len(tq) == nc and len(huff) == nc and all(0 <= t < 4 for t in tq) and all(0 <= d < 4 and 0 <= a < 4 for d, a in huff)
    return slot, tq, huff


def color_from_blocks(blocks_per_component, hv, mcux, mcuy, qts, tq, tables, huff, head=(), width=None, height=None, restart=None, ids=None):
    """jpegwriter.jpeg_from_blocks for three or four components with tables of the caller's choosing: a baseline file in one interleaved
    scan whose blocks carry exactly the coefficients given.  blocks_per_component[c]: int [mcux mcuy h v, 64] in decode order (MCU-major,
    v x h inside the MCU), zig-zag, absolute DC, before dequantisation.  qts: {slot: 64 zig-zag entries}, up to four; a table with an
    entry above 255 is written with 16-bit entries, the others with 8-bit ones.  tq[c]: component c's DQT slot.  tables: {(class, slot):
    (bits, vals)}, up to four pairs; huff[c] = (DC slot, AC slot).  head: segments behind SOI; width, height: the frame's (default the
    whole MCU grid; smaller values clip the last MCUs); restart=n: DRI n, RSTn every n MCUs.  -> ColorFile"""
    hv = [tuple(x) for x in hv]
    nc = len(hv)
    assert nc in (3, 4) and len(blocks_per_component) == nc
    slot, tq, huff = _slots(nc, tq, huff)
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    width = mcux * 8 * hmax if width is None else width
    height = mcuy * 8 * vmax if height is None else height
    assert -(-width // (8 * hmax)) == mcux and -(-height // (8 * vmax)) == mcuy, (width, height, mcux, mcuy)
    per_mcu = [h * v for h, v in hv]
    bpm = sum(per_mcu)
    blocks = [np.asarray(b, np.int64) for b in blocks_per_component]
    assert all(b.shape == (mcux * mcuy * k, 64) for b, k in zip(blocks, per_mcu)), [b.shape for b in blocks]
    qts = {int(s): [int(v) for v in q] for s, q in qts.items()}
    assert len(qts) <= 4 and all(t in qts for t in tq) and all(1 <= v <= 65535 for q in qts.values() for v in q)
    dhts = {(int(cls), int(s)): (list(t[0]), list(t[1])) for (cls, s), t in tables.items()}
    assert all((0, d) in dhts and (1, a) in dhts for d, a in huff)
    order = np.concatenate([b.reshape(mcux * mcuy, k, 64) for b, k in zip(blocks, per_mcu)], axis=1).reshape(-1, 64)
    owner = [c for c, k in enumerate(per_mcu) for _ in range(k)] * (mcux * mcuy)
    dc = {c: jw.huff_codes(*dhts[(0, huff[c][0])]) for c in range(nc)}
    ac = {c: jw.huff_codes(*dhts[(1, huff[c][1])]) for c in range(nc)}
    ent = jw.encode_scan_np(order, owner, dc, ac, restart_blocks=(restart or 0) * bpm)
    ids = list(ids) if ids is not None else list(range(1, nc + 1))
    comps = [(ids[c], h, v, tq[c], huff[c][0], huff[c][1]) for c, (h, v) in enumerate(hv)]
    wide = {s for s, q in qts.items() if max(q) > 255}
    data = with_head(jw.write_jpeg(width, height, comps, qts, dhts, ent, qt16=wide, restart_interval=restart or 0), *head)
    plain = tq == slot and huff == [(s, s) for s in slot]
    return ColorFile(data=data, hv=hv, blocks=blocks, qts=[qts[t] for t in tq], tables=dhts, slot=slot if plain else list(huff), tq=tq,
                     huff=huff, qt_slots=qts, width=width, height=height, mcux=mcux, mcuy=mcuy, hmax=hmax, vmax=vmax, bpm=bpm, order=order,
                     owner=owner, codes=(dc, ac), entropy=ent, restart=restart or 0, head=tuple(head))


def color_jpeg(width, height, hv, ids=None, head=(), quality=75, seed=0, restart=None, noise=4.0, k_swing=0.0, tq=None, huff=None,
               qts=None, tables=None):
    """A baseline file of len(hv) in (3, 4) components in one interleaved scan, written from float64 DCT coefficients: smooth plane
    waves plus gaussian noise per component at its own resolution over the whole MCU grid.  By default components 0 and 3 code with the
    luminance tables and DQT (slot 0), 1 and 2 with the chrominance ones (slot 1), as Adobe's writer does.  ids: the component ids
    (default 1, 2, ...); head: segments to put behind SOI (app0(), app14(t)).  k_swing: the last component gets a checkerboard of
    +- k_swing per 8 x 8 block on top, so that its DC differences are large and of both signs.  restart=n: DRI n, RSTn every n MCUs.
    tq: a DQT slot per component; huff: a (DC slot, AC slot) pair per component; qts: {slot: table}, up to four, 8-bit or 16-bit
    (default: the Annex K tables at `quality` on slots 0 and 1); tables: {(class, slot): (bits, vals)}, up to four pairs (default: the
    Annex K tables on slots 0 and 1)."""
    rng = np.random.default_rng(seed)
    hv = [tuple(x) for x in hv]
    nc = len(hv)
    assert nc in (3, 4)
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    _, tq, huff = _slots(nc, tq, huff)
    qt = {0: jw.quality_table(jw.ANNEX_K_LUMA, quality), 1: jw.quality_table(jw.ANNEX_K_CHROMA, quality)} if qts is None else dict(qts)
    if tables is None:
        ak = jw._annex_k_tables()
        tables = {(cls, s): ak[(cls, s)] for s in (0, 1) for cls in (0, 1)}
    blocks = []
    for c, (h, v) in enumerate(hv):
        ph, pw = mcuy * v * 8, mcux * h * 8
        yy, xx = np.mgrid[0:ph, 0:pw].astype(np.float64)
        p = np.zeros((ph, pw))
        for _ in range(3):
            fx, fy, ph0 = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0, 2 * np.pi)
            p += 20.0 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph0)
        p += rng.normal(0.0, noise, p.shape)
        if k_swing and c == nc - 1:
            p += k_swing * (1.0 - 2.0 * (((yy // 8) + (xx // 8)) % 2))
        p = np.clip(p, -128.0, 127.0)
        b = jw.fdct_quantise(p, qt[tq[c]])
        blocks.append(b.reshape(mcuy, v, mcux, h, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64))
    return color_from_blocks(blocks, hv, mcux, mcuy, qt, tq, tables, huff, head, width, height, restart, ids)


def cut_in_last_mcu(cf, keep=2):
    """The file cut inside its last MCU: everything up to the coding of all MCUs but the last, `keep` bytes more, and nothing
    behind them (no EOI).  The last MCU must be long enough for that to leave it incomplete by more than the decoder's look-ahead."""
    assert cf.data.endswith(cf.entropy + b"\xff\xd9")
    n = len(cf.order) - cf.bpm
    prefix = jw.encode_scan_np(cf.order[:n], cf.owner[:n], cf.codes[0], cf.codes[1])
    assert len(cf.entropy) - len(prefix) >= keep + 16, "the last MCU is too short for this cut"
    return cf.data[:len(cf.data) - 2 - len(cf.entropy) + len(prefix) + keep]


def component_twin(cf, c):
    """The one-component file that carries component c's blocks and quantisation table over the component's whole block grid
    (mcux h x mcuy v blocks): its packed decode has component c's byte at sample (x, y) in the R byte of pixel (x, y)."""
    h, v = cf.hv[c]
    raster = cf.blocks[c].reshape(cf.mcuy, cf.mcux, v, h, 64).transpose(0, 2, 1, 3, 4).reshape(-1, 64)
    td, ta = cf.slot[c] if isinstance(cf.slot[c], tuple) else (cf.slot[c], cf.slot[c])
    tables = {(0, 0): cf.tables[(0, td)], (1, 0): cf.tables[(1, ta)]}
    return jw.jpeg_from_blocks(raster, [(1, 1)], cf.mcux * h, cf.mcuy * v, [cf.qts[c]], tables, qt16=max(cf.qts[c]) > 255)


def ycc_twin(cf):
    """The three-component file that carries components 0 .. 2 (they must attain hmax and vmax, so that the geometry is the same):
    its packed decode is the (r, g, b) a YCCK picture multiplies by K."""
    hv = cf.hv[:3]
    assert max(h for h, _ in hv) == cf.hmax and max(v for _, v in hv) == cf.vmax
    if isinstance(cf.slot[0], tuple) and getattr(cf, "qt_slots", None) is not None:
        # (tables of the file's own choosing: each component keeps its DQT slot and its pair of Huffman slots)
        return color_from_blocks(cf.blocks[:3], hv, cf.mcux, cf.mcuy, {t: cf.qt_slots[t] for t in set(cf.tq[:3])}, cf.tq[:3],
                                 {(cls, s): cf.tables[(cls, s)] for d, a in cf.huff[:3] for cls, s in ((0, d), (1, a))}, cf.huff[:3],
                                 width=cf.width, height=cf.height).data
    per_mcu = [h * v for h, v in hv]
    n = cf.mcux * cf.mcuy
    order = np.concatenate([cf.blocks[c].reshape(n, per_mcu[c], 64) for c in range(3)], axis=1).reshape(-1, 64)
    # (jpeg_from_blocks codes component 0 with slot 0 and the others with slot 1: any tables that hold the symbols do)
    tables = {k: cf.tables[k] for k in ((0, 0), (1, 0), (0, 1), (1, 1)) if k in cf.tables}
    return jw.jpeg_from_blocks(order, hv, cf.mcux, cf.mcuy, cf.qts[:3], tables, width=cf.width, height=cf.height)


def read_baseline(data):
    """A file written by someone else (Pillow), read by a bit-serial decoder of this module's own: one interleaved baseline scan without
    restart intervals -> the ColorFile of it (blocks per component in decode order, zig-zag, absolute DC), from which the twins are
    built.  Slow and plain on purpose; for pictures of a few hundred blocks."""
    be16 = lambda b, k: (b[k] << 8) | b[k + 1]
    i, qt, dht, frame, sel = 2, {}, {}, None, None
    while sel is None:
        assert data[i] == 0xff
        m, ln = data[i + 1], be16(data, i + 2)
        p = data[i + 4:i + 2 + ln]
        if m == 0xdb:
            j = 0
            while j < len(p):
                wide = p[j] >> 4
                qt[p[j] & 15] = [be16(p, j + 1 + 2 * k) for k in range(64)] if wide else list(p[j + 1:j + 65])
                j += 129 if wide else 65
        elif m == 0xc4:
            j = 0
            while j < len(p):
                bits = list(p[j + 1:j + 17])
                dht[(p[j] >> 4, p[j] & 15)] = (bits, list(p[j + 17:j + 17 + sum(bits)]))
                j += 17 + sum(bits)
        elif m == 0xc0:
            height, width = be16(p, 1), be16(p, 3)
            frame = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(p[5])]
        elif m == 0xdd:
            assert be16(p, 0) == 0
        elif m == 0xda:
            sel = [(p[1 + 2 * c], p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
        i += 2 + ln
    assert frame is not None and [f[0] for f in frame] == [q[0] for q in sel]
    raw = bytearray()
    while not (data[i] == 0xff and data[i + 1] == 0xd9):
        raw.append(data[i])
        i += 2 if data[i] == 0xff and data[i + 1] == 0 else 1
    bitstr = "".join("{:08b}".format(b) for b in raw)
    pos = 0
    lookup = {}
    for key, (bits, vals) in dht.items():
        lookup[key] = {"{:0{}b}".format(code, ln): sym for sym, (code, ln) in jw.huff_codes(bits, vals).items()}

    def symbol(tab):
        nonlocal pos
        for ln in range(1, 17):
            s = tab.get(bitstr[pos:pos + ln])
            if s is not None:
                pos += ln
                return s
        raise ValueError("no code")

    def value(size):
        nonlocal pos
        if size == 0:
            return 0
        v = int(bitstr[pos:pos + size], 2)
        pos += size
        return v if v >> (size - 1) else v - (1 << size) + 1

    hv = [(f[1], f[2]) for f in frame]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    blocks, pred = [[] for _ in hv], [0] * len(hv)
    for _ in range(mcux * mcuy):
        for c, (h, v) in enumerate(hv):
            for _ in range(h * v):
                blk = [0] * 64
                pred[c] += value(symbol(lookup[(0, sel[c][1])]))
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(lookup[(1, sel[c][2])])
                    if rs == 0:
                        break
                    k += rs >> 4
                    if rs & 15:
                        blk[k] = value(rs & 15)
                    k += 1
                blocks[c].append(blk)
    return ColorFile(data=data, hv=hv, blocks=[np.asarray(b, np.int64) for b in blocks], qts=[qt[f[3]] for f in frame], tables=dht,
                     slot=[(q[1], q[2]) for q in sel], width=width, height=height, mcux=mcux, mcuy=mcuy, hmax=hmax, vmax=vmax,
                     bpm=sum(h * v for h, v in hv))


def replicate(plane, h, v, hmax, vmax, out_w, out_h):
    """Box replication at the output resolution: pixel (X, Y) takes sample (X h // hmax, Y v // vmax) of the component's plane."""
    ys = (np.arange(out_h) * v) // vmax
    xs = (np.arange(out_w) * h) // hmax
    return plane[np.ix_(ys, xs)]


def ink_mul(a, k):
    """(a k + 127) // 255 on uint8 arrays (mjx.h: mjx_ink_mul)."""
    return ((a.astype(np.uint32) * k.astype(np.uint32) + 127) // 255).astype(np.uint8)


def compose(model, cf, comp_bytes, out_w, out_h, rgb3=None):
    """The packed picture of `cf` under `model` ("rgb", "cmyk", "ycck") from the bytes of its components: comp_bytes[c] the R plane of
    component_twin(cf, c)'s packed decode (at the same scale), rgb3 the packed decode of ycc_twin(cf) for "ycck"."""
    s = [None if p is None else replicate(p, h, v, cf.hmax, cf.vmax, out_w, out_h) for p, (h, v) in zip(comp_bytes, cf.hv)]
    if model == "rgb":
        return np.stack(s[:3], axis=-1)
    if model == "cmyk":
        return np.stack([ink_mul(s[c], s[3]) for c in range(3)], axis=-1)
    assert model == "ycck" and rgb3 is not None and rgb3.shape[:2] == (out_h, out_w)
    return np.stack([ink_mul(255 - rgb3[..., c], s[3]) for c in range(3)], axis=-1)          # (C = 255 - R: libjpeg's ycck_cmyk_convert)

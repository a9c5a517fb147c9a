"""Numpy reference of the scaled decode (include/mjx.h, mjx_opts.scale_denom), in float64.

Inputs: the oracle's STANDARD-layout T0 coefficients (per component, blocks in decode order, MCU-major, v x h inside the MCU,
zig-zag order, DC prediction applied), the file's DQT tables and its SOF sampling factors.  Per block the low N x N corner
(N = 8 / s) of the dequantised coefficients goes through

    f(x,y) = 1/4 sum_{u,v<N} C(u) C(v) F(u,v) cos((2x+1) u pi / 2N) cos((2y+1) v pi / 2N),   C(0) = 1/sqrt(2), C(k>0) = 1

(+ 128 on luminance); output pixel (X, Y) takes the sample at (X h / Hmax, Y v / Vmax) of each component's plane, then the
STANDARD layout's colour formula (decoder.rs:392-402) and its clamping, truncating store (decoder.rs:382-390).
"""
import math
import struct

import numpy as np

import oracle_binding as orc

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])


def jpeg_tables(data):
    """-> (width, height, [(h, v, tq) per component in frame order], {slot: 64 DQT entries in zig-zag order}), from the
    first SOF0/SOF1 and the DQT segments in front of it."""
    qt, comps, i = {}, None, 2
    while i + 4 <= len(data):
        if data[i] != 0xFF:
            i += 1
            continue
        m = data[i + 1]
        if m in (0x01, 0xFF) or 0xD0 <= m <= 0xD8:
            i += 2 if m != 0xFF else 1
            continue
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + ln]
        if m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if pq:
                    qt[tq] = list(struct.unpack(">64H", seg[j + 1:j + 129]))
                    j += 129
                else:
                    qt[tq] = list(seg[j + 1:j + 65])
                    j += 65
        elif m in (0xC0, 0xC1):
            h_, w_ = struct.unpack(">HH", seg[1:5])
            nc = seg[5]
            comps = [(seg[6 + 3 * k + 1] >> 4, seg[6 + 3 * k + 1] & 15, seg[6 + 3 * k + 2]) for k in range(nc)]
            return w_, h_, comps, qt
        elif m == 0xDA:
            break
        i += 2 + ln
    raise ValueError("no baseline SOF")


def _basis(n):
    """M[x, u] = C(u) cos((2x+1) u pi / 2N)"""
    m = np.empty((n, n))
    for x in range(n):
        for u in range(n):
            m[x, u] = (math.sqrt(0.5) if u == 0 else 1.0) * math.cos((2 * x + 1) * u * math.pi / (2 * n))
    return m


def planes(data, scale, dec=None, magnitude=False):
    """-> (width, height, comps, [scaled plane per component, float64, the full MCU grid], hmax, vmax)
    magnitude=True: the planes hold, at every sample, S_c of its block instead: sum |coef q| / 8 over the N x N corner the transform
    reads (+ 128 on luminance) -- what a sample's rounding error scales with (rgb_interval)."""
    w, h, comps, qt = jpeg_tables(data)
    if dec is None:
        dec = orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)
    if len(comps) == 1:
        comps = [(1, 1, comps[0][2])]          # (one component: non-interleaved, one block per MCU whatever SOF0 says)
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    n = 8 // scale
    M = _basis(n)
    out = []
    for c, (hc, vc, tq) in enumerate(comps):
        co = dec.coefs[c].astype(np.float64)
        assert co.shape[0] == mcux * mcuy * hc * vc, (co.shape, mcux, mcuy, hc, vc)
        deq = co * np.asarray(qt[tq], np.float64)[None, :]
        nat = np.zeros_like(deq)
        nat[:, ZIGZAG] = deq                    # natural index = row (vertical frequency) * 8 + column
        F = nat.reshape(-1, 8, 8)[:, :n, :n]
        if magnitude:
            S = np.broadcast_to((np.abs(F).sum(axis=(1, 2)) / 8.0)[:, None, None], (F.shape[0], n, n))
        else:
            S = 0.25 * np.einsum("yv,bvu,xu->byx", M, F, M)
        if c == 0:
            S = S + 128.0
        S = S.reshape(mcuy, mcux, vc, hc, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * vc * n, mcux * hc * n)
        out.append(S)
    return w, h, comps, out, hmax, vmax


def to_u8(x):
    """decoder.rs:382-390 f32_to_u8: clamp to [0, 255], truncate.  A value within 1e-9 of an integer counts as that integer: the
    float64 sums can leave an exactly integral sample (a flat block, C(0)^2 = 1/2 times a negative DC) a few ulps below it, where
    truncation would drop a whole level the contract does not drop."""
    return np.trunc(np.clip(np.round(x, 9), 0.0, 255.0)).astype(np.uint8)


def _samples(data, scale, dec, magnitude=False):
    """-> [per component the plane sample (or its block's magnitude) under every output pixel, float64 [ceil(H/s), ceil(W/s)]]"""
    w, h, comps, pl, hmax, vmax = planes(data, scale, dec, magnitude)
    ow, oh = -(-w // scale), -(-h // scale)
    X, Y = np.arange(ow), np.arange(oh)
    return [p[(Y * vc // vmax)[:, None], (X * hc // hmax)[None, :]] for (hc, vc, _), p in zip(comps, pl)]


def rgb_f64(data, scale, dec=None):
    """-> the picture of `data` at 1/scale before the store, float64 [ceil(H/s), ceil(W/s), 3] (unclamped; one component: R = G = B)"""
    smp = _samples(data, scale, dec)
    if len(smp) == 1:
        return np.repeat(smp[0][:, :, None], 3, axis=2)
    y, cb, cr = smp
    c_red, c_green, c_blue = 0.299, 0.587, 0.114
    r = cr * (2 - 2 * c_red) + y
    b = cb * (2 - 2 * c_blue) + y
    g = (y - c_blue * b - c_red * r) / c_green
    return np.stack([r, g, b], axis=2)


def scaled_rgb(data, scale, dec=None):
    """-> the expected picture [ceil(H/s), ceil(W/s), 3] uint8 of `data` decoded at 1/scale (scale 1: the full-size picture)"""
    return to_u8(rgb_f64(data, scale, dec))


def magnitude(data, scale, dec=None):
    """m = S_Y + 2 S_Cb + 2 S_Cr under every output pixel, float64 [ceil(H/s), ceil(W/s)]: S_c = sum |coef q| / 8 over the corner
    of the block the pixel's sample of component c comes from (+ 128 on luminance).  Every float32 operation between the
    coefficients and a channel value works on numbers no larger than this (the colour formula's chroma gains are below 2)."""
    s = _samples(data, scale, dec, magnitude=True)
    return s[0] if len(s) == 1 else s[0] + 2.0 * s[1] + 2.0 * s[2]


def trunc_u8(x):
    """clamp to [0, 255], truncate: to_u8 without its 1e-9 rounding (rgb_interval's delta takes its place)"""
    return np.trunc(np.clip(x, 0.0, 255.0)).astype(np.uint8)


def rgb_interval(data, scale, K, dec=None):
    """-> (lo, hi), uint8 [ceil(H/s), ceil(W/s), 3]: the bytes a float32 decoder of `data` at 1/scale may produce.  With w the float64
    value of a channel (rgb_f64) and m the pixel's magnitude, delta = K 2^-24 m, lo = trunc_u8(w - delta), hi = trunc_u8(w + delta):
    K half-ulps of the largest number the sample's arithmetic handles.  lo == hi (nearly everywhere): the byte is float64's.
    A channel whose components' blocks have nothing inside the corner (all N x N coefficients zero; R takes Y and Cr, B takes Y and
    Cb, G all three) is exactly 128 in any arithmetic: there delta = 0 and lo = hi = 128."""
    w = rgb_f64(data, scale, dec)
    mag = _samples(data, scale, dec, magnitude=True)
    e = [s == (128.0 if c == 0 else 0.0) for c, s in enumerate(mag)]
    empty = np.stack([e[0]] * 3 if len(e) == 1 else [e[0] & e[2], e[0] & e[1] & e[2], e[0] & e[1]], axis=2)
    m = mag[0] if len(mag) == 1 else mag[0] + 2.0 * mag[1] + 2.0 * mag[2]
    d = (K * 2.0 ** -24 * m)[:, :, None]
    lo, hi = trunc_u8(w - d), trunc_u8(w + d)
    lo[empty], hi[empty] = 128, 128
    return lo, hi


# ---- RGB, CMYK and YCCK files (mjx.h: MJX_OPTS_COLOR) ------------------------------------------------------------------------------
def _color_file(cf_or_data):
    """a colorwriter.ColorFile as it is; a file's bytes (one interleaved baseline scan without restart intervals) read back into one"""
    if isinstance(cf_or_data, (bytes, bytearray)):
        import colorwriter
        return colorwriter.read_baseline(bytes(cf_or_data))
    return cf_or_data


def component_samples(cf, c, scale, qt=None):
    """-> (sample, magnitude) of component c under every output pixel of the picture at 1/scale, float64 [ceil(H/s), ceil(W/s)]: the
    sample without a level shift (planes()'s transform on the blocks written, box replication), and S_c = sum |coef q| / 8 over the
    corner of the sample's block.  qt: the table to dequantise with (default the component's own)."""
    n = 8 // scale
    M = _basis(n)
    hc, vc = cf.hv[c]
    deq = np.asarray(cf.blocks[c], np.float64) * np.asarray(cf.qts[c] if qt is None else qt, np.float64)[None, :]
    nat = np.zeros_like(deq)
    nat[:, ZIGZAG] = deq
    F = nat.reshape(-1, 8, 8)[:, :n, :n]
    S = 0.25 * np.einsum("yv,bvu,xu->byx", M, F, M)
    A = np.broadcast_to((np.abs(F).sum(axis=(1, 2)) / 8.0)[:, None, None], S.shape)
    ow, oh = -(-cf.width // scale), -(-cf.height // scale)
    ys, xs = (np.arange(oh) * vc // cf.vmax)[:, None], (np.arange(ow) * hc // cf.hmax)[None, :]
    grid = lambda p: p.reshape(cf.mcuy, cf.mcux, vc, hc, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(cf.mcuy * vc * n, cf.mcux * hc * n)[ys, xs]
    return grid(S), grid(A)


def byte_interval(sample, mag, K):
    """-> (lo, hi) uint8 of a component that leaves as a byte of its own: the sample + 128 moved by K half-ulps of its magnitude
    S_c + 128 and truncated, as rgb_interval does for grey; a block with nothing inside the corner is exactly 128."""
    w, m = sample + 128.0, mag + 128.0
    d = K * 2.0 ** -24 * m
    lo, hi = trunc_u8(w - d), trunc_u8(w + d)
    lo[mag == 0.0], hi[mag == 0.0] = 128, 128
    return lo, hi


def ink_mul(a, k):
    """(a k + 127) // 255 on uint8 arrays (mjx.h: mjx_ink_mul)"""
    return ((a.astype(np.uint32) * k.astype(np.uint32) + 127) // 255).astype(np.uint8)


def ycc_part(cf):
    """(the three-component file of components 0 .. 2, a stand-in for its decode) -- what rgb_f64 and rgb_interval take"""
    import types
    import colorwriter
    return colorwriter.ycc_twin(cf), types.SimpleNamespace(coefs=[np.asarray(b) for b in cf.blocks[:3]], mcus=cf.mcux * cf.mcuy)


def model_interval(cf_or_data, model, scale, K):
    """-> (lo, hi), uint8 [ceil(H/s), ceil(W/s), 3]: the bytes a float32 decoder of an "rgb", "cmyk" or "ycck" file may produce at
    1/scale.  Per component the float64 sample under every output pixel, + 128 on every component that leaves as a byte of its own,
    moved by K half-ulps of S_c + 128 and truncated (byte_interval).  RGB: the three intervals.  CMYK: [mul(lo_c, lo_K), mul(hi_c,
    hi_K)] -- ink_mul is non-decreasing in both arguments.  YCCK: rgb_interval of the three-component part, complemented (the ends
    swap), then the same product with K's interval."""
    cf = _color_file(cf_or_data)
    assert model in ("rgb", "cmyk", "ycck") and len(cf.hv) == (3 if model == "rgb" else 4)
    if model == "ycck":
        data3, dec3 = ycc_part(cf)
        rlo, rhi = rgb_interval(data3, scale, K, dec3)
        lo3, hi3 = 255 - rhi, 255 - rlo
    else:
        iv = [byte_interval(*component_samples(cf, c, scale), K) for c in range(3)]
        lo3, hi3 = np.stack([a for a, _ in iv], axis=2), np.stack([b for _, b in iv], axis=2)
    if model == "rgb":
        return lo3, hi3
    klo, khi = byte_interval(*component_samples(cf, 3, scale), K)
    return ink_mul(lo3, klo[:, :, None]), ink_mul(hi3, khi[:, :, None])


def model_bytes(cf_or_data, model, scale, plant=None):
    """-> the float64 picture of the file at 1/scale, uint8 [ceil(H/s), ceil(W/s), 3] (model_interval with K = 0, but for the samples
    that are exactly whole).  plant: one error on purpose, for the tests that show the inputs tell it from the truth --
      "k_table0"        K dequantised with component 0's table          "k_table0_scaled"  the same at scales 2, 4, 8 only
      "mul_no_127"      mul(a, k) = a k / 255 without the + 127          "ycck_no_complement"  R = mul(r, K) instead of mul(255 - r, K)
      "k_no_128"        K without its + 128                              "swap_1_3"  components 1 and 3 take each other's place"""
    cf = _color_file(cf_or_data)
    assert plant in (None, "k_table0", "k_table0_scaled", "mul_no_127", "ycck_no_complement", "k_no_128", "swap_1_3")
    order = [0, 3, 2, 1] if plant == "swap_1_3" else [0, 1, 2, 3]

    def byte_of(c, shift=128.0, qt=None):
        """component c's byte where the picture has component `order[c]`'s place: its own sampling, its own table"""
        return to_u8(component_samples(cf, c, scale, qt)[0] + shift)
    if model == "ycck":
        assert plant != "swap_1_3" or cf.hv[1] == cf.hv[3]
        data3, dec3 = ycc_part(cf)
        if plant == "swap_1_3":                     # (K's blocks in Cb's place and the other way round: the same sampling)
            import types
            swapped = types.SimpleNamespace(**cf.__dict__)
            swapped.blocks = [cf.blocks[k] for k in order]
            swapped.qts = [cf.qts[k] for k in order]
            return model_bytes(swapped, model, scale)
        three = to_u8(rgb_f64(data3, scale, dec3))
        if plant != "ycck_no_complement":
            three = 255 - three
    else:
        three = np.stack([byte_of(order[c]) for c in range(3)], axis=2)
    if model == "rgb":
        return three
    kq = cf.qts[0] if plant == "k_table0" or (plant == "k_table0_scaled" and scale > 1) else None
    k = byte_of(order[3], 0.0 if plant == "k_no_128" else 128.0, kq)[:, :, None]
    if plant == "mul_no_127":
        return ((three.astype(np.uint32) * k.astype(np.uint32)) // 255).astype(np.uint8)
    return ink_mul(three, k)


def box_mean(rgb, s):
    """s x s box mean of a full-size picture (edge boxes: what they cover) -> float64 [ceil(H/s), ceil(W/s), 3]"""
    h, w, _ = rgb.shape
    oh, ow = -(-h // s), -(-w // s)
    pad = np.zeros((oh * s, ow * s, 3))
    cnt = np.zeros((oh * s, ow * s, 1))
    pad[:h, :w] = rgb
    cnt[:h, :w] = 1
    ps = pad.reshape(oh, s, ow, s, 3).sum(axis=(1, 3))
    cs = cnt.reshape(oh, s, ow, s, 1).sum(axis=(1, 3))
    return ps / cs

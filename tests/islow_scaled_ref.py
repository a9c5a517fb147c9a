"""Numpy restatement of MJX_IDCT_ISLOW at scale_denom 2, 4 and 8 (include/mjx.h): libjpeg's reduced integer inverse DCTs, in int32 with
wrap-around.

The contract, with m = 8 / s: the picture is ceil(W / s) x ceil(H / s).  Component c takes the transform of size N_c -- from m, doubled
while N_c < 8 and the doubled size still divides the MCU's scaled extent in both directions (jdmaster.c) --, its plane holds
ceil(W h_c N_c / (8 hmax)) x ceil(H v_c N_c / (8 vmax)) samples and is upsampled by (hmax m / (h_c N_c), vmax m / (v_c N_c)).  Per block
d = coef x raw DQT entry; N = 8 is islow_ref's transform, N = 4 and N = 2 are jidctred.c's R4 and R2 (below), N = 1 is (d00 + 4) >> 3;
the sample is clamp(x + 128, 0, 255).  Behind it islow_ref's upsampling on the scaled planes and ratios (the narrow-plane rule on the
scaled width) -- but at s = 8 every component is replicated: jdsample.c has no fancy upsampling when min_DCT_scaled_size is 1 -- and
jdcolor.c's colour step.  Built on islow_ref and libjpeg_ref; nothing here is shared with the library.
"""
import numpy as np

import islow_ref
import libjpeg_ref
import scaled_ref

FIX = islow_ref.FIX


def D(x, n):
    return (x + np.int32(1 << (n - 1))) >> np.int32(n)


def R4(d, n):
    """d: int32 [..., 8] -> int32 [..., 4]; d[..., 4] is never read"""
    d = np.asarray(d, np.int32)
    d0, d1, d2, d3, _, d5, d6, d7 = (d[..., k] for k in range(8))
    with np.errstate(over="ignore"):
        t0 = d0 * np.int32(1 << 14)
        t2 = d2 * FIX(1.847759065) - d6 * FIX(0.765366865)
        t10, t12 = t0 + t2, t0 - t2
        z1, z2, z3, z4 = d7, d5, d3, d1
        a = -z1 * FIX(0.211164243) + z2 * FIX(1.451774981) - z3 * FIX(2.172734803) + z4 * FIX(1.061594337)
        b = -z1 * FIX(0.509795579) - z2 * FIX(0.601344887) + z3 * FIX(0.899976223) + z4 * FIX(2.562915447)
        return np.stack([D(t10 + b, n), D(t12 + a, n), D(t12 - a, n), D(t10 - b, n)], axis=-1).astype(np.int32)


def R2(d, n):
    """d: int32 [..., 8] -> int32 [..., 2]; reads d0, d1, d3, d5, d7"""
    d = np.asarray(d, np.int32)
    with np.errstate(over="ignore"):
        t10 = d[..., 0] * np.int32(1 << 15)
        t0 = -d[..., 7] * FIX(0.720959822) + d[..., 5] * FIX(0.850430095) - d[..., 3] * FIX(1.272758580) + d[..., 1] * FIX(3.624509785)
        return np.stack([D(t10 + t0, n), D(t10 - t0, n)], axis=-1).astype(np.int32)


def idct_blocks(coef, q, n):
    """coef: int [B, 8, 8] natural order ([v][u]), q: int [8, 8] or [B, 8, 8], n: 8, 4, 2 or 1 -> uint8 [B, n, n] samples"""
    if n == 8:
        return islow_ref.idct_blocks(coef, q)
    with np.errstate(over="ignore"):
        d = np.asarray(coef, np.int64).astype(np.int32) * np.asarray(q, np.int64).astype(np.int32)
        if n == 1:
            x = D(d[:, :1, :1], 3)
        else:
            R, n1, n2 = (R4, 12, 19) if n == 4 else (R2, 13, 20)
            p1 = R(np.swapaxes(d, 1, 2), n1)                # [B, u, y]: the column pass runs over v
            x = R(np.swapaxes(p1, 1, 2), n2)                # [B, y, u] -> [B, y, x]
    return np.clip(x.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def transform_size(m, hc, vc, hmax, vmax):
    n = m
    while n < 8 and (hmax * m) % (hc * n * 2) == 0 and (vmax * m) % (vc * n * 2) == 0:
        n *= 2
    return n


def geometry(w, h, comps, s, same_size=False):
    """comps: [(h_c, v_c)] -> [(N_c, plane width, plane height, rh, rv)]; same_size: the planted error N_c = m for every component"""
    m = 8 // s
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    out = []
    for hc, vc in comps:
        n = m if same_size else transform_size(m, hc, vc, hmax, vmax)
        out.append((n, -(-w * hc * n // (hmax * 8)), -(-h * vc * n // (vmax * 8)), hmax * m // (hc * n), vmax * m // (vc * n)))
    return out


def component_planes(data, s, dec=None, same_size=False):
    """-> (out_w, out_h, [uint8 plane of the component's scaled size], [(rh, rv)])"""
    w, h, comps, qt = scaled_ref.jpeg_tables(data)
    if dec is None:
        dec = scaled_ref.orc.decode(data, layout=scaled_ref.orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)
    if len(comps) == 1:
        comps = [(1, 1, comps[0][2])]
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    geo = geometry(w, h, [(c[0], c[1]) for c in comps], s, same_size)
    planes, ratios = [], []
    for c, (hc, vc, tq) in enumerate(comps):
        n, pw, ph, rh, rv = geo[c]
        co = np.asarray(dec.coefs[c], np.int16)
        assert co.shape[0] == mcux * mcuy * hc * vc, (co.shape, mcux, mcuy, hc, vc)
        nat = np.zeros(co.shape, np.int32)
        nat[:, scaled_ref.ZIGZAG] = co
        qn = np.zeros(64, np.int32)
        qn[scaled_ref.ZIGZAG] = np.asarray(qt[tq], np.int32)
        sm = idct_blocks(nat.reshape(-1, 8, 8), qn.reshape(8, 8), n)
        sm = sm.reshape(mcuy, mcux, vc, hc, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * vc * n, mcux * hc * n)
        planes.append(sm[:ph, :pw])
        ratios.append((rh, rv))
    return -(-w // s), -(-h // s), planes, ratios


def upsample(p, rh, rv, s, fancy_at_8=False):
    if s == 8 and not fancy_at_8:
        return np.repeat(np.repeat(np.asarray(p, np.int32), rv, axis=0), rh, axis=1)
    return islow_ref.upsample(p, rh, rv)


def pixels_from_planes(planes, ratios, ow, oh, s, fancy_at_8=False):
    up = [upsample(p, rh, rv, s, fancy_at_8)[:oh, :ow] for p, (rh, rv) in zip(planes, ratios)]
    assert all(u.shape == (oh, ow) for u in up), ([u.shape for u in up], ow, oh)
    if len(up) == 1:
        return np.repeat(up[0][:, :, None], 3, axis=2).astype(np.uint8)
    y, cb, cr = up
    return np.stack([libjpeg_ref.channel_r(y, cr), libjpeg_ref.channel_g(y, cb, cr), libjpeg_ref.channel_b(y, cb)], axis=2).astype(np.uint8)


def pixels(data, s, dec=None, fancy_at_8=False, same_size=False):
    """-> uint8 [ceil(H / s), ceil(W / s), 3]: the contract's picture of `data` at scale s (1: islow_ref's)"""
    if s == 1:
        return islow_ref.pixels(data, dec)
    ow, oh, pl, ratios = component_planes(data, s, dec, same_size)
    return pixels_from_planes(pl, ratios, ow, oh, s, fancy_at_8)


def luma(data, s, dec=None):
    """-> uint8 [ceil(H / s), ceil(W / s)]: component 0's plane, upsampled by its own scaled ratios"""
    if s == 1:
        return islow_ref.luma(data, dec)
    ow, oh, pl, ratios = component_planes(data, s, dec)
    return upsample(pl[0], *ratios[0], s)[:oh, :ow].astype(np.uint8)


def pillow(data, s):
    """Pillow's decode at scale 1 / s: what Image.draft() sets, set directly (draft's own size rule picks a coarser scale for ceil sizes)"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if s > 1:
        w, h = im.size
        size = (-(-w // s), -(-h // s))
        im.decoderconfig = (s, 0)
        im._size = size
        im.tile = [im.tile[0]._replace(extents=(0, 0) + size)]
    return np.asarray(im.convert("RGB"))

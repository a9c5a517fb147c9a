"""Numpy restatement of MJX_IDCT_ISLOW (include/mjx.h, MJX_OPTS_IDCT): libjpeg's integer slow inverse DCT, in int32 with wrap-around.

The contract, per 8 x 8 block: d = coef x raw DQT entry; pass 1 runs P with n = 11 on every column, pass 2 the same P with n = 18 on
every row of pass 1's output; the sample is clamp(x + 128, 0, 255).  Behind it the picture is libjpeg_ref's -- fancy upsampling and
jdcolor.c's colour step, no rounding: the samples are integers -- with wide_ref's rule for a ratio of 4 and the narrow-plane rule: a
component whose plane has at most two columns and whose ratios are (2, 1) or (2, 2) is replicated (jdsample.c's downsampled_width > 2).
Nothing here is shared with the library: the tests compare the two, and both with Pillow.
"""
import numpy as np

import libjpeg_ref
import scaled_ref


def FIX(x):
    return np.int32(int(x * 8192 + 0.5))


def P(d, n):
    """d: int32 [..., 8], the eight inputs along the last axis -> int32 [..., 8]; every product and sum wraps modulo 2^32"""
    d = np.asarray(d, np.int32)
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    with np.errstate(over="ignore"):
        z1 = (d2 + d6) * FIX(0.541196100)
        t2 = z1 - d6 * FIX(1.847759065)
        t3 = z1 + d2 * FIX(0.765366865)
        t0 = (d0 + d4) * np.int32(8192)
        t1 = (d0 - d4) * np.int32(8192)
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a, b, c, e = d7, d5, d3, d1
        z1, z2, z3, z4 = a + e, b + c, a + c, b + e
        z5 = (z3 + z4) * FIX(1.175875602)
        a = a * FIX(0.298631336)
        b = b * FIX(2.053119869)
        c = c * FIX(3.072711026)
        e = e * FIX(1.501321110)
        z1 = z1 * -FIX(0.899976223)
        z2 = z2 * -FIX(2.562915447)
        z3 = z3 * -FIX(1.961570560) + z5
        z4 = z4 * -FIX(0.390180644) + z5
        a = a + (z1 + z3)
        b = b + (z2 + z4)
        c = c + (z2 + z3)
        e = e + (z1 + z4)
        o = [t10 + e, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - e]
        half = np.int32(1 << (n - 1))
        return np.stack([(v + half) >> np.int32(n) for v in o], axis=-1).astype(np.int32)


def idct_blocks(coef, q):
    """coef: int [N, 8, 8] natural order ([v][u]), q: int [8, 8] or [N, 8, 8] -> uint8 [N, 8, 8] samples"""
    with np.errstate(over="ignore"):
        d = np.asarray(coef, np.int64).astype(np.int32) * np.asarray(q, np.int64).astype(np.int32)
    p1 = P(np.swapaxes(d, 1, 2), 11)                # [N, u, v]: the column pass runs over v
    p2 = P(np.swapaxes(p1, 1, 2), 18)               # [N, v, u]: the row pass runs over u
    return np.clip(p2.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def component_planes(data, dec=None):
    """-> (w, h, [uint8 plane of the component's true size], [(rh, rv)]) from the oracle's coefficients, or from `dec` (coefs per
    component in decode order, zig-zag: an oracle decode, or wide_ref.dec_of of a writer's blocks)"""
    w, h, comps, qt = scaled_ref.jpeg_tables(data)
    if dec is None:
        dec = scaled_ref.orc.decode(data, layout=scaled_ref.orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)
    if len(comps) == 1:
        comps = [(1, 1, comps[0][2])]
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    planes, ratios = [], []
    for c, (hc, vc, tq) in enumerate(comps):
        co = np.asarray(dec.coefs[c], np.int16)
        assert co.shape[0] == mcux * mcuy * hc * vc, (co.shape, mcux, mcuy, hc, vc)
        nat = np.zeros(co.shape, np.int32)
        nat[:, scaled_ref.ZIGZAG] = co
        qn = np.zeros(64, np.int32)
        qn[scaled_ref.ZIGZAG] = np.asarray(qt[tq], np.int32)
        s = idct_blocks(nat.reshape(-1, 8, 8), qn.reshape(8, 8))
        s = s.reshape(mcuy, mcux, vc, hc, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * vc * 8, mcux * hc * 8)
        planes.append(s[:-(-h * vc // vmax), :-(-w * hc // hmax)])
        ratios.append((hmax // hc, vmax // vc))
    return w, h, planes, ratios


def upsample(s, rh, rv, narrow=True):
    """uint8 / int plane [ch, cw] -> int32 [ch rv, cw rh]: replication where a ratio is 4 and, narrow=True, for a plane of at most two
    columns with ratios (2, 1) or (2, 2); libjpeg_ref's filters elsewhere"""
    s = np.asarray(s, np.int32)
    if rh == 4 or rv == 4 or (narrow and s.shape[1] <= 2 and rh == 2 and rv in (1, 2)):
        return np.repeat(np.repeat(s, rv, axis=0), rh, axis=1)
    return libjpeg_ref.upsample(s, rh, rv)


def pixels_from_planes(planes, ratios, w, h, narrow=True):
    up = [upsample(p, rh, rv, narrow)[:h, :w] for p, (rh, rv) in zip(planes, ratios)]
    assert all(u.shape == (h, w) for u in up), [u.shape for u in up]
    if len(up) == 1:
        return np.repeat(up[0][:, :, None], 3, axis=2).astype(np.uint8)
    y, cb, cr = up
    return np.stack([libjpeg_ref.channel_r(y, cr), libjpeg_ref.channel_g(y, cb, cr), libjpeg_ref.channel_b(y, cb)], axis=2).astype(np.uint8)


def pixels(data, dec=None, narrow=True):
    """-> uint8 [H, W, 3]: the contract's picture of `data`"""
    w, h, pl, ratios = component_planes(data, dec)
    return pixels_from_planes(pl, ratios, w, h, narrow)


def luma(data, dec=None):
    """-> uint8 [H, W]: component 0's plane, upsampled by its own ratios (the luminance output)"""
    w, h, pl, ratios = component_planes(data, dec)
    return upsample(pl[0], *ratios[0])[:h, :w].astype(np.uint8)

"""Numpy restatement of MJX_PIXELS_LIBJPEG (include/mjx.h, mjx_opts.pixels): what libjpeg's pipeline does behind its inverse DCT.

It works on scaled_ref.planes(data, 1): float64 samples from the oracle's coefficients (128 is on luminance there; it is added to
chroma here).  Per component: the plane of ceil(W h / hmax) x ceil(H v / vmax) samples, each rounded s = clamp(floor(f + 0.5), 0,
255); fancy upsampling by (hmax / h, vmax / v) in integers with edge replication (jdsample.c h2v1 / h2v2, and h1v2 as the same rule
down the columns); jdcolor.c's integer colour step.  Nothing here is shared with the library: the tests compare the two.
"""
import numpy as np

import scaled_ref


def round_u8(x):
    """clamp(floor(x + 0.5), 0, 255) -> int32"""
    return np.clip(np.floor(np.asarray(x, np.float64) + 0.5), 0, 255).astype(np.int32)


def _prev(s, axis):
    """s[i - 1] along axis, index clamped"""
    idx = np.maximum(np.arange(s.shape[axis]) - 1, 0)
    return np.take(s, idx, axis=axis)


def _next(s, axis):
    idx = np.minimum(np.arange(s.shape[axis]) + 1, s.shape[axis] - 1)
    return np.take(s, idx, axis=axis)


def upsample(s, rh, rv):
    """int plane [ch, cw] -> [ch * rv, cw * rh]: the contract's four cases"""
    s = np.asarray(s, np.int32)
    ch, cw = s.shape
    if rh == 1 and rv == 1:
        return s.copy()
    if rv == 1:
        out = np.empty((ch, 2 * cw), np.int32)
        out[:, 0::2] = (3 * s + _prev(s, 1) + 1) >> 2
        out[:, 1::2] = (3 * s + _next(s, 1) + 2) >> 2
        return out
    if rh == 1:
        out = np.empty((2 * ch, cw), np.int32)
        out[0::2] = (3 * s + _prev(s, 0) + 1) >> 2
        out[1::2] = (3 * s + _next(s, 0) + 2) >> 2
        return out
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for odd, far in ((0, _prev(s, 0)), (1, _next(s, 0))):
        t = 3 * s + far
        out[odd::2, 0::2] = (3 * t + _prev(t, 1) + 8) >> 4
        out[odd::2, 1::2] = (3 * t + _next(t, 1) + 7) >> 4
    return out


def fix(x):
    return int(x * 65536 + 0.5)


def channel_r(y, cr):
    return np.clip(y + ((fix(1.40200) * (cr - 128) + 32768) >> 16), 0, 255)


def channel_b(y, cb):
    return np.clip(y + ((fix(1.77200) * (cb - 128) + 32768) >> 16), 0, 255)


def channel_g(y, cb, cr):
    return np.clip(y + ((-fix(0.34414) * (cb - 128) + 32768 - fix(0.71414) * (cr - 128)) >> 16), 0, 255)


def pixels_from_planes(planes, ratios, w, h):
    """rounded int planes [ch, cw] per component and their (rh, rv) -> uint8 [h, w, 3]"""
    up = [upsample(p, rh, rv)[:h, :w] for p, (rh, rv) in zip(planes, ratios)]
    assert all(u.shape == (h, w) for u in up), [u.shape for u in up]
    if len(up) == 1:
        return np.repeat(up[0][:, :, None], 3, axis=2).astype(np.uint8)
    y, cb, cr = up
    return np.stack([channel_r(y, cr), channel_g(y, cb, cr), channel_b(y, cb)], axis=2).astype(np.uint8)


def component_planes(data, dec=None, magnitude=False):
    """-> (w, h, [float64 plane of the component's true size, 128 on every component], [(rh, rv)]); magnitude=True: S_c of
    scaled_ref.planes instead of the samples (as it stands there: 128 on luminance only)"""
    w, h, comps, pl, hmax, vmax = scaled_ref.planes(data, 1, dec, magnitude)
    out, ratios = [], []
    for c, ((hc, vc, _), p) in enumerate(zip(comps, pl)):
        cw, ch = -(-w * hc // hmax), -(-h * vc // vmax)
        out.append(p[:ch, :cw] + (128.0 if c > 0 and not magnitude else 0.0))
        ratios.append((hmax // hc, vmax // vc))
    return w, h, out, ratios


def libjpeg_pixels(data, dec=None):
    """-> uint8 [H, W, 3]: the contract's picture of `data`, from float64 samples"""
    w, h, pl, ratios = component_planes(data, dec)
    return pixels_from_planes([round_u8(p) for p in pl], ratios, w, h)


def interval(data, K=64, dec=None):
    """-> (lo, hi) uint8 [H, W, 3]: the bytes a float32 decoder may give.  delta = K 2^-24 S_c per sample; every step behind the
    rounding is monotone in every sample -- R and B rise with Y and their chroma, G rises with Y and falls with both chroma
    components -- so lo is the pipeline on round(w - delta) and hi on round(w + delta), the chroma bounds swapped for G."""
    w, h, pl, ratios = component_planes(data, dec)
    _, _, mag, _ = component_planes(data, dec, magnitude=True)
    lo = [upsample(round_u8(p - K * 2.0 ** -24 * m), rh, rv)[:h, :w] for p, m, (rh, rv) in zip(pl, mag, ratios)]
    hi = [upsample(round_u8(p + K * 2.0 ** -24 * m), rh, rv)[:h, :w] for p, m, (rh, rv) in zip(pl, mag, ratios)]
    if len(pl) == 1:
        return (np.repeat(lo[0][:, :, None], 3, axis=2).astype(np.uint8), np.repeat(hi[0][:, :, None], 3, axis=2).astype(np.uint8))
    out_lo = np.stack([channel_r(lo[0], lo[2]), channel_g(lo[0], hi[1], hi[2]), channel_b(lo[0], lo[1])], axis=2).astype(np.uint8)
    out_hi = np.stack([channel_r(hi[0], hi[2]), channel_g(hi[0], lo[1], lo[2]), channel_b(hi[0], hi[1])], axis=2).astype(np.uint8)
    return out_lo, out_hi

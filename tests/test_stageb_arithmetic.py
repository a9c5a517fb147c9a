"""Stage B's arithmetic -- dequantise, inverse DCT, colour, pack -- against float64 on chosen coefficients.

The parity tiers compare pictures of natural or smooth content within +-1.  A single AC coefficient moves a sample by at most
F q / 4, so on such content a 2 % error in one multiplier, one transform constant or one corner entry stays below one level; and
they keep every sample inside 0..255, so neither side of the saturating store is seen.  Here the files are written from chosen
coefficient blocks (jpegwriter.jpeg_from_blocks), the reference is the float64 picture of scaled_ref, and a device byte must lie in
[lo, hi] of scaled_ref.rgb_interval: the bytes float64 gives when moved by K half-ulps (2^-24) of the pixel's magnitude
m = S_Y + 2 S_Cb + 2 S_Cr, S_c = sum |coef q| / 8 (+ 128 on Y).  lo == hi nearly everywhere: equality with float64.

Coefficient classes (variants in VARIANTS):
  1 basis    one non-zero coefficient per block: every zig-zag position, both signs, amplitude 1 / the largest in range / 1023,
             quantisers 1, 255, 65535 (16-bit DQT), the three components on different tables
  2 pairs    two coefficients per block: (k, 63 - k) and (row-only, column-only) positions, tables that differ at every position
  3 dense    all 64 coefficients of every block from [-256, 255], [-5, 5], [-300, 300] and the negated draws, q = 1
  4 exact    DC-only luminance, chroma zero, levels -40 .. 300: every step exact in float32, the bytes must EQUAL clamp(level)
  5 sat      sparse +-1023 at q = 255 and 65535, dense +-1023 at q = 65535, mid luminance under a grid of far chroma
  6 over     AC of sizes 11 .. 15 (to +-32767) and DC to +-2047 from the all-symbols AC table

Which kernel instantiation each GPU test reaches, and why (planner rules: mjx_api.hip launch_idct_color's callers, planar_ok):
  test                                  input                                    instantiation
  test_standard[420-quad-sparse]        4:2:0, one scan, scan <= 1400 B / tile   k_idct_color<1, 8, 1>  (interior tiles by exchange,
                                        1035 x 490: 65 x 31 MCUs, tiles of 32    right / bottom edge form, row-break tiles)
  test_standard[420-quad-dense]         classes 3, 5: scan > 1400 B / tile       k_idct_color<1, 16, 1>
  test_standard[420-linear-sparse]      MJX_STREAM_LINEAR=1                      k_idct_color<1, kPrefetch, 0>
  test_standard[420-linear-dense]       MJX_STREAM_LINEAR=1, > 1400 B / tile     k_idct_color<1, kPrefetchDense, 0>
  test_standard[444|422|440|gray|       any other layout, 333 x 217              k_idct_color<0, 8, 1> (quad), <0, kPrefetch, 0> (linear).
                Y22_Cb21_Cr12-...]      The dense / sparse choice exists for MODE 1 only: for these layouts `density` merely splits
                                        the classes over two batches, and the density assertion is made for 4:2:0 alone.
  test_multiscan_twins                  two scripts of every variant, keep_coefs k_idct_color<1 | 0, 8, 2> (planar reads; the tile rule
                                        off, a tile touches <= 2 MCU rows        of planar_ok is asserted); with keep_coefs on, the
                                        (1035 x 490 4:2:0, 1000 x 40 4:4:4)      gathered linear stream: <1 | 0, kPrefetch*, 0>
  test_scaled[*-2|4]                    scale 2, 4                               k_idct_color<3 | 4, kPrefetch | 8, 0 | 1>
  test_scaled[*-8]                      scale 8                                  k_dc_color
  test_ref_compat                       REF_COMPAT, 4:4:4 320 x 216 and grey     k_idct_color<2, ...> + k_ref_color (pack_u8)
  test_roi_and_formats[*-1]             unaligned rectangles / an Output         k_idct_color, forms 0|1 of kSinkCropped, kSinkOut
  test_roi_and_formats[*-2|4|8]                                                  forms 3|4 of the same sinks, k_dc_color_roi,
                                                                                 k_dc_color_out
Every test asserts T0 (b.coefs(i) == the blocks written) wherever the batch keeps coefficients, so a pixel failure is stage B's.
"""
import functools
import math
import os
import types

import numpy as np
import pytest

import jpegwriter as jw
import oracle_binding as orc
import scaled_ref

# K of rgb_interval: 4 x the largest K any sample of the two float32 CPU computations needs, rounded up to a power of two
# (test_K_is_measured_and_the_ambiguous_share_is_small).  Measured: K_a = 9.13 (the oracle at scale 1; on basis_q65535, 4:2:0),
# K_b = 1.92 (the numpy float32 restatement of stage B at scales 1, 2, 4, 8; on sat_sparse_q255).  4 x 9.13 = 36.5 -> 64.  The margin
# of 4 covers the kernel's packed pairing and fused multiply-adds, which the restatement does not reproduce.
K = 64
AMBIGUOUS_CAP = 0.02

ZZ = np.array(jw.ZIGZAG)
F32, F64 = np.float32, np.float64
LAYOUTS = {"420": [(2, 2), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)],
           "gray": [(1, 1)], "Y22_Cb21_Cr12": [(2, 2), (2, 1), (1, 2)]}
CLASSES = {1: ["basis_q1", "basis_q255", "basis_q65535"], 2: ["pairs"],
           3: ["dense_256", "dense_256n", "dense_5", "dense_5n", "dense_300", "dense_300n"], 4: ["exact_q8", "exact_q2"],
           5: ["sat_sparse_q255", "sat_sparse_q65535", "sat_dense_q65535", "sat_chroma"], 6: ["over_q1", "over_q3"]}
VARIANTS = [v for c in sorted(CLASSES) for v in CLASSES[c]]
CLASS_OF = {v: c for c, vs in CLASSES.items() for v in vs}
CPU_SHAPE = ("420", 381, 250)           # 24 x 16 MCUs, the last column and row clipped
CPU_OTHER = [("444", 189, 131), ("gray", 187, 133), ("Y22_Cb21_Cr12", 317, 250)]


# ---- the coefficient classes ---------------------------------------------------------------------------------------------------------
def _cc(nat):
    """C(u) C(v) / 4 of a natural position (/ 8 at DC): the largest sample a unit dequantised coefficient there gives"""
    u, v = nat & 7, nat >> 3
    return (math.sqrt(0.5) if u == 0 else 1.0) * (math.sqrt(0.5) if v == 0 else 1.0) / 4.0


def _limits(ncomp):
    """peak excursion allowed per component so that R, G and B stay inside 0..255 around mid-grey (a fourth component, K, is a byte
    of its own: half the range of a single one, so that two excursions in one block still fit)"""
    return [120.0] if ncomp == 1 else [60.0, 30.0 / 1.772, 30.0 / 1.402, 60.0][:ncomp]


def _tables_q(Q, ncomp):
    """Q everywhere on luminance; chroma: Q on every other position and a neighbour of Q on the rest, the other way round on Cr; a
    fourth component: a factor of two or more away from Q at every position (3 for Q = 1, else Q // 2 -- odd for the Q in use,
    1, 255 and 65535)"""
    alt = 2 if Q == 1 else Q - 1
    k = np.arange(64)
    return [np.full(64, Q), np.where(k % 2 == 0, Q, alt), np.where(k % 2 == 1, Q, alt), np.full(64, 3 if Q == 1 else Q // 2)][:ncomp]


def _in_range_amp(limit, q, k):
    a = max(1, int(limit / (q * _cc(int(ZZ[k])))))
    if (a * q) % 8 == 0 and a > 1:
        a -= 1              # (F q / 8 whole: a flat block, or a corner of cos(pi/4) terms alone, lands on exact integers -- class 4's business)
    return min(a, 1023)


def _gen_basis(Q, per_mcu, mcus, rng):
    ncomp = len(per_mcu)
    qts, lim, out = _tables_q(Q, ncomp), _limits(ncomp), []
    for c, kc in enumerate(per_mcu):
        m, j = np.arange(mcus)[:, None], np.arange(kc)[None, :]
        kind = np.broadcast_to(m % 3, (mcus, kc))
        idx = ((m // 3) * kc + j + 37 * c) % 128
        pos, sign = idx // 2, 1 - 2 * (idx % 2)
        amp = np.array([[1] * 64, [_in_range_amp(lim[c], int(qts[c][k]), k) for k in range(64)], [1023] * 64])
        blk = np.zeros((mcus, kc, 64), np.int64)
        mm, jj = np.broadcast_to(m, (mcus, kc)), np.broadcast_to(j, (mcus, kc))
        blk[mm, jj, pos] = sign * amp[kind, pos]
        out.append(blk.reshape(-1, 64))
    return out, qts, Q > 255, "annex_k"


def _pair_configs():
    cfg = [(k, 63 - k) for k in range(32)]
    inv = np.argsort(ZZ)                                # natural -> zig-zag
    cfg += [(int(inv[u]), int(inv[8 * v])) for u in range(1, 8) for v in range(1, 8)]
    return [(a, b, 1, s) for a, b in cfg for s in (1, -1)]


def _gen_pairs(per_mcu, mcus, rng):
    ncomp = len(per_mcu)
    qts, lim, cfg, out = [2 * rng.integers(0, 16, 64) + 1 for _ in range(ncomp)], _limits(ncomp), _pair_configs(), []
    for c, kc in enumerate(per_mcu):
        blk = np.zeros((mcus * kc, 64), np.int64)
        for n in range(mcus * kc):
            a, b, sa, sb = cfg[(n + 37 * c) % len(cfg)]
            blk[n, a] = sa * _in_range_amp(lim[c] / 2, int(qts[c][a]), a)
            blk[n, b] = sb * _in_range_amp(lim[c] / 2, int(qts[c][b]), b)
        out.append(blk)
    return out, qts, False, "annex_k"


def _gen_dense(lo, hi, neg, per_mcu, mcus, rng):
    out = [(-1 if neg else 1) * rng.integers(lo, hi + 1, (mcus * kc, 64)) for kc in per_mcu]
    return out, [np.ones(64, np.int64)] * len(per_mcu), False, "annex_k"


EXACT_LEVELS = np.arange(-40, 301)


def _exact_level(n):
    return EXACT_LEVELS[(7 * n) % len(EXACT_LEVELS)]        # (7 and 341 are coprime: every level; neighbours differ by 7)


def _gen_exact(q, per_mcu, mcus, rng):
    out = [np.zeros((mcus * kc, 64), np.int64) for kc in per_mcu]
    out[0][:, 0] = (_exact_level(np.arange(mcus * per_mcu[0])) - 128) * 8 // q
    return out, [np.full(64, q), np.full(64, 3), np.full(64, 5)][:len(per_mcu)], False, "annex_k"


def _gen_sat_sparse(Q, per_mcu, mcus, rng):
    out = []
    for kc in per_mcu:
        blk = np.where(rng.random((mcus * kc, 64)) < 0.06, 1023, 0) * rng.choice([-1, 1], (mcus * kc, 64))
        blk[:, 0] = np.where(blk[:, 0] == 0, rng.choice([-1, 1], mcus * kc), blk[:, 0])      # (no block is all zero)
        out.append(blk)
    return out, _tables_q(Q, len(per_mcu)), Q > 255, "annex_k"


def _gen_sat_dense(Q, per_mcu, mcus, rng):
    out = [1023 * rng.choice([-1, 1], (mcus * kc, 64)) for kc in per_mcu]
    return out, _tables_q(Q, len(per_mcu)), Q > 255, "annex_k"


def _gen_sat_chroma(per_mcu, mcus, rng):
    """luminance around mid-grey (levels 14 .. 242); Cb and Cr on a 17 x 17 grid of DC levels from far below to far above (+-511, +-639), so that R, G
    and B leave 0..255 one by one and on both sides.  One component: its DC takes the grid."""
    grid = np.linspace(-1023, 1023, 17).astype(np.int64)
    out = []
    for c, kc in enumerate(per_mcu):
        n = np.arange(mcus * kc)
        blk = np.where(rng.random((mcus * kc, 64)) < 0.05, rng.integers(-6, 7, (mcus * kc, 64)), 0)
        if len(per_mcu) == 1:
            blk[:, 0] = grid[n % 17]
        elif c == 0:
            blk[:, 0] = rng.integers(-130, 131, mcus * kc)
        else:
            blk[:, 0] = grid[(n // (1 if c == 1 else 17)) % 17]
        out.append(blk)
    qts = [np.full(64, 4)] if len(per_mcu) == 1 else [np.full(64, 7), np.full(64, 4), np.full(64, 5)]
    return out, qts, False, "annex_k"


def _gen_over(qs, per_mcu, mcus, rng):
    out = []
    for kc in per_mcu:
        n = mcus * kc
        blk = np.zeros((n, 64), np.int64)
        big = np.nonzero(rng.random(n) < 0.25)[0]
        for _ in range(2):
            size = rng.integers(11, 16, len(big))
            mag = rng.integers(1 << (size - 1), 1 << size)                       # a value of exactly that size
            blk[big, rng.integers(1, 64, len(big))] = mag * rng.choice([-1, 1], len(big))
        top = 2047 if qs[0] == 1 else 1023          # (+-1023: the differences fit size 11 in any block order -- the multi-scan twins)
        dc, prev = np.zeros(n, np.int64), 0
        for i, d in enumerate(rng.integers(-top, top + 1, n)):                   # differences of up to size 11, sums inside +-2047
            prev = prev + int(d) if abs(prev + int(d)) <= top else prev - int(d)
            dc[i] = prev
        blk[:, 0] = dc
        out.append(blk)
    return out, [np.full(64, q) for q in qs][:len(per_mcu)], False, "full"


def _generate(variant, per_mcu, mcus):
    rng = np.random.default_rng([VARIANTS.index(variant), mcus, len(per_mcu)])
    kind, _, arg = variant.partition("_")
    if kind == "basis":
        return _gen_basis(int(arg[1:]), per_mcu, mcus, rng)
    if kind == "pairs":
        return _gen_pairs(per_mcu, mcus, rng)
    if kind == "dense":
        lo, hi = {"256": (-256, 255), "5": (-5, 5), "300": (-300, 300)}[arg.rstrip("n")]
        return _gen_dense(lo, hi, arg.endswith("n"), per_mcu, mcus, rng)
    if kind == "exact":
        return _gen_exact(int(arg[1:]), per_mcu, mcus, rng)
    if variant.startswith("sat_sparse"):
        return _gen_sat_sparse(int(variant.rsplit("q", 1)[1]), per_mcu, mcus, rng)
    if variant.startswith("sat_dense"):
        return _gen_sat_dense(int(variant.rsplit("q", 1)[1]), per_mcu, mcus, rng)
    if variant == "sat_chroma":
        return _gen_sat_chroma(per_mcu, mcus, rng)
    return _gen_over({"q1": (1, 1, 1, 3), "q3": (3, 2, 1, 5)}[arg], per_mcu, mcus, rng)


def _huffman(kind):
    if kind == "annex_k":
        return jw._annex_k_tables()
    return {(0, 0): jw.small_dc_table(11), (1, 0): jw.full_ac_table()}


@functools.lru_cache(maxsize=None)
def picture(variant, lname, w, h):
    """One class picture: .data (the file), .blocks (int16, what b.coefs must return), .per_comp, .qts, .dec (for scaled_ref)"""
    hv = LAYOUTS[lname]
    mcu_hv = [(1, 1)] if len(hv) == 1 else hv
    hmax, vmax = max(x for x, _ in mcu_hv), max(y for _, y in mcu_hv)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    per_mcu = [x * y for x, y in mcu_hv]
    per_comp, qts, qt16, huff = _generate(variant, per_mcu, mcux * mcuy)
    blocks = np.concatenate([p.reshape(mcux * mcuy, k, 64) for p, k in zip(per_comp, per_mcu)], axis=1).reshape(-1, 64)
    p = types.SimpleNamespace(variant=variant, cls=CLASS_OF[variant], layout=lname, hv=hv, w=w, h=h, mcux=mcux, mcuy=mcuy,
                              hmax=hmax, vmax=vmax, per_mcu=per_mcu, per_comp=per_comp, qts=[np.asarray(q, np.int64) for q in qts], qt16=qt16)
    p.data = jw.jpeg_from_blocks(blocks, hv, mcux, mcuy, qts, _huffman(huff), qt16=qt16, width=w, height=h)
    p.blocks = blocks.astype(np.int16)
    assert np.array_equal(p.blocks, blocks)
    p.dec = types.SimpleNamespace(coefs=per_comp, mcus=mcux * mcuy)
    return p


@functools.lru_cache(maxsize=None)
def interval(variant, lname, w, h, scale):
    """(lo, hi) of the picture at 1/scale.  Class 4: no interval -- lo = hi = the clamped exact level."""
    p = picture(variant, lname, w, h)
    if p.cls == 4:
        want = scaled_ref.to_u8(scaled_ref.rgb_f64(p.data, scale, p.dec))
        return want, want
    return scaled_ref.rgb_interval(p.data, scale, K, p.dec)


def needed_k(got, w, m):
    """the smallest K of rgb_interval under which every byte of `got` lies in its interval -> (K, index of the worst sample)"""
    got = got.astype(F64)
    t = scaled_ref.trunc_u8(w).astype(F64)
    need = np.where(got > t, got - w, np.where(got < t, w - (got + 1.0), 0.0)) / (2.0 ** -24 * m[:, :, None])
    need = np.where((got < t) & (need <= 0), 1e-9, need)        # (w - delta must fall strictly below got + 1)
    at = np.unravel_index(np.argmax(need), need.shape)
    return float(need[at]), at


def check(p, scale, got, tag):
    """every byte of the device picture `got` inside the picture's interval; on failure the worst sample is named"""
    lo, hi = interval(p.variant, p.layout, p.w, p.h, scale)
    assert got.shape == lo.shape, (tag, p.variant, got.shape, lo.shape)
    report = os.environ.get("MJX_STAGEB_REPORT")
    bad = (got < lo) | (got > hi)
    if bad.any() or report:
        w, m = scaled_ref.rgb_f64(p.data, scale, p.dec), scaled_ref.magnitude(p.data, scale, p.dec)
        k, (y, x, ch) = needed_k(got, w, m)
        if report:
            print("STAGEB %s %s class %d %s scale %d: K_device %.3f (%.4f delta), ambiguous %.5f" %
                  (tag, p.layout, p.cls, p.variant, scale, k, k / K, float((lo != hi).mean())))
        s = scale
        blk = (y * s // (8 * p.vmax)) * p.mcux + x * s // (8 * p.hmax)
        assert not bad.any(), ("%s %s %s scale %d: %d of %d bytes outside their interval; worst at (y %d, x %d, channel %d) in MCU %d: "
                               "got %d, float64 %.6f, interval [%d, %d], magnitude %.4g, needs K = %.1f (K = %d)"
                               % (tag, p.layout, p.variant, scale, int(bad.sum()), bad.size, y, x, ch, blk, got[y, x, ch], w[y, x, ch],
                                  lo[y, x, ch], hi[y, x, ch], m[y, x], k, K))


# ---- the numpy float32 restatement of stage B (mjx_plan.cpp's multipliers, mjx_kernels.hip's transforms, colour and store) -------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64; one rounding (but for rare double roundings)"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def qmult_f32(qt_zz, scale, mut=None):
    """p.qmult / p.qmult_scaled (mjx_plan.cpp): computed in double, rounded to float; zig-zag order; 0 outside the corner"""
    n = 8 // scale
    aan = [1.0 if k == 0 else math.cos(k * 3.14159265358979323846 / 16.0) * math.sqrt(2.0) for k in range(8)]
    inv = np.argsort(ZZ)
    qm = np.zeros(64, F32)
    for k in range(64):
        nat = int(ZZ[k])
        v, u = nat >> 3, nat & 7
        q = float(qt_zz[k])
        if mut == "qmult_transposed" and (v, u) == (1, 2):
            q = float(qt_zz[inv[8 * u + v]])
        if scale == 1 or scale == 8:
            qm[k] = F32(q * aan[v] * aan[u] / 8.0)
        elif u < n and v < n:
            cu, cv = (math.sqrt(0.5) if u == 0 else 1.0), (math.sqrt(0.5) if v == 0 else 1.0)
            qm[k] = F32(q * cu * cv / 4.0)
        if (mut == "pos63_2pct" and k == 63) or (mut == "corner11_2pct" and scale in (2, 4) and (v, u) == (1, 1)):
            qm[k] = F32(qm[k] * F32(1.02))
    return qm


def idct8_f32(i, mut=None):
    """idct8 of mjx_kernels.hip on eight float32 arrays"""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    c1, c2, c3, c4 = F32(1.414213562), F32(1.847759065), F32(1.082392200), F32(-2.613125930)
    if mut == "const_1e-4":
        c2 = F32(1.847759065 * (1 + 1e-4))
    t10, t11 = i0 + i4, i0 - i4
    t13 = i2 + i6
    t12 = (i2 - i6) * c1 - t13
    e0, e3, e1, e2 = t10 + t13, t10 - t13, t11 + t12, t11 - t12
    z13, z10, z11, z12 = i5 + i3, i5 - i3, i1 + i7, i1 - i7
    o7 = z11 + z13
    u11 = (z11 - z13) * c1
    z5 = (z10 + z12) * c2
    u10 = c3 * z12 - z5
    u12 = c4 * z10 + z5
    o6 = u12 - o7
    o5 = u11 - o6
    o4 = u10 + o5
    return [e0 + o7, e1 + o6, e2 + o5, e3 - o4, e3 + o4, e2 - o5, e1 - o6, e0 - o7]


def _idct4_f32(g, mut=None):
    g0, g1, g2, g3 = g
    c4, c1, c3 = F32(0.707106781), F32(0.923879533 * (1 + 1e-4 if mut == "corner_const_1e-4" else 1)), F32(0.382683432)
    e0, e1 = _fma(g2, c4, g0), _fma(g2, -c4, g0)
    o0, o1 = _fma(g1, c1, g3 * c3), _fma(g1, c3, g3 * -c1)
    return [e0 + o0, e1 + o1, e1 - o1, e0 - o0]


def _idct2_f32(g, mut=None):
    c4 = F32(0.707106781 * (1 + 1e-4 if mut == "corner_const_1e-4" else 1))
    return [_fma(g[1], c4, g[0]), _fma(g[1], -c4, g[0])]


def stageb_f32(p, scale, mut=None):
    """The picture of `p` at 1/scale as stage B computes it, restated in numpy float32 -> uint8 [ceil(H/s), ceil(W/s), 3].
    mut: a planted error (test_plants)."""
    n = 8 // scale
    late128 = mut == "plus128_after_clamp"
    planes = []
    for c, (blk, kc) in enumerate(zip(p.per_comp, p.per_mcu)):
        hc, vc = ((1, 1) if len(p.hv) == 1 else p.hv[c])
        qm = qmult_f32(p.qts[c], scale, mut)
        nat = np.zeros((blk.shape[0], 64), F32)
        nat[:, ZZ] = blk.astype(F32) * qm[None, :]
        if c == 0 and not late128:
            nat[:, 0] = nat[:, 0] + F32(128.0)                   # the level shift rides on the DC coefficient
        f = nat.reshape(-1, 8, 8)
        if scale == 1:
            rows = idct8_f32([f[:, :, u] for u in range(8)], mut)            # rows: along u
            f = np.stack(rows, axis=2)
            cols = idct8_f32([f[:, v, :] for v in range(8)], mut)            # columns: along v
            s = np.stack(cols, axis=1)
        elif scale in (2, 4):
            one = _idct4_f32 if n == 4 else _idct2_f32
            f = f[:, :n, :n]
            f = np.stack(one([f[:, :, u] for u in range(n)], mut), axis=2)
            s = np.stack(one([f[:, v, :] for v in range(n)], mut), axis=1)
        else:
            s = f[:, :1, :1]
        planes.append(s.reshape(p.mcuy, p.mcux, vc, hc, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(p.mcuy * vc * n, p.mcux * hc * n))
    ow, oh = -(-p.w // scale), -(-p.h // scale)
    X, Y = np.arange(ow), np.arange(oh)
    smp = []
    for c, pl in enumerate(planes):
        hc, vc = ((1, 1) if len(p.hv) == 1 else p.hv[c])
        smp.append(pl[(Y * vc // p.vmax)[:, None], (X * hc // p.hmax)[None, :]])
    if len(smp) == 1:
        v = np.repeat(smp[0][:, :, None], 3, axis=2)
    else:
        y, cb, cr = smp
        c_red, c_green, c_blue = F32(0.299), F32(0.586 if mut == "green_0.586" else 0.587), F32(0.114)
        kr, kb = F32(2.0) - F32(2.0) * c_red, F32(2.0) - F32(2.0) * c_blue
        tr, tb = cr * kr, cb * kb
        tg = _fma(cb, -(c_blue * kb / c_green), cr * -(c_red * kr / c_green))
        v = np.stack([y + tr, y + tg, y + tb], axis=2)
    if mut == "round_nearest":
        return np.rint(np.clip(v, 0, 255)).astype(np.uint8)
    if mut == "no_lower_clamp":
        return (np.trunc(np.minimum(v, 255)).astype(np.int64) & 0xff).astype(np.uint8)
    if late128:
        return np.trunc(np.minimum(np.clip(v, 0, 255) + F32(128.0), 255)).astype(np.uint8)
    return np.trunc(np.clip(v, 0, 255)).astype(np.uint8)


CORNER_MUTANTS = ["corner11_2pct", "corner_const_1e-4"]
MUTANTS = ["const_1e-4", "qmult_transposed", "pos63_2pct", "round_nearest", "no_lower_clamp", "green_0.586", "plus128_after_clamp"]


# ---- CPU tests --------------------------------------------------------------------------------------------------------------------
def _cpu_pictures(variants=VARIANTS, shapes=(CPU_SHAPE,)):
    return [picture(v, *s) for s in shapes for v in variants]


def _oracle(p):
    return orc.decode(p.data, layout=orc.LAYOUT_STD)


@pytest.mark.parametrize("shape", [CPU_SHAPE] + CPU_OTHER, ids=lambda s: s[0])
def test_writer_round_trip_through_the_oracle(shape):
    """The oracle's T0 of every class file -- every layout, clipped MCUs, 16-bit DQT, the over-range class with its status OK --
    equals the blocks written, and scaled_ref sees the same tables and geometry."""
    for p in _cpu_pictures(shapes=(shape,)):
        ref = _oracle(p)
        assert (ref.width, ref.height) == (p.w, p.h), p.variant
        assert np.array_equal(orc.interleave(ref), p.blocks), p.variant
        w, h, comps, qt = scaled_ref.jpeg_tables(p.data)
        assert (w, h) == (p.w, p.h) and [tuple(c[:2]) for c in comps] == [tuple(x) for x in p.hv]
        assert all(np.array_equal(qt[c[2]], p.qts[k]) for k, c in enumerate(comps)), p.variant


def test_writer_restart_intervals_round_trip():
    """jpeg_from_blocks(restart=n): DRI n and RSTn markers every n MCUs, the DC predictors starting again -- the oracle's T0 and
    picture are those of the file without restart intervals."""
    for lname, w, h in (CPU_SHAPE, CPU_OTHER[1]):
        for v, n in (("pairs", 5), ("dense_300", 1), ("over_q3", 7)):
            p = picture(v, lname, w, h)
            huff = _huffman("full" if p.cls == 6 else "annex_k")
            data = jw.jpeg_from_blocks(p.blocks, p.hv, p.mcux, p.mcuy, p.qts, huff, qt16=p.qt16, width=w, height=h, restart=n)
            assert data != p.data and data.count(b"\xff\xdd") == 1 and data.count(b"\xff\xd0") >= 1
            a, b = orc.decode(data, layout=orc.LAYOUT_STD, ext_dri=True), _oracle(p)
            assert np.array_equal(orc.interleave(a), p.blocks) and np.array_equal(a.rgb, b.rgb), (lname, v, n)


@pytest.mark.parametrize("lname,w,h", [("444", 189, 131), ("gray", 187, 133)])
def test_pillow_decodes_the_writers_files_alike(lname, w, h):
    """A sanity pin of the writer from outside the project: where Pillow accepts the file and its integer pipeline clamps nothing
    on the way (the in-range classes; layouts without chroma upsampling, which Pillow smooths), its picture is within 2 of
    float64's (one level from its integer inverse DCT, one from its fixed-point colour)."""
    import io
    from PIL import Image
    for v in ("pairs", "dense_5", "dense_5n"):
        p = picture(v, lname, w, h)
        want = scaled_ref.rgb_f64(p.data, 1, p.dec)
        assert want.min() > 2 and want.max() < 253, v
        got = np.asarray(Image.open(io.BytesIO(p.data)).convert("RGB")).astype(F64)
        assert np.abs(got - want).max() <= 2.0, (v, float(np.abs(got - want).max()))


def test_K_is_measured_and_the_ambiguous_share_is_small():
    """K: the smallest K_a under which every sample of the oracle's float32 picture (scale 1) and K_b under which every sample of
    the numpy restatement of stage B (every scale) lies in its interval, over every class picture; the module's K is 4 x the larger,
    rounded up to a power of two: 4 max <= K < 8 max.  And at that K the interval decides: per class and scale at most 2 % of the
    samples have lo != hi (class 4 has no interval).  The cap is the full-size pictures' statement (0.07 .. 1.14 % per class); at
    1/2, 1/4 and 1/8 it holds for every class as well, with one exception that is asserted as what it is: sat_dense_q65535 at 1/4
    has 11 % (class 5 pooled: 3.3 %).  Its 2 x 2 corner is four coefficients of one magnitude A = 1023 x 65535, each of which
    contributes +-A / 8 to every sample (C(0) cos(pi/4) = 1/2), so 6 of 16 sign patterns cancel to exactly 128 under a band of
    +-32 levels: a property of the class the issue asks for, not of K.  The other class-5 pictures keep the cap at 1/4."""
    ka = kb = 0.0
    amb = {}
    for p in _cpu_pictures() + _cpu_pictures(shapes=CPU_OTHER[:1]):
        for scale in (1, 2, 4, 8):
            w, m = scaled_ref.rgb_f64(p.data, scale, p.dec), scaled_ref.magnitude(p.data, scale, p.dec)
            if scale == 1:
                ka = max(ka, needed_k(_oracle(p).rgb, w, m)[0])
            k, at = needed_k(stageb_f32(p, scale), w, m)
            kb = max(kb, k)
            if p.cls != 4:
                lo, hi = interval(p.variant, p.layout, p.w, p.h, scale)
                a = amb.setdefault((p.cls, scale), [0, 0])
                a[0] += int((lo != hi).sum())
                a[1] += lo.size
    print("K_a = %.3f, K_b = %.3f; ambiguous share per (class, scale): %s" % (ka, kb, {c: round(a[0] / a[1], 5) for c, a in amb.items()}))
    assert 4.0 * max(ka, kb) <= K < 8.0 * max(ka, kb) and K == 2 ** round(math.log2(K)), (ka, kb, K)
    for (c, scale), a in amb.items():
        if (c, scale) != (5, 4):
            assert a[0] <= AMBIGUOUS_CAP * a[1], (c, scale, a[0] / a[1])
    for shape in (CPU_SHAPE, CPU_OTHER[0]):                  # the exception, picture by picture
        for v in CLASSES[5]:
            lo, hi = interval(v, *shape, 4)
            assert ((lo != hi).mean() <= AMBIGUOUS_CAP) == (v != "sat_dense_q65535"), (v, shape, float((lo != hi).mean()))


def test_class_conditions_on_the_float64_reference():
    """What each class is for, asserted on float64 alone: the in-range amplitudes are in range, the dense class still has samples
    in range, the exact class is exact and runs through every level, the saturating class leaves the range on both sides."""
    lname, w, h = CPU_SHAPE
    for v in CLASSES[1][:2]:                                                 # (q = 65535: no amplitude is in range)
        p = picture(v, lname, w, h)
        f = scaled_ref.rgb_f64(p.data, 1, p.dec)
        mcu = (np.arange(h)[:, None] // (8 * p.vmax)) * p.mcux + np.arange(w)[None, :] // (8 * p.hmax)
        s = f[mcu % 3 == 1]
        assert ((s > 0) & (s < 255)).mean() >= 0.80, v
        for c, blk in enumerate(p.per_comp):                                 # every position, both signs, every amplitude kind
            nz = np.argwhere(blk)
            assert len(nz) == len(blk) and set(map(tuple, np.stack([nz[:, 1], np.sign(blk[nz[:, 0], nz[:, 1]])], 1))) == \
                {(k, s_) for k in range(64) for s_ in (-1, 1)}, (v, c)
    assert len({tuple(q) for q in picture("basis_q255", lname, w, h).qts}) == 3
    assert all((blk != 0).sum(axis=1).max() == 2 for blk in picture("pairs", lname, w, h).per_comp)
    for v in CLASSES[3]:
        p = picture(v, lname, w, h)
        assert all((blk != 0).mean() > 0.9 for blk in p.per_comp), v
        f = scaled_ref.rgb_f64(p.data, 1, p.dec)
        assert ((f > 0) & (f < 255)).mean() >= 0.30, (v, float(((f > 0) & (f < 255)).mean()))
    for v in CLASSES[4]:
        p = picture(v, lname, w, h)
        q = int(p.qts[0][0])
        lev = p.per_comp[0][:, 0] * q // 8 + 128
        assert np.all(p.per_comp[0][:, 0] * q % 8 == 0) and set(lev) == set(range(-40, 301)), v
        assert np.all(np.diff(lev) != 0)
        for scale in (1, 2, 4, 8):                                          # the expected bytes, by integer arithmetic alone
            n = 8 // scale
            pl = np.clip(lev, 0, 255).reshape(p.mcuy, p.mcux, 2, 2)
            pl = np.repeat(np.repeat(pl.transpose(0, 2, 1, 3).reshape(p.mcuy * 2, p.mcux * 2), n, 0), n, 1)[:-(-h // scale), :-(-w // scale)]
            want = interval(v, lname, w, h, scale)[0]
            assert np.array_equal(want, np.repeat(pl[:, :, None], 3, 2).astype(np.uint8)), (v, scale)
            assert np.array_equal(stageb_f32(p, scale), want), (v, scale)                   # (exact in float32 as well)
    below = above = inside = total = 0
    for v in CLASSES[5]:
        p = picture(v, lname, w, h)
        f = scaled_ref.rgb_f64(p.data, 1, p.dec)
        below, above, inside, total = below + int((f < 0).sum()), above + int((f > 255).sum()), inside + int(((f > 0) & (f < 255)).sum()), total + f.size
    assert below >= 0.2 * total and above >= 0.2 * total and inside >= 0.001 * total, (below / total, above / total, inside / total)
    f = scaled_ref.rgb_f64(picture("sat_chroma", lname, w, h).data, 1, picture("sat_chroma", lname, w, h).dec)
    for ch in range(3):                                                      # the channels leave the range one by one
        others = [k for k in range(3) if k != ch]
        for out in (f[:, :, ch] < 0, f[:, :, ch] > 255):
            assert (out & np.all((f[:, :, others] > 0) & (f[:, :, others] < 255), axis=2)).any(), ch
    for v in CLASSES[6]:
        p = picture(v, lname, w, h)
        big = np.concatenate([np.abs(b[:, 1:]).ravel() for b in p.per_comp])
        assert big.max() > 16384 and {int(x).bit_length() for x in big[big > 1023]} == {11, 12, 13, 14, 15}, v
        assert max(np.abs(b[:, 0]).max() for b in p.per_comp) > (1900 if v == "over_q1" else 950)


def test_plants(mjx):
    """Each planted error in the restatement leaves the interval on at least one class picture (the seven of the full-size path at
    scale 1; a 2 % error in the corner multiplier of position (1, 1) and a corner-transform constant off by 1e-4 at 1/2 and 1/4).  Recorded beside it: whether the
    same error would have passed the older check, |difference| <= 1 against the oracle on a natural-content 4:2:0 picture at
    quality 75 -- the multiplier and constant errors do."""
    data = mjx.synth_jpeg(381, 250, "420", 75, seed=11)
    ref = orc.decode(data, layout=orc.LAYOUT_STD)
    _, _, comps, qt = scaled_ref.jpeg_tables(data)
    nat = types.SimpleNamespace(hv=LAYOUTS["420"], w=381, h=250, mcux=24, mcuy=16, hmax=2, vmax=2, per_mcu=[4, 1, 1],
                                per_comp=[c.astype(np.int64) for c in ref.coefs], qts=[np.asarray(qt[c[2]], np.int64) for c in comps])
    assert np.abs(stageb_f32(nat, 1).astype(int) - ref.rgb.astype(int)).max() <= 1          # the unmutated restatement passes both
    pics = _cpu_pictures()
    old_passes = {}
    for mut in MUTANTS:
        caught = []
        for p in pics:
            lo, hi = interval(p.variant, p.layout, p.w, p.h, 1)
            got = stageb_f32(p, 1, mut)
            if ((got < lo) | (got > hi)).any():
                caught.append(p.variant)
        assert caught, mut
        old_passes[mut] = bool(np.abs(stageb_f32(nat, 1, mut).astype(int) - ref.rgb.astype(int)).max() <= 1)
        print("plant %-20s caught by %2d of %d pictures; passes the +-1 check on natural content: %s" % (mut, len(caught), len(pics), old_passes[mut]))
    assert old_passes["pos63_2pct"] and old_passes["const_1e-4"], old_passes
    for mut in CORNER_MUTANTS:                                               # the corner forms: a multiplier and a constant of theirs
        for scale in (2, 4):
            caught = [p.variant for p in pics
                      if (lambda lo, hi, got: ((got < lo) | (got > hi)).any())(*interval(p.variant, p.layout, p.w, p.h, scale), stageb_f32(p, scale, mut))]
            print("plant %-20s at 1/%d caught by %2d of %d pictures" % (mut, scale, len(caught), len(pics)))
            assert caught, (mut, scale)
    for p in pics:                                                           # and nothing is caught without a plant
        lo, hi = interval(p.variant, p.layout, p.w, p.h, 1)
        got = stageb_f32(p, 1)
        assert not ((got < lo) | (got > hi)).any(), p.variant


REF_SHAPES = [("444", 320, 216), ("gray", 328, 216)]
REF_VARIANTS = CLASSES[1] + CLASSES[4] + CLASSES[5]


def test_ref_and_std_pictures_agree_on_the_ref_compat_geometries():
    """The REF_COMPAT test applies the STANDARD interval: on its geometries the oracle's two layouts give one picture."""
    for lname, w, h in REF_SHAPES:
        for v in REF_VARIANTS:
            p = picture(v, lname, w, h)
            a, b = orc.decode(p.data, layout=orc.LAYOUT_REF, strict_ref=True), orc.decode(p.data, layout=orc.LAYOUT_STD)
            assert np.array_equal(a.rgb, b.rgb) and all(np.array_equal(x, y) for x, y in zip(a.coefs, b.coefs)), (lname, v)


# ---- GPU tests --------------------------------------------------------------------------------------------------------------------
GPU_SHAPES = {"420": (1035, 490), "444": (333, 217), "422": (333, 217), "440": (333, 217), "gray": (333, 217), "Y22_Cb21_Cr12": (333, 217)}


def _decode(mjx, ctx, datas, keep_coefs=True, **kw):
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, keep_coefs=keep_coefs, **kw)
    assert all(s == mjx.OK for s in b.create_status), b.create_status
    b.decode()
    b.wait()
    b.scans = scans                      # (alive as long as the batch)
    return b


def _check_batch(mjx, b, pics, scale, tag, t0=True):
    for i, p in enumerate(pics):
        assert b.status(i) == mjx.OK, (tag, p.variant, b.status(i))
        if t0:
            assert np.array_equal(b.coefs(i), p.blocks), (tag, p.variant, "T0")
        check(p, scale, b.rgb(i), tag)


def _is_dense(mjx, p):
    """the planner's rule for the dense prefetch form, per picture: scan bytes > 1400 per stage-B tile (and one tile to spare)"""
    scan = mjx.ParsedScan(p.data)
    try:
        return scan.desc.scan_len > (scan.plan_tiles()["tiles_total"] + 1) * 1400
    finally:
        scan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("density", ["sparse", "dense"])
@pytest.mark.parametrize("stream", ["quad", "linear"])
@pytest.mark.parametrize("lname", list(GPU_SHAPES))
def test_standard(mjx, lname, stream, density):
    """STANDARD at scale 1, every class, through both stream sources and both prefetch forms.  The dense form is chosen per chunk
    at scan_bytes > tiles x 1400: every picture of the `dense` batch is above that on its own, every one of the `sparse` batch
    below, so whatever the chunks are, the batch says which form it ran."""
    w, h = GPU_SHAPES[lname]
    pics = [picture(v, lname, w, h) for v in VARIANTS]
    dense = [_is_dense(mjx, p) for p in pics]
    if lname == "420":                    # (the only kernel with a dense form; elsewhere `density` just splits the classes)
        assert all(d for p, d in zip(pics, dense) if p.cls == 3) and not any(d for p, d in zip(pics, dense) if p.cls in (1, 2, 4))
    else:
        dense = [p.cls in (3, 5) for p in pics]
    batch = [p for p, d in zip(pics, dense) if d == (density == "dense")]
    old = os.environ.get("MJX_STREAM_LINEAR")
    try:
        os.environ["MJX_STREAM_LINEAR"] = "1" if stream == "linear" else "0"
        ctx = mjx.Context(0)
        b = _decode(mjx, ctx, [p.data for p in batch])
        _check_batch(mjx, b, batch, 1, "standard-%s-%s" % (stream, density))
        b.close()
        ctx.close()
    finally:
        if old is None:
            os.environ.pop("MJX_STREAM_LINEAR", None)
        else:
            os.environ["MJX_STREAM_LINEAR"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("density", ["sparse", "dense"])
@pytest.mark.parametrize("lname,w,h", [("420", 1035, 490), ("444", 1000, 40)])
def test_multiscan_twins(mjx, gpu_ctx, lname, w, h, density):
    """Two multi-scan scripts of every class picture.  Without keep_coefs and with a tile on at most two MCU rows, stage B reads the
    scans' streams directly (SRC 2): planar_ok admits both scripts -- at most four segment kinds, an interleaved pair of two blocks
    per MCU -- and its tile rule is asserted here through test_sampling_layouts.planar_fits, so the row survives a change of tile
    size.  With keep_coefs the same files go through the gather (and give T0).  The sparse and the dense pictures go in batches of
    their own."""
    import test_sampling_layouts as sl
    scripts = {"Y;Cb;Cr": sum(v for _, v in LAYOUTS[lname]), "Cb Cr;Y": 1 + LAYOUTS[lname][0][1]}      # script: segment kinds per MCU
    assert all(sl.planar_fits(LAYOUTS[lname], w, 1, kinds) for kinds in scripts.values())
    # (over_q1 is left out: its DC values reach +-2047, and in a scan's own block order their differences would need size 12)
    pics = [picture(v, lname, w, h) for v in VARIANTS if v != "over_q1" and (CLASS_OF[v] in (3, 5)) == (density == "dense")]
    twins, owner = [], []
    for p in pics:
        ref = types.SimpleNamespace(coefs=[c.astype(np.int16) for c in p.per_comp], mcus=p.mcux * p.mcuy)
        for t in jw.script_twins(p.data, ref, list(scripts)):
            twins.append(t)
            owner.append(p)
    direct = _decode(mjx, gpu_ctx, twins, keep_coefs=False)
    _check_batch(mjx, direct, owner, 1, "twins-direct", t0=False)
    gathered = _decode(mjx, gpu_ctx, twins, keep_coefs=True)
    _check_batch(mjx, gathered, owner, 1, "twins-gathered")
    direct.close()
    gathered.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("lname", ["420", "Y22_Cb21_Cr12"])
def test_scaled(mjx, gpu_ctx, lname, scale):
    """The 4 x 4 and 2 x 2 corner transforms and the DC-only form, every class, against rgb_interval at that scale."""
    w, h = GPU_SHAPES[lname]
    pics = [picture(v, lname, w, h) for v in VARIANTS]
    b = _decode(mjx, gpu_ctx, [p.data for p in pics], scale=scale)
    _check_batch(mjx, b, pics, scale, "scaled")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lname,w,h", REF_SHAPES)
def test_ref_compat(mjx, gpu_ctx, lname, w, h):
    """REF_COMPAT (its own placement kernel, k_ref_color and the floor-then-convert store) on geometries where the reference's
    picture is the STANDARD one (asserted on the CPU above): classes 1, 4 and 5 inside the STANDARD interval."""
    pics = [picture(v, lname, w, h) for v in REF_VARIANTS]
    b = _decode(mjx, gpu_ctx, [p.data for p in pics], layout=mjx.LAYOUT_REF_COMPAT)
    _check_batch(mjx, b, pics, 1, "ref_compat")
    b.close()


def _rects(ow, oh):
    """two rectangles with odd corners and sizes, neither aligned to an MCU nor to four bytes"""
    a = (3, 5, max(1, ow // 2 + 1), max(1, oh // 2 + 2))
    x, y = (ow // 3) | 1, (oh // 4) | 1
    return [a, (x, y, max(1, ow - x - 2), max(1, oh - y - 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("lname", ["420", "444"])
def test_roi_and_formats(mjx, gpu_ctx, lname, scale):
    """The contracts of test_roi_decode.py and test_output_formats.py on the dense and the saturating class: a rectangle is the
    crop of the uncropped device picture byte for byte, an Output is the format table applied to it bit for bit."""
    import test_output_formats as tof
    w, h = GPU_SHAPES[lname]
    pics = [picture(v, lname, w, h) for v in CLASSES[3] + CLASSES[5]]
    datas = [p.data for p in pics]
    full = _decode(mjx, gpu_ctx, datas, scale=scale)
    _check_batch(mjx, full, pics, scale, "roi-full")
    whole = [full.rgb(i) for i in range(len(pics))]
    full.close()
    ow, oh = -(-w // scale), -(-h // scale)
    for r in _rects(ow, oh):
        b = _decode(mjx, gpu_ctx, datas, keep_coefs=False, scale=scale, rois=r)
        for i, p in enumerate(pics):
            assert b.status(i) == mjx.OK and np.array_equal(b.rgb(i), whole[i][r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), (p.variant, scale, r)
        b.close()
    formats = [mjx.Output("float32", planar=True, mean=tof.IMAGENET_MEAN, std=tof.IMAGENET_STD),
               mjx.Output("float16", planar=False, bgr=True, mean=tof.IMAGENET_MEAN[::-1], std=tof.IMAGENET_STD[::-1]), mjx.Output("uint8")]
    for fmt in formats:
        b = _decode(mjx, gpu_ctx, datas, keep_coefs=False, scale=scale, output=fmt)
        for i, p in enumerate(pics):
            assert b.status(i) == mjx.OK and tof.same_bits(b.output(i), tof.expected(whole[i], fmt)), (p.variant, scale, fmt.dtype, fmt.planar)
        b.close()

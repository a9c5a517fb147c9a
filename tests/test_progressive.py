"""Progressive JPEG (SOF2) on the device, behind MJX_OPTS_PROGRESSIVE (include/mjx.h): every test here needs the GPU.

References (tests/prog_cases.py builds them): (a) Pillow's baseline twin of every progressive file -- libjpeg codes identical
coefficients for both, and the twins' equality under Pillow is re-asserted when a pair is made; (b) tests/prog_ref.py, a serial Python
restatement of T.81 G.2 with the statuses include/mjx.h specifies; (c) tests/progwriter.py for scan scripts Pillow does not write.

Padding blocks: a progressive file carries nothing of the blocks that exist only as MCU padding beyond what an interleaved DC scan
sends, and the library hands them out as zeros; a baseline file codes them in full.  Coefficients are therefore compared on the blocks
of the components' own grids (prog_cases.real_blocks), exactly; no pixel of the picture comes from a padding block, and pictures are
compared byte for byte.  Without the opt-in every progressive file is MJX_ERR_UNSUPPORTED_FORMAT, so each test fails on a build that
lacks the feature.
"""
import ctypes

import numpy as np
import pytest

import prog_cases as pc
import prog_ref

pytestmark = pytest.mark.gpu


def _batch(mjx, ctx, datas, **kw):
    scans = [mjx.ParsedScan(d, progressive=True, color=kw.get("color")) for d in datas]
    b = mjx.Batch(ctx, scans, progressive=True, **kw)
    b.decode()
    b.wait()
    return b


class _DeviceMemory:
    """`n` slots of `nbytes` of caller-owned device memory from the HIP runtime the library is linked against, sentinel-filled"""

    def __init__(self, mjx, n, nbytes, sentinel):
        h = mjx.lib()
        h.hipMalloc.restype = h.hipFree.restype = h.hipMemset.restype = h.hipMemcpy.restype = h.hipDeviceSynchronize.restype = ctypes.c_int
        h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        h.hipFree.argtypes = [ctypes.c_void_p]
        h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        h.hipDeviceSynchronize.argtypes = []
        self.h, self.n, self.slot = h, n, (nbytes + 255) // 256 * 256
        self.base = ctypes.c_void_p()
        assert h.hipMalloc(ctypes.byref(self.base), n * self.slot) == 0
        assert h.hipMemset(self.base, sentinel, n * self.slot) == 0 and h.hipDeviceSynchronize() == 0

    def ptr(self, i):
        return self.base.value + i * self.slot

    def read(self):
        """-> uint8 [n, slot]"""
        mem = np.empty(self.n * self.slot, np.uint8)
        assert self.h.hipDeviceSynchronize() == 0 and self.h.hipMemcpy(mem.ctypes.data, self.base, mem.nbytes, 2) == 0
        return mem.reshape(self.n, self.slot)

    def free(self):
        self.h.hipFree(self.base)


def _refused_without_opt_in(mjx, data):
    with pytest.raises(mjx.MjxError) as e:
        mjx.ParsedScan(data)
    assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT


def _twin_check(mjx, ctx, base, prog):
    _refused_without_opt_in(mjx, prog)
    b = _batch(mjx, ctx, [base, prog], keep_coefs=True)
    assert [b.status(0), b.status(1)] == [mjx.OK, mjx.OK]
    inf = b.info(1)
    real = pc.real_blocks(inf["width"], inf["height"], pc.hv_of(prog))
    c0, c1 = b.coefs(0), b.coefs(1)
    assert c0.shape == c1.shape and real.shape[0] == c1.shape[0]
    assert np.array_equal(c1[real], c0[real])
    assert not c1[~real].any()
    assert np.array_equal(b.rgb(1), b.rgb(0))
    return b


@pytest.mark.parametrize("name", [x[0] for x in pc.LAYOUTS + pc.SIZES])
def test_twins_decode_to_the_baseline_coefficients_and_bytes(mjx, gpu_ctx, name):
    base, prog = pc.layout_pair(name)
    _twin_check(mjx, gpu_ctx, base, prog)
    # ... and without keep_coefs (the chunk's scratch stream)
    b = _batch(mjx, gpu_ctx, [prog, base])
    assert np.array_equal(b.rgb(0), b.rgb(1))


@pytest.mark.parametrize("quality", [30, 85, 100])
def test_twins_at_other_qualities(mjx, gpu_ctx, quality):
    for name in ("422_33x40", "420_70x52", "grey_23x31"):
        _twin_check(mjx, gpu_ctx, *pc.layout_pair(name, quality))


@pytest.mark.parametrize("shape", list(pc.WRITER_SHAPES))
def test_writer_scripts_on_constructed_blocks(mjx, gpu_ctx, shape):
    names = list(pc.writer_scripts(shape))
    cases = [pc.writer_case(shape, n) for n in names]
    for prog, _, _, _ in cases:
        _refused_without_opt_in(mjx, prog)
    b = _batch(mjx, gpu_ctx, [c[0] for c in cases] + [c[1] for c in cases], keep_coefs=True)
    n = len(cases)
    for k, (name, (prog, base, held, real)) in enumerate(zip(names, cases)):
        assert b.status(k) == mjx.OK and b.status(n + k) == mjx.OK, name
        got = b.coefs(k)
        assert np.array_equal(got[real], held[real]), name          # the blocks the file was written from (masked where the progression stops)
        assert not got[~real].any(), name
        assert np.array_equal(b.coefs(n + k)[real], held[real]), name
        assert np.array_equal(b.rgb(k), b.rgb(n + k)), name


def test_long_end_of_band_runs(mjx, gpu_ctx):
    """A flat 1024 x 1024 grey picture with one textured block: 16 384 blocks, whose AC scans are almost nothing but end-of-band
    runs.  The block's texture is a ramp: it has coefficients in the low band only, so the scans of the high band are ONE run over
    all 16 384 blocks -- category 14 (16 384 .. 32 767), which prog_ref's symbol statistics confirm."""
    from PIL import Image
    a = np.full((1024, 1024), 128, np.uint8)
    a[8:16, 8:16] = 128 + np.arange(8)[None, :] * 4 + np.arange(8)[:, None] * 2
    base, prog = pc.twins_of(Image.fromarray(a, "L"), 75)
    ref = prog_ref.decode(prog)
    assert ref.status == prog_ref.OK and ref.stats["max_eob_category"] == 14 and np.count_nonzero(ref.coefs[:, 1:]) > 0
    b = _twin_check(mjx, gpu_ctx, base, prog)
    assert np.array_equal(b.coefs(1), ref.coefs)


def test_restart_intervals(mjx, gpu_ctx):
    """the 56 x 40 pair with an interval of three MCUs, and one MCU row per interval: a lane per interval of every scan"""
    _twin_check(mjx, gpu_ctx, *pc.layout_pair("420_56x40_rst3"))
    _twin_check(mjx, gpu_ctx, *pc.pillow_pair(56, 40, "RGB", 2, 75, 0, 1))
    _twin_check(mjx, gpu_ctx, *pc.pillow_pair(23, 31, "L", 0, 75, 0, 1))


def _both(mjx, ctx, pair, getter, **kw):
    b = _batch(mjx, ctx, list(pair), **kw)
    assert [b.status(0), b.status(1)] == [mjx.OK, mjx.OK]
    x, y = getter(b, 0), getter(b, 1)
    if isinstance(x, tuple):
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    else:
        assert x.shape == y.shape and np.array_equal(x, y)
    return b


def test_composition_is_the_baseline_twin_through_the_same_call(mjx, gpu_ctx):
    pair = pc.layout_pair("420_70x52")
    rgb = lambda b, i: b.rgb(i)
    out = lambda b, i: b.output(i)
    for s in (2, 4, 8):
        _both(mjx, gpu_ctx, pair, rgb, scale=s)
    _both(mjx, gpu_ctx, pair, rgb, rois=(13, 9, 40, 30))
    _both(mjx, gpu_ctx, pair, rgb, rois=(5, 3, 20, 11), scale=2)
    _both(mjx, gpu_ctx, pair, out, output=mjx.Output("float16", planar=True, mean=[0.4, 0.5, 0.6], std=[0.2, 0.3, 0.25]))
    mem = _DeviceMemory(mjx, 2, 3 * 52 * 70 * 2, 0x5a)                      # float16 CHW into the caller's memory
    try:
        where = [(mem.ptr(i), 70, 52, 70, 52 * 70) for i in range(2)]
        b = _batch(mjx, gpu_ctx, list(pair), output=mjx.Output("float16", planar=True, mean=[0.4, 0.5, 0.6], std=[0.2, 0.3, 0.25], dst=where))
        assert [b.status(0), b.status(1)] == [mjx.OK, mjx.OK]
        got = mem.read()[:, :3 * 52 * 70 * 2]
        assert np.array_equal(got[0], got[1]) and not (got[1] == 0x5a).all()
    finally:
        mem.free()
    _both(mjx, gpu_ctx, pair, out, output=mjx.Output("uint8", channels=1))
    _both(mjx, gpu_ctx, pair, lambda b, i: b.planes(i), planes=mjx.Planes("uint8", interleave=True))
    _both(mjx, gpu_ctx, pair, out, resize=mjx.Resize(48, 48, filter="bicubic", fit="contain"), output=mjx.Output("uint8", pad=[9, 8, 7]))
    _both(mjx, gpu_ctx, pair, out, orient=mjx.Orient(exif=False, extra=6))
    _both(mjx, gpu_ctx, pair, rgb, pixels="libjpeg")
    _both(mjx, gpu_ctx, pair, rgb, color="file")
    _both(mjx, gpu_ctx, pc.layout_pair("grey_23x31"), rgb, color="file")
    _both(mjx, gpu_ctx, pc.layout_pair("444_17x9"), rgb, color="file")


def test_tiled_batches_and_repeated_decodes(mjx, gpu_ctx):
    """mjx_batch_tile carries the progressive pictures along; decoding a batch twice gives the same pictures and statuses"""
    base, prog = pc.layout_pair("420_70x52")
    rst = pc.layout_pair("420_56x40_rst3")[1]
    cut = prog[:len(prog) - 40]
    src = _batch(mjx, gpu_ctx, [prog, base, rst, cut])
    want = [mjx.OK, mjx.OK, mjx.OK, mjx.ERR_TRUNCATED]
    assert [src.status(i) for i in range(4)] == want
    t = src.tile(3)
    for _ in range(2):
        t.decode()
        t.wait()
        assert [t.status(i) for i in range(12)] == want * 3
        for r in range(3):
            assert np.array_equal(t.rgb(4 * r), src.rgb(1)) and np.array_equal(t.rgb(4 * r + 1), src.rgb(1))
            assert np.array_equal(t.rgb(4 * r + 2), src.rgb(2))
    # (the dense store is counted: 70 x 52 at 4:2:0 is 5 x 4 MCUs of 6 blocks, 56 x 40 is 4 x 3; the truncated picture counts nothing)
    assert src.bytes()["coef"] - _batch(mjx, gpu_ctx, [base]).bytes()["coef"] >= (20 + 12) * 6 * 128


def test_front_doors_take_the_option(mjx, gpu_ctx):
    """mjx_decode, the JPEGImage mirror and the pool beside the batch calls"""
    base, prog = pc.layout_pair("422_33x40")
    want = mjx.decode(base)
    assert np.array_equal(mjx.decode(prog, progressive=True), want)
    assert np.array_equal(mjx.decode(prog, progressive=True, scale=2), mjx.decode(base, scale=2))
    with pytest.raises(mjx.MjxError) as e:
        mjx.decode(prog)
    assert e.value.code == mjx.ERR_UNSUPPORTED_FORMAT
    with pytest.raises(mjx.MjxError) as e:
        mjx.decode(prog, progressive=2)
    assert e.value.code == mjx.ERR_INVALID_ARG
    img = mjx.JPEGImage.parse(prog, ctx=gpu_ctx, progressive=True)
    assert (img.width(), img.height()) == (33, 40)
    pool = mjx.Pool([0])
    try:
        res = pool.decode_batch([base, prog, prog[:len(prog) - 30]], progressive=True)
        try:
            assert list(res.status) == [mjx.OK, mjx.OK, mjx.ERR_TRUNCATED]
            assert np.array_equal(res.rgb(1), want) and np.array_equal(res.rgb(0), want)
        finally:
            res.close()
    finally:
        pool.close()


def test_mixed_call_with_slots_and_statuses(mjx, gpu_ctx):
    """one call mixing a baseline file, a progressive one, a multi-scan one and a truncated one; once more with one picture per chunk"""
    import os
    base, prog = pc.layout_pair("420_70x52")
    ms = open(os.path.join(pc.ROOT, "tests", "golden", "pil", "ms_420_odd.jpg"), "rb").read()
    cut = prog[:len(prog) - 40]
    assert prog_ref.decode(cut).status == prog_ref.TRUNCATED
    datas = [base, prog, ms, cut, prog]
    want = [mjx.OK, mjx.OK, mjx.OK, mjx.ERR_TRUNCATED, mjx.OK]
    solo = _batch(mjx, gpu_ctx, [ms]).rgb(0)
    for chunk in (0, 1):
        b, st = mjx.decode_batch(gpu_ctx, datas, chunk_images=chunk, progressive=True)
        assert len(b) == 5 and [b.status(i) for i in range(5)] == want and st == want, chunk
        assert np.array_equal(b.rgb(1), b.rgb(0)) and np.array_equal(b.rgb(4), b.rgb(0)), chunk
        assert np.array_equal(b.rgb(2), solo), chunk
        b2 = _batch(mjx, gpu_ctx, datas, chunk_images=chunk)
        assert [b2.status(i) for i in range(5)] == want, chunk
        assert np.array_equal(b2.rgb(1), b2.rgb(0)) and np.array_equal(b2.rgb(2), solo), chunk


def test_damaged_scans_answer_as_the_serial_reference(mjx, gpu_ctx):
    """The damaged set in one call: status -- the parser's refusals among them -- and, where OK, coefficients equal prog_ref's; a
    picture that is not OK hands out nothing: its caller-owned output keeps the sentinel.  Every case is compared."""
    datas = [pc.layout_pair("422_33x40")[1]] + pc.damaged_set()
    refs = [prog_ref.decode(d) for d in datas]
    assert refs[0].status == prog_ref.OK
    assert {prog_ref.OK, prog_ref.TRUNCATED, prog_ref.BAD_HUFFMAN} <= {r.status for r in refs}
    b, st = mjx.decode_batch(gpu_ctx, datas, progressive=True, keep_coefs=True)
    for i, r in enumerate(refs):
        assert st[i] == r.status and b.status(i) == r.status, i
        if r.status == prog_ref.OK:
            assert np.array_equal(b.coefs(i), r.coefs), i
    mem = _DeviceMemory(mjx, len(datas), 40 * 33 * 3, 77)
    try:
        where = [(mem.ptr(i), 33, 40, 99, 0) for i in range(len(datas))]
        b, st = mjx.decode_batch(gpu_ctx, datas, progressive=True, output=mjx.Output("uint8", dst=where))
        got = mem.read()
        assert not (got[0, :40 * 33 * 3] == 77).all() and (got[:, 40 * 33 * 3:] == 77).all()
        for i, r in enumerate(refs):
            assert st[i] == r.status, i
            assert (r.status == prog_ref.OK) or (got[i] == 77).all(), i
    finally:
        mem.free()

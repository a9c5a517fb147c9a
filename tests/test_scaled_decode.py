"""Scaled decode at 1/2, 1/4 and 1/8 in the DCT domain (mjx_opts.scale_denom, include/mjx.h).

The expected pictures come from tests/scaled_ref.py, a float64 numpy reference of the contract built on the oracle's
coefficients.  CPU tests check the reference itself (scale 1 = the oracle's picture; the scaled pictures are close to box means
of the full picture) and the argument checks; GPU tests compare every front door with it (TOL per byte, under 1 % of bytes
differing).
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import scaled_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1
SCALES = (2, 4, 8)


def _fixtures():
    out = sorted(glob.glob(os.path.join(ROOT, "tests", "data", "*.jp*g")))
    out += [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pil", "*.jpg"))) if "progressive" not in p]
    return out


FIXTURES = _fixtures()


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _oracle(orc, data):
    return orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= TOL, (what, int(d.max()), np.argwhere(d > TOL)[:4].tolist())
    assert (d > 0).mean() < 0.01, (what, float((d > 0).mean()))


# ---- CPU: the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_reference_at_scale_1_is_the_oracle(orc, path):
    data = _read(path)
    dec = _oracle(orc, data)
    got = scaled_ref.scaled_rgb(data, 1, dec)
    d = np.abs(got.astype(np.int32) - dec.rgb.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("name", ["opt_444_q40.jpg", "opt_gray_q70.jpg"])
@pytest.mark.parametrize("scale", SCALES)
def test_reference_is_near_the_box_mean_of_the_full_picture(orc, name, scale):
    # independent of the formula: a flat block keeps its level at every scale, and on smooth content the reduced transform is
    # close to averaging the full picture (a factor-2 slip on the AC terms fails this)
    data = _read(os.path.join(ROOT, "tests", "golden", "pil", name))
    dec = _oracle(orc, data)
    got = scaled_ref.scaled_rgb(data, scale, dec).astype(np.float64)
    want = scaled_ref.box_mean(dec.rgb.astype(np.float64), scale)
    assert got.shape == want.shape
    assert np.abs(got - want).mean() < 2.0, float(np.abs(got - want).mean())


# ---- CPU: argument checks ---------------------------------------------------------------------------------------------------
def test_ref_compat_and_other_denominators_are_invalid(mjx):
    scan = mjx.ParsedScan(_read(os.path.join(ROOT, "tests", "data", "lena.jpeg")))
    try:
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT, scale=2) == mjx.ERR_INVALID_ARG
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT, scale=1) == mjx.OK
        for s in (3, 16, 5, 255):
            assert scan.validate(scale=s) == mjx.ERR_INVALID_ARG, s
        for s in (0, 1, 2, 4, 8):
            assert scan.validate(scale=s) == mjx.OK, s
    finally:
        scan.close()
    # a multi-scan file is checked scan by scan and as a picture
    scan = mjx.ParsedScan(_read(os.path.join(ROOT, "tests", "golden", "pil", "ms_420_odd.jpg")))
    try:
        assert scan.validate(scale=4) == mjx.OK
        assert scan.validate(scale=6) == mjx.ERR_INVALID_ARG
    finally:
        scan.close()


def test_scaled_decode_without_a_device_is_a_device_error(tmp_path):
    """No fallback: mjx_decode with a scale and no visible device says MJX_ERR_DEVICE (a child process with the devices hidden)."""
    script = tmp_path / "nodev.py"
    script.write_text(
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "data = open(os.path.join(%r, 'tests', 'data', 'lena.jpeg'), 'rb').read()\n"
        "try:\n"
        "    mjx.decode(data, scale=4)\n"
        "    print('decoded')\n"
        "except mjx.MjxError as e:\n"
        "    print('rc', e.code)\n" % (ROOT, ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import importlib
    sys.path.insert(0, ROOT)
    ge = importlib.import_module("__graft_entry__")
    assert out.stdout.split() == ["rc", str(ge.load_package().ERR_DEVICE)], out.stdout


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
_CHILD = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import __graft_entry__ as ge, scaled_ref, oracle_binding as orc
mjx = ge.load_package()
ctx = mjx.Context(0)
paths = json.loads(%(paths)r)
bad = []
for p in paths:
    data = open(p, 'rb').read()
    dec = orc.decode(data, layout=orc.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)
    for s in (2, 4, 8):
        want = scaled_ref.scaled_rgb(data, s, dec)
        b = mjx.Batch(ctx, [mjx.ParsedScan(data)], scale=s)
        b.decode(); b.wait()
        if b.status(0) != 0:
            bad.append((os.path.basename(p), s, 'status', b.status(0))); b.close(); continue
        got = b.rgb(0)
        b.close()
        if got.shape != want.shape:
            bad.append((os.path.basename(p), s, 'shape', got.shape, want.shape)); continue
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        if d.max() > 1 or (d > 0).mean() >= 0.01:
            bad.append((os.path.basename(p), s, int(d.max()), float((d > 0).mean())))
print(json.dumps(bad))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("single_decode", [None, "0"], ids=["single_decode_default", "single_decode_0"])
def test_fixtures_at_every_scale(mjx, tmp_path, single_decode):
    import json
    script = tmp_path / "scaled.py"
    script.write_text(_CHILD % dict(root=ROOT, paths=json.dumps(FIXTURES)))
    env = {k: v for k, v in os.environ.items() if k != "MJX_SINGLE_DECODE"}
    if single_decode is not None:
        env["MJX_SINGLE_DECODE"] = single_decode
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == []


def _batch_rgb(mjx, ctx, data, scale):
    b = mjx.Batch(ctx, [mjx.ParsedScan(data)], scale=scale)
    try:
        b.decode()
        b.wait()
        assert b.status(0) == mjx.OK
        return b.rgb(0)
    finally:
        b.close()


SYNTH_SIZES = [(1, 1), (7, 5), (17, 33), (61, 45), (750, 595), (1001, 37)]      # (1001: ceil(1001 / s) * 3 is not a multiple of 4)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["gray", "420", "422", "440", "444"])
@pytest.mark.parametrize("quality", [50, 90])
def test_synthetic_pictures_odd_sizes(mjx, orc, gpu_ctx, sub, quality):
    for k, (w, h) in enumerate(SYNTH_SIZES):
        data = mjx.synth_jpeg(w, h, sub, quality, seed=k + 11)
        dec = _oracle(orc, data)
        for s in SCALES:
            _close(_batch_rgb(mjx, gpu_ctx, data, s), scaled_ref.scaled_rgb(data, s, dec), (sub, quality, w, h, s))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_synthetic_hd_and_4k(mjx, orc, gpu_ctx, w, h):
    for sub in ("420", "444"):
        data = mjx.synth_jpeg(w, h, sub, 75, seed=5)
        dec = _oracle(orc, data)
        for s in SCALES:
            _close(_batch_rgb(mjx, gpu_ctx, data, s), scaled_ref.scaled_rgb(data, s, dec), (sub, w, h, s))


@pytest.mark.gpu
def test_every_front_door_gives_the_batch_bytes(mjx, gpu_ctx, tmp_path):
    paths = [os.path.join(ROOT, "tests", "data", "lena.jpeg"), os.path.join(ROOT, "tests", "golden", "pil", "dri_422_rows.jpg"),
             os.path.join(ROOT, "tests", "golden", "pil", "ms_420_odd.jpg"), os.path.join(ROOT, "tests", "data", "lena-bw.jpeg")]
    datas = [_read(p) for p in paths]
    cli = os.path.join(os.path.dirname(mjx.lib_path()), "mjx_cli")
    for s in SCALES:
        want = [_batch_rgb(mjx, gpu_ctx, d, s) for d in datas]
        for d, w in zip(datas, want):
            assert np.array_equal(mjx.decode(d, scale=s), w)                                   # mjx_decode
            img = mjx.JPEGImage.parse(d, ctx=gpu_ctx, scale=s)
            assert (img.width(), img.height()) == (w.shape[1], w.shape[0])
            assert np.array_equal(img.image_data(), w)
        for dd in (True, False):                                                              # mjx_decode_batch
            b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd, scale=s)
            try:
                assert st == [mjx.OK] * len(datas)
                for i, w in enumerate(want):
                    assert b.info(i)["width"] == w.shape[1] and b.info(i)["height"] == w.shape[0]
                    assert np.array_equal(b.rgb(i), w), (dd, s, i)
                    assert b.rgb_device(i)[1] == w.nbytes
                assert b.bytes()["rgb"] == sum(w.nbytes for w in want)
                assert b.bytes()["pixels"] == sum(w.shape[0] * w.shape[1] for w in want)
            finally:
                b.close()
        pool = mjx.Pool([0])                                                                   # mjx_pool
        try:
            r = pool.decode_batch(datas, scale=s)
            try:
                assert r.status == [mjx.OK] * len(datas)
                for i, w in enumerate(want):
                    assert np.array_equal(r.rgb(i), w)
            finally:
                r.close()
        finally:
            pool.close()
        out = tmp_path / "o.ppm"                                                               # the CLI
        subprocess.check_call([cli, paths[0], str(out), "--p6", "--scale", str(s)])
        raw = out.read_bytes()
        head = raw.split(b"\n", 3)
        assert head[0] == b"P6" and head[1] == b"%d %d" % (want[0].shape[1], want[0].shape[0])
        assert np.array_equal(np.frombuffer(head[3], np.uint8).reshape(want[0].shape), want[0])
        b = mjx.Batch(gpu_ctx, [mjx.ParsedScan(d) for d in datas], scale=s)                    # tile() keeps the scale
        try:
            t = b.tile(3)
            try:
                t.decode()
                t.wait()
                for i in range(3 * len(datas)):
                    w = want[i % len(datas)]
                    assert (t.info(i)["width"], t.info(i)["height"]) == (w.shape[1], w.shape[0])
                    assert np.array_equal(t.rgb(i), w), (s, i)
            finally:
                t.close()
        finally:
            b.close()
    assert subprocess.call([cli, paths[0], str(tmp_path / "x.ppm"), "--scale", "3"]) == mjx.ERR_INVALID_ARG


@pytest.mark.gpu
def test_a_bad_picture_does_not_stop_the_others(mjx, orc, gpu_ctx):
    good = _read(os.path.join(ROOT, "tests", "data", "lena.jpeg"))
    bad = _read(os.path.join(ROOT, "tests", "golden", "pil", "progressive.jpg"))      # refused (DESIGN s8)
    datas = [good, bad, good]
    dec = _oracle(orc, good)
    for s in SCALES:
        want = scaled_ref.scaled_rgb(good, s, dec)
        b, st = mjx.decode_batch(gpu_ctx, datas, scale=s)
        try:
            assert st[0] == mjx.OK and st[2] == mjx.OK and st[1] != mjx.OK, st
            _close(b.rgb(0), want, s)
            _close(b.rgb(2), want, s)
        finally:
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 8])
def test_larger_tiled_batch(mjx, orc, gpu_ctx, scale):
    datas = [mjx.synth_jpeg(3840, 2160, "420", 75, seed=40 + k) for k in range(3)]
    b = mjx.Batch(gpu_ctx, [mjx.ParsedScan(d) for d in datas], scale=scale)
    try:
        t = b.tile(22)                                            # 66 pictures
        try:
            t.decode()
            t.wait()
            assert t.unconverged_runs() == 0
            for k, d in enumerate(datas):
                _close(t.rgb(k), scaled_ref.scaled_rgb(d, scale, _oracle(orc, d)), (scale, k))
            n = len(t)
            mine = list(range(3, n))
            mx, cnt = t.compare_rgb(mine, t, [i % 3 for i in mine])
            assert int(mx.max()) == 0 and int(cnt.sum()) == 0
        finally:
            t.close()
    finally:
        b.close()

"""Every sampling layout the decoder accepts: h, v in {1, 2} for each of Y, Cb and Cr (64 layouts, up to 12 blocks per MCU), and
greyscale frames whose SOF carries a factor of 2.

The files come from tests/jpegwriter.layout_jpeg (float64 DCT of smooth waves plus noise, Annex-K Huffman tables), not from the
project's synthetic generator, so the expected values do not come from the same encoder as the decoder's usual inputs.  A layout
is named by its factors, h then v: Y21_Cb12_Cr11 is luma 2 blocks wide and 1 tall, Cb 1 wide and 2 tall, Cr 1 x 1.

CPU tests check the writer and the references (the oracle's T0 is the writer's blocks; scaled_ref at scale 1 is the oracle's
picture; Pillow, where present, is close) and mjx_validate.  GPU tests decode through the C ABI and compare with the oracle or
scaled_ref: T0 bit-exact, RGB within TOL per byte and under 1 % of bytes differing.  Every GPU test collects all the cases that
fail before it asserts, so one run names every broken layout.
"""
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegwriter as jw
import oracle_binding as orc_mod
import scaled_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1
SCALES = (2, 4, 8)
HV = [(1, 1), (2, 1), (1, 2), (2, 2)]
LAYOUTS = [list(x) for x in itertools.product(HV, repeat=3)]
# (1, 1) and (7, 5): inside one MCU; (37, 29): partial MCUs in both directions; (64, 48): whole MCUs for every layout
SIZES = [(1, 1), (7, 5), (37, 29), (64, 48), (333, 217)]
ODD_SIZES = [(1, 1), (7, 5), (37, 29), (333, 217)]
TABLES = ("split", "shared", "three")


def name(hv):
    return "Y%d%d_Cb%d%d_Cr%d%d" % tuple(f for c in hv for f in c)


def parse_name(s):
    return [(int(p[-2]), int(p[-1])) for p in s.split("_")]


NAMES = [name(hv) for hv in LAYOUTS]
# decoded at 1280 x 720 too: the 12-block MCU, both crossed layouts, luma smaller than chroma, Cb != Cr, and two named controls
LARGE = ["Y22_Cb22_Cr22", "Y21_Cb12_Cr11", "Y12_Cb21_Cr11", "Y11_Cb22_Cr22", "Y22_Cb21_Cr12", "Y21_Cb12_Cr12", "Y12_Cb21_Cr21",
         "Y22_Cb12_Cr21", "Y11_Cb21_Cr12", "Y12_Cb11_Cr22", "Y22_Cb11_Cr11", "Y21_Cb11_Cr11"]
LARGE_SIZE = (1280, 720)
GRAYS = ["gray12", "gray21", "gray22"]


@functools.lru_cache(maxsize=None)
def layout_file(lname, w, h, tables="split", restart=None, quality=75, noise=4.0):
    """(bytes, per-component blocks) of layout `lname` ("gray21": a greyscale frame with SOF factors 2, 1); the content depends
    on the layout and the size only, so the file with and without restart intervals carries the same coefficients."""
    seed = (NAMES + GRAYS).index(lname) * 1000 + w * 7 + h
    if lname.startswith("gray"):
        return jw.layout_jpeg(w, h, None, quality=quality, seed=seed, restart=restart, gray_hv=(int(lname[4]), int(lname[5])),
                              noise=noise)
    return jw.layout_jpeg(w, h, parse_name(lname), quality=quality, seed=seed, tables=tables, restart=restart, noise=noise)


def data_of(*a, **k):
    return layout_file(*a, **k)[0]


@functools.lru_cache(maxsize=None)
def oracle_std(data):
    return orc_mod.decode(data, layout=orc_mod.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)


def oracle_ref(data):
    """-> (oracle status, decoded or the panic's message) in the reference's own layout"""
    try:
        return orc_mod.OK, orc_mod.decode(data, layout=orc_mod.LAYOUT_REF)
    except orc_mod.OracleError as e:
        return e.code, str(e)


def ref_runs_past_the_scan(lname, w, h):
    """The reference reads h x v blocks per "MCU" of a greyscale frame (decoder.rs:191-201) where the scan carries one per 8 x 8
    of the picture: when the count does not divide, it decodes the scan's 1-bit padding, the EOI marker and then its own 0xAA
    padding past the end (and panics when no code matches).  The host cannot know the outcome before decoding.  The device says
    MJX_ERR_BAD_HUFFMAN where no code matches inside the scan and MJX_ERR_TRUNCATED where the scan ends first (the difference
    DESIGN s2 documents); never OK."""
    if not lname.startswith("gray"):
        return False
    f = int(lname[4]) * int(lname[5])
    nb = -(-w // 8) * -(-h // 8)
    return -(-nb // f) * f > nb


def mcux_of(lname, w):
    hmax = 1 if lname.startswith("gray") else max(h for h, _ in parse_name(lname))
    return -(-w // (8 * hmax))


def rgb_problem(got, want):
    """None when `got` is within TOL of `want` on every byte and under 1 % of bytes differ, else what is wrong"""
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    if d.size and (d.max() > TOL or (d > 0).mean() >= 0.01):
        return ("rgb", int(d.max()), round(float((d > 0).mean()), 4), np.argwhere(d > TOL)[:2].tolist())
    return None


def std_cases(tables="split"):
    """[(case name, bytes)]: every layout at every size, and the LARGE layouts at LARGE_SIZE"""
    out = [("%s_%dx%d_%s" % (n, w, h, tables), data_of(n, w, h, tables)) for n in NAMES for w, h in SIZES]
    if tables == "split":
        out += [("%s_%dx%d" % ((n,) + LARGE_SIZE), data_of(n, *LARGE_SIZE)) for n in LARGE]
    return out


# ---- CPU: the writer and the references ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", NAMES + GRAYS)
def test_writer_round_trip(orc, lname):
    """The oracle's per-component T0 is exactly what the writer quantised: every size and table mode, and one restart interval
    per size (1, 3 and one MCU row in turn, the table mode rotating as well)."""
    k = (NAMES + GRAYS).index(lname)
    for j, (w, h) in enumerate(SIZES):
        rst = [1, 3, mcux_of(lname, w)][(k + j) % 3]
        cases = [(t, None) for t in TABLES] + [(TABLES[(k + j) % 3], rst)]
        for tables, restart in cases:
            if lname.startswith("gray") and tables != "split":
                continue
            data, blocks = layout_file(lname, w, h, tables, restart)
            dec = orc.decode(data, layout=orc.LAYOUT_STD, ext_dri=restart is not None)
            assert len(dec.coefs) == len(blocks)
            for c, b in enumerate(blocks):
                assert np.array_equal(dec.coefs[c], b), (lname, w, h, tables, restart, c)


@pytest.mark.parametrize("lname", NAMES + GRAYS)
def test_reference_at_scale_1_is_the_oracle(orc, lname):
    for w, h in SIZES:
        data = data_of(lname, w, h)
        dec = oracle_std(data)
        got = scaled_ref.scaled_rgb(data, 1, dec)
        d = np.abs(got.astype(np.int32) - dec.rgb.astype(np.int32))
        assert d.max() <= 1, (lname, w, h, int(d.max()))


def test_pillow_agrees_roughly(orc):
    """Third-party sanity check: libjpeg's picture is near the oracle's (its upsampling differs, so the bound is loose).  It refuses
    the 12-block MCU, which T.81 B.2.3 forbids (at most 10 blocks) and this decoder accepts."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    import io
    checked = 0
    for n in NAMES:
        data = data_of(n, 333, 217)
        dec = oracle_std(data)
        assert dec.rgb.shape == (217, 333, 3)
        if Image is None:
            continue
        try:
            pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        except OSError:
            assert sum(h * v for h, v in parse_name(n)) > 10, n
            continue
        checked += 1
        assert np.abs(pil.astype(np.int32) - dec.rgb.astype(np.int32)).mean() < 6.0, n
    assert Image is None or checked >= 60


@pytest.mark.parametrize("lname", NAMES + GRAYS)
def test_validate(mjx, orc, lname):
    """STANDARD accepts every layout at every scale; REF_COMPAT refuses with ERR_REF_PANIC exactly where the reference panics in
    placing the blocks (most layouts with a chroma factor above luma's, or crossed factors)."""
    for w, h in SIZES:
        data = data_of(lname, w, h)
        scan = mjx.ParsedScan(data)
        try:
            for s in (1, 2, 4, 8):
                assert scan.validate(scale=s) == mjx.OK, (lname, w, h, s)
            rc, _ = oracle_ref(data)
            want = {orc.OK: mjx.OK, orc.ERR_REF_PANIC: mjx.ERR_REF_PANIC}[rc]
            if ref_runs_past_the_scan(lname, w, h):
                want = mjx.OK                   # (the decode finds it: test_ref_compat_every_layout)
            assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT) == want, (lname, w, h, rc)
        finally:
            scan.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def decode_batch(mjx, ctx, datas, **kw):
    """-> (batch, scans); the caller closes both"""
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, **kw)
    b.decode()
    b.wait()
    return b, scans


def close_all(b, scans):
    b.close()
    for s in scans:
        s.close()


def check_std(mjx, b, i, data, coefs=True):
    if b.status(i) != mjx.OK:
        return ("status", b.status(i))
    ref = oracle_std(data)
    if coefs and not np.array_equal(b.coefs(i), orc_mod.interleave(ref)):
        return ("T0",)
    return rgb_problem(b.rgb(i), ref.rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("tables", TABLES)
def test_standard_one_picture_per_batch(mjx, gpu_ctx, tables):
    bad = []
    for cname, data in std_cases(tables):
        b, scans = decode_batch(mjx, gpu_ctx, [data], keep_coefs=True)
        try:
            p = check_std(mjx, b, 0, data)
        finally:
            close_all(b, scans)
        if p:
            bad.append((cname, p))
    assert bad == [], bad


@pytest.mark.gpu
@pytest.mark.parametrize("tables", TABLES)
def test_standard_mixed_batch(mjx, gpu_ctx, tables):
    cases = std_cases(tables)
    for keep in (True, False):
        b, scans = decode_batch(mjx, gpu_ctx, [d for _, d in cases], keep_coefs=keep, chunk_images=5)
        try:
            bad = [(cn, p) for i, (cn, d) in enumerate(cases) for p in [check_std(mjx, b, i, d, coefs=keep)] if p]
        finally:
            close_all(b, scans)
        assert bad == [], (keep, bad)


@pytest.mark.gpu
def test_ref_compat_every_layout(mjx, gpu_ctx):
    """One mixed batch: per picture the oracle's status; where it decodes, T0 and RGB equal the reference layout's.  The pictures
    that panic sit between ones that do not.  A greyscale frame whose reference decode runs past its scan fails (ref_runs_past_the_scan)."""
    cases = [("%s_%dx%d" % (n, w, h), n, w, h, data_of(n, w, h)) for n in NAMES + GRAYS for w, h in SIZES]
    b, scans = decode_batch(mjx, gpu_ctx, [c[-1] for c in cases], keep_coefs=True, layout=mjx.LAYOUT_REF_COMPAT)
    bad, npanic = [], 0
    try:
        for i, (cn, n, w, h, d) in enumerate(cases):
            rc, ref = oracle_ref(d)
            want = {{orc_mod.OK: mjx.OK, orc_mod.ERR_REF_PANIC: mjx.ERR_REF_PANIC}[rc]}
            if ref_runs_past_the_scan(n, w, h):
                rc, want = -1, {mjx.ERR_BAD_HUFFMAN, mjx.ERR_TRUNCATED}
            npanic += rc == orc_mod.ERR_REF_PANIC
            if b.status(i) not in want:
                bad.append((cn, "status", b.status(i), want))
                continue
            if rc != orc_mod.OK:
                continue
            if not np.array_equal(b.coefs(i), orc_mod.interleave(ref)):
                bad.append((cn, "T0"))
                continue
            p = rgb_problem(b.rgb(i), ref.rgb)
            if p:
                bad.append((cn, p))
    finally:
        close_all(b, scans)
    assert bad == [], bad
    assert 0 < npanic < len(cases)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_scaled_every_layout(mjx, gpu_ctx, scale):
    cases = [("%s_%dx%d" % (n, w, h), data_of(n, w, h)) for n in NAMES + GRAYS for w, h in ODD_SIZES]
    cases += [("%s_%dx%d" % ((n,) + LARGE_SIZE), data_of(n, *LARGE_SIZE)) for n in LARGE]
    b, scans = decode_batch(mjx, gpu_ctx, [d for _, d in cases], scale=scale, chunk_images=9)
    bad, rgb_bytes = [], 0
    try:
        for i, (cn, d) in enumerate(cases):
            w, h, _, _ = scaled_ref.jpeg_tables(d)
            ow, oh = -(-w // scale), -(-h // scale)
            rgb_bytes += ow * oh * 3
            inf = b.info(i)
            if (inf["width"], inf["height"]) != (ow, oh):
                bad.append((cn, "info", inf, ow, oh))
                continue
            if b.status(i) != mjx.OK:
                bad.append((cn, "status", b.status(i)))
                continue
            p = rgb_problem(b.rgb(i), scaled_ref.scaled_rgb(d, scale, oracle_std(d)))
            if p:
                bad.append((cn, p))
        by = b.bytes()
    finally:
        close_all(b, scans)
    assert bad == [], bad
    assert by["rgb"] == rgb_bytes and by["pixels"] * 3 == rgb_bytes


# (child processes: one context each, a runtime switch in the environment; they write every picture they decode to an .npz and
# print the statuses and, for the profiled batches, how often each kernel ran)
_CHILD = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as ge
mjx = ge.load_package()
job = json.load(open(%(job)r))
ctx = mjx.Context(0, profiling=job['profile'])
datas = [open(p, 'rb').read() for p in job['paths']]
out, status, kernels, expands = {}, {}, {}, {}

def expandable(b, k):
    try:
        b.coefs(k)
        return True
    except mjx.MjxError:
        return False

def run(c, g, s, tag, keep=False):
    scans = [mjx.ParsedScan(datas[i]) for i in g]
    b = mjx.Batch(c, scans, scale=s, chunk_images=job['chunk'], keep_coefs=keep)
    b.kernel_ms(reset=True)
    b.decode(); b.wait()
    counts = {k: v[1] for k, v in b.kernel_ms().items()}
    for k, i in enumerate(g):
        key = '%%d_%%d_%%s' %% (i, s, tag)
        status[key] = b.status(k)
        kernels[key] = counts
        if b.status(k) == 0:
            out[key] = b.rgb(k)
            if keep:
                out['coef_' + key] = b.coefs(k)
            elif len(g) == 1:
                expands[key] = expandable(b, k)
    b.close()
    for sc in scans:
        sc.close()

for s in job['scales']:
    run(ctx, list(range(len(datas))), s, 'all')
    if job['single']:
        for i in range(len(datas)):
            run(ctx, [i], s, 'one')
if job['throughput']:
    tctx = mjx.Context(0, profiling=True, throughput_plan=True)
    for i in job['throughput']:
        run(tctx, [i], 1, 'tp', keep=True)
np.savez(job['out'], **out)
print(json.dumps(dict(status=status, kernels=kernels, expands=expands)))
"""


def run_child(tmp_path, tag, datas, scales, env_set=None, single=False, chunk=0, profile=False, throughput=()):
    """Decodes `datas` in a child process: one mixed batch per scale (key '<index>_<scale>_all'); with single, one batch per
    picture as well ('<index>_<scale>_one'); the pictures listed in throughput alone at scale 1 with their coefficients, in a
    profiled context with the throughput plan ('<index>_1_tp', 'coef_<index>_1_tp').  profile: the other batches' context is
    profiled too.  -> ({key: array}, {key: status}, {key: {kernel: launches in that key's batch}},
    {'one' key: whether mjx_batch_copy_coefs can expand the picture's coefficients, see coefs_expand})"""
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s_%d.jpg" % (tag, i))
        p.write_bytes(d)
        paths.append(str(p))
    job = tmp_path / ("%s.json" % tag)
    out = tmp_path / ("%s.npz" % tag)
    job.write_text(json.dumps(dict(paths=paths, scales=list(scales), single=single, chunk=chunk, out=str(out), profile=profile,
                                   throughput=list(throughput))))
    script = tmp_path / ("%s.py" % tag)
    script.write_text(_CHILD % dict(root=ROOT, job=str(job)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_")}
    env.update(env_set or {})
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with np.load(str(out)) as z:
        return {k: z[k] for k in z.files}, res["status"], res["kernels"], res["expands"]


def gpu_pictures(mjx, ctx, datas, scale):
    b, scans = decode_batch(mjx, ctx, datas, scale=scale)
    try:
        return [b.rgb(i) if b.status(i) == mjx.OK else ("status", b.status(i)) for i in range(len(datas))]
    finally:
        close_all(b, scans)


def same(a, b):
    return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)


def planar_direct(lname, w, scale):
    """Whether stage B reads the multi-scan twin straight from its scans (planar_ok, mjx_api.hip) rather than through the gather:
    a stage-B tile of T MCUs (kTile420 = 32 for 4:2:0 at scale 1, else tile_mcus: the largest power of two with T * bpm <= 192,
    at most 128 / hmax) touches at most two MCU rows, and the scans give at most kPlanarKinds = 4 block rows per MCU (the sum of
    the v factors), at most kPlanarSegs = 8 segments per tile."""
    hv = parse_name(lname)
    return planar_fits(hv, w, scale, sum(v for _, v in hv))


def planar_fits(hv, w, scale, kinds):
    """planar_ok's tile rule for a picture of layout hv and width w whose scans give `kinds` block rows per MCU"""
    bpm, hmax = sum(a * b for a, b in hv), max(a for a, _ in hv)
    mcux = -(-w // (8 * hmax))
    if hv == [(2, 2), (1, 1), (1, 1)] and scale == 1:
        t = 32
    else:
        t = 1
        while t * 2 * bpm <= 192:
            t *= 2
        t = min(t, 128 // hmax)
    pieces = (mcux + t - 2) // mcux + 1
    return kinds <= 4 and pieces <= 2 and pieces * kinds <= 8


TWIN_SIZES = [(37, 29), (333, 217), (1000, 40)]


def test_twins_decode_to_the_same_picture(orc):
    """noninterleaved_twin (jpegwriter.encode_scan per component): the oracle decodes the twin to the interleaved file's picture.
    (Their T0 differ in the MCU padding: a component's own scan carries only the blocks of its own grid, T.81 A.2.2.)"""
    for n in NAMES:
        for w, h in TWIN_SIZES:
            d = data_of(n, w, h)
            ref, twin = oracle_std(d), oracle_std(jw.noninterleaved_twin(d, oracle_std(d)))
            assert np.array_equal(ref.rgb, twin.rgb), (n, w, h)


def coefs_expand(mjx, b, i):
    """Without keep_coefs, mjx_batch_copy_coefs expands a multi-scan picture's coefficients from the stream the gather built for it;
    a picture that stage B read straight from its scans has no such stream and the copy fails (test_gpu_parity2.py reads the
    path the same way in test_multi_scan_pictures_read_from_their_scans_streams_equal_the_gathered_ones).  In a batch of one
    picture, whose chunk stays resident."""
    try:
        b.coefs(i)
        return True
    except mjx.MjxError:
        return False


@pytest.mark.gpu
def test_multiscan_twins(mjx, gpu_ctx, tmp_path):
    """One scan per component (T.81 A.2.2) carries the same coefficients: the picture equals the interleaved file's GPU picture bit
    for bit at every scale, alone and in a mixed batch.  Alone, stage B must read the scans directly exactly where planar_direct
    says so (at (37, 29) no twin: a tile spans more than two MCU rows; at (1000, 40) every layout with at most one v = 2
    component) and take the gather everywhere else; with MJX_PLANAR_DIRECT=0 every twin takes the gather."""
    cases = [("%s_%dx%d" % (n, w, h), n, w, data_of(n, w, h)) for n in NAMES for w, h in TWIN_SIZES]
    twins = [jw.noninterleaved_twin(c[-1], oracle_std(c[-1])) for c in cases]
    scales = (1,) + SCALES
    bad, ndirect = [], 0
    want = {s: gpu_pictures(mjx, gpu_ctx, [c[-1] for c in cases], s) for s in scales}
    for s in scales:
        for i, (cn, n, w, d) in enumerate(cases):
            if not isinstance(want[s][i], np.ndarray):
                bad.append((cn, s, "interleaved", want[s][i]))
        got = gpu_pictures(mjx, gpu_ctx, twins, s)
        bad += [(cn, s, "mixed") for i, (cn, _, _, _) in enumerate(cases) if not same(got[i], want[s][i])]
        for i, (cn, n, w, _) in enumerate(cases):
            b, scans = decode_batch(mjx, gpu_ctx, [twins[i]], scale=s)
            try:
                g = b.rgb(0) if b.status(0) == mjx.OK else None
                direct = g is not None and not coefs_expand(mjx, b, 0)
            finally:
                close_all(b, scans)
            ndirect += direct
            if direct != planar_direct(n, w, s):
                bad.append((cn, s, "direct path taken" if direct else "gather taken"))
            if not same(g, want[s][i]):
                bad.append((cn, s, "alone", "direct" if direct else "gather"))
    out, status, _, expands = run_child(tmp_path, "gather", twins, scales, {"MJX_PLANAR_DIRECT": "0"}, single=True)
    for s in scales:
        for i, (cn, _, _, _) in enumerate(cases):
            for tag in ("all", "one"):
                k = "%d_%d_%s" % (i, s, tag)
                if not same(out.get(k), want[s][i]):
                    bad.append((cn, s, "gather", tag, status[k]))
            if not expands.get("%d_%d_one" % (i, s)):
                bad.append((cn, s, "not gathered with MJX_PLANAR_DIRECT=0"))
    assert bad == [], bad
    assert ndirect >= 4 * 32, ndirect


@pytest.mark.gpu
def test_restart_intervals(mjx, gpu_ctx):
    """DRI of 1, 3 and one MCU row: T0 and RGB as the oracle's (ext_dri), and the picture of the same file without DRI bit for bit."""
    bad = []
    for w, h in [(37, 29), (333, 217)]:
        cases, plain = [], []
        for n in NAMES + ["gray22"]:
            for r in (1, 3, mcux_of(n, w)):
                cases.append(("%s_%dx%d_dri%d" % (n, w, h, r), data_of(n, w, h, restart=r)))
                plain.append(data_of(n, w, h))
        b, scans = decode_batch(mjx, gpu_ctx, [d for _, d in cases], keep_coefs=True)
        try:
            got = []
            for i, (cn, d) in enumerate(cases):
                p = check_std(mjx, b, i, d)
                if p:
                    bad.append((cn, p))
                got.append(b.rgb(i) if b.status(i) == mjx.OK else None)
        finally:
            close_all(b, scans)
        want = gpu_pictures(mjx, gpu_ctx, plain, 1)
        bad += [(cn, "vs plain") for (cn, _), g, wnt in zip(cases, got, want) if g is not None and not same(g, wnt)]
    assert bad == [], bad


@pytest.mark.gpu
def test_runtime_switches_agree(mjx, orc, tmp_path):
    """The default, MJX_SINGLE_DECODE=0 and MJX_EMIT_MIN_SUB_BITS=256 decode the same bytes, in mixed batches and one picture per
    batch.  Which entropy kernels ran is checked, not assumed: with 256 the emitting pass (k_huff_emit) runs on the small scans of
    the mixed batch, and with MJX_SINGLE_DECODE=0 it never runs.  The dense 1080p picture of a layout no named scheme has holds
    a scan of over 0.8 MB: alone, in a context with the throughput plan (the cut of a batch that fills the device; a lone picture
    otherwise gets the latency plan's short subsequences), the default takes the emitting pass on its long subsequences without
    being forced; its T0 equals the oracle's and its picture is within TOL."""
    dense = data_of("Y12_Cb21_Cr11", 1920, 1080, quality=95, noise=30.0)
    assert len(dense) >= 800_000
    datas = [data_of(n, 333, 217) for n in NAMES] + [data_of(n, 37, 29) for n in NAMES] + [dense]
    nd = len(datas) - 1
    envs = [{}, {"MJX_SINGLE_DECODE": "0"}, {"MJX_EMIT_MIN_SUB_BITS": "256"}]
    runs = [run_child(tmp_path, "sw%d" % k, datas, (1, 4), e, single=True, profile=True, throughput=[nd]) for k, e in enumerate(envs)]
    base, st0, _, _ = runs[0]
    bad = [("status", k, v) for k, v in st0.items() if v != 0]
    for (out, st, _, _), e in zip(runs[1:], envs[1:]):
        bad += [("bytes", e, k) for k in base if not same(out.get(k), base[k])]
    emit = [[kern["%d_1_tp" % nd]["huff_emit"] for _, _, kern, _ in runs], [kern["0_1_all"]["huff_emit"] for _, _, kern, _ in runs]]
    if not (emit[0][0] > 0 and emit[0][1] == 0 and emit[0][2] > 0):
        bad.append(("dense: huff_emit launches (default, SINGLE_DECODE=0, MIN_SUB_BITS=256)", emit[0]))
    if not (emit[1][1] == 0 and emit[1][2] > 0):
        bad.append(("mixed batch: huff_emit launches (default, SINGLE_DECODE=0, MIN_SUB_BITS=256)", emit[1]))
    key = "%d_1_tp" % nd
    if key in base:
        ref = oracle_std(dense)
        if not np.array_equal(base["coef_" + key], orc.interleave(ref)):
            bad.append(("dense", "T0"))
        p = rgb_problem(base[key], ref.rgb)
        if p:
            bad.append(("dense", p))
    assert bad == [], bad


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 4])
def test_tiled_mixed_layout_batch(mjx, gpu_ctx, scale):
    datas = [data_of(n, 37, 29) for n in NAMES] + [data_of(n, 333, 217) for n in LARGE]
    n = len(datas)
    b = mjx.Batch(gpu_ctx, [mjx.ParsedScan(d) for d in datas], scale=scale)
    try:
        t = b.tile(3)
        try:
            t.decode()
            t.wait()
            assert [t.status(i) for i in range(3 * n)] == [mjx.OK] * (3 * n)
            mine = list(range(n, 3 * n))
            mx, cnt = t.compare_rgb(mine, t, [i % n for i in mine])
            assert int(mx.max()) == 0 and int(cnt.sum()) == 0, [i % n for i, m in zip(mine, mx) if m]
            for i in (0, n - 1):
                assert rgb_problem(t.rgb(i), scaled_ref.scaled_rgb(datas[i], scale, oracle_std(datas[i]))) is None, i
        finally:
            t.close()
    finally:
        b.close()

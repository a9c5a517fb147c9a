"""GPU parity tests, second file (pytest -m gpu): the holes the round-1 review found.
  * 16-bit quantisation tables end to end (src/jpeg/mod.rs:245-256)
  * semantically corrupt streams: where the reference clamps instead of panicking (src/jpeg/huffman.rs:170-189) the GPU's
    coefficient stream must equal the oracle's, not merely carry an acceptable status
  * T1: per-block samples against the reference-order IDCT (src/transform.rs:55-87), within 1 LSB
  * the harness's N > 1 path on one GPU (two ranks over gloo)
Every call goes through the C ABI.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decode(mjx, ctx, datas, layout=None, **kw):
    scans = [mjx.ParsedScan(d) for d in datas]
    b = mjx.Batch(ctx, scans, keep_coefs=True, layout=mjx.LAYOUT_STANDARD if layout is None else layout, **kw)
    b.decode()
    b.wait()
    return b


# ---- 16-bit DQT ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,sub,q", [(160, 96, "420", 1), (64, 48, "444", 2), (100, 60, "422", 4), (40, 24, "gray", 1),
                                       (1920, 1080, "420", 3), (333, 217, "440", 8), (512, 512, "420", 20)])
def test_16bit_quantisation_tables(mjx, orc, gpu_ctx, w, h, sub, q):
    """Pq = 1 tables with values up to 6050 (quality 1): coefficient stream equal to the oracle's, RGB within 1 in the
    STANDARD layout and, where the reference does not panic, in its own layout."""
    data = mjx.synth_jpeg(w, h, sub, q, seed=w + q, dqt16=True)
    scan = mjx.ParsedScan(data)
    assert max(scan.desc.qt[0][k] for k in range(64)) > 255 or q >= 20
    b = _decode(mjx, gpu_ctx, [data])
    assert b.status(0) == mjx.OK
    ref = orc.decode(data, layout=orc.LAYOUT_STD)
    assert np.array_equal(b.coefs(0), orc.interleave(ref))
    assert np.abs(b.rgb(0).astype(int) - ref.rgb.astype(int)).max() <= TOL
    b.close()
    try:
        ref2 = orc.decode(data, layout=orc.LAYOUT_REF, strict_ref=True)
    except orc.OracleError:
        assert scan.validate(layout=mjx.LAYOUT_REF_COMPAT) == mjx.ERR_REF_PANIC
        return
    b2 = _decode(mjx, gpu_ctx, [data], layout=mjx.LAYOUT_REF_COMPAT)
    assert b2.status(0) == mjx.OK
    assert np.array_equal(b2.coefs(0), orc.interleave(ref2))
    assert np.abs(b2.rgb(0).astype(int) - ref2.rgb.astype(int)).max() <= TOL
    b2.close()


def test_16bit_and_8bit_tables_mixed_in_one_batch(mjx, orc, gpu_ctx):
    datas = [mjx.synth_jpeg(320, 240, "420", q, seed=q, dqt16=d16) for q, d16 in [(2, True), (75, False), (5, True), (90, False)]]
    b = _decode(mjx, gpu_ctx, datas, chunk_images=3)
    for i, d in enumerate(datas):
        ref = orc.decode(d, layout=orc.LAYOUT_STD)
        assert b.status(i) == mjx.OK and np.array_equal(b.coefs(i), orc.interleave(ref))
        assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL
    b.close()


# ---- corrupt but decodable streams ----------------------------------------------------------------------
@pytest.mark.parametrize("w,h,comps", [(48, 32, "420"), (64, 64, "444"), (40, 24, "gray"), (256, 128, "420"), (512, 512, "444")])
def test_corrupt_streams_the_reference_clamps_decode_to_the_oracles_coefficients(mjx, orc, gpu_ctx, w, h, comps):
    """Random valid codes from a table holding all 256 run/size symbols, written with no regard to block structure.  The
    reference clamps runs onto coefficient 63, cuts ZRL short and decodes `0x?0` as zeros; it does not panic, so the
    oracle returns a picture -- and then the GPU's status must be OK and its T0 stream the oracle's, in both layouts."""
    import jpegwriter as jw
    import test_host
    data, _ = test_host._corrupt_stream_file(jw, w, h, comps, seed=w + h)
    good = mjx.synth_jpeg(96, 64, "420", 75, seed=1)
    for layout, olayout in ((mjx.LAYOUT_STANDARD, orc.LAYOUT_STD), (mjx.LAYOUT_REF_COMPAT, orc.LAYOUT_REF)):
        try:
            ref = orc.decode(data, layout=olayout, strict_ref=True)
        except orc.OracleError:
            assert olayout == orc.LAYOUT_REF                         # (a geometry the reference's placement panics on)
            continue
        assert ref.bits_used < 8 * (len(data) - 200)
        b = _decode(mjx, gpu_ctx, [good, data, good], layout=layout)
        assert [b.status(i) for i in range(3)] == [mjx.OK] * 3
        assert np.array_equal(b.coefs(1), orc.interleave(ref)), (w, h, comps, layout)
        gref = orc.decode(good, layout=olayout)
        for i in (0, 2):
            assert np.abs(b.rgb(i).astype(int) - gref.rgb.astype(int)).max() <= TOL
        b.close()


@pytest.mark.parametrize("w,h,comps", [(64, 48, "420"), (128, 64, "444"), (64, 40, "gray")])
def test_corrupt_streams_with_small_values_also_match_in_rgb(mjx, orc, gpu_ctx, w, h, comps):
    """The same with value sizes <= 3 and quantisers <= 12, so that samples stay inside the 0..255 range and the +-1 LSB
    comparison of the pictures is meaningful."""
    import jpegwriter as jw
    import test_host
    data, _ = test_host._corrupt_stream_file(jw, w, h, comps, seed=3 * w + h, max_size=3, qmax=12)
    ref = orc.decode(data, layout=orc.LAYOUT_STD, strict_ref=True)
    b = _decode(mjx, gpu_ctx, [data])
    assert b.status(0) == mjx.OK and np.array_equal(b.coefs(0), orc.interleave(ref))
    d = np.abs(b.rgb(0).astype(int) - ref.rgb.astype(int))
    assert d.max() <= TOL
    assert ref.rgb.std() > 2 and (ref.rgb == 0).mean() < 0.2 and (ref.rgb == 255).mean() < 0.2      # (not a flat or saturated picture)
    b.close()


def test_stream_that_ends_early_is_reported_not_guessed(mjx, orc, gpu_ctx):
    """Cut inside the entropy-coded segment: the reference goes on decoding its 0xAA padding (huffman.rs:236-246) and
    returns a picture of garbage; the GPU path reports MJX_ERR_TRUNCATED (documented difference, DESIGN s3.1), never OK with
    different coefficients."""
    import jpegwriter as jw
    import test_host
    data, _ = test_host._corrupt_stream_file(jw, 64, 64, "444", seed=5)
    sos = data.index(b"\xff\xda")
    cut = data[:sos + 14 + 40] + b"\xff\xd9"
    ref = None
    try:
        ref = orc.decode(cut, layout=orc.LAYOUT_STD, strict_ref=True)
    except orc.OracleError:
        pass
    import damaged_ref as dr
    want = dr.decode(dr.Picture(cut))                                  # the serial decode's verdict: the scan is short
    assert want.verdict == dr.TRUNCATED
    b = _decode(mjx, gpu_ctx, [cut])
    assert b.status(0) == mjx.ERR_TRUNCATED, b.status(0)
    b.close()


# ---- T1: per-block samples vs the reference-order IDCT -----------------------------------------------------
@pytest.mark.parametrize("qt16", [False, True])
def test_T1_per_block_samples_against_the_reference_order_idct(mjx, orc, gpu_ctx, qt16):
    """Greyscale pictures built block by block from chosen coefficients: sparse random blocks, DC-only blocks whose samples
    are exact integers (where truncation flips show), single high-frequency coefficients, dense blocks.  For every block
    f32_to_u8(idct(dequant(block)) + 128) computed with the reference's own summation order and cosf per term
    (transform.rs:55-87 through orc_idct_ref) must be within 1 of the GPU's sample; R = G = B."""
    import jpegwriter as jw
    rng = np.random.default_rng(42 + qt16)
    tables = jw.tables_from_jpeg(mjx.synth_jpeg(8, 8, "gray", 75, seed=0))
    nb, bx = 1024, 32
    qmax = 2000 if qt16 else 255
    qt = rng.integers(1, qmax + 1, 64).astype(int)
    qt[0] = 8 if not qt16 else 300
    blocks = np.zeros((nb, 64), np.int64)
    for k in range(nb):
        kind = k % 4
        if kind == 0:                                           # DC only: flat block, sample = DC*q/8 + 128
            blocks[k, 0] = int(rng.integers(-1016 // qt[0], 1016 // qt[0] + 1))
        elif kind == 1:                                         # sparse
            blocks[k, 0] = int(rng.integers(-60, 60)) * 8 // max(1, qt[0] // 8)
            for p in rng.choice(np.arange(1, 64), int(rng.integers(1, 6)), replace=False):
                blocks[k, p] = int(rng.integers(-300, 301) // qt[p]) or 1
        elif kind == 2:                                         # one high-frequency coefficient
            blocks[k, int(rng.integers(32, 64))] = int(rng.choice([-1, 1])) * max(1, int(200 // qt[63]))
        else:                                                   # dense, small
            blocks[k, :] = np.where(qt < 40, rng.integers(-2, 3, 64), 0)
            blocks[k, 0] = int(rng.integers(-40, 40)) * 8 // qt[0]
    blocks = np.clip(blocks, -1023, 1023)
    data = jw.grey_jpeg_from_blocks(blocks, bx, [int(v) for v in qt], tables, qt16=qt16)
    b = _decode(mjx, gpu_ctx, [data])
    assert b.status(0) == mjx.OK
    assert np.array_equal(b.coefs(0), blocks.astype(np.int16))                      # T0: exactly the blocks written
    rgb = b.rgb(0)
    b.close()
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 0], rgb[..., 2])
    worst, flips = 0, 0
    for k in range(nb):
        nat = np.zeros(64, np.float32)
        nat[jw.ZIGZAG] = blocks[k].astype(np.float32) * qt.astype(np.float32)   # decoder.rs:230-232 + zigzag_inverse
        want = orc.idct_ref(nat, faithful_cos=True) + np.float32(128.0)
        want_u8 = np.array([[orc.f32_trunc(v) for v in row] for row in want], np.int32)
        got = rgb[(k // bx) * 8:(k // bx) * 8 + 8, (k % bx) * 8:(k % bx) * 8 + 8, 0].astype(np.int32)
        d = np.abs(got - want_u8)
        worst = max(worst, int(d.max()))
        flips += int((d > 0).sum())
    assert worst <= TOL, worst
    assert flips < 0.02 * nb * 64, flips


def test_stage_b_forms_for_sparse_and_dense_streams(mjx, orc, gpu_ctx):
    """Stage B scatters a tile's stream entries in batches cut to what the tile holds (4, 6, 8 or all prefetched words per
    lane), reads interior 4:2:0 tiles with an exchange for zero instead of zero-filling them, and takes a deeper-prefetching form
    for chunks whose streams are dense (round 4).  Pictures from nearly empty tiles (flat content, coarse quantisation) to tiles
    that overflow the prefetched words (noise at quality 98), in batches of their own -- the form is chosen per chunk -- and
    mixed; every geometry has interior and edge tiles.  T0 equal, RGB within 1 of the oracle."""
    flat = np.full((496, 1040, 3), 90, np.uint8)
    flat[200:260, 300:700] = (200, 40, 120)
    cases = [("sparse", [mjx.encode_rgb(flat, "420", 30), mjx.synth_jpeg(1040, 496, "420", 10, seed=3, noise_sigma=1.0)]),
             ("medium", [mjx.synth_jpeg(1040, 496, "420", 75, seed=4), mjx.synth_jpeg(1536, 272, "420", 60, seed=5)]),
             ("dense", [mjx.synth_jpeg(1040, 496, "420", 98, seed=6, noise_sigma=40.0), mjx.synth_jpeg(1536, 272, "420", 95, seed=7, noise_sigma=25.0)])]
    everything = [d for _, ds in cases for d in ds]
    for name, datas in cases + [("mixed", everything)]:
        b = _decode(mjx, gpu_ctx, datas)
        for i, d in enumerate(datas):
            ref = orc.decode(d, layout=orc.LAYOUT_STD)
            assert b.status(i) == mjx.OK, (name, i)
            assert np.array_equal(b.coefs(i), orc.interleave(ref)), (name, i)
            assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, (name, i)
        b.close()


def test_both_stream_layouts_decode_alike(mjx, orc):
    """The compact coefficient stream between the entropy stage and stage B has two layouts (round 4): quad-interleaved columns,
    one per subsequence (pictures of one scan), and the packed runs (multi-scan pictures; every picture with MJX_STREAM_LINEAR=1).
    The same files through both, several chunks (keep_coefs: stage B alone must find every chunk's stream again), with
    restart intervals, a multi-scan file, REF_COMPAT placement, tiles that lie inside one subsequence (flat content) and tiles that
    span more subsequences than the per-tile table of stage B holds (noise at quality 100): T0 equal to the oracle's, RGB
    within 1, and the two layouts byte for byte the same."""
    pil = os.path.join(ROOT, "tests", "golden", "pil")
    flat = np.full((272, 1536, 3), 120, np.uint8)
    datas = [mjx.synth_jpeg(1040, 496, "420", 75, seed=21), mjx.synth_jpeg(640, 480, "444", 90, seed=22),
             mjx.encode_rgb(flat, "420", 50), mjx.synth_jpeg(1536, 272, "420", 100, seed=23, noise_sigma=60.0),
             mjx.synth_jpeg(333, 217, "422", 85, seed=24), mjx.synth_jpeg(64, 48, "gray", 60, seed=25),
             open(os.path.join(pil, "dri_420_r5.jpg"), "rb").read(), open(os.path.join(pil, "ms2_420_big.jpg"), "rb").read()]
    refs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_dri=True, ext_multiscan=True) for d in datas]
    got = {}
    old = os.environ.get("MJX_STREAM_LINEAR")
    try:
        for linear in (0, 1):
            os.environ["MJX_STREAM_LINEAR"] = str(linear)
            ctx = mjx.Context(0)
            b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas], keep_coefs=True, chunk_images=3)
            b.decode(mjx.STAGE_ENTROPY)
            b.wait()
            b.decode(mjx.STAGE_PIXELS)
            b.wait()
            for i, ref in enumerate(refs):
                assert b.status(i) == mjx.OK, (linear, i)
                assert np.array_equal(b.coefs(i), orc.interleave(ref)), (linear, i)
                rgb = b.rgb(i)
                assert np.abs(rgb.astype(int) - ref.rgb.astype(int)).max() <= TOL, (linear, i)
                got[(linear, i)] = rgb.copy()
            b.close()
            b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas[:2]], layout=mjx.LAYOUT_REF_COMPAT)
            b.decode()
            b.wait()
            for i in range(2):
                assert b.status(i) == mjx.OK, (linear, i)
                got[(linear, "ref", i)] = b.rgb(i).copy()
            b.close()
            ctx.close()
    finally:
        if old is None:
            os.environ.pop("MJX_STREAM_LINEAR", None)
        else:
            os.environ["MJX_STREAM_LINEAR"] = old
    for k in [k for k in got if k[0] == 0]:
        assert np.array_equal(got[k], got[(1,) + k[1:]]), k


# ---- the harness's N > 1 path, on one GPU ------------------------------------------------------------------------------
def test_bench_two_ranks_over_gloo_on_one_gpu(tmp_path):
    """bench.py under torch.distributed.run with two ranks (both on GPU 0): the shards are decoded independently, the
    barrier and the MAX-reduce go over gloo (no RCCL anywhere), rank 0 prints one JSON line and the parity gate passes."""
    import json
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--images-per-gpu", "64", "--width", "640", "--height", "480", "--unique", "16", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and rec["parity"]["ok"] and rec["parity"]["tiled_max_abs_diff"] == 0
    assert rec["parity"]["t0_equal"] and rec["parity"]["max_abs_diff"] <= 1
    # the N > 1 line is as complete as the N = 1 line (round-4 review, next #5): the CPU baseline timed in the same run on rank 0,
    # rooflines from the MAX over the ranks of every kernel class's time, the stand-alone pass and the from-bytes leg on every rank
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["cores"] >= 1 and rec["cpu_baseline"]["kind"] == "port"
    assert 0 < rec["roofline"]["frac"] < 1 and rec["roofline"]["bound"] == "hbm"
    assert rec["kernel_rooflines"]["idct_color"]["ms_per_step"] > 0 and "roofline_isolated" in rec
    assert rec["e2e_from_bytes"]["files"] == 1024 and rec["e2e_from_bytes"]["Mpixels/s"] > 0
    assert rec["parity"]["ref_compat_max_abs_diff"] <= 1


def test_bench_line_has_a_pool_leg_at_one_gpu():
    """The N = 1 --full line times the library's own multi-GPU front (mjx_pool_decode_batch over every visible device; one here), so
    the full run on an 8-GPU node measures it without a further flag."""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--images-per-gpu", "64", "--width", "640",
           "--height", "480", "--unique", "16", "--no-cpu-baseline", "--no-traffic", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    pool = rec["e2e_from_bytes_pool"]
    assert pool["devices"] >= 1 and pool["files"] == 512 * pool["devices"] and pool["Mpixels/s"] > 0
    assert len(pool["slots"]) == pool["devices"] and all(s["ms"] > 0 and s["files"] > 0 and s["parse_threads"] >= 1 for s in pool["slots"])


def test_plain_bench_line_and_dumped_outputs(mjx, orc, tmp_path):
    """A plain run (no --full) prints the headline fields and none of the full line's legs, and --dump-outputs writes the last
    timed step's RGB at the pictures and pixels bench.dump_sample() picks: float32, each within 1 of the CPU oracle's picture."""
    import json
    import subprocess
    import bench
    w, h, n, unique = 640, 480, 64, 16
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--images-per-gpu", str(n), "--width", str(w),
           "--height", str(h), "--unique", str(unique), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "Mpixels/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["unconverged_chunk_runs"] == 0
    assert not {"parity", "cpu_baseline", "extra_configs", "e2e_from_bytes", "roofline_isolated", "host_side"} & set(rec)
    assert os.listdir(str(tmp_path / "out")) == ["rgb.npy"]
    got = np.load(str(tmp_path / "out" / "rgb.npy"))
    pics, px = bench.dump_sample(n, w * h)
    assert got.dtype == np.float32 and got.shape == (len(pics), len(px), 3) and len(px) < w * h
    datas = bench.make_inputs(mjx, w, h, "420", 75, bench.shard_seeds(0, 1, unique))
    for k, i in enumerate(pics):                       # (picture i of the tiled batch is unique picture i % unique)
        ref = orc.decode(datas[i % unique], layout=orc.LAYOUT_STD).rgb.reshape(-1, 3)[px].astype(np.float32)
        assert np.abs(got[k] - ref).max() <= TOL, i


# ---- multi-GPU front: per-device work queues, no collective -------------------------------------------------
def test_pool_shards_files_over_device_slots(mjx, orc, data_dir=None):
    """mjx_pool with two slots on the one GPU of the test box: file i goes to slot i mod 2, every slot decodes its share on
    its own context and host thread, a file that does not parse keeps its status, and every picture matches the oracle."""
    root = os.path.join(ROOT, "tests")
    names = ["lena.jpeg", "2x2-chroma.jpeg", "huff_simple0.jpg", "lena-bw.jpeg"]
    datas = [open(os.path.join(root, "data", n), "rb").read() for n in names]
    datas += [mjx.synth_jpeg(w, h, s, 75, seed=i) for i, (w, h, s) in enumerate([(640, 480, "420"), (333, 217, "444"), (1920, 1080, "420"),
                                                                                 (64, 48, "gray"), (100, 60, "422")])]
    datas += [b"not a jpeg", open(os.path.join(root, "golden", "pil", "ms2_420_big.jpg"), "rb").read(),
              open(os.path.join(root, "golden", "pil", "dri_420_r5.jpg"), "rb").read()]
    datas = datas * 3
    pool = mjx.Pool([0, 0])
    pool.set_deal(round_robin=True)
    assert len(pool) == 2 and pool.device(0) == 0 and pool.device(1) == 0 and pool.device(2) == -1
    for _ in range(2):                                                   # the queues are persistent: a second call reuses them
        res = pool.decode_batch(datas, threads_per_device=4)
        assert res.slot_of == [i % 2 for i in range(len(datas))]
        for i, d in enumerate(datas):
            try:
                ref = orc.decode(d, layout=orc.LAYOUT_STD, ext_dri=True, ext_multiscan=True)
            except orc.OracleError:
                assert res.status[i] != mjx.OK and not res.ptrs[i], i
                continue
            assert res.status[i] == mjx.OK and res.ptrs[i], (i, res.status[i])
            assert res.locate(i)[0] == i % 2
            assert np.abs(res.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, i
        res.close()
    empty = pool.decode_batch([])
    assert empty.status == []
    empty.close()
    pool.close()


def test_pool_with_eight_slots_decodes_a_scaled_down_config_5(mjx, orc):
    """BASELINE config 5 in miniature on the one GPU of the test box: 16 384 pictures, 64 unique, eight device slots (all on
    device 0).  Round robin must give file i to slot i mod 8; dealing by bytes must keep the eight queues level; every
    picture equals its unique original bit for bit (compared on the device, across the slots' batches), and four pictures of
    every slot match the oracle."""
    uniq = [mjx.synth_jpeg(128, 96, "420", 75, seed=s) for s in range(64)]
    refs = [orc.decode(d, layout=orc.LAYOUT_STD) for d in uniq]
    datas = [uniq[i % 64] for i in range(16384)]
    pool = mjx.Pool([0] * 8)
    assert len(pool) == 8
    for rr in (True, False):
        pool.set_deal(round_robin=rr)
        res = pool.decode_batch(datas, threads_per_device=2)
        assert res.rc == mjx.OK and all(s == mjx.OK for s in res.status)
        if rr:
            assert res.slot_of == [i % 8 for i in range(len(datas))]
        load = [0] * 8
        for i, s in enumerate(res.slot_of):
            load[s] += len(datas[i])
        assert max(load) <= (1.10 if rr else 1.01) * min(load), load      # (round robin: a slot sees the same 8 of the 64 sizes over and over)
        idx = list(range(64, len(datas)))
        mx, cnt = res.compare_rgb(idx, [i % 64 for i in idx])
        assert int(mx.max()) == 0 and int(cnt.sum()) == 0
        seen = {}
        for i in range(len(datas)):
            s = res.slot_of[i]
            if seen.get(s, 0) < 4:
                seen[s] = seen.get(s, 0) + 1
                assert res.locate(i)[0] == s
                assert np.abs(res.rgb(i).astype(int) - refs[i % 64].rgb.astype(int)).max() <= TOL, i
        assert len(seen) == 8
        res.close()
    pool.close()


def test_pool_over_distinct_devices(mjx, orc):
    """BASELINE config 5's sharding on real devices (round-5 review, next #8): one slot per visible GPU, all of them different
    devices -- skipped on the 1-GPU boxes, runs the first time a multi-GPU node sees the suite.  File i of a round-robin deal must
    land on device i mod N; every slot reports the parse threads it ran with (the slots share the host's processors: at most
    max(2, P / 2N) each) and the NUMA node its host thread is bound to (the node of ITS device, or -1 where the platform names
    none); every picture equals the first copy of its original bit for bit -- compared on the devices, which only works between
    pictures of one device: the originals are decoded once per device for that -- and four pictures per device match the oracle."""
    import torch
    ndev = torch.cuda.device_count()                       # (counting devices does not initialise the GPU runtime in this process)
    if ndev < 2:
        pytest.skip("one visible device: the pool's multi-device path needs two")
    P = int(mjx.lib().mjx_host_processors())
    uniq = [mjx.synth_jpeg(640 + 16 * (s % 4), 480, ("420", "422", "444")[s % 3], 75, seed=s) for s in range(16)]
    refs = [orc.decode(d, layout=orc.LAYOUT_STD) for d in uniq]
    n = 64 * ndev
    datas = [uniq[(i // ndev) % 16] for i in range(n)]     # (file i and file i + 16 N hold the same picture and land on the same device)
    pool = mjx.Pool(list(range(ndev)))
    assert len(pool) == ndev and sorted(pool.device(s) for s in range(ndev)) == list(range(ndev))
    for rr in (True, False):
        pool.set_deal(round_robin=rr)
        res = pool.decode_batch(datas)
        assert res.rc == mjx.OK and all(s == mjx.OK for s in res.status)
        if rr:
            assert res.slot_of == [i % ndev for i in range(n)]
        per_slot = [sum(1 for s in res.slot_of if s == k) for k in range(ndev)]
        assert min(per_slot) > 0, per_slot
        nodes = []
        for k in range(ndev):
            threads, node = res.host(k)
            assert 1 <= threads <= max(2, P // (2 * ndev)), (k, threads, P)
            ctx = mjx.Context(pool.device(k))
            want = int(mjx.lib().mjx_ctx_numa_node(ctx.h))
            ctx.close()
            assert node in (-1, want), (k, node, want)
            nodes.append(node)
            assert res.slot_ms(k) > 0.0
        seen = {}
        for i in range(n):
            k = res.slot_of[i]
            assert res.locate(i)[0] == k
            if seen.get(k, 0) < 4:
                seen[k] = seen.get(k, 0) + 1
                assert np.abs(res.rgb(i).astype(int) - refs[(i // ndev) % 16].rgb.astype(int)).max() <= TOL, i
        assert len(seen) == ndev
        if rr:      # same picture, same device, 16 N files apart: equal bit for bit
            idx = [i for i in range(16 * ndev, n)]
            mx, cnt = res.compare_rgb(idx, [i - 16 * ndev for i in idx])
            assert int(mx.max()) == 0 and int(cnt.sum()) == 0
        res.close()
    pool.close()


def test_pool_slot_that_fails_keeps_the_other_slots_results(mjx, orc):
    """A device that errors must not poison the others: MJX_POOL_FAULT_SLOT=3 makes slot 3 of an eight-slot pool fail its call.
    Its files report the device error and have no picture, the call returns the error, and every file of the seven other
    slots is decoded and matches the oracle."""
    datas = [mjx.synth_jpeg(160 + 16 * (i % 5), 96, ("420", "444", "422")[i % 3], 80, seed=i) for i in range(64)]
    os.environ["MJX_POOL_FAULT_SLOT"] = "3"
    try:
        pool = mjx.Pool([0] * 8)
    finally:
        del os.environ["MJX_POOL_FAULT_SLOT"]
    pool.set_deal(round_robin=True)
    res = pool.decode_batch(datas, threads_per_device=2)
    assert res.rc == mjx.ERR_DEVICE
    for i, d in enumerate(datas):
        if i % 8 == 3:
            assert res.status[i] == mjx.ERR_DEVICE and not res.ptrs[i], i
        else:
            assert res.status[i] == mjx.OK and res.ptrs[i], (i, res.status[i])
            ref = orc.decode(d, layout=orc.LAYOUT_STD)
            assert np.abs(res.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, i
    res.close()
    pool.close()


def test_pool_deals_a_skewed_list_by_bytes(mjx, orc):
    """A list whose every eighth file is a hundred times the size of the others: round robin gives all of them to slot 0;
    dealt by compressed bytes the eight queues stay level.  The pictures are right either way."""
    big = [mjx.synth_jpeg(1920, 1080, "420", 85, seed=100 + k) for k in range(4)]
    small = [mjx.synth_jpeg(96, 64, "420", 60, seed=k) for k in range(16)]
    datas = [big[(i // 8) % 4] if i % 8 == 0 else small[i % 16] for i in range(256)]
    pool = mjx.Pool([0] * 8)
    loads = {}
    for rr in (True, False):
        pool.set_deal(round_robin=rr)
        res = pool.decode_batch(datas, threads_per_device=2)
        assert res.rc == mjx.OK and all(s == mjx.OK for s in res.status)
        load = [0] * 8
        for i, s in enumerate(res.slot_of):
            load[s] += len(datas[i])
        loads[rr] = load
        for i in (0, 1, 8, 9, 255):
            ref = orc.decode(datas[i], layout=orc.LAYOUT_STD)
            assert np.abs(res.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, i
        res.close()
    pool.close()
    assert max(loads[True]) > 20 * min(loads[True])                   # round robin: slot 0 carries every large file
    assert max(loads[False]) <= 1.25 * min(loads[False]), loads[False]


def test_pool_slots_share_the_hosts_processors(mjx, orc):
    """First contact with eight GPUs on one host (round-3 review): with threads_per_device = 0 every slot used to size its
    parse threads as if it were alone (eight slots on a 16-processor quota: 64 threads).  The slots now share the budget --
    max(2, P / 2N) each, P = the processors the process may use -- so eight slots together stay within P (or at two per
    slot on a host smaller than that), a largest-first deal keeps a skewed list level even when the large files come last,
    and the pictures equal the one-slot decode of the same list bit for bit."""
    P = int(mjx.lib().mjx_host_processors())
    assert P >= 1
    big = [mjx.synth_jpeg(1280, 720, "420", 85, seed=200 + k) for k in range(8)]
    small = [mjx.synth_jpeg(96 + 8 * (k % 3), 64, ("420", "444")[k % 2], 60, seed=k) for k in range(16)]
    datas = [small[i % 16] for i in range(248)] + big                      # the eight large files at the very end of the list
    one = mjx.Pool([0])
    r1 = one.decode_batch(datas)
    assert r1.rc == mjx.OK and all(s == mjx.OK for s in r1.status)
    assert r1.host(0)[0] == max(2, P // 2)
    pool = mjx.Pool([0] * 8)
    res = pool.decode_batch(datas)                                          # threads_per_device = 0: the budgeted default
    assert res.rc == mjx.OK and all(s == mjx.OK for s in res.status)
    per_slot = [res.host(s)[0] for s in range(8)]
    assert all(t == max(2, P // 16) for t in per_slot), (per_slot, P)
    assert sum(per_slot) <= max(P, 16), (per_slot, P)
    nodes = {res.host(s)[1] for s in range(8)}
    assert len(nodes) == 1                                                  # eight slots on one GPU: one node (or none named: -1)
    load = [0] * 8
    for i, s in enumerate(res.slot_of):
        load[s] += len(datas[i])
    assert max(load) <= 1.25 * min(load), load                              # (dealt in list order the last slot would carry 8 large files' worth more)
    for i in list(range(0, 248, 31)) + list(range(248, 256)):
        assert np.array_equal(res.rgb(i), r1.rgb(i)), i
    ref = orc.decode(datas[255], layout=orc.LAYOUT_STD)
    assert np.abs(res.rgb(255).astype(int) - ref.rgb.astype(int)).max() <= TOL
    res.close(); r1.close(); pool.close(); one.close()


def test_pipelined_decode_batch_equals_the_batch_api(mjx, gpu_ctx):
    """mjx_decode_batch cuts its list into groups that are parsed, uploaded and decoded in overlap; with groups of 1 MB a list
    of 70 mixed files becomes a dozen groups.  Every picture must equal, bit for bit, what the one-batch path
    (mjx_parse + mjx_batch_create + mjx_batch_decode) gives -- compared on the device across the group batches."""
    import subprocess
    rng = np.random.default_rng(9)
    datas = []
    for i in range(70):
        w, h = int(rng.integers(8, 700)), int(rng.integers(8, 500))
        datas.append(mjx.synth_jpeg(w, h, ["420", "422", "444", "gray", "440"][i % 5], int(rng.integers(20, 98)), seed=i, dqt16=(i % 7 == 0)))
    datas[13] = b"garbage" * 10
    root = os.path.join(ROOT, "tests")
    datas[29] = open(os.path.join(root, "golden", "pil", "ms_420_big.jpg"), "rb").read()
    datas[41] = open(os.path.join(root, "golden", "pil", "dri_420_720p_rows.jpg"), "rb").read()
    os.environ["MJX_GROUP_MB"] = "1"
    try:
        grouped, st = mjx.decode_batch(gpu_ctx, datas, threads=6)
    finally:
        os.environ.pop("MJX_GROUP_MB")
    assert grouped.geometry()["chunks"] >= 3                       # several groups, each a batch of its own
    good = [i for i in range(len(datas)) if i != 13]
    assert st[13] != mjx.OK and all(st[i] == mjx.OK for i in good)
    one = mjx.Batch(gpu_ctx, [mjx.ParsedScan(datas[i]) for i in good])
    one.decode()
    one.wait()
    mx, cnt = grouped.compare_rgb(good, one, list(range(len(good))))
    assert int(mx.max()) == 0 and int(cnt.sum()) == 0
    assert grouped.status(13) != mjx.OK and len(grouped) == len(datas)
    info = grouped.info(29)
    assert (info["width"], info["height"]) == (640, 480)
    one.close()
    grouped.close()


def test_small_batches_with_short_subsequences_equal_the_long_ones(mjx, orc, tmp_path):   # (and every other runtime switch)
    """A batch too small to fill the device is cut into 256-byte subsequences (build_batch; MJX_LATENCY_NSUB=0 switches
    that off).  Both cuts must give the same coefficients and the same pixels -- checked on the sample files, restart
    intervals, a multi-scan file and the slowly synchronising picture (which then needs the in-place repair rounds) --
    and the coefficients must be the oracle's."""
    import subprocess, sys
    script = tmp_path / "cuts.py"
    script.write_text(
        "import os, sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "root = os.path.join(%r, 'tests')\n"
        "names = ['data/lena.jpeg', 'data/lena-bw.jpeg', 'data/2x2-chroma.jpeg', 'golden/pil/dri_420_720p_rows.jpg', 'golden/pil/ms_420_big.jpg',\n"
        "         'golden/pil/slow_sync_444_q99.jpg', 'golden/pil/opt_420_q85.jpg']\n"
        "datas = [open(os.path.join(root, n), 'rb').read() for n in names] + [mjx.synth_jpeg(1920, 1080, '420', 90, seed=4)]\n"
        "for i, d in enumerate(datas):\n"
        "    b = mjx.Batch(ctx, [mjx.ParsedScan(d)], keep_coefs=True)\n"
        "    b.decode(); b.wait()\n"
        "    assert b.status(0) == 0, i\n"
        "    print(i, b.geometry()['subsequences'], hashlib.sha256(b.coefs(0).tobytes()).hexdigest(), hashlib.sha256(b.rgb(0).tobytes()).hexdigest())\n"
        "    b.close()\n"
        "b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas * 3], keep_coefs=True)      # ... and as one batch of 24 (the medium cut)\n"
        "b.decode(); b.wait()\n"
        "for i in range(len(datas)):\n"
        "    j = 2 * len(datas) + i\n"
        "    assert b.status(j) == 0, j\n"
        "    print(100 + i, b.geometry()['subsequences'], hashlib.sha256(b.coefs(j).tobytes()).hexdigest(), hashlib.sha256(b.rgb(j).tobytes()).hexdigest())\n"
        "b.close()\n" % (ROOT, ROOT))
    outs = []
    switches = ("MJX_LATENCY_NSUB", "MJX_MEDIUM_NSUB", "MJX_MERGE_LOOP", "MJX_LATENCY_SUB_BITS", "MJX_DC_ONE_PASS", "MJX_STREAMS", "MJX_HOST_INTERLEAVE",
                "MJX_SINGLE_DECODE", "MJX_EMIT_MIN_SUB_BITS", "MJX_EMIT_HEAD", "MJX_EMIT_WARM_BITS", "MJX_EMIT_CP_BITS")
    base_env = {k: v for k, v in os.environ.items() if k not in switches}
    # every runtime switch of the small-batch path and of the DC prediction: the bytes must not depend on any of them
    variants = ({}, {"MJX_LATENCY_NSUB": "0", "MJX_MEDIUM_NSUB": "0"}, {"MJX_MERGE_LOOP": "0"}, {"MJX_DC_ONE_PASS": "0"},
                {"MJX_LATENCY_SUB_BITS": "1024"}, {"MJX_STREAMS": "1"},
                {"MJX_HOST_INTERLEAVE": "0"},       # (the scan pool laid out by k_scan_interleave instead of by the host: the same bytes)
                # single decode (round 5): off; for every picture of one scan, whatever its subsequences' length; the same with no
                # warm-up, a checkpoint every 256 bits and NO head room -- prefixes that grow hand their pictures to the two-pass kernels
                {"MJX_SINGLE_DECODE": "0"}, {"MJX_EMIT_MIN_SUB_BITS": "256"},
                {"MJX_EMIT_MIN_SUB_BITS": "256", "MJX_EMIT_WARM_BITS": "0", "MJX_EMIT_CP_BITS": "256", "MJX_EMIT_HEAD": "0"},
                {"MJX_LATENCY_NSUB": "0", "MJX_MEDIUM_NSUB": "0", "MJX_EMIT_WARM_BITS": "512", "MJX_EMIT_CP_BITS": "2048"})
    for env_extra in variants:
        out = subprocess.run([sys.executable, str(script)], env=dict(base_env, **env_extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, str(env_extra) + out.stdout[-2000:] + out.stderr[-2000:]
        outs.append([l.split() for l in out.stdout.strip().splitlines()])
    assert all(len(o) == 16 for o in outs)
    more = 0
    for k, other in enumerate(outs[1:]):
        for short, long_ in zip(outs[0], other):
            assert short[0] == long_[0] and short[2:] == long_[2:], (variants[k + 1], short, long_)      # same coefficients, same pixels
    for short, long_ in zip(outs[0][:8], outs[1][:8]):
        more += int(short[1]) > int(long_[1])
    assert more >= 6                                                  # ... from different cuts (tiny scans are one subsequence either way)
    assert int(outs[0][8][1]) > int(outs[1][8][1])                   # the batch of 24 as well
    for a, b2 in zip(outs[0][:8], outs[0][8:]):
        assert a[2:] == b2[2:]                                        # a picture alone = the same picture inside the batch
    # and the coefficients are the oracle's
    data = open(os.path.join(ROOT, "tests", "data", "lena.jpeg"), "rb").read()
    ref = orc.decode(data, layout=orc.LAYOUT_STD)
    import hashlib
    assert hashlib.sha256(np.ascontiguousarray(orc.interleave(ref)).tobytes()).hexdigest() == outs[0][0][2]


def test_merge_loop_that_cannot_assemble_gives_up_and_the_rounds_go_on(mjx, orc, tmp_path):
    """k_huff_merge_loop runs all merge rounds of a small chunk in one launch; its workgroups wait for one another at a
    device-wide barrier.  If they cannot all be resident (a device crowded by other processes) a workgroup gives up after a
    while, everybody leaves, and mjx_batch_wait continues with one launch per round.  MJX_LOOP_FAULT=1 makes the kernel wait
    for a workgroup that does not exist: the pictures must come out right all the same, also on the second decode of the
    same batch (the chunk has stopped using the loop by then)."""
    import subprocess, sys
    script = tmp_path / "fault.py"
    script.write_text(
        "import os, sys, time, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import __graft_entry__ as ge, oracle_binding as orc\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "root = os.path.join(%r, 'tests')\n"
        "datas = [open(os.path.join(root, n), 'rb').read() for n in ('data/lena.jpeg', 'golden/pil/slow_sync_444_q99.jpg', 'golden/pil/dri_420_720p_rows.jpg')]\n"
        "datas.append(mjx.synth_jpeg(1920, 1080, '420', 85, seed=3))\n"
        "t = time.perf_counter()\n"
        "for d in datas:\n"
        "    ref = orc.decode(d, layout=orc.LAYOUT_STD, ext_dri=True)\n"
        "    b = mjx.Batch(ctx, [mjx.ParsedScan(d)], keep_coefs=True)\n"
        "    for rep in range(2):\n"
        "        b.decode(); b.wait()\n"
        "        assert b.status(0) == 0\n"
        "        assert np.array_equal(b.coefs(0), orc.interleave(ref))\n"
        "        assert np.abs(b.rgb(0).astype(int) - ref.rgb.astype(int)).max() <= 1\n"
        "    b.close()\n"
        "print('fault ok')\n" % (ROOT, ROOT, ROOT))
    for extra in ({"MJX_LOOP_FAULT": "1"}, {"MJX_MERGE_LOOP": "0"}):
        out = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "fault ok" in out.stdout, str(extra) + out.stdout[-2000:] + out.stderr[-2000:]


def test_dc_prediction_that_never_hears_from_its_predecessor_gives_up_and_two_passes_finish(mjx, orc, tmp_path):
    """k_dc_scan_t hands the running DC sums from one workgroup to the next through memory; a workgroup waits for the segment
    before it.  Nothing promises that the one it waits for was dispatched first, so the wait is bounded: after its limit a
    workgroup gives up, says so, and mjx_batch_wait decodes the chunk again with the two-pass kernels.  MJX_DC_FAULT=1 makes
    segment 0 of a chunk's first picture keep its sums to itself: the pictures (several DC segments each, one chunk and
    several, also next to pictures that take other kernels) must come out right all the same, on the first decode and on
    the ones after it (the batch stays with two passes)."""
    import subprocess, sys
    script = tmp_path / "dcfault.py"
    script.write_text(
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import __graft_entry__ as ge, oracle_binding as orc\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "root = os.path.join(%r, 'tests')\n"
        "datas = [mjx.synth_jpeg(1920, 1080, '420', 80, seed=5), mjx.synth_jpeg(1280, 720, '444', 70, seed=6),\n"
        "         open(os.path.join(root, 'data/lena.jpeg'), 'rb').read(), mjx.synth_jpeg(2048, 1536, '420', 60, seed=7),\n"
        "         open(os.path.join(root, 'golden/pil/dri_420_720p_rows.jpg'), 'rb').read()]\n"
        "refs = [orc.decode(d, layout=orc.LAYOUT_STD, ext_dri=True) for d in datas]\n"
        "for chunk in (0, 2):\n"
        "    b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas], keep_coefs=True, chunk_images=chunk)\n"
        "    for rep in range(3):\n"
        "        b.decode(); b.wait()\n"
        "        for i, ref in enumerate(refs):\n"
        "            assert b.status(i) == 0, (chunk, rep, i, b.status(i))\n"
        "            assert np.array_equal(b.coefs(i), orc.interleave(ref)), (chunk, rep, i)\n"
        "            assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= 1, (chunk, rep, i)\n"
        "    b.close()\n"
        "print('dc fault ok')\n" % (ROOT, ROOT, ROOT))
    # (the third: one synchronisation round enqueued, so the chunks are also unconverged -- the repair path's own decode must
    # not start the one-pass kernel again and leave its "gave up" word unread, round-3 review)
    for extra in ({"MJX_DC_FAULT": "1", "MJX_TIMING": "1", "MJX_DC_ONE_PASS": "1"},      # (pinned: the suite itself may run under MJX_DC_ONE_PASS=0)
                      {"MJX_DC_FAULT": "1", "MJX_STREAMS": "1", "MJX_DC_ONE_PASS": "1"},
                      {"MJX_DC_FAULT": "1", "MJX_FIX_PASSES": "1", "MJX_DC_ONE_PASS": "1", "MJX_MERGE_LOOP": "0"}, {"MJX_DC_ONE_PASS": "0"}):
        out = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "dc fault ok" in out.stdout, str(extra) + out.stdout[-2000:] + out.stderr[-2000:]
        if "MJX_TIMING" in extra:
            assert "one-pass DC prediction gave up" in out.stderr, out.stderr[-2000:]


def test_single_decode_in_256_lane_workgroups_for_1080p_class_scans(mjx, orc):
    """Round 6 (BASELINE config 4; mjx_plan.cpp::replan_subsequences): a scan of one picture that fills ONE 256-lane workgroup with
    long subsequences takes them, and the single-decode kernels (k_huff_emit, k_huff_prefix, k_block_gather) run at the chunk's
    workgroup size -- when every picture of the batch is such a scan.  Pictures of different content and size inside the rule's
    range, alone and tiled over two chunks: the emitting kernel must have run, T0 equal to the oracle, RGB within 1, the tiled copies
    equal to their originals bit for bit.  The same list with a picture outside the range (a 720p one) must keep the two-pass kernels
    for all of them, and MJX_LONG_FIT=0 (checked in a child process) gives the old cut -- same coefficients, same pictures."""
    import subprocess
    # (throughput_plan: the cut of a batch that fills the device, which a handful of pictures otherwise never gets -- bench.py's base batch)
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    specs = [(1920, 1080, "420", 75, 6.0, 1), (1600, 1200, "420", 78, 8.0, 3), (2048, 1152, "420", 70, 6.0, 5), (1280, 960, "444", 72, 8.0, 10),
             (1440, 1080, "420", 85, 6.0, 12), (1920, 1080, "422", 70, 4.0, 14)]
    datas = []
    for (w, h, sub, q, noise, seed) in specs:
        d = mjx.synth_jpeg(w, h, sub, q, seed=seed, noise_sigma=noise)
        sc = mjx.ParsedScan(d)
        bits = sc.desc.scan_len * 8
        sc.close()
        if 256 * 8192 * 7 // 8 <= bits <= 256 * 10240:               # (inside the rule's range: 1.835 .. 2.62 Mbit)
            datas.append(d)
    assert len(datas) == 6, len(datas)
    refs = [orc.decode(d, layout=orc.LAYOUT_STD) for d in datas]

    def check(batch, n, want_emit):
        batch.kernel_ms(reset=True)
        for rep in range(2):
            batch.decode(); batch.wait()
        k = batch.kernel_ms()
        assert (k["huff_emit"][1] > 0) == want_emit, k
        assert (k["huff_write"][1] > 0) == (not want_emit), k
        for i in range(n):
            assert batch.status(i) == mjx.OK, (i, batch.status(i))
            assert np.array_equal(batch.coefs(i), orc.interleave(refs[i])), i
            assert np.abs(batch.rgb(i).astype(int) - refs[i].rgb.astype(int)).max() <= TOL, i
    b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas], keep_coefs=True)
    check(b, len(datas), True)
    t = b.tile(40)
    t.decode(); t.wait()
    n = len(datas)
    mx, cnt = t.compare_rgb(list(range(n, len(t))), t, [i % n for i in range(n, len(t))])
    assert int(mx.max()) == 0 and int(cnt.sum()) == 0 and all(t.status(i) == mjx.OK for i in range(len(t)))
    t.close()
    b.close()
    small = mjx.synth_jpeg(1280, 720, "420", 75, seed=9)
    refs.append(orc.decode(small, layout=orc.LAYOUT_STD))
    b = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas + [small]], keep_coefs=True)
    check(b, len(datas) + 1, False)                                   # (a mixed batch: the short cut and the two passes for everyone)
    b.close()
    ctx.close()
    code = ("import os, sys, hashlib\nsys.path.insert(0, %r)\nimport __graft_entry__ as ge\nmjx = ge.load_package()\nctx = mjx.Context(0, throughput_plan=True)\n"
            "d = mjx.synth_jpeg(1920, 1080, '420', 75, seed=1, noise_sigma=6.0)\nb = mjx.Batch(ctx, [mjx.ParsedScan(d)] * 3, keep_coefs=True)\n"
            "b.decode(); b.wait()\nprint(b.geometry()['subsequences'], hashlib.sha256(b.coefs(2).tobytes() + b.rgb(2).tobytes()).hexdigest())\n" % ROOT)
    outs = []
    for env_extra in ({}, {"MJX_LONG_FIT": "0"}):
        env = {k: v for k, v in os.environ.items() if k != "MJX_LONG_FIT"}
        o = subprocess.run([sys.executable, "-c", code], env=dict(env, **env_extra), capture_output=True, text=True, timeout=600)
        assert o.returncode == 0, o.stdout[-1000:] + o.stderr[-2000:]
        outs.append(o.stdout.split())
    assert outs[0][1] == outs[1][1] and int(outs[1][0]) > 1.8 * int(outs[0][0]), outs      # same result; half the subsequences with the long cut


def test_device_destuffing_fills_the_look_ahead_of_very_short_subsequences(mjx, orc, tmp_path):
    """Round-5 advisor finding: k_destuff_scatter copied a subsequence's first 64 bytes into the look-ahead rows of the column in
    front only -- complete while a subsequence is at least 64 bytes long.  With MJX_FIT_SHORT=256 (32-byte subsequences) the look-ahead
    of column s would also need bytes of s + 2, which stayed 0xAA.  The scatter now writes every column in front that covers the
    byte.  (Today's planner gives device-de-stuffed scans 512-byte subsequences whatever the knob says, so the loop is defensive; what
    this test holds is the neighbourhood: small pictures under MJX_FIT_SHORT=256 -- 32-byte subsequences where the host de-stuffs --,
    de-stuffed on the device directly, through the linear copy, and on the host, in the cut of a large batch: every coefficient the
    oracle's, RGB within 1.)"""
    import subprocess
    script = tmp_path / "short.py"
    script.write_text(
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import __graft_entry__ as ge, oracle_binding as orc\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0, throughput_plan=True)\n"
        "datas = [mjx.synth_jpeg(w, h, sub, q, seed=i) for i, (w, h, sub, q) in enumerate([(64, 64, '420', 90), (120, 80, '444', 95), (200, 150, '420', 85),\n"
        "         (96, 96, '422', 98), (33, 47, 'gray', 99), (160, 120, '420', 97)])]\n"
        "refs = [orc.decode(d, layout=orc.LAYOUT_STD) for d in datas]\n"
        "subs = []\n"
        "for dd in (True, False):\n"
        "    b = mjx.Batch(ctx, [mjx.ParsedScan(d, device_destuff=dd) for d in datas], keep_coefs=True)\n"
        "    b.decode(); b.wait()\n"
        "    subs.append(b.geometry()['subsequences'])\n"
        "    for i, ref in enumerate(refs):\n"
        "        assert b.status(i) == 0, (dd, i, b.status(i))\n"
        "        assert np.array_equal(b.coefs(i), orc.interleave(ref)), (dd, i)\n"
        "        assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= 1, (dd, i)\n"
        "    b.close()\n"
        "print('short ok', subs)\n" % (ROOT, ROOT))
    for extra in ({"MJX_FIT_SHORT": "256"}, {"MJX_FIT_SHORT": "256", "MJX_DESTUFF_DIRECT": "0"}, {}):
        env = {k: v for k, v in os.environ.items() if k not in ("MJX_FIT_SHORT", "MJX_DESTUFF_DIRECT")}
        out = subprocess.run([sys.executable, str(script)], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "short ok" in out.stdout, str(extra) + out.stdout[-2000:] + out.stderr[-3000:]


def test_single_decode_beside_restart_pictures_and_device_destuffing(mjx, orc, tmp_path):
    """Round-5 fuzz find (tests/golden/fuzz_r05): seven small files -- three with restart intervals, which keep the two-pass kernels,
    beside pictures whose first decode emits -- de-stuffed on the device.  Flat pictures' prefixes out-grew the head room, and the
    fall-back then uploaded the host's DevImages over the geometry only the device knew (lengths, restart segments): a memory fault.
    Now the flagged pictures alone leave the single-decode path, patched on the device.  With and without head room, host- and
    device-side de-stuffing: every picture OK, coefficients the oracle's, RGB within 1."""
    import glob
    import subprocess
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "fuzz_r05", "mix_*.jpg")))
    assert len(files) == 7
    script = tmp_path / "mix.py"
    script.write_text(
        "import os, sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "files = %r\n"
        "for dd in (True, False):\n"
        "    scans = [mjx.ParsedScan(open(f, 'rb').read(), device_destuff=dd) for f in files]\n"
        "    for rep in range(2):\n"
        "        b = mjx.Batch(ctx, scans, keep_coefs=True, chunk_images=11)\n"
        "        b.decode(); b.wait(); b.decode(); b.wait()\n"
        "        print(int(dd), rep, [b.status(i) for i in range(len(files))], ' '.join(hashlib.sha256(b.coefs(i).tobytes() + b.rgb(i).tobytes()).hexdigest()[:16] for i in range(len(files))))\n"
        "        b.close()\n" % (ROOT, files))
    outs = []
    # (MJX_DESTUFF_DIRECT=0: the device-side de-stuffing through a linear copy + k_scan_interleave instead of straight into the
    # lane-interleaved region)
    for env_extra in ({}, {"MJX_EMIT_HEAD": "0"}, {"MJX_SINGLE_DECODE": "0"}, {"MJX_EMIT_MIN_SUB_BITS": "256", "MJX_EMIT_HEAD": "1"},
                      {"MJX_DESTUFF_DIRECT": "0"}, {"MJX_DESTUFF_DIRECT": "0", "MJX_EMIT_MIN_SUB_BITS": "256"}):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MJX_EMIT") and k not in ("MJX_SINGLE_DECODE", "MJX_DESTUFF_DIRECT")}
        out = subprocess.run([sys.executable, str(script)], env=dict(env, **env_extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, str(env_extra) + out.stdout[-2000:] + out.stderr[-3000:]
        lines = out.stdout.strip().splitlines()
        assert len(lines) == 4 and all("[0, 0, 0, 0, 0, 0, 0]" in l for l in lines), (env_extra, lines)
        outs.append([l.split("]")[1] for l in lines])
    assert all(o == outs[0] for o in outs) and len(set(outs[0])) == 1          # the same bytes whatever the path
    ctx = mjx.Context(0)
    scans = [mjx.ParsedScan(open(f, "rb").read(), device_destuff=True) for f in files]
    b = mjx.Batch(ctx, scans, keep_coefs=True)
    b.decode(); b.wait()
    for i, f in enumerate(files):
        ref = orc.decode(open(f, "rb").read(), layout=orc.LAYOUT_STD, ext_dri=True, ext_1bit=True)
        assert b.status(i) == mjx.OK and np.array_equal(b.coefs(i), orc.interleave(ref)), f
        assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, f
    b.close()
    ctx.close()


def test_multi_scan_pictures_read_from_their_scans_streams_equal_the_gathered_ones(mjx, orc, tmp_path):
    """Round 5 (DevImage::planar): without keep_coefs stage B reads a multi-scan picture's tiles straight from the scans' streams
    -- the write pass records where a tile's segments begin instead of an offset per block -- where the geometry allows (two MCU
    rows per tile at most, eight segments); other pictures, and every picture of a keep_coefs batch, go through the gather kernels.
    Twins of synthetic pictures in both scan forms, with restart intervals, odd MCU rows, 4:4:4 / 4:2:2 / 4:2:0, one picture too
    narrow for the direct path; tiled over several chunks.  The same bytes with MJX_PLANAR_DIRECT=0, the source's picture bit for
    bit, and the oracle's within 1."""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_multiscan
    cases = [((1936, 1088, "420", 75, 1), {}), ((1936, 1088, "420", 75, 1), {"chroma_together": True}), ((1000, 600, "420", 85, 2), {"restart": 50}),
             ((520, 264, "444", 60, 3), {}), ((1333, 217, "422", 80, 4), {"chroma_together": True}), ((40, 300, "420", 75, 5), {}),
             ((1024, 96, "420", 90, 6), {"restart": 64, "chroma_together": True})]
    srcs, twins = [], []
    for (w, h, sub, q, seed), kw in cases:
        srcs.append(mjx.synth_jpeg(w, h, sub, q, seed=seed))
        twins.append(make_multiscan.twin(srcs[-1], **kw))
    for i, d in enumerate(srcs + twins):
        (tmp_path / ("f%02d.jpg" % i)).write_bytes(d)
    n = len(cases)
    script = tmp_path / "planar.py"
    script.write_text(
        "import os, sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "files = [open(os.path.join(%r, 'f%%02d.jpg' %% i), 'rb').read() for i in range(%d)]\n"
        "scans = [mjx.ParsedScan(d) for d in files]\n"
        "for chunk in (0, 3):\n"
        "    base = mjx.Batch(ctx, scans, chunk_images=chunk)\n"
        "    b = base.tile(3)\n"
        "    b.decode(); b.wait(); b.decode(); b.wait()\n"
        "    st = [b.status(i) for i in range(len(b))]\n"
        "    direct = []\n"
        "    for i in range(%d, %d):\n"
        "        try:\n"
        "            b.coefs(len(b) - %d + i); direct.append(0)\n"
        "        except Exception:\n"
        "            direct.append(1)\n"
        "    print(chunk, sum(st), ''.join(map(str, direct)), ' '.join(hashlib.sha256(b.rgb(i).tobytes()).hexdigest()[:16] for i in range(len(b))))\n"
        "    b.close(); base.close()\n" % (ROOT, str(tmp_path), 2 * n, n, 2 * n, 2 * n))
    outs = {}
    for name, extra in (("direct", {}), ("gather", {"MJX_PLANAR_DIRECT": "0"})):
        env = {k: v for k, v in os.environ.items() if k != "MJX_PLANAR_DIRECT"}
        out = subprocess.run([sys.executable, str(script)], env=dict(env, **extra), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, name + out.stdout[-2000:] + out.stderr[-3000:]
        outs[name] = [l.split() for l in out.stdout.strip().splitlines()]
    for name, lines in outs.items():
        assert len(lines) == 2 and all(l[1] == "0" for l in lines), (name, lines)                  # every status OK
        for l in lines:
            h = l[3:]
            assert len(h) == 6 * n
            for rep in range(3):
                for k in range(n):
                    assert h[rep * 2 * n + n + k] == h[k] == h[rep * 2 * n + k], (name, l[0], rep, k)      # the twin's picture = its source's, every copy
    # which pictures took the direct path (the last copy's chunk is resident: their coefficients cannot be expanded): all but the
    # 40-pixel-wide one, whose tiles touch eleven MCU rows; none with MJX_PLANAR_DIRECT=0
    # (first line: one chunk; in the second the last copies' chunk holds only some of them, and the rest cannot be expanded anyway)
    assert outs["direct"][0][2] == "1111101", outs["direct"][0][:3]
    assert outs["gather"][0][2] == "0000000", outs["gather"][0][:3]
    assert [l[3:] for l in outs["direct"]] == [l[3:] for l in outs["gather"]]
    ctx = mjx.Context(0)
    scans = [mjx.ParsedScan(d) for d in twins]
    for keep in (False, True):
        b = mjx.Batch(ctx, scans, keep_coefs=keep)
        b.decode(); b.wait()
        for k, (src, tw) in enumerate(zip(srcs, twins)):
            ref = orc.decode(src, layout=orc.LAYOUT_STD)
            assert b.status(k) == mjx.OK and np.abs(b.rgb(k).astype(int) - ref.rgb.astype(int)).max() <= TOL, (keep, k)
            if keep:
                ref_ms = orc.decode(tw, layout=orc.LAYOUT_STD, ext_dri=True, ext_multiscan=True)
                assert np.array_equal(b.coefs(k), orc.interleave(ref_ms)), k
        b.close()
    ctx.close()


def test_runs_that_did_not_converge_in_time_are_counted(mjx, orc, tmp_path):
    """mjx_batch_unconverged_runs (round 5): several decodes enqueued before one wait -- bench.py's timed region -- are only whole
    work if every chunk's synchronisation rounds had converged when the kernels behind them ran; mjx_batch_wait repairs the last
    decode only.  With one round enqueued up front (MJX_FIX_PASSES=1) a batch of noisy pictures does not converge: the count goes
    up by one per decode and chunk until a wait has repaired the batch once -- the chunks remember what they needed --, the picture
    after the wait is right.  With the default rounds the count stays 0."""
    import subprocess
    script = tmp_path / "unconv.py"
    script.write_text(
        "import os, sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0, throughput_plan=True)\n"
        "datas = [mjx.synth_jpeg(1920, 1080, '420', 90, seed=s, noise_sigma=12.0) for s in range(4)]\n"
        "base = mjx.Batch(ctx, [mjx.ParsedScan(d) for d in datas])\n"
        "b = base.tile(64)\n"
        "for _ in range(3): b.decode()\n"
        "b.wait()\n"
        "u0 = b.unconverged_runs()\n"
        "for _ in range(2): b.decode()\n"
        "b.wait()\n"
        "print(u0, b.unconverged_runs(), b.geometry()['chunks'], sum(b.status(i) for i in range(len(b))), hashlib.sha256(b.rgb(len(b) - 1).tobytes()).hexdigest()[:16])\n" % ROOT)
    res = {}
    for name, extra in (("default", {}), ("one_round", {"MJX_FIX_PASSES": "1", "MJX_MERGE_LOOP": "0"})):
        env = {k: v for k, v in os.environ.items() if k not in ("MJX_FIX_PASSES", "MJX_MERGE_LOOP")}
        out = subprocess.run([sys.executable, str(script)], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, name + out.stdout[-2000:] + out.stderr[-3000:]
        res[name] = out.stdout.strip().split()
    assert res["default"][:2] == ["0", "0"] and res["default"][3] == "0", res
    # three decodes before the first wait: none of them whole; the wait's repair tells the chunks how many rounds they need
    # (Chunk::learned_passes), and the decodes after it are
    u0, u1, chunks, bad, _ = res["one_round"]
    assert int(u0) == 3 * int(chunks) and u1 == u0 and bad == "0", res
    assert res["one_round"][4] == res["default"][4]                      # the repaired picture = the picture


def test_small_pictures_in_a_large_batch_are_cut_to_fill_their_workgroup(mjx, orc, gpu_ctx):
    """replan_subsequences (round 5): a scan under three quarters of a workgroup's worth of 512-byte subsequences is cut shorter,
    so that its one workgroup is full (16384 x 512x512: 208 -> 323 Gpixels/s).  Geometry, T0 and RGB of such a batch."""
    if os.environ.get("MJX_FIT_SHORT") == "0":
        pytest.skip("the rule is switched off (A/B run)")
    datas = [mjx.synth_jpeg(512, 512, "420", 75, seed=s) for s in range(3)] + [mjx.synth_jpeg(256, 256, "444", 75, seed=7)]
    scans = [mjx.ParsedScan(d) for d in datas]
    ctx = mjx.Context(0, throughput_plan=True)
    b = mjx.Batch(ctx, scans, keep_coefs=True)
    geo = b.geometry()
    per_picture = geo["subsequences"] / len(datas)
    assert 90 <= per_picture <= 256, geo           # (at 512 bytes per subsequence: ~50 per 512x512 picture; now ~110: 128 lanes' worth, 1024 bits at least)
    b.decode(); b.wait()
    for i, d in enumerate(datas):
        ref = orc.decode(d, layout=orc.LAYOUT_STD)
        assert b.status(i) == mjx.OK and np.array_equal(b.coefs(i), orc.interleave(ref)), i
        assert np.abs(b.rgb(i).astype(int) - ref.rgb.astype(int)).max() <= TOL, i
    b.close()
    ctx.close()


def test_multi_scan_picture_whose_tiles_are_one_mcu_longer_than_its_rows(mjx, orc, gpu_ctx):
    """Round-5 fuzz find (tests/golden/fuzz_r05b/ms_482x638.jpg, three scans, 31 MCUs per row, tiles of 32): walking from tile to
    tile, the stage-B form that reads the scans' streams advanced the tile's first column by 32 and wrapped once -- from the row's
    last column that is two rows on, and tile 31 read one MCU from the wrong row.  Only workgroups that walk several tiles do
    that: 64 copies, against the gathered decode of the same batch and the oracle."""
    d = open(os.path.join(ROOT, "tests", "golden", "fuzz_r05b", "ms_482x638.jpg"), "rb").read()
    ref = orc.decode(d, layout=orc.LAYOUT_STD, ext_multiscan=True)
    rgbs = []
    for keep in (True, False):
        base = mjx.Batch(gpu_ctx, [mjx.ParsedScan(d)], keep_coefs=keep)
        b = base.tile(64)
        b.decode(); b.wait()
        assert all(b.status(i) == mjx.OK for i in range(len(b)))
        rgbs.append([b.rgb(i) for i in (0, 31, 63)])
        b.close(); base.close()
    for x in rgbs[0] + rgbs[1]:
        assert np.array_equal(x, rgbs[0][0])
    assert np.abs(rgbs[0][0].astype(int) - ref.rgb.astype(int)).max() <= TOL


def test_flat_content_is_exact_and_is_not_decoded_lane_by_lane(mjx, orc, tmp_path):
    """Round 5 (Gen2, mjx_kernels.hip): runs of identical flat MCUs are periodic bit strings; a decode that enters one out of phase
    stays on a self-consistent wrong parse, and the subsequences inside were put right one per synchronisation round, each decoded in
    full again (a two-tone 4K page: 104 ms).  With two recorded decodes per subsequence the truth meets the first decode at its first
    checkpoint and remembered exits cross a workgroup per round (1.5 ms).  Flat pictures of several kinds, alone and tiled: T0 equal to
    the oracle, RGB within 1, the same bytes with MJX_MERGE_MEMO=0 -- and, loosely, not slower than that by more than a half."""
    import subprocess
    # (the pictures are fixtures since round 6 -- tests/golden/flat_r06/, written by make_flat.py there with Pillow: two flat halves, a
    # white page with noisy lines, flat 4:4:4 tiles, a grey page with a dark square -- so the test never skips for want of Pillow)
    pics = [open(os.path.join(ROOT, "tests", "golden", "flat_r06", "flat%d.jpg" % i), "rb").read() for i in range(4)]
    for i, d in enumerate(pics):
        (tmp_path / ("flat%d.jpg" % i)).write_bytes(d)
    script = tmp_path / "flat.py"
    script.write_text(
        "import os, sys, time, hashlib\n"
        "sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "mjx = ge.load_package()\n"
        "ctx = mjx.Context(0)\n"
        "files = [open(os.path.join(%r, 'flat%%d.jpg' %% i), 'rb').read() for i in range(%d)]\n"
        "out, el = [], 0.0\n"
        "for d in files:\n"
        "    for copies in (1, 24):\n"
        "        base = mjx.Batch(ctx, [mjx.ParsedScan(d)], keep_coefs=copies == 1)\n"
        "        b = base.tile(copies) if copies > 1 else base\n"
        "        b.decode(); b.wait()\n"
        "        t = time.perf_counter(); b.decode(); b.wait(); el += time.perf_counter() - t\n"
        "        assert all(b.status(i) == 0 for i in range(len(b)))\n"
        "        out.append(hashlib.sha256(b.rgb(len(b) - 1).tobytes() + (b.coefs(0).tobytes() if copies == 1 else b'')).hexdigest()[:16])\n"
        "        b.close()\n"
        "        if b is not base: base.close()\n"
        "print(' '.join(out), '%%.3f' %% (el * 1e3))\n" % (ROOT, str(tmp_path), len(pics)))
    res = {}
    for name, extra in (("two", {}), ("one", {"MJX_MERGE_MEMO": "0"})):
        env = {k: v for k, v in os.environ.items() if k != "MJX_MERGE_MEMO"}
        o = subprocess.run([sys.executable, str(script)], env=dict(env, **extra), capture_output=True, text=True, timeout=900)
        assert o.returncode == 0, name + o.stdout[-2000:] + o.stderr[-3000:]
        res[name] = o.stdout.strip().split()
    assert res["two"][:-1] == res["one"][:-1], res
    assert float(res["two"][-1]) < 1.5 * float(res["one"][-1]) + 1.0, res          # (measured: 6 ms against 45)
    ctx = mjx.Context(0)
    for d in pics:
        ref = orc.decode(d, layout=orc.LAYOUT_STD)
        b = mjx.Batch(ctx, [mjx.ParsedScan(d)], keep_coefs=True)
        b.decode(); b.wait()
        assert b.status(0) == mjx.OK and np.array_equal(b.coefs(0), orc.interleave(ref))
        assert np.abs(b.rgb(0).astype(int) - ref.rgb.astype(int)).max() <= TOL
        b.close()
    ctx.close()

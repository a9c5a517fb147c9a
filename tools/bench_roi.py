#!/usr/bin/env python3
"""Region-of-interest decode (mjx_opts.rois) against the full-picture decode, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures per GPU, 64 unique ones tiled on the device -- decoded
  full      without a rectangle
  c1920     the centre 1920 x 1080
  c960      the centre 960 x 540
  r224      224 x 224 at a seeded random place per unique picture
  half      at 1/2 scale without a rectangle
  half_roi  at 1/2 scale with the rectangle 0, 0, 1920, 1080 -- the whole 1/2-scale picture through the cropped form: what the
            form itself costs against `half`
A base batch of the unique pictures is built once per variant; every repeat tiles it to the full batch, runs the warm-up and
`--steps` timed steps, and frees it again, so only one large batch is resident at a time.  The variants take turns inside every
repeat (their order rotates), so that a drift of the box does not show up as a difference between them.

Per variant: ms per step (best and median over the repeats), the per-class kernel ms per step from mjx_batch_kernel_ms
(idct_color is stage B), the RGB bytes of the batch, the tiles stage B reads of the picture's tiles (mjx_plan_tiles, summed over
the unique pictures) and the device memory the batch's arena took when it was built (free device memory before and after, from the
HIP runtime; 0 where the context handed the batch a cached block of an earlier, larger batch instead of allocating).
Every timed region must have converged and every picture must have decoded.  One JSON object on the last line.

    python tools/bench_roi.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--variants full,c1920,...]

Stage B's kernel time on its own comes from a separate run under `rocprofv3 --kernel-trace --stats` with one variant.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_device_bytes(mjx):
    hip = mjx.lib()                      # (the HIP runtime the library is linked against, through the library's own handle)
    hip.hipMemGetInfo.restype = ctypes.c_int
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t)] * 2
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    return free.value if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0 else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--variants", default="full,c1920,c960,r224,half,half_roi")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    threads = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    W, H = args.width, args.height
    rng = np.random.RandomState(224)
    side = min(224, W, H)
    table = {
        "full": (1, None),
        "c1920": (1, (W // 4, H // 4, W // 2, H // 2)),
        "c960": (1, (3 * W // 8, 3 * H // 8, W // 4, H // 4)),
        "r224": (1, [(int(rng.randint(0, W - side + 1)), int(rng.randint(0, H - side + 1)), side, side) for _ in range(args.unique)]),
        "half": (2, None),
        "half_roi": (2, (0, 0, -(-W // 2), -(-H // 2))),
    }
    names = [v for v in args.variants.split(",") if v]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)      # (as bench.py: cut like the batch the base becomes)
    bases, tiles = {}, {}
    for v in names:
        scale, rois = table[v]
        scans = [mjx.ParsedScan(d) for d in datas]
        bases[v] = mjx.Batch(ctx, scans, scale=scale, rois=rois)
        assert all(x == mjx.OK for x in bases[v].create_status), bases[v].create_status
        rd = tot = 0
        for k, sc in enumerate(scans):
            r = None if rois is None else rois[k] if isinstance(rois, list) else rois
            p = sc.plan_tiles(roi=r, scale=scale)
            rd += p["tiles_read"]
            tot += p["tiles_total"]
            sc.close()
        tiles[v] = (rd, tot)
    runs = {v: [] for v in names}
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        for v in order:
            free0 = free_device_bytes(mjx)
            b = bases[v].tile(reps)
            arena = max(0, free0 - free_device_bytes(mjx))
            try:
                for _ in range(args.warmup):
                    b.decode()
                    b.wait()
                b.kernel_ms(reset=True)
                u0 = b.unconverged_runs()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    b.decode()
                b.wait()
                ms = 1e3 * (time.perf_counter() - t0) / args.steps
                assert b.unconverged_runs() == u0, "a timed region had not converged (%s)" % v
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed (%s): %s" % (v, bad[:8])
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                by = b.bytes()
                runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "rgb_bytes": by["rgb"], "arena_bytes": arena})
                print("%-8s repeat %d: %.3f ms per step, stage B %.3f ms" % (v, r, ms, kms.get("idct_color", 0.0)), flush=True)
            finally:
                b.close()
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (W, H, args.quality), "steps": args.steps,
           "repeats": args.repeats, "variants": {}}
    for v in names:
        best = min(runs[v], key=lambda x: x["ms_per_step"])
        out["variants"][v] = {"scale": table[v][0], "ms_per_step_best": best["ms_per_step"],
                              "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                              "kernel_ms_per_step": best["kernel_ms_per_step"],
                              "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                              "rgb_bytes": best["rgb_bytes"], "tiles_read": tiles[v][0] * reps, "tiles_total": tiles[v][1] * reps,
                              "tile_share": round(tiles[v][0] / max(tiles[v][1], 1), 4),
                              "arena_bytes": max(x["arena_bytes"] for x in runs[v]),
                              "all_ms_per_step": [x["ms_per_step"] for x in runs[v]]}
    for b in bases.values():
        b.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

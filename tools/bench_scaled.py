#!/usr/bin/env python3
"""Scaled decode (mjx_opts.scale_denom) against the full-size decode, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures per GPU, 64 unique ones tiled on the device -- decoded at
1, 1/2, 1/4 and 1/8.  A base batch of the unique pictures is built once per scale; every repeat tiles it to the full batch,
runs the warm-up and `--steps` timed steps, and frees it again, so only one large batch is resident at a time.  The scales
take turns inside every repeat (their order rotates), so that a drift of the box does not show up as a difference between them.

Per scale: ms per step (best and median over the repeats), Gpixels/s of SOURCE pixels, and the per-class kernel ms per step from
mjx_batch_kernel_ms (idct_color is stage B: k_idct_color, or k_dc_color at 1/8).  Every timed region must have converged
(mjx_batch_unconverged_runs unchanged) and every picture must have decoded.  One JSON object on the last line.

    python tools/bench_scaled.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--scales", default="1,2,4,8")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    threads = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    scales = [int(s) for s in args.scales.split(",")]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)      # (as bench.py: cut like the batch the base becomes)
    bases = {}
    for s in scales:
        scans = [mjx.ParsedScan(d) for d in datas]
        bases[s] = mjx.Batch(ctx, scans, scale=s)
        assert all(x == mjx.OK for x in bases[s].create_status), bases[s].create_status
        for sc in scans:
            sc.close()
    runs = {s: [] for s in scales}
    for r in range(args.repeats):
        order = scales[r % len(scales):] + scales[:r % len(scales)]
        for s in order:
            b = bases[s].tile(reps)
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
                assert b.unconverged_runs() == u0, "a timed region had not converged (scale %d)" % s
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed at scale %d: %s" % (s, bad[:8])
                kms = {k: round(v[0] / args.steps, 4) for k, v in b.kernel_ms(reset=True).items() if v[1]}
                by = b.bytes()
                runs[s].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "rgb_bytes": by["rgb"], "out_pixels": by["pixels"]})
                print("scale 1/%d  repeat %d: %.3f ms per step, stage B %.3f ms" % (s, r, ms, kms.get("idct_color", 0.0)), flush=True)
            finally:
                b.close()
    src_pixels = n * args.width * args.height
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (args.width, args.height, args.quality),
           "steps": args.steps, "repeats": args.repeats, "scales": {}}
    for s in scales:
        best = min(runs[s], key=lambda x: x["ms_per_step"])
        med = statistics.median(x["ms_per_step"] for x in runs[s])
        out["scales"][str(s)] = {"ms_per_step_best": best["ms_per_step"], "ms_per_step_median": round(med, 4),
                                 "source_gpixels_per_s": round(src_pixels / (best["ms_per_step"] * 1e-3) / 1e9, 2),
                                 "kernel_ms_per_step": best["kernel_ms_per_step"], "rgb_bytes": best["rgb_bytes"],
                                 "out_pixels": best["out_pixels"], "all_ms_per_step": [x["ms_per_step"] for x in runs[s]]}
    for b in bases.values():
        b.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Luminance output (MJX_OUTPUT_CHANNELS = 1) against packed RGB, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures, 64 unique ones -- decoded whole at scales 1, 1/2 and 1/8 as
  rgb       packed R,G,B without an output description: the parent's path, the yardstick of the same run
  luma_u8   luminance, uint8 (k_idct_color's kSinkLuma forms, k_dc_color_luma at 1/8)
  luma_f32  luminance, float32 normalised
Every variant builds a base batch of the unique pictures once and tiles it per repeat (only one large batch is resident at a
time); the variants take turns inside every repeat.  Per variant: ms per step (every repeat, best, median), per-class kernel ms per
step (idct_color is stage B) and the bytes written.  One JSON object on the last line.

    python tools/bench_luma.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--scales 1,2,8] [--variants rgb,luma_u8,luma_f32]
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
    ap.add_argument("--scales", default="1,2,8")
    ap.add_argument("--variants", default="rgb,luma_u8,luma_f32")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    outputs = {"rgb": lambda: None, "luma_u8": lambda: mjx.Output("uint8", channels=1),
               "luma_f32": lambda: mjx.Output("float32", channels=1, mean=0.449, std=0.226)}
    names = [(v, int(s)) for s in args.scales.split(",") if s for v in args.variants.split(",") if v]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    scans = [mjx.ParsedScan(d) for d in datas]
    bases = {}
    for v, s in names:
        bases[(v, s)] = mjx.Batch(ctx, scans, scale=s, output=outputs[v]())
        assert all(x == mjx.OK for x in bases[(v, s)].create_status), bases[(v, s)].create_status
    runs = {k: [] for k in names}
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        for key in order:
            b = bases[key].tile(reps)
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
                assert b.unconverged_runs() == u0, "a timed region had not converged (%s)" % (key,)
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed (%s): %s" % (key, bad[:8])
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                runs[key].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "bytes_written": b.bytes()["rgb"]})
                print("%-9s 1/%d repeat %d: %.3f ms per step, stage B %.3f ms" % (key[0], key[1], r, ms, kms.get("idct_color", 0.0)), flush=True)
            finally:
                b.close()
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (args.width, args.height, args.quality), "steps": args.steps,
           "repeats": args.repeats, "variants": {}}
    for key in names:
        best = min(runs[key], key=lambda x: x["ms_per_step"])
        out["variants"]["%s_s%d" % key] = {"scale": key[1], "ms_per_step_best": best["ms_per_step"],
                                           "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[key]), 4),
                                           "all_ms_per_step": [x["ms_per_step"] for x in runs[key]],
                                           "kernel_ms_per_step": best["kernel_ms_per_step"],
                                           "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[key]],
                                           "bytes_written": best["bytes_written"]}
    for b in bases.values():
        b.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

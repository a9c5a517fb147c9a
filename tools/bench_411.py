#!/usr/bin/env python3
"""4:1:1 and 4:1:0 beside their 4:2:0 and 4:2:2 twins of the same content, one process.

Per size (3840x2160 and 1920x1080) the same synthetic pictures -- the generator's content depends on the seed alone -- are encoded
four ways at q75:
  411   Y 4x1: 6 blocks per MCU, the blocks per pixel of 4:2:0, stage B's generic form (32 x 8 MCUs, 32 per tile)
  410   Y 4x2: 10 blocks per MCU, 1.25 samples per pixel, the generic form (32 x 16 MCUs, 16 per tile)
  420   Y 2x2: stage B's dedicated form -- not the fair neighbour, the headline's
  422   Y 2x1: the generic form at 4 blocks per MCU -- the fair neighbour
Every variant builds a base batch of the unique pictures once and tiles it per repeat (only one large batch is resident at a
time); the variants take turns inside every repeat.  Per variant: ms per step (every repeat, best, median), per-class kernel ms per
step (idct_color is stage B), the scan bytes, and the timed steps that did not do the whole work (must be 0).  One JSON object on
the last line, and in --out (default profiles/bench_411.json).

    python tools/bench_411.py [--steps 5] [--warmup 1] [--repeats 3] [--images 512] [--sizes 3840x2160,1920x1080] [--modes 411,410,420,422]
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
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--modes", default="411,410,420,422")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_411.json"))
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",") if s]
    names = [(m, w, h) for w, h in sizes for m in args.modes.split(",") if m]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    bases, scans, scan_bytes = {}, {}, {}
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        for key in names:
            m, w, h = key
            datas = list(ex.map(lambda s: mjx.synth_jpeg(w, h, m, args.quality, s), range(args.unique)))
            scans[key] = [mjx.ParsedScan(d) for d in datas]
            scan_bytes[key] = sum(len(d) for d in datas) * reps
            bases[key] = mjx.Batch(ctx, scans[key])
            assert all(x == mjx.OK for x in bases[key].create_status), (key, bases[key].create_status)
    runs = {k: [] for k in names}
    unconverged = 0
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
                unconverged += b.unconverged_runs() - u0
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed (%s): %s" % (key, bad[:8])
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                runs[key].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms})
                print("%s %dx%d repeat %d: %.3f ms per step, stage B %.3f ms" % (key + (r, ms, kms.get("idct_color", 0.0))), flush=True)
            finally:
                b.close()
    out = {"images": n, "unique": args.unique, "quality": args.quality, "steps": args.steps, "repeats": args.repeats,
           "unconverged_runs": unconverged, "variants": {}}
    for key in names:
        m, w, h = key
        best = min(runs[key], key=lambda x: x["ms_per_step"])
        out["variants"]["%s_%dx%d" % key] = {"mode": m, "width": w, "height": h, "ms_per_step_best": best["ms_per_step"],
                                             "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[key]), 4),
                                             "all_ms_per_step": [x["ms_per_step"] for x in runs[key]],
                                             "gpixels_per_s_best": round(n * w * h / best["ms_per_step"] / 1e6, 3),
                                             "kernel_ms_per_step": best["kernel_ms_per_step"],
                                             "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[key]],
                                             "scan_bytes": scan_bytes[key]}
    for key in names:
        bases[key].close()
        for s in scans[key]:
            s.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert unconverged == 0, "%d timed steps did not do the whole work" % unconverged


if __name__ == "__main__":
    main()

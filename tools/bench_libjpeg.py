#!/usr/bin/env python3
"""libjpeg's pixels (mjx_opts.pixels = MJX_PIXELS_LIBJPEG) against the default pixels, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures, 64 unique ones -- decoded whole, packed RGB
  reference   the default pixels: stage B converts and stores the picture itself (the parent's path, measured in the same run)
  libjpeg     stage B stores component planes (about 1.5 bytes per pixel written and read again), k_upsample_color makes the picture
  libjpeg-exact  (--islow) the same with libjpeg's integer slow inverse DCT in stage B (MJX_OPTS_IDCT = MJX_IDCT_ISLOW): the price of
              byte-exact libjpeg pixels, against the float variant of the same run
  --scale S [S ...]  instead: the exact pixels at full size and at every scale S (2, 4, 8: libjpeg's reduced integer transforms in stage B,
              k_upsample_red behind it) and, in the same run, the default pixels at full size and at the same scales (DESIGN.md s14's
              scaled decode), all taking turns
All build a base batch of the unique pictures once and tile it per repeat (only one large batch is resident at a time); the variants
take turns inside every repeat and the figure is the best of the repeats.

Per variant: ms per step (every repeat, best, median), per-class kernel ms per step -- idct_color is stage B, resize the class of the
passes behind it, here k_upsample_color alone (k_upsample_red at a scale) --, the bytes written and the device memory the batch took when it was built.
One JSON object on the last line.

    python tools/bench_libjpeg.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--islow] [--scale 2 4 8]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def upsample_kernel(variant):
    """the kernel behind stage B that the `resize` class times for this variant"""
    if not variant.startswith("libjpeg"):
        return "(no pass)"
    return "k_upsample_red" if "/" in variant else "k_upsample_color"


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
    ap.add_argument("--islow", action="store_true", help="a third variant: libjpeg's pixels with its integer slow inverse DCT")
    ap.add_argument("--scale", type=int, nargs="+", choices=[2, 4, 8], default=[],
                    help="the exact pixels and the default pixels at full size and at these scales, in place of the variants above")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from bench_output import free_device_bytes
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    names = ["reference", "libjpeg"] + (["libjpeg-exact"] if args.islow else [])
    opts = {v: dict(pixels=v) for v in names}
    if args.scale:
        names = ["reference", "libjpeg-exact"] + ["%s/%d" % (v, s) for s in args.scale for v in ("reference", "libjpeg-exact")]
        opts = {v: dict(pixels=v.split("/")[0], scale=int(v.split("/")[1]) if "/" in v else 1) for v in names}
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    scans = [mjx.ParsedScan(d) for d in datas]
    bases = {v: mjx.Batch(ctx, scans, **opts[v]) for v in names}
    for v in names:
        assert all(x == mjx.OK for x in bases[v].create_status), bases[v].create_status
    runs = {v: [] for v in names}
    for r in range(args.repeats):
        for v in names[r % len(names):] + names[:r % len(names)]:
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
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / args.steps
                assert b.unconverged_runs() == u0, "a timed region had not converged (%s)" % v
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed (%s): %s" % (v, bad[:8])
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "bytes_written": b.bytes()["rgb"], "arena_bytes": arena})
                print("%-15s repeat %d: %.3f ms per step, stage B %.3f ms, %s %.3f ms, arena %.2f GB"
                      % (v, r, ms, kms.get("idct_color", 0.0), upsample_kernel(v), kms.get("resize", 0.0), arena / 1e9), flush=True)
            finally:
                b.close()
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (args.width, args.height, args.quality), "steps": args.steps,
           "repeats": args.repeats, "variants": {}}
    for v in names:
        best = min(runs[v], key=lambda x: x["ms_per_step"])
        out["variants"][v] = {"ms_per_step_best": best["ms_per_step"],
                              "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                              "all_ms_per_step": [x["ms_per_step"] for x in runs[v]],
                              "kernel_ms_per_step": best["kernel_ms_per_step"],
                              "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                              "upsample_kernel": upsample_kernel(v),
                              "upsample_ms_all": [x["kernel_ms_per_step"].get("resize", 0.0) for x in runs[v]],
                              "bytes_written": best["bytes_written"]}
        # (the device memory a batch took is the drop in free memory while it was built: 0 when the allocator served it from what an
        # earlier, larger batch of the run had returned -- such a figure says nothing and is left out)
        arena = max(x["arena_bytes"] for x in runs[v])
        if arena:
            out["variants"][v]["arena_bytes"] = arena
    if args.islow and not args.scale:
        f, x = out["variants"]["libjpeg"], out["variants"]["libjpeg-exact"]
        out["islow_over_float"] = {"step": round(x["ms_per_step_best"] / f["ms_per_step_best"], 4),
                                   "stage_b": round(x["kernel_ms_per_step"]["idct_color"] / f["kernel_ms_per_step"]["idct_color"], 4)}
    if args.scale:          # every scaled exact step against the full-size exact step of the same run, and against the default pixels at its scale
        full = out["variants"]["libjpeg-exact"]["ms_per_step_best"]
        out["scaled_exact"] = {str(s): {"over_full_size_exact": round(out["variants"]["libjpeg-exact/%d" % s]["ms_per_step_best"] / full, 4),
                                        "over_default_pixels_at_scale": round(out["variants"]["libjpeg-exact/%d" % s]["ms_per_step_best"]
                                                                              / out["variants"]["reference/%d" % s]["ms_per_step_best"], 4)}
                               for s in args.scale}
    for b in bases.values():
        b.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The colour models of MJX_COLOR_FILE beside their three-component twins, one process.

Pictures written by Pillow (quality 75, no subsampling) from the same synthetic content, `--unique` of them per variant:
  cmyk      four components, Adobe transform 0 (Pillow's CMYK), decoded with color="file"
  ycc_of_4  its three-component twin: the first three channels as an ordinary Y, Cb, Cr file -- the yardstick of the same run
  rgb       three components stored as R, G, B (Pillow's keep_rgb=True), decoded with color="file"
  ycc_of_3  the same picture as an ordinary 4:4:4 Y, Cb, Cr file -- its yardstick
Every variant builds a base batch of the unique pictures once and tiles it per repeat (only one large batch is resident at a time);
the variants take turns inside every repeat.  Per variant: ms per step (every repeat, best, median), Gpixels/s of the best step,
per-class kernel ms per step (dc_scan is the DC prediction, idct_color stage B) and the compressed bytes.  One JSON object on the
last line.

    python tools/bench_color.py [--steps 5] [--warmup 1] [--repeats 3] [--images 1024] [--unique 16] [--width 1920] [--height 1080]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pictures(width, height, unique, quality):
    import numpy as np
    from PIL import Image
    out = {"cmyk": [], "ycc_of_4": [], "rgb": [], "ycc_of_3": []}
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    for s in range(unique):
        rng = np.random.default_rng(s)
        a = np.stack([128 + 80 * np.sin(0.011 * (k + 1) * xx + 0.007 * (4 - k) * yy + k + s) + rng.normal(0, 6, (height, width))
                      for k in range(4)], axis=-1)
        a = np.clip(a, 0, 255).astype(np.uint8)

        def save(img, **kw):
            buf = io.BytesIO()
            img.save(buf, "JPEG", quality=quality, subsampling=0, **kw)
            return buf.getvalue()
        out["cmyk"].append(save(Image.fromarray(a, "CMYK")))
        rgb = Image.fromarray(np.ascontiguousarray(a[..., :3]), "RGB")
        out["ycc_of_4"].append(save(rgb))
        out["rgb"].append(save(rgb, keep_rgb=True))
        out["ycc_of_3"].append(out["ycc_of_4"][-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--variants", default="cmyk,ycc_of_4,rgb,ycc_of_3")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    files = pictures(args.width, args.height, args.unique, args.quality)
    names = [v for v in args.variants.split(",") if v]
    want = {"cmyk": mjx.MODEL_CMYK, "rgb": mjx.MODEL_RGB, "ycc_of_4": mjx.MODEL_YCBCR, "ycc_of_3": mjx.MODEL_YCBCR}
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    bases, scans = {}, []
    for v in names:
        color = "file" if v in ("cmyk", "rgb") else None
        sc = [mjx.ParsedScan(d, color=color) for d in files[v]]
        scans += sc
        bases[v] = mjx.Batch(ctx, sc, color=color)
        assert all(x == mjx.OK for x in bases[v].create_status), (v, bases[v].create_status)
        assert all(bases[v].color_model(i) == want[v] for i in range(args.unique)), v
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
                runs[key].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms})
                print("%-9s repeat %d: %.3f ms per step, DC %.3f ms, stage B %.3f ms" % (key, r, ms, kms.get("dc_scan", 0.0), kms.get("idct_color", 0.0)), flush=True)
            finally:
                b.close()
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:4:4 q%d" % (args.width, args.height, args.quality), "steps": args.steps,
           "repeats": args.repeats, "variants": {}}
    for key in names:
        best = min(runs[key], key=lambda x: x["ms_per_step"])
        out["variants"][key] = {"ms_per_step_best": best["ms_per_step"],
                                "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[key]), 4),
                                "all_ms_per_step": [x["ms_per_step"] for x in runs[key]],
                                "gpixels_per_s_best": round(n * args.width * args.height / best["ms_per_step"] / 1e6, 2),
                                "kernel_ms_per_step": best["kernel_ms_per_step"],
                                "compressed_bytes_per_picture": sum(len(d) for d in files[key]) // args.unique}
    for b in bases.values():
        b.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Progressive pictures (MJX_OPTS_PROGRESSIVE) beside their baseline twins of the same content, one process.

Per size (1920x1080 and 512x384) Pillow writes the same arrays twice at q75 4:2:0 -- progressive (libjpeg's ten-scan script, four
levels of k_prog_scan) and baseline -- and each variant is decoded as a batch (--images, the unique pictures tiled) and as a single
picture.  The progressive scans are decoded by serial lanes, one per scan and restart interval: a batch gets its
throughput from the number of pictures, a single picture is as slow as its longest chain of scans.  Per variant: ms per step (every
repeat, best, median), per-class kernel ms per step (huff_write holds k_prog_scan, gather the compaction, idct_color stage B), the
file bytes, and the timed steps that did not do the whole work (must be 0).  One JSON object on the last line, and in --out (default
profiles/bench_progressive.json).

    python tools/bench_progressive.py [--steps 3] [--warmup 1] [--repeats 3] [--images 512] [--unique 16] [--sizes 1920x1080,512x384]
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


def picture(w, h, seed):
    """photograph-like content: smooth colour fields, edges and some noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        for _ in range(6):
            fx, fy, ph = rng.uniform(0.002, 0.05), rng.uniform(0.002, 0.05), rng.uniform(0, 6.28)
            a[:, :, c] += rng.uniform(10, 40) * np.sin(fx * x + fy * y + ph)
    a += 128 + 40 * (((x // 97) + (y // 61)) % 2)[:, :, None] + rng.normal(0, 6, (h, w, 1)).astype(np.float32)
    return np.clip(a, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--sizes", default="1920x1080,512x384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_progressive.json"))
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    from PIL import Image
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",") if s]
    names = [(kind, w, h, count) for w, h in sizes for count in ("batch", "single") for kind in ("progressive", "baseline")]
    reps = max(1, args.images // args.unique)
    ctx = mjx.Context(0, profiling=True)
    bases, scans, file_bytes, pictures = {}, {}, {}, {}
    for w, h in sizes:
        arrays = [picture(w, h, s) for s in range(args.unique)]
        for kind in ("progressive", "baseline"):
            datas = []
            for a in arrays:
                b = io.BytesIO()
                Image.fromarray(a, "RGB").save(b, "JPEG", quality=args.quality, subsampling=2, progressive=(kind == "progressive"))
                datas.append(b.getvalue())
            for count in ("batch", "single"):
                key = (kind, w, h, count)
                use = datas if count == "batch" else datas[:1]
                scans[key] = [mjx.ParsedScan(d, progressive=True) for d in use]
                bases[key] = mjx.Batch(ctx, scans[key], progressive=True)
                assert all(x == mjx.OK for x in bases[key].create_status), (key, bases[key].create_status)
                pictures[key] = len(use) * (reps if count == "batch" else 1)
                file_bytes[key] = sum(len(d) for d in use) * (reps if count == "batch" else 1)
    runs = {k: [] for k in names}
    unconverged = 0
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        for key in order:
            b = bases[key].tile(reps if key[3] == "batch" else 1)
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
                print("%s %dx%d %s repeat %d: %.3f ms per step, %s" % (key + (r, ms, kms)), flush=True)
            finally:
                b.close()
    out = {"images": args.images, "unique": args.unique, "quality": args.quality, "steps": args.steps, "repeats": args.repeats,
           "unconverged_runs": unconverged, "variants": {}}
    for key in names:
        kind, w, h, count = key
        best = min(runs[key], key=lambda x: x["ms_per_step"])
        out["variants"]["%s_%dx%d_%s" % key] = {"kind": kind, "width": w, "height": h, "pictures": pictures[key],
                                                 "ms_per_step_best": best["ms_per_step"],
                                                 "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[key]), 4),
                                                 "all_ms_per_step": [x["ms_per_step"] for x in runs[key]],
                                                 "gpixels_per_s_best": round(pictures[key] * w * h / best["ms_per_step"] / 1e6, 3),
                                                 "kernel_ms_per_step": best["kernel_ms_per_step"],
                                                 "file_bytes": file_bytes[key]}
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

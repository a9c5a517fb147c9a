#!/usr/bin/env python3
"""Resize on the device (mjx_resize) against today's route, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures, 64 unique ones -- with one seeded random-resized-crop
rectangle per picture (area 8 .. 100 % of the picture, aspect 3/4 .. 4/3), every picture to 224 x 224 planar float16, ImageNet
mean / std, in ONE caller-owned 2048 x 3 x 224 x 224 tensor:
  a_auto    Resize(224, 224, antialias, auto_scale=True, filter=--filter): the library picks the DCT-domain scale per picture
  b_scale1  the same with auto_scale=False at scale 1: the resize kernel filters the full-size rectangle
  c_torch   today's route: the same rectangles decoded packed at scale 1, then per picture
            torch.nn.functional.interpolate(mode=--filter, antialias=True) and the normalisation into the tensor, timed to a
            device synchronise ("nearest" is torch's "nearest-exact")
Caller-owned destinations cannot be tiled, so every variant builds its batch from the 2048 inputs themselves (the 64 scans, each
named 32 times).  The variants take turns inside every repeat.

--fit: the fit mode of the library's variants (mjx_resize's fit byte) -- stretch, cover (centre-crop) or contain (letterbox, padded
with the mean colour's bytes); a comma-separated list runs every mode of it for a_auto and b_scale1, the modes taking turns inside
every repeat like the variants (a result is then named variant:mode).  With contain in the list the tool also times, in every
repeat, a hipMemsetAsync of the batch's whole output tensor on the null stream to a device synchronise (memset_ms_all) and writes
the comparison the mode is held to beside the figures: every contain step <= the stretch step of the same repeat + that memset.

Per variant: ms per step (every repeat, best, median), per-class kernel ms per step (idct_color is stage B, resize is
k_resize_out), the bytes written, the scales auto_scale chose.  One JSON object on the last line.

    python tools/bench_resize.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--variants a_auto,b_scale1,c_torch]
                                 [--filter bilinear|bicubic|nearest] [--fit stretch,cover,contain]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def random_resized_crops(n, W, H, seed):
    """torchvision's RandomResizedCrop rule, seeded: area 8 .. 100 %, log-uniform aspect 3/4 .. 4/3; the whole picture after ten misses"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        rect = (0, 0, W, H)
        for _ in range(10):
            area = W * H * rng.uniform(0.08, 1.0)
            aspect = np.exp(rng.uniform(np.log(3.0 / 4.0), np.log(4.0 / 3.0)))
            w, h = int(round(np.sqrt(area * aspect))), int(round(np.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                rect = (int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1)), w, h)
                break
        out.append(rect)
    return out


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
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--variants", default="a_auto,b_scale1,c_torch")
    ap.add_argument("--filter", default="bilinear", choices=("bilinear", "bicubic", "nearest"))
    ap.add_argument("--fit", default="stretch", help="stretch, cover, contain, or a comma-separated list of them")
    args = ap.parse_args()
    fits = [f for f in args.fit.split(",") if f]
    assert fits and all(f in ("stretch", "cover", "contain") for f in fits), "--fit: stretch, cover, contain"
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import torch.nn.functional as F
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    W, H, side = args.width, args.height, args.side
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    rects = random_resized_crops(n, W, H, seed=224)
    base_names = [v for v in args.variants.split(",") if v]
    # (a library variant per fit mode: the plain name for a single mode, variant:mode for a list)
    names = [v if v == "c_torch" or len(fits) == 1 else "%s:%s" % (v, f) for v in base_names for f in (fits if v != "c_torch" else fits[:1])]
    fit_of = {(v if v == "c_torch" or len(fits) == 1 else "%s:%s" % (v, f)): f for v in base_names for f in (fits if v != "c_torch" else fits[:1])}
    pad = tuple(int(round(255 * m)) for m in MEAN)
    dev = torch.device("cuda", 0)
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    scans = [mjx.ParsedScan(d) for d in datas]
    inputs = [scans[i % args.unique] for i in range(n)]
    sc_t = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    bi_t = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    runs = {v: [] for v in names}
    scales = {}
    memset_ms = []
    import ctypes
    hip = mjx.lib()                      # (the HIP runtime the library itself is linked against)
    hip.hipMemsetAsync.restype = hip.hipDeviceSynchronize.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        if "contain" in fits:            # the second term of contain's bar: clearing the batch's whole output, this repeat
            tensor = torch.empty((n, 3, side, side), dtype=torch.float16, device=dev)
            torch.cuda.synchronize()
            nbytes = tensor.numel() * 2
            assert hip.hipMemsetAsync(tensor.data_ptr(), 0, nbytes, None) == 0 and hip.hipDeviceSynchronize() == 0      # (warm)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                assert hip.hipMemsetAsync(tensor.data_ptr(), 0, nbytes, None) == 0
            assert hip.hipDeviceSynchronize() == 0
            memset_ms.append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            print("memset    repeat %d: %.3f ms per step (%d bytes)" % (r, memset_ms[-1], nbytes), flush=True)
            del tensor
        for v in order:
            tensor = torch.empty((n, 3, side, side), dtype=torch.float16, device=dev)
            torch.cuda.synchronize()
            per = 3 * side * side
            convert = None
            if v == "c_torch":
                b = mjx.Batch(ctx, inputs, rois=rects)
                assert all(x == mjx.OK for x in b.create_status)
                # the packed crops in the batch's pool: wrapped, not owned, through the array interface; one view per picture
                ptrs = [b.rgb_device(i) for i in range(n)]
                p0 = min(p for p, _ in ptrs)
                span = max(p + nb for p, nb in ptrs) - p0

                class Pool:
                    __cuda_array_interface__ = {"shape": (span,), "typestr": "|u1", "data": (p0, False), "version": 2}
                pool = torch.as_tensor(Pool(), device=dev)
                views = [pool.as_strided((1, rects[i][3], rects[i][2], 3), (0, rects[i][2] * 3, 3, 1), ptrs[i][0] - p0).permute(0, 3, 1, 2) for i in range(n)]

                def convert():
                    for i in range(n):
                        if args.filter == "nearest":
                            x = F.interpolate(views[i].to(torch.float32), size=(side, side), mode="nearest-exact")
                        else:
                            x = F.interpolate(views[i].to(torch.float32), size=(side, side), mode=args.filter, align_corners=False, antialias=True)
                        tensor[i:i + 1].copy_(torch.addcmul(bi_t, x, sc_t))
            else:
                fmt = mjx.Output("float16", planar=True, mean=MEAN, std=STD, pad=pad,
                                 dst=[(tensor.data_ptr() + 2 * per * i, side, side, side, side * side) for i in range(n)])
                b = mjx.Batch(ctx, inputs, rois=rects, output=fmt, resize=mjx.Resize(side, side, antialias=True, auto_scale=v.startswith("a_auto"), filter=args.filter, fit=fit_of[v]))
                assert all(x == mjx.OK for x in b.create_status)
                if v not in scales:
                    got = [b.scale(i) for i in range(n)]
                    scales[v] = {str(s): got.count(s) for s in (1, 2, 4, 8)}
            try:
                def step():
                    b.decode()
                    if convert:
                        b.wait()
                        convert()
                for _ in range(args.warmup):
                    step()
                    b.wait()
                    torch.cuda.synchronize()
                b.kernel_ms(reset=True)
                u0 = b.unconverged_runs()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                b.wait()
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / args.steps
                assert b.unconverged_runs() == u0, "a timed region had not converged (%s)" % v
                bad = [i for i in range(len(b)) if b.status(i) != mjx.OK]
                assert not bad, "pictures failed (%s): %s" % (v, bad[:8])
                assert bool(torch.isfinite(tensor).all()), "the tensor holds elements that were not written (%s)" % v
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "bytes_written": b.bytes()["rgb"]})
                print("%-9s repeat %d: %.3f ms per step, stage B %.3f ms, resize %.3f ms" % (v, r, ms, kms.get("idct_color", 0.0), kms.get("resize", 0.0)), flush=True)
            finally:
                b.close()
                del tensor
    out = {"filter": args.filter, "fit": fits, "images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (W, H, args.quality), "target": side, "steps": args.steps,
           "repeats": args.repeats, "variants": {}}
    for v in names:
        best = min(runs[v], key=lambda x: x["ms_per_step"])
        out["variants"][v] = {"ms_per_step_best": best["ms_per_step"],
                              "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                              "all_ms_per_step": [x["ms_per_step"] for x in runs[v]],
                              "kernel_ms_per_step": best["kernel_ms_per_step"],
                              "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                              "resize_ms_all": [x["kernel_ms_per_step"].get("resize", 0.0) for x in runs[v]],
                              "bytes_written": best["bytes_written"], "scales": scales.get(v)}
    if "contain" in fits:
        out["memset_ms_all"] = memset_ms
        for v in base_names:
            if v == "c_torch" or "stretch" not in fits:
                continue
            st, co = out["variants"]["%s:stretch" % v]["all_ms_per_step"], out["variants"]["%s:contain" % v]["all_ms_per_step"]
            out["contain_bar_%s" % v] = {"stretch_plus_memset": [round(a + m, 4) for a, m in zip(st, memset_ms)], "contain": co,
                                         "every_repeat_within": all(c <= a + m for c, a, m in zip(co, st, memset_ms))}
    if "a_auto" in names and "c_torch" in names:
        out["bar1_every_repeat_of_a_below_the_best_of_c"] = max(out["variants"]["a_auto"]["all_ms_per_step"]) < out["variants"]["c_torch"]["ms_per_step_best"]
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

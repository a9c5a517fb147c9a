#!/usr/bin/env python3
"""Orientation on the device (mjx_orient) against the two-step route, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures, 64 unique ones -- leaves as 224 x 224 planar float16,
ImageNet mean / std:
  a_fused      code 6 (a quarter turn clockwise), a seeded random 224 x 224 of the turned picture, through k_orient_out
  b_twostep    the same pixels as packed crops of the stored picture, then torch.rot90(...).contiguous() and the normalisation
               into one tensor, timed to a device synchronise: the route a user has without the orientation
  c_fused_rs   code 6, a seeded 600 x 600 of the turned picture resized to 224 x 224 (auto_scale), through k_resize_orient
  c_twostep_rs the same crops resized by the library without an orientation, then torch.rot90 of its output into one tensor
  r_code1 / r_code2 / r_code6   the 600 x 600 crops through the resize with codes 1, 2 and 6: what the column-wise horizontal read
               of the transposing codes costs over the row-wise one (ms per step and the MJX_K_RESIZE class's kernel ms)
Every variant builds a base batch of the unique pictures once and tiles it per repeat; the variants take turns inside every
repeat.  Per variant: ms per step (every repeat, best, median) and per-class kernel ms per step ("resize" is the class of the pass
behind stage B).  Bar: every repeat of a fused variant lies below the best repeat of its two-step one.  One JSON object on the
last line.

    python tools/bench_orient.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--variants a_fused,b_twostep,...]
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
    ap.add_argument("--variants", default="a_fused,b_twostep,c_fused_rs,c_twostep_rs,r_code1,r_code2,r_code6")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    W, H = args.width, args.height
    side, big = min(224, W, H), min(600, W, H) // 8 * 8
    rng = np.random.RandomState(224)
    # rectangles of the turned picture (code 6: H wide, W high) and of the stored one for code 1 / 2
    crops_d = [(int(rng.randint(0, H - side + 1)), int(rng.randint(0, W - side + 1)), side, side) for _ in range(args.unique)]
    # (origins on multiples of 8: the rectangles auto_scale rounds outward then have one size, so the pictures of a tiled batch lie
    # at equal distances in its pool and the two-step variants can view them as one tensor)
    big_d = [(int(rng.randint(0, (H - big) // 8 + 1)) * 8, int(rng.randint(0, (W - big) // 8 + 1)) * 8, big, big) for _ in range(args.unique)]
    scans = [mjx.ParsedScan(d) for d in datas]
    crops_s = [s.orient_plan(6, roi=r)["stored_rect"] for s, r in zip(scans, crops_d)]
    big_s = [s.orient_plan(6, roi=r)["stored_rect"] for s, r in zip(scans, big_d)]
    f16 = lambda: mjx.Output("float16", planar=True, mean=MEAN, std=STD)
    rs = mjx.Resize(side, side, antialias=True, auto_scale=True)
    turn = lambda c: mjx.Orient(exif=False, extra=c)
    table = {                            # rectangles, output, resize, orientation
        "a_fused": (crops_d, f16(), None, turn(6)), "b_twostep": (crops_s, None, None, None),
        "c_fused_rs": (big_d, f16(), rs, turn(6)), "c_twostep_rs": (big_s, f16(), rs, None),
        "r_code1": (big_s, f16(), rs, turn(1)), "r_code2": (big_s, f16(), rs, turn(2)), "r_code6": (big_d, f16(), rs, turn(6)),
    }
    names = [v for v in args.variants.split(",") if v]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    dev = torch.device("cuda", 0)
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    bases = {}
    for v in names:
        rois, out, resize, orient = table[v]
        bases[v] = mjx.Batch(ctx, scans, rois=rois, output=out, resize=resize, orient=orient)
        assert all(x == mjx.OK for x in bases[v].create_status), (v, bases[v].create_status)
    sc_t = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    bi_t = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    runs = {v: [] for v in names}
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        for v in order:
            tensor = None
            if v in ("b_twostep", "c_twostep_rs"):
                tensor = torch.empty((n, 3, side, side), dtype=torch.float16, device=dev)
                torch.cuda.synchronize()
            b = bases[v].tile(reps)
            convert = None
            if tensor is not None:
                # the pictures of the tiled batch lie at equal distances in its pool: one strided view of all of them
                # (the pool belongs to the library: wrapped, not owned, through the array interface)
                if v == "b_twostep":
                    p0, nb = b.rgb_device(0)
                    stride = b.rgb_device(1)[0] - p0
                    assert all(b.rgb_device(i)[0] == p0 + i * stride for i in (2, n // 2, n - 1)) and nb == side * side * 3

                    class Pool:
                        __cuda_array_interface__ = {"shape": (n * stride,), "typestr": "|u1", "data": (p0, False), "version": 2}
                    view = torch.as_tensor(Pool(), device=dev).as_strided((n, side, side, 3), (stride, side * 3, 3, 1))

                    def convert():
                        turned = torch.rot90(view, -1, (1, 2)).contiguous()
                        tensor.copy_(torch.addcmul(bi_t, turned.permute(0, 3, 1, 2).to(torch.float32), sc_t))
                else:
                    p0 = b.output_info(0)["dev"]
                    stride = b.output_info(1)["dev"] - p0
                    assert all(b.output_info(i)["dev"] == p0 + i * stride for i in (2, n // 2, n - 1)) and stride % 2 == 0

                    class Pool:
                        __cuda_array_interface__ = {"shape": (n * stride // 2,), "typestr": "<f2", "data": (p0, False), "version": 2}
                    view = torch.as_tensor(Pool(), device=dev).as_strided((n, 3, side, side), (stride // 2, side * side, side, 1))

                    def convert():
                        tensor.copy_(torch.rot90(view, -1, (2, 3)))
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
                kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "scale": b.scale(0), "code": b.orientation(0)})
                print("%-13s repeat %d: %.3f ms per step, stage B %.3f ms, behind it %.3f ms" % (v, r, ms, kms.get("idct_color", 0.0), kms.get("resize", 0.0)), flush=True)
            finally:
                b.close()
                del tensor
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (W, H, args.quality), "steps": args.steps, "repeats": args.repeats,
           "variants": {}, "bars": {}}
    for v in names:
        best = min(runs[v], key=lambda x: x["ms_per_step"])
        out["variants"][v] = {"code": best["code"], "scale": best["scale"], "ms_per_step_best": best["ms_per_step"],
                              "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                              "all_ms_per_step": [x["ms_per_step"] for x in runs[v]],
                              "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                              "resize_class_ms_all": [x["kernel_ms_per_step"].get("resize", 0.0) for x in runs[v]]}
    for fused, two in (("a_fused", "b_twostep"), ("c_fused_rs", "c_twostep_rs")):
        if fused in runs and two in runs:
            out["bars"][fused] = max(x["ms_per_step"] for x in runs[fused]) < min(x["ms_per_step"] for x in runs[two])
    for b in bases.values():
        b.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

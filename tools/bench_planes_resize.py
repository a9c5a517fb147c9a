#!/usr/bin/env python3
"""YCbCr planes at a fixed size (mjx_batch_create_planes_orient) against the routes a caller has today, one process.

Per picture size (--sizes, default 1920x1080 and 3840x2160; 4:2:0 q75 synthetic pictures, --unique of them tiled to --images with
mjx_batch_tile) and per target (--targets, default 224x224 and 640x360), the variants taking turns inside every repeat:
  a_nv12     this feature: Planes("uint8", interleave=True) + Resize(target, antialias, auto_scale=True): the library picks the
             DCT-domain scale per picture, stage B writes the small planes, k_resize_planes resamples them
  b_rgb      the existing packed-RGB resize to the same target (Resize with auto_scale, interleaved uint8)
  c_torch    today's route to planes at a fixed size: the full-size planes= decode (I420, uint8), then per picture and plane one
             torch.nn.functional.interpolate(mode="bilinear", antialias=True), rounded to uint8 into y / cb / cr tensors, timed to a
             device synchronise
  c_batched  the same with ONE interpolate per plane over the whole batch -- possible only because the tiled pictures share one size
             (the planes lie a constant stride apart in the pool); a folder of mixed sizes has c_torch
Per variant: ms per step for every repeat (best, median), stage-B (idct_color) and MJX_K_RESIZE (resize) kernel ms per step, the bytes
written, the scales auto_scale chose, and the timed steps that left work undone (mjx_batch_unconverged_runs; must be 0).  One JSON
object on the last line.

    python tools/bench_planes_resize.py [--steps 5] [--warmup 1] [--repeats 3] [--images 1024] [--unique 16]
                                        [--sizes 1920x1080,3840x2160] [--targets 224x224,640x360] [--variants a_nv12,b_rgb,c_torch,c_batched]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wh(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--targets", default="224x224,640x360")
    ap.add_argument("--variants", default="a_nv12,b_rgb,c_torch,c_batched")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import torch.nn.functional as F
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    names = [v for v in args.variants.split(",") if v]
    dev = torch.device("cuda", 0)
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    times = max(1, args.images // args.unique)
    n = times * args.unique
    out = {"images": n, "unique": args.unique, "quality": args.quality, "steps": args.steps, "repeats": args.repeats, "cases": []}
    for W, H in [wh(s) for s in args.sizes.split(",") if s]:
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            datas = list(ex.map(lambda s: mjx.synth_jpeg(W, H, "420", args.quality, s), range(args.unique)))
        scans = [mjx.ParsedScan(d) for d in datas]
        for tw, th in [wh(s) for s in args.targets.split(",") if s]:
            runs = {v: [] for v in names}
            scales = {}
            for r in range(args.repeats):
                for v in names[r % len(names):] + names[:r % len(names)]:
                    rs = mjx.Resize(tw, th, antialias=True, auto_scale=True)
                    convert = None
                    if v == "a_nv12":
                        base = mjx.Batch(ctx, scans, planes=mjx.Planes("uint8", interleave=True), resize=rs)
                    elif v == "b_rgb":
                        base = mjx.Batch(ctx, scans, resize=rs)
                    else:
                        base = mjx.Batch(ctx, scans, planes=mjx.Planes("uint8"))
                    assert all(x == mjx.OK for x in base.create_status), (v, base.create_status)
                    b = base.tile(times)
                    base.close()
                    if v in ("a_nv12", "b_rgb") and v not in scales:
                        got = [b.scale(i) for i in range(n)]
                        scales[v] = {str(s): got.count(s) for s in (1, 2, 4, 8)}
                    if v in ("c_torch", "c_batched"):
                        infos = [b.plane_info(i) for i in range(n)]
                        p0 = min(inf["dev"][0] for inf in infos)
                        span = max(inf["dev"][2] + inf["width"][2] * inf["height"][2] for inf in infos) - p0

                        class Pool:
                            __cuda_array_interface__ = {"shape": (span,), "typestr": "|u1", "data": (p0, False), "version": 2}
                        pool = torch.as_tensor(Pool(), device=dev)
                        sizes = [(th, tw), ((th + 1) // 2, (tw + 1) // 2), ((th + 1) // 2, (tw + 1) // 2)]
                        dst = [torch.empty((n,) + s, dtype=torch.uint8, device=dev) for s in sizes]
                        if v == "c_torch":
                            views = [[pool.as_strided((1, 1, inf["height"][c], inf["width"][c]), (0, 0, inf["row_pitch"][c], 1), inf["dev"][c] - p0)
                                      for c in range(3)] for inf in infos]

                            def convert():
                                for i in range(n):
                                    for c in range(3):
                                        x = F.interpolate(views[i][c].to(torch.float32), size=sizes[c], mode="bilinear", align_corners=False, antialias=True)
                                        dst[c][i].copy_(x[0, 0].round_().clamp_(0, 255))
                        else:
                            step = infos[1]["dev"][0] - infos[0]["dev"][0] if n > 1 else 0
                            assert all(infos[i]["dev"][c] - infos[0]["dev"][c] == i * step for i in range(n) for c in range(3)), "the pictures do not lie a constant stride apart"
                            whole = [pool.as_strided((n, 1, infos[0]["height"][c], infos[0]["width"][c]), (step, 0, infos[0]["row_pitch"][c], 1), infos[0]["dev"][c] - p0)
                                     for c in range(3)]

                            def convert():
                                for c in range(3):
                                    x = F.interpolate(whole[c].to(torch.float32), size=sizes[c], mode="bilinear", align_corners=False, antialias=True)
                                    dst[c].copy_(x[:, 0].round_().clamp_(0, 255))
                    try:
                        def one():
                            b.decode()
                            if convert:
                                b.wait()
                                convert()
                        for _ in range(args.warmup):
                            one()
                            b.wait()
                            torch.cuda.synchronize()
                        b.kernel_ms(reset=True)
                        u0 = b.unconverged_runs()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            one()
                        b.wait()
                        torch.cuda.synchronize()
                        ms = 1e3 * (time.perf_counter() - t0) / args.steps
                        undone = b.unconverged_runs() - u0
                        bad = [i for i in range(n) if b.status(i) != mjx.OK]
                        assert not bad, "pictures failed (%s): %s" % (v, bad[:8])
                        kms = {k: round(x[0] / args.steps, 4) for k, x in b.kernel_ms(reset=True).items() if x[1]}
                        written = b.bytes()["rgb"] + (sum(t.numel() for t in dst) if convert else 0)
                        runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "bytes_written": written, "steps_undone": int(undone)})
                        print("%dx%d -> %dx%d %-9s repeat %d: %.3f ms per step, stage B %.3f ms, resize %.3f ms, undone %d"
                              % (W, H, tw, th, v, r, ms, kms.get("idct_color", 0.0), kms.get("resize", 0.0), undone), flush=True)
                    finally:
                        b.close()
            case = {"picture": "%dx%d 4:2:0 q%d" % (W, H, args.quality), "target": "%dx%d" % (tw, th), "variants": {}}
            for v in names:
                best = min(runs[v], key=lambda x: x["ms_per_step"])
                case["variants"][v] = {"ms_per_step_best": best["ms_per_step"],
                                       "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                                       "all_ms_per_step": [x["ms_per_step"] for x in runs[v]],
                                       "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                                       "resize_ms_all": [x["kernel_ms_per_step"].get("resize", 0.0) for x in runs[v]],
                                       "bytes_written": best["bytes_written"], "scales": scales.get(v),
                                       "steps_undone": sum(x["steps_undone"] for x in runs[v])}
            assert all(c["steps_undone"] == 0 for c in case["variants"].values()), "a timed step left work undone: %s" % case
            out["cases"].append(case)
        for s in scans:
            s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

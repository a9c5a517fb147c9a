#!/usr/bin/env python3
"""Output formats (mjx_output) against packed RGB and against the two-step route, one process, the headline's inputs.

The batch of bench.py -- 2048 synthetic 3840x2160 4:2:0 q75 pictures, 64 unique ones -- decoded
  a_packed   224 x 224 at a seeded random place per unique picture, packed RGB: the existing path (tools/bench_roi.py's r224)
  b_fused    the same crops as planar float16, ImageNet mean / std, library-owned
  c_caller   the same into ONE caller-owned 2048 x 3 x 224 x 224 float16 allocation (a torch tensor)
  d_twostep  a_packed followed by the equivalent torch conversion of the batch's packed pictures into such a tensor, timed to a
             device synchronise: the two-step route a user has without the output formats
  e_quarter / e_quarter_f16   whole pictures at 1/4 scale, packed against planar float16
  f_full / f_full_u8          whole pictures at full size, packed against interleaved uint8 through the new kernel family: what
                              the form itself costs
a, b, e, f build a base batch of the unique pictures once and tile it per repeat (only one large batch is resident at a time).
mjx_batch_tile refuses caller-owned destinations, so c builds its batch from the 2048 inputs themselves (the 64 scans, each
named 32 times, every input with its own slot of the tensor); d views a's pool as 2048 crops -- the regions of a tiled batch
lie at equal distances -- so its conversion is one torch expression.  The variants take turns inside every repeat.

Per variant: ms per step (every repeat, best, median), per-class kernel ms per step (idct_color is stage B), the bytes written,
and the device memory the batch took when it was built (free memory before and after; 0 where the context reused a cached block).
One JSON object on the last line.

    python tools/bench_output.py [--steps 5] [--warmup 1] [--repeats 3] [--images 2048] [--variants a_packed,b_fused,...]
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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
    ap.add_argument("--variants", default="a_packed,b_fused,c_caller,d_twostep,e_quarter,e_quarter_f16,f_full,f_full_u8")
    args = ap.parse_args()
    import torch                         # (first: libmjx.so must find torch's HIP runtime already loaded, as in bench.py)
    import __graft_entry__ as ge
    ge.build()
    mjx = ge.load_package()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        datas = list(ex.map(lambda s: mjx.synth_jpeg(args.width, args.height, "420", args.quality, s), range(args.unique)))
    W, H = args.width, args.height
    rng = np.random.RandomState(224)
    side = min(224, W, H)
    crops = [(int(rng.randint(0, W - side + 1)), int(rng.randint(0, H - side + 1)), side, side) for _ in range(args.unique)]
    f16 = lambda: mjx.Output("float16", planar=True, mean=MEAN, std=STD)
    table = {                            # scale, rectangles, output
        "a_packed": (1, crops, None), "b_fused": (1, crops, f16()), "c_caller": (1, crops, "caller"), "d_twostep": (1, crops, None),
        "e_quarter": (4, None, None), "e_quarter_f16": (4, None, f16()),
        "f_full": (1, None, None), "f_full_u8": (1, None, mjx.Output("uint8")),
    }
    names = [v for v in args.variants.split(",") if v]
    reps = max(1, args.images // args.unique)
    n = reps * args.unique
    dev = torch.device("cuda", 0)
    ctx = mjx.Context(0, profiling=True, throughput_plan=True)
    scans = [mjx.ParsedScan(d) for d in datas]
    bases = {}
    for v in names:
        scale, rois, out = table[v]
        if out != "caller":
            bases[v] = mjx.Batch(ctx, scans, scale=scale, rois=rois, output=out)
            assert all(x == mjx.OK for x in bases[v].create_status), bases[v].create_status
    sc_t = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    bi_t = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    runs = {v: [] for v in names}
    for r in range(args.repeats):
        order = names[r % len(names):] + names[:r % len(names)]
        for v in order:
            scale, rois, out = table[v]
            tensor = None
            if v in ("c_caller", "d_twostep"):
                tensor = torch.empty((n, 3, side, side), dtype=torch.float16, device=dev)
                torch.cuda.synchronize()
            free0 = free_device_bytes(mjx)
            if v == "c_caller":
                per = 3 * side * side
                fmt = mjx.Output("float16", planar=True, mean=MEAN, std=STD,
                                 dst=[(tensor.data_ptr() + 2 * per * i, side, side, side, side * side) for i in range(n)])
                b = mjx.Batch(ctx, [scans[i % args.unique] for i in range(n)], rois=[crops[i % args.unique] for i in range(n)], output=fmt)
                assert all(x == mjx.OK for x in b.create_status)
            else:
                b = bases[v].tile(reps)
            arena = max(0, free0 - free_device_bytes(mjx))
            convert = None
            if v == "d_twostep":
                # the packed crops of the tiled batch lie at equal distances in its pool: one strided view of all of them
                p0, nb = b.rgb_device(0)
                p1, _ = b.rgb_device(1)
                stride = p1 - p0
                assert all(b.rgb_device(i)[0] == p0 + i * stride for i in (2, n // 2, n - 1)) and nb == side * side * 3
                # (the pool belongs to the library: wrapped, not owned, through the array interface)

                class Pool:
                    __cuda_array_interface__ = {"shape": (n * stride,), "typestr": "|u1", "data": (p0, False), "version": 2}
                pool = torch.as_tensor(Pool(), device=dev)
                view = pool.as_strided((n, side, side, 3), (stride, side * 3, 3, 1))

                def convert():
                    tensor.copy_(torch.addcmul(bi_t, view.permute(0, 3, 1, 2).to(torch.float32), sc_t))
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
                runs[v].append({"ms_per_step": round(ms, 4), "kernel_ms_per_step": kms, "bytes_written": b.bytes()["rgb"], "arena_bytes": arena})
                print("%-14s repeat %d: %.3f ms per step, stage B %.3f ms, arena %.2f GB" % (v, r, ms, kms.get("idct_color", 0.0), arena / 1e9), flush=True)
            finally:
                b.close()
                del tensor
    out = {"images": n, "unique": args.unique, "picture": "%dx%d 4:2:0 q%d" % (W, H, args.quality), "steps": args.steps, "repeats": args.repeats,
           "variants": {}}
    for v in names:
        best = min(runs[v], key=lambda x: x["ms_per_step"])
        out["variants"][v] = {"scale": table[v][0], "ms_per_step_best": best["ms_per_step"],
                              "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in runs[v]), 4),
                              "all_ms_per_step": [x["ms_per_step"] for x in runs[v]],
                              "kernel_ms_per_step": best["kernel_ms_per_step"],
                              "stage_b_ms_all": [x["kernel_ms_per_step"].get("idct_color", 0.0) for x in runs[v]],
                              "bytes_written": best["bytes_written"], "arena_bytes": max(x["arena_bytes"] for x in runs[v])}
    for b in bases.values():
        b.close()
    for s in scans:
        s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""bench.py -- Mpixels/s of the baseline-JPEG decode hot path on 4K 4:2:0 batches (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (N > 1: launched by torch.distributed.run, one rank per GPU)

A plain run does what the headline needs: it builds the batch, warms up, times K steps, checks that every timed step did
the whole work (unconverged_chunk_runs, picture statuses), writes --dump-outputs and prints the JSON line with the kernels'
HIP-event times of the timed region and the roofline objects computed from them (traffic from the committed collection under
profiles/).  --full adds everything else below: the parity gate, one_pass_latency_ms, host_side, the rocprofv3 traffic
passes, the one-stream pass, extra_configs, e2e_from_bytes(_pool) and cpu_baseline (--no-* switch single legs off again).

--dump-outputs DIR writes what the timed path computed in its last step (rank 0's batch): the decoded RGB of every picture
is W*H*3 bytes (51 GB at the headline size), so DIR/rgb.npy holds a fixed, seeded sample of it, float32 [pictures, pixels, 3]
(dump_outputs()).  The inputs are synthetic pictures from fixed seeds, so equal arguments give equal inputs.

A *step* = one pass of the whole hot path (entropy decode -> dequant -> IDCT -> upsample -> RGB) over the rank's batch:
`--images-per-gpu` synthetic 3840x2160 4:2:0 q75 baseline JPEGs (BASELINE.json configs[4] is 16384 images over 8 GPUs
= 2048 per GPU; per-GPU work is fixed as N grows -> weak scaling).  Inputs (de-stuffed scans, tables) are resident in
HBM before the timed region; outputs stay in HBM.  Images are independent, so ranks never exchange data: image i of the
global batch goes to rank i mod N.  The harness needs one barrier and one MAX-reduce of the elapsed time; both go over
gloo (host TCP) -- the north star says "no RCCL", and that holds for the harness as well as for the data path.

The JSON line carries, besides the contract fields ([full] = with --full only):
  roofline      what SURVEY.md s8(d) defines.  stages=all (the default, the headline): achieved = sum over the images of
                B_e2e = S + 3*W*H (compressed bytes in, packed RGB out) per step / wall time per step of the timed region, frac =
                that / the 8 TB/s HBM3E peak; `kernel` = the kernel class with the largest HIP-event time in the timed region,
                whose own per-launch figures (algorithmic bytes, average launch duration, fraction of peak) are in
                `dominant_kernel`; `traffic` = HBM bytes per step from rocprofv3 PMC passes (FETCH_SIZE x 2 + WRITE_SIZE, separate
                passes, as the MI355X microarchitecture guide prescribes) -- observed in this run with --full when rocprofv3 is on
                the box (`traffic_source`: "observed ..."), else scaled from the committed collection under profiles/.
                stages=pixels (the config-4 stage-B sweep): the pixel kernel on B_idct = 128*n_blocks + 3*W*H.
  kernel_rooflines  every kernel class on its own algorithmic bytes, from the timed region's event times
                (the library overlaps the entropy stages of two chunks and stage B on three streams: these durations include
                the contention); idct_color also with the bytes it physically moves (frac_physical)
  roofline_isolated / kernel_rooflines_isolated  [full] the same from a one-stream pass over the same batch: stand-alone durations
  upload_side   GPU work of the upload, outside the timed region (HIP-event time for the unique pictures scaled to the batch): 0
                since round 5 -- the host writes the lane-interleaved scan pool while it packs the scans for the transfer; with
                --device-destuff the de-stuffing kernels and k_scan_interleave
  one_pass_latency_ms  [full] ms_per_step is the pipelined rate (the steps are enqueued back to back, one wait); this is ONE pass of
                the same batch on its own, enqueue to the end of its last kernel (this rank); null in a plain run
  kernels       per kernel class: launches, total ms
  host_side     [full] parse and batch-creation times of the unique pictures, and the parser on one thread
  parity        [full] the gate behind `value`: every picture of the timed batch compared on the device with its
                unique original (bit-equal), pictures of the batch compared with the CPU oracle (coefficients equal, RGB
                within 1), and the pictures the cpu_baseline leg decodes compared with a REF_COMPAT decode on the GPU.
                The run fails if any check fails.
  extra_configs [full] the other measurement rows of SURVEY s8(d): BASELINE config 4 (4096 x 1080p) whole path and stage B alone
                (the ">= 60 % of HBM on B_idct" sweep), 4K at quality 50 and 90; each with Mpixels/s, Gbit/s of entropy-coded
                data and the dominant kernel's roofline fraction
  e2e_from_bytes  [full] mjx_decode_batch from JPEG file bytes in host memory to RGB in HBM (parse + H2D + decode), Mpixels/s;
                e2e_from_bytes_pool the same through the library's multi-GPU pool
  cpu_baseline  [full] the oracle (C restatement of the reference's algorithm, kind "port") on all host cores and on one core
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
SUBS = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4", "440": "4:4:0", "gray": "greyscale"}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images-per-gpu", type=int, default=2048)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--subsampling", default="420")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic images in the global batch (SURVEY s8(d))")
    ap.add_argument("--chunk-images", type=int, default=0)
    ap.add_argument("--stages", default="all", choices=["all", "pixels"], help="pixels = stage-B-only sweep on resident coefficients")
    ap.add_argument("--device-destuff", action="store_true", help="upload stuffed scans; FF00 compaction on the GPU at upload")
    ap.add_argument("--streams", type=int, default=0, choices=[0, 1, 2, 3], help="HIP streams of the context (0 = library default); with 2, "
                    "stage B of one chunk overlaps stage A of the next and per-kernel times include the contention")
    ap.add_argument("--full", action="store_true", help="besides the headline: parity gate, traffic passes, one-stream pass, extra configs, "
                    "from-bytes legs, CPU baseline (a plain run times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write a fixed, seeded sample of the last timed step's RGB to DIR/rgb.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-core CPU baseline (0 = every core the job may use: affinity mask capped by the cgroup quota)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip extra_configs, e2e_from_bytes and the traffic passes (main line only)")
    ap.add_argument("--no-traffic", action="store_true", help="with --full: do not run the rocprofv3 PMC passes that observe HBM traffic (roofline.traffic then comes from profiles/)")
    ap.add_argument("--traffic-images", type=int, default=256, help="pictures per launch in the PMC passes")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the oracle legs of the parity gate (the on-device check stays)")
    ap.add_argument("--parity-images", type=int, default=16, help="pictures of the timed batch checked against the CPU oracle (decoded in parallel on the host cores)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def algorithmic_bytes(kind, by, nsub_total, nblk):
    """Per-step algorithmic bytes of each kernel class; by = mjx.Batch.bytes().
    by["coef"] = bytes of the intermediate coefficient representation (4 per stream entry + 4 per block of DC).
    idct_color uses SURVEY.md s8(d)'s stage-B figure B_idct = 128*n_blocks + 3*W*H (6 B/px for 4:2:0); the kernel's
    real input is the smaller compact stream -- `algorithmic_bytes_physical` gives that variant."""
    S, rgb, coef = by["scan"], by["rgb"], by["coef"]
    state = 32 * nsub_total                       # entry + exit state per subsequence
    cps = 8 * 15 * nsub_total                     # two checkpoint words every 256 bits
    return {
        "gather": 2 * coef,                       # multi-scan pictures only: component streams in, picture stream out
        "huff_sync": S + state + cps,             # k_huff_spec: scan in, states + checkpoints out
        "huff_fix": S // 5 + state + cps // 5,    # k_huff_merge rounds: ~1/5 of the scan is re-read (median merge distance)
        "huff_scan": 24 * nsub_total,             # exit state in, block base + entry base out
        "huff_write": S + 24 * nsub_total + coef - 2 * nblk,  # scan + entry state + bases in, compact stream + 16-bit DC differences out
        # single decode (round 5): the emitting first decode reads the scan once plus the warm-up (an eighth of a subsequence more at
        # 1024 of 8192 bits), writes states, checkpoints at a quarter of the old density, the compact stream and one word per block
        "huff_emit": S + S // 8 + state + cps // 4 + coef,
        # ... the prefixes of the lanes whose entry was wrong (~5 % of the scan's symbols), then block words in, DC differences out
        "huff_prefix": S // 16 + state + 6 * nblk,
        "dc_scan": 6 * nblk,                      # 16-bit DC differences in, int32 predicted DC out
        "idct_color": 128 * nblk + rgb,           # B_idct
    }[kind]


def algorithmic_bytes_physical(kind, by, nsub_total, nblk):
    if kind == "idct_color":
        return by["coef"] + by["rgb"]             # compact stream + DC in, packed RGB out
    return algorithmic_bytes(kind, by, nsub_total, nblk)


KERNEL_ALIAS = {"k_huff_spec": "huff_sync", "k_huff_merge": "huff_fix", "k_huff_merge_tail": "huff_fix", "k_huff_merge_loop": "huff_fix",
                "k_huff_scan": "huff_scan", "k_huff_write": "huff_write", "k_idct_color": "idct_color", "k_ref_color": "idct_color",
                "k_dc_sums_t": "dc_scan", "k_dc_apply_t": "dc_scan", "k_dc_scan_t": "dc_scan", "k_dc_sums": "dc_scan",
                "k_dc_apply": "dc_scan", "k_dc_restart": "dc_scan", "k_planar_count": "gather", "k_planar_offsets": "gather",
                "k_planar_copy": "gather", "k_huff_emit": "huff_emit", "k_huff_prefix": "huff_prefix", "k_block_gather": "huff_prefix"}


def pmc_sum_by_class(directory, counters):
    """Sums of rocprofv3 --pmc counters over the dispatches of each decode kernel class: {class: {counter: value}}."""
    import collections, csv, glob
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    for f in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] not in counters:
                continue
            k = r["Kernel_Name"].split("(")[0].replace("void mjx::", "").split("<")[0].strip()
            if k in KERNEL_ALIAS:
                acc[KERNEL_ALIAS[k]][r["Counter_Name"]] += float(r["Counter_Value"])
    return {k: dict(v) for k, v in acc.items()}


# Units of a CU next to HBM (round-5 review, next #5): which one is busiest per kernel class.  Prices from tools/probes/op_cost_probe.hip
# (profiles/r06_op_costs.txt): a SIMD of gfx950 issues a wave64 v_add/mul/fma_f32, v_mov, v_and, v_add_u32 ... in 2 cycles when two or
# more of its waves have one ready (4 for a lone wave), and v_pk_*_f32, v_cvt_*, v_mad_*24, v_bfe, v_lshl_*, v_perm, v_cmp ... in 4
# cycles whatever the occupancy -- these kernels are made of the second kind, so the share is quoted at 4 cycles, with the 2-cycle
# figure beside it as the lower bound.  The chip's cycles during a dispatch = GRBM_GUI_ACTIVE / 8 (summed over the 8 XCDs, guide s.DVFS).
SQ_COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT", "SQ_WAVES", "GRBM_GUI_ACTIVE")
N_SIMD, N_CU, HBM_ACHIEVABLE_GBS = 1024, 256, 6300.0


def unit_shares(sq, hbm_bytes):
    """{class: shares of the chip's time its dispatches kept each unit busy} from the SQ pass (+ the traffic of the TCC passes)."""
    out = {}
    for k, c in sq.items():
        cyc = c.get("GRBM_GUI_ACTIVE", 0.0) / 8.0
        if cyc <= 0 or "SQ_INSTS_VALU" not in c:
            continue
        o = {"chip_cycles": int(cyc), "valu_insts": int(c["SQ_INSTS_VALU"]),
             "valu_issue_share_at_4_cycles": round(c["SQ_INSTS_VALU"] * 4.0 / (N_SIMD * cyc), 3),
             "valu_issue_share_at_2_cycles": round(c["SQ_INSTS_VALU"] * 2.0 / (N_SIMD * cyc), 3),
             "lds_active_share": round(c.get("SQ_LDS_IDX_ACTIVE", 0.0) / (N_CU * cyc), 3),
             "lds_bank_conflict_share_of_active": round(c.get("SQ_LDS_BANK_CONFLICT", 0.0) / max(c.get("SQ_LDS_IDX_ACTIVE", 0.0), 1.0), 3)}
        if k in hbm_bytes and c.get("ms"):
            o["ms_in_pmc_pass"] = round(c["ms"], 4)
            o["clock_GHz_in_pmc_pass"] = round(cyc / (c["ms"] * 1e6), 3)
            o["hbm_share_of_achievable"] = round(hbm_bytes[k] / (c["ms"] / 1e3) / 1e9 / HBM_ACHIEVABLE_GBS, 3)
        cand = {"valu_issue": o["valu_issue_share_at_4_cycles"], "lds": o["lds_active_share"], "hbm": o.get("hbm_share_of_achievable", 0.0)}
        o["busiest_unit"] = max(cand, key=cand.get)
        out[k] = o
    return out


def pmc_bytes_by_class(directory, counter):
    """Sum of a rocprofv3 --pmc counter (KB) over the dispatches of each decode kernel class, in bytes."""
    import collections, csv, glob
    acc = collections.defaultdict(float)
    for f in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            k = r["Kernel_Name"].split("(")[0].replace("void mjx::", "").split("<")[0].strip()
            if k in KERNEL_ALIAS:
                acc[KERNEL_ALIAS[k]] += float(r["Counter_Value"]) * 1024.0
    return dict(acc)


def profiler_attached():
    """True when this process runs under rocprofv3 / rocprof (its tool library is preloaded into us and would be inherited by
    every child): the nested PMC passes of observe_traffic() would then compete with the outer collection for the counter
    hardware and pollute its dispatch list, so they are skipped."""
    pre = os.environ.get("LD_PRELOAD", "")
    if "rocprof" in pre or "roctracer" in pre or "rocprofiler" in pre:
        return True
    return any(k.startswith(("ROCP_", "ROCPROF", "ROCPROFILER_", "ROCTRACER_")) for k in os.environ)


def observe_traffic(args):
    """HBM bytes per kernel class of one step, observed now: two rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE need separate
    passes: TCC counter slots) over a child `bench.py` of `--traffic-images` pictures, one stream (per-kernel counters mean
    something only without overlap), one step, no warm-up -- every decode kernel of the child runs exactly once.  FETCH_SIZE is
    doubled (gfx950 reports half the bytes of wide coalesced reads; for the narrow reads of the entropy kernels an upper bound).
    Returns ({class: bytes for the child's batch}, images, note) or None when rocprofv3 is missing or a pass fails."""
    import shutil, signal, subprocess, tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not exe:
        return None
    out = {}
    sq = None
    with tempfile.TemporaryDirectory(prefix="mjx_pmc_", dir="/tmp") as tmp:
        env = dict(os.environ, MJX_STREAMS="1", TMPDIR="/tmp")
        # (a third pass, SQ + GRBM counters: which unit of the CUs each kernel class keeps busiest -- unit_shares(); its failure
        # costs the line that object only)
        for counter in ("FETCH_SIZE", "WRITE_SIZE", "SQ"):
            d = os.path.join(tmp, counter)
            pmc = list(SQ_COUNTERS) if counter == "SQ" else [counter]
            cmd = [exe, "--pmc"] + pmc + ["-d", d, "-o", "out", "--output-format", "csv", "--", sys.executable, os.path.join(ROOT, "bench.py"),
                   "--no-cpu-baseline", "--no-extra", "--no-parity", "--steps", "1", "--warmup", "0", "--images-per-gpu", str(args.traffic_images),
                   "--width", str(args.width), "--height", str(args.height), "--subsampling", args.subsampling, "--quality", str(args.quality),
                   "--unique", str(min(args.unique, args.traffic_images))]
            child_out = os.path.join(tmp, counter + ".stdout")
            try:
                with open(child_out, "w") as fo:
                    p = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=fo, stderr=subprocess.DEVNULL, start_new_session=True)
                    try:
                        rc = p.wait(timeout=180)
                    except subprocess.TimeoutExpired:
                        os.killpg(p.pid, signal.SIGKILL)          # (the group this call started, nothing else)
                        p.wait()
                        rc = -1
            except OSError:
                rc = -1
            if counter == "SQ":
                if rc == 0:
                    try:
                        sq = pmc_sum_by_class(d, set(SQ_COUNTERS))
                        line = [l for l in open(child_out) if l.startswith("{")][-1]
                        for k, v in json.loads(line)["kernels"].items():        # the pass's own HIP-event times: the clock it ran at
                            if k in sq:
                                sq[k]["ms"] = v["ms"]
                    except Exception:
                        sq = None
                continue
            if rc != 0:
                return None
            out[counter] = pmc_bytes_by_class(d, counter)
    if not out["FETCH_SIZE"] or not out["WRITE_SIZE"]:
        return None
    # (the classes are SUMMED over the child's dispatches -- a batch of two chunks launches every kernel twice -- so the figure
    # is per step of `traffic_images` pictures whatever the chunking)
    classes = sorted(set(out["FETCH_SIZE"]) | set(out["WRITE_SIZE"]))
    per = {k: {"fetch_bytes": int(2 * out["FETCH_SIZE"].get(k, 0)), "write_bytes": int(out["WRITE_SIZE"].get(k, 0)),
               "hbm_bytes": int(2 * out["FETCH_SIZE"].get(k, 0) + out["WRITE_SIZE"].get(k, 0))} for k in classes}
    units = unit_shares(sq, {k: v["hbm_bytes"] for k, v in per.items()}) if sq else None
    return (per, args.traffic_images, "observed in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, FETCH x 2), "
            "%d pictures, one stream, one step" % args.traffic_images, units)


def committed_traffic():
    """The last PMC collection committed under profiles/ (tools/collect_traffic.py), as observe_traffic() returns it."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    if not files:
        return None
    t = json.load(open(files[-1]))
    if t.get("basis") != "per_step":
        # collections before round 5 averaged per LAUNCH; with two chunks per batch that is half a step's traffic under an
        # "images_per_launch" that names the whole batch (round-4 review, weak #7): refuse them rather than scale them
        return None
    k = dict(t["kernels"])
    if "huff_fix_tail" in k:                                   # (older collections list the straggler kernel on its own, per launch)
        k["huff_fix"] = {f: 6 * (k["huff_fix"][f] + k["huff_fix_tail"][f]) for f in ("fetch_bytes", "write_bytes", "hbm_bytes")}
    k = {c: v for c, v in k.items() if c in set(KERNEL_ALIAS.values())}
    return k, t["images_per_step"], "committed collection profiles/%s (not observed in this run)" % os.path.basename(files[-1]), t.get("units")


def shard_seeds(rank, world, unique):
    """Content seeds of this rank's images: global image i goes to rank i % world and has seed i % unique, so the
    rank sees the periodic sequence (rank + world*j) % unique; returns one period."""
    seeds, j = [], 0
    while True:
        s = (rank + world * j) % unique
        if j > 0 and s == seeds[0]:
            break
        seeds.append(s)
        j += 1
    return seeds


def reduce_elapsed(elapsed, world):
    """MAX over ranks of the timed region: a host-side reduction over gloo (the data path has no collective at all)."""
    if world <= 1:
        return elapsed
    import torch
    import torch.distributed as dist
    t = torch.tensor([elapsed], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


KERNEL_CLASSES = ["gather", "huff_sync", "huff_fix", "huff_scan", "huff_write", "dc_scan", "idct_color", "huff_emit", "huff_prefix"]


def reduce_record(rec, world):
    """N > 1: the timed region's wall clock and every kernel class's HIP-event time become the MAX over the ranks (the slowest GPU
    sets the job's rate, and the roofline objects of the line are computed from the reduced record); launches are the same on
    every rank (same workload)."""
    if world <= 1:
        return rec
    import torch
    import torch.distributed as dist
    t = torch.tensor([rec["elapsed"]] + [rec["kernels"].get(k, {"ms": 0.0})["ms"] for k in KERNEL_CLASSES], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    out = dict(rec, elapsed=float(t[0].item()), kernels={k: dict(v) for k, v in rec["kernels"].items()})
    for j, k in enumerate(KERNEL_CLASSES):
        if k in out["kernels"]:
            out["kernels"][k]["ms"] = round(float(t[1 + j].item()), 4)
    return out


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes show 256
    logical CPUs but run the job under a 16-CPU quota; threads beyond the quota only add contention)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(period)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / period
        except (OSError, ValueError):
            pass
    if quota:
        n = max(1, min(n, int(quota + 0.5)))
    return n, quota


def cpu_baseline(datas, width, height, threads, keep_rgb):
    """The reference's algorithm restated in C (oracle/, kind "port"), bug-compatible layout, cosf per term and linear-search
    Huffman like the Rust code: one picture per thread on every host core, then one picture on one core.  Returns the JSON
    object and the first `keep_rgb` pictures (for the REF_COMPAT leg of the parity gate)."""
    import oracle_binding as orc
    cores = os.cpu_count() or 1
    usable, quota = usable_cores()
    threads = max(1, min(threads or usable, 1024))
    sample = [datas[i % len(datas)] for i in range(threads)]
    keep_rgb = min(keep_rgb, len(sample))
    shapes = [(height, width)] * keep_rgb + [(1, 1)] * (len(sample) - keep_rgb)       # (RGB kept for the parity gate)
    t = time.perf_counter()
    px, st, rgbs = orc.decode_many(sample, threads, layout=orc.LAYOUT_REF, faithful=True, rgb_shapes=shapes)
    dt = time.perf_counter() - t
    ok = sum(1 for s in st if s == 0)
    t = time.perf_counter()
    px1, st1 = orc.decode_many(sample[:1], 1, layout=orc.LAYOUT_REF, faithful=True)
    dt1 = time.perf_counter() - t
    out = {
        "value": round(px / dt / 1e6, 4), "unit": "Mpixels/s", "cores": threads, "kind": "port",
        "one_core": {"value": round(px1 / dt1 / 1e6, 4), "unit": "Mpixels/s", "cores": 1, "seconds": round(dt1, 2)},
        "host": {"nproc": cores, "cpu_model": cpu_model(), "usable_cores": usable, "cgroup_cpu_quota": quota},
        "extrapolated_full_batch_s": {"this_run_batch": None, "config5_16384x4K": round(16384 * 3840 * 2160 / (px / dt), 1),
                                      "note": "linear: pixels of the batch / the all-core rate above (SURVEY s8(d))"},
        "sample": "%d pictures of the same %dx%d batch, one per thread on %d threads = every core the job may use (host: %d logical "
                  "CPUs, cgroup quota %s), reference algorithm restated "
                  "in C (oracle/: O(n^4) float IDCT with cosf per term, linear-search Huffman, the reference's own layout; "
                  "gcc -O2 -ffp-contract=off) -- not the Rust binary, which cannot be built here; %d decoded ok in %.1f s; "
                  "then 1 picture on 1 thread in %.1f s" % (len(sample), width, height, threads, cores, quota, ok, dt, dt1),
    }
    return out, [rgbs[i] for i in range(min(keep_rgb, len(rgbs))) if st[i] == 0], sample[:keep_rgb]


def host_threads():
    """Threads of the host-side pools (synthesis, parsing): the cores the job may use, at most 32."""
    return min(32, usable_cores()[0])


def make_inputs(mjx, width, height, subsampling, quality, seeds):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(host_threads()) as ex:
        return list(ex.map(lambda s: mjx.synth_jpeg(width, height, subsampling, quality, s), seeds))


DUMP_SEED, DUMP_PICTURES, DUMP_PIXELS = 1234, 16, 1 << 18


def dump_sample(n_pictures, pixels_per_picture):
    """The sample --dump-outputs writes: sorted picture indices of the batch and sorted row-major pixel indices within a
    picture (every pixel of pictures of at most DUMP_PIXELS), drawn from DUMP_SEED -- the same for the same arguments."""
    import numpy as np
    rng = np.random.default_rng(DUMP_SEED)
    pics = np.sort(rng.choice(n_pictures, size=min(n_pictures, DUMP_PICTURES), replace=False))
    if pixels_per_picture <= DUMP_PIXELS:
        return pics, np.arange(pixels_per_picture)
    return pics, np.sort(rng.choice(pixels_per_picture, size=DUMP_PIXELS, replace=False))


def dump_outputs(batch, directory):
    """--dump-outputs: DIR/rgb.npy = float32 [pictures, pixels, 3], the decoded RGB of the pictures and pixels dump_sample()
    picks (the pictures of a bench batch share one geometry): at most 16 x 2^18 x 3 x 4 B = 50 MB."""
    import numpy as np
    inf = batch.info(0)
    pics, px = dump_sample(len(batch), inf["width"] * inf["height"])
    rgb = np.stack([batch.rgb(int(i)).reshape(-1, 3)[px] for i in pics]).astype(np.float32)
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "rgb.npy"), rgb)


def _any_rank(value):
    """MAX of `value` over the ranks of a torch.distributed.run launch (the value itself at N = 1)."""
    try:
        import torch
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([int(value)], dtype=torch.int64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return int(t.item())
    except ImportError:
        pass
    return int(value)


def run_config(mjx, ctx, datas, per_gpu, stages, steps, warmup, chunk_images=0, device_destuff=False, sync_all=None,
               parity_images=0, host_side=None, latency_pass=False, compare_tiled=True, dump_dir=None):
    """Builds the device-resident batch (unique pictures uploaded once, tiled on the device), times `steps` passes, writes
    dump_outputs() to `dump_dir` and, with `compare_tiled`, runs the on-device half of the parity gate.  Returns (record, batch)
    -- the caller closes the batch."""
    from concurrent.futures import ThreadPoolExecutor
    period = len(datas)
    reps = max(1, per_gpu // period)
    per_gpu = reps * period
    t_h = time.perf_counter()
    with ThreadPoolExecutor(host_threads()) as ex:
        scans = list(ex.map(lambda d: mjx.ParsedScan(d, device_destuff=device_destuff), datas))
    t_parse = time.perf_counter() - t_h
    keep = stages == "pixels"
    t_h = time.perf_counter()
    base = mjx.Batch(ctx, scans, keep_coefs=keep, chunk_images=chunk_images)
    t_create = time.perf_counter() - t_h
    assert all(s == mjx.OK for s in base.create_status), base.create_status
    if host_side is not None:
        one = {}
        for rnd in range(3):                    # one thread, file after file: the host leg per file; the two modes in turn, the best of three
            for label, dd in (("host_destuff", False), ("device_destuff", True)):    # (a single pass right after the upload measured the box, not the parser:
                t1 = time.perf_counter()                                               # the round-3 driver run had the two the wrong way round)
                for d in datas:
                    mjx.ParsedScan(d, device_destuff=dd).close()
                v = round(1e3 * (time.perf_counter() - t1) / len(datas), 4)
                one[label] = v if label not in one else min(one[label], v)
        host_side.update({"files": len(datas), "parse_ms_per_file": round(1e3 * t_parse / len(datas), 3),
                          "parse_ms_per_file_one_thread": one,
                          "parse_threads": host_threads(),
                          "create_ms_per_file": round(1e3 * t_create / len(datas), 3),
                          "compressed_MB_per_file": round(sum(len(d) for d in datas) / len(datas) / 1e6, 3),
                          "note": "host marker walk + de-stuffing (threads), then planning + decode tables + H2D of the compressed "
                                  "scans and first-use allocations (mjx_batch_create) for the unique files; not part of `value`"})
    up_ms, up_n = base.kernel_ms().get("upload", (0.0, 0))
    batch = base.tile(reps) if reps > 1 else base
    if batch is not base:
        base.close()
    for s in scans:
        s.close()
    geo = batch.geometry()
    nsub_total, nblk = geo["subsequences"], geo["blocks"]
    st = mjx.STAGE_ALL if stages == "all" else mjx.STAGE_PIXELS
    if stages == "pixels":
        batch.decode(mjx.STAGE_ALL)
        batch.wait()
    for _ in range(warmup):
        batch.decode(st)
        batch.wait()
    # The steps are enqueued back to back and waited for once, and mjx_batch_wait repairs the LAST decode only: a step whose
    # synchronisation rounds had not converged skipped its pictures (no stream, no stage B) and would count as a fast step.  The
    # library counts such runs; a timed region that holds one is not a measurement.  The wait that found it has repaired the batch
    # and told its chunks how many rounds they need (Chunk::learned_passes), so the region is simply timed again -- at most twice.
    retimed = 0
    while True:
        batch.kernel_ms(reset=True)
        unconv0 = batch.unconverged_runs()
        if sync_all:
            sync_all()
        t0 = time.perf_counter()
        for _ in range(steps):
            batch.decode(st)
        batch.wait()
        if sync_all:
            sync_all()
        elapsed = time.perf_counter() - t0
        unconv = batch.unconverged_runs() - unconv0
        # (every rank must take the same decision: the region is bracketed by barriers)
        if not _any_rank(unconv) or retimed == 2 or os.environ.get("MJX_BENCH_IGNORE_STATUS"):
            break
        retimed += 1
    assert unconv == 0 or os.environ.get("MJX_BENCH_IGNORE_STATUS"), \
        "%d chunk runs of the timed region had not converged when their pictures were due: the steps did not do the whole work" % unconv
    # (round-4 review, weak #10: the figure above is the pipelined rate -- `steps` passes enqueued back to back, one wait;
    # the latency of ONE pass, enqueue to the end of its last kernel, measured on its own)
    bad = [i for i in range(len(batch)) if batch.status(i) != mjx.OK]
    assert not bad or os.environ.get("MJX_BENCH_IGNORE_STATUS"), "images failed: %s" % bad[:8]     # (the switch: measurement builds that decode garbage)
    kms = batch.kernel_ms(reset=True)           # (the timed region's kernels; the pass below is not among them)
    if dump_dir:
        dump_outputs(batch, dump_dir)
    one_pass = 0.0
    if latency_pass:                            # (not in the PMC / rocprof runs: their collections must hold exactly `steps` passes)
        t1 = time.perf_counter()
        batch.decode(st)
        batch.wait()
        one_pass = time.perf_counter() - t1
    by = batch.bytes()
    kernels = {k: {"launches": v[1], "ms": round(v[0], 4)} for k, v in kms.items() if v[1]}
    kernels.pop("upload", None)                   # (upload-time kernels of a batch that was not tiled: not part of a step)
    rec = {"elapsed": elapsed, "unconverged_chunk_runs": int(unconv), "timed_again_after_a_repair": retimed, "one_pass_ms": round(one_pass * 1e3, 4), "per_gpu": per_gpu, "period": period, "by": by, "kernels": kernels, "nsub": nsub_total, "nblk": nblk,
           "chunks": geo["chunks"],
           "upload_side": {"kernels_ms_unique": round(up_ms, 4), "unique_pictures": period, "launches": int(up_n),
                           "ms_per_batch": round(up_ms * per_gpu / max(period, 1), 4), "pictures_per_batch": per_gpu,
                           "device_destuff": bool(device_destuff),
                           "note": "HIP-event time of upload-time kernels for the unique pictures, scaled to the batch.  Since round 5 "
                                   "mjx_batch_create lays the de-stuffed scans out lane-interleaved on the host while it packs them for the "
                                   "transfer (build_batch / host_interleave_columns), so no kernel runs at upload and this is 0; with "
                                   "--device-destuff the de-stuffing kernels and k_scan_interleave run here (MJX_HOST_INTERLEAVE=0: "
                                   "k_scan_interleave for every scan, as before round 5)"}}
    # on-device half of the parity gate: every picture of the batch equals its unique original bit for bit
    n = len(batch)
    if compare_tiled and n > period:
        mx, cnt = batch.compare_rgb(list(range(period, n)), batch, [i % period for i in range(period, n)])
        rec["tiled_compared"] = int(n - period)
        rec["tiled_max_abs_diff"] = int(mx.max())
        rec["tiled_differing_bytes"] = int(cnt.sum())
    else:
        rec["tiled_compared"], rec["tiled_max_abs_diff"], rec["tiled_differing_bytes"] = 0, 0, 0
    return rec, batch


def rooflines(rec, steps, stages, traffic=None):
    """The roofline objects of one timed configuration (see the module docstring).  `traffic` = (per-class bytes, images they
    were collected on, source note) or None."""
    kernels, by, nsub_total, nblk = rec["kernels"], rec["by"], rec["nsub"], rec["nblk"]
    out = {}
    if not kernels:
        return out
    dom = max(kernels, key=lambda k: kernels[k]["ms"])          # largest event time in this timed region
    n_launch = kernels[dom]["launches"]
    avg_s = kernels[dom]["ms"] / 1e3 / n_launch
    per_launch = algorithmic_bytes(dom, by, nsub_total, nblk) * steps / n_launch
    per_launch_phys = algorithmic_bytes_physical(dom, by, nsub_total, nblk) * steps / n_launch
    ach = per_launch / avg_s / 1e9
    ach_phys = per_launch_phys / avg_s / 1e9
    scale = (rec["per_gpu"] / traffic[1]) if traffic else 0.0      # the collection's pictures -> one step of this batch
    def tr_step(kind):
        return int(traffic[0][kind]["hbm_bytes"] * scale) if traffic and kind in traffic[0] else None
    dom_obj = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(ach / HBM_PEAK_GBS, 5), "bytes_per_launch": int(per_launch), "avg_launch_ms": round(avg_s * 1e3, 5),
               "launches_per_step": round(n_launch / steps, 2), "traffic_per_step": tr_step(dom),
               "achieved_physical": round(ach_phys, 2), "frac_physical": round(ach_phys / HBM_PEAK_GBS, 5),
               "bytes_basis": "SURVEY s8(d) B_idct = 128*n_blocks + 3*W*H; *_physical: compact stream + DC + RGB, what the kernel moves"
               if dom == "idct_color" else "DESIGN.md s5"}
    out["kernel_rooflines"] = {}
    for k, v in kernels.items():
        if v["ms"] <= 0:
            continue
        gbs = algorithmic_bytes(k, by, nsub_total, nblk) * steps / (v["ms"] / 1e3) / 1e9
        o = {"GB/s": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4), "ms_per_step": round(v["ms"] / steps, 4), "traffic_per_step": tr_step(k)}
        if k == "idct_color":
            gp = algorithmic_bytes_physical(k, by, nsub_total, nblk) * steps / (v["ms"] / 1e3) / 1e9
            o.update({"GB/s_physical": round(gp, 1), "frac_physical": round(gp / HBM_PEAK_GBS, 4)})
        out["kernel_rooflines"][k] = o
    tot_ms = sum(v["ms"] for v in kernels.values())
    wall_ms = rec["elapsed"] / steps * 1e3
    if stages == "all":
        # the whole path on its compulsory traffic -- compressed bytes in, packed RGB out -- over the wall clock of
        # the timed region (not the sum of the kernel durations: the kernels of three streams overlap)
        e2e_bytes = by["scan"] + by["rgb"]
        e2e = e2e_bytes * steps / rec["elapsed"] / 1e9
        tot_traffic = sum(tr_step(k) or 0 for k in kernels) if traffic else None
        # what this design could reach at the bytes it really moves: its traffic at the ~6.3 TB/s the guide measures as achievable
        # (round-5 review, next #5) -- frac is what it reaches, ceiling_frac what it could, 0.60 what the north star asks
        ceiling_ms = tot_traffic / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3 if tot_traffic else None
        out["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": round(e2e, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(e2e / HBM_PEAK_GBS, 5), "traffic": tot_traffic,
                           "ceiling_ms_per_step": round(ceiling_ms, 3) if ceiling_ms else None,
                           "ceiling_frac": round(e2e_bytes / (ceiling_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4) if ceiling_ms else None,
                           "ceiling_definition": "traffic / 6.3 TB/s (HBM rate a copy reaches on MI355X): the step time, and the fraction of "
                                                 "the 8 TB/s roofline, this design would reach if every byte it moves moved at that rate",
                           "busiest_unit_per_kernel": (traffic[3] if traffic and len(traffic) > 3 else None),
                           "traffic_source": traffic[2] if traffic else None,
                           "bytes_per_step": int(e2e_bytes), "wall_ms_per_step": round(wall_ms, 4),
                           "kernel_ms_per_step_summed": round(tot_ms / steps, 4),
                           "definition": "SURVEY s8(d): sum over the images of B_e2e = S + 3*W*H per step / wall time per step of the timed "
                                         "region / 8 TB/s; `kernel` = the class with the largest HIP-event time in the timed region (its "
                                         "own per-launch figures: dominant_kernel); traffic = HBM bytes per step, all decode kernels",
                           "dominant_kernel": dom_obj}
    else:
        # the config-4 "HBM-bound IDCT sweep": stage B alone on B_idct
        out["roofline"] = dict(dom_obj, traffic=tr_step(dom), traffic_source=traffic[2] if traffic else None,
                               wall_ms_per_step=round(wall_ms, 4),
                               definition="SURVEY s8(d), stage B in isolation: B_idct = 128*n_blocks + 3*W*H per launch / the kernel's average launch duration / 8 TB/s")
    return out


def oracle_parity(mjx, batch, datas, period, k):
    """Pictures of the timed batch against the CPU oracle (STANDARD layout = what the batch was decoded in): the
    coefficient stream must be equal (T0), the RGB within 1 (T2).  The pictures are taken from the batch's last chunk, whose
    coefficients are still resident after the timed passes."""
    import numpy as np
    import oracle_binding as orc
    n = len(batch)
    picks = [n - 1 - j * max(1, period // max(k, 1)) for j in range(k)]
    picks = sorted({i for i in picks if 0 <= i < n})
    res = {"images": len(picks), "max_abs_diff": 0, "t0_equal": True, "differing_fraction": 0.0}
    diffs = 0
    total = 0
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(len(picks), usable_cores()[0]))) as ex:      # (the C call releases the GIL: one picture per core)
        refs = list(ex.map(lambda i: orc.decode(datas[i % period], layout=orc.LAYOUT_STD), picks))
    for i, ref in zip(picks, refs):
        try:
            t0 = bool(np.array_equal(batch.coefs(i), orc.interleave(ref)))
        except mjx.MjxError:
            t0 = None                     # picture not in the resident chunk
        if t0 is False:
            res["t0_equal"] = False
        d = np.abs(batch.rgb(i).astype(np.int16) - ref.rgb.astype(np.int16))
        res["max_abs_diff"] = max(res["max_abs_diff"], int(d.max()))
        diffs += int((d > 0).sum())
        total += d.size
    res["differing_fraction"] = round(diffs / max(total, 1), 6)
    return res


def ref_compat_parity(mjx, ctx, files, rgbs):
    """The pictures the cpu_baseline leg decoded (the reference's own layout, cosf per term) against a REF_COMPAT decode of
    the same files on the GPU: RGB within 1."""
    import numpy as np
    if not files:
        return {"images": 0, "max_abs_diff": 0}
    scans = [mjx.ParsedScan(d) for d in files]
    b = mjx.Batch(ctx, scans, layout=mjx.LAYOUT_REF_COMPAT)
    b.decode()
    b.wait()
    mx = 0
    for i, ref in enumerate(rgbs):
        assert b.status(i) == mjx.OK, "REF_COMPAT decode failed: %d" % b.status(i)
        mx = max(mx, int(np.abs(b.rgb(i).astype(np.int16) - ref.astype(np.int16)).max()))
    b.close()
    for s in scans:
        s.close()
    return {"images": len(rgbs), "max_abs_diff": mx}


def e2e_from_bytes(mjx, ctx, datas, n_files, width, height):
    """mjx_decode_batch: JPEG file bytes in host memory -> RGB in HBM (marker walk + de-stuffing on host threads, planning,
    H2D of the compressed scans, kernels).  Timed end to end after one warm-up call (the context keeps its pinned arena);
    with the stuffing removed on the host, on the GPU (the host copies the entropy-coded bytes untouched), and as the library chooses."""
    files = [datas[i % len(datas)] for i in range(n_files)]
    out = {}
    for label, dd in (("host_destuff", False), ("device_destuff", True), ("library_default", None)):
        best = None
        for _ in range(4):
            t = time.perf_counter()
            b, st = mjx.decode_batch(ctx, files, device_destuff=dd)
            dt = time.perf_counter() - t
            assert all(s == mjx.OK for s in st)
            b.close()
            best = dt if best is None or dt < best else best
        out[label] = {"ms": round(best * 1e3, 2), "Mpixels/s": round(n_files * width * height / best / 1e6, 1), "files/s": round(n_files / best, 1)}
    out.update(out["library_default"])
    out.update({"files": n_files, "compressed_MB": round(sum(len(f) for f in files) / 1e6, 1),
                "note": "host bytes -> device RGB through mjx_decode_batch, best of 4 calls; PCIe-inclusive, never part of `value`; "
                        "top-level ms / Mpixels/s: opts.device_destuff = MJX_DESTUFF_AUTO, the library's choice (the GPU for lists of 64 MB and more)"})
    return out


def e2e_pool(mjx, datas, files_per_device, width, height):
    """The library's own multi-GPU front (per-GPU host thread + work queue, no collective): ONE process,
    mjx_pool_decode_batch over every visible device, `files_per_device` files per slot dealt by compressed bytes -- the path a
    caller of the C ABI would use on an 8-GPU node, and the one whose host side (parse threads shared by the slots under the
    job's CPU quota) bounds the node's rate from file bytes.  Best of 3 calls after a warm-up; per slot the wall clock of its own
    mjx_decode_batch, its parse threads and NUMA node (mjx_pool_result_slot_ms / mjx_pool_result_host)."""
    import torch
    ndev = torch.cuda.device_count()
    n_files = files_per_device * ndev
    files = [datas[i % len(datas)] for i in range(n_files)]
    pool = mjx.Pool(list(range(ndev)))
    best, slots = None, None
    try:
        for it in range(4):
            t = time.perf_counter()
            res = pool.decode_batch(files)
            dt = time.perf_counter() - t
            ok = res.rc == mjx.OK and all(s == mjx.OK for s in res.status)
            info = []
            for s in range(ndev):
                thr, node = res.host(s)
                info.append({"slot": s, "device": pool.device(s), "files": sum(1 for x in res.slot_of if x == s), "ms": round(res.slot_ms(s), 2),
                             "parse_threads": thr, "numa_node": node})
            res.close()
            assert ok, "mjx_pool_decode_batch failed"
            if it > 0 and (best is None or dt < best):
                best, slots = dt, info
    finally:
        pool.close()
    # the host bound made visible (round-5 review, weak #8 / next #8): one thread's marker walk + de-stuffing rate on these files,
    # and what the slots' parse threads together could feed -- an 8-GPU node is host-bound when that is below 8 x the resident rate
    parse = {}
    for label, dd in (("host_destuff", False), ("device_destuff", True)):      # (the library takes the second for lists of 64 MB and more)
        t = time.perf_counter()
        probe = [mjx.ParsedScan(d, device_destuff=dd) for d in files[:64]]
        parse[label] = (time.perf_counter() - t) / len(probe)
        for sc in probe:
            sc.close()
    parse_s = parse["device_destuff"] if sum(len(f) for f in files) >= (64 << 20) else parse["host_destuff"]
    threads_total = sum(s["parse_threads"] for s in slots)
    for s in slots:
        s["files_per_s_per_parse_thread"] = round(s["files"] / (s["ms"] / 1e3) / max(s["parse_threads"], 1), 1) if s["ms"] > 0 else None
    return {"devices": ndev, "files": n_files, "ms": round(best * 1e3, 2), "Mpixels/s": round(n_files * width * height / best / 1e6, 1),
            "files/s": round(n_files / best, 1), "slots": slots,
            "parse_ms_per_file_one_thread": {k: round(v * 1e3, 4) for k, v in parse.items()}, "parse_files_per_s_per_thread": round(1.0 / parse_s, 1),
            "parse_threads_total": threads_total, "host_parse_bound_files_per_s": round(threads_total / parse_s, 1),
            "note": "one process, mjx_pool_decode_batch over all visible devices (host bytes -> RGB resident on the device that decoded "
                    "it), best of 3 calls; PCIe-inclusive, never part of `value`; slots[].ms = wall clock of the slot's own mjx_decode_batch"}


def build_unless_read_only(ge):
    """build() brings the native libraries up to date under lock files it creates in the tree.  A checkout this user may not
    write (built by another user) is measured as build() left it: nothing can be rebuilt there, and the package's loaders
    still refuse a tree in which a library was never built."""
    import errno
    try:
        ge.build()
    except OSError as e:
        if e.errno not in (errno.EACCES, errno.EPERM, errno.EROFS):
            raise
        sys.stderr.write("bench.py: the tree is not writable here (%s); measuring the libraries build() left\n" % e)


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    import torch                       # (first: libmjx.so must find torch's HIP runtime already loaded, not bring its own)
    import torch.distributed as dist
    import __graft_entry__ as ge
    build_unless_read_only(ge)
    # ---- HBM traffic of one step, observed with rocprofv3 PMC passes in child processes (before this process touches the GPU) ----
    full = args.full
    traffic = None
    if full and rank == 0 and world == 1 and not args.no_extra and not args.no_traffic and args.stages == "all" and not profiler_attached():
        traffic = observe_traffic(args)
    if traffic is None and args.width == 3840 and args.height == 2160 and args.quality == 75 and args.subsampling == "420":
        traffic = committed_traffic()            # (collected on this workload; other workloads: none)

    mjx = ge.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the decode path has no CPU fallback")
    device = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device)
    if world > 1:
        # host-side rendezvous only: ranks never exchange image data (north star: per-GPU work queues, no RCCL)
        dist.init_process_group(os.environ.get("MJX_BENCH_BACKEND", "gloo"))

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- this rank's shard of the global batch: global image i -> rank i % world, content seed i % unique ----
    seeds = shard_seeds(rank, world, args.unique)
    datas = make_inputs(mjx, args.width, args.height, args.subsampling, args.quality, seeds)
    if args.streams:
        os.environ["MJX_STREAMS"] = str(args.streams)
    ctx = mjx.Context(device, profiling=True, throughput_plan=True)       # (the batches are tiled from 64 unique pictures: cut them like the batch they become)
    host_side = {}
    rec, batch = run_config(mjx, ctx, datas, args.images_per_gpu, args.stages, args.steps, args.warmup, args.chunk_images,
                            args.device_destuff, sync_all, host_side=host_side if full else None,
                            latency_pass=full and not args.no_extra, compare_tiled=full,
                            dump_dir=args.dump_outputs if rank == 0 else None)
    rec = reduce_record(rec, world)            # N > 1: MAX over the ranks of the wall clock and of every kernel class's time
    per_gpu, period, by, kernels = rec["per_gpu"], rec["period"], rec["by"], rec["kernels"]
    elapsed = rec["elapsed"]
    total_px = by["pixels"] * world * args.steps
    value = total_px / elapsed / 1e6
    out = {
        "metric": "Mpixels/sec decode, 4K 4:2:0 baseline batch", "value": round(value, 2), "unit": "Mpixels/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "one_pass_latency_ms": rec["one_pass_ms"] or None,
        "unconverged_chunk_runs": rec["unconverged_chunk_runs"],       # (0, or the line is refused: every timed step did the whole work)
        "timed_again_after_a_repair": rec["timed_again_after_a_repair"],   # (times the region was measured again because a step had not converged)
        "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%d x %dx%d %s baseline JPEG q%d per GPU (%d unique, tiled on device), de-stuffed scans "
                               "resident in HBM, RGB out in HBM, stages=%s"
                               % (per_gpu, args.width, args.height, SUBS[args.subsampling], args.quality, period, args.stages),
                   "images_per_gpu": per_gpu, "width": args.width, "height": args.height, "subsampling": args.subsampling,
                   "quality": args.quality, "layout": "standard", "streams": args.streams or "library default",
                   "chunks_per_step": rec["chunks"],
                   "subsequence_bytes": round(by["scan"] / max(rec["nsub"], 1), 1),      # mean scan bytes per lane of the entropy kernels (512..640: the throughput cut)
                   "sharding": "image i -> gpu i %% %d, no collective (harness barrier over gloo)" % world},
        "entropy_Gbit_per_s": round(by["scan"] * 8 * world * args.steps / elapsed / 1e9, 2),
        "bits_per_pixel": round(by["scan"] * 8 / max(by["pixels"], 1), 4),
        "kernels": kernels,
    }
    if full:
        out["host_side"] = host_side
    out["upload_side"] = rec["upload_side"]
    if rec["upload_side"]["ms_per_batch"] > 0:
        out["upload_side"]["value_with_interleave_in_the_step"] = round(by["pixels"] * world / ((elapsed / args.steps) + rec["upload_side"]["ms_per_batch"] / 1e3) / 1e6, 2)

    # ---- parity gate, --full: every number of the full line stands behind it ----
    parity = {"tiled_images_compared_on_device": rec["tiled_compared"], "tiled_max_abs_diff": rec["tiled_max_abs_diff"],
              "tiled_differing_bytes": rec["tiled_differing_bytes"]}
    failures = []
    if rec["tiled_max_abs_diff"] != 0:
        failures.append("tiled pictures differ from their originals")
    if full and not args.no_parity and args.stages == "all":
        op = oracle_parity(mjx, batch, datas, period, args.parity_images)
        parity.update({"images": op["images"], "max_abs_diff": op["max_abs_diff"], "t0_equal": op["t0_equal"],
                       "differing_fraction": op["differing_fraction"],
                       "oracle": "oracle/ (C restatement of the reference), STANDARD layout, pictures of the timed batch's last chunk"})
        if op["max_abs_diff"] > 1:
            failures.append("RGB differs from the oracle by %d" % op["max_abs_diff"])
        if not op["t0_equal"]:
            failures.append("coefficient stream differs from the oracle")
    batch.close()

    out.update(rooflines(rec, args.steps, args.stages, traffic))
    if full and not args.no_extra and args.streams != 1:
        # The library runs the entropy stages of two chunks and stage B on three streams (overlapped), so the kernel durations of the
        # timed region above include the contention between them.  The same workload on one stream gives every kernel's
        # stand-alone duration.
        os.environ["MJX_STREAMS"] = "1"
        ctx1 = mjx.Context(device, profiling=True, throughput_plan=True)
        os.environ.pop("MJX_STREAMS")
        iso_steps = max(2, min(args.steps, 3))
        r1, b1 = run_config(mjx, ctx1, datas, args.images_per_gpu, args.stages, iso_steps, 1, args.chunk_images, args.device_destuff, sync_all)
        b1.close()
        r1 = reduce_record(r1, world)
        rl1 = rooflines(r1, iso_steps, args.stages, traffic)
        out["roofline_isolated"] = dict(rl1["roofline"], note="same workload with MJX_STREAMS=1 (no overlap between the entropy stage and stage B): "
                                        "stand-alone kernel durations", steps=iso_steps,
                                        value_single_stream=round(r1["by"]["pixels"] * world * iso_steps / r1["elapsed"] / 1e6, 2))
        out["kernel_rooflines_isolated"] = rl1["kernel_rooflines"]
        if r1["tiled_max_abs_diff"] != 0:
            failures.append("single-stream pass: tiled pictures differ from their originals")
        ctx1.close()

    extra = []
    if full and not args.no_extra and world == 1 and args.stages == "all":
        small_steps = max(2, min(args.steps, 5))
        for name, w, h, q, n_img, stg in [("config4_1080p_whole_path", 1920, 1080, 75, 4096, "all"),
                                          ("config4_1080p_stage_B_only", 1920, 1080, 75, 4096, "pixels"),
                                          ("4K_q50", 3840, 2160, 50, 2048, "all"), ("4K_q90", 3840, 2160, 90, 2048, "all")]:
            d2 = datas if (w, h, q) == (args.width, args.height, args.quality) else make_inputs(mjx, w, h, "420", q, seeds)
            r2, b2 = run_config(mjx, ctx, d2, n_img, stg, small_steps, 1, sync_all=sync_all)
            b2.close()
            rl = rooflines(r2, small_steps, stg)
            px = r2["by"]["pixels"] * small_steps
            e = {"name": name, "workload": "%d x %dx%d 4:2:0 q%d, stages=%s" % (r2["per_gpu"], w, h, q, stg),
                 "Mpixels/s": round(px / r2["elapsed"] / 1e6, 1), "ms_per_step": round(r2["elapsed"] / small_steps * 1e3, 3),
                 "steps": small_steps,
                 "entropy_Gbit_per_s": round(r2["by"]["scan"] * 8 * small_steps / r2["elapsed"] / 1e9, 2),
                 "bits_per_pixel": round(r2["by"]["scan"] * 8 / max(r2["by"]["pixels"], 1), 4),
                 "roofline": {k: rl["roofline"][k] for k in ("kernel", "achieved", "frac", "wall_ms_per_step")},
                 "dominant_kernel": {k: (rl["roofline"]["dominant_kernel"] if stg == "all" else rl["roofline"])[k]
                                     for k in ("kernel", "achieved", "frac", "achieved_physical", "frac_physical", "avg_launch_ms")},
                 "tiled_images_compared_on_device": r2["tiled_compared"], "tiled_max_abs_diff": r2["tiled_max_abs_diff"]}
            if r2["tiled_max_abs_diff"] != 0:
                failures.append(name + ": tiled pictures differ from their originals")
            extra.append(e)
        out["extra_configs"] = extra
    if full and not args.no_extra and args.stages == "all":
        # from file bytes: every rank on its own GPU at the same time (N > 1: the ranks share the host's cores and its PCIe roots --
        # that contention is what the figure is for); the job's rate = all files / the slowest rank's time
        sync_all()
        e2e = e2e_from_bytes(mjx, ctx, datas, 512, args.width, args.height)
        if world > 1:
            t = torch.tensor([e2e[k]["ms"] for k in ("host_destuff", "device_destuff", "library_default")], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            for j, k in enumerate(("host_destuff", "device_destuff", "library_default")):
                ms = float(t[j].item())
                e2e[k] = {"ms": round(ms, 2), "Mpixels/s": round(world * 512 * args.width * args.height / ms / 1e3, 1), "files/s": round(world * 512 / ms * 1e3, 1)}
            e2e.update(e2e["library_default"])
            e2e["files"] = 512 * world
            e2e["note"] += "; N > 1: every rank decodes 512 files on its own GPU at the same time, ms = MAX over the ranks, rates = all ranks' files / that"
        out["e2e_from_bytes"] = e2e
        if world == 1:
            # (an extra: on a multi-GPU node this is the library's first contact with more than one physical device -- whatever
            # happens there must not cost the run its headline line)
            try:
                out["e2e_from_bytes_pool"] = e2e_pool(mjx, datas, 512, args.width, args.height)
            except Exception as e:          # noqa: BLE001
                out["e2e_from_bytes_pool"] = {"error": "%s: %s" % (type(e).__name__, e)}

    if full and rank == 0 and not args.no_cpu_baseline:
        # (N > 1: rank 0 times the CPU baseline while the other ranks wait at the closing barrier -- the host's cores are idle then,
        # as they are at N = 1; north star: "next to the reference CPU decoder timed on the same host cores in the same run")
        # (every picture the baseline leg decodes is kept and compared with a REF_COMPAT decode on the GPU)
        cb, ref_rgbs, ref_files = cpu_baseline(datas, args.width, args.height, args.cpu_threads, 0 if args.no_parity else 1 << 30)
        cb["extrapolated_full_batch_s"]["this_run_batch"] = round(total_px / args.steps / (cb["value"] * 1e6), 1)
        out["cpu_baseline"] = cb
        if not args.no_parity:
            rp = ref_compat_parity(mjx, ctx, ref_files[:len(ref_rgbs)], ref_rgbs)
            parity["ref_compat_images"] = rp["images"]
            parity["ref_compat_max_abs_diff"] = rp["max_abs_diff"]
            if rp["max_abs_diff"] > 1:
                failures.append("REF_COMPAT RGB differs from the CPU baseline's pictures by %d" % rp["max_abs_diff"])
    if full:
        parity["ok"] = not failures
        out["parity"] = parity
    ctx.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))
    if failures:
        raise SystemExit("PARITY GATE FAILED: " + "; ".join(failures))


if __name__ == "__main__":
    main()

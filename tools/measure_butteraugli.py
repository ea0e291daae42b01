#!/usr/bin/env python3
"""What the butteraugli distance of an image pair costs on the MI355X (profiles/butteraugli_pair.json).

    measure_butteraugli.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  The passes can be run by hand as well:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_butteraugli.py --trace-pass
    measure_butteraugli.py --time-pass --times-out TIMES.json
    measure_butteraugli.py --trace DIR --times TIMES.json

At 1920x1080 and 3840x2160, uint8 HWC tensors on the GPU (tests/images.tiled against its one-pixel shift), warm contexts:
(a) Comparator.compare without a map and with a float32 map, by host clocks around calls that end in a synchronise,
profiler off; (b) gz_time_compare on the SAME context in the same process: the whole chain of a coefficient candidate,
reconstruction included, by events -- what a pixel comparison should cost about as much as (it runs the ingest kernel
instead of the reconstruction); (c) the emit kernel k_emit_map alone, from the kernel trace of the trace pass: `rounds`
comparisons with a float32 map per size, the first three dropped; (d) the one-shot butteraugli(), context creation and
the reference's psycho image included."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1920, 1080), (3840, 2160))
DROP = 3


def pair(torch, w, h):
    import images
    t0 = torch.from_numpy(images.tiled(w, h)).cuda()
    return t0, torch.roll(t0, 1, dims=1).contiguous()


def trace_pass(rounds):
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    for w, h in SIZES:
        t0, t1 = pair(torch, w, h)
        out = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with guetzli_amd.Comparator(t0) as cmp:
            first = cmp.compare(t1, distmap=out)[0]
            for _ in range(rounds - 1):
                assert cmp.compare(t1, distmap=out)[0] == first
            assert float(out.max()) == first                     # (what is timed is also right: the maximum of the map)
    print("trace pass:", rounds, "comparisons with a map at each of", SIZES)


def median_ms(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": runs}


def time_pass(path, runs):
    import numpy as np
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    res = {}
    for w, h in SIZES:
        t0, t1 = pair(torch, w, h)
        out = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r = {}
        with guetzli_amd.Comparator(t0) as cmp:
            r["compare"] = median_ms(lambda: cmp.compare(t1), runs)
            r["compare_with_f32_map"] = median_ms(lambda: cmp.compare(t1, distmap=out), runs)
            ctx = cmp._ctx                                        # the same context: the chain of a coefficient candidate
            ctx.encode_rgb(download=False)
            ctx.quantize(np.full((3, 64), 3, np.int32), download=False)
            ctx.time_compare(5)
            per = sorted(ctx.time_compare(20) / 20 for _ in range(runs))
            r["gz_time_compare_per_compare"] = {"median_ms": round(statistics.median(per), 4), "min_ms": round(per[0], 4),
                                                "max_ms": round(per[-1], 4), "runs": runs, "compares_per_run": 20}
            again = median_ms(lambda: cmp.compare(t1), runs)
            r["compare_after_the_candidate"] = again              # (the pixel comparison next to coefficient ones)
        r["butteraugli_one_shot"] = median_ms(lambda: guetzli_amd.butteraugli(t0, t1), max(3, runs // 3), warm=2)
        res[f"{w}x{h}"] = r
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def read_trace(directory):
    """The k_emit_map launches in time order: the first half is the first size's, the second the second's."""
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = [r for r in csv.DictReader(open(paths[0])) if re.search(r"\bk_emit_map<", r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert rows and len(rows) % len(SIZES) == 0, len(rows)
    assert all("<float,true>" in r["Kernel_Name"].replace(" ", "") for r in rows), rows[0]["Kernel_Name"]   # the 16-byte stores
    per = len(rows) // len(SIZES)
    out = {}
    for k, (w, h) in enumerate(SIZES):
        ts = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[k * per:(k + 1) * per]][DROP:]
        s = spread(ts)
        s["bytes"] = 8 * w * h                                    # 4 read + 4 written per pixel
        s["GB_per_s"] = round(s["bytes"] / s["median_us"] / 1e3, 1)
        out[f"{w}x{h}"] = s
    return out


def merge(trace_dir, times_path, head, out_path):
    emit = read_trace(trace_dir)
    times = json.load(open(times_path))
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "sizes": {}}
    for key, t in times.items():
        t = dict(t)
        t["k_emit_map_f32"] = emit[key]
        t["map_adds_median_ms"] = round(t["compare_with_f32_map"]["median_ms"] - t["compare"]["median_ms"], 4)
        result["sizes"][key] = t
    print(json.dumps(result, indent=1))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def run_all(workdir, head, out_path, rounds, runs):
    """Both passes as fresh child processes, each under its own time limit; the second only if the first ended well."""
    os.makedirs(workdir, exist_ok=True)
    trace_dir, times = os.path.join(workdir, "trace"), os.path.join(workdir, "times.json")
    me = os.path.abspath(__file__)
    steps = [(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--", sys.executable, me, "--trace-pass",
               "--rounds", str(rounds)], 300),
             ([sys.executable, me, "--time-pass", "--times-out", times, "--runs", str(runs)], 300)]
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"measure_butteraugli: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_butteraugli: a step ended with status {rc}: nothing more is started")
    merge(trace_dir, times, head, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="WORKDIR")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--time-pass", action="store_true")
    ap.add_argument("--times-out")
    ap.add_argument("--rounds", type=int, default=23)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--trace", help="the directory a rocprofv3 --kernel-trace run of --trace-pass wrote")
    ap.add_argument("--times", help="the file --time-pass wrote")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "butteraugli_pair.json"))
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.rounds)
    if a.time_pass:
        return time_pass(a.times_out, a.runs)
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    if a.run:
        return run_all(a.run, head, a.out, a.rounds, a.runs)
    merge(a.trace, a.times, head, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What butteraugli of LINEAR float images costs on the MI355X, beside the 8-bit path on the same tensors
(profiles/butteraugli_linear.json).

    measure_butteraugli_linear.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  The passes can be run by hand as well:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_butteraugli_linear.py --trace-pass
    measure_butteraugli_linear.py --time-pass --times-out TIMES.json
    measure_butteraugli_linear.py --trace DIR --times TIMES.json

At 1920x1080 and 3840x2160, float32 CHW tensors in [0, 1] on the GPU (tests/images.tiled against its one-pixel shift),
warm contexts, the two paths ALTERNATING call by call in one process: (a) Comparator(linear=True, scale=255).compare
beside Comparator.compare of the same tensors (which rounds them to bytes first), by host clocks around calls that end
in a synchronise, profiler off; (b) the kernels k_ingest_linear<float> and k_ingest_rgb<float> alone, from the kernel
trace of the trace pass: `rounds` comparisons per size and path, the first three dropped; (c) the one-shot
butteraugli_linear(), context creation and the reference's psycho image included."""
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
# bytes per pixel each kernel moves: 12 read; 12 written (three float planes), and k_ingest_rgb's 3 packed bytes besides
BYTES_PER_PIXEL = {"k_ingest_linear_f32": 24, "k_ingest_rgb_f32": 27}


def pair(torch, w, h):
    """Two float32 [3][h][w] tensors in [0, 1]: the tiled photograph and its one-pixel shift."""
    import images
    t0 = (torch.from_numpy(images.tiled(w, h)).cuda().permute(2, 0, 1).to(torch.float32) / 255.0).contiguous()
    return t0, torch.roll(t0, 1, dims=2).contiguous()


def trace_pass(rounds):
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    for w, h in SIZES:
        t0, t1 = pair(torch, w, h)
        torch.cuda.synchronize()
        with guetzli_amd.Comparator(t0, linear=True, scale=255) as lin, guetzli_amd.Comparator(t0) as srgb:
            first = (lin.compare(t1), srgb.compare(t1))
            assert lin.clamped == 0 and first[0] > 0 and first[1] > 0
            for _ in range(rounds - 1):
                assert (lin.compare(t1), srgb.compare(t1)) == first
    print("trace pass:", rounds, "comparisons by either path at each of", SIZES)


def stats_ms(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def alternating_ms(fa, fb, runs, warm=3):
    """fa and fb timed in turn, call by call: what disturbs one disturbs the other."""
    for _ in range(warm):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(runs):
        t = time.perf_counter()
        fa()
        ta.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        fb()
        tb.append((time.perf_counter() - t) * 1e3)
    return stats_ms(ta), stats_ms(tb)


def time_pass(path, runs):
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    res = {}
    for w, h in SIZES:
        t0, t1 = pair(torch, w, h)
        torch.cuda.synchronize()
        r = {}
        with guetzli_amd.Comparator(t0, linear=True, scale=255) as lin, guetzli_amd.Comparator(t0) as srgb:
            r["linear_compare"], r["srgb8_compare_of_the_same_tensors"] = alternating_ms(lambda: lin.compare(t1), lambda: srgb.compare(t1), runs)
            r["distance_linear"], r["distance_srgb8"] = lin.compare(t1), srgb.compare(t1)
        few = max(3, runs // 3)
        r["butteraugli_linear_one_shot"], r["butteraugli_one_shot"] = alternating_ms(
            lambda: guetzli_amd.butteraugli_linear(t0, t1, scale=255), lambda: guetzli_amd.butteraugli(t0, t1), few, warm=2)
        res[f"{w}x{h}"] = r
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def read_trace(directory):
    """The launches of either kernel in time order: per size the original's (the Comparator's creation), then `rounds`
    comparisons; the first half is the first size's, the second the second's."""
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    all_rows = list(csv.DictReader(open(paths[0])))
    out = {}
    for name, pattern in (("k_ingest_linear_f32", r"\bk_ingest_linear<float"), ("k_ingest_rgb_f32", r"\bk_ingest_rgb<float>")):
        rows = [r for r in all_rows if re.search(pattern, r["Kernel_Name"].replace(" ", ""))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        assert rows and len(rows) % len(SIZES) == 0, (name, len(rows))
        per = len(rows) // len(SIZES)
        for k, (w, h) in enumerate(SIZES):
            mine = rows[k * per:(k + 1) * per]
            ts = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine][DROP:]
            s = spread(ts)
            s["instantiation"] = sorted({r["Kernel_Name"].split("(")[0] for r in mine})
            s["bytes"] = BYTES_PER_PIXEL[name] * w * h
            s["GB_per_s"] = round(s["bytes"] / s["median_us"] / 1e3, 1)
            out.setdefault(f"{w}x{h}", {})[name] = s
    return out


def merge(trace_dir, times_path, head, out_path):
    kernels = read_trace(trace_dir)
    times = json.load(open(times_path))
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "sizes": {}}
    for key, t in times.items():
        t = dict(t)
        t.update(kernels[key])
        lin, rgb = t["k_ingest_linear_f32"], t["k_ingest_rgb_f32"]
        t["ingest_linear_over_ingest_rgb"] = round(lin["median_us"] / rgb["median_us"], 4)
        t["ingest_linear_no_slower_beyond_the_spread"] = lin["median_us"] <= rgb["median_us"] * (1 + max(lin["spread_pct"], rgb["spread_pct"]) / 100)
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
            sys.exit(f"measure_butteraugli_linear: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_butteraugli_linear: a step ended with status {rc}: nothing more is started")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "butteraugli_linear.json"))
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

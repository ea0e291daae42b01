#!/usr/bin/env python3
"""What butteraugli's masking entries cost on the MI355X, beside the one-shot butteraugli_linear() of the same tensors
(profiles/mask.json).

    measure_mask.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  The passes can be run by hand as well:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_mask.py --trace-pass
    measure_mask.py --time-pass --times-out TIMES.json
    measure_mask.py --trace DIR --times TIMES.json

At 1920x1080 and 3840x2160, float32 CHW tensors in [0, 1] on the GPU (tests/images.tiled), linear=True with scale=255,
float32 CHW results into tensors made once, warm pool: (a) opsin_dynamics(x), mask(x, dc=True), mask(x, y, dc=True) and
adaptive_quantization(x), each a whole call -- the context of the call, its image's psycho image, which create_context
computes and nothing here reads, included -- and the one-shot butteraugli_linear(x, y) as the known yardstick, timed in
turn call by call in one process by host clocks around calls that end in a synchronise, profiler off; (b) the kernel
k_emit_mask<float> alone in its both-masks and its Y-only mode, from the kernel trace of the trace pass: `rounds` calls
per size and mode, the first three dropped."""
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
# bytes per pixel each mode moves: three float planes read and six written; two read and one written
MODES = {"k_emit_mask_both_f32": (3, 36), "k_emit_mask_y_only_f32": (4, 12)}   # name -> (MODE template argument, bytes per pixel)


def pair(torch, w, h):
    """Two float32 [3][h][w] tensors in [0, 1]: the tiled photograph and its one-pixel shift."""
    import images
    t0 = (torch.from_numpy(images.tiled(w, h)).cuda().permute(2, 0, 1).to(torch.float32) / 255.0).contiguous()
    return t0, torch.roll(t0, 1, dims=2).contiguous()


def calls(torch, guetzli_amd, w, h):
    """name -> call, on tensors made once."""
    t0, t1 = pair(torch, w, h)
    xyb, m, dc = (torch.empty((3, h, w), dtype=torch.float32, device="cuda") for _ in range(3))
    q = torch.empty((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(linear=True, scale=255)
    return {"opsin_dynamics": lambda: guetzli_amd.opsin_dynamics(t0, out=xyb, **kw),
            "mask_of_one_image_both": lambda: guetzli_amd.mask(t0, out=m, out_dc=dc, **kw),
            "mask_of_a_pair_both": lambda: guetzli_amd.mask(t0, t1, out=m, out_dc=dc, **kw),
            "adaptive_quantization": lambda: guetzli_amd.adaptive_quantization(t0, scale=255, out=q),
            "butteraugli_linear_one_shot": lambda: guetzli_amd.butteraugli_linear(t0, t1, scale=255)}


def trace_pass(rounds):
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    for w, h in SIZES:
        c = calls(torch, guetzli_amd, w, h)
        for _ in range(rounds):
            c["mask_of_one_image_both"]()
            c["adaptive_quantization"]()
    print("trace pass:", rounds, "calls of mask(x, dc=True) and of adaptive_quantization(x) at each of", SIZES)


def stats_ms(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def in_turn_ms(fs, runs, warm=3):
    """The calls of `fs` timed in turn, call by call: what disturbs one disturbs the others."""
    import torch
    for _ in range(warm):
        for f in fs.values():
            f()
    ts = {k: [] for k in fs}
    for _ in range(runs):
        for k, f in fs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()                              # (ends in the call's own synchronise)
            ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: stats_ms(v) for k, v in ts.items()}


def time_pass(path, runs):
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    res = {}
    for w, h in SIZES:
        r = in_turn_ms(calls(torch, guetzli_amd, w, h), runs)
        q, m = r["adaptive_quantization"], r["mask_of_one_image_both"]
        r["adaptive_quantization_over_mask_of_one_image"] = round(q["median_ms"] / m["median_ms"], 4)
        r["adaptive_quantization_costs_less_beyond_the_spread"] = q["median_ms"] * (1 + max(q["spread_pct"], m["spread_pct"]) / 100) < m["median_ms"]
        res[f"{w}x{h}"] = r
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def read_trace(directory):
    """The launches of either mode in time order: the first half is the first size's, the second the second's."""
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    all_rows = list(csv.DictReader(open(paths[0])))
    out = {}
    for name, (mode, bpp) in MODES.items():
        rows = [r for r in all_rows if re.search(r"\bk_emit_mask<float,(\(int\))?%d>" % mode, r["Kernel_Name"].replace(" ", ""))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        assert rows and len(rows) % len(SIZES) == 0, (name, len(rows))
        per = len(rows) // len(SIZES)
        for k, (w, h) in enumerate(SIZES):
            mine = rows[k * per:(k + 1) * per]
            s = spread([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine][DROP:])
            s["instantiation"] = sorted({r["Kernel_Name"].split("(")[0] for r in mine})
            s["bytes"] = bpp * w * h
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
            sys.exit(f"measure_mask: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_mask: a step ended with status {rc}: nothing more is started")
    merge(trace_dir, times, head, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="WORKDIR")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--time-pass", action="store_true")
    ap.add_argument("--times-out")
    ap.add_argument("--rounds", type=int, default=13)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--trace", help="the directory a rocprofv3 --kernel-trace run of --trace-pass wrote")
    ap.add_argument("--times", help="the file --time-pass wrote")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask.json"))
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

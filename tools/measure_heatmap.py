#!/usr/bin/env python3
"""What the heat map's kernel costs on the MI355X, beside its two yardsticks (profiles/heatmap.json).

    measure_heatmap.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the trace pass below as a child process under rocprofv3 and a time limit, then reads what it wrote.  By hand:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_heatmap.py --trace-pass
    measure_heatmap.py --trace DIR

At 1920x1080 and 3840x2160, `rounds` launches each (the first three dropped), kernel times from the kernel trace:
k_emit_heat of a float32 map of uniform random distances 0 .. 3 (every colour segment up to the pastel range) into a
uint8 HWC and into a float32 CHW tensor (guetzli_amd.heatmap); k_emit_map float32 -> float32 of the same map
(gz_probe_emit_map) and k_emit_rgb into the same two destinations (gz_decode_coeffs_device): the yardsticks -- one
reads the 4 bytes per pixel the heat map reads, the other writes the 3 elements per pixel it writes."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1920, 1080), (3840, 2160))
DESTINATIONS = (("uint8", "HWC", 1), ("float32", "CHW", 4))   # dtype, layout, bytes per element
DROP = 3


def trace_pass(rounds):
    import numpy as np
    import torch
    import guetzli_amd
    from guetzli_amd.capi import GZ_DT_F32, device_map, device_output
    from guetzli_amd.encoder import DTYPE_CODES
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L = guetzli_amd.load()
    good, bad = L.default_heat_thresholds()
    for w, h in SIZES:
        torch.manual_seed(w)
        dist = torch.rand((h, w), device="cuda") * 3.0
        host = dist.cpu().numpy()
        coeffs = np.zeros((3, ((w + 7) // 8) * ((h + 7) // 8), 64), np.int16)
        coeffs[:, :, 0] = np.random.default_rng(w).integers(-1000, 1000, coeffs.shape[:2])
        for dtype, layout, _ in DESTINATIONS:
            out = torch.zeros((h, w, 3) if layout == "HWC" else (3, h, w), dtype=getattr(torch, dtype), device="cuda")
            torch.cuda.synchronize()
            for _ in range(rounds):
                guetzli_amd.heatmap(dist, out=out)
            strides = (3 * w, 3, 1) if layout == "HWC" else (w, 1, w * h)
            for _ in range(rounds):
                L.decode_coeffs_device(coeffs, w, h, device_output(out.data_ptr(), DTYPE_CODES[dtype], strides))
            assert len(torch.unique(out)) > 1
        copy = torch.zeros((h, w), device="cuda")
        for _ in range(rounds):
            L.probe_emit_map(host, device_map(copy.data_ptr(), GZ_DT_F32, (w, 1)))
        assert bool((copy == dist).all())
    print("trace pass:", rounds, "launches of each kernel at each of", SIZES)


def spread(ts, nbytes):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts), "bytes": nbytes,
            "GB_per_s": round(nbytes / (m / 1e3) / 1e3, 1)}


def read_trace(directory, rounds):
    """The launches of each kernel in time order, `rounds` per (size, destination) in the order the trace pass ran them."""
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))

    def durations(kernel):
        ts = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if re.search(r"\b%s<" % kernel, r["Kernel_Name"])]
        assert ts and len(ts) % rounds == 0, (kernel, len(ts))
        return [ts[i:i + rounds][DROP:] for i in range(0, len(ts), rounds)]
    heat, rgb, fmap = durations("k_emit_heat"), durations("k_emit_rgb"), durations("k_emit_map")
    assert len(heat) == len(rgb) == len(SIZES) * len(DESTINATIONS) and len(fmap) == len(SIZES), (len(heat), len(rgb), len(fmap))
    out = {}
    for k, (w, h) in enumerate(SIZES):
        r = {"k_emit_map_f32": spread(fmap[k], 8 * w * h)}
        for j, (dtype, layout, elem) in enumerate(DESTINATIONS):
            name = f"{dtype}_{layout}"
            r["k_emit_heat_" + name] = spread(heat[k * len(DESTINATIONS) + j], (4 + 3 * elem) * w * h)
            r["k_emit_rgb_" + name] = spread(rgb[k * len(DESTINATIONS) + j], (3 + 3 * elem) * w * h)
            r[f"heat_over_map_plus_rgb_{name}"] = round(r["k_emit_heat_" + name]["median_us"] /
                                                        (r["k_emit_map_f32"]["median_us"] + r["k_emit_rgb_" + name]["median_us"]), 2)
        out[f"{w}x{h}"] = r
    return out


def merge(trace_dir, rounds, head, out_path):
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "rounds": rounds, "dropped": DROP,
              "sizes": read_trace(trace_dir, rounds)}
    print(json.dumps(result, indent=1))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def run_all(workdir, head, out_path, rounds):
    """The trace pass as a fresh child process under its own time limit; nothing follows one that ended badly."""
    os.makedirs(workdir, exist_ok=True)
    trace_dir = os.path.join(workdir, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--", sys.executable, os.path.abspath(__file__),
           "--trace-pass", "--rounds", str(rounds)]
    print("+", " ".join(cmd), flush=True)
    try:
        rc = subprocess.run(cmd, timeout=400).returncode
    except subprocess.TimeoutExpired:
        sys.exit("measure_heatmap: the trace pass ran into its limit of 400 s")
    if rc != 0:
        sys.exit(f"measure_heatmap: the trace pass ended with status {rc}")
    merge(trace_dir, rounds, head, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="WORKDIR")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--rounds", type=int, default=23)
    ap.add_argument("--trace", help="the directory a rocprofv3 --kernel-trace run of --trace-pass wrote")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap.json"))
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.rounds)
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    if a.run:
        return run_all(a.run, head, a.out, a.rounds)
    merge(a.trace, a.rounds, head, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What reading the entropy-coded scan on the device costs on the MI355X (profiles/scan_decode.json).

    measure_scan_decode.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  By hand:

    measure_scan_decode.py --time-pass --workdir WORKDIR
    rocprofv3 --kernel-trace --output-format csv -d WORKDIR/trace -- python tools/measure_scan_decode.py --trace-pass --workdir WORKDIR
    measure_scan_decode.py --merge --workdir WORKDIR

Inputs: the quality-95 outputs of process() for tests/golden/bees.png tiled to 1920x1080 and 3840x2160 (images.tiled, as
bench.py tiles it); the time pass writes them into WORKDIR for the trace pass.
(a) Time pass, profiler off, host clocks around calls that end in a synchronise, the two modes ALTERNATING in one run:
decode(jpeg, out=tensor, stream=0, entropy="host") -- the parent commit's path, unchanged: the yardstick -- and
entropy="device".  Beside them the host's read of the stream alone (JpegSize: ReadJpeg with its block loop), which is the
host share of the host mode but for the dequantisation loop; the host share of the device mode is the whole decode minus
the kernels' and copies' time of (b).  Subsequences and rounds come from decode_info.
(b) Trace pass, under rocprofv3 --kernel-trace: decode(entropy="device") of either input, each kernel's time by name."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1920, 1080), (3840, 2160))
KERNELS = ("k_scandec_sync_first", "k_scandec_sync_next", "k_scan_offsets", "k_scandec_write", "k_scandec_dc", "k_chroma_samples",
           "k_reconstruct", "k_emit_rgb")
DROP = 3


def stats(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 1), "runs": len(ts)}


def jpeg_path(workdir, w, h):
    return os.path.join(workdir, f"bees_{w}x{h}_q95.jpg")


def time_pass(workdir, runs):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    import guetzli_amd
    import images
    host = guetzli_amd.load_host()
    os.makedirs(workdir, exist_ok=True)
    res = {}
    for w, h in SIZES:
        jpeg, _ = guetzli_amd.process(torch.from_numpy(images.tiled(w, h)).cuda(), quality=95)
        with open(jpeg_path(workdir, w, h), "wb") as f:
            f.write(jpeg)
        out = {m: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for m in ("host", "device")}
        torch.cuda.synchronize()
        ts = {"host": [], "device": [], "host_read": []}
        info = None
        for i in range(DROP + runs):
            for mode in ("host", "device"):
                t0 = time.perf_counter()
                guetzli_amd.decode(jpeg, out=out[mode], stream=0, entropy=mode)
                t1 = time.perf_counter()
                if i >= DROP:
                    ts[mode].append((t1 - t0) * 1e3)
            t0 = time.perf_counter()
            host.jpeg_size(jpeg)
            if i >= DROP:
                ts["host_read"].append((time.perf_counter() - t0) * 1e3)
        info = guetzli_amd.decode_info(jpeg, out=out["device"], stream=0, entropy="device")
        assert info["path"] == "device" and info["status"] == "DECODED", info
        assert torch.equal(out["host"], out["device"])          # (what is timed is also right)
        res[f"{w}x{h}"] = {"jpeg_bytes": len(jpeg), "subsequences": info["subsequences"], "sync_rounds": info["sync_rounds"],
                           "decode_entropy_host": stats(ts["host"]), "decode_entropy_device": stats(ts["device"]),
                           "host_read_of_the_stream": stats(ts["host_read"])}
    with open(os.path.join(workdir, "times.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace_pass(workdir, rounds):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    import guetzli_amd
    for w, h in SIZES:
        jpeg = open(jpeg_path(workdir, w, h), "rb").read()
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(DROP + rounds):
            guetzli_amd.decode(jpeg, out=out, stream=0, entropy="device")
    print("trace pass:", rounds, "decodes of each size")


def read_trace(workdir, rounds):
    paths = sorted(glob.glob(os.path.join(workdir, "trace", "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for k in KERNELS:
        mine = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if k + "(" in r["Kernel_Name"].replace("gz::", "").replace("<", "(")]
        if not mine:
            continue
        per = len(mine) // (len(SIZES) * (DROP + rounds))       # launches per decode (the rounds of sync_next)
        if per < 1 or per * len(SIZES) * (DROP + rounds) != len(mine):   # (not the same number at both sizes: the sum alone)
            out.setdefault("unsplit", {})[k] = {"launches": len(mine), "total_ms": round(sum(mine) / 1e6, 3)}
            continue
        for s, (w, h) in enumerate(SIZES):
            part = mine[s * per * (DROP + rounds):(s + 1) * per * (DROP + rounds)][per * DROP:]
            sums = [sum(part[i * per:(i + 1) * per]) / 1e6 for i in range(rounds)]
            out.setdefault(f"{w}x{h}", {})[k] = dict(stats(sums), launches_per_decode=per)
    return out


def merge(workdir, rounds, head, out_path):
    times = json.load(open(os.path.join(workdir, "times.json")))
    kernels = read_trace(workdir, rounds)
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "sizes": {}}
    if "unsplit" in kernels:
        result["kernels_not_split_by_size"] = kernels["unsplit"]
    for size, t in times.items():
        ks = kernels.get(size, {})
        total = round(sum(v["median_ms"] for v in ks.values()), 3)
        new = round(sum(v["median_ms"] for k, v in ks.items() if k.startswith("k_scandec") or k == "k_scan_offsets"), 3)
        h, d = t["decode_entropy_host"], t["decode_entropy_device"]
        result["sizes"][size] = dict(t, kernels_ms=ks, kernels_total_median_ms=total, scan_decoder_kernels_median_ms=new,
                                     device_mode_outside_kernels_ms=round(d["median_ms"] - total, 3),
                                     device_over_host=round(d["median_ms"] / h["median_ms"], 3),
                                     device_wins_beyond_spread=d["max_ms"] < h["min_ms"])
    print(json.dumps(result, indent=1))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def run_all(workdir, runs, rounds, head, out_path):
    """Both passes as fresh child processes, each under its own time limit; the second only if the first ended well."""
    me = os.path.abspath(__file__)
    steps = [([sys.executable, me, "--time-pass", "--workdir", workdir, "--runs", str(runs)], 420),
             (["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(workdir, "trace"), "--", sys.executable, me,
               "--trace-pass", "--workdir", workdir, "--rounds", str(rounds)], 300)]
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"measure_scan_decode: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_scan_decode: a step ended with status {rc}: nothing more is started")
    merge(workdir, rounds, head, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="WORKDIR")
    ap.add_argument("--time-pass", action="store_true")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--workdir")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_decode.json"))
    a = ap.parse_args()
    if a.time_pass:
        return time_pass(a.workdir, a.runs)
    if a.trace_pass:
        return trace_pass(a.workdir, a.rounds)
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    if a.run:
        return run_all(a.run, a.runs, a.rounds, head, a.out)
    merge(a.workdir, a.rounds, head, a.out)


if __name__ == "__main__":
    main()

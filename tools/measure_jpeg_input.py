#!/usr/bin/env python3
"""What reading a JPEG input's scan on the device does to an encode of it on the MI355X (profiles/jpeg_input.json).

    measure_jpeg_input.py [--runs 9] [--on-top-of COMMIT] [--out PATH]

Inputs: tests/golden/bees.png tiled to 1920x1080 and 3840x2160 (images.tiled, as bench.py tiles it), written by Pillow at
quality 95 in 4:4:4 and in Pillow's default 4:2:0 -- baseline streams, one scan, no restart interval: eligible.
Profiler off, host clocks around calls that return when their work is done, the two modes ALTERNATING in one run, the
first call of either untimed, the median of --runs with min .. max:
(a) the read alone: HostLibrary.read_jpeg_dump(entropy="host" | "device") -- ReadJpegInput and the canonical dump of its
    result, which both modes pay alike (a copy of the coefficients);
(b) the encode: HostLibrary.process_jpeg(entropy="host" | "device"), whose bytes must be equal.
A mode "wins beyond the spread" where its slowest run is faster than the other's fastest."""
import argparse
import io
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
SAMPLINGS = (("444", 0), ("420", 2))   # Pillow's subsampling argument; 2 is its default at this quality
MODES = ("host", "device")


def stats(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 1), "runs": len(ts)}


def verdict(t):
    h, d = t["host"], t["device"]
    return {"device_over_host": round(d["median_ms"] / h["median_ms"], 3), "device_wins_beyond_spread": d["max_ms"] < h["min_ms"],
            "host_wins_beyond_spread": h["max_ms"] < d["min_ms"]}


def alternating(runs, call):
    """call(mode) for the modes in turns, the first round untimed -> {mode: stats}, {mode: the last result}."""
    ts, last = {m: [] for m in MODES}, {}
    for i in range(1 + runs):
        for mode in MODES:
            t0 = time.perf_counter()
            last[mode] = call(mode)
            t1 = time.perf_counter()
            if i >= 1:
                ts[mode].append((t1 - t0) * 1e3)
    return {m: stats(ts[m]) for m in MODES}, last


def measure(runs):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    from PIL import Image
    import guetzli_amd
    import images
    host = guetzli_amd.load_host()
    res = {}
    for w, h in SIZES:
        rgb = images.tiled(w, h)
        for name, sub in SAMPLINGS:
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, "JPEG", quality=95, subsampling=sub)
            jpeg = b.getvalue()
            read, dumps = alternating(runs, lambda mode: host.read_jpeg_dump(jpeg, mode))
            assert dumps["device"][1]["path"] == "device" and dumps["host"][1]["path"] == "host", dumps["device"][1]
            assert dumps["device"][0] == dumps["host"][0]                 # (what is timed is also right)
            enc, outs = alternating(runs, lambda mode: host.process_jpeg(jpeg, entropy=mode)[0])
            assert outs["device"] == outs["host"]
            info = dumps["device"][1]
            res[f"{w}x{h}_{name}"] = {"jpeg_bytes": len(jpeg), "dump_bytes": len(dumps["host"][0]), "output_bytes": len(outs["host"]),
                                      "subsequences": info["subsequences"], "sync_rounds": info["sync_rounds"],
                                      "read": dict(read, **verdict(read)), "process_jpeg": dict(enc, **verdict(enc))}
            print(f"{w}x{h}_{name}", json.dumps(res[f"{w}x{h}_{name}"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_input.json"))
    a = ap.parse_args()
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "inputs": measure(a.runs)}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What decoding N JPEGs of one size in ONE batched device decode costs on the MI355X (profiles/decode_batch.json).

    measure_decode_batch.py --run WORKDIR [--on-top-of COMMIT] [--out PATH] [--distinct K]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  By hand:

    measure_decode_batch.py --time-pass --workdir WORKDIR
    rocprofv3 --kernel-trace --output-format csv -d WORKDIR/trace -- python tools/measure_decode_batch.py --trace-pass --workdir WORKDIR
    measure_decode_batch.py --merge --workdir WORKDIR

Inputs: the quality-95 outputs of process() of crops of the photograph mosaic (images.mosaic: the nine photographs of
tests/golden/photos), at most --distinct different crops per shape, repeated in turn to the shape's N (an encode costs
seconds, a decode a millisecond: the repeats keep the measurement inside its time limit; 0 = all N distinct); the time pass
writes them into WORKDIR for the trace pass.  Shapes: 64 x 256x256, 16 x 512x512, 8 x 1280x720, 1 x 1024x1024, and 16 x
256x256 half 4:4:4 and half 4:2:0 (force_420).
(a) Time pass, profiler off, host clocks around calls that end in a synchronise, the three variants ALTERNATING in one
run, the first round untimed, median of 9 with min .. max: decode_batch(entropy="device"); a loop of decode(entropy=
"device"); a loop of decode(entropy="host").  What the batch call spends outside its kernels -- the two header passes,
memchr, the upload, the verdict reads, Python -- is its time minus its kernels' of (b).
(b) Trace pass, under rocprofv3 --kernel-trace: decode_batch(entropy="device") of every shape, each kernel's time by name."""
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

# name -> (N, w, h, samplings in turn)
SHAPES = {"64x256x256": (64, 256, 256, ("444",)), "16x512x512": (16, 512, 512, ("444",)), "8x1280x720": (8, 1280, 720, ("444",)),
          "1x1024x1024": (1, 1024, 1024, ("444",)), "16x256x256_half_420": (16, 256, 256, ("444", "420"))}
MULTI = ("64x256x256", "16x512x512", "8x1280x720")
KERNELS = ("k_scandec_sync_first_batch", "k_scandec_sync_next_batch", "k_scan_offsets", "k_scandec_write_batch", "k_scandec_dc_batch",
           "k_chroma_samples_batch", "k_reconstruct420_batch", "k_reconstruct_batch", "k_emit_rgb")
DROP = 1


def stats(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 1), "runs": len(ts)}


def jpeg_path(workdir, name, i):
    return os.path.join(workdir, f"{name}_{i}.jpg")


def make_inputs(workdir, distinct):
    import torch
    import guetzli_amd
    import images
    os.makedirs(workdir, exist_ok=True)
    big = images.mosaic(2048, 1536)
    for name, (n, w, h, samplings) in SHAPES.items():
        k = n if distinct <= 0 else min(n, max(distinct, len(samplings)))
        made = []
        for i in range(k):
            x0, y0 = (i * 211) % (big.shape[1] - w + 1), (i * 97) % (big.shape[0] - h + 1)
            rgb = torch.from_numpy(big[y0:y0 + h, x0:x0 + w].copy()).cuda()
            out = guetzli_amd.process(rgb, quality=95, force_420=samplings[i % len(samplings)] == "420")
            made.append(out[0] if isinstance(out, tuple) else out)
        for i in range(n):
            with open(jpeg_path(workdir, name, i), "wb") as f:
                f.write(made[i % k])


def load_inputs(workdir, name):
    return [open(jpeg_path(workdir, name, i), "rb").read() for i in range(SHAPES[name][0])]


def time_pass(workdir, runs, distinct):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    import guetzli_amd
    make_inputs(workdir, distinct)
    res = {}
    for name, (n, w, h, _) in SHAPES.items():
        jpegs = load_inputs(workdir, name)
        out = {m: torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda") for m in ("batch", "loop_device", "loop_host")}
        torch.cuda.synchronize()
        ts = {m: [] for m in out}
        for i in range(DROP + runs):
            t0 = time.perf_counter()
            guetzli_amd.decode_batch(jpegs, out=out["batch"], stream=0, entropy="device")
            t1 = time.perf_counter()
            for k, j in enumerate(jpegs):
                guetzli_amd.decode(j, out=out["loop_device"][k], stream=0, entropy="device")
            t2 = time.perf_counter()
            for k, j in enumerate(jpegs):
                guetzli_amd.decode(j, out=out["loop_host"][k], stream=0, entropy="host")
            t3 = time.perf_counter()
            if i >= DROP:
                ts["batch"].append((t1 - t0) * 1e3)
                ts["loop_device"].append((t2 - t1) * 1e3)
                ts["loop_host"].append((t3 - t2) * 1e3)
        _, infos = guetzli_amd.decode_batch_info(jpegs, out=out["batch"], stream=0)
        assert all(i["path"] == "device" and i["status"] == "DECODED" for i in infos), infos
        assert torch.equal(out["batch"], out["loop_host"]) and torch.equal(out["loop_device"], out["loop_host"])   # (what is timed is also right)
        res[name] = {"images": n, "width": w, "height": h, "jpeg_bytes": sum(len(j) for j in jpegs),
                     "distinct_inputs": len(set(jpegs)), "subsequences": sum(i["subsequences"] for i in infos),
                     "sync_rounds_max": max(i["sync_rounds"] for i in infos),
                     "decode_batch_device": stats(ts["batch"]), "loop_decode_device": stats(ts["loop_device"]),
                     "loop_decode_host": stats(ts["loop_host"])}
    with open(os.path.join(workdir, "times.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace_pass(workdir, rounds):
    import torch
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    import guetzli_amd
    for name, (n, w, h, _) in SHAPES.items():
        jpegs = load_inputs(workdir, name)
        out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(DROP + rounds):
            guetzli_amd.decode_batch(jpegs, out=out, stream=0, entropy="device")
    print("trace pass:", rounds, "batched decodes of each shape")


def read_trace(workdir, rounds):
    paths = sorted(glob.glob(os.path.join(workdir, "trace", "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the calls in the order they were made: a call begins with its first k_scandec_sync_first_batch (one sampling a call but
    # in the mixed shape, whose two device calls are counted as one decode)
    calls, groups_per_call = [], {name: len(s[3]) for name, s in SHAPES.items()}
    for r in rows:
        k = r["Kernel_Name"].replace("gz::", "")
        k = k.split("<")[0].split("(")[0].replace("void ", "").strip()
        if k == "k_scandec_sync_first_batch":
            calls.append({})
        if calls and k in KERNELS:
            calls[-1][k] = calls[-1].get(k, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    out, at = {}, 0
    for name in SHAPES:
        per = groups_per_call[name]
        mine = calls[at:at + per * (DROP + rounds)]
        at += per * (DROP + rounds)
        decodes = [mine[i * per:(i + 1) * per] for i in range(DROP, DROP + rounds)]
        out[name] = {}
        for k in KERNELS:
            sums = [sum(c.get(k, 0) for c in d) / 1e6 for d in decodes]
            if any(sums):
                out[name][k] = stats(sums)
    assert at == len(calls), (at, len(calls))
    return out


def merge(workdir, rounds, head, out_path):
    times = json.load(open(os.path.join(workdir, "times.json")))
    kernels = read_trace(workdir, rounds)
    result = {"measured_on_top_of": head, "what": __doc__.split("\n\n")[0], "shapes": {}}
    for name, t in times.items():
        ks = kernels.get(name, {})
        total = round(sum(v["median_ms"] for v in ks.values()), 3)
        b, ld, lh = t["decode_batch_device"], t["loop_decode_device"], t["loop_decode_host"]
        result["shapes"][name] = dict(t, kernels_ms=ks, kernels_total_median_ms=total,
                                      batch_outside_kernels_ms=round(b["median_ms"] - total, 3),
                                      batch_outside_kernels_share=round((b["median_ms"] - total) / b["median_ms"], 3),
                                      dc_pass_median_us=round(ks.get("k_scandec_dc_batch", {}).get("median_ms", 0) * 1e3, 1),
                                      loop_device_over_batch=round(ld["median_ms"] / b["median_ms"], 2),
                                      loop_host_over_batch=round(lh["median_ms"] / b["median_ms"], 2),
                                      batch_slowest_beats_device_loop_fastest=b["max_ms"] < ld["min_ms"])
    result["claim_holds_at_the_multi_image_shapes"] = all(result["shapes"][n]["batch_slowest_beats_device_loop_fastest"] for n in MULTI)
    print(json.dumps(result, indent=1))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def run_all(workdir, runs, rounds, head, out_path, distinct):
    """Both passes as fresh child processes, each under its own time limit; the second only if the first ended well."""
    me = os.path.abspath(__file__)
    steps = [([sys.executable, me, "--time-pass", "--workdir", workdir, "--runs", str(runs), "--distinct", str(distinct)], 540),
             (["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(workdir, "trace"), "--", sys.executable, me,
               "--trace-pass", "--workdir", workdir, "--rounds", str(rounds)], 300)]
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"measure_decode_batch: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_decode_batch: a step ended with status {rc}: nothing more is started")
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
    ap.add_argument("--distinct", type=int, default=4, help="different crops per shape at the most (0: all)")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_batch.json"))
    a = ap.parse_args()
    if a.time_pass:
        return time_pass(a.workdir, a.runs, a.distinct)
    if a.trace_pass:
        return trace_pass(a.workdir, a.rounds)
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    if a.run:
        return run_all(a.run, a.runs, a.rounds, head, a.out, a.distinct)
    merge(a.workdir, a.rounds, head, a.out)


if __name__ == "__main__":
    main()

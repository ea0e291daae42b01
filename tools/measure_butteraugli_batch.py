#!/usr/bin/env python3
"""Measures guetzli_amd.butteraugli_batch against the loops it replaces, on the GPU, and writes
profiles/butteraugli_batch.json.

Per shape, with warm pools, the batched call and the loop ALTERNATING in one run, the first call of either untimed,
host clocks around calls that synchronise, median of 9 with min .. max:
  pairs      n distinct references: butteraugli_batch(refs, others)  against  a loop of one-shot butteraugli()
  broadcast  one reference for all: butteraugli_batch(ref, others)   against  a loop of Comparator.compare on ONE warm
             context -- the fastest path the library had for this
The verdict per comparison is the criterion of DESIGN.md 3.12 / 3.13: does the batch's SLOWEST run beat the loop's FASTEST.
The launch count of a batched call comes from the CPU emulation's counter (it does not depend on the size).

  --trace-run batch|single   no measurement: the workload alone, a few times, for a rocprofv3 --kernel-trace --stats
                             run of its own (64 x 256x256 batched, or ONE 256x256 pair through Comparator.compare)
  --kernel-stats BATCH.csv SINGLE.csv   folds the two runs' kernel_stats files into the JSON that exists
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "profiles", "butteraugli_batch.json")
SHAPES = ((64, 256, 256), (16, 512, 512), (8, 1280, 720), (1, 1024, 1024))
RUNS = 9


def batch_tensors(torch, n, w, h):
    import numpy as np
    import images
    base = images.tiled(w + 8 * n, h + 8)
    rng = np.random.default_rng(n * w + h)
    refs = np.stack([base[i % 8:i % 8 + h, 8 * i:8 * i + w] for i in range(n)])
    noise = rng.integers(-3, 4, refs.shape)
    others = np.clip(refs.astype(np.int16) + noise, 0, 255).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(refs)).cuda(), torch.from_numpy(others).cuda()


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def emulated_launches():
    """Launches of one batched call (distinct references / one for all; no maps), by the emulation's counter."""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    from guetzli_amd.capi import GZ_DT_U8, Library, device_batch
    L = Library(build_emu.build())
    L.lib.gz_emu_launch_calls.restype = C.c_long
    a = np.zeros((4, 16, 16, 3), np.uint8)
    d = np.zeros(4, np.float32)
    b4, b1 = device_batch(a.ctypes.data, GZ_DT_U8, (768, 48, 3, 1)), device_batch(a.ctypes.data, GZ_DT_U8, (0, 48, 3, 1))
    out = {}
    for name, ref, n_ref in (("pairs", b4, 4), ("broadcast", b1, 1)):
        before = L.lib.gz_emu_launch_calls()
        L.butteraugli_batch(ref, b4, 16, 16, 4, d.ctypes.data, n_ref=n_ref)
        out[name] = L.lib.gz_emu_launch_calls() - before
    return out


def measure():
    import torch
    import guetzli_amd
    rows = []
    for n, w, h in SHAPES:
        refs, others = batch_tensors(torch, n, w, h)
        torch.cuda.synchronize()
        with guetzli_amd.Comparator(refs[0]) as cmp:
            calls = {
                "pairs": (lambda: guetzli_amd.butteraugli_batch(refs, others),
                          lambda: [guetzli_amd.butteraugli(refs[i], others[i]) for i in range(n)]),
                "broadcast": (lambda: guetzli_amd.butteraugli_batch(refs[0], others),
                              lambda: [cmp.compare(others[i]) for i in range(n)]),
            }
            for kind, (batch, loop) in calls.items():
                batch(); loop()                     # untimed: pools, the first launches of every kernel
                tb, tl = [], []
                for _ in range(RUNS):
                    tb.append(timed(batch))
                    tl.append(timed(loop))
                row = {"n": n, "w": w, "h": h, "comparison": kind, "batch": summary(tb), "loop": summary(tl),
                       "loop_is": "one-shot butteraugli() per pair" if kind == "pairs" else "Comparator.compare on one warm context",
                       "speedup_of_medians": round(statistics.median(tl) / statistics.median(tb), 3),
                       "batch_slowest_beats_loop_fastest": max(tb) < min(tl)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "rows": rows, "launches_per_batched_call": emulated_launches(),
              "method": "batched call and loop alternating in one process, warm pools, first call untimed, host clocks around "
                        "synchronising calls, median of 9 (min .. max)"}
    from guetzli_amd import build as gzbuild
    result["csrc_digest"] = gzbuild.csrc_digest()
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


def trace_run(which):
    import torch
    import guetzli_amd
    refs, others = batch_tensors(torch, 64, 256, 256)
    torch.cuda.synchronize()
    if which == "batch":
        for _ in range(10):
            guetzli_amd.butteraugli_batch(refs, others)
    else:
        with guetzli_amd.Comparator(refs[0]) as cmp:
            for _ in range(10):
                cmp.compare(others[0])


def fold_kernel_stats(batch_csv, single_csv):
    """Average time per call of every kernel of the two trace runs (kernel_stats: Name, Calls, TotalDurationNs, ...)."""
    def read(path):
        out = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName")
                calls, total = int(r["Calls"]), float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)"))
                out[name.split("(")[0].replace("gz::", "").replace("void ", "")] = {"calls": calls, "avg_us": round(total / calls / 1e3, 2)}
        return out
    with open(OUT) as f:
        result = json.load(f)
    result["kernel_times"] = {"batched_64x256x256": read(batch_csv), "single_256x256": read(single_csv),
                              "method": "rocprofv3 --kernel-trace --stats, a run of its own per workload"}
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", choices=("batch", "single"))
    ap.add_argument("--kernel-stats", nargs=2, metavar=("BATCH_CSV", "SINGLE_CSV"))
    a = ap.parse_args()
    if a.trace_run:
        trace_run(a.trace_run)
    elif a.kernel_stats:
        fold_kernel_stats(*a.kernel_stats)
    else:
        measure()

#!/usr/bin/env python3
"""What device-resident input costs and saves, measured on the GPU in one process (profiles/device_input.json).

    measure_device_input.py [--rounds N] [--encodes N] [--kernel-stats SIZE=CSV ...] [--on-top-of COMMIT] [--out PATH]
    measure_device_input.py --profile-pass WxH        (the work a `rocprofv3 --kernel-trace --stats` run looks at)

At 3840x2160, 1024x1024 and 3834x2160 (tests/images.tiled) -- the last a width that is no multiple of 16, or of 4: no
16-byte loads for either form there, and byte stores into every other row of the packed image --, with the pools warm and every first call untimed, in alternation:
  gz_create from host pixels | gz_create_from_device from the same pixels resident as uint8 HWC | ... as float32 CHW
    -- wall clock of the call (it ends in a stream synchronise), median and the spread of the rounds;
  a whole guetzli_amd.process each way at quality 95 (numpy array | uint8 HWC tensor | float32 CHW tensor).
Kernel times come from a profiler run of their own (--profile-pass under rocprofv3, its *kernel_stats.csv given back
with --kernel-stats): k_ingest_rgb's bytes / time beside k_reconstruct's at the same size, bytes as the algorithm needs
them (ingest: the source once, 3 bytes and 3 floats per pixel out; k_reconstruct: 3 int16 coefficients per pixel in,
3 floats per pixel out).  The profiler pass runs each kernel ten times on the same source, so a source that fits the
256 MB Infinity Cache (the float32 4K image is 100 MB) is read from there after the first pass: an upper figure."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import images  # noqa: E402

SIZES = ((3840, 2160), (1024, 1024), (3834, 2160))
TARGET = 0.971769
Q = np.full((3, 64), 3, np.int32)


def device_forms(torch, rgb):
    """{name: (tensor that owns the memory, gz_device_image)} of the pixels resident on the GPU."""
    from guetzli_amd.capi import GZ_DT_F32, GZ_DT_U8, device_image
    h, w, _ = rgb.shape
    u8 = torch.from_numpy(rgb).cuda()
    f32 = torch.from_numpy(np.ascontiguousarray((rgb.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))).cuda()
    torch.cuda.synchronize()
    return {"u8_hwc": (u8, device_image(u8.data_ptr(), GZ_DT_U8, (3 * w, 3, 1))),
            "f32_chw": (f32, device_image(f32.data_ptr(), GZ_DT_F32, (w, 1, w * h)))}


def spread(ts):
    m = statistics.median(ts)
    return {"median_ms": round(m * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def time_creates(L, rgb, forms, rounds):
    h, w, _ = rgb.shape
    makers = {"gz_create_host": lambda: L.context(rgb, TARGET)}
    for name, (_, image) in forms.items():
        makers["gz_create_from_device_" + name] = (lambda image=image: L.context_from_device(image, w, h, TARGET))
    for make in makers.values():      # untimed: the pool takes the buffers, the code objects load
        make().close()
    ts = {k: [] for k in makers}
    for _ in range(rounds):
        for k, make in makers.items():   # alternating: what else runs on the box hits every form alike
            t0 = time.perf_counter()
            ctx = make()
            ts[k].append(time.perf_counter() - t0)
            ctx.close()
    return {k: spread(v) for k, v in ts.items()}


def time_encodes(rgb, forms, runs):
    import guetzli_amd
    inputs = {"process_host": rgb, "process_device_u8_hwc": forms["u8_hwc"][0], "process_device_f32_chw": forms["f32_chw"][0]}
    out, ref = {}, None
    for x in inputs.values():
        guetzli_amd.process(x, quality=95)   # untimed
    ts = {k: [] for k in inputs}
    for _ in range(runs):
        for k, x in inputs.items():
            t0 = time.perf_counter()
            jpg, _ = guetzli_amd.process(x, quality=95)
            ts[k].append(time.perf_counter() - t0)
            ref = ref or jpg
            assert jpg == ref, k + ": another JPEG than from host pixels"
    for k, v in ts.items():
        out[k] = {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4), "runs": len(v)}
    return out


def profile_pass(w, h):
    """What the profiler run looks at: creates from both device forms (k_ingest_rgb) and Compares (k_reconstruct)."""
    import torch
    import guetzli_amd
    L = guetzli_amd.load()
    rgb = images.tiled(w, h)
    forms = device_forms(torch, rgb)
    for _ in range(10):
        for _, image in forms.values():
            L.context_from_device(image, w, h, TARGET).close()
    with L.context(rgb, TARGET) as ctx:
        ctx.set_config(patch_reconstruct=0)
        ctx.encode_rgb(download=False)
        ctx.quantize(Q, download=False)
        for _ in range(10):
            ctx.compare(want_distmap=False, want_block_max=False)


def kernel_rates(path, w, h):
    """{kernel: {calls, average_us, bytes, GB_per_s}} of k_ingest_rgb<...> and k_reconstruct from a *kernel_stats.csv."""
    need = {"k_ingest_rgb<unsigned char>": 3 * w * h + 3 * w * h + 12 * w * h, "k_ingest_rgb<float>": 12 * w * h + 3 * w * h + 12 * w * h,
            "k_reconstruct": 6 * w * h + 12 * w * h}
    out = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"^void\s+|^gz::|\(.*$", "", r["Name"].strip().strip('"'))
        name = re.sub(r"^gz::", "", name)
        for key, nbytes in need.items():
            if name.startswith(key):
                us = float(r["AverageNs"]) / 1e3
                out[key] = {"calls": int(r["Calls"]), "average_us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--encodes", type=int, default=3)
    ap.add_argument("--profile-pass")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="WxH=path/to/kernel_stats.csv of a --profile-pass run")
    ap.add_argument("--on-top-of", help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_input.json"))
    a = ap.parse_args()
    if a.profile_pass:
        profile_pass(*(int(v) for v in a.profile_pass.split("x")))
        return
    import torch
    import guetzli_amd
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L = guetzli_amd.load()
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        import subprocess
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    result = {"measured_on_top_of": head, "device": torch.cuda.get_device_name(0), "what": __doc__.split("\n\n")[0], "sizes": {}}
    for w, h in SIZES:
        rgb = images.tiled(w, h)
        forms = device_forms(torch, rgb)
        entry = {"create": time_creates(L, rgb, forms, a.rounds), "encode_q95": time_encodes(rgb, forms, a.encodes)}
        c = entry["create"]
        host = c["gz_create_host"]["median_ms"]
        noise = max(v["spread_pct"] for v in c.values())
        entry["create_from_device_not_slower"] = {
            k: bool(v["median_ms"] <= host * (1 + noise / 100)) for k, v in c.items() if k != "gz_create_host"}
        entry["run_to_run_spread_pct"] = noise
        key = f"{w}x{h}"
        if key in stats:
            entry["kernels"] = kernel_rates(stats[key], w, h)
        result["sizes"][key] = entry
        print(key, json.dumps(entry), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

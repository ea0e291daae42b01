#!/usr/bin/env python3
"""timers["downsample"] of a force_420 + use_silver_screen encode: the figure profiles/silver_screen_device.json keeps.

    silver_time.py [--host-lib PATH] [--size WxH] [--runs N] [--quality Q]

Prints one JSON line: every run's downsample timer, their median, the whole encode's time, the output's sha256 and,
where the library reports them, the silver screen cell rounds evaluated and redone on the host.  --host-lib: another
build's libguetzli_amd_host.so (it loads the libguetzli_amd.so beside it) -- the parent commit's, for the comparison;
one library per process.  With the default library the device conversion is also timed alone, through
gz_probe_silver_yuv420 on the encode's image with the guard off (no host path, no waits for it) and at the production
guard: wall clock of the whole call per pass, 21 passes."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import images  # noqa: E402
from guetzli_amd.encoder import DEFAULT_HOST_LIB, HostLibrary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-lib", default=DEFAULT_HOST_LIB)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--quality", type=float, default=95.0)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    rgb = images.tiled(w, h)
    host = HostLibrary(a.host_lib)
    host.process(images.crop(64, 48, 100, 100), quality=a.quality, force_420=True, use_silver_screen=True)   # warm-up
    down, total, info, jpg = [], [], None, None
    for _ in range(a.runs):
        t0 = time.perf_counter()
        jpg, info = host.process(rgb, quality=a.quality, force_420=True, use_silver_screen=True)
        total.append(time.perf_counter() - t0)
        down.append(info["timers"]["downsample"])
    out = {"size": f"{w}x{h}", "quality": a.quality, "host_lib": os.path.relpath(a.host_lib, ROOT),
           "downsample_s": [round(v, 6) for v in down], "downsample_median_s": round(statistics.median(down), 6),
           "encode_median_s": round(statistics.median(total), 4), "jpeg_sha256": hashlib.sha256(jpg).hexdigest()}
    for k in ("silver screen cell rounds", "silver screen cell rounds on host"):
        if k in info["counters"]:
            out[k] = info["counters"][k]
    if os.path.abspath(a.host_lib) == os.path.abspath(DEFAULT_HOST_LIB):
        import guetzli_amd
        L = guetzli_amd.load()
        L.probe_silver_yuv420(images.crop(64, 48, 100, 100))
        for name, guard in (("probe_guard_off", 64), ("probe_guard_40", 40)):
            ts = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                cnt = L.probe_silver_yuv420(rgb, guard)[3]
                ts.append(time.perf_counter() - t0)
            out[name] = {"call_median_s": round(statistics.median(ts), 6), "per_pass_us": round(statistics.median(ts) / 21 * 1e6, 1),
                         "cell_rounds": cnt[0], "cell_rounds_on_host": cnt[1]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

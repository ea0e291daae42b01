#!/usr/bin/env python3
"""What the alpha-aware ingest costs beside the opaque one, kernel times at 3840x2160 (profiles/device_alpha.json).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_device_alpha.py --trace-pass --parent-lib PARENT.so
    measure_device_alpha.py --trace DIR [--on-top-of COMMIT] [--out PATH]

The trace pass, one process, in rounds that alternate four forms (what else runs on the machine hits every form alike):
  parent_u8_hwc_rgb   k_ingest_rgb<uint8> of the PARENT commit's library (--parent-lib: that commit's
                      libguetzli_amd.so, loaded beside this tree's) on HWC RGB uint8
  u8_hwc_rgb          this build's k_ingest_rgb<uint8> on the same pixels
  u8_hwc_rgba         k_ingest_rgba<uint8> on HWC RGBA uint8 (the four-vector path)
  f32_chw_rgba        k_ingest_rgba<float> on CHW RGBA float32 (the planar path)
each through gz_set_rgb_device[_pixels] on a standing context, which ends in a stream synchronise: the i-th ingest
launch of the trace belongs to form i mod 4.  The second call reads the trace: per form the median, minimum, maximum
and spread of the kernel's time over the rounds (the first three dropped: code objects load, pools fill), and the two
conditions
  opaque  u8_hwc_rgb <= parent_u8_hwc_rgb * (1 + spread)            the alpha work stayed out of the opaque kernel
  rgba    u8_hwc_rgba <= u8_hwc_rgb * (19 / 18 + spread)            19 bytes per pixel moved against 18
with spread = the largest run-to-run spread of the forms compared.  Every round reads the same sources, and a 4K
uint8 image (25 or 33 MB) fits the 256 MB Infinity Cache: the times are those of sources resident there."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import images  # noqa: E402

W, H = 3840, 2160
TARGET = 0.971769
FORMS = ("parent_u8_hwc_rgb", "u8_hwc_rgb", "u8_hwc_rgba", "f32_chw_rgba")
BYTES_PER_PIXEL = {"parent_u8_hwc_rgb": 3 + 3 + 12, "u8_hwc_rgb": 3 + 3 + 12, "u8_hwc_rgba": 4 + 3 + 12, "f32_chw_rgba": 16 + 3 + 12}
DROP = 3


def trace_pass(parent_lib, rounds):
    import torch
    import guetzli_amd
    from guetzli_amd.capi import GZ_DT_F32, GZ_DT_U8, device_image, device_pixels
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L = guetzli_amd.load()
    P = C.CDLL(parent_lib)   # the parent's C ABI: no gz_device_pixels there
    assert not hasattr(P, "gz_create_from_device_pixels"), "--parent-lib is a library of this tree"
    P.gz_create.restype = C.c_void_p
    P.gz_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.POINTER(C.c_int)]
    P.gz_set_rgb_device.argtypes = [C.c_void_p, C.c_void_p]
    P.gz_destroy.argtypes = [C.c_void_p]
    rgb = images.tiled(W, H)
    alpha = np.random.default_rng(1).integers(0, 256, (H, W, 1), dtype=np.uint8)
    rgba = np.concatenate([rgb, alpha], -1)
    u8 = torch.from_numpy(rgb).cuda()
    u8a = torch.from_numpy(rgba).cuda()
    f32a = torch.from_numpy(np.ascontiguousarray((rgba.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))).cuda()
    torch.cuda.synchronize()
    opaque = device_image(u8.data_ptr(), GZ_DT_U8, (3 * W, 3, 1))
    forms = [opaque,
             device_pixels(u8a.data_ptr(), GZ_DT_U8, (4 * W, 4, 1), 0, u8a.data_ptr() + 3, (30, 144, 255)),
             device_pixels(f32a.data_ptr(), GZ_DT_F32, (W, 1, W * H), 0, f32a.data_ptr() + 4 * 3 * W * H, (30, 144, 255))]
    # both contexts exist before the first ingest launch that counts: their creation (from host pixels) launches none
    err = C.c_int(0)
    with L.context(rgb, TARGET) as ctx:
        pctx = P.gz_create(0, W, H, rgb.ctypes.data, TARGET, C.byref(err))
        assert pctx, err.value
        for _ in range(rounds):
            rc = P.gz_set_rgb_device(pctx, C.byref(opaque))
            assert rc == 0, rc
            for image in forms:
                ctx.set_rgb_device(image)
        P.gz_destroy(pctx)
    print("trace pass:", rounds, "rounds of", ", ".join(FORMS))


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def read_trace(directory):
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = [r for r in csv.DictReader(open(paths[0])) if "k_ingest_rgb" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert rows and len(rows) % len(FORMS) == 0, len(rows)
    expect = ("k_ingest_rgb<unsigned char>", "k_ingest_rgb<unsigned char>", "k_ingest_rgba<unsigned char, 3>", "k_ingest_rgba<float, 1>")
    ts = {f: [] for f in FORMS}
    for i, r in enumerate(rows):
        k = i % len(FORMS)
        name = re.sub(r"^void\s+|gz::|\(.*$", "", r["Kernel_Name"].strip().strip('"'))
        assert name == expect[k], (i, name, expect[k])
        ts[FORMS[k]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return {f: v[DROP:] for f, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=23)
    ap.add_argument("--trace", help="the directory a rocprofv3 --kernel-trace run of --trace-pass wrote")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_alpha.json"))
    a = ap.parse_args()
    if a.trace_pass:
        trace_pass(a.parent_lib, a.rounds)
        return
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        import subprocess
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    kernels = {}
    for f, ts in read_trace(a.trace).items():
        kernels[f] = dict(spread(ts), bytes=BYTES_PER_PIXEL[f] * W * H)
        kernels[f]["GB_per_s"] = round(kernels[f]["bytes"] / kernels[f]["median_us"] / 1e3, 1)
    parent, opaque, rgba = (kernels[f] for f in FORMS[:3])
    s_opaque = max(parent["spread_pct"], opaque["spread_pct"])
    s_rgba = max(opaque["spread_pct"], rgba["spread_pct"])
    result = {"measured_on_top_of": head, "size": f"{W}x{H}", "what": __doc__.split("\n\n")[0], "kernels": kernels,
              "opaque_not_slower_than_parent": {"spread_pct": s_opaque, "limit_us": round(parent["median_us"] * (1 + s_opaque / 100), 2),
                                                "median_us": opaque["median_us"],
                                                "holds": bool(opaque["median_us"] <= parent["median_us"] * (1 + s_opaque / 100))},
              "rgba_within_19_18_of_opaque": {"spread_pct": s_rgba, "limit_us": round(opaque["median_us"] * (19 / 18 + s_rgba / 100), 2),
                                              "median_us": rgba["median_us"],
                                              "holds": bool(rgba["median_us"] <= opaque["median_us"] * (19 / 18 + s_rgba / 100))}}
    print(json.dumps(result, indent=1))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What decoding to device-resident pixels costs on the MI355X (profiles/decode_output.json).

    measure_decode.py --run WORKDIR [--on-top-of COMMIT] [--out PATH]

runs the two passes below as child processes, each under its own time limit and only if the one before ended well, then
merges what they wrote.  The passes can be run by hand as well:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_decode.py --trace-pass
    measure_decode.py --time-pass --times-out TIMES.json
    measure_decode.py --trace DIR --times TIMES.json

(a) The emit kernel's rate, with the ingest kernel's as the yardstick: the same bytes in the opposite direction.  The
trace pass, one process, alternates three destinations at 3840x2160 -- uint8 HWC, float32 CHW, bfloat16 CHW -- and for
each runs gz_reconstruct_device of a standing context into the tensor (k_reconstruct, then k_emit_rgb) and
gz_pack_rgb_device of the tensor it has just filled (k_ingest_rgb without the linear planes: 3 + 3 * element size bytes
per pixel either way).  Kernel times come from the kernel trace, not from events: an event pair around the call would
time k_reconstruct too.  The i-th launch of either kernel belongs to form i mod 3; the first three rounds are dropped
(code objects load, pools fill).  Every round touches the same tensors, and they fit the 256 MB Infinity Cache except
float32 (99.5 MB + 24.9 MB, which still does): the rates are those of cache-resident data, for both kernels alike.
(b) decode() of the 4K bees quality-95 output, by host clocks around calls that end in a synchronise, profiler off:
the host's read of the stream (ReadJpeg: the Huffman decode), the device call (coefficient upload, k_reconstruct,
k_emit_rgb, the wait), and the whole decode(); the emit kernel's own share is (a)'s uint8 HWC time.
(c) process(decoded=True) against process() on the same image and the same tensor, alternating.  The encode's code is
the parent commit's, unchanged, so process() of this tree stands for it."""
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

W, H = 3840, 2160
TARGET = 0.971769
FORMS = ("u8_hwc", "f32_chw", "bf16_chw")
ELEM = {"u8_hwc": 1, "f32_chw": 4, "bf16_chw": 2}
DROP = 3


def destinations(torch):
    return {"u8_hwc": torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"),
            "f32_chw": torch.zeros((3, H, W), dtype=torch.float32, device="cuda"),
            "bf16_chw": torch.zeros((3, H, W), dtype=torch.bfloat16, device="cuda")}


def descriptors(t, form):
    from guetzli_amd.capi import GZ_DT_BF16, GZ_DT_F32, GZ_DT_U8, device_image, device_output
    code = {"u8_hwc": GZ_DT_U8, "f32_chw": GZ_DT_F32, "bf16_chw": GZ_DT_BF16}[form]
    strides = (3 * W, 3, 1) if form == "u8_hwc" else (W, 1, W * H)
    return device_output(t.data_ptr(), code, strides), device_image(t.data_ptr(), code, strides)


def trace_pass(rounds):
    import numpy as np
    import torch
    import guetzli_amd
    import images
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L = guetzli_amd.load()
    rgb = images.tiled(W, H)
    dest = destinations(torch)
    torch.cuda.synchronize()
    with L.context(rgb, TARGET) as ctx:
        ctx.encode_rgb(download=False)
        ctx.quantize(np.full((3, 64), 3, np.int32), download=False)
        exp = ctx.reconstruct()[0]
        for _ in range(rounds):
            for form in FORMS:
                out, image = descriptors(dest[form], form)
                ctx.reconstruct_device(out)                      # k_reconstruct, k_emit_rgb; synchronises
                back = L.pack_rgb_device(image, W, H)            # k_ingest_rgb
                assert np.array_equal(back, exp), form           # (what is timed is also right)
    print("trace pass:", rounds, "rounds of", ", ".join(FORMS))


def median_ms(fn, runs, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    m = statistics.median(ts)
    return {"median_ms": round(m, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": runs}


def time_pass(path, runs):
    import numpy as np
    import torch
    import guetzli_amd
    import device_output_cases as doc
    import images
    from guetzli_amd.capi import GZ_DT_U8, device_output
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L, host = guetzli_amd.load(), guetzli_amd.load_host()
    rgb = images.tiled(W, H)
    t_in = torch.from_numpy(rgb).cuda()
    jpeg, _ = guetzli_amd.process(t_in)          # (the first encode: untimed)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"size": f"{W}x{H}", "jpeg_bytes": len(jpeg)}
    # (b)
    res["host_read"] = median_ms(lambda: host.jpeg_size(jpeg), runs)
    import ctypes as C
    host.lib.gzh_read_jpeg.restype = C.c_long
    host.lib.gzh_read_jpeg.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    buf = np.frombuffer(jpeg, np.uint8)
    dump = np.zeros(1 << 27, np.uint8)
    n = host.lib.gzh_read_jpeg(buf.ctypes.data, len(jpeg), dump.ctypes.data, dump.size)
    assert 0 < n <= dump.size
    co, factor = doc.frame_of_dump(doc.parse_jpeg_dump(dump[:n].tobytes()))
    o = device_output(out.data_ptr(), GZ_DT_U8, (3 * W, 3, 1))
    res["device_call_upload_reconstruct_emit"] = median_ms(lambda: L.decode_coeffs_device(co, W, H, o, chroma_factor=factor), runs)
    res["decode_total"] = median_ms(lambda: guetzli_amd.decode(jpeg, out=out, stream=0), runs)
    # (c) alternating, the same tensor
    plain, with_decoded, share = [], [], []
    for i in range(2 + runs):
        t0 = time.perf_counter()
        guetzli_amd.process(t_in)
        t1 = time.perf_counter()
        _, info = guetzli_amd.process(t_in, decoded=out)
        t2 = time.perf_counter()
        if i >= 2:
            plain.append((t1 - t0) * 1e3)
            with_decoded.append((t2 - t1) * 1e3)
            share.append(info["timers"]["decode_output"] * 1e3)
    res["process"] = {"median_ms": round(statistics.median(plain), 2), "min_ms": round(min(plain), 2), "max_ms": round(max(plain), 2), "runs": runs}
    res["process_decoded"] = {"median_ms": round(statistics.median(with_decoded), 2), "min_ms": round(min(with_decoded), 2),
                              "max_ms": round(max(with_decoded), 2), "runs": runs,
                              "decode_output_timer_median_ms": round(statistics.median(share), 2)}
    assert np.array_equal(out.cpu().numpy(), guetzli_amd.decode(jpeg, device="host"))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": round(m / 1e3, 2), "min_us": round(min(ts) / 1e3, 2), "max_us": round(max(ts) / 1e3, 2),
            "spread_pct": round((max(ts) - min(ts)) / m * 100, 2), "runs": len(ts)}


def read_trace(directory):
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, paths
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    expect = {"k_emit_rgb": ("unsigned char, 2", "float, 1", "ingest_bf16, 1"), "k_ingest_rgb": ("unsigned char", "float", "ingest_bf16")}
    out = {}
    for kernel, args in expect.items():
        mine = [r for r in rows if re.search(r"\b%s<" % kernel, r["Kernel_Name"])]
        assert mine and len(mine) % len(FORMS) == 0, (kernel, len(mine))
        ts = {f: [] for f in FORMS}
        for i, r in enumerate(mine):
            k = i % len(FORMS)
            assert args[k] in r["Kernel_Name"].replace("gz::", ""), (i, r["Kernel_Name"], args[k])
            ts[FORMS[k]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        out[kernel] = {f: v[DROP:] for f, v in ts.items()}
    recon = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if re.search(r"\bk_reconstruct\b", r["Kernel_Name"])]
    return out, recon[DROP * len(FORMS):]


def merge(trace_dir, times_path, head, out_path):
    kernels, recon = read_trace(trace_dir)
    rate = {}
    for form in FORMS:
        nbytes = (3 + 3 * ELEM[form]) * W * H
        e, g = spread(kernels["k_emit_rgb"][form]), spread(kernels["k_ingest_rgb"][form])
        for d in (e, g):
            d["GB_per_s"] = round(nbytes / d["median_us"] / 1e3, 1)
        rate[form] = {"bytes": nbytes, "k_emit_rgb": e, "k_ingest_rgb": g, "emit_over_ingest_rate": round(g["median_us"] / e["median_us"], 3)}
    times = json.load(open(times_path))
    emit_ms = rate["u8_hwc"]["k_emit_rgb"]["median_us"] / 1e3
    result = {"measured_on_top_of": head, "size": f"{W}x{H}", "what": __doc__.split("\n\n")[0],
              "a_emit_kernel_rate": rate, "k_reconstruct": spread(recon),
              "b_decode_split_ms": {"host_read": times["host_read"], "device_call_upload_reconstruct_emit": times["device_call_upload_reconstruct_emit"],
                                    "of_it_emit_kernel_ms": round(emit_ms, 4), "decode_total": times["decode_total"], "jpeg_bytes": times["jpeg_bytes"]},
              "c_process_ms": {"process": times["process"], "process_decoded": times["process_decoded"],
                               "added_median_ms": round(times["process_decoded"]["median_ms"] - times["process"]["median_ms"], 2)}}
    print(json.dumps(result, indent=1))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def run_all(workdir, head, out_path):
    """Both passes as fresh child processes, each under its own time limit; the second only if the first ended well."""
    os.makedirs(workdir, exist_ok=True)
    trace_dir, times = os.path.join(workdir, "trace"), os.path.join(workdir, "times.json")
    me = os.path.abspath(__file__)
    steps = [(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--", sys.executable, me, "--trace-pass"], 420),
             ([sys.executable, me, "--time-pass", "--times-out", times], 420)]
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"measure_decode: a step ran into its limit of {limit} s: nothing more is started")
        if rc != 0:
            sys.exit(f"measure_decode: a step ended with status {rc}: nothing more is started")
    merge(trace_dir, times, head, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="WORKDIR")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--time-pass", action="store_true")
    ap.add_argument("--times-out")
    ap.add_argument("--rounds", type=int, default=23)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--trace", help="the directory a rocprofv3 --kernel-trace run of --trace-pass wrote")
    ap.add_argument("--times", help="the file --time-pass wrote")
    ap.add_argument("--on-top-of", help="the parent commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_output.json"))
    a = ap.parse_args()
    if a.trace_pass:
        return trace_pass(a.rounds)
    if a.time_pass:
        return time_pass(a.times_out, a.runs)
    head = a.on_top_of
    if head is None:   # (a copy of the tree without its history says --on-top-of)
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    if a.run:
        return run_all(a.run, head, a.out)
    merge(a.trace, a.times, head, a.out)


if __name__ == "__main__":
    main()

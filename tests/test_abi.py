"""CPU: the product library loads and exports every symbol include/guetzli_amd.h declares,
argument errors are reported as codes, and -- without a GPU -- creating a context fails
loudly with GZ_E_NO_DEVICE instead of falling back to anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from guetzli_amd import build as gzbuild
from guetzli_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "guetzli_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gz_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    return gzbuild.build()


def test_every_declared_symbol_is_exported(lib_path):
    names = declared_functions()
    assert len(names) >= 25
    lib = C.CDLL(lib_path)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(capi.SIGNATURES) == names, "capi.SIGNATURES out of sync with the header"


def test_argument_errors_and_no_silent_fallback(lib_path):
    L = capi.Library(lib_path)
    assert L.lib.gz_abi_version() == 6
    assert L.lib.gz_strerror(-2).decode() == "no usable HIP device"
    err = C.c_int(0)
    rgb = np.zeros((16, 16, 3), np.uint8)
    assert not L.lib.gz_create(0, 4, 16, rgb.ctypes.data, 1.0, C.byref(err))
    assert err.value == -1                      # GZ_E_ARG: w < 8
    assert not L.lib.gz_create(0, 16, 16, None, 1.0, C.byref(err))
    assert err.value == -1
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        assert not L.lib.gz_create(0, 16, 16, rgb.ctypes.data, 1.0, C.byref(err))
        assert err.value == -2                  # GZ_E_NO_DEVICE, never a CPU path
        with pytest.raises(capi.GuetzliAmdError):
            L.context(rgb, 1.0)


def test_config_struct(lib_path, monkeypatch):
    """gz_config: filled from the environment once (gz_config_from_environment needs no device), bad arguments are
    codes."""
    L = capi.Library(lib_path)
    for k in ("GZ_BLUR_PK", "GZ_TILE_ROWS", "GZ_SINGLE_STREAM", "GZ_STORE_DISTMAP", "GZ_PATCH_RECON", "GZ_OPSIN_AHEAD"):
        monkeypatch.delenv(k, raising=False)
    d = L.config_from_environment().as_dict()
    assert d == {"struct_size": C.sizeof(capi.GzConfig), "blur_packed": -1, "tile_rows": 0, "single_stream": -1,
                 "store_distmap": 0, "patch_reconstruct": 1, "opsin_ahead": 1}
    monkeypatch.setenv("GZ_BLUR_PK", "0")
    monkeypatch.setenv("GZ_TILE_ROWS", "32")
    monkeypatch.setenv("GZ_SINGLE_STREAM", "1")
    monkeypatch.setenv("GZ_PATCH_RECON", "2")
    d = L.config_from_environment().as_dict()
    assert (d["blur_packed"], d["tile_rows"], d["single_stream"], d["patch_reconstruct"]) == (0, 32, 1, 2)
    monkeypatch.setenv("GZ_TILE_ROWS", "24")     # not a tile height: ignored
    assert L.config_from_environment().tile_rows == 0
    cfg = capi.GzConfig()
    assert L.lib.gz_config_from_environment(None) == -1
    assert L.lib.gz_get_config(None, C.byref(cfg)) == -1 and L.lib.gz_set_config(None, C.byref(cfg)) == -1
    assert L.lib.gz_device_pci_bus_id(0, None, 0) == -1


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(capi.GuetzliAmdError):
        capi.Library(str(tmp_path / "nope.so"))


def test_host_side_candidate_ranking(lib_path):
    """gz_rank_zeroing_candidates is pure host code of the PRODUCT library (hipcc-built):
    input_order of ComputeBlockZeroingOrder (processor.cc:381-400).  Checked against a
    numpy restatement using the order.inc tables (host tables must not live in device
    constant memory)."""
    import re
    import images
    from checkers import oracle
    src = open(os.path.join(ROOT, "oracle", "malta_offsets.inc")).read()

    def tab(name):
        m = re.search(r"%s\[192\] = \{(.*?)\};" % name, src, re.S)
        return np.array([float(v.strip().rstrip("f")) for v in m.group(1).split(",") if v.strip()],
                        np.float32)
    csf, bias = tab("kOrderCsf"), tab("kOrderBias")
    rgb = images.crop(64, 48, 100, 100)
    co = oracle.encode_rgb(rgb)
    cq, _, _ = oracle.reconstruct(co, 64, 48, np.full((3, 64), 3, np.int32))
    nb = co.shape[1]
    L = capi.Library(lib_path)
    off = np.zeros(nb + 1, np.int32)
    idx = np.zeros(nb * 192, np.uint8)
    assert L.lib.gz_rank_zeroing_candidates(cq.ctypes.data, co.ctypes.data, nb, 1,
                                            off.ctypes.data, idx.ctypes.data) == 0
    for b in range(nb):
        cand = [(c * 64 + k) for c in range(3) for k in range(1, 64) if cq[c, b, k] != 0]
        score = np.array([np.float32(np.float32(abs(int(co[i // 64, b, i % 64]))) * csf[i]) + bias[i]
                          for i in cand], np.float32)
        if len(set(score.tolist())) != len(score):
            continue   # ties: order is libstdc++-specific, covered by the GPU parity tests
        exp = [cand[j] for j in np.argsort(score, kind="stable")]
        assert idx[off[b]:off[b + 1]].tolist() == exp, b
    assert off[-1] > 500


def test_tensor_argument_rules_stand_alone(tmp_path):
    """tests/cpp/tensor_args.cc: the one extent rule, distinct-addresses rule and last-offset function behind every
    device-tensor entry (guetzli_amd/csrc/api/tensor.h) and the six ABI structs' adapters, compiled without HIP and without
    the emulation -- every small view against brute force, the 62-bit boundary, each struct's own rules -- as a plain
    program with AddressSanitizer and UBSan.  Its own process, nothing preloaded."""
    import subprocess
    exe = str(tmp_path / "tensor_args")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", os.path.join(ROOT, "tests", "cpp", "tensor_args.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tensor arguments: all as expected" in out.stdout


def test_new_entry_points_reject_bad_arguments(lib_path):
    """Phase-B / JPEG-input / dct_double entry points: null context or buffers give GZ_E_ARG
    (never a crash, never a fallback)."""
    L = capi.Library(lib_path)
    lib = L.lib
    z = np.zeros(64, np.int32)
    u64 = np.zeros(1, np.uint64)
    assert lib.gz_order_reset(None) == -1
    assert lib.gz_steps_histogram_delta(None, z.ctypes.data) == -1
    assert lib.gz_compare_begin(None) == -1 and lib.gz_compare_end(None, z.ctypes.data) == -1
    assert lib.gz_probe_rank_sort(0, None, None, 1, None) == -1
    assert lib.gz_probe_scan_offsets(0, None, 1, None, 1, 0, None) == -1
    assert lib.gz_probe_scan_offsets(0, z.ctypes.data, 1, z.ctypes.data, 1, 0x3fffffff, u64.ctypes.data) == -1
    assert lib.gz_probe_set_block_max(None, z.ctypes.data) == -1
    assert lib.gz_probe_set_search(None, 7, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1
    assert lib.gz_probe_order_state(None, z.ctypes.data, z.ctypes.data) == -1
    assert lib.gz_trim_pool() == 0          # nothing cached: nothing to release, no device needed
    assert lib.gz_order_build(None, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0, 0.0,
                              u64.ctypes.data, z.ctypes.data, None) == -1
    assert lib.gz_order_build_auto(None, 1, 1, 1.0, 0, z.ctypes.data, 0, 0.0, u64.ctypes.data,
                                   z.ctypes.data, None) == -1
    assert lib.gz_order_partition(None, 0, 10, u64.ctypes.data) == -1
    assert lib.gz_order_fetch(None, 0, 0, z.ctypes.data) == -1
    assert lib.gz_order_advance(None, 0.0, 1) == -1
    assert lib.gz_order_upload(None, None, 0) == -1
    assert lib.gz_apply_candidate_steps(None, 1, z.ctypes.data, z.ctypes.data, 1) == -1
    assert lib.gz_apply_coeff_edits(None, z.ctypes.data, z.ctypes.data, 1) == -1
    assert lib.gz_set_rgb(None, z.ctypes.data) == -1
    assert lib.gz_dct_double_blocks(0, None, 1, 0) == -1
    assert lib.gz_component_to_float_pixels(0, None, 8, 8, None) == -1
    assert lib.gz_component_set_downsampled(0, z.ctypes.data, 8, 8, 9, 1, z.ctypes.data) == -1
    assert lib.gz_encode_rgb_only(0, None, 8, 8, None) == -1
    assert lib.gz_encode_rgb_only(0, z.ctypes.data, 0, 8, z.ctypes.data) == -1

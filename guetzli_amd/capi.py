"""ctypes binding of the C ABI in include/guetzli_amd.h.

`load()` opens guetzli_amd/libguetzli_amd.so -- the hipcc-built gfx950 library -- and
nothing else: there is no CPU implementation behind this module, and a missing library or
a missing GPU is an error, not a fallback.  (The test-suite's CPU emulation build of the
kernel sources is loaded by tests through `Library(path)` explicitly; the package never
does that.)
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "libguetzli_amd.so")

GZ_OK = 0
ERRORS = {-1: "GZ_E_ARG", -2: "GZ_E_NO_DEVICE", -3: "GZ_E_HIP", -4: "GZ_E_STATE",
          -5: "GZ_E_NOMEM"}

_P = C.c_void_p
_I = C.c_int


class GzConfig(C.Structure):
    """gz_config of include/guetzli_amd.h."""
    _fields_ = [("struct_size", _I), ("blur_packed", _I), ("tile_rows", _I), ("single_stream", _I),
                ("store_distmap", _I), ("patch_reconstruct", _I), ("opsin_ahead", _I)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


GZ_DT_U8, GZ_DT_F32, GZ_DT_F16, GZ_DT_BF16 = 0, 1, 2, 3
GZ_DT_U16 = 4   # gz_device_pixels only
GZ_SAMPLES_SRGB8, GZ_SAMPLES_LINEAR = 0, 1   # how gz_opsin_device / gz_mask_device read an image's elements


class GzDeviceImage(C.Structure):
    """gz_device_image of include/guetzli_amd.h: a strided w x h x 3 image in device memory."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_y", C.c_int64), ("stride_x", C.c_int64),
                ("stride_c", C.c_int64), ("producer_stream", _P)]


def device_image(ptr, dtype, strides, stream=0):
    """A GzDeviceImage: ptr = device address of element (0, 0, 0), dtype = GZ_DT_*, strides = (y, x, c) in elements,
    stream = the hipStream_t whose work produced the data (0: none to wait for)."""
    sy, sx, sc = (int(v) for v in strides)
    return GzDeviceImage(C.sizeof(GzDeviceImage), int(dtype), int(ptr) or None, sy, sx, sc, int(stream) or None)


class GzDevicePixels(C.Structure):
    """gz_device_pixels of include/guetzli_amd.h: gz_device_image with GZ_DT_U16, an alpha pointer and a background."""
    _fields_ = GzDeviceImage._fields_ + [("alpha", _P), ("background", C.c_uint8 * 4)]


def device_pixels(ptr, dtype, strides, stream=0, alpha=0, background=(0, 0, 0)):
    """A GzDevicePixels: as device_image, and alpha = device address of the alpha sample of pixel (0, 0) (0: opaque),
    background = the bytes (r, g, b) the pixels are blended over."""
    sy, sx, sc = (int(v) for v in strides)
    r, g, b = (int(v) for v in background)
    return GzDevicePixels(C.sizeof(GzDevicePixels), int(dtype), int(ptr) or None, sy, sx, sc, int(stream) or None,
                          int(alpha) or None, (C.c_uint8 * 4)(r, g, b, 0))


class GzDeviceOutput(C.Structure):
    """gz_device_output of include/guetzli_amd.h: where decoded pixels go, a strided w x h x 3 image in device memory."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_y", C.c_int64), ("stride_x", C.c_int64),
                ("stride_c", C.c_int64), ("consumer_stream", _P)]


def device_output(ptr, dtype, strides, stream=0):
    """A GzDeviceOutput: ptr = device address of element (0, 0, 0), dtype = GZ_DT_*, strides = (y, x, c) in elements,
    stream = the hipStream_t that used the memory before and reads it afterwards (0: none)."""
    sy, sx, sc = (int(v) for v in strides)
    return GzDeviceOutput(C.sizeof(GzDeviceOutput), int(dtype), int(ptr) or None, sy, sx, sc, int(stream) or None)


class GzHuffmanSpec(C.Structure):
    _fields_ = [("counts", C.c_uint8 * 16), ("values", C.c_uint8 * 256)]


class GzScan(C.Structure):
    """gz_scan of include/guetzli_amd.h: an eligible baseline scan, its tables and quantisers."""
    _fields_ = [("struct_size", _I), ("w", _I), ("h", _I), ("ncomp", _I), ("chroma_factor", _I), ("data", _P), ("len", C.c_uint64),
                ("dc", GzHuffmanSpec * 3), ("ac", GzHuffmanSpec * 3), ("quant", (_I * 64) * 3), ("subseq_bytes", _I),
                ("max_sync_rounds", _I)]


class GzScanResult(C.Structure):
    _fields_ = [("status", _I), ("subsequences", _I), ("sync_rounds", _I), ("reserved", _I), ("end_offset", C.c_uint64)]


SCAN_STATUS = {0: "DECODED", 1: "NOT_CONVERGED", 2: "BAD_SYMBOL", 3: "RUN_PAST_BAND", 4: "DC_RANGE", 5: "COEFF_RANGE", 6: "ENDS_EARLY"}


def scan_spec(w, h, ncomp, chroma_factor, data, dc, ac, quant, subseq_bytes=0, max_sync_rounds=0):
    """A GzScan.  data: the bytes from behind the SOS header to the end of the file (kept alive by the returned object);
    dc / ac: per component (counts[16], values) as a DHT holds them; quant: per component 64 quantisers, natural order."""
    sc = GzScan()
    sc.struct_size = C.sizeof(GzScan)
    sc.w, sc.h, sc.ncomp, sc.chroma_factor = int(w), int(h), int(ncomp), int(chroma_factor)
    buf = np.frombuffer(bytes(data), np.uint8)
    sc._keep = buf
    sc.data = buf.ctypes.data if buf.size else None
    sc.len = buf.size
    for c in range(min(3, len(dc))):
        for spec, (counts, values) in ((sc.dc[c], dc[c]), (sc.ac[c], ac[c])):
            for i, v in enumerate(counts):
                spec.counts[i] = int(v)
            for i, v in enumerate(values):
                spec.values[i] = int(v)
        for k in range(64):
            sc.quant[c][k] = int(quant[c][k])
    sc.subseq_bytes, sc.max_sync_rounds = int(subseq_bytes), int(max_sync_rounds)
    return sc


class GzDeviceMap(C.Structure):
    """gz_device_map of include/guetzli_amd.h: where a distance map goes, a strided w x h image in device memory."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_y", C.c_int64), ("stride_x", C.c_int64),
                ("consumer_stream", _P)]


def device_map(ptr, dtype, strides, stream=0):
    """A GzDeviceMap: ptr = device address of element (0, 0), dtype = GZ_DT_F32 / GZ_DT_F16 / GZ_DT_BF16, strides =
    (y, x) in elements, stream = the hipStream_t that used the memory before and reads it afterwards (0: none)."""
    sy, sx = (int(v) for v in strides)
    return GzDeviceMap(C.sizeof(GzDeviceMap), int(dtype), int(ptr) or None, sy, sx, int(stream) or None)


class GzDeviceBatch(C.Structure):
    """gz_device_batch of include/guetzli_amd.h: n strided images of one size in device memory."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_n", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64), ("stride_c", C.c_int64), ("producer_stream", _P)]


def device_batch(ptr, dtype, strides, stream=0):
    """A GzDeviceBatch: ptr = device address of element (0, 0, 0, 0), dtype = GZ_DT_U8 / F32 / F16 / BF16, strides =
    (n, y, x, c) in elements, stream = the hipStream_t whose work produced the data (0: none to wait for)."""
    sn, sy, sx, sc = (int(v) for v in strides)
    return GzDeviceBatch(C.sizeof(GzDeviceBatch), int(dtype), int(ptr) or None, sn, sy, sx, sc, int(stream) or None)


class GzDeviceOutputBatch(C.Structure):
    """gz_device_output_batch of include/guetzli_amd.h: n strided images of one size in device memory that are written."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_n", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64), ("stride_c", C.c_int64), ("consumer_stream", _P), ("n", _I)]


def device_output_batch(ptr, dtype, strides, n, stream=0):
    """A GzDeviceOutputBatch: ptr = device address of element (0, 0, 0, 0), dtype = GZ_DT_*, strides = (n, y, x, c) in
    elements, n = its images, stream = the hipStream_t that used the memory before and reads it afterwards (0: none)."""
    sn, sy, sx, sc = (int(v) for v in strides)
    return GzDeviceOutputBatch(C.sizeof(GzDeviceOutputBatch), int(dtype), int(ptr) or None, sn, sy, sx, sc, int(stream) or None, int(n))


class GzDeviceMapBatch(C.Structure):
    """gz_device_map_batch of include/guetzli_amd.h: where n distance maps go."""
    _fields_ = [("struct_size", _I), ("dtype", _I), ("data", _P), ("stride_n", C.c_int64), ("stride_y", C.c_int64),
                ("stride_x", C.c_int64), ("consumer_stream", _P)]


def device_map_batch(ptr, dtype, strides, stream=0):
    """A GzDeviceMapBatch: ptr = device address of element (0, 0, 0), dtype = GZ_DT_F32 / F16 / BF16, strides = (n, y, x)
    in elements, stream = the hipStream_t that used the memory before and reads it afterwards (0: none)."""
    sn, sy, sx = (int(v) for v in strides)
    return GzDeviceMapBatch(C.sizeof(GzDeviceMapBatch), int(dtype), int(ptr) or None, sn, sy, sx, int(stream) or None)


# name -> (restype, argtypes); mirrors include/guetzli_amd.h one to one
SIGNATURES = {
    "gz_abi_version": (_I, []),
    "gz_device_count": (_I, []),
    "gz_strerror": (C.c_char_p, [_I]),
    "gz_last_error": (C.c_char_p, [_P]),
    "gz_hint_images_in_flight": (None, [_I]),
    "gz_device_pci_bus_id": (_I, [_I, _P, _I]),
    "gz_config_from_environment": (_I, [_P]),
    "gz_get_config": (_I, [_P, _P]),
    "gz_set_config": (_I, [_P, _P]),
    "gz_create": (_P, [_I, _I, _I, _P, C.c_float, C.POINTER(_I)]),
    "gz_destroy": (None, [_P]),
    "gz_set_rgb": (_I, [_P, _P]),
    "gz_create_from_device": (_P, [_I, _I, _I, _P, C.c_float, C.POINTER(_I)]),
    "gz_set_rgb_device": (_I, [_P, _P]),
    "gz_pack_rgb_device": (_I, [_I, _P, _I, _I, _P]),
    "gz_create_from_device_pixels": (_P, [_I, _I, _I, _P, C.c_float, C.POINTER(_I)]),
    "gz_set_rgb_device_pixels": (_I, [_P, _P]),
    "gz_pack_rgb_device_pixels": (_I, [_I, _P, _I, _I, _P]),
    "gz_decode_coeffs_device": (_I, [_I, _P, _I, _I, _I, _P]),
    "gz_decode_coeffs": (_I, [_I, _P, _I, _I, _I, _P]),
    "gz_reconstruct_device": (_I, [_P, _P]),
    "gz_decode_scan": (_I, [_I, _P, _P, _P]),
    "gz_decode_scan_device": (_I, [_I, _P, _P, _P]),
    "gz_decode_scan_input": (_I, [_I, _P, _P, _P, _P]),
    "gz_decode_scan_batch_device": (_I, [_I, _I, _P, _P, _P, _P, C.c_size_t]),
    "gz_compare_device_pixels": (_I, [_P, _P, _P, _P]),
    "gz_compare_rgb": (_I, [_P, _P, _P, _P]),
    "gz_distmap_device": (_I, [_P, _P]),
    "gz_probe_emit_map": (_I, [_I, _P, _I, _I, _P]),
    "gz_butteraugli_fuzzy_class": (C.c_double, [C.c_double]),
    "gz_butteraugli_fuzzy_inverse": (C.c_double, [C.c_double]),
    "gz_heatmap_device": (_I, [_P, C.c_double, C.c_double, _P]),
    "gz_compare_device_pixels_heat": (_I, [_P, _P, _P, _P, _P, C.c_double, C.c_double]),
    "gz_heatmap_from_map_device": (_I, [_I, _P, _I, _I, _I, C.c_double, C.c_double, _P]),
    "gz_probe_emit_heat": (_I, [_I, _P, _I, _I, C.c_double, C.c_double, _P]),
    "gz_probe_heat_thresholds": (_I, [_P]),
    "gz_create_from_device_linear": (_P, [_I, _I, _I, _P, C.c_float, C.POINTER(_I)]),
    "gz_set_linear_device": (_I, [_P, _P, C.c_float]),
    "gz_compare_device_linear": (_I, [_P, _P, C.c_float, _P, _P, _P, C.c_double, C.c_double, _P]),
    "gz_butteraugli_linear": (_I, [_I, _I, _I, _P, _P, C.c_float, _P, _P, _P, C.c_double, C.c_double, _P]),
    "gz_probe_linear_planes": (_I, [_P, _P]),
    "gz_butteraugli_batch": (_I, [_I, _I, _I, _I, _P, _I, _P, _P, _P, _P, C.c_size_t]),
    "gz_opsin_device": (_I, [_I, _I, _I, _P, _I, C.c_float, _P, _P]),
    "gz_mask_device": (_I, [_I, _I, _I, _P, _P, _I, C.c_float, _P, _P, _P]),
    "gz_adaptive_quantization": (_I, [_I, _I, _I, _P, C.c_float, _P, _P]),
    "gz_synchronize": (_I, [_P]),
    "gz_set_stream": (_I, [_P, _P]),
    "gz_encode_rgb": (_I, [_P, _P]),
    "gz_encode_rgb_only": (_I, [_I, _P, _I, _I, _P]),
    "gz_set_orig_coeffs": (_I, [_P, _P]),
    "gz_set_orig_coeffs_420": (_I, [_P, _P]),
    "gz_downsample": (_I, [_P, _P]),
    "gz_downsample_planes": (_I, [_P, _P, _P, _P, _P]),
    "gz_downsample_silver": (_I, [_P, _P, _P]),
    "gz_probe_silver_yuv420": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "gz_frame_layout": (_I, [_P, _P, _P, _P]),
    "gz_quantize": (_I, [_P, _P, _P]),
    "gz_set_coeffs": (_I, [_P, _P]),
    "gz_set_coeff_blocks": (_I, [_P, _P, _I, _P]),
    "gz_get_coeffs": (_I, [_P, _P]),
    "gz_reconstruct": (_I, [_P, _P, _P]),
    "gz_trim_pool": (_I, []),
    "gz_compare": (_I, [_P, _P, _P, _P]),
    "gz_compare_begin": (_I, [_P]),
    "gz_compare_end": (_I, [_P, _P]),
    "gz_compare_enqueue": (_I, [_P, _I]),
    "gz_last_distance": (_I, [_P, _P]),
    "gz_time_compare": (_I, [_P, _I, _P]),
    "gz_block_weights": (_I, [_P, _I, _I, C.c_double, _I, _P]),
    "gz_block_weights_factor": (_I, [_P, _I, _I, C.c_double, _I, _I, _P]),
    "gz_block_zeroing_orders": (_I, [_P, _I, _I, _P, _P, _P, _I]),
    "gz_block_zeroing_orders_masked": (_I, [_P, _I, _I, _I, _P, _P, _P, _I]),
    "gz_compare_blocks": (_I, [_P, _I, _P, _P, _P]),
    "gz_compare_block_pixels": (_I, [_P, _I, _P, _P, _P]),
    "gz_set_frame": (_I, [_P, _I]),
    "gz_search_evaluations": (_I, [_P, _P]),
    "gz_compare_counters": (_I, [_P]),
    "gz_rank_zeroing_candidates": (_I, [_P, _P, _I, _I, _P, _P]),
    "gz_probe_rank_sort": (_I, [_I, _P, _P, _I, _P]),
    "gz_order_build": (_I, [_P, _I, _P, _P, _P, _I, C.c_float, _P, _P, _P]),
    "gz_order_reset": (_I, [_P]),
    "gz_order_build_auto": (_I, [_P, _I, _I, C.c_double, _I, _P, _I, C.c_float, _P, _P, _P]),
    "gz_order_build_auto_begin": (_I, [_P, _I, _I, C.c_double, _I, _P, _I, C.c_float]),
    "gz_order_build_auto_descend_begin": (_I, [_P, _I, _I, C.c_double, _I, _P, _I, C.c_float, C.c_float, C.c_uint64, _I]),
    "gz_order_build_auto_end": (_I, [_P, _P, _P, _P]),
    "gz_order_advance": (_I, [_P, C.c_float, _I]),
    "gz_apply_coeff_edits": (_I, [_P, _P, _P, _I]),
    "gz_apply_candidate_steps": (_I, [_P, _I, _P, _P, _I]),
    "gz_steps_histogram_delta": (_I, [_P, _P]),
    "gz_order_upload": (_I, [_P, _P, C.c_uint64]),
    "gz_order_partition": (_I, [_P, C.c_uint64, C.c_uint64, _P]),
    "gz_order_fetch": (_I, [_P, C.c_uint64, C.c_uint64, _P]),
    "gz_order_host_mirror": (_I, [_P, C.c_uint64, _P]),
    "gz_order_exported": (_I, [_P, _P]),
    "gz_order_descend": (_I, [_P, C.c_uint64, C.c_uint64, _I, _P, _P]),
    "gz_order_descend_begin": (_I, [_P, C.c_float, C.c_uint64, _I]),
    "gz_order_descend_end": (_I, [_P, _P, _I, _P, _P]),
    "gz_jpeg_histograms": (_I, [_P, _P, _P]),
    "gz_jpeg_histograms_ncomp": (_I, [_P, _P, _I, _P]),
    "gz_jpeg_scan": (_I, [_P, _I, _P, _P, _P]),
    "gz_jpeg_scan_begin": (_I, [_P, _I, _P, _P]),
    "gz_jpeg_scan_end": (_I, [_P, _P]),
    "gz_jpeg_scan_keep": (_I, [_P]),
    "gz_jpeg_scan_bits": (_I, [_P, _P, _P]),
    "gz_jpeg_scan_bytes": (_I, [_P, _I, _P, C.c_size_t, _P]),
    "gz_probe_blur": (_I, [_P, _P, C.c_float, C.c_float, _P]),
    "gz_probe_opsin": (_I, [_P, _P, _P]),
    "gz_probe_separate_frequencies": (_I, [_P, _P, _P]),
    "gz_probe_diffmap": (_I, [_P, _P, _P, _P, _P]),
    "gz_probe_mask": (_I, [_P, _P, _P, _P, _P]),
    "gz_probe_idct_blocks": (_I, [_I, _P, _I, _P]),
    "gz_probe_fdct_blocks": (_I, [_I, _P, _I]),
    "gz_probe_arith": (_I, [_I, _I, _P, _P, _P, _P, _I]),
    "gz_probe_math": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "gz_probe_div2_sweep": (_I, [_I, _P, _I, C.c_uint, C.c_uint, _P, _P, C.c_size_t]),
    "gz_probe_scan_offsets": (_I, [_I, _P, _I, _P, _I, C.c_uint, _P]),
    "gz_probe_set_block_max": (_I, [_P, _P]),
    "gz_probe_set_search": (_I, [_P, _I, _P, _P, _P]),
    "gz_probe_order_state": (_I, [_P, _P, _P]),
    "gz_dct_double_blocks": (_I, [_I, _P, _I, _I]),
    "gz_component_to_float_pixels": (_I, [_I, _P, _I, _I, _P]),
    "gz_component_set_downsampled": (_I, [_I, _P, _I, _I, _I, _I, _P]),
}


class GuetzliAmdError(RuntimeError):
    pass


def _ptr(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"], "need a C-contiguous array"
    return a.ctypes.data


class Library:
    def __init__(self, path=DEFAULT_LIB):
        if not os.path.exists(path):
            raise GuetzliAmdError(
                f"{path} not found: build it with `python -m guetzli_amd.build` (hipcc, "
                "gfx950).  There is no CPU fallback.")
        self.path = path
        self.lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(self.lib, name)   # AttributeError if the ABI is incomplete
            f.restype, f.argtypes = res, args

    def check(self, rc, ctx=None):
        if rc != GZ_OK:
            msg = self.lib.gz_strerror(rc).decode()
            if ctx:
                msg += ": " + self.lib.gz_last_error(ctx).decode()
            raise GuetzliAmdError(f"{ERRORS.get(rc, rc)} ({msg})")

    def device_count(self):
        return self.lib.gz_device_count()

    def device_pci_bus_id(self, device=0):
        buf = C.create_string_buffer(32)
        self.check(self.lib.gz_device_pci_bus_id(device, buf, 32))
        return buf.value.decode()

    def config_from_environment(self):
        cfg = GzConfig()
        self.check(self.lib.gz_config_from_environment(C.byref(cfg)))
        return cfg

    def compare_counters(self, all=False):
        """(Compares that skipped the full reconstruction, of them checked against one, Compares in all) since load;
        all=True: + (Compares that found their opsin image in place, of them checked)."""
        n = np.zeros(5, np.uint64)
        self.check(self.lib.gz_compare_counters(_ptr(n)))
        return tuple(int(x) for x in (n if all else n[:3]))

    # ---- context-free probes ----
    def idct_blocks(self, blocks, device=0):
        b = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
        out = np.zeros(b.shape, np.uint8)
        self.check(self.lib.gz_probe_idct_blocks(device, _ptr(b), b.shape[0], _ptr(out)))
        return out

    def fdct_blocks(self, blocks, device=0):
        b = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64).copy()
        self.check(self.lib.gz_probe_fdct_blocks(device, _ptr(b), b.shape[0]))
        return b

    def encode_rgb_only(self, rgb, device=0):
        """EncodeRGBToJpeg's transform (q = 1) without a context, any size >= 1x1."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w, _ = rgb.shape
        nb = ((w + 7) // 8) * ((h + 7) // 8)
        out = np.zeros((3, nb, 64), np.int16)
        self.check(self.lib.gz_encode_rgb_only(device, _ptr(rgb), w, h, _ptr(out)))
        return out

    def dct_double_blocks(self, blocks, inverse=False, device=0):
        """ComputeBlockDCTDouble / ComputeBlockIDCTDouble (dct_double.cc:76-85) per block."""
        b = np.ascontiguousarray(blocks, np.float64).reshape(-1, 64).copy()
        self.check(self.lib.gz_dct_double_blocks(device, _ptr(b), b.shape[0], int(inverse)))
        return b

    def component_to_float_pixels(self, coeffs, w, h, device=0):
        """OutputImageComponent::ToFloatPixels (output_image.cc:99-121), stride 1."""
        nb = ((w + 7) // 8) * ((h + 7) // 8)
        co = np.ascontiguousarray(coeffs, np.int16)
        assert co.size == nb * 64
        out = np.zeros((h, w), np.float32)
        self.check(self.lib.gz_component_to_float_pixels(device, _ptr(co), w, h, _ptr(out)))
        return out

    def component_set_downsampled(self, pixels, fx, fy, device=0):
        """SetDownsampledCoefficients (output_image.cc:265-300) of an h x w float plane."""
        px = np.ascontiguousarray(pixels, np.float32)
        h, w = px.shape
        nb = ((w + 8 * fx - 1) // (8 * fx)) * ((h + 8 * fy - 1) // (8 * fy))
        out = np.zeros((nb, 64), np.int16)
        self.check(self.lib.gz_component_set_downsampled(device, _ptr(px), w, h, fx, fy,
                                                         _ptr(out)))
        return out

    def arith(self, op, a, b=None, c=None, device=0):
        dt = np.float64 if op in (2, 3, 5, 6) else np.float32
        odt = np.float64 if op in (2, 3, 5) else np.float32
        a = np.ascontiguousarray(a, dt)
        b = None if b is None else np.ascontiguousarray(b, dt)
        c = None if c is None else np.ascontiguousarray(c, dt)
        out = np.zeros(a.shape, odt)
        self.check(self.lib.gz_probe_arith(device, op, _ptr(a), _ptr(b), _ptr(c), _ptr(out),
                                           a.size))
        return out

    def probe_math(self, op, a, b=None, c=None, p=(), outs=1, device=0):
        """gz_probe_math: op = GZ_MATH_* of include/guetzli_amd.h; float arrays (doubles for
        GZ_MATH_INTERP_LUT512 = 15 and GZ_MATH_POW_TO_FLOAT = 17, int32 for GZ_MATH_QUANT_DIV = 16); returns [outs][n]."""
        dt = np.float64 if op in (15, 17) else np.int32 if op == 16 else np.float32
        a = np.ascontiguousarray(a, dt)
        b = None if b is None else np.ascontiguousarray(b, dt)
        c = None if c is None else np.ascontiguousarray(c, dt)
        n = a.size // 3 if op == 4 else a.size
        pp = np.ascontiguousarray(p, np.float64)
        out = np.zeros((outs, n), dt)
        self.check(self.lib.gz_probe_math(device, op, n, _ptr(a), _ptr(b), _ptr(c),
                                          _ptr(pp) if pp.size else None, pp.size, _ptr(out)))
        return out

    def probe_silver_yuv420(self, srgb, guard_log2=40, device=0):
        """gz_probe_silver_yuv420: RGBToYUV420 of a packed sRGB image on the device -> (y, u, v, counters), float32 [h][w]
        planes and (cell-passes evaluated, cell-passes redone on the host).  guard_log2: 40 as the encoder runs it,
        -1 every cell through the host path, 64 no guard."""
        rgb = np.ascontiguousarray(srgb, np.uint8)
        h, w, ch = rgb.shape
        assert ch == 3
        y, u, v = (np.zeros((h, w), np.float32) for _ in range(3))
        cnt = np.zeros(2, np.uint64)
        self.check(self.lib.gz_probe_silver_yuv420(device, _ptr(rgb), w, h, int(guard_log2), _ptr(y), _ptr(u), _ptr(v),
                                                   _ptr(cnt)))
        return y, u, v, (int(cnt[0]), int(cnt[1]))

    def probe_scan_offsets(self, values, lengths, start_epoch=0, device=0):
        """gz_probe_scan_offsets: k_scan_offsets once per entry of `lengths` on a prefix of `values`, back to back on
        one scratch -> a list of uint64 arrays off[0 .. lengths[i]]."""
        v = np.ascontiguousarray(values, np.uint32)
        ln = np.ascontiguousarray(lengths, np.int32)
        out = np.zeros(int(ln.astype(np.int64).sum()) + ln.size, np.uint64)
        self.check(self.lib.gz_probe_scan_offsets(device, _ptr(v), v.size, _ptr(ln), ln.size, int(start_epoch),
                                                  _ptr(out)))
        ends = np.cumsum(ln.astype(np.int64) + 1)
        return [out[e - n - 1:e] for e, n in zip(ends, ln)]

    def div2_sweep(self, numerators, stride=1, sample_every=1 << 20, device=0):
        """gz_probe_div2_sweep: (mismatches, sampled quotients [samples][len(numerators)])."""
        num = np.ascontiguousarray(numerators, np.float32)
        count = -(-(80 << 23) // stride)
        sample = np.zeros((-(-count // sample_every), num.size), np.float32)
        bad = C.c_uint64(0)
        self.check(self.lib.gz_probe_div2_sweep(device, _ptr(num), num.size, stride, sample_every,
                                                C.byref(bad), _ptr(sample), sample.size))
        return bad.value, sample

    def context(self, rgb, target, device=0):
        return Context(self, rgb, target, device)

    def context_from_device(self, image, w, h, target, device=0):
        """gz_create_from_device: a context whose original is the device-resident `image` (device_image(...))."""
        return Context.from_device(self, image, w, h, target, device)

    def context_from_device_linear(self, image, w, h, scale=1.0, device=0):
        """gz_create_from_device_linear: a context whose original is the LINEAR float image `image` (device_pixels(...)
        of float32 / float16 / bfloat16, raw intensity 0..255 after `scale`)."""
        return Context.from_device_linear(self, image, w, h, scale, device)

    def butteraugli_linear(self, ref, other, w, h, scale=1.0, dmap=None, heat=None, good=0.0, bad=0.0, device=0):
        """gz_butteraugli_linear: ButteraugliInterface of two linear float images (device_pixels(...)), any size from
        1 x 1 -> (distance, elements the clamp to [0, 255] altered, of both images)."""
        dist = np.zeros(1, np.float32)
        clamped = C.c_uint64(0)
        self.check(self.lib.gz_butteraugli_linear(device, w, h, C.byref(ref), C.byref(other), float(scale), _ptr(dist),
                                                  None if dmap is None else C.byref(dmap), None if heat is None else C.byref(heat),
                                                  good, bad, C.byref(clamped)))
        return float(dist[0]), clamped.value

    def butteraugli_batch(self, ref, other, w, h, n, distances, n_ref=None, maps=None, scratch_bytes=0, device=0):
        """gz_butteraugli_batch: n pairs of w x h images (device_batch(...); ref holds n_ref = n or 1 images) through one
        chain.  distances = device address of n float32; maps = device_map_batch(...) or None -> the n distances as a
        float32 array on the host."""
        host = np.zeros(n, np.float32)
        self.check(self.lib.gz_butteraugli_batch(device, w, h, n, C.byref(ref), n if n_ref is None else n_ref, C.byref(other),
                                                 int(distances) or None, _ptr(host), None if maps is None else C.byref(maps),
                                                 int(scratch_bytes)))
        return host

    def opsin_device(self, image, w, h, xyb, samples=GZ_SAMPLES_SRGB8, scale=1.0, device=0):
        """gz_opsin_device: OpsinDynamicsImage of `image` (device_pixels(...), read as `samples` say) into `xyb`
        (device_output(...) of a float type) -> elements the linear reader's clamp altered."""
        clamped = C.c_uint64(0)
        self.check(self.lib.gz_opsin_device(device, w, h, C.byref(image), samples, float(scale), C.byref(xyb), C.byref(clamped)))
        return clamped.value

    def mask_device(self, image0, image1, w, h, mask=None, mask_dc=None, samples=GZ_SAMPLES_SRGB8, scale=1.0, device=0):
        """gz_mask_device: Mask of the opsin images of `image0` and `image1` (None: image0 again) into `mask` and / or
        `mask_dc` (device_output(...) of a float type) -> elements the clamp altered, of both images."""
        clamped = C.c_uint64(0)
        self.check(self.lib.gz_mask_device(device, w, h, C.byref(image0), None if image1 is None else C.byref(image1), samples, float(scale),
                                           None if mask is None else C.byref(mask), None if mask_dc is None else C.byref(mask_dc),
                                           C.byref(clamped)))
        return clamped.value

    def adaptive_quantization(self, image, w, h, quant, scale=1.0, device=0):
        """gz_adaptive_quantization: ButteraugliAdaptiveQuantization of the linear float `image` (device_pixels(...)) into
        `quant` (device_map(...)) -> elements the clamp altered."""
        clamped = C.c_uint64(0)
        self.check(self.lib.gz_adaptive_quantization(device, w, h, C.byref(image), float(scale), C.byref(quant), C.byref(clamped)))
        return clamped.value

    def pack_rgb_device(self, image, w, h, device=0):
        """gz_pack_rgb_device / gz_pack_rgb_device_pixels: the ingest kernel's bytes of `image` (device_image(...) /
        device_pixels(...)) -> uint8 [h][w][3]."""
        out = np.zeros((h, w, 3), np.uint8)
        entry = self.lib.gz_pack_rgb_device_pixels if isinstance(image, GzDevicePixels) else self.lib.gz_pack_rgb_device
        self.check(entry(device, C.byref(image), w, h, _ptr(out)))
        return out

    def decode_coeffs(self, coeffs, w, h, chroma_factor=1, device=0):
        """gz_decode_coeffs: OutputImage::ToSRGB of dequantised coefficients (frame layout of the header) without a
        context -> uint8 [h][w][3]."""
        co = np.ascontiguousarray(coeffs, np.int16)
        out = np.zeros((h, w, 3), np.uint8)
        self.check(self.lib.gz_decode_coeffs(device, _ptr(co), w, h, chroma_factor, _ptr(out)))
        return out

    def decode_coeffs_device(self, coeffs, w, h, output, chroma_factor=1, device=0):
        """gz_decode_coeffs_device: the same written into `output` (device_output(...))."""
        co = np.ascontiguousarray(coeffs, np.int16)
        self.check(self.lib.gz_decode_coeffs_device(device, _ptr(co), w, h, chroma_factor, C.byref(output)))

    @staticmethod
    def _scan_result(res):
        return {"status": SCAN_STATUS.get(res.status, res.status), "subsequences": res.subsequences, "sync_rounds": res.sync_rounds,
                "end_offset": int(res.end_offset)}

    def decode_scan(self, scan, device=0):
        """gz_decode_scan: a baseline scan (scan_spec(...)) read on the device -> (dequantised coefficients int16
        [nb + 2 nbc][64] in the frame layout, or None where the status is not "DECODED"; the gz_scan_result as a dict)."""
        f = scan.chroma_factor if scan.chroma_factor in (1, 2) else 1
        nb = ((scan.w + 7) // 8) * ((scan.h + 7) // 8)
        nbc = ((scan.w + 8 * f - 1) // (8 * f)) * ((scan.h + 8 * f - 1) // (8 * f))
        out = np.full((max(nb + 2 * nbc, 1), 64), 0x5a5a, np.int16)
        res = GzScanResult()
        self.check(self.lib.gz_decode_scan(device, C.byref(scan), _ptr(out), C.byref(res)))
        r = self._scan_result(res)
        if r["status"] != "DECODED":
            assert (out == 0x5a5a).all(), "coefficients written without a verdict"
            return None, r
        return out, r

    def decode_scan_device(self, scan, output, device=0):
        """gz_decode_scan_device: the scan's pixels into `output` (device_output(...)) where the status is "DECODED"
        -> the gz_scan_result as a dict."""
        res = GzScanResult()
        self.check(self.lib.gz_decode_scan_device(device, C.byref(scan), C.byref(output), C.byref(res)))
        return self._scan_result(res)

    def decode_scan_batch_device(self, scans, slots, output, scratch_bytes=0, device=0, results=None):
        """gz_decode_scan_batch_device: the pixels of scans[i] (scan_spec(...)) into image slots[i] of `output`
        (device_output_batch(...)) where its status is "DECODED" -> the gz_scan_results as dicts.  results: a list that
        receives them whether the call succeeds or not."""
        n = len(scans)
        arr = (GzScan * max(n, 1))()
        for i, sc in enumerate(scans):
            C.memmove(C.byref(arr, i * C.sizeof(GzScan)), C.byref(sc), C.sizeof(GzScan))
        res = (GzScanResult * max(n, 1))()
        sl = (_I * max(n, 1))(*[int(v) for v in slots])
        try:
            self.check(self.lib.gz_decode_scan_batch_device(device, n, arr, sl, C.byref(output), res, int(scratch_bytes)))
        finally:
            if results is not None:
                results[:] = [self._scan_result(res[i]) for i in range(n)]
        return [self._scan_result(res[i]) for i in range(n)]

    def decode_scan_input(self, scan, device=0):
        """gz_decode_scan_input: the scan as the host READER leaves it -> (per component the quantised coefficients int16
        [height_in_blocks][width_in_blocks][64] on its grid padded to whole MCUs, or None where the status is not
        "DECODED"; CheckJpegSanity's verdict, True = refused, or None; the gz_scan_result as a dict)."""
        f = scan.chroma_factor if scan.chroma_factor in (1, 2) else 1
        cols, rows = (scan.w + 8 * f - 1) // (8 * f), (scan.h + 8 * f - 1) // (8 * f)
        grids = [(rows * f, cols * f)] + [(rows, cols)] * 2 if scan.ncomp == 3 else [(rows, cols)]
        total = sum(gh * gw for gh, gw in grids)
        out = np.full((max(total, 1), 64), 0x5a5a, np.int16)
        res, large = GzScanResult(), C.c_int(-1)
        self.check(self.lib.gz_decode_scan_input(device, C.byref(scan), _ptr(out), C.byref(large), C.byref(res)))
        r = self._scan_result(res)
        if r["status"] != "DECODED":
            assert (out == 0x5a5a).all() and large.value == -1, "coefficients written without a verdict"
            return None, None, r
        comps, at = [], 0
        for gh, gw in grids:
            comps.append(out[at:at + gh * gw].reshape(gh, gw, 64))
            at += gh * gw
        return comps, bool(large.value), r

    def probe_emit_map(self, plane, dmap, device=0):
        """gz_probe_emit_map: the float32 [h][w] `plane` (any bit patterns) through the map's emit kernel alone, into
        `dmap` (device_map(...))."""
        p = np.ascontiguousarray(plane, np.float32)
        h, w = p.shape
        self.check(self.lib.gz_probe_emit_map(device, _ptr(p), w, h, C.byref(dmap)))

    def fuzzy_class(self, score):
        """gz_butteraugli_fuzzy_class: ButteraugliFuzzyClass."""
        return self.lib.gz_butteraugli_fuzzy_class(float(score))

    def fuzzy_inverse(self, seek):
        """gz_butteraugli_fuzzy_inverse: ButteraugliFuzzyInverse."""
        return self.lib.gz_butteraugli_fuzzy_inverse(float(seek))

    def default_heat_thresholds(self):
        """(good, bad) as the reference's tool draws its heat maps: (fuzzy_inverse(1.5), fuzzy_inverse(0.5))."""
        return self.fuzzy_inverse(1.5), self.fuzzy_inverse(0.5)

    def heatmap_from_map_device(self, ptr, w, h, pitch, good, bad, output, device=0):
        """gz_heatmap_from_map_device: the heat map of the float32 device plane at `ptr` (`pitch` floats per row) into
        `output` (device_output(...))."""
        self.check(self.lib.gz_heatmap_from_map_device(device, int(ptr) or None, w, h, pitch, good, bad, C.byref(output)))

    def probe_emit_heat(self, plane, good, bad, output, device=0):
        """gz_probe_emit_heat: the float32 [h][w] `plane` through the heat map's kernel alone, into `output`
        (device_output(...))."""
        p = np.ascontiguousarray(plane, np.float32)
        h, w = p.shape
        self.check(self.lib.gz_probe_emit_heat(device, _ptr(p), w, h, good, bad, C.byref(output)))

    def probe_heat_thresholds(self):
        """gz_probe_heat_thresholds: float64 [255], entry k - 1 the least v whose byte is >= k."""
        thr = np.zeros(255, np.float64)
        self.check(self.lib.gz_probe_heat_thresholds(_ptr(thr)))
        return thr


class Context:
    """One (image, GPU) context == one guetzli::ButteraugliComparator + OutputImage."""

    def __init__(self, library, rgb, target, device=0):
        self.L = library
        self.rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w, ch = self.rgb.shape
        assert ch == 3
        self._set_geometry(w, h)
        err = C.c_int(0)
        self.handle = library.lib.gz_create(device, self.w, self.h, _ptr(self.rgb),
                                            float(target), C.byref(err))
        if not self.handle:
            library.check(err.value or -3)

    @classmethod
    def from_device(cls, library, image, w, h, target, device=0):
        """gz_create_from_device / gz_create_from_device_pixels: the original is the device-resident `image`
        (device_image(...) / device_pixels(...)).  The pixels stay where they are: such a context has rgb = None (as
        one whose original set_rgb_device replaced)."""
        self = cls.__new__(cls)
        self.L = library
        self.rgb = None
        self._set_geometry(w, h)
        err = C.c_int(0)
        entry = library.lib.gz_create_from_device_pixels if isinstance(image, GzDevicePixels) else library.lib.gz_create_from_device
        self.handle = entry(device, w, h, C.byref(image), float(target), C.byref(err))
        if not self.handle:
            library.check(err.value or -3)
        return self

    @classmethod
    def from_device_linear(cls, library, image, w, h, scale=1.0, device=0):
        """gz_create_from_device_linear: the original is the linear float image `image`; such a context has rgb = None
        and no coefficients (encode_rgb and the searches raise GZ_E_STATE until set_rgb* gives it 8-bit pixels)."""
        self = cls.__new__(cls)
        self.L = library
        self.rgb = None
        self._set_geometry(w, h)
        err = C.c_int(0)
        self.handle = library.lib.gz_create_from_device_linear(device, w, h, C.byref(image), float(scale), C.byref(err))
        if not self.handle:
            library.check(err.value or -3)
        return self

    def _set_geometry(self, w, h):
        self.w, self.h = w, h
        self.bw, self.bh = (self.w + 7) // 8, (self.h + 7) // 8
        self.nb = self.bw * self.bh
        # the frame: 4:4:4 (coefficient arrays [3][nb][64]) until downsample() /
        # set_orig_coeffs_420() make it 4:2:0 (flat [nb + 2*nbc][64]: Y, Cb, Cr)
        self.cfac = 1
        self.cbw, self.cbh = (self.w + 15) // 16, (self.h + 15) // 16
        self.nbc = self.cbw * self.cbh

    def close(self):
        if getattr(self, "handle", None):
            self.L.lib.gz_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        self.L.check(rc, self.handle)

    def _coeff_buf(self, cfac=None):
        if (cfac or self.cfac) == 2:
            return np.zeros((self.nb + 2 * self.nbc, 64), np.int16)
        return np.zeros((3, self.nb, 64), np.int16)

    @property
    def nblk(self):
        return self.nb + 2 * self.nbc if self.cfac == 2 else 3 * self.nb

    def split420(self, coeffs):
        """(Y [nb][64], Cb [nbc][64], Cr [nbc][64]) views of a 4:2:0 coefficient array."""
        co = np.asarray(coeffs).reshape(-1, 64)
        return co[:self.nb], co[self.nb:self.nb + self.nbc], co[self.nb + self.nbc:]

    def frame_layout(self):
        f, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.lib.gz_frame_layout(self.handle, C.byref(f), C.byref(a), C.byref(b)))
        return f.value, a.value, b.value

    def set_rgb(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape == (self.h, self.w, 3)
        self.rgb = rgb
        self._chk(self.L.lib.gz_set_rgb(self.handle, _ptr(rgb)))

    def set_rgb_device(self, image):
        """gz_set_rgb_device / gz_set_rgb_device_pixels: the original replaced by the device-resident `image`
        (device_image(...) / device_pixels(...), w x h)."""
        self.rgb = None
        entry = self.L.lib.gz_set_rgb_device_pixels if isinstance(image, GzDevicePixels) else self.L.lib.gz_set_rgb_device
        self._chk(entry(self.handle, C.byref(image)))

    def set_linear_device(self, image, scale=1.0):
        """gz_set_linear_device: the original replaced by the linear float image `image` (device_pixels(...), w x h)."""
        self.rgb = None
        self._chk(self.L.lib.gz_set_linear_device(self.handle, C.byref(image), float(scale)))

    def reconstruct_device(self, output):
        """gz_reconstruct_device: the candidate's pixels (gz_reconstruct's srgb) written into `output`
        (device_output(...), w x h)."""
        self._chk(self.L.lib.gz_reconstruct_device(self.handle, C.byref(output)))

    def synchronize(self):
        self._chk(self.L.lib.gz_synchronize(self.handle))

    def get_config(self):
        cfg = GzConfig()
        self._chk(self.L.lib.gz_get_config(self.handle, C.byref(cfg)))
        return cfg

    def set_config(self, **fields):
        """Replaces fields of the context's gz_config (blur_packed, tile_rows, single_stream, ...)."""
        cfg = self.get_config()
        for k, v in fields.items():
            assert k in dict(GzConfig._fields_), k
            setattr(cfg, k, v)
        self._chk(self.L.lib.gz_set_config(self.handle, C.byref(cfg)))
        return cfg

    def set_stream(self, stream_ptr):
        self._chk(self.L.lib.gz_set_stream(self.handle, stream_ptr))

    def encode_rgb(self, download=True):
        self.cfac = 1
        out = self._coeff_buf() if download else None
        self._chk(self.L.lib.gz_encode_rgb(self.handle, _ptr(out)))
        return out

    def set_orig_coeffs(self, coeffs):
        co = np.ascontiguousarray(coeffs, np.int16)
        assert co.size == 3 * self.nb * 64
        self._chk(self.L.lib.gz_set_orig_coeffs(self.handle, _ptr(co)))
        self.cfac = 1   # (only once the library has switched its frame)

    def set_orig_coeffs_420(self, coeffs):
        co = np.ascontiguousarray(coeffs, np.int16)
        assert co.size == (self.nb + 2 * self.nbc) * 64
        self._chk(self.L.lib.gz_set_orig_coeffs_420(self.handle, _ptr(co)))
        self.cfac = 2

    def downsample(self, download=True):
        """OutputImage::Downsample on the original: the frame becomes 4:2:0."""
        out = self._coeff_buf(2) if download else None
        self._chk(self.L.lib.gz_downsample(self.handle, _ptr(out)))
        self.cfac = 2   # (a failed call leaves the 4:4:4 layout in place on both sides)
        return out

    def downsample_planes(self, y, u, v, download=True):
        """The silver-screen branch of OutputImage::Downsample, given RGBToYUV420's planes."""
        pl = [np.ascontiguousarray(p, np.float32) for p in (y, u, v)]
        assert all(p.size == self.w * self.h for p in pl)
        out = self._coeff_buf(2) if download else None
        self._chk(self.L.lib.gz_downsample_planes(self.handle, _ptr(pl[0]), _ptr(pl[1]), _ptr(pl[2]), _ptr(out)))
        self.cfac = 2
        return out

    def downsample_silver(self, download=True):
        """The whole use_silver_screen branch of OutputImage::Downsample on the device -> (coefficients of the 4:2:0
        frame, (cell-passes evaluated, cell-passes redone on the host))."""
        out = self._coeff_buf(2) if download else None
        cnt = np.zeros(2, np.uint64)
        self._chk(self.L.lib.gz_downsample_silver(self.handle, _ptr(out), _ptr(cnt)))
        self.cfac = 2
        return out, (int(cnt[0]), int(cnt[1]))

    def quantize(self, q=None, download=True):
        qq = None if q is None else np.ascontiguousarray(q, np.int32)
        out = self._coeff_buf() if download else None
        self._chk(self.L.lib.gz_quantize(self.handle, _ptr(qq), _ptr(out)))
        return out

    def set_coeffs(self, coeffs):
        co = np.ascontiguousarray(coeffs, np.int16)
        assert co.size == self.nblk * 64
        self._chk(self.L.lib.gz_set_coeffs(self.handle, _ptr(co)))

    def set_coeff_blocks(self, block_index, blocks):
        bi = np.ascontiguousarray(block_index, np.int32)
        bl = np.ascontiguousarray(blocks, np.int16)
        assert bl.size == bi.size * 192
        self._chk(self.L.lib.gz_set_coeff_blocks(self.handle, _ptr(bi), bi.size, _ptr(bl)))

    def get_coeffs(self):
        out = self._coeff_buf()
        self._chk(self.L.lib.gz_get_coeffs(self.handle, _ptr(out)))
        return out

    def reconstruct(self):
        srgb = np.zeros((self.h, self.w, 3), np.uint8)
        lin = np.zeros((3, self.h, self.w), np.float32)
        self._chk(self.L.lib.gz_reconstruct(self.handle, _ptr(srgb), _ptr(lin)))
        return srgb, lin

    def compare(self, want_distmap=True, want_block_max=True):
        dist = np.zeros(1, np.float32)
        dm = np.zeros((self.h, self.w), np.float32) if want_distmap else None
        bm = np.zeros(self.nb, np.float32) if want_block_max else None
        self._chk(self.L.lib.gz_compare(self.handle, _ptr(dist), _ptr(dm), _ptr(bm)))
        return float(dist[0]), dm, bm

    def compare_device_pixels(self, other, dmap=None):
        """gz_compare_device_pixels: the distance of the device-resident image `other` (device_pixels(...), w x h) from
        the context's original, which is the reference; dmap (device_map(...)): where the distance map goes."""
        dist = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_compare_device_pixels(self.handle, C.byref(other), _ptr(dist),
                                                      None if dmap is None else C.byref(dmap)))
        return float(dist[0])

    def compare_device_pixels_heat(self, other, heat, good, bad, dmap=None):
        """gz_compare_device_pixels_heat: compare_device_pixels, and the comparison's heat map into `heat`
        (device_output(...)) under the thresholds good and bad."""
        dist = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_compare_device_pixels_heat(self.handle, C.byref(other), _ptr(dist), None if dmap is None else C.byref(dmap),
                                                           C.byref(heat), good, bad))
        return float(dist[0])

    def compare_device_linear(self, other, scale=1.0, dmap=None, heat=None, good=0.0, bad=0.0):
        """gz_compare_device_linear: compare_device_pixels for a LINEAR float image `other` (device_pixels(...) of
        float32 / float16 / bfloat16, raw intensity 0..255 after `scale`) -> (distance, elements the clamp altered);
        dmap (device_map(...)) and heat (device_output(...), under the thresholds good and bad) as there."""
        dist = np.zeros(1, np.float32)
        clamped = C.c_uint64(0)
        self._chk(self.L.lib.gz_compare_device_linear(self.handle, C.byref(other), float(scale), _ptr(dist),
                                                      None if dmap is None else C.byref(dmap), None if heat is None else C.byref(heat),
                                                      good, bad, C.byref(clamped)))
        return float(dist[0]), clamped.value

    def compare_rgb(self, rgb, want_distmap=True):
        """gz_compare_rgb: the same for host bytes uint8 [h][w][3] -> (distance, float32 [h][w] map or None)."""
        px = np.ascontiguousarray(rgb, np.uint8)
        assert px.shape == (self.h, self.w, 3)
        dist = np.zeros(1, np.float32)
        dm = np.zeros((self.h, self.w), np.float32) if want_distmap else None
        self._chk(self.L.lib.gz_compare_rgb(self.handle, _ptr(px), _ptr(dist), _ptr(dm)))
        return float(dist[0]), dm

    def distmap_device(self, dmap):
        """gz_distmap_device: the distance map of the last comparison that stored one, into dmap (device_map(...))."""
        self._chk(self.L.lib.gz_distmap_device(self.handle, C.byref(dmap)))

    def heatmap_device(self, good, bad, output):
        """gz_heatmap_device: the heat map of that distance map into `output` (device_output(...))."""
        self._chk(self.L.lib.gz_heatmap_device(self.handle, good, bad, C.byref(output)))

    def compare_begin(self):
        self._chk(self.L.lib.gz_compare_begin(self.handle))

    def compare_end(self):
        d = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_compare_end(self.handle, _ptr(d)))
        return float(d[0])

    def compare_enqueue(self, iters):
        self._chk(self.L.lib.gz_compare_enqueue(self.handle, iters))

    def last_distance(self):
        d = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_last_distance(self.handle, _ptr(d)))
        return float(d[0])

    def time_compare(self, iters):
        ms = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_time_compare(self.handle, iters, _ptr(ms)))
        return float(ms[0])

    def block_weights(self, direction, max_block_dist, target_mul, use_distmap=True,
                      weights=None):
        wgt = np.zeros(self.nb, np.float32) if weights is None else \
            np.ascontiguousarray(weights, np.float32).copy()
        self._chk(self.L.lib.gz_block_weights(self.handle, direction, max_block_dist,
                                              target_mul, int(use_distmap), _ptr(wgt)))
        return wgt

    def block_weights_factor(self, direction, max_block_dist, target_mul, factor,
                             use_distmap=True, weights=None):
        n = self.nbc if factor == 2 else self.nb
        wgt = np.zeros(n, np.float32) if weights is None else \
            np.ascontiguousarray(weights, np.float32).copy()
        self._chk(self.L.lib.gz_block_weights_factor(self.handle, direction, max_block_dist,
                                                     target_mul, int(use_distmap), factor, _ptr(wgt)))
        return wgt

    def block_zeroing_orders(self, lookahead=3, new_model=True, comp_mask=7):
        gn = self.nbc if (self.cfac == 2 and comp_mask == 6) else self.nb
        self.search_blocks = gn
        cap = gn * 189
        off = np.zeros(gn + 1, np.int32)
        idx = np.zeros(cap, np.uint8)
        err = np.zeros(cap, np.float32)
        self._chk(self.L.lib.gz_block_zeroing_orders_masked(self.handle, comp_mask, lookahead,
                                                            int(new_model), _ptr(off), _ptr(idx),
                                                            _ptr(err), cap))
        n = int(off[-1])
        return off, idx[:n].copy(), err[:n].copy()

    def search_evaluations(self):
        n = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_search_evaluations(self.handle, _ptr(n)))
        return int(n[0])

    def compare_blocks(self, block_xy, coeffs):
        """SwitchBlock + CompareBlock for n (block position, 3x64 coefficients) pairs."""
        xy = np.ascontiguousarray(block_xy, np.int32).reshape(-1, 2)
        co = np.ascontiguousarray(coeffs, np.int16).reshape(-1, 3, 64)
        assert len(xy) == len(co)
        out = np.zeros(len(xy), np.float64)
        self._chk(self.L.lib.gz_compare_blocks(self.handle, len(xy), _ptr(xy), _ptr(co), _ptr(out)))
        return out

    def compare_block_pixels(self, block_xy, ycc):
        """SwitchBlock + CompareBlock for n 8x8 windows given by their YCbCr pixels (n x 3 x 64 u8)."""
        xy = np.ascontiguousarray(block_xy, np.int32).reshape(-1, 2)
        px = np.ascontiguousarray(ycc, np.uint8).reshape(-1, 3, 64)
        assert len(xy) == len(px)
        out = np.zeros(len(xy), np.float64)
        self._chk(self.L.lib.gz_compare_block_pixels(self.handle, len(xy), _ptr(xy), _ptr(px), _ptr(out)))
        return out

    def set_frame(self, chroma_factor):
        self._chk(self.L.lib.gz_set_frame(self.handle, int(chroma_factor)))
        self.cfac = int(chroma_factor)

    # ---- global candidate order of phase B ----
    ORDER_DTYPE = np.dtype([("block", np.int32), ("val", np.float32)])

    def order_build(self, direction, next_cand, max_block_error, block_weight, limit=None):
        nc = np.ascontiguousarray(next_cand, np.int32)
        me = np.ascontiguousarray(max_block_error, np.float32)
        bw = np.ascontiguousarray(block_weight, np.float32)
        assert nc.size == me.size == bw.size == getattr(self, "search_blocks", self.nb)
        total, below = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        btc = np.zeros(1, np.int32)
        self._chk(self.L.lib.gz_order_build(self.handle, direction, _ptr(nc), _ptr(me), _ptr(bw),
                                            int(limit is not None), float(limit or 0.0),
                                            _ptr(total), _ptr(btc), _ptr(below)))
        return int(total[0]), int(btc[0]), int(below[0])

    def order_reset(self):
        self._chk(self.L.lib.gz_order_reset(self.handle))

    def order_build_auto(self, direction, max_block_dist, target_mul, use_distmap, next_cand,
                         limit=None):
        nc = np.ascontiguousarray(next_cand, np.int32)
        assert nc.size == getattr(self, "search_blocks", self.nb)
        total, below = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        btc = np.zeros(1, np.int32)
        self._chk(self.L.lib.gz_order_build_auto(self.handle, direction, max_block_dist,
                                                 target_mul, int(use_distmap), _ptr(nc),
                                                 int(limit is not None), float(limit or 0.0),
                                                 _ptr(total), _ptr(btc), _ptr(below)))
        return int(total[0]), int(btc[0]), int(below[0])

    def order_build_auto_begin(self, direction, max_block_dist, target_mul, use_distmap, next_cand,
                               limit=None):
        nc = np.ascontiguousarray(next_cand, np.int32)
        assert nc.size == getattr(self, "search_blocks", self.nb)
        self._chk(self.L.lib.gz_order_build_auto_begin(self.handle, direction, max_block_dist, target_mul,
                                                       int(use_distmap), _ptr(nc), int(limit is not None),
                                                       float(limit or 0.0)))

    def order_build_auto_end(self):
        """(total, blocks_to_change, below)."""
        total, below = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        btc = np.zeros(1, np.int32)
        self._chk(self.L.lib.gz_order_build_auto_end(self.handle, _ptr(total), _ptr(btc), _ptr(below)))
        return int(total[0]), int(btc[0]), int(below[0])

    def order_build_auto_descend_begin(self, direction, max_block_dist, target_mul, use_distmap, next_cand,
                                       per_block, threshold, max_levels, limit=None):
        nc = np.ascontiguousarray(next_cand, np.int32)
        assert nc.size == getattr(self, "search_blocks", self.nb)
        self._chk(self.L.lib.gz_order_build_auto_descend_begin(self.handle, direction, max_block_dist, target_mul,
                                                               int(use_distmap), _ptr(nc), int(limit is not None),
                                                               float(limit or 0.0), float(per_block), int(threshold),
                                                               int(max_levels)))

    def order_descend(self, last, threshold, max_levels):
        """The cut log [levels][3] = (lo, hi, cut) of the partitions made."""
        log = np.zeros((max(max_levels, 1), 3), np.uint64)
        levels = np.zeros(1, np.int32)
        self._chk(self.L.lib.gz_order_descend(self.handle, int(last), int(threshold), int(max_levels), _ptr(log),
                                              _ptr(levels)))
        return log[:int(levels[0])].copy()

    def order_descend_begin(self, per_block, threshold, max_levels):
        self._chk(self.L.lib.gz_order_descend_begin(self.handle, float(per_block), int(threshold), int(max_levels)))

    def order_descend_end(self, cap_levels=12):
        """(cut log [levels][3], last): the position the device derived and descended to."""
        log = np.zeros((max(cap_levels, 1), 3), np.uint64)
        levels = np.zeros(1, np.int32)
        last = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_order_descend_end(self.handle, _ptr(log), int(cap_levels), _ptr(levels), _ptr(last)))
        return log[:int(levels[0])].copy(), int(last[0])

    def order_exported(self):
        n = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_order_exported(self.handle, _ptr(n)))
        return int(n[0])

    def order_host_mirror(self, entries):
        """The context's page-locked copy of the order, grown to `entries`: a view that lives as long as the context
        does and no later order_host_mirror asks for more."""
        p = C.c_void_p()
        self._chk(self.L.lib.gz_order_host_mirror(self.handle, int(entries), C.byref(p)))
        if not p.value or entries == 0:
            return np.zeros(0, self.ORDER_DTYPE)
        buf = (C.c_char * (self.ORDER_DTYPE.itemsize * int(entries))).from_address(p.value)
        return np.frombuffer(buf, self.ORDER_DTYPE)

    def order_advance(self, val_threshold, direction):
        self._chk(self.L.lib.gz_order_advance(self.handle, float(val_threshold), direction))

    def apply_coeff_edits(self, pos, val):
        p = np.ascontiguousarray(pos, np.int32)
        v = np.ascontiguousarray(val, np.int16)
        assert p.size == v.size
        self._chk(self.L.lib.gz_apply_coeff_edits(self.handle, _ptr(p), _ptr(v), p.size))

    def apply_candidate_steps(self, direction, blocks, counts):
        b = np.ascontiguousarray(blocks, np.int32)
        n = np.ascontiguousarray(counts, np.int32)
        assert b.size == n.size
        self._chk(self.L.lib.gz_apply_candidate_steps(self.handle, direction, _ptr(b), _ptr(n),
                                                      b.size))

    def steps_histogram_delta(self):
        """AC statistics change of the last apply_candidate_steps, int64 [3][256]."""
        d = np.zeros((3, 256), np.int32)
        self._chk(self.L.lib.gz_steps_histogram_delta(self.handle, _ptr(d)))
        return d.astype(np.int64)

    def order_upload(self, entries):
        e = np.ascontiguousarray(entries, self.ORDER_DTYPE)
        self._chk(self.L.lib.gz_order_upload(self.handle, _ptr(e), e.size))

    def order_partition(self, lo, hi):
        cut = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_order_partition(self.handle, lo, hi, _ptr(cut)))
        return int(cut[0])

    def order_fetch(self, lo, hi, out=None):
        """Entries [lo, hi) into `out` (a view of order_host_mirror's array lands without a second copy)."""
        if out is None:
            out = np.zeros(hi - lo, self.ORDER_DTYPE)
        assert out.dtype == self.ORDER_DTYPE and out.size >= hi - lo
        self._chk(self.L.lib.gz_order_fetch(self.handle, lo, hi, _ptr(out)))
        return out

    # ---- entropy coding of the candidate ----
    def jpeg_histograms(self, q, ncomp=3):
        """(DC, AC) x component x symbol occurrence counts, uint32 [2][3][256]."""
        qq = np.ascontiguousarray(q, np.int32)
        assert qq.shape == (3, 64)
        counts = np.zeros((2, 3, 256), np.uint32)
        self._chk(self.L.lib.gz_jpeg_histograms_ncomp(self.handle, _ptr(qq), ncomp, _ptr(counts)))
        return counts

    def jpeg_scan(self, ncomp, depth, code):
        """Encodes the scan on the device; returns its exact (stuffed) size in bytes."""
        d = np.ascontiguousarray(depth, np.uint8)
        cd = np.ascontiguousarray(code, np.uint16)
        assert d.shape == (2, 3, 256) and cd.shape == (2, 3, 256)
        n = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_jpeg_scan(self.handle, ncomp, _ptr(d), _ptr(cd), _ptr(n)))
        return int(n[0])

    def jpeg_scan_begin(self, ncomp, depth, code):
        """jpeg_scan in two halves: enqueue (entropy stream) ..."""
        d = np.ascontiguousarray(depth, np.uint8)
        cd = np.ascontiguousarray(code, np.uint16)
        assert d.shape == (2, 3, 256) and cd.shape == (2, 3, 256)
        self._chk(self.L.lib.gz_jpeg_scan_begin(self.handle, ncomp, _ptr(d), _ptr(cd)))

    def jpeg_scan_end(self):
        """... and collect: the scan's exact (stuffed) size in bytes."""
        n = np.zeros(1, np.uint64)
        self._chk(self.L.lib.gz_jpeg_scan_end(self.handle, _ptr(n)))
        return int(n[0])

    def jpeg_scan_bits(self):
        """(bits, stuffed bytes) of the last scan: scan bytes = ceil(bits / 8) + stuffed."""
        b = np.zeros(2, np.uint64)
        self._chk(self.L.lib.gz_jpeg_scan_bits(self.handle, _ptr(b[:1]), _ptr(b[1:])))
        return int(b[0]), int(b[1])

    def jpeg_scan_keep(self):
        self._chk(self.L.lib.gz_jpeg_scan_keep(self.handle))

    def jpeg_scan_bytes(self, kept=False, cap=None):
        cap = cap or (self.nb * 3 * 64 * 4 + 1024)
        out = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._chk(self.L.lib.gz_jpeg_scan_bytes(self.handle, int(kept), _ptr(out), cap,
                                                C.byref(n)))
        return out[:n.value].tobytes()

    # ---- stage probes ----
    def probe_blur(self, plane, sigma, border_ratio):
        p = np.ascontiguousarray(plane, np.float32)
        assert p.shape == (self.h, self.w)
        out = np.zeros_like(p)
        self._chk(self.L.lib.gz_probe_blur(self.handle, _ptr(p), sigma, border_ratio, _ptr(out)))
        return out

    def probe_opsin(self, rgb3):
        p = np.ascontiguousarray(rgb3, np.float32)
        assert p.shape == (3, self.h, self.w)
        out = np.zeros_like(p)
        self._chk(self.L.lib.gz_probe_opsin(self.handle, _ptr(p), _ptr(out)))
        return out

    def probe_separate_frequencies(self, xyb3):
        p = np.ascontiguousarray(xyb3, np.float32)
        out = np.zeros((10, self.h, self.w), np.float32)
        self._chk(self.L.lib.gz_probe_separate_frequencies(self.handle, _ptr(p), _ptr(out)))
        return out

    def probe_diffmap(self, rgb0, rgb1):
        """The distance map and score of two linear images.  rgb0 MUST be the linear image of the
        context's current original (gz_create's, or the last set_rgb's): the mask branch reads the
        half precomputed from that original, and with another rgb0 the map is silently wrong.  Call
        set_rgb(original) first to probe another pair."""
        a = np.ascontiguousarray(rgb0, np.float32)
        b = np.ascontiguousarray(rgb1, np.float32)
        d = np.zeros((self.h, self.w), np.float32)
        s = np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_probe_diffmap(self.handle, _ptr(a), _ptr(b), _ptr(d), _ptr(s)))
        return d, float(s[0])

    def probe_linear_planes(self):
        """gz_probe_linear_planes: the context's linear planes as they are now -> float32 [3][h][w]."""
        out = np.zeros((3, self.h, self.w), np.float32)
        self._chk(self.L.lib.gz_probe_linear_planes(self.handle, _ptr(out)))
        return out

    def probe_mask(self, xyb0, xyb1):
        a = np.ascontiguousarray(xyb0, np.float32)
        b = np.ascontiguousarray(xyb1, np.float32)
        m = np.zeros((3, self.h, self.w), np.float32)
        mdc = np.zeros((3, self.h, self.w), np.float32)
        self._chk(self.L.lib.gz_probe_mask(self.handle, _ptr(a), _ptr(b), _ptr(m), _ptr(mdc)))
        return m, mdc

    # ---- phase B on chosen state (tests/order_domain.py) ----
    def probe_set_block_max(self, block_max):
        bm = np.ascontiguousarray(block_max, np.float32)
        assert bm.size == self.nb
        self._chk(self.L.lib.gz_probe_set_block_max(self.handle, _ptr(bm)))

    def probe_set_search(self, offsets, idx, err, comp_mask=7):
        """Candidates (CSR, as block_zeroing_orders returns them) in the place of a block search's."""
        off = np.ascontiguousarray(offsets, np.int32)
        ix = np.ascontiguousarray(idx, np.uint8)
        er = np.ascontiguousarray(err, np.float32)
        gn = self.nbc if (self.cfac == 2 and comp_mask == 6) else self.nb
        assert off.size == gn + 1 and ix.size == er.size == int(off[-1])
        ix = ix if ix.size else np.zeros(1, np.uint8)
        er = er if er.size else np.zeros(1, np.float32)
        self._chk(self.L.lib.gz_probe_set_search(self.handle, comp_mask, _ptr(off), _ptr(ix), _ptr(er)))
        self.search_blocks = gn

    def probe_order_state(self):
        """(block weights, max_block_error) of the device, a pending order_advance made first."""
        gn = getattr(self, "search_blocks", self.nb)
        wgt, me = np.zeros(gn, np.float32), np.zeros(gn, np.float32)
        self._chk(self.L.lib.gz_probe_order_state(self.handle, _ptr(wgt), _ptr(me)))
        return wgt, me


_default = None


def load():
    """The product library (gfx950).  Raises if it is missing."""
    global _default
    if _default is None:
        # GUETZLI_AMD_LIB: another build of the same library (kernel A/B runs of tools/)
        _default = Library(os.environ.get("GUETZLI_AMD_LIB", DEFAULT_LIB))
    return _default

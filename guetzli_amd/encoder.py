"""Python binding of the host search driver (guetzli_amd/host, libguetzli_amd_host.so):
guetzli_amd.process(rgb, quality=95) == guetzli::Process(params, stats, rgb, w, h, &out)
with the numeric hot path on the MI355X.  No CPU fallback: the host library links the
gfx950 C-ABI library and fails if no GPU is usable."""
import ctypes as C
import operator
import os

import numpy as np

import time

from . import device_arrays as da
from .device_arrays import is_device_resident   # (its home; importable and patchable here, as ever)
from .capi import GZ_DT_BF16, GZ_DT_F16, GZ_DT_F32, GZ_DT_U8, GZ_DT_U16, GZ_SAMPLES_LINEAR, GZ_SAMPLES_SRGB8, GzDevicePixels, device_batch, device_map, device_map_batch, device_output, device_output_batch, device_pixels

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_HOST_LIB = os.path.join(HERE, "libguetzli_amd_host.so")


def _jpeg_dimensions(data):
    """(width, height) of the first SOFn segment of a JPEG stream, (0, 0) if there is none."""
    i, n = 2, len(data)
    while i + 9 < n:
        if data[i] != 0xFF:
            i += 1
            continue
        m = data[i + 1]
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7 or m == 0xFF:
            i += 2 if m != 0xFF else 1
            continue
        seg = (data[i + 2] << 8) | data[i + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return (data[i + 7] << 8) | data[i + 8], (data[i + 5] << 8) | data[i + 6]
        i += 2 + seg
    return 0, 0


class HostLibrary:
    def __init__(self, path=DEFAULT_HOST_LIB):
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: run `python -m guetzli_amd.build`")
        self.lib = C.CDLL(path)
        self.lib.gzh_process.restype = C.c_long
        self.lib.gzh_process.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float,
                                         C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long,
                                         C.c_void_p, C.c_long]
        self.lib.gzh_process_jpeg.restype = C.c_long
        self.lib.gzh_process_jpeg.argtypes = [C.c_void_p, C.c_long, C.c_double, C.c_float, C.c_int,
                                              C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        self.lib.gzh_process_params.restype = C.c_long
        self.lib.gzh_process_params.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_double,
                                                C.c_float, C.c_void_p, C.c_void_p, C.c_long,
                                                C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        self.lib.gzh_process_device.restype = C.c_long
        self.lib.gzh_process_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_void_p,
                                                C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        self.lib.gzh_process_device_pixels.restype = C.c_long
        self.lib.gzh_process_device_pixels.argtypes = self.lib.gzh_process_device.argtypes
        self.lib.gzh_write_jpeg_factor.restype = C.c_long
        self.lib.gzh_write_jpeg_factor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                   C.c_int, C.c_void_p, C.c_long]
        self.lib.gzh_jpeg_head_factor.restype = C.c_long
        self.lib.gzh_jpeg_head_factor.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
        self.lib.gzh_read_png.restype = C.c_long
        self.lib.gzh_read_png.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long]
        self.lib.gzh_write_jpeg.restype = C.c_long
        self.lib.gzh_write_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_long]
        self.lib.gzh_jpeg_head.restype = C.c_long
        self.lib.gzh_jpeg_head.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
        self.lib.gzh_jpeg_size.restype = C.c_long
        self.lib.gzh_jpeg_size.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
        self.lib.gzh_decode_jpeg_device.restype = C.c_long
        self.lib.gzh_decode_jpeg_device.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        self.lib.gzh_decode_jpeg_device_sized.restype = C.c_long
        self.lib.gzh_decode_jpeg_device_sized.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int]
        self.lib.gzh_decode_jpeg.restype = C.c_long
        self.lib.gzh_decode_jpeg.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long]
        for name, args in (("gzh_decode_jpeg_device_entropy", [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
                           ("gzh_decode_jpeg_coeffs", [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p,
                                                       C.c_void_p, C.c_long, C.c_void_p])):
            if hasattr(self.lib, name):   # (a host library built before the device's scan decoder has neither)
                getattr(self.lib, name).restype = C.c_long
                getattr(self.lib, name).argtypes = args
        for name, args in (("gzh_process_jpeg_entropy", [C.c_void_p, C.c_long, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]),
                           ("gzh_read_jpeg_entropy", [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long])):
            if hasattr(self.lib, name):   # (... and one built before JPEG input could come from it has neither of these)
                getattr(self.lib, name).restype = C.c_long
                getattr(self.lib, name).argtypes = args
        if hasattr(self.lib, "gzh_decode_jpeg_batch_device"):   # (... and one built before batches were decoded lacks this one)
            self.lib.gzh_decode_jpeg_batch_device.restype = C.c_long
            self.lib.gzh_decode_jpeg_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                              C.c_uint64, C.c_void_p, C.c_void_p]
        self.lib.gzh_butteraugli_score_for_quality.restype = C.c_double
        self.lib.gzh_butteraugli_score_for_quality.argtypes = [C.c_double]

    def _process(self, data, w, h, quality, target, device, clear_metadata, try_420, force_420,
                 use_silver_screen, lookahead, new_model, want_trace, entropy_mode=None):
        """gzh_process_params -- or, for a capi.GzDevicePixels / GzDeviceImage, gzh_process_device_pixels /
        gzh_process_device; for JPEG bytes with an entropy_mode (_entropy_mode), gzh_process_jpeg_entropy, and the
        info gets "input" -- with a buffer that grows to what the library asks for."""
        is_jpeg = isinstance(data, (bytes, bytearray))
        on_device = not is_jpeg and not isinstance(data, np.ndarray)
        buf = np.frombuffer(data, np.uint8) if is_jpeg else data
        if is_jpeg:
            # from the frame header's dimensions (a heavily compressed input re-encoded at a high
            # quality can be many times its own size; a second call would repeat the whole search)
            jw, jh = _jpeg_dimensions(data)
            if jw * jh > (1 << 28):   # a header nobody has validated yet (65535 x 65535 = 12.9 GB):
                jw = jh = 0           # start small, the grow-and-retry path covers a real giant
            cap = max(3 * jw * jh + (1 << 16), 4 * len(data), 1 << 20)
        else:
            cap = 3 * w * h + (1 << 16)
        ip = (C.c_int * 7)(device, int(clear_metadata), int(try_420), int(force_420),
                           int(use_silver_screen), int(lookahead), int(new_model))
        tr = C.create_string_buffer(1 << 24) if want_trace else None
        tm = C.create_string_buffer(1 << 12)
        einfo = (C.c_int64 * 6)()
        for _ in range(2):
            out = np.empty(cap, np.uint8)
            qt = (-1.0 if target is not None else float(quality), float(target or 0.0))
            if entropy_mode is not None:
                n = self.lib.gzh_process_jpeg_entropy(buf.ctypes.data if len(data) else None, len(data), *qt, ip, entropy_mode, einfo,
                                                      out.ctypes.data, cap, tr, len(tr) if tr else 0, tm, len(tm))
            elif on_device:
                entry = self.lib.gzh_process_device_pixels if isinstance(data, GzDevicePixels) else self.lib.gzh_process_device
                n = entry(C.addressof(data), w, h, *qt, ip, out.ctypes.data, cap, tr, len(tr) if tr else 0, tm, len(tm))
            else:
                n = self.lib.gzh_process_params(buf.ctypes.data, len(data) if is_jpeg else -1, w, h, *qt, ip,
                                                out.ctypes.data, cap, tr, len(tr) if tr else 0, tm, len(tm))
            if n < 0:
                raise RuntimeError("guetzli_amd.Process failed (see stderr)" if n == -1 else
                                   "guetzli_amd.Process raised a C++ exception (see stderr)")
            if n <= cap:
                break
            cap = n   # the JPEG did not fit (nothing was copied): once more with room for it
        else:
            raise RuntimeError(f"guetzli_amd.Process: output of {n} bytes does not fit")
        timers, counters = {}, {}
        for item in tm.value.decode().split(";"):
            if "=" in item:
                k, v = item.split("=")
                if k.startswith("#"):
                    counters[k[1:]] = int(v)
                else:
                    timers[k] = float(v)
        info = {"trace": tr.value.decode() if tr else None, "timers": timers, "counters": counters}
        if entropy_mode is not None:
            info["input"] = self._entropy_info(einfo)
        return out[:n].tobytes(), info

    def process(self, rgb, quality=95.0, target=None, device=0, want_trace=False, try_420=False,
                force_420=False, use_silver_screen=False, lookahead=3, new_model=True):
        """guetzli::Process(params, stats, rgb, w, h, &out).  Returns (jpeg_bytes, info) where
        info has 'trace' (the --verbose text, if requested), 'timers' (seconds per phase) and
        'counters'.  The keyword arguments are the fields of guetzli::Params."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w, ch = rgb.shape
        assert ch == 3
        return self._process(rgb, w, h, quality, target, device, True, try_420, force_420,
                             use_silver_screen, lookahead, new_model, want_trace)

    def process_device(self, ptr, w, h, dtype, strides, stream=0, quality=95.0, target=None, device=0,
                       want_trace=False, try_420=False, force_420=False, use_silver_screen=False, lookahead=3,
                       new_model=True, alpha_offset=None, background=None):
        """guetzli_amd::Process(params, stats, DeviceImage, w, h, &out): the raw form.  ptr = address, in the memory of
        GPU `device`, of element (0, 0, 0) of a w x h x 3 image; dtype = "uint8" | "float32" | "float16" | "bfloat16"
        | "uint16" (or a GZ_DT_* code); strides = (y, x, c) in elements, each >= 0; stream = the hipStream_t whose work
        produced the data (0: nothing to wait for).  Floats are [0, 1]: byte = rint(clamp(x * 255, 0, 255)); uint16:
        the high byte.  alpha_offset = where, in elements from ptr, the alpha sample of pixel (0, 0) sits (it moves
        with the y and x strides; None: opaque), background = the bytes (r, g, b) such pixels are blended over:
        (v * a + bg * (255 - a) + 128) // 255.  Returns what process() returns."""
        code = DTYPE_CODES.get(dtype, dtype)
        alpha = da.alpha_address(ptr, alpha_offset, ITEMSIZE[code])
        image = device_pixels(ptr, code, strides, stream, alpha, _background(background) or (0, 0, 0))
        return self._process(image, w, h, quality, target, device, True, try_420, force_420,
                             use_silver_screen, lookahead, new_model, want_trace)

    def jpeg_size(self, data):
        """(w, h) of a JPEG the reader accepts; raises if the stream is rejected."""
        buf = np.frombuffer(data, np.uint8)
        wh = (C.c_int * 2)()
        if self.lib.gzh_jpeg_size(buf.ctypes.data, len(data), wh) != 0:
            raise ValueError("not a readable JPEG (see stderr)")
        return wh[0], wh[1]

    def decode_jpeg(self, data, device=0):
        """guetzli::DecodeJpegToRGB computed on GPU `device`, the pixels brought back: uint8 [h][w][3].  Raises if the
        stream is refused (one component, or YCbCr 4:4:4 / 4:2:0, are decoded; message on stderr)."""
        buf = np.frombuffer(data, np.uint8)
        w, h = _jpeg_dimensions(data)   # (the frame header: the stream is read once, by the decode itself)
        if w * h > (1 << 28):
            w = h = 0
        out = np.zeros(max(3 * w * h, 1), np.uint8)
        for _ in range(2):
            n = self.lib.gzh_decode_jpeg(buf.ctypes.data if len(data) else None, len(data), device, out.ctypes.data, out.size)
            if n < 0:
                raise ValueError("guetzli_amd.DecodeJpegToRGB: not a JPEG this library decodes (see stderr)")
            if n <= out.size:
                break
            out = np.zeros(n, np.uint8)
        w, h = self.jpeg_size(data) if n != 3 * w * h else (w, h)
        return out[:n].reshape(h, w, 3)

    def decode_jpeg_device(self, data, ptr, dtype, strides, stream=0, device=0, size=None):
        """guetzli_amd::DecodeJpegToRGB(jpeg, device, DeviceOutput, ...): the raw form.  ptr = address, in the memory of
        GPU `device`, of element (0, 0, 0) of the w x h x 3 image the JPEG decodes to (jpeg_size); dtype as
        process_device's; strides = (y, x, c) in elements, no two elements at one address; stream = the hipStream_t
        that used the memory before and reads it afterwards (0: none, the call waits for the pixels).  size = (w, h):
        what the destination was made for -- a stream of another size is refused instead of written."""
        buf = np.frombuffer(data, np.uint8)
        image = device_output(ptr, DTYPE_CODES.get(dtype, dtype), strides, stream)
        w, h = size or (0, 0)
        n = self.lib.gzh_decode_jpeg_device_sized(buf.ctypes.data if len(data) else None, len(data), device, C.addressof(image), w, h)
        if n != 0:
            raise RuntimeError("guetzli_amd.DecodeJpegToRGB failed (see stderr)" if n == -1 else
                               "guetzli_amd.DecodeJpegToRGB raised a C++ exception (see stderr)")

    @staticmethod
    def _entropy_mode(entropy, subseq_bytes=0, max_sync_rounds=0):
        if entropy not in ("host", "device"):
            raise ValueError(f"entropy={entropy!r}: 'host' or 'device'")
        return (C.c_int * 3)(int(entropy == "device"), int(subseq_bytes), int(max_sync_rounds))

    @staticmethod
    def _entropy_info(info):
        from .capi import SCAN_STATUS
        return {"path": "device" if info[0] else "host", "status": None if info[1] < 0 else SCAN_STATUS.get(info[1], info[1]),
                "subsequences": int(info[2]), "sync_rounds": int(info[3]), "end_offset": int(info[4]), "rc": int(info[5])}

    def decode_jpeg_device_entropy(self, data, ptr, dtype, strides, stream=0, device=0, size=None, entropy="device",
                                   subseq_bytes=0, max_sync_rounds=0):
        """decode_jpeg_device with the entropy-coded scan read by `entropy`: "host", or "device" -- the device's Huffman
        decoder where the scan is eligible and it reaches a verdict, the host's reader otherwise.  Returns which path
        produced the coefficients and the gz_scan_result of the attempt, as a dict."""
        buf = np.frombuffer(data, np.uint8)
        image = device_output(ptr, DTYPE_CODES.get(dtype, dtype), strides, stream)
        w, h = size or (0, 0)
        info = (C.c_int64 * 6)()
        n = self.lib.gzh_decode_jpeg_device_entropy(buf.ctypes.data if len(data) else None, len(data), device, C.addressof(image), w, h,
                                                    self._entropy_mode(entropy, subseq_bytes, max_sync_rounds), info)
        if n != 0:
            raise RuntimeError("guetzli_amd.DecodeJpegToRGB failed (see stderr)" if n == -1 else
                               "guetzli_amd.DecodeJpegToRGB raised a C++ exception (see stderr)")
        return self._entropy_info(info)

    def decode_jpeg_batch_device(self, jpegs, ptr, dtype, strides, size, stream=0, device=0, entropy="device", subseq_bytes=0,
                                 max_sync_rounds=0, scratch_bytes=0):
        """guetzli_amd::DecodeJpegBatchToRGB: the raw form.  jpegs: N bytes objects of size = (w, h) pixels each; ptr = address,
        in the memory of GPU `device`, of element (0, 0, 0, 0) of the N x h x w x 3 tensor they decode into; strides = (n, y,
        x, c) in elements.  Returns the N entropy infos of decode_jpeg_device_entropy.  ValueError names the file that was
        refused."""
        n = len(jpegs)
        bufs = [np.frombuffer(bytes(j), np.uint8) for j in jpegs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (C.c_long * n)(*[b.size for b in bufs])
        out = device_output_batch(ptr, DTYPE_CODES.get(dtype, dtype), strides, n, stream)
        info, failed = (C.c_int64 * (6 * n))(), C.c_int(-1)
        w, h = size
        rc = self.lib.gzh_decode_jpeg_batch_device(ptrs, lens, n, device, C.addressof(out), w, h,
                                                   self._entropy_mode(entropy, subseq_bytes, max_sync_rounds), int(scratch_bytes), info,
                                                   C.byref(failed))
        if rc != 0:
            if rc == -1 and failed.value >= 0:
                raise ValueError(f"jpegs[{failed.value}] is not a JPEG this library decodes to {w} x {h} pixels (see stderr)")
            raise RuntimeError("guetzli_amd.DecodeJpegBatchToRGB failed (see stderr)" if rc == -1 else
                               "guetzli_amd.DecodeJpegBatchToRGB raised a C++ exception (see stderr)")
        return [self._entropy_info(info[6 * i:6 * i + 6]) for i in range(n)]

    def decode_jpeg_coeffs(self, data, entropy="host", device=0, subseq_bytes=0, max_sync_rounds=0):
        """The dequantised coefficients DecodeJpegToRGB hands to the device, by either entropy path: (int16 [blocks][64] in
        the frame layout, (w, h, chroma_factor), the entropy info of decode_jpeg_device_entropy, the reader's metadata
        as bytes), or None where the stream is refused."""
        buf = np.frombuffer(data, np.uint8)
        whf, info, mlen = (C.c_int * 3)(), (C.c_int64 * 6)(), C.c_long(0)
        mode = self._entropy_mode(entropy, subseq_bytes, max_sync_rounds)
        w, h = _jpeg_dimensions(data)
        cap = 0 if w * h > (1 << 28) else 3 * ((w + 7) // 8) * ((h + 7) // 8) * 64
        meta = np.zeros(len(data) + 64, np.uint8)
        for _ in range(2):
            out = np.zeros(max(cap, 1), np.int16)
            n = self.lib.gzh_decode_jpeg_coeffs(buf.ctypes.data if len(data) else None, len(data), device, mode, whf, out.ctypes.data,
                                                cap, info, meta.ctypes.data, meta.size, C.byref(mlen))
            if n < 0:
                return None
            if n <= cap:
                break
            cap = n
        return out[:n].reshape(-1, 64), (whf[0], whf[1], whf[2]), self._entropy_info(info), meta[:mlen.value].tobytes()

    def read_png(self, data):
        """ReadPNG of the reference's front end (guetzli.cc:47-152): PNG bytes -> uint8
        [h][w][3] with alpha blended on black.  Raises if the stream is rejected."""
        buf = np.frombuffer(data, np.uint8)
        wh = (C.c_int * 2)()
        n = self.lib.gzh_read_png(buf.ctypes.data, len(data), wh, None, 0)
        if n < 0:
            raise ValueError("not a readable PNG (see stderr)")
        out = np.zeros(n, np.uint8)
        n2 = self.lib.gzh_read_png(buf.ctypes.data, len(data), wh, out.ctypes.data, n)
        assert n2 == n
        return out.reshape(wh[1], wh[0], 3)

    def process_jpeg(self, data, quality=95.0, target=None, device=0, clear_metadata=True,
                     want_trace=False, try_420=False, force_420=False, use_silver_screen=False,
                     lookahead=3, new_model=True, entropy="host", subseq_bytes=0, max_sync_rounds=0):
        """guetzli::Process(params, stats, jpeg_data, &out) for a YUV 4:4:4 or 4:2:0 JPEG.
        Returns (jpeg_bytes, trace) or raises if the input is refused (message on stderr).  entropy="device": the
        input's scan is read by the device's Huffman decoder where it is eligible and the decoder reaches a verdict,
        by the host otherwise, silently -- the same bytes and trace either way (process_jpeg_info says which)."""
        if entropy == "host" and not subseq_bytes and not max_sync_rounds:   # (the call every encode made before there was a choice)
            jpg, info = self._process(bytes(data), 0, 0, quality, target, device, clear_metadata,
                                      try_420, force_420, use_silver_screen, lookahead, new_model,
                                      want_trace)
        else:
            jpg, info = self.process_jpeg_info(data, quality, target, device, clear_metadata, want_trace, try_420, force_420,
                                               use_silver_screen, lookahead, new_model, entropy, subseq_bytes, max_sync_rounds)
        return jpg, info["trace"]

    def process_jpeg_info(self, data, quality=95.0, target=None, device=0, clear_metadata=True,
                          want_trace=False, try_420=False, force_420=False, use_silver_screen=False,
                          lookahead=3, new_model=True, entropy="host", subseq_bytes=0, max_sync_rounds=0):
        """process_jpeg with the whole record: (jpeg_bytes, info) with process()'s 'trace', 'timers', 'counters' and
        'input', what the read of the input says of its entropy path: 'path' ("device" | "host"), 'status' (the
        gz_scan_result's of the attempt, None: none was made), 'subsequences', 'sync_rounds', 'end_offset', 'rc'."""
        mode = self._entropy_mode(entropy, subseq_bytes, max_sync_rounds)
        return self._process(bytes(data), 0, 0, quality, target, device, clear_metadata, try_420, force_420,
                             use_silver_screen, lookahead, new_model, want_trace, entropy_mode=mode)

    def read_jpeg_dump(self, data, entropy="host", device=0, subseq_bytes=0, max_sync_rounds=0):
        """The reader's result as an encode of JPEG input gets it, as the canonical dump of host/reader_dump.h:
        (bytes, or None where the stream is refused; the entropy info as process_jpeg_info's 'input').  Test hook."""
        buf = np.frombuffer(data, np.uint8)
        mode = self._entropy_mode(entropy, subseq_bytes, max_sync_rounds)
        info = (C.c_int64 * 6)()
        # room for four components on grids padded to the largest MCU (32 x 32 pixels) and the metadata: one read as a rule
        w, h = _jpeg_dimensions(data)
        cap = (0 if w * h > (1 << 28) else 8 * (w + 32) * (h + 32)) + 2 * len(data) + 4096
        for _ in range(2):
            out = np.empty(cap, np.uint8)
            n = self.lib.gzh_read_jpeg_entropy(buf.ctypes.data if len(data) else None, len(data), device, mode, info, out.ctypes.data, cap)
            if n < 0:
                return None, self._entropy_info(info)
            if n <= cap:
                break
            cap = n
        return out[:n].tobytes(), self._entropy_info(info)

    def write_jpeg(self, coeffs, w, h, q=None, factor=1):
        """WriteJpeg of dequantised coefficients (frame layout of include/guetzli_amd.h:
        [3][nb][64] for factor 1, nb + 2*nbc blocks for the 4:2:0 factor 2) with quant matrices
        q[3][64]; q=None writes the q=1 'original' frame of EncodeRGBToJpeg."""
        co = np.ascontiguousarray(coeffs, np.int16)
        qq = None if q is None else np.ascontiguousarray(q, np.int32)
        cap = 6 * w * h + (1 << 16)
        for _ in range(2):
            out = np.zeros(cap, np.uint8)
            n = self.lib.gzh_write_jpeg_factor(co.ctypes.data, w, h,
                                               qq.ctypes.data if qq is not None else None,
                                               int(q is None), factor, out.ctypes.data, cap)
            if n < 0:
                raise RuntimeError("WriteJpeg failed")
            if n <= cap:
                return out[:n].tobytes()
            cap = n
        raise RuntimeError("WriteJpeg: output does not fit")

    def jpeg_head(self, counts, w, h, q=None, ncomp=3, factor=1):
        """SOI..SOS bytes + per-component Huffman codes (depth, code: [2][3][256]) from the
        symbol counts of gz_jpeg_histograms; q=None is the q=1 'original' frame."""
        cnt = np.ascontiguousarray(counts, np.uint32)
        assert cnt.shape == (2, 3, 256)
        qq = None if q is None else np.ascontiguousarray(q, np.int32)
        head = np.zeros(1 << 16, np.uint8)
        depth = np.zeros((2, 3, 256), np.uint8)
        code = np.zeros((2, 3, 256), np.uint16)
        n = self.lib.gzh_jpeg_head_factor(cnt.ctypes.data, qq.ctypes.data if qq is not None else None,
                                          w, h, ncomp, factor, head.ctypes.data, head.size,
                                          depth.ctypes.data, code.ctypes.data)
        assert 0 <= n <= head.size, n
        return head[:n].tobytes(), depth, code

    def butteraugli_score_for_quality(self, q):
        return self.lib.gzh_butteraugli_score_for_quality(q)


_default = None


def load_host():
    global _default
    if _default is None:
        _default = HostLibrary()
    return _default


DTYPE_CODES = {"uint8": GZ_DT_U8, "float32": GZ_DT_F32, "float16": GZ_DT_F16, "bfloat16": GZ_DT_BF16, "uint16": GZ_DT_U16}
ITEMSIZE = {GZ_DT_U8: 1, GZ_DT_F32: 4, GZ_DT_F16: 2, GZ_DT_BF16: 2, GZ_DT_U16: 2}


def _background(background):
    """None, or the bytes (r, g, b) of background=: three ints 0..255, or one int for a grey background."""
    if background is None:
        return None
    try:
        if isinstance(background, (bool, str, bytes)):
            raise TypeError
        vals = [operator.index(background)] * 3 if not hasattr(background, "__len__") else [operator.index(v) for v in background]
    except TypeError:
        raise ValueError(f"background={background!r}: three ints 0..255, or one for a grey background") from None
    if len(vals) != 3 or any(isinstance(v, bool) or not 0 <= v <= 255 for v in vals):
        raise ValueError(f"background={background!r}: three ints 0..255, or one for a grey background")
    return tuple(vals)


def blend_on_background(pixels, background):
    """The PNG front end's blend (BlendOnBlack at background 0) of uint8 [h][w][2] grey + alpha or [h][w][4] RGBA ->
    uint8 [h][w][3]: (v * a + bg * (255 - a) + 128) // 255, an integer division."""
    px = np.asarray(pixels, np.uint8).astype(np.uint32)
    v, a = px[..., :-1], px[..., -1:]
    if v.shape[-1] == 1:
        v = np.repeat(v, 3, axis=-1)
    bg = np.array(background, np.uint32)
    return ((v * a + bg * (255 - a) + 128) // 255).astype(np.uint8)


PER_THREAD_STREAM = 2   # hipStreamPerThread: the default stream of whichever thread uses the handle


class _Job:
    """One encode whose thread-dependent part is done: run(**params) -> (jpeg_bytes, info) on any thread."""

    def __init__(self, run, producer=0, keep=None):
        self.run, self.producer, self.keep = run, producer, keep   # keep: the object that owns the device memory


def decode(jpeg, out=None, dtype="uint8", layout="HWC", device=None, stream=None, entropy="host"):
    """guetzli::DecodeJpegToRGB with the pixels left on the GPU: the image a JPEG decodes to under the encoder's own
    pixel model -- the integer IDCT and colour conversion every butteraugli distance of the search was computed on.
    One-component (grey) and YCbCr 4:4:4 / 4:2:0 streams are decoded, everything else is refused.
    Returns a torch tensor on GPU `device` (None: torch's current one), [h][w][3] ("HWC") or [3][h][w] ("CHW") of
    `dtype`: uint8 the bytes, uint16 byte * 257, float32 / float16 / bfloat16 byte / 255 -- what process() reads back
    as the same bytes.  It is allocated on the calling thread's current stream, and work enqueued on that stream
    afterwards sees the pixels: no synchronisation is needed.
    out=: a GPU tensor, or an object with __cuda_array_interface__, of the JPEG's size in `layout` is filled in place
    and returned; dtype and strides are its own, so a crop inside a larger tensor is written without touching what
    surrounds it.  stream= overrides the consumer stream (a hipStream_t handle; 0: none -- the call waits).
    device="host": numpy uint8 [h][w][3] instead, computed on GPU 0.
    entropy="device": the entropy-coded scan is read on the GPU too (a self-synchronising parallel Huffman decoder) where
    it is a baseline scan of all components without restart intervals, one component or 4:4:4 / 4:2:0 -- what this
    library, Pillow and libjpeg write by default; every other stream, and every scan that decoder reaches no verdict
    on, is read by the host as with entropy="host", silently: the same streams are accepted and the same pixels
    returned.  decode_info() tells which path ran."""
    return _decode(jpeg, out, dtype, layout, device, stream, entropy)[0]


def decode_info(jpeg, entropy="device", out=None, dtype="uint8", layout="HWC", device=None, stream=None, subseq_bytes=0,
                max_sync_rounds=0):
    """decode() of `jpeg` that says what it did: {"path": "device" | "host" (whose reader produced the coefficients),
    "status": the device decoder's verdict (gz_scan_result: "DECODED", "NOT_CONVERGED", ...; None: it was not asked),
    "subsequences", "sync_rounds", "end_offset", "rc": what the device call returned (0; a GZ_E_* code: it failed, and the host
    read the scan instead), "decoded": the pixels}.  subseq_bytes / max_sync_rounds: gz_scan's."""
    pixels, info = _decode(jpeg, out, dtype, layout, device, stream, entropy, subseq_bytes, max_sync_rounds)
    info["decoded"] = pixels
    return info


def _decode(jpeg, out, dtype, layout, device, stream, entropy, subseq_bytes=0, max_sync_rounds=0):
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy={entropy!r}: 'host' or 'device'")
    lib = load_host()
    none = {"path": "host", "status": None, "subsequences": 0, "sync_rounds": 0, "end_offset": 0, "rc": 0}
    if isinstance(device, str):
        if device != "host" or out is not None:
            raise ValueError("device='host' (without out=) or a GPU ordinal")
        if entropy == "device":
            raise ValueError("entropy='device' leaves the pixels on the GPU: device='host' goes with entropy='host'")
        return lib.decode_jpeg(jpeg, 0), none
    w, h = _jpeg_dimensions(jpeg)   # (the frame header alone: the stream is read once, by the decode, which checks the size)
    if w <= 0 or h <= 0:
        raise ValueError("not a JPEG: no frame header")
    shape = da.image_shape(w, h, layout)   # (layout=None is refused: only decoded= and heatmap= guess)
    if out is None:
        if device is None:
            import torch
            device = torch.cuda.current_device()
        out = da.new_tensor(shape, dtype, device)
    dst = da.image_destination(out, w, h, layout, da.DTYPES, device, "out=")
    consumer = da.stream_or(stream, dst.stream)
    if entropy == "host":   # (the call every decode made before there was a choice)
        lib.decode_jpeg_device(jpeg, dst.ptr, dst.dtype, dst.strides, stream=consumer, device=dst.ordinal, size=(w, h))
        return out, none
    return out, lib.decode_jpeg_device_entropy(jpeg, dst.ptr, dst.dtype, dst.strides, stream=consumer, device=dst.ordinal, size=(w, h),
                                               entropy=entropy, subseq_bytes=subseq_bytes, max_sync_rounds=max_sync_rounds)


def decode_batch(jpegs, out=None, dtype="uint8", layout="HWC", device=None, stream=None, entropy="device", scratch_bytes=0):
    """decode() of N JPEGs of ONE decoded size into one tensor on the GPU, [N,H,W,3] ("HWC") or [N,3,H,W] ("CHW"): image i
    is, bit for bit, decode(jpegs[i]).  entropy="device" (this function's default, and its reason to exist): the baseline
    scans of the whole batch are read on the GPU by ONE launch of every kernel of the device's Huffman decoder per sampling
    (grey, 4:4:4, 4:2:0) instead of one set of launches and host round trips per file -- a minibatch of thumbnails costs
    little more than one of them.  Files whose scan that decoder does not take (restart intervals, progressive, other
    samplings) or reaches no verdict on are read by the host into their image, silently: mixed batches are fine.
    entropy="host": every file by the host's reader.
    jpegs: a sequence of bytes-likes; ValueError where their frame headers differ in size (it names the sizes and the
    first odd index), or where a file is refused (it names the index).  out=: a 4-D GPU tensor, or an object with
    __cuda_array_interface__, of that shape under ANY non-negative strides without aliasing -- x[::2], crops -- and any
    dtype of decode(); it is filled without touching what surrounds it, and returned.  device, stream, the element
    conversions: decode()'s.  scratch_bytes= caps the device memory of the call's temporaries (default 2 GiB; about 200
    bytes per pixel at 4:4:4, 100 at 4:2:0, plus the streams): a batch that needs more runs in chunks, with the same
    results."""
    return _decode_batch(jpegs, out, dtype, layout, device, stream, entropy, scratch_bytes)[0]


def decode_batch_info(jpegs, out=None, dtype="uint8", layout="HWC", device=None, stream=None, entropy="device", scratch_bytes=0,
                      subseq_bytes=0, max_sync_rounds=0):
    """decode_batch() that says what it did -> (pixels, infos): infos[i] as decode_info()'s dict for jpegs[i], without
    "decoded"."""
    return _decode_batch(jpegs, out, dtype, layout, device, stream, entropy, scratch_bytes, subseq_bytes, max_sync_rounds)


def _decode_batch(jpegs, out, dtype, layout, device, stream, entropy, scratch_bytes, subseq_bytes=0, max_sync_rounds=0):
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy={entropy!r}: 'host' or 'device'")
    if isinstance(jpegs, (bytes, bytearray, memoryview)):
        raise TypeError("jpegs is a sequence of JPEGs, not one: decode() takes one")
    jpegs = [bytes(j) for j in jpegs]
    if not jpegs:
        raise ValueError("jpegs is an empty batch")
    sizes = [_jpeg_dimensions(j) for j in jpegs]   # (the frame headers alone: the decode checks the size each stream really has)
    w, h = sizes[0]
    if w <= 0 or h <= 0:
        raise ValueError("jpegs[0] is not a JPEG: no frame header")
    odd = next((i for i, s in enumerate(sizes) if s != sizes[0]), None)
    if odd is not None:
        raise ValueError(f"the JPEGs differ in size: jpegs[{odd}] holds {sizes[odd][0]} x {sizes[odd][1]} pixels, jpegs[0] {w} x {h}")
    n = len(jpegs)
    shape = (n,) + da.image_shape(w, h, layout)
    if out is None:
        if device is None:
            import torch
            device = torch.cuda.current_device()
        out = da.new_tensor(shape, dtype, device)
    dst = da.batch_destination(out, n, w, h, layout, da.DTYPES, device, "out=")
    infos = load_host().decode_jpeg_batch_device(jpegs, dst.ptr, dst.dtype, dst.strides, (w, h), stream=da.stream_or(stream, dst.stream),
                                                 device=dst.ordinal, entropy=entropy, subseq_bytes=subseq_bytes,
                                                 max_sync_rounds=max_sync_rounds, scratch_bytes=scratch_bytes)
    return out, infos


def _with_decoded(job, decoded, w, h, ordinal):
    """`job` followed by the decode of the bytes it returns -- every exit of the driver is covered by this one
    mechanism -- into decoded= (True: a fresh uint8 [h][w][3] tensor on the encode's device).  Allocation and consumer
    stream are taken here, in the CALLER's thread."""
    if decoded is True:
        decoded = da.new_tensor((h, w, 3), "uint8", ordinal)
    dst = da.image_destination(decoded, w, h, None, da.DTYPES, ordinal, "decoded=")

    def run(**kw):
        jpeg, info = job.run(**kw)
        t0 = time.perf_counter()
        load_host().decode_jpeg_device(jpeg, dst.ptr, dst.dtype, dst.strides, stream=dst.stream, device=dst.ordinal, size=(w, h))
        info.setdefault("timers", {})["decode_output"] = time.perf_counter() - t0
        info["decoded"] = decoded
        return jpeg, info
    return _Job(run, job.producer, (job.keep, decoded))


def _prepared(rgb, layout, device, stream, background=None, decoded=None):
    """What of an encode must happen in the CALLER's thread -- torch's current stream is a property of the thread."""
    if decoded is not None and decoded is not False:
        job = _prepared(rgb, layout, device, stream, background)
        if is_device_resident(rgb):
            src = da.read(rgb, device, "rgb")
            (w, h, _, _), ordinal = da.source(src, layout, _background(background)), src.ordinal
        else:
            (h, w), ordinal = np.shape(rgb)[:2], 0 if device is None else device
        return _with_decoded(job, decoded, w, h, ordinal)
    background = _background(background)
    if not is_device_resident(rgb):
        if layout not in (None, "HWC"):
            raise ValueError("host pixels are [h][w][3]")
        if stream is not None:
            raise ValueError("stream= goes with device-resident pixels")
        if background is not None:   # uint8 [h][w][2] / [h][w][4]: blended here, by the device path's rule
            px = np.asarray(rgb)
            if px.dtype == np.uint8 and px.ndim == 3 and px.shape[2] in (2, 4):
                rgb = blend_on_background(px, background)
        return _Job(lambda **kw: load_host().process(rgb, device=0 if device is None else device, **kw))
    src = da.read(rgb, device, "rgb")
    w, h, strides, alpha = da.source(src, layout, background)
    producer = da.stream_or(stream, src.stream)
    blend = {} if alpha is None else {"alpha_offset": alpha, "background": background}
    return _Job(lambda **kw: load_host().process_device(src.ptr, w, h, src.dtype, strides, stream=producer, device=src.ordinal, **blend, **kw),
                producer, rgb)


def process(rgb, quality=95.0, layout=None, device=None, stream=None, background=None, decoded=None, **kw):
    """guetzli::Process of an image -> (jpeg_bytes, info).  `rgb` on the host: anything numpy turns into uint8
    [h][w][3].  `rgb` on the GPU -- a torch tensor with is_cuda, or an object with __cuda_array_interface__ -- is
    encoded where it is: uint8, uint16 (the high byte counts, as a 16-bit PNG is read), or float32 / float16 /
    bfloat16 in [0, 1]; "HWC" or "CHW" (layout=None: whichever of the first / last dimension is 3 -- where neither
    is, whichever is 1, or with background= 1, 2 or 4), any strides >= 0, 2-D or one channel = grey; on the tensor's
    device (an explicit device= must agree), behind the work enqueued so far on the producer's stream: the calling
    thread's current torch stream on that device, the interface's `stream` entry, or stream= (a hipStream_t handle;
    0: nothing to wait for).
    background=(r, g, b), or one int for a grey one, each 0..255: pixels with alpha -- 2 channels (grey + alpha) or 4
    (RGBA, not premultiplied), the alpha of the colours' dtype and last -- are blended over it as the PNG front end
    blends over black, on bytes: (v * a + bg * (255 - a) + 128) // 255.  The raw samples of a PNG as a GPU tensor, with
    background=0, give the JPEG process_png gives.  Without background= such shapes are refused: nothing is blended
    silently.  With an opaque image it has no effect.  A uint8 host array [h][w][2] or [h][w][4] is blended by the same
    rule in numpy.
    decoded=True: info["decoded"] is the image the returned bytes decode to (decode() of them: a uint8 [h][w][3] torch
    tensor on the encode's GPU, ready for work on the calling thread's current stream); decoded=tensor fills that image
    instead ([h][w][3] or [3][h][w]; dtype and strides its own).  The time it takes is info["timers"]["decode_output"]."""
    return _prepared(rgb, layout, device, stream, background, decoded).run(quality=quality, **kw)


def process_many(batch, workers=4, layout=None, device=None, stream=None, background=None, decoded=None, **kw):
    """A batch of images with `workers` of them in flight on one GPU (batch.encode_concurrent): a 4-D tensor
    [N,C,H,W] / [N,H,W,C] or a list of images, each as process() takes them (background= included).  Returns
    [(jpeg_bytes, info)] in order.
    The encodes run on worker threads, but every image's producer stream is the one process() would have taken in
    the CALLING thread, here and now: a batch made under `with torch.cuda.stream(s)` is encoded behind s.  (A
    __cuda_array_interface__ stream of 2, the per-thread default stream, is refused: it names another stream there.)
    decoded=True: every info["decoded"] is that image's decoded output, as process() makes it; the tensors are allocated
    here, on the calling thread's current stream, which is also the stream that may use them afterwards."""
    from .batch import encode_concurrent
    if decoded is not None and decoded is not False and decoded is not True:
        raise ValueError("process_many(decoded=): True, or nothing -- one destination cannot take a batch")
    jobs = [_prepared(batch[i], layout, device, stream, background, decoded) for i in range(len(batch))]
    if any(j.producer == PER_THREAD_STREAM for j in jobs):
        raise ValueError("a per-thread default stream cannot be waited for from the worker threads: synchronise it and "
                         "say stream=0, or encode with process()")
    return encode_concurrent(jobs, lambda job: job.run(**kw), workers=workers)


def read_png(data):
    """PNG bytes -> uint8 [h][w][3], as the reference's front end reads them (alpha on black)."""
    return load_host().read_png(data)


def process_png(data, quality=95.0, **kw):
    """`guetzli --quality Q in.png out.jpg`: ReadPNG + Process.  Returns (jpeg_bytes, info)."""
    return load_host().process(load_host().read_png(data), quality=quality, **kw)


def process_jpeg(data, quality=95.0, entropy="host", **kw):
    """`guetzli --quality Q in.jpg out.jpg`: Process(params, stats, jpeg_data, &out) for a YUV 4:4:4 or 4:2:0 JPEG.
    Returns (jpeg_bytes, info); info["input"] says who read the input's scan.  entropy="device": the GPU's Huffman
    decoder reads it where the scan is eligible (baseline, one scan, no restart interval) and the decoder reaches a
    verdict; every other stream is read by the host as with entropy="host", silently -- the same streams are accepted
    and the same bytes written either way.  The keywords are HostLibrary.process_jpeg_info's."""
    return load_host().process_jpeg_info(data, quality=quality, entropy=entropy, **kw)


# ---- the butteraugli distance of two images (capi: gz_compare_device_pixels / gz_compare_rgb / gz_distmap_device) ----
MAP_DTYPES = LINEAR_DTYPES = da.FLOAT_DTYPES


def _pair_library():
    """The C-ABI library the image-pair metric runs on (the product's; there is no other)."""
    from .capi import load
    return load()


def _map_output(x, shape, device, stream, what="distmap="):
    """The device-resident `x` that is to receive float planes of `shape` -- [h][w], or [n][h][w] -> capi.GzDeviceMap /
    GzDeviceMapBatch with the consumer's stream (stream=, or the one `x` was made on)."""
    dst = da.destination(x, shape, MAP_DTYPES, device, what)
    describe = device_map if len(shape) == 2 else device_map_batch
    return describe(dst.ptr, DTYPE_CODES[dst.dtype], dst.strides, da.stream_or(stream, dst.stream))


def _image_output(x, w, h, layout, device, stream, what, dtypes=da.DTYPES):
    """The device-resident `x` that is to receive w x h x 3 samples in `layout` (None: [h][w][3], or [3][h][w] where its
    shape says so) -> capi.GzDeviceOutput with the consumer's stream."""
    dst = da.image_destination(x, w, h, layout, dtypes, device, what)
    return device_output(dst.ptr, DTYPE_CODES[dst.dtype], dst.strides, da.stream_or(stream, dst.stream))


def _heat_thresholds(good, bad):
    """ScoreToRgb's thresholds: the caller's, or the reference tool's fuzzy_inverse(1.5) and fuzzy_inverse(0.5)."""
    if good is None or bad is None:
        dgood, dbad = _pair_library().default_heat_thresholds()
        good, bad = dgood if good is None else good, dbad if bad is None else bad
    good, bad = float(good), float(bad)
    if not 0 < good < bad < float("inf"):
        raise ValueError(f"heat map thresholds good={good}, bad={bad}: 0 < good < bad, both finite")
    return good, bad


def _heat_source(x):
    """(ptr, w, h, pitch in floats, device ordinal, what keeps the memory alive) of a float32 2-D distance map on a GPU."""
    src = da.read(x, None, "the distance map", dtypes=None)
    if src.dtype != "float32" or len(src.shape) != 2:
        raise TypeError(f"a distance map is a 2-D float32 image, not {src.shape} of {src.dtype}")
    (h, w), (sy, sx) = src.shape, src.strides
    if (w > 1 and sx != 1) or (h > 1 and sy < w):
        if not hasattr(x, "contiguous"):   # (a torch tensor is copied; what an interface object offers for that is not known)
            raise ValueError(f"a distance map with byte strides {(4 * sy, 4 * sx)}: make it contiguous in x first")
        return _heat_source(x.contiguous())
    return src.ptr, w, h, max(sy, w), src.ordinal, src.owner


class _PairImage:
    """One image of a pair, looked at but not touched: host bytes (rgb) or the description of device-resident pixels
    (pixels, a capi.GzDevicePixels; keep: the object that owns the memory)."""

    def __init__(self, w, h, rgb=None, pixels=None, ordinal=None, keep=None, linear=False, scale=1.0):
        self.w, self.h, self.rgb, self.pixels, self.ordinal, self.keep = w, h, rgb, pixels, ordinal, keep
        self.linear, self.scale = linear, scale   # linear: pixels are raw linear intensity 0..255 after `scale`, not sRGB samples


def _pair_image(x, layout, device, stream, background, what="image"):
    """`x` (the caller's parameter `what`) as process() accepts it -> _PairImage.  No device call."""
    background = _background(background)
    if not is_device_resident(x):
        if layout not in (None, "HWC"):
            raise ValueError("host pixels are [h][w][3]")
        if stream is not None:
            raise ValueError("stream= goes with device-resident pixels")
        px = np.asarray(x)
        if background is not None and px.dtype == np.uint8 and px.ndim == 3 and px.shape[2] in (2, 4):
            px = blend_on_background(px, background)
        rgb = np.ascontiguousarray(px, np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"host pixels are [h][w][3], not {rgb.shape}")
        return _PairImage(rgb.shape[1], rgb.shape[0], rgb=rgb)
    src = da.read(x, device, what)
    w, h, strides, alpha = da.source(src, layout, background)
    code = DTYPE_CODES[src.dtype]
    pixels = device_pixels(src.ptr, code, strides, da.stream_or(stream, src.stream), da.alpha_address(src.ptr, alpha, ITEMSIZE[code]),
                           background or (0, 0, 0))
    return _PairImage(w, h, pixels=pixels, ordinal=src.ordinal, keep=x)


def _linear_scale(scale):
    s = float(np.float32(scale))
    if not 0 < s < float("inf"):
        raise ValueError(f"scale={scale}: a finite float32 above 0 (1 for data in 0..255, 255 for data in [0, 1])")
    return s


def _linear_image(x, layout, device, stream, scale, what="image"):
    """`x` (the caller's parameter `what`) as a LINEAR float image -> _PairImage: a GPU tensor / __cuda_array_interface__
    object of float32, float16 or bfloat16 in any layout and strides process() takes, three channels or one; host float32 / float16 arrays are
    uploaded first.  ValueError for everything else.  No device call but that upload."""
    scale = _linear_scale(scale)
    if not is_device_resident(x):
        a = np.asarray(x)
        if a.dtype.name not in ("float32", "float16"):
            raise ValueError(f"dtype {a.dtype}: a linear image is float32, float16 or bfloat16 (no integers; convert float64 yourself: it is a rounding)")
        if a.ndim not in (2, 3):
            raise ValueError(f"an image has 2 or 3 dimensions, not {a.ndim}")
        x = da.upload(a, 0 if device is None else device)
    src = da.read(x, device, what, dtypes=LINEAR_DTYPES, error=ValueError)
    try:
        w, h, strides, _ = da.source(src, layout)
    except da.AlphaRefused:
        raise ValueError("a linear image has three channels, or one (grey): alpha is not supported") from None
    return _PairImage(w, h, pixels=device_pixels(src.ptr, DTYPE_CODES[src.dtype], strides, da.stream_or(stream, src.stream)),
                      ordinal=src.ordinal, keep=x, linear=True, scale=scale)


def _pair_sizes(ref, other):
    if min(ref.w, ref.h) < 8:
        raise ValueError(f"a {ref.w} x {ref.h} image: butteraugli needs at least 8 x 8")
    if other is not None and (other.w, other.h) != (ref.w, ref.h):
        raise ValueError(f"the images differ in size: {ref.w} x {ref.h} against {other.w} x {other.h}")


class Comparator:
    """One reference image against many distorted ones: the reference's psycho image (OpsinDynamicsImage +
    SeparateFrequencies + its half of the mask) is computed once, here, and kept on the GPU.  `reference` as process()
    accepts an image -- host pixels numpy turns into uint8 [h][w][3], or a GPU tensor / __cuda_array_interface__ object
    of any dtype, layout and strides process() takes, with layout=, background= and stream= as there.
    The metric is ASYMMETRIC: this image is butteraugli's first argument, the one the masking is computed from.  The
    bytes compared are the bytes process() would encode (floats in [0, 1] rounded to bytes, uint16's high byte, alpha
    blended over background=).
    linear=True: the images are LINEAR float images instead, as ButteraugliInterface takes them -- float32 / float16 /
    bfloat16, three channels or one, raw linear intensity 0..255 after the multiplication by scale= (scale=255 is for
    data in [0, 1]); nothing is rounded to a byte, so images closer than a byte step have a distance.  Values outside
    [0, 255] after the scale (NaN too) are CLAMPED to it, which the reference does not do; `clamped` counts them.
    linear= and scale= are the defaults of compare(), which may mix: an 8-bit image against a linear reference is its
    table-linearised bytes against it.
    A context manager; close() frees the GPU memory."""

    def __init__(self, reference, layout=None, device=None, stream=None, background=None, linear=False, scale=1.0):
        self.linear, self.scale = bool(linear), _linear_scale(scale)
        self.clamped = 0   # elements of the last compare()'s image that the clamp of linear=True altered
        if self.linear:
            if background is not None:
                raise ValueError("background= goes with 8-bit pixels: a linear image has no alpha")
            ref = _linear_image(reference, layout, device, stream, self.scale, "reference")
        else:
            ref = _pair_image(reference, layout, device, stream, background, "reference")
        _pair_sizes(ref, None)
        self._open(ref, ref.ordinal if ref.ordinal is not None else (0 if device is None else device))

    def _open(self, ref, ordinal):
        from .capi import Context
        lib = _pair_library()
        self.w, self.h, self.device = ref.w, ref.h, ordinal
        # (the target only scales gz_block_weights, which nothing here asks for)
        if ref.linear:
            self._ctx = Context.from_device_linear(lib, ref.pixels, ref.w, ref.h, ref.scale, ordinal)
        else:
            self._ctx = lib.context(ref.rgb, 1.0, ordinal) if ref.rgb is not None else Context.from_device(lib, ref.pixels, ref.w, ref.h, 1.0, ordinal)

    @classmethod
    def _of(cls, ref, ordinal):
        self = cls.__new__(cls)
        self.linear, self.scale, self.clamped = ref.linear, ref.scale, 0
        self._open(ref, ordinal)
        return self

    def close(self):
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx is not None:
            ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()

    def _destination(self, distmap, stream):
        """distmap= -> (what compare returns as the map, capi.GzDeviceMap) -- (None, None) without one."""
        if distmap is None or distmap is False:
            return None, None
        if distmap is True:
            distmap = da.new_tensor((self.h, self.w), "float32", self.device)
        return distmap, _map_output(distmap, (self.h, self.w), self.device, stream)

    def _heat_destination(self, heatmap, good, bad, stream):
        """heatmap= -> (what compare returns as the heat map, capi.GzDeviceOutput, good, bad) -- None without one."""
        if heatmap is None or heatmap is False:
            return None
        good, bad = _heat_thresholds(good, bad)
        if heatmap is True:
            heatmap = da.new_tensor((self.h, self.w, 3), "uint8", self.device)
        return heatmap, _image_output(heatmap, self.w, self.h, None, self.device, stream, "heatmap="), good, bad

    def _compare(self, other, out, dmap, heat=None):
        if self._ctx is None:
            raise ValueError("the Comparator is closed")
        self.clamped = 0
        if other.linear:
            d, self.clamped = self._ctx.compare_device_linear(other.pixels, other.scale, dmap, *(() if heat is None else (heat[1], heat[2], heat[3])))
        elif other.rgb is not None:   # host bytes: their map comes back to the host too, and is emitted from the plane it left
            d, _ = self._ctx.compare_rgb(other.rgb, want_distmap=dmap is not None or heat is not None)
            if dmap is not None:
                self._ctx.distmap_device(dmap)
            if heat is not None:
                self._ctx.heatmap_device(heat[2], heat[3], heat[1])
        elif heat is not None:
            d = self._ctx.compare_device_pixels_heat(other.pixels, heat[1], heat[2], heat[3], dmap)
        else:
            d = self._ctx.compare_device_pixels(other.pixels, dmap)
        if dmap is None and heat is None:
            return d
        return (d,) + (() if dmap is None else (out,)) + (() if heat is None else (heat[0],))

    def compare(self, distorted, distmap=None, layout=None, stream=None, background=None, heatmap=None, good=None, bad=None,
                linear=None, scale=None):
        """The butteraugli distance of `distorted` (as process() accepts an image; the reference's size, on its GPU)
        from the reference -> float, or with distmap= -> (float, map).  distmap=True: a fresh float32 [H, W] torch
        tensor on the reference's GPU, allocated on the calling thread's current stream; work enqueued on that stream
        afterwards sees the map.  distmap=tensor: that 2-D float32 / float16 / bfloat16 tensor (or
        __cuda_array_interface__ object) is filled under its own strides -- a crop inside a larger tensor is written
        without touching what surrounds it; flipped and expanded views are refused -- and returned.  stream= overrides
        the producer's stream of `distorted` and the consumer's of the map (a hipStream_t handle; 0: none).
        heatmap=: butteraugli's colour picture of the map (CreateHeatMapImage, byte for byte) is appended to the return
        value -- (float, heat) or (float, map, heat).  True: a fresh uint8 [H, W, 3] torch tensor on the reference's
        GPU; a tensor: filled in place, of any dtype, layout ([H, W, 3] or [3, H, W]) and crop view decode(out=) takes,
        with the same refusals.  good= and bad=: ScoreToRgb's thresholds, by default fuzzy_inverse(1.5) and
        fuzzy_inverse(0.5), as the reference's tool draws its heat maps.
        linear= and scale= (default: the Comparator's own): `distorted` is a linear float image, raw linear intensity
        0..255 after scale= (255 for data in [0, 1]); values outside [0, 255] are clamped, and `clamped` holds how many
        of this call's image were."""
        if self.linear if linear is None else linear:
            if background is not None:
                raise ValueError("background= goes with 8-bit pixels: a linear image has no alpha")
            other = _linear_image(distorted, layout, self.device, stream, self.scale if scale is None else scale, "distorted")
            consumer = stream
        else:
            other = _pair_image(distorted, layout, self.device if is_device_resident(distorted) else None, stream, background, "distorted")
            consumer = stream if is_device_resident(distorted) else None
        _pair_sizes(_PairImage(self.w, self.h), other)
        heat = self._heat_destination(heatmap, good, bad, consumer)
        out, dmap = self._destination(distmap, consumer)
        return self._compare(other, out, dmap, heat)


def butteraugli(reference, distorted, distmap=None, layout=None, device=None, stream=None, background=None, heatmap=None,
                good=None, bad=None):
    """The butteraugli distance (guetzli's, bit for bit) of two images of one size -> float, or with distmap= ->
    (float, map): distmap=True gives a float32 [H, W] torch tensor on the reference's GPU, distmap=tensor fills a 2-D
    float32 / float16 / bfloat16 tensor (see Comparator.compare).
    The metric is ASYMMETRIC: `reference` is butteraugli's first argument (the original, whose masking counts),
    `distorted` its second.  Both are accepted exactly as process() accepts an image -- host pixels, or GPU tensors /
    __cuda_array_interface__ objects of every dtype, layout and stride it takes; layout=, background= and stream=
    apply to both -- and the bytes compared are the bytes process() would encode.
    ValueError, before anything is computed: sizes that differ, sizes under 8 x 8, images on different devices.
    heatmap=, good=, bad=: the map's heat map, appended to the return value (see Comparator.compare).
    For many images against one reference, Comparator keeps the reference's half of the work."""
    ref = _pair_image(reference, layout, device, stream if is_device_resident(reference) else None, background, "reference")
    known = ref.ordinal if ref.ordinal is not None else device
    other = _pair_image(distorted, layout, known if is_device_resident(distorted) else None,
                        stream if is_device_resident(distorted) else None, background, "distorted")
    _pair_sizes(ref, other)
    ordinal = known if known is not None else (other.ordinal if other.ordinal is not None else 0)
    if distmap is not None and distmap is not False and distmap is not True:
        da.destination(distmap, (ref.h, ref.w), MAP_DTYPES, ordinal, "distmap=")   # (refused before the reference is worked on)
    if heatmap is not None and heatmap is not False:
        _heat_thresholds(good, bad)
        if heatmap is not True:
            da.image_destination(heatmap, ref.w, ref.h, None, da.DTYPES, ordinal, "heatmap=")
    with Comparator._of(ref, ordinal) as cmp:
        consumer = stream if (ref.pixels is not None or other.pixels is not None) else None
        heat = cmp._heat_destination(heatmap, good, bad, consumer)
        out, dmap = cmp._destination(distmap, consumer)
        return cmp._compare(other, out, dmap, heat)


BATCH_MAX_PIXELS = 1500000   # gz_butteraugli_batch: w * h below this
BATCH_DTYPES = ("uint8", "float32", "float16", "bfloat16")


def _batch_images(x, layout, device, stream, what, one_image_too=False):
    """A batch [N,3,H,W] / [N,H,W,3] (with one_image_too also one image, 2-D or 3-D: n = 1) -> (capi.GzDeviceBatch, n, w, h, ordinal, keep).
    Host arrays are uploaded first, on the calling thread's current stream."""
    if not is_device_resident(x):
        x = da.upload(np.asarray(x), 0 if device is None else device)
    src = da.read(x, device, what, dtypes=None)
    if src.dtype not in BATCH_DTYPES:
        raise ValueError(f"{what} has dtype {src.dtype}: a batch takes uint8, float32, float16 or bfloat16 (16-bit integer samples: "
                         "compare the images one by one with butteraugli())")
    if len(src.shape) == 4:
        n, sn, image = src.shape[0], src.strides[0], src._replace(shape=src.shape[1:], strides=src.strides[1:])
        if n < 1:
            raise ValueError(f"{what} is an empty batch")
    elif len(src.shape) in (2, 3) and one_image_too:
        n, sn, image = 1, 0, src
    else:
        raise ValueError(f"{what} has {len(src.shape)} dimensions: a batch is [N,3,H,W] or [N,H,W,3]")
    try:
        w, h, strides, _ = da.source(image, layout, outer=(sn,))
    except da.AlphaRefused:
        raise ValueError(f"{what} of shape {image.shape}: a batch takes 3 channels, or 1 (grey) -- no alpha; blend the images "
                         "first, or compare them one by one with butteraugli(background=)") from None
    return device_batch(src.ptr, DTYPE_CODES[src.dtype], (sn,) + strides, da.stream_or(stream, src.stream)), n, w, h, src.ordinal, x


def butteraugli_batch(reference, distorted, distmap=None, layout=None, device=None, stream=None, scratch_bytes=0):
    """The butteraugli distances of N image pairs of one size with the kernel launches of ONE comparison -> a float32 [N]
    tensor on the GPU, or with distmap= -> (distances, maps).  Pair i is, bit for bit, butteraugli(reference[i],
    distorted[i]).
    distorted: a 4-D GPU tensor [N,3,H,W] or [N,H,W,3] (or [N,1,H,W] / [N,H,W,1]: grey) of uint8, float32, float16 or
    bfloat16 under ANY non-negative strides -- a slice x[::2], crop views, an expanded image; layout= ("CHW" / "HWC",
    per image) where the shape does not say.  A host array is uploaded first.  reference: the same shape, or ONE 3-D
    image that all N are compared with (its half of the work is done once).  The metric is ASYMMETRIC, as butteraugli()'s.
    distmap=True: float32 [N,H,W]; distmap=tensor: that 3-D float32 / float16 / bfloat16 tensor is filled under its own
    strides (a view inside a larger tensor keeps its surroundings) and returned.  stream= overrides the producer's
    stream of both batches and the consumer's of the maps.  The call waits for its own work: the distances are complete
    when it returns, and work on the calling thread's current stream sees the maps.
    scratch_bytes= caps the device memory of the call's image arenas (172 bytes per pixel and image; default 2 GiB):
    a batch that needs more runs in chunks, with the same results.
    ValueError, before anything is computed: sizes that differ, sizes under 8 x 8, images of 1.5 MPix and more (they
    gain nothing: Comparator keeps one reference for many images), alpha or 2 / 4 channels, 16-bit integer samples."""
    other, n, w, h, ordinal, keep1 = _batch_images(distorted, layout, device, stream, "distorted")
    ref, n_ref, rw, rh, _, keep0 = _batch_images(reference, layout, ordinal, stream, "reference", one_image_too=True)
    if (rw, rh) != (w, h):
        raise ValueError(f"the images differ in size: {rw} x {rh} against {w} x {h}")
    if n_ref not in (1, n):
        raise ValueError(f"{n_ref} reference images against {n} distorted ones: as many, or one for all")
    if min(w, h) < 8:
        raise ValueError(f"a {w} x {h} image: butteraugli needs at least 8 x 8")
    if w * h >= BATCH_MAX_PIXELS:
        raise ValueError(f"{w} x {h} images: a batch takes images under {BATCH_MAX_PIXELS} pixels -- larger ones fill the GPU alone; "
                         "use Comparator (one reference, many images) or butteraugli()")
    maps = out = None
    if distmap is not None and distmap is not False:
        out = da.new_tensor((n, h, w), "float32", ordinal) if distmap is True else distmap
        maps = _map_output(out, (n, h, w), ordinal, stream)
    dist = da.new_tensor((n,), "float32", ordinal)
    dptr = da.read(dist, ordinal, "the distances").ptr
    _pair_library().butteraugli_batch(ref, other, w, h, n, dptr, n_ref=n_ref, maps=maps, scratch_bytes=int(scratch_bytes), device=ordinal)
    del keep0, keep1
    return dist if out is None else (dist, out)


def butteraugli_linear(reference, distorted, scale=1.0, distmap=None, heatmap=None, good=None, bad=None, layout=None, device=None,
                       stream=None, strict=False):
    """ButteraugliInterface (butteraugli.h:44-79) of two LINEAR float images of one size, from 1 x 1 up -> what
    butteraugli() returns: float, or with distmap= / heatmap= a tuple with the map and the heat map (see
    Comparator.compare).  `reference` is butteraugli's first argument; the metric is ASYMMETRIC.
    The values are raw linear intensity 0..255 AFTER the multiplication by scale=: scale=1 for data in 0..255, scale=255
    for data in [0, 1].  Nothing is rounded to a byte and nothing is gamma-decoded: images closer than a byte step have a
    distance, which butteraugli() cannot see.  Values outside [0, 255] after the scale (NaN too) are CLAMPED to it -- the
    reference is undefined there and does not clamp; strict=True raises ValueError after the call if any element of
    either image was.
    The images: GPU tensors / __cuda_array_interface__ objects of float32, float16 or bfloat16 -- HWC or CHW, three
    channels or one, crops and strided views, as process() takes them; host float32 / float16 arrays are uploaded first.
    Under 8 pixels in a dimension the images are extended by replicating their border, as the reference does; map and heat
    map are of the images' own size.
    ValueError, before anything is computed: sizes that differ, integer dtypes, four channels, images on different
    devices."""
    scale = _linear_scale(scale)
    ref = _linear_image(reference, layout, device, stream, scale, "reference")
    other = _linear_image(distorted, layout, ref.ordinal, stream, scale, "distorted")
    if (other.w, other.h) != (ref.w, ref.h):
        raise ValueError(f"the images differ in size: {ref.w} x {ref.h} against {other.w} x {other.h}")
    w, h, ordinal = ref.w, ref.h, ref.ordinal
    out = dmap = heat = None
    if distmap is not None and distmap is not False:
        out = da.new_tensor((h, w), "float32", ordinal) if distmap is True else distmap
        dmap = _map_output(out, (h, w), ordinal, stream)
    if heatmap is not None and heatmap is not False:
        good, bad = _heat_thresholds(good, bad)
        hout = da.new_tensor((h, w, 3), "uint8", ordinal) if heatmap is True else heatmap
        heat = (hout, _image_output(hout, w, h, None, ordinal, stream, "heatmap="))
    d, clamped = _pair_library().butteraugli_linear(ref.pixels, other.pixels, w, h, scale, dmap, None if heat is None else heat[1],
                                                    good if heat else 0.0, bad if heat else 0.0, device=ordinal)
    if strict and clamped:
        raise ValueError(f"{clamped} elements of the two images lie outside [0, 255] after scale={scale} (NaN included) and were clamped")
    if dmap is None and heat is None:
        return d
    return (d,) + (() if dmap is None else (out,)) + (() if heat is None else (heat[0],))


def fuzzy_class(score):
    """ButteraugliFuzzyClass (butteraugli.cc:1903-1921): a distance as a quality class between 2 (good) and 0 (bad)."""
    return _pair_library().fuzzy_class(score)


def fuzzy_inverse(seek):
    """ButteraugliFuzzyInverse (butteraugli.cc:1923-1934): the distance of the class `seek`."""
    return _pair_library().fuzzy_inverse(seek)


def heatmap(distmap, good=None, bad=None, out=None, dtype="uint8", layout="HWC", stream=None):
    """butteraugli's heat map (CreateHeatMapImage, byte for byte) of any float32 2-D distance map on a GPU -- a torch
    tensor, or an object with __cuda_array_interface__; a tensor that is not contiguous in x is copied first.
    Returns a torch tensor on the map's GPU, [H, W, 3] ("HWC") or [3, H, W] ("CHW") of `dtype` -- uint8 the bytes,
    uint16 byte * 257, float32 / float16 / bfloat16 byte / 255 -- or fills out= as decode(out=) does.  good= and bad=
    as in Comparator.compare.  The map must be complete on the calling thread's current stream (stream= overrides: a
    hipStream_t handle; 0: none -- the map is complete when the call starts); work enqueued there afterwards sees the
    picture."""
    good, bad = _heat_thresholds(good, bad)
    ptr, w, h, pitch, ordinal, keep = _heat_source(distmap)
    if out is None:
        out = da.new_tensor(da.image_shape(w, h, layout), dtype, ordinal)
    _pair_library().heatmap_from_map_device(ptr, w, h, pitch, good, bad, _image_output(out, w, h, None, ordinal, stream, "out="), device=ordinal)
    del keep
    return out


# ---- butteraugli's masking on the GPU: the opsin image, Mask, the quantisation field ----
def _masking_image(x, linear, image_layout, device, stream, background, scale, what="image"):
    """`x` as butteraugli() (linear=False) or butteraugli_linear() (linear=True) takes an image -> _PairImage with
    device-resident pixels: host arrays are uploaded first."""
    if linear:
        if background is not None:
            raise ValueError("background= goes with 8-bit pixels: a linear image has no alpha")
        return _linear_image(x, image_layout, device, stream, scale, what)
    if not is_device_resident(x):
        host = _pair_image(x, image_layout, None, None, background)      # (its checks, and the blend of host alpha)
        x, image_layout, background = da.upload(host.rgb, 0 if device is None else device), "HWC", None
    return _pair_image(x, image_layout, device, stream, background, what)


def _masking_size(img, least, what):
    if min(img.w, img.h) < least:
        raise ValueError(f"a {img.w} x {img.h} image: {what} needs at least {least} x {least}")


def _float_destination(out, w, h, dtype, layout, ordinal, stream, name="out="):
    """out= (None: a fresh tensor of `dtype` in `layout`) -> (the tensor, capi.GzDeviceOutput) for w x h x 3 floats."""
    shape = da.image_shape(w, h, layout)
    if out is None:
        if dtype not in MAP_DTYPES:
            raise TypeError(f"dtype {dtype}: float32, float16 or bfloat16")
        out = da.new_tensor(shape, dtype, ordinal)
    return out, _image_output(out, w, h, layout, ordinal, stream, name, MAP_DTYPES)


def _strict_clamp(strict, clamped, scale, what):
    if strict and clamped:
        raise ValueError(f"{clamped} elements of {what} lie outside [0, 255] after scale={scale} (NaN included) and were clamped")


def opsin_dynamics(image, linear=False, scale=1.0, out=None, dtype="float32", layout="CHW", device=None, stream=None,
                   background=None, strict=False, image_layout=None):
    """butteraugli's OpsinDynamicsImage -- the XYB image Mask is fed with -- of an image, on its GPU -> a torch tensor
    [3, H, W] ("CHW") or [H, W, 3] ("HWC") of `dtype` (float32: the reference's floats bit for bit; float16 / bfloat16:
    rounded to nearest even), or out= filled in place and returned (a GPU tensor of a float type in `layout`; a crop view
    is written without touching what surrounds it).
    linear=False: `image` as butteraugli() takes one -- host pixels or a GPU tensor of any dtype, alpha over background= --
    its bytes linearised by the sRGB table.  linear=True: as butteraugli_linear() takes one -- float32 / float16 /
    bfloat16, raw linear intensity 0..255 after scale=, values outside it CLAMPED (strict=True raises if any was).
    image_layout= names the layout of `image` where its shape is ambiguous.  stream= overrides the producer's stream of
    the image and the consumer's of the result.  ValueError, before anything is computed: an image under 8 x 8."""
    scale = _linear_scale(scale)
    img = _masking_image(image, linear, image_layout, device, stream, background, scale)
    _masking_size(img, 8, "the opsin image")
    out, dest = _float_destination(out, img.w, img.h, dtype, layout, img.ordinal, stream)
    clamped = _pair_library().opsin_device(img.pixels, img.w, img.h, dest, GZ_SAMPLES_LINEAR if linear else GZ_SAMPLES_SRGB8, scale,
                                           device=img.ordinal)
    _strict_clamp(strict, clamped, scale, "the image")
    return out


def mask(reference, distorted=None, dc=False, linear=False, scale=1.0, out=None, out_dc=None, dtype="float32", layout="CHW",
         device=None, stream=None, background=None, strict=False, image_layout=None):
    """butteraugli's Mask(OpsinDynamicsImage(reference), OpsinDynamicsImage(distorted)) on the GPU: the visual-masking
    image, which says where an error of a given size is visible -> a torch tensor [3, H, W] / [H, W, 3] as
    opsin_dynamics() returns one; dc=True (or out_dc=): the tuple (mask, mask_dc).  distorted=None is the mask of an
    image with itself, which the encoder's block search works with.  The images, linear=, scale=, the clamp, strict=,
    out= / out_dc=, dtype=, layout=, stream= and the 8 x 8 lower bound as for opsin_dynamics(); both images have one size
    and live on one GPU."""
    scale = _linear_scale(scale)
    ref = _masking_image(reference, linear, image_layout, device, stream, background, scale, "reference")
    other = None if distorted is None else _masking_image(distorted, linear, image_layout, ref.ordinal, stream, background, scale, "distorted")
    _masking_size(ref, 8, "Mask")
    if other is not None and (other.w, other.h) != (ref.w, ref.h):
        raise ValueError(f"the images differ in size: {ref.w} x {ref.h} against {other.w} x {other.h}")
    out, dest = _float_destination(out, ref.w, ref.h, dtype, layout, ref.ordinal, stream)
    out_dc, dest_dc = _float_destination(out_dc, ref.w, ref.h, dtype, layout, ref.ordinal, stream, "out_dc=") if dc or out_dc is not None else (None, None)
    clamped = _pair_library().mask_device(ref.pixels, None if other is None else other.pixels, ref.w, ref.h, dest, dest_dc,
                                          GZ_SAMPLES_LINEAR if linear else GZ_SAMPLES_SRGB8, scale, device=ref.ordinal)
    _strict_clamp(strict, clamped, scale, "the images")
    return out if out_dc is None else (out, out_dc)


def adaptive_quantization(image, scale=1.0, out=None, dtype="float32", layout=None, device=None, stream=None, strict=False):
    """ButteraugliAdaptiveQuantization (butteraugli.cc:1880-1901) on the GPU: the per-pixel field a codec multiplies its
    quantisation steps with -- plane 1 of Mask applied to the LINEAR RGB planes themselves, as the reference computes
    it -> a float [H, W] torch tensor of `dtype` on the image's GPU, or out= (a 2-D GPU tensor of a float type, crop views
    included) filled in place and returned.  `image` is a linear float image as butteraugli_linear() takes one (layout=
    names its layout where the shape is ambiguous), raw linear intensity 0..255 after scale=; values outside it are
    CLAMPED (strict=True raises if any was).  ValueError, before anything is computed: an image under 16 x 16, where the
    reference gives up."""
    scale = _linear_scale(scale)
    img = _linear_image(image, layout, device, stream, scale, "image")
    _masking_size(img, 16, "the quantisation field")
    if out is None:
        if dtype not in MAP_DTYPES:
            raise TypeError(f"dtype {dtype}: float32, float16 or bfloat16")
        out = da.new_tensor((img.h, img.w), dtype, img.ordinal)
    quant = _map_output(out, (img.h, img.w), img.ordinal, stream, "out=")
    clamped = _pair_library().adaptive_quantization(img.pixels, img.w, img.h, quant, scale, device=img.ordinal)
    _strict_clamp(strict, clamped, scale, "the image")
    return out

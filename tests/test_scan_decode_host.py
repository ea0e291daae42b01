"""The host driver with the device's scan decoder behind its reader (gzh_decode_jpeg_coeffs in both modes, on the CPU
emulation): test_jpeg_reader.py's Pillow cases and sizes -- baseline, progressive, optimised tables, restart intervals,
4:4:4 / 4:2:2 / 4:2:0, metadata -- give equal coefficients, sizes, metadata and tail bytes whoever reads the scan, and the
reported path is "device" exactly for the eligible ones.  CPU only."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "emu")]
import build_emu  # noqa: E402
import images  # noqa: E402

from PIL import Image  # noqa: E402,F401
from test_jpeg_reader import CASES, jpeg_bytes  # noqa: E402

SIZES = [(96, 64), (61, 43), (17, 9), (8, 8)]


def writable(kw):
    """Whether this Pillow knows every option of the case (restart_marker_blocks / _rows came with 10.2)."""
    try:
        jpeg_bytes(np.zeros((8, 8, 3), np.uint8), **kw)
    except TypeError:
        return False
    return True


WRITABLE = [(i, kw) for i, kw in enumerate(CASES) if writable(kw)]
assert any(kw.get("subsampling") == 2 and not kw.get("progressive") for _, kw in WRITABLE) and len(WRITABLE) >= 8


@pytest.fixture(scope="module")
def host():
    from guetzli_amd.encoder import HostLibrary
    return HostLibrary(build_emu.build_host())


def eligible(kw):
    return not kw.get("progressive") and not kw.get("restart_marker_blocks") and not kw.get("restart_marker_rows") and kw.get("subsampling") in (0, 2)


def both(host, data, expect_device):
    plain, got = host.decode_jpeg_coeffs(data, "host"), host.decode_jpeg_coeffs(data, "device")
    assert (plain is None) == (got is None)
    if plain is None:
        return None
    assert plain[2]["path"] == "host" and plain[2]["status"] is None
    assert got[2]["path"] == ("device" if expect_device else "host"), got[2]
    assert got[2]["status"] == ("DECODED" if expect_device else None), got[2]
    assert np.array_equal(got[0], plain[0]) and got[1] == plain[1]
    assert got[3] == plain[3]          # every APPn, COM and the tail
    return got


@pytest.mark.parametrize("kw", [kw for _, kw in WRITABLE], ids=[str(i) for i, _ in WRITABLE])
@pytest.mark.parametrize("wh", SIZES)
def test_both_modes_read_the_same(host, kw, wh):
    w, h = wh
    data = jpeg_bytes(images.crop(w, h, 120, 80), **kw)
    got = both(host, data, eligible(kw))
    if kw.get("subsampling") == 1:
        assert got is None      # 4:2:2: DecodeJpegToRGB has no pixels for it, in either mode
    elif eligible(kw):
        assert got is not None and got[1][:2] == (w, h) and got[2]["end_offset"] > 0 and got[2]["subsequences"] >= 1
    elif got is not None:       # (a case the reader refuses, as the reference does, is refused in both modes)
        assert got[1][:2] == (w, h)


def test_grey_metadata_and_tail(host):
    rgb = images.crop(80, 56, 10, 10)
    grey = jpeg_bytes(np.ascontiguousarray(rgb[:, :, 1]), quality=90)
    got = both(host, grey, True)
    assert got[1] == (80, 56, 1) and not got[0][70:].any()      # the two chroma components of a grey file are zero
    exif = b"Exif\x00\x00" + bytes(range(200))
    data = jpeg_bytes(rgb, quality=90, subsampling=0, exif=exif, comment=b"a comment") + b"trailing bytes after EOI"
    got = both(host, data, True)
    assert got[3].endswith(b"T%08d" % 24 + b"trailing bytes after EOI") and exif in got[3] and b"a comment" in got[3]


def test_what_follows_the_scan_gets_the_hosts_verdict(host):
    """The parser goes on where the device's decoder ends: a missing EOI, garbage in front of it, a second scan and a
    truncated scan are judged by the host reader as ever."""
    good = jpeg_bytes(images.crop(64, 48, 30, 30), quality=90, subsampling=0)
    sos = good.index(b"\xff\xda")
    for data, device in ((good[:-2], True), (good[:-2] + b"\x00\x01\x02\xff\xd9tail", True), (good[:-2] + good[sos:], True),
                         (good[:len(good) // 2], False), (good[:-2] + b"\xff\x00\xd9", False), (good[:-1] + b"\x00", True)):
        plain, got = host.decode_jpeg_coeffs(data, "host"), host.decode_jpeg_coeffs(data, "device")
        assert (plain is None) == (got is None), data[-12:]
        if plain is not None:
            assert np.array_equal(got[0], plain[0]) and got[3] == plain[3] and (got[2]["path"] == "device") == device, (data[-12:], got[2])

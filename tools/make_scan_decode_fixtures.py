"""Writes the JPEGs of tests/golden/scan_decode/ (run once, where Pillow is installed; the tests read the committed
files and need no Pillow): crops of tests/golden/bees.png at (120, 80) as Pillow's libjpeg writes them -- baseline scans
the device's Huffman decoder takes -- and beside each its twins the decoder must leave to the host: progressive, with a
restart interval, 4:2:2.

    python tools/make_scan_decode_fixtures.py
"""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "scan_decode")

# name: (w, h, quality, subsampling (Pillow's: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0; None: one component), optimize)
ELIGIBLE = {
    "64x48_q90_444": (64, 48, 90, 0, False),
    "61x43_q85_420": (61, 43, 85, 2, False),
    "96x64_q75_444_opt": (96, 64, 75, 0, True),
    "33x31_grey": (33, 31, 90, None, False),
    "8x8_444": (8, 8, 90, 0, False), "8x8_420": (8, 8, 90, 2, False),
    "1x1_444": (1, 1, 90, 0, False), "1x1_420": (1, 1, 90, 2, False),
    "9x8_444": (9, 8, 90, 0, False), "9x8_420": (9, 8, 90, 2, False),
    "17x9_444": (17, 9, 90, 0, False), "17x9_420": (17, 9, 90, 2, False),
    "160x120_q95_444": (160, 120, 95, 0, False),
}


def save(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    from PIL import Image
    import images
    os.makedirs(OUT, exist_ok=True)
    for name, (w, h, q, sub, opt) in ELIGIBLE.items():
        rgb = images.crop(w, h, 120, 80)
        im = Image.fromarray(rgb)
        if sub is None:
            im = im.convert("L")
        kw = {"quality": q, "optimize": opt}
        if sub is not None:
            kw["subsampling"] = sub
        files = {name: save(im, **kw),
                 name + "__progressive": save(im, progressive=True, **kw),
                 name + "__restart": save(im, restart_marker_blocks=2, **kw)}
        if sub is not None:
            files[name + "__422"] = save(im, **dict(kw, subsampling=1))
        for n, data in files.items():
            assert len(data) <= 20 * 1024 or n.startswith("160x120"), (n, len(data))
            with open(os.path.join(OUT, n + ".jpg"), "wb") as f:
                f.write(data)
            print(n, len(data))


if __name__ == "__main__":
    main()

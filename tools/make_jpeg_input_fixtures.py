"""Writes the JPEGs of tests/golden/jpeg_input_device/ (run once, where Pillow is installed; the tests read the
committed files and need no Pillow): crops of tests/golden/bees.png at (120, 80) as Pillow's libjpeg writes them, all
baseline, for encodes of JPEG input whose scan the device reads (process_jpeg(entropy="device")).  The sizes are chosen
for the MCU padding, which that path stores and a decode does not: libjpeg fills it by edge replication, so the padding
blocks hold real coefficients.
  40x40_420  a 5 x 5 luma grid in a padded one of 6 x 6: padding to the right, below and in the corner
  72x40_420  9 x 5 in 10 x 6: an odd luma grid in both directions, the chroma grid (5 x 3) whole
  64x40_420  8 x 5 in 8 x 6: padding below only
  40x40_444  no padding

    python tools/make_jpeg_input_fixtures.py
"""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_input_device")

# name: (w, h, quality, Pillow's subsampling: 0 = 4:4:4, 2 = 4:2:0)
FIXTURES = {
    "40x40_420": (40, 40, 90, 2),
    "72x40_420": (72, 40, 90, 2),
    "64x40_420": (64, 40, 90, 2),
    "40x40_444": (40, 40, 90, 0),
}


def main():
    from PIL import Image
    import images
    os.makedirs(OUT, exist_ok=True)
    for name, (w, h, q, sub) in FIXTURES.items():
        b = io.BytesIO()
        Image.fromarray(images.crop(w, h, 120, 80)).save(b, "JPEG", quality=q, subsampling=sub)
        data = b.getvalue()
        assert len(data) <= 20 * 1024, (name, len(data))
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        print(name, len(data))


if __name__ == "__main__":
    main()

"""Records the reference's heat map of one plane as a fixture: tests/golden/heatmap/plane_67x17.npy (float32 [17][67],
heatmap_cases.golden_plane: threshold, sweep, boundary and special distances under the default thresholds) and
heat_67x17.npy (uint8 [17][67][3], butteraugli::CreateHeatMapImage of it out of oracle/_ref/libgz_ref.so, through
tests/cpp/heatmap_ref.cc).  Needs oracle/_ref built; CPU only.

    python tools/gen_heatmap_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import heatmap_cases as hc  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = hc.reference_helper(tmp)
        if lib is None:
            sys.exit("oracle/_ref/libgz_ref.so is not built")
        good, bad = lib.ref_fuzzy_inverse(1.5), lib.ref_fuzzy_inverse(0.5)
        plane = hc.golden_plane(good, bad)
        heat = hc.reference_heat(lib, plane, good, bad)
    os.makedirs(hc.GOLDEN, exist_ok=True)
    np.save(os.path.join(hc.GOLDEN, "plane_67x17.npy"), plane)
    np.save(os.path.join(hc.GOLDEN, "heat_67x17.npy"), heat)
    print(f"good {good!r} bad {bad!r}: {len(np.unique(heat.reshape(-1, 3), axis=0))} colours in {heat.shape}")


if __name__ == "__main__":
    main()

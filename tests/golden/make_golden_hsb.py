#!/opt/conda/bin/python3.9
"""Generate tests/golden/hsb_skimage_*.npz with the REAL scikit-image (0.18.3: the conda python3.9 the HED goldens came from):

    /opt/conda/bin/python3.9 tests/golden/make_golden_hsb.py

The float definition the integer one of stainlib_amd/augmentation/hsb.py is measured against: skimage.color.rgb2hsv in binary64, the hue
turned by dh, saturation and brightness moved by x (1 + d) for d < 0 and x (1 + (1 - x) d) otherwise, skimage.color.hsv2rgb,
floor(255 x + 1/2).  Each file holds a 128 x 128 synth_tile, a 64 x 64 block of random colours, five (dh, ds, dv) triples and the ten
outputs.  Only arrays are written.
"""
import os
import sys

import numpy as np
import skimage
from skimage.color import hsv2rgb, rgb2hsv

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import stain_oracle as so  # noqa: E402  (the tile generator only)


def shift(x, d):
    return x * (1.0 + d) if d < 0 else x * (1.0 + (1.0 - x) * d)


def float_hsb(rgb, sig):
    dh, ds, dv = (float(v) for v in sig)
    hsv = rgb2hsv(rgb.astype(np.float64) / 255.0)
    hsv[..., 0] = np.mod(hsv[..., 0] + dh, 1.0)
    hsv[..., 1] = np.clip(shift(hsv[..., 1], ds), 0.0, 1.0)
    hsv[..., 2] = np.clip(shift(hsv[..., 2], dv), 0.0, 1.0)
    return np.floor(255.0 * hsv2rgb(hsv) + 0.5).astype(np.uint8)


def drawn(seed, k, lo, hi):
    """k triples as an augmenter draws them: uniform reals.  NOT short decimals: at ds = -0.1 the float expression's 255 p = M - 0.9 C is
    an exact half for every pixel whose C is an odd multiple of 5, at dv = -0.9 its 255 v' = 0.1 M for every M = 5 mod 10, and binary64
    rounding noise then decides 2-4 % of the golden's own bytes (measured: 2.4e-2 and 4.4e-2 of the bytes differ there, each by 1) --
    the ties the integer definition exists to remove.  A drawn real has no such lattice."""
    return [tuple(float(v) for v in row) for row in np.random.RandomState(seed).uniform(lo, hi, size=(k, 3))]


CASES = {
    # name: (tile seed, colour seed, five (dh, ds, dv)): zero, the extremes (+-1, dh = 0.9, a sextant boundary) and drawn values
    "light_s2": (2, 11, [(0.0, 0.0, 0.0)] + drawn(21, 4, -0.1, 0.1)),
    "strong_s3": (3, 12, [(0.9, 1.0, 1.0), (1.0 / 6.0, -1.0, -1.0)] + drawn(31, 3, -1.0, 1.0)),
}


def main():
    print("scikit-image", skimage.__version__)
    for name, (seed, cseed, sigmas) in CASES.items():
        tile = so.synth_tile(128, 128, seed)
        colours = np.random.RandomState(cseed).randint(0, 256, size=(64, 64, 3)).astype(np.uint8)
        rec = {"tile": tile, "colours": colours, "sigmas": np.array(sigmas, dtype=np.float64),
               "skimage_version": np.array(skimage.__version__)}
        rec["tile_out"] = np.stack([float_hsb(tile, s) for s in sigmas])
        rec["colours_out"] = np.stack([float_hsb(colours, s) for s in sigmas])
        path = os.path.join(HERE, "hsb_skimage_%s.npz" % name)
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

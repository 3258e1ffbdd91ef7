#!/usr/bin/env python3
"""Generate tests/golden/blur_scipy.npz with the REAL SciPy (1.15):

    python tests/golden/make_golden_blur.py

The float definition the integer one of stainlib_amd/augmentation/blur.py is measured against: scipy.ndimage.gaussian_filter1d(
mode="nearest", radius=r) along both axes in binary64 with r = min(8, ceil(3 sigma)), then floor(x + 1/2).  Three 96 x 80 x 3 images --
default_rng(0).integers(0, 256) noise, a smooth sinusoid / ramp image, a 0 / 255 checkerboard of 8-pixel squares -- under seven sigmas.
Only arrays are written.
"""
import math
import os

import numpy as np
import scipy
from scipy.ndimage import gaussian_filter1d

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 96, 80
SIGMAS = (0.34, 0.5, 1.0, 1.7, 2.0, 2.5, 8.0 / 3.0)


def images():
    noise = np.random.default_rng(0).integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = np.stack([127.5 + 127.5 * np.sin(y / 7.0) * np.cos(x / 11.0), 255.0 * x / (W - 1), 255.0 * (y + x) / (H + W - 2)], axis=-1)
    smooth = np.floor(smooth + 0.5).astype(np.uint8)
    yi, xi = np.mgrid[0:H, 0:W]
    checker = np.repeat((255 * (((yi // 8) + (xi // 8)) & 1)).astype(np.uint8)[..., None], 3, axis=-1)
    return {"noise": noise, "smooth": smooth, "checker": checker}


def float_blur(img, sigma):
    r = min(8, int(math.ceil(3.0 * sigma)))
    x = img.astype(np.float64)
    x = gaussian_filter1d(x, sigma, axis=1, mode="nearest", radius=r)
    x = gaussian_filter1d(x, sigma, axis=0, mode="nearest", radius=r)
    return np.floor(x + 0.5).astype(np.uint8)


def main():
    print("scipy", scipy.__version__)
    rec = {"sigmas": np.array(SIGMAS, dtype=np.float64), "scipy_version": np.array(scipy.__version__)}
    for name, img in images().items():
        rec[name] = img
        rec[name + "_out"] = np.stack([float_blur(img, s) for s in SIGMAS])
    path = os.path.join(HERE, "blur_scipy.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

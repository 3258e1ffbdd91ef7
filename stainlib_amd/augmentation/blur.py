"""Gaussian blur (the "focus" item of the usual histopathology augmentation set: Tellez et al., HoVer-Net-style nuclei recipes), an
extension: a per-tile separable filter defined in INTEGERS on bytes so that every route computes the same bits.

The definition (blur_codes, blur_reference: int64 numpy; csrc/view_blur_kernels.hpp: the same in 32 bits on the device).  R = 8 is the
largest radius, Q = 256 the weight sum per axis.  A tile's blur is nine int32 codes (w_0 .. w_8): every w_k >= 0,
w_0 + 2 (w_1 + .. + w_8) == 256; the radius r is the largest k with w_k != 0; (256, 0, .., 0) is the identity.  Per channel of an
(h, w, 3) uint8 image `full`:
    Hs[y, x] = sum_{k=-8..8} w_|k| full[y, clamp(x + k, 0, w - 1)]                         (<= 65280, exact)
    B[y, x]  = (sum_{k=-8..8} w_|k| Hs[clamp(y + k, 0, h - 1), x] + 32768) >> 16            (rounded once)
The border replicates the image's edge.  From sigma to codes (a host convenience; the codes are what a call returns and what reproduces
it): r = min(8, ceil(3 sigma)); sigma <= 0 gives the identity; g_k = exp(-k^2 / (2 sigma^2)) for |k| <= r, normalised to sum 1 in
binary64; w_k = floor(256 g_k + 1/2) for k >= 1; w_0 = 256 - 2 sum_{k >= 1} w_k.
Against SciPy's gaussian_filter1d(mode="nearest", radius=r) along both axes in binary64 with floor(x + 1/2) every byte is within 3
(tests/golden/blur_scipy.npz): 8-bit weights are another definition, not a rounding of SciPy's.
"""
from __future__ import annotations

import math

import numpy as np

from ..utils.excepts import InvalidRangeError
from ..utils.stain_utils import is_uint8_image
from .augmenter import AugmenterBase

R = 8
Q = 256
SIGMA_MAX = R / 3.0
IDENTITY = (Q,) + (0,) * R


def blur_codes(sigmas):
    """The int32 codes (w_0 .. w_8) of float sigmas: (n,) -> (n, 9); a scalar -> (9,).  A sigma <= 0 gives the identity; sigmas must be
    finite and at most 8 / 3 (ValueError): beyond it the radius 8 would cut the kernel inside 3 sigma."""
    try:
        s = np.asarray(sigmas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sigmas must hold one blur sigma per tile: an (N,) array") from None
    if s.ndim > 1:
        raise ValueError(f"sigmas must hold one blur sigma per tile: an (N,) array, not one of shape {s.shape}")
    if not np.isfinite(s).all():
        raise ValueError("sigmas must be finite")
    if (s > SIGMA_MAX).any():
        raise ValueError("a blur sigma must be at most 8 / 3: the largest radius is 8")
    flat = s.reshape(-1)
    out = np.zeros((flat.size, R + 1), dtype=np.int64)
    for t, sigma in enumerate(flat):
        r = min(R, int(math.ceil(3.0 * sigma))) if sigma > 0 else 0
        if r > 0:
            k = np.arange(-r, r + 1, dtype=np.float64)
            g = np.exp(-(k * k) / (2.0 * sigma * sigma))
            g = g / g.sum()
            out[t, 1:r + 1] = np.floor(256.0 * g[r + 1:] + 0.5).astype(np.int64)
        out[t, 0] = Q - 2 * out[t, 1:].sum()
    return out.astype(np.int32).reshape(s.shape + (R + 1,))


def codes_ok(codes, max_r=R):
    """Per row of (..., 9) integer codes: whether it passes the rule -- no negative weight, w_0 + 2 (w_1 + .. + w_8) == 256, no non-zero
    w_k beyond max_r.  A row that fails it is the identity to the kernel."""
    c = np.asarray(codes).astype(np.int64)
    ok = (c >= 0).all(axis=-1) & (c[..., 0] + 2 * c[..., 1:].sum(axis=-1) == Q)
    return ok & (c[..., int(max_r) + 1:] == 0).all(axis=-1)


def codes_radius(codes):
    """Per row of (..., 9) codes the largest k with w_k != 0"""
    c = np.asarray(codes)
    return np.where(c != 0, np.arange(R + 1), 0).max(axis=-1)


def effective_codes(codes, max_r=R):
    """The codes as the kernel takes them under the bound max_r: rows that fail the rule replaced by the identity."""
    c = np.asarray(codes).astype(np.int64).copy()
    c[~codes_ok(c, max_r)] = IDENTITY
    return c


def blur_reference(img, codes_row):
    """The definition in int64 numpy: `img` (h, w, 3) -- or (h, w) -- uint8 and one codes row (9,) -> uint8 of the same shape.  A row
    that fails the rule is the identity."""
    x = np.asarray(img)
    if x.dtype != np.uint8 or x.ndim not in (2, 3):
        raise ValueError("blur_reference expects a uint8 (h, w, 3) image")
    c = np.asarray(codes_row)
    if c.shape != (R + 1,) or c.dtype.kind not in "iu":
        raise ValueError("codes_row must hold (w_0 .. w_8): nine integers (blur_codes)")
    wts = effective_codes(c)
    h, w = x.shape[:2]
    v = x.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    hs = np.zeros_like(v)
    for k in range(-R, R + 1):
        if wts[abs(k)]:
            hs += wts[abs(k)] * v[:, np.clip(xs + k, 0, w - 1)]
    b = np.zeros_like(v)
    for k in range(-R, R + 1):
        if wts[abs(k)]:
            b += wts[abs(k)] * hs[np.clip(ys + k, 0, h - 1)]
    return ((b + 32768) >> 16).astype(np.uint8)


class GaussianBlurAugmenter(AugmenterBase):
    """Gaussian blur of a random sigma in sigma_range = (lo, hi), 0 <= lo <= hi <= 8 / 3 (InvalidRangeError), in the integer definition
    of this module.  randomize() draws one uniform sigma from the GLOBAL numpy stream; until then the lower bound applies, as in the
    colour augmenters."""

    def __init__(self, sigma_range):
        super().__init__(keyword="gaussian_blur")
        try:
            bad = len(sigma_range) != 2 or not (0.0 <= sigma_range[0] <= sigma_range[1] <= SIGMA_MAX)
        except TypeError:
            bad = True
        if bad:
            raise InvalidRangeError("Blur Sigma", sigma_range)
        self._sigma_range = (float(sigma_range[0]), float(sigma_range[1]))
        self._sigma = self._sigma_range[0]

    def randomize(self):
        """One draw from the global numpy stream."""
        self._sigma = float(np.random.uniform(low=self._sigma_range[0], high=self._sigma_range[1], size=None))

    def randomize_batch(self, n):
        """n successive randomize() calls (same global stream order) -> (n,) float64 sigmas."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        s = np.empty((n,), dtype=np.float64)
        for t in range(n):
            self.randomize()
            s[t] = self._sigma
        return s

    def transform(self, patch):
        """(H, W, 3) uint8 ndarray -> (H, W, 3) uint8 ndarray under the augmenter's current sigma: numpy to numpy (blur_reference)."""
        if not is_uint8_image(patch):
            raise TypeError("GaussianBlurAugmenter.transform expects a uint8 (H, W, 3) ndarray")
        return blur_reference(patch, blur_codes(self._sigma))

    def transform_batch(self, tiles, sigmas=None, out=None, tensor_format=None, view=None, windows=None):
        """Batched: (N,H,W,3) uint8 device tensor, per-tile (N,) sigmas (default: the augmenter's current one for every tile) ->
        (out, codes): the (N,H,W,3) uint8 image -- or, with ``tensor_format``, the (N,3,H,W) tensor, written directly -- and the (N, 9)
        int32 codes used.  The raw route of engine.normalize_blur_view: it works behind any uint8 result (Reinhard, HED, HSB, luminosity).
        ``view``: a ``stainlib_amd.TileView`` (crop / flip / rot90, ``shrink=``) -- per tile only the window ``windows[t]`` (default:
        ``view.draw(N, H, W)``) of the blurred tile, in ONE pass; the blur is of the whole tile, so the window's edge sees the tile's real
        neighbours.  Returns (out, codes, windows)."""
        from .. import engine
        if view is not None or windows is not None:
            engine._view_call(view, windows, tiles, draw=False)
        if sigmas is None:
            n = int(tiles.shape[0]) if hasattr(tiles, "shape") and len(tiles.shape) == 4 else 1
            sigmas = [self._sigma] * n
        engine._blur_call(self, sigmas, tiles, view)
        engine._check_tiles(tiles)
        x, windows, draw = engine.blur_stage(tiles, self, sigmas, view, windows, {}, fmt=tensor_format, out=out)
        if view is not None:
            return x, draw.codes, windows
        return x, draw.codes

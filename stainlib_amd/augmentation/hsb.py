"""Hue / saturation / brightness colour augmentation (the "HSV-light / HSV-strong" half of the Tellez et al. colour-augmenter family),
an extension: the sibling of HedColorAugmenter, defined in INTEGERS on bytes so that every route computes the same bits.

The definition (hsb_codes, hsb_reference: int64 numpy; csrc/hsb_math.hpp: the same in 32 bits, host and device).  Q = 32768.  Per tile
three int32 codes (dhq, dsq, dvq) from the float shifts dh (any real, in turns) and ds, dv in [-1, 1]:
    dhq = floor((dh mod 1) 6 Q + 1/2) mod 6 Q       dsq = floor(ds Q + 1/2)       dvq = floor(dv Q + 1/2)
With rdiv(a, c) = (2 a + c) // (2 c) and rnd(x) = (x + Q / 2) >> 15, per pixel (r, g, b): M = max, m = min, C = M - m;
    hue         hq = 0 when C == 0, else (base, num) = (4, r - g) if M == b, else (2, b - r) if M == g, else (0, g - b) -- blue wins ties
                over green, green over red, as in scikit-image -- and hq = (base Q + rdiv((num + C) Q, C) - Q) mod 6 Q
    saturation  s = 0 when M == 0, else rdiv(C Q, M)
    value       v = rdiv(M Q, 255)
    scale(x, d) = x if d == 0;  rnd(x (Q + d)) if d < 0;  rnd(x (Q + rnd((Q - x) d))) if d > 0 (towards 1, never past it)
    hq' = (hq + dhq) mod 6 Q,  s' = scale(s, dsq),  v' = scale(v, dvq),  hi = hq' // Q,  fq = hq' - hi Q
    p = rnd(v' (Q - s')),  q = rnd(v' (Q - rnd(fq s'))),  t = rnd(v' (Q - rnd((Q - fq) s')))
    (R, G, B) by hi: 0 (v', t, p), 1 (q, v', p), 2 (p, v', t), 3 (p, q, v'), 4 (t, p, v'), 5 (v', p, q);  byte = (X 255 + Q / 2) >> 15
In real numbers: the hue turns by dh, s (1 + ds) for ds < 0 and s (1 + (1 - s) ds) otherwise, the same rule for the brightness.  Zero
codes are the identity on every colour; against scikit-image's rgb2hsv / hsv2rgb in binary64 with floor(255 x + 1/2) every byte is
within 1 (tests/golden/hsb_skimage_*.npz).  Codes outside their ranges are reduced: dhq mod 6 Q, dsq and dvq clamped to +-Q.
"""
from __future__ import annotations

import numpy as np

from ..utils.stain_utils import _to_device, is_uint8_image
from .augmenter import ColorAugmenterBase, _checked

Q = 32768


def hsb_codes(sigmas):
    """The int32 codes (dhq, dsq, dvq) of float shifts (dh, ds, dv): (..., 3) -> (..., 3).  dh is any real (turns); ds and dv must lie in
    [-1, 1] (ValueError)."""
    try:
        s = np.asarray(sigmas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sigmas must hold (hue, saturation, brightness) shifts: an (N, 3) array") from None
    if s.ndim < 1 or s.shape[-1] != 3:
        raise ValueError(f"sigmas must hold (hue, saturation, brightness) shifts: an (N, 3) array, not one of shape {s.shape}")
    if not np.isfinite(s).all():
        raise ValueError("sigmas must be finite")
    if (np.abs(s[..., 1:]) > 1.0).any():
        raise ValueError("the saturation and brightness shifts must lie in [-1, 1]")
    out = np.empty(s.shape, dtype=np.int64)
    out[..., 0] = np.floor(np.mod(s[..., 0], 1.0) * (6 * Q) + 0.5).astype(np.int64) % (6 * Q)
    out[..., 1] = np.floor(s[..., 1] * Q + 0.5).astype(np.int64)
    out[..., 2] = np.floor(s[..., 2] * Q + 0.5).astype(np.int64)
    return out.astype(np.int32)


def reduce_codes(codes):
    """Codes of any int32 values brought into their ranges as the kernels do it: dhq mod 6 Q (non-negative), dsq and dvq clamped to +-Q."""
    c = np.asarray(codes).astype(np.int64).copy()
    c[..., 0] %= 6 * Q
    c[..., 1:] = np.clip(c[..., 1:], -Q, Q)
    return c


def _rdiv(a, c):
    return (2 * a + c) // (2 * c)


def _rnd(x):
    return (x + Q // 2) >> 15


def _scale(x, d):
    neg = _rnd(x * (Q + d))
    pos = _rnd(x * (Q + _rnd((Q - x) * d)))
    return np.where(d == 0, x, np.where(d < 0, neg, pos))


def hsb_reference(rgb_u8, codes):
    """The definition in int64 numpy: `rgb_u8` (..., 3) uint8 with one code triple (3,), or (N, ..., 3) with codes (N, 3) -> uint8 of
    the same shape.  Codes are reduced first (reduce_codes)."""
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError("hsb_reference expects a uint8 array whose last axis is (r, g, b)")
    c = reduce_codes(codes)
    if c.shape == (3,):
        c = c.reshape((1,) * (rgb.ndim - 1) + (3,))
    elif c.ndim == 2 and c.shape[1] == 3 and rgb.ndim >= 2 and c.shape[0] == rgb.shape[0]:
        c = c.reshape((c.shape[0],) + (1,) * (rgb.ndim - 2) + (3,))
    else:
        raise ValueError(f"codes must be (3,) or one (dhq, dsq, dvq) row per tile, not of shape {c.shape}")
    dh, ds, dv = c[..., 0], c[..., 1], c[..., 2]
    x = rgb.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    M = np.maximum(np.maximum(r, g), b)
    m = np.minimum(np.minimum(r, g), b)
    C = M - m
    is_b, is_g = M == b, M == g
    base = np.where(is_b, 4, np.where(is_g, 2, 0))
    num = np.where(is_b, r - g, np.where(is_g, b - r, g - b))
    Cs = np.maximum(C, 1)
    hq = np.where(C == 0, 0, (base * Q + _rdiv((num + C) * Q, Cs) - Q) % (6 * Q))
    s = np.where(M == 0, 0, _rdiv(C * Q, np.maximum(M, 1)))
    v = _rdiv(M * Q, 255)
    hq = (hq + dh) % (6 * Q)
    s = _scale(s, ds)
    v = _scale(v, dv)
    hi = hq // Q
    fq = hq - hi * Q
    p = _rnd(v * (Q - s))
    q = _rnd(v * (Q - _rnd(fq * s)))
    t = _rnd(v * (Q - _rnd((Q - fq) * s)))
    R = np.choose(hi, [v, q, p, p, t, v])
    G = np.choose(hi, [t, v, v, q, p, p])
    B = np.choose(hi, [p, p, t, v, v, q])
    out = np.stack([R, G, B], axis=-1)
    return ((out * 255 + Q // 2) >> 15).astype(np.uint8)


_NAMES = ("Hue Sigma", "Saturation Sigma", "Brightness Sigma")


class HsbColorAugmenter(ColorAugmenterBase):
    """Colour perturbation in hue / saturation / brightness: the hue turned by sigma_h (in turns), saturation and brightness moved by
    x (1 + sigma) for sigma < 0 and x (1 + (1 - x) sigma) otherwise, in the integer definition of this module.  Each range is None or
    (lo, hi) within [-1, 1].  randomize() draws hue, then saturation, then brightness from the GLOBAL numpy stream (a None range draws
    nothing and gives 0); until then the lower bounds apply, as in the HED family."""

    def __init__(self, hue_sigma_range, saturation_sigma_range, brightness_sigma_range):
        super().__init__(keyword="hsb_color")
        rngs = (hue_sigma_range, saturation_sigma_range, brightness_sigma_range)
        self._sigma_ranges = [_checked(name, r, -1.0) for name, r in zip(_NAMES, rngs)]
        self._sigmas = [float(r[0]) if r is not None else 0.0 for r in self._sigma_ranges]

    def randomize(self):
        """Up to three draws from the global numpy stream: hue, saturation, brightness."""
        self._sigmas = [float(np.random.uniform(low=r[0], high=r[1], size=None)) if r is not None else 0.0 for r in self._sigma_ranges]

    def randomize_batch(self, n):
        """n successive randomize() calls (same global stream order) -> (n, 3) float64 sigmas."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        s = np.empty((n, 3), dtype=np.float64)
        for t in range(n):
            self.randomize()
            s[t] = self._sigmas
        return s

    def transform(self, patch):
        """(H, W, 3) uint8 ndarray -> (H, W, 3) uint8 ndarray under the augmenter's current sigmas."""
        from .. import engine
        if not is_uint8_image(patch):
            raise TypeError("HsbColorAugmenter.transform expects a uint8 (H, W, 3) ndarray")
        out = engine.hsb_augment(_to_device(patch), hsb_codes([self._sigmas]))
        return out[0].cpu().numpy()

    def transform_batch(self, tiles, sigmas=None, out=None, tensor_format=None, view=None, windows=None):
        """Batched: (N,H,W,3) uint8 device tensor, per-tile (N, 3) sigmas (default: the augmenter's current ones for every tile) ->
        (out, codes): the (N,H,W,3) uint8 image -- or, with ``tensor_format``, the (N,3,H,W) tensor, written directly -- and the (N, 3)
        int32 codes used.
        ``view``: a ``stainlib_amd.TileView`` (crop / flip / rot90, ``shrink=``, ``scale=``) -- per tile only the window ``windows[t]``
        (default: ``view.draw(N, H, W)``) of that result, in ONE pass (engine.normalize_hsb_view): bit for bit
        ``tensor_format.convert(transform_batch(tiles, sigmas)[0], view=view, windows=windows)``.  Returns (out, codes, windows)."""
        from .. import engine
        if view is not None or windows is not None:
            engine._view_call(view, windows, tiles, draw=False)
        if sigmas is None:
            n = int(tiles.shape[0]) if hasattr(tiles, "shape") and len(tiles.shape) == 4 else 1
            sigmas = [self._sigmas] * n
        engine._hsb_call(self, sigmas, tiles, view)
        engine._check_tiles(tiles)
        codes = hsb_codes(sigmas)
        if view is not None:
            x, windows, draw = engine.hsb_stage(tiles, self, sigmas, view, windows, {}, fmt=tensor_format, out=out)
            return x, draw.codes, windows
        return engine.hsb_augment(tiles, codes, fmt=tensor_format, out=out), codes


class HsbLightColorAugmenter(HsbColorAugmenter):
    def __init__(self):
        super().__init__((-0.1, 0.1), (-0.1, 0.1), None)


class HsbStrongColorAugmenter(HsbColorAugmenter):
    def __init__(self):
        super().__init__((-1, 1), (-1, 1), None)

"""Additive Gaussian noise and tone curves (brightness / contrast / gamma): the last two items of the usual histopathology augmentation
set (Tellez et al., HoVer-Net), an extension.  Both are pointwise maps on bytes, defined in INTEGERS so that every route computes the
same bits, and both act on the OUTPUT of a call -- behind the view, the box shrink or the area resample, in front of the tensor
conversion: a sigma means what it says at the resolution the network sees.

The definition (post_reference: numpy; csrc/post_math.hpp: the same in 32 bits, host and device).  The post stage acts on a uint8 image
(N, oh, ow, 3); for one tile, pixel p = i * ow + j, channel c, byte b:

    tone    b1 = table[b]: one table of 256 bytes per tile, the same for the three channels.  arange(256) is the identity; any 256 bytes
            are a table.  tone_table(brightness, contrast, gamma), in binary64: x = v / 255,
            y = clip((x ** gamma - 0.5) * contrast + 0.5 + brightness, 0, 1), table[v] = floor(255 y + 1/2).  The TABLE is the contract
            between host and device, not the float expression: a call returns the tables it used.
    noise   four int32 codes per tile, (sq, k0, k1, mono); k0 and k1 are the bit patterns of two uint32.
            W = philox4x32_10(counter=(p, 0, 0, 0), key=(k0, k1)), the published Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
            constants 0x9E3779B9, 0xBB67AE85; ten rounds, the key bumped between rounds).  Channel c takes the word W[c], or W[3] for all
            three channels when mono != 0.  G = (the sum of the word's four bytes) - 510: in [-510, 510], mean 0, variance exactly 21845
            -- a four-fold Irwin-Hall sum: bell-shaped, NOT a Gaussian, its tails are cut at 510 / sqrt(21845) = 3.45 sigma.
            n = (G * sq + 32768) >> 16 (an arithmetic shift), b2 = clamp(b1 + n, 0, 255).
            sq = floor(sigma * 65536 / sqrt(21845) + 1/2) with sigma in bytes, 0 <= sigma <= 64, so sq <= SQ_MAX = 28378 and |G sq| < 2^24.
            sq = 0 is the identity on every byte.  Codes outside [0, SQ_MAX] are clamped (reduce_codes), as the kernels do it.

The order is tone, then noise.  A tile's noise depends on its key and on p, never on its position in the batch.  The per-pixel noise is
generated on the device; the per-tile parameters (sigma, key, brightness, contrast, gamma) are drawn on the host.
"""
from __future__ import annotations

import math

import numpy as np

from ..utils.excepts import InvalidRangeError
from ..utils.stain_utils import is_uint8_image
from .augmenter import AugmenterBase, ColorAugmenterBase

VAR_G = 21845                                    # the variance of G: 4 * (256^2 - 1) / 12
SIGMA_MAX = 64.0
SQ_MAX = 28378                                   # floor(64 * 65536 / sqrt(21845) + 1/2)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10: counter (..., 4) and key (2,) of uint32 values -> (..., 4) uint32.  uint64 products masked to 32 bits."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = [np.uint64(int(v) & 0xFFFFFFFF) for v in np.asarray(key).reshape(2).tolist()]
    if c.shape[-1] != 4:
        raise ValueError("counter must hold four uint32 words along its last axis")
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    for r in range(10):
        k0 = np.uint64((int(k[0]) + r * _W0) & 0xFFFFFFFF)
        k1 = np.uint64((int(k[1]) + r * _W1) & 0xFFFFFFFF)
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def noise_sq(sigmas):
    """sq = floor(sigma * 65536 / sqrt(21845) + 1/2) of sigmas in bytes, 0 <= sigma <= 64 (ValueError; NaN included) -> int32, same shape."""
    try:
        s = np.asarray(sigmas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("noise sigmas must be numbers in [0, 64] (bytes)") from None
    if not (np.isfinite(s).all() and (s >= 0.0).all() and (s <= SIGMA_MAX).all()):
        raise ValueError("a noise sigma must lie in [0, 64] (bytes)")
    return np.floor(s * 65536.0 / math.sqrt(VAR_G) + 0.5).astype(np.int32)


def noise_codes(sigmas, keys=(0, 0), mono=False):
    """The (N, 4) int32 codes (sq, k0, k1, mono) of (N,) sigmas in bytes (a scalar: one row): keys is one (k0, k1) pair for every tile or
    an (N, 2) array of uint32 values, stored as their int32 bit patterns.  ValueError for sigmas outside [0, 64], NaN included."""
    sq = np.atleast_1d(noise_sq(sigmas))
    if sq.ndim != 1:
        raise ValueError(f"noise sigmas must hold one sigma per tile: an (N,) array, not one of shape {sq.shape}")
    try:
        k = np.asarray(keys).astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError("keys must hold (k0, k1) uint32 pairs") from None
    if k.shape == (2,):
        k = np.tile(k, (sq.shape[0], 1))
    if k.shape != (sq.shape[0], 2) or (k < -2 ** 31).any() or (k >= 2 ** 32).any():
        raise ValueError("keys must be one (k0, k1) pair of uint32 values, or one pair per tile")
    out = np.empty((sq.shape[0], 4), dtype=np.int32)
    out[:, 0] = sq
    out[:, 1:3] = (k & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    out[:, 3] = 1 if mono else 0
    return out


def reduce_codes(codes):
    """Codes of any int32 values as the kernels take them: sq clamped to [0, SQ_MAX], mono to 0 / 1; the key words stay."""
    c = np.asarray(codes).astype(np.int64).copy()
    c[..., 0] = np.clip(c[..., 0], 0, SQ_MAX)
    c[..., 3] = c[..., 3] != 0
    return c


def tone_table(brightness=0.0, contrast=1.0, gamma=1.0):
    """The 256-byte table of a tone curve, in binary64: scalars -> (256,) uint8, (N,) arrays -> (N, 256).  brightness in [-1, 1], contrast
    in [0, 4], gamma in [0.25, 4] (ValueError).  (0, 1, 1) is arange(256) exactly."""
    try:
        b, c, g = (np.asarray(v, dtype=np.float64) for v in (brightness, contrast, gamma))
    except (TypeError, ValueError):
        raise ValueError("brightness, contrast and gamma must be numbers") from None
    if not (np.isfinite(b).all() and np.isfinite(c).all() and np.isfinite(g).all()):
        raise ValueError("brightness, contrast and gamma must be finite")
    if (np.abs(b) > 1.0).any() or (c < 0.0).any() or (c > 4.0).any() or (g < 0.25).any() or (g > 4.0).any():
        raise ValueError("brightness must lie in [-1, 1], contrast in [0, 4] and gamma in [0.25, 4]")
    x = np.arange(256, dtype=np.float64) / 255.0
    y = np.clip((x ** g[..., None] - 0.5) * c[..., None] + 0.5 + b[..., None], 0.0, 1.0)
    return np.floor(255.0 * y + 0.5).astype(np.uint8)


assert np.array_equal(tone_table(0.0, 1.0, 1.0), np.arange(256)), "the neutral tone curve must be the identity table"


def tone_tables(params):
    """(N, 3) rows (brightness, contrast, gamma) -> (N, 256) uint8 tables.  ValueError for a wrong shape or range."""
    try:
        p = np.asarray(params, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("tone params must hold (brightness, contrast, gamma) per tile: an (N, 3) array") from None
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"tone params must hold (brightness, contrast, gamma) per tile: an (N, 3) array, not one of shape {p.shape}")
    return tone_table(p[:, 0], p[:, 1], p[:, 2]).reshape(p.shape[0], 256)


def post_reference(u8, tables=None, codes=None):
    """The definition in numpy: `u8` (oh, ow, 3) uint8 with one table (256,) and / or one code row (4,), or (N, oh, ow, 3) with tables
    (N, 256) and / or codes (N, 4) -> uint8 of the same shape.  None: that half of the stage is absent.  Codes are reduced first."""
    img = np.asarray(u8)
    if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("post_reference expects a uint8 (oh, ow, 3) or (N, oh, ow, 3) array")
    single = img.ndim == 3
    x = img[None] if single else img
    n, oh, ow = x.shape[:3]
    if tables is not None:
        t = np.asarray(tables)
        t = t[None] if single and t.ndim == 1 else t
        if t.dtype != np.uint8 or t.shape != (n, 256):
            raise ValueError("tables must be uint8, 256 bytes per tile")
    if codes is not None:
        c = np.asarray(codes)
        c = c[None] if single and c.ndim == 1 else c
        if c.dtype.kind not in "iu" or c.shape != (n, 4):
            raise ValueError("codes must hold (sq, k0, k1, mono) per tile: four integers")
        c = reduce_codes(c)
    out = np.empty_like(x)
    ctr = np.zeros((oh * ow, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(oh * ow, dtype=np.uint64)
    for i in range(n):
        v = x[i].reshape(oh * ow, 3)
        if tables is not None:
            v = t[i][v]
        if codes is not None and c[i, 0] != 0:
            W = philox4x32_10(ctr, (c[i, 1], c[i, 2])).astype(np.int64)
            G = (W & 0xFF) + ((W >> 8) & 0xFF) + ((W >> 16) & 0xFF) + (W >> 24) - 510
            G = np.repeat(G[:, 3:4], 3, axis=1) if c[i, 3] else G[:, :3]
            v = np.clip(v.astype(np.int64) + ((G * c[i, 0] + 32768) >> 16), 0, 255)
        out[i] = v.astype(np.uint8).reshape(oh, ow, 3)
    return out[0] if single else out


def _batch_n(tiles):
    return int(tiles.shape[0]) if hasattr(tiles, "shape") and len(tiles.shape) == 4 else 1


def _post_transform_batch(noise, tone, arg, tiles, out, tensor_format, view, windows):
    """transform_batch of the two augmenters: the raw route of engine.normalize_post_view with one of the two halves."""
    from .. import engine
    if view is not None or windows is not None:
        engine._view_call(view, windows, tiles, draw=False)
    engine._post_call(noise, tone, arg if noise is not None else None, arg if tone is not None else None, tiles, view)
    engine._check_tiles(tiles)
    x, windows, draw = engine.post_stage(tiles, noise, tone, arg if noise is not None else None, arg if tone is not None else None, view,
                                         windows, {}, fmt=tensor_format, out=out)
    used = draw.noise_codes if noise is not None else draw.tone_tables
    return (x, used, windows) if view is not None else (x, used)


class GaussianNoiseAugmenter(AugmenterBase):
    """Additive noise of a random sigma in sigma_range = (lo, hi), in bytes, 0 <= lo <= hi <= 64 (InvalidRangeError), in the integer
    definition of this module: per pixel a four-fold Irwin-Hall value from Philox4x32-10 -- bell-shaped, tails cut at 3.45 sigma --,
    per channel (per_channel=True) or one value for the three channels.  randomize() draws from the GLOBAL numpy stream the sigma
    (uniform) and then the two key words (np.random.randint(0, 2**32, dtype=np.uint32) each); until then the lower bound and the key
    (0, 0) apply."""

    def __init__(self, sigma_range, per_channel=True):
        super().__init__(keyword="gaussian_noise")
        try:
            bad = len(sigma_range) != 2 or not (0.0 <= sigma_range[0] <= sigma_range[1] <= SIGMA_MAX)
        except TypeError:
            bad = True
        if bad:
            raise InvalidRangeError("Noise Sigma", sigma_range)
        self._sigma_range = (float(sigma_range[0]), float(sigma_range[1]))
        self._per_channel = bool(per_channel)
        self._sigma = self._sigma_range[0]
        self._key = (0, 0)

    def randomize(self):
        """Three draws from the global numpy stream: the sigma, then the two key words."""
        self._sigma = float(np.random.uniform(low=self._sigma_range[0], high=self._sigma_range[1], size=None))
        k0 = int(np.random.randint(0, 2 ** 32, dtype=np.uint32))
        k1 = int(np.random.randint(0, 2 ** 32, dtype=np.uint32))
        self._key = (k0, k1)

    def codes(self, sigmas=None, keys=None):
        """noise_codes under this augmenter's channel mode; by default its current sigma and key (one row)."""
        return noise_codes(self._sigma if sigmas is None else sigmas, self._key if keys is None else keys, mono=not self._per_channel)

    def randomize_batch(self, n):
        """n successive randomize() calls (same global stream order) -> ((n,) float64 sigmas, (n, 4) int32 codes)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        s = np.empty((n,), dtype=np.float64)
        keys = np.zeros((n, 2), dtype=np.int64)
        for t in range(n):
            self.randomize()
            s[t] = self._sigma
            keys[t] = self._key
        return s, self.codes(s, keys)

    def transform(self, patch):
        """(H, W, 3) uint8 ndarray -> (H, W, 3) uint8 ndarray under the augmenter's current sigma and key: numpy to numpy."""
        if not is_uint8_image(patch):
            raise TypeError("GaussianNoiseAugmenter.transform expects a uint8 (H, W, 3) ndarray")
        return post_reference(patch, codes=self.codes()[0])

    def transform_batch(self, tiles, sigmas=None, out=None, tensor_format=None, view=None, windows=None):
        """Batched, behind any uint8 result: (N,H,W,3) uint8 device tensor, per-tile (N,) sigmas under the augmenter's current key
        (default: its current sigma for every tile) -- or the (N, 4) int32 codes a call returned, which reproduce it -> (out, codes): the
        uint8 image, or with ``tensor_format`` the tensor, written directly, and the (N, 4) codes used.
        ``view``: a ``stainlib_amd.TileView`` (crop / flip / rot90, ``shrink=``, ``scale=``) -- the noise on the OUTPUT pixels of the view,
        in ONE pass (engine.normalize_post_view).  Returns (out, codes, windows)."""
        if sigmas is None:
            sigmas = [self._sigma] * _batch_n(tiles)
        return _post_transform_batch(self, None, sigmas, tiles, out, tensor_format, view, windows)


_TONE = (("Brightness", -1.0, 1.0, 0.0), ("Contrast", 0.0, 4.0, 1.0), ("Gamma", 0.25, 4.0, 1.0))


class ToneCurveAugmenter(ColorAugmenterBase):
    """Brightness / contrast / gamma as one 256-byte table per tile (tone_table).  Each range is None or (lo, hi): brightness within
    [-1, 1], contrast within [0, 4], gamma within [0.25, 4] (InvalidRangeError).  randomize() draws brightness and contrast uniformly and
    gamma log-uniformly (exp(uniform(log lo, log hi))) from the GLOBAL numpy stream; a None range draws nothing and gives the neutral
    value (0, 1, 1); until then the lower bounds apply."""

    def __init__(self, brightness_range=None, contrast_range=None, gamma_range=None):
        super().__init__(keyword="tone_curve")
        self._ranges = []
        for (name, lowest, highest, _), rng in zip(_TONE, (brightness_range, contrast_range, gamma_range)):
            if rng is not None:
                try:
                    bad = len(rng) != 2 or not (lowest <= rng[0] <= rng[1] <= highest)
                except TypeError:
                    bad = True
                if bad:
                    raise InvalidRangeError(name, rng)
                rng = (float(rng[0]), float(rng[1]))
            self._ranges.append(rng)
        self._params = [r[0] if r is not None else t[3] for r, t in zip(self._ranges, _TONE)]

    def randomize(self):
        """Up to three draws from the global numpy stream: brightness, contrast, gamma."""
        p = []
        for i, r in enumerate(self._ranges):
            if r is None:
                p.append(_TONE[i][3])
            elif i < 2:
                p.append(float(np.random.uniform(low=r[0], high=r[1], size=None)))
            else:
                p.append(min(max(float(np.exp(np.random.uniform(low=math.log(r[0]), high=math.log(r[1]), size=None))), r[0]), r[1]))
        self._params = p

    def randomize_batch(self, n):
        """n successive randomize() calls (same global stream order) -> ((n, 3) float64 params, (n, 256) uint8 tables)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        p = np.empty((n, 3), dtype=np.float64)
        for t in range(n):
            self.randomize()
            p[t] = self._params
        return p, tone_tables(p)

    def transform(self, patch):
        """(H, W, 3) uint8 ndarray -> (H, W, 3) uint8 ndarray under the augmenter's current parameters: numpy to numpy."""
        if not is_uint8_image(patch):
            raise TypeError("ToneCurveAugmenter.transform expects a uint8 (H, W, 3) ndarray")
        return post_reference(patch, tables=tone_table(*self._params))

    def transform_batch(self, tiles, params=None, out=None, tensor_format=None, view=None, windows=None):
        """Batched, behind any uint8 result: (N,H,W,3) uint8 device tensor, per-tile (N, 3) params (default: the augmenter's current
        ones for every tile) -- or the (N, 256) uint8 tables a call returned, which reproduce it -> (out, tables): the uint8 image, or with
        ``tensor_format`` the tensor, written directly, and the (N, 256) tables used.
        ``view``: a ``stainlib_amd.TileView`` -- the curve on the OUTPUT pixels of the view, in ONE pass (engine.normalize_post_view).
        Returns (out, tables, windows)."""
        if params is None:
            params = [self._params] * _batch_n(tiles)
        return _post_transform_batch(None, self, params, tiles, out, tensor_format, view, windows)

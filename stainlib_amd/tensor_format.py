"""TensorFormat: the model-ready output of the batched operators (an extension; the reference ends with a uint8 image).

A network wants its tiles as a float tensor, usually planar, scaled to [0, 1] and shifted / scaled per channel.  Passing a
``TensorFormat`` as ``tensor_format=`` to a ``transform_batch`` / ``transform_shard`` returns that tensor instead of the
``(N, H, W, 3)`` uint8 one -- computed by the library's kernels, where it pays inside the apply pass itself -- and
``TensorFormat.convert`` does the same for any uint8 result.

One definition everywhere: for a result byte ``b`` (the truncated uint8 the library produces without a format) of channel ``c``

    scale32[c] = float32(1.0 / (255.0 * std[c]))          binary64, rounded once
    shift32[c] = float32(-mean[c] / std[c])
    v          = fma(float32(b), scale32[c], shift32[c])   one fused multiply-add: one binary32 rounding
    out        = v converted to ``dtype``, round-to-nearest-even

so ``op(..., tensor_format=f)`` equals ``f.convert(op(...))`` bit for bit, and both are within a few binary32 roundings of
``((x.permute(0, 3, 1, 2).float() / 255) - mean[:, None, None]) / std[:, None, None]``.
"""
from __future__ import annotations

import math

_DTYPE_NAMES = ("float32", "float16", "bfloat16")


class TensorFormat(object):
    """dtype: torch.float32 (default), torch.float16 or torch.bfloat16 (or their names).  channels_last: the returned tensor has the
    logical shape (N, 3, H, W) either way, in contiguous (planar, False) or channels_last (interleaved, True) memory format.
    mean, std: three values each, in units of [0, 1] (the ImageNet constants are mean=(0.485, 0.456, 0.406),
    std=(0.229, 0.224, 0.225)); the means finite, the stds finite and > 0.  Anything else raises ValueError."""

    def __init__(self, dtype=None, channels_last=False, mean=(0, 0, 0), std=(1, 1, 1)):
        import torch
        if dtype is None:
            dtype = torch.float32
        if isinstance(dtype, str):
            if dtype not in _DTYPE_NAMES:
                raise ValueError(f"dtype must be one of torch.float32, torch.float16, torch.bfloat16, not {dtype!r}")
            dtype = getattr(torch, dtype)
        if not any(dtype is getattr(torch, name) for name in _DTYPE_NAMES):
            raise ValueError(f"dtype must be one of torch.float32, torch.float16, torch.bfloat16, not {dtype!r}")
        self.dtype = dtype
        self.channels_last = bool(channels_last)
        self.mean = self._three(mean, "mean")
        self.std = self._three(std, "std")
        if not all(s > 0 for s in self.std):
            raise ValueError(f"std must be three values > 0, not {std!r}")

    @staticmethod
    def _three(x, what):
        try:
            v = tuple(float(t) for t in x)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be three finite numbers, not {x!r}") from None
        if len(v) != 3 or not all(math.isfinite(t) for t in v):
            raise ValueError(f"{what} must be three finite numbers, not {x!r}")
        return v

    def convert(self, tiles_u8, out=None, view=None, windows=None, blur=None, blur_sigmas=None, noise=None, tone=None, noise_sigmas=None,
                tone_params=None, recipe=None, recipe_draw=None):
        """(N, H, W, 3) uint8 device tensor -> (N, 3, H, W) tensor in this format (one streaming sweep, engine.to_tensor).
        ``out``: a tensor of that shape, dtype and memory format to write into.
        ``view``: a ``stainlib_amd.TileView`` -- per tile only the window ``windows[t]`` (default: ``view.draw(N, H, W)``), flipped and
        turned, converted in the same sweep (engine.normalize_view): the crop / flip / rot90 behind ANY uint8 result (Reinhard, HED,
        luminosity ...).  Returns (the (N, 3, oh, ow) tensor, windows).
        ``blur``: a ``stainlib_amd.GaussianBlurAugmenter`` -- its integer Gaussian blur of every WHOLE tile in the same sweep
        (engine.normalize_blur_view), then the view (if any) and the conversion.  ``blur_sigmas``: (N,); by default
        ``blur.randomize_batch(N)``, drawn BEFORE the windows.  One more element at the end, ``engine.BlurDraw(sigmas, codes)``: the call
        returns (tensor, BlurDraw) or (tensor, windows, BlurDraw).  Not with a ``TileView(scale=)`` or a TileAffine.
        ``noise``, ``tone``: a ``stainlib_amd.GaussianNoiseAugmenter`` / ``ToneCurveAugmenter`` -- the post stage in the same sweep
        (engine.normalize_post_view): the tone curve, then the additive noise, per WRITTEN pixel -- behind the view (if any), in front of
        the conversion: bit for bit this call on ``augmentation.noise.post_reference`` of the uint8 view.  ``tone_params``: (N, 3),
        ``noise_sigmas``: (N,) -- or the tables / codes a call returned; by default ``tone.randomize_batch(N)``, then
        ``noise.randomize_batch(N)``, drawn BEFORE the windows.  One more element at the end, ``engine.PostDraw``.  Not with ``blur``, a
        TileAffine or a TileElastic.
        ``recipe``: a ``stainlib_amd.Recipe(view=, color=, noise=, tone=)`` -- a colour stage (HED or HSB) on the SOURCE pixels, a view of
        any kind and tone / noise on the WRITTEN pixels TOGETHER in the same sweep (engine.recipe_stage), drawn in the order colour,
        tone, noise, view.  Returns (tensor, ``engine.RecipeDraw(windows, color, post)``); ``recipe_draw``, that RecipeDraw passed back,
        reproduces the call.  Not together with any other keyword from ``view`` on."""
        from . import engine
        if engine._recipe_call(recipe, recipe_draw, tiles_u8, view=view, windows=windows, blur=blur, blur_sigmas=blur_sigmas, noise=noise,
                               tone=tone, noise_sigmas=noise_sigmas, tone_params=tone_params):
            engine._check_tiles(tiles_u8)
            return engine.recipe_stage(tiles_u8, recipe, recipe_draw, {}, fmt=self, out=out)
        if engine._post_call(noise, tone, noise_sigmas, tone_params, tiles_u8, view, blur=blur):
            if view is not None or windows is not None:
                engine._view_call(view, windows, tiles_u8, draw=False)
            engine._check_tiles(tiles_u8)
            x, windows, draw = engine.post_stage(tiles_u8, noise, tone, noise_sigmas, tone_params, view, windows, {}, fmt=self, out=out)
            return (x,) + ((windows,) if view is not None else ()) + (draw,)
        if engine._blur_call(blur, blur_sigmas, tiles_u8, view):
            if view is not None or windows is not None:
                engine._view_call(view, windows, tiles_u8, draw=False)
            engine._check_tiles(tiles_u8)
            x, windows, draw = engine.blur_stage(tiles_u8, blur, blur_sigmas, view, windows, {}, fmt=self, out=out)
            return (x,) + ((windows,) if view is not None else ()) + (draw,)
        if view is not None or windows is not None:
            return engine.view_pass(tiles_u8, view, windows, fmt=self, out=out)
        return engine.to_tensor(tiles_u8, self, out=out)

    def __repr__(self):
        return f"TensorFormat(dtype={self.dtype}, channels_last={self.channels_last}, mean={self.mean}, std={self.std})"

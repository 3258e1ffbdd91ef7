"""ExtractiveStainNormalizer (stainlib/normalization/normalizer.py:16-50) on the HIP engine.

Drop-in contract: ``fit(target)`` / ``transform(I)`` take and return numpy uint8 HWC images and set
``stain_matrix_target`` (2,3), ``maxC_target`` (1,2) and ``target_concentrations`` (P,2) exactly
like the reference.  Extension: ``transform_batch`` takes an (N,H,W,3) uint8 device tensor and
keeps everything in HBM -- that is the path bench.py measures.
"""
from __future__ import annotations

import warnings

import numpy as np

from ..utils.stain_utils import _UINT8_MSG, _to_device, get_concentrations, is_uint8_image, raise_for_status

_METHODS = ("macenko", "vahadane")
# A single image of this many pixels or more is not handled as ONE tile (whose finish steps run on one workgroup and
# grow with the tile) but as the vertical concatenation of its row bands: the pooled slide statistics are, by
# definition, the reference's statistics of that concatenation, i.e. of the image itself -- computed with chip-wide
# sweeps only (8192 x 8192: 1.9 instead of 4.9 ms).  The two paths agree to the rounding of the binary32 burst sums of the
# moments (stain matrix ~1e-7, maxC ~1e-6 relative: tests/test_gpu_macenko.py::test_large_single_image_goes_through_the_pooled_statistics),
# so results step by that much at this size; both are within 2e-6 of the reference.  The pooled path is
# host-driven (~1.3 ms whatever the size), so it only pays from the measured crossover on (tools/big_image.py:
# 4096^2 1.27 vs 1.58 ms, 6144^2 3.4 vs 1.9 ms).
BIG_IMAGE_PIXELS = 5 << 22        # ~21 Mpx
# transform_batch(tensor_format=...): "fused" = *_fit, then sl_normalize_apply_tensor; "convert" = *_transform into a uint8 scratch, then
# sl_to_tensor.  Both give the same bits (tests/test_gpu_tensor_format.py).  NOT MEASURED yet (tools/tensor_format_time.py decides it at
# 512 x 1024^2): "fused" on the byte count alone -- it saves the 3 B/px write and re-read of the scratch.
TENSOR_ROUTE = "fused"


def _row_bands(dev_img):
    """(1, H, W, 3) device image -> (H/r, r, W, 3) view, r = the largest divisor of H with r * W <= 2**20 (or 1)."""
    _, H, W, _ = dev_img.shape
    r = 1
    for cand in range(1, H + 1):
        if H % cand == 0 and cand * W <= (1 << 20):
            r = cand
    return dev_img.view(H // r, r, W, 3)


class ExtractiveStainNormalizer(object):
    def __init__(self, method):
        name = method.lower()
        if name not in _METHODS:
            raise Exception('Method not recognized.')                      # normalizer.py:25
        self.method = name
        if name == "macenko":
            from ..extraction.macenko_stain_extractor import MacenkoStainExtractor
            self.extractor = MacenkoStainExtractor
        else:
            from ..extraction.vahadane_stain_extractor import VahadaneStainExtractor
            self.extractor = VahadaneStainExtractor
        self._target = None
        self._target_concentrations = None

    # -- engine entry points of this method ------------------------------------------------------
    def _fit_tiles(self, tiles, ws=None):
        from .. import engine
        if self.method == "macenko":
            return engine.macenko_fit(tiles, ws=ws)
        M, maxC, status, _ = engine.vahadane_fit(tiles, ws=ws)
        return M, maxC, status

    def _target_on(self, device):
        """The 8 target doubles as device tensors, uploaded once per fit: as numpy arguments they are a small pageable
        copy per call, which queues behind any large upload in flight (see pipeline.py)."""
        import torch
        key = (str(device), np.asarray(self.stain_matrix_target, dtype=np.float64).tobytes(),
               np.asarray(self.maxC_target, dtype=np.float64).tobytes())        # by value: the attributes are public
        if getattr(self, "_target_dev_key", None) != key:
            self._target_dev = (torch.as_tensor(np.asarray(self.stain_matrix_target, dtype=np.float64), device=device).reshape(2, 3).contiguous(),
                                torch.as_tensor(np.asarray(self.maxC_target, dtype=np.float64), device=device).reshape(2).contiguous())
            self._target_dev_key = key
        return self._target_dev

    def _transform_tiles(self, tiles, out=None, ws=None):
        from .. import engine
        fn = engine.macenko_transform if self.method == "macenko" else engine.vahadane_transform
        M_t, c_t = self._target_on(tiles.device)
        return fn(tiles, M_t, c_t, out=out, ws=ws)

    def _big_image_statistics(self, dev):
        """(M (2,3), maxC (2,)) of one large image through the pooled statistics, or None when that path does not apply
        (Vahadane; degenerate images, which the per-tile path reports through its status codes)."""
        if self.method != "macenko" or dev.shape[1] * dev.shape[2] < BIG_IMAGE_PIXELS:
            return None
        from ..distributed import PooledSlideStatistics
        from ..utils.excepts import TissueMaskException
        try:
            M, maxC = PooledSlideStatistics(group=False)(_row_bands(dev))
        except (TissueMaskException, ValueError):
            return None
        if not (np.isfinite(M).all() and np.isfinite(maxC).all() and (maxC > 0).all()):
            return None
        G = M @ M.T
        if not (G[0, 0] * G[1, 1] - G[0, 1] ** 2 > 1e-8 * G[0, 0] * G[1, 1]):     # parallel stain vectors: the per-tile path reports it (status 2)
            return None
        return M, maxC

    # -- reference API -----------------------------------------------------------------------------
    def fit(self, target):
        """Fit to a target image (RGB uint8), normalizer.py:27-36."""
        assert is_uint8_image(target), _UINT8_MSG
        dev = _to_device(target)
        big = self._big_image_statistics(dev)
        if big is not None:
            self.stain_matrix_target, self.maxC_target = big[0], big[1].reshape((1, 2))
            self._target = target.copy()
            self._target_concentrations = None
            return
        M, maxC, status = self._fit_tiles(dev)
        raise_for_status(int(status[0]))
        self.stain_matrix_target = M[0].cpu().numpy()
        self.maxC_target = maxC[0].cpu().numpy().reshape((1, 2))
        self._target = target.copy()            # (the reference computes target_concentrations eagerly: later edits of the caller's array must not leak in)
        self._target_concentrations = None

    @property
    def target_concentrations(self):
        """(P, 2) concentrations of the target (normalizer.py:35); materialised on first use only --
        the reference stores this array but nothing reads it."""
        if self._target_concentrations is None and self._target is not None:
            self._target_concentrations = get_concentrations(self._target, self.stain_matrix_target)
        return self._target_concentrations

    def transform(self, I):
        """Transform an image (RGB uint8) to the fitted target's stain appearance, normalizer.py:39-50."""
        assert is_uint8_image(I), _UINT8_MSG
        dev = _to_device(I)
        big = self._big_image_statistics(dev)
        if big is not None:
            from .. import engine
            out = engine.normalize_apply(dev, big[0][None], big[1][None], self.stain_matrix_target, self.maxC_target.reshape(2))
            return out[0].cpu().numpy()
        out, _, _, status = self._transform_tiles(dev)
        st = int(status[0])
        raise_for_status(st)
        if st != 0:
            warnings.warn("99th-percentile concentration of the source is zero; the reference divides by it",
                          RuntimeWarning)
        return out[0].cpu().numpy()

    # -- batched extension -------------------------------------------------------------------------
    def fit_batch_targets(self, tiles, ws=None):
        """Per-tile (M, maxC, status) device tensors for a batch of candidate targets."""
        return self._fit_tiles(tiles, ws=ws)

    def _route_batch(self, tiles, target, jitter, out, ws, tensor_format, view, windows, hed, hsb=None, blur=None, post=None, recipe=None):
        """The view= / hed= routes of transform_batch and all of augment_batch: the checks that are left (every one before the fit and
        before any draw), the fit of the whole tiles, then engine.route_stage -- ONE pass under the target (target=True) or every tile's
        own matrix, with the jitter's alpha_beta / augment_background ({}: none).  hed: None, or (hed, hed_sigmas, hed_biases) that
        engine._hed_call has accepted; hsb: None, or (hsb, hsb_sigmas) that engine._hsb_call has accepted; blur: None, or (blur, blur_sigmas)
        that engine._blur_call has accepted; post: None, or (noise, tone, noise_sigmas, tone_params) that engine._post_call has accepted;
        recipe: None, or (Recipe, recipe_draw) that engine._recipe_call has accepted.
        -> (out, M_src, maxC_src, status[, windows][, HedDraw or HsbDraw or BlurDraw or PostDraw or RecipeDraw])."""
        from .. import engine
        if view is not None or windows is not None:
            engine._view_call(view, windows, tiles, draw=False)
        engine._check_tiles(tiles)
        fit = self._fit_tiles(tiles, ws=ws)
        M_t, c_t = self._target_on(tiles.device) if target else (None, None)
        return engine.route_stage(tiles, fit, dict(M_tgt=M_t, maxC_tgt=c_t, **jitter), tensor_format, out, view, windows, hed, hsb, blur, post,
                                  recipe)

    def transform_batch(self, tiles, out=None, ws=None, tensor_format=None, _tensor_route=None, view=None, windows=None, hed=None,
                        hed_sigmas=None, hed_biases=None, hsb=None, hsb_sigmas=None, blur=None, blur_sigmas=None, noise=None, tone=None, noise_sigmas=None, tone_params=None,
                        recipe=None, recipe_draw=None):
        """(N,H,W,3) uint8 device tensor -> (out, M_src, maxC_src, status) device tensors.  A tile whose
        status is non-zero (1 = empty tissue mask, 2 = degenerate, 3 = a zero 99th-percentile concentration) is passed through unchanged.
        ``ws``: an ``engine.Workspace`` to reuse (ONE stream at a time); by default every call takes its scratch from
        torch's stream-ordered caching allocator, so concurrent streams / threads never share it.
        ``tensor_format``: a ``stainlib_amd.TensorFormat``; `out` is then the (N,3,H,W) tensor in that format -- bit for bit
        ``tensor_format.convert`` of the uint8 result (a passed-through tile: of its source bytes).
        ``view``: a ``stainlib_amd.TileView`` -- the unchanged fit of the WHOLE tiles, then ONE pass that writes per tile only the window
        ``windows[t]`` (default: ``view.draw(N, H, W)``) of that result, flipped and turned (engine.normalize_view): `out` is
        (N,oh,ow,3) uint8 or the (N,3,oh,ow) tensor, and the call returns (out, M_src, maxC_src, status, windows).
        ``hed``: a ``HedColorAugmenter`` -- its transform (ranges, cutoff, skimage_mode) on every normalised tile in that same pass
        (engine.normalize_sums for its cutoff test on the image nobody writes, then engine.normalize_hed_view): bit for bit
        ``hed.transform_batch`` of the uint8 result, then the view and the conversion.  ``hed_sigmas``, ``hed_biases``: (N, 3) each; by
        default ``hed.randomize_batch(N)``, drawn BEFORE the windows.  Works with or without ``view`` / ``tensor_format``; the call then
        returns one more element at the end, ``engine.HedDraw(sigmas, biases, applied)``.
        ``hsb``: an ``HsbColorAugmenter`` -- its hue / saturation / brightness map on every normalised tile in that same pass
        (engine.normalize_hsb_view; no cutoff test, so nothing is read twice): bit for bit ``hsb.transform_batch`` of the uint8 result,
        then the view and the conversion.  ``hsb_sigmas``: (N, 3); by default ``hsb.randomize_batch(N)``, drawn BEFORE the windows.  The
        call then returns one more element at the end, ``engine.HsbDraw(sigmas, codes)``.  Not together with ``hed`` or a TileAffine.
        ``blur``: a ``GaussianBlurAugmenter`` -- its integer Gaussian blur of every normalised tile in that same pass
        (engine.normalize_blur_view): bit for bit ``blur.transform_batch`` of the uint8 result -- the blur of the WHOLE tile, so a window's
        edge sees the tile's real neighbours --, then the view and the conversion.  ``blur_sigmas``: (N,); by default
        ``blur.randomize_batch(N)``, drawn BEFORE the windows (or the (N, 9) codes a call returned, to reproduce it).  The call then returns
        one more element at the end, ``engine.BlurDraw(sigmas, codes)``.  Not together with ``hed`` or ``hsb`` (chain them), a
        ``TileView(scale=)`` or a TileAffine.
        ``noise``, ``tone``: a ``GaussianNoiseAugmenter`` / a ``ToneCurveAugmenter`` -- the post stage, in that same pass
        (engine.normalize_post_view): the tone curve, then the additive noise, per WRITTEN pixel -- behind the view, the box shrink or the
        area resample, in front of the conversion: bit for bit ``augmentation.noise.post_reference`` of the uint8 image the call writes
        without them.  ``tone_params``: (N, 3) (brightness, contrast, gamma), ``noise_sigmas``: (N,) in bytes -- or the tables / codes a
        call returned, to reproduce it; by default ``tone.randomize_batch(N)``, then ``noise.randomize_batch(N)``, drawn BEFORE the
        windows.  One more element at the end, ``engine.PostDraw(tone_params, tone_tables, noise_sigmas, noise_codes)``.  Not together
        with ``hed``, ``hsb`` or ``blur`` (chain them), a TileAffine or a TileElastic.
        ``recipe``: a ``stainlib_amd.Recipe(view=, color=, noise=, tone=)`` -- a colour stage (HED or HSB) on the normalised SOURCE pixels, a
        view of any kind and tone / noise on the WRITTEN pixels TOGETHER in that one pass (engine.recipe_stage): bit for bit the chain
        of the calls above.  The draws: ``color.randomize_batch(N)``, ``tone.randomize_batch(N)``, ``noise.randomize_batch(N)``,
        ``view.draw(N, H, W)``, in this order.  The call returns (out, M_src, maxC_src, status, ``engine.RecipeDraw(windows, color,
        post)``); ``recipe_draw``: that RecipeDraw passed back reproduces the call.  Not together with any other keyword above from
        ``view`` on."""
        from .. import engine
        if engine._recipe_call(recipe, recipe_draw, tiles, view=view, windows=windows, hed=hed, hed_sigmas=hed_sigmas, hed_biases=hed_biases,
                               hsb=hsb, hsb_sigmas=hsb_sigmas, blur=blur, blur_sigmas=blur_sigmas, noise=noise, tone=tone,
                               noise_sigmas=noise_sigmas, tone_params=tone_params):
            return self._route_batch(tiles, True, {}, out, ws, tensor_format, None, None, None, recipe=(recipe, recipe_draw))
        with_hed = engine._hed_call(hed, hed_sigmas, hed_biases, tiles, view)
        with_hsb = engine._hsb_call(hsb, hsb_sigmas, tiles, view, hed)
        with_blur = engine._blur_call(blur, blur_sigmas, tiles, view, hed, hsb)
        with_post = engine._post_call(noise, tone, noise_sigmas, tone_params, tiles, view, hed, hsb, blur)
        if with_hed or with_hsb or with_blur or with_post or view is not None or windows is not None:
            return self._route_batch(tiles, True, {}, out, ws, tensor_format, view, windows, (hed, hed_sigmas, hed_biases) if with_hed else None,
                                     (hsb, hsb_sigmas) if with_hsb else None, (blur, blur_sigmas) if with_blur else None,
                                     (noise, tone, noise_sigmas, tone_params) if with_post else None)
        if tensor_format is None:
            return self._transform_tiles(tiles, out=out, ws=ws)
        route = _tensor_route or TENSOR_ROUTE
        if route == "fused":           # the fit, then the apply pass that converts its bytes in registers: no uint8 image
            M, maxC, status = self._fit_tiles(tiles, ws=ws)
            M_t, c_t = self._target_on(tiles.device)
            x = engine.normalize_apply_tensor(tiles, M, maxC, M_t, c_t, tensor_format, out=out)
        elif route == "convert":       # today's transform into a uint8 scratch, then the converter
            u8, M, maxC, status = self._transform_tiles(tiles, ws=ws)
            x = tensor_format.convert(u8, out=out)
        else:
            raise ValueError("_tensor_route must be 'fused' or 'convert'")
        return x, M, maxC, status

    # -- stain separation (an extension: torchstain's normalize(..., stains=True), the concentration maps of staintools) ----
    def separate_batch(self, tiles, want=("norm", "h", "e", "conc"), conc_dtype=None, normalize=True, ws=None, tensor_format=None, view=None,
                       windows=None, blur=None, blur_sigmas=None, noise=None, tone=None, noise_sigmas=None, tone_params=None, recipe=None,
                       recipe_draw=None):
        """(N,H,W,3) uint8 device tensor -> (Separated, M_src, maxC_src, status): the per-tile fit, then ONE pass that writes what
        ``want`` names -- norm (transform_batch's image), h / e (the haematoxylin-only / eosin-only image, (N,H,W,3) uint8) and conc
        (the normalised concentrations, (N,2,H,W) planes of ``conc_dtype``: float32 by default, float16 or bfloat16).
        ``normalize=False``: no target (no fit() needed) -- every tile under its own stain matrix, conc = the raw concentrations.
        A tile whose status is non-zero: norm = the tile, h = e = white, conc = 0.
        ``view``: a ``stainlib_amd.TileView`` -- the unchanged fit of the WHOLE tiles, then ONE pass that writes per tile only the window
        ``windows[t]`` (default: ``view.draw(N, H, W)``, drawn behind every check) of each wanted output, flipped and turned
        (engine.stain_separate_view): bit for bit the torch slice / flip / rot90 of the call without a view, the images (N,oh,ow,3) and
        conc (N,2,oh,ow); the call then returns (Separated, M_src, maxC_src, status, windows).  ``TileView(shrink=2 or 4)`` box-shrinks
        the images as in transform_batch and does not go with 'conc' in ``want``; a resizing view (``TileView(scale=)``) is refused.
        ``tensor_format``: a ``stainlib_amd.TensorFormat`` (with ``view`` only; ``TileView(None, flip=False, rot90=False)`` is the
        fused full-tile tensor) -- norm, h and e are then (N,3,oh,ow) tensors, bit for bit ``tensor_format.convert`` of the uint8 views.
        ``blur``, ``blur_sigmas``: refused (ValueError) -- the separation pass has no blur stage.
        ``noise``, ``tone``, ``noise_sigmas``, ``tone_params``: refused (ValueError) -- the separation pass has no post stage.
        ``recipe``, ``recipe_draw``: refused (ValueError) -- the separation pass has no stages."""
        import torch
        from .. import engine
        engine._no_recipe(recipe, recipe_draw, "separate_batch", "its pass has no colour or post stage; take view= for the windows alone")
        engine._no_blur(blur, blur_sigmas, "separate_batch")
        engine._no_post(noise, tone, noise_sigmas, tone_params, "separate_batch")
        conc_dtype = torch.float32 if conc_dtype is None else conc_dtype
        want = engine._separate_want(want, conc_dtype)
        with_view = engine.separate_view_check(view, windows, tensor_format, want, conc_dtype, tiles)
        if normalize and not hasattr(self, "stain_matrix_target"):
            raise ValueError("separate_batch(normalize=True) needs a fitted target: call fit() first, or pass normalize=False")
        if with_view:
            engine._check_tiles(tiles)
        M, maxC, status = self._fit_tiles(tiles, ws=ws)
        M_t, c_t = self._target_on(tiles.device) if normalize else (None, None)
        if with_view:
            size, d_mask, windows, shrink = engine._view_call(view, windows, tiles)          # (the draw, behind every check)
            sep = engine.stain_separate_view(tiles, windows, size, M, maxC, M_t, c_t, d_mask=d_mask, want=want, conc_dtype=conc_dtype,
                                             fmt=tensor_format, shrink=shrink)
            return sep, M, maxC, status, windows
        sep = engine.stain_separate(tiles, M, maxC, M_t, c_t, want=want, conc_dtype=conc_dtype)
        return sep, M, maxC, status

    # -- stain jitter in the apply pass (an extension: RandStainNA / StainAugmentor-style augmentation of the normalised tiles) ----
    def augment_batch(self, tiles, alpha_beta, augment_background=False, normalize=True, out=None, ws=None, tensor_format=None, view=None,
                      windows=None, hed=None, hed_sigmas=None, hed_biases=None, hsb=None, hsb_sigmas=None, blur=None, blur_sigmas=None, noise=None, tone=None, noise_sigmas=None, tone_params=None,
                      recipe=None, recipe_draw=None):
        """(N,H,W,3) uint8 device tensor -> (out, M_src, maxC_src, status): the per-tile fit, then ONE pass that normalises every tile
        and perturbs its stains: C_i * alpha_i + beta_i on the normalised concentrations of tissue pixels (every pixel with
        ``augment_background``), under the target's stain matrix, clipped.  ``alpha_beta``: (N, 4) = alpha0, beta0, alpha1, beta1 per
        tile (``stainlib_amd.StainJitter(...).draw(N)``).  With alpha = 1, beta = 0 the result is transform_batch's.
        ``normalize=False``: no target (no fit() needed) -- every tile perturbed under its own stain matrix, a batched StainAugmentor.
        ``tensor_format``: a ``stainlib_amd.TensorFormat``; `out` is then the (N,3,H,W) tensor in that format, bit for bit
        ``tensor_format.convert`` of the uint8 result.  A tile whose status is non-zero comes back as its own bytes (their conversion).
        ``view``, ``windows``: as in transform_batch -- the crop / flip / quarter turn of every tile in the same pass; the call then
        returns (out, M_src, maxC_src, status, windows).
        ``hed``, ``hed_sigmas``, ``hed_biases``: as in transform_batch -- the HedColorAugmenter's transform of the perturbed tile in the
        same pass; one more element at the end of the returned tuple, ``engine.HedDraw``.
        ``hsb``, ``hsb_sigmas``: as in transform_batch -- the HsbColorAugmenter's map of the perturbed tile in the same pass; one more
        element at the end of the returned tuple, ``engine.HsbDraw``.
        ``blur``, ``blur_sigmas``: as in transform_batch -- the GaussianBlurAugmenter's blur of the perturbed tile in the same pass; one
        more element at the end of the returned tuple, ``engine.BlurDraw``.
        ``noise``, ``tone``, ``noise_sigmas``, ``tone_params``: as in transform_batch -- the post stage on the written pixels of the
        perturbed tile in the same pass; one more element at the end of the returned tuple, ``engine.PostDraw``.
        ``recipe``, ``recipe_draw``: as in transform_batch -- the Recipe's colour stage on the perturbed tile, its view and its tone / noise
        in the same pass; the call returns (out, M_src, maxC_src, status, ``engine.RecipeDraw``)."""
        from .. import engine
        engine._jitter_args(None, None, alpha_beta, None, tensor_format, out)
        if normalize and not hasattr(self, "stain_matrix_target"):
            raise ValueError("augment_batch(normalize=True) needs a fitted target: call fit() first, or pass normalize=False")
        if engine._recipe_call(recipe, recipe_draw, tiles, view=view, windows=windows, hed=hed, hed_sigmas=hed_sigmas, hed_biases=hed_biases,
                               hsb=hsb, hsb_sigmas=hsb_sigmas, blur=blur, blur_sigmas=blur_sigmas, noise=noise, tone=tone,
                               noise_sigmas=noise_sigmas, tone_params=tone_params):
            return self._route_batch(tiles, normalize, dict(alpha_beta=alpha_beta, augment_background=augment_background), out, ws,
                                     tensor_format, None, None, None, recipe=(recipe, recipe_draw))
        with_hed = engine._hed_call(hed, hed_sigmas, hed_biases, tiles, view)
        with_hsb = engine._hsb_call(hsb, hsb_sigmas, tiles, view, hed)
        with_blur = engine._blur_call(blur, blur_sigmas, tiles, view, hed, hsb)
        with_post = engine._post_call(noise, tone, noise_sigmas, tone_params, tiles, view, hed, hsb, blur)
        return self._route_batch(tiles, normalize, dict(alpha_beta=alpha_beta, augment_background=augment_background), out, ws,
                                 tensor_format, view, windows, (hed, hed_sigmas, hed_biases) if with_hed else None,
                                 (hsb, hsb_sigmas) if with_hsb else None, (blur, blur_sigmas) if with_blur else None,
                                 (noise, tone, noise_sigmas, tone_params) if with_post else None)

    def separate(self, I, normalize=True):
        """An image (RGB uint8) -> Separated of numpy arrays: norm (= transform(I)), h, e ((H,W,3) uint8) and conc ((2,H,W) float32)."""
        assert is_uint8_image(I), _UINT8_MSG
        from .. import engine
        dev = _to_device(I)
        if normalize:
            M_t, c_t = self._target_on(dev.device)
        else:
            M_t = c_t = None
        big = self._big_image_statistics(dev)
        if big is not None:
            sep = engine.stain_separate(dev, big[0][None], big[1][None], M_t, c_t)
        else:
            M, maxC, status = self._fit_tiles(dev)
            st = int(status[0])
            raise_for_status(st)
            if st != 0:
                warnings.warn("99th-percentile concentration of the source is zero; the reference divides by it",
                              RuntimeWarning)
            sep = engine.stain_separate(dev, M, maxC, M_t, c_t)
        return engine.Separated(*(t[0].cpu().numpy() for t in sep))

    def state_dict(self):
        return {"method": self.method, "stain_matrix_target": np.array(self.stain_matrix_target),
                "maxC_target": np.array(self.maxC_target)}

    def load_state_dict(self, d):
        assert d["method"] == self.method
        self.stain_matrix_target = np.array(d["stain_matrix_target"], dtype=np.float64).reshape(2, 3)
        self.maxC_target = np.array(d["maxC_target"], dtype=np.float64).reshape(1, 2)
        self._target = None                      # the state of an earlier fit() no longer describes this target
        self._target_concentrations = None


class MacenkoNormalizer(ExtractiveStainNormalizer):
    """StainTools-style alias named by BASELINE.json's north_star."""

    def __init__(self):
        super().__init__("macenko")


class VahadaneNormalizer(ExtractiveStainNormalizer):
    def __init__(self):
        super().__init__("vahadane")


class ReinhardStainNormalizer(object):
    """normalization/normalizer.py:54-94 (exported at stainlib/__init__.py:28): Reinhard colour transfer in cv2's 8-bit Lab.

    ``fit`` keeps ``target_means`` / ``target_stds`` as tuples of (1,1) float64 arrays like cv2.meanStdDev returns them.
    The whole transform is three sweeps of csrc/lab.hip (two histogram sweeps, one table-driven map); OpenCV's integer Lab
    conversions are restated there -- parity unpinned against cv2 itself, the reference's own arithmetic
    around them is golden-pinned."""

    def __init__(self, target_means=0, target_stds=0):
        self.target_means = target_means                                  # normalizer.py:61-62
        self.target_stds = target_stds

    def fit(self, target):
        from .. import engine
        st = engine.reinhard_stats(_to_device(target), standardize=True)[0].cpu().numpy()      # normalizer.py:65-66
        self.target_means = tuple(np.array([[st[1 + c]]]) for c in range(3))
        self.target_stds = tuple(np.array([[st[4 + c]]]) for c in range(3))

    def _targets(self):
        return ([float(np.asarray(m).reshape(-1)[0]) for m in self.target_means],
                [float(np.asarray(s).reshape(-1)[0]) for s in self.target_stds])

    def transform(self, I, mask_background=False, luminosity_threshold=0.8):
        """normalizer.py:70-94."""
        from .. import engine
        from ..utils.excepts import TissueMaskException
        tm, ts = self._targets()
        out, st = engine.reinhard_transform(_to_device(I), tm, ts, mask_background, luminosity_threshold)
        if mask_background and int(st[0, 7]) == 0:
            raise TissueMaskException("Empty tissue mask computed")       # stain_utils.py:46-47 via normalizer.py:86
        return out[0].cpu().numpy()

    def transform_batch(self, tiles, mask_background=False, luminosity_threshold=0.8, out=None, ws=None, tensor_format=None, view=None,
                        windows=None, blur=None, blur_sigmas=None, noise=None, tone=None, noise_sigmas=None, tone_params=None, recipe=None,
                        recipe_draw=None):
        """Batched extension: (N,H,W,3) uint8 device tensor -> (out, stats (N,8): p90, means, stds, tissue pixels).
        ``tensor_format``: a ``stainlib_amd.TensorFormat``; `out` is then the (N,3,H,W) tensor in that format (the map writes a uint8
        scratch, ``tensor_format.convert`` reads it).
        ``view``: a ``stainlib_amd.TileView`` -- the unchanged statistics of the WHOLE tiles, then ONE map sweep that writes per tile only
        the window ``windows[t]`` (default: ``view.draw(N, H, W)``) of that result, flipped and turned, as (N,oh,ow,3) uint8 or, with a
        ``tensor_format``, the (N,3,oh,ow) tensor -- no uint8 scratch (engine.reinhard_view); the call returns (out, stats, windows).
        ``TileView(None, flip=False, rot90=False)`` is the fused full-tile tensor.  ``windows`` without ``view`` is a ValueError.
        ``blur``, ``blur_sigmas``: refused (ValueError) -- the Lab family's fused pass has no blur stage; blur its uint8 result
        (``blur.transform_batch(view=, tensor_format=)``).  ``recipe``, ``recipe_draw``: refused (ValueError) likewise -- take the uint8
        result through ``tensor_format.convert(u8, recipe=)``."""
        from .. import engine
        engine._no_recipe(recipe, recipe_draw, "the Lab family's fused calls (ReinhardStainNormalizer.transform_batch)",
                          "take its uint8 result through TensorFormat.convert(u8, recipe=)")
        engine._no_blur(blur, blur_sigmas, "the Lab family's fused calls (ReinhardStainNormalizer.transform_batch)")
        engine._no_post(noise, tone, noise_sigmas, tone_params, "the Lab family's fused calls (ReinhardStainNormalizer.transform_batch)")
        tm, ts = self._targets()
        if engine.lab_view_check(view, windows, tiles):
            return engine.reinhard_view(tiles, windows, None, tm, ts, mask_background=mask_background,
                                        luminosity_threshold=luminosity_threshold, fmt=tensor_format, out=out, ws=ws, view=view)
        if tensor_format is None:
            return engine.reinhard_transform(tiles, tm, ts, mask_background, luminosity_threshold, out=out, ws=ws)
        u8, st = engine.reinhard_transform(tiles, tm, ts, mask_background, luminosity_threshold, ws=ws)
        return tensor_format.convert(u8, out=out), st

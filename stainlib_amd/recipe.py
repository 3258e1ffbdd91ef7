"""Recipe (an extension): the augmentation set of a segmentation loader as ONE pass -- a colour perturbation on the source pixels, a view
of any kind (crop / flip / turn, box shrink, random-resized crop, rotation / zoom / shear, elastic field) and a tone curve and noise on the
written pixels (the HoVer-Net / Tellez et al. recipe).  The definition is the composition of the stages' own:

    out[t] = convert( post( view( colour(full[t]) ) ) )

with `full[t]` the uint8 image the call writes without any stage or view; every absent stage is the identity.  The fill byte of a
TileAffine / TileElastic is in output space: it does not take the colour stage and it does take tone and noise.  The batch methods take a
Recipe as recipe= (transform_batch / augment_batch of the Macenko and Vahadane normalizers, StainAugmentor.augment_batch,
TensorFormat.convert); engine.recipe_stage makes the draws and the call."""
from .augmentation.augmenter import HedColorAugmenter
from .augmentation.hsb import HsbColorAugmenter
from .augmentation.noise import GaussianNoiseAugmenter, ToneCurveAugmenter
from .tile_view import TileAffine, TileView

_CHAIN_MODES = {1: "0.19", 2: "0.17", 3: "experimental_log10"}


class Recipe(object):
    """Recipe(view=None, color=None, noise=None, tone=None): at most one view (a TileView in all its forms, a TileAffine or a TileElastic),
    at most one colour stage on SOURCE pixels (a HedColorAugmenter of skimage_mode "0.18", or an HsbColorAugmenter) and the post stage
    on WRITTEN pixels (a ToneCurveAugmenter, then a GaussianNoiseAugmenter).  At least one of the four (ValueError).
    A recipe= call draws, from the global numpy stream and after the call's own alpha_beta: color.randomize_batch(N), then
    tone.randomize_batch(N), then noise.randomize_batch(N), then view.draw(N, H, W); it returns one engine.RecipeDraw(windows, color, post)
    at the end of its tuple, which reproduces the call as recipe_draw=.  Label maps go through recipe.view.apply(planes, draw.windows).
    A Gaussian blur is not part of a recipe (its halo does not fit a rotated source box): chain blur.transform_batch in front."""

    def __init__(self, view=None, color=None, noise=None, tone=None):
        if view is None and color is None and noise is None and tone is None:
            raise ValueError("an empty Recipe: give at least one of view=, color=, noise=, tone=")
        if view is not None and not isinstance(view, (TileView, TileAffine)):
            raise ValueError("view must be a stainlib_amd TileView, TileAffine or TileElastic")
        if color is not None and not isinstance(color, (HedColorAugmenter, HsbColorAugmenter)):
            raise ValueError("color must be a stainlib_amd HedColorAugmenter or HsbColorAugmenter (one colour stage; blur is not part of a "
                             "recipe)")
        if isinstance(color, HedColorAugmenter) and color._skimage_mode in _CHAIN_MODES:
            m = color._skimage_mode
            raise ValueError(f"skimage_mode {_CHAIN_MODES[m]!r} ({m}) goes through the hed_augment chain, which is not part of the one-pass "
                             "recipe: a Recipe needs a HedColorAugmenter of skimage_mode '0.18' (0)")
        if noise is not None and not isinstance(noise, GaussianNoiseAugmenter):
            raise ValueError("noise must be a stainlib_amd GaussianNoiseAugmenter (its range and channel mode are used)")
        if tone is not None and not isinstance(tone, ToneCurveAugmenter):
            raise ValueError("tone must be a stainlib_amd ToneCurveAugmenter (its ranges are used)")
        self.view, self.color, self.noise, self.tone = view, color, noise, tone

    def __repr__(self):
        return f"Recipe(view={self.view!r}, color={self.color!r}, noise={self.noise!r}, tone={self.tone!r})"

"""stainlib_amd -- MI355X-native drop-in for the hot path of sebastianffx/stainlib.

The export list mirrors stainlib/__init__.py:19-30.  ReinhardStainNormalizer and LuminosityStandardizer (SURVEY
8f-3 / 8f-4) sit on OpenCV's 8-bit Lab conversions, restated in csrc/lab.hip: parity unpinned against cv2 itself.
TensorFormat (an extension) turns the batched operators' uint8 results into model-ready float tensors.
StainJitter (an extension) draws the per-tile (alpha, beta) of the augment_batch methods: stain jitter inside the apply pass.
TileView (an extension) draws the per-tile crop / flip / quarter turn that view= applies inside the same pass.
TileAffine (an extension) draws a per-tile rotation by any angle, zoom, shear and translation for view=: bilinear, in integers.
TileElastic (an extension) adds an elastic deformation to it -- a quadratic B-spline of a coarse lattice of random displacements, in
integers, for images and label planes alike; its windows are an ElasticWindows(affine, field).
HsbColorAugmenter (an extension; HsbLight / HsbStrong presets) is the hue / saturation / brightness sibling of the HED augmenters, in integers.
GaussianBlurAugmenter (an extension) is the Gaussian blur of that set: a per-tile integer separable filter, fused into the view pass (blur=).
GaussianNoiseAugmenter and ToneCurveAugmenter (extensions) are its noise and brightness / contrast / gamma items: integer maps on the
WRITTEN pixels of the view pass (noise=, tone=); the per-pixel noise is a counter-based generator (Philox4x32-10) on the device.
Recipe (an extension) holds one colour stage, one view of any kind and the tone / noise stage for ONE pass (recipe=).
Separated (an extension) is what the normalizers' separate / separate_batch return: per-stain images and concentration maps.
Importing the package does not need a GPU; calling anything numeric does, and fails loudly without the
HIP library -- there is no CPU fallback.
"""
from . import _ffi  # noqa: F401
from .augmentation.augmenter import (HedLightColorAugmenter, HedLighterColorAugmenter,  # noqa: F401
                                     HedStrongColorAugmenter, StainAugmentor, GrayscaleAugmentor, StainJitter)
from .augmentation.hsb import HsbColorAugmenter, HsbLightColorAugmenter, HsbStrongColorAugmenter  # noqa: F401
from .augmentation.blur import GaussianBlurAugmenter  # noqa: F401
from .augmentation.noise import GaussianNoiseAugmenter, ToneCurveAugmenter  # noqa: F401
from .extraction.macenko_stain_extractor import MacenkoStainExtractor  # noqa: F401
from .extraction.vahadane_stain_extractor import VahadaneStainExtractor  # noqa: F401
from .normalization.normalizer import (ExtractiveStainNormalizer, MacenkoNormalizer,  # noqa: F401
                                       ReinhardStainNormalizer, VahadaneNormalizer)
from .tensor_format import TensorFormat  # noqa: F401
from .recipe import Recipe  # noqa: F401
from .separated import Separated  # noqa: F401
from .tile_view import ElasticWindows, TileAffine, TileElastic, TileView  # noqa: F401
from .utils.stain_utils import LuminosityStandardizer  # noqa: F401
from .utils.excepts import InvalidRangeError, TissueMaskException  # noqa: F401

__version__ = "0.6.0"

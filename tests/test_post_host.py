"""The post stage on the host side -- additive noise and tone curves on the bytes a call writes (stainlib_amd/augmentation/noise.py,
sl_post_augment, sl_normalize_post_view, noise= / tone= on the batch methods): the generator's known answers, the identities, the codes,
the statistics of the definition on a fixed key, the augmenters' draws and errors, every refusal before any draw, the draw order, the
header / binding / library agreement and the two stand-alone C / C++ programs -- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine
from stainlib_amd.augmentation import noise as P
from stainlib_amd.utils.excepts import InvalidRangeError
from tests.gpu_util import BAD_SHAPES, BAD_STATS, ROUTES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
BADARG = -1
RGB, OUT, D6, D2, AB, WIN, CD, TB = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x300400, 0x300501
N, HH, WW, OH, OW = 4, 64, 48, 40, 32
KEY = (12345, 678)                                 # the fixed key of the statistics below


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox4x32_10_gives_the_known_answers():
    for ctr, key, want in KNOWN:
        got = P.philox4x32_10(np.array(ctr, dtype=np.uint64), key)
        assert got.dtype == np.uint32 and " ".join("%08x" % v for v in got) == want
    both = P.philox4x32_10(np.array([KNOWN[0][0], (1, 0, 0, 0)]), (0, 0))                      # vectorised over counters
    assert " ".join("%08x" % v for v in both[0]) == KNOWN[0][2] and not np.array_equal(both[0], both[1])
    # the int32 bit patterns of a key are the key
    assert np.array_equal(P.philox4x32_10(np.array(KNOWN[1][0]), (-1, -1)), P.philox4x32_10(np.array(KNOWN[1][0]), KNOWN[1][1]))


def _cube():
    g = np.arange(0, 256, 3, dtype=np.uint8)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(86, 86 * 86, 3)           # a strided colour cube as one image


def test_sq_zero_and_the_identity_table_are_the_identity():
    cube = _cube()
    ident = np.arange(256, dtype=np.uint8)
    zero = P.noise_codes(0.0, KEY)[0]
    assert zero.tolist() == [0, 12345, 678, 0]
    assert np.array_equal(P.post_reference(cube, codes=zero), cube)
    assert np.array_equal(P.post_reference(cube, tables=ident), cube)
    assert np.array_equal(P.post_reference(cube, tables=ident, codes=zero), cube)
    assert np.array_equal(P.post_reference(cube[None], tables=ident[None], codes=zero[None])[0], cube)
    assert not np.array_equal(P.post_reference(cube, codes=P.noise_codes(1.0, KEY)[0]), cube)   # (the stage does something)


def test_tone_tables():
    assert np.array_equal(P.tone_table(0, 1, 1), np.arange(256)) and P.tone_table(0, 1, 1).dtype == np.uint8
    rng = np.random.RandomState(2)
    for _ in range(200):                                                                       # monotone for contrast >= 0
        t = P.tone_table(rng.uniform(-1, 1), rng.uniform(0, 4), np.exp(rng.uniform(np.log(0.25), np.log(4))))
        assert t.shape == (256,) and (np.diff(t.astype(np.int16)) >= 0).all()
    assert (P.tone_table(0, 0, 1) == 128).all() and (P.tone_table(1, 1, 1) == 255).all() and (P.tone_table(-1, 1, 1) == 0).all()
    assert P.tone_table(0, 1, 2.0)[128] == int(np.floor(255 * (128 / 255) ** 2 + 0.5))
    tabs = P.tone_tables([[0, 1, 1], [0.1, 1.2, 0.8]])
    assert tabs.shape == (2, 256) and np.array_equal(tabs[0], np.arange(256)) and np.array_equal(tabs[1], P.tone_table(0.1, 1.2, 0.8))
    for bad in ((1.5, 1, 1), (0, -0.1, 1), (0, 4.5, 1), (0, 1, 0.2), (0, 1, 5), (np.nan, 1, 1), (0, 1, np.inf)):
        with pytest.raises(ValueError):
            P.tone_table(*bad)
    with pytest.raises(ValueError, match="an \\(N, 3\\) array"):
        P.tone_tables(np.zeros((2, 4)))
    # the tone curve comes first, the noise second
    img = np.full((4, 4, 3), 10, np.uint8)
    tab = np.full(256, 200, np.uint8)
    c = P.noise_codes(3.0, KEY)[0]
    assert np.array_equal(P.post_reference(img, tables=tab, codes=c), P.post_reference(np.full((4, 4, 3), 200, np.uint8), codes=c))


def test_noise_codes_and_their_reduction():
    assert P.SQ_MAX == 28378 and int(P.noise_sq(64)) == 28378 and int(P.noise_sq(1)) == 443 and int(P.noise_sq(0)) == 0
    c = P.noise_codes([64, 1], [(0xffffffff, 1), (2, 0x80000000)], mono=True)
    assert c.dtype == np.int32 and c.tolist() == [[28378, -1, 1, 1], [443, 2, -2 ** 31, 1]]
    for bad in (-0.001, 64.001, np.nan, np.inf, [1, 65]):
        with pytest.raises(ValueError, match="\\[0, 64\\]"):
            P.noise_codes(bad)
    with pytest.raises(ValueError, match="an \\(N,\\) array"):
        P.noise_codes(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="keys"):
        P.noise_codes([1, 2], np.zeros((3, 2)))
    wild = np.array([[-5, 7, 8, 0], [28379, 7, 8, 9], [2 ** 31 - 1, -1, -2 ** 31, -3], [-2 ** 31, 0, 0, 0]], dtype=np.int32)
    red = P.reduce_codes(wild)
    assert red.tolist() == [[0, 7, 8, 0], [28378, 7, 8, 1], [28378, -1, -2 ** 31, 1], [0, 0, 0, 0]]
    img = np.random.RandomState(1).randint(0, 256, (4, 9, 11, 3)).astype(np.uint8)
    assert np.array_equal(P.post_reference(img, codes=wild), P.post_reference(img, codes=red.astype(np.int32)))
    assert np.array_equal(P.post_reference(img, codes=wild)[0], img[0])


# ---- statistics of the definition on a fixed key (a condition on the reference; deterministic) ----------------------------------------------
@pytest.mark.parametrize("sigma", [1, 5, 20])
def test_the_noise_of_the_definition_has_the_mean_and_variance_it_claims(sigma):
    grey = np.full((256, 256, 3), 128, np.uint8)
    code = P.noise_codes(sigma, KEY)[0]
    d = P.post_reference(grey, codes=code).astype(np.float64) - 128.0
    sigma_eff = float(code[0]) * np.sqrt(P.VAR_G) / 65536.0
    want_var = sigma_eff ** 2 + 1.0 / 12.0                        # the rounding to a byte adds a uniform's variance
    npx = 256 * 256
    for c in range(3):
        mean, var = d[..., c].mean(), d[..., c].var()
        print(f"sigma {sigma} channel {c}: mean {mean:.4f} (standard error {np.sqrt(want_var / npx):.4f}), std {np.sqrt(var):.4f}, wanted {np.sqrt(want_var):.4f}")
        assert abs(mean) <= 4.0 * np.sqrt(want_var / npx)
        assert abs(var / want_var - 1.0) <= 0.02
    r = np.corrcoef(d.reshape(-1, 3).T)
    assert max(abs(r[0, 1]), abs(r[0, 2]), abs(r[1, 2])) < 0.02
    mono = P.post_reference(grey, codes=P.noise_codes(sigma, KEY, mono=True)[0])
    assert np.array_equal(mono[..., 0], mono[..., 1]) and np.array_equal(mono[..., 0], mono[..., 2]) and mono.std() > 0.5 * sigma
    # clamping: white never passes 255, black never goes below 0 (the arithmetic is done in a wider type and clamped, not wrapped)
    code64 = P.noise_codes(64, KEY)[0]
    white = P.post_reference(np.full((64, 64, 3), 255, np.uint8), codes=code64)
    black = P.post_reference(np.zeros((64, 64, 3), np.uint8), codes=code64)
    assert white.min() < 255 and (white >= 128).mean() > 0.9 and (white == 255).mean() > 0.4
    assert black.max() > 0 and (black <= 127).mean() > 0.9 and (black == 0).mean() > 0.4


def test_a_tiles_noise_depends_on_its_key_not_on_its_place_in_the_batch():
    img = np.random.RandomState(3).randint(0, 256, (3, 8, 12, 3)).astype(np.uint8)
    codes = P.noise_codes([3, 7, 11], [(1, 2), (3, 4), (5, 6)])
    out = P.post_reference(img, codes=codes)
    perm = [2, 0, 1]
    assert np.array_equal(P.post_reference(img[perm], codes=codes[perm]), out[perm])
    assert np.array_equal(P.post_reference(img[1], codes=codes[1]), out[1])


# ---- the augmenters -------------------------------------------------------------------------------------------------------------------------
def test_the_noise_augmenter_draws_sigma_then_the_two_key_words():
    aug = stainlib_amd.GaussianNoiseAugmenter(sigma_range=(2, 9))
    assert aug.keyword == "gaussian_noise" and aug._sigma == 2.0 and aug._key == (0, 0)         # the lower bound and key (0, 0) until randomize()
    assert aug.shapes({"a": 1}) == {"a": 1}
    assert aug.codes().tolist() == [[int(P.noise_sq(2)), 0, 0, 0]]
    np.random.seed(9)
    aug.randomize()
    after = np.random.uniform()
    np.random.seed(9)
    want = (np.random.uniform(2, 9), int(np.random.randint(0, 2 ** 32, dtype=np.uint32)), int(np.random.randint(0, 2 ** 32, dtype=np.uint32)))
    assert np.random.uniform() == after and (aug._sigma, aug._key[0], aug._key[1]) == want
    np.random.seed(4)
    s, codes = aug.randomize_batch(3)
    after = np.random.uniform()
    np.random.seed(4)
    rows = [(np.random.uniform(2, 9), int(np.random.randint(0, 2 ** 32, dtype=np.uint32)), int(np.random.randint(0, 2 ** 32, dtype=np.uint32)))
            for _ in range(3)]
    assert np.random.uniform() == after
    assert s.shape == (3,) and s.dtype == np.float64 and np.array_equal(s, [r[0] for r in rows])
    assert codes.shape == (3, 4) and codes.dtype == np.int32
    assert np.array_equal(codes, P.noise_codes(s, [(r[1], r[2]) for r in rows]))
    assert np.array_equal(codes[:, 1:3].view(np.uint32), np.array([(r[1], r[2]) for r in rows], dtype=np.uint32))
    mono = stainlib_amd.GaussianNoiseAugmenter((1, 1), per_channel=False)
    assert mono.randomize_batch(2)[1][:, 3].tolist() == [1, 1]
    patch = np.random.RandomState(0).randint(0, 256, (7, 5, 3)).astype(np.uint8)
    assert np.array_equal(aug.transform(patch), P.post_reference(patch, codes=aug.codes()[0]))


def test_the_tone_augmenter_draws_brightness_contrast_then_log_uniform_gamma():
    aug = stainlib_amd.ToneCurveAugmenter(brightness_range=(-0.2, 0.3), contrast_range=(0.5, 1.5), gamma_range=(0.5, 2.0))
    assert aug.keyword == "tone_curve" and aug._params == [-0.2, 0.5, 0.5]                      # the lower bounds until randomize()
    np.random.seed(9)
    aug.randomize()
    after = np.random.uniform()
    np.random.seed(9)
    want = [np.random.uniform(-0.2, 0.3), np.random.uniform(0.5, 1.5), float(np.exp(np.random.uniform(np.log(0.5), np.log(2.0))))]
    assert np.random.uniform() == after and aug._params == want
    np.random.seed(4)
    p, tabs = aug.randomize_batch(3)
    np.random.seed(4)
    want = np.array([[np.random.uniform(-0.2, 0.3), np.random.uniform(0.5, 1.5), np.exp(np.random.uniform(np.log(0.5), np.log(2.0)))]
                     for _ in range(3)])
    assert p.shape == (3, 3) and np.array_equal(p, want) and tabs.shape == (3, 256) and tabs.dtype == np.uint8
    assert np.array_equal(tabs, P.tone_tables(p))
    # a None range draws nothing and gives the neutral value
    some = stainlib_amd.ToneCurveAugmenter(gamma_range=(0.8, 1.25))
    assert some._params == [0.0, 1.0, 0.8]
    np.random.seed(6)
    some.randomize()
    after = np.random.uniform()
    np.random.seed(6)
    g = float(np.exp(np.random.uniform(np.log(0.8), np.log(1.25))))
    assert np.random.uniform() == after and some._params == [0.0, 1.0, g]
    none = stainlib_amd.ToneCurveAugmenter()
    np.random.seed(4)
    p, tabs = none.randomize_batch(2)
    none.randomize()
    a = np.random.uniform()
    np.random.seed(4)
    assert np.random.uniform() == a and p.tolist() == [[0, 1, 1]] * 2 and np.array_equal(tabs, np.tile(np.arange(256), (2, 1)))
    patch = np.random.RandomState(0).randint(0, 256, (7, 5, 3)).astype(np.uint8)
    assert np.array_equal(aug.transform(patch), P.tone_table(*aug._params)[patch])


@pytest.mark.parametrize("rng", [(-1, 5), (5, 4), (0, 64.5), (1, 2, 3), 5])
def test_noise_ranges_outside_zero_to_sixty_four_raise_invalid_range_error(rng):
    with pytest.raises(InvalidRangeError):
        stainlib_amd.GaussianNoiseAugmenter(sigma_range=rng)


@pytest.mark.parametrize("kw", [dict(brightness_range=(-1.1, 0)), dict(brightness_range=(0.2, 0.1)), dict(brightness_range=(0, 1.5)),
                                dict(contrast_range=(-0.1, 1)), dict(contrast_range=(1, 4.5)), dict(contrast_range=(2, 1)),
                                dict(gamma_range=(0.2, 1)), dict(gamma_range=(1, 4.1)), dict(gamma_range=(2, 1)), dict(gamma_range=(0, 1)),
                                dict(gamma_range=(1, 2, 3)), dict(contrast_range=1.0)])
def test_tone_ranges_outside_their_bounds_raise_invalid_range_error(kw):
    with pytest.raises(InvalidRangeError):
        stainlib_amd.ToneCurveAugmenter(**kw)


def test_transform_refuses_what_is_no_uint8_image():
    with pytest.raises(TypeError):
        stainlib_amd.GaussianNoiseAugmenter((1, 2)).transform(np.zeros((4, 4, 3), dtype=np.float64))
    with pytest.raises(TypeError):
        stainlib_amd.ToneCurveAugmenter((0, 0.1)).transform(np.zeros((4, 4, 3), dtype=np.float32))


# ---- refusals: a ValueError that names its cause, before any draw (CPU tiles: an accepted call stops at the tile check) -----------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
_SG = np.array([2.0, 5.0])
_TP = np.array([[0.1, 1.1, 0.9], [0.0, 1.0, 1.0]])
_WIN = np.array([[0, 0, 0], [4, 4, 6]], dtype=np.int32)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def _methods():
    nz = stainlib_amd.MacenkoNormalizer()
    nz.stain_matrix_target, nz.maxC_target = np.array([[0.6, 0.7, 0.4], [0.2, 0.9, 0.4]]), np.array([[1.5, 1.1]])
    vz = stainlib_amd.VahadaneNormalizer()
    vz.stain_matrix_target, vz.maxC_target = nz.stain_matrix_target, nz.maxC_target
    sa = stainlib_amd.StainAugmentor("macenko")
    return nz, sa, [("transform_batch", lambda **k: nz.transform_batch(_TILES, **k)),
                    ("vahadane transform_batch", lambda **k: vz.transform_batch(_TILES, **k)),
                    ("augment_batch", lambda **k: nz.augment_batch(_TILES, _AB, **k)),
                    ("augment_batch own", lambda **k: vz.augment_batch(_TILES, _AB, normalize=False, **k)),
                    ("StainAugmentor", lambda **k: sa.augment_batch(_TILES, **k))]


def test_every_refusal_names_its_cause_and_draws_nothing():
    noise = stainlib_amd.GaussianNoiseAugmenter((1, 8))
    tone = stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), (0.8, 1.2), (0.8, 1.25))
    hed = stainlib_amd.HedLightColorAugmenter()
    hsb = stainlib_amd.HsbLightColorAugmenter()
    blur = stainlib_amd.GaussianBlurAugmenter((0.3, 2.0))
    view = stainlib_amd.TileView((5, 7), rot90=False)
    affine = stainlib_amd.TileAffine((5, 5))
    elastic = stainlib_amd.TileElastic((5, 5))
    fmt = stainlib_amd.TensorFormat()
    chain = "Chain them instead: take the uint8 result .* then noise.transform_batch\\(u8, tensor_format=\\)"
    calls = _methods()[2] + [("convert", lambda **k: fmt.convert(_TILES, **k))]
    for name, call in calls:
        np.random.seed(3)
        for stage in (dict(noise=noise), dict(tone=tone), dict(noise=noise, tone=tone)):
            if name != "convert":
                with pytest.raises(ValueError, match="noise= / tone= do not go together with hed=, hsb= or blur=.*" + chain):
                    call(hed=hed, **stage)
                with pytest.raises(ValueError, match="noise= / tone= do not go together with hed=, hsb= or blur="):
                    call(hsb=hsb, view=view, **stage)
            with pytest.raises(ValueError, match="noise= / tone= do not go together with hed=, hsb= or blur=.*" + chain):
                call(blur=blur, **stage)
            with pytest.raises(ValueError, match="an affine or elastic view .* is not supported by the post stage.*" + chain):
                call(view=affine, **stage)
            with pytest.raises(ValueError, match="an affine or elastic view .* is not supported by the post stage"):
                call(view=elastic, **stage)
            with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
                call(view=(5, 7), **stage)
            with pytest.raises(ValueError, match="windows= goes with view="):
                call(windows=_WIN, **stage)
            with pytest.raises(ValueError, match="does not fit"):
                call(view=stainlib_amd.TileView(10), **stage)
            # accepted arguments: the call stops at the tile check (CPU tiles) -- AFTER the argument checks, BEFORE any draw
            with pytest.raises(ValueError, match=_TILE_CHECK):
                call(**stage)
            with pytest.raises(ValueError, match=_TILE_CHECK):
                call(view=view, **stage)
        with pytest.raises(ValueError, match="noise must be a stainlib_amd GaussianNoiseAugmenter"):
            call(noise="strong")
        with pytest.raises(ValueError, match="noise must be a stainlib_amd GaussianNoiseAugmenter"):
            call(noise=tone, view=view)
        with pytest.raises(ValueError, match="tone must be a stainlib_amd ToneCurveAugmenter"):
            call(tone=noise)
        with pytest.raises(ValueError, match="noise_sigmas= goes with noise="):
            call(noise_sigmas=_SG)
        with pytest.raises(ValueError, match="noise_sigmas= goes with noise="):
            call(tone=tone, noise_sigmas=_SG)
        with pytest.raises(ValueError, match="tone_params= goes with tone="):
            call(tone_params=_TP)
        with pytest.raises(ValueError, match="tone_params= goes with tone="):
            call(noise=noise, tone_params=_TP)
        with pytest.raises(ValueError, match="an \\(N,\\) array"):
            call(noise=noise, noise_sigmas=np.zeros((2, 3)))
        with pytest.raises(ValueError, match="one entry per tile"):
            call(noise=noise, noise_sigmas=np.zeros(3))
        with pytest.raises(ValueError, match="\\[0, 64\\]"):
            call(noise=noise, noise_sigmas=np.array([0.5, 65.0]))
        with pytest.raises(ValueError, match="\\[0, 64\\]"):
            call(noise=noise, noise_sigmas=np.array([np.nan, 1.0]))
        with pytest.raises(ValueError, match="sq must lie in"):
            call(noise=noise, noise_sigmas=np.array([[28379, 0, 0, 0], [1, 0, 0, 0]], dtype=np.int32))
        with pytest.raises(ValueError, match="one entry per tile"):
            call(noise=noise, noise_sigmas=np.zeros((3, 4), dtype=np.int32))
        with pytest.raises(ValueError, match="an \\(N, 3\\) array"):
            call(tone=tone, tone_params=np.zeros((2, 4)))
        with pytest.raises(ValueError, match="one row per tile"):
            call(tone=tone, tone_params=np.tile(_TP[:1], (3, 1)))
        with pytest.raises(ValueError, match="gamma in \\[0.25, 4\\]"):
            call(tone=tone, tone_params=np.array([[0, 1, 0.1], [0, 1, 1]]))
        with pytest.raises(ValueError, match="an \\(N, 256\\) uint8 array"):
            call(tone=tone, tone_params=np.zeros((2, 256), dtype=np.int32))
        with pytest.raises(ValueError, match="one row per tile"):
            call(tone=tone, tone_params=np.zeros((3, 256), dtype=np.uint8))
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, name                    # nothing was consumed by a refused call
    np.random.seed(3)
    # the Lab family's fused calls and separate_batch have no post stage
    nz = _methods()[0]
    rz = stainlib_amd.ReinhardStainNormalizer()
    rz.target_means, rz.target_stds = (1.0, 2.0, 3.0), (1.0, 1.0, 1.0)
    for call in (lambda **k: rz.transform_batch(_TILES, **k), lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, **k)):
        with pytest.raises(ValueError, match="noise= / tone= are not supported by the Lab family's fused calls.*then noise.transform_batch"):
            call(noise=noise)
        with pytest.raises(ValueError, match="noise= / tone= are not supported by the Lab family's fused calls"):
            call(tone=tone, view=view, tone_params=_TP)
    with pytest.raises(ValueError, match="noise= / tone= are not supported by separate_batch.*then noise.transform_batch"):
        nz.separate_batch(_TILES, noise=noise)
    with pytest.raises(ValueError, match="noise= / tone= are not supported by separate_batch"):
        nz.separate_batch(_TILES, tone=tone, view=view, want=("norm",))
    # the augmenters' own batch calls and the engine
    for aug, arg in ((noise, _SG), (tone, _TP)):
        with pytest.raises(ValueError, match=_TILE_CHECK):
            aug.transform_batch(_TILES, view=view)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            aug.transform_batch(_TILES, arg)
        with pytest.raises(ValueError, match="an affine or elastic view .* is not supported by the post stage"):
            aug.transform_batch(_TILES, view=affine)
        with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
            aug.transform_batch(_TILES, view=(5, 7))
        with pytest.raises(ValueError, match="per tile"):
            aug.transform_batch(_TILES, np.concatenate([arg, arg[:1]]), view=view)
    c2, t2 = P.noise_codes(_SG), P.tone_tables(_TP)
    with pytest.raises(ValueError, match="needs tables= .* or codes="):
        engine.post_augment(_TILES)
    with pytest.raises(ValueError, match="needs tables= .* or codes="):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6)
    with pytest.raises(ValueError, match="codes must hold"):
        engine.post_augment(_TILES, codes=np.zeros((2, 4)))           # floats are no codes
    with pytest.raises(ValueError, match="codes must hold"):
        engine.post_augment(_TILES, codes=np.zeros((2, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="tables must hold"):
        engine.post_augment(_TILES, tables=np.zeros((2, 255), dtype=np.uint8))
    with pytest.raises(ValueError, match="tables must hold"):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6, tables=t2.astype(np.int16))
    with pytest.raises(ValueError, match="codes must have one row per tile"):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6, codes=np.tile(c2[:1], (3, 1)))
    with pytest.raises(ValueError, match="tables must have one row per tile"):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6, tables=np.tile(t2[:1], (3, 1)), codes=c2)
    with pytest.raises(ValueError, match="sq must lie in"):
        engine.post_augment(_TILES, codes=c2 - np.array([3000, 0, 0, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        engine.post_augment(_TILES, tables=t2, fmt="float16")
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6, codes=c2, fmt="float16")
    with pytest.raises(ValueError, match=_TILE_CHECK):
        engine.post_augment(_TILES, tables=t2, codes=c2)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        engine.normalize_post_view(_TILES, _WIN, (5, 7), 6, tables=t2)
    after = np.random.uniform()
    np.random.seed(3)
    assert np.random.uniform() == after


def test_the_draw_order_is_alpha_beta_then_tone_then_noise_then_windows(monkeypatch):
    """the engine calls replaced by stand-ins that record what they are handed: the global numpy stream gives alpha_beta (where the method
    draws one), then the tone draws of ALL tiles, then the noise draws of all tiles (sigma, key word, key word each), then the windows"""
    n, h, w = 2, 9, 11
    seen = {}
    fit = (torch.zeros((n, 2, 3), dtype=torch.float64), torch.ones((n, 2), dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "macenko_fit", lambda t, *a, **k: fit)
    monkeypatch.setattr(engine, "vahadane_fit", lambda t, *a, **k: fit + (None,))
    for cls in (stainlib_amd.MacenkoNormalizer, stainlib_amd.VahadaneNormalizer):
        monkeypatch.setattr(cls, "_target_on", lambda self, dev: (None, None))

    def post_view(tiles, win, size, d_mask, tables, codes, **kw):
        seen.update(win=win, size=size, d_mask=d_mask, tables=tables, codes=codes, kw=kw)
        return "out"
    monkeypatch.setattr(engine, "normalize_post_view", post_view)
    noise = stainlib_amd.GaussianNoiseAugmenter((1, 8))
    tone = stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), None, (0.8, 1.25))
    view = stainlib_amd.TileView((5, 5))
    fmt = stainlib_amd.TensorFormat()
    nz, sa, methods = _methods()

    def rand_key():
        return int(np.random.randint(0, 2 ** 32, dtype=np.uint32))
    for name, call in methods + [("convert", lambda **k: fmt.convert(_TILES, **k))]:
        for with_view in (True, False):
            for with_tone, with_noise in ((True, True), (True, False), (False, True)):
                np.random.seed(77)
                res = call(**(dict(tone=tone) if with_tone else {}), **(dict(noise=noise) if with_noise else {}),
                           **(dict(view=view) if with_view else {}))
                after = np.random.uniform()
                np.random.seed(77)
                ab = stainlib_amd.StainJitter().draw(n) if name == "StainAugmentor" else _AB
                tp = np.array([[np.random.uniform(-0.1, 0.1), 1.0, np.exp(np.random.uniform(np.log(0.8), np.log(1.25)))]
                               for _ in range(n)]) if with_tone else None
                rows = [(np.random.uniform(1, 8), rand_key(), rand_key()) for _ in range(n)] if with_noise else None
                win = view.draw(n, h, w) if with_view else None
                assert np.random.uniform() == after, name            # and nothing else was consumed
                draw = res[-1]
                assert isinstance(draw, engine.PostDraw) and res[0] == "out", name
                if with_tone:
                    assert np.array_equal(draw.tone_params, tp) and np.array_equal(draw.tone_tables, P.tone_tables(tp))
                    assert np.array_equal(seen["tables"], draw.tone_tables)
                else:
                    assert draw.tone_params is None and draw.tone_tables is None and seen["tables"] is None
                if with_noise:
                    assert np.array_equal(draw.noise_sigmas, [r[0] for r in rows])
                    assert np.array_equal(draw.noise_codes, P.noise_codes([r[0] for r in rows], [r[1:] for r in rows]))
                    assert np.array_equal(seen["codes"], draw.noise_codes)
                else:
                    assert draw.noise_sigmas is None and draw.noise_codes is None and seen["codes"] is None
                if "augment" in name or name == "StainAugmentor":
                    assert np.array_equal(np.asarray(seen["kw"]["alpha_beta"]), ab)
                else:
                    assert "alpha_beta" not in seen["kw"]
                base = 1 if name == "convert" else 4                 # what the call returns today, then [windows,] PostDraw
                if with_view:
                    assert len(res) == base + 2 and np.array_equal(res[base], win) and np.array_equal(seen["win"], win)
                    assert (seen["size"], seen["d_mask"]) == ((5, 5), 7)
                else:                                                # the full tile, code 0
                    assert len(res) == base + 1 and (seen["size"], seen["d_mask"]) == (None, 0) and not np.asarray(seen["win"]).any()
    # given sigmas / params, or the codes / tables a call returned: nothing but the windows is consumed
    c2, t2 = noise.codes(_SG), P.tone_tables(_TP)
    for sg, tp in ((_SG, _TP), (c2, t2)):
        np.random.seed(5)
        res = nz.transform_batch(_TILES, noise=noise, tone=tone, noise_sigmas=sg, tone_params=tp, view=view)
        after = np.random.uniform()
        np.random.seed(5)
        assert np.array_equal(res[4], view.draw(n, h, w)) and np.random.uniform() == after
        assert np.array_equal(res[5].noise_codes, c2) and np.array_equal(res[5].tone_tables, t2)
        assert (res[5].noise_sigmas is None) == (sg is c2) and (res[5].tone_params is None) == (tp is t2)
    out, codes, win = noise.transform_batch(_TILES, _SG, view=view)
    assert out == "out" and np.array_equal(codes, c2) and win.shape == (n, 3) and seen["kw"]["shrink"] == 1 and seen["tables"] is None
    out, codes = noise.transform_batch(_TILES)
    assert np.array_equal(codes, np.tile(noise.codes(), (n, 1)))                  # the augmenter's current sigma and key for every tile
    out, tabs = tone.transform_batch(_TILES, t2)
    assert np.array_equal(tabs, t2) and seen["codes"] is None
    out, tabs, win = tone.transform_batch(_TILES, view=stainlib_amd.TileView((4, 4), scale=(0.5, 1)))
    assert np.array_equal(tabs, np.tile(P.tone_table(*tone._params), (n, 1))) and win.shape == (n, 5) and seen["kw"]["resize"] is not None


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------
def _a(rgb=RGB, out=OUT, n=N, h=HH, w=WW, tb=TB, cd=CD, fmt=None):
    return _ffi.lib().sl_post_augment(rgb, out, n, h, w, tb, cd, C.byref(fmt) if fmt is not None else None, None)


def _v(rgb=RGB, out=OUT, n=N, h=HH, w=WW, oh=OH, ow=OW, win=WIN, d_mask=7, shrink=1, mh=0, mw=0, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0,
       params=None, fmt=None, tb=TB, cd=CD):
    return _ffi.lib().sl_normalize_post_view(rgb, out, n, h, w, oh, ow, win, d_mask, shrink, mh, mw, ms, cs, mt, ct, ab, bg,
                                             C.byref(params) if params is not None else None, C.byref(fmt) if fmt is not None else None,
                                             tb, cd, None)


def test_version_header_binding_and_library_agree():
    assert _ffi.lib().sl_version() == 600 and _ffi.EXPECTED_VERSION == 600        # an extension of ABI 600
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for name, count in (("sl_post_augment", 9), ("sl_normalize_post_view", 23)):
        assert name in declared and name in _ffi.EXPORTS
        proto = re.search(r"^SL_API int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        params = [p.strip() for p in proto.split(",")]
        res, args = _ffi._SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == count
        for p, a in zip(params, args):                               # parameter by parameter: a pointer or an int
            if "SlParams" in p or "SlTensorFormat" in p:
                assert a not in (C.c_int, C.c_void_p), p
            else:
                assert a is (C.c_void_p if "*" in p else C.c_int), p
    nm = shutil.which("nm")
    assert nm is not None
    out = subprocess.run([nm, "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sl_\w+)$", out, flags=re.M))
    assert exported == declared


# tables and codes: both, the tables alone, the codes alone -- each a valid pair, so that what is refused is the other argument
PAIRS = [dict(), dict(cd=None), dict(tb=None)]


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(tb=None, cd=None), dict(cd=CD + 2), dict(tb=None, cd=CD + 1),
                                             dict(n=2 ** 31 - 1, h=32768, w=32768)], ids=str)
def test_post_augment_bad_pointers_and_shapes_are_refused(kw):
    for pair in PAIRS if "cd" not in kw and "tb" not in kw else [dict()]:
        assert _a(**pair, **kw) == BADARG and _a(**pair, **kw, fmt=_ffi.default_tensor_format()) == BADARG


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(win=None), dict(oh=0), dict(ow=0), dict(oh=-1), dict(d_mask=-1),
                                             dict(d_mask=8), dict(tb=None, cd=None), dict(cd=CD + 1), dict(tb=None, cd=CD + 2)], ids=str)
def test_post_view_bad_pointers_shapes_and_masks_are_refused_fixed_and_resizing(kw):
    for pair in PAIRS if "cd" not in kw and "tb" not in kw else [dict()]:
        for route in ROUTES:
            args = {**route, **pair, **kw}
            assert _v(**args) == BADARG, args
            assert _v(**args, mh=HH, mw=WW) == BADARG, args
            assert _v(**args, bg=1, params=_ffi.default_params(), fmt=_ffi.default_tensor_format()) == BADARG, args


@pytest.mark.parametrize("kw", [dict(oh=HH + 1), dict(ow=WW + 1), dict(oh=HH, ow=WW, d_mask=7), dict(shrink=0), dict(shrink=3), dict(shrink=2),
                                dict(oh=16, ow=16, d_mask=6, shrink=4), dict(n=1 << 22, h=32768, w=32768, oh=32768, ow=32768),
                                dict(mw=WW), dict(mh=HH), dict(mh=-1, mw=WW), dict(mh=HH + 1, mw=WW), dict(mh=HH, mw=WW + 1),
                                dict(oh=16, ow=12, shrink=2, mh=HH, mw=WW), dict(h=4096, w=4096, mh=2049, mw=2048)], ids=str)
def test_post_view_bad_geometry_is_refused(kw):
    for pair in PAIRS:
        for route in ROUTES:
            assert _v(**{**route, **pair, **kw}) == BADARG, kw


@pytest.mark.parametrize("kw", BAD_STATS, ids=str)
def test_post_view_bad_statistics_are_refused(kw):
    for pair in PAIRS:
        assert _v(**pair, **kw) == BADARG and _v(**pair, **kw, mh=HH, mw=WW, fmt=_ffi.default_tensor_format()) == BADARG


def test_bad_params_and_format_structs_are_refused():
    for size in (0, 16, C.sizeof(_ffi.SlParams) - 8, C.sizeof(_ffi.SlParams) + 8):
        p = _ffi.default_params()
        p.struct_size = size
        for route in ROUTES:
            assert _v(**route, params=p) == BADARG and _v(**route, params=p, mh=HH, mw=WW, tb=None) == BADARG
    for field, value in (("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3), ("layout", -1),
                         ("layout", 2), ("std", 0.0), ("std", float("nan")), ("mean", float("inf"))):
        f = _ffi.default_tensor_format()
        if field in ("std", "mean"):
            getattr(f, field)[1] = value
        else:
            setattr(f, field, value)
        for pair in PAIRS:
            assert _a(fmt=f, **pair) == BADARG, (field, value)
        for route in ROUTES:
            assert _v(**route, fmt=f) == BADARG and _v(**route, fmt=f, mh=HH, mw=WW, cd=None) == BADARG, (field, value)


# ---- the stand-alone programs -----------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_the_per_pixel_arithmetic_equals_its_64_bit_restatement_under_the_host_sanitizers(tmp_path):
    """tests/post_math_check.cpp, a stand-alone program: csrc/post_math.hpp and csrc/view_geometry.hpp alone -- the generator's known
    answers, all 256 bytes x all 1021 values of G x a dozen sq, the write side's lane-to-pixel-index arithmetic on the GPU tests' shapes --
    built with the address and undefined-behaviour sanitizers."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "post_math_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", os.path.join(HERE, "post_math_check.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"^\d+ checks, 0 failures$", r.stdout, flags=re.M)
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr


def test_c_abi_argument_checks_of_the_post_entry_points_under_asan():
    """`make asan-post`: tests/abi_argcheck_post.c -- a stand-alone program -- against the library's HOST side built with AddressSanitizer:
    every refused call of the two entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if nothing has yet: a
    few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-post", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

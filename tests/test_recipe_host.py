"""The one-pass recipe on the host side (stainlib_amd.Recipe, recipe= / recipe_draw= on the batch methods, engine.normalize_stages_view*,
sl_normalize_stages_view / _view_affine / _view_elastic): the constructor, every refusal before any draw, the draw order, the replay
path's checkers, the header / binding / library agreement and the stand-alone C driver -- no GPU needed."""
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
from stainlib_amd.augmentation.hsb import hsb_codes
from stainlib_amd.augmentation.noise import noise_codes, tone_tables
from stainlib_amd.tile_view import ElasticWindows, elastic_grid_shape

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
RGB, OUT, D6, D2, AB, WIN, FLD = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x500100
SG, BS, AP, HC, CD, TB = 0x600000, 0x600100, 0x600200, 0x600300, 0x600400, 0x600501
N, HH, WW, OH, OW = 4, 64, 48, 40, 32
Q = 65536

_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def _augmenters():
    return dict(hed=stainlib_amd.HedLightColorAugmenter(), hsb=stainlib_amd.HsbLightColorAugmenter(),
                noise=stainlib_amd.GaussianNoiseAugmenter((1, 8)), tone=stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), None, (0.8, 1.25)),
                blur=stainlib_amd.GaussianBlurAugmenter((0.3, 2.0)), view=stainlib_amd.TileView((5, 7), rot90=False),
                affine=stainlib_amd.TileAffine((5, 5)), elastic=stainlib_amd.TileElastic((5, 5)))


def _methods():
    nz = stainlib_amd.MacenkoNormalizer()
    nz.stain_matrix_target, nz.maxC_target = np.array([[0.6, 0.7, 0.4], [0.2, 0.9, 0.4]]), np.array([[1.5, 1.1]])
    vz = stainlib_amd.VahadaneNormalizer()
    vz.stain_matrix_target, vz.maxC_target = nz.stain_matrix_target, nz.maxC_target
    sa = stainlib_amd.StainAugmentor("macenko")
    fmt = stainlib_amd.TensorFormat()
    return nz, [("transform_batch", lambda **k: nz.transform_batch(_TILES, **k)),
                ("vahadane transform_batch", lambda **k: vz.transform_batch(_TILES, **k)),
                ("augment_batch", lambda **k: nz.augment_batch(_TILES, _AB, **k)),
                ("augment_batch own", lambda **k: vz.augment_batch(_TILES, _AB, normalize=False, **k)),
                ("StainAugmentor", lambda **k: sa.augment_batch(_TILES, **k)),
                ("convert", lambda **k: fmt.convert(_TILES, **k))]


# ---- the constructor ----------------------------------------------------------------------------------------------------------------------------
def test_the_recipe_constructor():
    a = _augmenters()
    R = stainlib_amd.Recipe
    r = R(a["elastic"], a["hsb"], a["noise"], a["tone"])
    assert (r.view, r.color, r.noise, r.tone) == (a["elastic"], a["hsb"], a["noise"], a["tone"]) and "Recipe(view=TileElastic" in repr(r)
    for kw in (dict(view=a["view"]), dict(view=a["affine"]), dict(color=a["hed"]), dict(color=a["hsb"]), dict(noise=a["noise"]), dict(tone=a["tone"]),
               dict(view=stainlib_amd.TileView(4, shrink=2), color=a["hed"], tone=a["tone"]),
               dict(view=stainlib_amd.TileView(4, scale=(0.5, 1)), noise=a["noise"])):
        R(**kw)
    with pytest.raises(ValueError, match="an empty Recipe"):
        R()
    with pytest.raises(ValueError, match="view must be a stainlib_amd TileView, TileAffine or TileElastic"):
        R(view=(5, 5), noise=a["noise"])
    with pytest.raises(ValueError, match="color must be a stainlib_amd HedColorAugmenter or HsbColorAugmenter"):
        R(color=a["blur"])
    with pytest.raises(ValueError, match="color must be"):
        R(color=a["noise"])
    with pytest.raises(ValueError, match="color must be"):
        R(color=(a["hed"], a["hsb"]))                               # HED and HSB together: one colour stage
    with pytest.raises(ValueError, match="noise must be a stainlib_amd GaussianNoiseAugmenter"):
        R(noise=a["tone"])
    with pytest.raises(ValueError, match="tone must be a stainlib_amd ToneCurveAugmenter"):
        R(tone=a["noise"])
    for mode in ("0.19", "0.17", "experimental_log10"):             # the three chain modes, by name
        hed = stainlib_amd.augmentation.augmenter.HedColorAugmenter((-0.1, 0.1), (-0.1, 0.1), (-0.1, 0.1), (-0.1, 0.1), (-0.1, 0.1), (-0.1, 0.1),
                                                                    (0.05, 0.95), skimage_mode=mode)
        with pytest.raises(ValueError, match=f"skimage_mode '{mode}' .* goes through the hed_augment chain.*needs a HedColorAugmenter of skimage_mode '0.18'"):
            R(color=hed)


# ---- refusals: a ValueError that names its cause, before any draw ---------------------------------------------------------------------------------
def test_every_refusal_names_its_cause_and_draws_nothing():
    a = _augmenters()
    R = stainlib_amd.Recipe
    recipe = R(a["elastic"], a["hsb"], a["noise"], a["tone"])
    nz, methods = _methods()
    win = np.array([[0, 0, 0], [4, 4, 6]], dtype=np.int32)
    others = dict(view=a["view"], windows=win, hed=a["hed"], hed_sigmas=np.zeros((2, 3)), hed_biases=np.zeros((2, 3)), hsb=a["hsb"],
                  hsb_sigmas=np.zeros((2, 3)), blur=a["blur"], blur_sigmas=np.ones(2), noise=a["noise"], tone=a["tone"],
                  noise_sigmas=np.ones(2), tone_params=np.tile([0.0, 1.0, 1.0], (2, 1)))
    for name, call in methods:
        np.random.seed(3)
        for key, value in others.items():
            if name == "convert" and key.startswith(("hed", "hsb")):
                continue                                            # (convert has no such keyword)
            with pytest.raises(ValueError, match=f"recipe= does not go together with {key}=.*the recipe holds the call's view and every stage"):
                call(recipe=recipe, **{key: value})
        with pytest.raises(ValueError, match="recipe= does not go together with view=, noise="):
            call(recipe=recipe, view=a["view"], noise=a["noise"])
        with pytest.raises(ValueError, match="recipe_draw= goes with recipe="):
            call(recipe_draw=engine.RecipeDraw(None, None, None))
        with pytest.raises(ValueError, match="recipe must be a stainlib_amd.Recipe"):
            call(recipe=a["hsb"])
        with pytest.raises(ValueError, match="recipe must be a stainlib_amd.Recipe"):
            call(recipe=dict(view=a["view"]))
        with pytest.raises(ValueError, match="does not fit"):       # the view's own check, before any draw
            call(recipe=R(stainlib_amd.TileView(10), a["hsb"]))
        # accepted arguments: the call stops at the tile check (CPU tiles) -- AFTER the argument checks, BEFORE any draw
        for r in (recipe, R(a["affine"], a["hed"]), R(a["view"], a["hsb"], a["noise"]), R(None, a["hed"], None, a["tone"]), R(color=a["hsb"]),
                  R(noise=a["noise"]), R(stainlib_amd.TileView((4, 4), scale=(0.5, 1)), None, None, a["tone"])):
            with pytest.raises(ValueError, match=_TILE_CHECK):
                call(recipe=r)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, name                   # nothing was consumed by a refused call
    # a RecipeDraw whose parts do not match the recipe's stages, each part through the checker of its own keyword
    call = methods[0][1]
    gh, gw = elastic_grid_shape((5, 5), 32)
    ew = ElasticWindows(np.tile(np.array([[4 * Q, 5 * Q, Q, 0, 0, Q]], dtype=np.int32), (2, 1)), np.zeros((2, gh, gw, 2), dtype=np.int32))
    hsbd = engine.HsbDraw(np.zeros((2, 3)), np.zeros((2, 3), dtype=np.int32))
    hedd = engine.HedDraw(np.zeros((2, 3)), np.zeros((2, 3)), None)
    postd = engine.PostDraw(None, tone_tables(np.tile([0.0, 1.0, 1.0], (2, 1))), None, noise_codes(np.ones(2)))
    good = engine.RecipeDraw(ew, hsbd, postd)
    np.random.seed(3)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        call(recipe=recipe, recipe_draw=good)
    for draw, match in (((ew, hsbd, postd), "recipe_draw must be the engine.RecipeDraw"),
                        (good._replace(windows=None), "recipe_draw.windows does not match the recipe.*needs its windows"),
                        (good._replace(windows=ew.affine), "windows of an elastic view must be the stainlib_amd.ElasticWindows"),
                        (good._replace(windows=ElasticWindows(ew.affine[:1], ew.field)), "windows"),
                        (good._replace(windows=ElasticWindows(ew.affine, ew.field[:, :-1])), "field"),
                        (good._replace(color=None), "recipe_draw.color does not match the recipe.*HsbDraw"),
                        (good._replace(color=hedd), "recipe_draw.color does not match the recipe.*HsbDraw"),
                        (good._replace(color=engine.HsbDraw(None, np.zeros((3, 3), dtype=np.int32))), "recipe_draw.color.codes must have one row per tile"),
                        (good._replace(color=engine.HsbDraw(None, np.zeros((2, 3)))), "codes must hold \\(dhq, dsq, dvq\\)"),
                        (good._replace(post=None), "recipe_draw.post does not match the recipe.*PostDraw"),
                        (good._replace(post=postd._replace(tone_tables=None)), "recipe_draw.post.tone_tables does not match"),
                        (good._replace(post=postd._replace(noise_codes=None)), "recipe_draw.post.noise_codes does not match"),
                        (good._replace(post=postd._replace(tone_tables=np.zeros((2, 255), dtype=np.uint8))), "tone_params must hold"),
                        (good._replace(post=postd._replace(tone_tables=np.zeros((3, 256), dtype=np.uint8))), "one row per tile"),
                        (good._replace(post=postd._replace(noise_codes=np.zeros((3, 4), dtype=np.int32))), "one entry per tile"),
                        (good._replace(post=postd._replace(noise_codes=np.array([[28379, 0, 0, 0], [1, 0, 0, 0]], dtype=np.int32))), "sq must lie in")):
        with pytest.raises(ValueError, match=match):
            call(recipe=recipe, recipe_draw=draw)
    hed_recipe = R(None, a["hed"])
    for draw, match in ((engine.RecipeDraw(None, hsbd, None), "recipe_draw.color does not match the recipe.*HedDraw"),
                        (engine.RecipeDraw(ew, hedd, None), "recipe_draw.windows does not match the recipe: the recipe has no view"),
                        (engine.RecipeDraw(None, hedd, postd), "recipe_draw.post does not match the recipe: the recipe has no tone or noise"),
                        (engine.RecipeDraw(None, engine.HedDraw(np.zeros((3, 3)), np.zeros((2, 3)), None), None), "recipe_draw.color.sigmas must have one row"),
                        (engine.RecipeDraw(None, engine.HedDraw(np.zeros((2, 3)), np.zeros((2, 4)), None), None), "recipe_draw.color.biases must hold")):
        with pytest.raises(ValueError, match=match):
            call(recipe=hed_recipe, recipe_draw=draw)
    with pytest.raises(ValueError, match="recipe_draw.color does not match the recipe: the recipe has no colour stage"):
        call(recipe=R(noise=a["noise"]), recipe_draw=engine.RecipeDraw(None, hsbd, postd._replace(tone_tables=None)))
    # separate_batch and the Lab family's fused calls
    rz = stainlib_amd.ReinhardStainNormalizer()
    rz.target_means, rz.target_stds = (1.0, 2.0, 3.0), (1.0, 1.0, 1.0)
    for call in (lambda **k: rz.transform_batch(_TILES, **k), lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, **k)):
        with pytest.raises(ValueError, match="recipe= is not supported by the Lab family's fused calls.*TensorFormat.convert\\(u8, recipe=\\)"):
            call(recipe=recipe)
        with pytest.raises(ValueError, match="recipe= is not supported by the Lab family's fused calls"):
            call(recipe_draw=good)
    with pytest.raises(ValueError, match="recipe= is not supported by separate_batch"):
        nz.separate_batch(_TILES, recipe=recipe)
    # the engine calls: the stages
    w3, w6 = np.zeros((2, 3), dtype=np.int32), ew.affine
    t2, c2, h2 = postd.tone_tables, postd.noise_codes, hsb_codes(np.zeros((2, 3)))
    s2 = np.zeros((2, 3))
    ap = np.ones(2, dtype=np.int32)
    calls = (lambda **k: engine.normalize_stages_view(_TILES, w3, (5, 7), 6, **k),
             lambda **k: engine.normalize_stages_view_affine(_TILES, w6, (5, 5), Q, **k),
             lambda **k: engine.normalize_stages_view_elastic(_TILES, w6, ew.field, (5, 5), 32, Q, 0, **k))
    for call in calls:
        with pytest.raises(ValueError, match="a recipe call needs a stage"):
            call()
        with pytest.raises(ValueError, match="one colour stage"):
            call(hed_sigma=s2, hed_bias=s2, hed_applied=ap, hsb_codes=h2)
        for part in (dict(hed_sigma=s2), dict(hed_bias=s2, hed_applied=ap), dict(hed_sigma=s2, hed_bias=s2, tables=t2)):
            with pytest.raises(ValueError, match="hed_sigma, hed_bias and hed_applied go together"):
                call(**part)
        for mode in (1, 2, 3):
            with pytest.raises(ValueError, match="skimage_mode .* '0.18' \\(0\\) only"):
                call(hed_sigma=s2, hed_bias=s2, hed_applied=ap, skimage_mode=mode)
        with pytest.raises(ValueError, match="hed_sigma must have one row per tile"):
            call(hed_sigma=np.zeros((3, 3)), hed_bias=s2, hed_applied=ap)
        with pytest.raises(ValueError, match="hsb_codes must have one row per tile"):
            call(hsb_codes=np.zeros((3, 3), dtype=np.int32))
        with pytest.raises(ValueError, match="codes must hold \\(dhq, dsq, dvq\\)"):
            call(hsb_codes=np.zeros((2, 3)))
        with pytest.raises(ValueError, match="tables must have one row per tile"):
            call(tables=np.tile(t2[:1], (3, 1)))
        with pytest.raises(ValueError, match="sq must lie in"):
            call(codes=c2 - np.array([3000, 0, 0, 0], dtype=np.int32))
        with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
            call(codes=c2, fmt="float16")
        with pytest.raises(TypeError, match="unexpected keyword"):
            call(codes=c2, blur_codes=c2)
        for ok in (dict(tables=t2), dict(codes=c2), dict(hsb_codes=h2), dict(hed_sigma=s2, hed_bias=s2, hed_applied=ap),
                   dict(hsb_codes=h2, tables=t2, codes=c2), dict(hed_sigma=s2, hed_bias=s2, hed_applied=ap, codes=c2)):
            with pytest.raises(ValueError, match=_TILE_CHECK):
                call(**ok)
    after = np.random.uniform()
    np.random.seed(3)
    assert np.random.uniform() == after


# ---- the draw order and the replay path ----------------------------------------------------------------------------------------------------------
def test_the_draw_order_is_alpha_beta_then_colour_tone_noise_view_and_a_replay_hands_each_part_to_its_checker(monkeypatch):
    """the four draw functions and the engine calls replaced by stand-ins that record: the order of the draws, and what reaches the call"""
    n, h, w = 2, 9, 11
    order, seen, checked = [], {}, []
    fit = (torch.zeros((n, 2, 3), dtype=torch.float64), torch.ones((n, 2), dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "macenko_fit", lambda t, *a, **k: fit)
    monkeypatch.setattr(engine, "vahadane_fit", lambda t, *a, **k: fit + (None,))
    monkeypatch.setattr(engine, "hed_decide", lambda tiles, cutoff, **route: order.append("decide") or np.ones(n, dtype=np.int32))
    for cls in (stainlib_amd.MacenkoNormalizer, stainlib_amd.VahadaneNormalizer):
        monkeypatch.setattr(cls, "_target_on", lambda self, dev: (None, None))
    a = _augmenters()
    from stainlib_amd.augmentation.augmenter import HedColorAugmenter as hed_cls
    hsb_cls = stainlib_amd.HsbColorAugmenter
    for cls, tag in ((hed_cls, "color"), (hsb_cls, "color"), (stainlib_amd.ToneCurveAugmenter, "tone"), (stainlib_amd.GaussianNoiseAugmenter, "noise")):
        real = cls.randomize_batch
        monkeypatch.setattr(cls, "randomize_batch", lambda self, k, real=real, tag=tag: order.append(tag) or real(self, k))
    for cls in (stainlib_amd.TileView, stainlib_amd.TileAffine, stainlib_amd.TileElastic):       # (TileElastic.draw calls TileAffine.draw: once)
        real = cls.draw
        monkeypatch.setattr(cls, "draw", lambda self, k, hh, ww, real=real: (order[-1:] == ["view"] or order.append("view")) and None or real(self, k, hh, ww))

    def stand_in(name):
        def f(tiles, *args, **kw):
            seen.clear()
            seen.update(name=name, args=args, kw=kw)
            return "out"
        return f
    for name in ("normalize_stages_view", "normalize_stages_view_affine", "normalize_stages_view_elastic"):
        monkeypatch.setattr(engine, name, stand_in(name))
    R = stainlib_amd.Recipe
    nz, methods = _methods()
    cases = [(R(a["elastic"], a["hsb"], a["noise"], a["tone"]), ["color", "tone", "noise", "view"], "normalize_stages_view_elastic"),
             (R(a["affine"], a["hed"], a["noise"], a["tone"]), ["color", "tone", "noise", "view", "decide"], "normalize_stages_view_affine"),
             (R(a["view"], a["hsb"], None, a["tone"]), ["color", "tone", "view"], "normalize_stages_view"),
             (R(None, a["hed"], a["noise"]), ["color", "noise", "decide"], "normalize_stages_view"),
             (R(a["view"], None, a["noise"], a["tone"]), ["tone", "noise", "view"], "normalize_stages_view")]
    for name, call in methods:
        for recipe, want_order, entry in cases:
            del order[:]
            np.random.seed(77)
            res = call(recipe=recipe)
            after = np.random.uniform()
            np.random.seed(77)
            ab = stainlib_amd.StainJitter().draw(n) if name == "StainAugmentor" else _AB
            del order[:]
            color = recipe.color.randomize_batch(n) if recipe.color is not None else None
            tone = recipe.tone.randomize_batch(n) if recipe.tone is not None else None
            noise = recipe.noise.randomize_batch(n) if recipe.noise is not None else None
            win = recipe.view.draw(n, h, w) if recipe.view is not None else None
            assert np.random.uniform() == after, name                # and nothing else was consumed
            draw = res[-1]
            assert isinstance(draw, engine.RecipeDraw) and res[0] == "out" and len(res) == (2 if name == "convert" else 5), name
            assert seen["name"] == entry, (name, entry)
            kw = seen["kw"]
            if recipe.view is None:
                assert draw.windows is None and not np.asarray(seen["args"][0]).any() and seen["args"][1:3] == (None, 0)
            elif isinstance(win, ElasticWindows):
                assert np.array_equal(draw.windows.affine, win.affine) and np.array_equal(draw.windows.field, win.field)
                assert seen["args"][0] is draw.windows.affine and seen["args"][1] is draw.windows.field
            else:
                assert np.array_equal(draw.windows, win) and seen["args"][0] is draw.windows
            if isinstance(recipe.color, hsb_cls):
                assert isinstance(draw.color, engine.HsbDraw) and np.array_equal(draw.color.sigmas, color)
                assert np.array_equal(draw.color.codes, hsb_codes(color)) and kw["hsb_codes"] is draw.color.codes and "hed_sigma" not in kw
            elif recipe.color is not None:
                assert isinstance(draw.color, engine.HedDraw) and np.array_equal(draw.color.sigmas, color[0]) and np.array_equal(draw.color.biases, color[1])
                assert kw["hed_sigma"] is draw.color.sigmas and kw["hed_applied"] is draw.color.applied and kw["skimage_mode"] == 0
            else:
                assert draw.color is None and "hsb_codes" not in kw and "hed_sigma" not in kw
            assert np.array_equal(draw.post.tone_tables, tone[1]) if tone is not None else draw.post.tone_tables is None
            assert np.array_equal(draw.post.noise_codes, noise[1]) if noise is not None else draw.post.noise_codes is None
            assert kw.get("tables") is draw.post.tone_tables and kw.get("codes") is draw.post.noise_codes
            if "augment" in name or name == "StainAugmentor":
                assert np.array_equal(np.asarray(kw["alpha_beta"]), ab)
            else:
                assert "alpha_beta" not in kw
    # the order itself, and a replay: nothing is drawn, every part goes through the checker of its own keyword
    call = methods[2][1]
    for fn in ("_view_call", "_hed_rows", "_hsb_codes_rows", "_tone_arg", "_noise_arg"):
        real = getattr(engine, fn)
        monkeypatch.setattr(engine, fn, lambda *a, real=real, fn=fn, **k: checked.append(fn) or real(*a, **k))
    for recipe, want_order, entry in cases:
        del order[:]
        res = call(recipe=recipe)
        assert order == want_order, (order, want_order)
        del order[:], checked[:]
        np.random.seed(5)
        before = np.random.get_state()[1].copy()
        again = call(recipe=recipe, recipe_draw=res[-1])
        assert np.array_equal(np.random.get_state()[1], before) and order == [w for w in want_order if w == "decide"]
        want_checked = {"_view_call"} if recipe.view is not None else set()
        want_checked |= {"_hed_rows"} if isinstance(recipe.color, hed_cls) else ({"_hsb_codes_rows"} if recipe.color is not None else set())
        want_checked |= ({"_tone_arg"} if recipe.tone is not None else set()) | ({"_noise_arg"} if recipe.noise is not None else set())
        assert want_checked <= set(checked), (want_checked, checked)
        assert again[-1].windows is res[-1].windows
        if recipe.tone is not None:
            assert np.array_equal(again[-1].post.tone_tables, res[-1].post.tone_tables) and np.array_equal(seen["kw"]["tables"], res[-1].post.tone_tables)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------------
def _stages(sg=None, bs=None, ap=None, mode=0, hc=None, tb=None, cd=None, size=None):
    return _ffi.SlViewStages(C.sizeof(_ffi.SlViewStages) if size is None else size, sg, bs, ap, mode, hc, tb, cd)


def _calls(st, n=N, **kw):
    """the three entry points on the jitter route with a format, and on the raw route"""
    lib = _ffi.lib()
    p, f = _ffi.default_params(), _ffi.default_tensor_format()
    ref = C.byref(st) if st is not None else None
    out = []
    for route in ((D6, D2, D6, D2, AB, 0, C.byref(p), C.byref(f)), (None, None, None, None, None, 0, None, None)):
        out.append(lib.sl_normalize_stages_view(RGB, OUT, n, HH, WW, OH, OW, WIN, 7, 1, 0, 0, *route, ref, None))
        out.append(lib.sl_normalize_stages_view(RGB, OUT, n, HH, WW, OH, OW, WIN, 7, 1, HH, WW, *route, ref, None))
        out.append(lib.sl_normalize_stages_view_affine(RGB, OUT, n, HH, WW, OH, OW, WIN, Q, 0xffffff, *route, ref, None))
        out.append(lib.sl_normalize_stages_view_elastic(RGB, OUT, n, HH, WW, OH, OW, WIN, Q, FLD, 5, 4, 0, *route, ref, None))
    return out


def test_version_header_binding_and_library_agree():
    assert _ffi.lib().sl_version() == 600 and _ffi.EXPECTED_VERSION == 600        # an extension of ABI 600
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    parents = {"sl_normalize_stages_view": ("sl_normalize_post_view", 22, 2), "sl_normalize_stages_view_affine": ("sl_normalize_view_affine", 20, 0),
               "sl_normalize_stages_view_elastic": ("sl_normalize_view_elastic", 23, 0)}
    for name, (parent, count, dropped) in parents.items():
        assert name in declared and name in _ffi.EXPORTS
        proto = [p.strip() for p in re.search(r"^SL_API int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1).split(",")]
        pproto = [p.strip() for p in re.search(r"^SL_API int %s\((.*?)\);" % parent, hdr, flags=re.M | re.S).group(1).split(",")]
        res, args = _ffi._SIGNATURES[name]
        assert res is C.c_int and len(proto) == len(args) == count
        # the parent's arguments (for the fixed / resizing view without its tables and codes), then the struct, then the stream
        assert proto[:-2] == pproto[:len(pproto) - 1 - dropped] and proto[-2] == "const SlViewStages* stages" and proto[-1] == "void* stream"
        for p, a in zip(proto, args):
            if "SlParams" in p or "SlTensorFormat" in p or "SlViewStages" in p:
                assert a not in (C.c_int, C.c_void_p), p
            elif "uint32_t" in p:
                assert a is C.c_uint32, p
            else:
                assert a is (C.c_void_p if "*" in p else C.c_int), p
    # SlViewStages: the header's members, in order, are the binding's fields
    body = re.search(r"typedef struct SlViewStages \{(.*?)\} SlViewStages;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for decl in body.split(";"):
        if decl.strip():                                            # `const double *a, *b` -> a, b
            members += [m.strip().lstrip("* ") for m in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl.strip(), count=1).split(",")]
    assert members == [f[0] for f in _ffi.SlViewStages._fields_] == ["struct_size", "hed_sigma", "hed_bias", "hed_applied", "skimage_mode",
                                                                      "hsb_codes", "tone_tables", "noise_codes"]
    assert C.sizeof(_ffi.SlViewStages) == 64 and _ffi.SlViewStages.skimage_mode.offset == 32 and _ffi.SlViewStages.noise_codes.offset == 56
    nm = shutil.which("nm")
    assert nm is not None
    out = subprocess.run([nm, "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (sl_\w+)$", out, flags=re.M)) == declared


def test_refused_stages_and_an_empty_batch_through_the_binding():
    good = [_stages(SG, BS, AP), _stages(hc=HC), _stages(tb=TB, cd=CD), _stages(tb=TB), _stages(cd=CD), _stages(SG, BS, AP, tb=TB, cd=CD),
            _stages(hc=HC, cd=CD)]
    for st in good:
        assert _calls(st, n=0) == [0] * 8                           # n == 0: SL_OK, nothing launched
        assert _calls(st, n=-1) == [BADARG] * 8
    bad = [None, _stages(), _stages(SG, BS, AP, hc=HC), _stages(SG), _stages(bs=BS, ap=AP, tb=TB), _stages(SG, BS, cd=CD),
           _stages(SG, BS, AP, mode=1), _stages(hc=HC, mode=3), _stages(tb=TB, mode=-1), _stages(hc=HC + 2), _stages(cd=CD + 1),
           _stages(hc=HC, tb=TB, cd=CD + 3), _stages(hc=HC, size=0), _stages(hc=HC, size=16), _stages(hc=HC, size=C.sizeof(_ffi.SlViewStages) + 8)]
    for st in bad:
        assert _calls(st) == [BADARG] * 8 and _calls(st, n=0) == [BADARG] * 8


def test_c_abi_argument_checks_of_the_recipe_entry_points_under_asan():
    """`make asan-recipe`: tests/abi_argcheck_recipe.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the three entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if
    nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-recipe", "-j8"], capture_output=True, text=True,
                       timeout=1800)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

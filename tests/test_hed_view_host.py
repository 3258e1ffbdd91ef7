"""HED augmentation behind the apply pass (sl_normalize_sums, sl_normalize_hed_view, engine.normalize_sums / normalize_hed_view, hed= on
the batch methods) on the host side: header and binding agree, every bad argument is refused before anything is launched, a refused
call draws nothing and an accepted one draws in the documented order -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine
from tests.gpu_util import BAD_SHAPES, BAD_STATS, ROUTES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
INF = float("inf")
# device pointers: never read by the host side
RGB, OUT, D6, D2, AB, WIN, SG, BS, AP, SUMS = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x300400, 0x300500, 0x300600, 0x300700
N, H, W, OH, OW = 4, 64, 48, 40, 32


def _s(rgb=RGB, n=N, h=H, w=W, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0, params=None, lo=0.05, hi=0.95, sums=SUMS, ap=AP):
    return _ffi.lib().sl_normalize_sums(rgb, n, h, w, ms, cs, mt, ct, ab, bg, C.byref(params) if params is not None else None, lo, hi,
                                        sums, ap, None)


def _v(rgb=RGB, out=OUT, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0, params=None, fmt=None,
       sg=SG, bs=BS, ap=AP, mode=0):
    return _ffi.lib().sl_normalize_hed_view(rgb, out, n, h, w, oh, ow, win, d_mask, ms, cs, mt, ct, ab, bg,
                                            C.byref(params) if params is not None else None, C.byref(fmt) if fmt is not None else None,
                                            sg, bs, ap, mode, None)


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for name, count in (("sl_normalize_sums", 16), ("sl_normalize_hed_view", 22)):
        assert name in declared and name in _ffi.EXPORTS
        proto = re.search(r"^SL_API int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_ffi._SIGNATURES[name][1]) == count
    # sl_normalize_hed_view = sl_normalize_view's parameters, then sigma, bias, applied, skimage_mode, stream
    view, hed = _ffi._SIGNATURES["sl_normalize_view"][1], _ffi._SIGNATURES["sl_normalize_hed_view"][1]
    assert hed[:len(view) - 1] == view[:-1] and len(hed) == len(view) + 4
    assert _ffi.lib().sl_version() == 600                    # an extension of ABI 600: no existing struct or signature changes


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(sums=None), dict(sums=SUMS + 4), dict(sums=SUMS + 1), dict(lo=0.95, hi=0.05),
                                             dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=INF, hi=-INF)], ids=str)
def test_sums_bad_pointers_shapes_and_cutoffs_are_refused(kw):
    for route in ROUTES:
        args = {**route, **kw}
        assert _s(**args) == BADARG, args
        assert _s(**args, bg=1, params=_ffi.default_params(), ap=None) == BADARG, args


@pytest.mark.parametrize("kw", BAD_STATS, ids=str)
def test_sums_bad_statistics_are_refused(kw):
    assert _s(**kw) == BADARG and _s(**kw, lo=-INF, hi=INF, ap=None, params=_ffi.default_params()) == BADARG


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(win=None), dict(oh=0), dict(ow=0), dict(oh=-1), dict(oh=H + 1),
                                             dict(ow=W + 1), dict(d_mask=-1), dict(d_mask=8), dict(d_mask=1 << 20),
                                             dict(oh=H, ow=W, d_mask=7), dict(oh=H, ow=W, d_mask=1), dict(oh=W + 1, ow=W, d_mask=5),
                                             dict(n=1 << 22, h=32768, w=32768, oh=32768, ow=32768),
                                             dict(sg=None), dict(bs=None), dict(ap=None), dict(mode=-1), dict(mode=4), dict(mode=1 << 30),
                                             dict(mode=1), dict(mode=2), dict(mode=3)], ids=str)
def test_hed_view_bad_pointers_shapes_masks_and_modes_are_refused(kw):
    for route in ROUTES:
        args = {**route, **kw}
        assert _v(**args) == BADARG, args
        assert _v(**args, bg=1, params=_ffi.default_params(), fmt=_ffi.default_tensor_format()) == BADARG, args


@pytest.mark.parametrize("kw", BAD_STATS, ids=str)
def test_hed_view_bad_statistics_are_refused(kw):
    assert _v(**kw) == BADARG and _v(**kw, d_mask=6, oh=H, ow=W, fmt=_ffi.default_tensor_format()) == BADARG


def test_bad_params_and_format_structs_are_refused():
    for size in (0, 16, C.sizeof(_ffi.SlParams) - 8, C.sizeof(_ffi.SlParams) + 8):
        p = _ffi.default_params()
        p.struct_size = size
        for route in ROUTES:
            assert _s(**route, params=p) == BADARG and _v(**route, params=p) == BADARG
    p = _ffi.default_params()
    p.two_sweep = 9
    assert _s(params=p) == BADARG and _v(params=p) == BADARG
    for field, value in (("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3), ("layout", -1),
                         ("layout", 2), ("std", 0.0), ("std", float("nan")), ("mean", INF)):
        f = _ffi.default_tensor_format()
        if field in ("std", "mean"):
            getattr(f, field)[1] = value
        else:
            setattr(f, field, value)
        for route in ROUTES:
            assert _v(**route, fmt=f) == BADARG, (field, value)


# ---- the Python surface: ValueError before the device is touched (the tiles are CPU tensors: reaching the tile check raises ValueError
# too, "expected a contiguous CUDA uint8 tensor", so every case matches on its own message) -------------------------------------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_M, _MC = torch.zeros((2, 2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.float64)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
_WIN = np.array([[0, 0, 0], [4, 4, 6]], dtype=np.int32)
_SG = np.zeros((2, 3))
_AP = np.ones(2, dtype=np.int32)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def test_engine_calls_carry_normalize_views_checks():
    hv = lambda *a, **k: engine.normalize_hed_view(_TILES, _WIN, (5, 7), 6, _SG, _SG, _AP, 0, *a, **k)       # noqa: E731
    for call in (hv, lambda *a, **k: engine.normalize_sums(_TILES, *a, **k)):
        with pytest.raises(ValueError, match="go together"):
            call(_M, _MC, _M[0], None, _AB)
        with pytest.raises(ValueError, match="M_src=None is the view of the tiles' own bytes"):
            call(None, _MC)
        with pytest.raises(ValueError, match="M_src=None is the view of the tiles' own bytes"):
            call(alpha_beta=_AB)
        with pytest.raises(ValueError, match="M_src and maxC_src go together"):
            call(_M, None, None, None, _AB)
        with pytest.raises(ValueError, match="needs a target"):
            call(_M, _MC)
        with pytest.raises(ValueError, match="alpha_beta must"):
            call(_M, _MC, None, None, np.zeros((2, 3)))
        with pytest.raises(ValueError, match="alpha_beta must have one row per tile"):
            call(_M, _MC, None, None, np.zeros((3, 4)))
        with pytest.raises(ValueError, match="params must be"):
            call(params=0.01)
        with pytest.raises(ValueError, match=_TILE_CHECK):                       # accepted: the call goes on to the tiles themselves
            call(_M, _MC, None, None, _AB)
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        hv(fmt="float16")
    with pytest.raises(ValueError, match="outside the 9 x 11 tile"):
        engine.normalize_hed_view(_TILES, [[0, 0, 0], [5, 4, 6]], (5, 7), 6, _SG, _SG, _AP)
    with pytest.raises(ValueError, match="outside d_mask"):
        engine.normalize_hed_view(_TILES, [[0, 0, 1], [0, 0, 0]], (5, 7), 6, _SG, _SG, _AP)
    with pytest.raises(ValueError, match="does not fit"):
        engine.normalize_hed_view(_TILES, _WIN, (10, 5), 6, _SG, _SG, _AP)
    with pytest.raises(ValueError, match="hed_sigma must hold"):
        engine.normalize_hed_view(_TILES, _WIN, (5, 7), 6, np.zeros((2, 4)), _SG, _AP)
    with pytest.raises(ValueError, match="hed_bias must have one row per tile"):
        engine.normalize_hed_view(_TILES, _WIN, (5, 7), 6, _SG, np.zeros((3, 3)), _AP)
    with pytest.raises(ValueError, match="skimage_mode must be"):
        engine.normalize_hed_view(_TILES, _WIN, (5, 7), 6, _SG, _SG, _AP, 4)
    with pytest.raises(ValueError, match="hed_applied must hold"):
        engine.normalize_hed_view(_TILES, _WIN, (5, 7), 6, _SG, _SG, None)
    for bad in ((0.95, 0.05), (float("nan"), 1.0), 0.5, (0.1, 0.2, 0.3), "ab"):
        with pytest.raises(ValueError, match="cutoff must be a pair"):
            engine.normalize_sums(_TILES, cutoff=bad)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        engine.normalize_sums(_TILES, cutoff=(-INF, INF))


def _methods():
    nz = stainlib_amd.MacenkoNormalizer()
    nz.stain_matrix_target, nz.maxC_target = np.array([[0.6, 0.7, 0.4], [0.2, 0.9, 0.4]]), np.array([[1.5, 1.1]])
    sa = stainlib_amd.StainAugmentor("macenko")
    return nz, sa, [("transform_batch", lambda **k: nz.transform_batch(_TILES, **k)),
                    ("augment_batch", lambda **k: nz.augment_batch(_TILES, _AB, **k)),
                    ("augment_batch own", lambda **k: nz.augment_batch(_TILES, _AB, normalize=False, **k)),
                    ("StainAugmentor", lambda **k: sa.augment_batch(_TILES, **k))]


def test_bad_hed_arguments_are_value_errors_and_draw_nothing():
    aug = stainlib_amd.HedLightColorAugmenter()
    view = stainlib_amd.TileView((5, 7), rot90=False)
    for name, call in _methods()[2]:
        np.random.seed(3)
        with pytest.raises(ValueError, match="hed must be a stainlib_amd HedColorAugmenter"):
            call(hed="light")
        with pytest.raises(ValueError, match="hed must be a stainlib_amd HedColorAugmenter"):
            call(hed=stainlib_amd.StainJitter(), view=view)
        with pytest.raises(ValueError, match="go with hed="):
            call(hed_sigmas=_SG)
        with pytest.raises(ValueError, match="go with hed="):
            call(hed_biases=_SG, view=view)
        with pytest.raises(ValueError, match="hed_sigmas and hed_biases go together"):
            call(hed=aug, hed_sigmas=_SG)
        with pytest.raises(ValueError, match="hed_sigmas must hold"):
            call(hed=aug, hed_sigmas=np.zeros((2, 4)), hed_biases=_SG)
        with pytest.raises(ValueError, match="hed_sigmas must hold"):
            call(hed=aug, hed_sigmas=np.zeros(6), hed_biases=_SG)
        with pytest.raises(ValueError, match="hed_biases must have one row per tile"):
            call(hed=aug, hed_sigmas=_SG, hed_biases=np.zeros((3, 3)))
        with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
            call(hed=aug, view=(5, 7))
        with pytest.raises(ValueError, match="windows= goes with view="):
            call(hed=aug, windows=_WIN)
        with pytest.raises(ValueError, match="does not fit"):
            call(hed=aug, view=stainlib_amd.TileView(10))
        # accepted arguments: the call stops at the tile check (CPU tiles) -- AFTER the argument checks, BEFORE any draw
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(hed=aug)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(hed=aug, view=view)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, name                    # nothing was consumed by a refused call
    with pytest.raises(ValueError, match=_TILE_CHECK):
        aug.transform_batch(_TILES, view=view)
    with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
        aug.transform_batch(_TILES, view=(5, 7))
    with pytest.raises(ValueError, match="hed_sigmas must have one row per tile"):
        aug.transform_batch(_TILES, np.zeros((3, 3)), _SG, view=view)


def test_the_draw_order_is_alpha_beta_then_hed_then_windows(monkeypatch):
    """the engine calls replaced by stand-ins that record what they are handed: the global numpy stream gives alpha_beta (where the method
    draws one), then six uniforms per tile (sigma H, E, D, bias H, E, D), then the windows -- and nothing else"""
    n, h, w = 2, 9, 11
    seen = {}
    fit = (torch.zeros((n, 2, 3), dtype=torch.float64), torch.ones((n, 2), dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "macenko_fit", lambda t, *a, **k: fit)
    monkeypatch.setattr(stainlib_amd.MacenkoNormalizer, "_target_on", lambda self, dev: (None, None))
    monkeypatch.setattr(engine, "hed_decide", lambda t, cutoff, **route: seen.update(cutoff=tuple(cutoff), route=route) or "applied")

    def hed_view(tiles, win, size, d_mask, sig, bia, applied, mode=0, **kw):
        seen.update(win=win, size=size, d_mask=d_mask, sig=sig, bia=bia, applied=applied, mode=mode, kw=kw)
        return "out"
    monkeypatch.setattr(engine, "normalize_hed_view", hed_view)
    aug = stainlib_amd.HedStrongColorAugmenter()
    view = stainlib_amd.TileView((5, 5))
    nz, sa, methods = _methods()
    for name, call in methods:
        for with_view in (True, False):
            np.random.seed(77)
            res = call(hed=aug, **(dict(view=view) if with_view else {}))
            after = np.random.uniform()
            np.random.seed(77)
            ab = stainlib_amd.StainJitter().draw(n) if name == "StainAugmentor" else _AB
            sig = np.empty((n, 3))
            bia = np.empty((n, 3))
            for t in range(n):
                sig[t] = [np.random.uniform(-1.0, 1.0) for _ in range(3)]
                bia[t] = [np.random.uniform(-1.0, 1.0) for _ in range(3)]
            win = view.draw(n, h, w) if with_view else None
            assert np.random.uniform() == after, name                # and nothing else was consumed
            assert np.array_equal(seen["sig"], sig) and np.array_equal(seen["bia"], bia), name
            assert np.array_equal(np.asarray(seen["route"]["alpha_beta"]), ab) if "augment" in name or name == "StainAugmentor" else \
                "alpha_beta" not in seen["route"]
            assert seen["cutoff"] == (0.05, 0.95) and seen["mode"] == 0 and seen["applied"] == "applied"
            draw = res[-1]
            assert isinstance(draw, engine.HedDraw) and draw.applied == "applied" and draw.sigmas is seen["sig"] and res[0] == "out"
            if with_view:
                assert len(res) == 6 and np.array_equal(res[4], win) and np.array_equal(seen["win"], win)
                assert (seen["size"], seen["d_mask"]) == ((5, 5), 7)
            else:                                                    # the full tile, code 0
                assert len(res) == 5 and (seen["size"], seen["d_mask"]) == (None, 0) and not np.asarray(seen["win"]).any()
    # given draws: nothing but the windows is consumed
    np.random.seed(5)
    res = nz.transform_batch(_TILES, hed=aug, hed_sigmas=_SG, hed_biases=_SG, view=view)
    after = np.random.uniform()
    np.random.seed(5)
    assert np.array_equal(res[4], view.draw(n, h, w)) and np.random.uniform() == after and res[5].sigmas is _SG


def test_c_abi_argument_checks_of_the_hed_view_entry_points_under_asan():
    """`make asan-hedview`: tests/abi_argcheck_hedview.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the two entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if
    nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-hedview", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

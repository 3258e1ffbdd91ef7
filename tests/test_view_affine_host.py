"""The affine view (sl_normalize_view_affine, sl_view_planes_affine, TileAffine) on the host side: the numpy definition against the
existing views' rules, the draws, the constructor's limit, the range checks, the exports and their binding, every refused combination
before the library is called and without a draw, the C argument checks under AddressSanitizer, and the kernels' geometry lane by lane
on the CPU -- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine, tile_view
from stainlib_amd.tile_view import (AFFINE_MAX_R, AFFINE_Q as Q, TileAffine, affine_check_windows, affine_coords, affine_nearest,
                                    affine_resample, affine_row_sums, view_planes_reference)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 23, 31
DIHEDRAL = {0: (1, 0, 0, 1), 1: (0, 1, -1, 0), 2: (-1, 0, 0, -1), 3: (0, -1, 1, 0), 4: (1, 0, 0, -1), 5: (0, 1, 1, 0), 6: (-1, 0, 0, 1),
            7: (0, -1, -1, 0)}


def _img(seed=0, h=H, w=W):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ---- 1. the definition has the properties that tie it to the existing views -----------------------------------------------------------------
def test_identity():
    full = _img()
    row = [H * Q // 2, W * Q // 2, Q, 0, 0, Q]
    assert np.array_equal(affine_resample(full, row, (H, W)), full)
    assert np.array_equal(affine_nearest(full[..., 0].astype(np.int64) - 300, row, (H, W)), full[..., 0].astype(np.int64) - 300)
    Y, X = affine_coords(row, (H, W))
    assert Y.dtype == np.int64 and np.array_equal(Y[:, 0], np.arange(H) * Q + Q // 2) and np.array_equal(X[0], np.arange(W) * Q + Q // 2)


@pytest.mark.parametrize("size", [(8, 12), (7, 7), (9, 4)])
def test_the_eight_signed_permutations_are_the_dihedral_views(size):
    full = _img(1)
    oh, ow = size
    planes = np.arange(H * W, dtype=np.int32).reshape(1, H, W)
    for d in range(8):
        y0, x0 = 3 + d % 3, 5 + d % 4
        wh, ww = (ow, oh) if d & 1 else (oh, ow)
        row = [(2 * y0 + wh) * Q // 2, (2 * x0 + ww) * Q // 2] + [Q * v for v in DIHEDRAL[d]]
        win = full[y0:y0 + wh, x0:x0 + ww]
        want = np.rot90(win[:, ::-1] if d & 4 else win, d & 3)
        assert np.array_equal(affine_resample(full, row, size), want), d
        ref = view_planes_reference(planes, [[y0, x0, d]], size)[0]
        assert np.array_equal(affine_nearest(planes[0], row, size, -1), ref), d


def test_2I_is_the_shrink_2_box_rule_and_4I_is_not_the_4_box():
    full = _img(2, 24, 32)
    y0, x0, oh, ow = 2, 4, 9, 11
    row = [(y0 + oh) * Q, (x0 + ow) * Q, 2 * Q, 0, 0, 2 * Q]
    box = full[y0:y0 + 2 * oh, x0:x0 + 2 * ow].astype(np.int64).reshape(oh, 2, ow, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(affine_resample(full, row, (oh, ow)), ((box + 2) >> 2).astype(np.uint8))
    ref = view_planes_reference(np.moveaxis(full, 2, 0)[None], [[y0, x0, 0]], (oh, ow), shrink=2, mode="area")[0]
    assert np.array_equal(affine_resample(full, row, (oh, ow)), np.moveaxis(ref, 0, 2))
    # 4 I: four taps, the middle 2 x 2 of every 4 x 4 box -- NOT the 16-pixel mean
    oh, ow = 5, 7
    row4 = [(y0 + 2 * oh) * Q, (x0 + 2 * ow) * Q, 4 * Q, 0, 0, 4 * Q]
    got = affine_resample(full, row4, (oh, ow))
    win = full[y0:y0 + 4 * oh, x0:x0 + 4 * ow].astype(np.int64).reshape(oh, 4, ow, 4, 3)
    assert np.array_equal(got, ((win[:, 1:3, :, 1:3].sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8))
    assert not np.array_equal(got, ((win.sum(axis=(1, 3)) + 8) >> 4).astype(np.uint8))


def test_outside_the_tile_is_the_fill_with_the_stated_weights():
    full = _img(3)
    fill = (10, 30, 200)
    assert (affine_resample(full, [-50 * Q, W * Q // 2, Q, 0, 0, Q], (6, 8), fill) == np.array(fill, dtype=np.uint8)).all()
    assert (affine_resample(full, [H * Q // 2, (W + 40) * Q, 0, Q, -Q, 0], (6, 8), 77) == 77).all()
    assert (affine_nearest(full[..., 0], [-50 * Q, 0, Q, 0, 0, Q], (6, 8), 9) == 9).all()
    # a view whose rows sit a quarter pixel above the pixel centres, its first row half outside: ky = -1, fy = 192 --
    # b = (64 fill + 192 p + 128) >> 8 in row 0, the blend of rows i - 1 and i below
    oh, ow = 4, W
    row = [oh * Q // 2 - Q // 4, W * Q // 2, Q, 0, 0, Q]
    got = affine_resample(full, row, (oh, ow), fill).astype(np.int64)
    f = np.array(fill, dtype=np.int64)
    p = full.astype(np.int64)
    assert np.array_equal(got[0], (256 * (64 * f + 192 * p[0]) + 32768) >> 16)
    assert np.array_equal(got[1], (256 * (64 * p[0] + 192 * p[1]) + 32768) >> 16)
    # nearest at the same coordinates: Y >> 16 = i - 1 for i >= 1 ... no: Y = (i + 1/4) Q, so the element is row i itself
    assert np.array_equal(affine_nearest(full[..., 1], row, (oh, ow), 0), full[:oh, :, 1])
    # a corner tap: three taps outside, weights (256 - fy)(256 - fx) ... on the one inside
    row = [-Q // 4, -Q // 4, Q, 0, 0, Q]                                                       # output (0, 0) at (-1/4, -1/4): ty = -3/4
    got = affine_resample(full, row, (1, 1), fill).astype(np.int64)[0, 0]
    assert np.array_equal(got, (192 * (192 * f + 64 * f) + 64 * (192 * f + 64 * p[0, 0]) + 32768) >> 16)


# ---- 2. the draws --------------------------------------------------------------------------------------------------------------------------
def _by_hand(v, n, h, w):
    rows = []
    for _ in range(n):
        th = np.radians(np.random.uniform(*v.rotate))
        z = np.exp(np.random.uniform(np.log(v.zoom[0]), np.log(v.zoom[1])))
        t = np.tan(np.radians(np.random.uniform(*v.shear)))
        e = -1.0 if np.random.randint(2) and v.flip else 1.0
        ty = np.random.uniform(-v.translate[0], v.translate[0])
        tx = np.random.uniform(-v.translate[1], v.translate[1])
        c, s = np.cos(th), np.sin(th)
        rows.append([int(np.rint(65536 * x)) for x in ((0.5 + ty) * h, (0.5 + tx) * w, c / z, e * (c * t - s) / z, s / z, e * (s * t + c) / z)])
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize("flip", [True, False])
def test_draw_makes_six_draws_per_tile_in_the_stated_order(flip):
    v = TileAffine((40, 56), rotate=(-30, 75), zoom=(0.8, 1.25), shear=(-10, 5), translate=(0.1, 0.2), flip=flip)
    np.random.seed(3)
    win = v.draw(7, 96, 80)
    after = np.random.uniform()
    np.random.seed(3)
    want = _by_hand(v, 7, 96, 80)
    assert win.dtype == np.int32 and win.shape == (7, 6) and np.array_equal(win, want)
    assert np.random.uniform() == after                      # the stream stands where six draws per tile leave it, flip or not
    np.random.seed(3)
    assert np.array_equal(v.draw(7, 96, 80), win)
    affine_check_windows(win, 7, 96, 80, (40, 56), v.bound)
    det = win[:, 2].astype(np.int64) * win[:, 5] - win[:, 3].astype(np.int64) * win[:, 4]
    assert (det > 0).all() if not flip else ((det < 0).any() and (det > 0).any())
    assert v.draw(0, 96, 80).shape == (0, 6)


# ---- 3. the constructor's limit --------------------------------------------------------------------------------------------------------------
def test_constructor_refuses_what_could_pass_the_row_sum_limit():
    for kw, match in ((dict(rotate=(10, -10)), "rotate must be a pair"), (dict(zoom=(1.2, 0.8)), "zoom must be a pair"),
                      (dict(shear=(5, -5)), "shear must be a pair"), (dict(zoom=(0, 1)), "0 < lo"), (dict(zoom=(-1, 1)), "0 < lo"),
                      (dict(rotate=(0, np.inf)), "finite"), (dict(shear=(0, 90)), r"\(-90, 90\)"), (dict(translate=1.5), "translate"),
                      (dict(translate=(-0.1, 0)), "translate"), (dict(fill=256), "fill"), (dict(fill=(1, 2)), "fill"), (dict(fill=1.5), "fill"),
                      (dict(size=0), "size"),
                      (dict(zoom=(0.5, 1)), "at most 2"),                                       # sqrt 2 / 0.5 at 45 degrees
                      (dict(zoom=(0.7, 1)), "at most 2"),                                       # sqrt 2 / 0.7 = 2.02
                      (dict(rotate=(0, 0), zoom=(0.5, 1)), "at most 2"),                        # exactly 2: the + 1 of the rounding
                      (dict(rotate=(0, 0), shear=(0, 46)), "at most 2"),                        # 1 + tan 46 > 2
                      (dict(shear=(-30, 30), zoom=(0.9, 1)), "at most 2")):                     # sqrt((1 + tan 30)^2 + 1) / 0.9 = 2.07
        with pytest.raises(ValueError, match=match):
            TileAffine(**kw)


def _extreme_rows(v):
    """the integer rows at every corner of the ranges, on a fine grid of angles, both orientations"""
    rows = []
    for th in np.radians(np.unique(np.concatenate([np.linspace(v.rotate[0], v.rotate[1], 721), v.rotate]))):
        for z in v.zoom:
            for ph in v.shear:
                for e in (1.0, -1.0):
                    c, s, t = np.cos(th), np.sin(th), np.tan(np.radians(ph))
                    rows.append([0, 0] + [int(np.rint(65536 * x)) for x in (c / z, e * (c * t - s) / z, s / z, e * (s * t + c) / z)])
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("kw", [dict(zoom=(2 ** -0.5 * 1.00002, 1.5)),                          # any angle at the smallest zoom that passes
                                dict(rotate=(0, 0), zoom=(0.50001, 2)),
                                dict(rotate=(-10, 10), shear=(-20, 20), zoom=(0.76, 1)),
                                dict(rotate=(0, 0), shear=(-44.99, 44.99)),
                                dict(rotate=(80, 100), zoom=(0.58, 0.9)),
                                dict(zoom=(0.773, 1.2), shear=(-10, 10))])
def test_ranges_at_the_limit_pass_and_their_extreme_draws_are_in_range(kw):
    v = TileAffine(**kw)
    r = affine_row_sums(_extreme_rows(v))
    assert r.max() <= v.bound <= AFFINE_MAX_R
    assert v.bound - r.max() < 0.06 * Q, (v.bound, int(r.max()))       # the bound is tight: within 6 percent of a pixel of an extreme
    np.random.seed(9)
    win = v.draw(200, 512, 640)
    assert affine_row_sums(win).max() <= v.bound
    affine_check_windows(win, 200, 512, 640, None, v.bound)
    # a hair more is refused
    if "zoom" in kw:
        with pytest.raises(ValueError, match="at most 2"):
            TileAffine(**dict(kw, zoom=(kw["zoom"][0] * 0.98, kw["zoom"][1])))


def test_out_size_and_bound():
    v = TileAffine()
    assert v.out_size(100, 60) == (100, 60) and TileAffine(48).out_size(8, 8) == (48, 48) and TileAffine((3, 8192)).out_size(8192, 1) == (3, 8192)
    for size, hw in (((8193, 4), (8, 8)), (None, (8193, 8)), (4, (8, 8193))):
        with pytest.raises(ValueError, match="8192"):
            TileAffine(size).out_size(*hw)
    assert v.bound == int(np.ceil(65536 * np.sqrt(2) * (1 + 1e-12))) + 1 == 92683
    assert TileAffine(rotate=(0, 0)).bound == int(np.ceil(65536 * (1 + 1e-12))) + 1 == Q + 2
    assert v.fill == (255, 255, 255) and TileAffine(fill=(1, 2, 3)).fill_rgb == 1 | 2 << 8 | 3 << 16


# ---- 4. the range check of host windows ------------------------------------------------------------------------------------------------------
def test_affine_check_windows():
    good = np.array([[5 * Q, 7 * Q, Q, -Q, Q, Q], [-(1 << 28), 12 * Q + (1 << 28), 0, 0, 0, 0]], dtype=np.int32)
    out = affine_check_windows(good, 2, 10, 12)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, good)
    assert np.array_equal(affine_check_windows(torch.from_numpy(good), 2, 10, 12, (4, 4), AFFINE_MAX_R), good)
    assert np.array_equal(affine_check_windows(good.astype(np.int64).tolist(), 2, 10, 12), good)
    bad = lambda k, col, val: np.concatenate([good[:k], [[val if c == col else good[k, c] for c in range(6)]], good[k + 1:]]).astype(np.int64)
    for call, match in ((lambda: affine_check_windows(None, 2, 10, 12), r"\(N, 6\) int32 array \(TileAffine.draw\)"),
                        (lambda: affine_check_windows(good[:1], 2, 10, 12), r"\(2, 6\) array, not one of shape \(1, 6\)"),
                        (lambda: affine_check_windows(good[:, :5], 2, 10, 12), "not one of shape"),
                        (lambda: affine_check_windows(good.reshape(-1), 2, 10, 12), "not one of shape"),
                        (lambda: affine_check_windows(good.astype(np.float32), 2, 10, 12), "integer array"),
                        (lambda: affine_check_windows("x", 2, 10, 12), "integer array"),
                        (lambda: affine_check_windows(bad(0, 3, -Q - 1), 2, 10, 12), r"tile 0 .* row sum 131073 .* above 2 Q"),
                        (lambda: affine_check_windows(bad(1, 4, 2 * Q + 1), 2, 10, 12), "tile 1 .* above 2 Q"),
                        (lambda: affine_check_windows(good, 2, 10, 12, None, 2 * Q - 1), "tile 0 .* bound max_r = 131071"),
                        (lambda: affine_check_windows(good, 2, 10, 12, None, 0), "max_r"),
                        (lambda: affine_check_windows(good, 2, 10, 12, None, 2 * Q + 1), "max_r"),
                        (lambda: affine_check_windows(bad(1, 0, -(1 << 28) - 1), 2, 10, 12), "tile 1 .* centre cy"),
                        (lambda: affine_check_windows(bad(0, 0, 10 * Q + (1 << 28) + 1), 2, 10, 12), "tile 0 .* centre cy"),
                        (lambda: affine_check_windows(bad(1, 1, 12 * Q + (1 << 28) + 1), 2, 10, 12), "centre cx"),
                        (lambda: affine_check_windows(bad(0, 1, -(1 << 31)), 2, 10, 12), "centre cx"),
                        (lambda: affine_check_windows(good, 2, 8193, 12), "8192"),
                        (lambda: affine_check_windows(good, 2, 10, 8193), "8192"),
                        (lambda: affine_check_windows(good, 2, 10, 12, (8193, 1)), "8192"),
                        (lambda: affine_check_windows(good, 2, 10, 12, (1, 8193)), "8192")):
        with pytest.raises(ValueError, match=match):
            call()


# ---- 5. the exports ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_exports():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    ctype = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    want = {"sl_normalize_view_affine": ["const uint8_t* rgb", "void* out", "int n", "int h", "int w", "int oh", "int ow", "const int32_t* windows",
                                         "int max_r", "uint32_t fill_rgb", "const double* M_src", "const double* maxC_src", "const double* M_tgt",
                                         "const double* maxC_tgt", "const double* alpha_beta", "int augment_background", "const SlParams* params",
                                         "const SlTensorFormat* fmt", "void* stream"],
            "sl_view_planes_affine": ["const void* planes", "void* out", "int n", "int c", "int h", "int w", "int elem_bytes", "int oh", "int ow",
                                      "const int32_t* windows", "int max_r", "uint64_t fill_bits", "void* stream"]}
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, params in want.items():
        proto = re.search(r"^SL_API int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")] == params
        res, args = _ffi._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params)
        for p, a in zip(params, args):
            if "SlParams" in p or "SlTensorFormat" in p:
                assert a is C.POINTER(_ffi.SlParams if "SlParams" in p else _ffi.SlTensorFormat), p
            else:
                assert a is (C.c_void_p if "*" in p else ctype[p.split()[0]]), p
        assert re.search(r"\bT %s$" % name, nm, flags=re.M), name
        fn = getattr(_ffi.lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert _ffi.lib().sl_version() == 600 == _ffi.EXPECTED_VERSION


def test_the_library_refuses_bad_calls_before_a_launch():
    """a few of the refusals through the binding (the whole list: the AddressSanitizer driver below); the pointers are never read"""
    f = _ffi.lib().sl_normalize_view_affine
    good = [0x100000, 0x200000, 4, 64, 48, 8, 8, 0x300000, Q, 0] + [None] * 5 + [0, None, None, None]
    for i, v in ((0, None), (1, None), (7, None), (2, 0), (3, 8193), (4, 8193), (5, 8193), (6, 8193), (5, 0), (8, 0), (8, 2 * Q + 1), (9, 1 << 24),
                 (11, 0x400000)):
        a = list(good)
        a[i] = v
        assert f(*a) == -1, (i, v)
    f = _ffi.lib().sl_view_planes_affine
    good = [0x100000, 0x200000, 4, 3, 64, 48, 2, 8, 8, 0x300000, Q, 0, None]
    for i, v in ((0, None), (1, None), (9, None), (2, 0), (3, -1), (6, 3), (0, 0x100001), (4, 8193), (8, 8193), (10, 0), (10, 2 * Q + 1)):
        a = list(good)
        a[i] = v
        assert f(*a) == -1, (i, v)


# ---- 6. every refusal before the library is called, nothing drawn ------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(engine, "_call", lambda name, *a: pytest.fail(f"{name} was called"))


def _undrawn(call, match):
    np.random.seed(11)
    before = np.random.get_state()
    with pytest.raises(ValueError, match=match):
        call()
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_calls_that_refuse_an_affine_view_name_it_and_draw_nothing(no_library):
    tiles = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    v = TileAffine(8)
    ab = np.tile([1.0, 0.0, 1.0, 0.0], (2, 1))
    hed = stainlib_amd.HedLightColorAugmenter()
    nz = stainlib_amd.MacenkoNormalizer()
    for cls in (stainlib_amd.MacenkoNormalizer, stainlib_amd.VahadaneNormalizer):
        _undrawn(lambda: cls().transform_batch(tiles, view=v, hed=hed), "an affine view .* not supported by the HED stage")
        _undrawn(lambda: cls().augment_batch(tiles, ab, normalize=False, view=v, hed=hed), "affine view .* HED stage")
        _undrawn(lambda: cls().separate_batch(tiles, normalize=False, view=v), "affine view .* not supported by separate_batch")
    _undrawn(lambda: stainlib_amd.StainAugmentor("macenko").augment_batch(tiles, view=v, hed=hed), "affine view .* HED stage")
    _undrawn(lambda: hed.transform_batch(tiles, view=v), "affine view .* HED stage")
    rz = stainlib_amd.ReinhardStainNormalizer()
    rz.target_means, rz.target_stds = np.zeros(3), np.ones(3)
    _undrawn(lambda: rz.transform_batch(tiles, view=v), "affine view .* not supported by the Lab-family calls")
    _undrawn(lambda: stainlib_amd.LuminosityStandardizer.standardize_batch(tiles, view=v), "affine view .* Lab-family")
    _undrawn(lambda: engine.reinhard_view(tiles, None, None, np.zeros(3), np.ones(3), view=v), "affine view .* Lab-family")
    win = np.zeros((2, 6), dtype=np.int32)
    _undrawn(lambda: stainlib_amd.TileView(8).apply(torch.zeros((2, 16, 16), dtype=torch.int64), win), "six-column windows .* affine view")
    _undrawn(lambda: stainlib_amd.TileView(8).apply(torch.zeros((2, 16, 16), dtype=torch.int64), torch.from_numpy(win)), "affine view")
    # what the calls that TAKE it refuse, before the device: CPU tiles come last
    _undrawn(lambda: nz.augment_batch(tiles, ab, normalize=False, view=v, windows=win[:, :5]), "windows of an affine view must hold")
    _undrawn(lambda: nz.augment_batch(tiles, ab, normalize=False, view=v, windows=win[:1]), "affine view")
    big = win.copy()
    big[1, 2:] = (Q, Q + 1, 0, 0)
    _undrawn(lambda: nz.augment_batch(tiles, ab, normalize=False, view=v, windows=big), "tile 1 .* row sum")
    _undrawn(lambda: stainlib_amd.TensorFormat().convert(tiles, view=v, windows=big), "row sum")
    _undrawn(lambda: nz.augment_batch(tiles, ab, normalize=False, view=v, windows=win), "contiguous CUDA uint8")
    _undrawn(lambda: nz.augment_batch(tiles, ab, normalize=False, view=TileAffine((8193, 8))), "8192")
    _undrawn(lambda: v.apply(torch.zeros((2, 16, 16), dtype=torch.int64)), "windows is required")
    _undrawn(lambda: v.apply(torch.zeros((2, 16, 16), dtype=torch.int64), win), "not a CPU tensor")
    _undrawn(lambda: v.apply(torch.zeros((2, 16, 16), dtype=torch.int64), win[:, :3]), "windows of an affine view")
    _undrawn(lambda: v.apply(torch.zeros((2, 16, 16), dtype=torch.complex64), win), "not supported")
    _undrawn(lambda: v.apply(torch.zeros((2, 16, 16), dtype=torch.uint8), win, fill=300), "fill must be a number")
    _undrawn(lambda: engine.normalize_view_affine(tiles, win, 8, 0), "max_r")
    _undrawn(lambda: engine.normalize_view_affine(tiles, win, 8, Q, fill=(1, 2, 256)), "fill")
    _undrawn(lambda: engine.normalize_view_affine(tiles, win, 8, Q, M_src=np.zeros((2, 2, 3))), "M_src and maxC_src go together")
    _undrawn(lambda: engine.view_planes_affine(torch.zeros((2, 16, 16)), win, 8, 2 * Q + 1), "max_r")


def test_a_view_call_draws_after_every_check_and_hands_the_bound_on(monkeypatch):
    """the host windows' own largest row sum sizes the launch; device windows and a draw take the view's bound"""
    seen = []
    monkeypatch.setattr(engine, "normalize_view_affine", lambda *a, **k: seen.append((a, k)) or "out")
    tiles = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    v = TileAffine(8, zoom=(0.8, 1), fill=(1, 2, 3))
    win = np.array([[8 * Q, 8 * Q, Q, 0, 0, Q], [8 * Q, 8 * Q, Q // 2, -Q // 4, 0, 7]], dtype=np.int32)
    out, w2 = engine.view_pass(tiles, v, win, fmt=None, out=None, M_src=None)
    (a, k), = seen
    assert out == "out" and w2 is win and a[1] is win and a[2:] == ((8, 8), Q, (1, 2, 3)) and k == dict(fmt=None, out=None, M_src=None)
    seen.clear()
    np.random.seed(4)
    out, w3 = engine.view_pass(tiles, v, None)
    np.random.seed(4)
    assert np.array_equal(w3, v.draw(2, 16, 16)) and seen[0][0][3] == int(affine_row_sums(w3).max()) <= v.bound
    seen.clear()
    dev = torch.zeros((2, 6), dtype=torch.int32).as_subclass(type("Dev", (torch.Tensor,), {"is_cuda": True}))
    engine.view_pass(tiles, v, dev)
    assert seen[0][0][1] is dev and seen[0][0][3] == v.bound


# ---- 7. the C argument checks under AddressSanitizer -----------------------------------------------------------------------------------------
def test_c_abi_argument_checks_of_the_entry_points_under_asan():
    """`make asan-affine`: tests/abi_argcheck_affine.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of both entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if
    nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-affine", "-j8"], capture_output=True, text=True,
                       timeout=1800)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail


# ---- 8. the kernels' geometry, lane by lane, under the host sanitizers -----------------------------------------------------------------------
def _host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_geometry_tiles_the_output_keeps_every_tap_in_its_block_and_follows_the_definition(tmp_path):
    """tests/view_affine_geometry.cpp, a stand-alone program: view_affine_geometry.hpp alone, for every lane of every workgroup."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "view_affine_geometry")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", os.path.join(HERE, "view_affine_geometry.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"^\d+ cases, \d+ output elements checked, 0 failures$", r.stdout, flags=re.M)
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr


def test_the_numpy_definition_and_the_header_agree_on_the_patch_edge():
    """b = min(64, 1 + 62 Q // max(R, 1)): 63 at the identity, 44 at 45 degrees, 32 at the limit (the header's affine_patch_edge, restated)"""
    edge = lambda r: min(64, 1 + 62 * Q // max(r, 1))
    assert edge(Q) == 63 and edge(int(np.rint(Q * np.sqrt(2)))) == 44 and edge(2 * Q) == 32 and edge(0) == 64 and edge(1) == 64
    src = open(os.path.join(REPO, "stainlib_amd", "csrc", "view_affine_geometry.hpp")).read()
    assert "(62 * kAffineQ) / geom_max(r, 1)" in src and "q >= 63 ? 64 : 1 + q" in src

"""Hue / saturation / brightness augmentation on the host side (stainlib_amd/augmentation/hsb.py, sl_hsb_augment, sl_normalize_hsb_view,
hsb= on the batch methods): the integer definition against goldens written by the real scikit-image, its identity, the augmenter's draws
and errors, every refusal before any draw, the header / binding / library agreement and the two stand-alone C / C++ programs -- no GPU
needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine
from stainlib_amd.augmentation import hsb as H
from stainlib_amd.utils.excepts import InvalidRangeError
from tests.gpu_util import BAD_SHAPES, BAD_STATS, ROUTES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
Q = H.Q
BADARG = -1
RGB, OUT, D6, D2, AB, WIN, CD = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x300400
N, HH, WW, OH, OW = 4, 64, 48, 40, 32


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def test_the_definition_is_within_one_of_scikit_image_on_every_byte():
    """tests/golden/hsb_skimage_*.npz (tests/golden/make_golden_hsb.py under the real scikit-image 0.18.3: rgb2hsv, the shifts in binary64,
    hsv2rgb, floor(255 x + 1/2)): hsb_reference is within 1 on EVERY byte, and at most 1e-2 of the bytes differ at all (a cap; the
    definition showed at most 6.1e-3 on these files)."""
    files = sorted(glob.glob(os.path.join(HERE, "golden", "hsb_skimage_*.npz")))
    assert len(files) >= 2
    for path in files:
        z = np.load(path)
        assert str(z["skimage_version"]) == "0.18.3" and z["sigmas"].shape == (5, 3)
        assert z["tile"].shape == (128, 128, 3) and z["colours"].shape == (64, 64, 3)
        for key in ("tile", "colours"):
            for i, sig in enumerate(z["sigmas"]):
                got = H.hsb_reference(z[key], H.hsb_codes(sig))
                d = np.abs(got.astype(np.int16) - z[key + "_out"][i].astype(np.int16))
                share = float((d != 0).mean())
                print(f"{os.path.basename(path)} {key} sigmas {np.round(sig, 4)}: max |delta| {d.max()}, share of bytes that differ {share:.2e}")
                assert d.max() <= 1
                assert share <= 1e-2


def _edge_colours():
    """greys, black, white, the primaries and secondaries, M = 1, and the six channel-tie classes (r = g > b, r = g < b, ...)"""
    c = [(v, v, v) for v in (0, 1, 2, 127, 128, 254, 255)]
    c += [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)]
    for hi, lo in ((200, 50), (50, 200), (1, 0), (255, 254)):
        c += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi)]
    return np.array(c, dtype=np.uint8)


def test_zero_codes_are_the_identity():
    g = np.arange(0, 256, 3, dtype=np.uint8)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for colours in (cube, _edge_colours()):
        assert np.array_equal(H.hsb_reference(colours, np.zeros(3, dtype=np.int32)), colours)
        assert np.array_equal(H.hsb_reference(colours[None], np.zeros((1, 3), dtype=np.int32))[0], colours)


def test_codes_and_their_reduction():
    assert H.hsb_codes([[0.0, 0.0, 0.0]]).tolist() == [[0, 0, 0]] and H.hsb_codes([[0, 0, 0]]).dtype == np.int32
    assert H.hsb_codes([[1.0, 1.0, -1.0]]).tolist() == [[0, Q, -Q]]              # a whole turn is none
    assert H.hsb_codes([[-0.25, 0.5, -0.5]]).tolist() == [[4 * Q + Q // 2, Q // 2, -Q // 2]]
    assert H.hsb_codes([[1.0 - 1e-9, 0, 0]]).tolist() == [[0, 0, 0]]            # rounds up to 6 Q, which is 0
    assert H.hsb_codes([[7.5, 0.1, 0.0]])[0, 0] == 3 * Q
    for bad in ([[0, 1.5, 0]], [[0, 0, -1.01]], [[np.nan, 0, 0]], [[0, np.inf, 0]]):
        with pytest.raises(ValueError):
            H.hsb_codes(bad)
    with pytest.raises(ValueError, match="an \\(N, 3\\) array"):
        H.hsb_codes(np.zeros((2, 4)))
    wild = np.array([[-1, 40000, -40000], [6 * Q, Q + 1, -Q - 1], [-6 * Q - 5, 2 ** 31 - 1, -2 ** 31]], dtype=np.int32)
    assert H.reduce_codes(wild).tolist() == [[6 * Q - 1, Q, -Q], [0, Q, -Q], [6 * Q - 5, Q, -Q]]
    px = _edge_colours()
    assert np.array_equal(H.hsb_reference(px, wild[0]), H.hsb_reference(px, [6 * Q - 1, Q, -Q]))
    # the real-number reading on a plain case: a third of a turn takes red to green; ds = -1 greys; dv = -1 blackens
    assert H.hsb_reference(np.array([[255, 0, 0]], np.uint8), [2 * Q, 0, 0]).tolist() == [[0, 255, 0]]
    assert H.hsb_reference(np.array([[200, 100, 50]], np.uint8), [0, -Q, 0]).tolist() == [[200, 200, 200]]
    assert H.hsb_reference(np.array([[200, 100, 50]], np.uint8), [0, 0, -Q]).tolist() == [[0, 0, 0]]


# ---- the augmenter ------------------------------------------------------------------------------------------------------------------------
def test_the_augmenter_draws_hue_then_saturation_then_brightness():
    aug = stainlib_amd.HsbColorAugmenter((-0.3, 0.2), (-0.5, 0.5), (0.1, 0.4))
    assert aug.keyword == "hsb_color" and aug._sigmas == [-0.3, -0.5, 0.1]          # the lower bounds until randomize()
    assert aug.shapes({"a": 1}) == {"a": 1}
    np.random.seed(9)
    aug.randomize()
    np.random.seed(9)
    want = [np.random.uniform(-0.3, 0.2), np.random.uniform(-0.5, 0.5), np.random.uniform(0.1, 0.4)]
    assert aug._sigmas == want
    # a None range draws nothing and gives 0
    light = stainlib_amd.HsbLightColorAugmenter()
    assert light._sigma_ranges == [(-0.1, 0.1), (-0.1, 0.1), None] and light._sigmas == [-0.1, -0.1, 0.0]
    strong = stainlib_amd.HsbStrongColorAugmenter()
    assert strong._sigma_ranges == [(-1, 1), (-1, 1), None] and strong._sigmas == [-1.0, -1.0, 0.0]
    np.random.seed(4)
    s = light.randomize_batch(3)
    after = np.random.uniform()
    np.random.seed(4)
    want = np.array([[np.random.uniform(-0.1, 0.1), np.random.uniform(-0.1, 0.1), 0.0] for _ in range(3)])
    assert s.shape == (3, 3) and s.dtype == np.float64 and np.array_equal(s, want) and np.random.uniform() == after
    none = stainlib_amd.HsbColorAugmenter(None, None, None)
    np.random.seed(4)
    assert not none.randomize_batch(2).any()
    none.randomize()
    a = np.random.uniform()
    np.random.seed(4)
    assert np.random.uniform() == a


@pytest.mark.parametrize("ranges", [((-1.1, 0), None, None), (None, (0.2, 0.1), None), (None, None, (0, 1.5)), ((0, 0.1, 0.2), None, None)])
def test_ranges_outside_minus_one_to_one_raise_invalid_range_error(ranges):
    with pytest.raises(InvalidRangeError):
        stainlib_amd.HsbColorAugmenter(*ranges)


def test_transform_refuses_what_is_no_uint8_image():
    with pytest.raises(TypeError):
        stainlib_amd.HsbLightColorAugmenter().transform(np.zeros((4, 4, 3), dtype=np.float64))


# ---- refusals: a ValueError that names its cause, before any draw (CPU tiles: an accepted call stops at the tile check) -----------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
_SG = np.zeros((2, 3))
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
    aug = stainlib_amd.HsbStrongColorAugmenter()
    hed = stainlib_amd.HedLightColorAugmenter()
    view = stainlib_amd.TileView((5, 7), rot90=False)
    affine = stainlib_amd.TileAffine((5, 5))
    for name, call in _methods()[2]:
        np.random.seed(3)
        with pytest.raises(ValueError, match="hsb= and hed= do not go together"):
            call(hsb=aug, hed=hed)
        with pytest.raises(ValueError, match="hsb= and hed= do not go together"):
            call(hsb=aug, hed=hed, view=view, hsb_sigmas=_SG)
        with pytest.raises(ValueError, match="an affine view .* is not supported by the HSB stage"):
            call(hsb=aug, view=affine)
        with pytest.raises(ValueError, match="hsb must be a stainlib_amd HsbColorAugmenter"):
            call(hsb="strong")
        with pytest.raises(ValueError, match="hsb must be a stainlib_amd HsbColorAugmenter"):
            call(hsb=hed, view=view)
        with pytest.raises(ValueError, match="hsb_sigmas= goes with hsb="):
            call(hsb_sigmas=_SG)
        with pytest.raises(ValueError, match="an \\(N, 3\\) array"):
            call(hsb=aug, hsb_sigmas=np.zeros((2, 4)))
        with pytest.raises(ValueError, match="one .* row per tile"):
            call(hsb=aug, hsb_sigmas=np.zeros((3, 3)))
        with pytest.raises(ValueError, match="must lie in \\[-1, 1\\]"):
            call(hsb=aug, hsb_sigmas=np.array([[0, 2.0, 0], [0, 0, 0]]))
        with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
            call(hsb=aug, view=(5, 7))
        with pytest.raises(ValueError, match="windows= goes with view="):
            call(hsb=aug, windows=_WIN)
        with pytest.raises(ValueError, match="does not fit"):
            call(hsb=aug, view=stainlib_amd.TileView(10))
        # accepted arguments: the call stops at the tile check (CPU tiles) -- AFTER the argument checks, BEFORE any draw
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(hsb=aug)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(hsb=aug, view=view)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, name                    # nothing was consumed by a refused call
    np.random.seed(3)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        aug.transform_batch(_TILES, view=view)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        aug.transform_batch(_TILES)
    with pytest.raises(ValueError, match="an affine view .* is not supported by the HSB stage"):
        aug.transform_batch(_TILES, view=affine)
    with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
        aug.transform_batch(_TILES, view=(5, 7))
    with pytest.raises(ValueError, match="one .* row per tile"):
        aug.transform_batch(_TILES, np.zeros((3, 3)), view=view)
    with pytest.raises(ValueError, match="codes must hold"):
        engine.hsb_augment(_TILES, np.zeros((2, 3)))                  # floats are no codes
    with pytest.raises(ValueError, match="codes must have one row per tile"):
        engine.normalize_hsb_view(_TILES, _WIN, (5, 7), 6, np.zeros((3, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        engine.hsb_augment(_TILES, np.zeros((2, 3), dtype=np.int32), fmt="float16")
    with pytest.raises(ValueError, match=_TILE_CHECK):
        engine.normalize_hsb_view(_TILES, _WIN, (5, 7), 6, np.zeros((2, 3), dtype=np.int32))
    after = np.random.uniform()
    np.random.seed(3)
    assert np.random.uniform() == after


def test_the_draw_order_is_alpha_beta_then_hsb_then_windows(monkeypatch):
    """the engine calls replaced by stand-ins that record what they are handed: the global numpy stream gives alpha_beta (where the method
    draws one), then the augmenter's draws per tile (hue, saturation; the Strong preset has no brightness range), then the windows"""
    n, h, w = 2, 9, 11
    seen = {}
    fit = (torch.zeros((n, 2, 3), dtype=torch.float64), torch.ones((n, 2), dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "macenko_fit", lambda t, *a, **k: fit)
    monkeypatch.setattr(engine, "vahadane_fit", lambda t, *a, **k: fit + (None,))
    for cls in (stainlib_amd.MacenkoNormalizer, stainlib_amd.VahadaneNormalizer):
        monkeypatch.setattr(cls, "_target_on", lambda self, dev: (None, None))

    def hsb_view(tiles, win, size, d_mask, codes, **kw):
        seen.update(win=win, size=size, d_mask=d_mask, codes=codes, kw=kw)
        return "out"
    monkeypatch.setattr(engine, "normalize_hsb_view", hsb_view)
    aug = stainlib_amd.HsbStrongColorAugmenter()
    view = stainlib_amd.TileView((5, 5))
    nz, sa, methods = _methods()
    for name, call in methods:
        for with_view in (True, False):
            np.random.seed(77)
            res = call(hsb=aug, **(dict(view=view) if with_view else {}))
            after = np.random.uniform()
            np.random.seed(77)
            ab = stainlib_amd.StainJitter().draw(n) if name == "StainAugmentor" else _AB
            sig = np.array([[np.random.uniform(-1, 1), np.random.uniform(-1, 1), 0.0] for _ in range(n)])
            win = view.draw(n, h, w) if with_view else None
            assert np.random.uniform() == after, name                # and nothing else was consumed
            draw = res[-1]
            assert isinstance(draw, engine.HsbDraw) and np.array_equal(draw.sigmas, sig) and res[0] == "out", name
            assert np.array_equal(draw.codes, H.hsb_codes(sig)) and np.array_equal(seen["codes"], draw.codes)
            if "augment" in name or name == "StainAugmentor":
                assert np.array_equal(np.asarray(seen["kw"]["alpha_beta"]), ab)
            else:
                assert "alpha_beta" not in seen["kw"]
            if with_view:
                assert len(res) == 6 and np.array_equal(res[4], win) and np.array_equal(seen["win"], win)
                assert (seen["size"], seen["d_mask"]) == ((5, 5), 7)
            else:                                                    # the full tile, code 0
                assert len(res) == 5 and (seen["size"], seen["d_mask"]) == (None, 0) and not np.asarray(seen["win"]).any()
    # given sigmas: nothing but the windows is consumed
    np.random.seed(5)
    res = nz.transform_batch(_TILES, hsb=aug, hsb_sigmas=_SG, view=view)
    after = np.random.uniform()
    np.random.seed(5)
    assert np.array_equal(res[4], view.draw(n, h, w)) and np.random.uniform() == after and np.array_equal(res[5].sigmas, _SG)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------
def _a(rgb=RGB, out=OUT, n=N, h=HH, w=WW, cd=CD, fmt=None):
    return _ffi.lib().sl_hsb_augment(rgb, out, n, h, w, cd, C.byref(fmt) if fmt is not None else None, None)


def _v(rgb=RGB, out=OUT, n=N, h=HH, w=WW, oh=OH, ow=OW, win=WIN, d_mask=7, shrink=1, mh=0, mw=0, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0,
       params=None, fmt=None, cd=CD):
    return _ffi.lib().sl_normalize_hsb_view(rgb, out, n, h, w, oh, ow, win, d_mask, shrink, mh, mw, ms, cs, mt, ct, ab, bg,
                                            C.byref(params) if params is not None else None, C.byref(fmt) if fmt is not None else None,
                                            cd, None)


def test_version_header_binding_and_library_agree():
    assert _ffi.lib().sl_version() == 600 and _ffi.EXPECTED_VERSION == 600        # an extension of ABI 600
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for name, count in (("sl_hsb_augment", 8), ("sl_normalize_hsb_view", 22)):
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


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(cd=None), dict(cd=CD + 2), dict(n=2 ** 31 - 1, h=32768, w=32768)], ids=str)
def test_hsb_augment_bad_pointers_and_shapes_are_refused(kw):
    assert _a(**kw) == BADARG and _a(**kw, fmt=_ffi.default_tensor_format()) == BADARG


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(win=None), dict(oh=0), dict(ow=0), dict(oh=-1), dict(d_mask=-1),
                                             dict(d_mask=8), dict(cd=None), dict(cd=CD + 1)], ids=str)
def test_hsb_view_bad_pointers_shapes_and_masks_are_refused_fixed_and_resizing(kw):
    for route in ROUTES:
        args = {**route, **kw}
        assert _v(**args) == BADARG, args
        assert _v(**args, mh=HH, mw=WW) == BADARG, args
        assert _v(**args, bg=1, params=_ffi.default_params(), fmt=_ffi.default_tensor_format()) == BADARG, args


@pytest.mark.parametrize("kw", [dict(oh=HH + 1), dict(ow=WW + 1), dict(oh=HH, ow=WW, d_mask=7), dict(shrink=0), dict(shrink=3), dict(shrink=2),
                                dict(oh=16, ow=16, d_mask=6, shrink=4), dict(n=1 << 22, h=32768, w=32768, oh=32768, ow=32768),
                                dict(mw=WW), dict(mh=HH), dict(mh=-1, mw=WW), dict(mh=HH + 1, mw=WW), dict(mh=HH, mw=WW + 1),
                                dict(oh=16, ow=12, shrink=2, mh=HH, mw=WW), dict(h=4096, w=4096, mh=2049, mw=2048)], ids=str)
def test_hsb_view_bad_geometry_is_refused(kw):
    for route in ROUTES:
        assert _v(**{**route, **kw}) == BADARG, kw


@pytest.mark.parametrize("kw", BAD_STATS, ids=str)
def test_hsb_view_bad_statistics_are_refused(kw):
    assert _v(**kw) == BADARG and _v(**kw, mh=HH, mw=WW, fmt=_ffi.default_tensor_format()) == BADARG


def test_bad_params_and_format_structs_are_refused():
    for size in (0, 16, C.sizeof(_ffi.SlParams) - 8, C.sizeof(_ffi.SlParams) + 8):
        p = _ffi.default_params()
        p.struct_size = size
        for route in ROUTES:
            assert _v(**route, params=p) == BADARG
    for field, value in (("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3), ("layout", -1),
                         ("layout", 2), ("std", 0.0), ("std", float("nan")), ("mean", float("inf"))):
        f = _ffi.default_tensor_format()
        if field in ("std", "mean"):
            getattr(f, field)[1] = value
        else:
            setattr(f, field, value)
        assert _a(fmt=f) == BADARG, (field, value)
        for route in ROUTES:
            assert _v(**route, fmt=f) == BADARG, (field, value)


# ---- the stand-alone programs -----------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_the_per_pixel_function_equals_its_64_bit_restatement_under_the_host_sanitizers(tmp_path):
    """tests/hsb_math_check.cpp, a stand-alone program: csrc/hsb_math.hpp alone -- every division the map can see, the scale over [0, Q],
    a strided colour cube at a dozen code triples -- built with the address and undefined-behaviour sanitizers."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "hsb_math_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", os.path.join(HERE, "hsb_math_check.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"^\d+ checks, 0 failures$", r.stdout, flags=re.M)
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr


def test_c_abi_argument_checks_of_the_hsb_entry_points_under_asan():
    """`make asan-hsb`: tests/abi_argcheck_hsb.c -- a stand-alone program -- against the library's HOST side built with AddressSanitizer:
    every refused call of the two entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if nothing has yet: a
    few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-hsb", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

"""The stain-jitter entry point (sl_normalize_jitter), engine.normalize_jitter, the augment_batch methods and StainJitter on the host
side: the draws follow StainAugmentor.pop's order, and every bad argument is refused before anything is launched -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import _ffi, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
BADARG = -1
# device pointers: never read by the host side
RGB, OUT, D6, D2, AB = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200
N, H, W = 4, 64, 48


def _jit(rgb=RGB, out=OUT, n=N, h=H, w=W, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0, params=None, fmt=None):
    return _ffi.lib().sl_normalize_jitter(rgb, out, n, h, w, ms, cs, mt, ct, ab, bg, C.byref(params) if params is not None else None,
                                          C.byref(fmt) if fmt is not None else None, None)


# ---- StainJitter ------------------------------------------------------------------------------------------------------------------------
def test_stain_jitter_draws_in_the_order_of_successive_pops():
    assert stainlib_amd.StainJitter is stainlib_amd.augmentation.augmenter.StainJitter
    g = np.load(os.path.join(GOLDEN, "stainaug_128_s2_np7.npz"))
    j = stainlib_amd.StainJitter()
    assert (j.sigma1, j.sigma2, j.augment_background) == (0.2, 0.2, False)
    np.random.seed(int(g["npseed"]))
    ab = j.draw(2)
    after = np.random.uniform()
    assert ab.shape == (2, 4) and ab.dtype == np.float64
    np.testing.assert_array_equal(ab[0], g["draws0"])                       # the reference's own first pop: alpha0, beta0, alpha1, beta1
    # only the first pop is recorded there: both rows against two successive pops of the oracle's StainAugmentor
    a = so.StainAugmentor("macenko")
    seen = []
    a.pop_with = lambda al, be: seen.append([al[0], be[0], al[1], be[1]])
    np.random.seed(int(g["npseed"]))
    a.pop()
    a.pop()
    np.testing.assert_array_equal(ab, np.array(seen))
    assert np.random.uniform() == after                                     # and nothing else was consumed
    # and of the package's own class, other sigmas
    s = stainlib_amd.StainAugmentor("macenko", sigma1=0.1, sigma2=0.3)
    s.n_stains = 2
    seen = []
    s.pop_with = lambda row: seen.append(list(row))
    np.random.seed(5)
    for _ in range(3):
        s.pop()
    np.random.seed(5)
    np.testing.assert_array_equal(stainlib_amd.StainJitter(0.1, 0.3).draw(3), np.array(seen))
    assert stainlib_amd.StainJitter().draw(0).shape == (0, 4)
    with pytest.raises(ValueError):
        stainlib_amd.StainJitter().draw(-1)


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert "sl_normalize_jitter" in declared and "sl_normalize_jitter" in _ffi.EXPORTS
    assert declared == set(_ffi.EXPORTS)
    proto = re.search(r"^SL_API int sl_normalize_jitter\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(proto.split(",")) == len(_ffi._SIGNATURES["sl_normalize_jitter"][1]) == 14
    assert _ffi.lib().sl_version() == 600                    # an extension of ABI 600: no existing struct changes


@pytest.mark.parametrize("kw", [dict(rgb=None), dict(out=None), dict(ms=None), dict(cs=None), dict(ab=None), dict(mt=None), dict(ct=None),
                                dict(ab=None, mt=None, ct=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=-5), dict(h=65536, w=65536),
                                dict(h=32768, w=32769), dict(h=32768, w=32769, mt=None, ct=None)], ids=str)
def test_bad_pointers_targets_and_shapes_are_refused(kw):
    assert _jit(**kw) == BADARG
    assert _jit(**kw, bg=1, params=_ffi.default_params(), fmt=_ffi.default_tensor_format()) == BADARG


@pytest.mark.parametrize("size", [0, 16, -8, 8])
def test_params_struct_size_mismatch_is_refused(size):
    p = _ffi.default_params()
    p.struct_size = size if size in (0, 16) else C.sizeof(_ffi.SlParams) + size
    assert _jit(params=p) == BADARG and _jit(params=p, mt=None, ct=None, fmt=_ffi.default_tensor_format()) == BADARG


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3),
                                         ("dtype", 2 ** 31 - 1), ("layout", -1), ("layout", 2), ("layout", 99)])
def test_bad_format_header_is_refused(field, value):
    f = _ffi.default_tensor_format()
    assert C.sizeof(_ffi.SlTensorFormat) == 64
    setattr(f, field, value)
    assert _jit(fmt=f) == BADARG and _jit(fmt=f, mt=None, ct=None, bg=1) == BADARG


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("field,value", [("std", 0.0), ("std", -1.0), ("std", float("nan")), ("std", float("inf")),
                                         ("mean", float("nan")), ("mean", float("-inf"))])
def test_bad_format_values_are_refused(field, value, c):
    f = _ffi.default_tensor_format()
    getattr(f, field)[c] = value
    assert _jit(fmt=f) == BADARG


# ---- the Python surface: refused with ValueError before the device is touched (the tiles are CPU tensors: reaching the tile check
# would raise ValueError too, so every case matches on its own message) ---------------------------------------------------------------
_TILES = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
_M, _MC = torch.zeros((2, 2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.float64)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))


def _surfaces(alpha_beta=_AB, **kw):
    """the ways into the pass that take these arguments (engine keywords; the normalizers call fmt tensor_format and take no params)"""
    calls = [lambda: engine.normalize_jitter(_TILES, _M, _MC, None, None, alpha_beta, **kw)]
    if "params" not in kw:
        kw2 = {("tensor_format" if k == "fmt" else k): v for k, v in kw.items()}
        calls.append(lambda: stainlib_amd.MacenkoNormalizer().augment_batch(_TILES, alpha_beta, normalize=False, **kw2))
    return calls


@pytest.mark.parametrize("ab", [None, [1.0, 0.0, 1.0, 0.0], np.zeros((2, 3)), np.zeros((2, 4, 1)), torch.zeros((2, 2)), "draws", [[1, 0, 1, "x"]]],
                         ids=lambda a: type(a).__name__ + str(getattr(a, "shape", "")))
def test_bad_alpha_beta_is_a_value_error(ab):
    for call in _surfaces(alpha_beta=ab):
        with pytest.raises(ValueError, match="alpha_beta must"):
            call()
    if ab is not None:                                        # (None: StainAugmentor.augment_batch draws)
        with pytest.raises(ValueError, match="alpha_beta must"):
            stainlib_amd.StainAugmentor("macenko").augment_batch(_TILES, ab)


@pytest.mark.parametrize("fmt", ["float16", torch.float16, 3, (0.5, 0.5, 0.5)], ids=str)
def test_bad_format_is_a_value_error(fmt):
    for call in _surfaces(fmt=fmt):
        with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
            call()
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        stainlib_amd.StainAugmentor("vahadane").augment_batch(_TILES, _AB, tensor_format=fmt)


def test_bad_out_params_and_target_are_value_errors():
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16)
    for out, fmt in ((torch.zeros((2, 3, 8, 8)), None), ("x", None), (torch.zeros((2, 8, 8, 3), dtype=torch.uint8), f16),
                     (torch.zeros((2, 3, 8, 8)), f16)):
        for call in _surfaces(out=out, fmt=fmt):
            with pytest.raises(ValueError, match="out must be a torch"):
                call()
    for params in (dict(lasso_lambda=0.01), 0.01, _ffi.default_tensor_format()):
        with pytest.raises(ValueError, match="params must be"):
            engine.normalize_jitter(_TILES, _M, _MC, None, None, _AB, params=params)
    with pytest.raises(ValueError, match="go together"):
        engine.normalize_jitter(_TILES, _M, _MC, _M[0], None, _AB)
    with pytest.raises(ValueError, match="go together"):
        engine.normalize_jitter(_TILES, _M, _MC, None, _MC[0], _AB)
    for nz in (stainlib_amd.MacenkoNormalizer(), stainlib_amd.VahadaneNormalizer()):
        with pytest.raises(ValueError, match="needs a fitted target"):
            nz.augment_batch(_TILES, _AB)
        with pytest.raises(ValueError, match="needs a fitted target"):
            nz.augment_batch(_TILES, _AB, augment_background=True, tensor_format=f16)


def test_c_abi_argument_checks_of_the_jitter_entry_point_under_asan():
    """`make asan-jitter`: tests/abi_argcheck_jitter.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the entry point, among them a caller's SlParams and SlTensorFormat smaller than this
    header's at the end of their heap blocks.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if nothing has yet:
    about two minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-jitter", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

"""The tensor-output entry points (sl_default_tensor_format, sl_to_tensor, sl_normalize_apply_tensor) and
stainlib_amd.TensorFormat on the host side: every bad argument is refused before anything is launched -- no GPU needed."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
RGB, OUT, D6, D2 = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x300100))   # device pointers: never read by the host side
N, H, W = 4, 64, 48


def _both(rgb=RGB, out=OUT, n=N, h=H, w=W, fmt=None):
    """return codes of the two launching entry points for one set of arguments"""
    lib = _ffi.lib()
    f = C.byref(fmt) if fmt is not None else None
    return (lib.sl_to_tensor(rgb, out, n, h, w, f, None),
            lib.sl_normalize_apply_tensor(rgb, out, n, h, w, D6, D2, D6, D2, 0.01, f, None))


def test_default_tensor_format_and_version():
    f = _ffi.SlTensorFormat()
    _ffi.lib().sl_default_tensor_format(C.byref(f))
    assert f.struct_size == C.sizeof(_ffi.SlTensorFormat) == 64
    assert (f.dtype, f.layout, f.reserved) == (_ffi.DTYPE_F32, _ffi.LAYOUT_NCHW, 0)
    assert list(f.mean) == [0.0] * 3 and list(f.std) == [1.0] * 3
    _ffi.lib().sl_default_tensor_format(None)            # must not crash
    assert _ffi.lib().sl_version() == 600                  # an extension of ABI 600: SlParams and the version are untouched
    assert C.sizeof(_ffi.SlParams) == _ffi.default_params().struct_size


def test_header_constants_match_the_binding():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    for name, want in (("SL_DTYPE_F32", _ffi.DTYPE_F32), ("SL_DTYPE_F16", _ffi.DTYPE_F16), ("SL_DTYPE_BF16", _ffi.DTYPE_BF16),
                       ("SL_LAYOUT_NCHW", _ffi.LAYOUT_NCHW), ("SL_LAYOUT_NHWC", _ffi.LAYOUT_NHWC)):
        assert int(re.search(rf"^#define {name} (\d+)$", hdr, flags=re.M).group(1)) == want
    for name in ("sl_default_tensor_format", "sl_to_tensor", "sl_normalize_apply_tensor"):
        assert name in _ffi.EXPORTS


@pytest.mark.parametrize("kw", [dict(rgb=None), dict(out=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=-5), dict(h=65536, w=65536),
                                dict(h=32768, w=32769)], ids=str)
def test_bad_pointers_and_shapes_are_refused(kw):
    assert _both(fmt=_ffi.default_tensor_format(), **kw) == (BADARG, BADARG)


def test_missing_format_and_statistics_are_refused():
    assert _both(fmt=None) == (BADARG, BADARG)
    lib, f = _ffi.lib(), _ffi.default_tensor_format()
    for hole in range(4):
        stats = [D6, D2, D6, D2]
        stats[hole] = None
        assert lib.sl_normalize_apply_tensor(RGB, OUT, N, H, W, *stats, 0.01, C.byref(f), None) == BADARG


@pytest.mark.parametrize("size", [0, 16, 56, 72])
def test_struct_size_mismatch_is_refused(size):
    f = _ffi.default_tensor_format()
    f.struct_size = size
    assert _both(fmt=f) == (BADARG, BADARG)


@pytest.mark.parametrize("field", ["dtype", "layout"])
@pytest.mark.parametrize("value", [-1, 3, 99, -2 ** 31, 2 ** 31 - 1])
def test_unknown_dtype_or_layout_is_refused(field, value):
    f = _ffi.default_tensor_format()
    setattr(f, field, value)
    assert _both(fmt=f) == (BADARG, BADARG)


@pytest.mark.parametrize("c", range(3))
def test_non_finite_mean_and_bad_std_are_refused(c):
    for bad in (math.nan, math.inf, -math.inf):
        f = _ffi.default_tensor_format()
        f.mean[c] = bad
        assert _both(fmt=f) == (BADARG, BADARG), bad
    for bad in (0.0, -0.0, -1.0, math.nan, math.inf, -math.inf):
        f = _ffi.default_tensor_format()
        f.std[c] = bad
        assert _both(fmt=f) == (BADARG, BADARG), bad


def test_tensor_format_validation():
    TF = stainlib_amd.TensorFormat
    f = TF()
    assert f.dtype is torch.float32 and f.channels_last is False and f.mean == (0.0, 0.0, 0.0) and f.std == (1.0, 1.0, 1.0)
    g = TF(torch.bfloat16, True, mean=[0.485, 0.456, 0.406], std=torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64))
    assert g.dtype is torch.bfloat16 and g.channels_last is True and g.mean == (0.485, 0.456, 0.406) and g.std == (0.229, 0.224, 0.225)
    assert TF("float16").dtype is torch.float16
    for dtype in (torch.float64, torch.uint8, torch.int32, "float64", "half", 1, float):
        with pytest.raises(ValueError):
            TF(dtype)
    for mean in ((0, 0), (0, 0, 0, 0), (0, math.nan, 0), (math.inf, 0, 0), 0.5, "abc", (None, 0, 0)):
        with pytest.raises(ValueError):
            TF(mean=mean)
    for std in ((1, 1), (1, 1, 1, 1), (1, 0, 1), (1, 1, -0.5), (1, math.nan, 1), (math.inf, 1, 1), 1.0, (1, "x", 1)):
        with pytest.raises(ValueError):
            TF(std=std)


def test_engine_fills_the_struct_from_a_tensor_format():
    from stainlib_amd import engine
    s, dtype, cl = engine._tensor_format(stainlib_amd.TensorFormat(torch.float16, True, (0.5, 0.25, 0.125), (0.5, 2, 4)))
    assert (s.struct_size, s.dtype, s.layout) == (64, _ffi.DTYPE_F16, _ffi.LAYOUT_NHWC) and dtype is torch.float16 and cl is True
    assert list(s.mean) == [0.5, 0.25, 0.125] and list(s.std) == [0.5, 2.0, 4.0]


def test_graph_with_tensor_format_is_refused_before_any_work():
    """SlideNormalizer(graph=True).transform_shard(tensor_format=...) raises ValueError (capturing it is out of scope): checked before
    the tiles are looked at, so this needs no device."""
    from stainlib_amd.distributed import SlideNormalizer
    sn = SlideNormalizer(stainlib_amd.MacenkoNormalizer(), group=False, mode="pooled", graph=True)
    with pytest.raises(ValueError, match="tensor_format"):
        sn.transform_shard(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), tensor_format=stainlib_amd.TensorFormat())


def test_c_abi_argument_checks_of_the_tensor_entry_points_under_asan():
    """`make asan-tensor`: tests/abi_argcheck_tensor.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the three entry points, among them a caller's struct smaller than this header's at the
    end of its heap block.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if nothing has yet: about two minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-tensor", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

"""CPU-only: the surface of the pooled slide-level Reinhard / luminosity chain (sl_slab_*, csrc/slide_lab.hip) -- the names in the
header, the binding and the library, the argument checks of every entry point (each returns before anything is launched: no GPU
here), and the constructor / transform_shard refusals of SlideNormalizer."""
import ctypes as C
import os
import re

import pytest

import stainlib_amd
from stainlib_amd import _ffi
from stainlib_amd import distributed as sd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sl_slab_workspace_bytes", "sl_slab_bytes", "sl_slab_begin", "sl_slab_lab", "sl_slab_finish", "sl_slab_map")
BADARG, WORKSPACE = -1, -2


def test_the_new_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    lib = C.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _ffi.EXPORTS and hasattr(lib, name), name
    assert _ffi.lib().sl_version() == 600 and _ffi.EXPECTED_VERSION == 600
    # the state offsets of the binding are the header's
    for py, c in (("SLAB_STATE_DOUBLES", "SL_SLAB_STATE_DOUBLES"), ("SLAB_SUMS_A", "SL_SLAB_SUMS_A"), ("SLAB_SUMS_B", "SL_SLAB_SUMS_B"),
                  ("SLAB_P90", "SL_SLAB_P90"), ("SLAB_MEANS", "SL_SLAB_MEANS"), ("SLAB_STDS", "SL_SLAB_STDS"), ("SLAB_LPCT", "SL_SLAB_LPCT"),
                  ("SLAB_TISSUE", "SL_SLAB_TISSUE"), ("SLAB_NPX", "SL_SLAB_NPX"), ("SLAB_STATUS", "SL_SLAB_STATUS"),
                  ("SLAB_TABLES", "SL_SLAB_TABLES")):
        m = re.search(r"^#define %s (\d+)" % c, hdr, flags=re.M)
        assert m and int(m.group(1)) == getattr(_ffi, py), c
    # the header's comment block: what is restated, on what, and the family's caveat
    block = hdr[hdr.index("REINHARD / LUMINOSITY"):]
    assert "normalizer.py:70-94" in block and "stain_utils.py:52-67,146-194" in block and "on the concatenation" in block
    assert "not\n * pinned against a real cv2" in block or "not pinned against a real cv2" in block


def test_workspace_sizes():
    lib = _ffi.lib()
    assert lib.sl_slab_workspace_bytes(0, 64, 64) > 0                          # an empty shard is legal
    small, big = lib.sl_slab_workspace_bytes(1, 8, 8), lib.sl_slab_workspace_bytes(512, 1024, 1024)
    assert small >= 8 * _ffi.SLAB_SUMS_B and small % 256 == 0
    assert small <= big < (64 << 20)                                           # partial rows only: it does not grow with the shard
    for bad in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8), (1, 1 << 16, 1 << 15), (1 << 20, 1 << 12, 1 << 12)):
        assert lib.sl_slab_workspace_bytes(*bad) == 0, bad


def test_every_entry_point_refuses_bad_arguments_before_touching_a_device():
    lib = _ffi.lib()
    buf = (C.c_uint8 * (1 << 16))()            # host memory standing in for device pointers: the refused calls never look at it
    ws_ok = lib.sl_slab_workspace_bytes(4, 8, 8)
    # sl_slab_bytes(rgb, n, h, w, ws, ws_bytes, sums_out, stream)
    assert lib.sl_slab_bytes(None, 4, 8, 8, buf, ws_ok, buf, None) == BADARG
    assert lib.sl_slab_bytes(buf, 4, 8, 8, buf, ws_ok, None, None) == BADARG
    for n, h, w in ((-1, 8, 8), (4, 0, 8), (4, 8, 0), (4, -1, 8), (4, 8, -1)):
        assert lib.sl_slab_bytes(buf, n, h, w, buf, ws_ok, buf, None) == BADARG, (n, h, w)
    assert lib.sl_slab_bytes(buf, 4, 8, 8, None, ws_ok, buf, None) == WORKSPACE
    assert lib.sl_slab_bytes(buf, 4, 8, 8, buf, ws_ok - 1, buf, None) == WORKSPACE
    assert lib.sl_slab_bytes(buf, 4, 8, 8, C.byref(buf, 4), ws_ok, buf, None) == WORKSPACE       # misaligned
    assert lib.sl_slab_bytes(None, 0, 8, 8, None, 0, buf, None) == WORKSPACE                      # n == 0 passes the shape check, not a missing workspace
    # sl_slab_begin(state, sums_a, standardize, stream)
    assert lib.sl_slab_begin(None, buf, 1, None) == BADARG
    assert lib.sl_slab_begin(buf, None, 1, None) == BADARG
    assert lib.sl_slab_begin(None, None, 0, None) == BADARG
    # sl_slab_lab(rgb, n, h, w, state, thr, ws, ws_bytes, sums_out, stream)
    assert lib.sl_slab_lab(None, 4, 8, 8, buf, 0.8, buf, ws_ok, buf, None) == BADARG
    assert lib.sl_slab_lab(buf, 4, 8, 8, None, 0.8, buf, ws_ok, buf, None) == BADARG
    assert lib.sl_slab_lab(buf, 4, 8, 8, buf, 0.8, buf, ws_ok, None, None) == BADARG
    for n, h, w in ((-1, 8, 8), (4, 0, 8), (4, 8, 0), (4, -1, 8), (4, 8, -1)):
        assert lib.sl_slab_lab(buf, n, h, w, buf, 0.8, buf, ws_ok, buf, None) == BADARG, (n, h, w)
    assert lib.sl_slab_lab(buf, 4, 8, 8, buf, 0.8, None, ws_ok, buf, None) == WORKSPACE
    assert lib.sl_slab_lab(buf, 4, 8, 8, buf, 0.8, buf, ws_ok - 1, buf, None) == WORKSPACE
    assert lib.sl_slab_lab(None, 0, 8, 8, buf, 0.8, None, 0, buf, None) == WORKSPACE
    # sl_slab_finish(state, sums_b, mode, target_means, target_stds, percentile, mask_background, stream)
    assert lib.sl_slab_finish(None, buf, 0, buf, buf, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(buf, None, 0, buf, buf, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(buf, buf, 0, None, buf, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(buf, buf, 0, buf, None, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(buf, buf, 2, buf, buf, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(buf, buf, -1, buf, buf, 95.0, 0, None) == BADARG
    assert lib.sl_slab_finish(None, buf, 1, None, None, 95.0, 0, None) == BADARG
    # sl_slab_map(rgb, out, n, h, w, state, mode, mask_background, thr, stream): it takes no workspace (the tables live in the state)
    assert lib.sl_slab_map(None, buf, 4, 8, 8, buf, 0, 0, 0.8, None) == BADARG
    assert lib.sl_slab_map(buf, None, 4, 8, 8, buf, 0, 0, 0.8, None) == BADARG
    assert lib.sl_slab_map(buf, buf, 4, 8, 8, None, 0, 0, 0.8, None) == BADARG
    assert lib.sl_slab_map(buf, buf, 4, 8, 8, buf, 2, 0, 0.8, None) == BADARG
    for n, h, w in ((0, 8, 8), (-1, 8, 8), (4, 0, 8), (4, 8, 0), (4, -1, 8), (4, 8, -1), (1, 1 << 16, 1 << 15)):
        assert lib.sl_slab_map(buf, buf, n, h, w, buf, 0, 0, 0.8, None) == BADARG, (n, h, w)


def test_slide_normalizer_refusals_with_a_reinhard_normalizer():
    r = stainlib_amd.ReinhardStainNormalizer()
    with pytest.raises(ValueError):
        sd.SlideNormalizer(r, mode="median")
    with pytest.raises(ValueError):
        sd.SlideNormalizer(r)                                  # (the default mode is "median")
    with pytest.raises(ValueError):
        sd.SlideNormalizer(r, mode="pooled", graph=True)
    assert sd.SlideNormalizer(r, mode="pooled").mode == "pooled"
    m = sd.SlideNormalizer(stainlib_amd.ExtractiveStainNormalizer("macenko"), mode="pooled")
    with pytest.raises(ValueError):
        m.transform_shard(None, mask_background=True)          # refused before the tiles are looked at
    with pytest.raises(ValueError):
        m.transform_shard(None, luminosity_threshold=0.6)
    assert hasattr(sd, "PooledReinhardStatistics") and hasattr(sd, "slide_luminosity_standardize")

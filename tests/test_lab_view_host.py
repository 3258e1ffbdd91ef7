"""The Lab family in the one-pass loader (sl_reinhard_view, sl_luminosity_view, sl_slab_view; engine.reinhard_view / luminosity_view /
slab_view; view= on the Lab batch methods) on the host side: header and binding agree, every bad argument is refused before anything is
enqueued, a refused call draws nothing and an accepted one draws exactly TileView.draw -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine
from tests.gpu_util import BAD_SHAPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, WORKSPACE = -1, -2
INF = float("inf")
# device pointers: never read by the host side
RGB, OUT, TM, TS, ST, WIN, STATE, WS = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x400000, 0x500000
N, H, W, OH, OW = 4, 64, 48, 40, 32
WSB = 1 << 30


def _fmt(fmt):
    return C.byref(fmt) if fmt is not None else None


def _r(rgb=RGB, out=OUT, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, tm=TM, ts=TS, mask=1, thr=0.8, st=ST, ws=WS, wsb=WSB, fmt=None):
    return _ffi.lib().sl_reinhard_view(rgb, out, n, h, w, oh, ow, win, d_mask, tm, ts, mask, thr, st, ws, wsb, _fmt(fmt), None)


def _l(rgb=RGB, out=OUT, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, pct=95.0, p=ST, ws=WS, wsb=WSB, fmt=None):
    return _ffi.lib().sl_luminosity_view(rgb, out, n, h, w, oh, ow, win, d_mask, pct, p, ws, wsb, _fmt(fmt), None)


def _s(rgb=RGB, out=OUT, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, state=STATE, mode=0, mask=1, thr=0.8, fmt=None):
    return _ffi.lib().sl_slab_view(rgb, out, n, h, w, oh, ow, win, d_mask, state, mode, mask, thr, _fmt(fmt), None)


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for name, count in (("sl_reinhard_view", 18), ("sl_luminosity_view", 15), ("sl_slab_view", 15)):
        assert name in declared and name in _ffi.EXPORTS
        proto = re.search(r"^SL_API int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_ffi._SIGNATURES[name][1]) == count
    # each = (rgb, out, n, h, w, oh, ow, windows, d_mask), the existing call's arguments behind (rgb, out, n, h, w), fmt, stream
    view = _ffi._SIGNATURES["sl_normalize_view"][1]
    for new, old in (("sl_reinhard_view", "sl_reinhard_transform"), ("sl_luminosity_view", "sl_luminosity_standardize"),
                     ("sl_slab_view", "sl_slab_map")):
        a, b = _ffi._SIGNATURES[new][1], _ffi._SIGNATURES[old][1]
        assert a[:9] == view[:9] and a[9:-2] == b[5:-1] and a[-2:] == view[-2:], new
    assert _ffi.lib().sl_version() == 600                    # an extension of ABI 600: no existing struct or signature changes


GEOMETRY = [dict(out=None), dict(win=None), dict(out=RGB), dict(oh=0), dict(ow=0), dict(oh=-1), dict(oh=H + 1), dict(ow=W + 1),
            dict(d_mask=-1), dict(d_mask=8), dict(d_mask=1 << 20), dict(oh=H, ow=W, d_mask=7), dict(oh=H, ow=W, d_mask=1),
            dict(oh=W + 1, ow=W, d_mask=5)]


@pytest.mark.parametrize("kw", [k for k in BAD_SHAPES if k != dict(n=0)] + GEOMETRY, ids=str)
def test_bad_pointers_shapes_sizes_and_masks_are_refused_by_all_three(kw):
    for fmt in (None, _ffi.default_tensor_format()):
        assert _r(**kw, fmt=fmt) == BADARG and _l(**kw, fmt=fmt) == BADARG, kw
        assert _s(**kw, fmt=fmt) == BADARG and _s(**kw, mode=1, mask=0, fmt=fmt) == BADARG, kw


def test_the_calls_own_arguments_are_refused():
    assert _r(n=0) == BADARG and _l(n=0) == BADARG
    assert _r(n=1 << 22, h=32768, w=32768, oh=32768, ow=32768, d_mask=6, wsb=(1 << 64) - 1) == BADARG      # more pairs than a grid holds
    for kw in (dict(ws=None), dict(wsb=0), dict(ws=WS + 4), dict(wsb=int(_ffi.lib().sl_workspace_bytes(_ffi.OP_LAB_STATS, N, H, W)) - 1)):
        assert _r(**kw) == WORKSPACE and _l(**kw, fmt=_ffi.default_tensor_format()) == WORKSPACE, kw
    for kw in (dict(tm=None), dict(ts=None), dict(tm=None, ts=None)):
        assert _r(**kw) == BADARG and _r(**kw, mask=0, st=None, fmt=_ffi.default_tensor_format()) == BADARG, kw
    for kw in (dict(state=None), dict(mode=-1), dict(mode=2), dict(mode=1 << 30), dict(n=1 << 11, h=32768, w=32768)):
        assert _s(**kw) == BADARG and _s(**kw, fmt=_ffi.default_tensor_format()) == BADARG, kw


def test_an_empty_shard_is_ok_and_still_checked():
    assert _s(n=0) == 0 and _s(rgb=None, out=None, win=None, n=0, mode=1, fmt=_ffi.default_tensor_format()) == 0
    for kw in (dict(state=None), dict(mode=2), dict(oh=H + 1), dict(d_mask=8), dict(h=0)):
        assert _s(rgb=None, out=None, win=None, n=0, **kw) == BADARG, kw


def test_bad_format_structs_are_refused():
    for field, value in (("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3), ("layout", -1),
                         ("layout", 2), ("std", 0.0), ("std", float("nan")), ("mean", INF)):
        f = _ffi.default_tensor_format()
        if field in ("std", "mean"):
            getattr(f, field)[1] = value
        else:
            setattr(f, field, value)
        assert _r(fmt=f) == BADARG and _l(fmt=f) == BADARG and _s(fmt=f) == BADARG and _s(n=0, fmt=f) == BADARG, (field, value)


# ---- the Python surface: ValueError before the device is touched (the tiles are CPU tensors: reaching the tile check raises ValueError
# too, "expected a contiguous CUDA uint8 tensor", so every case matches on its own message) -------------------------------------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_WIN = np.array([[0, 0, 0], [4, 4, 6]], dtype=np.int32)
_T3 = [50.0, 3.0, -2.0]
_STATE = torch.zeros(_ffi.SLAB_STATE_DOUBLES, dtype=torch.float64)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def _engine_calls():
    return [("reinhard_view", lambda tiles=_TILES, win=_WIN, size=(5, 7), d_mask=6, **k: engine.reinhard_view(tiles, win, size, _T3, _T3, d_mask, **k)),
            ("luminosity_view", lambda tiles=_TILES, win=_WIN, size=(5, 7), d_mask=6, **k: engine.luminosity_view(tiles, win, size, d_mask=d_mask, **k)),
            ("slab_view", lambda tiles=_TILES, win=_WIN, size=(5, 7), d_mask=6, **k: engine.slab_view(tiles, win, size, _STATE, 0, d_mask, **k))]


def test_engine_calls_carry_normalize_views_checks_in_its_order():
    for name, call in _engine_calls():
        with pytest.raises(ValueError, match="does not fit"):
            call(size=(10, 5), win=None, fmt="float16")              # the size first
        with pytest.raises(ValueError, match="d_mask must be"):
            call(d_mask=8)
        with pytest.raises(ValueError, match="windows must hold"):
            call(win=None, fmt="float16")                            # then the windows
        with pytest.raises(ValueError, match="outside the 9 x 11 tile"):
            call(win=[[0, 0, 0], [5, 4, 6]])
        with pytest.raises(ValueError, match="outside d_mask"):
            call(win=[[0, 0, 1], [0, 0, 0]])
        with pytest.raises(ValueError, match=r"an \(2, 3\) array"):
            call(win=np.zeros((3, 3), dtype=np.int32))
        with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
            call(fmt="float16")                                      # then the format
        with pytest.raises(ValueError, match=_TILE_CHECK):           # accepted: the call goes on to the tiles themselves
            call()
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(tiles=torch.zeros((2, 9, 11), dtype=torch.uint8))
    with pytest.raises(ValueError, match="target_means must hold 3 values"):
        engine.reinhard_view(_TILES, _WIN, (5, 7), [1.0, 2.0], _T3, 6)
    with pytest.raises(ValueError, match="target_stds must hold 3 values"):
        engine.reinhard_view(_TILES, _WIN, (5, 7), _T3, "abc", 6)
    with pytest.raises(ValueError, match="percentile must be a number"):
        engine.luminosity_view(_TILES, _WIN, (5, 7), percentile=None, d_mask=6)
    with pytest.raises(ValueError, match="mode must be"):
        engine.slab_view(_TILES, _WIN, (5, 7), _STATE, 2, 6)
    with pytest.raises(ValueError, match="state must be"):
        engine.slab_view(_TILES, _WIN, (5, 7), _STATE[:8], 0, 6)


def _methods():
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    nz = stainlib_amd.ReinhardStainNormalizer([[50.0]], [[10.0]])
    nz.target_means, nz.target_stds = tuple(np.array([[v]]) for v in _T3), tuple(np.array([[v]]) for v in (10.0, 4.0, 5.0))
    sn = SlideNormalizer(nz, group=False, mode="pooled")
    return [("transform_batch", lambda **k: nz.transform_batch(_TILES, **k)),
            ("transform_batch masked", lambda **k: nz.transform_batch(_TILES, mask_background=True, **k)),
            ("standardize_batch", lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, **k)),
            ("transform_shard", lambda **k: sn.transform_shard(_TILES, **k)),
            ("slide_luminosity_standardize", lambda **k: slide_luminosity_standardize(_TILES, group=False, **k))]


def test_bad_view_arguments_are_value_errors_and_draw_nothing():
    view = stainlib_amd.TileView((5, 7), rot90=False)
    for name, call in _methods():
        np.random.seed(3)
        with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
            call(view=(5, 7))
        with pytest.raises(ValueError, match="windows= goes with view="):
            call(windows=_WIN)
        with pytest.raises(ValueError, match="does not fit"):
            call(view=stainlib_amd.TileView(10))
        with pytest.raises(ValueError, match="does not fit"):
            call(view=stainlib_amd.TileView((9, 11)))                # fits as it is, not transposed
        with pytest.raises(ValueError, match="outside the 9 x 11 tile"):
            call(view=view, windows=[[0, 0, 0], [5, 4, 6]])
        with pytest.raises(ValueError, match="outside d_mask"):
            call(view=view, windows=[[0, 0, 1], [0, 0, 0]])
        # accepted arguments: the call stops at the tile check (CPU tiles) -- AFTER the argument checks, BEFORE any draw
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(view=view)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(view=view, windows=_WIN)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, name                    # nothing was consumed by a refused call
    for name, call in _methods()[:3]:                                # (the pooled calls enqueue their statistics first: device needed)
        np.random.seed(4)
        with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
            call(view=view, tensor_format="float16")
        after = np.random.uniform()
        np.random.seed(4)
        assert np.random.uniform() == after, name
    from stainlib_amd.distributed import SlideNormalizer
    mz = stainlib_amd.MacenkoNormalizer()
    with pytest.raises(ValueError, match="Reinhard normalizer only"):
        SlideNormalizer(mz, group=False, mode="pooled").transform_shard(_TILES, view=view)


def test_the_draw_is_tile_view_draw_and_nothing_else(monkeypatch):
    """the C calls replaced by a stand-in that records what it is handed, the device helpers by host ones: the global numpy stream
    gives view.draw(n, h, w) -- and nothing else -- behind every check; given windows consume nothing"""
    n, h, w = 2, 9, 11
    seen = []
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "_scratch", lambda *a, **k: torch.zeros(256, dtype=torch.uint8))
    monkeypatch.setattr(engine, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(engine, "_f64", lambda x, shape, device: torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(shape))
    view = stainlib_amd.TileView((5, 5), rot90=False)                # (d_mask 6: the view's own, not the engine call's default)
    nz = stainlib_amd.ReinhardStainNormalizer()
    nz.target_means, nz.target_stds = tuple(np.array([[v]]) for v in _T3), tuple(np.array([[v]]) for v in (10.0, 4.0, 5.0))
    fmt = stainlib_amd.TensorFormat(dtype=torch.float16)
    calls = [("sl_reinhard_view", 3, lambda **k: nz.transform_batch(_TILES, mask_background=True, **k)),
             ("sl_luminosity_view", 3, lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, percentile=80, **k))]
    for cname, nret, call in calls:
        for kw in ({}, dict(tensor_format=fmt)):
            del seen[:]
            np.random.seed(77)
            res = call(view=view, **kw)
            after = np.random.uniform()
            np.random.seed(77)
            win = view.draw(n, h, w)
            assert np.random.uniform() == after, cname               # and nothing else was consumed
            assert len(res) == nret and np.array_equal(res[-1], win) and res[-1].dtype == np.int32
            assert [c[0] for c in seen] == [cname]
            args = seen[0][1]
            assert args[2:7] == (n, h, w, 5, 5) and args[8] == 6
            assert tuple(res[0].shape) == ((n, 3, 5, 5) if kw else (n, 5, 5, 3)) and res[0].dtype == (torch.float16 if kw else torch.uint8)
        np.random.seed(5)
        res = call(view=view, windows=_WIN_55)
        after = np.random.uniform()
        np.random.seed(5)
        assert res[-1] is _WIN_55 and np.random.uniform() == after
    # without a view the calls are today's: the scratch-plus-convert route included
    del seen[:]
    nz.transform_batch(_TILES)
    assert [c[0] for c in seen] == ["sl_reinhard_transform"]
    del seen[:]
    stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES)
    assert [c[0] for c in seen] == ["sl_luminosity_standardize"]


_WIN_55 = np.array([[0, 0, 0], [4, 6, 4]], dtype=np.int32)


def test_c_abi_argument_checks_of_the_lab_view_entry_points_under_asan():
    """`make asan-labview`: tests/abi_argcheck_labview.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the three entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library
    if nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-labview", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

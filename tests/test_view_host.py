"""The crop / flip / rot90 entry point (sl_normalize_view), engine.normalize_view, TileView and view= on the batch methods on the host
side: the draws follow the documented np.random calls, every drawn window fits, and every bad argument is refused before anything is
launched -- no GPU needed."""
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
# device pointers: never read by the host side
RGB, OUT, D6, D2, AB, WIN = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300
N, H, W, OH, OW = 4, 64, 48, 40, 32


def _v(rgb=RGB, out=OUT, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, ms=D6, cs=D2, mt=D6, ct=D2, ab=AB, bg=0, params=None, fmt=None):
    return _ffi.lib().sl_normalize_view(rgb, out, n, h, w, oh, ow, win, d_mask, ms, cs, mt, ct, ab, bg,
                                        C.byref(params) if params is not None else None, C.byref(fmt) if fmt is not None else None, None)


# ---- TileView ---------------------------------------------------------------------------------------------------------------------------
def test_tile_view_mask_and_codes():
    assert stainlib_amd.TileView is stainlib_amd.tile_view.TileView
    v = stainlib_amd.TileView()
    assert (v.size, v.flip, v.rot90, v.d_mask, v.codes) == (None, True, True, 7, list(range(8)))
    assert stainlib_amd.TileView(224).size == (224, 224) and stainlib_amd.TileView((5, 7)).size == (5, 7)
    for flip in (False, True):
        for rot in (False, True):
            v = stainlib_amd.TileView(8, flip=flip, rot90=rot)
            assert v.d_mask == (4 if flip else 0) | (3 if rot else 2 if flip else 0)
            assert v.codes == [c for c in range(8) if c & ~v.d_mask == 0]
    assert stainlib_amd.TileView(8, flip=True, rot90=False).codes == [0, 2, 4, 6]          # half turns go with flips
    assert stainlib_amd.TileView(8, flip=False, rot90=False).codes == [0]
    assert stainlib_amd.TileView(8, flip=False, rot90=True).codes == [0, 1, 2, 3]
    for bad in (0, -3, (4,), (4, 5, 6), "224", 2.5, (4, 0), (True, 4)):
        with pytest.raises(ValueError, match="size must be"):
            stainlib_amd.TileView(bad)


@pytest.mark.parametrize("h,w,size,flip,rot", [(256, 256, 224, True, True), (9, 11, (5, 7), True, False), (9, 11, (5, 5), True, True),
                                                (40, 72, None, True, False), (64, 64, (64, 64), True, True), (40, 72, (40, 40), False, True),
                                                (40, 72, (33, 40), False, False)])
def test_draw_replays_the_documented_calls_and_every_window_fits(h, w, size, flip, rot):
    v = stainlib_amd.TileView(size, flip=flip, rot90=rot)
    oh, ow = v.out_size(h, w)
    assert (oh, ow) == ((h, w) if size is None else v.size)
    n = 1000
    np.random.seed(1234)
    win = v.draw(n, h, w)
    after = np.random.uniform()
    assert win.shape == (n, 3) and win.dtype == np.int32
    # the draw order: the code, then y0, then x0 for that code's window, per tile
    np.random.seed(1234)
    codes = [c for c in range(8) if c & ~v.d_mask == 0]
    for t in range(n):
        d = codes[np.random.randint(len(codes))]
        wh, ww = (ow, oh) if d & 1 else (oh, ow)
        y0 = np.random.randint(0, h - wh + 1)
        x0 = np.random.randint(0, w - ww + 1)
        assert (int(win[t, 0]), int(win[t, 1]), int(win[t, 2])) == (y0, x0, d), t
    assert np.random.uniform() == after                                     # and nothing else was consumed
    d = win[:, 2]
    assert ((d & ~v.d_mask) == 0).all() and set(d.tolist()) == set(codes)
    wh, ww = np.where(d & 1, ow, oh), np.where(d & 1, oh, ow)
    assert (win[:, 0] >= 0).all() and (win[:, 0] + wh <= h).all() and (win[:, 1] >= 0).all() and (win[:, 1] + ww <= w).all()
    assert engine._view_windows(win, n, h, w, oh, ow, v.d_mask).dtype == np.int32
    assert v.draw(0, h, w).shape == (0, 3)


def test_draw_refuses_a_size_that_does_not_fit():
    with pytest.raises(ValueError, match="does not fit"):
        stainlib_amd.TileView(65).draw(1, 64, 64)
    with pytest.raises(ValueError, match="does not fit"):
        stainlib_amd.TileView((30, 80)).draw(1, 40, 72)
    with pytest.raises(ValueError, match="quarter turn"):                  # fits as it is, not transposed
        stainlib_amd.TileView((40, 72)).draw(1, 40, 72)
    with pytest.raises(ValueError, match="quarter turn"):
        stainlib_amd.TileView(None).draw(1, 40, 72)
    assert stainlib_amd.TileView((40, 72), rot90=False).draw(2, 40, 72)[:, :2].tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError, match="n must be"):
        stainlib_amd.TileView(8).draw(-1, 64, 64)


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert "sl_normalize_view" in declared and "sl_normalize_view" in _ffi.EXPORTS
    assert declared == set(_ffi.EXPORTS)
    proto = re.search(r"^SL_API int sl_normalize_view\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    assert len(proto.split(",")) == len(_ffi._SIGNATURES["sl_normalize_view"][1]) == 18
    assert _ffi.lib().sl_version() == 600                    # an extension of ABI 600: no existing struct changes


@pytest.mark.parametrize("kw", BAD_SHAPES + [dict(out=None), dict(win=None), dict(oh=0), dict(ow=0), dict(oh=-1), dict(oh=H + 1),
                                             dict(ow=W + 1), dict(d_mask=-1), dict(d_mask=8), dict(d_mask=1 << 20),
                                             dict(oh=H, ow=W, d_mask=7), dict(oh=H, ow=W, d_mask=1), dict(oh=W + 1, ow=W, d_mask=5),
                                             dict(n=1 << 22, h=32768, w=32768, oh=32768, ow=32768)], ids=str)
def test_bad_pointers_shapes_sizes_and_masks_are_refused(kw):
    for route in ROUTES:
        args = {**route, **kw}
        assert _v(**args) == BADARG, args
        assert _v(**args, bg=1, params=_ffi.default_params(), fmt=_ffi.default_tensor_format()) == BADARG, args


@pytest.mark.parametrize("kw", BAD_STATS, ids=str)
def test_bad_statistics_are_refused(kw):
    assert _v(**kw) == BADARG and _v(**kw, d_mask=6, oh=H, ow=W, fmt=_ffi.default_tensor_format()) == BADARG


@pytest.mark.parametrize("size", [0, 16, -8, 8])
def test_params_struct_size_mismatch_is_refused(size):
    p = _ffi.default_params()
    p.struct_size = size if size in (0, 16) else C.sizeof(_ffi.SlParams) + size
    for route in ROUTES:
        assert _v(**route, params=p) == BADARG
    p.struct_size = C.sizeof(_ffi.SlParams)
    p.two_sweep = 9
    assert _v(params=p) == BADARG


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("struct_size", 16), ("struct_size", 64 + 8), ("dtype", -1), ("dtype", 3),
                                         ("layout", -1), ("layout", 2), ("std", 0.0), ("std", float("nan")), ("mean", float("inf"))])
def test_bad_format_is_refused(field, value):
    f = _ffi.default_tensor_format()
    if field in ("std", "mean"):
        getattr(f, field)[1] = value
    else:
        setattr(f, field, value)
    for route in ROUTES:
        assert _v(**route, fmt=f) == BADARG


# ---- the Python surface: ValueError before the device is touched (the tiles are CPU tensors: reaching the tile check would raise
# ValueError too, so every case matches on its own message) ---------------------------------------------------------------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_M, _MC = torch.zeros((2, 2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.float64)
_AB = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
_WIN = np.array([[0, 0, 0], [4, 4, 6]], dtype=np.int32)


@pytest.mark.parametrize("win,d_mask,msg", [
    ([[0, 0, 0], [5, 4, 6]], 6, "outside the 9 x 11 tile"), ([[0, 0, 0], [4, 5, 6]], 6, "outside the 9 x 11 tile"),
    ([[-1, 0, 0], [0, 0, 0]], 6, "outside the 9 x 11 tile"), ([[0, -1, 0], [0, 0, 0]], 6, "outside the 9 x 11 tile"),
    ([[0, 0, 1], [0, 0, 0]], 6, "outside d_mask"), ([[0, 0, 8], [0, 0, 0]], 7, "outside d_mask"), ([[0, 0, -1], [0, 0, 0]], 7, "outside d_mask"),
    ([[0, 0, 0]], 6, "windows must hold"), ([[0, 0], [0, 0]], 6, "windows must hold"), ([[0.0, 0, 0], [0, 0, 0]], 6, "windows must hold"),
    (None, 6, "windows must hold"), ("wins", 6, "windows must hold")], ids=str)
def test_cpu_windows_are_range_checked(win, d_mask, msg):
    for as_tensor in (False, True):
        wn = torch.tensor(win) if as_tensor and isinstance(win, list) else (np.array(win) if isinstance(win, list) else win)
        with pytest.raises(ValueError, match=msg):
            engine.normalize_view(_TILES, wn, (5, 7), d_mask)
        with pytest.raises(ValueError, match=msg):
            engine.normalize_view(_TILES, wn, (5, 7), d_mask, _M, _MC, None, None, _AB)
    # a 5 x 5 view under d_mask = 7: the window of an odd code is checked as transposed (here the same), 7 x 5 does not fit transposed
    with pytest.raises(ValueError, match="quarter turn"):
        engine.normalize_view(_TILES, _WIN, (5, 10), 7)
    with pytest.raises(ValueError, match="does not fit"):
        engine.normalize_view(_TILES, _WIN, (10, 5), 6)
    with pytest.raises(ValueError, match="d_mask must be"):
        engine.normalize_view(_TILES, _WIN, (5, 5), 8)


def test_in_range_cpu_windows_reach_the_tile_check():
    """accepted windows: the call goes on to the check of the tiles themselves (CPU tensors here)"""
    for win in (_WIN, torch.from_numpy(_WIN), _WIN.astype(np.int64), _WIN.tolist()):
        with pytest.raises(ValueError, match="expected a contiguous CUDA uint8 tensor"):
            engine.normalize_view(_TILES, win, (5, 7), 6)
    with pytest.raises(ValueError, match="expected a contiguous CUDA uint8 tensor"):
        engine.normalize_view(_TILES, np.array([[4, 6, 7], [2, 6, 1]]), (5, 5), 7)          # 5 x 5: the corners of 9 x 11


def test_bad_statistics_format_and_view_are_value_errors():
    with pytest.raises(ValueError, match="go together"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, _M, _MC, _M[0], None, _AB)
    with pytest.raises(ValueError, match="M_src=None is the view of the tiles' own bytes"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, None, _MC)
    with pytest.raises(ValueError, match="M_src=None is the view of the tiles' own bytes"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, alpha_beta=_AB)
    with pytest.raises(ValueError, match="M_src and maxC_src go together"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, _M, None, None, None, _AB)
    with pytest.raises(ValueError, match="needs a target"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, _M, _MC)
    with pytest.raises(ValueError, match="alpha_beta must"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, _M, _MC, None, None, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="alpha_beta must have one row per tile"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, _M, _MC, None, None, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="params must be"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, params=0.01)
    with pytest.raises(ValueError, match="must be a stainlib_amd.TensorFormat"):
        engine.normalize_view(_TILES, _WIN, (5, 7), 6, fmt="float16")
    view = stainlib_amd.TileView((5, 7), rot90=False)
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16)
    nz = stainlib_amd.MacenkoNormalizer()
    sa = stainlib_amd.StainAugmentor("macenko")
    for call in (lambda **k: nz.transform_batch(_TILES, **k), lambda **k: nz.augment_batch(_TILES, _AB, normalize=False, **k),
                 lambda **k: sa.augment_batch(_TILES, _AB, **k), lambda **k: f16.convert(_TILES, **k)):
        with pytest.raises(ValueError, match="view must be a stainlib_amd.TileView"):
            call(view=(5, 7))
        with pytest.raises(ValueError, match="windows= goes with view="):
            call(windows=_WIN)
        with pytest.raises(ValueError, match="outside the 9 x 11 tile"):
            call(view=view, windows=[[0, 0, 0], [5, 4, 6]])
        with pytest.raises(ValueError, match="does not fit"):
            call(view=stainlib_amd.TileView(10))
    # nothing is drawn by a refused call
    np.random.seed(3)
    with pytest.raises(ValueError, match="does not fit"):
        sa.augment_batch(_TILES, view=stainlib_amd.TileView(10))
    after = np.random.uniform()
    np.random.seed(3)
    assert np.random.uniform() == after


def test_route_upload_keeps_none_and_shapes_the_rest():
    """engine._route_upload with the CPU as its device: under each of the four routes what is None stays None, and everything else comes
    back as a contiguous float64 tensor of the shape the C ABI reads, with the caller's values"""
    n = 3
    given = dict(M_src=np.arange(n * 6.0).reshape(n, 6), maxC_src=[[1.0, 2.0]] * n, M_tgt=torch.arange(6, dtype=torch.float32),
                 maxC_tgt=(1.5, 1.1), alpha_beta=np.ones((n, 4)))
    shapes = dict(M_src=(n, 2, 3), maxC_src=(n, 2), M_tgt=(2, 3), maxC_tgt=(2,), alpha_beta=(n, 4))
    cpu = torch.device("cpu")
    for drop in ((), ("alpha_beta",), ("M_tgt", "maxC_tgt"), tuple(given)):                  # jitter, apply, own, raw
        got = engine._route_upload(n, cpu, **{k: None if k in drop else v for k, v in given.items()})
        assert len(got) == 5
        for (k, v), t in zip(given.items(), got):
            if k in drop:
                assert t is None, (drop, k)
            else:
                assert t.dtype == torch.float64 and t.device == cpu and tuple(t.shape) == shapes[k] and t.is_contiguous(), (drop, k)
                assert np.array_equal(t.numpy().ravel(), np.asarray(v, dtype=np.float64).ravel()), (drop, k)
    M = torch.zeros((n, 2, 3), dtype=torch.float64)
    got = engine._route_upload(n, cpu, M, given["maxC_src"])                                  # the short form of the callers without a route
    assert got[0].data_ptr() == M.data_ptr() and got[2:] == (None, None, None)                # (already in place: not copied)


def test_c_abi_argument_checks_of_the_view_entry_point_under_asan():
    """`make asan-view`: tests/abi_argcheck_view.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the entry point.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if
    nothing has yet: about two minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-view", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

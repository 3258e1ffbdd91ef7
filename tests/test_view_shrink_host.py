"""The 2x / 4x box shrink of the view passes on the host side: TileView(shrink=), the window checks of the engine, the five
sl_*_view_shrink entry points and the calls that refuse a shrink -- every bad argument is refused before anything is launched or drawn.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine
from stainlib_amd.augmentation.augmenter import HedColorAugmenter
from stainlib_amd.tile_view import check_size

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
PARENTS = ("sl_normalize_view", "sl_normalize_hed_view", "sl_reinhard_view", "sl_luminosity_view", "sl_slab_view")
# device pointers: never read by the host side
RGB, OUT, D6, D2, AB, WIN = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300
N, H, W = 4, 64, 48


# ---- TileView(shrink=) --------------------------------------------------------------------------------------------------------------------
def test_shrink_is_validated_kept_and_shown():
    for s in (1, 2, 4, np.int32(2)):
        assert stainlib_amd.TileView(8, shrink=s).shrink == int(s)
    assert stainlib_amd.TileView(8).shrink == 1
    for bad in (0, 3, 8, 16, -2, "2", 2.0, True, None, (2,)):
        with pytest.raises(ValueError, match="shrink must be 1, 2 or 4"):
            stainlib_amd.TileView(8, shrink=bad)
        with pytest.raises(ValueError, match="shrink must be 1, 2 or 4"):
            check_size((4, 4), 64, 64, 6, bad)
    assert repr(stainlib_amd.TileView((5, 7), rot90=False, shrink=4)) == "TileView(size=(5, 7), flip=True, rot90=False, shrink=4)"
    assert repr(stainlib_amd.TileView((5, 7), shrink=1)) == repr(stainlib_amd.TileView((5, 7))) == "TileView(size=(5, 7), flip=True, rot90=True)"
    v = stainlib_amd.TileView(8, flip=False, shrink=2)
    assert (v.size, v.d_mask, v.codes) == ((8, 8), 3, [0, 1, 2, 3])          # size stays the OUTPUT size; the codes do not change


def test_out_size_and_check_size_take_the_s_times_window():
    TV = stainlib_amd.TileView
    assert TV((32, 24), rot90=False, shrink=2).out_size(64, 48) == (32, 24)            # a 64 x 48 window: the whole tile
    assert TV((16, 12), rot90=False, shrink=4).out_size(64, 48) == (16, 12)
    for size, s in (((33, 24), 2), ((32, 25), 2), ((17, 12), 4), ((16, 13), 4), ((64, 48), 2)):
        assert TV(size, rot90=False).out_size(64, 48) == size                          # fits at shrink = 1
        with pytest.raises(ValueError, match=rf"shrink={s} .* does not fit in a 64 x 48 tile"):
            TV(size, rot90=False, shrink=s).out_size(64, 48)
        with pytest.raises(ValueError, match="does not fit"):
            check_size(size, 64, 48, 6, s)
    # quarter turns: the transposed s-times window must fit too
    assert TV((24, 24), shrink=2).out_size(64, 48) == (24, 24)
    for size, s in (((32, 24), 2), ((25, 24), 2), ((13, 12), 4), ((16, 8), 4)):
        assert TV(size, rot90=False, shrink=s).out_size(64, 48) == size
        with pytest.raises(ValueError, match="quarter turn"):
            TV(size, shrink=s).out_size(64, 48)
        with pytest.raises(ValueError, match="quarter turn"):
            TV(size, shrink=s).draw(1, 64, 48)
    assert check_size((32, 24), 64, 48, 6) == check_size((32, 24), 64, 48, 6, 1) == (32, 24)


def test_size_none_is_the_tile_in_whole_boxes():
    TV = stainlib_amd.TileView
    assert TV(None, rot90=False, shrink=2).out_size(81, 151) == (40, 75)
    assert TV(None, rot90=False, shrink=4).out_size(81, 151) == (20, 37)
    assert TV(None, rot90=False, shrink=4).out_size(4, 7) == (1, 1)
    assert TV(None, shrink=2).out_size(64, 64) == (32, 32) and TV(None).out_size(64, 64) == (64, 64)
    assert TV(None, shrink=2).out_size(65, 64) == (32, 32)                             # (64 x 64 fits turned in 65 x 64)
    for h, w, s in ((3, 64, 4), (64, 1, 2), (1, 1, 2)):
        with pytest.raises(ValueError, match="below 1 x 1"):
            TV(None, rot90=False, shrink=s).out_size(h, w)
    with pytest.raises(ValueError, match="quarter turn"):
        TV(None, shrink=2).out_size(40, 72)
    win = TV(None, rot90=False, shrink=2).draw(50, 81, 151)                            # 80 x 150 out of 81 x 151: corners 0 or 1
    assert set(win[:, 0].tolist()) == {0, 1} and set(win[:, 1].tolist()) == {0, 1}


@pytest.mark.parametrize("h,w,size,flip,rot,s", [(256, 256, 112, True, True, 2), (81, 151, (33, 37), True, True, 2), (81, 151, (17, 18), True, True, 4),
                                                  (64, 48, (16, 12), True, False, 4), (40, 72, None, False, False, 2), (64, 64, None, True, True, 4)])
def test_draw_replays_the_documented_calls_inside_the_s_times_window(h, w, size, flip, rot, s):
    v = stainlib_amd.TileView(size, flip=flip, rot90=rot, shrink=s)
    oh, ow = v.out_size(h, w)
    assert (oh, ow) == ((h // s, w // s) if size is None else v.size)
    n = 500
    np.random.seed(1234)
    win = v.draw(n, h, w)
    after = np.random.uniform()
    np.random.seed(1234)
    codes = [c for c in range(8) if c & ~v.d_mask == 0]
    for t in range(n):
        d = codes[np.random.randint(len(codes))]
        wh, ww = (ow, oh) if d & 1 else (oh, ow)
        y0 = np.random.randint(0, h - s * wh + 1)
        x0 = np.random.randint(0, w - s * ww + 1)
        assert (int(win[t, 0]), int(win[t, 1]), int(win[t, 2])) == (y0, x0, d), t
    assert np.random.uniform() == after                                     # and nothing else was consumed
    d = win[:, 2]
    wh, ww = s * np.where(d & 1, ow, oh), s * np.where(d & 1, oh, ow)
    assert (win[:, 0] >= 0).all() and (win[:, 0] + wh <= h).all() and (win[:, 1] >= 0).all() and (win[:, 1] + ww <= w).all()
    assert win.dtype == np.int32 and engine._view_windows(win, n, h, w, oh, ow, v.d_mask, s).dtype == np.int32


@pytest.mark.parametrize("h,w,size,flip,rot", [(256, 256, 224, True, True), (9, 11, (5, 7), True, False), (40, 72, None, True, False)])
def test_shrink_one_draws_the_same_array_from_the_same_stream(h, w, size, flip, rot):
    v0, v1 = stainlib_amd.TileView(size, flip=flip, rot90=rot), stainlib_amd.TileView(size, flip, rot, 1)
    assert v0.out_size(h, w) == v1.out_size(h, w) and v0.d_mask == v1.d_mask
    np.random.seed(99)
    w0 = v0.draw(300, h, w)
    s0 = np.random.get_state()
    np.random.seed(99)
    w1 = v1.draw(300, h, w)
    s1 = np.random.get_state()
    assert np.array_equal(w0, w1) and w0.dtype == w1.dtype and s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]


# ---- the window checks of the engine --------------------------------------------------------------------------------------------------------
def test_view_windows_refuses_a_window_that_fits_only_unshrunk():
    n, h, w, oh, ow = 2, 64, 48, 20, 16
    win = np.array([[40, 30, 0], [24, 16, 6]], dtype=np.int32)               # 20 x 16 at (40, 30) ends at (60, 46): inside
    assert np.array_equal(engine._view_windows(win, n, h, w, oh, ow, 6), win)
    assert np.array_equal(engine._view_windows(win, n, h, w, oh, ow, 6, 1), win)
    with pytest.raises(ValueError, match=r"tile 0 has its 40 x 32 window at \(40, 30\), outside the 64 x 48 tile"):
        engine._view_windows(win, n, h, w, oh, ow, 6, 2)
    ok2 = np.array([[24, 16, 0], [0, 0, 6]], dtype=np.int32)                 # 40 x 32 at (24, 16): flush against the end
    assert np.array_equal(engine._view_windows(ok2, n, h, w, oh, ow, 6, 2), ok2)
    for bad in ([[25, 16, 0], [0, 0, 0]], [[24, 17, 0], [0, 0, 0]]):
        with pytest.raises(ValueError, match="outside the 64 x 48 tile"):
            engine._view_windows(np.array(bad), n, h, w, oh, ow, 6, 2)
    # an odd code takes the transposed s-times window: 32 x 40 at s = 2 out of 64 x 48
    assert engine._view_windows(np.array([[32, 8, 1], [0, 0, 3]]), n, h, w, oh, ow, 7, 2).dtype == np.int32
    with pytest.raises(ValueError, match=r"its 32 x 40 window at \(33, 8\)"):
        engine._view_windows(np.array([[33, 8, 1], [0, 0, 3]]), n, h, w, oh, ow, 7, 2)


_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_WIN = np.array([[0, 0, 0], [1, 3, 6]], dtype=np.int32)                       # 2 x 4 output: an 8 x 8 window at s = 2 fits at (1, 3)
_T3 = np.array([50.0, 2.0, 3.0])
_STATE = torch.zeros(_ffi.SLAB_STATE_DOUBLES, dtype=torch.float64)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def _engine_calls():
    sg, ap = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    return [("normalize_view", lambda win=_WIN, size=(4, 4), **k: engine.normalize_view(_TILES, win, size, 6, **k)),
            ("normalize_hed_view", lambda win=_WIN, size=(4, 4), **k: engine.normalize_hed_view(_TILES, win, size, 6, sg, sg, ap, **k)),
            ("reinhard_view", lambda win=_WIN, size=(4, 4), **k: engine.reinhard_view(_TILES, win, size, _T3, _T3, 6, **k)),
            ("luminosity_view", lambda win=_WIN, size=(4, 4), **k: engine.luminosity_view(_TILES, win, size, d_mask=6, **k)),
            ("slab_view", lambda win=_WIN, size=(4, 4), **k: engine.slab_view(_TILES, win, size, _STATE, 0, 6, **k))]


def test_the_engine_calls_check_the_shrink_and_the_s_times_window():
    for name, call in _engine_calls():
        for bad in (0, 3, 8, "2", None):
            with pytest.raises(ValueError, match="shrink must be 1, 2 or 4"):
                call(shrink=bad)
        with pytest.raises(ValueError, match=_TILE_CHECK):                    # accepted: on to the tile check (CPU tiles here)
            call(shrink=2)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(size=(2, 2), shrink=4)
        with pytest.raises(ValueError, match="does not fit"):                 # 5 x 4 fits; its 10 x 8 window does not
            call(size=(5, 4), shrink=2)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(size=(5, 4))
        with pytest.raises(ValueError, match="outside the 9 x 11 tile"):      # fits at (1, 4) as 4 x 4, not as 8 x 8
            call(win=np.array([[0, 0, 0], [1, 4, 6]]), shrink=2)
        with pytest.raises(ValueError, match=_TILE_CHECK):
            call(win=np.array([[0, 0, 0], [1, 4, 6]]))
        with pytest.raises(ValueError, match=_TILE_CHECK):                    # size=None: 4 x 5 boxes of 2 x 2
            call(win=np.array([[1, 1, 0], [0, 0, 6]]), size=None, shrink=2)
        with pytest.raises(ValueError, match="outside the 9 x 11 tile"):
            call(win=np.array([[2, 1, 0], [0, 0, 6]]), size=None, shrink=2)


def test_the_c_call_is_the_parent_at_shrink_one_and_the_shrink_export_otherwise(monkeypatch):
    n, h, w = 2, 9, 11
    seen = []
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "_scratch", lambda *a, **k: torch.zeros(256, dtype=torch.uint8))
    monkeypatch.setattr(engine, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(engine, "_f64", lambda x, shape, device: torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(shape))
    for (name, call), parent in zip(_engine_calls(), PARENTS):
        for s in (1, 2, 4):
            del seen[:]
            size = (4, 4) if s < 4 else (2, 2)
            res = call(size=size, shrink=s)
            out = res[0] if isinstance(res, tuple) else res
            assert tuple(out.shape) == (n, *size, 3)
            assert [c[0] for c in seen] == [parent if s == 1 else parent + "_shrink"], (name, s)
            args = seen[0][1]
            assert args[2:7] == (n, h, w, *size) and args[8] == 6
            assert len(args) + 1 == len(_ffi._SIGNATURES[seen[0][0]][1])    # (+ the stream)
            if s != 1:
                assert args[9] == s
    # a view= carries its shrink through the batch methods
    view = stainlib_amd.TileView((4, 4), rot90=False, shrink=2)
    nz = stainlib_amd.ReinhardStainNormalizer()
    nz.target_means, nz.target_stds = tuple(np.array([[v]]) for v in _T3), tuple(np.array([[v]]) for v in (10.0, 4.0, 5.0))
    for cname, call in (("sl_reinhard_view_shrink", lambda **k: nz.transform_batch(_TILES, **k)),
                        ("sl_luminosity_view_shrink", lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, **k)),
                        ("sl_normalize_view_shrink", lambda **k: (stainlib_amd.TensorFormat(dtype=torch.float16).convert(_TILES, **k)))):
        del seen[:]
        np.random.seed(7)
        res = call(view=view)
        after = np.random.uniform()
        np.random.seed(7)
        assert np.array_equal(res[-1], view.draw(n, h, w)) and np.random.uniform() == after
        assert [c[0] for c in seen] == [cname] and seen[0][1][5:10] == (4, 4, seen[0][1][7], 6, 2)


# ---- the HED modes that go through the chain do not know a shrink ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["0.19", "0.17", "experimental_log10"])
def test_chain_hed_modes_refuse_a_shrink_by_name_and_draw_nothing(mode):
    aug = HedColorAugmenter(*[(-0.1, 0.1)] * 6, cutoff_range=(0.0, 1.0), skimage_mode=mode)
    ok = HedColorAugmenter(*[(-0.1, 0.1)] * 6, cutoff_range=(0.0, 1.0))
    view = stainlib_amd.TileView((4, 4), rot90=False, shrink=2)
    plain = stainlib_amd.TileView((4, 4), rot90=False)
    nz = stainlib_amd.MacenkoNormalizer()
    sa = stainlib_amd.StainAugmentor("macenko")
    ab = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
    calls = [lambda hed, **k: nz.transform_batch(_TILES, hed=hed, **k), lambda hed, **k: nz.augment_batch(_TILES, ab, normalize=False, hed=hed, **k),
             lambda hed, **k: sa.augment_batch(_TILES, hed=hed, **k), lambda hed, **k: hed.transform_batch(_TILES, **k)]
    for call in calls:
        np.random.seed(3)
        with pytest.raises(ValueError, match=re.escape(repr(mode)) + r".*shrink=2"):
            call(aug, view=view)
        with pytest.raises(ValueError, match=re.escape(repr(mode)) + r".*shrink=2"):
            call(aug, view=view, windows=_WIN)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after                                    # nothing was drawn
        for hed, v in ((aug, plain), (ok, view)):                             # without a shrink, or in the pinned mode: on to the tile check
            with pytest.raises(ValueError, match=_TILE_CHECK):
                call(hed, view=v, windows=_WIN)
    sg, ap = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    code = {"0.19": 1, "0.17": 2, "experimental_log10": 3}[mode]
    with pytest.raises(ValueError, match=re.escape(repr(mode)) + r".*shrink=4"):
        engine.normalize_hed_view(_TILES, _WIN, (2, 2), 6, sg, sg, ap, code, shrink=4)
    with pytest.raises(ValueError, match=_TILE_CHECK):
        engine.normalize_hed_view(_TILES, _WIN, (2, 2), 6, sg, sg, ap, code)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_shrink_exports():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for parent in PARENTS:
        name = parent + "_shrink"
        assert name in declared and hasattr(_ffi.lib(), name)
        proto = [a.strip() for a in re.search(rf"^SL_API int {name}\((.*?)\);", hdr, flags=re.M | re.S).group(1).split(",")]
        old = [a.strip() for a in re.search(rf"^SL_API int {parent}\((.*?)\);", hdr, flags=re.M | re.S).group(1).split(",")]
        assert proto == old[:9] + ["int shrink"] + old[9:] and old[8] == "int d_mask"
        pa, na = _ffi._SIGNATURES[parent][1], _ffi._SIGNATURES[name][1]
        assert len(na) == len(proto) and na == pa[:9] + [C.c_int] + pa[9:]
    assert _ffi.lib().sl_version() == 600                    # added exports do not bump the version


def _v(oh, ow, d_mask, s, rgb=RGB, out=OUT, win=WIN, ms=D6):
    return _ffi.lib().sl_normalize_view_shrink(rgb, out, N, H, W, oh, ow, win, d_mask, s, ms, D2 if ms else None, ms, D2 if ms else None,
                                               AB if ms else None, 0, None, None, None)


@pytest.mark.parametrize("oh,ow,d_mask,s", [(8, 8, 7, 0), (8, 8, 7, 3), (8, 8, 7, 8), (8, 8, 7, -2), (8, 8, 7, 1 << 30), (33, 24, 6, 2), (32, 25, 6, 2),
                                            (17, 12, 6, 4), (16, 13, 6, 4), (64, 48, 0, 2), (2 ** 31 - 1, 1, 0, 2), (1, 2 ** 30, 0, 4),
                                            (32, 24, 7, 2), (25, 24, 3, 2), (13, 12, 5, 4), (16, 8, 1, 4), (0, 8, 6, 2), (8, 8, 8, 2)])
def test_the_view_export_refuses_bad_shrinks_and_windows_that_do_not_fit(oh, ow, d_mask, s):
    assert _v(oh, ow, d_mask, s) == BADARG and _v(oh, ow, d_mask, s, ms=None) == BADARG
    assert _v(8, 8, 7, 2, rgb=None) == BADARG and _v(8, 8, 7, 4, out=None) == BADARG and _v(8, 8, 7, 2, win=None) == BADARG


def test_c_abi_argument_checks_of_the_shrink_entry_points_under_asan():
    """`make asan-shrink`: tests/abi_argcheck_shrink.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the five entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library
    if nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-shrink", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

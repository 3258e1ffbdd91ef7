"""The resizing view (random-resized crop: TileView(scale=, ratio=), sl_normalize_view_resize, sl_normalize_hed_view_resize) on the host
side: the arguments of TileView, its draw, the (N, 5) window checks of the engine, the calls that refuse a resizing view, the two
exports -- and the numpy restatement of the definition (resample_ref, want_view), which tests/test_gpu_view_resize.py compares the
kernels against bit for bit.  No GPU needed."""
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
from stainlib_amd.tile_view import area_resample, overlap_matrix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
PARENTS = ("sl_normalize_view", "sl_normalize_hed_view")
RGB, OUT, D6, D2, AB, WIN, SG, AP = 0x100000, 0x200000, 0x300000, 0x300100, 0x300200, 0x300300, 0x300400, 0x300500   # never read by the host side
N, H, W = 4, 64, 48
MAX_AREA = 1 << 22


# ---- the definition, restated ---------------------------------------------------------------------------------------------------------------
def overlaps(nw, no):
    """c of the definition, interval by interval: c[i][k] = |[i nw, (i + 1) nw) & [k no, (k + 1) no)| in coordinates scaled by no"""
    c = np.zeros((no, nw), dtype=np.int64)
    for i in range(no):
        for k in range(nw):
            c[i, k] = max(0, min((i + 1) * nw, (k + 1) * no) - max(i * nw, k * no))
    return c


def resample_ref(window, nu, nv):
    """(wh, ww, 3) uint8 -> (nu, nv, 3) uint8: S = sum cy cx window in exact integers, b = (2 S + D) // (2 D) -- and S with it"""
    window = np.asarray(window)
    wh, ww = window.shape[:2]
    cy, cx = overlaps(wh, nu), overlaps(ww, nv)
    S = np.tensordot(np.tensordot(cy, window.astype(np.int64), axes=(1, 0)), cx, axes=(1, 1)).transpose(0, 2, 1)       # (nu, nv, c)
    D = wh * ww
    assert int(S.max()) <= 255 * D and 2 * 255 * D + D < 2 ** 63
    return ((2 * S + D) // (2 * D)).astype(np.uint8), S


def clamp_window(row, h, w, oh, ow, d_mask=7, resize=None):
    """one window (y0, x0, d, wh, ww) as the kernel clamps it -> (y0, x0, d, wh, ww, nu, nv)"""
    y0, x0, d, wh, ww = (int(v) for v in row)
    d &= d_mask
    nu, nv = (ow, oh) if d & 1 else (oh, ow)
    mh, mw = resize if resize is not None else (h, w)
    wh = max(1, min(wh, min(mh, 16 * nu)))
    ww = max(1, min(ww, min(mw, 16 * nv)))
    return max(0, min(y0, h - wh)), max(0, min(x0, w - ww)), d, wh, ww, nu, nv


def want_view(full, win, size, d_mask=7, resize=None, dihedral_first=False):
    """the definition on `full` ((n, h, w, 3) uint8 numpy) -> (n, oh, ow, 3) uint8: clamp, slice, resample, flip along the width, rot90 --
    or the dihedral transform of the window first, then the resample to (oh, ow) (they commute)"""
    full = np.asarray(full)
    n, h, w, _ = full.shape
    oh, ow = size
    outs = []
    for t in range(n):
        y0, x0, d, wh, ww, nu, nv = clamp_window(win[t], h, w, oh, ow, d_mask, resize)
        v = full[t, y0:y0 + wh, x0:x0 + ww]

        def dihedral(v):
            return np.rot90(v[:, ::-1] if d & 4 else v, d & 3, axes=(0, 1))

        b = resample_ref(dihedral(v), oh, ow)[0] if dihedral_first else dihedral(resample_ref(v, nu, nv)[0])
        assert b.shape == (oh, ow, 3)
        outs.append(b)
    return np.ascontiguousarray(np.stack(outs))


@pytest.mark.parametrize("nw,no", [(1, 1), (1, 33), (33, 1), (3, 33), (5, 37), (66, 33), (81, 33), (151, 37), (150, 37), (20, 37), (80, 5), (79, 5),
                                   (64, 4), (50, 29), (37, 37)])
def test_overlap_rows_sum_to_the_window_and_columns_to_the_output(nw, no):
    c = overlaps(nw, no)
    assert (c.sum(axis=1) == nw).all() and (c.sum(axis=0) == no).all() and (c >= 0).all()
    assert np.array_equal(c, overlap_matrix(nw, no))
    assert int((c > 0).sum(axis=1).max()) <= -(-nw // no) + 1                # ceil(nw / no) + 1 taps at the most: 17 at ratio 16
    if nw == 79:
        assert int((c > 0).sum(axis=1).max()) == 17


def test_the_definition_is_the_window_the_box_means_and_commutes_with_the_eight_codes():
    rng = np.random.RandomState(7)
    full = rng.randint(0, 256, (8, 81, 151, 3)).astype(np.uint8)
    w = full[0, 3:3 + 33, 5:5 + 37]
    assert np.array_equal(resample_ref(w, 33, 37)[0], w)                                       # identity
    for s, (oh, ow) in ((2, (33, 37)), (4, (17, 18))):                                         # the box sums of tests/test_gpu_view_shrink.py
        v = full[1, 2:2 + s * oh, 7:7 + s * ow]
        S = v.astype(np.int64).reshape(oh, s, ow, s, 3).sum(axis=(1, 3))
        b, S2 = resample_ref(v, oh, ow)
        assert np.array_equal(S2, S * oh * ow) and np.array_equal(b, ((S + s * s // 2) >> (2 * (s // 2))).astype(np.uint8))
    for wh, ww in ((81, 151), (81, 20), (3, 5), (1, 1), (47, 50)):                             # the package's own numpy form
        v = full[2, :wh, :ww]
        assert np.array_equal(resample_ref(v, 33, 37)[0], area_resample(v, 33, 37))
    win = np.array([[t, 2 * t, t, 40 + 5 * t, 30 + 9 * t] for t in range(8)])
    a, b = want_view(full, win, (33, 37)), want_view(full, win, (33, 37), dihedral_first=True)
    assert np.array_equal(a, b) and a.shape == (8, 33, 37, 3)                                  # resample(dihedral(.)) == dihedral(resample(.))
    assert (resample_ref(np.full((81, 151, 3), 255, np.uint8), 33, 37)[0] == 255).all()
    up = resample_ref(np.array([[[10] * 3, [201] * 3]], dtype=np.uint8), 1, 3)[0]              # upscaling: constant pieces, a blended edge
    assert up[0, :, 0].tolist() == [10, 106, 201]


# ---- TileView(scale=, ratio=) -----------------------------------------------------------------------------------------------------------------
def test_scale_and_ratio_are_validated_kept_and_shown():
    TV = stainlib_amd.TileView
    v = TV(224, scale=(0.08, 1))
    assert v.scale == (0.08, 1.0) and v.ratio == (0.75, 4.0 / 3.0) and v.resizing and v.shrink == 1 and v.size == (224, 224)
    assert not TV(224).resizing and TV(224).scale is None
    assert repr(TV(224)) == "TileView(size=(224, 224), flip=True, rot90=True)"                 # scale=None is today's object
    assert repr(TV((5, 7), rot90=False, scale=(0.5, 0.5), ratio=(1, 2))) == \
        "TileView(size=(5, 7), flip=True, rot90=False, scale=(0.5, 0.5), ratio=(1.0, 2.0))"
    for bad in ((0, 1), (-0.1, 0.5), (0.5, 0.4), (0.5, 1.01), 0.5, (0.5,), (0.1, 0.5, 1), "ab", (None, 1), (float("nan"), 1)):
        with pytest.raises(ValueError, match="scale must be a pair"):
            TV(8, scale=bad)
    for bad in ((0, 1), (2, 1), (-1, 1), 1.0, (1,), (1, float("inf")), "xy"):
        with pytest.raises(ValueError, match="ratio must be a pair"):
            TV(8, scale=(0.5, 1), ratio=bad)
    for s in (2, 4):
        with pytest.raises(ValueError, match=rf"scale=.*shrink={s}"):
            TV(8, shrink=s, scale=(0.5, 1))
    assert TV(8, shrink=1, scale=(0.5, 1)).resizing
    # the output need not fit in the tile, in any orientation; size=None is the tile's own size
    assert TV((100, 30), scale=(0.5, 1)).out_size(64, 48) == (100, 30) and TV(None, scale=(0.5, 1)).out_size(64, 48) == (64, 48)
    with pytest.raises(ValueError, match="2\\^30"):
        TV(2 ** 20, scale=(0.5, 1)).out_size(2048, 2048)


def _replay(v, n, h, w):
    """the documented order of draw, restated"""
    oh, ow = v.out_size(h, w)
    codes = [c for c in range(8) if c & ~v.d_mask == 0]
    big = max(oh, ow) if v.d_mask & 1 else 0
    bh, bw = min(h, 16 * (big or oh)), min(w, 16 * (big or ow))           # window_bound: one bound for every window of a call
    while bh * bw > MAX_AREA:
        f = np.sqrt(MAX_AREA / float(bh * bw))
        bh, bw = max(1, int(bh * f)), max(1, int(bw * f))
    assert (bh, bw) == v.window_bound(h, w)
    win = []
    for _ in range(n):
        d = codes[np.random.randint(len(codes))]
        nu, nv = (ow, oh) if d & 1 else (oh, ow)
        a = np.random.uniform(*v.scale)
        r = np.exp(np.random.uniform(np.log(v.ratio[0]), np.log(v.ratio[1])))
        wh = int(np.clip(np.floor(np.sqrt(a * h * w / r) + 0.5), 1, min(h, 16 * nu, bh)))
        ww = int(np.clip(np.floor(np.sqrt(a * h * w * r) + 0.5), 1, min(w, 16 * nv, bw)))
        y0 = np.random.randint(0, h - wh + 1)
        x0 = np.random.randint(0, w - ww + 1)
        win.append((y0, x0, d, wh, ww))
    return np.array(win, dtype=np.int32).reshape(n, 5)


@pytest.mark.parametrize("h,w,size,flip,rot,scale,ratio", [
    (1024, 1024, 224, True, True, (0.08, 1), (3 / 4, 4 / 3)), (81, 151, (33, 37), True, True, (0.08, 1), (3 / 4, 4 / 3)),
    (81, 151, (5, 4), True, True, (0.5, 1), (0.25, 4)),                      # the ratio limit clamps: 16 x the output
    (64, 48, (100, 30), False, False, (0.01, 0.02), (1, 1)), (40, 72, None, True, False, (1, 1), (0.1, 10)),
    (3000, 2500, 224, True, True, (0.9, 1), (0.5, 2))])                      # the area limit reduces: 7.5 M pixels
def test_draw_replays_the_documented_calls_inside_the_limits(h, w, size, flip, rot, scale, ratio):
    v = stainlib_amd.TileView(size, flip=flip, rot90=rot, scale=scale, ratio=ratio)
    oh, ow = v.out_size(h, w)
    n = 300
    np.random.seed(1234)
    win = v.draw(n, h, w)
    after = np.random.uniform()
    np.random.seed(1234)
    assert np.array_equal(win, _replay(v, n, h, w)) and np.random.uniform() == after           # five draws per tile and nothing else
    assert win.dtype == np.int32 and win.shape == (n, 5)
    y0, x0, d, wh, ww = win.T.astype(np.int64)
    nu, nv = np.where(d & 1, ow, oh), np.where(d & 1, oh, ow)
    assert ((d & ~v.d_mask) == 0).all() and (wh >= 1).all() and (ww >= 1).all() and (wh <= 16 * nu).all() and (ww <= 16 * nv).all()
    assert (wh * ww <= MAX_AREA).all() and (y0 >= 0).all() and (y0 + wh <= h).all() and (x0 >= 0).all() and (x0 + ww <= w).all()
    mh, mw = v.window_bound(h, w)
    assert (wh <= mh).all() and (ww <= mw).all() and 1 <= mh <= h and 1 <= mw <= w and mh * mw <= MAX_AREA
    assert engine._view_windows(win, n, h, w, oh, ow, v.d_mask, 1, (mh, mw)).dtype == np.int32
    assert engine._view_resize(v, win, torch.zeros((1, 1, 1, 1), dtype=torch.uint8).expand(n, h, w, 3)) == (int(wh.max()), int(ww.max()))
    if (h, w) == (3000, 2500):
        assert (wh * ww > MAX_AREA - 8000).any()                             # (the reduction is not a collapse)
    if size == (5, 4):
        assert ((wh == 16 * nu) | (ww == 16 * nv)).any()


def test_scale_none_draws_todays_array_from_todays_stream():
    v0, v1 = stainlib_amd.TileView(24), stainlib_amd.TileView(24, scale=None, ratio=(0.5, 2))
    np.random.seed(5)
    w0 = v0.draw(100, 64, 48)
    a0 = np.random.uniform()
    np.random.seed(5)
    w1 = v1.draw(100, 64, 48)
    assert np.array_equal(w0, w1) and w1.shape == (100, 3) and np.random.uniform() == a0


# ---- the (N, 5) window checks of the engine ---------------------------------------------------------------------------------------------------
def test_host_windows_are_range_checked():
    n, h, w, oh, ow = 2, 64, 48, 3, 2
    ok = np.array([[0, 0, 0, 48, 32], [16, 16, 1, 32, 32]], dtype=np.int32)            # 16 x the output; the odd code takes (2, 3) outputs
    chk = lambda win, d_mask=7, resize=(64, 48): engine._view_windows(win, n, h, w, oh, ow, d_mask, 1, resize)        # noqa: E731
    assert np.array_equal(chk(ok), ok) and chk(ok.astype(np.int64)).dtype == np.int32
    assert np.array_equal(chk(torch.from_numpy(ok)), ok)
    for bad, msg in (([[0, 0, 0, 49, 32], [0, 0, 0, 1, 1]], r"tile 0 has a 49 x 32 window, outside 1 x 1 \.\. 48 x 32"),
                     ([[0, 0, 0, 48, 33], [0, 0, 0, 1, 1]], "tile 0 has a 48 x 33 window"),
                     ([[0, 0, 0, 1, 1], [0, 0, 1, 33, 32]], r"tile 1 has a 33 x 32 window, outside 1 x 1 \.\. 32 x 48"),
                     ([[0, 0, 0, 0, 4], [0, 0, 0, 1, 1]], "tile 0 has a 0 x 4 window"),
                     ([[0, 0, 0, 4, -1], [0, 0, 0, 1, 1]], "tile 0 has a 4 x -1 window"),
                     ([[17, 0, 0, 48, 32], [0, 0, 0, 1, 1]], r"its 48 x 32 window at \(17, 0\), outside the 64 x 48 tile"),
                     ([[0, 17, 0, 48, 32], [0, 0, 0, 1, 1]], "outside the 64 x 48 tile"),
                     ([[-1, 0, 0, 4, 4], [0, 0, 0, 1, 1]], "outside the 64 x 48 tile"),
                     ([[0, 0, 8, 4, 4], [0, 0, 0, 1, 1]], "tile 0 has the code 8"),
                     ([[0, 0, 0, 4, 4], [0, 0, 1, 1, 1]], "tile 1 has the code 1, outside d_mask = 6")):
        with pytest.raises(ValueError, match=msg):
            chk(np.array(bad), 6 if "d_mask" in msg else 7)
    with pytest.raises(ValueError, match=r"tile 0 has a 48 x 32 window, outside 1 x 1 \.\. 40 x 32"):    # beyond the call's own bound
        chk(ok, resize=(40, 48))
    for bad in (None, ok[:, :3], ok[:1], ok.astype(np.float64), "windows"):
        with pytest.raises(ValueError, match=r"\(y0, x0, d, wh, ww\)"):
            chk(bad)
    # resize= itself
    tiles = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    for bad, msg in (((0, 4), "within 1 x 1 and the 64 x 48 tile"), ((65, 4), "within"), ((4, 49), "within"), ((4,), "resize must be"),
                     ((4.0, 4), "resize must be"), ("ab", "resize must be"), (True, "resize must be")):
        with pytest.raises(ValueError, match=msg):
            engine.normalize_view(tiles, ok, (oh, ow), 7, resize=bad)
    with pytest.raises(ValueError, match="at most 2\\^22 pixels"):
        engine.normalize_view(torch.zeros((1, 2049, 2048, 3), dtype=torch.uint8), np.array([[0, 0, 0, 4, 4]]), (224, 224), 7, resize=(2049, 2048))
    with pytest.raises(ValueError, match="does not go with shrink=2"):
        engine.normalize_view(tiles, ok, (oh, ow), 7, shrink=2, resize=(64, 48))
    with pytest.raises(ValueError, match="expected a contiguous CUDA uint8 tensor"):         # accepted: on to the tile check (CPU tiles here)
        engine.normalize_view(tiles, ok, (oh, ow), 7, resize=(64, 48))
    with pytest.raises(ValueError, match="expected a contiguous CUDA uint8 tensor"):
        engine.normalize_hed_view(tiles, ok, (100, 100), 7, np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int32), resize=(48, 32))


def test_the_c_call_is_the_resize_export_with_the_bound_behind_d_mask(monkeypatch):
    n, h, w = 2, 9, 11
    tiles = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    seen = []
    monkeypatch.setattr(engine, "_check_tiles", lambda t: (n, h, w))
    monkeypatch.setattr(engine, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(engine, "_f64", lambda x, shape, device: torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(shape))
    win = np.array([[0, 0, 0, 9, 11], [1, 3, 6, 5, 2]], dtype=np.int32)
    sg, ap = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
    for parent, call in (("sl_normalize_view", lambda **k: engine.normalize_view(tiles, win, (4, 6), 6, **k)),
                         ("sl_normalize_hed_view", lambda **k: engine.normalize_hed_view(tiles, win, (4, 6), 6, sg, sg, ap, **k))):
        del seen[:]
        out = call(resize=(9, 11))
        assert tuple(out.shape) == (n, 4, 6, 3) and [c[0] for c in seen] == [parent + "_resize"]
        args = seen[0][1]
        assert args[2:7] == (n, h, w, 4, 6) and args[8:11] == (6, 9, 11) and len(args) + 1 == len(_ffi._SIGNATURES[parent + "_resize"][1])
    # a view= carries its bound through the batch methods: host windows give their own largest sides, a draw the view's bound
    view = stainlib_amd.TileView((4, 6), rot90=False, scale=(0.3, 1))
    fmt = stainlib_amd.TensorFormat(dtype=torch.float16)
    del seen[:]
    x, w2 = fmt.convert(tiles, view=view, windows=win)
    assert w2 is win and tuple(x.shape) == (n, 3, 4, 6) and seen[0][0] == "sl_normalize_view_resize" and seen[0][1][8:11] == (6, 9, 11)
    del seen[:]
    fmt.convert(tiles, view=view, windows=np.array([[0, 0, 0, 3, 7], [1, 3, 6, 5, 2]]))
    assert seen[0][1][8:11] == (6, 5, 7)
    del seen[:]
    np.random.seed(7)
    x, wd = fmt.convert(tiles, view=view)
    after = np.random.uniform()
    np.random.seed(7)
    assert np.array_equal(wd, view.draw(n, h, w)) and wd.shape == (n, 5) and np.random.uniform() == after
    assert seen[0][0] == "sl_normalize_view_resize" and seen[0][1][8:11] == (6, int(wd[:, 3].max()), int(wd[:, 4].max()))
    assert view.window_bound(h, w) == (9, 11) == engine._view_resize(view, None, tiles)      # what windows on the device would take


# ---- the calls that refuse a resizing view ----------------------------------------------------------------------------------------------------
_TILES = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
_WIN = np.array([[0, 0, 0, 4, 4], [1, 3, 6, 8, 8]], dtype=np.int32)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"


def test_the_lab_family_refuses_a_resizing_view_by_name_and_draws_nothing():
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    view = stainlib_amd.TileView((4, 4), rot90=False, scale=(0.5, 1))
    nz = stainlib_amd.ReinhardStainNormalizer()
    nz.target_means, nz.target_stds = tuple(np.array([[v]]) for v in (50.0, 2.0, 3.0)), tuple(np.array([[v]]) for v in (10.0, 4.0, 5.0))
    t3 = np.array([50.0, 2.0, 3.0])
    state = torch.zeros(_ffi.SLAB_STATE_DOUBLES, dtype=torch.float64)
    calls = [lambda **k: nz.transform_batch(_TILES, **k),
             lambda **k: stainlib_amd.LuminosityStandardizer.standardize_batch(_TILES, **k),
             lambda **k: SlideNormalizer(nz, group=False, mode="pooled").transform_shard(_TILES, **k),
             lambda **k: slide_luminosity_standardize(_TILES, group=False, **k),
             lambda **k: engine.reinhard_view(_TILES, k.get("windows"), None, t3, t3, view=k["view"]),
             lambda **k: engine.luminosity_view(_TILES, k.get("windows"), None, view=k["view"]),
             lambda **k: engine.slab_view(_TILES, k.get("windows"), None, state, 0, view=k["view"])]
    for i, call in enumerate(calls):
        np.random.seed(3)
        for kw in (dict(view=view), dict(view=view, windows=_WIN)):
            with pytest.raises(ValueError, match=r"resizing view \(TileView\(.*scale=\(0\.5, 1\.0\).*Lab-family.*convert\(view=\)"):
                call(**kw)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after, i                                 # nothing was drawn


@pytest.mark.parametrize("mode", ["0.19", "0.17", "experimental_log10"])
def test_chain_hed_modes_refuse_a_resizing_view_by_name_and_draw_nothing(mode):
    aug = HedColorAugmenter(*[(-0.1, 0.1)] * 6, cutoff_range=(0.0, 1.0), skimage_mode=mode)
    ok = HedColorAugmenter(*[(-0.1, 0.1)] * 6, cutoff_range=(0.0, 1.0))
    view = stainlib_amd.TileView((4, 4), rot90=False, scale=(0.5, 1))
    nz = stainlib_amd.MacenkoNormalizer()
    sa = stainlib_amd.StainAugmentor("macenko")
    ab = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (2, 1))
    calls = [lambda hed, **k: nz.transform_batch(_TILES, hed=hed, **k), lambda hed, **k: nz.augment_batch(_TILES, ab, normalize=False, hed=hed, **k),
             lambda hed, **k: sa.augment_batch(_TILES, hed=hed, **k), lambda hed, **k: hed.transform_batch(_TILES, **k)]
    for call in calls:
        np.random.seed(3)
        for kw in (dict(view=view), dict(view=view, windows=_WIN)):
            with pytest.raises(ValueError, match=re.escape(repr(mode)) + r".*resizing view"):
                call(aug, **kw)
        after = np.random.uniform()
        np.random.seed(3)
        assert np.random.uniform() == after                                    # nothing was drawn
        with pytest.raises(ValueError, match=_TILE_CHECK):                     # in the pinned mode: on to the tile check
            call(ok, view=view, windows=_WIN)
    sg, ap = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    code = {"0.19": 1, "0.17": 2, "experimental_log10": 3}[mode]
    with pytest.raises(ValueError, match=re.escape(repr(mode)) + r".*resizing view"):
        engine.normalize_hed_view(_TILES, _WIN, (4, 4), 6, sg, sg, ap, code, resize=(9, 11))


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_resize_exports():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert declared == set(_ffi.EXPORTS)
    for parent in PARENTS:
        name = parent + "_resize"
        assert name in declared and hasattr(_ffi.lib(), name)
        proto = [a.strip() for a in re.search(rf"^SL_API int {name}\((.*?)\);", hdr, flags=re.M | re.S).group(1).split(",")]
        old = [a.strip() for a in re.search(rf"^SL_API int {parent}\((.*?)\);", hdr, flags=re.M | re.S).group(1).split(",")]
        assert proto == old[:9] + ["int max_wh", "int max_ww"] + old[9:] and old[8] == "int d_mask"
        pa, na = _ffi._SIGNATURES[parent][1], _ffi._SIGNATURES[name][1]
        assert len(na) == len(proto) and na == pa[:9] + [C.c_int, C.c_int] + pa[9:]
    assert _ffi.lib().sl_version() == 600 == _ffi.EXPECTED_VERSION           # added exports do not bump the version


def _v(oh, ow, d_mask, mh, mw, rgb=RGB, out=OUT, win=WIN, ms=D6, h=H, w=W, hed=False):
    route = (ms, D2 if ms else None, ms, D2 if ms else None, AB if ms else None, 0, None, None)
    if hed:
        return _ffi.lib().sl_normalize_hed_view_resize(rgb, out, N, h, w, oh, ow, win, d_mask, mh, mw, *route, SG, SG, AP, 0, None)
    return _ffi.lib().sl_normalize_view_resize(rgb, out, N, h, w, oh, ow, win, d_mask, mh, mw, *route, None)


@pytest.mark.parametrize("oh,ow,d_mask,mh,mw", [(8, 8, 7, 0, 8), (8, 8, 7, 8, 0), (8, 8, 7, -1, 8), (8, 8, 7, 65, 8), (8, 8, 7, 8, 49),
                                                (8, 8, 7, 2 ** 31 - 1, 8), (0, 8, 7, 8, 8), (8, 0, 7, 8, 8), (-1, -1, 0, 8, 8),
                                                (8, 8, 8, 8, 8), (8, 8, -1, 8, 8), (2 ** 31 - 1, 8, 0, 64, 48), (8, 2 ** 25, 6, 64, 48)])
def test_the_exports_refuse_bad_bounds_sizes_and_masks(oh, ow, d_mask, mh, mw):
    for hed in (False, True):
        assert _v(oh, ow, d_mask, mh, mw, hed=hed) == BADARG and _v(oh, ow, d_mask, mh, mw, ms=None, hed=hed) == BADARG


def test_the_exports_refuse_null_pointers_and_a_window_above_2_to_22_pixels():
    for hed in (False, True):
        assert _v(8, 8, 7, 8, 8, rgb=None, hed=hed) == BADARG and _v(8, 8, 7, 8, 8, out=None, hed=hed) == BADARG
        assert _v(8, 8, 7, 8, 8, win=None, hed=hed) == BADARG
        assert _v(224, 224, 7, 2049, 2048, h=4096, w=4096, hed=hed) == BADARG       # 2^22 + 2048 pixels
        assert _v(224, 224, 7, 4096, 1025, h=4096, w=4096, hed=hed) == BADARG
    lib = _ffi.lib()
    route = (None,) * 5 + (0, None, None)
    assert lib.sl_normalize_hed_view_resize(RGB, OUT, N, H, W, 8, 8, WIN, 7, 8, 8, *route, None, SG, AP, 0, None) == BADARG
    assert lib.sl_normalize_hed_view_resize(RGB, OUT, N, H, W, 8, 8, WIN, 7, 8, 8, *route, SG, SG, None, 0, None) == BADARG
    assert lib.sl_normalize_hed_view_resize(RGB, OUT, N, H, W, 8, 8, WIN, 7, 8, 8, *route, SG, SG, AP, 1, None) == BADARG
    assert lib.sl_normalize_view_resize(RGB, OUT, N, H, W, 8, 8, WIN, 7, 8, 8, D6, None, D6, D2, AB, 0, None, None, None) == BADARG


def test_c_abi_argument_checks_of_the_resize_entry_points_under_asan():
    """`make asan-resize`: tests/abi_argcheck_resize.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the two entry points.  Nothing is launched: no GPU needed.  (Builds the sanitizer library
    if nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-resize", "-j8"], capture_output=True, text=True,
                       timeout=1200)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

"""-m gpu: the Lab family in the one-pass loader (sl_reinhard_view, sl_luminosity_view, sl_slab_view; engine.reinhard_view /
luminosity_view / slab_view; view= on ReinhardStainNormalizer.transform_batch, LuminosityStandardizer.standardize_batch,
SlideNormalizer(reinhard, "pooled").transform_shard and slide_luminosity_standardize).

The definition under test is sl_normalize_view's "the same bits, elsewhere" with full[t] the image an EXISTING entry point writes for
the whole tile -- engine.reinhard_transform, engine.luminosity_standardize, or engine.slab_map behind the slab_* chain on one rank -- so
every comparison is exact: that result sliced, flipped and turned with torch (_ref of tests/test_gpu_view.py), through fmt.convert for a
tensor format.  Every call writes into a buffer with sentinel elements before and after the output (_guarded), also at an odd element
offset.  The kernel takes a RUN of 4 patches of 64 x 64 output pixels per workgroup (lab_view_kernels.hpp: kLabViewRun)."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests import big_batch
from tests.big_batch import guarded
from tests.test_gpu_jitter import SENTINEL, _dev_tiles, _formats, _same_bits
from tests.test_gpu_view import _ref, _windows

pytestmark = pytest.mark.gpu

_CACHE = {}


def _normalizer():
    if "nz" not in _CACHE:
        nz = stainlib_amd.ReinhardStainNormalizer()
        nz.fit(so.synth_tile(80, 80, 1001, so.M_TRUE_TGT))
        _CACHE["nz"] = nz
    return _CACHE["nz"]


def _tiles(n, h, w, seed0=40):
    """n synthetic H&E tiles with distinct statistics (each from its own seed, tile i darkened a little more): a wrong tile index
    cannot pass.  CPU tensor, cached."""
    key = (n, h, w, seed0)
    if key not in _CACHE:
        t = np.stack([(so.synth_tile(h, w, seed0 + 7 * i + h).astype(np.float64) * (1.0 - 0.06 * i)).astype(np.uint8) for i in range(n)])
        _CACHE[key] = torch.from_numpy(t)
    return _CACHE[key]


def _guarded(call, n, oh, ow, fmt, out_off=0):
    """call(out) -> whatever it returns, `out` a view 16 bytes + out_off elements into a buffer of SENTINEL with 16 more bytes behind
    it; everything outside the body must still hold SENTINEL afterwards.  -> (out on the CPU, the call's result)"""
    g = guarded(n * oh * ow * 3, fmt.dtype if fmt is not None else torch.uint8, out_off)       # (shared: tests/big_batch.py)
    assert SENTINEL == big_batch.SENTINEL
    out = g.image(n, oh, ow, fmt)
    res = call(out)
    assert res[0] is out
    g.check(f"{n} x {oh} x {ow} fmt={fmt} out+{out_off}")
    return out.cpu(), res


def _full(kind, dev, fmt=None, **kw):
    """(the existing entry point's full-tile result on the CPU, its stats / p on the CPU) -- computed once per case, shared"""
    from stainlib_amd import engine
    if kind == "reinhard":
        tm, ts = _normalizer()._targets()
        u8, extra = engine.reinhard_transform(dev, tm, ts, **kw)
    else:
        u8, extra = engine.luminosity_standardize(dev, **kw)
    return (u8 if fmt is None else fmt.convert(u8)).cpu(), extra.cpu()


def _view(kind, dev, win, size, d_mask, fmt=None, out_off=0, **kw):
    """the view call into a guarded buffer -> (out on the CPU, stats / p on the CPU)"""
    from stainlib_amd import engine
    n, h, w, _ = dev.shape
    oh, ow = (h, w) if size is None else size
    if kind == "reinhard":
        tm, ts = _normalizer()._targets()
        got, res = _guarded(lambda out: engine.reinhard_view(dev, win, size, tm, ts, d_mask, fmt=fmt, out=out, **kw), n, oh, ow, fmt, out_off)
    else:
        got, res = _guarded(lambda out: engine.luminosity_view(dev, win, size, d_mask=d_mask, fmt=fmt, out=out, **kw), n, oh, ow, fmt, out_off)
    return got, res[1].cpu()


def _same_f64(a, b):
    """equal bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


VARIANTS = [("reinhard", dict(mask_background=False)), ("reinhard", dict(mask_background=True)), ("luminosity", {})]


def _check(dev, win, size, d_mask, variants, fmts, out_offs=(0,), label=""):
    n, h, w, _ = dev.shape
    oh, ow = (h, w) if size is None else size
    for kind, kw in variants:
        u8, extra = _full(kind, dev, **kw)
        for fmt in fmts:
            want = _ref(u8 if fmt is None else fmt.convert(u8.cuda()).cpu(), win, oh, ow, d_mask)
            for off in out_offs:
                got, extra_v = _view(kind, dev, win, size, d_mask, fmt=fmt, out_off=off, **kw)
                assert _same_bits(got, want), f"{label} {kind} {kw} {n}x{h}x{w} -> {oh}x{ow} mask {d_mask} {fmt} out+{off}"
                assert _same_f64(extra_v, extra), f"{label} {kind} {kw}: the returned statistics"          # (case 8)


ALL_FMTS = [None] + _formats()


# ---- 1. outputs smaller than a patch from a tiny tile: every map, every output form ---------------------------------------------------
@pytest.mark.parametrize("size,d_mask", [((5, 7), 6), ((5, 5), 7)])
def test_tiny_tiles_every_map_and_format(size, d_mask):
    n, h, w = 8, 9, 11
    dev = _dev_tiles(_tiles(n, h, w), 0)
    _check(dev, _windows(n, h, w, *size, d_mask), size, d_mask, VARIANTS, ALL_FMTS, out_offs=(0, 1))


# ---- 2. ragged patches and rows: 2 x 2 ragged patches, all eight codes in one batch, windows at the corners and odd / even x0 -----------
@pytest.mark.parametrize("off", [0, 1])
def test_ragged_patches_all_codes_in_one_batch(off):
    n, h, w, size = 8, 67, 93, (65, 66)                           # 67 * 93 pixels: not a multiple of 4
    dev = _dev_tiles(_tiles(n, h, w), off)
    win = _windows(n, h, w, *size, 7)
    assert sorted(win[:, 2].tolist()) == list(range(8))
    _check(dev, win, size, 7, VARIANTS[1:], [None, _formats()[2], _formats()[1]], out_offs=(off,), label=f"+{off}")


# ---- 3. the patch run: 9 patches = two full runs of 4 and a run of 1, three tiles with distinct statistics -------------------------------
def test_more_patches_than_a_run():
    n, h, w, size = 3, 200, 136, (192, 130)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = np.array([(3, 2, 0), (8, 6, 6), (0, 5, 4)], dtype=np.int32)
    _check(dev, win, size, 6, VARIANTS[1:], [None, _formats()[2]])
    st = _full("reinhard", dev, mask_background=True)[1]
    assert len({tuple(r.tolist()) for r in st[:, 1:7]}) == n          # (distinct statistics: a wrong tile's tables cannot pass)


# ---- 4. the full tile, code 0: today's transform_batch(tensor_format=), bit for bit -----------------------------------------------------
def test_full_tile_view_is_the_tensor_of_today():
    n, h, w = 3, 67, 93
    dev = _dev_tiles(_tiles(n, h, w), 0)
    nz = _normalizer()
    view = stainlib_amd.TileView(None, flip=False, rot90=False)
    for fmt in (_formats()[0], _formats()[3], _formats()[4]):
        for mask in (False, True):
            want, st = nz.transform_batch(dev, mask_background=mask, tensor_format=fmt)
            x, st_v, win = nz.transform_batch(dev, mask_background=mask, tensor_format=fmt, view=view)
            assert np.array_equal(win, np.zeros((n, 3), dtype=np.int32)) and tuple(x.shape) == (n, 3, h, w)
            assert _same_bits(x.cpu(), want.cpu()) and _same_f64(st_v.cpu(), st.cpu()), f"{fmt} mask={mask}"
            assert x.is_contiguous(memory_format=torch.channels_last if fmt.channels_last else torch.contiguous_format)
        want, p = stainlib_amd.LuminosityStandardizer.standardize_batch(dev, tensor_format=fmt)
        x, p_v, _ = stainlib_amd.LuminosityStandardizer.standardize_batch(dev, tensor_format=fmt, view=view)
        assert _same_bits(x.cpu(), want.cpu()) and _same_f64(p_v.cpu(), p.cpu())
    u8, _ = nz.transform_batch(dev)
    x, _, _ = nz.transform_batch(dev, view=view)
    assert x.dtype == torch.uint8 and torch.equal(x, u8)


# ---- 5. background and degenerate tiles under mask_background ----------------------------------------------------------------------------
def test_background_and_degenerate_tiles_are_the_existing_maps_bytes():
    h, w, size = 67, 93, (40, 50)
    tiles = np.stack([so.synth_tile(h, w, 3), so.structured_tile("white_bg", w, h, 5).transpose(1, 0, 2).copy(),
                      np.full((h, w, 3), 255, dtype=np.uint8)])
    dev = torch.from_numpy(tiles).cuda()
    win = np.array([(5, 7, 1), (20, 30, 4), (27, 43, 2)], dtype=np.int32)
    u8, st = _full("reinhard", dev, mask_background=True)
    assert int(st[2, 7]) == 0 and int(st[0, 7]) > 0                  # the all-white tile has no tissue pixel: reported, nothing raises
    for fmt in (None, _formats()[2]):
        got, st_v = _view("reinhard", dev, win, size, 7, fmt=fmt, mask_background=True)
        want = _ref(u8 if fmt is None else fmt.convert(u8.cuda()).cpu(), win, *size, 7)
        assert _same_bits(got, want) and _same_f64(st_v, st) and int(st_v[2, 7]) == 0
    x, st_b, win_b = _normalizer().transform_batch(dev, mask_background=True, view=stainlib_amd.TileView(size), windows=win)
    assert win_b is win and torch.equal(x.cpu(), _ref(u8, win, *size, 7)) and _same_f64(st_b.cpu(), st)


# ---- 6. pooled: the shard calls with a view against the same calls without one ----------------------------------------------------------
def test_pooled_reinhard_shard_view():
    from stainlib_amd.distributed import SlideNormalizer
    n, h, w, size = 5, 67, 93, (65, 66)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    view = stainlib_amd.TileView(size)
    sn = SlideNormalizer(_normalizer(), group=False, mode="pooled")
    for mask in (False, True):
        full, means, stds, status = sn.transform_shard(dev, mask_background=mask)
        for fmt in (None, _formats()[2], _formats()[5]):
            np.random.seed(11)
            want_win = view.draw(n, h, w)
            after = np.random.uniform()
            np.random.seed(11)
            got, res = _guarded(lambda out: sn.transform_shard(dev, out=out, mask_background=mask, tensor_format=fmt, view=view),
                                n, *size, fmt, out_off=1 if fmt is not None else 0)
            assert len(res) == 5 and np.array_equal(res[4], want_win) and np.random.uniform() == after
            want = _ref((full if fmt is None else fmt.convert(full)).cpu(), want_win, *size, 7)
            assert _same_bits(got, want), f"mask={mask} {fmt}"
            assert _same_f64(res[1].cpu(), means.cpu()) and _same_f64(res[2].cpu(), stds.cpu()) and torch.equal(res[3], status)
    dwin = torch.from_numpy(want_win).cuda()                            # device windows are taken as they are
    x, _, _, _, win2 = sn.transform_shard(dev, mask_background=True, view=view, windows=dwin)
    assert win2 is dwin and torch.equal(x.cpu(), _ref(full.cpu(), want_win, *size, 7))


def test_pooled_luminosity_view():
    from stainlib_amd.distributed import slide_luminosity_standardize
    n, h, w, size = 5, 67, 93, (65, 66)
    dev = _dev_tiles(_tiles(n, h, w), 1)
    view = stainlib_amd.TileView(size)
    for pct in (95, 80):
        full, p = slide_luminosity_standardize(dev, percentile=pct, group=False)
        for fmt in (None, _formats()[2]):
            np.random.seed(12)
            got, res = _guarded(lambda out: slide_luminosity_standardize(dev, percentile=pct, group=False, out=out, tensor_format=fmt,
                                                                         view=view), n, *size, fmt)
            np.random.seed(12)
            win = view.draw(n, h, w)
            assert len(res) == 3 and res[1] == p and np.array_equal(res[2], win)
            assert _same_bits(got, _ref((full if fmt is None else fmt.convert(full)).cpu(), win, *size, 7)), f"{pct} {fmt}"


def test_an_all_white_slide_under_mask_background_gives_the_view_of_the_source_bytes():
    from stainlib_amd import _ffi
    from stainlib_amd.distributed import SlideNormalizer
    from stainlib_amd.utils.excepts import TissueMaskException
    n, h, w, size = 3, 67, 93, (65, 66)
    win = _windows(n, h, w, *size, 7)
    sn = SlideNormalizer(_normalizer(), group=False, mode="pooled")
    white = np.full((n, h, w, 3), 255, dtype=np.uint8)
    nearly = white.copy()
    nearly[:, ::7, ::5] = (250, 252, 249)                             # (still background only, but a view of it is not constant)
    for dev, fmt in ((torch.from_numpy(white).cuda(), None), (torch.from_numpy(nearly).cuda(), None),
                     (torch.from_numpy(nearly).cuda(), _formats()[1])):
        def call(out):
            with pytest.raises(TissueMaskException):
                sn.transform_shard(dev, out=out, mask_background=True, tensor_format=fmt, view=stainlib_amd.TileView(size), windows=win)
            return (out,)
        got, _ = _guarded(call, n, *size, fmt)
        assert sn.last_tissue == 0 and sn.last_pixels == n * h * w      # (the status was not SL_TILE_OK: _ffi.TILE_EMPTY_MASK)
        assert _same_bits(got, _ref((dev if fmt is None else fmt.convert(dev)).cpu(), win, *size, 7)), f"{fmt}"
    assert _ffi.TILE_EMPTY_MASK != 0


# ---- 7. device windows are clamped and masked by the kernel ------------------------------------------------------------------------------
def test_device_windows_out_of_range_equal_the_clamped_window():
    n, h, w, size = 8, 40, 72, (17, 30)                       # (fits transposed too: 30 <= 40, 17 <= 72)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    wild = np.array([(-1, -1, 0), (10 ** 9, 10 ** 9, 2), (-2 ** 31, 2 ** 31 - 1, 4), (2 ** 31 - 1, -2 ** 31, 6), (24, 43, 0x7ffffff8 | 2),
                     (23, 42, -1), (5, 100, 1), (100, 5, 3 | 8)], dtype=np.int64).astype(np.int32)
    dwin = torch.from_numpy(wild).cuda()
    fulls = {i: _full(kind, dev, **kw)[0] for i, (kind, kw) in enumerate(VARIANTS[1:])}
    for d_mask in (7, 6, 4, 0):
        for i, (kind, kw) in enumerate(VARIANTS[1:]):
            for fmt in (None, _formats()[2]):
                got, _ = _view(kind, dev, dwin, size, d_mask, fmt=fmt, **kw)
                want = _ref(fulls[i] if fmt is None else fmt.convert(fulls[i].cuda()).cpu(), wild, *size, d_mask)
                assert _same_bits(got, want), f"mask {d_mask} {kind} {fmt}"

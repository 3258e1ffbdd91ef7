"""-m gpu: hue / saturation / brightness augmentation (sl_hsb_augment, sl_normalize_hsb_view, engine.hsb_augment / normalize_hsb_view,
HsbColorAugmenter, hsb= on the batch methods).

The definition is in integers on bytes (stainlib_amd/augmentation/hsb.py: hsb_reference), so every comparison is exact: the full-tile
sweep against hsb_reference; a view against the EXISTING view pass (TensorFormat.convert(view=) / engine.view_pass) of hsb_reference's
image; the hsb= stage against its own two-call chain.  Outputs of the full-tile sweep are written into a buffer with sentinel elements
before and after the output, checked after the call."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd.augmentation.hsb import Q, hsb_codes, hsb_reference
from tests.big_batch import K, SHAPES, assert_periodic, base_tiles, guarded, need_memory, periodic_batch, periodic_rows, release
from tests.test_gpu_jitter import MEAN, STD, _dev_tiles, _same_bits
from tests.test_gpu_view_affine import FORMATS

pytestmark = pytest.mark.gpu

N = 6
# 96 x 80: P % 4 == 0 (the aligned sweep and the wide tensor stores); 37 x 53: P = 1961, ragged last chunk and group, unaligned tiles;
# 1 x 1: three bytes per tile (the byte path of the loads)
TILE_SHAPES = [(96, 80), (37, 53), (1, 1)]
_CACHE = {}


def _edge_colours():
    """greys, black, white, the primaries and secondaries, M = 1, and every channel-tie class"""
    c = [(v, v, v) for v in (0, 1, 2, 127, 128, 254, 255)]
    c += [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1),
          (0, 1, 1)]
    for hi, lo in ((200, 50), (50, 200), (1, 0), (255, 254), (255, 0)):
        c += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi)]
    return np.array(c, dtype=np.uint8)


def _tiles(n, h, w):
    """n tiles of random colours; tile 1 is the "edge" tile: the edge colours over and over (a 1 x 1 tile: black's neighbour, M = 1)"""
    key = ("tiles", n, h, w)
    if key not in _CACHE:
        t = np.random.RandomState(100 + h).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        e = _edge_colours()
        t[1] = e[(np.arange(h * w) + (1 if h * w == 1 else 0)) % len(e)].reshape(h, w, 3)
        _CACHE[key] = t
    return _CACHE[key]


def _code_groups():
    """18 code triples, three calls of six tiles: zero, the extremes, one hue on every sextant boundary, drawn Light and Strong values"""
    if "codes" not in _CACHE:
        rows = [(0, 0, 0), (6 * Q - 1, Q, Q), (Q, -Q, -Q), (0, 9000, -4000), (2 * Q, -12000, 3000), (3 * Q, 30000, 0), (4 * Q, 0, 20000),
                (5 * Q, -1, 1)]
        np.random.seed(1234)
        light, strong = stainlib_amd.HsbLightColorAugmenter(), stainlib_amd.HsbStrongColorAugmenter()
        wide = stainlib_amd.HsbColorAugmenter((-1, 1), (-1, 1), (-1, 1))
        rows += hsb_codes(light.randomize_batch(3)).tolist() + hsb_codes(strong.randomize_batch(3)).tolist()
        rows += hsb_codes(wide.randomize_batch(4)).tolist()
        codes = np.array(rows, dtype=np.int32)
        assert codes.shape == (18, 3)
        _CACHE["codes"] = codes.reshape(3, N, 3)
    return _CACHE["codes"]


def _want(h, w, g):
    """hsb_reference of the tiles of a shape under code group g, computed once"""
    key = ("want", h, w, g)
    if key not in _CACHE:
        _CACHE[key] = hsb_reference(_tiles(N, h, w), _code_groups()[g])
    return _CACHE[key]


def _augment(dev, codes, fmt, out_off=0):
    """engine.hsb_augment into a guarded buffer -> CPU tensor"""
    from stainlib_amd import engine
    n, h, w, _ = dev.shape
    g = guarded(n * h * w * 3, fmt.dtype if fmt is not None else torch.uint8, out_off=out_off)
    out = g.image(n, h, w, fmt)
    res = engine.hsb_augment(dev, codes, fmt=fmt, out=out)
    g.check(f"hsb_augment {h}x{w} {fmt}")
    assert res.data_ptr() == out.data_ptr()
    return res.cpu()


# ---- 1. the full-tile sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "u8" if f is None else str(f.dtype).split(".")[1] + ("_nhwc" if f.channels_last else ""))
@pytest.mark.parametrize("h,w", TILE_SHAPES)
def test_hsb_augment_is_the_definition_bit_for_bit(h, w, fmt):
    tiles = torch.from_numpy(_tiles(N, h, w))
    for off in ((0, 1) if (h, w) == (96, 80) else (0,)):         # 96 x 80 behind an unaligned pointer too: the other sweep
        dev = _dev_tiles(tiles, off)
        for g in range(3):
            want8 = torch.from_numpy(_want(h, w, g))
            got = _augment(dev, _code_groups()[g], fmt, out_off=off if fmt is None else 0)
            if fmt is None:
                assert got.dtype == torch.uint8 and torch.equal(got, want8), (h, w, off, g)
            else:
                assert _same_bits(got, fmt.convert(want8.cuda()).cpu()), (h, w, off, g, fmt)
    assert not np.array_equal(_want(h, w, 1), _tiles(N, h, w))    # (the map does something)
    assert np.array_equal(_want(h, w, 0)[0], _tiles(N, h, w)[0])  # zero codes: the identity


def test_codes_out_of_range_are_reduced_by_the_kernel():
    from stainlib_amd import engine
    h, w = 37, 53
    tiles = _tiles(N, h, w)
    wild = np.array([[-1, 40000, -40000], [6 * Q, Q + 1, -Q - 1], [-6 * Q - 5, 2 ** 31 - 1, -2 ** 31], [2 ** 31 - 1, 5, -5], [-2 ** 31, 0, 0],
                     [13 * Q + 7, -Q - 100, Q + 100]], dtype=np.int32)
    red = np.array([[6 * Q - 1, Q, -Q], [0, Q, -Q], [6 * Q - 5, Q, -Q], [(2 ** 31 - 1) % (6 * Q), 5, -5], [(-2 ** 31) % (6 * Q), 0, 0],
                    [Q + 7, -Q, Q]], dtype=np.int32)
    want = hsb_reference(tiles, red)
    dev = torch.from_numpy(tiles).cuda()
    for codes in (wild, torch.from_numpy(wild).cuda()):           # from the host and as a device tensor, never read back
        assert np.array_equal(engine.hsb_augment(dev, codes).cpu().numpy(), want)
    win = np.zeros((N, 3), dtype=np.int32)
    assert np.array_equal(engine.normalize_hsb_view(dev, win, None, 0, torch.from_numpy(wild).cuda()).cpu().numpy(), want)


def test_transform_of_one_patch_and_the_lower_bound_quirk():
    patch = _tiles(N, 37, 53)[0]
    aug = stainlib_amd.HsbLightColorAugmenter()
    out = aug.transform(patch)                                    # un-randomized: the lower bounds (-0.1, -0.1, 0)
    assert out.dtype == np.uint8 and np.array_equal(out, hsb_reference(patch, hsb_codes([-0.1, -0.1, 0.0])))
    np.random.seed(8)
    aug.randomize()
    assert np.array_equal(aug.transform(patch), hsb_reference(patch, hsb_codes(aug._sigmas)))


# ---- 2. the raw route of the view pass: HsbColorAugmenter.transform_batch(view=) ------------------------------------------------------------
NV, VH, VW = 8, 96, 80


def _view_setup():
    if "view" not in _CACHE:
        tiles = _tiles(NV, VH, VW)
        np.random.seed(77)
        sig = stainlib_amd.HsbColorAugmenter((-1, 1), (-1, 1), (-0.5, 0.5)).randomize_batch(NV)
        ref = hsb_reference(tiles, hsb_codes(sig))
        _CACHE["view"] = (torch.from_numpy(tiles).cuda(), sig, torch.from_numpy(ref).cuda())
    return _CACHE["view"]


def _fixed_windows(oh, ow, s=1):
    """all eight dihedral codes, corners that include the tile's last row and column"""
    win = np.empty((NV, 3), dtype=np.int32)
    for d in range(NV):
        wh, ww = (s * ow, s * oh) if d & 1 else (s * oh, s * ow)
        ymax, xmax = VH - wh, VW - ww
        win[d] = [(0, 0), (ymax, xmax), (ymax, 0), (0, xmax), (ymax // 2, xmax // 2 | 1), (1, 2), (ymax, xmax // 2), (ymax // 3, xmax)][d] + (d,)
        win[d, 1] = min(win[d, 1], xmax)
    return win


def _check_view(view, win):
    from stainlib_amd import engine
    dev, sig, ref = _view_setup()
    aug = stainlib_amd.HsbStrongColorAugmenter()
    oh, ow = view.out_size(VH, VW)
    for windows in (win, torch.from_numpy(win).cuda()):           # on the host (range-checked) and on the device (taken as they are)
        for fmt in FORMATS:
            got, codes, w_back = aug.transform_batch(dev, sig, view=view, windows=windows, tensor_format=fmt)
            assert np.array_equal(codes, hsb_codes(sig)) and w_back is windows
            if fmt is None:
                want, _ = engine.view_pass(ref, view, windows)
                assert tuple(got.shape) == (NV, oh, ow, 3) and torch.equal(got, want), (view, fmt)
            else:
                want, _ = fmt.convert(ref, view=view, windows=windows)
                assert tuple(got.shape) == (NV, 3, oh, ow) and _same_bits(got.cpu(), want.cpu()), (view, fmt)


@pytest.mark.parametrize("size", [(40, 56), (70, 70)])
def test_view_fixed_size_all_eight_codes_two_patches_per_axis(size):
    _check_view(stainlib_amd.TileView(size), _fixed_windows(*size))


@pytest.mark.parametrize("shrink,size", [(2, (40, 40)), (4, (20, 20))])
def test_view_box_shrink_acts_on_the_mapped_pixels(shrink, size):
    _check_view(stainlib_amd.TileView(size, shrink=shrink), _fixed_windows(*size, s=shrink))


def test_view_resizing_with_n_by_5_windows():
    view = stainlib_amd.TileView((40, 56), scale=(0.3, 1))
    np.random.seed(5)
    win = view.draw(NV, VH, VW)
    assert win.shape == (NV, 5) and len(set(map(tuple, win[:, 3:].tolist()))) > 1          # windows of their own sizes
    _check_view(view, win)


def test_transform_batch_draws_only_the_windows_and_full_tile_forms_agree():
    dev, sig, ref = _view_setup()
    aug = stainlib_amd.HsbStrongColorAugmenter()
    view = stainlib_amd.TileView(48)
    np.random.seed(21)
    x, codes, win = aug.transform_batch(dev, sig, view=view)
    after = np.random.uniform()
    np.random.seed(21)
    assert np.array_equal(win, view.draw(NV, VH, VW)) and np.random.uniform() == after
    # no view: (out, codes); the default sigmas are the augmenter's current ones for every tile
    out, codes = aug.transform_batch(dev, sig)
    assert torch.equal(out, ref) and np.array_equal(codes, hsb_codes(sig))
    out, codes = aug.transform_batch(dev)
    assert np.array_equal(codes, np.tile(hsb_codes([aug._sigmas]), (NV, 1))) and np.array_equal(out.cpu().numpy(), hsb_reference(_tiles(NV, VH, VW), codes))
    fmt = FORMATS[1]
    t, _ = aug.transform_batch(dev, sig, tensor_format=fmt)
    assert _same_bits(t.cpu(), fmt.convert(ref).cpu())


# ---- 3. hsb= on the batch methods: each against its own two-call chain -------------------------------------------------------------------------
def _class_batch():
    """five synthetic H&E tiles and an all-white one (no tissue: its fit fails, status != 0, and it takes the stage on its own bytes)"""
    t = np.stack([so.synth_tile(64, 64, 40 + 7 * i) for i in range(5)] + [np.full((64, 64, 3), 255, dtype=np.uint8)])
    t[5, 10:20, 10:20] = (250, 240, 245)                          # (bright, still no tissue; the HSB map moves these bytes)
    return torch.from_numpy(t).cuda()


def _f16():
    return stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD)


@pytest.mark.parametrize("method", ["macenko", "vahadane"])
def test_hsb_through_the_batch_methods_is_the_two_call_chain(method):
    from stainlib_amd import engine
    dev = _class_batch()
    n = dev.shape[0]
    nz = stainlib_amd.MacenkoNormalizer() if method == "macenko" else stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    aug = stainlib_amd.HsbStrongColorAugmenter()
    fmt = _f16()
    np.random.seed(9)
    ab = stainlib_amd.StainJitter().draw(n)
    for bg in (False, True):                                      # the jitter of tissue pixels, and of all pixels
        for view in (stainlib_amd.TileView(48), stainlib_amd.TileView(24, shrink=2), stainlib_amd.TileView((40, 33), scale=(0.4, 1)), None):
            for f in (fmt, None):
                kw = dict(view=view) if view is not None else {}
                np.random.seed(41)
                res = nz.augment_batch(dev, ab, augment_background=bg, hsb=aug, tensor_format=f, **kw)
                after = np.random.uniform()
                x, M, mc, st, draw = res[0], res[1], res[2], res[3], res[-1]
                win = res[4] if view is not None else None
                assert len(res) == (6 if view is not None else 5) and isinstance(draw, engine.HsbDraw)
                np.random.seed(41)
                sig = aug.randomize_batch(n)                      # the draws: HSB first, then the windows
                assert np.array_equal(draw.sigmas, sig) and np.array_equal(draw.codes, hsb_codes(sig))
                assert view is None or np.array_equal(win, view.draw(n, 64, 64))
                assert np.random.uniform() == after
                assert int(st[5]) != 0 and st[:5].cpu().tolist() == [0] * 5
                u8, M2, mc2, st2 = nz.augment_batch(dev, ab, augment_background=bg)
                assert torch.equal(st, st2) and torch.equal(M[st == 0], M2[st2 == 0]) and torch.equal(mc[st == 0], mc2[st2 == 0])
                assert torch.equal(u8[5], dev[5])                 # the failed fit: its own bytes ...
                want = aug.transform_batch(u8, sig, tensor_format=f, **(dict(view=view, windows=win) if view is not None else {}))[0]
                assert _same_bits(x.cpu(), want.cpu()), (method, bg, view, f)
                if view is None and f is None:
                    assert not torch.equal(x[5], dev[5])          # ... with the HSB map applied
    # transform_batch: the apply route, given sigmas and windows replayed from a first call
    view = stainlib_amd.TileView(48)
    x, _, _, st, win, draw = nz.transform_batch(dev, hsb=aug, view=view, tensor_format=fmt)
    x2, _, _, _, win2, draw2 = nz.transform_batch(dev, hsb=aug, hsb_sigmas=draw.sigmas, view=view, windows=win, tensor_format=fmt)
    assert win2 is win and np.array_equal(draw2.codes, draw.codes) and _same_bits(x.cpu(), x2.cpu())
    u8 = nz.transform_batch(dev)[0]
    want = aug.transform_batch(u8, draw.sigmas, view=view, windows=win, tensor_format=fmt)[0]
    assert _same_bits(x.cpu(), want.cpu()), method
    res = nz.transform_batch(dev, hsb=aug, hsb_sigmas=draw.sigmas)                     # without a view: the full tile, one element fewer
    assert len(res) == 5 and torch.equal(res[0], aug.transform_batch(u8, draw.sigmas)[0])
    res = nz.transform_batch(dev, hsb=aug, hsb_sigmas=draw.sigmas, tensor_format=fmt)  # a format alone
    assert len(res) == 5 and _same_bits(res[0].cpu(), aug.transform_batch(u8, draw.sigmas, tensor_format=fmt)[0].cpu())
    res = nz.transform_batch(dev, hsb=aug, hsb_sigmas=draw.sigmas, view=view, windows=win)      # a view alone
    assert len(res) == 6 and res[0].dtype == torch.uint8
    assert torch.equal(res[0], aug.transform_batch(u8, draw.sigmas, view=view, windows=win)[0])
    # StainAugmentor: alpha_beta, then the HSB draws, then the windows
    sa = stainlib_amd.StainAugmentor(method, sigma1=0.15, sigma2=0.1)
    np.random.seed(43)
    x, _, _, _, win, draw = sa.augment_batch(dev, hsb=aug, view=view)
    after = np.random.uniform()
    np.random.seed(43)
    ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
    sig2 = aug.randomize_batch(n)
    assert np.array_equal(win, view.draw(n, 64, 64)) and np.random.uniform() == after and np.array_equal(draw.sigmas, sig2)
    s8 = sa.augment_batch(dev, ab2)[0]
    want = aug.transform_batch(s8, sig2, view=view, windows=win)[0]
    assert torch.equal(x, want), method
    # ... with a format and a view, a format alone, neither
    for f, v in ((fmt, view), (fmt, None), (None, None)):
        kw = dict(view=v, windows=win) if v is not None else {}
        res = sa.augment_batch(dev, ab2, hsb=aug, hsb_sigmas=sig2, tensor_format=f, **kw)
        assert len(res) == (6 if v is not None else 5) and np.array_equal(res[-1].codes, hsb_codes(sig2))
        want = aug.transform_batch(s8, sig2, tensor_format=f, **kw)[0]
        assert _same_bits(res[0].cpu(), want.cpu()), (method, f, v)


# ---- 4. a batch whose byte offsets pass 2^31 and 2^32 ---------------------------------------------------------------------------------------
def test_hsb_augment_big_batch():
    """the K-periodic batch of tests/big_batch.py (odd tile size: every other tile starts at an odd byte): tile i + K must be tile i bit
    for bit, the first K tiles the definition's"""
    from stainlib_amd import engine
    h, w, n = SHAPES["odd"]
    B = n * h * w * 3
    assert B > 1 << 32
    need_memory(2 * B + (1 << 28))
    base_np = base_tiles(h, w)
    dev = periodic_batch(torch.from_numpy(base_np).cuda(), n)
    codes4 = np.array([(Q // 3, 9000, -4000), (6 * Q - 1, Q, Q), (3 * Q + 5, -20000, 12000), (Q, -Q, 100)], dtype=np.int32)
    codes = periodic_rows(torch.from_numpy(codes4).cuda(), n)
    g = guarded(B, torch.uint8, margin=4096)
    out = engine.hsb_augment(dev, codes, out=g.image(n, h, w))
    g.check("hsb_augment big batch")
    assert_periodic(out, label="hsb_augment")
    assert np.array_equal(out[:K].cpu().numpy(), hsb_reference(base_np, codes4))
    assert torch.equal(out[n - K:], out[:K])
    del out, dev, g
    release()

"""-m gpu: crop / flip / rot90 fused into the apply pass (sl_normalize_view, engine.normalize_view, TileView, view= on the batch methods).

The definition under test (include/stainlib_hip.h, sl_normalize_view) is "the same bits, elsewhere": per tile
    view[t] = rot90(flip_w_if(d & 4, full[t][y0:y0+wh, x0:x0+ww]), d & 3)
with full[t] the result of an EXISTING entry point (normalize_jitter, normalize_apply / normalize_apply_tensor, or the tiles themselves),
so every comparison is exact: the existing entry point's full-tile result, sliced, flipped and turned with torch.  Every call of _view
writes into a buffer with sentinel elements before and after the output, checked after the call.  Tiles and per-tile-distinct statistics:
the recipe of tests/test_gpu_jitter.py.  The kernel's patch is B x B output pixels (view_kernels.hpp: kViewB)."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.gpu_util import to_dev
from tests.test_gpu_jitter import (M_TGT, M_TGT_NEG, MAXC_TGT, MEAN, SENTINEL, STD, _dev_tiles, _formats, _same_bits, _stats, _tiles)

pytestmark = pytest.mark.gpu

B = 64
# which pass `full` is: the source bytes; normalize_apply (a target without / with a negative entry: the fast / the general cast);
# normalize_jitter on tissue / on every pixel, with a target / under the tile's own matrix
ROUTES = ["raw", "apply", "apply_neg", "tissue", "tissue_own", "all", "all_own"]


def _full(dev, route, M, mc, ab, fmt=None):
    """(the existing entry point's full-tile result on the CPU: (n,h,w,3) uint8 or (n,3,h,w) in fmt; the view call's statistics)"""
    from stainlib_amd import engine
    if route == "raw":
        return (dev if fmt is None else fmt.convert(dev)).cpu(), {}
    if route.startswith("apply"):
        Mt = M_TGT_NEG if route == "apply_neg" else M_TGT
        kw = dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=MAXC_TGT)
        full = engine.normalize_apply(dev, M, mc, Mt, MAXC_TGT) if fmt is None else engine.normalize_apply_tensor(dev, M, mc, Mt, MAXC_TGT, fmt)
        return full.cpu(), kw
    bg = route.startswith("all")
    Mt, mct = (None, None) if route.endswith("_own") else (M_TGT, MAXC_TGT)
    kw = dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=bg)
    return engine.normalize_jitter(dev, M, mc, Mt, mct, ab, augment_background=bg, fmt=fmt).cpu(), kw


def _ref(full, win, oh, ow, d_mask):
    """the definition, with torch, on the full-tile result: clamp, slice, flip along the width, then rot90"""
    chw = full.dtype != torch.uint8
    h, w = (full.shape[2], full.shape[3]) if chw else (full.shape[1], full.shape[2])
    outs = []
    for t, (y0, x0, d) in enumerate(np.asarray(win).tolist()):
        d &= d_mask
        k = d & 3
        wh, ww = (ow, oh) if k & 1 else (oh, ow)
        y0, x0 = min(max(y0, 0), h - wh), min(max(x0, 0), w - ww)
        v = (full[t].permute(1, 2, 0) if chw else full[t])[y0:y0 + wh, x0:x0 + ww]
        if d & 4:
            v = torch.flip(v, dims=(1,))
        v = torch.rot90(v, k, dims=(0, 1))
        assert tuple(v.shape) == (oh, ow, 3)
        outs.append(v.permute(2, 0, 1) if chw else v)
    return torch.stack(outs).contiguous()


def _view(dev, win, size, d_mask, fmt=None, out_off=0, **kw):
    """engine.normalize_view into a guarded buffer -> CPU tensor: the output sits 16 bytes + out_off elements into a buffer of SENTINEL
    with 16 more bytes behind it; everything outside the body must still hold SENTINEL afterwards (tests/test_gpu_jitter.py: _jit)."""
    from stainlib_amd import engine
    n, h, w, _ = dev.shape
    oh, ow = (h, w) if size is None else size
    dtype = fmt.dtype if fmt is not None else torch.uint8
    esize = torch.empty((), dtype=dtype).element_size()
    start, numel = 16 // esize + out_off, n * oh * ow * 3
    buf = torch.full((start + numel + 16 // esize,), SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    body = buf[start:start + numel]
    if fmt is None:
        out = body.view(n, oh, ow, 3)
    elif fmt.channels_last:
        out = body.view(n, oh, ow, 3).permute(0, 3, 1, 2)
    else:
        out = body.view(n, 3, oh, ow)
    res = engine.normalize_view(dev, win, size, d_mask, fmt=fmt, out=out, **kw)
    assert res is out
    torch.cuda.synchronize()
    got = buf.cpu()
    outside = torch.cat([got[:start], got[start + numel:]])
    assert bool((outside == SENTINEL).all()), f"{tuple(dev.shape)} -> {size} fmt={fmt} out+{out_off}: written outside the output"
    return out.cpu()


def _check(dev, win, size, d_mask, routes, fmts, regime="he", out_offs=(0,), label=""):
    n, h, w, _ = dev.shape
    oh, ow = (h, w) if size is None else size
    M, mc, ab = _stats(n, regime)
    for route in routes:
        for fmt in fmts:
            full, kw = _full(dev, route, M, mc, ab, fmt)
            want = _ref(full, win, oh, ow, d_mask)
            for off in out_offs:
                got = _view(dev, win, size, d_mask, fmt=fmt, out_off=off, **kw)
                assert _same_bits(got, want), f"{label} {n}x{h}x{w} -> {oh}x{ow} mask {d_mask} {route} {regime} {fmt} out+{off}"


def _windows(n, h, w, oh, ow, d_mask):
    """n distinct in-range windows cycling through the codes d_mask allows: the four corners of the code's range first, then corners
    in between with odd and even x0 (the row start 3 (y w + x0) takes every residue mod 4)."""
    codes = [c for c in range(8) if c & ~d_mask == 0]
    win = []
    for t in range(n):
        d = codes[t % len(codes)]
        wh, ww = (ow, oh) if d & 1 else (oh, ow)
        ymax, xmax = h - wh, w - ww
        win.append(([(0, 0), (0, xmax), (ymax, 0), (ymax, xmax)][t] if t < 4 else ((2 * t + 1) % (ymax + 1), (t - 1) % (xmax + 1))) + (d,))
    assert len(set(win)) == n
    return np.array(win, dtype=np.int32)


ALL_FMTS = [None] + _formats()


# ---- 1. outputs smaller than a patch from a tiny tile: every route, every output form --------------------------------------------------
@pytest.mark.parametrize("size,d_mask", [((5, 7), 6), ((5, 5), 7)])
def test_tiny_tiles_every_route_and_format(size, d_mask):
    n, h, w = 8, 9, 11
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = _windows(n, h, w, *size, d_mask)
    _check(dev, win, size, d_mask, ROUTES, ALL_FMTS, out_offs=(0, 1))
    _check(dev, win, size, d_mask, ["apply", "tissue", "all_own"], [None, _formats()[2]], regime="neg")


# ---- 2. ragged last patches in both directions, more than one patch each way, transposed edges, all eight codes in one batch ------------
@pytest.mark.parametrize("off", [0, 1])
def test_ragged_patches_all_codes_in_one_batch(off):
    """(2B+3) x (B-1) out of a square tile just large enough for the transposed window; the input at an aligned address and one byte
    past it; windows at all four corners and at x0 of all four residues mod 4; per-tile-distinct statistics."""
    n, h, oh, ow = 8, 2 * B + 3, 2 * B + 3, B - 1
    dev = _dev_tiles(_tiles(n, h, h), off)
    assert dev.data_ptr() % 4 == off
    win = np.array([(0, 0, 0), (68, 0, 1), (0, 1, 2), (67, 0, 3), (0, 2, 4), (3, 0, 5), (0, 3, 6), (0, 0, 7)], dtype=np.int32)
    assert sorted(win[:, 2].tolist()) == list(range(8)) and {int(x) % 4 for x in win[::2, 1]} == {0, 1, 2, 3}
    _check(dev, win, (oh, ow), 7, ["tissue"], ALL_FMTS, label=f"+{off}")
    _check(dev, win, (oh, ow), 7, ["apply", "all_own", "raw"], [None, _formats()[3]], label=f"+{off}")
    # the other corners of every code's range, and the other orientation of the output
    win2 = np.array([(0, 68, 0), (0, 0, 1), (0, 67, 2), (1, 0, 3), (0, 5, 4), (66, 0, 5), (0, 66, 6), (68, 0, 7)], dtype=np.int32)
    _check(dev, win2, (oh, ow), 7, ["tissue_own"], [None, _formats()[0]], label=f"+{off} other corners")
    win3 = win2[:, [1, 0, 2]].copy()
    _check(dev, win3, (ow, oh), 7, ["all"], [None, _formats()[5]], label=f"+{off} wide output")


# ---- 3. device windows are clamped and masked by the kernel ---------------------------------------------------------------------------
def test_device_windows_out_of_range_equal_the_clamped_window():
    """corners far outside the tile, codes with bits outside d_mask and above bit 2: the result is the clamped, masked window's"""
    n, h, w, size = 8, 40, 72, (17, 30)                       # (fits transposed too: 30 <= 40, 17 <= 72)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    wild = np.array([(-1, -1, 0), (10 ** 9, 10 ** 9, 2), (-2 ** 31, 2 ** 31 - 1, 4), (2 ** 31 - 1, -2 ** 31, 6), (24, 43, 0x7ffffff8 | 2),
                     (23, 42, -1), (5, 100, 1), (100, 5, 3 | 8)], dtype=np.int64).astype(np.int32)
    dwin = torch.from_numpy(wild).cuda()
    M, mc, ab = _stats(n)
    for d_mask in (7, 6, 4, 0):
        for route, fmt in (("tissue", None), ("apply", _formats()[2]), ("raw", _formats()[1])):
            full, kw = _full(dev, route, M, mc, ab, fmt)
            got = _view(dev, dwin, size, d_mask, fmt=fmt, **kw)
            assert _same_bits(got, _ref(full, wild, *size, d_mask)), f"mask {d_mask} {route}"


# ---- 4. the full tile: all eight codes are the torch dihedral of the whole result -------------------------------------------------------
def test_full_tile_views_are_the_dihedral_group():
    n, h = 8, 64
    dev = _dev_tiles(_tiles(n, h, h), 0)
    win = np.array([(0, 0, d) for d in range(8)], dtype=np.int32)
    _check(dev, win, None, 7, ["tissue", "apply", "raw"], [None, _formats()[0], _formats()[3]])
    M, mc, ab = _stats(n)
    full, kw = _full(dev, "tissue", M, mc, ab)
    got = _view(dev, win, None, 7, **kw)
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], torch.flip(full[2], dims=(0, 1)))
    assert torch.equal(got[4], torch.flip(full[4], dims=(1,))) and torch.equal(got[1], torch.rot90(full[1], 1, dims=(0, 1)))
    assert len({got[t].numpy().tobytes() for t in range(8)}) == 8


def test_non_square_tile_at_full_size_without_quarter_turns():
    n, h, w = 4, 40, 72
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = np.array([(0, 0, d) for d in (0, 2, 4, 6)], dtype=np.int32)
    _check(dev, win, None, 6, ["tissue", "apply_neg", "raw"], [None, _formats()[1], _formats()[4]])


# ---- 5. both lasso regimes and the general cast, with and without a target --------------------------------------------------------------
@pytest.mark.parametrize("regime", ["he", "neg"])
def test_lasso_regimes_and_casts(regime):
    n, h, w, size = 8, 70, 66, (33, 47)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = _windows(n, h, w, *size, 7)
    _check(dev, win, size, 7, ROUTES[1:], [None, _formats()[2]], regime=regime)
    if regime == "he":                                        # (the general cast does something: values pass 255 and wrap)
        M, mc, ab = _stats(n)
        from stainlib_amd import engine
        assert not torch.equal(engine.normalize_apply(dev, M, mc, M_TGT_NEG, MAXC_TGT), engine.normalize_jitter(
            dev, M, mc, M_TGT_NEG, MAXC_TGT, np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (n, 1))))


# ---- 6. a failed fit in the middle of a batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["nan_M", "zero_maxC"])
def test_a_failed_fit_gives_the_view_of_its_own_bytes(how):
    n, h, w, size = 3, 70, 66, (33, 47)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = np.array([(3, 5, 1), (7, 9, 5), (1, 2, 6)], dtype=np.int32)
    M, mc, ab = _stats(n)
    M, mc = M.copy(), mc.copy()
    if how == "nan_M":
        M[1] = np.nan
    else:
        mc[1] = [1.0, 0.0]
    for route in ("apply", "tissue", "all_own"):
        for fmt in (None, _formats()[0], _formats()[5]):
            full, kw = _full(dev, route, M, mc, ab, fmt)
            raw, _ = _full(dev, "raw", M, mc, ab, fmt)
            assert _same_bits(full[1], raw[1])                                 # (the existing pass hands the tile through)
            got = _view(dev, win, size, 7, fmt=fmt, **kw)
            assert _same_bits(got, _ref(full, win, *size, 7)), f"{how} {route} {fmt}"
            assert _same_bits(got[1:2], _ref(raw, win, *size, 7)[1:2])


# ---- 7. the M_src=None route and TensorFormat.convert(view=) ----------------------------------------------------------------------------
def test_raw_route_is_convert_then_torch():
    n, h, w, size = 5, 96, 80, (64, 65)
    dev = _dev_tiles(_tiles(n, h, w), 1)
    view = stainlib_amd.TileView(size)
    np.random.seed(17)
    win = view.draw(n, h, w)
    for fmt in _formats():
        want = _ref(fmt.convert(dev).cpu(), win, *size, 7)
        assert _same_bits(_view(dev, win, size, 7, fmt=fmt), want)
        np.random.seed(17)
        x, win2 = fmt.convert(dev, view=view)
        assert np.array_equal(win2, win) and tuple(x.shape) == (n, 3, *size) and _same_bits(x.cpu(), want)
        assert x.is_contiguous(memory_format=torch.channels_last if fmt.channels_last else torch.contiguous_format)
        x3, win3 = fmt.convert(dev, view=view, windows=torch.from_numpy(win).cuda())
        assert win3.is_cuda and _same_bits(x3.cpu(), want)
    assert torch.equal(_view(dev, win, size, 7), _ref(dev.cpu(), win, *size, 7))


# ---- 8. the class methods ---------------------------------------------------------------------------------------------------------------
def test_view_through_the_batch_methods():
    tiles = [so.synth_tile(64, 64, s) for s in (2, 3, 4, 5)]
    dev = to_dev(tiles)
    n, h, w = 4, 64, 64
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    view = stainlib_amd.TileView(48)
    fmt = stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD)
    np.random.seed(9)
    ab = stainlib_amd.StainJitter().draw(n)
    # transform_batch
    full_u8, Mf, mcf, stf = nz.transform_batch(dev)
    np.random.seed(31)
    x, M, mc, st, win = nz.transform_batch(dev, view=view)
    after = np.random.uniform()
    np.random.seed(31)
    assert np.array_equal(win, view.draw(n, h, w)) and np.random.uniform() == after
    assert win.dtype == np.int32 and torch.equal(M, Mf) and torch.equal(mc, mcf) and torch.equal(st, stf) and st.cpu().tolist() == [0] * n
    assert x.dtype == torch.uint8 and tuple(x.shape) == (n, 48, 48, 3) and torch.equal(x.cpu(), _ref(full_u8.cpu(), win, 48, 48, 7))
    xt, _, _, _, win_t = nz.transform_batch(dev, tensor_format=fmt, view=view, windows=win)
    assert win_t is win and _same_bits(xt.cpu(), _ref(nz.transform_batch(dev, tensor_format=fmt)[0].cpu(), win, 48, 48, 7))
    # augment_batch of the normalizer, into a caller's buffer
    for bg in (False, True):
        full, _, _, _ = nz.augment_batch(dev, ab, augment_background=bg, tensor_format=fmt)
        buf = torch.empty((n, 3, 48, 48), dtype=torch.float16, device="cuda", memory_format=torch.channels_last)
        np.random.seed(32)
        x, M, _, st, win = nz.augment_batch(dev, ab, augment_background=bg, tensor_format=fmt, out=buf, view=view)
        np.random.seed(32)
        assert x is buf and np.array_equal(win, view.draw(n, h, w)) and torch.equal(M, Mf)
        assert _same_bits(x.cpu(), _ref(full.cpu(), win, 48, 48, 7)), f"bg={bg}"
        own, _, _, _ = nz.augment_batch(dev, ab, augment_background=bg, normalize=False)
        x, _, _, _, _ = nz.augment_batch(dev, ab, augment_background=bg, normalize=False, view=view, windows=win)
        assert torch.equal(x.cpu(), _ref(own.cpu(), win, 48, 48, 7))
        # StainAugmentor.augment_batch draws alpha_beta, then the windows
        sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1, augment_background=bg)
        np.random.seed(33)
        x, _, _, _, win = sa.augment_batch(dev, view=stainlib_amd.TileView((40, 56), rot90=False))
        np.random.seed(33)
        ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
        assert np.array_equal(win, stainlib_amd.TileView((40, 56), rot90=False).draw(n, h, w)) and set(win[:, 2].tolist()) <= {0, 2, 4, 6}
        full, _, _, _ = sa.augment_batch(dev, ab2)
        assert tuple(x.shape) == (n, 40, 56, 3) and torch.equal(x.cpu(), _ref(full.cpu(), win, 40, 56, 6))

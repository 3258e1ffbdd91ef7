"""-m gpu: HED augmentation behind the apply pass, inside the view pass (sl_normalize_sums, sl_normalize_hed_view, engine.normalize_sums /
normalize_hed_view, HedColorAugmenter.transform_batch(view=), hed= on the batch methods).

The definitions under test (include/stainlib_hip.h) are compositions of EXISTING entry points, so every comparison is exact:
    sums[t]  = the byte sum of full[t], the image normalize_apply / normalize_jitter / nothing writes for the whole tile
    view[t]  = normalize_view's window, flip and turn of  hed_applied[t] ? hed_augment(full, cutoff never fails)[t] : full[t]
with `full` and the windows made as in tests/test_gpu_view.py (whose helpers are imported, not copied).  Every call of _hed_view writes
into a buffer with sentinel elements before and after the output, checked after the call."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.test_gpu_jitter import MEAN, SENTINEL, STD, _dev_tiles, _formats, _same_bits, _stats, _tiles
from tests.test_gpu_view import ALL_FMTS, B, ROUTES, _full, _ref, _windows

pytestmark = pytest.mark.gpu

INF = float("inf")
# (n, h, w, byte offset): P = 35 -- P % 4 = 3, unaligned rows; fewer than 12 bytes; an aligned and an unaligned pointer; P = 32 942 -- two
# parts with a ragged last chunk; three parts behind an unaligned pointer
SUM_SHAPES = [(3, 5, 7, 0), (1, 1, 2, 0), (2, 64, 64, 0), (2, 64, 64, 1), (2, 182, 181, 0), (1, 257, 257, 1)]


def _hed_draws(n, seed=11):
    """per-tile-distinct sigmas / biases in the Strong range (+-1)"""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-1.0, 1.0, (n, 3))


def _chain(dev, route, M, mc, ab, sig, bia, applied, mode=0):
    """(where(applied, hed_augment(full), full) as a uint8 DEVICE tensor, the route's keyword arguments): the existing entry points"""
    from stainlib_amd import engine
    full, kw = _full(dev, route, M, mc, ab)
    full = full.cuda()
    aug, ok = engine.hed_augment(full, sig, bia, cutoff=(-INF, INF), skimage_mode=mode)
    assert ok.cpu().tolist() == [1] * dev.shape[0]
    on = torch.as_tensor(np.asarray(applied) != 0).view(-1, 1, 1, 1).cuda()
    return torch.where(on, aug, full), kw


def _hed_view(dev, win, size, d_mask, sig, bia, applied, fmt=None, out_off=0, mode=0, **kw):
    """engine.normalize_hed_view into a guarded buffer -> CPU tensor (tests/test_gpu_view.py: _view)"""
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
    res = engine.normalize_hed_view(dev, win, size, d_mask, sig, bia, applied, mode, fmt=fmt, out=out, **kw)
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
    sig, bia = _hed_draws(n)
    applied = np.arange(n, dtype=np.int32) % 2                      # both branches, and a wrong tile index shows
    for route in routes:
        img, kw = _chain(dev, route, M, mc, ab, sig, bia, applied)
        plain, _ = _full(dev, route, M, mc, ab)
        assert not torch.equal(img.cpu()[1], plain[1]) and torch.equal(img.cpu()[0], plain[0])      # (the stage does something)
        for fmt in fmts:
            want = _ref((img if fmt is None else fmt.convert(img)).cpu(), win, oh, ow, d_mask)
            for off in out_offs:
                got = _hed_view(dev, win, size, d_mask, sig, bia, applied, fmt=fmt, out_off=off, **kw)
                assert _same_bits(got, want), f"{label} {n}x{h}x{w} -> {oh}x{ow} mask {d_mask} {route} {regime} {fmt} out+{off}"


# ---- 1. the byte sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,off", SUM_SHAPES)
def test_sums_are_the_byte_sums_of_the_image_the_route_writes(n, h, w, off):
    from stainlib_amd import engine
    dev = _dev_tiles(_tiles(n, h, w), off)
    assert dev.data_ptr() % 4 == off
    src = dev.cpu().to(torch.int64).sum(dim=(1, 2, 3))
    for regime in ("he", "neg"):
        for bad in ((None, 0) if n == 1 else (n - 1,)):             # one tile per batch with a failed fit (n = 1: also without)
            M, mc, ab = _stats(n, regime)
            if bad is not None:
                M = M.copy()
                M[bad] = np.nan
            for route in ROUTES:
                full, kw = _full(dev, route, M, mc, ab)
                sums, applied = engine.normalize_sums(dev, **kw)
                assert sums.dtype == torch.int64 and applied.dtype == torch.int32 and tuple(sums.shape) == tuple(applied.shape) == (n,)
                want = full.to(torch.int64).sum(dim=(1, 2, 3))
                assert sums.cpu().tolist() == want.tolist(), f"{n}x{h}x{w}+{off} {regime} {route} bad={bad}"
                if bad is not None:
                    assert int(sums[bad]) == int(src[bad])           # (a failed fit: the source bytes' sum)
                if route == "raw":
                    assert sums.cpu().tolist() == src.tolist()


@pytest.mark.parametrize("cutoff", [(0.05, 0.95), (0.0, 1.0), (0.66, 0.67)])
def test_applied_is_hed_augments_decision_on_that_image(cutoff):
    from stainlib_amd import engine
    n, h, w = 8, 64, 64
    dev = _dev_tiles(_tiles(n, h, w), 0)
    M, mc, ab = _stats(n)
    zero = np.zeros((n, 3))
    seen = set()
    for route in ROUTES:
        full, kw = _full(dev, route, M, mc, ab)
        _, want = engine.hed_augment(full.cuda(), zero, zero, cutoff=cutoff)
        _, applied = engine.normalize_sums(dev, cutoff=cutoff, **kw)
        assert torch.equal(applied, want), f"{route} {cutoff}"
        seen |= set(applied.cpu().tolist())
    assert seen == ({0, 1} if cutoff == (0.66, 0.67) else {1})      # (the narrow interval splits the batches)


# ---- 2. the HED view: outputs smaller than a patch from a tiny tile, every route, every output form -------------------------------------
@pytest.mark.parametrize("size,d_mask", [((5, 7), 6), ((5, 5), 7)])
def test_tiny_tiles_every_route_and_format(size, d_mask):
    n, h, w = 8, 9, 11
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = _windows(n, h, w, *size, d_mask)
    _check(dev, win, size, d_mask, ROUTES, ALL_FMTS, out_offs=(0, 1))
    _check(dev, win, size, d_mask, ["apply", "tissue", "all_own"], [None, _formats()[2]], regime="neg")


# ---- 3. ragged last patches in both directions, all eight codes in one batch (test_ragged_patches_all_codes_in_one_batch's geometry) -----
@pytest.mark.parametrize("off", [0, 1])
def test_ragged_patches_all_codes_in_one_batch(off):
    n, h, oh, ow = 8, 2 * B + 3, 2 * B + 3, B - 1
    dev = _dev_tiles(_tiles(n, h, h), off)
    assert dev.data_ptr() % 4 == off
    win = np.array([(0, 0, 0), (68, 0, 1), (0, 1, 2), (67, 0, 3), (0, 2, 4), (3, 0, 5), (0, 3, 6), (0, 0, 7)], dtype=np.int32)
    assert sorted(win[:, 2].tolist()) == list(range(8))
    _check(dev, win, (oh, ow), 7, ["tissue"], ALL_FMTS, label=f"+{off}")
    _check(dev, win, (oh, ow), 7, ["raw", "apply_neg", "all_own"], [None, _formats()[3]], label=f"+{off}")


# ---- 4. a failed fit in the middle of a batch ---------------------------------------------------------------------------------------------
def test_a_failed_fit_takes_the_stage_on_its_own_bytes():
    from stainlib_amd import engine
    n, h, w, size = 3, 70, 66, (33, 47)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = np.array([(3, 5, 1), (7, 9, 5), (1, 2, 6)], dtype=np.int32)
    M, mc, ab = _stats(n)
    M = M.copy()
    M[1] = np.nan
    sig, bia = _hed_draws(n)
    src_hed, _ = engine.hed_augment(dev, sig, bia, cutoff=(-INF, INF))
    for route in ("apply", "tissue", "all_own"):
        for fmt in (None, _formats()[0], _formats()[5]):
            for on in (1, 0):
                applied = np.array([1, on, 0], dtype=np.int32)
                img, kw = _chain(dev, route, M, mc, ab, sig, bia, applied)
                assert torch.equal(img[1], src_hed[1] if on else dev[1])          # (the chain: the HED of the source bytes, or they themselves)
                want = _ref((img if fmt is None else fmt.convert(img)).cpu(), win, *size, 7)
                got = _hed_view(dev, win, size, 7, sig, bia, applied, fmt=fmt, **kw)
                assert _same_bits(got, want), f"{route} {fmt} applied={on}"


# ---- 5. the unpinned skimage modes give their chain's bits through the Python surface -----------------------------------------------------
@pytest.mark.parametrize("mode", ["0.19", "0.17", "experimental_log10"])
def test_unpinned_modes_equal_their_chain(mode):
    n, h, w, size = 4, 40, 44, (20, 30)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = _windows(n, h, w, *size, 7)
    M, mc, ab = _stats(n)
    sig, bia = _hed_draws(n)
    applied = np.array([1, 0, 1, 1], dtype=np.int32)
    aug = stainlib_amd.HedStrongColorAugmenter(skimage_mode=mode)
    code = aug._skimage_mode
    assert code in (1, 2, 3)
    for route in ("raw", "tissue"):
        img, kw = _chain(dev, route, M, mc, ab, sig, bia, applied, mode=code)
        for fmt in (None, _formats()[2]):
            want = _ref((img if fmt is None else fmt.convert(img)).cpu(), win, *size, 7)
            assert _same_bits(_hed_view(dev, win, size, 7, sig, bia, applied, fmt=fmt, mode=code, **kw), want), f"{mode} {route} {fmt}"
    # and through the class: the raw route
    view = stainlib_amd.TileView(size)
    x, ok, win2 = aug.transform_batch(dev, sig, bia, view=view, windows=win)
    u8, ok2 = aug.transform_batch(dev, sig, bia)
    assert win2 is win and torch.equal(ok, ok2) and torch.equal(x.cpu(), _ref(u8.cpu(), win, *size, 7))


# ---- 6. the classes ---------------------------------------------------------------------------------------------------------------------
def _class_batch():
    """six synthetic tiles (means 0.64 - 0.67) and two whose mean fails the default cutoff: all 255 (1.0) and all 3 (0.012)"""
    t = _tiles(6, 64, 64)
    return _dev_tiles(torch.cat([t, torch.full((1, 64, 64, 3), 255, dtype=torch.uint8), torch.full((1, 64, 64, 3), 3, dtype=torch.uint8)]), 0)


def _f16():
    return stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD)


def test_hed_augmenter_with_a_view_is_its_own_chain():
    dev = _class_batch()
    n = dev.shape[0]
    aug = stainlib_amd.HedLighterColorAugmenter()
    view, fmt = stainlib_amd.TileView(48), _f16()
    rng = np.random.RandomState(3)
    for sig, bia in ((None, None), (rng.uniform(-0.03, 0.03, (n, 3)), rng.uniform(-0.03, 0.03, (n, 3)))):
        np.random.seed(21)
        x, applied, win = aug.transform_batch(dev, sig, bia, view=view, tensor_format=fmt)
        after = np.random.uniform()
        np.random.seed(21)
        assert np.array_equal(win, view.draw(n, 64, 64)) and np.random.uniform() == after        # only the windows are drawn
        u8, applied2 = aug.transform_batch(dev, sig, bia)
        want, _ = fmt.convert(u8, view=view, windows=win)
        assert torch.equal(applied, applied2) and applied.cpu().tolist() == [1] * 6 + [0, 0]
        assert tuple(x.shape) == (n, 3, 48, 48) and _same_bits(x.cpu(), want.cpu())
        x8, applied3, _ = aug.transform_batch(dev, sig, bia, view=view, windows=win)
        assert torch.equal(applied3, applied2) and torch.equal(x8.cpu(), _ref(u8.cpu(), win, 48, 48, 7))
    assert not torch.equal(u8[0], dev[0]) and torch.equal(u8[6], dev[6])


@pytest.mark.parametrize("method", ["macenko", "vahadane"])
def test_hed_through_the_batch_methods_is_the_three_call_chain(method):
    from stainlib_amd import engine
    dev = _class_batch()
    n = dev.shape[0]
    nz = stainlib_amd.MacenkoNormalizer() if method == "macenko" else stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    aug = stainlib_amd.HedLightColorAugmenter()
    view, fmt = stainlib_amd.TileView(48), _f16()
    np.random.seed(9)
    ab = stainlib_amd.StainJitter().draw(n)
    # augment_batch: the view and the tensor
    np.random.seed(41)
    x, M, mc, st, win, draw = nz.augment_batch(dev, ab, hed=aug, view=view, tensor_format=fmt)
    np.random.seed(41)
    sig, bia = aug.randomize_batch(n)                                # the draws: HED first, then the windows
    assert np.array_equal(draw.sigmas, sig) and np.array_equal(draw.biases, bia) and np.array_equal(win, view.draw(n, 64, 64))
    assert isinstance(draw, engine.HedDraw) and int(st[6]) != 0     # (the white tile has no tissue: it passes through)
    u8, M2, mc2, st2 = nz.augment_batch(dev, ab)
    h8, applied = aug.transform_batch(u8, draw.sigmas, draw.biases)
    want, _ = fmt.convert(h8, view=view, windows=win)
    assert torch.equal(st, st2) and torch.equal(M[st == 0], M2[st2 == 0]) and torch.equal(mc[st == 0], mc2[st2 == 0])
    assert torch.equal(draw.applied, applied) and set(applied.cpu().tolist()) == {0, 1}
    assert _same_bits(x.cpu(), want.cpu()), method
    # transform_batch: the uint8 view, given draws
    x, _, _, st, win, draw = nz.transform_batch(dev, hed=aug, hed_sigmas=sig, hed_biases=bia, view=view)
    h8, applied = aug.transform_batch(nz.transform_batch(dev)[0], sig, bia)
    assert torch.equal(draw.applied, applied) and draw.sigmas is sig
    assert x.dtype == torch.uint8 and torch.equal(x.cpu(), _ref(h8.cpu(), win, 48, 48, 7)), method
    # without a view: the full tile, one element fewer
    res = nz.transform_batch(dev, hed=aug, hed_sigmas=sig, hed_biases=bia, tensor_format=fmt)
    assert len(res) == 5 and _same_bits(res[0].cpu(), fmt.convert(h8).cpu())
    if method != "macenko":
        return
    # StainAugmentor: alpha_beta, then the HED draws
    sa = stainlib_amd.StainAugmentor(method, sigma1=0.15, sigma2=0.1)
    np.random.seed(43)
    x, _, _, _, draw = sa.augment_batch(dev, hed=aug)
    after = np.random.uniform()
    np.random.seed(43)
    ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
    sig2, bia2 = aug.randomize_batch(n)
    assert np.random.uniform() == after and np.array_equal(draw.sigmas, sig2) and np.array_equal(draw.biases, bia2)
    h8, applied = aug.transform_batch(sa.augment_batch(dev, ab2)[0], sig2, bia2)
    assert torch.equal(draw.applied, applied) and torch.equal(x, h8), method


def test_a_mean_on_the_cutoff_bound_is_decided_as_the_chain_decides_it():
    """the knife-edge rule: a cutoff bound within _CUTOFF_BAND of a tile's exact mean -- the reference's float32 mean decides, in the fused
    call as in HedColorAugmenter.transform_batch, on the raw route and behind normalisation"""
    from stainlib_amd import engine
    from stainlib_amd.augmentation.augmenter import _CUTOFF_BAND, HedColorAugmenter
    dev = _dev_tiles(_tiles(4, 64, 64), 0)
    n = dev.shape[0]
    sig, bia = _hed_draws(n, seed=5)
    sig, bia = 0.1 * sig, 0.1 * bia
    view = stainlib_amd.TileView(40)
    win = view.draw(n, 64, 64)
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    norm, M, mc, _ = nz.transform_batch(dev)
    M_t, c_t = nz._target_on(dev.device)
    for route in ("raw", "apply"):
        kw = {} if route == "raw" else dict(M_src=M, maxC_src=mc, M_tgt=M_t, maxC_tgt=c_t)
        sums, _ = engine.normalize_sums(dev, **kw)
        src = dev if route == "raw" else norm
        assert sums.cpu().tolist() == src.cpu().to(torch.int64).sum(dim=(1, 2, 3)).tolist()
        for t in range(n):
            m = int(sums[t]) / (64 * 64 * 3) / 255.0
            for lo in (m * (1 + 2e-6), m * (1 - 2e-6)):
                assert abs(m - lo) <= _CUTOFF_BAND * 1.0 and lo != m
                aug = HedColorAugmenter(*[(-0.1, 0.1)] * 6, cutoff_range=(lo, 1.0))
                u8, applied = aug.transform_batch(src, sig, bia)
                if route == "raw":
                    x, got, _ = aug.transform_batch(dev, sig, bia, view=view, windows=win)
                else:
                    x, _, _, _, _, draw = nz.transform_batch(dev, hed=aug, hed_sigmas=sig, hed_biases=bia, view=view, windows=win)
                    got = draw.applied
                assert torch.equal(got, applied), f"{route} tile {t} lo={lo!r}"
                assert torch.equal(x.cpu(), _ref(u8.cpu(), win, 40, 40, 7)), f"{route} tile {t}"

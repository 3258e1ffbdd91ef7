"""-m gpu: the 2x / 4x box shrink inside the view passes (sl_normalize_view_shrink and its four siblings; TileView(shrink=) through every
call that accepts view=).

The definition under test (include/stainlib_hip.h): with `full` the uint8 image the same call writes WITHOUT view=, per channel
    S[i, j] = sum of full[y0 + s i + a, x0 + s j + b], a, b in 0..s-1;   b[i, j] = (S[i, j] + s s / 2) >> (2 log2 s)
    result  = rot90(flip(b) if d & 4 else b, d & 3);   a tensor output = TensorFormat.convert(result)
Everything is integer arithmetic on bytes, so every comparison is exact: torch slicing, integer box sums, that rounding, flip / rot90
and TensorFormat.convert on the existing entry point's full-tile result.

Shapes: 9 tiles of 81 x 151 (odd: the rows start at every residue mod 4); s = 2 -> (33, 37) from 66 x 74 / 74 x 66 windows: 2 x 2 patches
of 32 output pixels with ragged edges and a ragged last lane; s = 4 -> (17, 18) from 68 x 72 / 72 x 68: 2 x 2 patches of 16; s = 1 at
the same sizes.  Tiles 0..7 take the eight dihedral codes with x0 over all residues mod 4, tile 0 sits at (0, 0), tiles 7 and 8 have their
windows flush against the tile's end, and tile 8 of the fitted batches is all white (a non-zero fit status: its own bytes, shrunk)."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.test_gpu_jitter import MEAN, STD, _dev_tiles, _formats, _same_bits, _stats
from tests.test_gpu_lab_view import _normalizer
from tests.test_gpu_lab_view import _view as _lab_view
from tests.test_gpu_view import _view

pytestmark = pytest.mark.gpu

N, H, W = 9, 81, 151
SIZES = {1: (33, 37), 2: (33, 37), 4: (17, 18)}
SHIFT = {1: 0, 2: 2, 4: 4}
_CACHE = {}


def _windows(s, size=None):
    oh, ow = size or SIZES[s]
    win = []
    for t in range(N):
        d = t if t < 8 else 3
        wh, ww = (s * ow, s * oh) if d & 1 else (s * oh, s * ow)
        ymax, xmax = H - wh, W - ww
        assert ymax >= 0 and xmax >= 30
        win.append((0, 0, d) if t == 0 else (ymax, xmax, d) if t >= 7 else ((3 * t + 1) % (ymax + 1), 5 * t, d))
    win = np.array(win, dtype=np.int32)
    assert {int(x) % 4 for x in win[:7, 1]} == {0, 1, 2, 3} and sorted(win[:8, 2].tolist()) == list(range(8))
    return win


def _shrunk(full, win, size, s, d_mask=7, dihedral_first=False):
    """the definition on `full` ((n, h, w, 3) uint8, CPU) -> (n, oh, ow, 3) uint8: clamp, slice, integer box sums, round half up,
    flip along the width, rot90 -- or the dihedral transform of the window first, then the boxes (they commute)"""
    oh, ow = size
    n, h, w, _ = full.shape
    outs = []
    for t, (y0, x0, d) in enumerate(np.asarray(win).tolist()):
        d &= d_mask
        k = d & 3
        wh, ww = (ow, oh) if k & 1 else (oh, ow)
        y0, x0 = min(max(y0, 0), h - s * wh), min(max(x0, 0), w - s * ww)
        v = full[t, y0:y0 + s * wh, x0:x0 + s * ww]

        def box(v):
            S = v.to(torch.int32).reshape(v.shape[0] // s, s, v.shape[1] // s, s, 3).sum(dim=(1, 3))
            assert int(S.max()) <= 255 * s * s
            return ((S + (s * s) // 2) >> SHIFT[s]).to(torch.uint8)

        def dihedral(v):
            return torch.rot90(torch.flip(v, dims=(1,)) if d & 4 else v, k, dims=(0, 1))

        b = box(dihedral(v)) if dihedral_first else dihedral(box(v))
        assert tuple(b.shape) == (oh, ow, 3)
        outs.append(b)
    return torch.stack(outs).contiguous()


def _want(full_u8, win, size, s, fmt=None, d_mask=7):
    u8 = _shrunk(full_u8.cpu(), win, size, s, d_mask)
    return u8 if fmt is None else fmt.convert(u8.cuda()).cpu()


def _batch():
    """8 synthetic H&E tiles, each from its own seed, and an all-white one (no tissue: every fit reports a status) -- on the device"""
    if "batch" not in _CACHE:
        t = np.stack([so.synth_tile(H, W, 60 + 7 * i) for i in range(N - 1)] + [np.full((H, W, 3), 255, dtype=np.uint8)])
        _CACHE["batch"] = _dev_tiles(torch.from_numpy(t), 1)
    return _CACHE["batch"]


def _raw_batch(s, win):
    """random bytes; tile 6: inside its window the box (i, j) of channel c sums to s s v + k with k = (i + s j + c) mod s s, so that
    S mod s s takes every value, the tie s s / 2 included; tile 7: all 255 (S = 4080 at s = 4: the largest sum, no carry between the
    packed lanes)"""
    rng = np.random.RandomState(100 + s)
    t = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    y0, x0, d = win[6].tolist()
    oh, ow = SIZES[s]
    wh, ww = (ow, oh) if d & 1 else (oh, ow)
    for i in range(wh):
        for j in range(ww):
            for c in range(3):
                blk = np.full(s * s, (7 * i + 3 * j + 5 * c) % 200, dtype=np.uint8)
                blk[:(i + s * j + c) % (s * s)] += 1
                t[6, y0 + s * i:y0 + s * i + s, x0 + s * j:x0 + s * j + s, c] = rng.permutation(blk).reshape(s, s)
    t[7] = 255
    return torch.from_numpy(t)


F16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=MEAN, std=STD)


# ---- 1. raw mode: TensorFormat.convert(view=) and the uint8 view on synthetic bytes, every output form; the commutation -------------------
@pytest.mark.parametrize("s", [2, 4])
def test_raw_bytes_every_output_form_and_the_commutation(s):
    size, win = SIZES[s], _windows(s)
    cpu = _raw_batch(s, win)
    dev = _dev_tiles(cpu, 1)
    want = _shrunk(cpu, win, size, s)
    assert torch.equal(want, _shrunk(cpu, win, size, s, dihedral_first=True))          # shrink(dihedral(.)) == dihedral(shrink(.))
    # (the inputs do what they were built for: every residue of S mod s s in tile 6's window, the all-255 tile stays 255)
    y0, x0, d = win[6].tolist()
    wh, ww = (s * size[1], s * size[0]) if d & 1 else (s * size[0], s * size[1])
    S = cpu[6, y0:y0 + wh, x0:x0 + ww].to(torch.int32).reshape(wh // s, s, ww // s, s, 3).sum(dim=(1, 3))
    assert set((S % (s * s)).reshape(-1).tolist()) == set(range(s * s)) and bool((want[7] == 255).all())
    got = _view(dev, win, size, 7, shrink=s)
    assert torch.equal(got, want)
    assert len({got[t].numpy().tobytes() for t in range(N)}) == N
    view = stainlib_amd.TileView(size, shrink=s)
    for fmt in _formats():
        wt = fmt.convert(want.cuda()).cpu()
        for off in (0, 1):
            assert _same_bits(_view(dev, win, size, 7, fmt=fmt, out_off=off, shrink=s), wt), f"{fmt} out+{off}"
        x, win2 = fmt.convert(dev, view=view, windows=win)
        assert win2 is win and tuple(x.shape) == (N, 3, *size) and _same_bits(x.cpu(), wt), f"{fmt}"
        assert x.is_contiguous(memory_format=torch.channels_last if fmt.channels_last else torch.contiguous_format)
    # drawn windows: the documented draws, every window inside the s-times range
    np.random.seed(5)
    x, wd = F16.convert(dev, view=view)
    np.random.seed(5)
    assert np.array_equal(wd, view.draw(N, H, W)) and _same_bits(x.cpu(), F16.convert(_shrunk(cpu, wd, size, s).cuda()).cpu())


# ---- 2. the extractive normalizers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_macenko_transform_and_augment_batch(s):
    dev, size, win = _batch(), SIZES[s], _windows(s)
    view = stainlib_amd.TileView(size, shrink=s)
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    full, Mf, mcf, stf = nz.transform_batch(dev)
    assert int(stf[8]) != 0 and stf[:8].cpu().tolist() == [0] * 8 and torch.equal(full[8], dev[8])
    for fmt in (None, F16):
        x, M, mc, st, win2 = nz.transform_batch(dev, tensor_format=fmt, view=view, windows=win)
        assert win2 is win and torch.equal(st, stf) and torch.equal(M[:8], Mf[:8]) and torch.equal(mc[:8], mcf[:8])
        assert _same_bits(x.cpu(), _want(full, win, size, s, fmt)), f"transform_batch {fmt}"
    ab = _stats(N)[2]
    for bg in (False, True):
        full = nz.augment_batch(dev, ab, augment_background=bg)[0]
        for fmt in (None, F16):
            x, _, _, st, _ = nz.augment_batch(dev, ab, augment_background=bg, tensor_format=fmt, view=view, windows=win)
            assert torch.equal(st, stf) and _same_bits(x.cpu(), _want(full, win, size, s, fmt)), f"augment_batch bg={bg} {fmt}"
    # drawn windows: alpha_beta first, then view.draw, which stays inside the s-times window
    sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1)
    np.random.seed(8)
    x, _, _, _, wd = sa.augment_batch(dev, view=view)
    np.random.seed(8)
    ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(N)
    assert np.array_equal(wd, view.draw(N, H, W))
    assert torch.equal(x.cpu(), _want(sa.augment_batch(dev, ab2)[0], wd, size, s))


def test_vahadane_transform_batch():
    s = 2
    dev, size, win = _batch(), SIZES[s], _windows(s)
    nz = stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    full, _, _, stf = nz.transform_batch(dev)
    x, _, _, st, _ = nz.transform_batch(dev, view=stainlib_amd.TileView(size, shrink=s), windows=win)
    assert torch.equal(st, stf) and int(st[8]) != 0 and torch.equal(x.cpu(), _want(full, win, size, s))


# ---- 3. HED behind the normalisation and on raw tiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_hed_stage_with_a_shrunk_view(s):
    dev, size, win = _batch(), SIZES[s], _windows(s)
    view = stainlib_amd.TileView(size, shrink=s)
    aug = stainlib_amd.HedLightColorAugmenter()
    rng = np.random.RandomState(3)
    sig, bia = rng.uniform(-0.03, 0.03, (N, 3)), rng.uniform(-0.03, 0.03, (N, 3))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    ab = _stats(N)[2]
    h8, applied = aug.transform_batch(nz.augment_batch(dev, ab)[0], sig, bia)          # the chain at source resolution
    assert 1 in applied.cpu().tolist()
    for fmt in (None, F16):
        x, _, _, _, win2, draw = nz.augment_batch(dev, ab, hed=aug, hed_sigmas=sig, hed_biases=bia, tensor_format=fmt, view=view, windows=win)
        assert win2 is win and torch.equal(draw.applied, applied)                     # the cutoff sums are the whole tile's
        assert _same_bits(x.cpu(), _want(h8, win, size, s, fmt)), f"augment_batch(hed=) {fmt}"
    # StainAugmentor.augment_batch(hed=): every tile under its own matrix
    sa = stainlib_amd.StainAugmentor("macenko")
    h8, applied = aug.transform_batch(sa.augment_batch(dev, ab)[0], sig, bia)
    x, _, _, _, _, draw = sa.augment_batch(dev, ab, view=view, windows=win, hed=aug, hed_sigmas=sig, hed_biases=bia)
    assert torch.equal(draw.applied, applied) and torch.equal(x.cpu(), _want(h8, win, size, s)), "StainAugmentor.augment_batch(hed=)"
    # HedColorAugmenter.transform_batch(view=) on raw tiles
    h8, applied = aug.transform_batch(dev, sig, bia)
    assert set(applied.cpu().tolist()) == {0, 1}                                       # (the white tile fails the cutoff)
    for fmt in (None, F16):
        x, applied_v, _ = aug.transform_batch(dev, sig, bia, tensor_format=fmt, view=view, windows=win)
        assert torch.equal(applied_v, applied) and _same_bits(x.cpu(), _want(h8, win, size, s, fmt)), f"transform_batch {fmt}"


# ---- 4. the Lab family: per tile and pooled -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_lab_family_per_tile_and_pooled(s):
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    dev, size, win = _batch(), SIZES[s], _windows(s)
    view = stainlib_amd.TileView(size, shrink=s)
    nz = _normalizer()
    full, stats = nz.transform_batch(dev, mask_background=True)
    lum, p = stainlib_amd.LuminosityStandardizer.standardize_batch(dev)
    sn = SlideNormalizer(nz, group=False, mode="pooled")
    pooled, means, stds, status = sn.transform_shard(dev, mask_background=True)
    plum, pp = slide_luminosity_standardize(dev, group=False)
    for fmt in (None, F16):
        x, st, win2 = nz.transform_batch(dev, mask_background=True, tensor_format=fmt, view=view, windows=win)
        assert win2 is win and torch.equal(st.cpu().view(torch.int64), stats.cpu().view(torch.int64))
        assert _same_bits(x.cpu(), _want(full, win, size, s, fmt)), f"reinhard {fmt}"
        x, p_v, _ = stainlib_amd.LuminosityStandardizer.standardize_batch(dev, tensor_format=fmt, view=view, windows=win)
        assert torch.equal(p_v, p) and _same_bits(x.cpu(), _want(lum, win, size, s, fmt)), f"luminosity {fmt}"
        res = sn.transform_shard(dev, mask_background=True, tensor_format=fmt, view=view, windows=win)
        assert len(res) == 5 and torch.equal(res[3], status) and _same_bits(res[0].cpu(), _want(pooled, win, size, s, fmt)), f"pooled reinhard {fmt}"
        x, pp_v, _ = slide_luminosity_standardize(dev, group=False, tensor_format=fmt, view=view, windows=win)
        assert pp_v == pp and _same_bits(x.cpu(), _want(plum, win, size, s, fmt)), f"pooled luminosity {fmt}"


def test_a_pooled_slide_without_tissue_gives_the_shrunk_view_of_its_own_bytes():
    from stainlib_amd.distributed import SlideNormalizer
    from stainlib_amd.utils.excepts import TissueMaskException
    s = 2
    size, win = SIZES[s], _windows(s)
    white = np.full((N, H, W, 3), 255, dtype=np.uint8)
    white[:, ::7, ::5] = (250, 252, 249)                                                # (background only, but not constant)
    dev = torch.from_numpy(white).cuda()
    sn = SlideNormalizer(_normalizer(), group=False, mode="pooled")
    out = torch.zeros((N, *size, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TissueMaskException):
        sn.transform_shard(dev, out=out, mask_background=True, view=stainlib_amd.TileView(size, shrink=s), windows=win)
    assert torch.equal(out.cpu(), _want(dev, win, size, s))


# ---- 5. device windows are clamped to the s-times window by the kernel ------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_device_windows_out_of_range_equal_the_clamped_window(s):
    from stainlib_amd import engine
    dev, size = _batch(), SIZES[s]
    wild = np.array([(-1, -1, 0), (10 ** 9, 10 ** 9, 1), (-2 ** 31, 2 ** 31 - 1, 2), (2 ** 31 - 1, -2 ** 31, 3), (H - s * size[0] + 1, 0, 4),
                     (0, W - s * size[0] + 1, 5), (16, 80, 6), (5, 100, 7), (100, 5, 3 | 8)], dtype=np.int64).astype(np.int32)
    dwin = torch.from_numpy(wild).cuda()
    clamped = wild.copy()
    for t, (y0, x0, d) in enumerate(wild.tolist()):
        wh, ww = (s * size[1], s * size[0]) if d & 1 else (s * size[0], s * size[1])
        clamped[t] = (min(max(y0, 0), H - wh), min(max(x0, 0), W - ww), d & 7)
    M, mc, ab = _stats(N)
    routes = [dict(), dict(M_src=M, maxC_src=mc, M_tgt=None, maxC_tgt=None, alpha_beta=ab, augment_background=False)]
    fulls = [dev, engine.normalize_jitter(dev, M, mc, None, None, ab)]
    for kw, full in zip(routes, fulls):
        for fmt in (None, F16):
            got = _view(dev, dwin, size, 7, fmt=fmt, shrink=s, **kw)
            assert _same_bits(got, _want(full, wild, size, s, fmt))
            assert _same_bits(got, _view(dev, clamped, size, 7, fmt=fmt, shrink=s, **kw))      # the clamped HOST windows
    tm, ts = _normalizer()._targets()
    full = engine.reinhard_transform(dev, tm, ts, mask_background=True)[0]
    got, _ = _lab_view("reinhard", dev, dwin, size, 7, mask_background=True, shrink=s)
    assert torch.equal(got, _want(full, wild, size, s))
    assert torch.equal(got, _lab_view("reinhard", dev, clamped, size, 7, mask_background=True, shrink=s)[0])


# ---- 6. shrink = 1 is today's result on every route -----------------------------------------------------------------------------------------
def test_shrink_one_is_todays_result_draws_and_entry_points():
    from stainlib_amd import _ffi, engine
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    dev = _batch()
    for size in (SIZES[2], SIZES[4]):
        win = _windows(1, size)
        v0, v1 = stainlib_amd.TileView(size), stainlib_amd.TileView(size, shrink=1)
        np.random.seed(4)
        w0 = v0.draw(N, H, W)
        a0 = np.random.uniform()
        np.random.seed(4)
        w1 = v1.draw(N, H, W)
        assert np.array_equal(w0, w1) and np.random.uniform() == a0
        # the C exports with shrink = 1 against their parents (the raw and the jitter route; uint8 and float16)
        M, mc, ab = _stats(N)
        dwin = torch.from_numpy(win).cuda()
        for kw in (dict(), dict(M_src=M, maxC_src=mc, alpha_beta=ab)):
            up = engine._route_upload(N, dev.device, kw.get("M_src"), kw.get("maxC_src"), None, None, kw.get("alpha_beta"))
            for fmt in (None, F16):
                want = engine.normalize_view(dev, win, size, 7, fmt=fmt, **kw)
                f, got = engine._image_out(None, dev, N, *size, fmt, "view")
                got.fill_(77)
                engine._call("sl_normalize_view_shrink", engine._ptr(dev), engine._ptr(got), N, H, W, *size, engine._ptr(dwin), 7, 1,
                             *(engine._ptr(x) for x in up), 0, None, engine._byref(f))
                assert _same_bits(got.cpu(), want.cpu()), f"sl_normalize_view_shrink(1) {sorted(kw)} {fmt}"
        nz = stainlib_amd.MacenkoNormalizer()
        nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
        aug = stainlib_amd.HedLightColorAugmenter()
        rng = np.random.RandomState(3)
        sig, bia = rng.uniform(-0.03, 0.03, (N, 3)), rng.uniform(-0.03, 0.03, (N, 3))
        rz = _normalizer()
        sn = SlideNormalizer(rz, group=False, mode="pooled")
        calls = [lambda v: F16.convert(dev, view=v, windows=win)[0],
                 lambda v: nz.transform_batch(dev, view=v, windows=win)[0],
                 lambda v: nz.augment_batch(dev, ab, augment_background=True, tensor_format=F16, view=v, windows=win)[0],
                 lambda v: nz.augment_batch(dev, ab, hed=aug, hed_sigmas=sig, hed_biases=bia, view=v, windows=win)[0],
                 lambda v: aug.transform_batch(dev, sig, bia, view=v, windows=win)[0],
                 lambda v: rz.transform_batch(dev, mask_background=True, view=v, windows=win)[0],
                 lambda v: stainlib_amd.LuminosityStandardizer.standardize_batch(dev, tensor_format=F16, view=v, windows=win)[0],
                 lambda v: sn.transform_shard(dev, mask_background=True, view=v, windows=win)[0],
                 lambda v: slide_luminosity_standardize(dev, group=False, view=v, windows=win)[0]]
        for i, call in enumerate(calls):
            assert _same_bits(call(v1).cpu(), call(v0).cpu()), f"route {i} {size}"
        assert torch.equal(calls[1](v1).cpu(), _want(nz.transform_batch(dev)[0], win, size, 1))
        assert _ffi.lib().sl_version() == _ffi.EXPECTED_VERSION

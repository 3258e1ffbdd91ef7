"""-m gpu: the resizing view (random-resized crop) inside the view passes: sl_normalize_view_resize, sl_normalize_hed_view_resize and
TileView(scale=) through every call of k_view / k_hed_view.

The definition under test (include/stainlib_hip.h): windows[t] = (y0, x0, d, wh, ww); with `full` the uint8 image the same call writes
WITHOUT view=, the window full[t][y0:y0+wh, x0:x0+ww] is resampled to (nu, nv) -- (oh, ow), transposed for an odd number of quarter
turns -- by exact pixel-area averaging, S = sum cy(i, k) cx(j, l) window[k, l], b = (2 S + D) // (2 D), D = wh ww, then flipped and
turned; a tensor is TensorFormat.convert(b).  Integer arithmetic on bytes: every comparison is exact, against the numpy restatement
of tests/test_view_resize_host.py (want_view) on the existing entry point's full-tile result.

Shapes: 9 tiles of 81 x 151 (odd: the rows start at every residue mod 4), output (33, 37).  ONE call mixes the eight dihedral codes, x0
over all residues mod 4 and these windows: the identity (a patch of 63), exact 2x, the whole tile 81 x 151 and 81 x 150 (non-integer
ratios; patches of 15 or 13 outputs along the width: three of them, so taps straddle patch edges), 81 x 20 (down vertically, up
horizontally), 3 x 5 and 1 x 1 (upscaling), and windows flush against the tile's end (the read side's tail).  A second call takes
output (5, 4) from 80 x 64 and 79 x 63 windows: ratio 16, and 17 taps."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.test_gpu_jitter import MEAN, STD, _dev_tiles, _formats, _same_bits, _stats
from tests.test_gpu_view import _view
from tests.test_gpu_view_shrink import SIZES
from tests.test_gpu_view_shrink import _batch
from tests.test_gpu_view_shrink import _windows as _shrink_windows
from tests.test_view_resize_host import clamp_window, resample_ref, want_view

pytestmark = pytest.mark.gpu

N, H, W = 9, 81, 151
SIZE = (33, 37)
BOUND = (H, W)
F16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=MEAN, std=STD)

# (y0, x0, d, wh, ww): see the module docstring
WIN = np.array([(0, 0, 0, 33, 37),              # the identity at the corner
                (3, 5, 1, 74, 66),              # exact 2x, turned: (nu, nv) = (37, 33)
                (0, 0, 2, 81, 151),             # the whole tile
                (0, 1, 3, 81, 150),             # nearly: turned
                (0, 10, 4, 81, 20),             # down vertically, up horizontally
                (40, 7, 5, 3, 5),               # upscaling
                (80, 150, 6, 1, 1),             # one pixel, the tile's last
                (H - 37, W - 33, 7, 37, 33),    # the identity, turned, flush against the end
                (H - 74, W - 66, 3, 74, 66)],   # exact 2x flush against the end
               dtype=np.int32)
assert {int(x) % 4 for x in WIN[:, 1]} == {0, 1, 2, 3} and sorted(WIN[:8, 2].tolist()) == list(range(8))
# output (5, 4): ratio 16 exactly (16 taps, aligned) and just below it (17 taps); odd codes take (4, 5) outputs
SIZE16 = (5, 4)
WIN16 = np.array([(0, 0, 0, 80, 64), (17, 71, 1, 64, 80), (1, 3, 2, 79, 63), (17, 70, 3, 63, 79), (0, 2, 4, 80, 63), (9, 5, 5, 63, 80),
                  (1, 86, 6, 80, 64), (17, 71, 7, 64, 80), (2, 88, 0, 79, 63)], dtype=np.int32)


def _want(full_u8, win, size, fmt=None, d_mask=7, resize=None):
    u8 = torch.from_numpy(want_view(full_u8.cpu().numpy(), win, size, d_mask, resize))
    return u8 if fmt is None else fmt.convert(u8.cuda()).cpu()


def _edge_batch():
    """every tile a vertical step edge at column 75, a to the left and b to the right with a + b odd; the windows are 47 x 50 at x0 = 50 --
    the edge at window column 25 of 50, a NON-integer ratio to 37 or 33 outputs, whose middle output is half a, half b: 2 S = D (a + b),
    a tie, which rounds up"""
    t = np.zeros((N, H, W, 3), dtype=np.uint8)
    for i in range(N):
        for c in range(3):
            a, b = 10 + 3 * i + c, 201 - 2 * i + 2 * c + (i + c) % 2
            b += (a + b + 1) % 2
            t[i, :, :75, c], t[i, :, 75:, c] = a, b
    win = np.array([(i, 50, i % 8, 47, 50) for i in range(N)], dtype=np.int32)      # (the sides are the TILE's: the edge stays a column)
    return t, win


# ---- 1. raw bytes: every output form, the extreme tiles and the ties ------------------------------------------------------------------------
def test_raw_bytes_every_output_form_extremes_and_ties():
    rng = np.random.RandomState(17)
    cpu = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    flat = np.stack([np.full((H, W, 3), 255 if t % 2 == 0 else 0, dtype=np.uint8) for t in range(N)])
    edge, ewin = _edge_batch()
    # the inputs do what they were built for (on the CPU): the ties are there, 255 stays 255
    for t in (0, 1):
        y0, x0, d, wh, ww, nu, nv = clamp_window(ewin[t], H, W, *SIZE)
        b, S = resample_ref(edge[t, y0:y0 + wh, x0:x0 + ww], nu, nv)
        D = wh * ww
        assert ww % nv != 0 and nv % ww != 0 and ((2 * S[:, nv // 2]) % (2 * D) == D).all()              # 2 S = D (mod 2 D) down a column
        assert (b[:, nv // 2, 0] == (int(edge[t, 0, 0, 0]) + int(edge[t, 0, 150, 0]) + 1) // 2).all()
    want_flat = want_view(flat, WIN, SIZE)
    assert all((want_flat[t] == (255 if t % 2 == 0 else 0)).all() for t in range(N))
    for tiles, win, size in ((cpu, WIN, SIZE), (flat, WIN, SIZE), (edge, ewin, SIZE), (cpu, WIN16, SIZE16)):
        dev = _dev_tiles(torch.from_numpy(tiles), 1)
        want = torch.from_numpy(want_view(tiles, win, size))
        bound = (int(win[:, 3].max()), int(win[:, 4].max()))
        got = _view(dev, win, size, 7, resize=BOUND)
        assert torch.equal(got, want)
        assert torch.equal(_view(dev, win, size, 7, resize=bound), want)                  # the tightest bound: fewer workgroups, same bits
        assert torch.equal(_view(dev, torch.from_numpy(win).cuda(), size, 7, resize=BOUND), want)      # the windows on the device
        view = stainlib_amd.TileView(size, scale=(0.08, 1))
        for fmt in _formats():
            wt = fmt.convert(want.cuda()).cpu()
            for off in (0, 1):
                assert _same_bits(_view(dev, win, size, 7, fmt=fmt, out_off=off, resize=BOUND), wt), f"{fmt} out+{off}"
            x, win2 = fmt.convert(dev, view=view, windows=win)
            assert win2 is win and tuple(x.shape) == (N, 3, *size) and _same_bits(x.cpu(), wt), f"{fmt}"
            assert x.is_contiguous(memory_format=torch.channels_last if fmt.channels_last else torch.contiguous_format)
    assert len({got[t].numpy().tobytes() for t in range(N)}) == N


# ---- 2. device against device: the identity is the view, 2x and 4x windows are the box shrink -----------------------------------------------
def test_identity_2x_and_4x_windows_are_todays_views():
    from stainlib_amd import engine
    dev = _batch()
    M, mc, ab = _stats(N)
    Mt, mct = so.M_TRUE_TGT, np.array([1.9, 1.1])
    routes = [dict(), dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct), dict(M_src=M, maxC_src=mc, alpha_beta=ab, augment_background=True)]
    for s in (1, 2, 4):
        size = SIZES[s]
        win3 = _shrink_windows(s)
        sides = np.array([(s * size[1], s * size[0]) if d & 1 else (s * size[0], s * size[1]) for d in win3[:, 2]], dtype=np.int32)
        win5 = np.concatenate([win3, sides], axis=1)
        for kw in routes:
            for fmt in (None, F16):
                want = engine.normalize_view(dev, win3, size, 7, fmt=fmt, shrink=s, **kw)
                got = engine.normalize_view(dev, win5, size, 7, fmt=fmt, resize=BOUND, **kw)
                assert _same_bits(got.cpu(), want.cpu()), f"s={s} {sorted(kw)} {fmt}"


# ---- 3. the routes: apply, the two jitters, hed= ---------------------------------------------------------------------------------------------
def test_routes_against_the_definition_on_the_full_image():
    dev = _batch()
    view = stainlib_amd.TileView(SIZE, scale=(0.08, 1))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    full, Mf, mcf, stf = nz.transform_batch(dev)
    assert int(stf[8]) != 0 and stf[:8].cpu().tolist() == [0] * 8 and torch.equal(full[8], dev[8])     # the white tile: its own bytes
    for fmt in (None, F16):
        x, M, mc, st, win2 = nz.transform_batch(dev, tensor_format=fmt, view=view, windows=WIN)
        assert win2 is WIN and torch.equal(st, stf) and torch.equal(M[:8], Mf[:8]) and torch.equal(mc[:8], mcf[:8])
        assert _same_bits(x.cpu(), _want(full, WIN, SIZE, fmt)), f"transform_batch {fmt}"
    ab = _stats(N)[2]
    for bg in (False, True):
        full = nz.augment_batch(dev, ab, augment_background=bg)[0]
        for fmt in (None, F16):
            x, _, _, st, _ = nz.augment_batch(dev, ab, augment_background=bg, tensor_format=fmt, view=view, windows=WIN)
            assert torch.equal(st, stf) and _same_bits(x.cpu(), _want(full, WIN, SIZE, fmt)), f"augment_batch bg={bg} {fmt}"
    aug = stainlib_amd.HedLightColorAugmenter()
    rng = np.random.RandomState(3)
    sig, bia = rng.uniform(-0.03, 0.03, (N, 3)), rng.uniform(-0.03, 0.03, (N, 3))
    h8, applied = aug.transform_batch(nz.augment_batch(dev, ab)[0], sig, bia)            # the chain at source resolution
    assert 1 in applied.cpu().tolist()
    for fmt in (None, F16):
        x, _, _, _, win2, draw = nz.augment_batch(dev, ab, hed=aug, hed_sigmas=sig, hed_biases=bia, tensor_format=fmt, view=view, windows=WIN)
        assert win2 is WIN and torch.equal(draw.applied, applied)                        # the cutoff sums are the whole tile's
        assert _same_bits(x.cpu(), _want(h8, WIN, SIZE, fmt)), f"augment_batch(hed=) {fmt}"
    h8, applied = aug.transform_batch(dev, sig, bia)                                     # HED on raw tiles
    assert set(applied.cpu().tolist()) == {0, 1}                                         # (the white tile fails the cutoff)
    for fmt in (None, F16):
        x, applied_v, _ = aug.transform_batch(dev, sig, bia, tensor_format=fmt, view=view, windows=WIN)
        assert torch.equal(applied_v, applied) and _same_bits(x.cpu(), _want(h8, WIN, SIZE, fmt)), f"transform_batch {fmt}"


# ---- 4. device windows out of range are clamped as documented ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size,bound", [(SIZE, BOUND), (SIZE, (60, 100)), ((4, 4), BOUND)])
def test_device_windows_out_of_range_equal_the_clamped_host_windows(size, bound):
    from stainlib_amd import engine
    dev = _batch()
    wild = np.array([(-1, -1, 0, 40, 40), (10 ** 9, 10 ** 9, 1, 50, 60), (-2 ** 31, 2 ** 31 - 1, 2, 0, 30), (2 ** 31 - 1, -2 ** 31, 3, 30, -5),
                     (70, 3, 4, 82, 152), (3, 140, 5, 2 ** 31 - 1, 2 ** 31 - 1), (16, 80, 6, -2 ** 31, 7), (5, 100, 7, 81, 151),
                     (100, 5, 3 | 8, 33, 37)], dtype=np.int64).astype(np.int32)
    clamped = np.array([clamp_window(r, H, W, *size, 7, bound)[:5] for r in wild], dtype=np.int32)
    if size == (4, 4):
        assert (clamped[:, 3:] <= 64).all() and (clamped[[4, 5, 7], 3:] == 64).all()    # a ratio above 16 comes down to 16
    else:
        assert (clamped[4, 3], clamped[4, 4]) == (min(81, bound[0]), min(151, bound[1])) and clamped[2, 3] == 1 and clamped[3, 4] == 1
    M, mc, ab = _stats(N)
    routes = [dict(), dict(M_src=M, maxC_src=mc, M_tgt=None, maxC_tgt=None, alpha_beta=ab, augment_background=False)]
    fulls = [dev, engine.normalize_jitter(dev, M, mc, None, None, ab)]
    dwin = torch.from_numpy(wild).cuda()
    for kw, full in zip(routes, fulls):
        for fmt in (None, F16):
            got = _view(dev, dwin, size, 7, fmt=fmt, resize=bound, **kw)
            assert _same_bits(got, _want(full, wild, size, fmt, resize=bound))
            assert _same_bits(got, _view(dev, clamped, size, 7, fmt=fmt, resize=bound, **kw))        # the clamped HOST windows
    with pytest.raises(ValueError, match="windows: tile "):                                         # as host windows they are refused
        engine.normalize_view(dev, wild, size, 7, resize=bound)


# ---- 5. the public API: the default draw is view.draw, where it stands today; the returned windows reproduce the bits ----------------------------
def test_public_api_draws_and_replays():
    dev = _batch()
    view = stainlib_amd.TileView(SIZE, scale=(0.08, 1))
    aug = stainlib_amd.HedLightColorAugmenter()
    mk = stainlib_amd.MacenkoNormalizer()
    mk.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    vh = stainlib_amd.VahadaneNormalizer()
    vh.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1)
    ab = _stats(N)[2]
    jit = lambda: stainlib_amd.StainJitter(0.15, 0.1).draw(N)              # noqa: E731
    hed = lambda: aug.randomize_batch(N)                                   # noqa: E731
    # (call, the draws in front of view.draw, where the windows are in the result, the uint8 chain on the draws and given windows)
    cases = [("convert", lambda **k: F16.convert(dev, **k), [], 1, None),
             ("macenko.transform_batch", lambda **k: mk.transform_batch(dev, **k), [], 4, lambda pre: mk.transform_batch(dev)[0]),
             ("vahadane.transform_batch", lambda **k: vh.transform_batch(dev, **k), [], 4, lambda pre: vh.transform_batch(dev)[0]),
             ("macenko.augment_batch", lambda **k: mk.augment_batch(dev, ab, **k), [], 4, lambda pre: mk.augment_batch(dev, ab)[0]),
             ("vahadane.augment_batch", lambda **k: vh.augment_batch(dev, ab, **k), [], 4, lambda pre: vh.augment_batch(dev, ab)[0]),
             ("StainAugmentor.augment_batch", lambda **k: sa.augment_batch(dev, **k), [jit], 4, lambda pre: sa.augment_batch(dev, pre[0])[0]),
             ("macenko.transform_batch(hed=)", lambda **k: mk.transform_batch(dev, hed=aug, **k), [hed], 4,
              lambda pre: aug.transform_batch(mk.transform_batch(dev)[0], *pre[0])[0]),
             ("vahadane.augment_batch(hed=)", lambda **k: vh.augment_batch(dev, ab, hed=aug, **k), [hed], 4,
              lambda pre: aug.transform_batch(vh.augment_batch(dev, ab)[0], *pre[0])[0]),
             ("StainAugmentor.augment_batch(hed=)", lambda **k: sa.augment_batch(dev, hed=aug, **k), [jit, hed], 4,
              lambda pre: aug.transform_batch(sa.augment_batch(dev, pre[0])[0], *pre[1])[0]),
             ("HedColorAugmenter.transform_batch", lambda **k: aug.transform_batch(dev, **k), [], 2,
              lambda pre: aug.transform_batch(dev)[0])]
    for i, (name, call, pre_draws, at, chain) in enumerate(cases):
        np.random.seed(100 + i)
        res = call(view=view)
        after = np.random.uniform()
        np.random.seed(100 + i)
        pre = [d() for d in pre_draws]
        wd = view.draw(N, H, W)
        assert np.random.uniform() == after, name                                       # the draws, in today's order, and nothing else
        assert np.array_equal(res[at], wd) and res[at].shape == (N, 5) and res[at].dtype == np.int32, name
        assert tuple(res[0].shape) == ((N, 3, *SIZE) if name == "convert" else (N, *SIZE, 3)), name
        if chain is not None:                                                           # the definition on the chain's full-tile image
            assert torch.equal(res[0].cpu(), _want(chain(pre), wd, SIZE)), name
        else:
            assert _same_bits(res[0].cpu(), _want(dev, wd, SIZE, F16)), name
        # the returned windows, passed back, reproduce the bits (the drawn HED and jitter values with them)
        kw = {}
        if jit in pre_draws:
            kw["alpha_beta"] = pre[pre_draws.index(jit)]
        if hed in pre_draws:
            kw["hed_sigmas"], kw["hed_biases"] = pre[pre_draws.index(hed)]
        again = call(view=view, windows=res[at], **kw)
        assert again[at] is res[at] and _same_bits(again[0].cpu(), res[0].cpu()), name

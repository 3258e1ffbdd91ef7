"""-m gpu: the elastic view (the affine view plus a smooth displacement field) inside the view pass: sl_normalize_view_elastic,
sl_view_planes_elastic and TileElastic through the calls that take it.

The definition under test (include/stainlib_hip.h; stainlib_amd.tile_view.elastic_resample / elastic_nearest in numpy): the affine
view's (Y, X) moved by the quadratic B-spline of a control lattice of displacements in 1/256 source pixel; from (Y, X) on everything
is the affine view's.  Integer arithmetic on bytes: every comparison is exact.

Shapes: N = 6 tiles of 96 x 80, outputs (40, 56) and (70, 70), cells of 16 outputs -- the 70 x 70 output has 2 x 2 patches at the
identity with max_d = 8 (patch edge 47) and 3 x 3 at the row-sum limit (24), and a lattice of 7 x 7 nodes."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import engine
from stainlib_amd.tile_view import (AFFINE_MAX_R, AFFINE_Q as Q, ElasticWindows, affine_row_sums, elastic_check_field, elastic_grid_shape,
                                    elastic_nearest, elastic_resample)
from tests.test_gpu_jitter import _dev_tiles, _same_bits, _stats
from tests.test_gpu_view_affine import FILL, FORMATS, H, N, SIZES, W, _raw_tiles, _rot, _row, _rows

pytestmark = pytest.mark.gpu

CELL = 16


def _fields(size, seed=0):
    """three fields per call of N tiles: zero; random within +-256 * 3; a +-2048 sign pattern -> [(field, max_d)]"""
    shape = (N,) + elastic_grid_shape(size, CELL) + (2,)
    rng = np.random.RandomState(100 + seed)
    return [(np.zeros(shape, dtype=np.int32), 0), (rng.randint(-768, 769, shape).astype(np.int32), 3),
            ((2048 * rng.choice((-1, 1), shape)).astype(np.int32), 8)]


def _want(full, win, field, size, fmt=None, fill=FILL):
    u8 = torch.from_numpy(np.stack([elastic_resample(full[t], win[t], field[t], size, CELL, fill) for t in range(len(win))]))
    return u8 if fmt is None else fmt.convert(u8.cuda()).cpu()


def _elastic(dev, win, field, size, fmt=None, max_r=AFFINE_MAX_R, max_d=8, fill=FILL, **route):
    return engine.normalize_view_elastic(dev, win, field, size, CELL, max_r, max_d, fill, fmt=fmt, **route).cpu()


# ---- 1. raw bytes: every matrix of the affine list under three fields, every output form ---------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_raw_route_every_matrix_three_fields_every_output_form(size):
    tiles = _raw_tiles()
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    rows = _rows(size)
    for k in range(0, 18, N):
        win = rows[k:k + N]
        tight = max(1, int(affine_row_sums(win).max()))
        for field, md in _fields(size, k):
            want = _want(tiles, win, field, size)
            for fmt in FORMATS:
                got = _elastic(dev, win, field, size, fmt)
                wt = want if fmt is None else fmt.convert(want.cuda()).cpu()
                assert _same_bits(got, wt), f"rows {k}..{k + N - 1} max_d {md} {fmt}"
            # the tightest bounds (fewer, larger patches where the matrices and the field allow) and both parts on the device: the same bits
            assert torch.equal(_elastic(dev, win, field, size, max_r=tight, max_d=md), want), f"rows {k}.. tight {tight} {md}"
            assert torch.equal(_elastic(dev, torch.from_numpy(win).cuda(), torch.from_numpy(field).cuda(), size), want)
    # the fields do something: under the sign pattern the identity's view is not the affine one
    win = rows[:N]
    assert not torch.equal(_want(tiles, win, _fields(size, 0)[2][0], size), _want(tiles, win, _fields(size, 0)[0][0], size))


# ---- 2. a zero field is the affine view, on every route ----------------------------------------------------------------------------------------
def test_a_zero_field_is_the_affine_view_on_every_route_and_a_failed_fit():
    tiles = np.stack([so.synth_tile(H, W, 70 + 7 * i) for i in range(N)])
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    M, mc, ab = _stats(N)
    M = M.copy()
    M[3] = np.nan                                                                               # a failed fit: the view of its own bytes
    Mt, mct = so.M_TRUE_TGT, np.array([1.9, 1.4])
    size = SIZES[1]
    win = _rows(size)[[0, 9, 10, 11, 14, 15]]
    zero = np.zeros((N,) + elastic_grid_shape(size, CELL) + (2,), dtype=np.int32)
    routes = {"raw": {},
              "apply": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct),
              "jitter-tissue": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=False),
              "jitter-all": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=True)}
    outs = {}
    for name, route in routes.items():
        for fmt in (None, FORMATS[1]):
            want = engine.normalize_view_affine(dev, win, size, AFFINE_MAX_R, FILL, fmt=fmt, **route).cpu()
            for md in (0, 8):                                                                   # (another patch edge, the same bits)
                assert _same_bits(_elastic(dev, win, zero, size, fmt, max_d=md, **route), want), f"{name} {fmt} max_d {md}"
            if fmt is None:
                outs[name] = want
    assert not torch.equal(outs["raw"], outs["apply"]) and not torch.equal(outs["apply"], outs["jitter-tissue"])
    assert not torch.equal(outs["jitter-tissue"], outs["jitter-all"])
    # a non-zero field on the jitter route: the view of the image the same call writes without a view
    field = _fields(size, 7)[1][0]
    full = engine.normalize_jitter(dev, M, mc, Mt, mct, ab, augment_background=False).cpu().numpy()
    assert np.array_equal(full[3], tiles[3]) and not np.array_equal(full[2], tiles[2])
    assert torch.equal(_elastic(dev, win, field, size, max_d=3, **routes["jitter-tissue"]), _want(full, win, field, size))


# ---- 3. a device field beyond the bound is clamped; a matrix beyond max_r fills its tile ---------------------------------------------------------
def test_device_fields_are_clamped_and_a_matrix_beyond_the_bound_fills_its_tile():
    tiles = _raw_tiles()
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    size = SIZES[1]
    shape = (N,) + elastic_grid_shape(size, CELL) + (2,)
    rng = np.random.RandomState(9)
    field = rng.randint(-4096, 4097, shape).astype(np.int64)
    field[0].reshape(-1)[::3] = -(2**31)
    field[0].reshape(-1)[1::3] = 2**31 - 1
    field[1] = rng.choice((-(2**31), 2**31 - 1), shape[1:])
    field = field.astype(np.int32)
    win = np.array([_row(H / 2, W / 2, *_rot(20)) for _ in range(N)], dtype=np.int32)
    win[4, 2:] = (Q, 0, 0, Q)
    win[5, 2:] = (Q // 2, 0, 0, Q // 2)
    with pytest.raises(ValueError, match="tile 0 .* control displacement"):
        engine.normalize_view_elastic(dev, win, field, size, CELL, AFFINE_MAX_R, 8, FILL)
    dwin, dfield = torch.from_numpy(win).cuda(), torch.from_numpy(field).cuda()
    fill = torch.tensor(FILL, dtype=torch.uint8)
    for md in (0, 2, 8):
        clamped = np.clip(field, -256 * md, 256 * md)
        elastic_check_field(clamped, N, size, CELL, md)
        want = _want(tiles, win, clamped, size)
        assert torch.equal(_elastic(dev, dwin, dfield, size, max_d=md), want), f"max_d {md}"
        # a smaller max_r than one tile needs fills that tile only: the rotated tiles have row sums of ~1.28 Q, the identity exactly Q
        want[:4] = fill
        for fmt in (None, FORMATS[1]):
            got = _elastic(dev, dwin, dfield, size, fmt, max_r=Q, max_d=md)
            assert _same_bits(got, want if fmt is None else fmt.convert(want.cuda()).cpu()), f"max_d {md} max_r Q {fmt}"
        assert not (want[4] == fill).all()


# ---- 4. companion planes: every element size through the windows an image call returned -------------------------------------------------------
@pytest.mark.parametrize("dtype,fill", [(torch.uint8, 7), (torch.float16, -2.5), (torch.int32, -100), (torch.int64, -(2**40) - 3)])
@pytest.mark.parametrize("c", [1, 3])
def test_planes_every_element_size_through_an_image_calls_windows(dtype, fill, c):
    size = SIZES[1]
    view = stainlib_amd.TileElastic(size, zoom=(0.8, 1.3), shear=(-8, 8), translate=(0.3, 0.3), fill=FILL, magnitude=(2, 4), cell=CELL)
    dev = _dev_tiles(torch.from_numpy(_raw_tiles()), 0)
    np.random.seed(5)
    fmt = FORMATS[1]
    x, win = fmt.convert(dev, view=view)
    assert isinstance(win, ElasticWindows) and win.affine.shape == (N, 6) and win.field.shape == (N, 7, 7, 2) and tuple(x.shape) == (N, 3, *size)
    rng = np.random.RandomState(3)
    if dtype.is_floating_point:
        planes = torch.from_numpy(rng.standard_normal((N, c, H, W)).astype(np.float32)).to(dtype)
    else:
        info = torch.iinfo(dtype)
        planes = torch.from_numpy(rng.randint(info.min, info.max, (N, c, H, W), dtype=np.int64)).to(dtype)
    planes = planes if c == 3 else planes[:, 0]
    got = view.apply(planes.cuda(), win, fill=fill).cpu()
    assert got.dtype == dtype and tuple(got.shape) == ((N, c) if c == 3 else (N,)) + size
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[planes.element_size()]
    pl, fl = planes.view(bits).numpy(), torch.tensor([fill], dtype=dtype).view(bits).numpy()[0]
    pl = pl if c == 3 else pl[:, None]
    want = np.stack([np.stack([elastic_nearest(pl[t, k], win.affine[t], win.field[t], size, CELL, fl) for k in range(c)]) for t in range(N)])
    want = want if c == 3 else want[:, 0]
    assert np.array_equal(got.view(bits).numpy(), want)
    assert (want == fl).any() and (want != fl).any()
    # both parts on the device, and a tile beyond the call's bound: all fill
    dwin = ElasticWindows(torch.from_numpy(win.affine).cuda(), torch.from_numpy(win.field).cuda())
    assert torch.equal(view.apply(planes.cuda(), dwin, fill=fill).cpu(), got)
    one = engine.view_planes_elastic(planes.cuda(), dwin.affine, dwin.field, size, CELL, 1, 4, fill=fill).cpu()
    assert (one.view(bits).numpy() == fl).all()


def test_a_label_plane_and_its_image_use_the_same_coordinates():
    """a one-hot image -- 255 in every channel where the 0/1 label is set -- and its label plane, both with fill 0.  With ty = Y - Q/2 the
    label's nearest element (Y >> 16, X >> 16) IS the tap (ky + (fy >= 128), kx + (fx >= 128)) of the image's four, the one with the
    largest weight, at least 128 x 128 of 65536.  A blend is 255 only if every clear tap weighs at most 128 of 65536 (255 w <= 32768), and 0
    only if every set tap does: so wherever the image view is 255 the label view is 1 and wherever it is 0 the label view is 0 -- if and
    only if both went through the same (Y, X) to within the weights' resolution."""
    size = SIZES[1]
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.stack([(((yy // (5 + t)) + (xx // (7 + t))) & 1) for t in range(N)]).astype(np.uint8)          # blocks of 5 x 7 and more
    img = np.repeat((255 * label)[..., None], 3, axis=-1).astype(np.uint8)
    view = stainlib_amd.TileElastic(size, zoom=(0.9, 1.2), magnitude=(3, 4), cell=CELL, fill=0)
    np.random.seed(8)
    win = view.draw(N, H, W)
    got_img = engine.normalize_view_elastic(torch.from_numpy(img).cuda(), win.affine, win.field, size, CELL, view.bound, view.max_d, 0).cpu().numpy()
    got_lab = view.apply(torch.from_numpy(label).cuda(), win, fill=0).cpu().numpy()
    assert np.array_equal(got_lab, np.stack([elastic_nearest(label[t], win.affine[t], win.field[t], size, CELL, 0) for t in range(N)]))
    full, none = (got_img == 255).all(axis=-1), (got_img == 0).all(axis=-1)
    assert (got_lab[full] == 1).all() and full.sum() > full.size // 8
    assert (got_lab[none] == 0).all() and none.sum() > none.size // 8
    assert (~full & ~none).any()                                                          # (edges between blocks blend)


# ---- 5. the public calls on 64 x 64 tiles: draw, replay, convert, apply, and the refused combinations ---------------------------------------
def _undrawn(call, match):
    np.random.seed(11)
    before = np.random.get_state()
    with pytest.raises(ValueError, match=match):
        call()
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_public_calls_draw_replay_convert_apply_and_refuse():
    tiles = np.stack([so.synth_tile(64, 64, s) for s in (2, 3, 4, 5)])
    dev = torch.from_numpy(tiles).cuda()
    n = 4
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    view = stainlib_amd.TileElastic(48, zoom=(0.8, 1.2), shear=(-10, 10), translate=0.1, fill=FILL, magnitude=(1, 4), cell=CELL)
    fmt = FORMATS[1]
    ab = stainlib_amd.StainJitter(0.2, 0.2).draw(n)
    full, Mf, _, _ = nz.augment_batch(dev, ab)

    def want_of(full_u8, win):
        return torch.from_numpy(np.stack([elastic_resample(full_u8[t], win.affine[t], win.field[t], (48, 48), CELL, FILL) for t in range(n)]))

    np.random.seed(32)
    x, M, _, st, win = nz.augment_batch(dev, ab, tensor_format=fmt, view=view)
    np.random.seed(32)
    again = view.draw(n, 64, 64)
    assert isinstance(win, ElasticWindows) and np.array_equal(win.affine, again.affine) and np.array_equal(win.field, again.field)
    assert torch.equal(M, Mf) and (st == 0).all() and win.field.any()
    want = want_of(full.cpu().numpy(), win)
    assert _same_bits(x.cpu(), fmt.convert(want.cuda()).cpu())
    x2, _, _, _, win2 = nz.augment_batch(dev, ab, tensor_format=fmt, view=view, windows=win)                 # the replay
    assert win2 is win and _same_bits(x2.cpu(), x.cpu())
    # view.apply follows it: a label plane through the same windows
    labels = torch.from_numpy(np.random.RandomState(1).randint(0, 5, (n, 64, 64)).astype(np.int64))
    got = view.apply(labels.cuda(), win, fill=255).cpu().numpy()
    assert np.array_equal(got, np.stack([elastic_nearest(labels[t].numpy(), win.affine[t], win.field[t], (48, 48), CELL, 255) for t in range(n)]))
    # transform_batch, the uint8 image; Vahadane; StainAugmentor (alpha_beta drawn BEFORE the windows)
    full_t = nz.transform_batch(dev)[0]
    xt, _, _, _, _ = nz.transform_batch(dev, view=view, windows=win)
    assert torch.equal(xt.cpu(), want_of(full_t.cpu().numpy(), win))
    vz = stainlib_amd.VahadaneNormalizer()
    vz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    xv, _, _, _, _ = vz.augment_batch(dev, ab, view=view, windows=win)
    assert torch.equal(xv.cpu(), want_of(vz.augment_batch(dev, ab)[0].cpu().numpy(), win))
    sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1)
    np.random.seed(33)
    xs, _, _, _, win_s = sa.augment_batch(dev, view=view)
    np.random.seed(33)
    ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
    again = view.draw(n, 64, 64)
    assert np.array_equal(win_s.affine, again.affine) and np.array_equal(win_s.field, again.field)
    assert torch.equal(xs.cpu(), want_of(sa.augment_batch(dev, ab2)[0].cpu().numpy(), win_s))
    # the raw route: convert(view=) behind any uint8 result gives the same bits
    xc, win_c = fmt.convert(full_t, view=view, windows=win)
    assert win_c is win and _same_bits(xc.cpu(), fmt.convert(want_of(full_t.cpu().numpy(), win).cuda()).cpu())
    assert _same_bits(fmt.convert(full, view=view, windows=win)[0].cpu(), x.cpu())
    # the refused combinations name the view and draw nothing
    hed = stainlib_amd.HedLightColorAugmenter()
    _undrawn(lambda: nz.augment_batch(dev, ab, view=view, hed=hed), "affine view")
    _undrawn(lambda: nz.transform_batch(dev, view=view, hsb=stainlib_amd.HsbLightColorAugmenter()), "affine view")
    _undrawn(lambda: nz.transform_batch(dev, view=view, blur=stainlib_amd.GaussianBlurAugmenter((0.5, 1.5))), "affine view")
    _undrawn(lambda: hed.transform_batch(dev, view=view), "affine view")
    _undrawn(lambda: nz.separate_batch(dev, view=view), "affine view")
    rz = stainlib_amd.ReinhardStainNormalizer()
    rz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    _undrawn(lambda: rz.transform_batch(dev, view=view), "affine view")
    _undrawn(lambda: stainlib_amd.LuminosityStandardizer.standardize_batch(dev, view=view), "affine view")
    _undrawn(lambda: nz.augment_batch(dev, ab, view=view, windows=win.affine), "ElasticWindows")
    _undrawn(lambda: nz.augment_batch(dev, ab, view=stainlib_amd.TileAffine(48), windows=win), "ElasticWindows of an elastic view")
    _undrawn(lambda: nz.augment_batch(dev, ab, view=stainlib_amd.TileView(48), windows=win), "ElasticWindows of an elastic view")
    _undrawn(lambda: nz.augment_batch(dev, ab, view=view, windows=ElasticWindows(torch.from_numpy(win.affine).cuda(), win.field)), "same side")

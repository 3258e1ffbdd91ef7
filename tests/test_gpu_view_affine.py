"""-m gpu: the affine view (rotation by any angle, zoom, shear, translation) inside the view pass: sl_normalize_view_affine,
sl_view_planes_affine and TileAffine through the calls that take it.

The definition under test (include/stainlib_hip.h; stainlib_amd.tile_view.affine_resample / affine_nearest in numpy): windows[t] =
(cy, cx, a00, a01, a10, a11) in 2^-16 source pixels; with `full` the uint8 image the same call writes WITHOUT view=, output pixel (i, j)
is the 8-bit-weight bilinear blend of the four taps of full[t] around (Y, X), a tap outside the tile the fill byte; a tensor is
TensorFormat.convert of that byte; a companion plane takes the element at (Y >> 16, X >> 16).  Integer arithmetic on bytes: every
comparison is exact.

Shapes: tiles of 96 x 80, outputs (40, 56) and (70, 70) -- the second has two patches per axis even at the largest patch edge (63) and
3 x 3 at the row-sum limit (32)."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import engine
from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_check_windows, affine_nearest, affine_resample, affine_row_sums
from tests.test_gpu_jitter import MEAN, STD, _dev_tiles, _same_bits, _stats

pytestmark = pytest.mark.gpu

N, H, W = 6, 96, 80
SIZES = ((40, 56), (70, 70))
FILL = (10, 30, 200)
FORMATS = (None,
           stainlib_amd.TensorFormat(dtype=torch.float16, mean=MEAN, std=STD),
           stainlib_amd.TensorFormat(dtype=torch.bfloat16, channels_last=True, mean=MEAN, std=STD),
           stainlib_amd.TensorFormat(dtype=torch.float32, mean=MEAN, std=STD))
# the dihedral code d as a signed permutation matrix (a00, a01, a10, a11) / Q: rot90(flip_w(window) if d & 4 else window, d & 3)
DIHEDRAL = {0: (1, 0, 0, 1), 1: (0, 1, -1, 0), 2: (-1, 0, 0, -1), 3: (0, -1, 1, 0), 4: (1, 0, 0, -1), 5: (0, 1, 1, 0), 6: (-1, 0, 0, 1),
            7: (0, -1, -1, 0)}


def _row(cy, cx, a00, a01, a10, a11):
    return [int(np.rint(Q * v)) for v in (cy, cx, a00, a01, a10, a11)]


def _dihedral_row(y0, x0, d, size, s=1):
    """the affine row of the plain view (y0, x0, d) under the shrink s: the centre on the window's centre, s times the permutation"""
    oh, ow = size
    wh, ww = (s * ow, s * oh) if d & 1 else (s * oh, s * ow)
    return [(2 * y0 + wh) * Q // 2, (2 * x0 + ww) * Q // 2] + [s * Q * v for v in DIHEDRAL[d]]


def _rot(deg, z=1.0):
    c, s = np.cos(np.radians(deg)) / z, np.sin(np.radians(deg)) / z
    return (c, -s, s, c)


def _rows(size):
    """one matrix per tile: 18 rows, three calls of six tiles"""
    rows = [_row(H / 2, W / 2, 1, 0, 0, 1)]                                                    # the identity about the centre
    rows += [_dihedral_row(5 + d, 3 + d, d, size) for d in range(8)]                            # the eight dihedral matrices
    rows += [_row(H / 2, W / 2, *_rot(30)), _row(H / 2, W / 2, *_rot(45)),
             _row(H / 2, W / 2, 1, -1, 1, 1),                                                   # 45 degrees at 1 / z = sqrt 2: the limit, b = 32
             _row(H / 2 + 0.5, W / 2 + 0.25, 1, 0, 0, 1),                                       # a fractional centre: fy = 128, fx = 64 (tile 0: ties)
             _row(H / 3, W / 3, 0, 0, 0, 0),                                                    # the zero matrix: a constant
             _row(H / 2, W / 2, 1, 0.4, 0.1, 0.9),                                              # a shear
             _row(0.25, W / 2 + 0.3701, *_rot(-17, 1.1)),                                       # half outside, a fractional centre, rotated
             _row(-300.0, W / 2, *_rot(10)),                                                    # wholly outside
             _row(H / 2, W + 0.5, 2, 0, 0, 2)]                                                  # the 2 x 2 box, half outside
    assert len(rows) == 18
    win = np.array(rows, dtype=np.int64)
    assert (affine_row_sums(win) <= AFFINE_MAX_R).all() and int(affine_row_sums(win).max()) == AFFINE_MAX_R
    return win.astype(np.int32)


def _raw_tiles():
    """random bytes; tile 0 a 0 / 255 checkerboard (every blend of the extremes, ties at half weights), tile 1 all 255, tile 2 all 0"""
    t = np.random.RandomState(7).randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    t[0] = (255 * ((yy + xx) & 1))[..., None]
    t[1], t[2] = 255, 0
    return t


def _want(full, win, size, fmt=None, fill=FILL):
    u8 = torch.from_numpy(np.stack([affine_resample(full[t], win[t], size, fill) for t in range(len(win))]))
    return u8 if fmt is None else fmt.convert(u8.cuda()).cpu()


def _affine(dev, win, size, fmt=None, max_r=AFFINE_MAX_R, fill=FILL, **route):
    return engine.normalize_view_affine(dev, win, size, max_r, fill, fmt=fmt, **route).cpu()


# ---- 1. raw bytes: every matrix of the list, every output form ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_raw_route_every_matrix_every_output_form(size):
    tiles = _raw_tiles()
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    rows = _rows(size)
    # the inputs do what they were built for: on the checkerboard of tile 0 row 12 blends 0 and 255 to 127.5 everywhere -- a tie, which
    # rounds up --, row 0 (the identity) keeps both extremes
    assert (affine_resample(tiles[0], rows[12], size, FILL) == 128).all()
    assert set(np.unique(affine_resample(tiles[0], rows[0], size, FILL)).tolist()) == {0, 255}
    for k in range(0, 18, N):
        win = rows[k:k + N]
        want = _want(tiles, win, size)
        for fmt in FORMATS:
            got = _affine(dev, win, size, fmt)
            wt = want if fmt is None else fmt.convert(want.cuda()).cpu()
            assert _same_bits(got, wt), f"rows {k}..{k + N - 1} {fmt}"
        # the tightest bound (fewer, larger patches where the matrices allow) and the windows on the device: the same bits
        tight = max(1, int(affine_row_sums(win).max()))
        assert torch.equal(_affine(dev, win, size, max_r=tight), want)
        assert torch.equal(_affine(dev, torch.from_numpy(win).cuda(), size), want)
    # wholly outside is the fill, the zero matrix a constant
    out = _want(tiles, rows[12:18], size)
    assert (out[4] == torch.tensor(FILL, dtype=torch.uint8)).all() and len(out[1].reshape(-1, 3).unique(dim=0)) == 1


# ---- 2. the apply and jitter routes: the view of the image the same call writes without a view ---------------------------------------------
def test_apply_and_jitter_routes_and_a_failed_fit():
    tiles = np.stack([so.synth_tile(H, W, 70 + 7 * i) for i in range(N)])
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    M, mc, ab = _stats(N)
    M = M.copy()
    M[3] = np.nan                                                                               # a failed fit: the view of its own bytes
    Mt, mct = so.M_TRUE_TGT, np.array([1.9, 1.4])
    size = SIZES[1]
    win = _rows(size)[[0, 9, 10, 11, 14, 15]]
    routes = {"apply": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct),
              "jitter-tissue": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=False),
              "jitter-all": dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=True),
              "jitter-own": dict(M_src=M, maxC_src=mc, alpha_beta=ab, augment_background=False)}
    fulls = {}
    for name, route in routes.items():
        if "alpha_beta" in route:
            full = engine.normalize_jitter(dev, route["M_src"], route["maxC_src"], route.get("M_tgt"), route.get("maxC_tgt"), ab,
                                           augment_background=route["augment_background"]).cpu().numpy()
        else:
            full = engine.normalize_apply(dev, M, mc, Mt, mct).cpu().numpy()
        fulls[name] = full
        assert np.array_equal(full[3], tiles[3]) and not np.array_equal(full[2], tiles[2])
        want = _want(full, win, size)
        assert torch.equal(_affine(dev, win, size, **route), want), name
        fmt = FORMATS[1]
        assert _same_bits(_affine(dev, win, size, fmt, **route), fmt.convert(want.cuda()).cpu()), name
    assert not np.array_equal(fulls["jitter-tissue"], fulls["jitter-all"]) and not np.array_equal(fulls["apply"], fulls["jitter-tissue"])


# ---- 3. device against device: dihedral matrices and 2 I are today's views ------------------------------------------------------------------
def test_dihedral_matrices_and_2I_are_todays_views():
    tiles = np.stack([so.synth_tile(H, W, 90 + 3 * i) for i in range(8)])
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    M, mc, ab = _stats(8)
    Mt, mct = so.M_TRUE_TGT, np.array([1.9, 1.4])
    route = dict(M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, alpha_beta=ab, augment_background=False)
    for size in SIZES:
        win3 = np.array([(5 + d, 3 + d, d) for d in range(8)], dtype=np.int32)
        win6 = np.array([_dihedral_row(5 + d, 3 + d, d, size) for d in range(8)], dtype=np.int32)
        for r in ({}, route):
            for fmt in (None, FORMATS[2]):
                want = engine.normalize_view(dev, win3, size, 7, fmt=fmt, **r).cpu()
                assert _same_bits(_affine(dev, win6, size, fmt, **r), want), f"{size} {fmt} {'route' if r else 'raw'}"
    size = (40, 33)                                                                             # 2 I: an 80 x 66 window (66 x 80 turned)
    win3 = np.array([(d, 0 if d & 1 else 2 * d, d) for d in range(8)], dtype=np.int32)
    win6 = np.array([_dihedral_row(y0, x0, d, size, s=2) for y0, x0, d in win3.tolist()], dtype=np.int32)
    for r in ({}, route):
        want = engine.normalize_view(dev, win3, size, 7, shrink=2, **r).cpu()
        assert torch.equal(_affine(dev, win6, size, **r), want)


# ---- 4. windows on the device: the centre is clamped, a matrix beyond the bound fills its tile --------------------------------------------
def test_device_windows_are_clamped_and_a_matrix_beyond_the_bound_fills_its_tile():
    tiles = _raw_tiles()
    dev = _dev_tiles(torch.from_numpy(tiles), 1)
    size = SIZES[0]
    slack = 1 << 28
    win = np.array([_row(H / 2, W / 2, *_rot(20)) for _ in range(N)], dtype=np.int64)
    win[0, 0], win[0, 1] = -(1 << 30), W * Q + slack + 12345                                    # centres out of range: clamped
    win[1, 0], win[1, 1] = 2**31 - 1, -(2**31)
    win[2, 2:] = (Q, Q + 1, 0, Q)                                                               # a row sum of 2 Q + 1: fill everywhere
    win[3, 2:] = (-(2**31), 2**31 - 1, -(2**31), -(2**31))
    win[4, 2:] = (Q, 0, 0, Q)
    clamped = win.copy()
    clamped[:, 0] = np.clip(win[:, 0], -slack, H * Q + slack)
    clamped[:, 1] = np.clip(win[:, 1], -slack, W * Q + slack)
    clamped[2, 2:] = clamped[3, 2:] = 0
    clamped[2, :2] = clamped[3, :2] = -slack                                                    # (a constant outside the tile: the fill)
    with pytest.raises(ValueError, match="centre"):
        engine.normalize_view_affine(dev, win.astype(np.int32)[:2].repeat(3, axis=0), size, AFFINE_MAX_R, FILL)
    with pytest.raises(ValueError, match="row sum"):
        engine.normalize_view_affine(dev, win.astype(np.int32), size, AFFINE_MAX_R, FILL)
    want = _want(tiles, clamped, size)
    got = _affine(dev, torch.from_numpy(win.astype(np.int32)).cuda(), size)
    assert torch.equal(got, want)
    fill = torch.tensor(FILL, dtype=torch.uint8)
    assert (got[2] == fill).all() and (got[3] == fill).all() and not (got[4] == fill).all()
    # a smaller max_r than one tile needs fills that tile only: the rotated tiles have row sums of ~1.28 Q, the identity exactly Q
    win = np.array([_row(H / 2, W / 2, *_rot(20)) for _ in range(N)], dtype=np.int32)
    win[4, 2:] = (Q, 0, 0, Q)
    win[5, 2:] = (Q // 2, 0, 0, Q // 2)
    want = _want(tiles, win, size)
    want[:4] = fill
    for fmt in (None, FORMATS[1]):
        got = _affine(dev, torch.from_numpy(win).cuda(), size, fmt, max_r=Q)
        assert _same_bits(got, want if fmt is None else fmt.convert(want.cuda()).cpu())


# ---- 5. companion planes: every element size through the windows an image call returned ---------------------------------------------------
@pytest.mark.parametrize("dtype,fill", [(torch.uint8, 7), (torch.float16, -2.5), (torch.int32, -100), (torch.int64, -(2**40) - 3)])
@pytest.mark.parametrize("c", [1, 3])
def test_planes_every_element_size_through_an_image_calls_windows(dtype, fill, c):
    size = SIZES[1]
    view = stainlib_amd.TileAffine(size, zoom=(0.8, 1.3), shear=(-8, 8), translate=(0.3, 0.3), fill=FILL)
    dev = _dev_tiles(torch.from_numpy(_raw_tiles()), 0)
    np.random.seed(5)
    fmt = FORMATS[1]
    x, win = fmt.convert(dev, view=view)
    assert win.shape == (N, 6) and win.dtype == np.int32 and tuple(x.shape) == (N, 3, *size)
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
    want = np.stack([np.stack([affine_nearest(pl[t, k], win[t], size, fl) for k in range(c)]) for t in range(N)])
    want = want if c == 3 else want[:, 0]
    assert np.array_equal(got.view(bits).numpy(), want)
    assert (want == fl).any() and (want != fl).any()
    # the windows on the device, and a tile beyond the call's bound: all fill
    assert torch.equal(view.apply(planes.cuda(), torch.from_numpy(win).cuda(), fill=fill).cpu(), got)
    one = engine.view_planes_affine(planes.cuda(), torch.from_numpy(win).cuda(), size, 1, fill=fill).cpu()
    assert (one.view(bits).numpy() == fl).all()


# ---- 6. the public calls on 64 x 64 tiles: draw, replay, convert, and the refused combinations -------------------------------------------
def _undrawn(call, match):
    np.random.seed(11)
    before = np.random.get_state()
    with pytest.raises(ValueError, match=match):
        call()
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_public_calls_draw_replay_convert_and_refuse():
    tiles = np.stack([so.synth_tile(64, 64, s) for s in (2, 3, 4, 5)])
    dev = torch.from_numpy(tiles).cuda()
    n = 4
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    view = stainlib_amd.TileAffine(48, zoom=(0.8, 1.2), shear=(-10, 10), translate=0.1, fill=FILL)
    fmt = FORMATS[1]
    ab = stainlib_amd.StainJitter(0.2, 0.2).draw(n)
    full, Mf, _, _ = nz.augment_batch(dev, ab)
    np.random.seed(32)
    x, M, _, st, win = nz.augment_batch(dev, ab, tensor_format=fmt, view=view)
    np.random.seed(32)
    assert np.array_equal(win, view.draw(n, 64, 64)) and torch.equal(M, Mf) and (st == 0).all()
    affine_check_windows(win, n, 64, 64, 48, view.bound)
    want = _want(full.cpu().numpy(), win, (48, 48))
    assert _same_bits(x.cpu(), fmt.convert(want.cuda()).cpu())
    x2, _, _, _, win2 = nz.augment_batch(dev, ab, tensor_format=fmt, view=view, windows=win)               # the replay
    assert win2 is win and _same_bits(x2.cpu(), x.cpu())
    # transform_batch, the uint8 image; Vahadane; StainAugmentor (alpha_beta drawn BEFORE the windows)
    full_t = nz.transform_batch(dev)[0]
    xt, _, _, _, _ = nz.transform_batch(dev, view=view, windows=win)
    assert torch.equal(xt.cpu(), _want(full_t.cpu().numpy(), win, (48, 48)))
    vz = stainlib_amd.VahadaneNormalizer()
    vz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    xv, _, _, _, _ = vz.augment_batch(dev, ab, view=view, windows=win)
    assert torch.equal(xv.cpu(), _want(vz.augment_batch(dev, ab)[0].cpu().numpy(), win, (48, 48)))
    sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1)
    np.random.seed(33)
    xs, _, _, _, win_s = sa.augment_batch(dev, view=view)
    np.random.seed(33)
    ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
    assert np.array_equal(win_s, view.draw(n, 64, 64))
    assert torch.equal(xs.cpu(), _want(sa.augment_batch(dev, ab2)[0].cpu().numpy(), win_s, (48, 48)))
    # the raw route: convert(view=) behind any uint8 result
    xc, win_c = fmt.convert(full_t, view=view, windows=win)
    assert win_c is win and _same_bits(xc.cpu(), fmt.convert(_want(full_t.cpu().numpy(), win, (48, 48)).cuda()).cpu())
    # the refused combinations name the affine view and draw nothing
    hed = stainlib_amd.HedLightColorAugmenter()
    _undrawn(lambda: nz.augment_batch(dev, ab, view=view, hed=hed), "affine view")
    _undrawn(lambda: nz.transform_batch(dev, view=view, hed=hed), "affine view")
    _undrawn(lambda: sa.augment_batch(dev, view=view, hed=hed), "affine view")
    _undrawn(lambda: hed.transform_batch(dev, view=view), "affine view")
    _undrawn(lambda: nz.separate_batch(dev, view=view), "affine view")
    rz = stainlib_amd.ReinhardStainNormalizer()
    rz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    _undrawn(lambda: rz.transform_batch(dev, view=view), "affine view")
    _undrawn(lambda: stainlib_amd.LuminosityStandardizer.standardize_batch(dev, view=view), "affine view")
    _undrawn(lambda: stainlib_amd.TileView(48).apply(torch.zeros((n, 64, 64), dtype=torch.int64, device="cuda"), win), "affine view")
    _undrawn(lambda: nz.augment_batch(dev, ab, view=view, windows=win[:, :5]), "affine view")

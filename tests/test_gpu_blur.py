"""-m gpu: Gaussian blur in the view pass (sl_normalize_blur_view, engine.normalize_blur_view, GaussianBlurAugmenter, blur= on the batch
methods and on TensorFormat.convert).

The definition is in integers on bytes (stainlib_amd/augmentation/blur.py: blur_reference), so every comparison is array_equal.  Every
expected value is built the same way: blur_reference (numpy) of the image the SAME call writes without blur= and without a view, then the
numpy view functions of stainlib_amd/tile_view.py (view_planes_reference: crop, box shrink, flip, quarter turns), then
TensorFormat.convert of those bytes."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import engine
from stainlib_amd.augmentation.blur import IDENTITY, blur_codes, blur_reference, codes_ok, codes_radius, effective_codes
from stainlib_amd.tile_view import view_planes_reference

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# the uint8 image, float16 NCHW, float32 NHWC, bfloat16 NCHW
FORMATS = (None,
           stainlib_amd.TensorFormat(dtype=torch.float16, mean=MEAN, std=STD),
           stainlib_amd.TensorFormat(dtype=torch.float32, channels_last=True, mean=MEAN, std=STD),
           stainlib_amd.TensorFormat(dtype=torch.bfloat16, mean=MEAN, std=STD))
BITS = {torch.uint8: torch.uint8, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
N, H, W = 5, 96, 80
# radii 0, 1, 3, 8, 8: three rows from sigmas, and two of the full radius -- no sigma <= 8 / 3 reaches w_8 >= 1 (256 g_8 < 1/2), so these
# are written out: a near-box and the codes of sigma = 2.5 with their last unit moved out to w_8
R8 = np.array([[16, 15, 15, 15, 15, 15, 15, 15, 15], [40, 38, 30, 20, 11, 6, 2, 0, 1]], dtype=np.int32)
CODES = np.concatenate([blur_codes([0.0, 0.3, 1.0]), R8]).astype(np.int32)
ROUTE_NAMES = ("raw", "apply", "jitter_tissue", "jitter_all")
_CACHE = {}


def _same_bits(got, want):
    """equal as integer views, element by element in logical order"""
    got, want = got.cpu(), want.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.contiguous().view(BITS[got.dtype]).numpy(),
                                                                                  want.contiguous().view(BITS[want.dtype]).numpy())


def _setup():
    """four synthetic H&E tiles and an all-white one whose fit fails (a few bright bytes in it, so that a blur of its own bytes shows), their
    fit, a target, a jitter draw, the codes"""
    if "setup" not in _CACHE:
        t = np.stack([so.synth_tile(H, W, 60 + 7 * i) for i in range(N - 1)] + [np.full((H, W, 3), 255, dtype=np.uint8)])
        t[4, 30:50, 20:45] = (250, 240, 245)
        t[4, 0:3, 70:80] = (251, 249, 244)
        dev = torch.from_numpy(t).cuda()
        M, mc, st = engine.macenko_fit(dev)[:3]
        Mt, mct, stt = engine.macenko_fit(torch.from_numpy(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT)[None]).cuda())[:3]
        assert st.cpu().tolist()[:4] == [0] * 4 and int(st[4]) != 0 and int(stt[0]) == 0
        np.random.seed(3)
        ab = stainlib_amd.StainJitter(0.3, 0.2).draw(N)
        codes = CODES
        assert codes_radius(codes).tolist() == [0, 1, 3, 8, 8] and codes_ok(codes).all()
        routes = {"raw": {},
                  "apply": dict(M_src=M, maxC_src=mc, M_tgt=Mt[0], maxC_tgt=mct[0]),
                  "jitter_tissue": dict(M_src=M, maxC_src=mc, M_tgt=Mt[0], maxC_tgt=mct[0], alpha_beta=ab, augment_background=False),
                  "jitter_all": dict(M_src=M, maxC_src=mc, M_tgt=Mt[0], maxC_tgt=mct[0], alpha_beta=ab, augment_background=True)}
        _CACHE["setup"] = (dev, routes, codes)
    return _CACHE["setup"]


def _full(dev, route):
    """the image the call writes without blur= and without a view: the full-tile view, code 0 -> numpy (n, h, w, 3)"""
    n = dev.shape[0]
    return engine.normalize_view(dev, np.zeros((n, 3), dtype=np.int32), None, 0, **route).cpu().numpy()


def _blurred(name):
    """blur_reference of the route's full image under the tiles' codes, computed once and left unchanged"""
    key = ("blurred", name)
    if key not in _CACHE:
        dev, routes, codes = _setup()
        full = _full(dev, routes[name])
        if name != "raw":
            assert np.array_equal(full[4], dev[4].cpu().numpy()) and not np.array_equal(full[0], dev[0].cpu().numpy())   # the failed fit: its own bytes
        b = np.stack([blur_reference(full[t], codes[t]) for t in range(N)])
        assert np.array_equal(b[0], full[0]) and not np.array_equal(b[4], full[4])
        b.setflags(write=False)
        _CACHE[key] = b
    return _CACHE[key]


def _view_np(blurred, win, size, shrink=1):
    """the numpy view of blurred bytes (n, h, w, 3) -> (n, oh, ow, 3) uint8"""
    planes = np.ascontiguousarray(blurred.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(view_planes_reference(planes, win, size, shrink=shrink, mode="area").transpose(0, 2, 3, 1))


def _expect(blurred, win, size, fmt, shrink=1):
    want = torch.from_numpy(_view_np(blurred, win, size, shrink)).cuda()
    return want if fmt is None else fmt.convert(want)


def _windows(oh, ow, s, first, h=H, w=W, n=N, allowed=tuple(range(8))):
    """n windows that touch the top, bottom, left and right edge of the tile and one interior, with the codes allowed[first], allowed[first
    + 1], ... (cyclically)"""
    win = np.empty((n, 3), dtype=np.int32)
    for t in range(n):
        d = allowed[(first + t) % len(allowed)]
        wh, ww = (s * ow, s * oh) if d & 1 else (s * oh, s * ow)
        ymax, xmax = h - wh, w - ww
        assert ymax >= 0 and xmax >= 0
        win[t] = [(0, xmax // 2), (ymax, xmax // 3), (ymax // 2, 0), (ymax // 3, xmax), (ymax // 2 | 1, xmax // 2 | 1)][t % 5] + (d,)
        win[t, 0], win[t, 1] = min(win[t, 0], ymax), min(win[t, 1], xmax)
    return win


def _check(name, size, shrink=1):
    dev, routes, codes = _setup()
    blurred = _blurred(name)
    oh, ow = (size, size) if isinstance(size, int) else size
    seen = set()
    for first in (0, 3):                                           # the codes 0 .. 4 and 3 .. 7: every dihedral code
        win = _windows(oh, ow, shrink, first)
        seen |= set(win[:, 2].tolist())
        for fmt in FORMATS:
            got = engine.normalize_blur_view(dev, win, size, 7, codes, fmt=fmt, shrink=shrink, **routes[name])
            want = _expect(blurred, win, (oh, ow), fmt, shrink)
            assert tuple(got.shape) == ((N, oh, ow, 3) if fmt is None else (N, 3, oh, ow))
            assert _same_bits(got, want), (name, size, shrink, first, fmt)
    assert seen == set(range(8))


# ---- 1. every route, every code, the four edges, two sizes, four formats -------------------------------------------------------------------
@pytest.mark.parametrize("size", [40, (33, 47)])
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_blurred_view_is_the_view_of_the_blurred_image(name, size):
    _check(name, size)


@pytest.mark.parametrize("shrink,size", [(2, 20), (4, 10)])
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_box_shrink_acts_on_the_blurred_bytes(name, shrink, size):
    _check(name, size, shrink)


# ---- 2. tiles smaller than a block or than the radius ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,crop,d_mask", [(40, 52, (33, 36), 7), (3, 70, (3, 33), 6), (1, 70, (1, 33), 6)])
def test_tiles_smaller_than_a_block_or_the_radius(h, w, crop, d_mask):
    n = 4
    t = np.random.RandomState(h).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    dev = torch.from_numpy(t).cuda()
    codes = np.concatenate([R8, R8[:1], blur_codes([2.0])]).astype(np.int32)
    assert codes_radius(codes).tolist()[:3] == [8, 8, 8]
    blurred = np.stack([blur_reference(t[k], codes[k]) for k in range(n)])
    for size in (None, crop):                                     # without and with a crop
        oh, ow = (h, w) if size is None else size
        dm = d_mask if size is not None else 6                   # (the full tile does not fit transposed)
        win = _windows(oh, ow, 1, 1, h, w, n, allowed=tuple(d for d in range(8) if d & ~dm == 0))
        for fmt in FORMATS[:2]:
            got = engine.normalize_blur_view(dev, win, size, dm, codes, fmt=fmt)
            assert _same_bits(got, _expect(blurred, win, (oh, ow), fmt)), (h, w, size, fmt)
            got8 = engine.normalize_blur_view(dev, win, size, dm, codes, max_r=8, fmt=fmt)      # the bound above a tile's own radius
            assert _same_bits(got8, got)


# ---- 3. seams between patches: 7 x 7 patches of 48 with ragged last ones -----------------------------------------------------------------------
def test_full_tile_view_of_300_by_301_has_no_seams():
    h, w = 300, 301
    rs = np.random.RandomState(11)
    t = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    t[1] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[..., None] // np.array([1, 2, 3]) % 256).astype(np.uint8)     # ramps: a seam shows as a step
    dev = torch.from_numpy(t).cuda()
    codes = R8
    blurred = np.stack([blur_reference(t[k], codes[k]) for k in range(2)])
    win = np.array([[0, 0, 0], [0, 0, 4]], dtype=np.int32)
    # the full-tile view: the blurred tile itself, tile 1 flipped along the width (view_planes_reference's rule at the tile's own size,
    # written out: its exact area average is a 300 x 300 integer matrix product per plane, a minute here)
    want8 = torch.from_numpy(np.stack([blurred[0], blurred[1][:, ::-1]])).cuda()
    for fmt in FORMATS[:2]:
        got = engine.normalize_blur_view(dev, win, None, 6, codes, max_r=8, fmt=fmt)
        assert _same_bits(got, want8 if fmt is None else fmt.convert(want8)), fmt
    # the result does not depend on how the patches cut the output: a crop whose patches start elsewhere gives the same pixels
    crop = np.array([[17, 29, 0], [17, 29, 0]], dtype=np.int32)
    got = engine.normalize_blur_view(dev, crop, (250, 260), 6, codes, max_r=8)
    assert np.array_equal(got.cpu().numpy(), blurred[:, 17:267, 29:289])


# ---- 4. the identity, a constant image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["raw", "jitter_all"])
def test_identity_codes_under_the_bound_8_give_normalize_view_bit_for_bit(name):
    dev, routes, _ = _setup()
    ident = np.tile(np.array(IDENTITY, dtype=np.int32), (N, 1))
    for shrink, size in ((1, (33, 47)), (2, 20)):
        win = _windows(*((size, size) if isinstance(size, int) else size), shrink, 2)
        for fmt in FORMATS:
            got = engine.normalize_blur_view(dev, win, size, 7, ident, max_r=8, fmt=fmt, shrink=shrink, **routes[name])
            want = engine.normalize_view(dev, win, size, 7, fmt=fmt, shrink=shrink, **routes[name])
            assert _same_bits(got, want), (name, shrink, fmt)


def test_a_constant_image_stays_constant():
    t = np.empty((3, 70, 90, 3), dtype=np.uint8)
    t[0], t[1], t[2] = (0, 255, 1), (255, 254, 128), (7, 0, 255)
    dev = torch.from_numpy(t).cuda()
    got = engine.normalize_blur_view(dev, np.zeros((3, 3), dtype=np.int32), None, 0, blur_codes([8.0 / 3.0, 1.0, 0.5]))
    assert np.array_equal(got.cpu().numpy(), t)


# ---- 5. device-resident windows and codes ------------------------------------------------------------------------------------------------------
def test_device_windows_are_clamped_and_invalid_device_codes_give_the_identity_without_a_sync():
    dev, routes, _ = _setup()
    good3, good1, r8 = blur_codes(1.0), blur_codes(0.3), blur_codes(2.5)
    bad_sum = good3.copy(); bad_sum[0] -= 1                                    # sum 255
    negative = np.array([258, -1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)       # sums to 256 with a negative weight
    codes = np.stack([good3, bad_sum, negative, r8, good1]).astype(np.int32)   # r8: a weight beyond max_r = 3
    eff = effective_codes(codes, 3)
    assert eff.tolist() == [good3.tolist(), list(IDENTITY), list(IDENTITY), list(IDENTITY), good1.tolist()]
    size = (33, 47)
    inside = _windows(33, 47, 1, 1)
    wild = inside.copy()
    wild[0, :2] = (-7, 10 ** 6); wild[1, :2] = (10 ** 6, -3); wild[3, :2] = (-2 ** 31, 2 ** 31 - 1)
    wild[:, 2] |= 8                                                            # bits the mask drops
    clamped = wild.copy()
    clamped[:, 2] &= 7
    for t in (0, 1, 3):
        wh, ww = (47, 33) if clamped[t, 2] & 1 else (33, 47)
        clamped[t, 0], clamped[t, 1] = np.clip(wild[t, 0], 0, H - wh), np.clip(wild[t, 1], 0, W - ww)
    d_win, d_codes = torch.from_numpy(wild).cuda(), torch.from_numpy(codes).cuda()
    for name in ("raw", "apply"):
        full = _full(dev, routes[name])
        blurred = np.stack([blur_reference(full[t], eff[t].astype(np.int32)) for t in range(N)])
        route = {k: (v.cuda() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v)).cuda() if k == "alpha_beta" else v)
                 for k, v in routes[name].items()}
        out = torch.empty((N, 33, 47, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                # a synchronising torch call raises
        try:
            got = engine.normalize_blur_view(dev, d_win, size, 7, d_codes, max_r=3, out=out, **route)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), _view_np(blurred, clamped, size)), name
    with pytest.raises(ValueError, match="max_r"):
        engine.normalize_blur_view(dev, d_win, size, 7, d_codes)               # device codes are never read back: they need the bound
    with pytest.raises(ValueError, match="rule"):
        engine.normalize_blur_view(dev, inside, size, 7, codes, max_r=8)       # host codes are rule-checked


# ---- 6. the class paths -------------------------------------------------------------------------------------------------------------------------
def _class_batch():
    """five synthetic H&E tiles and an all-white one (no tissue: its fit fails, and its own bytes are blurred)"""
    t = np.stack([so.synth_tile(64, 64, 40 + 7 * i) for i in range(5)] + [np.full((64, 64, 3), 255, dtype=np.uint8)])
    t[5, 10:20, 10:20] = (250, 240, 245)
    return torch.from_numpy(t).cuda()


def _class_expect(u8, draw, view, win, fmt):
    """blur_reference of the call's unblurred uint8 result, the numpy view, the conversion"""
    full = u8.cpu().numpy()
    b = np.stack([blur_reference(full[t], draw.codes[t]) for t in range(full.shape[0])])
    if view is None:
        want = torch.from_numpy(b).cuda()
        return want if fmt is None else fmt.convert(want)
    return _expect(b, win, view.out_size(64, 64), fmt, view.shrink)


def _check_class_path(call, plain, view, fmt, n=6):
    """call(**kw) -> the method's tuple with blur=; plain() -> its unblurred uint8 image.  The draws come before the windows; the returned
    codes and windows reproduce the bits."""
    aug = stainlib_amd.GaussianBlurAugmenter((0.4, 8.0 / 3.0))
    kw = dict(view=view) if view is not None else {}
    np.random.seed(41)
    res = call(blur=aug, tensor_format=fmt, **kw)
    after = np.random.uniform()
    draw = res[-1]
    win = res[-2] if view is not None else None
    assert isinstance(draw, engine.BlurDraw) and draw.codes.shape == (n, 9) and draw.codes.dtype == np.int32
    assert np.array_equal(draw.codes, blur_codes(draw.sigmas))
    want = _class_expect(plain(), draw, view, win, fmt)
    assert _same_bits(res[0], want), (view, fmt)
    back = dict(view=view, windows=win) if view is not None else {}
    again = call(blur=aug, blur_sigmas=draw.sigmas, tensor_format=fmt, **back)          # the sigmas and the windows fed back
    assert _same_bits(again[0], res[0]) and np.array_equal(again[-1].codes, draw.codes)
    again = call(blur=aug, blur_sigmas=draw.codes, tensor_format=fmt, **back)           # the codes fed back
    assert _same_bits(again[0], res[0]) and np.array_equal(again[-1].codes, draw.codes) and again[-1].sigmas is None
    return draw, win, after


VIEWS = (stainlib_amd.TileView(48), stainlib_amd.TileView(24, shrink=2), None)


@pytest.mark.parametrize("bg", [False, True])
def test_macenko_augment_batch_with_blur_view_and_tensor_format(bg):
    dev = _class_batch()
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    np.random.seed(9)
    ab = stainlib_amd.StainJitter().draw(6)
    u8 = nz.augment_batch(dev, ab, augment_background=bg)[0]
    assert torch.equal(u8[5], dev[5])
    for view in VIEWS:
        for fmt in (FORMATS[1], None):
            draw, win, after = _check_class_path(lambda **kw: nz.augment_batch(dev, ab, augment_background=bg, **kw), lambda: u8, view, fmt)
            np.random.seed(41)                                     # the draws: the sigmas first, then the windows
            aug = stainlib_amd.GaussianBlurAugmenter((0.4, 8.0 / 3.0))
            assert np.array_equal(draw.sigmas, aug.randomize_batch(6))
            assert view is None or np.array_equal(win, view.draw(6, 64, 64))
            assert np.random.uniform() == after


def test_vahadane_transform_batch_with_blur():
    dev = _class_batch()
    nz = stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    u8 = nz.transform_batch(dev)[0]
    for view, fmt in ((None, None), (VIEWS[0], FORMATS[3]), (None, FORMATS[2])):
        res_len = len(nz.transform_batch(dev, blur=stainlib_amd.GaussianBlurAugmenter((1, 1)), tensor_format=fmt, **(dict(view=view) if view else {})))
        assert res_len == (6 if view is not None else 5)
        _check_class_path(lambda **kw: nz.transform_batch(dev, **kw), lambda: u8, view, fmt)


def test_stain_augmentor_augment_batch_with_blur():
    dev = _class_batch()
    sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1)
    aug = stainlib_amd.GaussianBlurAugmenter((0.4, 8.0 / 3.0))
    view = VIEWS[0]
    np.random.seed(43)
    x, _, _, _, win, draw = sa.augment_batch(dev, blur=aug, view=view)
    after = np.random.uniform()
    np.random.seed(43)                                             # alpha_beta, then the sigmas, then the windows
    ab = stainlib_amd.StainJitter(0.15, 0.1).draw(6)
    sig = aug.randomize_batch(6)
    assert np.array_equal(draw.sigmas, sig) and np.array_equal(win, view.draw(6, 64, 64)) and np.random.uniform() == after
    s8 = sa.augment_batch(dev, ab)[0]
    assert _same_bits(x, _class_expect(s8, draw, view, win, None))
    for v, fmt in ((view, FORMATS[1]), (None, None), (VIEWS[1], None)):
        _check_class_path(lambda **kw: sa.augment_batch(dev, ab, **kw), lambda: s8, v, fmt)


def test_blur_augmenter_transform_batch_and_convert():
    dev = _class_batch()
    aug = stainlib_amd.GaussianBlurAugmenter((0.4, 8.0 / 3.0))
    np.random.seed(5)
    sig = aug.randomize_batch(6)
    codes = blur_codes(sig)
    draw = engine.BlurDraw(sig, codes)
    for view in VIEWS:
        for fmt in (None, FORMATS[1], FORMATS[2]):
            if view is None:
                out, c = aug.transform_batch(dev, sig, tensor_format=fmt)
                win = None
            else:
                np.random.seed(21)
                out, c, win = aug.transform_batch(dev, sig, view=view, tensor_format=fmt)
                after = np.random.uniform()
                np.random.seed(21)                                 # only the windows are drawn
                assert np.array_equal(win, view.draw(6, 64, 64)) and np.random.uniform() == after
                out2, _, win2 = aug.transform_batch(dev, sig, view=view, windows=win, tensor_format=fmt)
                assert win2 is win and _same_bits(out2, out)
            assert np.array_equal(c, codes)
            assert _same_bits(out, _class_expect(dev, draw, view, win, fmt)), (view, fmt)
            if fmt is not None:                                    # TensorFormat.convert(view=, blur=): the same pass
                res = fmt.convert(dev, blur=aug, blur_sigmas=sig, **(dict(view=view, windows=win) if view is not None else {}))
                assert len(res) == (3 if view is not None else 2) and np.array_equal(res[-1].codes, codes) and _same_bits(res[0], out)
                res = fmt.convert(dev, blur=aug, blur_sigmas=codes, **(dict(view=view, windows=win) if view is not None else {}))
                assert _same_bits(res[0], out)
    # the default sigmas: the augmenter's current one for every tile; transform() of one patch is the numpy definition
    out, c = aug.transform_batch(dev)
    assert np.array_equal(c, np.tile(blur_codes(aug._sigma), (6, 1)))
    assert np.array_equal(out[2].cpu().numpy(), aug.transform(dev[2].cpu().numpy()))
    # convert draws the sigmas, then the windows
    fmt, view = FORMATS[1], VIEWS[0]
    np.random.seed(77)
    x, win, d = fmt.convert(dev, view=view, blur=aug)
    after = np.random.uniform()
    np.random.seed(77)
    assert np.array_equal(d.sigmas, aug.randomize_batch(6)) and np.array_equal(win, view.draw(6, 64, 64)) and np.random.uniform() == after
    assert _same_bits(x, _class_expect(dev, d, view, win, fmt))

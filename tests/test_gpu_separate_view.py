"""-m gpu: stain separation in the view pass (sl_stain_separate_view, engine.stain_separate_view, separate_batch(view=, windows=,
tensor_format=)).

The definition under test (include/stainlib_hip.h, sl_stain_separate_view) is "the same bits, elsewhere": with full = what
sl_stain_separate writes for the whole tiles,
    an image   rot90(flip_w_if(d & 4, full.X[t][y0:y0+wh, x0:x0+ww]), d & 3); with shrink = s the box means of the s-times-larger window
               (stainlib_amd.tile_view.area_resample of those bytes), then the flip and the turn; under a format its fmt.convert
    conc       the same slice, flip and turn of each plane of full.conc[t], a permutation of elements
so every comparison is exact (torch.equal on bit patterns): the yardstick is engine.stain_separate's / TensorFormat.convert's full-tile
result, sliced with torch or numpy.  Every call of _sv writes into buffers with sentinel elements before and after each wanted output,
and whole sentinel buffers stand by for the outputs that are not wanted; all are checked after the call.  Tiles and per-tile-distinct
statistics: the recipe of tests/test_gpu_jitter.py.  The kernel's patch is 64 / shrink output pixels square."""
import ctypes as C

import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import _ffi
from stainlib_amd.tile_view import area_resample
from tests.gpu_util import to_dev
from tests.test_gpu_jitter import M_TGT, M_TGT_NEG, MAXC_TGT, SENTINEL, _dev_tiles, _formats, _same_bits, _stats, _tiles

pytestmark = pytest.mark.gpu

B = 64
FIELDS = ("norm", "h", "e", "conc")
IMAGES = FIELDS[:3]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
_CACHE = {}


def _targets(regime):
    """(the regime of tests.test_gpu_jitter._stats, M_tgt, maxC_tgt): "he" and "neg" take the branch-free and the general lasso under the
    H&E target; "tneg" is a target with a negative entry (values pass 255: the wrapping cast); "own" is no target"""
    return {"he": ("he", M_TGT, MAXC_TGT), "neg": ("neg", M_TGT, MAXC_TGT), "tneg": ("he", M_TGT_NEG, np.array([2.4, 1.0])),
            "own": ("he", None, None), "own_neg": ("neg", None, None)}[regime]


def _full(key, dev, M, mc, Mt, mct, conc_dtype):
    """engine.stain_separate on the whole tiles -> Separated of CPU tensors, computed once per case and never changed"""
    from stainlib_amd import engine
    key = ("full", key, conc_dtype)
    if key not in _CACHE:
        _CACHE[key] = stainlib_amd.Separated(*(t.cpu() for t in engine.stain_separate(dev, M, mc, Mt, mct, conc_dtype=conc_dtype)))
    return _CACHE[key]


def _ref(full, win, oh, ow, d_mask, shrink=1):
    """the definition on a channels-last full-tile tensor (n, h, w, c): clamp, slice, box means, flip along the width, then rot90 --
    _ref of tests/test_gpu_view.py with the window `shrink` times the output"""
    n, h, w, c = full.shape
    s = shrink
    outs = []
    for t, (y0, x0, d) in enumerate(np.asarray(win).tolist()):
        d &= d_mask
        k = d & 3
        wh, ww = (ow, oh) if k & 1 else (oh, ow)
        y0, x0 = min(max(y0, 0), h - s * wh), min(max(x0, 0), w - s * ww)
        v = full[t][y0:y0 + s * wh, x0:x0 + s * ww]
        if s != 1:
            assert v.dtype == torch.uint8
            v = torch.from_numpy(area_resample(v.numpy(), wh, ww))
        if d & 4:
            v = torch.flip(v, dims=(1,))
        v = torch.rot90(v, k, dims=(0, 1))
        assert tuple(v.shape) == (oh, ow, c)
        outs.append(v)
    return torch.stack(outs).contiguous()


def _want_of(full, win, oh, ow, d_mask, want, fmt=None, shrink=1):
    """what the view call must return for `want`, from the full-tile Separated"""
    res = {}
    for name in FIELDS:
        if name not in want:
            res[name] = None
        elif name == "conc":
            res[name] = _ref(full.conc.permute(0, 2, 3, 1), win, oh, ow, d_mask).permute(0, 3, 1, 2).contiguous()
        else:
            u8 = _ref(getattr(full, name), win, oh, ow, d_mask, shrink)
            res[name] = u8 if fmt is None else fmt.convert(u8.cuda()).cpu()
    return stainlib_amd.Separated(**res)


def _sv(dev, win, size, d_mask, M, mc, Mt=None, mct=None, want=FIELDS, conc_dtype=torch.float32, fmt=None, shrink=1, out_off=0):
    """engine.stain_separate_view into guarded buffers -> Separated of CPU tensors.  All four output buffers exist, filled with SENTINEL and
    16 bytes longer at either end; only the wanted ones are handed over (out_off elements past an aligned address); everything outside
    the wanted bodies must still hold SENTINEL afterwards."""
    from stainlib_amd import engine
    n = dev.shape[0]
    oh, ow = size
    bufs, outs = {}, {}
    for name in FIELDS:
        dt = conc_dtype if name == "conc" else (fmt.dtype if fmt is not None else torch.uint8)
        numel = n * (2 if name == "conc" else 3) * oh * ow
        esize = torch.empty((), dtype=dt).element_size()
        start = 16 // esize + out_off
        buf = torch.full((start + numel + 16 // esize,), SENTINEL, dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        bufs[name] = (buf, start, numel)
        body = buf[start:start + numel]
        if name == "conc":
            view = body.view(n, 2, oh, ow)
        elif fmt is None:
            view = body.view(n, oh, ow, 3)
        elif fmt.channels_last:
            view = body.view(n, oh, ow, 3).permute(0, 3, 1, 2)
        else:
            view = body.view(n, 3, oh, ow)
        outs[name] = view if name in want else None
    res = engine.stain_separate_view(dev, win, size, M, mc, Mt, mct, d_mask=d_mask, want=want, conc_dtype=conc_dtype, fmt=fmt,
                                     out=stainlib_amd.Separated(**outs), shrink=shrink)
    torch.cuda.synchronize()
    got = {}
    for k, name in enumerate(FIELDS):
        buf, start, numel = bufs[name]
        host = buf.cpu()
        if name not in want:
            assert res[k] is None and bool((host == SENTINEL).all()), f"want={want}: the unrequested {name} buffer was written"
            got[name] = None
            continue
        assert res[k] is outs[name]
        outside = torch.cat([host[:start], host[start + numel:]])
        assert bool((outside == SENTINEL).all()), f"{tuple(dev.shape)} -> {size} want={want} fmt={fmt} out+{out_off}: written outside {name}"
        got[name] = outs[name].cpu()
    return stainlib_amd.Separated(**got)


def _assert_same(got, want, label):
    for name, g, w in zip(FIELDS, got, want):
        assert (g is None) == (w is None), f"{label}: {name}"
        if g is not None:
            assert _same_bits(g, w), f"{label}: {name} differs"


def _check(key, dev, win, size, d_mask, regime, want=FIELDS, conc_dtype=torch.float32, fmt=None, shrink=1, out_off=0, label=""):
    n = dev.shape[0]
    stats_regime, Mt, mct = _targets(regime)
    M, mc, _ = _stats(n, stats_regime)
    full = _full((key, regime), dev, M, mc, Mt, mct, conc_dtype)
    got = _sv(dev, win, size, d_mask, M, mc, Mt, mct, want=want, conc_dtype=conc_dtype, fmt=fmt, shrink=shrink, out_off=out_off)
    _assert_same(got, _want_of(full, win, *size, d_mask, want, fmt, shrink),
                 f"{label} {tuple(dev.shape)} -> {size} mask {d_mask} s={shrink} {regime} want={want} {conc_dtype} {fmt} out+{out_off}")


def _windows(n, h, w, oh, ow, d_mask, shrink=1):
    """n distinct in-range windows cycling through the codes d_mask allows: the four corners of the code's range first, then corners
    in between with odd and even x0 (_windows of tests/test_gpu_view.py, the window `shrink` times the output)"""
    codes = [c for c in range(8) if c & ~d_mask == 0]
    win = []
    for t in range(n):
        d = codes[t % len(codes)]
        wh, ww = (ow, oh) if d & 1 else (oh, ow)
        ymax, xmax = h - shrink * wh, w - shrink * ww
        win.append(([(0, 0), (0, xmax), (ymax, 0), (ymax, xmax)][t] if t < 4 else ((2 * t + 1) % (ymax + 1), (t - 1) % (xmax + 1))) + (d,))
    assert len(set(win)) == n
    return np.array(win, dtype=np.int32)


# ---- 1. outputs smaller than a patch from a tiny tile: every want, every plane type, every image form, both output alignments -----------
@pytest.mark.parametrize("size,d_mask", [((5, 7), 6), ((5, 5), 7)])
def test_tiny_tiles_every_want_type_and_format(size, d_mask):
    n, h, w = 8, 9, 11
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = _windows(n, h, w, *size, d_mask)
    for want in [(f,) for f in FIELDS] + [FIELDS]:
        for fmt in ([None] + _formats()) if set(want) & set(IMAGES) else [None]:
            for cdt in DTYPES if "conc" in want else DTYPES[:1]:
                for off in (0, 1):
                    _check("tiny", dev, win, size, d_mask, "he", want=want, conc_dtype=cdt, fmt=fmt, out_off=off)
    _check("tiny", dev, win, size, d_mask, "neg", conc_dtype=torch.bfloat16, fmt=_formats()[2])
    _check("tiny", dev, win, size, d_mask, "own", want=("e", "conc"))


# ---- 2. ragged last patches in both directions, more than one patch each way, all eight codes in one batch -----------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_ragged_patches_all_codes_in_one_batch(off):
    """(2B+3) x (B-1) out of a square tile just large enough for the transposed window; the input at an aligned address and one byte
    past it; windows at all four corners and at x0 of all four residues mod 4; per-tile-distinct statistics; both lasso forms and
    both casts"""
    n, h, oh, ow = 8, 2 * B + 3, 2 * B + 3, B - 1
    dev = _dev_tiles(_tiles(n, h, h), off)
    assert dev.data_ptr() % 4 == off
    key = ("ragged", off)
    win = np.array([(0, 0, 0), (68, 0, 1), (0, 1, 2), (67, 0, 3), (0, 2, 4), (3, 0, 5), (0, 3, 6), (0, 0, 7)], dtype=np.int32)
    assert sorted(win[:, 2].tolist()) == list(range(8)) and {int(x) % 4 for x in win[::2, 1]} == {0, 1, 2, 3}
    f = _formats()
    _check(key, dev, win, (oh, ow), 7, "he", label=f"+{off}")
    _check(key, dev, win, (oh, ow), 7, "he", conc_dtype=torch.float16, fmt=f[3], label=f"+{off}")
    _check(key, dev, win, (oh, ow), 7, "neg", label=f"+{off}")
    _check(key, dev, win, (oh, ow), 7, "tneg", label=f"+{off}")
    _check(key, dev, win, (oh, ow), 7, "tneg", conc_dtype=torch.bfloat16, fmt=f[0], out_off=1, label=f"+{off}")
    # the other corners of every code's range, without a target; and the other orientation of the output
    win2 = np.array([(0, 68, 0), (0, 0, 1), (0, 67, 2), (1, 0, 3), (0, 5, 4), (66, 0, 5), (0, 66, 6), (68, 0, 7)], dtype=np.int32)
    _check(key, dev, win2, (oh, ow), 7, "own", label=f"+{off} other corners")
    _check(key, dev, win2, (oh, ow), 7, "own_neg", want=("h", "conc"), conc_dtype=torch.float16, fmt=f[4], label=f"+{off} other corners")
    win3 = win2[:, [1, 0, 2]].copy()
    _check(key, dev, win3, (ow, oh), 7, "he", label=f"+{off} wide output")
    # the whole tile under every code: 3 x 3 patches, the middle one with neighbours on every side
    win4 = np.array([(0, 0, d) for d in range(8)], dtype=np.int32)
    _check(key, dev, win4, (h, h), 7, "he", conc_dtype=torch.float16, fmt=f[2], label=f"+{off} whole tile")
    _check(key, dev, win4, (h, h), 7, "own_neg", label=f"+{off} whole tile")
    _check(key, dev, win3, (ow, oh), 7, "neg", conc_dtype=torch.bfloat16, fmt=f[5], out_off=1, label=f"+{off} wide output")


# ---- 3. the 2x / 4x box shrink of the images -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink,size", [(2, (31, 30)), (2, (33, 40)), (4, (15, 13)), (4, (17, 21))])
def test_shrunk_images_are_the_box_means_of_the_full_tile_bytes(shrink, size):
    """output widths that are no multiple of 4, one ragged patch, and a full 64 / s patch next to a ragged one in both directions;
    compared with area_resample of the full-tile bytes, then flipped and turned, as uint8 and as float16 NCHW"""
    n, h = 8, 2 * B + 3
    dev = _dev_tiles(_tiles(n, h, h), 0)
    win = _windows(n, h, h, *size, 7, shrink)
    for regime in ("he", "tneg"):
        for fmt in (None, _formats()[2]):
            _check(("ragged", 0), dev, win, size, 7, regime, want=IMAGES, fmt=fmt, shrink=shrink)
    _check(("ragged", 0), dev, win, size, 7, "own", want=("e",), shrink=shrink, out_off=1)


def test_a_shrunk_conc_is_refused_from_c_and_from_python():
    from stainlib_amd import engine
    n, h = 2, 16
    dev = _dev_tiles(_tiles(n, h, h), 0)
    M, mc, _ = _stats(n)
    win = np.zeros((n, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="shrink=2 does not go with 'conc'"):
        engine.stain_separate_view(dev, win, (4, 4), M, mc, shrink=2)
    with pytest.raises(ValueError, match="shrink=2 does not go with 'conc'"):
        stainlib_amd.MacenkoNormalizer().separate_batch(dev, normalize=False, view=stainlib_amd.TileView(4, shrink=2))
    conc = torch.full((n, 2, 4, 4), SENTINEL, dtype=torch.float32, device="cuda")
    o = _ffi.default_separate_out()
    o.conc = conc.data_ptr()
    dw, dM, dmc = torch.from_numpy(win).cuda(), torch.as_tensor(M).cuda(), torch.as_tensor(mc).cuda()
    rc = _ffi.lib().sl_stain_separate_view(C.c_void_p(dev.data_ptr()), n, h, h, 4, 4, C.c_void_p(dw.data_ptr()), 7, 2, C.c_void_p(dM.data_ptr()),
                                           C.c_void_p(dmc.data_ptr()), None, None, 0.01, C.byref(o), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and bool((conc == SENTINEL).all())


# ---- 4. tiles whose fit failed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["he", "own"])
def test_failed_tiles_follow_k_separates_rule_under_the_view(regime):
    """NaN M_src in one tile and a non-positive maxC_src in another, in the middle of a batch: norm is the view of the source bytes, h and
    e are white, conc is +0 -- and the neighbours are what they are without the failures"""
    n, h, w, size = 6, 70, 70, (66, 35)                       # two patches down
    cpu = _tiles(n, h, w)
    dev = _dev_tiles(cpu, 0)
    win = _windows(n, h, w, *size, 7)
    _, Mt, mct = _targets(regime)
    M, mc, _ = _stats(n)
    Mf, mcf = M.copy(), mc.copy()
    Mf[2] = np.nan
    mcf[4, 1] = 0.0
    good = _full(("failed", regime, "good"), dev, M, mc, Mt, mct, torch.float32)
    full = _full(("failed", regime), dev, Mf, mcf, Mt, mct, torch.float32)
    src = _ref(cpu, win, *size, 7)
    for fmt, cdt in ((None, torch.float32), (_formats()[1], torch.float16)):
        got = _sv(dev, win, size, 7, Mf, mcf, Mt, mct, conc_dtype=cdt, fmt=fmt)
        conv = (lambda u8: u8) if fmt is None else (lambda u8: fmt.convert(u8.cuda()).cpu())
        white = conv(torch.full((1,) + size + (3,), 255, dtype=torch.uint8))[0]
        for t in (2, 4):
            assert _same_bits(got.norm[t], conv(src)[t]), f"{regime} {fmt}: norm of failed tile {t}"
            assert _same_bits(got.h[t], white) and _same_bits(got.e[t], white), f"{regime} {fmt}: h / e of failed tile {t}"
            assert bool((got.conc[t].view(torch.int32 if cdt == torch.float32 else torch.int16) == 0).all()), f"{regime}: conc of failed tile {t}"
        want_good = _want_of(good, win, *size, 7, FIELDS, fmt)
        for t in (0, 1, 3, 5):                                # the neighbours: untouched by the failures
            for name in IMAGES:
                assert _same_bits(getattr(got, name)[t], getattr(want_good, name)[t]), f"{regime} {fmt}: {name} of tile {t}"
            assert _same_bits(got.conc[t], want_good.conc[t].to(cdt)), f"{regime} {fmt}: conc of tile {t}"
        if cdt == torch.float32:                              # and the whole batch is the view of stain_separate's
            _assert_same(got, _want_of(full, win, *size, 7, FIELDS, fmt), f"failed {regime} {fmt}")


# ---- 5. device windows are clamped and masked by the kernel ---------------------------------------------------------------------------------
def test_device_windows_out_of_range_equal_the_clamped_window():
    """corners far outside the tile (negative, past the end), codes with bits outside d_mask and above bit 2: the result is the clamped,
    masked window's, exactly as _ref of tests/test_gpu_view.py clamps"""
    n, h, w, size = 8, 40, 72, (17, 30)                       # (fits transposed too: 30 <= 40, 17 <= 72)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    win = np.array([(-5, -7, 0), (1000, 1000, 1), (-1, 50, 2), (30, -2, 3), (24, 43, 4 | 8), (2 ** 31 - 1, -2 ** 31, 5 | 64), (-2 ** 31, 2 ** 31 - 1, 6),
                    (23, 42, 7 | 1024)], dtype=np.int64).astype(np.int32)
    dwin = torch.from_numpy(win).cuda()
    M, mc, _ = _stats(n)
    full = _full("clamp", dev, M, mc, M_TGT, MAXC_TGT, torch.float32)
    for d_mask in (7, 6, 4, 0):
        got = _sv(dev, dwin, size, d_mask, M, mc, M_TGT, MAXC_TGT)
        _assert_same(got, _want_of(full, win, *size, d_mask, FIELDS), f"device windows, mask {d_mask}")
    s2 = _sv(dev, dwin, (8, 15), 7, M, mc, M_TGT, MAXC_TGT, want=IMAGES, shrink=2)
    _assert_same(s2, _want_of(full, win, 8, 15, 7, IMAGES, shrink=2), "device windows, shrink 2")


# ---- 6. the batch method ----------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("method", ["macenko", "vahadane"])
def test_separate_batch_with_a_view_is_the_view_of_separate_batch(method):
    tiles = [so.synth_tile(96, 80, 20 + s) for s in range(6)] + [np.full((96, 80, 3), 255, dtype=np.uint8)]
    dev = to_dev(tiles)
    n, h, w = len(tiles), 96, 80
    nz = stainlib_amd.MacenkoNormalizer() if method == "macenko" else stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    view = stainlib_amd.TileView(48)
    w_given = _windows(n, h, w, 48, 48, 7)
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    for normalize in (True, False):
        sep, M, mc, status = nz.separate_batch(dev, normalize=normalize)
        assert status.cpu().tolist()[-1] != 0 and status.cpu().tolist()[:2] == [0, 0]          # the white tile failed
        full = stainlib_amd.Separated(*(t.cpu() for t in sep))
        got, M2, mc2, st2, w_back = nz.separate_batch(dev, normalize=normalize, view=view, windows=w_given)
        assert w_back is w_given and torch.equal(st2, status) and _bits_equal(M2, M) and _bits_equal(mc2, mc)
        _assert_same(stainlib_amd.Separated(*(t.cpu() for t in got)), _want_of(full, w_given, 48, 48, 7, FIELDS), f"{method} normalize={normalize}")
        got, _, _, _, _ = nz.separate_batch(dev, want=("h", "conc"), conc_dtype=torch.float16, normalize=normalize, tensor_format=f16, view=view,
                                            windows=w_given)
        assert got.norm is None and got.e is None
        want = _want_of(full, w_given, 48, 48, 7, ("h", "conc"), f16)
        assert _same_bits(got.h.cpu(), want.h) and _same_bits(got.conc.cpu(), want.conc.to(torch.float16)), f"{method} normalize={normalize} f16"
        # the default windows: view.draw from the global stream, replayed from the same seed
        np.random.seed(77)
        got, _, _, st3, w_drawn = nz.separate_batch(dev, want=("norm", "e"), normalize=normalize, view=view)
        after = np.random.uniform()
        np.random.seed(77)
        assert np.array_equal(w_drawn, view.draw(n, h, w)) and np.random.uniform() == after and torch.equal(st3, status)
        _assert_same(stainlib_amd.Separated(*(t.cpu() if t is not None else None for t in got)),
                     _want_of(full, w_drawn, 48, 48, 7, ("norm", "e")), f"{method} normalize={normalize} drawn")
    # a shrinking view: the images at half the magnification
    got, _, _, _, w2 = nz.separate_batch(dev, want=IMAGES, view=stainlib_amd.TileView(40, shrink=2), windows=_windows(n, h, w, 40, 40, 7, 2))
    sep = stainlib_amd.Separated(*(t.cpu() for t in nz.separate_batch(dev)[0]))
    _assert_same(stainlib_amd.Separated(*(t.cpu() if t is not None else None for t in got)), _want_of(sep, w2, 40, 40, 7, IMAGES, shrink=2),
                 f"{method} shrink 2")


# ---- 7. the identity view ---------------------------------------------------------------------------------------------------------------------
def test_the_identity_view_is_separate_batch():
    tiles = [so.synth_tile(96, 80, 20 + s) for s in range(2)] + [np.full((96, 80, 3), 255, dtype=np.uint8)]
    dev = to_dev(tiles)
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    sep, M, mc, status = nz.separate_batch(dev)
    got, M2, mc2, st2, win = nz.separate_batch(dev, view=stainlib_amd.TileView(None, flip=False, rot90=False))
    assert np.array_equal(win, np.zeros((3, 3), dtype=np.int32)) and torch.equal(st2, status) and _bits_equal(M2, M) and _bits_equal(mc2, mc)
    for name, a, b in zip(FIELDS, got, sep):
        assert _same_bits(a.cpu(), b.cpu()), name

"""-m gpu: the resampling views -- sl_normalize_view_resize (engine.normalize_view(resize=)) and sl_normalize_view_affine (engine.
normalize_view_affine) -- over the route matrix tests/test_gpu_view.py runs k_view over.

view_resize_body and k_view_affine each hold a copy of view_body's per-source-pixel arithmetic: the K.fast / general cast, the
g12 >= 0 / general lasso and the failed-fit pass-through.  Here every copy takes every route of ROUTES under both regimes of _stats,
failed fits of both kinds, and tiny tiles with every output form at both output alignments.

The definition is "the numpy resample of the image the existing entry point writes": full = the uint8 full-tile result of
normalize_apply / normalize_jitter / nothing (tests/test_gpu_view.py: _full), want = want_view (tests/test_view_resize_host.py) or
affine_resample (stainlib_amd.tile_view) on it, a tensor TensorFormat.convert of that.  Integer arithmetic on bytes: every comparison
is exact.  Every call writes into a buffer with sentinel elements before and after the output, checked after the call."""
import numpy as np
import pytest
import torch

from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_check_windows, affine_resample, affine_row_sums
from tests.test_gpu_jitter import M_TGT_NEG, MAXC_TGT, SENTINEL, _dev_tiles, _formats, _same_bits, _stats, _tiles
from tests.test_gpu_view import ROUTES, _full, _view
from tests.test_view_resize_host import want_view

pytestmark = pytest.mark.gpu

FILL = (10, 30, 200)
KERNELS = ["resize", "affine"]


def _affine_view(dev, win, size, fmt=None, out_off=0, max_r=AFFINE_MAX_R, fill=FILL, **kw):
    """engine.normalize_view_affine into a guarded buffer -> CPU tensor: tests/test_gpu_view.py's _view for the affine call.  The output
    sits 16 bytes + out_off elements into a buffer of SENTINEL with 16 more bytes behind it; both margins must still hold SENTINEL
    afterwards."""
    from stainlib_amd import engine
    n, h, w, _ = dev.shape
    oh, ow = (h, w) if size is None else ((size, size) if isinstance(size, int) else size)
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
    res = engine.normalize_view_affine(dev, win, size, max_r, fill, fmt=fmt, out=out, **kw)
    assert res is out
    torch.cuda.synchronize()
    got = buf.cpu()
    outside = torch.cat([got[:start], got[start + numel:]])
    assert bool((outside == SENTINEL).all()), f"{tuple(dev.shape)} -> {size} fmt={fmt} out+{out_off}: written outside the output"
    return out.cpu()


def _row(cy, cx, a00, a01, a10, a11):
    return [int(np.rint(Q * v)) for v in (cy, cx, a00, a01, a10, a11)]


def _rot(deg, z=1.0):
    c, s = np.cos(np.radians(deg)) / z, np.sin(np.radians(deg)) / z
    return (c, -s, s, c)


def _affine_rows(h, w):
    """eight rows: the identity, 30 and 45 degrees, a shear, a negative determinant, a centre half outside (rotated, fractional), the
    row-sum limit (45 degrees at sqrt 2) and a transposition about a fractional centre"""
    rows = [_row(h / 2, w / 2, 1, 0, 0, 1), _row(h / 2, w / 2, *_rot(30)), _row(h / 2, w / 2, *_rot(45)), _row(h / 2, w / 2, 1, 0.4, 0.1, 0.9),
            _row(h / 2, w / 2, 0.8, 0.3, 0.2, -1.1), _row(0.25, w / 2 + 0.3701, *_rot(-17, 1.1)), _row(h / 2, w / 2, 1, -1, 1, 1),
            _row(h / 2 + 0.5, w / 2 + 0.25, 0, 1, 1, 0)]
    win = np.array(rows, dtype=np.int64)
    assert int(affine_row_sums(win).max()) == AFFINE_MAX_R and win[4, 2] * win[4, 5] - win[4, 3] * win[4, 4] < 0
    return affine_check_windows(win, len(rows), h, w)


# resizing windows (y0, x0, d, wh, ww) of 70 x 66 tiles for the output (33, 47) -- an odd code resamples to (47, 33): the eight codes,
# x0 over every residue mod 4, the identity straight and turned (flush against the tile's end), the whole tile, non-integer ratios down
# along both axes, up along one and down along the other both ways round, pure upscaling, one pixel (the tile's last)
WIN_70x66 = np.array([(0, 0, 0, 33, 47), (0, 2, 1, 70, 50), (0, 0, 2, 70, 66), (3, 0, 3, 20, 66), (5, 7, 4, 50, 30), (40, 3, 5, 3, 5),
                      (69, 65, 6, 1, 1), (70 - 47, 66 - 33, 7, 47, 33)], dtype=np.int32)
# ... of 9 x 11 tiles for the output (5, 7)
WIN_9x11 = np.array([(0, 0, 0, 5, 7), (0, 0, 1, 9, 11), (0, 0, 2, 9, 11), (2, 3, 3, 7, 5), (1, 1, 4, 3, 10), (4, 2, 5, 2, 3), (8, 10, 6, 1, 1),
                     (0, 6, 7, 9, 5)], dtype=np.int32)
for _w in (WIN_70x66, WIN_9x11):
    assert sorted(_w[:, 2].tolist()) == list(range(8)) and {int(x) % 4 for x in _w[:, 1]} == {0, 1, 2, 3}


class _Kernel(object):
    """one of the two resampling views: its windows for a tile shape, its guarded call and its numpy definition on `full`"""

    def __init__(self, kind, h, w):
        self.kind, self.bound = kind, (h, w)
        self.win = _affine_rows(h, w) if kind == "affine" else {(70, 66): WIN_70x66, (9, 11): WIN_9x11}[(h, w)]

    def call(self, dev, win, size, fmt=None, out_off=0, **kw):
        if self.kind == "affine":
            return _affine_view(dev, win, size, fmt, out_off, **kw)
        return _view(dev, win, size, 7, fmt=fmt, out_off=out_off, resize=self.bound, **kw)

    def want(self, full, win, size):
        full = full.numpy()
        if self.kind == "affine":
            return torch.from_numpy(np.stack([affine_resample(full[t], win[t], size, FILL) for t in range(len(win))]))
        return torch.from_numpy(want_view(full, win, size, 7, self.bound))


def _check(K, dev, win, size, routes, fmts, regime="he", out_offs=(0,)):
    n, h, w, _ = dev.shape
    M, mc, ab = _stats(n, regime)
    fulls = {}
    for route in routes:
        full, kw = _full(dev, route, M, mc, ab)
        fulls[route] = full
        want = K.want(full, win, size)
        assert tuple(want.shape) == (n, *size, 3)
        for fmt in fmts:
            wt = want if fmt is None else fmt.convert(want.cuda()).cpu()
            for off in out_offs:
                got = K.call(dev, win, size, fmt, off, **kw)
                assert _same_bits(got, wt), f"{K.kind} {n}x{h}x{w} -> {size} {route} {regime} {fmt} out+{off}"
    return fulls


# ---- 1. both lasso regimes and both casts, with and without a target, on every route ---------------------------------------------------
@pytest.mark.parametrize("regime", ["he", "neg"])
@pytest.mark.parametrize("kind", KERNELS)
def test_lasso_regimes_and_casts_on_every_route(kind, regime):
    from stainlib_amd import engine
    n, h, w, size = 8, 70, 66, (33, 47)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    K = _Kernel(kind, h, w)
    fulls = _check(K, dev, K.win, size, ROUTES, [None, _formats()[3]], regime=regime)
    # the general paths do something, on the device: under a target with a negative entry values pass 255 -- the general cast wraps
    # them, the saturating one does not --, and the images of the two regimes differ on every route that computes
    M, mc, ab = _stats(n, regime)
    assert not torch.equal(engine.normalize_apply(dev, M, mc, M_TGT_NEG, MAXC_TGT), engine.normalize_jitter(
        dev, M, mc, M_TGT_NEG, MAXC_TGT, np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (n, 1))))
    if regime == "neg":
        he = _stats(n, "he")
        for route in ROUTES[1:]:
            assert not torch.equal(fulls[route], _full(dev, route, *he)[0]), route
    assert len({fulls[r].numpy().tobytes() for r in ROUTES}) == len(ROUTES)                   # (seven different images)


# ---- 2. a failed fit in the middle of a batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["nan_M", "zero_maxC"])
@pytest.mark.parametrize("kind", KERNELS)
def test_a_failed_fit_gives_the_view_of_its_own_bytes(kind, how):
    n, h, w, size = 3, 70, 66, (33, 47)
    dev = _dev_tiles(_tiles(n, h, w), 0)
    K = _Kernel(kind, h, w)
    win = np.ascontiguousarray(K.win[[1, 4, 3]])
    M, mc, ab = _stats(n)
    M, mc = M.copy(), mc.copy()
    if how == "nan_M":
        M[1] = np.nan
    else:
        mc[1] = [1.0, 0.0]
    raw = K.want(dev.cpu(), win, size)
    for route in ("apply", "tissue", "all_own"):
        full, kw = _full(dev, route, M, mc, ab)
        assert torch.equal(full[1], dev[1].cpu()) and not torch.equal(full[0], dev[0].cpu())   # (the existing pass hands the tile through)
        want = K.want(full, win, size)
        assert torch.equal(want[1], raw[1]) and not torch.equal(want[0], raw[0]) and not torch.equal(want[2], raw[2])
        for fmt in (None, _formats()[0], _formats()[5]):
            got = K.call(dev, win, size, fmt, **kw)
            wt, rt = (want, raw) if fmt is None else (fmt.convert(want.cuda()).cpu(), fmt.convert(raw.cuda()).cpu())
            assert _same_bits(got, wt), f"{kind} {how} {route} {fmt}"
            assert _same_bits(got[1:2], rt[1:2])


# ---- 3. tiny tiles: every route, every output form, both output alignments ----------------------------------------------------------------
@pytest.mark.parametrize("kind,size", [("resize", (5, 7)), ("affine", (5, 7)), ("affine", (13, 12))])
def test_tiny_tiles_every_route_and_format(kind, size):
    n, h, w = 8, 9, 11
    dev = _dev_tiles(_tiles(n, h, w), 0)
    K = _Kernel(kind, h, w)
    _check(K, dev, K.win, size, ROUTES, [None] + _formats(), out_offs=(0, 1))
    _check(K, dev, K.win, size, ["apply", "tissue", "all_own"], [None, _formats()[2]], regime="neg")

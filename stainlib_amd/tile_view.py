"""TileView: the geometric half of a training loader's augmentation -- a random crop, a random flip and a random quarter turn, different
for every tile -- drawn on the host and applied INSIDE the apply pass (engine.normalize_view, sl_normalize_view): only the window's
pixels are read, computed and written, and the model-ready tensor comes out cropped, flipped and turned.

A view of one tile is (y0, x0, d): the window's corner in the tile and a dihedral code d = k | 4 f -- f: flip along the width FIRST,
then k quarter turns counter-clockwise (torch.rot90(., k, dims=(0, 1)) of the (H, W, 3) image).  The output size (oh, ow) is one for
the whole batch, so a code with odd k takes an (ow, oh) window.

shrink = s in {1, 2, 4} is a change of magnification in the same pass (sl_normalize_view_shrink): the window is s times the output in
both directions, and every output pixel is the rounded mean of an s x s box of the image at source resolution -- per channel
(sum + s s / 2) >> (2 log2 s) of the uint8 bytes, boxes counted from the window's corner (any pixel, not only a multiple of s).

scale = (lo, hi) makes the view a random-resized crop (sl_normalize_view_resize): a view of one tile is then (y0, x0, d, wh, ww), a
window of wh rows and ww columns in the TILE's orientation, of random area and aspect ratio, resampled to the output size by exact
pixel-area averaging in integers -- OpenCV's INTER_AREA for shrinking.  Along an axis of nw window pixels and no outputs, in coordinates
scaled by no, source pixel k covers [k no, (k + 1) no), output i covers [i nw, (i + 1) nw) and c(i, k) is the length of their overlap;
per channel b = (2 S + D) // (2 D) with S = sum cy(i, k) cx(j, l) window[k, l] and D = wh ww.  A window smaller than the output comes
out piecewise constant with blended edges (the same formula), not bilinear.  area_resample below is that definition in numpy.

TileAffine (behind the views above) is the affine view: rotation by ANY angle, zoom, shear and translation, a view of one tile six
int32 in 2^-16 source pixels, the image sampled bilinearly with 8-bit weights and its label maps by the nearest element, both in
integers (sl_normalize_view_affine, sl_view_planes_affine); affine_coords / affine_resample / affine_nearest are that definition in numpy.

TileElastic (at the end of the module) is the elastic view: a TileAffine plus a smooth per-pixel displacement, the quadratic B-spline of
a coarse lattice of random control displacements in 1/256 source pixel, in integers (sl_normalize_view_elastic, sl_view_planes_elastic);
its windows are an ElasticWindows(affine, field); elastic_displacement / elastic_coords / elastic_resample / elastic_nearest are that
definition in numpy.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SHRINKS = (1, 2, 4)
RESIZE_MAX_RATIO = 16            # a window side is at most 16 times the output side it is resampled to (17 source pixels per output)
RESIZE_MAX_AREA = 1 << 22        # wh ww: the weighted sums stay below 2^31
RESIZE_MAX_PRODUCT = 1 << 30     # an output side times a window side: the scaled coordinates are 32-bit


def _size2(size):
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        size = (size, size)
    try:
        oh, ow = size
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (oh, ow)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"size must be None (the full tile), an int or (oh, ow) ints, not {size!r}") from None
    if oh < 1 or ow < 1:
        raise ValueError(f"size must be at least 1 x 1, not {size!r}")
    return int(oh), int(ow)


def check_shrink(shrink):
    """shrink as an int, or ValueError unless it is 1, 2 or 4"""
    if isinstance(shrink, bool) or not isinstance(shrink, (int, np.integer)) or int(shrink) not in SHRINKS:
        raise ValueError(f"shrink must be 1, 2 or 4, not {shrink!r}")
    return int(shrink)


def check_size(size, h, w, d_mask, shrink=1):
    """(oh, ow) of a view of size `size` (None: the full tile, (h // shrink, w // shrink)) out of (h, w) tiles, or ValueError when its
    window -- shrink times the size -- does not fit in every orientation d_mask allows (quarter turns take the transposed window)."""
    if not (isinstance(d_mask, (int, np.integer)) and not isinstance(d_mask, bool) and 0 <= d_mask <= 7):
        raise ValueError(f"d_mask must be an int in 0..7, not {d_mask!r}")
    s = check_shrink(shrink)
    if s == 1:
        oh, ow = (int(h), int(w)) if size is None else _size2(size)
    elif size is None:
        oh, ow = int(h) // s, int(w) // s
        if oh < 1 or ow < 1:
            raise ValueError(f"a {h} x {w} tile has no {s} x {s} box: the full tile at shrink={s} is below 1 x 1")
    else:
        oh, ow = _size2(size)
    what = f"a {oh} x {ow} view" if s == 1 else f"a {oh} x {ow} view at shrink={s} (a {s * oh} x {s * ow} window)"
    if s * oh > h or s * ow > w:
        raise ValueError(f"{what} does not fit in a {h} x {w} tile")
    if (d_mask & 1) and (s * ow > h or s * oh > w):
        raise ValueError(f"a quarter turn of {what} takes a {s * ow} x {s * oh} window, which does not fit in a {h} x {w} tile "
                         "(rot90=False keeps flips and half turns)")
    return oh, ow


def _range2(x, what, upper=None):
    try:
        lo, hi = (float(v) for v in x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (lo, hi), not {x!r}") from None
    if not (0.0 < lo <= hi and np.isfinite(hi)) or (upper is not None and hi > upper):
        raise ValueError(f"{what} must be a pair (lo, hi) with 0 < lo <= hi" + (f" <= {upper:g}" if upper is not None else "") + f", not {x!r}")
    return lo, hi


def check_resize_size(size, h, w, d_mask):
    """(oh, ow) of a resizing view of size `size` (None: the tile's own (h, w)) out of (h, w) tiles: any size at least 1 x 1 -- the
    window is resampled to it --, or ValueError beyond the 32-bit limit of the scaled coordinates."""
    if not (isinstance(d_mask, (int, np.integer)) and not isinstance(d_mask, bool) and 0 <= d_mask <= 7):
        raise ValueError(f"d_mask must be an int in 0..7, not {d_mask!r}")
    oh, ow = (int(h), int(w)) if size is None else _size2(size)
    if max(oh, ow) * max(int(h), int(w)) > RESIZE_MAX_PRODUCT:
        raise ValueError(f"a {oh} x {ow} resizing view of a {h} x {w} tile is too large: the larger output side times the larger tile "
                         f"side must not exceed 2^30")
    return oh, ow


def resize_side_max(no, side):
    """the largest window side along an axis of `no` outputs in a tile side `side`"""
    return min(int(side), RESIZE_MAX_RATIO * int(no))


def overlap_matrix(nw, no):
    """c of the definition: (no, nw) int64, c[i, k] = the overlap of [i nw, (i + 1) nw) and [k no, (k + 1) no)"""
    i = np.arange(no, dtype=np.int64)[:, None]
    k = np.arange(nw, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * nw, (k + 1) * no) - np.maximum(i * nw, k * no))


def area_resample(window, nu, nv):
    """The definition of the resizing view in numpy: the (wh, ww, C) uint8 `window` resampled to (nu, nv, C) uint8 by exact pixel-area
    averaging, round half up -- per channel (2 S + D) // (2 D), S = cy @ window @ cx.T, D = wh ww."""
    window = np.asarray(window)
    wh, ww = window.shape[:2]
    cy, cx = overlap_matrix(wh, nu), overlap_matrix(ww, nv)
    S = np.einsum("ik,klc,jl->ijc", cy, window.astype(np.int64), cx)
    D = wh * ww
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def nearest_index(nw, no):
    """The centre sample of the companion planes (TileView.apply, sl_view_planes) along an axis of nw window pixels and no outputs:
    (no,) int64, k[i] = ((2 i + 1) nw) // (2 no), the pixel under the centre of output i -- i itself when nw == no, s i + s // 2 when
    nw == s no."""
    nw, no = int(nw), int(no)
    if nw < 1 or no < 1:
        raise ValueError(f"nearest_index needs at least one window pixel and one output, not ({nw}, {no})")
    i = np.arange(no, dtype=np.int64)
    return ((2 * i + 1) * nw) // (2 * no)


def nearest_resample(window, nu, nv):
    """The definition of mode="nearest" in numpy: the (wh, ww, ...) `window` of any dtype resampled to (nu, nv, ...) by the centre
    sample, a copy of elements -- window[nearest_index(wh, nu)][:, nearest_index(ww, nv)]."""
    window = np.asarray(window)
    wh, ww = window.shape[:2]
    return window[nearest_index(wh, nu)][:, nearest_index(ww, nv)]


def view_planes_reference(planes, windows, size, shrink=1, mode="nearest"):
    """TileView.apply in numpy, on windows already in range (what engine._view_windows accepts): `planes` (N, H, W) or (N, C, H, W) of
    any dtype, `windows` (N, 3) rows (y0, x0, d) under `shrink`, or (N, 5) rows (y0, x0, d, wh, ww) of a resizing view; size = (oh, ow).
    Per tile and plane: the window resampled in the TILE's orientation -- nearest_resample, or for mode="area" (uint8) area_resample,
    of which the shrink's box mean (S + s s / 2) >> (2 log2 s) is the case wh = s nu --, THEN flipped along the width if d & 4 and
    turned d & 3 quarter turns counter-clockwise."""
    planes = np.asarray(planes)
    windows = np.asarray(windows)
    if mode not in ("nearest", "area"):
        raise ValueError(f"mode must be 'nearest' or 'area', not {mode!r}")
    if mode == "area" and planes.dtype != np.uint8:
        raise ValueError("mode='area' is defined on uint8 planes only")
    oh, ow = _size2(size)
    s = check_shrink(shrink)
    x = planes[:, None] if planes.ndim == 3 else planes
    out = np.empty(x.shape[:2] + (oh, ow), dtype=x.dtype)
    for t in range(x.shape[0]):
        y0, x0, d = (int(v) for v in windows[t, :3])
        nu, nv = (ow, oh) if d & 1 else (oh, ow)
        wh, ww = (int(windows[t, 3]), int(windows[t, 4])) if windows.shape[1] == 5 else (s * nu, s * nv)
        for c in range(x.shape[1]):
            win = x[t, c, y0:y0 + wh, x0:x0 + ww]
            r = nearest_resample(win, nu, nv) if mode == "nearest" else area_resample(win[..., None], nu, nv)[..., 0]
            out[t, c] = np.rot90(r[:, ::-1] if d & 4 else r, d & 3)
    return out[:, 0] if planes.ndim == 3 else out


class TileView(object):
    """size: None (the full tile), an int or (oh, ow) -- the size of the OUTPUT.  flip: draw flips.  rot90: draw quarter turns (the
    view must then fit transposed as well).  Half turns are drawn whenever flips are: a flip along the height is a flip along the
    width and a half turn.  shrink: 1, 2 or 4 -- the window is shrink times the output, averaged down in boxes (see the module);
    size=None is then (h // shrink, w // shrink).
    scale: None, or (lo, hi) with 0 < lo <= hi <= 1 -- the view is a random-resized crop: per tile a window of a random share of the
    tile's area in [lo, hi] and a random aspect ratio ww / wh in ratio = (lo, hi), log-uniform, resampled to the output size by exact
    area averaging (see the module).  Not with a shrink.  size=None is then the tile's own size."""

    def __init__(self, size=None, flip=True, rot90=True, shrink=1, scale=None, ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.size = None if size is None else _size2(size)
        self.flip = bool(flip)
        self.rot90 = bool(rot90)
        self.shrink = check_shrink(shrink)
        self.scale = None if scale is None else _range2(scale, "scale", 1.0)
        self.ratio = _range2(ratio, "ratio")
        if self.scale is not None and self.shrink != 1:
            raise ValueError(f"scale= (a resizing view) does not go with shrink={self.shrink}: the window's size is drawn per tile")

    @property
    def resizing(self):
        """whether the view draws (y0, x0, d, wh, ww) and resamples (scale=)"""
        return self.scale is not None

    @property
    def d_mask(self):
        return (4 if self.flip else 0) | (3 if self.rot90 else 2 if self.flip else 0)

    @property
    def codes(self):
        """the dihedral codes this view draws from, ascending"""
        return [c for c in range(8) if c & ~self.d_mask == 0]

    def out_size(self, h, w):
        if self.resizing:
            return check_resize_size(self.size, h, w, self.d_mask)
        return check_size(self.size, h, w, self.d_mask, self.shrink)

    def window_bound(self, h, w):
        """(max_wh, max_ww) of a resizing view of (h, w) tiles: the largest window sides a draw can give, in any orientation -- what
        a call with windows on the device sizes its launch from.  The tile's sides, at most 16 times the larger output side they can
        map to, and for a tile of more than 2^22 pixels both scaled down together (by sqrt(2^22 / (h w)), rounded down) until their
        product is at most 2^22: a call takes ONE bound for all its windows, so no two of them may be tall and wide beyond it."""
        oh, ow = self.out_size(h, w)
        big = max(oh, ow) if self.d_mask & 1 else None
        mh, mw = resize_side_max(big or oh, h), resize_side_max(big or ow, w)
        return _reduce_area(mh, mw)

    def draw(self, n, h, w):
        """(n, 3) int32: y0, x0, d per tile, from the GLOBAL numpy stream (the convention of StainJitter.draw).  Per tile, in order:
        d = the np.random.randint(len(codes))-th code; y0 = np.random.randint(0, h - s wh + 1); x0 = np.random.randint(0, w - s ww + 1),
        (wh, ww) the output size as that code's window sees it and s the shrink.  A resizing view (scale=) returns (n, 5) int32,
        y0, x0, d, wh, ww per tile: five draws per tile, in the order _draw_resize documents."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        oh, ow = self.out_size(h, w)
        if self.resizing:
            return self._draw_resize(n, int(h), int(w), oh, ow)
        s = self.shrink
        codes = self.codes
        win = np.empty((n, 3), dtype=np.int32)
        for t in range(n):
            d = codes[np.random.randint(len(codes))]
            wh, ww = (ow, oh) if d & 1 else (oh, ow)
            win[t, 0] = np.random.randint(0, h - s * wh + 1)
            win[t, 1] = np.random.randint(0, w - s * ww + 1)
            win[t, 2] = d
        return win

    def _draw_resize(self, n, h, w, oh, ow):
        """(n, 5) int32: y0, x0, d, wh, ww per tile, from the GLOBAL numpy stream.  Per tile, in order: d as in draw;
        a = np.random.uniform(*scale); r = exp(np.random.uniform(log ratio[0], log ratio[1]));
        wh = clip(floor(sqrt(a h w / r) + 0.5), 1, min(h, 16 nu, bh)), ww = clip(floor(sqrt(a h w r) + 0.5), 1, min(w, 16 nv, bw)) with
        (nu, nv) the output size as that code's window sees it and (bh, bw) = window_bound(h, w), which keeps wh ww <= 2^22 (it is
        (h, w) itself up to 2048 x 2048); y0 = np.random.randint(0, h - wh + 1); x0 = np.random.randint(0, w - ww + 1).  Five draws per tile, always: a
        window that does not fit is CLAMPED, not redrawn -- this is not torchvision's rejection loop (ten tries, then a centre crop),
        whose number of draws varies."""
        codes = self.codes
        lr0, lr1 = np.log(self.ratio[0]), np.log(self.ratio[1])
        bh, bw = self.window_bound(h, w)
        win = np.empty((n, 5), dtype=np.int32)
        for t in range(n):
            d = codes[np.random.randint(len(codes))]
            nu, nv = (ow, oh) if d & 1 else (oh, ow)
            a = np.random.uniform(self.scale[0], self.scale[1])
            r = np.exp(np.random.uniform(lr0, lr1))
            wh = int(np.clip(np.floor(np.sqrt(a * h * w / r) + 0.5), 1, resize_side_max(nu, min(h, bh))))
            ww = int(np.clip(np.floor(np.sqrt(a * h * w * r) + 0.5), 1, resize_side_max(nv, min(w, bw))))
            win[t] = (np.random.randint(0, h - wh + 1), np.random.randint(0, w - ww + 1), d, wh, ww)
        return win

    def apply(self, planes, windows=None, mode="nearest", out=None):
        """The per-pixel companions of a batch -- class map, instance map, loss mask, tissue mask, distance map -- through the windows
        their images went through (sl_view_planes): `planes` is a contiguous device tensor (N, H, W) or (N, C, H, W) of any 1-, 2-, 4-
        or 8-byte dtype, `windows` what the image call with this view returned for (H, W) tiles (or self.draw(N, H, W)); returns
        (N, oh, ow) / (N, C, oh, ow) of the same dtype.  Nothing is drawn here.
        mode="nearest": every output element is a bit copy of the element under its centre (labels are never averaged), sampled in the
        TILE's orientation and then flipped and turned (see nearest_index); mode="area" (uint8 only: 0 / 255 masks, soft maps): the
        images' own box mean / area average per plane.  Without shrink or scale both are the same permutation.
        Host windows are range-checked as for the image calls (ValueError); device windows are clamped by the kernel with the image
        kernels' rules.  out: a tensor to write into."""
        from . import engine
        if windows is None:
            raise ValueError("windows is required: pass what the image call with this view returned, or view.draw(N, H, W) "
                             "-- apply draws nothing itself")
        if len(getattr(windows, "shape", ())) == 2 and windows.shape[1] == 6:
            raise ValueError("six-column windows are those of an affine view (TileAffine.draw): take the planes through that "
                             "TileAffine's apply -- a TileView's windows are (y0, x0, d) or (y0, x0, d, wh, ww)")
        if isinstance(windows, ElasticWindows):
            raise ValueError("these windows are the ElasticWindows of an elastic view: take the planes through the apply of the "
                             "TileElastic that drew them")
        h, w = engine.planes_hw(planes)
        return engine.view_planes(planes, windows, self.size, self.d_mask, mode=mode, out=out, shrink=self.shrink,
                                  resize=engine._view_resize_hw(self, windows, h, w))

    def __repr__(self):
        tail = f", shrink={self.shrink}" if self.shrink != 1 else ""
        if self.resizing:
            tail += f", scale={self.scale}, ratio={self.ratio}"
        return f"TileView(size={self.size}, flip={self.flip}, rot90={self.rot90}{tail})"


def _reduce_area(wh, ww):
    """(wh, ww) as they are, or both scaled by sqrt(2^22 / (wh ww)) and rounded down (at least 1), until wh ww <= 2^22"""
    while wh * ww > RESIZE_MAX_AREA:
        f = np.sqrt(RESIZE_MAX_AREA / float(wh * ww))
        wh, ww = max(1, int(wh * f)), max(1, int(ww * f))           # (f < 1: a side above 1 gets smaller, so this ends)
    return int(wh), int(ww)


# ---- the affine view: rotation by any angle, zoom, shear and translation (sl_normalize_view_affine, sl_view_planes_affine) ------------------
# A view of one tile is a row of six int32, (cy, cx, a00, a01, a10, a11), all in units of 2^-16 source pixel; pixel k of an axis covers
# [k, k + 1).  (cy, cx): the source position of the centre of the output; a..: the source displacement per output pixel.  The functions
# below ARE the definition; the kernels are tested against them bit for bit.
AFFINE_Q = 65536                 # one source pixel
AFFINE_MAX_SIDE = 8192           # h, w, oh, ow
AFFINE_MAX_R = 2 * AFFINE_Q      # a row sum |a00| + |a01|, |a10| + |a11|: at most two source pixels per output pixel
AFFINE_CENTRE_SLACK = 1 << 28    # a centre lies within this of the tile


def affine_coords(row, size):
    """(Y, X), two (oh, ow) int64 arrays: the source position (2^-16 pixels) of every output pixel of a view `row` = (cy, cx, a00, a01,
    a10, a11) with size = (oh, ow).  With u = 2 i + 1 - oh, v = 2 j + 1 - ow: Y = cy + ((a00 u + a01 v) >> 1), X = cx + ((a10 u + a11 v)
    >> 1), the shift arithmetic (a floor)."""
    oh, ow = _size2(size)
    cy, cx, a00, a01, a10, a11 = (int(v) for v in np.asarray(row).reshape(6))
    u = (2 * np.arange(oh, dtype=np.int64) + 1 - oh)[:, None]
    v = (2 * np.arange(ow, dtype=np.int64) + 1 - ow)[None, :]
    return cy + ((a00 * u + a01 * v) >> 1), cx + ((a10 * u + a11 * v) >> 1)


def _fill3(fill):
    """fill= of the images as three ints 0 .. 255 (an int: that byte in every channel), or ValueError"""
    try:
        f = (fill,) * 3 if isinstance(fill, (int, np.integer)) and not isinstance(fill, bool) else tuple(fill)
        if len(f) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255 for v in f):
            raise TypeError
    except TypeError:
        raise ValueError(f"fill of an affine view must be an int or three ints in 0 .. 255 (output bytes, r g b), not {fill!r}") from None
    return tuple(int(v) for v in f)


def affine_resample(full, row, size, fill=255):
    """The definition of the affine view of an image in numpy: the (h, w, C) uint8 `full` sampled bilinearly with 8-bit weights at
    affine_coords(row, size) -> (oh, ow, C) uint8.  ty = Y - Q/2, ky = ty >> 16, fy = (ty >> 8) & 255 (x likewise); p00 .. p11 the bytes
    at (ky, kx), (ky, kx + 1), (ky + 1, kx), (ky + 1, kx + 1), a tap outside the image the fill byte of its channel (fill: an int or one
    int per channel); b = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16."""
    full = np.asarray(full)
    if full.dtype != np.uint8 or full.ndim != 3:
        raise ValueError("affine_resample is defined on an (h, w, C) uint8 image")
    return _bilinear_at(full, *affine_coords(row, size), fill)


def affine_nearest(plane, row, size, fill=0):
    """The definition of the affine view of a companion plane in numpy: the (h, w) `plane` of any dtype -> (oh, ow) of that dtype, the
    element at (Y >> 16, X >> 16) copied bit for bit, outside the plane `fill` (as an element of the plane's dtype)."""
    plane = np.asarray(plane)
    if plane.ndim != 2:
        raise ValueError("affine_nearest is defined on an (h, w) plane")
    h, w = plane.shape
    Y, X = affine_coords(row, size)
    ky, kx = Y >> 16, X >> 16
    inside = (ky >= 0) & (ky < h) & (kx >= 0) & (kx < w)
    out = np.full(ky.shape, np.asarray(fill).astype(plane.dtype), dtype=plane.dtype)
    out[inside] = plane[ky[inside], kx[inside]]
    return out


def affine_row_sums(windows):
    """(n,) int64: max(|a00| + |a01|, |a10| + |a11|) per row of (n, 6) windows"""
    a = np.abs(np.asarray(windows).astype(np.int64)[:, 2:6])
    return np.maximum(a[:, 0] + a[:, 1], a[:, 2] + a[:, 3])


def affine_check_size(size, h, w):
    """(oh, ow) of an affine view of size `size` (None: the tile's own (h, w)) out of (h, w) tiles: any size, or ValueError beyond the
    limit that keeps the coordinates 32-bit (h, w, oh, ow <= 8192)."""
    oh, ow = (int(h), int(w)) if size is None else _size2(size)
    if min(int(h), int(w)) < 1 or max(oh, ow, int(h), int(w)) > AFFINE_MAX_SIDE:
        raise ValueError(f"an affine view takes tiles and outputs of 1 .. {AFFINE_MAX_SIDE} pixels a side (32-bit coordinates), "
                         f"not a {oh} x {ow} view of a {h} x {w} tile")
    return oh, ow


def affine_check_windows(windows, n, h, w, size=None, bound=AFFINE_MAX_R):
    """The (n, 6) int32 windows of an affine view of (h, w) tiles, in range, as a contiguous int32 array -- or ValueError: a wrong shape
    or a dtype that is not an integer one; a side above 8192; a row sum |a00| + |a01| or |a10| + |a11| above 2 Q (more than two source
    pixels per output pixel: shrink= / scale= downsample further) or above `bound`, the max_r of the call; a centre outside
    [-2^28, side Q + 2^28].  Zero and singular matrices are legal."""
    what = "windows of an affine view must hold (cy, cx, a00, a01, a10, a11) per tile"
    if windows is None:
        raise ValueError(f"{what}: an (N, 6) int32 array (TileAffine.draw)")
    affine_check_size(size, h, w)
    if isinstance(bound, bool) or not isinstance(bound, (int, np.integer)) or not 1 <= int(bound) <= AFFINE_MAX_R:
        raise ValueError(f"the bound max_r of an affine view must be an int in 1 .. 2 Q = {AFFINE_MAX_R} (2^-16 pixels), not {bound!r}")
    try:
        win = windows.numpy() if hasattr(windows, "numpy") and not isinstance(windows, np.ndarray) else np.asarray(windows)
        if win.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: an (N, 6) integer array") from None
    if win.shape != (int(n), 6):
        raise ValueError(f"{what}: an ({int(n)}, 6) array, not one of shape {win.shape}")
    win = win.astype(np.int64)
    r = affine_row_sums(win)
    bad = r > min(int(bound), AFFINE_MAX_R)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"windows: tile {t} of the affine view has the row sum {int(r[t])} (2^-16 pixels), above "
                         + (f"2 Q = {AFFINE_MAX_R}: more than two source pixels per output pixel (shrink= / scale= downsample further)"
                            if r[t] > AFFINE_MAX_R else f"the call's bound max_r = {int(bound)}"))
    for k, side, name in ((0, int(h), "cy"), (1, int(w), "cx")):
        bad = (win[:, k] < -AFFINE_CENTRE_SLACK) | (win[:, k] > side * AFFINE_Q + AFFINE_CENTRE_SLACK)
        if bad.any():
            t = int(np.argmax(bad))
            raise ValueError(f"windows: tile {t} of the affine view has the centre {name} = {int(win[t, k])}, outside "
                             f"[-2^28, {side} Q + 2^28]")
    return np.ascontiguousarray(win.astype(np.int32))


def _pair(x, what, positive=False):
    try:
        lo, hi = (float(v) for v in x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (lo, hi), not {x!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi) or (positive and lo <= 0.0):
        raise ValueError(f"{what} must be a pair (lo, hi) of finite numbers with " + ("0 < " if positive else "") + f"lo <= hi, not {x!r}")
    return lo, hi


def _max_mix(a, b, lo, hi):
    """max over theta in [lo, hi] degrees of a |cos theta| + b |sin theta| (a, b >= 0): the end points and the maxima
    theta = k 180 +- atan(b / a) that lie inside"""
    if hi - lo >= 180.0:
        return float(np.hypot(a, b))
    f = lambda d: a * abs(np.cos(np.radians(d))) + b * abs(np.sin(np.radians(d)))
    best = max(f(lo), f(hi))
    peak = np.degrees(np.arctan2(b, a))
    for k in range(int(np.floor(lo / 180.0)) - 1, int(np.ceil(hi / 180.0)) + 2):
        for d in (180.0 * k + peak, 180.0 * k - peak):
            if lo <= d <= hi:
                best = max(best, f(d))
    return float(best)


class TileAffine(object):
    """The affine half of a segmentation loader's augmentation -- a rotation by ANY angle, a zoom, a shear, a translation and a flip,
    different for every tile -- drawn on the host and applied INSIDE the view pass (engine.normalize_view_affine): the image bilinearly
    with 8-bit weights in integers (affine_resample is the definition), its label maps by the nearest element (apply, affine_nearest).
    size: None (the tile's own size), an int or (oh, ow) -- the size of the OUTPUT; it need not fit in the tile.
    rotate: (lo, hi) degrees; zoom: (lo, hi), log-uniform, z > 1 magnifies; shear: (lo, hi) degrees, |shear| < 90; translate: (ty, tx)
    or one number, the largest shift of the centre as a share of the tile's side, 0 .. 1; flip: draw mirror images;
    fill: what lies outside the tile, an int or three ints 0 .. 255 -- OUTPUT bytes, not normalised.
    A view of one tile is (cy, cx, a00, a01, a10, a11) in 2^-16 source pixels (see draw).  The kernels take at most two source pixels
    per output pixel: both row sums |a00| + |a01|, |a10| + |a11| <= 2 Q.  Nothing is redrawn or clamped, so the CONSTRUCTOR refuses
    ranges from which a draw could pass that limit, by this sufficient bound: with T = max |tan shear|, the real row sums are
    (|c| + |c t - s|) / z <= ((1 + T) |c| + |s|) / z and (|s| + |s t + c|) / z <= ((1 + T) |s| + |c|) / z; R = the larger of the two
    maxima over the rotate range (sqrt((1 + T)^2 + 1) once it spans 180 degrees) divided by zoom[0]; every entry is rounded to
    the nearest 2^-16, at most 1/2 each, so an integer row sum is at most 65536 R + 1, and the constructor wants
    ceil(65536 R (1 + 10^-12)) + 1 <= 2 Q = 131072.  That number is `bound`, the max_r of a call with windows on the device.
    (zoom = 0.5 at no rotation meets the limit exactly and is refused by the + 1; zoom[0] = 0.50001 passes.)"""

    def __init__(self, size=None, rotate=(-180, 180), zoom=(1, 1), shear=(0, 0), translate=(0, 0), flip=True, fill=255):
        self.size = None if size is None else _size2(size)
        self.rotate = _pair(rotate, "rotate")
        self.zoom = _pair(zoom, "zoom", positive=True)
        self.shear = _pair(shear, "shear")
        if not (-90.0 < self.shear[0] and self.shear[1] < 90.0):
            raise ValueError(f"shear must lie within (-90, 90) degrees, not {shear!r}")
        if isinstance(translate, (int, float, np.integer, np.floating)) and not isinstance(translate, bool):
            translate = (translate, translate)
        try:
            ty, tx = (float(v) for v in translate)
            if not (0.0 <= ty <= 1.0 and 0.0 <= tx <= 1.0):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"translate must be a number or (ty, tx), shares of the tile's side in 0 .. 1, not {translate!r}") from None
        self.translate = (ty, tx)
        self.flip = bool(flip)
        self.fill = _fill3(fill)
        T = max(abs(np.tan(np.radians(self.shear[0]))), abs(np.tan(np.radians(self.shear[1]))))
        lo, hi = self.rotate
        R = max(_max_mix(1.0 + T, 1.0, lo, hi), _max_mix(1.0, 1.0 + T, lo, hi)) / self.zoom[0]
        bound = int(np.ceil(AFFINE_Q * R * (1.0 + 1e-12))) + 1
        if bound > AFFINE_MAX_R:
            raise ValueError(f"TileAffine(rotate={rotate!r}, zoom={zoom!r}, shear={shear!r}) could draw a matrix with a row sum of "
                             f"{bound / AFFINE_Q:.5f} source pixels per output pixel; the affine view takes at most 2 (bilinear aliases "
                             "beyond): raise zoom[0] or narrow shear / rotate -- TileView(shrink=) / TileView(scale=) downsample further")
        self._bound = bound

    # what the view= plumbing of the batch methods asks of a view
    resizing = False
    shrink = 1
    d_mask = 0

    @property
    def bound(self):
        """max_r: an upper bound (2^-16 pixels) of the row sums of every matrix this view can draw -- what a call with windows on the
        device sizes its launch from"""
        return self._bound

    @property
    def fill_rgb(self):
        """the fill as sl_normalize_view_affine takes it: r | g << 8 | b << 16"""
        return self.fill[0] | (self.fill[1] << 8) | (self.fill[2] << 16)

    def out_size(self, h, w):
        return affine_check_size(self.size, h, w)

    def draw(self, n, h, w):
        """(n, 6) int32: cy, cx, a00, a01, a10, a11 per tile, from the GLOBAL numpy stream.  Six draws per tile, always, in this order:
        theta = np.random.uniform(*rotate) degrees; z = exp(np.random.uniform(log zoom[0], log zoom[1])); phi = np.random.uniform(*shear)
        degrees; e = -1 if np.random.randint(2) and flip else 1 (drawn also with flip=False); ty = np.random.uniform(-translate[0],
        translate[0]); tx = np.random.uniform(-translate[1], translate[1]).  With c = cos theta, s = sin theta, t = tan phi:
        A = (1 / z) [[c, e (c t - s)], [s, e (s t + c)]], the centre ((0.5 + ty) h, (0.5 + tx) w); every entry int(np.rint(65536 x)).
        Nothing is redrawn or clamped (the constructor has refused ranges that could leave the limits)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        self.out_size(h, w)
        lz0, lz1 = np.log(self.zoom[0]), np.log(self.zoom[1])
        win = np.empty((n, 6), dtype=np.int32)
        for k in range(n):
            theta = np.radians(np.random.uniform(self.rotate[0], self.rotate[1]))
            z = np.exp(np.random.uniform(lz0, lz1))
            t = np.tan(np.radians(np.random.uniform(self.shear[0], self.shear[1])))
            e = -1.0 if np.random.randint(2) and self.flip else 1.0
            ty = np.random.uniform(-self.translate[0], self.translate[0])
            tx = np.random.uniform(-self.translate[1], self.translate[1])
            c, s = np.cos(theta), np.sin(theta)
            row = ((0.5 + ty) * h, (0.5 + tx) * w, c / z, e * (c * t - s) / z, s / z, e * (s * t + c) / z)
            win[k] = [int(np.rint(AFFINE_Q * x)) for x in row]
        return win

    def apply(self, planes, windows=None, fill=0, out=None):
        """The per-pixel companions of a batch through the windows their images went through (sl_view_planes_affine): `planes` is a
        contiguous device tensor (N, H, W) or (N, C, H, W) of any 1-, 2-, 4- or 8-byte dtype, `windows` what the image call with this
        view returned for (H, W) tiles (or self.draw(N, H, W)); returns (N, oh, ow) / (N, C, oh, ow) of the same dtype: per element
        the NEAREST source element, (Y >> 16, X >> 16), a bit copy -- labels are never blended --, outside the plane `fill` (a
        number, cast to the planes' dtype; e.g. an ignore index).  Nothing is drawn here.  Host windows are range-checked
        (ValueError); device windows are taken as they are under this view's bound.  out: a tensor to write into."""
        from . import engine
        if windows is None:
            raise ValueError("windows is required: pass what the image call with this view returned, or view.draw(N, H, W) "
                             "-- apply draws nothing itself")
        return engine.view_planes_affine(planes, windows, self.size, engine._affine_bound(self, windows), fill=fill, out=out)

    def __repr__(self):
        return (f"TileAffine(size={self.size}, rotate={self.rotate}, zoom={self.zoom}, shear={self.shear}, translate={self.translate}, "
                f"flip={self.flip}, fill={self.fill})")


# ---- the elastic view: the affine view plus a smooth displacement field (sl_normalize_view_elastic, sl_view_planes_elastic) ------------------
# A view of one tile is an affine row AND a control lattice field[t] of shape (gh, gw, 2): displacements (dy, dx) in units of 1/256 source
# pixel -- the resolution of the 8-bit bilinear weights -- on a grid of cells of `cell` OUTPUT pixels, interpolated by a uniform quadratic
# B-spline whose weights are exact integers.  The functions below ARE the definition; the kernels are tested against them bit for bit.
ELASTIC_UNIT = 256               # field units per source pixel
ELASTIC_MAX_D = 8                # the largest displacement, in source pixels
ELASTIC_CELLS = (16, 32, 64, 128, 256)

ElasticWindows = namedtuple("ElasticWindows", ["affine", "field"])
ElasticWindows.__doc__ = """The windows of an elastic view: affine, (N, 6) int32 -- TileAffine's rows --, and field, (N, gh, gw, 2) int32 --
the control displacements (dy, dx) in 1/256 source pixel (elastic_grid_shape).  Both on the host or both on the device."""


def _cell_log2(cell):
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or int(cell) not in ELASTIC_CELLS:
        raise ValueError(f"cell of an elastic view must be a power of two from 16 to 256 (output pixels per lattice cell), not {cell!r}")
    return int(cell).bit_length() - 1


def elastic_grid_shape(size, cell):
    """(gh, gw): the control lattice of an elastic view of size = (oh, ow) with cells of `cell` output pixels; with k = log2 cell,
    gh = ((oh + 2^k - 1) >> k) + 2, gw likewise -- every output pixel has its 3 x 3 nodes"""
    oh, ow = _size2(size)
    k = _cell_log2(cell)
    return ((oh + (1 << k) - 1) >> k) + 2, ((ow + (1 << k) - 1) >> k) + 2


def _elastic_weights(no, k):
    """(a, w): per output 0 .. no - 1 of an axis the first of its three nodes and their (no, 3) int64 weights out of 2^17:
    t = ((2 o + 1) << 8) >> (k + 1), a = t >> 8, f = t & 255, w = ((256 - f)^2, 131072 - (256 - f)^2 - f^2, f^2)"""
    t = ((2 * np.arange(no, dtype=np.int64) + 1) << 8) >> (k + 1)
    a, f = t >> 8, t & 255
    w0, w2 = (256 - f) ** 2, f ** 2
    return a, np.stack([w0, 131072 - w0 - w2, w2], axis=1)


def elastic_displacement(field, size, cell):
    """(oh, ow, 2) int64: the displacement (dy, dx), in 1/256 source pixel, of every output pixel under the (gh, gw, 2) control lattice
    `field`: the uniform quadratic B-spline r[q] = (sum_p wx[p] field[a + q][b + p] + 65536) >> 17, d = (sum_q wy[q] r[q] + 65536) >> 17
    (arithmetic shifts; the weights of _elastic_weights).  |d| <= max |field|; 32-bit for |field| <= 2048."""
    oh, ow = _size2(size)
    k = _cell_log2(cell)
    field = np.asarray(field)
    if field.dtype.kind not in "iu" or field.shape != elastic_grid_shape(size, cell) + (2,):
        raise ValueError(f"the field of one tile must be an integer array of shape {elastic_grid_shape(size, cell) + (2,)}, not "
                         f"{field.dtype} {field.shape}")
    f = field.astype(np.int64)
    a, wy = _elastic_weights(oh, k)
    b, wx = _elastic_weights(ow, k)
    # r[g, j, m]: every lattice row g at every output column j
    r = (sum(wx[None, :, p, None] * f[:, b + p, :] for p in range(3)) + 65536) >> 17
    return (sum(wy[:, None, q, None] * r[a + q] for q in range(3)) + 65536) >> 17


def elastic_coords(row, field, size, cell):
    """(Y, X), two (oh, ow) int64 arrays: affine_coords(row, size) plus the displacement, Y += d[0] << 8, X += d[1] << 8"""
    Y, X = affine_coords(row, size)
    d = elastic_displacement(field, size, cell)
    return Y + (d[..., 0] << 8), X + (d[..., 1] << 8)


def _bilinear_at(full, Y, X, fill):
    """affine_resample from (Y, X) on: affine_taps, the four taps with the fill outside the image, affine_blend"""
    h, w, ch = full.shape
    f = np.asarray(_fill3(fill) if ch == 3 else (int(fill),) * ch, dtype=np.int64)
    ty, tx = Y - AFFINE_Q // 2, X - AFFINE_Q // 2
    ky, kx, fy, fx = ty >> 16, tx >> 16, ((ty >> 8) & 255)[..., None], ((tx >> 8) & 255)[..., None]

    def tap(y, x):
        inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        v = full[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        return np.where(inside[..., None], v, f)
    top = (256 - fx) * tap(ky, kx) + fx * tap(ky, kx + 1)
    bot = (256 - fx) * tap(ky + 1, kx) + fx * tap(ky + 1, kx + 1)
    return (((256 - fy) * top + fy * bot + 32768) >> 16).astype(np.uint8)


def elastic_resample(full, row, field, size, cell, fill=255):
    """The definition of the elastic view of an image in numpy: the (h, w, C) uint8 `full` sampled at elastic_coords(row, field, size,
    cell) exactly as affine_resample samples at affine_coords -> (oh, ow, C) uint8."""
    full = np.asarray(full)
    if full.dtype != np.uint8 or full.ndim != 3:
        raise ValueError("elastic_resample is defined on an (h, w, C) uint8 image")
    return _bilinear_at(full, *elastic_coords(row, field, size, cell), fill)


def elastic_nearest(plane, row, field, size, cell, fill=0):
    """The definition of the elastic view of a companion plane in numpy: the element at (Y >> 16, X >> 16) of the (h, w) `plane`, (Y, X)
    = elastic_coords(row, field, size, cell), copied bit for bit; outside the plane `fill`."""
    plane = np.asarray(plane)
    if plane.ndim != 2:
        raise ValueError("elastic_nearest is defined on an (h, w) plane")
    h, w = plane.shape
    Y, X = elastic_coords(row, field, size, cell)
    ky, kx = Y >> 16, X >> 16
    inside = (ky >= 0) & (ky < h) & (kx >= 0) & (kx < w)
    out = np.full(ky.shape, np.asarray(fill).astype(plane.dtype), dtype=plane.dtype)
    out[inside] = plane[ky[inside], kx[inside]]
    return out


def elastic_check_max_d(max_d):
    if isinstance(max_d, bool) or not isinstance(max_d, (int, np.integer)) or not 0 <= int(max_d) <= ELASTIC_MAX_D:
        raise ValueError(f"the bound max_d of an elastic view must be an int in 0 .. {ELASTIC_MAX_D} (source pixels), not {max_d!r}")
    return int(max_d)


def elastic_check_field(field, n, size, cell, max_d):
    """The (n, gh, gw, 2) int32 field of an elastic view of size = (oh, ow), in range, as a contiguous int32 array -- or ValueError: a
    wrong shape (elastic_grid_shape) or a dtype that is not an integer one; a cell that is no power of two in 16 .. 256; max_d outside
    0 .. 8; a control value beyond +-256 max_d, the call's bound (the message names the tile)."""
    what = "the field of an elastic view must hold (dy, dx) per lattice node and tile, in 1/256 source pixel"
    gh, gw = elastic_grid_shape(size, cell)
    max_d = elastic_check_max_d(max_d)
    if field is None:
        raise ValueError(f"{what}: an (N, {gh}, {gw}, 2) int32 array (TileElastic.draw)")
    try:
        f = field.numpy() if hasattr(field, "numpy") and not isinstance(field, np.ndarray) else np.asarray(field)
        if f.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: an (N, {gh}, {gw}, 2) integer array") from None
    if f.shape != (int(n), gh, gw, 2):
        raise ValueError(f"{what}: an ({int(n)}, {gh}, {gw}, 2) array (cell = {int(cell)}), not one of shape {f.shape}")
    f = f.astype(np.int64)
    bad = (np.abs(f) > ELASTIC_UNIT * max_d).reshape(int(n), -1).any(axis=1)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"field: tile {t} of the elastic view has a control displacement of {int(np.abs(f[t]).max())} (1/256 pixel), above "
                         f"the call's bound 256 max_d = {ELASTIC_UNIT * max_d}")
    return np.ascontiguousarray(f.astype(np.int32))


class TileElastic(TileAffine):
    """Elastic deformation -- the U-Net recipe: random displacements on a coarse grid, interpolated smoothly -- on top of TileAffine's
    rotation / zoom / shear / translation / flip, drawn on the host and applied INSIDE the view pass (engine.normalize_view_elastic): the
    image bilinearly (elastic_resample is the definition), its label maps by the nearest element (apply, elastic_nearest), both through
    the same (Y, X).  TileAffine's arguments and defaults, plus
    magnitude: (lo, hi) source pixels, 0 <= lo <= hi <= 8 -- per tile the largest control displacement m is uniform in [lo, hi] and every
    control value uniform in [-m, m]; cell: the lattice spacing in OUTPUT pixels, a power of two from 16 to 256.
    The displacement of an output pixel is a quadratic B-spline of the lattice (C1-smooth; |d| <= m).  Its slope is at most 2 m / cell
    source pixels per output pixel (adjacent control values differ by at most 2 m, and the spline's derivative is a convex combination
    of adjacent differences over a cell), so the CONSTRUCTOR refuses magnitude[1] > cell / 4: below that the slope is at most 1/2 and
    the map cannot fold at the identity.  This is a sufficient bound, not a necessary one; under a zoom that magnifies it is looser still.
    max_d = ceil(magnitude[1]) is the displacement bound of a call whose field lives on the device; `bound` stays TileAffine's."""

    def __init__(self, size=None, rotate=(-180, 180), zoom=(1, 1), shear=(0, 0), translate=(0, 0), flip=True, fill=255, magnitude=(0, 4),
                 cell=32):
        super().__init__(size, rotate, zoom, shear, translate, flip, fill)
        self.cell_log2 = _cell_log2(cell)
        self.cell = int(cell)
        try:
            lo, hi = (float(v) for v in magnitude)
            if not (0.0 <= lo <= hi <= float(ELASTIC_MAX_D)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"magnitude must be a pair (lo, hi) of source pixels with 0 <= lo <= hi <= {ELASTIC_MAX_D}, not "
                             f"{magnitude!r}") from None
        if hi > self.cell / 4.0:
            raise ValueError(f"TileElastic(magnitude={magnitude!r}, cell={cell}) could fold the tile: the spline's slope is at most "
                             f"2 magnitude / cell source pixels per output pixel, and magnitude[1] <= cell / 4 = {self.cell / 4.0:g} keeps it "
                             "at most 1/2 -- lower magnitude[1] or raise cell")
        self.magnitude = (lo, hi)

    @property
    def max_d(self):
        """max_d: an upper bound (source pixels, an int 0 .. 8) of every control displacement this view can draw -- what a call with the
        field on the device sizes its launch from"""
        return int(np.ceil(self.magnitude[1]))

    def draw(self, n, h, w):
        """ElasticWindows(affine, field) from the GLOBAL numpy stream, in this order: TileAffine.draw(n, h, w), unchanged -- six draws
        per tile --; m = np.random.uniform(lo, hi, n); z = np.random.uniform(-1, 1, (n, gh, gw, 2)), (gh, gw) = elastic_grid_shape(
        out_size(h, w), cell).  field = np.rint(256 m z) as int32: |field| <= 256 m <= 256 max_d.  Uniform draws are bounded: nothing is
        clipped or redrawn."""
        affine = super().draw(n, h, w)
        gh, gw = elastic_grid_shape(self.out_size(h, w), self.cell)
        m = np.random.uniform(self.magnitude[0], self.magnitude[1], int(n))
        z = np.random.uniform(-1.0, 1.0, (int(n), gh, gw, 2))
        return ElasticWindows(affine, np.rint(ELASTIC_UNIT * m[:, None, None, None] * z).astype(np.int32))

    def apply(self, planes, windows=None, fill=0, out=None):
        """TileAffine.apply through an elastic view (sl_view_planes_elastic): `windows` is the ElasticWindows the image call with this
        view returned for (H, W) tiles (or self.draw(N, H, W)); per element the NEAREST source element at the image's own (Y, X)
        (elastic_nearest), a bit copy, outside the plane `fill`.  Nothing is drawn here.  Host windows are range-checked (ValueError);
        device windows are taken as they are under this view's bound and max_d."""
        from . import engine
        if windows is None:
            raise ValueError("windows is required: pass the ElasticWindows the image call with this view returned, or view.draw(N, H, W) "
                             "-- apply draws nothing itself")
        affine, field = engine._elastic_parts(windows)
        max_r, max_d = engine._elastic_bound(self, windows)
        return engine.view_planes_elastic(planes, affine, field, self.size, self.cell, max_r, max_d, fill=fill, out=out)

    def __repr__(self):
        return (f"TileElastic(size={self.size}, rotate={self.rotate}, zoom={self.zoom}, shear={self.shear}, translate={self.translate}, "
                f"flip={self.flip}, fill={self.fill}, magnitude={self.magnitude}, cell={self.cell})")

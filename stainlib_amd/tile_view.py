"""TileView: the geometric half of a training loader's augmentation -- a random crop, a random flip and a random quarter turn, different
for every tile -- drawn on the host and applied INSIDE the apply pass (engine.normalize_view, sl_normalize_view): only the window's
pixels are read, computed and written, and the model-ready tensor comes out cropped, flipped and turned.

A view of one tile is (y0, x0, d): the window's corner in the tile and a dihedral code d = k | 4 f -- f: flip along the width FIRST,
then k quarter turns counter-clockwise (torch.rot90(., k, dims=(0, 1)) of the (H, W, 3) image).  The output size (oh, ow) is one for
the whole batch, so a code with odd k takes an (ow, oh) window.

shrink = s in {1, 2, 4} is a change of magnification in the same pass (sl_normalize_view_shrink): the window is s times the output in
both directions, and every output pixel is the rounded mean of an s x s box of the image at source resolution -- per channel
(sum + s s / 2) >> (2 log2 s) of the uint8 bytes, boxes counted from the window's corner (any pixel, not only a multiple of s).
"""
from __future__ import annotations

import numpy as np

SHRINKS = (1, 2, 4)


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


class TileView(object):
    """size: None (the full tile), an int or (oh, ow) -- the size of the OUTPUT.  flip: draw flips.  rot90: draw quarter turns (the
    view must then fit transposed as well).  Half turns are drawn whenever flips are: a flip along the height is a flip along the
    width and a half turn.  shrink: 1, 2 or 4 -- the window is shrink times the output, averaged down in boxes (see the module);
    size=None is then (h // shrink, w // shrink)."""

    def __init__(self, size=None, flip=True, rot90=True, shrink=1):
        self.size = None if size is None else _size2(size)
        self.flip = bool(flip)
        self.rot90 = bool(rot90)
        self.shrink = check_shrink(shrink)

    @property
    def d_mask(self):
        return (4 if self.flip else 0) | (3 if self.rot90 else 2 if self.flip else 0)

    @property
    def codes(self):
        """the dihedral codes this view draws from, ascending"""
        return [c for c in range(8) if c & ~self.d_mask == 0]

    def out_size(self, h, w):
        return check_size(self.size, h, w, self.d_mask, self.shrink)

    def draw(self, n, h, w):
        """(n, 3) int32: y0, x0, d per tile, from the GLOBAL numpy stream (the convention of StainJitter.draw).  Per tile, in order:
        d = the np.random.randint(len(codes))-th code; y0 = np.random.randint(0, h - s wh + 1); x0 = np.random.randint(0, w - s ww + 1),
        (wh, ww) the output size as that code's window sees it and s the shrink."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        oh, ow = self.out_size(h, w)
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

    def __repr__(self):
        return f"TileView(size={self.size}, flip={self.flip}, rot90={self.rot90}" + (f", shrink={self.shrink})" if self.shrink != 1 else ")")

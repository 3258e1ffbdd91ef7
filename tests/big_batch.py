"""Helpers of the big-batch tests (tests/test_gpu_big_batch.py, tests/test_gpu_big_shard.py): batches whose byte offsets pass 2^31 and
2^32, checked without ever bringing them to the host.

A batch is K distinct tiles repeated: tile i of the batch is tile i % K of the base.  Every per-tile entry point must then give tile
i + K the bytes (and the side results) of tile i -- one device-side torch.equal of the batch against itself, K tiles on -- and the
first K tiles are held to the oracle under the bar the project states for that entry point.  A 32-bit product in an address shows as a
tile that is not its twin (neither 2^31 nor 2^32 bytes is a whole number of tiles or of K tiles into the batches below, so a write
that wraps lands mid-tile in a tile of another class), a shift common to every tile as a miss of the anchor.

Nothing here needs a GPU to import; every check works on whatever device its tensors live on (the CPU tests of the checker itself:
tests/test_big_batch_checker.py)."""
import numpy as np
import pytest
import torch

from oracle import stain_oracle as so

K = 4                       # distinct tiles of a batch
SENTINEL = 77               # exactly representable in uint8, float16, bfloat16, float32 (tests/test_gpu_jitter.py)
# (h, w, n): the smallest batches of K-periodic tiles that cross both 2^31 and 2^32 bytes.
#   aligned  3 P = 786 432 bytes: 2^31 falls inside tile 2730, 2^32 inside tile 5461
#   odd      3 P = 789 459 bytes, odd: every other tile starts at an odd byte; 2^32 falls inside tile 5440
SHAPES = {"aligned": (512, 512, 5464), "odd": (509, 517, 5444)}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def base_tiles(h, w):
    """The K = 4 distinct tiles, (4, h, w, 3) uint8 numpy: a synthetic H&E tile, a structured tile with saturated white background, a
    darkened synthetic tile with statistics of its own (_tiles of tests/test_gpu_lab_view.py) and an all-white tile (empty tissue mask:
    the fits fail on it and the apply passes copy it through)."""
    dark = (so.synth_tile(h, w, 47 + h).astype(np.float64) * 0.82).astype(np.uint8)
    return np.stack([so.synth_tile(h, w, 40 + h), so.structured_tile("white_bg", h, w, 5), dark, np.full((h, w, 3), 255, dtype=np.uint8)])


def periodic_batch(base, n):
    """base: (K, ...) tensor of K distinct tiles -> base[arange(n) % K], contiguous, on base's device"""
    idx = torch.arange(n, device=base.device) % base.shape[0]
    return base.index_select(0, idx).contiguous()


def periodic_rows(rows, n):
    """per-tile arguments with the batch's period: rows (K, ...) -> (n, ...)"""
    return periodic_batch(rows, n)


def bits(t):
    """t as integers of its element size: comparisons that are NaN-safe and see the sign of zero (_same_f64 of test_gpu_lab_view.py)"""
    return t if not t.is_floating_point() else t.view(_INT_VIEW[t.element_size()])


def first_mismatch(a, b):
    """index along dim 0 of the first slice where a and b differ in a bit, or None (a, b: same shape; works slice by slice)"""
    step = max(1, (1 << 28) // max(1, a[0].numel()))
    for i0 in range(0, a.shape[0], step):
        ne = (bits(a[i0:i0 + step]) != bits(b[i0:i0 + step])).reshape(min(step, a.shape[0] - i0), -1).any(dim=1)
        if bool(ne.any()):
            return i0 + int(torch.nonzero(ne)[0])
    return None


def assert_periodic(out, period=K, label=""):
    """out: a tensor with the tile on its first axis, or a tuple / list of such (the side results: status, M, maxC, statistics, sums,
    applied, p).  Asserts out[period:] == out[:-period] bit for bit along the tile axis, on the tensor's device, with one torch.equal."""
    if isinstance(out, (tuple, list)):
        for k, t in enumerate(out):
            if t is not None:
                assert_periodic(t, period, f"{label}[{k}]")
        return
    assert out.shape[0] > period, label
    a, b = bits(out)[period:], bits(out)[:-period]
    if not torch.equal(a, b):
        t = first_mismatch(a, b)
        raise AssertionError(f"{label}: tile {t + period} differs from tile {t} ({tuple(out.shape)} {out.dtype}, period {period})")


class Guarded:
    """An output body of `numel` elements inside a buffer with `margin` bytes of SENTINEL before (plus out_off elements) and after it
    (_guarded of tests/test_gpu_lab_view.py, shareable; the body is pre-filled with SENTINEL too, so a region nothing wrote shows in
    the comparison that follows).  check() -- after the call -- asserts that both margins still hold SENTINEL, on the buffer's
    device."""

    def __init__(self, numel, dtype, out_off=0, margin=16, device="cuda"):
        esize = torch.empty((), dtype=dtype).element_size()
        assert margin % 16 == 0
        self.start, self.numel = margin // esize + out_off, numel
        self.buf = torch.full((self.start + numel + margin // esize,), SENTINEL, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.body = self.buf[self.start:self.start + numel]

    def image(self, n, oh, ow, fmt=None):
        """the body as the output of an image pass: (n, oh, ow, 3) uint8 without a format, else (n, 3, oh, ow) in the format's layout"""
        if fmt is None:
            return self.body.view(n, oh, ow, 3)
        if fmt.channels_last:
            return self.body.view(n, oh, ow, 3).permute(0, 3, 1, 2)
        return self.body.view(n, 3, oh, ow)

    def check(self, label=""):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        before, after = self.buf[:self.start], self.buf[self.start + self.numel:]
        assert bool((before == SENTINEL).all()) and bool((after == SENTINEL).all()), f"{label}: written outside the output"


def guarded(numel, dtype, out_off=0, margin=16, device="cuda"):
    return Guarded(numel, dtype, out_off, margin, device)


def need_memory(nbytes, resident=0):
    """nbytes: everything on the device while the test runs, `resident` of it there already (shared batches).  No test may hold more
    than 40 GB; skip, with the figure, when the device shows less free memory than the rest needs."""
    assert nbytes <= 40 * 10 ** 9, f"a big-batch test may hold at most 40 GB, not {nbytes / 1e9:.1f}"
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes - resident:
        pytest.skip(f"needs {(nbytes - resident) / 1e9:.1f} GB more of device memory, {free / 1e9:.1f} GB free")


def release():
    """what every big-batch test ends with (its own references are gone when it returns)"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def period8_windows(n, h, w, oh, ow):
    """(n, 3) int32 windows of period 8 over the tiles: all eight dihedral codes, corners that include the tile's last row and last
    column, odd and even x0"""
    win = np.empty((8, 3), dtype=np.int32)
    for t in range(8):
        wh, ww = (ow, oh) if t & 1 else (oh, ow)
        ymax, xmax = h - wh, w - ww
        y0, x0 = [(0, 0), (0, xmax), (ymax, 0), (ymax, xmax), (ymax, xmax // 2 | 1), (ymax // 2, xmax), (1, 2), (ymax - 1, xmax - 1)][t]
        win[t] = (y0, x0, t)
    return win[np.arange(n) % 8]


def period8_resize_windows(n, h, w):
    """(n, 5) int32 windows (y0, x0, d, wh, ww) of a resizing view with period 8 over the tiles: the eight codes; 64 x 64 windows
    (tiles 0 .. 3 of a period) and 128 x 96 ones (4 .. 7) at period8_windows' corners, the tile's last row and last column among them.
    The call's bound of the window sides is (128, 96)."""
    win = np.empty((8, 5), dtype=np.int32)
    for t in range(8):
        wh, ww = (64, 64) if t < 4 else (128, 96)
        ymax, xmax = h - wh, w - ww                          # (the sides are the TILE's, whatever the code)
        y0, x0 = [(0, 0), (0, xmax), (ymax, 0), (ymax, xmax), (ymax, xmax // 2 | 1), (ymax // 2, xmax), (1, 2), (ymax - 1, xmax - 1)][t]
        win[t] = (y0, x0, t, wh, ww)
    assert (win[:, 0] + win[:, 3] <= h).all() and (win[:, 1] + win[:, 4] <= w).all() and (win[:, 0] + win[:, 3] == h).any() \
        and (win[:, 1] + win[:, 4] == w).any()
    return win[np.arange(n) % 8]


# the dihedral code d as the matrix (a00, a01, a10, a11) / Q of an affine view: rot90(flip_w(window) if d & 4 else window, d & 3)
AFFINE_DIHEDRAL = {0: (1, 0, 0, 1), 1: (0, 1, -1, 0), 2: (-1, 0, 0, -1), 3: (0, -1, 1, 0), 4: (1, 0, 0, -1), 5: (0, 1, 1, 0), 6: (-1, 0, 0, 1),
                   7: (0, -1, -1, 0)}


def period8_affine_windows(n, h, w, oh, ow, kind):
    """(n, 6) int32 rows (cy, cx, a00, a01, a10, a11; 2^-16 source pixels) of an affine view with period 8 over the tiles.
    kind "dihedral": the eight dihedral matrices about period8_windows' corner windows -- the plain view's bits.
    kind "rotated": 30 and 45 degrees centred so that the patch reaches past the tile's last row and last column, a centre half
    outside the tile (rotated, fractional), 30 degrees at the first row and column, a shear, a negative determinant, the row-sum limit
    (45 degrees at sqrt 2) and the identity about a fractional centre."""
    Q = 65536
    if kind == "dihedral":
        rows = []
        for y0, x0, d in period8_windows(8, h, w, oh, ow).tolist():
            wh, ww = (ow, oh) if d & 1 else (oh, ow)
            rows.append([(2 * y0 + wh) * Q // 2, (2 * x0 + ww) * Q // 2] + [Q * v for v in AFFINE_DIHEDRAL[d]])
    else:
        def rot(deg, z=1.0):
            c, s = np.cos(np.radians(deg)) / z, np.sin(np.radians(deg)) / z
            return (c, -s, s, c)
        r = max(oh, ow) / 2.0
        reach30, reach45 = r * (np.cos(np.radians(30)) + np.sin(np.radians(30))), r * np.sqrt(2.0)
        rows = [(h - reach30 + 4, w - reach30 + 4) + rot(30), (h - reach45 + 3, w - reach45 + 3) + rot(45),
                (0.25, w / 2 + 0.3701) + rot(-17, 1.1), (reach30 - 4, reach30 - 4) + rot(30), (h / 2, w / 2, 1, 0.4, 0.1, 0.9),
                (h - 50, 50, 0.8, 0.3, 0.2, -1.1), (h / 2, w / 2, 1, -1, 1, 1), (h / 2 + 0.5, w / 2 + 0.25, 1, 0, 0, 1)]
        rows = [[int(np.rint(Q * v)) for v in row] for row in rows]
    win = np.array(rows, dtype=np.int64)
    assert win.shape == (8, 6) and int(np.abs(win[:, 2:]).reshape(8, 2, 2).sum(axis=2).max()) <= 2 * Q
    return win.astype(np.int32)[np.arange(n) % 8]

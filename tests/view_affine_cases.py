"""Helpers of the affine-view edge tests (tests/test_gpu_view_affine_edges.py, tests/test_view_affine_cases.py): seeded random affine
rows up to the row-sum limit, random-byte tiles distinct per tile, and the numpy reference of a case, made once and shared.

A case is (h, w, (oh, ow)): N = 64 tiles of h x w random bytes, one random matrix each -- in the spirit of the last loop of
tests/view_affine_geometry.cpp: the row sums ry, rx uniform in [0, 2 Q), split at a random point between the two entries of a row,
with random signs; the centre uniform over the tile stretched by 20 % on every side, at the full 2^-16 resolution.  A small matrix
about a centre outside the tile gives a tile of fill alone, and two of those are the same tile: a row whose reference tile repeats an
earlier tile of its case is drawn again, so a case keeps at most one tile of fill alone and a wrong tile index cannot pass.  Nothing
here needs a GPU to import."""
import types

import numpy as np

from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_check_windows, affine_nearest, affine_resample, affine_row_sums

N = 64
FILL = (10, 30, 200)
# (h, w) -> output sizes.  Between them: tiles of 3, 6 and 9 bytes (load12's byte path) and of 12 exactly; tiles narrower than a chunk;
# odd widths (rows start at every residue mod 4); source blocks that are the whole tile, or 64 wide inside a wider tile; ow % 4 of 0,
# 1, 2 and 3; second patches 1, 2 and 3 outputs wide (65, 66 and 67 outputs against patch edges of 32 .. 64).
CASES = [(1, 1, (1, 1)), (1, 1, (5, 3)), (1, 2, (3, 5)), (1, 3, (2, 7)), (2, 2, (4, 4)), (9, 11, (5, 7)), (9, 11, (13, 66)), (5, 67, (7, 65)),
         (67, 5, (66, 6)), (81, 151, (33, 37)), (81, 151, (70, 67))]
PLANE_CASES = [(1, 1, (5, 3)), (1, 3, (2, 7)), (9, 11, (13, 66)), (5, 67, (7, 65)), (81, 151, (33, 37))]
SEED = 20240
_CACHE = {}


def case_id(case):
    h, w, (oh, ow) = case
    return f"{h}x{w}-{oh}x{ow}"


def random_rows(rng, n, h, w):
    """(n, 6) int32 rows (cy, cx, a00, a01, a10, a11): see the module docstring"""
    rows = np.empty((n, 6), dtype=np.int64)
    rows[:, 0] = rng.randint(-(h * Q) // 5, h * Q + (h * Q) // 5 + 1, n)
    rows[:, 1] = rng.randint(-(w * Q) // 5, w * Q + (w * Q) // 5 + 1, n)
    for k in (2, 4):
        r = rng.randint(0, AFFINE_MAX_R, n)                                      # [0, 2 Q)
        a = np.minimum((r * rng.uniform(size=n)).astype(np.int64), r)
        rows[:, k] = a * rng.choice((-1, 1), n)
        rows[:, k + 1] = (r - a) * rng.choice((-1, 1), n)
    assert int(affine_row_sums(rows).max()) < AFFINE_MAX_R
    return rows.astype(np.int32)


def case_data(case):
    """tiles (N, h, w, 3) uint8, rows (N, 6) int32 -- passed through affine_check_windows --, want (N, oh, ow, 3) uint8: the definition
    (affine_resample) under FILL, and mixed: how many reference tiles hold both fill and non-fill pixels"""
    if case not in _CACHE:
        h, w, size = case
        rng = np.random.RandomState(SEED + CASES.index(case))
        tiles = rng.randint(0, 256, (N, h, w, 3)).astype(np.uint8)
        rows, want, seen = [], [], set()
        for t in range(N):                                   # a row whose reference tile repeats an earlier one is drawn again: see above
            for _ in range(100):
                row = random_rows(rng, 1, h, w)[0]
                ref = affine_resample(tiles[t], row, size, FILL)
                if ref.tobytes() not in seen:
                    break
            else:
                raise AssertionError(f"{case_id(case)}: no row of tile {t} gives a reference tile of its own")
            seen.add(ref.tobytes())
            rows.append(row)
            want.append(ref)
        rows, want = affine_check_windows(np.stack(rows), N, h, w, size), np.stack(want)
        is_fill = (want == np.array(FILL, dtype=np.uint8)).all(axis=-1).reshape(N, -1)
        mixed = int((is_fill.any(axis=1) & ~is_fill.all(axis=1)).sum())
        for a in (tiles, rows, want):
            a.setflags(write=False)
        _CACHE[case] = types.SimpleNamespace(h=h, w=w, size=size, tiles=tiles, rows=rows, want=want, mixed=mixed)
    return _CACHE[case]


def check_case(case):
    """the conditions a case's draw must meet, so that no comparison passes on a degenerate one"""
    C = case_data(case)
    assert len({C.tiles[t].tobytes() for t in range(N)}) == N and len({C.want[t].tobytes() for t in range(N)}) == N, case_id(case)
    if case != (1, 1, (1, 1)):
        assert C.mixed >= 16, f"{case_id(case)}: {C.mixed} of {N} reference tiles hold both fill and non-fill pixels"
    return C


def plane_bits(case, c, es):
    """random planes of a case as unsigned integers of es bytes: (N, c, h, w), the case's rows beside them (a seed of their own)"""
    h, w, _ = case
    rng = np.random.RandomState(SEED + 100 + 10 * PLANE_CASES.index(case) + es)
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[es]
    return rng.randint(0, 256, (N, c, h, w, es)).astype(np.uint8).view(dt)[..., 0]


def planes_want(bits, rows, size, fill_bits):
    """affine_nearest per tile and plane on the integer view -> (N, c, oh, ow)"""
    n, c = bits.shape[:2]
    return np.stack([np.stack([affine_nearest(bits[t, k], rows[t], size, fill_bits) for k in range(c)]) for t in range(n)])

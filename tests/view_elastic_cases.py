"""Helpers of the elastic-view edge tests (tests/test_gpu_view_elastic_edges.py, tests/test_view_elastic_cases.py), in the style of
tests/view_affine_cases.py: per case (h, w, (oh, ow)) N = 64 tiles of random bytes, one random affine row each (random_rows: up to
the row-sum limit, the centre anywhere over the stretched tile) plus one random control lattice within +-256 MAX_D at the smallest
cell, and the numpy reference of the case (stainlib_amd.tile_view.elastic_resample: the definition), made once and shared.  A row and
field whose reference tile repeats an earlier tile of its case are drawn again, so that a wrong tile index cannot pass.  Nothing here
needs a GPU to import."""
import types

import numpy as np

from stainlib_amd.tile_view import affine_check_windows, elastic_check_field, elastic_grid_shape, elastic_nearest, elastic_resample
from tests.view_affine_cases import FILL, N, random_rows

# a tile of 3 bytes under an output larger than itself; a tile narrower than a patch with a second patch 2 outputs wide; a tile wider
# than the 64-pixel block with 2 x 2 patches even at the identity (47 outputs at MAX_D = 8) and ow % 4 = 3
CASES = [(1, 1, (5, 3)), (9, 11, (13, 66)), (81, 151, (70, 67))]
CELL = 16
MAX_D = 8
SEED = 31070
_CACHE = {}


def case_id(case):
    h, w, (oh, ow) = case
    return f"{h}x{w}-{oh}x{ow}"


def case_data(case):
    """tiles (N, h, w, 3) uint8, rows (N, 6) int32, field (N, gh, gw, 2) int32 -- passed through the host checks --, want (N, oh, ow, 3)
    uint8: the definition under FILL, and mixed: how many reference tiles hold both fill and non-fill pixels"""
    if case not in _CACHE:
        h, w, size = case
        rng = np.random.RandomState(SEED + CASES.index(case))
        tiles = rng.randint(0, 256, (N, h, w, 3)).astype(np.uint8)
        shape = elastic_grid_shape(size, CELL) + (2,)
        rows, fields, want, seen = [], [], [], set()
        for t in range(N):
            for _ in range(100):
                row = random_rows(rng, 1, h, w)[0]
                field = rng.randint(-256 * MAX_D, 256 * MAX_D + 1, shape).astype(np.int32)
                ref = elastic_resample(tiles[t], row, field, size, CELL, FILL)
                if ref.tobytes() not in seen:
                    break
            else:
                raise AssertionError(f"{case_id(case)}: no draw of tile {t} gives a reference tile of its own")
            seen.add(ref.tobytes())
            rows.append(row)
            fields.append(field)
            want.append(ref)
        rows, field, want = affine_check_windows(np.stack(rows), N, h, w, size), elastic_check_field(np.stack(fields), N, size, CELL, MAX_D), np.stack(want)
        is_fill = (want == np.array(FILL, dtype=np.uint8)).all(axis=-1).reshape(N, -1)
        mixed = int((is_fill.any(axis=1) & ~is_fill.all(axis=1)).sum())
        for a in (tiles, rows, field, want):
            a.setflags(write=False)
        _CACHE[case] = types.SimpleNamespace(h=h, w=w, size=size, tiles=tiles, rows=rows, field=field, want=want, mixed=mixed)
    return _CACHE[case]


def check_case(case):
    """the conditions a case's draw must meet, so that no comparison passes on a degenerate one: at least 16 of the 64 reference tiles
    hold both fill and non-fill pixels (not asked of the 1 x 1 tile), and no two reference tiles are equal"""
    C = case_data(case)
    assert len({C.tiles[t].tobytes() for t in range(N)}) == N and len({C.want[t].tobytes() for t in range(N)}) == N, case_id(case)
    if (C.h, C.w) != (1, 1):
        assert C.mixed >= 16, f"{case_id(case)}: {C.mixed} of {N} reference tiles hold both fill and non-fill pixels"
    return C


def planes_want(bits, C, fill_bits):
    """elastic_nearest per tile and plane on an integer view (N, c, h, w) -> (N, c, oh, ow)"""
    n, c = bits.shape[:2]
    return np.stack([np.stack([elastic_nearest(bits[t, k], C.rows[t], C.field[t], C.size, CELL, fill_bits) for k in range(c)]) for t in range(n)])

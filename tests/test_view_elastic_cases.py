"""The inputs of tests/test_gpu_view_elastic_edges.py do what they were drawn for (tests/view_elastic_cases.py): checked on the numpy
reference, so that no device comparison can pass on a degenerate draw.  No GPU needed."""
import numpy as np
import pytest

from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_resample, affine_row_sums, elastic_displacement
from tests.view_affine_cases import FILL, N
from tests.view_elastic_cases import CASES, CELL, MAX_D, case_data, case_id, check_case


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_has_distinct_reference_tiles_and_enough_that_mix_fill_and_image(case):
    C = check_case(case)
    h, w, size = case
    assert C.rows.shape == (N, 6) and C.rows.dtype == np.int32 and C.field.dtype == np.int32 and C.want.shape == (N, *size, 3)
    assert 256 * (MAX_D - 1) < np.abs(C.field).max() <= 256 * MAX_D and CELL == 16          # (the tightest max_d of the call is MAX_D)
    # the field matters: the reference differs from the affine view of the same row wherever the tile shows (any tile larger than a pixel)
    moved = sum(not np.array_equal(C.want[t], affine_resample(C.tiles[t], C.rows[t], size, FILL)) for t in range(N))
    d = np.abs(elastic_displacement(C.field[0], size, CELL)).max()
    print(f"{case_id(case)}: {C.mixed} of {N} reference tiles mix fill and image, {moved} differ from their affine view, largest row sum "
          f"{affine_row_sums(C.rows).max() / Q:.3f} Q, largest displacement of tile 0 {d / 256:.2f} px")
    if (h, w) != (1, 1):
        assert moved >= N // 2


def test_the_row_sums_reach_the_limit():
    assert 1.9 * Q < max(int(affine_row_sums(case_data(c).rows).max()) for c in CASES) <= AFFINE_MAX_R

"""The inputs of tests/test_gpu_view_affine_edges.py do what they were drawn for (tests/view_affine_cases.py): checked on the numpy
reference, so that no device comparison can pass on a degenerate draw.  No GPU needed."""
import numpy as np
import pytest

from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_check_windows, affine_row_sums
from tests.view_affine_cases import CASES, FILL, N, PLANE_CASES, case_data, case_id, check_case, plane_bits, planes_want


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_has_distinct_tiles_and_enough_that_mix_fill_and_image(case):
    C = check_case(case)
    h, w, size = case
    assert C.rows.shape == (N, 6) and C.rows.dtype == np.int32 and C.want.shape == (N, *size, 3)
    assert np.array_equal(affine_check_windows(C.rows, N, h, w, size), C.rows)
    cy, cx = C.rows[:, 0].astype(np.int64), C.rows[:, 1].astype(np.int64)
    assert cy.min() >= -(h * Q) // 5 and cy.max() <= h * Q + (h * Q) // 5 and cx.min() >= -(w * Q) // 5 and cx.max() <= w * Q + (w * Q) // 5
    if h * w >= 99:
        assert (cy < 0).any() and (cy > h * Q).any() and (cy & 0xff).any()       # outside on both sides, below the weights' resolution
    print(f"{case_id(case)}: {C.mixed} of {N} reference tiles mix fill and image, largest row sum {affine_row_sums(C.rows).max() / Q:.3f} Q")


def test_the_row_sums_reach_the_limit_and_the_cases_cover_what_they_claim():
    assert max(int(affine_row_sums(case_data(c).rows).max()) for c in CASES) > 1.9 * Q
    assert max(int(affine_row_sums(case_data(c).rows).max()) for c in CASES) <= AFFINE_MAX_R
    assert {3 * h * w for h, w, _ in CASES} >= {3, 6, 9, 12} and {ow % 4 for _, _, (_, ow) in CASES} == {0, 1, 2, 3}
    assert {ow - 64 for _, _, (_, ow) in CASES if ow > 64} == {1, 2, 3} and all(c in CASES for c in PLANE_CASES)
    assert len(FILL) == 3 and len(set(FILL)) == 3


@pytest.mark.parametrize("case", PLANE_CASES, ids=case_id)
def test_plane_references_hold_fill_and_elements(case):
    C = case_data(case)
    for es, fill in ((1, 1), (2, 0xC020), (8, 2 ** 63 + 5)):
        bits = plane_bits(case, 2, es)
        want = planes_want(bits, C.rows, C.size, fill)
        assert want.shape == (N, 2, *C.size) and want.dtype == bits.dtype and (want == fill).any() and (want != fill).any()
        assert not np.array_equal(want[:, 0], want[:, 1])

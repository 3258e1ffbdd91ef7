"""-m gpu: the elastic kernels (sl_normalize_view_elastic, sl_view_planes_elastic) at the edges tests/test_gpu_view_elastic.py leaves out:
random matrices up to the row-sum limit under random fields at max_d = 8, 64 tiles per call, on a tile of 3 bytes, a tile narrower than
a patch and a tile wider than the LDS block; outputs larger than the tile, ow % 4 of 2 and 3, second patches 2 and more outputs wide;
every output form, the input at an aligned address and one byte past it.

The cases, their rows, fields and numpy reference (stainlib_amd.tile_view.elastic_resample / elastic_nearest: the definition) come from
tests/view_elastic_cases.py, made once per case and shared; tests/test_view_elastic_cases.py holds their draw to what it was made for.
Integer arithmetic on bytes: every element of every output is compared, exactly."""
import numpy as np
import pytest
import torch

from stainlib_amd import engine
from stainlib_amd.tile_view import AFFINE_MAX_R, affine_row_sums
from tests.test_gpu_jitter import _dev_tiles, _formats, _same_bits
from tests.view_affine_cases import FILL, N
from tests.view_elastic_cases import CASES, CELL, MAX_D, case_id, check_case, planes_want

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_random_matrices_and_fields_every_output_form(case):
    C = check_case(case)                                      # distinct reference tiles, enough that mix fill and image
    want = torch.tensor(C.want)
    fmts = [None] + _formats()
    wants = [want] + [f.convert(want.cuda()).cpu() for f in fmts[1:]]
    for in_off in (0, 1):
        dev = _dev_tiles(torch.tensor(C.tiles), in_off)
        assert dev.data_ptr() % 4 == in_off
        for fmt, wt in zip(fmts, wants):
            got = engine.normalize_view_elastic(dev, C.rows, C.field, C.size, CELL, AFFINE_MAX_R, MAX_D, FILL, fmt=fmt).cpu()
            assert _same_bits(got, wt), f"{case_id(case)} in+{in_off} {fmt}"
    # both parts on the device; the tightest max_r of the call (fewer, larger patches where the matrices allow)
    got = engine.normalize_view_elastic(dev, torch.tensor(C.rows).cuda(), torch.tensor(C.field).cuda(), C.size, CELL, AFFINE_MAX_R, MAX_D, FILL)
    assert torch.equal(got.cpu(), want)
    tight = max(1, int(affine_row_sums(C.rows).max()))
    assert tight < AFFINE_MAX_R
    assert torch.equal(engine.normalize_view_elastic(dev, C.rows, C.field, C.size, CELL, tight, MAX_D, FILL).cpu(), want)


@pytest.mark.parametrize("dtype,fill", [(torch.bool, True), (torch.int16, -12345), (torch.float64, -1e300)])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_planes_at_the_edges(case, dtype, fill):
    C = check_case(case)
    es = torch.empty((), dtype=dtype).element_size()
    ints = {1: torch.uint8, 2: torch.int16, 8: torch.int64}[es]
    rng = np.random.RandomState(5 + es)
    dt = {1: np.uint8, 2: np.uint16, 8: np.uint64}[es]
    bits = rng.randint(0, 256, (N, 2, C.h, C.w, es)).astype(np.uint8).view(dt)[..., 0]
    if dtype == torch.bool:
        bits = bits & 1
    fl = int(torch.tensor([fill], dtype=dtype).view(ints)[0]) & ((1 << (8 * es)) - 1)
    want = planes_want(bits, C, fl)
    assert (want == fl).any() and (want != fl).any()
    signed = {1: np.uint8, 2: np.int16, 8: np.int64}[es]
    planes = torch.from_numpy(bits.view(signed)).view(dtype).cuda()
    for rows, field in ((C.rows, C.field), (torch.tensor(C.rows).cuda(), torch.tensor(C.field).cuda())):
        got = engine.view_planes_elastic(planes, rows, field, C.size, CELL, AFFINE_MAX_R, MAX_D, fill=fill).cpu()
        assert got.dtype == dtype and np.array_equal(got.view(ints).numpy(), want.view(signed)), f"{case_id(case)} {dtype}"

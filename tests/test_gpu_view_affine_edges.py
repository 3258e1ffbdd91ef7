"""-m gpu: the affine kernels (sl_normalize_view_affine, sl_view_planes_affine) at the edges tests/test_gpu_view_affine.py leaves out:
random matrices up to the row-sum limit, 64 tiles per call, on tiles of 3 to 12 bytes, tiles narrower than a chunk, odd widths, outputs
of one pixel and outputs larger than the tile, every ow % 4, second patches 1, 2 and 3 outputs wide; every output form at both output
alignments behind sentinel margins (tests/test_gpu_view_routes.py: _affine_view), the input at an aligned address and one byte past it.

The cases, their rows and their numpy reference (stainlib_amd.tile_view.affine_resample / affine_nearest: the definition) come from
tests/view_affine_cases.py, made once per case and shared; tests/test_view_affine_cases.py holds their draw to what it was made for.
Integer arithmetic on bytes: every element of every output is compared, exactly."""
import numpy as np
import pytest
import torch

from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_resample, affine_row_sums
from tests.test_gpu_jitter import SENTINEL, _dev_tiles, _formats, _same_bits
from tests.test_gpu_view_routes import _affine_view
from tests.view_affine_cases import CASES, FILL, N, PLANE_CASES, case_data, case_id, check_case, plane_bits, planes_want

pytestmark = pytest.mark.gpu

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---- 1. random matrices, many tiles per call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_random_matrices_every_output_form_and_alignment(case):
    C = check_case(case)                                      # distinct tiles, distinct reference tiles, enough that mix fill and image
    want = torch.tensor(C.want)
    fmts = [None] + _formats()
    wants = [want] + [f.convert(want.cuda()).cpu() for f in fmts[1:]]
    for in_off in (0, 1):
        dev = _dev_tiles(torch.tensor(C.tiles), in_off)
        assert dev.data_ptr() % 4 == in_off
        for fmt, wt in zip(fmts, wants):
            for off in (0, 1):
                got = _affine_view(dev, C.rows, C.size, fmt, out_off=off)
                assert _same_bits(got, wt), f"{case_id(case)} in+{in_off} {fmt} out+{off}"
    # the windows on the device; the tightest bound of the call (fewer, larger patches where the matrices allow)
    assert torch.equal(_affine_view(dev, torch.tensor(C.rows).cuda(), C.size), want)
    tight = max(1, int(affine_row_sums(C.rows).max()))
    assert tight < AFFINE_MAX_R
    for fmt, wt in ((None, want), (fmts[4], wants[4])):
        assert _same_bits(_affine_view(dev, C.rows, C.size, fmt, out_off=1, max_r=tight), wt), f"{case_id(case)} max_r={tight} {fmt}"


def test_the_row_sums_reach_the_limit():
    assert max(int(affine_row_sums(case_data(c).rows).max()) for c in CASES) > 1.9 * Q


# ---- 2. the forms of size= and fill= ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[5], CASES[9]], ids=case_id)
def test_size_and_fill_forms(case):
    C = case_data(case)
    h, w = C.h, C.w
    dev = _dev_tiles(torch.tensor(C.tiles), 1)
    fmt = _formats()[3]

    def want(size, fill):
        return torch.from_numpy(np.stack([affine_resample(C.tiles[t], C.rows[t], size, fill) for t in range(N)]))

    for size, full_size, fill in ((None, (h, w), FILL), (7, (7, 7), FILL), (C.size, C.size, 99), (C.size, C.size, (0, 0, 0)),
                                  (C.size, C.size, (255, 255, 255))):
        wt = want(full_size, fill)
        f3 = (fill,) * 3 if isinstance(fill, int) else fill
        is_fill = (wt == torch.tensor(f3, dtype=torch.uint8)).all(dim=-1)
        assert tuple(wt.shape) == (N, *full_size, 3) and bool(is_fill.any()) and not bool(is_fill.all())
        for off in (0, 1):
            assert torch.equal(_affine_view(dev, C.rows, size, out_off=off, fill=fill), wt), f"{case_id(case)} size={size} fill={fill} out+{off}"
            assert _same_bits(_affine_view(dev, C.rows, size, fmt, out_off=off, fill=fill), fmt.convert(wt.cuda()).cpu())
    assert not torch.equal(want(C.size, (0, 0, 0)), want(C.size, (255, 255, 255)))


# ---- 3. companion planes at the same edges ----------------------------------------------------------------------------------------------------
def _guarded_planes(shape, dtype, out_off):
    """(buffer of SENTINEL in the integer type of the element size, start, numel, the contiguous out= tensor of `shape` and `dtype` that
    starts 16 bytes + out_off elements into it); 16 more bytes lie behind the output"""
    es = torch.empty((), dtype=dtype).element_size()
    numel = int(np.prod(shape))
    start = 16 // es + out_off
    buf = torch.full((start + numel + 16 // es,), SENTINEL, dtype=_INT[es], device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[start:start + numel].view(dtype).view(shape)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + start * es
    return buf, start, numel, out


@pytest.mark.parametrize("dtype,fill", [(torch.bool, True), (torch.int8, -7), (torch.bfloat16, -2.5), (torch.float64, -1e300), (torch.int16, -12345)])
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("case", PLANE_CASES, ids=case_id)
def test_planes_at_the_edges_into_a_guarded_buffer(case, c, dtype, fill):
    from stainlib_amd import engine
    C = case_data(case)
    es = torch.empty((), dtype=dtype).element_size()
    bits = plane_bits(case, c, es)
    if dtype == torch.bool:
        bits = bits & 1
    fl = int(torch.tensor([fill], dtype=dtype).view(_INT[es])[0]) & ((1 << (8 * es)) - 1)
    want = planes_want(bits, C.rows, C.size, fl)
    assert (want == fl).any() and (want != fl).any()
    signed = {1: np.uint8, 2: np.int16, 8: np.int64}[es]
    planes = torch.from_numpy(bits.view(signed)).view(dtype)
    planes, want = (planes, want) if c == 2 else (planes[:, 0].contiguous(), want[:, 0])
    shape = ((N, c) if c == 2 else (N,)) + C.size
    dp = planes.cuda()
    for win in (C.rows, torch.tensor(C.rows).cuda()):
        for off in (0, 1):
            buf, start, numel, out = _guarded_planes(shape, dtype, off)
            res = engine.view_planes_affine(dp, win, C.size, AFFINE_MAX_R, fill=fill, out=out)
            assert res is out
            torch.cuda.synchronize()
            got = buf.cpu()
            assert bool((torch.cat([got[:start], got[start + numel:]]) == SENTINEL).all()), f"{case_id(case)} {dtype} out+{off}: outside"
            assert np.array_equal(got[start:start + numel].view(shape).numpy(), want.view(signed)), f"{case_id(case)} c={c} {dtype} out+{off}"

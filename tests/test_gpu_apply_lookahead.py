"""-m gpu: the apply sweep of the fused kernels (apply_kernels.hpp: lookahead_sweep under apply_sweep) keeps two trips of chunks in flight
in two register sets, the loop body is two trips long, and an odd number of trips runs its second half clamped and masked.  The loop can
go wrong at the trip and parity boundaries, so the shapes sit on them: a trip of the 512-thread kernel is 4 x 512 chunks = 8 192 pixels,
one of the 1 024-thread kernel 16 384 (the general lasso takes two chunks per trip: half of that).
Every case forces the fused schedule on three tiles and compares with the one-launch-per-phase schedule on the same tiles: the output
bytes with torch.equal (both share apply_px by construction: no tolerance), and the statistics the bytes are made from.  Each fused
output is also compared with the stand-alone apply pass (k_apply) under the fused kernel's OWN (M, maxC), which takes the fit out of
the comparison altogether."""
import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests.gpu_util import oracle_fit_tile, to_dev

pytestmark = pytest.mark.gpu

_TARGET = []


def _target():
    if not _TARGET:
        _TARGET.append(oracle_fit_tile(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT)))
    return _TARGET[0]


def _tiles(h, w, seed, white_middle=False):
    t = [so.synth_tile(h, w, seed + i) for i in range(3)]
    if white_middle:
        t[1] = np.full((h, w, 3), 255, np.uint8)                  # a failed fit between two good ones: the copy path beside fused_apply
    return t


def _compare(tiles, fused, method="macenko", Mt=None, label="", same_stats=True):
    """fused (SlParams of the fused schedule) against schedule = 1 and against k_apply under the fused kernel's own statistics"""
    from stainlib_amd import engine
    fn = engine.macenko_transform if method == "macenko" else engine.vahadane_transform
    M_tgt, mc_tgt = _target()
    if Mt is not None:
        M_tgt = Mt
    dev = to_dev(tiles)
    res = []
    for kw in (fused, dict(schedule=1)):
        out, M, mc, st = fn(dev, M_tgt, mc_tgt, params=engine.make_params(**kw))
        torch.cuda.synchronize()
        res.append((out, M, mc, st))
    (a, Ma, mca, sta), (b, Mb, mcb, stb) = res
    ok = (sta == 0).cpu().numpy()
    stats_equal = torch.equal(Ma.view(torch.int64), Mb.view(torch.int64)) and torch.equal(mca.view(torch.int64), mcb.view(torch.int64))
    print(f"{label}: status {sta.cpu().numpy().tolist()} statistics bit-equal {stats_equal} "
          f"bytes differing from schedule 1: {int((a != b).sum())} of {a.numel()}")
    assert torch.equal(sta, stb), f"{label}: status"
    if same_stats:
        assert stats_equal, f"{label}: M / maxC of the two schedules differ"
    assert torch.equal(a, b), f"{label}: the fused schedule's bytes differ from the per-phase schedule's"
    # the stand-alone apply pass under the fused kernel's own (M, maxC): tiles with a fit
    idx = np.flatnonzero(ok)
    assert len(idx) >= 2
    sel = torch.from_numpy(idx).cuda()
    want = engine.normalize_apply(dev[sel].contiguous(), Ma[sel], mca[sel], M_tgt, mc_tgt)
    torch.cuda.synchronize()
    assert torch.equal(a[sel], want), f"{label}: the fused apply sweep differs from k_apply under the same statistics"
    for i in np.flatnonzero(~ok):                                  # a failed fit: the input comes back
        assert torch.equal(a[int(i)], dev[int(i)]), f"{label}: tile {i} (no fit) is not its input"
    return a


# pixels: half a trip, one trip, one chunk over, 1.5, two, one chunk over, 2.5, three (an odd count), four trips -- all aligned
ALIGNED_512 = [(64, 64), (64, 128), (2, 4098), (96, 128), (128, 128), (2, 8194), (160, 128), (192, 128), (256, 128)]
RAGGED_512 = [(61, 67), (127, 129), (181, 183)]                    # unaligned bytes, a ragged last chunk: 4 087, 16 383, 33 123 pixels


@pytest.mark.parametrize("h,w", ALIGNED_512 + RAGGED_512)
def test_fused_512_against_per_phase(h, w):
    white = (h, w) in ((96, 128), (127, 129))
    out = _compare(_tiles(h, w, 300 + h + w, white), dict(schedule=2), label=f"fused 512 threads {h}x{w}")
    assert out.shape == (3, h, w, 3)


@pytest.mark.parametrize("h,w", [(128, 128), (2, 8194), (192, 256)])
def test_fused_1024_against_per_phase(h, w):
    """schedule 3: one 1 024-thread workgroup per CU (a batch of no more tiles than CUs); each half of the workgroup sweeps half the tile"""
    _compare(_tiles(h, w, 500 + h + w, (h, w) == (2, 8194)), dict(schedule=3), label=f"fused 1024 threads {h}x{w}")


@pytest.mark.parametrize("h,w", [(128, 128), (127, 129)])
def test_fused_vahadane_against_per_phase(h, w):
    """k_fused<vahadane> calls the same fused_apply.  (The two schedules of the dictionary differ in their binary64 summation order,
    test_gpu_vahadane.py; the bytes are held to equality all the same, and to k_apply under the fused kernel's own dictionary.)"""
    _compare(_tiles(h, w, 700 + h + w), dict(schedule=2), method="vahadane", label=f"fused vahadane {h}x{w}", same_stats=False)


@pytest.mark.parametrize("h,w", [(128, 128), (127, 129), (2, 2050), (96, 128)])
def test_fused_general_lasso_against_per_phase(h, w):
    """A target matrix with a negative entry: ApplyK.fast is false and apply_sweep runs the general lasso and pack, two chunks per trip
    (4 096 pixels): one trip and one chunk over, 1.5 (odd), two and a ragged tile."""
    Mt = np.array(_target()[0], dtype=np.float64).copy()
    Mt[1, 2] = -0.05
    _compare(_tiles(h, w, 900 + h + w), dict(schedule=2), Mt=Mt, label=f"fused general lasso {h}x{w}")


def test_fused_stream_tile_against_per_phase():
    """512 x 512 = 768 KiB >= kStreamBytes: the non-temporal instantiation of the sweep, 32 trips"""
    from stainlib_amd import engine
    M_tgt, mc_tgt = _target()
    dev = to_dev([so.synth_tile(512, 512, 77)])
    a, Ma, mca, sta = engine.macenko_transform(dev, M_tgt, mc_tgt, params=engine.make_params(schedule=2))
    b, Mb, mcb, stb = engine.macenko_transform(dev, M_tgt, mc_tgt, params=engine.make_params(schedule=1))
    torch.cuda.synchronize()
    assert int(sta[0]) == 0 and int(stb[0]) == 0
    assert torch.equal(Ma.view(torch.int64), Mb.view(torch.int64)) and torch.equal(mca.view(torch.int64), mcb.view(torch.int64))
    assert torch.equal(a, b)
    assert torch.equal(a, engine.normalize_apply(dev, Ma, mca, M_tgt, mc_tgt))

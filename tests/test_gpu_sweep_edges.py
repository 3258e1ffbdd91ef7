"""-m gpu: the boundaries of the pipelined sweep loop (csrc/sweep_pipeline.hpp and the copy in moments_sweep_b: clamped
look-ahead loads, the one ragged trip per wave, its in-range test) through four kernels that run it, at the tile sizes where the
loop changes its path.

Every shape is a batch of three tiles -- so that tiles 1 and 2 start at an odd byte offset when 3 P is odd -- taken twice:
as a tensor of its own and as the slice [1:] of a four-tile tensor (the whole batch then starts at byte 3 P).  Tile 1 is
the white-background variant (all white below 255 pixels: the empty-mask status).  Oracles and tolerances are those of the tests
that check the same quantities elsewhere: the tissue count of test_gpu_lab.py, the radix histograms of
test_gpu_api.py::test_slide_window_sweep_agrees_with_the_radix_histograms, u8_parity on the normalised bytes against the oracle's,
and M_ATOL / MAXC_RTOL of test_gpu_macenko.py where those bars are stated: on tiles with at least 200 tissue pixels (the floor of
test_gpu_stress.py; tools/small_tile_errors.py measured them there).  Below it the covariance of a handful of pixels is close to
rank one and amplifies the 1e-7 of the binary32 sums (3 pixels, eigenvalues 0.17 / 0.0016: |dM| = 6.9e-7, the same before the sweeps
shared their loop), so there the statistics are judged by the bytes they produce."""
import functools

import numpy as np
import pytest

from oracle import stain_oracle as so
from tests.gpu_util import oracle_fit_tile, to_dev, u8_parity
from tests.test_gpu_macenko import M_ATOL, MAXC_RTOL

pytestmark = pytest.mark.gpu

TRIP = 4 * 4 * 512           # pixels of one full trip of a 512-thread workgroup: 4 pixels x kPhaseTrip chunks x kSweepThreads lanes
# fewer than one chunk / two chunks (byte-wise load path, a trip that is all tail); one wave row +-1 pixel; one full trip and the
# first chunk of the ragged one; the smallest tile with two parts (32771 pixels = 8193 chunks: part 0 is three full trips, part 1
# one full trip and ONE ragged chunk of three pixels past it)
PIXELS = [1, 3, 5, 4 * 64 - 1, 4 * 64, 4 * 64 + 1, TRIP - 3, TRIP - 1, TRIP, TRIP + 1, TRIP + 2, 32768 + 3]


def _shape(P):
    return {4 * 64: (16, 16), TRIP: (64, 128), TRIP + 2: (2, (TRIP + 2) // 2)}.get(P, (1, P))


def _tissue(I):
    return (so.lab_l8(I) / 255.0) < 0.8                    # LuminosityThresholdTissueLocator at the default threshold


@functools.lru_cache(maxsize=None)
def _case(P):
    """the three tiles of a shape with what the oracle says about each: tissue count, expected status, (M, maxC) where it is 0"""
    h, w = _shape(P)
    white = so.structured_tile("white_bg", h, w, 40 + P % 89) if P >= 255 else np.full((h, w, 3), 255, np.uint8)
    tiles = [so.synth_tile(h, w, 700 + P % 97), white, so.synth_tile(h, w, 800 + P % 97)]
    info = []
    for I in tiles:
        nt = int(_tissue(I).sum())
        # no tissue: SL_TILE_EMPTY_MASK; one tissue pixel: the reference's np.cov is NaN, reported as degenerate (as in
        # test_gpu_macenko.py::test_failed_tiles_do_not_poison_batch)
        status = 1 if nt == 0 else (2 if nt == 1 else 0)
        info.append((nt, status, oracle_fit_tile(I) if status == 0 else None))
    return tiles, info


def _batches(tiles):
    """the batch as a tensor of its own, and as the slice [1:] of a larger one"""
    own = to_dev(tiles)
    big = to_dev([tiles[2]] + list(tiles))
    return [("own tensor", own), ("slice [1:]", big[1:])]


@pytest.mark.parametrize("P", PIXELS)
def test_tile_moments_count_every_tissue_pixel_once(P):
    from stainlib_amd import engine
    tiles, info = _case(P)
    for label, dev in _batches(tiles):
        mom = engine.tile_moments(dev).cpu().numpy()
        assert [int(m) for m in mom[:, 0]] == [nt for nt, _, _ in info], label
        for i, (nt, _, _) in enumerate(info):
            if nt == 0:
                assert not mom[i].any(), label                   # nothing past the tile's end leaks into the sums


@pytest.mark.parametrize("P", PIXELS)
def test_window_sweep_agrees_with_the_radix_histograms(P):
    """As test_gpu_api.py::test_slide_window_sweep_agrees_with_the_radix_histograms: the window on a 16-bit prefix must report
    the radix kernels' 65536 bins and count below; the key totals are the pixel / tissue counts numpy gives."""
    from stainlib_amd import _ffi, engine
    tiles, info = _case(P)
    V = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 2)))[0]
    M_pos = so.M_TRUE_TGT / np.linalg.norm(so.M_TRUE_TGT, axis=1, keepdims=True)
    totals = {_ffi.KEYSET_ANGLE: sum(nt for nt, _, _ in info), _ffi.KEYSET_CONC: 3 * P}
    for label, dev in _batches(tiles):
        for keyset, basis in ((_ffi.KEYSET_ANGLE, V.reshape(6)), (_ffi.KEYSET_CONC, M_pos.reshape(6))):
            h0 = engine.slide_key_histogram(dev, keyset, basis, (0, 0), 0).cpu().numpy()
            assert int(h0[0].sum()) == totals[keyset] and int(h0[1].sum()) == totals[keyset], label
            pre16 = []                                      # the 16-bit prefixes holding the 30 % and the 90 % key of target 0 / target 1
            for t, frac in ((0, 0.3), (1, 0.9)):
                if totals[keyset] == 0:
                    pre16.append((0, 0))
                    continue
                k = int(frac * (totals[keyset] - 1))
                b8 = int(np.searchsorted(np.cumsum(h0[t]), k, side="right"))
                h1 = engine.slide_key_histogram(dev, keyset, basis, (b8, b8), 8).cpu().numpy()
                below8 = int(h0[t][:b8].sum())
                b16 = int(np.searchsorted(np.cumsum(h1[t]), k - below8, side="right"))
                pre16.append(((b8 << 8) | b16, below8 + int(h1[t][:b16].sum())))
            want = engine.slide_key_histogram16(dev, keyset, basis, (pre16[0][0], pre16[1][0])).cpu().numpy().reshape(2, 65536)
            got = engine.slide_key_window(dev, keyset, basis, (pre16[0][0] << 16, pre16[1][0] << 16)).cpu().numpy()
            assert np.array_equal(got[:65536], want[0]) and np.array_equal(got[65536:131072], want[1]), label
            assert int(got[131072]) == pre16[0][1] and int(got[131073]) == pre16[1][1], label
            assert (int(want[0].sum()) > 0 and int(want[1].sum()) > 0) or totals[keyset] == 0


M_FLOOR = 200            # tissue pixels from which M_ATOL / MAXC_RTOL are stated (test_gpu_stress.py)


def _check_fit(M, mc, st, info, label):
    assert list(st) == [s for _, s, _ in info], label
    for i, (nt, status, fit) in enumerate(info):
        if status:
            assert np.isnan(M[i]).all(), label
            continue
        np.testing.assert_allclose(np.linalg.norm(M[i], axis=1), 1.0, rtol=0, atol=1e-12, err_msg=label)
        assert M[i][0, 0] > M[i][1, 0], label                           # H row first
        if nt >= M_FLOOR:
            np.testing.assert_allclose(M[i], fit[0], rtol=0, atol=M_ATOL, err_msg=label)
            np.testing.assert_allclose(mc[i], fit[1], rtol=MAXC_RTOL, err_msg=label)


def _check_bytes(out, tiles, info, want, label):
    for i, (_, status, _) in enumerate(info):
        if status:
            assert np.array_equal(out[i], tiles[i]), label              # passed through
        else:
            u8_parity(out[i], want[i], label=f"{label}, tile {i}")


@functools.lru_cache(maxsize=None)
def _target():
    Mt, mct = oracle_fit_tile(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT))
    n = so.ExtractiveStainNormalizer("macenko")
    n.stain_matrix_target, n.maxC_target = Mt, mct.reshape(1, 2)
    return Mt, mct, n


@functools.lru_cache(maxsize=None)
def _want(P):
    """the oracle's normalised bytes of the shape's tiles (a tile the fit refuses passes through)"""
    tiles, info = _case(P)
    n = _target()[2]
    return [n.transform(I) if status == 0 else I for I, (_, status, _) in zip(tiles, info)]


@pytest.mark.parametrize("P", PIXELS)
def test_fit_one_launch_per_phase(P):
    """sl_macenko_fit on the per-phase schedule (k_moments, k_select), its statistics applied by sl_normalize_apply"""
    from stainlib_amd import engine
    tiles, info = _case(P)
    Mt, mct, _ = _target()
    for label, dev in _batches(tiles):
        M, mc, st = engine.macenko_fit(dev, params=engine.make_params(schedule=1))
        _check_fit(M.cpu().numpy(), mc.cpu().numpy(), st.cpu().numpy(), info, label)
        out = engine.normalize_apply(dev, M, mc, Mt, mct)
        _check_bytes(out.cpu().numpy(), tiles, info, _want(P), f"{P} pixels, per-phase fit, {label}")


@pytest.mark.parametrize("P", PIXELS)
def test_transform_fused(P):
    from stainlib_amd import engine
    tiles, info = _case(P)
    Mt, mct, _ = _target()
    for label, dev in _batches(tiles):
        out, M, mc, st = engine.macenko_transform(dev, Mt, mct, params=engine.make_params(schedule=2))
        _check_fit(M.cpu().numpy(), mc.cpu().numpy(), st.cpu().numpy(), info, label)
        _check_bytes(out.cpu().numpy(), tiles, info, _want(P), f"{P} pixels, fused transform, {label}")

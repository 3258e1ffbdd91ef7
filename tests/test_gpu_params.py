"""-m gpu: the three numbers a user can set -- angular_percentile, luminosity_threshold, lasso_lambda -- over their whole accepted range,
through every route that reads them, against the float64 oracle at the same setting.

The selection machinery is built around "two thin tails at 1 % / 99 %"; here the percentile goes down to the middle of the distribution
(overlapping sample brackets), to its ends (a rank at the very end of a list, zero-sigma brackets) and below 50 (the library folds p
onto max(p, 100 - p): the reference takes the pair (100 - p, p) and orders the stain vectors afterwards, asserted on the oracle below);
the threshold passes 1 (saturated white becomes tissue: a third of a tile is one run of tied angle keys) and goes to 0 and NaN (no
tissue anywhere); the lasso penalty goes to 0 and up to where it zeroes every concentration.

Bars are the suite's own, imported: M_ATOL / MAXC_RTOL on tiles with at least M_FLOOR tissue pixels (test_gpu_sweep_edges.py; the count
is the oracle's), u8_parity on bytes, 5e-6 and the KKT certificate on concentrations, 2e-5 relative on pre-quantisation values
(test_gpu_apply.py), 5e-7 / 1e-6 on the pooled chains (test_gpu_pool2.py), and across routes identical bytes and status with M and maxC
within 1e-12."""
import functools

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests.gpu_util import oracle_fit_tile, to_dev, u8_parity
from tests.test_gpu_macenko import M_ATOL, MAXC_RTOL
from tests.test_gpu_sweep_edges import M_FLOOR

pytestmark = pytest.mark.gpu

# (256, 320): the smallest tile whose sample has a closed box (the merged sweep's box path, the cube pre-filter and the SL_RESWEEP_*
# reasons are reachable); (33, 47): the byte-wise load path, 1551 pixels; (96, 130): in between, the pooled slide's tile
SIZES = [(96, 130), (33, 47), (256, 320)]
PCTS = [100, 99.9, 90, 75, 55, 52, 50, 25, 1, 0]
THRS = [0.0, 0.2, 0.5, 0.95, 1.0, 1.01, 2.0, float("nan")]
LAMS = [0.0, 0.1, 1.0, 3.0]
RESWEEPS = {0, 1, 2, 3, 4}        # "no resweep" and SL_RESWEEP_NO_BOX ... SL_RESWEEP_LIST_FULL (include/stainlib_hip.h)
UNTOUCHED = 77
WHITE = 5                         # index of the all-white tile of a batch
DIRECT = 1                        # SL_TWOSWEEP_DIRECT
# Cases whose conditioning puts them above M_ATOL / MAXC_RTOL with every route in agreement and the bytes in parity: (h, w, threshold,
# tile) -> (M atol, maxC rtol), 2-4 x the measured error, never above the 1e-5 the suite accepts for an ill-conditioned tile
# (test_first_eigenvector_with_a_negative_component_...).  Measurements and the oracle-only argument: profiles/params_grid_errors.txt.
#   (256, 320) blobs at threshold 0.2: 253 tissue pixels of one smooth blob, eigenvalues 0.208 / 3.2e-4 / 3.5e-5 -- the covariance is
#   close to rank one and the second eigenvector is decided by a gap of 2.8e-4: a relative 1e-7 in the covariance (the binary32 burst
#   sums) moves the oracle's own M by up to 1.6e-6, binary32 keys alone by 3e-8.  Measured: |dM| 7.34e-7, |dmaxC| 5.21e-7.
BARS = {(256, 320, 0.2, 4): (2e-6, 2e-6)}


@functools.lru_cache(maxsize=None)
def _tiles(h, w):
    """six tiles: two i.i.d. stain mixtures, white background, JPEG-like quantisation, smooth blobs, and one all-white tile -- a tile that
    fails (no tissue below a threshold of 1) and must not poison its neighbours"""
    return (so.synth_tile(h, w, 3), so.synth_tile(h, w, 4), so.structured_tile("white_bg", h, w, 5), so.structured_tile("quantized", h, w, 6),
            so.structured_tile("blobs", h, w, 7), np.full((h, w, 3), 255, np.uint8))


@functools.lru_cache(maxsize=None)
def _target():
    return oracle_fit_tile(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT))


def _nt(I, thr):
    """tissue pixels as the reference counts them: L8 / 255.0 < thr (NaN and 0: none)"""
    return int(((so.lab_l8(I) / 255.0) < thr).sum())


@functools.lru_cache(maxsize=None)
def _oracle(h, w, i, thr, pct, lam):
    """What the oracle says about tile i of the (h, w) batch at one setting -> dict(nt, status, M, mc, out, pre).  status: 1 no tissue,
    2 parallel stain vectors (pct = 50) or a single tissue pixel, 3 a zero concentration percentile, else 0.  NaN thresholds are keyed
    as the string "nan" by the callers (NaN != NaN would defeat the cache)."""
    thr = float("nan") if thr == "nan" else thr
    I = _tiles(h, w)[i]
    nt = _nt(I, thr)
    if nt == 0:
        return dict(nt=0, status=1)
    if nt == 1:
        return dict(nt=1, status=2)
    M = so.macenko_stain_matrix(I, thr, pct)
    if abs(M[0] @ M[1]) > 1 - 1e-12:
        return dict(nt=nt, status=2, M=M)
    C = so.get_concentrations(I, M, lam)
    mc = np.percentile(C, 99, axis=0)
    if not (mc > 0).all():
        return dict(nt=nt, status=3, M=M, mc=mc)
    Mt, mct = _target()
    pre = (255 * np.exp(-(C * (mct / mc)) @ Mt)).reshape(I.shape)
    return dict(nt=nt, status=0, M=M, mc=mc, pre=pre, out=so.truncate_u8(pre), cos=float(M[0] @ M[1]))


def _key(thr):
    return "nan" if thr != thr else thr


def _run(dev, transform, thr=0.8, pct=99.0, lam=0.01, **kw):
    """one fit or transform call with the diagnostics attached -> dict of numpy arrays"""
    from stainlib_amd import engine
    n = dev.shape[0]
    p = engine.make_params(luminosity_threshold=float(thr), angular_percentile=float(pct), lasso_lambda=float(lam), **kw)
    fb = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    rs = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    ts = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    p.fallbacks_out, p.resweeps_out, p.twosweep_out = fb.data_ptr(), rs.data_ptr(), ts.data_ptr()
    Mt, mct = _target()
    if transform:
        out, M, mc, st = engine.macenko_transform(dev, Mt, mct, params=p)
    else:
        out = None
        M, mc, st = engine.macenko_fit(dev, params=p)
    torch.cuda.synchronize()
    return dict(out=None if out is None else out.cpu().numpy(), M=M.cpu().numpy(), mc=mc.cpu().numpy(), st=st.cpu().numpy(),
                fb=fb.cpu().numpy(), rs=rs.cpu().numpy(), ts=ts.cpu().numpy(), fused=kw.get("schedule") != 1)


def _diagnostics(r, label):
    assert ((r["fb"] >= 0) & (r["fb"] <= 4)).all(), f"{label}: fallbacks {r['fb']}"
    if r["fused"]:
        assert set(r["rs"].tolist()) <= RESWEEPS, f"{label}: resweeps {r['rs']}"
    else:
        assert (r["rs"] == UNTOUCHED).all(), f"{label}: the per-phase schedule wrote resweeps_out"


def _same(a, b, label):
    """across routes: identical bytes and status, M within 1e-12, maxC within 1e-12 relative"""
    assert list(a["st"]) == list(b["st"]), f"{label}: status {a['st']} vs {b['st']}"
    if a["out"] is not None and b["out"] is not None:
        assert np.array_equal(a["out"], b["out"]), f"{label}: bytes"
    np.testing.assert_allclose(a["M"], b["M"], rtol=0, atol=1e-12, equal_nan=True, err_msg=label)
    np.testing.assert_allclose(a["mc"], b["mc"], rtol=1e-12, atol=0, equal_nan=True, err_msg=label)


def _against_oracle(r, h, w, thr, pct, lam, label, stats_only_M=False):
    """one route's results against the oracle, tile by tile.  stats_only_M: M at the bar, maxC and bytes not compared (pct 52 / 55)."""
    tiles = _tiles(h, w)
    for i, I in enumerate(tiles):
        o = _oracle(h, w, i, _key(thr), pct, lam)
        lab = f"{label}, tile {i} ({o['nt']} tissue pixels)"
        assert int(r["st"][i]) == o["status"], f"{lab}: status {r['st'][i]}, the oracle says {o['status']}"
        if o["status"] in (1, 2):
            assert np.isnan(r["M"][i]).all() and np.isnan(r["mc"][i]).all(), lab
        if o["status"]:
            if r["out"] is not None:
                assert np.array_equal(r["out"][i], I), f"{lab}: a refused tile must pass through byte for byte"
            continue
        np.testing.assert_allclose(np.linalg.norm(r["M"][i], axis=1), 1.0, rtol=0, atol=1e-12, err_msg=lab)
        assert r["M"][i][0, 0] > r["M"][i][1, 0], lab                        # H row first
        dM = float(np.abs(r["M"][i] - o["M"]).max())
        dmc = float(np.abs(r["mc"][i] / o["mc"] - 1).max())
        print(f"{lab}: |dM| {dM:.2e} |dmaxC| {dmc:.2e} cos {o['cos']:.6f} fallbacks {r['fb'][i]} resweep {r['rs'][i]}")
        m_atol, mc_rtol = BARS.get((h, w, thr, i), (M_ATOL, MAXC_RTOL))
        if o["nt"] >= M_FLOOR:
            np.testing.assert_allclose(r["M"][i], o["M"], rtol=0, atol=m_atol, err_msg=lab)
            if not stats_only_M:
                np.testing.assert_allclose(r["mc"][i], o["mc"], rtol=mc_rtol, err_msg=lab)
        if r["out"] is not None and not stats_only_M:
            u8_parity(r["out"][i], o["out"], label=lab, src=I, prequant=o["pre"])


# what reads the percentile: both entry points on the three schedules; the fused kernel also without / always behind the colour-cube
# mask, without the two-sweep route and with it forced (test_gpu_twosweep.py: two_sweep = 2)
ROUTES = [("fit per phase", False, dict(schedule=1)), ("fit fused", False, dict(schedule=2)), ("fit wide", False, dict(schedule=3)),
          ("transform per phase", True, dict(schedule=1)), ("transform fused", True, dict(schedule=2)), ("transform wide", True, dict(schedule=3)),
          ("transform fused, no cube", True, dict(schedule=2, prefilter=1)), ("transform fused, cube forced", True, dict(schedule=2, prefilter=2)),
          ("transform fused, three sweeps", True, dict(schedule=2, two_sweep=1)), ("transform fused, two sweeps forced", True, dict(schedule=2, two_sweep=2))]


# ---- (a) angular percentile ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", PCTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_angular_percentile_over_its_whole_range_on_every_route(h, w, pct):
    """pct in {100, 99.9, 90, 75, 25, 1, 0}: status 0, M and maxC at the bars, bytes in parity, all routes identical.
    pct = 50: the oracle's two rows are parallel (asserted), its concentrations divide by a singular Gram matrix: SL_TILE_DEGENERATE_COV
    on every route, NaN statistics, the tile passed through (the convention of test_degenerate_colour_sets_are_reported_the_same_by_
    both_schedules), the all-white neighbour still SL_TILE_EMPTY_MASK.
    pct in {52, 55}: order statistics in the dense middle of the angle distribution -- M is held to M_ATOL -- but the two rows are nearly
    parallel (the oracle's cosine on synth_tile(96, 130, 3): 0.99976 at 52, 0.99850 at 55; printed per tile) and 1 / (1 - cos^2) =
    300 ... 2000 multiplies any error of M in the lasso: maxC and bytes are NOT compared with the oracle there, only across routes,
    for identity."""
    tiles = _tiles(h, w)
    dev = to_dev(list(tiles))
    for i, I in enumerate(tiles[:WHITE]):
        assert _nt(I, 0.8) >= 2
        # the reference is symmetric about 50: what justifies running the kernels with max(pct, 100 - pct)
        assert np.array_equal(so.macenko_stain_matrix(I, 0.8, pct), so.macenko_stain_matrix(I, 0.8, 100 - pct))
        if pct == 50:
            M = so.macenko_stain_matrix(I, 0.8, 50)
            assert abs(M[0] @ M[1]) > 1 - 1e-12
    first = None
    for name, transform, kw in ROUTES:
        label = f"{h}x{w} pct {pct} {name}"
        r = _run(dev, transform, pct=pct, **kw)
        _diagnostics(r, label)
        print(f"{label}: status {r['st'].tolist()} fallbacks {r['fb'].tolist()} resweeps {r['rs'].tolist()} two-sweep attempts {r['ts'].tolist()}")
        if pct == 50:
            assert list(r["st"]) == [2] * WHITE + [1], f"{label}: status {r['st']}"
        if kw.get("two_sweep") == 2 and pct in (100, 0) and h * w >= (1 << 14):
            # at 100 % the upper rank is the LAST tissue pixel and has no successor: the finish's coverage test clamps k + 1 like every
            # other site; unclamped, no bracket could ever cover it and every tile would leave the route as SL_TWOSWEEP_BRACKET
            assert (r["ts"][:4] == DIRECT).all(), f"{label}: two-sweep attempts {r['ts']}"
        _against_oracle(r, h, w, 0.8, pct, 0.01, label, stats_only_M=pct in (52, 55))
        if first is None:
            first = r
        else:
            _same(first, r, f"{label} against {ROUTES[0][0]}")
        if transform and first["out"] is None:
            first = dict(first, out=r["out"])


def test_a_bad_percentile_is_a_value_error_like_numpys():
    """np.percentile raises ValueError("Percentiles must be in the range [0, 100]") for 101, -1 and NaN; the Python classes raise the
    same themselves (no StainlibHipError surfaces), the engine refuses the SlParams."""
    import stainlib_amd as sl
    from stainlib_amd import _ffi, engine
    from stainlib_amd.distributed import PooledSlideStatistics
    I = _tiles(33, 47)[0]
    dev = to_dev([I])
    for bad in (101, -1, float("nan")):
        with pytest.raises(ValueError, match=r"Percentiles must be in the range \[0, 100\]"):
            np.percentile(np.arange(4.0), bad)
        with pytest.raises(ValueError, match=r"Percentiles must be in the range \[0, 100\]"):
            sl.MacenkoStainExtractor.get_stain_matrix(I, 0.8, bad)
        with pytest.raises(ValueError, match=r"Percentiles must be in the range \[0, 100\]"):
            PooledSlideStatistics(group=False, angular_percentile=bad)
        with pytest.raises(_ffi.StainlibHipError):
            engine.macenko_fit(dev, params=engine.make_params(angular_percentile=float(bad)))
    for bad in (-0.01, float("nan")):
        with pytest.raises(_ffi.StainlibHipError):
            engine.macenko_fit(dev, params=engine.make_params(lasso_lambda=bad))
        with pytest.raises(_ffi.StainlibHipError):
            engine.concentrations(dev, so.normalize_rows(so.M_TRUE_SRC)[None], bad)
    np.testing.assert_allclose(sl.MacenkoStainExtractor.get_stain_matrix(I, 0.8, 25), so.macenko_stain_matrix(I, 0.8, 25), rtol=0, atol=M_ATOL)


# ---- (b) luminosity threshold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", THRS, ids=[f"thr{t}" for t in THRS])
@pytest.mark.parametrize("h,w", SIZES)
def test_luminosity_threshold_over_its_whole_range(h, w, thr):
    """0.0 and NaN: the reference's L < thr is all false -- status 1 on every tile, passed through.  0.2: a few hundred tissue pixels on
    the (256, 320) tiles, fewer on the small ones (judged by their bytes only below M_FLOOR, as test_gpu_sweep_edges.py does).  Above 1
    every pixel is tissue, saturated white included (OD 1e-6 in every channel: on the white-background tile a third of the keys tie)."""
    from stainlib_amd import engine
    tiles = _tiles(h, w)
    dev = to_dev(list(tiles))
    want_nt = [_nt(I, thr) for I in tiles]
    mom = engine.tile_moments(dev, params=engine.make_params(luminosity_threshold=thr)).cpu().numpy()
    assert [int(m) for m in mom[:, 0]] == want_nt
    if thr != thr or thr <= 0:
        assert want_nt == [0] * len(tiles)
    if thr > 1:
        assert want_nt == [h * w] * len(tiles)
    res = []
    for name, kw in (("per phase", dict(schedule=1)), ("fused", dict(schedule=2))):
        label = f"{h}x{w} thr {thr} transform {name}"
        r = _run(dev, True, thr=thr, **kw)
        _diagnostics(r, label)
        _against_oracle(r, h, w, thr, 99.0, 0.01, label)
        res.append(r)
    _same(res[0], res[1], f"{h}x{w} thr {thr}: fused against per phase")


@pytest.mark.parametrize("h,w", SIZES)
def test_only_saturated_white_separates_threshold_1_from_1_01_and_2_equals_1_01(h, w):
    from stainlib_amd import engine
    tiles = _tiles(h, w)
    dev = to_dev(list(tiles))
    count = lambda thr: engine.tile_moments(dev, params=engine.make_params(luminosity_threshold=thr)).cpu().numpy()[:, 0].astype(np.int64)   # noqa: E731
    n255 = np.array([int((so.lab_l8(I) == 255).sum()) for I in tiles])
    assert n255[2] > 0 and n255[WHITE] == h * w
    assert np.array_equal(count(1.01) - count(1.0), n255)
    for kw in (dict(schedule=1), dict(schedule=2)):
        a, b = _run(dev, True, thr=1.01, **kw), _run(dev, True, thr=2.0, **kw)
        for k in ("out", "M", "mc", "st"):
            assert np.array_equal(a[k], b[k], equal_nan=k in ("M", "mc")), (kw, k)


def test_python_classes_raise_on_a_threshold_without_tissue():
    import stainlib_amd as sl
    from stainlib_amd.utils.stain_utils import LuminosityThresholdTissueLocator
    I = _tiles(33, 47)[0]
    for thr in (0.0, float("nan")):
        with pytest.raises(so.TissueMaskException):
            so.macenko_stain_matrix(I, thr)
        with pytest.raises(sl.TissueMaskException, match="Empty tissue mask computed"):
            sl.MacenkoStainExtractor.get_stain_matrix(I, thr)
        with pytest.raises(sl.TissueMaskException, match="Empty tissue mask computed"):
            LuminosityThresholdTissueLocator.get_tissue_mask(I, thr)


def test_tissue_mask_at_every_threshold():
    """One 256 x 256 tile of a grey ramp (every L8 boundary), the 8 cube corners and random colours: the oracle's mask and count exactly.
    (All 2^24 colours at three ordinary thresholds: test_gpu_lab.py.)"""
    from stainlib_amd import engine
    rng = np.random.RandomState(12)
    I = rng.randint(0, 256, size=(256, 256, 3)).astype(np.uint8)
    I[:2] = np.repeat(np.arange(256, dtype=np.uint8), 2).reshape(2, 256, 1)
    I[2, :8] = [[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    dev = to_dev([I])
    L = so.lab_l8(I) / 255.0
    for thr in THRS:
        want = L < thr
        mask, counts = engine.tissue_mask(dev, thr)
        assert int(counts[0]) == int(want.sum()), thr
        assert np.array_equal(mask[0].cpu().numpy().astype(bool), want), thr
        mom = engine.tile_moments(dev, params=engine.make_params(luminosity_threshold=thr)).cpu().numpy()
        assert int(mom[0, 0]) == int(want.sum()), thr                        # the sweeps' binary32 twin of the test


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.01])
def test_reinhard_mask_background_at_the_ends_of_the_threshold(thr):
    """ReinhardStainNormalizer.transform(mask_background=True) against the oracle's, byte for byte as that family is; at 0.0 the oracle's
    get_tissue_mask raises on the empty mask, and so does the class."""
    import stainlib_amd as sl
    I = so.structured_tile("white_bg", 61, 67, 5)
    tgt = so.synth_tile(80, 80, 1001, so.M_TRUE_TGT)
    n, on = sl.ReinhardStainNormalizer(), so.ReinhardStainNormalizer()
    n.fit(tgt)
    on.fit(tgt)
    if thr <= 0:
        with pytest.raises(so.TissueMaskException):
            on.transform(I, mask_background=True, luminosity_threshold=thr)
        with pytest.raises(sl.TissueMaskException, match="Empty tissue mask computed"):
            n.transform(I, mask_background=True, luminosity_threshold=thr)
        out, st = n.transform_batch(to_dev([I]), mask_background=True, luminosity_threshold=thr)
        assert int(st[0, 7]) == 0
        return
    want = on.transform(I, mask_background=True, luminosity_threshold=thr)
    assert np.array_equal(n.transform(I, mask_background=True, luminosity_threshold=thr), want)
    out, st = n.transform_batch(to_dev([I, I]), mask_background=True, luminosity_threshold=thr)
    assert np.array_equal(out[1].cpu().numpy(), want)
    assert int(st[1, 7]) == int(so.tissue_mask(so.standardize_brightness(I), thr).sum())


# ---- (c) lasso lambda ---------------------------------------------------------------------------------------------------------------------
M_HE = so.normalize_rows(so.M_TRUE_SRC)
M_NEG = so.normalize_rows(np.array([[0.9, -0.3, 0.3], [-0.2, 0.95, 0.25]]))            # g12 < 0 (test_gpu_apply.py)


def _active_sets(C):
    return [int(((C[:, 0] > 0) & (C[:, 1] > 0)).sum()), int(((C[:, 0] > 0) & (C[:, 1] == 0)).sum()), int(((C[:, 0] == 0) & (C[:, 1] > 0)).sum())]


@pytest.mark.parametrize("lam", LAMS)
def test_concentrations_at_every_lambda(lam):
    """sl_concentrations under the H&E pair and under M_NEG (g12 < 0: lasso2's active-set enumeration) at 5e-6 with the KKT certificate
    at that lambda.  Which active sets occur is asserted on the oracle.  Under M_NEG, lambda = 0 admits ONE set only: the unconstrained
    solution is a_1 ~ OD . (g22 M_0 - g12 M_1), a_2 ~ OD . (g11 M_1 - g12 M_0), both vectors are positive for this pair (asserted), and
    an optical density is >= 1e-6 in every channel -- so both concentrations are positive for every colour there is.  The sets with
    one stain switched off need the penalty: all three occur at 0.1 and 1.0 once the input holds colours off the H&E plane (the third
    tile: random colours, for this purpose only); at 3.0 everything is zero under either pair except where a colour is nearly black."""
    from stainlib_amd import engine
    assert M_NEG[0] @ M_NEG[1] < 0 < M_HE[0] @ M_HE[1]
    g11, g22, g12 = M_NEG[0] @ M_NEG[0], M_NEG[1] @ M_NEG[1], M_NEG[0] @ M_NEG[1]
    assert (g22 * M_NEG[0] - g12 * M_NEG[1] > 0).all() and (g11 * M_NEG[1] - g12 * M_NEG[0] > 0).all()
    tiles = [so.synth_tile(96, 130, 3), so.synth_tile(33, 47, 4), np.random.RandomState(12).randint(0, 256, size=(96, 130, 3)).astype(np.uint8)]
    for t, I in enumerate(tiles):
        OD = so.rgb_to_od(I).reshape(-1, 3)
        for name, M in (("H&E", M_HE), ("g12 < 0", M_NEG)):
            Cg = engine.concentrations(to_dev([I]), M[None], lam).cpu().numpy()[0].astype(np.float64)
            Co = so.get_concentrations(I, M, lam)
            kkt = so.lasso_kkt_violation(OD, M, Cg, lam)
            sets = _active_sets(Co)
            print(f"lam {lam} {name} tile {t}: max |dC| {np.abs(Cg - Co).max():.2e} KKT {kkt:.2e} active sets (both, first, second) {sets}")
            np.testing.assert_allclose(Cg, Co, rtol=0, atol=5e-6)
            assert kkt < 5e-6
            if M is M_NEG and lam == 0.0:
                assert sets[0] == len(Co) and sets[1:] == [0, 0]
            if M is M_NEG and lam in (0.1, 1.0) and t == 2:
                assert min(sets) > 0, sets


@pytest.mark.parametrize("lam", LAMS)
def test_normalize_apply_at_every_lambda(lam):
    """sl_normalize_apply under the oracle's own statistics at that lambda: pre-quantisation values at 2e-5, bytes by u8_parity.  At 3.0
    a concentration percentile is 0 in the oracle (asserted; both on all tiles but one): such statistics pass the tile through."""
    from stainlib_amd import engine
    Mt, mct = _target()
    for h, w in ((96, 130), (33, 47)):
        tiles = _tiles(h, w)[:2]
        os_ = [_oracle(h, w, i, 0.8, 99.0, lam) for i in range(2)]
        dev = to_dev(list(tiles))
        if lam == 3.0:
            assert all(o["status"] == 3 and not (o["mc"] > 0).all() for o in os_)
            out = engine.normalize_apply(dev, np.stack([o["M"] for o in os_]), np.stack([o["mc"] for o in os_]), Mt, mct, lasso_lambda=lam)
            assert torch.equal(out, dev)
            continue
        assert all(o["status"] == 0 for o in os_)
        out, pre = engine.normalize_apply(dev, np.stack([o["M"] for o in os_]), np.stack([o["mc"] for o in os_]), Mt, mct, lasso_lambda=lam,
                                          want_prequant=True)
        out, pre = out.cpu().numpy(), pre.cpu().numpy()
        for i, o in enumerate(os_):
            rel = np.abs(pre[i] - o["pre"]) / np.maximum(np.abs(o["pre"]), 1e-30)
            print(f"lam {lam} {h}x{w} tile {i}: prequant rel {rel.max():.2e}")
            assert rel.max() < 2e-5
            u8_parity(out[i], o["out"], label=f"normalize_apply lam {lam} {h}x{w} tile {i}")


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("h,w", SIZES)
def test_transform_at_every_lambda(h, w, lam):
    """sl_macenko_transform with make_params(lasso_lambda=lam) on both schedules: maxC is the oracle's percentile AT that lambda.  3.0
    exceeds every pixel's projection: both percentiles are 0, SL_TILE_ZERO_MAXC, passed through."""
    dev = to_dev(list(_tiles(h, w)))
    res = []
    for name, kw in (("per phase", dict(schedule=1)), ("fused", dict(schedule=2))):
        label = f"{h}x{w} lam {lam} transform {name}"
        r = _run(dev, True, lam=lam, **kw)
        _diagnostics(r, label)
        _against_oracle(r, h, w, 0.8, 99.0, lam, label)
        if lam == 3.0:
            assert list(r["st"]) == [3] * WHITE + [1], label
        res.append(r)
    _same(res[0], res[1], f"{h}x{w} lam {lam}: fused against per phase")


def test_every_apply_route_reads_the_same_lambda():
    """stain_separate's norm, normalize_jitter with the identity jitter, normalize_view of the full tile and normalize_apply_tensor at
    lambda = 0.1: each equals normalize_apply at that lambda the way its own suite states it -- the bytes, or convert of them -- and
    differs from the default lambda's image (the argument is read)."""
    import stainlib_amd
    from stainlib_amd import engine
    lam = 0.1
    h, w = 96, 130
    tiles = _tiles(h, w)[:3]
    n = len(tiles)
    dev = to_dev(list(tiles))
    os_ = [_oracle(h, w, i, 0.8, 99.0, lam) for i in range(n)]
    M, mc = np.stack([o["M"] for o in os_]), np.stack([o["mc"] for o in os_])
    Mt, mct = _target()
    want = engine.normalize_apply(dev, M, mc, Mt, mct, lasso_lambda=lam)
    assert not torch.equal(want, engine.normalize_apply(dev, M, mc, Mt, mct))
    p = engine.make_params(lasso_lambda=lam)
    assert torch.equal(engine.stain_separate(dev, M, mc, Mt, mct, lasso_lambda=lam, want=("norm",)).norm, want)
    ident = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (n, 1))
    assert torch.equal(engine.normalize_jitter(dev, M, mc, Mt, mct, ident, params=p), want)
    win = np.zeros((n, 3), dtype=np.int32)
    assert torch.equal(engine.normalize_view(dev, win, None, 6, M_src=M, maxC_src=mc, M_tgt=Mt, maxC_tgt=mct, params=p), want)
    fmt = stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=(0.5, 0.4, 0.6), std=(0.2, 0.25, 0.3))
    got = engine.normalize_apply_tensor(dev, M, mc, Mt, mct, fmt, lasso_lambda=lam)
    assert torch.equal(got.view(torch.int16), fmt.convert(want).view(torch.int16))


# ---- (d) pooled chains --------------------------------------------------------------------------------------------------------------------
POOLED = [(0.8, 100, 0.01), (0.8, 75, 0.01), (0.8, 25, 0.01), (1.01, 99, 0.01), (0.8, 99, 0.1)]


@functools.lru_cache(maxsize=None)
def _slide_oracle(thr, pct, lam):
    tall = np.concatenate(_tiles(96, 130), axis=0)
    M = so.macenko_stain_matrix(tall, thr, pct)
    return M, np.percentile(so.get_concentrations(tall, M, lam), 99, axis=0)


@pytest.mark.parametrize("thr,pct,lam", POOLED)
def test_pooled_chains_at_the_ends_of_the_parameters(thr, pct, lam):
    """PooledSlideStatistics on a six-tile slide against the oracle on the concatenation, bars of test_gpu_pool2.py.  The one-sweep
    route may report a miss (its sample estimate needs a cone between the brackets); what a caller gets is the three-sweep result to
    1e-13 either way."""
    from stainlib_amd.distributed import PooledSlideStatistics
    dev = to_dev(list(_tiles(96, 130)))
    M_ref, mc_ref = _slide_oracle(thr, pct, lam)
    st = PooledSlideStatistics(group=False, luminosity_threshold=thr, angular_percentile=pct, lasso_lambda=lam)
    old = st(dev, merged=False)
    path_old = list(st.last_path)
    new = st.finish(st.enqueue_merged(dev))
    print(f"thr {thr} pct {pct} lam {lam}: three-sweep path {path_old}; one sweep {'settled' if new is not None else 'missed'} "
          f"(miss {st.last_miss}, why {st.last_why}); |dM| {np.abs(old[0] - M_ref).max():.2e} |dmaxC| {np.abs(old[1] / mc_ref - 1).max():.2e}")
    got = st(dev)
    for r in (got,) + ((new,) if new is not None else ()):
        np.testing.assert_allclose(r[0], old[0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(r[1], old[1], rtol=1e-13)
    np.testing.assert_allclose(old[0], M_ref, rtol=0, atol=5e-7)
    np.testing.assert_allclose(old[1], mc_ref, rtol=1e-6)
    if pct < 50:
        mirror = PooledSlideStatistics(group=False, luminosity_threshold=thr, angular_percentile=100 - pct, lasso_lambda=lam)(dev, merged=False)
        assert np.array_equal(mirror[0], old[0]) and np.array_equal(mirror[1], old[1])
        host = st(dev, device_driven=False)
        np.testing.assert_allclose(host[0], old[0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(host[1], old[1], rtol=1e-13)


def test_pooled_chains_report_percentile_50_like_the_per_tile_path():
    """pct = 50: one stain vector twice.  The per-tile path reports SL_TILE_DEGENERATE_COV, which MacenkoStainExtractor raises as
    LinAlgError; so does the pooled path on every route, and an apply pass behind the chain's state writes nothing but the input."""
    import stainlib_amd as sl
    from stainlib_amd import _ffi, engine
    from stainlib_amd.distributed import PooledSlideStatistics
    tiles = _tiles(96, 130)
    dev = to_dev(list(tiles))
    M = so.macenko_stain_matrix(np.concatenate(tiles, axis=0), 0.8, 50)
    assert abs(M[0] @ M[1]) > 1 - 1e-12
    with pytest.raises(np.linalg.LinAlgError):
        sl.MacenkoStainExtractor.get_stain_matrix(tiles[0], 0.8, 50)
    st = PooledSlideStatistics(group=False, angular_percentile=50)
    Mt, mct = _target()
    n = dev.shape[0]
    for enqueue in (st.enqueue, st.enqueue_merged):
        state = enqueue(dev)
        s = state.cpu().numpy()
        status, miss = int(s[_ffi.POOL_STATUS]), int(s[_ffi.POOL_MISS])
        assert status == _ffi.TILE_DEGENERATE_COV or (enqueue == st.enqueue_merged and miss != 0), (status, miss)
        assert np.isnan(s[_ffi.POOL_M:_ffi.POOL_M + 6]).all() and np.isnan(s[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2]).all()
        M_s = state[_ffi.POOL_M:_ffi.POOL_M + 6].reshape(2, 3).expand(n, 2, 3).contiguous()
        mc_s = state[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2].expand(n, 2).contiguous()
        assert torch.equal(engine.normalize_apply(dev, M_s, mc_s, Mt, mct), dev)
        if status == _ffi.TILE_DEGENERATE_COV:
            with pytest.raises(np.linalg.LinAlgError):
                st.finish(state)
    for kw in (dict(merged=False), dict()):
        with pytest.raises(np.linalg.LinAlgError):
            st(dev, **kw)

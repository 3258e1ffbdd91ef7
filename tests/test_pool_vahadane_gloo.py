"""CPU, world_size = 2, gloo: the pooled slide-level Vahadane statistics (stainlib_amd/distributed.py PooledVahadaneStatistics).

The orchestration under test is the product's: the rank-independent sample density, blocks of (sweep -> all-reduce -> step) rounds
with one read-back per block, the agreement of the ranks without a broadcast, the dl_max_sweeps budget, the concentration stage
through key_rank_pairs, ranks without tiles.  The device steps (sl_sdict_sweep / sl_sdict_step, sl_slide_key_*) are the numpy stand-ins
of tests/pool_vahadane_standins.py and tests/pool_standins.py, which keep the contracts of include/stainlib_hip.h: a sweep returns this rank's 31 class-moment sums and its pixel count, a step
updates the dictionary from the ALL-REDUCED sums alone.  The stand-in step is one plain block-coordinate pass per round (the
kernel's accelerated solve is tested on the GPU, tests/test_gpu_pool_vahadane.py), so the fixed point is the oracle's."""
import numpy as np
import pytest
import torch

from stainlib_amd import distributed as sd
from tests.pool_vahadane_standins import LAM, ab_from_moments, bcd_pass, class_moments
from tests.ranks import run_ranks


def test_bcd_on_summed_per_tile_class_moments_is_the_dictionary_of_the_concatenation():
    """Pure numpy: the sums decompose.  Per-tile class moments under a shared D, added up, give the A and B of the concatenated
    slide's exact codes, and iterating the update on them reaches vahadane_dictionary's result on the concatenated OD."""
    from oracle import stain_oracle as so
    tiles = [so.synth_tile(40, 56, 500 + s) for s in range(3)] + [so.structured_tile("white_bg", 48, 40, 3).transpose(1, 0, 2).copy()]
    ods = [so.rgb_to_od(t).reshape(-1, 3)[so.tissue_mask(t).ravel()] for t in tiles]
    od_all = np.concatenate(ods)
    D = so.vahadane_init(od_all)
    for _ in range(3):
        mom = sum(class_moments(od, D) for od in ods)
        A, B = ab_from_moments(mom, D)
        C = so.lasso2_nonneg(od_all, D, LAM)
        np.testing.assert_allclose(A, C.T @ C, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(B, od_all.T @ C, rtol=1e-9, atol=1e-9)
        D = bcd_pass(A, B, D)
    D = so.vahadane_init(od_all)
    for _ in range(40):
        D = bcd_pass(*ab_from_moments(sum(class_moments(od, D) for od in ods), D), D)
    np.testing.assert_allclose(D, so.vahadane_dictionary(od_all, LAM, max_sweeps=40, tol=0.0), rtol=0, atol=1e-10)


def _slide(kind):
    from oracle import stain_oracle as so
    if kind == "empty":
        return [np.full((40, 48, 3), 250, np.uint8) for _ in range(3)]
    return [so.synth_tile(40, 48, 700 + s) for s in range(4)] + [so.structured_tile("white_bg", 48, 40, 5).transpose(1, 0, 2).copy()]


def _worker(rank, world, shards, pass_total, max_sweeps, kind):
    from tests import pool_standins, pool_vahadane_standins
    pool_standins.install()
    calls = []
    pool_vahadane_standins.install(calls)
    from stainlib_amd.utils.excepts import TissueMaskException
    tiles = _slide(kind)
    lo = sum(shards[:rank])
    mine = torch.from_numpy(np.stack(tiles)[lo:lo + shards[rank]].copy())
    stats = sd.PooledVahadaneStatistics(dl_tol=1e-9, dl_max_sweeps=max_sweeps)
    try:
        M, maxC = stats(mine, n_tiles_total=len(tiles) if pass_total else None)
        return rank, M, maxC, stats.last_sweeps, stats.last_rounds, list(stats.last_path), len(calls)
    except TissueMaskException:
        return rank, "empty"


def _run(shards, pass_total=True, max_sweeps=600, kind="slide"):
    return run_ranks(_worker, len(shards), shards, pass_total, max_sweeps, kind, timeout=300)


_ONE = {}


def _one_process_and_oracle():
    from oracle import stain_oracle as so
    if not _ONE:
        tall = np.concatenate(_slide("slide"), axis=0)
        M_ref = so.vahadane_stain_matrix(tall, max_sweeps=2000, tol=1e-11)
        _ONE.update(one=_run((5,), True)[0], M_ref=M_ref, c_ref=np.percentile(so.get_concentrations(tall, M_ref), 99, axis=0))
    return _ONE["one"], _ONE["M_ref"], _ONE["c_ref"]


@pytest.mark.parametrize("shards,pass_total", [((3, 2), True), ((2, 3), False), ((5, 0), False), ((0, 5), True)])
def test_pooled_vahadane_on_two_gloo_ranks_matches_the_oracle_on_the_concatenation(shards, pass_total):
    res = _run(shards, pass_total)
    one, M_ref, c_ref = _one_process_and_oracle()
    for rank, M, maxC, sweeps, rounds, path, n_calls in res:
        assert np.array_equal(M, res[0][1]) and np.array_equal(maxC, res[0][2])     # the ranks agree to the bit
        assert (sweeps, rounds, path, n_calls) == res[0][3:]                          # ... and on every round they took
        assert n_calls % (2 * sd.PooledVahadaneStatistics.ROUNDS_PER_BLOCK) == 0      # whole blocks of rounds
        np.testing.assert_allclose(M, one[1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(maxC, one[2], rtol=1e-9)
        np.testing.assert_allclose(M, M_ref, rtol=0, atol=1e-7)
        np.testing.assert_allclose(maxC, c_ref, rtol=2e-6)


def test_pooled_vahadane_honours_the_sweep_budget_on_two_gloo_ranks():
    res = _run((3, 2), max_sweeps=3)
    one = _run((5,), max_sweeps=3)[0]
    for r in res:
        assert r[3] == 3                                                              # stopped at the budget, with the last iterate
        assert np.array_equal(r[1], res[0][1])
        np.testing.assert_allclose(r[1], one[1], rtol=0, atol=1e-12)
    assert one[3] == 3


def test_pooled_vahadane_empty_tissue_raises_on_every_rank():
    res = _run((2, 1), kind="empty")
    assert [r[1] for r in res] == ["empty", "empty"]


def test_slide_normalizer_refuses_graph_capture_with_a_vahadane_normalizer():
    class _V:
        method = "vahadane"
    with pytest.raises(ValueError):
        sd.SlideNormalizer(_V(), mode="pooled", graph=True)

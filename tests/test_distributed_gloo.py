"""CPU, world_size = 2, gloo: the N>1 host path (sharding, stats gather with uneven shards, slide statistics).
No GPU compute is involved: per-tile statistics are synthetic tensors."""
import numpy as np
import pytest
import torch

from stainlib_amd import distributed as sd
from tests.ranks import run_ranks
from tests.standin_math import f2ord as _f2ord


def test_shard_range_partitions_exactly():
    for n in (0, 1, 7, 8, 100000):
        for world in (1, 2, 3, 8):
            spans = [sd.shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        sd.shard_range(4, 2, 2)


def _table(n, seed=0):
    rng = np.random.RandomState(seed)
    M = rng.rand(n, 2, 3) + 0.1
    M /= np.linalg.norm(M, axis=2, keepdims=True)
    maxC = rng.rand(n, 2) + 1.0
    status = (rng.rand(n) < 0.2).astype(np.int32)
    status[0] = 0
    return torch.from_numpy(M), torch.from_numpy(maxC), torch.from_numpy(status)


def _worker(rank, world, n):
    M, maxC, status = _table(n)
    lo, hi = sd.shard_range(n, rank, world)
    Ma, ca, sa = sd.gather_tile_stats(M[lo:hi], maxC[lo:hi], status[lo:hi])
    Ms, cs = sd.slide_statistics(Ma, ca, sa)
    return rank, Ma.numpy(), ca.numpy(), sa.numpy(), Ms.numpy(), cs.numpy()


@pytest.mark.parametrize("n", [7, 10])           # 7: uneven shards (3 + 4)
def test_gather_and_slide_statistics_world2(n):
    res = run_ranks(_worker, 2, n, timeout=120)
    M, maxC, status = _table(n)
    Ms1, cs1 = sd.slide_statistics(M, maxC, status)          # the single-process answer
    for rank, Ma, ca, sa, Ms, cs in res:
        assert np.array_equal(Ma, M.numpy()) and np.array_equal(ca, maxC.numpy()) and np.array_equal(sa, status.numpy())
        assert np.array_equal(Ms, Ms1.numpy()) and np.array_equal(cs, cs1.numpy())   # identical on every rank
    np.testing.assert_allclose(np.linalg.norm(res[0][4], axis=1), 1.0, atol=1e-12)


def test_single_process_passthrough_and_errors():
    M, maxC, status = _table(5)
    Ma, ca, sa = sd.gather_tile_stats(M, maxC, status)
    assert torch.equal(Ma, M) and torch.equal(ca, maxC) and torch.equal(sa, status)
    with pytest.raises(ValueError):
        sd.slide_statistics(M, maxC, torch.ones(5, dtype=torch.int32))


# ---- pooled slide-level mode: the distributed exact order statistic (radix select over all-reduced histograms) ----
def _keys(rank, world, n=5000, seed=3):
    rng = np.random.RandomState(seed)
    run = np.float32(2.0) + np.arange(40, dtype=np.float32) * np.spacing(np.float32(2.0))       # 40 consecutive binary32 values
    allk = np.concatenate([rng.randn(n).astype(np.float32), np.zeros(400, np.float32), np.float32([1.5] * 7), run])  # ties + zeros
    rng.shuffle(allk)
    lo, hi = sd.shard_range(len(allk), rank, world)
    return allk, allk[lo:hi]


def _rank_pairs_with_numpy_histograms(mine, ks, wide=False):
    """Stand-in for the device kernels: histograms / next-above of THIS rank's keys with numpy; target 0 = the keys,
    target 1 = their negation (so the two targets walk different prefixes in lockstep)."""
    o = [_f2ord(mine).astype(np.uint64), _f2ord(-mine).astype(np.uint64)]

    def hist_fn(prefixes, bits):
        rows = []
        for t in range(2):
            sel = o[t] if bits == 0 else o[t][(o[t] >> np.uint64(32 - bits)) == np.uint64(prefixes[t])]
            b = (sel >> np.uint64(24 - bits)) & np.uint64(255)
            rows.append(np.bincount(b.astype(np.int64), minlength=256).astype(np.int64))
        return torch.from_numpy(np.stack(rows))

    def next_above_fn(keys):
        out = []
        for t in range(2):
            g = o[t][o[t] > np.uint64(keys[t])]
            out.append(int(g.min()) if len(g) else 0xffffffff)
        return out
    def hist16_fn(prefixes):                       # the last two rounds in one: low 16 bits under a 16-bit prefix
        rows = []
        for t in range(2):
            sel = o[t][(o[t] >> np.uint64(16)) == np.uint64(prefixes[t])]
            rows.append(np.bincount((sel & np.uint64(0xffff)).astype(np.int64), minlength=65536).astype(np.int64))
        return torch.from_numpy(np.stack(rows))
    return sd.exact_rank_pairs(hist_fn, next_above_fn, ks, hist16_fn=hist16_fn if wide else None)


def _worker_rank_pair(rank, world, ks, wide=False):
    _, mine = _keys(rank, world)
    return rank, [_rank_pairs_with_numpy_histograms(mine, (k, k2), wide) for k, k2 in ks]


@pytest.mark.parametrize("wide", [False, True])      # True: 8 + 8 + 16 bits (three rounds), False: four 8-bit rounds
def test_exact_rank_pairs_world2_match_sorted_union(wide):
    ks = [(0, 5406), (53, 2699), (2500, 2500), (5399, 17), (10 ** 9, 0)]   # incl. inside the block of ties and beyond the end
    res = run_ranks(_worker_rank_pair, 2, ks, wide, timeout=120)
    allk, _ = _keys(0, 1)
    srt = [np.sort(allk), np.sort(-allk)]
    assert res[0][1] == res[1][1]                            # identical on every rank
    for (k0, k1), pair in zip(ks, res[0][1]):
        for t, k in enumerate((k0, k1)):
            a, b, total = pair[t]
            kk = min(k, len(srt[t]) - 1)
            assert total == len(srt[t])
            assert sd.ord_to_float(a) == srt[t][kk] and sd.ord_to_float(b) == srt[t][min(kk + 1, len(srt[t]) - 1)]


def test_exact_rank_pairs_successor_inside_the_last_window():
    """Ranks inside a run of consecutive binary32 values: the k+1-th key comes from the last histogram round (no
    next_above sweep); checked against the sorted keys (single process: the rounds are the same without a group)."""
    allk, _ = _keys(0, 1)
    srt = [np.sort(allk), np.sort(-allk)]
    k2 = int(np.searchsorted(srt[0], np.float32(2.0)))
    calls = []
    o = [_f2ord(allk).astype(np.uint64), _f2ord(-allk).astype(np.uint64)]

    def hist_fn(prefixes, bits):
        rows = []
        for t in range(2):
            sel = o[t] if bits == 0 else o[t][(o[t] >> np.uint64(32 - bits)) == np.uint64(prefixes[t])]
            rows.append(np.bincount(((sel >> np.uint64(24 - bits)) & np.uint64(255)).astype(np.int64), minlength=256).astype(np.int64))
        return torch.from_numpy(np.stack(rows))

    def next_above_fn(keys):
        calls.append(tuple(keys))
        return [int(o[t][o[t] > np.uint64(keys[t])].min()) if (o[t] > np.uint64(keys[t])).any() else 0xffffffff for t in range(2)]
    n = len(allk)
    for k in (k2 + 3, k2 + 17, k2 + 38):
        kneg = n - 1 - (k + 1)                       # the same pair of values seen from the negated keys
        res = sd.exact_rank_pairs(hist_fn, next_above_fn, (k, kneg))
        for t, kk in enumerate((k, kneg)):
            a, b, total = res[t]
            assert total == n and sd.ord_to_float(a) == srt[t][kk] and sd.ord_to_float(b) == srt[t][kk + 1]
    assert calls == []                               # every successor sat inside the 256-key window


def _window_fns(mine):
    """numpy stand-ins for sl_slide_key_histogram_sampled (every 4th key as the sample) and sl_slide_key_window."""
    o = [_f2ord(mine).astype(np.uint64), _f2ord(-mine).astype(np.uint64)]
    smp = [x[::4] for x in o]

    def sample_hist_fn(prefixes, bits):
        rows = []
        for t in range(2):
            sel = smp[t] if bits == 0 else smp[t][(smp[t] >> np.uint64(32 - bits)) == np.uint64(prefixes[t])]
            rows.append(np.bincount(((sel >> np.uint64(24 - bits)) & np.uint64(255)).astype(np.int64), minlength=256).astype(np.int64))
        return torch.from_numpy(np.stack(rows))

    def window_fn(lo):
        out = np.zeros(2 * 65536 + 2, np.int64)
        for t in range(2):
            d = o[t].astype(np.int64) - int(lo[t])
            out[2 * 65536 + t] = int((d < 0).sum())
            out[t * 65536:(t + 1) * 65536] = np.bincount(d[(d >= 0) & (d < 65536)], minlength=65536)
        return torch.from_numpy(out)
    return sample_hist_fn, window_fn


def _worker_window(rank, world, ks, n_total):
    _, mine = _keys(rank, world)
    sf, wf = _window_fns(mine)
    return rank, [sd.window_rank_pairs(sf, wf, kk, (n_total, n_total)) for kk in ks]


def test_window_rank_pairs_world2():
    """One-sweep selection: exact when the window (centred on the sample estimate) holds ranks k and k+1, None otherwise
    -- identically on every rank.  The keys are N(0,1): 65536 consecutive binary32 values span ~0.8 % of a value, so
    central ranks of 5447 keys miss the window (None -> the caller's radix rounds) while the block of 400 zeros
    and the run of consecutive values around 2.0 are hit."""
    allk, _ = _keys(0, 1)
    n = len(allk)
    srt = [np.sort(allk), np.sort(-allk)]
    kz = int(np.searchsorted(srt[0], np.float32(0.0))) + 100          # inside the zeros (ties)
    k2 = int(np.searchsorted(srt[0], np.float32(2.0))) + 5            # inside the run of consecutive values
    ks = [(kz, n - 1 - kz - 1), (k2, n - 1 - k2 - 1), (10, 10)]
    res = run_ranks(_worker_window, 2, ks, n, timeout=120)
    assert res[0][1] == res[1][1]
    hits = 0
    for kk, pair in zip(ks, res[0][1]):
        if pair is None:
            continue
        hits += 1
        for t, k in enumerate(kk):
            a, b, total = pair[t]
            assert total == n and sd.ord_to_float(a) == srt[t][k] and sd.ord_to_float(b) == srt[t][min(k + 1, n - 1)]
    assert hits >= 2 and res[0][1][2] is None or hits == 3


def test_percentile_position_and_lerp_follow_numpy():
    rng = np.random.RandomState(0)
    x = np.sort(rng.rand(1001))
    for pct in (1.0, 99.0, 50.0, 0.0, 100.0):
        k, g = sd.percentile_position(len(x), pct)
        assert sd.np_lerp(x[k], x[min(k + 1, len(x) - 1)], g) == np.percentile(x, pct)


# ---- the REAL PooledSlideStatistics.__call__ / SlideNormalizer.transform_shard on two gloo ranks ------------------------
# The engine's device sweeps are replaced by the numpy stand-ins of tests/pool_standins.py (see there for their contracts);
# everything else is the product code of stainlib_amd/distributed.py executing.
def _slide_tiles(big=False):
    from oracle import stain_oracle as so
    if big:      # ~100 k pixels: neighbouring order statistics lie well inside one 65536-key window, both stages take the one-sweep path
        return [so.synth_tile(128, 128, 300 + s) for s in range(5)] + [so.structured_tile("white_bg", 128, 128, 7)]
    return [so.synth_tile(48, 64, 300 + s) for s in range(5)] + [so.structured_tile("white_bg", 64, 48, 7).transpose(1, 0, 2).copy()]


class _FittedTarget:                       # what SlideNormalizer needs of a fitted normalizer
    def __init__(self):
        from oracle import stain_oracle as so
        n = so.ExtractiveStainNormalizer("macenko")
        n.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
        self.stain_matrix_target, self.maxC_target = n.stain_matrix_target, n.maxC_target


def _pooled_worker(rank, world, force_radix, big=False):
    from tests import pool_standins
    pool_standins.install(force_radix)
    tiles = _slide_tiles(big)
    lo, hi = sd.shard_range(len(tiles), rank, world)              # 6 tiles -> 3 + 3; rank 1 holds the white-background tile
    mine = torch.from_numpy(np.stack(tiles[lo:hi]))
    stats = sd.PooledSlideStatistics()
    M, maxC = stats(mine, merged=False)                           # the three-sweep chain (the one-sweep chain: further down)
    out, M_s, mc_s, st = sd.SlideNormalizer(_FittedTarget(), mode="pooled", merged=False).transform_shard(mine)
    return rank, M, maxC, list(stats.last_path), out.numpy(), M_s.numpy(), mc_s.numpy()


@pytest.mark.parametrize("force_radix", [False, True])
def test_pooled_slide_statistics_real_call_on_two_gloo_ranks(force_radix):
    from oracle import stain_oracle as so
    res = run_ranks(_pooled_worker, 2, force_radix, timeout=300)
    # the single-rank run of the same code, and the reference's statistics of the concatenated slide
    one = run_ranks(_pooled_worker, 1, force_radix, timeout=300)[0]
    tall = np.concatenate(_slide_tiles(), axis=0)
    M_ref = so.macenko_stain_matrix(tall)
    c_ref = np.percentile(so.get_concentrations(tall, M_ref), 99, axis=0)
    for rank, M, maxC, path, out, M_s, mc_s in res:
        # (on a slide of 18 k pixels the ranks k and k+1 of the 99th percentile lie further apart than one window is wide:
        #  that stage legitimately falls back -- on every rank alike, since the decision is made on all-reduced counts)
        assert path == (["radix", "radix"] if force_radix else ["window", "radix"]) and path == one[3]
        assert np.array_equal(M, res[0][1]) and np.array_equal(maxC, res[0][2])    # the ranks agree to the bit (no broadcast needed)
        np.testing.assert_allclose(M, one[1], rtol=0, atol=1e-12)                  # = the single-rank run up to the order of the
        np.testing.assert_allclose(maxC, one[2], rtol=1e-12)                       #   moment sums (all-reduce of two partial sums)
        np.testing.assert_allclose(M, M_ref, rtol=0, atol=2e-6)                    # = the reference on the concatenated image
        np.testing.assert_allclose(maxC, c_ref, rtol=2e-6)
        assert np.array_equal(M_s, M) and np.array_equal(mc_s, maxC)
    both = np.concatenate([res[0][4], res[1][4]])                                  # the two shards' outputs = the single-rank output
    d = both.astype(np.int16) - one[4].astype(np.int16)
    assert np.abs(d).max() <= 1 and (d != 0).sum() <= 2                            # (1e-16 in M can flip a byte on a knife edge)


def test_device_driven_pooled_statistics_on_two_gloo_ranks():
    """The device-driven chain (PooledSlideStatistics.enqueue / finish: per step one all-reduce, decisions in the pool state, one
    read-back at the end) on two gloo ranks with a slide large enough for both windows to catch their ranks: the ranks agree to
    the bit, match the single-rank run and the reference's statistics of the concatenated slide, and no host-driven round ran."""
    from oracle import stain_oracle as so
    res = run_ranks(_pooled_worker, 2, False, True, timeout=600)
    one = run_ranks(_pooled_worker, 1, False, True, timeout=600)[0]
    tall = np.concatenate(_slide_tiles(True), axis=0)
    M_ref = so.macenko_stain_matrix(tall)
    c_ref = np.percentile(so.get_concentrations(tall, M_ref), 99, axis=0)
    for rank, M, maxC, path, out, M_s, mc_s in res:
        assert path == ["window", "window"] and path == one[3]                     # the device-driven path settled both stages
        assert np.array_equal(M, res[0][1]) and np.array_equal(maxC, res[0][2])    # the ranks agree to the bit
        np.testing.assert_allclose(M, one[1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(maxC, one[2], rtol=1e-12)
        np.testing.assert_allclose(M, M_ref, rtol=0, atol=2e-6)
        np.testing.assert_allclose(maxC, c_ref, rtol=2e-6)
        assert np.array_equal(M_s, M) and np.array_equal(mc_s, maxC)


def _density_worker(rank, world, pass_total):
    """Uneven shards (3 + 4 tiles of 1024^2 on two ranks): what sample density does each rank hand to the sampled histogram passes?"""
    from stainlib_amd import _ffi, engine
    seen = []
    engine.make_params = lambda **kw: None
    engine.tile_moments = lambda tiles, params=None, ws=None: torch.zeros((tiles.shape[0], 10), dtype=torch.float64)
    engine.pool_begin = lambda mom, state=None, params=None: torch.zeros((_ffi.POOL_STATE_DOUBLES,), dtype=torch.float64)

    def pool_histogram(tiles, keyset, state, rnd, slog, hist_out, params=None):
        seen.append(int(slog))
        return hist_out
    engine.pool_histogram = pool_histogram
    engine.pool_pick = lambda state, keyset, rnd, h: None
    engine.pool_window = lambda tiles, keyset, state, buf, params=None: buf
    engine.pool_resolve = lambda state, keyset, win, params=None: None
    lo, hi = sd.shard_range(7, rank, world)
    mine = torch.empty((hi - lo, 1024, 1024, 3), dtype=torch.uint8)
    sd.PooledSlideStatistics().enqueue(mine, n_tiles_total=7 if pass_total else None)
    return rank, hi - lo, seen


@pytest.mark.parametrize("pass_total", [False, True])
def test_uneven_shards_agree_on_the_sample_density(pass_total):
    """Round-3 advisor finding: the density was derived from each rank's OWN tile count; with 3 + 4 tiles of 1024^2 on two ranks
    (2 x 4 Mpx = 8.4 Mpx -> every other row; 2 x 3 Mpx = 6.3 Mpx -> every row) the all-reduced sample histograms mixed densities."""
    res = run_ranks(_density_worker, 2, pass_total, timeout=300)
    assert sorted(r[1] for r in res) == [3, 4]
    assert res[0][2] == res[1][2] and len(res[0][2]) == 6 and len(set(res[0][2])) == 1
    assert res[0][2][0] == (0 if pass_total else 1)          # 7 Mpx -> every row; agreed-on 2 x 4 Mpx -> every other row


# ---- the ONE-SWEEP pooled chain (PooledSlideStatistics.enqueue_merged, sl_pool2_*) on two gloo ranks: the product orchestration with
# the numpy stand-ins of tests/pool2_standins.py (see there for what they restate and what they replace by harness knowledge) ----------
def _many_tiles():
    """48 tiles of 384 x 256 (4.7 Mpx: the chain's sample is one pixel in two), two of them background"""
    from oracle import stain_oracle as so
    return [so.synth_tile(384, 256, 500 + s) for s in range(46)] + [np.full((384, 256, 3), 255, np.uint8)] * 2


def _merged_worker(rank, world, break_it=False, tiles_fn="big"):
    from tests import pool2_standins, pool_standins
    pool_standins.install(False)
    tiles = _slide_tiles(True) if tiles_fn == "big" else _many_tiles()
    pool2_standins.install(tiles, break_it)
    lo, hi = sd.shard_range(len(tiles), rank, world)
    mine = torch.from_numpy(np.stack(tiles[lo:hi]))
    stats = sd.PooledSlideStatistics()
    direct = stats.finish(stats.enqueue_merged(mine, n_tiles_total=len(tiles)))
    miss = stats.last_miss
    M, maxC = stats(mine, n_tiles_total=len(tiles))
    path = list(stats.last_path)
    out, M_s, mc_s, st = sd.SlideNormalizer(_FittedTarget(), mode="pooled").transform_shard(mine, n_tiles_total=len(tiles))
    return rank, direct is not None, miss, M, maxC, path, out.numpy(), M_s.numpy(), mc_s.numpy()


def _run_merged(world, break_it=False, tiles_fn="big"):
    res = run_ranks(_merged_worker, world, break_it, tiles_fn, timeout=900)
    return res


@pytest.mark.parametrize("tiles_fn", ["big", "many"])
def test_one_sweep_pooled_chain_on_two_gloo_ranks(tiles_fn):
    """PooledSlideStatistics.enqueue_merged / SlideNormalizer.transform_shard (the product orchestration) on two gloo ranks: the ranks
    agree to the bit without a broadcast, match the single-rank run and the reference's statistics of the concatenated slide, and
    the one-sweep chain settled both stages ("big": the sample is every pixel; "many": one pixel in two)."""
    from oracle import stain_oracle as so
    res, one = _run_merged(2, tiles_fn=tiles_fn), _run_merged(1, tiles_fn=tiles_fn)[0]
    tiles = _slide_tiles(True) if tiles_fn == "big" else _many_tiles()
    tall = np.concatenate(tiles, axis=0)
    M_ref = so.macenko_stain_matrix(tall)
    c_ref = np.percentile(so.get_concentrations(tall, M_ref), 99, axis=0)
    for rank, direct, miss, M, maxC, path, out, M_s, mc_s in res:
        assert direct and miss == 0 and path == ["merged", "merged"] and path == one[5]
        assert np.array_equal(M, res[0][3]) and np.array_equal(maxC, res[0][4])         # the ranks agree to the bit
        np.testing.assert_allclose(M, one[3], rtol=0, atol=1e-10)                       # = the single-rank run up to the order of the moment sums
        np.testing.assert_allclose(maxC, one[4], rtol=1e-10)                            #   (numpy's pairwise sums over 4.7 M pixels: 1e-11)
        np.testing.assert_allclose(M, M_ref, rtol=0, atol=2e-6)                         # = the reference on the concatenated image
        np.testing.assert_allclose(maxC, c_ref, rtol=2e-6)
        assert np.array_equal(M_s, M) and np.array_equal(mc_s, maxC)
    both = np.concatenate([res[0][6], res[1][6]])
    d = both.astype(np.int16) - one[6].astype(np.int16)
    assert np.abs(d).max() <= 1 and (d != 0).sum() <= 2


def test_one_sweep_pooled_chain_reports_a_miss_and_the_caller_falls_back_on_two_gloo_ranks():
    """A candidate list that lacks pixels it should hold (the stand-in's sweep drops the end of the lower angular tail): the chain's
    checks catch it on every rank alike (a miss, NaN statistics, never a wrong number) and __call__ / transform_shard settle the slide
    with the three-sweep chain -- same numbers as the reference."""
    from oracle import stain_oracle as so
    res = _run_merged(2, break_it=True)
    tall = np.concatenate(_slide_tiles(True), axis=0)
    M_ref = so.macenko_stain_matrix(tall)
    for rank, direct, miss, M, maxC, path, out, M_s, mc_s in res:
        assert not direct and (miss & 1) and path == ["window", "window"]
        assert np.array_equal(M, res[0][3]) and np.array_equal(maxC, res[0][4])
        np.testing.assert_allclose(M, M_ref, rtol=0, atol=2e-6)
        assert np.array_equal(M_s, M)


def test_sample_density_of_the_one_sweep_chain_is_a_function_of_the_slide_alone():
    """sample_log2_for: the whole slide up to 4 Mpx, then a sample that grows like pixels^(2/3) (one 64-pixel sub-row in 2^s) -- a pure
    function of the agreed pixel count, so that every rank picks the same density without a collective; the forced density of the
    tests (PooledSlideStatistics.sample_log2) overrides it on the instance only."""
    from stainlib_amd.distributed import PooledSlideStatistics as S
    assert [S.sample_log2_for(n) for n in (1, 1 << 20, 1 << 22)] == [0, 0, 0]
    assert S.sample_log2_for((1 << 22) + 1) == S.sample_log2_for(5_000_000) == 3
    assert S.sample_log2_for(512 << 20) == 6 and S.sample_log2_for(12_500 << 20) == 7 and S.sample_log2_for(100_000 << 20) == 8
    last = 0
    for e in range(0, 41):
        s = S.sample_log2_for(1 << e)
        assert 0 <= s <= 12 and s >= last                         # monotone, within what sl_pool2_* accept
        last = s
    a, b = S(group=False), S(group=False)
    a.sample_log2 = 4
    assert b.sample_log2 is None and S(group=False).sample_log2 is None

"""Multi-GPU sharding of the stain-normalization path: one process per GPU, torch.distributed.

Tiles are independent in the reference (ExtractiveStainNormalizer.transform re-estimates the stain
matrix and the 99th-percentile concentrations from each tile, normalizer.py:45-47), so the per-tile
mode shards contiguous tile ranges over ranks and needs NO data-path collective.

The only exchange is small and optional:
  * ``gather_tile_stats``  all-gather of the per-tile (M 2x3, maxC 2, status) = 9 numbers/tile, for QC
    and for
  * slide-level mode (BASELINE.json configs[4]): every tile of a slide is normalised with ONE stain
    matrix / ONE pair of 99th-percentile concentrations -- the per-slide median of the per-tile
    estimates over valid tiles.  Each rank fits its own tiles, the 9 numbers per tile are all-gathered
    (RCCL over xGMI on GPUs, gloo in the CPU tests; latency-bound: 36 B/tile), every rank reduces the
    same gathered table to the same slide statistics, and the apply pass runs locally.
This is an extension (the reference has no notion of a slide); its check is the same recipe run on one process.

  * POOLED slide-level mode (``SlideNormalizer(..., mode="pooled")``): the slide statistics are
    exactly those the reference computes from the vertical concatenation of ALL tiles as one tall image --
    covariance over every tissue pixel of the slide, 1st/99th angular percentiles over those pixels, 99th
    percentile of each concentration over every pixel.  Sums and order statistics decompose over tiles and
    ranks: per-tile moment sums are all-reduced (10 doubles), and each exact order statistic of the binary32
    key is pinned by a 4-round radix select whose 256-bin histograms are all-reduced (two order statistics per
    sweep, 4 KiB per round).  All
    collectives are tiny and latency-bound.  Oracle: the reference restatement on the concatenated image.
    With a Vahadane normalizer (``PooledVahadaneStatistics``) the stain matrix is the dictionary learnt on every tissue pixel of the
    slide: under one shared dictionary a sweep reduces each rank's tiles to 31 class-moment sums, those are all-reduced (32 doubles
    with the pixel count), and one workgroup takes the update on every rank alike; a few such rounds reach the fixed point.  The 99th
    percentile of each concentration under that matrix is pinned by the same order-statistic machinery as Macenko's.
    With a Reinhard normalizer (``PooledReinhardStatistics``) everything is a sum of integers -- the histogram of all bytes, the histogram
    of L8 and four sums over a8 and b8 --, so two small all-reduces give the reference's result on the concatenation byte for byte;
    ``slide_luminosity_standardize`` is LuminosityStandardizer on the concatenation from the same L8 histogram.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous range [lo, hi) of the n tiles owned by `rank` (sizes differ by at most one)."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    return (rank * n) // world, ((rank + 1) * n) // world


# Test hook: run the collectives even in a ONE-rank process group, so that a single GPU exercises the RCCL path end to end
# (bench.py sets it under SL_BENCH_FORCE_DIST=1; tests/test_gpu_rccl.py).  Off: a one-rank job pays for no collective.
COLLECTIVES_AT_WORLD_1 = False


def _coll(world: int, group=None) -> bool:
    """Whether the collectives of a step run: more than one rank, or the test hook above with a live process group."""
    if world > 1:
        return True
    return bool(COLLECTIVES_AT_WORLD_1 and group is not False and dist.is_available() and dist.is_initialized())


def _reduced(t: torch.Tensor, world: int, group=None) -> torch.Tensor:
    """t, summed over the ranks in place when the collectives run (``_coll``)."""
    if _coll(world, group):
        dist.all_reduce(t, group=group)
    return t


def _world(group=None):
    if group is False:           # "this process only": no collective even when a process group exists
        return 0, 1
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def gather_tile_stats(M: torch.Tensor, maxC: torch.Tensor, status: torch.Tensor, group=None):
    """All ranks' per-tile statistics in global tile order: (M_all (N,2,3), maxC_all (N,2), status_all (N,)).

    Shards may have different sizes; they are padded to the largest for the all-gather and trimmed after."""
    rank, world = _world(group)
    n_local = M.shape[0]
    packed = torch.cat([M.reshape(n_local, 6).double(), maxC.reshape(n_local, 2).double(),
                        status.reshape(n_local, 1).double()], dim=1)
    if not _coll(world, group):
        return M.reshape(n_local, 2, 3), maxC.reshape(n_local, 2), status.reshape(n_local)
    counts = torch.zeros(world, dtype=torch.int64, device=packed.device)
    counts[rank] = n_local
    dist.all_reduce(counts, group=group)
    n_max = int(counts.max())
    pad = torch.zeros((n_max, 9), dtype=torch.float64, device=packed.device)
    pad[:n_local] = packed
    bucket = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bucket, pad, group=group)
    allp = torch.cat([bucket[r][: int(counts[r])] for r in range(world)], dim=0)
    return allp[:, :6].reshape(-1, 2, 3), allp[:, 6:8], allp[:, 8].to(torch.int32)


def slide_statistics(M_all: torch.Tensor, maxC_all: torch.Tensor, status_all: torch.Tensor):
    """Per-slide stain matrix (2,3; unit-norm rows) and maxC (2,): element-wise median over the tiles whose
    fit succeeded.  Deterministic, so every rank derives identical values from the same gathered table."""
    ok = status_all == 0
    if int(ok.sum()) == 0:
        raise ValueError("no tile of the slide has a valid stain estimate")
    M = torch.quantile(M_all[ok].double(), 0.5, dim=0)            # numpy-style median (mean of the middle two)
    M = M / M.norm(dim=1, keepdim=True)
    maxC = torch.quantile(maxC_all[ok].double(), 0.5, dim=0)
    return M, maxC


# ---- exact order statistics of a key that is spread over tiles and ranks ------------------------------------------
def ord_to_float(o: int) -> float:
    """Inverse of the order-preserving uint32 image of a binary32 value (include/stainlib_hip.h)."""
    import struct
    bits = (o & 0x7fffffff) if (o & 0x80000000) else (~o & 0xffffffff)
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def percentile_position(n: int, pct: float):
    """numpy.percentile(method='linear'): 0-based rank k and interpolation weight g between ranks k and k+1."""
    vi = min(max((pct / 100.0) * (n - 1), 0.0), float(n - 1))
    k = math.floor(vi)
    return int(k), vi - k


def np_lerp(a: float, b: float, t: float) -> float:
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def exact_rank_pairs(hist_fn, next_above_fn, ks, group=None, hist16_fn=None, fractions=None, stop_bits=32):
    """For each of TWO targets t: the keys of ranks ks[t] and min(ks[t]+1, N_t-1) (0-based, ascending) of the union of
    every rank's keys of that target, as ordered uint32: [(key_k, key_k1, N_t), ...].

    hist_fn(prefixes, prefix_bits) -> int64 (2, 256) tensor: per target THIS rank's histogram of the next 8 key bits
    among its keys whose top prefix_bits bits equal prefixes[t]; next_above_fn(keys) -> per target this rank's smallest
    key above keys[t] (0xffffffff if none).  Both targets advance in lockstep, so the all-reduced histogram rounds that
    pin one order statistic exactly pin both (one sweep over the tiles per round).  With hist16_fn(prefixes16) ->
    int64 (2, 65536) (the low 16 bits of the keys under a 16-bit prefix) the last two rounds are one sweep: 8 + 8 + 16
    bits.  The k+1-th key is read off the last round's histogram (its bins are keys); the extra next_above sweep only
    runs when the k-th key is the largest of its window and unique."""
    _, world = _world(group)
    prefix, below, in_bin, total, k = [0, 0], [0, 0], [0, 0], [None, None], [int(ks[0]), int(ks[1])]
    succ = [None, None]          # the next larger key inside the last round's window, if there is one
    rounds = [(0, 8), (8, 8), (16, 16)] if hist16_fn is not None else [(0, 8), (8, 8), (16, 8), (24, 8)]
    for bits, width in rounds:
        if bits >= stop_bits:        # an estimate is enough: the remaining low bits are set to the middle of their range
            rest = 32 - bits
            return [((prefix[t] << rest) | (1 << (rest - 1)), (prefix[t] << rest) | (1 << (rest - 1)), total[t]) for t in range(2)]
        h = hist16_fn(prefix) if width == 16 else hist_fn(prefix, bits)
        if _coll(world, group):
            dist.all_reduce(h, group=group)
        hc = h.detach().cpu().numpy().astype(np.int64)
        last = bits + width == 32
        for t in range(2):
            if total[t] is None:
                total[t] = int(hc[t].sum())
                if total[t] == 0:
                    raise ValueError("no pixel carries this key")
                if fractions is not None:          # the rank as a fraction of however many keys there turn out to be
                    k[t] = int(fractions[t] * (total[t] - 1))
                k[t] = min(max(k[t], 0), total[t] - 1)
            cum = np.cumsum(hc[t])
            b = int(np.searchsorted(cum, k[t] - below[t], side="right"))     # first bin with below + cum[b] > k
            if last:                 # the bins of the last round ARE keys: the successor is the next non-empty bin
                nz = np.nonzero(hc[t][b + 1:])[0]
                succ[t] = None if len(nz) == 0 else ((prefix[t] << width) | (b + 1 + int(nz[0])))
            below[t] += int(cum[b] - hc[t][b])
            in_bin[t] = int(hc[t][b])
            prefix[t] = (prefix[t] << width) | b
    need = [not (k[t] + 1 < below[t] + in_bin[t] or k[t] + 1 >= total[t]) for t in range(2)]
    nxt = list(prefix)
    for t in range(2):           # the sweep for the next larger key is only needed when the window holds none
        if need[t] and succ[t] is not None:
            nxt[t], need[t] = succ[t], False
    if any(need) and next_above_fn is not None:
        got = next_above_fn(prefix)
        if _coll(world, group):
            tt = torch.tensor(got, dtype=torch.int64, device="cuda" if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MIN, group=group)
            got = [int(x) for x in tt.tolist()]
        nxt = [(got[t] if (need[t] and got[t] != 0xffffffff) else nxt[t]) for t in range(2)]
    return [(prefix[t], nxt[t], total[t]) for t in range(2)]


def window_rank_pairs(sample_hist_fn, window_fn, ks, totals, group=None):
    """The same result as exact_rank_pairs in ONE sweep over the tiles (plus four over a 1/64 pixel sample), or None.

    sample_hist_fn(prefixes, prefix_bits) -> (2, 256) int64: this rank's histogram over its pixel SAMPLE; the exact
    order statistic of the union of the samples at the same fraction estimates the key.  window_fn(lo) -> (2 * 65536 + 2,)
    int64: per target this rank's histogram of key - lo[t] inside [lo[t], lo[t] + 65536) and its count of keys below
    lo[t].  The window is centred on the estimate; if the wanted ranks k and k + 1 (totals[t] keys in all) do not both
    fall inside it -- the estimate was off by more than 32768 consecutive binary32 values -- the answer is None and the
    caller takes the radix rounds.  Everything is all-reduced, so all ranks decide alike."""
    _, world = _world(group)
    fr = [(int(ks[t]) / (totals[t] - 1)) if totals[t] > 1 else 0.0 for t in range(2)]
    try:
        est = exact_rank_pairs(sample_hist_fn, None, (0, 0), group, fractions=[min(max(f, 0.0), 1.0) for f in fr], stop_bits=24)
    except ValueError:
        return None
    lo = [min(max(est[t][0] - 32768, 0), 0xffffffff - 65535) for t in range(2)]
    buf = window_fn(lo)
    if _coll(world, group):
        dist.all_reduce(buf, group=group)
    b = buf.detach().cpu().numpy().astype(np.int64)
    out = []
    for t in range(2):
        hist, below, n = b[t * 65536:(t + 1) * 65536], int(b[2 * 65536 + t]), int(totals[t])
        k = min(max(int(ks[t]), 0), n - 1)
        k1 = min(k + 1, n - 1)
        inside = int(hist.sum())
        if not (below <= k and k1 < below + inside):
            return None
        cum = np.cumsum(hist)
        i0 = int(np.searchsorted(cum, k - below, side="right"))
        i1 = int(np.searchsorted(cum, k1 - below, side="right"))
        out.append((lo[t] + i0, lo[t] + i1, n))
    return out


def key_rank_pairs(tiles_local: torch.Tensor, keyset: int, basis, ks, totals, sample_log2: int, params, group=None, path=None):
    """Per target of the key set under ``basis``: the binary32 keys of ranks ks[t] and ks[t] + 1 of the whole slide as floats.  One sweep
    with the window centred on an estimate from a pixel sample (one row in 2**sample_log2), the radix rounds if it missed; appends
    "window" or "radix" to ``path``.  A rank without tiles takes part in every collective with empty histograms."""
    from . import engine
    dev = tiles_local.device
    empty = tiles_local.shape[0] == 0
    if empty:                    # (the library refuses n == 0: the counts of no pixel are zeros)
        hist_s = lambda pre, bits: torch.zeros((2, 256), dtype=torch.int64, device=dev)
        win = lambda lo: torch.zeros((2 * 65536 + 2,), dtype=torch.int64, device=dev)
        hist = lambda pre, bits: torch.zeros((2, 256), dtype=torch.int64, device=dev)
        hist16 = lambda pre: torch.zeros((2, 65536), dtype=torch.int64, device=dev)
        above = lambda o: [0xffffffff, 0xffffffff]
    else:
        hist_s = lambda pre, bits: engine.slide_key_histogram_sampled(tiles_local, keyset, basis, pre, bits, sample_log2, params=params)
        win = lambda lo: engine.slide_key_window(tiles_local, keyset, basis, lo, params=params)
        hist = lambda pre, bits: engine.slide_key_histogram(tiles_local, keyset, basis, pre, bits, params=params)
        hist16 = lambda pre: engine.slide_key_histogram16(tiles_local, keyset, basis, pre, params=params)
        above = lambda o: engine.slide_key_next_above(tiles_local, keyset, basis, o, params=params)
    res = window_rank_pairs(hist_s, win, ks, totals, group)
    if path is not None:
        path.append("window" if res is not None else "radix")
    if res is None:
        res = exact_rank_pairs(hist, above, ks, group, hist16_fn=hist16)
    return [(ord_to_float(a), ord_to_float(b)) for a, b, _ in res]


def _agreed_pixels(tiles_local, n_tiles_total, world, group):
    """The slide's pixel count as every rank computes it alike.  A sample density must be the SAME on every rank (the sampled histograms
    are all-reduced), so it is derived from a rank-independent tile count: the caller's n_tiles_total, else the largest shard (shard_range
    gives ceil(n / world) to some rank) agreed on with one tiny MAX all-reduce whose result is read back -- NOT from this rank's own n_local,
    which differs by one tile across ranks on uneven shards and can sit on the other side of a power of two (3 vs 4 tiles of 1024^2 on two
    ranks; round-3 advisor finding).  Results never depend on it, only which route settles them."""
    n_local, h, w, _ = tiles_local.shape
    if n_tiles_total is not None:
        return int(n_tiles_total) * h * w
    if _coll(world, group) and world > 1:
        nl = torch.tensor([n_local], dtype=torch.int64, device=tiles_local.device if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(nl, op=dist.ReduceOp.MAX, group=group)
        return world * int(nl.item()) * h * w
    return world * n_local * h * w


def window_sample_log2(n_pixels: int) -> int:
    """Density of the window path's pixel sample (one row in 2**result): ~4 M pixels of the slide or more, everything for small slides."""
    return min(6, max(0, int(math.floor(math.log2(max(n_pixels, 1) / 4.0e6))))) if n_pixels > 4.0e6 else 0


def pooled_max_concentrations(tiles_local: torch.Tensor, M, n_pixels: int, params, group=None, path=None):
    """99th percentile of each concentration under the stain matrix M (numpy 2x3) over the slide's n_pixels pixels (normalizer.py:36,47),
    both columns per sweep, as numpy float64 (2,).  Appends the route of ``key_rank_pairs`` to ``path``."""
    from . import _ffi
    k, g = percentile_position(n_pixels, 99.0)
    (ca0, cb0), (ca1, cb1) = key_rank_pairs(tiles_local, _ffi.KEYSET_CONC, M.reshape(6), (k, k), (n_pixels, n_pixels),
                                            window_sample_log2(n_pixels), params, group, path)
    return np.array([np_lerp(float(ca0), float(cb0), g), np_lerp(float(ca1), float(cb1), g)], dtype=np.float64)


class _PooledStatistics:
    """What the pooled statistics of both methods share: the process group and the normalizer's parameters."""

    def __init__(self, group=None, luminosity_threshold=0.8, angular_percentile=99.0, lasso_lambda=0.01):
        from .utils.stain_utils import check_percentile
        self.group = group
        self.thr, self.pct, self.lam = luminosity_threshold, check_percentile(angular_percentile), lasso_lambda
        self.last_path = []          # how each stage of the last call settled ("merged", "window" or "radix")
        self.sample_log2 = None      # None: the sample density follows the slide's pixel count (sample_log2_for); 0...12: one 64-pixel sub-row in 2^s
                                     # (tests and experiments; the same on every rank -- the RESULT does not depend on it, only which route settles it)

    def params(self):
        from . import engine
        return engine.make_params(luminosity_threshold=self.thr, angular_percentile=self.pct, lasso_lambda=self.lam)


class PooledSlideStatistics(_PooledStatistics):
    """Stain matrix and 99th-percentile concentrations of the tall image made of every tile on every rank."""

    last_miss = 0                # state[POOL_MISS] of the last device-driven chain read back
    last_why = 0                 # state[POOL2_WHY] of the last one-sweep chain (why the sample gave no estimate)

    def enqueue(self, tiles_local: torch.Tensor, ws=None, n_tiles_total: Optional[int] = None) -> torch.Tensor:
        """DEVICE-DRIVEN: enqueue the whole computation (4 full sweeps, 6 sampled passes, the all-reduces between them and the
        single-workgroup decision steps) on the current stream and return the pool state tensor (device float64,
        _ffi.POOL_STATE_DOUBLES): state[POOL_M:POOL_M+6] / state[POOL_MAXC:+2] are the slide's stain matrix and maxC once
        state[POOL_STATUS] == 0 and state[POOL_MISS] == 0 (``finish`` checks them with one read-back).  Every rank reaches the same
        state: each step consumes all-reduced data only.
        With ``n_tiles_total`` (the slide's tile count over ALL ranks -- every rank must pass the same value, or none of them may) nothing
        is read back and no extra collective runs; on one rank the chain is then graph-capturable.  WITHOUT it, on more than one rank,
        the sample density is agreed on with one small MAX all-reduce of the shard sizes whose result IS read back (a host
        synchronisation per call): pass the total where the call sits on a latency-critical path.  Ranks that disagree on whether they
        pass it issue different collective sequences and hang -- it is part of the call's collective contract."""
        from . import engine, _ffi
        params = self.params()
        _, world = _world(self.group)
        n_local, h, w, _ = tiles_local.shape
        dev = tiles_local.device
        # 10 moment sums + this rank's pixel count (torch.full: a fill kernel -- a scalar copied from the host could not be captured)
        mom = _reduced(torch.cat([engine.tile_moments(tiles_local, params=params, ws=ws).sum(dim=0),
                                  torch.full((1,), float(n_local * h * w), dtype=torch.float64, device=dev)]), world, self.group)
        state = engine.pool_begin(mom, params=params)
        slog = window_sample_log2(_agreed_pixels(tiles_local, n_tiles_total, world, self.group))
        hists = torch.zeros((2, 3, 2, 256), dtype=torch.int64, device=dev)
        wins = torch.zeros((2, 2 * 65536 + 2), dtype=torch.int64, device=dev)
        for si, keyset in enumerate((_ffi.KEYSET_ANGLE, _ffi.KEYSET_CONC)):
            for rnd in range(3):
                hb = engine.pool_histogram(tiles_local, keyset, state, rnd, slog, hists[si, rnd], params=params)
                engine.pool_pick(state, keyset, rnd, _reduced(hb, world, self.group))
            wb = engine.pool_window(tiles_local, keyset, state, wins[si], params=params)
            engine.pool_resolve(state, keyset, _reduced(wb, world, self.group), params=params)
        return state

    MERGED_LEVELS = 3            # window levels enqueued per key set by the one-sweep chain (11 key bits each; SL_POOL2_LEVELS)
    one_call = True              # on one process the chain is enqueued by sl_pool2_local (False: step by step, as on several ranks)

    @staticmethod
    def sample_log2_for(n_pixels: int) -> int:
        """Density of the merged chain's pixel sample (one 64-pixel sub-row in 2**result): everything up to 4 Mpx, then the sample grows
        like the slide's size to the power 2/3 -- the candidate lists shrink like 1/sqrt(sample) while the sample passes grow with it."""
        if n_pixels <= (1 << 22):
            return 0
        return int(min(12, max(0, math.floor((math.log2(n_pixels) - 11.0) / 3.0))))

    def enqueue_merged(self, tiles_local: torch.Tensor, ws=None, n_tiles_total: Optional[int] = None) -> torch.Tensor:
        """DEVICE-DRIVEN, ONE full sweep (round 6; csrc/slide_merged.hip): a stratified pixel sample of the whole slide gives an estimate
        of the eigenvectors, the angular brackets and the stain matrix; the one sweep over the tiles computes the exact moment sums AND
        appends every pixel that is not proven plain under that estimate to a candidate list; the exact order statistics are then those
        of the candidates (four passes over the list).  Ten small all-reduces: the sample moments, the two sample histograms, the sweep
        totals and six candidate levels -- and one MAX more when n_tiles_total is None on more than one rank.  Returns the pool state
        (device float64, _ffi.POOL2_STATE_DOUBLES) with the layout of ``enqueue``'s in its first ten entries.  state[POOL_MISS] != 0 at the
        end: a check of the estimate failed (or a list overflowed) -- results never depend on the sample, the caller takes ``enqueue`` then.
        n_tiles_total: as for ``enqueue`` (the same on every rank, or on none).  ws: None, or a dict the caller keeps between calls (the
        chain's workspace -- sample list, candidate list of up to 1/8 of the pixels -- is then allocated once per shape)."""
        from . import engine, _ffi
        params = self.params()
        _, world = _world(self.group)
        n_local, h, w, _ = tiles_local.shape
        dev = tiles_local.device
        slog = self.sample_log2_for(_agreed_pixels(tiles_local, n_tiles_total, world, self.group)) if self.sample_log2 is None else int(self.sample_log2)
        if ws is None or ws.get("key") != (n_local, h, w, slog, dev):
            buf = engine.pool2_workspace(n_local, h, w, slog, dev)
            if ws is not None:               # a caller's cache (a dict): the buffer is reused by its next call with this shape
                ws.clear()
                ws.update(key=(n_local, h, w, slog, dev), buf=buf)
            ws = {"buf": buf}
        ws = ws["buf"]
        if not _coll(world, self.group) and self.one_call:   # one process: the chain enqueued by ONE call into the library (the same kernels in the same order)
            self._merged_ws = ws
            return engine.pool2_local(tiles_local, slog, ws, params=params)
        shape = (n_local, h, w)
        hists = torch.empty((2 + 2 * self.MERGED_LEVELS, _ffi.POOL2_HIST_WORDS), dtype=torch.int64, device=dev)   # every pass writes its buffer whole
        mom = _reduced(engine.pool2_sample(tiles_local, slog, ws, params=params), world, self.group)
        state = engine.pool2_begin(mom, slog, params=params)
        for i, keyset in enumerate((_ffi.KEYSET_ANGLE, _ffi.KEYSET_CONC)):
            hist = engine.pool2_hist(0, keyset, 0, shape, slog, state, ws, hists[i], params=params)
            engine.pool2_bands(state, keyset, _reduced(hist, world, self.group))
        engine.pool2_exact(_reduced(engine.pool2_sweep(tiles_local, slog, state, ws, params=params), world, self.group), state)
        for i, keyset in enumerate((_ffi.KEYSET_ANGLE, _ffi.KEYSET_CONC)):
            for level in range(self.MERGED_LEVELS):      # (a settled key set turns its remaining passes and steps into no-ops)
                hist = engine.pool2_hist(1, keyset, 1, shape, slog, state, ws, hists[2 + self.MERGED_LEVELS * i + level], params=params)
                engine.pool2_step(state, keyset, _reduced(hist, world, self.group))
        self._merged_ws = ws             # (kept until the next call: the chain's kernels are still queued when this returns)
        return state

    def finish(self, state: torch.Tensor):
        """The one read-back of the device-driven path: (M, maxC) as numpy, or None when a window missed (the caller then runs the
        host-driven rounds).  Raises like the reference on an empty tissue mask, and like MacenkoStainExtractor.get_stain_matrix on a
        degenerate slide (fewer than two tissue pixels, or two parallel stain vectors -- an angular percentile of 50 makes them so:
        the host-driven rounds have no such check and would divide by the singular Gram matrix)."""
        from . import _ffi
        from .utils.stain_utils import raise_for_status
        s = state.cpu().numpy()
        status, miss = int(s[_ffi.POOL_STATUS]), int(s[_ffi.POOL_MISS])
        raise_for_status(status)
        self.last_miss = miss
        if len(s) > _ffi.POOL2_WHY:
            self.last_why = int(s[_ffi.POOL2_WHY])
        if status != 0 or miss != 0:
            return None
        self.last_path = ["merged", "merged"] if len(s) == _ffi.POOL2_STATE_DOUBLES else ["window", "window"]
        return s[_ffi.POOL_M:_ffi.POOL_M + 6].reshape(2, 3).copy(), s[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2].copy()

    def settle(self, tiles_local: torch.Tensor, n_tiles_total: Optional[int] = None, merged: bool = True, ws=None, behind=None, first=None):
        """(M, maxC, state) of the slide: the one-sweep chain (``merged``; or first(), a replay of it that returns its state), the three-sweep
        chain if one of its checks fails, the host-driven radix rounds if a window misses -- the same numbers whichever route settles them.
        behind(state) enqueues work behind each eager chain, before its one read-back.  state: the pool state of the chain that settled
        them, None after the host-driven rounds.  n_tiles_total: see ``enqueue``; ws: the one-sweep chain's cache (``enqueue_merged``)."""
        def eager(enqueue, **kw):
            state = enqueue(tiles_local, n_tiles_total=n_tiles_total, **kw)
            if behind is not None:
                behind(state)
            return state
        rungs = ([first or (lambda: eager(self.enqueue_merged, ws=ws))] if merged else []) + [lambda: eager(self.enqueue)]
        for rung in rungs:
            state = rung()
            got = self.finish(state)
            if got is not None:
                return got + (state,)
        return self.host_driven(tiles_local) + (None,)

    def __call__(self, tiles_local: torch.Tensor, device_driven: bool = True, n_tiles_total: Optional[int] = None, merged: bool = True):
        """(M, maxC) of the slide, settled as ``settle`` does; device_driven=False: the host-driven rounds only.  n_tiles_total: see
        ``enqueue`` (the same on every rank, or on none)."""
        if not device_driven:
            return self.host_driven(tiles_local)
        return self.settle(tiles_local, n_tiles_total, merged)[:2]

    def host_driven(self, tiles_local: torch.Tensor):
        """The same statistics with the decisions on the host (a read-back per step): the radix fallback lives here."""
        from . import engine, _ffi
        from .utils.excepts import TissueMaskException
        params = self.params()
        self.last_path = []
        _, world = _world(self.group)
        n_local, h, w, _ = tiles_local.shape
        # ---- covariance of the optical density over every tissue pixel (macenko_stain_extractor.py:18-27)
        mom = engine.tile_moments(tiles_local, params=params).sum(dim=0)
        npx = torch.tensor([float(n_local * h * w)], dtype=torch.float64, device=mom.device)
        if _coll(world, self.group):
            dist.all_reduce(mom, group=self.group)
            dist.all_reduce(npx, group=self.group)
        m = mom.cpu().numpy()
        T, n_pixels = int(round(m[0])), int(round(float(npx.item())))
        if T < 1:
            raise TissueMaskException("Empty tissue mask computed")
        mean = m[1:4] / T
        S2 = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
        cov = (S2 - T * np.outer(mean, mean)) / (T - 1.0)
        _, V = np.linalg.eigh(cov)
        V = V[:, [2, 1]].copy()
        for i in range(2):
            if V[0, i] < 0:
                V[:, i] *= -1.0
        Vf = V.astype(np.float32).astype(np.float64)                # the keys are evaluated in binary32
        # ---- exact angular percentiles over those pixels (:29-34): both in the same four sweeps
        def angle_of_pseudo(p):
            if abs(p) <= 1.0:
                return math.atan2(p, 1.0 - abs(p))
            pp = 2.0 - p if p > 0 else -2.0 - p
            return math.atan2(pp, -(1.0 - abs(pp)))
        pct = max(self.pct, 100.0 - self.pct)       # (100 - pct, pct) is the same pair either way; the window sweeps want target 0 below target 1
        (k_lo, g_lo), (k_hi, g_hi) = percentile_position(T, 100.0 - pct), percentile_position(T, pct)
        (xa0, xb0), (xa1, xb1) = key_rank_pairs(tiles_local, _ffi.KEYSET_ANGLE, Vf.reshape(6), (k_lo, k_hi), (T, T),
                                                window_sample_log2(n_pixels), params, self.group, self.last_path)
        phis = [np_lerp(angle_of_pseudo(xa0), angle_of_pseudo(xb0), g_lo), np_lerp(angle_of_pseudo(xa1), angle_of_pseudo(xb1), g_hi)]
        v1 = V @ np.array([math.cos(phis[0]), math.sin(phis[0])])          # :36-37
        v2 = V @ np.array([math.cos(phis[1]), math.sin(phis[1])])
        M = np.array([v1, v2]) if v1[0] > v2[0] else np.array([v2, v1])     # :40-43
        M = M / np.linalg.norm(M, axis=1, keepdims=True)                    # :44
        return M, pooled_max_concentrations(tiles_local, M, n_pixels, params, self.group, self.last_path)


class PooledVahadaneStatistics(_PooledStatistics):
    """Vahadane stain matrix and 99th-percentile concentrations of the tall image made of every tile on every rank
    (vahadane_stain_extractor.py:28-43 and normalizer.py:36,47 on the concatenation; csrc/slide_dict.hip).

    The dictionary stage is DEVICE-DRIVEN: blocks of ROUNDS_PER_BLOCK rounds (sweep -> all-reduce of 32 doubles -> step) are enqueued
    without a read-back; one read-back of the state per block says whether another block is needed.  Every rank reads the same state
    (each step consumes all-reduced sums only), so the ranks agree on it without a collective.  The concentrations are then pinned
    exactly by ``key_rank_pairs`` under the learnt matrix.  A rank may hold no tile; it still takes part in every collective."""

    ROUNDS_PER_BLOCK = 4         # rounds enqueued between two read-backs (like kDictFixedSweeps of the per-tile schedule)

    def __init__(self, group=None, luminosity_threshold=0.8, angular_percentile=99.0, lasso_lambda=0.01, dl_lambda=0.1, dl_tol=1e-7,
                 dl_max_sweeps=200):
        super().__init__(group, luminosity_threshold, angular_percentile, lasso_lambda)
        self.dl_lambda, self.dl_tol, self.dl_max_sweeps = dl_lambda, dl_tol, int(dl_max_sweeps)
        self.last_status = 0         # SL_TILE_* of the last call
        self.last_rounds = 0         # dictionary updates taken (sampled and full)
        self.last_sweeps = 0         # full sweeps among them
        self.last_blocks = 0         # read-backs of the dictionary stage
        self._ws = None

    @staticmethod
    def sample_log2_for(n_pixels: int) -> int:
        """Density of the sampled rounds: 1/64 of the sub-rows up to 4 Mpx (the per-tile fit samples 1/64 of the pixels), sparser beyond
        like the one-sweep Macenko chain's sample (PooledSlideStatistics.sample_log2_for), at most one sub-row in 4096."""
        return int(min(12, PooledSlideStatistics.sample_log2_for(n_pixels) + 6))

    def params(self):
        from . import engine
        return engine.make_params(luminosity_threshold=self.thr, angular_percentile=self.pct, lasso_lambda=self.lam,
                                  dl_lambda=self.dl_lambda, dl_tol=self.dl_tol, dl_max_sweeps=self.dl_max_sweeps)

    def dictionary(self, tiles_local: torch.Tensor, n_tiles_total: Optional[int] = None):
        """The dictionary stage; returns the final state as a float64 numpy array (_ffi.SDICT_STATE_DOUBLES).
        n_tiles_total: the slide's tile count over ALL ranks (the same on every rank, or on none -- part of the collective contract, as for
        ``PooledSlideStatistics.enqueue``); without it one MAX all-reduce agrees on the sample density."""
        from . import engine, _ffi
        params = self.params()
        _, world = _world(self.group)
        n_local, h, w, _ = tiles_local.shape
        dev = tiles_local.device
        slog = self.sample_log2_for(_agreed_pixels(tiles_local, n_tiles_total, world, self.group)) if self.sample_log2 is None else int(self.sample_log2)
        if self._ws is None or self._ws[0] != (n_local, h, w, dev):
            self._ws = ((n_local, h, w, dev), engine.sdict_workspace(n_local, h, w, dev))
        ws = self._ws[1]
        state = engine.sdict_begin(slog, dev, params=params)
        sums = torch.empty((self.ROUNDS_PER_BLOCK, _ffi.SDICT_SUMS), dtype=torch.float64, device=dev)
        # the sample stage takes at most 40 updates and the full sweeps dl_max_sweeps: the iteration settles within this many blocks
        max_blocks = (40 + self.dl_max_sweeps + 1) // self.ROUNDS_PER_BLOCK + 2
        for blk in range(max_blocks):
            for r in range(self.ROUNDS_PER_BLOCK):
                part = engine.sdict_sweep(tiles_local, slog, state, ws, sums=sums[r], params=params)
                engine.sdict_step(state, _reduced(part, world, self.group), params=params)
            s = state.cpu().numpy()
            if int(s[_ffi.SDICT_MODE]) == 0:
                break
        else:
            raise RuntimeError("the slide dictionary did not settle within its sweep budget")
        self.last_blocks = blk + 1
        self.last_rounds, self.last_sweeps = int(s[_ffi.SDICT_ROUNDS]), int(s[_ffi.SDICT_SWEEPS])
        return s

    def __call__(self, tiles_local: torch.Tensor, n_tiles_total: Optional[int] = None):
        """(M (2, 3), maxC (2,)) of the slide as numpy float64.  Raises TissueMaskException on an empty tissue mask (stain_utils.py:46-47).
        A degenerate dictionary (a dead atom, parallel atoms) or a zero concentration percentile gives NaN and self.last_status != 0."""
        from . import _ffi
        from .utils.excepts import TissueMaskException
        self.last_path = []
        s = self.dictionary(tiles_local, n_tiles_total)
        status = int(s[_ffi.SDICT_STATUS])
        self.last_status = status
        if status == _ffi.TILE_EMPTY_MASK:
            raise TissueMaskException("Empty tissue mask computed")
        if status != 0:
            return np.full((2, 3), np.nan), np.full(2, np.nan)
        M = s[_ffi.SDICT_M:_ffi.SDICT_M + 6].reshape(2, 3).copy()
        maxC = pooled_max_concentrations(tiles_local, M, int(round(float(s[_ffi.SDICT_NPX]))), self.params(), self.group, self.last_path)
        if not (maxC > 0).all():             # normalizer.py:48 would divide by it
            self.last_status = _ffi.TILE_ZERO_MAXC
        return M, maxC


class PooledReinhardStatistics:
    """The statistics ReinhardStainNormalizer.transform / LuminosityStandardizer.standardize take from an image (normalizer.py:78-80,
    stain_utils.py:64,188-194), of the tall image made of every tile on every rank (csrc/slide_lab.hip).

    DEVICE-DRIVEN: the sums of this rank's tiles, the two all-reduces (256 and 262 int64) and the single-workgroup steps are enqueued on
    the current stream; every step consumes all-reduced integer sums only, so every rank reaches the same state without a broadcast, and
    the state is the reference's on the concatenation exactly -- there is no fallback route.  ``finish`` is the one read-back.  A rank may
    hold no tile; it still takes part in both collectives."""

    def __init__(self, group=None):
        self.group = group
        self.last_status = 0                 # SL_TILE_* of the last state read back
        self.last_p90 = float("nan")         # 90th percentile of the slide's bytes (NaN for the luminosity chain)
        self.last_percentile = float("nan")  # the L percentile of the luminosity chain
        self.last_means = self.last_stds = None      # numpy (3,) float64
        self.last_tissue = self.last_pixels = 0
        self._ws = None

    def _workspace(self, tiles_local):
        from . import engine
        n_local, h, w, _ = tiles_local.shape
        key = (n_local, h, w, tiles_local.device)
        if self._ws is None or self._ws[0] != key:
            self._ws = (key, engine.slab_workspace(n_local, h, w, tiles_local.device))
        return self._ws[1]

    def enqueue(self, tiles_local: torch.Tensor, target_means, target_stds, mask_background=False, luminosity_threshold=0.8) -> torch.Tensor:
        """The Reinhard chain: bytes -> all-reduce -> begin -> Lab sums -> all-reduce -> finish.  Returns the state (device float64,
        _ffi.SLAB_STATE_DOUBLES); ``engine.slab_map(tiles, state, 0, ...)`` behind it maps the tiles."""
        from . import engine
        _, world = _world(self.group)
        ws = self._workspace(tiles_local)
        state = engine.slab_begin(_reduced(engine.slab_bytes(tiles_local, ws), world, self.group), True, tiles_local.device)
        sums = _reduced(engine.slab_lab(tiles_local, state, luminosity_threshold, ws), world, self.group)
        engine.slab_finish(state, sums, 0, target_means, target_stds, mask_background=mask_background)
        return state

    def enqueue_luminosity(self, tiles_local: torch.Tensor, percentile=95) -> torch.Tensor:
        """The luminosity chain: identity brightness (no bytes sweep), Lab sums -> all-reduce -> finish(mode 1)."""
        from . import engine
        _, world = _world(self.group)
        ws = self._workspace(tiles_local)
        state = engine.slab_begin(None, False, tiles_local.device)
        sums = _reduced(engine.slab_lab(tiles_local, state, 0.8, ws), world, self.group)
        engine.slab_finish(state, sums, 1, percentile=percentile)
        return state

    def finish(self, state: torch.Tensor):
        """The one read-back: the reported numbers into last_*; raises like the reference on an empty tissue mask (or an empty slide)."""
        from . import _ffi
        from .utils.excepts import TissueMaskException
        s = state[:_ffi.SLAB_TABLES].cpu().numpy()
        self.last_status = int(s[_ffi.SLAB_STATUS])
        self.last_p90, self.last_percentile = float(s[_ffi.SLAB_P90]), float(s[_ffi.SLAB_LPCT])
        self.last_means = s[_ffi.SLAB_MEANS:_ffi.SLAB_MEANS + 3].copy()
        self.last_stds = s[_ffi.SLAB_STDS:_ffi.SLAB_STDS + 3].copy()
        self.last_tissue, self.last_pixels = int(s[_ffi.SLAB_TISSUE]), int(s[_ffi.SLAB_NPX])
        if self.last_status == _ffi.TILE_EMPTY_MASK:
            raise TissueMaskException("Empty tissue mask computed")
        return self.last_status


def slide_luminosity_standardize(tiles_local: torch.Tensor, percentile=95, group=None, out: Optional[torch.Tensor] = None,
                                 tensor_format=None, view=None, windows=None):
    """LuminosityStandardizer.standardize (stain_utils.py:52-67) on the concatenation of every tile on every rank: (out, p), p the
    `percentile` of the slide's L8 as a float.  One sweep for the L8 histogram, one small all-reduce, the map.
    tensor_format: a stainlib_amd.TensorFormat; `out` is then the (n_local,3,H,W) tensor in that format (the map writes a uint8 scratch,
    tensor_format.convert reads it).
    view: a stainlib_amd.TileView -- the map sweep writes per tile only the window windows[t] (default: view.draw(n_local, H, W), drawn
    behind the statistics) of its result, flipped and turned, as (n_local,oh,ow,3) uint8 or the (n_local,3,oh,ow) tensor, without a
    scratch (engine.slab_view); the call returns (out, p, windows).  windows without view is a ValueError."""
    from . import engine
    with_view = engine.lab_view_check(view, windows, tiles_local)          # (before any collective: a refused call enqueues nothing)
    if with_view:
        engine._check_shard(tiles_local)
    stats = PooledReinhardStatistics(group)
    state = stats.enqueue_luminosity(tiles_local, percentile)
    if with_view:
        out, windows = engine.slab_view(tiles_local, windows, None, state, 1, fmt=tensor_format, out=out, view=view)
        stats.finish(state)
        return out, stats.last_percentile, windows
    if tensor_format is not None:
        out = tensor_format.convert(engine.slab_map(tiles_local, state, 1), out=out)
    else:
        out = engine.slab_map(tiles_local, state, 1, out=out)
    stats.finish(state)
    return out, stats.last_percentile


class SlideNormalizer:
    """Slide-level Macenko/Vahadane/Reinhard normalisation over a sharded set of tiles (see module docstring).

    mode="median" (default): per-tile fits, all-gather, element-wise median.  mode="pooled": the exact statistics
    of the concatenated slide -- ``PooledSlideStatistics`` for a Macenko normalizer, ``PooledVahadaneStatistics`` for a Vahadane one
    (dispatched on ``normalizer.method``), ``PooledReinhardStatistics`` for a ReinhardStainNormalizer (pooled mode only: mode="median" or
    graph=True with one raises ValueError).

    graph=True (pooled mode on ONE process: no collective sits between the steps): the one-sweep chain and the apply pass behind it --
    some fifty launches -- are captured into a HIP graph the first time a (tiles buffer, out buffer) pair is seen and REPLAYED on every
    later call with the same buffers (a pipeline that refills fixed staging buffers): 512 tiles 1.92 -> 1.84 ms, 128 tiles 0.79 -> 0.77.
    The read-back after the replay is the same one; a replay that ends in a miss falls back exactly like the eager chain.  `out` is
    allocated once and reused when the caller passes none.  Macenko only: graph=True with a Vahadane normalizer raises ValueError
    (its dictionary stage reads the state back between blocks of rounds)."""

    def __init__(self, normalizer, group=None, mode="median", merged=True, graph=False):
        if mode not in ("median", "pooled"):
            raise ValueError("mode must be 'median' or 'pooled'")
        if graph and getattr(normalizer, "method", "macenko") == "vahadane":
            raise ValueError("graph=True is not supported with a Vahadane normalizer")
        from .normalization.normalizer import ReinhardStainNormalizer
        self._reinhard = isinstance(normalizer, ReinhardStainNormalizer)
        self._reinhard_targets = None
        if self._reinhard and (mode != "pooled" or graph):
            raise ValueError("a Reinhard normalizer supports mode='pooled' without graph capture only")
        self.normalizer = normalizer          # a fitted stainlib_amd ExtractiveStainNormalizer
        self.group = group
        self.mode = mode
        self.merged = merged                  # pooled mode: the one-sweep chain first (PooledSlideStatistics.enqueue_merged)
        self.graph = graph
        self._pool2_ws = {}                   # its workspace, kept between calls
        self._graphed = None                  # (key, engine.Graphed, pinned tensors) of the last captured chain

    def _targets(self, device):
        """The normalizer's 8 target doubles for the apply pass: its cached device tensors where it has them (uploaded once per fit; as
        numpy arguments they are two small pageable copies per call), else the public attributes as they are."""
        cached = getattr(self.normalizer, "_target_on", None)
        if cached is not None:
            return cached(device)
        return self.normalizer.stain_matrix_target, self.normalizer.maxC_target.reshape(2)

    @staticmethod
    def _apply(tiles_local, M_s, maxC_s, Mt, mct, out, fmt=None):
        """The apply pass of every tile under the one slide matrix M_s (2, 3) and maxC_s (2,) (device float64); with a TensorFormat the
        pass that converts its bytes in registers (no uint8 image is written)."""
        from . import engine
        n = tiles_local.shape[0]
        M_n, maxC_n = M_s.expand(n, 2, 3).contiguous(), maxC_s.expand(n, 2).contiguous()
        if fmt is not None:
            return engine.normalize_apply_tensor(tiles_local, M_n, maxC_n, Mt, mct, fmt, out=out)
        return engine.normalize_apply(tiles_local, M_n, maxC_n, Mt, mct, out=out)

    @staticmethod
    def _slide_stats(state):         # views of the slide's (M, maxC) in a pool state
        from . import _ffi
        return state[_ffi.POOL_M:_ffi.POOL_M + 6].reshape(2, 3), state[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2]

    def transform_shard(self, tiles_local: torch.Tensor, out: Optional[torch.Tensor] = None, n_tiles_total: Optional[int] = None, *,
                        mask_background=False, luminosity_threshold=0.8, tensor_format=None, view=None, windows=None):
        """tiles_local: this rank's (n_local,H,W,3) uint8 device tensor.  Returns (out, M_slide, maxC_slide, status_local).
        n_tiles_total (pooled mode, optional): the slide's tile count over all ranks; saves the one tiny all-reduce that otherwise
        agrees on the sample density.  On failure (TissueMaskException) `out` holds a copy of the input tiles.
        With a Reinhard normalizer: returns (out, means, stds, status_local) -- the slide's Lab means and standard deviations as device
        float64 (3,) -- and sets ``last_p90``; mask_background / luminosity_threshold are ReinhardStainNormalizer.transform's (the
        extractive normalizers have no such arguments: a non-default value with one raises ValueError).
        tensor_format: a stainlib_amd.TensorFormat; `out` is then the (n_local,3,H,W) tensor in that format, bit for bit
        tensor_format.convert of the uint8 result: the apply pass of the extractive normalizers converts its bytes in registers, the
        Reinhard map writes a uint8 scratch that the converter reads.  Not with graph=True (ValueError).
        view, windows (a Reinhard normalizer only; ValueError otherwise): a stainlib_amd.TileView -- the pooled map sweep writes per tile
        only the window windows[t] (default: view.draw(n_local, H, W), drawn behind the statistics) of its result, flipped and turned,
        as (n_local,oh,ow,3) uint8 or the (n_local,3,oh,ow) tensor, without a scratch (engine.slab_view); `windows` is appended to the
        returned tuple.  On failure `out` then holds the view of the input tiles."""
        if tensor_format is not None and self.graph:
            raise ValueError("tensor_format is not supported with graph=True")
        if (view is not None or windows is not None) and not self._reinhard:
            raise ValueError("view / windows apply to a Reinhard normalizer only (the extractive normalizers' views: transform_batch)")
        if self._reinhard:
            return self._transform_reinhard(tiles_local, out, mask_background, luminosity_threshold, tensor_format, view, windows)
        if mask_background or luminosity_threshold != 0.8:
            raise ValueError("mask_background / luminosity_threshold apply to a Reinhard normalizer only")
        if self.mode == "median":
            return self._transform_median(tiles_local, out, tensor_format)
        if getattr(self.normalizer, "method", "macenko") == "vahadane":
            return self._transform_vahadane(tiles_local, out, n_tiles_total, tensor_format)
        return self._transform_macenko(tiles_local, out, n_tiles_total, tensor_format)

    def _transform_median(self, tiles_local: torch.Tensor, out: Optional[torch.Tensor], fmt=None):
        """Per-tile fits, all-gathered; every tile normalised with their element-wise median."""
        M, maxC, status = self.normalizer.fit_batch_targets(tiles_local)
        M_s, maxC_s = slide_statistics(*gather_tile_stats(M, maxC, status, self.group))
        out = self._apply(tiles_local, M_s, maxC_s, *self._targets(tiles_local.device), out, fmt)
        return out, M_s, maxC_s, status

    def _transform_macenko(self, tiles_local: torch.Tensor, out: Optional[torch.Tensor], n_tiles_total: Optional[int], fmt=None):
        """Pooled mode with a Macenko normalizer.  Device-driven: the statistics AND the apply pass are enqueued before anything is read
        back; the one read-back afterwards only confirms that both windows caught their ranks (else the next chain, or the host-driven
        rounds, and the pass again).  When a chain ends in an unusable state (a window miss, an empty tissue mask, a degenerate
        covariance) its last step leaves NaN in (M, maxC) and the enqueued apply pass COPIES the tiles through (k_apply's rule for
        unusable statistics): `out` then holds the input, never exp(NaN) bytes, until a later route rewrites it -- or, on an empty mask,
        when TissueMaskException leaves this function."""
        stats = PooledSlideStatistics(self.group)
        dev = tiles_local.device
        n = tiles_local.shape[0]
        Mt, mct = self._targets(dev)
        _, world = _world(self.group)
        first = None
        if self.graph and self.merged and stats.one_call and not _coll(world, self.group):
            graphed, out = self._captured_chain(stats, tiles_local, out, n_tiles_total, Mt, mct)
            first = graphed.replay

        def behind(st):                     # the apply pass behind each eager chain; the next route writes the same `out`
            nonlocal out
            out = self._apply(tiles_local, *self._slide_stats(st), Mt, mct, out, fmt)
        M_np, maxC_np, state = stats.settle(tiles_local, n_tiles_total, self.merged, ws=self._pool2_ws, first=first, behind=behind)
        if state is None:                   # the host-driven rounds settled it: the pass again, under their numbers
            M_s = torch.as_tensor(M_np, dtype=torch.float64, device=dev)
            maxC_s = torch.as_tensor(maxC_np, dtype=torch.float64, device=dev)
            out = self._apply(tiles_local, M_s, maxC_s, Mt, mct, out, fmt)
        else:
            M_s, maxC_s = (t.clone() for t in self._slide_stats(state))
        self.last_path = stats.last_path             # per stage: "merged" (one sweep for both), "window" (one each) or "radix"
        self.last_miss, self.last_why = stats.last_miss, stats.last_why
        return out, M_s, maxC_s, torch.zeros((n,), dtype=torch.int32, device=dev)

    def _captured_chain(self, stats, tiles_local: torch.Tensor, out: Optional[torch.Tensor], n_tiles_total: Optional[int], Mt, mct):
        """graph=True: (engine.Graphed of the one-sweep chain with the apply pass behind it, the `out` it writes).  The same buffers as
        last time are replayed; else the chain is captured (one warm-up run, one run under capture)."""
        from . import engine
        dev = tiles_local.device
        tgt_key = (np.asarray(self.normalizer.stain_matrix_target, dtype=np.float64).tobytes(),
                   np.asarray(self.normalizer.maxC_target, dtype=np.float64).tobytes())          # (host values: no device read-back for the key)
        if out is None:
            out = self._graphed[2]["out"] if (self._graphed and self._graphed[2]["out"].shape == tiles_local.shape
                                              and self._graphed[2]["out"].device == dev) else torch.empty_like(tiles_local)
        key = (tiles_local.data_ptr(), out.data_ptr(), tuple(tiles_local.shape), n_tiles_total, str(dev), stats.thr, stats.pct, stats.lam, tgt_key)
        if self._graphed is None or self._graphed[0] != key:
            keep = {"out": out, "tiles": tiles_local,
                    "Mt": torch.as_tensor(Mt, dtype=torch.float64, device=dev).reshape(2, 3).clone(),
                    "mct": torch.as_tensor(mct, dtype=torch.float64, device=dev).reshape(2).clone()}

            def captured():
                state = stats.enqueue_merged(tiles_local, n_tiles_total=n_tiles_total, ws=self._pool2_ws)
                self._apply(tiles_local, *self._slide_stats(state), keep["Mt"], keep["mct"], out)
                return state
            self._graphed = None                       # (the old graph goes before its buffers do)
            self._graphed = (key, engine.Graphed(captured), keep)
        return self._graphed[1], out

    def _transform_vahadane(self, tiles_local: torch.Tensor, out: Optional[torch.Tensor], n_tiles_total: Optional[int], fmt=None):
        """Pooled mode with a Vahadane normalizer: the slide's dictionary and concentrations, then the apply pass of the Macenko mode."""
        from .utils.excepts import TissueMaskException
        if self.graph:
            raise ValueError("graph=True is not supported with a Vahadane normalizer")
        stats = PooledVahadaneStatistics(self.group)
        dev = tiles_local.device
        n = tiles_local.shape[0]
        if fmt is not None:
            def through():             # "unchanged" in the format: the source bytes converted
                return fmt.convert(tiles_local, out=out)
        else:
            if out is None:
                out = torch.empty_like(tiles_local)

            def through():
                return out.copy_(tiles_local)
        try:
            M_np, maxC_np = stats(tiles_local, n_tiles_total=n_tiles_total)
        except TissueMaskException:
            through()
            raise
        finally:
            self.last_path = stats.last_path
            self.last_rounds, self.last_sweeps = stats.last_rounds, stats.last_sweeps
        M_s = torch.as_tensor(M_np, dtype=torch.float64, device=dev)
        maxC_s = torch.as_tensor(maxC_np, dtype=torch.float64, device=dev)
        if stats.last_status != 0:             # unusable statistics: the tiles go through unchanged, as k_apply does for a failed tile
            return through(), M_s, maxC_s, torch.full((n,), stats.last_status, dtype=torch.int32, device=dev)
        if n:
            out = self._apply(tiles_local, M_s, maxC_s, *self._targets(dev), out, fmt)
        elif fmt is not None:
            out = through()                    # an empty shard: the empty tensor in the format
        return out, M_s, maxC_s, torch.zeros((n,), dtype=torch.int32, device=dev)

    def _transform_reinhard(self, tiles_local: torch.Tensor, out: Optional[torch.Tensor], mask_background, luminosity_threshold, fmt=None,
                            view=None, windows=None):
        """Pooled mode with a Reinhard normalizer.  Device-driven: the statistics AND the map are enqueued before the one read-back; with
        an unusable status (an empty tissue mask under mask_background, an empty slide) the map copies the tiles through."""
        from . import engine, _ffi
        with_view = engine.lab_view_check(view, windows, tiles_local)      # (before any collective: a refused call enqueues nothing)
        if with_view:
            engine._check_shard(tiles_local)
        stats = PooledReinhardStatistics(self.group)
        tm, ts = self.normalizer._targets()
        key = (str(tiles_local.device), tuple(tm), tuple(ts))         # the six target doubles on the device, uploaded once per fit (cf. _target_on)
        if self._reinhard_targets is None or self._reinhard_targets[0] != key:
            self._reinhard_targets = (key, torch.tensor(tm, dtype=torch.float64, device=tiles_local.device),
                                      torch.tensor(ts, dtype=torch.float64, device=tiles_local.device))
        _, tm, ts = self._reinhard_targets
        state = stats.enqueue(tiles_local, tm, ts, mask_background, luminosity_threshold)
        if with_view:                          # the map, the view and the conversion in one sweep
            out, windows = engine.slab_view(tiles_local, windows, None, state, 0, mask_background=mask_background,
                                            luminosity_threshold=luminosity_threshold, fmt=fmt, out=out, view=view)
        elif fmt is not None:                  # the map into a uint8 scratch, then the converter
            out = fmt.convert(engine.slab_map(tiles_local, state, 0, mask_background, luminosity_threshold), out=out)
        else:
            out = engine.slab_map(tiles_local, state, 0, mask_background, luminosity_threshold, out=out)
        means = state[_ffi.SLAB_MEANS:_ffi.SLAB_MEANS + 3].clone()
        stds = state[_ffi.SLAB_STDS:_ffi.SLAB_STDS + 3].clone()
        try:
            stats.finish(state)
        finally:
            self.last_p90 = stats.last_p90
            self.last_tissue, self.last_pixels = stats.last_tissue, stats.last_pixels
        return (out, means, stds, torch.zeros((tiles_local.shape[0],), dtype=torch.int32, device=tiles_local.device)) + (
            (windows,) if with_view else ())

"""CPU, world_size = 2, gloo: the pooled slide-level Vahadane statistics (stainlib_amd/distributed.py PooledVahadaneStatistics).

The orchestration under test is the product's: the rank-independent sample density, blocks of (sweep -> all-reduce -> step) rounds
with one read-back per block, the agreement of the ranks without a broadcast, the dl_max_sweeps budget, the concentration stage
through key_rank_pairs, ranks without tiles.  The device steps (sl_sdict_sweep / sl_sdict_step, sl_slide_key_*) are numpy stand-ins
that keep the contracts of include/stainlib_hip.h: a sweep returns this rank's 31 class-moment sums and its pixel count, a step
updates the dictionary from the ALL-REDUCED sums alone.  The stand-in step is one plain block-coordinate pass per round (the
kernel's accelerated solve is tested on the GPU, tests/test_gpu_pool_vahadane.py), so the fixed point is the oracle's."""
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from stainlib_amd import distributed as sd
from tests.test_distributed_gloo import _free_port, _install_numpy_engine

LAM = 0.1


def _codes_classes(od, D, lam=LAM):
    from oracle import stain_oracle as so
    C = so.lasso2_nonneg(od, D, lam)
    a, b = C[:, 0] > 0, C[:, 1] > 0
    return C, (a & b, a & ~b, ~a & b)


def class_moments(od, D, lam=LAM):
    """the 31 sums a sweep under D returns: per class (both stains, stain 1 only, stain 2 only) {n, sum x (3), sum x x^T (6)}, tissue count"""
    _, cls = _codes_classes(od, D, lam)
    out = np.zeros(31)
    for c, m in enumerate(cls):
        x = od[m]
        S = x.T @ x
        out[10 * c:10 * c + 10] = [len(x), *x.sum(0), S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]
    out[30] = len(od)
    return out


def ab_from_moments(mom, D, lam=LAM):
    """A = sum alpha alpha^T, B = sum x alpha^T from the class moments (the codes of a class are affine in x: alpha = W x - w)"""
    G = D @ D.T
    A, B = np.zeros((2, 2)), np.zeros((3, 2))
    for c in range(3):
        m = mom[10 * c:10 * c + 10]
        n, s = m[0], m[1:4]
        S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
        if n <= 0:
            continue
        act = [0, 1] if c == 0 else [c - 1]
        P = np.zeros((2, 2))
        P[np.ix_(act, act)] = np.linalg.inv(G[np.ix_(act, act)])
        W, w = P @ D, lam * P @ np.ones(2)
        Ws = W @ s
        A += W @ S @ W.T - np.outer(Ws, w) - np.outer(w, Ws) + n * np.outer(w, w)
        B += S @ W.T - np.outer(s, w)
    return A, B


def bcd_pass(A, B, D):
    Dn = D.copy()
    for j in range(2):
        if A[j, j] > 1e-300:
            u = np.maximum((B[:, j] - Dn.T @ A[:, j]) / A[j, j] + Dn[j], 0.0)
            Dn[j] = u / max(np.linalg.norm(u), 1.0)
    return Dn


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


def _install_sdict(calls):
    """numpy stand-ins of sl_sdict_* (state layout of include/stainlib_hip.h SL_SDICT_*)"""
    from oracle import stain_oracle as so
    from stainlib_amd import _ffi, engine
    engine.make_params = lambda **kw: types.SimpleNamespace(**kw)

    def od_of(tiles, slog):
        T = tiles.numpy()
        if len(T) == 0:
            return np.zeros((0, 3)), 0
        rows = [so.rgb_to_od(t).reshape(-1, 3)[(so.lab_l8(t) / 255.0 < 0.8).ravel()][:: 1 << slog] for t in T]
        return np.concatenate(rows), T.shape[0] * T.shape[1] * T.shape[2]

    def sdict_workspace(n, h, w, device):
        return torch.empty(256, dtype=torch.uint8)

    def sdict_begin(slog, device, state=None, params=None):
        st = torch.zeros(_ffi.SDICT_STATE_DOUBLES, dtype=torch.float64)
        st[_ffi.SDICT_D:_ffi.SDICT_D + 6] = torch.from_numpy(so.normalize_rows(np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])).reshape(6))
        st[_ffi.SDICT_M:_ffi.SDICT_M + 6] = float("nan")
        st[_ffi.SDICT_MODE] = 1
        return st

    def sdict_sweep(tiles, slog, state, ws, sums=None, params=None):
        calls.append("sweep")
        out = np.zeros(_ffi.SDICT_SUMS)
        mode = int(state[_ffi.SDICT_MODE])
        od, npx = od_of(tiles, slog if mode == 1 else 0)
        if mode:
            out[:31] = class_moments(od, state[_ffi.SDICT_D:_ffi.SDICT_D + 6].numpy().reshape(2, 3), params.dl_lambda)
        out[31] = npx
        return torch.from_numpy(out)

    def sdict_step(state, sums, params=None):
        calls.append("step")
        s = sums.numpy()
        mode = int(state[_ffi.SDICT_MODE])
        if mode == 0:
            return
        if int(state[_ffi.SDICT_ROUNDS]) == 0:
            state[_ffi.SDICT_NPX] = float(s[31])
        state[_ffi.SDICT_ROUNDS] += 1
        D = state[_ffi.SDICT_D:_ffi.SDICT_D + 6].numpy().reshape(2, 3).copy()
        settled = False
        if s[30] < 1:
            delta = 0.0
            if mode == 2:
                state[_ffi.SDICT_STATUS] = _ffi.TILE_EMPTY_MASK
                settled = True
        else:
            Dn = bcd_pass(*ab_from_moments(s[:31], D, params.dl_lambda), D)
            delta = np.abs(Dn - D).max()
            D = Dn
            state[_ffi.SDICT_D:_ffi.SDICT_D + 6] = torch.from_numpy(D.reshape(6))
        if mode == 1:
            if delta < 1e-4:
                state[_ffi.SDICT_MODE] = 2
        else:
            state[_ffi.SDICT_SWEEPS] += 1
            settled = settled or delta < params.dl_tol or int(state[_ffi.SDICT_SWEEPS]) >= params.dl_max_sweeps
        if settled:
            if int(state[_ffi.SDICT_STATUS]) == 0:
                M = D[[1, 0]] if D[0, 0] < D[1, 0] else D
                state[_ffi.SDICT_M:_ffi.SDICT_M + 6] = torch.from_numpy(so.normalize_rows(M).reshape(6))
            state[_ffi.SDICT_MODE] = 0

    engine.sdict_workspace, engine.sdict_begin, engine.sdict_sweep, engine.sdict_step = sdict_workspace, sdict_begin, sdict_sweep, sdict_step


def _slide(kind):
    from oracle import stain_oracle as so
    if kind == "empty":
        return [np.full((40, 48, 3), 250, np.uint8) for _ in range(3)]
    return [so.synth_tile(40, 48, 700 + s) for s in range(4)] + [so.structured_tile("white_bg", 48, 40, 5).transpose(1, 0, 2).copy()]


def _worker(rank, world, port, shards, pass_total, max_sweeps, kind, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _install_numpy_engine()
        calls = []
        _install_sdict(calls)
        from stainlib_amd.utils.excepts import TissueMaskException
        tiles = _slide(kind)
        lo = sum(shards[:rank])
        mine = torch.from_numpy(np.stack(tiles)[lo:lo + shards[rank]].copy())
        stats = sd.PooledVahadaneStatistics(dl_tol=1e-9, dl_max_sweeps=max_sweeps)
        try:
            M, maxC = stats(mine, n_tiles_total=len(tiles) if pass_total else None)
            res = (rank, M, maxC, stats.last_sweeps, stats.last_rounds, list(stats.last_path), len(calls))
        except TissueMaskException:
            res = (rank, "empty")
        q.put(res)
        if world > 1:
            dist.barrier()
    finally:
        if world > 1:
            dist.destroy_process_group()


def _run(shards, pass_total=True, max_sweeps=600, kind="slide"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, len(shards), port, shards, pass_total, max_sweeps, kind, q)) for r in range(len(shards))]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


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

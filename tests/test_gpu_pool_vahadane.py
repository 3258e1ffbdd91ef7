"""-m gpu: the pooled slide-level Vahadane statistics (SlideNormalizer(VahadaneNormalizer(), mode="pooled"), csrc/slide_dict.hip)
against the oracle on the vertical concatenation of the slide's tiles: the converged dictionary (vahadane_stain_extractor.py:28-43),
the 99th-percentile concentrations over every pixel (normalizer.py:36,47) and the bytes of the apply pass."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests.gpu_util import to_dev, u8_parity
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu
V_ATOL = 1e-7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _target():
    import stainlib_amd as sl
    nrm = sl.VahadaneNormalizer()
    nrm.fit(so.synth_tile(256, 256, 1001, so.M_TRUE_TGT))
    return nrm


def _oracle_slide(tiles):
    tall = np.concatenate(tiles, axis=0)
    M = so.vahadane_stain_matrix(tall, max_sweeps=600, tol=1e-10)
    return M, np.percentile(so.get_concentrations(tall, M), 99, axis=0)


def _ihc_quarters():
    ihc = np.load(os.path.join(ROOT, "tests", "golden", "tissue_ihc_512.npz"))["input"]
    return [ihc[i:i + 256, j:j + 256].copy() for i in (0, 256) for j in (0, 256)]


SLIDES = {
    "synth8": lambda: [so.synth_tile(256, 256, 40 + 7 * s) for s in range(8)],
    "structured": lambda: [so.synth_tile(256, 256, 61), so.structured_tile("white_bg", 256, 256, 9), so.structured_tile("blobs", 256, 256, 5),
                           so.structured_tile("palette12", 256, 256, 4), so.structured_tile("quantized", 256, 256, 4)],
    "ihc4": _ihc_quarters,
    "synth2x1024": lambda: [so.synth_tile(1024, 1024, 90 + s) for s in range(2)],
}


# The dictionary's fixed point is the one of the binary32 class-moment bursts (stats_dict.hpp): a pixel next to a class boundary may
# land on the other side than in binary64.  On the IHC crop -- few distinct colours, so a whole colour cluster moves at once -- that
# shifts the fixed point by 1.37e-7 from the binary64 oracle, whatever dl_tol (measured 1e-7 ... 1e-9), and the per-tile fit of the
# concatenated image lands on the same point (to 1e-10): the bar there is 2e-7, and the pooled result must be the per-tile map's.
M_ATOL = {"ihc4": 2e-7}


@pytest.mark.parametrize("name", list(SLIDES))
def test_pooled_vahadane_matches_the_oracle_on_the_concatenated_slide(name):
    from stainlib_amd.distributed import SlideNormalizer
    tiles = SLIDES[name]()
    nrm = _target()
    sn = SlideNormalizer(nrm, mode="pooled")
    out, M_s, mc_s, st = sn.transform_shard(to_dev(tiles))
    M_s, mc_s, out = M_s.cpu().numpy(), mc_s.cpu().numpy(), out.cpu().numpy()
    assert (st.cpu().numpy() == 0).all()
    M_o, mc_o = _oracle_slide(tiles)
    print(name, "rounds", sn.last_rounds, "full sweeps", sn.last_sweeps, "maxC path", sn.last_path, "M err", np.abs(M_s - M_o).max())
    np.testing.assert_allclose(M_s, M_o, rtol=0, atol=M_ATOL.get(name, V_ATOL))
    np.testing.assert_allclose(mc_s, mc_o, rtol=2e-6)
    if name in M_ATOL:
        from stainlib_amd import engine
        M_t, _, s_t, _ = engine.vahadane_fit(to_dev([np.concatenate(tiles, axis=0)]))
        assert int(s_t[0]) == 0
        np.testing.assert_allclose(M_s, M_t[0].cpu().numpy(), rtol=0, atol=1e-8)
    Mt, mct = np.asarray(nrm.stain_matrix_target), np.asarray(nrm.maxC_target).reshape(1, 2)
    for i, I in enumerate(tiles):
        Cc = so.get_concentrations(I, M_o) * (mct / mc_o.reshape(1, 2))
        pre = 255 * np.exp(-1 * np.dot(Cc, Mt))
        want = so.truncate_u8(pre).reshape(I.shape)
        u8_parity(out[i], want, label=f"{name}[{i}]", src=I, prequant=pre.reshape(I.shape))


def _pooled(tiles_dev, **kw):
    from stainlib_amd.distributed import PooledVahadaneStatistics
    st = PooledVahadaneStatistics(group=False, **kw)
    M, mc = st(tiles_dev)
    return M, mc, st


def test_one_tile_slide_follows_the_per_tile_fit():
    from stainlib_amd import engine
    I = so.synth_tile(512, 384, 77)
    M1, mc1, s1, _ = engine.vahadane_fit(to_dev([I]))
    assert int(s1[0]) == 0
    M, mc, st = _pooled(to_dev([I]))
    np.testing.assert_allclose(M, M1[0].cpu().numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(mc, mc1[0].cpu().numpy(), rtol=2e-6)


def test_repeated_tile_gives_the_one_tile_dictionary():
    I = so.synth_tile(256, 320, 78)
    M1, _, _ = _pooled(to_dev([I]))
    M4, _, _ = _pooled(to_dev([I] * 4))
    np.testing.assert_allclose(M4, M1, rtol=0, atol=2e-7)


def test_two_calls_are_bit_identical():
    tiles = to_dev([so.synth_tile(256, 256, 80 + s) for s in range(6)])
    a = _pooled(tiles)
    b = _pooled(tiles)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].last_rounds == b[2].last_rounds


def test_empty_tissue_raises_and_leaves_the_input_in_out():
    from stainlib_amd.distributed import SlideNormalizer
    from stainlib_amd.utils.excepts import TissueMaskException
    tiles = to_dev([np.full((128, 160, 3), 245, np.uint8), np.full((128, 160, 3), 250, np.uint8)])
    out = torch.zeros_like(tiles)
    with pytest.raises(TissueMaskException):
        SlideNormalizer(_target(), mode="pooled").transform_shard(tiles, out=out)
    assert torch.equal(out, tiles)


def test_graph_capture_is_refused_for_vahadane():
    from stainlib_amd.distributed import SlideNormalizer
    with pytest.raises(ValueError):
        SlideNormalizer(_target(), mode="pooled", graph=True)


def test_sdict_entry_points_refuse_bad_arguments_and_accept_an_empty_shard():
    from stainlib_amd import _ffi, engine
    lib = _ffi.lib()
    BAD, WS = -1, -2
    dev = torch.device("cuda", 0)
    p = _ffi.default_params()
    bad_size = _ffi.default_params()
    bad_size.struct_size = 8
    rgb = to_dev([so.synth_tile(64, 64, 3)])
    state = engine.sdict_begin(0, dev)
    sums = torch.full((_ffi.SDICT_SUMS,), 7.0, dtype=torch.float64, device=dev)
    ws = engine.sdict_workspace(1, 64, 64, dev)
    torch.cuda.synchronize()
    before = state.clone()
    P = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.sl_sdict_workspace_bytes(-1, 64, 64) == 0 and lib.sl_sdict_workspace_bytes(1, 0, 64) == 0
    assert lib.sl_sdict_workspace_bytes(0, 64, 64) > 0
    assert lib.sl_sdict_begin(C.byref(p), 13, P(state), s) == BAD
    assert lib.sl_sdict_begin(C.byref(p), -1, P(state), s) == BAD
    assert lib.sl_sdict_begin(C.byref(p), 0, null, s) == BAD
    assert lib.sl_sdict_begin(C.byref(bad_size), 0, P(state), s) == BAD
    sw = lambda rgb_, n, h, w, par, slog, st_, ws_, wsb, out: lib.sl_sdict_sweep(rgb_, n, h, w, par, slog, st_, ws_, wsb, out, s)
    assert sw(null, 1, 64, 64, C.byref(p), 0, P(state), P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), -1, 64, 64, C.byref(p), 0, P(state), P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), 1, 0, 64, C.byref(p), 0, P(state), P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), 1, 64, 64, C.byref(p), 13, P(state), P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), 1, 64, 64, C.byref(p), 0, null, P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), 1, 64, 64, C.byref(p), 0, P(state), P(ws), ws.numel(), null) == BAD
    assert sw(P(rgb), 1, 64, 64, C.byref(bad_size), 0, P(state), P(ws), ws.numel(), P(sums)) == BAD
    assert sw(P(rgb), 1, 64, 64, C.byref(p), 0, P(state), P(ws), 8, P(sums)) == WS                # workspace too small
    assert sw(P(rgb), 1, 64, 64, C.byref(p), 0, P(state), null, ws.numel(), P(sums)) == WS         # workspace missing
    assert lib.sl_sdict_step(null, P(sums), C.byref(p), s) == BAD
    assert lib.sl_sdict_step(P(state), null, C.byref(p), s) == BAD
    assert lib.sl_sdict_step(P(state), P(sums), C.byref(bad_size), s) == BAD
    torch.cuda.synchronize()
    assert torch.equal(sums, torch.full_like(sums, 7.0))                                        # nothing was launched
    assert torch.equal(state.view(torch.int64), before.view(torch.int64))                       # (bitwise: the state holds NaN)
    # n == 0: legal, writes zero sums and a pixel count of 0
    empty = torch.empty((0, 64, 64, 3), dtype=torch.uint8, device=dev)
    ws0 = engine.sdict_workspace(0, 64, 64, dev)
    got = engine.sdict_sweep(empty, 0, state, ws0).cpu().numpy()
    assert (got == 0).all()


def _two_rank_worker(rank, world, shards):
    """one of two processes that SHARE the GPU: its contiguous shard of the slide through the product's Vahadane dictionary rounds,
    with gloo carrying the all-reduces of device tensors between the steps"""
    from stainlib_amd.distributed import PooledVahadaneStatistics
    dev = torch.device("cuda", 0)
    tiles = [so.synth_tile(256, 256, 120 + s) for s in range(sum(shards))]
    lo = sum(shards[:rank])
    mine = torch.from_numpy(np.stack(tiles)[lo:lo + shards[rank]].copy()).to(dev)
    st = PooledVahadaneStatistics()
    M, mc = st(mine)
    return rank, M, mc, st.last_rounds


# (the case ids are the ones these cases have always had: their numbers were rendezvous ports once, and name nothing now)
@pytest.mark.parametrize("shards", [(2, 2), (3, 2), (5, 0)], ids=["shards0-29641", "shards1-29642", "shards2-29643"])
def test_two_ranks_sharing_the_gpu_learn_the_slide_dictionary_over_gloo(shards):
    res = run_ranks(_two_rank_worker, 2, shards, timeout=600)
    tiles = [so.synth_tile(256, 256, 120 + s) for s in range(sum(shards))]
    M1, mc1, _ = _pooled(to_dev(tiles))
    for rank, M, mc, rounds in res:
        assert np.array_equal(M, res[0][1]) and np.array_equal(mc, res[0][2]) and rounds == res[0][3]    # the ranks agree to the bit
        np.testing.assert_allclose(M, M1, rtol=0, atol=1e-7)
        np.testing.assert_allclose(mc, mc1, rtol=2e-6)

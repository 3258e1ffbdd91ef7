"""-m gpu: the pooled slide chains on shards past 2^31 / 2^32 bytes and, once, past 2^32 PIXELS (tests/big_batch.py).

A shard of R repeats of a K-tile block is the block's pixel population with every pixel taken R times, so its reference statistics
follow exactly from the block (tests/standin_math.py: replicated_percentile, replicated_macenko): mean and covariance unchanged,
integer sums and counts times R, order statistics at the replicated position.  All with group=False (one process), every comparison of
the shard with itself on the device; the bars are the ones the pooled tests already state (test_gpu_pool2.py, test_gpu_pool_vahadane.py,
test_gpu_pool_reinhard.py) -- nobody had measured them at 1.4 Gpixel: the errors are printed."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.big_batch import K, SHAPES, assert_periodic, base_tiles, bits, guarded, need_memory, periodic_batch, release
from tests.gpu_util import u8_parity
from tests.standin_math import replicated_macenko, replicated_percentile_hist

pytestmark = pytest.mark.gpu
_C = {}


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _C.clear()
    release()


def _target_tile():
    return so.synth_tile(128, 128, 1001, so.M_TRUE_TGT)


def _macenko_block():
    """(block (K, 512, 512, 3) numpy, its device copy): the K tiles of the per-tile tests -- the all-white one adds background pixels"""
    if "mb" not in _C:
        b = base_tiles(512, 512)
        _C["mb"] = (b, torch.from_numpy(b).cuda())
    return _C["mb"]


def _macenko_ref(R):
    key = ("mref", R)
    if key not in _C:
        _C[key] = replicated_macenko(list(_macenko_block()[0]), R)
    return _C[key]


def _report(label, got, ref):
    eM, eC = float(np.abs(got[0] - ref[0]).max()), float(np.abs(got[1] / ref[1] - 1).max())
    print(f"{label}: max |M - M_ref| = {eM:.2e} (bar 5e-7), max |maxC / maxC_ref - 1| = {eC:.2e} (bar 5e-7)")
    return eM, eC


def test_pooled_macenko_both_chains_and_the_bytes_on_5464_tiles():
    """One-sweep and three-sweep chain on the 5464-tile shard (1.43 Gpixel, 4.3 GB): against replicated_macenko under the fixed-slide
    bars of tests/test_gpu_pool2.py, against each other under its 1e-13 bars; the bytes of SlideNormalizer(mode="pooled")."""
    from stainlib_amd.distributed import PooledSlideStatistics, SlideNormalizer
    h, w, n = SHAPES["aligned"]
    B = n * h * w * 3
    need_memory(3 * B)
    block, base = _macenko_block()
    dev = periodic_batch(base, n)
    st = PooledSlideStatistics(group=False)
    new = st.finish(st.enqueue_merged(dev))
    path, miss, why = list(st.last_path), st.last_miss, st.last_why
    print(f"one-sweep chain: path {path} miss {miss} why {why}")
    assert new is not None, f"the one-sweep chain did not settle this shard (miss {miss}, why {why})"
    # the three-sweep chain as tests/test_gpu_pool2.py runs it: device-driven, the host-driven radix rounds behind it where one of its
    # 65536-key windows misses its rank -- the numbers do not depend on the route, which is printed
    # (On THIS content both windows missed when this was written (miss 3), presumably for this reason: the window sits on an estimate from a pixel sample, and a sample of a shard of
    # K repeated tiles is worth no more than the block's 0.8 M distinct tissue pixels, however many it draws -- its rank error is some
    # 1e5 of the 1e9 ranks, the size of a window.  So the route cannot be pinned to "window" here; what is pinned is that the chain
    # says which route it took, that a route other than the window's comes with a reported miss, and that the numbers are the same.)
    old = st(dev, merged=False)
    print(f"three-sweep chain: path {st.last_path} miss {st.last_miss}")
    assert len(st.last_path) == 2 and set(st.last_path) <= {"window", "radix"}
    assert (st.last_path == ["window", "window"]) == (st.last_miss == 0)
    ref = _macenko_ref(n // K)
    _report("5464 tiles, one-sweep chain  ", new, ref)
    _report("5464 tiles, three-sweep chain", old, ref)
    np.testing.assert_allclose(new[0], old[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(new[1], old[1], rtol=1e-13)
    for got in (new, old):
        np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=5e-7)
        np.testing.assert_allclose(got[1], ref[1], rtol=5e-7)
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(_target_tile())
    g = guarded(B, torch.uint8, margin=4096)
    sn = SlideNormalizer(nz, group=False, mode="pooled")
    out, M_s, mc_s, status = sn.transform_shard(dev, out=g.body.view(n, h, w, 3))
    g.check("pooled macenko")
    assert_periodic(out, label="pooled macenko output")
    assert not bool(status.any())
    np.testing.assert_allclose(M_s.cpu().numpy(), ref[0], rtol=0, atol=5e-7)
    np.testing.assert_allclose(mc_s.cpu().numpy(), ref[1], rtol=5e-7)
    assert sn.last_path == ["merged", "merged"] and sn.last_miss == 0      # the one-sweep chain settled it: no fallback behind transform_shard
    Mt, mct = np.asarray(nz.stain_matrix_target), np.asarray(nz.maxC_target).reshape(1, 2)
    got = out[:K].cpu().numpy()
    for i, I in enumerate(block):                          # the oracle's recipe (normalizer.py:46-50) under the slide's reference statistics
        pre = 255 * np.exp(-1 * np.dot(so.get_concentrations(I, ref[0]) * (mct / ref[1].reshape(1, 2)), Mt))
        u8_parity(got[i], so.truncate_u8(pre).reshape(I.shape), label=f"pooled macenko tile {i}", src=I, prequant=pre.reshape(I.shape))
    del out, g, dev
    release()


def test_pooled_macenko_one_sweep_chain_past_2_pow_32_pixels():
    """16 388 tiles of 512 x 512: 4 296 015 872 pixels (12.9 GB) -- the one case where a pixel index, not a byte offset, can overflow."""
    from stainlib_amd.distributed import PooledSlideStatistics
    n, h, w = 16388, 512, 512
    assert n * h * w > 1 << 32 and n % K == 0
    need_memory(n * h * w * 3 + (8 << 30))
    _, base = _macenko_block()
    dev = periodic_batch(base, n)
    st = PooledSlideStatistics(group=False)
    new = st.finish(st.enqueue_merged(dev))
    print(f"one-sweep chain: path {st.last_path} miss {st.last_miss} why {st.last_why}")
    assert new is not None, (st.last_miss, st.last_why)
    ref = _macenko_ref(n // K)
    _report("16388 tiles, one-sweep chain", new, ref)
    np.testing.assert_allclose(new[0], ref[0], rtol=0, atol=5e-7)
    np.testing.assert_allclose(new[1], ref[1], rtol=5e-7)
    del dev
    release()


def test_pooled_vahadane_on_5464_tiles():
    """Against the K-block's own pooled result under the bars of tests/test_gpu_pool_vahadane.py (a repeated block gives the block's
    dictionary: 2e-7; maxC 2e-6) -- not bit identity: the dictionary sees the sample, whose density follows the pixel count."""
    from stainlib_amd.distributed import PooledVahadaneStatistics, SlideNormalizer
    h, w, n = SHAPES["aligned"]
    B = n * h * w * 3
    need_memory(3 * B)
    _, base = _macenko_block()
    M4, mc4 = PooledVahadaneStatistics(group=False)(base)
    dev = periodic_batch(base, n)
    nz = stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(256, 256, 1001, so.M_TRUE_TGT))
    g = guarded(B, torch.uint8, margin=4096)
    sn = SlideNormalizer(nz, group=False, mode="pooled")
    out, M_s, mc_s, status = sn.transform_shard(dev, out=g.body.view(n, h, w, 3))
    g.check("pooled vahadane")
    M_s, mc_s = M_s.cpu().numpy(), mc_s.cpu().numpy()
    print(f"pooled vahadane 5464 tiles: rounds {sn.last_rounds} sweeps {sn.last_sweeps} |dM| vs the block {np.abs(M_s - M4).max():.2e} "
          f"maxC rel {np.abs(mc_s / mc4 - 1).max():.2e}")
    np.testing.assert_allclose(M_s, M4, rtol=0, atol=2e-7)
    np.testing.assert_allclose(mc_s, mc4, rtol=2e-6)
    assert_periodic(out, label="pooled vahadane output")
    assert not bool(status.any())                         # (a pooled shard has ONE status: the all-white tiles are normalised like the rest)
    del out, g, dev
    release()


# ---- pooled Reinhard / luminosity ------------------------------------------------------------------------------------------------------------
def _dark_block(h, w):
    """K darkened tiles (class b of tests/test_gpu_pool_reinhard.py: tile i times 0.55 + 0.05 i): the slide's p90 is below 255"""
    key = ("dark", h, w)
    if key not in _C:
        b = np.stack([(so.synth_tile(h, w, 900 + i).astype(np.float64) * (0.55 + 0.05 * i)).astype(np.uint8) for i in range(K)])
        _C[key] = (b, torch.from_numpy(b).cuda())
    return _C[key]


def _reinhard_pair():
    ref = so.ReinhardStainNormalizer()
    ref.fit(_target_tile())
    return ref, stainlib_amd.ReinhardStainNormalizer(ref.target_means, ref.target_stds)


@pytest.mark.parametrize("name", ["aligned", "odd"])
def test_pooled_reinhard_and_luminosity(name):
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    h, w, n = SHAPES[name]
    B, R = n * h * w * 3, n // K
    need_memory(3 * B)
    block, base = _dark_block(h, w)
    tall = np.concatenate(list(block), axis=0)
    p90 = float(np.percentile(tall, 90))
    hist = np.bincount(tall.ravel(), minlength=256)
    assert p90 < 255 and replicated_percentile_hist(hist, R, 90) == p90          # (checked on the CPU: the replicated value is the block's)
    means, stds = so.get_mean_std(so.standardize_brightness(tall))
    ref, nrm = _reinhard_pair()
    dev = periodic_batch(base, n)
    for kw in ({}, dict(mask_background=True)):
        want = ref.transform(tall, **kw).reshape(K, h, w, 3)
        g = guarded(B, torch.uint8, margin=4096)
        sn = SlideNormalizer(nrm, group=False, mode="pooled")
        out, m, s, status = sn.transform_shard(dev, out=g.body.view(n, h, w, 3), **kw)
        g.check(f"pooled reinhard {kw}")
        assert_periodic(out, label=f"pooled reinhard {name} {kw}")
        assert np.array_equal(out[:K].cpu().numpy(), want), (name, kw)
        assert sn.last_p90 == p90 and not bool(status.any())
        assert sn.last_pixels == R * tall.shape[0] * tall.shape[1]
        assert sn.last_tissue == R * int(so.tissue_mask(so.standardize_brightness(tall)).sum())
        np.testing.assert_allclose(m.cpu().numpy(), np.ravel(means), rtol=1e-13)
        np.testing.assert_allclose(s.cpu().numpy(), np.ravel(stds), rtol=1e-12)
        del out, g
        release()
    L = so.lab_l8(tall)
    p_want = replicated_percentile_hist(np.bincount(L.ravel(), minlength=256), R, 95)
    assert p_want == float(np.percentile(L.astype(float), 95))
    g = guarded(B, torch.uint8, margin=4096)
    out, p = slide_luminosity_standardize(dev, group=False, out=g.body.view(n, h, w, 3))
    g.check("pooled luminosity")
    assert_periodic(out, label=f"pooled luminosity {name}")
    assert p == p_want
    assert np.array_equal(out[:K].cpu().numpy(), so.luminosity_standardize(tall).reshape(K, h, w, 3))
    del out, g, dev
    release()


def test_pooled_reinhard_slab_view_full_tile_float32():
    """the slab view once with float32 full-tile output (17 GB): the bits of the converter on the shard call's uint8 image"""
    from stainlib_amd import engine
    from stainlib_amd.distributed import SlideNormalizer
    from tests.test_gpu_jitter import MEAN, STD
    h, w, n = SHAPES["aligned"]
    B = n * h * w * 3
    need_memory(9 * B + B // 8)                           # the shard, two float32 tensors of it, the mask of one eighth's comparison
    _, base = _dark_block(h, w)
    _, nrm = _reinhard_pair()
    fmt = stainlib_amd.TensorFormat(dtype=torch.float32, channels_last=False, mean=MEAN, std=STD)
    dev = periodic_batch(base, n)
    sn = SlideNormalizer(nrm, group=False, mode="pooled")
    u8 = sn.transform_shard(dev, mask_background=True)[0]
    want = engine.to_tensor(u8, fmt)
    del u8
    release()
    g = guarded(B, torch.float32, margin=4096)
    view = stainlib_amd.TileView(None, flip=False, rot90=False)
    res = sn.transform_shard(dev, out=g.image(n, h, w, fmt), mask_background=True, tensor_format=fmt, view=view,
                             windows=torch.zeros((n, 3), dtype=torch.int32, device="cuda"))
    g.check("slab view")
    assert res[0].numel() > 1 << 32
    step = (n + 7) // 8
    for i0 in range(0, n, step):                          # (in eighths: the whole test stays under 40 GB)
        assert torch.equal(bits(res[0][i0:i0 + step]), bits(want[i0:i0 + step])), f"slab view: tiles {i0}..{i0 + step - 1}"
    del res, want, g, dev
    release()

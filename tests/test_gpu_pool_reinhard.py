"""GPU: the pooled slide-level Reinhard / luminosity chain (sl_slab_*, csrc/slide_lab.hip; SlideNormalizer with a
ReinhardStainNormalizer, slide_luminosity_standardize) against the oracle on the vertical concatenation of the slide's tiles.

The statistics are sums of integers, so the bar is equality: every output byte and p90 equal the oracle's; the means and standard
deviations agree to the rounding of two different summation orders (rtol 1e-13 / 1e-12, the per-tile bars of tests/test_gpu_lab.py).
The seeds are the first ones tried; the CPU gloo test runs the same class-b recipe and holds the equality there."""
import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

MASKS = (("plain", {}), ("mask", dict(mask_background=True)), ("mask06", dict(mask_background=True, luminosity_threshold=0.6)))


def _dark(tiles, lo=0.55, step=0.05):
    return [(t.astype(np.float64) * (lo + step * i)).astype(np.uint8) for i, t in enumerate(tiles)]


def _slide(cls):
    if cls == "a":          # eight 128^2 tiles: four synthetic, four structured
        return [so.synth_tile(128, 128, 40 + s) for s in range(4)] + [so.structured_tile(k, 128, 128, 4) for k in ("blobs", "palette12", "white_bg", "quantized")]
    if cls == "b":          # five ragged tiles, tile i times 0.55 + 0.05 i: the slide's p90 is below 255 and differs from every tile's
        return _dark([so.synth_tile(61, 67, 900 + i) for i in range(5)])
    if cls == "c":          # 1024^2 tiles (the middle one darkened: p90 of the slide below 255 here too)
        t = [so.synth_tile(1024, 1024, 70 + s) for s in range(3)]
        return [t[0], _dark([t[1]], 0.7)[0], t[2]]
    if cls == "white":
        return [np.full((61, 67, 3), 250, np.uint8) for _ in range(5)]
    raise ValueError(cls)


_REF = {}


def _target():
    if "ref" not in _REF:
        ref = so.ReinhardStainNormalizer()
        ref.fit(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT))
        _REF["ref"] = ref
    return _REF["ref"]


def _normalizer():
    import stainlib_amd
    ref = _target()
    return stainlib_amd.ReinhardStainNormalizer(ref.target_means, ref.target_stds)


def _dev(tiles):
    return torch.from_numpy(np.ascontiguousarray(np.stack(tiles))).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy().tobytes()


@pytest.mark.parametrize("cls", ["a", "b", "c"])
def test_pooled_reinhard_equals_the_oracle_on_the_concatenation(cls):
    from stainlib_amd.distributed import SlideNormalizer
    tiles = _slide(cls)
    tall = np.concatenate(tiles, axis=0)
    ref, dev = _target(), _dev(tiles)
    p90 = float(np.percentile(tall, 90))
    means, stds = so.get_mean_std(so.standardize_brightness(tall))
    if cls != "a":
        assert p90 < 255 and all(float(np.percentile(t, 90)) != p90 for t in tiles)      # the brightness step is not the identity, nor any tile's
    for name, kw in MASKS:
        want = ref.transform(tall, **kw)
        sn = SlideNormalizer(_normalizer(), group=False, mode="pooled")
        out, m, s, status = sn.transform_shard(dev, **kw)
        got = out.cpu().numpy().reshape(want.shape)
        diff = int((got != want).sum())
        print(f"class {cls} {name}: {diff} of {want.size} bytes differ; p90 {sn.last_p90} (oracle {p90}); means {m.cpu().numpy()} stds {s.cpu().numpy()}")
        assert np.array_equal(got, want), (cls, name, diff)
        assert sn.last_p90 == p90
        assert m.dtype == torch.float64 and m.shape == (3,) and s.shape == (3,) and status.shape == (len(tiles),) and not status.any()
        np.testing.assert_allclose(m.cpu().numpy(), np.ravel(means), rtol=1e-13)
        np.testing.assert_allclose(s.cpu().numpy(), np.ravel(stds), rtol=1e-12)
        assert sn.last_pixels == tall.shape[0] * tall.shape[1]
        assert sn.last_tissue == int(so.tissue_mask(so.standardize_brightness(tall), kw.get("luminosity_threshold", 0.8)).sum())


def test_the_slides_statistics_were_used_not_the_tiles():
    from stainlib_amd.distributed import SlideNormalizer
    tiles = _slide("b")
    dev = _dev(tiles)
    nrm = _normalizer()
    pooled = SlideNormalizer(nrm, group=False, mode="pooled").transform_shard(dev)[0]
    per_tile, st = nrm.transform_batch(dev)
    frac = float((pooled != per_tile).float().mean())
    print(f"pooled vs per-tile on class b: {frac:.3f} of the bytes differ; per-tile p90 {st[:, 0].cpu().tolist()}")
    assert frac > 0.05
    # ... while a one-tile slide IS the per-tile transform
    one = SlideNormalizer(nrm, group=False, mode="pooled").transform_shard(dev[2:3])[0]
    assert torch.equal(one, per_tile[2:3])


def _twin_tile(shape):
    if shape == "61x67":        # tile 2 of the class-b slide, in place: it starts 24522 bytes into the batch (the unaligned kernels), 4087 pixels
        return _dev(_slide("b"))[2:3]
    if shape == "64x64":        # aligned, one workgroup on both sides
        return _dev(_dark([so.synth_tile(64, 64, 64)], 0.7))
    if shape == "191x193":      # 36863 pixels = 9216 chunks, the last one ragged: two parts per tile, three spans per slide
        return _dev(_dark([so.synth_tile(191, 193, 191)], 0.7))
    raise ValueError(shape)


@pytest.mark.parametrize("shape", ["61x67", "64x64", "191x193"])
def test_a_one_tile_slide_is_the_per_tile_family_on_another_partition(shape):
    """The pooled chain and the per-tile family run the same device bodies (csrc/lab_device.hpp) over two cuts of the pixels: on a slide
    of one tile they must agree to the byte, the integer statistics exactly, the means and standard deviations at this file's bars."""
    from stainlib_amd import engine
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    dev = _twin_tile(shape)
    nrm = _normalizer()
    for name, kw in MASKS:
        per_tile, st = nrm.transform_batch(dev, **kw)
        sn = SlideNormalizer(nrm, group=False, mode="pooled")
        out, m, s, status = sn.transform_shard(dev, **kw)
        st = st[0].cpu().numpy()
        print(f"{shape} {name}: {int((out != per_tile).sum())} bytes differ; p90 {sn.last_p90} / {st[0]}; tissue {sn.last_tissue} / {st[7]}; "
              f"means {m.cpu().numpy()} / {st[1:4]}; stds {s.cpu().numpy()} / {st[4:7]}")
        assert torch.equal(out, per_tile) and not status.any()
        assert sn.last_p90 == st[0] and st[0] < 255 and sn.last_tissue == int(st[7])
        np.testing.assert_allclose(m.cpu().numpy(), st[1:4], rtol=1e-13)
        np.testing.assert_allclose(s.cpu().numpy(), st[4:7], rtol=1e-12)
    for pct in (95, 80):
        per_tile, p_tile = engine.luminosity_standardize(dev, pct)
        out, p = slide_luminosity_standardize(dev, percentile=pct, group=False)
        print(f"{shape} luminosity {pct}: {int((out != per_tile).sum())} bytes differ; p {p} / {float(p_tile[0])}")
        assert torch.equal(out, per_tile) and p == float(p_tile[0])


def _chain(dev_parts, tm, ts, mask_background=False, thr=0.8):
    """the chain with the sums of the parts added by hand (no process group): (state, [out per part])"""
    from stainlib_amd import engine
    device = dev_parts[0].device
    wss = [engine.slab_workspace(p.shape[0], p.shape[1], p.shape[2], device) for p in dev_parts]
    sa = sum(engine.slab_bytes(p, ws) for p, ws in zip(dev_parts, wss))
    state = engine.slab_begin(sa, True, device)
    sb = sum(engine.slab_lab(p, state, thr, ws) for p, ws in zip(dev_parts, wss))
    engine.slab_finish(state, sb, 0, tm, ts, mask_background=mask_background)
    return state, [engine.slab_map(p, state, 0, mask_background, thr) for p in dev_parts], sa, sb


@pytest.mark.parametrize("cls,cut", [("b", 2), ("a", 3), ("b", 0)])
def test_sums_of_two_halves_added_by_hand_give_the_state_and_bytes_of_the_whole_shard(cls, cut):
    dev = _dev(_slide(cls))
    tm, ts = _normalizer()._targets()
    for mask in (False, True):
        st1, out1, sa1, sb1 = _chain([dev], tm, ts, mask)
        st2, out2, sa2, sb2 = _chain([dev[:cut], dev[cut:]], tm, ts, mask)       # (cut 0: an empty first part; class b: the second part starts on an odd byte)
        assert torch.equal(sa1, sa2) and torch.equal(sb1, sb2)
        assert int(sa1.sum()) == dev.numel() and int(sb1[:256].sum()) == int(sb1[261]) == dev.numel() // 3
        assert _bits(st1) == _bits(st2)
        assert torch.equal(out1[0], torch.cat(out2, dim=0))


def test_sum_calls_on_an_empty_shard_write_zeros():
    from stainlib_amd import _ffi, engine
    dev = _dev(_slide("b"))
    empty = dev[:0]
    ws = engine.slab_workspace(0, 61, 67, dev.device)
    sa = torch.full((_ffi.SLAB_SUMS_A,), 7, dtype=torch.int64, device=dev.device)
    assert engine.slab_bytes(empty, ws, sums=sa) is sa and not sa.any()
    state = engine.slab_begin(engine.slab_bytes(dev, engine.slab_workspace(5, 61, 67, dev.device)), True, dev.device)
    sb = torch.full((_ffi.SLAB_SUMS_B,), 7, dtype=torch.int64, device=dev.device)
    assert engine.slab_lab(empty, state, 0.8, ws, sums=sb) is sb and not sb.any()
    assert engine.slab_map(empty, state, 0).shape == empty.shape


def test_two_runs_and_a_side_stream_give_identical_bits():
    tiles = _slide("a")
    dev = _dev(tiles)
    tm, ts = _normalizer()._targets()
    runs = [_chain([dev], tm, ts, True) for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(_chain([dev], tm, ts, True))
    side.synchronize()
    torch.cuda.synchronize()
    for st, out, sa, sb in runs[1:]:
        assert _bits(st) == _bits(runs[0][0]) and torch.equal(out[0], runs[0][1][0])
        assert torch.equal(sa, runs[0][2]) and torch.equal(sb, runs[0][3])


def test_an_all_white_slide_with_mask_background_raises_and_leaves_the_input():
    from stainlib_amd.distributed import SlideNormalizer
    from stainlib_amd.utils.excepts import TissueMaskException
    dev = _dev(_slide("white"))
    out = torch.zeros_like(dev)
    sn = SlideNormalizer(_normalizer(), group=False, mode="pooled")
    with pytest.raises(TissueMaskException):
        sn.transform_shard(dev, out=out, mask_background=True)
    assert torch.equal(out, dev) and sn.last_tissue == 0 and sn.last_pixels == 5 * 61 * 67
    with pytest.raises(so.TissueMaskException):
        _target().transform(np.concatenate(_slide("white"), axis=0), mask_background=True)      # where the reference raises too


@pytest.mark.parametrize("cls", ["a", "b", "c"])
def test_slide_luminosity_standardize_equals_the_oracle_on_the_concatenation(cls):
    from stainlib_amd.distributed import slide_luminosity_standardize
    tiles = _slide(cls)
    tall = np.concatenate(tiles, axis=0)
    dev = _dev(tiles)
    L = so.rgb2lab_u8(tall)[..., 0].astype(float)
    for pct in (95, 80):
        want = so.luminosity_standardize(tall, pct)
        out, p = slide_luminosity_standardize(dev, percentile=pct, group=False)
        got = out.cpu().numpy().reshape(want.shape)
        print(f"class {cls} luminosity {pct}: {int((got != want).sum())} bytes differ; p {p} (oracle {np.percentile(L, pct)})")
        assert np.array_equal(got, want) and p == float(np.percentile(L, pct))
    out2 = torch.empty_like(dev)
    assert slide_luminosity_standardize(dev, percentile=80, group=False, out=out2)[0] is out2 and torch.equal(out2, out)


def _two_rank_worker(rank, world, shards):
    """one of two processes that SHARE the GPU: its contiguous shard of the class-b slide through the product's chain, gloo carrying the
    two all-reduces of device tensors"""
    from stainlib_amd.distributed import SlideNormalizer, slide_luminosity_standardize
    lo = sum(shards[:rank])
    mine = _dev(_slide("b"))[lo:lo + shards[rank]].contiguous()
    sn = SlideNormalizer(_normalizer(), mode="pooled")
    out, m, s, _ = sn.transform_shard(mine, mask_background=True)
    lum, p = slide_luminosity_standardize(mine, percentile=95)
    return rank, out.cpu().numpy(), m.cpu().numpy(), s.cpu().numpy(), sn.last_p90, lum.cpu().numpy(), p


def test_two_ranks_sharing_the_gpu_run_the_pooled_reinhard_chain_over_gloo():
    """Two processes on cuda:0 with an uneven split (3 + 2) and with a rank that holds no tile (5 + 0): both reach the oracle's bytes on
    the concatenation and report identical means, stds and p90 to the bit."""
    tall = np.concatenate(_slide("b"), axis=0)
    want = _target().transform(tall, mask_background=True)
    want_lum = so.luminosity_standardize(tall, 95)
    for shards in ((3, 2), (5, 0)):
        res = run_ranks(_two_rank_worker, 2, shards, timeout=600)
        assert np.array_equal(np.concatenate([r[1] for r in res], axis=0).reshape(want.shape), want)
        assert np.array_equal(np.concatenate([r[5] for r in res], axis=0).reshape(want_lum.shape), want_lum)
        assert res[0][2].tobytes() == res[1][2].tobytes() and res[0][3].tobytes() == res[1][3].tobytes()
        assert res[0][4] == res[1][4] == float(np.percentile(tall, 90)) and res[0][6] == res[1][6]

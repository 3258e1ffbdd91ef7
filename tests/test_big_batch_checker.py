"""No GPU: the checker of the big-batch tests (tests/big_batch.py) bites, and the replicated-population stand-ins of
tests/standin_math.py equal numpy on the population written out."""
import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests import big_batch as bb
from tests.standin_math import replicated_macenko, replicated_percentile, replicated_percentile_hist


def _periodic(n=23, tile=96, dtype=torch.uint8, out_off=0):
    """a guarded CPU buffer holding a K-periodic batch of n tiles of `tile` elements -> (Guarded, the (n, tile) body)"""
    g = bb.guarded(n * tile, dtype, out_off=out_off, device="cpu")
    base = torch.arange(bb.K * tile).reshape(bb.K, tile).remainder(251).to(dtype)
    body = g.body.view(n, tile)
    body.copy_(bb.periodic_batch(base, n))
    return g, body


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float16, torch.float64])
def test_a_clean_periodic_buffer_passes(dtype):
    g, body = _periodic(dtype=dtype, out_off=1)
    bb.assert_periodic(body, label="clean")
    bb.assert_periodic((body, None, body[:, :3]), label="clean tuple")
    g.check("clean")


def test_one_wrong_byte_in_the_last_tile_fails_the_periodicity_check():
    g, body = _periodic()
    body[-1, 95] += 1
    with pytest.raises(AssertionError, match="tile 22 differs from tile 18"):
        bb.assert_periodic(body, label="planted")
    g.check("planted")                                   # (the margins are intact)


def test_one_wrong_byte_in_a_margin_fails_the_guard():
    for where in (0, -1):
        g, body = _periodic(out_off=3)
        g.buf[where] = bb.SENTINEL + 1
        bb.assert_periodic(body, label="margin")
        with pytest.raises(AssertionError, match="written outside the output"):
            g.check("margin")
    g, _ = _periodic()
    g.buf[g.start - 1] = 0                               # the element right in front of the body
    with pytest.raises(AssertionError, match="written outside"):
        g.check("margin")


def test_nan_and_negative_zero_count_as_bits():
    g, body = _periodic(dtype=torch.float64)
    body[1::bb.K, 5] = float("nan")                      # NaN in every twin: periodic
    bb.assert_periodic(body, label="nan")
    body[bb.K + 2, 7] = -0.0 if float(body[2, 7]) == 0.0 else -float(body[2, 7])
    with pytest.raises(AssertionError, match="differs from tile"):
        bb.assert_periodic(body, label="sign")


@pytest.mark.parametrize("k", [8, 10])
def test_a_block_written_at_its_offset_modulo_2_to_the_k_fails(k):
    """what a 32-bit address does, in small: the bytes meant for offset `off` >= 2^k land at off mod 2^k.  Neither 2^k nor the block's
    start is a whole number of tiles (or of K tiles) into the batch, as in SHAPES."""
    tile, n = 96, 23
    g, body = _periodic(n, tile)
    flat = g.body
    off, length = (1 << k) + 5 * tile + 17, 40
    assert off + length <= flat.numel() and (off % (1 << k)) % (bb.K * tile) != off % (bb.K * tile)
    block = flat[off:off + length].clone()
    flat[off:off + length] = bb.SENTINEL                  # never written where it belongs
    flat[off % (1 << k):off % (1 << k) + length] = block  # written where the wrapped address points
    with pytest.raises(AssertionError, match="differs from tile"):
        bb.assert_periodic(body, label="wrapped")
    # the wrapped copy alone (the right place written too) is caught as well: it lands mid-tile in a tile of another class
    g, body = _periodic(n, tile)
    g.body[off % (1 << k):off % (1 << k) + length] = g.body[off:off + length].clone()
    with pytest.raises(AssertionError, match="differs from tile"):
        bb.assert_periodic(body, label="wrapped copy")


def test_the_shapes_cross_both_lines_mid_tile():
    for name, (h, w, n) in bb.SHAPES.items():
        nbytes = 3 * h * w
        for line in (1 << 31, 1 << 32):
            assert line < n * nbytes and line % nbytes != 0 and line % (bb.K * nbytes) != 0
            assert n - line // nbytes > 1                 # at least one whole tile behind the line
        assert n * nbytes * 4 > 1 << 34 and n * h * w * 3 > 1 << 32       # float32 bytes, elements of a tensor output
    assert bb.SHAPES["odd"][0] * bb.SHAPES["odd"][1] * 3 % 2 == 1
    win = bb.period8_windows(20, 512, 512, 64, 64)
    assert sorted(win[:8, 2].tolist()) == list(range(8)) and np.array_equal(win[8:16], win[:8])
    assert (win[:, 0] + 64 <= 512).all() and (win[:, 1] + 64 <= 512).all() and (win[:8, 0] == 448).any() and (win[:8, 1] == 448).any()


# ---- the replicated-population stand-ins --------------------------------------------------------------------------------------------------
def test_replicated_percentile_is_numpys_on_the_repeated_array():
    rng = np.random.RandomState(7)
    worst = 0.0
    for case in range(300):
        m, R = int(rng.randint(1, 200)), int(rng.randint(1, 9))
        q = float(rng.choice([0.0, 1.0, 5.0, 50.0, 90.0, 95.0, 99.0, 100.0, rng.uniform(0, 100)]))
        x = rng.normal(size=m) if case % 3 else rng.randint(0, 6, size=m).astype(np.float64)       # ties too
        want = float(np.percentile(np.repeat(x, R), q))
        got = replicated_percentile(x, R, q)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12, (case, m, R, q, got, want)
        b = rng.randint(0, 256, size=m)
        want_b = float(np.percentile(np.repeat(b, R), q))
        assert abs(replicated_percentile_hist(np.bincount(b, minlength=256), R, q) - want_b) <= 1e-12, (case, m, R, q)
    print(f"replicated_percentile: worst |error| over 300 cases {worst:.1e}")


def test_replicated_macenko_is_the_oracle_on_the_stacked_block():
    R = 3
    tiles = [so.synth_tile(64, 64, 11), so.structured_tile("white_bg", 64, 64, 5), (so.synth_tile(64, 64, 13) * 0.85).astype(np.uint8)]
    tall = np.concatenate(tiles * R, axis=0)
    M_o = so.macenko_stain_matrix(tall)
    mc_o = np.percentile(so.get_concentrations(tall, M_o), 99, axis=0)
    info = {}
    M, mc = replicated_macenko(tiles, R, details=info)
    assert info["n_pixels"] == tall.shape[0] * tall.shape[1] and info["n_tissue"] == int(so.tissue_mask(tall).sum())
    np.testing.assert_allclose(M, M_o, rtol=0, atol=1e-12)
    np.testing.assert_allclose(mc, mc_o, rtol=1e-11)
    # and it is NOT the block's own statistic where the replicated rank interpolates elsewhere
    assert replicated_percentile(np.arange(10.0), 3, 95) == float(np.percentile(np.repeat(np.arange(10.0), 3), 95)) == 9.0
    assert float(np.percentile(np.arange(10.0), 95)) < 8.6

"""-m gpu: the serial steps of the fused Macenko kernel's two-sweep route -- phase 0 (the cluster sample read back in batches instead
of held in registers), the verification glue, finish 2 (whole-tile keys made only where the exact fallback runs, and that out of line).
None of it may change a result: every SlParams.two_sweep mode gives the same bytes, statistics and status as every other, and as the
one-launch-per-phase schedule, on shapes that take each path of those steps."""
import os

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests.gpu_util import oracle_fit_tile, to_dev, u8_parity

pytestmark = pytest.mark.gpu

M_ATOL = 5e-7
MAXC_RTOL = 5e-7
DIRECT, OFF = 1, 0
MODES = (0, 1, 2, 3, 4)            # automatic, off (three sweeps), forced, forced with a failing plane check, forced with a tilted sample plane


def _run(dev, Mt, mct, **kw):
    from stainlib_amd import engine
    n = dev.shape[0]
    p = engine.make_params(**kw)
    fb = engine.attach_fallbacks(p, n, device="cuda")
    ts = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    p.twosweep_out = ts.data_ptr()
    out, M, mc, st = engine.macenko_transform(dev, Mt, mct, params=p)
    torch.cuda.synchronize()
    return dict(out=out, M=M, mc=mc, st=st, fb=fb.cpu().numpy(), ts=ts.cpu().numpy())


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b, label):
    """byte identity: the float64 statistics are compared as their bit patterns (a NaN equals the same NaN)"""
    for k in ("out", "st", "M", "mc"):
        x, y = _bits(a[k]), _bits(b[k])
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
            if k in ("M", "mc"):
                d = (a[k] - b[k]).abs().nan_to_num(nan=0.0).max().item()
                print(f"{label}: {k} differs on tiles {bad[:8]}, max |delta| {d:.3e}")
            raise AssertionError(f"{label}: {k} differs on tiles {bad[:8]}")


def _kinds(h, w, n):
    """i.i.d. tiles with a white-background, a quantised, a 12-colour (ties: the exact fallback of the order statistics) and an empty tile"""
    tiles = [so.synth_tile(h, w, 700 + s) for s in range(n)]
    tiles[1] = so.structured_tile("white_bg", h, w, 5)
    tiles[2] = so.structured_tile("quantized", h, w, 6)
    tiles[3] = so.structured_tile("palette12", h, w, 8)
    if n > 4:
        tiles[4] = np.full((h, w, 3), 255, np.uint8)
        tiles[5] = so.structured_tile("blobs", h, w, 7)
    return tiles


def _many(h, w, n):
    base = _kinds(h, w, 8)
    dev = to_dev(base)
    return dev[torch.arange(n, device="cuda") % 8].contiguous()


_TARGET = []


def _target():
    if not _TARGET:
        _TARGET.append(oracle_fit_tile(so.synth_tile(128, 128, 1001, so.M_TRUE_TGT)))
    return _TARGET[0]


# 128x128: the smallest size that tries the route; 96x128: below it, three sweeps whatever is asked; 503x527: unaligned, streaming, a
# ragged tail; 1024^2: the headline's size; 600 tiles of 64x64: more tiles than resident workgroups; and the same count at 128x128, where
# a workgroup runs phase 0 again on its second tile, after finish 2 has rebuilt the row table.
CASES = [(8, 128, 128), (8, 96, 128), (4, 503, 527), (4, 1024, 1024), (600, 64, 64), (600, 128, 128)]


@pytest.mark.parametrize("n,h,w", CASES, ids=[f"{n}x{h}x{w}" for n, h, w in CASES])
def test_every_mode_and_the_per_phase_schedule_give_the_same_bytes(n, h, w):
    dev = _many(h, w, n) if n > 8 else to_dev(_kinds(h, w, n))
    Mt, mct = _target()
    runs = {mode: _run(dev, Mt, mct, schedule=2, two_sweep=mode) for mode in MODES}
    for mode in MODES:
        r = runs[mode]
        codes, counts = np.unique(r["ts"], return_counts=True)
        print(f"{n} x {h}x{w} two_sweep={mode}: attempts {dict(zip(codes.tolist(), counts.tolist()))} fallbacks {int(r['fb'].sum())} "
              f"status {np.unique(r['st'].cpu().numpy()).tolist()}")
    tries = h * w >= (1 << 14)
    assert (runs[1]["ts"] == OFF).all()
    if tries:
        assert (runs[2]["ts"][0::8] == DIRECT).all(), runs[2]["ts"][:8]          # the i.i.d. tiles take the direct route when it is forced
        assert (runs[3]["ts"][0::8] != DIRECT).all() and (runs[4]["ts"][0::8] != DIRECT).all()     # ... and leave it when a check fails
    else:
        for mode in MODES:
            assert (runs[mode]["ts"] == OFF).all(), (mode, runs[mode]["ts"][:8])
    assert int(runs[1]["st"][0]) == 0
    for mode in (0, 2, 3, 4):
        _same(runs[1], runs[mode], f"{n} x {h}x{w}: two_sweep=1 against two_sweep={mode}")
    phased = _run(dev, Mt, mct, schedule=1)
    for mode in MODES:
        _same(phased, runs[mode], f"{n} x {h}x{w}: one launch per phase against the fused kernel, two_sweep={mode}")


def test_the_exact_fallback_of_the_order_statistics_gives_the_same_bytes_in_every_mode():
    """A 12-colour tile puts every order statistic inside a run of ties longer than the member lists: finish 2 takes its out-of-line
    whole-tile selection (fallbacks > 0), in every mode and in the per-phase schedule, with the same results."""
    tiles = [so.synth_tile(512, 512, 3), so.structured_tile("palette12", 512, 512, 4), so.structured_tile("quantized", 512, 512, 4)]
    dev = to_dev(tiles)
    Mt, mct = _target()
    ref = _run(dev, Mt, mct, schedule=1)
    print("one launch per phase: fallbacks", ref["fb"].tolist())
    assert ref["fb"][0] == 0 and ref["fb"][1] > 0 and (ref["st"] == 0).all()
    for mode in MODES:
        r = _run(dev, Mt, mct, schedule=2, two_sweep=mode)
        print(f"two_sweep={mode}: attempts {r['ts'].tolist()} fallbacks {r['fb'].tolist()}")
        assert r["fb"][0] == 0 and r["fb"][1] > 0
        _same(ref, r, f"ties, two_sweep={mode}")


def test_forced_two_sweep_route_against_the_oracle():
    """The reference's golden 256^2 case with the route forced: M and maxC at the bars of test_gpu_macenko.py, the bytes at the uint8 bar."""
    from stainlib_amd import engine
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "macenko_256_s1.npz"))
    size, seed = int(g["size"]), int(g["seed"])
    I = so.synth_tile(size, size, seed)
    tgt = so.synth_tile(size, size, 1000 + seed, so.M_TRUE_TGT)
    p = engine.make_params(schedule=2, two_sweep=2)
    ts = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    p.twosweep_out = ts.data_ptr()
    Mt, mct, st = engine.macenko_fit(to_dev([tgt]), params=p)
    assert int(st[0]) == 0 and int(ts[0]) == DIRECT
    Mo, mco = oracle_fit_tile(tgt)
    np.testing.assert_allclose(Mt.cpu().numpy()[0], Mo, rtol=0, atol=M_ATOL)
    np.testing.assert_allclose(mct.cpu().numpy()[0], mco, rtol=MAXC_RTOL)
    np.testing.assert_allclose(Mt.cpu().numpy()[0], g["M_target"], rtol=0, atol=M_ATOL)
    np.testing.assert_allclose(mct.cpu().numpy()[0], g["maxC_target"].reshape(2), rtol=MAXC_RTOL)
    out, M, mc, st = engine.macenko_transform(to_dev([I]), Mt[0], mct[0], params=p)
    assert int(st[0]) == 0 and int(ts[0]) == DIRECT
    Mo, mco = oracle_fit_tile(I)
    np.testing.assert_allclose(M.cpu().numpy()[0], Mo, rtol=0, atol=M_ATOL)
    np.testing.assert_allclose(mc.cpu().numpy()[0], mco, rtol=MAXC_RTOL)
    np.testing.assert_allclose(M.cpu().numpy()[0], g["M"], rtol=0, atol=M_ATOL)
    np.testing.assert_allclose(mc.cpu().numpy()[0], g["maxC"].reshape(2), rtol=MAXC_RTOL)
    u8_parity(out.cpu().numpy()[0], g["out"], label="macenko_256_s1, two-sweep forced", src=I)

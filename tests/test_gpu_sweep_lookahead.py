"""-m gpu: the merged moments + candidates sweep (stats_twosweep.hpp: ts_sweep) on the two-trip look-ahead loop of sweep_lookahead.hpp
-- two chunk sets, a loop body of two trips, each chunk refilled two trips ahead behind its second reader, an odd full trip and the
ragged trip behind the loop.  None of it may change a result:
  * every route gives the same bytes, statistics and status as every other: SlParams.two_sweep = 1 (off), 2 (forced), 3 (forced, the
    plane check made to fail) of the fused kernel and the one-launch-per-phase schedule (schedule = 1); twosweep_out, fallbacks_out and
    resweeps_out say which route a tile took, so they are held to what the parent commit wrote for that route;
  * M and maxC are the oracle's at the bars of test_gpu_macenko.py;
  * all forced routes share the loop, so the yardstick that does not: what the PARENT commit 6072600 ("Fused apply sweep: two trips of
    loads in flight, below other phases") computed for the same inputs (tests/golden/sweep_lookahead_parent.json, written by record()
    below under STAINLIB_HIP_LIB = a build of that commit) -- the CRC32 of the output bytes, M and maxC bit for bit (float.hex()),
    status, and per route twosweep_out, fallbacks_out and resweeps_out.  A pixel that enters the ring twice, not at all or in another
    order moves a list and with it the counters even where the final bytes survive; a chunk summed in another trip moves M's last bits.
The shapes sit on the edges of the loop (a trip is 4 chunks x 512 lanes x 4 pixels = 8192 pixels, the loop body two trips):
64x64 (under one trip: the ragged instantiation alone; too small for the two-sweep route), 128x128 (exactly two trips, the smallest
tile that tries the two-sweep route), 128x192 (three trips: an odd count, the odd one runs behind the loop), 157x157 (three trips
and a ragged one, unaligned bytes, P mod 4 = 1), 129x256 (four trips and a ragged one), 181x183, 503x527 (non-temporal loads, the shape
of DESIGN 4.0 hazard 3), the real-tissue fixture (a full ring) and 256x256 with 60 % near-white pixels (a ring that stays empty for
whole trips).  Two tiles per case."""
import json
import os
import zlib

import numpy as np
import pytest

from oracle import stain_oracle as so
from tests.gpu_util import oracle_fit_tile, to_dev
from tests.test_gpu_merged_sweep_slots import M_ATOL, MAXC_RTOL, ROUTES, _hex, _ihc, _white60, run_route

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sweep_lookahead_parent.json")

CASES = {
    "iid_64x64": lambda: [so.synth_tile(64, 64, 61), so.synth_tile(64, 64, 62)],
    "iid_128x128": lambda: [so.synth_tile(128, 128, 63), so.synth_tile(128, 128, 64)],
    "iid_128x192": lambda: [so.synth_tile(128, 192, 65), so.synth_tile(128, 192, 66)],
    "iid_157x157": lambda: [so.synth_tile(157, 157, 67), so.synth_tile(157, 157, 68)],
    "iid_129x256": lambda: [so.synth_tile(129, 256, 69), so.synth_tile(129, 256, 70)],
    "iid_181x183": lambda: [so.synth_tile(181, 183, 71), so.synth_tile(181, 183, 72)],
    "iid_503x527": lambda: [so.synth_tile(503, 527, 73), so.synth_tile(503, 527, 74)],
    "tissue_ihc_512": lambda: [np.ascontiguousarray(_ihc()), np.ascontiguousarray(_ihc()[:, ::-1])],
    "white60_256x256": lambda: [_white60(256, 256, 75), _white60(256, 256, 76)],
}
# tiles too small for the two-sweep route: it is declined whatever two_sweep asks for (the three-sweep route alone runs)
THREE_SWEEP_ONLY = {"iid_64x64"}


def record(name):
    """the golden entry of one case from the library in use"""
    dev = to_dev(CASES[name]())
    runs = {r: run_route(dev, **kw) for r, kw in ROUTES.items()}
    a = runs["off"]
    return dict(crc=zlib.crc32(a["out"].tobytes()), M=_hex(a["M"]), mc=_hex(a["mc"]), st=a["st"],
                ts={r: runs[r]["ts"] for r in ROUTES}, fb={r: runs[r]["fb"] for r in ROUTES}, rs={r: runs[r]["rs"] for r in ROUTES})


def _parent():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_every_route_gives_the_parents_bits(name):
    tiles = CASES[name]()
    dev = to_dev(tiles)
    runs = {r: run_route(dev, **kw) for r, kw in ROUTES.items()}
    for r in ROUTES:
        x = runs[r]
        print(f"{name} {r}: crc {zlib.crc32(x['out'].tobytes()):#010x} status {x['st']} twosweep {x['ts']} fallbacks {x['fb']} resweeps {x['rs']}")
    # (i) the routes agree byte for byte (float64 statistics as their bit patterns: a NaN equals the same NaN)
    a = runs["off"]
    for r in ("forced", "forced_fail", "per_phase"):
        b = runs[r]
        assert np.array_equal(a["out"], b["out"]), f"{name}: bytes of {r} differ from the three-sweep route's"
        assert a["st"] == b["st"], f"{name}: status of {r}"
        assert np.array_equal(a["M"].view(np.int64), b["M"].view(np.int64)), f"{name}: M of {r}"
        assert np.array_equal(a["mc"].view(np.int64), b["mc"].view(np.int64)), f"{name}: maxC of {r}"
    # (ii) the oracle
    for i, t in enumerate(tiles):
        Mo, mco = oracle_fit_tile(t)
        print(f"{name} tile {i}: |M - oracle| {np.abs(a['M'][i] - Mo).max():.2e}  maxC rel {np.abs(a['mc'][i] / mco - 1).max():.2e}")
        np.testing.assert_allclose(a["M"][i], Mo, rtol=0, atol=M_ATOL)
        np.testing.assert_allclose(a["mc"][i], mco, rtol=MAXC_RTOL)
    # (iii) the parent commit
    want = _parent()[name]
    assert zlib.crc32(a["out"].tobytes()) == want["crc"], f"{name}: output bytes differ from the parent's"
    assert _hex(a["M"]) == want["M"] and _hex(a["mc"]) == want["mc"] and a["st"] == want["st"], f"{name}: statistics differ from the parent's"
    for r in ROUTES:
        for k in ("ts", "fb", "rs"):
            assert runs[r][k] == want[k][r], f"{name} {r}: {k} {runs[r][k]} against the parent's {want[k][r]}"
    # what each case is here for did happen: the merged sweep ran on both tiles (or, under one trip, could not)
    if name in THREE_SWEEP_ONLY:
        assert all(v != 1 for v in runs["forced"]["ts"]), f"{name}: the two-sweep route ran on a tile this small: {runs['forced']['ts']}"
    else:
        assert runs["forced"]["ts"] == [1, 1], f"{name}: the forced route was not taken: {runs['forced']['ts']}"
        assert runs["forced_fail"]["ts"] == [-3, -3], f"{name}: the merged sweep did not run before the plane check: {runs['forced_fail']['ts']}"

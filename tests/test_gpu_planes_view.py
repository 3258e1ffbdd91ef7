"""-m gpu: companion planes through the windows of a view (sl_view_planes, engine.view_planes, TileView.apply).

The definition under test (include/stainlib_hip.h, sl_view_planes): per tile and plane the window is resampled in the TILE's orientation
-- the centre sample ((2 i + 1) nw) // (2 no), a bit copy, or for uint8 the images' own box mean / area average -- and THEN flipped and
turned.  The yardstick is _ref below: torch slicing, explicit index tensors, flip and rot90 on the CPU, not the module's restatement.
All comparisons are on bit patterns (integer views of the element's width); there is no tolerance anywhere.

Every call writes into a buffer with sentinel elements before and after the output, which starts one element past an aligned address
in half of the cases; the margins are checked after the call.  Element values differ from position to position (per plane distinct
where the element is wide enough), and both dwords of an 8-byte element are distinct.

The batches past 2^32 bytes of both planes kernels are here too (6): sl_view_planes on uint8, sl_view_planes_affine on int64."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd.tile_view import area_resample
from tests.big_batch import SHAPES, assert_periodic, need_memory, period8_windows, periodic_batch, release
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

H, W, N = 70, 131, 8
DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.float16, torch.bfloat16, torch.int32, torch.float32, torch.int64,
          torch.float64]
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SIZES = {1: [(1, 1), (37, 65), (64, 64), (65, 63)], 2: [(1, 1), (18, 32), (33, 34)], 4: [(1, 1), (9, 17), (17, 16)]}
_calls = [0]


def _bits(t):
    """t as integers of its element width (bool: its bytes)"""
    return t.view(_INT[t.element_size()])


def _planes(dtype, shape):
    """a CPU tensor of `dtype` whose bits change from position to position: per plane distinct where the width allows, both dwords of
    an 8-byte element distinct"""
    numel = int(np.prod(shape))
    e = np.arange(numel, dtype=np.uint64)
    es = torch.empty((), dtype=dtype).element_size()
    if dtype == torch.bool:
        return torch.from_numpy((((e * 37 + (e >> 3) * 5 + (e >> 7)) >> 1) & 1).astype(np.uint8).reshape(shape)).view(torch.bool)
    if es == 1:
        v = ((e * 37 + (e >> 8) * 11 + 3) & 0xff).astype(np.uint8)
    elif es == 2:
        v = ((e * 40503 + 7) & 0xffff).astype(np.uint16).view(np.int16)
    elif es == 4:
        v = ((e * 2654435761 + 12345) & 0xffffffff).astype(np.uint32).view(np.int32)
    else:
        v = ((((e * 40503 + 0x9e3779b9) & 0xffffffff) << 32) | ((e * 2654435761 + 12345) & 0xffffffff)).view(np.int64)
    return torch.from_numpy(v.reshape(shape)).view(dtype)


def _clamp(win, h, w, oh, ow, d_mask, shrink=1, resize=None):
    """the kernels' clamp rule on int64 rows, in plain numpy: what a device window is taken as"""
    out = []
    for r in np.asarray(win, dtype=np.int64):
        d = int(r[2]) & d_mask
        nu, nv = (ow, oh) if d & 1 else (oh, ow)
        if resize is None:
            wh, ww = shrink * nu, shrink * nv
        else:
            wh = max(1, min(int(r[3]), min(16 * nu, resize[0])))
            ww = max(1, min(int(r[4]), min(16 * nv, resize[1])))
        y0, x0 = max(0, min(int(r[0]), h - wh)), max(0, min(int(r[1]), w - ww))
        out.append((y0, x0, d) + ((wh, ww) if resize is not None else ()))
    return np.array(out, dtype=np.int32)


def _ref(x, win, oh, ow, shrink=1, mode="nearest", after_flip=False):
    """The definition on CPU tensors with torch slicing, explicit index tensors, flip and rot90: x (N, H, W) or (N, C, H, W), win in
    range -- (N, 3) rows under `shrink`, or (N, 5) rows of a resizing view.  after_flip: the WRONG order (sample the reversed window),
    for the test that shows the two orders differ."""
    xb = _bits(x)
    x4 = xb[:, None] if xb.dim() == 3 else xb
    out = torch.empty(x4.shape[:2] + (oh, ow), dtype=x4.dtype)
    for t in range(x4.shape[0]):
        y0, x0, d = (int(v) for v in win[t][:3])
        k = d & 3
        nu, nv = (ow, oh) if k & 1 else (oh, ow)
        wh, ww = (int(win[t][3]), int(win[t][4])) if len(win[t]) == 5 else (shrink * nu, shrink * nv)
        Wn = x4[t, :, y0:y0 + wh, x0:x0 + ww]
        assert Wn.shape[1:] == (wh, ww)
        if mode == "area":
            R = torch.stack([torch.from_numpy(area_resample(p.numpy()[..., None], nu, nv)[..., 0]) for p in Wn])
        else:
            ky = ((2 * torch.arange(nu) + 1) * wh) // (2 * nu)
            kx = ((2 * torch.arange(nv) + 1) * ww) // (2 * nv)
            if after_flip:
                R = Wn.flip(-1)[:, ky][:, :, kx] if d & 4 else Wn[:, ky][:, :, kx]
            else:
                R = Wn[:, ky][:, :, kx]
        if d & 4 and not (after_flip and mode == "nearest"):
            R = R.flip(-1)
        out[t] = torch.rot90(R, k, dims=(-2, -1))
    return out[:, 0] if xb.dim() == 3 else out


def _run(call, x, shape, label=""):
    """call(out) on a guarded output of `shape` and x's dtype: 16 sentinel elements before and after, the output one element past an
    aligned address on every other call; returns the output's bits on the CPU"""
    _calls[0] += 1
    off = _calls[0] & 1
    numel = int(np.prod(shape))
    it = _INT[x.element_size()]
    buf = torch.full((16 + off + numel + 16,), 0x4d, dtype=it, device="cuda")
    assert buf.data_ptr() % 16 == 0
    body = buf[16 + off:16 + off + numel]
    out = body.view(x.dtype).view(shape)
    assert out.data_ptr() == buf.data_ptr() + (16 + off) * x.element_size()
    got = call(out)
    torch.cuda.synchronize()
    assert got is out
    assert bool((buf[:16 + off] == 0x4d).all()) and bool((buf[16 + off + numel:] == 0x4d).all()), f"{label}: written outside the output"
    return body.view(shape).cpu()


def _view(x_cpu, win, size, label="", **kw):
    """engine.view_planes of x (moved to the device) under host or device windows, guarded"""
    from stainlib_amd import engine
    x = x_cpu.cuda()
    shape = x.shape[:-2] + tuple(size)
    return _run(lambda o: engine.view_planes(x, win, size, out=o, **kw), x, shape, label)


def _windows(oh, ow, s=1):
    """8 windows, the eight codes, at the four corners, on the last row / column and in the middle"""
    return period8_windows(N, H, W, s * oh, s * ow)


# ---- 1. crop / flip / turn ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_crop_flip_turn_is_a_permutation_of_bits(dtype):
    for shape in ((N, H, W), (N, 3, H, W)):
        x = _planes(dtype, shape)
        for oh, ow in SIZES[1]:
            win = _windows(oh, ow)
            assert sorted(win[:, 2].tolist()) == list(range(8))
            want = _ref(x, win, oh, ow)
            for mode in (("nearest", "area") if dtype == torch.uint8 else ("nearest",)):
                got = _view(x, win, (oh, ow), f"{dtype} {shape} {oh}x{ow} {mode}", mode=mode)
                assert got.dtype == want.dtype and torch.equal(got, want), (dtype, shape, oh, ow, mode)
    if dtype == torch.int32:                                           # the output allocated by the call, device windows, a full-tile view
        from stainlib_amd import engine
        x = _planes(dtype, (N, 3, H, W))
        win = _windows(37, 65)
        got = engine.view_planes(x.cuda(), torch.from_numpy(win).cuda(), (37, 65))
        assert got.dtype == dtype and got.is_contiguous() and torch.equal(_bits(got.cpu()), _ref(x, win, 37, 65))
        w0 = np.array([(0, 0, d) for d in (0, 2, 4, 6)] * 2, dtype=np.int32)
        assert torch.equal(_view(x, w0, (H, W), d_mask=6), _ref(x, w0, H, W))


# ---- 2. shrink 2 and 4: the centre sample, in the tile's orientation ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_shrink_takes_the_centre_of_every_box(dtype):
    for shape in ((N, H, W), (N, 3, H, W)):
        x = _planes(dtype, shape)
        for s in (2, 4):
            for oh, ow in SIZES[s]:
                win = _windows(oh, ow, s)
                want = _ref(x, win, oh, ow, shrink=s)
                got = _view(x, win, (oh, ow), f"{dtype} {shape} {oh}x{ow} s={s}", shrink=s)
                assert torch.equal(got, want), (dtype, shape, oh, ow, s)


def test_the_sample_is_taken_before_the_flip():
    """nw / no even: sampling the reversed window would give other elements; the kernel must mirror the index, not the formula"""
    x = _planes(torch.int32, (N, H, W))
    for s, (oh, ow) in ((2, (18, 32)), (4, (9, 17))):
        win = _windows(oh, ow, s)
        got = _view(x, win, (oh, ow), shrink=s)
        wrong = _ref(x, win, oh, ow, shrink=s, after_flip=True)
        assert torch.equal(got, _ref(x, win, oh, ow, shrink=s))
        for t in range(N):
            d = int(win[t, 2])
            # only a flip along the window's width reverses its sampled axis: the two orders agree without one and differ with one
            assert torch.equal(got[t], wrong[t]) == (not d & 4), (s, t, d)


# ---- 3. resizing windows -------------------------------------------------------------------------------------------------------------------------
def _resize_windows(oh, ow, side):
    """8 resizing windows, the eight codes; side(nu, nv) -> (wh, ww); corners and the middle by turns"""
    win = np.empty((N, 5), dtype=np.int32)
    for t in range(N):
        nu, nv = (ow, oh) if t & 1 else (oh, ow)
        wh, ww = side(nu, nv)
        ymax, xmax = H - wh, W - ww
        y0, x0 = [(0, 0), (0, xmax), (ymax, 0), (ymax, xmax), (ymax, xmax // 2 | 1 if xmax else 0), (ymax // 2, xmax), (min(1, ymax), min(2, xmax)),
                  (max(ymax - 1, 0), max(xmax - 1, 0))][t]
        win[t] = (y0, x0, t, wh, ww)
    return win


RESIZE_CASES = {"identity": ((37, 65), lambda nu, nv: (nu, nv)), "2x": ((18, 32), lambda nu, nv: (2 * nu, 2 * nv)),
                "4x": ((9, 17), lambda nu, nv: (4 * nu, 4 * nv)), "16x": ((4, 4), lambda nu, nv: (16 * nu, 16 * nv)),
                "45x77->32x48": ((32, 48), lambda nu, nv: (45, 77)), "5x7->37x65": ((37, 65), lambda nu, nv: (5, 7)),
                "1x1": ((3, 5), lambda nu, nv: (1, 1))}


@pytest.mark.parametrize("case", list(RESIZE_CASES))
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32, torch.int64], ids=lambda d: str(d).split(".")[-1])
def test_resizing_windows_nearest(dtype, case):
    (oh, ow), side = RESIZE_CASES[case]
    win = _resize_windows(oh, ow, side)
    for shape in ((N, H, W), (N, 3, H, W)):
        x = _planes(dtype, shape)
        got = _view(x, win, (oh, ow), f"{dtype} {case}", resize=(H, W))
        assert torch.equal(got, _ref(x, win, oh, ow)), (dtype, case, shape)
        if case in ("2x", "4x"):                                       # an exact ratio is the shrink's result on the same corners and codes
            s = int(case[0])
            assert torch.equal(got, _view(x, np.ascontiguousarray(win[:, :3]), (oh, ow), shrink=s))
        if case == "identity":
            assert torch.equal(got, _view(x, np.ascontiguousarray(win[:, :3]), (oh, ow)))


# ---- 4. mode="area" on uint8 ------------------------------------------------------------------------------------------------------------------------
def test_area_mode_is_area_resample_per_plane_and_the_image_kernels_result():
    from stainlib_amd import engine
    x = _planes(torch.uint8, (N, 3, H, W))
    tiles = x.permute(0, 2, 3, 1).contiguous().cuda()                  # the same data as (N, H, W, 3) images

    def image(win, size, **kw):                                        # the existing kernels on their raw route, uint8 out, permuted back
        return engine.normalize_view(tiles, win, size, 7, **kw).permute(0, 3, 1, 2).contiguous().cpu()

    for s in (2, 4):
        for oh, ow in SIZES[s]:
            win = _windows(oh, ow, s)
            got = _view(x, win, (oh, ow), f"area s={s}", shrink=s, mode="area")
            assert torch.equal(got, _ref(x, win, oh, ow, shrink=s, mode="area")), (s, oh, ow)
            assert torch.equal(got, image(win, (oh, ow), shrink=s)), (s, oh, ow)
            assert torch.equal(_view(x[:, 1].contiguous(), win, (oh, ow), shrink=s, mode="area"), got[:, 1])
    for case, ((oh, ow), side) in RESIZE_CASES.items():
        win = _resize_windows(oh, ow, side)
        got = _view(x, win, (oh, ow), f"area {case}", resize=(H, W), mode="area")
        assert torch.equal(got, _ref(x, win, oh, ow, mode="area")), case
        assert torch.equal(got, image(win, (oh, ow), resize=(H, W))), case


# ---- 5. device windows out of range are the clamped host windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d_mask", [7, 6])
def test_device_windows_out_of_range_equal_the_clamped_host_windows(d_mask):
    from stainlib_amd import engine
    x = _planes(torch.int16, (N, 3, H, W))
    x8 = _planes(torch.uint8, (N, 3, H, W))
    wild3 = np.array([(-1, -1, 0), (10 ** 9, 10 ** 9, 1), (-2 ** 31, 2 ** 31 - 1, 2), (2 ** 31 - 1, -2 ** 31, 3), (69, 3, 4 | 8), (3, 130, 5 | 16),
                      (16, 80, 6 | 64), (-5, 100, -1)], dtype=np.int64).astype(np.int32)
    for s, (oh, ow) in ((1, (37, 65)), (2, (18, 32)), (4, (9, 16))):
        clamped = _clamp(wild3, H, W, oh, ow, d_mask, shrink=s)
        dwin = torch.from_numpy(wild3).cuda()
        got = _view(x, dwin, (oh, ow), f"wild s={s}", shrink=s, d_mask=d_mask)
        assert torch.equal(got, _ref(x, clamped, oh, ow, shrink=s)) and torch.equal(got, _view(x, clamped, (oh, ow), shrink=s, d_mask=d_mask))
        if s > 1:
            got = _view(x8, dwin, (oh, ow), shrink=s, d_mask=d_mask, mode="area")
            assert torch.equal(got, _ref(x8, clamped, oh, ow, shrink=s, mode="area"))
        with pytest.raises(ValueError, match="windows: tile "):                                       # as host windows they are refused
            engine.view_planes(x.cuda(), wild3, (oh, ow), shrink=s, d_mask=d_mask)
    wild5 = np.array([(-1, -1, 0, 40, 40), (10 ** 9, 10 ** 9, 1, 50, 60), (-2 ** 31, 2 ** 31 - 1, 2, 0, 30), (2 ** 31 - 1, -2 ** 31, 3, 30, -5),
                      (69, 3, 4, 82, 152), (3, 130, 5, 2 ** 31 - 1, 2 ** 31 - 1), (16, 80, 6, -2 ** 31, 7), (5, 100, 7 | 8, 81, 151)],
                     dtype=np.int64).astype(np.int32)
    for (oh, ow), bound in (((32, 48), (H, W)), ((32, 48), (50, 60)), ((4, 4), (H, W)), ((4, 4), (33, 37))):
        clamped = _clamp(wild5, H, W, oh, ow, d_mask, resize=bound)
        assert (clamped[:, 3] <= min(bound[0], 16 * max(oh, ow))).all() and (clamped[:, 3:] >= 1).all()
        dwin = torch.from_numpy(wild5).cuda()
        got = _view(x, dwin, (oh, ow), f"wild resize {bound}", resize=bound, d_mask=d_mask)
        assert torch.equal(got, _ref(x, clamped, oh, ow)) and torch.equal(got, _view(x, clamped, (oh, ow), resize=bound, d_mask=d_mask))
        got = _view(x8, dwin, (oh, ow), resize=bound, d_mask=d_mask, mode="area")
        assert torch.equal(got, _ref(x8, clamped, oh, ow, mode="area"))
        with pytest.raises(ValueError, match="windows: tile "):
            engine.view_planes(x.cuda(), wild5, (oh, ow), resize=bound, d_mask=d_mask)


# ---- 6. byte offsets past 2^31 and 2^32 ----------------------------------------------------------------------------------------------------------------
def test_big_batch_of_uint8_planes_past_4_gib():
    """uint8 planes with c = 3: the image tests' byte count (n x 3 x 509 x 517), 2^31 and 2^32 bytes fall mid-plane.  K = 4 distinct
    tiles under windows of period 8: tile t + 8 must be tile t bit for bit, and the first period the definition."""
    from stainlib_amd import engine
    h, w, n = SHAPES["odd"]
    nbytes = n * 3 * h * w
    assert nbytes > 1 << 32 and (1 << 31) % (h * w) != 0 and (1 << 32) % (h * w) != 0
    need_memory(nbytes + (1 << 28))
    base = _planes(torch.uint8, (4, 3, h, w))
    x = periodic_batch(base.cuda(), n)
    win = period8_windows(n, h, w, 64, 64)
    dwin = torch.from_numpy(win).cuda()
    body = _run(lambda o: engine.view_planes(x, dwin, (64, 64), out=o), x, (n, 3, 64, 64), "big batch")
    assert_periodic(body, period=8, label="view_planes big batch")
    want = _ref(base[torch.arange(8) % 4], win[:8], 64, 64)
    assert torch.equal(body[:8], want)
    del x, body
    release()


def test_big_batch_of_int64_planes_through_an_affine_view_past_4_gib():
    """sl_view_planes_affine on int64 planes (n, 509, 517) of period 8, n the smallest whose bytes pass 2^32; 2^31 and 2^32 bytes fall
    mid-plane.  The identity about the centre at full size is a bit copy of the input (output offsets pass 2^32 too); a rotated
    64 x 64 view is periodic and its first period the definition (stainlib_amd.tile_view.affine_nearest)."""
    from stainlib_amd import engine
    from stainlib_amd.tile_view import AFFINE_MAX_R, AFFINE_Q as Q, affine_nearest
    from tests.big_batch import period8_affine_windows
    h, w, _ = SHAPES["odd"]
    pb = h * w * 8
    n = (1 << 32) // pb + 1
    nbytes = n * pb
    assert nbytes > 1 << 32 >= nbytes - pb and (1 << 31) % pb != 0 and (1 << 32) % pb != 0 and n > 16
    need_memory(2 * nbytes + nbytes // 8 + (1 << 28))                             # the planes, the full-size output, one comparison's mask
    base = _planes(torch.int64, (8, h, w))
    assert len({base[t].numpy().tobytes() for t in range(8)}) == 8
    x = periodic_batch(base.cuda(), n)
    numel = n * h * w
    buf = torch.full((16 + numel + 16,), 0x4d, dtype=torch.int64, device="cuda")
    out = buf[16:16 + numel].view(n, h, w)
    ident = torch.tensor([h * Q // 2, w * Q // 2, Q, 0, 0, Q], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
    assert engine.view_planes_affine(x, ident, None, Q, fill=-1, out=out) is out
    torch.cuda.synchronize()
    assert bool((buf[:16] == 0x4d).all()) and bool((buf[16 + numel:] == 0x4d).all()), "identity: written outside the output"
    assert torch.equal(out, x), "the identity at full size is not a bit copy"
    del out, buf, ident
    release()
    fill = -(2 ** 40) - 3
    win = period8_affine_windows(n, h, w, 64, 64, "rotated")
    dwin = torch.from_numpy(win).cuda()
    body = _run(lambda o: engine.view_planes_affine(x, dwin, (64, 64), AFFINE_MAX_R, fill=fill, out=o), x, (n, 64, 64), "big affine planes")
    assert_periodic(body, period=8, label="view_planes_affine big batch")
    want = np.stack([affine_nearest(base[t].numpy(), win[t], (64, 64), fill) for t in range(8)])
    assert all((want[t] == fill).any() and (want[t] != fill).any() for t in range(4))
    assert np.array_equal(body[:8].numpy(), want)
    del x, body
    release()


# ---- 7. the public route: companions behind a batch method's view ----------------------------------------------------------------------------------
def test_apply_behind_separate_batch_and_augment_batch():
    from stainlib_amd import engine
    tiles = [so.synth_tile(64, 64, 20 + s) for s in range(6)]
    dev = to_dev(tiles)
    n = len(tiles)
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    labels = _planes(torch.int64, (n, 64, 64))
    mask = engine.tissue_mask(dev)[0]
    assert mask.shape == (n, 64, 64) and mask.dtype == torch.uint8 and 0 < int(mask.sum()) < mask.numel()
    jitter = stainlib_amd.StainJitter(0.15, 0.1)

    def loop(x, windows, oh, ow, s):
        """the per-tile torch loop a loader writes today, on the windows the image call returned"""
        out = []
        for t in range(n):
            y0, x0, d = (int(v) for v in windows[t][:3])
            nu, nv = (ow, oh) if d & 1 else (oh, ow)
            wh, ww = (int(windows[t][3]), int(windows[t][4])) if len(windows[t]) == 5 else (s * nu, s * nv)
            r = x[t, y0:y0 + wh, x0:x0 + ww]
            r = r[((2 * torch.arange(nu) + 1) * wh) // (2 * nu)][:, ((2 * torch.arange(nv) + 1) * ww) // (2 * nv)]
            out.append(torch.rot90(r.flip(1) if d & 4 else r, d & 3, (0, 1)))
        return torch.stack(out)

    np.random.seed(5)
    for v, call in ((stainlib_amd.TileView(48), lambda v: nz.separate_batch(dev, want=("h",), view=v)),
                    (stainlib_amd.TileView(16, shrink=2), lambda v: nz.separate_batch(dev, want=("h",), view=v)),
                    (stainlib_amd.TileView(32, scale=(0.08, 1)), lambda v: nz.augment_batch(dev, jitter.draw(n), view=v))):
        res = call(v)
        windows = res[4]
        oh, ow = v.out_size(64, 64)
        assert isinstance(windows, np.ndarray) and windows.shape == (n, 5 if v.resizing else 3)
        state = np.random.get_state()
        got = _run(lambda o: v.apply(labels.cuda(), windows, out=o), labels, (n, oh, ow), repr(v))
        assert torch.equal(got, loop(labels, windows, oh, ow, v.shrink)), v
        got = v.apply(mask, windows)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), loop(mask.cpu(), windows, oh, ow, v.shrink)), v
        assert torch.equal(v.apply(mask, torch.from_numpy(windows).cuda()), got)                  # the windows on the device: the same window
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # apply draws nothing

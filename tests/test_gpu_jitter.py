"""-m gpu: stain jitter in the apply pass (sl_normalize_jitter, engine.normalize_jitter, the augment_batch methods, StainJitter).

The definition under test (include/stainlib_hip.h, sl_normalize_jitter) makes the pass equal its neighbours bit for bit:
    no target            = the bytes of engine.stain_augment (golden-pinned to the reference)
    alpha = 1, beta = 0  = the bytes of engine.normalize_apply (targets without a negative entry)
    a tensor format      = TensorFormat.convert of the uint8 result
so most of this file compares against other kernels with torch.equal; the oracle comparison (4) is independent of the library.
Every call of _jit writes into a buffer with sentinel elements before and after the output, checked after the call."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from tests.gpu_util import to_dev, u8_parity

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
SENTINEL = 77                                                 # exactly representable in all four element types
# (n, h, w, byte offset of the input inside a larger buffer): P = 35 -- the unaligned path, a ragged last chunk, a ragged last half-type
# group; fewer than 12 bytes; aligned with wide stores; P = 36 864 > 32 768 -- two parts per tile; P a multiple of 4 behind an
# unaligned pointer
SHAPES = [(3, 5, 7, 0), (1, 1, 2, 0), (2, 64, 64, 0), (1, 192, 192, 0), (2, 64, 64, 1)]
M_NEG = so.normalize_rows(np.array([[0.9, -0.3, 0.3], [-0.2, 0.95, 0.25]]))               # g12 < 0 (tests/test_gpu_apply.py)
M_TGT = so.normalize_rows(so.M_TRUE_TGT)
MAXC_TGT = np.array([1.5, 1.1])
M_TGT_NEG = so.normalize_rows(np.array([[0.55, 0.80, -0.25], [0.10, 0.95, 0.20]]))        # a negative entry in row H
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_CACHE = {}


def _tiles(n, h, w):
    """n synthetic H&E tiles (CPU tensor), each from its own seed; pixel 0 of tile 0 is background white."""
    key = ("tiles", n, h, w)
    if key not in _CACHE:
        t = np.stack([so.synth_tile(h, w, 40 + 7 * i + h) for i in range(n)])
        t[0, 0, 0] = 255
        _CACHE[key] = torch.from_numpy(t)
    return _CACHE[key]


def _stats(n, regime="he"):
    """(M_src (n,2,3), maxC_src (n,2), alpha_beta (n,4)), DISTINCT per tile so that a wrong tile index cannot pass -- the per-pixel sweep
    does not care whether M fits the tile.  "he": positively correlated rows (the branch-free lasso); "neg": g12 < 0 (the general one).
    Draws as in test_configs3_tile_size_stain_augmentor_and_hed_batch: alpha in [0.8, 1.2], beta in [-0.2, 0.2]."""
    base = so.M_TRUE_SRC if regime == "he" else M_NEG
    tilt = np.array([[0.03, -0.02, 0.01], [0.01, 0.02, -0.03]])
    M = np.stack([so.normalize_rows(base + i * tilt) for i in range(n)])
    assert all((m[0] @ m[1] >= 0) == (regime == "he") for m in M)
    mc = np.stack([np.array([1.6 + 0.11 * i, 1.2 + 0.07 * i]) for i in range(n)])
    rng = np.random.RandomState(5 + n)
    ab = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.8, 1.2, n), rng.uniform(-0.2, 0.2, n)], axis=1)
    return M, mc, ab


def _dev_tiles(cpu, off):
    """the tiles on the device, `off` bytes past an aligned address (a contiguous view of a larger buffer)"""
    buf = torch.zeros(cpu.numel() + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + cpu.numel()] = cpu.reshape(-1).cuda()
    return buf[off:off + cpu.numel()].view(cpu.shape)


def _jit(dev, M, mc, Mt, mct, ab, bg, fmt=None, params=None, out_off=0):
    """engine.normalize_jitter into a guarded buffer -> CPU tensor ((n,h,w,3) uint8, or (n,3,h,w) in the format's memory layout).
    The output sits 16 bytes + out_off elements into a buffer of SENTINEL with 16 more bytes behind it; everything outside the body
    must still hold SENTINEL afterwards."""
    from stainlib_amd import engine
    n, h, w, _ = dev.shape
    dtype = fmt.dtype if fmt is not None else torch.uint8
    esize = torch.empty((), dtype=dtype).element_size()
    start, size = 16 // esize + out_off, n * h * w * 3
    buf = torch.full((start + size + 16 // esize,), SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    body = buf[start:start + size]
    if fmt is None:
        out = body.view(n, h, w, 3)
    elif fmt.channels_last:
        out = body.view(n, h, w, 3).permute(0, 3, 1, 2)
    else:
        out = body.view(n, 3, h, w)
    res = engine.normalize_jitter(dev, M, mc, Mt, mct, ab, augment_background=bg, params=params, fmt=fmt, out=out)
    assert res is out
    torch.cuda.synchronize()
    got = buf.cpu()
    outside = torch.cat([got[:start], got[start + size:]])
    assert bool((outside == SENTINEL).all()), f"{tuple(dev.shape)} fmt={fmt} out+{out_off}: written outside the output"
    return out.cpu()


def _same_bits(a, b):
    """equal as integer views, element by element in logical order (the memory layout of `got` is how _jit read the buffer)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _formats():
    return [stainlib_amd.TensorFormat(dtype=dt, channels_last=cl, mean=MEAN, std=STD) for dt in DTYPES for cl in (False, True)]


# ---- 1. no target is engine.stain_augment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [False, True])
@pytest.mark.parametrize("n,h,w,off", SHAPES)
def test_no_target_is_stain_augment(n, h, w, off, bg):
    from stainlib_amd import engine
    dev = _dev_tiles(_tiles(n, h, w), off)
    for regime in ("he", "neg"):
        M, mc, ab = _stats(n, regime)
        for params in (None, engine.make_params(luminosity_threshold=0.7, lasso_lambda=0.02)):
            want = engine.stain_augment(dev, M, ab, augment_background=bg, params=params).cpu()
            got = _jit(dev, M, mc, None, None, ab, bg, params=params)
            assert torch.equal(got, want), f"{n}x{h}x{w}+{off} {regime} bg={bg} params={'set' if params else 'default'}"
            if h * w >= 4096 and params is None:
                assert int((want != dev.cpu()).sum()) > 0                       # (the perturbation does something)


# ---- 2. alpha = 1, beta = 0 is engine.normalize_apply -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [False, True])
@pytest.mark.parametrize("n,h,w,off", SHAPES)
def test_identity_jitter_is_normalize_apply(n, h, w, off, bg):
    from stainlib_amd import engine
    dev = _dev_tiles(_tiles(n, h, w), off)
    M, mc, _ = _stats(n)
    ident = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (n, 1))
    for Mt, mct in ((M_TGT, MAXC_TGT), (so.normalize_rows(np.array([[0.60, 0.70, 0.30], [0.15, 0.90, 0.25]])), np.array([1.9, 0.8]))):
        assert (Mt >= 0).all()
        want = engine.normalize_apply(dev, M, mc, Mt, mct).cpu()
        assert torch.equal(_jit(dev, M, mc, Mt, mct, ident, bg), want), f"{n}x{h}x{w}+{off} bg={bg}"


# ---- 3. the tensor output is convert(uint8 result) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [False, True])
@pytest.mark.parametrize("n,h,w,off", SHAPES)
def test_tensor_output_is_convert_of_the_uint8_result(n, h, w, off, bg):
    dev = _dev_tiles(_tiles(n, h, w), off)
    M, mc, ab = _stats(n)
    for Mt, mct in ((M_TGT, MAXC_TGT), (None, None)):
        u8 = _jit(dev, M, mc, Mt, mct, ab, bg).cuda()
        for fmt in _formats():
            want = fmt.convert(u8).cpu()
            for out_off in (0, 1):                            # the wide path (where the shape allows it); the element-wise path
                got = _jit(dev, M, mc, Mt, mct, ab, bg, fmt=fmt, out_off=out_off)
                assert _same_bits(got, want), f"{n}x{h}x{w}+{off} bg={bg} {fmt} out+{out_off} target={Mt is not None}"


# ---- 4. the general case against the oracle, in binary64 --------------------------------------------------------------------------------
def _oracle_case(h, seeds):
    """tiles, their device fit (isolates the pass: the fit has its own tests) and their draws, computed once per size"""
    from stainlib_amd import engine
    key = ("oracle", h, seeds)
    if key not in _CACHE:
        tiles = [so.synth_tile(h, h, s) for s in seeds]
        dev = to_dev(tiles)
        M, mc, st = engine.macenko_fit(dev)
        assert (st.cpu().numpy() == 0).all()
        np.random.seed(11 + h)
        ab = np.array([[np.random.uniform(0.8, 1.2), np.random.uniform(-0.2, 0.2), np.random.uniform(0.8, 1.2), np.random.uniform(-0.2, 0.2)]
                       for _ in tiles])
        _CACHE[key] = (tiles, dev, M.cpu().numpy(), mc.cpu().numpy(), ab)
    return _CACHE[key]


def _oracle_check(tiles, got, M, mc, Mt, mct, ab, bg, label):
    for i, I in enumerate(tiles):
        a = so.StainAugmentor("macenko", augment_background=bg)
        a.image_shape, a.stain_matrix = I.shape, Mt
        a.source_concentrations = so.get_concentrations(I, M[i]) * (mct / mc[i])
        a.tissue_mask = so.tissue_mask(I).ravel()
        det = {}
        want = a.pop_with([ab[i, 0], ab[i, 2]], [ab[i, 1], ab[i, 3]], details=det)
        u8_parity(got[i].numpy(), want, label=f"{label} tile {i} bg={bg}", src=I, prequant=det["prequant"])


@pytest.mark.parametrize("bg", [False, True])
@pytest.mark.parametrize("h,seeds", [(64, (2, 3, 4)), (192, (5, 6)), (512, (700,))])
def test_against_the_oracle(h, seeds, bg):
    tiles, dev, M, mc, ab = _oracle_case(h, seeds)
    got = _jit(dev, M, mc, M_TGT, MAXC_TGT, ab, bg)
    _oracle_check(tiles, got, M, mc, M_TGT, MAXC_TGT, ab, bg, f"jitter {h}^2")


@pytest.mark.parametrize("bg", [False, True])
def test_against_the_oracle_with_a_negative_target_entry(bg):
    """values pass 255 here: the saturating cast against the oracle's clip (k_apply's general path would wrap them modulo 256)"""
    tiles, dev, M, mc, ab = _oracle_case(192, (5, 6))
    mct = np.array([2.4, 1.0])
    got = _jit(dev, M, mc, M_TGT_NEG, mct, ab, bg)
    _oracle_check(tiles, got, M, mc, M_TGT_NEG, mct, ab, bg, "jitter 192^2, negative target entry")
    assert int((got == 255).sum()) > 0


# ---- 5. a failed fit among good ones ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_a_failed_fit_comes_back_as_its_own_bytes(normalize):
    from stainlib_amd import engine
    good = [so.synth_tile(64, 64, s) for s in (2, 3)]
    white = np.full((64, 64, 3), 255, dtype=np.uint8)
    dev = to_dev([good[0], white, good[1]])
    _, _, ab = _stats(3)
    nz = stainlib_amd.MacenkoNormalizer()
    if normalize:
        nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    out, M, mc, status = nz.augment_batch(dev, ab, normalize=normalize)
    assert status.cpu().tolist() == [0, 1, 0]
    assert torch.equal(out[1], dev[1])
    ref, _, _, st2 = nz.augment_batch(dev[[0, 2]].contiguous(), ab[[0, 2]], normalize=normalize)      # the neighbours: as in a call without it
    assert st2.cpu().tolist() == [0, 0]
    assert torch.equal(out[[0, 2]], ref) and int((ref != dev[[0, 2]]).sum()) > 0
    # the raw pass-through rules on every path: NaN M_src, a zero maxC_src; aligned and not; uint8 and every format
    Mn, mcn = M.cpu().numpy().copy(), mc.cpu().numpy().copy()
    Mn[1], mcn[1] = so.normalize_rows(so.M_TRUE_SRC), [1.0, 0.0]
    Mt, mct = (nz.stain_matrix_target, nz.maxC_target.reshape(2)) if normalize else (None, None)
    for stats in ((M, mc), (Mn, mcn)):
        for tiles in (dev, dev[:, :5, :7].contiguous()):
            u8 = _jit(tiles, *stats, Mt, mct, ab, False)
            assert torch.equal(u8[1], tiles[1].cpu())
            for fmt in _formats():
                got = _jit(tiles, *stats, Mt, mct, ab, False, fmt=fmt)
                assert _same_bits(got, fmt.convert(u8.cuda()).cpu()), f"{tuple(tiles.shape)} {fmt}"
    x, _, _, _ = nz.augment_batch(dev, ab, normalize=normalize, tensor_format=_formats()[3])
    assert _same_bits(x.cpu(), _formats()[3].convert(out).cpu())


# ---- 6. augment_batch through both classes ----------------------------------------------------------------------------------------------
def test_augment_batch_through_both_classes():
    from stainlib_amd import engine
    tiles = [so.synth_tile(64, 64, s) for s in (2, 3, 4)]
    dev = to_dev(tiles)
    np.random.seed(3)
    ab = stainlib_amd.StainJitter(0.2, 0.2).draw(3)
    assert ab.shape == (3, 4) and ab.dtype == np.float64
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    Mf, mcf, stf = nz._fit_tiles(dev)
    for bg in (False, True):
        out, M, mc, status = nz.augment_batch(dev, ab, augment_background=bg)
        assert torch.equal(M, Mf) and torch.equal(mc, mcf) and torch.equal(status, stf) and status.cpu().tolist() == [0, 0, 0]
        want = engine.normalize_jitter(dev, Mf, mcf, nz.stain_matrix_target, nz.maxC_target.reshape(2), ab, augment_background=bg)
        assert out.dtype == torch.uint8 and out.shape == dev.shape and torch.equal(out, want)
        assert int((out != nz.transform_batch(dev)[0]).sum()) > 0
        sa = stainlib_amd.StainAugmentor("macenko", augment_background=bg)
        o2, M2, mc2, st2 = sa.augment_batch(dev, ab)
        assert torch.equal(M2, Mf) and torch.equal(st2, stf)
        assert torch.equal(o2, engine.normalize_jitter(dev, Mf, mcf, None, None, ab, augment_background=bg))
        own, _, _, _ = nz.augment_batch(dev, ab, augment_background=bg, normalize=False)
        assert torch.equal(own, o2)
    # identity jitter: transform_batch's image
    ident = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (3, 1))
    assert torch.equal(nz.augment_batch(dev, ident)[0], nz.transform_batch(dev)[0])
    # a caller's buffer and a tensor format
    fmt = stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD)
    buf = torch.empty((3, 3, 64, 64), dtype=torch.float16, device="cuda", memory_format=torch.channels_last)
    x, _, _, _ = nz.augment_batch(dev, ab, out=buf, tensor_format=fmt)
    assert x is buf and _same_bits(x.cpu(), fmt.convert(nz.augment_batch(dev, ab)[0]).cpu())
    x2, _, _, _ = stainlib_amd.StainAugmentor("macenko").augment_batch(dev, ab, tensor_format=fmt)
    assert _same_bits(x2.cpu(), fmt.convert(stainlib_amd.StainAugmentor("macenko").augment_batch(dev, ab)[0]).cpu())
    # StainAugmentor.augment_batch on one tile draws and computes what fit(I); pop() does
    for bg in (False, True):
        sa = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1, augment_background=bg)
        np.random.seed(23)
        one, _, _, _ = sa.augment_batch(dev[:1])
        after = np.random.uniform()
        sb = stainlib_amd.StainAugmentor("macenko", sigma1=0.15, sigma2=0.1, augment_background=bg)
        sb.fit(tiles[0])
        np.random.seed(23)
        popped = sb.pop()
        assert np.random.uniform() == after                                       # the same four draws were consumed
        assert np.array_equal(one[0].cpu().numpy(), popped), f"bg={bg}"


def test_vahadane_augment_batch():
    from stainlib_amd import engine
    tile = to_dev([so.synth_tile(64, 64, 2)])
    ab = np.array([[1.1, 0.05, 0.9, -0.1]])
    nz = stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    out, M, mc, status = nz.augment_batch(tile, ab)
    assert status.cpu().tolist() == [0]
    Mf, mcf, _ = nz.fit_batch_targets(tile)
    assert torch.equal(M, Mf) and torch.equal(mc, mcf)
    assert torch.equal(out, engine.normalize_jitter(tile, Mf, mcf, nz.stain_matrix_target, nz.maxC_target.reshape(2), ab))
    o2, M2, _, _ = stainlib_amd.StainAugmentor("vahadane").augment_batch(tile, ab)
    assert torch.equal(M2, Mf) and torch.equal(o2, engine.stain_augment(tile, Mf, ab))


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fmt", [False, True])
def test_graph_capture_replays_to_the_same_bytes(with_fmt):
    from stainlib_amd import engine
    n, h, w = 2, 64, 64
    cpu = _tiles(n, h, w)
    M, mc, ab = _stats(n)
    dev = cpu.cuda()
    d = [torch.as_tensor(a, dtype=torch.float64, device="cuda").contiguous() for a in (M, mc, M_TGT, MAXC_TGT, ab)]
    fmt = _formats()[2] if with_fmt else None
    want = engine.normalize_jitter(dev, *d, fmt=fmt).clone()
    out = torch.zeros_like(want)
    g = engine.Graphed(lambda: engine.normalize_jitter(dev, *d, fmt=fmt, out=out))
    out.zero_()
    res = g.replay()
    torch.cuda.synchronize()
    assert res is out and _same_bits(out.cpu(), want.cpu())
    # refilled in place: the graph follows the tensors
    other = torch.from_numpy(np.stack([so.synth_tile(h, w, 90 + i) for i in range(n)])).cuda()
    dev.copy_(other)
    d[4].copy_(torch.as_tensor(ab[::-1].copy(), device="cuda"))
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(out.cpu(), engine.normalize_jitter(other, d[0], d[1], d[2], d[3], ab[::-1].copy(), fmt=fmt).cpu())

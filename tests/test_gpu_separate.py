"""-m gpu: stain separation (sl_stain_separate, engine.stain_separate, separate_batch / separate).

The definitions under test (include/stainlib_hip.h, SlSeparateOut) make "separate" equal "compose it yourself", bit for bit:
    norm      = the bytes of sl_normalize_apply
    stain[i]  = the bytes of sl_normalize_apply with the OTHER row of M_tgt zeroed (wherever both take the same lasso form)
    conc      = c_i * float32(ratio_i 2^k), planar; the half types = that binary32 value rounded to nearest even
so most of this file compares against engine.normalize_apply (another kernel) with torch.equal; the oracle comparison (3) is independent
of the library.  Every call goes through _run: the raw C entry point on buffers with sentinel elements before and after each output
(and whole sentinel buffers where an output is not requested), all checked after the call."""
import ctypes as C

import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import _ffi
from stainlib_amd.utils.excepts import TissueMaskException
from tests.gpu_util import oracle_fit_tile, to_dev, u8_parity

pytestmark = pytest.mark.gpu

FIELDS = ("norm", "h", "e", "conc")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
SENTINEL = 77                                                 # exactly representable in all four element types
# the tensor-output test's set -- fewer than 4 pixels; a ragged chunk with misaligned tiles; aligned; two parts (more than 32 Ki pixels)
# ragged; two parts aligned -- and (6, 6): P a multiple of 4 but not of 8, where the wide path of the half types must decline
SHAPES = [(1, 1), (5, 7), (8, 8), (181, 183), (192, 192), (6, 6)]
M_NEG = so.normalize_rows(np.array([[0.9, -0.3, 0.3], [-0.2, 0.95, 0.25]]))               # g12 < 0 (tests/test_gpu_apply.py)
M_TGT_NEG = so.normalize_rows(np.array([[0.55, 0.80, -0.25], [0.10, 0.95, 0.20]]))        # a negative entry in row H
_CACHE = {}


def _tiles(h, w):
    """3 tiles of random bytes; pixel 0 of tile 0 is background white.  With n = 3 the second and third tile start at odd byte offsets
    whenever h w is odd."""
    if ("tiles", h, w) not in _CACHE:
        t = np.random.RandomState(h * 1000 + w).randint(0, 256, size=(3, h, w, 3)).astype(np.uint8)
        t[0, 0, 0] = 255
        _CACHE[("tiles", h, w)] = torch.from_numpy(t)
    return _CACHE[("tiles", h, w)]


def _regime(name):
    """(M_src (3,2,3), maxC_src (3,2), M_tgt (2,3), maxC_tgt (2,)) -- the per-pixel sweep does not care whether M fits the tile."""
    if ("regime", name) not in _CACHE:
        if name == "he":                  # the fast path: three fitted H&E sources, the H&E target
            fits = [oracle_fit_tile(so.synth_tile(64, 64, s)) for s in (2, 3, 4)]
            r = (np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]), so.normalize_rows(so.M_TRUE_TGT), np.array([1.5, 1.1]))
        elif name == "neg":               # negatively correlated source rows: the general lasso on both sides
            assert M_NEG[0] @ M_NEG[1] < 0
            r = (np.stack([M_NEG] * 3), np.stack([np.array([1.7, 1.3])] * 3), so.normalize_rows(so.M_TRUE_TGT), np.array([1.5, 1.1]))
        else:                             # "tneg": a target with a negative entry (values pass 255: the wrapping cast)
            r = (np.stack([so.normalize_rows(so.M_TRUE_SRC)] * 3), np.stack([np.array([1.6, 1.2])] * 3), M_TGT_NEG, np.array([2.4, 1.0]))
        _CACHE[("regime", name)] = r
    return _CACHE[("regime", name)]


def _f64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda() if a is not None else None


def _run(cpu, M, mc, Mt=None, mct=None, want=FIELDS, dtype=torch.float32, in_off=0, out_off=0):
    """sl_stain_separate on the tiles `cpu` ((n,h,w,3) uint8 CPU tensor) -> Separated of CPU tensors.  The input sits in_off bytes,
    every output out_off elements past an aligned address.  All four output buffers exist, filled with SENTINEL and 16 bytes longer at
    either end; only the wanted ones are handed over; everything outside the wanted bodies must still hold SENTINEL afterwards."""
    n, h, w, _ = cpu.shape
    P = h * w
    src = torch.empty(cpu.numel() + 1, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + cpu.numel()] = cpu.reshape(-1).cuda()
    o = _ffi.default_separate_out()
    o.conc_dtype = {torch.float32: _ffi.DTYPE_F32, torch.float16: _ffi.DTYPE_F16, torch.bfloat16: _ffi.DTYPE_BF16}[dtype]
    bufs = {}
    for name in FIELDS:
        dt, size = (dtype, n * 2 * P) if name == "conc" else (torch.uint8, n * P * 3)
        esize = torch.empty((), dtype=dt).element_size()
        start = 16 // esize + out_off
        buf = torch.full((start + size + 16 // esize,), SENTINEL, dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        bufs[name] = (buf, start, size)
        if name in want:
            p = buf.data_ptr() + start * esize
            if name == "conc":
                o.conc = p
            elif name == "norm":
                o.norm = p
            else:
                o.stain["he".index(name)] = p
    stats = [_f64(M), _f64(mc), _f64(Mt), _f64(mct)]
    rc = _ffi.lib().sl_stain_separate(C.c_void_p(src.data_ptr() + in_off), n, h, w, *(C.c_void_p(t.data_ptr() if t is not None else 0) for t in stats),
                                      0.01, C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, h, w, want)
    torch.cuda.synchronize()
    res = {}
    for name, (buf, start, size) in bufs.items():
        got = buf.cpu()
        if name not in want:
            assert bool((got == SENTINEL).all()), f"{h}x{w} want={want}: the unrequested {name} buffer was written"
            res[name] = None
            continue
        outside = torch.cat([got[:start], got[start + size:]])
        assert bool((outside == SENTINEL).all()), f"{h}x{w} in+{in_off} out+{out_off} want={want}: written outside {name}"
        res[name] = got[start:start + size].reshape((n, 2, h, w) if name == "conc" else (n, h, w, 3)).clone()
    return stainlib_amd.Separated(**res)


def _apply(cpu, M, mc, Mt, mct):
    """engine.normalize_apply -> CPU tensor"""
    from stainlib_amd import engine
    return engine.normalize_apply(cpu.cuda(), M, mc, Mt, mct).cpu()


def _composed(h, w, regime):
    """What a caller composes at the parent commit: (norm, H-only, E-only) = three normalize_apply calls (computed once per case)."""
    key = ("composed", h, w, regime)
    if key not in _CACHE:
        M, mc, Mt, mct = _regime(regime)
        only_h, only_e = Mt.copy(), Mt.copy()
        only_h[1] = 0.0
        only_e[0] = 0.0
        cpu = _tiles(h, w)
        _CACHE[key] = tuple(_apply(cpu, M, mc, T, mct) for T in (Mt, only_h, only_e))
    return _CACHE[key]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


# ---- 1. norm is sl_normalize_apply ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_norm_is_normalize_apply(h, w):
    M, mc, Mt, mct = _regime("he")
    cpu = _tiles(h, w)
    want_norm = _composed(h, w, "he")[0]
    for want in (FIELDS, ("norm",)):
        for in_off, out_off in ((0, 0), (1, 0), (0, 1)):
            got = _run(cpu, M, mc, Mt, mct, want=want, in_off=in_off, out_off=out_off)
            assert torch.equal(got.norm, want_norm), f"{h}x{w} want={want} in+{in_off} out+{out_off}"


# ---- 2. the stain images are the single-row apply ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["he", "neg", "tneg"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_stain_images_are_the_single_row_apply(h, w, regime):
    M, mc, Mt, mct = _regime(regime)
    norm, only_h, only_e = _composed(h, w, regime)
    got = _run(_tiles(h, w), M, mc, Mt, mct)
    assert torch.equal(got.norm, norm)
    assert torch.equal(got.h, only_h), f"{h}x{w} {regime}: H image"
    if regime != "tneg":
        assert torch.equal(got.e, only_e), f"{h}x{w} {regime}: E image"
    else:
        # The full target has a negative entry in row H, so the separation takes the general lasso; the single-row apply of row E sees
        # a target without one and takes the branch-free form: two binary32 evaluations of the same optimum, held to the byte bar.
        for i in range(3):
            u8_parity(got.e[i].numpy(), only_e[i].numpy(), label=f"{h}x{w} tneg E image, tile {i}")
    if regime == "tneg" and h * w >= 64:
        assert int((got.h != only_e).sum()) > 0 and int((got.h != norm).sum()) > 0      # (the three images are three different images)


# ---- 3. against the oracle, independently of the library --------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["fit", "neg"])
@pytest.mark.parametrize("h,w,seeds", [(96, 130, (2, 3)), (33, 47, (4,))])
def test_against_the_oracle(h, w, seeds, regime):
    tiles = [so.synth_tile(h, w, s) for s in seeds]
    Mt, mct = so.normalize_rows(so.M_TRUE_TGT), np.array([1.5, 1.1])
    if regime == "fit":
        fits = [oracle_fit_tile(I) for I in tiles]
        M, mc = np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits])
    else:
        M, mc = np.stack([M_NEG] * len(tiles)), np.stack([np.array([1.7, 1.3])] * len(tiles))
    got = _run(torch.from_numpy(np.stack(tiles)), M, mc, Mt, mct)
    for i, I in enumerate(tiles):
        ratio = mct / mc[i]
        Cn = so.get_concentrations(I, M[i]) * ratio
        u8_parity(got.norm[i].numpy(), so.truncate_u8((255 * np.exp(-Cn @ Mt)).reshape(I.shape)), label=f"{regime} norm")
        for k, img in enumerate((got.h, got.e)):
            want = so.truncate_u8((255 * np.exp(-Cn[:, k, None] * Mt[k])).reshape(I.shape))
            u8_parity(img[i].numpy(), want, label=f"{regime} stain {k}")
        conc = got.conc[i].numpy().reshape(2, -1).astype(np.float64)
        for k in range(2):
            err = float(np.abs(conc[k] - Cn[:, k]).max())
            print(f"{regime} {h}x{w} tile {i} conc[{k}]: max abs error {err:.2e} (bound {5e-6 * max(1.0, ratio[k]):.2e})")
            assert err <= 5e-6 * max(1.0, ratio[k])
        if regime == "neg" and i == 0 and h * w > 10000:          # all four active sets occur under the negatively correlated pair
            a, b = Cn[:, 0] > 0, Cn[:, 1] > 0
            assert (a & b).any() and (a & ~b).any() and (~a & b).any() and (~a & ~b).any()
            ga, gb = conc[0] > 0, conc[1] > 0
            assert (ga & gb).any() and (ga & ~gb).any() and (~ga & gb).any() and (~ga & ~gb).any()


# ---- 4. the half types ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["he", "neg"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_half_types_round_the_float32_planes(h, w, regime):
    M, mc, Mt, mct = _regime(regime)
    cpu = _tiles(h, w)
    ref = _run(cpu, M, mc, Mt, mct)
    c32 = ref.conc
    assert bool((c32 >= 0).all()) and bool(torch.isfinite(c32).all())
    # the background pixel: exactly +0 in both planes, 255 in every byte of both stain images
    assert torch.equal(c32[0, :, 0, 0].view(torch.int32), torch.zeros(2, dtype=torch.int32))
    assert bool((ref.h[0, 0, 0] == 255).all()) and bool((ref.e[0, 0, 0] == 255).all())
    if h * w >= 64:
        assert bool((c32 > 0).any())
    for dtype in (torch.float16, torch.bfloat16):
        want = c32.to(dtype)                                  # torch on the CPU: round-to-nearest-even
        for out_off in (0, 1):                                # the wide path (where the shape allows it); the element-wise path
            for fields in (FIELDS, ("conc",)):
                got = _run(cpu, M, mc, Mt, mct, want=fields, dtype=dtype, out_off=out_off)
                assert _same_bits(got.conc, want), f"{h}x{w} {dtype} out+{out_off} want={fields}"
    for out_off, in_off in ((1, 0), (0, 1)):                  # float32 itself, off the wide path
        assert _same_bits(_run(cpu, M, mc, Mt, mct, want=("conc",), out_off=out_off, in_off=in_off).conc, c32)
        assert _same_bits(_run(cpu, M, mc, Mt, mct, want=("h", "e", "conc"), out_off=out_off, in_off=in_off).conc, c32)


# ---- 5. no target -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (64, 64), (181, 183)])
def test_no_target_is_every_tile_under_its_own_matrix(h, w):
    from stainlib_amd import engine
    M, mc, _, _ = _regime("he")
    tiles = [so.synth_tile(h, w, s) for s in (2, 3, 4)]
    dev = to_dev(tiles)
    sep = engine.stain_separate(dev, M, mc)
    assert sep.norm.shape == (3, h, w, 3) and sep.h.shape == sep.e.shape == (3, h, w, 3) and sep.conc.shape == (3, 2, h, w)
    assert sep.conc.dtype == torch.float32 and sep.norm.dtype == sep.h.dtype == sep.e.dtype == torch.uint8
    for i, I in enumerate(tiles):
        own = engine.normalize_apply(dev[i:i + 1], M[i:i + 1], mc[i:i + 1], M[i], mc[i])
        assert torch.equal(sep.norm[i:i + 1], own), f"tile {i}"
        only_h = M[i].copy()
        only_h[1] = 0.0
        assert torch.equal(sep.h[i:i + 1], engine.normalize_apply(dev[i:i + 1], M[i:i + 1], mc[i:i + 1], only_h, mc[i]))
        Co = so.get_concentrations(I, M[i])
        err = float(np.abs(sep.conc[i].cpu().numpy().reshape(2, -1).T - Co).max())
        print(f"no target {h}x{w} tile {i}: conc max abs error {err:.2e}")
        assert err <= 5e-6
    # the raw entry point agrees, sentinels intact
    raw = _run(torch.from_numpy(np.stack(tiles)), M, mc)
    for a, b in zip(raw, sep):
        assert torch.equal(a, b.cpu())


# ---- 6. failed fits and guards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan_M", "zero_maxC"])
@pytest.mark.parametrize("h,w", [(5, 7), (8, 8), (181, 183), (192, 192), (6, 6)])
def test_a_failed_fit_is_passed_through(h, w, bad):
    M, mc, Mt, mct = _regime("he")
    M, mc = M.copy(), mc.copy()
    if bad == "nan_M":
        M[1] = np.nan
    else:
        mc[1, 1] = 0.0
    cpu = _tiles(h, w)
    outer = torch.stack([cpu[0], cpu[2]])
    for dtype in DTYPES:
        got = _run(cpu, M, mc, Mt, mct, dtype=dtype)
        assert torch.equal(got.norm[1], cpu[1])
        assert bool((got.h[1] == 255).all()) and bool((got.e[1] == 255).all())
        assert bool((got.conc[1].contiguous().view(BITS[dtype]) == 0).all()), "conc of a failed tile must be +0 (bit pattern)"
        ref = _run(outer, M[[0, 2]], mc[[0, 2]], Mt, mct, dtype=dtype)          # the outer tiles: as in a call without the bad one
        for a, b in zip(got, ref):
            assert _same_bits(a[[0, 2]], b) if a.dtype != torch.uint8 else torch.equal(a[[0, 2]], b)
    got = _run(cpu, M, mc, want=("norm", "e", "conc"), out_off=1)             # no target, off the aligned path
    assert torch.equal(got.norm[1], cpu[1]) and bool((got.e[1] == 255).all()) and bool((got.conc[1].view(torch.int32) == 0).all())


@pytest.mark.parametrize("want", [("norm",), ("h",), ("e",), ("conc",), ("h", "e"), ("norm", "conc"), ("norm", "h"), ("e", "conc")], ids=str)
def test_output_subsets_write_what_was_asked_and_nothing_else(want):
    """_run hands over only the wanted pointers -- ("h",) alone leaves stain[1] NULL -- and checks that the other buffers and every
    guard element still hold the sentinel."""
    M, mc, Mt, mct = _regime("he")
    for h, w in ((5, 7), (8, 8), (181, 183)):
        full = _run(_tiles(h, w), M, mc, Mt, mct)
        for dtype in ((torch.float32, torch.bfloat16) if "conc" in want else (torch.float32,)):
            got = _run(_tiles(h, w), M, mc, Mt, mct, want=want, dtype=dtype)
            for name in FIELDS:
                a, b = getattr(got, name), getattr(full, name)
                if name not in want:
                    assert a is None
                elif name == "conc":
                    assert _same_bits(a, b.to(dtype))
                else:
                    assert torch.equal(a, b), (h, w, want, name)


# ---- 7. the Python surface --------------------------------------------------------------------------------------------------------------
def test_separate_batch_and_separate():
    from stainlib_amd import engine
    tiles = [so.synth_tile(64, 64, s) for s in (2, 3)] + [np.full((64, 64, 3), 255, dtype=np.uint8)]
    dev = to_dev(tiles)
    nz = stainlib_amd.MacenkoNormalizer()
    raw, Mr, mcr, st = nz.separate_batch(dev, normalize=False)                  # no target: works on an unfitted normalizer
    assert st.cpu().tolist() == [0, 0, 1]
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    sep, M, mc, status = nz.separate_batch(dev)
    assert status.cpu().tolist() == [0, 0, 1]
    Mf, mcf, stf = nz.fit_batch_targets(dev)
    assert torch.equal(M[:2], Mf[:2]) and torch.equal(mc[:2], mcf[:2]) and torch.equal(status, stf)
    want = engine.stain_separate(dev, Mf, mcf, nz.stain_matrix_target, nz.maxC_target.reshape(2))
    for a, b in zip(sep, want):
        assert torch.equal(a, b)
    for a, b in zip(raw, engine.stain_separate(dev, Mf, mcf)):
        assert torch.equal(a, b)
    # norm is transform_batch's image
    assert torch.equal(sep.norm, nz.transform_batch(dev)[0])
    # the white tile is passed through
    for s in (sep, raw):
        assert torch.equal(s.norm[2], dev[2]) and bool((s.h[2] == 255).all()) and bool((s.e[2] == 255).all())
        assert bool((s.conc[2].view(torch.int32) == 0).all())
    # want / conc_dtype
    part, _, _, _ = nz.separate_batch(dev, want=("h", "conc"), conc_dtype=torch.float16)
    assert part.norm is None and part.e is None and torch.equal(part.h, sep.h)
    assert part.conc.dtype == torch.float16 and _same_bits(part.conc.cpu(), sep.conc.cpu().to(torch.float16))
    # a caller's buffers are the ones returned
    out = engine.Separated(norm=torch.empty_like(dev), conc=torch.empty((3, 2, 64, 64), dtype=torch.bfloat16, device="cuda"))
    res = engine.stain_separate(dev, Mf, mcf, nz.stain_matrix_target, nz.maxC_target.reshape(2), want=("norm", "conc"),
                                conc_dtype=torch.bfloat16, out=out)
    assert res.norm is out.norm and res.conc is out.conc and res.h is None and res.e is None
    assert torch.equal(res.norm, sep.norm) and _same_bits(res.conc.cpu(), sep.conc.cpu().to(torch.bfloat16))
    for bad in (engine.Separated(norm=torch.empty((3, 64, 64, 3), dtype=torch.uint8)),                       # on the CPU
                engine.Separated(norm=torch.empty((2, 64, 64, 3), dtype=torch.uint8, device="cuda")),         # shape
                engine.Separated(h=torch.empty((3, 64, 64, 6), dtype=torch.uint8, device="cuda")[..., ::2])):  # not contiguous
        with pytest.raises(ValueError, match="must be a contiguous"):
            engine.stain_separate(dev, Mf, mcf, out=bad)
    # separate(I): numpy in, numpy out
    one = nz.separate(tiles[0])
    assert isinstance(one, stainlib_amd.Separated)
    assert all(isinstance(a, np.ndarray) for a in one)
    assert one.norm.shape == one.h.shape == one.e.shape == (64, 64, 3) and one.norm.dtype == one.h.dtype == one.e.dtype == np.uint8
    assert one.conc.shape == (2, 64, 64) and one.conc.dtype == np.float32
    assert np.array_equal(one.norm, nz.transform(tiles[0])) and np.array_equal(one.h, sep.h[0].cpu().numpy())
    assert np.array_equal(one.conc, sep.conc[0].cpu().numpy())
    own = nz.separate(tiles[0], normalize=False)
    assert np.array_equal(own.conc, raw.conc[0].cpu().numpy()) and np.array_equal(own.e, raw.e[0].cpu().numpy())
    with pytest.raises(TissueMaskException):
        nz.separate(tiles[2])
    with pytest.raises(TissueMaskException):
        nz.transform(tiles[2])


def test_vahadane_separate_batch():
    from stainlib_amd import engine
    tile = to_dev([so.synth_tile(64, 64, 2)])
    nz = stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    sep, M, mc, status = nz.separate_batch(tile)
    assert status.cpu().tolist() == [0]
    Mf, mcf, _ = nz.fit_batch_targets(tile)
    assert torch.equal(M, Mf) and torch.equal(mc, mcf)
    for a, b in zip(sep, engine.stain_separate(tile, Mf, mcf, nz.stain_matrix_target, nz.maxC_target.reshape(2))):
        assert torch.equal(a, b)
    assert torch.equal(sep.norm, nz.transform_batch(tile)[0])

"""-m gpu: the model-ready tensor output (sl_to_tensor, sl_normalize_apply_tensor, TensorFormat, tensor_format=).

The definition under test (include/stainlib_hip.h): for a result byte b of channel c
    v = fma(float32(b), scale32[c], shift32[c]),  scale32 = float32(1 / (255 std)),  shift32 = float32(-mean / std)
    out = v converted to the output type, round-to-nearest-even.
The expected table is computed here, independently of the code under test, as
    T[b, c] = float32(float64(b) * float64(scale32[c]) + float64(shift32[c]))
which is exact in binary64 -- hence rounded once, like the FMA -- when the binary exponents of scale32 and shift32 differ by at most
20: the 8 x 24-bit product and the 24-bit addend then fit 53 bits together.  _table asserts that precondition on its constants.
For the half types the expectation is T.to(dtype) (torch on the CPU: round-to-nearest-even)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import _ffi
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

FORMATS = {
    "identity": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "uneven": ((0.5, 0.25, 0.7), (0.5, 0.3, 0.125)),          # exponents of scale32 / shift32: 2^-7 / 2^0, 2^-7 / 2^-1, 2^-5 / 2^2
}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
SENTINEL = 77.0                                               # exactly representable in all three types; no table entry equals it
_CACHE = {}


def _fmt(dtype, channels_last, name):
    mean, std = FORMATS[name]
    return stainlib_amd.TensorFormat(dtype, channels_last, mean, std)


def _table(name):
    """T (256, 3) float32 of a format set (computed once)."""
    if ("T", name) not in _CACHE:
        mean, std = (np.asarray(v, dtype=np.float64) for v in FORMATS[name])
        scale32 = (1.0 / (255.0 * std)).astype(np.float32)
        shift32 = (-mean / std).astype(np.float32)
        for c in range(3):                                    # the precondition of the exactness argument in the module docstring
            if shift32[c] != 0:
                assert abs(math.frexp(float(scale32[c]))[1] - math.frexp(float(shift32[c]))[1]) <= 20, (name, c)
        b = np.arange(256, dtype=np.float64)[:, None]
        T = (b * scale32.astype(np.float64)[None, :] + shift32.astype(np.float64)[None, :]).astype(np.float32)
        assert not (T == SENTINEL).any()
        _CACHE[("T", name)] = torch.from_numpy(T)
    return _CACHE[("T", name)]


def _expected(tiles_u8_cpu, name, dtype, channels_last):
    """(n, 3, h, w) tensor in the format's memory layout, from the table"""
    T = _table(name)
    nhwc = T[tiles_u8_cpu.long(), torch.arange(3)]            # (n, h, w, 3) float32
    x = nhwc.permute(0, 3, 1, 2).to(dtype)
    return x.contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def _memory(x, channels_last):
    """the elements of an (n, 3, h, w) tensor in memory order, as integers (bit-for-bit comparison, NaN-proof)"""
    flat = (x.permute(0, 2, 3, 1) if channels_last else x).contiguous().reshape(-1)
    return flat.view(BITS[x.dtype])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _tiles(h, w):
    """3 tiles of h x w: random bytes, the middle one arange-filled (byte k = k mod 256: with 256 pixels or more every value occurs in
    every channel, since gcd(3, 256) = 1).  With n = 3 the second and third tile start at odd byte offsets whenever h w is odd."""
    if ("tiles", h, w) not in _CACHE:
        rs = np.random.RandomState(h * 1000 + w)
        t = rs.randint(0, 256, size=(3, h, w, 3)).astype(np.uint8)
        t[1] = (np.arange(h * w * 3) % 256).astype(np.uint8).reshape(h, w, 3)
        if h * w >= 256:
            for c in range(3):
                assert len(np.unique(t[1][..., c])) == 256
        _CACHE[("tiles", h, w)] = torch.from_numpy(t)
    return _CACHE[("tiles", h, w)]


# the smallest shapes at which the kernel can go wrong: fewer than 4 pixels; a ragged chunk and misaligned planes; aligned; two parts
# (more than 32 Ki pixels) ragged; two parts aligned
SHAPES = [(1, 1), (5, 7), (8, 8), (181, 183), (192, 192)]


@pytest.mark.parametrize("name", list(FORMATS))
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_converter_bit_for_bit(dtype, channels_last, name):
    from stainlib_amd import engine
    lib = _ffi.lib()
    f, _, _ = engine._tensor_format(_fmt(dtype, channels_last, name))
    stream = torch.cuda.current_stream().cuda_stream
    esize = torch.empty((), dtype=dtype).element_size()
    for h, w in SHAPES:
        cpu = _tiles(h, w)
        n, P = 3, h * w
        want = _memory(_expected(cpu, name, dtype, channels_last), channels_last)
        src = torch.empty(cpu.numel() + 1, dtype=torch.uint8, device="cuda")
        # (input byte offset, output element offset): plain; a byte-offset view of the input; an `out` view offset by one element
        for in_off, out_off in ((0, 0), (1, 0), (0, 1)):
            src[in_off:in_off + cpu.numel()] = cpu.reshape(-1).cuda()
            dst = torch.full((n * 3 * P + 2,), SENTINEL, dtype=dtype, device="cuda")
            rc = lib.sl_to_tensor(C.c_void_p(src.data_ptr() + in_off), C.c_void_p(dst.data_ptr() + out_off * esize), n, h, w, C.byref(f), stream)
            assert rc == 0, (rc, h, w)
            got = dst.cpu()
            body = got[out_off:out_off + n * 3 * P].view(BITS[dtype])
            bad = int((body != want).sum())
            assert bad == 0, f"{h}x{w} in+{in_off} out+{out_off}: {bad} of {body.numel()} elements differ from the table"
            outside = torch.cat([got[:out_off], got[out_off + n * 3 * P:]])
            assert bool((outside == SENTINEL).all()), f"{h}x{w} in+{in_off} out+{out_off}: written outside the output"
    # the Python entry point: shape, dtype, memory format, and a caller's `out`
    dev = _tiles(5, 7).cuda()
    fmt = _fmt(dtype, channels_last, name)
    x = fmt.convert(dev)
    assert x.shape == (3, 3, 5, 7) and x.dtype == dtype
    assert x.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert _same_bits(x.cpu(), _expected(_tiles(5, 7), name, dtype, channels_last))
    out = torch.empty_like(x)
    assert fmt.convert(dev, out=out) is out and _same_bits(out, x)


def test_out_is_checked():
    fmt = stainlib_amd.TensorFormat(torch.float16)
    dev = _tiles(8, 8).cuda()
    for bad in (torch.empty((3, 3, 8, 8), dtype=torch.float32, device="cuda"), torch.empty((3, 3, 8, 8), dtype=torch.float16),
                torch.empty((3, 8, 8, 3), dtype=torch.float16, device="cuda"),
                torch.empty((3, 3, 8, 8), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last),
                torch.empty((3, 3, 8, 16), dtype=torch.float16, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            fmt.convert(dev, out=bad)
    with pytest.raises(ValueError):
        stainlib_amd.TensorFormat(torch.float16, channels_last=True).convert(dev, out=torch.empty((3, 3, 8, 8), dtype=torch.float16, device="cuda"))


@pytest.mark.parametrize("name", list(FORMATS))
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_close_to_the_torch_expression(channels_last, name):
    """float32 against the line every user writes: |ours - ((x / 255 - mean) / std)| <= 8 * 2^-24 * (1 + |mean_c|) / std_c -- three
    roundings on each side plus the roundings of the constants, each at most 2^-24 of a magnitude of at most (1 + |mean_c|) / std_c."""
    dev = _tiles(181, 183).cuda()
    mean, std = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in FORMATS[name])
    ours = _fmt(torch.float32, channels_last, name).convert(dev)
    theirs = ((dev.permute(0, 3, 1, 2).float() / 255) - mean[:, None, None]) / std[:, None, None]
    err = (ours.double() - theirs.double()).abs().amax(dim=(0, 2, 3)).cpu()
    bound = torch.tensor([8 * 2.0 ** -24 * (1 + abs(m)) / s for m, s in zip(*FORMATS[name])], dtype=torch.float64)
    print(f"{name} {'nhwc' if channels_last else 'nchw'}: max |ours - torch| per channel {err.tolist()}, bound {bound.tolist()}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())


def _apply_inputs():
    """(tiles 5 x 64^2 [4 synthetic + a white one whose M_src is NaN], M, maxC), (one 37 x 41 tile, M, maxC), targets: the usual one
    (K.fast) and one with a negative entry (the general truncation: values past 255 wrap)"""
    if "apply" not in _CACHE:
        from stainlib_amd import engine
        a = to_dev([so.synth_tile(64, 64, s) for s in (2, 3, 4, 5)] + [np.full((64, 64, 3), 255, np.uint8)])
        b = to_dev([so.synth_tile(37, 41, 6)])
        Ma, ca, sa = engine.macenko_fit(a)
        Mb, cb, sb = engine.macenko_fit(b)
        assert sa[:4].tolist() == [0] * 4 and sb.tolist() == [0]
        Ma, ca = Ma.clone(), ca.clone()
        Ma[4], ca[4] = math.nan, 1.0                          # pass-through by the NaN matrix alone
        Mt, ct, st = engine.macenko_fit(to_dev([so.synth_tile(64, 64, 1001, so.M_TRUE_TGT)]))
        assert int(st[0]) == 0
        M_neg = Mt[0].clone()
        M_neg[1, 2] = -0.3
        _CACHE["apply"] = ((a, Ma, ca), (b, Mb, cb), ((Mt[0], ct[0]), (M_neg, ct[0])))
    return _CACHE["apply"]


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fused_apply_equals_convert_after(dtype, channels_last):
    from stainlib_amd import engine
    batch_a, batch_b, targets = _apply_inputs()
    fmt = _fmt(dtype, channels_last, "imagenet")
    for k, (Mt, ct) in enumerate(targets):
        for tiles, M, maxC in (batch_a, batch_b):
            u8 = engine.normalize_apply(tiles, M, maxC, Mt, ct)
            fused = engine.normalize_apply_tensor(tiles, M, maxC, Mt, ct, fmt)
            after = engine.to_tensor(u8, fmt)
            assert _same_bits(fused, after), (k, tuple(tiles.shape))
            assert _same_bits(after.cpu(), _expected(u8.cpu(), "imagenet", dtype, channels_last))
            assert not torch.equal(u8[0], tiles[0])           # (the pass did something)
            if tiles.shape[0] == 5:
                assert torch.equal(u8[4], tiles[4])           # the white tile went through unchanged: its source bytes are converted
        if k == 1:      # (a positive exponent weight makes K.fast false whatever the pixels are; how far past 255 they went, for the log)
            pre = engine.normalize_apply(batch_a[0], batch_a[1], batch_a[2], Mt, ct, want_prequant=True)[1]
            print(f"general truncation: largest value before the cast {float(pre[:4].max()):.1f}")


def _equal_nan(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a,
                                              b.contiguous().view(torch.int64) if b.dtype == torch.float64 else b)


CLASS_FORMATS = [(torch.float16, False, "imagenet"), (torch.float32, True, "uneven"), (torch.bfloat16, False, "identity")]


def _target_tile():
    return so.synth_tile(128, 128, 1001, so.M_TRUE_TGT)


@pytest.mark.parametrize("method", ["macenko", "vahadane"])
def test_extractive_transform_batch(method):
    if method == "macenko":
        nrm = stainlib_amd.MacenkoNormalizer()
        dev = to_dev([so.synth_tile(96, 128, 10 + s) for s in range(6)] + [np.full((96, 128, 3), 255, np.uint8)])
    else:
        nrm = stainlib_amd.VahadaneNormalizer()
        dev = to_dev([so.synth_tile(96, 96, 20 + s) for s in range(3)])
    nrm.fit(_target_tile())
    u8, M, maxC, status = nrm.transform_batch(dev)
    if method == "macenko":
        assert status.tolist() == [0] * 6 + [1] and torch.equal(u8[6], dev[6])
    for dtype, cl, name in CLASS_FORMATS:
        fmt = _fmt(dtype, cl, name)
        want = fmt.convert(u8)
        res = {route: nrm.transform_batch(dev, tensor_format=fmt, _tensor_route=route) for route in (None, "fused", "convert")}
        for route, (x, M2, maxC2, status2) in res.items():
            assert _same_bits(x, want), (method, route, dtype, cl)
            assert x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            assert _equal_nan(M2, M) and _equal_nan(maxC2, maxC) and torch.equal(status2, status), (method, route)
        out = torch.empty_like(want)
        assert nrm.transform_batch(dev, out=out, tensor_format=fmt)[0] is out and _same_bits(out, want)
    with pytest.raises(ValueError):
        nrm.transform_batch(dev, tensor_format=_fmt(torch.float32, False, "identity"), _tensor_route="other")


def test_reinhard_and_hed_transform_batch():
    dev = to_dev([so.synth_tile(96, 128, 30 + s) for s in range(3)])
    rn = stainlib_amd.ReinhardStainNormalizer()
    rn.fit(_target_tile())
    u8, st = rn.transform_batch(dev)
    aug = stainlib_amd.HedLighterColorAugmenter()
    np.random.seed(7)
    sig, bias = aug.randomize_batch(3)
    a8, applied = aug.transform_batch(dev, sig, bias)
    for dtype, cl, name in CLASS_FORMATS:
        fmt = _fmt(dtype, cl, name)
        x, st2 = rn.transform_batch(dev, tensor_format=fmt)
        assert _same_bits(x, fmt.convert(u8)) and _equal_nan(st2, st)
        xm, _ = rn.transform_batch(dev, mask_background=True, tensor_format=fmt)
        assert _same_bits(xm, fmt.convert(rn.transform_batch(dev, mask_background=True)[0]))
        y, applied2 = aug.transform_batch(dev, sig, bias, tensor_format=fmt)
        assert _same_bits(y, fmt.convert(a8)) and torch.equal(applied2, applied)


@pytest.mark.parametrize("kind", ["macenko", "vahadane", "reinhard"])
def test_pooled_slide_normalizer(kind):
    """SlideNormalizer(mode="pooled") on one process: the tensor_format= result is TensorFormat.convert of the uint8 result of the same
    call, and the slide's statistics and the status are the same."""
    from stainlib_amd.distributed import SlideNormalizer
    nrm = {"macenko": stainlib_amd.MacenkoNormalizer, "vahadane": stainlib_amd.VahadaneNormalizer,
           "reinhard": stainlib_amd.ReinhardStainNormalizer}[kind]()
    nrm.fit(_target_tile())
    dev = to_dev([so.synth_tile(96, 128, 50 + s) for s in range(4)])
    sn = SlideNormalizer(nrm, group=False, mode="pooled")
    u8, a, b, status = sn.transform_shard(dev)
    assert not torch.equal(u8, dev)
    for dtype, cl, name in CLASS_FORMATS:
        fmt = _fmt(dtype, cl, name)
        x, a2, b2, status2 = sn.transform_shard(dev, tensor_format=fmt)
        assert _same_bits(x, fmt.convert(u8)), (kind, dtype, cl)
        assert _equal_nan(a2, a) and _equal_nan(b2, b) and torch.equal(status2, status)
    if kind == "macenko":                                     # the median mode takes the same fused pass
        sm = SlideNormalizer(nrm, group=False, mode="median")
        fmt = _fmt(*CLASS_FORMATS[0])
        m8, Mm, cm, stm = sm.transform_shard(dev)
        xm, Mm2, cm2, stm2 = sm.transform_shard(dev, tensor_format=fmt)
        assert _same_bits(xm, fmt.convert(m8)) and _equal_nan(Mm2, Mm) and _equal_nan(cm2, cm) and torch.equal(stm2, stm)


def test_slide_luminosity_standardize():
    from stainlib_amd.distributed import slide_luminosity_standardize
    dev = to_dev([so.synth_tile(61, 67, 900 + i) for i in range(3)])
    u8, p = slide_luminosity_standardize(dev, percentile=90, group=False)
    for dtype, cl, name in CLASS_FORMATS:
        fmt = _fmt(dtype, cl, name)
        x, p2 = slide_luminosity_standardize(dev, percentile=90, group=False, tensor_format=fmt)
        assert _same_bits(x, fmt.convert(u8)) and p2 == p


def test_graph_with_tensor_format_raises():
    from stainlib_amd.distributed import SlideNormalizer
    nrm = stainlib_amd.MacenkoNormalizer()
    nrm.fit(_target_tile())
    sn = SlideNormalizer(nrm, group=False, mode="pooled", graph=True)
    with pytest.raises(ValueError):
        sn.transform_shard(to_dev([so.synth_tile(96, 128, 50)]), tensor_format=stainlib_amd.TensorFormat())

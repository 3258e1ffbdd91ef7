"""The stain separation in the view pass (sl_stain_separate_view, engine.stain_separate_view, separate_batch(view=, windows=,
tensor_format=)) on the host side: the export and its binding, and every bad argument refused before anything is launched, drawn or
sent to the device -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1
NAME = "sl_stain_separate_view"
# device pointers: never read by the host side
RGB, O1, O2, O3, CONC, D6, D2, WIN = 0x100000, 0x200000, 0x210000, 0x220000, 0x230000, 0x300000, 0x300100, 0x400000
N, H, W, OH, OW = 4, 64, 48, 32, 24


def _full(conc=True):
    """a complete request: every refusal below is its own"""
    o = _ffi.default_separate_out()
    o.norm, o.stain[0], o.stain[1], o.conc = O1, O2, O3, (CONC if conc else None)
    return o


def _fmt(dtype=_ffi.DTYPE_F16, layout=_ffi.LAYOUT_NCHW):
    f = _ffi.default_tensor_format()
    f.dtype, f.layout = dtype, layout
    return f


def _sv(rgb=RGB, n=N, h=H, w=W, oh=OH, ow=OW, win=WIN, d_mask=7, shrink=1, ms=D6, cs=D2, mt=D6, ct=D2, lam=0.01, outs="full", fmt=None):
    o = _full() if isinstance(outs, str) else outs
    return _ffi.lib().sl_stain_separate_view(rgb, n, h, w, oh, ow, win, d_mask, shrink, ms, cs, mt, ct, lam,
                                             C.byref(o) if o is not None else None, C.byref(fmt) if fmt is not None else None, None)


def _put(o, name, v):
    if name in ("h", "e"):
        o.stain["he".index(name)] = v
    else:
        setattr(o, name, v)


# ---- the export --------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_export():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert NAME in declared and NAME in _ffi.EXPORTS and declared == set(_ffi.EXPORTS)
    proto = re.search(r"^SL_API int sl_stain_separate_view\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    params = [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")]
    res, args = _ffi._SIGNATURES[NAME]
    assert res is C.c_int and len(params) == len(args) == 17
    kinds = {"int": C.c_int, "double": C.c_double}
    for p, a in zip(params, args):                               # parameter by parameter: a pointer, an int or the one double
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(_ffi.SlSeparateOut), C.POINTER(_ffi.SlTensorFormat)), p
            assert (a is C.POINTER(_ffi.SlSeparateOut)) == ("SlSeparateOut" in p) and (a is C.POINTER(_ffi.SlTensorFormat)) == ("SlTensorFormat" in p)
        else:
            assert a is kinds[p.split()[0]], p
    assert [p.split()[-1].lstrip("*") for p in params] == ["rgb", "n", "h", "w", "oh", "ow", "windows", "d_mask", "shrink", "M_src", "maxC_src",
                                                            "M_tgt", "maxC_tgt", "lasso_lambda", "outs", "fmt", "stream"]
    fn = getattr(_ffi.lib(), NAME)                               # the library exports it, bound with this signature
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_abi_version_and_struct_are_unchanged():
    assert _ffi.lib().sl_version() == 600 == _ffi.EXPECTED_VERSION
    assert C.sizeof(_ffi.SlSeparateOut) == 40 == _ffi.default_separate_out().struct_size
    assert C.sizeof(_ffi.SlTensorFormat) == _ffi.default_tensor_format().struct_size


# ---- SL_ERR_BADARG before anything is launched -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(rgb=None), dict(ms=None), dict(cs=None), dict(outs=None), dict(mt=None), dict(ct=None),
                                dict(n=0), dict(n=-1), dict(h=0), dict(w=-5), dict(h=65536, w=65536), dict(h=32768, w=32769),
                                dict(h=32768, w=32769, mt=None, ct=None)], ids=str)
@pytest.mark.parametrize("fmt", [None, "f16"])
def test_what_sl_stain_separate_refuses_of_pointers_targets_and_shapes(kw, fmt):
    assert _sv(fmt=_fmt() if fmt else None, **kw) == BADARG


@pytest.mark.parametrize("lam", [-0.5, -1e-300, float("nan"), float("-inf")])
def test_lasso_lambda_rule(lam):
    assert _sv(lam=lam) == BADARG and _sv(lam=lam, mt=None, ct=None, fmt=_fmt()) == BADARG


@pytest.mark.parametrize("size", [0, 32, 48, 16])
def test_struct_size_mismatch_is_refused(size):
    o = _full()
    o.struct_size = size
    assert _sv(outs=o) == BADARG and _sv(outs=o, mt=None, ct=None) == BADARG


@pytest.mark.parametrize("with_conc", [True, False])
@pytest.mark.parametrize("value", [-1, 3, 99, -2 ** 31, 2 ** 31 - 1])
def test_unknown_conc_dtype_is_refused(value, with_conc):
    o = _full(with_conc)
    o.conc_dtype = value
    assert _sv(outs=o) == BADARG


def test_no_output_is_refused():
    o = _ffi.default_separate_out()
    assert _sv(outs=o) == BADARG and _sv(outs=o, mt=None, ct=None) == BADARG and _sv(outs=o, shrink=2, oh=8, ow=8, fmt=_fmt()) == BADARG


@pytest.mark.parametrize("kw", [dict(win=None), dict(oh=0), dict(ow=0), dict(oh=-1), dict(oh=H + 1, d_mask=6), dict(ow=W + 1, d_mask=6),
                                dict(oh=H, ow=W), dict(oh=49, ow=48, d_mask=1), dict(d_mask=-1), dict(d_mask=8),
                                dict(shrink=0), dict(shrink=3), dict(shrink=8), dict(shrink=-2),
                                dict(shrink=2, oh=33, d_mask=6), dict(shrink=2, ow=25, d_mask=6), dict(shrink=4, oh=17, ow=12, d_mask=6),
                                dict(shrink=2), dict(shrink=4, oh=16, ow=13),
                                dict(n=2 ** 31 - 1, h=128, w=128, oh=65, ow=65)], ids=str)
def test_what_view_geometry_refuses(kw):
    """size, d_mask, shrink not in {1, 2, 4}, NULL windows, too many (tile, patch) pairs -- on a request without planes, so that a legal
    shrink would pass"""
    assert _sv(outs=_full(conc=False), **kw) == BADARG
    assert _sv(outs=_full(conc=False), fmt=_fmt(_ffi.DTYPE_F32, _ffi.LAYOUT_NHWC), **kw) == BADARG


@pytest.mark.parametrize("shrink,oh,ow", [(2, 16, 12), (4, 8, 8), (2, 1, 1)])
def test_a_shrink_with_planes_is_refused(shrink, oh, ow):
    assert _sv(shrink=shrink, oh=oh, ow=ow) == BADARG and _sv(shrink=shrink, oh=oh, ow=ow, fmt=_fmt()) == BADARG
    o = _ffi.default_separate_out()
    o.conc = CONC
    assert _sv(shrink=shrink, oh=oh, ow=ow, outs=o, mt=None, ct=None) == BADARG


def _bad_formats():
    def mk(**kw):
        f = _fmt()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(f, k)[v[0]] = v[1]
            else:
                setattr(f, k, v)
        return f
    return [mk(struct_size=0), mk(struct_size=C.sizeof(_ffi.SlTensorFormat) + 8), mk(struct_size=16), mk(dtype=-1), mk(dtype=3),
            mk(layout=2), mk(layout=-1), mk(std=(1, 0.0)), mk(std=(2, -1.0)), mk(std=(0, float("nan"))), mk(std=(0, float("inf"))),
            mk(mean=(0, float("inf"))), mk(mean=(2, float("nan")))]


@pytest.mark.parametrize("i", range(13))
def test_a_bad_format_is_refused(i):
    f = _bad_formats()[i]
    assert _sv(fmt=f) == BADARG and _sv(fmt=f, outs=_full(conc=False), shrink=2, oh=8, ow=8) == BADARG


@pytest.mark.parametrize("name", ["norm", "h", "e"])
@pytest.mark.parametrize("dtype,off", [(_ffi.DTYPE_F32, 1), (_ffi.DTYPE_F32, 2), (_ffi.DTYPE_F32, 3), (_ffi.DTYPE_F16, 1), (_ffi.DTYPE_BF16, 1),
                                       (_ffi.DTYPE_F16, 3)])
def test_an_image_pointer_not_aligned_to_its_element_is_refused(name, dtype, off):
    o = _full()
    _put(o, name, 0x500000 + off)
    assert _sv(outs=o, fmt=_fmt(dtype)) == BADARG and _sv(outs=o, fmt=_fmt(dtype, _ffi.LAYOUT_NHWC)) == BADARG
    o = _ffi.default_separate_out()
    _put(o, name, 0x500000 + off)
    assert _sv(outs=o, fmt=_fmt(dtype), shrink=2, oh=8, ow=8) == BADARG


@pytest.mark.parametrize("dtype,off", [(_ffi.DTYPE_F16, 1), (_ffi.DTYPE_BF16, 1), (_ffi.DTYPE_F32, 1), (_ffi.DTYPE_F32, 2)])
def test_misaligned_conc_is_refused(dtype, off):
    o = _full()
    o.conc_dtype, o.conc = dtype, CONC + off
    assert _sv(outs=o) == BADARG and _sv(outs=o, fmt=_fmt()) == BADARG


@pytest.mark.parametrize("a,b", [("norm", "h"), ("norm", "e"), ("h", "e"), ("norm", "conc"), ("h", "conc"), ("e", "conc")])
@pytest.mark.parametrize("fmt", [None, "f32"])
def test_aliased_outputs_and_an_output_at_the_input_are_refused(a, b, fmt):
    f = _fmt(_ffi.DTYPE_F32) if fmt else None
    o = _full()
    _put(o, a, 0x500000)
    _put(o, b, 0x500000)
    assert _sv(outs=o, fmt=f) == BADARG
    for name in (a, b):
        o = _full()
        _put(o, name, RGB)
        assert _sv(outs=o, fmt=f) == BADARG
        o = _ffi.default_separate_out()
        _put(o, name, RGB)
        assert _sv(outs=o, fmt=f) == BADARG


# ---- the Python surface: ValueError before the device is touched and before anything is drawn (the tiles are CPU tensors: reaching the
# tile check would raise ValueError too, so every case matches on its own message) ---------------------------------------------------------
_TILES = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
_M, _MC = torch.zeros((2, 2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.float64)
_WIN = np.array([[0, 0, 0], [1, 2, 6]], dtype=np.int32)
_W0 = np.zeros((2, 3), dtype=np.int32)
_TILE_CHECK = "expected a contiguous CUDA uint8 tensor"
TV = stainlib_amd.TileView
F16 = stainlib_amd.TensorFormat(dtype=torch.float16)


def _undrawn(call, match):
    """call() raises ValueError(match) and takes nothing from the global numpy stream"""
    np.random.seed(11)
    with pytest.raises(ValueError, match=match):
        call()
    after = np.random.uniform()
    np.random.seed(11)
    assert np.random.uniform() == after


def _fitted():
    nz = stainlib_amd.MacenkoNormalizer()
    nz.stain_matrix_target = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
    nz.maxC_target = np.array([[1.9, 1.0]])
    return nz


@pytest.mark.parametrize("nz", [stainlib_amd.MacenkoNormalizer, stainlib_amd.VahadaneNormalizer])
def test_separate_batch_value_errors_name_their_cause_and_draw_nothing(nz):
    nz = nz()
    kw = dict(normalize=False)
    _undrawn(lambda: nz.separate_batch(_TILES, windows=_WIN, **kw), r"windows= goes with view=")
    _undrawn(lambda: nz.separate_batch(_TILES, tensor_format=F16, **kw),
             r"tensor_format= goes with view=.*TileView\(None, flip=False, rot90=False\)")
    for w in (None, np.array([[0, 0, 0, 4, 4], [0, 0, 0, 4, 4]], dtype=np.int32)):
        _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4, scale=(0.5, 1)), windows=w, **kw),
                 r"resizing view \(TileView\(.*scale=\(0\.5, 1\.0\).*separate_batch.*convert\(view=\)")
    for s in (2, 4):
        for want in (("norm", "h", "e", "conc"), ("conc",), "conc", ("h", "conc")):
            _undrawn(lambda: nz.separate_batch(_TILES, want=want, view=TV(2, shrink=s), **kw), rf"shrink={s} does not go with 'conc'")
        _undrawn(lambda: nz.separate_batch(_TILES, view=TV(2, shrink=s), windows=_W0, **kw), rf"shrink={s} does not go with 'conc'")
    # what the shared helpers refuse, each behind the new arguments
    _undrawn(lambda: nz.separate_batch(_TILES, view="x", **kw), "view must be a stainlib_amd.TileView")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(9), **kw), "does not fit")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV((4, 10)), **kw), "quarter turn")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4), windows=_WIN[:1], **kw), "windows must hold")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4), windows=np.array([[5, 0, 0], [0, 0, 0]]), **kw), "outside the 8 x 12 tile")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4, rot90=False), windows=np.array([[0, 0, 1], [0, 0, 0]]), **kw), "outside d_mask")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4), tensor_format="f16", **kw), "fmt must be a stainlib_amd.TensorFormat")
    _undrawn(lambda: nz.separate_batch(_TILES, want=("rgb",), view=TV(4), **kw), "want must")
    _undrawn(lambda: nz.separate_batch(_TILES, conc_dtype=torch.float64, view=TV(4), **kw), "conc_dtype must")
    _undrawn(lambda: nz.separate_batch(_TILES, view=TV(4)), "needs a fitted target")
    # every check passed: on to the tile check, still without a draw (the draw comes behind the fit)
    for view_kw in (dict(view=TV(4)), dict(view=TV(4), windows=_WIN), dict(view=TV(2, shrink=2), want=("norm", "h", "e")),
                    dict(view=TV(4), tensor_format=F16), dict(view=TV(None, flip=False, rot90=False), tensor_format=F16)):
        _undrawn(lambda: nz.separate_batch(_TILES, **view_kw, **kw), _TILE_CHECK)
        _undrawn(lambda: _fitted().separate_batch(_TILES, **view_kw), _TILE_CHECK)


def test_engine_value_errors_come_in_normalize_views_order_before_the_device():
    sv = engine.stain_separate_view
    S = engine.Separated
    for call, match in (
            (lambda: sv(_TILES[0], _WIN, 4, _M, _MC), _TILE_CHECK),
            (lambda: sv(_TILES, _WIN, 9, _M, _MC), "does not fit"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, d_mask=8), "d_mask must be"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, shrink=3), "shrink must be 1, 2 or 4"),
            (lambda: sv(_TILES, _WIN, (2, 5), _M, _MC, shrink=2, want="h"), "quarter turn"),
            (lambda: sv(_TILES, None, 4, _M, _MC), "windows must hold"),
            (lambda: sv(_TILES, _WIN[:1], 4, _M, _MC), "windows must hold"),
            (lambda: sv(_TILES, np.array([[0, 9, 0], [0, 0, 0]]), 4, _M, _MC), "outside the 8 x 12 tile"),
            (lambda: sv(_TILES, np.array([[0, 5, 0], [0, 0, 0]]), 2, _M, _MC, shrink=4, d_mask=6, want="norm"), "outside the 8 x 12 tile"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, d_mask=2), "outside d_mask"),
            (lambda: sv(_TILES, _WIN, 4, None, _MC), "M_src and maxC_src are needed"),
            (lambda: sv(_TILES, _WIN, 4, _M, None), "M_src and maxC_src are needed"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, M_tgt=_M[0]), "go together"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, maxC_tgt=_MC[0]), "go together"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, want=()), "want must"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, conc_dtype=torch.int32), "conc_dtype must"),
            (lambda: sv(_TILES, _WIN, 2, _M, _MC, shrink=2), "shrink=2 does not go with 'conc'"),
            (lambda: sv(_TILES, _W0, 2, _M, _MC, shrink=4, d_mask=6, want=("e", "conc")), "shrink=4 does not go with 'conc'"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, fmt="NCHW"), "fmt must be a stainlib_amd.TensorFormat"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, out=(None, None)), "out must be"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, want="h", out=S(norm=torch.zeros(1, dtype=torch.uint8))), "out.norm is given"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, out=S(norm=torch.zeros(1))), "out.norm must be a torch.uint8"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, fmt=F16, out=S(h=torch.zeros(1, dtype=torch.uint8))), "out.h must be a torch.float16"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC, fmt=F16, out=S(conc=torch.zeros(1, dtype=torch.float16))), "out.conc must be a torch.float32"),
            (lambda: sv(_TILES, _WIN, 4, _M, _MC), _TILE_CHECK),
            (lambda: sv(_TILES, _WIN, 2, _M, _MC, shrink=2, want=("norm", "h", "e"), fmt=F16), _TILE_CHECK)):
        _undrawn(call, match)


def test_separate_batch_without_the_new_arguments_is_the_call_it_was(monkeypatch):
    """same route (engine.stain_separate, never the view call), same four-element return"""
    seen = []
    nz = _fitted()
    monkeypatch.setattr(nz, "_fit_tiles", lambda tiles, ws=None: ("M", "maxC", "status"))
    monkeypatch.setattr(nz, "_target_on", lambda device: ("Mt", "ct"))
    monkeypatch.setattr(engine, "stain_separate", lambda *a, **k: seen.append((a, k)) or "sep")
    monkeypatch.setattr(engine, "stain_separate_view", lambda *a, **k: pytest.fail("the view call"))
    assert nz.separate_batch(_TILES) == ("sep", "M", "maxC", "status")
    assert nz.separate_batch(_TILES, ("h",), torch.float16, False, None) == ("sep", "M", "maxC", "status")
    assert seen[0] == ((_TILES, "M", "maxC", "Mt", "ct"), dict(want=("norm", "h", "e", "conc"), conc_dtype=torch.float32))
    assert seen[1] == ((_TILES, "M", "maxC", None, None), dict(want=("h",), conc_dtype=torch.float16))


def test_c_abi_argument_checks_of_the_entry_point_under_asan():
    """`make asan-sepview`: tests/abi_argcheck_sepview.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the entry point, among them callers' structs smaller than this header's at the end of
    their heap blocks.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-sepview", "-j8"], capture_output=True, text=True,
                       timeout=1800)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail

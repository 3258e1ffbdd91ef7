"""Companion planes through the windows of a view (sl_view_planes, engine.view_planes, TileView.apply) on the host side: the export and
its binding, the numpy restatement of the definition on hand-written values, every bad argument refused before the library is called
and without a draw, the C argument checks under AddressSanitizer, and the kernel's lane-to-address arithmetic lane by lane on the CPU
-- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stainlib_amd
from stainlib_amd import _ffi, engine, tile_view
from stainlib_amd.tile_view import area_resample, nearest_index, nearest_resample, view_planes_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "sl_view_planes"
TV = stainlib_amd.TileView


# ---- 1. the export -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_export():
    hdr = open(os.path.join(REPO, "include", "stainlib_hip.h")).read()
    declared = set(re.findall(r"^SL_API (?:int|size_t|void|const char\*)\s+(sl_\w+)\(", hdr, flags=re.M))
    assert NAME in declared and NAME in _ffi.EXPORTS and declared == set(_ffi.EXPORTS)
    proto = re.search(r"^SL_API int sl_view_planes\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    params = [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")]
    res, args = _ffi._SIGNATURES[NAME]
    assert res is C.c_int and len(params) == len(args) == 16
    for p, a in zip(params, args):                               # parameter by parameter: a pointer or an int
        assert a is (C.c_void_p if "*" in p else C.c_int), p
        assert "*" in p or p.split()[0] == "int", p
    assert [p.split()[-1].lstrip("*") for p in params] == ["planes", "out", "n", "c", "h", "w", "elem_bytes", "oh", "ow", "windows", "d_mask",
                                                            "shrink", "max_wh", "max_ww", "mode", "stream"]
    assert re.search(r"^#define SL_PLANES_NEAREST\s+0$", hdr, flags=re.M) and re.search(r"^#define SL_PLANES_AREA\s+1$", hdr, flags=re.M)
    assert (_ffi.PLANES_NEAREST, _ffi.PLANES_AREA) == (0, 1)
    fn = getattr(_ffi.lib(), NAME)                               # the library exports it, bound with this signature
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert _ffi.lib().sl_version() == 600 == _ffi.EXPECTED_VERSION


def test_the_library_refuses_bad_calls_before_a_launch():
    """a few of the refusals through the binding (the whole list: the AddressSanitizer driver below); the pointers are never read"""
    f = _ffi.lib().sl_view_planes
    good = [0x100000, 0x200000, 4, 3, 64, 48, 2, 8, 8, 0x300000, 7, 1, 0, 0, 0, None]
    for i, v in ((0, None), (1, None), (9, None), (2, 0), (3, -1), (6, 3), (0, 0x100001), (14, 2), (14, 1), (12, 8), (11, 3), (10, 8), (7, 49)):
        a = list(good)
        a[i] = v
        assert f(*a) == -1, (i, v)


# ---- 2. / 3. the centre sample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,no,want", [(5, 5, [0, 1, 2, 3, 4]), (10, 5, [1, 3, 5, 7, 9]), (20, 5, [2, 6, 10, 14, 18]),
                                        (3, 7, [0, 0, 1, 1, 1, 2, 2]), (16, 1, [8])])
def test_nearest_index_on_hand_written_values(nw, no, want):
    k = nearest_index(nw, no)
    assert k.dtype == np.int64 and k.tolist() == want


def test_the_centre_sample_does_not_commute_with_a_reversal():
    """nw = 10, no = 5: sampling the row and reversing gives 9 7 5 3 1; reversing the row and sampling would give 8 6 4 2 0.  The
    definition is the first: resample in the tile's orientation, THEN flip."""
    row = np.arange(10, dtype=np.int16)[None, :]
    sampled = nearest_resample(row, 1, 5)
    assert sampled.tolist() == [[1, 3, 5, 7, 9]]
    assert sampled[:, ::-1].tolist() == [[9, 7, 5, 3, 1]]
    assert nearest_resample(row[:, ::-1], 1, 5).tolist() == [[8, 6, 4, 2, 0]]
    planes = np.tile(np.arange(10, dtype=np.int16), (2, 1))[None]              # (1, 2, 10): both rows 0 .. 9
    assert view_planes_reference(planes, [[0, 0, 4]], (1, 5), shrink=2).tolist() == [[[9, 7, 5, 3, 1]]]                 # a flip
    assert view_planes_reference(planes, [[0, 0, 4, 1, 10]], (1, 5)).tolist() == [[[9, 7, 5, 3, 1]]]                    # the resizing row
    got = view_planes_reference(np.arange(20, dtype=np.int16).reshape(1, 2, 10), [[0, 0, 1]], (5, 1), shrink=2)         # a quarter turn
    assert got.tolist() == [[[19], [17], [15], [13], [11]]]                      # row s / 2 = 1 of the window, its centres, turned


# ---- 4. the area mode of the restatement ---------------------------------------------------------------------------------------------------
def test_area_mode_of_the_restatement_is_area_resample_per_plane():
    rng = np.random.RandomState(5)
    x = rng.randint(0, 256, size=(3, 2, 23, 31)).astype(np.uint8)
    win = np.array([[2, 3, 0, 16, 20], [0, 0, 5, 21, 9], [1, 4, 6, 5, 7]], dtype=np.int32)
    got = view_planes_reference(x, win, (8, 10), mode="area")
    for t in range(3):
        y0, x0, d, wh, ww = (int(v) for v in win[t])
        nu, nv = (10, 8) if d & 1 else (8, 10)
        for c in range(2):
            r = area_resample(x[t, c, y0:y0 + wh, x0:x0 + ww][..., None], nu, nv)[..., 0]
            assert np.array_equal(got[t, c], np.rot90(r[:, ::-1] if d & 4 else r, d & 3))
    # under a shrink it is the images' box mean
    w3 = np.array([[1, 2, 0], [0, 0, 7], [3, 3, 6]], dtype=np.int32)
    got = view_planes_reference(x[:, 0], w3, (5, 4), shrink=4, mode="area")
    for t in range(3):
        y0, x0, d = (int(v) for v in w3[t])
        nu, nv = (4, 5) if d & 1 else (5, 4)
        box = x[t, 0, y0:y0 + 4 * nu, x0:x0 + 4 * nv].astype(np.int64).reshape(nu, 4, nv, 4).sum(axis=(1, 3))
        r = ((box + 8) >> 4).astype(np.uint8)
        assert np.array_equal(got[t], np.rot90(r[:, ::-1] if d & 4 else r, d & 3))
    with pytest.raises(ValueError, match="uint8"):
        view_planes_reference(x.astype(np.int16), win, (8, 10), mode="area")


# ---- 5. every ValueError before the library is called, nothing drawn -------------------------------------------------------------------------
_PL = torch.zeros((2, 8, 12), dtype=torch.int64)                  # CPU planes: every case below is refused on its own message first
_WIN = np.array([[0, 0, 0], [1, 2, 6]], dtype=np.int32)
_WIN5 = np.array([[0, 0, 0, 4, 4], [1, 2, 6, 5, 7]], dtype=np.int32)


@pytest.fixture
def no_library(monkeypatch):
    """the library is not called: any sl_* call through the binding fails the test"""
    monkeypatch.setattr(engine, "_call", lambda name, *a: pytest.fail(f"{name} was called"))


def _undrawn(call, match):
    """call() raises ValueError(match) and leaves the global numpy stream as it was"""
    np.random.seed(11)
    before = np.random.get_state()
    with pytest.raises(ValueError, match=match):
        call()
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_apply_value_errors_name_their_cause_and_draw_nothing(no_library):
    v = TV(4)
    _undrawn(lambda: v.apply(_PL), r"windows is required.*image call.*view\.draw")
    _undrawn(lambda: v.apply(_PL, None), r"windows is required")
    _undrawn(lambda: v.apply(_PL, _WIN), "not a CPU tensor")
    _undrawn(lambda: v.apply(_PL[:, :, ::2], _WIN), "CPU tensor")
    _undrawn(lambda: v.apply(_PL[0], _WIN), r"shape \(N, H, W\) or \(N, C, H, W\), not one of rank 2")
    _undrawn(lambda: v.apply(_PL[None, None], _WIN), "not one of rank 5")
    _undrawn(lambda: v.apply(_PL.numpy(), _WIN), r"shape \(N, H, W\) or \(N, C, H, W\)")
    _undrawn(lambda: v.apply(_PL.to(torch.complex64), _WIN), "complex64 are not supported")
    _undrawn(lambda: v.apply(_PL.to(torch.complex128), _WIN), "complex128 are not supported")
    _undrawn(lambda: v.apply(_PL, _WIN, mode="area"), "mode='area'.*uint8 planes only, not torch.int64")
    _undrawn(lambda: v.apply(_PL.to(torch.int8), _WIN, mode="area"), "uint8 planes only, not torch.int8")
    _undrawn(lambda: v.apply(_PL, _WIN, mode="bilinear"), "mode must be 'nearest' or 'area', not 'bilinear'")
    _undrawn(lambda: v.apply(_PL, _WIN, mode=0), "mode must be")
    # what the image calls refuse of the size and of host windows, in their words
    _undrawn(lambda: TV(9).apply(_PL, _WIN), "does not fit")
    _undrawn(lambda: TV((4, 10)).apply(_PL, _WIN), "quarter turn")
    _undrawn(lambda: TV(8, shrink=2).apply(_PL, _WIN), r"shrink=2 \(a 16 x 16 window\) does not fit")
    _undrawn(lambda: v.apply(_PL, _WIN[:1]), "windows must hold")
    _undrawn(lambda: v.apply(_PL, _WIN5), "windows must hold")
    _undrawn(lambda: v.apply(_PL, _WIN.astype(np.float32)), "windows must hold")
    _undrawn(lambda: v.apply(_PL, np.array([[5, 0, 0], [0, 0, 0]])), "outside the 8 x 12 tile")
    _undrawn(lambda: TV(2, shrink=4).apply(_PL, np.array([[1, 0, 0], [0, 0, 0]])), "outside the 8 x 12 tile")
    _undrawn(lambda: TV(4, rot90=False).apply(_PL, np.array([[0, 0, 1], [0, 0, 0]])), "outside d_mask")
    rv = TV(4, scale=(0.5, 1))
    _undrawn(lambda: rv.apply(_PL, _WIN), "resizing view must hold")
    _undrawn(lambda: rv.apply(_PL, np.array([[0, 0, 0, 9, 4], [0, 0, 0, 4, 4]])), r"has a 9 x 4 window, outside 1 x 1")
    _undrawn(lambda: rv.apply(_PL, np.array([[5, 0, 0, 4, 4], [0, 0, 0, 4, 4]])), "outside the 8 x 12 tile")
    # every check without a device passed: on to the planes themselves, still without a draw
    for view, win in ((v, _WIN), (TV(2, shrink=2), _WIN), (rv, _WIN5), (TV(None, flip=False, rot90=False), np.zeros((2, 3), dtype=np.int32))):
        _undrawn(lambda: view.apply(_PL, win), "not a CPU tensor")
        _undrawn(lambda: view.apply(_PL[:, None].to(torch.uint8), win, mode="area"), "not a CPU tensor")


def test_engine_value_errors_come_before_the_library(no_library):
    vp = engine.view_planes
    for call, match in (
            (lambda: vp(_PL[0], _WIN, 4), "not one of rank 2"),
            (lambda: vp("x", _WIN, 4), r"shape \(N, H, W\) or \(N, C, H, W\)"),
            (lambda: vp(_PL.to(torch.complex64), _WIN, 4), "not supported"),
            (lambda: vp(_PL, _WIN, 4, mode="mode"), "mode must be"),
            (lambda: vp(_PL, _WIN, 4, mode="area"), "uint8 planes only"),
            (lambda: vp(_PL, _WIN, 9), "does not fit"),
            (lambda: vp(_PL, _WIN, 4, d_mask=8), "d_mask must be"),
            (lambda: vp(_PL, _WIN, 4, shrink=3), "shrink must be 1, 2 or 4"),
            (lambda: vp(_PL, _WIN, (2, 5), shrink=2), "quarter turn"),
            (lambda: vp(_PL, None, 4), "windows must hold"),
            (lambda: vp(_PL, _WIN, 4, d_mask=2), "outside d_mask"),
            (lambda: vp(_PL, _WIN5, 4, resize=(8, 13)), r"resize = \(8, 13\) must lie within"),
            (lambda: vp(_PL, _WIN5, 4, resize=(8, 12), shrink=2), "does not go with shrink=2"),
            (lambda: vp(_PL, _WIN5, 4, resize=8), "resize must be None or"),
            (lambda: vp(_PL, _WIN, 4, resize=(8, 12)), "resizing view must hold"),
            (lambda: vp(_PL, _WIN5, 4, resize=(4, 12)), "has a 5 x 7 window"),
            (lambda: vp(_PL, _WIN, 4), "not a CPU tensor"),
            (lambda: vp(_PL, _WIN5, 4, resize=(8, 12)), "not a CPU tensor"),
            (lambda: vp(_PL, _WIN, 4, out=torch.zeros((2, 4, 4), dtype=torch.int64)), "not a CPU tensor")):
        _undrawn(call, match)


def test_out_and_layout_are_checked_before_the_library(no_library, monkeypatch):
    """the checks behind the CPU refusal, on tensors that only CLAIM to live on the device"""
    class Dev(torch.Tensor):
        is_cuda = True
    pl = torch.zeros((2, 3, 8, 12), dtype=torch.int16).as_subclass(Dev)
    _undrawn(lambda: engine.view_planes(pl.transpose(2, 3), _WIN, 2), "not contiguous")
    _undrawn(lambda: engine.view_planes(pl, _WIN, 4, out=torch.zeros((2, 3, 4, 5), dtype=torch.int16)), r"out must be a contiguous torch.int16 tensor of shape \(2, 3, 4, 4\)")
    _undrawn(lambda: engine.view_planes(pl, _WIN, 4, out=torch.zeros((2, 3, 4, 4), dtype=torch.int32)), "out must be a contiguous torch.int16")
    _undrawn(lambda: engine.view_planes(pl, _WIN, 4, out=torch.zeros((2, 3, 4, 4), dtype=torch.int16, device="meta")), "out must be a contiguous")
    _undrawn(lambda: engine.view_planes(pl, _WIN, 4, out="x"), "out must be a contiguous")
    _undrawn(lambda: engine.view_planes(pl, np.zeros((2, 3), dtype=np.int32), (8, 12), d_mask=6, out=pl), "must not be planes itself")


def test_apply_hands_the_image_calls_arguments_on(monkeypatch):
    """size, d_mask, shrink and the resize bound are the ones the image call of the same view and windows gets"""
    seen = []
    monkeypatch.setattr(engine, "view_planes", lambda *a, **k: seen.append((a, k)) or "out")
    tiles = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
    for v, win in ((TV(4), _WIN), (TV(2, shrink=2, rot90=False), _WIN), (TV(4, scale=(0.5, 1)), _WIN5), (TV(4, scale=(0.5, 1), flip=False), None)):
        seen.clear()
        if win is None:
            win = torch.zeros((2, 5), dtype=torch.int32).as_subclass(type("Dev", (torch.Tensor,), {"is_cuda": True}))
        assert v.apply(_PL, win, mode="area", out="o") == "out"
        (a, k), = seen
        assert a == (_PL, win, v.size, v.d_mask) and k == dict(mode="area", out="o", shrink=v.shrink, resize=engine._view_resize(v, win, tiles))
    assert k["resize"] == TV(4, scale=(0.5, 1), flip=False).window_bound(8, 12)


# ---- 6. the C argument checks under AddressSanitizer -----------------------------------------------------------------------------------------
def test_c_abi_argument_checks_of_the_entry_point_under_asan():
    """`make asan-planes`: tests/abi_argcheck_planes.c -- a stand-alone program -- against the library's HOST side built with
    AddressSanitizer: every refused call of the entry point.  Nothing is launched: no GPU needed.  (Builds the sanitizer library if
    nothing has yet: a few minutes.)"""
    r = subprocess.run(["make", "-C", os.path.join(REPO, "stainlib_amd", "csrc"), "asan-planes", "-j8"], capture_output=True, text=True,
                       timeout=1800)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert re.search(r"^OK: \d+ checks, 0 failed$", r.stdout, flags=re.M), tail
    assert "AddressSanitizer" not in r.stdout + r.stderr, tail


# ---- 7. the kernel's lane-to-address arithmetic, lane by lane, under the host sanitizers ------------------------------------------------------
def _host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_lane_to_address_arithmetic_stays_inside_the_buffers_and_follows_the_definition(tmp_path):
    """tests/planes_view_geometry.cpp, a stand-alone program: planes_view_geometry.hpp for every lane of every workgroup on byte
    buffers of exactly the input's and the output's size -- every output element written once, from the element the definition names."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "planes_view_geometry")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", os.path.join(HERE, "planes_view_geometry.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"^\d+ cases, \d+ output elements checked, 0 failures$", r.stdout, flags=re.M)
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

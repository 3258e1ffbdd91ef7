"""Batched device-level operators: torch uint8 NHWC tensors in HBM -> the C ABI.

PyTorch is plumbing here (device memory, streams); every computation is a call into
``libstainlib_hip.so``.  All functions enqueue on torch's current stream and return
device tensors without synchronising.
"""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import _ffi
from .separated import Separated


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _params(params):
    """ctypes reference to the caller's SlParams, or to the defaults when params is None."""
    return C.byref(params if params is not None else _ffi.default_params())


def _byref(struct):
    """ctypes reference to an optional SlParams / SlTensorFormat: NULL for None."""
    return C.byref(struct) if struct is not None else None


def _call(name, *args):
    """lib().<name>(*args, current stream); an error code raises StainlibHipError("<name> failed: ...")."""
    _ffi.check(getattr(_ffi.lib(), name)(*args, _stream()), name)


def _check_tiles(rgb: torch.Tensor):
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4
            and rgb.shape[-1] == 3 and rgb.is_contiguous()):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w, _ = rgb.shape
    return n, h, w


def _f64(x, shape, device):
    if not isinstance(x, torch.Tensor):
        import numpy as np
        x = np.asarray(x, dtype=np.float64)
    t = torch.as_tensor(x, dtype=torch.float64, device=device).reshape(shape)
    return t.contiguous()


def _route_upload(n, device, M_src, maxC_src, M_tgt=None, maxC_tgt=None, alpha_beta=None):
    """The statistics of an apply-pass route as device float64 tensors of the shapes the C ABI reads, None staying None ->
    (M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)."""
    def up(x, shape):
        return _f64(x, shape, device) if x is not None else None
    return up(M_src, (n, 2, 3)), up(maxC_src, (n, 2)), up(M_tgt, (2, 3)), up(maxC_tgt, (2,)), up(alpha_beta, (n, 4))


def make_params(**kw) -> _ffi.SlParams:
    p = _ffi.default_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def attach_fallbacks(params: _ffi.SlParams, n: int, device="cuda") -> torch.Tensor:
    """Give ``params`` a device buffer of n int32 that sl_macenko_* / sl_vahadane_* fill with the per-tile count of order
    statistics that needed the slow exact selection (SlParams.fallbacks_out; diagnostics only).  Returns the tensor --
    keep it alive as long as ``params`` is used."""
    t = torch.zeros((n,), dtype=torch.int32, device=device)
    params.fallbacks_out = t.data_ptr()
    return t


class Workspace:
    """Caller-owned scratch the library asks for via sl_workspace_bytes (grown on demand).

    One Workspace must only ever be in use on ONE stream at a time: the kernels of a call keep their per-tile state in it.
    Pass your own (``ws=``) to pin a buffer to a pipeline stage; without one every call takes a fresh block from torch's
    caching allocator, which is stream-ordered -- two streams or threads can then never share scratch."""

    def __init__(self):
        self.buf = None

    def get(self, op: int, n: int, h: int, w: int, device, params=None) -> torch.Tensor:
        need = _ws_need(op, n, h, w, params)
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            self.buf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        return self.buf


def _ws_need(op, n, h, w, params=None) -> int:
    """what THIS call needs (sl_workspace_bytes_for: the schedule its SlParams select), not the maximum over every SlParams"""
    return int(_ffi.lib().sl_workspace_bytes_for(op, n, h, w, _byref(params)))


def _scratch(ws, op, n, h, w, device, params=None) -> torch.Tensor:
    """The workspace of one call: the caller's Workspace, or a block of torch's caching allocator owned by the current
    stream for the duration of the call's kernels (freed blocks are reused on the same stream only after them)."""
    if ws is not None:
        return ws.get(op, n, h, w, device, params)
    need = _ws_need(op, n, h, w, params)
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


class Graphed:
    """A sequence of engine calls captured ONCE into a HIP graph and replayed.  Every fit / transform / apply / augment
    entry point of the C ABI is capture-safe -- kernel launches on the caller's stream, no allocation, no synchronisation,
    no host read-back; so is the one-sweep chain of the pooled slide mode on one process, which SlideNormalizer(graph=True)
    captures with the apply pass behind it.  What it buys is the
    LATENCY of an isolated small call on the one-launch-per-phase schedule (7 launches for Macenko, 11 for Vahadane), whose
    first kernels otherwise wait for the host to issue the next launch: 1024^2 Macenko transform, call-to-completion, 16
    tiles 274 -> 239 us, 128 tiles 671 -> 623 us.  Calls queued back to back gain nothing (the host already runs ahead
    of the device: 16 tiles 0.237 vs 0.235 ms per call).

        g = engine.Graphed(lambda: engine.macenko_transform(tiles, M_t, maxC_t, out=out, ws=ws))
        ...   # refill `tiles` in place (same tensors), then
        out, M, maxC, status = g.replay()

    fn must use only tensors that stay alive and in place (pass out= and ws=); it runs once for warm-up and once under
    capture.  replay() enqueues the graph on the current stream and returns what fn returned (the same tensors)."""

    def __init__(self, fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                     # warm-up outside the capture: workspace growth, lazy initialisation
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.result = fn()

    def replay(self):
        self.graph.replay()
        return self.result


def normalize_apply(rgb, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda=0.01, out=None, want_prequant=False):
    """OD + reconstruction pass (sl_normalize_apply).  Returns out, or (out, prequant)."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M_src, maxC_src, M_tgt, maxC_tgt, _ = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt)
    if out is None:
        out = torch.empty_like(rgb)
    pre = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if want_prequant else None
    _call("sl_normalize_apply", _ptr(rgb), _ptr(out), n, h, w, _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt),
          float(lasso_lambda), _ptr(pre))
    return (out, pre) if want_prequant else out


# ---- model-ready tensor output (sl_to_tensor / sl_normalize_apply_tensor; see SlTensorFormat in include/stainlib_hip.h) --------------
_TENSOR_DTYPES = {torch.float32: _ffi.DTYPE_F32, torch.float16: _ffi.DTYPE_F16, torch.bfloat16: _ffi.DTYPE_BF16}


def _tensor_format(fmt):
    """(SlTensorFormat, torch dtype, channels_last) of a stainlib_amd.TensorFormat."""
    f = _ffi.default_tensor_format()
    f.dtype = _TENSOR_DTYPES[fmt.dtype]
    f.layout = _ffi.LAYOUT_NHWC if fmt.channels_last else _ffi.LAYOUT_NCHW
    for c in range(3):
        f.mean[c] = float(fmt.mean[c])
        f.std[c] = float(fmt.std[c])
    return f, fmt.dtype, bool(fmt.channels_last)


def _tensor_out(out, n, h, w, dtype, channels_last, device):
    """The (N, 3, H, W) result tensor in the format's memory layout: the caller's, checked, or a fresh one."""
    if out is None:
        return torch.empty((n, 3, h, w), dtype=dtype, device=device,
                           memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    # (strides, not is_contiguous(memory_format=...): that test ignores the strides of size-1 dimensions, the kernel does not)
    want = (3 * h * w, 1, 3 * w, 3) if channels_last else (3 * h * w, h * w, w, 1)
    if not (isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == device and tuple(out.shape) == (n, 3, h, w)
            and tuple(out.stride()) == want):
        raise ValueError(f"out must be a {dtype} tensor of shape ({n}, 3, {h}, {w}) on {device} in "
                         f"{'channels_last' if channels_last else 'contiguous'} memory format")
    return out


def _image_out(out, rgb, n, h, w, fmt, what):
    """(SlTensorFormat or None, out) of a pass that writes n images of h x w from rgb: without a format the (n, h, w, 3) uint8 `out`,
    checked or fresh, and not the input (what: "jitter" / "view", for that message); else _tensor_out's."""
    dev = rgb.device
    if fmt is not None:
        f, dtype, cl = _tensor_format(fmt)
        return f, _tensor_out(out, n, h, w, dtype, cl, dev)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == dev and tuple(out.shape) == (n, h, w, 3)
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {(n, h, w, 3)} on {dev}")
    if out.data_ptr() == rgb.data_ptr():
        raise ValueError(f"out must not be the input (no in-place {what})")
    return None, out


def to_tensor(rgb, fmt, out=None):
    """(N,H,W,3) uint8 -> (N,3,H,W) tensor of fmt.dtype, contiguous or channels_last: fma(b, 1/(255 std), -mean/std) of every byte,
    rounded to nearest even (sl_to_tensor).  fmt: a stainlib_amd.TensorFormat."""
    n, h, w = _check_shard(rgb)
    f, dtype, cl = _tensor_format(fmt)
    out = _tensor_out(out, n, h, w, dtype, cl, rgb.device)
    if n == 0:                   # an empty shard of the slide modes
        return out
    _call("sl_to_tensor", _ptr(rgb), _ptr(out), n, h, w, C.byref(f))
    return out


def normalize_apply_tensor(rgb, M_src, maxC_src, M_tgt, maxC_tgt, fmt, lasso_lambda=0.01, out=None):
    """normalize_apply and to_tensor in one pass (sl_normalize_apply_tensor): equal to to_tensor(normalize_apply(...), fmt) bit for
    bit, without the uint8 image in between."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M_src, maxC_src, M_tgt, maxC_tgt, _ = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt)
    f, dtype, cl = _tensor_format(fmt)
    out = _tensor_out(out, n, h, w, dtype, cl, dev)
    _call("sl_normalize_apply_tensor", _ptr(rgb), _ptr(out), n, h, w, _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt),
          float(lasso_lambda), C.byref(f))
    return out


# ---- stain separation (sl_stain_separate; see SlSeparateOut in include/stainlib_hip.h) -------------------------------------------------

def _separate_want(want, conc_dtype):
    """The wanted outputs as a tuple of field names, checked (no device needed)."""
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        raise ValueError("want must be a sequence of 'norm', 'h', 'e', 'conc'") from None
    if not want or len(set(want)) != len(want) or any(not isinstance(k, str) or k not in Separated._fields for k in want):
        raise ValueError(f"want must name at least one of {Separated._fields}, each once; got {want!r}")
    if conc_dtype not in _TENSOR_DTYPES:
        raise ValueError("conc_dtype must be torch.float32, torch.float16 or torch.bfloat16")
    return want


def _separate_out_fields(out, want, conc_dtype, image_dtype=torch.uint8):
    """What can be said about `out` without the tiles (no device needed): its form, and per field presence and dtype (image_dtype: of the
    three images -- uint8, or the format's under stain_separate_view(fmt=))."""
    if out is None:
        return
    if not (isinstance(out, tuple) and len(out) == 4):
        raise ValueError("out must be an engine.Separated of caller buffers (None where the library allocates)")
    for name, t in zip(Separated._fields, out):
        if t is None:
            continue
        if name not in want:
            raise ValueError(f"out.{name} is given but {name!r} is not in want")
        dtype = conc_dtype if name == "conc" else image_dtype
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype):
            raise ValueError(f"out.{name} must be a {dtype} tensor")


def _separate_out(out, want, n, h, w, conc_dtype, device):
    """The four result tensors (None where not wanted): the caller's, checked, or fresh ones."""
    res = []
    for k, name in enumerate(Separated._fields):
        shape, dtype = ((n, 2, h, w), conc_dtype) if name == "conc" else ((n, h, w, 3), torch.uint8)
        t = out[k] if out is not None else None
        if name not in want:
            res.append(None)
        elif t is None:
            res.append(torch.empty(shape, dtype=dtype, device=device))
        elif not (t.device == device and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError(f"out.{name} must be a contiguous {dtype} tensor of shape {shape} on {device}")
        else:
            res.append(t)
    return Separated(*res)


def stain_separate(rgb, M_src, maxC_src, M_tgt=None, maxC_tgt=None, lasso_lambda=0.01, want=("norm", "h", "e", "conc"),
                   conc_dtype=torch.float32, out=None):
    """normalize_apply's pass with up to four outputs from one read and one lasso solve per pixel (sl_stain_separate) -> Separated:
    norm = normalize_apply's bytes; h / e = the image of one stain alone (normalize_apply with the other row of M_tgt zeroed);
    conc = the normalised concentrations C * maxC_tgt / maxC_src as (N,2,H,W) planes of conc_dtype.
    M_tgt=None (and maxC_tgt=None): no target -- every tile under its own M_src, conc = the raw get_concentrations."""
    want = _separate_want(want, conc_dtype)
    if (M_tgt is None) != (maxC_tgt is None):
        raise ValueError("M_tgt and maxC_tgt go together: both, or neither (no target)")
    _separate_out_fields(out, want, conc_dtype)
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    res = _separate_out(out, want, n, h, w, conc_dtype, dev)
    M_src, maxC_src, M_tgt, maxC_tgt, _ = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt)
    o = _ffi.default_separate_out()
    o.conc_dtype = _TENSOR_DTYPES[conc_dtype]
    o.norm, o.stain[0], o.stain[1], o.conc = (t.data_ptr() if t is not None else None for t in res)
    _call("sl_stain_separate", _ptr(rgb), n, h, w, _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), float(lasso_lambda), C.byref(o))
    return res


# ---- stain jitter in the apply pass (sl_normalize_jitter; see include/stainlib_hip.h) ---------------------------------------------------

def _jitter_args(M_tgt, maxC_tgt, alpha_beta, params, fmt, out):
    """What can be said about a normalize_jitter call without the tiles (no device needed)."""
    from .tensor_format import TensorFormat
    if (M_tgt is None) != (maxC_tgt is None):
        raise ValueError("M_tgt and maxC_tgt go together: both, or neither (no target)")
    if alpha_beta is None:
        raise ValueError("alpha_beta must hold (alpha0, beta0, alpha1, beta1) per tile: an (N, 4) array (StainJitter.draw)")
    if not isinstance(alpha_beta, torch.Tensor):
        import numpy as np
        try:
            shape = np.asarray(alpha_beta, dtype=np.float64).shape
        except (TypeError, ValueError):
            raise ValueError("alpha_beta must hold (alpha0, beta0, alpha1, beta1) per tile: an (N, 4) array") from None
    else:
        shape = tuple(alpha_beta.shape)
    if len(shape) != 2 or shape[1] != 4:
        raise ValueError(f"alpha_beta must hold (alpha0, beta0, alpha1, beta1) per tile: an (N, 4) array, not one of shape {shape}")
    if params is not None and not isinstance(params, _ffi.SlParams):
        raise ValueError("params must be an SlParams (engine.make_params) or None")
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    if out is not None:
        dtype = fmt.dtype if fmt is not None else torch.uint8
        if not (isinstance(out, torch.Tensor) and out.dtype == dtype):
            raise ValueError(f"out must be a {dtype} tensor")
    return shape[0]


def _route_check(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, n=None):
    """The checks of the arguments by which normalize_view, normalize_hed_view and normalize_sums name `full` -- the tiles' own bytes
    (M_src=None), normalize_apply's image (M_src and a target) or normalize_jitter's (alpha_beta) -- and of params (no device needed) ->
    the rows of alpha_beta, or None.  n: the rows alpha_beta must have."""
    if (M_tgt is None) != (maxC_tgt is None):
        raise ValueError("M_tgt and maxC_tgt go together: both, or neither (no target)")
    if M_src is None:
        if not (maxC_src is None and M_tgt is None and alpha_beta is None):
            raise ValueError("M_src=None is the view of the tiles' own bytes: maxC_src, M_tgt, maxC_tgt and alpha_beta must be None too")
    elif maxC_src is None:
        raise ValueError("M_src and maxC_src go together")
    elif alpha_beta is None and M_tgt is None:
        raise ValueError("without alpha_beta the view is normalize_apply's, which needs a target: pass M_tgt and maxC_tgt")
    n_ab = _jitter_args(M_tgt, maxC_tgt, alpha_beta, None, None, None) if alpha_beta is not None else None
    if n is not None and n_ab is not None and n_ab != n:
        raise ValueError(f"alpha_beta must have one row per tile ({n})")
    if params is not None and not isinstance(params, _ffi.SlParams):
        raise ValueError("params must be an SlParams (engine.make_params) or None")
    return n_ab


def normalize_jitter(rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background=False, params=None, fmt=None, out=None):
    """normalize_apply and StainAugmentor.pop's perturbation in ONE pass (sl_normalize_jitter): per tile C_i * alpha_i + beta_i on the
    NORMALISED concentrations C * maxC_tgt / maxC_src of tissue pixels (all pixels with augment_background), reconstructed under the
    target, clipped.  alpha_beta: (N, 4) = alpha0, beta0, alpha1, beta1 per tile (StainJitter.draw).
    M_tgt=None (and maxC_tgt=None): no target -- every tile under its own M_src: stain_augment's bytes.
    fmt: a stainlib_amd.TensorFormat -> the (N,3,H,W) tensor, bit for bit fmt.convert of the uint8 result; None -> (N,H,W,3) uint8.
    params: lasso_lambda and luminosity_threshold are read."""
    n_ab = _jitter_args(M_tgt, maxC_tgt, alpha_beta, params, fmt, out)
    n, h, w = _check_tiles(rgb)
    if n_ab != n:
        raise ValueError(f"alpha_beta has {n_ab} rows for {n} tiles")
    M_src, maxC_src, M_tgt, maxC_tgt, ab = _route_upload(n, rgb.device, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    f, out = _image_out(out, rgb, n, h, w, fmt, "jitter")
    _call("sl_normalize_jitter", _ptr(rgb), _ptr(out), n, h, w, _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab),
          1 if augment_background else 0, _byref(params), _byref(f))
    return out


# ---- crop / flip / rot90 in the apply pass (sl_normalize_view; see include/stainlib_hip.h and stainlib_amd/tile_view.py) -------------------

def _call_view(name, shrink, head, *tail, resize=None):
    """The C call of a view pass: `name` as it is at shrink = 1, else its `_shrink` export, which takes shrink behind d_mask (the last
    of head); with resize = (max_wh, max_ww) its `_resize` export, which takes those two there."""
    if resize is not None:
        _call(name + "_resize", *head, int(resize[0]), int(resize[1]), *tail)
    elif shrink == 1:
        _call(name, *head, *tail)
    else:
        _call(name + "_shrink", *head, int(shrink), *tail)


def _check_resize(resize, h, w, shrink=1):
    """resize= of normalize_view / normalize_hed_view as (max_wh, max_ww) ints, or ValueError: the bound of the window sides of the call."""
    from .tile_view import RESIZE_MAX_AREA
    import numpy as np
    try:
        mh, mw = resize
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (mh, mw)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"resize must be None or (max_wh, max_ww) ints, the largest window sides of the call, not {resize!r}") from None
    if shrink != 1:
        raise ValueError(f"resize= (windows of their own sizes) does not go with shrink={shrink}")
    if not (1 <= mh <= h and 1 <= mw <= w):
        raise ValueError(f"resize = ({mh}, {mw}) must lie within 1 x 1 and the {h} x {w} tile")
    if int(mh) * int(mw) > RESIZE_MAX_AREA:
        raise ValueError(f"resize = ({mh}, {mw}): a window may hold at most 2^22 pixels")
    return int(mh), int(mw)


def _resize_windows(windows, n, h, w, oh, ow, d_mask, resize):
    """_view_windows for a resizing view: the (n, 5) int32 windows (y0, x0, d, wh, ww).  numpy / CPU windows are range-checked here
    (ValueError); device windows are taken as they are -- the kernel masks the code and clamps the sides and the corner."""
    import numpy as np
    from .tile_view import RESIZE_MAX_AREA, RESIZE_MAX_RATIO
    what = "windows of a resizing view must hold (y0, x0, d, wh, ww) per tile"
    if windows is None:
        raise ValueError(f"{what}: an (N, 5) int32 array (TileView(scale=).draw)")
    if isinstance(windows, torch.Tensor) and windows.is_cuda:
        if not (windows.dtype == torch.int32 and tuple(windows.shape) == (n, 5) and windows.is_contiguous()):
            raise ValueError(f"device windows of a resizing view must be a contiguous int32 tensor of shape ({n}, 5)")
        return windows
    try:
        win = windows.numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if win.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: an (N, 5) integer array") from None
    if win.shape != (n, 5):
        raise ValueError(f"{what}: an ({n}, 5) array, not one of shape {win.shape}")
    win = win.astype(np.int64)
    d, wh, ww = win[:, 2], win[:, 3], win[:, 4]
    bad = (d < 0) | (d > 7) | ((d & ~int(d_mask)) != 0)
    if bad.any():
        raise ValueError(f"windows: tile {int(np.argmax(bad))} has the code {int(d[np.argmax(bad)])}, outside d_mask = {d_mask}")
    odd = (d & 1) != 0
    nu, nv = np.where(odd, ow, oh), np.where(odd, oh, ow)
    hi_h = np.minimum(min(int(resize[0]), h), RESIZE_MAX_RATIO * nu.astype(np.int64))
    hi_w = np.minimum(min(int(resize[1]), w), RESIZE_MAX_RATIO * nv.astype(np.int64))
    bad = (wh < 1) | (wh > hi_h) | (ww < 1) | (ww > hi_w) | (wh * ww > RESIZE_MAX_AREA)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"windows: tile {t} has a {int(wh[t])} x {int(ww[t])} window, outside 1 x 1 .. {int(hi_h[t])} x {int(hi_w[t])} "
                         f"(resize = {tuple(resize)}, at most 16 times its {int(nu[t])} x {int(nv[t])} output and 2^22 pixels)")
    bad = (win[:, 0] < 0) | (win[:, 0] > h - wh) | (win[:, 1] < 0) | (win[:, 1] > w - ww)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"windows: tile {t} has its {int(wh[t])} x {int(ww[t])} window at ({int(win[t, 0])}, {int(win[t, 1])}), "
                         f"outside the {h} x {w} tile")
    return np.ascontiguousarray(win.astype(np.int32))


def _view_windows(windows, n, h, w, oh, ow, d_mask, shrink=1, resize=None):
    """The (n, 3) int32 windows of a normalize_view call (no device needed).  numpy / CPU windows are range-checked here (ValueError) and
    come back as numpy; device windows are taken as they are -- the kernel masks the code and clamps the corner, nothing is read back.
    shrink: the window is shrink times the (oh, ow) output (TileView(shrink=)).  resize: (max_wh, max_ww) -- the (n, 5) windows of a
    resizing view (_resize_windows)."""
    import numpy as np
    if resize is not None:
        return _resize_windows(windows, n, h, w, oh, ow, d_mask, resize)
    if windows is None:
        raise ValueError("windows must hold (y0, x0, d) per tile: an (N, 3) int32 array (TileView.draw)")
    if isinstance(windows, torch.Tensor) and windows.is_cuda:
        if not (windows.dtype == torch.int32 and tuple(windows.shape) == (n, 3) and windows.is_contiguous()):
            raise ValueError(f"device windows must be a contiguous int32 tensor of shape ({n}, 3)")
        return windows
    try:
        win = windows.numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if win.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("windows must hold (y0, x0, d) per tile: an (N, 3) integer array") from None
    if win.shape != (n, 3):
        raise ValueError(f"windows must hold (y0, x0, d) per tile: an ({n}, 3) array, not one of shape {win.shape}")
    win = win.astype(np.int64)
    d = win[:, 2]
    bad = (d < 0) | (d > 7) | ((d & ~int(d_mask)) != 0)
    if bad.any():
        raise ValueError(f"windows: tile {int(np.argmax(bad))} has the code {int(d[np.argmax(bad)])}, outside d_mask = {d_mask}")
    odd = (d & 1) != 0
    wh, ww = int(shrink) * np.where(odd, ow, oh), int(shrink) * np.where(odd, oh, ow)
    bad = (win[:, 0] < 0) | (win[:, 0] > h - wh) | (win[:, 1] < 0) | (win[:, 1] > w - ww)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"windows: tile {t} has its {int(wh[t])} x {int(ww[t])} window at ({int(win[t, 0])}, {int(win[t, 1])}), "
                         f"outside the {h} x {w} tile")
    return np.ascontiguousarray(win.astype(np.int32))


def _view_prepare(rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out, before_device=None, shrink=1,
                  resize=None):
    """The checks of normalize_view (ValueError, in its order, nothing on the device before they pass; before_device(n): a caller's own
    checks at the end of them) and its arguments on the device -> (n, h, w, oh, ow, windows, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
    SlTensorFormat or None, out)."""
    from .tensor_format import TensorFormat
    from .tile_view import check_resize_size, check_size
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and rgb.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in rgb.shape[:3])
    if resize is not None:                                   # a resizing view: any output size, windows of their own sizes
        resize = _check_resize(resize, h, w, shrink)
        oh, ow = check_resize_size(size, h, w, d_mask)
    else:
        oh, ow = check_size(size, h, w, d_mask, shrink)
    win = _view_windows(windows, n, h, w, oh, ow, d_mask, shrink, resize)
    _route_check(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, n)
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    if before_device is not None:
        before_device(n)
    _check_tiles(rgb)
    dev = rgb.device
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    if win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    stats = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    return (n, h, w, oh, ow, win) + stats + _image_out(out, rgb, n, oh, ow, fmt, "view")


def normalize_view(rgb, windows, size, d_mask=7, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                   augment_background=False, params=None, fmt=None, out=None, shrink=1, resize=None):
    """A crop, flip and quarter turn per tile INSIDE the apply pass (sl_normalize_view): per tile the window windows[t] = (y0, x0, d) of
    the image that normalize_jitter (alpha_beta given), normalize_apply (M_src given) or nothing (M_src=None: the tiles' own bytes)
    writes, flipped along the width when d & 4 and then turned d & 3 quarter turns counter-clockwise -- torch.rot90(torch.flip(
    full[t][y0:y0+wh, x0:x0+ww], (1,)) if d & 4 else ..., d & 3, (0, 1)), bit for bit, without the pixels outside the window.
    size: (oh, ow) of the OUTPUT, an int, or None (the full tile); a code with odd d & 3 takes an (ow, oh) window.
    d_mask: the bits of d that count (7: everything; 6: no quarter turns -- the size need not fit transposed).
    windows: (N, 3) int32 (TileView.draw).  numpy or CPU tensor: range-checked, ValueError.  Device tensor: taken as it is, the kernel
    clamps every window into the tile; nothing is synchronised.
    fmt: a stainlib_amd.TensorFormat -> the (N,3,oh,ow) tensor, else (N,oh,ow,3) uint8.  The statistics are the WHOLE tile's.
    shrink: 1, 2 or 4 (sl_normalize_view_shrink) -- the window is shrink times (oh, ow) and every output pixel the rounded mean of a
    shrink x shrink box of `full`, per channel (sum + shrink^2 / 2) >> (2 log2 shrink), boxes counted from the window's corner; the
    flip and the turn as before (they commute with it).  size=None is then (h // shrink, w // shrink).
    resize: (max_wh, max_ww) -- a random-resized crop (sl_normalize_view_resize): windows is (N, 5) int32, (y0, x0, d, wh, ww) per tile
    (TileView(scale=).draw), a window of wh x ww pixels in the tile's orientation, resampled to the output size by exact pixel-area
    averaging in integers (stainlib_amd.tile_view.area_resample: the definition), then flipped and turned.  (max_wh, max_ww) is an
    upper bound of the window sides, within the tile and at most 2^22 pixels together: the launch is sized from it.  A window side is
    at most 16 times the output side it maps to; host windows beyond a limit are a ValueError, device windows are clamped.  (oh, ow)
    need not fit in the tile (size=None: the tile's own size); a window smaller than the output comes out piecewise constant with
    blended edges, not bilinear."""
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out, shrink=shrink, resize=resize)
    _call_view("sl_normalize_view", shrink, (_ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask)), _ptr(M_src), _ptr(maxC_src),
               _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), resize=resize)
    return out


# ---- companion planes through the windows of a view (sl_view_planes; see include/stainlib_hip.h and TileView.apply) ---------------------

PLANES_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.float16, torch.bfloat16, torch.int32, torch.float32, torch.int64,
                 torch.float64)
_PLANES_MODES = {"nearest": _ffi.PLANES_NEAREST, "area": _ffi.PLANES_AREA}


def planes_hw(planes):
    """(H, W) of companion planes (N, H, W) or (N, C, H, W), or ValueError (no device needed)"""
    if not (isinstance(planes, torch.Tensor) and planes.dim() in (3, 4)):
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W)"
                         + (f", not one of rank {planes.dim()}" if isinstance(planes, torch.Tensor) else ""))
    return int(planes.shape[-2]), int(planes.shape[-1])


def view_planes(planes, windows, size, d_mask=7, mode="nearest", out=None, shrink=1, resize=None):
    """Companion planes through the windows of a view pass (sl_view_planes): `planes` (N, H, W) or (N, C, H, W), contiguous, on the
    device, of a 1-, 2-, 4- or 8-byte dtype (PLANES_DTYPES; complex is refused) -> (N, oh, ow) or (N, C, oh, ow) of the same dtype.
    windows, size, d_mask, shrink, resize: those of the normalize_view call of the images -- (N, 3) rows (y0, x0, d), or with
    resize = (max_wh, max_ww) the (N, 5) rows of a resizing view; host windows are range-checked by _view_windows (ValueError), device
    windows are clamped by the kernel with the image kernels' rules.
    mode: "nearest" -- per tile and plane the window is sampled in the TILE's orientation at the pixel under each output's centre,
    ((2 i + 1) nw) // (2 no) along an axis (stainlib_amd.tile_view.nearest_index), a bit copy, THEN flipped along the width if d & 4
    and turned d & 3 quarter turns; "area" -- uint8 only, the images' box mean / area average per plane.
    out: a contiguous tensor of the result's shape, dtype and device to write into (not `planes` itself)."""
    from .tile_view import check_resize_size, check_size
    h, w = planes_hw(planes)
    n = int(planes.shape[0])
    c = int(planes.shape[1]) if planes.dim() == 4 else 1
    if planes.dtype not in PLANES_DTYPES:
        raise ValueError(f"planes of dtype {planes.dtype} are not supported: an element must have 1, 2, 4 or 8 bytes "
                         "(bool, uint8, int8, int16, float16, bfloat16, int32, float32, int64, float64)")
    if not isinstance(mode, str) or mode not in _PLANES_MODES:
        raise ValueError(f"mode must be 'nearest' or 'area', not {mode!r}")
    if mode == "area" and planes.dtype != torch.uint8:
        raise ValueError(f"mode='area' averages and is defined on uint8 planes only, not {planes.dtype} (labels go with mode='nearest')")
    if resize is not None:
        resize = _check_resize(resize, h, w, shrink)
        oh, ow = check_resize_size(size, h, w, d_mask)
    else:
        oh, ow = check_size(size, h, w, d_mask, shrink)
    win = _view_windows(windows, n, h, w, oh, ow, d_mask, shrink, resize)
    if not planes.is_cuda:
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W), not a CPU tensor")
    if not planes.is_contiguous():
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W): this one is not contiguous "
                         "(channels-last planes are not supported)")
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise ValueError(f"planes of shape {tuple(planes.shape)} hold no element")
    dev = planes.device
    shape = (n, oh, ow) if planes.dim() == 3 else (n, c, oh, ow)
    if out is None:
        out = torch.empty(shape, dtype=planes.dtype, device=dev)
    elif not (isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == planes.dtype and out.device == dev
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {planes.dtype} tensor of shape {shape} on {dev}")
    elif out.data_ptr() == planes.data_ptr():
        raise ValueError("out must not be planes itself: the view is not done in place")
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    if win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    mh, mw = resize if resize is not None else (0, 0)
    _call("sl_view_planes", _ptr(planes), _ptr(out), n, c, h, w, planes.element_size(), oh, ow, _ptr(win), int(d_mask), int(shrink), mh, mw,
          _PLANES_MODES[mode])
    return out


# ---- the affine views: rotation by any angle, zoom, shear, translation (sl_normalize_view_affine, sl_view_planes_affine; TileAffine) ------

def _is_affine(view):
    from .tile_view import TileAffine
    return isinstance(view, TileAffine)


def _no_affine(view, what, instead):
    """ValueError for an affine view in a call that has no bilinear write side"""
    if _is_affine(view):
        raise ValueError(f"an affine view ({view!r}) is not supported by {what}: {instead}")


def _affine_windows(windows, n, h, w, size, max_r):
    """The (n, 6) int32 windows of an affine call (no device needed).  numpy / CPU windows are range-checked (tile_view.
    affine_check_windows: ValueError) and come back as numpy; device windows are taken as they are -- the kernel clamps the centres and
    writes a tile whose row sums pass max_r as fill; nothing is read back."""
    from .tile_view import ElasticWindows, affine_check_windows
    if isinstance(windows, ElasticWindows):
        raise ValueError("these windows are the ElasticWindows of an elastic view: pass them with the TileElastic that drew them, or "
                         "windows.affine for the affine part alone")
    if isinstance(windows, torch.Tensor) and windows.is_cuda:
        if not (windows.dtype == torch.int32 and tuple(windows.shape) == (n, 6) and windows.is_contiguous()):
            raise ValueError(f"device windows of an affine view must be a contiguous int32 tensor of shape ({n}, 6)")
        affine_check_windows(torch.zeros((n, 6), dtype=torch.int32), n, h, w, size, max_r)      # (the size and the bound alone)
        return windows
    return affine_check_windows(windows, n, h, w, size, max_r)


def _affine_bound(view, windows):
    """max_r of the call behind an affine view (no device needed): of host windows their own largest row sum (at least 1; beyond the
    limit: the limit, and affine_check_windows says so), of device windows (never read back) or none yet the largest the view can
    draw (TileAffine.bound)."""
    import numpy as np
    from .tile_view import AFFINE_MAX_R, affine_row_sums
    if windows is None or (isinstance(windows, torch.Tensor) and windows.is_cuda):
        return view.bound
    try:
        win = windows.numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if win.dtype.kind not in "iu" or win.ndim != 2 or win.shape[1] != 6 or win.shape[0] == 0:
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        return view.bound                                    # (affine_check_windows says what is wrong with them)
    return max(1, min(AFFINE_MAX_R, int(affine_row_sums(win).max())))


def normalize_view_affine(rgb, windows, size, max_r, fill=255, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                          augment_background=False, params=None, fmt=None, out=None):
    """A rotation by any angle, zoom, shear and translation per tile INSIDE the apply pass (sl_normalize_view_affine): per tile the image
    that normalize_jitter (alpha_beta given), normalize_apply (M_src given) or nothing (M_src=None: the tiles' own bytes) writes, sampled
    bilinearly with 8-bit weights at the positions windows[t] = (cy, cx, a00, a01, a10, a11) names (2^-16 source pixels; stainlib_amd.
    tile_view.affine_resample is the definition, bit for bit).  The image is normalised / jittered per SOURCE pixel and the statistics
    are the WHOLE tile's.
    size: (oh, ow) of the OUTPUT, an int, or None (the tile's own size); it need not fit in the tile.  h, w, oh, ow <= 8192.
    max_r: an int, 1 .. 2 Q = 131072 -- an upper bound of the row sums |a00| + |a01|, |a10| + |a11| of the call's windows (TileAffine.bound);
    the launch is sized from it.
    fill: an int or three ints 0 .. 255, the OUTPUT bytes of what lies outside the tile (not normalised).
    windows: (N, 6) int32 (TileAffine.draw).  numpy or CPU tensor: range-checked, ValueError.  Device tensor: taken as it is -- the kernel
    clamps the centres into their range and writes a tile whose row sums pass max_r as fill everywhere; nothing is synchronised.
    fmt: a stainlib_amd.TensorFormat -> the (N,3,oh,ow) tensor, else (N,oh,ow,3) uint8."""
    return _view_affine_call(None, rgb, windows, size, max_r, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params,
                             fmt, out)


def _view_affine_call(stages, rgb, windows, size, max_r, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt,
                      out):
    """normalize_view_affine (stages=None) and normalize_stages_view_affine (stages: _stages_check's keyword arguments): the checks in
    normalize_view_affine's order, the stages' behind them and before anything is on the device, then the one call."""
    from .tensor_format import TensorFormat
    from .tile_view import _fill3, affine_check_size
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and rgb.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in rgb.shape[:3])
    oh, ow = affine_check_size(size, h, w)
    f3 = _fill3(fill)
    win = _affine_windows(windows, n, h, w, size, max_r)
    _route_check(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, n)
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    if stages is not None:
        _stages_check(n, **stages)
    _check_tiles(rgb)
    dev = rgb.device
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    if win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    M_src, maxC_src, M_tgt, maxC_tgt, ab = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    f, out = _image_out(out, rgb, n, oh, ow, fmt, "view")
    st, keep = _stages_upload(n, dev, **stages) if stages is not None else ((), None)
    _call("sl_normalize_view_affine" if stages is None else "sl_normalize_stages_view_affine", _ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win),
          int(max_r), f3[0] | (f3[1] << 8) | (f3[2] << 16), _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab),
          1 if augment_background else 0, _byref(params), _byref(f), *st)
    return out


def _fill_bits(fill, dtype):
    """the bit pattern of `fill` as one element of a planes dtype, as an unsigned int (ValueError if it is no number of that dtype)"""
    try:
        t = torch.tensor([fill], dtype=dtype)
    except (TypeError, ValueError, RuntimeError, OverflowError):
        raise ValueError(f"fill must be a number that a {dtype} element can hold, not {fill!r}") from None
    es = t.element_size()
    bits = int(t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[es])[0])
    return bits & ((1 << (8 * es)) - 1)


def view_planes_affine(planes, windows, size, max_r, fill=0, out=None):
    """Companion planes through the windows of an affine view (sl_view_planes_affine): `planes` (N, H, W) or (N, C, H, W), contiguous, on
    the device, of a 1-, 2-, 4- or 8-byte dtype (PLANES_DTYPES) -> (N, oh, ow) or (N, C, oh, ow) of the same dtype: per element the
    NEAREST source element (Y >> 16, X >> 16) of the image view's coordinates, a bit copy (stainlib_amd.tile_view.affine_nearest is
    the definition), outside the plane `fill` cast to the planes' dtype.  windows, size, max_r: those of the normalize_view_affine call of
    the images.  out: a contiguous tensor of the result's shape, dtype and device to write into (not `planes` itself)."""
    from .tile_view import affine_check_size
    h, w = planes_hw(planes)
    n = int(planes.shape[0])
    c = int(planes.shape[1]) if planes.dim() == 4 else 1
    if planes.dtype not in PLANES_DTYPES:
        raise ValueError(f"planes of dtype {planes.dtype} are not supported: an element must have 1, 2, 4 or 8 bytes "
                         "(bool, uint8, int8, int16, float16, bfloat16, int32, float32, int64, float64)")
    oh, ow = affine_check_size(size, h, w)
    bits = _fill_bits(fill, planes.dtype)
    win = _affine_windows(windows, n, h, w, size, max_r)
    if not planes.is_cuda:
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W), not a CPU tensor")
    if not planes.is_contiguous():
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W): this one is not contiguous "
                         "(channels-last planes are not supported)")
    if n < 1 or c < 1:
        raise ValueError(f"planes of shape {tuple(planes.shape)} hold no element")
    dev = planes.device
    shape = (n, oh, ow) if planes.dim() == 3 else (n, c, oh, ow)
    if out is None:
        out = torch.empty(shape, dtype=planes.dtype, device=dev)
    elif not (isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == planes.dtype and out.device == dev
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {planes.dtype} tensor of shape {shape} on {dev}")
    elif out.data_ptr() == planes.data_ptr():
        raise ValueError("out must not be planes itself: the view is not done in place")
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    if win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    _call("sl_view_planes_affine", _ptr(planes), _ptr(out), n, c, h, w, planes.element_size(), oh, ow, _ptr(win), int(max_r), bits)
    return out


# ---- the elastic views: the affine view plus a smooth displacement field (sl_normalize_view_elastic, sl_view_planes_elastic; TileElastic) ---

def _is_elastic(view):
    from .tile_view import TileElastic
    return isinstance(view, TileElastic)


def _on_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _elastic_parts(windows):
    """(affine, field) of the windows= of an elastic view (no device needed), or ValueError: anything but an ElasticWindows, or one
    with a part on each side"""
    from .tile_view import ElasticWindows
    if not isinstance(windows, ElasticWindows):
        raise ValueError("windows of an elastic view must be the stainlib_amd.ElasticWindows(affine, field) a call with this TileElastic "
                         "returned (or view.draw(N, H, W)), not " + ("a plain array of affine rows: wrap it as ElasticWindows(rows, field) "
                                                                     "with a field of elastic_grid_shape" if hasattr(windows, "shape")
                                                                     else type(windows).__name__))
    if _on_device(windows.affine) != _on_device(windows.field):
        raise ValueError("the two parts of an ElasticWindows must live on the same side: both on the host (range-checked) or both on the "
                         "device (clamped by the kernel) -- move one of them")
    return windows.affine, windows.field


def _elastic_field(field, n, size, cell, max_d):
    """The (n, gh, gw, 2) int32 field of an elastic call (no device needed).  A numpy / CPU field is range-checked (tile_view.
    elastic_check_field: ValueError) and comes back as numpy; a device field is taken as it is -- the kernel clamps every control value
    to +-256 max_d; nothing is read back."""
    from .tile_view import elastic_check_field, elastic_grid_shape
    if _on_device(field):
        shape = (n,) + elastic_grid_shape(size, cell) + (2,)
        if not (field.dtype == torch.int32 and tuple(field.shape) == shape and field.is_contiguous()):
            raise ValueError(f"the device field of an elastic view must be a contiguous int32 tensor of shape {shape}")
        elastic_check_field(torch.zeros(shape, dtype=torch.int32), n, size, cell, max_d)        # (the cell and the bound alone)
        return field
    return elastic_check_field(field, n, size, cell, max_d)


def _elastic_bound(view, windows):
    """(max_r, max_d) of the call behind an elastic view (no device needed): max_r as _affine_bound; max_d of a host field its own
    largest control displacement in whole pixels, rounded up (beyond the limit: the limit, and elastic_check_field says so), of a
    device field (never read back) or none yet the largest the view can draw (TileElastic.max_d)."""
    import numpy as np
    from .tile_view import ELASTIC_MAX_D, ELASTIC_UNIT, ElasticWindows
    if not isinstance(windows, ElasticWindows):
        return view.bound, view.max_d
    max_r = _affine_bound(view, windows.affine)
    field = windows.field
    if _on_device(field):
        return max_r, view.max_d
    try:
        f = field.numpy() if isinstance(field, torch.Tensor) else np.asarray(field)
        if f.dtype.kind not in "iu" or f.size == 0:
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        return max_r, view.max_d                             # (elastic_check_field says what is wrong with it)
    return max_r, min(ELASTIC_MAX_D, (int(np.abs(f.astype(np.int64)).max()) + ELASTIC_UNIT - 1) // ELASTIC_UNIT)


def normalize_view_elastic(rgb, windows, field, size, cell, max_r, max_d, fill=255, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None,
                           alpha_beta=None, augment_background=False, params=None, fmt=None, out=None):
    """normalize_view_affine with a smooth per-pixel displacement on top (sl_normalize_view_elastic): per tile the image the statistics
    pattern names, sampled bilinearly at the affine positions of windows[t] moved by the quadratic B-spline of the control lattice
    field[t] (stainlib_amd.tile_view.elastic_resample is the definition, bit for bit).
    windows, size, max_r, fill, the statistics, fmt, out: normalize_view_affine's.
    field: (N, gh, gw, 2) int32, (dy, dx) per lattice node in 1/256 source pixel, (gh, gw) = tile_view.elastic_grid_shape(size, cell).
    numpy or CPU tensor: range-checked against max_d, ValueError.  Device tensor: taken as it is -- the kernel clamps every control
    value to +-256 max_d.  Both windows and field on the host, or both on the device.
    cell: the lattice spacing in OUTPUT pixels, a power of two 16 .. 256.  max_d: an int 0 .. 8, an upper bound in source pixels of
    the control displacements of the call (TileElastic.max_d); the launch is sized from max_r and max_d."""
    return _view_elastic_call(None, rgb, windows, field, size, cell, max_r, max_d, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                              augment_background, params, fmt, out)


def _view_elastic_call(stages, rgb, windows, field, size, cell, max_r, max_d, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                       augment_background, params, fmt, out):
    """normalize_view_elastic (stages=None) and normalize_stages_view_elastic (stages: _stages_check's keyword arguments), as
    _view_affine_call."""
    from .tensor_format import TensorFormat
    from .tile_view import _cell_log2, _fill3, affine_check_size
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and rgb.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in rgb.shape[:3])
    oh, ow = affine_check_size(size, h, w)
    f3 = _fill3(fill)
    if _on_device(windows) != _on_device(field):
        raise ValueError("windows and field of an elastic view must live on the same side: both on the host or both on the device")
    win = _affine_windows(windows, n, h, w, size, max_r)
    fld = _elastic_field(field, n, (oh, ow), cell, max_d)
    _route_check(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, n)
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    if stages is not None:
        _stages_check(n, **stages)
    _check_tiles(rgb)
    dev = rgb.device
    if not isinstance(win, torch.Tensor):
        win, fld = torch.from_numpy(win).to(dev), torch.from_numpy(fld).to(dev)
    if win.device != dev or fld.device != dev:
        raise ValueError(f"windows and field must be on {dev}")
    M_src, maxC_src, M_tgt, maxC_tgt, ab = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    f, out = _image_out(out, rgb, n, oh, ow, fmt, "view")
    st, keep = _stages_upload(n, dev, **stages) if stages is not None else ((), None)
    _call("sl_normalize_view_elastic" if stages is None else "sl_normalize_stages_view_elastic", _ptr(rgb), _ptr(out), n, h, w, oh, ow,
          _ptr(win), int(max_r), _ptr(fld), _cell_log2(cell), int(max_d), f3[0] | (f3[1] << 8) | (f3[2] << 16), _ptr(M_src), _ptr(maxC_src),
          _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), *st)
    return out


def view_planes_elastic(planes, windows, field, size, cell, max_r, max_d, fill=0, out=None):
    """view_planes_affine through an elastic view (sl_view_planes_elastic): per element the NEAREST source element (Y >> 16, X >> 16) of
    the image view's coordinates (stainlib_amd.tile_view.elastic_nearest is the definition), outside the plane `fill`.  windows, field,
    size, cell, max_r, max_d: those of the normalize_view_elastic call of the images; planes, fill, out: view_planes_affine's."""
    from .tile_view import _cell_log2, affine_check_size
    h, w = planes_hw(planes)
    n = int(planes.shape[0])
    c = int(planes.shape[1]) if planes.dim() == 4 else 1
    if planes.dtype not in PLANES_DTYPES:
        raise ValueError(f"planes of dtype {planes.dtype} are not supported: an element must have 1, 2, 4 or 8 bytes "
                         "(bool, uint8, int8, int16, float16, bfloat16, int32, float32, int64, float64)")
    oh, ow = affine_check_size(size, h, w)
    bits = _fill_bits(fill, planes.dtype)
    if _on_device(windows) != _on_device(field):
        raise ValueError("windows and field of an elastic view must live on the same side: both on the host or both on the device")
    win = _affine_windows(windows, n, h, w, size, max_r)
    fld = _elastic_field(field, n, (oh, ow), cell, max_d)
    if not planes.is_cuda:
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W), not a CPU tensor")
    if not planes.is_contiguous():
        raise ValueError("planes must be a contiguous CUDA tensor of shape (N, H, W) or (N, C, H, W): this one is not contiguous "
                         "(channels-last planes are not supported)")
    if n < 1 or c < 1:
        raise ValueError(f"planes of shape {tuple(planes.shape)} hold no element")
    dev = planes.device
    shape = (n, oh, ow) if planes.dim() == 3 else (n, c, oh, ow)
    if out is None:
        out = torch.empty(shape, dtype=planes.dtype, device=dev)
    elif not (isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == planes.dtype and out.device == dev
              and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {planes.dtype} tensor of shape {shape} on {dev}")
    elif out.data_ptr() == planes.data_ptr():
        raise ValueError("out must not be planes itself: the view is not done in place")
    if not isinstance(win, torch.Tensor):
        win, fld = torch.from_numpy(win).to(dev), torch.from_numpy(fld).to(dev)
    if win.device != dev or fld.device != dev:
        raise ValueError(f"windows and field must be on {dev}")
    _call("sl_view_planes_elastic", _ptr(planes), _ptr(out), n, c, h, w, planes.element_size(), oh, ow, _ptr(win), int(max_r), _ptr(fld),
          _cell_log2(cell), int(max_d), bits)
    return out


# ---- stain separation in the view pass (sl_stain_separate_view; see include/stainlib_hip.h) ---------------------------------------------

def _separate_view_args(want, conc_dtype, fmt, out, shrink, M_tgt, maxC_tgt):
    """What can be said about a stain_separate_view call behind its size and windows and without the tiles (no device needed) -> want."""
    from .tensor_format import TensorFormat
    if (M_tgt is None) != (maxC_tgt is None):
        raise ValueError("M_tgt and maxC_tgt go together: both, or neither (no target)")
    want = _separate_want(want, conc_dtype)
    if shrink != 1 and "conc" in want:
        raise ValueError(f"shrink={shrink} does not go with 'conc' in want: a shrunk concentration plane would be a mean of floats, "
                         "another definition; ask for the images alone, or take conc at shrink=1")
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 images)")
    _separate_out_fields(out, want, conc_dtype, fmt.dtype if fmt is not None else torch.uint8)
    return want


def stain_separate_view(rgb, windows, size, M_src, maxC_src, M_tgt=None, maxC_tgt=None, d_mask=7, lasso_lambda=0.01,
                        want=("norm", "h", "e", "conc"), conc_dtype=torch.float32, fmt=None, out=None, shrink=1):
    """stain_separate under normalize_view's crop, flip and quarter turn per tile, in ONE pass (sl_stain_separate_view) -> Separated:
    per tile the window windows[t] = (y0, x0, d) of what stain_separate writes, flipped along the width when d & 4 and then turned d & 3
    quarter turns -- bit for bit the torch slice / flip / rot90 of the full-tile result, without the pixels outside the window: one read
    and one lasso solve per source pixel of the window.
    size, d_mask, windows: normalize_view's (numpy / CPU windows are range-checked, device windows are clamped by the kernel; nothing
    is synchronised).  M_tgt=None (and maxC_tgt=None): no target, as in stain_separate.
    fmt: a stainlib_amd.TensorFormat -> norm, h and e are (N,3,oh,ow) tensors, bit for bit fmt.convert of the uint8 views; None ->
    (N,oh,ow,3) uint8.  conc is (N,2,oh,ow) planes of conc_dtype either way.
    shrink: 1, 2 or 4 -- the images box-shrunk as in normalize_view (the window is shrink times (oh, ow)); not with 'conc' in want.
    out: a Separated of caller buffers in the view's shapes (None where the library allocates).
    A tile whose fit failed (NaN M_src, maxC_src <= 0): norm = the view of the tile, h = e = white, conc = 0."""
    from .tile_view import check_size
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and rgb.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in rgb.shape[:3])
    oh, ow = check_size(size, h, w, d_mask, shrink)
    win = _view_windows(windows, n, h, w, oh, ow, d_mask, shrink)
    if M_src is None or maxC_src is None:
        raise ValueError("M_src and maxC_src are needed: the per-tile fit (macenko_fit / vahadane_fit)")
    want = _separate_view_args(want, conc_dtype, fmt, out, shrink, M_tgt, maxC_tgt)
    _check_tiles(rgb)
    dev = rgb.device
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    if win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    f, res = None, []
    for k, name in enumerate(Separated._fields):
        t = out[k] if out is not None else None
        if name not in want:
            res.append(None)
        elif name != "conc":
            f, t = _image_out(t, rgb, n, oh, ow, fmt, "view")
            res.append(t)
        elif t is None:
            res.append(torch.empty((n, 2, oh, ow), dtype=conc_dtype, device=dev))
        elif not (t.device == dev and tuple(t.shape) == (n, 2, oh, ow) and t.is_contiguous()):
            raise ValueError(f"out.conc must be a contiguous {conc_dtype} tensor of shape {(n, 2, oh, ow)} on {dev}")
        else:
            res.append(t)
    if fmt is not None and f is None:                                # (conc alone: the format is still checked by the C side)
        f = _tensor_format(fmt)[0]
    res = Separated(*res)
    M_src, maxC_src, M_tgt, maxC_tgt, _ = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt)
    o = _ffi.default_separate_out()
    o.conc_dtype = _TENSOR_DTYPES[conc_dtype]
    o.norm, o.stain[0], o.stain[1], o.conc = (t.data_ptr() if t is not None else None for t in res)
    _call("sl_stain_separate_view", _ptr(rgb), n, h, w, oh, ow, _ptr(win), int(d_mask), int(shrink), _ptr(M_src), _ptr(maxC_src),
          _ptr(M_tgt), _ptr(maxC_tgt), float(lasso_lambda), C.byref(o), _byref(f))
    return res


def separate_view_check(view, windows, tensor_format, want, conc_dtype, tiles):
    """The view= / windows= / tensor_format= arguments of separate_batch, checked without a device and without a draw (ValueError) ->
    whether the call goes through stain_separate_view."""
    if view is None:
        if windows is not None:
            raise ValueError("view must be a stainlib_amd.TileView (windows= goes with view=)")
        if tensor_format is not None:
            raise ValueError("tensor_format= goes with view=: the fused full-tile tensor is view=TileView(None, flip=False, rot90=False)")
        return False
    _no_affine(view, "separate_batch", "take the full-tile images through TensorFormat.convert(view=), which samples bilinearly "
               "(bilinear concentration planes are another definition)")
    if getattr(view, "resizing", False):
        raise ValueError(f"a resizing view ({view!r}) is not supported by separate_batch: take the full-tile images through "
                         "TensorFormat.convert(view=), which resamples")
    _, _, _, shrink = _view_call(view, windows, tiles, draw=False)
    _separate_view_args(want, conc_dtype, tensor_format, None, shrink, None, None)
    return True


# ---- HED augmentation behind the apply pass (sl_normalize_sums, sl_normalize_hed_view; see include/stainlib_hip.h) ------------------------

HedDraw = collections.namedtuple("HedDraw", ["sigmas", "biases", "applied"])
HedDraw.__doc__ = """What the hed= stage of a batch method did: the (N, 3) sigmas and biases it used (given or drawn) and applied, the (N,)
int32 device tensor of the cutoff test's decisions (0: the tile came back without the HED transform)."""


def _cutoff(cutoff):
    try:
        lo, hi = (float(v) for v in cutoff)
    except (TypeError, ValueError):
        raise ValueError("cutoff must be a pair (lo, hi) with lo <= hi") from None
    if not lo <= hi:
        raise ValueError("cutoff must be a pair (lo, hi) with lo <= hi")
    return lo, hi


def normalize_sums(rgb, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None, augment_background=False, params=None,
                   cutoff=(0.05, 0.95)):
    """The exact byte sums of the image an apply-pass route WOULD write, without writing it (sl_normalize_sums: 3 B/px read) ->
    (sums (N,) int64, applied (N,) int32).  The route is normalize_view's: nothing (M_src=None: the tiles' own bytes), normalize_apply
    (M_src and a target) or normalize_jitter (alpha_beta).  applied[t] = cutoff[0] <= sums[t] / (3 H W) / 255 <= cutoff[1]: what
    hed_augment(full, ..., cutoff=cutoff) reports for that image."""
    n_ab = _route_check(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params)
    lo, hi = _cutoff(cutoff)
    if n_ab is not None and isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and n_ab != rgb.shape[0]:
        raise ValueError(f"alpha_beta must have one row per tile ({rgb.shape[0]})")
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M_src, maxC_src, M_tgt, maxC_tgt, ab = _route_upload(n, dev, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    sums = torch.empty((n,), dtype=torch.int64, device=dev)
    applied = torch.empty((n,), dtype=torch.int32, device=dev)
    _call("sl_normalize_sums", _ptr(rgb), n, h, w, _ptr(M_src), _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab),
          1 if augment_background else 0, _byref(params), lo, hi, _ptr(sums), _ptr(applied))
    return sums, applied


def _full_image(rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params):
    """`full` of a view route, materialised by the existing entry point (the chain the fused passes are defined by)."""
    if M_src is None:
        return rgb
    if alpha_beta is None:
        lam = params.lasso_lambda if params is not None else _ffi.default_params().lasso_lambda
        return normalize_apply(rgb, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda=lam)
    return normalize_jitter(rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params=params)


def _hed_rows(x, what):
    """The rows of an (N, 3) sigma / bias argument (no device needed)."""
    import numpy as np
    try:
        shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64).shape
    except (TypeError, ValueError):
        raise ValueError(f"{what} must hold (H, E, D) per tile: an (N, 3) array") from None
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{what} must hold (H, E, D) per tile: an (N, 3) array, not one of shape {shape}")
    return shape[0]


def normalize_hed_view(rgb, windows, size, d_mask, hed_sigma, hed_bias, hed_applied, skimage_mode=0, M_src=None, maxC_src=None, M_tgt=None,
                       maxC_tgt=None, alpha_beta=None, augment_background=False, params=None, fmt=None, out=None, shrink=1, resize=None):
    """normalize_view of hed_applied[t] ? HED(full[t]) : full[t] in ONE pass (sl_normalize_hed_view): `full` is normalize_view's (the
    route arguments are the same), HED(.) is hed_augment with the tile's hed_sigma / hed_bias ((N, 3) each), skimage_mode and a cutoff that
    never fails -- bit for bit hed_augment then normalize_view of the result, without a pixel outside the window being touched.
    hed_applied: (N,) int32, the decision per tile (normalize_sums gives it).
    skimage_mode 0 ("0.18", the pinned one) runs in the kernel; the other three go through that chain (same bits, two more passes).
    shrink: normalize_view's, on that image (sl_normalize_hed_view_shrink); skimage_mode 0 only -- the chain does not know it.
    resize: normalize_view's, on that image (sl_normalize_hed_view_resize), with (N, 5) windows; skimage_mode 0 only."""
    def hed_checks(n):
        for x, what in ((hed_sigma, "hed_sigma"), (hed_bias, "hed_bias")):
            if _hed_rows(x, what) != n:
                raise ValueError(f"{what} must have one row per tile ({n})")
        if skimage_mode not in (_ffi.HED_SKIMAGE_018, _ffi.HED_SKIMAGE_019, _ffi.HED_SKIMAGE_017, _ffi.HED_EXPERIMENTAL_LOG10):
            raise ValueError("skimage_mode must be one of the HED_* modes (0..3)")
        _hed_shrink_ok(skimage_mode, shrink, resize)
        if hed_applied is None:
            raise ValueError("hed_applied must hold the decision per tile: (N,) int32 (normalize_sums)")
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out, before_device=hed_checks, shrink=shrink,
        resize=resize)
    dev = rgb.device
    sigma = _f64(hed_sigma, (n, 3), dev)
    bias = _f64(hed_bias, (n, 3), dev)
    applied = torch.as_tensor(hed_applied, device=dev).to(torch.int32).reshape(n).contiguous()
    if skimage_mode != _ffi.HED_SKIMAGE_018:                 # the chain itself
        full = _full_image(rgb, M_src, maxC_src, M_tgt, maxC_tgt, ab, augment_background, params)
        aug, _ = hed_augment(full, sigma, bias, cutoff=(-float("inf"), float("inf")), skimage_mode=skimage_mode)
        img = torch.where((applied != 0).view(n, 1, 1, 1), aug, full)
        return normalize_view(img, win, size, d_mask, fmt=fmt, out=out)
    _call_view("sl_normalize_hed_view", shrink, (_ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask)), _ptr(M_src), _ptr(maxC_src),
               _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), _ptr(sigma), _ptr(bias),
               _ptr(applied), int(skimage_mode), resize=resize)
    return out


def _hed_shrink_ok(skimage_mode, shrink, resize=None):
    """ValueError for a HED skimage_mode that goes through the chain (every one but HED_SKIMAGE_018) under a view with a shrink or a
    resizing view (resize: anything but None): the chain does not know either."""
    names = {_ffi.HED_SKIMAGE_019: "0.19", _ffi.HED_SKIMAGE_017: "0.17", _ffi.HED_EXPERIMENTAL_LOG10: "experimental_log10"}
    if resize is not None and skimage_mode != _ffi.HED_SKIMAGE_018:
        raise ValueError(f"skimage_mode {names.get(skimage_mode, skimage_mode)!r} ({skimage_mode}) goes through the hed_augment chain, which does "
                         "not resample: a resizing view (TileView(scale=), resize=) needs skimage_mode '0.18' (0)")
    if shrink != 1 and skimage_mode != _ffi.HED_SKIMAGE_018:
        raise ValueError(f"skimage_mode {names.get(skimage_mode, skimage_mode)!r} ({skimage_mode}) goes through the hed_augment chain, which has "
                         f"no shrink: a view with shrink={shrink} needs skimage_mode '0.18' (0)")


def _hed_call(hed, hed_sigmas, hed_biases, tiles, view=None):
    """The hed= / hed_sigmas= / hed_biases= arguments of a batch method, checked without a device (ValueError).  True when the call has a
    HED stage.  view: the call's view= (checked elsewhere) -- its shrink must be one the HED mode knows (_hed_shrink_ok)."""
    from .augmentation.augmenter import HedColorAugmenter
    if hed is None:
        if hed_sigmas is not None or hed_biases is not None:
            raise ValueError("hed_sigmas= and hed_biases= go with hed= (a HedColorAugmenter)")
        return False
    _no_affine(view, "the HED stage (hed=, HedColorAugmenter.transform_batch(view=))",
               "take the HED result as a uint8 image through TensorFormat.convert(view=), which samples bilinearly")
    if not isinstance(hed, HedColorAugmenter):
        raise ValueError("hed must be a stainlib_amd HedColorAugmenter (its ranges, cutoff and skimage_mode are used)")
    if (hed_sigmas is None) != (hed_biases is None):
        raise ValueError("hed_sigmas and hed_biases go together: both, or neither (drawn: hed.randomize_batch)")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n = int(tiles.shape[0])
    for x, what in ((hed_sigmas, "hed_sigmas"), (hed_biases, "hed_biases")):
        if x is not None and _hed_rows(x, what) != n:
            raise ValueError(f"{what} must have one row per tile ({n})")
    _hed_shrink_ok(hed._skimage_mode, getattr(view, "shrink", 1), getattr(view, "scale", None))
    return True


def _near_cutoff(sums, pixels, cutoff):
    """The knife-edge rule of HedColorAugmenter's cutoff test -> the indices of the tiles it applies to: those whose EXACT mean, the byte
    sum sums[t] (an (N,) int64 tensor) / (3 pixels) / 255, lies within _CUTOFF_BAND (relative) of a bound of cutoff = (lo, hi).
    The device tests that exact mean; the reference tests np.mean of the float32 image / 255 (augmenter.py:291-293), whose pairwise
    binary32 sum can be off by ~2e-6 relative on a large patch.  For the tiles named here the reference's own value decides
    (_reference_cutoff_test), so that a tile gets the same answer alone and in a batch.  One 8-byte-per-tile read-back; such tiles are rare."""
    from .augmentation.augmenter import _CUTOFF_BAND
    lo, hi = cutoff
    exact = sums.to(torch.float64) / float(pixels * 3) / 255.0
    band = _CUTOFF_BAND * max(abs(lo), abs(hi), 1e-30)
    return torch.nonzero(torch.minimum((exact - lo).abs(), (exact - hi).abs()) <= band).reshape(-1).tolist()


def _reference_cutoff_test(patch, cutoff):
    """The reference's own cutoff test (augmenter.py:291-293) of a host patch ((H, W, 3) uint8 ndarray): its float32 mean inside cutoff."""
    import numpy as np
    return bool(cutoff[0] <= np.mean(a=patch.astype(dtype=np.float32)) / 255.0 <= cutoff[1])


def hed_decide(tiles, cutoff, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None, augment_background=False, params=None):
    """HedColorAugmenter's cutoff decision per tile for the image a route would write -> applied (N,) int32 on the device: normalize_sums,
    then the knife-edge rule (_near_cutoff); only for a tile it names is `full` materialised (that one tile, by the existing entry point)
    and tested on the host."""
    cutoff = _cutoff(cutoff)
    sums, applied = normalize_sums(tiles, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, cutoff=cutoff)
    n, h, w = (int(v) for v in tiles.shape[:3])
    near = _near_cutoff(sums, h * w, cutoff)
    if near:
        M_src, maxC_src, M_tgt, maxC_tgt, ab = _route_upload(n, tiles.device, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta)
    for i in near:
        one = lambda x: x[i:i + 1] if x is not None else None        # noqa: E731
        patch = _full_image(tiles[i:i + 1], one(M_src), one(maxC_src), M_tgt, maxC_tgt, one(ab), augment_background, params)[0].cpu().numpy()
        applied[i] = 1 if _reference_cutoff_test(patch, cutoff) else 0
    return applied


def hed_stage(tiles, hed, hed_sigmas, hed_biases, view, windows, route, fmt=None, out=None):
    """The hed= stage of the batch methods, behind their fit and their own draws, on arguments _hed_call / _view_call(draw=False) have
    accepted: the draws the caller left open -- hed.randomize_batch(N), THEN view.draw --, the cutoff decision (hed_decide) and ONE fused
    pass (normalize_hed_view).  route: normalize_view's keyword arguments that name `full` ({}: the tiles themselves).  Without a view
    the result is the full tile, code 0.  -> (out, windows or None, HedDraw)."""
    import numpy as np
    n = int(tiles.shape[0])
    if hed_sigmas is None:
        hed_sigmas, hed_biases = hed.randomize_batch(n)
    if view is not None:
        size, d_mask, windows, shrink = _view_call(view, windows, tiles)
        win = windows
    else:
        size, d_mask, windows, win, shrink = None, 0, None, np.zeros((n, 3), dtype=np.int32), 1
    applied = hed_decide(tiles, hed._cutoff_range, **route)
    x = normalize_hed_view(tiles, win, size, d_mask, hed_sigmas, hed_biases, applied, hed._skimage_mode, fmt=fmt, out=out, shrink=shrink,
                           resize=_view_resize(view, win, tiles), **route)
    return x, windows, HedDraw(hed_sigmas, hed_biases, applied)


# ---- hue / saturation / brightness augmentation (sl_hsb_augment, sl_normalize_hsb_view; see include/stainlib_hip.h, augmentation/hsb.py) ----

HsbDraw = collections.namedtuple("HsbDraw", ["sigmas", "codes"])
HsbDraw.__doc__ = """What the hsb= stage of a batch method did: the (N, 3) float64 sigmas it used (given or drawn: hue, saturation,
brightness) and the (N, 3) int32 codes they gave (augmentation.hsb.hsb_codes), both numpy."""


def _hsb_codes_rows(codes):
    """The rows of an (N, 3) codes argument (no device needed): a device int32 tensor, or host integers that fit int32."""
    import numpy as np
    what = "codes must hold (dhq, dsq, dvq) per tile: an (N, 3) int32 array (augmentation.hsb.hsb_codes)"
    if isinstance(codes, torch.Tensor):
        if codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[1] != 3:
            raise ValueError(what)
        return int(codes.shape[0])
    try:
        arr = np.asarray(codes)
        if arr.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(what) from None
    if arr.ndim != 2 or arr.shape[1] != 3:
        raise ValueError(f"{what}, not one of shape {arr.shape}")
    if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
        raise ValueError("codes must fit int32")
    return int(arr.shape[0])


def _hsb_codes_device(codes, n, device):
    import numpy as np
    if _hsb_codes_rows(codes) != n:
        raise ValueError(f"codes must have one row per tile ({n})")
    if isinstance(codes, torch.Tensor):
        return codes.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(codes).astype(np.int32))).to(device)


def hsb_augment(rgb, codes, fmt=None, out=None):
    """The HSB map of every tile in one sweep (sl_hsb_augment): codes (N, 3) int32 = (dhq, dsq, dvq) per tile (augmentation.hsb.hsb_codes;
    a device tensor is taken as it is, out-of-range values are reduced by the kernel) -> (N,H,W,3) uint8, bit for bit
    augmentation.hsb.hsb_reference; or with fmt (a stainlib_amd.TensorFormat) the (N,3,H,W) tensor, bit for bit fmt.convert of that image,
    written directly."""
    from .tensor_format import TensorFormat
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    _hsb_codes_rows(codes)
    n, h, w = _check_tiles(rgb)
    c = _hsb_codes_device(codes, n, rgb.device)
    f, out = _image_out(out, rgb, n, h, w, fmt, "HSB augmentation")
    _call("sl_hsb_augment", _ptr(rgb), _ptr(out), n, h, w, _ptr(c), _byref(f))
    return out


def normalize_hsb_view(rgb, windows, size, d_mask, codes, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                       augment_background=False, params=None, fmt=None, out=None, shrink=1, resize=None):
    """normalize_view of HSB(full[t]) in ONE pass (sl_normalize_hsb_view): `full` is normalize_view's (the route arguments are the same),
    HSB(.) is hsb_augment with the tile's codes -- bit for bit hsb_augment of `full`, then normalize_view of the result, without a pixel
    outside the window being touched.  shrink, resize: normalize_view's, acting on the HSB-mapped pixels.  A tile whose fit failed: the
    view of HSB(its own bytes)."""
    def codes_ok(n):
        if _hsb_codes_rows(codes) != n:
            raise ValueError(f"codes must have one row per tile ({n})")
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out, before_device=codes_ok, shrink=shrink,
        resize=resize)
    c = _hsb_codes_device(codes, n, rgb.device)
    mh, mw = (int(resize[0]), int(resize[1])) if resize is not None else (0, 0)
    _call("sl_normalize_hsb_view", _ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask), int(shrink), mh, mw, _ptr(M_src),
          _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), _ptr(c))
    return out


def _hsb_call(hsb, hsb_sigmas, tiles, view=None, hed=None):
    """The hsb= / hsb_sigmas= arguments of a batch method, checked without a device and before any draw (ValueError).  True when the call
    has an HSB stage.  view, hed: the call's view= and hed= -- an affine view and a HED stage do not go with it."""
    from .augmentation.hsb import HsbColorAugmenter, hsb_codes
    if hsb is None:
        if hsb_sigmas is not None:
            raise ValueError("hsb_sigmas= goes with hsb= (an HsbColorAugmenter)")
        return False
    if hed is not None:
        raise ValueError("hsb= and hed= do not go together: a pass has one colour-augmentation stage (chain hed.transform_batch or "
                         "hsb.transform_batch behind the call for the second)")
    _no_affine(view, "the HSB stage (hsb=, HsbColorAugmenter.transform_batch(view=))",
               "take the HSB result as a uint8 image through TensorFormat.convert(view=), which samples bilinearly")
    if not isinstance(hsb, HsbColorAugmenter):
        raise ValueError("hsb must be a stainlib_amd HsbColorAugmenter (its ranges are used)")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    if hsb_sigmas is not None:
        codes = hsb_codes(hsb_sigmas)
        if codes.ndim != 2 or codes.shape[0] != int(tiles.shape[0]):
            raise ValueError(f"hsb_sigmas must have one (hue, saturation, brightness) row per tile ({int(tiles.shape[0])})")
    return True


def hsb_stage(tiles, hsb, hsb_sigmas, view, windows, route, fmt=None, out=None):
    """The hsb= stage of the batch methods, behind their fit and their own draws, on arguments _hsb_call / _view_call(draw=False) have
    accepted: the draws the caller left open -- hsb.randomize_batch(N), THEN view.draw -- and ONE fused pass (normalize_hsb_view).  route:
    normalize_view's keyword arguments that name `full` ({}: the tiles themselves).  Without a view the result is the full tile, code 0.
    -> (out, windows or None, HsbDraw)."""
    import numpy as np
    from .augmentation.hsb import hsb_codes
    n = int(tiles.shape[0])
    if hsb_sigmas is None:
        hsb_sigmas = hsb.randomize_batch(n)
    sigmas = np.array(hsb_sigmas, dtype=np.float64)
    codes = hsb_codes(sigmas)
    if view is not None:
        size, d_mask, windows, shrink = _view_call(view, windows, tiles)
        win = windows
    else:
        size, d_mask, windows, win, shrink = None, 0, None, np.zeros((n, 3), dtype=np.int32), 1
    x = normalize_hsb_view(tiles, win, size, d_mask, codes, fmt=fmt, out=out, shrink=shrink, resize=_view_resize(view, win, tiles), **route)
    return x, windows, HsbDraw(sigmas, codes)


# ---- Gaussian blur in the view pass (sl_normalize_blur_view; see include/stainlib_hip.h, augmentation/blur.py) ---------------------------

BlurDraw = collections.namedtuple("BlurDraw", ["sigmas", "codes"])
BlurDraw.__doc__ = """What the blur= stage of a batch method did: the (N,) float64 sigmas it used (given or drawn; None when the call was
given codes) and the (N, 9) int32 codes (w_0 .. w_8 per tile: augmentation.blur.blur_codes), both numpy.  The codes reproduce the call:
pass them back as blur_sigmas=."""


def _blur_codes_rows(codes, max_r=None):
    """The rows of an (N, 9) codes argument (no device needed): a device int32 tensor (taken as it is: the kernel gives a tile whose codes
    fail the rule the identity), or host integers, which are rule-checked here (ValueError) -- under max_r when that is given."""
    import numpy as np
    from .augmentation.blur import R, codes_ok
    what = "codes must hold (w_0 .. w_8) per tile: an (N, 9) int32 array (augmentation.blur.blur_codes)"
    if isinstance(codes, torch.Tensor) and codes.is_cuda:
        if codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[1] != R + 1 or not codes.is_contiguous():
            raise ValueError(what + ", contiguous")
        return int(codes.shape[0])
    try:
        arr = codes.numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
        if arr.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(what) from None
    if arr.ndim != 2 or arr.shape[1] != R + 1:
        raise ValueError(f"{what}, not one of shape {arr.shape}")
    bad = ~codes_ok(arr, R if max_r is None else max_r)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError(f"codes: tile {t} has {arr[t].tolist()}, which fails the rule: every w_k >= 0, w_0 + 2 (w_1 + .. + w_8) == 256"
                         + (f", no weight beyond max_r = {max_r}" if max_r is not None else ""))
    return int(arr.shape[0])


def _blur_max_r(max_r, codes):
    """max_r of a normalize_blur_view call (no device needed): 0 .. 8 as given; by default the largest radius of host codes (device codes
    are never read back: they need it)."""
    import numpy as np
    from .augmentation.blur import R, codes_radius
    if max_r is None:
        if isinstance(codes, torch.Tensor) and codes.is_cuda:
            raise ValueError("codes on the device need max_r=, the largest radius among them (0 .. 8): the launch is sized from it")
        arr = codes.numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
        return int(codes_radius(arr).max()) if arr.size else 0
    if isinstance(max_r, bool) or not isinstance(max_r, (int, np.integer)) or not 0 <= max_r <= R:
        raise ValueError(f"max_r must be an int in 0 .. {R}, not {max_r!r}")
    return int(max_r)


def normalize_blur_view(rgb, windows, size, d_mask, codes, max_r=None, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                        augment_background=False, params=None, shrink=1, fmt=None, out=None):
    """normalize_view of the BLURRED `full` in ONE pass (sl_normalize_blur_view): `full` is normalize_view's (the route arguments are the
    same), the blur is augmentation.blur.blur_reference with the tile's codes -- of the whole tile, its border replicated, and the view
    then cuts it: bit for bit blur_reference of `full`, then normalize_view of the result, without the pixels farther than max_r from the
    window being touched.  codes: (N, 9) int32 = (w_0 .. w_8) per tile (blur_codes).  Host codes are rule-checked (ValueError) and max_r
    defaults to their largest radius; a device tensor is taken as it is and needs max_r -- a tile whose codes fail the rule (a negative
    weight, a sum other than 256, a weight beyond max_r) gets the identity; nothing is synchronised.  shrink: normalize_view's, the box
    mean taken of the blurred bytes.  A tile whose fit failed: the view of its own blurred bytes."""
    import numpy as np
    _blur_codes_rows(codes)
    mr = _blur_max_r(max_r, codes)

    def codes_ok(n):
        if _blur_codes_rows(codes, mr) != n:
            raise ValueError(f"codes must have one row per tile ({n})")
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out, before_device=codes_ok, shrink=shrink)
    if isinstance(codes, torch.Tensor) and codes.is_cuda:
        if codes.device != rgb.device:
            raise ValueError(f"codes must be on {rgb.device}")
        c = codes
    else:
        arr = codes.numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
        c = torch.from_numpy(np.ascontiguousarray(arr.astype(np.int32))).to(rgb.device)
    _call("sl_normalize_blur_view", _ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask), int(shrink), mr, _ptr(M_src),
          _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), _ptr(c))
    return out


def _blur_sigmas_or_codes(blur_sigmas, n=None):
    """blur_sigmas= of a batch method (no device needed) -> (sigmas or None, codes): (N,) float sigmas -- or, to reproduce a call, the
    (N, 9) integer codes it returned (BlurDraw.codes), rule-checked.  ValueError."""
    import numpy as np
    from .augmentation.blur import R, blur_codes
    arr = None
    if not isinstance(blur_sigmas, torch.Tensor):
        try:
            arr = np.asarray(blur_sigmas)
        except (TypeError, ValueError):
            arr = None
    elif not blur_sigmas.is_cuda:
        arr = blur_sigmas.numpy()
    if arr is not None and arr.ndim == 2 and arr.dtype.kind in "iu" and arr.shape[1] == R + 1:
        _blur_codes_rows(arr)
        sigmas, codes = None, np.ascontiguousarray(arr.astype(np.int32))
    else:
        if arr is None:
            raise ValueError("blur_sigmas must hold one blur sigma per tile: an (N,) array (or the (N, 9) codes a call returned)")
        codes = blur_codes(arr)
        if codes.ndim != 2:
            raise ValueError("blur_sigmas must hold one blur sigma per tile: an (N,) array (or the (N, 9) codes a call returned)")
        sigmas = np.array(arr, dtype=np.float64)
    if n is not None and codes.shape[0] != n:
        raise ValueError(f"blur_sigmas must have one entry per tile ({n})")
    return sigmas, codes


def _blur_call(blur, blur_sigmas, tiles, view=None, hed=None, hsb=None):
    """The blur= / blur_sigmas= arguments of a batch method, checked without a device and before any draw (ValueError).  True when the call
    has a blur stage.  view, hed, hsb: the call's view=, hed= and hsb= -- a resizing or affine view and a colour stage do not go with it."""
    from .augmentation.blur import GaussianBlurAugmenter
    if blur is None:
        if blur_sigmas is not None:
            raise ValueError("blur_sigmas= goes with blur= (a GaussianBlurAugmenter)")
        return False
    if hed is not None or hsb is not None:
        raise ValueError("blur= does not go together with hed= or hsb=: a pass has one augmentation stage behind the route.  Chain them "
                         "instead: augment_batch(hsb=), then blur.transform_batch(view=, tensor_format=)")
    _no_affine(view, "the blur stage (blur=, GaussianBlurAugmenter.transform_batch(view=))",
               "blur first (blur.transform_batch), then take the uint8 result through TensorFormat.convert(view=)")
    if view is not None and getattr(view, "resizing", False):
        raise ValueError("blur= does not go with a resizing view (TileView(scale=)): the blurred view has fixed-size windows.  Blur first "
                         "(blur.transform_batch), then take the uint8 result through TensorFormat.convert(view=)")
    if not isinstance(blur, GaussianBlurAugmenter):
        raise ValueError("blur must be a stainlib_amd GaussianBlurAugmenter (its range is used)")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    if blur_sigmas is not None:
        _blur_sigmas_or_codes(blur_sigmas, int(tiles.shape[0]))
    return True


def _no_blur(blur, blur_sigmas, what):
    """ValueError for blur= in a call that has no blurred pass"""
    if blur is not None or blur_sigmas is not None:
        raise ValueError(f"blur= is not supported by {what}: take its uint8 result through blur.transform_batch(view=, tensor_format=)")


def blur_stage(tiles, blur, blur_sigmas, view, windows, route, fmt=None, out=None):
    """The blur= stage of the batch methods, behind their fit and their own draws, on arguments _blur_call / _view_call(draw=False) have
    accepted: the draws the caller left open -- blur.randomize_batch(N), THEN view.draw -- and ONE fused pass (normalize_blur_view).
    route: normalize_view's keyword arguments that name `full` ({}: the tiles themselves).  Without a view the result is the full tile,
    code 0.  -> (out, windows or None, BlurDraw)."""
    import numpy as np
    n = int(tiles.shape[0])
    if blur_sigmas is None:
        blur_sigmas = blur.randomize_batch(n)
    sigmas, codes = _blur_sigmas_or_codes(blur_sigmas, n)
    if view is not None:
        size, d_mask, windows, shrink = _view_call(view, windows, tiles)
        win = windows
    else:
        size, d_mask, windows, win, shrink = None, 0, None, np.zeros((n, 3), dtype=np.int32), 1
    x = normalize_blur_view(tiles, win, size, d_mask, codes, fmt=fmt, out=out, shrink=shrink, **route)
    return x, windows, BlurDraw(sigmas, codes)


# ---- the post stage: tone curve and additive noise on the bytes a call writes (sl_post_augment, sl_normalize_post_view; see
# ---- include/stainlib_hip.h, augmentation/noise.py) ---------------------------------------------------------------------------------------

PostDraw = collections.namedtuple("PostDraw", ["tone_params", "tone_tables", "noise_sigmas", "noise_codes"])
PostDraw.__doc__ = """What the tone= / noise= stage of a batch method did: the (N, 3) float64 (brightness, contrast, gamma) it used (given
or drawn; None when the call was given tables) and the (N, 256) uint8 tables they gave; the (N,) float64 noise sigmas (None when the call
was given codes) and the (N, 4) int32 codes (sq, k0, k1, mono), all numpy.  The fields of an absent augmenter are None.  The tables and
the codes reproduce the call: pass them back as tone_params= / noise_sigmas=."""


def _post_host(x):
    """a host array of an argument, or None for a device tensor (taken as it is, never read back)"""
    import numpy as np
    if isinstance(x, torch.Tensor):
        return None if x.is_cuda else x.numpy()
    return np.asarray(x)


def _post_tables_rows(tables):
    """The rows of an (N, 256) tables argument (no device needed): uint8, on the device (contiguous) or the host.  Any bytes are a table."""
    what = "tables must hold one tone curve per tile: an (N, 256) uint8 array (augmentation.noise.tone_table)"
    try:
        arr = _post_host(tables)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(what) from None
    if arr is None:
        if tables.dtype != torch.uint8 or tables.dim() != 2 or tables.shape[1] != 256 or not tables.is_contiguous():
            raise ValueError(what + ", contiguous")
        return int(tables.shape[0])
    if arr.dtype.name != "uint8" or arr.ndim != 2 or arr.shape[1] != 256:
        raise ValueError(f"{what}, not {arr.dtype} of shape {arr.shape}")
    return int(arr.shape[0])


def _post_codes_rows(codes):
    """The rows of an (N, 4) codes argument (no device needed): a device int32 tensor (taken as it is: the kernel clamps sq), or host
    integers that fit int32 and whose sq lies in [0, SQ_MAX] (ValueError)."""
    from .augmentation.noise import SQ_MAX
    what = "codes must hold (sq, k0, k1, mono) per tile: an (N, 4) int32 array (augmentation.noise.noise_codes)"
    try:
        arr = _post_host(codes)
        if arr is not None and arr.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(what) from None
    if arr is None:
        if codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[1] != 4 or not codes.is_contiguous():
            raise ValueError(what + ", contiguous")
        return int(codes.shape[0])
    if arr.ndim != 2 or arr.shape[1] != 4:
        raise ValueError(f"{what}, not one of shape {arr.shape}")
    if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
        raise ValueError("codes must fit int32 (the key words as their bit patterns)")
    if arr.size and (arr[:, 0].min() < 0 or arr[:, 0].max() > SQ_MAX):
        raise ValueError(f"codes: sq must lie in [0, {SQ_MAX}] (a sigma of 0 .. 64 bytes)")
    return int(arr.shape[0])


def _post_check(tables, codes, n=None):
    if tables is None and codes is None:
        raise ValueError("the post stage needs tables= (a tone curve per tile) or codes= (the noise codes per tile), or both")
    for x, rows, name in ((tables, _post_tables_rows, "tables"), (codes, _post_codes_rows, "codes")):
        if x is not None and rows(x) != n and n is not None:
            raise ValueError(f"{name} must have one row per tile ({n})")


def _post_device(x, dtype, device):
    import numpy as np
    if x is None:
        return None
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.device != device:
            raise ValueError(f"tables and codes must be on {device}")
        return x
    return torch.from_numpy(np.ascontiguousarray(_post_host(x).astype(dtype))).to(device)


def post_augment(u8, tables=None, codes=None, fmt=None, out=None):
    """The post stage on every full tile in one sweep (sl_post_augment): tables (N, 256) uint8 and / or codes (N, 4) int32 = (sq, k0, k1,
    mono) per tile (augmentation.noise: tone_table, noise_codes; host arrays are checked, a device tensor is taken as it is and sq is
    clamped by the kernel) -> (N,H,W,3) uint8, bit for bit augmentation.noise.post_reference; or with fmt (a stainlib_amd.TensorFormat)
    the (N,3,H,W) tensor, bit for bit fmt.convert of that image, written directly."""
    import numpy as np
    from .tensor_format import TensorFormat
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    _post_check(tables, codes)
    n, h, w = _check_tiles(u8)
    _post_check(tables, codes, n)
    t, c = _post_device(tables, np.uint8, u8.device), _post_device(codes, np.int32, u8.device)
    f, out = _image_out(out, u8, n, h, w, fmt, "post stage")
    _call("sl_post_augment", _ptr(u8), _ptr(out), n, h, w, _ptr(t), _ptr(c), _byref(f))
    return out


def normalize_post_view(rgb, windows, size, d_mask, tables=None, codes=None, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None,
                        alpha_beta=None, augment_background=False, params=None, shrink=1, resize=None, fmt=None, out=None):
    """post(normalize_view of `full`) in ONE pass (sl_normalize_post_view): `full` is normalize_view's (the route arguments are the same),
    post(.) is post_augment with the tile's table and codes on the view's OUTPUT -- bit for bit normalize_view to uint8, then
    post_augment of the result, then the conversion.  shrink, resize: normalize_view's; the stage acts behind them, per written pixel.  A
    tile whose fit failed: post(the view of its own bytes)."""
    import numpy as np
    _post_check(tables, codes)
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out,
        before_device=lambda n: _post_check(tables, codes, n), shrink=shrink, resize=resize)
    t, c = _post_device(tables, np.uint8, rgb.device), _post_device(codes, np.int32, rgb.device)
    mh, mw = (int(resize[0]), int(resize[1])) if resize is not None else (0, 0)
    _call("sl_normalize_post_view", _ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask), int(shrink), mh, mw, _ptr(M_src),
          _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), _ptr(t), _ptr(c))
    return out


_POST_CHAIN = "take the uint8 result (or view) first, then noise.transform_batch(u8, tensor_format=) / tone.transform_batch(u8, tensor_format=)"


def _noise_arg(noise, noise_sigmas, n=None):
    """noise_sigmas= of a batch method (no device needed) -> (sigmas or None, codes): (N,) float sigmas under the augmenter's current key
    -- or, to reproduce a call, the (N, 4) integer codes it returned (PostDraw.noise_codes; a device tensor is taken as it is).  ValueError."""
    import numpy as np
    what = "noise_sigmas must hold one noise sigma per tile: an (N,) array (or the (N, 4) codes a call returned)"
    try:
        arr = _post_host(noise_sigmas)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(what) from None
    if arr is None or (arr.ndim == 2 and arr.dtype.kind in "iu"):
        rows, sigmas = _post_codes_rows(noise_sigmas), None
        codes = noise_sigmas if arr is None else np.ascontiguousarray(arr.astype(np.int32))
    else:
        if arr.ndim != 1:
            raise ValueError(what)
        codes = noise.codes(arr, None)
        rows, sigmas = codes.shape[0], np.array(arr, dtype=np.float64)
    if n is not None and rows != n:
        raise ValueError(f"noise_sigmas must have one entry per tile ({n})")
    return sigmas, codes


def _tone_arg(tone_params, n=None):
    """tone_params= of a batch method (no device needed) -> (params or None, tables): (N, 3) float (brightness, contrast, gamma) -- or,
    to reproduce a call, the (N, 256) uint8 tables it returned (PostDraw.tone_tables; a device tensor is taken as it is).  ValueError."""
    import numpy as np
    from .augmentation.noise import tone_tables
    what = "tone_params must hold (brightness, contrast, gamma) per tile: an (N, 3) array (or the (N, 256) uint8 tables a call returned)"
    try:
        arr = _post_host(tone_params)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(what) from None
    if arr is None or (arr.ndim == 2 and arr.shape[1] == 256):
        rows, params, tables = _post_tables_rows(tone_params), None, tone_params if arr is None else np.ascontiguousarray(arr)
    else:
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise ValueError(what)
        tables = tone_tables(arr)
        rows, params = tables.shape[0], np.array(arr, dtype=np.float64)
    if n is not None and rows != n:
        raise ValueError(f"tone_params must have one row per tile ({n})")
    return params, tables


def _post_call(noise, tone, noise_sigmas, tone_params, tiles, view=None, hed=None, hsb=None, blur=None):
    """The noise= / tone= / noise_sigmas= / tone_params= arguments of a batch method, checked without a device and before any draw
    (ValueError).  True when the call has a post stage.  view, hed, hsb, blur: the call's other stages -- an affine or elastic view and
    a stage on source pixels do not go with it."""
    from .augmentation.noise import GaussianNoiseAugmenter, ToneCurveAugmenter
    if noise is None and noise_sigmas is not None:
        raise ValueError("noise_sigmas= goes with noise= (a GaussianNoiseAugmenter)")
    if tone is None and tone_params is not None:
        raise ValueError("tone_params= goes with tone= (a ToneCurveAugmenter)")
    if noise is None and tone is None:
        return False
    if hed is not None or hsb is not None or blur is not None:
        raise ValueError("noise= / tone= do not go together with hed=, hsb= or blur=: those act on source pixels, the post stage on the "
                         "written ones, and a pass has one augmentation stage.  Chain them instead: " + _POST_CHAIN)
    if _is_affine(view) or _is_elastic(view):
        raise ValueError(f"an affine or elastic view ({view!r}) is not supported by the post stage (noise=, tone=): its write side is "
                         "bilinear.  Chain them instead: " + _POST_CHAIN)
    if noise is not None and not isinstance(noise, GaussianNoiseAugmenter):
        raise ValueError("noise must be a stainlib_amd GaussianNoiseAugmenter (its range and channel mode are used)")
    if tone is not None and not isinstance(tone, ToneCurveAugmenter):
        raise ValueError("tone must be a stainlib_amd ToneCurveAugmenter (its ranges are used)")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n = int(tiles.shape[0])
    if tone_params is not None:
        _tone_arg(tone_params, n)
    if noise_sigmas is not None:
        _noise_arg(noise, noise_sigmas, n)
    return True


def _no_post(noise, tone, noise_sigmas, tone_params, what):
    """ValueError for noise= / tone= in a call that has no post stage"""
    if noise is not None or tone is not None or noise_sigmas is not None or tone_params is not None:
        raise ValueError(f"noise= / tone= are not supported by {what}: " + _POST_CHAIN)


def post_stage(tiles, noise, tone, noise_sigmas, tone_params, view, windows, route, fmt=None, out=None):
    """The noise= / tone= stage of the batch methods, behind their fit and their own draws, on arguments _post_call /
    _view_call(draw=False) have accepted: the draws the caller left open -- tone.randomize_batch(N), THEN noise.randomize_batch(N), THEN
    view.draw -- and ONE fused pass (normalize_post_view).  route: normalize_view's keyword arguments that name `full` ({}: the tiles
    themselves).  Without a view the result is the full tile, code 0.  -> (out, windows or None, PostDraw)."""
    import numpy as np
    n = int(tiles.shape[0])
    params = tables = sigmas = codes = None
    if tone is not None:
        params, tables = tone.randomize_batch(n) if tone_params is None else _tone_arg(tone_params, n)
    if noise is not None:
        sigmas, codes = noise.randomize_batch(n) if noise_sigmas is None else _noise_arg(noise, noise_sigmas, n)
    if view is not None:
        size, d_mask, windows, shrink = _view_call(view, windows, tiles)
        win = windows
    else:
        size, d_mask, windows, win, shrink = None, 0, None, np.zeros((n, 3), dtype=np.int32), 1
    x = normalize_post_view(tiles, win, size, d_mask, tables, codes, fmt=fmt, out=out, shrink=shrink,
                            resize=_view_resize(view, win, tiles), **route)
    return x, windows, PostDraw(params, tables, sigmas, codes)


def _view_call(view, windows, tiles, draw=True):
    """(size, d_mask, windows, shrink) of the view= / windows= pair of a batch method, checked without a device (ValueError): the windows
    as given, or drawn (TileView.draw; draw=False: left None for a later call)."""
    from .tile_view import ElasticWindows, TileView
    if not isinstance(view, TileView) and not _is_affine(view):
        raise ValueError("view must be a stainlib_amd.TileView" + (" (windows= goes with view=)" if view is None else ""))
    if isinstance(windows, ElasticWindows) and not _is_elastic(view):
        raise ValueError(f"these windows are the ElasticWindows of an elastic view and do not go with {view!r}: pass them with the "
                         "TileElastic that drew them, or windows.affine for the affine part alone")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in tiles.shape[:3])
    oh, ow = view.out_size(h, w)
    if _is_elastic(view):                                    # ElasticWindows(affine, field); view_pass makes the call
        if windows is not None:
            affine, field = _elastic_parts(windows)
            max_r, max_d = _elastic_bound(view, windows)
            _affine_windows(affine, n, h, w, view.size, max_r)
            _elastic_field(field, n, (oh, ow), view.cell, max_d)
        elif draw:
            windows = view.draw(n, h, w)
        return view.size, 0, windows, 1
    if _is_affine(view):                                     # (cy, cx, a00, a01, a10, a11) per tile; _view_pass makes the call
        if windows is not None:
            _affine_windows(windows, n, h, w, view.size, _affine_bound(view, windows))
        elif draw:
            windows = view.draw(n, h, w)
        return view.size, 0, windows, 1
    if windows is not None:
        _view_windows(windows, n, h, w, oh, ow, view.d_mask, view.shrink, _view_resize(view, windows, tiles))
    elif draw:
        windows = view.draw(n, h, w)
    return view.size, view.d_mask, windows, view.shrink


def _view_resize(view, windows, tiles):
    """resize= of the normalize_view call behind a batch method's view= (no device needed): None unless the view resizes
    (TileView(scale=)); else the bound of the window sides -- of host windows their own largest sides, of device windows (never read
    back) or none yet the largest the view can draw (TileView.window_bound)."""
    if view is None or not view.resizing:
        return None
    return _view_resize_hw(view, windows, *(int(v) for v in tiles.shape[1:3]))


def _view_resize_hw(view, windows, h, w):
    """_view_resize on the tile size itself (TileView.apply has planes, not tiles)"""
    import numpy as np
    if view is None or not view.resizing:
        return None
    if windows is None or (isinstance(windows, torch.Tensor) and windows.is_cuda):
        return view.window_bound(h, w)
    try:
        win = windows.numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if win.dtype.kind not in "iu" or win.ndim != 2 or win.shape[1] != 5 or win.shape[0] == 0:
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        return view.window_bound(h, w)                       # (_resize_windows says what is wrong with them)
    return max(1, min(h, int(win[:, 3].max()))), max(1, min(w, int(win[:, 4].max())))


def route_stage(tiles, fit, route, fmt=None, out=None, view=None, windows=None, hed=None, hsb=None, blur=None, post=None, recipe=None):
    """The tail of the batch methods, behind their fit and their own draws, on arguments _jitter_args / _view_call(draw=False) / _hed_call
    have accepted: ONE pass over the tiles and the tuple the method returns, (out, M_src, maxC_src, status[, windows][, HedDraw]).
    fit: the fit's (M_src, maxC_src, status); route: the other arguments that name `full` (M_tgt, maxC_tgt and, for a jitter, alpha_beta
    and augment_background).  hed = (HedColorAugmenter, hed_sigmas, hed_biases): hed_stage; else with a view: normalize_view, the
    windows drawn here if not given; else normalize_jitter.  hsb = (HsbColorAugmenter, hsb_sigmas) that _hsb_call has accepted (never
    with hed): hsb_stage, and HsbDraw at the end of the tuple.  blur = (GaussianBlurAugmenter, blur_sigmas) that _blur_call has accepted
    (never with hed or hsb): blur_stage, and BlurDraw at the end of the tuple.  post = (noise, tone, noise_sigmas, tone_params) that
    _post_call has accepted (never with hed, hsb or blur): post_stage, and PostDraw at the end of the tuple.  recipe = (Recipe,
    recipe_draw) that _recipe_call has accepted (never with any of the others or a view): recipe_stage, and (out, M_src, maxC_src,
    status, RecipeDraw)."""
    M, maxC, status = fit
    route = dict(M_src=M, maxC_src=maxC, **route)
    if recipe is not None:
        x, draw = recipe_stage(tiles, *recipe, route, fmt=fmt, out=out)
        return x, M, maxC, status, draw
    if post is not None:
        x, windows, draw = post_stage(tiles, *post, view, windows, route, fmt=fmt, out=out)
        return (x, M, maxC, status) + ((windows,) if view is not None else ()) + (draw,)
    if blur is not None:
        x, windows, draw = blur_stage(tiles, *blur, view, windows, route, fmt=fmt, out=out)
        return (x, M, maxC, status) + ((windows,) if view is not None else ()) + (draw,)
    if hsb is not None:
        x, windows, draw = hsb_stage(tiles, *hsb, view, windows, route, fmt=fmt, out=out)
        return (x, M, maxC, status) + ((windows,) if view is not None else ()) + (draw,)
    if hed is not None:
        x, windows, draw = hed_stage(tiles, *hed, view, windows, route, fmt=fmt, out=out)
        return (x, M, maxC, status) + ((windows,) if view is not None else ()) + (draw,)
    if view is not None:
        x, windows = view_pass(tiles, view, windows, fmt=fmt, out=out, **route)
        return x, M, maxC, status, windows
    return normalize_jitter(tiles, fmt=fmt, out=out, **route), M, maxC, status


def view_pass(tiles, view, windows, fmt=None, out=None, **route):
    """The ONE pass behind a view= argument, dispatched on the view's type -> (out, windows): the windows as given or drawn here
    (_view_call), then normalize_view_elastic for a TileElastic, normalize_view_affine for a TileAffine, normalize_view (its shrink, its resizing bound) for a TileView.  route:
    the keyword arguments that name `full` ({}: the tiles themselves)."""
    size, d_mask, windows, shrink = _view_call(view, windows, tiles)
    if _is_elastic(view):
        max_r, max_d = _elastic_bound(view, windows)
        return normalize_view_elastic(tiles, windows.affine, windows.field, size, view.cell, max_r, max_d, view.fill, fmt=fmt, out=out,
                                      **route), windows
    if _is_affine(view):
        return normalize_view_affine(tiles, windows, size, _affine_bound(view, windows), view.fill, fmt=fmt, out=out, **route), windows
    return normalize_view(tiles, windows, size, d_mask, fmt=fmt, out=out, shrink=shrink, resize=_view_resize(view, windows, tiles),
                          **route), windows


# ---- the one-pass recipe: a colour stage, any view and the post stage together (sl_normalize_stages_view*; see include/stainlib_hip.h) ------

RecipeDraw = collections.namedtuple("RecipeDraw", ["windows", "color", "post"])
RecipeDraw.__doc__ = """What a recipe= call did: `windows` as the view's own call returns them ((N, 3 | 5 | 6) int32 or ElasticWindows; None
without a view), `color` the HedDraw or HsbDraw of its colour stage (or None) and `post` the PostDraw of its tone / noise stage (or None).
Passed back as recipe_draw= with the same Recipe it reproduces the call."""

_STAGE_KEYS = ("hed_sigma", "hed_bias", "hed_applied", "skimage_mode", "hsb_codes", "tables", "codes")


def _stages_check(n, hed_sigma=None, hed_bias=None, hed_applied=None, skimage_mode=0, hsb_codes=None, tables=None, codes=None):
    """The stage arguments of normalize_stages_view* (no device needed; ValueError): at most one colour stage -- the HED triple of
    normalize_hed_view (skimage_mode 0 only) or the codes of normalize_hsb_view --, the tables / codes of normalize_post_view, at
    least one stage, one row per tile each."""
    hed = [x is not None for x in (hed_sigma, hed_bias, hed_applied)]
    if any(hed) and not all(hed):
        raise ValueError("hed_sigma, hed_bias and hed_applied go together: the (N, 3) sigmas and biases and the (N,) decision per tile")
    if all(hed) and hsb_codes is not None:
        raise ValueError("a recipe has one colour stage: the HED triple or hsb_codes, not both")
    if skimage_mode != _ffi.HED_SKIMAGE_018:
        raise ValueError(f"skimage_mode {skimage_mode!r}: the recipe's HED stage runs in the kernel, which knows skimage_mode '0.18' (0) only")
    if not any(hed) and hsb_codes is None and tables is None and codes is None:
        raise ValueError("a recipe call needs a stage: the HED triple, hsb_codes=, tables= or codes=")
    if all(hed):
        for x, what in ((hed_sigma, "hed_sigma"), (hed_bias, "hed_bias")):
            if _hed_rows(x, what) != n:
                raise ValueError(f"{what} must have one row per tile ({n})")
    if hsb_codes is not None and _hsb_codes_rows(hsb_codes) != n:
        raise ValueError(f"hsb_codes must have one row per tile ({n})")
    if tables is not None or codes is not None:
        _post_check(tables, codes, n)


def _stages_upload(n, dev, hed_sigma=None, hed_bias=None, hed_applied=None, skimage_mode=0, hsb_codes=None, tables=None, codes=None):
    """The stages _stages_check has accepted on the device -> ((reference to the SlViewStages,), what must outlive the call)."""
    import numpy as np
    keep = [
        _f64(hed_sigma, (n, 3), dev) if hed_sigma is not None else None,
        _f64(hed_bias, (n, 3), dev) if hed_bias is not None else None,
        torch.as_tensor(hed_applied, device=dev).to(torch.int32).reshape(n).contiguous() if hed_applied is not None else None,
        _hsb_codes_device(hsb_codes, n, dev) if hsb_codes is not None else None,
        _post_device(tables, np.uint8, dev),
        _post_device(codes, np.int32, dev),
    ]
    ptr = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
    st = _ffi.SlViewStages(C.sizeof(_ffi.SlViewStages), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), int(skimage_mode), ptr(keep[3]), ptr(keep[4]),
                           ptr(keep[5]))
    keep.append(st)
    return (C.byref(st),), keep


def normalize_stages_view(rgb, windows, size, d_mask, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                          augment_background=False, params=None, fmt=None, out=None, shrink=1, resize=None, **stages):
    """convert(post(view(colour(full)))) in ONE pass on a fixed-size, box-shrinking or resizing view (sl_normalize_stages_view): `full`,
    windows, size, d_mask, shrink, resize, fmt, out are normalize_view's.  stages (keywords): hed_sigma, hed_bias, hed_applied[,
    skimage_mode=0] -- normalize_hed_view's stage on SOURCE pixels -- or hsb_codes -- normalize_hsb_view's --; tables, codes --
    normalize_post_view's stage on WRITTEN pixels, p counted in the view's output.  At least one stage, at most one colour stage
    (ValueError).  Bit for bit the chain of those calls; an absent stage is the identity."""
    bad = sorted(set(stages) - set(_STAGE_KEYS))
    if bad:
        raise TypeError(f"normalize_stages_view got unexpected keyword arguments {bad}")
    n, h, w, oh, ow, win, M_src, maxC_src, M_tgt, maxC_tgt, ab, f, out = _view_prepare(
        rgb, windows, size, d_mask, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, params, fmt, out,
        before_device=lambda n: _stages_check(n, **stages), shrink=shrink, resize=resize)
    st, keep = _stages_upload(n, rgb.device, **stages)
    mh, mw = (int(resize[0]), int(resize[1])) if resize is not None else (0, 0)
    _call("sl_normalize_stages_view", _ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask), int(shrink), mh, mw, _ptr(M_src),
          _ptr(maxC_src), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(ab), 1 if augment_background else 0, _byref(params), _byref(f), *st)
    del keep
    return out


def normalize_stages_view_affine(rgb, windows, size, max_r, fill=255, M_src=None, maxC_src=None, M_tgt=None, maxC_tgt=None, alpha_beta=None,
                                 augment_background=False, params=None, fmt=None, out=None, **stages):
    """normalize_stages_view on an affine view (sl_normalize_stages_view_affine): windows, size, max_r, fill and the rest are
    normalize_view_affine's, stages normalize_stages_view's.  The fill is in OUTPUT space: it does not take the colour stage and it does
    take the post stage, and so does a tile written entirely as fill (device windows beyond max_r)."""
    bad = sorted(set(stages) - set(_STAGE_KEYS))
    if bad:
        raise TypeError(f"normalize_stages_view_affine got unexpected keyword arguments {bad}")
    return _view_affine_call(stages, rgb, windows, size, max_r, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params,
                             fmt, out)


def normalize_stages_view_elastic(rgb, windows, field, size, cell, max_r, max_d, fill=255, M_src=None, maxC_src=None, M_tgt=None,
                                  maxC_tgt=None, alpha_beta=None, augment_background=False, params=None, fmt=None, out=None, **stages):
    """normalize_stages_view on an elastic view (sl_normalize_stages_view_elastic): windows, field, size, cell, max_r, max_d, fill and the
    rest are normalize_view_elastic's, stages and the fill's treatment normalize_stages_view_affine's."""
    bad = sorted(set(stages) - set(_STAGE_KEYS))
    if bad:
        raise TypeError(f"normalize_stages_view_elastic got unexpected keyword arguments {bad}")
    return _view_elastic_call(stages, rgb, windows, field, size, cell, max_r, max_d, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                              augment_background, params, fmt, out)


def _recipe_draw_check(recipe, draw, tiles):
    """recipe_draw= against its recipe (no device needed; ValueError): a complete RecipeDraw whose parts match the recipe's stages, each
    part through the checker of its own keyword (_view_call, _hed_rows, _hsb_codes_rows, _tone_arg, _noise_arg)."""
    from .augmentation.augmenter import HedColorAugmenter
    n = int(tiles.shape[0])
    if not isinstance(draw, RecipeDraw):
        raise ValueError("recipe_draw must be the engine.RecipeDraw(windows, color, post) a recipe= call returned")
    if (recipe.view is None) != (draw.windows is None):
        raise ValueError("recipe_draw.windows does not match the recipe: " + ("the recipe has no view" if recipe.view is None else
                                                                               f"the recipe's view ({recipe.view!r}) needs its windows"))
    if recipe.view is not None:
        _view_call(recipe.view, draw.windows, tiles, draw=False)
    if recipe.color is None:
        if draw.color is not None:
            raise ValueError("recipe_draw.color does not match the recipe: the recipe has no colour stage")
    elif isinstance(recipe.color, HedColorAugmenter):
        if not isinstance(draw.color, HedDraw):
            raise ValueError("recipe_draw.color does not match the recipe: a HedColorAugmenter needs the engine.HedDraw the call returned")
        for x, what in ((draw.color.sigmas, "recipe_draw.color.sigmas"), (draw.color.biases, "recipe_draw.color.biases")):
            if _hed_rows(x, what) != n:
                raise ValueError(f"{what} must have one row per tile ({n})")
    else:
        if not isinstance(draw.color, HsbDraw):
            raise ValueError("recipe_draw.color does not match the recipe: an HsbColorAugmenter needs the engine.HsbDraw the call returned")
        if _hsb_codes_rows(draw.color.codes) != n:
            raise ValueError(f"recipe_draw.color.codes must have one row per tile ({n})")
    if recipe.noise is None and recipe.tone is None:
        if draw.post is not None:
            raise ValueError("recipe_draw.post does not match the recipe: the recipe has no tone or noise stage")
        return
    if not isinstance(draw.post, PostDraw):
        raise ValueError("recipe_draw.post does not match the recipe: tone= / noise= need the engine.PostDraw the call returned")
    if (recipe.tone is None) != (draw.post.tone_tables is None):
        raise ValueError("recipe_draw.post.tone_tables does not match the recipe's tone stage")
    if (recipe.noise is None) != (draw.post.noise_codes is None):
        raise ValueError("recipe_draw.post.noise_codes does not match the recipe's noise stage")
    if recipe.tone is not None:
        _tone_arg(draw.post.tone_tables, n)
    if recipe.noise is not None:
        _noise_arg(recipe.noise, draw.post.noise_codes, n)


def _recipe_call(recipe, recipe_draw, tiles, **others):
    """The recipe= / recipe_draw= arguments of a batch method, checked without a device and before any draw (ValueError).  True when the
    call has a recipe.  others: the call's own view and stage keywords by name -- none of them goes with a recipe."""
    from .recipe import Recipe
    if recipe is None:
        if recipe_draw is not None:
            raise ValueError("recipe_draw= goes with recipe= (the stainlib_amd.Recipe that made it)")
        return False
    if not isinstance(recipe, Recipe):
        raise ValueError("recipe must be a stainlib_amd.Recipe")
    given = [k for k, v in others.items() if v is not None]
    if given:
        raise ValueError("recipe= does not go together with " + ", ".join(k + "=" for k in given) + ": the recipe holds the call's view and "
                         "every stage (Recipe(view=, color=, noise=, tone=)); to reproduce a call pass the RecipeDraw it returned as recipe_draw=")
    if not (isinstance(tiles, torch.Tensor) and tiles.dim() == 4 and tiles.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    if recipe_draw is not None:
        _recipe_draw_check(recipe, recipe_draw, tiles)
    elif recipe.view is not None:
        _view_call(recipe.view, None, tiles, draw=False)
    return True


def _no_recipe(recipe, recipe_draw, what, instead):
    """ValueError for recipe= in a call that has no recipe"""
    if recipe is not None or recipe_draw is not None:
        raise ValueError(f"recipe= is not supported by {what}: {instead}")


def recipe_stage(tiles, recipe, recipe_draw, route, fmt=None, out=None):
    """The recipe= stage of the batch methods, behind their fit and their own draws, on arguments _recipe_call has accepted: the draws --
    color.randomize_batch(N), THEN tone.randomize_batch(N), THEN noise.randomize_batch(N), THEN view.draw -- or the parts of recipe_draw
    in their place, the HED cutoff decision (hed_decide, also on a replay) and ONE fused pass (normalize_stages_view*, by the view's
    type).  route: normalize_view's keyword arguments that name `full` ({}: the tiles themselves).  Without a view the result is the
    full tile, code 0.  -> (out, RecipeDraw)."""
    import numpy as np
    from .augmentation.augmenter import HedColorAugmenter
    from .augmentation.hsb import hsb_codes
    n = int(tiles.shape[0])
    view, color, noise, tone = recipe.view, recipe.color, recipe.noise, recipe.tone
    is_hed = isinstance(color, HedColorAugmenter)
    stages, cdraw, pdraw = {}, None, None
    if color is not None:
        if is_hed:
            sigmas, biases = color.randomize_batch(n) if recipe_draw is None else (recipe_draw.color.sigmas, recipe_draw.color.biases)
        elif recipe_draw is None:
            sigmas = np.array(color.randomize_batch(n), dtype=np.float64)
            codes = hsb_codes(sigmas)
        else:
            sigmas, codes = recipe_draw.color.sigmas, recipe_draw.color.codes
    if tone is not None or noise is not None:
        params = tables = nsig = ncodes = None
        if tone is not None:
            params, tables = tone.randomize_batch(n) if recipe_draw is None else (recipe_draw.post.tone_params,
                                                                                   _tone_arg(recipe_draw.post.tone_tables, n)[1])
        if noise is not None:
            nsig, ncodes = noise.randomize_batch(n) if recipe_draw is None else (recipe_draw.post.noise_sigmas,
                                                                                 _noise_arg(noise, recipe_draw.post.noise_codes, n)[1])
        pdraw = PostDraw(params, tables, nsig, ncodes)
        stages.update(tables=tables, codes=ncodes)
    windows = None
    if view is not None:
        size, d_mask, windows, shrink = _view_call(view, recipe_draw.windows if recipe_draw is not None else None, tiles)
    if color is not None:
        if is_hed:
            applied = hed_decide(tiles, color._cutoff_range, **route)
            cdraw = HedDraw(sigmas, biases, applied)
            stages.update(hed_sigma=sigmas, hed_bias=biases, hed_applied=applied, skimage_mode=color._skimage_mode)
        else:
            cdraw = HsbDraw(sigmas, codes)
            stages.update(hsb_codes=codes)
    if view is None:
        x = normalize_stages_view(tiles, np.zeros((n, 3), dtype=np.int32), None, 0, fmt=fmt, out=out, **route, **stages)
    elif _is_elastic(view):
        max_r, max_d = _elastic_bound(view, windows)
        x = normalize_stages_view_elastic(tiles, windows.affine, windows.field, size, view.cell, max_r, max_d, view.fill, fmt=fmt, out=out,
                                          **route, **stages)
    elif _is_affine(view):
        x = normalize_stages_view_affine(tiles, windows, size, _affine_bound(view, windows), view.fill, fmt=fmt, out=out, **route, **stages)
    else:
        x = normalize_stages_view(tiles, windows, size, d_mask, fmt=fmt, out=out, shrink=shrink, resize=_view_resize(view, windows, tiles),
                                  **route, **stages)
    return x, RecipeDraw(windows, cdraw, pdraw)


def _fit(fn_name, op, rgb, params, ws, with_sweeps=False):
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M = torch.empty((n, 2, 3), dtype=torch.float64, device=dev)
    maxC = torch.empty((n, 2), dtype=torch.float64, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    wsb = _scratch(ws, op, n, h, w, dev, params)
    sweeps = (torch.empty((n,), dtype=torch.int32, device=dev),) if with_sweeps else ()
    _call(fn_name, _ptr(rgb), n, h, w, _params(params), _ptr(M), _ptr(maxC), _ptr(status), *map(_ptr, sweeps), _ptr(wsb), wsb.numel())
    return (M, maxC, status) + sweeps


def macenko_fit(rgb, params=None, ws=None):
    """Per-tile Macenko stain matrix (N,2,3) f64, 99th-percentile concentrations (N,2) f64, status (N,) i32."""
    return _fit("sl_macenko_fit", _ffi.OP_MACENKO_FIT, rgb, params, ws)


def vahadane_fit(rgb, params=None, ws=None):
    """As macenko_fit with the sparse-NMF dictionary; also returns sweeps used per tile."""
    return _fit("sl_vahadane_fit", _ffi.OP_VAHADANE_FIT, rgb, params, ws, with_sweeps=True)


def _transform(fn_name, op, rgb, M_tgt, maxC_tgt, params, out, ws):
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M_tgt = _f64(M_tgt, (2, 3), dev)
    maxC_tgt = _f64(maxC_tgt, (2,), dev)
    if out is None:
        out = torch.empty_like(rgb)
    M = torch.empty((n, 2, 3), dtype=torch.float64, device=dev)
    maxC = torch.empty((n, 2), dtype=torch.float64, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    wsb = _scratch(ws, op, n, h, w, dev, params)
    _call(fn_name, _ptr(rgb), _ptr(out), n, h, w, _params(params), _ptr(M_tgt), _ptr(maxC_tgt), _ptr(M), _ptr(maxC), _ptr(status),
          _ptr(wsb), wsb.numel())
    return out, M, maxC, status


def macenko_transform(rgb, M_tgt, maxC_tgt, params=None, out=None, ws=None):
    """Batched ExtractiveStainNormalizer('macenko').transform -> (out, M_src, maxC_src, status)."""
    return _transform("sl_macenko_transform", _ffi.OP_MACENKO_TRANSFORM, rgb, M_tgt, maxC_tgt, params, out, ws)


def vahadane_transform(rgb, M_tgt, maxC_tgt, params=None, out=None, ws=None):
    return _transform("sl_vahadane_transform", _ffi.OP_VAHADANE_TRANSFORM, rgb, M_tgt, maxC_tgt, params, out, ws)


def hed_augment(rgb, sigma, bias, cutoff=(0.05, 0.95), skimage_mode=0, out=None, ws=None, want_sums=False):
    """Batched HedColorAugmenter.transform for uint8 tiles -> (out, applied (N,) i32)[, exact byte sums (N,) int64]."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    sigma = _f64(sigma, (n, 3), dev)
    bias = _f64(bias, (n, 3), dev)
    if out is None:
        out = torch.empty_like(rgb)
    applied = torch.empty((n,), dtype=torch.int32, device=dev)
    wsb = _scratch(ws, _ffi.OP_HED_AUGMENT, n, h, w, dev)
    _call("sl_hed_augment", _ptr(rgb), _ptr(out), n, h, w, _ptr(sigma), _ptr(bias), float(cutoff[0]), float(cutoff[1]), int(skimage_mode),
          _ptr(applied), _ptr(wsb), wsb.numel())
    if want_sums:
        return out, applied, wsb[:8 * n].view(torch.int64).clone()
    return out, applied


def hed_augment_float(patches, sigma, bias, cutoff=(0.05, 0.95), skimage_mode=0):
    """Float branch: (N,H,W,3) float64 CUDA tensor in [0,1] -> (out float64, applied)."""
    if not (patches.is_cuda and patches.dtype == torch.float64 and patches.dim() == 4 and patches.is_contiguous()):
        raise ValueError("expected a contiguous CUDA float64 tensor of shape (N, H, W, 3)")
    n, h, w, _ = patches.shape
    dev = patches.device
    sigma = _f64(sigma, (n, 3), dev)
    bias = _f64(bias, (n, 3), dev)
    out = torch.empty_like(patches)
    applied = torch.empty((n,), dtype=torch.int32, device=dev)
    wsb = torch.empty(max(8 * n, 256), dtype=torch.uint8, device=dev)
    _call("sl_hed_augment_f64", _ptr(patches), _ptr(out), n, h, w, _ptr(sigma), _ptr(bias), float(cutoff[0]), float(cutoff[1]),
          int(skimage_mode), _ptr(applied), _ptr(wsb), wsb.numel())
    return out, applied


def rgb_to_od(rgb):
    """convert_RGB_to_OD materialised: (N,H,W,3) float64."""
    n, h, w = _check_tiles(rgb)
    od = torch.empty((n, h, w, 3), dtype=torch.float64, device=rgb.device)
    _call("sl_rgb_to_od", _ptr(rgb), n, h, w, _ptr(od))
    return od


def stain_augment(rgb, M, alpha_beta, augment_background=False, params=None, out=None):
    """Batched StainAugmentor.pop given per-tile M (N,2,3) and (alpha0,beta0,alpha1,beta1) (N,4)."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M = _f64(M, (n, 2, 3), dev)
    ab = _f64(alpha_beta, (n, 4), dev)
    if out is None:
        out = torch.empty_like(rgb)
    _call("sl_stain_augment", _ptr(rgb), _ptr(out), n, h, w, _ptr(M), _ptr(ab), 1 if augment_background else 0, _params(params))
    return out


def grayscale_augment(rgb, alpha_beta, out=None):
    """GrayscaleAugmentor.pop on a batch: alpha_beta (n, 2) -> (n, H, W, 3) uint8 with three equal channels."""
    n, h, w = _check_tiles(rgb)
    ab = _f64(alpha_beta, (n, 2), rgb.device)
    if out is None:
        out = torch.empty_like(rgb)
    _call("sl_grayscale_augment", _ptr(rgb), _ptr(out), n, h, w, _ptr(ab))
    return out


def tissue_mask(rgb, luminosity_threshold=0.8, want_mask=True):
    """(mask (N,H,W) uint8 or None, counts (N,) int64)."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_mask else None
    counts = torch.empty((n,), dtype=torch.int64, device=dev)
    _call("sl_tissue_mask", _ptr(rgb), n, h, w, float(luminosity_threshold), _ptr(mask), _ptr(counts))
    return mask, counts


def concentrations(rgb, M, lasso_lambda=0.01):
    """get_concentrations materialised: (N, H*W, 2) float32."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    M = _f64(M, (n, 2, 3), dev)
    Cout = torch.empty((n, h * w, 2), dtype=torch.float32, device=dev)
    _call("sl_concentrations", _ptr(rgb), n, h, w, _ptr(M), float(lasso_lambda), _ptr(Cout))
    return Cout


def od_to_rgb(od):
    """convert_OD_to_RGB on a float64 CUDA tensor of any shape -> (uint8 tensor of the same shape, negative flag (1,) i32)."""
    if not (od.is_cuda and od.dtype == torch.float64 and od.is_contiguous()):
        raise ValueError("expected a contiguous CUDA float64 tensor")
    out = torch.empty(od.shape, dtype=torch.uint8, device=od.device)
    neg = torch.zeros((1,), dtype=torch.int32, device=od.device)
    _call("sl_od_to_rgb", _ptr(od), od.numel(), _ptr(out), _ptr(neg))
    return out, neg


# ---- OpenCV 8-bit Lab family (lab.hip) ---------------------------------------------------------------
def rgb_to_lab8(rgb):
    """cv2.cvtColor(COLOR_RGB2LAB) on uint8 tiles -> (N,H,W,3) uint8."""
    n, h, w = _check_tiles(rgb)
    out = torch.empty_like(rgb)
    _call("sl_rgb_to_lab8", _ptr(rgb), _ptr(out), n, h, w)
    return out


def lab8_to_rgb(lab):
    """cv2.cvtColor(COLOR_LAB2RGB) on uint8 tiles."""
    n, h, w = _check_tiles(lab)
    out = torch.empty_like(lab)
    _call("sl_lab8_to_rgb", _ptr(lab), _ptr(out), n, h, w)
    return out


def lab_split(rgb):
    """lab_split: three (N,H,W) float32 planes L8/2.55, a8-128, b8-128."""
    n, h, w = _check_tiles(rgb)
    I1, I2, I3 = (torch.empty((n, h, w), dtype=torch.float32, device=rgb.device) for _ in range(3))
    _call("sl_lab_split", _ptr(rgb), n, h, w, _ptr(I1), _ptr(I2), _ptr(I3))
    return I1, I2, I3


def lab_merge(I1, I2, I3):
    """merge_back: three (N,H,W) planes of one float dtype (float32 or float64) -> (N,H,W,3) uint8 RGB."""
    if not (I1.dtype == I2.dtype == I3.dtype and I1.dtype in (torch.float32, torch.float64) and I1.shape == I2.shape == I3.shape
            and I1.dim() == 3 and all(t.is_cuda and t.is_contiguous() for t in (I1, I2, I3))):
        raise ValueError("expected three contiguous CUDA (N, H, W) planes of one float dtype")
    n, h, w = I1.shape
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=I1.device)
    _call("sl_lab_merge", _ptr(I1), _ptr(I2), _ptr(I3), 1 if I1.dtype == torch.float64 else 0, n, h, w, _ptr(out))
    return out


def standardize_brightness(rgb, out=None, ws=None):
    """standardize_brightness per tile -> (out, p90 (N,) f64)."""
    n, h, w = _check_tiles(rgb)
    if out is None:
        out = torch.empty_like(rgb)
    p = torch.empty((n,), dtype=torch.float64, device=rgb.device)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, rgb.device)
    _call("sl_standardize_brightness", _ptr(rgb), _ptr(out), n, h, w, _ptr(p), _ptr(wsb), wsb.numel())
    return out, p


def reinhard_stats(rgb, standardize=True, ws=None):
    """(N, 8) float64 per tile: p90, mean L/a/b, std L/a/b (cv2.meanStdDev of the lab_split planes), tissue count."""
    n, h, w = _check_tiles(rgb)
    st = torch.empty((n, 8), dtype=torch.float64, device=rgb.device)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, rgb.device)
    _call("sl_reinhard_stats", _ptr(rgb), n, h, w, 1 if standardize else 0, _ptr(st), _ptr(wsb), wsb.numel())
    return st


def reinhard_transform(rgb, target_means, target_stds, mask_background=False, luminosity_threshold=0.8, out=None, ws=None):
    """Batched ReinhardStainNormalizer.transform -> (out, stats (N, 8))."""
    n, h, w = _check_tiles(rgb)
    dev = rgb.device
    tm, ts = _f64(target_means, (3,), dev), _f64(target_stds, (3,), dev)
    if out is None:
        out = torch.empty_like(rgb)
    st = torch.empty((n, 8), dtype=torch.float64, device=dev)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, dev)
    _call("sl_reinhard_transform", _ptr(rgb), _ptr(out), n, h, w, _ptr(tm), _ptr(ts), 1 if mask_background else 0,
          float(luminosity_threshold), _ptr(st), _ptr(wsb), wsb.numel())
    return out, st


def luminosity_standardize(rgb, percentile=95, out=None, ws=None):
    """Batched LuminosityStandardizer.standardize -> (out, p (N,) f64)."""
    n, h, w = _check_tiles(rgb)
    if out is None:
        out = torch.empty_like(rgb)
    p = torch.empty((n,), dtype=torch.float64, device=rgb.device)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, rgb.device)
    _call("sl_luminosity_standardize", _ptr(rgb), _ptr(out), n, h, w, float(percentile), _ptr(p), _ptr(wsb), wsb.numel())
    return out, p


# ---- the Lab family behind the view (sl_reinhard_view, sl_luminosity_view, sl_slab_view; see include/stainlib_hip.h) ------------------
def _lab_view_prepare(rgb, windows, size, d_mask, fmt, out, view=None, before_device=None, shrink=1):
    """_view_prepare for a Lab map: its checks in its order (size, windows, format, before_device(n), then _check_tiles and out;
    ValueError) -> (n, h, w, oh, ow, d_mask, windows on the device, SlTensorFormat or None, out, windows as given or drawn, shrink).
    view: a TileView (a batch method's view=) -- size, d_mask and shrink are its own (_view_call), and windows=None means view.draw(n, h, w)
    from the global numpy stream, drawn behind every check: a refused call draws nothing, and nothing goes to the device before it."""
    from .tensor_format import TensorFormat
    from .tile_view import check_size
    _lab_no_resize(view)
    if view is not None:
        size, d_mask, _, shrink = _view_call(view, windows, rgb, draw=False)
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() == 4 and rgb.shape[-1] == 3):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w = (int(v) for v in rgb.shape[:3])
    oh, ow = check_size(size, h, w, d_mask, shrink)
    win = _view_windows(windows, n, h, w, oh, ow, d_mask, shrink) if (windows is not None or view is None) else None
    if fmt is not None and not isinstance(fmt, TensorFormat):
        raise ValueError("fmt must be a stainlib_amd.TensorFormat or None (the uint8 image)")
    if before_device is not None:
        before_device(n)
    _check_tiles(rgb)
    dev = rgb.device
    if isinstance(win, torch.Tensor) and win.device != dev:
        raise ValueError(f"windows must be on {dev}")
    f, out = _image_out(out, rgb, n, oh, ow, fmt, "view")
    if win is None:
        windows = win = view.draw(n, h, w)
    if not isinstance(win, torch.Tensor):
        win = torch.from_numpy(win).to(dev)
    return n, h, w, oh, ow, int(d_mask), win, f, out, windows, int(shrink)


def _three(x, what):
    """three float64 on the host (ValueError), or the device tensor as it is"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.numel() != 3:
            raise ValueError(f"{what} must hold 3 values (L, a, b)")
        return x
    import numpy as np
    try:
        v = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what} must hold 3 values (L, a, b)") from None
    if v.shape != (3,):
        raise ValueError(f"{what} must hold 3 values (L, a, b)")
    return v


def reinhard_view(rgb, windows, size, target_means, target_stds, d_mask=7, mask_background=False, luminosity_threshold=0.8, fmt=None,
                  out=None, ws=None, view=None, shrink=1):
    """reinhard_transform with normalize_view's crop, flip and quarter turn per tile in its map sweep (sl_reinhard_view): the unchanged
    statistics of the WHOLE tiles, then ONE sweep that reads, maps and writes window pixels only -- bit for bit the view of
    reinhard_transform's image (fmt: its fmt.convert).  windows, size, d_mask, fmt, out: normalize_view's; view: a TileView in place of
    size, d_mask and shrink, whose draw gives the windows when windows is None; shrink: normalize_view's (sl_reinhard_view_shrink).
    -> (out, stats (N, 8), windows)."""
    tm_ts = []
    n, h, w, oh, ow, d_mask, win, f, out, windows, shrink = _lab_view_prepare(
        rgb, windows, size, d_mask, fmt, out, view,
        lambda n: tm_ts.extend((_three(target_means, "target_means"), _three(target_stds, "target_stds"))), shrink)
    dev = rgb.device
    tm, ts = _f64(tm_ts[0], (3,), dev), _f64(tm_ts[1], (3,), dev)
    st = torch.empty((n, 8), dtype=torch.float64, device=dev)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, dev)
    _call_view("sl_reinhard_view", shrink, (_ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask)), _ptr(tm), _ptr(ts),
               1 if mask_background else 0, float(luminosity_threshold), _ptr(st), _ptr(wsb), wsb.numel(), _byref(f))
    return out, st, windows


def luminosity_view(rgb, windows, size, percentile=95, d_mask=7, fmt=None, out=None, ws=None, view=None, shrink=1):
    """luminosity_standardize with the view in its map sweep (sl_luminosity_view; see reinhard_view) -> (out, p (N,) f64, windows)."""
    def pct_ok(n):
        try:
            float(percentile)
        except (TypeError, ValueError):
            raise ValueError("percentile must be a number") from None
    n, h, w, oh, ow, d_mask, win, f, out, windows, shrink = _lab_view_prepare(rgb, windows, size, d_mask, fmt, out, view, pct_ok, shrink)
    p = torch.empty((n,), dtype=torch.float64, device=rgb.device)
    wsb = _scratch(ws, _ffi.OP_LAB_STATS, n, h, w, rgb.device)
    _call_view("sl_luminosity_view", shrink, (_ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask)), float(percentile), _ptr(p),
               _ptr(wsb), wsb.numel(), _byref(f))
    return out, p, windows


def slab_view(rgb, windows, size, state, mode, d_mask=7, mask_background=False, luminosity_threshold=0.8, fmt=None, out=None, view=None,
              shrink=1):
    """slab_map with the view in its sweep (sl_slab_view): per tile the window of the image slab_map writes under the slide's tables (a
    non-OK status: of the tile's own bytes), as the uint8 image or the tensor.  An empty shard gives the empty output.
    -> (out, windows)."""
    def state_ok(n):
        if mode not in (0, 1):
            raise ValueError("mode must be 0 (Reinhard) or 1 (luminosity)")
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.float64 and state.numel() == _ffi.SLAB_STATE_DOUBLES
                and state.is_contiguous()):
            raise ValueError(f"state must be the ({_ffi.SLAB_STATE_DOUBLES},) float64 tensor of slab_begin / slab_finish")
    n, h, w, oh, ow, d_mask, win, f, out, windows, shrink = _lab_view_prepare(rgb, windows, size, d_mask, fmt, out, view, state_ok, shrink)
    if n:
        _call_view("sl_slab_view", shrink, (_ptr(rgb), _ptr(out), n, h, w, oh, ow, _ptr(win), int(d_mask)), _ptr(state), int(mode),
                   1 if mask_background else 0, float(luminosity_threshold), _byref(f))
    return out, windows


def _lab_no_resize(view):
    """ValueError for a resizing view (TileView(scale=)) in a Lab-family call: their fused pass has no resampling write side."""
    _no_affine(view, "the Lab-family calls (Reinhard, luminosity, pooled or per tile)",
               "take their full-tile result through TensorFormat.convert(view=), which samples bilinearly")
    if getattr(view, "resizing", False):
        raise ValueError(f"a resizing view ({view!r}) is not supported by the Lab-family calls (Reinhard, luminosity, pooled or per "
                         "tile): take their full-tile result through TensorFormat.convert(view=), which resamples")


def lab_view_check(view, windows, tiles):
    """The view= / windows= pair of a Lab batch method, checked without a device and without a draw (ValueError: windows= without
    view=, and what _view_call refuses) -> whether there is a view."""
    _lab_no_resize(view)
    if view is None and windows is None:
        return False
    _view_call(view, windows, tiles, draw=False)
    return True


# ---- pooled slide-level mode: per-process reductions (combined over ranks in stainlib_amd.distributed) -------------
def tile_moments(rgb, params=None, ws=None):
    """(n, 10) float64 per tile: tissue count, sum od[3], sum od od^T [xx, xy, xz, yy, yz, zz]  (sl_tile_moments)."""
    n, h, w = _check_tiles(rgb)
    out = torch.empty((n, 10), dtype=torch.float64, device=rgb.device)
    wsb = _scratch(ws, _ffi.OP_TILE_MOMENTS, n, h, w, rgb.device)
    _call("sl_tile_moments", _ptr(rgb), n, h, w, _params(params), _ptr(out), _ptr(wsb), wsb.numel())
    return out


def _basis6(basis):
    import numpy as np
    b = np.ascontiguousarray(np.asarray(basis, dtype=np.float64).reshape(6))
    return b, b.ctypes.data_as(C.POINTER(C.c_double))


def slide_key_histogram(rgb, keyset, basis, prefixes, prefix_bits, hist=None, params=None):
    """Accumulate into hist ((2, 256) int64, device), for both targets of the key set, the next 8 key bits of this
    process's pixels whose key starts with prefixes[t]."""
    n, h, w = _check_tiles(rgb)
    if hist is None:
        hist = torch.zeros((2, 256), dtype=torch.int64, device=rgb.device)
    keep, bp = _basis6(basis)
    pre = (C.c_uint32 * 2)(int(prefixes[0]) & 0xffffffff, int(prefixes[1]) & 0xffffffff)
    _call("sl_slide_key_histogram", _ptr(rgb), n, h, w, _params(params), int(keyset), bp, pre, int(prefix_bits), _ptr(hist))
    return hist


def slide_key_histogram16(rgb, keyset, basis, prefixes16, hist=None, params=None):
    """Accumulate into hist ((2, 65536) int64, device), for both targets, the LOW 16 key bits of this process's pixels
    whose key's top 16 bits equal prefixes16[t] (the last two radix rounds in one sweep)."""
    n, h, w = _check_tiles(rgb)
    if hist is None:
        hist = torch.zeros((2, 65536), dtype=torch.int64, device=rgb.device)
    keep, bp = _basis6(basis)
    pre = (C.c_uint32 * 2)(int(prefixes16[0]) & 0xffff, int(prefixes16[1]) & 0xffff)
    _call("sl_slide_key_histogram16", _ptr(rgb), n, h, w, _params(params), int(keyset), bp, pre, _ptr(hist))
    return hist


def slide_key_histogram_sampled(rgb, keyset, basis, prefixes, prefix_bits, sample_log2, params=None):
    """slide_key_histogram over a stratified pixel sample (one 64-chunk row in 2**sample_log2); returns a fresh (2, 256) int64."""
    n, h, w = _check_tiles(rgb)
    hist = torch.zeros((2, 256), dtype=torch.int64, device=rgb.device)
    keep, bp = _basis6(basis)
    pre = (C.c_uint32 * 2)(int(prefixes[0]) & 0xffffffff, int(prefixes[1]) & 0xffffffff)
    _call("sl_slide_key_histogram_sampled", _ptr(rgb), n, h, w, _params(params), int(keyset), bp, pre, int(prefix_bits), int(sample_log2),
          _ptr(hist))
    return hist


def slide_key_window(rgb, keyset, basis, window_lo, params=None):
    """Per target: histogram of key - window_lo[t] over this process's keys inside [window_lo[t], window_lo[t] + 65536) and the
    number of its keys below the window.  Returns one (2 * 65536 + 2,) int64 device tensor: hist[0], hist[1], below[0], below[1]."""
    n, h, w = _check_tiles(rgb)
    buf = torch.zeros((2 * 65536 + 2,), dtype=torch.int64, device=rgb.device)
    keep, bp = _basis6(basis)
    lo = (C.c_uint32 * 2)(int(window_lo[0]) & 0xffffffff, int(window_lo[1]) & 0xffffffff)
    _call("sl_slide_key_window", _ptr(rgb), n, h, w, _params(params), int(keyset), bp, lo, _ptr(buf))
    return buf


# ---- device-driven pooled statistics (sl_pool_*): every step is enqueued, nothing is read back -------------------------------
def pool_begin(moments11, state=None, params=None):
    """moments11: device float64 (11,) = the tile moments summed over all tiles and ranks + the pixel count.  Returns the state tensor."""
    if state is None:
        state = torch.empty((_ffi.POOL_STATE_DOUBLES,), dtype=torch.float64, device=moments11.device)
    _call("sl_pool_begin", _ptr(moments11), _params(params), _ptr(state))
    return state


def pool_histogram(rgb, keyset, state, rnd, sample_log2, hist, params=None):
    """This process's sampled (2, 256) histogram of radix round `rnd` under the prefixes in `state`, accumulated into hist (zeroed by the caller)."""
    n, h, w = _check_tiles(rgb)
    _call("sl_pool_histogram", _ptr(rgb), n, h, w, _params(params), int(keyset), _ptr(state), int(rnd), int(sample_log2), _ptr(hist))
    return hist


def pool_pick(state, keyset, rnd, hist_reduced):
    _call("sl_pool_pick", _ptr(state), int(keyset), int(rnd), _ptr(hist_reduced))


def pool_window(rgb, keyset, state, buf, params=None):
    """This process's window histogram + counts below ((2 * 65536 + 2,) int64, zeroed by the caller) around the windows in `state`."""
    n, h, w = _check_tiles(rgb)
    _call("sl_pool_window", _ptr(rgb), n, h, w, _params(params), int(keyset), _ptr(state), _ptr(buf))
    return buf


def pool_resolve(state, keyset, window_reduced, params=None):
    _call("sl_pool_resolve", _ptr(state), int(keyset), _ptr(window_reduced), _params(params))


# ---- the pooled statistics in ONE full sweep (sl_pool2_*): see include/stainlib_hip.h ------------------------------------------------
def pool2_workspace(n, h, w, sample_log2, device) -> torch.Tensor:
    need = int(_ffi.lib().sl_pool2_workspace_bytes(int(n), int(h), int(w), int(sample_log2)))
    if need == 0:
        raise ValueError("sl_pool2_workspace_bytes: bad arguments")
    return torch.empty(need, dtype=torch.uint8, device=device)


def pool2_sample(rgb, sample_log2, ws, params=None):
    """S1: this process's sample (packed list in ws) and its moment sums -> (16,) float64 to be all-reduced."""
    n, h, w = _check_tiles(rgb)
    out = torch.empty((16,), dtype=torch.float64, device=rgb.device)
    _call("sl_pool2_sample", _ptr(rgb), n, h, w, _params(params), int(sample_log2), _ptr(ws), ws.numel(), _ptr(out))
    return out


def pool2_begin(moments16, sample_log2, state=None, params=None):
    if state is None:
        state = torch.empty((_ffi.POOL2_STATE_DOUBLES,), dtype=torch.float64, device=moments16.device)
    _call("sl_pool2_begin", _ptr(moments16), _params(params), int(sample_log2), _ptr(state))
    return state


def pool2_hist(which, keyset, mode, shape, sample_log2, state, ws, hist, params=None):
    """A pass over the sample list (which=0, mode=0: a uniform grid) or the candidate list (which=1, mode=1: a window) of ws: the
    histogram of the key set under the constants in `state`, written into hist ((POOL2_HIST_WORDS,) int64)."""
    n, h, w = shape
    _call("sl_pool2_hist", int(which), int(keyset), int(mode), int(n), int(h), int(w), _params(params), int(sample_log2), _ptr(state),
          _ptr(ws), ws.numel(), _ptr(hist))
    return hist


def pool2_bands(state, keyset, hist_reduced):
    _call("sl_pool2_bands", _ptr(state), int(keyset), _ptr(hist_reduced))


def pool2_sweep(rgb, sample_log2, state, ws, params=None):
    """THE full sweep: exact moment sums + the raw candidates (into ws) -> (16,) float64 to be all-reduced."""
    n, h, w = _check_tiles(rgb)
    out = torch.empty((16,), dtype=torch.float64, device=rgb.device)
    _call("sl_pool2_sweep", _ptr(rgb), n, h, w, _params(params), int(sample_log2), _ptr(state), _ptr(ws), ws.numel(), _ptr(out))
    return out


def pool2_exact(totals16, state):
    _call("sl_pool2_exact", _ptr(totals16), _ptr(state))


def pool2_local(rgb, sample_log2, ws, state=None, params=None):
    """The whole one-sweep chain on ONE process, enqueued by one call (sl_pool2_local).  Returns the state tensor."""
    n, h, w = _check_tiles(rgb)
    if state is None:
        state = torch.empty((_ffi.POOL2_STATE_DOUBLES,), dtype=torch.float64, device=rgb.device)
    _call("sl_pool2_local", _ptr(rgb), n, h, w, _params(params), int(sample_log2), _ptr(ws), ws.numel(), _ptr(state))
    return state


def pool2_step(state, keyset, hist_reduced):
    """One level of the exact selection on the candidates (see sl_pool2_step)."""
    _call("sl_pool2_step", _ptr(state), int(keyset), _ptr(hist_reduced))


# ---- the pooled slide-level Vahadane dictionary (sl_sdict_*): rounds of sweep -> all-reduce -> step, nothing read back ----------------
def sdict_workspace(n, h, w, device) -> torch.Tensor:
    need = int(_ffi.lib().sl_sdict_workspace_bytes(int(n), int(h), int(w)))
    if need == 0:
        raise ValueError("sl_sdict_workspace_bytes: bad arguments")
    return torch.empty(need, dtype=torch.uint8, device=device)


def sdict_begin(sample_log2, device, state=None, params=None):
    """The dictionary iteration at the Ruifrok start.  Returns the state tensor ((SDICT_STATE_DOUBLES,) float64)."""
    if state is None:
        state = torch.empty((_ffi.SDICT_STATE_DOUBLES,), dtype=torch.float64, device=device)
    _call("sl_sdict_begin", _params(params), int(sample_log2), _ptr(state))
    return state


def sdict_sweep(rgb, sample_log2, state, ws, sums=None, params=None):
    """One round over this process's tiles (n may be 0) under the state's dictionary -> (SDICT_SUMS,) float64 to be all-reduced."""
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[-1] == 3
            and rgb.is_contiguous()):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w, _ = rgb.shape
    if sums is None:
        sums = torch.empty((_ffi.SDICT_SUMS,), dtype=torch.float64, device=rgb.device)
    _call("sl_sdict_sweep", _ptr(rgb) if n else C.c_void_p(0), n, h, w, _params(params), int(sample_log2), _ptr(state), _ptr(ws),
          ws.numel(), _ptr(sums))
    return sums


def sdict_step(state, sums_reduced, params=None):
    _call("sl_sdict_step", _ptr(state), _ptr(sums_reduced), _params(params))


# ---- the pooled slide-level Reinhard / luminosity statistics (sl_slab_*): two sums -> all-reduce -> step, then the map ----------------
def _check_shard(rgb: torch.Tensor):
    """like _check_tiles, for a shard that may hold no tile"""
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[-1] == 3
            and rgb.is_contiguous()):
        raise ValueError("expected a contiguous CUDA uint8 tensor of shape (N, H, W, 3)")
    n, h, w, _ = rgb.shape
    return n, h, w


def slab_workspace(n, h, w, device) -> torch.Tensor:
    need = int(_ffi.lib().sl_slab_workspace_bytes(int(n), int(h), int(w)))
    if need == 0:
        raise ValueError("sl_slab_workspace_bytes: bad arguments")
    return torch.empty(need, dtype=torch.uint8, device=device)


def slab_bytes(rgb, ws, sums=None):
    """The byte counts of this process's tiles (n may be 0) -> (SLAB_SUMS_A,) int64 to be all-reduced."""
    n, h, w = _check_shard(rgb)
    if sums is None:
        sums = torch.empty((_ffi.SLAB_SUMS_A,), dtype=torch.int64, device=rgb.device)
    _call("sl_slab_bytes", _ptr(rgb) if n else C.c_void_p(0), n, h, w, _ptr(ws), ws.numel(), _ptr(sums))
    return sums


def slab_begin(sums_a_reduced, standardize, device, state=None):
    """p90 and the brightness table from the all-reduced byte counts (standardize=False: identity brightness, no counts needed).
    Returns the state tensor ((SLAB_STATE_DOUBLES,) float64)."""
    if state is None:
        state = torch.empty((_ffi.SLAB_STATE_DOUBLES,), dtype=torch.float64, device=device)
    _call("sl_slab_begin", _ptr(state), _ptr(sums_a_reduced), 1 if standardize else 0)
    return state


def slab_lab(rgb, state, luminosity_threshold, ws, sums=None):
    """The Lab sums of this process's (standardised) tiles (n may be 0) -> (SLAB_SUMS_B,) int64 to be all-reduced."""
    n, h, w = _check_shard(rgb)
    if sums is None:
        sums = torch.empty((_ffi.SLAB_SUMS_B,), dtype=torch.int64, device=rgb.device)
    _call("sl_slab_lab", _ptr(rgb) if n else C.c_void_p(0), n, h, w, _ptr(state), float(luminosity_threshold), _ptr(ws), ws.numel(), _ptr(sums))
    return sums


def slab_finish(state, sums_b_reduced, mode, target_means=None, target_stds=None, percentile=95.0, mask_background=False):
    """The slide's statistics, tables and status from the all-reduced Lab sums.  mode 0: Reinhard (target_means / target_stds: 3 values
    each), mode 1: luminosity (percentile)."""
    tm = _f64(target_means, (3,), state.device) if target_means is not None else None
    ts = _f64(target_stds, (3,), state.device) if target_stds is not None else None
    _call("sl_slab_finish", _ptr(state), _ptr(sums_b_reduced), int(mode), _ptr(tm), _ptr(ts), float(percentile), 1 if mask_background else 0)


def slab_map(rgb, state, mode, mask_background=False, luminosity_threshold=0.8, out=None):
    """The map of this process's tiles under the slide's tables (a non-OK status copies them through).  An empty shard is returned as is."""
    n, h, w = _check_shard(rgb)
    if out is None:
        out = torch.empty_like(rgb)
    if n:
        _call("sl_slab_map", _ptr(rgb), _ptr(out), n, h, w, _ptr(state), int(mode), 1 if mask_background else 0, float(luminosity_threshold))
    return out


def slide_key_next_above(rgb, keyset, basis, key_ords, params=None):
    """Per target: smallest key (ordered uint32, Python ints) above key_ords[t] among this process's pixels; 0xffffffff if none."""
    n, h, w = _check_tiles(rgb)
    mn = torch.full((2,), -1, dtype=torch.int32, device=rgb.device)        # 0xffffffff
    keep, bp = _basis6(basis)
    ko = (C.c_uint32 * 2)(int(key_ords[0]) & 0xffffffff, int(key_ords[1]) & 0xffffffff)
    _call("sl_slide_key_next_above", _ptr(rgb), n, h, w, _params(params), int(keyset), bp, ko, _ptr(mn))
    v = mn.cpu().tolist()
    return [int(v[0]) & 0xffffffff, int(v[1]) & 0xffffffff]

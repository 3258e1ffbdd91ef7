"""numpy stand-ins of the sl_slab_* engine wrappers (stainlib_amd/engine.py slab_*) for the CPU tests of the pooled Reinhard / luminosity
chain.  They keep the contracts of include/stainlib_hip.h: the two sums calls return THIS rank's integer sums (int64, SLAB_SUMS_A /
SLAB_SUMS_B; zeros for an empty shard, the pixel count last), begin / finish work from the (reduced) sums they are handed and nothing
else, the state header carries the SL_SLAB_* entries, and the map copies the tiles through under a non-OK status.  The table area of the
state is private to an implementation: the stand-ins keep the few scalars there from which they rebuild their tables.

The arithmetic is restated from the reference's formulas on histograms (NOT taken from the oracle's transform, which the tests compare
against): np.percentile of the population a histogram describes, cv2.meanStdDev's sums from the L8 histogram and the four a/b sums,
normalizer.py:81-83 on the 256 possible bytes of each channel."""
import numpy as np
import torch

T_STD, T_MODE, T_MASK, T_THR, T_TM, T_TS, T_PCT = 0, 1, 2, 3, 4, 7, 10       # offsets inside the private table area


def _percentile_of_hist(hist, pct):
    pop = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(hist, dtype=np.int64))
    return float(np.percentile(pop, pct)) if pop.size else float("nan")


def _lut(state, _ffi):
    t = state[_ffi.SLAB_TABLES:].numpy()
    if not t[T_STD]:
        return np.arange(256, dtype=np.uint8)
    with np.errstate(all="ignore"):
        v = np.clip(np.arange(256) * 255.0 / float(state[_ffi.SLAB_P90]), 0, 255)          # stain_utils.py:194
    return np.where(np.isnan(v), 0, v).astype(np.uint8)


def install(calls=None):
    """Replace engine.slab_* by the stand-ins (in this process)."""
    from oracle import stain_oracle as so
    from stainlib_amd import _ffi, engine

    def note(name):
        if calls is not None:
            calls.append(name)

    def slab_workspace(n, h, w, device):
        return torch.empty(256, dtype=torch.uint8)

    def slab_bytes(rgb, ws, sums=None):
        note("bytes")
        return torch.from_numpy(np.bincount(rgb.numpy().ravel(), minlength=256).astype(np.int64))

    def slab_begin(sums_a_reduced, standardize, device, state=None):
        note("begin")
        st = torch.zeros(_ffi.SLAB_STATE_DOUBLES, dtype=torch.float64)
        st[_ffi.SLAB_MEANS:_ffi.SLAB_LPCT + 1] = float("nan")
        st[_ffi.SLAB_P90] = _percentile_of_hist(sums_a_reduced.numpy(), 90) if standardize else float("nan")
        st[_ffi.SLAB_TABLES + T_STD] = 1.0 if standardize else 0.0
        return st

    def lab_of(rgb, state):
        T = rgb.numpy()
        return so.rgb2lab_u8(_lut(state, _ffi)[T].reshape(-1, 1, 3)).reshape(-1, 3)

    def slab_lab(rgb, state, luminosity_threshold, ws, sums=None):
        note("lab")
        out = np.zeros(_ffi.SLAB_SUMS_B, dtype=np.int64)
        if rgb.shape[0]:
            lab = lab_of(rgb, state).astype(np.int64)
            out[:256] = np.bincount(lab[:, 0], minlength=256)
            out[256:260] = [lab[:, 1].sum(), (lab[:, 1] ** 2).sum(), lab[:, 2].sum(), (lab[:, 2] ** 2).sum()]
            out[260] = int((lab[:, 0] / 255.0 < luminosity_threshold).sum())
            out[261] = len(lab)
        return torch.from_numpy(out)

    def slab_finish(state, sums_b_reduced, mode, target_means=None, target_stds=None, percentile=95.0, mask_background=False):
        note("finish")
        s = sums_b_reduced.numpy().astype(np.int64)
        hist, n = s[:256].astype(np.float64), float(s[:256].sum())
        x = (np.arange(256, dtype=np.float32) / np.float32(2.55)).astype(np.float64)        # lab_split's binary32 L, promoted
        with np.errstate(all="ignore"):
            s1 = [float((hist * x).sum()), float(s[256]) - 128.0 * n, float(s[258]) - 128.0 * n]
            s2 = [float((hist * x * x).sum()), float(s[257]) - 256.0 * float(s[256]) + 16384.0 * n,
                  float(s[259]) - 256.0 * float(s[258]) + 16384.0 * n]
            for ch in range(3):
                mean = np.float64(s1[ch]) / np.float64(n)
                var = np.float64(s2[ch]) / np.float64(n) - mean * mean
                state[_ffi.SLAB_MEANS + ch] = float(mean)
                state[_ffi.SLAB_STDS + ch] = float(np.sqrt(var if var > 0 else 0.0)) if n else float("nan")
        state[_ffi.SLAB_LPCT] = _percentile_of_hist(s[:256], percentile) if mode == 1 else float("nan")
        state[_ffi.SLAB_TISSUE], state[_ffi.SLAB_NPX] = float(s[260]), float(s[261])
        empty = s[261] == 0 or (mode == 0 and mask_background and s[260] == 0)
        state[_ffi.SLAB_STATUS] = _ffi.TILE_EMPTY_MASK if empty else _ffi.TILE_OK
        t = state[_ffi.SLAB_TABLES:]
        t[T_MODE], t[T_MASK], t[T_PCT] = float(mode), float(bool(mask_background)), float(percentile)
        if mode == 0:
            t[T_TM:T_TM + 3] = torch.as_tensor(np.asarray(target_means, dtype=np.float64).reshape(3))
            t[T_TS:T_TS + 3] = torch.as_tensor(np.asarray(target_stds, dtype=np.float64).reshape(3))

    def slab_map(rgb, state, mode, mask_background=False, luminosity_threshold=0.8, out=None):
        note("map")
        if out is None:
            out = torch.empty_like(rgb)
        if rgb.shape[0] == 0:
            return out
        if int(state[_ffi.SLAB_STATUS]) != _ffi.TILE_OK:
            out.copy_(rgb)
            return out
        t = state[_ffi.SLAB_TABLES:].numpy()
        lab = lab_of(rgb, state)
        v = np.arange(256, dtype=np.float32)
        tabs = []
        with np.errstate(all="ignore"):
            if mode == 0:
                means, stds = state[_ffi.SLAB_MEANS:_ffi.SLAB_MEANS + 3].numpy(), state[_ffi.SLAB_STDS:_ffi.SLAB_STDS + 3].numpy()
                for ch in range(3):
                    x = ((v / np.float32(2.55)) if ch == 0 else (v - np.float32(128.0))).astype(np.float64)
                    nrm = ((x - means[ch]) * (t[T_TS + ch] / stds[ch])) + t[T_TM + ch]                  # normalizer.py:81-83
                    tabs.append(np.clip(nrm * 2.55 if ch == 0 else nrm + 128.0, 0, 255))                # merge_back
            else:
                tabs = [np.clip(255 * v.astype(np.float64) / float(state[_ffi.SLAB_LPCT]), 0, 255), v, v]  # stain_utils.py:65
        tabs = [np.where(np.isnan(tb), 0, tb).astype(np.uint8) for tb in tabs]
        lab2 = np.stack([tabs[ch][lab[:, ch]] for ch in range(3)], axis=-1)
        if mode == 0 and mask_background:
            bg = ~(lab[:, 0] / 255.0 < luminosity_threshold)
            lab2[bg] = (255, 128, 128)                                   # L 254 on the L/2.55 scale clips to 255; a = b = 0 + 128
        out.copy_(torch.from_numpy(so.lab2rgb_u8(lab2.reshape(-1, 1, 3)).reshape(tuple(rgb.shape))))
        return out

    engine.slab_workspace, engine.slab_bytes, engine.slab_begin = slab_workspace, slab_bytes, slab_begin
    engine.slab_lab, engine.slab_finish, engine.slab_map = slab_lab, slab_finish, slab_map

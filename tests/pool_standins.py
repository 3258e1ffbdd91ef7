"""numpy stand-ins for the device steps of the THREE-SWEEP pooled chain (sl_tile_moments, sl_slide_key_*, sl_pool_*,
sl_normalize_apply), for the world-size-2 gloo tests on the CPU.

The engine's device sweeps are replaced by numpy stand-ins built on the oracle, with the same contracts as
include/stainlib_hip.h; everything else -- the moment / pixel-count all-reduces, the sampled estimate, the window all-reduce,
the radix fallback, the broadcast-free agreement of the ranks, the apply pass with the slide statistics -- is the product code
of stainlib_amd/distributed.py executing."""
import numpy as np
import torch

from stainlib_amd import distributed as sd
from tests.standin_math import angle_keys, conc_keys, eig2, f2ord, matrix_from, moments, od_of, ord2f, tissue


def install(force_radix=False):
    """Replace the engine's three-sweep steps by the stand-ins (in this process)."""
    from oracle import stain_oracle as so
    from stainlib_amd import _ffi, engine

    def keys(tiles, keyset, basis):
        """ordered-uint32 keys of this rank's pixels, per target: [k0, k1] (angle: tissue pixels only, one key set twice)"""
        px = tiles.numpy().reshape(-1, 3)
        od = od_of(px).astype(np.float32)
        if keyset == _ffi.KEYSET_ANGLE:
            k = f2ord(angle_keys(od[tissue(px)], basis))
            return [k, k]
        C = conc_keys(od, basis)
        return [f2ord(C[:, 0]), f2ord(C[:, 1])]

    def tile_moments(tiles, params=None, ws=None):
        return torch.tensor([moments(od_of(t)[tissue(t)]) for t in tiles.numpy()], dtype=torch.float64)

    def hist(tiles, keyset, basis, prefixes, bits, hist=None, params=None, every=1):
        ks = keys(tiles, keyset, basis)
        rows = []
        for t in range(2):
            o = ks[t][::every]
            sel = o if bits == 0 else o[(o >> np.uint64(32 - bits)) == np.uint64(prefixes[t])]
            rows.append(np.bincount(((sel >> np.uint64(24 - bits)) & np.uint64(255)).astype(np.int64), minlength=256))
        return torch.from_numpy(np.stack(rows).astype(np.int64))

    def hist16(tiles, keyset, basis, prefixes16, hist=None, params=None):
        ks = keys(tiles, keyset, basis)
        rows = [np.bincount((ks[t][(ks[t] >> np.uint64(16)) == np.uint64(prefixes16[t])] & np.uint64(0xffff)).astype(np.int64), minlength=65536)
                for t in range(2)]
        return torch.from_numpy(np.stack(rows).astype(np.int64))

    def window(tiles, keyset, basis, lo, params=None):
        if force_radix:                       # a window that sees nothing: the caller must fall back to the radix rounds
            return torch.zeros((2 * 65536 + 2,), dtype=torch.int64)
        ks = keys(tiles, keyset, basis)
        out = np.zeros(2 * 65536 + 2, np.int64)
        for t in range(2):
            d = ks[t].astype(np.int64) - int(lo[t])
            out[t * 65536:(t + 1) * 65536] = np.bincount(d[(d >= 0) & (d < 65536)], minlength=65536)
            out[2 * 65536 + t] = int((d < 0).sum())
        return torch.from_numpy(out)

    def next_above(tiles, keyset, basis, key_ords, params=None):
        ks = keys(tiles, keyset, basis)
        out = []
        for t in range(2):
            g = ks[t][ks[t] > np.uint64(key_ords[t])]
            out.append(int(g.min()) if len(g) else 0xffffffff)
        return out

    def normalize_apply(rgb, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda=0.01, out=None, want_prequant=False):
        res = []
        for i, t in enumerate(rgb.numpy()):
            C = so.get_concentrations(t, np.asarray(M_src[i])) * (np.asarray(maxC_tgt).reshape(2) / np.asarray(maxC_src[i]))
            res.append(so.truncate_u8(255 * np.exp(-C @ np.asarray(M_tgt))).reshape(t.shape))
        return torch.from_numpy(np.stack(res))

    # ---- the device-driven steps (sl_pool_*): numpy restatements of the single-workgroup decision kernels of csrc/slide.hip on a
    # CPU float64 "state" tensor with the layout of include/stainlib_hip.h (SL_POOL_*) -- the orchestration in
    # PooledSlideStatistics.enqueue / finish is the product code
    K_T, K_NPX, K_VD, K_VF, K_K, K_G, K_TOT, K_KS, K_BELOW, K_PREFIX, K_WLO, K_RES = 10, 11, 12, 18, 24, 26, 28, 30, 32, 34, 36, 43

    def pool_begin(mom11, state=None, params=None):
        m = mom11.numpy()
        st = torch.zeros((_ffi.POOL_STATE_DOUBLES,), dtype=torch.float64)
        T = m[0]
        st[K_T], st[K_NPX] = T, m[10]
        if T < 1:
            st[_ffi.POOL_STATUS] = _ffi.TILE_EMPTY_MASK
            return st
        V = eig2(m)
        st[K_VD:K_VD + 6] = torch.from_numpy(V.reshape(6))
        st[K_VF:K_VF + 6] = torch.from_numpy(V.astype(np.float32).astype(np.float64).reshape(6))
        for t, pct in enumerate((1.0, 99.0)):
            k, g = sd.percentile_position(int(T), pct)
            st[K_K + t], st[K_G + t] = k, g
        return st

    def basis_of(state, keyset):
        return state[K_VF:K_VF + 6].numpy() if keyset == _ffi.KEYSET_ANGLE else state[_ffi.POOL_M:_ffi.POOL_M + 6].numpy()

    def pool_histogram(tiles, keyset, state, rnd, slog, hist_out, params=None):
        pre = [int(state[K_PREFIX + t]) for t in range(2)]
        hist_out += hist(tiles, keyset, basis_of(state, keyset), pre, 8 * rnd, every=1 << slog)
        return hist_out

    def pool_pick(state, keyset, rnd, h):
        N = float(state[K_T] if keyset == _ffi.KEYSET_ANGLE else state[K_NPX])
        hc = h.numpy()
        for t in range(2):
            if rnd == 0:
                tot = int(hc[t].sum())
                f = min(max(float(state[K_K + t]) / (N - 1.0) if N > 1 else 0.0, 0.0), 1.0)
                state[K_TOT + t], state[K_KS + t], state[K_BELOW + t], state[K_PREFIX + t] = tot, (np.floor(f * (tot - 1.0)) if tot else 0.0), 0.0, 0.0
                if tot == 0:
                    state[_ffi.POOL_MISS] = float(int(state[_ffi.POOL_MISS]) | (1 if keyset == _ffi.KEYSET_ANGLE else 2))
            want = int(state[K_KS + t] - state[K_BELOW + t])
            cum, b = 0, 0
            while b < 255 and not (cum + int(hc[t][b]) > want):
                cum += int(hc[t][b]); b += 1
            state[K_BELOW + t] += cum
            state[K_PREFIX + t] = float((int(state[K_PREFIX + t]) << 8) | b)
        if rnd == 2:
            for t in range(2):
                est = (int(state[K_PREFIX + t]) << 8) | 0x80
                state[K_WLO + t] = float(min(max(est - 32768, 0), 0xffffffff - 65535))
                state[K_PREFIX + t] = 0.0

    def pool_window(tiles, keyset, state, buf, params=None):
        buf += window(tiles, keyset, basis_of(state, keyset), [int(state[K_WLO]), int(state[K_WLO + 1])])
        return buf

    def pool_resolve(state, keyset, win, params=None):
        N = int(state[K_T] if keyset == _ffi.KEYSET_ANGLE else state[K_NPX])
        b = win.numpy()
        res = []
        for t in range(2):
            histo, below = b[t * 65536:(t + 1) * 65536], int(b[2 * 65536 + t])
            k = min(max(int(state[K_K + t]), 0), N - 1)
            k1 = min(k + 1, N - 1)
            if not (N >= 1 and below <= k and k1 < below + int(histo.sum())):
                state[_ffi.POOL_MISS] = float(int(state[_ffi.POOL_MISS]) | (1 if keyset == _ffi.KEYSET_ANGLE else 2))
                if keyset != _ffi.KEYSET_ANGLE:                  # like k_pool_resolve: an unusable state ends with NaN in (M, maxC)
                    state[_ffi.POOL_M:_ffi.POOL_M + 6] = float("nan")
                    state[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2] = float("nan")
                return
            cum = np.cumsum(histo)
            lo = int(state[K_WLO + t])
            res += [ord2f(lo + int(np.searchsorted(cum, k - below, side="right"))), ord2f(lo + int(np.searchsorted(cum, k1 - below, side="right")))]
        state[K_RES:K_RES + 4] = torch.tensor(res, dtype=torch.float64)
        if keyset == _ffi.KEYSET_ANGLE:
            V = state[K_VD:K_VD + 6].numpy().reshape(3, 2)
            M = matrix_from(V, res[0], res[1], float(state[K_G]), res[2], res[3], float(state[K_G + 1]))
            state[_ffi.POOL_M:_ffi.POOL_M + 6] = torch.from_numpy(M.reshape(6))
            k, g = sd.percentile_position(int(state[K_NPX]), 99.0)
            state[K_K], state[K_K + 1], state[K_G], state[K_G + 1] = k, k, g, g
        else:
            for t in range(2):
                state[_ffi.POOL_MAXC + t] = sd.np_lerp(res[2 * t], res[2 * t + 1], float(state[K_G + t]))
            if int(state[_ffi.POOL_MISS]) != 0 or int(state[_ffi.POOL_STATUS]) != 0:
                state[_ffi.POOL_M:_ffi.POOL_M + 6] = float("nan")
                state[_ffi.POOL_MAXC:_ffi.POOL_MAXC + 2] = float("nan")

    engine.pool_begin, engine.pool_histogram, engine.pool_pick = pool_begin, pool_histogram, pool_pick
    engine.pool_window, engine.pool_resolve = pool_window, pool_resolve
    engine.make_params = lambda **kw: None
    engine.tile_moments = tile_moments
    engine.slide_key_histogram = hist
    engine.slide_key_histogram_sampled = lambda tiles, keyset, basis, pre, bits, slog, params=None: hist(tiles, keyset, basis, pre, bits, every=1 << slog)
    engine.slide_key_histogram16 = hist16
    engine.slide_key_window = window
    engine.slide_key_next_above = next_above
    engine.normalize_apply = normalize_apply

"""numpy stand-ins of the sl_sdict_* engine wrappers (state layout of include/stainlib_hip.h SL_SDICT_*) for the CPU tests of the
pooled Vahadane chain, and the three pieces of arithmetic they rest on.  A sweep returns THIS rank's 31 class-moment sums and its
pixel count, a step updates the dictionary from the ALL-REDUCED sums alone; the stand-in step is one plain block-coordinate pass
per round, so the fixed point is the oracle's."""
import types

import numpy as np
import torch

from tests.standin_math import moments, od_of, tissue

LAM = 0.1


def class_moments(od, D, lam=LAM):
    """the 31 sums a sweep under D returns: per class (both stains, stain 1 only, stain 2 only) {n, sum x (3), sum x x^T (6)}, tissue count"""
    from oracle import stain_oracle as so
    C = so.lasso2_nonneg(od, D, lam)
    a, b = C[:, 0] > 0, C[:, 1] > 0
    out = np.zeros(31)
    for c, m in enumerate((a & b, a & ~b, ~a & b)):
        out[10 * c:10 * c + 10] = moments(od[m])
    out[30] = len(od)
    return out


def ab_from_moments(mom, D, lam=LAM):
    """A = sum alpha alpha^T, B = sum x alpha^T from the class moments (the codes of a class are affine in x: alpha = W x - w)"""
    G = D @ D.T
    A, B = np.zeros((2, 2)), np.zeros((3, 2))
    for c in range(3):
        m = mom[10 * c:10 * c + 10]
        n, s = m[0], m[1:4]
        S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
        if n <= 0:
            continue
        act = [0, 1] if c == 0 else [c - 1]
        P = np.zeros((2, 2))
        P[np.ix_(act, act)] = np.linalg.inv(G[np.ix_(act, act)])
        W, w = P @ D, lam * P @ np.ones(2)
        Ws = W @ s
        A += W @ S @ W.T - np.outer(Ws, w) - np.outer(w, Ws) + n * np.outer(w, w)
        B += S @ W.T - np.outer(s, w)
    return A, B


def bcd_pass(A, B, D):
    Dn = D.copy()
    for j in range(2):
        if A[j, j] > 1e-300:
            u = np.maximum((B[:, j] - Dn.T @ A[:, j]) / A[j, j] + Dn[j], 0.0)
            Dn[j] = u / max(np.linalg.norm(u), 1.0)
    return Dn


def install(calls):
    """Replace engine.sdict_* by the stand-ins (in this process); `calls` collects "sweep" / "step" in the order they ran."""
    from oracle import stain_oracle as so
    from stainlib_amd import _ffi, engine
    engine.make_params = lambda **kw: types.SimpleNamespace(**kw)

    def sampled_od(tiles, slog):
        T = tiles.numpy()
        if len(T) == 0:
            return np.zeros((0, 3)), 0
        return np.concatenate([od_of(t)[tissue(t)][:: 1 << slog] for t in T]), T.shape[0] * T.shape[1] * T.shape[2]

    def sdict_workspace(n, h, w, device):
        return torch.empty(256, dtype=torch.uint8)

    def sdict_begin(slog, device, state=None, params=None):
        st = torch.zeros(_ffi.SDICT_STATE_DOUBLES, dtype=torch.float64)
        st[_ffi.SDICT_D:_ffi.SDICT_D + 6] = torch.from_numpy(so.normalize_rows(np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])).reshape(6))
        st[_ffi.SDICT_M:_ffi.SDICT_M + 6] = float("nan")
        st[_ffi.SDICT_MODE] = 1
        return st

    def sdict_sweep(tiles, slog, state, ws, sums=None, params=None):
        calls.append("sweep")
        out = np.zeros(_ffi.SDICT_SUMS)
        mode = int(state[_ffi.SDICT_MODE])
        od, npx = sampled_od(tiles, slog if mode == 1 else 0)
        if mode:
            out[:31] = class_moments(od, state[_ffi.SDICT_D:_ffi.SDICT_D + 6].numpy().reshape(2, 3), params.dl_lambda)
        out[31] = npx
        return torch.from_numpy(out)

    def sdict_step(state, sums, params=None):
        calls.append("step")
        s = sums.numpy()
        mode = int(state[_ffi.SDICT_MODE])
        if mode == 0:
            return
        if int(state[_ffi.SDICT_ROUNDS]) == 0:
            state[_ffi.SDICT_NPX] = float(s[31])
        state[_ffi.SDICT_ROUNDS] += 1
        D = state[_ffi.SDICT_D:_ffi.SDICT_D + 6].numpy().reshape(2, 3).copy()
        settled = False
        if s[30] < 1:
            delta = 0.0
            if mode == 2:
                state[_ffi.SDICT_STATUS] = _ffi.TILE_EMPTY_MASK
                settled = True
        else:
            Dn = bcd_pass(*ab_from_moments(s[:31], D, params.dl_lambda), D)
            delta = np.abs(Dn - D).max()
            D = Dn
            state[_ffi.SDICT_D:_ffi.SDICT_D + 6] = torch.from_numpy(D.reshape(6))
        if mode == 1:
            if delta < 1e-4:
                state[_ffi.SDICT_MODE] = 2
        else:
            state[_ffi.SDICT_SWEEPS] += 1
            settled = settled or delta < params.dl_tol or int(state[_ffi.SDICT_SWEEPS]) >= params.dl_max_sweeps
        if settled:
            if int(state[_ffi.SDICT_STATUS]) == 0:
                M = D[[1, 0]] if D[0, 0] < D[1, 0] else D
                state[_ffi.SDICT_M:_ffi.SDICT_M + 6] = torch.from_numpy(so.normalize_rows(M).reshape(6))
            state[_ffi.SDICT_MODE] = 0

    engine.sdict_workspace, engine.sdict_begin, engine.sdict_sweep, engine.sdict_step = sdict_workspace, sdict_begin, sdict_sweep, sdict_step

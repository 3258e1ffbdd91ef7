"""The arithmetic the numpy stand-ins of the pooled slide chains share (tests/pool_standins.py, pool2_standins.py,
pool_vahadane_standins.py), once each: the ordered-uint32 key map, tissue mask / OD / moment row of a run of pixels, the
eigenvector plane from ten moments, the angle and concentration keys, and the stain matrix from four resolved angle keys.
Keys are binary32 as on the device; ordered keys are returned as uint64 so that shifts and differences cannot wrap."""
import math

import numpy as np

from oracle import stain_oracle as so
from stainlib_amd import distributed as sd


def _lerp(a, b, t):
    """numpy's _lerp (lib/function_base.py), restated here: the reference of the stand-ins takes nothing from the library under test"""
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def _replicated_position(count, R, q):
    """numpy.percentile's (method='linear') position among count * R values: (k, g) with the result lerp(v[k], v[k + 1], g)"""
    n = float(count) * float(R)
    qq = q / 100.0
    vi = min(max(n * qq + (1.0 + qq * (1.0 - 1.0 - 1.0)) - 1.0, 0.0), n - 1.0)          # numpy's _compute_virtual_index, alpha = beta = 1
    k = int(math.floor(vi))
    return k, vi - k


def replicated_percentile(x, R, q):
    """np.percentile(np.repeat(x, R), q) without the repeat: a population in which every element of x occurs R times.  Position
    pos = (R m - 1) q / 100 of the sorted population is element floor(pos) // R of sorted x; interpolate to its successor."""
    xs = np.sort(np.asarray(x, dtype=np.float64).ravel())
    k, g = _replicated_position(len(xs), R, q)
    lo, hi = xs[k // R], xs[min(k + 1, len(xs) * R - 1) // R]
    return float(_lerp(lo, hi, g))


def replicated_percentile_hist(hist, R, q):
    """replicated_percentile for a byte population given by its 256 counts (np.bincount(x, minlength=256))"""
    cum = np.cumsum(np.asarray(hist, dtype=np.int64)) * int(R)
    k, g = _replicated_position(int(cum[-1]) // int(R), R, q)
    lo, hi = (int(np.searchsorted(cum, p, side="right")) for p in (k, min(k + 1, int(cum[-1]) - 1)))
    return float(_lerp(float(lo), float(hi), g))


def replicated_macenko(block_tiles, R, luminosity_threshold=0.8, angular_percentile=99, details=None):
    """The oracle's Macenko recipe (so.macenko_stain_matrix, then the 99th percentile of so.get_concentrations) for a slide of R
    repeats of the tiles in block_tiles -> (M (2, 3), maxC (2,)), from the block alone: mean and covariance of the population are the
    block's (np.cov's divisor changes the scale only, which the eigenvectors do not see), the percentile calls become
    replicated_percentile."""
    px = np.concatenate([np.asarray(t).reshape(-1, 3) for t in block_tiles]).reshape(1, -1, 3)
    mask = so.tissue_mask(px, luminosity_threshold).reshape(-1)
    OD = so.rgb_to_od(px).reshape(-1, 3)[mask]
    _, V = np.linalg.eigh(np.cov(OD, rowvar=False))
    V = V[:, [2, 1]]
    for i in range(2):
        if V[0, i] < 0:
            V[:, i] *= -1
    That = OD @ V
    phi = np.arctan2(That[:, 1], That[:, 0])
    lo, hi = replicated_percentile(phi, R, 100 - angular_percentile), replicated_percentile(phi, R, angular_percentile)
    v1, v2 = V @ np.array([np.cos(lo), np.sin(lo)]), V @ np.array([np.cos(hi), np.sin(hi)])
    M = so.normalize_rows(np.array([v1, v2]) if v1[0] > v2[0] else np.array([v2, v1]))
    C = so.get_concentrations(px, M)
    maxC = np.array([replicated_percentile(C[:, j], R, 99) for j in range(2)])
    if details is not None:
        details.update(n_tissue=int(mask.sum()) * R, n_pixels=px.shape[1] * R)
    return M, maxC


def f2ord(a):
    """binary32 -> the unsigned integer with the same order (in uint64)"""
    u = np.asarray(a, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)


def ord2f(o):
    o = int(o)
    bits = (o & 0x7fffffff) if (o & 0x80000000) else (~o & 0xffffffff)
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def tissue(px):
    """the tissue mask (L8 / 255 < 0.8) of the pixels of a tile or of an (n, 3) run, flat"""
    return (so.lab_l8(px.reshape(1, -1, 3)) / 255.0 < 0.8).ravel()


def od_of(px):
    return so.rgb_to_od(px.reshape(1, -1, 3)).reshape(-1, 3)


def moments(od):
    """{n, sum x (3), upper triangle of sum x x^T (6)}"""
    S = od.T @ od
    return [float(len(od)), *od.sum(0), S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]


def eig2(m):
    """the two leading eigenvectors (columns, first component non-negative) of the covariance the ten moments describe"""
    T = m[0]
    mean = m[1:4] / T
    S2 = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    _, V = np.linalg.eigh((S2 - T * np.outer(mean, mean)) / (T - 1.0))
    V = V[:, [2, 1]].copy()
    for i in range(2):
        if V[0, i] < 0:
            V[:, i] *= -1.0
    return V


def angle_keys(od32, V):
    """the pseudo-angle in [-2, 2] of the binary32 OD projected on the plane V (six numbers, 3 x 2)"""
    th = od32 @ np.asarray(V, np.float64).reshape(3, 2).astype(np.float32)
    x, y = th[:, 0], th[:, 1]
    d = np.abs(x) + np.abs(y)
    p = np.where(d > 0, y / np.where(d > 0, d, 1), 0).astype(np.float32)
    return np.where(x < 0, np.where(y >= 0, 2.0, -2.0).astype(np.float32) - p, p).astype(np.float32)


def conc_keys(od32, M):
    return so.lasso2_nonneg(od32.astype(np.float64), np.asarray(M, np.float64).reshape(2, 3), 0.01).astype(np.float32)


def angle_of(p):
    """pseudo-angle -> angle"""
    if abs(p) <= 1.0:
        return math.atan2(p, 1.0 - abs(p))
    pp = 2.0 - p if p > 0 else -2.0 - p
    return math.atan2(pp, -(1.0 - abs(pp)))


def matrix_from(V, pa0, pb0, g0, pa1, pb1, g1):
    """the stain matrix from the keys at ranks k, k + 1 of the two angular percentiles and their interpolation weights"""
    phis = [sd.np_lerp(angle_of(pa0), angle_of(pb0), g0), sd.np_lerp(angle_of(pa1), angle_of(pb1), g1)]
    v1, v2 = V @ np.array([math.cos(phis[0]), math.sin(phis[0])]), V @ np.array([math.cos(phis[1]), math.sin(phis[1])])
    M = np.array([v1, v2]) if v1[0] > v2[0] else np.array([v2, v1])
    return M / np.linalg.norm(M, axis=1, keepdims=True)

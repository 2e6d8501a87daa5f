"""Tap tables of the device Gaussian blur (include/vsd.h THE BLUR CONTRACT; csrc/blur.hip), in one place: how a sigma becomes a table,
and the host-side check of a table.  The contract is about what taps DO; this file is the only place that says how they are made."""
import math

import numpy as np

MAX_RADIUS = 32   # include/vsd.h VSD_BLUR_MAX_RADIUS
ONE = 16384       # include/vsd.h VSD_BLUR_ONE: w_0 + 2 * (w_1 + ... + w_R)
TAPS = 34         # int32 {R, w_0 .. w_32}
MAX_SIGMA = 10.0  # R = ceil(3 * sigma) <= 30
TILE_W, TILE_H = 32, 64  # csrc/blur_core.h BLUR_TILE_W (BYTE columns of a row of C*w bytes), BLUR_TILE_H: the kernel's tile, for the tests' shapes


def identity_taps() -> np.ndarray:
    """the table that returns its source byte for byte"""
    t = np.zeros(TAPS, dtype=np.int32)
    t[0], t[1] = 1, ONE
    return t


def gauss_taps(sigma) -> np.ndarray:
    """sigma -> int32 [34] = {R, w_0 .. w_32}.  0: the identity table.  Else 0 < sigma <= 10: R = max(1, ceil(3 sigma)),
    g_i = exp(-i^2 / (2 sigma^2)) in float64, G = g_0 + 2 sum g_i, w_i = floor(16384 g_i / G + 0.5) for i >= 1 and w_0 takes the rest,
    so the sum is 16384 exactly (w_0 may then lie 1-2 below w_1 at a large sigma: the contract does not ask for monotone taps)."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"a blur sigma must be a number in [0, {MAX_SIGMA:g}] (0: no blur), not {sigma!r}") from None
    if isinstance(sigma, bool) or not 0.0 <= s <= MAX_SIGMA:  # (NaN fails both comparisons)
        raise ValueError(f"a blur sigma must be a number in [0, {MAX_SIGMA:g}] (0: no blur), not {sigma!r}")
    if s == 0.0:
        return identity_taps()
    R = max(1, math.ceil(3.0 * s))
    g = [math.exp(-(i * i) / (2.0 * s * s)) for i in range(R + 1)]
    G = g[0] + 2.0 * sum(g[1:])
    t = np.zeros(TAPS, dtype=np.int32)
    t[0] = R
    for i in range(1, R + 1):
        t[1 + i] = math.floor(ONE * g[i] / G + 0.5)
    t[1] = ONE - 2 * int(t[2:].sum())
    return check_taps(t)


def check_taps(table) -> np.ndarray:
    """the validity rules of THE BLUR CONTRACT, as `vsd_gauss_blur_host` applies them -> the table as a fresh contiguous int32 [34]"""
    t = np.asarray(table)
    if t.shape != (TAPS,) or t.dtype.kind not in "iu":
        raise ValueError(f"a tap table must be {TAPS} integers {{R, w_0 .. w_{MAX_RADIUS}}}, not {getattr(t, 'dtype', None)} of shape {getattr(t, 'shape', None)}")
    v = [int(x) for x in t]
    R = v[0]
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"a tap table's radius must be 1..{MAX_RADIUS}, not {R}")
    negative = [i for i, w in enumerate(v[1:]) if w < 0]
    if negative:
        raise ValueError(f"a tap table's weights must not be negative: w_{negative[0]} = {v[1 + negative[0]]}")
    beyond = [i for i in range(R + 1, MAX_RADIUS + 1) if v[1 + i] != 0]
    if beyond:
        raise ValueError(f"a tap table's weights beyond its radius {R} must be 0: w_{beyond[0]} = {v[1 + beyond[0]]}")
    total = v[1] + 2 * sum(v[2:])
    if total != ONE:
        raise ValueError(f"a tap table's weights must sum to {ONE} exactly (w_0 + 2 * (w_1 + ... + w_R)), not {total}")
    return np.array(v, dtype=np.int32)

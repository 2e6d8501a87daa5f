"""THE EDGE CONTRACT of include/vsd.h restated in numpy (nothing of the library in it), and the frames the Canny tests share.

`canny_numpy` is what vsd_canny_host, the kernels of csrc/canny.hip and the engine are held to, byte for byte.  Components are labelled
with a plain breadth-first search.  The generators are deterministic; `reference(kind, h, w, low, high)` computes a case once per
process and hands out read-only arrays, and `assert_exercises` states -- on the reference -- what a case must exercise, so that a weak
input fails loudly instead of passing vacuously."""
import functools
from collections import deque

import numpy as np

MAX_MAG = 2040
THRESHOLDS = ((100, 200), (50, 150))
NOISE_SIZES = ((72, 120), (64, 64), (37, 301), (128, 128))
SERPENTINE_SIZES = ((72, 120), (40, 520), (136, 264))
SERPENTINE_CANDIDATES = {(72, 120): 1837, (40, 520): 4117, (136, 264): 8285}  # with the seed; one fewer without it
SMALL_SIZES = ((1, 1), (1, 7), (7, 1), (3, 3), (2, 2))


def gray_L(rgb):
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.int64)


def classify(gray, low, high):
    """-> (candidates, strong candidates, magnitudes) of a gray image"""
    p = np.pad(gray, 1, mode="edge")  # border replicated
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    mag = np.abs(dx) + np.abs(dy)
    m = np.pad(mag, 1)  # 0 outside the image
    c = m[1:-1, 1:-1]
    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horiz = y < t22
    vert = ~horiz & (y > t67)
    diag = ~(horiz | vert)
    left, right, up, down = m[1:-1, :-2], m[1:-1, 2:], m[:-2, 1:-1], m[2:, 1:-1]
    ul, ur, dl, dr = m[:-2, :-2], m[:-2, 2:], m[2:, :-2], m[2:, 2:]
    neg = (dx ^ dy) < 0  # s = -1: (row - 1, col + 1) and (row + 1, col - 1)
    ok = (horiz & (c > left) & (c >= right)) | (vert & (c > up) & (c >= down)) | (diag & neg & (c > ur) & (c > dl)) | (diag & ~neg & (c > ul) & (c > dr))
    cand = ok & (c > low)
    return cand, cand & (c > high), mag


def label(cand):
    """8-connected components of a boolean image by breadth-first search -> (labels 1..n, 0 elsewhere; n)"""
    h, w = cand.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(cand)):
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        todo = deque([(int(y0), int(x0))])
        while todo:
            y, x = todo.popleft()
            for yy in range(max(y - 1, 0), min(y + 2, h)):
                for xx in range(max(x - 1, 0), min(x + 2, w)):
                    if cand[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = n
                        todo.append((yy, xx))
    return lab, n


def canny_parts(rgb, low, high):
    """-> dict(edge u8 [h][w] 255 / 0, cand, strong, labels, n)"""
    low, high = int(low), int(high)
    assert 0 <= low <= high <= MAX_MAG
    cand, strong, _mag = classify(gray_L(np.asarray(rgb)), low, high)
    lab, n = label(cand)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[strong])] = True
    keep[0] = False
    return dict(edge=(keep[lab] * 255).astype(np.uint8), cand=cand, strong=strong, labels=lab, n=n)


def canny_numpy(rgb, low, high):
    return canny_parts(rgb, low, high)["edge"]


def noise_frame(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
    return np.clip(base[..., None] + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def serpentine_frame(h, w, seed_at=True, pitch=8, width=3, bg=100, fg=130, seedv=190):
    """background `bg`; a `width`-pixel band of `fg` snakes across rows 4, 4 + pitch, ... inside a 4-pixel margin, connectors alternating
    right and left; optionally 6 pixels of `seedv` at the start of the first row (the only strong edges of the frame)"""
    g = np.full((h, w), bg, np.uint8)
    rows = list(range(4, h - 4 - width, pitch))
    for i, y in enumerate(rows):
        g[y:y + width, 4:w - 4] = fg
        if i + 1 < len(rows):
            x = w - 4 - width if i % 2 == 0 else 4
            g[y:rows[i + 1] + width, x:x + width] = fg
    if seed_at:
        g[rows[0]:rows[0] + width, 4:10] = seedv
    return np.repeat(g[..., None], 3, axis=2)


def constant_frame(h, w, value=93):
    return np.full((h, w, 3), value, np.uint8)


def frame(kind, h, w):
    if kind == "noise":
        return noise_frame(h, w)
    if kind in ("serpentine", "serpentine_noseed"):
        return serpentine_frame(h, w, seed_at=kind == "serpentine")
    if kind == "constant":
        return constant_frame(h, w)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, h, w, low=100, high=200):
    """-> (frame, parts of canny_parts), computed once per process; the arrays are read-only"""
    f = frame(kind, h, w)
    parts = canny_parts(f, low, high)
    for a in [f] + [v for v in parts.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return f, parts


def hysteresis_counts(parts):
    weak = parts["cand"] & ~parts["strong"]
    return int((weak & (parts["edge"] > 0)).sum()), int((weak & (parts["edge"] == 0)).sum())  # promoted, dropped


def assert_exercises(kind, h, w, parts):
    """what a generated case has to exercise, asserted on the reference"""
    if kind == "noise":
        promoted, dropped = hysteresis_counts(parts)
        assert promoted >= 100 and dropped >= 100, (kind, h, w, promoted, dropped)  # both outcomes of hysteresis
        assert 0.2 < parts["cand"].mean() < 0.45 and parts["strong"].sum() >= 50
    elif kind in ("serpentine", "serpentine_noseed"):
        seeded = kind == "serpentine"
        assert parts["n"] == 1, parts["n"]  # ONE component that crosses the whole frame
        assert int(parts["cand"].sum()) == SERPENTINE_CANDIDATES[(h, w)] - (0 if seeded else 1)
        assert int(parts["strong"].sum()) == (16 if seeded else 0)
        assert int((parts["edge"] > 0).sum()) == (int(parts["cand"].sum()) if seeded else 0)
    elif kind == "constant":
        assert not parts["cand"].any()

"""The colour contract of the I420 path (include/vsd.h) in a few lines of numpy -- written from the formulas, not by calling the library --
and the frames and sizes tests/test_i420_host.py and tests/test_i420_gpu.py hold the host loops and the kernels to, byte for byte."""
import numpy as np

# (h, w) of the I420 input; odd sizes are legal on input
SIZES = [(720, 1280), (1080, 1920), (480, 640), (97, 131), (99, 100), (1, 1), (2, 3), (721, 1283)]
KINDS = ["noise", "corners", "outside", "gradient"]
# RGB -> I420 needs even sides: the sizes above rounded up to even
EVEN_SIZES = sorted({(h + (h & 1), w + (w & 1)) for h, w in SIZES})


def chroma_hw(h, w):
    return (h + 1) // 2, (w + 1) // 2


def contract_i420_to_rgb(y, u, v, ox=0, oy=0):
    """y: uint8 [h][w]; u, v: uint8 planes whose sample [0][0] is chroma sample (ox >> 1, oy >> 1) of the frame -> uint8 [h][w][3]"""
    h, w = y.shape
    ci = ((oy & 1) + np.arange(h)) >> 1
    cj = ((ox & 1) + np.arange(w)) >> 1
    c = y.astype(np.int64) - 16
    d = u.astype(np.int64)[np.ix_(ci, cj)] - 128
    e = v.astype(np.int64)[np.ix_(ci, cj)] - 128
    r = (298 * c + 409 * e + 128) >> 8
    g = (298 * c - 100 * d - 208 * e + 128) >> 8
    b = (298 * c + 516 * d + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def contract_rgb_to_i420(rgb):
    """uint8 [h][w][3], h and w even -> (y [h][w], u [h/2][w/2], v [h/2][w/2]); the range is asserted, not clamped"""
    h, w = rgb.shape[:2]
    assert h % 2 == 0 and w % 2 == 0
    p = rgb.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    m = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    mr, mg, mb = m[..., 0], m[..., 1], m[..., 2]
    u = ((-38 * mr - 74 * mg + 112 * mb + 128) >> 8) + 128
    v = ((112 * mr - 94 * mg - 18 * mb + 128) >> 8) + 128
    assert 16 <= y.min() and y.max() <= 235 and 16 <= min(u.min(), v.min()) and max(u.max(), v.max()) <= 240
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def contract_packed(rgb):
    """contract_rgb_to_i420 as the packed buffer of an I420Frame: Y, then U, then V"""
    return np.concatenate([p.reshape(-1) for p in contract_rgb_to_i420(rgb)])


# the 8 corners of the RGB cube as studio-range (Y, U, V): black, white, the primaries and their complements
CORNERS_YUV = [(16, 128, 128), (235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (210, 16, 146), (170, 166, 16), (106, 202, 222)]


def yuv_frame(hw, kind="noise", seed=0):
    """(y, u, v) uint8 planes of an h x w frame"""
    h, w = hw
    ch, cw = chroma_hw(h, w)
    rng = np.random.default_rng(2000 + seed)
    if kind == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
    if kind == "corners":  # blocks of the 8 corner colours, chroma constant over each 2 x 2 luma block
        idx = (np.add.outer(np.arange(ch), np.arange(cw)) // 3) % 8
        t = np.array(CORNERS_YUV, np.uint8)
        return np.repeat(np.repeat(t[idx, 0], 2, 0), 2, 1)[:h, :w].copy(), t[idx, 1].copy(), t[idx, 2].copy()
    if kind == "outside":  # bytes outside studio range: Y = 0 and 255, chroma 0 and 255 (the clamps)
        y = rng.choice(np.array([0, 255, 1, 254, 15, 236], np.uint8), (h, w))
        return y, rng.choice(np.array([0, 255, 15, 241], np.uint8), (ch, cw)), rng.choice(np.array([0, 255, 15, 241], np.uint8), (ch, cw))
    if kind == "gradient":
        y = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)
        u = (np.add.outer(np.arange(ch), np.arange(cw) * 5) % 256).astype(np.uint8)
        v = (np.add.outer(np.arange(ch) * 7, np.arange(cw)) % 256).astype(np.uint8)
        return y, u, v
    raise ValueError(kind)


def rgb_frame(hw, kind="noise", seed=0):
    h, w = hw
    rng = np.random.default_rng(3000 + seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "corners":
        idx = np.add.outer(np.arange(h) // 3, np.arange(w) // 5) % 8
        return np.stack([(idx & 1) * 255, ((idx >> 1) & 1) * 255, ((idx >> 2) & 1) * 255], -1).astype(np.uint8)
    if kind == "outside":  # (every RGB byte is legal: the extremes, where the chroma range is widest)
        return rng.choice(np.array([0, 255], np.uint8), (h, w, 3))
    if kind == "gradient":
        g = np.add.outer(np.arange(h) * 3, np.arange(w) * 2)
        return np.stack([g % 256, (g // 2) % 256, (255 - g) % 256], -1).astype(np.uint8)
    raise ValueError(kind)


def padded(plane, pad, fill=0x5A):
    """a view of `plane` inside rows that are `pad` bytes longer (the padding filled with `fill`)"""
    h, w = plane.shape
    buf = np.full((h, w + pad), fill, np.uint8)
    buf[:, :w] = plane
    return buf[:, :w]

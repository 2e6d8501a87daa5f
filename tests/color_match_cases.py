"""THE COLOUR CONTRACT of include/vsd.h restated in numpy (nothing of the library in it), and the cases the colour-match tests share.

`color_match_numpy` is what vsd_color_match_host, the kernels of csrc/color_match.hip and the engine are held to, byte for byte: integer
histograms and prefix sums, Python integers for the 64-bit moments, one np.float64 operation per operation of the contract.  The
generators are deterministic; `case(name)` builds a case once per process and hands out read-only arrays.

Shapes (a workgroup of the device form covers at least 16384 bytes of a frame, at most 64 workgroups per frame, 256 threads, 16-byte
vectors): the smallest frame; 1 x 17 and 5 x 7 with three frames (51 and 105 bytes per frame: frame bases off every alignment, head and
tail only or a few vectors); 8 x 8 (fewer bytes than a workgroup has threads); 64 x 64 (one workgroup) and 72 x 120 (two workgroups) with 1, 3
and 5 frames; 264 x 256 with an all-255 source (Q = 255^2 * 67584 passes 2^32; 13 workgroups of 15597 bytes); 2 x 16384 (a side at the
maximum; 6 workgroups of 16384 bytes, so spans start on every channel); 600 x 601 (1 081 800 bytes: the cap of 64 workgroups, spans of
16904 bytes -- no multiple of 16 or of 3 --, and the partial sums of launch 2 over all 64)."""
import functools
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers_fake_pipeline import FakePipeline  # noqa: E402

MODES = {"histogram": 0, "meanstd": 1}  # include/vsd.h VSD_COLOR_HIST, VSD_COLOR_MEANSTD
AMOUNTS = (0, 1, 128, 255, 256)
FRAME_AMOUNTS = (0, 256, 77, 128, 255)  # amounts that differ within one call: frame f of a call takes FRAME_AMOUNTS[f]
MAX_GAIN = 4.0
MAX_SIDE = 16384
MAX_PIXELS = 1 << 23

SHAPES = ((1, 1, 1), (1, 17, 3), (5, 7, 3), (8, 8, 1), (64, 64, 1), (64, 64, 3), (64, 64, 5), (72, 120, 1), (72, 120, 3), (72, 120, 5),
          (264, 256, 1), (2, MAX_SIDE, 1), (600, 601, 1))  # (h, w, frames)
CONTENTS = ("random", "two_valued", "const_dst", "const_src", "same", "gain_cap")
NAMES = [f"{h}x{w}x{f}-{c}" for h, w, f in SHAPES for c in CONTENTS] + ["264x256x1-src255"]


# ------------------------------------------------------------------------------------------ the contract
def histograms(img):
    """[h][w][3] u8 -> exact counts [3][256]"""
    return np.stack([np.bincount(img[..., c].reshape(-1), minlength=256) for c in range(3)]).astype(np.int64)


def matched_hist(Hs, Hd):
    """HIST: m(v) = the smallest u with 2 Cs[u] >= 2 Cd[v] - Hd[v]"""
    Cs, Cd = np.cumsum(Hs), np.cumsum(Hd)
    assert 2 * Cs[-1] < 2 ** 32
    return np.searchsorted(2 * Cs, 2 * Cd - Hd, side="left").astype(np.int64)


def moments(H):
    v = np.arange(256, dtype=np.int64)
    return int((v * H).sum()), int((v * v * H).sum())


def gain(N, Hs, Hd, capped=True):
    (Ss, Qs), (Sd, Qd) = moments(Hs), moments(Hd)
    Vs, Vd = N * Qs - Ss * Ss, N * Qd - Sd * Sd  # (Python integers: exact)
    assert 0 <= Vs < 2 ** 63 and 0 <= Vd < 2 ** 63 and N * Qs < 2 ** 63 and N * Qd < 2 ** 63
    if Vd == 0:
        return np.float64(0.0)
    g = np.sqrt(np.float64(Vs) / np.float64(Vd))
    return min(g, np.float64(MAX_GAIN)) if capped else g


def matched_meanstd(N, Hs, Hd):
    """MEANSTD: m(v) = clamp(floor((Ss + g (N v - Sd)) / N + 0.5), 0, 255), every operation rounded on its own"""
    Ss, Sd = moments(Hs)[0], moments(Hd)[0]
    g = gain(N, Hs, Hd)
    v = np.arange(256, dtype=np.int64)
    t = (np.float64(Ss) + g * (N * v - Sd).astype(np.float64)) / np.float64(N) + np.float64(0.5)
    return np.clip(np.floor(t), 0, 255).astype(np.int64)


def matched(src, dst, mode):
    """-> m [3][256] of one frame pair"""
    N = src.shape[0] * src.shape[1]
    assert src.shape == dst.shape and src.shape[2] == 3 and N <= MAX_PIXELS
    Hs, Hd = histograms(src), histograms(dst)
    if mode == "histogram":
        return np.stack([matched_hist(Hs[c], Hd[c]) for c in range(3)])
    assert mode == "meanstd"
    return np.stack([matched_meanstd(N, Hs[c], Hd[c]) for c in range(3)])


def apply(dst, m, a):
    """amount and apply: lut[v] = (v (256 - a) + m(v) a + 128) >> 8; dst[p][c] = lut_c[dst[p][c]]"""
    assert 0 <= a <= 256
    v = np.arange(256, dtype=np.int64)
    lut = ((v * (256 - a) + m * a + 128) >> 8).astype(np.uint8)
    return np.stack([lut[c][dst[..., c]] for c in range(3)], axis=-1)


def color_match_numpy(src, dst, mode, a):
    """one frame pair [h][w][3] u8 -> the new dst"""
    return apply(dst, matched(src, dst, mode), a)


# ------------------------------------------------------------------------------------------ the cases
def _content(kind, rng, h, w):
    shape = (h, w, 3)
    full = lambda: rng.integers(0, 256, shape, dtype=np.uint8)  # noqa: E731
    if kind == "random":
        return full(), full()
    if kind == "two_valued":
        return (np.where(rng.integers(0, 2, shape) > 0, 200, 30).astype(np.uint8), np.where(rng.integers(0, 3, shape) > 0, 100, 90).astype(np.uint8))
    if kind == "const_dst":  # Vd = 0, one bin
        return full(), np.full(shape, 77, np.uint8)
    if kind == "const_src":
        return np.full(shape, 200, np.uint8), full()
    if kind == "same":
        s = full()
        return s, s.copy()
    if kind == "gain_cap":  # a dst half a level wide against a full-range src: the gain would be ~150
        return full(), (128 + rng.integers(0, 2, shape)).astype(np.uint8)
    if kind == "src255":  # Q passes 2^32
        return np.full(shape, 255, np.uint8), full()
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (src, dst): read-only u8 [frames][h][w][3]"""
    shape, kind = name.split("-")
    h, w, f = (int(x) for x in shape.split("x"))
    rng = np.random.default_rng([h, w, f, CONTENTS.index(kind) if kind in CONTENTS else len(CONTENTS)])
    pairs = [_content(kind, rng, h, w) for _ in range(f)]
    src, dst = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


@functools.lru_cache(maxsize=None)
def matched_of(name, mode):
    """m [frames][3][256] of a case, computed once (the amount enters only in `apply`)"""
    src, dst = case(name)
    m = np.stack([matched(s, d, mode) for s, d in zip(src, dst)])
    m.setflags(write=False)
    return m


def expected(name, mode, amounts):
    """the new dst [frames][h][w][3] of a case with one amount per frame"""
    _src, dst = case(name)
    m = matched_of(name, mode)
    assert len(amounts) == len(dst)
    return np.stack([apply(d, m[i], a) for i, (d, a) in enumerate(zip(dst, amounts))])


def amount_lists(frames):
    """every amount for all frames, and (more than one frame) amounts that differ within the call"""
    out = [(a,) * frames for a in AMOUNTS]
    if frames > 1:
        out.append(tuple(FRAME_AMOUNTS[:frames]))
    return out


# ------------------------------------------------------------------------------------------ a stand-in for the worker test
class ColorFakePipeline(FakePipeline):
    """helpers_fake_pipeline.FakePipeline with the colour-match surface of VideoSDPipeline: `set_color_match` notes the amount, and every
    frame carries the amount that was in place when it was made in its pixel [0][0][2] (the contract's integer, halved to fit a byte)"""

    def __init__(self, **config):
        super().__init__(**config)
        self.amount = float(config.get("color_amount", 1.0))

    def set_color_match(self, amount):
        if not 0.0 <= amount <= 1.0:
            raise ValueError(f"color_amount must be a number in [0, 1], not {amount!r}")
        self.amount = float(amount)
        return self.amount

    @staticmethod
    def _tag(img, amount):
        a = np.array(img)
        a[0, 0, 2] = int(amount * 256) // 2
        return Image.fromarray(a, "RGB")

    def infer(self, img, **opts):
        return self._tag(super().infer(img, **opts), self.amount)

    def infer_batch(self, imgs, **opts):
        return [self._tag(o, self.amount) for o in super().infer_batch(imgs, **opts)]

    def submit_batch(self, imgs, lane=0, **opts):  # (the two-phase form of the worker loop: a launch keeps the amount it was submitted with)
        return super().submit_batch(imgs, lane=lane, **opts), self.amount

    def collect_batch(self, handle):
        return [self._tag(o, handle[1]) for o in super().collect_batch(handle[0])]

"""Shared by tests/test_keep_mask_host.py and tests/test_keep_mask_gpu.py: the shapes, the masks and the numpy restatement of
THE KEEP MASK (include/vsd.h) that the host twins -- and through them the kernels -- are held to, to the bit.

The restatement is written from the contract text, not from csrc/keep_mask_core.h: integers for the pixel stage and the latent weight,
and for the latent anchor fp32 operations one at a time, the fma evaluated exactly (product and sum in float64, rounded to odd, then
once to fp32: 53 >= 2 * 24 + 2 bits, so the double rounding is innocuous)."""
import functools

import numpy as np
from PIL import Image

from helpers_fake_pipeline import FakePipeline

BLEND_SHAPES = [(1, 1), (3, 5), (8, 24), (16, 40), (72, 120)]  # below a vector step, one vector step and ends, several, three workgroups
LATENT_SHAPES = [(8, 8), (16, 24), (72, 120)]
FRAME_COUNTS = (1, 3)
MASK_KINDS = ("zeros", "full", "edges", "random")
EDGE_VALUES = (0, 1, 127, 128, 254, 255)  # where m >> 7 changes, and the ends
KEEP_HW = (1, 135, 255, 256, 257)  # below a workgroup, one and two workgroups, either side of the edge
KEEP_BATCH = (1, 3)
KEEP_STRIDES = (0, 8)


# ------------------------------------------------------------------------------------------ the contract in numpy
def weight(m):
    m = np.asarray(m).astype(np.int32)
    return m + (m >> 7)


def blend_numpy(src, dst, mask):
    """[..., h, w, 3] u8 x 2, [..., h, w] u8 -> the new dst"""
    a = weight(mask)[..., None]
    return ((src.astype(np.int32) * (256 - a) + dst.astype(np.int32) * a + 128) >> 8).astype(np.uint8)


def latent_numpy(mask):
    """[frames][h][w] u8 -> fp32 [frames][h/8 * w/8]"""
    f, h, w = mask.shape
    S = weight(mask).reshape(f, h // 8, 8, w // 8, 8).sum(axis=(2, 4))
    assert S.min() >= 0 and S.max() <= 16384
    return (S.astype(np.float32) / np.float32(16384.0)).reshape(f, -1)


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, elementwise"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                      # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # two-sum: s + err = p + c exactly
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)  # rounded to odd
    return odd.astype(np.float32)


def keep_step_numpy(x0, wl, n0, coef, stride, hw, batch, lat):
    """x0, lat: f16 [batch*hw][8]; wl: f32 [batch*hw]; n0: f32 [4][hw]; coef: f32, image b's six at b * stride -> the new lat"""
    out = lat.copy()
    for b in range(batch):
        sap, sbp = np.float32(coef[b * stride + 4]), np.float32(coef[b * stride + 5])
        rows = slice(b * hw, (b + 1) * hw)
        w = wl[rows].astype(np.float32)
        for c in range(4):
            kept = fma32(sap, x0[rows, c].astype(np.float32), sbp * n0[c].astype(np.float32))
            v = fma32(w, lat[rows, c].astype(np.float32), (np.float32(1.0) - w) * kept)
            out[rows, c] = np.where(w == 1.0, lat[rows, c], v.astype(np.float16))
    return out


def keep_final_numpy(x0, wl, den):
    out = den.copy()
    w = wl.astype(np.float32)
    for c in range(4):
        v = fma32(w, den[:, c].astype(np.float32), (np.float32(1.0) - w) * x0[:, c].astype(np.float32))
        out[:, c] = np.where(w == 1.0, den[:, c], v.astype(np.float16))
    return out


# ------------------------------------------------------------------------------------------ operands
def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mask(kind, frames, h, w):
    rng = np.random.default_rng(1000 * h + 10 * w + frames)
    if kind == "zeros":
        m = np.zeros((frames, h, w), np.uint8)
    elif kind == "full":
        m = np.full((frames, h, w), 255, np.uint8)
    elif kind == "edges":
        m = np.resize(np.array(EDGE_VALUES, np.uint8), frames * h * w).reshape(frames, h, w)
    else:
        m = rng.integers(0, 256, (frames, h, w), dtype=np.uint8)
    return _ro(m)


@functools.lru_cache(maxsize=None)
def frames_pair(frames, h, w):
    rng = np.random.default_rng(7 + 1000 * h + 10 * w + frames)
    return _ro(rng.integers(0, 256, (frames, h, w, 3), dtype=np.uint8)), _ro(rng.integers(0, 256, (frames, h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def keep_case(hw, batch, stride):
    """-> x0, lat, den (f16 [batch*hw][8]), wl (f32 [batch*hw]), n0 (f32 [4][hw]), coef (f32 [max(1, batch * stride) or 6])"""
    rng = np.random.default_rng(31 * hw + 7 * batch + stride)
    n = batch * hw
    x0, lat, den = ((rng.standard_normal((n, 8)) * s).astype(np.float16) for s in (1.0, 2.0, 1.5))
    wl = (rng.integers(0, 16385, n) / 16384.0).astype(np.float32)
    special = np.array([0.0, 1.0, 1.0 / 16384.0, 0.5, 1.0, 16383.0 / 16384.0], np.float32)
    wl[:min(n, len(special))] = special[:min(n, len(special))] if n > 1 else special[:1]
    if n > 1:  # a row the anchor must leave alone, signed zeros included
        lat[1, :4] = np.array([-0.0, 0.0, -0.0, 1.0], np.float16)
        den[1, :4] = np.array([0.0, -0.0, -0.0, -1.0], np.float16)
    lat[:, 4:], den[:, 4:] = np.float16(0.25), np.float16(-0.5)  # channels 4..7 stay as they are
    n0 = rng.standard_normal((4, hw)).astype(np.float32)
    coef = rng.uniform(0.1, 1.0, max(6, batch * stride)).astype(np.float32)
    return tuple(_ro(a) for a in (x0, lat, den, wl, n0, coef))


def engine_masks(B, H, W):
    """one mask per frame: a half plane, a soft ramp, a small disc (then the three again)"""
    yy, xx = np.mgrid[0:H, 0:W]
    half = np.where(xx < W // 2, 0, 255).astype(np.uint8)
    ramp = np.broadcast_to(np.linspace(0, 255, W).round().astype(np.uint8)[None, :], (H, W)).copy()
    disc = np.where((yy - H // 2) ** 2 + (xx - W // 3) ** 2 <= (min(H, W) // 5) ** 2, 0, 255).astype(np.uint8)
    return np.stack([(half, ramp, disc)[b % 3] for b in range(B)])


# ------------------------------------------------------------------------------------------ a worker stand-in
class KeepFakePipeline(FakePipeline):
    """helpers_fake_pipeline.FakePipeline with the keep-mask surface of VideoSDPipeline: `set_mask` notes the mask, and every frame carries
    the mean of the mask that was in place when it was submitted in its pixel [0][0][2]"""

    def __init__(self, **config):
        super().__init__(**config)
        self.level, self.masks = 255, 0

    def set_mask(self, mask):
        if mask is not None and not (isinstance(mask, Image.Image) and mask.mode in ("L", "1")) and getattr(np.asarray(mask), "ndim", 0) != 2:
            raise ValueError("a mask must be a PIL L / 1 image or a 2-D u8 array")
        self.level = 255 if mask is None else int(np.asarray(mask.convert("L") if isinstance(mask, Image.Image) else mask).mean())
        self.masks += 1
        return self.masks

    @staticmethod
    def _tag(img, level):
        a = np.array(img)
        a[0, 0, 2] = level
        return Image.fromarray(a, "RGB")

    def infer(self, img, **opts):
        return self._tag(super().infer(img, **opts), self.level)

    def infer_batch(self, imgs, **opts):
        return [self._tag(o, self.level) for o in super().infer_batch(imgs, **opts)]

    def submit_batch(self, imgs, lane=0, **opts):  # (the two-phase form of the worker loop: a launch keeps the mask it was submitted with)
        return super().submit_batch(imgs, lane=lane, **opts), self.level

    def collect_batch(self, handle):
        return [self._tag(o, handle[1]) for o in super().collect_batch(handle[0])]

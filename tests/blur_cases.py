"""Shared by tests/test_blur_host.py and tests/test_blur_gpu.py: the shapes, tap tables, image contents and the numpy restatement of
THE BLUR CONTRACT (include/vsd.h) that the host twin -- and the kernel -- are held to, byte for byte; the op emulator and the worker
stand-in with the blur surface; the engine cases the GPU tests and their poisoned child run.

`blur_numpy` is written from the header's text, not from csrc/blur_core.h: two passes of integer sums over clamped PIXEL indices, the two
rounding shifts, nothing about tiles, bytes of a row or words."""
import functools

import numpy as np
import torch

from fake_ops import FakeOps
from helpers_fake_pipeline import FakePipeline

from videosd_amd import blur as BL

# the kernel's tile, mirrored next to `gauss_taps` (videosd_amd/blur.py) and pinned to csrc/blur_core.h by test_blur_host.py: BYTE columns
# of a row of C*w bytes x rows.  With C = 1 the three shapes below are one tile exactly, one byte / row short of it and one beyond it.
TILE_W, TILE_H = BL.TILE_W, BL.TILE_H
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 5), (31, 33), (72, 120), (130, 200),
          (TILE_H, TILE_W), (TILE_H - 1, TILE_W - 1), (TILE_H + 1, TILE_W + 1)]  # (h, w)
CHANNELS = (1, 3)
FRAME_COUNTS = (1, 3)
SKEWS = (0, 1)  # bytes past a 16-byte boundary, for src and dst independently
CONTENTS = ("random", "full", "corners")


def _flat32():
    t = np.zeros(BL.TAPS, np.int32)
    t[0] = 32
    t[2:] = BL.ONE // 65
    t[1] = BL.ONE - 64 * (BL.ONE // 65)  # the residue in the centre
    return t


def _far(R):
    t = np.zeros(BL.TAPS, np.int32)
    t[0], t[1 + R] = R, BL.ONE // 2  # only the two taps R away: a wrong tap index, a wrong clamp or a halo one row short shows
    return t


TAP_SETS = {"identity": BL.identity_taps(), "s0.5": BL.gauss_taps(0.5), "s1.4": BL.gauss_taps(1.4), "s4.0": BL.gauss_taps(4.0),
            "s10.0": BL.gauss_taps(10.0), "flat32": _flat32(), "far1": _far(1), "far32": _far(32)}
for _t in TAP_SETS.values():
    _t.setflags(write=False)


# ------------------------------------------------------------------------------------------ the contract in numpy
def blur_numpy(src, taps):
    """src: u8 [frames][h][w][C] (or [frames][h][w] for C = 1); taps: the int32 [34] table -> dst, the same shape"""
    a = np.asarray(src)
    assert a.dtype == np.uint8
    x = a[..., None] if a.ndim == 3 else a
    t = [int(v) for v in taps]
    R, wt = t[0], t[1:]
    _f, h, w, _c = x.shape
    s = x.astype(np.int64)
    H = np.zeros_like(s)
    for i in range(-R, R + 1):
        H += wt[abs(i)] * s[:, :, np.clip(np.arange(w) + i, 0, w - 1), :]
    h16 = (H + 32) >> 6
    assert h16.max() <= 65280
    V = np.zeros_like(s)
    for j in range(-R, R + 1):
        V += wt[abs(j)] * h16[:, np.clip(np.arange(h) + j, 0, h - 1), :, :]
    assert V.max() + (1 << 21) < 1 << 31
    out = ((V + (1 << 21)) >> 22).astype(np.uint8)
    return out.reshape(a.shape)


# ------------------------------------------------------------------------------------------ operands
def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def image(content, frames, h, w, C):
    if content == "random":
        a = np.random.default_rng(100000 * h + 100 * w + 10 * frames + C).integers(0, 256, (frames, h, w, C), dtype=np.uint8)
    elif content == "full":
        a = np.full((frames, h, w, C), 255, np.uint8)
    else:  # a single 255 pixel in each corner
        a = np.zeros((frames, h, w, C), np.uint8)
        a[:, [0, 0, -1, -1], [0, -1, 0, -1], :] = 255
    return _ro(a)


@functools.lru_cache(maxsize=None)
def expected(content, frames, h, w, C, taps_name):
    """the reference of one case, computed once and shared by the host and the GPU tests"""
    return _ro(blur_numpy(image(content, frames, h, w, C), TAP_SETS[taps_name]))


# ------------------------------------------------------------------------------------------ the op emulator with the blur
class BlurFakeOps(FakeOps):
    """fake_ops.FakeOps with `gauss_blur` through `blur_numpy`, stand-ins for the stages it composes with, and a count of the uploads"""

    def __init__(self):
        super().__init__()
        self.uploads = []

    def clone(self, lane=None):
        return BlurFakeOps()

    def upload(self, dst, src):
        self.uploads.append(dst.data_ptr())
        super().upload(dst, src)

    def gauss_blur(self, src, dst, frames, h, w, channels, taps_dev):
        assert src.dtype == dst.dtype == torch.uint8 and src.numel() == dst.numel() == frames * h * w * channels
        assert taps_dev.dtype == torch.int32 and taps_dev.numel() == BL.TAPS
        out = blur_numpy(src.numpy().reshape(frames, h, w, channels), BL.check_taps(taps_dev.numpy()))
        dst.view(-1).copy_(torch.from_numpy(out.reshape(-1)))

    # the keep-mask ops and the other stages: stand-ins that say where they stand and what they were handed
    def mask_latent(self, mask_u8, frames, h, w, weights_f32):
        weights_f32.copy_(mask_u8.view(frames, h // 8, 8, w // 8, 8).float().mean(dim=(2, 4)).view(frames, -1) / 255.0)

    def latent_keep(self, *a, **k):
        pass

    def mask_blend(self, src_u8, dst_u8, mask_u8, frames, h, w):
        m = mask_u8.view(frames, h, w, 1).int()
        dst_u8.view(frames, h, w, 3).copy_(((src_u8.view(frames, h, w, 3).int() * (255 - m) + dst_u8.view(frames, h, w, 3).int() * m + 127) // 255).to(torch.uint8))

    def color_match(self, *a, **k):
        pass

    def canny_control(self, rgb_u8, h, w, low, high, edge_u8, control_out):
        self.sobel_control(rgb_u8, h, w, 0.11, 0.8, edge_u8, control_out)


# ------------------------------------------------------------------------------------------ a worker stand-in
class BlurFakePipeline(FakePipeline):
    """helpers_fake_pipeline.FakePipeline with the blur surface of VideoSDPipeline: the constructor's `edge_blur` / `mask_feather` and the
    two setters; every frame carries ten times the two sigmas that were in place when it was submitted in its pixels [0][0][1] and [0][0][2]"""

    def __init__(self, **config):
        super().__init__(**config)
        self.sigmas = {k: config.get(k) for k in ("edge_blur", "mask_feather")}

    def _set(self, switch, sigma):
        if self.sigmas[switch] is None:
            raise ValueError(f"set_{switch} needs a pipeline built with {switch}=<sigma>")
        BL.gauss_taps(sigma)
        self.sigmas[switch] = float(sigma)
        return self.sigmas[switch]

    def set_edge_blur(self, sigma):
        return self._set("edge_blur", sigma)

    def set_mask_feather(self, sigma):
        return self._set("mask_feather", sigma)

    def _level(self):
        return tuple(0 if v is None else int(round(10 * v)) for v in (self.sigmas["edge_blur"], self.sigmas["mask_feather"]))

    @staticmethod
    def _tag(img, level):
        from PIL import Image

        a = np.array(img)
        a[0, 0, 1], a[0, 0, 2] = level
        return Image.fromarray(a, "RGB")

    def infer(self, img, **opts):
        return self._tag(super().infer(img, **opts), self._level())

    def infer_batch(self, imgs, **opts):
        return [self._tag(o, self._level()) for o in super().infer_batch(imgs, **opts)]

    def submit_batch(self, imgs, lane=0, **opts):  # (the two-phase form of the worker loop: a launch keeps the sigmas it was submitted with)
        return super().submit_batch(imgs, lane=lane, **opts), self._level()

    def collect_batch(self, handle):
        return [self._tag(o, handle[1]) for o in super().collect_batch(handle[0])]


# ------------------------------------------------------------------------------------------ the engine cases of the GPU tests
B, STEPS = 3, 2
PREP = dict(controlnet_scale=1.5, use_controlnet=True, batch=B, autotune=False, use_graph=True)
EDGE_CASES = (("canny", 64, 64), ("sobel", 72, 120))
EDGE_SIGMA, FEATHER_SIGMA = 1.4, 4.0


def camera(H, W):
    """B noisy ramps (at 64 x 64 the frames behind tests/golden/default_frames_mini_64x64_before_color_match.npy)"""
    rng = np.random.default_rng(11)
    ramp = np.linspace(0, 255, W, dtype=np.float64)[None, :, None]
    tints = np.array([[1.0, 0.6, 0.3], [0.3, 1.0, 0.7], [0.8, 0.8, 0.2]])
    return np.stack([np.clip(ramp * tints[b][None, None, :] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8) for b in range(B)])


def edge_camera(H, W):
    """the camera frames with hard-edged shapes drawn in -- a bright bar, a dark disc, a mid-gray box per frame --, so that the edge ops find
    edges with and without a blur ahead of them (on the noisy ramps alone a blurred frame has none above the Canny thresholds)"""
    a = camera(H, W).copy()
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        a[b, H // 8:H // 8 + H // 5, W // 6 + 3 * b:W - W // 6] = 250
        a[b][(yy - (2 * H) // 3) ** 2 + (xx - W // 3 - 5 * b) ** 2 <= (min(H, W) // 6) ** 2] = 4
        a[b, H // 2:H // 2 + H // 4, (2 * W) // 3:(2 * W) // 3 + W // 5] = (90, 160, 30)
    return a


def make_engine():
    from videosd_amd import config as C
    from videosd_amd import weights as Wt
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu = Wt.synthesize(Wt.unet_spec(C.MINI_UNET), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(C.MINI_CONTROLNET), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(C.TAESD), "vae.", device="cuda")
    eng = Engine(HipOps(0), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def edge_case(eng, mode, H, W, sigma=EDGE_SIGMA):
    """`edges=mode, edge_blur=sigma` on the frames of `edge_camera` -> out_u8, edge_u8, the control buffer and x0 (fp16 as u16)"""
    eng.prepare(H, W, STEPS, 0.6, edges=mode, edge_blur=sigma, **PREP)
    out = eng.infer_u8(edge_camera(H, W)).copy()
    return dict(out=out, edge=_cpu(eng.edge_u8), control=_cpu(eng.buffers["control"]).view(np.uint16), x0=_cpu(eng.buffers["x0"]).view(np.uint16))


def feather_case(eng, masks, H=64, W=64, sigma=FEATHER_SIGMA):
    """`keep_mask=True, mask_feather=sigma` with `masks` on the camera frames -> out_u8"""
    eng.prepare(H, W, STEPS, 0.6, keep_mask=True, mask_feather=sigma, **PREP)
    eng.set_masks(masks)
    return dict(out=eng.infer_u8(camera(H, W)).copy())


def digest(case):
    import hashlib

    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in case.items()}

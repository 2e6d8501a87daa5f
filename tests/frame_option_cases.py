"""TEST-ONLY helpers of the per-frame option tests: numpy restatements of the four ops of a `frame_options` program (include/vsd.h
vsd_add_noise_frames, vsd_lcm_step_frames, vsd_groupnorm_addvec, vsd_cn_merge_frames) on top of the op emulator, which has none of them
(tests/fake_ops.py), the layouts' slots restated from their definition, and a stand-in pipeline for the worker tests."""
import numpy as np
import torch

from frame_prompt_cases import FramePromptFakeOps
from helpers_fake_pipeline import FakePipeline

SENTINEL = 0xA5
# (strength, controlnet_scale) of the engine tests: both give two timesteps at steps = 2
OPT_A, OPT_B = (0.6, 1.5), (0.9, 0.4)


def per_image(t, count: int, width: int, stride: int):
    """image b's `width` elements at t + b * stride elements: what a kernel that is handed frame 0's pointer and a stride reads"""
    return t.as_strided((count, width), (stride, 1))


def groupnorm_addvec_ref(x, vec, groups, eps, gamma, beta, silu):
    """x [B][hw][c], vec [B][c], gamma / beta [c], all float64 numpy -> GroupNorm of x + vec per image"""
    B, hw, c = x.shape
    s = (x + vec[:, None, :]).reshape(B, hw, groups, c // groups)
    mean = s.mean(axis=(1, 3), keepdims=True)
    var = ((s - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((s - mean) / np.sqrt(var + eps)).reshape(B, hw, c) * gamma + beta
    return y / (1.0 + np.exp(-y)) if silu else y


def cn_merge_ref(z, u, scale):
    """z, u: fp16 [B][rows][c]; scale fp32 [B] -> fp16(fp32(fp64 fma)): exact inputs make the fp64 fma exact (the GPU test asserts that)"""
    f = z.astype(np.float64) * scale.astype(np.float64)[:, None, None] + u.astype(np.float64)
    return f.astype(np.float32).astype(np.float16)


def slot_bytes(lay, name, frame):
    """[first, last) byte of frame `frame`'s slot of item `name`, from the layout's definition"""
    off, nb = lay.items[name]
    return off + frame * nb, off + (frame + 1) * nb


class FrameOptionFakeOps(FramePromptFakeOps):
    """the op emulator plus the four ops of a `frame_options` program; counts the merge launches (and, inherited, the installs per slot)"""

    def __init__(self):
        super().__init__()
        self.merges = 0

    def clone(self, lane=None):
        return FrameOptionFakeOps()

    def add_noise_frames(self, x0, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, out):
        assert (noise_f32 is None) != (seeds_dev is None) and seeds_dev is None, "the emulator has the table noise only"
        assert coef_stride >= 2
        k = per_image(coef_dev, batch, 2, coef_stride)
        for b in range(batch):
            self.add_noise(x0[b * hw:(b + 1) * hw], noise_f32, float(k[b, 0]), float(k[b, 1]), hw, out[b * hw:(b + 1) * hw])

    def lcm_step_frames(self, eps, sample, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, prev, denoised, dec_in=None):
        assert seeds_dev is None, "the emulator has the table noise only"
        assert coef_stride >= 6
        k = per_image(coef_dev, batch, 6, coef_stride)
        sl = lambda t, b: None if t is None else t[b * hw:(b + 1) * hw]  # noqa: E731
        for b in range(batch):
            self.lcm_step(sl(eps, b), sl(sample, b), noise_f32, [float(v) for v in k[b]], hw, sl(prev, b), sl(denoised, b), sl(dec_in, b))

    def groupnorm_addvec(self, src, addvec, ld_addvec, c, hw, groups, eps, gamma, beta, silu, out, batch=1):
        assert ld_addvec % 8 == 0 and c % 8 == 0 and addvec.dtype == torch.float16
        vec = per_image(addvec, batch, c, ld_addvec).double().numpy()
        x = src[:batch * hw, :c].double().numpy().reshape(batch, hw, c)
        y = groupnorm_addvec_ref(x, vec, groups, eps, gamma.double().numpy(), beta.double().numpy(), silu)
        out[:batch * hw, :c] = torch.from_numpy(y.reshape(batch * hw, c)).half()

    def cn_merge_frames(self, segs_dev, nseg, scales_dev, scale_stride, batch, tensors=None):
        assert tuple(segs_dev.shape) == (nseg, 6) and 1 <= nseg <= 16 and len(tensors) == nseg
        assert tuple(scales_dev.shape) == (batch, scale_stride)
        self.merges += 1
        for (za, ua, oa, rows, c, col), (z, u, o) in zip(segs_dev.tolist(), tensors):
            assert (za, ua, oa) == (z.data_ptr(), u.data_ptr(), o.data_ptr()) and c % 8 == 0 and 0 <= col < scale_stride
            assert tuple(z.shape) == tuple(u.shape) == tuple(o.shape) == (batch * rows, c)
            got = cn_merge_ref(z.numpy().reshape(batch, rows, c), u.numpy().reshape(batch, rows, c), scales_dev[:, col].numpy())
            o.copy_(torch.from_numpy(got.reshape(batch * rows, c)))


class OptionPipeline(FakePipeline):
    """stand-in for the worker tests: records what every launch was given; takes `strength` / `controlnet_scale` as lists"""
    SUBMITS = []

    def submit_batch(self, imgs, lane=0, **opts):
        type(self).SUBMITS.append((len(imgs), opts.get("strength"), opts.get("controlnet_scale"), opts.get("steps")))
        first = lambda v: v[0] if isinstance(v, list) else v  # noqa: E731
        opts = dict(opts, strength=first(opts.get("strength", 0.4)), controlnet_scale=first(opts.get("controlnet_scale", 1)))
        return super().submit_batch(imgs, lane=lane, **opts)


class PerFrameOptionPipeline(OptionPipeline):
    per_frame_options = True
    NEEDS_IDLE = []

    def option_class(self, options):
        from videosd_amd.lcm import lcm_timesteps

        return len(lcm_timesteps(float(options.get("strength", 0.4)), int(options.get("steps", 20))))

    def needs_idle(self, **options):
        type(self).NEEDS_IDLE.append(options.get("strength"))
        return False

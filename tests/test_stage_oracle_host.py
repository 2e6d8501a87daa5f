"""The frame-level reference of the opt-in stages, without a GPU (tests/stage_oracle.py):

  * the pin: with every hook off `stage_frame` returns `OraclePipeline.infer(..., keep_trace=True)`'s frame and traces bit for bit, so
    the restated loop cannot drift from the oracle that tests/golden_guard.py digests;
  * the engine on the op emulator with `keep_mask=True` -- alone, with seeded noise, with per-frame options, and with every per-frame
    switch at once -- against `stage_frame` per frame, each frame with its own inputs;
  * the separation: every mutant of `stage_frame` (one wiring error of the keep mask each) lies at least 3 x the case's bound from the
    right frame, so the bound the GPU test holds the kernels to tells the right wiring from each of them.

The emulator carries every switch: the keep-mask ops, `color_match` and `canny_control` are the numpy restatements of their contracts
(no built library is needed here), the seeded forms draw from `seed_cases.normal_draw`; nothing is left to the GPU test alone but the
kernels themselves.  What the walks of tests/test_keep_mask_host.py / tests/test_keep_mask_gpu.py prove call by call, this file proves
of the frame."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import canny_cases as CC  # noqa: E402
import color_match_cases as CM  # noqa: E402
import keep_mask_cases as KM  # noqa: E402
import seed_cases as SC  # noqa: E402
import stage_oracle as SO  # noqa: E402
from prompt_mix_cases import PromptMixFakeOps  # noqa: E402

from oracle.pipeline import OraclePipeline  # noqa: E402
from videosd_amd import blocks as BK  # noqa: E402
from videosd_amd import config as C  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

MAD_MAX = 1.5  # mean |difference| in LSB: the bound of tests/test_frame_prompts_gpu.py `_engine_case`, as the GPU test takes it


# ------------------------------------------------------------------------------------------ the emulator with every switch
class StageFakeOps(PromptMixFakeOps):
    """the op emulator with per-frame prompts, mixes and options (inherited) plus: the three keep-mask ops, `color_match` and
    `canny_control` as the numpy restatements of their contracts, and the seeded forms of the scheduler ops and of `latent_keep`, which
    draw from `seed_cases.normal_draw`.  Keeps the frame `postprocess_rgb` wrote, ahead of the post stages."""

    def __init__(self):
        super().__init__()
        self.before = None

    def clone(self, lane=None):
        return StageFakeOps()

    def postprocess_rgb(self, img, ld, hw, rgb_u8):
        super().postprocess_rgb(img, ld, hw, rgb_u8)
        self.before = rgb_u8.clone()

    # ---- THE NOISE CONTRACT
    @staticmethod
    def _draw(seeds_dev, b, kind, draw, hw):
        return torch.from_numpy(SC.normal_draw(int(seeds_dev[b]) % (1 << 64), kind, draw, hw)).float()

    def add_noise_seeded(self, x0, seeds_dev, kind, draw, coef_dev, hw, batch, out):
        for b in range(batch):
            self.add_noise_dev(x0[b * hw:(b + 1) * hw], self._draw(seeds_dev, b, kind, draw, hw), coef_dev, hw, 1, out[b * hw:(b + 1) * hw])

    def lcm_step_seeded(self, eps, sample, seeds_dev, kind, draw, coef_dev, hw, batch, prev, denoised, dec_in=None):
        sl = lambda t, b: None if t is None else t[b * hw:(b + 1) * hw]  # noqa: E731
        for b in range(batch):
            nz = self._draw(seeds_dev, b, kind, draw, hw) if draw > 0 else None
            self.lcm_step_dev(sl(eps, b), sl(sample, b), nz, coef_dev, hw, 1, sl(prev, b), sl(denoised, b), sl(dec_in, b))

    def add_noise_frames(self, x0, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, out):
        if seeds_dev is None:
            return super().add_noise_frames(x0, noise_f32, None, kind, draw, coef_dev, coef_stride, hw, batch, out)
        assert noise_f32 is None and coef_stride >= 2
        k = coef_dev.as_strided((batch, 2), (coef_stride, 1))
        for b in range(batch):
            self.add_noise(x0[b * hw:(b + 1) * hw], self._draw(seeds_dev, b, kind, draw, hw), float(k[b, 0]), float(k[b, 1]), hw, out[b * hw:(b + 1) * hw])

    def lcm_step_frames(self, eps, sample, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, prev, denoised, dec_in=None):
        if seeds_dev is None and not draw:
            return super().lcm_step_frames(eps, sample, noise_f32, None, kind, draw, coef_dev, coef_stride, hw, batch, prev, denoised, dec_in)
        assert noise_f32 is None and seeds_dev is not None and coef_stride >= 6
        k = coef_dev.as_strided((batch, 6), (coef_stride, 1))
        sl = lambda t, b: None if t is None else t[b * hw:(b + 1) * hw]  # noqa: E731
        for b in range(batch):
            self.lcm_step(sl(eps, b), sl(sample, b), self._draw(seeds_dev, b, kind, draw, hw), [float(v) for v in k[b]], hw, sl(prev, b), sl(denoised, b),
                          sl(dec_in, b))

    # ---- THE EDGE CONTRACT, THE COLOUR CONTRACT
    def canny_control(self, rgb_u8, h, w, low, high, edge_u8, control_out):
        e = torch.from_numpy(CC.canny_numpy(rgb_u8.reshape(h, w, 3).numpy(), low, high).reshape(-1).copy())
        edge_u8.copy_(e)
        control_out.zero_()
        for c in range(3):
            control_out[:, c] = (e > 0).half()

    def color_match(self, src_u8, dst_u8, frames, h, w, mode, amounts_dev):
        src, dst = src_u8.reshape(frames, h, w, 3).numpy(), dst_u8.reshape(frames, h, w, 3)
        for f in range(frames):
            dst[f].copy_(torch.from_numpy(CM.color_match_numpy(src[f], dst[f].numpy(), mode, int(amounts_dev[f]))))

    # ---- THE KEEP MASK
    def mask_blend(self, src_u8, dst_u8, mask_u8, frames, h, w):
        out = KM.blend_numpy(src_u8.numpy().reshape(frames, h, w, 3), dst_u8.numpy().reshape(frames, h, w, 3), mask_u8.numpy().reshape(frames, h, w))
        dst_u8.view(-1).copy_(torch.from_numpy(out.reshape(-1)))

    def mask_latent(self, mask_u8, frames, h, w, weights_f32):
        weights_f32.view(-1).copy_(torch.from_numpy(KM.latent_numpy(mask_u8.numpy().reshape(frames, h, w)).reshape(-1)))

    def latent_keep(self, x0, weights_f32, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, lat=None, den=None, dec_in=None):
        wl = weights_f32.numpy().reshape(-1)
        if lat is None:
            assert noise_f32 is None and seeds_dev is None and coef_dev is None
            den.copy_(torch.from_numpy(KM.keep_final_numpy(x0.numpy(), wl, den.numpy())))
            dec_in.zero_()
            dec_in[:, :4] = (torch.tanh(den[:, :4].float() / 3.0) * 3.0).half()
            return
        assert (noise_f32 is None) != (seeds_dev is None) and (kind, draw) == (0, 0) and den is None and dec_in is None
        six = coef_dev.as_strided((batch, 6), (coef_stride, 1)).contiguous().numpy()  # (stride 0: every image the launch's one set)
        for b in range(batch):
            rows = slice(b * hw, (b + 1) * hw)
            n0 = (noise_f32.contiguous() if seeds_dev is None else self._draw(seeds_dev, b, 0, 0, hw)).numpy().reshape(4, hw)
            lat[rows] = torch.from_numpy(KM.keep_step_numpy(x0[rows].numpy(), wl[rows], n0, six[b], 0, hw, 1, lat[rows].numpy()))


# ------------------------------------------------------------------------------------------ networks
@functools.lru_cache(maxsize=None)
def _nets(which):
    ucfg, ccfg = (C.MINI_UNET, C.MINI_CONTROLNET) if which == "mini" else (C.SD15_UNET, C.SD15_CONTROLNET)
    wu = W.synthesize(W.unet_spec(ucfg), "unet.")
    wc = W.synthesize(W.controlnet_spec(ccfg), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    return ucfg, ccfg, wu, wc, wv, SO.texts(ucfg.cross_dim)


@functools.lru_cache(maxsize=None)
def _oracle(which):
    ucfg, ccfg, wu, wc, wv, _t = _nets(which)
    return OraclePipeline(ucfg, ccfg, wu, wc, wv)


@functools.lru_cache(maxsize=None)
def _engine(which="mini"):
    ucfg, ccfg, wu, wc, wv, (ta, tb) = _nets(which)
    eng = Engine(StageFakeOps(), ucfg, ccfg, C.TAESD, wu, wc, wv)
    eng.set_text_embeds(ta)
    a, b = eng.build_prompt(ta), eng.build_prompt(tb)
    return eng, (a, b, BK.PromptMix([a, b], SO.MIX_WEIGHTS))


# ------------------------------------------------------------------------------------------ 1. the pin
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("cn", [True, False])
@pytest.mark.parametrize("which", ["mini", "sd15"])
def test_with_every_hook_off_the_loop_is_the_oracles_bit_for_bit(which, cn, steps):
    orc = _oracle(which)
    ta = _nets(which)[5][0]
    img = Image.fromarray(SO.frames(64, 64)[0], "RGB")
    kw = dict(height=64, width=64, strength=SO.STRENGTH, steps=steps, controlnet_scale=SO.SCALE, use_controlnet=cn)
    ref = np.asarray(orc.infer(img, ta[None].float(), seed=23, keep_trace=True, **kw))
    want = orc.trace
    real = torch.randn
    got = SO.stage_frame(orc, img, ta, rng_seed=23, **kw)
    assert torch.randn is real
    eq = lambda x, y: x.shape == y.shape and np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))  # noqa: E731
    assert eq(got.init_latents, want["init_latents"]) and eq(got.noisy_latents, want["noisy_latents"]) and eq(got.decoded, want["decoded"])
    assert len(got.denoised) == len(want["denoised"]) == steps and all(eq(x, y) for x, y in zip(got.denoised, want["denoised"]))
    assert np.array_equal(got.before, ref) and np.array_equal(got.frame, ref) and got.wl is None
    assert got.timesteps == orc.sched.timesteps.tolist() and len(got.timesteps) == steps


def test_the_mask_hook_at_its_ends():
    """an all-255 mask is the plain frame bit for bit (wl = 1: x * 1 + 0 * kept); an all-0 mask keeps the input's latents and the camera's frame"""
    orc, ta = _oracle("mini"), _nets("mini")[5][0]
    cam = SO.frames(64, 64)[1]
    img = Image.fromarray(cam, "RGB")
    kw = dict(height=64, width=64, strength=SO.STRENGTH, steps=SO.STEPS, controlnet_scale=SO.SCALE)
    plain = SO.stage_frame(orc, img, ta, **kw)
    full = SO.stage_frame(orc, img, ta, mask=np.full((64, 64), 255, np.uint8), **kw)
    assert torch.equal(full.denoised[-1], plain.denoised[-1]) and np.array_equal(full.frame, plain.frame)
    none = SO.stage_frame(orc, img, ta, mask=np.zeros((64, 64), np.uint8), **kw)
    assert torch.equal(none.denoised[-1], none.init_latents) and np.array_equal(none.frame, cam) and not np.array_equal(none.before, cam)


# ------------------------------------------------------------------------------------------ 2. the engine on the emulator, and the mutants
@functools.lru_cache(maxsize=None)
def measure(case, H, Wd, which="mini", mutants=SO.MUTANTS):
    """-> per frame: (r1 of the emulator's engine against the stage oracle, r1 over the mixed latent pixels, mean LSB over the restyled pixels
    ahead of the post stages, {mutant: r1 of the mutant from the right oracle frame}); asserts what is exact on the way"""
    eng, blocks = _engine(which)
    orc = _oracle(which)
    camera, ms = SO.frames(H, Wd), SO.masks(H, Wd)
    SO.prepare_case(eng, case, H, Wd, blocks, use_graph=False)
    got = SO.launch_case(eng, case, camera)
    before = eng.ops.before.numpy().reshape(SO.B, H, Wd, 3).copy()
    sw = SO.CASES[case]
    h0, w0 = H // 8, Wd // 8
    assert np.array_equal(eng.mask_w.numpy(), KM.latent_numpy(ms))
    rows = []
    for b in range(SO.B):
        # the final frame: the numpy post stages on the engine's own frame ahead of them, byte for byte
        assert np.array_equal(got[b], SO.post_stages(camera[b], before[b], ms[b], sw.get("color_match"))), (case, b)
        assert np.array_equal(got[b][ms[b] == 0], camera[b][ms[b] == 0])
        right = SO.oracle_case(orc, case, H, Wd, b, _nets(which)[5], camera)
        assert eng.plan["timesteps"] == right.timesteps or sw.get("frame_options")
        den, ref = SO.latents_of(eng.buffers["denoised"], b, h0, w0), right.denoised[-1][0]
        r0 = SO.r1(SO.latents_of(eng.buffers["x0"], b, h0, w0), right.init_latents[0])
        assert r0 <= SO.R0_MAX, (case, b, r0)
        mixed = ((right.wl[0] > 0) & (right.wl[0] < 1)).expand(4, h0, w0)
        far = {m: SO.r1(SO.oracle_case(orc, case, H, Wd, b, _nets(which)[5], camera, mutant=m).denoised[-1][0], ref) for m in mutants}
        rows.append((SO.r1(den, ref), SO.r1(den, ref, mixed) if bool(mixed.any()) else 0.0, SO.mad(before[b], right.before, ms[b] == 255), far))
    return rows


@pytest.mark.parametrize("case,H,Wd,which", list(SO.MEASURED))
def test_engine_on_the_emulator_and_every_mutant(case, H, Wd, which):
    rows = measure(case, H, Wd, which)
    bound = SO.bound(case, H, Wd, which)
    for b, (r1, r1_mixed, lsb, far) in enumerate(rows):
        nearest = min(far, key=far.get)
        print(f"{case} {which} {Wd}x{H} frame {b}: r1 {r1:.2e} (mixed {r1_mixed:.2e}) LSB {lsb:.3f} | bound {bound:.2e} | nearest mutant {nearest} {far[nearest]:.2e} | "
              + " ".join(f"{m} {d:.2e}" for m, d in far.items()))
    for b, (r1, r1_mixed, lsb, far) in enumerate(rows):
        # the emulator itself within half the bound: the other half is the kernels' (bound = 4 x the recorded emulator distance)
        assert r1 <= bound / 2 and r1_mixed <= bound / 2 and lsb <= MAD_MAX, (case, b, r1, r1_mixed, lsb, bound)
        for m, d in far.items():
            assert d >= SO.SEPARATION * bound, (case, b, m, d, bound)


def test_the_recorded_measurements_are_these():
    """the constants of tests/stage_oracle.py against what this machine measures, so that the table beside the bounds stays a measurement.
    A mutant's distance is the oracle against the oracle, fp32 on both sides: within a quarter of the recorded one.  The emulator's distance
    is the sum of the fp16 roundings of its stores, which fall differently with another BLAS or thread count (one frame read 8.8e-4 on one
    machine and 1.15e-3 on another): the largest of a case, which is what the bound is made of, within a factor of two either way."""
    assert {k[:3] for k in SO.MEASURED if k[3] == "mini"} == {(c, H, Wd) for c in SO.CASES for H, Wd in SO.SIZES}
    for (case, H, Wd, which), recorded in SO.MEASURED.items():
        rows = measure(case, H, Wd, which)
        worst, rec_worst = max(r[0] for r in rows), max(r1 for r1, _far in recorded)
        assert 0.5 * rec_worst <= worst <= 2.0 * rec_worst, (case, H, Wd, which, worst, rec_worst)
        for b, ((_r1, _r1m, _lsb, far), (_rec_r1, rec_far)) in enumerate(zip(rows, recorded)):
            assert 0.75 * rec_far <= min(far.values()) <= 1.25 * rec_far, (case, H, Wd, b, min(far.values()), rec_far)

"""The oracle's frame loop with the opt-in stages, each stated from its contract in include/vsd.h: the frame-level reference of
tests/test_stage_oracle_host.py and tests/test_stage_oracle_gpu.py.

`stage_frame` restates the loop of `OraclePipeline.infer` (oracle/pipeline.py) for one frame, in fp32 on the CPU: the same `oracle.nets`
forwards and `oracle.scheduler` methods in the same order, so that with every hook off it returns that method's frame and traces bit for
bit (tests/test_stage_oracle_host.py pins that; oracle/ itself is digested by tests/golden_guard.py and does not change).  The hooks:

  edges     "canny": `canny_cases.canny_numpy` (THE EDGE CONTRACT) in place of `sobel_edges`
  seed      draw d of the frame is `seed_cases.normal_draw(seed, 0, d, hw)` (THE NOISE CONTRACT) in place of the d-th `torch.randn`
  text      the frame's own embeddings, or [(embeddings, weight), ...]: the weighted sum of the embeddings (THE PROMPT MIX is linear in them)
  strength, controlnet_scale: the frame's own
  mask      THE KEEP MASK: wl = `keep_mask_cases.latent_numpy(mask)`; behind every step but the last
            latents = wl * latents + (1 - wl) * sched.add_noise(init, draw 0, ts[i + 1]); behind the last den = wl * den + (1 - wl) * init,
            which is what is decoded.  The kept latents come from the oracle scheduler's `alphas_cumprod` by TIMESTEP: no table of the
            engine is read here, and nothing of the library is imported.
  color_match, mask: the post stages in the engine's order -- `color_match_cases.color_match_numpy` over the whole decoded frame, then
            `keep_mask_cases.blend_numpy` of the camera's frame into it.

`mutant=` makes ONE deliberate wiring error of the keep mask (MUTANTS); the host test shows that every one of them lies at least
3 x the bound of its case from the right frame, so a bound that passes says the wiring is none of these."""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

import canny_cases as CC
import color_match_cases as CM
import keep_mask_cases as KM
import seed_cases as SC
from oracle import nets
from oracle.pipeline import center_crop_resize, postprocess, preprocess_control, preprocess_image, reset_rng, sobel_edges
from oracle.scheduler import w_embedding

# one wiring error each: the anchor noised to THIS step's timestep | with a draw nobody else used | with draw 1 | no anchor at all (neither
# the steps' nor the final one) | the anchor's (and the final blend's) latents those of another frame | the final blend left out
MUTANTS = ("this_t", "fresh", "draw1", "none", "other_init", "no_final")

# ------------------------------------------------------------------------------------------ the shared cases
STEPS, B = 3, 3
SIZES = ((64, 64), (72, 120))  # (H, W): 8 x 8 latents, and 9 x 15 -- odd sides, rows and columns that differ
SCALE = 1.5
STRENGTH = 0.6
OPTIONS = ((0.5, 1.5), (0.8, 0.4), (0.65, 1.0))  # (strength, controlnet_scale) per frame: three timesteps each at 3 steps, all different
SEEDS = (5, 2 ** 40 + 7, 99)  # one above 2^32
CANNY = (100, 200)
MIX_WEIGHTS = (0.25, 0.75)
R0_MAX = 5e-3  # x0 against init_latents: the bound of tests/test_seed_gpu.py and tests/test_pipeline_gpu.py


def frames(H, W):
    """three camera frames: a tinted wave pattern of its own under noise each (edges for both edge stages, colours that differ per
    channel, and latents that differ from frame to frame, so that another frame's latents are a wrong anchor)"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    tints = np.array([[1.0, 0.6, 0.3], [0.3, 1.0, 0.7], [0.8, 0.8, 0.2]])
    out = []
    for b in range(B):
        base = 127 + 100 * np.sin(xx / (7.0 + 2 * b) + b) * np.cos(yy / (5.0 + b) + 2 * b)
        out.append(np.clip(base[..., None] * tints[b] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def masks(H, W):
    """one mask per frame -- a half plane, a soft ramp, a disc: 255 restyled, 0 kept.  The disc is the KEPT part, an ellipse with half axes
    of 3/8 of the sides (44 % of the frame): with the disc of `keep_mask_cases.engine_masks` (a fifth of the shorter side; a dozen kept
    latent pixels of 64) the wrong-timestep mutant lies 1.3e-2 from the right frame, which 3 x the bound does not separate; with this
    one every mutant lies 2e-2 or more away (MEASURED below)."""
    yy, xx = np.mgrid[0:H, 0:W]
    half = np.where(xx < W // 2, 0, 255).astype(np.uint8)
    ramp = np.broadcast_to(np.linspace(0, 255, W).round().astype(np.uint8)[None, :], (H, W)).copy()
    disc = np.where(((yy - H // 2) / (3 * H / 8)) ** 2 + ((xx - W // 2) / (3 * W / 8)) ** 2 <= 1.0, 0, 255).astype(np.uint8)
    return np.stack([half, ramp, disc])


def texts(cross_dim):
    """the two prompts of the per-frame prompt tests (text B with twice the spread, as tests/test_prompt_mix_gpu.py has it)"""
    a = (torch.randn(77, cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half()
    b = torch.randn(77, cross_dim, generator=torch.Generator().manual_seed(8)).half()
    return a, b


def frame_texts(a, b):
    """what frame 0, 1, 2 of an all-switches launch is prompted with: A, the mix, B -- in `stage_frame`'s form"""
    return [a, [(a, MIX_WEIGHTS[0]), (b, MIX_WEIGHTS[1])], b]


CASES = {  # the switches of `Engine.prepare` besides keep_mask=True
    "keep": dict(),
    "seed": dict(device_seed=True),
    "options": dict(frame_options=True),
    "all": dict(frame_prompts=True, frame_options=True, device_seed=True, edges="canny", canny_thresholds=CANNY, color_match="histogram"),
}


def prepare_case(eng, case, H, W, blocks, **kw):
    """`eng` prepared for `case` with the case's masks, options and prompts installed; blocks: (A, B, the mix) of `eng.build_prompt` /
    PromptMix.  -> the plan"""
    sw = CASES[case]
    a, _b, _mix = blocks
    if sw.get("frame_prompts"):
        eng.use_prompts(list(blocks_of_frames(blocks)))
    else:
        eng.use_prompt(a)
    first = OPTIONS[0] if sw.get("frame_options") else (STRENGTH, SCALE)
    plan = eng.prepare(H, W, STEPS, first[0], controlnet_scale=first[1], use_controlnet=True, batch=B, keep_mask=True, **sw, **kw)
    assert plan["n"] == STEPS and plan["keep_mask"] is True
    if sw.get("frame_options"):
        eng.use_options(list(OPTIONS))
    eng.set_masks(masks(H, W))
    return plan


def blocks_of_frames(blocks):
    a, b, mix = blocks
    return a, mix, b


def launch_case(eng, case, camera):
    """one launch of the prepared case -> the frames"""
    eng.submit_u8(camera, **({"seeds": list(SEEDS)} if CASES[case].get("device_seed") else {}))
    return eng.collect_u8()


def oracle_case(orc, case, H, W, b, text_ab, camera, mutant=None):
    """frame b of `case` by `stage_frame`, with that frame's own inputs"""
    sw = CASES[case]
    strength, scale = OPTIONS[b] if sw.get("frame_options") else (STRENGTH, SCALE)
    text = frame_texts(*text_ab)[b] if sw.get("frame_prompts") else text_ab[0]
    return stage_frame(orc, Image.fromarray(camera[b], "RGB"), text, H, W, strength, STEPS, controlnet_scale=scale, use_controlnet=True,
                       seed=SEEDS[b] if sw.get("device_seed") else None, edges=sw.get("edges", "sobel"), mask=masks(H, W)[b],
                       color_match=sw.get("color_match"), mutant=mutant, other=Image.fromarray(camera[(b + 1) % B], "RGB"))


# ------------------------------------------------------------------------------------------ the bounds
# bound(case) = 4 x the largest r1 (relative L2 distance of the final denoised latents, per frame) of the engine on the op emulator
# against `stage_frame`, both computed on the CPU: the emulator has the engine's fp16 storage and fp32 arithmetic; 4 gives room for the
# kernels' fp16 MFMA arithmetic over it (README: 0.9e-3 to 1.1e-3 on the device as well).  Measured (tests/test_stage_oracle_host.py
# prints them; frame 0 / 1 / 2 = half plane / ramp / disc), with the smallest distance of any mutant from the right frame beside them:
#
#   (case, H, W, networks): per frame (emulator r1, smallest mutant distance)
MEASURED = {
    ("keep", 64, 64, "mini"): [(9.67e-04, 4.97e-02), (8.78e-04, 6.25e-02), (7.27e-04, 2.92e-02)],
    ("keep", 72, 120, "mini"): [(8.70e-04, 3.28e-02), (9.58e-04, 6.02e-02), (8.33e-04, 2.92e-02)],
    ("seed", 64, 64, "mini"): [(6.56e-04, 2.59e-02), (9.02e-04, 5.47e-02), (7.82e-04, 3.57e-02)],
    ("seed", 72, 120, "mini"): [(8.98e-04, 2.71e-02), (9.41e-04, 5.56e-02), (8.80e-04, 2.99e-02)],
    ("options", 64, 64, "mini"): [(1.03e-03, 6.86e-02), (9.37e-04, 3.15e-02), (7.81e-04, 2.38e-02)],
    ("options", 72, 120, "mini"): [(9.21e-04, 4.12e-02), (1.08e-03, 3.13e-02), (8.98e-04, 2.44e-02)],
    ("all", 64, 64, "mini"): [(7.55e-04, 3.20e-02), (6.50e-04, 2.70e-02), (9.50e-04, 2.72e-02)],
    ("all", 72, 120, "mini"): [(9.64e-04, 3.51e-02), (9.47e-04, 2.74e-02), (8.01e-04, 2.50e-02)],
    ("keep", 64, 64, "sd15"): [(7.54e-04, 3.35e-02), (9.43e-04, 5.80e-02), (7.12e-04, 2.65e-02)],
    ("all", 64, 64, "sd15"): [(7.65e-04, 3.02e-02), (6.86e-04, 2.45e-02), (6.43e-04, 2.22e-02)],
}
BOUNDS = {case: 4.0 * max(r1 for r1, _m in rows) for case, rows in MEASURED.items()}
SEPARATION = 3.0  # every mutant lies at least this many bounds from the right frame


def bound(case, H, W, which="mini"):
    return BOUNDS[(case, H, W, which)]


# ------------------------------------------------------------------------------------------ the quantities compared
def r1(a, b, sel=None):
    """the relative L2 distance of `a` from the reference `b` (over the elements `sel`)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if sel is not None:
        a, b = a[sel], b[sel]
    return float((a - b).norm() / b.norm())


def mad(a, b, sel=None):
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return float((d if sel is None else d[sel]).mean())


def psnr(a, b, sel=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    mse = float((d if sel is None else d[sel]).mean())
    return 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def latents_of(buf, b, h0, w0):
    """image b of an engine's [B * hw][8] latent buffer as the oracle's [4][h0][w0] fp32"""
    hw = h0 * w0
    return buf[b * hw:(b + 1) * hw, :4].float().cpu().reshape(h0, w0, 4).permute(2, 0, 1)


def post_stages(camera, decoded, mask=None, color_match=None, color_amount=256):
    """the engine's post stages on one frame, by the contracts: the colours of `camera` onto `decoded`, then `camera` kept where the mask says"""
    out = np.array(decoded, dtype=np.uint8)
    if color_match is not None:
        out = CM.color_match_numpy(camera, out, color_match, int(color_amount))
    if mask is not None:
        out = KM.blend_numpy(camera, out, mask)
    return out


# ------------------------------------------------------------------------------------------ the loop
@contextlib.contextmanager
def _draws_in_call_order(draws, first):
    """while inside: `torch.randn` hands out draws[first], draws[first + 1], ... (the scheduler's step draws its noise by that name)"""
    real, k = torch.randn, [first]

    def randn(*size, **kw):
        z = draws[k[0]]
        k[0] += 1
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        assert tuple(z.shape) == shape, (z.shape, shape)
        return z.clone().to(kw.get("dtype") or torch.float32)

    torch.randn = randn
    try:
        yield
    finally:
        torch.randn = real


def _embeds(text):
    if isinstance(text, (list, tuple)):
        mix = None
        for e, w in text:
            term = float(w) * e.reshape(-1, e.shape[-1]).float()
            mix = term if mix is None else mix + term
        return mix[None]
    return text.reshape(1, -1, text.shape[-1]).float()


@torch.no_grad()
def stage_frame(orc, img, text, height, width, strength, steps, controlnet_scale=1.0, use_controlnet=True, rng_seed=42, seed=None,
                edges="sobel", canny_thresholds=CANNY, mask=None, color_match=None, color_amount=256, mutant=None, other=None):
    """One frame by `orc` (an OraclePipeline: its weights, configurations and scheduler) with the stages above.  img, other: PIL RGB images;
    mask: u8 [height][width] or None; seed: None = the reference's own draws (a fresh generator per frame, whatever `rng_seed`).
    -> namespace(init_latents, noisy_latents, denoised [per step], decoded, before (u8 frame ahead of the post stages), frame (u8), wl, timesteps)"""
    assert mutant is None or (mutant in MUTANTS and mask is not None)
    sched = orc.sched
    img = center_crop_resize(img, width, height)
    camera = np.asarray(img.convert("RGB"), dtype=np.uint8)
    if edges == "canny":
        edge = Image.fromarray(CC.canny_numpy(camera, *canny_thresholds), mode="L")
    else:
        edge = sobel_edges(img, 0.11, 0.8)
    reset_rng(rng_seed)
    image = preprocess_image(img)
    control = preprocess_control(edge)
    ts = sched.set_timesteps(strength, steps, 50)
    n = len(ts)
    init = nets.taesd_encode(orc.w_vae, image)
    h0, w0 = init.shape[2:]
    # draw 0, one draw per scheduler step of a schedule of several, and one more that no stage uses (the `fresh` mutant's)
    if seed is None:
        draws = [torch.randn(init.shape, dtype=init.dtype) for _ in range(n + 2)]
    else:
        draws = [torch.from_numpy(SC.normal_draw(seed, 0, d, h0 * w0).reshape(1, 4, h0, w0)).to(init.dtype) for d in range(n + 2)]
    latents = sched.add_noise(init, draws[0], ts[:1])
    w_emb = None
    if orc.unet_cfg.cond_proj_dim:
        w_emb = w_embedding(torch.tensor(orc.guidance_scale).repeat(1), orc.unet_cfg.cond_proj_dim)
    text = _embeds(text)
    wl = anchor = None
    if mask is not None:
        wl = torch.from_numpy(KM.latent_numpy(np.asarray(mask)[None])).reshape(1, 1, h0, w0)
        anchor = init
        if mutant == "other_init":
            anchor = nets.taesd_encode(orc.w_vae, preprocess_image(center_crop_resize(other, width, height)))
    trace = SimpleNamespace(init_latents=init.clone(), noisy_latents=latents.clone(), denoised=[], wl=wl, timesteps=ts.tolist())
    denoised = None
    with _draws_in_call_order(draws, 1):
        for i, t in enumerate(ts):
            tt = torch.full((1,), int(t), dtype=torch.long)
            down = mid = None
            if use_controlnet:
                down, mid = nets.controlnet_forward(orc.w_cn, orc.cn_cfg, latents, tt, text, control, conditioning_scale=controlnet_scale,
                                                    guess_mode=True)
            eps = nets.unet_forward(orc.w_unet, orc.unet_cfg, latents, tt, text, w_emb, down, mid, None, ref=None)
            latents, denoised = sched.step(eps, i, t, latents)
            if mask is not None and i + 1 < n and mutant != "none":
                at = ts[i:i + 1] if mutant == "this_t" else ts[i + 1:i + 2]
                z = draws[{"fresh": n + 1, "draw1": 1}.get(mutant, 0)]
                latents = wl * latents + (1 - wl) * sched.add_noise(anchor, z, at)
            if mask is not None and i + 1 == n and mutant not in ("none", "no_final"):
                denoised = wl * denoised + (1 - wl) * anchor
            trace.denoised.append(denoised.clone())
    out = nets.taesd_decode(orc.w_vae, denoised)
    trace.decoded = out.clone()
    trace.before = postprocess(out)
    trace.frame = post_stages(camera, trace.before, mask, color_match, color_amount)
    return trace


# ------------------------------------------------------------------------------------------ an engine's frame against the oracle's
def frames_ahead_of_the_post_stages(eng, H, W):
    """Run the engine's `program_serial` call by call over the inputs of its last launch (they are still in place), as `walk()` of
    tests/test_keep_mask_gpu.py does -> (out_u8 right behind `postprocess_rgb`, out_u8 at the end), both u8 [B][H][W][3]"""
    before = None
    for fn, a, k in eng.program_serial.calls:
        fn(*a, **k)
        if fn.__name__ == "postprocess_rgb":
            eng.ops.synchronize()
            before = eng.out_u8.detach().cpu().numpy().reshape(-1, H, W, 3).copy()
    eng.ops.synchronize()
    assert before is not None
    return before, eng.out_u8.detach().cpu().numpy().reshape(-1, H, W, 3).copy()


def figures(eng, b, right, camera, before, frame, mask, color_match=None):
    """what is compared of frame b of an engine's last launch with `right`, its `stage_frame`: r0 of x0, r1 of the final denoised latents
    over all latent pixels and over the mixed ones (0 < wl < 1), mean LSB and PSNR over the restyled pixels (mask == 255) ahead of the
    post stages, and whether the final frame is the numpy post stages of the engine's own frame ahead of them, byte for byte"""
    h0, w0 = right.init_latents.shape[2:]
    den, ref = latents_of(eng.buffers["denoised"], b, h0, w0), right.denoised[-1][0]
    mixed = ((right.wl[0] > 0) & (right.wl[0] < 1)).expand(4, h0, w0)
    restyled = mask == 255
    return dict(r0=r1(latents_of(eng.buffers["x0"], b, h0, w0), right.init_latents[0]), r1=r1(den, ref),
                r1_mixed=r1(den, ref, mixed) if bool(mixed.any()) else 0.0, lsb=mad(before, right.before, restyled),
                psnr=psnr(before, right.before, restyled), post_exact=bool(np.array_equal(frame, post_stages(camera, before, mask, color_match))))

"""VideoSDPipeline — the reference's per-GPU worker class, re-hosted on the MI355X engine.

Mirrors /root/reference/diffusert/videopipeline.py:11-128: same constructor kwargs (`model`, `controlnet`
required, `device` optional, extras such as `gpus` / `compile` ignored), same `infer` signature and
defaults, same `load_model` / `compile_model` methods, so diffusert/server.py:104-117,317-321 can drive it
unchanged (`VideoSDPipeline.remote(**config)` and `await pipelines[gpu].infer.remote(img, **options)` are
provided by videosd_amd/dispatch.py without Ray).

What differs underneath: no diffusers / TensorRT / torch.compile; the frame goes through
videosd_amd.engine.Engine (libvsd.so HIP kernels replayed as one hipGraph).
"""
import gc
import inspect
import math
import os
import statistics
import time
import zlib
from collections import OrderedDict
from typing import Any, List, NamedTuple, Optional, Union

import numpy as np
import torch
from PIL import Image

from . import config as C
from . import checkpoints as CK
from . import promptmix as PM
from . import weights as W
from .blur import gauss_taps
from .engine import BLUR_SWITCHES
from .frames import I420Frame, is_i420
from .lcm import lcm_timesteps
from .lib import COLOR_MAX_AMOUNT, RESAMPLE_MAX_SIDE, check_color_amount, check_color_match, check_edges


def center_crop_resize(img: Image.Image, width: int, height: int) -> Image.Image:
    """Center crop to the target aspect ratio (float box) and LANCZOS-resize: videopipeline.py:92-107."""
    if img.width / img.height > width / height:
        new_width = img.height * (width / height)
        box = ((img.width - new_width) / 2, 0, (img.width + new_width) / 2, img.height)
    else:
        new_height = img.width * (height / width)
        box = (0, (img.height - new_height) / 2, img.width, (img.height + new_height) / 2)
    return img.crop(box).resize((width, height), resample=Image.Resampling.LANCZOS)


def _weights_dir() -> Optional[str]:
    d = os.environ.get("VSD_WEIGHTS")
    return d if d and os.path.isdir(d) else None


def _flat(name: str) -> Optional[str]:
    """`$VSD_WEIGHTS/<name>` (the flat layout), if it is there"""
    d = _weights_dir()
    return os.path.join(d, name) if d and os.path.exists(os.path.join(d, name)) else None


def _text_files(mdir: Optional[str], tower: str, tokenizer: str, flat_tokenizer: Optional[str] = None):
    """-> (checkpoint of a text tower or None, the directory of its vocabulary files): `<snapshot>/<tower>/model.safetensors` and
    `<snapshot>/<tokenizer>/`, else flat under `$VSD_WEIGHTS`: `<tower>.safetensors`, the vocabulary in `flat_tokenizer/` or beside it."""
    sub = os.path.join(mdir, tokenizer) if mdir else None
    return (CK.checkpoint_file(mdir, tower, stems=("model",)) or _flat(tower + ".safetensors"),
            sub if sub and os.path.isdir(sub) else (flat_tokenizer and _flat(flat_tokenizer)) or _weights_dir())


def load_or_synthesize(spec, prefix: str, filename: str, device, snapshot_file: Optional[str] = None):
    """-> (weights, source).  In this order: the safetensors file of a `from_pretrained` directory (`snapshot_file`, found by
    weights.checkpoint_file), `$VSD_WEIGHTS/<filename>` (flat layout), seeded synthetic tensors (no checkpoint exists offline).
    A file that lacks a tensor of the architecture, or holds it in another shape, is refused with the tensor's name."""
    path = snapshot_file or _flat(filename)
    if path is not None:
        w = CK.load_safetensors(path, device=device)
        CK.check_against_spec(w, spec, path if snapshot_file else filename)
        return w, path
    return W.synthesize(spec, prefix, device=device), "synthetic"


def _prompt_key(prompt):
    """what the prompt cache (and an SDXL plan) knows a prompt by: the string, the list as a tuple, the canonical form of a mix"""
    return PM.prompt_key(prompt)


class PlanKey(NamedTuple):
    """What a captured program depends on, and so what the plan cache is keyed by (`VideoSDPipeline._plan_key` builds it).  `strength` and
    `controlnet_scale` are not in it: they only change constants the graph reads from device memory (Engine.update_options), so a slider
    drag in the client (server.py:163-197) does not rebuild or re-capture anything -- only the NUMBER of timesteps they give is."""
    height: int
    width: int
    steps: int
    n_eff: int                   # timesteps of (strength, steps): the program's length
    use_cn: bool
    use_ref: bool
    prompt: Any = None           # SDXL: the pooled text embedding is baked into the time embeddings at `prepare`, so the prompt is part of the program
    device_seed: bool = False    # the three modes of Engine.prepare
    frame_prompts: bool = False
    frame_options: bool = False  # (the EFFECTIVE switch: SDXL and reference-only programs keep one pair of options per plan)


class Launch(NamedTuple):
    """The handle `submit_batch` returns and `collect_batch` takes; the pipeline keeps those not yet collected, oldest first."""
    engine: Any
    frames: int
    lane: int
    yuv: Optional[List[bool]]  # which results go back as I420 (None: none of them) ...
    on_device: bool            # ... and whether the device converts them
    keep: tuple                # the prompt blocks and option entries of the launch: their installs may not have executed yet


class _Plan:
    """One cached program: `root` owns the schedule constants, `engines` maps (frames per launch, lane) to the root and its slots, `opts` is
    the (strength, controlnet_scale) those constants hold (None with `frame_options`: every frame slot of every engine has its own)."""

    def __init__(self, root, opts):
        self.root, self.opts, self.engines = root, opts, {}

    def busy(self, in_flight) -> bool:
        return any(h.engine is e for e in self.engines.values() for h in in_flight)

    def destroy(self) -> int:
        """release the graphs of every engine -> how many there were"""
        for e in self.engines.values():
            e._destroy_graphs()
        return len(self.engines)


class VideoSDPipeline:
    """One instance = one GPU = one full weight replica (the reference's Ray actor with num_gpus=1)."""

    def __init__(self, *args, **kwargs):
        self._init_state(kwargs)
        try:
            self.load_model(kwargs["model"], kwargs["controlnet"])
        except KeyError:
            print("Model name and controlnet model must be specified")  # videopipeline.py:24-26
            raise
        self.frame_options = self.frame_options and not self.is_xl  # (SDXL programs keep the default form)

    def _init_state(self, kwargs):
        """Every attribute the object ever has, from the constructor kwargs alone: touches neither the GPU nor the library.  The switches
        are extensions of the reference's surface, all off by default:
        honor_controlnet_flag / honor_ref_flag: `controlnet` / `ref` of `infer` are obeyed, not accepted and ignored (videopipeline.py:84-85);
            `ref=True` then runs the reference-only mode (lcm_reference_pipeline.py, dead code at the reference's v2).
        device_resize (a server should turn it on): the centre crop + LANCZOS resize in front of every frame
            (videopipeline.py:92-107) runs on the GPU instead of in PIL on this host thread -- the same bytes (csrc/resample.hip).  RGB frames
            whose target size is a multiple of 8 take it; everything else keeps the host path.
        device_seed: `seed` changes the picture: the noise of every frame is drawn on the device from ITS seed (include/vsd.h THE NOISE
            CONTRACT), one seed per frame.  Off: the reference's CPU-contract draws, the same for every frame and seed.
        frame_prompts: every frame of a launch has a prompt of its own (`prompts`, one per frame); the program then reads K / V^T per frame
            and runs every cross-attention in the explicit form.  Off: one prompt per launch, the absorbed form at the wide levels.
        frame_options: every frame of a launch has a `strength` and a `controlnet_scale` of its own (a number, or a sequence of one per frame);
            the program then reads the scheduler coefficients, time tables and ControlNet scales per frame, and a changed option rewrites a
            frame slot ahead of the launch, so nothing is drained.  Off: one pair per plan (`Engine.update_options`).  SDXL and
            reference-only programs keep the default form either way.
        The last three are modes of `Engine.prepare`; a worker coalesces frames that differ in what they make per-frame (`per_frame_*`).
        edges="canny", canny_thresholds=(100, 200): the ControlNet is conditioned on real Canny edges, computed on the device by THE EDGE
            CONTRACT of include/vsd.h (gray value, 3 x 3 Sobel, |dx| + |dy|, non-maximum suppression, hysteresis: binary and one pixel wide,
            what control_v11p_sd15_canny was trained on).  The thresholds are integers on |dx| + |dy|, 0 <= low <= high <= 2040 (floats are
            floored).  The arithmetic is the one OpenCV documents for Canny(aperture 3, L1 norm); equality with cv2's bytes is not measured.
            Default edges="sobel": the reference's stand-in (canny_gpu.py:27-44), the same programs and bits as before.  Fixed for the life
            of the object; composes with every switch above; such a pipeline has no `export_plan`.  SDXL has no ControlNet tower: there
            the switch is accepted and inert.
        color_match="histogram" | "meanstd", color_amount=1.0: the colours of every input frame (after crop / resize / I420 conversion: what
            the model sees) are transferred onto its output frame on the device, inside the captured program, by THE COLOUR CONTRACT of
            include/vsd.h -- per channel, by histogram matching or by mean and standard deviation -- and blended with the unmatched
            output by `color_amount` in [0, 1]: the cure video tools call colour coherence, against TAESD's desaturation and the
            frame-to-frame colour flicker of a few-step LCM.  Default None: no such stage, the same programs and bits as before.  The mode
            is fixed for the life of the object; `set_color_match(amount)` changes the amount live (no re-capture; a worker collects its launches in flight first).  Composes with every
            switch above, with I420 frames, reference-only mode and SDXL; such a pipeline has no `export_plan`.
        keep_mask=True: part of every frame is kept as the camera saw it, by THE KEEP MASK of include/vsd.h: `set_mask(mask)` (255 / white:
            restyled, 0 / black: kept, values between blend; everything restyled until then) holds for every launch submitted from then
            on, `infer_batch(imgs, masks=[...])` takes one mask per frame.  Inside the captured program the kept region of the latents is
            the input's own, noised to the step's timestep, at every denoising step -- the model sees what surrounds the part it paints --
            and the camera's pixels are blended over the output behind the decoder, so PIL, numpy and I420 callers all get the blended
            frame.  Default False: no such stages, the same programs and bits as before.  Fixed for the life of the object; a new mask is
            one copy ahead of the next launch, no re-capture.  Composes with every switch above and with I420 frames; not with SDXL or
            reference-only frames (refused by name); such a pipeline has no `export_plan` / `export_prompt`.
        edge_blur=SIGMA: a Gaussian blur of that sigma (0..10; THE BLUR CONTRACT of include/vsd.h, `videosd_amd.blur.gauss_taps`) ahead of the
            edge op, inside the captured program: the ControlNet's edges are taken from a calmed copy of the frame, so sensor noise no
            longer makes one-pixel `edges="canny"` lines appear and vanish from frame to frame (what OpenCV recipes do with `GaussianBlur`
            ahead of `Canny`); the encoder, colour match and mask blend keep reading the camera's own frame.  Applies to either `edges`
            mode; without a ControlNet tower (SDXL) it is accepted and inert.  Default None: no such stage, the same programs and bits.
            `set_edge_blur(sigma)` changes it live (136 bytes ahead of an engine's next launch, no re-capture; 0: no blur).
        mask_feather=SIGMA (needs keep_mask=True): the same blur over the keep masks ahead of both mask stages -- the "mask blur" slider of
            inpainting UIs, so a hard-edged mask drawn or segmented on a client leaves no seam.  An all-255 mask stays all-255.
            `set_mask_feather(sigma)` changes it live.  Neither switch has `export_plan` / `export_prompt`.
        lanes: launch lanes this instance may keep in flight (`submit_batch(lane=...)`, the worker loop of dispatch.py): lane l runs on launch
            stream l (ops.HipOps); with at most two lanes every lane also has a stream for its side branch.
        tuning_mode: "auto": shapes missing from the table are timed on this GPU at `prepare`; "table": never -- they take the deterministic
            heuristic (ops.choose_tile), so that every rank of a group builds the SAME kernels and a frame's bits do not depend on the rank
            it lands on (dispatch.spawn_workers sets this for groups; `sync_tuning` spreads rank 0's measured choices).
        Per-session state without stalls (server.py:90-93: options live on each VideoSDTrack; :132-137: every session's frames go through
        the same actors) is two LRU caches.  `_prompts`: prompt key -> PromptBlock (cross-attention K / V^T + absorbed weights of every
        layer, ~40 MB, built on the GPU in ~1 ms); an engine takes a cached prompt with one device-to-device copy on its own stream.
        `_plans`: PlanKey -> _Plan, each with its own schedule constants, so sessions with different sizes / steps alternate frame by frame
        with their graphs intact; `max_plans` counts PROGRAMS.  Every engine owns its activation arena (1-6 GB at 512x512, one to five
        frames per launch): `memory_budget` (fraction of the device's memory) bounds what the cache may hold (`_trim_memory`)."""
        self._kwargs = dict(kwargs)
        self.device = kwargs.get("device", 0)
        for switch in ("honor_controlnet_flag", "honor_ref_flag", "device_resize", "device_seed", "frame_prompts", "frame_options"):
            setattr(self, switch, bool(kwargs.get(switch, False)))
        self.edges, self.canny_thresholds = check_edges(kwargs.get("edges", "sobel"), kwargs.get("canny_thresholds", (100, 200)))
        self.color_match, self._color_a = check_color_match(kwargs.get("color_match"), kwargs.get("color_amount", 1.0))
        self.keep_mask = bool(kwargs.get("keep_mask", False))
        self._mask_img, self._mask_epoch, self._mask_sized = None, 0, {}  # `set_mask`: the mask as an "L" image, its count, (width, height) -> u8 [h][w]
        self._blur = {k: self._check_sigma(k, kwargs[k]) for k in BLUR_SWITCHES if kwargs.get(k) is not None}  # switch -> sigma (`set_edge_blur`, `set_mask_feather`)
        if "mask_feather" in self._blur and not self.keep_mask:
            raise ValueError("mask_feather needs keep_mask=True: it feathers the keep masks, and this pipeline has none")
        self._loras = self._check_loras(kwargs.get("loras"))  # [(name, path, scale)]: loaded by `load_model`, fused on the device
        self.lora_skip_text_encoder = bool(kwargs.get("lora_skip_text_encoder", False))
        self._lora_scales, self.lora_text_encoder_keys_skipped = OrderedDict((n, s) for n, _p, s in self._loras), 0
        self.max_lanes = max(1, int(kwargs.get("lanes", 2)))
        self.tuning_mode = str(kwargs.get("tuning_mode", "auto"))
        self.max_prompts = int(kwargs.get("max_prompts", 8))
        self.max_plans = int(kwargs.get("max_plans", 3))
        self.memory_budget = float(kwargs.get("memory_budget", 0.6))
        self.is_xl, self.unet_cfg, self.model, self.text_encoder, self.weight_sources, self._xl_prompts = False, C.SD15_UNET, None, None, {}, {}  # (`load_model`)
        self._ref_img, self._ref_epoch = None, 0
        self._prompts, self._plans, self.evictions = OrderedDict(), OrderedDict(), 0
        self.prompt_builds = 0  # `Engine.build_prompt` calls of the prompt cache (a mix of cached prompts causes none)
        self._in_flight: List[Launch] = []  # submitted, not yet collected
        self._host_ms = {k: [] for k in ("crop_resize", "upload_enqueue", "wait_download", "to_pil", "to_i420", "gpu", "prepare", "update_options", "prompt")}
        self._io_bytes = {"up": None, "down": None}  # per frame of the last launch submitted / collected

    per_frame_seed = property(lambda self: self.device_seed, doc="may a worker coalesce frames that differ in `seed`? (read by dispatch.py)")
    per_frame_prompt = property(lambda self: self.frame_prompts, doc="... in `prompt`?")
    per_frame_options = property(lambda self: self.frame_options, doc="... in `strength` / `controlnet_scale`, within one `option_class`?")

    # ------------------------------------------------------------------ model loading
    def load_model(self, model_name, controlnet_model="lllyasviel/control_v11p_sd15_canny"):
        """videopipeline.py:49-72.  Like the reference, `model_name` is accepted but the UNet is always the
        LCM-distilled SD1.5 UNet (the reference hard-codes SimianLuo/LCM_Dreamshaper_v7), the VAE is TAESD and
        the ControlNet is SD1.5-canny."""
        from .engine import Engine
        from .ops import HipOps  # raises without a ROCm GPU / libvsd.so: there is no CPU path

        ops = HipOps(int(self.device))
        dev = ops.device
        # per-shape kernel configurations found on an MI355X (shapes not in the table are timed at `prepare`)
        ops.load_tuning(os.environ.get("VSD_TUNING") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tuning_mi355x.json"))
        # Extension (BASELINE.json configs[3]; the reference only knows SD1.5): a model name containing "xl" selects the
        # SDXL-base UNet topology (LCM-SDXL weights as `unet_sdxl.safetensors`, TAESD-XL as `taesdxl.safetensors`),
        # without a ControlNet tower; prompts then need 2048-wide embeddings + a 1280-wide pooled vector.
        self.is_xl = "xl" in str(model_name).lower()
        self.unet_cfg = C.SDXL_UNET if self.is_xl else C.SD15_UNET
        # What `from_pretrained` reads (videopipeline.py:51-69), offline: `model` / `controlnet` given as DIRECTORIES in the
        # Hugging Face snapshot layout -- <model>/unet/diffusion_pytorch_model.safetensors, <model>/text_encoder/model.safetensors,
        # <model>/tokenizer/{vocab.json, merges.txt}; the ControlNet's and TAESD's diffusion_pytorch_model.safetensors at the top
        # level of theirs -- or hub ids with a snapshot in the local HF cache; fp32 or fp16 tensors, cast to fp16 like
        # torch_dtype=float16.  Then the flat $VSD_WEIGHTS/*.safetensors files, then seeded synthetic tensors.  Like the
        # reference, a hub id that is not SimianLuo/LCM_Dreamshaper_v7 still gets that UNet (it hard-codes the id, :57); the VAE is
        # `madebyollin/taesd` (:68) unless the extension kwarg `vae=` names another directory.
        mdir = CK.find_snapshot(model_name) or (None if self.is_xl else CK.find_snapshot("SimianLuo/LCM_Dreamshaper_v7"))
        vdir = CK.find_snapshot(self._kwargs.get("vae") or ("madebyollin/taesdxl" if self.is_xl else "madebyollin/taesd"))
        if self.is_xl and self._loras:
            raise ValueError("loras=[...] with an SDXL model: adapters are read against the SD1.5 UNet only (SDXL is out of scope)")
        if self.is_xl:
            wu, self.weight_sources["unet"] = load_or_synthesize(W.unet_spec(C.SDXL_UNET), "sdxl.", "unet_sdxl.safetensors", dev, CK.checkpoint_file(mdir, "unet"))
            wv, self.weight_sources["vae"] = load_or_synthesize(W.taesd_spec(C.TAESD), "vae.", "taesdxl.safetensors", dev, CK.checkpoint_file(vdir))
            self.model = Engine(ops, C.SDXL_UNET, None, C.TAESD, wu, None, wv)
            # the two text towers of an SDXL snapshot (<model>/text_encoder, <model>/text_encoder_2, tokenizer, tokenizer_2;
            # flat: $VSD_WEIGHTS/text_encoder.safetensors + text_encoder_2.safetensors, vocabulary files in $VSD_WEIGHTS[/tokenizer_2])
            (f1, tok1), (f2, tok2) = _text_files(mdir, "text_encoder", "tokenizer"), _text_files(mdir, "text_encoder_2", "tokenizer_2", "tokenizer_2")
            self.weight_sources.update({k: f or "stand-in embeddings seeded by the prompt text" for k, f in (("text_encoder", f1), ("text_encoder_2", f2))})
            if f1 is not None and f2 is not None:
                from . import clip as K

                towers = []
                for f, cfg, tok in ((f1, K.SDXL_CLIP_L, tok1), (f2, K.SDXL_CLIP_G, tok2)):
                    wt = CK.load_safetensors(f, device=dev)
                    CK.check_against_spec(wt, K.text_tower_spec(cfg), f)
                    towers.append(K.ClipTextEncoder(ops, cfg, wt, tokenizer_dir=tok))
                self.text_encoder = K.SdxlTextEncoders(*towers)
            return self.model
        cdir = CK.find_snapshot(controlnet_model)
        wu, self.weight_sources["unet"] = load_or_synthesize(W.unet_spec(C.SD15_UNET), "unet.", "unet.safetensors", dev, CK.checkpoint_file(mdir, "unet"))
        wc, self.weight_sources["controlnet"] = load_or_synthesize(W.controlnet_spec(C.SD15_CONTROLNET), "cn.", "controlnet.safetensors", dev, CK.checkpoint_file(cdir))
        wv, self.weight_sources["vae"] = load_or_synthesize(W.taesd_spec(C.TAESD), "vae.", "taesd.safetensors", dev, CK.checkpoint_file(vdir))
        self.model = Engine(ops, C.SD15_UNET, C.SD15_CONTROLNET, C.TAESD, wu, wc, wv)
        self._load_loras(wu)
        clip_file, tok_dir = _text_files(mdir, "text_encoder", "tokenizer")
        self.weight_sources["text_encoder"] = clip_file or "stand-in embeddings seeded by the prompt text"
        if clip_file is not None:
            from .clip import ClipTextEncoder

            wt = CK.load_safetensors(clip_file, device=dev)
            CK.check_against_spec(wt, W.clip_spec(C.CLIP_L), clip_file)
            self.text_encoder = ClipTextEncoder(ops, C.CLIP_L, wt, tokenizer_dir=tok_dir)
        return self.model

    def compile_model(self):
        """videopipeline.py:35-47: build the replayable graph and run the 768x768 warm-up frame."""
        return self.infer(Image.new("RGB", (768, 768)), prompt="warmup", height=768, width=768, strength=0.8, steps=4)

    # ------------------------------------------------------------------ prompt
    def encode_prompt(self, prompt: Union[str, List[str]]) -> torch.Tensor:
        """[77, 768] fp16 embeddings.  With CLIP weights + tokenizer files under $VSD_WEIGHTS the HIP CLIP encoder
        runs; otherwise (no vocabulary offline) a deterministic stand-in seeded by the prompt text is used."""
        text = self._one_prompt(prompt)
        if self.text_encoder is not None and self.text_encoder.has_tokenizer:
            return self._xl_encode(text)[0] if self.is_xl else self.text_encoder.encode(text)
        g = torch.Generator().manual_seed(zlib.crc32(text.encode()))
        return (torch.randn(77, self.unet_cfg.cross_dim, generator=g) * 0.5).half()

    @staticmethod
    def _one_prompt(prompt: Union[str, List[str]]) -> str:
        """The ONE prompt of a frame.  The reference hands a list to the tokenizer as a BATCH: `batch_size = len(prompt)`
        (lcm_controlnet.py:433-438), i.e. a two-element list asks for two images from one input frame -- which its own
        `infer` cannot return (videopipeline.py:126-128 takes `.images[0]`) and `prepare_latents` cannot build from a single
        encoded frame without duplicating it.  Every call site of the reference passes a string or the one-element default
        `["pixar, cg"]` (videopipeline.py:77; server.py:166-171 sets a string): that is what is supported here, and anything
        else is refused instead of silently meaning something different (rounds 1-4 joined the elements with spaces)."""
        if isinstance(prompt, str):
            return prompt
        items = list(prompt)
        if len(items) != 1 or not isinstance(items[0], str):
            raise ValueError(f"prompt must be a string or a one-element list of strings, got {len(items)} element(s): the reference treats "
                             "a list as a batch of prompts (batch_size = len(prompt), lcm_controlnet.py:433-438), which this per-frame "
                             "path (one image in, one image out, videopipeline.py:126-128) does not have")
        return items[0]

    def _xl_encode(self, text: str):
        """SDXL: (prompt_embeds [77, 2048], pooled_prompt_embeds [1280]) of both text towers, once per prompt text (the pooled
        vector is asked for separately, per engine: keep the last few pairs)."""
        hit = self._xl_prompts.get(text)
        if hit is None:
            hit = self._xl_prompts[text] = self.text_encoder.encode(text)
            while len(self._xl_prompts) > 8:
                self._xl_prompts.pop(next(iter(self._xl_prompts)))
        return hit

    def encode_pooled(self, prompt: Union[str, List[str]]) -> torch.Tensor:
        """SDXL only: the pooled text embedding [1280] = the second tower's `text_embeds` (with both towers' checkpoints and
        tokenizer files present; otherwise a stand-in seeded by the prompt text, like `encode_prompt`)."""
        text = self._one_prompt(prompt)
        if self.text_encoder is not None and self.text_encoder.has_tokenizer:
            return self._xl_encode(text)[1]
        g = torch.Generator().manual_seed(zlib.crc32(("pooled:" + text).encode()))
        return (torch.randn(self.unet_cfg.add_pooled_dim, generator=g) * 0.5).half()

    @property
    def prompt_shape(self):
        """Shape of the embeddings `set_prompt_embeds` takes (what the RCCL broadcast of dispatch.py carries)."""
        return (77, self.unet_cfg.cross_dim)

    def set_prompt_embeds(self, embeds: torch.Tensor, key=None):
        """Install embeddings produced elsewhere (rank 0 broadcasts them over RCCL, dispatch.py) as prompt `key`: they join
        the prompt cache; nothing in flight is disturbed."""
        return self._cache_prompt(key, embeds)

    def _prompts_in_use(self):
        """ids of the cache entries a launch in flight on a `frame_prompts` engine reads (its installs may not have executed yet)"""
        srcs = [b for h in self._in_flight for b in (h.engine._prompt_slots.src if h.engine._prompt_slots is not None else ()) if b is not None]
        return {id(c) for b in srcs for c in getattr(b, "components", (b,))}  # (a slot that holds a mix reads the mix's components)

    def _cache_prompt(self, key, embeds=None, prompt=None, keep=()):
        """The block of prompt `key`, built from `embeds` or from the text `prompt` when the cache lacks it (or holds other embeddings).  Over
        `max_prompts` the least recently used entries go -- never `key`, never one of the launch being put together (`keep`), never one a
        launch in flight reads: the cache then grows.  An engine that still holds an evicted block keeps it alive until it switches."""
        blk = self._prompts.get(key)
        if blk is not None and embeds is not None and blk.text is not None:
            # the same embeddings for a key this worker already holds (a repeated sync, a dispatcher that lost track of what the
            # workers know): keep the block -- rebuilding it is 23 K / V GEMMs + 16 folds + a synchronise, and every engine
            # would re-copy its 40 MB at its next launch
            e = embeds.reshape(-1, embeds.shape[-1]).to(device=blk.text.device, dtype=torch.float16)
            if e.shape == blk.text.shape and bool(torch.equal(e, blk.text)):
                embeds = None
        if blk is None or embeds is not None:
            t0 = time.perf_counter()
            blk = self.model.build_prompt(embeds if embeds is not None else self.encode_prompt(prompt))
            self._prompts[key] = blk
            self.prompt_builds += 1
            self._note("prompt", t0)
            if len(self._prompts) > max(1, self.max_prompts):
                busy = self._prompts_in_use()
                for k in [k for k, b in self._prompts.items() if k != key and k not in keep and id(b) not in busy]:
                    if len(self._prompts) <= max(1, self.max_prompts):
                        break
                    del self._prompts[k]
        self._prompts.move_to_end(key)
        return blk

    def set_reference(self, img):
        """The reference image of the reference-only mode (`honor_ref_flag=True`, `infer(..., ref=True)`).  Without one the
        first frame seen with `ref=True` becomes the reference."""
        self._require_idle("change the reference image")
        self._ref_img = img
        self._ref_epoch += 1

    def set_color_match(self, amount: float) -> float:
        """The colour-match amount, a number in [0, 1], of every launch submitted from now on (`color_match=` of the constructor chose
        the mode).  Every cached engine takes it on its own stream ahead of its next launch (`Engine.set_color_amount`): no
        re-capture, and launches in flight keep the amount they were submitted with.  Called on this object nothing waits; through a
        worker (`VideoSDPipeline.remote(...).set_color_match`) the call runs alone like every method but `infer`, so the worker first
        collects the launches it has in flight."""
        if self.color_match is None:
            raise ValueError('set_color_match needs a pipeline built with color_match="histogram" or "meanstd"')
        self._color_a = check_color_amount(amount)
        return self.color_amount

    @staticmethod
    def _mask_image(mask) -> Image.Image:
        """a mask as callers give it -- a PIL "L" / "1" image or a 2-D u8 array, of any size -- as an "L" image"""
        if isinstance(mask, Image.Image):
            if mask.mode not in ("L", "1"):
                raise ValueError(f'a mask image must have mode "L" or "1" (255 / white: restyled, 0 / black: kept), not "{mask.mode}"')
            img = mask.convert("L")
        else:
            m = np.asarray(mask)
            if m.ndim != 2 or m.dtype != np.uint8:
                raise ValueError(f"a mask must be a PIL L / 1 image or a 2-D u8 array, not {type(mask).__name__} of shape {getattr(m, 'shape', None)}, {getattr(m, 'dtype', None)}")
            img = Image.fromarray(np.ascontiguousarray(m), mode="L")
        if min(img.size) < 1:
            raise ValueError("a mask must have at least one pixel")
        return img

    @staticmethod
    def _size_mask(img: Image.Image, width: int, height: int) -> np.ndarray:
        """the mask at the size of a launch's frames, by the rule that sizes a frame (`_launch_frames`): the centre crop + LANCZOS resize of
        `center_crop_resize`, then, for a size that is not a multiple of 8, the second LANCZOS step down to one -- so a mask drawn over the
        camera picture lines up with the camera's frames"""
        out = center_crop_resize(img, width, height)
        if height % 8 or width % 8:
            out = out.resize((width - width % 8, height - height % 8), resample=Image.Resampling.LANCZOS)
        return np.array(out, dtype=np.uint8)

    def set_mask(self, mask) -> int:
        """The keep mask of every launch submitted from now on (`keep_mask=True` of the constructor): a PIL "L" / "1" image or a 2-D u8 array
        of ANY size -- 255 / white: restyled, 0 / black: kept as the camera saw it -- or None: everything restyled.  For each frame size in
        use it is cropped and resized ONCE on the host, as a frame of that size is, and every cached engine takes it on its own stream
        ahead of its next launch (`Engine.set_masks`): no re-capture, and launches in flight keep the mask they were submitted with.
        Through a worker (`VideoSDPipeline.remote(...).set_mask`) the call runs alone like every method but `infer`.  -> how many masks
        this object has been given."""
        if not self.keep_mask:
            raise ValueError("set_mask needs a pipeline built with keep_mask=True")
        self._mask_img = None if mask is None else self._mask_image(mask)
        self._mask_sized = {}
        self._mask_epoch += 1
        return self._mask_epoch

    def _launch_masks(self, masks, n: int, width: int, height: int):
        """-> what `_install` gives the engine: None without `keep_mask`; one u8 [h][w] array per frame for `masks=[...]`; else the
        (epoch, array or None) of `set_mask` at this frame size (sized once per size and mask)"""
        if masks is not None:
            if not self.keep_mask:
                raise ValueError("masks= (one keep mask per frame) needs a pipeline built with keep_mask=True")
            masks = list(masks)
            if len(masks) != n:
                raise ValueError(f"masks must hold one mask per frame: {len(masks)} mask(s) for {n} frame(s)")
            return [np.full((height - height % 8, width - width % 8), 255, np.uint8) if m is None else self._size_mask(self._mask_image(m), width, height)
                    for m in masks]
        if not self.keep_mask:
            return None
        if self._mask_img is None:
            return (self._mask_epoch, None)
        if (width, height) not in self._mask_sized:
            self._mask_sized[(width, height)] = self._size_mask(self._mask_img, width, height)
        return (self._mask_epoch, self._mask_sized[(width, height)])

    @staticmethod
    def _check_sigma(switch: str, sigma) -> float:
        try:
            gauss_taps(sigma)
        except ValueError as e:
            raise ValueError(f"{switch}: {e}") from None
        return float(sigma)

    def _set_blur(self, switch: str, sigma) -> float:
        if switch not in self._blur:
            raise ValueError(f"set_{switch} needs a pipeline built with {switch}=<sigma> (0 for none yet)")
        self._blur[switch] = self._check_sigma(switch, sigma)
        return self._blur[switch]

    def set_edge_blur(self, sigma: float) -> float:
        """The sigma, in [0, 10] (0: no blur), of the blur ahead of the edge op for every launch submitted from now on (`edge_blur=` of the
        constructor switched the stage on).  Every cached engine takes the new tap table on its own stream ahead of its next launch
        (`Engine.set_edge_blur`): no re-capture, and launches in flight keep the table they were submitted with.  Through a worker
        (`VideoSDPipeline.remote(...).set_edge_blur`) the call runs alone like every method but `infer`.  -> the sigma."""
        return self._set_blur("edge_blur", sigma)

    def set_mask_feather(self, sigma: float) -> float:
        """the same for the blur of the keep masks (`mask_feather=` of the constructor)"""
        return self._set_blur("mask_feather", sigma)

    color_amount = property(lambda self: self._color_a / COLOR_MAX_AMOUNT, doc="the colour-match amount in [0, 1], as the contract rounds it")

    # ------------------------------------------------------------------ LoRA adapters (include/vsd.h THE ADAPTER FUSE)
    @staticmethod
    def _check_loras(loras):
        """`loras=` of the constructor (also a config.yaml key): up to four {"path": p, "scale": 0.8, "name": "ink"} -> [(name, path, scale)]"""
        from .lora import MAX_ADAPTERS

        out = []
        for i, d in enumerate(loras or ()):
            if not isinstance(d, dict) or "path" not in d or set(d) - {"path", "scale", "name"}:
                raise ValueError(f'loras[{i}] must be {{"path": ..., "scale": ..., "name": ...}} (scale and name optional), not {d!r}')
            scale = float(d.get("scale", 1.0))
            if not math.isfinite(scale):
                raise ValueError(f"loras[{i}]: scale must be a finite number, not {d.get('scale')!r}")
            out.append((str(d.get("name") or os.path.splitext(os.path.basename(str(d["path"])))[0]), str(d["path"]), scale))
        if len(out) > MAX_ADAPTERS:
            raise ValueError(f"loras: {len(out)} adapters, at most {MAX_ADAPTERS} can be loaded at once")
        if len({n for n, _p, _s in out}) != len(out):
            raise ValueError(f"loras: the adapters' names must differ, got {[n for n, _p, _s in out]}")
        return out

    def _load_loras(self, w_unet):
        """`load_model`: read the adapter files against the UNet's own tensor names, keep base copies of the tensors they touch, and fuse
        once at the constructor's scales.  Without `loras` nothing is read, kept or launched."""
        if not self._loras:
            return
        from .lora import load_adapter

        spec = W.unet_spec(self.unet_cfg)
        ads = [load_adapter(p, spec, skip_text_encoder=self.lora_skip_text_encoder, name=n) for n, p, _s in self._loras]
        self.lora_text_encoder_keys_skipped = sum(a.text_encoder_keys_skipped for a in ads)
        self.model.load_adapters(ads, w_unet)
        self.model.set_adapter_scales(list(self._lora_scales.values()))

    def set_lora_scales(self, scales) -> dict:
        """{name: scale} for some or all of the loaded adapters: "how much of this style", live.  ONE launch recomputes every adapted
        weight from its base copy in place (`Engine.set_adapter_scales`): nothing is re-captured, the plan cache survives, cached prompts
        are rebuilt from their embeddings before their next use.  The weights are shared by every lane, so no launch may be in flight;
        through a worker the call runs alone, after the launches in flight have been collected."""
        if not self._lora_scales:
            raise ValueError("set_lora_scale needs a pipeline built with loras=[...]")
        new = OrderedDict(self._lora_scales)
        for name, value in dict(scales).items():
            if name not in new:
                raise ValueError(f"no adapter named {name!r}: the loaded adapters are {list(new)}")
            value = float(value)
            if not math.isfinite(value):
                raise ValueError(f"the scale of {name!r} must be a finite number, not {value!r}")
            new[name] = value
        self._require_idle("change a LoRA scale")
        if self.model is not None and new != self._lora_scales:
            self.model.set_adapter_scales(list(new.values()))
        self._lora_scales = new
        return dict(new)

    def set_lora_scale(self, name: str, value: float) -> dict:
        return self.set_lora_scales({name: value})

    lora_scales = property(lambda self: dict(self._lora_scales), doc="{name: scale} of the loaded adapters")

    def option_class(self, options) -> int:
        """What two requests must share to run in ONE launch of a `frame_options` pipeline although their `strength` / `controlnet_scale`
        differ: the NUMBER of timesteps of (strength, steps) -- the program's length (`options`: the kwargs of an `infer` call)."""
        return len(lcm_timesteps(float(options.get("strength", INFER_DEFAULTS["strength"])), int(options.get("steps", INFER_DEFAULTS["steps"]))))

    @staticmethod
    def _per_frame(value, n: int, name: str):
        """`strength` / `controlnet_scale` of a launch of n frames -> n floats: a number for every frame, or a sequence of one per frame"""
        if isinstance(value, (int, float, np.integer, np.floating)):
            return [float(value)] * n
        vals = [float(v) for v in value]
        if len(vals) != n:
            raise ValueError(f"{name} must be a number or a sequence of one per frame: {len(vals)} value(s) for {n} frame(s)")
        return vals

    def can_batch(self, **options) -> bool:
        """May the worker coalesce queued frames with these options into one launch?  (reference-only frames go alone)"""
        return not (self.honor_ref_flag and options.get("ref", False))

    def _require_idle(self, what: str):
        """Prompt constants (cross-attention K / V^T) and plans are shared by every lane: rewriting them under a launch
        that is still running would hand that launch's caller another plan's frame."""
        if self._in_flight:
            raise RuntimeError(f"cannot {what} while {len(self._in_flight)} launch(es) are in flight: collect them first")

    def _note(self, what: str, t0: float):
        v = self._host_ms[what]
        v.append((time.perf_counter() - t0) * 1e3)
        if len(v) > 256:
            del v[:128]

    def metrics(self):
        """Per-stage host / device milliseconds of this worker (medians over the last frames): where a frame's time goes
        between `infer` entry and the PIL image (per-stage ms per GPU)."""
        out = {k: (round(statistics.median(v), 3) if v else None) for k, v in self._host_ms.items()}
        out["plans_cached"] = len(self._engines)
        out["programs_cached"] = len(self._plans)
        out["prompts_cached"] = len(self._prompts)
        out["prompt_builds"] = self.prompt_builds
        out["engines_evicted_for_memory"] = self.evictions
        if self._loras:
            out["lora_text_encoder_keys_skipped"] = self.lora_text_encoder_keys_skipped
        free, total = torch.cuda.mem_get_info(int(self.device))  # what a leak across plan / prompt changes would show in
        return {"stage_ms_p50": out, "io_bytes_per_frame": dict(self._io_bytes), "device_free_mb": free >> 20, "device_total_mb": total >> 20,
                "allocated_mb": torch.cuda.memory_allocated(int(self.device)) >> 20}

    def stage_profile(self, batch: int = 1):
        """Per-kernel-family device ms of ONE eager pass of the current plan (vsd_stage_times; the captured graph cannot be
        bracketed per launch).  On demand only: it re-runs the program un-captured."""
        self._require_idle("profile")
        if not self._plans:
            raise RuntimeError("no plan prepared yet: call infer first")
        eng = next(reversed(self._plans.values())).root  # the most recently used program
        ops = eng.ops
        eng.program.run()
        ops.synchronize()
        ops.profile_begin()
        eng.program.run()
        ops.synchronize()
        return {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ops.profile_end().items()}

    # ------------------------------------------------------------------ per frame
    def infer(
        self,
        img,
        prompt=["pixar, cg"],
        height=360,
        width=640,
        strength=0.4,
        steps=20,
        guidance_scale=7.5,
        ref=False,
        style_fidelity=0.0,
        controlnet=False,
        seed=42,
        controlnet_scale=1,
    ):
        """Same contract as videopipeline.py:75-128.  `guidance_scale`, `ref`, `style_fidelity` and
        `controlnet` are accepted and ignored exactly like the reference (ControlNet always runs; 7.5 is baked
        in); `seed` does not change the result because the reference resets the CPU generator state per frame -- unless the
        object was built with `device_seed=True`: then the frame's noise is a function of `seed` (include/vsd.h).
        `prompt`: a string or a one-element list as in the reference, or a weighted mix of up to four texts as JSON-able data,
        `{"mix": [["text a", 0.3], ["text b", 0.7]]}` (promptmix.py has the rules): the engine blends the CACHED constants of the texts on the
        device in one small launch (include/vsd.h THE PROMPT MIX), so a prompt slider or a fade costs no prompt build and no cache entry."""
        return self.infer_batch([img], prompt=prompt, height=height, width=width, strength=strength, steps=steps,
                                guidance_scale=guidance_scale, ref=ref, style_fidelity=style_fidelity,
                                controlnet=controlnet, seed=seed, controlnet_scale=controlnet_scale)[0]

    def infer_batch(self, imgs, prompt=["pixar, cg"], height=360, width=640, strength=0.4, steps=20, guidance_scale=7.5,
                    ref=False, style_fidelity=0.0, controlnet=False, seed=42, controlnet_scale=1, prompts=None, masks=None):
        """Several frames (of different sessions, or consecutive frames of one stream) with the SAME options through
        one batched launch: the result `infer` gives each frame, up to kernel rounding (frames are denoised independently), one pass over the
        weights for all of them.  Extension of the reference surface; `RemotePipeline(batch=B)` coalesces queued
        `infer` calls into this.
        prompts (objects built with `frame_prompts=True`): one prompt per frame, each what `prompt` accepts; frame i is then what `infer`
        gives it with prompts[i].  None: `prompt` for every frame.
        strength / controlnet_scale (objects built with `frame_options=True`): a number, or a sequence of one per frame; all strengths of a
        launch must give the same number of timesteps.
        masks (objects built with `keep_mask=True`): one keep mask per frame, each what `set_mask` accepts (None: that frame is restyled
        whole), for this launch alone; None: the mask of `set_mask` for every frame."""
        extra = {} if prompts is None else {"prompts": prompts}
        if masks is not None:
            extra["masks"] = masks
        return self.collect_batch(self.submit_batch(imgs, prompt=prompt, height=height, width=width, strength=strength, steps=steps,
                                                    guidance_scale=guidance_scale, ref=ref, style_fidelity=style_fidelity,
                                                    controlnet=controlnet, seed=seed, controlnet_scale=controlnet_scale, **extra))

    def warm_up(self, batches=(1,), lanes: int = 1, **options):
        """Prepare every (batch size, lane) engine a stream with these `infer` options will use -- plan, captured graph
        and one replay on black frames -- so that no frame of the stream pays for a `prepare` (tens of ms each, a
        visible stall in a 30 ms/frame stream).  A server calls it once per worker at start-up or after a respawn
        (`FrameDispatcher(warm_options=...)`); returns how many engines are ready."""
        w, h = options.get("width", INFER_DEFAULTS["width"]), options.get("height", INFER_DEFAULTS["height"])
        black = Image.new("RGB", (w, h))
        ready = 0
        for b in batches:
            handles = [self.submit_batch([black] * int(b), lane=l, **options) for l in range(max(1, int(lanes)))]
            for hd in handles:
                self.collect_batch(hd)
            ready += len(handles)
        return ready

    def submit_batch(self, imgs, lane: int = 0, prompt=["pixar, cg"], height=360, width=640, strength=0.4, steps=20,
                     guidance_scale=7.5, ref=False, style_fidelity=0.0, controlnet=False, seed=42, controlnet_scale=1, prompts=None, masks=None):
        """First half of `infer_batch`: crop / resize, upload, enqueue -- returns a handle for `collect_batch` without
        waiting for the GPU.  `lane` picks one of the prepared engines of that (options, batch size): two lanes keep two
        launches in flight while the host works on the frames around them (the worker loop of dispatch.py does that).  Six phases in this
        order -- prompts, frames, switches and options, seeds, engine and installs, enqueue: what is refused is refused before any device work."""
        if not 0 <= int(lane) < self.max_lanes:
            raise ValueError(f"lane {lane}: this pipeline was built for {self.max_lanes} launch lane(s) (kwarg `lanes`)")
        prompt, plist = self._launch_prompts(len(imgs), prompt, prompts, ref)
        t0 = time.perf_counter()
        masks = self._launch_masks(masks, len(imgs), width, height)  # (at the size asked for: sized by the rule `_launch_frames` sizes frames by)
        imgs, raw, i420, yuv, height, width = self._launch_frames(imgs, width, height, ref)
        self._note("crop_resize", t0)
        if plist is not None:  # one cache entry per frame (the same object for equal prompts)
            keys = [_prompt_key(c) for p in plist for c in PM.component_prompts(p)]
            pblock = [self._prompt_source(p, keys) for p in plist]
        else:
            pblock = self._prompt_source(prompt)  # cached: nothing to do; new: ~1 ms on the GPU, nobody waits
        key, pairs = self._launch_options(imgs, raw, strength, controlnet_scale,
                                          dict(prompt=prompt, height=height, width=width, steps=steps, ref=ref, controlnet=controlnet))
        seeds = self._launch_seeds(seed, len(imgs))
        eng = self._engine_for(key, pairs[0], len(imgs), lane, prompt=pblock, prompt_text=prompt)
        self._install(eng, key, pblock, pairs, masks)
        np.random.seed(seed if seeds is None else seeds[0] & 0xFFFFFFFF)  # kept for parity with videopipeline.py:112 (nothing downstream consumes it)
        t0 = time.perf_counter()
        self._enqueue(eng, lane, imgs, raw, i420, width, height, seeds)
        handle = Launch(eng, len(imgs), int(lane), yuv if any(yuv) else None, i420 is not None,
                        (tuple(pblock) if plist is not None else ()) + (tuple(e for e, _c in eng._want_opts) if key.frame_options else ()))
        self._in_flight.append(handle)
        self._note("upload_enqueue", t0)
        return handle

    def _prompt_source(self, prompt, keep=()):
        """What an engine takes for `prompt` (canonical): the cache entry of a text, or a PromptMix of the cache entries of a mix's texts.
        Each component goes through the prompt cache; the mix itself never enters it and is never built or encoded."""
        if not isinstance(prompt, PM.Mix):
            return self._cache_prompt(_prompt_key(prompt), prompt=prompt, keep=keep)
        from .blocks import PromptMix

        keep = tuple(keep) + prompt.texts  # (no component evicts another)
        return PromptMix([self._cache_prompt(t, prompt=t, keep=keep) for t in prompt.texts], prompt.weights)

    def _launch_prompts(self, n: int, prompt, prompts, ref):
        """Phase 1 -> (the launch's `prompt`, one prompt per frame or None in the one-prompt-per-launch mode), every prompt in its canonical
        form (promptmix.canonical: a mix that is not one is refused here, a mix of one component is that text)."""
        plist = None
        prompt = PM.canonical(prompt)
        if self.is_xl and isinstance(prompt, PM.Mix):
            raise ValueError("prompt: a mix of more than one component is not possible here: an SDXL program has the pooled text embedding "
                             "of ITS prompt baked in")
        if prompts is not None:
            if not self.frame_prompts:
                raise ValueError("prompts= (one prompt per frame) needs a pipeline built with frame_prompts=True; this one runs one prompt per launch (`prompt`)")
            plist = [PM.canonical(p) for p in prompts]
            if len(plist) != n:
                raise ValueError(f"prompts must hold one prompt per frame: {len(plist)} prompt(s) for {n} frame(s)")
        elif self.frame_prompts:
            plist = [prompt] * n
        if plist is None:
            return prompt, None
        if self.is_xl and any(isinstance(p, PM.Mix) for p in plist):
            raise ValueError("prompts: a mix of more than one component is not possible here: an SDXL program has the pooled text embedding "
                             "of ITS prompt baked in")
        if len({_prompt_key(p) for p in plist}) > 1 and (self.is_xl or (bool(ref) and self.honor_ref_flag)):
            raise ValueError("prompts: more than one distinct prompt in a launch is not possible here: " +
                             ("an SDXL program has the pooled text embedding of ITS prompt baked in" if self.is_xl else
                              "reference-only frames run one frame per launch"))
        return plist[0], plist

    def _launch_frames(self, imgs, width: int, height: int, ref):
        """Phase 2 -> (frames, raw, i420, yuv, height, width): which of the three input paths the launch takes, and its size.
        WebRTC frames (planar YUV 4:2:0: an `I420Frame`, or an av.VideoFrame by duck typing; `yuv` says which are): when EVERY frame of the
        launch is one, the planes go to the device as they are and the result comes back as I420 (`i420`, see `_i420_on_device`); otherwise
        such a frame is converted here by the host loop of the same colour contract and takes the path of a PIL image -- the same bytes either
        way.  `raw`: `device_resize` takes the frames as they came (`_raw_frames`); neither: cropped / resized here.
        A size that is not a multiple of the VAE stride: `VaeImageProcessor.preprocess` (lcm_controlnet.py:457, 230) rounds it DOWN to a
        multiple of 8 with a Lanczos resize and the pipeline returns that size.  (There the control image is the Sobel map of the unrounded
        frame, resized; here it is the Sobel map of the rounded frame -- sizes the client offers are multiples of 8.)"""
        yuv = [is_i420(im) for im in imgs]
        i420 = None
        if any(yuv):
            imgs = [I420Frame.coerce(im) if k else im for im, k in zip(imgs, yuv)]
            if all(yuv) and self._i420_on_device(imgs, width, height, ref):
                i420 = imgs
            else:
                imgs = [Image.fromarray(im.to_rgb(), mode="RGB") if k else im for im, k in zip(imgs, yuv)]
        raw = self._raw_frames(imgs, width, height) if self.device_resize and i420 is None else None
        if raw is None and i420 is None:
            imgs = [center_crop_resize(im, width, height) for im in imgs]
        if height % 8 or width % 8:
            height, width = height - height % 8, width - width % 8
            if height <= 0 or width <= 0:
                raise ValueError("height and width must be at least 8")
            imgs = [im.resize((width, height), resample=Image.Resampling.LANCZOS) for im in imgs]
        return imgs, raw, i420, yuv, height, width

    def _switches(self, controlnet, ref):
        """-> (use_cn, use_ref, frame_options in effect) for a frame with these `infer` flags.  SDXL has no ControlNet tower and the
        reference-only pipeline no ControlNet (lcm_reference_pipeline.py:855-890); both keep one pair of options per plan."""
        use_ref = bool(ref) and self.honor_ref_flag and not self.is_xl
        use_cn = not self.is_xl and not use_ref and (bool(controlnet) if self.honor_controlnet_flag else True)
        return use_cn, use_ref, self.frame_options and not self.is_xl and not use_ref

    def _plan_key(self, o) -> PlanKey:
        """The program a frame with the `infer` options `o` (all of them present, `strength` a number) runs on this object: the ONE place
        a key is built, for the launch (`submit_batch`) and for the question whether it must wait (`needs_idle`)."""
        use_cn, use_ref, frame_opts = self._switches(o["controlnet"], o["ref"])
        return PlanKey(o["height"] - o["height"] % 8, o["width"] - o["width"] % 8, int(o["steps"]),
                       len(lcm_timesteps(float(o["strength"]), int(o["steps"]))), use_cn, use_ref,
                       _prompt_key(o["prompt"]) if self.is_xl else None, self.device_seed, self.frame_prompts, frame_opts)

    def _launch_options(self, imgs, raw, strength, controlnet_scale, o):
        """Phase 3 -> (the PlanKey of the launch, one (strength, controlnet_scale) per frame); `o`: the other options the key depends on.
        The launch's program is fixed by the COMMON number of timesteps of its strengths.  The first frame seen with an honoured
        `ref=True` becomes the reference image, stored as the host path stores it."""
        n = len(imgs)
        _use_cn, use_ref, frame_opts = self._switches(o["controlnet"], o["ref"])
        if use_ref:
            if n != 1:
                raise ValueError("ref=True: one frame per call (the reference-only program runs one frame per launch)")
            if self._ref_img is None:
                self._ref_img = imgs[0] if raw is None else center_crop_resize(imgs[0], o["width"], o["height"])
                self._ref_epoch += 1
        strengths = self._per_frame(strength, n, "strength")
        cn_scales = self._per_frame(controlnet_scale, n, "controlnet_scale")
        if not frame_opts and (len(set(strengths)) > 1 or len(set(cn_scales)) > 1):
            raise ValueError("strength / controlnet_scale with different values per frame need a pipeline built with frame_options=True "
                             "(and neither an SDXL nor a reference-only program): this launch runs one pair of options")
        key = self._plan_key(dict(o, strength=strengths[0]))  # ValueError for an empty schedule: the caller's problem
        counts = [key.n_eff] + [len(lcm_timesteps(v, key.steps)) for v in dict.fromkeys(strengths[1:])]
        if len(set(counts)) > 1:
            raise ValueError(f"the strengths {strengths} give different numbers of timesteps at steps={key.steps} ({sorted(set(counts))}): "
                             "the frames of one launch run one program; launch them separately")
        return key, list(zip(strengths, cn_scales))

    def _launch_seeds(self, seed, n: int):
        """Phase 4 -> one int per frame with `device_seed`; None without (engines of the default mode, and stand-ins, are called as before)"""
        if not self.device_seed:
            return None
        seeds = [seed] * n if isinstance(seed, (int, np.integer)) else list(seed)
        if len(seeds) != n or not all(isinstance(v, (int, np.integer)) for v in seeds):
            raise ValueError(f"seed must be an int or a sequence of {n} ints (one per frame)")
        return [int(v) for v in seeds]

    def _install(self, eng, key: PlanKey, pblock, pairs, masks=None):
        """Phase 5, after `_engine_for`: this lane's launch reads ITS copy of the constants (the other lanes may run other prompts); a changed
        frame slot is rewritten on this lane's stream ahead of the program, so nobody waits."""
        eng.use_prompts(pblock) if isinstance(pblock, list) else eng.use_prompt(pblock)
        if key.frame_options:
            eng.use_options(pairs)
        if self.color_match is not None and set(eng.color_a) != {self._color_a}:  # (`set_color_match` since this engine's last launch)
            eng.set_color_amount(self.color_amount)
        for switch, sigma in self._blur.items():  # (`set_edge_blur` / `set_mask_feather` since this engine's last launch)
            if eng.taps[switch].sigma != sigma:
                eng._set_blur(switch, sigma)
        if isinstance(masks, list):  # `masks=[...]`: this launch's own; the next launch without them takes `set_mask`'s again
            eng.set_masks(masks)
            eng._mask_pipe_epoch = None
        elif masks is not None and eng._mask_pipe_epoch != masks[0]:  # (`set_mask` since this engine's last launch, or a new engine)
            eng.set_masks(masks[1])
            eng._mask_pipe_epoch = masks[0]
        if key.use_ref and eng._ref_epoch != self._ref_epoch:
            rf = np.asarray(center_crop_resize(self._ref_img.convert("RGB"), key.width, key.height), dtype=np.uint8)
            eng.ops.upload(eng.ref_u8, torch.from_numpy(np.array(rf, copy=True)))  # (PIL's buffer is read-only)
            eng._ref_epoch = self._ref_epoch

    def _enqueue(self, eng, lane, imgs, raw, i420, width, height, seeds):
        """Phase 6: upload and launch by the path `_launch_frames` chose; counts the bytes handed to the host-to-device copy per frame"""
        skw = dict(overlap=self._overlap_now(lane), **({} if seeds is None else {"seeds": seeds}))
        if i420 is not None:
            eng.submit_raw_i420(i420[0] if len(i420) == 1 else i420, **skw)
            up = eng.last_upload_bytes
        elif raw is not None:
            eng.submit_raw_u8(raw[0] if len(raw) == 1 else raw, **skw)
            up = sum((b[2] - b[0]) * (b[3] - b[1]) * 3 for b in (eng.ops.center_crop_box(f.shape[1], f.shape[0], width, height) for f in raw))
        else:
            frames = np.stack([np.asarray(im if im.mode == "RGB" else im.convert("RGB"), dtype=np.uint8) for im in imgs])
            eng.submit_u8(frames[0] if len(imgs) == 1 else frames, **skw)
            up = frames.nbytes
        self._io_bytes["up"] = up // len(imgs)  # (counted, not timed)

    def _i420_on_device(self, frames, width: int, height: int, ref) -> bool:
        """Do these `I420Frame`s take the device path (`Engine.submit_raw_i420` / `collect_i420`)?  Not what `_raw_frames` sends to the
        host either: a target size that is not a multiple of 8, `ref=True` on an object that honours it, an ops object without the
        kernels, a side above the limit.  Independent of `device_resize`: a new input type has no earlier behaviour to keep."""
        ops = getattr(self.model, "ops", None)
        if height % 8 or width % 8 or height <= 0 or width <= 0 or not all(hasattr(ops, a) for a in ("i420_to_rgb", "rgb_to_i420", "resample_rgb")):
            return False
        if (bool(ref) and self.honor_ref_flag and not self.is_xl) or max(height, width) > RESAMPLE_MAX_SIDE:
            return False
        return all(max(f.size) <= RESAMPLE_MAX_SIDE for f in frames)

    def _raw_frames(self, imgs, width: int, height: int):
        """`device_resize`: the frames as uint8 [h][w][3] arrays for `Engine.submit_raw_u8`, or None when this call keeps the host
        path: a frame that is not RGB, a target size that is not a multiple of 8 (the second Lanczos step below), a side the
        kernel refuses, an ops object without the kernel."""
        if height % 8 or width % 8 or height <= 0 or width <= 0 or not hasattr(getattr(self.model, "ops", None), "resample_rgb") or max(height, width) > RESAMPLE_MAX_SIDE:
            return None
        for im in imgs:
            if getattr(im, "mode", None) != "RGB" or min(im.size) < 1 or max(im.size) > RESAMPLE_MAX_SIDE:
                return None
        return [np.asarray(im, dtype=np.uint8) for im in imgs]

    def _overlap_now(self, lane: int) -> bool:
        """ONE policy for every caller (bench.py's engine legs follow the same rule): a launch runs its ControlNet encoder on
        the lane's side stream when it will have a command-processor pipe to itself -- at most two launches in flight, all on
        lanes 0 / 1 (lane l's side stream is lane l + 2's own stream).  A lone frame gains ~4 ms from it; with three or four
        lanes busy the side streams ARE the other lanes' streams and the launch stays on its own."""
        if os.environ.get("VSD_OVERLAP_CN") is not None:
            return os.environ.get("VSD_OVERLAP_CN") == "1"
        return int(lane) < 2 and all(h.lane < 2 for h in self._in_flight) and len(self._in_flight) < 2

    def collect_batch(self, handle: Launch):
        """Second half of `infer_batch`: wait for the launch of `handle`, bring its frames back -> PIL images, or I420Frames where I420 came in"""
        eng, n, yuv, on_device = handle.engine, handle.frames, handle.yuv, handle.on_device
        t0 = time.perf_counter()
        try:
            out = eng.collect_i420() if on_device else eng.collect_u8()
        finally:
            self._in_flight[:] = [h for h in self._in_flight if h is not handle]
        self._note("wait_download", t0)
        self._io_bytes["down"] = (eng.last_download_bytes if on_device else out.nbytes) // n
        if eng.last_gpu_ms is not None:
            self._host_ms["gpu"].append(eng.last_gpu_ms)
        t0 = time.perf_counter()
        if on_device:  # (the conversion ran on the device: nothing is left for the host)
            res = [out] if n == 1 else out
        else:
            res = [I420Frame.from_rgb(o) if k else Image.fromarray(o, mode="RGB") for o, k in zip(out[None] if n == 1 else out, yuv or [False] * n)]
        self._note("to_pil" if yuv is None else "to_i420", t0)
        return res

    @property
    def _engines(self):
        """(plan_key, frames per launch, lane) -> prepared engine, over all cached plans"""
        return {(pk, b, l): e for pk, pl in self._plans.items() for (b, l), e in pl.engines.items()}

    def needs_idle(self, **options) -> bool:
        """Would a frame with these `infer` options have to wait for launches in flight?  Only a change of `strength` /
        `controlnet_scale` of a plan that is running does (its graphs read those constants); other prompts, sizes, step
        counts and batch sizes go beside what is running.  (dispatch.py's worker drains before such a frame.)"""
        try:
            o = dict(INFER_DEFAULTS, **options)
            key = self._plan_key(o)
            if key.use_ref:
                return bool(self._in_flight)  # (reference image upload + one frame per launch: keep it simple)
            if key.frame_options:
                return False  # (options are per frame slot of the lane's own engine: a new value never waits for another lane)
            plan = self._plans.get(key)
            return plan is not None and plan.opts != (float(o["strength"]), float(o["controlnet_scale"])) and plan.busy(self._in_flight)
        except Exception:
            return bool(self._in_flight)

    def _engine_for(self, plan_key, opts, batch: int, lane: int = 0, prompt=None, prompt_text=None):
        """A prepared engine per (program, frames per launch, lane).  A program's first engine owns its schedule constants;
        the others are slots of it (shared weights and constants, own arena / prompt constants / graph), so that switching
        between batch sizes, lanes, prompts and PROGRAMS costs nothing per frame.  `opts` = (strength, controlnet_scale): a
        change rewrites that program's device constants, nothing else."""
        strength, cn_scale = opts
        frame_opts = plan_key.frame_options  # (options per frame slot of each engine: the plan has none, `opts` only seeds `prepare`)
        plan = self._plans.get(plan_key)
        if plan is not None:
            self._plans.move_to_end(plan_key)
            if not frame_opts and opts != plan.opts:
                if plan.busy(self._in_flight):
                    raise RuntimeError("cannot change strength / controlnet_scale of a plan with launches in flight: collect them first")
                t0 = time.perf_counter()
                if not plan.root.update_options(strength, cn_scale):  # (cannot happen: the timestep count is in the key)
                    raise RuntimeError("update_options refused a schedule with the same number of timesteps")
                plan.opts = opts
                self._note("update_options", t0)
            eng = plan.engines.get((batch, lane))
            if eng is not None:
                if any(h.engine is eng for h in self._in_flight):
                    raise RuntimeError("this lane's previous launch has not been collected")
                return eng
        t0 = time.perf_counter()
        self._trim_memory(keep=plan_key)
        if plan is None:
            # least recently used PROGRAMS go first, but never one with a launch still running (the cache then grows)
            for pk in list(self._plans):
                if len(self._plans) < max(1, self.max_plans):
                    break
                if not self._plans[pk].busy(self._in_flight):
                    self._evict(pk)
            eng = self.model.make_slot(share_plan=False, lane=lane)  # its own schedule constants: the other programs keep running
            plan = self._plans[plan_key] = _Plan(eng, None if frame_opts else opts)
        else:
            eng = plan.root.make_slot(lane=lane)
        if prompt is not None:
            eng.use_prompts(prompt) if isinstance(prompt, list) else eng.use_prompt(prompt)
        if self.is_xl:  # micro-conditioning: original size = target size = the frame size, no crop
            eng.set_added_cond(self.encode_pooled(prompt_text if prompt_text is not None else ""),
                               (plan_key.height, plan_key.width, 0, 0, plan_key.height, plan_key.width))
        # (every engine is captured both ways -- ControlNet encoder on the lane's side stream / everything on the lane's own stream;
        #  `submit_batch` picks per launch, see `_overlap_now`)
        # Kernel choices: coalesced launches of a worker with three or four lanes are the loaded case -- the forms that cost least with four
        # lanes busy; one-frame launches and workers with one or two lanes are the latency case -- the forms that are fastest alone.  Fixed
        # per plan, the same on every lane (same bits whichever lane a frame lands on).
        eng.tune_for_lanes = self.max_lanes >= 3 and batch > 1
        mode = {k: True for k in ("device_seed", "frame_prompts", "frame_options") if getattr(plan_key, k)}  # (the default mode, and stand-ins: none)
        if self.edges != "sobel":  # (not in the plan key: constant for the life of this object)
            mode.update(edges=self.edges, canny_thresholds=self.canny_thresholds)
        if self.color_match is not None:  # (likewise)
            mode.update(color_match=self.color_match, color_amount=self.color_amount)
        if self.keep_mask:  # (likewise; SDXL and reference-only programs are refused by `prepare`, by name)
            mode.update(keep_mask=True)
        mode.update(self._blur)  # (likewise: edge_blur / mask_feather, at the sigma of the moment)
        eng.prepare(plan_key.height, plan_key.width, plan_key.steps, strength, controlnet_scale=cn_scale, use_controlnet=plan_key.use_cn,
                    batch=batch, ref_mode=plan_key.use_ref, autotune=self.tuning_mode != "table", **mode)
        plan.engines[(batch, lane)] = eng
        self._note("prepare", t0)
        return eng

    def _memory_used_and_limit(self, before=None):
        dev = int(self.device)
        used = torch.cuda.memory_allocated(dev)
        if before is not None and used >= before:  # an evicted engine still referenced from a cycle: collect it now
            gc.collect()
            used = torch.cuda.memory_allocated(dev)
        return used, self.memory_budget * torch.cuda.mem_get_info(dev)[1]

    def _evict(self, key) -> int:
        """drop the (idle) program `key` from the cache and release its engines' graphs -> how many engines went"""
        return self._plans.pop(key).destroy()

    def _trim_memory(self, keep=None):
        """Before another engine (= another arena) is allocated: while the allocator holds more than the budget, drop idle
        cached state, cheapest to rebuild last -- other programs (least recently used first), then the idle slots of the
        program `keep` itself (never its root: it owns the schedule constants the slots share).  Engines with a launch in
        flight are never touched; if nothing idle is left the allocation goes ahead (and may fail loudly in the allocator)."""
        used, limit = self._memory_used_and_limit()
        if used <= limit:
            return 0
        dropped = 0
        for pk in list(self._plans):
            if pk == keep or self._plans[pk].busy(self._in_flight):
                continue
            dropped += self._evict(pk)
            used = self._memory_used_and_limit(before=used)[0]
            if used <= limit:
                break
        plan = self._plans.get(keep)
        if plan is not None and used > limit:
            for k, e in list(plan.engines.items()):
                if e is plan.root or any(h.engine is e for h in self._in_flight):
                    continue
                del plan.engines[k]
                e._destroy_graphs()
                dropped += 1
                e = None
                used = self._memory_used_and_limit(before=used)[0]
                if used <= limit:
                    break
        self.evictions += dropped
        return dropped

    def export_plan(self, path: str, frames_per_launch: int = 1, **options) -> dict:
        """The program `infer(img, **options)` runs on this pipeline -- model, prompt, frame size, steps, strength, ControlNet scale --
        as a FILE for hosts without Python: include/vsd.h vsd_plan_load / vsd_plan_infer (examples/plan_host.c) replay it with the
        same kernels and arguments, bit for bit this class's frames.  The host feeds frames already cropped / resized to
        (height, width) (videopipeline.py:92-107 does that with PIL); another size or step count is another plan, another prompt is
        `export_prompt`, another strength / ControlNet scale is vsd_plan_set_options on the loaded plan.
        `frames_per_launch` > 1: the coalesced program of `infer_batch`.  Returns the exporter's summary (videosd_amd/plan.py)."""
        from .plan import export_plan

        if self.frame_prompts:
            raise ValueError("export_plan: this pipeline was built with frame_prompts=True; a plan file holds ONE prompt's constants and the C "
                             "library has no per-frame prompt entry point yet: export from a pipeline built without it")
        if self.frame_options:
            raise ValueError("export_plan: this pipeline was built with frame_options=True; its programs call vsd_add_noise_frames, "
                             "vsd_lcm_step_frames, vsd_groupnorm_addvec and vsd_cn_merge_frames, which are not plan functions: export from a "
                             "pipeline built without it (a loaded plan follows the sliders through vsd_plan_set_options)")
        if self.edges != "sobel":
            raise ValueError(f'export_plan: this pipeline was built with edges="{self.edges}"; its programs call vsd_canny_control, which is not a '
                             'plan function: export from a pipeline built with edges="sobel" (the default)')
        if self.color_match is not None:
            raise ValueError(f'export_plan: this pipeline was built with color_match="{self.color_match}"; its programs call vsd_color_match, which is '
                             'not a plan function: export from a pipeline built with color_match=None (the default)')
        if self._blur:
            raise ValueError(f"export_plan: this pipeline was built with {' and '.join(self._blur)}; its programs call vsd_gauss_blur, which is not a "
                             "plan function: export from a pipeline built without it")
        if self.keep_mask:
            raise ValueError("export_plan: this pipeline was built with keep_mask=True; its programs call vsd_mask_latent, vsd_latent_keep and "
                             "vsd_mask_blend, which are not plan functions: export from a pipeline built without it")
        if self._loras:
            raise ValueError("export_plan: this pipeline was built with loras=[...]; a plan file would freeze the weights at the scales of the "
                             "moment and the C library has no entry point that moves them: export from a pipeline built without adapters")
        if isinstance(PM.canonical(options.get("prompt", INFER_DEFAULTS["prompt"])), PM.Mix):
            raise ValueError("export_plan: `prompt` is a mix; a plan file holds ONE cached prompt's constants and the C library forms no mix "
                             "for a plan (vsd_prompt_mix is not a plan function): export with one of the texts")
        self._require_idle("export a plan")
        w, h = int(options.get("width", INFER_DEFAULTS["width"])), int(options.get("height", INFER_DEFAULTS["height"]))
        imgs = [Image.new("RGB", (w, h), (127, 127, 127)) for _ in range(int(frames_per_launch))]
        handle = self.submit_batch(imgs, **options)
        self.collect_batch(handle)
        return export_plan(handle.engine, path)

    def export_prompt(self, path: str, prompt) -> int:
        """Another prompt's constants as a file for vsd_plan_load_prompt (a loaded plan takes it without a new plan)."""
        from .plan import export_prompt

        if self._blur:
            raise ValueError(f"export_prompt: this pipeline was built with {' and '.join(self._blur)}; its programs have no plan file a prompt file "
                             "could belong to (vsd_gauss_blur is not a plan function): export from a pipeline built without it")
        if self.keep_mask:
            raise ValueError("export_prompt: this pipeline was built with keep_mask=True; its programs have no plan file a prompt file could "
                             "belong to (vsd_mask_latent, vsd_latent_keep and vsd_mask_blend are not plan functions): export from a pipeline "
                             "built without it")
        if self._loras:
            raise ValueError("export_prompt: this pipeline was built with loras=[...]; a prompt's constants depend on the adapted weights and a "
                             "plan file knows nothing of them: export from a pipeline built without adapters")
        if isinstance(PM.canonical(prompt), PM.Mix):
            raise ValueError("export_prompt: `prompt` is a mix; a prompt file holds ONE cached prompt's constants (it does not say which of its "
                             "bytes are fp16, fp32 or independent of the prompt, so the C side could not mix two of them): export the texts")
        return export_prompt(self._cache_prompt(_prompt_key(prompt), prompt=prompt), path)

    def set_tuning_mode(self, mode: str):
        """ "auto" (time the candidates of shapes the table lacks at `prepare`) or "table" (never: deterministic heuristic)."""
        if mode not in ("auto", "table"):
            raise ValueError("tuning_mode must be 'auto' or 'table'")
        self.tuning_mode = mode
        return mode

    def export_tuning(self):
        """The per-shape kernel choices of this process (table + what `prepare` measured), for `import_tuning` elsewhere."""
        return {k: tuple(v) for k, v in self.model.ops.tile_override.items()}

    def import_tuning(self, table):
        """Take another process's choices for shapes this one has none for yet (rank 0's after its warm-up: every rank then
        builds the same kernels for the same shapes -- same bits whichever rank a frame lands on)."""
        n = 0
        for k, v in table.items():
            if k not in self.model.ops.tile_override:
                self.model.ops.tile_override[k] = tuple(v)
                n += 1
        return n

    # `VideoSDPipeline.remote(**config)` -> awaitable handle (replaces the Ray actor API, server.py:320-321)
    @classmethod
    def remote(cls, **config):
        from .dispatch import RemotePipeline

        return RemotePipeline(**config)

    @classmethod
    def remote_group(cls, gpus: int, **config):
        """`gpus` workers, one per GPU, in one RCCL process group (config.yaml `gpus: N`, server.py:273-274, 317-321)."""
        from .dispatch import spawn_workers

        return spawn_workers(int(gpus), **config)


VideoPipeline = VideoSDPipeline  # BASELINE.json's north_star calls the class by this name
# the defaults of `infer` (its three literal signatures mirror the reference's), for everything here that completes an option dict
INFER_DEFAULTS = {k: v.default for k, v in inspect.signature(VideoSDPipeline.infer).parameters.items() if v.default is not v.empty}

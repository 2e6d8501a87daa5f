"""Per-frame denoising engine: sequences the libvsd kernels for TAESD-encode -> N x (ControlNet, UNet,
LCM step) -> TAESD-decode, records the sequence once as a static program, and replays it as ONE hipGraph
per frame.

Replaces the body of LatentConsistencyModelPipeline_controlnet.__call__
(/root/reference/diffusert/lcm/lcm_controlnet.py:379-618) and the diffusers modules it drives.  All
compute goes through an `ops` object (videosd_amd.ops.HipOps -> libvsd.so); this module only decides
which buffers each kernel reads and writes.  The packed weights are netweights.py, the arena / recorder / capture of the
static program program.py, the prompt and option blocks with their layouts blocks.py; their names are importable from here.

Data layout in HBM
  * activations: fp16 [H*W][C] (channels-last), bump-allocated from one arena that is rewound at every
    denoising step so all steps reuse the same addresses;
  * 4-channel latent-like tensors: row stride 8, channels 4..7 zero;
  * weights: fp16 [N][Kp], K ordered (ky,kx,c) (videosd_amd/packing.py), resident for the process lifetime;
  * per-(strength,steps) constants: time-embedding projections of every ResnetBlock for every step, the
    noise draws, scheduler coefficients; per-prompt constants: cross-attention K and V^T of every layer.
"""
import copy
import os
import weakref
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import blur
from . import lib as L
from .blocks import (FRAME_OPTION_OPS, MAX_OPTION_ENTRIES, FramePromptLayout, FrameSlots, OptionEntry, OptionLayout,  # noqa: F401
                     PromptBlock, PromptLayout, PromptMix, controlnet_scales, mix_segments, option_segments, prompt_segments, same_source,
                     schedule_constants)
from .config import ControlNetConfig, TAESDConfig, UNetConfig
from .convform import OWN_SPLIT, lookup
from .lcm import LCMSchedule, timestep_sinusoid, w_embedding
from .netweights import XATTN_ABSORB_MIN_C, BlockW, NetWeights, ResnetW, TAESDWeights, TransformerW  # noqa: F401
from .ops import Geom
from .packing import _round_up as _ru
from .program import SYNC_OPS, Arena, Recorder, capture, flat_calls, launches_by_kind

KEEP_MASK_OPS = ("mask_latent", "latent_keep", "mask_blend")  # what `prepare(keep_mask=True)` records besides the default program's ops
BLUR_SWITCHES = ("edge_blur", "mask_feather")  # the two uses of the device blur (include/vsd.h THE BLUR CONTRACT): `prepare` kwargs, keys of `Engine.taps`


class TapBlock:
    """One tap table of the device blur as an engine holds it: int32 [34] on the device, read by the recorded `gauss_blur` when it runs (a
    captured graph holds the address), its pinned mirror, and the table the next launch runs with -- the pattern of the masks and the
    colour amounts: a setter only notes, `sync` sends a changed table ahead of the program."""

    def __init__(self, ops, sigma):
        self.dev = ops.zeros(blur.TAPS, dtype=torch.int32)
        self.host = torch.zeros(blur.TAPS, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        self.sigma, self.want, self.epoch, self.sent = None, None, 0, None
        self.set(sigma)

    def set(self, sigma):
        taps = blur.gauss_taps(sigma)  # (refuses by name)
        self.sigma = float(sigma)
        if self.want is None or not np.array_equal(taps, self.want):
            self.want = taps
            self.epoch += 1

    def sync(self, ops):
        """136 bytes on the lane's stream, when the table changed (the lane's previous launch has been collected: nothing reads the mirror)"""
        if self.sent != self.epoch:
            self.host.numpy()[:] = self.want
            ops.upload(self.dev, self.host)
            self.sent = self.epoch


def _env_switch(name: str, default: bool) -> bool:
    """an A/B switch of the environment: unset -> `default`, "1" -> on, anything else -> off"""
    v = os.environ.get(name)
    return default if v is None else v == "1"


class SchedulerOps:
    """Records a plan's scheduler ops for the noise source and the coefficient form `prepare` chose (include/vsd.h: kind 0 draw d =
    noise[d], kind 1 draw d = noise_ref[d]; a step with draw 0 adds none).  seeds: one per frame, on the device (`device_seed`), else the
    host draws `noise` / `noise_ref`; coef_stride: floats between two frames' coefficients (`frame_options`), 0: one set per launch."""

    def __init__(self, hw: int, noise=None, noise_ref=None, seeds=None, coef_stride: int = 0):
        self.hw, self.noise, self.noise_ref, self.seeds, self.coef_stride = hw, noise, noise_ref, seeds, coef_stride

    def add_noise(self, r, x0, kind, draw, coef, batch, out):
        hw, seeds, cs = self.hw, self.seeds, self.coef_stride
        table = None if seeds is not None else (self.noise_ref if kind else self.noise)[draw]
        if cs and seeds is not None:
            r.add_noise_frames(x0, None, seeds, kind, draw, coef, cs, hw, batch, out)
        elif cs:
            r.add_noise_frames(x0, table, None, 0, 0, coef, cs, hw, batch, out)
        elif seeds is not None:
            r.add_noise_seeded(x0, seeds, kind, draw, coef, hw, batch, out)
        else:
            r.add_noise_dev(x0, table, coef, hw, batch, out)

    def lcm_step(self, r, eps, cur, draw, coef, batch, nxt, den, dec_in):
        hw, seeds, cs = self.hw, self.seeds, self.coef_stride
        table = self.noise[draw] if seeds is None and draw else None
        if cs and seeds is not None:  # (draw 0: the step adds no noise -- neither source)
            r.lcm_step_frames(eps, cur, None, seeds if draw else None, 0, draw, coef, cs, hw, batch, nxt, den, dec_in)
        elif cs:
            r.lcm_step_frames(eps, cur, table, None, 0, 0, coef, cs, hw, batch, nxt, den, dec_in)
        elif seeds is not None:
            r.lcm_step_seeded(eps, cur, seeds, 0, draw, coef, hw, batch, nxt, den, dec_in)
        else:
            r.lcm_step_dev(eps, cur, table, coef, hw, batch, nxt, den, dec_in)

    def latent_keep(self, r, x0, weights, coef, batch, lat):
        """the step form of the keep mask's latent anchor behind an `lcm_step`: that step's coefficients, this plan's coefficient form and
        draw 0 of kind 0 from this plan's noise source (what `add_noise` gave the frame)"""
        seeds = self.seeds
        r.latent_keep(x0, weights, None if seeds is not None else self.noise[0], seeds, 0, 0, coef, self.coef_stride, self.hw, batch, lat, None, None)

    def latent_keep_final(self, r, x0, weights, batch, den, dec_in):
        r.latent_keep(x0, weights, None, None, 0, 0, None, 0, self.hw, batch, None, den, dec_in)


class RefCtx:
    """Bookkeeping of the reference-only mode while the program is recorded (SURVEY.md 8f-4;
    /root/reference/diffusert/lcm/lcm_reference_pipeline.py:498-794).  mode "write": the UNet pass over the noised reference
    latents leaves, per BasicTransformerBlock, its self-attention K rows and V^T columns in the SECOND half of buffers the
    read pass fills the first half of (the bank of norm1 outputs, :527, enters attention only through to_k / to_v, and
    those projections are exactly the write pass's own K / V), and per gated block output its per-channel (sum, sumsq)
    (:587-598).  mode "read": self-attention runs over [x ; bank] keys (:535-539) and the gated outputs are AdaIN-ed to the
    banked statistics (:593-603)."""

    def __init__(self, cfg):
        self.mode = "write"
        self.kv = {}      # kv_index -> (qk_full [2*hw][2c], vt_full [c][ldvt])
        self.stats = {}   # (kind, i, j) -> fp32 [c][2] of the write pass
        nd = nu = len(cfg.block_out_channels)
        self.nd, self.nu = nd, nu

    def gate(self, kind, i, weight=1.0):
        # module.gn_weight, lcm_reference_pipeline.py:816-846 (gn_auto_machine_weight = 1.0)
        gw = 0.0 if kind == "mid" else (2.0 * (1.0 - i / self.nd) if kind == "down" else 2.0 * i / self.nu)
        return weight >= gw


# ------------------------------------------------------------------------------------------ the engine
class Engine:
    """One engine = one GPU, one weight replica (reference: one Ray actor, videopipeline.py:11-32)."""

    def __init__(self, ops, unet_cfg: UNetConfig, cn_cfg: ControlNetConfig, vae_cfg: TAESDConfig,
                 w_unet: Dict[str, torch.Tensor], w_cn: Optional[Dict[str, torch.Tensor]], w_vae: Dict[str, torch.Tensor],
                 guidance_scale: float = 7.5):
        self.ops = ops
        self.ucfg, self.ccfg, self.vcfg = unet_cfg, cn_cfg, vae_cfg
        # (the width threshold is read from THIS module when an engine is made: tests lower `engine.XATTN_ABSORB_MIN_C`)
        self.unet = NetWeights(ops, unet_cfg, w_unet, absorb_min_c=XATTN_ABSORB_MIN_C)
        self.cn = NetWeights(ops, cn_cfg.unet, w_cn, True, cn_cfg, absorb_min_c=XATTN_ABSORB_MIN_C) if w_cn is not None else None
        self.vae = TAESDWeights(ops, w_vae)
        # ---- what a family shares: everything a slot (`make_slot`) inherits besides the weights above
        self.guidance_scale = guidance_scale  # never forwarded by the reference (videopipeline.py:114-124): 7.5
        self.text = None
        self.added = None  # SDXL: (pooled text embeds, 6 time ids)
        self.use_graph = True
        self.is_slot = False
        self.batch = 1
        # record the ControlNet encoder for a second stream, parallel to the UNet encoder (`VSD_OVERLAP_CN`: A/B switch; callers that
        # set the attribute afterwards still win)
        self.overlap_controlnet = _env_switch("VSD_OVERLAP_CN", True)
        self.overlap_launch = True      # ... and launch it that way by default (`launch(overlap=...)` decides per launch)
        # kernel choices of the plan: False = each layer's fastest form ALONE on an idle GPU (a lone launch: latency), True = the
        # form that costs least with four launch lanes busy (throughput; ops.HipOps.tune_conv).  Fixed per plan at `prepare`.
        self.tune_for_lanes = False
        # ... and, optionally, while that stream is otherwise idle: the ControlNet skip merges beside the mid block / decoder
        # start and Sobel + conditioning embedding beside the TAESD encoder (`use_side_stream`).  Measured on MI355X (512x512,
        # 4 steps): one frame alone 23.8 -> 23.2 ms, but with two launches in flight 97 -> 81 frames/s -- four busy hardware
        # queues instead of two cost more than the filled gaps give.  Round 4, launch streams on their own pipes: level either
        # way (one frame 47.8 vs 47.6 launches/s, 5 x 2 128.0 vs 128.4).  Off; `VSD_SIDE=1` switches it on.  (Round 2 also
        # moved the decoder's 1x1 shortcut convs there: 23.6 ms, removed.)
        self.use_side_stream = _env_switch("VSD_SIDE", False)
        # what a slot shares with its parent besides the weights: the per-plan constant block (schedule coefficients,
        # ControlNet scales) that the captured graphs READ, so that `update_options` reaches every graph at once
        self.shared = {}
        # what EVERY engine made from this one shares (weights aside): the prompt-constant layout and the default prompt
        # (`set_text_embeds`); an engine follows the default unless `use_prompt` gave it one of its own
        self.family = {}
        self.absorb_cross_attention = True  # cross-attention of the wide blocks as two GEMMs (vsd_xattn_fold)
        self.use_fused_tail = True          # 320-wide blocks: per-token chains as fused launches (csrc/fused_tail.hip)
        self.group_merges = not os.environ.get("VSD_NO_GROUP")  # the ControlNet merges of a step as two grouped launches
        # the one-stream form of the program runs the UNet and the ControlNet encoder of a step in lock step, twin layers as one
        # grid (`prepare`: both forms are recorded, `launch` picks)
        self.twin_encoders = not os.environ.get("VSD_NO_TWIN")
        self.group_shortcuts = not os.environ.get("VSD_NO_GROUP_SHORTCUT")  # (a ResnetBlock's shortcut conv in conv1's grid)
        self.tail_b_min_rows = 1024         # ... the feed-forward chain from this many tokens per launch on (see _transformer)
        # ---- what belongs to this engine alone
        self._reset_own_state()

    def _reset_own_state(self):
        """EVERY attribute that belongs to one engine -- what two engines of a family running side by side on different lanes must not
        share -- at its empty value.  `__init__` and `make_slot` call it; no other place creates an attribute of an engine."""
        self._reset_plan_state()
        # the prompt: outlives a plan (a `prepare` for the same text length keeps the block and what it holds)
        self.pblock = None          # this engine's own prompt constants (the addresses its program / graph reads)
        self._installed = None      # the PromptBlock (or PromptMix) whose bytes a single-prompt `pblock` currently holds
        self._want = None           # `use_prompt`: this engine's prompt (None: the family default)
        self._want_list = None      # `use_prompts`: one PromptBlock per frame of the launch (None: `_want` / the default for every frame)
        self._prompt_slots = None   # FrameSlots of a per-frame `pblock` (`prepare(frame_prompts=True)`): the PromptBlock each slot holds
        self._prompt_epoch = 0      # the family's "weights_epoch" (`set_adapter_scales`) that `_installed` / `_prompt_slots` were written under
        # device memory and pinned host memory that is reused from plan to plan
        self._vt_pool = {}          # (C, columns, index) -> zero-padded V^T buffer of a self-attention, outside the rewound arena
        self._stage = None          # (shape, pinned frame in, pinned frame out, event before the launch, event after it): `_staging`
        self._raw_stage = None      # (pinned bytes, device bytes) of the crop boxes of camera frames: `_raw_staging`
        self._i420_stage = None     # (device bytes, pinned bytes) of the I420 output: `_enqueue_i420`
        # what the last submit / collect measured
        self.last_gpu_ms = None         # the launch alone, between the events of `_stage`
        self.last_upload_bytes = 0      # `submit_raw_i420`: bytes handed to the host-to-device copies
        self.last_download_bytes = 0    # `collect_i420`: bytes brought back

    def _reset_plan_state(self):
        """The part of an engine's own state that ONE `prepare` makes: `prepare` starts from these values (after `_destroy_graphs`)."""
        self.plan = None             # the prepared plan's description (what `prepare` returns)
        self.program = None          # the recorded program: what a lone launch runs
        self.program_serial = None   # ... and its one-stream form
        self.graph = None            # the captured launch sequence of `program`
        self.graph_serial = None     # ... of `program_serial` (the same object when the two forms do not differ)
        self.arena = None            # the activations' bump allocator
        self._vt_count = 0           # index of the next V^T buffer of a denoising step in `_vt_pool`
        self.buffers = None          # name -> the program's persistent tensors (latents, eps, ...), for tests and probes
        self.frame_u8 = None         # the launch's input frame(s)
        self.out_u8 = None           # ... its output frame(s)
        self.edge_u8 = None          # ... its edge map(s)
        self.edges = None            # what `edge_u8` and the ControlNet's conditioning hold: "sobel" (the reference's stand-in) or "canny"
        self.canny_thresholds = None  # `edges="canny"`: (low, high), integers on |dx| + |dy|
        self.color_mode = None       # the colour-match stage behind `postprocess_rgb`: None, "histogram" or "meanstd"
        self.color_amounts = None    # ... its amounts on the device, int32 [B] (0..256): the program reads them when it runs
        self._color_host = None      # ... their pinned mirror
        self.color_a = None          # ... what the next launch runs with: a tuple of B integers (`set_color_amount`)
        self._color_sent = None      # ... and what `color_amounts` holds (`_sync_color`)
        self.keep_mask = False       # the keep-mask stages (include/vsd.h THE KEEP MASK) are part of the program
        self.mask_u8 = None          # ... the masks on the device, u8 [B][H][W] (255: restyled, 0: kept): the program reads them when it runs
        self.mask_w = None           # ... their latent weights, fp32 [B][hw0], written by the program's `mask_latent`
        self._mask_host = None       # ... the masks' pinned mirror
        self._mask_want = None       # ... what the next launch runs with: u8 [B][H][W] on the host (`set_masks`)
        self._mask_epoch = 0         # ... counts the `set_masks` calls that changed `_mask_want`
        self._mask_sent = None       # ... and the epoch `mask_u8` holds (`_sync_mask`)
        self._mask_pipe_epoch = None  # ... and which mask of the pipeline `_mask_want` is (VideoSDPipeline sets it; None: a launch's own masks)
        self.taps = {}               # the device blur's tap tables: "edge_blur" / "mask_feather" -> TapBlock, for the switches `prepare` was given
        self.blur_u8 = None          # `edge_blur` with a ControlNet: the blurred frames, u8 [B][H][W][3]: what the edge ops read
        self.mask_soft = None        # `mask_feather`: the feathered masks, u8 [B][H][W]: what `mask_latent` and `mask_blend` read
        self.ref_u8 = None           # `ref_mode`: the reference image
        self._ref_epoch = None       # ... and which reference image of the pipeline `ref_u8` holds (VideoSDPipeline sets it)
        self.noise = None            # the host draws on the device (None: `device_seed`)
        self.noise_ref = None        # `ref_mode`: the draws of the reference latents
        self.seed_dev = None         # `device_seed`: one seed per frame of the launch
        self._seed_host = None       # ... and its pinned mirror
        self.frame_prompts = False   # `pblock` is a per-frame block (FramePromptLayout)
        self.frame_options = False   # strength / controlnet_scale per frame of the launch (`use_options`)
        self.fo_layout = None        # `frame_options`: the OptionLayout of this engine's own block, one slot per frame
        self.fo_buf = None           # ... the block
        self._option_slots = None    # ... its FrameSlots: the OptionEntry each slot holds
        self._want_opts = None       # `use_options`: (OptionEntry, controlnet_scale) per frame (None: the plan's own options for every frame)
        self.fo_scale = None         # `frame_options` with a ControlNet: fp32 [B][16] residual scales per frame
        self._fo_scale_host = None   # ... their pinned mirror
        self._fo_scale_last = None   # ... and what was last uploaded
        self._merge_tabs = []        # the segment tables of the recorded `cn_merge_frames` calls (their addresses are in the graph)
        self._cn_scale_consts = None  # the default program's fp32 [nres] residual scales, a view of shared["consts"]
        self._twin_now = False       # this plan's one-stream form runs the encoders in lock step
        self._i420_queued = False    # `rgb_to_i420` of `out_u8` is already queued behind the last launch

    def make_slot(self, share_plan: bool = True, lane: Optional[int] = None) -> "Engine":
        """A further engine on the same GPU and the same weights, with its own streams, arena, I/O buffers, prompt constants
        and graph.
        share_plan=True: a further frame in flight of THIS engine's plan -- shares its schedule constants (`update_options`
        on the parent reaches it).  Call `prepare` on the parent first, then on the slot with the same arguments.  (The
        reference keeps one frame in flight per Ray actor; frames are independent, so a second one fills the gaps the
        first leaves between its small dependent kernels.)
        share_plan=False: an independent plan (another frame size / step count / session) with constants of its own: it is
        prepared and updated like a parent, while the other plans keep running (server.py:90-93: options are per session,
        every session's frames go through the same actors).
        lane: the launch lane whose streams the engine uses (HipOps.clone; default: the next unused lane).  Engines of one lane
        take turns on its streams, engines of different lanes run side by side."""
        e = copy.copy(self)  # what a family shares ...
        e.ops = self.ops.clone(lane)
        e._reset_own_state()  # ... and nothing of what is this engine's own
        e.is_slot = bool(share_plan)
        if not share_plan:
            e.shared = {}
        return e

    # ---------------------------------------------------------------- prompt-dependent constants
    def _networks(self, use_controlnet: bool = True):
        """(name, net) of the networks in play: the UNet, and the ControlNet when it is loaded and the plan uses it"""
        return [("unet", self.unet)] + ([("cn", self.cn)] if use_controlnet and self.cn is not None else [])

    def _nets(self):
        return [net for _name, net in self._networks()]

    def build_prompt(self, embeds: torch.Tensor) -> PromptBlock:
        """embeds: [77, cross_dim] (or [1,77,cross_dim]) -> a fresh PromptBlock: cross-attention K and V^T of every layer (the
        to_k / to_v projections diffusers recomputes every step, attn2 of each block) and, for the wide blocks, the query /
        output weights with K / V folded in (vsd_xattn_fold) -- all on the GPU (~1 ms), touching nothing a running launch
        reads: a prompt cache is filled while frames of other prompts are in flight."""
        ops = self.ops
        e = embeds.reshape(-1, embeds.shape[-1]).to(torch.float16).contiguous()
        text = ops.to_device(e)
        tl = text.shape[0]
        # one layout OBJECT per text length for the whole family: prepared plans and cached prompt blocks compare layouts by
        # identity, so a 77 -> other -> 77 sequence of prompt lengths must come back to the first object
        lays = self.family.setdefault("layouts", {})
        lay = lays.get(tl)
        if lay is None:
            lay = lays[tl] = PromptLayout(self._nets(), tl)
        self.family["layout"] = lay
        blk = PromptBlock(ops, lay)
        blk.text = text
        self._fill_prompt(blk)
        return blk

    def _fill_prompt(self, blk: PromptBlock):
        """the constants of `blk.text` under the weights as they are now, into `blk` (a fresh block, or one built before a LoRA scale change)"""
        ops, lay, text = self.ops, blk.layout, blk.text
        tl = lay.tl
        for ni, net in enumerate(self._nets()):
            for bi, t in enumerate(net.transformers):
                c = t.kv2.n // 2
                k, vt = blk.kv(ni, bi)
                ops.conv(text, None, Geom.linear(tl), t.kv2, k, ldo=c, out_t=vt, ldt=lay.ldt, t_col0=c)
                if (ni, bi) in lay.absorbed:
                    wq, ga, be = t.xa_raw
                    heads = net.cfg.heads_for(c)
                    ops.xattn_fold(k, vt, tl, wq, t.out2.weight, ga, be, c, heads, (c // heads) ** -0.5, blk.view(ni, bi, "xa1_w"),
                                   blk.view(ni, bi, "xa1_s"), blk.view(ni, bi, "xa1_t"), blk.view(ni, bi, "xa2_w"))
                    ops.copy_(blk.view(ni, bi, "xa2_b"), t.out2.bias)
        ops.synchronize()
        blk.epoch = self.family.get("weights_epoch", 0)

    def set_text_embeds(self, embeds: torch.Tensor):
        """The prompt of this engine AND of every engine made from it that was not given one of its own (`use_prompt`).
        Prepared plans stay valid: an engine copies the new constants over its own block before its next launch."""
        blk = self.build_prompt(embeds)
        self.family["prompt"] = blk
        self._want = None
        self.text = blk.text

    def use_prompt(self, blk: Optional[PromptBlock]):
        """This engine's launches use `blk` (from `build_prompt`, e.g. a prompt cache entry) from the next launch on, whatever
        the other engines of the family run; None: follow the family default again.  Call it with no launch of THIS engine
        in flight (the other lanes are not affected: every engine reads its own copy).
        `blk` may be a PromptMix of such blocks (include/vsd.h THE PROMPT MIX): the engine then forms the mix in its own block by ONE
        `prompt_mix` launch where a block takes one copy -- stream-ordered, no allocation, nobody waits; the same mix again costs nothing."""
        self._want = blk
        self._want_list = None

    def use_prompts(self, blks):
        """`frame_prompts` engines: frame i of this engine's launches uses blks[i] (one `build_prompt` result per frame of the launch, e.g.
        prompt cache entries; the same object may appear several times) from the next launch on.  Only the frame slots whose entry
        changed since this engine's last launch are rewritten, each by one `prompt_install` launch on the engine's own stream ahead of the
        program: nothing is re-captured, nobody waits.  Call it with no launch of THIS engine in flight.
        An entry may be a PromptMix: its slot is then written by one `prompt_mix` launch."""
        self._want_list = list(blks)
        self._want = None

    def _frame_sources(self, batch: int):
        """frame_prompts: the PromptBlock of every frame of a launch of `batch` frames, checked (count, one text length)"""
        want = self._want_list
        if want is None:
            d = self._want if self._want is not None else self.family.get("prompt")
            if d is None:
                raise RuntimeError("set_text_embeds (or use_prompt / use_prompts) must be called before a launch")
            want = [d] * batch
        if len(want) != batch:
            raise ValueError(f"use_prompts: {len(want)} prompt(s) for a launch of {batch} frame(s)")
        if any(b.layout.tl != want[0].layout.tl for b in want):
            raise ValueError(f"all frames of a launch must have the same text length, got {[b.layout.tl for b in want]}")
        return want

    def _seg_table(self, src, dst, mix: bool = False):
        """(device table, segments) of `prompt_install` for this pair of layouts -- a prompt into a per-frame prompt block, an option entry
        into a per-frame option block -- or, `mix`, of `prompt_mix` (a mix of prompts into a block of their own layout, or into a per-frame
        prompt block): built once per family"""
        tabs = self.family.setdefault("mix_tables" if mix else "seg_tables", {})
        got = tabs.get((src, dst))
        if got is None:
            segs = mix_segments(src, dst) if mix else (option_segments if isinstance(dst, OptionLayout) else prompt_segments)(src, dst)
            got = tabs[(src, dst)] = (self.ops.to_device(torch.tensor(segs, dtype=torch.int64)), len(segs))
            self.ops.synchronize()  # (the other lanes' streams read it too)
            if mix and hasattr(self.ops, "prompt_mix_table"):
                self.ops.prompt_mix_table(*got)  # (the library's one-time check of the table, here and not under a frame)
        return got

    def _mix_tables(self, src_layout):
        """`prepare`: the segment table a PromptMix of prompts of `src_layout` would need for this engine's block, built now, so that the
        first mix of a stream finds it (no upload, no synchronise under a frame).  Nothing without the op `prompt_mix`."""
        if hasattr(self.ops, "prompt_mix") and src_layout is not None:
            tab, nseg = self._seg_table(src_layout, self.pblock.layout, mix=True)
            if hasattr(self.ops, "prompt_mix_table"):
                self.ops.prompt_mix_table(tab, nseg)  # (every lane's context checks a table once: this engine's does so here)

    def _sync_weights(self):
        """Ahead of a launch, after a LoRA scale change (`set_adapter_scales` moved the family's "weights_epoch"): everything derived from
        the UNet's weights outside the packed buffers is stale.  (a) The time tables the plan reads (`shared["temb"]`: time_embedding,
        cond_proj and every time_emb_proj) are written again by the first engine that launches from this `shared`; (b) option entries of a
        `frame_options` plan and (c) cached prompts (kv2, out2, to_q) are rebuilt IN PLACE, from their stored schedule / text embeddings,
        before their next use; (d) what this engine had installed of either is forgotten.  Nothing happens without adapters."""
        ep = self.family.get("weights_epoch", 0)
        if ep == 0 and self.family.get("adapters") is None:
            return
        sh = self.shared
        if not self.frame_options and "sched" in sh and sh.get("weights_epoch", 0) != ep:
            self._write_time_tables(sh["sched"], sh["sched_cn"])
        if ep != self._prompt_epoch:
            self._installed = None
            for slots in (self._prompt_slots, self._option_slots):
                if slots is not None:
                    slots.src = [None] * len(slots.src)
            self._prompt_epoch = ep
        for ent, _c in self._want_opts or ():
            if ent.epoch != ep:
                self._fill_option_entry(ent)
        sources = self._want_list if self._want_list is not None else [self._want if self._want is not None else self.family.get("prompt")]
        for src in sources:
            for b in (src.components if isinstance(src, PromptMix) else (src,)):
                if b is not None and b.epoch != ep:
                    if b.text is None:
                        raise RuntimeError("a prompt block without its text embeddings cannot follow a LoRA scale change: build it with build_prompt")
                    self._fill_prompt(b)

    def _sync_prompt(self):
        self._sync_weights()
        if self.frame_prompts:
            want = self._frame_sources(self.batch)
            lay = self.pblock.layout
            if want[0].layout.tl != lay.tl:
                raise ValueError(f"the prompts' text length ({want[0].layout.tl}) differs from the one this plan was prepared for ({lay.tl}): prepare again")
            self._prompt_slots.install(self.ops, want, self._seg_table)
            return
        src = self._want if self._want is not None else self.family.get("prompt")
        if src is None:
            raise RuntimeError("set_text_embeds (or use_prompt) must be called before a launch")
        if not same_source(src, self._installed):
            if self.pblock is None or src.layout is not self.pblock.layout:
                raise RuntimeError("the prompt's text length differs from the one this plan was prepared for: prepare again")
            if isinstance(src, PromptMix):  # ONE launch on this engine's own stream in place of the copy
                if not hasattr(self.ops, "prompt_mix"):
                    raise ValueError("a prompt mix needs the op prompt_mix, which this ops object does not have")
                tab, nseg = self._seg_table(src.layout, self.pblock.layout, mix=True)
                self.ops.prompt_mix([c.buf for c in src.components], src.weights, self.pblock.buf, tab, nseg, 0)
            else:
                self.ops.copy_(self.pblock.buf, src.buf)  # one device-to-device copy on this engine's own stream
            self._installed = src

    # ---------------------------------------------------------------- LoRA adapters (include/vsd.h THE ADAPTER FUSE)
    def _family_idle(self, what: str):
        n = len(self.family.get("in_flight", ()))
        if n:
            raise RuntimeError(f"cannot {what} while {n} launch(es) of this family of engines are in flight: collect them first")

    def load_adapters(self, adapters, w_unet):
        """adapters: 1..4 lora.Adapter (lora.load_adapter / lora.parse_adapter); w_unet: the checkpoint dict this family's UNet was built
        from (the base copies are taken from it, for the tensors some adapter touches and no others).  Builds the base copies and the
        segment table once; every scale starts at 0, so nothing changes until `set_adapter_scales`.  The ControlNet is never adapted.
        A checkpoint that lives on the device is aliased by the packed buffers whose layout needs no change, so a later fuse rewrites
        those entries of `w_unet` in place: the base copies are taken here, before that, and `w_unet` is not looked at again."""
        from .lora import AdapterSet

        if self.family.get("adapters") is not None:
            raise RuntimeError("adapters are loaded already: unload_adapters() first")
        if not hasattr(self.ops, "lora_fuse"):
            raise ValueError("LoRA adapters need the op lora_fuse, which this ops object does not have")
        self._family_idle("load adapters")
        aset = AdapterSet(self.ops, self.unet, w_unet, adapters)
        self.ops.lora_fuse_table(aset.table, aset.nseg)
        self.family["adapters"] = aset
        return aset

    def set_adapter_scales(self, scales):
        """One launch on this engine's stream: every adapted tensor's fused weight from its base copy, straight into the packed buffers the
        recorded programs read by address -- nothing is re-captured, no plan is lost.  Always computed from the base copies: no drift, no
        dependence on the scales before.  The weights are shared by every engine of the family, so none of them may have a launch in
        flight.  Time tables, option entries and cached prompts follow lazily (`_sync_weights`)."""
        aset = self.family.get("adapters")
        if aset is None:
            raise RuntimeError("no adapters are loaded: load_adapters first")
        sc = tuple(float(x) for x in scales)
        if len(sc) != len(aset.adapters) or not all(np.isfinite(x) for x in sc):
            raise ValueError(f"set_adapter_scales: {len(aset.adapters)} finite scale(s) wanted, one per loaded adapter, got {list(scales)!r}")
        self._family_idle("change a LoRA scale")
        self.ops.lora_fuse(aset.table, aset.nseg, sc)
        if not any(sc):
            aset.restore_fold(self.ops)
        self.ops.synchronize()  # (the other lanes' streams read these weights)
        aset.scales = sc
        self.family["weights_epoch"] = self.family.get("weights_epoch", 0) + 1

    def unload_adapters(self):
        """the load-time bytes back (a fuse with every scale zero, the fold vectors by copy), then the base copies and the table freed"""
        aset = self.family.get("adapters")
        if aset is None:
            return
        self.set_adapter_scales((0.0,) * len(aset.adapters))
        self.ops.lora_fuse_table(aset.table, 0)
        self.family["adapters"] = None

    # ---------------------------------------------------------------- per-frame options
    def _nres(self) -> int:
        return 13 if self.cn is None else len(self.cn.zero_convs) + 1

    def _option_cols(self, use_controlnet: bool) -> Dict[str, int]:
        return {name: net.temb_proj.n for name, net in self._networks(use_controlnet)}

    def option_entry(self, strength: float, steps: int, use_controlnet: bool = True) -> OptionEntry:
        """The constants of the schedule `(strength, steps)` as a cache entry, keyed by its TIMESTEPS (`lcm_timesteps` maps many strengths
        to one tuple): scheduler coefficients and both time tables in one device buffer, built once (~1 ms on the GPU: the ~10 tiny
        GEMMs of the time path) and kept in an LRU cache every engine of the family shares.  Touches nothing a running launch reads."""
        sched = LCMSchedule(strength, steps)
        key = (tuple(int(t) for t in sched.timesteps), bool(use_controlnet))
        cache = self.family.setdefault("option_entries", OrderedDict())
        ent = cache.get(key)
        if ent is None:
            n = len(sched)
            lays = self.family.setdefault("option_layouts", {})  # (one layout OBJECT per (steps, networks): the copy lists are per pair)
            lay = lays.get((n, bool(use_controlnet)))
            if lay is None:
                lay = lays[(n, bool(use_controlnet))] = OptionLayout(n, self._option_cols(use_controlnet), 1)
            buf = self.ops.zeros(lay.nbytes, dtype=torch.uint8)
            vals = schedule_constants(sched)
            host = torch.zeros(lay.coef_stride, dtype=torch.float32)
            host[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
            self.ops.upload(lay.view(buf, "coef"), host)
            ent = cache[key] = OptionEntry(lay, buf, key[0])
            ent.sched, ent.cn = sched, bool(use_controlnet)
            self._fill_option_entry(ent)
            self.family["option_builds"] = self.family.get("option_builds", 0) + 1
            while len(cache) > max(1, int(self.family.get("max_option_entries", MAX_OPTION_ENTRIES))):
                cache.popitem(last=False)  # least recently used first; an engine (or a launch's handle) that still holds it keeps it alive
        else:
            cache.move_to_end(key)
            if ent.epoch != self.family.get("weights_epoch", 0):  # built before a LoRA scale change
                self._fill_option_entry(ent)
        return ent

    def _fill_option_entry(self, ent: OptionEntry):
        """the time tables of an option entry from the weights as they are now (a fresh entry, or IN PLACE one built before a LoRA scale
        change: the family is idle then, and every engine installs it again)"""
        for name, net in self._networks(ent.cn):
            self._time_embeddings(net, ent.sched, ent.layout.view(ent.buf, name))
        self.ops.synchronize()  # (the other lanes' streams read it too)
        ent.epoch = self.family.get("weights_epoch", 0)

    def use_options(self, pairs):
        """`frame_options` engines: frame i of this engine's launches runs with pairs[i] = (strength, controlnet_scale) from the next launch
        on.  Every strength must give the plan's NUMBER of timesteps (another number is another program), else ValueError.  A frame slot
        whose timesteps changed since this engine's last launch is rewritten by ONE `prompt_install` launch on the engine's own stream ahead
        of the program; the ControlNet scales go from a pinned mirror with one stream-ordered copy, when any changed.  Unchanged slots cost
        nothing; nothing is re-captured, nobody waits.  Call it with no launch of THIS engine in flight."""
        if not self.frame_options or self.plan is None:
            raise ValueError("use_options needs an engine prepared with frame_options=True (a default plan takes update_options)")
        pairs = [(float(s), float(c)) for s, c in pairs]
        B, n, steps = self.plan["batch"], self.plan["n"], self.plan["steps"]
        if len(pairs) != B:
            raise ValueError(f"use_options: {len(pairs)} option pair(s) for a launch of {B} frame(s)")
        from .lcm import lcm_timesteps

        counts = [len(lcm_timesteps(s, steps)) for s, _c in pairs]
        if any(k != n for k in counts):
            raise ValueError(f"use_options: every frame of this plan runs {n} timestep(s) (steps={steps}); the strengths "
                             f"{[s for s, _c in pairs]} give {counts}: another number of timesteps is another program")
        self._want_opts = [(self.option_entry(s, steps, self.plan["cn"]), c) for s, c in pairs]

    def _sync_options(self):
        """ahead of a launch of a `frame_options` engine: the frame slots whose entry changed, and the scales when any changed"""
        if not self.frame_options:
            return
        p = self.plan
        want = self._want_opts
        if want is None:
            want = self._want_opts = [(self.option_entry(p["strength"], p["steps"], p["cn"]), float(p["cn_scale"]))] * p["batch"]
        self._option_slots.install(self.ops, [ent for ent, _c in want], self._seg_table)
        if self.fo_scale is not None:
            nres = self._nres()
            scales = [tuple(controlnet_scales(nres, c).tolist()) for _e, c in want]
            if scales != self._fo_scale_last:
                host = self._fo_scale_host
                host.zero_()
                host[:, :nres] = torch.tensor(scales, dtype=torch.float32)
                self.ops.upload(self.fo_scale, host)  # (the lane's previous launch has been collected: nothing in flight reads the mirror)
                self._fo_scale_last = scales

    def set_added_cond(self, pooled: torch.Tensor, time_ids):
        """SDXL micro-conditioning: pooled text embedding [add_pooled_dim] and the 6 time ids
        (orig_h, orig_w, crop_top, crop_left, target_h, target_w).  Takes effect at the next `prepare`."""
        self.added = (pooled.detach().float().cpu().reshape(-1), [float(v) for v in time_ids])

    # ---------------------------------------------------------------- schedule-dependent constants
    def _time_embeddings(self, net: NetWeights, sched: LCMSchedule, out: torch.Tensor, use_cond: bool = True):
        """out[i] = concat over ResnetBlocks of time_emb_proj(SiLU(time_embedding(t_i))) + conv1.bias.
        Replaces Timesteps/TimestepEmbedding + every ResnetBlock2D.time_emb_proj (K9 in SURVEY.md)."""
        ops, cfg = self.ops, net.cfg
        n = len(sched)
        c0 = cfg.block_out_channels[0]
        t_emb = ops.to_device(timestep_sinusoid(sched.timesteps, c0).half())
        x = t_emb
        if net.cond_proj is not None and use_cond:  # (the reference-only WRITE pass passes no timestep_cond)
            wemb = ops.to_device(w_embedding(self.guidance_scale, cfg.cond_proj_dim).half().expand(n, -1).contiguous())
            x = ops.empty(n, c0)
            ops.conv(wemb, None, Geom.linear(n), net.cond_proj, x, residual=t_emb)
        h1 = ops.empty(n, cfg.temb_dim)
        ops.conv(x, None, Geom.linear(n), net.time_l1, h1, act=L.ACT_SILU)
        h2 = ops.empty(n, cfg.temb_dim)
        if net.add_l1 is not None:
            # SDXL text_time conditioning: temb += add_embedding(cat[pooled text embeds, sinusoids of the 6 time ids])
            # (UNet2DConditionModel.get_aug_embed); the same vector for every step
            if self.added is None:
                raise RuntimeError("this UNet needs set_added_cond(pooled, time_ids) before prepare")
            pooled, time_ids = self.added
            tid = timestep_sinusoid([float(v) for v in time_ids], cfg.add_time_dim).reshape(1, -1)
            a0 = ops.to_device(torch.cat([pooled.float().reshape(1, -1), tid], dim=-1).half().expand(n, -1).contiguous())
            a1 = ops.empty(n, cfg.temb_dim)
            ops.conv(a0, None, Geom.linear(n), net.add_l1, a1, act=L.ACT_SILU)
            aug = ops.empty(n, cfg.temb_dim)
            ops.conv(a1, None, Geom.linear(n), net.add_l2, aug)
            ops.conv(h1, None, Geom.linear(n), net.time_l2, h2, residual=aug, act=L.ACT_SILU | L.ACT_POST)
        else:
            ops.conv(h1, None, Geom.linear(n), net.time_l2, h2, act=L.ACT_SILU)  # SiLU(temb): all consumers apply it
        ops.conv(h2, None, Geom.linear(n), net.temb_proj, out[:n])
        ops.synchronize()

    def _temb(self, net):
        """this plan's per-step time-embedding projections of `net` (device constants shared by the plan's engines)"""
        return self.shared["temb"]["cn" if net is self.cn else "unet"]

    # ---------------------------------------------------------------- network builders (record ops)
    def _resnet(self, r, rw: ResnetW, net, step, x, x2, c0, c1, hw, geom, out=None, out2=None, add2=None, residual2=None,
                temb=None, stat_out=None):
        """x (and optional concat partner x2) -> ResnetBlock2D output [batch*hw][cout]  (hw = pixels per image).
        temb: another time-projection table than the plan's; stat_out: fp32 [cout][2] to receive the output's per-channel
        (sum, sumsq) (reference-only AdaIN)."""
        a, cfg = self.arena, net.cfg
        cin = c0 + c1
        rows = self.batch * hw
        t1 = a.alloc(rows, cin)
        self._gn(r, x, x2, c0, c1, hw, cfg.groups, 1e-5, rw.n1[0], rw.n1[1], True, t1)
        h = a.alloc(rows, rw.cout)
        fo = self.frame_options  # conv1 without the time vector; norm2 adds the FRAME's slice of the time table to its input instead
        if fo:
            tab = self.fo_layout.view(self.fo_buf, "cn" if net is self.cn else "unet")  # frame 0's table: frame b's lies ld_tv halfs further
            tv, ld_tv = tab[step, rw.temb_off:rw.temb_off + rw.cout], tab.numel()
        else:
            tv = (self._temb(net) if temb is None else temb)[step, rw.temb_off:rw.temb_off + rw.cout]
        c1kw = {} if fo else dict(rowvec=tv)
        sc = x
        # The shortcut conv (ResnetBlock2D.conv_shortcut: 16 per denoising step with the ControlNet) depends on the block's INPUT only:
        # it shares conv1's grid (vsd_conv_gemm_group, every member at the split it has as a launch of its own: same bits) instead of
        # being one more dependent launch between norm2 and conv2 -- 64 launches of a 4-step frame less.
        grouped = (rw.shortcut is not None and self.group_shortcuts and hasattr(self.ops, "conv_group") and
                   cin % 64 == 0 and c0 % 64 == 0 and c1 % 64 == 0 and rw.cout % 64 == 0 and (geom.hi, geom.wi) == (geom.hs, geom.ws))
        if grouped:
            sc = a.alloc(rows, rw.cout)
            r.conv_group([((t1, None, geom, rw.conv1, h), c1kw),
                          ((x, x2, Geom.linear(rows), rw.shortcut, sc), dict(c0=c0, c1=c1))], split="own")
        else:
            r.conv(t1, None, geom, rw.conv1, h, **c1kw)
        t2 = a.alloc(rows, rw.cout)
        if fo:
            r.groupnorm_addvec(h, tv, ld_tv, rw.cout, hw, cfg.groups, 1e-5, rw.n2[0], rw.n2[1], True, t2, batch=self.batch)
        else:
            self._gn(r, h, None, rw.cout, 0, hw, cfg.groups, 1e-5, rw.n2[0], rw.n2[1], True, t2)
        if rw.shortcut is not None and not grouped:
            sc = a.alloc(rows, rw.cout)
            r.conv(x, x2, Geom.linear(rows), rw.shortcut, sc, c0=c0, c1=c1)
        out = out if out is not None else a.alloc(rows, rw.cout)
        r.conv(t2, None, geom, rw.conv2, out, residual=sc, residual2=residual2, out2=out2, add2=add2,
               chanstat_out=stat_out)
        return out

    def _transformer(self, r, tw: TransformerW, net, x, hw, out2=None, add2=None, ref: Optional[RefCtx] = None, stat_out=None):
        a, cfg = self.arena, net.cfg
        c = tw.c
        heads = cfg.heads_for(c)
        d = c // heads
        B = self.batch
        rows = B * hw                      # the token matrix of all images in flight: [B*hw][C]
        lin = Geom.linear(rows)
        t = a.alloc(rows, c)
        self._gn(r, x, None, c, 0, hw, cfg.groups, 1e-6, tw.norm[0], tw.norm[1], False, t)
        # The three LayerNorms are never materialised: every producer of the token stream leaves per-row
        # (sum, sumsq) partials (rowstat_out) and the consuming GEMM applies the norm in its epilogue (ln_part).
        ng = c // 64
        stat = lambda: a.alloc(rows, ng * 2, dtype=torch.float32).view(rows, ng, 2)  # noqa: E731
        h = a.alloc(rows, c)
        rs = stat()
        r.conv(t, None, lin, tw.proj_in, h, rowstat_out=rs)
        t_img = _ru(hw, 64)                # V^T columns per image (key padding stays zero)
        ldvt = B * t_img
        for bi, bw in enumerate(tw.blocks):
            # self-attention (per image: keys never cross an image boundary)
            att = a.alloc(rows, c)
            if ref is None:
                qk = a.alloc(rows, 2 * c)
                vt = self._vt_buffer(c, ldvt)
                r.conv(h, None, Geom.linear(hw, batch=B), bw.qkv, qk, ldo=2 * c, out_t=vt, ldt=ldvt, t_col0=2 * c, ln_part=rs,
                       t_img=t_img)
                r.attention(qk, 2 * c, qk[:, c:], 2 * c, vt, ldvt, att, c, hw, hw, heads, d, d ** -0.5, batch=B, k_brows=hw,
                            vt_bcols=t_img)
            else:
                # reference-only: K rows / V^T columns [0, hw) belong to the frame (read pass), [hw, 2 hw) to the reference
                # (write pass); the read pass attends over all 2 hw keys (lcm_reference_pipeline.py:535-539)
                if ref.mode == "write":
                    # the write pass reads whole 64-key tiles from column hw on: the row must hold hw + ru(hw, 64) columns
                    # so that its masked tail keys are this buffer's zero padding, not the next row's read-pass columns
                    # (masked probabilities are 0, but 0 x a stale Inf/NaN is NaN in the PV product)
                    ld2 = _ru(hw + _ru(hw, 64), 64)
                    ref.kv[bw.kv_index] = (a.alloc(2 * hw, 2 * c), self._vt_buffer(c, ld2))
                qk_full, vt_full = ref.kv[bw.kv_index]
                ld2 = vt_full.shape[1]
                off = hw if ref.mode == "write" else 0
                qk = qk_full[off:off + hw]
                r.conv(h, None, Geom.linear(hw), bw.qkv, qk, ldo=2 * c, out_t=vt_full[:, off:], ldt=ld2, t_col0=2 * c, ln_part=rs)
                if ref.mode == "write":
                    r.attention(qk, 2 * c, qk[:, c:], 2 * c, vt_full[:, off:], ld2, att, c, hw, hw, heads, d, d ** -0.5)
                else:
                    r.attention(qk, 2 * c, qk_full[:, c:], 2 * c, vt_full, ld2, att, c, hw, 2 * hw, heads, d, d ** -0.5)
            ni = 1 if net is self.cn else 0
            kt, vtt = self.pblock.kv(ni, bw.kv_index)
            xa = self.pblock.xa(ni, bw.kv_index) if self.absorb_cross_attention else None  # (a per-frame block has none: explicit form)
            fused = (self.use_fused_tail and c == getattr(self.ops, "TAIL_C", 0) and len(tw.blocks) == 1 and ref is None and
                     stat_out is None and out2 is None and hasattr(self.ops, "tail_a"))
            if fused:
                # the block's per-token chains as fused launches around the cross-attention (csrc/fused_tail.hip): the token
                # tile's owner streams only the weights; h1 / q (and in tail_b h2, the GEGLU hidden state, h3) stay on chip.
                # Measured on MI355X (us, fused vs the launches it replaces; the library picks the tile height per token count):
                # tail_a 10 vs 19 at 4096 tokens, 15 vs 31 at 12288, 21 vs 53 at 20480; tail_b 44 vs 59 at 4096 (every
                # workgroup streams all 2.9 MB of feed-forward weights whatever the token count), 61 vs 111 at 12288,
                # 91 vs 214 at 20480.  Below ~2048 tokens (small frames) the separate launches win.
                h1 = a.alloc(rows, c)
                q = a.alloc(rows, c)
                r.tail_a(att, h, rows, bw.out1, bw.q2, h1, q)
                self._cross_attention(r, q, kt, vtt, att, c, hw, heads, d)
                if rows >= self.tail_b_min_rows:
                    out = a.alloc(rows, c)
                    r.tail_b(att, h1, x, rows, bw.out2, bw.ff1, bw.ff2, tw.proj_out, out)
                    return out
                h2 = a.alloc(rows, c)
                rs2 = stat()
                r.conv(att, None, lin, bw.out2, h2, residual=h1, rowstat_out=rs2)
                f = a.alloc(rows, 4 * c)
                r.conv(h2, None, lin, bw.ff1, f, ln_part=rs2)
                h3 = a.alloc(rows, c)
                r.conv(f, None, lin, bw.ff2, h3, residual=h2)
                h = h3
                continue
            h1 = a.alloc(rows, c)
            rs1 = stat()
            r.conv(att, None, lin, bw.out1, h1, residual=h, rowstat_out=rs1)
            # cross-attention over the cached text K / V^T (shared by all images)
            h2 = a.alloc(rows, c)
            rs2 = stat()
            if xa is not None:
                # wide blocks: probabilities = softmax per head of LN(h1) G^T (one 128-column tile per head, softmax in the
                # GEMM epilogue), then h2 = P Z^T + bias + h1 -- two launches instead of three, fewer FLOPs for C >= 1024
                pr = a.alloc(rows, xa[0].n)
                r.conv(h1, None, lin, xa[0], pr, ln_part=rs1, act=L.ACT_SOFTMAX, softmax_cols=kt.shape[0])
                r.conv(pr, None, lin, xa[1], h2, residual=h1, rowstat_out=rs2)
            else:
                q = a.alloc(rows, c)
                r.conv(h1, None, lin, bw.q2, q, ln_part=rs1)
                self._cross_attention(r, q, kt, vtt, att, c, hw, heads, d)
                r.conv(att, None, lin, bw.out2, h2, residual=h1, rowstat_out=rs2)
            # GEGLU feed-forward
            f = a.alloc(rows, 4 * c)
            r.conv(h2, None, lin, bw.ff1, f, ln_part=rs2)
            h3 = a.alloc(rows, c)
            last = bi == len(tw.blocks) - 1
            rs = None if last else stat()  # the next block's norm1 statistics
            r.conv(f, None, lin, bw.ff2, h3, residual=h2, rowstat_out=rs)
            h = h3
        out = a.alloc(rows, c)
        r.conv(h, None, lin, tw.proj_out, out, residual=x, out2=out2, add2=add2,
               chanstat_out=stat_out)
        return out

    def _cross_attention(self, r, q, kt, vtt, att, c, hw, heads, d):
        """q [B*hw][c] over the text's K / V^T: shared by all images of the launch (the queries are one problem of B*hw rows), or -- a
        per-frame block -- image b over ITS rows of K and columns of V^T (one problem per image, as self-attention)"""
        if self.frame_prompts:
            lay = self.pblock.layout
            r.attention(q, c, kt, c, vtt, vtt.shape[1], att, c, hw, lay.tl, heads, d, d ** -0.5, batch=self.batch, k_brows=lay.tl,
                        vt_bcols=lay.ldt)
        else:
            r.attention(q, c, kt, c, vtt, vtt.shape[1], att, c, self.batch * hw, kt.shape[0], heads, d, d ** -0.5)

    def _gn(self, r, x, x2, c0, c1, hw, groups, eps, gamma, beta, silu, out):
        # (round 1-2 could also take the statistics from the producing conv's epilogue (chanstat_out): slower than the separate,
        #  overlappable statistics kernel on MI355X, removed in round 3 -- chanstat_out remains for the reference-only AdaIN)
        r.groupnorm(x, x2, c0, c1, hw, groups, eps, gamma, beta, silu, out, batch=self.batch)

    def _vt_buffer(self, c, ldvt):
        # V^T buffers live outside the rewound arena: their key-padding columns must stay zero forever
        key = (c, ldvt, self._vt_count)
        self._vt_count += 1
        buf = self._vt_pool.get(key)
        if buf is None:
            buf = self.ops.zeros(c, ldvt)
            self._vt_pool[key] = buf
        return buf

    def _ref_site(self, r, ref: Optional[RefCtx], kind, i, j, c):
        """-> stat buffer the block's last conv must fill (or None) for the reference-only AdaIN at this block output"""
        if ref is None or not ref.gate(kind, i):
            return None
        st = self.arena.alloc(c, 2, dtype=torch.float32)
        if ref.mode == "write":
            ref.stats[(kind, i, j)] = st
        return st

    def _ref_adain(self, r, ref: Optional[RefCtx], kind, i, j, h, st, rows, c):
        """read pass: AdaIN the block output to the statistics the write pass banked for the same site"""
        if ref is None or st is None or ref.mode != "read" or (kind, i, j) not in ref.stats:
            return h
        o = self.arena.alloc(rows, c)
        r.adain(h, st, ref.stats[(kind, i, j)], rows, c, o)
        return o

    def _down_mid(self, r, net: NetWeights, step, h, sizes, ref: Optional[RefCtx] = None, temb=None):
        """conv_in output h -> (mid block output, skip list [(tensor, channels, level)])."""
        a = self.arena
        ch = net.cfg.block_out_channels
        skips = []
        for i, c in enumerate(ch):
            hh, ww = sizes[i]
            hw = hh * ww
            g3 = Geom.conv(hh, ww, batch=self.batch)
            for j, (rw, tw) in enumerate(net.down[i]):
                st = self._ref_site(r, ref, "down", i, j, c)
                h = self._resnet(r, rw, net, step, h, None, rw.cin, 0, hw, g3, temb=temb, stat_out=st if tw is None else None)
                if tw is not None:
                    h = self._transformer(r, tw, net, h, hw, ref=ref, stat_out=st)
                h = self._ref_adain(r, ref, "down", i, j, h, st, self.batch * hw, c)
                skips.append((h, c, i))
            ds = net.downsamplers[i]
            if ds is not None:
                h2, w2 = sizes[i + 1]
                o = a.alloc(self.batch * h2 * w2, c)
                r.conv(h, None, Geom.conv(hh, ww, stride=2, batch=self.batch), ds, o)
                h = o
                skips.append((o, c, i + 1))
        hh, ww = sizes[-1]
        hw = hh * ww
        g3 = Geom.conv(hh, ww, batch=self.batch)
        c = ch[-1]
        h = self._resnet(r, net.mid[0], net, step, h, None, c, 0, hw, g3, temb=temb)
        h = self._transformer(r, net.mid[1], net, h, hw, ref=ref)
        st = self._ref_site(r, ref, "mid", 0, 0, c)
        h = self._resnet(r, net.mid[2], net, step, h, None, c, 0, hw, g3, temb=temb, stat_out=st)
        h = self._ref_adain(r, ref, "mid", 0, 0, h, st, self.batch * hw, c)
        return h, skips

    def _unet_encoder(self, r, step, lat, sizes, ref: Optional[RefCtx] = None, temb=None):
        a, net = self.arena, self.unet
        ch = net.cfg.block_out_channels
        h0, w0 = sizes[0]
        x = a.alloc(self.batch * h0 * w0, ch[0])
        r.conv(lat, None, Geom.conv(h0, w0, batch=self.batch), net.conv_in, x)
        h, skips = self._down_mid(r, net, step, x, sizes, ref=ref, temb=temb)
        return h, [(x, ch[0], 0)] + skips

    def _unet_decoder(self, r, step, h, skips, sizes, eps_out, ref: Optional[RefCtx] = None, temb=None):
        a, net = self.arena, self.unet
        ch = net.cfg.block_out_channels
        h0, w0 = sizes[0]
        hw0 = h0 * w0
        skips = list(skips)
        nlev = len(ch)
        cprev = ch[-1]
        for i in range(nlev):
            lvl = nlev - 1 - i
            hh, ww = sizes[lvl]
            hw = hh * ww
            g3 = Geom.conv(hh, ww, batch=self.batch)
            for j, (rw, tw) in enumerate(net.up[i]):
                s, sc, slvl, *ev = skips.pop()
                assert slvl == lvl and rw.cin == cprev + sc, (slvl, lvl, rw.cin, cprev, sc)
                if ev and ev[0]:
                    r.wait(ev[0])  # this skip's ControlNet merge ran on the second stream
                st = self._ref_site(r, ref, "up", i, j, rw.cout)
                h = self._resnet(r, rw, net, step, h, s, cprev, sc, hw, g3, temb=temb, stat_out=st if tw is None else None)
                cprev = rw.cout
                if tw is not None:
                    h = self._transformer(r, tw, net, h, hw, ref=ref, stat_out=st)
                h = self._ref_adain(r, ref, "up", i, j, h, st, self.batch * hw, cprev)
            up = net.upsamplers[i]
            if up is not None:
                h2, w2 = sizes[lvl - 1]
                o = a.alloc(self.batch * h2 * w2, cprev)
                # nearest resize to the next skip's size folded into the conv's gather (Upsample2D)
                r.conv(h, None, Geom.conv(hh, ww, up_to=(h2, w2), batch=self.batch), up, o)
                h = o
        t = a.alloc(self.batch * hw0, ch[0])
        self._gn(r, h, None, ch[0], 0, hw0, net.cfg.groups, 1e-5, net.norm_out[0], net.norm_out[1], True, t)
        r.conv(t, None, Geom.conv(h0, w0, batch=self.batch), net.conv_out, eps_out, ldo=8)

    def _controlnet_encoder(self, r, step, lat, sizes, cond_emb):
        a, net = self.arena, self.cn
        ch = net.cfg.block_out_channels
        h0, w0 = sizes[0]
        x = a.alloc(self.batch * h0 * w0, ch[0])
        r.conv(lat, None, Geom.conv(h0, w0, batch=self.batch), net.conv_in, x, residual=cond_emb)
        h, skips = self._down_mid(r, net, step, x, sizes)
        return h, [(x, ch[0], 0)] + skips

    def _merges(self, cn_mid, cn_skips, u_mid, u_skips, sizes):
        """The 13 merges of a step in the order the decoder needs them -- the mid block's, then the skips' deepest first: (ControlNet
        tensor, UNet tensor, zero-conv, channels, rows, scale column, level; None for the mid block)"""
        net, B = self.cn, self.batch
        hh, ww = sizes[-1]
        yield cn_mid, u_mid, net.zero_mid, net.cfg.block_out_channels[-1], B * hh * ww, len(cn_skips), None
        for i in reversed(range(len(cn_skips))):
            (s, c, lvl), (us, uc, ulvl) = cn_skips[i], u_skips[i]
            assert (c, lvl) == (uc, ulvl)
            hh, ww = sizes[lvl]
            yield s, us, net.zero_convs[i], c, B * hh * ww, i, lvl

    def _can_group(self, todo):
        """(a grouped launch exists for the buffer-load operand path only: every merge's channel count a multiple of 64 -- the shipped
        SD1.5 / SDXL / MINI configs; a ControlNet of other widths takes the one-by-one merges: ADVICE r5)"""
        return self.group_merges and all(m[3] % 64 == 0 for m in todo) and hasattr(self.ops, "conv_group")

    @staticmethod
    def _conv_groups(r, calls, gmax=7):
        """conv calls that do not depend on each other as ONE grid per group of up to seven (vsd_conv_gemm_group), in the order given"""
        for g0 in range(0, len(calls), gmax):
            r.conv_group(calls[g0:g0 + gmax])

    def _controlnet_merge(self, r, cn_mid, cn_skips, u_mid, u_skips, sizes):
        """The 13 zero-convs, each writing UNet tensor + scale_i * (conv + bias) in one epilogue
        (ControlNetModel's guess-mode scaling, always on in the reference: lcm_controlnet.py:399,447, and the
        `down_block_additional_residuals` / `mid_block_additional_residual` adds of UNet2DConditionModel)."""
        if self.frame_options:
            return self._controlnet_merge_frames(r, cn_mid, cn_skips, u_mid, u_skips, sizes)
        a = self.arena
        todo = list(self._merges(cn_mid, cn_skips, u_mid, u_skips, sizes))
        sc = self._cn_scale_consts  # fp32 [nres] in device memory: logspace(-1, 0, nres) * controlnet_scale
        assert sc.numel() >= len(todo)
        merged = [None] * len(cn_skips)

        def merge(src, u, zc, c, rows, col, lvl):
            o = a.alloc(rows, c)
            return o, ((src, None, Geom.linear(rows), zc, o), dict(out_scale_dev=sc[col:col + 1], residual=u))

        # Only the mid-block merge is on the critical path; the decoder consumes the skips deepest first, one per ResnetBlock.
        # With the second stream free after the encoders' join, the 12 skip merges run there, in the order the decoder
        # needs them, each followed by a named event the consuming ResnetBlock waits for.
        side = self.overlap_controlnet and self.use_side_stream
        if not side and self._can_group(todo):
            # The 13 merges do not depend on each other and are small (11.5 us of a lone frame each as launches of their own: leaving
            # the 12 skip merges out of a 4-step frame takes 0.55 ms off it): ONE grid per group of up to eight of them
            # (vsd_conv_gemm_group) -- first the mid block's and the deepest skips' (what the decoder needs first), then the rest.
            calls, mid = [], None
            for m in todo:
                o, call = merge(*m)
                calls.append(call)
                if m[6] is None:
                    mid = o
                else:
                    merged[m[5]] = (o, m[3], m[6], None)
            self._conv_groups(r, calls)
            return mid, merged
        if side:
            r.signal("enc_done")
            r.use_stream(1)
            r.wait("enc_done")
        for m in todo[1:]:
            o, (aa, kk) = merge(*m)
            r.conv(*aa, **kk)
            ev = None
            if side:
                ev = f"skip{m[5]}"
                r.signal(ev)
            merged[m[5]] = (o, m[3], m[6], ev)
        if side:
            r.use_stream(0)
        mid, (aa, kk) = merge(*todo[0])
        r.conv(*aa, **kk)
        return mid, merged

    def _controlnet_merge_frames(self, r, cn_mid, cn_skips, u_mid, u_skips, sizes):
        """`frame_options`: the scale depends on the IMAGE, which an M tile of the zero-conv's GEMM does not know.  The zero-convs are
        recorded with out_scale = 1 and no residual (in the same grouped launches), and ONE `cn_merge_frames` launch then writes
        out = u + scale[image][i] * z for all 13 of them (include/vsd.h)."""
        a, B = self.arena, self.batch
        todo = list(self._merges(cn_mid, cn_skips, u_mid, u_skips, sizes))
        assert len(todo) <= L.MERGE_SEG_MAX and len(todo) <= self.fo_scale.shape[1]
        calls, segs, keep = [], [], []
        mid, merged = None, [None] * len(cn_skips)
        for src, u, zc, c, rows, col, lvl in todo:
            if c % 8:
                raise ValueError(f"frame_options: a {c}-wide ControlNet residual: rows must be whole 16-byte chunks (C a multiple of 8)")
            z, o = a.alloc(rows, c), a.alloc(rows, c)
            calls.append(((src, None, Geom.linear(rows), zc, z), {}))
            segs.append((z.data_ptr(), u.data_ptr(), o.data_ptr(), rows // B, c, col))
            keep.append((z, u, o))
            if lvl is None:
                mid = o
            else:
                merged[col] = (o, c, lvl, None)
        if self._can_group(todo):
            self._conv_groups(r, calls)
        else:
            for aa, kk in calls:
                r.conv(*aa, **kk)
        tab = self.ops.to_device(torch.tensor(segs, dtype=torch.int64))
        self._merge_tabs.append(tab)
        r.cn_merge_frames(tab, len(segs), self.fo_scale, self.fo_scale.shape[1], B, tensors=keep)
        return mid, merged

    @staticmethod
    def _zip_pairs(r, first, second):
        """two recorded call lists of one topology -> pairs; calls without a twin (another op, or one list longer) go out alone"""
        sync = Engine.SYNC_OPS
        first = [c for c in first if c[0].__name__ not in sync]
        second = [c for c in second if c[0].__name__ not in sync]
        for i in range(max(len(first), len(second))):
            a = first[i] if i < len(first) else None
            b = second[i] if i < len(second) else None
            if a is not None and b is not None and a[0].__name__ == b[0].__name__ and a[0].__name__ in ("conv", "groupnorm", "groupnorm_addvec", "attention", "tail_a", "tail_b"):
                r.pair(a, b)
            else:
                for c in (a, b):
                    if c is not None:
                        r.calls.append(c)

    def _cond_embedding(self, r, ctrl, H, W):
        a, net = self.arena, self.cn
        h, hh, ww = ctrl, H, W
        for pw, stride in net.cond_convs:
            g = Geom.conv(hh, ww, stride=stride, batch=self.batch)
            o = a.alloc(g.m, pw.n)
            r.conv(h, None, g, pw, o, act=L.ACT_SILU)
            h, hh, ww = o, g.ho, g.wo
        g = Geom.conv(hh, ww, batch=self.batch)
        o = a.alloc(g.m, net.cond_out.n)
        r.conv(h, None, g, net.cond_out, o)
        return o

    def _taesd_block(self, r, blk, x, hh, ww):
        a = self.arena
        g = Geom.conv(hh, ww, batch=self.batch)
        c = blk[0].n
        t1 = a.alloc(g.m, c)
        r.conv(x, None, g, blk[0], t1, act=L.ACT_RELU)
        t2 = a.alloc(g.m, c)
        r.conv(t1, None, g, blk[1], t2, act=L.ACT_RELU)
        o = a.alloc(g.m, c)
        r.conv(t2, None, g, blk[2], o, residual=x, act=L.ACT_RELU | L.ACT_POST)
        return o

    def _encode(self, r, img8, H, W, out):
        a, v = self.arena, self.vae
        c = v.enc_in.n
        B = self.batch
        h = a.alloc(B * H * W, c)
        r.conv(img8, None, Geom.conv(H, W, batch=B), v.enc_in, h)
        for b in v.enc_blocks0:
            h = self._taesd_block(r, b, h, H, W)
        hh, ww = H, W
        for down, bs in v.enc_stages:
            g = Geom.conv(hh, ww, stride=2, batch=B)
            o = a.alloc(g.m, c)
            r.conv(h, None, g, down, o)
            h, hh, ww = o, g.ho, g.wo
            for b in bs:
                h = self._taesd_block(r, b, h, hh, ww)
        r.conv(h, None, Geom.conv(hh, ww, batch=B), v.enc_out, out, ldo=8)

    def _decode(self, r, z8, hh, ww, out):
        a, v = self.arena, self.vae
        c = v.dec_in.n
        B = self.batch
        h = a.alloc(B * hh * ww, c)
        r.conv(z8, None, Geom.conv(hh, ww, batch=B), v.dec_in, h, act=L.ACT_RELU)
        for bs, up in v.dec_stages:
            for b in bs:
                h = self._taesd_block(r, b, h, hh, ww)
            g = Geom.conv(hh, ww, up_to=(2 * hh, 2 * ww), batch=B)  # nn.Upsample(scale_factor=2) folded into the conv
            o = a.alloc(g.m, c)
            r.conv(h, None, g, up, o)
            h, hh, ww = o, g.ho, g.wo
        h = self._taesd_block(r, v.dec_last_block, h, hh, ww)
        r.conv(h, None, Geom.conv(hh, ww, batch=B), v.dec_out, out, ldo=8)

    # ---------------------------------------------------------------- prepare: build + capture
    def autotune(self, verbose: bool = False):
        """Pick (tile, split-K, reduction form) per distinct conv shape of the recorded program by timing the
        candidates on the GPU (the hipBLASLt/MIOpen "find" step, done on our own kernel)."""
        ops = self.ops
        if not hasattr(ops, "tune_conv"):
            return {}
        seen = {}
        # throughput-mode plans: candidates are timed with four lanes busy only offline / on request (ops.tune_lanes_online);
        # otherwise a shape without a throughput-mode entry takes its alone-timed choice, timed now if that is missing too
        mode = ops.tune_mode  # (an ops object that tunes is HipOps: no probing past this point)
        online = mode == 0 or ops.tune_lanes_online
        try:
            # the two-stream form first: a twin pair of the one-stream form runs at the split its members have as launches of their own
            calls = self.program.calls + (self.program_serial.calls if self.program_serial is not self.program else [])
            for fn, a, k in calls:
                if fn.__name__ in ("conv_group", "pair"):
                    ops.tune_mode = mode if online else 0  # (a group's form is timed alone either way; see ops.tune_group)
                    members, split = a[0], k.get("split")
                    if fn.__name__ == "pair":
                        if a[0][0].__name__ != "conv" or a[1][0].__name__ != "conv":
                            continue
                        if mode == 1:  # (throughput mode: a pair runs in its members' own form, ops.pair -- nothing to time)
                            continue
                        members = [(a[0][1], a[0][2]), (a[1][1], a[1][2])]
                    if fn.__name__ == "pair" or split == OWN_SPLIT:
                        # (members at their own splits, a pair the one-stream form alone holds: the members' own forms first)
                        for aa, kk in members:
                            mk = ops.conv_key_of(aa[2], aa[3], kk)
                            if mk not in ops.tile_override and kk.get("tile") is None:
                                seen[mk] = ops.tune_conv(aa, kk)[0]
                    if fn.__name__ == "pair":
                        split = ops.pair_split(*members[0], *members[1])
                        if split is None:
                            continue
                    key = ops.group_key(members, split)
                    if key not in seen and key not in ops.tile_override:
                        seen[key] = ops.tune_group(members, split=split)[0]
                        if verbose:
                            print("tune", key, "->", seen[key], flush=True)
                    continue
                if fn.__name__ != "conv":
                    continue
                ops.tune_mode = mode
                key = ops.conv_key_of(a[2], a[3], k)
                if k.get("tile") is not None or (ops.tile_override.get(key) if online else lookup(ops.tile_override, key)) is not None:
                    continue
                if not online:  # (the alone-timed choice, which a throughput-mode key without an entry takes)
                    ops.tune_mode, key = 0, key[:-1] + (0,)
                if key in seen:
                    continue
                best, table = ops.tune_conv(a, k)
                seen[key] = best
                if verbose:
                    print("tune", key, "->", best, flush=True)
        finally:
            ops.tune_mode = mode
        return seen

    def prepare(self, H: int, W: int, steps: int, strength: float, controlnet_scale: float = 1.0,
                use_controlnet: bool = True, use_graph: Optional[bool] = None, autotune: bool = True, batch: int = 1,
                ref_mode: bool = False, device_seed: bool = False, frame_prompts: bool = False, frame_options: bool = False,
                edges: str = "sobel", canny_thresholds=(100, 200), color_match: Optional[str] = None, color_amount=1.0,
                keep_mask: bool = False, edge_blur=None, mask_feather=None):
        """Fix the frame geometry and schedule; build the static program and capture it into a hipGraph
        (the reference's intent at videopipeline.py:35-47, `compile_model`).

        ref_mode: the reference-only variant (lcm_reference_pipeline.py:855-890; no ControlNet, one frame per launch): per
        step a WRITE pass of the UNet over the noised latents of the reference image (upload it into `ref_u8`) banks
        self-attention keys / values and block-output statistics, the READ pass over the frame's latents uses them.

        batch > 1: that many frames (of independent streams / sessions, or consecutive frames of one stream) go
        through every kernel together, stacked along the GEMM M dimension: one pass over the 2.45 GB of weights and
        one launch per layer serve all of them.  Each frame is still denoised independently (own GroupNorm statistics,
        own attention, same noise draws as a lone frame: the reference resets its RNG per frame).

        device_seed: the noise is drawn on the device, inside the captured program, as a function of one seed PER FRAME of the
        launch (include/vsd.h THE NOISE CONTRACT; `submit_*(seeds=...)`): the program records vsd_add_noise_seeded /
        vsd_lcm_step_seeded in place of the `_dev` forms -- launch for launch -- and reads the seeds from `seed_dev`, a buffer of
        this engine's own; there is no host noise table.  A new seed is 8 bytes per frame copied ahead of the launch: no drain,
        no `update_options`, no re-capture.  Default: the CPU-contract draws of `host_noise`, the same for every frame.

        frame_prompts: every frame of the launch has a prompt of its own (`use_prompts`): the program reads K / V^T from a per-frame block
        (FramePromptLayout) and records every cross-attention in the explicit form -- q GEMM over all B*hw rows, attention with image b on
        its own key rows / V^T columns, out GEMM -- at all widths (no absorbed weights: they would be per frame).  A cached prompt enters
        a frame slot by one `prompt_install` launch ahead of the program.  Default: one prompt per launch, as before.

        frame_options: every frame of the launch has a `strength` and a `controlnet_scale` of its own (`use_options`; `strength` and
        `controlnet_scale` here are what a launch runs with until then).  The program reads the scheduler coefficients, the time tables and
        the ControlNet scales from blocks of THIS engine with one slot per frame (OptionLayout; not shared with the plan's other engines):
        the scheduler ops are the `_frames` forms, conv1 of every ResnetBlock is recorded without its time vector and norm2 adds the
        frame's slice of the time table to its input (`groupnorm_addvec`), the zero-convs are recorded without scale and residual and one
        `cn_merge_frames` launch per step merges all 13 residuals with the frame's scales.  Composes with device_seed and frame_prompts;
        not with ref_mode or an SDXL UNet.  Default: one set of options per plan (`update_options`), as before.

        edges: what the ControlNet is conditioned on.  "sobel" (default): the reference's stand-in, the Sobel magnitude over the frame's
        maximum (canny_gpu.py:27-44).  "canny": real Canny edges by THE EDGE CONTRACT of include/vsd.h -- binary, one pixel wide, what
        control_v11p_sd15_canny was trained on; the program records `canny_control` in place of `sobel_control`, call for call.
        canny_thresholds = (low, high): integers with 0 <= low <= high <= 2040 on |dx| + |dy| (floats are floored), read by "canny" only.
        Composes with every other mode (none of them touches the edge stage); without a ControlNet there is no edge stage and the
        switch is inert.  A "canny" program has no plan-file export (`vsd_canny_control` is not a plan function).

        color_match: None (default: the program as before, call for call), "histogram" or "meanstd": the colours of every input frame
        are transferred onto its output frame by THE COLOUR CONTRACT of include/vsd.h -- the program records one `color_match` over
        all B frames right behind `postprocess_rgb`, from `frame_u8` onto `out_u8` in place.  color_amount: a number in [0, 1] (0: the
        output as it is, 1: fully matched), the value every frame starts with; `set_color_amount` changes it per frame from the next launch on
        without a re-capture.  Composes with every other mode (the source is whatever ended up in `frame_u8`; ref_mode and SDXL
        included).  Such a program has no plan-file export (`vsd_color_match` is not a plan function).

        keep_mask: every frame of the launch has a u8 [H][W] mask (`set_masks`; 255: restyled, 0: kept as the camera saw it; all 255 until
        then) by THE KEEP MASK of include/vsd.h.  The program records `mask_latent` once ahead of the first step, a `latent_keep` right
        behind every `lcm_step` (in the kept region the next sample is the input's latents noised to the next timestep with the frame's own
        draw 0, so the UNet sees the real surroundings at every step) and one more, the final form, behind the last (the denoised latents
        give way to the input's), and `mask_blend(frame_u8 -> out_u8)` behind `postprocess_rgb` -- behind `color_match` when both are
        on: colours are matched over the whole frame first.  With all-255 masks the frames are the default program's bit for bit.  New
        masks are one B*H*W-byte copy ahead of the next launch (`_sync_mask`), no re-capture; a slot has masks of its own.  Composes with
        device_seed, frame_prompts, frame_options, edges and color_match; not with ref_mode or an SDXL UNet.  No plan-file export.

        edge_blur / mask_feather: None (no buffer, no table, no launch: the program of before) or a sigma in [0, 10] of the device
        Gaussian blur (THE BLUR CONTRACT of include/vsd.h; `videosd_amd.blur.gauss_taps`; 0: the identity table).  edge_blur: ONE
        `gauss_blur` over all B frames ahead of the per-frame edge op, on its stream; `canny_control` / `sobel_control` read the blurred
        copy (webcam noise no longer makes one-pixel edges flicker), `preprocess_rgb`, the encoder, `color_match` and `mask_blend` keep
        reading the camera's frame.  Without a ControlNet (SDXL; use_controlnet=False) it is accepted and inert, as `edges` is.
        mask_feather (needs keep_mask): ONE `gauss_blur` with C = 1 ahead of `mask_latent`; `mask_latent` and `mask_blend` read the soft
        mask, `set_masks` keeps uploading the caller's own.  An all-255 mask stays all-255, so it still gives the default frames.
        `set_edge_blur` / `set_mask_feather` change the sigma from the next launch on: 136 bytes ahead of the program, no re-capture.
        No plan-file export (`vsd_gauss_blur` is not a plan function)."""
        edges, canny_thresholds = L.check_edges(edges, canny_thresholds)
        if edges == "canny" and not hasattr(self.ops, "canny_control"):
            raise ValueError('edges="canny" needs the op canny_control, which this ops object does not have')
        color_match, color_a = L.check_color_match(color_match, color_amount)
        if color_match is not None and not hasattr(self.ops, "color_match"):
            raise ValueError(f'color_match="{color_match}" needs the op color_match, which this ops object does not have')
        if color_match is not None and H * W > L.COLOR_MAX_PIXELS:
            raise ValueError(f'color_match="{color_match}": a {W} x {H} frame has more than {L.COLOR_MAX_PIXELS} pixels (include/vsd.h VSD_COLOR_MAX_PIXELS)')
        if keep_mask:
            missing = [f for f in KEEP_MASK_OPS if not hasattr(self.ops, f)]
            if missing:
                raise ValueError(f"keep_mask=True needs the op(s) {', '.join(missing)}, which this ops object does not have")
            if ref_mode or self.unet.add_l1 is not None:
                raise ValueError("keep_mask=True: reference-only (ref_mode) and SDXL programs have no keep-mask stages")
        if mask_feather is not None and not keep_mask:
            raise ValueError("mask_feather needs keep_mask=True: it feathers the keep masks, and this program has none")
        sigmas = {k: v for k, v in (("edge_blur", edge_blur), ("mask_feather", mask_feather)) if v is not None}
        for k, v in sigmas.items():
            try:
                blur.gauss_taps(v)
            except ValueError as e:
                raise ValueError(f"{k}: {e}") from None
        if sigmas and not hasattr(self.ops, "gauss_blur"):
            raise ValueError(f"{' / '.join(sigmas)} needs the op gauss_blur, which this ops object does not have")
        self._check_arguments(H, W, batch, use_controlnet, ref_mode, device_seed, frame_prompts, frame_options)
        sched = LCMSchedule(strength, steps)
        self._prepare_prompt_block(batch, frame_prompts)
        # from here on the engine's previous plan is gone
        self._destroy_graphs()
        self._reset_plan_state()
        self.batch = batch
        self.frame_prompts, self.frame_options = bool(frame_prompts), bool(frame_options)
        self.edges, self.canny_thresholds = edges, canny_thresholds if edges == "canny" else None
        self.color_mode = color_match
        if color_match is not None:  # (this engine's own, like the seeds: a slot has its own)
            self.color_amounts = self.ops.zeros(batch, dtype=torch.int32)
            self._color_host = torch.zeros(batch, dtype=torch.int32, pin_memory=torch.cuda.is_available())
            self.set_color_amount(color_a / L.COLOR_MAX_AMOUNT)
        self.keep_mask = bool(keep_mask)
        if keep_mask:  # (this engine's own as well)
            self.mask_u8 = self.ops.zeros(batch, H, W, dtype=torch.uint8)
            self.mask_w = self.ops.zeros(batch, (H // 8) * (W // 8), dtype=torch.float32)
            self._mask_host = torch.zeros(batch, H, W, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            self.set_masks(None)
        self.taps = {k: TapBlock(self.ops, v) for k, v in sigmas.items()}  # (this engine's own as well)
        if "mask_feather" in self.taps:
            self.mask_soft = self.ops.zeros(batch, H, W, dtype=torch.uint8)
        # The lock-step encoders are the one-stream form of EVERY program.  What a pair's grid looks like depends on the mode: a one-frame
        # program (latency mode) takes the pair's own table entry, timed alone; a coalesced launch on busy lanes (throughput mode) runs
        # the pair in the form its members have as launches of their own -- a latency-chosen form there occupies more workgroup-time
        # than the two launches (profiles/round5f_pairs_at_5x4.txt).  Measured on one box with / without pairs: 1 x 4 89.7 / 83.5,
        # 2 x 4 122.2 / 118.8, 3 x 4 133.8 / 131.3, 3 x 3 127.7 / 123.0, 4 x 4 138.8 / 138.3, 5 x 4 140.2 / 140.4 frames/s.
        self._twin_now = self.twin_encoders
        if hasattr(self.ops, "tune_mode"):
            self.ops.tune_mode = 1 if self.tune_for_lanes else 0
        if use_graph is not None:
            self.use_graph = use_graph
        coef = self._prepare_constants(sched, controlnet_scale, use_controlnet, ref_mode)
        sops = self._prepare_noise(len(sched), H // 8, W // 8, ref_mode, device_seed)
        self._record(sched, sops, coef, H, W, use_controlnet, ref_mode)
        self.plan = dict(H=H, W=W, steps=steps, strength=strength, cn_scale=controlnet_scale, cn=use_controlnet, n=len(sched), batch=batch,
                         ref_mode=bool(ref_mode), device_seed=bool(device_seed), frame_prompts=bool(frame_prompts), frame_options=bool(frame_options), tuned_for_lanes=bool(self.tune_for_lanes),
                         edge_mode=self.edges, canny_thresholds=self.canny_thresholds,  # ("edges" is taken: the event edges of the captured sequence)
                         color_match=self.color_mode, keep_mask=self.keep_mask, edge_blur="edge_blur" in self.taps, mask_feather="mask_feather" in self.taps,
                         sizes=self._level_sizes(H, W), timesteps=sched.timesteps, n_ops=len(self.program.calls), arena_bytes=self.arena.peak)
        self._warm_up_and_capture(autotune)
        return self.plan

    def _check_arguments(self, H, W, batch, use_controlnet, ref_mode, device_seed, frame_prompts, frame_options):
        """what `prepare` refuses, before it touches anything; the ops object's capabilities first (they read nothing but `self.ops`)"""
        if frame_options:
            missing = [f for f in FRAME_OPTION_OPS if not hasattr(self.ops, f)]
            if missing:
                raise ValueError(f"frame_options=True needs the op(s) {', '.join(missing)}, which this ops object does not have")
            if ref_mode or self.unet.add_l1 is not None:
                raise ValueError("frame_options=True: reference-only and SDXL programs keep one set of options per plan (update_options)")
        if frame_prompts and not hasattr(self.ops, "prompt_install"):
            raise ValueError("frame_prompts=True needs the op prompt_install, which this ops object does not have")
        if device_seed and not all(hasattr(self.ops, f) for f in ("add_noise_seeded", "lcm_step_seeded")):
            raise ValueError("device_seed=True needs the ops add_noise_seeded and lcm_step_seeded, which this ops object does not have")
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if H % 8 or W % 8:
            raise ValueError("height and width must be multiples of 8 (TAESD / latent stride)")
        if self._want is None and self.family.get("prompt") is None and not (frame_prompts and self._want_list):
            raise RuntimeError("set_text_embeds must be called before prepare")
        if use_controlnet and self.cn is None:
            raise RuntimeError("no ControlNet weights loaded")
        if ref_mode and (batch != 1 or use_controlnet or (H // 8) * (W // 8) % 8):
            raise ValueError("ref_mode: one frame per launch, no ControlNet (the reference-only pipeline has none), "
                             "latent pixels a multiple of 8")

    def _prepare_prompt_block(self, batch: int, frame_prompts: bool):
        """`pblock` for the prompt(s) this engine is to run: kept, with what it holds, when the one of the plan before has the layout"""
        if frame_prompts:
            tl = self._frame_sources(batch)[0].layout.tl
            lays = self.family.setdefault("frame_layouts", {})  # (one layout OBJECT per (text length, frames), as for `layouts`)
            lay = lays.get((tl, batch))
            if lay is None:
                lay = lays[(tl, batch)] = FramePromptLayout(self._nets(), tl, batch)
            if self.pblock is None or self.pblock.layout is not lay:
                self.pblock = PromptBlock(self.ops, lay)
                self._prompt_slots = FrameSlots(self.pblock.buf, lay)
            self._mix_tables(self._frame_sources(batch)[0].layout)
            return
        src = self._want if self._want is not None else self.family.get("prompt")
        if self.pblock is None or self.pblock.layout is not src.layout:
            self.pblock = PromptBlock(self.ops, src.layout)
            self._installed = self._prompt_slots = None
        self._mix_tables(src.layout)

    def _prepare_constants(self, sched: LCMSchedule, controlnet_scale: float, use_controlnet: bool, ref_mode: bool):
        """Per-plan constants the captured graph reads from device memory: [0:2] add_noise coefficients, [2 + 6i : 8 + 6i]
        the scheduler coefficients of step i, then the 13 ControlNet residual scales; plus the time-embedding projections
        of every step.  `update_options` rewrites them in place -- a new strength / controlnet_scale needs no re-capture.
        -> the coefficients as the program reads them (`frame_options`: frame 0's)."""
        ops, n, B = self.ops, len(sched), self.batch
        ncn = 16
        if self.frame_options:
            # this engine's OWN blocks, one slot per frame: the program records frame 0's addresses and the strides; `_sync_options` fills
            # the slots ahead of every launch (before the warm-up run, with the options `prepare` was given)
            self.fo_layout = OptionLayout(n, self._option_cols(use_controlnet), B)
            self.fo_buf = ops.zeros(self.fo_layout.nbytes, dtype=torch.uint8)
            self._option_slots = FrameSlots(self.fo_buf, self.fo_layout)
            if use_controlnet:
                assert self._nres() <= ncn
                self.fo_scale = ops.zeros(B, ncn, dtype=torch.float32)
                self._fo_scale_host = torch.zeros(B, ncn, dtype=torch.float32, pin_memory=torch.cuda.is_available())
            self.shared["n"] = n
            return self.fo_layout.view(self.fo_buf, "coef")
        c = self.shared.get("consts")
        if self.is_slot:  # computed by the parent engine's prepare / update_options
            assert c is not None and self.shared.get("n") == n, "prepare the parent engine with the same schedule first"
        else:
            if c is None or self.shared.get("n") != n:
                self.shared["consts"] = c = ops.zeros(2 + 6 * n + ncn, dtype=torch.float32)
                self.shared["n"] = n
            temb = self.shared.setdefault("temb", {})
            for name, net in self._networks(use_controlnet) + ([("ref", self.unet)] if ref_mode else []):
                if name not in temb or temb[name].shape[0] != n:
                    temb[name] = ops.zeros(n, net.temb_proj.n)
            self.shared["ref_mode"] = bool(ref_mode)
            self._write_constants(sched, controlnet_scale, use_controlnet)
        self._cn_scale_consts = c[2 + 6 * n:]
        return c

    def _prepare_noise(self, n: int, h0: int, w0: int, ref_mode: bool, device_seed: bool) -> SchedulerOps:
        """Where the noise comes from, chosen once per plan.  Default: the reference resets the global CPU generator to a
        fresh-Generator state on every frame (videopipeline.py:126), so for a fixed shape the draws are the same every frame."""
        ops = self.ops
        cstride = self.fo_layout.coef_stride if self.frame_options else 0
        if device_seed:
            # one seed per frame of the launch, u32 (low, high) pairs = little-endian u64: this engine's own (a slot has its own)
            self.seed_dev = ops.zeros(self.batch, dtype=torch.int64)
            self._seed_host = torch.zeros(self.batch, dtype=torch.int64, pin_memory=torch.cuda.is_available())
            return SchedulerOps(h0 * w0, seeds=self.seed_dev, coef_stride=cstride)
        draws, ref_draws = self.host_noise(n, h0, w0, ref=ref_mode)
        self.noise = ops.to_device(draws)
        if ref_draws is not None:
            self.noise_ref = ops.to_device(ref_draws)
        return SchedulerOps(h0 * w0, noise=self.noise, noise_ref=self.noise_ref, coef_stride=cstride)

    def _level_sizes(self, H: int, W: int):
        """(height, width) of the latents at every level of the UNet"""
        sizes = [(H // 8, W // 8)]
        for _ in range(len(self.ucfg.block_out_channels) - 1):
            ph, pw_ = sizes[-1]
            sizes.append(((ph + 1) // 2, (pw_ + 1) // 2))
        return sizes

    def _record(self, sched: LCMSchedule, sops: SchedulerOps, c, H: int, W: int, use_controlnet: bool, ref_mode: bool):
        """arena, I/O tensors and the static program, in both forms"""
        ops, B, n = self.ops, self.batch, len(sched)
        sizes = self._level_sizes(H, W)
        h0, w0 = sizes[0]
        hw0 = h0 * w0
        self.arena = a = Arena(ops, chunk_bytes=max(256 << 20, _ru(B * H * W * 64 * 2, 1 << 20)))  # >= one TAESD tensor
        # persistent per-frame I/O
        frame_b = ops.zeros(B, H, W, 3, dtype=torch.uint8)
        out_b = ops.zeros(B, H, W, 3, dtype=torch.uint8)
        # public I/O buffers: [H][W][3] for a single frame (as before), [B][H][W][3] for a batch
        self.frame_u8 = frame_b[0] if B == 1 else frame_b
        self.out_u8 = out_b[0] if B == 1 else out_b
        self.edge_u8 = ops.zeros(B * H * W, dtype=torch.uint8)
        enc_in = a.alloc(B * H * W, 8)
        x0 = a.alloc(B * hw0, 8)
        lat = [a.alloc(B * hw0, 8), a.alloc(B * hw0, 8)]
        eps = a.alloc(B * hw0, 8)
        den = a.alloc(B * hw0, 8)
        dec_in = a.alloc(B * hw0, 8)
        dec_out = a.alloc(B * H * W, 8)
        for t in (x0, lat[0], lat[1], eps, den, dec_in):
            ops.zero_(t)
        self.buffers = {"x0": x0, "lat": lat, "eps": eps, "denoised": den, "dec_in": dec_in, "dec_out": dec_out}
        r = Recorder(ops)
        img = lambda t, b, n: t[b * n:(b + 1) * n]  # noqa: E731  rows of image b
        r.preprocess_rgb(frame_b, B * H, W, enc_in)
        cond_emb = None
        if use_controlnet:
            ctrl = a.alloc(B * H * W, 8)
            side0 = self.overlap_controlnet and self.use_side_stream
            if side0:  # Sobel + the conditioning embedding only feed the ControlNet encoder (which runs on stream 1 too)
                r.fork()
                r.use_stream(1)
            edge_src = frame_b
            if "edge_blur" in self.taps:  # the edge ops alone read the calmed copy; everything else keeps the camera's frame
                edge_src = self.blur_u8 = ops.zeros(B, H, W, 3, dtype=torch.uint8)
                r.gauss_blur(frame_b, edge_src, B, H, W, 3, self.taps["edge_blur"].dev)
            for b in range(B):  # the edge map is normalised by ITS frame's maximum (canny_gpu.py:39)
                if self.edges == "canny":
                    r.canny_control(edge_src[b], H, W, *self.canny_thresholds, img(self.edge_u8, b, H * W), img(ctrl, b, H * W))
                else:
                    r.sobel_control(edge_src[b], H, W, 0.11, 0.8, img(self.edge_u8, b, H * W), img(ctrl, b, H * W))  # videopipeline.py:109
            cond_emb = self._cond_embedding(r, ctrl, H, W)
            self.buffers["control"], self.buffers["cond_emb"] = ctrl, cond_emb
            if side0:
                r.use_stream(0)
        self._encode(r, enc_in, H, W, x0)
        if ref_mode:
            ref_b = ops.zeros(1, H, W, 3, dtype=torch.uint8)
            self.ref_u8 = ref_b[0]
            ref_in, ref_x0, ref_xt, ref_eps = a.alloc(H * W, 8), a.alloc(hw0, 8), a.alloc(hw0, 8), a.alloc(hw0, 8)
            for t in (ref_x0, ref_xt, ref_eps):
                ops.zero_(t)
            r.preprocess_rgb(ref_b, H, W, ref_in)
            self._encode(r, ref_in, H, W, ref_x0)
            self.buffers["ref_x0"] = ref_x0
        # every frame gets the same draws: the reference resets its RNG per frame
        sops.add_noise(r, x0, 0, 0, c[0:2], B, lat[0])
        mask_read = self.mask_u8
        if self.mask_soft is not None:  # the feathered masks: what both mask stages read from here on
            r.gauss_blur(self.mask_u8, self.mask_soft, B, H, W, 1, self.taps["mask_feather"].dev)
            mask_read = self.mask_soft
        if self.keep_mask:  # the latent weights of this launch's masks, ahead of the first step
            r.mask_latent(mask_read, B, H, W, self.mask_w)
        mark = a.mark()
        for i in range(n):
            a.rewind(mark)
            self._vt_count = 0
            cur, nxt = lat[i & 1], lat[(i + 1) & 1]
            if use_controlnet:
                # the ControlNet encoder and the UNet encoder both depend only on the current latents: run them
                # on two streams (two parallel branches of the captured graph), join before the zero-convs
                # ... or in lock step on ONE stream: the ControlNet is a copy of the UNet encoder's topology, so the k-th call of
                # one is the k-th call of the other with another weight set -- each such pair goes out as one grid per kernel
                # (ops.pair): a quarter of a frame's launches less, and the small layers fill twice the chip.  Measured on MI355X
                # (one frame per launch, 512x512 4-step): a lone launch 20.8 ms on two streams | 21.3 ms in lock step; with three /
                # four lanes busy (no second stream to be had) 75.0 / 84.1 | 82.1 / 88.8 frames/s.  So both forms are recorded
                # -- same buffers, same results -- and `launch` takes the one its moment calls for.
                rc_, ru_ = Recorder(ops), Recorder(ops)
                cn_mid, cn_skips = self._controlnet_encoder(rc_, i, cur, sizes, cond_emb)
                u_mid, u_skips = self._unet_encoder(ru_, i, cur, sizes)
                two = Recorder(ops)
                if self.overlap_controlnet:
                    two.fork()
                    two.use_stream(1)
                two.calls += rc_.calls
                two.use_stream(0)
                two.calls += ru_.calls
                if self.overlap_controlnet:
                    two.join()
                if self._twin_now and hasattr(ops, "pair"):
                    twin = Recorder(ops)
                    self._zip_pairs(twin, ru_.calls, rc_.calls)
                    r.variants(two.calls, twin.calls)
                else:
                    r.variants(two.calls, two.calls)
                u_mid, u_skips = self._controlnet_merge(r, cn_mid, cn_skips, u_mid, u_skips, sizes)
            elif ref_mode:
                rc = RefCtx(self.ucfg)
                # ref_xt = add_noise(ref latents, fresh draw, t_i) (lcm_reference_pipeline.py:861-871); the coefficients of
                # timestep t_i are the first two of the step's scheduler coefficients
                sops.add_noise(r, ref_x0, 1, i, c[2 + 6 * i:4 + 6 * i], 1, ref_xt)  # (kind 1: the reference latents' draws, one per step)
                w_mid, w_skips = self._unet_encoder(r, i, ref_xt, sizes, ref=rc, temb=self.shared["temb"]["ref"])
                self._unet_decoder(r, i, w_mid, w_skips, sizes, ref_eps, ref=rc, temb=self.shared["temb"]["ref"])
                rc.mode = "read"
                u_mid, u_skips = self._unet_encoder(r, i, cur, sizes, ref=rc)
            else:
                u_mid, u_skips = self._unet_encoder(r, i, cur, sizes)
            self._unet_decoder(r, i, u_mid, u_skips, sizes, eps, ref=rc if ref_mode else None)
            last = i == n - 1
            # (draw i + 1; 0: a one-step schedule adds none)
            sops.lcm_step(r, eps, cur, i + 1 if sched.multistep else 0, c[2 + 6 * i:8 + 6 * i], B, nxt, den, dec_in if last else None)
            if self.keep_mask:  # the kept region of the next sample: x0 noised to the next timestep (the step's own coefficients 4, 5)
                sops.latent_keep(r, x0, self.mask_w, c[2 + 6 * i:8 + 6 * i], B, nxt)
                if last:
                    sops.latent_keep_final(r, x0, self.mask_w, B, den, dec_in)
        self._decode(r, dec_in, h0, w0, dec_out)
        r.postprocess_rgb(dec_out, 8, B * H * W, out_b)
        if self.color_mode is not None:  # ahead of everything that reads `out_u8` (`collect_u8`, the queued `rgb_to_i420`)
            r.color_match(frame_b, out_b, B, H, W, self.color_mode, self.color_amounts)
        if self.keep_mask:  # (likewise ahead of every reader; the colours were matched over the whole frame first)
            r.mask_blend(frame_b, out_b, mask_read, B, H, W)
        # program: what a lone launch runs (the ControlNet encoder on the side stream when `overlap_controlnet`);
        # program_serial: everything on the lane's own stream (the encoders in lock step when `twin_encoders`)
        self.program = r.flavor(0 if self.overlap_controlnet or not self._twin_now else 1)
        self.program_serial = r.flavor(1) if self._twin_now and self.overlap_controlnet and use_controlnet else self.program

    def _warm_up_and_capture(self, autotune: bool):
        """per-shape kernel configuration (timed once per shape, cached in ops.tile_override), warm-up, capture"""
        ops = self.ops
        torch.cuda.synchronize() if torch.cuda.is_available() else None  # allocation fills vs. kernel streams
        self._sync_prompt()
        self._sync_options()
        self._sync_color()
        self._sync_mask()
        self._sync_blur()
        if autotune:  # (only shapes missing from the shared table are timed: a slot with the parent's batch size finds all)
            self.autotune()
        self.program.run()
        if self.program_serial is not self.program:
            self.program_serial.run()
        ops.synchronize()
        if self.use_graph:
            # two launch sequences of the SAME program (same kernels, same buffers): the ControlNet encoder on the lane's side
            # stream (a lone launch: ~4 ms less per frame), and everything on the lane's own stream (what a launch takes when
            # three or four lanes are busy: the side stream IS another lane's stream).  `launch(overlap=...)` picks per launch.
            self.graph = self._capture(self.program)
            self.plan["graphs"], self.plan["edges"] = ops.seq_count(self.graph)
            two_forms = self.plan["edges"] or self.program_serial is not self.program
            self.graph_serial = self._capture(self.program_serial, serial=True) if two_forms else self.graph

    SYNC_OPS = SYNC_OPS
    flat_calls = staticmethod(flat_calls)

    def launches_by_kind(self, serial: bool = False):
        """kernel launches one replay of the recorded program (serial: of its one-stream form) issues, by kind -> (total, {kind: launches})"""
        return launches_by_kind(self.ops, self.program_serial if serial else self.program)

    def _capture(self, r: Recorder, serial: bool = False):
        """the recorded program -> a launch sequence (program.capture)"""
        return capture(self.ops, r, serial)

    def _destroy_graphs(self):
        g, gs = self.graph, self.graph_serial
        self.graph = self.graph_serial = None
        if g is not None:
            self.ops.seq_destroy(g)
        if gs is not None and gs is not g:
            self.ops.seq_destroy(gs)

    def _write_constants(self, sched: LCMSchedule, controlnet_scale: float, use_controlnet: bool):
        """Schedule- and option-dependent constants -> the device block / time-embedding tables the graphs read."""
        vals = schedule_constants(sched) + controlnet_scales(self._nres(), controlnet_scale).tolist()
        c = self.shared["consts"]
        host = torch.zeros(c.numel(), dtype=torch.float32)
        host[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
        self.ops.upload(c, host)
        self._write_time_tables(sched, use_controlnet)

    def _write_time_tables(self, sched: LCMSchedule, use_controlnet: bool):
        """the per-step time-embedding projections of the plan(s) that share `shared`, from the weights as they are NOW; remembers the
        schedule and the family's "weights_epoch", so that the first launch after a LoRA scale change can write them again"""
        for name, net in self._networks(use_controlnet):
            self._time_embeddings(net, sched, self.shared["temb"][name])
        if self.shared.get("ref_mode"):  # the reference-only WRITE pass: same timesteps, no guidance embedding
            self._time_embeddings(self.unet, sched, self.shared["temb"]["ref"], use_cond=False)
        self.ops.synchronize()
        self.shared["sched"], self.shared["sched_cn"] = sched, bool(use_controlnet)
        self.shared["weights_epoch"] = self.family.get("weights_epoch", 0)

    def update_options(self, strength: float, controlnet_scale: float) -> bool:
        """New `strength` / `controlnet_scale` for the prepared plan WITHOUT re-capturing: the captured graph reads the
        scheduler coefficients, the ControlNet scales and the per-step time-embedding projections from device memory, so
        a slider drag (server.py:163-197: strength in steps of 0.02, controlnet_scale 0.05-3) costs a few small uploads and
        the ~10 tiny GEMMs of the time path.  Returns False when the new strength gives another NUMBER of timesteps (then
        the program itself changes: call `prepare`).  Call it on the parent engine, with no launch in flight; its slots
        follow (they share the constant block)."""
        if self.plan is None or self.is_slot:
            raise RuntimeError("update_options: prepare the parent engine first")
        if self.plan.get("frame_options"):
            raise RuntimeError("update_options: a frame_options plan takes its options per launch (use_options)")
        sched = LCMSchedule(strength, self.plan["steps"])
        if len(sched) != self.plan["n"]:
            return False
        self._write_constants(sched, controlnet_scale, self.plan["cn"])
        self.plan.update(strength=strength, cn_scale=controlnet_scale, timesteps=sched.timesteps)
        return True

    def set_color_amount(self, amount):
        """The colour-match amount of the launches from the next one on: a number in [0, 1] for every frame, or one per frame of the
        launch.  Only noted here (a launch in flight keeps the amounts it was submitted with); `launch` sends a changed value ahead of
        the program (`_sync_color`), as the seeds travel: no re-capture, no drain."""
        if self.color_amounts is None:
            raise ValueError("set_color_amount needs an engine prepared with color_match=\"histogram\" or \"meanstd\"")
        B = self.color_amounts.numel()
        vals = list(amount) if isinstance(amount, (list, tuple, np.ndarray)) else [amount] * B
        if len(vals) != B:
            raise ValueError(f"color_amount must be a number or a sequence of {B} numbers (one per frame of the launch)")
        self.color_a = tuple(L.check_color_amount(v) for v in vals)

    def _sync_color(self):
        """the amounts of `set_color_amount` on the lane's stream ahead of the program, when they changed: 4 bytes per frame from the pinned
        mirror (the lane's previous launch has been collected, so nothing in flight reads the mirror)"""
        if self.color_a != self._color_sent:
            self._color_host.numpy()[:] = np.array(self.color_a, dtype=np.int32)
            self.ops.upload(self.color_amounts, self._color_host)
            self._color_sent = self.color_a

    def set_masks(self, masks):
        """The keep masks of the launches from the next one on: one u8 [H][W] array for every frame, B of them ([B][H][W] or a sequence),
        or None for all 255 (everything restyled).  Only noted here (a launch in flight keeps the masks it was submitted with); `launch`
        sends changed masks ahead of the program (`_sync_mask`): no re-capture, no drain."""
        if self.mask_u8 is None:
            raise ValueError("set_masks needs an engine prepared with keep_mask=True")
        B, H, W = self.mask_u8.shape
        if masks is None:
            want = np.full((B, H, W), 255, dtype=np.uint8)
        else:
            if isinstance(masks, (list, tuple)):
                if len(masks) != B:
                    raise ValueError(f"masks must be one [H][W] array or {B} of them (one per frame of the launch), not {len(masks)}")
                masks = [np.asarray(m) for m in masks]
                if any(m.shape != (H, W) for m in masks):
                    raise ValueError(f"every mask must be a u8 array of shape ({H}, {W}), not {[m.shape for m in masks]}")
                if any(m.dtype != np.uint8 for m in masks):
                    raise ValueError("every mask must be a u8 array")
                masks = np.stack(masks)
            m = np.asarray(masks)
            if m.dtype != np.uint8:
                raise ValueError(f"masks must be u8 (255: restyled, 0: kept), not {m.dtype}")
            if m.shape == (H, W):
                m = np.broadcast_to(m, (B, H, W))
            elif m.shape != (B, H, W):
                raise ValueError(f"masks must have shape ({H}, {W}) or ({B}, {H}, {W}), not {m.shape}")
            want = np.array(m, dtype=np.uint8, order="C")  # (a copy: the caller may draw on in its array)
        if self._mask_want is None or not np.array_equal(want, self._mask_want):
            self._mask_want = want
            self._mask_epoch += 1

    def _sync_mask(self):
        """the masks of `set_masks` on the lane's stream ahead of the program, when they changed: B*H*W bytes from the pinned mirror (the
        lane's previous launch has been collected, so nothing in flight reads the mirror)"""
        if self.mask_u8 is not None and self._mask_sent != self._mask_epoch:
            self._mask_host.numpy()[:] = self._mask_want
            self.ops.upload(self.mask_u8, self._mask_host)
            self._mask_sent = self._mask_epoch

    def _set_blur(self, switch: str, sigma):
        if switch not in self.taps:
            raise ValueError(f"set_{switch} needs an engine prepared with {switch}=<sigma> (0 for none yet): this program has no such blur")
        try:
            self.taps[switch].set(sigma)
        except ValueError as e:
            raise ValueError(f"{switch}: {e}") from None

    def set_edge_blur(self, sigma):
        """The sigma of the blur ahead of the edge op, in [0, 10] (0: the identity table), for the launches from the next one on.  Only noted
        here (a launch in flight keeps the table it was submitted with); `launch` sends a changed table ahead of the program: no
        re-capture, no drain."""
        self._set_blur("edge_blur", sigma)

    def set_mask_feather(self, sigma):
        """the same for the blur of the keep masks"""
        self._set_blur("mask_feather", sigma)

    def _sync_blur(self):
        """changed tap tables of `set_edge_blur` / `set_mask_feather` on the lane's stream ahead of the program"""
        for block in self.taps.values():
            block.sync(self.ops)

    @staticmethod
    def host_noise(n_steps: int, h: int, w: int, ref: bool = False):
        """The CPU draws of one frame, in the reference's order: draw 0 = prepare_latents noise
        (lcm_controlnet.py:331, generator not forwarded), then one torch.randn per scheduler step
        (:1033) when the schedule has more than one step.  fp32 [(n+1), 4, h*w].
        ref=True (reference-only mode): every step first draws the noise of the reference latents
        (lcm_reference_pipeline.py:861-863) from the same stream; returns (draws, ref_draws [n, 4, h*w])."""
        st = torch.get_rng_state()
        try:
            torch.manual_seed(0)
            torch.default_generator.set_state(torch.Generator(device="cpu").get_state())
            draws = [torch.randn(1, 4, h, w)]
            ref_draws = []
            for _ in range(n_steps):
                if ref:
                    ref_draws.append(torch.randn(1, 4, h, w))
                if n_steps > 1:
                    draws.append(torch.randn(1, 4, h, w))
            if n_steps <= 1:
                draws.append(torch.zeros(1, 4, h, w))
        finally:
            torch.set_rng_state(st)
        d = torch.cat(draws, dim=0).reshape(len(draws), 4, h * w).contiguous()
        if not ref:
            return d, None
        return d, torch.cat(ref_draws, dim=0).reshape(n_steps, 4, h * w).contiguous()

    # ---------------------------------------------------------------- per frame
    def launch(self, overlap: Optional[bool] = None):
        """Enqueue one frame's work (frame_u8 -> out_u8) on the lane's stream(s).  overlap: run the ControlNet encoder on the
        lane's side stream (default: `self.overlap_launch`); pass False when a launch of the lane that OWNS that stream
        (lane + 2 mod 4) may be in flight -- two busy queues on one command-processor pipe take turns (ops.HipOps)."""
        self._sync_prompt()
        self._sync_options()
        self._sync_color()
        self._sync_mask()
        self._sync_blur()
        if self.graph is not None:
            ov = self.overlap_launch if overlap is None else overlap
            self.ops.seq_launch(self.graph if ov else self.graph_serial)
        else:
            if hasattr(self.ops, "tune_mode"):
                self.ops.tune_mode = 1 if self.tune_for_lanes else 0
            ov = self.overlap_launch if overlap is None else overlap
            (self.program if ov else self.program_serial).run()

    def _want_shape(self):
        p = self.plan
        return (p["H"], p["W"], 3) if p["batch"] == 1 else (p["batch"], p["H"], p["W"], 3)

    def _staging(self):
        """Pinned host buffers of this plan's frame(s): H2D / D2H run as asynchronous DMA on the kernel stream instead of
        going through the runtime's pageable-memory staging copies."""
        key = tuple(self.frame_u8.shape)
        st = self._stage
        if st is None or st[0] != key:
            pin = torch.cuda.is_available()
            st = (key, torch.empty(key, dtype=torch.uint8, pin_memory=pin), torch.empty(key, dtype=torch.uint8, pin_memory=pin),
                  torch.cuda.Event(enable_timing=True) if pin else None, torch.cuda.Event(enable_timing=True) if pin else None)
            self._stage = st
        return st

    def _check_seeds(self, seeds):
        """`seeds=` of a submit -> None (keep the seeds in place) or a list of B ints, refused BEFORE anything is enqueued"""
        if seeds is None:
            return None
        if self.seed_dev is None:
            raise ValueError("seeds= needs an engine prepared with device_seed=True (the default noise does not depend on a seed)")
        B = self.plan["batch"]
        vals = [seeds] * B if isinstance(seeds, (int, np.integer)) else list(seeds)
        if len(vals) != B or not all(isinstance(v, (int, np.integer)) for v in vals):
            raise ValueError(f"seeds must be an int or a sequence of {B} ints (one per frame of the launch)")
        return [int(v) & 0xFFFFFFFFFFFFFFFF for v in vals]

    def _upload_seeds(self, vals):
        """the launch's seeds (`_check_seeds`) on the lane's stream ahead of the graph launch, like the frame upload: 8 bytes per
        frame from the pinned mirror (the lane's previous launch has been collected, so nothing in flight reads the mirror)"""
        if vals is not None:
            self._seed_host.numpy().view(np.uint64)[:] = np.array(vals, dtype=np.uint64)
            self.ops.upload(self.seed_dev, self._seed_host)

    def submit_u8(self, frame: np.ndarray, overlap: Optional[bool] = None, seeds=None):
        """Upload + enqueue one frame (or batch) without waiting: pair with `collect_u8`.  Lets the host prepare the
        next frames / post-process the previous ones while this one is on the GPU.  overlap: see `launch`.
        seeds (device_seed engines): an int, or one int per frame of the launch; None keeps the seeds of the launch before."""
        want = self._want_shape()
        if frame.shape != want or frame.dtype != np.uint8:
            raise ValueError(f"frame must be uint8 {want}, got {frame.dtype} {frame.shape}")
        self._upload_seeds(self._check_seeds(seeds))
        hin = self._staging()[1]
        hin.numpy()[...] = frame.reshape(hin.shape)
        self.ops.upload(self.frame_u8, hin)
        self._launch_timed(overlap)

    def _launch_timed(self, overlap: Optional[bool]):
        """`launch` between the two events of this engine's staging: `last_gpu_ms` is the program alone, without the copies around it"""
        e0, e1 = self._staging()[3:]
        if e0 is not None:
            e0.record(self.ops.stream)
        self.launch(overlap)
        self.family.setdefault("in_flight", weakref.WeakSet()).add(self)  # (until the collect: what `set_adapter_scales` must not run beside; an engine that is dropped uncollected leaves by itself)
        if e1 is not None:
            e1.record(self.ops.stream)

    def _raw_frames(self, frame, kind, size_of):
        """`frame` of a raw submit -> [(frame, (left, top, right, bottom))] for the B frames of a launch: one `kind` object (B = 1) or a
        sequence of B; size_of(f) -> (width, height), or ValueError for what is no frame; the reference's crop box, refused when empty"""
        p = self.plan
        H, W, B = p["H"], p["W"], p["batch"]
        frames = [frame] if B == 1 and isinstance(frame, kind) else list(frame)
        if len(frames) != B:
            raise ValueError(f"this engine takes {B} frame(s) per launch, got {len(frames)}")
        out = []
        for f in frames:
            w, h = size_of(f)
            l, t, r, b = self.ops.center_crop_box(w, h, W, H)
            if not (0 <= l < r <= w and 0 <= t < b <= h):
                raise ValueError(f"the crop box of a {w} x {h} frame for {W} x {H} is empty")
            out.append((f, (l, t, r, b)))
        return out

    def _raw_staging(self, nbytes: int):
        """Pinned host bytes and device bytes for the crop boxes of camera frames (`submit_raw_u8`); grown, never shrunk.  The lane's
        previous launch has been collected (= its stream waited for) before the next submit, so nothing in flight reads the old ones."""
        st = self._raw_stage
        if st is None or st[0].numel() < nbytes:
            n = _ru(max(nbytes, 1 << 20), 1 << 20)
            st = (torch.empty(n, dtype=torch.uint8, pin_memory=torch.cuda.is_available()), self.ops.empty(n, dtype=torch.uint8))
            self._raw_stage = st
        return st

    def submit_raw_u8(self, frame, overlap: Optional[bool] = None, seeds=None):
        """`submit_u8` for CAMERA frames: uint8 [h][w][3] of any size (prepared with batch B > 1: a list of B frames, possibly of
        different sizes).  The reference's centre crop + LANCZOS resize (videopipeline.py:92-107) runs on the device: the crop box
        alone is uploaded and resampled into `frame_u8` by an ordinary launch in front of the captured program, bit for bit what
        PIL gives on the host.  A frame already of the plan's size goes straight into `frame_u8`.  seeds: see `submit_u8`."""
        p = self.plan
        seeds = self._check_seeds(seeds)
        H, W, B = p["H"], p["W"], p["batch"]

        def size_of(f):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError(f"frame must be uint8 [h][w][3], got {getattr(f, 'dtype', type(f))} {getattr(f, 'shape', '')}")
            return f.shape[1], f.shape[0]

        boxes, total = [], 0
        for f, (l, t, r, b) in self._raw_frames(frame, np.ndarray, size_of):
            boxes.append((f, (l, t, r, b, total)))
            total += _ru((r - l) * (b - t) * 3, 256)
        hraw, draw = self._raw_staging(total)
        self._upload_seeds(seeds)
        for i, (f, (l, t, r, b, off)) in enumerate(boxes):
            bw, bh = r - l, b - t
            n = bw * bh * 3
            hraw.numpy()[off:off + n].reshape(bh, bw, 3)[...] = f[t:b, l:r]  # (only the crop box travels)
            dst = self.frame_u8 if B == 1 else self.frame_u8[i]
            if (bh, bw) == (H, W):
                self.ops.upload(dst, hraw[off:off + n])
            else:
                self.ops.upload(draw[off:off + n], hraw[off:off + n])
                self.ops.resample_rgb(draw[off:off + n], bh, bw, bw * 3, (0, 0, bw, bh), dst, H, W)
        self._launch_timed(overlap)

    def infer_raw_u8(self, frame) -> np.ndarray:
        """camera frame(s) of any size -> uint8 [H][W][3] ([B][H][W][3]): `infer_u8` of the centre-cropped, LANCZOS-resized frame(s)"""
        self.submit_raw_u8(frame)
        return self.collect_u8()

    def submit_raw_i420(self, frame, overlap: Optional[bool] = None, seeds=None):
        """`submit_raw_u8` for planar YUV 4:2:0 camera frames (`frames.I420Frame`, any size, odd sizes included; prepared with batch
        B > 1: a list of B frames, possibly of different sizes).  Per frame: the reference's crop box on the full frame size, widened
        to an even left / top edge so that it starts on a chroma sample; only those plane rectangles are copied into the pinned
        staging and uploaded (1.5 bytes per pixel); `i420_to_rgb` into device scratch (straight into `frame_u8` when the box already
        has the plan's size), `resample_rgb` of the box inside that rectangle into `frame_u8`; then `launch`.  The bytes of "convert
        the whole frame by the colour contract (include/vsd.h), crop, LANCZOS-resize with PIL".  seeds: see `submit_u8`."""
        from .frames import I420Frame

        p = self.plan
        seeds = self._check_seeds(seeds)
        H, W, B = p["H"], p["W"], p["batch"]

        def size_of(f):
            if not isinstance(f, I420Frame):
                raise ValueError(f"frame must be an I420Frame, got {type(f).__name__}")
            return f.width, f.height

        rects, total, scratch = [], 0, 0
        for f, (l, t, r, b) in self._raw_frames(frame, I420Frame, size_of):
            el, et = l & ~1, t & ~1
            rw, rh = r - el, b - et
            cw, ch = (rw + 1) // 2, (rh + 1) // 2
            ys, cs = _ru(rw, 4), _ru(cw, 4)  # (device rows start on a dword: the conversion's dword-wide form)
            rects.append((f, (l, t, r, b, el, et, rw, rh, cw, ch, ys, cs, total)))
            total += _ru(ys * rh + 2 * cs * ch, 256)
            if not ((r - l, b - t) == (W, H) and (el, et) == (l, t)):
                scratch = max(scratch, _ru(rw * 3, 4) * rh)
        hraw, draw = self._raw_staging(total)
        rgb = self.ops.workspace("i420_rgb", scratch) if scratch else None
        self._upload_seeds(seeds)
        hb = hraw.numpy()
        for i, (f, (l, t, r, b, el, et, rw, rh, cw, ch, ys, cs, off)) in enumerate(rects):
            ou, ov = off + ys * rh, off + ys * rh + cs * ch
            hb[off:ou].reshape(rh, ys)[:, :rw] = f.y[et:b, el:r]  # (only the crop box's plane rectangles travel)
            hb[ou:ov].reshape(ch, cs)[:, :cw] = f.u[et // 2:et // 2 + ch, el // 2:el // 2 + cw]
            hb[ov:ov + cs * ch].reshape(ch, cs)[:, :cw] = f.v[et // 2:et // 2 + ch, el // 2:el // 2 + cw]
            n = ys * rh + 2 * cs * ch
            self.ops.upload(draw[off:off + n], hraw[off:off + n])
            dst = self.frame_u8 if B == 1 else self.frame_u8[i]
            dy, du, dv = draw[off:ou], draw[ou:ov], draw[ov:ov + cs * ch]
            if (r - l, b - t) == (W, H) and (el, et) == (l, t):
                self.ops.i420_to_rgb(dy, ys, du, dv, cs, 0, 0, rh, rw, dst, W * 3)
            else:
                row = _ru(rw * 3, 4)
                self.ops.i420_to_rgb(dy, ys, du, dv, cs, 0, 0, rh, rw, rgb, row)
                self.ops.resample_rgb(rgb, rh, rw, row, (l - el, t - et, r - el, b - et), dst, H, W)
        self.last_upload_bytes = total  # (counted: what `upload` was handed; VideoSDPipeline.metrics reports it per frame)
        self._launch_timed(overlap)
        self._enqueue_i420()  # (behind the captured program at submit, as vsd_plan_submit_frame_i420 does: nothing is launched at collect)

    def _enqueue_i420(self):
        """`rgb_to_i420` of `out_u8` on the lane's stream into a device buffer of this engine (packed I420 per frame)"""
        p = self.plan
        H, W, B = p["H"], p["W"], p["batch"]
        if (H | W) & 1:
            raise ValueError(f"I420 output: a {W} x {H} frame has an odd side")
        one = H * W * 3 // 2
        st = self._i420_stage
        if st is None or st[0].numel() != B * one:
            st = (self.ops.empty(B * one, dtype=torch.uint8), torch.empty(B * one, dtype=torch.uint8, pin_memory=torch.cuda.is_available()))
            self._i420_stage = st
        dev = st[0]
        for i in range(B):
            o = i * one
            src = self.out_u8 if B == 1 else self.out_u8[i]
            self.ops.rgb_to_i420(src, H, W, dev[o:o + H * W], dev[o + H * W:o + H * W * 5 // 4], dev[o + H * W * 5 // 4:o + one])
        self._i420_queued = True

    def collect_i420(self):
        """Wait for the frame(s) enqueued by the last submit and bring them to the host as I420, 1.5 bytes per pixel through pinned
        memory.  After `submit_raw_i420` the conversion is already queued behind the program; after another submit it is launched here.
        Returns an `I420Frame` (a list of B)."""
        from .frames import I420Frame

        p = self.plan
        H, W, B = p["H"], p["W"], p["batch"]
        if not self._i420_queued:
            self._enqueue_i420()
        self._i420_queued = False
        dev, host = self._i420_stage
        one = H * W * 3 // 2
        _, _hin, _hout, e0, e1 = self._staging()
        self.ops.download_into(host, dev)
        self.family.get("in_flight", set()).discard(self)
        self.last_download_bytes = B * one
        if e0 is not None:
            self.last_gpu_ms = e0.elapsed_time(e1)  # the graph alone, as `collect_u8` reports it
        out = [I420Frame(host.numpy()[i * one:(i + 1) * one].copy(), W, H) for i in range(B)]
        return out[0] if B == 1 else out

    def infer_raw_i420(self, frame):
        """I420 camera frame(s) of any size -> I420Frame(s) of the plan's size"""
        self.submit_raw_i420(frame)
        return self.collect_i420()

    def collect_u8(self) -> np.ndarray:
        """Wait for the frame(s) enqueued by the last `submit_u8` and bring them to the host (a fresh array)."""
        want = self._want_shape()
        _, _hin, hout, e0, e1 = self._staging()
        self.ops.download_into(hout, self.out_u8)
        self.family.get("in_flight", set()).discard(self)
        if e0 is not None:
            self.last_gpu_ms = e0.elapsed_time(e1)  # the graph alone (between the H2D and the D2H copies)
        return hout.numpy().reshape(want).copy()

    def infer_u8(self, frame: np.ndarray) -> np.ndarray:
        """frame: uint8 [H][W][3] already cropped/resized by the caller -> uint8 [H][W][3]
        (prepared with batch B > 1: uint8 [B][H][W][3] -> [B][H][W][3])."""
        self.submit_u8(frame)
        return self.collect_u8()

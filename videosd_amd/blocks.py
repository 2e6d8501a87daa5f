"""The device blocks of constants a program reads besides the weights, and how they are laid out and filled: a prompt's cross-attention
constants (one per launch, or one slot per frame), the constants that depend on a frame's options, the copy lists of
`vsd_prompt_install`, and the installer of frame slots."""
from typing import Dict, List

import torch

from .lcm import LCMSchedule
from .lib import MIX_COPY, MIX_F16, MIX_F32, MIX_MAX
from .packing import PackedConv
from .packing import _round_up as _ru


class PromptLayout:
    """Byte layout of ONE prompt's device constants for a family of engines (same weights): per BasicTransformerBlock of the
    UNet / ControlNet its cross-attention K [tl][C] and V^T [C][ldt], and for the wide blocks the "absorbed" query / output
    weights (xa1: weights [heads*128][C] + ln_s / ln_t, xa2: weights [C][heads*128] + bias).  Everything lives in ONE
    contiguous buffer (~40 MB for SD1.5 + ControlNet), so that switching an engine to another cached prompt is a single
    device-to-device copy and a prompt cache entry is a single allocation."""

    def __init__(self, nets, tl: int):
        self.tl, self.ldt = tl, _ru(tl, 64)
        self.items = {}   # (net index, block index, name) -> (offset, shape, dtype)
        self.absorbed = set()
        off = 0

        def add(key, shape, dtype):
            nonlocal off
            n = 1
            for d in shape:
                n *= d
            self.items[key] = (off, tuple(shape), dtype)
            off = _ru(off + n * torch.empty(0, dtype=dtype).element_size(), 256)

        for ni, net in enumerate(nets):
            for bi, t in enumerate(net.transformers):
                c = t.kv2.n // 2
                add((ni, bi, "k"), (tl, c), torch.float16)
                add((ni, bi, "vt"), (c, self.ldt), torch.float16)
                if t.xa_raw is not None and tl <= 128:
                    hg = net.cfg.heads_for(c) * 128
                    self.absorbed.add((ni, bi))
                    add((ni, bi, "xa1_w"), (hg, c), torch.float16)
                    add((ni, bi, "xa1_s"), (hg,), torch.float32)
                    add((ni, bi, "xa1_t"), (hg,), torch.float32)
                    add((ni, bi, "xa2_w"), (c, hg), torch.float16)
                    add((ni, bi, "xa2_b"), (c,), torch.float16)
        self.nbytes = max(off, 256)


class FramePromptLayout:
    """Byte layout of the cross-attention constants of a launch whose B frames have prompts of their OWN (`Engine.prepare(frame_prompts=True)`):
    per BasicTransformerBlock K as [B*tl][C], frame b owning rows [b*tl, (b+1)*tl), and V^T as [C][B*ldt], frame b owning columns
    [b*ldt, (b+1)*ldt) with zeros beyond its tl keys -- what `attention(batch=B, k_brows=tl, vt_bcols=ldt)` reads.  No absorbed weights: they
    would be per frame too (B weight sets per layer), so every cross-attention of such a program runs in the explicit form."""

    def __init__(self, nets, tl: int, frames: int):
        self.tl, self.ldt, self.frames = tl, _ru(tl, 64), int(frames)
        self.items = {}
        self.absorbed = frozenset()
        off = 0
        for ni, net in enumerate(nets):
            for bi, t in enumerate(net.transformers):
                c = t.kv2.n // 2
                if c % 8:
                    raise ValueError(f"frame_prompts: a {c}-wide transformer block: rows must be whole 16-byte chunks (C a multiple of 8)")
                for name, shape in (("k", (self.frames * tl, c)), ("vt", (c, self.frames * self.ldt))):
                    self.items[(ni, bi, name)] = (off, shape, torch.float16)
                    off = _ru(off + shape[0] * shape[1] * 2, 256)
        self.nbytes = max(off, 256)


def prompt_segments(src: PromptLayout, dst: FramePromptLayout):
    """The copy list of `vsd_prompt_install` (include/vsd.h vsd_prompt_seg) that puts a cache entry of layout `src` into ONE frame slot of a
    block of layout `dst`: per tensor (src_off, dst_off, rows, row_bytes, dst_pitch, dst_frame_stride), bytes except the count `rows`.
    K is one run; V^T is C rows of ALL ldt columns (the zero padding travels with the data) at the destination's pitch."""
    if src.tl != dst.tl:
        raise ValueError(f"a prompt of {src.tl} tokens into a per-frame block of {dst.tl}: all frames of a launch must have the same text length")
    B, segs = dst.frames, []
    for key, (doff, _dshape, _dt) in dst.items.items():
        soff, sshape, _st = src.items[key]
        if key[2] == "k":
            n = sshape[0] * sshape[1] * 2
            segs.append((soff, doff, 1, n, B * n, n))
        else:
            c, ldt = sshape
            segs.append((soff, doff, c, ldt * 2, B * ldt * 2, ldt * 2))
    assert all(v % 16 == 0 for sg in segs for v in sg[:2] + sg[3:])
    return segs


# How every item NAME of a PromptLayout takes part in a prompt mix (include/vsd.h THE PROMPT MIX).  Linear in the text embeddings: K and V^T
# are to_k / to_v of them, xa1_w / xa1_s / xa1_t are G = scale * K_h * Wq_h and its LayerNorm fold, xa2_w is Z = Wo_h * V_h^T.  xa2_b is
# to_out.0.bias: it does not depend on the prompt and is copied, never summed.  A new item name has no entry here and `mix_segments` refuses
# it until someone decides which kind it is (tests/test_prompt_mix_host.py proves the linear ones linear).
MIX_ITEM_KINDS = {"k": MIX_F16, "vt": MIX_F16, "xa1_w": MIX_F16, "xa1_s": MIX_F32, "xa1_t": MIX_F32, "xa2_w": MIX_F16, "xa2_b": MIX_COPY}


def mix_segments(src: PromptLayout, dst):
    """The segment list of `vsd_prompt_mix` (include/vsd.h vsd_mix_seg) that writes a mix of prompts of layout `src` into a block of layout
    `dst`: per tensor (src_off, dst_off, rows, row_bytes, dst_pitch, dst_frame_stride, kind, 0).  `dst is src`: a whole block, every item one
    run in place.  `dst` a FramePromptLayout: ONE frame slot, the K / V^T segments of `prompt_segments` as fp16 mixes."""
    if dst is src:
        segs = []
        for (_ni, _bi, name), (off, shape, dtype) in src.items.items():
            if name not in MIX_ITEM_KINDS:
                raise ValueError(f"prompt mix: the item {name!r} of a prompt's constants has no entry in blocks.MIX_ITEM_KINDS: is it linear in "
                                 "the text embeddings, or independent of the prompt?")
            n = torch.empty(0, dtype=dtype).element_size()
            for d in shape:
                n *= d
            n = _ru(n, 16)  # (items start at multiples of 256: the bytes up to the next chunk are the block's own padding)
            segs.append((off, off, 1, n, n, n, MIX_ITEM_KINDS[name], 0))
    else:
        segs = [sg + (MIX_ITEM_KINDS[key[2]], 0) for sg, key in zip(prompt_segments(src, dst), dst.items)]
    assert all(v % 16 == 0 for sg in segs for v in sg[:2] + sg[3:6])
    return segs


class OptionLayout:
    """Byte layout of the constants that depend on a frame's OPTIONS (`Engine.prepare(frame_options=True)`) for `frames` frames: per item a
    run of `frames` slots of equal size, frame f owning bytes [off + f * size, off + (f + 1) * size) --
      "coef": fp32 [coef_stride]: [0:2] the add_noise coefficients, [2 + 6i : 8 + 6i] the scheduler coefficients of step i (the layout of
              the default program's constant block), padded to whole 16-byte units;
      one item per network ("unet", "cn"): fp16 [n][cols], its per-step time-embedding projections (conv1's bias folded in).
    frames = 1 is the layout of an option ENTRY (one schedule's constants, a cache entry); an engine's own block has its batch size.  Every
    offset and size is a multiple of 16 bytes: a slot is installed by `prompt_install`, a segmented copy of 16-byte chunks."""

    def __init__(self, n: int, cols: Dict[str, int], frames: int):
        self.n, self.frames, self.cols = int(n), int(frames), dict(cols)
        self.coef_stride = _ru(2 + 6 * self.n, 4)  # floats
        self.items = {}  # name -> (offset, bytes per frame)
        off = 0
        for name, nb in [("coef", self.coef_stride * 4)] + [(k, self.n * c * 2) for k, c in self.cols.items()]:
            if nb % 16:
                raise ValueError(f"frame_options: {name}: {nb} bytes per frame: the time tables' columns must be a multiple of 8")
            self.items[name] = (off, nb)
            off = _ru(off + self.frames * nb, 256)
        self.nbytes = max(off, 256)

    def view(self, buf, name, frame: int = 0):
        """frame `frame`'s slot of item `name` in `buf` (bytes of this layout): fp32 [coef_stride], or fp16 [n][cols]"""
        off, nb = self.items[name]
        raw = buf[off + frame * nb:off + (frame + 1) * nb]
        return raw.view(torch.float32) if name == "coef" else raw.view(torch.float16).view(self.n, self.cols[name])


def option_segments(src: OptionLayout, dst: OptionLayout):
    """The copy list of `vsd_prompt_install` (include/vsd.h vsd_prompt_seg) that puts an option entry (layout `src`, one frame) into ONE frame
    slot of an engine's block (layout `dst`): per item one run (src_off, dst_off, 1, bytes, frames * bytes, bytes)."""
    if src.frames != 1 or src.n != dst.n or src.cols != dst.cols:
        raise ValueError("an option entry of another schedule length or other networks than the block it is installed into")
    segs = [(src.items[k][0], doff, 1, nb, dst.frames * nb, nb) for k, (doff, nb) in dst.items.items()]
    assert all(v % 16 == 0 for sg in segs for v in sg[:2] + sg[3:])
    return segs


class OptionEntry:
    """One schedule's constants in device memory (layout: OptionLayout with one frame): what every `strength` that gives these timesteps
    shares.  Engines read THEIR OWN block; an entry is installed into a frame slot by copying."""

    def __init__(self, layout: OptionLayout, buf, timesteps):
        self.layout, self.buf, self.timesteps = layout, buf, tuple(timesteps)
        self.sched, self.cn, self.epoch = None, True, 0  # what `Engine._fill_option_entry` rebuilds it from, and the "weights_epoch" it was built under


def schedule_constants(sched: LCMSchedule) -> List[float]:
    """A schedule's floats of the constant block: [0:2] the add_noise coefficients, [2 + 6i : 8 + 6i] the scheduler coefficients of step i"""
    vals = list(sched.add_noise_coef())
    for i in range(len(sched)):
        vals += [float(x) for x in sched.step_coef(i)]
    return vals


def controlnet_scales(nres: int, controlnet_scale: float):
    """ControlNetModel guess mode: logspace(-1, 0, nres) * conditioning_scale (always on: lcm_controlnet.py:399,447), fp32"""
    return torch.logspace(-1, 0, nres) * float(controlnet_scale)


FRAME_OPTION_OPS = ("add_noise_frames", "lcm_step_frames", "groupnorm_addvec", "cn_merge_frames", "prompt_install")
MAX_OPTION_ENTRIES = 64  # (at most 50 timestep tuples per `steps`; an entry is a few hundred KB)


class PromptBlock:
    """One prompt's constants in device memory (layout: PromptLayout).  Engines read THEIR OWN block (its addresses are in
    their captured graphs); a cached prompt is installed by copying its block over the engine's."""

    def __init__(self, ops, layout: PromptLayout):
        self.layout = layout
        self.buf = ops.zeros(layout.nbytes, dtype=torch.uint8)  # zero: V^T key padding and the unused rows of the xa weights
        self._xa = {}
        self.text = None
        self.epoch = 0  # the family's "weights_epoch" (LoRA scale changes) the constants were built under

    def view(self, ni, bi, name):
        off, shape, dtype = self.layout.items[(ni, bi, name)]
        n = 1
        for d in shape:
            n *= d
        return self.buf[off:off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(*shape)

    def kv(self, ni, bi):
        return self.view(ni, bi, "k"), self.view(ni, bi, "vt")

    def xa(self, ni, bi):
        """(xa1, xa2) PackedConv pair of an absorbed block (views into this block), or None"""
        if (ni, bi) not in self.layout.absorbed:
            return None
        got = self._xa.get((ni, bi))
        if got is None:
            w1, w2 = self.view(ni, bi, "xa1_w"), self.view(ni, bi, "xa2_w")
            hg, c = w1.shape
            x1 = PackedConv(w1, None, hg, c, c, c, 1, ln_s=self.view(ni, bi, "xa1_s"), ln_t=self.view(ni, bi, "xa1_t"), tile128=True)
            x2 = PackedConv(w2, self.view(ni, bi, "xa2_b"), c, hg, hg, hg, 1)
            got = self._xa[(ni, bi)] = (x1, x2)
        return got


class PromptMix:
    """A weighted mix of cached prompts (include/vsd.h THE PROMPT MIX): 1..4 PromptBlocks of ONE layout and their fp32 weights (made to sum
    to 1 by promptmix.normalized).  It has no bytes of its own: an engine forms it in its own block, or in a frame slot, by one
    `prompt_mix` launch.  It holds references to its components, so a component evicted from a prompt cache lives as long as something
    that reads it."""

    def __init__(self, components, weights):
        self.components, self.weights = tuple(components), tuple(float(w) for w in weights)
        if not 1 <= len(self.components) <= MIX_MAX or len(self.weights) != len(self.components):
            raise ValueError(f"a prompt mix has 1..{MIX_MAX} components and one weight each, got {len(self.components)} component(s) and "
                             f"{len(self.weights)} weight(s)")
        if any(not (w >= 0.0 and w != float("inf")) for w in self.weights):
            raise ValueError(f"the weights of a prompt mix are finite and not negative, got {list(self.weights)}")
        self.layout = self.components[0].layout
        if any(c.layout is not self.layout for c in self.components):
            raise ValueError(f"all components of a prompt mix must have the same text length, got {[c.layout.tl for c in self.components]}")

    def same_as(self, other) -> bool:
        """the same component blocks with the same weights: what is installed need not be formed again"""
        return (isinstance(other, PromptMix) and len(other.components) == len(self.components) and
                all(a is b for a, b in zip(self.components, other.components)) and self.weights == other.weights)


def same_source(a, b) -> bool:
    """do the sources `a` and `b` of a prompt install give the same bytes without looking at them? (the same object, or equal mixes)"""
    return a is b or (isinstance(a, PromptMix) and a.same_as(b))


class FrameSlots:
    """The frame slots of a device block (`buf`, laid out by `layout`, one slot per frame of a launch): which source each slot holds (a
    reference: the source outlives its install), and `prompt_install` -- `prompt_mix` for a PromptMix -- for every slot whose source
    changed.  A source is anything with `.buf` and `.layout` (a PromptBlock, an OptionEntry), or a PromptMix of such."""

    def __init__(self, buf, layout):
        self.buf, self.layout = buf, layout
        self.src = [None] * layout.frames

    def install(self, ops, want, seg_table):
        """want: one source per slot; seg_table(source layout, this layout[, mix=True]) -> (device table, segments)"""
        for f, s in enumerate(want):
            if not same_source(s, self.src[f]):
                if isinstance(s, PromptMix):
                    tab, nseg = seg_table(s.layout, self.layout, mix=True)
                    ops.prompt_mix([c.buf for c in s.components], s.weights, self.buf, tab, nseg, f)
                else:
                    tab, nseg = seg_table(s.layout, self.layout)
                    ops.prompt_install(s.buf, self.buf, tab, nseg, f)
                self.src[f] = s

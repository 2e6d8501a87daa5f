"""Device-resident, kernel-layout weights of the networks an engine runs: UNet / ControlNet encoder (NetWeights) and TAESD."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .config import ControlNetConfig, UNetConfig
from .packing import PackedConv, add_frag, pack_conv, pack_geglu_ln, pack_linear, pack_linear_cat, pack_linear_ln
from .weights import skip_channels


@dataclass
class Place:
    """Where one checkpoint weight landed in the kernel-layout buffers: what THE ADAPTER FUSE (include/vsd.h) needs to write a fused weight
    over it.  `pack.weight` rows [row0, row0 + rows) (through `geglu`'s tile map), columns [0, pack.k)."""
    pack: PackedConv
    rows: int
    row0: int = 0
    geglu: bool = False                 # rows go through the GEGLU tile map of packing.pack_geglu
    cin_pad: Optional[int] = None       # a conv: k = (ky, kx, c) with c padded to this (None: as in the checkpoint)
    fold: Optional[tuple] = None        # (gamma, beta) of the LayerNorm folded in (checkpoint tensors): pack.ln_s / pack.ln_t follow the weight
    fold_bias: Optional[torch.Tensor] = None  # ... and the bias packing._fold_ln adds to ln_t
    raw_copy: Optional[torch.Tensor] = None   # a second copy of the raw fp16 weight [rows][k] (BlockW.xa_raw[0])
    frag: bool = False                  # pack.weight_frag is a second, fragment-major copy of pack.weight


@dataclass
class ResnetW:
    cin: int
    cout: int
    n1: Tuple[torch.Tensor, torch.Tensor]
    conv1: PackedConv          # bias folded into the time projection
    n2: Tuple[torch.Tensor, torch.Tensor]
    conv2: PackedConv
    shortcut: Optional[PackedConv]
    temb_off: int              # column offset into the concatenated time-projection output


@dataclass
class BlockW:
    """One BasicTransformerBlock."""
    qkv: PackedConv            # LayerNorm norm1 folded in (pack_linear_ln)
    out1: PackedConv
    q2: PackedConv             # norm2 folded in
    kv2: PackedConv
    out2: PackedConv
    ff1: PackedConv            # norm3 folded in, GEGLU tile-packed
    ff2: PackedConv
    kv_index: int              # index of this block's entries in a prompt's constants (PromptLayout)
    # "absorbed" cross-attention (C >= XATTN_ABSORB_MIN_C): the text's key / value projections folded into the query and
    # output weights, rebuilt per prompt on the GPU (vsd_xattn_fold); what that needs besides out2: device copies of
    xa_raw: Optional[tuple] = None     # (raw to_q weight fp16 [C][C], norm2 gamma, norm2 beta)


@dataclass
class TransformerW:
    """Transformer2DModel: GroupNorm, proj_in, `depth` blocks (1 for SD1.5; 2 / 10 for SDXL), proj_out."""
    c: int
    norm: Tuple[torch.Tensor, torch.Tensor]
    proj_in: PackedConv
    blocks: List[BlockW]
    proj_out: PackedConv


# Cross-attention as two GEMMs pays when one 128-column tile per head is not wider than the query projection it
# replaces: 8 heads * 128 = 1024 columns against C (SD1.5: the 640- and 1280-wide levels; see pack_cross_attention)
XATTN_ABSORB_MIN_C = 640


class NetWeights:
    """Device-resident, kernel-layout weights of one UNet-shaped network (UNet or ControlNet encoder)."""

    def __init__(self, ops, cfg: UNetConfig, w: Dict[str, torch.Tensor], is_controlnet=False,
                 cn_cfg: Optional[ControlNetConfig] = None, absorb_min_c: int = XATTN_ABSORB_MIN_C):
        self.ops, self.cfg, self.is_cn = ops, cfg, is_controlnet
        self.absorb_min_c = absorb_min_c  # blocks at least this wide keep what the absorbed cross-attention needs (xa_raw)
        self._w = w
        self._temb_w, self._temb_b = [], []
        self._temb_cols = 0
        self.transformers: List[BlockW] = []  # every BasicTransformerBlock, in kv_cache order
        self.places: Dict[str, Place] = {}    # checkpoint name of every kind-"w" weight -> where it landed (host-side bookkeeping only)
        self._temb_names = []
        dev = ops.to_device
        ch = cfg.block_out_channels
        self.conv_in = self._conv("conv_in", cin_pad=8)
        self.time_l1 = self._lin("time_embedding.linear_1")
        self.time_l2 = self._lin("time_embedding.linear_2")
        self.cond_proj = self._lin("time_embedding.cond_proj") if cfg.cond_proj_dim else None
        self.add_l1 = self._lin("add_embedding.linear_1") if cfg.add_time_dim else None
        self.add_l2 = self._lin("add_embedding.linear_2") if cfg.add_time_dim else None
        self.down: List[List[Tuple[ResnetW, Optional[TransformerW]]]] = []
        self.downsamplers: List[Optional[PackedConv]] = []
        cin = ch[0]
        for i, cout in enumerate(ch):
            blk = []
            for j in range(cfg.layers_per_block):
                r = self._resnet(f"down_blocks.{i}.resnets.{j}", cin if j == 0 else cout, cout)
                t = (self._transformer(f"down_blocks.{i}.attentions.{j}", cout, cfg.transformer_depth[i])
                     if cfg.down_attn[i] else None)
                blk.append((r, t))
            self.down.append(blk)
            self.downsamplers.append(self._conv(f"down_blocks.{i}.downsamplers.0.conv") if i < len(ch) - 1 else None)
            cin = cout
        self.mid = (self._resnet("mid_block.resnets.0", ch[-1], ch[-1]),
                    self._transformer("mid_block.attentions.0", ch[-1], cfg.mid_depth),
                    self._resnet("mid_block.resnets.1", ch[-1], ch[-1]))
        if not is_controlnet:
            skips = skip_channels(cfg)
            rev = list(reversed(ch))
            self.up: List[List[Tuple[ResnetW, Optional[TransformerW]]]] = []
            self.upsamplers: List[Optional[PackedConv]] = []
            prev = ch[-1]
            for i, cout in enumerate(rev):
                blk = []
                for j in range(cfg.layers_per_block + 1):
                    sc = skips.pop()
                    r = self._resnet(f"up_blocks.{i}.resnets.{j}", (prev if j == 0 else cout) + sc, cout)
                    t = (self._transformer(f"up_blocks.{i}.attentions.{j}", cout, cfg.up_depth[i])
                         if cfg.up_attn[i] else None)
                    blk.append((r, t))
                self.up.append(blk)
                self.upsamplers.append(self._conv(f"up_blocks.{i}.upsamplers.0.conv") if i < len(rev) - 1 else None)
                prev = cout
            self.norm_out = self._norm("conv_norm_out")
            self.conv_out = self._conv("conv_out")
        else:
            cc = cn_cfg.cond_channels
            p = "controlnet_cond_embedding"
            self.cond_convs = [(self._conv(f"{p}.conv_in", cin_pad=8), 1)]
            k = 0
            for i in range(len(cc) - 1):
                self.cond_convs.append((self._conv(f"{p}.blocks.{k}"), 1))
                self.cond_convs.append((self._conv(f"{p}.blocks.{k + 1}"), 2))
                k += 2
            self.cond_out = self._conv(f"{p}.conv_out")
            self.zero_convs = [self._conv(f"controlnet_down_blocks.{i}") for i in range(len(skip_channels(cfg)))]
            self.zero_mid = self._conv("controlnet_mid_block")
        # all per-ResnetBlock time projections as ONE linear layer: [sum Cout][temb_dim]
        tw = pack_linear_cat(self._temb_w, self._temb_b)
        self.temb_proj = self._to_dev(tw)
        for name, off, rows in self._temb_names:
            self.places[name] = Place(self.temb_proj, rows, row0=off)
        self._w = None
        self._temb_w = self._temb_b = None

    # --- helpers
    def _to_dev(self, p: PackedConv) -> PackedConv:
        for f in ("weight", "bias", "ln_s", "ln_t", "weight_frag"):
            v = getattr(p, f)
            if v is not None:
                setattr(p, f, self.ops.to_device(v.contiguous()))
        return p

    def _conv(self, name, cin_pad=None, with_bias=True) -> PackedConv:
        b = self._w.get(name + ".bias") if with_bias else None
        p = self._to_dev(pack_conv(self._w[name + ".weight"], b, cin_pad=cin_pad))
        self.places[name + ".weight"] = Place(p, p.n, cin_pad=cin_pad)
        return p

    def _lin(self, name) -> PackedConv:
        p = self._to_dev(pack_linear(self._w[name + ".weight"], self._w.get(name + ".bias")))
        self.places[name + ".weight"] = Place(p, p.n)
        return p

    def _norm(self, name):
        return (self.ops.to_device(self._w[name + ".weight"].half().contiguous()),
                self.ops.to_device(self._w[name + ".bias"].half().contiguous()))

    def _resnet(self, p, cin, cout) -> ResnetW:
        off = self._temb_cols
        self._temb_w.append(self._w[p + ".time_emb_proj.weight"])
        self._temb_names.append((p + ".time_emb_proj.weight", off, cout))
        # conv1's bias is folded into the time projection's bias: both are per-channel constants added
        # to conv1's output before norm2 (ResnetBlock2D.forward).
        self._temb_b.append((self._w[p + ".time_emb_proj.bias"].float() + self._w[p + ".conv1.bias"].float()))
        self._temb_cols += cout
        sc = self._conv(p + ".conv_shortcut") if (p + ".conv_shortcut.weight") in self._w else None
        return ResnetW(cin, cout, self._norm(p + ".norm1"), self._conv(p + ".conv1", with_bias=False),
                       self._norm(p + ".norm2"), self._conv(p + ".conv2"), sc, off)

    def _transformer(self, p, c, depth=1) -> TransformerW:
        w = self._w
        blocks = []
        for kb in range(depth):
            b = f"{p}.transformer_blocks.{kb}"
            ln = lambda n: (w[f"{b}.{n}.weight"], w[f"{b}.{n}.bias"])  # noqa: E731
            qkv = self._to_dev(pack_linear_ln([w[f"{b}.attn1.to_q.weight"], w[f"{b}.attn1.to_k.weight"],
                                               w[f"{b}.attn1.to_v.weight"]], None, *ln("norm1")))
            q2 = self._to_dev(pack_linear_ln([w[f"{b}.attn2.to_q.weight"]], None, *ln("norm2")))
            kv2 = self._to_dev(pack_linear_cat([w[f"{b}.attn2.to_k.weight"], w[f"{b}.attn2.to_v.weight"]]))
            ff1 = self._to_dev(pack_geglu_ln(w[f"{b}.ff.net.0.proj.weight"], w[f"{b}.ff.net.0.proj.bias"], *ln("norm3")))
            blk = BlockW(qkv, self._lin(b + ".attn1.to_out.0"), q2, kv2, self._lin(b + ".attn2.to_out.0"), ff1,
                         self._lin(b + ".ff.net.2"), len(self.transformers))
            for i, n in enumerate(("to_q", "to_k", "to_v")):
                self.places[f"{b}.attn1.{n}.weight"] = Place(qkv, c, row0=i * c, fold=ln("norm1"))
            self.places[f"{b}.attn2.to_q.weight"] = Place(q2, c, fold=ln("norm2"))
            self.places[f"{b}.attn2.to_k.weight"] = Place(kv2, c, row0=0)
            self.places[f"{b}.attn2.to_v.weight"] = Place(kv2, c, row0=c)
            self.places[f"{b}.ff.net.0.proj.weight"] = Place(ff1, ff1.n, geglu=True, fold=ln("norm3"), fold_bias=w[f"{b}.ff.net.0.proj.bias"])
            heads = self.cfg.heads_for(c)
            if c >= self.absorb_min_c and c % heads == 0 and c % 64 == 0 and (c // heads) % 8 == 0:
                dv = lambda t: self.ops.to_device(t.detach().to(torch.float16).contiguous())  # noqa: E731
                blk.xa_raw = (dv(w[f"{b}.attn2.to_q.weight"]), dv(ln("norm2")[0]), dv(ln("norm2")[1]))
                self.places[f"{b}.attn2.to_q.weight"].raw_copy = blk.xa_raw[0]
            self.transformers.append(blk)
            blocks.append(blk)
        # use_linear_projection (SDXL): Linear on the token matrix == the 1x1 conv of SD1.5 in this layout
        proj = self._lin if self.cfg.linear_proj else self._conv
        tw = TransformerW(c, self._norm(p + ".norm"), proj(p + ".proj_in"), blocks, proj(p + ".proj_out"))
        if c == getattr(self.ops, "TAIL_C", 0) and depth == 1:
            # the fused per-token chains (csrc/fused_tail.hip) read these six matrices fragment-major
            for pc in (blocks[0].out1, blocks[0].q2, blocks[0].out2, blocks[0].ff1, blocks[0].ff2, tw.proj_out):
                pc.weight_frag = self.ops.to_device(add_frag(PackedConv(pc.weight.cpu(), None, pc.n, pc.k, pc.kp, pc.cin, pc.ksize)).weight_frag)
            for pl in self.places.values():
                pl.frag = pl.pack.weight_frag is not None
        return tw


class TAESDWeights:
    def __init__(self, ops, w: Dict[str, torch.Tensor]):
        self.ops = ops

        def cv(name, cin_pad=None):
            p = pack_conv(w[name + ".weight"], w.get(name + ".bias"), cin_pad=cin_pad)
            p.weight = ops.to_device(p.weight)
            if p.bias is not None:
                p.bias = ops.to_device(p.bias)
            return p

        def blk(p):
            return [cv(f"{p}.conv.{k}") for k in (0, 2, 4)]

        e = "encoder.layers"
        self.enc_in = cv(f"{e}.0", cin_pad=8)
        self.enc_blocks0 = [blk(f"{e}.1")]
        self.enc_stages = []
        n = 2
        for _ in range(3):
            down = cv(f"{e}.{n}")
            n += 1
            bs = []
            for _ in range(3):
                bs.append(blk(f"{e}.{n}"))
                n += 1
            self.enc_stages.append((down, bs))
        self.enc_out = cv(f"{e}.{n}")
        d = "decoder.layers"
        self.dec_in = cv(f"{d}.0", cin_pad=8)
        self.dec_stages = []
        n = 2
        for nb in (3, 3, 3):
            bs = []
            for _ in range(nb):
                bs.append(blk(f"{d}.{n}"))
                n += 1
            n += 1
            up = cv(f"{d}.{n}")
            n += 1
            self.dec_stages.append((bs, up))
        self.dec_last_block = blk(f"{d}.{n}")
        n += 1
        self.dec_out = cv(f"{d}.{n}")

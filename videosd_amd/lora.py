"""LoRA adapter files for the UNet (include/vsd.h THE ADAPTER FUSE): reading them, and the device-side set an engine fuses from.

Files are safetensors.  Two key conventions are read, both RESTATED from the public formats (neither `peft` nor `diffusers` is a dependency
and no file written by them has gone through this code; the conventions are unpinned):
  PEFT / diffusers   unet.<module>.lora_A.weight (down) / unet.<module>.lora_B.weight (up); older files: <module>.lora.down.weight /
                     <module>.lora.up.weight; optional <module>.alpha
  kohya              lora_unet_<module with _ for .>.lora_down.weight / .lora_up.weight / .alpha; the underscored name is looked up in a
                     table built from the UNet's own tensor names (weights.unet_spec), never split by guessing
A module is a tensor of kind "w" of the spec without its ".weight".  Without an alpha key alpha = rank.  Anything else is refused with an
error that names the first offending key and says how many there are: a picture that silently differs from what the file means is not
served.  Text-encoder keys are refused too, unless skip_text_encoder=True drops (and counts) them.  The ControlNet is never adapted."""
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import lib as L

MAX_ADAPTERS = L.LORA_MAX
MAX_RANK = L.LORA_MAX_RANK

_OTHER_METHODS = ("dora_scale", "lora_magnitude_vector", "hada_", "lokr_", ".on_input", "lora_mid")  # DoRA / LoHa / LoKr / LoCon mid
_SDXL = ("lora_te1_", "lora_te2_", "text_encoder_2.", "lora_unet_input_blocks_", "lora_unet_output_blocks_", "lora_unet_middle_block_",
         "add_embedding", "label_emb")
_TEXT = ("lora_te_", "text_encoder.", "lora_te.")


class AdapterError(ValueError):
    pass


@dataclass
class AdapterTensor:
    up: torch.Tensor      # fp16 [rows][r]
    down: torch.Tensor    # fp16 [r] + the checkpoint tensor's shape[1:]
    a: float              # fp32(alpha / r), as a Python float holding that fp32 value
    rank: int


@dataclass
class Adapter:
    name: str
    tensors: Dict[str, AdapterTensor] = field(default_factory=dict)  # by checkpoint tensor name ("….weight")
    text_encoder_keys_skipped: int = 0
    path: Optional[str] = None


def module_table(spec) -> Dict[str, tuple]:
    """{module: shape} of every adaptable tensor of the spec"""
    return {n[:-len(".weight")]: tuple(sh) for n, sh, kind in spec if kind == "w" and n.endswith(".weight")}


def kohya_table(spec) -> Dict[str, str]:
    """{module with _ for .: module}; two modules that collapse to one underscored name would make the convention ambiguous"""
    out = {}
    for m in module_table(spec):
        u = m.replace(".", "_")
        if u in out:
            raise AdapterError(f"the UNet's modules {out[u]!r} and {m!r} share the kohya name {u!r}")
        out[u] = m
    return out


def _refuse(what: str, keys: List[str]):
    raise AdapterError(f"adapter file: {what}: {keys[0]!r}" + (f" and {len(keys) - 1} more" if len(keys) > 1 else "") + f" ({len(keys)} in all)")


_PEFT = re.compile(r"^(?:unet\.)?(?P<mod>.+?)\.(?:(?P<a>lora_A|lora\.down|lora_down)|(?P<b>lora_B|lora\.up|lora_up))\.weight$")
_PEFT_ALPHA = re.compile(r"^(?:unet\.)?(?P<mod>.+?)\.alpha$")
_KOHYA = re.compile(r"^lora_unet_(?P<mod>[^.]+)\.(?:(?P<a>lora_down\.weight)|(?P<b>lora_up\.weight)|(?P<alpha>alpha))$")


def parse_adapter(tensors: Dict[str, object], spec, skip_text_encoder: bool = False, name: str = "") -> Adapter:
    """tensors: {key: torch tensor or numpy array} as read from a safetensors file; spec: weights.unet_spec(cfg) of the UNet it is for"""
    mods = module_table(spec)
    kohya = kohya_table(spec)
    keys = sorted(tensors)
    bad = [k for k in keys if any(s in k for s in _OTHER_METHODS)]
    if bad:
        _refuse("DoRA / LoHa / LoKr keys are not LoRA", bad)
    bad = [k for k in keys if any(s in k for s in _SDXL)]
    if bad:
        _refuse("keys of an SDXL pipeline", bad)
    text = [k for k in keys if k.startswith(_TEXT)]
    if text and not skip_text_encoder:
        _refuse("text-encoder keys (pass lora_skip_text_encoder=True to drop them: the pictures then differ from what the file means)", text)
    parts: Dict[str, dict] = {}
    unknown, order = [], []
    for k in keys:
        if k in text:
            continue
        mod = which = None
        m = _KOHYA.match(k)
        if m:
            mod = kohya.get(m.group("mod"))
            which = "down" if m.group("a") else "up" if m.group("b") else "alpha"
        else:
            m = _PEFT.match(k)
            if m:
                mod, which = m.group("mod"), "down" if m.group("a") else "up"
            else:
                m = _PEFT_ALPHA.match(k)
                if m:
                    mod, which = m.group("mod"), "alpha"
        if mod is None or mod not in mods:
            unknown.append(k)
            continue
        if mod not in parts:
            order.append(mod)
        parts.setdefault(mod, {})[which] = k
    if unknown:
        _refuse("keys that match no UNet tensor", unknown)
    unpaired = [p.get("down") or p.get("up") or p["alpha"] for p in parts.values() if "down" not in p or "up" not in p]
    if unpaired:
        _refuse("a module needs both its down and its up matrix", unpaired)
    out = Adapter(name=name, text_encoder_keys_skipped=len(text))
    misfit, too_wide, nonfinite = [], [], []
    for mod in order:
        p = parts[mod]
        shape = mods[mod]
        down = torch.as_tensor(np.asarray(tensors[p["down"]]) if not isinstance(tensors[p["down"]], torch.Tensor) else tensors[p["down"]])
        up = torch.as_tensor(np.asarray(tensors[p["up"]]) if not isinstance(tensors[p["up"]], torch.Tensor) else tensors[p["up"]])
        r = int(down.shape[0]) if down.dim() else 0
        one = (1,) * (len(shape) - 2)
        down_ok = r >= 1 and (tuple(down.shape) == (r,) + shape[1:] or (all(d == 1 for d in shape[2:]) and tuple(down.shape) in ((r, shape[1]), (r, shape[1], 1, 1))))
        up_ok = tuple(up.shape) in ((shape[0], r), (shape[0], r, 1, 1), (shape[0], r) + one)
        if not down_ok:
            misfit.append(p["down"])
            continue
        if not up_ok:
            misfit.append(p["up"])
            continue
        if r > MAX_RANK:
            too_wide.append(p["down"])
            continue
        alpha = float(r)
        if "alpha" in p:
            av = tensors[p["alpha"]]
            alpha = float(av.item() if hasattr(av, "item") else av)
        down16 = down.detach().to("cpu", torch.float16).reshape((r,) + shape[1:]).contiguous()
        up16 = up.detach().to("cpu", torch.float16).reshape(shape[0], r).contiguous()
        a = float(np.float32(alpha / r))
        for key, t in ((p["down"], down16), (p["up"], up16)):
            if not bool(torch.isfinite(t).all()):
                nonfinite.append(key)
        if not np.isfinite(a):
            nonfinite.append(p.get("alpha", p["down"]))
        out.tensors[mod + ".weight"] = AdapterTensor(up16, down16, a, r)
    if misfit:
        _refuse("shapes that do not fit the UNet tensor", misfit)
    if too_wide:
        _refuse(f"rank above {MAX_RANK}", too_wide)
    if nonfinite:
        _refuse("values that are not finite (as fp16)", nonfinite)
    if not out.tensors:
        raise AdapterError("adapter file: no UNet tensor is adapted (0 in all)")
    return out


def load_adapter(path: str, spec, skip_text_encoder: bool = False, name: Optional[str] = None) -> Adapter:
    if not str(path).endswith(".safetensors"):
        raise AdapterError(f"adapter file: {path!r}: safetensors files only")
    from safetensors.torch import load_file

    ad = parse_adapter(load_file(path), spec, skip_text_encoder=skip_text_encoder, name=name or str(path))
    ad.path = str(path)
    return ad


def pack_down(down: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """an adapter's down matrix in the k order of the packed weight it goes into: [r][cin] as it is; a conv's [r][cin][kh][kw] ->
    [r][(ky, kx, c)] with the input channels zero-padded as packing.pack_conv pads the weight's"""
    if down.dim() == 2:
        return down.contiguous()
    d = down.permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad != d.shape[-1]:
        d = torch.nn.functional.pad(d, (0, cin_pad - d.shape[-1]))
    return d.reshape(d.shape[0], -1).contiguous()


class AdapterSet:
    """What an engine fuses from (Engine.load_adapters): per checkpoint tensor that some adapter touches, the base copy W0 in the packed k
    order, the adapters' up / down matrices and fold vectors on the device, and ONE table of vsd_lora_seg naming where
    `NetWeights.places` says the tensor landed.  Also the load-time bytes of every LayerNorm-fold vector it will overwrite: with every
    scale zero the weights come back by the arithmetic, the fold vectors (summed in another order at load) by copy."""

    def __init__(self, ops, net, weights: Dict[str, torch.Tensor], adapters: List[Adapter]):
        from .packing import pack_conv

        if not 1 <= len(adapters) <= MAX_ADAPTERS:
            raise AdapterError(f"{len(adapters)} adapters: 1..{MAX_ADAPTERS} can be loaded at once")
        self.adapters = list(adapters)
        self.names = [a.name for a in adapters]
        if len(set(self.names)) != len(self.names):
            raise AdapterError(f"adapter names must differ, got {self.names}")
        self.scales = (0.0,) * len(adapters)
        self._keep = []          # every device tensor the table points at
        self._f32 = {}           # id of a checkpoint vector -> its fp32 device copy
        self._saved_fold = {}    # id of a pack -> (pack, load-time ln_s, load-time ln_t)
        self.base_bytes = 0
        touched = sorted({n for a in adapters for n in a.tensors})
        missing = [n for n in touched if n not in net.places]
        if missing:
            _refuse("tensors this network has no place for", missing)
        dev = lambda t: self._hold(ops.to_device(t.contiguous()))  # noqa: E731
        segs = []
        for name in touched:
            pl = net.places[name]
            w = weights[name].detach()
            k = pl.pack.k
            if w.dim() == 4:
                w0 = pack_conv(w.cpu(), None, cin_pad=pl.cin_pad).weight[:, :k]
            else:
                w0 = w.cpu().to(torch.float16)
            if tuple(w0.shape) != (pl.rows, k):
                raise AdapterError(f"{name}: the checkpoint tensor is {tuple(w0.shape)} in the packed order, its place {(pl.rows, k)}")
            w0 = dev(w0)
            self.base_bytes += w0.numel() * 2
            s = L.LoraSeg()
            s.w0, s.dst = w0.data_ptr(), pl.pack.weight.data_ptr()
            s.rows, s.k, s.kp, s.row0 = pl.rows, k, pl.pack.kp, pl.row0
            s.map = L.LORA_MAP_GEGLU if pl.geglu else L.LORA_MAP_ID
            i = 0
            for slot, a in enumerate(adapters):
                t = a.tensors.get(name)
                if t is None:
                    continue
                s.up[i], s.down[i] = dev(t.up).data_ptr(), dev(pack_down(t.down, pl.cin_pad)).data_ptr()
                s.rank[i], s.slot[i], s.a[i] = t.rank, slot, t.a
                i += 1
            s.n = i
            if pl.fold is not None:
                s.gamma, s.beta = self._vec(ops, pl.fold[0]).data_ptr(), self._vec(ops, pl.fold[1]).data_ptr()
                s.ln_s, s.ln_t = pl.pack.ln_s.data_ptr(), pl.pack.ln_t.data_ptr()
                if pl.fold_bias is not None:
                    s.bias = self._vec(ops, pl.fold_bias).data_ptr()
                if id(pl.pack) not in self._saved_fold:
                    self._saved_fold[id(pl.pack)] = (pl.pack, self._hold(pl.pack.ln_s.clone()), self._hold(pl.pack.ln_t.clone()))
            if pl.frag:
                s.copy_kind, s.copy = L.LORA_COPY_FRAG, pl.pack.weight_frag.data_ptr()
            elif pl.raw_copy is not None:
                s.copy_kind, s.copy = L.LORA_COPY_RAW, pl.raw_copy.data_ptr()
            segs.append(s)
            if pl.frag and pl.raw_copy is not None:
                # both second copies (an absorbed block at the fused tail's width): the raw copy through a segment of its own, whose plain
                # destination is scratch
                r = L.LoraSeg.from_buffer_copy(bytes(s))
                scratch = self._hold(ops.empty(pl.rows, pl.pack.kp))
                r.dst, r.row0, r.map = scratch.data_ptr(), 0, L.LORA_MAP_ID
                r.gamma = r.beta = r.bias = r.ln_s = r.ln_t = None
                r.copy_kind, r.copy = L.LORA_COPY_RAW, pl.raw_copy.data_ptr()
                segs.append(r)
        self.touched = touched
        self.nseg = len(segs)
        arr = (L.LoraSeg * self.nseg)(*segs)
        self.table = ops.to_device(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone())
        ops.synchronize()

    def _hold(self, t):
        self._keep.append(t)
        return t

    def _vec(self, ops, v):
        got = self._f32.get(id(v))
        if got is None:
            got = self._f32[id(v)] = self._hold(ops.to_device(v.detach().cpu().float().contiguous()))
        return got

    def restore_fold(self, ops):
        """the load-time bytes of every fold vector the fuse writes (after a fuse with every scale zero)"""
        for pack, s, t in self._saved_fold.values():
            ops.copy_(pack.ln_s, s)
            ops.copy_(pack.ln_t, t)

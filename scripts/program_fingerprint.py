"""One hash per configuration over the program `Engine.prepare` records (both forms, flattened, in order): what a change to the engine's
host code must leave alone.  Run it before and after such a change and compare the listings line by line.
The hash covers, per call: the op's name; every tensor argument as (index of its storage by first appearance, storage offset, shape, strides,
dtype); every PackedConv by first appearance; every Geom by its fields; scalars and keyword names as they are.
Configurations: the MINI network at 64x64 with 2 steps -- ControlNet on / off x batch 1 / 2 x {default, device_seed, frame_prompts,
frame_options, all three}, ref_mode, use_side_stream, twin_encoders / group_merges / group_shortcuts off, a 1-step schedule, a slot.
Uses only Engine, prepare(use_graph=False, autotune=False), program, program_serial and Engine.flat_calls.  With a GPU the ops object is
HipOps; without one the op emulator of the tests, with stand-ins for the seeded scheduler ops it lacks (the recorded calls do not depend on
what an op computes).
    python scripts/program_fingerprint.py [--out listing.txt]"""
import dataclasses
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videosd_amd import config as C  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402
from videosd_amd.ops import Geom  # noqa: E402
from videosd_amd.packing import PackedConv  # noqa: E402

H = Wd = 64
STEPS = 2
MODES = {"default": {}, "device_seed": dict(device_seed=True), "frame_prompts": dict(frame_prompts=True),
         "frame_options": dict(frame_options=True), "all_three": dict(device_seed=True, frame_prompts=True, frame_options=True)}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def make_ops():
    if torch.cuda.is_available():
        from videosd_amd.ops import HipOps

        return HipOps(0)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from frame_option_cases import FrameOptionFakeOps

    class Ops(FrameOptionFakeOps):
        def clone(self, lane=None):
            return Ops()

        def add_noise_seeded(self, *a, **k):
            pass

        def lcm_step_seeded(self, *a, **k):
            pass

        def add_noise_frames(self, x0, noise_f32, seeds_dev, *a, **k):
            if seeds_dev is None:
                super().add_noise_frames(x0, noise_f32, seeds_dev, *a, **k)

        def lcm_step_frames(self, eps, sample, noise_f32, seeds_dev, *a, **k):
            if seeds_dev is None:
                super().lcm_step_frames(eps, sample, noise_f32, seeds_dev, *a, **k)

    return Ops()


class Fingerprint:
    def __init__(self):
        self.h = hashlib.sha256()
        self.storages, self.convs = {}, {}

    def item(self, v):
        if isinstance(v, torch.Tensor):
            key = v.untyped_storage().data_ptr() if v.numel() else ("empty", id(v))
            return ("T", self.storages.setdefault(key, len(self.storages)), v.storage_offset(), tuple(v.shape), tuple(v.stride()), str(v.dtype))
        if isinstance(v, PackedConv):
            return ("W", self.convs.setdefault(id(v), len(self.convs)))
        if isinstance(v, Geom):
            return ("G",) + dataclasses.astuple(v)
        if isinstance(v, (list, tuple)):
            return ("L",) + tuple(self.item(x) for x in v)
        if isinstance(v, dict):
            return ("D",) + tuple((k, self.item(x)) for k, x in v.items())
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (np.integer, np.floating)):
            return v.item()
        raise TypeError(f"program_fingerprint: an argument of type {type(v).__name__}")

    def calls(self, calls):
        for fn, a, k in Engine.flat_calls(calls):
            self.h.update(repr((fn.__name__, self.item(a), self.item(k))).encode())


def fingerprint(eng):
    f = Fingerprint()
    f.calls(eng.program.calls)
    f.h.update(b"|serial|")
    f.calls(eng.program_serial.calls)
    return f.h.hexdigest()[:24], len(eng.program.calls), len(eng.program_serial.calls)


def configurations():
    """(name, engine attributes set before prepare, prepare's keywords, as a slot)"""
    out = []
    for cn in (True, False):
        for batch in (1, 2):
            for mode, kw in MODES.items():
                out.append((f"cn={int(cn)} batch={batch} {mode}", {}, dict(use_controlnet=cn, batch=batch, **kw), False))
    out.append(("ref_mode", {}, dict(use_controlnet=False, ref_mode=True), False))
    for knob, val in (("use_side_stream", True), ("twin_encoders", False), ("group_merges", False), ("group_shortcuts", False)):
        out.append((f"{knob}={val}", {knob: val}, dict(use_controlnet=True), False))
    out.append(("one step", {}, dict(use_controlnet=True, steps=1), False))
    out.append(("slot of cn=1 batch=1 default", {}, dict(use_controlnet=True), True))
    return out


def build(name, attrs, kw, as_slot, weights, texts, **prep_kw):
    """the prepared engine of one configuration (prep_kw: further keywords of `prepare`)"""
    eng = Engine(make_ops(), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, *weights)
    for k, v in attrs.items():
        setattr(eng, k, v)
    eng.set_text_embeds(texts[0])
    kw = dict(kw, **prep_kw)
    steps = kw.pop("steps", STEPS)
    if kw.get("frame_prompts"):
        blocks = [eng.build_prompt(t) for t in texts]
        eng.use_prompts([blocks[b % 2] for b in range(kw.get("batch", 1))])
    eng.prepare(H, Wd, steps, 0.6, controlnet_scale=1.5, **kw)
    if as_slot:
        eng = eng.make_slot()
        eng.prepare(H, Wd, steps, 0.6, controlnet_scale=1.5, **kw)
    return eng


def inputs():
    weights = (W.synthesize(W.unet_spec(C.MINI_UNET), "unet."), W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn."),
               W.synthesize(W.taesd_spec(C.TAESD), "vae."))
    texts = [(torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(s)) * 0.5).half() for s in (7, 8)]
    return weights, texts


def main():
    out_path = arg("--out", None)
    weights, texts = inputs()
    lines = []
    for cfg in configurations():
        digest, n0, n1 = fingerprint(build(*cfg, weights, texts, use_graph=False, autotune=False))
        lines.append(f"{cfg[0]:34s} {digest}  calls {n0} / {n1}")
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

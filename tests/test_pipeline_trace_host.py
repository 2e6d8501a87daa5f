"""VideoSDPipeline's host side, pinned call by call without a GPU: the class is built over a stand-in `model` whose `make_slot` returns
recording engines, a fixed script of `submit_batch` / `collect_batch` / `needs_idle` / `warm_up` calls is driven through its public
surface, and what the engines were asked -- every call, its arguments, its order -- is compared with what the rules below give:

  * a launch builds the prompt blocks the cache lacks, then takes the engine of its (program, frames per launch, lane); a missing engine
    is made (`make_slot` of the model for a new program, of the program's root otherwise), given the prompt(s), the SDXL conditioning,
    and prepared with the mode switches of the pipeline; a program is (size rounded down to 8, steps, timestep count, ControlNet,
    reference-only[, the prompt for SDXL]);
  * the launch then installs its prompt(s) and, with `frame_options`, its option pairs, uploads the reference image an engine has not
    seen, and submits by ONE of three paths: I420 planes as they are (every frame I420, size a multiple of 8, no honoured `ref`), raw RGB
    (`device_resize`, every frame RGB, size a multiple of 8), or frames cropped / resized here;
  * `strength` / `controlnet_scale` of an idle program change by `update_options`; of a running one they are refused and `needs_idle`
    says so beforehand; programs and prompts leave least recently used first, never one a launch in flight reads.

Nothing here reads a private attribute other than those the class documents as its surface (`_plans`, `_engines`, `_prompts`,
`evictions`), so the same file pins any rewrite of the class."""
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from videosd_amd import config as C  # noqa: E402
from videosd_amd.frames import I420Frame  # noqa: E402
from videosd_amd.pipeline import VideoSDPipeline, center_crop_resize  # noqa: E402


# ------------------------------------------------------------------------------------------ the stand-ins
def _desc(x):
    """what a submit was handed, as something comparable: shapes / sizes and a checksum of the bytes"""
    if isinstance(x, (list, tuple)):
        return tuple(_desc(v) for v in x)
    if isinstance(x, I420Frame):
        return ("i420", x.size, zlib.crc32(np.ascontiguousarray(x.data).tobytes()))
    return (tuple(x.shape), zlib.crc32(np.ascontiguousarray(x).tobytes()))


class _Ops:
    def __init__(self, log):
        self.log = log

    def upload(self, dst, src):
        self.log.append(("upload", dst, tuple(src.shape)))

    def center_crop_box(self, sw, sh, tw, th):
        return (0, 0, sw, sh)

    def resample_rgb(self, *a): ...
    def i420_to_rgb(self, *a): ...
    def rgb_to_i420(self, *a): ...


class _Engine:
    """records every call; `collect_*` hand back frames of the prepared size"""

    def __init__(self, world, name):
        self.world, self.name, self.log, self.ops = world, name, world.log, world.ops
        self._prompt_slots = self._want_opts = self._ref_epoch = None
        self._blks = ()
        self.last_gpu_ms, self.last_upload_bytes, self.last_download_bytes = 1.5, 0, 0
        self.ref_u8 = name + ".ref"
        self.tune_for_lanes = None

    def make_slot(self, share_plan=True, lane=None):
        e = _Engine(self.world, f"e{len(self.world.engines) + 1}")
        self.world.engines.append(e)
        self.world.live += 1
        self.log.append(("make_slot", self.name, e.name, share_plan, lane))
        return e

    def build_prompt(self, embeds):
        self.world.blocks += 1
        blk = SimpleNamespace(name=f"b{self.world.blocks}", text=embeds.reshape(-1, embeds.shape[-1]).half())
        self.log.append(("build_prompt", blk.name, tuple(embeds.shape)))
        return blk

    def prepare(self, height, width, steps, strength, controlnet_scale=1.0, use_controlnet=True, batch=1, ref_mode=False, autotune=True,
                device_seed=False, frame_prompts=False, frame_options=False):
        self.size, self.batch = (height, width), batch
        self._prompt_slots = SimpleNamespace(src=list(self._blks)) if frame_prompts else None
        self.log.append(("prepare", self.name, height, width, steps, strength, controlnet_scale, use_controlnet, batch, ref_mode, autotune,
                         device_seed, frame_prompts, frame_options, self.tune_for_lanes))

    def update_options(self, strength, cn_scale):
        self.log.append(("update_options", self.name, strength, cn_scale))
        return True

    def use_prompt(self, blk):
        self.log.append(("use_prompt", self.name, blk.name))

    def use_prompts(self, blks):
        self._blks = list(blks)
        if self._prompt_slots is not None:
            self._prompt_slots.src = list(blks)
        self.log.append(("use_prompts", self.name, [b.name for b in blks]))

    def use_options(self, pairs):
        self._want_opts = [(("entry", s), c) for s, c in pairs]
        self.log.append(("use_options", self.name, list(pairs)))

    def set_added_cond(self, pooled, sizes):
        self.log.append(("set_added_cond", self.name, tuple(pooled.shape), tuple(sizes)))

    def _submit(self, what, frame, overlap, seeds):
        self.log.append((what, self.name, _desc(frame), overlap, seeds))

    def submit_u8(self, frame, overlap=None, seeds=None):
        self._submit("submit_u8", frame, overlap, seeds)

    def submit_raw_u8(self, frame, overlap=None, seeds=None):
        self._submit("submit_raw_u8", frame, overlap, seeds)

    def submit_raw_i420(self, frame, overlap=None, seeds=None):
        self.last_upload_bytes = 1024
        self._submit("submit_raw_i420", frame, overlap, seeds)

    def collect_u8(self):
        self.log.append(("collect_u8", self.name))
        h, w = self.size
        return np.full((h, w, 3) if self.batch == 1 else (self.batch, h, w, 3), 7, np.uint8)

    def collect_i420(self):
        self.log.append(("collect_i420", self.name))
        self.last_download_bytes = 2048
        h, w = self.size
        out = [I420Frame.from_rgb(np.full((h, w, 3), 7, np.uint8)) for _ in range(self.batch)]
        return out[0] if self.batch == 1 else out

    def _destroy_graphs(self):
        self.world.live -= 1
        self.log.append(("destroy_graphs", self.name))


def _pipeline(**kwargs):
    """-> (pipeline, log): a VideoSDPipeline whose `load_model` installs the recording model instead of opening a GPU"""
    world = SimpleNamespace(log=[], engines=[], blocks=0, live=0, limit=10 ** 9)
    world.ops = _Ops(world.log)

    class Traced(VideoSDPipeline):
        def load_model(self, model_name, controlnet_model=None):
            self.is_xl = "xl" in str(model_name).lower()
            self.unet_cfg = C.SDXL_UNET if self.is_xl else C.SD15_UNET
            self.text_encoder, self.weight_sources, self.tuning_mode = None, {}, "table"
            self.model = _Engine(world, "m")
            return self.model

        def _memory_used_and_limit(self, before=None):
            return world.live, world.limit

    kwargs.setdefault("model", "stand-in")
    p = Traced(controlnet="stand-in", **kwargs)
    p.world = world
    return p, world.log


@pytest.fixture(autouse=True)
def _no_overlap_override(monkeypatch):
    monkeypatch.delenv("VSD_OVERLAP_CN", raising=False)


# ------------------------------------------------------------------------------------------ inputs
def _rgb(seed, hw=(30, 40)):
    return np.random.default_rng(seed).integers(0, 256, hw + (3,), dtype=np.uint8)


def _inputs(kind, n):
    pil = [Image.fromarray(_rgb(k), "RGB") for k in range(n)]
    if kind == "pil":
        return pil
    if kind == "rgba":
        return [im.convert("RGBA") for im in pil]
    yuv = [I420Frame.from_rgb(_rgb(10 + k)) for k in range(n)]
    return yuv if kind == "i420" else [yuv[0]] + pil[1:]  # "mixed": an I420 frame and a PIL image in one launch


def _host_frames(imgs, w, h):
    """the frames the host path submits: videopipeline.py's crop / resize, then the rounding of a size that is no multiple of 8"""
    imgs = [center_crop_resize(im, w, h) for im in imgs]
    if h % 8 or w % 8:
        imgs = [im.resize((w - w % 8, h - h % 8), resample=Image.Resampling.LANCZOS) for im in imgs]
    return np.stack([np.asarray(im.convert("RGB"), dtype=np.uint8) for im in imgs])


def _one(xs):
    return xs[0] if len(xs) == 1 else xs


# ------------------------------------------------------------------------------------------ the rules, kept beside the pipeline
class Shadow:
    """What the rules of the module docstring make of a launch (no eviction: the cross below stays inside every cache)."""

    def __init__(self, xl=False, honor_ref_flag=False, honor_controlnet_flag=False, device_resize=False, device_seed=False,
                 frame_prompts=False, frame_options=False, lanes=2):
        self.xl, self.honor_ref_flag, self.honor_controlnet_flag, self.device_resize = xl, honor_ref_flag, honor_controlnet_flag, device_resize
        self.device_seed, self.frame_prompts, self.frame_options, self.lanes = device_seed, frame_prompts, frame_options, lanes
        self.blocks, self.plans, self.engines, self.ref_seen = {}, {}, 0, set()

    def launch(self, imgs, lane, o):
        """-> (the engine calls of submit_batch + collect_batch, which results are I420Frames, the size of every result)"""
        n, out = len(imgs), []
        h, w, steps = o["height"], o["width"], o["steps"]
        prompts = list(o.get("prompts") or [o.get("prompt", ["pixar, cg"])] * n) if self.frame_prompts else [o.get("prompt", ["pixar, cg"])]
        keys = [p if isinstance(p, str) else tuple(p) for p in prompts]
        for k in keys:
            if k not in self.blocks:
                self.blocks[k] = f"b{len(self.blocks) + 1}"
                out.append(("build_prompt", self.blocks[k], (77, (C.SDXL_UNET if self.xl else C.SD15_UNET).cross_dim)))
        names = [self.blocks[k] for k in keys]
        use_ref = bool(o.get("ref")) and self.honor_ref_flag and not self.xl
        use_cn = False if self.xl or use_ref else (bool(o.get("controlnet")) if self.honor_controlnet_flag else True)
        frame_opts = self.frame_options and not self.xl and not use_ref
        per = lambda v: [float(v)] * n if isinstance(v, (int, float)) else [float(x) for x in v]  # noqa: E731
        strengths, scales = per(o.get("strength", 0.4)), per(o.get("controlnet_scale", 1))
        h8, w8 = h - h % 8, w - w % 8
        n_eff = 1 if strengths[0] < 0.05 else steps  # (the strengths of this file at steps = 2: 0.02 gives one timestep, the others two)
        plan = self.plans.setdefault((h8, w8, steps, n_eff, use_cn, use_ref) + ((keys[0],) if self.xl else ()), {})
        eng = plan.get((n, lane))
        install = ("use_prompts", None, names) if self.frame_prompts else ("use_prompt", None, names[0])
        if eng is None:
            self.engines += 1
            eng = plan[(n, lane)] = f"e{self.engines}"
            out.append(("make_slot", plan.get("root", "m"), eng, "root" in plan, lane))
            plan.setdefault("root", eng)
            out.append((install[0], eng, install[2]))
            if self.xl:
                out.append(("set_added_cond", eng, (C.SDXL_UNET.add_pooled_dim,), (h8, w8, 0, 0, h8, w8)))
            out.append(("prepare", eng, h8, w8, steps, strengths[0], scales[0], use_cn, n, use_ref, False, self.device_seed, self.frame_prompts,
                        frame_opts, self.lanes >= 3 and n > 1))
        out.append((install[0], eng, install[2]))
        if frame_opts:
            out.append(("use_options", eng, list(zip(strengths, scales))))
        if use_ref and eng not in self.ref_seen:
            self.ref_seen.add(eng)
            out.append(("upload", eng + ".ref", (h8, w8, 3)))
        seed = o.get("seed", 42)
        seeds = ([seed] * n if isinstance(seed, int) else list(seed)) if self.device_seed else None
        yuv = [isinstance(im, I420Frame) for im in imgs]
        mult8 = h % 8 == 0 and w % 8 == 0
        on_device = all(yuv) and mult8 and not use_ref
        if on_device:
            out += [("submit_raw_i420", eng, _desc(_one(imgs)), True, seeds), ("collect_i420", eng)]
        else:
            imgs = [Image.fromarray(im.to_rgb(), mode="RGB") if k else im for im, k in zip(imgs, yuv)]
            if self.device_resize and mult8 and all(im.mode == "RGB" for im in imgs):
                out.append(("submit_raw_u8", eng, _desc(_one([np.asarray(im) for im in imgs])), True, seeds))
            else:
                out.append(("submit_u8", eng, _desc(_one(list(_host_frames(imgs, w, h)))) if n == 1 else _desc(_host_frames(imgs, w, h)), True, seeds))
            out.append(("collect_u8", eng))
        return out, [True] * n if on_device else yuv, (w8, h8)


SIZES = [dict(height=16, width=16), dict(height=100, width=150)]  # (the second becomes 96 x 144)
MODES = {  # name -> (constructor kwargs, [options of a launch of n frames, ...])
    "default": ({}, [lambda n: {}]),
    "device_seed": (dict(device_seed=True), [lambda n: dict(seed=[5, 6][:n])]),
    "frame_prompts": (dict(frame_prompts=True), [lambda n: dict(prompts=["a", ["b"]][:n])]),
    "frame_options": (dict(frame_options=True), [lambda n: dict(strength=[0.6, 0.9][:n], controlnet_scale=[1.0, 0.5][:n])]),
    "all_three": (dict(device_seed=True, frame_prompts=True, frame_options=True),
                  [lambda n: dict(seed=[5, 6][:n], prompts=["a", "b"][:n], strength=[0.6, 0.9][:n], controlnet_scale=[1.0, 0.5][:n]),
                   lambda n: dict(seed=9)]),  # (... and the same switches with one value for every frame)
    "sdxl": (dict(model="stabilityai/sdxl-lcm", frame_options=True), [lambda n: {}, lambda n: dict(prompt="other")]),
    "honor_ref": (dict(honor_ref_flag=True), [lambda n: dict(ref=True)]),
    "honor_controlnet": (dict(honor_controlnet_flag=True), [lambda n: dict(controlnet=True), lambda n: dict(controlnet=False)]),
}


@pytest.mark.parametrize("device_resize", [False, True], ids=["host_resize", "device_resize"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_mode_size_batch_lane_and_input_asks_the_engines_for_exactly_this(mode, device_resize):
    """every mode x both sizes x one and two frames x both lanes x PIL / RGBA / I420 / mixed input, with `device_resize` on and off: the
    engine calls of each launch are exactly those of `Shadow.launch`, the results come back in the kind and size they should"""
    ctor, variants = MODES[mode]
    p, log = _pipeline(device_resize=device_resize, max_plans=16, **ctor)
    sw = {k: v for k, v in ctor.items() if k != "model"}
    shadow = Shadow(xl="model" in ctor, device_resize=device_resize, **sw)
    # what dispatch.py reads (with `getattr(pipe, name, False)`) follows the switches; an SDXL object has no per-frame options
    assert bool(getattr(p, "per_frame_options", False)) == p.frame_options == (mode in ("frame_options", "all_three"))
    assert bool(getattr(p, "per_frame_seed", False)) == p.device_seed and bool(getattr(p, "per_frame_prompt", False)) == p.frame_prompts
    for variant in variants:
        for size in SIZES:
            for n in (1, 2):
                for lane in (0, 1):
                    for kind in ("pil", "rgba", "i420") + (("mixed",) if n == 2 else ()):
                        opts = dict(dict(size, steps=2, strength=0.6), **variant(n))
                        imgs, at = _inputs(kind, n), len(log)
                        if mode == "honor_ref" and n == 2:  # (reference-only: one frame per launch)
                            with pytest.raises(ValueError, match="one frame per call"):
                                p.submit_batch(imgs, lane=lane, **opts)
                            assert log[at:] == []
                            continue
                        want, yuv, wh = shadow.launch(imgs, lane, opts)
                        assert p.needs_idle(**{k: v for k, v in opts.items() if k in ("height", "width", "steps", "ref", "controlnet", "prompt")}) is False
                        handle = p.submit_batch(imgs, lane=lane, **opts)
                        assert handle[0].name == want[-1][1]
                        res = p.collect_batch(handle)
                        assert log[at:] == want, (mode, size, n, lane, kind)
                        assert [isinstance(r, I420Frame) for r in res] == yuv and all(r.size == wh for r in res)
                        assert all(isinstance(r, (I420Frame, Image.Image)) for r in res)
    assert len(p._plans) == len(shadow.plans) and len(p._engines) == shadow.engines and p.evictions == 0
    assert sorted(map(str, p._prompts)) == sorted(map(str, shadow.blocks))
    assert sorted(pk[:2] for pk in p._plans) == sorted(pk[:2] for pk in shadow.plans)


# ------------------------------------------------------------------------------------------ options of a plan, lanes, refusals
A = dict(height=16, width=16, steps=2)
BLACK1 = _desc(np.zeros((16, 16, 3), np.uint8))
BLACK2 = _desc(np.zeros((2, 16, 16, 3), np.uint8))


def _prep(eng, n, strength=0.6, scale=1.0, hw=(16, 16), lanes=2, **mode):
    m = dict(dict(device_seed=False, frame_prompts=False, frame_options=False), **mode)
    return ("prepare", eng, hw[0], hw[1], 2, strength, scale, True, n, False, False, m["device_seed"], m["frame_prompts"], m["frame_options"],
            lanes >= 3 and n > 1)


def _black(n=1, hw=(16, 16)):
    return [Image.new("RGB", (hw[1], hw[0]))] * n


def test_a_strength_change_on_an_idle_and_on_a_busy_plan():
    p, log = _pipeline()
    p.collect_batch(p.submit_batch(_black(), strength=0.6, **A))
    assert log == [("build_prompt", "b1", (77, 768)), ("make_slot", "m", "e1", False, 0), ("use_prompt", "e1", "b1"), _prep("e1", 1),
                   ("use_prompt", "e1", "b1"), ("submit_u8", "e1", BLACK1, True, None), ("collect_u8", "e1")]
    # idle: nobody has to wait, the program's constants are rewritten ahead of the launch
    del log[:]
    assert p.needs_idle(strength=0.9, **A) is False
    p.collect_batch(p.submit_batch(_black(), strength=0.9, controlnet_scale=2, **A))
    assert log == [("update_options", "e1", 0.9, 2.0), ("use_prompt", "e1", "b1"), ("submit_u8", "e1", BLACK1, True, None), ("collect_u8", "e1")]
    # busy: the change has to wait; everything else goes beside the launch
    del log[:]
    h0 = p.submit_batch(_black(), strength=0.9, controlnet_scale=2, **A)
    assert p.needs_idle(strength=0.6, controlnet_scale=2, **A) is True and p.needs_idle(strength=0.9, **A) is True  # (the scale differs)
    assert p.needs_idle(strength=0.9, controlnet_scale=2, **A) is False
    assert p.needs_idle(strength=0.9, controlnet_scale=2, **dict(A, height=24)) is False       # another program
    assert p.needs_idle(strength=0.02, **A) is False                                           # another timestep count: another program
    assert p.needs_idle(strength=0.9, controlnet_scale=2, prompt="other", **A) is False        # another prompt
    assert p.needs_idle(strength=0.9, **dict(A, steps="many")) is True                         # options nobody can read: wait
    with pytest.raises(RuntimeError, match="cannot change strength / controlnet_scale of a plan with launches in flight"):
        p.submit_batch(_black(), lane=1, strength=0.6, controlnet_scale=2, **A)
    with pytest.raises(RuntimeError, match="previous launch has not been collected"):
        p.submit_batch(_black(), lane=0, strength=0.9, controlnet_scale=2, **A)
    with pytest.raises(RuntimeError, match="cannot change the reference image while 1 launch"):
        p.set_reference(_black()[0])
    with pytest.raises(ValueError, match="lane 2: this pipeline was built for 2 launch lane"):
        p.submit_batch(_black(), lane=2, **A)
    h1 = p.submit_batch(_black(2), lane=1, strength=0.9, controlnet_scale=2, **A)
    assert [len(p.collect_batch(h)) for h in (h0, h1)] == [1, 2]
    assert log == [("use_prompt", "e1", "b1"), ("submit_u8", "e1", BLACK1, True, None),
                   ("make_slot", "e1", "e2", True, 1), ("use_prompt", "e2", "b1"), _prep("e2", 2, 0.9, 2.0),
                   ("use_prompt", "e2", "b1"), ("submit_u8", "e2", BLACK2, True, None), ("collect_u8", "e1"), ("collect_u8", "e2")]
    assert p.needs_idle(strength=0.9, **dict(A, steps="many")) is False and len(p._plans) == 1 and sorted(k[1:] for k in p._engines) == [(1, 0), (2, 1)]


def test_needs_idle_with_per_frame_options_and_with_reference_only():
    p, log = _pipeline(frame_options=True)
    h0 = p.submit_batch(_black(), strength=0.6, **A)
    assert p.needs_idle(strength=0.9, **A) is False and p.needs_idle(strength=0.9, **dict(A, steps="many")) is True
    h1 = p.submit_batch(_black(), lane=1, strength=0.9, controlnet_scale=0.5, **A)  # (no drain, no refusal: the pair is this lane's own)
    p.collect_batch(h0), p.collect_batch(h1)
    assert [c for c in log if c[0] in ("use_options", "update_options")] == [("use_options", "e1", [(0.6, 1.0)]), ("use_options", "e2", [(0.9, 0.5)])]
    q, _ = _pipeline(honor_ref_flag=True)
    assert q.needs_idle(ref=True, **A) is False and q.can_batch(ref=True) is False and q.can_batch(ref=False) is True and p.can_batch(ref=True) is True
    h = q.submit_batch(_black(), **A)
    assert q.needs_idle(ref=True, **A) is True and q.needs_idle(**A) is False
    q.collect_batch(h)


def test_warm_up_prepares_every_batch_size_on_every_lane():
    p, log = _pipeline(device_seed=True)
    assert p.warm_up(batches=(1, 2), lanes=2, strength=0.6, **A) == 4
    def new(eng, root, lane, n):  # noqa: E306
        return [("make_slot", root or "m", eng, root is not None, lane), ("use_prompt", eng, "b1"), _prep(eng, n, device_seed=True),
                ("use_prompt", eng, "b1"), ("submit_u8", eng, BLACK1 if n == 1 else BLACK2, True, [42] * n)]
    assert log == ([("build_prompt", "b1", (77, 768))] + new("e1", None, 0, 1) + new("e2", "e1", 1, 1) + [("collect_u8", "e1"), ("collect_u8", "e2")]
                   + new("e3", "e1", 0, 2) + new("e4", "e1", 1, 2) + [("collect_u8", "e3"), ("collect_u8", "e4")])
    assert len(p._plans) == 1 and sorted(k[1:] for k in p._engines) == [(1, 0), (1, 1), (2, 0), (2, 1)]
    # the defaults of `infer`: 640 x 360, twenty steps at strength 0.4
    del log[:]
    assert p.warm_up() == 1 and [c[:6] for c in log if c[0] == "prepare"] == [("prepare", "e5", 360, 640, 20, 0.4)]
    assert p.option_class({}) == 20 and p.option_class(dict(strength=0.02, steps=2)) == 1
    # with four lanes a third launch has no command-processor pipe for its side branch, and coalesced launches are tuned for the loaded case
    q, qlog = _pipeline(lanes=4)
    hs = [q.submit_batch(_black(2), lane=l, strength=0.6, **A) for l in (0, 1, 3)]
    assert [c[3] for c in qlog if c[0] == "submit_u8"] == [True, True, False]
    assert [c for c in qlog if c[0] == "prepare"] == [_prep(e, 2, lanes=4) for e in ("e1", "e2", "e3")]
    q.collect_batch(hs[1])
    assert [c[1] for c in qlog if c[0] == "collect_u8"] == ["e2"]
    hs[1] = q.submit_batch(_black(2), lane=1, strength=0.6, **A)
    assert [c[3] for c in qlog if c[0] == "submit_u8"][-1] is False  # (lane 3 is still busy: lane 1's side stream is lane 3's own)
    for h in hs:
        q.collect_batch(h)
    del qlog[:]
    hs = [q.submit_batch(_black(n), lane=l, strength=0.6, **A) for n, l in ((2, 0), (2, 1), (1, 0))]  # a third launch beside two, all on lanes 0 / 1
    assert [c[3] for c in qlog if c[0] == "submit_u8"] == [True, True, False]
    for h in hs:
        q.collect_batch(h)


@pytest.mark.parametrize("ctor, extra", [(dict(device_seed=True), {}), (dict(frame_prompts=True), {}), (dict(device_seed=True, frame_prompts=True), {}),
                                         (dict(model="sdxl", frame_options=True), dict(prompt="a cat")), (dict(honor_controlnet_flag=True), dict(controlnet=True)),
                                         (dict(device_resize=True), dict(height=20, width=22))],
                         ids=["device_seed", "frame_prompts", "both", "sdxl", "honor_controlnet", "rounded_size"])
def test_needs_idle_finds_the_running_plan_in_every_mode(ctor, extra):
    """`needs_idle` and `submit_batch` must name a program alike: a slider change on the plan that is running waits -- in every mode"""
    p, log = _pipeline(**ctor)
    o = dict(A, strength=0.6, **extra)
    assert p.needs_idle(**o) is False
    h = p.submit_batch(_black(), **o)
    assert p.needs_idle(**o) is False and p.needs_idle(**dict(o, strength=0.9)) is True and p.needs_idle(**dict(o, controlnet_scale=0.5)) is True
    assert p.needs_idle(**dict(o, steps=4)) is False and p.needs_idle(**dict(o, strength=0.02)) is False
    if "model" in ctor:  # (SDXL: the prompt is part of the program)
        assert p.needs_idle(**dict(o, strength=0.9, prompt="a dog")) is False
    if "honor_controlnet_flag" in ctor:
        assert p.needs_idle(**dict(o, strength=0.9, controlnet=False)) is False
    with pytest.raises(RuntimeError, match="launches in flight"):
        p.submit_batch(_black(), lane=1, **dict(o, strength=0.9))
    p.collect_batch(h)
    assert p.needs_idle(**dict(o, strength=0.9)) is False and len(p._plans) == 1 and [c[0] for c in log].count("prepare") == 1


def test_what_is_refused_and_which_refusal_comes_first():
    p, log = _pipeline()
    two = _black(2)
    for match, kw in [("needs a pipeline built with frame_prompts=True", dict(prompts=["a", "b"])),
                      ("lane 5", dict(lane=5, prompts=["a", "b"])),                              # the lane, before the prompts
                      ("frame_prompts=True", dict(prompts=["a", "b"], height=4)),                 # the prompts, before the size
                      ("height and width must be at least 8", dict(height=4, strength=[0.6, 0.9], steps=2)),   # the size, before the options
                      ("one-element list", dict(prompt=["a", "b"])),
                      ("strength must be a number or a sequence of one per frame: 3 value", dict(strength=[0.6, 0.9, 0.3], seed=[1])),
                      ("different values per frame need a pipeline built with frame_options=True", dict(strength=[0.6, 0.9], steps=2, seed=[1])),
                      ("different values per frame need a pipeline built with frame_options=True", dict(controlnet_scale=[1, 2])),
                      ("strength=0.0 gives an empty LCM schedule", dict(strength=0.0, steps=2))]:
        with pytest.raises(ValueError, match=match):
            p.submit_batch(two, **dict(A, **kw))
    assert log == [("build_prompt", "b1", (77, 768))] and len(p._plans) == 0 and p.needs_idle(steps="many") is False  # (nothing is in flight)
    q, qlog = _pipeline(device_seed=True, frame_prompts=True, frame_options=True, honor_ref_flag=True)
    for match, kw in [("one prompt per frame: 3 prompt", dict(prompts=["a", "b", "c"])),
                      ("reference-only frames run one frame per launch", dict(prompts=["a", "b"], ref=True)),
                      ("ref=True: one frame per call", dict(ref=True, strength=[0.6, 0.02])),      # before the options
                      ("different numbers of timesteps at steps=2", dict(strength=[0.6, 0.02], seed=[1])),  # before the seeds
                      ("seed must be an int or a sequence of 2 ints", dict(seed=[1])),
                      ("seed must be an int or a sequence of 2 ints", dict(seed=[1, 2.5]))]:
        with pytest.raises(ValueError, match=match):
            q.submit_batch(two, **dict(A, **kw))
    assert [c[0] for c in qlog] == ["build_prompt"] and len(q._plans) == 0
    x, _ = _pipeline(model="sdxl", frame_prompts=True)
    with pytest.raises(ValueError, match="an SDXL program has the pooled text embedding of ITS prompt baked in"):
        x.submit_batch(two, prompts=["a", "b"], **A)
    with pytest.raises(KeyError):
        VideoSDPipeline(model="no controlnet named")


# ------------------------------------------------------------------------------------------ the caches
def _size(s):
    return dict(height=s, width=s, steps=2, strength=0.6)


def test_a_fourth_program_evicts_the_least_recently_used_idle_one():
    p, log = _pipeline(max_plans=3)
    for s in (16, 24, 32):
        p.collect_batch(p.submit_batch(_black(1, (s, s)), **_size(s)))
    p.collect_batch(p.submit_batch(_black(2, (16, 16)), lane=1, **_size(16)))  # (a second engine of the oldest program; it is now the newest)
    assert [pk[0] for pk in p._plans] == [24, 32, 16] and len(p._engines) == 4
    del log[:]
    p.collect_batch(p.submit_batch(_black(1, (40, 40)), **_size(40)))
    assert log[:3] == [("destroy_graphs", "e2"), ("make_slot", "m", "e5", False, 0), ("use_prompt", "e5", "b1")]
    assert [pk[0] for pk in p._plans] == [32, 16, 40] and p.evictions == 0
    # never one with a launch in flight: the next oldest goes
    h = p.submit_batch(_black(1, (32, 32)), **_size(32))
    del log[:]
    p.collect_batch(p.submit_batch(_black(1, (48, 48)), lane=1, **_size(48)))
    assert [c for c in log if c[0] == "destroy_graphs"] == [("destroy_graphs", "e1"), ("destroy_graphs", "e4")]
    assert [pk[0] for pk in p._plans] == [40, 32, 48]
    # ... and when every program is busy the cache grows
    h2 = p.submit_batch(_black(1, (40, 40)), lane=1, **_size(40))
    h3 = p.submit_batch(_black(1, (48, 48)), lane=0, **_size(48))
    del log[:]
    with pytest.raises(RuntimeError, match="previous launch has not been collected"):
        p.submit_batch(_black(1, (32, 32)), **_size(32))
    p.collect_batch(h)
    h = p.submit_batch(_black(1, (56, 56)), **_size(56))
    assert [c for c in log if c[0] == "destroy_graphs"] == [("destroy_graphs", "e3")] and [pk[0] for pk in p._plans] == [40, 48, 56]
    for x in (h, h2, h3):
        p.collect_batch(x)
    assert p.evictions == 0 and len(p._prompts) == 1


def test_a_memory_budget_drops_idle_programs_then_idle_slots():
    p, log = _pipeline(max_plans=8)
    for s, n in ((16, 1), (16, 2), (24, 1), (32, 1), (32, 2)):
        p.collect_batch(p.submit_batch(_black(n, (s, s)), **_size(s)))
    assert p.world.live == 5 and p.evictions == 0
    p.world.limit = 3
    del log[:]
    p.collect_batch(p.submit_batch(_black(3, (32, 32)), **_size(32)))  # five engines held, three allowed: the oldest program's two go
    assert log[:3] == [("destroy_graphs", "e1"), ("destroy_graphs", "e2"), ("make_slot", "e4", "e6", True, 0)]
    assert p.evictions == 2 and [pk[0] for pk in p._plans] == [24, 32]
    p.world.limit = 1
    h = p.submit_batch(_black(2, (32, 32)), **_size(32))  # in flight: e5 stays
    del log[:]
    p.collect_batch(p.submit_batch(_black(4, (32, 32)), lane=1, **_size(32)))  # the other program, then the idle slots of this one; never the root
    assert log[:3] == [("destroy_graphs", "e3"), ("destroy_graphs", "e6"), ("make_slot", "e4", "e7", True, 1)]
    p.collect_batch(h)
    assert p.evictions == 4 and [pk[0] for pk in p._plans] == [32] and sorted(k[1:] for k in p._engines) == [(1, 0), (2, 0), (4, 1)]


def test_nine_prompts_in_a_cache_of_eight():
    p, log = _pipeline(max_prompts=8)
    for k in range(9):
        p.collect_batch(p.submit_batch(_black(), prompt=f"p{k}", **_size(16)))
    assert list(p._prompts) == [f"p{k}" for k in range(1, 9)]
    assert [c[1] for c in log if c[0] == "build_prompt"] == [f"b{k}" for k in range(1, 10)]
    p.collect_batch(p.submit_batch(_black(), prompt=["p1"], **_size(16)))  # a one-element list is another key for the same text
    p.collect_batch(p.submit_batch(_black(), prompt="p3", **_size(16)))
    assert list(p._prompts) == ["p2", "p4", "p5", "p6", "p7", "p8", ("p1",), "p3"]
    assert [c[2] for c in log if c[0] == "use_prompt"][-2:] == ["b10", "b4"] and len(p._plans) == 1
    assert p.set_prompt_embeds(p.encode_prompt("p3"), key="p3").name == "b4"           # the same embeddings again: the block stays
    assert p.set_prompt_embeds(p.encode_prompt("p3") + 1, key="p3").name == "b11"      # others: rebuilt in place
    assert list(p._prompts)[-1] == "p3" and len(p._prompts) == 8

    q, qlog = _pipeline(max_prompts=8, frame_prompts=True)
    for k in range(0, 8, 2):
        q.collect_batch(q.submit_batch(_black(2), prompts=[f"p{k}", f"p{k + 1}"], **_size(16)))
    assert list(q._prompts) == [f"p{k}" for k in range(8)]
    h = q.submit_batch(_black(2), prompts=["p0", "p1"], **_size(16))  # in flight: its two entries stay, whatever their age
    q.collect_batch(q.submit_batch(_black(2), lane=1, prompts=["p8", "p9"], **_size(16)))
    assert list(q._prompts) == ["p4", "p5", "p6", "p7", "p0", "p1", "p8", "p9"]
    # one launch that names the oldest entry and a new one: the entry of the launch being put together stays too
    q.collect_batch(q.submit_batch(_black(2), lane=1, prompts=["p10", "p4"], **_size(16)))
    assert list(q._prompts) == ["p6", "p7", "p0", "p1", "p8", "p9", "p10", "p4"] and "p5" not in q._prompts
    q.collect_batch(h)
    assert [c[2] for c in qlog if c[0] == "use_prompts"][-1] == ["b11", "b5"] and q.evictions == 0

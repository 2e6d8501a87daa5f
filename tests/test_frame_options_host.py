"""Per-frame options without a GPU: the recorded form of a `frame_options` program and its frames through the op emulator (a mixed launch
against uniform launches), which frame slots get installed when, the option layouts' bounds and alignment, the entry cache keyed by
timesteps, the worker's coalescing of requests that differ in `strength` / `controlnet_scale`, the class's checks that come before any
device work, and the agreement of header, binding and build list on the new entry points."""
import multiprocessing as mp
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_option_cases as FO  # noqa: E402
from frame_prompt_cases import apply_segments  # noqa: E402

import videosd_amd.engine as E  # noqa: E402
from videosd_amd import config as C  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402
from videosd_amd.lcm import LCMSchedule, lcm_timesteps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = Wd = 64
STEPS, B = 2, 3
OPTS = (FO.OPT_A, FO.OPT_B)
PREP = dict(use_controlnet=True, use_graph=False)
NEW_SYMBOLS = ["vsd_add_noise_frames", "vsd_lcm_step_frames", "vsd_groupnorm_addvec", "vsd_cn_merge_frames"]


def _frame(h, w, seed=1):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = ((xx * 5 + yy * 3) % 256).astype(np.uint8)[..., None]
    return (base // 2 + grad // 2).astype(np.uint8)


def _mad(a, b):
    return float(np.abs(a.astype(int) - b.astype(int)).mean())


def _names(eng):
    return [fn.__name__ for fn, _a, _k in Engine.flat_calls(eng.program.calls)]


@pytest.fixture(scope="module")
def world():
    """ONE engine on the op emulator and every launch the tests below compare, computed once"""
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    eng = Engine(FO.FrameOptionFakeOps(), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    frames = np.stack([_frame(H, Wd, s) for s in (1, 2, 3)])
    out = {"eng": eng, "frames": frames}
    # the default program, one launch per pair of options
    plan = eng.prepare(H, Wd, STEPS, OPTS[0][0], controlnet_scale=OPTS[0][1], batch=B, **PREP)
    out["default_plan"], out["default_names"] = dict(plan), _names(eng)
    out["default_calls"] = list(Engine.flat_calls(eng.program.calls))
    out["default"] = [eng.infer_u8(frames)]
    eng.update_options(*OPTS[1])
    out["default"].append(eng.infer_u8(frames))
    # the per-frame program
    ops = eng.ops
    plan = eng.prepare(H, Wd, STEPS, OPTS[0][0], controlnet_scale=OPTS[0][1], batch=B, frame_options=True, **PREP)
    out["plan"], out["names"] = dict(plan), _names(eng)
    out["calls"] = list(Engine.flat_calls(eng.program.calls))
    out["installs_prepare"] = list(ops.installs)
    runs = {}
    for name, idx in (("000", [0, 0, 0]), ("010", [0, 1, 0]), ("100", [1, 0, 0]), ("111", [1, 1, 1])):
        del ops.installs[:]
        eng.use_options([OPTS[i] for i in idx])
        runs[name] = (eng.infer_u8(frames), list(ops.installs))
    # controlnet_scale alone: the same entries, other scales -- no install
    del ops.installs[:]
    eng.use_options([(OPTS[1][0], 2.0)] * B)
    runs["scale"] = (eng.infer_u8(frames), list(ops.installs))
    out["runs"] = runs
    out["builds"] = (eng.family["option_builds"], len(eng.family["option_entries"]))
    return out


# ------------------------------------------------------------------------------------------ the recorded programs
def test_the_default_program_is_unchanged(world):
    names = world["default_names"]
    assert world["default_plan"]["frame_options"] is False
    assert not set(names) & {"add_noise_frames", "lcm_step_frames", "groupnorm_addvec", "cn_merge_frames"}
    assert names.count("add_noise_dev") == 1 and names.count("lcm_step_dev") == STEPS
    convs = [k for fn, _a, k in world["default_calls"] if fn.__name__ == "conv"]
    assert sum(1 for k in convs if k.get("rowvec") is not None) > 0 and sum(1 for k in convs if k.get("out_scale_dev") is not None) == (len(world["eng"].cn.zero_convs) + 1) * STEPS


def test_the_per_frame_program_reads_every_option_per_frame(world):
    eng, names, calls = world["eng"], world["names"], world["calls"]
    assert world["plan"]["frame_options"] is True and world["plan"]["n"] == STEPS
    assert not set(names) & {"add_noise_dev", "lcm_step_dev", "add_noise_seeded", "lcm_step_seeded"}
    assert names.count("add_noise_frames") == 1 and names.count("lcm_step_frames") == STEPS and names.count("cn_merge_frames") == STEPS
    # every conv1 lost its time vector, every zero-conv its scale and residual: no conv of the program has either
    convs = [k for fn, _a, k in calls if fn.__name__ == "conv"]
    assert not any(k.get("rowvec") is not None or k.get("out_scale_dev") is not None for k in convs)
    blocks_cn = sum(len(b) for b in eng.cn.down) + 2  # the encoder's ResnetBlocks: the levels' and the mid block's two
    blocks_unet = sum(len(b) for b in eng.unet.down) + 2 + sum(len(b) for b in eng.unet.up)
    assert names.count("groupnorm_addvec") == STEPS * (blocks_unet + blocks_cn)  # norm2 of every ResnetBlock
    # ... as many plain GroupNorms less than the default program has
    assert world["default_names"].count("groupnorm") - names.count("groupnorm") == names.count("groupnorm_addvec")
    lay = eng.fo_layout
    for fn, a, k in calls:
        if fn.__name__ == "groupnorm_addvec":  # frame 0's slice of a time table of the engine's own block; the next frame's lies one table further
            assert a[2] in (lay.n * lay.cols["unet"], lay.n * lay.cols["cn"]) and a[1].numel() == a[3] and k["batch"] == B
            assert a[1].untyped_storage().data_ptr() == eng.fo_buf.untyped_storage().data_ptr()
        elif fn.__name__ in ("add_noise_frames", "lcm_step_frames"):
            coef, stride = (a[5], a[6]) if fn.__name__ == "add_noise_frames" else (a[6], a[7])
            assert stride == lay.coef_stride and coef.untyped_storage().data_ptr() == eng.fo_buf.untyped_storage().data_ptr()
        elif fn.__name__ == "cn_merge_frames":
            nres = len(eng.cn.zero_convs) + 1
            assert a[1] == nres and a[2] is eng.fo_scale and a[3] == eng.fo_scale.shape[1] == 16 and a[4] == B
            assert sorted(r[5] for r in a[0].tolist()) == list(range(nres))  # one scale column per residual
    with pytest.raises(RuntimeError, match="use_options"):
        eng.update_options(0.5, 1.0)


# ------------------------------------------------------------------------------------------ results
def test_frames_of_a_mixed_launch_are_the_frames_of_uniform_launches(world):
    runs = world["runs"]
    uniform = {0: runs["000"][0], 1: runs["111"][0]}
    for name, idx in (("010", [0, 1, 0]), ("100", [1, 0, 0])):
        for i, oi in enumerate(idx):
            assert np.array_equal(runs[name][0][i], uniform[oi][i]), (name, i)  # (the emulator has no rounding that depends on the neighbours)
    for i in range(B):
        assert _mad(uniform[0][i], uniform[1][i]) > 1.0        # the options matter ...
        d = [_mad(uniform[k][i], world["default"][k][i]) for k in (0, 1)]
        print(f"frame {i}: per-frame program vs default program {d[0]:.3f} / {d[1]:.3f} LSB")
        assert max(d) < _mad(uniform[0][i], uniform[1][i]) / 4  # ... and each pair gives the default program's picture of THAT pair
    assert _mad(runs["scale"][0][0], uniform[1][0]) > 0.1     # controlnet_scale alone changes the picture too


def test_only_the_changed_slots_are_installed(world):
    runs = world["runs"]
    assert sorted(world["installs_prepare"]) == [0, 1, 2]  # a fresh block: every slot, once
    assert runs["000"][1] == []                            # the options `prepare` was given: nothing to do
    assert runs["010"][1] == [1]
    assert sorted(runs["100"][1]) == [0, 1]
    assert sorted(runs["111"][1]) == [1, 2]
    assert runs["scale"][1] == []                          # the same timesteps: the scales travel by their own copy
    assert world["builds"] == (2, 2)  # two timestep tuples in all those launches: two entries, each built once


def test_the_entry_cache_is_keyed_by_timesteps(world):
    eng = world["eng"]
    assert lcm_timesteps(0.6, STEPS) == lcm_timesteps(0.61, STEPS) != lcm_timesteps(0.62, STEPS)
    builds = eng.family["option_builds"]
    a, b = eng.option_entry(0.6, STEPS), eng.option_entry(0.61, STEPS)
    assert a is b and eng.family["option_builds"] == builds  # two strengths, one tuple, one entry (built by `prepare`)
    c = eng.option_entry(0.62, STEPS)
    assert c is not a and eng.family["option_builds"] == builds + 1 and c.timesteps == tuple(lcm_timesteps(0.62, STEPS))
    # the entry holds that schedule's coefficients in the default block's layout, and both time tables
    lay, s = c.layout, LCMSchedule(0.62, STEPS)
    coef = lay.view(c.buf, "coef")
    want = list(s.add_noise_coef()) + [float(v) for i in range(STEPS) for v in s.step_coef(i)]
    assert torch.equal(coef[:len(want)], torch.tensor(want, dtype=torch.float32)) and not coef[len(want):].any()
    ref = torch.zeros(STEPS, eng.unet.temb_proj.n, dtype=torch.float16)
    eng._time_embeddings(eng.unet, s, ref)
    assert torch.equal(lay.view(c.buf, "unet"), ref) and lay.view(c.buf, "cn").abs().sum() > 0
    # least recently used out, the newest kept
    keep = eng.family.get("max_option_entries")
    eng.family["max_option_entries"] = 2
    try:
        d = eng.option_entry(0.3, STEPS)
        assert list(eng.family["option_entries"].values())[-1] is d and len(eng.family["option_entries"]) == 2
    finally:
        eng.family.pop("max_option_entries") if keep is None else eng.family.__setitem__("max_option_entries", keep)
    # errors of use_options: the count, another number of timesteps, an engine of the default form
    with pytest.raises(ValueError, match="2 option pair"):
        eng.use_options([OPTS[0], OPTS[1]])
    with pytest.raises(ValueError, match="timestep"):
        eng.use_options([OPTS[0], (0.02, 1.0), OPTS[0]])
    eng.use_options([OPTS[0], OPTS[1], OPTS[0]])
    assert np.array_equal(eng.infer_u8(world["frames"]), world["runs"]["010"][0])  # ... and nothing was disturbed


# ------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("frames", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_option_layouts_bounds_alignment_and_copy_list(frames, n):
    cols = {"unet": 5048, "cn": 2488}
    src, dst = E.OptionLayout(n, cols, 1), E.OptionLayout(n, cols, frames)
    assert dst.coef_stride >= 2 + 6 * n and dst.coef_stride % 4 == 0
    spans = []
    for lay in (src, dst):
        for name, (off, nb) in lay.items.items():
            assert off % 16 == 0 and nb % 16 == 0 and off + lay.frames * nb <= lay.nbytes
            assert nb == (lay.coef_stride * 4 if name == "coef" else n * cols[name] * 2)
            if lay is dst:
                spans.append((off, off + lay.frames * nb))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # the items do not overlap
    segs = E.option_segments(src, dst)
    assert len(segs) == 3
    for so, do, rows, rb, pitch, fs in segs:
        assert all(v % 16 == 0 and v >= 0 for v in (so, do, rb, pitch, fs)) and rows == 1
        assert pitch == frames * fs and fs == rb  # what vsd_prompt_install asks of a table: the frame slots of a destination row
        assert so + rb <= src.nbytes and do + frames * fs <= dst.nbytes
    rng = np.random.default_rng(10 * frames + n)
    entry = rng.integers(0, 256, src.nbytes, dtype=np.uint8)
    for f in range(frames):
        blk = np.full(dst.nbytes, FO.SENTINEL, np.uint8)
        apply_segments(segs, entry, blk, f)
        want = np.full(dst.nbytes, FO.SENTINEL, np.uint8)
        for name in dst.items:
            (a0, a1), (s0, s1) = FO.slot_bytes(dst, name, f), FO.slot_bytes(src, name, 0)
            want[a0:a1] = entry[s0:s1]
        assert np.array_equal(blk, want), f  # slot f holds the entry, every other slot and the padding still the sentinel
        # ... and the views the engine records address exactly those bytes
        t = torch.from_numpy(blk)
        for name in dst.items:
            v = dst.view(t, name, f)
            a0, a1 = FO.slot_bytes(dst, name, f)
            assert v.data_ptr() - t.data_ptr() == a0 and v.numel() * v.element_size() == a1 - a0
    with pytest.raises(ValueError, match="another schedule length"):
        E.option_segments(E.OptionLayout(n + 1, cols, 1), dst)
    with pytest.raises(ValueError, match="multiple of 8"):
        E.OptionLayout(1, {"unet": 12}, 2)


# ------------------------------------------------------------------------------------------ dispatch
def _serve(factory, requests, max_batch=3):
    """the worker loop in a thread of this process, with the requests ALREADY queued when it starts -> (launches, replies)"""
    from videosd_amd.dispatch import _worker_main

    del FO.OptionPipeline.SUBMITS[:]
    del FO.PerFrameOptionPipeline.NEEDS_IDLE[:]
    parent, child = mp.Pipe()
    for k, opts in enumerate(requests):
        img = Image.fromarray(np.full((12, 16, 3), 10 * (k + 1), np.uint8), "RGB")
        parent.send((k, "infer", (img,), dict(height=12, width=16, **opts)))
    parent.send(None)
    t = threading.Thread(target=_worker_main, args=(child, factory, dict(model="m", controlnet="c", device=0)), kwargs=dict(max_batch=max_batch))
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert parent.recv() == ("ready", None)
    replies = {}
    while parent.poll(0):
        rid, ok, payload = parent.recv()
        assert ok, payload
        replies[rid] = np.asarray(payload)
    return list(FO.OptionPipeline.SUBMITS), replies


def test_worker_coalesces_requests_that_differ_in_strength_and_scale():
    reqs = [dict(strength=0.6, controlnet_scale=1.5, steps=2), dict(strength=0.9, controlnet_scale=0.4, steps=2), dict(strength=0.3, steps=2)]
    launches, replies = _serve("frame_option_cases:PerFrameOptionPipeline", reqs)
    assert launches == [(3, [0.6, 0.9, 0.3], [1.5, 0.4, 1], 2)], launches  # ONE launch, lists in request order (a missing scale: `infer`'s default)
    assert sorted(replies) == [0, 1, 2]
    for k in range(3):  # each reply is its request's frame (inverted by the stand-in), out of a launch of three
        assert int(replies[k][1, 1, 0]) == 255 - 10 * (k + 1) and int(replies[k][0, 0, 1]) == 3


def test_worker_keeps_another_option_class_and_other_options_apart():
    # strength 0.02 gives one timestep at steps = 2: another program; another step count is another option anyway
    reqs = [dict(strength=0.6, steps=2), dict(strength=0.02, steps=2), dict(strength=0.03, steps=2), dict(strength=0.6, steps=4), dict(strength=0.9, steps=4)]
    launches, replies = _serve("frame_option_cases:PerFrameOptionPipeline", reqs)
    assert launches == [(1, [0.6], [1], 2), (2, [0.02, 0.03], [1, 1], 2), (2, [0.6, 0.9], [1, 1], 4)], launches
    assert [int(replies[k][0, 0, 1]) for k in range(5)] == [1, 2, 2, 2, 2]
    # a request whose options differ from the launch in flight asks the pipeline whether it must wait -- and it need not
    assert FO.PerFrameOptionPipeline.NEEDS_IDLE == [0.02, 0.6]


def test_worker_without_the_attribute_behaves_as_before():
    reqs = [dict(strength=0.6, controlnet_scale=1.5), dict(strength=0.9, controlnet_scale=1.5), dict(strength=0.9, controlnet_scale=1.5),
            dict(strength=0.9, controlnet_scale=0.4)]
    launches, replies = _serve("frame_option_cases:OptionPipeline", reqs)
    assert launches == [(1, 0.6, 1.5, None), (2, 0.9, 1.5, None), (1, 0.9, 0.4, None)], launches  # numbers, never lists
    assert [int(replies[k][0, 0, 1]) for k in range(4)] == [1, 2, 2, 1]


# ------------------------------------------------------------------------------------------ the class, before any device work
def _bare_pipeline(**attrs):
    from helpers_fake_pipeline import bare_pipeline

    return bare_pipeline(_cache_prompt=lambda key, **kw: None, **attrs)  # (no engine behind it)


def test_the_class_checks_options_before_any_device_work(tmp_path):
    imgs = [Image.new("RGB", (16, 16))] * 2
    kw = dict(height=16, width=16, steps=2)
    p = _bare_pipeline(frame_options=True)
    assert p.option_class(dict(strength=0.6, steps=2)) == 2 and p.option_class(dict(strength=0.02, steps=2)) == 1 and p.option_class({}) == 20
    with pytest.raises(ValueError, match="one per frame"):
        p.submit_batch(imgs, strength=[0.6, 0.9, 0.3], **kw)
    with pytest.raises(ValueError, match="one per frame"):
        p.submit_batch(imgs, controlnet_scale=[1.0], **kw)
    with pytest.raises(ValueError, match="numbers of timesteps"):
        p.submit_batch(imgs, strength=[0.6, 0.02], **kw)
    with pytest.raises(ValueError, match="frame_options=True"):
        p.export_plan(str(tmp_path / "x.vsdplan"))
    assert p.needs_idle(strength=0.9, **kw) is False
    # without the switch: different values per frame are refused, by name
    with pytest.raises(ValueError, match="frame_options=True"):
        _bare_pipeline().submit_batch(imgs, strength=[0.6, 0.9], **kw)
    with pytest.raises(ValueError, match="frame_options=True"):
        _bare_pipeline().submit_batch(imgs, controlnet_scale=[1.0, 0.5], **kw)
    # ... and an SDXL / reference-only launch of a pipeline with it keeps one pair per launch
    with pytest.raises(ValueError, match="SDXL"):
        _bare_pipeline(frame_options=True, is_xl=True).submit_batch(imgs, strength=[0.6, 0.9], **kw)


def test_prepare_names_the_missing_op():
    class NoMergeOps(FO.FrameOptionFakeOps):
        cn_merge_frames = property()  # (hasattr is False)

    e = Engine.__new__(Engine)
    e.ops = NoMergeOps()
    with pytest.raises(ValueError, match="cn_merge_frames"):
        e.prepare(96, 160, 2, 0.5, frame_options=True)
    from fake_ops import FakeOps

    e.ops = FakeOps()
    with pytest.raises(ValueError, match="add_noise_frames.*lcm_step_frames.*groupnorm_addvec.*cn_merge_frames"):
        e.prepare(96, 160, 2, 0.5, frame_options=True)


# ------------------------------------------------------------------------------------------ header, binding, build list
def test_header_binding_and_build_list_agree_on_the_new_entry_points():
    import ctypes as Ct

    from videosd_amd import build as Bd
    from videosd_amd import plan as P

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    letter = {"void*": Ct.c_void_p, "int": Ct.c_int, "float": Ct.c_float}
    for name in NEW_SYMBOLS:
        m = re.search(r"^int " + name + r"\(vsd_ctx\* ctx, ([^;]*)\);", header, re.M)
        assert m, name
        args = []
        for a in re.sub(r"\s+", " ", m.group(1)).split(", "):
            typ = a.rsplit(" ", 1)[0].replace("const ", "")
            args.append(Ct.c_void_p if typ.endswith("*") else letter[typ])
        res, sig = L.SIGNATURES[name]
        assert res is Ct.c_int and sig == [Ct.c_void_p] + args, name
        assert name not in P.PLAN_FUNCS  # not plan-recordable
        src = [f for f in Bd.SOURCES if re.search(r'extern "C" int ' + name + r"\(", open(os.path.join(Bd.CSRC, f)).read())]
        assert len(src) == 1, (name, src)
    assert "frame_options.hip" in Bd.SOURCES and os.path.exists(os.path.join(Bd.CSRC, "frame_options.hip"))
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header
    assert "#define VSD_MERGE_SEG_MAX %d" % L.MERGE_SEG_MAX in header
    for op in ("add_noise_frames", "lcm_step_frames", "groupnorm_addvec", "cn_merge_frames"):
        from videosd_amd.ops import HipOps

        assert callable(getattr(HipOps, op)) and op in E.FRAME_OPTION_OPS

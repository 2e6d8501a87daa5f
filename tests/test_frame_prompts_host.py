"""Per-frame prompts without a GPU: the recorded form of a `frame_prompts` program, its frames through the op emulator (against uniform
launches and the default absorbed program), which frame slots get installed when, the copy list of `vsd_prompt_install` against a numpy
restatement, the worker's coalescing of frames that differ in `prompt`, and the error paths."""
import multiprocessing as mp
import os
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_prompt_cases as FC  # noqa: E402
from helpers_fake_pipeline import FakePipeline, bare_pipeline as _bare_pipeline  # noqa: E402

import videosd_amd.engine as E  # noqa: E402
from videosd_amd import config as C  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

H = Wd = 64
STEPS, B = 2, 3
PREP = dict(controlnet_scale=1.0, use_controlnet=True, use_graph=False)


def _frame(h, w, seed=1):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = ((xx * 5 + yy * 3) % 256).astype(np.uint8)[..., None]
    return (base // 2 + grad // 2).astype(np.uint8)


def _text(seed, tl=77):
    return (torch.randn(tl, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(seed)) * 0.5).half()


def _mad(a, b):
    return float(np.abs(a.astype(int) - b.astype(int)).mean())


def _names(eng):
    return [fn.__name__ for fn, _a, _k in Engine.flat_calls(eng.program.calls)]


def _attn(eng):
    return [(a, k) for fn, a, k in Engine.flat_calls(eng.program.calls) if fn.__name__ == "attention"]


def _is_cross(a):
    # self-attention reads q and k from one [rows][2c] buffer (ldq = 2c); cross-attention reads q from a [rows][c] buffer (ldq = c = heads * d)
    return a[1] == a[10] * a[11]


@pytest.fixture(scope="module")
def world():
    """ONE engine family with the width threshold lowered (so that the default program of the reduced-width network is the absorbed
    one), and every launch the tests below compare, computed once"""
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    keep = E.XATTN_ABSORB_MIN_C
    E.XATTN_ABSORB_MIN_C = 1
    try:
        eng = Engine(FC.FramePromptFakeOps(), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    finally:
        E.XATTN_ABSORB_MIN_C = keep
    assert all(t.xa_raw is not None for t in eng.unet.transformers)
    p = [eng.build_prompt(_text(7)), eng.build_prompt(_text(8))]
    eng.set_text_embeds(_text(7))
    frames = np.stack([_frame(H, Wd, 1), _frame(H, Wd, 2), _frame(H, Wd, 3)])
    out = {"eng": eng, "p": p, "frames": frames, "weights": (wu, wc, wv)}
    # the default program (absorbed), one launch per prompt
    eng.use_prompt(p[0])
    eng.prepare(H, Wd, STEPS, 0.6, batch=B, **PREP)
    out["default_names"] = _names(eng)
    out["default_attn"] = _attn(eng)
    out["default_soft"] = sum(1 for fn, a, k in Engine.flat_calls(eng.program.calls) if fn.__name__ == "conv" and k.get("softmax_cols"))
    out["default"] = [eng.infer_u8(frames)]
    eng.use_prompt(p[1])
    out["default"].append(eng.infer_u8(frames))
    # the per-frame program
    eng.use_prompts([p[0], p[1], p[0]])
    plan = eng.prepare(H, Wd, STEPS, 0.6, batch=B, frame_prompts=True, **PREP)
    out["plan"] = dict(plan)
    out["fp_names"] = _names(eng)
    out["fp_attn"] = _attn(eng)
    out["fp_soft"] = sum(1 for fn, a, k in Engine.flat_calls(eng.program.calls) if fn.__name__ == "conv" and k.get("softmax_cols"))
    ops = eng.ops
    out["installs_prepare"] = list(ops.installs)
    runs = {}
    for name, idx in (("010", [0, 1, 0]), ("100", [1, 0, 0]), ("000", [0, 0, 0]), ("111", [1, 1, 1])):
        del ops.installs[:]
        eng.use_prompts([p[i] for i in idx])
        runs[name] = (eng.infer_u8(frames), list(ops.installs))
    out["runs"] = runs
    return out


# ------------------------------------------------------------------------------------------ the recorded programs
def test_default_program_is_unchanged(world):
    """frame_prompts off: the absorbed program of test_engine_host_logic.test_absorbed_cross_attention_wiring -- per block and step one
    softmax_cols conv, and the self-attentions as the only attention calls, none of them a cross-attention"""
    eng = world["eng"]
    nblk = len(eng.unet.transformers) + len(eng.cn.transformers)
    assert world["default_soft"] == STEPS * nblk and len(world["default_attn"]) == STEPS * nblk
    assert not any(_is_cross(a) for a, _k in world["default_attn"])
    # ... and with the shipped threshold (no block of this network is wide enough): the explicit form with ONE problem of B*hw query rows
    wu, wc, wv = world["weights"]
    e2 = Engine(FC.FramePromptFakeOps(), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    e2.set_text_embeds(_text(7))
    plan = e2.prepare(H, Wd, STEPS, 0.6, batch=B, **PREP)
    assert plan["frame_prompts"] is False and e2.ops.installs == []
    att = _attn(e2)
    cross = [(a, k) for a, k in att if _is_cross(a)]
    soft = sum(1 for fn, a, k in Engine.flat_calls(e2.program.calls) if fn.__name__ == "conv" and k.get("softmax_cols"))
    assert soft == 0 and len(att) == 2 * STEPS * nblk and len(cross) == STEPS * nblk
    for a, k in cross:
        assert k == {} and a[9] == 77 and a[8] % B == 0 and tuple(a[2].shape) == (77, a[1]) and a[5] == 128
    names = _names(e2)
    # the per-frame program of the same engine: the same calls in the same order, only the cross-attention's arguments differ
    e2.prepare(H, Wd, STEPS, 0.6, batch=B, frame_prompts=True, **PREP)
    assert _names(e2) == names
    # ... and back: the default program again, reading a single-prompt block
    plan = e2.prepare(H, Wd, STEPS, 0.6, batch=B, **PREP)
    assert plan["frame_prompts"] is False and _names(e2) == names and isinstance(e2.pblock.layout, E.PromptLayout)
    assert all(k == {} for a, k in _attn(e2) if _is_cross(a))


def test_per_frame_program_records_every_cross_attention_in_the_explicit_form(world):
    eng = world["eng"]
    nblk = len(eng.unet.transformers) + len(eng.cn.transformers)
    assert world["plan"]["frame_prompts"] is True
    assert world["fp_soft"] == 0  # no absorbed cross-attention although every block is wide enough for it
    att = world["fp_attn"]
    cross = [(a, k) for a, k in att if _is_cross(a)]
    assert len(att) == 2 * STEPS * nblk and len(cross) == STEPS * nblk
    sizes = {(H // 8 >> i) * (Wd // 8 >> i) for i in range(len(C.MINI_UNET.block_out_channels))}
    for a, k in cross:
        c = a[1]
        assert k == dict(batch=B, k_brows=77, vt_bcols=128), k
        assert a[9] == 77 and a[8] in sizes  # sk = the text length, sq = the tokens of ONE image
        assert tuple(a[2].shape) == (B * 77, c) and tuple(a[4].shape) == (c, B * 128) and a[5] == B * 128
    # the layout holds K and V^T only
    lay = eng.pblock.layout
    assert isinstance(lay, E.FramePromptLayout) and {k[2] for k in lay.items} == {"k", "vt"} and not lay.absorbed
    assert (lay.tl, lay.ldt, lay.frames) == (77, 128, B)


# ------------------------------------------------------------------------------------------ results
def test_frames_of_a_mixed_launch_are_the_frames_of_uniform_launches(world):
    runs = world["runs"]
    mixed, uniform = runs["010"][0], {0: runs["000"][0], 1: runs["111"][0]}
    for i, pi in enumerate([0, 1, 0]):
        assert np.array_equal(mixed[i], uniform[pi][i]), i  # (the emulator has no rounding that depends on the neighbours)
        # the default absorbed program with that prompt: the bound of the absorbed-versus-explicit test
        assert _mad(mixed[i], world["default"][pi][i]) < 0.3, (i, _mad(mixed[i], world["default"][pi][i]))
    # the prompt matters: the existing prompt-change assertion on this network, frame for frame
    for i in range(B):
        assert _mad(uniform[0][i], uniform[1][i]) > 1.0


def test_only_the_changed_slots_are_installed(world):
    runs = world["runs"]
    assert sorted(world["installs_prepare"]) == [0, 1, 2]  # a fresh per-frame block: every slot, once
    assert runs["010"][1] == []            # the lists `prepare` saw: nothing to do
    assert sorted(runs["100"][1]) == [0, 1]  # [p0,p1,p0] -> [p1,p0,p0]
    assert runs["000"][1] == [0]           # -> [p0,p0,p0]
    assert sorted(runs["111"][1]) == [0, 1, 2]
    uniform = {0: runs["000"][0], 1: runs["111"][0]}
    for i, pi in enumerate([1, 0, 0]):
        assert np.array_equal(runs["100"][0][i], uniform[pi][i]), i


def test_two_slots_on_different_lanes_keep_their_own_lists(world):
    eng, p, frames, runs = world["eng"], world["p"], world["frames"], world["runs"]
    slot = eng.make_slot(lane=1)
    assert slot.pblock is None and slot._prompt_slots is None and slot._want_list is None
    slot.use_prompts([p[1], p[1], p[0]])
    slot.prepare(H, Wd, STEPS, 0.6, batch=B, frame_prompts=True, **PREP)
    assert slot.pblock is not eng.pblock and slot.pblock.layout is eng.pblock.layout
    assert slot.family["seg_tables"] is eng.family["seg_tables"] and len(eng.family["seg_tables"]) == 1
    eng.use_prompts([p[0], p[1], p[0]])
    a1 = eng.infer_u8(frames)
    b1 = slot.infer_u8(frames)
    a2 = eng.infer_u8(frames)
    assert np.array_equal(a1, runs["010"][0]) and np.array_equal(a2, a1)
    uniform = {0: runs["000"][0], 1: runs["111"][0]}
    for i, pi in enumerate([1, 1, 0]):
        assert np.array_equal(b1[i], uniform[pi][i]), i
    del slot.ops.installs[:]
    slot.infer_u8(frames)
    assert slot.ops.installs == []


# ------------------------------------------------------------------------------------------ the copy list against numpy
@pytest.mark.parametrize("frames", [1, 2, 5])
def test_segment_table_against_numpy(frames):
    widths = (320, 640, 1280)
    nets = FC.stub_nets(widths)
    src_lay = E.PromptLayout(nets, 77)
    dst_lay = E.FramePromptLayout(nets, 77, frames)
    assert src_lay.absorbed == {(0, 1), (0, 2)}  # (the cache entry's absorbed weights lie between the tensors that are copied)
    segs = E.prompt_segments(src_lay, dst_lay)
    assert len(segs) == 2 * len(widths)
    for so, do, rows, rb, pitch, fstride in segs:
        assert all(v % 16 == 0 and v >= 0 for v in (so, do, rb, pitch, fstride)) and rows >= 1
        assert pitch == frames * fstride and fstride == rb  # the frame slots of a destination row
        assert so + rows * rb <= src_lay.nbytes and do + (rows - 1) * pitch + frames * fstride <= dst_lay.nbytes
    ks = [s for s, key in zip(segs, dst_lay.items) if key[2] == "k"]
    vs = [s for s, key in zip(segs, dst_lay.items) if key[2] == "vt"]
    assert [(s[2], s[3]) for s in ks] == [(1, 77 * c * 2) for c in widths]          # K: one run
    assert [(s[2], s[3], s[4]) for s in vs] == [(c, 256, frames * 256) for c in widths]  # V^T: c rows of all ldt columns
    rng = np.random.default_rng(frames)
    src = rng.integers(0, 256, src_lay.nbytes, dtype=np.uint8)
    for f in range(frames):
        dst = np.full(dst_lay.nbytes, FC.SENTINEL, np.uint8)
        want = FC.expected_install(src_lay, dst_lay, src, dst, f)
        FC.apply_segments(segs, src, dst, f)
        assert np.array_equal(dst, want), f
        # slot f holds the source, every other slot and the padding between the tensors still the sentinel
        for key, item in dst_lay.items.items():
            d, s = FC.tensor_u16(dst, item), FC.tensor_u16(src, src_lay.items[key])
            mine = d[f * 77:(f + 1) * 77] if key[2] == "k" else d[:, f * 128:(f + 1) * 128]
            assert np.array_equal(mine, s)
        assert int((dst != FC.SENTINEL).sum()) <= sum(s[2] * s[3] for s in segs)
        assert int((want == FC.SENTINEL).sum()) >= dst_lay.nbytes - sum(s[2] * s[3] for s in segs)
    with pytest.raises(ValueError, match="same text length"):
        E.prompt_segments(E.PromptLayout(nets, 64), dst_lay)


# ------------------------------------------------------------------------------------------ dispatch: frames that differ in `prompt`
SUBMITS = []


class PromptPipeline(FakePipeline):
    """stand-in that records what every launch was given"""

    def submit_batch(self, imgs, lane=0, **opts):
        SUBMITS.append((len(imgs), opts.get("prompt"), opts.get("prompts"), opts.get("seed"), opts.get("strength")))
        return super().submit_batch(imgs, lane=lane, **opts)


class PerFramePromptPipeline(PromptPipeline):
    per_frame_prompt = True
    per_frame_seed = True


def _serve(factory, requests):
    """the worker loop in a thread of this process, with the requests ALREADY queued when it starts -> (launches, replies)"""
    from videosd_amd.dispatch import _worker_main

    del SUBMITS[:]
    parent, child = mp.Pipe()
    for k, opts in enumerate(requests):
        img = Image.fromarray(np.full((12, 16, 3), 10 * (k + 1), np.uint8), "RGB")
        parent.send((k, "infer", (img,), dict(height=12, width=16, **opts)))
    parent.send(None)
    t = threading.Thread(target=_worker_main, args=(child, factory, dict(model="m", controlnet="c", device=0)), kwargs=dict(max_batch=3))
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert parent.recv() == ("ready", None)
    replies = {}
    while parent.poll(0):
        rid, ok, payload = parent.recv()
        assert ok, payload
        replies[rid] = np.asarray(payload)
    return list(SUBMITS), replies


def test_worker_coalesces_frames_that_differ_in_prompt_and_seed():
    reqs = [dict(prompt="a cat", seed=7), dict(prompt="a dog", seed=8), dict(prompt=["a cat"], seed=9)]
    launches, replies = _serve("test_frame_prompts_host:PerFramePromptPipeline", reqs)
    assert launches == [(3, "a cat", ["a cat", "a dog", ["a cat"]], [7, 8, 9], None)], launches  # ONE launch, request order
    assert sorted(replies) == [0, 1, 2]
    for k in range(3):  # each reply is its request's frame (inverted by the stand-in), out of a launch of three
        assert int(replies[k][1, 1, 0]) == 255 - 10 * (k + 1) and int(replies[k][0, 0, 1]) == 3


def test_worker_without_the_attribute_sends_other_prompts_out_separately():
    reqs = [dict(prompt="a cat"), dict(prompt="a dog"), dict(prompt="a dog")]
    launches, replies = _serve("test_frame_prompts_host:PromptPipeline", reqs)
    assert launches == [(1, "a cat", None, None, None), (2, "a dog", None, None, None)], launches  # as today: `prompts` never appears
    assert int(replies[0][0, 0, 1]) == 1 and int(replies[1][0, 0, 1]) == 2 and int(replies[2][0, 0, 1]) == 2


def test_worker_never_merges_a_frame_whose_strength_differs():
    reqs = [dict(prompt="a cat", strength=0.4), dict(prompt="a dog", strength=0.4), dict(prompt="a dog", strength=0.6)]
    launches, replies = _serve("test_frame_prompts_host:PerFramePromptPipeline", reqs)
    assert launches == [(2, "a cat", ["a cat", "a dog"], [42, 42], 0.4), (1, "a dog", ["a dog"], [42], 0.6)], launches
    assert [int(replies[k][0, 0, 1]) for k in range(3)] == [2, 2, 1]


# ------------------------------------------------------------------------------------------ error paths
def test_error_paths(world, tmp_path):
    imgs = [Image.new("RGB", (16, 16))] * 2
    with pytest.raises(ValueError, match="frame_prompts=True"):  # `prompts` without the switch
        _bare_pipeline().submit_batch(imgs, prompts=["a", "b"])
    with pytest.raises(ValueError, match="one prompt per frame"):  # the wrong length
        _bare_pipeline(frame_prompts=True).submit_batch(imgs, prompts=["a", "b", "c"])
    with pytest.raises(ValueError, match="SDXL"):  # the pooled embedding is part of an SDXL program
        _bare_pipeline(frame_prompts=True, is_xl=True).submit_batch(imgs, prompts=["a", "b"])
    with pytest.raises(ValueError, match="one frame per launch"):
        _bare_pipeline(frame_prompts=True, honor_ref_flag=True).submit_batch(imgs, prompts=["a", "b"], ref=True)
    with pytest.raises(ValueError, match="frame_prompts=True"):
        _bare_pipeline(frame_prompts=True).export_plan(str(tmp_path / "x.vsdplan"))
    # the engine: the wrong count, mixed text lengths (at prepare and at a launch), a plan file of a per-frame program
    from videosd_amd.plan import export_plan

    eng, p = world["eng"], world["p"]
    with pytest.raises(ValueError, match="frame_prompts=True"):
        export_plan(eng, str(tmp_path / "y.vsdplan"))
    short = eng.build_prompt(_text(9, tl=64))
    eng.family["prompt"] = p[0]  # (build_prompt does not change the default prompt; the layout of the last build is not used by these paths)
    eng.use_prompts([p[0], p[1]])
    with pytest.raises(ValueError, match="2 prompt"):
        eng.launch()
    eng.use_prompts([p[0], short, p[0]])
    with pytest.raises(ValueError, match="same text length"):
        eng.launch()
    with pytest.raises(ValueError, match="same text length"):
        eng.prepare(H, Wd, STEPS, 0.6, batch=B, frame_prompts=True, **PREP)
    eng.use_prompts([short] * B)
    with pytest.raises(ValueError, match="prepare again"):  # a whole launch of another length: another layout, as for one prompt per launch
        eng.launch()
    eng.use_prompts([p[0], p[1], p[0]])
    assert np.array_equal(eng.infer_u8(world["frames"]), world["runs"]["010"][0])  # ... and nothing was disturbed

    class NoInstallOps:
        pass

    e = Engine.__new__(Engine)
    e.ops = NoInstallOps()
    with pytest.raises(ValueError, match="prompt_install"):
        e.prepare(96, 160, 2, 0.5, frame_prompts=True)

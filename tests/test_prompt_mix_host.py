"""Prompt mixes without a GPU (include/vsd.h THE PROMPT MIX): the canonical form of a mix and its refusals (videosd_amd/promptmix.py), the
linearity of every item of a prompt's constants in the text embeddings, the host twin vsd_prompt_mix_host against the numpy restatement
byte for byte, the engine on the op emulator, the worker's coalescing and the dispatcher's component syncs."""
import asyncio
import concurrent.futures
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_prompt_cases as FC  # noqa: E402
import prompt_mix_cases as MC  # noqa: E402
import test_frame_prompts_host as FPH  # noqa: E402
from helpers_fake_pipeline import bare_pipeline  # noqa: E402

import videosd_amd.engine as E  # noqa: E402
from videosd_amd import blocks as BK  # noqa: E402
from videosd_amd import config as C  # noqa: E402
from videosd_amd import dispatch as D  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import pipeline as P  # noqa: E402
from videosd_amd import promptmix as PM  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

VSD_ERR_ARG = -1


# ------------------------------------------------------------------------------------------ the canonical form
def test_a_mix_of_one_component_is_that_prompt():
    for spelled in ({"mix": [["a cat", 1.0]]}, {"mix": [["a cat", 0.2], ["a cat", 5]]}, {"mix": [["a dog", 0.0], ["a cat", 3.0]]},
                    {"mix": (("a cat", 1e-3),)}):
        assert PM.canonical(spelled) == "a cat"
        assert PM.prompt_key(spelled) == "a cat" == PM.prompt_key("a cat") == D.prompt_key(spelled) == P._prompt_key(spelled)
        assert PM.component_prompts(spelled) == ["a cat"]
    # plain prompts pass through unchanged, with the keys they always had
    lst = ["pixar, cg"]
    assert PM.canonical("x") == "x" and PM.canonical(lst) is lst
    assert PM.prompt_key(lst) == ("pixar, cg",) == D.prompt_key(lst) == P._prompt_key(lst) and PM.component_prompts(lst) == [lst]
    # ... and the class takes the object path of the plain prompt: the cache entry itself, no PromptMix
    p = bare_pipeline()
    blk = object()
    p._prompts["a cat"] = blk
    prompt, plist = p._launch_prompts(1, {"mix": [["a cat", 2.0]]}, None, False)
    assert prompt == "a cat" and plist is None and p._prompt_source(prompt) is blk and list(p._prompts) == ["a cat"]


def test_merging_zero_dropping_ordering_and_weights():
    m = PM.canonical({"mix": [["b", 1.0], ["a", 0.5], ["c", 0.0], ["b", 0.5], ["d", 1.0]]})
    assert isinstance(m, PM.Mix) and m.texts == ("a", "b", "d")
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    assert m.weights == (f32(0.5 / 3.0), f32(1.5 / 3.0), f32(1.0 / 3.0))
    assert all(w == f32(w) for w in m.weights) and abs(sum(m.weights) - 1.0) < 2e-7
    # weights are fp32(w / sum) with the quotient in fp64 -- whatever scale the caller wrote them in
    for a, b in ((0.3, 0.7), (3, 7), (1e-9, 7e-9 / 3), (1, 2 ** 25), (0.1, 0.2)):
        m = PM.canonical({"mix": [["x", a], ["y", b]]})
        assert m.weights == (f32(np.float64(a) / (np.float64(a) + np.float64(b))), f32(np.float64(b) / (np.float64(a) + np.float64(b))))
    assert PM.fp32(0.1) == f32(0.1) and PM.fp32(1.0 + 2.0 ** -24) == 1.0 and PM.fp32(1.0 + 3 * 2.0 ** -24) == f32(1.0 + 2.0 ** -22)
    # two spellings of one mix compare equal, hash equal, and are one key everywhere
    s1 = {"mix": [["text a", 0.3], ["text b", 0.7]]}
    s2 = {"mix": [["text b", 0.35], ["text a", 0.3], ["text b", 0.35], ["zzz", 0]]}
    assert PM.canonical(s1) == PM.canonical(s2) and hash(PM.prompt_key(s1)) == hash(PM.prompt_key(s2))
    assert D.prompt_key(s1) == P._prompt_key(s2) == PM.canonical(s1)
    assert PM.canonical(s1) != PM.canonical({"mix": [["text a", 0.31], ["text b", 0.69]]})
    assert PM.component_prompts(s2) == ["text a", "text b"]
    assert PM.canonical(PM.canonical(s1)) is not None and PM.canonical(PM.canonical(s1)) == PM.canonical(s1)  # idempotent
    four = PM.canonical({"mix": [[t, 1] for t in "dcba"]})
    assert four.texts == ("a", "b", "c", "d") and four.weights == (0.25,) * 4


@pytest.mark.parametrize("bad,match", [
    ({"blend": [["a", 1.0]]}, "must be a mix"),
    ({"mix": [["a", 1], ["b", 1]], "fade": 3}, 'one key "mix"'),
    ({"mix": [[t, 1.0] for t in "abcde"]}, "at most 4 components, this one has 5"),
    ({"mix": [["a", 0.0], ["b", 0]]}, "positive weight"),
    ({"mix": []}, "positive weight"),
    ({"mix": [["a", 1.0], ["b", -0.25]]}, "negative"),
    ({"mix": [["a", 1.0], ["b", float("nan")]]}, "not finite"),
    ({"mix": [["a", 1.0], ["b", float("inf")]]}, "not finite"),
    ({"mix": [["a", 1.0], [7, 1.0]]}, "must be a string"),
    ({"mix": [["a", 1.0], [["b"], 1.0]]}, "must be a string"),
    ({"mix": [["a", "1.0"]]}, "must be a number"),
    ({"mix": [["a", 1.0, 2.0]]}, "pair"),
    ({"mix": 5}, "list of"),
])
def test_refusals_come_before_any_device_work(bad, match):
    with pytest.raises(ValueError, match=match):
        PM.canonical(bad)
    imgs = [Image.new("RGB", (16, 16))] * 2
    # phase 1 of submit_batch: a bare pipeline has no model, so anything that got past the check would fail differently
    with pytest.raises(ValueError, match=match):
        bare_pipeline().submit_batch(imgs[:1], prompt=bad)
    with pytest.raises(ValueError, match=match):
        bare_pipeline(frame_prompts=True).submit_batch(imgs, prompts=["fine", bad])


def test_five_components_that_merge_to_four_are_a_mix():
    m = PM.canonical({"mix": [["a", 1], ["b", 1], ["c", 1], ["d", 1], ["a", 1]]})
    assert m.texts == ("a", "b", "c", "d") and m.weights[0] == float(np.float32(0.4))


def test_sdxl_and_the_plan_files_refuse_a_mix_by_name(tmp_path):
    mix = {"mix": [["a", 0.5], ["b", 0.5]]}
    imgs = [Image.new("RGB", (16, 16))] * 2
    with pytest.raises(ValueError, match="mix of more than one component.*SDXL program has the pooled text embedding"):
        bare_pipeline(is_xl=True).submit_batch(imgs[:1], prompt=mix)
    with pytest.raises(ValueError, match="mix of more than one component.*SDXL program has the pooled text embedding"):
        bare_pipeline(is_xl=True, frame_prompts=True).submit_batch(imgs, prompts=[mix, mix])
    with pytest.raises(ValueError, match="export_plan: `prompt` is a mix"):
        bare_pipeline().export_plan(str(tmp_path / "x.vsdplan"), prompt=mix)
    with pytest.raises(ValueError, match="export_prompt: `prompt` is a mix"):
        bare_pipeline().export_prompt(str(tmp_path / "x.vsdprompt"), mix)


# ------------------------------------------------------------------------------------------ linearity guard
PROMPT_INDEPENDENT = {"xa2_b"}


def _item_names():
    lay = E.PromptLayout(FC.stub_nets((320, 640)), 77)
    assert lay.absorbed  # (the layout under test has absorbed blocks: every item name appears)
    return sorted({k[2] for k in lay.items})


def _block_fp64(e, wk, wv, wq, wo, bo, gamma, beta, heads):
    """every item of ONE transformer block's prompt constants from the embeddings `e`, in fp64: the K / V projections (to_k / to_v, no
    bias) and the absorbed weights through packing.pack_cross_attention"""
    from videosd_amd.packing import pack_cross_attention

    k, v = e @ wk.t(), e @ wv.t()
    x1, x2 = pack_cross_attention(k, v, wq, wo, bo, gamma, beta, heads, dtype=torch.float64)
    return {"k": k, "vt": v.t(), "xa1_w": x1.weight, "xa1_s": x1.ln_s, "xa1_t": x1.ln_t, "xa2_w": x2.weight, "xa2_b": x2.bias}


def test_every_item_is_linear_in_the_embeddings_or_listed_as_independent():
    """block(sum w_i e_i) == sum w_i block(e_i) to fp64 rounding for every item name of PromptLayout.items that is not listed as
    prompt-independent; the listed ones do not move with the prompt at all.  A NEW item name fails here (and in blocks.mix_segments) until
    someone decides which kind it is."""
    names = _item_names()
    assert set(names) == set(BK.MIX_ITEM_KINDS), "a prompt item without a mix kind (blocks.MIX_ITEM_KINDS), or a kind without an item"
    assert {n for n, k in BK.MIX_ITEM_KINDS.items() if k == L.MIX_COPY} == PROMPT_INDEPENDENT
    assert {n for n, k in BK.MIX_ITEM_KINDS.items() if k == L.MIX_F32} == {"xa1_s", "xa1_t"}
    g = torch.Generator().manual_seed(5)
    c, heads, cross, tl = 32, 4, 24, 9
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    wk, wv, wq, wo, bo, gamma, beta = rnd(c, cross), rnd(c, cross), rnd(c, c), rnd(c, c), rnd(c), rnd(c), rnd(c)
    es = [rnd(tl, cross) for _ in range(3)]
    ws = [0.25, 0.625, 0.125]
    blocks = [_block_fp64(e, wk, wv, wq, wo, bo, gamma, beta, heads) for e in es]
    mixed = _block_fp64(sum(w * e for w, e in zip(ws, es)), wk, wv, wq, wo, bo, gamma, beta, heads)
    assert set(mixed) == set(names), "an item the test does not compute"
    for name in names:
        if name in PROMPT_INDEPENDENT:
            assert all(torch.equal(b[name], blocks[0][name]) for b in blocks) and torch.equal(mixed[name], blocks[0][name]), name
            continue
        ref = sum(w * b[name] for w, b in zip(ws, blocks))
        err = float((mixed[name] - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
        assert err < 1e-12, (name, err)
        assert float((blocks[0][name] - blocks[1][name]).abs().max()) > 1e-3, name  # (it does depend on the prompt)
    with pytest.raises(ValueError, match="MIX_ITEM_KINDS"):  # a new item name, before anyone has decided
        lay = E.PromptLayout(FC.stub_nets((320,)), 77)
        lay.items[(0, 0, "new_item")] = (lay.nbytes, (16,), torch.float16)
        BK.mix_segments(lay, lay)


# ------------------------------------------------------------------------------------------ the host twin against the restatement
def _seg_array(segs):
    return np.ascontiguousarray(np.array(segs, dtype=np.int64).reshape(-1, 8))


def _host(srcs, weights, dst, segs, frame, n=None):
    """vsd_prompt_mix_host on numpy byte arrays -> status (dst is written in place)"""
    lib = L.load()
    n = len(srcs) if n is None else n
    ptrs = (ctypes.c_void_p * max(1, len(srcs)))(*[s.ctypes.data for s in srcs])
    ws = (ctypes.c_float * max(1, len(weights)))(*weights)
    tab = _seg_array(segs)
    return lib.vsd_prompt_mix_host(ptrs, ws, n, dst.ctypes.data, tab.ctypes.data, len(segs), frame)


def _aligned(nbytes, fill=None, src=None):
    """a 16-byte aligned uint8 array of nbytes"""
    raw = np.empty(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes]
    if fill is not None:
        a[:] = fill
    if src is not None:
        a[:] = src
    return a


WEIGHTS = {1: (1.0,), 2: (0.25, 0.75), 3: (0.5, 0.3, 0.2), 4: (0.1, 0.2, 0.3, 0.4)}


def mix_problem(n, seed=0, B=3):
    segs, sbytes, dbytes = MC.awkward_segments(B)
    rng = np.random.default_rng(100 * n + seed)
    srcs = [_aligned(sbytes, src=MC.finite_block(rng, sbytes, segs)) for _ in range(n)]
    return segs, srcs, PM.normalized(WEIGHTS[n]), sbytes, dbytes


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_host_twin_against_the_restatement_byte_for_byte(n):
    B = 3
    segs, srcs, ws, sbytes, dbytes = mix_problem(n)
    assert n == 1 or abs(sum(ws) - 1.0) < 2e-7
    assert ws == (1.0,) or n > 1
    tail = 64  # sentinel bytes behind the destination
    written = {f: None for f in range(B)}
    for f in range(B):  # one frame slot of a per-frame destination: the pitched segments
        dst = _aligned(dbytes + tail, fill=MC.SENTINEL)
        want = MC.mix_numpy(srcs, ws, dst.copy(), segs, f)
        assert _host(srcs, ws, dst, segs, f) == 0
        assert np.array_equal(dst, want), (n, f, int((dst != want).sum()))
        assert bool((dst[dbytes:] == MC.SENTINEL).all())
        written[f] = dst != MC.SENTINEL
        # slot f holds the mix, the other slots and the gaps the sentinel: nothing outside the segments' own rows of slot f was touched
        mask = np.zeros(dbytes + tail, bool)
        for _so, do, rows, rb, pitch, fs, _k, _r in segs:
            for r in range(rows):
                mask[do + f * fs + r * pitch:do + f * fs + r * pitch + rb] = True
        assert bool((dst[~mask] == MC.SENTINEL).all())
    assert not (written[0] & written[1] & written[2]).any()
    # a whole block of the sources' own layout
    wsegs = MC.whole_segments(segs)
    dst = _aligned(sbytes + tail, fill=MC.SENTINEL)
    want = MC.mix_numpy(srcs, ws, dst.copy(), wsegs, 0)
    assert _host(srcs, ws, dst, wsegs, 0) == 0 and np.array_equal(dst, want)
    assert bool((dst[sbytes:] == MC.SENTINEL).all())
    for so, _do, rows, rb, _p, _f, kind, _r in segs:
        if kind == MC.COPY or n == 1:  # the copy segment is component 0's bytes; weight 1 alone is a byte-wise copy of everything
            assert np.array_equal(dst[so:so + rows * rb], srcs[0][so:so + rows * rb])
    if n > 1:
        assert not np.array_equal(dst[segs[0][0]:segs[0][0] + 80], srcs[0][segs[0][0]:segs[0][0] + 80])


def test_one_component_copies_any_bytes_and_zero_padding_stays_zero():
    segs, sbytes, _dbytes = MC.awkward_segments(1)
    wsegs = MC.whole_segments(segs)
    rng = np.random.default_rng(3)
    raw = _aligned(sbytes, src=rng.integers(0, 256, sbytes, dtype=np.uint8))  # NaNs, infinities, anything
    dst = _aligned(sbytes, fill=MC.SENTINEL)
    assert _host([raw], (1.0,), dst, wsegs, 0) == 0
    for so, _do, rows, rb, _p, _f, _k, _r in segs:
        assert np.array_equal(dst[so:so + rows * rb], raw[so:so + rows * rb])
    # zeros (V^T key padding, unused weight rows) stay +0 under any weights
    zs = [_aligned(sbytes, fill=0) for _ in range(4)]
    dst = _aligned(sbytes, fill=MC.SENTINEL)
    assert _host(zs, PM.normalized(WEIGHTS[4]), dst, wsegs, 0) == 0
    for so, _do, rows, rb, _p, _f, _k, _r in segs:
        assert not dst[so:so + rows * rb].any()


def test_host_twin_refusals():
    segs, srcs, ws, sbytes, dbytes = mix_problem(2)
    dst = _aligned(dbytes, fill=MC.SENTINEL)
    before = dst.copy()
    assert _host(srcs, ws, dst, segs, 3) == VSD_ERR_ARG and _host(srcs, ws, dst, segs, -1) == VSD_ERR_ARG  # frame outside [0, B)
    assert _host(srcs, ws, dst, segs, 0, n=0) == VSD_ERR_ARG and _host(srcs * 3, ws * 3, dst, segs, 0, n=5) == VSD_ERR_ARG
    for bad in ((-0.5, 1.5), (float("nan"), 1.0), (float("inf"), 0.0)):
        assert _host(srcs, bad, dst, segs, 0) == VSD_ERR_ARG
    assert _host([srcs[0], srcs[1][8:]], ws, dst, segs, 0) == VSD_ERR_ARG  # a misaligned source
    assert _host(srcs, ws, dst[8:], segs, 0) == VSD_ERR_ARG
    for field in (0, 1, 3, 4, 5):
        off = [list(s) for s in segs]
        off[2][field] += 8
        assert _host(srcs, ws, dst, off, 0) == VSD_ERR_ARG, field
    off = [list(s) for s in segs]
    off[1][6] = 3  # an unknown kind
    assert _host(srcs, ws, dst, off, 0) == VSD_ERR_ARG
    lib = L.load()
    assert lib.vsd_prompt_mix_host(None, None, 2, dst.ctypes.data, _seg_array(segs).ctypes.data, len(segs), 0) == VSD_ERR_ARG
    assert np.array_equal(dst, before)  # ... and nothing was written


def test_segment_lists_of_the_layouts():
    nets = FC.stub_nets((320, 640, 1280))
    src = E.PromptLayout(nets, 77)
    whole = BK.mix_segments(src, src)
    assert len(whole) == len(src.items)
    for (key, (off, shape, dt)), sg in zip(src.items.items(), whole):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
        assert sg == (off, off, 1, n, n, n, BK.MIX_ITEM_KINDS[key[2]], 0) and n % 16 == 0 and off + n <= src.nbytes
    for B in (1, 3):
        dst = E.FramePromptLayout(nets, 77, B)
        per = BK.mix_segments(src, dst)
        assert [s[:6] for s in per] == E.prompt_segments(src, dst) and all(s[6:] == (L.MIX_F16, 0) for s in per)
    with pytest.raises(ValueError, match="same text length"):
        BK.mix_segments(E.PromptLayout(nets, 64), E.FramePromptLayout(nets, 77, 2))


# ------------------------------------------------------------------------------------------ the engine on the op emulator
H = Wd = 64
STEPS, B = 2, 3
PREP = dict(controlnet_scale=1.0, use_controlnet=True, use_graph=False)


@pytest.fixture(scope="module")
def world():
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    keep = E.XATTN_ABSORB_MIN_C
    E.XATTN_ABSORB_MIN_C = 1  # (the absorbed program: every item kind is in the block)
    try:
        eng = Engine(MC.PromptMixFakeOps(), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    finally:
        E.XATTN_ABSORB_MIN_C = keep
    blocks = [eng.build_prompt(FPH._text(s)) for s in (7, 8, 9)]
    eng.set_text_embeds(FPH._text(7))
    frames = np.stack([FPH._frame(H, Wd, s) for s in (1, 2, 3)])
    return eng, blocks, frames


def _restated_block(mix):
    lay = mix.layout
    want = np.zeros(lay.nbytes, np.uint8)
    MC.mix_numpy([c.buf.numpy() for c in mix.components], mix.weights, want, BK.mix_segments(lay, lay), 0)
    return want


def test_default_engine_forms_a_mix_with_one_launch_and_nothing_else(world, monkeypatch):
    eng, blocks, frames = world
    ops = eng.ops
    assert {k[2] for k in blocks[0].layout.items} == set(BK.MIX_ITEM_KINDS)
    frames = frames[0]  # (one frame per launch: what is under test is the step ahead of the program)
    eng.use_prompt(blocks[0])
    eng.prepare(H, Wd, STEPS, 0.6, batch=1, **PREP)
    plain = eng.infer_u8(frames)
    base_syncs = None
    builds = []
    monkeypatch.setattr(Engine, "build_prompt", lambda self, e: builds.append(1))
    for mix in (BK.PromptMix(blocks[:2], PM.normalized((0.25, 0.75))), BK.PromptMix(blocks, PM.normalized((0.2, 0.3, 0.5)))):
        del ops.mixes[:]
        ops.copies = ops.syncs = 0
        eng.use_prompt(mix)
        out = eng.infer_u8(frames)
        assert len(ops.mixes) == 1 and ops.mixes[0] == (tuple(c.buf.data_ptr() for c in mix.components), mix.weights, 0)
        assert ops.copies == 0 and builds == []
        base_syncs = ops.syncs if base_syncs is None else base_syncs
        assert np.array_equal(eng.pblock.buf.numpy(), _restated_block(mix))  # bit for bit the restatement
        assert torch.equal(eng.pblock.view(0, 0, "xa2_b"), blocks[0].view(0, 0, "xa2_b"))  # the bias: component 0's, not a sum
        assert not np.array_equal(out, plain)
        # the same mix again -- the same object, or an equal one made anew -- costs nothing
        del ops.mixes[:]
        ops.syncs = 0
        eng._sync_prompt()
        eng.use_prompt(BK.PromptMix(mix.components, mix.weights))
        again = eng.infer_u8(frames)
        assert ops.mixes == [] and ops.copies == 0 and np.array_equal(again, out)
        assert ops.syncs == base_syncs  # what a launch synchronises anyway (the emulator's infer_u8), nothing for the mix
    # a plain launch synchronises exactly as often: the mix added none
    eng.use_prompt(blocks[0])
    ops.syncs = ops.copies = 0
    assert np.array_equal(eng.infer_u8(frames), plain) and ops.copies == 1 and ops.syncs == base_syncs
    # other weights, or the components the other way round: a new launch
    for mix in (BK.PromptMix(blocks[:2], PM.normalized((0.5, 0.5))), BK.PromptMix(blocks[1::-1], PM.normalized((0.5, 0.5)))):
        del ops.mixes[:]
        eng.use_prompt(mix)
        eng._sync_prompt()  # (what `launch` runs ahead of the program)
        assert len(ops.mixes) == 1 and np.array_equal(eng.pblock.buf.numpy(), _restated_block(mix))
    # one component: the component's bytes
    eng.use_prompt(BK.PromptMix([blocks[1]], (1.0,)))
    eng._sync_prompt()
    assert np.array_equal(eng.pblock.buf.numpy(), blocks[1].buf.numpy())


def test_frame_prompt_engine_rewrites_only_the_slot_of_the_mix(world):
    eng, blocks, frames = world
    slot = eng.make_slot(lane=1)
    ops = slot.ops
    a, b = blocks[0], blocks[1]
    mix = BK.PromptMix([a, b], PM.normalized((0.25, 0.75)))
    slot.use_prompts([a, a, b])
    slot.prepare(H, Wd, STEPS, 0.6, batch=B, frame_prompts=True, **PREP)
    base = slot.infer_u8(frames)
    del ops.installs[:], ops.mixes[:]
    ops.copies = 0
    slot.use_prompts([a, mix, b])
    got = slot.infer_u8(frames)
    assert ops.installs == [] and ops.copies == 0 and [m[2] for m in ops.mixes] == [1]  # slot 1 only, by one prompt_mix
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]) and not np.array_equal(got[1], base[1])
    # the slot holds the restatement's K rows / V^T columns
    lay, src_lay = slot.pblock.layout, a.layout
    want = np.full(lay.nbytes, MC.SENTINEL, np.uint8)
    MC.mix_numpy([a.buf.numpy(), b.buf.numpy()], mix.weights, want, BK.mix_segments(src_lay, lay), 1)
    touched = want != MC.SENTINEL
    assert np.array_equal(slot.pblock.buf.numpy()[touched], want[touched])
    del ops.mixes[:]
    slot.use_prompts([a, BK.PromptMix([a, b], mix.weights), b])  # an equal mix: nothing to do
    assert np.array_equal(slot.infer_u8(frames), got) and ops.mixes == [] and ops.installs == []
    slot.use_prompts([mix, mix, mix])
    uniform = slot.infer_u8(frames)
    assert sorted(m[2] for m in ops.mixes) == [0, 2] and np.array_equal(uniform[1], got[1])
    # a mix whose components differ in text length, and one of another length than the plan's
    short = eng.build_prompt(FPH._text(9, tl=64))
    eng.family["prompt"] = a
    with pytest.raises(ValueError, match="same text length"):
        BK.PromptMix([a, short], (0.5, 0.5))
    slot.use_prompts([BK.PromptMix([short, short], (0.5, 0.5))] * 3)
    with pytest.raises(ValueError, match="prepare again"):
        slot.launch()
    eng.use_prompt(BK.PromptMix([short, short], (0.5, 0.5)))
    with pytest.raises(RuntimeError, match="prepare again"):
        eng.launch()
    eng.use_prompt(a)
    with pytest.raises(ValueError, match="1..4 components"):
        BK.PromptMix([a] * 5, (0.2,) * 5)
    with pytest.raises(ValueError, match="finite and not negative"):
        BK.PromptMix([a, b], (1.5, -0.5))


def test_the_class_caches_components_and_never_the_mix():
    """VideoSDPipeline._prompt_source with a stand-in for the cache's builder: every component goes through `_cache_prompt`, the mix
    itself never does; a sweep leaves the cache with its two texts; components of one launch do not evict each other"""
    p = bare_pipeline(max_prompts=2)
    lay = SimpleNamespace(tl=77)
    built = []

    def build(embeds):
        built.append(embeds)
        return SimpleNamespace(layout=lay, text=None, buf=None)

    p.model = SimpleNamespace(build_prompt=build)
    p.encode_prompt = lambda text: text
    for i in range(20):
        prompt, plist = p._launch_prompts(1, {"mix": [["text a", 1.0 - i / 20], ["text b", i / 20]]}, None, False)
        src = p._prompt_source(prompt)
        if i == 0:
            assert src is p._prompts["text a"]  # weight zero for "text b": the plain prompt
        else:
            assert isinstance(src, BK.PromptMix) and src.components == (p._prompts["text a"], p._prompts["text b"])
            assert src.weights == PM.normalized((1.0 - i / 20, i / 20))
    assert list(p._prompts) == ["text a", "text b"] and built == ["text a", "text b"]
    # three components with room for two: none of the launch's own is dropped while it is put together
    src = p._prompt_source(PM.canonical({"mix": [["x", 1], ["y", 1], ["z", 1]]}))
    assert [c for c in src.components] == [p._prompts[t] for t in "xyz"] and built[2:] == ["x", "y", "z"]
    # a launch in flight on a per-frame engine protects the components of the mixes its slots hold
    eng = SimpleNamespace(_prompt_slots=SimpleNamespace(src=[src, None]))
    p._in_flight.append(P.Launch(eng, 2, 0, None, False, ()))
    assert p._prompts_in_use() == {id(c) for c in src.components}
    p._cache_prompt("w", prompt="w")
    assert {"x", "y", "z", "w"} <= set(p._prompts)


# ------------------------------------------------------------------------------------------ the worker
MIXES = [{"mix": [["a cat", 0.3], ["a dog", 0.7]]}, {"mix": [["a cat", 0.5], ["a dog", 0.5]]}, {"mix": [["a dog", 0.9], ["a cat", 0.1]]}]


def test_worker_coalesces_frames_that_differ_in_their_mix():
    launches, replies = FPH._serve("test_frame_prompts_host:PerFramePromptPipeline", [dict(prompt=m) for m in MIXES])
    assert launches == [(3, MIXES[0], MIXES, [42, 42, 42], None)], launches  # ONE launch, the mixes in request order
    assert sorted(replies) == [0, 1, 2] and all(int(replies[k][0, 0, 1]) == 3 for k in range(3))


def test_worker_without_per_frame_prompts_shares_a_launch_between_equal_mixes_only():
    reqs = [dict(prompt=MIXES[0]), dict(prompt={"mix": [["a cat", 0.3], ["a dog", 0.7]]}), dict(prompt=MIXES[1])]
    launches, replies = FPH._serve("test_frame_prompts_host:PromptPipeline", reqs)
    assert launches == [(2, MIXES[0], None, None, None), (1, MIXES[1], None, None, None)], launches
    assert [int(replies[k][0, 0, 1]) for k in range(3)] == [2, 2, 1]


# ------------------------------------------------------------------------------------------ the dispatcher
class _GroupMember:
    """what FrameDispatcher reads of a worker handle in a group, with a `sync_prompt` that records what it was sent"""

    def __init__(self, rank):
        self.group = {"rank": rank, "world": 2}
        self.synced = []
        self.sync_prompt = SimpleNamespace(remote=self._sync)

    def _sync(self, prompt, header=None, collective=True):
        self.synced.append(prompt)
        f = concurrent.futures.Future()
        f.set_result({"via": "group"})
        return f


def test_dispatcher_syncs_the_unknown_component_and_never_the_mix():
    async def go():
        ws = [_GroupMember(0), _GroupMember(1)]
        d = D.FrameDispatcher(ws, depth=4)
        assert d.group_ok
        d._sync_prompt({"prompt": "a known text"})
        assert d.prompt_syncs == 1 and list(d._prompts_known) == ["a known text"]
        d._sync_prompt({"prompt": {"mix": [["an unknown text", 0.4], ["a known text", 0.6]]}})
        assert d.prompt_syncs == 2 and [w.synced for w in ws] == [["a known text", "an unknown text"]] * 2
        assert list(d._prompts_known) == ["a known text", "an unknown text"] and not d._prompts_pending  # (texts only: no key of a mix)
        for wts in ((0.5, 0.5), (0.1, 0.9)):  # a sweep over the two: nothing more
            d._sync_prompt({"prompt": {"mix": [["a known text", wts[0]], ["an unknown text", wts[1]]]}})
        assert d.prompt_syncs == 2
        d._sync_prompt({"prompt": {"mix": [["a known text", 1.0], ["never used", 0.0]]}})  # comes down to the known prompt
        d._sync_prompt({"prompt": {"blend": []}})  # not a mix: the worker refuses the frame, nothing is synced
        assert d.prompt_syncs == 2 and all(len(w.synced) == 2 for w in ws)

    asyncio.run(go())


# ------------------------------------------------------------------------------------------ the example
def test_the_example_writes_a_cross_fade_as_k_mixes():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import frame_loop

    fade = [frame_loop.crossfade("a", "b", k, 4) for k in range(6)]
    assert [PM.canonical(p) for p in fade[:1] + fade[4:]] == ["a", "b", "b"]  # the ends are the plain prompts
    mids = [PM.canonical(p) for p in fade[1:4]]
    assert all(isinstance(m, PM.Mix) and m.texts == ("a", "b") for m in mids) and [m.weights for m in mids] == [(0.75, 0.25), (0.5, 0.5), (0.25, 0.75)]
    assert frame_loop.crossfade("a", "b", 3, 0) == "b"

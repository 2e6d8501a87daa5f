"""Prompt mixes on the GPU (include/vsd.h THE PROMPT MIX): vsd_prompt_mix bit for bit against the numpy restatement that
tests/test_prompt_mix_host.py holds the host twin to, the mixed block of the MINI networks against the block of the mixed embeddings,
the engine's frames (a mix of one, replay, the oracle handed the mixed embeddings, one slot of a per-frame launch, two lanes in flight),
the drop-in class, and a real worker process."""
import functools
import inspect
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prompt_mix_cases as MC  # noqa: E402
import test_frame_prompts_gpu as FP  # noqa: E402
import test_prompt_mix_host as MH  # noqa: E402
from test_ops_gpu import check  # noqa: E402
from test_pipeline_gpu import _frame, _psnr  # noqa: E402

import videosd_amd.engine as E  # noqa: E402
from videosd_amd import blocks as BK  # noqa: E402
from videosd_amd import promptmix as PM  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, STRENGTH, SCALE = FP.STEPS, FP.STRENGTH, FP.SCALE
WEIGHTS = PM.normalized((0.25, 0.75))
# the oracle bounds of test_frame_prompts_gpu._engine_case: taken from its source, so that they cannot drift apart
ORACLE_BOUNDS = "r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0"
R1_MAX, MAD_MAX, PSNR_MIN = 2e-2, 1.5, 38.0
APART = 0.5  # LSB mean: the "really ran with its prompt" margin of test_frame_prompts_gpu.test_the_class_takes_one_prompt_per_frame


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


_mad = FP._mad


# ------------------------------------------------------------------------------------------ the kernel against the restatement
@functools.lru_cache(maxsize=None)
def _problem(n):
    """the segment lists and sources of the host-twin test, and the restatement's result for every destination, computed once"""
    segs, srcs, ws, sbytes, dbytes = MH.mix_problem(n)
    tail = 64
    want = {}
    for f in (0, 2):
        want[f] = MC.mix_numpy(srcs, ws, np.full(dbytes + tail, MC.SENTINEL, np.uint8), segs, f)
    wsegs = MC.whole_segments(segs)
    want["whole"] = MC.mix_numpy(srcs, ws, np.full(sbytes + tail, MC.SENTINEL, np.uint8), wsegs, 0)
    return segs, wsegs, srcs, ws, sbytes, dbytes, tail, want


def _table(ops, segs):
    return ops.to_device(torch.tensor(segs, dtype=torch.int64))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_kernel_against_the_restatement_bit_for_bit(ops, n):
    segs, wsegs, srcs, ws, sbytes, dbytes, tail, want = _problem(n)
    # bounds, before anything runs: every source read and every destination write lies inside its buffer
    assert max(so + rows * rb for so, _do, rows, rb, _p, _f, _k, _r in segs) <= sbytes
    assert max(do + (rows - 1) * p + 3 * fs for _so, do, rows, _rb, p, fs, _k, _r in segs) <= dbytes
    assert max(do + rows * rb for _so, do, rows, rb, _p, _f, _k, _r in wsegs) <= sbytes
    src_d = [ops.to_device(torch.from_numpy(s.copy())) for s in srcs]
    tab, wtab = _table(ops, segs), _table(ops, wsegs)
    for f in (0, 2):  # slots 0 and 2 of B = 3
        dst = ops.to_device(torch.full((dbytes + tail,), MC.SENTINEL, dtype=torch.uint8))
        ops.prompt_mix(src_d, ws, dst, tab, len(segs), f)
        ops.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got, want[f]), (n, f, int((got != want[f]).sum()))  # the other slots, the gaps and the tail: still the sentinel
    dst = ops.to_device(torch.full((sbytes + tail,), MC.SENTINEL, dtype=torch.uint8))
    ops.prompt_mix(src_d, ws, dst, wtab, len(wsegs), 0)  # a whole block of the sources' layout
    ops.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got, want["whole"]), (n, int((got != want["whole"]).sum()))
    if n == 1:  # weight 1 alone is a byte-wise copy
        for so, _do, rows, rb, _p, _f, _k, _r in segs:
            assert np.array_equal(got[so:so + rows * rb], srcs[0][so:so + rows * rb])


def test_kernel_refusals(ops):
    segs, _wsegs, srcs, ws, _sbytes, dbytes, tail, _want = _problem(2)
    src_d = [ops.to_device(torch.from_numpy(s.copy())) for s in srcs]
    tab = _table(ops, segs)
    before = torch.full((dbytes + tail,), MC.SENTINEL, dtype=torch.uint8)
    dst = ops.to_device(before)
    bad = r"vsd_prompt_mix failed \(-1\)"
    for frame in (3, -1):
        with pytest.raises(RuntimeError, match=bad + ".*frame"):
            ops.prompt_mix(src_d, ws, dst, tab, len(segs), frame)
    with pytest.raises(ValueError, match="1..4 components"):
        ops.prompt_mix(src_d * 3, ws * 3, dst, tab, len(segs), 0)
    with pytest.raises(ValueError, match="1..4 components"):
        ops.prompt_mix([], (), dst, tab, len(segs), 0)
    for w in ((-0.5, 1.5), (float("nan"), 1.0), (float("inf"), 0.0)):
        with pytest.raises(RuntimeError, match=bad + ".*weight"):
            ops.prompt_mix(src_d, w, dst, tab, len(segs), 0)
    with pytest.raises(RuntimeError, match=bad + ".*misaligned"):
        ops.prompt_mix([src_d[0], src_d[1][8:]], ws, dst, tab, len(segs), 0)
    with pytest.raises(RuntimeError, match=bad + ".*misaligned"):
        ops.prompt_mix(src_d, ws, dst[8:], tab, len(segs), 0)
    for field in (0, 1, 3, 4, 5):
        off = [list(s) for s in segs]
        off[-1][field] += 8
        with pytest.raises(RuntimeError, match=bad + ".*segment"):
            ops.prompt_mix(src_d, ws, dst, _table(ops, off), len(segs), 0)
    off = [list(s) for s in segs]
    off[0][6] = 3
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*kind"):
        ops.prompt_mix_table(_table(ops, off), len(segs))
    lib, ctx = ops.ctx.lib, ops.ctx.h
    import ctypes as C

    one = (C.c_void_p * 1)(src_d[0].data_ptr())
    w1 = (C.c_float * 1)(1.0)
    for n in (0, 5):  # n outside 1..4, at the C boundary itself
        assert lib.vsd_prompt_mix(ctx, one, w1, n, C.c_void_p(dst.data_ptr()), C.c_void_p(tab.data_ptr()), len(segs), 0, ops.raw_stream(0)) == -1
    assert lib.vsd_prompt_mix(ctx, None, w1, 1, C.c_void_p(dst.data_ptr()), C.c_void_p(tab.data_ptr()), len(segs), 0, ops.raw_stream(0)) == -1
    ops.synchronize()
    assert torch.equal(dst.cpu(), before)  # ... and nothing was written


# ------------------------------------------------------------------------------------------ block level
def test_mixed_block_against_the_block_of_the_mixed_embeddings():
    """MINI networks, tl = 77, weights (0.25, 0.75), the blocks of width >= 128 absorbed so that every item kind is in the block: every
    item of mix(block(A), block(B)) against an fp32 host computation of block(0.25 A + 0.75 B), held to test_ops_gpu.check -- the bound the
    directly built block's ops are held to.  xa2_b is the bias, bit for bit."""
    from videosd_amd import config as C
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps
    from videosd_amd.packing import pack_cross_attention
    from test_pipeline_gpu import _build

    wu, wc, wv, text_a = _build(C.MINI_UNET, C.MINI_CONTROLNET)
    keep = E.XATTN_ABSORB_MIN_C
    E.XATTN_ABSORB_MIN_C = 128
    try:
        eng = Engine(HipOps(0), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    finally:
        E.XATTN_ABSORB_MIN_C = keep
    text_b = (torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(8)) * 0.5).half()
    a, b = eng.build_prompt(text_a), eng.build_prompt(text_b)
    lay = a.layout
    assert lay is b.layout and lay.absorbed and {k[2] for k in lay.items} == set(BK.MIX_ITEM_KINDS)
    dst = BK.PromptBlock(eng.ops, lay)
    tab, nseg = eng._seg_table(lay, lay, mix=True)
    eng.ops.prompt_mix([a.buf, b.buf], WEIGHTS, dst.buf, tab, nseg, 0)
    eng.ops.synchronize()
    e_mix = WEIGHTS[0] * text_a.float() + WEIGHTS[1] * text_b.float()
    for ni, net in enumerate(eng._nets()):
        for bi, t in enumerate(net.transformers):
            c = t.kv2.n // 2
            wkv = t.kv2.weight[:, :t.kv2.k].float().cpu()
            k, v = e_mix @ wkv[:c].t(), e_mix @ wkv[c:].t()
            check(dst.view(ni, bi, "k"), k, f"K net {ni} block {bi}")
            vt = dst.view(ni, bi, "vt").cpu()
            check(vt[:, :77], v.t(), f"V^T net {ni} block {bi}")
            assert not vt[:, 77:].any()  # the key padding is still zero
            if (ni, bi) not in lay.absorbed:
                continue
            wq, ga, be = (x.cpu() for x in t.xa_raw)
            heads = net.cfg.heads_for(c)
            x1, x2 = pack_cross_attention(k, v, wq[:, :c], t.out2.weight[:, :c].cpu(), t.out2.bias.cpu(), ga, be, heads)
            check(dst.view(ni, bi, "xa1_w"), x1.weight[:, :c], f"xa1_w net {ni} block {bi}")
            check(dst.view(ni, bi, "xa1_s"), x1.ln_s, f"xa1_s net {ni} block {bi}")
            check(dst.view(ni, bi, "xa1_t"), x1.ln_t, f"xa1_t net {ni} block {bi}")
            check(dst.view(ni, bi, "xa2_w"), x2.weight[:, :heads * 128], f"xa2_w net {ni} block {bi}")
            assert torch.equal(dst.view(ni, bi, "xa2_b").cpu(), t.out2.bias.cpu())  # copied from component 0 = the bias itself
            assert torch.equal(a.view(ni, bi, "xa2_b"), b.view(ni, bi, "xa2_b"))


# ------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def mini():
    """the MINI engine and oracle of the per-frame prompt tests; text B with twice the spread of text A, so that the oracle's pictures of
    A, B and the mix (0.25, 0.75) lie 2.5 to 6 LSB apart at both sizes (measured on the CPU; with the spread of A they lie 0.8 apart)"""
    from videosd_amd import config as C

    eng, orc, (text_a, _t2), (blk_a, _b2) = FP._setup(C.MINI_UNET, C.MINI_CONTROLNET)
    text_b = torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(8)).half()
    return eng, orc, (text_a, text_b), (blk_a, eng.build_prompt(text_b))


def _oracle(orc, frame, embeds, H, W):
    img = np.asarray(orc.infer(Image.fromarray(frame, "RGB"), embeds[None].float(), height=H, width=W, strength=STRENGTH, steps=STEPS, seed=23,
                               controlnet_scale=SCALE, use_controlnet=True, keep_trace=True))
    return img, orc.trace["denoised"][-1][0]


@pytest.mark.parametrize("H,W", [(120, 72), (128, 128)])
def test_engine_frames_of_a_mix(mini, H, W):
    assert ORACLE_BOUNDS in inspect.getsource(FP._engine_case)
    eng, orc, texts, (a, b) = mini
    B = 3
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)])
    prep = dict(controlnet_scale=SCALE, use_controlnet=True, batch=B, autotune=False)
    mix = BK.PromptMix([a, b], WEIGHTS)
    eng.use_prompt(a)
    eng.prepare(H, W, STEPS, STRENGTH, **prep)
    only = {}
    for name, blk in (("a", a), ("b", b)):
        eng.use_prompt(blk)
        only[name] = eng.infer_u8(frames)
    # (a) a mix of one component: the plain prompt's frames, bit for bit
    eng.use_prompt(BK.PromptMix([a], (1.0,)))
    assert np.array_equal(eng.infer_u8(frames), only["a"])
    # (b) two components: deterministic replay, the oracle handed the mixed EMBEDDINGS, and neither component's picture
    eng.use_prompt(mix)
    got = eng.infer_u8(frames)
    h0, w0 = H // 8, W // 8
    den = eng.buffers["denoised"][:, :4].float().cpu().reshape(B, h0, w0, 4).permute(0, 3, 1, 2)
    assert np.array_equal(got, eng.infer_u8(frames))
    eng.use_prompt(b)
    eng.infer_u8(frames)
    eng.use_prompt(BK.PromptMix([a, b], WEIGHTS))
    assert np.array_equal(got, eng.infer_u8(frames))  # formed again after another prompt: the same bits
    e_mix = WEIGHTS[0] * texts[0].float() + WEIGHTS[1] * texts[1].float()
    for i in range(B):
        ref, ref_den = _oracle(orc, frames[i], e_mix, H, W)
        r1 = float((den[i] - ref_den).norm() / ref_den.norm())
        mad, psnr = _mad(got[i], ref), _psnr(got[i], ref)
        da, db = _mad(got[i], only["a"][i]), _mad(got[i], only["b"][i])
        print(f"{W}x{H} frame {i} mix: r1 {r1:.3g} mad {mad:.3f} psnr {psnr:.1f}; from A alone {da:.2f}, from B alone {db:.2f} LSB")
        assert r1 <= R1_MAX and mad <= MAD_MAX and psnr >= PSNR_MIN, (i, r1, mad, psnr)
        assert da > APART and db > APART, (i, da, db)
    # (c) a per-frame engine with [A, mix, B]: frames 0 and 2 of [A, A, B], frame 1 of [mix, mix, mix], bit for bit
    eng.use_prompts([a, mix, b])
    plan = eng.prepare(H, W, STEPS, STRENGTH, frame_prompts=True, **prep)
    assert plan["frame_prompts"] is True
    amb = eng.infer_u8(frames)
    assert np.array_equal(amb, eng.infer_u8(frames))
    eng.use_prompts([a, a, b])
    aab = eng.infer_u8(frames)
    eng.use_prompts([mix, mix, mix])
    mmm = eng.infer_u8(frames)
    assert np.array_equal(amb[0], aab[0]) and np.array_equal(amb[2], aab[2]) and np.array_equal(amb[1], mmm[1])
    assert _mad(amb[1], aab[1]) > APART  # (slot 1 really held the mix)
    for i in range(B):  # the explicit form against the default program with the same mix: the existing bound between the two programs
        assert _mad(mmm[i], got[i]) < 0.5, (i, _mad(mmm[i], got[i]))


def test_two_lanes_in_flight_with_different_mixes(mini):
    eng, _orc, _texts, (a, b) = mini
    H = W = 128
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)])
    prep = dict(controlnet_scale=SCALE, use_controlnet=True, batch=3, autotune=False)
    mixes = [BK.PromptMix([a, b], PM.normalized(w)) for w in ((0.25, 0.75), (0.75, 0.25), (0.5, 0.5), (0.1, 0.9))]
    eng.use_prompt(mixes[0])
    eng.prepare(H, W, STEPS, STRENGTH, **prep)
    slot = eng.make_slot(lane=1)
    slot.use_prompt(mixes[1])
    slot.prepare(H, W, STEPS, STRENGTH, **prep)
    engines = [eng, slot]
    rounds = [(mixes[0], mixes[1]), (mixes[2], mixes[3])]  # (the second round re-forms the block of both engines)
    seq = []
    for pair in rounds:
        for e, m in zip(engines, pair):
            e.use_prompt(m)
            seq.append(e.infer_u8(frames))
    assert not np.array_equal(seq[0], seq[1])
    outs = []
    for pair in rounds:
        for e, m in zip(engines, pair):
            e.use_prompt(m)
            e.submit_u8(frames)  # both launches are now in flight on their lanes' streams
        for e in engines:
            outs.append(e.collect_u8())
    for got, ref in zip(outs, seq):
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------ the drop-in class
TEXT_A, TEXT_B = "a watercolor painting", "a charcoal sketch"
OPTS = dict(height=96, width=160, strength=STRENGTH, steps=STEPS, controlnet_scale=SCALE)


def _mix(wa, wb):
    return {"mix": [[TEXT_A, wa], [TEXT_B, wb]]}


def test_the_class_takes_a_mix(monkeypatch, tmp_path):
    img = Image.fromarray(_frame(96, 160, seed=3), "RGB")
    p = FP._pipeline(monkeypatch)
    only_a = np.asarray(p.infer(img, prompt=TEXT_A, **OPTS))
    only_b = np.asarray(p.infer(img, prompt=TEXT_B, **OPTS))
    builds = p.metrics()["stage_ms_p50"]["prompt_builds"]
    assert builds == 2 and list(p._prompts) == [TEXT_A, TEXT_B]
    mid = np.asarray(p.infer(img, prompt=_mix(0.5, 0.5), **OPTS))
    assert _mad(mid, only_a) > APART and _mad(mid, only_b) > APART
    assert np.array_equal(mid, np.asarray(p.infer(img, prompt={"mix": [[TEXT_B, 2], [TEXT_A, 1], [TEXT_A, 1]]}, **OPTS)))  # another spelling
    assert np.array_equal(only_a, np.asarray(p.infer(img, prompt=_mix(1.0, 0.0), **OPTS)))  # comes down to the plain prompt
    for i in range(20):  # a sweep: a new mix value on every launch
        p.infer(img, prompt=_mix(1.0 - (i + 0.5) / 20, (i + 0.5) / 20), **OPTS)
    m = p.metrics()["stage_ms_p50"]
    assert sorted(p._prompts) == sorted([TEXT_A, TEXT_B]) and m["prompts_cached"] == 2 and m["prompt_builds"] == builds
    assert len(p._plans) == 1 and len(p._engines) == 1  # one program, one engine: nothing was prepared or captured for a mix
    with pytest.raises(ValueError, match="export_plan: `prompt` is a mix"):
        p.export_plan(str(tmp_path / "x.vsdplan"), prompt=_mix(0.5, 0.5), **OPTS)
    with pytest.raises(ValueError, match="at most 4 components"):
        p.infer(img, prompt={"mix": [[t, 1] for t in "abcde"]}, **OPTS)
    monkeypatch.setattr(p, "is_xl", True)  # (phase 1 refuses before anything looks at the model)
    with pytest.raises(ValueError, match="SDXL program has the pooled text embedding"):
        p.infer(img, prompt=_mix(0.5, 0.5), **OPTS)
    del p
    # a mix inside `prompts` of a per-frame pipeline: each frame within the bound of a launch of two against a launch of one
    q = FP._pipeline(monkeypatch, frame_prompts=True)
    imgs = [Image.fromarray(_frame(96, 160, seed=s), "RGB") for s in (3, 4)]
    mix = _mix(0.25, 0.75)
    outs = [np.asarray(o) for o in q.infer_batch(imgs, prompts=[TEXT_A, mix], **OPTS)]
    singles = [np.asarray(q.infer(imgs[0], prompt=TEXT_A, **OPTS)), np.asarray(q.infer(imgs[1], prompt=mix, **OPTS))]
    for o, s in zip(outs, singles):
        assert _mad(o, s) < 0.5, _mad(o, s)
    assert _mad(outs[1], np.asarray(q.infer(imgs[1], prompt=TEXT_B, **OPTS))) > APART  # the second frame really ran with the mix
    assert sorted(q._prompts) == sorted([TEXT_A, TEXT_B])


def test_a_real_worker_serves_queued_mixes_in_order(monkeypatch):
    from videosd_amd.dispatch import RemotePipeline

    cfg = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table")
    imgs = [Image.fromarray(_frame(96, 160, seed=s), "RGB") for s in (5, 6, 7)]
    mixes = [_mix(0.25, 0.75), _mix(0.5, 0.5), _mix(0.9, 0.1)]
    p = FP._pipeline(monkeypatch)
    want = [np.asarray(p.infer(im, prompt=m, **OPTS)) for im, m in zip(imgs, mixes)]
    assert not np.array_equal(want[0], np.asarray(p.infer(imgs[0], prompt=mixes[1], **OPTS)))
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    w = RemotePipeline(factory="prompt_mix_cases:mini_pipeline", **cfg)
    try:
        futs = [w.infer.remote(im, prompt=m, **OPTS) for im, m in zip(imgs, mixes)]  # all queued before the first is answered
        got = [np.asarray(f.result(timeout=300)) for f in futs]
    finally:
        w.close()
    for g, r in zip(got, want):
        assert np.array_equal(g, r)

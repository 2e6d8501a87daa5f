"""Per-frame prompts on the GPU: `vsd_prompt_install` byte for byte against a torch scatter, the cross-attention of a `frame_prompts`
program (image b on its own key rows / V^T columns, text length 77 in 128-column slots) against the fp64 reference of
tests/test_attention_forms_gpu.py, the engine's frames against uniform launches, the oracle and the default program, the drop-in class,
and two lanes in flight with different prompt lists."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_prompt_cases as FC  # noqa: E402
from test_attention_forms_gpu import PAD, SENTINEL, check_kinds, make_problem, reference  # noqa: E402  (check_kinds: the rel = 3e-3 bound)
from test_pipeline_gpu import _build, _cpu, _frame, _psnr  # noqa: E402

import videosd_amd.engine as E  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS, STRENGTH, SCALE = 2, 0.6, 1.5


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _mad(a, b):
    return float(np.abs(a.astype(int) - b.astype(int)).mean())


# ------------------------------------------------------------------------------------------ vsd_prompt_install
def _scatter(src_lay, dst_lay, src, dst_before, frame):
    """the per-frame block after installing `src` into slot `frame`, by torch indexing of the layouts' tensors"""
    want = dst_before.clone()
    tl, ldt = dst_lay.tl, dst_lay.ldt
    for key, (doff, dshape, _dt) in dst_lay.items.items():
        soff, sshape, _st = src_lay.items[key]
        s = src[soff:soff + sshape[0] * sshape[1] * 2].view(torch.int16).view(*sshape)
        d = want[doff:doff + dshape[0] * dshape[1] * 2].view(torch.int16).view(*dshape)
        if key[2] == "k":
            d[frame * tl:(frame + 1) * tl] = s
        else:
            d[:, frame * ldt:(frame + 1) * ldt] = s
    return want


@pytest.mark.parametrize("tl", [77, 8])
@pytest.mark.parametrize("frames", [1, 2, 5])
def test_prompt_install_byte_for_byte(ops, frames, tl):
    nets = FC.stub_nets((320, 1280))
    src_lay, dst_lay = E.PromptLayout(nets, tl), E.FramePromptLayout(nets, tl, frames)
    segs = E.prompt_segments(src_lay, dst_lay)
    assert max(do + (rows - 1) * pitch + frames * fs for _so, do, rows, _rb, pitch, fs in segs) <= dst_lay.nbytes  # (bounds, before anything runs)
    assert max(so + rows * rb for so, _do, rows, rb, _p, _f in segs) <= src_lay.nbytes
    tab = ops.to_device(torch.tensor(segs, dtype=torch.int64))
    g = torch.Generator().manual_seed(100 * frames + tl)
    src = torch.randint(0, 256, (src_lay.nbytes,), generator=g, dtype=torch.uint8)
    src_d = ops.to_device(src)
    before = torch.full((dst_lay.nbytes,), FC.SENTINEL, dtype=torch.uint8)
    for f in range(frames):
        dst_d = ops.to_device(before)
        ops.prompt_install(src_d, dst_d, tab, len(segs), f)
        ops.synchronize()
        got = dst_d.cpu()
        assert torch.equal(got, _scatter(src_lay, dst_lay, src, before, f)), (frames, tl, f)
        copied = sum(rows * rb for _so, _do, rows, rb, _p, _f in segs)
        assert int((got == FC.SENTINEL).sum()) >= dst_lay.nbytes - copied  # the sentinel survives everywhere else
    # refused before anything is launched: a frame slot the destination does not have, misaligned blocks, a table with a misaligned field
    dst_d = ops.to_device(before)
    for bad in (frames, -1):
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*frame"):
            ops.prompt_install(src_d, dst_d, tab, len(segs), bad)
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        ops.prompt_install(src_d[8:], dst_d, tab, len(segs), 0)
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        ops.prompt_install(src_d, dst_d[8:], tab, len(segs), 0)
    for field in (0, 1, 3, 4, 5):
        off = [list(s) for s in segs]
        off[-1][field] += 8
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*segment"):
            ops.prompt_install(src_d, dst_d, ops.to_device(torch.tensor(off, dtype=torch.int64)), len(segs), 0)
    ops.synchronize()
    assert torch.equal(dst_d.cpu(), before)  # ... and nothing was written
    ops.prompt_install(src_d, dst_d, tab, len(segs), frames - 1)  # the table is still good
    ops.synchronize()
    assert torch.equal(dst_d.cpu(), _scatter(src_lay, dst_lay, src, before, frames - 1))


# ------------------------------------------------------------------------------------------ cross-attention in the recorded form
@pytest.mark.parametrize("heads,d", [(8, 40), (8, 80), (8, 160)])
@pytest.mark.parametrize("sq", [1, 16, 117])
def test_cross_attention_in_the_recorded_form(ops, sq, heads, d):
    """what `Engine._cross_attention` records for a per-frame block: K [B*77][c] with k_batch_rows = 77 (no gap between the images), V^T
    [c][B*128] with vt_batch_cols = 128 and finite garbage in every slot's columns beyond key 77"""
    B, sk, ldt = 3, 77, 128
    c = heads * d
    q, k, v, kinds = make_problem(sq, sk, heads, d, B, seed=sq + d)
    vt = torch.full((c, B * ldt), PAD, dtype=torch.float16)
    for b in range(B):
        vt[:, b * ldt:b * ldt + sk] = v[b * sk:(b + 1) * sk].t()
    out = torch.full((B * sq + 3, c), SENTINEL, dtype=torch.float16, device=DEV)
    ops.attention(q.to(DEV), c, k.to(DEV), c, vt.to(DEV), B * ldt, out, c, sq, sk, heads, d, d ** -0.5, batch=B, k_brows=sk, vt_bcols=ldt)
    ops.synchronize()
    ref = torch.cat([reference(q[b * sq:(b + 1) * sq], k[b * sk:(b + 1) * sk], v[b * sk:(b + 1) * sk], heads) for b in range(B)])
    check_kinds(out[:B * sq], ref, kinds, heads, d, f"cross-attention sq={sq} d={d}")
    assert bool((out[B * sq:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------ the engine
def _setup(unet_cfg, cn_cfg):
    from oracle.pipeline import OraclePipeline
    from videosd_amd import config as C
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu, wc, wv, text = _build(unet_cfg, cn_cfg)
    eng = Engine(HipOps(0), unet_cfg, cn_cfg, C.TAESD, wu, wc, wv)
    text2 = (torch.randn(77, unet_cfg.cross_dim, generator=torch.Generator().manual_seed(8)) * 0.5).half()
    eng.set_text_embeds(text)
    orc = OraclePipeline(unet_cfg, cn_cfg, _cpu(wu), _cpu(wc), _cpu(wv))
    return eng, orc, (text, text2), (eng.build_prompt(text), eng.build_prompt(text2))


@pytest.fixture(scope="module")
def mini():
    from videosd_amd import config as C

    return _setup(C.MINI_UNET, C.MINI_CONTROLNET)


def _engine_case(setup, H, W, idx):
    """frames of a launch with prompts `idx`: deterministic, bit for bit the frames of uniform launches, at the oracle's bounds with their
    own prompt, within 0.5 LSB mean of the default program with that prompt"""
    eng, orc, texts, blocks = setup
    B = len(idx)
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)[:B]])
    prep = dict(controlnet_scale=SCALE, use_controlnet=True, batch=B, autotune=False)
    default = []
    eng.use_prompt(blocks[0])
    eng.prepare(H, W, STEPS, STRENGTH, **prep)
    for blk in blocks:
        eng.use_prompt(blk)
        default.append(eng.infer_u8(frames))
    eng.use_prompts([blocks[i] for i in idx])
    plan = eng.prepare(H, W, STEPS, STRENGTH, frame_prompts=True, **prep)
    assert plan["frame_prompts"] is True
    got = eng.infer_u8(frames)
    assert np.array_equal(got, eng.infer_u8(frames))  # deterministic replay
    h0, w0 = H // 8, W // 8
    den = eng.buffers["denoised"][:, :4].float().cpu().reshape(B, h0, w0, 4).permute(0, 3, 1, 2)
    uniform = []
    for blk in blocks:
        eng.use_prompts([blk] * B)
        uniform.append(eng.infer_u8(frames))
    for b, pi in enumerate(idx):
        assert np.array_equal(got[b], uniform[pi][b]), (b, _mad(got[b], uniform[pi][b]))
        assert not np.array_equal(uniform[0][b], uniform[1][b])
        ref = np.asarray(orc.infer(Image.fromarray(frames[b], "RGB"), texts[pi][None].float(), height=H, width=W, strength=STRENGTH,
                                   steps=STEPS, seed=23, controlnet_scale=SCALE, use_controlnet=True, keep_trace=True))
        ref_den = orc.trace["denoised"][-1][0]
        r1 = float((den[b] - ref_den).norm() / ref_den.norm())
        mad, psnr, d_def = _mad(got[b], ref), _psnr(got[b], ref), _mad(got[b], default[pi][b])
        print(f"{W}x{H} frame {b} prompt {pi}: r1 {r1:.3g} mad {mad:.3f} psnr {psnr:.1f} vs default program {d_def:.3f} LSB")
        assert r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0, (b, r1, mad, psnr)
        assert d_def < 0.5, (b, d_def)
    return frames, got, uniform


@pytest.mark.parametrize("H,W", [(120, 72), (128, 128)])
def test_mini_engine_frames_follow_their_own_prompts(mini, H, W):
    _engine_case(mini, H, W, [0, 1, 0])


def test_sd15_widths_frames_follow_their_own_prompts():
    """head dims 40 / 80 / 160, the fused tail at C = 320, 64 / 16 / 4 / 1 tokens per image"""
    from videosd_amd import config as C

    _engine_case(_setup(C.SD15_UNET, C.SD15_CONTROLNET), 64, 64, [0, 1])


def test_two_lanes_in_flight_with_different_prompt_lists(mini):
    eng, _orc, _texts, blocks = mini
    H = W = 128
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)])
    prep = dict(controlnet_scale=SCALE, use_controlnet=True, batch=3, autotune=False, frame_prompts=True)
    eng.use_prompts([blocks[0], blocks[1], blocks[0]])
    eng.prepare(H, W, STEPS, STRENGTH, **prep)
    slot = eng.make_slot(lane=1)
    slot.use_prompts([blocks[1], blocks[1], blocks[0]])
    slot.prepare(H, W, STEPS, STRENGTH, **prep)
    engines = [eng, slot]
    lists = [([0, 1, 0], [1, 1, 0]), ([1, 0, 0], [0, 0, 1])]  # (the second round rewrites slots of both engines)
    seq = []
    for la, lb in lists:
        for e, l in zip(engines, (la, lb)):
            e.use_prompts([blocks[i] for i in l])
            seq.append(e.infer_u8(frames))
    assert not np.array_equal(seq[0], seq[1])
    outs = []
    for la, lb in lists:
        for e, l in zip(engines, (la, lb)):
            e.use_prompts([blocks[i] for i in l])
            e.submit_u8(frames)  # both launches are now in flight on their lanes' streams
        for e in engines:
            outs.append(e.collect_u8())
    for got, ref in zip(outs, seq):
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------ the drop-in class
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


def test_the_class_takes_one_prompt_per_frame(monkeypatch, tmp_path):
    H, W = 96, 160
    opts = dict(height=H, width=W, strength=STRENGTH, steps=STEPS, controlnet_scale=SCALE)
    imgs = [Image.fromarray(_frame(H, W, seed=s), "RGB") for s in (3, 4)]
    a, b = "a watercolor painting", ["a charcoal sketch"]
    p = _pipeline(monkeypatch, frame_prompts=True)
    assert p.per_frame_prompt is True and p.per_frame_seed is False
    outs = [np.asarray(o) for o in p.infer_batch(imgs, prompts=[a, b], **opts)]
    singles = [np.asarray(p.infer(imgs[0], prompt=a, **opts)), np.asarray(p.infer(imgs[1], prompt=b, **opts))]
    for o, s in zip(outs, singles):
        assert _mad(o, s) < 0.5, _mad(o, s)
    assert _mad(outs[1], np.asarray(p.infer(imgs[1], prompt=a, **opts))) > 0.5  # the second frame really ran with ITS prompt
    assert all(e.plan["frame_prompts"] for e in p._engines.values()) and len(p._plans) == 1
    # `prompt` keeps its meaning: every frame that prompt
    same = [np.asarray(o) for o in p.infer_batch(imgs, prompt=a, **opts)]
    assert _mad(same[0], singles[0]) < 0.5 and np.array_equal(same[0], np.asarray(p.infer_batch(imgs, prompts=[a, a], **opts)[0]))
    with pytest.raises(ValueError, match="one prompt per frame"):
        p.infer_batch(imgs, prompts=[a], **opts)
    with pytest.raises(ValueError, match="frame_prompts=True"):
        p.export_plan(str(tmp_path / "x.vsdplan"), **opts)
    # more prompts than the cache holds, all of them in one launch: none is dropped while the launch needs it
    p.max_prompts = 1
    handle = p.submit_batch(imgs, prompts=["x", "y"], **opts)
    assert {"x", "y"} <= set(p._prompts) and len(handle.keep) == 2
    p.collect_batch(handle)
    del p
    # seeds and prompts per frame together
    q = _pipeline(monkeypatch, frame_prompts=True, device_seed=True)
    assert q.per_frame_prompt is True and q.per_frame_seed is True
    outs = [np.asarray(o) for o in q.infer_batch([imgs[0]] * 2, prompts=[a, b], seed=[1, 2], **opts)]
    singles = [np.asarray(q.infer(imgs[0], prompt=a, seed=1, **opts)), np.asarray(q.infer(imgs[0], prompt=b, seed=2, **opts))]
    for o, s in zip(outs, singles):
        assert _mad(o, s) < 0.5, _mad(o, s)
    assert _mad(outs[0], np.asarray(q.infer(imgs[0], prompt=a, seed=2, **opts))) > 0.5  # the seed counts ...
    assert _mad(outs[0], np.asarray(q.infer(imgs[0], prompt=b, seed=1, **opts))) > 0.5  # ... and so does the prompt
    del q
    # the unchanged default
    r = _pipeline(monkeypatch)
    assert r.per_frame_prompt is False
    with pytest.raises(ValueError, match="frame_prompts=True"):
        r.infer_batch(imgs, prompts=[a, b], **opts)
    r.infer_batch(imgs, prompt=a, **opts)
    assert not any(e.plan["frame_prompts"] for e in r._engines.values())

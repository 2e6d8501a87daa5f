"""Colour match on the MI355X (csrc/color_match.hip) against the host twin vsd_color_match_host, which tests/test_color_match_host.py
holds to the numpy restatement of THE COLOUR CONTRACT (include/vsd.h): every byte of every frame of every case of
tests/color_match_cases.py, both modes, every amount, with the operands at odd byte offsets inside larger buffers whose other bytes
must stay as they were; determinism; the engine (eager, replayed, a new amount between two launches, I420 output); the drop-in class.

Shapes: see tests/color_match_cases.py (smaller than a vector, than a workgroup's threads, one / two / thirteen workgroups per frame,
1 / 3 / 5 frames per call, a side at the maximum)."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import color_match_cases as CM  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN_FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "default_frames_mini_64x64_before_color_match.npy")
CANARY = 0xC3
PAD = 48  # canary bytes either side of an operand


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def twin(src, dst, mode, a):
    """vsd_color_match_host on one [h][w][3] frame pair -> the new dst"""
    from videosd_amd import lib as L

    src = np.ascontiguousarray(src, dtype=np.uint8)
    out = np.array(dst, dtype=np.uint8)
    h, w = src.shape[:2]
    assert L.load().vsd_color_match_host(src.ctypes.data, out.ctypes.data, h, w, CM.MODES[mode], int(a)) == 0
    return out


def twin_frames(src, dst, mode, amounts):
    return np.stack([twin(s, d, mode, a) for s, d, a in zip(src, dst, amounts)])


def _placed(arr, skew):
    """the bytes of `arr` `skew` bytes past a 16-byte boundary inside a buffer of canaries -> (holder, view of the operand)"""
    n = arr.size
    holder = torch.full((PAD + 16 + n + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + ((-(holder.data_ptr() + PAD)) % 16) + skew
    view = holder[start:start + n]
    assert view.data_ptr() % 16 == skew % 16
    view.copy_(torch.from_numpy(np.array(arr, dtype=np.uint8)).reshape(-1))  # (a copy: the shared cases are read-only)
    return holder, view, start


def _canaries_intact(holder, start, n):
    h = holder.cpu().numpy()
    return bool((h[:start] == CANARY).all() and (h[start + n:] == CANARY).all())


def run_device(ops, src, dst, mode, amounts, skew_src=0, skew_dst=0):
    """ops.color_match on operands placed at the given skews -> the new dst [frames][h][w][3]; src and all canaries checked"""
    frames, h, w = src.shape[:3]
    hs, vs, ss = _placed(src, skew_src)
    hd, vd, sd = _placed(dst, skew_dst)
    am = torch.tensor(list(amounts), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the operands were placed on torch's stream; the op runs on its own)
    ops.color_match(vs, vd, frames, h, w, mode, am)
    ops.synchronize()
    assert _canaries_intact(hs, ss, src.size) and _canaries_intact(hd, sd, dst.size), "bytes outside the operands were written"
    assert np.array_equal(vs.cpu().numpy(), src.reshape(-1)), "src was written"
    return vd.cpu().numpy().reshape(dst.shape)


# ------------------------------------------------------------------------------------------ 1. device against host
@pytest.mark.parametrize("mode", list(CM.MODES))
@pytest.mark.parametrize("name", CM.NAMES)
def test_device_equals_host(ops, name, mode):
    src, dst = CM.case(name)
    k = CM.NAMES.index(name)
    for j, amounts in enumerate(CM.amount_lists(len(src))):
        skews = ((5 * k + 3 * j + 1) % 16, (11 * k + 7 * j + 2) % 16)  # (odd offsets, other ones for src and dst, every residue over the cases)
        want = twin_frames(src, dst, mode, amounts)
        got = run_device(ops, src, dst, mode, amounts, *skews)
        assert np.array_equal(got, want), (name, mode, amounts, skews, int((got != want).sum()), "bytes differ")
        if set(amounts) == {0}:
            assert np.array_equal(got, dst)


@pytest.mark.parametrize("skew", range(16))
def test_device_equals_host_at_every_alignment(ops, skew):
    for name in ("5x7x3-random", "72x120x3-two_valued"):
        src, dst = CM.case(name)
        amounts = CM.FRAME_AMOUNTS[:len(src)]
        for mode in CM.MODES:
            want = twin_frames(src, dst, mode, amounts)
            assert np.array_equal(run_device(ops, src, dst, mode, amounts, skew, (skew * 7 + 5) % 16), want), (name, mode, skew)
            assert np.array_equal(run_device(ops, src, dst, mode, amounts, (skew * 3 + 1) % 16, skew), want), (name, mode, skew)


def test_amounts_outside_the_range_are_clamped_and_bad_arguments_refused(ops):
    src, dst = CM.case("64x64x3-random")
    got = run_device(ops, src, dst, "histogram", (-7, 300, 1 << 20))
    assert np.array_equal(got, twin_frames(src, dst, "histogram", (0, 256, 256)))
    f = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    am = torch.zeros(4, dtype=torch.int32, device="cuda")
    for frames, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 16385), (1, 4096, 4096)):
        with pytest.raises(RuntimeError, match="color_match"):
            ops.color_match(f, f, frames, h, w, "histogram", am)
    with pytest.raises(KeyError):
        ops.color_match(f, f, 1, 8, 8, "lab", am)


# ------------------------------------------------------------------------------------------ 2. determinism
def test_the_same_call_twice_gives_the_same_bytes(ops):
    for name in ("72x120x5-random", "264x256x1-src255"):
        src, dst = CM.case(name)
        amounts = CM.FRAME_AMOUNTS[:len(src)]
        for mode in CM.MODES:
            a = run_device(ops, src, dst, mode, amounts, 3, 9)
            ops.workspace("color_match", 1).fill_(0x5A)  # (whatever the workspace held: every word the later launches read is written first)
            torch.cuda.synchronize()
            b = run_device(ops, src, dst, mode, amounts, 3, 9)
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ 3. the engine
H, W, STEPS, B = 64, 64, 2, 3


@pytest.fixture(scope="module")
def engine():
    from videosd_amd import config as C
    from videosd_amd import weights as Wt
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu = Wt.synthesize(Wt.unet_spec(C.MINI_UNET), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(C.MINI_CONTROLNET), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(C.TAESD), "vae.", device="cuda")
    eng = Engine(HipOps(0), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def _frames():
    rng = np.random.default_rng(11)
    ramp = np.linspace(0, 255, W, dtype=np.float64)[None, :, None]
    tints = np.array([[1.0, 0.6, 0.3], [0.3, 1.0, 0.7], [0.8, 0.8, 0.2]])
    return np.stack([np.clip(ramp * tints[b][None, None, :] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8) for b in range(B)])


PREP = dict(controlnet_scale=1.5, use_controlnet=True, batch=B, autotune=False)


@pytest.fixture(scope="module")
def plain(engine):
    """what the default program makes of the frames (its call list too): the operand the colour-match engine's output is derived from"""
    frames = _frames()
    plan = engine.prepare(H, W, STEPS, 0.6, use_graph=True, **PREP)
    assert plan["color_match"] is None and engine.color_amounts is None
    out = engine.infer_u8(frames).copy()
    assert np.array_equal(engine.frame_u8.cpu().numpy(), frames)
    # ... and they are the frames of the commit before the stage existed: out_u8 of this very engine (MINI networks, 64 x 64, 2 steps, 3
    # frames per launch, autotune=False: the deterministic kernel choice), recorded on an MI355X from that commit's own sources and library
    assert np.array_equal(out, np.load(GOLDEN_FRAMES)), "the default engine's frames are not the parent commit's"
    names = [fn.__name__ for fn, _a, _k in engine.flat_calls(engine.program.calls)]
    assert "color_match" not in names
    return frames, out, names


@pytest.mark.parametrize("mode", list(CM.MODES))
def test_engine_output_is_the_twin_of_frame_and_default_output(engine, plain, mode):
    """out_u8 of the colour-match engine = the host twin applied to (frame_u8, out_u8 of the default engine), byte for byte: replayed and
    eager; a `set_color_amount` between two launches moves the second launch to the twin at the new amounts without a new capture; the
    I420 output is the conversion of the matched RGB; at amount 0 the frames are the default engine's, which the `plain` fixture holds to
    the frames recorded on the parent commit (the rest of the program is the default program, call for call)."""
    from videosd_amd import lib as L

    frames, base, plain_names = plain
    want = twin_frames(frames, base, mode, (256,) * B)
    assert not np.array_equal(want, base)
    plan = engine.prepare(H, W, STEPS, 0.6, use_graph=True, color_match=mode, **PREP)
    assert plan["color_match"] == mode and engine.graph is not None
    names = [fn.__name__ for fn, _a, _k in engine.flat_calls(engine.program.calls)]
    i = names.index("color_match")
    assert names[i - 1] == "postprocess_rgb" and names[:i] + names[i + 1:] == plain_names
    got = engine.infer_u8(frames)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(engine.infer_u8(frames), want)  # replay is deterministic
    # a new amount per frame between two launches: the same graph objects, the twin's bytes at the new amounts
    graph, graph_serial, program = engine.graph, engine.graph_serial, engine.program
    engine.set_color_amount([0.0, 0.5, 77 / 256])
    got = engine.infer_u8(frames)
    assert engine.graph is graph and engine.graph_serial is graph_serial and engine.program is program
    assert np.array_equal(got, twin_frames(frames, base, mode, (0, 128, 77)))
    assert np.array_equal(got[0], base[0])
    engine.set_color_amount(0.0)
    assert np.array_equal(engine.infer_u8(frames), base)  # amount 0: the default engine's frames
    # I420 output: the conversion queued behind the program reads the matched frame
    engine.set_color_amount(1.0)
    engine.submit_u8(frames)
    yuv = engine.collect_i420()
    lib = L.load()
    for b in range(B):
        y, u, v = np.empty((H, W), np.uint8), np.empty((H // 2, W // 2), np.uint8), np.empty((H // 2, W // 2), np.uint8)
        rgb = np.ascontiguousarray(want[b])
        assert lib.vsd_rgb_to_i420_host(rgb.ctypes.data, H, W, y.ctypes.data, u.ctypes.data, v.ctypes.data, W, W // 2) == 0
        assert np.array_equal(yuv[b].y, y) and np.array_equal(yuv[b].u, u) and np.array_equal(yuv[b].v, v), b
    # eager equals replay
    engine.prepare(H, W, STEPS, 0.6, use_graph=False, color_match=mode, color_amount=0.5, **PREP)
    assert engine.graph is None and engine.color_a == (128,) * B
    assert np.array_equal(engine.infer_u8(frames), twin_frames(frames, base, mode, (128,) * B))


def test_a_slot_has_amounts_of_its_own(engine, plain):
    frames, base, _names = plain
    engine.prepare(H, W, STEPS, 0.6, use_graph=True, color_match="meanstd", color_amount=1.0, **PREP)
    slot = engine.make_slot()
    slot.prepare(H, W, STEPS, 0.6, use_graph=True, color_match="meanstd", color_amount=0.25, **PREP)
    assert slot.color_amounts.data_ptr() != engine.color_amounts.data_ptr()
    for e in (engine, slot):
        e.submit_u8(frames)  # both in flight, on two lanes
    assert np.array_equal(engine.collect_u8(), twin_frames(frames, base, "meanstd", (256,) * B))
    assert np.array_equal(slot.collect_u8(), twin_frames(frames, base, "meanstd", (64,) * B))


# ------------------------------------------------------------------------------------------ 4. the class
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


def test_the_class_matches_colours_and_follows_set_color_match(monkeypatch):
    opts = dict(prompt="a watercolor painting", height=H, width=W, strength=0.6, steps=STEPS, controlnet_scale=1.5)
    frames = _frames()[:2]
    imgs = [Image.fromarray(f, "RGB") for f in frames]
    base = [np.asarray(o) for o in _pipeline(monkeypatch).infer_batch(imgs, **opts)]
    p = _pipeline(monkeypatch, color_match="histogram", color_amount=0.5)
    handle = p.submit_batch(imgs, **opts)
    outs = [np.asarray(o) for o in p.collect_batch(handle)]
    eng = handle.engine
    assert eng.plan["color_match"] == "histogram" and eng.color_a == (128, 128)
    for b in range(2):
        assert np.array_equal(outs[b], twin(frames[b], base[b], "histogram", 128)), b
    graph = eng.graph
    assert p.set_color_match(1.0) == 1.0
    handle = p.submit_batch(imgs, **opts)
    outs = [np.asarray(o) for o in p.collect_batch(handle)]
    assert handle.engine is eng and eng.graph is graph and eng.color_a == (256, 256)  # the same engine and capture, a new amount
    for b in range(2):
        assert np.array_equal(outs[b], twin(frames[b], base[b], "histogram", 256)), b
    one = np.asarray(p.infer(imgs[1], **opts))  # an engine prepared after the change starts with the amount in place
    base_one = np.asarray(_pipeline(monkeypatch).infer(imgs[1], **opts))
    assert np.array_equal(one, twin(frames[1], base_one, "histogram", 256))

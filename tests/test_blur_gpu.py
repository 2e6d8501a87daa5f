"""The device Gaussian blur on the MI355X (csrc/blur.hip) against the numpy restatement of THE BLUR CONTRACT (include/vsd.h) of
tests/blur_cases.py, byte for byte: every shape x channel count x frame count x tap table x content with src and dst each 16-byte
aligned and one byte off, inside buffers of canaries; a captured graph that follows a new table; the engine (`edge_blur` ahead of
either edge op feeds that op and nothing else; `mask_feather` is the plain keep-mask engine on the blurred masks, bit for bit; live
changes; two lanes); the class; one poisoned run of the engine cases.

Shapes: the smallest that reach each path -- narrower than any radius, one tile exactly, one byte / row short of it and beyond it,
several tiles per frame; MINI networks, 2 steps, 64 x 64 and 72 x 120."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import blur_cases as BC  # noqa: E402
import keep_mask_cases as KM  # noqa: E402

from videosd_amd import blur as BL  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FRAMES = os.path.join(HERE, "golden", "default_frames_mini_64x64_before_color_match.npy")
CANARY = 0xC3
PAD = 64  # canary bytes either side of an operand


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _placed(n, skew, fill=None):
    """n bytes `skew` bytes past a 16-byte boundary inside a buffer of canaries -> (holder, view of the operand, its start)"""
    holder = torch.full((PAD + 16 + n + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + ((-(holder.data_ptr() + PAD)) % 16) + skew
    view = holder[start:start + n]
    assert view.data_ptr() % 16 == skew
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill, dtype=np.uint8)).reshape(-1))  # (a copy: the shared cases are read-only)
    return holder, view, start


def _canaries_intact(holder, start, n):
    h = holder.cpu().numpy()
    return bool((h[:start] == CANARY).all() and (h[start + n:] == CANARY).all())


def _taps_dev(taps):
    return torch.from_numpy(np.array(taps, dtype=np.int32)).cuda()


# ------------------------------------------------------------------------------------------ 1. the kernel against the contract
@pytest.mark.parametrize("channels", BC.CHANNELS)
@pytest.mark.parametrize("shape", BC.SHAPES)
def test_kernel_equals_the_contract_at_every_base(ops, shape, channels):
    h, w = shape
    tables = {name: _taps_dev(t) for name, t in BC.TAP_SETS.items()}
    for frames in BC.FRAME_COUNTS:
        n = frames * h * w * channels
        for ks in BC.SKEWS:
            for kd in BC.SKEWS:
                for content in BC.CONTENTS:
                    src = BC.image(content, frames, h, w, channels)
                    sh, sv, s0 = _placed(n, ks, src)
                    for name in BC.TAP_SETS:
                        dh, dv, d0 = _placed(n, kd)
                        torch.cuda.synchronize()  # (the operands were placed on torch's stream; the op runs on its own)
                        ops.gauss_blur(sv, dv, frames, h, w, channels, tables[name])
                        ops.synchronize()
                        got, want = dv.cpu().numpy().reshape(src.shape), BC.expected(content, frames, h, w, channels, name)
                        assert np.array_equal(got, want), (shape, channels, frames, (ks, kd), content, name, int((got != want).sum()), "bytes differ")
                        assert _canaries_intact(dh, d0, n), "bytes outside dst were written"
                    assert _canaries_intact(sh, s0, n) and np.array_equal(sv.cpu().numpy(), src.reshape(-1)), "src changed"


def test_a_captured_graph_reads_the_pointer_to_the_taps(ops):
    """captured once; the tap block is overwritten and the graph replayed: the new table's bytes come out"""
    frames, h, w, c = 3, 72, 120, 3
    src = BC.image("random", frames, h, w, c)
    dsrc, ddst = torch.from_numpy(np.array(src)).cuda(), torch.zeros(src.shape, dtype=torch.uint8, device="cuda")
    taps = _taps_dev(BC.TAP_SETS["s1.4"])
    torch.cuda.synchronize()
    ops.gauss_blur(dsrc, ddst, frames, h, w, c, taps)  # (once outside the capture: the module is loaded)
    ops.synchronize()
    ops.graph_begin()
    ops.gauss_blur(dsrc, ddst, frames, h, w, c, taps)
    g = ops.graph_end()
    try:
        for name in ("s1.4", "far32", "s10.0", "identity"):
            taps.copy_(_taps_dev(BC.TAP_SETS[name]))
            ddst.zero_()
            torch.cuda.synchronize()
            ops.graph_launch(g)
            ops.synchronize()
            assert np.array_equal(ddst.cpu().numpy(), BC.expected("random", frames, h, w, c, name)), name
    finally:
        ops.graph_destroy(g)


def test_bad_arguments_are_refused_with_a_message(ops):
    buf = torch.zeros(2 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    taps = _taps_dev(BC.TAP_SETS["s1.4"])
    a, b = buf[:64 * 64 * 3], buf[64 * 64 * 3:]
    for frames, h, w, c in ((0, 8, 8, 1), (1025, 1, 1, 1), (1, 0, 8, 3), (1, 8, 16385, 1), (1, 8, 8, 2)):
        with pytest.raises(RuntimeError, match="gauss_blur.*frames must be"):
            ops.gauss_blur(a, b, frames, h, w, c, taps)
    with pytest.raises(RuntimeError, match="gauss_blur: src and dst overlap"):
        ops.gauss_blur(a, buf[100:], 1, 64, 64, 3, taps)
    with pytest.raises(RuntimeError, match="gauss_blur: null pointer, or taps_dev not 4-byte aligned"):
        ops.gauss_blur(a, b, 1, 64, 64, 3, taps.view(torch.uint8)[1:])


# ------------------------------------------------------------------------------------------ 2. the engine
@pytest.fixture(scope="module")
def engine():
    return BC.make_engine()


@pytest.fixture(scope="module")
def results():
    """digests of the engine cases of this process, for the poisoned child to be held to"""
    return {}


@pytest.mark.parametrize("mode,H,W", BC.EDGE_CASES)
def test_edge_blur_feeds_the_edge_op_and_nothing_else(engine, results, mode, H, W):
    frames = BC.edge_camera(H, W)
    got = BC.edge_case(engine, mode, H, W)
    assert got["edge"].any()
    results[f"{mode}_{H}x{W}"] = BC.digest(got)
    graph, program = engine.graph, engine.program
    assert graph is not None and [fn.__name__ for fn, _a, _k in engine.flat_calls(program.calls)].count("gauss_blur") == 1
    assert np.array_equal(engine.blur_u8.cpu().numpy(), BC.blur_numpy(frames, BL.gauss_taps(BC.EDGE_SIGMA)))
    assert np.array_equal(engine.frame_u8.cpu().numpy(), frames)  # the camera's frames stay as they came
    # live: sigma 0 gives the switch-less engine's edges; another sigma those of a fresh engine prepared with it; no re-capture
    engine.set_edge_blur(0)
    engine.infer_u8(frames)
    zero = dict(edge=BC._cpu(engine.edge_u8), control=BC._cpu(engine.buffers["control"]).view(np.uint16))
    engine.set_edge_blur(3.0)
    out3 = engine.infer_u8(frames).copy()
    live = dict(out=out3, edge=BC._cpu(engine.edge_u8), control=BC._cpu(engine.buffers["control"]).view(np.uint16))
    assert engine.graph is graph and engine.program is program
    fresh = BC.edge_case(engine, mode, H, W, sigma=3.0)
    assert all(np.array_equal(live[k], fresh[k]) for k in live) and not np.array_equal(fresh["edge"], got["edge"])
    # the engine WITHOUT the switch: on the blurred frames its edge map and control buffer are ours; on the camera's frames its x0 is ours
    plan = engine.prepare(H, W, BC.STEPS, 0.6, edges=mode, **BC.PREP)
    assert plan["edge_blur"] is False and engine.taps == {}
    engine.infer_u8(BC.blur_numpy(frames, BL.gauss_taps(BC.EDGE_SIGMA)))
    assert np.array_equal(BC._cpu(engine.edge_u8), got["edge"]) and np.array_equal(BC._cpu(engine.buffers["control"]).view(np.uint16), got["control"])
    engine.infer_u8(frames)
    assert np.array_equal(BC._cpu(engine.buffers["x0"]).view(np.uint16), got["x0"])
    assert np.array_equal(BC._cpu(engine.edge_u8), zero["edge"]) and np.array_equal(BC._cpu(engine.buffers["control"]).view(np.uint16), zero["control"])
    assert not np.array_equal(zero["edge"], got["edge"])  # (the blur did change the edges)


def test_mask_feather_is_the_keep_mask_engine_on_the_blurred_masks(engine, results):
    H = W = 64
    frames, masks = BC.camera(H, W), KM.engine_masks(BC.B, H, W)
    soft = BC.blur_numpy(masks, BL.gauss_taps(BC.FEATHER_SIGMA))
    got = BC.feather_case(engine, masks)
    results["feather"] = BC.digest(got)
    graph, program = engine.graph, engine.program
    assert np.array_equal(engine.mask_soft.cpu().numpy(), soft) and np.array_equal(engine.mask_u8.cpu().numpy(), masks)
    # an all-255 mask still reproduces the recorded default frames
    engine.set_masks(None)
    assert np.array_equal(engine.infer_u8(frames), np.load(GOLDEN_FRAMES))
    # live changes: another sigma gives the frames of a fresh engine prepared with it, 0 those of the switch-less engine; no re-capture
    engine.set_masks(masks)
    engine.set_mask_feather(1.4)
    live14 = engine.infer_u8(frames).copy()
    engine.set_mask_feather(0)
    live0 = engine.infer_u8(frames).copy()
    assert engine.graph is graph and engine.program is program
    # two lanes in flight with a change between their submissions: each keeps the table it was submitted with
    slot = engine.make_slot()
    slot.prepare(H, W, BC.STEPS, 0.6, keep_mask=True, mask_feather=BC.FEATHER_SIGMA, **BC.PREP)
    slot.set_masks(masks)
    engine.set_mask_feather(BC.FEATHER_SIGMA)
    engine.submit_u8(frames)
    slot.set_mask_feather(1.4)
    slot.submit_u8(frames)
    engine.set_mask_feather(0)  # (noted for the launch after this one)
    assert np.array_equal(engine.collect_u8(), got["out"]) and np.array_equal(slot.collect_u8(), live14)
    assert np.array_equal(BC.feather_case(engine, masks, sigma=1.4)["out"], live14)
    # the engine WITHOUT the feather, handed the blurred masks: bit for bit
    plan = engine.prepare(H, W, BC.STEPS, 0.6, keep_mask=True, **BC.PREP)
    assert plan["mask_feather"] is False
    engine.set_masks(soft)
    assert np.array_equal(engine.infer_u8(frames), got["out"])
    engine.set_masks(masks)
    plain = engine.infer_u8(frames)
    assert np.array_equal(plain, live0) and not np.array_equal(plain, got["out"]) and not np.array_equal(live14, got["out"])


def test_the_engine_cases_with_every_fresh_buffer_poisoned(engine, results):
    """one run of each engine case under VSD_POISON=1, in a child process: the same bytes"""
    for mode, H, W in BC.EDGE_CASES:  # (the tests above left their digests; run alone, this test makes them itself)
        if f"{mode}_{H}x{W}" not in results:
            results[f"{mode}_{H}x{W}"] = BC.digest(BC.edge_case(engine, mode, H, W))
    if "feather" not in results:
        results["feather"] = BC.digest(BC.feather_case(engine, KM.engine_masks(BC.B, 64, 64)))
    res = subprocess.run([sys.executable, os.path.join(HERE, "poison_check_blur.py")], env=dict(os.environ, VSD_POISON="1"), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]) == results


# ------------------------------------------------------------------------------------------ 3. the class
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


def test_the_class_changes_both_sigmas_between_two_lanes_in_flight(monkeypatch):
    opts = dict(prompt="a watercolor painting", height=64, width=64, strength=0.6, steps=BC.STEPS, controlnet_scale=1.5)
    rng = np.random.default_rng(4)
    cams = [Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), "RGB") for _ in range(2)]
    left = np.full((96, 128), 255, np.uint8)
    left[:, :64] = 0
    plain = _pipeline(monkeypatch, keep_mask=True, edges="canny")
    plain.set_mask(left)
    base = [np.asarray(o) for o in plain.infer_batch(cams, **opts)]
    p = _pipeline(monkeypatch, keep_mask=True, edges="canny", edge_blur=1.4, mask_feather=4.0, lanes=2)
    p.set_mask(left)
    first = p.submit_batch(cams, lane=0, **opts)
    assert p.set_edge_blur(0) == 0.0 and p.set_mask_feather(0) == 0.0
    second = p.submit_batch(cams, lane=1, **opts)
    blurred, unblurred = ([np.asarray(o) for o in p.collect_batch(h)] for h in (first, second))
    assert first.engine is not second.engine and first.engine.taps["mask_feather"].sigma == 4.0 and second.engine.taps["mask_feather"].sigma == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(unblurred, base))  # sigma 0: the frames of the pipeline without the switches
    assert not any(np.array_equal(a, b) for a, b in zip(blurred, base))
    graph = first.engine.graph
    again = p.submit_batch(cams, lane=0, **opts)  # lane 0's engine takes the new tables ahead of its next launch, capture intact
    assert again.engine is first.engine and all(np.array_equal(np.asarray(a), b) for a, b in zip(p.collect_batch(again), base)) and again.engine.graph is graph
    fresh = _pipeline(monkeypatch, keep_mask=True, edges="canny", edge_blur=1.4, mask_feather=4.0)
    fresh.set_mask(left)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(fresh.infer_batch(cams, **opts), blurred))

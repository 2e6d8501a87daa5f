"""Canny edges on the MI355X (csrc/canny.hip) against the host twin vsd_canny_host, which tests/test_canny_host.py holds to the numpy
restatement of THE EDGE CONTRACT (include/vsd.h): every byte of the edge map, every lane of the conditioning rows; determinism; the
engine, the CPU oracle fed the restatement's edge map, and the drop-in class.

Shapes (tile of launch 1: 32 x 16 pixels): frames smaller than a tile, one pixel either side of two tiles' width and of two tiles' height,
many tiles in both directions (the serpentine's one component crosses every border of the frame many times, so a missing or a wrong
union between tiles shows as missing edges), and the sizes the host tests use."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import canny_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 16  # csrc/canny_core.h CANNY_TW, CANNY_TH


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def canny_host(rgb, low, high):
    from videosd_amd import lib as L

    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    edge = np.full((h, w), 77, np.uint8)
    assert L.load().vsd_canny_host(rgb.ctypes.data, h, w, int(low), int(high), edge.ctypes.data) == 0
    return edge


def run_device(ops, rgb, low, high, skew=0, poison=0xA5):
    """ops.canny_control on a frame that starts `skew` bytes into its buffer, into poisoned outputs -> (edge [h][w], control [h*w][8])"""
    h, w = rgb.shape[:2]
    holder = torch.full((skew + h * w * 3 + 64,), 255, dtype=torch.uint8, device="cuda")  # 255s around: a read outside the frame would show
    frame = holder[skew:skew + h * w * 3]
    frame.copy_(torch.from_numpy(np.array(rgb, dtype=np.uint8)).reshape(-1))  # (a copy: the shared references are read-only)
    edge = torch.full((h * w,), poison, dtype=torch.uint8, device="cuda")
    ctrl = torch.full((h * w, 8), float("nan"), dtype=torch.float16, device="cuda")
    ops.canny_control(frame, h, w, low, high, edge, ctrl)
    ops.synchronize()
    return edge.cpu().numpy().reshape(h, w), ctrl.cpu()


def assert_device_equals_host(ops, rgb, low, high, skew=0):
    ref = canny_host(rgb, low, high)
    edge, ctrl = run_device(ops, rgb, low, high, skew)
    assert np.array_equal(edge, ref), (rgb.shape, low, high, skew, int((edge != ref).sum()), "bytes differ")
    want = torch.zeros(ref.size, 8, dtype=torch.float16)
    want[:, :3] = torch.from_numpy((ref.reshape(-1) > 0).astype(np.float32)).half()[:, None]
    assert torch.equal(ctrl.view(torch.int16), want.view(torch.int16))  # exact 0 / 1 rows, zero padding lanes, as bits
    return ref


# ------------------------------------------------------------------------------------------ 1. device against host
@pytest.mark.parametrize("thr", CC.THRESHOLDS)
@pytest.mark.parametrize("h,w", [(72, 120), (37, 301), (64, 64)])
def test_device_equals_host_on_noise(ops, h, w, thr):
    f, parts = CC.reference("noise", h, w, *thr)
    CC.assert_exercises("noise", h, w, parts)
    ref = assert_device_equals_host(ops, f, *thr)
    assert np.array_equal(ref, parts["edge"])


@pytest.mark.parametrize("kind", ["serpentine", "serpentine_noseed"])
@pytest.mark.parametrize("h,w", CC.SERPENTINE_SIZES)
def test_device_equals_host_on_the_serpentine(ops, h, w, kind):
    f, parts = CC.reference(kind, h, w)
    CC.assert_exercises(kind, h, w, parts)
    assert h > 2 * TILE_H and w > 2 * TILE_W  # several tiles in both directions
    ref = assert_device_equals_host(ops, f, 100, 200)
    assert np.array_equal(ref, parts["edge"])


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (3, 3), (7, 1), (2, 2)])
def test_device_equals_host_on_tiny_frames(ops, h, w):
    rng = np.random.default_rng(h * 100 + w)
    for thr in ((0, 0), (100, 200)):
        for _ in range(3):
            assert_device_equals_host(ops, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), *thr)


@pytest.mark.parametrize("h,w", [(24, 2 * TILE_W - 1), (24, 2 * TILE_W + 1), (2 * TILE_H - 1, 70), (2 * TILE_H + 1, 70), (2 * TILE_H, 2 * TILE_W)])
def test_device_equals_host_around_tile_multiples(ops, h, w):
    f = CC.noise_frame(h, w, seed=h * 1000 + w)
    assert CC.canny_parts(f, 50, 150)["edge"].any()
    assert_device_equals_host(ops, f, 50, 150)
    rng = np.random.default_rng(w)
    binary = np.repeat((rng.integers(0, 2, (h, w, 1)) * 255).astype(np.uint8), 3, axis=2)  # dense candidates, many ties, unions across every border
    assert_device_equals_host(ops, binary, 0, 0)


@pytest.mark.parametrize("skew", range(1, 16))
def test_device_equals_host_with_a_skewed_frame_pointer(ops, skew):
    assert_device_equals_host(ops, CC.reference("noise", 37, 301)[0], 100, 200, skew=skew)


def test_a_constant_frame_has_no_edges_and_no_nan(ops):
    for value in (0, 93, 255):
        edge, ctrl = run_device(ops, CC.constant_frame(40, 70, value), 0, 0)
        assert not edge.any() and torch.equal(ctrl.view(torch.int16), torch.zeros(40 * 70, 8, dtype=torch.int16))


def test_bad_arguments_are_refused_by_name(ops):
    f = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device="cuda")
    edge, ctrl = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(64, 8, dtype=torch.float16, device="cuda")
    for low, high in ((-1, 10), (10, 5), (0, 2041)):
        with pytest.raises(RuntimeError, match="low <= high"):
            ops.canny_control(f, 8, 8, low, high, edge, ctrl)


# ------------------------------------------------------------------------------------------ 2. determinism
def test_the_same_call_twice_gives_the_same_bytes(ops):
    for kind, h, w in (("noise", 72, 120), ("serpentine", 136, 264)):
        f = CC.reference(kind, h, w)[0]
        a = run_device(ops, f, 100, 200, poison=0xA5)
        b = run_device(ops, f, 100, 200, poison=0x5A)
        assert np.array_equal(a[0], b[0]) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


# ------------------------------------------------------------------------------------------ 3. the engine
H, W, STEPS = 120, 72, 2
THR = (100, 200)


def _build(unet_cfg, cn_cfg):
    from videosd_amd import config as C
    from videosd_amd import weights as Wt

    wu = Wt.synthesize(Wt.unet_spec(unet_cfg), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(cn_cfg), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(C.TAESD), "vae.", device="cuda")
    text = (torch.randn(77, unet_cfg.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half()
    return wu, wc, wv, text


def _cpu(w):
    return {k: v.cpu() for k, v in w.items()}


def _setup(unet_cfg, cn_cfg):
    from oracle.pipeline import OraclePipeline
    from videosd_amd import config as C
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu, wc, wv, text = _build(unet_cfg, cn_cfg)
    eng = Engine(HipOps(0), unet_cfg, cn_cfg, C.TAESD, wu, wc, wv)
    eng.set_text_embeds(text)
    return eng, OraclePipeline(unet_cfg, cn_cfg, _cpu(wu), _cpu(wc), _cpu(wv)), text


@pytest.fixture(scope="module")
def mini_setup():
    from videosd_amd import config as C

    return _setup(C.MINI_UNET, C.MINI_CONTROLNET)


def _frames():
    return np.stack([CC.noise_frame(H, W, seed=s) for s in (1, 2, 3)])


def _edges_of(eng, b=0):
    return eng.edge_u8[b * H * W:(b + 1) * H * W].cpu().numpy().reshape(H, W)


def test_engine_three_frames_replay_eager_and_lone_frames(mini_setup):
    """A 3-frame launch of three different frames.  What the edge stage writes -- every frame's edge map and conditioning rows -- equals the
    host twin's and the lone-frame launch's bit for bit, and replay equals eager bit for bit, output frames included.  The OUTPUT frame of
    a 3-frame launch against the lone-frame launch is held to the bound tests/test_pipeline_gpu.py
    test_batched_frames_match_oracle_and_single_frames holds the default program to (mean |difference| < 0.5 LSB): the denoiser picks
    other tiles / split-K for another M, so its fp32 sums run in another order -- with either edge stage (measured here: 0.10 LSB mean,
    the frames not equal, while the edge maps and conditioning rows are)."""
    eng, _orc, _text = mini_setup
    frames = _frames()
    want = [canny_host(f, *THR) for f in frames]
    assert all(e.any() for e in want) and not np.array_equal(want[0], want[1])
    prep = dict(controlnet_scale=1.5, use_controlnet=True, edges="canny", canny_thresholds=THR)
    plan = eng.prepare(H, W, STEPS, 0.6, batch=3, use_graph=True, **prep)
    assert plan["edge_mode"] == "canny" and plan["canny_thresholds"] == THR
    got = eng.infer_u8(frames).copy()
    for b in range(3):
        assert np.array_equal(_edges_of(eng, b), want[b]), b
    ctrl = eng.buffers["control"].cpu()
    flat = np.concatenate([e.reshape(-1) for e in want])
    ref_ctrl = torch.zeros(3 * H * W, 8, dtype=torch.float16)
    ref_ctrl[:, :3] = torch.from_numpy((flat > 0).astype(np.float32)).half()[:, None]
    assert torch.equal(ctrl.view(torch.int16), ref_ctrl.view(torch.int16))
    assert np.array_equal(eng.infer_u8(frames), got)  # replay is deterministic
    eng.prepare(H, W, STEPS, 0.6, batch=3, use_graph=False, **prep)
    assert np.array_equal(eng.infer_u8(frames), got)  # replay equals eager
    eng.prepare(H, W, STEPS, 0.6, batch=1, use_graph=True, **prep)
    for b in range(3):
        lone = eng.infer_u8(frames[b])
        assert np.array_equal(_edges_of(eng), want[b])
        assert torch.equal(eng.buffers["control"].cpu().view(torch.int16), ref_ctrl[b * H * W:(b + 1) * H * W].view(torch.int16))
        mad = float(np.abs(lone.astype(int) - got[b].astype(int)).mean())
        print(f"frame {b}: 3-frame launch against lone launch, mean |difference| {mad:.4f} LSB, equal: {np.array_equal(lone, got[b])}")
        assert mad < 0.5
    # and the mode changes the picture: the Sobel program conditions on another map
    eng.prepare(H, W, STEPS, 0.6, controlnet_scale=1.5, use_controlnet=True)
    assert eng.plan["edge_mode"] == "sobel" and not np.array_equal(eng.infer_u8(frames[2]), lone)


def test_two_lanes_in_flight_equal_the_sequential_run(mini_setup):
    """Two engines on two launch lanes, each with its own workspace (ops.canny_control): launches in flight at once give the sequential bytes."""
    eng, _orc, _text = mini_setup
    prep = dict(controlnet_scale=1.0, use_controlnet=True, edges="canny", canny_thresholds=THR)
    eng.prepare(H, W, STEPS, 0.6, **prep)
    frames = [CC.noise_frame(H, W, seed=s) for s in (11, 12)] + [np.ascontiguousarray(CC.serpentine_frame(H, W)), CC.noise_frame(H, W, seed=14)]
    seq, seq_edges = [], []
    for f in frames:
        seq.append(eng.infer_u8(f).copy())
        seq_edges.append(_edges_of(eng).copy())
        assert np.array_equal(seq_edges[-1], canny_host(f, *THR))
    slot = eng.make_slot()
    assert slot.ops is not eng.ops and slot.ops.lane != eng.ops.lane
    slot.prepare(H, W, STEPS, 0.6, **prep)
    engines = [eng, slot]
    for _rep in range(3):
        for pair in ((0, 1), (2, 3)):
            for e, k in zip(engines, pair):
                e.ops.upload(e.frame_u8, torch.from_numpy(frames[k]))
                e.launch()  # both graphs are now in flight on different streams
            for e, k in zip(engines, pair):
                assert np.array_equal(e.ops.download(e.out_u8).numpy(), seq[k]), k
                assert np.array_equal(_edges_of(e), seq_edges[k]), k


# ------------------------------------------------------------------------------------------ 4. end to end against the oracle
def _oracle_with_canny(monkeypatch):
    import oracle.pipeline as OP

    def canny_edges(img, low=None, high=None):  # (the oracle passes the Sobel stand-in's thresholds: not used here)
        return Image.fromarray(CC.canny_numpy(np.asarray(img.convert("RGB")), *THR), mode="L")

    monkeypatch.setattr(OP, "sobel_edges", canny_edges)


def _compare(eng, orc, frame, text, h, w, steps, cn_scale):
    """the comparison of tests/test_pipeline_gpu.py `_compare`, with its tolerances"""
    got = eng.infer_u8(frame)
    ref = np.asarray(orc.infer(Image.fromarray(frame, "RGB"), text[None].float(), height=h, width=w, strength=0.6, steps=steps, seed=23,
                               controlnet_scale=cn_scale, use_controlnet=True, keep_trace=True))
    h0, w0 = h // 8, w // 8
    x0 = eng.buffers["x0"][:, :4].float().cpu().reshape(h0, w0, 4).permute(2, 0, 1)
    ref_x0 = orc.trace["init_latents"][0]
    r0 = float((x0 - ref_x0).norm() / ref_x0.norm())
    den = eng.buffers["denoised"][:, :4].float().cpu().reshape(h0, w0, 4).permute(2, 0, 1)
    ref_den = orc.trace["denoised"][-1][0]
    r1 = float((den - ref_den).norm() / ref_den.norm())
    mse = np.mean((got.astype(np.float64) - ref.astype(np.float64)) ** 2)
    psnr = 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
    mad = float(np.abs(got.astype(int) - ref.astype(int)).mean())
    print(f"{h} x {w}, {steps} steps: r0 {r0:.2e} r1 {r1:.2e} mean abs {mad:.3f} LSB psnr {psnr:.1f} dB")
    assert r0 <= 5e-3 and r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0, (r0, r1, mad, psnr)
    return got


def test_mini_pipeline_with_canny_matches_the_oracle(mini_setup, monkeypatch):
    eng, orc, text = mini_setup
    f = CC.noise_frame(128, 128, seed=5)
    assert CC.canny_numpy(f, *THR).any()
    eng.prepare(128, 128, 2, 0.6, controlnet_scale=1.5, use_controlnet=True)
    sobel = eng.infer_u8(f).copy()
    eng.prepare(128, 128, 2, 0.6, controlnet_scale=1.5, use_controlnet=True, edges="canny", canny_thresholds=THR)
    _oracle_with_canny(monkeypatch)
    got = _compare(eng, orc, f, text, 128, 128, 2, 1.5)
    assert not np.array_equal(got, sobel)  # (the conditioning does reach the picture: an oracle on the Sobel map is another frame)


def test_sd15_width_pipeline_with_canny_matches_the_oracle(monkeypatch):
    from videosd_amd import config as C

    eng, orc, text = _setup(C.SD15_UNET, C.SD15_CONTROLNET)
    f = CC.noise_frame(64, 64, seed=6)
    assert CC.canny_numpy(f, *THR).any()
    eng.prepare(64, 64, 2, 0.6, controlnet_scale=1.0, use_controlnet=True, edges="canny", canny_thresholds=THR)
    _oracle_with_canny(monkeypatch)
    _compare(eng, orc, f, text, 64, 64, 2, 1.0)


# ------------------------------------------------------------------------------------------ 5. the class; the default untouched
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


OPTS = dict(prompt="a watercolor painting", height=H, width=W, strength=0.6, steps=STEPS, controlnet_scale=1.5)


def test_the_default_is_untouched(monkeypatch):
    """a pipeline built with edges="sobel" spelled out produces the bytes of one built without the kwarg"""
    img = Image.fromarray(CC.noise_frame(H, W, seed=3), "RGB")
    plain = np.asarray(_pipeline(monkeypatch).infer(img, **OPTS))
    explicit = np.asarray(_pipeline(monkeypatch, edges="sobel").infer(img, **OPTS))
    assert np.array_equal(plain, explicit)


def test_the_class_runs_canny_when_asked(monkeypatch):
    f = CC.noise_frame(H, W, seed=3)
    img = Image.fromarray(f, "RGB")
    p = _pipeline(monkeypatch, edges="canny", canny_thresholds=(50.5, 150))
    assert p.edges == "canny" and p.canny_thresholds == (50, 150)
    handle = p.submit_batch([img, img], **OPTS)
    outs = [np.asarray(o) for o in p.collect_batch(handle)]
    eng = handle.engine
    assert eng.plan["edge_mode"] == "canny" and eng.plan["canny_thresholds"] == (50, 150)
    want = canny_host(f, 50, 150)
    assert want.any() and np.array_equal(_edges_of(eng, 0), want) and np.array_equal(_edges_of(eng, 1), want)
    assert not np.array_equal(outs[0], np.asarray(_pipeline(monkeypatch).infer(img, **OPTS)))

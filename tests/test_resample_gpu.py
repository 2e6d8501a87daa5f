"""The centre crop + LANCZOS resize on the device (csrc/resample.hip) against PIL on the host, through every layer that uses it:
the op, the engine, the drop-in class and the plan entry points of a C host.  Every comparison is np.array_equal: there is no
tolerance anywhere in this feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import resample_cases as R
from test_plan_gpu import _engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _host(f, tw, th):
    from videosd_amd.pipeline import center_crop_resize

    return np.asarray(center_crop_resize(Image.fromarray(f, "RGB"), tw, th))


def _device(ops, f, box, dst_hw, pad=0, canary=64):
    """ops.resample_rgb of frame f (rows padded by `pad` bytes) into a destination with `canary` bytes in front of and behind it"""
    h, w = f.shape[:2]
    row = 3 * w + pad
    src = np.full((h, row), 0x5A, np.uint8)
    src[:, :3 * w] = f.reshape(h, 3 * w)
    n = dst_hw[0] * dst_hw[1] * 3
    dsrc = torch.from_numpy(src).to(ops.device)
    ddst = torch.full((canary + n + canary,), 0xA5, dtype=torch.uint8, device=ops.device)
    ops.synchronize()
    torch.cuda.synchronize()
    ops.resample_rgb(dsrc, h, w, row, box, ddst[canary:canary + n], dst_hw[0], dst_hw[1])
    ops.synchronize()
    out = ddst.cpu().numpy()
    assert (out[:canary] == 0xA5).all() and (out[canary + n:] == 0xA5).all(), "the kernel wrote outside its destination"
    return out[canary:canary + n].reshape(dst_hw[0], dst_hw[1], 3)


@pytest.mark.parametrize("case", R.CENTRE_CASES, ids=R.case_id)
def test_the_device_resample_gives_pillows_bytes(ops, case):
    (sh, sw), (th, tw), kind = case
    f = R.frame((sh, sw), kind)
    box = ops.center_crop_box(sw, sh, tw, th)
    assert box == R.python_box(sw, sh, tw, th)
    assert np.array_equal(_device(ops, f, box, (th, tw)), _host(f, tw, th))


@pytest.mark.parametrize("case", R.BOX_CASES, ids=R.case_id)
def test_an_explicit_box_that_skips_one_pass(ops, case):
    src, box, dst = case
    f = R.frame(src)
    assert np.array_equal(_device(ops, f, box, dst), R.pillow_box_resize(f, box, dst))


@pytest.mark.parametrize("pad,canary", [(5, 64), (64, 61), (1, 3)])
def test_padded_source_rows_and_an_untouched_neighbourhood_of_the_destination(ops, pad, canary):
    """src_row_bytes > 3 * w, and a destination that does not start on a 4-byte boundary (the byte-wide form of the vertical pass)"""
    f = R.frame((720, 1280), seed=pad)
    box = ops.center_crop_box(1280, 720, 512, 512)
    assert np.array_equal(_device(ops, f, box, (512, 512), pad=pad, canary=canary), _host(f, 512, 512))
    f = R.frame((300, 301), seed=pad + 1)  # an odd target width: rows of the intermediate that are no multiple of 4 bytes
    box = ops.center_crop_box(301, 300, 250, 200)
    assert np.array_equal(_device(ops, f, box, (200, 250), pad=pad, canary=canary), _host(f, 250, 200))


def test_what_the_op_does_not_support_is_refused_with_a_reason(ops):
    src = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device=ops.device)
    dst = torch.zeros(32 * 32 * 3, dtype=torch.uint8, device=ops.device)
    with pytest.raises(RuntimeError, match="box"):
        ops.resample_rgb(src, 64, 64, 192, (0, 0, 65, 64), dst, 32, 32)
    with pytest.raises(RuntimeError, match="box"):
        ops.resample_rgb(src, 64, 64, 192, (10, 0, 10, 64), dst, 32, 32)
    with pytest.raises(RuntimeError, match="src_row_bytes"):
        ops.resample_rgb(src, 64, 64, 100, (0, 0, 64, 64), dst, 32, 32)
    with pytest.raises(RuntimeError, match="side"):
        ops.ctx.call("vsd_resample_rgb", ops._p(src), 64, 20000, 60000, (C.c_int * 4)(0, 0, 64, 64), ops._p(dst), 32, 32, None, None, None, ops.s)
    with pytest.raises(RuntimeError, match="table"):
        ops.ctx.call("vsd_resample_rgb", ops._p(src), 64, 64, 192, (C.c_int * 4)(0, 0, 64, 64), ops._p(dst), 32, 32, None, None, None, ops.s)
    ops.synchronize()
    assert len(ops._resample_tables) <= ops.RESAMPLE_TABLES


@pytest.mark.parametrize("H,W", [(512, 512), (360, 640)])
def test_the_engine_takes_camera_frames(H, W):
    """Engine.infer_raw_u8(frame) == Engine.infer_u8(PIL's crop + resize of it): one frame, and a batch of three sources of different sizes"""
    eng = _engine(batch=1, H=H, W=W)
    f = R.frame((720, 1280), seed=H)
    want = eng.infer_u8(_host(f, W, H)).copy()
    assert np.array_equal(eng.infer_raw_u8(f), want)
    same = R.frame((H, W), seed=H + 1)  # already the target size: no kernel, the frame goes straight in
    assert np.array_equal(eng.infer_raw_u8(same), eng.infer_u8(same))
    assert np.array_equal(eng.infer_raw_u8(f), want)
    with pytest.raises(ValueError):
        eng.infer_raw_u8(f[..., :2])
    eng3 = _engine(batch=3, H=H, W=W)
    fs = [R.frame((720, 1280), seed=1), R.frame((1080, 1920), seed=2), R.frame((200, 300), seed=3)]
    want3 = eng3.infer_u8(np.stack([_host(x, W, H) for x in fs])).copy()
    assert np.array_equal(eng3.infer_raw_u8(fs), want3)
    with pytest.raises(ValueError):
        eng3.infer_raw_u8(fs[:2])


# tuning_mode="table": two objects must build the SAME kernels for a shape the tuning table lacks (the default times the candidates
# at `prepare`, and two timings may pick two forms whose roundings differ by an LSB -- the mode dispatch.spawn_workers sets for the
# ranks of a group, for the same reason); what is compared here is the path of the frame into the engine, not that choice
CFG = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table")
OPTS = dict(prompt="a watercolor painting", height=192, width=256, strength=0.6, steps=2, seed=7, controlnet_scale=1.5)


@pytest.fixture(scope="module")
def pipes():
    from videosd_amd.pipeline import VideoSDPipeline

    # (honor_ref_flag: `ref=True` runs the reference-only program on both objects; it changes nothing for the other frames)
    return VideoSDPipeline(honor_ref_flag=True, **CFG), VideoSDPipeline(device_resize=True, honor_ref_flag=True, **CFG)


def _img(w, h, seed, mode="RGB"):
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, (h, w, len(mode)), dtype=np.uint8), mode)


def test_the_class_returns_the_same_image_with_device_resize_on(pipes):
    off, on = pipes
    assert off.device_resize is False and on.device_resize is True  # off unless asked for
    img = _img(1280, 720, 1)
    want = np.asarray(off.infer(img, **OPTS))
    got = on.infer(img, **OPTS)
    assert got.size == (256, 192) and np.array_equal(np.asarray(got), want)
    assert any(getattr(e.ops, "_resample_tables", None) for e in on._engines.values())  # (the kernel ran: its tables are cached)
    assert not any(getattr(e.ops, "_resample_tables", None) for e in off._engines.values())
    # a batch of camera frames of different sizes through one launch
    imgs = [_img(1280, 720, 2), _img(1920, 1080, 3), _img(300, 200, 4)]
    for a, b in zip(off.infer_batch(imgs, **OPTS), on.infer_batch(imgs, **OPTS)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # the fall-backs keep the host path, and with it today's result: an RGBA frame, a target that is no multiple of 8, a frame
    # already of the target size
    rgba = _img(1280, 720, 5, "RGBA")
    assert np.array_equal(np.asarray(on.infer(rgba, **OPTS)), np.asarray(off.infer(rgba, **OPTS)))
    o150 = dict(OPTS, height=100, width=150)
    a, b = on.infer(img, **o150), off.infer(img, **o150)
    assert a.size == (144, 96) and np.array_equal(np.asarray(a), np.asarray(b))
    sized = _img(256, 192, 6)
    assert np.array_equal(np.asarray(on.infer(sized, **OPTS)), np.asarray(off.infer(sized, **OPTS)))
    # ref=True (the reference-only mode): the first frame becomes the stored reference image
    r = dict(OPTS, ref=True)
    first, second = _img(1280, 720, 7), _img(1280, 720, 8)
    for im in (first, second):
        assert np.array_equal(np.asarray(on.infer(im, **r)), np.asarray(off.infer(im, **r)))
    assert on.metrics()["stage_ms_p50"]["crop_resize"] is not None


def test_a_c_host_feeds_camera_frames_to_a_plan(tmp_path):
    """vsd_plan_infer_frame on a raw 1280 x 720 frame == CPlan.infer on the host-resized frame; examples/camera_host.c writes those bytes too"""
    from videosd_amd.plan import CPlan, export_plan

    H, W = 128, 96
    eng = _engine(batch=1, H=H, W=W)
    f = R.frame((720, 1280), seed=11)
    path = str(tmp_path / "frame.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    try:
        want = plan.infer(_host(f, W, H))
        assert np.array_equal(want, eng.infer_u8(_host(f, W, H)))
        assert np.array_equal(plan.infer_frame(f), want)
        g = R.frame((480, 640), seed=12)  # another camera size: new tables, the same plan
        assert np.array_equal(plan.infer_frame(g), plan.infer(_host(g, W, H)))
        same = R.frame((H, W), seed=13)
        assert np.array_equal(plan.infer_frame(same), plan.infer(same))
        assert np.array_equal(plan.infer_frame(f), want)
        with pytest.raises(ValueError):
            plan.infer_frame(f[None])
    finally:
        plan.close()
    exe = str(tmp_path / "camera_host")
    libdir = os.path.join(ROOT, "videosd_amd")
    subprocess.run(["gcc", "-O2", os.path.join(ROOT, "examples", "camera_host.c"), "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lvsd",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    (tmp_path / "camera.raw").write_bytes(f.tobytes())
    r = subprocess.run([exe, path, str(tmp_path / "camera.raw"), "1280", "720", str(tmp_path / "out.raw"), "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    assert "frames/s" in r.stdout
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want)


def test_a_plan_with_several_frames_per_launch_takes_camera_frames(tmp_path):
    from videosd_amd.plan import CPlan, export_plan

    H, W = 128, 96
    eng = _engine(batch=2, H=H, W=W)
    fs = np.stack([R.frame((360, 640), seed=21), R.frame((360, 640), seed=22)])
    path = str(tmp_path / "two.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    try:
        assert np.array_equal(plan.infer_frame(fs), plan.infer(np.stack([_host(x, W, H) for x in fs])))
    finally:
        plan.close()

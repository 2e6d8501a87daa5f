"""WebRTC frames (planar YUV 4:2:0) converted on the device (csrc/yuv.hip), through every layer that uses the kernels: the two ops, the
engine, the drop-in class, a real worker behind shared memory and the plan entry points of a C host.  The reference is the numpy
statement of the colour contract in yuv_cases.py (written from include/vsd.h's formulas) around the existing RGB path; every
comparison is np.array_equal -- there is no tolerance anywhere in this file."""
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import yuv_cases as Y
from test_plan_gpu import _engine
from test_resample_gpu import CFG, OPTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _dev_plane(ops, plane, pad, lead):
    """`plane` in device memory inside rows `pad` bytes longer, starting `lead` bytes into its buffer: (buffer, view of the first byte, stride)"""
    h, w = plane.shape
    host = np.full(lead + h * (w + pad), 0x5A, np.uint8)
    host[lead:].reshape(h, w + pad)[:, :w] = plane
    buf = torch.from_numpy(host).to(ops.device)
    return buf, buf[lead:], w + pad


def _device_to_rgb(ops, y, u, v, ox=0, oy=0, pad=0, lead=0, canary=64):
    """ops.i420_to_rgb into a destination with `canary` bytes in front of and behind it and rows `pad` bytes longer than 3 * w"""
    h, w = y.shape
    _by, dy, ys = _dev_plane(ops, y, pad, lead)
    _bu, du, cs = _dev_plane(ops, u, pad, lead)
    _bv, dv, _ = _dev_plane(ops, v, pad, lead)
    row = 3 * w + pad
    n = h * row
    ddst = torch.full((canary + n + canary,), 0xA5, dtype=torch.uint8, device=ops.device)
    torch.cuda.synchronize()
    ops.i420_to_rgb(dy, ys, du, dv, cs, ox, oy, h, w, ddst[canary:canary + n], row)
    ops.synchronize()
    out = ddst.cpu().numpy()
    assert (out[:canary] == 0xA5).all() and (out[canary + n:] == 0xA5).all(), "the kernel wrote outside its destination"
    body = out[canary:canary + n].reshape(h, row)
    assert (body[:, 3 * w:] == 0xA5).all(), "the kernel wrote into the padding of its destination rows"
    return body[:, :3 * w].reshape(h, w, 3)


def _device_to_i420(ops, rgb, pad=0, canary=64):
    """ops.rgb_to_i420 into three planes, each with canaries around it and rows `pad` bytes longer"""
    h, w = rgb.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(rgb)).to(ops.device)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    bufs = [torch.full((canary + r * (c + pad) + canary,), 0xA5, dtype=torch.uint8, device=ops.device) for r, c in shapes]
    views = [b[canary:canary + r * (c + pad)] for b, (r, c) in zip(bufs, shapes)]
    torch.cuda.synchronize()
    ops.rgb_to_i420(src, h, w, views[0], views[1], views[2], w + pad, w // 2 + pad)
    ops.synchronize()
    planes = []
    for b, (r, c) in zip(bufs, shapes):
        out = b.cpu().numpy()
        n = r * (c + pad)
        assert (out[:canary] == 0xA5).all() and (out[canary + n:] == 0xA5).all(), "the kernel wrote outside a destination plane"
        body = out[canary:canary + n].reshape(r, c + pad)
        assert (body[:, c:] == 0xA5).all(), "the kernel wrote into the padding of a plane's rows"
        planes.append(body[:, :c])
    return planes


# ------------------------------------------------------------------------------------------------------------------ 1. the ops
@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("hw", Y.SIZES, ids=lambda s: "%dx%d" % s)
def test_i420_to_rgb_on_the_device_is_the_contract_byte_for_byte(ops, hw, kind):
    y, u, v = Y.yuv_frame(hw, kind, seed=hw[1])
    want = Y.contract_i420_to_rgb(y, u, v)
    assert np.array_equal(_device_to_rgb(ops, y, u, v), want)                              # tight rows: the dword-wide form where w % 4 == 0
    assert np.array_equal(_device_to_rgb(ops, y, u, v, pad=4), want)                       # padded strides, still multiples of 4
    assert np.array_equal(_device_to_rgb(ops, y, u, v, pad=5, lead=1, canary=61), want)    # nothing on a 4-byte boundary: the byte-wide form
    assert np.array_equal(_device_to_rgb(ops, y, u, v, pad=0, lead=0, canary=3), want)     # an unaligned destination alone


@pytest.mark.parametrize("hw", [(97, 131), (99, 100), (480, 640), (2, 3), (721, 1283)], ids=lambda s: "%dx%d" % s)
def test_a_rectangle_with_odd_edges_is_the_crop_of_the_converted_frame_on_the_device(ops, hw):
    y, u, v = Y.yuv_frame(hw, "noise", seed=11)
    whole = Y.contract_i420_to_rgb(y, u, v)
    h, w = hw
    for ox, oy in [(1, 0), (0, 1), (1, 1), (3, 5), (w - 1, h - 1), (w // 2, h // 3)]:
        if ox >= w or oy >= h:
            continue
        for rw, rh in [(w - ox, h - oy), (max(1, (w - ox) // 2), max(1, (h - oy) // 2))]:
            ys = np.ascontiguousarray(y[oy:oy + rh, ox:ox + rw])
            ch, cw = ((oy & 1) + rh + 1) >> 1, ((ox & 1) + rw + 1) >> 1
            us = np.ascontiguousarray(u[oy >> 1:(oy >> 1) + ch, ox >> 1:(ox >> 1) + cw])
            vs = np.ascontiguousarray(v[oy >> 1:(oy >> 1) + ch, ox >> 1:(ox >> 1) + cw])
            want = whole[oy:oy + rh, ox:ox + rw]
            assert np.array_equal(_device_to_rgb(ops, ys, us, vs, ox, oy), want)
            assert np.array_equal(_device_to_rgb(ops, ys, us, vs, ox, oy, pad=3, lead=2, canary=5), want)


@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("hw", Y.EVEN_SIZES, ids=lambda s: "%dx%d" % s)
def test_rgb_to_i420_on_the_device_is_the_contract_byte_for_byte(ops, hw, kind):
    rgb = Y.rgb_frame(hw, kind, seed=hw[0])
    want = Y.contract_rgb_to_i420(rgb)
    for pad, canary in [(0, 64), (4, 64), (5, 61), (0, 3), (1, 2)]:
        got = _device_to_i420(ops, rgb, pad=pad, canary=canary)
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_)


def test_what_the_ops_do_not_support_is_refused_with_a_reason_and_nothing_is_written(ops):
    y, u, v = Y.yuv_frame((8, 12))
    dy, du, dv = (torch.from_numpy(p.copy()).to(ops.device) for p in (y, u, v))
    dst = torch.full((64 + 8 * 36 + 64,), 0xA5, dtype=torch.uint8, device=ops.device)
    body = dst[64:64 + 8 * 36]
    with pytest.raises(RuntimeError, match="y_stride"):
        ops.i420_to_rgb(dy, 11, du, dv, 6, 0, 0, 8, 12, body, 36)
    with pytest.raises(RuntimeError, match="uv_stride"):
        ops.i420_to_rgb(dy, 12, du, dv, 5, 0, 0, 8, 12, body, 36)
    with pytest.raises(RuntimeError, match="dst_row_bytes"):
        ops.i420_to_rgb(dy, 12, du, dv, 6, 0, 0, 8, 12, body, 35)
    with pytest.raises(RuntimeError, match="null"):
        ops.i420_to_rgb(dy, 12, None, dv, 6, 0, 0, 8, 12, body, 36)
    with pytest.raises(RuntimeError, match="side"):
        ops.i420_to_rgb(dy, 1 << 20, du, dv, 1 << 20, 0, 0, 8, 20000, body, 1 << 20)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.i420_to_rgb(body, 12, du, dv, 6, 0, 0, 8, 12, body, 36)
    rgb = torch.zeros(8 * 12 * 3, dtype=torch.uint8, device=ops.device)
    planes = torch.full((64 + 8 * 12 * 3 // 2 + 64,), 0xA5, dtype=torch.uint8, device=ops.device)
    py, pu, pv = planes[64:64 + 96], planes[64 + 96:64 + 120], planes[64 + 120:64 + 144]
    with pytest.raises(RuntimeError, match="odd"):
        ops.rgb_to_i420(rgb, 7, 12, py, pu, pv)
    with pytest.raises(RuntimeError, match="odd"):
        ops.rgb_to_i420(rgb, 8, 11, py, pu, pv)
    with pytest.raises(RuntimeError, match="uv_stride"):
        ops.rgb_to_i420(rgb, 8, 12, py, pu, pv, 12, 5)
    with pytest.raises(RuntimeError, match="null"):
        ops.rgb_to_i420(rgb, 8, 12, py, None, pv)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.rgb_to_i420(rgb, 8, 12, py, pu, pu)
    ops.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all() and (planes.cpu().numpy() == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------------ 2. the engine
def _frame(hw, seed=0, kind="noise"):
    from videosd_amd.frames import I420Frame

    return I420Frame.from_planes(*Y.yuv_frame(hw, kind, seed=seed))


def _host_rgb(f, tw, th):
    """the RGB frame the existing path would be given: the contract's conversion of the whole frame, PIL's centre crop + LANCZOS resize"""
    from videosd_amd.pipeline import center_crop_resize

    return np.asarray(center_crop_resize(Image.fromarray(Y.contract_i420_to_rgb(f.y, f.u, f.v), "RGB"), tw, th))


@pytest.mark.parametrize("H,W", [(512, 512), (360, 640)])
def test_the_engine_takes_and_returns_i420_frames(H, W):
    from videosd_amd.frames import I420Frame

    eng = _engine(batch=1, H=H, W=W)
    for hw in [(720, 1280), (721, 1283)]:  # (721 x 1283 -> 360 x 640: a crop box with an odd left edge)
        f = _frame(hw, seed=H + hw[0])
        want = Y.contract_packed(eng.infer_u8(_host_rgb(f, W, H)))
        got = eng.infer_raw_i420(f)
        assert isinstance(got, I420Frame) and got.size == (W, H) and np.array_equal(got.data, want)
    if (H, W) == (360, 640):
        assert eng.ops.center_crop_box(1283, 721, W, H)[0] & 1 == 1
    same = _frame((H, W), seed=5)  # already the plan's size: converted straight into the input frame
    assert np.array_equal(eng.infer_raw_i420(same).data, Y.contract_packed(eng.infer_u8(Y.contract_i420_to_rgb(same.y, same.u, same.v))))
    with pytest.raises(ValueError):
        eng.infer_raw_i420(np.zeros((H, W, 3), np.uint8))
    eng3 = _engine(batch=3, H=H, W=W)
    fs = [_frame((720, 1280), seed=1), _frame((1080, 1920), seed=2), _frame((201, 301), seed=3)]
    want3 = eng3.infer_u8(np.stack([_host_rgb(x, W, H) for x in fs])).copy()
    got3 = eng3.infer_raw_i420(fs)
    assert len(got3) == 3
    for g, w_ in zip(got3, want3):
        assert np.array_equal(g.data, Y.contract_packed(w_))
    with pytest.raises(ValueError):
        eng3.infer_raw_i420(fs[:2])


# ------------------------------------------------------------------------------------------------------------------ 3. the class
@pytest.fixture(scope="module")
def pipes():
    from videosd_amd.pipeline import VideoSDPipeline

    return VideoSDPipeline(honor_ref_flag=True, **CFG), VideoSDPipeline(device_resize=True, honor_ref_flag=True, **CFG)


def _as_pil(f):
    return Image.fromarray(Y.contract_i420_to_rgb(f.y, f.u, f.v), "RGB")


def test_the_class_takes_i420_frames_and_leaves_pil_frames_alone(pipes):
    from videosd_amd.frames import I420Frame

    off, on = pipes
    f = _frame((720, 1280), seed=1)
    want = Y.contract_packed(np.asarray(off.infer(_as_pil(f), **OPTS)))
    for p in (off, on):  # (the I420 device path does not depend on `device_resize`)
        got = p.infer(f, **OPTS)
        assert isinstance(got, I420Frame) and got.size == (OPTS["width"], OPTS["height"]) and np.array_equal(got.data, want)
        m = p.metrics()
        assert m["stage_ms_p50"]["to_i420"] is not None
        assert m["io_bytes_per_frame"] == {"up": 960 * 720 * 3 // 2, "down": OPTS["width"] * OPTS["height"] * 3 // 2}  # the 960 x 720 crop box's planes alone
    # a mixed list through one launch: RGB comes down, the I420 caller's result is converted by the host loop -- the same bytes
    g = _frame((1080, 1920), seed=2)
    pil = Image.fromarray(Y.rgb_frame((720, 1280), "noise", seed=3), "RGB")
    want_mixed = off.infer_batch([_as_pil(f), pil, _as_pil(g)], **OPTS)
    for p in (off, on):
        got = p.infer_batch([f, pil, g], **OPTS)
        assert isinstance(got[0], I420Frame) and isinstance(got[1], Image.Image) and isinstance(got[2], I420Frame)
        assert np.array_equal(got[0].data, Y.contract_packed(np.asarray(want_mixed[0])))
        assert np.array_equal(np.asarray(got[1]), np.asarray(want_mixed[1]))
        assert np.array_equal(got[2].data, Y.contract_packed(np.asarray(want_mixed[2])))
    # an all-I420 list: the device converts every result
    want_all = off.infer_batch([_as_pil(f), _as_pil(g)], **OPTS)
    for a, b in zip(on.infer_batch([f, g], **OPTS), want_all):
        assert np.array_equal(a.data, Y.contract_packed(np.asarray(b)))
    # the fall-backs: a target that is no multiple of 8, and ref=True on objects that honour it
    o150 = dict(OPTS, height=100, width=150)
    a, b = on.infer(f, **o150), off.infer(_as_pil(f), **o150)
    assert a.size == (144, 96) and np.array_equal(a.data, Y.contract_packed(np.asarray(b)))
    r = dict(OPTS, ref=True)
    for fr in (_frame((720, 1280), seed=7), _frame((720, 1280), seed=8)):
        assert np.array_equal(on.infer(fr, **r).data, Y.contract_packed(np.asarray(off.infer(_as_pil(fr), **r))))
    # a PIL frame: exactly the earlier path and result, on both objects
    assert np.array_equal(np.asarray(on.infer(pil, **OPTS)), np.asarray(off.infer(pil, **OPTS)))
    assert isinstance(off.infer(pil, **OPTS), Image.Image)


# ------------------------------------------------------------------------------------------------------------------ 4. a real worker
def test_a_real_worker_takes_an_i420_frame_through_shared_memory(pipes):
    from videosd_amd.frames import I420Frame
    from videosd_amd.pipeline import VideoSDPipeline

    off, _on = pipes
    f = _frame((1080, 1920), seed=4)  # (3 110 400 bytes: fits the default 3 MiB slot, where the RGB frame does not)
    want = Y.contract_packed(np.asarray(off.infer(_as_pil(f), **OPTS)))  # (the contract around the RGB path, not the path under test)
    w = VideoSDPipeline.remote(**CFG)
    try:
        got = w.infer(f, **OPTS)
        assert isinstance(got, I420Frame) and got.size == (OPTS["width"], OPTS["height"]) and np.array_equal(got.data, want)
        assert w.host_s["frames"] == 1 and w.host_s["slot_write"] > 0.0
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the plan API
def test_a_c_host_feeds_i420_frames_to_a_plan(tmp_path):
    from videosd_amd import plan as P
    from videosd_amd.plan import CPlan, export_plan

    assert P.VERSION == 1 and not any("i420" in name for name in P.PLAN_FUNCS)  # plan files do not change
    H, W = 128, 96
    eng = _engine(batch=1, H=H, W=W)
    path = str(tmp_path / "frame.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    f = _frame((720, 1280), seed=11)
    try:
        want = eng.infer_raw_i420(f)
        assert np.array_equal(want.data, Y.contract_packed(eng.infer_u8(_host_rgb(f, W, H))))
        assert plan.infer_frame_i420(f) == want
        g = _frame((481, 643), seed=12)  # another camera size, odd: new tables, the same plan
        assert plan.infer_frame_i420(g) == eng.infer_raw_i420(g)
        same = _frame((H, W), seed=13)
        assert plan.infer_frame_i420(same) == eng.infer_raw_i420(same)
        assert plan.infer_frame_i420(f) == want
        with pytest.raises(ValueError):
            plan.infer_frame_i420([f, f])
    finally:
        plan.close()
    exe = str(tmp_path / "camera_host")
    libdir = os.path.join(ROOT, "videosd_amd")
    subprocess.run(["gcc", "-O2", os.path.join(ROOT, "examples", "camera_host.c"), "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lvsd",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    (tmp_path / "camera.yuv").write_bytes(f.data.tobytes())
    r = subprocess.run([exe, path, str(tmp_path / "camera.yuv"), "1280", "720", str(tmp_path / "out.yuv"), "2", "i420"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    assert "frames/s" in r.stdout and "I420" in r.stdout
    assert np.array_equal(np.frombuffer((tmp_path / "out.yuv").read_bytes(), dtype=np.uint8), want.data)


def test_a_plan_with_two_frames_per_launch_takes_i420_frames(tmp_path):
    from videosd_amd.plan import CPlan, export_plan

    H, W = 128, 96
    eng = _engine(batch=2, H=H, W=W)
    fs = [_frame((360, 640), seed=21), _frame((360, 640), seed=22)]
    path = str(tmp_path / "two.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    try:
        got = plan.infer_frame_i420(fs)
        want = eng.infer_raw_i420(fs)
        assert len(got) == 2 and got[0] == want[0] and got[1] == want[1]
    finally:
        plan.close()

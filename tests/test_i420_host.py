"""The I420 path without a GPU: the library's host loops of the colour contract (include/vsd.h vsd_i420_to_rgb_host / vsd_rgb_to_i420_host)
against the numpy statement of it in yuv_cases.py, byte for byte; the contract itself against real-valued BT.601 (the ONE tolerance
of this feature: 1 LSB, a property of the published integer formulas, not of the code under test); `frames.I420Frame`; and I420
frames through `RemotePipeline`'s shared-memory transport."""
import asyncio
import os
import pickle
import sys

import numpy as np
import pytest
from PIL import Image

import yuv_cases as Y

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["PYTHONPATH"] = os.path.dirname(os.path.abspath(__file__)) + os.pathsep + os.environ.get("PYTHONPATH", "")


@pytest.fixture(scope="module")
def lib():
    from videosd_amd import lib as L

    return L.load()


def _p(a):
    return a.ctypes.data


def _host_to_rgb(lib, y, u, v, ox=0, oy=0, pad=0):
    h, w = y.shape
    out = np.full((h, 3 * w + pad), 0xA5, np.uint8)
    assert y.strides[1] == 1 and u.strides[1] == 1 and u.strides[0] == v.strides[0]
    assert lib.vsd_i420_to_rgb_host(_p(y), y.strides[0], _p(u), _p(v), u.strides[0], ox, oy, h, w, _p(out), out.strides[0]) == 0
    assert (out[:, 3 * w:] == 0xA5).all()
    return out[:, :3 * w].reshape(h, w, 3)


@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("hw", Y.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_loop_to_rgb_is_the_contract_byte_for_byte(lib, hw, kind):
    y, u, v = Y.yuv_frame(hw, kind, seed=hw[0])
    want = Y.contract_i420_to_rgb(y, u, v)
    assert np.array_equal(_host_to_rgb(lib, y, u, v), want)
    # padded strides on every plane and on the destination
    assert np.array_equal(_host_to_rgb(lib, Y.padded(y, 5), Y.padded(u, 3), Y.padded(v, 3), pad=7), want)


@pytest.mark.parametrize("kind", Y.KINDS)
@pytest.mark.parametrize("hw", Y.EVEN_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_loop_to_i420_is_the_contract_byte_for_byte(lib, hw, kind):
    rgb = Y.rgb_frame(hw, kind, seed=hw[1])
    h, w = hw
    wy, wu, wv = Y.contract_rgb_to_i420(rgb)
    for pad in (0, 5):
        y = np.full((h, w + pad), 0xA5, np.uint8)
        u = np.full((h // 2, w // 2 + pad), 0xA5, np.uint8)
        v = np.full((h // 2, w // 2 + pad), 0xA5, np.uint8)
        assert lib.vsd_rgb_to_i420_host(_p(rgb), h, w, _p(y), _p(u), _p(v), y.strides[0], u.strides[0]) == 0
        assert np.array_equal(y[:, :w], wy) and np.array_equal(u[:, :w // 2], wu) and np.array_equal(v[:, :w // 2], wv)
        assert (y[:, w:] == 0xA5).all() and (u[:, w // 2:] == 0xA5).all() and (v[:, w // 2:] == 0xA5).all()


@pytest.mark.parametrize("hw", [(97, 131), (99, 100), (480, 640), (2, 3)], ids=lambda s: "%dx%d" % s)
def test_a_rectangle_with_the_right_parities_is_the_crop_of_the_converted_frame(lib, hw):
    y, u, v = Y.yuv_frame(hw, "noise", seed=7)
    whole = Y.contract_i420_to_rgb(y, u, v)
    h, w = hw
    for ox, oy in [(0, 0), (1, 0), (0, 1), (1, 1), (3, 5), (w - 1, h - 1), (w // 2, h // 3)]:
        if ox >= w or oy >= h:
            continue
        for rw, rh in [(w - ox, h - oy), (max(1, (w - ox) // 2), max(1, (h - oy) // 2)), (1, 1)]:
            ys, us, vs = y[oy:oy + rh, ox:ox + rw], u[oy >> 1:, ox >> 1:], v[oy >> 1:, ox >> 1:]
            want = whole[oy:oy + rh, ox:ox + rw]
            assert np.array_equal(Y.contract_i420_to_rgb(ys, us, vs, ox, oy), want)  # (the numpy statement agrees with itself)
            assert np.array_equal(_host_to_rgb(lib, ys, us, vs, ox, oy, pad=2), want)


def test_what_the_host_loops_do_not_support_is_refused(lib):
    from videosd_amd import lib as L

    y, u, v = Y.yuv_frame((4, 6))
    out = np.zeros((4, 18), np.uint8)
    assert lib.vsd_i420_to_rgb_host(None, 6, _p(u), _p(v), 3, 0, 0, 4, 6, _p(out), 18) == -1        # null plane
    assert lib.vsd_i420_to_rgb_host(_p(y), 5, _p(u), _p(v), 3, 0, 0, 4, 6, _p(out), 18) == -1      # short luma stride
    assert lib.vsd_i420_to_rgb_host(_p(y), 6, _p(u), _p(v), 3, 1, 0, 4, 6, _p(out), 18) == -1      # an odd left edge needs 4 chroma columns
    assert lib.vsd_i420_to_rgb_host(_p(y), 6, _p(u), _p(v), 3, 0, 0, 4, 6, _p(out), 17) == -1      # short destination rows
    assert lib.vsd_i420_to_rgb_host(_p(y), 6, _p(u), _p(v), 3, 0, 0, 4, L.RESAMPLE_MAX_SIDE + 1, _p(out), 1 << 20) == -1
    assert lib.vsd_i420_to_rgb_host(_p(y), 6, _p(u), _p(v), 3, 0, 0, 4, 6, _p(y), 18) == -1        # destination over a source plane
    rgb = np.zeros((4, 6, 3), np.uint8)
    assert lib.vsd_rgb_to_i420_host(_p(rgb), 3, 6, _p(y), _p(u), _p(v), 6, 3) == -1                # odd height
    assert lib.vsd_rgb_to_i420_host(_p(rgb), 4, 5, _p(y), _p(u), _p(v), 6, 3) == -1                # odd width
    assert lib.vsd_rgb_to_i420_host(_p(rgb), 4, 6, _p(y), _p(u), _p(v), 6, 2) == -1                # short chroma stride
    assert lib.vsd_rgb_to_i420_host(_p(rgb), 4, 6, _p(y), None, _p(v), 6, 3) == -1
    assert lib.vsd_rgb_to_i420_host(_p(rgb), 4, 6, _p(y), _p(u), _p(v), 6, 3) == 0


def test_the_integer_contract_is_within_one_lsb_of_real_valued_bt601():
    """All 2^24 (Y, U, V) triples: the published integer form against the real-valued studio-range BT.601 matrix, rounded half up and
    clamped.  True of the formulas alone; the differing share is reported (3-6 % of triples per channel)."""
    yy = np.arange(256, dtype=np.int64)[:, None, None]
    uu = np.arange(256, dtype=np.int64)[None, :, None]
    vv = np.arange(256, dtype=np.int64)[None, None, :]
    c, d, e = yy - 16, uu - 128, vv - 128
    integer = [(298 * c + 409 * e + 128) >> 8, (298 * c - 100 * d - 208 * e + 128) >> 8, (298 * c + 516 * d + 128) >> 8]
    k = 255.0 / 219.0
    real = [k * c + 1.596027 * e, k * c - 0.391762 * d - 0.812968 * e, k * c + 2.017232 * d]
    for name, a, b in zip("RGB", integer, real):
        a = np.clip(np.broadcast_to(a, (256, 256, 256)), 0, 255)
        b = np.clip(np.floor(np.broadcast_to(b, (256, 256, 256)) + 0.5), 0, 255).astype(np.int64)
        diff = np.abs(a - b)
        print(f"{name}: max |integer - real| = {int(diff.max())} LSB, differing in {100.0 * np.count_nonzero(diff) / diff.size:.2f} % of triples")
        assert diff.max() <= 1
    # the range statement of the other direction: black, white and the primaries
    for rgb, want in [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128))]:
        y, u, v = Y.contract_rgb_to_i420(np.full((2, 2, 3), rgb, np.uint8))
        assert (int(y[0, 0]), int(u[0, 0]), int(v[0, 0])) == want
    ext = [Y.contract_rgb_to_i420(np.full((2, 2, 3), [(i >> 0 & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255], np.uint8)) for i in range(8)]
    assert max(int(max(u.max(), v.max())) for _y, u, v in ext) == 240 and min(int(min(u.min(), v.min())) for _y, u, v in ext) == 16


# ------------------------------------------------------------------------------------------------------------------ I420Frame
class _PlaneBytes(bytes):
    """a bytes object with a `line_size`: the buffer protocol on every Python version"""
    line_size = 0


def _plane(plane, line_size):
    rows, cols = plane.shape
    buf = np.full((rows, line_size), 0x33, np.uint8)
    buf[:, :cols] = plane
    p = _PlaneBytes(buf.tobytes())
    p.line_size = line_size
    return p


class _Format:
    def __init__(self, name):
        self.name = name


class FakeAvFrame:
    """a stand-in for av.VideoFrame: `format.name`, `width`, `height`, `planes` with padded `line_size`"""

    def __init__(self, y, u, v, name="yuv420p", pad=32):
        self.format = _Format(name)
        self.height, self.width = y.shape
        self.planes = [_plane(y, y.shape[1] + pad), _plane(u, u.shape[1] + pad // 2), _plane(v, v.shape[1] + pad // 2)]


def test_i420frame_shapes_strides_layout_and_pickle():
    from videosd_amd.frames import I420Frame, is_i420

    for hw in [(97, 131), (99, 100), (1, 1), (2, 3), (480, 640)]:
        y, u, v = Y.yuv_frame(hw, "noise", seed=3)
        f = I420Frame.from_planes(Y.padded(y, 9), Y.padded(u, 4)[:, :], v[::1, ::1])
        h, w = hw
        assert f.size == (w, h) and f.y.shape == (h, w) and f.u.shape == f.v.shape == ((h + 1) // 2, (w + 1) // 2)
        assert f.data.size == h * w + 2 * f.u.size and f.data.flags.c_contiguous
        assert np.array_equal(f.y, y) and np.array_equal(f.u, u) and np.array_equal(f.v, v)
        g = pickle.loads(pickle.dumps(f))
        assert isinstance(g, I420Frame) and g == f and g.data is not f.data
        assert is_i420(f) and not is_i420(Image.new("RGB", (4, 4))) and not is_i420(np.zeros((4, 4, 3), np.uint8))
        if h % 2 == 0 and w % 2 == 0:
            a = f.to_ndarray()
            assert a.shape == (h * 3 // 2, w) and np.array_equal(a[:h], y)
            assert np.array_equal(a[h:].reshape(-1), np.concatenate([u.reshape(-1), v.reshape(-1)]))
        else:
            with pytest.raises(ValueError, match="even"):
                f.to_ndarray()
    # strided (non-contiguous) plane inputs: every second column of wider arrays
    y, u, v = Y.yuv_frame((6, 8))
    wide = [np.repeat(p, 2, axis=1) for p in (y, u, v)]
    assert I420Frame.from_planes(*[p[:, ::2] for p in wide]) == I420Frame.from_planes(y, u, v)
    with pytest.raises(ValueError, match="4:2:0"):
        I420Frame.from_planes(y, u[:, :-1], v[:, :-1])
    with pytest.raises(ValueError):
        I420Frame.from_planes(y.astype(np.uint16), u, v)


def test_i420frame_from_an_av_like_frame_and_what_it_refuses():
    from videosd_amd.frames import I420Frame, is_i420

    for hw in [(480, 640), (97, 131)]:
        y, u, v = Y.yuv_frame(hw, "gradient")
        av = FakeAvFrame(y, u, v)
        assert is_i420(av)
        f = I420Frame.from_av(av)
        assert f == I420Frame.from_planes(y, u, v)
    for name, why in [("yuvj420p", "full-range"), ("nv12", "semi-planar"), ("yuv444p", "4:4:4"), ("yuv420p10le", "8 bits"), ("rgb24", "not 8-bit planar")]:
        with pytest.raises(ValueError, match=why):
            I420Frame.from_av(FakeAvFrame(y, u, v, name=name))
    short = FakeAvFrame(y, u, v)
    short.planes[0] = _plane(y[:-1], y.shape[1] + 32)
    with pytest.raises(ValueError, match="does not hold"):
        I420Frame.from_av(short)


def test_i420frame_to_rgb_and_from_rgb_are_the_contract():
    from videosd_amd.frames import I420Frame

    y, u, v = Y.yuv_frame((97, 131), "noise", seed=9)
    assert np.array_equal(I420Frame.from_planes(y, u, v).to_rgb(), Y.contract_i420_to_rgb(y, u, v))
    rgb = Y.rgb_frame((96, 132), "noise", seed=9)
    assert np.array_equal(I420Frame.from_rgb(rgb).data, Y.contract_packed(rgb))
    assert np.array_equal(I420Frame.from_rgb(Image.fromarray(rgb, "RGB")).data, Y.contract_packed(rgb))
    with pytest.raises(ValueError, match="even"):
        I420Frame.from_rgb(rgb[:-1])


def test_the_class_sends_to_the_host_what_the_device_path_does_not_take():
    """VideoSDPipeline._i420_on_device (no GPU: the decision alone, as test_resample_host does for `_raw_frames`)"""
    from helpers_fake_pipeline import bare_pipeline
    from videosd_amd.frames import I420Frame

    class Ops:
        def i420_to_rgb(self): ...
        def rgb_to_i420(self): ...
        def resample_rgb(self): ...

    class Model:
        ops = Ops()

    p = bare_pipeline(model=Model(), honor_ref_flag=True, is_xl=False)
    f = I420Frame.from_planes(*Y.yuv_frame((97, 131)))
    assert p._i420_on_device([f], 512, 512, False) is True
    assert p._i420_on_device([f], 150, 100, False) is False          # not a multiple of 8: the second Lanczos step stays on the host
    assert p._i420_on_device([f], 512, 512, True) is False           # ref=True on an object that honours it
    p.honor_ref_flag = False
    assert p._i420_on_device([f], 512, 512, True) is True            # (accepted and ignored, as the reference does)
    assert p._i420_on_device([f], 32768, 512, False) is False        # a side above the limit
    Model.ops = object()
    assert p._i420_on_device([f], 512, 512, False) is False          # an ops object without the kernels


# ------------------------------------------------------------------------------------------------------------------ transport
class InvertPipeline:
    """TEST-ONLY stand-in with VideoSDPipeline's `infer` surface: an I420Frame comes back as `255 - plane`, a PIL image as
    helpers_fake_pipeline.FakePipeline returns it."""

    def __init__(self, **config):
        from helpers_fake_pipeline import FakePipeline

        self.pil = FakePipeline(**config)
        self.seen = []

    def infer(self, img, **opts):
        from videosd_amd.frames import I420Frame

        if isinstance(img, I420Frame):
            self.seen.append(("i420", img.size, bool(img.data.flags.owndata)))
            return I420Frame(255 - img.data, img.width, img.height)
        self.seen.append(("pil", img.size, True))
        return self.pil.infer(img, **opts)

    def kinds_seen(self):
        return list(self.seen)


INVERT = "test_i420_host:InvertPipeline"


def _remote(**kw):
    from videosd_amd.dispatch import RemotePipeline

    return RemotePipeline(factory=INVERT, model="m", controlnet="c", device=2, **kw)


def test_i420_frames_cross_through_shared_memory_and_pickled():
    from helpers_fake_pipeline import FakePipeline
    from videosd_amd.frames import I420Frame

    frames = [I420Frame.from_planes(*Y.yuv_frame(hw, "noise", seed=i)) for i, hw in enumerate([(480, 640), (97, 131), (1080, 1920)])]
    av = FakeAvFrame(*Y.yuv_frame((360, 640), "gradient"))
    pil = Image.fromarray(Y.rgb_frame((12, 16), "noise"), "RGB")
    want_pil = np.asarray(FakePipeline(model="m", controlnet="c", device=2).infer(pil, height=12, width=16))
    for slots in (8, 0):  # shared memory (the DEFAULT 3 MiB slot: a 1920 x 1080 I420 frame fits) | pickled
        p = _remote(shm_slots=slots)
        try:
            async def go():
                futs = [p.infer.remote(f) for f in frames] + [p.infer.remote(av)]
                return [await f for f in futs]

            outs = asyncio.run(go())
            for f, o in zip(frames, outs):
                assert isinstance(o, I420Frame) and o.size == f.size and np.array_equal(o.data, 255 - f.data)
                assert o.data.flags.owndata or o.data.base is not None  # (a copy: the reply slot is free again)
            assert outs[3] == I420Frame(255 - I420Frame.from_av(av).data, 640, 360)
            # a PIL frame sent to the same worker still comes back a PIL image with today's bytes
            got = p.infer(pil, height=12, width=16)
            assert isinstance(got, Image.Image) and np.array_equal(np.asarray(got), want_pil)
            seen = p.method("kinds_seen")()
            assert [k for k, _s, _o in seen] == ["i420"] * 4 + ["pil"]
            if slots:
                assert p.host_s["frames"] == 5                     # every frame came back through a slot ...
                assert not any(own for k, _s, own in seen if k == "i420")  # ... and reached the worker as views of one
            else:
                assert p.host_s["frames"] == 0
            with pytest.raises(ValueError, match="full-range"):
                p.infer(FakeAvFrame(*Y.yuv_frame((8, 8)), name="yuvj420p"))
            # a frame that is refused is refused before a slot is taken: none leaks
            short = FakeAvFrame(*Y.yuv_frame((8, 8)))
            short.planes[1] = _plane(Y.yuv_frame((8, 8))[1][:-1], 4 + 16)
            free = len(p._free_slots)
            for _ in range(slots + 2):
                with pytest.raises(ValueError, match="does not hold"):
                    p.infer(short)
            assert len(p._free_slots) == free
            assert p.infer(frames[1]) == I420Frame(255 - frames[1].data, *frames[1].size)
        finally:
            p.close()


def test_an_i420_frame_too_large_for_a_slot_travels_pickled():
    from videosd_amd.frames import I420Frame

    f = I420Frame.from_planes(*Y.yuv_frame((480, 640), "noise", seed=5))
    p = _remote(shm_slots=4, shm_slot_bytes=64 * 1024)
    try:
        o = p.infer(f)
        assert isinstance(o, I420Frame) and np.array_equal(o.data, 255 - f.data) and p.host_s["frames"] == 0
    finally:
        p.close()

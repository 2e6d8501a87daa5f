"""The host half of the device crop + LANCZOS resize (include/vsd.h vsd_center_crop_box, vsd_resample_table_host), without a GPU:
the crop box is Python's `int(round(.))` of the reference's float box, and the weight tables, applied by numpy integer code, give
exactly Pillow's bytes."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import resample_cases as R
from videosd_amd import lib as L
from videosd_amd.pipeline import center_crop_resize


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _box(lib, src_w, src_h, w, h):
    b = (C.c_int * 4)()
    assert lib.vsd_center_crop_box(src_w, src_h, w, h, b) == 0
    return tuple(b)


TARGETS = sorted({c[1] for c in R.CENTRE_CASES})  # (h, w) of every case: nine sizes


def test_the_crop_box_is_pythons_round_half_to_even_of_the_float_box(lib):
    assert len(TARGETS) >= 5
    ties = 0
    for th, tw in TARGETS:
        for sh in range(90, 141):
            for sw in range(90, 141):
                want = R.python_box(sw, sh, tw, th)
                assert _box(lib, sw, sh, tw, th) == want, (sw, sh, tw, th)
                nw = sh * (tw / th)
                ties += ((sw - nw) / 2) % 1 == 0.5
    assert ties > 100  # the sweep is full of boxes whose edges fall on .5
    assert _box(lib, 100, 97, 512, 512) == (2, 0, 98, 97)  # half to even, not half away from zero
    for (sh, sw), (th, tw), _ in R.CENTRE_CASES:
        assert _box(lib, sw, sh, tw, th) == R.python_box(sw, sh, tw, th)
    assert lib.vsd_center_crop_box(0, 10, 8, 8, (C.c_int * 4)()) == -1


@pytest.mark.parametrize("case", R.CENTRE_CASES, ids=R.case_id)
def test_the_tables_applied_in_integer_arithmetic_give_pillows_bytes(lib, case):
    (sh, sw), (th, tw), kind = case
    f = R.frame((sh, sw), kind)
    want = np.asarray(center_crop_resize(Image.fromarray(f, "RGB"), tw, th))
    got = R.resample_with_tables(lib, f, _box(lib, sw, sh, tw, th), (th, tw))
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", R.BOX_CASES, ids=R.case_id)
def test_an_explicit_box_that_skips_one_pass(lib, case):
    src, box, dst = case
    f = R.frame(src)
    assert np.array_equal(R.resample_with_tables(lib, f, box, dst), R.pillow_box_resize(f, box, dst))


def test_table_sizes_and_limits(lib):
    assert lib.vsd_resample_table_bytes(720, 512) == 4 * 512 * (2 + 11)  # scale 1.40625: support 4.22, ksize 11
    assert lib.vsd_resample_table_bytes(100, 200) == 4 * 200 * (2 + 7)   # upscale: the filter keeps its own support
    assert lib.vsd_resample_table_bytes(0, 8) == 0 and lib.vsd_resample_table_bytes(8, L.RESAMPLE_MAX_SIDE + 1) == 0
    assert lib.vsd_resample_table_bytes(L.RESAMPLE_MAX_SIDE, 8) > 0
    assert lib.vsd_resample_workspace_bytes(720, 512) == 720 * 512 * 3
    xmin, count, k = R.host_table(lib, 2160, 512)
    assert (xmin >= 0).all() and (count > 0).all() and (xmin + count <= 2160).all() and (count <= k.shape[1]).all()
    assert (np.abs(k.sum(axis=1) - (1 << 22)) <= k.shape[1]).all()  # every row sums to 1.0 up to the rounding of its weights


def test_which_frames_the_class_sends_down_the_device_path():
    """`device_resize=True`: RGB frames with a target size that is a multiple of 8 go to the kernel; everything else keeps the host path
    (other modes, other target sizes, sides the kernel refuses, ops objects without the kernel such as tests/fake_ops.py)."""
    from types import SimpleNamespace

    from helpers_fake_pipeline import bare_pipeline

    pipe = bare_pipeline(model=SimpleNamespace(ops=SimpleNamespace(resample_rgb=lambda *a: None)))
    rgb = Image.fromarray(R.frame((72, 128)), "RGB")
    raw = pipe._raw_frames([rgb, rgb], 64, 64)
    assert len(raw) == 2 and raw[0].shape == (72, 128, 3) and raw[0].dtype == np.uint8 and np.array_equal(raw[0], R.frame((72, 128)))
    assert pipe._raw_frames([rgb], 150, 100) is None                   # the second Lanczos step of a size that is no multiple of 8
    assert pipe._raw_frames([rgb, rgb.convert("RGBA")], 64, 64) is None
    assert pipe._raw_frames([rgb.convert("L")], 64, 64) is None
    assert pipe._raw_frames([Image.new("RGB", (L.RESAMPLE_MAX_SIDE + 1, 2))], 64, 64) is None
    pipe.model = SimpleNamespace(ops=SimpleNamespace())                  # an ops object without the kernel
    assert pipe._raw_frames([rgb], 64, 64) is None

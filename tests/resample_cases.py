"""The cases of the device crop + LANCZOS resize (tests/test_resample_host.py, tests/test_resample_gpu.py) and the few lines of numpy
integer code that apply a weight table the way Pillow's 8-bit resample does."""
import ctypes as C

import numpy as np
from PIL import Image

# (source h, w) -> (target h, w); seeded uniform random bytes unless the third entry says otherwise
CENTRE_CASES = [
    ((720, 1280), (512, 512), None),
    ((720, 1280), (1024, 1024), None),
    ((720, 1280), (720, 1280), None),  # identity
    ((480, 640), (360, 640), "bw"),    # saturating black / white frame
    ((1080, 1920), (512, 512), None),
    ((1080, 1920), (256, 256), None),
    ((2160, 3840), (512, 512), None),
    ((200, 300), (360, 640), None),    # upscale
    ((360, 640), (360, 640), None),
    ((721, 1283), (432, 768), None),
    ((97, 131), (512, 512), None),
    ((97, 100), (512, 512), None),     # box edges on .5: (2, 0, 98, 97)
    ((16, 16), (512, 512), None),
    ((99, 100), (64, 64), None),
    ((480, 640), (512, 512), None),
    ((1280, 720), (512, 512), None),   # portrait
    ((600, 800), (768, 768), None),
    ((1088, 1920), (576, 1024), None),
    ((9, 2000), (360, 640), None),
]
# an explicit box instead of the centre crop, so that one pass is skipped: (source h, w), box (l, t, r, b), (target h, w)
BOX_CASES = [
    ((720, 1280), (100, 0, 612, 720), (512, 512)),   # 512 wide already: vertical pass only
    ((720, 1280), (0, 0, 1000, 512), (512, 512)),    # 512 high already: horizontal pass only
]


def case_id(c):
    src, dst = c[0], (c[1] if len(c[1]) == 2 else c[2])
    return "%dx%d-to-%dx%d" % (src + dst) + ("-box%d" % c[1][0] if len(c[1]) == 4 else "")


def frame(src_hw, kind=None, seed=0):
    rng = np.random.default_rng(1000 + seed)
    f = rng.integers(0, 256, (src_hw[0], src_hw[1], 3), dtype=np.uint8)
    if kind == "bw":
        f = np.where(f > 127, 255, 0).astype(np.uint8)
    return f


def python_box(src_w, src_h, width, height):
    """The float box of pipeline.center_crop_resize (same expression order), then what PIL's Image.crop does with it."""
    if src_w / src_h > width / height:
        new_width = src_h * (width / height)
        box = ((src_w - new_width) / 2, 0, (src_w + new_width) / 2, src_h)
    else:
        new_height = src_w * (height / width)
        box = (0, (src_h - new_height) / 2, src_w, (src_h + new_height) / 2)
    return tuple(int(round(v)) for v in box)


def pillow_box_resize(f, box, dst_hw):
    return np.asarray(Image.fromarray(f, "RGB").crop(box).resize((dst_hw[1], dst_hw[0]), resample=Image.Resampling.LANCZOS))


def host_table(lib, n_in, n_out):
    """(xmin [out], count [out], k [out][ksize]) of vsd_resample_table_host"""
    nbytes = int(lib.vsd_resample_table_bytes(n_in, n_out))
    assert nbytes > 0 and nbytes % (4 * n_out) == 0
    ksize = nbytes // (4 * n_out) - 2
    xmin = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    assert lib.vsd_resample_table_host(n_in, n_out, p(xmin), p(count), p(k)) == ksize
    return xmin, count, k


def apply_table(img, table, axis):
    """One pass of Pillow's 8-bit resample along `axis` (0 = vertical, 1 = horizontal) of a uint8 [h][w][3] image:
    clamp((2^21 + sum pixel * k) >> 22, 0, 255) in 32-bit integers."""
    xmin, count, k = table
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + a.shape[1:], np.uint8)
    for i in range(len(xmin)):
        n = int(count[i])
        acc = (1 << 21) + np.tensordot(k[i, :n].astype(np.int64), a[xmin[i]:xmin[i] + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31  # (Pillow accumulates in a 32-bit int)
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resample_with_tables(lib, f, box, dst_hw):
    """crop + horizontal pass into 8 bits + vertical pass, a pass whose input length equals its output length skipped"""
    l, t, r, b = box
    img = f[t:b, l:r]
    if r - l != dst_hw[1]:
        img = apply_table(img, host_table(lib, r - l, dst_hw[1]), 1)
    if b - t != dst_hw[0]:
        img = apply_table(img, host_table(lib, b - t, dst_hw[0]), 0)
    return np.ascontiguousarray(img)

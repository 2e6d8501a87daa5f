"""TEST-ONLY helpers of the per-frame prompt tests: the copy list of `vsd_prompt_install` restated in numpy, stand-in networks that
give the prompt layouts something to lay out, and the op emulator with `prompt_install` (tests/fake_ops.py has none)."""
from types import SimpleNamespace

import numpy as np

from fake_ops import FakeOps

SENTINEL = 0xA5


def apply_segments(segs, src: np.ndarray, dst: np.ndarray, frame: int):
    """include/vsd.h vsd_prompt_seg, row by row: `rows` dense source rows of `row_bytes` to dst_off + frame * dst_frame_stride + row * dst_pitch"""
    for so, do, rows, rb, pitch, fstride in segs:
        for r in range(rows):
            d0 = do + frame * fstride + r * pitch
            dst[d0:d0 + rb] = src[so + r * rb:so + (r + 1) * rb]


def stub_nets(widths, absorbed_from=640):
    """objects with what PromptLayout / FramePromptLayout read of a NetWeights: one transformer block per width"""
    cfg = SimpleNamespace(heads_for=lambda c: 8)
    blocks = [SimpleNamespace(kv2=SimpleNamespace(n=2 * c), xa_raw=() if c >= absorbed_from else None) for c in widths]
    return [SimpleNamespace(transformers=blocks, cfg=cfg)]


def tensor_u16(buf: np.ndarray, item):
    """a layout item (offset, shape, fp16) of a byte buffer as a u16 array view"""
    off, shape, _dt = item
    n = shape[0] * shape[1] * 2
    return buf[off:off + n].view(np.uint16).reshape(shape)


def expected_install(src_lay, dst_lay, src: np.ndarray, dst_before: np.ndarray, frame: int) -> np.ndarray:
    """what the per-frame block must hold after installing `src` into slot `frame`, written from the LAYOUTS (tensor views), not the copy list"""
    want = dst_before.copy()
    tl, ldt = dst_lay.tl, dst_lay.ldt
    for key, item in dst_lay.items.items():
        s = tensor_u16(src, src_lay.items[key])
        d = tensor_u16(want, item)
        if key[2] == "k":
            d[frame * tl:(frame + 1) * tl] = s
        else:
            d[:, frame * ldt:(frame + 1) * ldt] = s
    return want


class FramePromptFakeOps(FakeOps):
    """the op emulator plus `prompt_install` (the numpy restatement above); counts the installs per frame slot"""

    def __init__(self):
        super().__init__()
        self.installs = []

    def prompt_install(self, src_buf, dst_buf, segs_dev, nseg, frame):
        assert 0 <= frame and tuple(segs_dev.shape) == (nseg, 6)
        self.installs.append(int(frame))
        apply_segments(segs_dev.tolist(), src_buf.numpy(), dst_buf.numpy(), int(frame))

    def clone(self, lane=None):
        return FramePromptFakeOps()

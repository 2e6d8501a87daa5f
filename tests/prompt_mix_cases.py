"""TEST-ONLY helpers of the prompt-mix tests: THE PROMPT MIX of include/vsd.h restated in numpy, written from the header's text and not from
the kernel (every fp32 product and fma is evaluated in fp64 and rounded ONCE, which is what IEEE asks of the fp32 operation: the exact
product of two fp32 numbers fits in fp64, and the exact fp32 product plus an fp32 addend, rounded to fp64 and then to fp32, gives the
rounding of the exact value but for double-rounding ties that `_fma32` resolves exactly), awkward segment lists, and the op emulator
with `prompt_mix` (tests/fake_ops.py has none)."""
from fractions import Fraction

import numpy as np

from frame_option_cases import FrameOptionFakeOps

SENTINEL = 0xA5
F16, F32, COPY = 0, 1, 2  # include/vsd.h VSD_MIX_*


def _fma32(w, x, acc):
    """fp32 fma(w, x, acc), elementwise: w * x is exact in fp64 (24 + 24 bits), the sum is rounded to fp64 and then to fp32; where that
    second rounding lands on a tie of fp32 (the fp64 sum lies exactly half-way between two fp32 numbers although the exact sum does not,
    or the other way round) the element is recomputed with exact rationals."""
    p = w.astype(np.float64) * x.astype(np.float64)
    s = p + acc.astype(np.float64)
    out = s.astype(np.float32)
    # an fp64 whose low 29 bits are 0x10000000 sits exactly half-way between two fp32 values (normal range): recompute those exactly
    # (only where the fp64 sum was itself rounded -- the error term of Knuth's TwoSum is not zero: an exact half-way sum is a true tie,
    #  which the conversion above has already sent to even)
    a64 = acc.astype(np.float64)
    t = s - p
    inexact = ((p - (s - t)) + (a64 - t)) != 0.0
    bits = np.ascontiguousarray(s).view(np.uint64)
    tie = np.flatnonzero(((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & np.isfinite(s) & inexact)
    for i in tie:
        exact = Fraction(float(w[i])) * Fraction(float(x[i])) + Fraction(float(acc[i]))
        lo, hi = np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))
        best = min((out[i], lo, hi), key=lambda c: (abs(Fraction(float(c)) - exact), int(np.float32(c).view(np.uint32)) & 1))
        out[i] = best
    return out


def mix_elements(weights, xs, kind):
    """the element arithmetic of the contract on flat arrays: xs[i] the elements of component i (fp16 or fp32 by `kind`)"""
    n = len(xs)
    if n == 1 or kind == COPY:
        return xs[0].copy()
    w = [np.float32(v) for v in weights]
    x = [a.astype(np.float32) for a in xs]
    acc = (np.full(x[0].shape, w[0], np.float64) * x[0].astype(np.float64)).astype(np.float32)  # one fp32 multiply (exact in fp64, one rounding)
    for i in range(1, n):
        acc = _fma32(np.full(x[i].shape, w[i], np.float32), x[i], acc)
    return acc.astype(np.float16) if kind == F16 else acc


def mix_numpy(srcs, weights, dst, segs, frame):
    """include/vsd.h vsd_mix_seg, row by row, into the byte array `dst` (in place)"""
    for so, do, rows, rb, pitch, fstride, kind, _res in segs:
        dt = np.float32 if kind == F32 else np.float16
        for r in range(rows):
            xs = [s[so + r * rb:so + (r + 1) * rb].view(np.uint8 if kind == COPY else dt) for s in srcs]
            d0 = do + frame * fstride + r * pitch
            dst[d0:d0 + rb] = mix_elements(weights, xs, kind).view(np.uint8)
    return dst


def finite_block(rng, nbytes, segs):
    """`nbytes` of source data: random bytes where nothing computes (copy segments, the gaps), finite fp16 / fp32 values of mixed magnitude
    (with subnormals, zeros and negative zeros among them) where a segment mixes"""
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    for so, _do, rows, rb, _p, _f, kind, _r in segs:
        if kind == COPY:
            continue
        n = rows * rb // (4 if kind == F32 else 2)
        v = rng.standard_normal(n) * np.exp2(rng.integers(-18 if kind == F16 else -30, 4, n))
        v[rng.integers(0, n, max(1, n // 50))] = 0.0
        v[rng.integers(0, n, max(1, n // 50))] = -0.0
        buf[so:so + rows * rb] = v.astype(np.float32 if kind == F32 else np.float16).view(np.uint8)
    return buf


def awkward_segments(B=3):
    """-> (segments, source bytes, destination bytes): a per-frame destination of B slots with one-chunk rows, a pitched fp16 segment (the
    V^T columns of a slot: rows of 64 bytes at pitch B * 64), an fp32 run, a copy segment, a long fp16 run that is no multiple of a
    workgroup's stride, and gaps between them that nothing may touch"""
    segs, so, do = [], 0, 0

    def add(rows, rb, kind, gap=16):
        nonlocal so, do
        segs.append((so, do, rows, rb, B * rb, rb, kind, 0))
        so += rows * rb + gap
        do += rows * B * rb + gap

    add(5, 16, F16)            # one-chunk rows
    add(7, 64, F16, gap=48)    # pitched: 7 rows of 4 chunks
    add(1, 80, F32)            # an fp32 run
    add(1, 32, COPY)           # the prompt-independent item
    add(3, 16, F32, gap=32)    # fp32, one-chunk rows
    add(1, 16 * (32 * 256 * 4 + 37), F16)  # more chunks than one pass of the whole grid (MX_BLOCKS_X * MX_THREADS * MX_UNROLL), odd tail
    add(300, 48, F16)          # rows of 3 chunks: a grid stride is no whole number of rows
    return segs, so, do


def whole_segments(segs):
    """the same items as one block of the sources' own layout (every item one run in place): the destination of a default engine"""
    return [(so, so, 1, rows * rb, rows * rb, rows * rb, kind, 0) for so, _do, rows, rb, _p, _f, kind, _r in segs]


class PromptMixFakeOps(FrameOptionFakeOps):
    """the op emulator plus `prompt_mix` (the numpy restatement above); records every mix as (components, weights, frame) and counts the
    copies and synchronises, so that a test can see what a launch cost"""

    def __init__(self):
        super().__init__()
        self.mixes, self.copies, self.syncs = [], 0, 0

    def clone(self, lane=None):
        return PromptMixFakeOps()

    def copy_(self, dst, src):
        self.copies += 1
        super().copy_(dst, src)

    def synchronize(self):
        self.syncs += 1

    def prompt_mix_table(self, segs_dev, nseg):
        assert tuple(segs_dev.shape) == (nseg, 8)

    def prompt_mix(self, src_bufs, weights, dst_buf, segs_dev, nseg, frame=0):
        assert 1 <= len(src_bufs) == len(weights) <= 4 and tuple(segs_dev.shape) == (nseg, 8)
        self.mixes.append((tuple(b.data_ptr() for b in src_bufs), tuple(weights), int(frame)))
        mix_numpy([b.numpy() for b in src_bufs], weights, dst_buf.numpy(), segs_dev.tolist(), int(frame))


def mini_pipeline(**config):
    """factory of a worker process (`RemotePipeline(factory="prompt_mix_cases:mini_pipeline")`): VideoSDPipeline on the MINI topologies
    with synthetic weights, as tests/test_frame_prompts_gpu.py `_pipeline` builds it in the test's own process"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    Cf.SD15_UNET, Cf.SD15_CONTROLNET = Cf.MINI_UNET, Cf.MINI_CONTROLNET  # (this process only: a worker is spawned, not forked)
    return VideoSDPipeline(**config)

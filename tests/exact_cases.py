"""Exact-arithmetic cases (tests/test_exact_host.py, tests/test_exact_gpu.py): inputs for which every intermediate value of a conv /
GEMM launch is exactly representable, so that the right answer is known to the bit.

Activations are non-zero integers in {+-1, +-2, +-3}, weights non-zero integers in {+-1, +-2}, bias / rowvec / residuals / add2 small
integers (a `big` case: bias magnitudes of 1900..2040, so that outputs pass 2048 where fp16 has a spacing of 2 and every odd value is
a tie), out_scale a power of two.  Every product is exact, every partial sum is an integer (or half-integer) below 2^24 -- exact in
fp32 in ANY order, split over K or not, fused multiply-add or not -- and the one rounding left is fp32 -> fp16 at the store.  The
expected output is fp16(exact arithmetic), computed here in float64 (every value an integer far below 2^53: exact), and compared with
torch.equal.  No operand is zero: each of the K products of each output changes the answer when it is dropped, duplicated or taken
from the neighbouring pixel or channel.  tests/test_exact_host.py checks these conditions for every case of the table.

Also here: numpy statements of the small elementwise kernels' arithmetic (include/vsd.h and the comments of csrc/elementwise.hip)."""
import dataclasses
import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

ACT_NONE, ACT_RELU, ACT_POST = 0, 1, 256
SENTINEL = 0.3330078125  # fp16; no case can produce it (outputs are integers or half-integers)

# ---------------------------------------------------------------------------------------------------------------- the cases
# A kernel form is (tile, pipeline, split_k, reduce in the launch); (None, None, None, True) = whatever the heuristic picks.
T128x128, T128x64, T64x64, T64x128, T256x128, T256x64, T256x256 = range(7)


@dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    c0: int                                  # real channels of src0 (stored padded to cin_pad when that is set)
    cout: int
    c1: int = 0
    ksize: int = 3
    stride: int = 1
    up: Optional[Tuple[int, int]] = None      # folded nearest resize to (hi, wi)
    batch: int = 1
    cin_pad: Optional[int] = None
    bias: bool = True
    rowvec: bool = False
    residual: bool = False
    residual2: bool = False
    out_scale: float = 1.0
    scale_dev: bool = False                   # out_scale through out_scale_dev
    act: int = ACT_NONE
    out2: bool = False
    t_col0: Optional[int] = None              # columns >= t_col0 go to out_t
    t_img: int = 0
    rowstat: bool = False
    chanstat: bool = False
    big: bool = False                         # bias magnitudes 1900..2040: outputs beyond 2048
    thin: bool = False                        # pipeline 10's Cout <= 8 form: ldo = 8, padding channels written as zeros
    forms: tuple = ((None, None, None, True),)
    data: str = ""                            # cases of one geometry that share their tensors name the same data

    @property
    def cin(self):
        return (self.cin_pad or self.c0) + self.c1

    @property
    def hi_wi(self):
        return self.up if self.up is not None else (self.h, self.w)

    @property
    def ho_wo(self):
        hi, wi = self.hi_wi
        pad = self.ksize // 2
        return (hi + 2 * pad - self.ksize) // self.stride + 1, (wi + 2 * pad - self.ksize) // self.stride + 1

    @property
    def m(self):
        ho, wo = self.ho_wo
        return self.batch * ho * wo

    @property
    def k(self):
        return self.ksize * self.ksize * self.cin

    @property
    def ldo(self):
        return 8 if self.thin else (self.cout + 7) // 8 * 8 + 8  # (at least 8 padding columns that must stay untouched)

    @property
    def ldr(self):
        return (self.cout + 7) // 8 * 8


def _forms(tiles, pipelines, splits):
    """every (tile, pipeline) at every split; a split launch runs with both reducers (in-launch `counters`, splitk_reduce)"""
    out = []
    for t in tiles:
        for p in pipelines:
            for s in splits:
                out += [(t, p, s, True)] + ([(t, p, s, False)] if s > 1 else [])
    return tuple(out)


_BASE = dict(h=18, w=14, c0=128, cout=200, rowvec=True, residual=True, big=True)   # M = 252, N = 200, K = 1152: ragged for every tile
_EPI_FORMS = ((T64x64, 3, 1, True), (T128x128, 3, 1, True), (T64x64, 3, 3, True), (T128x128, 3, 3, True))
_MIX = ((T64x64, 3, 1, True), (T128x128, 5, 3, True), (T128x64, 0, 3, False), (T64x128, 4, 1, True), (T128x128, 8, 1, True))
_MIX_HALO = _MIX + ((T128x64, 7, 1, True), (T256x64, 7, 2, True))
_MIX_GATHER = ((T64x64, 3, 1, True), (T128x128, 0, 1, True), (T64x128, 5, 3, True), (T128x64, 4, 3, False))  # (stride 2 / resize: no buffer-load path)
_SHORT = ((T64x64, 3, 1, True), (T128x128, 5, 1, True), (T128x64, 0, 1, True), (T64x128, 4, 1, True), (T128x128, 9, 1, True))

CASES = [
    # ---- base geometry: 3x3 stride 1, 18 x 14 pixels, 128 -> 200 channels, bias + rowvec + residual
    Case("base-four-wave", **_BASE, data="base", forms=_forms((0, 1, 2, 3), (0, 3, 4, 5, 6), (1, 3))),
    Case("base-eight-wave", **_BASE, data="base", forms=_forms((T128x128, T256x128), (8, 9), (1, 3)) + _forms((T256x256,), (8, 9), (1,))),
    Case("base-halo", **_BASE, data="base", forms=_forms((T128x128, T128x64, T256x128, T256x64), (7,), (1, 2))),
    # ---- the persistent 64-channel form (pipeline 10)
    Case("c64-37x50-b2", h=37, w=50, c0=64, cout=64, batch=2, residual=True, big=True, forms=((T256x64, 10, 1, True),)),
    Case("c64-16x24-up32x48", h=16, w=24, c0=64, cout=64, up=(32, 48), residual=True, forms=((T256x64, 10, 1, True),)),
    Case("c64-thin-n3", h=37, w=50, c0=64, cout=3, batch=2, thin=True, forms=((T256x64, 10, 1, True),)),
    Case("c64-thin-n4", h=16, w=24, c0=64, cout=4, up=(32, 48), thin=True, forms=((T256x64, 10, 1, True),)),
    # ---- short and deep K
    Case("k64-1x1", h=9, w=11, c0=64, cout=72, ksize=1, rowvec=True, forms=_SHORT),
    Case("k128-1x1", h=9, w=11, c0=128, cout=72, ksize=1, rowvec=True, forms=_SHORT + ((T64x64, 3, 2, True), (T64x64, 3, 2, False))),
    Case("k320-1x1", h=9, w=11, c0=320, cout=72, ksize=1, rowvec=True, forms=_SHORT + ((T64x64, 5, 3, True), (T128x64, 3, 3, False))),
    Case("k23040-concat", h=8, w=8, c0=1280, c1=1280, cout=1280, rowvec=True, residual=True),  # (the heuristic's own tile and split)
    # ---- operand gathering: concat
    Case("concat-128+64-3x3", h=18, w=14, c0=128, c1=64, cout=200, residual=True, big=True, forms=_MIX_HALO),
    Case("concat-64+128-3x3", h=18, w=14, c0=64, c1=128, cout=200, residual=True, forms=_MIX_HALO),
    Case("concat-128+64-1x1", h=18, w=14, c0=128, c1=64, cout=200, ksize=1, residual=True, forms=_MIX),
    Case("concat-64+128-1x1", h=18, w=14, c0=64, c1=128, cout=200, ksize=1, residual=True, big=True, forms=_MIX),
    # ---- stride 2
    Case("stride2-27x48", h=27, w=48, c0=128, cout=72, stride=2, residual=True, forms=_MIX_GATHER),
    Case("stride2-7x12", h=7, w=12, c0=128, cout=72, stride=2, residual=True, forms=_MIX_GATHER),
    Case("stride2-1x1px", h=1, w=1, c0=128, cout=72, stride=2, residual=True, forms=_MIX_GATHER),
    # ---- folded nearest resize
    Case("resize-7x12-14x24", h=7, w=12, c0=128, cout=72, up=(14, 24), residual=True, forms=_MIX_GATHER + ((T128x64, 7, 1, True),)),
    Case("resize-14x24-27x48", h=14, w=24, c0=128, cout=72, up=(27, 48), residual=True, forms=_MIX_GATHER + ((T256x64, 7, 2, True),)),
    Case("resize-4x4-8x8", h=4, w=4, c0=128, cout=72, up=(8, 8), residual=True, forms=_MIX_GATHER + ((T128x128, 7, 2, False),)),
    # ---- the generic small-channel operand path / thin outputs through the GEMM tiles
    Case("generic-3-64", h=18, w=14, c0=3, cin_pad=8, cout=64, residual=True, forms=_forms((T64x64, T128x128), (0, 3, 5), (1,))),
    Case("generic-4-320", h=18, w=14, c0=4, cin_pad=8, cout=320, residual=True, forms=_forms((T64x64, T128x64), (0, 3, 5), (1,))),
    Case("generic-64-3", h=18, w=14, c0=64, cout=3, residual=True, forms=_forms((T64x64, T128x64), (0, 3, 5), (1,))),
    Case("generic-320-4", h=18, w=14, c0=320, cout=4, residual=True, forms=_forms((T64x64,), (0, 3, 5), (1, 3))),
    # ---- batch: three images, each with its own border
    Case("batch3-stride1", h=18, w=14, c0=128, cout=200, batch=3, residual=True, big=True, forms=_MIX_HALO),
    Case("batch3-stride2", h=18, w=14, c0=128, cout=200, batch=3, stride=2, residual=True, forms=_MIX_GATHER),
    Case("batch3-resize", h=9, w=7, c0=128, cout=200, batch=3, up=(18, 14), residual=True, forms=_MIX_GATHER + ((T128x64, 7, 1, True),)),
    Case("batch3-out_t", h=18, w=14, c0=128, cout=200, batch=3, rowvec=True, t_col0=128, t_img=256, forms=_EPI_FORMS + ((T64x64, 0, 3, False),)),
    # ---- the linear epilogue, part by part (tile 64x64 and 128x128, unsplit and split 3)
    Case("epi-residual2", **_BASE, residual2=True, forms=_EPI_FORMS),
    Case("epi-scale-0.5", **_BASE, out_scale=0.5, forms=_EPI_FORMS),
    Case("epi-scale-2", **_BASE, out_scale=2.0, forms=_EPI_FORMS),
    Case("epi-scale-dev-0.5", **_BASE, out_scale=0.5, scale_dev=True, forms=_EPI_FORMS),
    Case("epi-relu", **_BASE, act=ACT_RELU, forms=_EPI_FORMS),
    Case("epi-relu-post", **_BASE, act=ACT_RELU | ACT_POST, forms=_EPI_FORMS),
    Case("epi-out2", **_BASE, out2=True, forms=_EPI_FORMS),
    Case("epi-out2-n196", **{**_BASE, "cout": 196}, out2=True, forms=_EPI_FORMS),   # (a last chunk of 4 columns: the scalar tail of the store)
    Case("epi-out_t", h=18, w=14, c0=128, cout=200, rowvec=True, big=True, t_col0=128, forms=_EPI_FORMS),
    Case("epi-rowstat", h=18, w=14, c0=128, cout=192, rowvec=True, residual=True, rowstat=True, forms=_EPI_FORMS),
    Case("epi-chanstat", h=18, w=14, c0=128, cout=200, rowvec=True, residual=True, chanstat=True, forms=_EPI_FORMS),
]
# Left out, with the sentence of include/vsd.h that refuses the combination:
#   - tile 256x128 on pipelines 0, 4, 6 and tile 256x64 off the halo form: "VSD_TILE_256x128 = 4 /* Cin % 64 == 0, no resize, pipeline 3, 5
#     or 7 only */, VSD_TILE_256x64 = 5 /* pipeline 7 (halo patch) only */" (pipelines 8 / 9: "tiles of 128x128 and larger").
#   - tile 256x256 split over K or with chanstat_out: "VSD_TILE_256x256 = 6 /* eight waves (pipeline 8 or 9), Cin % 64 == 0, no resize,
#     unsplit, no chanstat_out */".
#   - pipelines 8 / 9 on 64-row or 64-column tiles, with a resize or Cin % 64 != 0: "8 / 9 = the 3-stage ring
#     ... on eight waves (tiles of 128x128 and larger, buffer-load path)".
#   - the halo form with stride 2, 1x1 layers, residual2, out2, out_t, out_scale != 1, statistics: "7 = halo patch: 3x3 stride-1 convs
#     only (Cin % 64 == 0 per source, tile 128x128, 128x64, 256x128 or 256x64, plain epilogue)"; with out_scale_dev: "General epilogue only
#     (not the halo-patch form)".
#   - pipeline 10 split over K, with Cout other than 64 or <= 8, a residual on the thin form: "10 = the persistent form for 3x3
#     stride-1 convs with Cin = Cout = 64 from one source (... tile 256x64, unsplit, plain epilogue)".
#   - rowstat_out at Cout = 200: "fp32 [M][n/64][2]: ... over each 64-column group" (the row-statistics case runs at Cout = 192).
#   - chanstat_out with batch > 1: "per output CHANNEL ... over all M rows".
#   - a group on tiles of 256 rows, pipelines 0 / 4 / 6 / 7 / 10 or the generic path: "the same tile (64x64, 64x128, 128x64 or 128x128)
#     and pipeline (3 or 5), the buffer-load operand path (Cin % 64 == 0 per source, no resize)".
# The residual of a case with out_t is left out: the header's epilogue line does not say whether transposed columns take it (the
# kernels do not add it there; the networks never ask).

# one vsd_conv_gemm_group of three members of different M; every member in each of these forms (tile, split, in-launch, pipeline)
GROUP_MEMBERS = [
    Case("group-a-1x1", h=18, w=14, c0=128, cout=200, ksize=1, residual=True, out_scale=0.5, scale_dev=True, big=True),
    Case("group-b-3x3", h=9, w=11, c0=64, cout=72, rowvec=True),
    Case("group-c-1x1", h=5, w=7, c0=320, cout=136, ksize=1, residual=True, act=ACT_RELU),
]
GROUP_FORMS = [(T64x64, 1, True, 3), (T128x128, 3, True, 5), (T128x64, 3, False, 3), (T128x128, 1, True, 9)]
# one ops.pair of twin layers (one shape, two weight sets)
PAIR_MEMBERS = [Case("pair-a", **_BASE), Case("pair-b", **_BASE)]

ALL_CASES = CASES + GROUP_MEMBERS + PAIR_MEMBERS
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------- the lattices
def _choice(rng, values, shape):
    return np.asarray(values, dtype=np.int16)[rng.integers(0, len(values), size=shape)]


def _signed(rng, lo, hi, shape):
    """non-zero integers with magnitudes lo..hi"""
    return (rng.integers(lo, hi + 1, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)).astype(np.int16)


@dataclass
class Data:
    src: list            # per source: int16 [batch][h][w][stored channels] (padding channels of cin_pad zero)
    weight: np.ndarray   # int16 [cout][c0 + c1][k][k]: the conv weight as the networks hold it (packing.pack_conv packs it)
    bias: Optional[np.ndarray]
    rowvec: Optional[np.ndarray]
    residual: Optional[np.ndarray]    # int16 [M][ldr]
    residual2: Optional[np.ndarray]
    add2: Optional[np.ndarray]        # int16 [M][ldo]


def _key(case):
    return dataclasses.replace(case, name=case.data or case.name, forms=(), data="")


@functools.lru_cache(maxsize=None)
def _data(key) -> Data:
    c = key
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    src = []
    for ch, stored in ((c.c0, c.cin_pad or c.c0), (c.c1, c.c1)):
        if ch:
            x = np.zeros((c.batch, c.h, c.w, stored), dtype=np.int16)
            x[..., :ch] = _choice(rng, (-3, -2, -1, 1, 2, 3), (c.batch, c.h, c.w, ch))
            src.append(x)
    weight = _choice(rng, (-2, -1, 1, 2), (c.cout, c.c0 + c.c1, c.ksize, c.ksize))
    bias = None
    if c.bias:
        bias = _signed(rng, 1, 8, c.cout)
        if c.big:
            bias = np.where(np.arange(c.cout) % 2 == 0, _signed(rng, 1900, 2040, c.cout), bias).astype(np.int16)
    rowvec = _signed(rng, 1, 8, c.cout) if c.rowvec else None
    residual = _signed(rng, 1, 64, (c.m, c.ldr)) if c.residual else None
    residual2 = _signed(rng, 1, 64, (c.m, c.ldr)) if c.residual2 else None
    add2 = _signed(rng, 1, 32, (c.m, c.ldo)) if c.out2 else None
    return Data(src, weight, bias, rowvec, residual, residual2, add2)


def data(case) -> Data:
    return _data(_key(case))


# ---------------------------------------------------------------------------------------------------------------- the reference
def gather(case, src) -> np.ndarray:
    """A [M][K] of the descriptor: channel concat, nearest resize to (hi, wi), zero padding, stride, every image with its own border;
    k = (ky, kx, c)."""
    x = np.concatenate(src, axis=-1)
    hi, wi = case.hi_wi
    x = x[:, (np.arange(hi) * case.h) // hi][:, :, (np.arange(wi) * case.w) // wi]
    pad, ks, st = case.ksize // 2, case.ksize, case.stride
    x = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    ho, wo = case.ho_wo
    taps = [x[:, ky:ky + st * (ho - 1) + 1:st, kx:kx + st * (wo - 1) + 1:st, :] for ky in range(ks) for kx in range(ks)]
    return np.concatenate(taps, axis=-1).reshape(case.m, case.k)


def weight_matrix(case, weight) -> np.ndarray:
    """[cout][K] with k = (ky, kx, c), the first source's channels padded to cin_pad"""
    w = weight.transpose(0, 2, 3, 1)
    if case.cin_pad:
        w = np.pad(w, ((0, 0), (0, 0), (0, 0), (0, case.cin_pad - case.c0)))
    return w.reshape(case.cout, case.k)


@dataclass
class Ref:
    exact: np.ndarray                 # float64 [M][cout]: v before the store (columns >= t_col0: the transposed columns' v)
    bound: np.ndarray                 # float64 [M][cout]: sum |a w| and the epilogue's terms -- the largest partial sum there can be
    out: np.ndarray                   # fp16 [M][cout]
    out2: Optional[np.ndarray]
    rowstat: Optional[np.ndarray]     # float64 [M][cout / 64][2]
    chanstat: Optional[np.ndarray]    # float64 [cout][2]


@functools.lru_cache(maxsize=None)
def _reference(key) -> Ref:
    c, d = key, _data(key)
    a = gather(c, d.src).astype(np.float64)
    w = weight_matrix(c, d.weight).astype(np.float64)
    v = a @ w.T                      # (integers below 2^24: float64 holds every partial sum exactly)
    bound = np.abs(a) @ np.abs(w).T
    for vec in (d.bias, d.rowvec):
        if vec is not None:
            v = v + vec
            bound = bound + np.abs(vec)
    if c.act == ACT_RELU:
        v = np.maximum(v, 0.0)
    v = v * c.out_scale
    bound = bound * max(c.out_scale, 1.0)
    t0 = c.cout if c.t_col0 is None else c.t_col0
    for r in (d.residual, d.residual2):
        if r is not None:
            v[:, :t0] += r[:, :t0]
            bound[:, :t0] += np.abs(r[:, :t0])
    if c.act == ACT_RELU | ACT_POST:
        v = np.maximum(v, 0.0)
    with np.errstate(over="ignore"):
        out = v.astype(np.float16)   # (numpy rounds float64 -> fp16 once, to nearest even)
    out2 = None
    if c.out2:
        out2 = (out.astype(np.float64) + d.add2[:, :c.cout]).astype(np.float16)  # out2 = out + add2: of the STORED out
        bound = bound + np.abs(d.add2[:, :c.cout])
    o = out.astype(np.float64)
    rowstat = chanstat = None
    if c.rowstat:
        g = o.reshape(c.m, c.cout // 64, 64)
        rowstat = np.stack([g.sum(-1), (g * g).sum(-1)], axis=-1)
    if c.chanstat:
        chanstat = np.stack([o.sum(0), (o * o).sum(0)], axis=-1)
    return Ref(v, bound, out, out2, rowstat, chanstat)


def reference(case) -> Ref:
    return _reference(_key(case))


def transposed(case, ref_out) -> np.ndarray:
    """what out_t holds: fp16 [cout - t_col0][ldt], image b's row m at column b * t_img + m, the SENTINEL everywhere else"""
    ho, wo = case.ho_wo
    hw = ho * wo
    t_img = case.t_img or hw
    ldt = (case.batch * t_img + 7) // 8 * 8
    t = np.full((case.cout - case.t_col0, ldt), SENTINEL, dtype=np.float16)
    for b in range(case.batch):
        t[:, b * t_img:b * t_img + hw] = ref_out[b * hw:(b + 1) * hw, case.t_col0:].T
    return t


# ---------------------------------------------------------------------------------------------------------------- small kernels
F32 = np.float32


def postprocess_patterns():
    """fp16 [65536][3]: channel c of pixel i holds bit pattern (i + 21845 c) mod 65536 -- every pattern in every channel position"""
    i = np.arange(65536, dtype=np.int64)
    return np.stack([((i + 21845 * c) % 65536).astype(np.uint16) for c in range(3)], axis=1).view(np.float16)


def postprocess_chain(x16) -> np.ndarray:
    """vsd_postprocess_rgb: y = fp16(2c - 1), z = fp16(y / 2 + 0.5), clamp to [0, 1] (a NaN clamps to 0), * 255 in fp32, rounded half to even"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x16.astype(F32) * F32(2) - F32(1)).astype(np.float16)
        z = (y.astype(F32) * F32(0.5) + F32(0.5)).astype(np.float16)
        f = np.fmin(np.fmax(z.astype(F32), F32(0)), F32(1))  # (fmax / fmin return the other operand for a NaN)
        return np.rint(f * F32(255)).astype(np.uint8)


def preprocess_chain(u8) -> np.ndarray:
    """vsd_preprocess_rgb: u / 255 in fp32 -> fp16(2x - 1) -> fp16(+ 1) -> fp16(* 0.5)"""
    x = u8.astype(F32) / F32(255)
    y = (F32(2) * x - F32(1)).astype(np.float16)
    z = (y.astype(F32) + F32(1)).astype(np.float16)
    return (z.astype(F32) * F32(0.5)).astype(np.float16)


def embed_reference(ids, tok16, pos16) -> np.ndarray:
    idx = np.clip(ids, 0, tok16.shape[0] - 1)
    return (tok16[idx].astype(F32) + pos16[:len(ids)].astype(F32)).astype(np.float16)


AXPY_N_LONG = 8 * (2 * 2048 * 256 + 77)   # more 8-wide chunks than the grid's 2048 * 256 threads: the grid-stride loop runs
AXPY_EXACT_SCALES = (1.0, 0.5, 3.0, -2.0)  # scale * b is exact in fp32 (b has 11 significant bits): fma == multiply, add


def axpy_operands(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal(n).astype(np.float16), rng.standard_normal(n).astype(np.float16)


def axpy_exact(a16, b16, scale) -> np.ndarray:
    """fp16(fp32(a + scale b)): the product is exact, the fp32 sum rounds once, the store once more"""
    return (a16.astype(F32) + F32(scale) * b16.astype(F32)).astype(np.float16)


def axpy_real(a16, b16, scale) -> np.ndarray:
    return (a16.astype(np.float64) + np.float64(F32(scale)) * b16.astype(np.float64)).astype(np.float16)


def ulp_distance(a16, b16) -> np.ndarray:
    """distance in fp16 steps (finite values)"""
    def order(x):
        i = x.view(np.int16).astype(np.int32)
        return np.where(i < 0, -(i & 0x7FFF), i)
    return np.abs(order(np.ascontiguousarray(a16)) - order(np.ascontiguousarray(b16)))


ADAIN_SHAPES = [(84, 320), (4096, 2560)]   # the second: 4096 * 320 chunks = 5120 blocks of 256, over the 4096-block grid cap
ADAIN_EPS = 1e-6
ADAIN_CONST_CHANNEL = 5


@functools.lru_cache(maxsize=None)
def adain_operands(rows, c):
    """x fp16 [rows][c]; stats / stats_ref fp32 [c][2] = (sum, sum of squares): of x itself / of a second tensor.  |mean| <= sd per
    channel, so that E[x^2] - mean^2 loses no more than a bit; channel ADAIN_CONST_CHANNEL is constant 0.5 (variance 0 < eps).
    The kernel's fp32 error is about 1e-6 RELATIVE to the terms it adds; "one fp16 step" is relative to the RESULT, so the operands
    keep every result away from a cancellation: |x - mean| >= 0.4 sd (no element sits on its channel's mean) and |mean_ref| <=
    0.25 sd_ref, hence |out| >= 0.15 sd_ref.  (With plain Gaussian x some of 10^7 results land within 1e-4 of zero, where an fp16
    step is 1e-7 -- below fp32's error on terms of size one: no fp32 AdaIN can meet a one-step bound there.)"""
    rng = np.random.default_rng(rows * 10007 + c)
    out = []
    for mean_share in (0.9, 0.25):
        sd = rng.uniform(0.25, 2.0, c)
        mean = sd * rng.uniform(-mean_share, mean_share, c)
        z = rng.standard_normal((rows, c))
        z = np.sign(z) * (0.5 + np.abs(z))
        z = (z - z.mean(0)) / z.std(0)   # (the sample's own mean and deviation, so that the promise holds at 84 rows too)
        x = (mean + sd * z).astype(np.float16)
        x[:, ADAIN_CONST_CHANNEL] = 0.5
        x64 = x.astype(np.float64)
        out.append((x, np.stack([x64.sum(0), (x64 * x64).sum(0)], axis=-1).astype(F32)))
    return out[0][0], out[0][1], out[1][1]


def adain_reference(x16, st, st_ref, rows, eps=ADAIN_EPS) -> np.ndarray:
    """float64 from the same fp32 statistics, rounded to fp16 once"""
    e = np.float64(F32(eps))

    def ms(s):
        s = s.astype(np.float64)
        mean = s[:, 0] / rows
        return mean, np.sqrt(np.maximum(np.maximum(s[:, 1] / rows - mean * mean, 0.0), e))
    (mean, sd), (mean_r, sd_r) = ms(st), ms(st_ref)
    return (((x16.astype(np.float64) - mean) / sd) * sd_r + mean_r).astype(np.float16)


def adain_float32(x16, st, st_ref, rows, eps=ADAIN_EPS) -> np.ndarray:
    """the kernel's own fp32 arithmetic (csrc/elementwise.hip adain_kernel), operation by operation"""
    inv = F32(1) / F32(rows)

    def ms(s):
        mean = s[:, 0] * inv
        var = np.maximum(s[:, 1] * inv - mean * mean, F32(0))
        return mean, np.sqrt(np.maximum(var, F32(eps)))
    (mean, sd), (mean_r, sd_r) = ms(st), ms(st_ref)
    return (((x16.astype(F32) - mean) / sd) * sd_r + mean_r).astype(np.float16)


def adain_conditions(got16, ref16):
    """(largest fp16 step distance, share of elements that differ at all) -- the bounds are 1 and 1 %"""
    d = ulp_distance(got16, ref16)
    return int(d.max()), float((d != 0).mean())

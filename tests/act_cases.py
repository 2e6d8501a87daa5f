"""Non-linear epilogue cases (tests/test_act_cases_host.py, tests/test_act_forms_gpu.py): SiLU, quick-GELU, erf-GELU, GEGLU and the
tile softmax of the conv / GEMM library in every kernel form, against float64, with a bound PER ELEMENT.

The idea: an exactly known pre-activation.  The lattice of tests/exact_cases.py made dyadic -- activations in {+-1, +-2, +-3},
weights in {+-1, +-2} * 2^-s, bias and rowvec non-zero integers (1..8) * 2^-s.  Every partial sum is an integer multiple of 2^-s, below
2^24 units: exact in fp32 in ANY order, split over K or not.  So the argument x the kernel hands to its activation is known to the
bit, and the only errors left are the activation's own fp32 evaluation and the one fp16 store.  s per case (about log2(sqrt(11.7 K)
/ 2)) spreads x with a deviation of about 2 over [-10, 10]: tests/test_act_cases_host.py asserts |x| <= 16, at least 4 % of x <= -3
(where the GELUs differ and 1 + erf cancels) and at least 10 % of |x| <= 0.5.  out_scale is a power of two; residuals are non-zero
integers (1..8) * 2^-6 -- small, so that the fp16 step of an output stays that of the activation's value and a wrong activation
is not hidden under a residual's coarser step; x * sc + r (the argument of the VSD_ACT_POST forms) is exact.

Reference: float64 of the exact x, rounded to fp16 once.  Bound per element: |got - ref64| <= half an fp16 step of ref64 (subnormals
included: 2^-25 there) + the slack of the function's fp32 evaluation:
  SiLU, quick-GELU   2^-19 |act(x)| |sc|: the exponential's argument rounded once (relative 2^-24 * 1.702 |x| <= 2^-20 for |1.702 x|
                     <= 16 -- asserted for the quick-GELU cases), __expf, the add, v_rcp and the multiply at most 1 ulp each.
                     (The same term tests/norm_cases.py grants GroupNorm's SiLU.)
  erf-GELU           (|x| 2^-21 + 2^-22 |gelu(x)|) |sc|: csrc/common.h's Abramowitz-Stegun erf is within 1.5e-7 ABSOLUTE, three fp32
                     roundings of 1 - p t e and 1 + erf, times 0.5 |x|.  In the negative tail 1 + erf cancels: the fp32 model below
                     lands two fp16 steps from float64 for x in [-5.5, -3.8] while its absolute error stays below 2.4e-7 |x| -- a
                     "one fp16 step" criterion would be wrong there; this bound is not.
  additions behind the activation (not VSD_ACT_POST): fma(act(x), sc, r) rounds ONCE in fp32 and residual2 adds a second rounding;
                     each is at most one fp32 ulp of the sum, 2^-23 |out|.  (An eight-thousandth of the half step: it only matters
                     for a value that lies that close to a tie.)  Activation after the residuals: the argument is exact, no such term.
  GEGLU              ref = h gelu(g), h and g exact: |h| (|g| 2^-21 + 2^-22 |gelu(g)|) + 2^-24 |ref| (the product's rounding).
  tile softmax       the scores are exact; ref = float64 softmax over the first softmax_cols columns of each 128-column group; 2^-17 ref:
                     the log2(e) product, the subtraction of the maximum and exp2 are within 48 * 2^-24 relative per term (|score| <=
                     16) in numerator and denominator, the sum runs over 8 sequential and 4 shuffle additions, one division, one
                     product: < 113 * 2^-24.  Columns >= softmax_cols are exactly +0.
fp16 SUBNORMAL outputs (SiLU / GELU of x <= -9, softmax probabilities below 6e-5) are expected to be STORED, not flushed to zero: their
bound is half the subnormal spacing (2^-25) plus the slack like everyone else's.  A device that flushed them would fail here, and
that would be a finding to report with the case, not a reason to drop the small outputs.

fp32 models: for each function the kernel's arithmetic in numpy fp32, operation by operation (fmaf through float64, rounded once).
The host test asserts that the model's fp32 value is within HALF the slack of float64 on every element of every case: the other half
is for the device's __expf / v_rcp / exp2 being 1-ulp instructions where numpy's are correctly rounded.

Mutations: the answers of kernels that are wrong in the ways these epilogues can be wrong (another GELU, 1.7 for 1.702, SiLU for
quick-GELU, the activation on the wrong side of the scale or the residual, GEGLU's halves swapped or the gate of the neighbouring
64-column group, a softmax over three columns more or without the bias), from the same float64 arithmetic.  The host test shows that
each breaks the bound on at least 5 % of the elements of every case it applies to: the data would notice."""
import dataclasses
import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np

from exact_cases import (SENTINEL, Case, Data, gather, weight_matrix, ulp_distance,  # noqa: F401  (ulp_distance: the fp16 step distance the tests report)
                         T128x128, T128x64, T64x64, T64x128, T256x128, T256x64, T256x256)
from norm_cases import half_step

F32 = np.float32
ACT_NONE, ACT_RELU, ACT_SILU, ACT_GEGLU, ACT_QUICKGELU, ACT_SOFTMAX, ACT_GELU = range(7)
ACT_POST = 256
ACT_NAMES = {ACT_SILU: "silu", ACT_QUICKGELU: "quick", ACT_GELU: "erf", ACT_SILU | ACT_POST: "silu-post", ACT_QUICKGELU | ACT_POST: "quick-post"}
RES_SHIFT = 6            # residuals, residual2 and add2 are non-zero integers (1..8) * 2^-6
X_MAX = 16.0
QUICK_ARG_MAX = 16.0     # |1.702 x|


# ---------------------------------------------------------------------------------------------------------------- conv / GEMM cases
@dataclass(frozen=True)
class ActCase(Case):
    s: int = 6               # weights, bias, rowvec in units of 2^-s
    reaches: str = ""        # the copy of the activation arithmetic this case is here for


def _forms(tiles, pipelines, splits):
    out = []
    for t in tiles:
        for p in pipelines:
            for sp in splits:
                out += [(t, p, sp, True)] + ([(t, p, sp, False)] if sp > 1 else [])
    return tuple(out)


_BASE = dict(h=18, w=14, c0=128, cout=200, rowvec=True, residual=True, s=6, data="base")   # M = 252, N = 200, K = 1152: ragged for every tile
_WALK = (_forms((T64x64, T128x64, T64x128, T128x128), (0, 3, 5), (1,)) + _forms((T64x64,), (3,), (3,)) + _forms((T128x128,), (5,), (3,)) +
         ((T256x128, 3, 1, True),) + _forms((T128x128, T256x128), (8, 9), (1,)) + _forms((T256x256,), (8, 9), (1,)))
_EPI = ((T64x64, 3, 1, True), (T128x128, 3, 1, True), (T64x64, 3, 3, True), (T128x128, 3, 3, False))
_SCALE = ((T64x64, 3, 1, True), (T128x128, 3, 3, True), (T128x64, 0, 3, False))
_SHORT = ((T64x64, 3, 1, True), (T128x128, 5, 1, True), (T128x64, 0, 1, True), (T64x128, 3, 1, True), (T128x128, 9, 1, True),
          (T64x64, 5, 3, True), (T128x64, 3, 3, False))
_HALO = _forms((T128x128, T128x64, T256x128, T256x64), (7,), (1, 2))
_C64 = ((T256x64, 10, 1, True),)


def _per_act(act):
    a = ACT_NAMES[act]
    post = bool(act & ACT_POST)
    walk = ("the 'keep it correct' branch of conv_epilogue.inc -> epilogue_store8" if post or act == ACT_GELU else
            f"straight-line walk ACT {2 if act == ACT_SILU else 4} of conv_epilogue.inc")

    def scaled(sc):
        """the activation after the residual sees x * sc + r: there the lattice's unit moves with the scale, so that this argument, not x,
        covers what the base cases' x covers (and |1.702 * argument| stays below 16)"""
        s = 6 + int(math.log2(sc)) if post else 6
        return _BASE if s == 6 else {**_BASE, "s": s, "data": f"base-s{s}"}

    return [
        ActCase(f"{a}-walk", **_BASE, act=act, forms=_WALK, reaches=walk + "; its from_slabs form; splitk_reduce_kernel"),
        ActCase(f"{a}-res2", **_BASE, act=act, residual2=True, forms=_EPI, reaches="general loop: epilogue_store8, 8-wide"),
        ActCase(f"{a}-out2", **_BASE, act=act, out2=True, forms=_EPI, reaches="general loop: epilogue_store8, 8-wide, out2"),
        ActCase(f"{a}-n196", **{**_BASE, "cout": 196}, act=act, forms=_EPI, reaches="epilogue_store8's scalar tail (N % 8 = 4)"),
        ActCase(f"{a}-scale-0.5", **scaled(0.5), act=act, out_scale=0.5, forms=_SCALE),
        ActCase(f"{a}-scale-2", **scaled(2.0), act=act, out_scale=2.0, forms=_SCALE),
        ActCase(f"{a}-scale-dev-2", **scaled(2.0), act=act, out_scale=2.0, scale_dev=True, forms=_SCALE, reaches="out_scale_dev"),
        ActCase(f"{a}-1x1-m99", h=9, w=11, c0=320, cout=72, ksize=1, rowvec=True, residual=True, s=5, act=act, forms=_SHORT, data="m99"),
        ActCase(f"{a}-1x1-m1", h=1, w=1, c0=320, cout=200, ksize=1, rowvec=True, residual=True, s=5, act=act, forms=_SHORT, data="m1"),
    ]


def _out_t(act):
    a = ACT_NAMES[act]
    g = dict(w=14, c0=128, cout=200, rowvec=True, t_col0=128, s=6, act=act)
    tt = "transposed-tile path of conv_epilogue.inc"
    return [
        ActCase(f"{a}-out_t-hw252", h=18, **g, forms=_EPI + ((T64x64, 0, 3, False),), data="base", reaches=tt + ", scalar stores"),
        ActCase(f"{a}-out_t-hw224", h=16, **g, forms=_EPI, data="hw224", reaches=tt + ", 16-byte stores"),
        ActCase(f"{a}-out_t-hw252-b3", h=18, **g, batch=3, t_img=256, forms=_EPI + ((T64x64, 0, 3, False),), data="b3", reaches=tt + ", batch 3, scalar stores"),
        ActCase(f"{a}-out_t-hw224-b3", h=16, **g, batch=3, t_img=256, forms=_EPI, data="hw224-b3", reaches=tt + ", batch 3, 16-byte stores"),
        ActCase(f"{a}-out_t-n196", h=18, **{**g, "cout": 196}, forms=_EPI, data="base", reaches="the transposed branch of epilogue_store8 (N % 8 != 0)"),
        ActCase(f"{a}-out_t-out2", h=18, **g, out2=True, forms=_EPI, data="base", reaches="the transposed branch of epilogue_store8 (out2)"),
    ]


CONV_CASES = [c for act in ACT_NAMES for c in _per_act(act)] + _out_t(ACT_SILU) + _out_t(ACT_QUICKGELU) + [
    ActCase("silu-halo", **_BASE, act=ACT_SILU, forms=_HALO, reaches="`finish` of csrc/conv_halo.hip, its in-launch reduction, splitk_reduce_kernel"),
    ActCase("silu-c64-37x50-b2", h=37, w=50, c0=64, cout=64, batch=2, residual=True, s=5, act=ACT_SILU, forms=_C64, reaches="csrc/conv_c64.hip, 64-wide"),
    ActCase("silu-c64-16x24-up32x48", h=16, w=24, c0=64, cout=64, up=(32, 48), s=5, act=ACT_SILU, forms=_C64, reaches="csrc/conv_c64.hip, 64-wide, no residual"),
    ActCase("silu-c64-thin-n3", h=37, w=50, c0=64, cout=3, batch=2, thin=True, s=5, act=ACT_SILU, forms=_C64, reaches="csrc/conv_c64.hip, thin"),
    ActCase("silu-c64-thin-n4", h=16, w=24, c0=64, cout=4, up=(32, 48), thin=True, s=5, act=ACT_SILU, forms=_C64, reaches="csrc/conv_c64.hip, thin"),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)

# what csrc/conv_gemm.hip refuses (VSD_ERR_ARG): erf-GELU off the general walk, an activation after the residual with a transposed output
REFUSED = [
    ActCase("erf-out_t", h=18, w=14, c0=128, cout=200, rowvec=True, t_col0=128, act=ACT_GELU, data="base"),
    ActCase("erf-rowstat", h=18, w=14, c0=128, cout=192, rowvec=True, rowstat=True, act=ACT_GELU, data="base192"),
    ActCase("erf-post", **_BASE, act=ACT_GELU | ACT_POST),
    ActCase("silu-post-out_t", h=18, w=14, c0=128, cout=200, rowvec=True, t_col0=128, act=ACT_SILU | ACT_POST, data="base"),
    ActCase("quick-post-out_t", h=18, w=14, c0=128, cout=200, rowvec=True, t_col0=128, act=ACT_QUICKGELU | ACT_POST, data="base"),
    ActCase("relu-post-out_t", h=18, w=14, c0=128, cout=200, rowvec=True, t_col0=128, act=ACT_RELU | ACT_POST, data="base"),
]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _signed(rng, lo, hi, shape):
    return (rng.integers(lo, hi + 1, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)).astype(np.float64)


def _choice(rng, values, shape):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), size=shape)]


@functools.lru_cache(maxsize=None)
def _conv_data(name, h, w, c0, cout, ksize, batch, up, s):
    """every tensor a case of this geometry may ask for, in the values themselves (float64, all dyadic and exact in fp16)"""
    c = Case(name, h, w, c0, cout, ksize=ksize, batch=batch, up=up)
    rng = _rng("act", name, h, w, c0, cout, ksize, batch, up, s)
    u, ru = 2.0 ** -s, 2.0 ** -RES_SHIFT
    ldr, ldo = (cout + 7) // 8 * 8, (cout + 7) // 8 * 8 + 8
    return dict(src=[_choice(rng, (-3, -2, -1, 1, 2, 3), (batch, h, w, c0))],
                weight=_choice(rng, (-2, -1, 1, 2), (cout, c0, ksize, ksize)) * u,
                bias=_signed(rng, 1, 8, cout) * u, rowvec=_signed(rng, 1, 8, cout) * u,
                residual=_signed(rng, 1, 8, (c.m, ldr)) * ru, residual2=_signed(rng, 1, 8, (c.m, ldr)) * ru,
                add2=_signed(rng, 1, 8, (c.m, ldo)) * ru)


def conv_data(c: ActCase) -> Data:
    t = _conv_data(c.data or c.name, c.h, c.w, c.c0, c.cout, c.ksize, c.batch, c.up, c.s)
    add2 = t["add2"]
    if c.thin:
        add2 = None
    return Data(t["src"], t["weight"], t["bias"] if c.bias else None, t["rowvec"] if c.rowvec else None,
                t["residual"] if c.residual else None, t["residual2"] if c.residual2 else None, add2 if c.out2 else None)


def argument(c: ActCase, d: Data, x):
    """what the activation is evaluated on: x, or x * sc + the residuals with VSD_ACT_POST (exact either way)"""
    if not c.act & ACT_POST:
        return x
    return x * c.out_scale + sum(t[:, :c.cout] for t in (d.residual, d.residual2) if t is not None)


def preactivation(c: ActCase, d: Data):
    """-> (x float64 [M][cout]: exact, the largest partial sum there can be in units of 2^-s)"""
    a = gather(c, d.src)
    w = weight_matrix(c, d.weight)
    x, big = a @ w.T, np.abs(a) @ np.abs(w).T
    for v in (d.bias, d.rowvec):
        if v is not None:
            x, big = x + v, big + np.abs(v)
    return x, big * 2.0 ** c.s


# ---------------------------------------------------------------------------------------------------------------- float64 functions
def _erf(x):
    """float64 erf (the C library's, through torch where it is installed: ten million elements in the fused-tail cases)"""
    try:
        import torch
    except ImportError:
        return np.vectorize(math.erf, otypes=[np.float64])(x)
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def silu64(x):
    return x / (1.0 + np.exp(-x))


def quick64(x, k=1.702):
    return x / (1.0 + np.exp(-k * x))


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x * math.sqrt(0.5)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


ACT64 = {ACT_SILU: silu64, ACT_QUICKGELU: quick64, ACT_GELU: gelu64}


def act_slack(kind, x, a):
    """the fp32 evaluation's share of the bound, before the scale: x the argument, a = act(x) in float64"""
    if kind == ACT_GELU:
        return np.abs(x) * 2.0 ** -21 + 2.0 ** -22 * np.abs(a)
    return 2.0 ** -19 * np.abs(a)


@dataclass
class Ref:
    out: np.ndarray     # float64 [M][cout] (columns >= t_col0: what out_t holds, transposed back)
    slack: np.ndarray   # float64: the bound above half an fp16 step of out

    @property
    def bound(self):
        return half_step(self.out) + self.slack


def epilogue64(c: ActCase, d: Data, x, fn=None, order="", slack_of=None) -> Ref:
    """the epilogue of include/vsd.h in float64 on the exact x.  fn: another function than the case's (a mutation); order: "" as the
    case says, "scale-first": the activation after the scale, "flip-post": VSD_ACT_POST read the other way round"""
    kind, post = c.act & 0xff, bool(c.act & ACT_POST)
    fn = fn or ACT64[kind]
    if order == "flip-post":
        post = not post
    sc = c.out_scale
    t0 = c.cout if c.t_col0 is None else c.t_col0
    r = np.zeros_like(x)
    for t in (d.residual, d.residual2):
        if t is not None:
            r[:, :t0] += t[:, :t0]
    if post:
        arg = x * sc + r
        out = fn(arg)
        slack = act_slack(kind, arg, out)
    elif order == "scale-first":
        out = fn(x * sc) + r
        slack = np.zeros_like(x)
    else:
        a = fn(x)
        out = a * sc
        slack = act_slack(kind, x, a) * abs(sc)
        for t in (d.residual, d.residual2):   # each addition rounds once in fp32: one ulp of ITS sum at most
            if t is not None:
                out[:, :t0] += t[:, :t0]
                slack[:, :t0] += 2.0 ** -23 * np.abs(out[:, :t0])
    return Ref(out, slack)


@functools.lru_cache(maxsize=None)
def _conv_reference(c: ActCase):
    d = conv_data(c)
    x, _ = preactivation(c, d)
    return x, epilogue64(c, d, x)


def conv_reference(c: ActCase):
    """-> (x, Ref)"""
    return _conv_reference(dataclasses.replace(c, forms=(), reaches=""))


def violations(got16, ref: Ref):
    """bool per element: outside the bound (a non-finite value is outside)"""
    return ~(np.abs(got16.astype(np.float64) - ref.out) <= ref.bound)


# ---------------------------------------------------------------------------------------------------------------- the fp32 models
def _fma32(a, b, c):
    """fmaf on fp32 operands: the product is exact in float64, the sum rounds to 53 bits and then to 24"""
    a, b, c = (np.asarray(v) for v in (a, b, c))
    assert a.dtype == F32 and b.dtype == F32 and c.dtype == F32
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def silu32(x):
    """csrc/common.h silu_f: x * rcp(1 + exp(-x))"""
    with np.errstate(over="ignore"):
        return x * (F32(1) / (F32(1) + np.exp(-x)))


def quick32(x):
    """quick_gelu_f: x * rcp(1 + exp(-1.702f * x))"""
    with np.errstate(over="ignore"):
        return x * (F32(1) / (F32(1) + np.exp(F32(-1.702) * x)))


def erf_as32(x):
    """erf_as_f: Abramowitz & Stegun 7.1.26 with one rcp, one exp and five fused multiply-adds"""
    ax = np.abs(x)
    t = F32(1) / _fma32(ax, F32(0.3275911), F32(1.0))
    p = _fma32(t, F32(1.061405429), F32(-1.453152027))
    p = _fma32(p, t, F32(1.421413741))
    p = _fma32(p, t, F32(-0.284496736))
    p = _fma32(p, t, F32(0.254829592))
    r = F32(1) - p * t * np.exp(-ax * ax)
    return np.copysign(r, x)


def gelu32(x):
    """gelu_erf_f: 0.5f * x * (1 + erf_as_f(x * 0.70710678f))"""
    return F32(0.5) * x * (F32(1) + erf_as32(x * F32(0.70710678118654752)))


ACT32 = {ACT_SILU: silu32, ACT_QUICKGELU: quick32, ACT_GELU: gelu32}


def epilogue32(c: ActCase, d: Data, x) -> np.ndarray:
    """the kernels' epilogue in fp32 on the exact x (csrc/conv_kernels.h epilogue_store8 and the walks of csrc/conv_epilogue.inc are
    the same operations): act, fma(v, sc, residual), + residual2, the activation here instead with VSD_ACT_POST.  -> fp32, before the store"""
    kind, post = c.act & 0xff, bool(c.act & ACT_POST)
    fn = ACT32[kind]
    t0 = c.cout if c.t_col0 is None else c.t_col0
    v = x.astype(F32)
    assert (v.astype(np.float64) == x).all()
    if not post:
        v = fn(v)
    r = np.zeros(x.shape, dtype=F32)
    if d.residual is not None:
        r[:, :t0] = d.residual[:, :t0]
    v = _fma32(v, F32(c.out_scale), r)
    if d.residual2 is not None:
        v[:, :t0] = v[:, :t0] + d.residual2[:, :t0].astype(F32)
    if post:
        v = fn(v)
    assert v.dtype == F32
    return v


# ---------------------------------------------------------------------------------------------------------------- the mutations
# name -> (applies(case), wrong(case, data, x) -> float64 [M][cout])
def _kind(c):
    return c.act & 0xff


def _has_res(c):
    return c.residual or c.residual2


CONV_MUTATIONS = {
    "tanh-GELU for erf-GELU": (lambda c: _kind(c) == ACT_GELU, lambda c, d, x: epilogue64(c, d, x, fn=gelu_tanh64).out),
    "quick-GELU for erf-GELU": (lambda c: _kind(c) == ACT_GELU, lambda c, d, x: epilogue64(c, d, x, fn=quick64).out),
    "erf-GELU for quick-GELU": (lambda c: _kind(c) == ACT_QUICKGELU, lambda c, d, x: epilogue64(c, d, x, fn=gelu64).out),
    "1.7 for 1.702": (lambda c: _kind(c) == ACT_QUICKGELU, lambda c, d, x: epilogue64(c, d, x, fn=lambda v: quick64(v, 1.7)).out),
    "SiLU for quick-GELU": (lambda c: _kind(c) == ACT_QUICKGELU, lambda c, d, x: epilogue64(c, d, x, fn=silu64).out),
    "the activation after the scale": (lambda c: c.out_scale != 1.0 and not c.act & ACT_POST, lambda c, d, x: epilogue64(c, d, x, order="scale-first").out),
    "VSD_ACT_POST read the other way round": (lambda c: _has_res(c) and c.t_col0 is None and _kind(c) != ACT_GELU,
                                              lambda c, d, x: epilogue64(c, d, x, order="flip-post").out),
}
MUTATION_SHARE = 0.05


# ---------------------------------------------------------------------------------------------------------------- GEGLU and softmax
@dataclass(frozen=True)
class LinCase:
    name: str
    kind: int                # ACT_GEGLU | ACT_SOFTMAX
    m: int
    k: int
    n: int                   # columns of the GEMM (GEGLU: hidden + gate, the output has n / 2)
    s: int
    forms: tuple = ()
    reaches: str = ""


_GEGLU_FORMS = ((T128x128, 3, 1, True), (T64x128, 3, 1, True), (T256x128, 3, 1, True), (T128x128, 8, 1, True), (T256x256, 8, 1, True), (T256x256, 9, 1, True))
GEGLU_CASES = [LinCase(f"geglu-m{m}-n{n}", ACT_GEGLU, m, 320, n, 5, _GEGLU_FORMS,
                       "GEGLU, bias form: workgroup-wide epilogue; per wave on the 256x256 tile") for m in (252, 99, 1) for n in (256, 640)]
SOFTMAX_COLS = (1, 8, 9, 77, 127, 128)
_SOFTMAX_FORMS = tuple((t, 3, sp, True) for t in (T64x128, T128x128, T256x128) for sp in (1, 2, 4))
SOFTMAX_CASES = [LinCase(f"softmax-m{m}", ACT_SOFTMAX, m, 512, 1024, 5, _SOFTMAX_FORMS, "tile softmax, bias form, unsplit and from_slabs") for m in (99, 1)]


# Three special score rows in the softmax case of 99 rows -- the only zeros of these tables: the last three input channels are
# zero in every lattice row, a special row is zero everywhere else and 1 in its own channel, and that channel's weights are
# (target - bias): all scores equal (1 / cols each); column 0 of every group 32 above the rest (exactly 1, the rest 0); scores descending
# in steps of 1/4 from column 0 on, across the boundary of a lane's 8-column chunk at column 8.  (|score| <= 32 there; the bound's
# derivation holds: the exponent's argument is within 2^-18 absolute, 2^-18.5 relative in exp2, and every term that small is far
# below the subnormal half step.)
SPECIAL_ROWS = (1, 64, 98)   # inside the first 64-row tile, first of the second, the last row (ragged on every tile height)


def special_targets(n):
    col = np.arange(n) % 128
    return np.stack([np.zeros(n), np.where(col == 0, 32.0, 0.0), -col / 4.0])


def has_special(c: LinCase):
    return c.kind == ACT_SOFTMAX and c.m > max(SPECIAL_ROWS)


@functools.lru_cache(maxsize=None)
def lin_data(c: LinCase):
    """-> a [m][k], w [n][k] (GEGLU: rows [0, n/2) hidden, [n/2, n) gate, as the networks hold it), bias [n]: float64, dyadic"""
    rng = _rng("lin", c.name)
    u = 2.0 ** -c.s
    a, w, b = (_choice(rng, (-3, -2, -1, 1, 2, 3), (c.m, c.k)), _choice(rng, (-2, -1, 1, 2), (c.n, c.k)) * u, _signed(rng, 1, 8, c.n) * u)
    if has_special(c):
        a[:, -3:] = 0
        for i, r in enumerate(SPECIAL_ROWS):
            a[r] = 0
            a[r, c.k - 3 + i] = 1
        w[:, -3:] = (special_targets(c.n) - b).T
    return a, w, b


def lin_pre(c: LinCase):
    """-> (x [m][n] exact, the largest partial sum in units of 2^-s)"""
    a, w, b = lin_data(c)
    return a @ w.T + b, (np.abs(a) @ np.abs(w).T + np.abs(b)) * 2.0 ** c.s


def geglu64(x, fn=gelu64, swap=False, gate_shift=0) -> np.ndarray:
    f = x.shape[1] // 2
    h, g = x[:, :f], x[:, f:]
    if gate_shift:   # the gate of the neighbouring 64-column group
        g = np.roll(g.reshape(len(x), f // 64, 64), -gate_shift, axis=1).reshape(len(x), f)
    return fn(h) * g if swap else h * fn(g)


def geglu_reference(c: LinCase) -> Ref:
    x, _ = lin_pre(c)
    f = c.n // 2
    h, g = x[:, :f], x[:, f:]
    a = gelu64(g)
    out = h * a
    return Ref(out, np.abs(h) * act_slack(ACT_GELU, g, a) + 2.0 ** -24 * np.abs(out))


def geglu32(x) -> np.ndarray:
    f = x.shape[1] // 2
    v = x.astype(F32)
    return v[:, :f] * gelu32(v[:, f:])


GEGLU_MUTATIONS = {
    "tanh-GELU": lambda x: geglu64(x, fn=gelu_tanh64),
    "gelu(h) * g": lambda x: geglu64(x, swap=True),
    "the gate of the neighbouring 64-column group": lambda x: geglu64(x, gate_shift=1),
}


def softmax64(x, cols) -> np.ndarray:
    m, n = x.shape
    v = x.reshape(m, n // 128, 128)[:, :, :cols]
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    out = np.zeros((m, n // 128, 128))
    out[:, :, :cols] = e / e.sum(axis=-1, keepdims=True)
    return out.reshape(m, n)


def softmax_reference(c: LinCase, cols) -> Ref:
    out = softmax64(lin_pre(c)[0], cols)
    return Ref(out, 2.0 ** -17 * out)


def softmax32(x, cols) -> np.ndarray:
    """the softmax epilogue of csrc/conv_epilogue.inc in fp32: * log2(e), the maximum, exp2, the sum over a lane's 8 columns in order
    and then over the row's 16 lanes by four xor-shuffles, one division, one product"""
    m, n = x.shape
    v = x.astype(F32).reshape(m, n // 128, 16, 8) * F32(1.4426950408889634)
    live = (np.arange(128) < cols).reshape(16, 8)
    v = np.where(live, v, F32(-3.0e38))
    mx = v.max(axis=(2, 3), keepdims=True)
    with np.errstate(over="ignore"):
        e = np.where(live, np.exp2(v - mx), F32(0)).astype(F32)
    lane = np.zeros(e.shape[:3], dtype=F32)
    for i in range(8):
        lane = lane + e[..., i]
    for o in (1, 2, 4, 8):
        lane = lane + lane[..., np.arange(16) ^ o]
    inv = F32(1) / lane
    out = e * inv[..., None]
    assert out.dtype == F32
    return out.reshape(m, n)


SOFTMAX_MUTATIONS = {   # (cols it applies to, wrong(case, cols))
    "three columns more": ((77,), lambda c, cols: softmax64(lin_pre(c)[0], cols + 3)),
    "without the bias": (SOFTMAX_COLS[1:], lambda c, cols: softmax64(lin_pre(c)[0] - lin_data(c)[2], cols)),
}


def report(got16, ref: Ref):
    """(worst |got - ref| / bound, the largest share of the SLACK -- the bound above half an fp16 step -- an element needs, the farthest
    element in fp16 steps from fp16(ref), the share of elements that differ from it at all)"""
    err = np.abs(got16.astype(np.float64) - ref.out)
    with np.errstate(over="ignore"):
        steps = ulp_distance(got16, ref.out.astype(np.float16))
    over = np.maximum(err - half_step(ref.out), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        used = np.where(over > 0, over / ref.slack, 0.0)
    return float((err / ref.bound).max()), float(used.max()), int(steps.max()), float((steps != 0).mean())


# ---------------------------------------------------------------------------------------------------------------- folded LayerNorm
# The consumer GEMM runs on the raw rows h with W' = W * gamma and finishes v = rstd * (acc - mean * s) + t in its epilogue (ln_part;
# csrc/conv_kernels.h ln_row_stats / ln_transform8), from the per-row (sum, sum of squares) partials the producing GEMM left.  Rows
# as in tests/norm_cases.py: integers m_r + clip(s_r * k, -3, 3), centre m_r in -4..4 different for adjacent rows, spread s_r in
# {1, 2}, k in {+-1, +-2, +-3} -- or, the large-mean draw, centres of +-48 alternating with offsets +-1..3 (|h| <= 51: exact in fp16).  S
# and Q are integers below 2^24: exact in any order.  gamma in {1/2, 1, 2}, beta and the weights dyadic: W * gamma, s, t and acc are exact.
# Bound on v: 2^-20 T, T = |rstd acc| + |rstd mean s| + |t| (tests/norm_cases.py's term: 16 fp32 roundings of the terms the kernel adds).  For the
# ordinary rows that is all: the fp32 model below stays within half of it (the host test asserts so).  For the centre-48 rows it is NOT --
# the model is 40 times outside -- because it leaves out the variance's own cancellation: var = Q / K - mean^2 is the difference of
# two numbers of size E[h^2] = 2300 that leaves 4.7.  Each rounding is at most 2^-24 relative: 1 / K (1), mean = S / K (2 in all), mean^2
# (2 * 2 + 1), Q / K (2) -- up to 7 * 2^-24 E[h^2] absolute in var, half of that relative to var in rstd, and v - t moves with rstd.
# So those rows get, beside 2^-20 T:  2^-22 (E[h^2] / var) |v - t|  (3.5 rounded up to 4; E[h^2] / var is about 500 there).  A statement
# about one-pass variance in fp32, derived from the format, not from the kernel's output; profiles/act_forms.txt has what the device uses of it.
# Through an activation: * 1.13 (|act'| <= 1.13); softmax: 2 * the largest such bound of the row, relative.
LN_EPS = 1e-5


@dataclass(frozen=True)
class LnCase:
    name: str
    kind: str                # "qkv": Q, K plain and V transposed (n = 3 c, t_col0 = 2 c) | "geglu" | "softmax"
    m: int
    c: int
    n: int
    s: int
    centre: int = 0          # 48: the large-mean draw
    forms: tuple = ()
    reaches: str = ""


_QKV_FORMS = ((T64x64, 3, 1, True), (T64x64, 3, 2, True), (T64x64, 3, 2, False), (T128x128, 5, 1, True))
LN_CASES = [
    LnCase("ln-qkv-c320", "qkv", 99, 320, 960, 4, forms=_QKV_FORMS, reaches="straight-line walk <0, LN>; transposed-tile path with ln_part; from_slabs; splitk_reduce_kernel"),
    LnCase("ln-qkv-c1280", "qkv", 99, 1280, 3840, 5, forms=_QKV_FORMS),
    LnCase("ln-qkv-c320-centre48", "qkv", 99, 320, 960, 4, centre=48, forms=_QKV_FORMS),
    LnCase("ln-qkv-c1280-centre48", "qkv", 99, 1280, 3840, 5, centre=48, forms=_QKV_FORMS),
] + [LnCase(f"ln-geglu-m{m}-n{n}", "geglu", m, 320, n, 4, forms=_GEGLU_FORMS, reaches="GEGLU, ln_part form") for m in (252, 99, 1) for n in (256, 640)] + [
] + [
    LnCase(f"ln-softmax-m{m}", "softmax", m, 320, 1024, 4, forms=tuple((t, 3, sp, True) for t in (T64x128, T128x128, T256x128) for sp in (1, 2)),
           reaches="tile softmax, ln_part form") for m in (99, 1)
]


@functools.lru_cache(maxsize=None)
def ln_data(c: LnCase):
    """-> h [m][c] integers, gamma [c], beta [c], w [n][c], bias [n] or None: float64, all exact in fp16"""
    rng = _rng("ln", c.name)
    k = _signed(rng, 1, 3, (c.m, c.c))
    if c.centre:
        centre = c.centre * np.where(np.arange(c.m) % 2 == 0, 1.0, -1.0)
        h = centre[:, None] + k
    else:
        centre = (np.cumsum(rng.integers(1, 9, size=c.m)) + rng.integers(0, 9)) % 9 - 4.0
        spread = rng.integers(1, 3, size=c.m).astype(np.float64)
        h = centre[:, None] + np.clip(spread[:, None] * k, -3, 3)
    gamma = _choice(rng, (0.5, 1.0, 2.0), c.c)
    beta = _signed(rng, 1, 4, c.c) * 0.125
    w = _choice(rng, (-2, -1, 1, 2), (c.n, c.c)) * 2.0 ** -c.s
    bias = None if c.kind == "qkv" else _signed(rng, 1, 8, c.n) * 2.0 ** -c.s
    return h, gamma, beta, w, bias


@dataclass
class LnPre:
    v: np.ndarray        # float64 [m][n]: LN(h) W^T + b
    slack: np.ndarray    # the bound on the kernel's v
    acc: np.ndarray      # h W'^T (exact)
    big: np.ndarray      # sum |h W'| in units of 2^-(s + 1)
    s: np.ndarray        # [n]
    t: np.ndarray
    mean: np.ndarray     # [m][1]
    rstd: np.ndarray


def fold_rows(h, gamma, beta, w, bias, shift, variance_term=False, stats_from=None) -> LnPre:
    """float64 LayerNorm(h) W^T + b in the folded form, and the bound on the kernel's value of it.  stats_from: the row whose (mean, rstd)
    row r uses -- None: its own; a mutation passes the neighbours'"""
    wp = w * gamma
    acc, big = h @ wp.T, (np.abs(h) @ np.abs(wp).T) * 2.0 ** (shift + 1)
    s, t = wp.sum(axis=1), w @ beta + (0.0 if bias is None else bias)
    mean = h.mean(axis=1, keepdims=True)
    q = (h * h).mean(axis=1, keepdims=True)
    var = h.var(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + np.float64(F32(LN_EPS)))
    if stats_from is not None:
        mean, rstd = mean[stats_from], rstd[stats_from]
    v = rstd * (acc - mean * s) + t
    slack = 2.0 ** -20 * (np.abs(rstd * acc) + np.abs(rstd * mean * s) + np.abs(t))
    if variance_term:
        slack = slack + 2.0 ** -22 * (q / var) * np.abs(v - t)
    return LnPre(v, slack, acc, big, s, t, mean, rstd)


def fold_rows32(h, p: LnPre) -> np.ndarray:
    """the kernels' arithmetic in fp32: ln_row_stats (S, Q exact; * 1 / K; the variance in one pass; rsqrt) and ln_transform8 -- and
    store_tile_and_stats / the q and GEGLU lines of csrc/fused_tail.hip, which are the same operations"""
    S, Q = h.sum(axis=1, keepdims=True).astype(F32), (h * h).sum(axis=1, keepdims=True).astype(F32)
    inv = F32(1) / F32(h.shape[1])
    mean = S * inv
    rstd = F32(1) / np.sqrt(np.maximum(Q * inv - mean * mean, F32(0)) + F32(LN_EPS))
    v = rstd * (p.acc.astype(F32) - mean * p.s.astype(F32)) + p.t.astype(F32)
    assert v.dtype == F32
    return v


def ln_fold(c: LnCase, stats_from=None) -> LnPre:
    h, gamma, beta, w, bias = ln_data(c)
    return fold_rows(h, gamma, beta, w, bias, c.s, bool(c.centre), stats_from)


def ln_fold32(c: LnCase) -> np.ndarray:
    return fold_rows32(ln_data(c)[0], ln_fold(c))


def geglu_ln_reference(ph: LnPre, pg: LnPre) -> Ref:
    """h gelu(g) behind the fold: the GEGLU bound with both factors' own bounds (|gelu'| <= 1.13)"""
    a = gelu64(pg.v)
    out = ph.v * a
    da = act_slack(ACT_GELU, pg.v, a) + 1.13 * pg.slack
    return Ref(out, np.abs(ph.v) * da + np.abs(a) * ph.slack + ph.slack * da + 2.0 ** -24 * np.abs(out))


def ln_reference(c: LnCase, cols=0, stats_from=None) -> Ref:
    """what the consumer stores: qkv -> v itself; geglu -> h gelu(g); softmax -> probabilities over `cols` columns per group"""
    p = ln_fold(c, stats_from)
    if c.kind == "qkv":
        return Ref(p.v, p.slack)
    if c.kind == "geglu":
        f = c.n // 2
        half = lambda lo, hi: LnPre(*(getattr(p, k)[:, lo:hi] for k in ("v", "slack", "acc", "big")), p.s[lo:hi], p.t[lo:hi], p.mean, p.rstd)  # noqa: E731
        return geglu_ln_reference(half(0, f), half(f, c.n))
    out = softmax64(p.v, cols)
    return Ref(out, out * (2.0 ** -17 + 2.0 * p.slack.max(axis=1, keepdims=True)))


def ln_model32(c: LnCase, cols=0) -> np.ndarray:
    v = ln_fold32(c)
    if c.kind == "qkv":
        return v
    if c.kind == "geglu":
        f = c.n // 2
        return v[:, :f] * gelu32(v[:, f:])
    return softmax32(v.astype(np.float64), cols)


def ln_next_row(c: LnCase):
    """the mutation: row r finished with row r + 1's mean and rstd (the last row with the first's)"""
    return (np.arange(c.m) + 1) % c.m


# ---------------------------------------------------------------------------------------------------------------- csrc/fused_tail.hip
# The 320-wide blocks run vsd_tail_a / vsd_tail_b, with a LayerNorm fold and a GEGLU of their own.
# tail_a on a dense integer lattice: att in {+-1, +-2, +-3}, W_out in {+-1, +-2}, b_out and the residual h integers 1..8: h1 = att W^T + b
# + h is an integer (|h1| < 2048) known to the bit, its row statistics are exact (sum h1^2 < 2^24 per row), and q = LN(h1) Wq'^T is held to the fold's
# bound 2^-20 T.  m = 200 and 4100: the 16- and the 32-row tiles, both ending ragged -- the two heights pick_tail_bm gives tail_a.
# tail_b with PROBE weights that make the inner GEGLU visible: the out-projection is a signed permutation (h2 = +-att2[perm] + b + h1 is
# a row of the ordinary LayerNorm lattice above), w_ff2 = 64 * a one-hot selection of 320 of the 1280 hidden columns (four launches cover
# them all), b_ff2 = 0, proj_out = identity, b_proj = 0, x = 0.  Where csrc/fused_tail.hip rounds: Hc = fp16(hv * gelu(gv)) into LDS
# (geglu_to_lds); acc3 = 64 Hc exactly; h3 = acc3 + 0 + h2 in fp32 -- exact, 64 Hc is a multiple of 2^-18 below 2^13 -- and fp16(h3) into
# the token tile (store_tile_and_stats); proj_out of the identity returns that tile, + 0 + 0, and the last store rounds nothing.  So
# out = fp16(64 fp16(Hc) + h2): bound = 64 * (half a step of Hc + the GEGLU-behind-the-fold slack of Hc) + half a step of 64 Hc + h2.
TAIL_C = 320
TAIL_A_M = (200, 4100)
TAIL_B_M = (200, 8000, 8008, 12000)   # 16-row tiles ending ragged; 32-row tiles, 250 full ones / ending ragged; 48-row tiles
TAIL_SHIFT = 4


@functools.lru_cache(maxsize=2)
def tail_a_data(m):
    """-> att, h, w_out, b_out (integers), gamma, beta, wq: float64"""
    rng, c = _rng("tail_a", m), TAIL_C
    return (_choice(rng, (-3, -2, -1, 1, 2, 3), (m, c)), _signed(rng, 1, 8, (m, c)), _choice(rng, (-2, -1, 1, 2), (c, c)), _signed(rng, 1, 8, c),
            _choice(rng, (0.5, 1.0, 2.0), c), _signed(rng, 1, 4, c) * 0.125, _choice(rng, (-2, -1, 1, 2), (c, c)) * 2.0 ** -TAIL_SHIFT)


def tail_a_reference(m, stats_from=None):
    """-> (h1 float64 [m][320], exact; the fold of q)"""
    att, h, wo, bo, gamma, beta, wq = tail_a_data(m)
    h1 = att @ wo.T + bo + h
    return h1, fold_rows(h1, gamma, beta, wq, None, TAIL_SHIFT, False, stats_from)


@functools.lru_cache(maxsize=2)
def tail_b_data(m):
    """-> att2, h1, perm, sign, b_out, h2 (= sign * att2[:, perm] + b_out + h1), gamma, beta, wf1 [2560][320], bf1 [2560]"""
    rng, c = _rng("tail_b", m), TAIL_C
    centre = (np.cumsum(rng.integers(1, 9, size=m)) + rng.integers(0, 9)) % 9 - 4.0
    spread = rng.integers(1, 3, size=m).astype(np.float64)
    h2 = centre[:, None] + np.clip(spread[:, None] * _signed(rng, 1, 3, (m, c)), -3, 3)
    att2 = _choice(rng, (-3, -2, -1, 1, 2, 3), (m, c))
    perm, sign, bo = rng.permutation(c), _choice(rng, (-1, 1), c), _signed(rng, 1, 2, c)
    h1 = h2 - (sign * att2[:, perm] + bo)
    return (att2, h1, perm, sign, bo, h2, _choice(rng, (0.5, 1.0, 2.0), c), _signed(rng, 1, 4, c) * 0.125,
            _choice(rng, (-2, -1, 1, 2), (8 * c, c)) * 2.0 ** -TAIL_SHIFT, _signed(rng, 1, 8, 8 * c) * 2.0 ** -TAIL_SHIFT)


def tail_b_select(launch):
    """the 320 hidden columns launch 0..3 makes visible"""
    return launch + 4 * np.arange(TAIL_C)


@dataclass
class TailB:
    hc: Ref            # the GEGLU value of the selected columns and its slack
    out: np.ndarray    # float64: 64 Hc + h2
    bound: np.ndarray
    ph: LnPre
    pg: LnPre


def tail_b_reference(m, launch, stats_from=None, fn=None) -> TailB:
    att2, h1, perm, sign, bo, h2, gamma, beta, wf1, bf1 = tail_b_data(m)
    sel, f = tail_b_select(launch), 4 * TAIL_C
    ph = fold_rows(h2, gamma, beta, wf1[sel], bf1[sel], TAIL_SHIFT, False, stats_from)
    pg = fold_rows(h2, gamma, beta, wf1[f + sel], bf1[f + sel], TAIL_SHIFT, False, stats_from)
    hc = geglu_ln_reference(ph, pg)
    if fn is not None:
        hc = Ref(ph.v * fn(pg.v), hc.slack)
    out = 64.0 * hc.out + h2
    return TailB(hc, out, 64.0 * hc.bound + half_step(out), ph, pg)


def tail_b_model32(m, launch) -> np.ndarray:
    """fp16(64 fp16(hv gelu(gv)) + h2), the kernel's operations in fp32"""
    h2 = tail_b_data(m)[5]
    r = tail_b_reference(m, launch)
    hc = (fold_rows32(h2, r.ph) * gelu32(fold_rows32(h2, r.pg))).astype(np.float16)
    h3 = F32(64) * hc.astype(F32) + h2.astype(F32)
    assert np.array_equal(h3.astype(np.float64), 64.0 * hc.astype(np.float64) + h2)   # (exact in fp32)
    return h3.astype(np.float16)

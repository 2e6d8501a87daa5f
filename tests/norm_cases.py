"""GroupNorm / LayerNorm cases (tests/test_norm_cases_host.py, tests/test_norm_forms_gpu.py): every kernel form of csrc/norm.hip on
data whose groups, images and rows all have DIFFERENT statistics, against float64, with a bound per element.

Exact-statistics data (GroupNorm, groupnorm_addvec).  Every input element is an integer, |x| <= 7.  Within (image b, group g) the
values are m[b, g] + clip(s[b, g] * k, -3, 3): a centre m in -4..4, a spread s in {1, 2}, k from {+-1, +-2, +-3} -- no element sits
on its centre.  Adjacent groups, and the same group of adjacent images, have different centres (hence different (m, s) pairs).  For
addvec the SUM x + a is that lattice and a is a non-zero integer vector in -3..3, different for adjacent images: x, a and x + a are
exact in fp16 and in fp32.  Every partial sum of x and of x^2 is then an integer below 2^24 (hw * cpg * 49 < 2^24 for every case):
S and Q are exact in fp32 in ANY reduction order, and the kernel's only roundings are the handful after the fold -- S / n, Q / n,
mean^2, the subtraction, rsqrt, rstd * gamma, beta - mean * a, x * a + b, the store (and SiLU's exp and rcp).

The bound per element (SiLU off):  |got - ref| <= half an fp16 step of ref + 2^-20 * T,  T = |x a| + |mean a| + |beta|, a = rstd * gamma,
all in float64: the magnitudes of the terms the kernel adds in fp32, 2^-20 = 16 fp32 roundings.  `groupnorm_float32` -- the kernel's
post-fold arithmetic in numpy fp32 -- needs at most a few 2^-24 * T (tests/test_norm_cases_host.py asserts that it is inside the bound
for every case).  SiLU on: T scaled by 1.1 (|silu'| <= 1.1) plus 2^-19 * |ref| for the rounding of the exponential's argument and the
1-ulp exp / rcp (|v| <= 16 in every case).

Mutations: the answers of kernels that are wrong in the ways these kernels can be wrong (a neighbouring group's, image's or row's
statistics; a row missing from the statistics; the concat's second source read one channel early), computed from the same float64
arithmetic.  The host test shows that every one of them breaks the bound on the elements it touches: the data would notice."""
import dataclasses
import functools
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

from exact_cases import ulp_distance  # noqa: F401  (the fp16 step distance the tests report)

F32 = np.float32
EPS = 1e-5
SENT16 = 0x5A5A          # the bits of every sentinel half (tests/test_frame_options_gpu.py)
ADDVEC_PAD = 24          # ld_addvec = C + 24, the padding holds sentinels
BALANCED_BELOW_HW = 16   # below: every group's offsets come in +- pairs (mean exactly m, variance never zero, however few samples);
                         # from here on: the last row of every image lies beyond its groups' centres, away from zero (mutation d)


# ---------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class GnCase:
    name: str
    c0: int
    hw: int
    c1: int = 0
    groups: int = 32
    batch: int = 1
    addvec: bool = False
    launches: int = 1          # what vsd_groupnorm_launches must say (1: gn_fused_kernel, 2: gn_stats_kernel + gn_apply_kernel)
    no_fused: bool = False     # run with VSD_GN_NO_FUSED set: the two-launch form at a shape that would take one launch
    kind: str = "exact"        # "exact" | "ratio16" | "ratio100" (general fp16 data, mean / deviation = 16 or 100)
    reaches: str = ""          # the instantiation or edge this case is here for
    salt: int = 0              # another draw of the same shape (the second member of a pair)

    @property
    def c(self):
        return self.c0 + self.c1

    @property
    def cpg(self):
        return self.c // self.groups

    @property
    def ld_addvec(self):
        return self.c + ADDVEC_PAD


def _gn_table():
    cases = []
    # ---- one-launch form: gn_fused_kernel<VW, NV>, one workgroup per (image, group).  Threads = 64 / 128 / 256 / 1024 for hw <= 64 /
    #      128 / 256 / 1024: both sides of every step; hw = 1: one live lane.  Every shape at batch 1 and 3, plain and addvec.
    one = [(1280, 40, "<8,5>"), (256, 8, "<8,1>"), (512, 16, "<8,2>"), (640, 20, "<4,5>"), (128, 4, "<4,1>"), (384, 12, "<4,3>"),
           (320, 10, "<2,5>"), (64, 2, "<2,1>"), (192, 6, "<2,3>")]
    for c, cpg, inst in one:
        hws = [1, 64, 65, 128, 129, 256] + ([257, 1024] if cpg <= 20 else [])
        for hw in hws:
            for batch in (1, 3):
                for av in (False, True):
                    cases.append(GnCase(f"one-c{c}-hw{hw}-b{batch}{'-av' if av else ''}", c, hw, batch=batch, addvec=av, launches=1,
                                        reaches=f"gn_fused_kernel{inst}, {64 if hw <= 64 else 128 if hw <= 128 else 256 if hw <= 256 else 1024} threads"))
    # cpg = 40 leaves the one-launch form above 256 pixels
    cases.append(GnCase("two-c1280-hw257", 1280, 257, launches=2, reaches="cpg 40 at hw 257: statistics + apply"))
    # a concat boundary INSIDE a group (group 16 of each): the vector that starts at c0 reads the second source's first channels
    for c0, c1, inst in ((648, 632, "<8,5>"), (328, 312, "<4,5>"), (168, 152, "<2,5>")):
        for hw, batch in ((64, 1), (129, 3)):
            cases.append(GnCase(f"one-cat{c0}+{c1}-hw{hw}-b{batch}", c0, hw, c1=c1, batch=batch, launches=1,
                                reaches=f"gn_fused_kernel{inst}, concat boundary inside group 16"))
    # ---- two-launch form, natural shapes
    cases += [
        GnCase("two-c320-hw1025", 320, 1025, launches=2, reaches="rpp 12, 22 statistics workgroups, vectors straddle groups (cpg 10)"),
        GnCase("two-cat320+640-hw100", 320, 100, c1=640, launches=2, reaches="cpg 30, concat, rpp 4"),
        GnCase("two-c1920-hw64", 1920, 64, launches=2, reaches="cpg 60, rpp 2"),
        GnCase("two-cat1280+1280-hw70", 1280, 70, c1=1280, launches=2, reaches="cpg 80, rpp 1, concat"),
        GnCase("two-c64-g1-hw9", 64, 9, groups=1, launches=2, reaches="one group of 64 channels, rpp clipped to hw = 9, fold with 2 pairs"),
        GnCase("two-c320-hw1025-b3-av", 320, 1025, batch=3, addvec=True, launches=2, reaches="gn_stats / gn_apply <true>, per-image part offset"),
        GnCase("two-c1280-hw300-b2-av", 1280, 300, batch=2, addvec=True, launches=2, reaches="gn_stats / gn_apply <true>, cpg 40, rpp 3"),
    ]
    # ---- two-launch form forced (VSD_GN_NO_FUSED) at shapes that take one launch otherwise
    cases += [
        GnCase("forced-c64-hw5", 64, 5, launches=2, no_fused=True, reaches="rpp 64 clipped to hw = 5: 40 threads"),
        GnCase("forced-c320-hw1", 320, 1, launches=2, no_fused=True, reaches="one row: 40 threads fold 64 pairs (nch 0 -> 1)"),
        GnCase("forced-c320-hw47", 320, 47, launches=2, no_fused=True, reaches="rpp 12, one ragged statistics workgroup"),
        GnCase("forced-c2048-g256-hw3", 2048, 3, groups=256, launches=2, no_fused=True, reaches="256 groups: 512 pairs on 512 threads"),
        GnCase("forced-c1280-hw256", 1280, 256, launches=2, no_fused=True, reaches="the shape of one-c1280-hw256-b1 in the other form"),
    ]
    # ---- statistics-workgroup count edges at C = 320 (rpp 12: cdiv(hw, 48) workgroups, capped at max(32, 160 / batch) and GN_MAX_PART)
    cases += [
        GnCase("part-c320-hw4100", 320, 4100, launches=2, reaches="86 statistics workgroups"),
        GnCase("part-c320-hw4100-b5", 320, 4100, batch=5, launches=2, reaches="nblk_cap: 86 capped at 32"),
        GnCase("part-c320-hw6149", 320, 6149, launches=2, reaches="129 -> GN_MAX_PART = 128 workgroups: the fold loop beyond 16 * nch = 112"),
    ]
    # ---- ratio-16 regime (mean 8, deviation 0.5; general fp16 data): the one-pass sums' regression guard
    cases += [
        GnCase("ratio16-c320-hw4100", 320, 4100, launches=2, kind="ratio16"),
        GnCase("ratio16-c640-hw1024", 640, 1024, launches=1, kind="ratio16"),
        GnCase("ratio16-c1280-hw256-b3-av", 1280, 256, batch=3, addvec=True, launches=1, kind="ratio16"),
    ]
    return cases


GN_CASES = _gn_table()
# measured, not asserted (profiles/norm_forms.txt): mean 50, deviation 0.5
RATIO100_CASES = [GnCase(c.name.replace("ratio16", "ratio100"), c.c0, c.hw, batch=c.batch, addvec=c.addvec, launches=c.launches, kind="ratio100")
                  for c in GN_CASES if c.kind == "ratio16"]
# pairs (vsd_pair_begin / join / end): two tensors of one shape, different (m, s) tables, gamma, beta and vectors
PAIR_CASES = [
    (GnCase("pair-one-c1280-hw129", 1280, 129, launches=1, reaches="gn_fused_pair_kernel<8,5,1,false>"), 1),
    (GnCase("pair-one-c320-hw65-b3-av", 320, 65, batch=3, addvec=True, launches=1, reaches="gn_fused_pair_kernel<2,5,1,true>"), 1),
    (GnCase("pair-two-c320-hw1025", 320, 1025, launches=2, reaches="gn_stats_pair_kernel<false>, gn_apply_pair_kernel<false>"), 2),
    (GnCase("pair-two-c1280-hw300-b2-av", 1280, 300, batch=2, addvec=True, launches=2, reaches="gn_stats_pair_kernel<true>, gn_apply_pair_kernel<true>"), 2),
]


def pair_members(c: GnCase):
    """the two tensors of a pair: one shape, the second another draw of everything (salt 1)"""
    return c, dataclasses.replace(c, name=c.name + "-second", salt=1)


PAIR_MEMBERS = [m for p, _ in PAIR_CASES for m in pair_members(p)]
GN_BY_NAME = {c.name: c for c in GN_CASES + RATIO100_CASES + PAIR_MEMBERS}
assert len(GN_BY_NAME) == len(GN_CASES) + len(RATIO100_CASES) + len(PAIR_MEMBERS)

# (rows, C): layernorm_kernel<NCH>, NCH = cdiv(C / 8, 64); one wave per row, four rows per workgroup
LN_CASES = [(5, 8),        # <1>, one live lane, a ragged workgroup
            (7, 520),      # <2>, the second chunk has ONE live lane
            (4, 512),      # <1>, every lane live
            (6, 1032),     # <3>, one live lane in the third chunk
            (9, 1544),     # <4>, one live lane in the fourth chunk
            (3, 2048),     # <4>, every lane live: the largest C
            (77, 768)]     # <2>: the CLIP shape, 20 workgroups, the last ragged
LN_REFUSED = [(4, 2056), (4, 12)]

TAIL_M = [200, 17000]      # 16-row and 80-row tiles of csrc/fused_tail.hip, both ragged
TAIL_BLOCK = 16
TAIL_SCALES = tuple(float(v) for v in np.geomspace(0.25, 4.0, 7))   # period 7: coprime to every tile height (16, 32, 48, 64, 80)


# ---------------------------------------------------------------------------------------------------------------- the data
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _distinct16(v64):
    """fp16 of v with every channel different from the eight before it (a collision moves one fp16 step up)"""
    v = v64.astype(np.float16)
    for i in range(1, len(v)):
        while v[i] in v[max(0, i - 8):i]:
            v[i] = np.nextafter(v[i], np.float16(4.0))
    return v


def gamma_beta(c, *key):
    rng = _rng("gamma-beta", c, *key)
    return _distinct16(1 + 0.1 * rng.standard_normal(c)), _distinct16(0.1 * rng.standard_normal(c))


@dataclass
class GnData:
    src: list                      # per source: fp16 [batch * hw][channels]
    addvec: Optional[np.ndarray]   # fp16 [batch][ld_addvec], sentinels in the padding
    total: np.ndarray              # float64 [batch][hw][C]: what is normalised (concat of the sources, + the image's vector)
    gamma: np.ndarray              # fp16 [C]
    beta: np.ndarray
    m: Optional[np.ndarray]        # int [batch][groups] (exact data)
    s: Optional[np.ndarray]


def _tables(rng, batch, groups):
    """centres in -4..4: adjacent groups differ (a random non-zero step mod 9), adjacent images differ (4 per image mod 9); spreads random"""
    base = np.cumsum(rng.integers(1, 9, size=groups)) + rng.integers(0, 9)
    m = (base[None, :] + 4 * np.arange(batch)[:, None]) % 9 - 4
    s = rng.integers(1, 3, size=(batch, groups))
    return m.astype(np.int64), s.astype(np.int64)


def _offsets(rng, c: GnCase, m, s):
    """int [batch][hw][groups][cpg]: clip(s * k, -3, 3), k non-zero"""
    B, hw, G, cpg = c.batch, c.hw, c.groups, c.cpg
    if hw < BALANCED_BELOW_HW:
        n = hw * cpg  # (even: every cpg is)
        half = rng.integers(1, 4, size=(B, G, n // 2)) * (rng.integers(0, 2, size=(B, G, n // 2)) * 2 - 1)
        k = rng.permuted(np.concatenate([half, -half], axis=-1), axis=-1).reshape(B, G, hw, cpg).transpose(0, 2, 1, 3)
    else:
        k = rng.integers(1, 4, size=(B, hw, G, cpg)) * (rng.integers(0, 2, size=(B, hw, G, cpg)) * 2 - 1)
        # the last row of every image lies beyond its groups' centres, away from zero: |x| >= |m| + 1 for all of it, so that a kernel
        # which loses that row loses a sum of at least cpg (mutation d)
        k[:, -1] = np.abs(k[:, -1]) * np.where(m < 0, -1, 1)[:, :, None]
    return np.clip(s[:, None, :, None] * k, -3, 3)


@functools.lru_cache(maxsize=8)
def gn_data(c: GnCase) -> GnData:
    rng = _rng("gn", c.name if c.kind != "exact" else (c.c0, c.c1, c.hw, c.groups, c.batch, c.addvec), c.salt)
    B, hw, G, cpg, C = c.batch, c.hw, c.groups, c.cpg, c.c
    gamma, beta = gamma_beta(C, c.salt)
    m = s = None
    if c.kind == "exact":
        assert hw * cpg * 49 < 2 ** 24 and (hw * cpg) % 2 == 0
        m, s = _tables(rng, B, G)
        total = (m[:, None, :, None] + _offsets(rng, c, m, s)).reshape(B, hw, C)
        vec = None
        if c.addvec:
            lattice = np.array([-3, -2, -1, 1, 2, 3])
            vec = lattice[(rng.integers(0, 6, size=C)[None, :] + np.arange(B)[:, None]) % 6]   # adjacent images differ in every channel
        x = total - (vec[:, None, :] if c.addvec else 0)
        total = total.astype(np.float64)
    else:
        mean = {"ratio16": 8.0, "ratio100": 50.0}[c.kind] * (rng.integers(0, 2, size=(B, G)) * 2 - 1)
        mean_c = np.repeat(mean, cpg, axis=1)                       # [B][C]
        noise = 0.5 * rng.standard_normal((B, hw, C))
        if c.addvec:   # the vector supplies the mean
            vec, x = mean_c.astype(np.float16), noise.astype(np.float16)
            total = x.astype(np.float64) + vec.astype(np.float64)[:, None, :]
        else:
            vec, x = None, (mean_c[:, None, :] + noise).astype(np.float16)
            total = x.astype(np.float64)
    x16 = np.ascontiguousarray(x.reshape(B * hw, C)).astype(np.float16)
    src = [np.ascontiguousarray(x16[:, :c.c0]), np.ascontiguousarray(x16[:, c.c0:])] if c.c1 else [x16]
    av = None
    if c.addvec:
        av = np.full((B, c.ld_addvec), SENT16, dtype=np.uint16).view(np.float16)
        av[:, :C] = vec.astype(np.float16)
    return GnData(src, av, total, gamma, beta, m, s)


def ln_data(rows, c):
    """-> x fp16 [rows][c], gamma, beta: row r has its own mean in [-4, 4] (all different, a shuffled ladder) and deviation in {0.25, 0.5, 1, 2}"""
    rng = _rng("ln", rows, c)
    mean = rng.permutation(np.linspace(-4.0, 4.0, rows))
    dev = np.array([0.25, 0.5, 1.0, 2.0])[(np.arange(rows) + rng.integers(0, 4)) % 4]
    x = (mean[:, None] + dev[:, None] * rng.standard_normal((rows, c))).astype(np.float16)
    return (x,) + gamma_beta(c, "ln", rows)


def tail_rows(m, c, seed):
    """fp16 [m][c]: row r = mean_r + scale_r * N(0, 1), scale of period 7 over TAIL_SCALES, mean_r uniform in [-4, 4]"""
    rng = _rng("tail", m, c, seed)
    scale = np.array(TAIL_SCALES)[np.arange(m) % 7]
    mean = rng.uniform(-4.0, 4.0, m)
    return (mean[:, None] + scale[:, None] * rng.standard_normal((m, c))).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- the reference
def silu64(v):
    return v / (1.0 + np.exp(-v))


def half_step(ref):
    """half the fp16 spacing at |ref| (2^-25 below the smallest normal)"""
    f, e = np.frexp(np.abs(ref))                      # |ref| = f 2^e, f in [0.5, 1); zero: f = 0
    return 0.5 * np.ldexp(1.0, np.where(f > 0, np.maximum(e - 11, -24), -24))


@dataclass
class Ref:
    pre: np.ndarray    # float64, before SiLU
    t: np.ndarray      # float64: |x a| + |mean a| + |beta|
    mean: np.ndarray   # float64 [batch][groups] (LayerNorm: [rows][1])
    rstd: np.ndarray

    def out(self, silu):
        return silu64(self.pre) if silu else self.pre

    def bound(self, silu):
        if not silu:
            return half_step(self.pre) + 2.0 ** -20 * self.t
        ref = silu64(self.pre)
        return half_step(ref) + 2.0 ** -20 * 1.1 * self.t + 2.0 ** -19 * np.abs(ref)


def _normalise(x, mean, rstd, gamma, beta):
    """x, mean, rstd: float64 [..][groups][cpg] / [..][groups][1]; gamma, beta: [groups][cpg]"""
    a = rstd * gamma
    return (x - mean) * a + beta, np.abs(x * a) + np.abs(mean * a) + np.abs(beta)


def gn_reference(total, groups, gamma16, beta16, eps=EPS) -> Ref:
    """float64 GroupNorm of total [batch][hw][C]; eps as the kernel holds it: float64(float32(eps))"""
    B, hw, C = total.shape
    cpg = C // groups
    x = total.reshape(B, hw, groups, cpg)
    mean = x.mean(axis=(1, 3), keepdims=True)
    var = x.var(axis=(1, 3), keepdims=True)   # (two passes in float64)
    rstd = 1.0 / np.sqrt(var + np.float64(F32(eps)))
    g, b = gamma16.astype(np.float64).reshape(groups, cpg), beta16.astype(np.float64).reshape(groups, cpg)
    pre, t = _normalise(x, mean, rstd, g, b)
    return Ref(pre.reshape(B * hw, C), t.reshape(B * hw, C), mean.reshape(B, groups), rstd.reshape(B, groups))


def ln_reference(x16, gamma16, beta16, eps=EPS) -> Ref:
    x = x16.astype(np.float64)
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=1, keepdims=True) + np.float64(F32(eps)))
    pre, t = _normalise(x, mean, rstd, gamma16.astype(np.float64), beta16.astype(np.float64))
    return Ref(pre, t, mean, rstd)


def case_reference(c: GnCase, d: GnData) -> Ref:
    return gn_reference(d.total, c.groups, d.gamma, d.beta)


def violations(got, ref: Ref, silu):
    """bool per element: outside the bound (a non-finite value is outside)"""
    err = np.abs(got.astype(np.float64) - ref.out(silu))
    return ~(err <= ref.bound(silu))


def survey_blocks(got, want, block_rows, block_cols):
    """SURVEY 8c per block: (largest max-abs / (2^-8 max|ref| + 1e-6), largest rel-L2) over blocks of [block_rows][block_cols]"""
    r, c = want.shape
    nr = -(-r // block_rows)
    worst_abs = worst_l2 = 0.0
    for i in range(nr):
        g = got[i * block_rows:(i + 1) * block_rows].astype(np.float64)
        w = want[i * block_rows:(i + 1) * block_rows]
        g, w = g.reshape(g.shape[0], c // block_cols, block_cols), w.reshape(w.shape[0], c // block_cols, block_cols)
        err = np.abs(g - w).max(axis=(0, 2)) / (2.0 ** -8 * np.abs(w).max(axis=(0, 2)) + 1e-6)
        l2 = np.sqrt(((g - w) ** 2).sum(axis=(0, 2)) / ((w * w).sum(axis=(0, 2)) + 1e-24))
        worst_abs, worst_l2 = max(worst_abs, float(err.max())), max(worst_l2, float(l2.max()))
    return worst_abs, worst_l2


# ---------------------------------------------------------------------------------------------------------------- the fp32 models
def _silu32(v):
    with np.errstate(over="ignore"):
        return v * (F32(1) / (F32(1) + np.exp(-v)))


def groupnorm_float32(total, groups, gamma16, beta16, silu, eps=EPS) -> np.ndarray:
    """The kernels' arithmetic after the fold (gn_apply_body / gn_fused_body), operation by operation in fp32.  S and Q are summed
    here in float64 and rounded once: for exact-statistics data that is what ANY fp32 summation order gives."""
    B, hw, C = total.shape
    cpg = C // groups
    x = total.reshape(B, hw, groups, cpg)
    S = x.sum(axis=(1, 3), keepdims=True).astype(F32)
    Q = (x * x).sum(axis=(1, 3), keepdims=True).astype(F32)
    n = F32(hw) * F32(cpg)
    mean = S / n
    var = np.maximum(Q / n - mean * mean, F32(0))
    rstd = F32(1) / np.sqrt(var + F32(eps))
    a = rstd * gamma16.astype(F32).reshape(groups, cpg)
    b = beta16.astype(F32).reshape(groups, cpg) - mean * a
    v = x.astype(F32) * a + b
    assert v.dtype == F32
    return (_silu32(v) if silu else v).astype(np.float16).reshape(B * hw, C)


def layernorm_float32(x16, gamma16, beta16, eps=EPS) -> np.ndarray:
    """layernorm_kernel in fp32: the mean first, then the squared distances to it (numpy's pairwise sums for the wave's)"""
    x = x16.astype(F32)
    c = F32(x.shape[1])
    mean = x.sum(axis=1, keepdims=True, dtype=F32) / c
    d = x - mean
    rstd = F32(1) / np.sqrt((d * d).sum(axis=1, keepdims=True, dtype=F32) / c + F32(eps))
    return (d * rstd * gamma16.astype(F32) + beta16.astype(F32)).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- the mutations
# Each returns (the wrong kernel's pre-SiLU answer in float64 [rows][C], bool [rows][C]: the elements it touches) or None where the case
# gives it nothing to get wrong.
def _regroup(c: GnCase, d: GnData, ref: Ref):
    B, hw, G, cpg = c.batch, c.hw, c.groups, c.cpg
    g = d.gamma.astype(np.float64).reshape(G, cpg)
    b = d.beta.astype(np.float64).reshape(G, cpg)
    return d.total.reshape(B, hw, G, cpg), ref.mean.reshape(B, 1, G, 1), ref.rstd.reshape(B, 1, G, 1), g, b


def mut_next_group_stats(c: GnCase, d: GnData, ref: Ref):
    """(a) the last channel of group g normalised with group g + 1's (mean, rstd)"""
    if c.groups < 2:
        return None
    x, mean, rstd, g, b = _regroup(c, d, ref)
    out = ref.pre.reshape(x.shape).copy()
    out[:, :, :-1, -1] = (x[:, :, :-1, -1] - mean[:, :, 1:, 0]) * rstd[:, :, 1:, 0] * g[:-1, -1] + b[:-1, -1]
    hit = np.zeros(x.shape, dtype=bool)
    hit[:, :, :-1, -1] = True
    return out.reshape(ref.pre.shape), hit.reshape(ref.pre.shape)


def mut_next_image_stats(c: GnCase, d: GnData, ref: Ref):
    """(b) image b normalised with image b + 1's statistics"""
    if c.batch < 2:
        return None
    x, mean, rstd, g, b = _regroup(c, d, ref)
    out = ref.pre.reshape(x.shape).copy()
    out[:-1] = (x[:-1] - mean[1:]) * (rstd[1:] * g) + b
    hit = np.zeros(x.shape, dtype=bool)
    hit[:-1] = True
    return out.reshape(ref.pre.shape), hit.reshape(ref.pre.shape)


def mut_next_row_stats(x16, gamma16, beta16, ref: Ref):
    """(c) LayerNorm row r normalised with row r + 1's statistics"""
    if x16.shape[0] < 2:
        return None
    x = x16.astype(np.float64)
    out = ref.pre.copy()
    out[:-1] = (x[:-1] - ref.mean[1:]) * ref.rstd[1:] * gamma16.astype(np.float64) + beta16.astype(np.float64)
    hit = np.zeros(x.shape, dtype=bool)
    hit[:-1] = True
    return out, hit


def mut_drop_last_row(c: GnCase, d: GnData, ref: Ref):
    """(d) the last row of every image missing from the statistics (the divisor still hw * cpg rows' worth: the kernel's n)"""
    if c.hw < 2:
        return None
    G, cpg = c.groups, c.cpg
    x = d.total.reshape(c.batch, c.hw, G, cpg)
    n = c.hw * cpg
    sx = x[:, :-1]
    mean = sx.sum(axis=(1, 3), keepdims=True) / n
    var = np.maximum((sx * sx).sum(axis=(1, 3), keepdims=True) / n - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + np.float64(F32(EPS)))
    pre, _ = _normalise(x, mean, rstd, d.gamma.astype(np.float64).reshape(G, cpg), d.beta.astype(np.float64).reshape(G, cpg))
    return pre.reshape(ref.pre.shape), np.ones(ref.pre.shape, dtype=bool)


def mut_concat_early(c: GnCase, d: GnData, ref: Ref):
    """(e) the second source read one half early: its channel j is its channel j - 1, channel 0 the previous row's last (row 0: as it
    should be).  Touched: the elements whose input changed (the rest of their groups moves with the statistics, by much less)."""
    if not c.c1:
        return None
    s1 = d.src[1].astype(np.float64)
    flat = s1.reshape(-1)
    early = np.concatenate([flat[:1], flat[:-1]]).reshape(s1.shape)
    early[0, 0] = s1[0, 0]
    total = np.concatenate([d.src[0].astype(np.float64), early], axis=1).reshape(c.batch, c.hw, c.c)
    wrong = gn_reference(total, c.groups, d.gamma, d.beta)
    return wrong.pre, (total != d.total).reshape(ref.pre.shape)


GN_MUTATIONS = {"a": mut_next_group_stats, "b": mut_next_image_stats, "d": mut_drop_last_row, "e": mut_concat_early}
# (d) is judged where the data is built for it: from BALANCED_BELOW_HW rows on the last row's values are all at least 1 from zero, on
# one side (below, a last row may be all zeros: losing it loses nothing).  Losing it moves a group's mean by (|m| + about 2.3) / hw and
# the output by at least 0.4 gamma / hw: beyond a thousand rows that is below the fp16 step of most outputs -- no test of fp16 outputs
# can see one missing row of 6149.
DROP_ROW_HW = (BALANCED_BELOW_HW, 1100)
# (a), (b), (e) must show on every element they touch ((a), (b): but for the one x at which the right and the wrong line cross, should that
# be an integer of the group) once a group has this many samples.  With fewer the outputs themselves are too
# few to tell: two samples normalise to +-1 whatever their mean and spread, so a neighbour's statistics that also map x to +-1 -- x is
# one of the neighbour's two values -- give the right answer.
ALL_TOUCHED_FROM_SAMPLES = 64

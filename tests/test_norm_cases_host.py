"""The GroupNorm / LayerNorm case table of tests/norm_cases.py, checked on the CPU: the data is what its header promises (integers,
bounds, exact sums, neighbours with different statistics), a correct fp32 kernel -- the committed numpy model of one -- is inside the
bound, and every way these kernels can be wrong (norm_cases' mutations) is outside it on the elements it touches.  The last is the point:
it shows that tests/test_norm_forms_gpu.py would notice."""
import numpy as np
import pytest

import norm_cases as N

EXACT = [c for c in N.GN_CASES + N.PAIR_MEMBERS if c.kind == "exact"]
GENERAL = [c for c in N.GN_CASES + N.RATIO100_CASES if c.kind != "exact"]
ids = lambda cases: [c.name for c in cases]  # noqa: E731


def test_the_table_reaches_every_form():
    """by (C, groups, hw, batch, concat, addvec): the nine one-launch instantiations, the two-launch form natural, forced, capped and with
    more than 112 partials, and the four layernorm_kernel instantiations"""
    one = {(c.cpg, c.hw) for c in N.GN_CASES if c.launches == 1 and c.kind == "exact" and not c.c1}
    for cpg in (40, 8, 16, 20, 4, 12, 10, 2, 6):
        want = {1, 64, 65, 128, 129, 256} | ({257, 1024} if cpg <= 20 else set())
        assert {hw for g, hw in one if g == cpg} == want, cpg
        for hw in want:
            combos = {(c.batch, c.addvec) for c in N.GN_CASES if c.launches == 1 and c.cpg == cpg and c.hw == hw and not c.c1 and c.kind == "exact"}
            assert combos == {(1, False), (1, True), (3, False), (3, True)}, (cpg, hw)
    assert {(c.c0, c.c1) for c in N.GN_CASES if c.c1 and c.launches == 1} == {(648, 632), (328, 312), (168, 152)}
    for c in N.GN_CASES:
        if c.c1 and c.launches == 1:
            assert c.c0 % c.cpg != 0   # the boundary is inside a group
    two = [c for c in N.GN_CASES if c.launches == 2 and c.kind == "exact"]
    assert any(c.no_fused for c in two) and any(not c.no_fused for c in two)
    assert {c.cpg for c in two} >= {10, 30, 40, 60, 64, 80, 8, 2}
    assert any(c.groups == 1 for c in two) and any(c.groups == 256 for c in two)
    rpp = lambda c: min(c.hw, max(1, 512 // (c.c // 8)))  # noqa: E731  (csrc/norm.hip gn_run)
    nblk = lambda c: min(-(-c.hw // (4 * rpp(c))), max(32, 160 // c.batch), 128)  # noqa: E731
    counts = {c.name: (-(-c.hw // (4 * rpp(c))), nblk(c)) for c in two}
    assert counts["part-c320-hw4100"] == (86, 86) and counts["part-c320-hw4100-b5"] == (86, 32) and counts["part-c320-hw6149"] == (129, 128)
    assert 128 > 16 * ((40 * 12) // 64)   # C = 320: 480 threads, 64 pairs -> nch 7: partials 112.. take the fold's tail loop
    assert any(c.addvec and c.batch > 1 for c in two)
    assert {-(-(c // 8) // 64) for _, c in N.LN_CASES} == {1, 2, 3, 4}
    assert any((c // 8) % 64 == 1 for _, c in N.LN_CASES)   # a chunk with a single live lane
    assert {(c.launches, c.addvec) for c, _ in N.PAIR_CASES} == {(1, False), (1, True), (2, False), (2, True)}
    assert all(n == c.launches for c, n in N.PAIR_CASES)


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_exact_statistics_case(case):
    c, d = case, N.gn_data(case)
    B, hw, G, cpg, C = c.batch, c.hw, c.groups, c.cpg, c.c
    # ---- the exactness conditions
    x = np.concatenate([s.astype(np.float64) for s in d.src], axis=1)
    assert x.shape == (B * hw, C) and np.array_equal(x, np.rint(x))
    tot = d.total
    assert np.array_equal(tot, np.rint(tot)) and np.abs(tot).max() <= 7
    if c.addvec:
        vec = d.addvec[:, :C].astype(np.float64)
        assert np.array_equal(vec, np.rint(vec)) and vec.min() >= -3 and vec.max() <= 3 and not (vec == 0).any()
        assert np.array_equal(x.reshape(B, hw, C) + vec[:, None, :], tot) and np.abs(x).max() <= 10
        assert (vec[1:] != vec[:-1]).all()                                    # adjacent images: another vector in every channel
        assert (d.addvec[:, C:].view(np.uint16) == N.SENT16).all() and d.addvec.shape[1] == C + N.ADDVEC_PAD
    else:
        assert np.array_equal(x.reshape(B, hw, C), tot)
    off = tot.reshape(B, hw, G, cpg) - d.m[:, None, :, None]
    assert np.abs(off).max() <= 3 and np.abs(off).min() >= 1                  # no element on its centre
    assert np.abs(d.m).max() <= 4 and set(np.unique(d.s)) <= {1, 2}
    assert hw * cpg * 49 < 2 ** 24 and (tot.reshape(B, hw, G, cpg) ** 2).sum(axis=(1, 3)).max() < 2 ** 24
    # ---- the distinctness conditions
    assert (d.m[:, 1:] != d.m[:, :-1]).all() and (d.m[1:] != d.m[:-1]).all()
    for v in (d.gamma, d.beta):
        assert all((v[k:] != v[:-k]).all() for k in range(1, min(8, C - 1) + 1))
    ref = N.case_reference(c, d)
    if G > 1:   # ... and they show in the statistics themselves, not only in the tables
        assert (np.abs(ref.mean[:, 1:] - ref.mean[:, :-1]) > 0.25).all()
    if B > 1:
        assert (np.abs(ref.mean[1:] - ref.mean[:-1]) > 0.25).all()
    mutants = {name: mutate(c, d, ref) for name, mutate in N.GN_MUTATIONS.items()}
    assert (mutants["a"] is not None) == (G > 1) and (mutants["b"] is not None) == (B > 1) and (mutants["e"] is not None) == bool(c.c1)
    for silu in (False, True):
        want, bound = ref.out(silu), ref.bound(silu)
        # ---- the fp32 model of a correct kernel is inside the bound, and almost always on the float64 answer's own fp16 value
        model = N.groupnorm_float32(tot, G, d.gamma, d.beta, silu)
        assert (np.abs(model.astype(np.float64) - want) <= bound).all(), silu
        with np.errstate(over="ignore"):
            steps = N.ulp_distance(model, want.astype(np.float16))
        assert steps.max() <= 1 and (steps != 0).mean() <= 0.01, (silu, steps.max(), (steps != 0).mean())
        # ---- every mutation is outside it
        for name, m in mutants.items():
            if m is None or (name == "d" and not N.DROP_ROW_HW[0] <= hw <= N.DROP_ROW_HW[1]):
                continue
            wrong, hit = m
            assert hit.any(), name
            got = N.silu64(wrong) if silu else wrong
            bad = ~(np.abs(got - want) <= bound)
            missed = (int((~bad[hit]).sum()), int(hit.sum()))
            if name == "d":   # every (image, group) shows it
                assert bad.reshape(B, hw, G, cpg).any(axis=(1, 3)).all(), (name, silu)
            elif not silu and hw * cpg >= N.ALL_TOUCHED_FROM_SAMPLES and name == "e":
                assert bad[hit].all(), (name, silu, missed)
            elif not silu and hw * cpg >= N.ALL_TOUCHED_FROM_SAMPLES:
                # the right and the wrong statistics are two different lines in x: they cross at ONE x at most, and where that x is one
                # of the group's (at most seven) integers the two agree there -- one-c384-hw64-b3: (1 + 2.150) 0.4698 = (1 + 2.978) 0.3721.
                # So: within an (image, group) everything missed has one and the same x, and it is rare.
                miss = (hit & ~bad).reshape(B, hw, G, cpg)
                levels = sum(((miss & (tot.reshape(B, hw, G, cpg) == v)).any(axis=(1, 3))).astype(int) for v in range(-7, 8))
                assert levels.max() <= 1 and bad[hit].mean() >= 0.99, (name, silu, missed)
            elif not silu:
                assert bad[hit].mean() >= 0.75, (name, silu, missed)
            else:
                # SiLU is not one-to-one (it turns at v = -1.28: silu(-1) = silu(-1.6)) and a channel of this data takes six values per
                # image: a wrong v that lands on the right output takes a sixth of its channel with it.  (Every case also runs without.)
                assert bad[hit].mean() >= (0.9 if hw * cpg >= N.ALL_TOUCHED_FROM_SAMPLES else 0.6), (name, silu, missed)


@pytest.mark.parametrize("case", GENERAL, ids=ids(GENERAL))
def test_large_mean_case(case):
    c, d = case, N.gn_data(case)
    ratio = {"ratio16": 16.0, "ratio100": 100.0}[c.kind]
    ref = N.case_reference(c, d)
    assert np.allclose(np.abs(ref.mean) * ref.rstd, ratio, rtol=0.05)
    sign = np.sign(ref.mean)
    assert (sign == 1).any() and (sign == -1).any()
    if c.addvec:
        assert np.abs(d.src[0].astype(np.float64)).max() < 4 and np.abs(d.addvec[:, :c.c].astype(np.float64)).min() >= 8
    # a kernel with the neighbouring image's or group's statistics where the sign differs is off by 2 * ratio deviations: far outside
    # the tolerance of the block it happens in
    for name in ("a", "b"):
        m = N.GN_MUTATIONS[name](c, d, ref)
        if m is None:
            continue
        wrong, hit = m
        a, l2 = N.survey_blocks(wrong, ref.pre, c.hw, c.cpg)
        assert a > 1.0 and l2 > 2e-3, (name, a, l2)
    a, l2 = N.survey_blocks(ref.pre.astype(np.float16), ref.pre, c.hw, c.cpg)
    assert a <= 1.0 and l2 <= 2e-3   # the float64 answer's fp16 rounding is inside (with room: l2 is about 3e-4)


@pytest.mark.parametrize("rows,c", N.LN_CASES)
def test_layernorm_case(rows, c):
    x, gamma, beta = N.ln_data(rows, c)
    ref = N.ln_reference(x, gamma, beta)
    assert x.shape == (rows, c) and np.isfinite(x.astype(np.float64)).all()
    assert np.abs(ref.mean).max() < 6 and len(np.unique(ref.mean)) == rows    # every row its own mean ...
    ratio = ref.rstd[1:, 0] / ref.rstd[:-1, 0]
    assert c < 64 or ((ratio > 1.5) | (ratio < 1 / 1.5)).all()                # ... and a deviation that is not the next row's
    model = N.layernorm_float32(x, gamma, beta)
    assert not N.violations(model, ref, False).any()
    wrong, hit = N.mut_next_row_stats(x, gamma, beta, ref)
    bad = ~(np.abs(wrong - ref.pre) <= ref.bound(False))
    # general data: at the one x per row where the two lines (x - m) r and (x - m') r' cross nothing can be seen -- c = 8 has 8 elements
    # per row, all the others at least 99 in 100
    assert bad[:-1].any(axis=1).all() and bad[hit].mean() >= (0.99 if c > 8 else 0.75), bad[hit].mean()


def test_tail_rows_have_their_own_scale_and_mean():
    x = N.tail_rows(200, 320, 2).astype(np.float64)
    sd, mean = x.std(axis=1), x.mean(axis=1)
    assert np.allclose(sd / np.array(N.TAIL_SCALES)[np.arange(200) % 7], 1.0, atol=0.25)
    assert np.abs(mean).max() < 4.5 and np.abs(np.diff(mean)).min() > 0 and len(N.TAIL_SCALES) == 7
    assert all(np.gcd(7, t) == 1 for t in (16, 32, 48, 64, 80))


def test_bound_and_half_step():
    v = np.array([1.0, 1.5, 0.999, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0, 2048.0])
    want = np.array([2.0 ** -11, 2.0 ** -11, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -10, 1.0])
    assert np.array_equal(N.half_step(v), want)
    for x in v[:5]:   # half a step is what rounding to fp16 can cost, and no more
        assert abs(float(np.float16(x * (1 + 2.0 ** -12))) - x * (1 + 2.0 ** -12)) <= N.half_step(np.array([x * (1 + 2.0 ** -12)]))[0]

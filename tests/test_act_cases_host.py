"""The conditions under which tests/test_act_forms_gpu.py may judge the non-linear epilogues per element (no GPU): for every case of
tests/act_cases.py the pre-activation is exact (every partial sum below 2^24 units of 2^-s, no operand zero, every operand exact in
fp16), it covers the region where the activations differ, the fp32 model of the kernel's arithmetic sits within HALF the slack the
bound grants above half an fp16 step, and every mutation -- the answer of a kernel that is wrong in a way these epilogues can be wrong
-- breaks the bound on at least 5 % of the elements of every case it applies to."""
import numpy as np
import pytest
import torch

import act_cases as A

EXACT = float(2 ** 24)


def _is_fp16(t):
    return np.array_equal(t.astype(np.float16).astype(np.float64), t)


def _unique_data(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.data or c.name, c.cout, c.h, c.batch, c.s, c.act, c.out_scale, c.residual, c.residual2, c.t_col0)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


CONV = _unique_data(A.CONV_CASES)   # (scale_dev, out2 and the forms change nothing of the arithmetic judged here)


def test_the_reduced_table_leaves_no_arithmetic_out():
    assert {(c.act, c.out_scale, c.residual2, c.t_col0 is not None, c.thin, c.cout % 8 == 0) for c in CONV} == \
           {(c.act, c.out_scale, c.residual2, c.t_col0 is not None, c.thin, c.cout % 8 == 0) for c in A.CONV_CASES}


@pytest.mark.parametrize("case", A.CONV_CASES, ids=lambda c: c.name)
def test_the_pre_activation_is_exact_and_covers_the_region_where_the_functions_differ(case):
    c, d = case, A.conv_data(case)
    x, big = A.preactivation(c, d)
    assert big.max() < EXACT, "a partial sum could leave fp32's integers"
    assert (x * 2.0 ** c.s == np.rint(x * 2.0 ** c.s)).all()
    for s in d.src:
        assert (s != 0).all() and np.abs(s).max() <= 3
    assert (d.weight != 0).all() and np.abs(d.weight).max() <= 2 * 2.0 ** -c.s
    for t in (d.weight, d.bias, d.rowvec, d.residual, d.residual2, d.add2):
        assert t is None or ((t != 0).all() and _is_fp16(t))
    assert np.log2(c.out_scale) == int(np.log2(c.out_scale))
    # what the activation is evaluated on (x * sc + the residuals with VSD_ACT_POST) is exact in fp32 and covers the region
    arg = A.argument(c, d, x)
    assert np.array_equal(arg.astype(np.float32).astype(np.float64), arg)
    assert np.abs(x).max() <= A.X_MAX and np.abs(arg).max() <= A.X_MAX
    if c.act & 0xff == A.ACT_QUICKGELU:
        assert 1.702 * np.abs(arg).max() <= A.QUICK_ARG_MAX
    low, small = float((arg <= -3).mean()), float((np.abs(arg) <= 0.5).mean())
    assert low >= 0.04 and small >= 0.10, (low, small)
    ref = A.conv_reference(c)[1]
    assert np.isfinite(ref.out).all()


def test_some_cases_store_fp16_subnormals():
    """outputs below 2^-14 (expected stored, not flushed): in the cases without a residual, and among the softmax probabilities"""
    n = sum(int(((np.abs(A.conv_reference(c)[1].out) < 2.0 ** -14) & (np.abs(A.conv_reference(c)[1].out) > 2.0 ** -25)).sum()) for c in CONV)
    assert n >= 100, n
    sm = A.softmax_reference(A.SOFTMAX_CASES[0], 77).out
    assert ((sm < 2.0 ** -14) & (sm > 2.0 ** -25)).sum() >= 100


@pytest.mark.parametrize("case", CONV, ids=lambda c: c.name)
def test_the_fp32_model_sits_within_half_the_slack(case):
    c, d = case, A.conv_data(case)
    x, ref = A.conv_reference(c)
    v = A.epilogue32(c, d, x)
    err = np.abs(v.astype(np.float64) - ref.out)
    inside = err <= 0.5 * ref.slack
    assert inside.all(), f"{c.name}: the fp32 model is outside half the slack on {int((~inside).sum())} elements, first at x = {x[~inside][0]}: {err[~inside][0]:.3g} > {0.5 * ref.slack[~inside][0]:.3g}"
    with np.errstate(over="ignore"):
        assert not A.violations(v.astype(np.float16), ref).any()


def test_the_erf_model_is_two_fp16_steps_off_in_the_negative_tail_and_inside_the_bound():
    """why the erf-GELU bound is absolute in |x| and not "one fp16 step": on a grid of x in [-5.5, -3.8] the kernel's arithmetic lands
    two steps from float64, with an absolute error below 2.4e-7 |x|"""
    x = np.arange(-5.5, -3.8, 2.0 ** -10)
    got, want = A.gelu32(x.astype(np.float32)), A.gelu64(x)
    assert A.ulp_distance(got.astype(np.float16), want.astype(np.float16)).max() >= 2
    assert (np.abs(got - want) <= 2.4e-7 * np.abs(x)).all()
    assert (np.abs(got - want) <= 0.5 * A.act_slack(A.ACT_GELU, x, want)).all()


@pytest.mark.parametrize("case", CONV, ids=lambda c: c.name)
def test_every_mutation_breaks_the_bound_on_a_twentieth_of_the_case(case):
    c, d = case, A.conv_data(case)
    x, ref = A.conv_reference(c)
    applied = 0
    for name, (applies, wrong) in A.CONV_MUTATIONS.items():
        if not applies(c):
            continue
        applied += 1
        with np.errstate(over="ignore"):
            got = wrong(c, d, x).astype(np.float16)
        share = float(A.violations(got, ref).mean())
        assert share >= A.MUTATION_SHARE, f"{c.name}: '{name}' is outside the bound on {share:.1%} of the elements only"
    assert applied or (c.act == A.ACT_SILU and c.out_scale == 1.0 and (not (c.residual or c.residual2) or c.t_col0 is not None))


def test_mutation_shares_on_a_uniform_grid():
    """x in [-8, 8] in steps of 1/64, no scale, no residual: the shares beyond the bound (26 % tanh, 78 % quick <-> erf, 50 % 1.7,
    99.8 % SiLU for quick-GELU on the CPU this was written on)"""
    x = np.arange(-8.0, 8.0 + 2.0 ** -7, 2.0 ** -6)

    def share(kind, wrong):
        a = A.ACT64[kind](x)
        ref = A.Ref(a, A.act_slack(kind, x, a))
        return float(A.violations(wrong(x).astype(np.float16), ref).mean())
    assert share(A.ACT_GELU, A.gelu_tanh64) >= 0.2
    assert share(A.ACT_GELU, A.quick64) >= 0.7 and share(A.ACT_QUICKGELU, A.gelu64) >= 0.7
    assert share(A.ACT_QUICKGELU, lambda v: A.quick64(v, 1.7)) >= 0.4
    assert share(A.ACT_QUICKGELU, A.silu64) >= 0.99


# ---------------------------------------------------------------------------------------------------------------- GEGLU, softmax
@pytest.mark.parametrize("case", A.GEGLU_CASES + A.SOFTMAX_CASES, ids=lambda c: c.name)
def test_linear_cases_are_exact(case):
    a, w, b = A.lin_data(case)
    x, big = A.lin_pre(case)
    assert big.max() < EXACT and (x * 2.0 ** case.s == np.rint(x * 2.0 ** case.s)).all()
    assert (w != 0).all() and (b != 0).all() and all(_is_fp16(t) for t in (a, w, b))
    lattice = np.ones(case.m, dtype=bool)
    if A.has_special(case):   # three rows of chosen scores, through three input channels of their own: the only zeros
        lattice[list(A.SPECIAL_ROWS)] = False
        assert (a[lattice][:, :-3] != 0).all() and not a[lattice][:, -3:].any()
        assert np.array_equal(a[~lattice][:, -3:], np.eye(3)) and not a[~lattice][:, :-3].any()
        assert np.array_equal(x[~lattice], A.special_targets(case.n)) and np.abs(x[~lattice]).max() <= 32
        for cols in A.SOFTMAX_COLS:
            sp = A.softmax64(x, cols)[~lattice].reshape(3, -1, 128)
            assert np.array_equal(sp[0, :, :cols].astype(np.float16), np.full(sp[0, :, :cols].shape, np.float16(1.0 / cols)))
            assert (sp[1, :, 0].astype(np.float16) == 1).all() and not sp[1, :, 1:].astype(np.float16).any()
            assert cols < 10 or (np.diff(sp[2, :, :10], axis=-1) < 0).all()
    else:
        assert (a != 0).all()
    assert np.abs(x[lattice]).max() <= A.X_MAX
    assert case.n % 128 == 0
    if case.kind == A.ACT_GEGLU:
        g = x[:, case.n // 2:]
        low, small = float((g <= -3).mean()), float((np.abs(g) <= 0.5).mean())
        assert low >= 0.04 and small >= 0.10, (low, small)


@pytest.mark.parametrize("case", A.GEGLU_CASES, ids=lambda c: c.name)
def test_geglu_model_and_mutations(case):
    x, _ = A.lin_pre(case)
    ref = A.geglu_reference(case)
    err = np.abs(A.geglu32(x).astype(np.float64) - ref.out)
    assert (err <= 0.5 * ref.slack).all(), float((err / ref.slack).max())
    for name, wrong in A.GEGLU_MUTATIONS.items():
        share = float(A.violations(wrong(x).astype(np.float16), ref).mean())
        assert share >= A.MUTATION_SHARE, f"{case.name}: '{name}' is outside the bound on {share:.1%} of the elements only"


def test_the_geglu_reference_is_the_packed_layouts():
    """act_cases.geglu64 reads hidden and gate as the networks hold them ([0, n/2) and [n/2, n)); the GPU test uploads
    packing.pack_geglu's tiles: 64 hidden rows and their 64 gate rows per 128 -- the emulator of tests/fake_ops.py unpacks them"""
    from videosd_amd.packing import pack_geglu

    c = A.GEGLU_CASES[1]
    a, w, b = A.lin_data(c)
    p = pack_geglu(torch.from_numpy(w).float(), torch.from_numpy(b).float())
    y = (torch.from_numpy(a) @ p.weight[:, :p.k].double().T + p.bias.double()).numpy().reshape(c.m, c.n // 128, 2, 64)
    x, _ = A.lin_pre(c)
    assert np.array_equal(y[:, :, 0].reshape(c.m, -1), x[:, :c.n // 2]) and np.array_equal(y[:, :, 1].reshape(c.m, -1), x[:, c.n // 2:])


@pytest.mark.parametrize("cols", A.SOFTMAX_COLS)
@pytest.mark.parametrize("case", A.SOFTMAX_CASES, ids=lambda c: c.name)
def test_softmax_model_and_mutations(case, cols):
    x, _ = A.lin_pre(case)
    ref = A.softmax_reference(case, cols)
    assert np.allclose(ref.out.reshape(case.m, -1, 128).sum(-1), 1.0, atol=1e-12) and not ref.out.reshape(case.m, -1, 128)[:, :, cols:].any()
    got = A.softmax32(x, cols)
    err = np.abs(got.astype(np.float64) - ref.out)
    assert (err <= 0.5 * ref.slack).all(), float((err / np.maximum(ref.slack, 1e-300)).max())
    assert not got.reshape(case.m, -1, 128)[:, :, cols:].any()
    if cols == 1:
        assert (got.reshape(case.m, -1, 128)[:, :, 0] == 1).all()
    for name, (where, wrong) in A.SOFTMAX_MUTATIONS.items():
        if cols in where:
            share = float(A.violations(wrong(case, cols).astype(np.float16), ref).mean())
            assert share >= A.MUTATION_SHARE, f"{case.name} cols {cols}: '{name}' is outside the bound on {share:.1%} of the elements only"


# ---------------------------------------------------------------------------------------------------------------- folded LayerNorm
def _ln_pack(c):
    from videosd_amd.packing import pack_geglu_ln, pack_linear_ln

    h, gamma, beta, w, bias = (None if t is None else torch.from_numpy(t).float() for t in A.ln_data(c))
    if c.kind == "geglu":
        return pack_geglu_ln(w, bias, gamma.half(), beta.half())
    return pack_linear_ln([w], None if bias is None else [bias], gamma.half(), beta.half())


@pytest.mark.parametrize("case", A.LN_CASES, ids=lambda c: c.name)
def test_layernorm_rows_and_the_fold_are_exact(case):
    c = case
    h, gamma, beta, w, bias = A.ln_data(c)
    p = A.ln_fold(c)
    assert (h == np.rint(h)).all() and np.abs(h).max() <= (51 if c.centre else 7) and all(_is_fp16(t) for t in (h, gamma, beta, w, w * gamma))
    assert (w != 0).all() and (beta != 0).all() and set(np.unique(gamma)) <= {0.5, 1.0, 2.0}
    assert (h * h).sum(axis=1).max() < EXACT and p.big.max() < EXACT            # S, Q and every partial sum of acc: exact in any order
    mean = h.mean(axis=1)
    assert c.m == 1 or (np.diff(mean) != 0).all(), "adjacent rows share a mean"
    assert h.var(axis=1).min() >= 1.0
    # the packed operands are these numbers: W * gamma in fp16, s and t in fp32, without a rounding
    pk = _ln_pack(c)
    wp, s, t = pk.weight[:, :pk.k].double().numpy(), pk.ln_s.double().numpy(), pk.ln_t.double().numpy()
    if c.kind == "geglu":   # (tile-packed: 64 hidden rows and their 64 gate rows per 128)
        f = c.n // 2
        order = np.stack([np.arange(f).reshape(-1, 64), f + np.arange(f).reshape(-1, 64)], axis=1).reshape(-1)
    else:
        order = np.arange(c.n)
    assert np.array_equal(wp, (w * gamma)[order]) and np.array_equal(s, p.s[order]) and np.array_equal(t, p.t[order])
    assert np.abs(p.v).max() <= A.X_MAX
    if c.kind != "qkv":
        g = p.v[:, c.n // 2:] if c.kind == "geglu" else p.v
        assert c.m == 1 or ((g <= -3).mean() >= 0.04 and (np.abs(g) <= 0.5).mean() >= 0.10)


@pytest.mark.parametrize("case", A.LN_CASES, ids=lambda c: c.name)
def test_layernorm_model_sits_within_half_the_slack_and_a_neighbours_statistics_do_not(case):
    c = case
    for cols in (A.SOFTMAX_COLS if c.kind == "softmax" else (0,)):
        ref = A.ln_reference(c, cols)
        err = np.abs(A.ln_model32(c, cols).astype(np.float64) - ref.out)
        assert (err <= 0.5 * ref.slack).all(), (c.name, cols, float((err / np.maximum(ref.slack, 1e-300)).max()))
        if c.m > 1 and cols != 1:
            wrong = A.ln_reference(c, cols, A.ln_next_row(c)).out.astype(np.float16)
            share = float(A.violations(wrong, ref).mean())
            assert share >= A.MUTATION_SHARE, f"{c.name} cols {cols}: the neighbouring row's statistics are outside the bound on {share:.1%} only"


def test_the_sixteen_roundings_term_alone_does_not_hold_one_pass_variance_at_centre_48():
    """why the centre-48 rows carry a variance term: the fp32 model of the kernel's own arithmetic is tens of times outside 2^-20 T there,
    and within half of it on the ordinary rows"""
    for c in A.LN_CASES[:4]:
        p = A.ln_fold(c)
        t20 = 2.0 ** -20 * (np.abs(p.rstd * p.acc) + np.abs(p.rstd * p.mean * p.s) + np.abs(p.t))
        worst = float((np.abs(A.ln_fold32(c) - p.v) / t20).max())
        assert (worst > 10) if c.centre else (worst <= 0.5), (c.name, worst)


# ---------------------------------------------------------------------------------------------------------------- fused tails
@pytest.mark.parametrize("m", A.TAIL_A_M)
def test_tail_a_lattice_is_exact_and_its_model_inside(m):
    att, h, wo, bo, gamma, beta, wq = A.tail_a_data(m)
    h1, p = A.tail_a_reference(m)
    assert (np.abs(att) @ np.abs(wo).T + np.abs(bo) + np.abs(h)).max() < 2048 and (h1 == np.rint(h1)).all()   # every partial sum exact, fp16 holds h1
    assert all((t != 0).all() for t in (att, h, wo, bo, wq, beta))
    assert (h1 * h1).sum(axis=1).max() < EXACT and np.abs(h1).sum(axis=1).max() < EXACT and p.big.max() < EXACT
    assert _is_fp16(wq * gamma) and np.abs(p.v).max() <= A.X_MAX
    err = np.abs(A.fold_rows32(h1, p).astype(np.float64) - p.v)
    assert (err <= 0.5 * p.slack).all(), float((err / p.slack).max())
    ref = A.Ref(p.v, p.slack)
    wrong = A.tail_a_reference(m, (np.arange(m) + 1) % m)[1].v.astype(np.float16)
    assert A.violations(wrong, ref).mean() >= A.MUTATION_SHARE


@pytest.mark.parametrize("m", A.TAIL_B_M)
def test_tail_b_probe_shows_the_inner_geglu(m):
    att2, h1, perm, sign, bo, h2, gamma, beta, wf1, bf1 = A.tail_b_data(m)
    assert np.array_equal(sign * att2[:, perm] + bo + h1, h2) and np.abs(h1).max() <= 16 and (h1 == np.rint(h1)).all()
    assert np.abs(h2).max() <= 7 and h2.var(axis=1).min() >= 1.0 and (np.diff(h2.mean(axis=1)) != 0).all()
    assert sorted(np.concatenate([A.tail_b_select(i) for i in range(4)])) == list(range(4 * A.TAIL_C))
    for launch in ((0, 1, 2, 3) if m < 1000 else (m % 4,)):   # (the long cases: one selection here, all four on the GPU)
        r = A.tail_b_reference(m, launch)
        assert max(r.ph.big.max(), r.pg.big.max()) < EXACT and max(np.abs(r.ph.v).max(), np.abs(r.pg.v).max()) <= A.X_MAX
        assert ((r.pg.v <= -3).mean() >= 0.04) and ((np.abs(r.pg.v) <= 0.5).mean() >= 0.10)
        assert np.abs(r.out).max() < 65504
        got = A.tail_b_model32(m, launch)
        half = 64.0 * (A.half_step(r.hc.out) + 0.5 * r.hc.slack) + A.half_step(r.out)
        assert (np.abs(got.astype(np.float64) - r.out) <= half).all()
        for wrong in (A.tail_b_reference(m, launch, fn=A.gelu_tanh64), A.tail_b_reference(m, launch, stats_from=(np.arange(m) + 1) % m)):
            with np.errstate(over="ignore"):
                share = float((~(np.abs(wrong.out.astype(np.float16).astype(np.float64) - r.out) <= r.bound)).mean())
            assert share >= A.MUTATION_SHARE, share

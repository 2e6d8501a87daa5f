"""The conditions under which tests/test_exact_gpu.py may ask for bits (no GPU): for every case of tests/exact_cases.py the partial
sums stay below 2^24, the results inside fp16, the statistic sums below 2^24, no operand is zero, torch's CPU fp32 conv2d gives the
same integers as the float64 gather, and some cases reach beyond 2048.  And the numpy statements of the small kernels' arithmetic
against tests/fake_ops.py where that emulator states the same op."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as X

EXACT = float(2 ** 24)


@pytest.mark.parametrize("case", X.ALL_CASES, ids=lambda c: c.name)
def test_every_intermediate_value_of_the_case_is_exact(case):
    d, r = X.data(case), X.reference(case)
    assert r.bound.max() < EXACT, "a partial sum could leave fp32's integers"
    assert np.abs(r.exact).max() < 65504 and np.isfinite(r.out.astype(np.float64)).all()
    assert (r.exact * 2 == np.rint(r.exact * 2)).all()  # integers, or half-integers behind out_scale 0.5
    assert np.log2(case.out_scale) == int(np.log2(case.out_scale))
    for x, ch in zip(d.src, (case.c0, case.c1) if case.c1 else (case.c0,)):
        assert (x[..., :ch] != 0).all() and (x[..., ch:] == 0).all() and np.abs(x).max() <= 3
    assert (d.weight != 0).all() and np.abs(d.weight).max() <= 2
    for t in (d.bias, d.rowvec, d.residual, d.residual2, d.add2):   # fp16 holds every integer up to 2048
        assert t is None or np.abs(t).max() <= 2048
    if case.rowstat:
        assert case.cout % 64 == 0 and r.rowstat[..., 1].max() < EXACT and np.abs(r.rowstat[..., 0]).max() < EXACT
        assert np.abs(r.out.astype(np.float64)).reshape(case.m, -1, 64).sum(-1).max() < EXACT  # (any order of the 64 terms)
    if case.chanstat:
        assert r.chanstat[:, 1].max() < EXACT and np.abs(r.out.astype(np.float64)).sum(0).max() < EXACT
    assert float(X.SENTINEL) == float(np.float16(X.SENTINEL)) and not (r.out == np.float16(X.SENTINEL)).any()


@pytest.mark.parametrize("case", [c for c in X.ALL_CASES if c.cout * c.k < 4_000_000], ids=lambda c: c.name)
def test_torch_cpu_conv2d_gives_the_same_integers(case):
    """a second, independent statement of the geometry: torch.cat, F.interpolate(nearest), F.conv2d in fp32 (exact on these integers)"""
    d = X.data(case)
    x = torch.cat([torch.from_numpy(s[..., :ch].astype(np.float32)) for s, ch in zip(d.src, (case.c0, case.c1))], dim=-1).permute(0, 3, 1, 2)
    if case.up is not None:
        x = F.interpolate(x, size=case.up, mode="nearest")
    y = F.conv2d(x, torch.from_numpy(d.weight.astype(np.float32)), stride=case.stride, padding=case.ksize // 2)
    y = y.permute(0, 2, 3, 1).reshape(case.m, case.cout).double().numpy()
    a = X.gather(case, d.src).astype(np.float64) @ X.weight_matrix(case, d.weight).astype(np.float64).T
    assert y.shape == a.shape and np.array_equal(y, a)


def test_the_weight_matrix_is_the_packed_layout():
    """exact_cases.weight_matrix states the [N][(ky, kx, c)] layout on its own; the GPU test uploads packing.pack_conv's"""
    from videosd_amd.packing import pack_conv

    for name in ("base-four-wave", "generic-3-64", "concat-64+128-1x1"):
        case = X.BY_NAME[name]
        p = pack_conv(torch.from_numpy(X.data(case).weight.astype(np.float32)), None, cin_pad=case.cin_pad)
        assert (p.n, p.k, p.cin) == (case.cout, case.k, case.cin if not case.c1 else case.c0 + case.c1)
        assert np.array_equal(p.weight[:, :p.k].float().numpy(), X.weight_matrix(case, X.data(case).weight))
        assert not p.weight[:, p.k:].any()


def test_some_cases_reach_beyond_2048_and_meet_ties():
    beyond, ties = 0, 0
    for case in X.CASES:
        v = X.reference(case).exact
        beyond += bool((np.abs(v) > 2048).any())
        ties += bool(((np.abs(v) > 2048) & (np.abs(v) < 4096) & (v % 2 == 1)).any())   # an odd integer there lies between two fp16 values
    assert beyond >= 2 and ties >= 2, (beyond, ties)


def test_the_table_covers_the_forms_it_promises():
    forms = {c.name: set(c.forms) for c in X.CASES}
    assert {(t, p, s) for t, p, s, _ in forms["base-four-wave"]} == {(t, p, s) for t in range(4) for p in (0, 3, 4, 5, 6) for s in (1, 3)}
    assert all((t, p, 3, i) in forms["base-four-wave"] for t in range(4) for p in (0, 3, 4, 5, 6) for i in (True, False))
    assert {(t, p) for t, p, _, _ in forms["base-eight-wave"]} == {(t, p) for t in (0, 4, 6) for p in (8, 9)}
    assert all(s == 1 for t, _, s, _ in forms["base-eight-wave"] if t == 6)
    assert {(t, s) for t, p, s, _ in forms["base-halo"]} == {(t, s) for t in (0, 1, 4, 5) for s in (1, 2)}
    for name in ("epi-residual2", "epi-scale-0.5", "epi-scale-2", "epi-scale-dev-0.5", "epi-relu", "epi-relu-post", "epi-out2", "epi-out_t",
                 "epi-rowstat", "epi-chanstat"):
        assert {(t, s) for t, _, s, _ in forms[name]} == {(2, 1), (0, 1), (2, 3), (0, 3)}, name


# ---------------------------------------------------------------------------------------------------------------- small kernels
def _Fake():
    from fake_ops import FakeOps

    return FakeOps()


def test_postprocess_chain_is_the_emulators_on_every_finite_pattern_and_clamps_the_rest():
    x = X.postprocess_patterns()
    got = X.postprocess_chain(x)
    fin = np.isfinite(x.astype(np.float32)).all(axis=1)
    u8 = torch.zeros(int(fin.sum()) * 3, dtype=torch.uint8)
    _Fake().postprocess_rgb(torch.from_numpy(x[fin]), 3, int(fin.sum()), u8)
    assert np.array_equal(u8.numpy().reshape(-1, 3), got[fin])
    x32 = x.astype(np.float32)
    assert (got[np.isnan(x32)] == 0).all() and (got[x32 == np.inf] == 255).all() and (got[x32 == -np.inf] == 0).all()
    assert got[x32 >= 1].min() == 255 and got[x32 <= 0].max() == 0 and len(np.unique(got)) == 256


def test_preprocess_chain_is_the_emulators_and_torchs():
    u = np.stack([(np.arange(256) + 85 * c) % 256 for c in range(3)], axis=1).astype(np.uint8)
    got = X.preprocess_chain(u)
    out = torch.zeros(256, 8, dtype=torch.float16)
    _Fake().preprocess_rgb(torch.from_numpy(u), 16, 16, out)
    assert np.array_equal(out[:, :3].numpy(), got) and not out[:, 3:].any()
    assert np.abs(got.astype(np.float64) - u / 255.0).max() <= 2.0 ** -11   # three fp16 roundings below 1


def test_embed_and_axpy_statements_are_the_emulators():
    rng = np.random.default_rng(3)
    tok, pos = rng.standard_normal((50, 16)).astype(np.float16), rng.standard_normal((9, 16)).astype(np.float16)
    ids = np.array([0, 49, 50, -1, 2 ** 40, 7, 7, 31, 2], dtype=np.int64)
    ref = X.embed_reference(ids, tok, pos)
    for row, t in ((2, 49), (3, 0), (4, 49)):   # vocab, -1 and 2^40 clamp to the table's ends
        assert np.array_equal(ref[row], (tok[t].astype(np.float32) + pos[row].astype(np.float32)).astype(np.float16))
    out = torch.zeros(9, 16, dtype=torch.float16)
    _Fake().embed_tokens(torch.from_numpy(np.clip(ids, 0, 49)), torch.from_numpy(tok), torch.from_numpy(pos), out)
    assert np.array_equal(out.numpy(), ref)
    a, b = X.axpy_operands(4096)
    for s in X.AXPY_EXACT_SCALES:
        prod = np.float32(s) * b.astype(np.float32)
        assert np.array_equal(prod.astype(np.float64), np.float64(s) * b.astype(np.float64))   # the product is exact
        o = torch.zeros(4096, dtype=torch.float16)
        _Fake().axpy(torch.from_numpy(a), torch.from_numpy(b), s, 4096, o)
        assert np.array_equal(o.numpy(), X.axpy_exact(a, b, s))
    assert X.ulp_distance(X.axpy_exact(a, b, 0.3), X.axpy_real(a, b, 0.3)).max() <= 1
    assert X.AXPY_N_LONG // 8 > 2048 * 256 and X.AXPY_N_LONG % 8 == 0
    assert list(X.ulp_distance(np.array([0.0, 1.0, -6e-8], np.float16), np.array([-0.0, 1.001, 6e-8], np.float16))) == [0, 1, 2]


@pytest.mark.parametrize("rows,c", X.ADAIN_SHAPES)
def test_adain_in_float32_stays_inside_both_conditions(rows, c):
    """the kernel's arithmetic restated in numpy float32 against the float64 reference: no element further than one fp16 step, at
    most 1 % different at all; the emulator's fp32 statement too; the statistics are benign as promised"""
    x, st, st_ref = X.adain_operands(rows, c)
    ref = X.adain_reference(x, st, st_ref, rows)
    for s in (st, st_ref):
        mean = s[:, 0].astype(np.float64) / rows
        var = s[:, 1].astype(np.float64) / rows - mean * mean
        live = np.arange(c) != X.ADAIN_CONST_CHANNEL
        assert (np.abs(mean[live]) <= np.sqrt(var[live])).all() and abs(var[X.ADAIN_CONST_CHANNEL]) < X.ADAIN_EPS
    assert np.isfinite(ref.astype(np.float32)).all()
    far, share = X.adain_conditions(X.adain_float32(x, st, st_ref, rows), ref)
    assert far <= 1 and share <= 0.01, (far, share)
    if rows * c < 100_000:
        out = torch.zeros(rows, c, dtype=torch.float16)
        _Fake().adain(torch.from_numpy(x), torch.from_numpy(st), torch.from_numpy(st_ref), rows, c, out, eps=X.ADAIN_EPS)
        far, share = X.adain_conditions(out.numpy(), ref)
        assert far <= 1 and share <= 0.01, (far, share)
    assert (rows * (c // 8) + 255) // 256 > 4096 or rows < 4096

"""Exact arithmetic on the MI355X: the conv / GEMM kernel forms and the small elementwise kernels against answers known to the bit.

tests/exact_cases.py builds integer operands for which every product and every partial sum is exact in fp32 in any order, so the only
rounding of a launch is fp32 -> fp16 at the store; the expected tensor is fp16(float64 arithmetic) and the comparison is
torch.equal.  No operand is zero: one product dropped, duplicated or fetched from the neighbouring pixel or channel changes the output,
as does a second rounding in an epilogue (the `big` cases reach beyond 2048, where every odd value is a tie).  tests/test_exact_host.py
checks, without a GPU, that the cases are what they claim to be.  SiLU, the GELUs, GEGLU, the tile softmax and the fused LayerNorm
are not exact: tests/test_act_forms_gpu.py holds them to a bound per element on the same lattice made dyadic (and the tolerance tests of
tests/test_ops_gpu.py stay)."""
import numpy as np
import pytest
import torch

import exact_cases as X
from conv_problem import ExactProblem as Problem, run_form, sentinel   # (shared with tests/test_act_forms_gpu.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_conv_gemm_is_exact_in_every_form(ops, case):
    prob = Problem(ops, case)
    for form in case.forms:
        d = run_form(ops, prob, form)
    if case.name == "k23040-concat":
        assert d.split_k > 1, "the deep-K case is meant to run split over K"
    # the tickets of the in-launch reductions (split-K tiles, channel statistics) are back at zero
    assert not any(bool(c.any()) for c in ops._counters + ops._chan_counters)


def test_a_group_of_three_is_exact(ops):
    """one vsd_conv_gemm_group of members of different M (252, 99, 35), in four forms"""
    probs = [Problem(ops, c) for c in X.GROUP_MEMBERS]
    for form in X.GROUP_FORMS:
        outs = [p.outputs() for p in probs]
        ops.conv_group([p.call(o, kw) for p, (o, kw) in zip(probs, outs)], form=form)
        ops.synchronize()
        for p, (o, kw) in zip(probs, outs):
            p.check(o, f"in a group, form {form}")
    assert not any(bool(c.any()) for c in ops._counters)


def test_a_pair_of_twin_convs_is_exact(ops):
    """ops.pair (the engine's entry point for the twin layers of UNet and ControlNet): two weight sets, one grid"""
    probs = [Problem(ops, c) for c in X.PAIR_MEMBERS]
    outs = [p.outputs() for p in probs]
    (aa, ka), (ab, kb) = [p.call(o, kw) for p, (o, kw) in zip(probs, outs)]
    assert ops.pair_split(aa, ka, ab, kb) is not None   # (they do share a grid)
    ops.pair((ops.conv, aa, ka), (ops.conv, ab, kb))
    ops.synchronize()
    for p, (o, kw) in zip(probs, outs):
        p.check(o, "in a pair")
    assert not torch.equal(outs[0][0]["out"], outs[1][0]["out"])


# ---------------------------------------------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("ld", [8, 3])
def test_postprocess_rgb_on_every_fp16_bit_pattern(ops, ld):
    x = X.postprocess_patterns()                      # [65536][3]: every pattern in every channel position
    img = np.zeros((65536, ld), dtype=np.float16)
    img[:, :3] = x
    u8 = torch.full((65536 * 3 + 16,), 77, dtype=torch.uint8, device="cuda")
    ops.postprocess_rgb(torch.from_numpy(img).cuda(), ld, 65536, u8)
    ops.synchronize()
    got = u8.cpu().numpy()
    exp = X.postprocess_chain(x)
    assert (got[65536 * 3:] == 77).all()
    got = got[:65536 * 3].reshape(65536, 3)
    bad = np.argwhere(got != exp)
    assert not len(bad), f"{len(bad)} bytes differ, first: pattern {x.view(np.uint16)[tuple(bad[0])]:#06x} -> {got[tuple(bad[0])]} (chain: {exp[tuple(bad[0])]})"
    x32 = x.astype(np.float32)
    assert (got[np.isnan(x32)] == 0).all() and (got[x32 == np.inf] == 255).all() and (got[x32 == -np.inf] == 0).all()


def test_preprocess_rgb_on_every_byte_value(ops):
    h, w = 21, 37   # 777 pixels: three full workgroups and a ragged one
    hw = h * w
    u = np.stack([(np.arange(hw) + 85 * c) % 256 for c in range(3)], axis=1).astype(np.uint8)
    assert all(len(np.unique(u[:, c])) == 256 for c in range(3))
    out = sentinel(hw + 2, 8)
    ops.preprocess_rgb(torch.from_numpy(u).cuda(), h, w, out)
    ops.synchronize()
    got = out.cpu().numpy()
    exp = X.preprocess_chain(u)
    # (u / 255 is an IEEE fp32 division on the device: should a byte value differ, torch's CPU result of the same chain decides)
    x = torch.from_numpy(u).float() / 255.0
    t = (((2.0 * x - 1.0).half().float() + 1.0).half().float() * 0.5).half().numpy()
    assert np.array_equal(t, exp)
    bad = np.argwhere(got[:hw, :3] != exp)
    assert not len(bad), f"{len(bad)} values differ, first: byte {u[tuple(bad[0])]} -> {got[:hw, :3][tuple(bad[0])]!r} (chain: {exp[tuple(bad[0])]!r})"
    assert not got[:hw, 3:].any() and (got[hw:] == np.float16(X.SENTINEL)).all()


@pytest.mark.parametrize("n,c", [(77, 768), (5, 8)])
def test_embed_tokens_clamps_and_adds_once(ops, n, c):
    vocab = 1000
    rng = np.random.default_rng(n)
    tok, pos = rng.standard_normal((vocab, c)).astype(np.float16), rng.standard_normal((n + 3, c)).astype(np.float16)
    ids = rng.integers(0, vocab, n).astype(np.int64)
    ids[:5] = [0, vocab - 1, vocab, -1, 2 ** 40]
    out = sentinel(n + 2, c)
    ops.embed_tokens(torch.from_numpy(ids).cuda(), torch.from_numpy(tok).cuda(), torch.from_numpy(pos).cuda(), out[:n])
    ops.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], X.embed_reference(ids, tok, pos)) and (got[n:] == np.float16(X.SENTINEL)).all()


@pytest.mark.parametrize("n", [X.AXPY_N_LONG, 8])
def test_axpy_exact_scales_general_scale_and_in_place(ops, n):
    a, b = X.axpy_operands(n)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for scale in X.AXPY_EXACT_SCALES:
        out = sentinel(n + 8)
        ops.axpy(da, db, scale, n, out)
        ops.synchronize()
        assert torch.equal(out[:n], torch.from_numpy(X.axpy_exact(a, b, scale)).cuda()), f"scale {scale}"
        assert bool((out[n:] == X.SENTINEL).all())
    out = sentinel(n)
    ops.axpy(da, db, 0.3, n, out)
    inplace = da.clone()
    ops.axpy(inplace, db, 0.3, n, inplace)
    ops.synchronize()
    far = X.ulp_distance(out.cpu().numpy(), X.axpy_real(a, b, 0.3))
    assert far.max() <= 1, f"scale 0.3: {int((far > 1).sum())} elements further than one fp16 step, the farthest {int(far.max())}"
    assert torch.equal(inplace, out), "in place differs from out of place"


@pytest.mark.parametrize("rows,c", X.ADAIN_SHAPES)
def test_adain_within_one_step_of_float64(ops, rows, c):
    x, st, st_ref = X.adain_operands(rows, c)
    dx = torch.from_numpy(x).cuda()
    out = sentinel(rows + 1, c)
    ops.adain(dx, torch.from_numpy(st).cuda(), torch.from_numpy(st_ref).cuda(), rows, c, out[:rows], eps=X.ADAIN_EPS)
    inplace = dx.clone()
    ops.adain(inplace, torch.from_numpy(st).cuda(), torch.from_numpy(st_ref).cuda(), rows, c, inplace, eps=X.ADAIN_EPS)   # (x and out may alias)
    ops.synchronize()
    got = out.cpu().numpy()
    far, share = X.adain_conditions(got[:rows], X.adain_reference(x, st, st_ref, rows))
    print(f"adain {rows} x {c}: farthest {far} fp16 steps, {share:.3%} of the elements differ")
    assert far <= 1 and share <= 0.01, (far, share)
    assert (got[rows:] == np.float16(X.SENTINEL)).all() and torch.equal(inplace, out[:rows])

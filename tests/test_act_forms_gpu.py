"""The non-linear epilogues of the conv / GEMM library on the MI355X, every kernel form, per element against float64
(tests/act_cases.py: the cases, the exactly known pre-activations, the references, the bound per element; tests/test_act_cases_host.py:
the proof that a wrong activation, a wrong order of scale / residual / activation, swapped GEGLU halves or a softmax over other
columns is outside that bound).  Every launch is framed by sentinels (rows past M, padding columns, out_t's padding) and leaves the
split-K and channel tickets at zero.  Each test prints, per case and form, the worst |got - float64| / bound, the farthest element in
fp16 steps from fp16(float64) and the share of elements that differ from it at all (profiles/act_forms.txt)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import act_cases as A
from conv_problem import TAIL_ROWS, Problem, dev16, run_form, sentinel

pytestmark = pytest.mark.gpu
SENT = np.float16(A.SENTINEL)


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    o = HipOps(0)
    yield o
    o.synchronize()   # (hand torch's allocator cache back, as tests/test_norm_forms_gpu.py does and says why)
    del o
    gc.collect()
    torch.cuda.empty_cache()


def tickets_at_zero(ops):
    return not any(bool(c.any()) for c in ops._counters + ops._chan_counters)


def judge(name, what, got, ref):
    """every element inside its bound"""
    worst, used, steps, share = A.report(got, ref)
    print(f"ACTFORM {name} [{what}] worst_err_over_bound={worst:.3f} slack_used={used:.3f} max_fp16_steps={steps} differing={share:.5f}")
    bad = A.violations(got, ref)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name} {what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {i}: got {float(got[i])!r}, "
                             f"float64 {ref.out[i]!r}, bound {ref.bound[i]:.3g}; worst {worst:.3g} bounds")


class ActProblem(Problem):
    """a case of act_cases.CONV_CASES: every output element within its bound of float64, the sentinel frame untouched"""

    def __init__(self, ops, case):
        super().__init__(ops, case, A.conv_data(case))
        self.data = A.conv_data(case)
        self.x, self.ref = A.conv_reference(case)

    def check(self, o, what):
        c, n = self.case, self.case.cout
        t0 = n if c.t_col0 is None else c.t_col0
        out = o["out"].cpu().numpy()
        frame = out[:c.m, n:] if not c.thin else out[:0]
        assert (out[c.m:] == SENT).all() and (frame == SENT).all() and (out[:c.m, t0:n] == SENT).all(), f"{c.name} {what}: the frame of out was written"
        if c.thin:
            assert not out[:c.m, n:].any()   # (the persistent form's thin output writes whole 8-wide rows: padding channels zero)
        got = out[:c.m, :n].copy()
        if c.t_col0 is not None:
            t = o["out_t"].cpu().numpy()
            ho, wo = c.ho_wo
            hw, t_img = ho * wo, c.t_img or ho * wo
            written = np.zeros(t.shape, dtype=bool)
            for b in range(c.batch):
                got[b * hw:(b + 1) * hw, t0:] = t[:n - t0, b * t_img:b * t_img + hw].T
                written[:n - t0, b * t_img:b * t_img + hw] = True
            assert (t[~written] == SENT).all(), f"{c.name} {what}: the frame of out_t was written"
        judge(c.name, what, got, self.ref)
        if c.out2:   # out2 = fp16(out + add2) of the STORED out: to the bit
            out2 = o["out2"].cpu().numpy()
            exp2 = np.full(out2.shape, SENT)
            exp2[:c.m, :t0] = (got[:, :t0].astype(np.float64) + self.data.add2[:, :t0]).astype(np.float16)
            assert np.array_equal(out2.view(np.uint16), exp2.view(np.uint16)), f"{c.name} {what}: out2 is not fp16(out + add2)"


@pytest.mark.parametrize("case", A.CONV_CASES, ids=lambda c: c.name)
def test_activation_in_every_form(ops, case):
    prob = ActProblem(ops, case)
    for form in case.forms:
        run_form(ops, prob, form)
    assert tickets_at_zero(ops)


@pytest.mark.parametrize("case", A.REFUSED, ids=lambda c: c.name)
def test_combinations_without_a_kernel_are_refused(ops, case):
    """erf-GELU exists in the general walk only; an activation after the residual does not exist with a transposed output (both
    transposed paths would store no activation at all) -- VSD_ERR_ARG, not a wrong tensor"""
    prob = Problem(ops, case, A.conv_data(case))
    o, kw = prob.outputs()
    args, kwargs = prob.call(o, kw)
    for tile, split in ((A.T64x64, 1), (A.T128x128, 3)):
        with pytest.raises(RuntimeError, match="conv_gemm: "):
            ops.conv(*args, tile=tile, split_k=split, pipeline=3, **kwargs)
    ops.synchronize()
    assert all(bool((t == A.SENTINEL).all()) for t in o.values() if t.dtype == torch.float16), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------------------------- GEGLU, softmax
def _linear(ops, c, act, forms, out_cols, pack, **kw):
    from videosd_amd.ops import Geom

    a, w, b = A.lin_data(c)
    pw = ops.to_device_pack(pack(torch.from_numpy(w).float(), torch.from_numpy(b).float()))
    x = dev16(a)
    ldo = out_cols + 8
    for form in forms:
        tile, pipeline, split, inkernel = form
        out = sentinel(c.m + TAIL_ROWS, ldo)
        d = ops.conv(x, None, Geom.linear(c.m), pw, out, ldo=ldo, act=act, tile=tile, split_k=split, pipeline=pipeline, inkernel=inkernel,
                     _desc_only=True, **kw)
        assert (d.tile, d.pipeline, d.split_k, bool(d.counters), d.act) == (tile, pipeline, split, split > 1, act), form
        ops.ctx.call("vsd_conv_gemm", C.byref(d), ops.s)
        ops.synchronize()
        got = out.cpu().numpy()
        what = f"tile {tile} pipeline {pipeline} split {split}"
        assert (got[c.m:] == SENT).all() and (got[:c.m, out_cols:] == SENT).all(), f"{c.name} {what}: the frame of out was written"
        yield what, got[:c.m, :out_cols]
    assert tickets_at_zero(ops)


@pytest.mark.parametrize("case", A.GEGLU_CASES, ids=lambda c: c.name)
def test_geglu_in_every_form(ops, case):
    from videosd_amd.packing import pack_geglu

    ref = A.geglu_reference(case)
    for what, got in _linear(ops, case, A.ACT_GEGLU, case.forms, case.n // 2, pack_geglu):
        judge(case.name, what, got, ref)


@pytest.mark.parametrize("cols", A.SOFTMAX_COLS)
@pytest.mark.parametrize("case", A.SOFTMAX_CASES, ids=lambda c: c.name)
def test_tile_softmax_in_every_form(ops, case, cols):
    from videosd_amd.packing import pack_linear

    ref = A.softmax_reference(case, cols)
    for what, got in _linear(ops, case, A.ACT_SOFTMAX, case.forms, case.n, pack_linear, softmax_cols=cols):
        judge(f"{case.name}-cols{cols}", what, got, ref)
        dead = got.reshape(case.m, -1, 128)[:, :, cols:]
        assert not dead.view(np.uint16).any(), f"{case.name} cols {cols} {what}: a column past softmax_cols is not +0"


# ---------------------------------------------------------------------------------------------------------------- folded LayerNorm
def _ln_operands(ops, c):
    """the rows through an identity producer GEMM that leaves their (sum, sum of squares) partials, as the networks' producers do"""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_geglu_ln, pack_linear, pack_linear_ln

    h, gamma, beta, w, bias = A.ln_data(c)
    tw, tg, tb = torch.from_numpy(w).float(), torch.from_numpy(gamma).half(), torch.from_numpy(beta).half()
    tbias = None if bias is None else torch.from_numpy(bias).float()
    pw = ops.to_device_pack(pack_geglu_ln(tw, tbias, tg, tb) if c.kind == "geglu" else pack_linear_ln([tw], None if bias is None else [tbias], tg, tb))
    eye = ops.to_device_pack(pack_linear(torch.eye(c.c).half(), None))
    rows = sentinel(c.m, c.c)
    rs = torch.full((c.m, c.c // 64, 2), -1.0, dtype=torch.float32, device="cuda")
    ops.conv(dev16(h), None, Geom.linear(c.m), eye, rows, rowstat_out=rs, tile=A.T64x64)
    ops.synchronize()
    assert np.array_equal(rows.cpu().numpy().astype(np.float64), h)
    st = rs.cpu().numpy().astype(np.float64).sum(axis=1)
    assert np.array_equal(st[:, 0], h.sum(axis=1)) and np.array_equal(st[:, 1], (h * h).sum(axis=1))   # (exact: integers below 2^24)
    return rows, rs, pw


def _ln_launches(ops, c, rows, rs, pw, out_cols, **kw):
    from videosd_amd.ops import Geom

    ldo = out_cols + 8
    for tile, pipeline, split, inkernel in c.forms:
        out = sentinel(c.m + TAIL_ROWS, ldo)
        extra = {k: (v() if callable(v) else v) for k, v in kw.items()}
        d = ops.conv(rows, None, Geom.linear(c.m), pw, out, ldo=ldo, ln_part=rs, ln_eps=A.LN_EPS, tile=tile, split_k=split, pipeline=pipeline,
                     inkernel=inkernel, _desc_only=True, **extra)
        assert (d.tile, d.pipeline, d.split_k, bool(d.counters)) == (tile, pipeline, split, inkernel and split > 1), (tile, pipeline, split, inkernel)
        ops.ctx.call("vsd_conv_gemm", C.byref(d), ops.s)
        ops.synchronize()
        got = out.cpu().numpy()
        what = f"tile {tile} pipeline {pipeline} split {split} {'in-launch' if d.counters else 'reducer' if split > 1 else 'unsplit'}"
        assert (got[c.m:] == SENT).all() and (got[:c.m, out_cols:] == SENT).all(), f"{c.name} {what}: the frame of out was written"
        yield what, got[:c.m, :out_cols], extra
    assert tickets_at_zero(ops)


LN_BY_KIND = {k: [c for c in A.LN_CASES if c.kind == k] for k in ("qkv", "geglu", "softmax")}


@pytest.mark.parametrize("case", LN_BY_KIND["qkv"], ids=lambda c: c.name)
def test_layernorm_consumers_without_activation(ops, case):
    """Q and K plain, V transposed; the centre-48 draws are judged like the others (their bound carries the variance term)"""
    c = case
    rows, rs, pw = _ln_operands(ops, c)
    ref = A.ln_reference(c)
    ldt = (c.m + 7) // 8 * 8
    for what, qk, extra in _ln_launches(ops, c, rows, rs, pw, 2 * c.c, out_t=lambda: sentinel(c.c + 2, ldt), ldt=ldt, t_col0=2 * c.c):
        vt = extra["out_t"].cpu().numpy()
        assert (vt[c.c:] == SENT).all() and (vt[:, c.m:] == SENT).all(), f"{c.name} {what}: the frame of out_t was written"
        judge(c.name, what, np.concatenate([qk, vt[:c.c, :c.m].T], axis=1), ref)


@pytest.mark.parametrize("case", LN_BY_KIND["geglu"], ids=lambda c: c.name)
def test_geglu_behind_the_folded_layernorm(ops, case):
    rows, rs, pw = _ln_operands(ops, case)
    ref = A.ln_reference(case)
    for what, got, _ in _ln_launches(ops, case, rows, rs, pw, case.n // 2):
        judge(case.name, what, got, ref)


@pytest.mark.parametrize("cols", A.SOFTMAX_COLS)
@pytest.mark.parametrize("case", LN_BY_KIND["softmax"], ids=lambda c: c.name)
def test_tile_softmax_behind_the_folded_layernorm(ops, case, cols):
    rows, rs, pw = _ln_operands(ops, case)
    ref = A.ln_reference(case, cols)
    for what, got, _ in _ln_launches(ops, case, rows, rs, pw, case.n, act=A.ACT_SOFTMAX, softmax_cols=cols):
        judge(f"{case.name}-cols{cols}", what, got, ref)
        assert not got.reshape(case.m, -1, 128)[:, :, cols:].view(np.uint16).any(), f"{case.name} cols {cols} {what}: a column past softmax_cols is not +0"


# ---------------------------------------------------------------------------------------------------------------- csrc/fused_tail.hip
def _frag(ops, p):
    from videosd_amd.packing import add_frag

    return ops.to_device_pack(add_frag(p))


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@pytest.mark.parametrize("m", A.TAIL_A_M)
def test_tail_a_h1_to_the_bit_and_q_within_the_folds_bound(ops, m):
    """16-row tiles (m = 200) and 32-row tiles (m = 4100), both ending ragged: the two heights the library gives tail_a"""
    from videosd_amd.packing import pack_linear, pack_linear_ln

    att, h, wo, bo, gamma, beta, wq = A.tail_a_data(m)
    h1_ref, p = A.tail_a_reference(m)
    out1 = _frag(ops, pack_linear(_t(wo), _t(bo)))
    q2 = _frag(ops, pack_linear_ln([_t(wq)], None, _t(gamma, torch.float16), _t(beta, torch.float16)))
    h1, q = sentinel(m + TAIL_ROWS, A.TAIL_C), sentinel(m + TAIL_ROWS, A.TAIL_C)
    ops.tail_a(dev16(att), dev16(h), m, out1, q2, h1, q, ln_eps=A.LN_EPS)
    ops.synchronize()
    assert torch.equal(h1[:m], dev16(h1_ref)), "tail_a h1 is not fp16(exact)"
    assert bool((h1[m:] == A.SENTINEL).all()) and bool((q[m:] == A.SENTINEL).all())
    judge(f"tail_a-m{m}", "q", q[:m].cpu().numpy(), A.Ref(p.v, p.slack))


@pytest.mark.parametrize("m", A.TAIL_B_M)
def test_tail_b_inner_geglu_through_probe_weights(ops, m):
    """out = fp16(64 fp16(Hc[selected columns]) + h2): four launches make all 1280 hidden columns of the inner GEGLU visible"""
    from videosd_amd.packing import pack_conv, pack_geglu_ln, pack_linear

    c = A.TAIL_C
    att2, h1, perm, sign, bo, h2, gamma, beta, wf1, bf1 = A.tail_b_data(m)
    wo = np.zeros((c, c))
    wo[np.arange(c), perm] = sign   # h2[:, j] = sign[j] att2[:, perm[j]] + b[j] + h1[:, j]
    zero = torch.zeros(c)
    out2 = _frag(ops, pack_linear(_t(wo), _t(bo)))
    ff1 = _frag(ops, pack_geglu_ln(_t(wf1), _t(bf1), _t(gamma, torch.float16), _t(beta, torch.float16)))
    proj = _frag(ops, pack_conv(torch.eye(c).reshape(c, c, 1, 1), zero))
    d_att2, d_h1, d_x = dev16(att2), dev16(h1), torch.zeros(m, c, dtype=torch.float16, device="cuda")
    for launch in range(4):
        w2 = np.zeros((c, 4 * c))
        w2[np.arange(c), A.tail_b_select(launch)] = 64.0
        ff2 = _frag(ops, pack_linear(_t(w2), zero))
        out = sentinel(m + TAIL_ROWS, c)
        ops.tail_b(d_att2, d_h1, d_x, m, out2, ff1, ff2, proj, out, ln_eps=A.LN_EPS)
        ops.synchronize()
        got = out.cpu().numpy()
        assert (got[m:] == SENT).all(), "tail_b wrote past row m"
        r = A.tail_b_reference(m, launch)
        err = np.abs(got[:m].astype(np.float64) - r.out)
        with np.errstate(over="ignore"):
            steps = A.ulp_distance(got[:m], r.out.astype(np.float16))
        print(f"ACTFORM tail_b-m{m} [hidden columns {launch} + 4 j] worst_err_over_bound={float((err / r.bound).max()):.3f} "
              f"max_fp16_steps={int(steps.max())} differing={float((steps != 0).mean()):.5f}")
        bad = ~(err <= r.bound)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"tail_b m={m} launch {launch}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {i}: got "
                                 f"{float(got[i])!r}, float64 {r.out[i]!r} (Hc {r.hc.out[i]!r}, h2 {h2[i]!r}), bound {r.bound[i]:.3g}")


def test_erf_gelu_behind_the_folded_layernorm_is_refused(ops):
    """the fourth combination erf-GELU has no kernel for (out_t, rowstat_out and VSD_ACT_POST: test_combinations_without_a_kernel_are_refused)"""
    from videosd_amd.ops import Geom

    c = LN_BY_KIND["softmax"][0]
    rows, rs, pw = _ln_operands(ops, c)
    out = sentinel(c.m, c.n)
    with pytest.raises(RuntimeError, match="conv_gemm: erf GELU"):
        ops.conv(rows, None, Geom.linear(c.m), pw, out, ln_part=rs, ln_eps=A.LN_EPS, act=A.ACT_GELU, tile=A.T64x64, split_k=1, pipeline=3)
    ops.synchronize()
    assert bool((out == A.SENTINEL).all())

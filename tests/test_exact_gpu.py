"""Exact arithmetic on the MI355X: the conv / GEMM kernel forms and the small elementwise kernels against answers known to the bit.

tests/exact_cases.py builds integer operands for which every product and every partial sum is exact in fp32 in any order, so the only
rounding of a launch is fp32 -> fp16 at the store; the expected tensor is fp16(float64 arithmetic) and the comparison is
torch.equal.  No operand is zero: one product dropped, duplicated or fetched from the neighbouring pixel or channel changes the output,
as does a second rounding in an epilogue (the `big` cases reach beyond 2048, where every odd value is a tie).  tests/test_exact_host.py
checks, without a GPU, that the cases are what they claim to be.  SiLU, the GELUs, GEGLU, the tile softmax and the fused LayerNorm
are not exact and stay with the tolerance tests of tests/test_ops_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float16)).cuda()


def sentinel(*shape):
    return torch.full(shape, X.SENTINEL, dtype=torch.float16, device="cuda")


class Problem:
    """the device side of one case: operands uploaded once, fresh sentinel-filled outputs per launch"""

    def __init__(self, ops, case):
        from videosd_amd.ops import Geom
        from videosd_amd.packing import pack_conv

        self.ops, self.case = ops, case
        d, r = X.data(case), X.reference(case)
        self.src = [dev16(s.reshape(-1, s.shape[-1])) for s in d.src]
        self.pw = ops.to_device_pack(pack_conv(torch.from_numpy(d.weight.astype(np.float32)), None if d.bias is None else torch.from_numpy(
            d.bias.astype(np.float32)), cin_pad=case.cin_pad))
        assert (self.pw.n, self.pw.k) == (case.cout, case.k)
        self.geom = Geom.conv(case.h, case.w, ksize=case.ksize, stride=case.stride, up_to=case.up, batch=case.batch)
        assert self.geom.m == case.m
        self.kw = dict(ldo=case.ldo, c0=case.cin - case.c1, c1=case.c1, act=case.act)
        if d.rowvec is not None:
            self.kw["rowvec"] = dev16(d.rowvec)
        if d.residual is not None:
            self.kw.update(residual=dev16(d.residual), ldr=case.ldr)
        if d.residual2 is not None:
            self.kw["residual2"] = dev16(d.residual2)
        if case.scale_dev:
            self.kw["out_scale_dev"] = torch.tensor([case.out_scale], dtype=torch.float32, device="cuda")
        else:
            self.kw["out_scale"] = case.out_scale
        if d.add2 is not None:
            self.kw["add2"] = dev16(d.add2)
        n = case.cout
        exp = np.full((case.m + 4, case.ldo), X.SENTINEL, dtype=np.float16)   # rows past M and the padding columns stay as they were
        t0 = n if case.t_col0 is None else case.t_col0
        exp[:case.m, :t0] = r.out[:, :t0]
        if case.thin:
            exp[:case.m, n:] = 0   # (the persistent form's thin output writes whole 8-wide rows: padding channels zero)
        self.exp = dev16(exp)
        self.exp2 = self.exp_t = self.exp_rs = self.exp_cs = None
        if case.out2:
            exp2 = exp.copy()
            exp2[:case.m, :n] = r.out2
            self.exp2 = dev16(exp2)
        if case.t_col0 is not None:
            t = X.transposed(case, r.out)
            self.exp_t = dev16(np.concatenate([t, np.full((2, t.shape[1]), X.SENTINEL, dtype=np.float16)]))
        if case.rowstat:
            self.exp_rs = torch.from_numpy(r.rowstat.astype(np.float32)).cuda()
        if case.chanstat:
            self.exp_cs = torch.from_numpy(r.chanstat.astype(np.float32)).cuda()

    def outputs(self):
        case = self.case
        o = dict(out=sentinel(case.m + 4, case.ldo))
        kw = {}
        if case.out2:
            o["out2"] = kw["out2"] = sentinel(case.m + 4, case.ldo)
        if case.t_col0 is not None:
            o["out_t"] = kw["out_t"] = sentinel(*self.exp_t.shape)
            kw.update(ldt=self.exp_t.shape[1], t_col0=case.t_col0, t_img=case.t_img)
        if case.rowstat:
            o["rowstat"] = kw["rowstat_out"] = torch.full((case.m, case.cout // 64, 2), -1.0, dtype=torch.float32, device="cuda")
        if case.chanstat:
            o["chanstat"] = kw["chanstat_out"] = torch.full((case.cout, 2), -1.0, dtype=torch.float32, device="cuda")
        return o, kw

    def call(self, o, kw):
        """(args, kwargs) of HipOps.conv for this problem"""
        return (self.src[0], self.src[1] if len(self.src) > 1 else None, self.geom, self.pw, o["out"]), {**self.kw, **kw}

    def check(self, o, what):
        def same(got, exp, name):
            if not torch.equal(got, exp):
                bad = (got != exp).nonzero()
                i = tuple(int(v) for v in bad[0])
                raise AssertionError(f"{self.case.name} {what}: {name} differs in {len(bad)} of {exp.numel()} places, first at {i}: "
                                     f"got {float(got[i])!r}, exact {float(exp[i])!r}")
        same(o["out"], self.exp, "out")
        for key, exp in (("out2", self.exp2), ("out_t", self.exp_t), ("rowstat", self.exp_rs), ("chanstat", self.exp_cs)):
            if exp is not None:
                same(o[key], exp, key)


def run_form(ops, prob, form):
    """one launch in exactly the kernel form asked for (HipOps.conv swaps the halo / persistent forms out for calls they cannot take:
    a swapped form would test something else, so the descriptor is checked before it goes to the library)"""
    tile, pipeline, split, inkernel = form
    o, kw = prob.outputs()
    args, kwargs = prob.call(o, kw)
    ops.inkernel_splitk = inkernel
    try:
        d = ops.conv(*args, tile=tile, split_k=split, pipeline=pipeline, _desc_only=True, **kwargs)
    finally:
        ops.inkernel_splitk = True
    if tile is not None:
        assert (d.tile, d.pipeline, d.split_k, bool(d.counters)) == (tile, pipeline, split, inkernel and split > 1), form
    ops.ctx.call("vsd_conv_gemm", C.byref(d), ops.s)
    ops.synchronize()
    prob.check(o, f"tile {d.tile} pipeline {d.pipeline} split {d.split_k} {'in-launch' if d.counters else 'reducer'}")
    return d


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

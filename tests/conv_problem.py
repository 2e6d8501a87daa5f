"""The device side of one conv / GEMM case of tests/exact_cases.py's `Case` table, shared by tests/test_exact_gpu.py (answers known
to the bit) and tests/test_act_forms_gpu.py (answers known to a bound per element): operands uploaded once, fresh sentinel-filled
outputs per launch, one launch in exactly the kernel form asked for.  What is expected and how it is compared is the subclass's."""
import ctypes as C

import numpy as np
import torch

import exact_cases as X


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float16)).cuda()


def sentinel(*shape):
    return torch.full(shape, X.SENTINEL, dtype=torch.float16, device="cuda")


TAIL_ROWS = 4   # sentinel rows behind every output (out_t: 2)


def transposed_shape(case):
    ho, wo = case.ho_wo
    return case.cout - case.t_col0 + 2, (case.batch * (case.t_img or ho * wo) + 7) // 8 * 8


class Problem:
    """operands of `case` from `d` (an exact_cases.Data: arrays of the values themselves, whatever their dtype)"""

    def __init__(self, ops, case, d):
        from videosd_amd.ops import Geom
        from videosd_amd.packing import pack_conv

        self.ops, self.case = ops, case
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

    def outputs(self):
        case = self.case
        o = dict(out=sentinel(case.m + TAIL_ROWS, case.ldo))
        kw = {}
        if case.out2:
            o["out2"] = kw["out2"] = sentinel(case.m + TAIL_ROWS, case.ldo)
        if case.t_col0 is not None:
            rows, ldt = transposed_shape(case)
            o["out_t"] = kw["out_t"] = sentinel(rows, ldt)
            kw.update(ldt=ldt, t_col0=case.t_col0, t_img=case.t_img)
        if case.rowstat:
            o["rowstat"] = kw["rowstat_out"] = torch.full((case.m, case.cout // 64, 2), -1.0, dtype=torch.float32, device="cuda")
        if case.chanstat:
            o["chanstat"] = kw["chanstat_out"] = torch.full((case.cout, 2), -1.0, dtype=torch.float32, device="cuda")
        return o, kw

    def call(self, o, kw):
        """(args, kwargs) of HipOps.conv for this problem"""
        return (self.src[0], self.src[1] if len(self.src) > 1 else None, self.geom, self.pw, o["out"]), {**self.kw, **kw}

    def check(self, o, what):
        raise NotImplementedError


class ExactProblem(Problem):
    """a case of exact_cases.CASES: every output torch.equal to fp16(exact arithmetic)"""

    def __init__(self, ops, case):
        super().__init__(ops, case, X.data(case))
        r = X.reference(case)
        n = case.cout
        exp = np.full((case.m + TAIL_ROWS, case.ldo), X.SENTINEL, dtype=np.float16)   # rows past M and the padding columns stay as they were
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
            assert tuple(self.exp_t.shape) == transposed_shape(case)
        if case.rowstat:
            self.exp_rs = torch.from_numpy(r.rowstat.astype(np.float32)).cuda()
        if case.chanstat:
            self.exp_cs = torch.from_numpy(r.chanstat.astype(np.float32)).cuda()

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
    prob.check(o, f"tile {d.tile} pipeline {d.pipeline} split {d.split_k} {'in-launch' if d.counters else 'reducer' if d.split_k > 1 else 'unsplit'}")
    return d

"""Per-kernel parity on the MI355X: every C-ABI op against a plain PyTorch fp32 CPU reference of the
same op on the same fp16-rounded inputs.  Tolerance (proposed; the reference states none):
max-abs <= 2^-8 * max|ref| and relative L2 <= 2e-3 for fp16 outputs; integer outputs exact or +-1 LSB."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as X
from videosd_amd.convform import conv_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def to_nhwc(x):  # [1,C,H,W] -> [H*W, C]
    return x[0].permute(1, 2, 0).reshape(-1, x.shape[1]).contiguous()


def from_nhwc(y, h, w):  # [H*W, C] -> [1,C,H,W]
    return y.reshape(h, w, -1).permute(2, 0, 1)[None]


def check(got, ref, what="", atol_scale=2.0 ** -8, rel=2e-3):
    got = got.float().cpu()
    ref = ref.float()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    lim = atol_scale * ref.abs().max().item() + 1e-6
    l2 = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
    assert err <= lim and l2 <= rel, f"{what}: max-abs {err:.4g} (limit {lim:.4g}), rel-L2 {l2:.3g}"


def run_conv(ops, x_list, h, w, weight, bias, *, ksize, stride=1, up_to=None, tile=None, split_k=None, act=0,
             rowvec=None, residual=None, residual2=None, out_scale=1.0, cin_pad=None, pipeline=None):
    """x_list: NCHW fp16 CPU tensors (concat sources). Returns (got [M,N] fp16 on cpu, ref NCHW fp32)."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    pw = pack_conv(weight, bias, cin_pad=cin_pad)
    pw.weight = pw.weight.cuda()
    pw.bias = None if pw.bias is None else pw.bias.cuda()
    g = Geom.conv(h, w, ksize=ksize, stride=stride, up_to=up_to)
    srcs = []
    for x in x_list:
        xn = to_nhwc(x)
        if cin_pad is not None and xn.shape[1] != cin_pad:
            xn = F.pad(xn, (0, cin_pad - xn.shape[1]))
        srcs.append(xn.cuda())
    n = weight.shape[0]
    ldo = max(8, (n + 7) // 8 * 8)
    out = torch.zeros(g.m, ldo, dtype=torch.float16, device="cuda")
    kw = {}
    if rowvec is not None:
        kw["rowvec"] = rowvec.cuda()
    if residual is not None:
        kw["residual"] = residual.cuda()
        kw["ldr"] = residual.shape[1]
    if residual2 is not None:
        kw["residual2"] = residual2.cuda()
    c0 = srcs[0].shape[1]
    c1 = srcs[1].shape[1] if len(srcs) > 1 else 0
    ops.conv(srcs[0], srcs[1] if len(srcs) > 1 else None, g, pw, out, ldo=ldo, c0=c0, c1=c1, act=act, out_scale=out_scale,
             tile=tile, split_k=split_k, pipeline=pipeline, **kw)
    ops.synchronize()
    # reference
    xin = torch.cat([x.float() for x in x_list], dim=1)
    if up_to is not None:
        xin = F.interpolate(xin, size=up_to, mode="nearest")
    ref = F.conv2d(xin, weight.float(), None if bias is None else bias.float(), stride=stride, padding=ksize // 2)
    if rowvec is not None:
        ref = ref + rowvec.float()[None, :, None, None]
    if act == 1:
        ref = F.relu(ref)
    elif act == 2:
        ref = F.silu(ref)
    elif act == 4:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif act == 6:
        ref = F.gelu(ref)
    ref = ref * out_scale
    if residual is not None:
        ref = ref + from_nhwc(residual.float(), g.ho, g.wo)
    if residual2 is not None:
        ref = ref + from_nhwc(residual2.float(), g.ho, g.wo)
    return out[:, :n].cpu(), to_nhwc(ref)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("split_k", [1, 3])
@pytest.mark.parametrize("pipeline", [0, 3, 4, 5, 6])
def test_conv3x3_all_tiles_splitk(ops, tile, split_k, pipeline):
    h, w, cin, cout = 18, 14, 128, 192  # M=252: ragged in M for every tile
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    b = rnd(cout, seed=3, scale=0.1)
    rv = rnd(cout, seed=4, scale=0.1)
    res = rnd(h * w, cout, seed=5)
    got, ref = run_conv(ops, [x], h, w, wt, b, ksize=3, tile=tile, split_k=split_k, rowvec=rv, residual=res,
                        pipeline=pipeline)
    check(got, ref, f"conv3x3 tile={tile} split={split_k} pipeline={pipeline}")


@pytest.mark.parametrize("tile", [0, 4, 6])
@pytest.mark.parametrize("pipeline", [8, 9])
def test_eight_wave_forms_give_the_bits_of_the_four_wave_forms(ops, tile, pipeline):
    """Pipelines 8 / 9 (round 6): the 3-stage buffer-load ring on EIGHT waves -- 4 x 2 waves, two per SIMD, half the accumulators
    and half the LDS-DMA instructions per wave.  The K order of every output element is the four-wave form's, so every epilogue
    class must give the four-wave form's bits: a 3x3 conv over a channel concat with time vector, SiLU and residual (ragged M
    and N), split over K in the launch and behind the reducer; a producer with row statistics; the LayerNorm-consuming qkv
    projection with its transposed V^T; GEGLU; the tile softmax.  Against fp32 too."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_geglu, pack_linear, pack_linear_ln

    base = 3 if pipeline == 8 else 5
    base_tile = 0  # (always against the 128 x 128 four-wave form: the four-wave 256 x 128 GEGLU walk rounds 3 of 256 000 outputs the
    #                other way -- a contraction the compiler picks differently in that one instantiation, scripts/geglu_bits.py)
    splits = ((1, True),) if tile == 6 else ((1, True), (3, True), (3, False))  # (... and unsplit only: its epilogue runs in row bands)
    h, w, c0, c1, cout = 18, 30, 128, 64, 328   # M = 540, N = 328: ragged for every tile
    a, b = rnd(1, c0, h, w, seed=1), rnd(1, c1, h, w, seed=2)
    wt = rnd(cout, c0 + c1, 3, 3, seed=3, scale=((c0 + c1) * 9) ** -0.5)
    bias, rv, res = rnd(cout, seed=4, scale=0.1), rnd(cout, seed=5, scale=0.1), rnd(h * w, cout, seed=6)
    for sp, ink in splits:
        ops.inkernel_splitk = ink
        try:
            got, ref = run_conv(ops, [a, b], h, w, wt, bias, ksize=3, tile=tile, split_k=sp, rowvec=rv, residual=res, act=2, pipeline=pipeline)
            four, _ = run_conv(ops, [a, b], h, w, wt, bias, ksize=3, tile=base_tile, split_k=sp, rowvec=rv, residual=res, act=2, pipeline=base)
        finally:
            ops.inkernel_splitk = True
        check(got, ref, f"eight waves, tile {tile} pipeline {pipeline} split {sp} in-launch {ink}")
        assert torch.equal(got, four), f"eight waves differ from four: tile {tile} pipeline {pipeline} split {sp} in-launch {ink}"
    # producer with row statistics -> LayerNorm-consuming qkv with V^T
    m, c = 1000, 384   # (V^T starts at column 2c = 768: a multiple of every tile's width)
    x, r0 = rnd(m, c, seed=11), rnd(m, c, seed=12)
    w0, b0 = rnd(c, c, seed=13, scale=c ** -0.5), rnd(c, seed=14, scale=0.1)
    p0 = ops.to_device_pack(pack_linear(w0, b0))
    gamma, beta = (1 + 0.1 * rnd(c, seed=15).float()).half(), rnd(c, seed=16, scale=0.1)
    wq, wk, wv = (rnd(c, c, seed=i, scale=c ** -0.5) for i in (17, 18, 19))
    pq = ops.to_device_pack(pack_linear_ln([wq, wk, wv], None, gamma, beta))
    ldt = 1024
    outs = []
    for tl, pl in ((base_tile, base), (tile, pipeline)):
        hh = torch.zeros(m, c, dtype=torch.float16, device="cuda")
        rs = torch.zeros(m, c // 64, 2, dtype=torch.float32, device="cuda")
        ops.conv(x.cuda(), None, Geom.linear(m), p0, hh, residual=r0.cuda(), rowstat_out=rs, split_k=1, tile=tl, pipeline=pl)
        qk = torch.zeros(m, 2 * c, dtype=torch.float16, device="cuda")
        vt = torch.zeros(c, ldt, dtype=torch.float16, device="cuda")
        ops.conv(hh, None, Geom.linear(m), pq, qk, ldo=2 * c, out_t=vt, ldt=ldt, t_col0=2 * c, ln_part=rs, split_k=1, tile=tl, pipeline=pl)
        ops.synchronize()
        outs.append((hh.cpu(), rs.cpu(), qk.cpu(), vt.cpu()))
    check(outs[1][0], F.linear(x.float(), w0.float(), b0.float()) + r0.float(), "eight waves: row-statistics producer")
    ln = F.layer_norm(outs[1][0].float(), (c,), gamma.float(), beta.float(), 1e-5)
    check(outs[1][2][:, :c], F.linear(ln, wq.float()), "eight waves: ln -> q", rel=3e-3)
    check(outs[1][3][:, :m], F.linear(ln, wv.float()).t(), "eight waves: ln -> v^T", rel=3e-3)
    for u, v in zip(outs[0], outs[1]):
        assert torch.equal(u, v), "eight waves differ from four (row statistics / fused LayerNorm / V^T)"
    # GEGLU
    hid = 256
    wg, bg = rnd(2 * hid, c, seed=21, scale=c ** -0.5), rnd(2 * hid, seed=22, scale=0.1)
    pg = ops.to_device_pack(pack_geglu(wg, bg))
    outs = []
    for tl, pl in ((base_tile, base), (tile, pipeline)):
        o = torch.zeros(m, hid, dtype=torch.float16, device="cuda")
        ops.conv(x.cuda(), None, Geom.linear(m), pg, o, tile=tl, split_k=1, pipeline=pl)
        ops.synchronize()
        outs.append(o.cpu())
    y = F.linear(x.float(), wg.float(), bg.float())
    check(outs[1], y[:, :hid] * F.gelu(y[:, hid:]), "eight waves: GEGLU")
    assert torch.equal(outs[0], outs[1]), "eight waves differ from four (GEGLU)"


def test_splitk_in_the_launch_on_a_grid_larger_than_the_chip(ops):
    """More workgroups than resident slots (20 480 rows): the in-launch split-K hand-over (slabs + arrival tickets, the last
    arriver sums eight slabs per round trip and runs the straight-line epilogue walk) with row statistics on the producer and a
    LayerNorm-consuming qkv projection with a transposed V^T on the consumer; the interleaved pipeline gives the same bits as the
    plain ring, the split forms agree with the fp32 reference.  (Round 4's persistent stream-K form had this test; the form left
    the library in round 5.)"""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_linear, pack_linear_ln

    m, c = 20480, 320
    x = rnd(m, c, seed=1)
    res = rnd(m, c, seed=2)
    w0, b0 = rnd(c, c, seed=3, scale=c ** -0.5), rnd(c, seed=4, scale=0.1)
    p0 = ops.to_device_pack(pack_linear(w0, b0))
    outs = []
    for pl, sp in ((3, 1), (5, 1), (3, 3)):
        h = torch.zeros(m, c, dtype=torch.float16, device="cuda")
        rs = torch.zeros(m, c // 64, 2, dtype=torch.float32, device="cuda")
        ops.conv(x.cuda(), None, Geom.linear(m), p0, h, residual=res.cuda(), rowstat_out=rs, split_k=sp, tile=3, pipeline=pl)
        ops.synchronize()
        check(h, F.linear(x.float(), w0.float(), b0.float()) + res.float(), f"producer pipeline={pl} parts={sp}")
        outs.append((h.cpu(), rs.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # (split 3: the fp32 partial sums are grouped differently from the one-pass accumulation, so the rows agree to rounding, not
    #  bit for bit; checked against the reference above)
    hq = outs[0][0].float()
    gamma, beta = (1 + 0.1 * rnd(c, seed=5).float()).half(), rnd(c, seed=6, scale=0.1)
    ln = F.layer_norm(hq, (c,), gamma.float(), beta.float(), 1e-5)
    wq, wk, wv = (rnd(c, c, seed=i, scale=c ** -0.5) for i in (7, 8, 9))
    pq = ops.to_device_pack(pack_linear_ln([wq, wk, wv], None, gamma, beta))
    ldt = m
    got = []
    for pl, sp in ((3, 1), (5, 1), (3, 2)):
        qk = torch.zeros(m, 2 * c, dtype=torch.float16, device="cuda")
        vt = torch.zeros(c, ldt, dtype=torch.float16, device="cuda")
        ops.conv(outs[0][0].cuda(), None, Geom.linear(m), pq, qk, ldo=2 * c, out_t=vt, ldt=ldt, t_col0=2 * c, ln_part=outs[0][1].cuda(),
                 split_k=sp, tile=3, pipeline=pl)
        ops.synchronize()
        check(qk[:, :c], F.linear(ln, wq.float()), f"ln->q pipeline={pl}", rel=3e-3)
        check(vt, F.linear(ln, wv.float()).t(), f"ln->v^T pipeline={pl}", rel=3e-3)
        got.append((qk.cpu(), vt.cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_conv_group_equals_its_members_launched_one_by_one(ops):
    """vsd_conv_gemm_group (round 5): several independent problems in ONE grid, every workgroup running what the plain kernel would
    run for its problem.  Members of different shapes -- the ControlNet merges (1x1, a scale read from device memory, the UNet tensor
    as residual; M from 64 to 4096, ragged M and N) and a 3x3 layer with a time vector -- in every kernel form a group may take:
    bit for bit what the members give launched one by one in that form, against fp32 too; the tuned form is remembered per group;
    what a group cannot hold is refused by name."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv, pack_linear

    members, refs = [], []
    scales = torch.tensor([0.1, 0.4, 1.0, 2.5, 1.0, 1.0], dtype=torch.float32, device="cuda")
    for i, (m, c, n) in enumerate([(4096, 320, 320), (1024, 640, 640), (256, 1280, 1280), (64, 1280, 1280), (100, 320, 200)]):
        x, res = rnd(m, c, seed=10 + i), rnd(m, n, seed=20 + i)
        wt, b = rnd(n, c, seed=30 + i, scale=c ** -0.5), rnd(n, seed=40 + i, scale=0.1)
        pw = ops.to_device_pack(pack_linear(wt, b))
        out = torch.zeros(m, (n + 7) // 8 * 8, dtype=torch.float16, device="cuda")
        members.append(((x.cuda(), None, Geom.linear(m), pw, out), dict(out_scale_dev=scales[i:i + 1], residual=res.cuda(), ldo=out.shape[1], ldr=n)))
        refs.append((F.linear(x.float(), wt.float(), b.float()) * float(scales[i]) + res.float(), n))
    h, w, c, n = 18, 14, 128, 192   # a 3x3 member with a time vector and SiLU
    x = rnd(1, c, h, w, seed=50)
    wt, b, rv = rnd(n, c, 3, 3, seed=51, scale=(9 * c) ** -0.5), rnd(n, seed=52, scale=0.1), rnd(n, seed=53, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, b))
    out = torch.zeros(h * w, n, dtype=torch.float16, device="cuda")
    members.append(((to_nhwc(x).cuda(), None, Geom.conv(h, w), pw, out), dict(rowvec=rv.cuda(), act=2)))
    refs.append((to_nhwc(F.silu(F.conv2d(x.float(), wt.float(), b.float(), padding=1) + rv.float()[None, :, None, None])), n))
    for form in ops.GROUP_FORMS:
        for a, kw in members:
            a[4].zero_()
        ops.conv_group(members, form=(form[0], 1, True, form[1]))
        ops.synchronize()
        got = [a[4].clone() for a, kw in members]
        for (a, kw), g_, (ref, n_) in zip(members, got, refs):
            check(g_[:, :n_], ref, f"group form {form}")
            a[4].zero_()
            ops.conv(*a, tile=form[0], split_k=1, pipeline=form[1], **kw)
            ops.synchronize()
            assert torch.equal(a[4], g_), f"member alone differs from the group, form {form}"
    best, table = ops.tune_group(members)
    # (members of different shapes: unsplit forms + "every member as a launch of its own")
    assert ops.tile_override[ops.group_key(members)] == (best[1], 1, True, best[4]) and len(table) == len(ops.GROUP_FORMS) + 1
    ops.conv_group(members)  # (takes the remembered form)
    ops.synchronize()
    check(members[0][0][4][:, :320], refs[0][0], "group, tuned form")
    with pytest.raises(ValueError):
        ops.conv_group(members + members)  # more than VSD_CONV_GROUP_MAX
    x8 = rnd(64, 8, seed=60)  # Cin % 64 != 0: the generic operand path, which a group does not have
    p8 = ops.to_device_pack(pack_linear(rnd(64, 8, seed=61), None))
    with pytest.raises(RuntimeError, match="buffer-load"):
        ops.conv_group([((x8.cuda(), None, Geom.linear(64), p8, torch.zeros(64, 64, dtype=torch.float16, device="cuda")), {})])


def test_group_members_at_their_own_splits_and_scaled_residuals_in_every_reduction_form(ops):
    """(1) conv_group(split=OWN_SPLIT) -- a ResnetBlock's conv1 (3x3, time vector, split over K at the deep levels) and its shortcut conv
    (1x1 over the concat of two sources, unsplit) in ONE grid, every member at the split its own table entry has: bit for bit the two
    launches, in every form the tuner may pick for the group, against fp32 too; a member whose own form is the halo patch sends
    the members out alone.  (2) A scaled layer with a residual (the ControlNet merges: out_scale_dev + the UNet tensor) has the
    same bits behind the reducer kernel, the in-launch tail and unsplit-tile walks: scale and residual are ONE fused multiply-add
    everywhere (round 5: the reducer's epilogue rounded twice)."""
    from videosd_amd import lib as L
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv, pack_linear

    h = w = 8
    c0, c1, n = 1280, 1280, 1280
    x, skip = rnd(1, c0, h, w, seed=100), rnd(1, c1, h, w, seed=101)
    t1 = rnd(1, c0 + c1, h, w, seed=102)
    w1, rv = rnd(n, c0 + c1, 3, 3, seed=103, scale=(9 * (c0 + c1)) ** -0.5), rnd(n, seed=104, scale=0.1)
    ws, bs = rnd(n, c0 + c1, seed=105, scale=(c0 + c1) ** -0.5), rnd(n, seed=106, scale=0.1)
    p1, ps = ops.to_device_pack(pack_conv(w1, None)), ops.to_device_pack(pack_linear(ws, bs))
    o1 = torch.zeros(h * w, n, dtype=torch.float16, device="cuda")
    o2 = torch.zeros(h * w, n, dtype=torch.float16, device="cuda")
    members = [((to_nhwc(t1).cuda(), None, Geom.conv(h, w), p1, o1), dict(rowvec=rv.cuda())),
               ((to_nhwc(x).cuda(), to_nhwc(skip).cuda(), Geom.linear(h * w), ps, o2), dict(c0=c0, c1=c1))]
    refs = [to_nhwc(F.conv2d(t1.float(), w1.float(), None, padding=1) + rv.float()[None, :, None, None]),
            F.linear(torch.cat([to_nhwc(x).float(), to_nhwc(skip).float()], 1), ws.float(), bs.float())]
    k1 = ops.conv_key_of(members[0][0][2], p1, members[0][1])
    k2 = ops.conv_key_of(members[1][0][2], ps, members[1][1])
    saved = {k: ops.tile_override.get(k) for k in (k1, k2)}
    try:
        ops.tile_override[k1] = (L.TILE_64x128, 12, False, 5)   # conv1: split 12 + reducer, as the table has it at 8 x 8
        ops.tile_override[k2] = (L.TILE_64x64, 1, False, 5)     # the shortcut: unsplit
        assert ops.own_splits(members) == [12, 1]
        alone = []
        for a, kw in members:
            a[4].zero_()
            ops.conv(*a, **kw)
            ops.synchronize()
            alone.append(a[4].clone())
        cands = ops.group_candidates(members, split=ops.OWN_SPLIT)
        assert all(f[1] == 0 for f in cands if f[0] != ops.GROUP_ALONE) and any(not f[2] for f in cands) and cands[-1][0] == ops.GROUP_ALONE
        for form in cands:
            for a, kw in members:
                a[4].zero_()
            for _ in range(2):
                ops.conv_group(members, form=form, split=ops.OWN_SPLIT)
            ops.synchronize()
            for (a, kw), al, ref in zip(members, alone, refs):
                check(a[4], ref, f"own-split group form {form}")
                assert torch.equal(a[4], al), f"own-split group form {form}: bits differ from the member's own launch"
        best, table = ops.tune_group(members, split=ops.OWN_SPLIT)
        assert ops.group_key(members, ops.OWN_SPLIT) in ops.tile_override and len(table) == len(cands)
        for a, kw in members:
            a[4].zero_()
        ops.conv_group(members, split=ops.OWN_SPLIT)  # (the remembered form)
        ops.synchronize()
        assert all(torch.equal(a[4], al) for (a, kw), al in zip(members, alone))
        ops.tile_override[k1] = (L.TILE_128x64, 1, True, 7)   # conv1 in the halo-patch form: another K order -> no shared grid
        assert ops.own_splits(members) is None
        for a, kw in members:
            a[4].zero_()
        ops.conv_group(members, split=ops.OWN_SPLIT)
        ops.synchronize()
        for (a, kw), ref in zip(members, refs):
            check(a[4], ref, "members sent out alone")
    finally:
        for k, v in saved.items():
            if v is None:
                ops.tile_override.pop(k, None)
            else:
                ops.tile_override[k] = v
        ops.tile_override.pop(ops.group_key(members, ops.OWN_SPLIT), None)
    # (2) scale + residual
    m, c, n = 256, 1280, 1280
    xs, res = rnd(m, c, seed=110), rnd(m, n, seed=111)
    wt, b = rnd(n, c, seed=112, scale=c ** -0.5), rnd(n, seed=113, scale=0.1)
    pw = ops.to_device_pack(pack_linear(wt, b))
    scale = torch.tensor([0.3162], dtype=torch.float32, device="cuda")
    ref = F.linear(xs.float(), wt.float(), b.float()) * 0.3162 + res.float()
    outs = []
    for tile, sp, ink, pl in [(L.TILE_64x64, 4, True, 3), (L.TILE_64x128, 4, False, 5), (L.TILE_128x64, 4, True, 5), (L.TILE_64x64, 4, False, 0)]:
        ops.inkernel_splitk = ink
        o = torch.zeros(m, n, dtype=torch.float16, device="cuda")
        ops.conv(xs.cuda(), None, Geom.linear(m), pw, o, out_scale_dev=scale, residual=res.cuda(), ldr=n, tile=tile, split_k=sp, pipeline=pl)
        ops.synchronize()
        check(o, ref, f"scaled residual, tile {tile} split {sp} inkernel {ink}")
        outs.append(o)
    ops.inkernel_splitk = True
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "a scaled layer with a residual: the reduction forms differ in their bits"
    o1 = torch.zeros(m, n, dtype=torch.float16, device="cuda")
    ops.conv(xs.cuda(), None, Geom.linear(m), pw, o1, out_scale=0.3162, residual=res.cuda(), ldr=n, residual2=res.cuda(), tile=L.TILE_64x64, split_k=1)
    o2 = torch.zeros(m, n, dtype=torch.float16, device="cuda")
    ops.inkernel_splitk = False
    ops.conv(xs.cuda(), None, Geom.linear(m), pw, o2, out_scale=0.3162, residual=res.cuda(), ldr=n, residual2=res.cuda(), tile=L.TILE_64x64, split_k=1,
             pipeline=0)
    ops.inkernel_splitk = True
    ops.synchronize()
    assert torch.equal(o1, o2)


def test_twin_convs_split_over_k_share_a_grid_and_a_reducer(ops):
    """A group whose members are split over K (round 5: the twin layers of the UNet and the ControlNet encoder, one shape, two weight
    sets): slabs reduced by ONE more launch for the group, or by the last workgroup of each tile in the launch -- every member with a
    workspace and a counter set of its own.  Bit for bit the members launched one by one in the same form; the tuner's table for such
    a pair holds split forms and the "alone" entry, and what it picks reproduces the reference."""
    from videosd_amd import lib as L
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    h = w = 8
    c, n = 1280, 1280
    members, refs = [], []
    for i in range(2):
        x = rnd(1, c, h, w, seed=70 + i)
        wt, b, rv = rnd(n, c, 3, 3, seed=72 + i, scale=(9 * c) ** -0.5), rnd(n, seed=74 + i, scale=0.1), rnd(n, seed=76 + i, scale=0.1)
        res = rnd(h * w, n, seed=78 + i)
        pw = ops.to_device_pack(pack_conv(wt, b))
        out = torch.zeros(h * w, n, dtype=torch.float16, device="cuda")
        members.append(((to_nhwc(x).cuda(), None, Geom.conv(h, w), pw, out), dict(rowvec=rv.cuda(), residual=res.cuda())))
        refs.append(to_nhwc(F.conv2d(x.float(), wt.float(), b.float(), padding=1) + rv.float()[None, :, None, None]) + res.float())
    for form in [(L.TILE_64x64, 6, False, 3), (L.TILE_64x64, 6, True, 3), (L.TILE_64x128, 4, False, 5), (L.TILE_128x64, 8, True, 5),
                 (L.TILE_64x64, 12, False, 5)]:
        for a, kw in members:
            a[4].zero_()
        for _ in range(3):  # (the counters of the in-launch form return to zero: a second and third launch see them clean)
            ops.conv_group(members, form=form)
        ops.synchronize()
        got = [a[4].clone() for a, kw in members]
        ops.inkernel_splitk = form[2]
        for (a, kw), g_, ref in zip(members, got, refs):
            check(g_, ref, f"twin group form {form}")
            a[4].zero_()
            ops.conv(*a, tile=form[0], split_k=form[1], pipeline=form[3], **kw)
            ops.synchronize()
            assert torch.equal(a[4], g_), f"member alone differs from the twin group, form {form}"
        ops.inkernel_splitk = True
    best, table = ops.tune_group(members, split=6)
    forms = {t[1:] for t in table}
    assert any(f[1] == 6 and not f[2] for f in forms) and any(f[1] == 6 and f[2] for f in forms) and (ops.GROUP_ALONE, 1, True, 0) in forms
    assert all(f[1] == 6 for f in forms if f[0] != ops.GROUP_ALONE) and ops.group_key(members, 6) in ops.tile_override
    # `pair` (the engine's entry point) runs two twin convs at the split they have as launches of their own -- a conv's bits depend
    # on its split alone, not on tile / pipeline / where the slabs are summed -- so the pair gives the bits the two launches give
    for a, kw in members:
        a[4].zero_()
        ops.conv(*a, **kw)
    ops.synchronize()
    alone = [a[4].clone() for a, kw in members]
    sp = ops.pair_split(*members[0], *members[1])
    assert sp is not None and sp == ops.conv(*members[0][0], _desc_only=True, **members[0][1]).split_k
    ops.tune_group(members, split=sp)
    for a, kw in members:
        a[4].zero_()
    ops.pair((ops.conv, members[0][0], members[0][1]), (ops.conv, members[1][0], members[1][1]))
    ops.synchronize()
    for (a, kw), ref, al in zip(members, refs, alone):
        check(a[4], ref, "twin pair")
        assert torch.equal(a[4], al), "the pair's bits differ from the two launches'"
    # members whose own forms sum over K in different orders (here: one forced into the halo-patch form) do not share a grid
    key = ops.conv_key_of(members[0][0][2], members[0][0][3], members[0][1])
    saved = ops.tile_override.get(key)
    ops.tile_override[key] = (L.TILE_128x64, 1, True, 7)
    halo_ok = conv_call(members[0][0][2], members[0][0][3]).halo_ok
    assert (ops.pair_split(*members[0], *members[1]) is None) == halo_ok
    if saved is None:
        del ops.tile_override[key]
    else:
        ops.tile_override[key] = saved


def test_pair_runs_two_calls_of_one_op_as_one_grid(ops):
    """vsd_pair_begin / join / end (round 5): the second operation's launches join the first one's -- GroupNorm (one-launch and
    two-launch forms), attention, the fused transformer tails -- same bits as the two calls alone; the library reports how many
    launches went out as pairs; a second operation of another shape joins nothing and both still run; pair calls out of order are
    refused."""
    import ctypes as C

    def joined(run_a, run_b):
        ops.ctx.call("vsd_pair_begin")
        run_a()
        ops.ctx.call("vsd_pair_join")
        ops._widx = 1
        try:
            run_b()
        finally:
            ops._widx = None
        n = C.c_int(-1)
        ops.ctx.call("vsd_pair_end", C.byref(n))
        return n.value

    # GroupNorm: 16x16x1280 (one launch), 64x64x320 (two launches)
    for hw, c, want in ((256, 1280, 1), (4096, 320, 2)):
        xs = [rnd(hw, c, seed=80 + i).cuda() for i in range(2)]
        gb = [(rnd(c, seed=82 + i).cuda(), rnd(c, seed=84 + i).cuda()) for i in range(2)]
        alone = [torch.zeros(hw, c, dtype=torch.float16, device="cuda") for _ in range(2)]
        both = [torch.zeros(hw, c, dtype=torch.float16, device="cuda") for _ in range(2)]
        for i in range(2):
            ops.groupnorm(xs[i], None, c, 0, hw, 32, 1e-5, gb[i][0], gb[i][1], True, alone[i])
        n = joined(lambda: ops.groupnorm(xs[0], None, c, 0, hw, 32, 1e-5, gb[0][0], gb[0][1], True, both[0]),
                   lambda: ops.groupnorm(xs[1], None, c, 0, hw, 32, 1e-5, gb[1][0], gb[1][1], True, both[1]))
        ops.synchronize()
        assert n == want, (hw, c, n)
        assert torch.equal(alone[0], both[0]) and torch.equal(alone[1], both[1]) and not torch.equal(both[0], both[1])
        ref = F.silu(F.group_norm(xs[1].float().t().reshape(1, c, hw), 32, gb[1][0].float(), gb[1][1].float(), 1e-5))[0].t()
        check(both[1], ref.cpu(), f"paired groupnorm {hw}x{c}")
    # attention: 1024 queries x 77 keys, 8 heads of 80 (the 640-wide level's cross-attention)
    sq, sk, heads, d = 1024, 77, 8, 80
    qs = [rnd(sq, heads * d, seed=90 + i).cuda() for i in range(2)]
    ks = [rnd(sk, heads * d, seed=92 + i).cuda() for i in range(2)]
    vts = [torch.zeros(heads * d, 128, dtype=torch.float16, device="cuda") for _ in range(2)]
    for i in range(2):
        vts[i][:, :sk] = rnd(heads * d, sk, seed=94 + i).cuda()
    alone = [torch.zeros(sq, heads * d, dtype=torch.float16, device="cuda") for _ in range(2)]
    both = [torch.zeros(sq, heads * d, dtype=torch.float16, device="cuda") for _ in range(2)]
    att = lambda i, o: ops.attention(qs[i], heads * d, ks[i], heads * d, vts[i], 128, o, heads * d, sq, sk, heads, d, d ** -0.5)  # noqa: E731
    for i in range(2):
        att(i, alone[i])
    assert joined(lambda: att(0, both[0]), lambda: att(1, both[1])) == 1
    ops.synchronize()
    assert torch.equal(alone[0], both[0]) and torch.equal(alone[1], both[1]) and not torch.equal(both[0], both[1])
    qh = qs[1].float().reshape(sq, heads, d).transpose(0, 1)
    kh = ks[1].float().reshape(sk, heads, d).transpose(0, 1)
    vh = vts[1][:, :sk].float().reshape(heads, d, sk).transpose(1, 2)
    ref = (torch.softmax(qh @ kh.transpose(1, 2) * d ** -0.5, -1) @ vh).transpose(0, 1).reshape(sq, heads * d)
    check(both[1], ref.cpu(), "paired attention")
    # the fused transformer tails, through ops.pair (the engine's entry point)
    c, m = 320, 4096
    _w, packs = _tail_weights(c)
    pk = {k: ops.to_device_pack(v) for k, v in packs.items()}
    ins = [(rnd(m, c, seed=110 + i).cuda(), (rnd(m, c, seed=112 + i).float() * 2 + 0.5).half().cuda(), rnd(m, c, seed=114 + i).cuda(),
            rnd(m, c, seed=116 + i).cuda()) for i in range(2)]
    z = lambda: torch.zeros(m, c, dtype=torch.float16, device="cuda")  # noqa: E731
    alone = [(z(), z(), z()) for _ in range(2)]
    both = [(z(), z(), z()) for _ in range(2)]
    for i in range(2):
        ops.tail_a(ins[i][0], ins[i][1], m, pk["out1"], pk["q2"], alone[i][0], alone[i][1])
        ops.tail_b(ins[i][3], alone[i][0], ins[i][2], m, pk["out2"], pk["ff1"], pk["ff2"], pk["proj"], alone[i][2])
    ops.pair((ops.tail_a, (ins[0][0], ins[0][1], m, pk["out1"], pk["q2"], both[0][0], both[0][1]), {}),
             (ops.tail_a, (ins[1][0], ins[1][1], m, pk["out1"], pk["q2"], both[1][0], both[1][1]), {}))
    ops.pair((ops.tail_b, (ins[0][3], both[0][0], ins[0][2], m, pk["out2"], pk["ff1"], pk["ff2"], pk["proj"], both[0][2]), {}),
             (ops.tail_b, (ins[1][3], both[1][0], ins[1][2], m, pk["out2"], pk["ff1"], pk["ff2"], pk["proj"], both[1][2]), {}))
    ops.synchronize()
    for i in range(2):
        for j in range(3):
            assert torch.equal(alone[i][j], both[i][j]) and float(both[i][j].abs().sum()) > 0, (i, j)
    assert not torch.equal(both[0][2], both[1][2])
    # a second operation of another shape: nothing joins, both run
    y0, y1 = torch.zeros(256, 1280, dtype=torch.float16, device="cuda"), torch.zeros(1024, 640, dtype=torch.float16, device="cuda")
    x1 = rnd(1024, 640, seed=99).cuda()
    g1, b1 = rnd(640, seed=98).cuda(), rnd(640, seed=97).cuda()
    n = joined(lambda: ops.groupnorm(xs[0][:256].contiguous() if xs[0].shape[0] != 256 else xs[0], None, 320, 0, 256, 32, 1e-5,
                                     g1[:320].contiguous(), b1[:320].contiguous(), False, y0),
               lambda: ops.groupnorm(x1, None, 640, 0, 1024, 32, 1e-5, g1, b1, False, y1))
    ops.synchronize()
    assert n == 0 and float(y0[:, :320].abs().sum()) > 0 and float(y1.abs().sum()) > 0
    # protocol errors are reported, and leave no pair open
    with pytest.raises(RuntimeError, match="pair_join"):
        ops.ctx.call("vsd_pair_join")
    with pytest.raises(RuntimeError, match="pair_end"):
        ops.ctx.call("vsd_pair_end", None)
    ops.ctx.call("vsd_pair_begin")
    with pytest.raises(RuntimeError, match="already open"):
        ops.ctx.call("vsd_pair_begin")
    ops.ctx.call("vsd_pair_join")
    ops.ctx.call("vsd_pair_end", None)


def test_throughput_mode_tuning_times_candidates_with_four_lanes_busy(ops):
    """HipOps.tune_conv with tune_mode = 1: every candidate alone first, then the shortlist with four copies in flight on the four
    launch lanes (captured graphs); the choice lands under a key of its own (last field 1) beside the latency-mode entry, and a
    conv run with it still matches the reference."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_linear

    m, n, k = 1280, 640, 640
    x, res = rnd(m, k, seed=1), rnd(m, n, seed=2)
    wt, b = rnd(n, k, seed=3, scale=k ** -0.5), rnd(n, seed=4, scale=0.1)
    pw = ops.to_device_pack(pack_linear(wt, b))
    out = torch.zeros(m, n, dtype=torch.float16, device="cuda")
    args, kw = (x.cuda(), None, Geom.linear(m), pw, out), dict(residual=res.cuda())
    saved = dict(ops.tile_override)
    try:
        ops.tune_mode = 0
        best0, table0 = ops.tune_conv(args, kw)
        key0 = ops.conv_key_of(args[2], pw, kw)
        ops.tune_mode = 1
        best1, table1 = ops.tune_conv(args, kw)
        key1 = ops.conv_key_of(args[2], pw, kw)
        assert key0[:-1] == key1[:-1] and (key0[-1], key1[-1]) == (0, 1)
        assert key0 in ops.tile_override and key1 in ops.tile_override
        # (the shortlist of mode 1 is cut from ITS candidates -- the eight-wave forms exist there only -- so it may be the longer table)
        assert len(table1) >= 1 and len(table0) >= 1 and all(us > 0 for us, *_ in table1)
        ops.conv(*args, **kw)   # (takes the throughput-mode entry: tune_mode is still 1)
        ops.synchronize()
        check(out, F.linear(x.float(), wt.float(), b.float()) + res.float(), "conv with the throughput-mode choice")
    finally:
        ops.tune_mode = 0
        ops.tile_override.clear()
        ops.tile_override.update(saved)


@pytest.mark.parametrize("pipeline", [0, 3, 4, 5, 6])
def test_pipelines_are_bit_identical_and_handle_short_k(ops, pipeline):
    # K = 1..5 tiles (shorter than the ring), ragged M and N
    for cin in (64, 128, 320):
        h, w, cout = 9, 11, 72
        x = rnd(1, cin, h, w, seed=1)
        wt = rnd(cout, cin, 1, 1, seed=2, scale=cin ** -0.5)
        got, ref = run_conv(ops, [x], h, w, wt, rnd(cout, seed=3, scale=0.1), ksize=1, tile=2, pipeline=pipeline)
        base, _ = run_conv(ops, [x], h, w, wt, rnd(cout, seed=3, scale=0.1), ksize=1, tile=2, pipeline=0)
        check(got, ref, f"short-K cin={cin} pipeline={pipeline}")
        assert torch.equal(got, base)


def test_splitk_inkernel_reduction_is_bit_identical_to_reduce_kernel(ops):
    h, w, cin, cout = 16, 16, 640, 320
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    b = rnd(cout, seed=3, scale=0.1)
    res = rnd(h * w, cout, seed=5)
    outs = []
    for inkernel in (True, False, True):
        ops.inkernel_splitk = inkernel
        got, ref = run_conv(ops, [x], h, w, wt, b, ksize=3, tile=2, split_k=6, residual=res, act=2)
        check(got, ref, f"split-K inkernel={inkernel}")
        outs.append(got)
    ops.inkernel_splitk = True
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert int(ops._counters[0].abs().sum()) == 0  # every tile's arrival counter is back at zero


def test_conv3x3_sd_width_deep_k(ops):
    h, w, cin, cout = 8, 8, 2560, 1280  # the deepest K of the UNet (23040), small M -> split-K heuristic path
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    got, ref = run_conv(ops, [x[:, :1280], x[:, 1280:]], h, w, wt, None, ksize=3)
    check(got, ref, "conv 2560->1280 concat")


@pytest.mark.parametrize("c0,c1", [(128, 64), (64, 128), (320, 320)])
def test_conv_concat_sources(ops, c0, c1):
    h, w, cout = 12, 10, 128
    a, b = rnd(1, c0, h, w, seed=1), rnd(1, c1, h, w, seed=2)
    wt = rnd(cout, c0 + c1, 3, 3, seed=3, scale=((c0 + c1) * 9) ** -0.5)
    got, ref = run_conv(ops, [a, b], h, w, wt, rnd(cout, seed=4, scale=0.1), ksize=3)
    check(got, ref, "concat conv3x3")
    wt1 = rnd(cout, c0 + c1, 1, 1, seed=5, scale=(c0 + c1) ** -0.5)
    got, ref = run_conv(ops, [a, b], h, w, wt1, None, ksize=1)
    check(got, ref, "concat conv1x1 (shortcut)")


@pytest.mark.parametrize("hs,ws,up", [(7, 12, (14, 24)), (14, 24, (27, 48)), (4, 4, (8, 8))])
def test_conv_nearest_upsample_folded(ops, hs, ws, up):
    cin, cout = 128, 64
    x = rnd(1, cin, hs, ws, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    got, ref = run_conv(ops, [x], hs, ws, wt, rnd(cout, seed=3, scale=0.1), ksize=3, up_to=up)
    check(got, ref, f"upsample {hs}x{ws}->{up}")


@pytest.mark.parametrize("h,w", [(16, 16), (27, 48), (7, 12), (1, 1)])
def test_conv_stride2(ops, h, w):
    cin, cout = 64, 64
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    got, ref = run_conv(ops, [x], h, w, wt, None, ksize=3, stride=2)
    check(got, ref, f"stride2 {h}x{w}")


@pytest.mark.parametrize("cin,cout,pad", [(3, 64, 8), (4, 320, 8), (16, 32, None), (96, 256, None), (64, 3, None), (320, 4, None)])
def test_conv_small_channels_generic_path(ops, cin, cout, pad):
    h, w = 20, 12
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    for pl in (0, 3, 5):
        got, ref = run_conv(ops, [x], h, w, wt, rnd(cout, seed=3, scale=0.1), ksize=3, cin_pad=pad, act=2, pipeline=pl)
        check(got, ref, f"generic conv {cin}->{cout} pipeline={pl}")


@pytest.mark.parametrize("act", [0, 1, 2, 4, 6])  # none, ReLU, SiLU, quick-GELU (CLIP-L), erf GELU (SDXL's second text tower)
def test_linear_epilogues(ops, act):
    m, k, n = 77, 768, 320
    x = rnd(1, k, 1, m, seed=1)
    wt = rnd(n, k, 1, 1, seed=2, scale=k ** -0.5)
    res, res2 = rnd(m, n, seed=3), rnd(m, n, seed=4)
    got, ref = run_conv(ops, [x], 1, m, wt, rnd(n, seed=5, scale=0.1), ksize=1, act=act, residual=res, residual2=res2,
                        out_scale=0.37)
    check(got, ref, f"linear act={act}")
    if act == 6:  # ... and behind the split-K reducer / the in-launch reduction
        for inkernel in (False, True):
            ops.inkernel_splitk = inkernel
            got, ref = run_conv(ops, [x], 1, m, wt, rnd(n, seed=5, scale=0.1), ksize=1, act=act, residual=res, split_k=3, tile=2)
            check(got, ref, f"linear act=6 split-K inkernel={inkernel}")
        ops.inkernel_splitk = True


@pytest.mark.parametrize("tile", [0, 3])
def test_geglu_fused(ops, tile):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_geglu

    m, c = 200, 320
    x = rnd(m, c, seed=1)
    wt = rnd(8 * c, c, seed=2, scale=c ** -0.5)
    b = rnd(8 * c, seed=3, scale=0.1)
    pw = pack_geglu(wt, b)
    pw.weight, pw.bias = pw.weight.cuda(), pw.bias.cuda()
    out = torch.zeros(m, 4 * c, dtype=torch.float16, device="cuda")
    ops.conv(x.cuda(), None, Geom.linear(m), pw, out, tile=tile)
    ops.synchronize()
    y = F.linear(x.float(), wt.float(), b.float())
    hid, gate = y.chunk(2, dim=-1)
    check(out, hid * F.gelu(gate), "geglu")


@pytest.mark.parametrize("m,c", [(300, 320), (64, 1280), (1000, 128)])
def test_fused_layernorm_producer_rowstats_and_consumer(ops, m, c):
    """out1 GEMM leaves per-row (sum, sumsq); the next GEMM (QKV with V^T, GEGLU) applies LayerNorm from them."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_geglu_ln, pack_linear, pack_linear_ln

    x = rnd(m, c, seed=1)
    res = (rnd(m, c, seed=2).float() * 3 + 1.5).half()
    w0, b0 = rnd(c, c, seed=3, scale=c ** -0.5), rnd(c, seed=4, scale=0.1)
    p0 = ops.to_device_pack(pack_linear(w0, b0))
    h = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    rs = torch.zeros(m, c // 64, 2, dtype=torch.float32, device="cuda")
    for split in (1, 2):
        ops.conv(x.cuda(), None, Geom.linear(m), p0, h, residual=res.cuda(), rowstat_out=rs, split_k=split, tile=2)
        ops.synchronize()
        href = F.linear(x.float(), w0.float(), b0.float()) + res.float()
        check(h, href, "producer out")
        hq = h.float().cpu()
        tot = rs.sum(dim=1).cpu()
        assert torch.allclose(tot[:, 0], hq.sum(dim=1), rtol=1e-4, atol=1e-2)
        assert torch.allclose(tot[:, 1], (hq * hq).sum(dim=1), rtol=1e-4, atol=1e-2)
    gamma, beta = (1 + 0.1 * rnd(c, seed=5).float()).half(), rnd(c, seed=6, scale=0.1)
    ln = F.layer_norm(hq, (c,), gamma.float(), beta.float(), 1e-5)
    # consumer 1: fused QKV with transposed V
    wq, wk, wv = (rnd(c, c, seed=i, scale=c ** -0.5) for i in (7, 8, 9))
    pq = ops.to_device_pack(pack_linear_ln([wq, wk, wv], None, gamma, beta))
    ldt = (m + 63) // 64 * 64
    qk = torch.zeros(m, 2 * c, dtype=torch.float16, device="cuda")
    vt = torch.zeros(c, ldt, dtype=torch.float16, device="cuda")
    for split, ink in ((1, True), (2, True), (2, False)):
        ops.inkernel_splitk = ink
        ops.conv(h, None, Geom.linear(m), pq, qk, ldo=2 * c, out_t=vt, ldt=ldt, t_col0=2 * c, ln_part=rs, split_k=split, tile=2)
        ops.synchronize()
        check(qk[:, :c], F.linear(ln, wq.float()), f"ln->q split={split}", rel=3e-3)
        check(qk[:, c:], F.linear(ln, wk.float()), f"ln->k split={split}", rel=3e-3)
        check(vt[:, :m], F.linear(ln, wv.float()).t(), f"ln->v^T split={split}", rel=3e-3)
    ops.inkernel_splitk = True
    # consumer 2: GEGLU
    wf, bf = rnd(8 * c, c, seed=10, scale=c ** -0.5), rnd(8 * c, seed=11, scale=0.1)
    pf = ops.to_device_pack(pack_geglu_ln(wf, bf, gamma, beta))
    f = torch.zeros(m, 4 * c, dtype=torch.float16, device="cuda")
    ops.conv(h, None, Geom.linear(m), pf, f, ln_part=rs)
    ops.synchronize()
    hid, gate = F.linear(ln, wf.float(), bf.float()).chunk(2, dim=-1)
    check(f, hid * F.gelu(gate), "ln->geglu", rel=3e-3)


@pytest.mark.parametrize("c", [320, 1280])
def test_fused_layernorm_on_rows_with_a_large_mean_and_outlier_channels(ops, c):
    """the folded LayerNorm computes rstd * (x.W' - mean * s) from one-pass (sum, sumsq) partials -- two large
    terms cancel.  Real SD residual streams have rows with |mean| >> std and a few outlier channels; check that regime
    (mean 50, std 0.5, four channels 100x larger) against an explicit fp32 LayerNorm + linear of the same fp16 rows."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_geglu_ln, pack_linear, pack_linear_ln

    m = 256
    g = torch.Generator().manual_seed(5)
    h0 = 50.0 + 0.5 * torch.randn(m, c, generator=g)
    h0[:, [3, 77, 130, c - 5]] *= 100.0
    # the rows reach the consumer through a producer GEMM (identity weights) that also leaves the row partials
    eye = torch.eye(c).half()
    p0 = ops.to_device_pack(pack_linear(eye, None))
    h = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    rs = torch.zeros(m, c // 64, 2, dtype=torch.float32, device="cuda")
    ops.conv(h0.half().cuda(), None, Geom.linear(m), p0, h, rowstat_out=rs, tile=2)
    ops.synchronize()
    hq = h.float().cpu()
    assert torch.equal(hq, h0.half().float())
    gamma, beta = (1 + 0.1 * rnd(c, seed=5).float()).half(), rnd(c, seed=6, scale=0.1)
    ln = F.layer_norm(hq, (c,), gamma.float(), beta.float(), 1e-5)
    wq = rnd(c, c, seed=7, scale=c ** -0.5)
    pq = ops.to_device_pack(pack_linear_ln([wq], None, gamma, beta))
    q = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    ops.conv(h, None, Geom.linear(m), pq, q, ln_part=rs, tile=2)
    ops.synchronize()
    check(q, F.linear(ln, wq.float()), "ln(large mean)->q", rel=5e-3)
    wf, bf = rnd(8 * c, c, seed=10, scale=c ** -0.5), rnd(8 * c, seed=11, scale=0.1)
    pf = ops.to_device_pack(pack_geglu_ln(wf, bf, gamma, beta))
    f = torch.zeros(m, 4 * c, dtype=torch.float16, device="cuda")
    ops.conv(h, None, Geom.linear(m), pf, f, ln_part=rs)
    ops.synchronize()
    hid, gate = F.linear(ln, wf.float(), bf.float()).chunk(2, dim=-1)
    check(f, hid * F.gelu(gate), "ln(large mean)->geglu", rel=5e-3)


def test_qkv_transposed_output_and_dual_output(ops):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_linear_cat

    s, c = 300, 128
    x = rnd(s, c, seed=1)
    wq, wk, wv = (rnd(c, c, seed=i, scale=c ** -0.5) for i in (2, 3, 4))
    pw = pack_linear_cat([wq, wk, wv])
    pw.weight = pw.weight.cuda()
    ldt = (s + 63) // 64 * 64
    qk = torch.zeros(s, 2 * c, dtype=torch.float16, device="cuda")
    vt = torch.zeros(c, ldt, dtype=torch.float16, device="cuda")
    for split in (1, 2):
        qk.zero_()
        vt.zero_()
        ops.conv(x.cuda(), None, Geom.linear(s), pw, qk, ldo=2 * c, out_t=vt, ldt=ldt, t_col0=2 * c, split_k=split, tile=2)
        ops.synchronize()
        check(qk[:, :c], F.linear(x.float(), wq.float()), "q")
        check(qk[:, c:], F.linear(x.float(), wk.float()), "k")
        check(vt[:, :s], F.linear(x.float(), wv.float()).t(), "v^T")
        assert (vt[:, s:] == 0).all()
    # dual output: out2 = out + add2
    pwq = pack_linear_cat([wq])
    pwq.weight = pwq.weight.cuda()
    o1 = torch.zeros(s, c, dtype=torch.float16, device="cuda")
    o2 = torch.zeros(s, c, dtype=torch.float16, device="cuda")
    add = rnd(s, c, seed=9)
    ops.conv(x.cuda(), None, Geom.linear(s), pwq, o1, out2=o2, add2=add.cuda())
    ops.synchronize()
    ref = F.linear(x.float(), wq.float())
    check(o1, ref, "out")
    check(o2, ref + add.float(), "out2")


@pytest.mark.parametrize("c0,c1,hw,silu,eps", [(320, 0, 4096, True, 1e-5), (1280, 640, 256, True, 1e-5),
                                                (2560, 0, 64, False, 1e-6), (64, 0, 100, True, 1e-5),
                                                (128, 64, 35, False, 1e-5), (640, 320, 1024, True, 1e-5),
                                                # one-launch form (hw <= 1024, 8- or 16-byte aligned groups)
                                                (640, 0, 1024, True, 1e-5), (1280, 0, 256, True, 1e-5), (1280, 1280, 70, True, 1e-5),
                                                (128, 0, 1000, False, 1e-6), (256, 128, 300, True, 1e-5), (1280, 0, 1, True, 1e-5)])
def test_groupnorm(ops, c0, c1, hw, silu, eps):
    c = c0 + c1
    a = rnd(hw, c0, seed=1) * 2 + 0.5
    b = rnd(hw, c1, seed=2) if c1 else None
    gamma, beta = (1 + 0.1 * rnd(c, seed=3).float()).half(), rnd(c, seed=4, scale=0.1)
    out = torch.zeros(hw, c, dtype=torch.float16, device="cuda")
    ops.groupnorm(a.cuda(), None if b is None else b.cuda(), c0, c1, hw, 32, eps, gamma.cuda(), beta.cuda(), silu, out)
    ops.synchronize()
    x = a.float() if b is None else torch.cat([a.float(), b.float()], dim=1)
    ref = F.group_norm(x.t()[None], 32, gamma.float(), beta.float(), eps)[0].t()
    if silu:
        ref = F.silu(ref)
    check(out, ref, f"groupnorm C={c} hw={hw}")


@pytest.mark.parametrize("h,w,c0,c1,cout,tile,split", [(16, 16, 128, 64, 192, 2, 1), (18, 14, 64, 0, 320, 1, 3),
                                                        (64, 64, 64, 0, 64, 0, 1), (8, 8, 640, 640, 1280, 2, 4)])
def test_conv_channel_statistics_output(ops, h, w, c0, c1, cout, tile, split):
    """conv epilogue leaves per-channel (sum, sumsq) of its output (chanstat_out: the reference-only mode's AdaIN statistics)."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    hw = h * w
    xs = [rnd(1, c0, h, w, seed=1)] + ([rnd(1, c1, h, w, seed=2)] if c1 else [])
    cin = c0 + c1
    wt = rnd(cout, cin, 3, 3, seed=3, scale=(cin * 9) ** -0.5)
    b = rnd(cout, seed=4, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, b))
    srcs = [to_nhwc(x).cuda() for x in xs]
    out = torch.zeros(hw, cout, dtype=torch.float16, device="cuda")
    cs = torch.zeros(cout, 2, dtype=torch.float32, device="cuda")
    for rep in range(2):  # twice: the arrival counters must come back to zero
        ops.conv(srcs[0], srcs[1] if c1 else None, Geom.conv(h, w), pw, out, c0=c0, c1=c1, tile=tile, split_k=split,
                 chanstat_out=cs)
        ops.synchronize()
        o = out.float().cpu()
        assert torch.allclose(cs[:, 0].cpu(), o.sum(dim=0), rtol=1e-4, atol=2e-2), rep
        assert torch.allclose(cs[:, 1].cpu(), (o * o).sum(dim=0), rtol=1e-4, atol=2e-2), rep
    assert int(ops._chan_counters[0].abs().sum()) == 0


@pytest.mark.parametrize("rows,c", [(4096, 320), (77, 768), (5, 1280), (1000, 64), (64, 1536)])
def test_layernorm(ops, rows, c):
    x = rnd(rows, c, seed=1) * 3 + 1
    gamma, beta = (1 + 0.1 * rnd(c, seed=3).float()).half(), rnd(c, seed=4, scale=0.1)
    out = torch.zeros(rows, c, dtype=torch.float16, device="cuda")
    ops.layernorm(x.cuda(), rows, c, gamma.cuda(), beta.cuda(), 1e-5, out)
    ops.synchronize()
    check(out, F.layer_norm(x.float(), (c,), gamma.float(), beta.float(), 1e-5), f"layernorm {rows}x{c}")


def attention_ref(q, k, v, heads, scale, causal=False):
    sq, c = q.shape
    sk = k.shape[0]
    d = c // heads
    qh = q.float().view(sq, heads, d).transpose(0, 1)
    kh = k.float().view(sk, heads, d).transpose(0, 1)
    vh = v.float().view(sk, heads, d).transpose(0, 1)
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        s = s + torch.full((sq, sk), float("-inf")).triu(1)
    return (torch.softmax(s, dim=-1) @ vh).transpose(0, 1).reshape(sq, c)


@pytest.mark.parametrize("sq,sk,heads,d,causal", [
    (4096, 4096, 8, 40, False), (1024, 1024, 8, 80, False), (256, 256, 8, 160, False), (64, 64, 8, 160, False),
    (4096, 77, 8, 40, False), (1024, 77, 8, 80, False), (77, 77, 12, 64, True), (130, 200, 2, 8, False),
    (100, 100, 3, 16, False), (1296, 1296, 4, 32, False), (300, 77, 2, 64, False), (60, 200, 2, 128, True)])
def test_attention(ops, sq, sk, heads, d, causal):
    c = heads * d
    q, k, v = rnd(sq, c, seed=1), rnd(sk, c, seed=2), rnd(sk, c, seed=3)
    # one spiky key so that the online-softmax rescale branch is exercised on a late tile
    if sk > 70:
        k[sk - 3] *= 6.0
    ldvt = (sk + 63) // 64 * 64
    vt = torch.zeros(c, ldvt, dtype=torch.float16)
    vt[:, :sk] = v.t()
    out = torch.zeros(sq, c, dtype=torch.float16, device="cuda")
    scale = d ** -0.5
    ops.attention(q.cuda(), c, k.cuda(), c, vt.cuda(), ldvt, out, c, sq, sk, heads, d, scale, causal)
    ops.synchronize()
    check(out, attention_ref(q, k, v, heads, scale, causal), f"attention {sq}x{sk} h{heads} d{d}", rel=3e-3)


@pytest.mark.parametrize("sq,sk,heads,d", [(4096, 4096, 8, 40), (1024, 1024, 8, 80), (1024, 77, 8, 80)])
def test_attention_with_peaked_softmax_rows(ops, sq, sk, heads, d):
    """N(0, 1/sqrt(fan_in)) weights give near-uniform softmax rows.  Trained attention has logits with
    a dynamic range of 10-30: a few keys take almost all the mass, the running maximum is raised many times along the
    key loop and most probabilities underflow to 0 in fp16.  Logit spread here: std ~6, |s| up to ~30."""
    c = heads * d
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(sq, c, generator=g) * 2.5).half()
    k = (torch.randn(sk, c, generator=g) * 2.5).half()
    v = torch.randn(sk, c, generator=g).half()
    ldvt = (sk + 63) // 64 * 64
    vt = torch.zeros(c, ldvt, dtype=torch.float16)
    vt[:, :sk] = v.t()
    out = torch.zeros(sq, c, dtype=torch.float16, device="cuda")
    scale = d ** -0.5
    s0 = (q[:, :d].float() @ k[:, :d].float().t()) * scale
    assert 4.0 < float(s0.std()) < 9.0 and float(s0.abs().max()) > 20.0
    ops.attention(q.cuda(), c, k.cuda(), c, vt.cuda(), ldvt, out, c, sq, sk, heads, d, scale, False)
    ops.synchronize()
    check(out, attention_ref(q, k, v, heads, scale), f"peaked attention {sq}x{sk} d{d}", rel=4e-3)


@pytest.mark.parametrize("m,c,heads", [(768, 1280, 8), (3072, 640, 8), (200, 640, 8), (1, 1280, 8)])  # (1 row: an 8 x 8 frame's latent)
def test_absorbed_cross_attention_matches_explicit_attention(ops, m, c, heads):
    """Cross-attention over the 77 text tokens as two GEMMs (packing.pack_cross_attention: K folded into the query
    weights, V into the output weights, per-head tile softmax in the first GEMM's epilogue) against the explicit
    LayerNorm -> to_q -> softmax(q K^T / sqrt(d)) V -> to_out + residual in fp32."""
    from videosd_amd import lib as L
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_cross_attention, pack_linear

    tl, d = 77, c // heads
    x = (rnd(m, c, seed=1).float() * 2 + 0.3).half()
    text_k, text_v = rnd(tl, c, seed=2, scale=1.5), rnd(tl, c, seed=3)
    wq, wo, bo = rnd(c, c, seed=4, scale=c ** -0.5), rnd(c, c, seed=5, scale=c ** -0.5), rnd(c, seed=6, scale=0.1)
    gamma, beta = (1 + 0.1 * rnd(c, seed=7).float()).half(), rnd(c, seed=8, scale=0.1)
    # producer: identity GEMM that leaves the rows and their LayerNorm partials
    p0 = ops.to_device_pack(pack_linear(torch.eye(c).half(), None))
    h = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    rs = torch.zeros(m, c // 64, 2, dtype=torch.float32, device="cuda")
    ops.conv(x.cuda(), None, Geom.linear(m), p0, h, rowstat_out=rs, tile=2)
    xa1, xa2 = pack_cross_attention(text_k.float(), text_v.float(), wq, wo, bo, gamma, beta, heads)
    xa1, xa2 = ops.to_device_pack(xa1), ops.to_device_pack(xa2)
    pr = torch.zeros(m, heads * 128, dtype=torch.float16, device="cuda")
    out = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    for tile, split in ((0, 1), (3, 1), (3, 4), (0, 2)):
        ops.conv(h, None, Geom.linear(m), xa1, pr, ln_part=rs, act=L.ACT_SOFTMAX, softmax_cols=tl, tile=tile, split_k=split)
        ops.conv(pr, None, Geom.linear(m), xa2, out, residual=h)
        ops.synchronize()
        xf = x.float()
        ln = F.layer_norm(xf, (c,), gamma.float(), beta.float(), 1e-5)
        q = F.linear(ln, wq.float()).view(m, heads, d).transpose(0, 1)
        kk = text_k.float().view(tl, heads, d).transpose(0, 1)
        vv = text_v.float().view(tl, heads, d).transpose(0, 1)
        att = torch.softmax(q @ kk.transpose(-1, -2) * d ** -0.5, dim=-1)
        prob = pr.float().cpu().view(m, heads, 128)
        assert float(prob[:, :, tl:].abs().max()) == 0.0 and torch.allclose(prob[:, :, :tl].sum(-1), torch.ones(m, heads), atol=4e-3)
        check(prob[:, :, :tl].transpose(0, 1), att, f"probabilities tile={tile}", rel=6e-3)
        ref = F.linear((att @ vv).transpose(0, 1).reshape(m, c), wo.float(), bo.float()) + xf
        check(out, ref, f"absorbed cross-attention tile={tile}", rel=3e-3)
    with pytest.raises(RuntimeError, match="softmax"):
        ops.conv(h, None, Geom.linear(m), xa1, pr, ln_part=rs, act=L.ACT_SOFTMAX, softmax_cols=tl, tile=1, split_k=1)


@pytest.mark.parametrize("c,heads,tl", [(640, 8, 77), (1280, 8, 77), (1280, 20, 77), (128, 8, 50), (640, 10, 128)])
def test_xattn_fold_on_the_gpu_matches_the_host_packing(ops, c, heads, tl):
    """vsd_xattn_fold (csrc/prompt_fold.hip: a prompt's K / V folded into the query / output weights of an absorbed
    cross-attention block, per prompt, on the GPU) against packing.pack_cross_attention (fp32 on the host, what round 2 ran per
    prompt change): weights to fp16 rounding, ln_s / ln_t to fp32 summation order, zero rows / columns beyond the text length."""
    from videosd_amd.packing import pack_cross_attention

    ldt = (tl + 63) // 64 * 64
    k, v = rnd(tl, c, seed=2, scale=1.5), rnd(tl, c, seed=3)
    wq, wo, bo = rnd(c, c, seed=4, scale=c ** -0.5), rnd(c, c, seed=5, scale=c ** -0.5), rnd(c, seed=6, scale=0.1)
    gamma, beta = (1 + 0.1 * rnd(c, seed=7).float()).half(), rnd(c, seed=8, scale=0.1)
    x1, x2 = pack_cross_attention(k.float(), v.float(), wq, wo, bo, gamma, beta, heads)
    vt = torch.zeros(c, ldt, dtype=torch.float16)
    vt[:, :tl] = v.t()
    hg = heads * 128
    dev = lambda t: t.cuda().contiguous()  # noqa: E731
    w1 = torch.full((hg, c), 7.0, dtype=torch.float16, device="cuda")   # poisoned: every element must be written
    s1, t1 = torch.full((hg,), 7.0, device="cuda"), torch.full((hg,), 7.0, device="cuda")
    w2 = torch.full((c, hg), 7.0, dtype=torch.float16, device="cuda")
    ops.xattn_fold(dev(k), dev(vt), tl, dev(wq), dev(wo), dev(gamma), dev(beta), c, heads, (c // heads) ** -0.5, w1, s1, t1, w2)
    ops.synchronize()
    check(w1, x1.weight[:, :c], "xa1 weights", rel=2e-3)
    check(w2, x2.weight[:, :hg], "xa2 weights", rel=2e-3)
    assert float((s1.cpu() - x1.ln_s).abs().max()) <= 2e-3 * float(x1.ln_s.abs().max()) + 1e-4
    assert float((t1.cpu() - x1.ln_t).abs().max()) <= 1e-4 * float(x1.ln_t.abs().max()) + 1e-5
    if tl < 128:
        g = w1.cpu().view(heads, 128, c)
        assert float(g[:, tl:].abs().max()) == 0.0 and float(w2.cpu().view(c, heads, 128)[:, :, tl:].abs().max()) == 0.0
        assert float(s1.cpu().view(heads, 128)[:, tl:].abs().max()) == 0.0 and float(t1.cpu().view(heads, 128)[:, tl:].abs().max()) == 0.0


def _tail_weights(c=320, seed=0):
    from videosd_amd.packing import pack_conv, pack_geglu_ln, pack_linear, pack_linear_ln

    g = torch.Generator().manual_seed(seed)
    r = lambda *s_, sc=1.0: (torch.randn(*s_, generator=g) * sc).half()  # noqa: E731
    w = dict(wo1=r(c, c, sc=c ** -0.5), bo1=r(c, sc=0.1), wq=r(c, c, sc=c ** -0.5), g2=(1 + 0.1 * r(c).float()).half(), be2=r(c, sc=0.1),
             wo2=r(c, c, sc=c ** -0.5), bo2=r(c, sc=0.1), g3=(1 + 0.1 * r(c).float()).half(), be3=r(c, sc=0.1),
             wf1=r(8 * c, c, sc=c ** -0.5), bf1=r(8 * c, sc=0.1), wf2=r(c, 4 * c, sc=(4 * c) ** -0.5), bf2=r(c, sc=0.1),
             wp=r(c, c, 1, 1, sc=c ** -0.5), bp=r(c, sc=0.1))
    from videosd_amd.packing import add_frag

    packs = dict(out1=pack_linear(w["wo1"], w["bo1"]), q2=pack_linear_ln([w["wq"]], None, w["g2"], w["be2"]),
                 out2=pack_linear(w["wo2"], w["bo2"]), ff1=pack_geglu_ln(w["wf1"], w["bf1"], w["g3"], w["be3"]),
                 ff2=pack_linear(w["wf2"], w["bf2"]), proj=pack_conv(w["wp"], w["bp"]))
    return w, {k: add_frag(v) for k, v in packs.items()}


@pytest.mark.parametrize("m", [12288, 4096, 200, 64, 20480, 17000, 8000, 12000, 16384])
def test_fused_transformer_tail_matches_the_unfused_chain(ops, m):
    """csrc/fused_tail.hip against explicit fp32 torch: tail_a = out-projection + residual, LayerNorm, query projection;
    tail_b = out-projection + residual, LayerNorm, GEGLU feed-forward + residual, proj_out + residual.  m = 200 has a ragged
    last tile.  The library picks the tile height per token count (16 / 32 / 48 / 64 / 80 rows: the cheapest rounds of
    <= 256 workgroups): 64, 200, 4096 -> 16; 8000 -> 32; 12000, 12288 -> 48; 16384 -> 64; 17000, 20480 -> 80; 200, 8000,
    12000 and 17000 end in a ragged tile."""
    c = 320
    w, packs = _tail_weights(c)
    pk = {k: ops.to_device_pack(v) for k, v in packs.items()}
    att, h, x = rnd(m, c, seed=1), (rnd(m, c, seed=2).float() * 2 + 0.5).half(), rnd(m, c, seed=3)
    h1 = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    q = torch.zeros_like(h1)
    ops.tail_a(att.cuda(), h.cuda(), m, pk["out1"], pk["q2"], h1, q)
    ops.synchronize()
    h1_ref = F.linear(att.float(), w["wo1"].float(), w["bo1"].float()) + h.float()
    check(h1, h1_ref, "tail_a h1")
    q_ref = F.linear(F.layer_norm(h1.float().cpu(), (c,), w["g2"].float(), w["be2"].float(), 1e-5), w["wq"].float())
    check(q, q_ref, "tail_a q", rel=3e-3)
    att2 = rnd(m, c, seed=4)
    out = torch.zeros_like(h1)
    ops.tail_b(att2.cuda(), h1, x.cuda(), m, pk["out2"], pk["ff1"], pk["ff2"], pk["proj"], out)
    ops.synchronize()
    h2 = F.linear(att2.float(), w["wo2"].float(), w["bo2"].float()) + h1.float().cpu()
    ln = F.layer_norm(h2.half().float(), (c,), w["g3"].float(), w["be3"].float(), 1e-5)
    hid, gate = F.linear(ln, w["wf1"].float(), w["bf1"].float()).chunk(2, dim=-1)
    h3 = F.linear(hid * F.gelu(gate), w["wf2"].float(), w["bf2"].float()) + h2
    ref = F.linear(h3, w["wp"].float().reshape(c, c), w["bp"].float()) + x.float()
    check(out, ref, "tail_b out", rel=3e-3)
    # deterministic, and nothing written past row m
    out2 = torch.full((m + 64, c), 7.0, dtype=torch.float16, device="cuda")
    ops.tail_b(att2.cuda(), h1, x.cuda(), m, pk["out2"], pk["ff1"], pk["ff2"], pk["proj"], out2)
    ops.synchronize()
    assert torch.equal(out2[:m], out) and bool((out2[m:] == 7.0).all())


def test_preprocess_and_postprocess(ops):
    h, w = 40, 56
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = torch.zeros(h * w, 8, dtype=torch.float16, device="cuda")
    ops.preprocess_rgb(torch.from_numpy(img).cuda(), h, w, out)
    ops.synchronize()
    # (to the bit: the chain of fp16 roundings the kernel's comments promise, tests/exact_cases.py; every byte value: tests/test_exact_gpu.py)
    assert np.array_equal(out[:, :3].cpu().numpy(), X.preprocess_chain(img.reshape(h * w, 3)))
    assert (out[:, 3:] == 0).all()
    # postprocess: decoder value c -> u8
    cvals = torch.linspace(-0.2, 1.2, h * w * 3).reshape(h * w, 3)
    dec = torch.zeros(h * w, 8, dtype=torch.float16)
    dec[:, :3] = cvals.half()
    u8 = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    ops.postprocess_rgb(dec.cuda(), 8, h * w, u8)
    ops.synchronize()
    assert np.array_equal(u8.cpu().numpy(), X.postprocess_chain(dec[:, :3].numpy()).reshape(-1))   # (every byte, not +-1)


def test_sobel_control_matches_oracle(ops):
    from PIL import Image

    from oracle.pipeline import sobel_edges

    h, w = 48, 64
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = ((xx * 4 + yy * 2) % 256).astype(np.uint8)[..., None]
    img = (base // 2 + grad // 2).astype(np.uint8)
    ref = np.asarray(sobel_edges(Image.fromarray(img, "RGB"), 0.11, 0.8))
    edge = torch.zeros(h * w, dtype=torch.uint8, device="cuda")
    ctrl = torch.zeros(h * w, 8, dtype=torch.float16, device="cuda")
    ops.sobel_control(torch.from_numpy(img).cuda(), h, w, 0.11, 0.8, edge, ctrl)
    ops.synchronize()
    got = edge.cpu().numpy().reshape(h, w)
    diff = np.abs(got.astype(int) - ref.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.01, (diff.max(), (diff > 0).mean())
    check(ctrl[:, 0], torch.from_numpy(got.reshape(-1).astype(np.float32) / 255.0), "control", atol_scale=2.0 ** -10)
    assert (ctrl[:, 0] == ctrl[:, 2]).all() and (ctrl[:, 3:] == 0).all()


@pytest.mark.parametrize("h,w,skew", [(8, 8, 0), (24, 40, 0), (16, 264, 0), (40, 520, 0), (24, 40, 3), (16, 264, 7), (9, 257, 1)])
def test_sobel_control_ragged_and_unaligned(ops, h, w, skew):
    """Row tiles of 256 pixels with 16-byte aligned loads: widths that are not a multiple of the tile, tiles that end
    inside a 16-byte piece, one-pixel-wide last tiles, and a frame that does not start on a 16-byte boundary."""
    from PIL import Image

    from oracle.pipeline import sobel_edges

    rng = np.random.default_rng(h * 1000 + w + skew)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = np.asarray(sobel_edges(Image.fromarray(img, "RGB"), 0.11, 0.8))
    holder = torch.full((skew + h * w * 3 + 64,), 255, dtype=torch.uint8, device="cuda")  # 255s around: leaks would show
    frame = holder[skew:skew + h * w * 3]
    frame.copy_(torch.from_numpy(img).reshape(-1))
    edge = torch.zeros(h * w, dtype=torch.uint8, device="cuda")
    ctrl = torch.zeros(h * w, 8, dtype=torch.float16, device="cuda")
    ops.sobel_control(frame, h, w, 0.11, 0.8, edge, ctrl)
    ops.synchronize()
    got = edge.cpu().numpy().reshape(h, w)
    diff = np.abs(got.astype(int) - ref.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.01, (diff.max(), (diff > 0).mean())
    assert torch.equal(ctrl[:, 0].float().cpu(), torch.from_numpy(got.reshape(-1).astype(np.float32) / 255.0).half().float())


def test_scheduler_kernels_match_oracle(ops):
    from oracle.scheduler import LCMSchedulerOracle
    from videosd_amd.lcm import LCMSchedule

    hw = 24 * 20
    sch = LCMSchedulerOracle()
    ts = sch.set_timesteps(0.6, 4)
    plan = LCMSchedule(0.6, 4)
    assert plan.timesteps == ts.tolist()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(1, 4, 24, 20, generator=g).half()
    noise = torch.randn(1, 4, 24, 20, generator=g)
    x0p = F.pad(to_nhwc(x0), (0, 4)).cuda()
    lat = torch.zeros(hw, 8, dtype=torch.float16, device="cuda")
    sa, sb = plan.add_noise_coef()
    ops.add_noise(x0p, noise.cuda(), sa, sb, hw, lat)
    ops.synchronize()
    ref = sch.add_noise(x0.float(), noise, ts[:1])
    check(lat[:, :4], to_nhwc(ref), "add_noise", atol_scale=2.0 ** -10)
    assert (lat[:, 4:] == 0).all()
    cur = ref
    for i, t in enumerate(ts):
        eps = torch.randn(1, 4, 24, 20, generator=g).half()
        torch.manual_seed(100 + i)
        prev_ref, den_ref = sch.step(eps.float(), i, t, cur.half().float())
        torch.manual_seed(100 + i)
        nz = torch.randn(1, 4, 24, 20)
        prev = torch.zeros(hw, 8, dtype=torch.float16, device="cuda")
        den = torch.zeros(hw, 8, dtype=torch.float16, device="cuda")
        dec = torch.zeros(hw, 8, dtype=torch.float16, device="cuda")
        ops.lcm_step(F.pad(to_nhwc(eps), (0, 4)).cuda(), F.pad(to_nhwc(cur.half()), (0, 4)).cuda(), nz.cuda(),
                     plan.step_coef(i), hw, prev, den, dec)
        ops.synchronize()
        check(den[:, :4], to_nhwc(den_ref), f"denoised step {i}", atol_scale=2.0 ** -9)
        check(prev[:, :4], to_nhwc(prev_ref), f"prev step {i}", atol_scale=2.0 ** -9)
        check(dec[:, :4], to_nhwc(torch.tanh(den_ref / 3) * 3), f"dec_in step {i}", atol_scale=2.0 ** -9)
        cur = prev_ref


def test_graph_replay_equals_eager(ops):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    h, w, c = 16, 16, 64
    x = rnd(h * w, c, seed=1).cuda()
    pw = pack_conv(rnd(c, c, 3, 3, seed=2, scale=(9 * c) ** -0.5), rnd(c, seed=3, scale=0.1))
    pw.weight, pw.bias = pw.weight.cuda(), pw.bias.cuda()
    gamma, beta = torch.ones(c, dtype=torch.float16, device="cuda"), torch.zeros(c, dtype=torch.float16, device="cuda")
    t1, t2 = (torch.zeros(h * w, c, dtype=torch.float16, device="cuda") for _ in range(2))

    def body():
        ops.groupnorm(x, None, c, 0, h * w, 32, 1e-5, gamma, beta, True, t1)
        ops.conv(t1, None, Geom.conv(h, w), pw, t2, residual=x, split_k=2, tile=2)

    body()
    ops.synchronize()
    eager = t2.clone()
    t2.zero_()
    ops.workspace("splitk", 2 * h * w * c * 4)
    ops.graph_begin()
    body()
    g = ops.graph_end()
    for _ in range(3):
        t2.zero_()
        ops.graph_launch(g)
        ops.synchronize()
        assert torch.equal(t2, eager)
    ops.graph_destroy(g)


def test_launch_sequence_orders_graphs_on_two_streams_by_its_event_edges(ops):
    """include/vsd.h vsd_seq / vsd_stream_pool at the C-ABI level: a sequence of three single-branch graphs on two of the
    process's launch streams -- A on the lane's stream, B on its side stream AFTER A (edge), C on the lane's stream AFTER B
    (edge) -- must produce the dependent result every replay, and the four pool streams must be four different handles on
    four different command-processor pipes."""
    pool = ops.pool_streams()
    assert len({st.cuda_stream for st in pool}) == 4 and ops.streams[0].cuda_stream == pool[ops.lane % 4].cuda_stream
    assert ops.streams[1].cuda_stream == pool[(ops.lane + 2) % 4].cuda_stream
    assert ops.pool_check(chain=60) < 1.5
    n = 1 << 20
    a = torch.full((n,), 1.0, dtype=torch.float16, device="cuda")
    b = torch.full((n,), 2.0, dtype=torch.float16, device="cuda")
    x, y, z = (torch.zeros(n, dtype=torch.float16, device="cuda") for _ in range(3))
    ops.synchronize()
    seq = ops.seq_create()
    ops.seq_capture_begin(0)
    ops.axpy(a, b, 3.0, n, x)           # A: x = 1 + 2 * 3 = 7
    ops.seq_capture_end(seq, 0)
    ops.seq_wait(seq, 1, ops.seq_record(seq, 0))
    ops.seq_capture_begin(1)
    ops.axpy(x, b, 0.5, n, y)           # B (side stream): y = x + 2 * 0.5 = 8
    ops.seq_capture_end(seq, 1)
    ops.seq_wait(seq, 0, ops.seq_record(seq, 1))
    ops.seq_capture_begin(0)
    ops.axpy(y, x, 1.0, n, z)           # C: z = y + x = 15
    ops.seq_capture_end(seq, 0)
    ops.use_stream(0)
    assert ops.seq_count(seq) == (3, 2)
    for rep in range(5):
        for t in (x, y, z):
            ops.zero_(t)
        ops.seq_launch(seq)
        ops.synchronize()
        assert float(z.float().min()) == 15.0 and float(z.float().max()) == 15.0, rep
    ops.seq_destroy(seq)


def test_errors_are_reported_not_fatal(ops):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    pw = pack_conv(rnd(64, 64, 3, 3), None)
    pw.weight = pw.weight.cuda()
    x = rnd(16, 64).cuda()
    out = torch.zeros(16, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="concat|multiple|K="):
        ops.conv(x, x, Geom.conv(4, 4), pw, out, c0=40, c1=24)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attention(x, 64, x, 64, x, 64, out, 64, 16, 16, 1, 12, 1.0)
    # erf GELU lives in the general epilogue walk only; an activation the enum does not know is refused
    lin = pack_conv(rnd(64, 64, 1, 1), None)
    lin.weight = lin.weight.cuda()
    vt = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="GELU"):
        ops.conv(x, None, Geom.linear(16), lin, out, act=6, out_t=vt, ldt=64)
    with pytest.raises(RuntimeError, match="activation"):
        ops.conv(x, None, Geom.linear(16), lin, out, act=9)


# ---------------------------------------------------------------------------------------------- batched launches
@pytest.mark.parametrize("h,w,stride,up,c1,pipeline,tile,split", [(18, 14, 1, None, 0, 3, 2, 1), (18, 14, 1, None, 64, 0, 1, 3),
                                                                   (27, 48, 2, None, 0, 5, 0, 1), (7, 12, 1, (14, 24), 0, 4, 3, 2),
                                                                   (9, 9, 1, None, 0, 6, 2, 4)])
def test_conv_batched_images_keep_their_borders(ops, h, w, stride, up, c1, pipeline, tile, split):
    """vsd_conv_desc.batch: B images stacked along M; zero padding, stride, nearest resize and channel concat are per
    image (no bleeding across the image boundary)."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    B, c0, cout = 3, 128, 96
    cin = c0 + c1
    xs = rnd(B, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    bias = rnd(cout, seed=3, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, bias))
    g = Geom.conv(h, w, stride=stride, up_to=up, batch=B)
    nhwc = xs.permute(0, 2, 3, 1).reshape(B * h * w, cin)
    s0 = nhwc[:, :c0].contiguous().cuda()
    s1 = nhwc[:, c0:].contiguous().cuda() if c1 else None
    res = rnd(g.m, cout, seed=5)
    out = torch.zeros(g.m, cout, dtype=torch.float16, device="cuda")
    ops.conv(s0, s1, g, pw, out, c0=c0, c1=c1, residual=res.cuda(), act=2, tile=tile, split_k=split, pipeline=pipeline)
    ops.synchronize()
    xin = xs.float()
    if up is not None:
        xin = F.interpolate(xin, size=up, mode="nearest")
    ref = F.silu(F.conv2d(xin, wt.float(), bias.float(), stride=stride, padding=1))
    ref = ref.permute(0, 2, 3, 1).reshape(g.m, cout) + res.float()
    check(out, ref, f"batched conv {h}x{w} stride={stride} up={up}")


def test_qkv_batched_transposed_output_slabs(ops):
    """Transposed (V^T) output with batch: image b's tokens land in columns [b*t_img, b*t_img + hw), padding stays 0."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_linear_cat

    B, hw, c = 3, 84, 128  # 84 tokens (7x12 latent): not a multiple of 8
    t_img = 128
    x = rnd(B * hw, c, seed=1)
    wq, wk, wv = (rnd(c, c, seed=i, scale=c ** -0.5) for i in (2, 3, 4))
    pw = ops.to_device_pack(pack_linear_cat([wq, wk, wv]))
    qk = torch.zeros(B * hw, 2 * c, dtype=torch.float16, device="cuda")
    vt = torch.zeros(c, B * t_img, dtype=torch.float16, device="cuda")
    for split in (1, 2):
        vt.zero_()
        ops.conv(x.cuda(), None, Geom.linear(hw, batch=B), pw, qk, ldo=2 * c, out_t=vt, ldt=B * t_img, t_col0=2 * c,
                 t_img=t_img, split_k=split, tile=2)
        ops.synchronize()
        check(qk[:, :c], F.linear(x.float(), wq.float()), "q")
        v = F.linear(x.float(), wv.float())
        for b in range(B):
            check(vt[:, b * t_img: b * t_img + hw], v[b * hw:(b + 1) * hw].t(), f"v^T image {b}")
            assert (vt[:, b * t_img + hw:(b + 1) * t_img] == 0).all()


@pytest.mark.parametrize("c0,c1,hw,silu", [(320, 0, 1024, True), (128, 64, 35, False), (1280, 1280, 64, True),
                                           # several groups per workgroup (80-byte row pieces): 2 x 20 channels, also over a concat whose
                                           # boundary falls between two pieces, a ragged row count, and 4 x 10 channels at 16 x 16
                                           (640, 0, 1024, True), (320, 320, 1024, False), (640, 0, 1000, True), (320, 0, 256, True)])
def test_groupnorm_batched(ops, c0, c1, hw, silu):
    B, c = 3, c0 + c1
    a = rnd(B * hw, c0, seed=1) * torch.tensor([1.0, 3.0, 0.3]).repeat_interleave(hw)[:, None].half() + 0.5
    b = rnd(B * hw, c1, seed=2) if c1 else None
    gamma, beta = (1 + 0.1 * rnd(c, seed=3).float()).half(), rnd(c, seed=4, scale=0.1)
    out = torch.zeros(B * hw, c, dtype=torch.float16, device="cuda")
    ops.groupnorm(a.cuda(), None if b is None else b.cuda(), c0, c1, hw, 32, 1e-5, gamma.cuda(), beta.cuda(), silu, out, batch=B)
    ops.synchronize()
    x = a.float() if b is None else torch.cat([a.float(), b.float()], dim=1)
    ref = F.group_norm(x.reshape(B, hw, c).transpose(1, 2), 32, gamma.float(), beta.float(), 1e-5).transpose(1, 2).reshape(B * hw, c)
    if silu:
        ref = F.silu(ref)
    check(out, ref, f"batched groupnorm C={c} hw={hw}")


@pytest.mark.parametrize("sq,heads,d", [(84, 8, 40), (256, 4, 64), (1024, 8, 80)])
def test_attention_batched_self(ops, sq, heads, d):
    """Self-attention of B images in one launch: keys never cross an image boundary."""
    B, c = 3, heads * d
    t_img = (sq + 63) // 64 * 64
    q, k, v = rnd(B * sq, c, seed=1), rnd(B * sq, c, seed=2), rnd(B * sq, c, seed=3)
    vt = torch.zeros(c, B * t_img, dtype=torch.float16)
    for b in range(B):
        vt[:, b * t_img: b * t_img + sq] = v[b * sq:(b + 1) * sq].t()
    out = torch.zeros(B * sq, c, dtype=torch.float16, device="cuda")
    ops.attention(q.cuda(), c, k.cuda(), c, vt.cuda(), B * t_img, out, c, sq, sq, heads, d, d ** -0.5, batch=B, k_brows=sq,
                  vt_bcols=t_img)
    ops.synchronize()
    sp = lambda t: t.float().reshape(B, sq, heads, d).transpose(1, 2)  # noqa: E731
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(B * sq, c)
    check(out, ref, f"batched attention sq={sq} d={d}", rel=3e-3)


@pytest.mark.parametrize("pipeline,split_k", [(3, 1), (5, 1), (3, 3), (5, 2)])
def test_conv_256x128_tile(ops, pipeline, split_k):
    """VSD_TILE_256x128 (buffer-load path): ragged M and N, concat sources, fused epilogue, split-K."""
    h, w, c0, c1, cout = 30, 22, 128, 64, 200  # M = 660 (2.6 tiles), N = 200 (1.6 tiles)
    a, b = rnd(1, c0, h, w, seed=1), rnd(1, c1, h, w, seed=2)
    wt = rnd(cout, c0 + c1, 3, 3, seed=3, scale=((c0 + c1) * 9) ** -0.5)
    res = rnd(h * w, cout, seed=5)
    got, ref = run_conv(ops, [a, b], h, w, wt, rnd(cout, seed=4, scale=0.1), ksize=3, tile=4, split_k=split_k, pipeline=pipeline,
                        residual=res, act=2)
    check(got, ref, f"256x128 tile pipeline={pipeline} split={split_k}")
    x = rnd(1, 320, 1, 700, seed=7)
    wl = rnd(384, 320, 1, 1, seed=8, scale=320 ** -0.5)
    got, ref = run_conv(ops, [x], 1, 700, wl, None, ksize=1, tile=4, split_k=1, pipeline=pipeline)
    check(got, ref, "256x128 tile linear")


@pytest.mark.parametrize("h,w,c0,c1,cout,tile,split,act", [(16, 16, 128, 0, 192, 1, 1, 0), (8, 32, 64, 64, 200, 0, 1, 2),
                                                            (24, 16, 320, 0, 320, 1, 3, 0), (16, 32, 128, 64, 64, 1, 2, 1),
                                                            (64, 64, 64, 0, 64, 1, 1, 1 | 256),
                                                            # patches hanging over the image edge (27x48, 7x12, 8x8 latents)
                                                            (27, 48, 128, 0, 128, 1, 1, 2), (7, 12, 128, 128, 72, 1, 2, 0),
                                                            (8, 8, 1280, 0, 128, 0, 5, 0),
                                                            # 16x16 patches, 8 waves (tiles 256x128 = 4, 256x64 = 5)
                                                            (32, 32, 128, 0, 192, 4, 1, 2), (16, 48, 64, 64, 200, 5, 1, 0),
                                                            (27, 48, 128, 0, 128, 5, 2, 1), (64, 64, 64, 0, 64, 5, 1, 1 | 256)])
def test_conv3x3_halo_patch(ops, h, w, c0, c1, cout, tile, split, act):
    """pipeline 7: the (8+2)x(16+2) input patch of each 64-channel block staged in LDS once for all nine taps; image
    borders (zero padding) at every patch edge, concat sources, split-K over channel blocks, fused epilogue."""
    xs = [rnd(1, c0, h, w, seed=1)] + ([rnd(1, c1, h, w, seed=2)] if c1 else [])
    cin = c0 + c1
    wt = rnd(cout, cin, 3, 3, seed=3, scale=(cin * 9) ** -0.5)
    res = rnd(h * w, cout, seed=5)
    rv = rnd(cout, seed=6, scale=0.1)
    if act & 256:  # ReLU after the residual (TAESD block)
        got, ref = run_conv(ops, xs, h, w, wt, rnd(cout, seed=4, scale=0.1), ksize=3, tile=tile, split_k=split, pipeline=7, residual=res)
        # run_conv's reference has no post-activation: apply it to a second run with act given through the ops call
        from videosd_amd.ops import Geom
        from videosd_amd.packing import pack_conv

        pw = ops.to_device_pack(pack_conv(wt, rnd(cout, seed=4, scale=0.1)))
        out = torch.zeros(h * w, cout, dtype=torch.float16, device="cuda")
        ops.conv(to_nhwc(xs[0]).cuda(), None, Geom.conv(h, w), pw, out, residual=res.cuda(), act=act, tile=tile, split_k=split, pipeline=7)
        ops.synchronize()
        check(got, ref, "halo conv + residual")
        check(out, F.relu(ref), "halo conv + residual + post-ReLU")
        return
    got, ref = run_conv(ops, xs, h, w, wt, rnd(cout, seed=4, scale=0.1), ksize=3, tile=tile, split_k=split, pipeline=7, residual=res,
                        rowvec=rv, act=act)
    check(got, ref, f"halo conv {h}x{w} {cin}->{cout} tile={tile} split={split}")
    if split > 1:  # the in-launch reduction (default) and the reducer kernel sum the slabs in the same order: same bits
        ops.inkernel_splitk = False
        try:
            two, _ = run_conv(ops, xs, h, w, wt, rnd(cout, seed=4, scale=0.1), ksize=3, tile=tile, split_k=split, pipeline=7,
                              residual=res, rowvec=rv, act=act)
        finally:
            ops.inkernel_splitk = True
        assert torch.equal(got, two)
        assert int(ops._counters[0].abs().sum()) == 0


@pytest.mark.parametrize("B,hs,ws,up,act,res", [(1, 64, 64, None, 1, False), (1, 64, 64, None, 1 | 256, True), (3, 32, 48, None, 0, True),
                                                 (2, 27, 45, None, 2, False), (1, 16, 16, (32, 32), 0, False), (2, 14, 24, (27, 48), 1, False),
                                                 (5, 128, 128, None, 1 | 256, True), (1, 7, 5, None, 1, True)])
def test_persistent_64_channel_conv_matches_fp32_and_the_halo_forms_bits(ops, B, hs, ws, up, act, res):
    """pipeline 10 (csrc/conv_c64.hip): every conv of a TAESD block (3x3, 64 -> 64 channels; lcm_controlnet.py:299, 594) as one
    persistent launch -- weights resident, 16x16-pixel patches through two LDS buffers, register epilogue.  Against fp32 torch at the
    plain tolerances and bit for bit against the halo-patch form (same sums in the same order); patches hanging over the image edge,
    several images per launch (a workgroup walks from one image into the next), the folded 2x nearest upsample of the decoder,
    bias / ReLU / SiLU / residual / ReLU after the residual, more patches than workgroups (5 x 128 x 128: 320 patches on 256 CUs)."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    c = 64
    xs = rnd(B, c, hs, ws, seed=1)
    wt = rnd(c, c, 3, 3, seed=2, scale=(c * 9) ** -0.5)
    bias = rnd(c, seed=3, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, bias))
    g = Geom.conv(hs, ws, up_to=up, batch=B)
    x = xs.permute(0, 2, 3, 1).reshape(B * hs * ws, c).contiguous().cuda()
    r = rnd(g.m, c, seed=5) if res else None
    outs = []
    for pipeline in (10, 7):
        out = torch.full((g.m + 16, c), 7.0, dtype=torch.float16, device="cuda")  # (rows past M: must stay as they are)
        ops.conv(x, None, g, pw, out[:g.m], residual=None if r is None else r.cuda(), act=act, tile=5, split_k=1, pipeline=pipeline)
        ops.synchronize()
        assert bool((out[g.m:] == 7.0).all())
        outs.append(out[:g.m].cpu())
    xin = xs.float() if up is None else F.interpolate(xs.float(), size=up, mode="nearest")
    ref = F.conv2d(xin, wt.float(), bias.float(), padding=1)
    if (act & 255) == 1 and not act & 256:
        ref = F.relu(ref)
    if (act & 255) == 2:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 3, 1).reshape(g.m, c)
    if res:
        ref = ref + r.float()
    if act & 256:
        ref = F.relu(ref)
    check(outs[0], ref, f"persistent 64-channel conv B={B} {hs}x{ws} up={up} act={act}")
    assert torch.equal(outs[0], outs[1]), "pipeline 10 differs from the halo-patch form"


@pytest.mark.parametrize("B,h,w,n,act,up", [(1, 64, 64, 3, 0, None), (2, 37, 50, 4, 0, None), (5, 128, 128, 3, 0, None), (1, 16, 24, 8, 1, (32, 48)),
                                            (1, 9, 9, 3, 2, None)])
def test_persistent_64_channel_conv_with_a_thin_output(ops, B, h, w, n, act, up):
    """pipeline 10's form for Cout <= 8 into 8-wide rows (TAESD's last decoder conv 64 -> 3 at full image size, the encoder's 64 -> 4
    projection): against fp32 torch and bit for bit against the GEMM-form tile on the real channels; the padding channels of a row are
    written as zeros, rows past M stay untouched."""
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    c = 64
    xs = rnd(B, c, h, w, seed=1)
    wt = rnd(n, c, 3, 3, seed=2, scale=(c * 9) ** -0.5)
    bias = rnd(n, seed=3, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, bias))
    g = Geom.conv(h, w, up_to=up, batch=B)
    x = xs.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous().cuda()
    outs = []
    for tile, pipeline in ((5, 10), (2, 3)):
        out = torch.full((g.m + 16, 8), 7.0, dtype=torch.float16, device="cuda")
        ops.conv(x, None, g, pw, out[:g.m], ldo=8, act=act, tile=tile, split_k=1, pipeline=pipeline)
        ops.synchronize()
        assert bool((out[g.m:] == 7.0).all())
        outs.append(out[:g.m].cpu())
    assert bool((outs[0][:, n:] == 0).all())
    xin = xs.float() if up is None else F.interpolate(xs.float(), size=up, mode="nearest")
    ref = F.conv2d(xin, wt.float(), bias.float(), padding=1)
    ref = F.relu(ref) if act == 1 else (F.silu(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1).reshape(g.m, n)
    check(outs[0][:, :n], ref, f"thin persistent conv B={B} {h}x{w} n={n} act={act} up={up}")
    assert torch.equal(outs[0][:, :n], outs[1][:, :n]), "pipeline 10 (thin) differs from the GEMM-form tile"


def test_persistent_64_channel_form_is_refused_for_other_layers(ops):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    pw = ops.to_device_pack(pack_conv(rnd(128, 64, 3, 3, seed=1, scale=0.05), rnd(128, seed=2)))
    x = rnd(256, 64, seed=3).cuda()
    out = torch.zeros(256, 128, dtype=torch.float16, device="cuda")
    # through HipOps the call falls back to the halo-patch form (the safety net for shared table entries) ...
    ops.conv(x, None, Geom.conv(16, 16), pw, out, tile=5, split_k=1, pipeline=10)
    ops.synchronize()
    # ... the C entry point itself refuses it
    d = ops.conv(x, None, Geom.conv(16, 16), pw, out, tile=5, split_k=1, pipeline=7, _desc_only=True)
    d.pipeline = 10
    with pytest.raises(RuntimeError, match="pipeline 10"):
        ops.ctx.call("vsd_conv_gemm", __import__("ctypes").byref(d), ops.s)


@pytest.mark.parametrize("hs,ws,up,tile,split", [(8, 8, (16, 16), 1, 1), (14, 24, (27, 48), 5, 2), (16, 16, (32, 32), 0, 1)])
def test_conv3x3_halo_patch_with_folded_upsample(ops, hs, ws, up, tile, split):
    cin, cout = 128, 64
    x = rnd(1, cin, hs, ws, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    got, ref = run_conv(ops, [x], hs, ws, wt, rnd(cout, seed=3, scale=0.1), ksize=3, up_to=up, tile=tile, split_k=split, pipeline=7)
    check(got, ref, f"halo conv with upsample {hs}x{ws}->{up}")


def test_conv3x3_halo_patch_batched(ops):
    from videosd_amd.ops import Geom
    from videosd_amd.packing import pack_conv

    B, h, w, cin, cout = 3, 16, 16, 128, 128
    xs = rnd(B, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5)
    bias = rnd(cout, seed=3, scale=0.1)
    pw = ops.to_device_pack(pack_conv(wt, bias))
    g = Geom.conv(h, w, batch=B)
    out = torch.zeros(g.m, cout, dtype=torch.float16, device="cuda")
    ops.conv(xs.permute(0, 2, 3, 1).reshape(B * h * w, cin).contiguous().cuda(), None, g, pw, out, act=2, tile=0, split_k=1, pipeline=7)
    ops.synchronize()
    ref = F.silu(F.conv2d(xs.float(), wt.float(), bias.float(), padding=1)).permute(0, 2, 3, 1).reshape(g.m, cout)
    check(out, ref, "batched halo conv")


@pytest.mark.parametrize("h,w,cin,cout,ks,tile,split,pipeline", [(32, 32, 128, 256, 3, 3, 1, 5), (32, 32, 128, 256, 3, 1, 2, 7),
                                                                  (16, 64, 256, 512, 1, 0, 1, 3), (64, 64, 64, 128, 3, 4, 1, 7),
                                                                  (16, 16, 512, 256, 3, 2, 4, 3)])
def test_every_workgroup_order_gives_the_same_bits(ops, h, w, cin, cout, ks, tile, split, pipeline):
    """block -> tile orders (csrc/conv_kernels.h block_to_tile): whole weight-tile groups per XCD, whole M tiles per XCD, the
    XCDs as a 2 x 4 / 4 x 2 grid -- placement only, never the result (VSD_CONV_ORDER forces one where the tile counts allow)."""
    import os

    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, ks, ks, seed=2, scale=(cin * ks * ks) ** -0.5)
    b = rnd(cout, seed=3, scale=0.1)
    outs = {}
    try:
        for order in ("0", "1", "2", "3", "1d"):
            os.environ["VSD_CONV_ORDER"] = order
            got, ref = run_conv(ops, [x], h, w, wt, b, ksize=ks, tile=tile, split_k=split, pipeline=pipeline, act=2)
            outs[order] = got
    finally:
        os.environ.pop("VSD_CONV_ORDER", None)
    check(outs["0"], ref, "conv, order 0")
    for order, o in outs.items():
        assert torch.equal(o, outs["0"]), order


def test_no_op_writes_outside_its_buffers_on_random_ragged_shapes():
    """scripts/guard_fuzz.py for 20 s: conv (every tile / pipeline / split-K form), QKV with transposed V^T output, GroupNorm,
    LayerNorm and attention on random ragged shapes, every writable buffer cut out of a larger allocation between canaries --
    the canaries stay intact and the results match the fp32 references."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "guard_fuzz.py"), "20", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "guard fuzz passed" in r.stdout, (r.stdout[-600:], r.stderr[-1200:])


def test_no_op_touches_a_byte_past_its_operands_on_random_ragged_shapes():
    """scripts/guard_page_fuzz.py for 25 s: the same random ragged shapes with EVERY operand (inputs, weights, bias, residual,
    statistics, split-K workspace, outputs) in a buffer that ends at -- or starts right after -- an unmapped page (HIP's
    virtual-memory API): an out-of-bounds READ takes a GPU memory fault there and then.  Round 4's fault (the tile-softmax epilogue
    behind split-K reading slab rows past M) depended on what the allocator had placed behind the workspace; this does not."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "guard_page_fuzz.py"), "25", "7"], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "guard page fuzz passed" in r.stdout, (r.stdout[-800:], r.stderr[-1200:])

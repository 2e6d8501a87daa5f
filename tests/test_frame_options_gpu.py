"""Per-frame options on the GPU (include/vsd.h: strength and ControlNet scale per frame of one launch): the scheduler kernels with
coefficients per image against the `_dev` / `_seeded` kernels bit for bit, `vsd_groupnorm_addvec` against `vsd_groupnorm_batched` bit for
bit where the sum is exact and against fp32 torch otherwise, `vsd_cn_merge_frames` bit for bit against an exactly evaluated fma, the
engine's frames against uniform launches, the oracle and the default program, two lanes in flight, and the drop-in class."""
import inspect
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_option_cases as FO  # noqa: E402
import test_frame_prompts_gpu as FP  # noqa: E402  (its engine set-up, its pipeline factory and -- by source -- its oracle bounds)
from test_ops_gpu import check  # noqa: E402  (max-abs 2^-8 * max|ref|, rel-L2 2e-3)
from test_pipeline_gpu import _frame, _psnr  # noqa: E402

from videosd_amd.lcm import LCMSchedule  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 2
OPTS = (FO.OPT_A, FO.OPT_B)
SENT16 = 0x5A5A  # the bits of every sentinel half
TAIL = 3         # sentinel rows behind every output
# the oracle bounds of test_frame_prompts_gpu._engine_case: taken from its source, so that they cannot drift apart
ORACLE_BOUNDS = "r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0"
R1_MAX, MAD_MAX, PSNR_MIN = 2e-2, 1.5, 38.0


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _mad(a, b):
    return float(np.abs(a.astype(int) - b.astype(int)).mean())


def _sentinel(ops, rows, cols):
    """a device buffer of rows + TAIL rows, every half the sentinel"""
    return ops.to_device(torch.full((rows + TAIL, cols), SENT16, dtype=torch.int16).view(torch.float16))


def _bits(ops, t):
    ops.synchronize()
    return t.cpu().contiguous().view(torch.int16).numpy()


def _tail_ok(ops, t, rows):
    return bool((_bits(ops, t)[rows:] == SENT16).all())


# ------------------------------------------------------------------------------------------ scheduler kernels, coefficients per image
def _coef_block(B, stride):
    """fp32 [B][stride]: image b the coefficients of LCMSchedule(strength_b, 2) in the engine's layout, sentinels in the padding"""
    blk = torch.full((B, stride), 777.0, dtype=torch.float32)
    for b in range(B):
        s = LCMSchedule((0.3, 0.6, 0.9)[b % 3], 2)
        blk[b, 0:2] = torch.tensor(s.add_noise_coef(), dtype=torch.float32)
        blk[b, 2:8] = torch.tensor([float(v) for v in s.step_coef(0)], dtype=torch.float32)
    return blk


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("hw", [1, 135, 1024])
def test_scheduler_kernels_with_coefficients_per_image(ops, hw, batch):
    B, stride = batch, 16
    g = torch.Generator().manual_seed(10 * hw + B)
    rnd = lambda: ops.to_device(torch.randn(B * hw, 8, generator=g).half())  # noqa: E731
    x0, eps, sample = rnd(), rnd(), rnd()
    coef = ops.to_device(_coef_block(B, stride))
    if B > 1:
        assert not torch.equal(coef[0, :8], coef[1, :8])
    noise = ops.to_device(torch.randn(4, hw, generator=g))
    seeds = ops.to_device(torch.tensor([7, 8, 9, 7, 11][:B], dtype=torch.int64))
    rows = lambda t, b: t[b * hw:(b + 1) * hw]  # noqa: E731
    new = lambda: _sentinel(ops, B * hw, 8)  # noqa: E731
    # add_noise: the shared table, and per-image seeds
    for seeded in (False, True):
        got, want = new(), new()
        if seeded:
            ops.add_noise_frames(x0, None, seeds, 0, 0, coef[0, 0:2], stride, hw, B, got)
        else:
            ops.add_noise_frames(x0, noise, None, 0, 0, coef[0, 0:2], stride, hw, B, got)
        for b in range(B):
            if seeded:
                ops.add_noise_seeded(rows(x0, b), seeds[b:b + 1], 0, 0, coef[b, 0:2], hw, 1, rows(want, b))
            else:
                ops.add_noise_dev(rows(x0, b), noise, coef[b, 0:2], hw, 1, rows(want, b))
        assert np.array_equal(_bits(ops, got), _bits(ops, want)), ("add_noise", seeded)
        assert _tail_ok(ops, got, B * hw)
    # lcm_step: table noise, seeded noise (draw 1), and the step that adds none; with and without dec_in
    for mode in ("table", "seeded", "none"):
        for with_dec in (True, False):
            gp, gd, gi = new(), new(), new() if with_dec else None
            wp, wd, wi = new(), new(), new() if with_dec else None
            ops.lcm_step_frames(eps, sample, noise if mode == "table" else None, seeds if mode == "seeded" else None, 0, 1 if mode == "seeded" else 0,
                                coef[0, 2:8], stride, hw, B, gp, gd, gi)
            for b in range(B):
                if mode == "seeded":
                    ops.lcm_step_seeded(rows(eps, b), rows(sample, b), seeds[b:b + 1], 0, 1, coef[b, 2:8], hw, 1, rows(wp, b), rows(wd, b),
                                        rows(wi, b) if with_dec else None)
                else:
                    ops.lcm_step_dev(rows(eps, b), rows(sample, b), noise if mode == "table" else None, coef[b, 2:8], hw, 1, rows(wp, b),
                                     rows(wd, b), rows(wi, b) if with_dec else None)
            for name, a, w in (("prev", gp, wp), ("denoised", gd, wd)) + ((("dec_in", gi, wi),) if with_dec else ()):
                assert np.array_equal(_bits(ops, a), _bits(ops, w)), (mode, with_dec, name)
                assert _tail_ok(ops, a, B * hw)
            if mode == "none":
                assert np.array_equal(_bits(ops, gp), _bits(ops, gd))  # no noise: prev = denoised


def test_scheduler_kernels_refuse_bad_arguments(ops):
    hw, B, stride = 16, 2, 16
    x = ops.to_device(torch.randn(B * hw, 8).half())
    coef = ops.to_device(_coef_block(B, stride))
    noise = ops.zeros(4, hw, dtype=torch.float32)
    seeds = ops.zeros(B, dtype=torch.int64)
    out, out2 = _sentinel(ops, B * hw, 8), _sentinel(ops, B * hw, 8)
    bad_add = [dict(noise=noise, seeds=seeds), dict(noise=None, seeds=None), dict(noise=noise, seeds=None, stride=1),
               dict(noise=noise, seeds=None, batch=0), dict(noise=noise, seeds=None, batch=65536), dict(noise=noise, seeds=None, hw=0),
               dict(noise=None, seeds=seeds, draw=-1)]
    for k in bad_add:
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*add_noise_frames"):
            ops.add_noise_frames(x, k["noise"], k["seeds"], 0, k.get("draw", 0), coef[0, 0:2], k.get("stride", stride), k.get("hw", hw),
                                 k.get("batch", B), out)
    bad_step = [dict(noise=noise, seeds=seeds, draw=1), dict(noise=None, seeds=seeds, draw=0), dict(noise=noise, seeds=None, stride=5),
                dict(noise=None, seeds=None, batch=0), dict(noise=None, seeds=None, hw=-1)]
    for k in bad_step:
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*lcm_step_frames"):
            ops.lcm_step_frames(x, x, k["noise"], k["seeds"], 0, k.get("draw", 0), coef[0, 2:8], k.get("stride", stride), k.get("hw", hw),
                                k.get("batch", B), out, out2, None)
    for t in (out, out2):
        assert bool((_bits(ops, t) == SENT16).all())  # nothing was launched


# ------------------------------------------------------------------------------------------ groupnorm_addvec
GN_SHAPES = [(64, 32), (320, 32), (1280, 32)]
GN_HW = [1, 4, 64, 135, 1024]
GN_BATCH = [1, 2, 5]


def test_groupnorm_addvec_cases_cover_both_launch_forms(ops):
    forms = {ops.groupnorm_launches(c, 0, hw, g, B) for c, g in GN_SHAPES for hw in GN_HW for B in GN_BATCH}
    assert forms == {1, 2}, forms


def _gn_run(ops, x, vec, ld, c, hw, B, groups, gamma, beta, silu):
    """-> (bits of groupnorm_addvec's output, tail intact); vec: [B][c] (None: plain batched GroupNorm), placed at pitch ld"""
    out = _sentinel(ops, B * hw, c)
    if vec is None:
        ops.groupnorm(x, None, c, 0, hw, groups, 1e-5, gamma, beta, silu, out, batch=B)
    else:
        av = torch.full((B, ld), 3.0, dtype=torch.float16)
        av[:, :c] = vec
        ops.groupnorm_addvec(x, ops.to_device(av), ld, c, hw, groups, 1e-5, gamma, beta, silu, out, batch=B)
    return _bits(ops, out)[:B * hw], _tail_ok(ops, out, B * hw), out


@pytest.mark.parametrize("batch", GN_BATCH)
@pytest.mark.parametrize("hw", GN_HW)
@pytest.mark.parametrize("c,groups", GN_SHAPES)
def test_groupnorm_addvec(ops, c, groups, hw, batch):
    B, ld = batch, c + 24
    g = torch.Generator().manual_seed(c + 7 * hw + B)
    gamma = ops.to_device((1 + 0.1 * torch.randn(c, generator=g)).half())
    beta = ops.to_device((0.1 * torch.randn(c, generator=g)).half())
    # general data, a different vector per image (images at different scales, as test_ops_gpu's batched case)
    x = (torch.randn(B * hw, c, generator=g) * torch.tensor([1.0, 3.0, 0.3, 2.0, 0.5][:B]).repeat_interleave(hw)[:, None] + 0.5).half()
    vec = (torch.randn(B, c, generator=g) * 0.7).half()
    # exact data: multiples of 2^-4 below 8, so that the fp16 sum is exact
    xe = (torch.randint(-127, 128, (B * hw, c), generator=g).float() / 16).half()
    ve = (torch.randint(-127, 128, (B, c), generator=g).float() / 16).half()
    se = xe.float().reshape(B, hw, c) + ve.float()[:, None, :]
    assert torch.equal(se.half().float(), se)  # the sum is exact in fp16
    xd, xed, sed = ops.to_device(x), ops.to_device(xe), ops.to_device(se.half().reshape(B * hw, c))
    for silu in (True, False):
        # a zero vector: vsd_groupnorm_batched's bits
        plain, ok0, _ = _gn_run(ops, xd, None, 0, c, hw, B, groups, gamma, beta, silu)
        zero, ok1, _ = _gn_run(ops, xd, torch.zeros(B, c, dtype=torch.float16), ld, c, hw, B, groups, gamma, beta, silu)
        assert ok0 and ok1 and np.array_equal(zero, plain), ("zero vector", silu)
        # an exact sum: vsd_groupnorm_batched(x + a), bit for bit
        want, _, _ = _gn_run(ops, sed, None, 0, c, hw, B, groups, gamma, beta, silu)
        got, ok, _ = _gn_run(ops, xed, ve, ld, c, hw, B, groups, gamma, beta, silu)
        assert ok and np.array_equal(got, want), ("exact sum", silu)
        # general data: fp32 torch on the fp16-rounded inputs
        _, ok, out = _gn_run(ops, xd, vec, ld, c, hw, B, groups, gamma, beta, silu)
        s = x.float().reshape(B, hw, c) + vec.float()[:, None, :]
        ref = F.group_norm(s.transpose(1, 2), groups, gamma.float().cpu(), beta.float().cpu(), 1e-5).transpose(1, 2).reshape(B * hw, c)
        if silu:
            ref = F.silu(ref)
        assert ok
        check(out[:B * hw], ref, f"groupnorm_addvec C={c} hw={hw} B={B} silu={silu}")
        if B > 1 and hw > 1:  # the vector is the image's own: with image 0's vector for every image the output differs
            same, _, _ = _gn_run(ops, xd, vec[0:1].expand(B, c), ld, c, hw, B, groups, gamma, beta, silu)
            assert not np.array_equal(same, _bits(ops, out)[:B * hw])


def test_groupnorm_addvec_refuses_bad_arguments(ops):
    c, hw, B = 64, 4, 2
    x = ops.to_device(torch.randn(B * hw, c).half())
    gamma, beta = ops.to_device(torch.ones(c).half()), ops.to_device(torch.zeros(c).half())
    av = ops.to_device(torch.zeros(B, c + 8).half())
    out = _sentinel(ops, B * hw, c)
    for vec, ld, cc, groups in ((av.view(-1)[4:], c + 8, c, 32), (av, c + 4, c, 32), (av, -8, c, 32), (av, c + 8, c - 4, 32), (av, c + 8, c, 48)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            ops.groupnorm_addvec(x, vec, ld, cc, hw, groups, 1e-5, gamma, beta, True, out, batch=B)
    assert bool((_bits(ops, out) == SENT16).all())


# ------------------------------------------------------------------------------------------ cn_merge_frames
MERGE_SHAPES = [(rows, c) for rows in (1, 4, 64, 135) for c in (8, 320, 1280)]


def _exact_halves(g, shape):
    """fp16 values that are zero or have a magnitude in [2^-6, 16): a random 11-bit significand, exponent -6..3, one in ten zero"""
    m = torch.randint(1024, 2048, shape, generator=g).double()
    e = torch.randint(-6, 4, shape, generator=g).double()
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    v = sgn * m / 1024 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)
    v = torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros_like(v), v)
    h = v.half()
    assert torch.equal(h.double(), v)
    return h


def _merge_problem(ops, shapes, B, seed):
    """segments of the given (rows per image, channels), distinct scale columns -> (table rows, tensors, scales [B][stride], stride)"""
    g = torch.Generator().manual_seed(seed)
    stride = 16
    scales = torch.randint(0, 1024, (B, stride), generator=g).float() / 256  # multiples of 2^-8 below 4
    cols = torch.randperm(stride, generator=g)[:len(shapes)].tolist()
    segs, tens = [], []
    for (rows, c), col in zip(shapes, cols):
        z, u = _exact_halves(g, (B * rows, c)), _exact_halves(g, (B * rows, c))
        zd, ud, od = ops.to_device(z), ops.to_device(u), _sentinel(ops, B * rows, c)
        segs.append((zd.data_ptr(), ud.data_ptr(), od.data_ptr(), rows, c, col))
        tens.append((z, u, zd, ud, od))
    return segs, tens, scales, stride


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("nseg", [1, 3, 13])
def test_cn_merge_frames_bit_for_bit(ops, nseg, batch):
    """every (rows per image, channels) of MERGE_SHAPES with this segment count and batch: launches of `nseg` segments each, the last one
    filled up from the start of the list"""
    B = batch
    todo = list(MERGE_SHAPES)
    while len(todo) % nseg:
        todo.append(MERGE_SHAPES[len(todo) % len(MERGE_SHAPES)])
    checked = 0
    for k in range(0, len(todo), nseg):
        shapes = todo[k:k + nseg]
        segs, tens, scales, stride = _merge_problem(ops, shapes, B, seed=100 * nseg + 10 * B + k)
        assert len({s[5] for s in segs}) == nseg  # distinct scale columns
        tab = ops.to_device(torch.tensor(segs, dtype=torch.int64))
        ops.cn_merge_frames(tab, nseg, ops.to_device(scales), stride, B)
        for (za, ua, oa, rows, c, col), (z, u, _zd, _ud, od) in zip(segs, tens):
            sc = scales[:, col].double().repeat_interleave(rows)[:, None]
            f64 = z.double() * sc + u.double()  # exact in fp64 (asserted on a sample below): so this IS the fma's unrounded value
            want = f64.float().half().view(torch.int16).numpy()
            got = _bits(ops, od)
            assert np.array_equal(got[:B * rows], want), (rows, c, col, B)
            assert bool((got[B * rows:] == SENT16).all())
            if checked < 4:  # the exactness claim, with rationals
                idx = torch.randint(0, B * rows * c, (16,), generator=torch.Generator().manual_seed(checked)).tolist()
                for i in idx:
                    r, ch = divmod(i, c)
                    exact = Fraction(float(z[r, ch])) * Fraction(float(scales[r // rows, col])) + Fraction(float(u[r, ch]))
                    assert Fraction(float(f64[r, ch])) == exact
                checked += 1


def test_cn_merge_frames_refuses_bad_arguments(ops):
    B = 2
    segs, tens, scales, stride = _merge_problem(ops, [(4, 8), (4, 320)], B, seed=5)
    sd = ops.to_device(scales)
    good = ops.to_device(torch.tensor(segs, dtype=torch.int64))

    def table(edit):
        rows = [list(s) for s in segs]
        edit(rows)
        return ops.to_device(torch.tensor(rows, dtype=torch.int64))

    many = ops.to_device(torch.tensor([segs[0]] * 17, dtype=torch.int64))
    cases = [(many, 17, sd, stride, B), (good, -1, sd, stride, B), (good, 2, sd, stride, 0), (good, 2, sd, stride, 65536),
             (table(lambda r: r[1].__setitem__(0, r[1][0] + 8)), 2, sd, stride, B),   # a misaligned z
             (table(lambda r: r[0].__setitem__(2, r[0][2] + 2)), 2, sd, stride, B),   # a misaligned out
             (table(lambda r: r[1].__setitem__(4, 12)), 2, sd, stride, B),            # channels no multiple of 8
             (table(lambda r: r[0].__setitem__(3, 0)), 2, sd, stride, B),             # no rows
             (table(lambda r: r[0].__setitem__(5, stride)), 2, sd, stride, B),        # a scale column beyond the stride
             (good.view(-1)[1:].view(torch.int64), 1, sd, stride, B),                 # a misaligned table
             (good, 2, sd.view(-1)[1:].view(torch.int16)[1:], stride, B)]             # misaligned scales
    for tab, nseg, s, st, b in cases:
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*cn_merge_frames"):
            ops.cn_merge_frames(tab, nseg, s, st, b)
    for _z, _u, _zd, _ud, od in tens:
        assert bool((_bits(ops, od) == SENT16).all())  # ... and nothing was written
    ops.cn_merge_frames(good, 2, sd, stride, B)  # the good table still works
    assert not bool((_bits(ops, tens[0][4])[:B * 4] == SENT16).all())


# ------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def mini():
    from videosd_amd import config as C

    return FP._setup(C.MINI_UNET, C.MINI_CONTROLNET)


def _engine_case(setup, H, W, idx):
    """frames of a launch whose frame b runs with OPTS[idx[b]]: deterministic, bit for bit the frames of uniform launches of the same
    program, at the oracle's bounds with their own options; the distance to the default program with those options is printed"""
    assert ORACLE_BOUNDS in inspect.getsource(FP._engine_case)
    eng, orc, texts, blocks = setup
    B = len(idx)
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)[:B]])
    prep = dict(use_controlnet=True, batch=B, autotune=False)
    eng.use_prompt(blocks[0])
    plan = eng.prepare(H, W, STEPS, OPTS[0][0], controlnet_scale=OPTS[0][1], **prep)
    assert plan["frame_options"] is False and plan["n"] == 2
    default = [eng.infer_u8(frames)]
    assert eng.update_options(*OPTS[1])
    default.append(eng.infer_u8(frames))
    plan = eng.prepare(H, W, STEPS, OPTS[0][0], controlnet_scale=OPTS[0][1], frame_options=True, **prep)
    assert plan["frame_options"] is True and plan["n"] == 2
    eng.use_options([OPTS[i] for i in idx])
    got = eng.infer_u8(frames)
    assert np.array_equal(got, eng.infer_u8(frames))  # deterministic replay
    h0, w0 = H // 8, W // 8
    den = eng.buffers["denoised"][:, :4].float().cpu().reshape(B, h0, w0, 4).permute(0, 3, 1, 2)
    uniform = []
    for o in OPTS:
        eng.use_options([o] * B)
        uniform.append(eng.infer_u8(frames))
    for b, oi in enumerate(idx):
        assert np.array_equal(got[b], uniform[oi][b]), (b, _mad(got[b], uniform[oi][b]))
        assert not np.array_equal(uniform[0][b], uniform[1][b])
        refs = []
        for k in (oi, 1 - oi):  # the frame's own options (its trace is read below), then the other pair
            refs.append(np.asarray(orc.infer(Image.fromarray(frames[b], "RGB"), texts[0][None].float(), height=H, width=W, strength=OPTS[k][0],
                                             steps=STEPS, seed=23, controlnet_scale=OPTS[k][1], use_controlnet=True, keep_trace=True)))
            if k == oi:
                ref_den = orc.trace["denoised"][-1][0]
        ref = refs[0]
        assert _mad(refs[0], refs[1]) > 2 * MAD_MAX, _mad(refs[0], refs[1])  # the options matter far beyond the bound below
        r1 = float((den[b] - ref_den).norm() / ref_den.norm())
        mad, psnr, d_def = _mad(got[b], ref), _psnr(got[b], ref), _mad(got[b], default[oi][b])
        print(f"{W}x{H} frame {b} options {OPTS[oi]}: r1 {r1:.3g} mad {mad:.3f} psnr {psnr:.1f} vs default program {d_def:.3f} LSB")
        assert r1 <= R1_MAX and mad <= MAD_MAX and psnr >= PSNR_MIN, (b, r1, mad, psnr)
    return frames, got, uniform


@pytest.mark.parametrize("H,W", [(120, 72), (128, 128)])
def test_mini_engine_frames_follow_their_own_options(mini, H, W):
    _engine_case(mini, H, W, [0, 1, 0])


def test_sd15_widths_frames_follow_their_own_options():
    from videosd_amd import config as C

    _engine_case(FP._setup(C.SD15_UNET, C.SD15_CONTROLNET), 64, 64, [0, 1])


def test_two_lanes_in_flight_with_different_option_lists(mini):
    eng, _orc, _texts, blocks = mini
    H = W = 128
    frames = np.stack([_frame(H, W, seed=s) for s in (21, 22, 23)])
    prep = dict(controlnet_scale=OPTS[0][1], use_controlnet=True, batch=3, autotune=False, frame_options=True)
    eng.use_prompt(blocks[0])
    eng.prepare(H, W, STEPS, OPTS[0][0], **prep)
    slot = eng.make_slot(lane=1)
    slot.use_prompt(blocks[0])
    slot.prepare(H, W, STEPS, OPTS[0][0], **prep)
    assert slot.fo_buf is not eng.fo_buf and slot.fo_scale is not eng.fo_scale  # blocks of its own
    assert slot.family["option_entries"] is eng.family["option_entries"]         # ... entries from the family's cache
    engines = [eng, slot]
    lists = [([0, 1, 0], [1, 1, 0]), ([1, 0, 0], [0, 0, 1])]  # (the second round rewrites slots of both engines)
    seq = []
    for la, lb in lists:
        for e, l in zip(engines, (la, lb)):
            e.use_options([OPTS[i] for i in l])
            seq.append(e.infer_u8(frames))
    assert not np.array_equal(seq[0], seq[1])
    outs = []
    for la, lb in lists:
        for e, l in zip(engines, (la, lb)):
            e.use_options([OPTS[i] for i in l])
            e.submit_u8(frames)  # both launches are now in flight on their lanes' streams
        for e in engines:
            outs.append(e.collect_u8())
    for got, ref in zip(outs, seq):
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------ the drop-in class
def test_the_class_takes_options_per_frame(monkeypatch, tmp_path):
    H, W = 96, 160
    base = dict(height=H, width=W, steps=STEPS)
    imgs = [Image.fromarray(_frame(H, W, seed=s), "RGB") for s in (3, 4)]
    (sa, ca), (sb, cb) = OPTS
    p = FP._pipeline(monkeypatch, frame_options=True)
    assert p.per_frame_options is True and p.option_class(dict(strength=sa, steps=STEPS)) == p.option_class(dict(strength=sb, steps=STEPS)) == 2
    assert p.option_class(dict(strength=0.02, steps=STEPS)) == 1
    outs = [np.asarray(o) for o in p.infer_batch(imgs, strength=[sa, sb], controlnet_scale=[ca, cb], **base)]
    singles = [np.asarray(p.infer(imgs[0], strength=sa, controlnet_scale=ca, **base)), np.asarray(p.infer(imgs[1], strength=sb, controlnet_scale=cb, **base))]
    for o, s in zip(outs, singles):  # (the bound of the per-frame prompt test for a frame of a launch of two against a launch of one)
        assert _mad(o, s) < 0.5, _mad(o, s)
    assert _mad(outs[1], np.asarray(p.infer(imgs[1], strength=sa, controlnet_scale=ca, **base))) > 0.5  # the second frame really ran with ITS options
    assert all(e.plan["frame_options"] for e in p._engines.values()) and len(p._plans) == 1
    assert all(pl.opts is None for pl in p._plans.values())
    # a number keeps its meaning: every frame that value
    same = [np.asarray(o) for o in p.infer_batch(imgs, strength=sa, controlnet_scale=ca, **base)]
    assert np.array_equal(same[0], np.asarray(p.infer_batch(imgs, strength=[sa, sa], controlnet_scale=[ca, ca], **base)[0]))
    assert _mad(same[0], singles[0]) < 0.5
    # a changed option while another lane's launch is in flight: no drain, no error (the default class raises "collect them first" here)
    assert not p.needs_idle(strength=sb, controlnet_scale=cb, **base)
    h0 = p.submit_batch(imgs, lane=0, strength=sa, controlnet_scale=ca, **base)
    h1 = p.submit_batch(imgs, lane=1, strength=sb, controlnet_scale=cb, **base)
    assert len(h0[5]) == 2 and h0[5][0] is h0[5][1] and h1[5][0] is not h0[5][0]  # the handles hold their launches' option entries
    fly = [[np.asarray(o) for o in p.collect_batch(h)] for h in (h0, h1)]
    one = [[np.asarray(o) for o in p.collect_batch(p.submit_batch(imgs, lane=l, strength=s, controlnet_scale=c, **base))] for l, (s, c) in enumerate(OPTS)]
    for a, b in zip(fly, one):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _mad(fly[0][0], fly[1][0]) > 0.5
    # errors: the wrong length, mixed numbers of timesteps, a plan file
    with pytest.raises(ValueError, match="one per frame"):
        p.infer_batch(imgs, strength=[sa], controlnet_scale=ca, **base)
    with pytest.raises(ValueError, match="one per frame"):
        p.infer_batch(imgs, strength=sa, controlnet_scale=[ca, cb, ca], **base)
    with pytest.raises(ValueError, match="numbers of timesteps"):
        p.infer_batch(imgs, strength=[sa, 0.02], controlnet_scale=ca, **base)
    with pytest.raises(ValueError, match="frame_options=True"):
        p.export_plan(str(tmp_path / "x.vsdplan"), strength=sa, controlnet_scale=ca, **base)
    from videosd_amd.plan import export_plan

    with pytest.raises(ValueError, match="frame_options=True"):
        export_plan(next(iter(p._engines.values())), str(tmp_path / "y.vsdplan"))
    del p
    # all three per-frame modes together
    q = FP._pipeline(monkeypatch, frame_options=True, frame_prompts=True, device_seed=True)
    assert q.per_frame_options is True and q.per_frame_prompt is True and q.per_frame_seed is True
    pa, pb = "a watercolor painting", ["a charcoal sketch"]
    outs = [np.asarray(o) for o in q.infer_batch([imgs[0]] * 2, prompts=[pa, pb], seed=[1, 2], strength=[sa, sb], controlnet_scale=[ca, cb], **base)]
    singles = [np.asarray(q.infer(imgs[0], prompt=pa, seed=1, strength=sa, controlnet_scale=ca, **base)),
               np.asarray(q.infer(imgs[0], prompt=pb, seed=2, strength=sb, controlnet_scale=cb, **base))]
    for o, s in zip(outs, singles):
        assert _mad(o, s) < 0.5, _mad(o, s)
    plan = next(iter(q._engines.values())).plan
    assert plan["frame_options"] and plan["frame_prompts"] and plan["device_seed"]
    assert _mad(outs[0], np.asarray(q.infer(imgs[0], prompt=pa, seed=1, strength=sb, controlnet_scale=cb, **base))) > 0.5  # the options count ...
    assert _mad(outs[0], np.asarray(q.infer(imgs[0], prompt=pa, seed=2, strength=sa, controlnet_scale=ca, **base))) > 0.5  # ... and the seed
    assert _mad(outs[0], np.asarray(q.infer(imgs[0], prompt=pb, seed=1, strength=sa, controlnet_scale=ca, **base))) > 0.5  # ... and the prompt
    del q
    # the unchanged default: the default program, one pair of options per launch, and the drain it needs
    r = FP._pipeline(monkeypatch)
    assert r.per_frame_options is False
    with pytest.raises(ValueError, match="frame_options=True"):
        r.infer_batch(imgs, strength=[sa, sb], controlnet_scale=ca, **base)
    r.infer_batch(imgs, strength=[sa, sa], controlnet_scale=ca, **base)  # (equal values are one pair)
    assert not any(e.plan["frame_options"] for e in r._engines.values())
    names = {fn.__name__ for e in r._engines.values() for fn, _a, _k in e.flat_calls(e.program.calls)}
    assert not names & {"add_noise_frames", "lcm_step_frames", "groupnorm_addvec", "cn_merge_frames"} and "lcm_step_dev" in names
    h0 = r.submit_batch(imgs, lane=0, strength=sa, controlnet_scale=ca, **base)
    with pytest.raises(RuntimeError, match="collect them first"):
        r.submit_batch(imgs, lane=1, strength=sb, controlnet_scale=cb, **base)
    r.collect_batch(h0)

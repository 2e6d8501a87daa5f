"""Per-frame seeded noise on the MI355X (include/vsd.h THE NOISE CONTRACT; csrc/noise.hip): the kernels against the numpy restatement of the
contract (seed_cases.py: the Philox integers bit for bit, the normals against fp64), the fused scheduler kernels against "fill, then the
existing kernel" bit for bit, the engine, the CPU oracle fed the restatement's draws, the drop-in class and plan files.

Shapes: hw in {1, 15, 257, 4097} -- a lone thread, a 3 x 5 latent, one past a wave / a workgroup boundary, more than one workgroup plus a
tail; the engine cases are the MINI nets at 96 x 160 with 2 steps (step noise and the ControlNet are exercised; a case takes seconds).

The bound on the normals, 8e-6 absolute: 4 x 1.85e-6, the latter the largest error over 2^24 normals (seed 42, draw 3) of the contract's
formulas evaluated in fp32 with numpy against fp64; the factor 4 covers a device logf / sincosf of ~2 ulp where numpy's measured ~1, at
r <= 5.77.  The test prints what the device reaches; scripts/seed_noise.py measures it over 2^20 normals per draw (profiles/seed_noise.txt)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, STEPS = 96, 160, 2
STRENGTH, SCALE = 0.6, 1.5
NORMAL_BOUND = 8e-6


# (the frame, weights and text of tests/test_pipeline_gpu.py's helpers, re-stated)
def _frame(h, w, seed=1):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = ((xx * 5 + yy * 3) % 256).astype(np.uint8)[..., None]
    return (base // 2 + grad // 2).astype(np.uint8)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@functools.lru_cache(maxsize=None)
def _mini():
    from videosd_amd import config as Cf
    from videosd_amd import weights as Wt

    wu = Wt.synthesize(Wt.unet_spec(Cf.MINI_UNET), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(Cf.MINI_CONTROLNET), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(Cf.TAESD), "vae.", device="cuda")
    text = (torch.randn(77, Cf.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half()
    return wu, wc, wv, text


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def eng(ops):
    from videosd_amd import config as Cf
    from videosd_amd.engine import Engine

    wu, wc, wv, text = _mini()
    e = Engine(ops, Cf.MINI_UNET, Cf.MINI_CONTROLNET, Cf.TAESD, wu, wc, wv)
    e.set_text_embeds(text)
    return e


def _fill(ops, seed, kind, draw, hw, raw):
    out = ops.zeros(hw, 4, dtype=torch.int32) if raw else ops.zeros(4, hw, dtype=torch.float32)
    ops.noise_fill(seed, kind, draw, hw, out, raw=raw)
    ops.synchronize()
    a = out.cpu().numpy()
    return a.view(np.uint32) if raw else a


# ------------------------------------------------------------------------------------------ 1. the integers
@pytest.mark.parametrize("hw", [1, 15, 257, 4097])
def test_the_philox_integers_equal_the_restatement(ops, hw):
    for seed in SC.SEEDS:
        for kind in (0, 1):
            for draw in (0, 4):
                got = _fill(ops, seed, kind, draw, hw, raw=True)
                assert got.shape == (hw, 4) and np.array_equal(got, SC.raw_draw(seed, kind, draw, hw)), (seed, kind, draw)
    # seed 0 / kind 0 / draw 0 / pixel 0: the all-zero known answer of Random123
    assert tuple(int(v) for v in _fill(ops, 0, 0, 0, hw, raw=True)[0]) == SC.KNOWN_ANSWERS[0][2]


# ------------------------------------------------------------------------------------------ 2. the normals
def test_the_normals_are_within_the_fp32_bound_of_the_fp64_restatement(ops):
    hw = 4097
    worst = 0.0
    for seed, kind, draw in [(42, 0, 3), (0, 0, 0), (2 ** 64 - 1, 1, 4), (2 ** 32 + 5, 0, 1)]:
        got = _fill(ops, seed, kind, draw, hw, raw=False)
        want = SC.normal_draw(seed, kind, draw, hw)
        assert got.dtype == np.float32 and got.shape == (4, hw) and np.isfinite(got).all()
        assert np.abs(got).max() <= 5.77
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"seed {seed} kind {kind} draw {draw}: max |device - fp64| = {err:.3e}")
        worst = max(worst, err)
    assert worst <= NORMAL_BOUND, worst


# ------------------------------------------------------------------------------------------ 3. fused = fill + the existing kernel
@pytest.mark.parametrize("hw", [15, 4097, 262145])
def test_the_seeded_scheduler_kernels_equal_fill_plus_the_existing_kernels_bit_for_bit(ops, hw):
    B, seeds = 3, (7, 8, 7)
    g = torch.Generator().manual_seed(hw)
    rnd = lambda: ops.to_device(torch.randn(B * hw, 8, generator=g).half())  # noqa: E731
    x0, eps, sample = rnd(), rnd(), rnd()
    coef = ops.to_device(torch.tensor([0.8321, 0.5547, 0.3071, 0.9517, 0.9123, 0.4095], dtype=torch.float32))
    seeds_dev = ops.to_device(torch.tensor(seeds, dtype=torch.int64))
    noise = ops.zeros(4, hw, dtype=torch.float32)
    rows = lambda t, b: t[b * hw:(b + 1) * hw]  # noqa: E731
    new = lambda: ops.zeros(B * hw, 8)  # noqa: E731

    def host(t):
        ops.synchronize()
        return t.cpu().numpy().view(np.uint16).reshape(B, hw, 8)

    # add_noise: draw 0 (kind 0) and draw 1 of kind 1
    for kind, draw in ((0, 0), (1, 1)):
        got, want = new(), new()
        ops.add_noise_seeded(x0, seeds_dev, kind, draw, coef[0:2], hw, B, got)
        for b in range(B):
            ops.noise_fill(seeds[b], kind, draw, hw, noise)
            ops.add_noise_dev(rows(x0, b), noise, coef[0:2], hw, 1, rows(want, b))
        g_, w_ = host(got), host(want)
        assert np.array_equal(g_, w_), (kind, draw)
    # lcm_step: a noisy step (draw 2) and the step without noise (draw 0), with and without dec_in
    for draw in (2, 0):
        for with_dec in (True, False):
            gp, gd, gi = new(), new(), new() if with_dec else None
            wp, wd, wi = new(), new(), new() if with_dec else None
            ops.lcm_step_seeded(eps, sample, seeds_dev, 0, draw, coef, hw, B, gp, gd, gi)
            for b in range(B):
                if draw > 0:
                    ops.noise_fill(seeds[b], 0, draw, hw, noise)
                ops.lcm_step_dev(rows(eps, b), rows(sample, b), noise if draw > 0 else None, coef, hw, 1, rows(wp, b), rows(wd, b),
                                 rows(wi, b) if with_dec else None)
            for name, a, b_ in (("prev", gp, wp), ("denoised", gd, wd)) + ((("dec_in", gi, wi),) if with_dec else ()):
                assert np.array_equal(host(a), host(b_)), (draw, with_dec, name)
            p = host(gp)
            if draw > 0:
                assert not np.array_equal(p[0], p[1])  # (images 0 and 2 differ in their inputs here: the draws are compared above)
            else:
                assert np.array_equal(p, host(gd))  # no noise: prev = denoised
    # same inputs for every image: images 0 and 2 (seed 7) get the same bits, image 1 (seed 8) does not
    same = ops.to_device(rows(eps, 0).repeat(B, 1).contiguous())
    same_x = ops.to_device(rows(sample, 0).repeat(B, 1).contiguous())
    gp, gd = new(), new()
    ops.lcm_step_seeded(same, same_x, seeds_dev, 0, 2, coef, hw, B, gp, gd, None)
    p, d = host(gp), host(gd)
    assert np.array_equal(p[0], p[2]) and not np.array_equal(p[0], p[1]) and np.array_equal(d[0], d[1])
    lat = new()
    ops.add_noise_seeded(same_x, seeds_dev, 0, 0, coef[0:2], hw, B, lat)
    lt = host(lat)
    assert np.array_equal(lt[0], lt[2]) and not np.array_equal(lt[0], lt[1])


# ------------------------------------------------------------------------------------------ 4. the engine
def _names(e):
    from videosd_amd.engine import Engine

    return [fn.__name__ for fn, _a, _k in Engine.flat_calls(e.program.calls)]


def test_the_seed_reaches_the_picture_and_nothing_else_does(eng):
    f = _frame(H, W)
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True, device_seed=True)
    assert eng.plan["device_seed"] is True and eng.noise is None
    eng.submit_u8(f, seeds=23)
    a = eng.collect_u8()
    eng.submit_u8(f, seeds=23)
    assert np.array_equal(eng.collect_u8(), a)
    eng.submit_u8(f, seeds=24)
    b = eng.collect_u8()
    assert not np.array_equal(a, b)  # (what fails without the feature: two frames that differ only in `seed` were bit-identical)
    eng.submit_u8(f)  # no seeds given: those of the launch before
    assert np.array_equal(eng.collect_u8(), b)
    eng.submit_u8(f, seeds=23 + 2 ** 64)  # modulo 2^64
    assert np.array_equal(eng.collect_u8(), a)
    with pytest.raises(ValueError):
        eng.submit_u8(f, seeds=[1, 2])
    seeded_total, seeded_names = eng.launches_by_kind()[0], _names(eng)
    # the default program: call for call what it was, and the seeded one differs from it in the three scheduler calls alone
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True)
    default_names, default_total = _names(eng), eng.launches_by_kind()[0]
    assert eng.plan["device_seed"] is False and eng.seed_dev is None and eng.noise is not None
    with pytest.raises(ValueError, match="device_seed"):
        eng.submit_u8(f, seeds=1)
    d0 = eng.infer_u8(f)
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True, device_seed=False)
    assert _names(eng) == default_names and not any("seeded" in n or n == "noise_fill" for n in default_names)
    assert default_names.count("add_noise_dev") == 1 and default_names.count("lcm_step_dev") == STEPS
    assert np.array_equal(eng.infer_u8(f), d0)
    swap = {"add_noise_dev": "add_noise_seeded", "lcm_step_dev": "lcm_step_seeded"}
    assert seeded_names == [swap.get(n, n) for n in default_names]
    assert seeded_total == default_total


def test_a_frames_seed_is_its_own_inside_a_launch(eng):
    f = _frame(H, W)
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True, batch=3, device_seed=True)
    frames = np.stack([f, f, f])
    eng.submit_u8(frames, seeds=[11, 12, 13])
    first = eng.collect_u8()
    eng.submit_u8(frames, seeds=[11, 14, 13])
    second = eng.collect_u8()
    # the same place in the same launch shape gives the same bits
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2])
    assert not np.array_equal(first[1], second[1])
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[0], first[2])


def test_reference_only_mode_with_seeded_noise(eng):
    h = w = 64
    f, ref = _frame(h, w, seed=1), _frame(h, w, seed=9)
    eng.prepare(h, w, 2, STRENGTH, use_controlnet=False, ref_mode=True, device_seed=True)
    eng.ops.upload(eng.ref_u8, torch.from_numpy(ref))
    names = _names(eng)
    assert names.count("add_noise_seeded") == 1 + 2 and "add_noise_dev" not in names and eng.noise_ref is None
    eng.submit_u8(f, seeds=5)
    a = eng.collect_u8()
    eng.submit_u8(f, seeds=6)
    b = eng.collect_u8()
    eng.submit_u8(f, seeds=5)
    assert np.array_equal(eng.collect_u8(), a) and not np.array_equal(a, b)
    assert torch.isfinite(eng.buffers["denoised"].float()).all()


# ------------------------------------------------------------------------------------------ 5. the oracle, fed the contract's draws
@pytest.mark.parametrize("h,w,steps,cn", [(H, W, STEPS, True), (128, 128, 1, False)])
def test_seeded_frames_match_the_oracle_given_the_same_draws(eng, monkeypatch, h, w, steps, cn):
    from oracle.pipeline import OraclePipeline
    from videosd_amd import config as Cf

    wu, wc, wv, text = _mini()
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    orc = OraclePipeline(Cf.MINI_UNET, Cf.MINI_CONTROLNET, cpu(wu), cpu(wc), cpu(wv))
    seed, h0, w0 = 23, h // 8, w // 8
    f = _frame(h, w)
    eng.prepare(h, w, steps, STRENGTH, controlnet_scale=SCALE, use_controlnet=cn, device_seed=True)
    eng.submit_u8(f, seeds=seed)
    got = eng.collect_u8()
    # torch.randn hands out the restatement's draws in call order: draw 0, then the draw of every scheduler step
    calls = []
    real = torch.randn

    def randn(*size, **kw):
        d = len(calls)
        calls.append(size)
        z = SC.normal_draw(seed, 0, d, h0 * w0).reshape(1, 4, h0, w0)
        return torch.from_numpy(z).to(kw.get("dtype") or torch.float32)

    with monkeypatch.context() as m:
        m.setattr(torch, "randn", randn)
        ref = np.asarray(orc.infer(Image.fromarray(f, "RGB"), text[None].float(), height=h, width=w, strength=STRENGTH, steps=steps, seed=seed,
                                   controlnet_scale=SCALE, use_controlnet=cn, keep_trace=True))
    assert torch.randn is real and len(calls) == (1 + steps if steps > 1 else 1)
    x0 = eng.buffers["x0"][:, :4].float().cpu().reshape(h0, w0, 4).permute(2, 0, 1)
    ref_x0 = orc.trace["init_latents"][0]
    r0 = float((x0 - ref_x0).norm() / ref_x0.norm())
    den = eng.buffers["denoised"][:, :4].float().cpu().reshape(h0, w0, 4).permute(2, 0, 1)
    ref_den = orc.trace["denoised"][-1][0]
    r1 = float((den - ref_den).norm() / ref_den.norm())
    mad = float(np.abs(got.astype(int) - ref.astype(int)).mean())
    psnr = _psnr(got, ref)
    print(f"{h} x {w}, {steps} step(s): r0 {r0:.2e} r1 {r1:.2e} mean abs {mad:.3f} LSB psnr {psnr:.1f} dB")
    assert r0 <= 5e-3 and r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0, (r0, r1, mad, psnr)


# ------------------------------------------------------------------------------------------ 6. the class
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


def test_the_class_honours_seed_only_when_asked(monkeypatch):
    opts = dict(prompt="a watercolor painting", height=H, width=W, strength=STRENGTH, steps=STEPS, controlnet_scale=SCALE)
    img = Image.fromarray(_frame(H, W, seed=3), "RGB")
    p = _pipeline(monkeypatch, device_seed=True)
    assert p.per_frame_seed is True
    one = np.asarray(p.infer(img, seed=1, **opts))
    two = np.asarray(p.infer(img, seed=2, **opts))
    assert not np.array_equal(one, two)
    assert np.array_equal(np.asarray(p.infer(img, seed=1, **opts)), one)
    outs = [np.asarray(o) for o in p.infer_batch([img] * 3, seed=[1, 2, 1], **opts)]
    assert not np.array_equal(outs[0], outs[1])
    spread = int(np.abs(outs[0].astype(int) - outs[2].astype(int)).max())
    print("frames 0 and 2 of one launch, same seed: max difference", spread, "LSB")
    assert spread <= 2  # the documented batch-position spread
    with pytest.raises(ValueError, match="one per frame"):
        p.infer_batch([img] * 3, seed=[1, 2], **opts)
    assert len(p._plans) == 1 and all(e.plan["device_seed"] for e in p._engines.values())
    del p
    q = _pipeline(monkeypatch)  # the unchanged default: `seed` is inert
    assert q.per_frame_seed is False
    a = np.asarray(q.infer(img, seed=1, **opts))
    assert np.array_equal(np.asarray(q.infer(img, seed=2, **opts)), a)
    assert not any(e.plan["device_seed"] for e in q._engines.values())


# ------------------------------------------------------------------------------------------ 7. plan files
def test_a_seeded_plan_gives_the_engines_bits_and_every_lane_keeps_its_seeds(eng, tmp_path):
    from videosd_amd.plan import CPlan, export_plan

    B = 2
    frames = np.stack([_frame(H, W, seed=1), _frame(H, W, seed=2)])
    set_a, set_b = [3, 4], [2 ** 40 + 1, 3]
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True, batch=B, device_seed=True)
    want = {}
    for s in (set_b, set_a):
        eng.submit_u8(frames, seeds=s)
        want[tuple(s)] = eng.collect_u8()
    assert not np.array_equal(want[tuple(set_a)], want[tuple(set_b)])
    path = str(tmp_path / "seeded.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    clone = None
    try:
        assert np.array_equal(plan.infer(frames), want[tuple(set_a)])  # a fresh plan holds the seeds of the engine at export
        plan.set_seeds(set_b)
        assert np.array_equal(plan.infer(frames), want[tuple(set_b)])
        plan.set_seeds(set_a)
        assert np.array_equal(plan.infer(frames), want[tuple(set_a)])
        clone = plan.clone()
        plan.set_seeds(set_b)
        assert np.array_equal(plan.infer(frames), want[tuple(set_b)])
        assert np.array_equal(clone.infer(frames), want[tuple(set_a)])  # the clone's seeds are its own
        for n in (1, 3):
            with pytest.raises(RuntimeError, match=r"\(-1\).*frame\(s\) per launch"):
                plan.set_seeds(list(range(n)))
        arr = (C.c_uint64 * B)(1, 2)
        assert plan.ctx.lib.vsd_plan_set_seeds(plan.ctx.h, plan.h, arr, B + 1) == -1
        assert np.array_equal(plan.infer(frames), want[tuple(set_b)])  # a refused call changed nothing
    finally:
        if clone is not None:
            clone.close()
        plan.close()
    # a plan of the default mode has no seeds
    eng.prepare(H, W, STEPS, STRENGTH, controlnet_scale=SCALE, use_controlnet=True, batch=1)
    first = eng.infer_u8(frames[0])
    path = str(tmp_path / "default.vsdplan")
    export_plan(eng, path)
    plan = CPlan(path)
    try:
        with pytest.raises(RuntimeError, match=r"\(-1\).*no seeded noise"):
            plan.set_seeds(1)
        assert np.array_equal(plan.infer(frames[0]), first)
    finally:
        plan.close()

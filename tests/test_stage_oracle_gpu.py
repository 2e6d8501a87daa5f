"""Keep-mask and all-opt-in frames on the MI355X against the stage oracle (tests/stage_oracle.py), end to end: every frame of a launch of
three against `stage_frame` with that frame's own camera frame, mask, seed, prompt (one of them a mix), strength and ControlNet scale.

What is compared, per frame: x0 against the oracle's init latents (r0); the final denoised latents by r1, over all latent pixels and over
the mixed ones (0 < wl < 1); the frame ahead of the post stages (`program_serial` run up to `postprocess_rgb`) against the oracle's
decoded frame over the restyled pixels, mean LSB and PSNR; the final frame against the numpy post stages applied to that frame, byte for
byte.  The r1 bounds are those of tests/stage_oracle.py (4 x the op emulator's distance, measured on the CPU), which
tests/test_stage_oracle_host.py shows to lie a factor 3 or more below every wiring error of the keep mask it knows: the wrong timestep's
row, another draw, another frame's x0, no anchor, no final blend.  LSB and PSNR are the bounds of tests/test_frame_prompts_gpu.py, taken
from its source.  The only reference of `latent_keep` with seeds, of masks with a coefficient stride, and of the program with every
per-frame switch on.

Shapes: the MINI networks at 64 x 64 and 120 x 72 (8 x 8 and 15 x 9 latents) and the SD1.5 widths at 64 x 64; three frames, three steps."""
import functools
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stage_oracle as SO  # noqa: E402
import test_frame_prompts_gpu as FP  # noqa: E402

pytestmark = pytest.mark.gpu

# the oracle bounds of test_frame_prompts_gpu._engine_case: taken from its source, so that they cannot drift apart
ORACLE_BOUNDS = "r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0"
MAD_MAX, PSNR_MIN = 1.5, 38.0
SHAPES = [("mini", 64, 64), ("mini", 72, 120), ("sd15", 64, 64)]
MINI_SHAPES = SHAPES[:2]


# ------------------------------------------------------------------------------------------ engines and oracles, one per network family
@functools.lru_cache(maxsize=None)
def _setup(which):
    """-> (engine, oracle, (text A, text B), (block A, block B, the mix))"""
    from oracle.pipeline import OraclePipeline
    from videosd_amd import blocks as BK
    from videosd_amd import config as C
    from videosd_amd import weights as Wt
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    ucfg, ccfg = (C.MINI_UNET, C.MINI_CONTROLNET) if which == "mini" else (C.SD15_UNET, C.SD15_CONTROLNET)
    wu = Wt.synthesize(Wt.unet_spec(ucfg), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(ccfg), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(C.TAESD), "vae.", device="cuda")
    ta, tb = SO.texts(ucfg.cross_dim)
    eng = Engine(HipOps(0), ucfg, ccfg, C.TAESD, wu, wc, wv)
    eng.set_text_embeds(ta)
    a, b = eng.build_prompt(ta), eng.build_prompt(tb)
    orc = OraclePipeline(ucfg, ccfg, FP._cpu(wu), FP._cpu(wc), FP._cpu(wv))
    return eng, orc, (ta, tb), (a, b, BK.PromptMix([a, b], SO.MIX_WEIGHTS))


@functools.lru_cache(maxsize=None)
def _right(which, case, H, W, b):
    """frame b of a case by the stage oracle: computed once, shared by the tests, never written to"""
    _eng, orc, text_ab, _blocks = _setup(which)
    return SO.oracle_case(orc, case, H, W, b, text_ab, SO.frames(H, W))


def _hold(eng, which, case, H, W, got, label):
    """the engine's last launch (frames `got`) against the stage oracle, frame by frame, at the bounds -> the frames ahead of the post stages"""
    assert ORACLE_BOUNDS in inspect.getsource(FP._engine_case)
    camera, masks, bound = SO.frames(H, W), SO.masks(H, W), SO.bound(case, H, W, which)
    before, eager = SO.frames_ahead_of_the_post_stages(eng, H, W)
    assert np.array_equal(eager, got), f"{label}: the serial program run call by call does not give the launch's bytes"
    figs = [SO.figures(eng, b, _right(which, case, H, W, b), camera[b], before[b], got[b], masks[b], SO.CASES[case].get("color_match")) for b in range(SO.B)]
    for b, f in enumerate(figs):
        print(f"{label} {which} {W}x{H} frame {b}: r0 {f['r0']:.2e} (<= {SO.R0_MAX:.0e}) r1 {f['r1']:.2e} mixed {f['r1_mixed']:.2e} (<= {bound:.2e}) "
              f"LSB {f['lsb']:.3f} (<= {MAD_MAX}) psnr {f['psnr']:.1f} (>= {PSNR_MIN}) post stages exact {f['post_exact']}")
    for b, f in enumerate(figs):
        assert f["r0"] <= SO.R0_MAX and f["r1"] <= bound and f["r1_mixed"] <= bound, (label, b, f, bound)
        assert f["lsb"] <= MAD_MAX and f["psnr"] >= PSNR_MIN and f["post_exact"], (label, b, f)
        assert np.array_equal(got[b][masks[b] == 0], camera[b][masks[b] == 0])
    return before


def _case(which, case, H, W, use_graph=True):
    eng, _orc, _texts, blocks = _setup(which)
    plan = SO.prepare_case(eng, case, H, W, blocks, use_graph=use_graph, autotune=False)
    assert (eng.graph is not None) == use_graph and all(plan[k] is True for k in SO.CASES[case] if k in ("device_seed", "frame_prompts", "frame_options"))
    return eng, SO.launch_case(eng, case, SO.frames(H, W))


# ------------------------------------------------------------------------------------------ a. masks alone, table noise
@pytest.mark.parametrize("which,H,W", SHAPES)
def test_a_keep_mask_with_table_noise_replayed_and_eager(which, H, W):
    eng, got = _case(which, "keep", H, W)
    assert eng.noise is not None and eng.seed_dev is None
    _hold(eng, which, "keep", H, W, got, "a replay")
    eng, eager = _case(which, "keep", H, W, use_graph=False)
    assert np.array_equal(eager, got)


# ------------------------------------------------------------------------------------------ b. with seeds: `latent_keep` draws draw 0 itself
@pytest.mark.parametrize("which,H,W", MINI_SHAPES)
def test_b_keep_mask_with_seeded_noise(which, H, W):
    eng, got = _case(which, "seed", H, W)
    keeps = [a for fn, a, _k in eng.program_serial.calls if fn.__name__ == "latent_keep"]
    assert len(keeps) == SO.STEPS + 1 and all(a[3] is eng.seed_dev and a[2] is None for a in keeps[:-1]) and max(SO.SEEDS) > 2 ** 32
    _hold(eng, which, "seed", H, W, got, "b")
    eng.submit_u8(SO.frames(H, W), seeds=[SO.SEEDS[0]] * SO.B)  # the seed reaches the kept region's noise: frame 1 with frame 0's seed differs
    other = eng.collect_u8()
    assert np.array_equal(other[0], got[0]) and not np.array_equal(other[1], got[1])


# ------------------------------------------------------------------------------------------ c. with per-frame options: a coefficient stride
@pytest.mark.parametrize("which,H,W", MINI_SHAPES)
def test_c_keep_mask_with_per_frame_options(which, H, W):
    eng, got = _case(which, "options", H, W)
    keeps = [a for fn, a, _k in eng.program_serial.calls if fn.__name__ == "latent_keep"]
    assert all(a[7] == eng.fo_layout.coef_stride >= 6 for a in keeps[:-1]) and len(set(SO.OPTIONS)) == SO.B
    _hold(eng, which, "options", H, W, got, "c")
    for b in range(SO.B):  # a frame of the mixed launch is that frame of a uniform launch, bit for bit
        eng.use_options([SO.OPTIONS[b]] * SO.B)
        uniform = eng.infer_u8(SO.frames(H, W))
        assert np.array_equal(uniform[b], got[b]), b
        assert not np.array_equal(uniform[(b + 1) % SO.B], got[(b + 1) % SO.B])


# ------------------------------------------------------------------------------------------ d. every switch at once
def _all_slots_carry(eng, blocks, b, H, W):
    """a launch whose three slots all carry frame b's inputs -> its frames"""
    camera, masks = SO.frames(H, W), SO.masks(H, W)
    eng.use_prompts([SO.blocks_of_frames(blocks)[b]] * SO.B)
    eng.use_options([SO.OPTIONS[b]] * SO.B)
    eng.set_masks(np.stack([masks[b]] * SO.B))
    eng.submit_u8(np.stack([camera[b]] * SO.B), seeds=[SO.SEEDS[b]] * SO.B)
    return eng.collect_u8()


@pytest.mark.parametrize("which,H,W", SHAPES)
def test_d_all_switches_at_once(which, H, W):
    eng, got = _case(which, "all", H, W)
    plan = eng.plan
    assert plan["edge_mode"] == "canny" and plan["color_match"] == "histogram" and plan["keep_mask"] and plan["frame_options"] and plan["frame_prompts"] and plan["device_seed"]
    names = [fn.__name__ for fn, _a, _k in eng.program_serial.calls]
    assert names[-3:] == ["postprocess_rgb", "color_match", "mask_blend"] and names.count("canny_control") == SO.B
    before = _hold(eng, which, "all", H, W, got, "d")
    assert not np.array_equal(before, got)
    for b in range(SO.B):  # the final frame of the mixed launch is that frame's when all three slots carry its inputs, bit for bit
        same = _all_slots_carry(eng, _setup(which)[3], b, H, W)
        assert np.array_equal(same[b], got[b]), (b, SO.mad(same[b], got[b]))


# ------------------------------------------------------------------------------------------ e. the class
def test_e_the_class_gives_the_engines_frames(monkeypatch):
    from videosd_amd import blocks as BK

    which, H, W = "mini", 64, 64
    camera, masks = SO.frames(H, W), SO.masks(H, W)
    ta, tb = SO.texts(_setup(which)[1].unet_cfg.cross_dim)
    p = FP._pipeline(monkeypatch, frame_prompts=True, frame_options=True, device_seed=True, edges="canny", canny_thresholds=SO.CANNY,
                     color_match="histogram", keep_mask=True)
    p.set_prompt_embeds(ta, key="A")
    p.set_prompt_embeds(tb, key="B")
    mix = {"mix": [["A", SO.MIX_WEIGHTS[0]], ["B", SO.MIX_WEIGHTS[1]]]}
    handle = p.submit_batch([Image.fromarray(f, "RGB") for f in camera], prompts=["A", mix, "B"], height=H, width=W, steps=SO.STEPS,
                            strength=[s for s, _c in SO.OPTIONS], controlnet_scale=[c for _s, c in SO.OPTIONS], seed=list(SO.SEEDS),
                            masks=[Image.fromarray(m, "L") for m in masks])
    outs = np.stack([np.asarray(o) for o in p.collect_batch(handle)])
    used = handle.engine
    assert used.plan["keep_mask"] and used.plan["frame_options"] and used.plan["frame_prompts"] and used.plan["device_seed"] and used.plan["edge_mode"] == "canny"
    assert np.array_equal(used.mask_u8.cpu().numpy(), masks)
    # an engine of the same family, driven as case (d) is: the same bytes; and those are held to the stage oracle like (d)'s
    a, b = p._prompts["A"], p._prompts["B"]
    eng = p.model.make_slot(share_plan=False, lane=handle.lane)
    eng.tune_for_lanes = used.tune_for_lanes
    SO.prepare_case(eng, "all", H, W, (a, b, BK.PromptMix([a, b], SO.MIX_WEIGHTS)), autotune=False)
    got = SO.launch_case(eng, "all", camera)
    assert np.array_equal(outs, got), SO.mad(outs, got)
    _hold(eng, which, "all", H, W, got, "e")


# ------------------------------------------------------------------------------------------ f. two lanes in flight
def test_f_a_slot_in_flight_with_other_masks_seeds_and_options():
    which, H, W = "mini", 72, 120
    eng, got = _case(which, "all", H, W)
    camera, masks = SO.frames(H, W), SO.masks(H, W)
    blocks = _setup(which)[3]
    slot = eng.make_slot(lane=1)
    slot.use_prompts(list(SO.blocks_of_frames(blocks))[::-1])
    slot.prepare(H, W, SO.STEPS, SO.OPTIONS[0][0], controlnet_scale=SO.OPTIONS[0][1], use_controlnet=True, batch=SO.B, keep_mask=True, autotune=False,
                 **SO.CASES["all"])
    other_seeds = [7, 2 ** 33 + 1, 11]
    slot.use_options(list(SO.OPTIONS[::-1]))
    slot.set_masks(masks[::-1])
    slot.submit_u8(camera, seeds=other_seeds)
    alone = slot.collect_u8()
    assert not np.array_equal(alone, got) and np.array_equal(alone[masks[::-1] == 0], camera[masks[::-1] == 0])
    for _round in range(2):
        eng.submit_u8(camera, seeds=list(SO.SEEDS))
        slot.submit_u8(camera, seeds=other_seeds)  # both in flight, on two lanes
        assert np.array_equal(eng.collect_u8(), got)
        assert np.array_equal(slot.collect_u8(), alone)


# ------------------------------------------------------------------------------------------ g. with every uninitialised byte poisoned
def test_g_all_switches_with_poisoned_allocations():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VSD_POISON="1")
    res = subprocess.run([sys.executable, os.path.join(here, "poison_check_stages.py")], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(out) == {f"{W}x{H}" for _w, H, W in MINI_SHAPES}
    for (_which, H, W) in MINI_SHAPES:
        rows, bound = out[f"{W}x{H}"], SO.bound("all", H, W, "mini")
        print(f"poisoned {W}x{H}:", rows)
        assert len(rows) == SO.B
        for f in rows:
            assert f["r0"] <= SO.R0_MAX and f["r1"] <= bound and f["r1_mixed"] <= bound and f["lsb"] <= MAD_MAX and f["psnr"] >= PSNR_MIN and f["post_exact"], (f, bound)

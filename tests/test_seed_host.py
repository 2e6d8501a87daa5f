"""Per-frame seeded noise without a GPU: the numpy restatement of the noise contract (seed_cases.py) against the published Philox known
answers, the worker's coalescing of frames that differ only in `seed`, and the places the new entry points must appear in (plan entry
point ids, header, ctypes signatures)."""
import multiprocessing as mp
import os
import re
import sys
import threading

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seed_cases as SC  # noqa: E402
from helpers_fake_pipeline import FakePipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the contract's restatement
def test_restatement_reproduces_the_random123_known_answers():
    for ctr, key, want in SC.KNOWN_ANSWERS:
        got = tuple(int(v) for v in SC.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key, [hex(v) for v in got])
    # seed 0 / kind 0 / draw 0 / pixel 0 is the all-zero case; the key is (low, high) of the seed modulo 2^64
    assert tuple(int(v) for v in SC.raw_draw(0, 0, 0, 1)[0]) == SC.KNOWN_ANSWERS[0][2]
    assert SC.key_of(2 ** 32 + 5) == (5, 1) and SC.key_of(2 ** 64 - 1) == (SC.MASK, SC.MASK) and SC.key_of(2 ** 64 + 7) == (7, 0) and SC.key_of(-1) == SC.key_of(2 ** 64 - 1)
    # pixel i is counter word 0, the draw word 1, the kind word 2
    a = SC.raw_draw(42, 1, 4, 9)
    assert tuple(int(v) for v in a[7]) == tuple(int(v) for v in SC.philox4x32_10(7, 4, 1, 0, 42, 0))


def test_uniform_map_is_exact_in_fp32_and_open():
    x = np.array([0, 1, 511, 512, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    u = SC.uniform(x)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # every value is an fp32 number
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    z = SC.normal_draw(42, 0, 3, 4097)
    assert z.shape == (4, 4097) and np.isfinite(z).all() and np.abs(z).max() <= SC.Z_MAX
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05
    # a draw depends on (seed, kind, draw, pixel) alone: a longer draw starts with the shorter one
    assert np.array_equal(SC.normal_draw(42, 0, 3, 15), z[:, :15])
    assert not np.array_equal(SC.normal_draw(43, 0, 3, 15), z[:, :15]) and not np.array_equal(SC.normal_draw(42, 1, 3, 15), z[:, :15])


# ------------------------------------------------------------------------------------------ dispatch: frames that differ in `seed`
SUBMITS = []  # (frames in the launch, the `seed` it was given), per stand-in launch of this process


class SeedPipeline(FakePipeline):
    """stand-in that records its launches and writes every frame's seed into the frame it returns"""

    def submit_batch(self, imgs, lane=0, **opts):
        SUBMITS.append((len(imgs), opts.get("seed")))
        return super().submit_batch(imgs, lane=lane, **opts)

    def collect_batch(self, handle):
        outs = super().collect_batch(handle)
        seed = handle[2].get("seed")
        seeds = list(seed) if isinstance(seed, (list, tuple)) else [seed] * len(outs)
        res = []
        for o, s in zip(outs, seeds):
            a = np.asarray(o).copy()
            a[0, 1, 0] = s
            res.append(Image.fromarray(a, "RGB"))
        return res


class PerFrameSeedPipeline(SeedPipeline):
    per_frame_seed = True


def _serve(factory, seeds):
    """the worker loop in a thread of this process, with the three requests ALREADY queued when it starts -> (launches, replies)"""
    from videosd_amd.dispatch import _worker_main

    del SUBMITS[:]
    parent, child = mp.Pipe()
    for k, s in enumerate(seeds):
        img = Image.fromarray(np.full((12, 16, 3), 10 * (k + 1), np.uint8), "RGB")
        parent.send((k, "infer", (img,), dict(height=12, width=16, seed=s)))
    parent.send(None)
    t = threading.Thread(target=_worker_main, args=(child, factory, dict(model="m", controlnet="c", device=0)), kwargs=dict(max_batch=3))
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert parent.recv() == ("ready", None)
    replies = {}
    while parent.poll(0):
        rid, ok, payload = parent.recv()
        assert ok, payload
        replies[rid] = np.asarray(payload)
    return list(SUBMITS), replies


def test_frames_that_differ_only_in_seed_share_a_launch_when_the_pipeline_says_so():
    launches, replies = _serve("test_seed_host:PerFrameSeedPipeline", [7, 8, 9])
    assert launches == [(3, [7, 8, 9])], launches  # ONE launch, the seeds as a list in request order
    assert sorted(replies) == [0, 1, 2]
    for k, s in enumerate([7, 8, 9]):  # each reply is its request's frame (inverted by the stand-in) with its request's seed
        assert int(replies[k][1, 1, 0]) == 255 - 10 * (k + 1) and int(replies[k][0, 1, 0]) == s and int(replies[k][0, 0, 1]) == 3


def test_without_the_attribute_a_seed_change_is_another_launch_as_before():
    launches, replies = _serve("test_seed_host:SeedPipeline", [7, 8, 9])
    assert launches == [(1, 7), (1, 8), (1, 9)], launches  # three launches, `seed` as the caller gave it
    for k, s in enumerate([7, 8, 9]):
        assert int(replies[k][1, 1, 0]) == 255 - 10 * (k + 1) and int(replies[k][0, 1, 0]) == s
    # ... and equal seeds still coalesce, with `seed` untouched
    launches, _ = _serve("test_seed_host:SeedPipeline", [5, 5, 5])
    assert launches == [(3, 5)], launches


# ------------------------------------------------------------------------------------------ plan entry points, header, bindings
OLD_PLAN_FUNCS = ["vsd_preprocess_rgb", "vsd_sobel_control", "vsd_conv_gemm", "vsd_conv_gemm_group", "vsd_pair_begin", "vsd_pair_join",
                  "vsd_pair_end", "vsd_groupnorm", "vsd_groupnorm_batched", "vsd_attention", "vsd_attention_batched", "vsd_tail_a", "vsd_tail_b",
                  "vsd_add_noise_dev", "vsd_lcm_step_dev", "vsd_postprocess_rgb", "vsd_adain", "vsd_layernorm"]
NEW_SYMBOLS = ["vsd_noise_fill", "vsd_add_noise_seeded", "vsd_lcm_step_seeded", "vsd_plan_set_seeds"]


def test_plan_entry_points_keep_their_ids_and_the_seeded_ones_come_last():
    from videosd_amd import plan as P

    assert P.PLAN_FUNCS[:len(OLD_PLAN_FUNCS)] == OLD_PLAN_FUNCS
    assert P.PLAN_FUNCS[len(OLD_PLAN_FUNCS):] == ["vsd_add_noise_seeded", "vsd_lcm_step_seeded"]
    tags = dict(t.split(":") for t in P.signature_tags())
    assert tags["vsd_add_noise_seeded"] == "ppiipiipp" and tags["vsd_lcm_step_seeded"] == "pppiipiipppp"
    inc = open(os.path.join(ROOT, "videosd_amd", "csrc", "plan_dispatch.inc")).read()
    assert "case 18:" in inc and "vsd_add_noise_seeded(ctx" in inc and "case 19:" in inc and "vsd_lcm_step_seeded(ctx" in inc


def test_header_declares_the_new_symbols_as_the_binding_has_them():
    import ctypes as C

    from videosd_amd import lib as L

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int": C.c_int, "uint32_t": C.c_uint32, "void*": C.c_void_p, "const void*": C.c_void_p, "vsd_ctx*": C.c_void_p, "vsd_plan*": C.c_void_p,
             "const uint64_t*": C.POINTER(C.c_uint64)}
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        params = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        assert L.SIGNATURES[name] == (C.c_int, [ctype[p] for p in params]), (name, params)
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header
    assert "csrc/noise.hip" in open(os.path.join(ROOT, "include", "vsd.h")).read()
    from videosd_amd import build as B

    assert "noise.hip" in B.SOURCES


def test_device_seed_is_refused_by_name_on_an_ops_object_without_the_ops():
    import pytest

    from videosd_amd.engine import Engine

    class NoSeedOps:
        pass

    e = Engine.__new__(Engine)
    e.ops = NoSeedOps()
    with pytest.raises(ValueError, match="add_noise_seeded.*lcm_step_seeded"):
        e.prepare(96, 160, 2, 0.5, device_seed=True)


# ------------------------------------------------------------------------------------------ the engine's wiring, through the op emulator
def _seeded_fake_ops():
    import torch

    from fake_ops import FakeOps

    class SeededFakeOps(FakeOps):
        """the op emulator plus the two seeded ops, written from the contract: the restatement's draw, then the emulator's own `_dev` op"""

        @staticmethod
        def _draw(seeds_dev, b, kind, draw, hw):
            return torch.from_numpy(SC.normal_draw(int(seeds_dev[b]), kind, draw, hw)).float()

        def add_noise_seeded(self, x0, seeds_dev, kind, draw, coef_dev, hw, batch, out):
            for b in range(batch):
                self.add_noise_dev(x0[b * hw:(b + 1) * hw], self._draw(seeds_dev, b, kind, draw, hw), coef_dev, hw, 1, out[b * hw:(b + 1) * hw])

        def lcm_step_seeded(self, eps, sample, seeds_dev, kind, draw, coef_dev, hw, batch, prev, denoised, dec_in=None):
            sl = lambda t, b: None if t is None else t[b * hw:(b + 1) * hw]  # noqa: E731
            for b in range(batch):
                nz = self._draw(seeds_dev, b, kind, draw, hw) if draw > 0 else None
                self.lcm_step_dev(sl(eps, b), sl(sample, b), nz, coef_dev, hw, 1, sl(prev, b), sl(denoised, b), sl(dec_in, b))

        def clone(self, lane=None):
            return SeededFakeOps()

    return SeededFakeOps()


def test_engine_with_device_seed_records_the_seeded_ops_and_matches_the_oracle_given_the_draws(monkeypatch):
    import torch

    from oracle.pipeline import OraclePipeline
    from videosd_amd import config as Cf
    from videosd_amd import weights as Wt
    from videosd_amd.engine import Engine

    wu = Wt.synthesize(Wt.unet_spec(Cf.MINI_UNET), "unet.")
    wc = Wt.synthesize(Wt.controlnet_spec(Cf.MINI_CONTROLNET), "cn.")
    wv = Wt.synthesize(Wt.taesd_spec(Cf.TAESD), "vae.")
    text = (torch.randn(77, Cf.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half()
    H = W = 64
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    names = lambda e: [fn.__name__ for fn, _a, _k in Engine.flat_calls(e.program.calls)]  # noqa: E731
    eng = Engine(_seeded_fake_ops(), Cf.MINI_UNET, Cf.MINI_CONTROLNET, Cf.TAESD, wu, wc, wv)
    eng.set_text_embeds(text)
    eng.prepare(H, W, 2, 0.6, controlnet_scale=1.5, use_controlnet=True, use_graph=False, batch=2)
    default_names = names(eng)
    assert eng.plan["device_seed"] is False and eng.seed_dev is None and not any("seeded" in n for n in default_names)
    ff = np.stack([f, f])
    base = eng.infer_u8(ff)[0]
    import pytest

    with pytest.raises(ValueError, match="device_seed"):
        eng.submit_u8(ff, seeds=3)
    eng.prepare(H, W, 2, 0.6, controlnet_scale=1.5, use_controlnet=True, use_graph=False, batch=2, device_seed=True)
    assert eng.plan["device_seed"] is True and eng.noise is None and tuple(eng.seed_dev.shape) == (2,)
    swap = {"add_noise_dev": "add_noise_seeded", "lcm_step_dev": "lcm_step_seeded"}
    assert names(eng) == [swap.get(n, n) for n in default_names]
    assert default_names.count("add_noise_dev") == 1 and default_names.count("lcm_step_dev") == 2
    eng.submit_u8(ff, seeds=[23, 24])
    a = eng.collect_u8()
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], base)  # the frames differ in their seed alone
    eng.submit_u8(ff, seeds=[24, 23 + 2 ** 64])
    b = eng.collect_u8()
    assert np.array_equal(b[0], a[1]) and np.array_equal(b[1], a[0])  # (the emulator has no batch-position rounding)
    eng.submit_u8(ff)  # no seeds: those of the launch before
    assert np.array_equal(eng.collect_u8(), b)
    with pytest.raises(ValueError):
        eng.submit_u8(ff, seeds=[1, 2, 3])
    # the oracle, handed the contract's draws for seed 23 in call order
    calls = []

    def randn(*size, **kw):
        z = SC.normal_draw(23, 0, len(calls), (H // 8) * (W // 8)).reshape(1, 4, H // 8, W // 8)
        calls.append(size)
        return torch.from_numpy(z).to(kw.get("dtype") or torch.float32)

    orc = OraclePipeline(Cf.MINI_UNET, Cf.MINI_CONTROLNET, wu, wc, wv)
    with monkeypatch.context() as m:
        m.setattr(torch, "randn", randn)
        ref = np.asarray(orc.infer(Image.fromarray(f, "RGB"), text[None].float(), height=H, width=W, strength=0.6, steps=2, seed=23,
                                   controlnet_scale=1.5, use_controlnet=True))
    assert len(calls) == 3
    assert np.abs(a[0].astype(int) - ref.astype(int)).mean() < 1.5
    # a slot has seeds of its own
    slot = eng.make_slot()
    assert slot.seed_dev is None

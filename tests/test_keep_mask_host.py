"""Keep masks without a GPU: the host twins vsd_mask_blend_host / vsd_mask_latent_host / vsd_latent_keep_host against the numpy
restatement of THE KEEP MASK (include/vsd.h) to the bit on every case of tests/keep_mask_cases.py; what they refuse; header, binding
and build list; the engine's wiring of `keep_mask=` on the op emulator (backed by the twins); the class's `set_mask` and a worker.
The wiring tests here say which buffers each recorded call is handed; that the FRAME is the contract's frame (the right timestep, draw and
latents behind those pointers) is held per frame against the CPU oracle by tests/test_stage_oracle_host.py and tests/test_stage_oracle_gpu.py."""
import ctypes as Ct
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keep_mask_cases as KM  # noqa: E402
from fake_ops import FakeOps  # noqa: E402
from helpers_fake_pipeline import bare_pipeline  # noqa: E402

from videosd_amd import config as C  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"vsd_mask_blend": "keep_mask.hip", "vsd_mask_latent": "keep_mask.hip", "vsd_mask_blend_host": "keep_mask.hip",
           "vsd_mask_latent_host": "keep_mask.hip", "vsd_latent_keep": "noise.hip", "vsd_latent_keep_host": "noise.hip"}
VSD_ERR_ARG = -1


def _ptr(a):
    return None if a is None else a.ctypes.data


def blend_host(src, dst, mask):
    out = np.array(dst, dtype=np.uint8)
    f, h, w = mask.shape
    rc = L.load().vsd_mask_blend_host(_ptr(np.ascontiguousarray(src)), _ptr(out), _ptr(np.ascontiguousarray(mask)), f, h, w)
    return rc, out


def latent_host(mask):
    f, h, w = mask.shape
    out = np.full((f, (h // 8) * (w // 8)), -1.0, np.float32)
    return L.load().vsd_mask_latent_host(_ptr(np.ascontiguousarray(mask)), f, h, w, _ptr(out)), out


def keep_host(x0, wl, n0, coef, stride, hw, batch, lat=None, den=None):
    """-> (status, the new lat or den)"""
    out = np.array(lat if lat is not None else den, dtype=np.float16)
    c = [np.ascontiguousarray(a) if a is not None else None for a in (x0, wl, n0, coef)]
    rc = L.load().vsd_latent_keep_host(_ptr(c[0]), _ptr(c[1]), _ptr(c[2]), _ptr(c[3]), stride, hw, batch, _ptr(out) if lat is not None else None,
                                       _ptr(out) if den is not None else None)
    return rc, out


# ------------------------------------------------------------------------------------------ the host twins against the contract
@pytest.mark.parametrize("frames", KM.FRAME_COUNTS)
@pytest.mark.parametrize("shape", KM.BLEND_SHAPES)
def test_blend_host_equals_the_contract(shape, frames):
    src, dst = KM.frames_pair(frames, *shape)
    for kind in KM.MASK_KINDS:
        m = KM.mask(kind, frames, *shape)
        rc, got = blend_host(src, dst, m)
        assert rc == 0 and np.array_equal(got, KM.blend_numpy(src, dst, m)), (shape, frames, kind)
        if kind == "zeros":
            assert np.array_equal(got, src)
        if kind == "full":
            assert np.array_equal(got, dst)


def test_the_weight_is_256_at_255_alone():
    a = KM.weight(np.arange(256))
    assert a[0] == 0 and a[127] == 127 and a[128] == 129 and a[254] == 255 and a[255] == 256 and (np.diff(a) >= 1).all()


@pytest.mark.parametrize("frames", KM.FRAME_COUNTS)
@pytest.mark.parametrize("shape", KM.LATENT_SHAPES)
def test_latent_host_equals_the_contract(shape, frames):
    for kind in KM.MASK_KINDS:
        m = KM.mask(kind, frames, *shape)
        rc, got = latent_host(m)
        want = KM.latent_numpy(m)
        assert rc == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, frames, kind)
        if kind in ("zeros", "full"):
            assert (got == (1.0 if kind == "full" else 0.0)).all()
        assert np.array_equal(np.float32(1.0) - got, (1.0 - got.astype(np.float64)).astype(np.float32))  # 1 - wl is exact


@pytest.mark.parametrize("stride", KM.KEEP_STRIDES)
@pytest.mark.parametrize("batch", KM.KEEP_BATCH)
@pytest.mark.parametrize("hw", KM.KEEP_HW)
def test_latent_keep_host_equals_the_contract(hw, batch, stride):
    x0, lat, den, wl, n0, coef = KM.keep_case(hw, batch, stride)
    rc, got = keep_host(x0, wl, n0, coef, stride, hw, batch, lat=lat)
    want = KM.keep_step_numpy(x0, wl, n0, coef, stride, hw, batch, lat)
    assert rc == 0 and np.array_equal(got.view(np.uint16), want.view(np.uint16)), int((got.view(np.uint16) != want.view(np.uint16)).sum())
    rc, gotd = keep_host(x0, wl, None, None, 0, hw, batch, den=den)
    wantd = KM.keep_final_numpy(x0, wl, den)
    assert rc == 0 and np.array_equal(gotd.view(np.uint16), wantd.view(np.uint16))
    keep = wl == 1.0
    for a, b in ((got, lat), (gotd, den)):
        assert np.array_equal(a[keep].view(np.uint16), b[keep].view(np.uint16))  # untouched, -0.0 included
        assert np.array_equal(a[:, 4:].view(np.uint16), b[:, 4:].view(np.uint16))  # channels 4..7 stay
        if (~keep).any():
            assert not np.array_equal(a[~keep, :4].view(np.uint16), b[~keep, :4].view(np.uint16))
    zero = wl == 0.0
    assert np.array_equal(gotd[zero, :4].view(np.uint16) & 0x7FFF, x0[zero, :4].view(np.uint16) & 0x7FFF)  # wl = 0: x0 (fma(0, den, x0); the sign of a zero aside)


def test_fma32_is_a_correctly_rounded_fma():
    from fractions import Fraction

    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(4000).astype(np.float32), rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * rng.choice([1.0, 1.0 + 2.0 ** -20, 3.0], 4000).astype(np.float32)  # cancellation
    got = KM.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(exact))  # float(Fraction) rounds once to fp64 -- so compare against the fp32 neighbours exactly
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, got[i], best)


def test_bad_arguments_are_refused():
    lib = L.load()
    f = np.zeros((1, 8, 8, 3), np.uint8)
    m = np.zeros((1, 8, 8), np.uint8)
    out = np.zeros(64, np.float32)
    for frames, h, w in ((0, 8, 8), (1025, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8), (1, 16385, 8), (1, 8, 16385)):
        assert lib.vsd_mask_blend_host(_ptr(f), _ptr(f), _ptr(m), frames, h, w) == VSD_ERR_ARG, (frames, h, w)
        assert lib.vsd_mask_latent_host(_ptr(m), frames, h, w, _ptr(out)) == VSD_ERR_ARG, (frames, h, w)
    for h, w in ((7, 8), (8, 12), (1, 1), (4, 4), (9, 16)):  # sides that are not multiples of 8: the latent weight refuses, the blend does not
        assert lib.vsd_mask_latent_host(_ptr(m), 1, h, w, _ptr(out)) == VSD_ERR_ARG, (h, w)
    assert lib.vsd_mask_blend_host(_ptr(f), _ptr(f), _ptr(m), 1, 7, 5) == 0
    for args in ((None, _ptr(f), _ptr(m)), (_ptr(f), None, _ptr(m)), (_ptr(f), _ptr(f), None)):
        assert lib.vsd_mask_blend_host(*args, 1, 8, 8) == VSD_ERR_ARG
    assert lib.vsd_mask_latent_host(None, 1, 8, 8, _ptr(out)) == VSD_ERR_ARG and lib.vsd_mask_latent_host(_ptr(m), 1, 8, 8, None) == VSD_ERR_ARG
    x0, lat, den, wl, n0, coef = KM.keep_case(135, 1, 0)
    assert keep_host(x0, wl, None, coef, 0, 135, 1, lat=lat)[0] == VSD_ERR_ARG        # the step form without noise
    assert keep_host(x0, wl, n0, None, 0, 135, 1, lat=lat)[0] == VSD_ERR_ARG          # ... without coefficients
    assert keep_host(x0, wl, n0, coef, 3, 135, 1, lat=lat)[0] == VSD_ERR_ARG          # ... a stride below six
    assert keep_host(x0, wl, n0, coef, 0, 135, 1, den=den)[0] == VSD_ERR_ARG          # the final form with a noise source
    assert keep_host(x0, wl, n0, coef, 0, 0, 1, lat=lat)[0] == VSD_ERR_ARG and keep_host(x0, wl, n0, coef, 0, 135, 0, lat=lat)[0] == VSD_ERR_ARG
    c = [np.ascontiguousarray(a) for a in (x0, wl, n0, coef)]
    both = np.array(lat), np.array(den)
    assert lib.vsd_latent_keep_host(_ptr(c[0]), _ptr(c[1]), _ptr(c[2]), _ptr(c[3]), 0, 135, 1, _ptr(both[0]), _ptr(both[1])) == VSD_ERR_ARG  # both forms
    assert lib.vsd_latent_keep_host(_ptr(c[0]), _ptr(c[1]), None, None, 0, 135, 1, None, None) == VSD_ERR_ARG  # neither
    # the device entry points without a context
    assert lib.vsd_mask_blend(None, _ptr(f), _ptr(f), _ptr(m), 1, 8, 8, None) == VSD_ERR_ARG
    assert lib.vsd_mask_latent(None, _ptr(m), 1, 8, 8, _ptr(out), None) == VSD_ERR_ARG
    assert lib.vsd_latent_keep(None, _ptr(c[0]), _ptr(c[1]), _ptr(c[2]), None, 0, 0, _ptr(c[3]), 0, 135, 1, _ptr(both[0]), None, None, None) == VSD_ERR_ARG


# ------------------------------------------------------------------------------------------ header, binding, build list
def test_version_and_plan_functions_stay():
    from videosd_amd import plan as P

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header
    assert not [f for f in P.PLAN_FUNCS if "mask" in f or "keep" in f]


def test_header_binding_and_build_list_agree_on_the_six_symbols():
    from videosd_amd import build as Bd
    from videosd_amd.ops import HipOps

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert "THE KEEP MASK" in header and "#define VSD_MASK_MAX_FRAMES 1024" in header
    letter = {"void*": Ct.c_void_p, "vsd_ctx*": Ct.c_void_p, "float*": Ct.c_void_p, "int": Ct.c_int}
    for name, source in SYMBOLS.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        args = [letter[a.rsplit(" ", 1)[0].replace("const ", "")] for a in re.sub(r"\s+", " ", m.group(1)).split(", ")]
        res, sig = L.SIGNATURES[name]
        assert res is Ct.c_int and sig == args, name
        src = [f for f in Bd.SOURCES if re.search(r'extern "C" int ' + name + r"\(", open(os.path.join(Bd.CSRC, f)).read())]
        assert src == [source], (name, src)
        assert hasattr(L.load(), name)
    assert Bd.OWN_HEADERS["keep_mask.hip"] == ["keep_mask_core.h"] and "-ffp-contract=off" in Bd.EXTRA_FLAGS["keep_mask.hip"]
    assert os.path.exists(os.path.join(Bd.CSRC, "keep_mask_core.h"))
    for op in ("mask_blend", "mask_latent", "latent_keep"):
        assert callable(getattr(HipOps, op))


# ------------------------------------------------------------------------------------------ the engine's wiring, on the op emulator
class KeepFakeOps(FakeOps):
    """the op emulator with the three keep-mask ops backed by the host twins (and `dec_in` of the final form by the emulator's own
    expression for it); counts the uploads"""

    def __init__(self):
        super().__init__()
        self.uploads = []

    def clone(self, lane=None):
        return KeepFakeOps()

    def upload(self, dst, src):
        self.uploads.append(dst.data_ptr())
        super().upload(dst, src)

    def mask_blend(self, src_u8, dst_u8, mask_u8, frames, h, w):
        assert src_u8.dtype == dst_u8.dtype == mask_u8.dtype == torch.uint8 and mask_u8.numel() == frames * h * w
        assert L.load().vsd_mask_blend_host(src_u8.data_ptr(), dst_u8.data_ptr(), mask_u8.data_ptr(), frames, h, w) == 0

    def mask_latent(self, mask_u8, frames, h, w, weights_f32):
        assert weights_f32.dtype == torch.float32 and weights_f32.numel() == frames * (h // 8) * (w // 8)
        assert L.load().vsd_mask_latent_host(mask_u8.data_ptr(), frames, h, w, weights_f32.data_ptr()) == 0

    def color_match(self, src_u8, dst_u8, frames, h, w, mode, amounts_dev):
        pass  # (a stand-in: where the call stands in the program is what is checked)

    def latent_keep(self, x0, weights_f32, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, lat=None, den=None, dec_in=None):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        assert seeds_dev is None and weights_f32.numel() == batch * hw
        if noise_f32 is not None:
            noise_f32 = noise_f32.contiguous()
            assert noise_f32.dtype == torch.float32 and noise_f32.numel() == 4 * hw
        assert L.load().vsd_latent_keep_host(p(x0), p(weights_f32), p(noise_f32), p(coef_dev), coef_stride, hw, batch, p(lat), p(den)) == 0
        if dec_in is not None:
            dec_in.zero_()
            dec_in[:, :4] = (torch.tanh(den[:, :4].float() / 3.0) * 3.0).half()


def _calls(eng, serial=False):
    return list(Engine.flat_calls((eng.program_serial if serial else eng.program).calls))


def _names(eng, serial=False):
    return [fn.__name__ for fn, _a, _k in _calls(eng, serial)]


def _engine(ops):
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    eng = Engine(ops, C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def _without(names, inserted):
    """the call list with the calls at the indices `inserted` taken out"""
    return [n for i, n in enumerate(names) if i not in inserted]


H, Wd, B, STEPS = 64, 64, 3, 2
PREP = dict(batch=B, use_controlnet=True, use_graph=False)


@pytest.fixture(scope="module")
def eng():
    return _engine(KeepFakeOps())


@pytest.fixture(scope="module")
def plain(eng):
    frames = np.random.default_rng(3).integers(0, 256, (B, H, Wd, 3), dtype=np.uint8)
    plan = eng.prepare(H, Wd, STEPS, 1.0, **PREP)
    assert plan["keep_mask"] is False and eng.mask_u8 is None and plan["n"] == STEPS
    names = _names(eng)
    assert not [n for n in names if "mask" in n or "keep" in n]
    with pytest.raises(ValueError, match="set_masks needs"):
        eng.set_masks(None)
    return frames, eng.infer_u8(frames).copy(), names, _names(eng, serial=True)


def test_prepare_inserts_the_calls_at_the_stated_places(eng, plain, tmp_path):
    frames, base, plain_names, plain_serial = plain
    plan = eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, **PREP)
    assert plan["keep_mask"] is True and tuple(eng.mask_u8.shape) == (B, H, Wd) and tuple(eng.mask_w.shape) == (B, 64)
    assert bool((eng.mask_u8 == 255).all()) and bool((eng.mask_w == 1.0).all())  # all 255 until `set_masks`, sent and weighed by the warm-up run
    for serial, want in ((False, plain_names), (True, plain_serial)):
        names = _names(eng, serial)
        at = {k: [i for i, n in enumerate(names) if n == k] for k in ("mask_latent", "latent_keep", "mask_blend")}
        assert [len(at[k]) for k in at] == [1, STEPS + 1, 1]
        assert _without(names, set(sum(at.values(), []))) == want  # exactly those inserted, nothing else moved
        steps = [i for i, n in enumerate(names) if n.startswith("lcm_step")]
        assert len(steps) == STEPS and at["latent_keep"] == [s + 1 for s in steps] + [steps[-1] + 2]  # right behind every step; the final form last
        assert names[at["mask_latent"][0] - 1].startswith("add_noise") and at["mask_latent"][0] < steps[0]
        assert names[at["mask_blend"][0] - 1] == "postprocess_rgb" and at["mask_blend"][0] == len(names) - 1
    calls = _calls(eng)
    names = _names(eng)
    x0, lat, den, dec_in = (eng.buffers[k] for k in ("x0", "lat", "denoised", "dec_in"))
    keeps = [calls[i] for i, n in enumerate(names) if n == "latent_keep"]
    step_calls = [calls[i] for i, n in enumerate(names) if n.startswith("lcm_step")]
    for i, (_fn, a, _k) in enumerate(keeps[:-1]):  # the step form: the step's own coefficients, table draw 0, the sample that step wrote
        st = step_calls[i][1]
        assert a[0] is x0 and a[1] is eng.mask_w and a[2].data_ptr() == eng.noise[0].data_ptr() and a[3] is None and a[4:6] == (0, 0)
        assert a[6].data_ptr() == st[3].data_ptr() and a[7] == 0 and a[8:10] == (64, B)
        assert a[10].data_ptr() == st[6].data_ptr() == lat[(i + 1) & 1].data_ptr() and a[11] is None and a[12] is None
    a = keeps[-1][1]  # the final form
    assert a[0] is x0 and a[1] is eng.mask_w and a[2] is None and a[3] is None and a[6] is None and a[10] is None and a[11] is den and a[12] is dec_in
    _fn, a, _k = calls[names.index("mask_latent")]
    assert a[0] is eng.mask_u8 and a[1:4] == (B, H, Wd) and a[4] is eng.mask_w
    _fn, a, _k = calls[names.index("mask_blend")]
    assert a[0].data_ptr() == eng.frame_u8.data_ptr() and a[1].data_ptr() == eng.out_u8.data_ptr() and a[2] is eng.mask_u8 and a[3:] == (B, H, Wd)
    # all 255: the default program's frames; all 0: the camera's frames and the input's latents
    assert np.array_equal(eng.infer_u8(frames), base)
    eng.set_masks(np.zeros((H, Wd), np.uint8))
    assert np.array_equal(eng.infer_u8(frames), frames)
    assert np.array_equal(den[:, :4].numpy().view(np.uint16) & 0x7FFF, x0[:, :4].numpy().view(np.uint16) & 0x7FFF)
    # mixed masks: the output is the blend of the camera's frame into what the program decoded (whatever that is), per frame
    masks = KM.engine_masks(B, H, Wd)
    program = eng.program
    eng.set_masks(masks)
    got = eng.infer_u8(frames)
    assert eng.program is program and not np.array_equal(got, base) and not np.array_equal(got, frames)
    assert np.array_equal(eng.mask_w.numpy(), KM.latent_numpy(masks))
    kept = masks == 0
    assert np.array_equal(got[kept], frames[kept])
    from videosd_amd.plan import export_plan

    with pytest.raises(ValueError, match="keep_mask=True"):
        export_plan(eng, str(tmp_path / "x.vsdplan"))


def test_with_color_match_the_blend_follows_it(eng):
    eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, color_match="histogram", **PREP)
    assert _names(eng)[-3:] == ["postprocess_rgb", "color_match", "mask_blend"] and _names(eng, serial=True)[-2:] == ["color_match", "mask_blend"]


def test_a_shorter_schedule_and_no_controlnet(eng):
    plan = eng.prepare(H, Wd, 4, 0.5, keep_mask=True, batch=1, use_controlnet=False, use_graph=False)
    names = _names(eng)
    assert names.count("latent_keep") == plan["n"] + 1 == len([n for n in names if n.startswith("lcm_step")]) + 1 and names[-1] == "mask_blend"


def test_prepare_names_the_missing_op_and_refuses_ref_mode_and_sdxl(eng, monkeypatch):
    e = Engine.__new__(Engine)
    e.ops = FakeOps()
    with pytest.raises(ValueError, match="keep_mask=True needs the op.*mask_latent, latent_keep, mask_blend"):
        e.prepare(64, 64, 2, 0.5, keep_mask=True)

    class Partial(FakeOps):
        mask_blend = mask_latent = lambda self, *a: None

    e.ops = Partial()
    with pytest.raises(ValueError, match=r"needs the op\(s\) latent_keep,"):
        e.prepare(64, 64, 2, 0.5, keep_mask=True)
    with pytest.raises(ValueError, match="keep_mask=True: reference-only"):
        eng.prepare(H, Wd, 2, 0.6, use_controlnet=False, ref_mode=True, use_graph=False, keep_mask=True)
    monkeypatch.setattr(eng.unet, "add_l1", object())  # (what makes a UNet an SDXL one to `prepare`)
    with pytest.raises(ValueError, match="keep_mask=True: .*SDXL"):
        eng.prepare(H, Wd, 2, 0.6, keep_mask=True, **PREP)


def test_set_masks_checks_and_uploads_only_on_change(eng):
    ops = eng.ops
    ops.uploads.clear()
    eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, **PREP)
    sent = lambda: ops.uploads.count(eng.mask_u8.data_ptr())  # noqa: E731
    assert sent() == 1  # the all-255 masks, ahead of the warm-up run
    eng.launch()
    eng.set_masks(None)  # what is there already
    eng.launch()
    assert sent() == 1
    one = KM.engine_masks(1, H, Wd)[0]
    eng.set_masks(one)
    assert sent() == 1 and bool((eng.mask_u8 == 255).all())  # only noted: the next launch sends it
    eng.launch()
    assert sent() == 2 and np.array_equal(eng.mask_u8.numpy(), np.broadcast_to(one, (B, H, Wd)))
    eng.set_masks(one.copy())  # the same bytes again
    eng.set_masks([one] * B)
    eng.launch()
    assert sent() == 2
    per_frame = KM.engine_masks(B, H, Wd)
    eng.set_masks(list(per_frame))
    per_frame_sent = per_frame.copy()
    per_frame[:] = 7  # (the caller's array afterwards: the engine kept a copy)
    eng.launch()
    assert sent() == 3 and np.array_equal(eng.mask_u8.numpy(), per_frame_sent)
    for bad in (np.zeros((H, Wd), np.float32), np.zeros((H, Wd + 8), np.uint8), np.zeros((B + 1, H, Wd), np.uint8), [one] * (B - 1),
                [one, one, one[:8]], np.zeros((H, Wd, 3), np.uint8), [one, one, one.astype(np.int32)]):
        with pytest.raises(ValueError, match="mask"):
            eng.set_masks(bad)
    eng.launch()
    assert sent() == 3  # a refused call changes nothing
    slot = eng.make_slot()
    slot.prepare(H, Wd, STEPS, 1.0, keep_mask=True, **PREP)
    assert slot.mask_u8.data_ptr() != eng.mask_u8.data_ptr() and bool((slot.mask_u8 == 255).all())  # a slot has masks of its own


# ------------------------------------------------------------------------------------------ the class, before any device work
def test_set_mask_sizes_the_mask_as_a_frame_is_sized(tmp_path):
    import inspect

    from videosd_amd.dispatch import PER_FRAME
    from videosd_amd.pipeline import INFER_DEFAULTS, VideoSDPipeline, center_crop_resize

    with pytest.raises(ValueError, match="set_mask needs"):
        bare_pipeline().set_mask(None)
    with pytest.raises(ValueError, match="masks= .* needs a pipeline built with keep_mask=True"):
        bare_pipeline()._launch_masks([None], 1, 64, 64)
    p = VideoSDPipeline.__new__(VideoSDPipeline)
    p._init_state(dict(keep_mask=True))
    assert p.keep_mask is True and p._launch_masks(None, 2, 64, 64) == (0, None)
    rng = np.random.default_rng(2)
    big = Image.fromarray(rng.integers(0, 256, (96, 128), dtype=np.uint8), "L")  # 128 x 96, as a camera's picture
    assert p.set_mask(big) == 1
    for width, height in ((64, 64), (48, 80), (128, 96)):
        epoch, m = p._launch_masks(None, 1, width, height)
        want = np.asarray(center_crop_resize(big, width, height))
        assert epoch == 1 and m.dtype == np.uint8 and np.array_equal(m, want) and m.shape == (height, width)
        # ... which is how a frame with the mask in every channel is sized
        rgb = np.asarray(center_crop_resize(Image.merge("RGB", [big] * 3), width, height))
        assert np.array_equal(rgb[..., 0], m)
        assert p._launch_masks(None, 1, width, height)[1] is m  # sized once per size and mask
    assert np.array_equal(p._launch_masks(None, 1, 128, 96)[1], np.asarray(big))
    m = p._launch_masks(None, 1, 70, 52)[1]  # not a multiple of 8: the second step down, as `_launch_frames` does
    assert m.shape == (48, 64) and np.array_equal(m, np.asarray(center_crop_resize(big, 70, 52).resize((64, 48), resample=Image.Resampling.LANCZOS)))
    # an array and a "1" image are taken as well; None goes back to everything restyled
    assert p.set_mask(np.asarray(big)) == 2 and p._mask_sized == {} and np.array_equal(p._launch_masks(None, 1, 128, 96)[1], np.asarray(big))
    one = Image.fromarray(np.asarray(big) > 127)
    assert one.mode == "1" and p.set_mask(one) == 3 and set(np.unique(p._launch_masks(None, 1, 128, 96)[1])) == {0, 255}
    assert p.set_mask(None) == 4 and p._launch_masks(None, 1, 64, 64) == (4, None)
    for bad in (Image.new("RGB", (8, 8)), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.float32), "mask.png", np.zeros((0, 8), np.uint8)):
        with pytest.raises(ValueError, match="mask"):
            p.set_mask(bad)
    assert p._mask_epoch == 4
    # per-frame masks of a launch: one per frame, any size, None = restyled whole
    ms = p._launch_masks([big, None, np.zeros((10, 10), np.uint8)], 3, 64, 64)
    assert len(ms) == 3 and np.array_equal(ms[0], np.asarray(center_crop_resize(big, 64, 64))) and (ms[1] == 255).all() and (ms[2] == 0).all()
    with pytest.raises(ValueError, match="one mask per frame"):
        p._launch_masks([big], 2, 64, 64)
    # no plan files, by name; `infer` keeps the reference's signature and no per-request option came with the switch
    with pytest.raises(ValueError, match="export_plan: .*keep_mask=True"):
        p.export_plan(str(tmp_path / "x.vsdplan"))
    with pytest.raises(ValueError, match="export_prompt: .*keep_mask=True"):
        p.export_prompt(str(tmp_path / "x.vsdprompt"), "a prompt")
    assert not [k for k in INFER_DEFAULTS if "mask" in k] and not [r for r in PER_FRAME if "mask" in repr(r)]
    assert "mask" not in str(inspect.signature(VideoSDPipeline.infer))
    assert "masks" in inspect.signature(VideoSDPipeline.infer_batch).parameters and "masks" in inspect.signature(VideoSDPipeline.submit_batch).parameters


def test_install_hands_an_engine_the_mask_once_per_change():
    from videosd_amd.pipeline import PlanKey

    class Eng:
        color_a, _mask_pipe_epoch, _ref_epoch = (), None, 0

        def __init__(self):
            self.got = []

        use_prompt = use_prompts = lambda self, p: None

        def set_masks(self, m):
            self.got.append(m)

    p = bare_pipeline(keep_mask=True)
    key = PlanKey(64, 64, 2, 2, True, False)
    e = Eng()
    p._install(e, key, None, [(0.5, 1.0)], p._launch_masks(None, 1, 64, 64))
    p._install(e, key, None, [(0.5, 1.0)], p._launch_masks(None, 1, 64, 64))
    assert e.got == [None]  # a new engine takes the state once
    p.set_mask(np.zeros((4, 4), np.uint8))
    p._install(e, key, None, [(0.5, 1.0)], p._launch_masks(None, 1, 64, 64))
    p._install(e, key, None, [(0.5, 1.0)], p._launch_masks(None, 1, 64, 64))
    assert len(e.got) == 2 and e.got[1].shape == (64, 64) and not e.got[1].any()
    own = p._launch_masks([None], 1, 64, 64)
    p._install(e, key, None, [(0.5, 1.0)], own)  # a launch's own masks ...
    p._install(e, key, None, [(0.5, 1.0)], p._launch_masks(None, 1, 64, 64))  # ... and `set_mask`'s again behind it
    assert len(e.got) == 4 and e.got[2] is own and e.got[3] is e.got[1]
    p2 = bare_pipeline()
    p2._install(e, key, None, [(0.5, 1.0)], p2._launch_masks(None, 1, 64, 64))  # without the switch nothing is called
    assert len(e.got) == 4


def test_a_worker_takes_set_mask_between_frames():
    """`VideoSDPipeline.remote(...).set_mask`: the call reaches the worker's object in order with the frames around it (it runs alone, after
    the launches in flight), returns what the object returns, and a refusal comes back as the caller's ValueError"""
    import asyncio

    from videosd_amd.dispatch import RemotePipeline

    img = Image.fromarray(np.full((12, 16, 3), 10, np.uint8), "RGB")
    p = RemotePipeline(factory="keep_mask_cases:KeepFakePipeline", model="m", controlnet="c", device=1, delay=0.02, batch=2, lanes=2)
    try:
        async def go():
            first = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            change = p.set_mask.remote(Image.new("L", (40, 30), 64))
            later = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            return [await f for f in first], await change, [await f for f in later]

        first, answer, later = asyncio.run(go())
        assert answer == 1
        assert [int(np.asarray(o)[0, 0, 2]) for o in first] == [255] * 4 and [int(np.asarray(o)[0, 0, 2]) for o in later] == [64] * 4
        assert p.set_mask(np.full((5, 7), 200, np.uint8)) == 2 and int(np.asarray(p.infer(img, height=12, width=16))[0, 0, 2]) == 200
        with pytest.raises(ValueError, match="mask"):
            p.set_mask("nonsense")
        assert p.set_mask(None) == 3 and int(np.asarray(p.infer(img, height=12, width=16))[0, 0, 2]) == 255
    finally:
        p.close()

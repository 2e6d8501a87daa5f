"""The device Gaussian blur without a GPU: `gauss_taps` / `check_taps` (videosd_amd/blur.py); the host twin vsd_gauss_blur_host against
the numpy restatement of THE BLUR CONTRACT (include/vsd.h) byte for byte on every case of tests/blur_cases.py; the contract's
consequences (identity, constant images, any split of the frames); header, binding and build list; the engine's wiring of `edge_blur=`
and `mask_feather=` on the op emulator; the class's setters and a worker.

The recorded default programs are compared with tests/golden/program_fingerprints_before_color_match.txt, as
tests/test_color_match_host.py does."""
import ctypes as Ct
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import blur_cases as BC  # noqa: E402
import keep_mask_cases as KM  # noqa: E402
from fake_ops import FakeOps  # noqa: E402
from helpers_fake_pipeline import bare_pipeline  # noqa: E402

from videosd_amd import blur as BL  # noqa: E402
from videosd_amd import config as C  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSD_ERR_ARG = -1


def blur_host(src, taps, skews=(0, 0)):
    """vsd_gauss_blur_host with src / dst `skews` bytes past a 16-byte boundary -> (status, dst)"""
    f, h, w, c = src.shape
    n = src.size
    bufs = []
    for k in skews:
        raw = np.full(n + 32, 0xC3, np.uint8)
        start = (-raw.ctypes.data) % 16 + k
        bufs.append((raw, start))
    (sraw, s0), (draw, d0) = bufs
    sraw[s0:s0 + n] = src.reshape(-1)
    t = np.ascontiguousarray(taps, dtype=np.int32)
    rc = L.load().vsd_gauss_blur_host(sraw.ctypes.data + s0, draw.ctypes.data + d0, f, h, w, c, t.ctypes.data)
    assert (draw[:d0] == 0xC3).all() and (draw[d0 + n:] == 0xC3).all() and np.array_equal(sraw[s0:s0 + n], src.reshape(-1))
    return rc, draw[d0:d0 + n].reshape(src.shape).copy()


# ------------------------------------------------------------------------------------------ tap tables
def test_gauss_taps_sum_exactly_over_a_sigma_grid():
    for k in range(5, 1001):  # 0.05 .. 10.00 in steps of 0.01
        s = k / 100.0
        t = BL.gauss_taps(s)
        R = int(t[0])
        assert t.dtype == np.int32 and t.shape == (34,) and R == max(1, int(np.ceil(3 * s))) <= 30
        assert int(t[1]) + 2 * int(t[2:].sum()) == 16384 and (t[1:] >= 0).all() and not t[2 + R:].any(), s
        assert np.array_equal(BL.check_taps(t), t)


def test_gauss_taps_identity_pinned_tables_and_refusals():
    ident = BL.gauss_taps(0)
    assert ident.tolist() == [1, 16384] + [0] * 32 and np.array_equal(BL.gauss_taps(0.0), ident)
    assert BL.gauss_taps(1.4).tolist() == [5, 4668, 3618, 1683, 470, 79, 8] + [0] * 27
    assert BL.gauss_taps(4.0).tolist() == [12, 1636, 1587, 1445, 1236, 993, 749, 531, 354, 222, 130, 72, 37, 18] + [0] * 20
    assert [int(BL.gauss_taps(s)[0]) for s in (0.5, 1.4, 4.0, 10.0)] == [2, 5, 12, 30]
    for bad in (-0.1, 10.01, float("nan"), float("inf"), -1, "wide", None, True):
        with pytest.raises(ValueError, match=r"sigma must be a number in \[0, 10\].*not " + re.escape(repr(bad))):
            BL.gauss_taps(bad)


def test_check_taps_refuses_every_single_rule_violation():
    good = BL.gauss_taps(1.4)
    lib = L.load()
    src = np.zeros((1, 4, 4, 1), np.uint8)

    def refused(t, text):
        with pytest.raises(ValueError, match=text):
            BL.check_taps(t)
        if np.asarray(t).shape == (34,) and np.asarray(t).dtype == np.int32:  # the host twin applies the same rules
            assert blur_host(src, t)[0] == VSD_ERR_ARG

    for r in (0, -1, 33):
        t = good.copy()
        t[0] = r
        refused(t, "radius must be 1..32")
    t = good.copy()
    t[3], t[1] = -1, t[1] + 2
    refused(t, "must not be negative")
    t = good.copy()
    t[1 + 6], t[1] = 1, t[1] - 2  # the sum still holds; the tap lies beyond R = 5
    refused(t, "beyond its radius 5 must be 0")
    for d in (1, -1):
        t = good.copy()
        t[1] += d
        refused(t, "must sum to 16384 exactly")
    refused(good[:33], "34 integers")
    refused(good.astype(np.float32), "34 integers")
    assert blur_host(src, good)[0] == 0 and lib.vsd_gauss_blur_host(None, None, 1, 4, 4, 1, good.ctypes.data) == VSD_ERR_ARG
    for f, h, w, c in ((0, 4, 4, 1), (1025, 1, 1, 1), (1, 0, 4, 1), (1, 4, 16385, 1), (1, 4, 4, 2), (1, 4, 4, 4)):
        assert lib.vsd_gauss_blur_host(src.ctypes.data, src.ctypes.data, f, h, w, c, good.ctypes.data) == VSD_ERR_ARG
    assert lib.vsd_gauss_blur(None, src.ctypes.data, src.ctypes.data, 1, 4, 4, 1, good.ctypes.data, None) == VSD_ERR_ARG  # no context


# ------------------------------------------------------------------------------------------ the host twin against the contract
@pytest.mark.parametrize("channels", BC.CHANNELS)
@pytest.mark.parametrize("shape", BC.SHAPES)
def test_host_twin_equals_the_contract(shape, channels):
    turn = 0
    for frames in BC.FRAME_COUNTS:
        for name, taps in BC.TAP_SETS.items():
            for content in BC.CONTENTS:
                src, want = BC.image(content, frames, *shape, channels), BC.expected(content, frames, *shape, channels, name)
                skews = [(a, b) for a in BC.SKEWS for b in BC.SKEWS]
                # (the host loops do not look at addresses: every case at one pair of bases, the pairs taking turns; the random image at all four)
                for sk in (skews if content == "random" else [skews[turn % 4]]):
                    rc, got = blur_host(src, taps, sk)
                    assert rc == 0 and np.array_equal(got, want), (shape, channels, frames, name, content, sk, int((got != want).sum()))
                turn += 1
                if name == "identity":
                    assert np.array_equal(want, src)
                if content == "full":
                    assert (want == 255).all()


def test_a_constant_image_stays_constant_and_the_frames_may_be_split_anyhow():
    for v in (0, 1, 127, 255):
        src = np.full((1, 9, 11, 3), v, np.uint8)
        for name, taps in BC.TAP_SETS.items():
            assert (BC.blur_numpy(src, taps) == v).all() and (blur_host(src, taps)[1] == v).all(), (v, name)
    src, taps = BC.image("random", 3, 31, 33, 3), BC.TAP_SETS["s4.0"]
    whole = blur_host(src, taps)[1]
    parts = np.concatenate([blur_host(src[:1], taps)[1], blur_host(src[1:], taps)[1]])
    assert np.array_equal(whole, parts) and np.array_equal(whole, BC.expected("random", 3, 31, 33, 3, "s4.0"))
    # a column of 70 with 255 at both ends, only the taps 32 away: row y reads rows clamp(y - 32) and clamp(y + 32), so rows 0..32 reach the
    # top corner, rows 37..69 the bottom one (half of 255, rounded up) and rows 33..36 neither
    far = BC.blur_numpy(BC.image("corners", 1, 70, 1, 1), BC.TAP_SETS["far32"]).reshape(-1)
    assert far.tolist() == [128] * 33 + [0] * 4 + [128] * 33


# ------------------------------------------------------------------------------------------ header, binding, build list, tile
def test_header_binding_build_list_and_tile_constants_agree():
    from videosd_amd import build as Bd
    from videosd_amd import plan as P
    from videosd_amd.ops import HipOps

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert "THE BLUR CONTRACT" in header and "#define VSD_BLUR_MAX_RADIUS 32" in header and "#define VSD_BLUR_ONE 16384" in header
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header and not [f for f in P.PLAN_FUNCS if "blur" in f]
    letter = {"void*": Ct.c_void_p, "vsd_ctx*": Ct.c_void_p, "int32_t*": Ct.c_void_p, "int": Ct.c_int}
    for name in ("vsd_gauss_blur", "vsd_gauss_blur_host"):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        args = [letter[a.strip().rsplit(" ", 1)[0].replace("const ", "")] for a in re.sub(r"\s+", " ", decl).split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is Ct.c_int and sig == args, name
        src = [f for f in Bd.SOURCES if re.search(r'extern "C" int ' + name + r"\(", open(os.path.join(Bd.CSRC, f)).read())]
        assert src == ["blur.hip"] and hasattr(L.load(), name)
    assert Bd.OWN_HEADERS["blur.hip"] == ["blur_core.h"] and callable(HipOps.gauss_blur)
    core = open(os.path.join(Bd.CSRC, "blur_core.h")).read()
    m = re.search(r"constexpr int BLUR_TILE_W = (\d+), BLUR_TILE_H = (\d+);", core)
    assert (int(m.group(1)), int(m.group(2))) == (BL.TILE_W, BL.TILE_H) == (BC.TILE_W, BC.TILE_H)
    assert (BL.TILE_H, BL.TILE_W) in BC.SHAPES and (BL.TILE_H - 1, BL.TILE_W - 1) in BC.SHAPES and (BL.TILE_H + 1, BL.TILE_W + 1) in BC.SHAPES
    assert (BL.TILE_H + 2 * BL.MAX_RADIUS) * BL.TILE_W * 2 <= 64 * 1024  # the LDS image, sized for R = 32
    assert (BL.MAX_RADIUS, BL.ONE, BL.TAPS) == (32, 16384, 34)


# ------------------------------------------------------------------------------------------ the engine's wiring, on the op emulator
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


H, Wd, B, STEPS = 64, 64, 3, 2
PREP = dict(batch=B, use_controlnet=True, use_graph=False)


@pytest.fixture(scope="module")
def eng():
    return _engine(BC.BlurFakeOps())


def test_the_default_programs_are_those_of_the_commit_before(monkeypatch):
    """both switches None: the emulator's fingerprints of every default program of scripts/program_fingerprint.py, against the listing
    that script wrote before any of the opt-in stages existed"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import program_fingerprint as pf

    golden = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "program_fingerprints_before_color_match.txt")):
        m = re.match(r"^(.*?)\s+([0-9a-f]{24})  calls (\d+) / (\d+)$", line.rstrip("\n"))
        golden[m.group(1)] = (m.group(2), int(m.group(3)), int(m.group(4)))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (on the emulator also where there is a GPU: the listing was recorded on it)
    weights, texts = pf.inputs()
    got = {cfg[0]: pf.fingerprint(pf.build(*cfg, weights, texts, use_graph=False, autotune=False)) for cfg in pf.configurations()}
    assert got == golden


@pytest.mark.parametrize("mode", ["canny", "sobel"])
def test_edge_blur_adds_one_call_that_feeds_the_edge_ops_alone(eng, mode):
    frames = BC.camera(H, Wd)
    plan = eng.prepare(H, Wd, STEPS, 1.0, edges=mode, **PREP)
    assert plan["edge_blur"] is False and plan["mask_feather"] is False and eng.taps == {} and eng.blur_u8 is None
    plain, plain_serial = _names(eng), _names(eng, serial=True)
    assert "gauss_blur" not in plain
    for setter in (eng.set_edge_blur, eng.set_mask_feather):
        with pytest.raises(ValueError, match="needs an engine prepared with (edge_blur|mask_feather)="):
            setter(1.0)
    base_x0 = None
    eng.infer_u8(frames)
    base_x0 = eng.buffers["x0"].clone()
    eng.infer_u8(BC.blur_numpy(frames, BL.gauss_taps(1.4)))
    want_edge, want_ctrl = eng.edge_u8.clone(), eng.buffers["control"].clone()
    plan = eng.prepare(H, Wd, STEPS, 1.0, edges=mode, edge_blur=1.4, **PREP)
    assert plan["edge_blur"] is True and plan["mask_feather"] is False and tuple(eng.blur_u8.shape) == (B, H, Wd, 3)
    assert np.array_equal(eng.taps["edge_blur"].dev.numpy(), BL.gauss_taps(1.4))  # sent ahead of the warm-up run
    op = mode + "_control"
    for serial, want in ((False, plain), (True, plain_serial)):
        names = _names(eng, serial)
        at = [i for i, n in enumerate(names) if n == "gauss_blur"]
        assert len(at) == 1 and [n for i, n in enumerate(names) if i != at[0]] == want  # today's program plus exactly one call
        assert names[at[0] + 1] == op and names.index("preprocess_rgb") < at[0]  # right ahead of the first edge op
    calls, names = _calls(eng), _names(eng)
    _fn, a, _k = calls[names.index("gauss_blur")]
    assert a[0].data_ptr() == eng.frame_u8.data_ptr() and a[1] is eng.blur_u8 and a[2:6] == (B, H, Wd, 3) and a[6] is eng.taps["edge_blur"].dev
    edge_calls = [c for c, n in zip(calls, names) if n == op]
    assert [c[1][0].data_ptr() for c in edge_calls] == [eng.blur_u8[b].data_ptr() for b in range(B)]
    for n in ("preprocess_rgb", "postprocess_rgb"):  # ... and nobody else reads the blurred copy
        assert all(getattr(t, "data_ptr", lambda: 0)() != eng.blur_u8.data_ptr() for t in calls[names.index(n)][1])
    _fn, a, _k = calls[names.index("preprocess_rgb")]
    assert a[0].data_ptr() == eng.frame_u8.data_ptr()
    eng.infer_u8(frames)
    assert torch.equal(eng.edge_u8, want_edge) and torch.equal(eng.buffers["control"], want_ctrl) and torch.equal(eng.buffers["x0"], base_x0)
    assert np.array_equal(eng.blur_u8.numpy(), BC.blur_numpy(frames, BL.gauss_taps(1.4)))


def test_edge_blur_without_a_controlnet_is_inert(eng):
    plan = eng.prepare(H, Wd, STEPS, 1.0, edge_blur=2.0, batch=1, use_controlnet=False, use_graph=False)
    assert plan["edge_blur"] is True and "gauss_blur" not in _names(eng) and eng.blur_u8 is None
    eng.set_edge_blur(1.0)  # accepted all the same
    eng.launch()


def test_mask_feather_adds_one_call_ahead_of_mask_latent(eng, tmp_path):
    frames, masks = BC.camera(H, Wd), KM.engine_masks(B, H, Wd)
    soft = BC.blur_numpy(masks, BL.gauss_taps(4.0))
    assert not np.array_equal(soft, masks)
    eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, **PREP)
    plain, plain_serial = _names(eng), _names(eng, serial=True)
    eng.set_masks(soft)
    want = eng.infer_u8(frames).copy()
    want_w = eng.mask_w.clone()
    plan = eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, mask_feather=4.0, **PREP)
    assert plan["mask_feather"] is True and plan["edge_blur"] is False and tuple(eng.mask_soft.shape) == (B, H, Wd)
    for serial, names_before in ((False, plain), (True, plain_serial)):
        names = _names(eng, serial)
        at = [i for i, n in enumerate(names) if n == "gauss_blur"]
        assert len(at) == 1 and [n for i, n in enumerate(names) if i != at[0]] == names_before and names[at[0] + 1] == "mask_latent"
    calls, names = _calls(eng), _names(eng)
    _fn, a, _k = calls[names.index("gauss_blur")]
    assert a[0] is eng.mask_u8 and a[1] is eng.mask_soft and a[2:6] == (B, H, Wd, 1) and a[6] is eng.taps["mask_feather"].dev
    assert calls[names.index("mask_latent")][1][0] is eng.mask_soft and calls[names.index("mask_blend")][1][2] is eng.mask_soft
    assert bool((eng.mask_soft == 255).all())  # all 255 until `set_masks`: the soft mask of the warm-up run is all 255 too
    program = eng.program
    eng.set_masks(masks)
    got = eng.infer_u8(frames)
    assert eng.program is program and np.array_equal(eng.mask_u8.numpy(), masks)  # the caller's mask is uploaded untouched
    assert np.array_equal(eng.mask_soft.numpy(), soft) and torch.equal(eng.mask_w, want_w) and np.array_equal(got, want)
    from videosd_amd.plan import export_plan

    with pytest.raises(ValueError, match="export_plan: .*mask_feather.*vsd_gauss_blur"):
        export_plan(eng, str(tmp_path / "x.vsdplan"))


def test_setters_note_a_table_and_upload_on_change_without_re_recording(eng):
    ops = eng.ops
    eng.prepare(H, Wd, STEPS, 1.0, keep_mask=True, edges="canny", edge_blur=1.4, mask_feather=4.0, **PREP)
    assert _names(eng).count("gauss_blur") == 2
    ops.uploads.clear()
    program, serial = eng.program, eng.program_serial
    blocks = eng.taps
    sent = lambda k: ops.uploads.count(blocks[k].dev.data_ptr())  # noqa: E731
    eng.launch()
    assert sent("edge_blur") == sent("mask_feather") == 0  # (sent ahead of the warm-up run already)
    eng.set_edge_blur(1.4)  # what is there already
    eng.launch()
    assert sent("edge_blur") == 0
    eng.set_edge_blur(3.0)
    assert sent("edge_blur") == 0 and np.array_equal(blocks["edge_blur"].dev.numpy(), BL.gauss_taps(1.4))  # only noted: the next launch sends it
    eng.launch()
    assert sent("edge_blur") == 1 and sent("mask_feather") == 0 and np.array_equal(blocks["edge_blur"].dev.numpy(), BL.gauss_taps(3.0))
    eng.set_mask_feather(0)
    eng.launch()
    assert sent("mask_feather") == 1 and np.array_equal(blocks["mask_feather"].dev.numpy(), BL.identity_taps())
    assert eng.program is program and eng.program_serial is serial and eng.taps is blocks
    for bad in (-1, 11, float("nan"), "x"):
        with pytest.raises(ValueError, match="edge_blur: .*sigma must be a number"):
            eng.set_edge_blur(bad)
    eng.launch()
    assert sent("edge_blur") == 1  # a refused call changes nothing
    slot = eng.make_slot()
    slot.prepare(H, Wd, STEPS, 1.0, keep_mask=True, edges="canny", edge_blur=1.4, mask_feather=4.0, **PREP)
    assert slot.taps["edge_blur"].dev.data_ptr() != blocks["edge_blur"].dev.data_ptr()  # a slot has tables of its own


def test_prepare_refusals_by_name(eng, tmp_path):
    with pytest.raises(ValueError, match="mask_feather needs keep_mask=True"):
        eng.prepare(H, Wd, STEPS, 1.0, mask_feather=2.0, **PREP)
    with pytest.raises(ValueError, match=r"edge_blur: .*sigma must be a number in \[0, 10\]"):
        eng.prepare(H, Wd, STEPS, 1.0, edge_blur=12.0, **PREP)
    e = Engine.__new__(Engine)
    e.ops = FakeOps()
    with pytest.raises(ValueError, match="edge_blur needs the op gauss_blur"):
        e.prepare(64, 64, 2, 0.5, edge_blur=1.0)
    eng.prepare(H, Wd, STEPS, 1.0, edge_blur=0, **PREP)  # 0 is a sigma: the stage is there, with the identity table
    assert _names(eng).count("gauss_blur") == 1 and np.array_equal(eng.taps["edge_blur"].dev.numpy(), BL.identity_taps())
    from videosd_amd.plan import export_plan

    with pytest.raises(ValueError, match="export_plan: .*edge_blur.*vsd_gauss_blur"):
        export_plan(eng, str(tmp_path / "x.vsdplan"))


# ------------------------------------------------------------------------------------------ the class, before any device work
def test_the_class_takes_checks_and_passes_on_the_switches(tmp_path):
    from videosd_amd.pipeline import PlanKey, VideoSDPipeline

    p = bare_pipeline()
    assert p._blur == {}
    for setter in (p.set_edge_blur, p.set_mask_feather):
        with pytest.raises(ValueError, match="needs a pipeline built with (edge_blur|mask_feather)="):
            setter(1.0)
    q = VideoSDPipeline.__new__(VideoSDPipeline)
    with pytest.raises(ValueError, match="mask_feather needs keep_mask=True"):
        q._init_state(dict(mask_feather=2.0))
    with pytest.raises(ValueError, match="edge_blur: .*sigma must be a number"):
        q._init_state(dict(edge_blur=-2))
    p = VideoSDPipeline.__new__(VideoSDPipeline)
    p._init_state(dict(keep_mask=True, edge_blur=1.4, mask_feather=0))
    assert p._blur == {"edge_blur": 1.4, "mask_feather": 0.0}
    assert p.set_edge_blur(2) == 2.0 and p.set_mask_feather(4.5) == 4.5 and p._blur == {"edge_blur": 2.0, "mask_feather": 4.5}
    with pytest.raises(ValueError, match="mask_feather: .*sigma"):
        p.set_mask_feather(10.5)
    assert p._blur["mask_feather"] == 4.5
    with pytest.raises(ValueError, match="export_plan: .*edge_blur and mask_feather.*vsd_gauss_blur"):
        p.export_plan(str(tmp_path / "x.vsdplan"))
    with pytest.raises(ValueError, match="export_prompt: .*edge_blur and mask_feather"):
        p.export_prompt(str(tmp_path / "x.vsdprompt"), "a prompt")

    class Block:
        def __init__(self, sigma):
            self.sigma = sigma

    class Eng:  # what `_install` hands an engine: the sigma of the moment, once per change
        color_a, _mask_pipe_epoch, _ref_epoch = (), 0, 0
        use_prompt = use_prompts = lambda self, p: None

        def __init__(self):
            self.taps, self.got = {"edge_blur": Block(1.4), "mask_feather": Block(4.5)}, []

        def _set_blur(self, switch, sigma):
            self.got.append((switch, sigma))
            self.taps[switch].sigma = sigma

        def set_masks(self, m):
            pass

    e, key = Eng(), PlanKey(64, 64, 2, 2, True, False)
    p._install(e, key, None, [(0.5, 1.0)], None)
    p._install(e, key, None, [(0.5, 1.0)], None)
    assert e.got == [("edge_blur", 2.0)]
    p.set_mask_feather(0)
    p._install(e, key, None, [(0.5, 1.0)], None)
    assert e.got == [("edge_blur", 2.0), ("mask_feather", 0.0)]


def test_a_worker_takes_the_options_and_the_setters_between_frames():
    """the constructor's `edge_blur` / `mask_feather` reach the worker's object; `VideoSDPipeline.remote(...).set_edge_blur` /
    `.set_mask_feather` run in order with the frames around them (alone, after the launches in flight): frames queued before a setter keep
    the old value; a refusal comes back as the caller's ValueError"""
    import asyncio

    from videosd_amd.dispatch import RemotePipeline

    img = Image.fromarray(np.full((12, 16, 3), 10, np.uint8), "RGB")
    p = RemotePipeline(factory="blur_cases:BlurFakePipeline", model="m", controlnet="c", device=1, delay=0.02, batch=2, lanes=2,
                       edge_blur=1.5, mask_feather=4.0)
    tags = lambda outs: [tuple(int(v) for v in np.asarray(o)[0, 0, 1:]) for o in outs]  # noqa: E731
    try:
        async def go():
            first = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            change = p.set_edge_blur.remote(3.0)
            later = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            return [await f for f in first], await change, [await f for f in later]

        first, answer, later = asyncio.run(go())
        assert answer == 3.0 and tags(first) == [(15, 40)] * 4 and tags(later) == [(30, 40)] * 4
        assert p.set_mask_feather(0) == 0.0 and tags([p.infer(img, height=12, width=16)]) == [(30, 0)]  # the synchronous form
        with pytest.raises(ValueError, match="sigma"):
            p.set_mask_feather(99)
    finally:
        p.close()

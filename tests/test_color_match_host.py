"""Colour match without a GPU: vsd_color_match_host against the numpy restatement of THE COLOUR CONTRACT (include/vsd.h) byte for byte
on every case of tests/color_match_cases.py; header, binding and build list; `check_color_match`; the engine's wiring of
`color_match=` on the op emulator; the pipeline's constructor checks.

The recorded default programs are compared with tests/golden/program_fingerprints_before_color_match.txt, the listing of
scripts/program_fingerprint.py on the op emulator from the commit before this stage existed."""
import ctypes as Ct
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import color_match_cases as CM  # noqa: E402
from fake_ops import FakeOps  # noqa: E402

from videosd_amd import config as C  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vsd_color_match_workspace_bytes", "vsd_color_match", "vsd_color_match_host"]
VSD_ERR_ARG = -1


def color_match_host(src, dst, mode, a):
    """vsd_color_match_host on one [h][w][3] frame pair -> (status, the new dst)"""
    lib = L.load()
    src = np.ascontiguousarray(src, dtype=np.uint8)
    out = np.array(dst, dtype=np.uint8)  # (a copy: rewritten in place)
    h, w = src.shape[:2]
    rc = lib.vsd_color_match_host(src.ctypes.data, out.ctypes.data, h, w, CM.MODES[mode] if isinstance(mode, str) else mode, int(a))
    return rc, out


# ------------------------------------------------------------------------------------------ the host twin against the contract
@pytest.mark.parametrize("mode", list(CM.MODES))
@pytest.mark.parametrize("name", CM.NAMES)
def test_host_equals_the_contract(name, mode):
    src, dst = CM.case(name)
    for amounts in CM.amount_lists(len(src)):
        want = CM.expected(name, mode, amounts)
        for f, a in enumerate(amounts):
            rc, got = color_match_host(src[f], dst[f], mode, a)
            assert rc == 0 and np.array_equal(got, want[f]), (name, mode, a, f, int((got != want[f]).sum()))
            if a == 0:
                assert np.array_equal(got, dst[f])  # the identity, byte for byte
    if name.endswith("-same"):  # both modes leave dst as it is
        assert np.array_equal(CM.expected(name, mode, (256,) * len(src)), dst)


def test_the_cases_exercise_what_they_are_for():
    v = np.arange(256, dtype=np.int64)
    src, dst = CM.case("264x256x1-src255")
    assert int((v * v * CM.histograms(src[0])[0]).sum()) > 2 ** 32  # Q passes 2^32
    for name in CM.NAMES:
        src, dst = CM.case(name)
        N = src.shape[1] * src.shape[2]
        if name.endswith("-gain_cap") and N >= 64:
            for c in range(3):
                assert CM.gain(N, CM.histograms(src[0])[c], CM.histograms(dst[0])[c], capped=False) > 4 * CM.MAX_GAIN
                assert CM.gain(N, CM.histograms(src[0])[c], CM.histograms(dst[0])[c]) == CM.MAX_GAIN
        if name.endswith("-const_dst"):
            assert CM.gain(N, CM.histograms(src[0])[0], CM.histograms(dst[0])[0]) == 0.0  # Vd = 0
            got = CM.expected(name, "histogram", (256,) * len(src))[0]
            assert len(np.unique(got[..., 0])) == 1 and (N < 64 or 64 <= int(got[0, 0, 0]) <= 192)  # the source's median, not its maximum
    assert max(max(CM.case(n)[0].shape[1:3]) for n in CM.NAMES) == CM.MAX_SIDE
    # frame bases of the multi-frame cases fall off 16-byte alignment
    assert {(f * 3 * 17) % 16 for f in range(3)} != {0} and {(f * 3 * 35) % 16 for f in range(3)} != {0}


def test_the_two_modes_and_the_amount_do_something():
    src, dst = CM.case("64x64x1-two_valued")
    hist, mean = CM.expected("64x64x1-two_valued", "histogram", (256,)), CM.expected("64x64x1-two_valued", "meanstd", (256,))
    assert not np.array_equal(hist, dst) and not np.array_equal(mean, dst) and not np.array_equal(hist, mean)
    assert set(np.unique(hist)) <= {30, 200}  # histogram matching of a two-valued dst lands on the source's values
    half = CM.expected("64x64x1-two_valued", "histogram", (128,))
    assert not np.array_equal(half, hist) and not np.array_equal(half, dst)


def test_bad_arguments_are_refused():
    lib = L.load()
    f = np.zeros((8, 8, 3), np.uint8)
    for mode in (-1, 2, 7):
        assert color_match_host(f, f, mode, 128)[0] == VSD_ERR_ARG
    for a in (-1, 257, 1 << 20):
        assert color_match_host(f, f, 0, a)[0] == VSD_ERR_ARG
    out = np.zeros(64 * 3, np.uint8)
    for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (16385, 1), (1, 16385), (4096, 4096), (16384, 16384)):
        assert lib.vsd_color_match_host(f.ctypes.data, out.ctypes.data, h, w, 0, 128) == VSD_ERR_ARG, (h, w)
        assert lib.vsd_color_match_workspace_bytes(1, h, w) == 0
    assert lib.vsd_color_match_host(None, out.ctypes.data, 8, 8, 0, 128) == VSD_ERR_ARG
    assert lib.vsd_color_match_host(f.ctypes.data, None, 8, 8, 0, 128) == VSD_ERR_ARG
    assert lib.vsd_color_match_workspace_bytes(0, 8, 8) == 0 and lib.vsd_color_match_workspace_bytes(1025, 8, 8) == 0
    assert lib.vsd_color_match_workspace_bytes(1, 8, 8) >= 6 * 256 * 4 + 768
    assert lib.vsd_color_match_workspace_bytes(5, 512, 512) >= 5 * (48 * 6 * 256 * 4 + 768)
    assert lib.vsd_color_match_workspace_bytes(1, 2048, 4096) > 0  # VSD_COLOR_MAX_PIXELS itself
    assert lib.vsd_color_match(None, f.ctypes.data, out.ctypes.data, 1, 8, 8, 0, out.ctypes.data, out.ctypes.data, None) == VSD_ERR_ARG


# ------------------------------------------------------------------------------------------ header, binding, build list, check_color_match
def test_version_and_plan_functions_stay():
    from videosd_amd import plan as P

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header
    assert not [f for f in P.PLAN_FUNCS if "color" in f]


def test_header_binding_and_build_list_agree_on_the_three_symbols():
    from videosd_amd import build as Bd

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert "THE COLOUR CONTRACT" in header
    for name, value in (("VSD_COLOR_HIST", 0), ("VSD_COLOR_MEANSTD", 1)):
        assert re.search(rf"^#define {name} {value}$", header, re.M)
    assert "#define VSD_COLOR_MAX_PIXELS (1 << 23)" in header and L.COLOR_MAX_PIXELS == CM.MAX_PIXELS == 1 << 23
    assert L.COLOR_MODES == CM.MODES
    letter = {"void*": Ct.c_void_p, "vsd_ctx*": Ct.c_void_p, "int": Ct.c_int}
    for name in SYMBOLS:
        m = re.search(r"^(int64_t|int) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        args = [letter[a.rsplit(" ", 1)[0].replace("const ", "")] for a in re.sub(r"\s+", " ", m.group(2)).split(", ")]
        res, sig = L.SIGNATURES[name]
        assert res is (Ct.c_int64 if m.group(1) == "int64_t" else Ct.c_int) and sig == args, name
        src = [f for f in Bd.SOURCES if re.search(r'extern "C" (int64_t|int) ' + name + r"\(", open(os.path.join(Bd.CSRC, f)).read())]
        assert src == ["color_match.hip"], (name, src)
        assert hasattr(L.load(), name)
    assert Bd.OWN_HEADERS["color_match.hip"] == ["color_match_core.h"] and "-ffp-contract=off" in Bd.EXTRA_FLAGS["color_match.hip"]
    from videosd_amd.ops import HipOps

    assert callable(HipOps.color_match)


def test_check_color_match_accepts_and_refuses():
    assert L.check_color_match(None) == (None, 256)
    assert L.check_color_match("histogram", 1.0) == ("histogram", 256)
    assert L.check_color_match("meanstd", 0) == ("meanstd", 0)
    assert L.check_color_match("meanstd", 0.5) == ("meanstd", 128)
    assert L.check_color_match("histogram", 1 / 512) == ("histogram", 1)  # halves round up: round(0.5) = 1
    assert L.check_color_match("histogram", np.float32(0.25)) == ("histogram", 64)
    assert L.check_color_match("histogram", 0.9999)[1] == 256 and L.check_color_match("histogram", 0.001)[1] == 0
    for bad in ("hist", "lab", 0, True, ""):
        with pytest.raises(ValueError, match="histogram.*meanstd"):
            L.check_color_match(bad, 1.0)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "1", None, True, (0.5,)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            L.check_color_match("histogram", bad)


# ------------------------------------------------------------------------------------------ the engine's wiring, on the op emulator
class ColorFakeOps(FakeOps):
    """the op emulator with a `color_match` that is the numpy restatement of the contract"""

    def clone(self, lane=None):
        return ColorFakeOps()

    def color_match(self, src_u8, dst_u8, frames, h, w, mode, amounts_dev):
        assert amounts_dev.dtype == torch.int32 and amounts_dev.numel() == frames and mode in CM.MODES
        src, dst = src_u8.reshape(frames, h, w, 3).numpy(), dst_u8.reshape(frames, h, w, 3)
        for f in range(frames):
            dst[f].copy_(torch.from_numpy(CM.color_match_numpy(src[f], dst[f].numpy(), mode, int(amounts_dev[f]))))


def _calls(eng):
    return list(Engine.flat_calls(eng.program.calls))


def _names(eng):
    return [fn.__name__ for fn, _a, _k in _calls(eng)]


def _engine(ops):
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    eng = Engine(ops, C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def test_prepare_records_one_call_behind_postprocess_rgb(tmp_path):
    H, Wd, B = 64, 64, 3
    eng = _engine(ColorFakeOps())
    frames = np.random.default_rng(3).integers(0, 256, (B, H, Wd, 3), dtype=np.uint8)
    plan = eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False)
    plain_names = _names(eng)
    assert plan["color_match"] is None and eng.color_amounts is None and "color_match" not in plain_names
    plain = eng.infer_u8(frames)
    assert eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False, color_match=None)["color_match"] is None
    assert _names(eng) == plain_names  # the explicit default records what the default records
    with pytest.raises(ValueError, match="set_color_amount needs"):
        eng.set_color_amount(0.5)

    for mode in CM.MODES:
        plan = eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False, color_match=mode, color_amount=0.5)
        names = _names(eng)
        assert plan["color_match"] == mode and eng.color_a == (128,) * B and eng.color_amounts.tolist() == [128] * B  # (sent before the warm-up run)
        i = names.index("color_match")
        assert names.count("color_match") == 1 and names[i - 1] == "postprocess_rgb" and names[:i] + names[i + 1:] == plain_names
        assert [fn.__name__ for fn, _a, _k in Engine.flat_calls(eng.program_serial.calls)].count("color_match") == 1
        _fn, args, _kw = _calls(eng)[i]
        post_out = _calls(eng)[i - 1][1][3]
        src, dst = args[0], args[1]
        assert src.data_ptr() == eng.frame_u8.data_ptr() and tuple(src.shape) == (B, H, Wd, 3)  # frame_b
        assert dst.data_ptr() == eng.out_u8.data_ptr() == post_out.data_ptr() and tuple(dst.shape) == (B, H, Wd, 3)  # out_b
        assert args[2:6] == (B, H, Wd, mode) and args[6] is eng.color_amounts
        # the frames are the twin's of (frame_u8, the default program's out_u8), per frame, at the amount in place
        program = eng.program
        got = eng.infer_u8(frames)
        assert np.array_equal(got, np.stack([CM.color_match_numpy(frames[b], plain[b], mode, 128) for b in range(B)]))
        # a new amount, per frame: no re-record, and the next launch follows it
        eng.set_color_amount([0.0, 1.0, 77 / 256])
        assert eng.program is program and eng.color_a == (0, 256, 77)
        assert eng.color_amounts.tolist() == [128] * B  # only noted: what a launch in flight reads stays, the next launch sends it
        got = eng.infer_u8(frames)
        assert eng.color_amounts.tolist() == [0, 256, 77]
        assert np.array_equal(got, np.stack([CM.color_match_numpy(frames[b], plain[b], mode, a) for b, a in enumerate((0, 256, 77))]))
        assert np.array_equal(got[0], plain[0])
        eng.set_color_amount(1.0)  # a scalar sets every frame
        assert eng.program is program and eng.color_a == (256,) * B
        for bad in ([0.5, 0.5], [0.5] * 4, 1.5, "x", [0.1, 0.2, -1]):
            with pytest.raises(ValueError, match="color_amount"):
                eng.set_color_amount(bad)
        assert eng.color_a == (256,) * B and eng.color_amounts.tolist() == [0, 256, 77]  # a refused call changes nothing
        eng.launch()
        assert eng.color_amounts.tolist() == [256] * B
        # no plan file for this mode, by name
        from videosd_amd.plan import export_plan

        with pytest.raises(ValueError, match="color_match="):
            export_plan(eng, str(tmp_path / "x.vsdplan"))
    # reference-only mode and a program without a ControlNet take the stage as well
    eng.prepare(H, Wd, 2, 0.6, use_controlnet=False, use_graph=False, color_match="meanstd")
    assert _names(eng).count("color_match") == 1 and _names(eng)[-1] == "color_match"
    eng.prepare(H, Wd, 2, 0.6, use_controlnet=False, ref_mode=True, use_graph=False, color_match="histogram")
    assert _names(eng)[-2:] == ["postprocess_rgb", "color_match"] and _calls(eng)[-1][1][0].data_ptr() == eng.frame_u8.data_ptr()


def test_prepare_names_the_missing_op_and_bad_arguments():
    e = Engine.__new__(Engine)
    e.ops = FakeOps()
    with pytest.raises(ValueError, match="needs the op color_match"):
        e.prepare(64, 64, 2, 0.5, color_match="histogram")
    e.ops = ColorFakeOps()
    with pytest.raises(ValueError, match="histogram.*meanstd"):
        e.prepare(64, 64, 2, 0.5, color_match="lab")
    for bad in (-0.5, 2, None, "1"):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            e.prepare(64, 64, 2, 0.5, color_match="histogram", color_amount=bad)
    with pytest.raises(ValueError, match="VSD_COLOR_MAX_PIXELS"):
        e.prepare(4096, 4096, 2, 0.5, color_match="histogram")


def test_the_default_programs_are_those_of_the_commit_before(monkeypatch):
    """the emulator's fingerprints of every default program of scripts/program_fingerprint.py (no `color_match`), against the listing that
    script wrote on the commit before the stage existed"""
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


def test_a_worker_takes_set_color_match_between_frames():
    """`VideoSDPipeline.remote(...).set_color_match`: the call reaches the worker's object in order with the frames around it (it runs alone,
    after the launches in flight), returns what the object returns, and a refusal comes back as the caller's ValueError"""
    import asyncio

    from PIL import Image

    from videosd_amd.dispatch import RemotePipeline

    img = Image.fromarray(np.full((12, 16, 3), 10, np.uint8), "RGB")
    p = RemotePipeline(factory="color_match_cases:ColorFakePipeline", model="m", controlnet="c", device=1, color_amount=0.25, delay=0.02, batch=2, lanes=2)
    try:
        async def go():
            first = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            change = p.set_color_match.remote(0.75)
            later = [p.infer.remote(img, height=12, width=16) for _ in range(4)]
            return [await f for f in first], await change, [await f for f in later]

        first, answer, later = asyncio.run(go())
        assert answer == 0.75
        assert [int(np.asarray(o)[0, 0, 2]) for o in first] == [32] * 4 and [int(np.asarray(o)[0, 0, 2]) for o in later] == [96] * 4
        assert p.set_color_match(1.0) == 1.0 and int(np.asarray(p.infer(img, height=12, width=16))[0, 0, 2]) == 128  # the synchronous form
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            p.set_color_match(1.5)
        assert int(np.asarray(p.infer(img, height=12, width=16))[0, 0, 2]) == 128
    finally:
        p.close()


# ------------------------------------------------------------------------------------------ the class, before any device work
def test_the_pipeline_reads_and_checks_the_switch(tmp_path):
    import inspect

    from videosd_amd.dispatch import PER_FRAME
    from videosd_amd.pipeline import INFER_DEFAULTS, VideoSDPipeline

    def state(**kw):
        p = VideoSDPipeline.__new__(VideoSDPipeline)
        p._init_state(kw)
        return p

    p = state()
    assert p.color_match is None and p.color_amount == 1.0
    with pytest.raises(ValueError, match="set_color_match needs"):
        p.set_color_match(0.5)
    p = state(color_match="histogram")
    assert p.color_match == "histogram" and p.color_amount == 1.0
    p = state(color_match="meanstd", color_amount=0.3)
    assert p.color_match == "meanstd" and p.color_amount == 77 / 256
    assert p.set_color_match(0.5) == 0.5 and p.color_amount == 0.5
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        p.set_color_match(1.5)
    assert p.color_amount == 0.5
    with pytest.raises(ValueError, match="histogram.*meanstd"):
        state(color_match="lab")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        state(color_match="histogram", color_amount=7)
    with pytest.raises(ValueError, match="color_match="):
        state(color_match="histogram").export_plan(str(tmp_path / "x.vsdplan"))
    # no per-request option came with it
    assert not [k for k in INFER_DEFAULTS if "color" in k] and not [r for r in PER_FRAME if "color" in repr(r)]
    assert "color" not in str(inspect.signature(VideoSDPipeline.infer))

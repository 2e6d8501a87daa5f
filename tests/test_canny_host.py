"""Canny edges without a GPU: vsd_canny_host against the numpy restatement of THE EDGE CONTRACT (include/vsd.h) byte for byte; header,
binding and build list; the engine's wiring of `edges="canny"` on the op emulator; the pipeline's constructor checks."""
import ctypes as Ct
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import canny_cases as CC  # noqa: E402
from fake_ops import FakeOps  # noqa: E402

from videosd_amd import config as C  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import weights as W  # noqa: E402
from videosd_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vsd_canny_workspace_bytes", "vsd_canny_control", "vsd_canny_host"]
VSD_ERR_ARG = -1


def canny_host(rgb, low, high):
    """vsd_canny_host on a [h][w][3] uint8 array -> (status, edge [h][w])"""
    lib = L.load()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    edge = np.full((h, w), 77, np.uint8)  # (poison: every byte must be written)
    rc = lib.vsd_canny_host(rgb.ctypes.data, h, w, int(low), int(high), edge.ctypes.data)
    return rc, edge


def _same(rgb, low, high):
    rc, got = canny_host(rgb, low, high)
    assert rc == 0
    ref = CC.canny_numpy(rgb, low, high)
    assert set(np.unique(got)) <= {0, 255}
    assert np.array_equal(got, ref), (rgb.shape, low, high, int((got != ref).sum()))
    return got


# ------------------------------------------------------------------------------------------ the host twin against the contract
@pytest.mark.parametrize("thr", CC.THRESHOLDS)
@pytest.mark.parametrize("h,w", CC.NOISE_SIZES)
def test_host_equals_the_contract_on_noise(h, w, thr):
    f, parts = CC.reference("noise", h, w, *thr)
    CC.assert_exercises("noise", h, w, parts)
    rc, got = canny_host(f, *thr)
    assert rc == 0 and np.array_equal(got, parts["edge"])


@pytest.mark.parametrize("kind", ["serpentine", "serpentine_noseed"])
@pytest.mark.parametrize("h,w", CC.SERPENTINE_SIZES)
def test_host_equals_the_contract_on_the_serpentine(h, w, kind):
    f, parts = CC.reference(kind, h, w)
    CC.assert_exercises(kind, h, w, parts)
    rc, got = canny_host(f, 100, 200)
    assert rc == 0 and np.array_equal(got, parts["edge"])


@pytest.mark.parametrize("h,w", CC.SMALL_SIZES)
def test_host_equals_the_contract_on_tiny_frames(h, w):
    rng = np.random.default_rng(h * 100 + w)
    for thr in ((0, 0), (100, 200), (300, 300)):
        for _ in range(8):
            _same(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), *thr)


def test_a_constant_frame_has_no_edges():
    for value in (0, 93, 255):
        for thr in ((0, 0), (100, 200)):
            got = _same(CC.constant_frame(40, 70, value), *thr)
            assert not got.any()


def test_threshold_corners():
    f = CC.noise_frame(64, 64)
    low_eq_high = _same(f, 120, 120)
    parts = CC.canny_parts(f, 120, 120)
    assert parts["cand"].sum() > 500 and np.array_equal(parts["cand"], parts["strong"]) and np.array_equal(low_eq_high > 0, parts["cand"])
    assert _same(f, 0, 0).sum() > 0            # every local maximum with a gradient
    assert not _same(f, 2040, 2040).any()      # nothing exceeds the largest magnitude
    rng = np.random.default_rng(5)
    binary = np.repeat((rng.integers(0, 2, (50, 90, 1)) * 255).astype(np.uint8), 3, axis=2)  # magnitudes up to the maximum, many ties
    _same(binary, 0, 0)
    _same(binary, 1000, 2039)


def test_bad_thresholds_and_sizes_are_refused():
    f = CC.noise_frame(8, 8)
    for low, high in ((-1, 10), (10, 5), (0, 2041), (2041, 2041), (-5, -1)):
        assert canny_host(f, low, high)[0] == VSD_ERR_ARG, (low, high)
    lib = L.load()
    edge = np.zeros(64, np.uint8)
    for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (16385, 1), (1, 16385)):
        assert lib.vsd_canny_host(f.ctypes.data, h, w, 100, 200, edge.ctypes.data) == VSD_ERR_ARG, (h, w)
        assert lib.vsd_canny_workspace_bytes(h, w) == 0
    assert lib.vsd_canny_host(None, 8, 8, 100, 200, edge.ctypes.data) == VSD_ERR_ARG
    assert lib.vsd_canny_host(f.ctypes.data, 8, 8, 100, 200, None) == VSD_ERR_ARG
    assert lib.vsd_canny_workspace_bytes(8, 8) >= 8 * 8 * 6
    assert lib.vsd_canny_control(None, f.ctypes.data, 8, 8, 100, 200, edge.ctypes.data, edge.ctypes.data, edge.ctypes.data, None) == VSD_ERR_ARG


# ------------------------------------------------------------------------------------------ header, binding, build list
def test_version_and_plan_functions_stay():
    from videosd_amd import plan as P

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert L.VERSION == 10 and "#define VSD_VERSION 10" in header
    assert not [f for f in P.PLAN_FUNCS if "canny" in f]


def test_header_binding_and_build_list_agree_on_the_three_symbols():
    from videosd_amd import build as Bd

    header = open(os.path.join(ROOT, "include", "vsd.h")).read()
    assert "THE EDGE CONTRACT" in header
    letter = {"void*": Ct.c_void_p, "vsd_ctx*": Ct.c_void_p, "int": Ct.c_int}
    for name in SYMBOLS:
        m = re.search(r"^(int64_t|int) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        args = []
        for a in re.sub(r"\s+", " ", m.group(2)).split(", "):
            args.append(letter[a.rsplit(" ", 1)[0].replace("const ", "")])
        res, sig = L.SIGNATURES[name]
        assert res is (Ct.c_int64 if m.group(1) == "int64_t" else Ct.c_int) and sig == args, name
        src = [f for f in Bd.SOURCES if re.search(r'extern "C" (int64_t|int) ' + name + r"\(", open(os.path.join(Bd.CSRC, f)).read())]
        assert src == ["canny.hip"], (name, src)
        assert hasattr(L.load(), name)
    from videosd_amd.ops import HipOps

    assert callable(HipOps.canny_control)


# ------------------------------------------------------------------------------------------ the engine's wiring, on the op emulator
class CannyFakeOps(FakeOps):
    """the op emulator with a `canny_control` that is the numpy restatement of the contract"""

    def clone(self, lane=None):
        return CannyFakeOps()

    def canny_control(self, rgb_u8, h, w, low, high, edge_u8, control_out):
        assert isinstance(low, int) and isinstance(high, int)
        e = torch.from_numpy(CC.canny_numpy(rgb_u8.reshape(h, w, 3).numpy(), low, high).reshape(-1).copy())
        edge_u8.copy_(e)
        control_out.zero_()
        for c in range(3):
            control_out[:, c] = (e > 0).half()


def _names(eng):
    return [fn.__name__ for fn, _a, _k in Engine.flat_calls(eng.program.calls)]


def _engine(ops):
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.")
    eng = Engine(ops, C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def test_prepare_records_the_chosen_edge_op_once_per_frame(tmp_path):
    H, Wd, B = 64, 64, 2
    eng = _engine(CannyFakeOps())
    plan = eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False)
    sobel_names = _names(eng)
    assert plan["edge_mode"] == "sobel" and plan["canny_thresholds"] is None
    assert sobel_names.count("sobel_control") == B and "canny_control" not in sobel_names
    assert _names(eng) == sobel_names and eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False, edges="sobel")["edge_mode"] == "sobel"
    assert _names(eng) == sobel_names  # the explicit default records what the default records

    plan = eng.prepare(H, Wd, 2, 0.6, batch=B, use_controlnet=True, use_graph=False, edges="canny", canny_thresholds=(50.9, 150))
    names = _names(eng)
    assert plan["edge_mode"] == "canny" and plan["canny_thresholds"] == (50, 150)  # a float is floored
    assert names.count("canny_control") == B and "sobel_control" not in names
    assert [n if n != "canny_control" else "sobel_control" for n in names] == sobel_names  # call for call, nothing else moved
    calls = [(a, k) for fn, a, k in Engine.flat_calls(eng.program.calls) if fn.__name__ == "canny_control"]
    assert all(a[1:5] == (H, Wd, 50, 150) for a, _k in calls)
    # the frames' edge maps are the contract's, frame by frame
    frames = np.stack([CC.noise_frame(H, Wd, seed=s) for s in (1, 2)])
    out = eng.infer_u8(frames)
    assert out.shape == frames.shape
    for b in range(B):
        assert np.array_equal(eng.edge_u8[b * H * Wd:(b + 1) * H * Wd].numpy().reshape(H, Wd), CC.canny_numpy(frames[b], 50, 150))
    # no plan file for this mode, by name
    from videosd_amd.plan import export_plan

    with pytest.raises(ValueError, match="edges="):
        export_plan(eng, str(tmp_path / "x.vsdplan"))
    # without a ControlNet there is no edge stage: the switch is inert
    eng.prepare(H, Wd, 2, 0.6, use_controlnet=False, use_graph=False, edges="canny")
    assert not {"canny_control", "sobel_control"} & set(_names(eng))


def test_prepare_names_the_missing_op_and_bad_arguments():
    e = Engine.__new__(Engine)
    e.ops = FakeOps()
    with pytest.raises(ValueError, match="canny_control"):
        e.prepare(64, 64, 2, 0.5, edges="canny")
    e.ops = CannyFakeOps()
    with pytest.raises(ValueError, match="sobel.*canny"):
        e.prepare(64, 64, 2, 0.5, edges="prewitt")
    for bad in ((200, 100), (-1, 5), (0, 2041), (1,), "ab", None, (float("nan"), 3)):
        with pytest.raises(ValueError, match="canny_thresholds"):
            e.prepare(64, 64, 2, 0.5, edges="canny", canny_thresholds=bad)


# ------------------------------------------------------------------------------------------ the class, before any device work
def test_the_pipeline_reads_and_checks_the_switch(tmp_path):
    from videosd_amd.pipeline import VideoSDPipeline

    def state(**kw):
        p = VideoSDPipeline.__new__(VideoSDPipeline)
        p._init_state(kw)
        return p

    p = state()
    assert p.edges == "sobel" and p.canny_thresholds == (100, 200)
    p = state(edges="canny")
    assert p.edges == "canny" and p.canny_thresholds == (100, 200)
    p = state(edges="canny", canny_thresholds=(60.7, 180.2))
    assert p.canny_thresholds == (60, 180) and all(isinstance(v, int) for v in p.canny_thresholds)
    with pytest.raises(ValueError, match="sobel.*canny"):
        state(edges="prewitt")
    for bad in ((200, 100), (0, 5000), (-3, 7), 5):
        with pytest.raises(ValueError, match="canny_thresholds"):
            state(edges="canny", canny_thresholds=bad)
    with pytest.raises(ValueError, match="edges="):
        state(edges="canny").export_plan(str(tmp_path / "x.vsdplan"))

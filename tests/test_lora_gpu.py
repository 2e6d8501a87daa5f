"""LoRA adapters on the GPU (include/vsd.h THE ADAPTER FUSE): vsd_lora_fuse bit for bit against the host twin on the case list of
tests/lora_cases.py, and the engine on the MINI networks: every weight-side tensor after a scale change against a fresh engine built
from the restatement-fused checkpoint, the rebuilt prompt blocks, the frames against the oracle, and the way back to the base bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_cases as LC  # noqa: E402
import test_lora_host as LH  # noqa: E402

from videosd_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = LC.case_list()


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


# ------------------------------------------------------------------------------------------ the kernel against the host twin
def _device_case(ops, case, arrays):
    """the case's arrays on the device (a shared destination once) and the table of its segments"""
    dev, by_id = [], {}
    for a in arrays:
        d = {}
        for name, x in a.items():
            if id(x) not in by_id:
                by_id[id(x)] = ops.to_device(torch.from_numpy(x.copy()))
            d[name] = by_id[id(x)]
        dev.append(d)
    segs = LC.as_struct_array(L, case, lambda i, name: dev[i][name].data_ptr())
    table = ops.to_device(torch.frombuffer(bytearray(bytes(segs)), dtype=torch.uint8).clone())
    return dev, table


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_equals_the_host_twin_bit_for_bit(ops, case):
    arrays = LC.make_arrays(case)
    assert all(LC.bounds_ok(g, a) for g, a in zip(case.segs, arrays))  # before anything runs: every access lies inside its buffer
    dev, table = _device_case(ops, case, arrays)
    assert table.data_ptr() % 16 == 0
    assert LH.run_host(case, arrays) == 0  # the twin writes into `arrays`
    ops.lora_fuse(table, len(case.segs), case.scales)
    ops.synchronize()
    for i, (a, d) in enumerate(zip(arrays, dev)):
        for name in ("dst", "ln_s", "ln_t", "copy"):
            if name in a:
                got = d[name].cpu().numpy().view(np.uint8).reshape(-1)
                want = a[name].view(np.uint8).reshape(-1)
                assert np.array_equal(got, want), (case.name, i, name, int((got != want).sum()))  # canaries included


def test_all_segments_in_one_launch_and_a_second_set_of_scales(ops):
    """every single-destination case as ONE table (blockIdx.y = the segment), twice: s1, then s2 over the same buffers gives what s2
    alone gives (the fuse always starts from the base copies)"""
    cases = [c for c in CASES if len(c.segs) == 1]
    big = LC.Case("all", [c.segs[0] for c in cases], (0.5, -0.25, 0.0, 1.25))
    arrays = [LC.make_arrays(c)[0] for c in cases]
    dev, table = _device_case(ops, big, arrays)
    for scales in ((0.5, -0.25, 0.0, 1.25), (0.0, 1.0, -3.0, 0.125)):
        case = LC.Case("all", big.segs, scales)
        assert LH.run_host(case, arrays) == 0
        ops.lora_fuse(table, len(case.segs), scales)
        ops.synchronize()
        for i, (a, d) in enumerate(zip(arrays, dev)):
            for name in ("dst", "ln_s", "ln_t", "copy"):
                if name in a:
                    assert np.array_equal(d[name].cpu().numpy().view(np.uint8).reshape(-1), a[name].view(np.uint8).reshape(-1)), (scales, cases[i].name, name)


def test_kernel_refusals_write_nothing(ops):
    case = next(c for c in CASES if c.name == "fold_raw_copy")
    arrays = LC.make_arrays(case)
    dev, table = _device_case(ops, case, arrays)
    bad = r"vsd_lora_fuse failed \(-1\)"
    with pytest.raises(RuntimeError, match=bad + ".*not finite"):
        ops.lora_fuse(table, 1, (float("nan"),))
    with pytest.raises(ValueError, match="at most 4"):
        ops.lora_fuse(table, 1, (1.0,) * 5)
    with pytest.raises(RuntimeError, match=bad + ".*segments"):
        ops.lora_fuse(table, 0, (1.0,))
    with pytest.raises(RuntimeError, match=bad + ".*aligned"):
        ops.lora_fuse(table[8:], 1, (1.0,))
    for field, value in (("k", 60), ("rows", 0), ("n", 5), ("map", 7), ("copy_kind", 9)):
        segs = LC.as_struct_array(L, case, lambda i, name: dev[i][name].data_ptr())
        setattr(segs[0], field, value)
        t = ops.to_device(torch.frombuffer(bytearray(bytes(segs)), dtype=torch.uint8).clone())
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*segment 0"):
            ops.lora_fuse_table(t, 1)
    ops.synchronize()
    for name in ("dst", "ln_s", "ln_t", "copy"):
        assert np.array_equal(dev[0][name].cpu().numpy().view(np.uint8), arrays[0][name].view(np.uint8)), name


# ------------------------------------------------------------------------------------------ the engine on the MINI networks
H = W = 64
STEPS, STRENGTH, CN_SCALE = 2, 0.6, 1.5
S1, S2 = (0.8, -0.5), (0.25, 1.5)


@pytest.fixture(scope="module")
def mini():
    """MINI networks with the blocks of width >= 128 absorbed, two adapters that together touch every UNet tensor, the base engine's
    digest and frame taken BEFORE anything is loaded"""
    import test_pipeline_gpu as TP
    import videosd_amd.engine as E
    from videosd_amd import config as CFG
    from videosd_amd import weights as Wt
    from videosd_amd.ops import HipOps

    import gc

    old = E.XATTN_ABSORB_MIN_C
    E.XATTN_ABSORB_MIN_C = 128
    try:
        # Seen once, in a run of the whole suite (this file alone, and behind tests/test_i420_gpu.py, passed): the first stream capture of
        # this fixture ended with hipErrorStreamCaptureInvalidated.  SUPPOSED cause, read in csrc/api.hip and not confirmed: a full garbage
        # collection inside `prepare` -- the adapters below make ~10^5 Python objects -- finalises a lib.Context left by an earlier module,
        # and vsd_destroy calls hipFree, which an open capture on any stream does not survive.  Every capture in the suite, and in a
        # long-lived process that drops engines, has that exposure (the LoRA section, lists it as open); here what is garbage is
        # collected before anything is captured.
        gc.collect()
        wu, wc, wv, text = TP._build(CFG.MINI_UNET, CFG.MINI_CONTROLNET)
        spec = Wt.unet_spec(CFG.MINI_UNET)
        ads, objs = LH._adapter_objects(spec, [(1, 4, None, 1), (2, 2, 1.0, 3)])
        gc.collect()

        def engine(weights):
            e = E.Engine(HipOps(0), CFG.MINI_UNET, CFG.MINI_CONTROLNET, CFG.TAESD, weights, wc, wv)
            e.set_text_embeds(text)
            e.prepare(H, W, STEPS, STRENGTH, controlnet_scale=CN_SCALE, use_controlnet=True, autotune=False)  # (the table's forms: two engines, one choice)
            return e

        # a checkpoint synthesized on the device is ALIASED by the packed buffers whose layout needs no change (Tensor.to of a tensor that
        # is already there), so a fuse rewrites those entries of `wu` in place: the restatement starts from a host copy taken before
        wu_host = TP._cpu(wu)
        eng = engine(wu)
        frame = TP._frame(H, W)
        st = dict(eng=eng, engine=engine, wu=wu_host, wc=wc, wv=wv, text=text, ads=ads, objs=objs, frame=frame,
                  base_digest=LC.digest(eng.unet), base_frame=eng.infer_u8(frame), base_prompt=eng.family["prompt"].buf.clone())
        st["base_temb"], st["entry"] = eng.shared["temb"]["unet"].clone(), eng.option_entry(STRENGTH, STEPS, True)
        st["base_entry"] = st["entry"].buf.clone()
        assert any(t.xa_raw is not None for t in eng.unet.transformers)
        eng.load_adapters(objs, wu_host)
        yield st
    finally:
        E.XATTN_ABSORB_MIN_C = old


def test_loading_changes_nothing(mini):
    eng = mini["eng"]
    assert LC.digest(eng.unet) == mini["base_digest"]
    assert np.array_equal(eng.infer_u8(mini["frame"]), mini["base_frame"])
    assert eng.family["adapters"].base_bytes > 0 and len(eng.family["adapters"].touched) == 283


def test_scale_change_equals_a_fresh_engine_and_meets_the_oracle(mini):
    import test_pipeline_gpu as TP
    from oracle.pipeline import OraclePipeline
    from videosd_amd import config as CFG

    eng = mini["eng"]
    eng.set_adapter_scales(S1)
    fw = LC.fused_weights(mini["wu"], list(zip(mini["ads"], S1)))
    fresh = mini["engine"](fw)
    assert LC.compare_networks(eng.unet, fresh.unet, fw) > 300  # every tensor reachable from Engine.unet, found by walking the dataclasses
    orc = OraclePipeline(CFG.MINI_UNET, CFG.MINI_CONTROLNET, TP._cpu(fw), TP._cpu(mini["wc"]), TP._cpu(mini["wv"]))
    r0, r1, mad, psnr, got = TP._compare(eng, orc, mini["frame"], mini["text"], H, W, STEPS, True, cn_scale=CN_SCALE)
    print(f"adapted frame vs the oracle handed the fused weights: r0 {r0:.2e} r1 {r1:.2e} mad {mad:.3f} psnr {psnr:.1f}")
    assert r0 <= 5e-3 and r1 <= 2e-2 and mad <= 1.5 and psnr >= 38.0, (r0, r1, mad, psnr)  # the MINI bounds of tests/test_pipeline_gpu.py
    assert np.abs(got.astype(int) - mini["base_frame"].astype(int)).mean() > 0.5  # ... and it is another picture than the base's
    # the rebuilt prompt block (rebuilt lazily, by the launch above) is the fresh engine's, byte for byte
    assert torch.equal(eng.family["prompt"].buf.cpu(), fresh.family["prompt"].buf.cpu())
    assert not torch.equal(eng.family["prompt"].buf.cpu(), mini["base_prompt"].cpu())
    fresh.infer_u8(mini["frame"])
    assert torch.equal(eng.pblock.buf.cpu(), fresh.pblock.buf.cpu())
    # ... and so are the plan's time tables (time_embedding, cond_proj and every time_emb_proj feed them, outside the packed buffers) and
    # a cached option entry: the same weights through the same kernels
    assert set(eng.shared["temb"]) == set(fresh.shared["temb"]) == {"unet", "cn"}
    for name in eng.shared["temb"]:
        assert torch.equal(eng.shared["temb"][name].cpu(), fresh.shared["temb"][name].cpu()), name
    assert not torch.equal(eng.shared["temb"]["unet"].cpu(), mini["base_temb"].cpu())
    assert torch.equal(eng.option_entry(STRENGTH, STEPS, True).buf.cpu(), fresh.option_entry(STRENGTH, STEPS, True).buf.cpu())
    assert torch.equal(mini["entry"].buf.cpu(), fresh.option_entry(STRENGTH, STEPS, True).buf.cpu())  # the entry built before loading, in place
    mini["d1"] = LC.digest(eng.unet)
    mini["frame1"] = got


def test_s1_s2_s1_gives_the_bytes_of_s1(mini):
    eng = mini["eng"]
    if "d1" not in mini:
        eng.set_adapter_scales(S1)
        mini["d1"], mini["frame1"] = LC.digest(eng.unet), eng.infer_u8(mini["frame"])
    eng.set_adapter_scales(S2)
    assert LC.digest(eng.unet) != mini["d1"]
    f2 = eng.infer_u8(mini["frame"])
    assert not np.array_equal(f2, mini["frame1"])
    eng.set_adapter_scales(S1)
    assert LC.digest(eng.unet) == mini["d1"]
    assert np.array_equal(eng.infer_u8(mini["frame"]), mini["frame1"])


def test_a_scale_change_with_a_launch_in_flight_is_refused(mini):
    eng = mini["eng"]
    eng.submit_u8(mini["frame"])
    with pytest.raises(RuntimeError, match="collect them first"):
        eng.set_adapter_scales(S2)
    eng.collect_u8()
    eng.set_adapter_scales(eng.family["adapters"].scales)


def test_zero_scales_and_unload_give_the_base_bytes_and_frames_back(mini):
    eng = mini["eng"]
    eng.set_adapter_scales(S2)
    eng.set_adapter_scales((0.0, 0.0))
    assert LC.digest(eng.unet) == mini["base_digest"]
    assert np.array_equal(eng.infer_u8(mini["frame"]), mini["base_frame"])
    assert torch.equal(eng.family["prompt"].buf.cpu(), mini["base_prompt"].cpu())
    assert torch.equal(eng.shared["temb"]["unet"].cpu(), mini["base_temb"].cpu())
    assert eng.option_entry(STRENGTH, STEPS, True) is mini["entry"] and torch.equal(mini["entry"].buf.cpu(), mini["base_entry"].cpu())
    eng.set_adapter_scales(S1)
    eng.unload_adapters()
    assert LC.digest(eng.unet) == mini["base_digest"] and eng.family["adapters"] is None
    assert np.array_equal(eng.infer_u8(mini["frame"]), mini["base_frame"])
    eng.load_adapters(mini["objs"], mini["wu"])  # (the fixture's state for whatever test runs next)


def test_width_320_fragment_major_copies_follow(ops):
    """a two-level network (320, 640): the six fragment-major copies of the fused tail exist at C == TAIL_C == 320 and must follow the fuse"""
    import videosd_amd.engine as E
    from videosd_amd import config as CFG
    from videosd_amd import weights as Wt

    assert getattr(ops, "TAIL_C", 0) == 320
    cfg = CFG.UNetConfig(block_out_channels=(320, 640), transformer_depth=(1, 1), layers_per_block=1, cross_dim=128, cond_proj_dim=64)
    spec = Wt.unet_spec(cfg)
    wu = Wt.synthesize(spec, "unet.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(CFG.TAESD), "vae.", device="cuda")
    ads, objs = LH._adapter_objects(spec, [(5, 2, 3.0, 1)])
    eng = E.Engine(ops, cfg, None, CFG.TAESD, wu, None, wv)
    wu = {k: v.cpu() for k, v in wu.items()}  # (before any fuse: see the fixture `mini`)
    assert sum(pl.frag for pl in eng.unet.places.values()) == 6 * 3  # (three attention sites at C = 320: down, up, up)
    base = LC.digest(eng.unet)
    eng.load_adapters(objs, wu)
    eng.set_adapter_scales((0.9,))
    fw = LC.fused_weights(wu, [(ads[0], 0.9)])
    fresh = E.Engine(ops.clone(), cfg, None, CFG.TAESD, fw, None, wv)
    n = LC.compare_networks(eng.unet, fresh.unet, fw)
    assert n > 100 and any("weight_frag" in p for p, _t in LC.walk_tensors(eng.unet))
    eng.unload_adapters()
    assert LC.digest(eng.unet) == base


# ------------------------------------------------------------------------------------------ through the class
OPTS = dict(prompt="a watercolor painting", height=96, width=160, strength=0.6, steps=2, controlnet_scale=1.5)
WORKER = dict(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table")


def _adapter_file(tmp_path):
    from safetensors.numpy import save_file
    from videosd_amd import config as CFG
    from videosd_amd import weights as Wt

    path = str(tmp_path / "ink.safetensors")
    save_file(LC.write_kohya(LC.synthetic_adapter(Wt.unet_spec(CFG.MINI_UNET), 9, rank=4, alpha=8.0)), path)
    return path


def _default_widths(monkeypatch):
    """the module-scoped fixture `mini` lowers engine.XATTN_ABSORB_MIN_C for as long as this module runs; the class is tested, and compared
    with a worker process, at the product's own threshold"""
    import videosd_amd.engine as E
    from videosd_amd import netweights as NW

    monkeypatch.setattr(E, "XATTN_ABSORB_MIN_C", NW.XATTN_ABSORB_MIN_C)


def _mad(a, b):
    return float(np.abs(np.asarray(a).astype(int) - np.asarray(b).astype(int)).mean())


def test_the_class_moves_a_scale_between_launches_and_refuses_under_one(monkeypatch, tmp_path):
    import gc

    import test_color_match_gpu as CM
    import test_pipeline_gpu as TP
    from PIL import Image

    gc.collect()
    _default_widths(monkeypatch)
    img = Image.fromarray(TP._frame(96, 160, seed=5), "RGB")
    base = np.asarray(CM._pipeline(monkeypatch).infer(img, **OPTS))
    p = CM._pipeline(monkeypatch, loras=[{"path": _adapter_file(tmp_path), "scale": 0.8, "name": "ink"}])
    assert p.lora_scales == {"ink": 0.8}
    styled = np.asarray(p.infer(img, **OPTS))
    assert _mad(styled, base) > 0.5  # the adapter really is in the weights
    handle = p.submit_batch([img], **OPTS)
    with pytest.raises(RuntimeError, match="collect them first"):
        p.set_lora_scale("ink", 0.2)
    assert np.array_equal(np.asarray(p.collect_batch(handle)[0]), styled) and p.lora_scales == {"ink": 0.8}
    eng, graph = handle.engine, handle.engine.graph
    p.set_lora_scale("ink", 0.0)
    assert np.array_equal(np.asarray(p.infer(img, **OPTS)), base)  # scale zero: bit for bit the pipeline without adapters
    p.set_lora_scale("ink", 0.8)
    handle = p.submit_batch([img], **OPTS)
    assert np.array_equal(np.asarray(p.collect_batch(handle)[0]), styled)  # and back, whatever came between
    assert handle.engine is eng and eng.graph is graph  # the same engine, the same capture
    with pytest.raises(ValueError, match="export_plan: this pipeline was built with loras"):
        p.export_plan(str(tmp_path / "x.vsdplan"), **OPTS)


def test_a_worker_takes_set_lora_scale_between_frames(monkeypatch, tmp_path):
    import gc

    import test_color_match_gpu as CM
    import test_pipeline_gpu as TP
    from PIL import Image
    from videosd_amd.dispatch import RemotePipeline

    gc.collect()
    _default_widths(monkeypatch)
    path = _adapter_file(tmp_path)
    img = Image.fromarray(TP._frame(96, 160, seed=6), "RGB")
    p = CM._pipeline(monkeypatch, loras=[{"path": path, "scale": 0.8, "name": "ink"}])
    want_a = np.asarray(p.infer(img, **OPTS))
    p.set_lora_scale("ink", -0.4)
    want_b = np.asarray(p.infer(img, **OPTS))
    assert _mad(want_a, want_b) > 0.5
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    w = RemotePipeline(factory="prompt_mix_cases:mini_pipeline", loras=[{"path": path, "scale": 0.8, "name": "ink"}], **WORKER)
    try:
        first = w.infer.remote(img, **OPTS)
        change = w.set_lora_scale.remote("ink", -0.4)  # queued behind the frame: it runs alone, after the launch has been collected
        second = w.infer.remote(img, **OPTS)
        got_a, new, got_b = np.asarray(first.result(timeout=300)), change.result(timeout=300), np.asarray(second.result(timeout=300))
    finally:
        w.close()
    print(f"worker: first vs a {_mad(got_a, want_a):.4f} vs b {_mad(got_a, want_b):.4f}; second vs a {_mad(got_b, want_a):.4f} vs b {_mad(got_b, want_b):.4f}")
    assert new == {"ink": -0.4}
    assert np.array_equal(got_a, want_a), (_mad(got_a, want_a), _mad(got_a, want_b))
    assert np.array_equal(got_b, want_b), (_mad(got_b, want_a), _mad(got_b, want_b))  # the new style's frame

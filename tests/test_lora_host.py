"""LoRA adapters without a GPU (include/vsd.h THE ADAPTER FUSE): the file parser and its refusals, the registry of where every checkpoint
tensor landed, the host twin vsd_lora_fuse_host bit for bit against the numpy restatement of tests/lora_cases.py, and the restatement
against what packing.py makes of a fused checkpoint."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_cases as LC  # noqa: E402

from videosd_amd import config as CFG  # noqa: E402
from videosd_amd import lib as L  # noqa: E402
from videosd_amd import lora as LR  # noqa: E402
from videosd_amd import packing as P  # noqa: E402
from videosd_amd import weights as W  # noqa: E402

CASES = LC.case_list()


# ------------------------------------------------------------------------------------------ the host twin against the restatement
def run_host(case, arrays):
    segs = LC.as_struct_array(L, case, lambda i, name: LC.np_addr(arrays[i][name]))
    sc = (C.c_float * 4)(*(list(case.scales) + [0.0] * (4 - len(case.scales))))
    return L.load().vsd_lora_fuse_host(segs, len(case.segs), sc)


def check_against(case, arrays, want, what):
    for i, (g, a, w) in enumerate(zip(case.segs, arrays, want)):
        for name in ("dst", "ln_s", "ln_t", "copy"):
            if name in w:
                got = a[name].view(np.uint16 if a[name].dtype == np.float16 else np.uint32)
                exp = w[name].view(got.dtype)
                assert np.array_equal(got.reshape(-1), exp.reshape(-1)), (what, case.name, i, name, int((got.reshape(-1) != exp.reshape(-1)).sum()))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_twin_equals_the_restatement_bit_for_bit(case):
    arrays = LC.make_arrays(case)
    assert all(LC.bounds_ok(g, a) for g, a in zip(case.segs, arrays))
    want = LC.expect_numpy(case, arrays)
    assert run_host(case, arrays) == 0
    check_against(case, arrays, want, "host twin")  # pad columns, other rows and the fold vectors of other rows: still the canaries


def test_all_zero_scales_give_the_base_bytes_back():
    case = next(c for c in CASES if c.name == "all_zero_scales")
    arrays = LC.make_arrays(case)
    assert run_host(case, arrays) == 0
    g, a = case.segs[0], arrays[0]
    assert np.array_equal(a["dst"][:, :g.k].view(np.uint16), a["w0"].view(np.uint16))  # a -0 stays -0
    assert (a["w0"].view(np.uint16) == 0x8000).any()
    assert (a["dst"][:, g.k:].view(np.uint16) == LC.CANARY).all()


def test_argument_errors_return_err_arg_and_write_nothing():
    case = next(c for c in CASES if c.name == "fold_raw_copy")
    lib = L.load()
    sc = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)

    def attempt(mutate, scales=sc, nseg=1):
        arrays = LC.make_arrays(case)
        before = {k: v.copy() for k, v in arrays[0].items()}
        segs = LC.as_struct_array(L, case, lambda i, name: LC.np_addr(arrays[i][name]))
        mutate(segs[0])
        assert lib.vsd_lora_fuse_host(segs, nseg, scales) == -1
        for k, v in arrays[0].items():
            assert np.array_equal(v.view(np.uint8), before[k].view(np.uint8)), k

    def setter(field, value, idx=None):
        def f(s):
            if idx is None:
                setattr(s, field, value)
            else:
                getattr(s, field)[idx] = value
        return f

    for m in (setter("w0", None), setter("dst", None), setter("rows", 0), setter("k", 60), setter("k", 0), setter("kp", 56), setter("row0", -1),
              setter("n", 0), setter("n", 5), setter("rank", 0, 0), setter("rank", 129, 0), setter("slot", 4, 0), setter("slot", -1, 0),
              setter("a", float("nan"), 0), setter("map", 2), setter("map", LC.MAP_GEGLU), setter("copy_kind", 3), setter("copy", None),
              setter("beta", None), setter("ln_s", None), setter("reserved", 1), setter("up", None, 0), setter("down", None, 0)):
        attempt(m)
    attempt(lambda s: setattr(s, "dst", s.dst + 8))                      # misaligned
    attempt(lambda s: (setattr(s, "copy_kind", LC.COPY_FRAG), setattr(s, "rows", 24)))  # fragment-major needs rows % 16 == 0
    attempt(lambda s: None, scales=(C.c_float * 4)(float("inf"), 0, 0, 0))
    attempt(lambda s: None, scales=None)
    attempt(lambda s: None, nseg=0)
    attempt(lambda s: None, nseg=65536)
    assert lib.vsd_lora_fuse_host(None, 1, sc) == -1
    two = next(c for c in CASES if c.name == "row_offset_two_of_four")
    arrays = LC.make_arrays(two)
    segs = LC.as_struct_array(L, two, lambda i, name: LC.np_addr(arrays[i][name]))
    segs[0].slot[1] = segs[0].slot[0]  # slots must increase
    assert lib.vsd_lora_fuse_host(segs, 1, sc) == -1
    assert lib.vsd_lora_seg_size() == C.sizeof(L.LoraSeg)


# ------------------------------------------------------------------------------------------ the restatement against packing.py
def _bound(terms64):
    """(K-1) * 2^-24 * sum_k |term_k|: the fp32 summation bound for ANY order (Higham, Accuracy and Stability, 4.2 with u = 2^-24)"""
    k = terms64.shape[1]
    return (k - 1) * 2.0 ** -24 * np.abs(terms64).sum(axis=1)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _fold_sums_ok(wf, gamma, beta, bias, ln_s, ln_t, wp):
    ts = wp.astype(np.float64)
    tt = (wf.astype(np.float32) * beta[None, :]).astype(np.float64)  # (each term is one fp32 product: the contract's fmul)
    assert (np.abs(ln_s - ts.sum(axis=1)) <= _bound(ts) + 1e-30).all()
    want_t = tt.sum(axis=1) + (0 if bias is None else bias.astype(np.float64))
    slack = 0 if bias is None else 2.0 ** -24 * np.abs(want_t)  # the one further rounding of fadd(sum, bias)
    assert (np.abs(ln_t - want_t) <= _bound(tt) + slack + 1e-30).all()


def _adapters(rng, rows, k, ranks):
    return [((rng.standard_normal((rows, r)) * 0.1).astype(np.float16), (rng.standard_normal((r, k)) * 0.1).astype(np.float16), np.float32(a), i)
            for i, (r, a) in enumerate(ranks)]


def _seg_for(w0, ads, dst, **kw):
    s = L.LoraSeg()
    s.w0, s.dst = LC.np_addr(w0), LC.np_addr(dst)
    s.rows, s.k, s.kp, s.row0 = w0.shape[0], w0.shape[1], dst.shape[1], kw.get("row0", 0)
    s.map, s.n, s.copy_kind = kw.get("map", 0), len(ads), kw.get("copy_kind", 0)
    for i, (up, down, a, slot) in enumerate(ads):
        s.up[i], s.down[i], s.rank[i], s.slot[i], s.a[i] = LC.np_addr(up), LC.np_addr(down), up.shape[1], slot, float(a)
    for f in ("gamma", "beta", "bias", "ln_s", "ln_t", "copy"):
        if kw.get(f) is not None:
            setattr(s, f, LC.np_addr(kw[f]))
    return s


def _run(segs, scales):
    arr = (L.LoraSeg * len(segs))(*segs)
    sc = (C.c_float * 4)(*(list(scales) + [0.0] * (4 - len(scales))))
    assert L.load().vsd_lora_fuse_host(arr, len(segs), sc) == 0


def test_fused_then_packed_linear_ln_equals_the_twin():
    rng = np.random.default_rng(11)
    c, k, scales = 24, 64, (0.7, -0.4)
    ws = [(rng.standard_normal((c, k)) * 0.05).astype(np.float16) for _ in range(3)]
    gamma, beta = (1 + 0.1 * rng.standard_normal(k)).astype(np.float16), (0.1 * rng.standard_normal(k)).astype(np.float16)
    ads = [_adapters(rng, c, k, [(4, 1.0), (12, 0.5)]) for _ in range(3)]
    fused = [LC.fuse_numpy(w, a, scales) for w, a in zip(ws, ads)]
    pk = P.pack_linear_ln([_t(f) for f in fused], None, _t(gamma), _t(beta))
    dst = np.full((3 * c, pk.kp), LC.CANARY, np.uint16).view(np.float16)
    ln_s, ln_t = np.zeros(3 * c, np.float32), np.zeros(3 * c, np.float32)
    g32, b32 = gamma.astype(np.float32), beta.astype(np.float32)
    _run([_seg_for(w, a, dst, row0=i * c, gamma=g32, beta=b32, ln_s=ln_s, ln_t=ln_t) for i, (w, a) in enumerate(zip(ws, ads))], scales)
    assert np.array_equal(dst.view(np.uint16), pk.weight.numpy().view(np.uint16))
    _fold_sums_ok(np.concatenate(fused), g32, b32, None, ln_s, ln_t, dst[:, :k])
    # ... and packing's own sums (another order) lie within the same bound of the same fp64 sums
    _fold_sums_ok(np.concatenate(fused), g32, b32, None, pk.ln_s.numpy(), pk.ln_t.numpy(), dst[:, :k])


def test_fused_then_packed_geglu_ln_equals_the_twin():
    rng = np.random.default_rng(12)
    n, k, scales = 256, 64, (1.1,)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float16)
    bias = (0.1 * rng.standard_normal(n)).astype(np.float16)
    gamma, beta = (1 + 0.1 * rng.standard_normal(k)).astype(np.float16), (0.1 * rng.standard_normal(k)).astype(np.float16)
    ads = _adapters(rng, n, k, [(4, 2.0)])
    fused = LC.fuse_numpy(w, ads, scales)
    pk = P.pack_geglu_ln(_t(fused), _t(bias), _t(gamma), _t(beta))
    dst = np.full((n, pk.kp), LC.CANARY, np.uint16).view(np.float16)
    ln_s, ln_t = np.zeros(n, np.float32), np.zeros(n, np.float32)
    g32, b32, bias32 = gamma.astype(np.float32), beta.astype(np.float32), bias.astype(np.float32)
    _run([_seg_for(w, ads, dst, map=LC.MAP_GEGLU, gamma=g32, beta=b32, bias=bias32, ln_s=ln_s, ln_t=ln_t)], scales)
    assert np.array_equal(dst.view(np.uint16), pk.weight.numpy().view(np.uint16))
    inv = LC.map_rows(LC.MAP_GEGLU, n)  # source row -> destination row
    _fold_sums_ok(fused, g32, b32, bias32, ln_s[inv], ln_t[inv], dst[inv][:, :k])
    _fold_sums_ok(fused, g32, b32, bias32, pk.ln_s.numpy()[inv], pk.ln_t.numpy()[inv], dst[inv][:, :k])


@pytest.mark.parametrize("cin,cin_pad,ksize", [(4, 8, 3), (8, None, 3), (16, None, 1)])
def test_fused_then_packed_conv_equals_the_twin(cin, cin_pad, ksize):
    rng = np.random.default_rng(13)
    cout, r, scales = 24, 4, (0.9,)
    w = (rng.standard_normal((cout, cin, ksize, ksize)) * 0.05).astype(np.float16)
    up = (rng.standard_normal((cout, r)) * 0.1).astype(np.float16)
    down = (rng.standard_normal((r, cin, ksize, ksize)) * 0.1).astype(np.float16)
    fused = LC.fuse_numpy(w.reshape(cout, -1), [(up, down.reshape(r, -1), np.float32(0.5), 0)], scales).reshape(w.shape)
    pk = P.pack_conv(_t(fused), None, cin_pad=cin_pad)
    base = P.pack_conv(_t(w), None, cin_pad=cin_pad)
    w0 = np.ascontiguousarray(base.weight.numpy()[:, :base.k])   # the base copy: the packed k order, padded channels zero
    dpk = LR.pack_down(_t(down), cin_pad).numpy()
    assert dpk.shape == (r, base.k)
    dst = base.weight.numpy().copy()                              # the engine's buffer: the pad columns hold packing's zeros
    _run([_seg_for(w0, [(up, dpk, np.float32(0.5), 0)], dst)], scales)
    assert np.array_equal(dst.view(np.uint16), pk.weight.numpy().view(np.uint16))


def test_fragment_major_copy_equals_pack_mfma_frag():
    rng = np.random.default_rng(14)
    n, k, scales = 320, 320, (0.6, 0.2)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float16)
    ads = _adapters(rng, n, k, [(4, 1.0), (1, 1.0)])
    fused = LC.fuse_numpy(w, ads, scales)
    pk = P.add_frag(P.pack_linear(_t(fused)))
    dst = np.zeros((n, pk.kp), np.float16)
    frag = np.zeros(n * k, np.float16)
    _run([_seg_for(w, ads, dst, copy_kind=LC.COPY_FRAG, copy=frag)], scales)
    assert np.array_equal(dst.view(np.uint16), pk.weight.numpy().view(np.uint16))
    assert np.array_equal(frag.view(np.uint16), pk.weight_frag.numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------ the parser
SPECS = {"mini": W.unet_spec(CFG.MINI_UNET), "sd15": W.unet_spec(CFG.SD15_UNET)}
WRITERS = {"peft": lambda ad: LC.write_peft(ad, True), "peft_old": lambda ad: LC.write_peft(ad, False), "peft_bare": lambda ad: LC.write_peft(ad, True, prefix=""),
           "kohya": LC.write_kohya}


@pytest.mark.parametrize("spec_name", ["mini", "sd15"])
@pytest.mark.parametrize("conv", sorted(WRITERS))
def test_each_convention_maps_every_tensor(spec_name, conv):
    spec = SPECS[spec_name]
    shapes = {n: sh for n, sh, kind in spec if kind == "w"}
    ad = LC.synthetic_adapter(spec, 3, rank=2, alpha=1.0 if conv == "kohya" else None)
    got = LR.parse_adapter(WRITERS[conv](ad), spec, name="x")
    assert set(got.tensors) == set(shapes) == set(ad)
    for n, t in got.tensors.items():
        up, down, alpha = ad[n]
        assert tuple(t.up.shape) == (shapes[n][0], 2) and tuple(t.down.shape) == (2,) + tuple(shapes[n][1:]) and t.rank == 2
        assert t.a == (0.5 if alpha is not None else 1.0)
        assert torch.equal(t.up, _t(up)) and torch.equal(t.down, _t(down))
    assert got.text_encoder_keys_skipped == 0


def test_kohya_names_with_underscored_modules_resolve():
    spec = SPECS["mini"]
    ad = LC.synthetic_adapter(spec, 4, rank=1)
    want = [n for n in ad if any(s in n for s in ("to_out.0", "ff.net.0.proj", "time_emb_proj", "ff.net.2", "conv_shortcut", "proj_in"))]
    assert len({n.split(".")[-2] for n in want}) >= 5
    got = LR.parse_adapter(LC.write_kohya({n: ad[n] for n in want}), spec)
    assert set(got.tensors) == set(want)
    assert "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_ff_net_0_proj.lora_down.weight" in LC.write_kohya(ad)


def test_safetensors_round_trip(tmp_path):
    from safetensors.numpy import save_file

    spec = SPECS["mini"]
    ad = LC.synthetic_adapter(spec, 5, rank=3, alpha=6.0, every=7)
    p = str(tmp_path / "a.safetensors")
    save_file(LC.write_kohya(ad), p)
    got = LR.load_adapter(p, spec, name="ink")
    assert got.name == "ink" and set(got.tensors) == set(ad) and all(t.a == 2.0 for t in got.tensors.values())
    with pytest.raises(LR.AdapterError, match="safetensors files only"):
        LR.load_adapter(str(tmp_path / "a.ckpt"), spec)


def test_refusals_name_the_key_and_the_count():
    spec = SPECS["mini"]
    ad = LC.synthetic_adapter(spec, 6, rank=2, every=40)
    base = LC.write_peft(ad)
    k0 = sorted(k for k in base if "lora_A" in k)[0]
    mod = k0[len("unet."):-len(".lora_A.weight")]

    def refused(extra, match, drop=(), **kw):
        t = {k: v for k, v in base.items() if k not in drop}
        t.update(extra)
        with pytest.raises(LR.AdapterError, match=match):
            LR.parse_adapter(t, spec, **kw)

    z = np.zeros((2, 2), np.float16)
    refused({"unet.nowhere.to_q.lora_A.weight": z, "unet.nowhere.to_q.lora_B.weight": z}, r"match no UNet tensor: 'unet\.nowhere\.to_q\.lora_A\.weight' and 1 more \(2 in all\)")
    refused({"lora_unet_down_blocks_9_x.lora_down.weight": z}, r"match no UNet tensor: 'lora_unet_down_blocks_9_x\.lora_down\.weight' \(1 in all\)")
    refused({k0: np.zeros((2, 3), np.float16)}, r"shapes that do not fit.*" + k0.replace(".", r"\.") + r"' \(1 in all\)")
    up_key = k0.replace("lora_A", "lora_B")
    refused({up_key: np.zeros((3, 2), np.float16)}, r"shapes that do not fit.*lora_B")
    shape = dict((n, sh) for n, sh, _k in spec)[mod + ".weight"]
    refused({k0: np.zeros((129,) + tuple(shape[1:]), np.float16), up_key: np.zeros((shape[0], 129), np.float16)}, r"rank above 128: '" + k0.replace(".", r"\."))
    bad = base[k0].copy()
    bad.reshape(-1)[0] = np.inf
    refused({k0: bad}, r"not finite.*lora_A.*\(1 in all\)")
    refused({k0: base[k0].astype(np.float32) * np.float32(1e9)}, r"not finite")  # finite in fp32, not as fp16
    refused({}, r"both its down and its up", drop=(up_key,))
    refused({f"unet.{mod}.lora_magnitude_vector": z}, r"DoRA / LoHa / LoKr.*lora_magnitude_vector")
    refused({"lora_unet_x.dora_scale": z}, r"DoRA / LoHa / LoKr")
    refused({"lora_unet_x.hada_w1_a": z}, r"DoRA / LoHa / LoKr")
    refused({"lora_unet_x.lokr_w1": z}, r"DoRA / LoHa / LoKr")
    refused({"lora_te1_text_model_x.lora_down.weight": z}, r"SDXL")
    refused({"lora_unet_input_blocks_4_1_proj_in.lora_down.weight": z}, r"SDXL")
    refused({"text_encoder_2.x.lora_A.weight": z}, r"SDXL")
    te = {"lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": z, "text_encoder.text_model.x.lora_A.weight": z}
    refused(te, r"text-encoder keys.*'lora_te_text_model.*and 1 more \(2 in all\)")
    t = dict(base)
    t.update(te)
    got = LR.parse_adapter(t, spec, skip_text_encoder=True)
    assert got.text_encoder_keys_skipped == 2 and set(got.tensors) == set(ad)
    with pytest.raises(LR.AdapterError, match="no UNet tensor is adapted"):
        LR.parse_adapter(te, spec, skip_text_encoder=True)


# ------------------------------------------------------------------------------------------ the registry, and the engine's host logic
from fake_ops import FakeOps  # noqa: E402

import videosd_amd.engine as E  # noqa: E402
from videosd_amd.netweights import NetWeights  # noqa: E402


class LoraFakeOps(FakeOps):
    """the op emulator with `lora_fuse` = the host twin over the same table (CPU tensors: their addresses are host addresses)"""
    TAIL_C = 64  # (so that the MINI networks keep fragment-major copies too)

    def clone(self, lane=None):
        return LoraFakeOps()

    def lora_fuse_table(self, segs, nseg):
        pass

    def lora_fuse(self, segs, nseg, scales):
        sc = (C.c_float * 4)(*(list(scales) + [0.0] * (4 - len(scales))))
        assert L.load().vsd_lora_fuse_host(C.c_void_p(segs.data_ptr()), nseg, sc) == 0


@pytest.fixture(scope="module")
def mini_weights():
    return W.synthesize(SPECS["mini"], "unet.")


@pytest.mark.parametrize("absorb", [640, 64])
def test_registry_covers_every_weight_and_no_two_places_overlap(mini_weights, absorb):
    net = NetWeights(LoraFakeOps(), CFG.MINI_UNET, dict(mini_weights), absorb_min_c=absorb)
    names = [n for n, _sh, kind in SPECS["mini"] if kind == "w"]
    assert set(net.places) == set(names)
    used, fold_used = {}, {}
    for n in names:
        pl = net.places[n]
        shape = dict((a, b) for a, b, _c in SPECS["mini"])[n]
        assert pl.rows == shape[0]
        dr = pl.row0 + LC.map_rows(LC.MAP_GEGLU if pl.geglu else LC.MAP_ID, pl.rows)
        assert dr.min() >= 0 and dr.max() < pl.pack.n and pl.pack.weight.shape == (pl.pack.n, pl.pack.kp)
        mask = used.setdefault(id(pl.pack), np.zeros((pl.pack.n, pl.pack.kp), np.int32))  # a fake allocator: who wrote which element
        mask[dr, :pl.pack.k] += 1
        if pl.fold is not None:
            fold_used.setdefault(id(pl.pack), np.zeros(pl.pack.n, np.int32))[dr] += 1
            assert pl.pack.ln_s is not None and pl.pack.ln_s.shape == (pl.pack.n,)
        else:
            assert pl.pack.ln_s is None
        assert pl.frag == (pl.pack.weight_frag is not None)
    for m in list(used.values()) + list(fold_used.values()):
        assert m.max() == 1                        # no two places overlap
    for pid, m in used.items():
        assert (m[:, :1].min() == 1) and m.sum() > 0  # ... and together they cover every row of every adapted buffer
    assert sum(pl.frag for pl in net.places.values()) > 0
    assert (sum(pl.raw_copy is not None for pl in net.places.values()) > 0) == (absorb == 64)
    # every packed weight buffer of the network is some place's: nothing derived from a checkpoint weight is missed
    place_bufs = {id(pl.pack.weight) for pl in net.places.values()} | {id(pl.pack.weight_frag) for pl in net.places.values() if pl.frag} | \
        {id(pl.raw_copy) for pl in net.places.values() if pl.raw_copy is not None}
    for path, t in LC.walk_tensors(net):
        if path.endswith(".weight") or path.endswith(".weight_frag") or ".xa_raw[0]" in path:
            assert id(t) in place_bufs, path


def _adapter_objects(spec, seeds_ranks):
    ads, objs = [], []
    for i, (seed, rank, alpha, every) in enumerate(seeds_ranks):
        ad = LC.synthetic_adapter(spec, seed, rank=rank, alpha=alpha, every=every)
        ads.append(ad)
        objs.append(LR.parse_adapter(LC.write_kohya(ad) if i % 2 else LC.write_peft(ad), spec, name=f"a{i}"))
    return ads, objs


def test_engine_scale_change_equals_a_fresh_engine_from_fused_weights(mini_weights, monkeypatch):
    monkeypatch.setattr(E, "XATTN_ABSORB_MIN_C", 128)
    spec = SPECS["mini"]
    wv = W.synthesize(W.taesd_spec(CFG.TAESD), "vae.")
    ads, objs = _adapter_objects(spec, [(1, 4, None, 1), (2, 2, 1.0, 3)])
    eng = E.Engine(LoraFakeOps(), CFG.MINI_UNET, CFG.MINI_CONTROLNET, CFG.TAESD, dict(mini_weights), None, wv)
    text = (torch.randn(77, CFG.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half()
    eng.set_text_embeds(text)
    base = LC.digest(eng.unet)
    blk0 = eng.family["prompt"].buf.clone()
    aset = eng.load_adapters(objs, mini_weights)
    assert LC.digest(eng.unet) == base and aset.nseg >= len(aset.touched) == 283
    with pytest.raises(ValueError, match="one per loaded adapter"):
        eng.set_adapter_scales((1.0,))
    with pytest.raises(RuntimeError, match="unload_adapters"):
        eng.load_adapters(objs, mini_weights)

    def fresh(scales):
        fw = LC.fused_weights(mini_weights, list(zip(ads, scales)))
        e = E.Engine(LoraFakeOps(), CFG.MINI_UNET, CFG.MINI_CONTROLNET, CFG.TAESD, fw, None, wv)
        e.set_text_embeds(text)
        return e, fw

    s1, s2 = (0.8, -0.5), (0.25, 1.5)
    eng.set_adapter_scales(s1)
    assert LC.digest(eng.unet) != base
    f1, fw1 = fresh(s1)
    assert LC.compare_networks(eng.unet, f1.unet, fw1) > 300
    d1 = LC.digest(eng.unet)
    eng.prepare(64, 64, 2, 0.6, use_controlnet=False)
    f1.prepare(64, 64, 2, 0.6, use_controlnet=False)
    ent, ent_f = eng.option_entry(0.6, 2, False), f1.option_entry(0.6, 2, False)
    assert torch.equal(ent.buf, ent_f.buf) and torch.equal(eng.shared["temb"]["unet"], f1.shared["temb"]["unet"])
    temb1 = eng.shared["temb"]["unet"].clone()
    eng._sync_prompt()  # the cached prompt is rebuilt before its next use ...
    assert torch.equal(eng.family["prompt"].buf, f1.family["prompt"].buf) and not torch.equal(eng.family["prompt"].buf, blk0)
    assert torch.equal(eng.pblock.buf, f1.family["prompt"].buf)  # ... and installed again
    eng.set_adapter_scales(s2)
    f2, fw2 = fresh(s2)
    LC.compare_networks(eng.unet, f2.unet, fw2)
    # what is derived from the weights OUTSIDE the packed buffers follows before the next launch: the plan's time tables (time_embedding,
    # cond_proj, every time_emb_proj) and the cached option entries, the one in hand rebuilt in place
    f2.prepare(64, 64, 2, 0.6, use_controlnet=False)
    assert torch.equal(eng.shared["temb"]["unet"], temb1)  # (still the tables of s1 ...)
    eng._sync_prompt()                                     # (... until what every launch starts with has run)
    assert torch.equal(eng.shared["temb"]["unet"], f2.shared["temb"]["unet"]) and not torch.equal(eng.shared["temb"]["unet"], temb1)
    assert eng.option_entry(0.6, 2, False) is ent and torch.equal(ent.buf, f2.option_entry(0.6, 2, False).buf) and not torch.equal(ent.buf, ent_f.buf)
    assert torch.equal(eng.family["prompt"].buf, f2.family["prompt"].buf)
    blk = E.PromptBlock(eng.ops, eng.family["prompt"].layout)  # a block that cannot follow is refused, not run stale
    blk.epoch = -1
    eng.use_prompt(blk)
    with pytest.raises(RuntimeError, match="without its text embeddings"):
        eng._sync_prompt()
    eng.use_prompt(None)
    eng.set_adapter_scales(s1)
    assert LC.digest(eng.unet) == d1  # s1 -> s2 -> s1: the bytes of s1, whatever came between
    eng.family["in_flight"] = {eng}
    with pytest.raises(RuntimeError, match="collect them first"):
        eng.set_adapter_scales(s2)
    eng.family["in_flight"] = set()
    eng.set_adapter_scales((0.0, 0.0))
    assert LC.digest(eng.unet) == base
    eng.set_adapter_scales(s2)
    eng.unload_adapters()
    assert LC.digest(eng.unet) == base and eng.family["adapters"] is None
    base_eng = E.Engine(LoraFakeOps(), CFG.MINI_UNET, CFG.MINI_CONTROLNET, CFG.TAESD, dict(mini_weights), None, wv)
    base_eng.set_text_embeds(text)
    base_eng.prepare(64, 64, 2, 0.6, use_controlnet=False)
    eng._sync_prompt()
    assert torch.equal(eng.family["prompt"].buf, blk0) and torch.equal(eng.pblock.buf, blk0)
    assert torch.equal(eng.shared["temb"]["unet"], base_eng.shared["temb"]["unet"]) and torch.equal(ent.buf if eng.option_entry(0.6, 2, False) is ent else None, base_eng.option_entry(0.6, 2, False).buf)
    with pytest.raises(RuntimeError, match="no adapters are loaded"):
        eng.set_adapter_scales(s1)


# ------------------------------------------------------------------------------------------ the class's surface (no model loaded)
def test_the_class_takes_loras_and_moves_their_scales():
    from videosd_amd.pipeline import VideoSDPipeline as Real

    def VideoSDPipeline(**kwargs):  # the object as `_init_state` leaves it: every attribute from the kwargs alone, no model, no GPU
        p = Real.__new__(Real)
        p._init_state(kwargs)
        return p

    p = VideoSDPipeline(loras=[{"path": "styles/ink.safetensors", "scale": 0.8, "name": "ink"}, {"path": "styles/oil.safetensors"}])
    assert p.lora_scales == {"ink": 0.8, "oil": 1.0}

    class Model:
        calls = []

        def set_adapter_scales(self, scales):
            self.calls.append(list(scales))

    p.model = Model()
    assert p.set_lora_scale("ink", 0.35) == {"ink": 0.35, "oil": 1.0} and Model.calls == [[0.35, 1.0]]
    assert p.set_lora_scales({"oil": -0.5, "ink": 0.35}) == {"ink": 0.35, "oil": -0.5} and Model.calls[-1] == [0.35, -0.5]
    p.set_lora_scales({"oil": -0.5})
    assert len(Model.calls) == 2  # the same values again: no launch
    with pytest.raises(ValueError, match="no adapter named 'wash'"):
        p.set_lora_scale("wash", 1.0)
    with pytest.raises(ValueError, match="finite"):
        p.set_lora_scale("ink", float("nan"))
    p._in_flight.append(object())
    with pytest.raises(RuntimeError, match="collect them first"):
        p.set_lora_scale("ink", 0.5)
    p._in_flight.clear()
    with pytest.raises(ValueError, match="export_plan: this pipeline was built with loras"):
        p.export_plan("x.vsdplan")
    with pytest.raises(ValueError, match="export_prompt: this pipeline was built with loras"):
        p.export_prompt("x.vsdprompt", "a prompt")
    assert p.lora_scales == {"ink": 0.35, "oil": -0.5}
    q = VideoSDPipeline()
    assert q.lora_scales == {}
    with pytest.raises(ValueError, match="needs a pipeline built with loras"):
        q.set_lora_scale("ink", 1.0)
    for bad in ([{"scale": 1}], [{"path": "a.safetensors"}] * 2, [{"path": f"{i}.safetensors"} for i in range(5)]):
        with pytest.raises(ValueError, match="loras"):
            VideoSDPipeline(loras=bad)


def test_without_loras_the_program_fingerprints_are_the_stored_ones(monkeypatch):
    """default unchanged: the emulator's fingerprints of every default program of scripts/program_fingerprint.py against the stored
    listing (recorded before the colour-match stage, and before this one)"""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import program_fingerprint as pf

    golden = {}
    for line in open(os.path.join(root, "tests", "golden", "program_fingerprints_before_color_match.txt")):
        m = re.match(r"^(.*?)\s+([0-9a-f]{24})  calls (\d+) / (\d+)$", line.rstrip("\n"))
        golden[m.group(1)] = (m.group(2), int(m.group(3)), int(m.group(4)))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (on the emulator also where there is a GPU: the listing was recorded on it)
    weights, texts = pf.inputs()
    got = {cfg[0]: pf.fingerprint(pf.build(*cfg, weights, texts, use_graph=False, autotune=False)) for cfg in pf.configurations()}
    assert got == golden and len(got) > 3

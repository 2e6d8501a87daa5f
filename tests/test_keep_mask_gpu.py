"""Keep masks on the MI355X (csrc/keep_mask.hip, vsd_latent_keep in csrc/noise.hip) against the host twins, which
tests/test_keep_mask_host.py holds to the numpy restatement of THE KEEP MASK (include/vsd.h): every byte / bit of every case of
tests/keep_mask_cases.py, the pointers of the blend skewed by 0..3 bytes each inside buffers of canaries; determinism; the engine (all-255
and all-0 masks, mixed masks walked call by call, replay, new masks between two launches, a slot, device_seed, frame_options,
color_match, I420 output); the drop-in class.

Shapes: the smallest that reach each path -- below a 16-pixel vector step, one step with scalar ends, three workgroups per frame; one and
three frames (frame bases then fall off 16-byte alignment); latent rows either side of a 256-thread workgroup."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keep_mask_cases as KM  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN_FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "default_frames_mini_64x64_before_color_match.npy")
CANARY = 0xC3
PAD = 48  # canary bytes either side of an operand


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def _lib():
    from videosd_amd import lib as L

    return L.load()


def _p(a):
    return None if a is None else a.ctypes.data


def blend_twin(src, dst, mask):
    out = np.array(dst, dtype=np.uint8)
    f, h, w = mask.shape
    assert _lib().vsd_mask_blend_host(_p(np.ascontiguousarray(src)), _p(out), _p(np.ascontiguousarray(mask)), f, h, w) == 0
    return out


def latent_twin(mask):
    f, h, w = mask.shape
    out = np.empty((f, (h // 8) * (w // 8)), np.float32)
    assert _lib().vsd_mask_latent_host(_p(np.ascontiguousarray(mask)), f, h, w, _p(out)) == 0
    return out


def keep_twin(x0, wl, n0, coef, stride, hw, batch, lat=None, den=None):
    out = np.array(lat if lat is not None else den, dtype=np.float16)
    c = [None if a is None else np.ascontiguousarray(a) for a in (x0, wl, n0, coef)]
    assert _lib().vsd_latent_keep_host(_p(c[0]), _p(c[1]), _p(c[2]), _p(c[3]), stride, hw, batch, _p(out) if lat is not None else None,
                                       _p(out) if den is not None else None) == 0
    return out


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _placed(arr, skew):
    """the bytes of `arr` `skew` bytes past a 16-byte boundary inside a buffer of canaries -> (holder, view of the operand, its start)"""
    n = arr.size
    holder = torch.full((PAD + 16 + n + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + ((-(holder.data_ptr() + PAD)) % 16) + skew
    view = holder[start:start + n]
    assert view.data_ptr() % 16 == skew % 16
    view.copy_(torch.from_numpy(np.array(arr, dtype=np.uint8)).reshape(-1))  # (a copy: the shared cases are read-only)
    return holder, view, start


def _canaries_intact(holder, start, n):
    h = holder.cpu().numpy()
    return bool((h[:start] == CANARY).all() and (h[start + n:] == CANARY).all())


def run_blend(ops, src, dst, mask, skews=(0, 0, 0)):
    """ops.mask_blend on operands placed at the given skews -> the new dst; src, mask and all canaries checked"""
    frames, h, w = mask.shape
    placed = [_placed(a, k) for a, k in zip((src, dst, mask), skews)]
    torch.cuda.synchronize()  # (the operands were placed on torch's stream; the op runs on its own)
    ops.mask_blend(placed[0][1], placed[1][1], placed[2][1], frames, h, w)
    ops.synchronize()
    for (holder, view, start), a in zip(placed, (src, dst, mask)):
        assert _canaries_intact(holder, start, a.size), "bytes outside the operands were written"
    assert np.array_equal(placed[0][1].cpu().numpy(), src.reshape(-1)) and np.array_equal(placed[2][1].cpu().numpy(), mask.reshape(-1))
    return placed[1][1].cpu().numpy().reshape(dst.shape)


# ------------------------------------------------------------------------------------------ 1. the two u8 kernels against their twins
@pytest.mark.parametrize("frames", KM.FRAME_COUNTS)
@pytest.mark.parametrize("shape", KM.BLEND_SHAPES)
def test_blend_equals_the_twin_at_every_skew(ops, shape, frames):
    src, dst = KM.frames_pair(frames, *shape)
    wants = {kind: blend_twin(src, dst, KM.mask(kind, frames, *shape)) for kind in KM.MASK_KINDS}
    assert np.array_equal(wants["zeros"], src) and np.array_equal(wants["full"], dst)
    for ks in range(4):
        for kd in range(4):
            for km in range(4):  # (0, 0, 0) and (3, 3, 1) take the 16-pixel steps, the others single pixels
                for kind in KM.MASK_KINDS:
                    got = run_blend(ops, src, dst, KM.mask(kind, frames, *shape), (ks, kd, km))
                    assert np.array_equal(got, wants[kind]), (shape, frames, kind, (ks, kd, km), int((got != wants[kind]).sum()), "bytes differ")


def test_the_vector_steps_are_reached():
    """the walk of csrc/keep_mask_core.h, restated: which of the skews above take 16-pixel steps"""
    def nvec(ks, kd, km, n):
        head = min((16 - km) % 16, n)
        return (n - head) // 16 if (ks + 3 * head) % 16 == 0 and (kd + 3 * head) % 16 == 0 else 0

    took = {(ks, kd, km) for ks in range(4) for kd in range(4) for km in range(4) if nvec(ks, kd, km, 8 * 24)}
    assert took == {(0, 0, 0), (3, 3, 1)} and nvec(0, 0, 0, 15) == 0 and nvec(0, 0, 0, 16) == 1


@pytest.mark.parametrize("frames", KM.FRAME_COUNTS)
@pytest.mark.parametrize("shape", KM.LATENT_SHAPES)
def test_latent_weights_equal_the_twin(ops, shape, frames):
    n = frames * (shape[0] // 8) * (shape[1] // 8)
    for kind in KM.MASK_KINDS:
        m = KM.mask(kind, frames, *shape)
        want = latent_twin(m)
        for skew in range(4):  # (0: rows as 4-byte words; else byte by byte)
            holder, view, start = _placed(m, skew)
            out = torch.full((n + 2,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ops.mask_latent(view, frames, *shape, out[1:1 + n])
            ops.synchronize()
            assert np.array_equal(bits(out[1:1 + n]), bits(want.reshape(-1))), (shape, frames, kind, skew)
            assert out[0].item() == -7.0 and out[-1].item() == -7.0 and _canaries_intact(holder, start, m.size)


def test_the_same_call_twice_over_a_dirtied_destination_gives_the_same_bytes(ops):
    frames, h, w = 3, 72, 120
    src, dst = KM.frames_pair(frames, h, w)
    m = KM.mask("random", frames, h, w)
    a = run_blend(ops, src, dst, m, (3, 3, 1))
    b = run_blend(ops, src, dst, m, (3, 3, 1))  # (the destination is an operand: placed afresh, at the skew that takes the vector steps)
    assert np.array_equal(a, b) and np.array_equal(a, blend_twin(src, dst, m))
    dm = torch.from_numpy(np.array(m)).cuda()
    out = torch.full((frames, (h // 8) * (w // 8)), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ops.mask_latent(dm, frames, h, w, out)
    ops.synchronize()
    first = bits(out).copy()
    out.fill_(123.0)
    torch.cuda.synchronize()
    ops.mask_latent(dm, frames, h, w, out)
    ops.synchronize()
    assert np.array_equal(bits(out), first) and np.array_equal(first, bits(latent_twin(m)))


# ------------------------------------------------------------------------------------------ 2. the latent anchor
def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("stride", KM.KEEP_STRIDES)
@pytest.mark.parametrize("batch", KM.KEEP_BATCH)
@pytest.mark.parametrize("hw", KM.KEEP_HW)
def test_latent_keep_equals_the_twin(ops, hw, batch, stride):
    x0, lat, den, wl, n0, coef = KM.keep_case(hw, batch, stride)
    keep = wl == 1.0
    dx0, dwl, dn0, dcoef = _dev(x0), _dev(wl), _dev(n0), _dev(coef)
    # the step form, table noise
    dlat = _dev(lat)
    torch.cuda.synchronize()
    ops.latent_keep(dx0, dwl, dn0, None, 0, 0, dcoef, stride, hw, batch, lat=dlat)
    ops.synchronize()
    want = keep_twin(x0, wl, n0, coef, stride, hw, batch, lat=lat)
    assert np.array_equal(bits(dlat), bits(want)), (hw, batch, stride, int((bits(dlat) != bits(want)).sum()))
    assert np.array_equal(bits(dlat)[keep], bits(lat)[keep]) and np.array_equal(bits(dlat)[:, 4:], bits(lat)[:, 4:])  # untouched, -0.0 included
    # the seeded form = the table form fed by vsd_noise_fill of the same (seed, kind 0, draw 0), image by image
    seeds = [0x1234567 + 0x100000001 * b for b in range(batch)]
    dseeds = torch.tensor(seeds, dtype=torch.int64, device="cuda")
    dlat_s = _dev(lat)
    torch.cuda.synchronize()
    ops.latent_keep(dx0, dwl, None, dseeds, 0, 0, dcoef, stride, hw, batch, lat=dlat_s)
    table = torch.empty(4, hw, dtype=torch.float32, device="cuda")
    dlat_t = _dev(lat)
    for b in range(batch):
        rows = slice(b * hw, (b + 1) * hw)
        ops.noise_fill(seeds[b], 0, 0, hw, table)
        ops.latent_keep(dx0[rows], dwl[rows], table, None, 0, 0, dcoef[b * stride:], 0, hw, 1, lat=dlat_t[rows])
        ops.synchronize()
    assert np.array_equal(bits(dlat_s), bits(dlat_t)) and not np.array_equal(bits(dlat_s), bits(dlat))  # (another draw than the table's)
    # the final form: den against the twin; dec_in against the scheduler step's own expression on the blended den
    dden, ddec = _dev(den), torch.full((batch * hw, 8), 9.0, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    ops.latent_keep(dx0, dwl, None, None, 0, 0, None, 0, hw, batch, den=dden, dec_in=ddec)
    ops.synchronize()
    wantd = keep_twin(x0, wl, None, None, 0, hw, batch, den=den)
    assert np.array_equal(bits(dden), bits(wantd))
    assert np.array_equal(bits(dden)[keep], bits(den)[keep]) and np.array_equal(bits(dden)[:, 4:], bits(den)[:, 4:])
    assert np.array_equal(bits(ddec), bits(dec_in_by_lcm_step(ops, dden)))
    # the same calls again over dirtied destinations
    ddec.fill_(-3.0)
    dden2, dlat2 = _dev(den), _dev(lat)
    torch.cuda.synchronize()
    ops.latent_keep(dx0, dwl, None, None, 0, 0, None, 0, hw, batch, den=dden2, dec_in=ddec)
    ops.latent_keep(dx0, dwl, dn0, None, 0, 0, dcoef, stride, hw, batch, lat=dlat2)
    ops.synchronize()
    assert np.array_equal(bits(dden2), bits(wantd)) and np.array_equal(bits(dlat2), bits(want)) and np.array_equal(bits(ddec), bits(dec_in_by_lcm_step(ops, dden)))


def dec_in_by_lcm_step(ops, den):
    """`dec_in` as the existing vsd_lcm_step writes it for `den` as its sample: coefficients {1, 0, 1, 0, 1, 0} and no noise make its
    denoised output the sample itself, and dec_in the same device expression of it"""
    n = den.shape[0]
    eps = torch.zeros(n, 8, dtype=torch.float16, device="cuda")
    d2, out = torch.empty_like(eps), torch.empty_like(eps)
    torch.cuda.synchronize()
    ops.lcm_step(eps, den, None, [1.0, 0.0, 1.0, 0.0, 1.0, 0.0], n, None, d2, out)
    ops.synchronize()
    assert np.array_equal(bits(d2)[:, :4] & 0x7FFF, bits(den)[:, :4] & 0x7FFF)
    return out


def test_bad_combinations_are_refused_with_a_message(ops):
    x0, lat, den, wl, n0, coef = (_dev(a) for a in KM.keep_case(135, 1, 0))
    seeds = torch.zeros(1, dtype=torch.int64, device="cuda")
    dec = torch.zeros_like(den)
    for kw, text in ((dict(noise=n0, seeds=seeds, lat=lat), "exactly one"), (dict(lat=lat), "exactly one"), (dict(noise=n0, den=den, dec=dec), "no noise source"),
                     (dict(seeds=seeds, den=den, dec=dec), "no noise source"), (dict(noise=n0, lat=lat, den=den), "neither den nor dec_in"),
                     (dict(den=den), "den and dec_in"), (dict(), "den and dec_in"), (dict(noise=n0, lat=lat, stride=3), "coef_stride"),
                     (dict(noise=n0, lat=lat, coef=None), "coef_dev")):
        with pytest.raises(RuntimeError, match="latent_keep.*" + text):
            ops.latent_keep(x0, wl, kw.get("noise"), kw.get("seeds"), 0, 0, kw.get("coef", coef), kw.get("stride", 0), 135, 1, lat=kw.get("lat"),
                            den=kw.get("den"), dec_in=kw.get("dec"))
    m = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    w = torch.zeros(64, dtype=torch.float32, device="cuda")
    for h, wd in ((12, 8), (8, 20), (7, 7)):
        with pytest.raises(RuntimeError, match="mask_latent.*multiples of 8"):
            ops.mask_latent(m, 1, h, wd, w)
    for frames, h, wd in ((0, 8, 8), (1025, 1, 1), (1, 0, 8), (1, 8, 16385)):
        with pytest.raises(RuntimeError, match="mask_blend"):
            ops.mask_blend(m, m, m, frames, h, wd)


# ------------------------------------------------------------------------------------------ 3. the engine
H, W, STEPS, B = 64, 64, 2, 3
HW0 = (H // 8) * (W // 8)


@pytest.fixture(scope="module")
def engine():
    from videosd_amd import config as C
    from videosd_amd import weights as Wt
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu = Wt.synthesize(Wt.unet_spec(C.MINI_UNET), "unet.", device="cuda")
    wc = Wt.synthesize(Wt.controlnet_spec(C.MINI_CONTROLNET), "cn.", device="cuda")
    wv = Wt.synthesize(Wt.taesd_spec(C.TAESD), "vae.", device="cuda")
    eng = Engine(HipOps(0), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
    eng.set_text_embeds((torch.randn(77, C.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(7)) * 0.5).half())
    return eng


def _frames():
    rng = np.random.default_rng(11)
    ramp = np.linspace(0, 255, W, dtype=np.float64)[None, :, None]
    tints = np.array([[1.0, 0.6, 0.3], [0.3, 1.0, 0.7], [0.8, 0.8, 0.2]])
    return np.stack([np.clip(ramp * tints[b][None, None, :] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8) for b in range(B)])


PREP = dict(controlnet_scale=1.5, use_controlnet=True, batch=B, autotune=False)
OURS = ("mask_latent", "latent_keep", "mask_blend")


def _cpu(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def walk(eng, seeds=None):
    """Run `program_serial` call by call.  Around every keep-mask call: snapshot the operands, run the call, compare what it wrote with
    the host twin applied to the snapshot, to the bit (`dec_in` by the lcm_step route).  -> (calls checked by name, out_u8 ahead of the
    first call behind postprocess_rgb, out_u8 at the end).  Every call is checked on ITS OWN arguments: that they are the contract's (the
    next timestep's row, the frame's draw 0, its own x0) is the frame-level claim of tests/test_stage_oracle_gpu.py."""
    ops, Bn = eng.ops, eng.batch
    seen, raw = {k: 0 for k in OURS}, None
    for fn, a, k in eng.program_serial.calls:
        name = fn.__name__
        if name not in OURS:
            fn(*a, **k)
            if name == "postprocess_rgb":
                ops.synchronize()
                raw = _cpu(eng.out_u8).reshape(Bn, H, W, 3)
            continue
        ops.synchronize()
        seen[name] += 1
        if name == "mask_latent":
            m = _cpu(a[0])
            fn(*a, **k)
            ops.synchronize()
            assert np.array_equal(bits(a[4]), bits(latent_twin(m)))
        elif name == "mask_blend":
            src, dst, m = _cpu(a[0]), _cpu(a[1]), _cpu(a[2])
            fn(*a, **k)
            ops.synchronize()
            assert np.array_equal(_cpu(a[1]), blend_twin(src, dst, m))
        else:
            x0, wl, table, sd, kind, draw, coef, stride, hw, batch, lat, den, dec_in = a
            sx0, swl = _cpu(x0), _cpu(wl).reshape(-1)
            assert hw == HW0 and batch == Bn
            if lat is not None:  # the step form, image by image: the image's own coefficients and its own draw 0
                before = _cpu(lat)
                rows6 = _cpu(torch.as_strided(coef, (batch, 6), (stride, 1)))
                fn(*a, **k)
                ops.synchronize()
                after = _cpu(lat)
                fill = torch.empty(4, hw, dtype=torch.float32, device="cuda")
                for b in range(batch):
                    rows = slice(b * hw, (b + 1) * hw)
                    if sd is not None:
                        assert table is None and (kind, draw) == (0, 0)
                        torch.cuda.synchronize()
                        ops.noise_fill(seeds[b], 0, 0, hw, fill)
                        ops.synchronize()
                    n0 = _cpu(fill if sd is not None else table).reshape(4, hw)
                    want = keep_twin(sx0[rows], swl[rows], n0, rows6[b], 0, hw, 1, lat=before[rows])
                    assert np.array_equal(bits(after[rows]), bits(want)), (seen, b)
            else:
                before = _cpu(den)
                fn(*a, **k)
                ops.synchronize()
                assert table is None and sd is None
                assert np.array_equal(bits(den), bits(keep_twin(sx0, swl, None, None, 0, hw, batch, den=before)))
                assert np.array_equal(bits(dec_in), bits(dec_in_by_lcm_step(ops, den)))
    ops.synchronize()
    return seen, raw, _cpu(eng.out_u8).reshape(Bn, H, W, 3)


@pytest.fixture(scope="module")
def plain(engine):
    frames = _frames()
    plan = engine.prepare(H, W, STEPS, 0.6, use_graph=True, **PREP)
    assert plan["keep_mask"] is False and engine.mask_u8 is None
    out = engine.infer_u8(frames).copy()
    assert np.array_equal(out, np.load(GOLDEN_FRAMES)), "the default engine's frames are not the recorded ones"
    names = [fn.__name__ for fn, _a, _k in engine.flat_calls(engine.program.calls)]
    assert not [n for n in names if n in OURS]
    return frames, out, plan["n"]


def test_engine_full_zero_and_mixed_masks(engine, plain):
    from videosd_amd import lib as L

    frames, base, n = plain
    plan = engine.prepare(H, W, STEPS, 0.6, use_graph=True, keep_mask=True, **PREP)
    assert plan["keep_mask"] is True and engine.graph is not None
    # all 255 (the state after `prepare`): the recorded default frames, byte for byte
    assert np.array_equal(engine.infer_u8(frames), np.load(GOLDEN_FRAMES))
    graph, graph_serial, program = engine.graph, engine.graph_serial, engine.program
    # all 0: the camera's frames, and the input's latents where the decoder reads
    engine.set_masks(np.zeros((H, W), np.uint8))
    got = engine.infer_u8(frames)
    assert np.array_equal(got, frames) and np.array_equal(engine.frame_u8.cpu().numpy(), frames)
    assert torch.equal(engine.buffers["denoised"][:, :4].float(), engine.buffers["x0"][:, :4].float())  # (fma(0, den, x0): x0, the sign of a zero aside)
    # mixed masks, one per frame: new masks between two launches keep the capture and move the output
    masks = KM.engine_masks(B, H, W)
    engine.set_masks(masks)
    replay = engine.infer_u8(frames)
    assert engine.graph is graph and engine.graph_serial is graph_serial and engine.program is program
    assert not np.array_equal(replay, base) and not np.array_equal(replay, frames)
    assert np.array_equal(replay[masks == 0], frames[masks == 0]) and np.array_equal(engine.infer_u8(frames), replay)
    seen, raw, eager = walk(engine)
    assert seen == {"mask_latent": 1, "latent_keep": n + 1, "mask_blend": 1}
    assert np.array_equal(eager, replay) and np.array_equal(eager, blend_twin(frames, raw, masks))
    # the latent anchor did something beyond the paste: what the decoder made of the restyled part differs from the default program's
    assert not np.array_equal(raw[masks == 255], base[masks == 255])
    # I420 output: the conversion queued behind the program reads the blended frame
    engine.submit_u8(frames)
    yuv = engine.collect_i420()
    lib = L.load()
    for b in range(B):
        y, u, v = np.empty((H, W), np.uint8), np.empty((H // 2, W // 2), np.uint8), np.empty((H // 2, W // 2), np.uint8)
        rgb = np.ascontiguousarray(replay[b])
        assert lib.vsd_rgb_to_i420_host(rgb.ctypes.data, H, W, y.ctypes.data, u.ctypes.data, v.ctypes.data, W, W // 2) == 0
        assert np.array_equal(yuv[b].y, y) and np.array_equal(yuv[b].u, u) and np.array_equal(yuv[b].v, v), b
    # a slot in flight with other masks
    slot = engine.make_slot()
    slot.prepare(H, W, STEPS, 0.6, use_graph=True, keep_mask=True, **PREP)
    assert slot.mask_u8.data_ptr() != engine.mask_u8.data_ptr()
    slot.set_masks(masks[::-1])
    for e in (engine, slot):
        e.submit_u8(frames)  # both in flight, on two lanes
    assert np.array_equal(engine.collect_u8(), replay)
    other = slot.collect_u8()
    assert not np.array_equal(other, replay) and np.array_equal(other[masks[::-1] == 0], frames[masks[::-1] == 0])
    engine.set_masks(masks[::-1])
    assert np.array_equal(engine.infer_u8(frames), other)  # ... which are the frames the parent makes of those masks
    # eager engines give the replayed bytes
    engine.prepare(H, W, STEPS, 0.6, use_graph=False, keep_mask=True, **PREP)
    engine.set_masks(masks)
    assert engine.graph is None and np.array_equal(engine.infer_u8(frames), replay)


@pytest.mark.parametrize("mode", ["device_seed", "frame_options"])
def test_engine_walk_with_seeds_and_with_per_frame_options(engine, plain, mode):
    frames, _base, n = plain
    engine.prepare(H, W, STEPS, 0.6, use_graph=True, keep_mask=True, **{mode: True}, **PREP)
    masks = KM.engine_masks(B, H, W)
    engine.set_masks(masks)
    seeds = [5, 2 ** 40 + 7, 99] if mode == "device_seed" else None
    engine.submit_u8(frames, **({} if seeds is None else {"seeds": seeds}))
    replay = engine.collect_u8()
    seen, raw, eager = walk(engine, seeds)
    assert seen == {"mask_latent": 1, "latent_keep": n + 1, "mask_blend": 1}
    assert np.array_equal(eager, replay) and np.array_equal(eager, blend_twin(frames, raw, masks))
    keeps = [a for fn, a, _k in engine.program_serial.calls if fn.__name__ == "latent_keep"]
    if mode == "device_seed":
        assert all(a[3] is engine.seed_dev and a[2] is None for a in keeps[:-1])
    else:
        assert all(a[7] == engine.fo_layout.coef_stride >= 6 for a in keeps[:-1])


def test_engine_with_color_match_blends_the_matched_frame(engine, plain):
    frames, _base, _n = plain
    engine.prepare(H, W, STEPS, 0.6, use_graph=True, keep_mask=True, color_match="histogram", **PREP)
    masks = KM.engine_masks(B, H, W)
    engine.set_masks(masks)
    replay = engine.infer_u8(frames)
    names = [fn.__name__ for fn, _a, _k in engine.program_serial.calls]
    assert names[-3:] == ["postprocess_rgb", "color_match", "mask_blend"]
    _seen, raw, eager = walk(engine)
    matched = np.array(raw)
    for b in range(B):
        src = np.ascontiguousarray(frames[b])
        assert _lib().vsd_color_match_host(src.ctypes.data, matched[b].ctypes.data, H, W, 0, 256) == 0
    assert not np.array_equal(matched, raw)
    assert np.array_equal(replay, blend_twin(frames, matched, masks)) and np.array_equal(eager, replay)


# ------------------------------------------------------------------------------------------ 4. the class
def _pipeline(monkeypatch, **kw):
    """VideoSDPipeline as tests/test_dropin_gpu.py builds it (synthetic weights: no checkpoint offline), on the MINI topologies"""
    from videosd_amd import config as Cf
    from videosd_amd.pipeline import VideoSDPipeline

    monkeypatch.setattr(Cf, "SD15_UNET", Cf.MINI_UNET)
    monkeypatch.setattr(Cf, "SD15_CONTROLNET", Cf.MINI_CONTROLNET)
    monkeypatch.delenv("VSD_WEIGHTS", raising=False)
    return VideoSDPipeline(model="SimianLuo/LCM_Dreamshaper_v7", controlnet="lllyasviel/control_v11p_sd15_canny", gpus=1, compile=False, tuning_mode="table", **kw)


def test_the_class_keeps_what_the_mask_keeps(monkeypatch):
    from videosd_amd.pipeline import center_crop_resize

    opts = dict(prompt="a watercolor painting", height=H, width=W, strength=0.6, steps=STEPS, controlnet_scale=1.5)
    rng = np.random.default_rng(4)
    cams = [Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), "RGB") for _ in range(2)]  # 128 x 96, as the camera's
    sized = [np.asarray(center_crop_resize(c, W, H)) for c in cams]
    base = [np.asarray(o) for o in _pipeline(monkeypatch).infer_batch(cams, **opts)]
    p = _pipeline(monkeypatch, keep_mask=True)
    whole = [np.asarray(o) for o in p.infer_batch(cams, **opts)]
    assert all(np.array_equal(a, b) for a, b in zip(whole, base))  # no mask yet: the default pipeline's frames
    left = np.full((96, 128), 255, np.uint8)
    left[:, :64] = 0
    assert p.set_mask(Image.fromarray(left, "L")) == 1
    m = np.asarray(center_crop_resize(Image.fromarray(left, "L"), W, H))
    assert (m == 0).sum() > 64 * 20 and (m == 255).sum() > 64 * 20
    handle = p.submit_batch(cams, **opts)
    outs = [np.asarray(o) for o in p.collect_batch(handle)]
    eng, graph = handle.engine, handle.engine.graph
    assert np.array_equal(eng.mask_u8.cpu().numpy(), np.stack([m, m]))
    for b in range(2):
        assert np.array_equal(outs[b][m == 0], sized[b][m == 0]) and not np.array_equal(outs[b][m == 255], sized[b][m == 255]), b
    top = np.full((30, 40), 255, np.uint8)  # another mask, another size: the same engine and capture serve
    top[:15] = 0
    assert p.set_mask(top) == 2
    m2 = np.asarray(center_crop_resize(Image.fromarray(top, "L"), W, H))
    handle = p.submit_batch(cams, **opts)
    outs2 = [np.asarray(o) for o in p.collect_batch(handle)]
    assert handle.engine is eng and eng.graph is graph
    for b in range(2):
        assert np.array_equal(outs2[b][m2 == 0], sized[b][m2 == 0]) and not np.array_equal(outs2[b], outs[b]), b
    # one mask per frame, for this launch alone
    per = [np.asarray(o) for o in p.infer_batch(cams, masks=[Image.fromarray(left, "L"), None], **opts)]
    assert np.array_equal(per[0], outs[0]) and np.array_equal(per[1], base[1])
    again = [np.asarray(o) for o in p.infer_batch(cams, **opts)]  # ... and `set_mask`'s again behind it
    assert all(np.array_equal(a, b) for a, b in zip(again, outs2))

"""Live strength / ControlNet scale on a loaded plan and lanes that share weights (include/vsd.h vsd_plan_set_options,
vsd_plan_clone_lane, vsd_plan_memory; plan files of format 2).  Expected bits always come from the Python engine: its own
`update_options`, and an engine freshly prepared at those options.  Everything is compared bit for bit.

Shapes: the MINI nets at 64 x 64 with 2 steps -- both time tables, the constant block of a multi-step schedule and both networks are
exercised, and a case takes a few seconds."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 64
STEPS = 2
EXPORTED = (0.6, 1.5)
SLIDER = [(0.3, 1.5), (0.6, 0.4), (0.58, 2.75), (1.0, 0.05)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _weights():
    from videosd_amd import config as Cf, weights as W_

    return (W_.synthesize(W_.unet_spec(Cf.MINI_UNET), "unet.", device="cuda"), W_.synthesize(W_.controlnet_spec(Cf.MINI_CONTROLNET), "cn.", device="cuda"),
            W_.synthesize(W_.taesd_spec(Cf.TAESD), "vae.", device="cuda"))


def _embeds(seed=3):
    from videosd_amd import config as Cf

    return (torch.randn(77, Cf.MINI_UNET.cross_dim, generator=torch.Generator().manual_seed(seed)) * 0.5).half()


def _engine(batch, cn, strength, scale, choices=None):
    """tests/test_plan_gpu.py's engine: the MINI nets, prepared at the given options.  choices: the kernel-choice table of another
    engine (ops.tile_override) -- `prepare` times the candidates of every conv shape per HipOps, and two timings may pick two split-K
    forms with two summation orders; a fresh engine that is to give the same BITS takes the same choices, as two processes that load
    one tuning file do."""
    from videosd_amd import config as Cf
    from videosd_amd.engine import Engine
    from videosd_amd.ops import HipOps

    wu, wc, wv = _weights()
    eng = Engine(HipOps(0, tile_override=None if choices is None else dict(choices)), Cf.MINI_UNET, Cf.MINI_CONTROLNET, Cf.TAESD, wu, wc, wv)
    eng.set_text_embeds(_embeds())
    eng.prepare(H, W, STEPS, strength, controlnet_scale=scale, use_controlnet=cn, batch=batch)
    return eng


def _frame(batch, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3) if batch == 1 else (batch, H, W, 3), dtype=np.uint8)


class _World:
    """one exported program: the engine, its plan file and the engine's frames per option, computed once and left unchanged"""

    def __init__(self, tmp, batch, cn):
        from videosd_amd.plan import export_plan

        self.batch, self.cn = batch, cn
        self.eng = _engine(batch, cn, *EXPORTED)
        self.frame = _frame(batch)
        self.first = self.eng.infer_u8(self.frame).copy()
        self.path = str(tmp / f"b{batch}cn{int(cn)}.vsdplan")
        self.info = export_plan(self.eng, self.path)
        assert np.array_equal(self.eng.infer_u8(self.frame), self.first)  # (the export left the engine as it was)
        self._want = {EXPORTED: self.first}

    def want(self, strength, scale):
        """the engine's frame after update_options(strength, scale)"""
        key = (strength, scale)
        if key not in self._want:
            assert self.eng.update_options(strength, scale)
            self._want[key] = self.eng.infer_u8(self.frame).copy()
            assert self.eng.update_options(*EXPORTED)
        return self._want[key]


_worlds = {}


@pytest.fixture
def world(tmp_path_factory):
    def get(batch, cn):
        if (batch, cn) not in _worlds:
            _worlds[(batch, cn)] = _World(tmp_path_factory.mktemp("plans"), batch, cn)
        return _worlds[(batch, cn)]

    return get


@pytest.mark.parametrize("batch,cn", [(1, True), (2, True), (1, False)])
def test_a_slider_step_on_a_plan_gives_the_engines_bits(world, batch, cn):
    from videosd_amd.plan import CPlan

    w = world(batch, cn)
    assert w.info["options"] is True and w.info["shared_bytes"] > 0
    plan = CPlan(w.path)
    try:
        assert np.array_equal(plan.infer(w.frame), w.first)
        seen = [w.first]
        for strength, scale in (SLIDER if cn else SLIDER[2:3]):
            assert plan.set_options(strength, scale) is True
            got = plan.infer(w.frame)
            assert np.array_equal(got, w.want(strength, scale)), (strength, scale)
            fresh = _engine(batch, cn, strength, scale, choices=w.eng.ops.tile_override)
            assert np.array_equal(got, fresh.infer_u8(w.frame)), (strength, scale)
            del fresh
            assert not any(np.array_equal(got, s) for s in seen), "the options changed nothing"
            seen.append(got)
        assert plan.set_options(*EXPORTED) is True
        assert np.array_equal(plan.infer(w.frame), w.first)
    finally:
        plan.close()


def test_a_strength_that_needs_another_program_is_refused_and_changes_nothing(world):
    from videosd_amd.lcm import lcm_timesteps
    from videosd_amd.plan import CPlan

    w = world(1, True)
    assert len(lcm_timesteps(0.02, STEPS)) == 1 and w.eng.plan["n"] == 2
    plan = CPlan(w.path)
    try:
        assert plan.set_options(0.3, 1.5) is True
        assert plan.set_options(0.02, 0.7) is False
        assert np.array_equal(plan.infer(w.frame), w.want(0.3, 1.5))
        with pytest.raises(RuntimeError, match="empty LCM schedule"):
            plan.set_options(0.01, 1.0)
        assert np.array_equal(plan.infer(w.frame), w.want(0.3, 1.5))
    finally:
        plan.close()


class _Pinned:
    def __init__(self, ctx, like):
        self.ctx, self.n = ctx, like.nbytes
        self.p = ctx.lib.vsd_pinned_alloc(ctx.h, self.n)
        assert self.p
        self.a = np.ctypeslib.as_array((C.c_uint8 * self.n).from_address(self.p)).reshape(like.shape)

    def free(self):
        self.a = None
        self.ctx.lib.vsd_pinned_free(self.ctx.h, self.p)


def test_options_are_ordered_with_the_frames_on_the_plans_stream(world):
    """submit A | set_options | submit B | one wait: A has the old options' bits, B the new ones'"""
    from videosd_amd.plan import CPlan

    w = world(1, True)
    plan = CPlan(w.path)
    bufs = [_Pinned(plan.ctx, w.frame) for _ in range(4)]
    try:
        ina, outa, inb, outb = bufs
        ina.a[...] = w.frame
        inb.a[...] = w.frame
        outa.a[...] = 0
        outb.a[...] = 0
        plan.ctx.call("vsd_plan_submit", plan.h, ina.p, outa.p)
        assert plan.set_options(0.3, 1.5) is True
        plan.ctx.call("vsd_plan_submit", plan.h, inb.p, outb.p)
        plan.ctx.call("vsd_plan_wait", plan.h)
        assert np.array_equal(outa.a, w.first)
        assert np.array_equal(outb.a, w.want(0.3, 1.5))
    finally:
        plan.close()
        for b in bufs:
            b.free()


def test_lanes_share_the_weights_and_keep_their_own_options_and_prompts(world, tmp_path):
    from videosd_amd.plan import CPlan, export_prompt

    w = world(1, True)
    other = str(tmp_path / "other.vsdprompt")
    export_prompt(w.eng.build_prompt(_embeds(seed=11)), other)
    # what a single plan gives with those settings
    solo = CPlan(w.path)
    try:
        assert solo.set_options(0.58, 2.75)
        want_opts = solo.infer(w.frame)
        assert np.array_equal(want_opts, w.want(0.58, 2.75))
        assert solo.set_options(*EXPORTED)
        solo.load_prompt(other)
        want_prompt = solo.infer(w.frame)
        assert not np.array_equal(want_prompt, w.first)
    finally:
        solo.close()
    lanes = [CPlan(w.path, lane=0)]
    bufs = []
    try:
        lanes += [lanes[0].clone(lane=l) for l in (1, 2, 3)]
        owned0, shared0 = lanes[0].memory()
        assert shared0 == w.info["shared_bytes"] > 0 and owned0 > 0
        for p in lanes[1:]:
            owned, shared = p.memory()
            assert shared == w.info["shared_bytes"] and owned == (owned0 + shared0) - shared0
        total = sum(p.memory()[0] for p in lanes) + shared0
        assert 4 * (owned0 + shared0) - total == 3 * shared0
        assert lanes[1].set_options(0.58, 2.75)
        lanes[2].load_prompt(other)
        want = [w.first, want_opts, want_prompt, w.first]
        for _ in range(2):
            for p, x in zip(lanes, want):
                assert np.array_equal(p.infer(w.frame), x)
        # four frames in flight, one per lane, once
        ctx = lanes[0].ctx
        bufs = [(_Pinned(ctx, w.frame), _Pinned(ctx, w.frame)) for _ in lanes]
        for p, (i, o) in zip(lanes, bufs):
            i.a[...] = w.frame
            o.a[...] = 0
            ctx.call("vsd_plan_submit", p.h, i.p, o.p)
        for p in lanes:
            ctx.call("vsd_plan_wait", p.h)
        for (i, o), x in zip(bufs, want):
            assert np.array_equal(o.a, x)
        # the source goes first: the clones keep the weights
        lanes[0].close()
        for p, x in zip(lanes[1:], want[1:]):
            assert np.array_equal(p.infer(w.frame), x)
        # a clone starts with its source's current prompt and options
        again = lanes[1].clone(lane=0)
        lanes.append(again)
        assert np.array_equal(again.infer(w.frame), want_opts)
    finally:
        for p in lanes:
            p.close()
        for i, o in bufs:
            i.free()
            o.free()


def test_the_c_example_clones_its_lanes_and_sets_options(world, tmp_path):
    """examples/plan_host.c with `5 2 0.3 0.4`: two lanes, strength 0.3, scale 0.4 -- the engine's bits for those options"""
    w = world(2, True)
    exe = str(tmp_path / "plan_host")
    libdir = os.path.join(ROOT, "videosd_amd")
    subprocess.run(["gcc", "-O2", os.path.join(ROOT, "examples", "plan_host.c"), "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lvsd",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    (tmp_path / "in.raw").write_bytes(w.frame.tobytes())
    r = subprocess.run([exe, w.path, str(tmp_path / "in.raw"), str(tmp_path / "out.raw"), "5", "2", "0.3", "0.4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    assert "frames/s" in r.stdout and "2 lane(s)" in r.stdout
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(w.frame.shape)
    assert np.array_equal(got, w.want(0.3, 0.4))
    assert not np.array_equal(got, w.first)


def test_damaged_format_2_files_are_refused_while_parsing(world, tmp_path):
    """a call whose argument tag does not fit its entry point, another interface version, a cut inside the options section: each ends
    in a plan_load error before any GPU work, and the intact file loads afterwards"""
    from videosd_amd import lib as L, plan as P

    w = world(1, False)
    data = open(w.path, "rb").read()
    o = P.file_offsets(data)
    assert data[8:12] == (2).to_bytes(4, "little") and o["ext"] == P.HEADER_BYTES
    assert int.from_bytes(data[o["interface_version"]:o["interface_version"] + 4], "little") == L.VERSION
    assert int.from_bytes(data[o["signature_hash"]:o["signature_hash"] + 8], "little") == P.signature_hash()
    ctx = L.Context(0)
    h = C.c_void_p()

    def refused(name, blob, match):
        bad = tmp_path / name
        bad.write_bytes(blob)
        with pytest.raises(RuntimeError, match=match):
            ctx.call("vsd_plan_load", str(bad).encode(), C.byref(h))

    at = o["first_arg"]
    tag = int.from_bytes(data[at:at + 4], "little")
    fn = int.from_bytes(data[o["calls"]:o["calls"] + 4], "little")
    assert P.signature_tags()[fn].split(":")[1][0] == {P.T_I32: "i", P.T_F32: "f", P.T_PTR: "p", P.T_DESC: "d"}[tag]
    swapped = P.T_I32 if tag != P.T_I32 else P.T_PTR
    refused("tag.vsdplan", data[:at] + swapped.to_bytes(4, "little") + data[at + 4:], "plan_load: an argument tag that does not fit")
    v = o["interface_version"]
    refused("iface.vsdplan", data[:v] + (L.VERSION + 1).to_bytes(4, "little") + data[v + 4:], "plan_load: written for another interface version")
    s = o["signature_hash"]
    refused("hash.vsdplan", data[:s] + (P.signature_hash() ^ 1).to_bytes(8, "little") + data[s + 8:], "plan_load: written against other entry point signatures")
    assert o["options"] + 20 < o["options_end"]
    refused("cut.vsdplan", data[:o["options"] + 20], "plan_load: truncated options section")
    refused("cut2.vsdplan", data[:o["options_end"] - 4], "plan_load: truncated options section")
    ctx.call("vsd_plan_load", w.path.encode(), C.byref(h))
    ctx.lib.vsd_plan_free(ctx.h, h)


def test_a_format_1_file_still_loads_and_says_why_it_has_no_live_options(world, tmp_path):
    """the version 1 layout of the same program: no extension, no region flags"""
    from videosd_amd import plan as P

    w = world(1, False)
    data = open(w.path, "rb").read()
    o = P.file_offsets(data)
    nreg = int.from_bytes(data[24:28], "little")
    table = bytearray(data[o["regions"]:o["calls"]])
    for i in range(nreg):
        table[i * P.REGION_BYTES + 12:i * P.REGION_BYTES + 16] = bytes(4)
    old = tmp_path / "v1.vsdplan"
    old.write_bytes(data[:8] + (1).to_bytes(4, "little") + data[12:P.HEADER_BYTES] + bytes(table) + data[o["calls"]:])
    plan = P.CPlan(str(old))
    try:
        assert np.array_equal(plan.infer(w.frame), w.first)
        assert plan.memory()[1] == 0
        with pytest.raises(RuntimeError, match="format version 1"):
            plan.set_options(0.3, 1.0)
        twin = plan.clone()
        try:
            assert np.array_equal(twin.infer(w.frame), w.first) and twin.memory() == plan.memory()
        finally:
            twin.close()
    finally:
        plan.close()

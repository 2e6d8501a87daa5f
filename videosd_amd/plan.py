"""A prepared frame program as a FILE that a host without Python can run (include/vsd.h vsd_plan_load / vsd_plan_infer).

SURVEY.md section 8b sketched whole-frame C entry points (vsd_load_weights / vsd_prepare / vsd_infer); the sequencing of a frame lives
in engine.py, so rounds 1-5 exported ops only and a non-Python host could not drive a frame (missing #3).  This closes
that without a second engine: `export_plan(engine, path)` runs the engine's one-stream program ONCE with every C-ABI call recorded
-- entry point, scalar arguments, descriptors -- and every device pointer rewritten as (region, offset): a region is one allocation
of the process (weights, per-plan constants, the prompt block, counters, I/O buffers: saved with their bytes; activations and
workspaces: size only).  `vsd_plan_load` allocates the regions, uploads the saved bytes, patches the pointers, replays the calls
under stream capture and keeps the graph; `vsd_plan_infer` is upload, launch, download.  Same kernels, same arguments: the frame a plan
produces is bit for bit the engine's (tests/test_plan_gpu.py).

A plan is one (size, steps, frames per launch): prompt (`export_prompt` / vsd_plan_load_prompt), strength and ControlNet scale
(vsd_plan_set_options) change on the loaded plan -- and, for an engine prepared with device_seed, the seed of every frame of a launch
(vsd_plan_set_seeds).  That needs no field in the file: the loader finds the seed buffer as the `seeds_dev` argument of the program's
vsd_add_noise_seeded call, a region of the plan's own like every other constant.

LIVE OPTIONS.  Three things in a prepared program depend on strength / controlnet_scale, all written by Engine._write_constants: the
fp32 constant block, and per network the per-step time-embedding table.  LCM timesteps take only the 50 values 19, 39, ... 999, so
`export_plan` computes, with the engine's own code, a 50-row time table per network (Engine._time_embeddings in chunks of exactly n
rows -- the launch shape, and so the tuned kernel form and split, of the engine's own call: a row is bit for bit what the engine writes
for that timestep), a coefficient table fp32 [50][6] (sqrt(a_t), sqrt(1 - a_t), c_skip, c_out and the two add-noise values, from
lcm.LCMSchedule.step_coef / add_noise_coef) followed by fp32 logspace(-1, 0, nres), and records where the live block and tables sit.
vsd_plan_set_options picks rows: one small launch, stream-ordered.

LANES.  Regions that hold network weight tensors and nothing else (found by walking the engine's NetWeights / TAESDWeights) are
flagged read-only: vsd_plan_clone_lane shares them between the plans of a process instead of uploading them once per lane.

File (little endian), format version 2 (FORMAT_VERSION; VERSION = 1 names the base layout both versions share: the fixed fields, the
region records and the call encoding, which did not change): "VSDPLAN1", u32 version, H, W, batch, n_regions, n_calls, u32 in_region, u64 in_offset, u32
out_region, u64 out_offset, u32 prompt_region, u64 prompt_offset, u64 prompt_bytes (the engine's prompt block: vsd_plan_load_prompt
replaces its bytes with another prompt's, `export_prompt`) -- HEADER_BYTES = 76, as in version 1.  Version 2 puts its EXTENSION right
behind these fixed fields, in front of the region table (the loader has everything it checks before it allocates, and a reader of the
fixed fields finds them where version 1 had them): u32 bytes of the extension that follow, u32 interface version (lib.VERSION), u64
signature hash (FNV-1a of `signature_tags()`), then the options section: u32 n (timesteps of the program), u32 steps, u32 nres, u32
number of time tables, f64 strength, f64 controlnet_scale (as exported), u32 region of the live constant block, u32 region of the
coefficient table, u64 offset of each, then per time table (unet, cn, ref as the program has them) u32 region of the 50-row table, u32
region of the live table, u64 offset of each, u64 row stride of the live table, u64 row bytes (= the 50-row table's stride).
Regions: u64 size, u32 saved, u32 flags (bit 0: read-only network weights, shareable between lanes; version 1: 0).  Calls: u32 entry
point (PLAN_FUNCS index), u32 nargs, args of 16 bytes
(u32 tag, u32 aux, u64 value): 0 int32, 1 float32 bits, 2 pointer (aux = region, value = offset), 3 null, 4 the plan's stream,
5 descriptor array (aux = count, value = bytes; followed by the bytes, u32 nfix, nfix x (u32 byte offset, u32 region, u64 offset));
then the bytes of the saved regions in order.  `file_offsets` finds the parts of a file.  Version 1 files (no extension, no flags)
still load; they have no live options and share nothing."""
import bisect
import ctypes as C
import struct

import numpy as np
import torch

from . import lib as L

MAGIC = b"VSDPLAN1"
VERSION = 1               # the base layout (magic, fixed fields, region records, calls): what every reader of either version parses
FORMAT_VERSION = 2        # what `export_plan` writes: the base layout plus the extension and the region flags
HEADER_BYTES = 76         # the fixed fields (both versions)
EXT_FIXED_BYTES = 16      # version 2, behind them: u32 bytes that follow, u32 interface version, u64 signature hash ...
OPT_FIXED_BYTES = 56      # ... and the options section: its fixed part,
OPT_TABLE_BYTES = 40      # and one record per time table
REGION_BYTES = 16         # a region record
ARG_BYTES = 16            # an argument of a call (after the call's u32 entry point, u32 nargs)
REGION_SHARED = 1         # region flag, bit 0: read-only network weights, shareable between lanes
OPT_ROWS = 50             # timesteps an LCM schedule can hold: 19, 39, ... 999
OTHER_PROGRAM = 1         # include/vsd.h VSD_PLAN_OTHER_PROGRAM
# entry points a frame program may call, by id (csrc/plan_dispatch.inc is generated from this list: scripts/gen_plan_dispatch.py)
PLAN_FUNCS = ["vsd_preprocess_rgb", "vsd_sobel_control", "vsd_conv_gemm", "vsd_conv_gemm_group", "vsd_pair_begin", "vsd_pair_join",
              "vsd_pair_end", "vsd_groupnorm", "vsd_groupnorm_batched", "vsd_attention", "vsd_attention_batched", "vsd_tail_a", "vsd_tail_b",
              "vsd_add_noise_dev", "vsd_lcm_step_dev", "vsd_postprocess_rgb", "vsd_adain", "vsd_layernorm",
              # (new entry points go to the END: the ids of the ones above are in every plan file written so far)
              "vsd_add_noise_seeded", "vsd_lcm_step_seeded"]
T_I32, T_F32, T_PTR, T_NULL, T_STREAM, T_DESC = range(6)


def signature_tags():
    """per PLAN_FUNCS entry "name:tags", one letter per argument after the context: p pointer, i int32, f float, d descriptor array,
    o optional int output (null in a plan) -- what vsd_plan_load checks a recorded call against (csrc/plan_dispatch.inc)"""
    letter = {C.c_void_p: "p", C.c_int: "i", C.c_int32: "i", C.c_float: "f", C.POINTER(L.ConvDesc): "d", C.POINTER(C.c_int): "o"}
    return [name + ":" + "".join(letter[t] for t in L.SIGNATURES[name][1][1:]) for name in PLAN_FUNCS]


def signature_hash() -> int:
    """64-bit FNV-1a of the lines of `signature_tags`, each followed by a newline: a file written against other signatures is refused"""
    h = 0xCBF29CE484222325
    for b in "".join(line + "\n" for line in signature_tags()).encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def file_offsets(data: bytes) -> dict:
    """byte offsets of the parts of a plan file's head: the extension and its fields (version 2), the region table, the call list"""
    version, = struct.unpack_from("<I", data, 8)
    nreg, = struct.unpack_from("<I", data, 24)
    o = {"version": 8, "ext": None, "interface_version": None, "signature_hash": None, "options": None, "options_end": None}
    regions = HEADER_BYTES
    if version >= 2:
        ext, = struct.unpack_from("<I", data, HEADER_BYTES)
        o.update(ext=HEADER_BYTES, interface_version=HEADER_BYTES + 4, signature_hash=HEADER_BYTES + 8, options=HEADER_BYTES + EXT_FIXED_BYTES)
        regions = HEADER_BYTES + 4 + ext
        o["options_end"] = regions
    o["regions"] = regions
    o["calls"] = regions + nreg * REGION_BYTES
    o["first_arg"] = o["calls"] + 8  # (u32 tag, u32 aux, u64 value) of the first call's first argument
    return o


_PTR_FIELDS = [(name, getattr(L.ConvDesc, name).offset) for name, t in L.ConvDesc._fields_ if t is C.c_void_p]


class _Regions:
    """the process's live device allocations (torch's caching allocator) that the program points into"""

    def __init__(self, device):
        blocks = []
        for seg in torch.cuda.memory_snapshot():
            if seg.get("device", 0) != device:
                continue
            addr = seg["address"]
            for b in seg["blocks"]:
                if b["state"].startswith("active"):
                    blocks.append((b.get("address", addr), b["size"]))
                addr += b["size"]
        blocks.sort()
        self.starts = [a for a, _ in blocks]
        self.blocks = blocks
        self.used = {}  # block index -> region id

    def find(self, ptr: int):
        """index of the allocation that holds `ptr` (None: no live one)"""
        i = bisect.bisect_right(self.starts, ptr) - 1
        return None if i < 0 or ptr >= self.blocks[i][0] + self.blocks[i][1] else i

    def locate(self, ptr: int):
        i = self.find(ptr)
        if i is None:
            raise RuntimeError(f"plan export: device pointer {ptr:#x} lies in no live allocation of this process")
        rid = self.used.setdefault(i, len(self.used))
        return rid, ptr - self.blocks[i][0]


class _LibProxy:
    """the ctypes library with vsd_pair_end recorded (HipOps.pair calls it past Context.call)"""

    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "vsd_pair_end":
            return fn

        def pair_end(h, joined):
            self._rec("vsd_pair_end", (None,))
            return fn(h, joined)

        return pair_end


def _weight_tensors(obj, seen):
    """every tensor reachable from a NetWeights / TAESDWeights object (its packed layers, norms, raw cross-attention weights) -- not
    through `ops`, which holds workspaces"""
    if obj is None or id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _weight_tensors(v, seen)
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _weight_tensors(v, seen)
    elif type(obj).__module__.startswith(__package__ + ".") and hasattr(obj, "__dict__"):
        for k, v in vars(obj).items():
            if k != "ops":
                yield from _weight_tensors(v, seen)


def option_coefficients(nres: int) -> torch.Tensor:
    """fp32 [50][6] per timestep 19, 39, ... 999 -- sqrt(a_t), sqrt(1 - a_t), c_skip, c_out, the two add-noise values, by
    lcm.LCMSchedule.step_coef / add_noise_coef themselves -- followed by logspace(-1, 0, nres): what vsd_plan_set_options builds the
    constant block of any schedule from (step i takes columns 0..3 of its timestep's row and columns 0..1 of the next step's)"""
    from .blocks import controlnet_scales
    from .lcm import LCMSchedule, lcm_timesteps

    sched = LCMSchedule(1.0, 1)
    rows = []
    for t in sorted(lcm_timesteps(1.0, OPT_ROWS)):
        sched.timesteps = [t]
        rows.append(list(sched.step_coef(0)[:4]) + list(sched.add_noise_coef()))
    return torch.cat([torch.tensor(rows, dtype=torch.float32).reshape(-1), controlnet_scales(nres, 1.0)])


def _option_tables(engine):
    """The option-dependent constants of EVERY schedule the program can run (module docstring, LIVE OPTIONS), by the code that computes
    them for one schedule today: [(name, live table, 50-row table)], the coefficient table with the logspace behind it, nres."""
    from .lcm import LCMSchedule, lcm_timesteps

    ops, p = engine.ops, engine.plan
    n = p["n"]
    every = sorted(lcm_timesteps(1.0, OPT_ROWS))  # 19, 39, ... 999: row j holds timestep 20 j + 19
    assert len(every) == OPT_ROWS and all(t == 20 * j + 19 for j, t in enumerate(every))
    sched = LCMSchedule(1.0, 1)
    nets = [(name, net, True) for name, net in engine._networks(p["cn"])]
    if engine.shared.get("ref_mode"):
        nets.append(("ref", engine.unet, False))
    tables = []
    for name, net, use_cond in nets:
        live = engine.shared["temb"][name]
        table = ops.zeros(OPT_ROWS, live.shape[1], dtype=live.dtype)
        chunk = ops.zeros(*live.shape, dtype=live.dtype)  # an allocation like the live table: the engine's own launch
        for r0 in range(0, OPT_ROWS, n):
            ts = every[r0:r0 + n]
            sched.timesteps = ts + [ts[-1]] * (n - len(ts))
            engine._time_embeddings(net, sched, chunk, use_cond=use_cond)
            with torch.cuda.stream(ops.stream):
                table[r0:r0 + len(ts)].copy_(chunk[:len(ts)])
        tables.append((name, live, table))
    nres = engine._nres()
    coef_dev = ops.to_device(option_coefficients(nres))
    ops.synchronize()
    return tables, coef_dev, nres


def export_plan(engine, path: str) -> dict:
    """Write the prepared engine's program (one-stream form) to `path`.  The engine must have run a frame (prompt installed)."""
    from .engine import Engine

    ops = engine.ops
    if engine.plan is None:
        raise RuntimeError("export_plan: prepare the engine first")
    if engine.plan.get("frame_prompts"):
        raise ValueError("export_plan: this engine was prepared with frame_prompts=True; a plan file holds ONE prompt's constants (per-frame "
                         "prompts have no C entry point yet): export the plan of an engine prepared without it")
    if engine.plan.get("frame_options"):
        raise ValueError("export_plan: this engine was prepared with frame_options=True; its program calls vsd_add_noise_frames, vsd_lcm_step_frames, "
                         "vsd_groupnorm_addvec and vsd_cn_merge_frames, which are not plan functions: export the plan of an engine prepared "
                         "without it (a loaded plan follows strength / ControlNet scale through vsd_plan_set_options)")
    if engine.plan.get("edge_mode", "sobel") != "sobel":
        raise ValueError(f'export_plan: this engine was prepared with edges="{engine.plan["edge_mode"]}"; its program calls vsd_canny_control, which is not a '
                         'plan function: export the plan of an engine prepared with edges="sobel" (the default)')
    if engine.plan.get("color_match") is not None:
        raise ValueError(f'export_plan: this engine was prepared with color_match="{engine.plan["color_match"]}"; its program calls vsd_color_match, which is '
                         'not a plan function: export the plan of an engine prepared with color_match=None (the default)')
    if engine.plan.get("edge_blur") or engine.plan.get("mask_feather"):
        on = " and ".join(k for k in ("edge_blur", "mask_feather") if engine.plan.get(k))
        raise ValueError(f"export_plan: this engine was prepared with {on}; its program calls vsd_gauss_blur, which is not a plan function: "
                         "export the plan of an engine prepared without it")
    if engine.plan.get("keep_mask"):
        raise ValueError("export_plan: this engine was prepared with keep_mask=True; its program calls vsd_mask_latent, vsd_latent_keep and "
                         "vsd_mask_blend, which are not plan functions: export the plan of an engine prepared without it")
    ops.synchronize()
    calls = []

    def rec(name, args):
        calls.append((name, args))

    ctx = ops.ctx
    orig_call, orig_lib = ctx.call, ctx.lib

    def recording_call(name, *args):
        rec(name, args)
        return orig_call(name, *args)

    ctx.call, ctx.lib = recording_call, _LibProxy(orig_lib, rec)
    try:
        if hasattr(ops, "tune_mode"):
            ops.tune_mode = 1 if engine.tune_for_lanes else 0
        with torch.cuda.stream(ops.stream):
            for fn, a, k in engine.program_serial.calls:
                if getattr(fn, "__name__", "") in Engine.SYNC_OPS:
                    continue
                fn(*a, **k)
        ops.synchronize()
    finally:
        ctx.call, ctx.lib = orig_call, orig_lib
    tables, coef_dev, nres = _option_tables(engine)
    regs = _Regions(ops.device.index if hasattr(ops.device, "index") and ops.device.index is not None else 0)
    stream = ops.s.value
    if not stream:
        raise RuntimeError("plan export: the engine launches on the null stream")
    body = bytearray()
    for name, args in calls:
        if name not in PLAN_FUNCS:
            raise RuntimeError(f"plan export: the program calls {name}, which a plan cannot hold")
        types = L.SIGNATURES[name][1][1:]
        if len(types) != len(args):
            raise RuntimeError(f"plan export: {name} recorded with {len(args)} arguments, declared with {len(types)}")
        body += struct.pack("<II", PLAN_FUNCS.index(name), len(args))
        for t, v in zip(types, args):
            if t is C.c_void_p:
                v = v.value if isinstance(v, C.c_void_p) else v
                if v is None or v == 0:
                    body += struct.pack("<IIQ", T_NULL, 0, 0)
                elif int(v) == stream:
                    body += struct.pack("<IIQ", T_STREAM, 0, 0)
                else:
                    rid, off = regs.locate(int(v))
                    body += struct.pack("<IIQ", T_PTR, rid, off)
            elif t in (C.c_int, C.c_int32):
                body += struct.pack("<IIq", T_I32, 0, int(v))
            elif t is C.c_float:
                body += struct.pack("<IIQ", T_F32, 0, struct.unpack("<I", struct.pack("<f", float(v)))[0])
            elif t == C.POINTER(C.c_int):
                body += struct.pack("<IIQ", T_NULL, 0, 0)  # (vsd_pair_end's optional output)
            elif t == C.POINTER(L.ConvDesc):
                obj = v._obj if hasattr(v, "_obj") else v  # byref(desc) | an array of descriptors
                count = len(obj) if isinstance(obj, C.Array) else 1
                raw = C.string_at(C.addressof(obj), C.sizeof(obj))
                fix = []
                for j in range(count):
                    d = obj[j] if count > 1 or isinstance(obj, C.Array) else obj
                    for fname, foff in _PTR_FIELDS:
                        p = getattr(d, fname)
                        if p:
                            rid, off = regs.locate(int(p))
                            fix.append((j * C.sizeof(L.ConvDesc) + foff, rid, off))
                body += struct.pack("<IIQ", T_DESC, count, len(raw)) + raw + struct.pack("<I", len(fix))
                for boff, rid, off in fix:
                    body += struct.pack("<IIQ", boff, rid, off)
            else:
                raise RuntimeError(f"plan export: {name}: argument type {t} has no plan encoding")
    pr_r, pr_off = regs.locate(engine.pblock.buf.data_ptr())
    in_r, in_off = regs.locate(engine.frame_u8.data_ptr())
    out_r, out_off = regs.locate(engine.out_u8.data_ptr())
    # what is scratch (no bytes saved): the activation arena and the op workspaces
    scratch = {t.data_ptr() for t in engine.arena.chunks}
    scratch |= {t.data_ptr() for t in ops._ws.values()}
    p = engine.plan
    # the options section: where the live constants sit and where the tables to pick their rows from
    consts = engine.shared["consts"]
    c_r, c_off = regs.locate(consts.data_ptr())
    k_r, k_off = regs.locate(coef_dev.data_ptr())
    opts = struct.pack("<IIIIdd", p["n"], p["steps"], nres, len(tables), float(p["strength"]), float(p["cn_scale"]))
    opts += struct.pack("<IIQQ", c_r, k_r, c_off, k_off)
    for name, live, table in tables:
        t_r, t_off = regs.locate(table.data_ptr())
        l_r, l_off = regs.locate(live.data_ptr())
        assert live.stride(1) == 1 and table.is_contiguous()
        opts += struct.pack("<IIQQQQ", t_r, l_r, t_off, l_off, live.stride(0) * live.element_size(), table.shape[1] * table.element_size())
    assert len(opts) == OPT_FIXED_BYTES + OPT_TABLE_BYTES * len(tables)
    ext = struct.pack("<IQ", L.VERSION, signature_hash()) + opts
    # what may be shared between lanes: allocations that hold a network's weight tensor -- and are nothing the program writes
    private = [engine.pblock.buf, consts, coef_dev, engine.noise, engine.seed_dev, engine.frame_u8, engine.out_u8, engine.edge_u8, engine.noise_ref,
               engine.ref_u8] + [t for _, live, table in tables for t in (live, table)] + list(engine.shared["temb"].values())
    never = {regs.find(t.untyped_storage().data_ptr()) for t in private if t is not None} | {regs.find(s) for s in scratch}
    seen = set()
    weights = {regs.find(t.untyped_storage().data_ptr()) for net in (engine.unet, engine.cn, engine.vae) for t in _weight_tensors(net, seen) if t.is_cuda}
    shared = (weights - never) & set(regs.used)
    order = sorted(regs.used.items(), key=lambda kv: kv[1])
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<IIIIII", FORMAT_VERSION, p["H"], p["W"], p["batch"], len(order), len(calls)))
        f.write(struct.pack("<IQIQ", in_r, in_off, out_r, out_off))
        f.write(struct.pack("<IQQ", pr_r, pr_off, engine.pblock.buf.numel()))
        assert f.tell() == HEADER_BYTES
        f.write(struct.pack("<I", len(ext)) + ext)
        saved = []
        for bi, rid in order:
            addr, size = regs.blocks[bi]
            keep = not any(addr <= s < addr + size for s in scratch)
            saved.append(keep)
            f.write(struct.pack("<QII", size, int(keep), REGION_SHARED if keep and bi in shared else 0))
        f.write(body)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for (bi, rid), keep in zip(order, saved):
            if not keep:
                continue
            addr, size = regs.blocks[bi]
            host = np.empty(size, dtype=np.uint8)
            rc = hip.hipMemcpy(host.ctypes.data, addr, size, 2)  # hipMemcpyDeviceToHost
            if rc != 0:
                raise RuntimeError(f"plan export: hipMemcpy of a {size}-byte region failed ({rc})")
            f.write(host.tobytes())
    return {"regions": len(order), "saved_bytes": sum(regs.blocks[bi][1] for (bi, _), k in zip(order, saved) if k),
            "scratch_bytes": sum(regs.blocks[bi][1] for (bi, _), k in zip(order, saved) if not k), "calls": len(calls),
            "shared_bytes": sum(regs.blocks[bi][1] for (bi, _), k in zip(order, saved) if k and bi in shared), "options": True}


PROMPT_MAGIC = b"VSDPRMT1"


def export_prompt(pblock, path: str) -> int:
    """Another prompt's constants (an engine.PromptBlock: cross-attention K / V^T of every layer and the folded weights, built on the GPU
    from the text encoder's output) as a file for vsd_plan_load_prompt: a C host changes the prompt of a loaded plan without a new plan.
    The block must have the plan's layout (same networks, same text length)."""
    data = pblock.buf.cpu().numpy().tobytes()
    with open(path, "wb") as f:
        f.write(PROMPT_MAGIC + struct.pack("<Q", len(data)) + data)
    return len(data)


class CPlan:
    """vsd_plan_load / vsd_plan_infer through ctypes (tests, examples): what a C host does with a plan file"""

    def __init__(self, path: str, device_id: int = 0, lane: int = -1, _clone_of=None):
        h = C.c_void_p()
        if _clone_of is None:
            self.ctx = L.Context(device_id)
            self.ctx.call("vsd_plan_load_lane", path.encode(), lane, C.byref(h))
        else:  # (a clone lives in its source's context)
            self.ctx = _clone_of.ctx
            self.ctx.call("vsd_plan_clone_lane", _clone_of.h, lane, C.byref(h))
        self.h = h
        dims = (C.c_int * 3)()
        self.ctx.call("vsd_plan_info", self.h, dims)
        self.H, self.W, self.batch = int(dims[0]), int(dims[1]), int(dims[2])

    def infer(self, frame: np.ndarray) -> np.ndarray:
        want = (self.H, self.W, 3) if self.batch == 1 else (self.batch, self.H, self.W, 3)
        if frame.shape != want or frame.dtype != np.uint8:
            raise ValueError(f"frame must be uint8 {want}")
        frame = np.ascontiguousarray(frame)
        out = np.empty_like(frame)
        self.ctx.call("vsd_plan_infer", self.h, frame.ctypes.data, out.ctypes.data)
        return out

    def infer_frame(self, frame: np.ndarray) -> np.ndarray:
        """vsd_plan_infer_frame: camera frame(s) of any size, uint8 [h][w][3] ([batch][h][w][3] of one size), cropped and resampled on the device"""
        nd = 3 if self.batch == 1 else 4
        if frame.dtype != np.uint8 or frame.ndim != nd or frame.shape[-1] != 3 or (nd == 4 and frame.shape[0] != self.batch):
            raise ValueError("frame must be uint8 [h][w][3]" if nd == 3 else f"frames must be uint8 [{self.batch}][h][w][3]")
        frame = np.ascontiguousarray(frame)
        out = np.empty((self.H, self.W, 3) if self.batch == 1 else (self.batch, self.H, self.W, 3), np.uint8)
        h, w = frame.shape[-3], frame.shape[-2]
        self.ctx.call("vsd_plan_infer_frame", self.h, frame.ctypes.data, h, w, 3 * w, out.ctypes.data)
        return out

    def infer_frame_i420(self, frame):
        """vsd_plan_infer_frame_i420: `frames.I420Frame` camera frame(s) of any size (a list of `batch` frames of one size) in, I420Frame(s)
        of the plan's size out -- planes up, packed I420 down, converted on the device"""
        from .frames import I420Frame

        frames = [frame] if isinstance(frame, I420Frame) else list(frame)
        if len(frames) != self.batch or not all(isinstance(f, I420Frame) and f.size == frames[0].size for f in frames):
            raise ValueError(f"{self.batch} I420Frame(s) of one size")
        w, h = frames[0].size
        ch, cw = (h + 1) // 2, (w + 1) // 2
        y = np.ascontiguousarray(np.stack([f.y for f in frames]))
        u = np.ascontiguousarray(np.stack([f.u for f in frames]))
        v = np.ascontiguousarray(np.stack([f.v for f in frames]))
        one = self.H * self.W * 3 // 2
        out = np.empty(self.batch * one, np.uint8)
        self.ctx.call("vsd_plan_infer_frame_i420", self.h, y.ctypes.data, w, u.ctypes.data, v.ctypes.data, cw, h, w, out.ctypes.data)
        res = [I420Frame(out[i * one:(i + 1) * one].copy(), self.W, self.H) for i in range(self.batch)]
        return res[0] if self.batch == 1 else res

    def load_prompt(self, path: str):
        self.ctx.call("vsd_plan_load_prompt", self.h, path.encode())

    def set_options(self, strength: float, controlnet_scale: float) -> bool:
        """vsd_plan_set_options: Engine.update_options for a loaded plan -- stream-ordered, no re-capture.  False (and nothing changed)
        when the strength needs another program: another number of timesteps than the plan's."""
        rc = self.ctx.lib.vsd_plan_set_options(self.ctx.h, self.h, float(strength), float(controlnet_scale))
        if rc == OTHER_PROGRAM:
            return False
        self.ctx.check(rc, "vsd_plan_set_options")
        return True

    def set_seeds(self, seeds):
        """vsd_plan_set_seeds: one seed per frame of the launch (an int: the same for all) for the frames submitted from now on --
        stream-ordered, no re-capture.  Only a plan exported from an engine prepared with device_seed has seeds."""
        vals = [seeds] * self.batch if isinstance(seeds, (int, np.integer)) else list(seeds)
        arr = (C.c_uint64 * len(vals))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in vals])
        self.ctx.call("vsd_plan_set_seeds", self.h, arr, len(vals))

    def clone(self, lane: int = -1) -> "CPlan":
        """vsd_plan_clone_lane: a further plan of this program on launch stream `lane` that shares this one's weights; it starts with
        this plan's current prompt and options and keeps its own afterwards"""
        return CPlan(None, lane=lane, _clone_of=self)

    def memory(self):
        """vsd_plan_memory: (bytes of the regions this plan owns, bytes of the regions it shares with its clones)"""
        out = (C.c_uint64 * 2)()
        self.ctx.call("vsd_plan_memory", self.h, out)
        return int(out[0]), int(out[1])

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.vsd_plan_free(self.ctx.h, self.h)
            self.h = None

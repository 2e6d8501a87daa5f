"""HipOps: the op interface the engine is written against, bound to libvsd.so through ctypes.

Tensors are torch CUDA(ROCm) tensors used purely as device buffers (`.data_ptr()`); every compute
call goes through the C-ABI of include/vsd.h on `self.stream`.
"""
import ctypes as C
import json
import time
from dataclasses import dataclass
from functools import partial
from typing import Optional

import torch

from . import convform as CF
from . import lib as L
from .convform import choose_tile  # noqa: F401  (scripts import it from here)
from .packing import PackedConv

import os as _os

POISON = bool(_os.environ.get("VSD_POISON"))


@dataclass(frozen=True)
class Geom:
    """Spatial geometry of one implicit-GEMM conv: stored source size, logical (resized) input size, output size."""
    hs: int
    ws: int
    hi: int
    wi: int
    ho: int
    wo: int
    ksize: int = 1
    stride: int = 1
    pad: int = 0
    batch: int = 1  # images stacked along M (frames of independent streams sharing one launch)

    @staticmethod
    def linear(rows: int, batch: int = 1) -> "Geom":
        """`rows` per image; a plain GEMM does not care where one image ends (batch only matters to a transposed
        output, which keeps each image in its own column slab)."""
        return Geom(1, rows, 1, rows, 1, rows, 1, 1, 0, batch)

    @staticmethod
    def conv(h: int, w: int, ksize=3, stride=1, up_to=None, batch=1) -> "Geom":
        hi, wi = (h, w) if up_to is None else up_to
        pad = ksize // 2
        ho = (hi + 2 * pad - ksize) // stride + 1
        wo = (wi + 2 * pad - ksize) // stride + 1
        return Geom(h, w, hi, wi, ho, wo, ksize, stride, pad, batch)

    @property
    def m(self) -> int:
        return self.batch * self.ho * self.wo


class LaneBook:
    """What the HipOps objects of one process and device share about launch lanes: which lanes have a live object (weak
    references: a dropped slot gives its lane back), and the helper objects the throughput-mode tuner times candidates with."""

    def __init__(self):
        import weakref

        self._weakref = weakref
        self.users = {}          # lane -> WeakSet of HipOps
        self.tune_helpers = {}   # lane -> HipOps kept for HipOps._time_candidates_on_lanes (made once per process)
        self.warned = False

    def register(self, ops: "HipOps"):
        self.users.setdefault(ops.lane, self._weakref.WeakSet()).add(ops)

    def next_free(self) -> int:
        """the lowest lane no live object runs on; when all four launch streams have one, lanes are shared round-robin (their
        objects then take turns on a stream: said once, since engines meant to run side by side would not)"""
        for lane in range(L.POOL_STREAMS):
            if not len(self.users.get(lane, ())):
                return lane
        if not self.warned:
            self.warned = True
            import warnings

            warnings.warn(f"HipOps.clone(): all {L.POOL_STREAMS} launch lanes have a live object; further auto-numbered clones share a lane's "
                          "streams with an existing one and take turns with it (pass lane= to choose)")
        return min(range(L.POOL_STREAMS), key=lambda l: len(self.users.get(l, ())))


class HipOps:
    name = "hip"

    def __init__(self, device_id: int = 0, stream: Optional[torch.cuda.Stream] = None, make_current: bool = True,
                 tile_override: Optional[dict] = None, lane: int = 0, _lanes: Optional[LaneBook] = None, _register: bool = True):
        if not torch.cuda.is_available():
            raise RuntimeError("HipOps needs a ROCm GPU; there is no CPU fallback in the product path")
        self.device = torch.device("cuda", device_id)
        torch.cuda.set_device(self.device)
        self.ctx = L.Context(device_id)
        # Launch lanes.  Everything that can be in flight at once on this GPU must sit on a hardware queue AND a command-processor
        # pipe of its own; with plain streams both are accidents of what the process created before (DESIGN.md section 3,
        # "launches in flight").  libvsd keeps four launch streams per process and device (vsd_stream_pool: four queues on four
        # pipes); lane l launches on pool stream l mod 4 and runs its side branch (the ControlNet encoder beside the UNet
        # encoder) on stream (l + 2) mod 4: two lanes with side branches, or four lanes without, never share a pipe.
        # VSD_STREAMS=plain takes torch's pool streams instead (A/B measurements only).
        self.lane = int(lane)
        self._lanes = _lanes if _lanes is not None else LaneBook()  # shared with every clone
        self._plain = _os.environ.get("VSD_STREAMS") == "plain"
        if stream is not None:
            self.streams = [stream, torch.cuda.Stream(device=self.device)]
        elif self._plain:
            self.streams = [torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)]
        else:
            pool = self.pool_streams()
            self.streams = [pool[self.lane % L.POOL_STREAMS], pool[(self.lane + 2) % L.POOL_STREAMS]]
        self.stream = self.streams[0]
        if _register:  # (the tuner's helper objects do not occupy a lane)
            self._lanes.register(self)
        # torch-side plumbing (allocation fills, H2D/D2H copies) must be ordered with the kernels: make the
        # kernel stream this thread's current torch stream.
        if make_current:
            torch.cuda.set_stream(self.stream)
        self.device_id = device_id
        self._sidx = 0
        self._widx = None  # scratch set of the call being issued when it is not the stream's own (members of a pair / group)
        self._events = {}
        self._ws = {}
        self.tile_override = {} if tile_override is None else tile_override
        # 0: kernel choices timed alone (latency), 1: timed with four lanes busy (throughput).  Set by Engine.prepare for the plan
        # it records / captures; part of the tuning key.
        self.tune_mode = 0
        # timing with four lanes busy takes ~80 s per plan: done offline (scripts/retune_all.py sets this) or on request
        # (VSD_TUNE_LANES=1); a live worker that meets a shape the table has no throughput-mode entry for takes the alone-timed
        # choice (a second or two per plan, as before) instead of stalling a stream for minutes
        self.tune_lanes_online = bool(_os.environ.get("VSD_TUNE_LANES"))
        self.inkernel_splitk = True
        self.one_launch_bias_us = float(_os.environ.get("VSD_ONE_LAUNCH_BIAS_US", "0.5"))  # tune_conv: see there
        self.no_halo = bool(__import__("os").environ.get("VSD_NO_HALO"))  # debugging: run halo-tuned shapes on the generic ring
        self.default_pipeline = 3
        self.no_c64 = bool(_os.environ.get("VSD_NO_C64"))  # (development: keep the persistent 64-channel conv form out of the tuner / the plans)
        self.no_w8 = bool(_os.environ.get("VSD_NO_W8"))  # (development: keep the eight-wave conv forms out of the tuner)
        with torch.cuda.stream(self.stream):
            self._counters = [torch.zeros(L.SPLITK_MAX_TILES, dtype=torch.int32, device=self.device) for _ in range(2)]
        with torch.cuda.stream(self.stream):
            self._chan_counters = [torch.zeros(4096, dtype=torch.int32, device=self.device) for _ in range(2)]
        self.stream.synchronize()

    # ------------------------------------------------------------------ helpers
    def pool_streams(self):
        """the process's four launch streams on this device, as torch streams (include/vsd.h vsd_stream_pool)"""
        h = (C.c_void_p * L.POOL_STREAMS)()
        self.ctx.call("vsd_stream_pool", h)
        return [torch.cuda.ExternalStream(int(h[i]), device=self.device) for i in range(L.POOL_STREAMS)]

    def pool_check(self, chain: int = 100) -> float:
        """time of four frame-like kernel chains on the four launch streams at once / one chain alone: ~1.0 when they run side
        by side, >= 2 when two of them share a command-processor pipe (vsd_stream_pool_check)"""
        r = C.c_float()
        self.ctx.call("vsd_stream_pool_check", int(chain), C.byref(r))
        return float(r.value)

    def _stream(self, idx: int):
        return self.streams[idx]

    @property
    def s(self):
        return C.c_void_p(self._stream(self._sidx).cuda_stream)

    def raw_stream(self, idx: int = 0):
        return C.c_void_p(self._stream(idx).cuda_stream)

    # ---- two-stream fork/join.  Run live (eager mode) these are events between the two streams; in a captured program the
    #      engine turns them into the edges of a launch sequence (Engine._capture), never into branches of one graph.
    def use_stream(self, idx: int):
        self._sidx = idx

    def fork(self):
        e = torch.cuda.Event()
        e.record(self._stream(0))
        self._stream(1).wait_event(e)

    def join(self):
        e = torch.cuda.Event()
        e.record(self._stream(1))
        self._stream(0).wait_event(e)

    # ---- named dependencies between the two streams (edges of the captured graph): `signal` marks a point of the
    #      current stream, `wait` makes the current stream wait for it
    def signal(self, name: str):
        e = torch.cuda.Event()
        e.record(self._stream(self._sidx))
        self._events[name] = e

    def wait(self, name: str):
        self._stream(self._sidx).wait_event(self._events[name])

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def clone(self, lane: Optional[int] = None, _register: bool = True) -> "HipOps":
        """Same GPU, own context / scratch, shared tuning table, the streams of launch lane `lane` (default: the next unused
        one): a further frame in flight.  Objects of ONE lane share its streams -- they are meant to take turns (the engines of a
        lane's several plans / batch sizes); objects of different lanes run side by side."""
        if lane is None:
            lane = self._lanes.next_free()
        return HipOps(self.device_id, make_current=False, tile_override=self.tile_override, lane=int(lane), _lanes=self._lanes,
                      _register=_register)

    # Debugging hook (scripts/guard_page_engine.py): a callable(nbytes) -> uint8 device tensor.  When set, EVERY buffer this object
    # hands out -- activations (the engine's arena then allocates tensor by tensor), packed weights, uploads, workspaces -- comes
    # from it, e.g. from an allocator that ends each buffer at an unmapped page so that an out-of-bounds access faults.
    allocator = None

    def _alloc(self, shape, dtype):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        raw = self.allocator(max(nbytes, 16))
        return raw[:nbytes].view(dtype).view(*shape)

    def empty(self, *shape, dtype=torch.float16):
        if self.allocator is not None:
            with torch.cuda.stream(self.stream):
                t = self._alloc(shape, dtype)
                t.view(torch.uint8).fill_(255 if POISON else 0)
                return t
        with torch.cuda.stream(self.stream):
            t = torch.empty(*shape, dtype=dtype, device=self.device)
            if POISON:  # VSD_POISON=1 (tests): every "uninitialised" byte is 0xFF (fp16 / fp32 NaN), so that a kernel
                t.view(torch.uint8).fill_(255)  # relying on what the allocator happened to hand out fails every time
            return t

    def zeros(self, *shape, dtype=torch.float16):
        with torch.cuda.stream(self.stream):
            if self.allocator is not None:
                t = self._alloc(shape, dtype)
                t.view(torch.uint8).zero_()
                return t
            return torch.zeros(*shape, dtype=dtype, device=self.device)

    def to_device(self, t: torch.Tensor):
        with torch.cuda.stream(self.stream):
            if self.allocator is not None:
                d = self._alloc(tuple(t.shape), t.dtype)
                d.copy_(t.contiguous())
                return d
            return t.to(self.device)

    def zero_(self, t: torch.Tensor):
        with torch.cuda.stream(self.stream):
            t.zero_()

    def copy_(self, dst: torch.Tensor, src: torch.Tensor):
        """device-to-device copy ordered on this ops' kernel stream"""
        with torch.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)

    def to_device_pack(self, p: PackedConv) -> PackedConv:
        for f in ("weight", "bias", "ln_s", "ln_t", "weight_frag"):
            v = getattr(p, f)
            if v is not None:
                setattr(p, f, self.to_device(v) if self.allocator is not None else v.to(self.device).contiguous())
        return p

    @property
    def _scratch(self) -> int:
        return self._sidx if self._widx is None else self._widx

    def _counter_set(self, sets, n):
        """split-K / channel-statistics counters of the current scratch set (zeroed once; the kernels leave them at zero)"""
        while len(sets) <= self._scratch:
            with torch.cuda.stream(self.stream):
                sets.append(torch.zeros(n, dtype=torch.int32, device=self.device))
            self.stream.synchronize()
        return sets[self._scratch]

    def workspace(self, key: str, nbytes: int) -> torch.Tensor:
        key = (key, self._scratch)  # kernels on different streams / members of one grid may run concurrently: separate scratch
        cur = self._ws.get(key)
        if cur is None or cur.numel() < nbytes:
            with torch.cuda.stream(self.stream):
                if self.allocator is not None:
                    cur = self.allocator(max(nbytes, 256))
                else:
                    cur = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
                if POISON:
                    cur.fill_(255)
            self._ws[key] = cur
        if self.allocator is not None and cur.numel() != max(nbytes, 256):  # (hook mode: exactly the size asked for, every time)
            with torch.cuda.stream(self.stream):
                cur = self._ws[key] = self.allocator(max(nbytes, 256))
        return cur

    def synchronize(self):
        for st in reversed(self.streams):
            st.synchronize()

    def upload(self, dst: torch.Tensor, src_cpu: torch.Tensor):
        """H2D on the kernel stream.  Asynchronous only from PINNED memory (the caller keeps that buffer alive, e.g. the
        engine's frame staging); from pageable memory the call returns when the bytes have left the source, so a
        temporary may be passed (an async copy from a temporary that is freed right after read freed memory: seen as
        a garbage reference image on the MI355X)."""
        with torch.cuda.stream(self.stream):
            dst.copy_(src_cpu.view(dst.shape), non_blocking=src_cpu.is_pinned())

    def download(self, src: torch.Tensor) -> torch.Tensor:
        with torch.cuda.stream(self.stream):
            out = src.to("cpu", non_blocking=False)
        return out

    def download_into(self, dst_cpu: torch.Tensor, src: torch.Tensor):
        """D2H into a (pinned) host tensor on the kernel stream, then wait for that stream."""
        with torch.cuda.stream(self.stream):
            dst_cpu.view(src.shape).copy_(src, non_blocking=True)
        self.stream.synchronize()

    # ------------------------------------------------------------------ ops
    def conv(self, src0, src1, g: Geom, w: PackedConv, out, *, ldo=None, c0=None, c1=0, rowvec=None, residual=None,
             residual2=None, ldr=None, out_scale=1.0, act=L.ACT_NONE, out2=None, add2=None, out_t=None, ldt=0,
             t_col0=0, tile=None, split_k=None, workspace=None, pipeline=None, rowstat_out=None, ln_part=None,
             ln_eps=1e-5, chanstat_out=None, t_img=0, out_scale_dev=None, softmax_cols=0, inkernel=None, _desc_only=False):
        """t_img: with g.batch > 1, columns of out_t per image (image b's pixels start at column b * t_img).
        out_scale_dev: one fp32 in device memory that replaces out_scale at run time (changeable under a captured graph).
        tile / split_k / pipeline / inkernel (None: `self.inkernel_splitk`): the form where the caller names it, else convform.resolve's."""
        m = g.m
        c0 = c0 if c0 is not None else (w.cin - c1)
        call = CF.conv_call(g, w, c1=c1, act=act, out_scale=out_scale, ldo=ldo, t_col0=t_col0, residual=residual, residual2=residual2,
                            out2=out2, out_t=out_t, rowstat_out=rowstat_out, chanstat_out=chanstat_out, ln_part=ln_part,
                            out_scale_dev=out_scale_dev)
        act = call.act  # (GEGLU weights: the GEGLU epilogue)
        tile, split_k, inkernel, pipeline = CF.resolve(call, self.tile_override, self.tune_mode, CF.flags_of(self), tile, split_k, pipeline,
                                                       self.inkernel_splitk if inkernel is None else inkernel)
        d = L.ConvDesc()
        d.src0, d.src1 = self._p(src0), self._p(src1)
        d.c0, d.c1 = c0, c1
        d.hs, d.ws, d.hi, d.wi, d.ho, d.wo = g.hs, g.ws, g.hi, g.wi, g.ho, g.wo
        d.ksize, d.stride, d.pad = g.ksize, g.stride, g.pad
        d.weight = self._p(w.weight)
        d.n, d.k, d.kp = w.n, w.k, w.kp
        d.bias = self._p(w.bias)
        if ln_part is not None:
            if w.ln_s is None:
                raise RuntimeError("conv: ln_part given but the weights were not packed with pack_linear_ln")
            d.ln_part, d.ln_groups, d.ln_eps = self._p(ln_part), ln_part.shape[1], ln_eps
            d.ln_s, d.ln_t = self._p(w.ln_s), self._p(w.ln_t)
        d.rowstat_out = self._p(rowstat_out)
        if chanstat_out is not None:
            d.chanstat_out = self._p(chanstat_out)
            d.chanstat_part = self._p(self.workspace("chanpart", (-(-m // 64)) * w.n * 8))
            d.chan_counters = self._p(self._counter_set(self._chan_counters, 4096))
        d.rowvec = self._p(rowvec)
        d.residual, d.residual2 = self._p(residual), self._p(residual2)
        d.ldr = ldr if ldr is not None else w.n_out
        d.out_scale = out_scale
        d.out_scale_dev = self._p(out_scale_dev)
        d.softmax_cols = softmax_cols
        d.act = act
        d.out = self._p(out)
        d.ldo = call.ldo
        d.out2, d.add2 = self._p(out2), self._p(add2)
        d.out_t, d.ldt, d.t_col0 = self._p(out_t), ldt, t_col0
        d.batch, d.t_img = g.batch, t_img
        d.tile, d.split_k, d.pipeline = tile, split_k, pipeline
        if split_k > 1:
            ws = workspace if workspace is not None else self.workspace("splitk", split_k * m * w.n * 4)
            d.workspace = self._p(ws)
            if inkernel:
                d.counters = self._p(self._counter_set(self._counters, L.SPLITK_MAX_TILES))
        elif workspace is not None:  # (development probes pass a buffer through)
            d.workspace = self._p(workspace)
        if _desc_only:
            return d
        self.ctx.call("vsd_conv_gemm", C.byref(d), self.s)

    # ---- several independent convs as ONE launch (include/vsd.h vsd_conv_gemm_group)
    GROUP_FORMS, GROUP_ALONE, OWN_SPLIT = CF.GROUP_FORMS, CF.GROUP_ALONE, CF.OWN_SPLIT  # (see there)

    def _policy(self):  # (what convform's functions take after the calls: the table, the tuning mode, the development switches)
        return self.tile_override, self.tune_mode, CF.flags_of(self)

    def own_splits(self, calls):
        return CF.own_splits(calls, *self._policy())

    def group_key(self, calls, split=None):
        return CF.group_key(calls, split, self.tune_mode)

    def group_candidates(self, calls, split=None):
        return CF.group_candidates(calls, *self._policy(), split=split)

    def conv_group(self, calls, form=None, split=None, default=None):
        """calls: [(args, kwargs), ...] as for `conv` (1 x 1 / 3 x 3 layers on the buffer-load path): ONE launch for all of them
        (plus one reducer launch for the members that leave split-K slabs), every member in the same kernel form
        (tile, split_k, reduce in the launch, pipeline) -- `form`, else this group's entry of the tuning table (`tune_group`), else
        64 x 64 tiles on the 3-stage ring, unsplit (`split`: split that many times -- the table entry is then looked up for that
        split).  Member i works in a scratch set of its own (split-K slabs, counters).  Same bits as the members launched one by one at the
        same split_k, whatever their tile and pipeline (a conv's bits depend on the split alone: scripts/conv_bits_probe.py).  A
        table entry may also say that the members are better off alone.  split = OWN_SPLIT: members of DIFFERENT shapes that also
        exist as launches of their own in another form of the program (a ResnetBlock's conv1 and its shortcut conv) -- every member
        at the split its own table entry has (own_splits), the group's entry (split field 0) names tile / reduction form / pipeline."""
        if not 1 <= len(calls) <= L.CONV_GROUP_MAX:
            raise ValueError(f"conv_group: {len(calls)} members (1..{L.CONV_GROUP_MAX})")
        own = None
        if split == self.OWN_SPLIT:
            own = self.own_splits(calls)
            if own is None:
                form = CF.ALONE
        if form is None:
            ent = CF.lookup(self.tile_override, self.group_key(calls, split))
            form = ent if ent is not None else (default or (L.TILE_64x64, (0 if own else split) or 1, True, 3))
        tile, split_k, inkernel, pipeline = form
        if tile == self.GROUP_ALONE:
            for a, kw in calls:
                self.conv(*a, **kw)
            return
        descs = (L.ConvDesc * len(calls))()
        try:
            for i, (a, kw) in enumerate(calls):
                # scratch set of member i on stream s: 2 i + s -- member 0 works in its stream's own set, the others in sets no launch of
                # EITHER stream uses (a group on the side stream beside split-K layers on the main one: the shortcut groups of the
                # two encoders.  With `i` alone the ControlNet's conv1 shared slabs and tickets with the UNet encoder's layers: wrong
                # frames from the captured two-stream form, found by the mini-pipeline parity tests)
                self._widx = 2 * i + self._sidx
                descs[i] = self.conv(*a, tile=tile, split_k=own[i] if own else split_k, pipeline=pipeline, inkernel=bool(inkernel),
                                     _desc_only=True, **CF.unnamed(kw))
        finally:
            self._widx = None
        self.ctx.call("vsd_conv_gemm_group", descs, len(calls), self.s)

    def _stopwatch(self, launch, reps: int, trials: int) -> float:
        """us per call of `launch`, issued back to back on this stream: two calls to warm up, then the best of `trials` runs of `reps`"""
        for _ in range(2):
            launch()
        best = 1e30
        for _trial in range(trials):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(reps):
                launch()
            e1.record(self.stream)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps * 1e3)
        return best

    def _time_forms(self, launcher, forms, reps: int, trials: int, what: str):
        """[(us per call of launcher(form)(), *form)] of every form the library takes, fastest first; none ran: an error that says why"""
        table, refused = [], None
        for form in forms:
            try:
                table.append((self._stopwatch(launcher(form), reps, trials),) + tuple(form))
            except RuntimeError as e:
                refused = e
        if not table:  # (every form was refused: say for what and why instead of an IndexError)
            raise RuntimeError(f"{what}: no kernel form ran: {refused}")
        return sorted(table)

    def tune_group(self, calls, reps: int = 12, split=None):
        """time the forms a group may take (`group_candidates`) back to back on this stream; remember the fastest"""
        table = self._time_forms(lambda form: partial(self.conv_group, calls, form=form, split=split if split == self.OWN_SPLIT else None),
                                 self.group_candidates(calls, split), reps, 2, "tune_group")
        b = table[0]
        self.tile_override[self.group_key(calls, split)] = (b[1], b[2], bool(b[3]), b[4])
        return b, table

    # ---- two independent calls of one op as ONE grid per kernel (include/vsd.h vsd_pair_begin): the twin layers of the UNet and
    #      the ControlNet encoder.  a, b: recorded calls (bound method, args, kwargs).  b works in scratch set 1.
    def pair(self, a, b):
        (fa, aa, ka), (fb, ab, kb) = a, b
        if fa.__name__ == "conv" and fb.__name__ == "conv":
            shared = CF.pair_form(aa, ka, ab, kb, *self._policy(), inkernel=self.inkernel_splitk)
            if shared is not None:
                sp, own = shared
                # Latency mode (one-frame programs): the pair's table entry (`tune_group`, timed alone), else the form its first member
                # has alone.  Throughput mode (coalesced launches on busy lanes): ALWAYS the members' own form -- a group's entry is
                # chosen by launch latency, and in such a form a pair of the 5-frame program's layers occupied 14 % more workgroup-time
                # than the two launches (profiles/round5f_pairs_at_5x4.txt); in their own form the pair costs what they cost and
                # saves the launch.
                return self.conv_group([(aa, ka), (ab, kb)], form=own if self.tune_mode == 1 else None, split=sp, default=own)
            fa(*aa, **ka)
            self._widx = 1
            try:
                fb(*ab, **kb)
            finally:
                self._widx = None
            return
        self.ctx.call("vsd_pair_begin")
        done = False
        try:
            fa(*aa, **ka)
            self.ctx.call("vsd_pair_join")
            self._widx = 1
            fb(*ab, **kb)
            done = True
        finally:
            self._widx = None
            rc = self.ctx.lib.vsd_pair_end(self.ctx.h, None)  # (always closes the pair; held launches go out alone)
            if done:
                self.ctx.check(rc, "vsd_pair_end")

    def pair_split(self, aa, ka, ab, kb):
        """the split over K at which two twin convs share a grid, or None: launch them one by one (convform.pair_form)"""
        shared = CF.pair_form(aa, ka, ab, kb, *self._policy(), inkernel=self.inkernel_splitk)
        return shared and shared[0]

    def conv_key_of(self, g: Geom, w: PackedConv, kwargs: dict):
        """the tuning key of a recorded conv call (args[2], args[3], its keyword arguments)"""
        return CF.conv_call(g, w, **kwargs).key(self.tune_mode)

    def tune_conv(self, args, kwargs, reps: int = 12):
        """Time every (tile, split_k, reduction form) candidate for one recorded conv call on the GPU and
        remember the fastest in tile_override.  Returns (best, table)."""
        g, w = args[2], args[3]
        call = CF.conv_call(g, w, **kwargs)
        key = call.key(self.tune_mode)
        cands = CF.candidates(call, self.tune_mode, CF.flags_of(self))
        kw = CF.unnamed(kwargs)
        self.tile_override.pop(key, None)

        # every candidate alone, back to back (in throughput mode once: a pre-pass; else twice, the better run counts)
        table = self._time_forms(lambda form: partial(self.conv, *args, **form._asdict(), **kw), cands, reps, 1 if self.tune_mode == 1 else 2,
                                 f"tune_conv M={g.m} N={w.n} K={w.k} ksize={g.ksize}")
        if self.tune_mode == 1:
            # Throughput mode.  Timed alone, a candidate is judged by its launch latency on an idle chip -- small tiles and many
            # workgroups win.  With four lanes busy the chip is shared, other launches fill whatever a launch leaves idle, and
            # what a candidate costs is its CU-time: larger tiles (less operand re-streaming per FLOP) win back.  Measured on
            # MI355X (scripts/tune_lanes_probe.py, us per launch alone | with four copies in flight): 5x32x32 640->640 3x3:
            # 64x128 GEMM form 54.8 | 48.9, 256x128 halo form 81.6 | 38.7; 1280x1280x5120: 64x64 35.2 | 30.4, 128x64 42.3 | 23.8.
            # So: every candidate alone first (cheap), then the ones within 2.5x of the best with four copies at once.
            cut = 2.5 * table[0][0]
            # (the 256 x 256 tile always makes the shortlist: a handful of workgroups is slow ALONE by construction -- 2-5 x on an idle
            #  chip -- and what it is for is the shared one)
            short = [CF.Form(*row[1:]) for row in table if row[0] <= cut or (row[1] == L.TILE_256x256 and row[0] <= 6.0 * table[0][0])]
            table = self._time_candidates_on_lanes(args, kw, short, reps) or table
        best = table[0]
        if self.tune_mode != 1 and best[2] > 1 and not best[3] and self.one_launch_bias_us > 0:
            # a two-launch form won: take a one-launch form that is within the bias instead (one graph node less; back-to-back
            # timing on an otherwise idle GPU flatters the second launch, which in a frame also delays the NEXT layer's start)
            for cand in table[1:]:
                if cand[0] > best[0] + self.one_launch_bias_us:
                    break
                if cand[2] == 1 or cand[3]:
                    best = cand
                    break
        self.tile_override[key] = (best[1], best[2], best[3], best[4])
        return best, table

    def _time_candidates_on_lanes(self, args, kw, cands, reps, n_lanes: int = 4):
        """us per launch with `n_lanes` copies of the candidate in flight, one per launch lane (captured graphs of `reps`
        launches each, so that the host is out of the picture); every lane has its own input / output / scratch"""
        # this object on ITS lane, helpers on the other lanes (one set per process, kept on the shared lane book; an engine on
        # lane 1-3 that tunes online must not put two copies on its own stream: ADVICE r4)
        others = [l for l in range(L.POOL_STREAMS) if l != self.lane % L.POOL_STREAMS][:max(0, n_lanes - 1)]
        for l in others:
            if l not in self._lanes.tune_helpers:
                self._lanes.tune_helpers[l] = self.clone(lane=l, _register=False)
        lanes = [self] + [self._lanes.tune_helpers[l] for l in others]
        for o in lanes:
            o.tune_mode = self.tune_mode
        src0, src1, g, w, out = args[:5]
        # every lane writes its OWN buffers: the output and every other tensor the launch writes (transposed output, second
        # output, statistics) -- four launches at once into one buffer would time a write conflict, not the candidate
        writes = ("out2", "out_t", "rowstat_out", "chanstat_out")
        per_lane = [(src0, src1, out, kw)]
        for _ in lanes[1:]:
            kwl = dict(kw)
            for name in writes:
                if kwl.get(name) is not None:
                    kwl[name] = kwl[name].clone()
            per_lane.append((src0.clone(), None if src1 is None else src1.clone(), out.clone(), kwl))
        table = []
        for form in cands:
            graphs = []
            try:
                for o, (a0, a1, oo, kwl) in zip(lanes, per_lane):
                    o.conv(a0, a1, g, w, oo, *args[5:], **form._asdict(), **kwl)
                    o.synchronize()
                    o.graph_begin()
                    try:
                        for _ in range(reps):
                            o.conv(a0, a1, g, w, oo, *args[5:], **form._asdict(), **kwl)
                    finally:
                        graphs.append((o, o.graph_end()))
                best = 1e30
                for _trial in range(3):
                    for o, gr in graphs:
                        o.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(2):
                        for o, gr in graphs:
                            o.graph_launch(gr)
                    for o, gr in graphs:
                        o.synchronize()
                    best = min(best, (time.perf_counter() - t0) / (2 * reps * len(graphs)) * 1e6)
                table.append((best,) + form)
            except RuntimeError:
                pass
            finally:
                for o, gr in graphs:
                    o.graph_destroy(gr)
        table.sort()
        return table

    # ---- tuning table persistence (the "find" results are per device generation and shape)
    @staticmethod
    def _read_table(path: str):
        """[(key, entry)] of the table file at `path`; none when there is no such file"""
        if not _os.path.exists(path):
            return []
        return [(tuple(k), tuple(v)) for k, v in json.load(open(path)).get("table", [])]

    def save_tuning(self, path: str):
        """Write this process's choices INTO the table at `path` (entries of other shapes -- other batch sizes, other
        frame sizes -- are kept)."""
        try:
            merged = dict(self._read_table(path))
        except Exception:
            merged = {}
        merged.update(self.tile_override)
        with open(path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(self.device),
                       "table": [[list(k), list(v)] for k, v in sorted(merged.items(), key=str)]}, f, indent=0)

    def load_tuning(self, path: str) -> int:
        n = 0
        for key, v in self._read_table(path):
            if isinstance(key[-1], bool):
                continue  # a round-3 table (last field: "has a statistics output"): its entries name no epilogue class
            if len(key) == 9 and key[0] != "group":
                key = key + (0,)  # (a table written before the tuning mode joined the key: timed alone)
            if key not in self.tile_override:
                self.tile_override[key] = (int(v[0]), int(v[1]), bool(v[2]), int(v[3]))
                n += 1
        return n

    # ---- fused per-token chains of a transformer block at the 320-wide level (csrc/fused_tail.hip)
    TAIL_C = 320

    def tail_a(self, att, h, m, out1: PackedConv, q2: PackedConv, h1_out, q_out, ln_eps=1e-5):
        """h1 = att Wo^T + b + h ; q = LN(h1) Wq'^T"""
        self.ctx.call("vsd_tail_a", self._p(att), self._p(h), m, self._p(out1.weight_frag), self._p(out1.bias), self._p(q2.weight_frag),
                      self._p(q2.ln_s), self._p(q2.ln_t), ln_eps, self._p(h1_out), self._p(q_out), self.s)

    def tail_b(self, att2, h1, x, m, out2: PackedConv, ff1: PackedConv, ff2: PackedConv, proj: PackedConv, out, ln_eps=1e-5):
        """h2 = att2 Wo^T + b + h1 ; h3 = GEGLU-FF(LN(h2)) + h2 ; out = h3 Wp^T + b + x"""
        self.ctx.call("vsd_tail_b", self._p(att2), self._p(h1), self._p(x), m, self._p(out2.weight_frag), self._p(out2.bias),
                      self._p(ff1.weight_frag), self._p(ff1.ln_s), self._p(ff1.ln_t), ln_eps, self._p(ff2.weight_frag),
                      self._p(ff2.bias), self._p(proj.weight_frag), self._p(proj.bias), self._p(out), self.s)

    def groupnorm_launches(self, c0, c1, hw, groups, batch=1) -> int:
        """kernel launches one `groupnorm` call issues (the library's own decision: csrc/norm.hip)"""
        return int(self.ctx.lib.vsd_groupnorm_launches(c0, c1, hw, max(1, batch), groups))

    def groupnorm(self, src0, src1, c0, c1, hw, groups, eps, gamma, beta, silu, out, batch=1):
        ws = self.workspace("gn", max(1, batch) * int(self.ctx.lib.vsd_groupnorm_workspace_bytes(hw, c0 + c1, groups)))
        if batch > 1:
            self.ctx.call("vsd_groupnorm_batched", self._p(src0), self._p(src1), c0, c1, hw, batch, groups, eps,
                          self._p(gamma), self._p(beta), int(silu), self._p(out), self._p(ws), self.s)
            return
        self.ctx.call("vsd_groupnorm", self._p(src0), self._p(src1), c0, c1, hw, groups, eps, self._p(gamma),
                      self._p(beta), int(silu), self._p(out), self._p(ws), self.s)

    def layernorm(self, x, rows, c, gamma, beta, eps, out):
        self.ctx.call("vsd_layernorm", self._p(x), rows, c, self._p(gamma), self._p(beta), eps, self._p(out), self.s)

    def attention(self, q, ldq, k, ldk, vt, ldvt, out, ldo, sq, sk, heads, d, scale, causal=False, batch=1, k_brows=0,
                  vt_bcols=0):
        """batch > 1: image b uses q/out rows [b*sq, (b+1)*sq), K rows from b*k_brows, V^T columns from b*vt_bcols."""
        if batch > 1:
            self.ctx.call("vsd_attention_batched", self._p(q), ldq, self._p(k), ldk, self._p(vt), ldvt, self._p(out), ldo,
                          sq, sk, heads, d, scale, int(causal), batch, k_brows, vt_bcols, self.s)
            return
        self.ctx.call("vsd_attention", self._p(q), ldq, self._p(k), ldk, self._p(vt), ldvt, self._p(out), ldo, sq, sk,
                      heads, d, scale, int(causal), self.s)

    RESAMPLE_TABLES = 16  # (in, out) weight tables kept per object: a camera that changes resolution costs a table, not more

    def center_crop_box(self, src_w: int, src_h: int, dst_w: int, dst_h: int):
        """the reference's crop box (videopipeline.py:92-107) with PIL's rounding: (left, top, right, bottom)"""
        b = (C.c_int * 4)()
        if self.ctx.lib.vsd_center_crop_box(int(src_w), int(src_h), int(dst_w), int(dst_h), b) != 0:  # (host only: no context)
            raise ValueError(f"center_crop_box: {src_w} x {src_h} -> {dst_w} x {dst_h}: every side must be at least 1")
        return tuple(b)

    def resample_table(self, n_in: int, n_out: int) -> torch.Tensor:
        """Pillow's LANCZOS weight table for one axis (built on the host by the library), in device memory; least recently used out"""
        tabs = self.__dict__.setdefault("_resample_tables", {})
        t = tabs.pop((n_in, n_out), None)
        if t is None:
            nbytes = int(self.ctx.lib.vsd_resample_table_bytes(int(n_in), int(n_out)))
            if nbytes <= 0:
                raise RuntimeError(f"resample: {n_in} -> {n_out}: lengths must be 1..{L.RESAMPLE_MAX_SIDE}")
            with torch.cuda.stream(self.stream):
                t = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
            self.ctx.call("vsd_resample_table_upload", int(n_in), int(n_out), self._p(t), self.raw_stream(0))
            while len(tabs) >= self.RESAMPLE_TABLES:
                tabs.pop(next(iter(tabs)))
        tabs[(n_in, n_out)] = t
        return t

    def resample_rgb(self, src_u8, src_h, src_w, src_row_bytes, box, dst_u8, dst_h, dst_w):
        """`img.crop(box).resize((dst_w, dst_h), LANCZOS)` of packed u8 RGB rows in device memory into dst_u8 [dst_h][dst_w][3],
        bit for bit Pillow's (csrc/resample.hip)"""
        bw, bh = int(box[2]) - int(box[0]), int(box[3]) - int(box[1])
        tx = self.resample_table(bw, dst_w) if bw != dst_w and bw > 0 else None
        ty = self.resample_table(bh, dst_h) if bh != dst_h and bh > 0 else None
        ws = self.workspace("resample", int(self.ctx.lib.vsd_resample_workspace_bytes(bh, dst_w))) if tx is not None and ty is not None else None
        self.ctx.call("vsd_resample_rgb", self._p(src_u8), int(src_h), int(src_w), int(src_row_bytes), (C.c_int * 4)(*[int(v) for v in box]),
                      self._p(dst_u8), int(dst_h), int(dst_w), self._p(tx), self._p(ty), self._p(ws), self.s)

    def i420_to_rgb(self, y, y_stride, u, v, uv_stride, ox, oy, h, w, dst_rgb, dst_row_bytes=None):
        """An h x w rectangle of an I420 frame in device memory (first luma sample at frame position (ox, oy); u / v point at chroma
        sample (ox >> 1, oy >> 1)) to packed RGB rows, by the colour contract of include/vsd.h (csrc/yuv.hip)"""
        self.ctx.call("vsd_i420_to_rgb", self._p(y), int(y_stride), self._p(u), self._p(v), int(uv_stride), int(ox), int(oy), int(h), int(w),
                      self._p(dst_rgb), int(3 * w if dst_row_bytes is None else dst_row_bytes), self.s)

    def rgb_to_i420(self, rgb_u8, h, w, dst_y, dst_u, dst_v, y_stride=None, uv_stride=None):
        """packed [h][w][3] in device memory (h, w even) to three planes, by the same contract"""
        self.ctx.call("vsd_rgb_to_i420", self._p(rgb_u8), int(h), int(w), self._p(dst_y), self._p(dst_u), self._p(dst_v),
                      int(w if y_stride is None else y_stride), int(w // 2 if uv_stride is None else uv_stride), self.s)

    def preprocess_rgb(self, rgb_u8, h, w, out):
        self.ctx.call("vsd_preprocess_rgb", self._p(rgb_u8), h, w, self._p(out), self.s)

    def sobel_control(self, rgb_u8, h, w, low, high, edge_u8, control_out):
        ws = self.workspace("sobel", int(self.ctx.lib.vsd_sobel_workspace_bytes(h, w)))
        self.ctx.call("vsd_sobel_control", self._p(rgb_u8), h, w, low, high, self._p(edge_u8), self._p(control_out),
                      self._p(ws), self.s)

    def canny_control(self, rgb_u8, h, w, low, high, edge_u8, control_out):
        """Canny edges by THE EDGE CONTRACT of include/vsd.h (csrc/canny.hip): the same inputs and outputs as `sobel_control`, integer
        thresholds on |dx| + |dy| (0..2040).  The workspace carries the labels between the call's four launches: it is this object's,
        keyed like "sobel" by the scratch set of the stream in use -- objects are per launch lane (`clone`), so two lanes never share it,
        and the calls of one object on one stream run one after the other."""
        ws = self.workspace("canny", int(self.ctx.lib.vsd_canny_workspace_bytes(h, w)))
        self.ctx.call("vsd_canny_control", self._p(rgb_u8), int(h), int(w), int(low), int(high), self._p(edge_u8), self._p(control_out),
                      self._p(ws), self.s)

    def color_match(self, src_u8, dst_u8, frames, h, w, mode, amounts_dev):
        """The colours of `src_u8` onto `dst_u8` in place, `frames` packed [h][w][3] frames each, by THE COLOUR CONTRACT of include/vsd.h
        (csrc/color_match.hip).  mode: a key of lib.COLOR_MODES; amounts_dev: int32 [frames] in device memory, the contract's integer
        amounts 0..256, read when the kernels run (a captured graph follows a later copy into it).  Three launches; the workspace carries
        the partial histograms and the LUTs between them: it is this object's, keyed like "canny" by the scratch set of the stream in use."""
        ws = self.workspace("color_match", int(self.ctx.lib.vsd_color_match_workspace_bytes(int(frames), int(h), int(w))))
        self.ctx.call("vsd_color_match", self._p(src_u8), self._p(dst_u8), int(frames), int(h), int(w), int(L.COLOR_MODES[mode]),
                      self._p(amounts_dev), self._p(ws), self.s)

    def gauss_blur(self, src, dst, frames, h, w, channels, taps_dev):
        """`src` blurred into `dst` by THE BLUR CONTRACT of include/vsd.h (csrc/blur.hip): `frames` packed u8 [h][w][channels] frames each,
        channels 1 or 3, any alignment, no overlap.  taps_dev: int32 [34] = {R, w_0 .. w_32} in device memory (`videosd_amd.blur`), read
        when the kernel runs (a captured graph follows a later copy into it).  One launch, no workspace."""
        self.ctx.call("vsd_gauss_blur", self._p(src), self._p(dst), int(frames), int(h), int(w), int(channels), self._p(taps_dev), self.s)

    def mask_blend(self, src_u8, dst_u8, mask_u8, frames, h, w):
        """`src_u8` blended into `dst_u8` in place by THE KEEP MASK of include/vsd.h (csrc/keep_mask.hip): `frames` packed [h][w][3] frames
        each, one u8 [h][w] mask per frame (255: dst stays, 0: the src pixel).  One launch, no workspace."""
        self.ctx.call("vsd_mask_blend", self._p(src_u8), self._p(dst_u8), self._p(mask_u8), int(frames), int(h), int(w), self.s)

    def mask_latent(self, mask_u8, frames, h, w, weights_f32):
        """the masks' latent weights: fp32 [frames][h/8 * w/8], the mean of the integer weight over every 8 x 8 block (one launch)"""
        self.ctx.call("vsd_mask_latent", self._p(mask_u8), int(frames), int(h), int(w), self._p(weights_f32), self.s)

    def latent_keep(self, x0, weights_f32, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, lat=None, den=None, dec_in=None):
        """The latent anchor of a keep mask, in place.  Step form (`lat`; exactly one of noise_f32 / seeds_dev): where the weight is below 1,
        `lat` moves towards x0 noised to the next timestep with draw 0 (coefficients 4, 5 of the six at coef_dev; image b's at
        + b * coef_stride floats, 0: shared).  Final form (`den`, `dec_in`; no noise source): `den` moves towards x0, `dec_in` follows."""
        self.ctx.call("vsd_latent_keep", self._p(x0), self._p(weights_f32), self._p(noise_f32), self._p(seeds_dev), int(kind), int(draw),
                      self._p(coef_dev), int(coef_stride), int(hw), int(batch), self._p(lat), self._p(den), self._p(dec_in), self.s)

    def add_noise(self, x0, noise_f32, sqrt_a, sqrt_b, hw, out):
        self.ctx.call("vsd_add_noise", self._p(x0), self._p(noise_f32), sqrt_a, sqrt_b, hw, self._p(out), self.s)

    def lcm_step(self, eps, sample, noise_f32, coef, hw, prev, denoised, dec_in=None):
        arr = (C.c_float * 6)(*[float(x) for x in coef])
        self.ctx.call("vsd_lcm_step", self._p(eps), self._p(sample), self._p(noise_f32), arr, hw, self._p(prev),
                      self._p(denoised), self._p(dec_in), self.s)

    def add_noise_dev(self, x0, noise_f32, coef_dev, hw, batch, out):
        """coef_dev: fp32 [2] in device memory (sqrt_a, sqrt_b); `batch` images per launch, one noise draw for all."""
        self.ctx.call("vsd_add_noise_dev", self._p(x0), self._p(noise_f32), self._p(coef_dev), hw, batch, self._p(out), self.s)

    def lcm_step_dev(self, eps, sample, noise_f32, coef_dev, hw, batch, prev, denoised, dec_in=None):
        """coef_dev: fp32 [6] in device memory, as `lcm_step`'s coef."""
        self.ctx.call("vsd_lcm_step_dev", self._p(eps), self._p(sample), self._p(noise_f32), self._p(coef_dev), hw, batch,
                      self._p(prev), self._p(denoised), self._p(dec_in), self.s)

    # ---- seeded noise (include/vsd.h THE NOISE CONTRACT; csrc/noise.hip)
    def noise_fill(self, seed: int, kind: int, draw: int, hw: int, out, raw: bool = False):
        """one draw of `hw` latent pixels for `seed` (any int, taken modulo 2^64): fp32 [4][hw], or raw=True the Philox integers u32 [hw][4]"""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.ctx.call("vsd_noise_fill", seed & 0xFFFFFFFF, seed >> 32, int(kind), int(draw), hw, int(bool(raw)), self._p(out), self.s)

    def add_noise_seeded(self, x0, seeds_dev, kind, draw, coef_dev, hw, batch, out):
        """`add_noise_dev` with the draw computed in the kernel; seeds_dev: u32 [batch][2] (low, high) in device memory"""
        self.ctx.call("vsd_add_noise_seeded", self._p(x0), self._p(seeds_dev), int(kind), int(draw), self._p(coef_dev), hw, batch,
                      self._p(out), self.s)

    def lcm_step_seeded(self, eps, sample, seeds_dev, kind, draw, coef_dev, hw, batch, prev, denoised, dec_in=None):
        """`lcm_step_dev` with the draw computed in the kernel; draw <= 0: the step adds no noise"""
        self.ctx.call("vsd_lcm_step_seeded", self._p(eps), self._p(sample), self._p(seeds_dev), int(kind), int(draw), self._p(coef_dev),
                      hw, batch, self._p(prev), self._p(denoised), self._p(dec_in), self.s)

    def prompt_install(self, src_buf, dst_buf, segs_dev, nseg: int, frame: int):
        """one cached prompt (PromptBlock.buf of a PromptLayout) into frame slot `frame` of a per-frame block (FramePromptLayout), one launch on
        this object's own stream (include/vsd.h vsd_prompt_install; csrc/prompt_install.hip).  segs_dev: int64 [nseg][6] in device memory
        (engine.prompt_segments).  The library checks a table when it first sees it and remembers it by address: the table is kept alive here."""
        self.__dict__.setdefault("_seg_tables", {})[segs_dev.data_ptr()] = segs_dev
        self.ctx.call("vsd_prompt_install", self._p(src_buf), self._p(dst_buf), self._p(segs_dev), int(nseg), int(frame), self.raw_stream(0))

    def prompt_mix_table(self, segs_dev, nseg: int):
        """have the library check the segment table of `prompt_mix` now (one blocking copy) and remember it by address, so that no launch
        waits for that; segs_dev: int64 [nseg][8] in device memory (blocks.mix_segments).  The table is kept alive here."""
        self.__dict__.setdefault("_seg_tables", {})[segs_dev.data_ptr()] = segs_dev
        self.ctx.call("vsd_prompt_mix_table", self._p(segs_dev), int(nseg))

    def prompt_mix(self, src_bufs, weights, dst_buf, segs_dev, nseg: int, frame: int = 0):
        """a weighted mix of 1..4 cached prompts (their PromptBlock.buf, one layout) into `dst_buf` -- a whole block of that layout, or frame
        slot `frame` of a per-frame block -- in ONE launch on this object's own stream (include/vsd.h THE PROMPT MIX; csrc/prompt_mix.hip).
        The sources' addresses and the fp32 weights travel as launch arguments: no upload, no allocation, nobody waits."""
        n = len(src_bufs)
        if n != len(weights) or not 1 <= n <= L.MIX_MAX:
            raise ValueError(f"prompt_mix: {n} source(s) and {len(weights)} weight(s): a mix has 1..{L.MIX_MAX} components, one weight each")
        self.__dict__.setdefault("_seg_tables", {})[segs_dev.data_ptr()] = segs_dev
        srcs = (C.c_void_p * n)(*[b.data_ptr() for b in src_bufs])
        ws = (C.c_float * n)(*[float(w) for w in weights])
        self.ctx.call("vsd_prompt_mix", srcs, ws, n, self._p(dst_buf), self._p(segs_dev), int(nseg), int(frame), self.raw_stream(0))

    # ---- LoRA adapters (include/vsd.h THE ADAPTER FUSE)
    def lora_fuse_table(self, segs_dev, nseg: int):
        """have the library check the segment table of `lora_fuse` now (one blocking copy) and remember it by address; segs_dev: the bytes of
        nseg lib.LoraSeg in device memory (videosd_amd/lora.py AdapterSet).  nseg = 0 forgets it.  The table is kept alive here."""
        if nseg:
            self.__dict__.setdefault("_seg_tables", {})[segs_dev.data_ptr()] = segs_dev
        self.ctx.call("vsd_lora_fuse_table", self._p(segs_dev), int(nseg))
        if not nseg:
            self.__dict__.get("_seg_tables", {}).pop(segs_dev.data_ptr(), None)

    def lora_fuse(self, segs_dev, nseg: int, scales):
        """every segment's fused weight from its base copy and adapters, straight into the packed buffers, ONE launch on this object's own
        stream (csrc/lora.hip).  scales: up to four floats, launch arguments; the missing ones are 0."""
        if len(scales) > L.LORA_MAX:
            raise ValueError(f"lora_fuse: {len(scales)} scales: at most {L.LORA_MAX} adapters")
        self.__dict__.setdefault("_seg_tables", {})[segs_dev.data_ptr()] = segs_dev
        sc = (C.c_float * L.LORA_MAX)(*([float(x) for x in scales] + [0.0] * (L.LORA_MAX - len(scales))))
        self.ctx.call("vsd_lora_fuse", self._p(segs_dev), int(nseg), sc, self.raw_stream(0))

    # ---- per-frame options (include/vsd.h: strength and ControlNet scale per frame of one launch)
    def add_noise_frames(self, x0, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, out):
        """`add_noise_dev` (noise_f32) or `add_noise_seeded` (seeds_dev, kind, draw) -- exactly one of the two -- with image b reading its two
        coefficients at coef_dev + b * coef_stride floats"""
        self.ctx.call("vsd_add_noise_frames", self._p(x0), self._p(noise_f32), self._p(seeds_dev), int(kind), int(draw), self._p(coef_dev),
                      int(coef_stride), hw, batch, self._p(out), self.s)

    def lcm_step_frames(self, eps, sample, noise_f32, seeds_dev, kind, draw, coef_dev, coef_stride, hw, batch, prev, denoised, dec_in=None):
        """`lcm_step_dev` / `lcm_step_seeded` with image b reading its six coefficients at coef_dev + b * coef_stride floats; neither noise
        source: the step adds no noise"""
        self.ctx.call("vsd_lcm_step_frames", self._p(eps), self._p(sample), self._p(noise_f32), self._p(seeds_dev), int(kind), int(draw),
                      self._p(coef_dev), int(coef_stride), hw, batch, self._p(prev), self._p(denoised), self._p(dec_in), self.s)

    def groupnorm_addvec(self, src, addvec, ld_addvec, c, hw, groups, eps, gamma, beta, silu, out, batch=1):
        """`groupnorm` of fp32(src) + fp32(addvec of the image): addvec fp16, image b's vector at addvec + b * ld_addvec halfs"""
        ws = self.workspace("gn", max(1, batch) * int(self.ctx.lib.vsd_groupnorm_workspace_bytes(hw, c, groups)))
        self.ctx.call("vsd_groupnorm_addvec", self._p(src), self._p(addvec), int(ld_addvec), c, hw, max(1, batch), groups, eps, self._p(gamma),
                      self._p(beta), int(silu), self._p(out), self._p(ws), self.s)

    def cn_merge_frames(self, segs_dev, nseg: int, scales_dev, scale_stride: int, batch: int, tensors=None):
        """out = u + scale[image][col] * z for every segment of the table, one launch.  segs_dev: int64 [nseg][6] in device memory =
        (z address, u address, out address, rows per image, channels, scale column) per segment; scales_dev: fp32 [batch][scale_stride].
        tensors: the (z, u, out) tensors the table names, where the caller has them (the op emulator of the tests works on those; unused
        here).  The library checks a table when it first sees it -- one blocking copy, so never first inside a capture -- and remembers it
        by address: the table is kept alive here."""
        self.__dict__.setdefault("_merge_tables", {})[segs_dev.data_ptr()] = segs_dev
        self.ctx.call("vsd_cn_merge_frames", self._p(segs_dev), int(nseg), self._p(scales_dev), int(scale_stride), int(batch), self.s)

    def adain(self, x, stats, stats_ref, rows, c, out, eps=1e-6):
        """reference-only AdaIN: per-channel re-normalisation of x to the banked statistics (fp32 [c][2] sum / sumsq)"""
        self.ctx.call("vsd_adain", self._p(x), self._p(stats), self._p(stats_ref), rows, c, eps, self._p(out), self.s)

    def xattn_fold(self, k, vt, tl, wq, wo, gamma, beta, c, heads, scale, xa1_w, xa1_s, xa1_t, xa2_w):
        """per-prompt constants of one absorbed cross-attention block (include/vsd.h vsd_xattn_fold)"""
        self.ctx.call("vsd_xattn_fold", self._p(k), k.stride(0), self._p(vt), vt.stride(0), tl, self._p(wq), self._p(wo), self._p(gamma),
                      self._p(beta), c, heads, float(scale), self._p(xa1_w), self._p(xa1_s), self._p(xa1_t), self._p(xa2_w), self.s)

    def embed_tokens(self, ids_i64, tok_emb, pos_emb, out):
        n, c = out.shape
        self.ctx.call("vsd_embed_tokens", self._p(ids_i64), self._p(tok_emb), self._p(pos_emb), n, c, tok_emb.shape[0],
                      self._p(out), self.s)

    def postprocess_rgb(self, img, ld, hw, rgb_u8):
        self.ctx.call("vsd_postprocess_rgb", self._p(img), ld, hw, self._p(rgb_u8), self.s)

    def axpy(self, a, b, scale, n, out):
        self.ctx.call("vsd_axpy", self._p(a), self._p(b), scale, n, self._p(out), self.s)

    # ------------------------------------------------------------------ graphs / profiling
    def graph_begin(self):
        self.ctx.call("vsd_graph_begin", self.s)

    def graph_end(self):
        g = C.c_void_p()
        self.ctx.call("vsd_graph_end", self.s, C.byref(g))
        return g

    def graph_launch(self, g):
        self.ctx.call("vsd_graph_launch", g, self.s)

    def graph_destroy(self, g):
        self.ctx.call("vsd_graph_destroy", g)

    # ---- launch sequences (include/vsd.h vsd_seq): single-branch graphs on this object's streams + event edges between them
    def seq_create(self):
        q = C.c_void_p()
        self.ctx.call("vsd_seq_create", C.byref(q))
        return q

    def seq_capture_begin(self, sidx: int):
        self._sidx = sidx
        self.ctx.call("vsd_graph_begin", self.raw_stream(sidx))

    def seq_capture_end(self, seq, sidx: int):
        g = C.c_void_p()
        self.ctx.call("vsd_graph_end", self.raw_stream(sidx), C.byref(g))
        self.ctx.call("vsd_seq_add_graph", seq, g, self.raw_stream(sidx))

    def seq_record(self, seq, sidx: int) -> int:
        ev = C.c_int()
        self.ctx.call("vsd_seq_add_record", seq, self.raw_stream(sidx), C.byref(ev))
        return int(ev.value)

    def seq_wait(self, seq, sidx: int, ev: int):
        self.ctx.call("vsd_seq_add_wait", seq, self.raw_stream(sidx), int(ev))

    def seq_count(self, seq):
        g, e = C.c_int(), C.c_int()
        self.ctx.call("vsd_seq_count", seq, C.byref(g), C.byref(e))
        return int(g.value), int(e.value)

    def seq_launch(self, seq):
        self.ctx.call("vsd_seq_launch", seq)

    def seq_destroy(self, seq):
        self.ctx.call("vsd_seq_destroy", seq)

    def profile_begin(self):
        self.ctx.call("vsd_profile_begin")

    def profile_overhead_ms(self, n: int = 200) -> float:
        ms = C.c_float()
        self.ctx.call("vsd_profile_overhead", self.s, n, C.byref(ms))
        return float(ms.value)

    def profile_end(self):
        self.ctx.call("vsd_profile_end")
        return self.ctx.stage_times()

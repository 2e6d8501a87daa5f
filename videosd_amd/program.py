"""The static program of a plan: the arena its activations come from, the recorder of op calls, and what is done with a recorded
program besides running it -- flattening it for analysis, counting its kernel launches, capturing it into a launch sequence."""
from typing import List, Tuple

import torch

from . import convform as CF
from .packing import _round_up as _ru


class Arena:
    """Bump allocator over large device chunks; `mark`/`rewind` give every denoising step the same addresses."""

    def __init__(self, ops, chunk_bytes: int = 256 << 20):
        self.ops = ops
        self.chunk_bytes = chunk_bytes
        self.chunks: List[torch.Tensor] = []
        self.ci = 0
        self.off = 0
        self.peak = 0

    def alloc(self, rows: int, cols: int, dtype=torch.float16) -> torch.Tensor:
        esz = torch.empty(0, dtype=dtype).element_size()
        nbytes = _ru(rows * cols * esz, 256)
        if getattr(self.ops, "allocator", None) is not None:  # debugging hook (ops.HipOps.allocator): tensor by tensor
            self.peak += nbytes
            return self.ops.empty(rows, cols, dtype=dtype)
        while True:
            if self.ci >= len(self.chunks):  # (a tensor larger than the usual chunk gets a chunk of its own size)
                self.chunks.append(self.ops.empty(max(self.chunk_bytes, nbytes), dtype=torch.uint8))
                self.off = 0
            if self.off + nbytes <= self.chunks[self.ci].numel():
                break
            self.ci += 1
            self.off = 0
        t = self.chunks[self.ci][self.off:self.off + rows * cols * esz].view(dtype).view(rows, cols)
        self.off += nbytes
        self.peak = max(self.peak, sum(c.numel() for c in self.chunks[:self.ci]) + self.off)
        return t

    def mark(self) -> Tuple[int, int]:
        return (self.ci, self.off)

    def rewind(self, m: Tuple[int, int]):
        self.ci, self.off = m


class Recorder:
    """Records op calls as a static program; `run` replays them on the real ops object."""

    def __init__(self, ops):
        self.ops = ops
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self.ops, name)

        def rec(*a, **k):
            self.calls.append((fn, a, k))

        return rec

    def run(self):
        for fn, a, k in self.calls:
            fn(*a, **k)

    # a stretch of the program recorded in two FORMS (same buffers, same results): `flavor(i)` is the program with form i
    def variants(self, form0, form1):
        self.calls.append((_variants, (form0, form1), {}))

    def flavor(self, i: int) -> "Recorder":
        out = Recorder(self.ops)
        for c in self.calls:
            if c[0] is _variants:
                out.calls += c[1][i]
            else:
                out.calls.append(c)
        return out


def _variants(*a, **k):
    raise RuntimeError("a program with variants is run through Recorder.flavor")


SYNC_OPS = ("use_stream", "fork", "join", "signal", "wait")


def flat_calls(calls):
    """the recorded calls as single-op calls: the members of pairs and groups one by one (analysis scripts)"""
    for fn, a, k in calls:
        if fn.__name__ == "pair":
            yield a[0]
            yield a[1]
        elif fn.__name__ == "conv_group":
            for aa, kk in a[0]:
                yield (fn.__self__.conv, aa, kk)
        else:
            yield (fn, a, k)

def launches_by_kind(ops, program: Recorder):
    """kernel launches one replay of a recorded program issues, by kind ("pair_*": two twin calls in one grid; "convs_in_groups" counts
    members, not launches) -> (total, {kind: launches})"""
    kinds = {}

    def count(name, n=1):
        if n:
            kinds[name] = kinds.get(name, 0) + n

    def gn_launches(a, k=None):  # (csrc/norm.hip gn_try_fused: one launch for small images, else statistics + apply)
        if hasattr(ops, "groupnorm_launches"):  # (the library's own decision; the rule below serves the CPU op emulator of the tests)
            return ops.groupnorm_launches(a[2], a[3], a[4], a[5], (k or {}).get("batch", 1))
        c, hw, groups = a[2] + a[3], a[4], a[5]
        cpg = c // groups
        fused = ((hw <= 256 and cpg <= 40) or (hw <= 1024 and cpg <= 20)) and cpg in (40, 8, 16, 20, 4, 12, 10, 2, 6)
        return 1 if fused else 2

    table, mode, flags = ops.tile_override, getattr(ops, "tune_mode", 0), CF.flags_of(ops)

    def conv_reducer(a, k):
        ent = CF.lookup(table, CF.recorded(a, k).key(mode))
        return int(ent is not None and ent[1] > 1 and not ent[2] and not a[3].tile128)

    for fn, a, k in program.calls:
        name = fn.__name__
        if name in SYNC_OPS:
            continue
        if name == "pair":
            (fa, aa, ka), (fb, ab, kb) = a
            op = fa.__name__
            if op == "conv":
                shared = CF.pair_form(aa, ka, ab, kb, table, mode, flags, inkernel=getattr(ops, "inkernel_splitk", True))
                ent = CF.ALONE
                if shared is not None:
                    # throughput mode: the members' own form, as ops.pair.  A pair without an entry counts as reduced in the launch, as
                    # it always has here, although ops.pair runs it in the first member's own form (docs/NOTEBOOK.md: to follow up)
                    sp, own = shared
                    ent = own if mode == 1 else CF.lookup(table, CF.group_key([(aa, ka), (ab, kb)], sp, mode)) or CF.Form(0, sp, True, 3)
                if ent[0] != CF.GROUP_ALONE:
                    count("pair_conv")
                    count("pair_splitk_reduce", int(ent[1] > 1 and not ent[2]))
                else:
                    count("conv", 2)
                    count("splitk_reduce", conv_reducer(aa, ka) + conv_reducer(ab, kb))
            elif op == "groupnorm":
                count("pair_groupnorm")
                count("pair_gn_second", gn_launches(aa, ka) - 1)
            elif op == "groupnorm_addvec":  # (src, addvec, ld, c, hw, groups, ...)
                count("pair_groupnorm_addvec")
                count("pair_gn_second", gn_launches((None, None, aa[3], 0, aa[4], aa[5]), ka) - 1)
            else:
                count("pair_" + op)
            continue
        if name == "conv_group":
            split = k.get("split")
            own = CF.own_splits(a[0], table, mode, flags) if split == CF.OWN_SPLIT else None
            ent = CF.lookup(table, CF.group_key(a[0], split, mode))
            if (split is not None and own is None) or (ent is not None and ent[0] == CF.GROUP_ALONE):
                for aa, kk in a[0]:  # (a group whose table entry -- or a member's own form -- sends the members out alone)
                    count("conv")
                    count("splitk_reduce", conv_reducer(aa, kk))
                continue
            count(name)
            count("convs_in_groups", len(a[0]))
            if ent is not None and not ent[2] and ((own and max(own) > 1) or (not own and ent[1] > 1)):
                count("group_splitk_reduce")
            continue
        count(name)
        if name == "conv":
            count("splitk_reduce", conv_reducer(a, k))
        elif name == "groupnorm":
            count("gn_second", gn_launches(a, k) - 1)
        elif name == "groupnorm_addvec":
            count("gn_second", gn_launches((None, None, a[3], 0, a[4], a[5]), k) - 1)
    return sum(v for k, v in kinds.items() if k != "convs_in_groups"), kinds

def capture(ops, r: Recorder, serial: bool = False):
    """serial=True: every call on stream 0, no edges (the program's fork / join / signal / wait markers are dropped: in one
    in-order stream they hold by construction) -- one graph.
    The recorded program -> a launch sequence (include/vsd.h vsd_seq): every run of kernel calls on one stream becomes ONE
    single-branch hipGraph on that stream, every fork / join / signal / wait an event edge between the two streams, issued
    in program order by `vsd_seq_launch`.  A program without a second stream is one graph, as before.  (One graph with
    parallel branches is what rounds 1-3 captured; on this runtime two such graphs in flight serialise -- DESIGN.md
    section 3, "launches in flight".)"""
    seq = ops.seq_create()
    cur, run, names = 0, [], {}

    def flush():
        nonlocal run
        if run:
            ops.seq_capture_begin(cur)
            try:
                for fn, a, k in run:
                    fn(*a, **k)
            finally:
                ops.seq_capture_end(seq, cur)
            run = []

    try:
        for fn, a, k in r.calls:
            name = getattr(fn, "__name__", "")
            if name not in SYNC_OPS:
                run.append((fn, a, k))
                continue
            if serial:
                continue
            if name == "use_stream":
                if a[0] != cur:
                    flush()
                    cur = a[0]
                continue
            flush()
            if name == "fork":
                ops.seq_wait(seq, 1, ops.seq_record(seq, 0))
            elif name == "join":
                ops.seq_wait(seq, 0, ops.seq_record(seq, 1))
            elif name == "signal":
                names[a[0]] = ops.seq_record(seq, cur)
            else:
                ops.seq_wait(seq, cur, names[a[0]])
        flush()
    except Exception:
        ops.use_stream(0)
        ops.seq_destroy(seq)
        raise
    ops.use_stream(0)
    return seq

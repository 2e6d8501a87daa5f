"""Cases of the conv kernel-form policy (tests/test_convform_host.py): which kernel form -- (tile, split_k, reduce in the launch,
pipeline) -- a conv call runs in and which forms the tuner may time for it (videosd_amd/convform.py).

Three lists.  CALLS: single conv calls that between them take every branch of the policy (the shapes of the real networks; only the
shape fields of a PackedConv and the PRESENCE of the optional tensors matter, so the weights are built directly and every tensor is
a placeholder).  EXPLICIT: calls that name tile / split_k / pipeline / the reduction form themselves.  And the programs
scripts/program_fingerprint.py builds: the MINI network recorded on the op emulator, whose conv, pair and group calls are looked at
call by call under three tuning tables.  What the policy answered at the commit named in tests/golden/conv_forms.json is recorded
there; the test asserts equality."""
import hashlib
import json
import os
import sys
import zlib

import torch

from videosd_amd import lib as L
from videosd_amd.ops import Geom
from videosd_amd.packing import PackedConv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_forms.json")
TABLE = os.path.join(ROOT, "profiles", "tuning_mi355x.json")

MODES = (0, 1)
# the development switches: all off, then each one on
FLAG_SETS = ({}, {"no_halo": True}, {"no_c64": True}, {"no_w8": True})
P = torch.zeros(8)            # "this optional tensor is present"
LN_PART = torch.zeros(1, 2, 2)  # (ln_part's second dimension is read for the descriptor)


def weight(cin, n, ksize=3, geglu=False, tile128=False, ln=False, k=None):
    k = cin * ksize * ksize if k is None else k
    return PackedConv(P.half(), None, n, k, -(-k // 64) * 64, cin, ksize, geglu, P if ln else None, P if ln else None, tile128)


def square(m):
    """Geom arguments (h, w, batch) of M rows: 64 = 8 x 8 ... 4096 = 64 x 64, 20480 = five frames of 64 x 64"""
    batch = 5 if m == 20480 else 1
    side = int(round((m // batch) ** 0.5))
    assert batch * side * side == m
    return side, side, batch


def _calls():
    out = []

    def add(name, g, w, **kw):
        out.append((name, (None, None, g, w, None), kw))

    def conv3(name, cin, n, m, **kw):
        h, w_, b = square(m)
        add(name, Geom.conv(h, w_, batch=b), weight(cin, n), **kw)

    def lin(name, cin, n, m, w=None, **kw):
        add(name, Geom.linear(m), w or weight(cin, n, 1), **kw)

    for cin in (64, 128, 320, 1280):
        for m in (64, 256, 1024, 4096, 20480):
            conv3(f"3x3 {cin}->{cin} M={m}", cin, cin, m)
    for m in (1024, 4096, 20480):
        lin(f"1x1 320->1280 M={m}", 320, 1280, m)
        lin(f"1x1 1280->320 M={m}", 1280, 320, m)
        lin(f"geglu 320->2560 M={m}", 320, 2560, m, w=weight(320, 2560, 1, geglu=True))
        lin(f"softmax tile 320->1024 M={m}", 320, 1024, m, w=weight(320, 1024, 1, tile128=True), act=L.ACT_SOFTMAX, softmax_cols=77)
    for m in (1024, 4096):
        lin(f"ln_part 320->960 M={m}", 320, 960, m, w=weight(320, 960, 1, ln=True), ln_part=LN_PART)
        lin(f"ln_part + rowstat 320->960 M={m}", 320, 960, m, w=weight(320, 960, 1, ln=True), ln_part=LN_PART, rowstat_out=P)
        lin(f"rowstat 320->320 M={m}", 320, 320, m, rowstat_out=P, residual=P)
        conv3(f"chanstat 3x3 320->320 M={m}", 320, 320, m, chanstat_out=P)
        for t_col0 in (0, 64, 128):
            lin(f"out_t t_col0={t_col0} 320->256 M={m}", 320, 256, m, out_t=P, ldt=m, t_col0=t_col0)
        conv3(f"out2 3x3 320->320 M={m}", 320, 320, m, out2=P, add2=P)
        conv3(f"residual2 3x3 320->320 M={m}", 320, 320, m, residual=P, residual2=P)
        conv3(f"out_scale 0.5 3x3 320->320 M={m}", 320, 320, m, out_scale=0.5, residual=P)
        conv3(f"out_scale_dev 3x3 320->320 M={m}", 320, 320, m, out_scale_dev=P)
        lin(f"out_scale_dev 1x1 320->320 M={m}", 320, 320, m, out_scale_dev=P)
        conv3(f"silu + time vector 3x3 320->320 M={m}", 320, 320, m, act=L.ACT_SILU, rowvec=P)
        conv3(f"relu after residual 3x3 64->64 M={m}", 64, 64, m, act=L.ACT_RELU | L.ACT_POST, residual=P)
        conv3(f"silu after residual 3x3 320->320 M={m}", 320, 320, m, act=L.ACT_SILU | L.ACT_POST, residual=P)
        conv3(f"quick-gelu 3x3 320->320 M={m}", 320, 320, m, act=L.ACT_QUICKGELU)
        lin(f"quick-gelu 1x1 320->1280 M={m}", 320, 1280, m, act=L.ACT_QUICKGELU)
    for cin in (64, 320):
        add(f"resized 16x16 -> 32x32 3x3 {cin}->{cin}", Geom.conv(16, 16, up_to=(32, 32)), weight(cin, cin))
        add(f"stride 2 3x3 {cin}->{cin} 32x32", Geom.conv(32, 32, stride=2), weight(cin, cin))
    for c0, c1 in ((64, 64), (320, 320), (640, 320), (64, 8)):
        add(f"two sources {c0}+{c1} -> 320 32x32", Geom.conv(32, 32), weight(c0 + c1, 320), c1=c1)
        add(f"two sources {c0}+{c1} -> 320 1x1 M=1024", Geom.linear(1024), weight(c0 + c1, 320, 1), c1=c1)
    add("odd Cin 4 3x3 -> 320 64x64", Geom.conv(64, 64), weight(4, 320, k=36))
    add("odd Cin 8 3x3 -> 320 64x64", Geom.conv(64, 64), weight(8, 320))
    add("odd Cin 8 3x3 -> 64 512x512", Geom.conv(512, 512), weight(8, 64), act=L.ACT_RELU)
    for side in (32, 512):
        g = Geom.conv(side, side)
        add(f"taesd 64->64 {side}x{side}", g, weight(64, 64))
        add(f"taesd 64->64 relu {side}x{side}", g, weight(64, 64), act=L.ACT_RELU)
        add(f"taesd 64->64 relu after residual {side}x{side}", g, weight(64, 64), act=L.ACT_RELU | L.ACT_POST, residual=P)
        add(f"taesd 64->64 out_scale 0.5 {side}x{side}", g, weight(64, 64), out_scale=0.5)
        add(f"taesd 64->64 out_scale_dev {side}x{side}", g, weight(64, 64), out_scale_dev=P)
        add(f"taesd 64->64 silu after residual {side}x{side}", g, weight(64, 64), act=L.ACT_SILU | L.ACT_POST, residual=P)
        add(f"taesd 64->3 ldo=8 {side}x{side}", g, weight(64, 3), ldo=8)
        add(f"taesd 64->3 ldo=8 residual {side}x{side}", g, weight(64, 3), ldo=8, residual=P)
        add(f"taesd 64->3 own rows {side}x{side}", g, weight(64, 3))
        add(f"taesd 64->4 ldo=8 relu-post {side}x{side}", g, weight(64, 4), ldo=8, act=L.ACT_RELU | L.ACT_POST)
    add("taesd 64->64 two frames 256x256", Geom.conv(256, 256, batch=2), weight(64, 64), act=L.ACT_RELU)
    add("taesd upsample 64->64 256x256 -> 512x512", Geom.conv(256, 256, up_to=(512, 512)), weight(64, 64))
    return out


CALLS = _calls()

# entries a call's own key may hold although the call cannot take them (a key is shared by the calls of one epilogue class)
PLANTED = {"pipeline 10": (L.TILE_256x64, 1, False, 10), "pipeline 7, 256 rows": (L.TILE_256x128, 2, False, 7),
           "pipeline 7, 256x64 inkernel": (L.TILE_256x64, 2, True, 7), "pipeline 7, 128 rows": (L.TILE_128x64, 1, False, 7)}

# calls that name their form (or part of it) themselves: (keywords of conv, value of inkernel_splitk)
EXPLICIT_FORMS = [(dict(tile=L.TILE_128x64), True), (dict(split_k=2), True), (dict(split_k=2), False), (dict(pipeline=5), True),
                  (dict(tile=L.TILE_64x64, split_k=4, pipeline=0), False), (dict(tile=L.TILE_256x64, pipeline=10), True),
                  (dict(tile=L.TILE_256x128, split_k=2, pipeline=7), False), (dict(tile=L.TILE_256x64, split_k=2, pipeline=7), True),
                  (dict(tile=L.TILE_128x128, split_k=0), True)]
EXPLICIT_CALLS = ["3x3 320->320 M=1024", "taesd 64->64 32x32", "taesd 64->3 ldo=8 32x32", "quick-gelu 3x3 320->320 M=1024",
                  "softmax tile 320->1024 M=1024", "odd Cin 8 3x3 -> 320 64x64", "out_scale_dev 3x3 320->320 M=1024",
                  "silu after residual 3x3 320->320 M=1024", "taesd 64->3 own rows 32x32"]

# groups of the calls above, as `tune_group` / `conv_group` get them: (name, member names, split)
OWN = "own"
GROUPS = [("two 1x1", ["1x1 320->1280 M=1024", "1x1 1280->320 M=1024"], None), ("two 1x1 split 6", ["1x1 1280->320 M=1024"] * 2, 6),
          ("with row statistics split 4", ["rowstat 320->320 M=1024", "1x1 320->1280 M=1024"], 4),
          ("with a softmax tile split 2", ["softmax tile 320->1024 M=1024", "1x1 320->1280 M=1024"], 2),
          ("conv1 + shortcut, own splits", ["3x3 1280->1280 M=64", "1x1 1280->320 M=1024"], OWN),
          ("3x3 + 1x1, own splits", ["3x3 320->320 M=1024", "1x1 320->1280 M=1024"], OWN),
          ("chanstat, own splits", ["chanstat 3x3 320->320 M=1024", "3x3 1280->1280 M=256"], OWN)]
PAIRS = [("3x3 320->320 M=1024", "silu + time vector 3x3 320->320 M=1024"), ("3x3 1280->1280 M=64", "3x3 1280->1280 M=64"),
         ("3x3 1280->1280 M=64", "3x3 1280->1280 M=256"), ("resized 16x16 -> 32x32 3x3 64->64", "taesd 64->64 32x32"),
         ("odd Cin 8 3x3 -> 320 64x64", "odd Cin 8 3x3 -> 320 64x64"), ("two sources 64+8 -> 320 32x32", "two sources 64+8 -> 320 32x32"),
         ("1x1 320->1280 M=1024", "1x1 320->1280 M=1024"), ("taesd 64->64 32x32", "taesd 64->64 relu 32x32")]


def table_states(key0, key1, committed):
    """(name, table) a call is resolved under; key0 / key1: its alone-timed and its throughput-mode key"""
    yield "empty", {}
    yield "committed", committed
    for name, ent in PLANTED.items():
        yield name, {key0: ent}  # (in throughput mode: reached through the mode fallback)
    yield "both modes", {key0: PLANTED["pipeline 10"], key1: (L.TILE_64x128, 2, False, 5)}


def call(name):
    for n, a, kw in CALLS:
        if n == name:
            return a, kw
    raise KeyError(name)


def committed_table():
    """profiles/tuning_mi355x.json as `load_tuning` reads it"""
    t = {}
    for k, v in json.load(open(TABLE))["table"]:
        key = tuple(k)
        if len(key) == 9 and key[0] != "group":
            key = key + (0,)
        t.setdefault(key, (int(v[0]), int(v[1]), bool(v[2]), int(v[3])))
    return t


def digest(items):
    """length and sha256 of an ordered list (of forms, of per-call answers): what the fixture keeps of the long ones"""
    items = json.loads(json.dumps(items))  # (tuples and lists, numpy and plain integers: one spelling)
    return [len(items), hashlib.sha256(json.dumps(items).encode()).hexdigest()[:16]]


def form4(f):
    return None if f is None else [int(f[0]), int(f[1]), bool(f[2]), int(f[3])]


# ------------------------------------------------------------------------------------------------ the recorded programs
def programs():
    """(name, recorded calls of the two-stream form, of the one-stream form) of every configuration of scripts/program_fingerprint.py"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import program_fingerprint as pf

    weights, texts = pf.inputs()
    for cfg in pf.configurations():
        has_gpu = torch.cuda.is_available
        torch.cuda.is_available = lambda: False  # (on the emulator also where there is a GPU: the fixture was recorded on it)
        try:
            eng = pf.build(*cfg, weights, texts, use_graph=False, autotune=False)
        finally:
            torch.cuda.is_available = has_gpu
        yield cfg[0], eng.program, eng.program_serial


SYNTH_CONV = [(L.TILE_64x64, 1, True, 3), (L.TILE_128x64, 2, False, 3), (L.TILE_128x128, 2, True, 5), (L.TILE_128x128, 1, False, 7),
              (L.TILE_256x128, 1, False, 3), (L.TILE_64x64, 4, True, 0), (L.TILE_128x64, 2, False, 7), (L.TILE_64x128, 3, True, 5),
              (L.TILE_128x128, 2, True, 8), (L.TILE_256x64, 1, False, 10), (L.TILE_64x64, 2, True, 3)]
SYNTH_GROUP = [(L.TILE_64x64, True, 3), (L.TILE_128x64, False, 5), (-1, True, 0), (L.TILE_128x128, True, 9), (L.TILE_64x128, False, 3)]


def pick(key, choices):
    return choices[zlib.crc32(repr(key).encode()) % len(choices)]


def synthetic_conv_entries(conv_keys):
    """a made-up table over a program's own conv keys (the committed table knows few shapes of the MINI network), so that its pairs
    and groups meet members of every kind: split or not, halo form, 256-row tiles, entries the call cannot take.  Alone-timed
    keys only for two thirds of them: the rest falls to the heuristic, and throughput-mode lookups take the mode fallback."""
    return {k: pick(k, SYNTH_CONV) for k in conv_keys if k[-1] == 0 and zlib.crc32(repr(k).encode()) % 3}


def synthetic_group_entry(key):
    """the entry of a group / pair key, or None (one in four has none); the split field is the key's"""
    if zlib.crc32(repr(key).encode()) % 4 == 0:
        return None
    t, ink, pl = pick(key, SYNTH_GROUP)
    sp = key[key.index("split") + 1] if "split" in key else 1
    return (t, 1, True, 0) if t == -1 else (t, sp, ink, pl)


def conv_members(calls):
    """the conv calls of a recorded program one by one, members of pairs and groups included: (args, kwargs)"""
    for fn, a, k in calls:
        name = fn.__name__
        if name == "conv":
            yield a, k
        elif name == "conv_group":
            yield from a[0]
        elif name == "pair" and a[0][0].__name__ == "conv" and a[1][0].__name__ == "conv":
            yield a[0][1], a[0][2]
            yield a[1][1], a[1][2]


def synthetic_table(ops, calls):
    """the made-up table of one program (see synthetic_conv_entries): conv entries first, then -- pairs share a grid at the split
    their members' OWN entries give -- the entries of its groups and pairs"""
    ops.tune_mode, ops.tile_override = 0, {}
    ops.tile_override.update(synthetic_conv_entries([ops.conv_key_of(a[2], a[3], k) for a, k in conv_members(calls)]))
    groups = {}
    for fn, a, k in calls:
        key = None
        if fn.__name__ == "conv_group":
            key = ops.group_key(a[0], k.get("split"))
        elif fn.__name__ == "pair" and a[0][0].__name__ == "conv" and a[1][0].__name__ == "conv":
            sp = ops.pair_split(a[0][1], a[0][2], a[1][1], a[1][2])
            key = None if sp is None else ops.group_key([a[0][1:], a[1][1:]], sp)
        if key is not None and synthetic_group_entry(key) is not None:
            groups[key] = synthetic_group_entry(key)
    ops.tile_override.update(groups)
    return ops.tile_override


def program_answers(ops, calls, resolved, pair_form):
    """what the policy says about every conv, pair and group call of a recorded program, in order.  resolved(ops, args, kwargs) ->
    the form a conv call runs in; pair_form(ops, aa, ka, ab, kb) -> (shared split or None, the members' own form)"""
    out = []
    for a, k in conv_members(calls):
        out.append(["conv", ops.conv_key_of(a[2], a[3], k), form4(resolved(ops, a, k))])
    for fn, a, k in calls:
        if fn.__name__ == "conv_group":
            split = k.get("split")
            out.append(["group", ops.group_key(a[0], split), ops.own_splits(a[0]) if split == OWN else None,
                        [form4(f) for f in ops.group_candidates(a[0], split)]])
        elif fn.__name__ == "pair" and a[0][0].__name__ == "conv" and a[1][0].__name__ == "conv":
            members = (a[0][1], a[0][2], a[1][1], a[1][2])
            sp, own = pair_form(ops, *members)
            assert sp == ops.pair_split(*members)
            out.append(["pair", sp, form4(own) if sp is not None else None, None if sp is None else ops.group_key([a[0][1:], a[1][1:]], sp)])
    return out


def cpu_hip_ops():
    """HipOps without a device: the plain attributes its policy reads, CPU tensors for scratch.  Good for everything short of a
    launch: keys, descriptors (`conv(..., _desc_only=True)`), own_splits, pair_split, group_candidates."""
    from videosd_amd.ops import HipOps

    class CpuHipOps(HipOps):
        def __init__(self):
            self.device, self.stream, self.tile_override = torch.device("cpu"), None, {}
            self.tune_mode, self.inkernel_splitk, self.default_pipeline = 0, True, 3
            self.no_halo = self.no_c64 = self.no_w8 = False
            self.one_launch_bias_us = 0.5
            self._sidx, self._widx, self._ws, self._counters, self._chan_counters = 0, None, {}, [], []

        def workspace(self, key, nbytes):
            return P

        def _counter_set(self, sets, n):
            return P

        @property
        def groupnorm_launches(self):  # (the library's launch count is not to be had: launches_by_kind falls to its own rule)
            raise AttributeError("groupnorm_launches")

    return CpuHipOps()


def desc_form(ops, a, kw):
    """the form a call's descriptor names; the reduction form shows only where there is something to reduce"""
    d = ops.conv(*a, _desc_only=True, **kw)
    return (int(d.tile), int(d.split_k), bool(d.counters), int(d.pipeline))


CONV_KINDS = ("conv", "splitk_reduce", "pair_conv", "pair_splitk_reduce", "conv_group", "convs_in_groups", "group_splitk_reduce")


def conv_launches(counted):
    """of `launches_by_kind`'s answer: the total and the kinds the conv policy decides"""
    total, kinds = counted
    return [total, {k: kinds[k] for k in CONV_KINDS if k in kinds}]

"""Which kernel form -- (tile, split_k, reduce in the launch, pipeline) -- a conv call runs in, and which forms it may run in: plain
data and pure functions.  `resolve` is what `HipOps.conv` does before it fills a descriptor: the call's table entry (`lookup`), else
the heuristic (`choose_tile`), then the safety nets.  `candidates` / `group_candidates` list what the tuner times; `own_splits` /
`pair_form` say when calls may share a grid without changing their bits.  Nothing here touches the device, so the launch accounting,
the scripts and the tests' op emulator (a `tile_override` and nothing else) ask the same functions as HipOps."""
from collections import namedtuple
from typing import NamedTuple

from . import lib as L
from .packing import PackedConv


class Form(NamedTuple):
    """a kernel form; still the 4-tuple of the tuning table, `tile_override` and GROUP_FORMS"""
    tile: int
    split_k: int
    inkernel: bool
    pipeline: int

    @property
    def ring_order(self) -> bool:
        """sums over K in the order the buffer-load ring does: at one split_k every such form gives the same bits
        (scripts/conv_bits_probe.py).  Not the halo-patch form (channel block outer, tap inner), not the 256-row tiles."""
        return self.pipeline != 7 and self.tile not in (L.TILE_256x128, L.TILE_256x64, L.TILE_256x256)


# the development switches of an ops object that bear on the choice (HipOps.__init__ reads them from the environment)
Flags = namedtuple("Flags", "no_halo no_c64 no_w8 default_pipeline", defaults=(False, False, False, 3))


def flags_of(ops) -> Flags:
    return Flags(*(getattr(ops, f, d) for f, d in Flags._field_defaults.items()))


GROUP_FORMS = [(L.TILE_64x64, 3), (L.TILE_64x64, 5), (L.TILE_64x128, 3), (L.TILE_64x128, 5), (L.TILE_128x64, 3), (L.TILE_128x64, 5),
               (L.TILE_128x128, 3), (L.TILE_128x128, 5), (L.TILE_128x128, 8), (L.TILE_128x128, 9)]
GROUP_ALONE = -1  # tile field of a group's table entry: "these members are faster as launches of their own"
OWN_SPLIT = "own"  # conv_group(split=...): every member at the split ITS OWN table entry has (split field 0 in the group's entry)
ALONE = Form(GROUP_ALONE, 1, True, 0)

# Epilogue classes of the tuning key.  By scripts/wg_timeline.py the epilogue kind moves a workgroup's fixed cost from 1.0
# to 4.6 us, and some classes exclude kernel forms (statistics outputs: no reducer kernel; softmax: 128-column tiles;
# anything but the plain one: no halo-patch form) -- layers of one (M, N, K) with different epilogues get their own entry.
EPI_PLAIN, EPI_LN, EPI_ROWSTAT, EPI_LN_ROWSTAT, EPI_SOFTMAX, EPI_GENERAL, EPI_PLAIN_ACT = range(7)

NOT_PLAIN = ("residual2", "out2", "out_t", "rowstat_out", "chanstat_out", "ln_part")  # what the halo form's plain epilogue lacks
OPTIONAL = ("residual", "out_scale_dev") + NOT_PLAIN  # the tensors of a call whose presence the policy looks at


class ConvCall(NamedTuple):
    """what the policy looks at in one conv call: shapes, epilogue scalars, and which optional tensors are there"""
    m: int
    n: int
    kp: int
    cin: int
    c1: int
    ksize: int
    stride: int
    batch: int
    ho: int
    wo: int
    resized: bool
    geglu: bool
    tile128: bool
    act: int
    out_scale: float
    ldo: int
    t_col0: int
    present: frozenset

    def has(self, *names) -> bool:
        return not self.present.isdisjoint(names)

    @property
    def wide(self) -> bool:  # epilogues that need whole 128-column tiles and no split-K
        return self.geglu or self.tile128

    @property
    def epilogue_class(self) -> int:
        if self.tile128 or (self.act & 0xff) == L.ACT_SOFTMAX:
            return EPI_SOFTMAX
        if self.has("chanstat_out", "residual2", "out2", "out_scale_dev") or self.out_scale != 1.0:
            return EPI_GENERAL
        if self.has("ln_part"):
            return EPI_LN_ROWSTAT if self.has("rowstat_out") else EPI_LN
        if self.has("rowstat_out"):
            return EPI_ROWSTAT
        # (activations other than none / ReLU / SiLU / ReLU-after-residual leave the halo-patch form: quick-GELU of CLIP)
        return EPI_PLAIN if (self.act & 0xff) in (L.ACT_NONE, L.ACT_RELU, L.ACT_SILU, L.ACT_GEGLU) else EPI_PLAIN_ACT

    def key(self, mode: int):
        # the call's key of the tuning table.  Last field: 0 = the choice that is fastest ALONE on an idle GPU (a lone launch:
        # latency), 1 = the choice that costs the least when FOUR launch lanes are busy (throughput): see HipOps.tune_conv
        return (self.m, self.n, self.kp, self.ksize, self.stride, self.resized, self.geglu, self.t_col0, self.epilogue_class, int(mode))

    @property
    def buffer_path(self) -> bool:
        # on the buffer-load operand path (`p.fast` of csrc/conv_gemm.hip): what the 256-row tiles, the eight-wave forms and
        # vsd_conv_gemm_group take
        return self.cin % 64 == 0 and self.c1 % 64 == 0 and not self.resized

    @property
    def halo_ok(self) -> bool:
        """What vsd_conv_gemm's halo-patch form (pipeline 7) accepts: a 3x3 stride-1 conv with the plain epilogue."""
        return (not self.has(*NOT_PLAIN) and not self.geglu and
                self.ksize == 3 and self.stride == 1 and self.cin % 64 == 0 and self.c1 % 64 == 0 and self.n % 8 == 0 and
                self.out_scale == 1.0 and self.act in (L.ACT_NONE, L.ACT_RELU, L.ACT_SILU, L.ACT_RELU | L.ACT_POST))

    @property
    def c64_ok(self) -> bool:
        """What the persistent 64-input-channel form (pipeline 10, csrc/conv_c64.hip) accepts: the halo form's layer with Cin = 64
        from one source and Cout = 64 -- or Cout <= 8 into 8-wide rows without a residual (TAESD's 64 -> 3 / 64 -> 4 projections)."""
        if self.cin != 64 or self.c1:
            return False
        if self.n == 64:
            return self.halo_ok
        return (self.n <= 8 and self.ldo == 8 and not self.has("residual", *NOT_PLAIN) and not self.geglu and self.ksize == 3 and
                self.stride == 1 and self.out_scale == 1.0 and self.act in (L.ACT_NONE, L.ACT_RELU, L.ACT_SILU))


def conv_call(g, w: PackedConv, *, c1=0, act=L.ACT_NONE, out_scale=1.0, ldo=None, t_col0=0, **kw) -> ConvCall:
    """from a call's Geom, weights and keyword arguments -- `HipOps.conv`'s own, or a recorded call's (args[2], args[3], kwargs)"""
    return ConvCall(g.m, w.n, w.kp, w.cin, c1 or 0, g.ksize, g.stride, g.batch, g.ho, g.wo, (g.hi, g.wi) != (g.hs, g.ws), w.geglu,
                    w.tile128, L.ACT_GEGLU if w.geglu else act, out_scale, w.n_out if ldo is None else ldo, t_col0,
                    frozenset(k for k in OPTIONAL if kw.get(k) is not None))


def recorded(args, kwargs: dict) -> ConvCall:  # of a recorded call: (src0, src1, g, w, out), its keyword arguments
    return conv_call(args[2], args[3], **kwargs)


def named_form(kwargs: dict) -> dict:  # the part of a form a recorded call names itself
    return {k: kwargs[k] for k in Form._fields if k in kwargs}


def unnamed(kwargs: dict) -> dict:  # a recorded call's keyword arguments without that part
    return {k: v for k, v in kwargs.items() if k not in Form._fields}


def lookup(table: dict, key):
    """the entry of `key`; for a throughput-mode key that has none, the alone-timed choice (conv and group keys end in the mode)"""
    ent = table.get(key)
    return table.get(key[:-1] + (0,)) if ent is None and key[-1] == 1 else ent


def choose_tile(m: int, n: int, kp: int, geglu: bool = False, t_col0: int = 0):
    """Heuristic (tile, split_k): minimise padding waste, prefer big tiles, then split K until the grid
    covers the 256 CUs.  The engine's autotuner can override this per layer."""
    cands = [L.TILE_128x128, L.TILE_64x128] if geglu else [L.TILE_128x128, L.TILE_128x64, L.TILE_64x128, L.TILE_64x64]
    pen = {L.TILE_128x128: 1.0, L.TILE_128x64: 1.12, L.TILE_64x128: 1.12, L.TILE_64x64: 1.3}
    kt = kp // 64
    best = None
    for t in cands:
        bm, bn = L.TILE_DIMS[t]
        if t_col0 % bn:
            continue
        tm, tn = -(-m // bm), -(-n // bn)
        blocks = tm * tn
        waste = (tm * bm * tn * bn) / float(m * n)
        split = 1
        if not geglu and blocks < 256 and kt >= 8:
            split = max(1, min(-(-320 // blocks), kt // 4))
        total = blocks * split
        fill = min(1.0, total / 256.0)
        # rounds of 256-CU waves at ~2 blocks/CU
        cost = waste * pen[t] / max(fill, 0.05) * (1.0 + 0.04 * (split - 1))
        if best is None or cost < best[0]:
            best = (cost, t, split)
    return best[1], best[2]


def resolve(call: ConvCall, table: dict, mode: int, flags: Flags, tile=None, split_k=None, pipeline=None, inkernel=True) -> Form:
    """the form a call runs in.  tile / split_k / pipeline / inkernel: what the caller names itself (a named tile keeps the table out)"""
    if tile is None:
        ent = lookup(table, call.key(mode))
        if ent is not None:
            # (the key names the epilogue class since round 4: an entry always fits the call it is looked up for -- rounds
            #  2-3 keyed on the shape alone and widened 64-column tiles / left the halo form after the fact)
            tile, split_k, inkernel, pipeline = ent
        else:
            tile, sk = choose_tile(call.m, call.n, call.kp, call.wide, call.t_col0 if call.has("out_t") else 0)
            split_k = sk if split_k is None else split_k
    split_k = split_k or 1
    if call.tile128:
        inkernel = True  # (the tile softmax runs in the reducing workgroup's epilogue)
    if pipeline == 10 and (flags.no_c64 or call.has("out_scale_dev") or not call.c64_ok):
        # (safety net, as below: an entry shared by a call the persistent form cannot take)
        pipeline, tile, split_k = (7, L.TILE_256x64, 1) if call.n % 8 == 0 else (3, L.TILE_64x64, 1)
    if pipeline == 7 and (flags.no_halo or call.has("out_scale_dev") or not call.halo_ok):
        # (safety net: a plain-class entry shared by a call the halo form cannot take -- e.g. SiLU after the residual)
        pipeline = 3
        tile = {L.TILE_256x128: L.TILE_128x128, L.TILE_256x64: L.TILE_128x64}.get(tile, tile)
        inkernel = True
    return Form(tile, split_k, bool(inkernel), flags.default_pipeline if pipeline is None else pipeline)


def candidates(call: ConvCall, mode: int, flags: Flags):
    """every form the tuner times for one call (HipOps.tune_conv), in the order it times them"""
    kt = call.kp // 64
    tiles = [L.TILE_128x128, L.TILE_64x128] if call.wide else [L.TILE_128x128, L.TILE_128x64, L.TILE_64x128, L.TILE_64x64]
    # the 256x128 tile (buffer-load path only: Cin % 64 == 0, no resize) pays when M is large (batched frames, TAESD)
    if call.buffer_path and call.m >= 1024:
        tiles = tiles + [L.TILE_256x128]
    # the eight-wave forms only among the throughput-mode candidates: alone on an idle chip they measure 0-40 % slower than the
    # four-wave ones, with four lanes busy 7-18 % faster on the wide 1 x 1 layers -- profiles/round6_w8_probe_*.txt
    w8_ok = call.buffer_path and not flags.no_w8 and mode == 1
    # the 256x256 tile (eight waves, unsplit, row-banded epilogue): least L2 -> LDS fill per FLOP; for layers with enough of both
    # M and N to give the chip's lanes something to do (a softmax / transposed-output tile is 128 columns: not for those)
    huge_ok = w8_ok and call.m >= 1024 and call.n >= 512 and not call.tile128 and not call.has("out_t", "chanstat_out")
    halo_ok = not call.wide and call.halo_ok
    one_launch_only = call.has("rowstat_out", "chanstat_out") or call.tile128  # (statistics outputs / softmax: no reducer kernel)

    def halo_forms(t, patch_rows):  # split-K (over channel blocks) = the two-kernel form
        hblocks = call.batch * -(-call.ho // patch_rows) * -(-call.wo // 16) * -(-call.n // L.TILE_DIMS[t][1])
        for sp in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20):
            if sp > call.cin // 64 or (sp > 1 and hblocks * sp > 1536):
                break
            yield Form(t, sp, False, 7)
            if sp > 1 and hblocks <= L.SPLITK_MAX_TILES:
                yield Form(t, sp, True, 7)

    cands = [Form(L.TILE_256x256, 1, False, pl) for pl in (8, 9)] if huge_ok else []
    for t in tiles:
        bm, bn = L.TILE_DIMS[t]
        if call.has("out_t") and call.t_col0 % bn:
            continue
        blocks = -(-call.m // bm) * -(-call.n // bn)
        # pipelines 8 / 9: the 3-stage ring on eight waves (two per SIMD), buffer-load path, tiles of 128 x 128 and larger
        w8 = (8, 9) if w8_ok and bm * bn >= 128 * 128 else ()
        cands += [Form(t, 1, False, pl) for pl in ((3, 5) if t == L.TILE_256x128 else (0, 3, 4, 5, 6)) + w8]
        if halo_ok and bm == 128:  # LDS halo patch (pipeline 7), 8x16 patches
            cands += halo_forms(t, 8)
        if call.geglu or blocks >= 384:
            continue
        for sp in (2, 3, 4, 6, 8, 12, 16, 24):
            if sp > kt // 2 or blocks * sp > 1536:
                break
            for pl in ((3, 5) if t == L.TILE_256x128 else (0, 3, 5)) + w8:
                if not one_launch_only:
                    cands.append(Form(t, sp, False, pl))
                cands.append(Form(t, sp, True, pl))
    if halo_ok:  # 16x16 patches (8 waves): half the weight traffic of the 8x16 patch
        for t in (L.TILE_256x128, L.TILE_256x64):
            cands += halo_forms(t, 16)
    # the persistent 64 -> 64 channel form (csrc/conv_c64.hip, pipeline 10): TAESD's block convs
    if not flags.no_c64 and not call.wide and not call.has("out_scale_dev") and call.c64_ok:
        cands.append(Form(L.TILE_256x64, 1, False, 10))
    return cands


# ---- calls that share a grid (vsd_conv_gemm_group): groups, and the twin pairs of the UNet and the ControlNet encoder.
#      calls: recorded calls [(args, kwargs), ...]
def group_key(calls, split, mode: int):
    k = ["group"]
    for a, _kw in calls:
        k += [a[2].m, a[3].n, a[3].kp]
    if split is not None:  # (a twin pair: the members' own split over K is part of the problem, see pair_form; "own": OWN_SPLIT)
        k += ["split", 0 if split == OWN_SPLIT else int(split)]
    return tuple(k) + (int(mode),)


def own_splits(calls, table: dict, mode: int, flags: Flags):
    """the split over K each member has as a launch of its own (its table entry / default form), or None when a member's own
    form sums over K in another order than the buffer-load ring does (the halo-patch form, the 256-row tiles' callers keep
    their form) -- then the group's bits would differ from the launches' and the members go out alone"""
    forms = [resolve(recorded(a, kw), table, mode, flags) for a, kw in calls]
    return [f.split_k for f in forms] if all(f.ring_order for f in forms) else None


def group_candidates(calls, table: dict, mode: int, flags: Flags, split=None):
    """the kernel forms `tune_group` times: GROUP_FORMS at the given split over K (slabs reduced by one more launch for the group,
    or in the launch), and the members as launches of their own"""
    if split == OWN_SPLIT:  # (entry's split field 0 = every member at its own)
        own = own_splits(calls, table, mode, flags)
        if own is None:
            return [ALONE]
        sp, any_split = 0, max(own) > 1
    else:
        sp, any_split = split or 1, (split or 1) > 1
    cands = [Form(t, sp, True, pl) for t, pl in GROUP_FORMS]
    if any_split and not any(a[3].tile128 or recorded(a, kw).has("rowstat_out", "chanstat_out") for a, kw in calls):
        cands += [Form(t, sp, False, pl) for t, pl in GROUP_FORMS]
    return cands + [ALONE]


def pair_form(aa, ka, ab, kb, table: dict, mode: int, flags: Flags, inkernel=True):
    """Two twin convs (recorded: args and kwargs of each) share a grid when both are on the buffer-load operand path (what
    vsd_conv_gemm_group takes) and the forms they have as launches of their own sum over K in the SAME order -- the same split_k,
    both in ring order.  Then the pair at that split gives the bits the two launches give, and a frame does not depend on which
    form of the program ran it.  -> (that split_k, the first member's own form as a group's: what the pair runs in when its key
    has no entry, and always in throughput mode), or None (launch them one by one)."""
    forms = []
    for a, k in ((aa, ka), (ab, kb)):
        call = recorded(a, k)
        if not call.buffer_path or call.ksize * call.ksize > 32:
            return None
        forms.append(resolve(call, table, mode, flags, **{"inkernel": inkernel, **named_form(k)}))
        if not forms[-1].ring_order or forms[-1].split_k != forms[0].split_k:
            return None
    f = forms[0]
    return f.split_k, Form(f.tile, f.split_k, f.inkernel or f.split_k <= 1, f.pipeline if f.pipeline in (5, 8, 9) else 3)

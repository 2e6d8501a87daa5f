"""THE ADAPTER FUSE of include/vsd.h restated in numpy, seeded synthetic adapters, writers for the key conventions of adapter files, and
the case list that the host twin (tests/test_lora_host.py) and the kernel (tests/test_lora_gpu.py) are both held to.

The restatement is plain np.float32 array arithmetic: every operation rounds on its own, there is no fma (the product of two fp16
values is exact in fp32, so a rank step needs none)."""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

F32, F16 = np.float32, np.float16
CANARY = 0x5A5A  # an fp16 pattern no computation here produces (~210.5): pad columns and rows of other tensors must keep it
MAP_ID, MAP_GEGLU = 0, 1
COPY_NONE, COPY_RAW, COPY_FRAG = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------------ the restatement
def fuse_numpy(w0, adapters, scales):
    """Wf of the contract.  w0: fp16 [rows][K]; adapters: (up fp16 [rows][r], down fp16 [r][K], a, slot) in slot order; scales: by slot."""
    assert w0.dtype == F16
    acc = w0.astype(F32)
    for up, down, a, slot in adapters:
        s = F32(scales[slot]) if slot < len(scales) else F32(0)
        if s == 0:
            continue  # skipped, not multiplied by zero
        d = np.zeros(acc.shape, F32)
        for j in range(up.shape[1]):
            d = d + up[:, j:j + 1].astype(F32) * down[j:j + 1, :].astype(F32)
        sa = F32(s) * F32(a)
        acc = acc + sa * d
    return acc.astype(F16)


def row_sum_numpy(x):
    """the contract's order: 64 partials, chunk c of 8 columns on partial c mod 64, elements in increasing k, then the fixed tree"""
    rows, k = x.shape
    assert x.dtype == F32 and k % 8 == 0
    nch = k // 8
    passes = -(-nch // 64)
    xp = np.zeros((rows, passes * 64 * 8), F32)  # (the partials start at +0 and +0 + 0 = +0: the padding adds nothing)
    xp[:, :k] = x
    xp = xp.reshape(rows, passes, 64, 8)
    p = np.zeros((rows, 64), F32)
    for c in range(passes):
        live = min(64, nch - c * 64)  # a partial only adds the chunks that exist
        for e in range(8):
            p[:, :live] = p[:, :live] + xp[:, c, :live, e]
    h = 32
    while h >= 1:
        p[:, :h] = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0].copy()


def fold_numpy(wf, gamma, beta, bias):
    """(wp fp16, ln_s fp32, ln_t fp32) of a LayerNorm-folded destination, by source row"""
    w = wf.astype(F32)
    wp = (w * gamma[None, :].astype(F32)).astype(F16)
    s = row_sum_numpy(wp.astype(F32))
    t = row_sum_numpy(w * beta[None, :].astype(F32))
    if bias is not None:
        t = t + bias.astype(F32)
    return wp, s, t


def map_rows(kind, rows):
    """destination row (before row0) of every source row"""
    r = np.arange(rows)
    if kind == MAP_ID:
        return r
    f = rows // 2
    rr = np.where(r < f, r, r - f)
    return 128 * (rr // 64) + np.where(r < f, 0, 64) + rr % 64


def frag_numpy(w2d):
    """pack_mfma_frag of packing.py on a numpy [N][K] matrix"""
    n, k = w2d.shape
    return w2d.reshape(n // 16, 16, k // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(-1).copy()


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Seg:
    """one segment: the arrays it reads and the geometry of what it writes"""
    rows: int
    k: int
    kp: int
    n_dst: int                       # rows of the destination matrix (and of ln_s / ln_t)
    row0: int = 0
    map: int = MAP_ID
    fold: bool = False
    bias: bool = False
    copy: int = COPY_NONE
    adapters: List[Tuple[int, float, int]] = field(default_factory=list)  # (rank, alpha, slot)
    dst: str = ""                    # name of the destination it shares with other segments ("" = its own)
    zero_from: Optional[int] = None  # the columns c >= zero_from of every 8 are zero in W0 and down (padded input channels)
    neg_zero: bool = False           # plant -0 in W0


@dataclass
class Case:
    name: str
    segs: List[Seg]
    scales: Tuple[float, ...]


def case_list():
    A = lambda *a: list(a)  # noqa: E731
    return [
        Case("conv_out_rows4_k72", [Seg(4, 72, 128, 4, adapters=A((4, 4.0, 0)))], (0.8,)),
        Case("conv_in_padded_channels", [Seg(24, 72, 128, 24, adapters=A((12, 6.0, 0)), zero_from=4)], (1.0,)),
        Case("rank1_negative_scale", [Seg(64, 64, 64, 64, adapters=A((1, 1.0, 0)))], (-0.75,)),
        Case("four_adapters_320_frag", [Seg(320, 320, 320, 320, copy=COPY_FRAG,
                                            adapters=A((1, 1.0, 0), (4, 8.0, 1), (12, 12.0, 2), (128, 64.0, 3)))], (0.5, -0.25, 0.0, 1.25)),
        Case("row_offset_two_of_four", [Seg(24, 64, 64, 88, row0=40, adapters=A((4, 2.0, 1), (12, 12.0, 3)))], (9.0, 0.6, 9.0, -1.5)),
        Case("geglu_two_tiles_fold_bias", [Seg(256, 64, 64, 256, map=MAP_GEGLU, fold=True, bias=True, adapters=A((4, 4.0, 0)))], (0.7,)),
        Case("fold_bias_two_passes_rank40", [Seg(24, 576, 576, 48, row0=24, fold=True, bias=True,
                                                 adapters=A((40, 20.0, 0), (4, 4.0, 1), (1, 3.0, 2)))], (0.3, 1.0, -2.0)),
        Case("fold_raw_copy", [Seg(64, 64, 64, 64, fold=True, copy=COPY_RAW, adapters=A((4, 1.0, 0)))], (1.0,)),
        Case("fold_frag_320", [Seg(320, 320, 320, 320, fold=True, copy=COPY_FRAG, adapters=A((4, 4.0, 0)))], (0.8,)),
        Case("all_zero_scales", [Seg(24, 72, 128, 24, adapters=A((4, 4.0, 0), (12, 1.0, 2)), neg_zero=True)], (0.0, 5.0, 0.0, 0.0)),
        Case("grid_stride_640_rows", [Seg(640, 64, 64, 640, adapters=A((4, 4.0, 0)))], (1.0,)),
        Case("k320_rank128", [Seg(24, 320, 320, 24, adapters=A((128, 128.0, 0)))], (1.0,)),
        # qkv-like: three matrices, one folded destination and one pair of fold vectors, one launch
        Case("three_segments_one_destination", [Seg(24, 64, 64, 72, row0=0, fold=True, dst="qkv", adapters=A((4, 4.0, 0))),
                                                Seg(24, 64, 64, 72, row0=24, fold=True, dst="qkv", adapters=A((12, 4.0, 0), (4, 4.0, 1))),
                                                Seg(24, 64, 64, 72, row0=48, fold=True, dst="qkv", adapters=A((1, 1.0, 1)))], (0.5, 0.9)),
    ]


def make_arrays(case: Case, seed=0):
    """-> per segment a dict of numpy arrays: w0, up_i, down_i, gamma, beta, bias and the destinations dst / ln_s / ln_t / copy as they
    are BEFORE the call (canaries; a shared destination is one array).  Seeded by the case's name."""
    rng = np.random.default_rng([seed] + [ord(c) for c in case.name])
    shared = {}
    out = []
    for g in case.segs:
        a = {}
        a["w0"] = (rng.standard_normal((g.rows, g.k)) * 0.05).astype(F16)
        if g.neg_zero:
            a["w0"][::3, ::5] = F16(-0.0)
        for i, (r, _alpha, _slot) in enumerate(g.adapters):
            a[f"up{i}"] = (rng.standard_normal((g.rows, r)) * 0.1).astype(F16)
            a[f"down{i}"] = (rng.standard_normal((r, g.k)) * 0.1).astype(F16)
        if g.zero_from is not None:
            z = (np.arange(g.k) % 8) >= g.zero_from
            a["w0"][:, z] = 0
            for i in range(len(g.adapters)):
                a[f"down{i}"][:, z] = 0
        if g.fold:
            a["gamma"] = (1.0 + 0.1 * rng.standard_normal(g.k)).astype(F32)
            a["beta"] = (0.1 * rng.standard_normal(g.k)).astype(F32)
            if g.bias:
                a["bias"] = (0.1 * rng.standard_normal(g.rows)).astype(F32)
        key = g.dst or id(g)
        if key not in shared:
            d = {"dst": np.full((g.n_dst, g.kp), CANARY, np.uint16).view(F16)}
            if g.fold:
                d["ln_s"] = np.full(g.n_dst, 1234.5, F32)
                d["ln_t"] = np.full(g.n_dst, -4321.5, F32)
            shared[key] = d
        a.update(shared[key])
        if g.copy == COPY_RAW:
            a["copy"] = np.full((g.rows, g.k), CANARY, np.uint16).view(F16)
        elif g.copy == COPY_FRAG:
            a["copy"] = np.full(g.n_dst * g.k, CANARY, np.uint16).view(F16)
        out.append(a)
    return out


def adapters_of(g: Seg, a):
    return [(a[f"up{i}"], a[f"down{i}"], F32(alpha / r), slot) for i, (r, alpha, slot) in enumerate(g.adapters)]


def expect_numpy(case: Case, arrays):
    """the destinations after the call, by the restatement, written into COPIES of the arrays' destinations: a list of dicts
    {dst, ln_s, ln_t, copy} per segment (a shared destination: the same object in each of its segments)"""
    copies = {}
    out = []
    for g, a in zip(case.segs, arrays):
        res = {}
        for name in ("dst", "ln_s", "ln_t"):
            if name in a:
                res[name] = copies.setdefault(id(a[name]), a[name].copy())
        wf = fuse_numpy(a["w0"], adapters_of(g, a), case.scales)
        dr = g.row0 + map_rows(g.map, g.rows)
        val = wf
        if g.fold:
            val, s, t = fold_numpy(wf, a["gamma"], a["beta"], a.get("bias"))
            res["ln_s"][dr] = s
            res["ln_t"][dr] = t
        res["dst"][dr, :g.k] = val
        if g.copy == COPY_RAW:
            res["copy"] = wf.copy()
        elif g.copy == COPY_FRAG:
            full = np.full((g.n_dst, g.k), CANARY, np.uint16).view(F16)
            full[dr] = val
            res["copy"] = frag_numpy(full)
        out.append(res)
    return out


def fill_segment(seg_struct, g: Seg, addr):
    """fill one lib.LoraSeg; addr(name) -> the address of the segment's array `name`, or None"""
    s = seg_struct
    s.w0, s.dst = addr("w0"), addr("dst")
    s.rows, s.k, s.kp, s.row0 = g.rows, g.k, g.kp, g.row0
    s.map, s.n, s.copy_kind, s.reserved = g.map, len(g.adapters), g.copy, 0
    for i, (r, alpha, slot) in enumerate(g.adapters):
        s.up[i], s.down[i] = addr(f"up{i}"), addr(f"down{i}")
        s.rank[i], s.slot[i] = r, slot
        s.a[i] = float(F32(alpha / r))
    if g.fold:
        s.gamma, s.beta, s.ln_s, s.ln_t = addr("gamma"), addr("beta"), addr("ln_s"), addr("ln_t")
        s.bias = addr("bias") if g.bias else None
    s.copy = addr("copy") if g.copy != COPY_NONE else None
    return s


def bounds_ok(g: Seg, a):
    """every read and write of the segment lies inside its arrays (checked before anything runs on a GPU)"""
    dr = g.row0 + map_rows(g.map, g.rows)
    ok = a["w0"].shape == (g.rows, g.k) and a["dst"].shape == (g.n_dst, g.kp) and dr.max() < g.n_dst and dr.min() >= 0 and g.k <= g.kp
    ok = ok and len(set(dr.tolist())) == g.rows
    for i, (r, _al, _sl) in enumerate(g.adapters):
        ok = ok and a[f"up{i}"].shape == (g.rows, r) and a[f"down{i}"].shape == (r, g.k)
    if g.fold:
        ok = ok and a["gamma"].shape == (g.k,) and a["beta"].shape == (g.k,) and a["ln_s"].shape == (g.n_dst,) and a["ln_t"].shape == (g.n_dst,)
        ok = ok and (not g.bias or a["bias"].shape == (g.rows,))
    if g.copy == COPY_RAW:
        ok = ok and a["copy"].shape == (g.rows, g.k)
    if g.copy == COPY_FRAG:
        ok = ok and a["copy"].size == g.n_dst * g.k and g.k % 32 == 0 and g.n_dst % 16 == 0
    return bool(ok)


# ------------------------------------------------------------------------------------------------------------------ adapter files
def synthetic_adapter(spec, seed, rank=4, alpha=None, every=1, dtype=F16):
    """an adapter over every `every`-th kind-"w" tensor of `spec` (weights.unet_spec): {tensor name: (up [rows][r], down [r][cin(,kh,kw)],
    alpha or None)}.  A conv tensor gets a conv adapter: down [r][cin][kh][kw], up [cout][r] (stored [cout][r][1][1] by the writers)."""
    rng = np.random.default_rng(seed)
    out = {}
    names = [(n, sh) for n, sh, kind in spec if kind == "w" and n.endswith(".weight")]
    for n, sh in names[::every]:
        up = (rng.standard_normal((sh[0], rank)) * 0.05).astype(dtype)
        down = (rng.standard_normal((rank,) + tuple(sh[1:])) * 0.05).astype(dtype)
        out[n] = (up, down, alpha)
    return out


def _up_stored(up, down):
    return up.reshape(up.shape + (1, 1)) if down.ndim == 4 else up


def write_peft(adapter, new_style=True, prefix="unet."):
    """-> {key: numpy array} in the PEFT / diffusers convention (lora_A / lora_B, or the older lora.down / lora.up)"""
    out = {}
    for name, (up, down, alpha) in adapter.items():
        mod = name[:-len(".weight")]
        if new_style:
            out[f"{prefix}{mod}.lora_A.weight"], out[f"{prefix}{mod}.lora_B.weight"] = down, _up_stored(up, down)
        else:
            out[f"{prefix}{mod}.lora.down.weight"], out[f"{prefix}{mod}.lora.up.weight"] = down, _up_stored(up, down)
        if alpha is not None:
            out[f"{prefix}{mod}.alpha"] = np.asarray(alpha, dtype=F32)
    return out


def write_kohya(adapter):
    """-> {key: numpy array} in the kohya convention: lora_unet_<module with _ for .>.lora_down.weight / .lora_up.weight / .alpha"""
    out = {}
    for name, (up, down, alpha) in adapter.items():
        mod = "lora_unet_" + name[:-len(".weight")].replace(".", "_")
        out[f"{mod}.lora_down.weight"], out[f"{mod}.lora_up.weight"] = down, _up_stored(up, down)
        if alpha is not None:
            out[f"{mod}.alpha"] = np.asarray(alpha, dtype=F32)
    return out


def fused_weights(weights, adapters_and_scales):
    """the checkpoint dict with every adapted tensor replaced by the restatement's Wf (torch fp16, natural layout): what an engine built
    from scratch, or the oracle, is handed.  adapters_and_scales: [(adapter dict of synthetic_adapter, scale)], in slot order."""
    import torch

    out = dict(weights)
    touched = sorted({n for ad, _s in adapters_and_scales for n in ad})
    scales = [s for _ad, s in adapters_and_scales]
    for n in touched:
        w = weights[n].detach().cpu().to(torch.float16).numpy()
        rows = w.shape[0]
        ads = []
        for slot, (ad, _s) in enumerate(adapters_and_scales):
            if n in ad:
                up, down, alpha = ad[n]
                r = up.shape[1]
                ads.append((up.astype(F16), down.reshape(r, -1).astype(F16), F32((r if alpha is None else alpha) / r), slot))
        wf = fuse_numpy(w.reshape(rows, -1), ads, scales).reshape(w.shape)
        out[n] = torch.from_numpy(wf).to(weights[n].device)
    return out


def as_struct_array(lib_mod, case: Case, addr_of):
    """(lib.LoraSeg * nseg) filled for `case`; addr_of(segment index, array name) -> address"""
    arr = (lib_mod.LoraSeg * len(case.segs))()
    for i, g in enumerate(case.segs):
        fill_segment(arr[i], g, lambda name, i=i: addr_of(i, name))
    return arr


def np_addr(x):
    return x.ctypes.data_as(C.c_void_p).value


# ------------------------------------------------------------------------------------------------------------------ engines
def walk_tensors(obj, path="", seen=None):
    """every tensor reachable from `obj` through dataclasses, lists, tuples and dicts (and the attributes of a NetWeights): [(path, tensor)],
    each tensor once, in a fixed order.  This is how the tests find what an engine's networks hold -- not by asking the registry."""
    import dataclasses

    import torch

    seen = set() if seen is None else seen
    out = []
    if isinstance(obj, torch.Tensor):
        if id(obj) not in seen:
            seen.add(id(obj))
            out.append((path, obj))
    elif dataclasses.is_dataclass(obj) and not isinstance(obj, type):
        for f in dataclasses.fields(obj):
            out += walk_tensors(getattr(obj, f.name), f"{path}.{f.name}", seen)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            out += walk_tensors(v, f"{path}[{i}]", seen)
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            out += walk_tensors(obj[k], f"{path}[{k!r}]", seen)
    elif type(obj).__name__ == "NetWeights":
        for k in sorted(vars(obj)):
            if k not in ("places", "ops", "cfg"):  # (the registry is what is under test; its tensors are reached through the networks)
                out += walk_tensors(getattr(obj, k), f"{path}.{k}", seen)
    return out


def digest(net) -> str:
    """a digest over every weight-side buffer of a network"""
    import hashlib

    h = hashlib.sha256()
    for path, t in walk_tensors(net):
        h.update(path.encode())
        h.update(t.detach().cpu().contiguous().view(-1).view(__import__("torch").uint8).numpy().tobytes())
    return h.hexdigest()


def fold_bounds(net, weights):
    """per folded pack of `net` (built from `weights`): {id(pack): (bound on ln_s, bound on ln_t)} by destination row, the fp32 summation
    bound (K-1) * 2^-24 * sum_k |term_k| for ANY order; ln_t has one more rounding where a bias is added"""
    out = {}
    for name, pl in net.places.items():
        if pl.fold is None:
            continue
        w = weights[name].detach().cpu().to(__import__("torch").float16).numpy().astype(F32)
        beta = pl.fold[1].detach().cpu().float().numpy()
        dr = pl.row0 + map_rows(MAP_GEGLU if pl.geglu else MAP_ID, pl.rows)
        k = pl.pack.k
        wp = pl.pack.weight.detach().cpu().numpy()[dr, :k].astype(np.float64)
        bs, bt = out.setdefault(id(pl.pack), (np.zeros(pl.pack.n), np.zeros(pl.pack.n)))
        bs[dr] = (k - 1) * 2.0 ** -24 * np.abs(wp).sum(axis=1)
        tt = np.abs((w * beta[None, :]).astype(np.float64)).sum(axis=1)
        bt[dr] = (k - 1) * 2.0 ** -24 * tt + 2.0 ** -23 * (tt + (0 if pl.fold_bias is None else np.abs(pl.fold_bias.detach().cpu().float().numpy())))
    return out


def compare_networks(got, want, want_weights):
    """every tensor of the network `got` against the same-path tensor of `want` (a fresh build from `want_weights`): bytes, but for the fold
    vectors ln_s / ln_t, which two summation orders may leave up to twice the derived bound apart.  -> the number of tensors compared"""
    a, b = walk_tensors(got), walk_tensors(want)
    assert [p for p, _t in a] == [p for p, _t in b]
    bounds = fold_bounds(want, want_weights)
    packs = {}
    for pl in want.places.values():
        if pl.fold is not None:
            packs[id(pl.pack.ln_s)], packs[id(pl.pack.ln_t)] = (id(pl.pack), 0), (id(pl.pack), 1)
    for (path, x), (_p, y) in zip(a, b):
        xc, yc = x.detach().cpu(), y.detach().cpu()
        assert xc.shape == yc.shape and xc.dtype == yc.dtype, path
        if id(y) in packs:
            pid, which = packs[id(y)]
            diff = np.abs(xc.numpy().astype(np.float64) - yc.numpy().astype(np.float64))
            assert (diff <= 2 * bounds[pid][which] + 1e-30).all(), (path, float(diff.max()))
        else:
            xb, yb = xc.contiguous().view(-1).view(__import__("torch").uint8), yc.contiguous().view(-1).view(__import__("torch").uint8)
            assert bool((xb == yb).all()), (path, int((xb != yb).sum()))
    return len(a)

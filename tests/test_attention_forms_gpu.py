"""Every form of the attention kernel (csrc/attention.hip) the dispatcher can launch, against an fp64 / fp32 reference of the
same operation on the same fp16 inputs.

vsd_attention_batched picks one of 25 kernels: 8 head_dim classes <NQK, NPV> (ceil(d / 16) -> <1,1> <2,1> <3,2> <4,2> <5,3> <6,3>
<8,4> <10,5>) x 3 launch shapes (4 waves, 2 waves, 4 waves in two key-split groups merged through LDS; the key split only for
d <= 96), plus the LAZY forms of d = 40 (the running maximum subtracted inside the QK^T MFMA), and a pair kernel of each.  The
data is built so that softmax bookkeeping errors show: within one launch some query rows have their maximum in the last, ragged
key tile and move the running maximum on most tiles, others have it in tile 0; some are peaked, some split their mass between two
keys of different key-split groups, some have logits in the hundreds (positive, or all far below zero), and V carries a common
offset of 50 on every other head, so that an error in the row sum is a visible scale error.  Every row kind and head group is
checked on its own, so that a few wrong rows are not averaged away."""
import ctypes as C

import pytest
import torch

from test_ops_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = ("4,1,1", "2,1,1", "4,1,2")  # VSD_ATTN_SHAPE: waves, query blocks per wave, key-split groups
KINDS = ("ramp_up", "ramp_down", "peaked", "split", "shift_up", "shift_down", "spike")
V_OFFSET = 50.0   # added to V on the even heads
PAD = 1000.0      # finite garbage in V^T padding and batch gaps: a masked key's probability must be exactly 0
K_GAP = 3.0       # K rows between two images' keys
SENTINEL = -1234.0


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


def ru(x, m):
    return (x + m - 1) // m * m


def shapes_for(d):
    return SHAPES if d <= 96 else SHAPES[:2]


def make_problem(sq, sk, heads, d, B=1, seed=0):
    """fp16 q [B*sq, c], k [B*sk, c], v [B*sk, c] on the CPU, and the row kind (index into KINDS) of every query row.

    K dims per head: 0 a ramp over the keys (-1 .. 1), 1 spike keys (1 at three keys, the last key among them), 2 two keys of
    identical rows (from dim 2 on) in neighbouring 64-key tiles, 3 a constant 1 (a query's coefficient on it shifts all its logits),
    4.. N(0, 1).  A query row's coefficients select its kind; logits below are in natural units (after the scale d^-0.5)."""
    c, nd = heads * d, d - 4
    scale = d ** -0.5
    g = torch.Generator().manual_seed(seed)
    ntiles = (sk + 63) // 64
    k = torch.randn(B, sk, heads, d, generator=g)
    k[..., 0] = torch.linspace(-1.0, 1.0, sk)[None, :, None] if sk > 1 else 0.0
    k[..., 1] = 0.0
    k[:, sorted({sk // 3, (2 * sk) // 3, sk - 1}), :, 1] = 1.0
    k[..., 2] = 0.0
    t = max(ntiles // 2 - 1, 0)
    j1, j2 = min(64 * t + 5, sk - 1), min(64 * (t + 1) + 17, sk - 1)
    k[:, [j1, j2], :, 2] = 1.0
    k[:, j2, :, 4:] = k[:, j1, :, 4:]
    k[..., 3] = 1.0

    kinds = (torch.arange(sq)[None, :] * 3 + torch.arange(B)[:, None]) % len(KINDS)  # [B, sq]: every wave sees every kind
    noise = torch.randn(B, sq, heads, nd, generator=g)
    sigma = torch.tensor([1.0, 1.0, 6.0, 1.0, 3.0, 3.0, 1.0])[kinds]  # logit std of the N(0, 1) part
    q = torch.zeros(B, sq, heads, d)
    q[..., 4:] = noise * (sigma / (scale * nd ** 0.5))[..., None, None]
    span = 6.0 * 0.6931 * max(ntiles, 2)  # the ramp rises ~6 log2 units per tile: the running maximum (LAZY: its offset) moves
    coef = {0: (0, span / 2), 1: (0, -span / 2), 3: (2, 25.0), 4: (3, 300.0), 5: (3, -300.0), 6: (1, 200.0)}
    for kind, (dim, logit) in coef.items():
        sel = kinds == kind
        q[..., dim][sel] = logit / scale
    v = torch.randn(B, sk, heads, d, generator=g)
    v[:, :, 0::2] += V_OFFSET
    half = lambda t_, rows: t_.reshape(B * rows, c).half()  # noqa: E731
    return half(q, sq), half(k, sk), half(v, sk), kinds.reshape(-1)


def reference(q, k, v, heads, causal=False, dtype=torch.float64):
    """softmax(q k^T d^-0.5) v of one image; q [n, c] (any rows; causal: the first n rows of the image), k / v [sk, c]."""
    n, c = q.shape
    d = c // heads
    qh = q.to(dtype).view(n, heads, d).transpose(0, 1)
    kh = k.to(dtype).view(-1, heads, d).transpose(0, 1)
    vh = v.to(dtype).view(-1, heads, d).transpose(0, 1)
    s = qh @ kh.transpose(-1, -2) * d ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(n, k.shape[0], dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(0, 1).reshape(n, c)


def check_kinds(got, ref, kinds, heads, d, what, rel=3e-3):
    """check() on every (row kind, head group) block of the output: rows of one kind, even heads (V offset) / odd heads."""
    got = got.float().cpu()
    for h0, grp in ((0, "V+50"), (1, "V")):
        if h0 >= heads:
            continue
        cols = torch.cat([torch.arange(h * d, (h + 1) * d) for h in range(h0, heads, 2)])
        for i, kind in enumerate(KINDS):
            rows = (kinds == i).nonzero().flatten()
            if len(rows):
                check(got[rows][:, cols], ref[rows][:, cols], f"{what}: {kind} rows, {grp} heads", rel=4e-3 if kind == "peaked" else rel)


class Standalone:
    """The operands of one problem in their own buffers: q [B*sq, c]; K rows of image b from b*k_brows (a gap of K_GAP rows between
    images); V^T [c, ldvt] with image b's keys from column b*vt_bcols and PAD in every other column; out [B*sq + 3, ldo] (SENTINEL)."""

    def __init__(self, sq, sk, heads, d, B=1, seed=0, ldo=None):
        self.sq, self.sk, self.heads, self.d, self.B = sq, sk, heads, d, B
        self.c = c = heads * d
        self.q, self.k, self.v, self.kinds = make_problem(sq, sk, heads, d, B, seed)
        self.k_brows = sk + 5 if B > 1 else 0
        self.vt_bcols = ru(sk, 64) + 64 if B > 1 else 0
        self.ldvt = (B - 1) * self.vt_bcols + ru(sk, 64)
        kb = torch.full((max(B * self.k_brows, sk), c), K_GAP, dtype=torch.float16)
        vt = torch.full((c, self.ldvt), PAD, dtype=torch.float16)
        for b in range(B):
            kb[b * self.k_brows: b * self.k_brows + sk] = self.k[b * sk:(b + 1) * sk]
            vt[:, b * self.vt_bcols: b * self.vt_bcols + sk] = self.v[b * sk:(b + 1) * sk].t()
        self.ldo = ldo or c
        self.qd, self.kd, self.vtd = self.q.to(DEV), kb.to(DEV), vt.to(DEV)
        self.out = torch.full((B * sq + 3, self.ldo), SENTINEL, dtype=torch.float16, device=DEV)

    def run(self, ops, causal=False, out=None):
        out = self.out if out is None else out
        ops.attention(self.qd, self.c, self.kd, self.c, self.vtd, self.ldvt, out, self.ldo, self.sq, self.sk, self.heads, self.d,
                      self.d ** -0.5, causal, batch=self.B, k_brows=self.k_brows, vt_bcols=self.vt_bcols)
        return out

    def result(self, out=None):
        out = self.out if out is None else out
        return out[:self.B * self.sq, :self.c]

    def ref(self, causal=False):
        sq, sk = self.sq, self.sk
        return torch.cat([reference(self.q[b * sq:(b + 1) * sq], self.k[b * sk:(b + 1) * sk], self.v[b * sk:(b + 1) * sk], self.heads,
                                    causal) for b in range(self.B)])

    def check(self, what, causal=False, out=None):
        check_kinds(self.result(out), self.ref(causal), self.kinds, self.heads, self.d, what)


def _shape_env(monkeypatch, shape):
    if shape == "auto":
        monkeypatch.delenv("VSD_ATTN_SHAPE", raising=False)
    else:
        monkeypatch.setenv("VSD_ATTN_SHAPE", shape)


# ---- 1 + 2: the form matrix: every head_dim, every launch shape, causal for the shapes without a key split, one and two images
MATRIX = [(d, shape, causal, B) for d in range(8, 161, 8) for shape in shapes_for(d) for causal in ((False, True) if shape != "4,1,2" else (False,))
          for B in (1, 2)]


@pytest.mark.parametrize("d,shape,causal,B", MATRIX, ids=[f"d{d}-{s}-{'causal' if c else 'full'}-B{b}" for d, s, c, b in MATRIX])
def test_every_form_on_data_that_shows_softmax_errors(ops, monkeypatch, d, shape, causal, B):
    """sq 231 / 200 (ragged query blocks), sk 601 / 650 (10 / 11 key tiles, a ragged last one), three heads."""
    _shape_env(monkeypatch, shape)
    sq, sk = (231, 601) if B == 1 else (200, 650)
    p = Standalone(sq, sk, 3, d, B, seed=d + B)
    p.run(ops, causal)
    ops.synchronize()
    p.check(f"d={d} shape={shape} causal={causal} B={B}", causal)


# ---- 3: the engine's launches, natural dispatch, the engine's operand layout
def _sample_rows(sq, B, n=512, seed=0):
    """About n query rows of B images: the first and last rows, the last (partial) 128-query block of every image, random others."""
    if B * sq <= n:
        return torch.arange(B * sq)
    g = torch.Generator().manual_seed(seed)
    rows = {0, 1, B * sq - 1}
    for b in range(B):
        rows.update(range(b * sq + (sq - 1) // 128 * 128, (b + 1) * sq))
        rows.update({b * sq, b * sq + sq - 1})
    rows.update(torch.randint(0, B * sq, (max(n - len(rows), 0),), generator=g).tolist())
    return torch.tensor(sorted(rows))


def _ref_rows(q, k, v, rows, sq, sk, heads):
    out = []
    for b in range((int(rows.max()) // sq) + 1):
        r = rows[(rows >= b * sq) & (rows < (b + 1) * sq)]
        if len(r):
            out.append(reference(q[r], k[b * sk:(b + 1) * sk], v[b * sk:(b + 1) * sk], heads, dtype=torch.float32))
    return torch.cat(out)


ENGINE = [(4096, 8, 40, 1), (4096, 8, 40, 3), (4096, 8, 40, 5), (1024, 8, 80, 1), (1024, 8, 80, 3), (1024, 8, 80, 5),
          (256, 8, 160, 1), (256, 8, 160, 3), (256, 8, 160, 5), (64, 8, 160, 1), (64, 8, 160, 3), (64, 8, 160, 5),
          (9216, 8, 40, 1), (4096, 10, 64, 1), (1024, 20, 64, 1), (5184, 8, 40, 1), (5184, 8, 40, 3), (3600, 8, 40, 1),
          (3600, 8, 40, 2), (32400, 8, 40, 1)]


@pytest.mark.parametrize("hw,heads,d,B", ENGINE, ids=[f"{hw}x{h}x{d}-B{b}" for hw, h, d, b in ENGINE])
def test_engine_self_attention_layout(ops, monkeypatch, hw, heads, d, B):
    """The engine's self-attention (engine.py): q and k interleaved in one [B*hw, 2c] buffer (k = qk[:, c:]), V^T [c, B*ru(hw, 64)]
    zero-padded, one launch for B images.  SD1.5 512^2 levels at 1 / 3 / 5 images, 768^2, SDXL's 64-wide heads, 54 x 96 latents
    (ragged against the 128-query block), 45 x 80 (ragged against 64 keys) and 1920 x 1080 (32 400 tokens)."""
    monkeypatch.delenv("VSD_ATTN_SHAPE", raising=False)
    c = heads * d
    q, k, v, kinds = make_problem(hw, hw, heads, d, B, seed=hw + B)
    t_img = ru(hw, 64)
    qk = torch.empty(B * hw, 2 * c, dtype=torch.float16)
    qk[:, :c], qk[:, c:] = q, k
    vt = torch.zeros(c, B * t_img, dtype=torch.float16)
    for b in range(B):
        vt[:, b * t_img: b * t_img + hw] = v[b * hw:(b + 1) * hw].t()
    qk = qk.to(DEV)
    out = torch.full((B * hw, c), SENTINEL, dtype=torch.float16, device=DEV)
    ops.attention(qk, 2 * c, qk[:, c:], 2 * c, vt.to(DEV), B * t_img, out, c, hw, hw, heads, d, d ** -0.5, batch=B, k_brows=hw,
                  vt_bcols=t_img)
    ops.synchronize()
    rows = _sample_rows(hw, B)
    check_kinds(out[rows.to(DEV)], _ref_rows(q, k, v, rows, hw, hw, heads), kinds[rows], heads, d, f"engine {hw}x{heads}x{d} B={B}")


@pytest.mark.parametrize("sq", [4096, 1024])
def test_engine_cross_attention_over_77_text_tokens(ops, monkeypatch, sq):
    """The 77-key cross-attention of the 320- and 640-wide levels (V^T [c, 128], one ragged key tile)."""
    monkeypatch.delenv("VSD_ATTN_SHAPE", raising=False)
    heads, d = 8, 40 if sq == 4096 else 80
    p = Standalone(sq, 77, heads, d, seed=77)
    p.run(ops)
    ops.synchronize()
    p.check(f"cross-attention {sq}x77 d={d}")


@pytest.mark.parametrize("hw", [4096, 3600])
def test_engine_reference_only_read_and_write_layout(ops, monkeypatch, hw):
    """Reference-only mode (engine.py): K rows / V^T columns [0, hw) are the frame's, [hw, 2 hw) the reference's, in one
    [2 hw, 2c] buffer and one V^T of ld2 = ru(hw + ru(hw, 64), 64) columns.  The write pass attends the reference's queries over
    its own keys (V^T at column offset hw); the read pass the frame's queries over all 2 hw keys."""
    monkeypatch.delenv("VSD_ATTN_SHAPE", raising=False)
    heads, d = 8, 40
    c = heads * d
    q_r, k, v, kinds_r = make_problem(hw, 2 * hw, heads, d, seed=5)   # frame queries (read pass) over all 2 hw keys
    q_w, _, _, kinds_w = make_problem(hw, 2 * hw, heads, d, seed=6)   # reference queries (write pass)
    ld2 = ru(hw + ru(hw, 64), 64)
    qk = torch.empty(2 * hw, 2 * c, dtype=torch.float16)
    qk[:hw, :c], qk[hw:, :c], qk[:, c:] = q_r, q_w, k
    vt = torch.zeros(c, ld2, dtype=torch.float16)
    vt[:, :2 * hw] = v.t()
    qk, vt = qk.to(DEV), vt.to(DEV)
    att_w = torch.full((hw, c), SENTINEL, dtype=torch.float16, device=DEV)
    att_r = torch.full((hw, c), SENTINEL, dtype=torch.float16, device=DEV)
    ops.attention(qk[hw:], 2 * c, qk[hw:, c:], 2 * c, vt[:, hw:], ld2, att_w, c, hw, hw, heads, d, d ** -0.5)
    ops.attention(qk[:hw], 2 * c, qk[:, c:], 2 * c, vt, ld2, att_r, c, hw, 2 * hw, heads, d, d ** -0.5)
    ops.synchronize()
    rows = _sample_rows(hw, 1)
    check_kinds(att_w[rows.to(DEV)], reference(q_w[rows], k[hw:], v[hw:], heads, dtype=torch.float32), kinds_w[rows], heads, d,
                f"reference-only write pass hw={hw}")
    check_kinds(att_r[rows.to(DEV)], reference(q_r[rows], k, v, heads, dtype=torch.float32), kinds_r[rows], heads, d,
                f"reference-only read pass hw={hw}")


# ---- 4: pairs (vsd_pair_begin / join / end): two problems of one grid as one launch
def _joined(ops, run_a, run_b):
    ops.ctx.call("vsd_pair_begin")
    run_a()
    ops.ctx.call("vsd_pair_join")
    ops._widx = 1
    try:
        run_b()
    finally:
        ops._widx = None
    n = C.c_int(-1)
    ops.ctx.call("vsd_pair_end", C.byref(n))
    return n.value


def _pair_case(ops, a, b):
    alone = [p.run(ops, out=p.out.clone()) for p in (a, b)]
    n = _joined(ops, lambda: a.run(ops), lambda: b.run(ops))
    ops.synchronize()
    assert n == 1, f"{n} launches joined"
    for p, o in zip((a, b), alone):
        assert torch.equal(p.out, o), "the paired launch differs from the call alone"
    assert not torch.equal(a.result(), b.result())
    b.check("second problem of the pair")


PAIRS = [(d, shape) for d in (8, 32, 40, 48, 64, 80, 96, 128, 160) for shape in shapes_for(d)]


@pytest.mark.parametrize("d,shape", PAIRS, ids=[f"d{d}-{s}" for d, s in PAIRS])
def test_pair_form_equals_the_calls_alone(ops, monkeypatch, d, shape):
    """One representative head_dim per class (d = 40: LAZY, d = 48: the plain <3,2> form); two problems of one grid but
    different data and key counts."""
    _shape_env(monkeypatch, shape)
    _pair_case(ops, Standalone(231, 601, 3, d, seed=d), Standalone(231, 587, 3, d, seed=d + 1))


@pytest.mark.parametrize("B", [1, 2])
def test_lazy_pair_at_the_headline_shape(ops, monkeypatch, B):
    """4096 x 4096 keys, 8 heads of 40, natural dispatch: the key split at one image, attention_lazy_pair_kernel at two."""
    monkeypatch.delenv("VSD_ATTN_SHAPE", raising=False)
    a, b = Standalone(4096, 4096, 8, 40, B, seed=40), Standalone(4096, 4096, 8, 40, B, seed=41)
    alone = [p.run(ops, out=p.out.clone()) for p in (a, b)]
    assert _joined(ops, lambda: a.run(ops), lambda: b.run(ops)) == 1
    ops.synchronize()
    assert torch.equal(a.out, alone[0]) and torch.equal(b.out, alone[1]) and not torch.equal(a.out, b.out)
    rows = _sample_rows(4096, B)
    check_kinds(b.result()[rows.to(DEV)], _ref_rows(b.q, b.k, b.v, rows, 4096, 4096, 8), b.kinds[rows], 8, 40,
                f"second problem of the LAZY pair B={B}")


# ---- 5: edges and bookkeeping
EDGE_D = (40, 64, 80)


@pytest.mark.parametrize("shape", ("auto",) + SHAPES)
@pytest.mark.parametrize("d", EDGE_D)
@pytest.mark.parametrize("sq", [1, 63, 65, 127, 129])
def test_query_counts_at_the_edges_of_a_query_block(ops, monkeypatch, sq, d, shape):
    """One query, and one row short of / past a workgroup's 64 (two waves) or 128 (four waves) queries."""
    _shape_env(monkeypatch, shape)
    p = Standalone(sq, 601, 3, d, seed=sq)
    p.run(ops)
    ops.synchronize()
    p.check(f"sq={sq} d={d} shape={shape}")


@pytest.mark.parametrize("shape", ("auto",) + SHAPES)
@pytest.mark.parametrize("d", EDGE_D)
@pytest.mark.parametrize("sk", [1, 63, 64, 65, 448, 512])
def test_key_counts_at_the_edges_of_a_key_tile(ops, monkeypatch, sk, d, shape):
    """One key, one short of / exactly / one past a 64-key tile, 7 and exactly 8 tiles (the dispatcher's key-split threshold)."""
    _shape_env(monkeypatch, shape)
    p = Standalone(200, sk, 3, d, seed=sk)
    p.run(ops)
    ops.synchronize()
    p.check(f"sk={sk} d={d} shape={shape}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("d", [40, 48, 64, 160])
def test_output_stride_and_rows_past_the_problem_keep_the_sentinel(ops, monkeypatch, d, shape):
    """ldo > c: every column outside [0, c) and every row past B*sq keeps what was there; two identical calls give the same bits."""
    _shape_env(monkeypatch, shape)
    p = Standalone(137, 601, 3, d, B=2, seed=d, ldo=3 * d + 24)
    first = p.run(ops, out=p.out.clone())
    p.run(ops)
    ops.synchronize()
    p.check(f"ldo={p.ldo} d={d} shape={shape}")
    sentinel = torch.full_like(p.out, SENTINEL)
    outside = torch.ones_like(p.out, dtype=torch.bool)
    outside[:p.B * p.sq, :p.c] = False
    assert torch.equal(p.out[outside], sentinel[outside]), "a write outside [0, B*sq) x [0, c)"
    assert torch.equal(first, p.out), "two identical calls differ"


# ---- 6: the LAZY key split when one group gets no key tile
@pytest.mark.parametrize("sk", [1, 40, 64])
def test_lazy_key_split_with_a_single_key_tile(ops, monkeypatch, sk):
    """VSD_ATTN_SHAPE=4,1,2 at d = 40 with one key tile: key-split group 1 sees no tile.  The shift_down rows have every logit near
    -300 (natural units), so group 0's running maximum is far below zero; group 1 must not take part in the merge."""
    _shape_env(monkeypatch, "4,1,2")
    p = Standalone(200, sk, 3, 40, seed=sk)
    low = p.q[p.kinds == KINDS.index("shift_down")].float().view(-1, 3, 40).transpose(0, 1)
    assert float((low @ p.k.float().view(sk, 3, 40).permute(1, 2, 0)).max()) * 40 ** -0.5 < -200  # (every logit of those rows)
    p.run(ops)
    ops.synchronize()
    p.check(f"LAZY key split, sk={sk}")

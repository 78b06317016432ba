"""Checks of the ABI 12 kernels (csrc/causal.hip: MTX_OP_CAUSAL_ATTN, MTX_OP_GREEDY; MTX_EW_QK_ROPE at any head width), written once and run on
the simulator (tests/test_paddle_ocr_vl_sim.py) and on the product library (tests/test_paddle_ocr_vl_gpu.py).

Causal attention, exact selection: scores are built as sums of exact integer products so that, for query row i, ONE key scores 0, every other
visible key at most -120 and the first key of the future +8.  exp(-120) underflows to exactly 0 in fp32, so the output must be the chosen V row
bit for bit; a future key that is not masked would win instead.  The score matrix is
    M[i][j] = 128 (j - (pos + i))  -  120 [j != w]  +  128 (pos + i - w) [j == w]            (w = the fixed winner, 0 or pos)
    M[i][j] = 128 (j - (pos + i))                                                              (winner = the row's own key)
a sum of rank-one terms, each a (function of i) x (function of j) held in a few head dimensions with numbers split in base 16 so that every
entry is exact in bf16 and f16.
Causal attention, random: against fp32 torch (explicit causal mask, repeat_interleave of the kv heads) on the same 16-bit inputs, with the
bound of manga_ocr_checks.check_decode_attn_random: half a spacing of T at the reference (the one rounding) plus the fp32 softmax's own error
over at most 300 keys, 300 * 2^-23 of the largest value (the largest case here has 133 + 131 = 264 keys).
Head layouts: HEADS gives one chunk of G = 1, 2 or 8 query heads per kv head; STEP_LAYOUTS adds G = 4 and several chunks per kv head for every
G (`step_layout` restates the launcher's rule), and `check_causal_selection_per_head` gives every query head a winner of its own, so that a
result which lands at another head of its group is a wrong V row."""
import ctypes as C

import pytest
import torch

from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _sync

MANT = {abi.BF16: 7, abi.F16: 10}
D = 128
TQ, TK, S = abi.CAUSAL_TQ, abi.CAUSAL_TK, abi.CAUSAL_S
ROWS = [1, 2, TQ - 1, TQ, TQ + 1, 2 * TQ + 3]
POSITIONS = [0, 1, TK - 1, TK, TK + 1, 2 * S + 5]
HEADS = [(2, 2), (4, 2), (16, 2)]
# head layouts of the step kernels that HEADS (G = 1, 2, 8 with one chunk of query heads per kv head) does not reach; see `step_layout`
STEP_LAYOUTS = [(8, 2), (24, 2), (32, 2), (6, 2), (12, 2), (12, 3)]
GUARD = 4                             # cache rows behind max_len that nobody may touch
NAN_BITS = 0x7FC1                     # a NaN bit pattern of both 16-bit types
MTX_ERR_UNSUPPORTED = -3                 # include/mtx_hip.h


def _bits(t):
    return t.contiguous().view(torch.int16)


class CausalRig:
    """one recorded MTX_OP_CAUSAL_ATTN over caches with a guard band; `run` launches it"""

    def __init__(self, lib, dtype, rows, heads, kv_heads, max_len, d=D, scale=None, pad_qkv=0, pad_o=0):
        self.lib, self.dev, self.td = lib, _dev(lib), TD[dtype]
        self.rows, self.heads, self.kv, self.max_len = rows, heads, kv_heads, max_len
        self.w = (heads + 2 * kv_heads) * D
        self.ld_qkv, self.ld_o = self.w + pad_qkv, heads * D + pad_o          # row strides; the padding columns belong to the test
        pb = PlanBuilder(lib, self.dev, dtype)
        self.qkv = pb.buf((rows, self.ld_qkv), self.td, zero=True)
        self.kc = pb.buf((max_len + GUARD, kv_heads * D), self.td, zero=True)
        self.vc = pb.buf((max_len + GUARD, kv_heads * D), self.td, zero=True)
        self.pos = pb.buf((1,), torch.int32, zero=True)
        self.o = pb.buf((rows, self.ld_o), self.td, zero=True)
        self.scale = D ** -0.5 if scale is None else scale
        pb.causal_attention(self.qkv, self.kc, self.vc, self.pos, self.o, rows, heads, kv_heads, d, max_len, self.scale,
                            ld_qkv=self.ld_qkv, ld_o=self.ld_o)
        self.pb, self.plan = pb, None

    def run(self, qkv=None, kc=None, vc=None, pos=None):
        if qkv is not None:
            self.qkv.copy_(qkv)
        if kc is not None:
            self.kc.copy_(kc)
        if vc is not None:
            self.vc.copy_(vc)
        if pos is not None:
            self.pos.fill_(pos)
        if self.plan is None:
            self.plan = self.pb.build()
        self.plan.run()
        _sync(self.lib)
        return self.o.cpu()


def causal_ref(qkv, kc, vc, pos, heads, kv, scale):
    """fp32 scores and softmax, float64 weighted sum, on the same 16-bit inputs: [rows, heads * D] float64"""
    rows = qkv.shape[0]
    q = qkv[:, :heads * D].float().view(rows, heads, D)
    K = torch.cat([kc[:pos].float().view(pos, kv, D), qkv[:, heads * D:(heads + kv) * D].float().view(rows, kv, D)], 0)
    V = torch.cat([vc[:pos].double().view(pos, kv, D), qkv[:, (heads + kv) * D:].double().view(rows, kv, D)], 0)
    K, V = K.repeat_interleave(heads // kv, 1), V.repeat_interleave(heads // kv, 1)
    s = torch.einsum("ihd,jhd->hij", q, K) * scale
    mask = torch.arange(pos + rows)[None, :] > (pos + torch.arange(rows))[:, None]
    s = s.masked_fill(mask[None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hij,jhd->ihd", p.double(), V).reshape(rows, heads * D)


def _poisoned_caches(rig, pos, g):
    """random caches; everything from `pos` on (this launch's own positions, the free tail, the guard band) is NaN"""
    n = rig.max_len + GUARD
    kc = torch.randn(n, rig.kv * D, generator=g).to(rig.td)
    vc = torch.randn(n, rig.kv * D, generator=g).to(rig.td)
    for c in (kc, vc):
        c.view(torch.int16)[pos:] = NAN_BITS
    return kc, vc


def _check_caches(rig, kc, vc, qkv, pos, what):
    """only cache[pos .. pos + rows) has changed, and it holds the rows' k | v"""
    h, kv, rows = rig.heads, rig.kv, rig.rows
    want_k, want_v = kc.clone(), vc.clone()
    want_k[pos:pos + rows] = qkv[:, h * D:(h + kv) * D]
    want_v[pos:pos + rows] = qkv[:, (h + kv) * D:]
    assert torch.equal(_bits(rig.kc.cpu()), _bits(want_k)) and torch.equal(_bits(rig.vc.cpu()), _bits(want_v)), \
        f"{what}: the caches changed elsewhere than at [pos, pos + rows), or hold other values there"


def check_causal_random(lib, dtype, rows, pos, heads, kv, seed=0):
    """returns the largest error relative to its bound; also the cache discipline of the launch"""
    max_len = pos + rows + 3
    g = torch.Generator().manual_seed(seed * 1000 + rows * 31 + pos * 7 + heads)
    rig = CausalRig(lib, dtype, rows, heads, kv, max_len)
    kc, vc = _poisoned_caches(rig, pos, g)
    qkv = (torch.randn(rows, rig.w, generator=g) * 1.5).to(rig.td)
    got = rig.run(qkv, kc, vc, pos).double()
    what = f"causal attention rows={rows} pos={pos} heads={heads}/{kv}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (a cache entry at or beyond pos was read)"
    ref = causal_ref(qkv, kc, vc, pos, heads, kv, rig.scale)
    vmax = float(qkv[:, (heads + kv) * D:].double().abs().max().clamp_min(vc[:pos].double().abs().max() if pos else 0.0))
    bound = ref.abs() * 2.0 ** -(MANT[dtype] + 1) * (1 + 2.0 ** -6) + 300 * 2.0 ** -23 * vmax
    ratio = float(((got - ref).abs() / bound).max())
    assert ratio <= 1.0, f"{what}: error {ratio:.2f} x the bound (one rounding + fp32 softmax)"
    _check_caches(rig, kc, vc, qkv, pos, what)
    return ratio


def _b16(n):
    """n (tensor of non-negative integers) as (16 * (n // 16), n % 16): both exact in bf16 up to n < 4096"""
    return (n // 16 * 16).double(), (n % 16).double()


def check_causal_selection(lib, dtype, rows, pos, heads, kv, winner, seed=0):
    """winner: "own" (j = pos + i), "pos" (j = pos) or "zero" (j = 0).  scale = 1; see the module docstring for the score matrix"""
    max_len = pos + rows + 2
    n = max_len + GUARD
    g = torch.Generator().manual_seed(seed + rows * 31 + pos * 7 + heads)
    rig = CausalRig(lib, dtype, rows, heads, kv, max_len, scale=1.0)
    td = rig.td
    j = torch.arange(n)
    i_abs = pos + torch.arange(rows)
    w = None if winner == "own" else (pos if winner == "pos" else 0)
    # key features (same for every kv head)
    phi = torch.zeros(n, D, dtype=torch.float64)
    phi[:, 0], phi[:, 1] = (j // 16).double(), (j % 16).double()
    phi[:, 2] = 1.0
    phi[:, 3] = 1.0
    if w is not None:
        phi[:, 4] = (j != w).double()
        phi[:, 5] = (j == w).double()
        phi[:, 6] = (j == w).double()
    # query features (same for every head)
    psi = torch.zeros(rows, D, dtype=torch.float64)
    hi, lo = _b16(i_abs)
    psi[:, 0], psi[:, 1], psi[:, 2], psi[:, 3] = 128.0 * 16, 128.0, -128.0 * hi, -128.0 * lo
    if w is not None:
        hi, lo = _b16(i_abs - w)
        psi[:, 4], psi[:, 5], psi[:, 6] = -120.0, 128.0 * hi, 128.0 * lo
    M = psi @ phi.t()
    for t in (phi, psi):
        assert torch.equal(t, t.to(td).double()), "the test's own premise: every feature is exact in the storage type"
    win = i_abs if w is None else torch.full((rows,), w)
    for i in range(rows):
        vis = M[i, :pos + i + 1]
        assert vis[win[i]] == 0 and int((vis > -120).sum()) == 1 and M[i, pos + i + 1] == (128.0 if w is None else 8.0)
    keys = phi.to(td)[:, None, :].expand(n, kv, D).reshape(n, kv * D)
    vals = torch.randn(n, kv * D, generator=g).to(td)
    qkv = torch.cat([psi.to(td)[:, None, :].expand(rows, heads, D).reshape(rows, heads * D), keys[pos:pos + rows], vals[pos:pos + rows]], 1)
    kc, vc = keys.clone(), vals.clone()
    for c in (kc, vc):
        cb = c.view(torch.int16)
        cb[pos:pos + rows] = NAN_BITS                # the launch's own positions are read from its rows, not from the cache
        cb[pos + rows + 1:] = NAN_BITS               # cache[pos + rows] keeps the key of the future that would outscore the winner
    got = rig.run(qkv, kc, vc, pos)
    want = vals[win].view(rows, kv, D).repeat_interleave(heads // kv, 1).reshape(rows, heads * D)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, (f"causal attention rows={rows} pos={pos} heads={heads}/{kv} winner={winner}: {bad} of {want.numel()} elements differ "
                      f"from the chosen V row")
    _check_caches(rig, kc, vc, qkv, pos, f"causal attention (selection) rows={rows} pos={pos}")


def check_causal_full_cache_is_a_no_op(lib, dtype, rows, heads, kv):
    """pos = max_len - rows + 1: the rows do not fit, nothing at all changes (caches, guard band, o)"""
    max_len = rows + 40
    g = torch.Generator().manual_seed(rows)
    rig = CausalRig(lib, dtype, rows, heads, kv, max_len)
    kc = torch.randn(max_len + GUARD, kv * D, generator=g).to(rig.td)
    vc = torch.randn(max_len + GUARD, kv * D, generator=g).to(rig.td)
    qkv = torch.randn(rows, rig.w, generator=g).to(rig.td)
    sentinel = torch.full((rows, heads * D), 7.0).to(rig.td)
    for pos in (max_len - rows + 1, -1):
        rig.o.copy_(sentinel)
        got = rig.run(qkv, kc, vc, pos)
        assert torch.equal(_bits(got), _bits(sentinel)), f"pos={pos}: o was written"
        assert torch.equal(_bits(rig.kc.cpu()), _bits(kc)) and torch.equal(_bits(rig.vc.cpu()), _bits(vc)), f"pos={pos}: a cache was written"
    # and the last position that fits still works
    pos = max_len - rows
    rig.run(qkv, kc, vc, pos)
    _check_caches(rig, kc, vc, qkv, pos, f"causal attention rows={rows} at the end of the cache")


def check_prefill_equals_steps(lib, dtype, T, pos0, heads, kv, seed=0):
    """T rows in one launch against T launches of one row over the growing cache: within one unit in the last place of the storage type.
    (Not bit-equal: the prefill kernel sums keys in 32-key tiles on the matrix pipe with the softmax weights as two 16-bit halves, the step
    kernel sums 16 interleaved key streams in fp32 and merges 64-key splits; both round once, from fp32 values that differ in their last
    bits, and a tie broken the other way moves the result by one step.)  The values are positive (0.25 + |N(0, 1)|): an output is then of the
    size of its terms and a unit in its last place stands far above the fp32 sums' own error.  With signed values outputs cancel down to 1e-4
    and below, where a step of bf16 is 2^-20 and one of f16 (subnormal) 2^-24 — the size of the fp32 error itself, 2^-23 of the largest value
    per key, so two correct fp32 kernels differ there by 2 steps (measured on the simulator: 3 of 50 688 elements in bf16, 7 in f16); the
    signed case is held to the reference in check_causal_random.  Returns the number of elements that differ."""
    max_len = pos0 + T
    g = torch.Generator().manual_seed(seed + T)
    pre = CausalRig(lib, dtype, T, heads, kv, max_len)
    step = CausalRig(lib, dtype, 1, heads, kv, max_len)
    kc, vc = _poisoned_caches(pre, pos0, g)
    vc[:pos0] = (vc[:pos0].float().abs() + 0.25).to(pre.td)
    qkv = (torch.randn(T, pre.w, generator=g) * 1.5).to(pre.td)
    qkv[:, (heads + kv) * D:] = (qkv[:, (heads + kv) * D:].float().abs() + 0.25).to(pre.td)
    o_pre = pre.run(qkv, kc, vc, pos0)
    step.kc.copy_(kc); step.vc.copy_(vc)
    rows = []
    for i in range(T):
        rows.append(step.run(qkv[i:i + 1], pos=pos0 + i).clone())
    o_step = torch.cat(rows, 0)
    assert torch.equal(_bits(step.kc.cpu()), _bits(pre.kc.cpu())) and torch.equal(_bits(step.vc.cpu()), _bits(pre.vc.cpu())), "the two caches differ"
    a, b = o_pre.double(), o_step.double()
    ulp = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -14).log2().floor().exp2() * 2.0 ** -MANT[dtype]
    worst = float(((a - b).abs() / ulp).max())
    assert worst <= 1.0, f"prefill vs {T} steps: {worst} ulp"
    return int((a != b).sum())


def check_step_is_deterministic(lib, dtype, pos, heads, kv, repeats=5):
    """identical calls give identical bytes (the split merge has a fixed order whoever draws the last ticket)"""
    g = torch.Generator().manual_seed(pos)
    rig = CausalRig(lib, dtype, 1, heads, kv, pos + 1)
    kc, vc = _poisoned_caches(rig, pos, g)
    qkv = (torch.randn(1, rig.w, generator=g) * 1.5).to(rig.td)
    first = _bits(rig.run(qkv, kc, vc, pos)).clone()
    for _ in range(repeats):
        assert torch.equal(_bits(rig.run()), first)


def check_gqa_mapping(lib, dtype, rows, heads=4, kv=2):
    """value head v holds the constant v + 1: query head h returns (h // (heads / kv)) + 1 — at (4, 2) query heads 0, 1 read kv head 0 and
    heads 2, 3 read kv head 1"""
    pos = 5
    g = torch.Generator().manual_seed(rows)
    rig = CausalRig(lib, dtype, rows, heads, kv, pos + rows)
    kc = torch.randn(pos + rows + GUARD, kv * D, generator=g).to(rig.td)
    vc = torch.cat([torch.full((pos + rows + GUARD, D), v + 1.0) for v in range(kv)], 1).to(rig.td)
    qkv = torch.randn(rows, rig.w, generator=g).to(rig.td)
    qkv[:, (heads + kv) * D:] = vc[:rows]
    got = rig.run(qkv, kc, vc, pos).float().view(rows, heads, D)
    want = (torch.arange(heads) // (heads // kv) + 1.0)[None, :, None].expand(rows, heads, D)
    if (heads, kv) == (4, 2):
        assert torch.equal(want[0, :, 0], torch.tensor([1.0, 1.0, 2.0, 2.0]))
    assert torch.equal(got, want), f"GQA mapping heads={heads}/{kv}: head means {got.mean((0, 2)).tolist()}"


# ---- head layouts of the step kernels ----------------------------------------------------------------------------------------------------------
def step_layout(heads, kv):
    """causal_attn_launch's rule restated: (G, nz) = (query heads that share one pass over the keys, chunks of G heads per kv head).  The
    step runs causal_step_kernel<T, G> on a grid (splits, kv, nz); the batched step causal_step_batch_kernel<T, G> on (splits, kv, slots * nz)"""
    assert heads % kv == 0
    gfull = heads // kv
    G = 8 if gfull % 8 == 0 else (4 if gfull % 4 == 0 else (2 if gfull % 2 == 0 else 1))
    return G, gfull // G


# the instantiation every layout-parametrised case is meant for: causal_step_kernel<T, G> / causal_step_batch_kernel<T, G> with nz chunks per kv head
LAYOUT_OF = {(8, 2): (4, 1), (24, 2): (4, 3), (32, 2): (8, 2), (6, 2): (1, 3), (12, 2): (2, 3), (12, 3): (4, 1), (16, 2): (8, 1)}
assert [LAYOUT_OF[hk] for hk in STEP_LAYOUTS] == [(4, 1), (4, 3), (8, 2), (1, 3), (2, 3), (4, 1)]


def assert_layout(heads, kv):
    """the case runs the (G, nz) it is meant for; -> (G, nz)"""
    assert step_layout(heads, kv) == LAYOUT_OF[(heads, kv)], f"heads {heads}/{kv} runs (G, nz) = {step_layout(heads, kv)}, the case is meant for {LAYOUT_OF[(heads, kv)]}"
    return LAYOUT_OF[(heads, kv)]


assert all(step_layout(h, k)[1] == 1 and step_layout(h, k)[0] != 4 for h, k in HEADS), "what HEADS leaves open"
assert all(any(step_layout(h, k) == (G, nz) and nz > 1 for h, k in STEP_LAYOUTS for nz in (2, 3)) for G in (1, 2, 4, 8)), \
    "every G needs a layout with more than one chunk of query heads per kv head"
assert any(k > 2 for _, k in STEP_LAYOUTS)
STEP_POSITIONS = [0, TK + 1, 2 * S + 5]
VARIANTS = ("own", "pos", "zero")


def per_head_selection(td, n, pos, rows, heads):
    """check_causal_selection's construction with a winner PER QUERY HEAD: head h plays VARIANTS[h % 3].  The key features of the two fixed
    winners lie side by side (columns 4-6 for w = pos, 7-9 for w = 0) and a head holds zeros in the columns of the variant it does not play, so
    the keys are the same for every kv head while the heads of one group expect different rows.
    -> (phi [n, D], psi [rows, heads, D], win [rows, heads]), float64 / int64; asserts the premise per head from its own score matrix"""
    j = torch.arange(n)
    i_abs = pos + torch.arange(rows)
    phi = torch.zeros(n, D, dtype=torch.float64)
    phi[:, 0], phi[:, 1] = (j // 16).double(), (j % 16).double()
    phi[:, 2] = 1.0
    phi[:, 3] = 1.0
    for c, w in ((4, pos), (7, 0)):
        phi[:, c] = (j != w).double()
        phi[:, c + 1] = (j == w).double()
        phi[:, c + 2] = (j == w).double()
    psi = torch.zeros(rows, heads, D, dtype=torch.float64)
    hi, lo = _b16(i_abs)
    psi[:, :, 0], psi[:, :, 1] = 128.0 * 16, 128.0
    psi[:, :, 2], psi[:, :, 3] = (-128.0 * hi)[:, None], (-128.0 * lo)[:, None]
    win = torch.zeros(rows, heads, dtype=torch.long)
    for h in range(heads):
        variant = VARIANTS[h % 3]
        if variant == "own":
            win[:, h] = i_abs
            continue
        c, w = (4, pos) if variant == "pos" else (7, 0)
        hi, lo = _b16(i_abs - w)
        psi[:, h, c], psi[:, h, c + 1], psi[:, h, c + 2] = -120.0, 128.0 * hi, 128.0 * lo
        win[:, h] = w
    for t in (phi, psi):
        assert torch.equal(t, t.to(td).double()), "the test's own premise: every feature is exact in the storage type"
    for h in range(heads):
        M = psi[:, h] @ phi.t()
        for i in range(rows):
            vis = M[i, :pos + i + 1]
            assert vis[win[i, h]] == 0 and int((vis > -120).sum()) == 1 and M[i, pos + i + 1] == (128.0 if h % 3 == 0 else 8.0)
    if pos > 0 and heads >= 3:                       # (in the first row "own" and "pos" name the same key; "zero" never does)
        assert win[0, 1] != win[0, 2] and win[-1, 0] != win[-1, 2], "neighbouring heads must expect different rows"
    return phi, psi, win


def check_causal_selection_per_head(lib, dtype, rows, pos, heads, kv, seed=0):
    """query head h must return, bit for bit, row win_h(i) of the values of kv head h // (heads / kv): with a different winner per head, a
    result that lands at another head of its group (m[g], l[g], acc[g], part[wave][g], the record of head h0 + g) is a wrong V row"""
    max_len = pos + rows + 2
    n = max_len + GUARD
    g = torch.Generator().manual_seed(seed + rows * 31 + pos * 7 + heads)
    rig = CausalRig(lib, dtype, rows, heads, kv, max_len, scale=1.0)
    td = rig.td
    phi, psi, win = per_head_selection(td, n, pos, rows, heads)
    keys = phi.to(td)[:, None, :].expand(n, kv, D).reshape(n, kv * D)
    vals = torch.randn(n, kv * D, generator=g).to(td)
    qkv = torch.cat([psi.to(td).reshape(rows, heads * D), keys[pos:pos + rows], vals[pos:pos + rows]], 1)
    kc, vc = keys.clone(), vals.clone()
    for c in (kc, vc):
        cb = c.view(torch.int16)
        cb[pos:pos + rows] = NAN_BITS                # the launch's own positions are read from its rows, not from the cache
        cb[pos + rows + 1:] = NAN_BITS               # cache[pos + rows] keeps the key of the future that would outscore the winner
    got = rig.run(qkv, kc, vc, pos)
    kvh = torch.arange(heads) // (heads // kv)
    want = vals.view(n, kv, D)[win, kvh[None, :].expand(rows, heads)].reshape(rows, heads * D)
    if pos > 0 and heads // kv >= 3:
        assert not torch.equal(_bits(want.view(rows, heads, D)[:, 1]), _bits(want.view(rows, heads, D)[:, 2])), "heads 1 and 2 share a kv head and must expect different rows"
    wrong = (_bits(got) != _bits(want)).view(rows, heads, D).any(-1).any(0).nonzero().flatten().tolist()
    assert not wrong, (f"causal attention rows={rows} pos={pos} heads={heads}/{kv} (G, nz) = {step_layout(heads, kv)}: query heads {wrong} differ "
                       f"from their own chosen V row")
    _check_caches(rig, kc, vc, qkv, pos, f"causal attention (selection per head) rows={rows} pos={pos}")


def check_causal_padded_strides(lib, dtype, rows, heads=24, kv=2, pos=TK + 1, seed=0):
    """ld_qkv = w + 24 and ld_o = heads * D + 8 (both multiples of 8, as the launcher asks): the bytes of the unpadded case, NaN patterns in
    the padding of qkv are not read, the padding of o keeps its sentinel"""
    assert_layout(heads, kv)                       # (24, 2): G = 4 in three chunks per kv head for the step, h / G in the prefill
    max_len = pos + rows + 3
    g = torch.Generator().manual_seed(seed + rows)
    plain = CausalRig(lib, dtype, rows, heads, kv, max_len)
    wide = CausalRig(lib, dtype, rows, heads, kv, max_len, pad_qkv=24, pad_o=8)
    assert (wide.ld_qkv, wide.ld_o) == (plain.w + 24, heads * D + 8) and wide.ld_qkv % 8 == 0 and wide.ld_o % 8 == 0
    kc, vc = _poisoned_caches(plain, pos, g)
    qkv = (torch.randn(rows, plain.w, generator=g) * 1.5).to(plain.td)
    want = plain.run(qkv, kc, vc, pos)
    assert bool(torch.isfinite(want.float()).all())
    padded = torch.full((rows, wide.ld_qkv), NAN_BITS, dtype=torch.int16).view(plain.td)
    padded[:, :plain.w] = qkv
    sentinel = torch.full((rows, wide.ld_o), 7.0).to(plain.td)
    wide.o.copy_(sentinel)
    got = wide.run(padded, kc, vc, pos)
    what = f"causal attention with padded strides rows={rows} heads={heads}/{kv}"
    assert torch.equal(_bits(got[:, :heads * D]), _bits(want)), f"{what}: differs from the unpadded case"
    assert torch.equal(_bits(got[:, heads * D:]), _bits(sentinel[:, heads * D:])), f"{what}: the padding of o was written"
    assert torch.equal(_bits(wide.kc.cpu()), _bits(plain.kc.cpu())) and torch.equal(_bits(wide.vc.cpu()), _bits(plain.vc.cpu())), f"{what}: the caches differ"


def check_causal_refusals(lib):
    for d, heads, kv in ((64, 4, 2), (128, 3, 2)):
        rig = CausalRig(lib, abi.BF16, 1, heads, kv, 8, d=d)
        args = rig.pb.ops[-1].u.cattn
        rc = lib.mtx_causal_attention(C.byref(args), C.c_void_p(0))
        assert rc == MTX_ERR_UNSUPPORTED, f"d={d} heads={heads}/{kv}: rc {rc}"
        with pytest.raises(ModelError):
            rig.run()


# ---- greedy pick -------------------------------------------------------------------------------------------------------------------------
VOCABS = [1, 255, 256, 257, 103424]


def _greedy(lib, logits, state, max_new, eos, advance, out=None):
    """one launch -> (state, out) on the host"""
    dev = _dev(lib)
    pb = PlanBuilder(lib, dev, abi.F16)
    lg = pb.const(logits.float())
    st = pb.const(torch.tensor(state, dtype=torch.int32))
    ot = pb.const(torch.full((max_new,), -7, dtype=torch.int32) if out is None else out.to(torch.int32))
    pb.greedy_pick(lg, st, ot, logits.numel(), max_new, eos=eos, advance=advance)
    pb.build().run()
    _sync(lib)
    return st.cpu().tolist(), ot.cpu().tolist()


def check_greedy_argmax(lib, vocab, seed=0):
    """the maximum at the first index, the last index, both sides of every chunk boundary; two equal maxima give the lower index; a NaN
    beside the maximum loses; -inf everywhere gives index 0"""
    g = torch.Generator().manual_seed(seed + vocab)
    base = torch.randn(vocab, generator=g)
    spots = sorted({0, vocab - 1, vocab // 2} | {b + o for b in range(abi.GREEDY_CHUNK, vocab, abi.GREEDY_CHUNK) for o in (-1, 0)} | {min(255, vocab - 1), min(256, vocab - 1)})
    if vocab > 50000:
        spots = spots[:6] + spots[-6:]
    for s in spots:
        lg = base.clone()
        lg[s] = 9.0
        st, out = _greedy(lib, lg, [10, 0, 0, -1], 4, [], 1)
        assert st == [11, 1, 0, s] and out[0] == s, f"vocab {vocab}: maximum at {s}, state {st}"
        if s + 1 < vocab:                            # an equal maximum further on (next index, and the last one) does not win
            for t in {s + 1, vocab - 1}:
                lg2 = lg.clone(); lg2[t] = 9.0
                st, _ = _greedy(lib, lg2, [0, 0, 0, -1], 4, [], 1)
                assert st[3] == s, f"vocab {vocab}: equal maxima at {s} and {t} gave {st[3]}"
        if vocab > 1:                                # a NaN beside it (before and after) loses
            for t in {(s + 1) % vocab, (s - 1) % vocab, 0 if s else vocab - 1}:
                lg2 = lg.clone(); lg2[t] = float("nan")
                st, _ = _greedy(lib, lg2, [0, 0, 0, -1], 4, [], 1)
                assert st[3] == s, f"vocab {vocab}: NaN at {t} beside the maximum at {s} gave {st[3]}"
    st, _ = _greedy(lib, torch.full((vocab,), float("-inf")), [0, 0, 0, -1], 4, [], 1)
    assert st[3] == 0


def check_greedy_state(lib):
    vocab = 300
    lg = torch.zeros(vocab); lg[41] = 1.0
    # plain step: out[n_out++] = t, token = t, pos += advance
    st, out = _greedy(lib, lg, [17, 2, 0, 5], 6, [3, 9], 1, out=torch.tensor([11, 12, -7, -7, -7, -7]))
    assert st == [18, 3, 0, 41] and out == [11, 12, 41, -7, -7, -7]
    st, out = _greedy(lib, lg, [0, 0, 0, 5], 6, [3, 9], 23)                  # the prompt's pick: advance = T
    assert st == [23, 1, 0, 41] and out[0] == 41
    for eos in ([41], [3, 41], [3, 9, 11, 41]):                                 # done by EOS (any of up to four)
        st, out = _greedy(lib, lg, [17, 2, 0, 5], 6, eos, 1)
        assert st == [18, 3, 1, 41] and out[2] == 41
    st, out = _greedy(lib, lg, [17, 5, 0, 5], 6, [3], 1)                        # done by max_new
    assert st == [18, 6, 1, 41] and out[5] == 41
    # a finished sequence changes no byte
    before = torch.tensor([11, 12, 13, -7, -7, -7])
    st, out = _greedy(lib, lg, [17, 3, 1, 13], 6, [3], 1, out=before)
    assert st == [17, 3, 1, 13] and out == before.tolist()
    # refusals
    pb = PlanBuilder(lib, _dev(lib), abi.F16)
    pb.greedy_pick(pb.buf((4,)), pb.buf((4,), torch.int32, zero=True), pb.buf((2,), torch.int32), 0, 2)
    with pytest.raises(ModelError):
        pb.build().run()


def check_greedy_run_of_steps(lib):
    """eight recorded picks replayed in one plan with an EOS at the fourth: the output ends there and the later picks change nothing"""
    vocab, max_new = 64, 16
    dev = _dev(lib)
    pb = PlanBuilder(lib, dev, abi.F16)
    toks = [5, 6, 7, 2, 8, 9, 10, 11]
    st = pb.const(torch.tensor([30, 0, 0, -1], dtype=torch.int32))
    ot = pb.const(torch.full((max_new,), -7, dtype=torch.int32))
    for t in toks:
        lg = torch.zeros(vocab); lg[t] = 1.0
        pb.greedy_pick(pb.const(lg), st, ot, vocab, max_new, eos=[2], advance=1)
    pb.build().run()
    _sync(lib)
    assert st.cpu().tolist() == [34, 4, 1, 2] and ot.cpu().tolist() == [5, 6, 7, 2] + [-7] * 12


def greedy_chunks(vocab):
    """greedy_launch's rule restated: chunk records per row; the folding wave reads record c in lane c % 64 on trip c // 64"""
    return (vocab + abi.GREEDY_CHUNK - 1) // abi.GREEDY_CHUNK


VOCAB_65 = 64 * abi.GREEDY_CHUNK + 1
assert greedy_chunks(VOCAB_65) == 65 and max(greedy_chunks(v) for v in VOCABS) <= 64, "VOCABS stays within one trip of the folding wave"


def greedy_65_cases(seed=0):
    """[(name, logits [VOCAB_65], expected token)]: record 64 is the one a lane reads on its second trip.  The expected token comes from the
    stated rule alone (largest value, lowest index among equals, a NaN never wins) and is asserted against torch here"""
    C_ = abi.GREEDY_CHUNK
    base = torch.randn(VOCAB_65, generator=torch.Generator().manual_seed(seed)).clamp_(-4.0, 4.0)
    alone = base.clone(); alone[64 * C_] = 9.0
    tie = base.clone(); tie[5] = 9.0; tie[64 * C_] = 9.0
    nan = base.clone(); nan[63 * C_ + 7] = 9.0; nan[64 * C_] = float("nan")
    cases = [("the maximum alone in chunk 64", alone, 64 * C_), ("equal maxima in chunks 0 and 64", tie, 5), ("a maximum in chunk 63, a NaN in chunk 64", nan, 63 * C_ + 7)]
    for name, lg, want in cases:
        clean = torch.nan_to_num(lg, nan=float("-inf"))
        assert float(clean.max()) == 9.0 and int((clean == 9.0).nonzero()[0]) == want, name
    assert alone[:64 * C_].max() < 9.0 and 64 * C_ // C_ == 64 and (63 * C_ + 7) // C_ == 63 and 5 // C_ == 0
    return cases


def check_greedy_65_chunks(lib):
    """three launches of the single op at 65 chunk records (greedy_final_kernel's loop takes a second trip in lane 0)"""
    for name, lg, want in greedy_65_cases():
        st, out = _greedy(lib, lg, [10, 1, 0, -1], 4, [], 1)
        assert st == [11, 2, 0, want] and out == [-7, want, -7, -7], f"65 chunks, {name}: state {st}, expected token {want}"


def check_greedy_damaged_state(lib):
    """n_out = -1 and n_out = max_new with done = 0: done = 1, every other state word and all of `out` unchanged"""
    vocab, max_new = 300, 6
    lg = torch.zeros(vocab); lg[41] = 1.0
    before = torch.tensor([11, 12, 13, -7, -7, -7])
    for n_out in (-1, max_new, max_new + 3):
        st, out = _greedy(lib, lg, [17, n_out, 0, 5], max_new, [3], 1, out=before)
        assert st == [17, n_out, 1, 5] and out == before.tolist(), f"damaged state n_out={n_out}: state {st} out {out}"


def check_greedy_all_nan(lib, vocab):
    """all-NaN logits: no record ever replaces the start value, the token is 0 and the state advances as for any other token"""
    lg = torch.full((vocab,), float("nan"))
    st, out = _greedy(lib, lg, [17, 2, 0, 5], 6, [3], 1, out=torch.tensor([11, 12, -7, -7, -7, -7]))
    assert st == [18, 3, 0, 0] and out == [11, 12, 0, -7, -7, -7], f"all NaN, vocab {vocab}: state {st} out {out}"
    st, out = _greedy(lib, lg, [17, 2, 0, 5], 6, [0], 1)          # and token 0 is an end-of-sequence token like any other
    assert st == [18, 3, 1, 0]


# ---- MTX_EW_QK_ROPE at head width 72 ---------------------------------------------------------------------------------------------------------
def check_rope_widths(lib, dtype, widths=(64, 72, 128), rows=37, heads=2, seed=0):
    """random q | k and angles at every width on the SAME draws (a width reads the leading columns of one set): within 1 unit in the last place
    of the fp32 formula rounded once (the kernel may contract x0 c - x1 s where torch does not: a last-bit difference in fp32 can move the
    rounded value by one step, not more); 64 and 128 are the control.  Returns {width: (ulp, differing elements)}."""
    import sam3_checks as s3
    dev = "cpu" if lib.is_simulator else "cuda:0"
    g = torch.Generator().manual_seed(seed)
    dmax = max(widths)
    ang_all = torch.rand(rows, dmax // 2, generator=g) * 6.28
    x_all = torch.randn(rows, 3, heads, dmax, generator=g)
    out = {}
    for d in widths:
        ang = ang_all[:, :d // 2]
        tab = torch.stack([ang.cos(), ang.sin()], 1)
        cs = torch.stack([tab, tab * 0.5])                        # the q heads read the second copy
        qkv = x_all[..., :d].reshape(rows, 3 * heads * d).to(TD[dtype]).float()
        want = s3.rope_formula(qkv, cs, heads, d).to(TD[dtype]).float()
        got = s3.run_qk_rope(lib, dev, dtype, qkv, cs, heads, d)
        assert torch.equal(got[:, 2 * heads * d:], qkv[:, 2 * heads * d:]), f"d={d}: the v slice was touched"
        ulp = torch.maximum(want.abs(), torch.full_like(want, 2.0 ** -14)).log2().floor().exp2() * 2.0 ** -MANT[dtype]
        worst = float(((got - want).abs() / ulp).max())
        assert worst <= 1.0, f"qk_rope d={d}: {worst} ulp"
        out[d] = (worst, int((got != want).sum()))
    return out


def check_rope_exact(lib, dtype, d):
    """exact inputs (sam3_checks.check_qk_rope_exact): bit for bit the formula, at the new width and at the two old ones"""
    import sam3_checks as s3
    s3.check_qk_rope_exact(lib, "cpu" if lib.is_simulator else "cuda:0", dtype, d)


def check_rope_refusals(lib):
    dev = _dev(lib)
    for d in (4, 68, 136):
        pb = PlanBuilder(lib, dev, abi.BF16)
        buf = pb.buf((3, 3 * 2 * d), torch.bfloat16, zero=True)
        tab = pb.buf((3, 2, d // 2), torch.float32, zero=True)
        pb.qk_rope(Act(buf.view(1, 1, 3, 6 * d), 1, 1, 3, 4 * d), tab, d)
        with pytest.raises(ModelError):
            pb.build().run()


# ---- the model against the transformers oracle ----------------------------------------------------------------------------------------------------
# Tiny configuration used throughout: vision 144 wide / 2 layers / 2 heads (head width 72) / MLP 256 / image_size 56; text 256 wide / 2 layers /
# 4 query heads over 2 key-value heads / head_dim 128 / MLP 384 / vocabulary 512 / mrope_section [16, 24, 24]; torch.manual_seed(seed) before
# construction, then every tensor of >= 2 dimensions and every bias redrawn N(0, 0.1) from torch.Generator().manual_seed(1000 + seed) (with the
# wheel's 0.02 the tied head just repeats the last token and greedy decoding shows nothing).  The oracle is the wheel's model in fp32 on the CPU.
import functools
import json

IMAGE, VIDEO, V_START, V_END = 500, 501, 502, 503
EOS_TINY = 2
TINY = dict(v=dict(hidden_size=144, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14),
            t=dict(vocab_size=512, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128))
REAL = dict(v=dict(), t=dict(vocab_size=8192))                     # the wheel's default sizes with the vocabulary cut to 8 192
STEPS = 20


SIGMA = 0.1                        # the teacher-forced tests' weights
GREEDY_SIGMA = 0.06                # the greedy test's (see tests/test_paddle_ocr_vl_sim.py, test_greedy_tokens_on_decided_prefixes)


@functools.lru_cache(maxsize=18)
def oracle(seed, real=False, sigma=SIGMA):
    """(config, model) — built once per (seed, sigma) and shared, never modified"""
    from transformers import PaddleOCRVLConfig, PaddleOCRVLForConditionalGeneration
    dims = REAL if real else TINY
    rope = dict(rope_type="default", rope_theta=10000.0, mrope_section=[16, 24, 24])
    cfg = PaddleOCRVLConfig(vision_config=dict(dims["v"]), text_config=dict(dims["t"], rope_parameters=rope, eos_token_id=EOS_TINY, pad_token_id=0, bos_token_id=1),
                            image_token_id=IMAGE, video_token_id=VIDEO, vision_start_token_id=V_START, vision_end_token_id=V_END)
    torch.manual_seed(seed)
    model = PaddleOCRVLForConditionalGeneration(cfg).eval()
    if not real:
        g = torch.Generator().manual_seed(1000 + seed)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.dim() >= 2 or name.endswith(".bias"):
                    p.copy_(torch.randn(p.shape, generator=g) * sigma)
        model.tie_weights()
    return cfg, model


def make_inputs(seed, grid=(4, 6), before=(1, 10, 11), after=(20, 21, 22), extra=()):
    """prompt ids [1, T] (text, image start, the merged grid's placeholders, image end, text, then `extra` tokens), pixel values, grid"""
    gh, gw = grid
    ids = torch.tensor([list(before) + [V_START] + [IMAGE] * (gh * gw // 4) + [V_END] + list(after) + list(extra)])
    pix = torch.randn(gh * gw, 3, 14, 14, generator=torch.Generator().manual_seed(100 + seed))
    return ids, pix, torch.tensor([[1, gh, gw]])


def oracle_logits(model, ids, pix, thw):
    with torch.no_grad():
        out = model(input_ids=ids, pixel_values=pix, image_grid_thw=thw, mm_token_type_ids=(ids == IMAGE).int(), attention_mask=torch.ones_like(ids))
    return out.logits[0].float()


@functools.lru_cache(maxsize=40)
def oracle_greedy(seed, grid=(4, 6), before=(1, 10, 11), after=(20, 21, 22), steps=STEPS, sigma=SIGMA):
    """the oracle's own greedy continuation, EOS not honoured: (tokens [steps], log-probs [steps, vocab], top-1 / top-2 gaps [steps])"""
    _, model = oracle(seed, sigma=sigma)
    toks, lps, gaps = [], [], []
    for _ in range(steps):
        ids, pix, thw = make_inputs(seed, grid, before, after, tuple(toks))
        lp = torch.log_softmax(oracle_logits(model, ids, pix, thw)[-1], -1)
        top = torch.topk(lp, 2).values
        toks.append(int(lp.argmax())); lps.append(lp); gaps.append(float(top[0] - top[1]))
        if IMAGE <= toks[-1] <= V_END:               # a placeholder token cannot be fed back (the wheel counts them against the image): the run,
            gaps[-1] = 0.0                         # and with it any decided prefix, ends before it
            break
    return toks, torch.stack(lps), gaps


def hip_model(lib, dtype, seed, real=False, sigma=SIGMA, **kw):
    from mangatranslator_amd.core.ml import paddle_ocr_vl as pv
    cfg, model = oracle(seed, real, sigma)
    hp = pv.hparams_from_config(cfg.to_dict(), model.generation_config.to_dict())
    hp.update(kw.pop("hp", {}))
    sd = pv.normalise_state_dict(dict(model.state_dict()), hp)
    kw.setdefault("max_new_tokens", 48)
    kw.setdefault("max_prompt", 64)
    return pv.PaddleOcrVlHip(sd, hp, device=_dev(lib), lib=lib, dtype=dtype, **kw)


def check_teacher_forced(lib, dtype, seed, grid=(4, 6), before=(1, 10, 11), after=(20, 21, 22), sigma=SIGMA):
    """the prompt's last row and STEPS - 1 steps fed with the oracle's own tokens: (max, rms) absolute log-prob error over STEPS distributions"""
    toks, ref, _ = oracle_greedy(seed, grid, before, after, sigma=sigma)
    ids, pix, thw = make_inputs(seed, grid, before, after)
    m = hip_model(lib, dtype, seed, sigma=sigma)
    try:
        T = m.prefill(ids, pix, thw)
        assert m.read_state()[:3] == [T, 1, 0]
        rows = [m.logits[0].float().cpu().clone()]
        for t in toks[:-1]:
            rows.append(m.step_logits(t))
    finally:
        m.close()
    assert len(rows) == ref.shape[0] and (sigma != SIGMA or len(rows) == STEPS)
    err = torch.log_softmax(torch.stack(rows), -1) - ref
    assert bool(torch.isfinite(err).all())
    return float(err.abs().max()), float(err.pow(2).mean().sqrt())


def decided_prefix(seed, delta, sigma=GREEDY_SIGMA):
    """how many leading steps of the oracle's greedy run are decided (its own top-1 / top-2 gap >= delta), ending at its first EOS"""
    toks, _, gaps = oracle_greedy(seed, sigma=sigma)
    n = 0
    for t, g in zip(toks, gaps):
        if g < delta:
            break
        n += 1
        if t == EOS_TINY:
            break
    return toks, n


def check_greedy_tokens(lib, dtype, seed, delta, check_every=8, sigma=GREEDY_SIGMA):
    """the device loop's tokens equal the oracle's over the decided prefix; returns its length"""
    toks, n = decided_prefix(seed, delta, sigma)
    ids, pix, thw = make_inputs(seed)
    m = hip_model(lib, dtype, seed, sigma=sigma)
    try:
        out = m.generate(input_ids=ids, pixel_values=pix, image_grid_thw=thw, max_new_tokens=STEPS, check_every=check_every)
    finally:
        m.close()
    assert out.dtype == torch.int64 and out.shape[0] == 1 and torch.equal(out[0, :ids.shape[1]], ids[0])
    got = out[0, ids.shape[1]:].tolist()
    assert got[:n] == toks[:n], f"seed {seed}: device {got[:n]} != oracle {toks[:n]} over the decided prefix of {n}"
    return n


def check_generate_matches_wheel(seed=0, steps=8):
    """the manual greedy loop above is `generate(do_sample=False)` (up to the wheel's EOS)"""
    _, model = oracle(seed)
    ids, pix, thw = make_inputs(seed)
    with torch.no_grad():
        gen = model.generate(input_ids=ids, pixel_values=pix, image_grid_thw=thw, mm_token_type_ids=(ids == IMAGE).int(), attention_mask=torch.ones_like(ids),
                             max_new_tokens=steps, do_sample=False)
    got = gen[0, ids.shape[1]:].tolist()
    want = oracle_greedy(seed)[0][:steps]
    if EOS_TINY in want:
        want = want[:want.index(EOS_TINY) + 1]
    assert got[:len(want)] == want


def check_device_loop(lib, dtype, seed=0):
    """check_every 1 and 8 give the same tokens; an EOS in the middle of a run of 8 ends the output there"""
    toks, _, _ = oracle_greedy(seed)
    ids, pix, thw = make_inputs(seed)
    runs = {}
    for every in (1, 8):
        m = hip_model(lib, dtype, seed)
        try:
            runs[every] = m.generate(input_ids=ids, pixel_values=pix, image_grid_thw=thw, max_new_tokens=12, check_every=every)[0, ids.shape[1]:].tolist()
        finally:
            m.close()
    assert runs[1] == runs[8] and len(runs[1]) == 12 or EOS_TINY in runs[1], runs
    assert runs[1] == runs[8]
    stop = runs[8][3]                                       # the fourth token as the end-of-sequence token: the run of 8 holds it in its middle
    first = runs[8].index(stop)
    m = hip_model(lib, dtype, seed, hp=dict(eos=[stop]))
    try:
        out = m.generate(input_ids=ids, pixel_values=pix, image_grid_thw=thw, max_new_tokens=12, check_every=8)[0, ids.shape[1]:].tolist()
        st = m.read_state()
    finally:
        m.close()
    assert out == runs[8][:first + 1] and st[1] == first + 1 and st[2] == 1, (out, runs[8], st)
    # a smaller budget than the model was built for ends the output there
    m = hip_model(lib, dtype, seed)
    try:
        assert m.generate(input_ids=ids, pixel_values=pix, image_grid_thw=thw, max_new_tokens=5, check_every=8)[0, ids.shape[1]:].tolist() == runs[8][:5]
    finally:
        m.close()


def check_refusals():
    from mangatranslator_amd.core.ml import paddle_ocr_vl as pv
    cfg, model = oracle(0)
    base = cfg.to_dict()

    def bad(edit, gen=None):
        c = json.loads(json.dumps(base, default=str))
        edit(c)
        with pytest.raises(ModelError):
            pv.hparams_from_config(c, gen)
    bad(lambda c: c["text_config"]["rope_parameters"].update(rope_type="yarn"))
    bad(lambda c: c["text_config"].update(layer_types=["sliding_attention", "full_attention"]))
    bad(lambda c: c["text_config"].update(head_dim=64))
    bad(lambda c: None, gen=dict(do_sample=True))
    bad(lambda c: None, gen=dict(num_beams=4))
    bad(lambda c: None, gen=dict(repetition_penalty=1.2))
    hp = pv.hparams_from_config(base, model.generation_config.to_dict())
    sd = dict(model.state_dict())
    tied = dict(sd); tied.pop("lm_head.weight")
    assert "lm_head.weight" in pv.normalise_state_dict(tied, hp)
    # the hub file's names (the wheel's conversion mapping, which its save_pretrained applies backwards) and the tensors the wheel drops
    hub = {}
    for k, v in tied.items():
        k = "mlp_AR" + k[len("model.projector"):] if k.startswith("model.projector") else k
        k = k[len("model."):] if k.startswith("model.visual") else k
        k = "model" + k[len("model.language_model"):] if k.startswith("model.language_model") else k
        hub[k] = v
    hub["visual.vision_model.head.probe.weight"] = torch.zeros(1)
    assert "mlp_AR.linear_1.weight" in hub and "model.embed_tokens.weight" in hub and "visual.vision_model.post_layernorm.bias" in hub
    back = pv.normalise_state_dict(hub, hp)
    assert set(back) == set(sd) and all(back[k] is sd[k] or torch.equal(back[k], sd[k]) for k in sd)
    for edit in (lambda d: d.pop("model.projector.linear_1.bias"), lambda d: d.update({"model.visual.vision_model.extra.probe": torch.zeros(1)})):
        d = dict(sd); edit(d)
        with pytest.raises(ModelError):
            pv.normalise_state_dict(d, hp)


def check_input_refusals(lib):
    m = hip_model(lib, abi.F16, 0)
    ids, pix, thw = make_inputs(0)
    try:
        for kw in (dict(input_ids=torch.cat([ids, ids])), dict(image_grid_thw=torch.cat([thw, thw])), dict(pixel_values_videos=pix), dict(do_sample=True),
                   dict(num_beams=2), dict(repetition_penalty=1.3), dict(max_new_tokens=10 ** 6)):
            with pytest.raises(ModelError):
                m.generate(**dict(dict(input_ids=ids, pixel_values=pix, image_grid_thw=thw), **kw))
    finally:
        m.close()


# ---- a staged directory ----------------------------------------------------------------------------------------------------------------------------
TEMPLATE = ("<s> {% for m in messages %}User: {% for c in m['content'] %}{% if c['type'] == 'image' %}<|IMAGE_START|> <|IMAGE_PLACEHOLDER|> <|IMAGE_END|> "
            "{% else %}{{ c['text'] }} {% endif %}{% endfor %}{% endfor %}{% if add_generation_prompt %}Assistant:{% endif %}")
SIZE = {"shortest_edge": 28 * 28 * 4, "longest_edge": 28 * 28 * 16}


def stage_directory(root, seed=0, eos=None):
    """`save_pretrained` of the tiny oracle plus a synthetic processor: a 512-entry WordLevel vocabulary with the placeholder tokens at the
    config's ids, a one-line chat template, the PIL image processor's settings with small size bounds"""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from transformers.models.paddleocr_vl.image_processing_pil_paddleocr_vl import PaddleOCRVLImageProcessorPil
    _, model = oracle(seed)
    root.mkdir(parents=True, exist_ok=True)
    model.save_pretrained(str(root), safe_serialization=True)
    if eos is not None:
        gen = json.loads((root / "generation_config.json").read_text()) if (root / "generation_config.json").is_file() else {}
        gen["eos_token_id"] = eos
        (root / "generation_config.json").write_text(json.dumps(gen))
    words = ["<pad>", "<s>", "</s>", "<unk>"] + [f"w{i}" for i in range(4, IMAGE)] + ["<|IMAGE_PLACEHOLDER|>", "<|VIDEO_PLACEHOLDER|>", "<|IMAGE_START|>", "<|IMAGE_END|>"]
    words += [f"x{i}" for i in range(len(words), 512)]
    vocab = {w: i for i, w in enumerate(words)}
    for word, old in (("OCR:", "w10"), ("User:", "w11"), ("Assistant:", "w12")):
        vocab[word] = vocab.pop(old)
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    PreTrainedTokenizerFast(tokenizer_object=tok, bos_token="<s>", eos_token="</s>", pad_token="<pad>", unk_token="<unk>",
                            additional_special_tokens=["<|IMAGE_PLACEHOLDER|>", "<|VIDEO_PLACEHOLDER|>", "<|IMAGE_START|>", "<|IMAGE_END|>"],
                            extra_special_tokens={"image_token": "<|IMAGE_PLACEHOLDER|>", "video_token": "<|VIDEO_PLACEHOLDER|>"}).save_pretrained(str(root))
    (root / "chat_template.jinja").write_text(TEMPLATE)
    ip = PaddleOCRVLImageProcessorPil().to_dict()
    ip.update(size=SIZE, resample=3, image_mean=list(ip["image_mean"]), image_std=list(ip["image_std"]))
    (root / "preprocessor_config.json").write_text(json.dumps(ip))
    return root


def test_image():
    import numpy as np
    from PIL import Image
    yy, xx = np.mgrid[0:50, 0:90]
    return Image.fromarray(((xx * 7 + yy * 13) % 97 + 80).astype(np.uint8)).convert("RGB")


def check_end_to_end(lib, tmp_path, monkeypatch):
    """staged directory -> get_model_manager().get_paddle_ocr_vl() -> the unchanged driver: two strings, the second the marker, the first the
    oracle's tokens decoded; nothing staged -> ModelError and markers; unload_ocr_models empties the slot"""
    from mangatranslator_amd.core.image import ocr_detection as od
    from mangatranslator_amd.core.ml import paddle_ocr_vl as pv
    from mangatranslator_amd.core.ml.model_manager import ModelType, get_model_manager
    mgr = get_model_manager()
    monkeypatch.setitem(mgr.model_paths, ModelType.PADDLE_OCR_VL, tmp_path / "paddleocr-vl-1.6")
    monkeypatch.setitem(mgr.models, ModelType.PADDLE_OCR_VL, None)
    assert not mgr.paddle_ocr_vl_available()
    with pytest.raises(ModelError, match="paddleocr-vl-1.6"):
        mgr.get_paddle_ocr_vl()
    img = test_image()
    assert od.extract_text_with_paddle_ocr_vl([img, None]) == ["[OCR FAILED]", "[OCR FAILED]"]
    # what the oracle reads: its greedy tokens on the processor's own tensors, the sixth one made the end-of-sequence token
    root = stage_directory(tmp_path / "paddleocr-vl-1.6")
    proc = pv.build_processor(root)
    messages = [{"role": "user", "content": [{"type": "image", "image": img}, {"type": "text", "text": "OCR:"}]}]
    inputs = proc.apply_chat_template(messages, add_generation_prompt=True, tokenize=True, return_dict=True, return_tensors="pt",
                                      processor_kwargs={"images_kwargs": {"size": SIZE}})
    assert set(inputs) >= {"input_ids", "attention_mask", "mm_token_type_ids", "pixel_values", "image_grid_thw"} and inputs["pixel_values"].shape[1:] == (3, 14, 14)
    _, model = oracle(0)
    toks = []
    for _ in range(6):
        ids = torch.cat([inputs["input_ids"], torch.tensor([toks], dtype=torch.long)], 1)
        toks.append(int(oracle_logits(model, ids, inputs["pixel_values"], inputs["image_grid_thw"])[-1].argmax()))
    stop = toks[5]
    want = proc.decode(toks[:toks.index(stop)]).strip()
    stage_directory(root, eos=stop)
    if lib.is_simulator:
        monkeypatch.setattr(pv, "get_library", lambda: lib)
        monkeypatch.setattr(mgr, "device", torch.device("cpu"))
    assert mgr.paddle_ocr_vl_available()
    try:
        texts = od.extract_text_with_paddle_ocr_vl([img, None])
        assert texts == [want, "[OCR FAILED]"], (texts, want, toks)
        assert mgr.is_loaded(ModelType.PADDLE_OCR_VL) and mgr.get_paddle_ocr_vl() is mgr.get_paddle_ocr_vl()
    finally:
        mgr.unload_ocr_models()
    assert not mgr.is_loaded(ModelType.PADDLE_OCR_VL)


def check_published_widths(lib, dtype, seed=0, steps=40):
    """seeded weights at the wheel's default sizes (vocabulary 8 192), grid 20 x 28, 40 teacher-forced random tokens; positions 0-9 and 30-39:
    (max, rms) absolute log-prob error"""
    _, model = oracle(seed, real=True)
    g = torch.Generator().manual_seed(seed)
    teacher = torch.randint(3, 8000, (steps,), generator=g).tolist()
    ids, pix, thw = make_inputs(seed, grid=(20, 28), extra=tuple(teacher[:-1]))
    T = ids.shape[1] - (steps - 1)
    ref = torch.log_softmax(oracle_logits(model, ids, pix, thw)[T - 1:], -1)                    # [steps, vocab]
    m = hip_model(lib, dtype, seed, real=True, max_new_tokens=steps + 8, max_prompt=T + 8)
    try:
        assert m.prefill(ids[:, :T], pix, thw) == T
        rows = [m.logits[0].float().cpu().clone()]
        for t in teacher[:-1]:
            rows.append(m.step_logits(t))
    finally:
        m.close()
    err = torch.log_softmax(torch.stack(rows), -1) - ref
    err = torch.cat([err[:10], err[30:40]])
    return float(err.abs().max()), float(err.pow(2).mean().sqrt())

"""Checks of MTX_OP_REL_ATTN (csrc/relattn.hip: attention with a Toeplitz bias and a device-side key count), written once and run on the
simulator (tests/test_rel_attn_sim.py) and on the product library (tests/test_rel_attn_gpu.py).

Exact checks (in the style of paddle_ocr_vl_checks.check_causal_selection): one key of a row scores 0 and every other visible key at most
-120; exp(-120) underflows to exactly 0 in fp32, so the row must be that key's V row of ITS kv head, bit for bit.
  bias alone      q = 0; head h's table is 0 at offset DELTAS[h] and -120 elsewhere.  A sign flip or an off-by-one in j - i + s - 1, a table row
                  of another head or a wrong GQA group returns another V row.  Rows whose winner falls outside [0, s) weigh all keys alike
                  and are held to the fp32 reference under the random bound.
  bias after scale   scores scale * q.k = -160 [j != 0] from ONE exact product (q = -1280, k = [j != 0], scale = 2^-3); the table holds +320 at
                  the offsets +1 and 1 - s, so key b = (i + 1) mod s scores 160 and wins by 160.  Read as scale * (q.k + bias) it scores -120
                  and key 0 wins by 120.
  key limit       q = 0; head h's table is -120 below offset d_h, 0 at d_h and +8 above, d_h = n - 1 - r_h: in row r_h the last visible key
                  n - 1 scores 0 and every key at or beyond n_keys scores 8.  That row must be V[n - 1] bit for bit; the other rows are held
                  to the reference.  The scalar is rewritten between replays of ONE recorded plan.
Random: against fp32 torch (scores and softmax in fp32, the weighted sum in float64) on the same 16-bit inputs, with the bound of
paddle_ocr_vl_checks.check_causal_random: half a spacing of T at the reference (the one rounding) plus the fp32 softmax's own error,
s * 2^-23 of the largest value.
Every rig pads the row strides, poisons the padding and the rows behind s of q, k, v with NaN patterns and keeps a guard band of sentinel
rows and columns around o."""
import ctypes as C

import pytest
import torch

from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _sync
from paddle_ocr_vl_checks import MANT, NAN_BITS, CausalRig, _bits

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 77, 131]
WIDTHS = [64, 128]
HEADS = [(2, 2), (4, 2), (8, 2)]
DTYPES = [abi.BF16, abi.F16]
DELTAS = [0, 1, -2, 3, -4, 5, -6, 7]          # head h's winning offset j - i: distinct, both signs
GUARD = 3                                     # rows before and behind o, and behind q, k, v
PAD = 8                                       # columns behind every row
SENTINEL = 7.0
MTX_ERR_INVALID, MTX_ERR_UNSUPPORTED = -1, -3      # include/mtx_hip.h
MASKED = abi.REL_MASKED


def key_limits(s):
    """the issue's n_keys cases that name at least one key"""
    return sorted({n for n in (1, 31, 32, 33, s - 1, s, s + 5) if n >= 1})


def causal_table(heads, s, masked=MASKED, ld=None):
    """fp32 [heads, ld]: 0 for j <= i (entries 0 .. s - 1), masked above"""
    t = torch.full((heads, ld or 2 * s - 1), float(masked))
    t[:, :s] = 0.0
    return t


class RelRig:
    """one recorded MTX_OP_REL_ATTN; `run` fills the operands and launches it.  q [s + GUARD, heads * d + PAD], k and v [s + GUARD,
    kv * d + PAD], o [GUARD + s + GUARD, heads * d + PAD] entered at row GUARD, rel [heads, 2 s - 1 + 2] (an odd row length: rows are 4-byte
    aligned only), n_keys an int32 scalar"""

    def __init__(self, lib, dtype, s, heads, kv, d, scale=None, biased=True, limited=True):
        self.lib, self.dev, self.td, self.dtype = lib, _dev(lib), TD[dtype], dtype
        self.s, self.heads, self.kv, self.d = s, heads, kv, d
        self.scale = d ** -0.5 if scale is None else scale
        self.ld_q, self.ld_kv, self.ld_rel = heads * d + PAD, kv * d + PAD, 2 * s - 1 + 2
        pb = PlanBuilder(lib, self.dev, dtype)
        self.q = pb.buf((s + GUARD, self.ld_q), self.td, zero=True)
        self.k = pb.buf((s + GUARD, self.ld_kv), self.td, zero=True)
        self.v = pb.buf((s + GUARD, self.ld_kv), self.td, zero=True)
        self.o = pb.buf((s + 2 * GUARD, self.ld_q), self.td, zero=True)
        self.rel = pb.buf((heads, self.ld_rel), torch.float32, zero=True) if biased else None
        self.n_keys = pb.buf((1,), torch.int32, zero=True) if limited else None
        pb.rel_attention(self.q, self.k, self.v, self.o, s, heads, kv, d, (self.ld_q, d), (self.ld_kv, d), (self.ld_kv, d), (self.ld_q, d),
                         self.scale, rel=self.rel, n_keys=self.n_keys, o_off=GUARD * self.ld_q)
        self.pb, self.plan = pb, None

    def _padded(self, x, ld):
        """[s, w] -> [s + GUARD, ld] with NaN patterns in the padding columns and in the rows behind s"""
        out = torch.full((self.s + GUARD, ld), NAN_BITS, dtype=torch.int16).view(self.td)
        out[:self.s, :x.shape[1]] = x.to(self.td)
        return out

    def run(self, q=None, k=None, v=None, rel=None, n_keys=None):
        """q [s, heads * d], k / v [s, kv * d], rel [heads, 2 s - 1]; what is None keeps its bytes.  -> o [s, heads * d] on the host"""
        if q is not None:
            self.q.copy_(self._padded(q, self.ld_q))
        if k is not None:
            self.k.copy_(self._padded(k, self.ld_kv))
        if v is not None:
            self.v.copy_(self._padded(v, self.ld_kv))
        if rel is not None:
            full = torch.full((self.heads, self.ld_rel), float("nan"))
            full[:, :2 * self.s - 1] = rel
            self.rel.copy_(full)
        if n_keys is not None:
            self.n_keys.fill_(n_keys)
        self.o.fill_(SENTINEL)
        if self.plan is None:
            self.plan = self.pb.build()
        self.plan.run()
        _sync(self.lib)
        o = self.o.cpu()
        w = self.heads * self.d
        guard = torch.cat([o[:GUARD].flatten(), o[GUARD + self.s:].flatten(), o[GUARD:GUARD + self.s, w:].flatten()])
        assert bool((guard.float() == SENTINEL).all()), f"rel_attn s={self.s} heads={self.heads}/{self.kv} d={self.d}: the guard band of o was written"
        return o[GUARD:GUARD + self.s, :w].clone()


def rel_ref(q, k, v, rel, n_keys, scale, heads, kv, d):
    """fp32 scores and softmax, float64 weighted sum, on the same 16-bit inputs: [s, heads * d] float64.  A row without a visible key is 0"""
    s = q.shape[0]
    G = heads // kv
    qf = q.float().view(s, heads, d)
    kf = k.float().view(s, kv, d).repeat_interleave(G, 1)
    vf = v.double().view(s, kv, d).repeat_interleave(G, 1)
    sc = torch.einsum("ihd,jhd->hij", qf, kf) * scale
    i, j = torch.arange(s)[:, None], torch.arange(s)[None, :]
    hidden = (j >= min(s, n_keys if n_keys is not None else s)).expand(s, s)[None].expand(heads, s, s)
    if rel is not None:
        bias = rel[:, (j - i + s - 1)]
        hidden = hidden | ~(bias > MASKED)
        sc = sc + torch.where(hidden, torch.zeros(()), bias)
    sc = sc.masked_fill(hidden, float("-inf"))
    p = torch.softmax(sc, dim=-1)
    p = torch.where(hidden.all(-1, keepdim=True), torch.zeros(()), p)
    return torch.einsum("hij,jhd->ihd", p.double(), vf).reshape(s, heads * d)


def ratio_to_bound(got, ref, v, dtype, s):
    """largest error of `got` relative to: half a spacing of T at the reference + s * 2^-23 of the largest value"""
    vmax = float(v.double().abs().max())
    bound = ref.abs() * 2.0 ** -(MANT[dtype] + 1) * (1 + 2.0 ** -6) + s * 2.0 ** -23 * vmax
    return float(((got.double() - ref).abs() / bound).max())


def _rows_of(vals, rows, heads, kv, d):
    """vals [s, kv * d], rows [s, heads] of key indices -> [s, heads * d]: V[rows[i, h]] of head h's kv head"""
    s = vals.shape[0]
    kvh = torch.arange(heads) // (heads // kv)
    return vals.view(s, kv, d)[rows, kvh[None, :].expand(s, heads)].reshape(s, heads * d)


# ---- 1. the bias alone selects ------------------------------------------------------------------------------------------------------------------
def check_bias_selects(lib, dtype, s, heads, kv, d, seed=0):
    g = torch.Generator().manual_seed(seed + s * 31 + heads * 7 + d)
    rig = RelRig(lib, dtype, s, heads, kv, d, limited=False)
    rel = torch.full((heads, 2 * s - 1), -120.0)
    win = torch.zeros(s, heads, dtype=torch.long)
    has = torch.zeros(s, heads, dtype=torch.bool)
    i = torch.arange(s)
    for h in range(heads):
        dl = DELTAS[h]
        if -s < dl < s:
            rel[h, dl + s - 1] = 0.0
        win[:, h] = (i + dl).clamp(0, s - 1)
        has[:, h] = (i + dl >= 0) & (i + dl < s)
    q = torch.zeros(s, heads * d)
    k = torch.randn(s, kv * d, generator=g)
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    got = rig.run(q, k, v, rel)
    what = f"rel_attn (bias selects) s={s} heads={heads}/{kv} d={d}"
    want = _rows_of(v, win, heads, kv, d)
    differ = (_bits(got) != _bits(want)).view(s, heads, d).any(-1) & has
    wrong = differ.any(0).nonzero().flatten().tolist()
    assert not wrong, f"{what}: heads {wrong} differ from V[i + delta_h] of their kv head ({int(differ.sum())} rows)"
    ref = rel_ref(q.to(rig.td), k.to(rig.td), v, rel, None, rig.scale, heads, kv, d)
    loose = ~has[:, :, None].expand(s, heads, d).reshape(s, heads * d)
    if bool(loose.any()):
        r = ratio_to_bound(torch.where(loose, got.double(), ref), ref, v, dtype, s)
        assert r <= 1.0, f"{what}: rows without a winner are {r:.2f} x the bound from the reference"
    return int(has.sum())


# ---- 2. the bias is added after the scale ----------------------------------------------------------------------------------------------------------
def check_bias_after_scale(lib, dtype, s, heads, kv, d, seed=0):
    assert s >= 2
    g = torch.Generator().manual_seed(seed + s)
    scale = 2.0 ** -3
    rig = RelRig(lib, dtype, s, heads, kv, d, scale=scale, limited=False)
    j = torch.arange(s)
    q = torch.zeros(s, heads, d)
    q[:, :, 0] = -1280.0
    k = torch.zeros(s, kv, d)
    k[:, :, 0] = (j != 0).float()[:, None]
    assert torch.equal(q, q.to(rig.td).float()), "the test's own premise: every feature is exact in the storage type"
    rel = torch.zeros(heads, 2 * s - 1)
    rel[:, 1 + s - 1] = 320.0
    rel[:, 1 - s + s - 1] = 320.0
    b = (j + 1) % s
    # the premise, from the score matrices of both readings
    qk = q[:, 0] @ k[:, 0].t()
    bias = rel[0][(j[None, :] - j[:, None] + s - 1)]
    right, wrong = qk * scale + bias, (qk + bias) * scale
    for i in range(s):
        others = torch.ones(s, dtype=torch.bool); others[b[i]] = False
        assert right[i, b[i]] - right[i, others].max() >= 120
        if b[i] != 0:
            others0 = torch.ones(s, dtype=torch.bool); others0[0] = False
            assert wrong[i, 0] - wrong[i, others0].max() >= 120
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    got = rig.run(q.reshape(s, heads * d), k.reshape(s, kv * d), v, rel)
    want = _rows_of(v, b[:, None].expand(s, heads), heads, kv, d)
    bad = (_bits(got) != _bits(want)).view(s, heads * d).any(-1)
    took_a = (_bits(got) == _bits(_rows_of(v, torch.zeros(s, heads, dtype=torch.long), heads, kv, d))).view(s, -1).all(-1) & (b != 0)
    assert not bool(bad.any()), (f"rel_attn (bias after scale) s={s} heads={heads}/{kv} d={d}: {int(bad.sum())} rows differ from V[(i + 1) mod s]; "
                                 f"{int((took_a & bad).sum())} of them are V[0], the winner when the bias is scaled too")


# ---- 3. the key limit -----------------------------------------------------------------------------------------------------------------------------
def check_key_limit(lib, dtype, s, heads, kv, d, seed=0):
    """every n of key_limits(s) and n = 0, -3 on ONE recorded plan; -> the number of replays"""
    g = torch.Generator().manual_seed(seed + s * 13 + heads)
    rig = RelRig(lib, dtype, s, heads, kv, d)
    q = torch.zeros(s, heads * d)
    k = torch.randn(s, kv * d, generator=g).to(rig.td)
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    first = True
    off = torch.arange(2 * s - 1) - (s - 1)
    limits = key_limits(s)
    for n in limits + limits[:1]:                  # (the first once more: the scalar goes down again as well as up)
        nk = min(n, s)
        rows = [(h * 37 + 5) % nk for h in range(heads)]           # r_h < nk <= s
        rel = torch.zeros(heads, 2 * s - 1)
        for h in range(heads):
            dh = nk - 1 - rows[h]
            rel[h] = torch.where(off < dh, torch.tensor(-120.0), torch.where(off == dh, torch.tensor(0.0), torch.tensor(8.0)))
        got = rig.run(q if first else None, k if first else None, v if first else None, rel, n)
        first = False
        what = f"rel_attn (key limit) s={s} n_keys={n} heads={heads}/{kv} d={d}"
        for h in range(heads):
            want = v.view(s, kv, d)[nk - 1, h // (heads // kv)]
            assert torch.equal(_bits(got.view(s, heads, d)[rows[h], h]), _bits(want)), \
                f"{what}: row {rows[h]} of head {h} is not V[n_keys - 1] (a key at or beyond the limit scores 8 above it)"
        ref = rel_ref(q.to(rig.td), k, v, rel, n, rig.scale, heads, kv, d)
        r = ratio_to_bound(got, ref, v, dtype, s)
        assert r <= 1.0, f"{what}: {r:.2f} x the bound from the reference"
    for n in (0, -3):
        got = rig.run(n_keys=n)
        assert bool((_bits(got) == 0).all()), f"rel_attn s={s} n_keys={n}: the rows are not zero"
    return len(limits) + 3


# ---- 4. masked entries ----------------------------------------------------------------------------------------------------------------------------
def check_masked_entries(lib, dtype, s, heads, kv, d, seed=0):
    """-inf and -1e30 both weigh 0: the causal table written either way gives the same bytes, within the bound of the reference; a table that
    hides every key of the last rows gives zero rows and no NaN"""
    g = torch.Generator().manual_seed(seed + s + d)
    rig = RelRig(lib, dtype, s, heads, kv, d, limited=False)
    q = (torch.randn(s, heads * d, generator=g) * 1.5).to(rig.td)
    k = (torch.randn(s, kv * d, generator=g) * 1.5).to(rig.td)
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    what = f"rel_attn (masked entries) s={s} heads={heads}/{kv} d={d}"
    a = rig.run(q, k, v, causal_table(heads, s, MASKED))
    b = rig.run(rel=causal_table(heads, s, float("-inf")))
    assert torch.equal(_bits(a), _bits(b)), f"{what}: -inf and -1e30 give different bytes"
    mixed = causal_table(heads, s, MASKED)
    mixed[:, s::2] = float("-inf")
    mixed[:, :s] = torch.randn(heads, s, generator=g)
    got = rig.run(rel=mixed)
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    r = ratio_to_bound(got, rel_ref(q, k, v, mixed, None, rig.scale, heads, kv, d), v, dtype, s)
    assert r <= 1.0, f"{what}: {r:.2f} x the bound"
    # offsets j - i >= cut hidden (alternately -inf and -1e30): row i sees the keys j < i + cut only, the first rows see none
    cut = -(s // 2)
    hide = torch.zeros(heads, 2 * s - 1)
    hide[:, cut + s - 1:] = MASKED
    hide[:, cut + s - 1::2] = float("-inf")
    got = rig.run(rel=hide)
    assert bool(torch.isfinite(got.float()).all()), f"{what}: a NaN in a row without a visible key"
    dark = torch.arange(s) + cut <= 0
    assert bool(dark.any()) and bool((_bits(got)[dark] == 0).all()), f"{what}: rows without a visible key are not zero"
    r = ratio_to_bound(got, rel_ref(q, k, v, hide, None, rig.scale, heads, kv, d), v, dtype, s)
    assert r <= 1.0, f"{what}: {r:.2f} x the bound"


# ---- random ---------------------------------------------------------------------------------------------------------------------------------------
def check_random(lib, dtype, s, heads, kv, d, n_keys=None, seed=0):
    """random table (N(0, 2), a tenth of the entries masked), twice: equal bytes; -> error / bound"""
    g = torch.Generator().manual_seed(seed * 1000 + s * 31 + heads + d)
    rig = RelRig(lib, dtype, s, heads, kv, d, limited=n_keys is not None)
    q = (torch.randn(s, heads * d, generator=g) * 1.5).to(rig.td)
    k = (torch.randn(s, kv * d, generator=g) * 1.5).to(rig.td)
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    rel = torch.randn(heads, 2 * s - 1, generator=g) * 2.0
    rel[torch.rand(heads, 2 * s - 1, generator=g) < 0.1] = MASKED
    got = rig.run(q, k, v, rel, n_keys)
    what = f"rel_attn s={s} heads={heads}/{kv} d={d} n_keys={n_keys}"
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output (padding or a row behind s was read)"
    again = rig.run()
    assert torch.equal(_bits(got), _bits(again)), f"{what}: two runs give different bytes"
    r = ratio_to_bound(got, rel_ref(q, k, v, rel, n_keys, rig.scale, heads, kv, d), v, dtype, s)
    assert r <= 1.0, f"{what}: error {r:.2f} x the bound (one rounding + fp32 softmax)"
    return r


def check_no_table(lib, dtype, s, heads, kv, d, seed=0):
    """rel = NULL and n_keys = NULL: plain bidirectional attention"""
    g = torch.Generator().manual_seed(seed + s)
    rig = RelRig(lib, dtype, s, heads, kv, d, biased=False, limited=False)
    q = (torch.randn(s, heads * d, generator=g) * 1.5).to(rig.td)
    k = (torch.randn(s, kv * d, generator=g) * 1.5).to(rig.td)
    v = torch.randn(s, kv * d, generator=g).to(rig.td)
    r = ratio_to_bound(rig.run(q, k, v), rel_ref(q, k, v, None, None, rig.scale, heads, kv, d), v, dtype, s)
    assert r <= 1.0, f"rel_attn without a table s={s}: {r:.2f} x the bound"


def check_equals_causal_op(lib, dtype, s, heads, kv, seed=0):
    """the causal table at d = 128 against mtx_causal_attention(pos = 0) on the same operands, under the random bound"""
    d = 128
    g = torch.Generator().manual_seed(seed + s * 3 + heads)
    rig = RelRig(lib, dtype, s, heads, kv, d, limited=False)
    ca = CausalRig(lib, dtype, s, heads, kv, s)
    qkv = (torch.randn(s, ca.w, generator=g) * 1.5).to(rig.td)
    q, k, v = qkv[:, :heads * d], qkv[:, heads * d:(heads + kv) * d], qkv[:, (heads + kv) * d:]
    got = rig.run(q, k, v, causal_table(heads, s))
    want = ca.run(qkv, pos=0).double()
    r = ratio_to_bound(got, want, v, dtype, s)
    assert r <= 1.0, f"rel_attn with the causal table vs causal_attention s={s} heads={heads}/{kv}: {r:.2f} x the bound"
    ref = rel_ref(q, k, v, causal_table(heads, s), None, rig.scale, heads, kv, d)
    assert ratio_to_bound(got, ref, v, dtype, s) <= 1.0
    return r


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    def rc_of(change, **kw):
        rig = RelRig(lib, abi.BF16, kw.pop("s", 8), kw.pop("heads", 4), kw.pop("kv", 2), kw.pop("d", 64))
        args = rig.pb.ops[-1].u.relattn
        change(args)
        rc = lib.mtx_rel_attention(C.byref(args), C.c_void_p(0))
        if rc != 0:
            with pytest.raises(ModelError):
                rig.pb.build().run()
        return rc

    def put(name, value):
        return lambda a: setattr(a, name, value)

    assert rc_of(lambda a: None) == 0
    _sync(lib)
    for what, change in (("d = 96", put("d", 96)), ("d = 32", put("d", 32)), ("s = 0", put("s", 0)),
                         ("s = 1025", put("s", abi.REL_ATTN_SMAX + 1)), ("heads 3 over 2", put("heads", 3)), ("kv_heads = 0", put("kv_heads", 0))):
        assert rc_of(change) == MTX_ERR_UNSUPPORTED, what
    for name in ("q", "k", "v", "o"):
        assert rc_of(put(name, None)) == MTX_ERR_INVALID, f"null {name}"
        assert rc_of(lambda a, name=name: setattr(a, name, getattr(a, name) + 8)) == MTX_ERR_INVALID, f"{name} 8-byte aligned only"
    for name in ("q_ss", "q_hs", "k_ss", "k_hs", "v_ss", "v_hs", "o_ss", "o_hs"):
        assert rc_of(lambda a, name=name: setattr(a, name, getattr(a, name) + 4)) == MTX_ERR_INVALID, f"{name} % 8 != 0"
    assert rc_of(put("dtype", abi.F32)) == MTX_ERR_INVALID
    assert rc_of(put("ld_rel", 2 * 8 - 2)) == MTX_ERR_INVALID
    assert rc_of(put("ld_rel", 2 * 8 - 1)) == 0
    _sync(lib)

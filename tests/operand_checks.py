"""Exact-input checks of the fp8 operand producers (every site that makes e4m3 bytes, with or without E8M0 block scales) and of the FLUX row
kernels (per-head RMSNorm + rotary, row softmax, the first-block cache probe) against references that share no arithmetic with the kernels.

THE TWO FORMATS, restated on the host in float64 and integers:

  e4m3   round to nearest, ties to the even code, from the table of the 127 finite non-negative magnitudes (code c: c < 8 -> c * 2^-9, else
         (1 + (c & 7) / 8) * 2^((c >> 3) - 7); code 126 = 448); the sign bit is kept, also on zero; inputs arrive clamped to +-448.
  E8M0   per 32 consecutive k: eb = the smallest value with 448 * 2^(eb - 127) >= amax IN EXACT ARITHMETIC, clamped to [1, 253], 127 for amax = 0.
         With amax = m * 2^e, m in [0.5, 1): eb = 127 + e - 9 + (m > 0.875) — no division.  (For every finite bf16 / f16 magnitude this equals
         the kernels' fp32 rule, exponent of fl(amax * fl(1 / 448)) rounded up; the scaled maximum then lies in (224, 448].)

The reference is compared with torch's CPU float8_e4m3fn cast on every input it sees: that checks the reference, not the kernels.

THE CENSUS: every finite bit pattern of the storage type, both signs and both zeros.  A 32-value block carries one ANCHOR (random slot, random
sign) that fixes its scale, and 31 census values with |v| <= anchor.  Anchors are the type's values 448 * 2^j — exact maxima — with their
predecessor and successor in the type, plus what the ends of the range need: the type's largest value and its values below the smallest
448 * 2^j.  Every value sits once under its smallest anchor (results in (224, 448]: nine distinct bytes only) and once more under an exact
anchor 2 .. 2^18 times larger, which is what reaches the small codes, the e4m3 subnormals and the underflow to +-0.

Every case asserts its preconditions from the reference alone before the kernel runs.  Same layout as exact_checks.py / stream_checks.py:
written once, run on the simulator and on the product library."""
import math

import torch

from exact_checks import EXACT, INT_CAP, MANT, ROUNDS_FROM, _assert_equal, _ints, _round, _spacing
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder, glu_interleave, residual_distance
from op_checks import TD, _dev, _run
from stream_checks import GARBAGE, NAME, SENTINEL, _assert_bound, _balanced, _exact_in, _norm_formula, _signed, _slack

BITS = {abi.BF16: 0x7F80, abi.F16: 0x7C00}                            # the first non-finite magnitude pattern: patterns below it are the finite magnitudes
SCALE_RANGE = {abi.BF16: (1, 247), abi.F16: (95, 135)}                # smallest / largest scale byte a block of finite values of T can get
Q_SENTINEL, S_SENTINEL = 0xA5, 0x5A5A5A5A                             # around e4m3 bytes / scale words
MAX_SHIFT = 18

_c = torch.arange(127, dtype=torch.float64)
E4M3 = torch.where(_c < 8, _c * 2.0 ** -9, (1.0 + (_c % 8) / 8.0) * torch.exp2(torch.div(_c, 8, rounding_mode="floor") - 7.0))
assert float(E4M3[126]) == 448.0 and float(E4M3[8]) == 2.0 ** -6 and bool((E4M3[1:] > E4M3[:-1]).all())


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def e4m3_rne(v, ties=None):
    """float64 (already clamped to +-448) -> e4m3 bytes, round to nearest even by table.  ties: a dict that receives the counts of exact ties
    resolved towards zero ("down") and away from it ("up")"""
    v = v.double().cpu()
    a = v.abs()
    assert float(a.max()) <= 448.0, "the caller clamps"
    hi = torch.searchsorted(E4M3, a.contiguous()).clamp_max(126)          # first code whose magnitude is >= a
    lo = (hi - 1).clamp_min(0)
    d_lo, d_hi = a - E4M3[lo], E4M3[hi] - a                               # exact: both operands have few bits and lie within a factor of two
    tie = (d_lo == d_hi) & (hi != lo)
    code = torch.where(d_hi < d_lo, hi, lo)
    code = torch.where(tie, torch.where(hi % 2 == 0, hi, lo), code)
    code = torch.where(a == E4M3[hi], hi, code)
    if ties is not None:
        ties["down"] = ties.get("down", 0) + int((tie & (code == lo)).sum())
        ties["up"] = ties.get("up", 0) + int((tie & (code == hi)).sum())
    out = (code + torch.signbit(v).long() * 128).to(torch.uint8)
    # the reference against torch's own cast (fp32 holds every input exactly, or rounds it far below the smallest e4m3 step)
    want = v.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(out, want), f"the e4m3 reference differs from torch's cast in {int((out != want).sum())} places"
    return out


def mx_scale(amax):
    """float64 block maxima -> scale bytes (int64) by the exact rule of the module docstring"""
    m, e = torch.frexp(amax.double())
    eb = (127 + e.long() - 9 + (m > 0.875).long()).clamp(1, 253)
    return torch.where(amax == 0, torch.full_like(eb, 127), eb)


def q_ref(x, ties=None):
    """x [rows, k] (values of T as float64, k % 128 == 0) -> (bytes uint8 [rows, k], scale bytes int64 [rows, k / 32], words int32 [k / 128, rows])"""
    x = x.double().cpu()
    rows, k = x.shape
    xb = x.view(rows, k // 32, 32)
    eb = mx_scale(xb.abs().amax(-1))
    scaled = torch.ldexp(xb, (127 - eb)[..., None].expand_as(xb).to(torch.int32))
    q = e4m3_rne(scaled.clamp(-448.0, 448.0), ties).view(rows, k)
    words = (eb.view(rows, k // 128, 4) << torch.tensor([0, 8, 16, 24])).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).t().contiguous()
    return q, eb, words


def _assert_bytes(got, want, what):
    got, want = got.cpu(), want.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} differ from the reference; first at {i}: got {int(got[i]) & 0xffffffff:#x}, want {int(want[i]) & 0xffffffff:#x}")


# ---- the census ---------------------------------------------------------------------------------------------------------------------------
def _from_bits(bits, dtype):
    return bits.to(torch.int16).view(TD[dtype]).double()


def all_values(dtype):
    """every finite value of T as float64, both signs, -0 included; [2 * count]"""
    mag = torch.arange(BITS[dtype], dtype=torch.int32)
    return _from_bits(torch.cat([mag, mag - 0x8000]), dtype)


def _anchors(dtype):
    """sorted anchor magnitudes (float64) and the subset that is exactly 448 * 2^j"""
    top = BITS[dtype]
    mag = _from_bits(torch.arange(top, dtype=torch.int32), dtype)
    exact = torch.tensor([448.0 * 2.0 ** j for j in range(-160, 130)], dtype=torch.float64)
    exact = exact[(exact.to(TD[dtype]).double() == exact) & (exact <= mag[-1])]
    idx = torch.searchsorted(mag, exact)
    assert torch.equal(mag[idx], exact)
    low = torch.arange(1, int(idx[0]))                                    # the values below the smallest 448 * 2^j (pattern 0 is zero)
    pick = torch.cat([idx - 1, idx, idx + 1, low, torch.tensor([top - 1])]).clamp(1, top - 1).unique()
    return mag[pick], exact


def census_blocks(dtype, seed=0):
    """-> [blocks, 32] float64: the census of the module docstring, the special blocks last"""
    g = torch.Generator().manual_seed(seed)
    vals = all_values(dtype)
    vals = vals[torch.randperm(vals.numel(), generator=g)]
    anchors, exact = _anchors(dtype)
    amag = vals.abs()
    own = anchors[torch.searchsorted(anchors, amag)]                      # the smallest anchor >= |v|
    shift = torch.arange(vals.numel()) % MAX_SHIFT + 1                    # (the permutation above decorrelates it from the value)
    base = exact[torch.searchsorted(exact, amag).clamp_max(exact.numel() - 1)]      # the smallest exact anchor >= |v| (values beyond the largest one: dropped by `keep`)
    far = base * torch.exp2(shift.double())
    while True:                                                           # an anchor beyond the type's range: the largest shift that still exists
        over = far > exact[-1]
        if not bool(over.any()):
            break
        far = torch.where(over, far / 2, far)
    keep = (far > own) & (amag <= exact[-1])
    value = torch.cat([vals, vals[keep]])
    anchor = torch.cat([own, far[keep]])
    assert bool((value.abs() <= anchor).all())
    order = torch.argsort(anchor, stable=True)
    value, anchor = value[order], anchor[order]
    uniq, counts = torch.unique_consecutive(anchor, return_counts=True)
    nblk = (counts + 30) // 31
    first_blk = torch.cumsum(nblk, 0) - nblk
    first_val = torch.cumsum(counts, 0) - counts
    group = torch.repeat_interleave(torch.arange(uniq.numel()), counts)
    within = torch.arange(value.numel()) - first_val[group]
    blk, slot = first_blk[group] + within // 31, within % 31
    total = int(nblk.sum())
    body = torch.zeros(total, 31, dtype=torch.float64)                    # a short last block of an anchor is filled up with +0
    body[blk, slot] = value
    a_blk = torch.repeat_interleave(uniq, nblk) * (torch.randint(0, 2, (total,), generator=g) * 2 - 1).double()
    pos = torch.randint(0, 32, (total,), generator=g)
    j = torch.arange(32)[None, :]
    src = (j - (j > pos[:, None]).long()).clamp_max(30)
    blocks = torch.where(j == pos[:, None], a_blk[:, None], torch.gather(body, 1, src))
    special = [torch.zeros(32, dtype=torch.float64), -torch.zeros(32, dtype=torch.float64),
               torch.where(torch.arange(32) % 3 == 0, -0.0, 0.0).double()]
    if dtype == abi.BF16:                                                 # a maximum below 448 * 2^-126: the scale byte is clamped to 1
        sub = _from_bits(torch.randint(1, 0x0100, (32,), generator=g, dtype=torch.int32), dtype) * (torch.randint(0, 2, (32,), generator=g) * 2 - 1)
        assert 0.0 < float(sub.abs().max()) < 448.0 * 2.0 ** -126
        special.append(sub)
    return torch.cat([blocks, torch.stack(special)])


_CENSUS = {}


def census(dtype):
    """the blocks, computed once per storage type and never changed"""
    if dtype not in _CENSUS:
        _CENSUS[dtype] = census_blocks(dtype)
    return _CENSUS[dtype]


def _bit_patterns(x, dtype):
    return x.to(TD[dtype]).view(torch.int16).flatten().unique()


def check_quantize_census(lib, dtype):
    """mtx_quantize_mx (plain) on the whole census in three matrices that share the blocks: K = 1152 (37 rows, ldx / ldq padded), K = 128 (row count
    not a multiple of 16, lds > rows) and the rest as K = 128 again without padding.  Bytes and scale words: zero differing elements."""
    dev, td = _dev(lib), TD[dtype]
    blocks = census(dtype)
    what = f"quantize_mx census [{NAME[dtype]}]"
    assert _exact_in(blocks, td)
    n_a = 37 * 36
    rest = blocks[n_a:]
    half = (rest.shape[0] // 2 + 3) // 4 * 4
    parts = [blocks[:n_a].reshape(37, 1152), rest[:half].reshape(-1, 128)]
    tail = rest[half:]
    fill = -tail.shape[0] % 4
    parts.append(torch.cat([tail, blocks[:fill]]).reshape(-1, 128))
    if parts[1].shape[0] % 16 == 0:
        parts[1] = torch.cat([parts[1], blocks[:4].reshape(1, 128)])
    assert parts[1].shape[0] % 16 and sum(p.numel() for p in parts) < 500000
    # ---- preconditions, from the reference alone
    seen = torch.cat([_bit_patterns(p, dtype) for p in parts]).unique()
    assert seen.numel() == 2 * BITS[dtype], f"{what}: only {seen.numel()} of {2 * BITS[dtype]} finite bit patterns appear"
    ties = {}
    refs = [q_ref(p, ties) for p in parts]
    qa, xa = torch.cat([r[0].flatten() for r in refs]), torch.cat([p.flatten() for p in parts])
    eba = torch.cat([r[1].flatten() for r in refs])
    have = set(qa.unique().tolist())
    assert have == set(range(0x00, 0x7F)) | set(range(0x80, 0xFF)), f"{what}: byte coverage — missing {sorted((set(range(256)) - {0x7F, 0xFF}) - have)}, extra {sorted(have & {0x7F, 0xFF})}"
    assert ties["down"] >= 100 and ties["up"] >= 100, f"{what}: {ties} exact ties"
    assert 0x7E in have and 0xFE in have, f"{what}: no result of exactly +-448"
    assert int(((qa & 0x7F) < 8).logical_and((qa & 0x7F) > 0).sum()) > 0, f"{what}: no e4m3 subnormal result"
    assert int((((qa & 0x7F) == 0) & (xa != 0)).sum()) > 0, f"{what}: no non-zero input rounds to zero"
    lo, hi = SCALE_RANGE[dtype]
    assert int(eba.min()) == lo and int(eba.max()) == hi, f"{what}: scale bytes {int(eba.min())} .. {int(eba.max())}, the type reaches {lo} .. {hi}"
    assert int((eba == 127).sum()) >= 3
    print(f"{what}: {xa.numel()} elements in {sum(p.shape[0] for p in parts)} rows, ties {ties}, scale bytes {lo} .. {hi}")
    # ---- the kernel
    pb = PlanBuilder(lib, dev, dtype)
    outs = []
    for i, (p, (ldx_extra, ldq_extra, lds_extra)) in enumerate(zip(parts, ((8, 16, 3), (0, 0, 7), (0, 0, 0)))):
        rows, k = p.shape
        xb = pb.buf((rows, k + ldx_extra), td)
        xb.fill_(GARBAGE)
        xb[:, :k] = p.to(td)
        q = pb.buf((rows + 1, k + ldq_extra), torch.uint8)
        q.fill_(Q_SENTINEL)
        sc = pb.buf((k // 128, rows + lds_extra), torch.int32)
        sc.fill_(S_SENTINEL)
        pb.quantize(xb, rows, k, ldx=k + ldx_extra, q=q, scale=sc, lds=rows + lds_extra, ldq=k + ldq_extra)
        outs.append((q, sc))
    _run(pb)
    for i, (p, (q, sc), (q_want, _, w_want)) in enumerate(zip(parts, outs, refs)):
        rows, k = p.shape
        _assert_bytes(q[:rows, :k], q_want, f"{what}, matrix {i} ({rows} x {k}): e4m3 bytes")
        _assert_bytes(sc[:, :rows], w_want, f"{what}, matrix {i} ({rows} x {k}): scale words")
        assert bool((q[:rows, k:] == Q_SENTINEL).all()) and bool((q[rows:] == Q_SENTINEL).all()), f"{what}, matrix {i}: bytes outside the matrix were written"
        assert bool((sc[:, rows:] == S_SENTINEL).all()), f"{what}, matrix {i}: scale words beyond the rows were written"


def _scale_bytes(sc, rows):
    """scale plane [k / 128, lds] int32 -> int64 [rows, k / 32]"""
    w = sc.cpu()[:, :rows].t().contiguous().long()
    return torch.stack([(w >> (8 * b)) & 0xff for b in range(4)], -1).reshape(rows, -1)


# ---- per-tensor e4m3: the rotary twin and MTX_EW_V_F8T ----------------------------------------------------------------------------------
def _rope_args(pb, dtype, xt, cst, gm, rows, c, d, split, lda, ldb, eps, y8=None, ldy8=0, y8_mul=1.0, col=0, gamma_off=0):
    e = abi.EwArgs()
    e.a = e.y = xt.data_ptr() + col * xt.element_size()
    e.b, e.s = cst.data_ptr(), (gm.data_ptr() + 4 * gamma_off if gm is not None else None)
    e.n, e.h, e.w, e.c = 1, 1, rows, c
    e.lda = e.ldy = lda
    e.ldb, e.lds = ldb, 0
    e.kind, e.act, e.act_param, e.i0, e.i1, e.dtype = abi.EW_QK_NORM_ROPE, 0, eps, d, split, dtype
    if y8 is not None:
        e.y8, e.ldy8, e.y8_mul = y8.data_ptr(), ldy8, y8_mul
    pb._add(abi.OP_EW, e, "rope")


def check_rope_twin_census(lib, dtype, y8_mul=0.75):
    """The rotary kernel as a carrier: x = +-1 (mean square 1, eps = 0, no gamma), sin = 0 and cos = a census value, so that the launch stores every
    finite value of T — |v| > 448 included — and its e4m3 twin must be RNE(clamp(y * y8_mul on the q head)), saturating at 0x7E / 0xFE."""
    dev, td = _dev(lib), TD[dtype]
    what = f"rotary twin census [{NAME[dtype]}]"
    g = torch.Generator().manual_seed(3)
    d, c = 128, 256                                                       # one q head and one k head
    mags = _from_bits(torch.arange(BITS[dtype], dtype=torch.int32), dtype)
    rows = mags.numel() // (d // 2)
    assert rows * (d // 2) == mags.numel()
    cos = mags[torch.randperm(mags.numel(), generator=g)].view(rows, d // 2)
    table = torch.stack([cos, torch.zeros_like(cos)], 1)                  # [rows][2][d / 2]
    x = ((torch.randint(0, 2, (rows, c // 2), generator=g) * 2 - 1)[..., None] * torch.tensor([1, -1])).reshape(rows, c).double()      # every pair holds both signs
    x0, x1, cc, ss = x[:, 0::2], x[:, 1::2], cos.repeat(1, 2), torch.zeros(rows, d)
    y_want = torch.stack([x0 * cc - x1 * ss, x1 * cc + x0 * ss], -1).reshape(rows, c)     # the kernel's formula: it also fixes the sign of a zero
    assert _exact_in(y_want, td)
    seen = _bit_patterns(y_want, dtype)
    assert seen.numel() >= 2 * BITS[dtype] - 1, f"{what}: {seen.numel()} bit patterns"       # (every pair holds both signs; -0 only where the signs of the zero pair allow it)
    mul = torch.cat([torch.full((d,), y8_mul), torch.ones(d)]).double()
    ties = {}
    want8 = e4m3_rne((y_want * mul).clamp(-448.0, 448.0), ties)
    assert float((y_want * mul).abs().max()) > 448.0 and {0x7E, 0xFE} <= set(want8.unique().tolist()) and ties["down"] >= 100 and ties["up"] >= 100
    pb = PlanBuilder(lib, dev, dtype)
    xt, cst = pb.const(x.to(td)), pb.const(torch.stack([table, table]).float())       # the q head reads the second copy (ldb)
    y8 = pb.buf((rows + 1, c + 16), torch.uint8)
    y8.fill_(Q_SENTINEL)
    _rope_args(pb, dtype, xt, cst, None, rows, c, d, 1, c, rows * d, 0.0, y8, c + 16, y8_mul)
    _run(pb)
    _assert_equal(xt.cpu(), y_want, what + ": the 16-bit values")
    _assert_bytes(y8[:rows, :c], want8, what + ": e4m3 bytes")
    assert bool((y8[:rows, c:] == Q_SENTINEL).all()) and bool((y8[rows:] == Q_SENTINEL).all()), f"{what}: bytes outside the twin were written"


def v_f8t_ref(q):
    """e4m3 bytes [ld, heads, 128] (ld a multiple of 64) -> [heads * 128, ld] in the byte order of MTX_EW_V_F8T (include/mtx_hip.h)"""
    ld, heads, d = q.shape
    j = torch.arange(64)
    key = 32 * (j >> 5) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * ((j >> 4) & 1)
    return q.view(ld // 64, 64, heads, d)[:, key].permute(2, 3, 0, 1).reshape(heads * d, ld).contiguous()


def check_v_f8t_census(lib, dtype):
    """MTX_EW_V_F8T on every finite value of T (saturation included), a ragged key count (the reference holds zeros for the padding keys), row stride > c on the input
    and ldy8 wider than the padded rows (sentinels survive)"""
    dev, td = _dev(lib), TD[dtype]
    what = f"v_f8t census [{NAME[dtype]}]"
    g = torch.Generator().manual_seed(4)
    heads, d = 2, 128
    vals = all_values(dtype)
    rows = vals.numel() // (heads * d)
    assert rows * heads * d == vals.numel() and rows % 64, f"{what}: needs a ragged last key tile"
    v = vals[torch.randperm(vals.numel(), generator=g)].view(rows, heads * d)
    ld = (rows + 63) // 64 * 64
    ties = {}
    q = torch.zeros(ld, heads, d, dtype=torch.uint8)
    q[:rows] = e4m3_rne(v.clamp(-448.0, 448.0), ties).view(rows, heads, d)
    want = v_f8t_ref(q)
    assert {0x7E, 0xFE, 0x00, 0x80} <= set(want.unique().tolist()) and ties["down"] >= 100 and ties["up"] >= 100 and float(v.abs().max()) > 448.0
    pb = PlanBuilder(lib, dev, dtype)
    vb = pb.buf((rows, heads * d + 8), td)
    vb.fill_(GARBAGE)
    vb[:, :heads * d] = v.to(td)
    ldy8 = ld + 64
    out = pb.buf((heads * d + 1, ldy8), torch.uint8)
    out.fill_(Q_SENTINEL)
    got, ld_got = pb.v_f8t(vb, rows, heads, heads * d + 8, out=out)
    getattr(pb.ops[-1].u, abi.UNION_FIELD[abi.OP_EW]).ldy8 = ldy8
    assert ld_got == ld
    _run(pb)
    _assert_bytes(out[:heads * d, :ld], want, what)
    assert bool((out[:heads * d, ld:] == Q_SENTINEL).all()) and bool((out[heads * d:] == Q_SENTINEL).all()), f"{what}: bytes outside V^T were written"


# ---- the fused producers: MTX_QUANT_SWIGLU and the norm twin ----------------------------------------------------------------------------
def _swiglu_formula(a, b, dt):
    a, b = a.to(dt), b.to(dt)
    return a / (1.0 + torch.exp(-a)) * b


def check_swiglu_producers(lib, dtype, rows=21, hid=256, seed=0):
    """MTX_QUANT_SWIGLU with and without its 16-bit copy, and MTX_EW_SWIGLU on the same operands.  The contract: the bytes are Q_ref of the 16-bit
    values the same launch stores; those values lie within the stream_checks bound of silu(a) * b in float64.  Rows: moderate a with b across several
    binades; b = +0 over whole blocks with a < 0 (results -0, bytes 0x80, scale byte 127); a = -600 .. 600, where e^-a overflows fp32 on one
    side (the result is -0 or +0 there and a * b on the other side, never NaN)."""
    dev, td = _dev(lib), TD[dtype]
    what = f"swiglu producers {rows}x{hid}"
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(rows, hid, generator=g) * 16.0 - 8.0)
    b = _signed(g, (rows, hid), 0.5, 2.0) * torch.exp2(torch.randint(-6, 7, (rows, hid // 32), generator=g).float()).repeat_interleave(32, 1)
    ext = torch.arange(0, rows, 3)                                        # the extreme rows
    a[ext] = torch.linspace(-600.0, 600.0, hid)[None, :] * torch.where(torch.arange(ext.numel()) % 2 == 0, 1.0, -1.0)[:, None]
    b[ext] = _signed(g, (ext.numel(), hid), 0.5, 2.0)
    zero_rows, zero_cols = torch.arange(1, rows, 4), slice(64, 128)       # two whole blocks of b = +0 under negative a
    a[zero_rows, zero_cols] = -a[zero_rows, zero_cols].abs() - 0.25
    b[zero_rows, zero_cols] = 0.0
    a, b = a.to(td).double(), b.to(td).double()
    ref = _swiglu_formula(a, b, torch.float64)
    assert bool(torch.isfinite(ref).all()) and float(a.abs().max()) == 600.0
    zr = ref[zero_rows, zero_cols]
    assert bool((zr == 0).all()) and bool(torch.signbit(zr).all()), f"{what}: precondition — the zero blocks are not -0 in the reference"
    assert bool((_round(ref[ext], td)[:, :8].abs() == 0).any()), f"{what}: precondition — no underflow at a = -600"
    gap, slack, denom = _slack(_swiglu_formula(a, b, torch.float32), ref, dtype, what)

    ab = torch.cat([a, b], 1).to(td)
    R, r_off = rows + 9, 5
    lds = R + 3
    pb = PlanBuilder(lib, dev, dtype)
    abt = pb.const(ab)
    outs = []
    for with_y in (True, False):
        q = pb.buf((R, 2 * hid + 8), torch.uint8)
        q.fill_(Q_SENTINEL)
        sc = pb.buf((2 * hid // 128, lds), torch.int32)
        sc.fill_(S_SENTINEL)
        y = None
        if with_y:
            y = pb.buf((rows + 1, hid + 8), td)
            y.fill_(SENTINEL)
        pb.quantize(abt, rows, hid, ldx=2 * hid, q=q, scale=sc, row_off=r_off, lds=lds, ldq=2 * hid + 8, q_col_off=hid, swiglu_b=abt, b_off=hid, ldb=2 * hid,
                    y=y, ldy=hid + 8)
        outs.append((q, sc, y))
    va, vb = Act(abt.view(1, 1, rows, 2 * hid), 1, 1, rows, hid, 0), Act(abt.view(1, 1, rows, 2 * hid), 1, 1, rows, hid, hid)
    ew = pb.ew(abi.EW_SWIGLU, va, b=vb)
    _run(pb)
    (q1, s1, y1), (q2, s2, _) = outs
    got = y1[:rows, :hid].cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite values"
    assert bool((y1[:rows, hid:] == SENTINEL).all()) and bool((y1[rows:] == SENTINEL).all()), f"{what}: the surroundings of y were written"
    _assert_bound(got, ref, denom, gap, slack, dtype, what, "swiglu.exact.fp32_gap")
    gz = got[zero_rows, zero_cols].double()
    assert bool((gz == 0).all()) and bool(torch.signbit(gz).all()), f"{what}: silu(a < 0) * +0 must be -0"
    assert torch.equal(ew.t.view(rows, hid).cpu().view(torch.int16), got.view(torch.int16)), f"{what}: MTX_EW_SWIGLU and the quantiser's 16-bit copy differ"
    q_want, eb_want, w_want = q_ref(got.double())
    assert bool((q_want[zero_rows, zero_cols] == 0x80).all()) and bool((eb_want[zero_rows, 2:4] == 127).all())
    _assert_bytes(q1[r_off:r_off + rows, hid:2 * hid], q_want, what + ": e4m3 bytes")
    _assert_bytes(s1[hid // 128:, r_off:r_off + rows], w_want, what + ": scale words")
    for q_, s_ in ((q1, s1), (q2, s2)):
        keep = torch.ones_like(q_, dtype=torch.bool)
        keep[r_off:r_off + rows, hid:2 * hid] = False
        assert bool((q_[keep] == Q_SENTINEL).all()), f"{what}: bytes outside the target window were written"
        keep = torch.ones_like(s_, dtype=torch.bool)
        keep[hid // 128:, r_off:r_off + rows] = False
        assert bool((s_[keep] == S_SENTINEL).all()), f"{what}: scale words outside the target window were written"
    assert torch.equal(q1, q2) and torch.equal(s1, s2), f"{what}: the form without y differs from the form with y"


def check_norm_twin(lib, dtype, rows, c, seed=0):
    """mtx_norm_args.q: LayerNorm of the balanced rows of stream_checks with a modulation row per row — 1 + scale = 2^j, j = -6 .. 6, so the row maxima
    cross thirteen binades; scale = -1 and shift = 0 over one 32-column span: an all-zero block — the shift spreads the values inside a block.
    Bytes and scale words are Q_ref of the 16-bit values the launch stores; the form without y gives the same bytes; y within the stream_checks bound."""
    dev, td = _dev(lib), TD[dtype]
    what = f"norm twin {rows}x{c}"
    g = torch.Generator().manual_seed(seed)
    x, m, a = _balanced(g, rows, c)
    assert _exact_in(x, td) and c * float(x.abs().max()) < EXACT
    j = (torch.arange(rows) * 5) % 13 - 6
    ms = (torch.exp2(j.double()) - 1.0)[:, None].repeat(1, c)
    mh = (torch.rand(rows, c, generator=g, dtype=torch.float64) * 2 - 1) * torch.exp2(j.double())[:, None]
    span = slice(96, 128)
    ms[:, span], mh[:, span] = -1.0, 0.0
    ms, mh = ms.to(td), mh.to(td)
    assert _exact_in((1.0 + ms.double()), td) and len(set(j.tolist())) >= min(rows, 13) - 1
    ref = _norm_formula(x, c, 0, None, None, ms, mh, torch.float64)
    assert bool((ref[:, span] == 0).all()), f"{what}: precondition — the modulated span is not zero"
    gap, slack, denom = _slack(_norm_formula(x, c, 0, None, None, ms, mh, torch.float32), ref, dtype, what)
    R, r_off = rows + 6, 3
    lds = R + 5
    pb = PlanBuilder(lib, dev, dtype)
    xt, mst, mht = pb.const(x.to(td)), pb.const(ms), pb.const(mh)
    outs = []
    for with_y in (True, False):
        q = pb.buf((R, c), torch.uint8)
        q.fill_(Q_SENTINEL)
        s = pb.buf((c // 128, lds), torch.int32)
        s.fill_(S_SENTINEL)
        y = None
        if with_y:
            y = pb.buf((rows + 1, c + 8), td)
            y.fill_(SENTINEL)
        pb.norm(xt, y, rows, c, ldy=c + 8, eps=1e-6, kind=0, mod_scale=mst, mod_shift=mht, rows_per=1, ldmod=c, q8=(q, s), q_row_off=r_off, lds_q=lds)
        outs.append((q, s, y))
    _run(pb)
    (q1, s1, y1), (q2, s2, _) = outs
    got = y1[:rows, :c].cpu()
    assert bool((y1[:rows, c:] == SENTINEL).all()) and bool((y1[rows:] == SENTINEL).all()), f"{what}: the surroundings of y were written"
    _assert_bound(got, ref, denom, gap, slack, dtype, what, "norm.twin.fp32_gap")
    q_want, eb_want, w_want = q_ref(got.double())
    assert bool((eb_want[:, 3] == 127).all()) and int(eb_want.max()) - int(eb_want.min()) >= 10, f"{what}: the scale bytes do not spread"
    _assert_bytes(q1[r_off:r_off + rows], q_want, what + ": e4m3 bytes")
    _assert_bytes(s1[:, r_off:r_off + rows], w_want, what + ": scale words")
    for q_, s_ in ((q1, s1), (q2, s2)):
        assert bool((q_[:r_off] == Q_SENTINEL).all()) and bool((q_[r_off + rows:] == Q_SENTINEL).all()), f"{what}: bytes outside the target rows were written"
        assert bool((s_[:, :r_off] == S_SENTINEL).all()) and bool((s_[:, r_off + rows:] == S_SENTINEL).all()), f"{what}: scale words outside the target rows were written"
    assert torch.equal(q1, q2) and torch.equal(s1, s2), f"{what}: the form without y differs from the form with y"


# ---- row kernels on exact inputs ----------------------------------------------------------------------------------------------------------
def _kraft_depths(g, count, cap=14):
    """`count` code lengths with sum 2^-l = 1, none beyond `cap`: a random binary tree grown by splitting leaves"""
    assert 1 <= count <= 2 ** cap
    hist = [0] * (cap + 1)
    hist[0] = 1
    for _ in range(count - 1):
        w = torch.tensor(hist[:cap], dtype=torch.float64)
        l = int(torch.multinomial(w, 1, generator=g))
        hist[l] -= 1
        hist[l + 1] += 2
    d = torch.repeat_interleave(torch.arange(cap + 1), torch.tensor(hist))
    assert d.numel() == count and float(torch.exp2(-d.double()).sum()) == 1.0
    return d


def check_softmax_exact(lib, dtype, seed=0):
    """MTX_EW_SOFTMAX_ROWS at act_param = ln 2 on integer rows whose multiset satisfies Kraft's equality (plus an integer offset per row): every
    probability is a power of two >= 2^-14, exact in T, and the fp32 error (a few ulp of the scale, the sum and the reciprocal: below 2^-18 relative)
    is far below half a spacing of T — the output is bit-equal.  Padding columns (i0) hold the largest finite value of T and come out 0."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    big = float(torch.finfo(td).max)
    pb = PlanBuilder(lib, dev, dtype)
    checks = []
    for c, valid, rows in ((8, 0, 5), (264, 259, 6), (2056, 2050, 5)):
        n = valid or c
        what = f"softmax {rows}x{c} (valid {n}) [{NAME[dtype]}]"
        x = torch.full((rows, c), big, dtype=torch.float64)
        ref = torch.zeros(rows, c, dtype=torch.float64)
        for r in range(rows):
            d = _kraft_depths(g, n)[torch.randperm(n, generator=g)]
            if r % 2:                                                     # the maximum in the last chunk, on the last valid column
                i = int(d.argmin())
                d[[i, n - 1]] = d[[n - 1, i]]
                assert int(d[n - 1]) == int(d.min())
            off = int(torch.randint(-60, 61, (1,), generator=g))
            x[r, :n] = off - d.double()
            ref[r, :n] = torch.exp2(-(d - d.min()).double())
        ref = ref / ref.sum(-1, keepdim=True)
        assert bool((ref.sum(-1) == 1.0).all()) and _exact_in(ref, td) and _exact_in(x, td), f"{what}: precondition — inputs or probabilities are not exact in T"
        assert float(ref[ref > 0].min()) >= 2.0 ** -14 and bool((ref[:, n:] == 0).all())
        xb = pb.buf((rows, c + 8), td)
        xb.fill_(GARBAGE)
        xb[:, :c] = x.to(td)
        yb = pb.buf((rows + 1, c + 16), td)
        yb.fill_(SENTINEL)
        pb.ew(abi.EW_SOFTMAX_ROWS, Act(xb.view(1, 1, rows, c + 8), 1, 1, rows, c), out=Act(yb[:rows].view(1, 1, rows, c + 16), 1, 1, rows, c), act_param=math.log(2.0), i0=valid)
        checks.append((yb, ref, rows, c, what))
    _run(pb)
    for yb, ref, rows, c, what in checks:
        _assert_equal(yb[:rows, :c].cpu(), ref, what)
        assert bool((yb[:rows, c:] == SENTINEL).all()) and bool((yb[rows:] == SENTINEL).all()), f"{what}: the surroundings of y were written"


def check_residual_dist_exact(lib, dtype, rows, c, ld_extra=0, seed=0, expect_trips=1):
    """MTX_EW_RESIDUAL_DIST on integers: r = round_T(a - b) really rounds, |prev - r| and |prev| are integers and every workgroup's sums stay below 2^24,
    so the parts add up to the float64 sums exactly, residual_distance(parts) is their quotient, and a second launch gives the same bytes"""
    dev, td = _dev(lib), TD[dtype]
    what = f"residual_dist {rows}x{c} [{NAME[dtype]}]"
    g = torch.Generator().manual_seed(seed)
    cap, ld = INT_CAP[dtype], c + ld_extra
    a, b, prev = _ints(g, (rows, c), cap), _ints(g, (rows, c), cap), _ints(g, (rows, c), cap // 8)
    r = _round(a - b, td)
    assert float((r != a - b).double().mean()) > 0.05, f"{what}: precondition — hardly any residual needs rounding"
    dd, mm = (prev - r).abs(), prev.abs()
    chunk = torch.arange(rows * c // 8)
    part = (chunk // 256) % abi.RESDIST_PARTS                             # chunk idx belongs to workgroup (idx / 256) % PARTS (grid stride)
    trips = -(-chunk.numel() // (256 * abi.RESDIST_PARTS))
    assert trips == expect_trips, f"{what}: {trips} grid-stride trips"
    for v in (dd, mm):
        per = torch.zeros(abi.RESDIST_PARTS, dtype=torch.float64).index_add_(0, part, v.view(-1, 8).sum(1))
        assert float(per.max()) < EXACT, f"{what}: precondition — a workgroup's sum reaches {float(per.max())}"
    D, M = float(dd.sum()), float(mm.sum())
    pb = PlanBuilder(lib, dev, dtype)

    def padded(v):
        t = pb.buf((rows, ld), td)
        t.fill_(GARBAGE)
        t[:, :c] = v.to(td)
        return t
    at, bt, pt = padded(a), padded(b), pb.const(prev.to(td))
    p1 = pb.residual_dist(at, bt, pt, rows, c, ld=ld)
    p2 = pb.residual_dist(at, bt, pt, rows, c, ld=ld)
    _run(pb)
    got = p1.cpu().double()
    assert (float(got[:, 0].sum()), float(got[:, 1].sum())) == (D, M), f"{what}: sums {float(got[:, 0].sum())}, {float(got[:, 1].sum())}; want {D}, {M}"
    assert residual_distance(p1) == D / M
    assert torch.equal(p1.cpu().view(torch.int32), p2.cpu().view(torch.int32)), f"{what}: two launches differ"


# ---- MTX_EW_QK_NORM_ROPE ------------------------------------------------------------------------------------------------------------------
def _rope_ref(xn_t, tab, d):
    """xn_t [rows, heads, d] (the normalised values as rounded to T), tab [rows, 2, d / 2] -> the rotary sums [rows, heads, d], unrounded"""
    x0, x1 = xn_t[..., 0::2], xn_t[..., 1::2]
    c, s = tab[:, None, 0], tab[:, None, 1]
    return torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(xn_t.shape)


def _rope_launches(pb, dtype, buf, cst, gm, rows, hq, hk, d, fused, ld, eps, y8, ldy8, y8_mul):
    D = (hq + hk) * d
    if fused:
        _rope_args(pb, dtype, buf, cst, gm, rows, D, d, hq, ld, rows * d, eps, y8, ldy8, y8_mul)
    else:                                     # q and k heads on their own: no split, hence the first table and no y8_mul for both
        _rope_args(pb, dtype, buf, cst, gm, rows, hq * d, d, 0, ld, 0, eps, y8, ldy8, y8_mul)
        if hk == 0:
            return
        y8k = y8[:, hq * d:] if y8 is not None else None
        _rope_args(pb, dtype, buf, cst, gm, rows, hk * d, d, 0, ld, 0, eps, y8k, ldy8, y8_mul, col=hq * d, gamma_off=d)


def _rope_finish(what, dtype, buf, y8, before, ref, ref8, rows, D):
    td = TD[dtype]
    _assert_equal(buf[:rows, :D].cpu(), ref, what)
    assert torch.equal(buf[:rows, D:].cpu(), before[:rows, D:]) and torch.equal(buf[rows:].cpu(), before[rows:]), f"{what}: the v slice, the padding or the spare row changed"
    if y8 is not None:
        _assert_bytes(y8[:rows, :D], ref8, what + ": the e4m3 twin")
        assert bool((y8[:rows, D:] == Q_SENTINEL).all()) and bool((y8[rows:] == Q_SENTINEL).all()), f"{what}: bytes outside the twin were written"


def check_rope_exact(lib, dtype, rows, hq, hk, d, fused=True, twin=True, y8_mul=96.0, seed=0):
    """Head rows with a mean square of exactly 4^j (all +-2^j / a quarter +-2^(j+1) / a sixteenth +-2^(j+2), the rest 0), eps = 0: the reciprocal root
    is 2^-j; gamma = k / 8 and a table of dyadics with MANT + 2 bits (not unit length; the q heads read a second, different copy through ldb):
    the normalised value is exact in T, the rotary sums are exact in fp32 and need rounding in T.  The 16-bit output is the float64 value rounded
    once, bit for bit; the twin is RNE_e4m3(clamp(that * y8_mul on the q heads of the fused form))."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    H, D = hq + hk, (hq + hk) * d
    what = f"qk_norm_rope exact {rows}x({hq}+{hk})x{d}{'' if fused else ' separate'}"
    j = torch.randint(-2, 4, (rows, H, 1), generator=g)
    pattern = (torch.arange(rows)[:, None] + torch.arange(H)[None, :]) % 3
    rank = torch.rand(rows, H, d, generator=g).argsort(-1)
    live = rank < (d >> (2 * pattern))[..., None]                                                       # d, d / 4, d / 16 entries
    sign = (torch.randint(0, 2, (rows, H, d), generator=g) * 2 - 1).double()
    x = torch.where(live, sign * torch.exp2((j + pattern[..., None]).double()), torch.zeros(()).double())
    assert torch.equal((x * x).mean(-1, keepdim=True), torch.exp2(2.0 * j.double())), f"{what}: precondition — the mean squares are not 4^j"
    gamma = (torch.randint(1, 16, (2, d), generator=g) * (torch.randint(0, 2, (2, d), generator=g) * 2 - 1)).double() / 8.0
    bits = MANT[dtype] + 2
    tabs = (torch.randint(1, 2 ** bits, (2, rows, 2, d // 2), generator=g) * (torch.randint(0, 2, (2, rows, 2, d // 2), generator=g) * 2 - 1)).double() / 2.0 ** bits
    is_q = torch.arange(H) < hq
    xn = x * torch.exp2(-j.double()) * torch.where(is_q[None, :, None], gamma[0], gamma[1])
    assert _exact_in(x, td) and _exact_in(xn, td), f"{what}: precondition — the normalised values are not exact in T"
    o = torch.where(is_q[None, :, None], _rope_ref(xn, tabs[1 if fused else 0], d), _rope_ref(xn, tabs[0], d))
    x0, x1 = xn[..., 0::2], xn[..., 1::2]
    for t in tabs[:, :, None]:
        for prod in (x0 * t[..., 0, :], x1 * t[..., 1, :], x1 * t[..., 0, :], x0 * t[..., 1, :]):
            assert torch.equal(prod.float().double(), prod)
    assert torch.equal(o.float().double(), o), f"{what}: precondition — the rotary sums are not exact in fp32"
    ref = _round(o, td)
    share = float((ref != o).double().mean())
    assert share >= 0.20, f"{what}: precondition — only {share:.1%} of the outputs need rounding in T"
    mul = torch.where(is_q, y8_mul if fused else 1.0, 1.0).double()[None, :, None]
    ref8 = None
    if twin:
        ref8 = e4m3_rne((ref * mul).clamp(-448.0, 448.0)).view(rows, D)
        twice = int((e4m3_rne((o * mul).clamp(-448.0, 448.0)).view(rows, D) != ref8).sum())
        assert twice >= 8, f"{what}: precondition — only {twice} bytes tell the stored values from the unrounded ones"
        if fused:
            assert float((ref * mul).abs().max()) > 448.0 > float(ref.abs().max()), f"{what}: precondition — y8_mul must reach the clamp on the q heads only"
    ld = D + d + 8                                                                                      # q | k | one head of v | padding
    before = torch.full((rows + 1, ld), SENTINEL, dtype=td)
    before[:rows, :D] = x.view(rows, D).to(td)
    pb = PlanBuilder(lib, dev, dtype)
    buf, cst, gm = pb.const(before), pb.const(tabs.float()), pb.const(gamma.float().reshape(-1))
    y8 = None
    if twin:
        y8 = pb.buf((rows + 1, D + 16), torch.uint8)
        y8.fill_(Q_SENTINEL)
    _rope_launches(pb, dtype, buf, cst, gm, rows, hq, hk, d, fused, ld, 0.0, y8, D + 16, y8_mul)
    _run(pb)
    _rope_finish(f"{what} [{NAME[dtype]}]", dtype, buf, y8, before, ref.view(rows, D), ref8, rows, D)
    return share


def check_rope_general(lib, dtype, rows, hq, hk, d, seed=0, q_fold=0.1275):
    """eps = 1e-6, random magnitudes, a unit-length table in steps of 2^-12 (the q copy times q_fold): the stream_checks bound.  The kernel rounds the normalised value
    to T before the rotary product, so a float64 value next to a rounding boundary of T would make that step ambiguous: head rows are drawn until
    enough of them have every normalised value at least 2^-19 (relative) away from a boundary — decided on the float64 values alone."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    H, D = hq + hk, (hq + hk) * d
    what = f"qk_norm_rope general {rows}x({hq}+{hk})x{d}"
    eps = float(torch.tensor(1e-6, dtype=torch.float32))
    gamma = (1.0 + 0.2 * torch.randn(2, d, generator=g)).float().double()
    is_q = torch.arange(H) < hq
    gm = torch.where(is_q[:, None], gamma[0], gamma[1])                                                 # [H, d]
    pool = (torch.randn(rows * 12, H, d, generator=g) * torch.exp(torch.randn(rows * 12, H, 1, generator=g))).to(td).double()
    xn = pool / torch.sqrt((pool * pool).mean(-1, keepdim=True) + eps) * gm
    frac = torch.remainder(xn.abs() / _spacing(xn, dtype), 1.0)
    good = ((frac - 0.5).abs() > 2.0 ** -19 * 2.0 ** (MANT[dtype] + 1)).all(-1)                        # per (candidate, head): a head row is normalised on its own
    assert int(good.sum(0).min()) >= rows, f"{what}: precondition — only {int(good.sum(0).min())} of {rows * 12} candidate head rows keep clear of T's rounding boundaries"
    x = torch.stack([pool[good[:, h], h][:rows] for h in range(H)], 1)
    ang = torch.rand(rows, d // 2, generator=g, dtype=torch.float64) * 6.28
    tab = torch.stack([ang.cos(), ang.sin()], 1)
    tabs = torch.round(torch.stack([tab, tab * q_fold]) * 4096.0) / 4096.0             # twelve bits: the products with a value of T are exact in fp32, only the sum rounds

    def formula(dt):
        v = x.to(dt)
        n = v * (1.0 / torch.sqrt((v * v).sum(-1, keepdim=True) / d + eps)) * gm.to(dt)
        n = n.to(td).to(dt)
        return torch.where(is_q[None, :, None], _rope_ref(n, tabs[1].to(dt), d), _rope_ref(n, tabs[0].to(dt), d)).view(rows, D)
    ref = formula(torch.float64)
    gap, slack, denom = _slack(formula(torch.float32), ref, dtype, what)
    ld = D + d + 8
    before = torch.full((rows + 1, ld), SENTINEL, dtype=td)
    before[:rows, :D] = x.view(rows, D).to(td)
    pb = PlanBuilder(lib, dev, dtype)
    buf, cst, gmt = pb.const(before), pb.const(tabs.float()), pb.const(gamma.float().reshape(-1))
    _rope_launches(pb, dtype, buf, cst, gmt, rows, hq, hk, d, True, ld, 1e-6, None, 0, 1.0)
    _run(pb)
    assert torch.equal(buf[:rows, D:].cpu(), before[:rows, D:]) and torch.equal(buf[rows:].cpu(), before[rows:]), f"{what}: the v slice, the padding or the spare row changed"
    return _assert_bound(buf[:rows, :D].cpu(), ref, denom, gap, slack, dtype, what, "rope.general.fp32_gap")


ROPE_CASES = [
    dict(rows=37, hq=3, hk=3, d=64),
    dict(rows=21, hq=2, hk=2, d=128),
    dict(rows=33, hq=2, hk=1, d=128, fused=False),
    dict(rows=30, hq=1, hk=2, d=64, fused=False, twin=False, seed=1),
    dict(rows=6, hq=9, hk=9, d=128, seed=2),                             # c / 8 = 288 chunks: two workgroups per row group, the second one ragged
]
ROPE_CASES_GPU = [dict(rows=16389, hq=1, hk=0, d=128, fused=False, seed=3)]      # more than 4096 * 4 rows: the grid-stride loop takes a second trip


# ---- the gated epilogue of the fp8 GEMM ---------------------------------------------------------------------------------------------------
def check_gemm_glu_exact(lib, dtype, m, col0, hid, k, r=2, alpha=1.0 / 16, row_off=0, q_col_off=0, seed=0):
    """mtx_gemm_args.glu_* on integer operands in [-r, r] (exact in MX e4m3, as in exact_checks.check_gemm_exact): a and b are then the exact
    products alpha * A W^T rounded to T, and the bytes must be Q_ref(round_T(silu(a) * b)).  silu cannot be exact, so an element whose float64 value
    lies closer to a rounding boundary of T than the measured slack (stream_checks protocol) has two legitimate values in T: its byte is left
    out, and a whole block is left out when the two candidates give its scale byte two values.  Left out: at most 2 % of the elements, never
    an element of a zero block — b = 0 over whole 32-column spans (an exact zero factor gives an exact zero in any arithmetic)."""
    dev, td = _dev(lib), TD[dtype]
    what = f"gated epilogue {m}x({col0}+2x{hid})x{k}"
    g = torch.Generator().manual_seed(seed)
    n = col0 + 2 * hid
    A, W = _ints(g, (m, k), r), _ints(g, (n, k), r)
    zero_spans = torch.arange(1, hid // 32, 3)                            # b columns 32 s .. 32 s + 31 are zero: the W rows that make them are
    for s in zero_spans.tolist():
        W[col0 + hid + 32 * s:col0 + hid + 32 * s + 32] = 0.0
    assert r <= 7 and k * r * r * max(alpha, 1.0) < EXACT
    P = (A @ W.t()) * alpha
    PT = _round(P, td)
    a, b = PT[:, col0:col0 + hid], PT[:, col0 + hid:]
    assert bool(torch.isfinite(PT).all()) and float(PT.abs().max()) < 60000.0, f"{what}: precondition — a or b leaves the finite range of T"
    ref = _swiglu_formula(a, b, torch.float64)
    gap, slack, denom = _slack(_swiglu_formula(a, b, torch.float32), ref, dtype, what)
    near = _round(ref, td)
    sp = _spacing(ref, dtype)
    ambiguous = (0.5 * sp - (ref - near).abs() <= slack * denom) & (ref != 0)
    other = torch.where(ambiguous, near + torch.sign(ref - near) * sp, near)
    assert _exact_in(other, td)
    lo, hi = torch.minimum(near.abs(), other.abs()), torch.maximum(near.abs(), other.abs())
    eb_lo, eb_hi = mx_scale(lo.view(m, hid // 32, 32).amax(-1)), mx_scale(hi.view(m, hid // 32, 32).amax(-1))
    settled = eb_lo == eb_hi                                              # [m, hid / 32]
    compare = settled.repeat_interleave(32, 1) & ~ambiguous
    left_out = 1.0 - float(compare.double().mean())
    zero_block = torch.zeros(hid // 32, dtype=torch.bool)
    zero_block[zero_spans] = True
    assert bool((near.view(m, hid // 32, 32)[:, zero_block] == 0).all()) and bool(compare.view(m, hid // 32, 32)[:, zero_block].all()), f"{what}: precondition — a zero block is left out"
    assert left_out <= 0.02, f"{what}: precondition — {left_out:.2%} of the elements are left out"
    ties = {}
    q_want, eb_want, _ = q_ref(near, ties)
    assert bool((eb_want[:, zero_block] == 127).all()) and {0x00, 0x80} <= set(q_want.view(m, hid // 32, 32)[:, zero_block].unique().tolist())
    assert ties["down"] + ties["up"] > 0 and int(eb_want.max()) - int(eb_want[eb_want != 127].min()) >= 3
    print(f"{what} [{NAME[dtype]}]: fp32 gap {gap:.3g}, slack {slack:.3g}, left out {left_out:.3%}, blocks unsettled {int((~settled).sum())}")

    R, QW = row_off + m + 3, q_col_off + hid
    lds = (R + 63) // 64 * 64
    pb = PlanBuilder(lib, dev, dtype)
    aq, asc, lds_a = pb.quantize(pb.const(A.to(td)), m, k)
    wq, wsc, lds_w = pb.quantize(pb.const(W[glu_interleave(col0, hid)].contiguous().to(td)), n, k)
    q8 = pb.buf((R, QW), torch.uint8)
    q8.fill_(Q_SENTINEL)
    sc = pb.buf((QW // 128, lds), torch.int32)
    sc.fill_(S_SENTINEL)
    cbuf = pb.buf((m, n), td, zero=True) if col0 else None
    pb.gemm(aq, wq, m, n, k, out=cbuf, f8=(asc, lds_a, wsc, lds_w, 0, 0), alpha=alpha, flags=abi.GEMM_FORCE_TILE256, glu=(q8, sc, QW, lds, col0, row_off, q_col_off))
    _run(pb)
    got_q = q8[row_off:row_off + m, q_col_off:].cpu()
    got_eb = _scale_bytes(sc[q_col_off // 128:, row_off:], m)
    bad = (got_eb != eb_want) & settled
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} scale bytes differ from the reference; first at {tuple(bad.nonzero()[0].tolist())}"
    bad = (got_q != q_want) & compare
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(compare.sum())} compared e4m3 bytes differ from the reference; first at {tuple(bad.nonzero()[0].tolist())}"
    keep = torch.ones_like(q8, dtype=torch.bool)
    keep[row_off:row_off + m, q_col_off:] = False
    assert bool((q8[keep] == Q_SENTINEL).all()), f"{what}: bytes outside the target window were written"
    keep = torch.ones_like(sc, dtype=torch.bool)
    keep[q_col_off // 128:, row_off:row_off + m] = False
    assert bool((sc[keep] == S_SENTINEL).all()), f"{what}: scale words outside the target window were written"
    if col0:
        _assert_equal(cbuf[:, :col0].cpu(), PT[:, :col0], what + ": the ungated columns")


# ---- the activation + MX-fp8 epilogue of the fp8 GEMM ---------------------------------------------------------------------------------------
def gemm256_act_instantiation(act):
    """with_gemm256_act (csrc/gemm.hip) restated: the ACT template argument of the 256-tile kernels; -1 = the runtime switch"""
    return act if act in (abi.ACT_NONE, abi.ACT_SILU, abi.ACT_GELU_TANH) else -1


def _act_formula(v, act, dt, slope):
    v = v.to(dt)
    if act == abi.ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    if act == abi.ACT_GELU_TANH:
        return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))
    if act == abi.ACT_RELU:
        return v.clamp_min(0.0)
    if act == abi.ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    assert act == abi.ACT_NONE
    return v


ACTQ_EXACT_ACTS = (abi.ACT_NONE, abi.ACT_RELU, abi.ACT_LEAKY)
ACTQ_SLOPE = 2.0 ** -2


def check_gemm_actq_exact(lib, dtype, m, n, k, act, instantiation, row_off=0, q_col_off=0, seed=0):
    """mtx_gemm_args.actq_* (gemm256_f8_actq_kernel<T, ACT>) against Q_ref(round_T(act(alpha acc + bias))) — a reference that shares no
    arithmetic with the kernel, where kontext_fp8_checks.check_gemm_f8_actq compares with mtx_quantize_mx.  Integer operands in [-r, r],
    r <= 7, times a power of two per row of A (exact in MX e4m3: the block scale is a power of two; the factors spread the scale bytes), an
    integer bias.  NONE, RELU and LEAKY with slope 2^-2 give h exactly: every byte and every scale byte is compared.  SILU and GELU_TANH
    take the slack protocol of check_gemm_glu_exact unchanged (cap: 2 % left out, never an element of a zero block) on a narrower operand
    range, so that act() sees |t| of a few units.  A zero block: 32 zero rows of W with a zero bias.  `instantiation` = the ACT the case
    is meant for.  Returns (left-out share, rounding share)."""
    dev, td = _dev(lib), TD[dtype]
    assert gemm256_act_instantiation(act) == instantiation, f"act {act} runs gemm256_f8_actq_kernel<T, {gemm256_act_instantiation(act)}>, the case is meant for {instantiation}"
    assert n % 256 == 0 and k % 128 == 0
    exact = act in ACTQ_EXACT_ACTS
    what = f"activation + MX-fp8 epilogue {m}x{n}x{k} act {act}"
    g = torch.Generator().manual_seed(seed)
    if exact:
        from exact_checks import operand_range
        r, alpha = operand_range(dtype, k, cap=7)
        bias_cap = INT_CAP[dtype]
    elif act == abi.ACT_SILU:
        r, alpha, bias_cap = 2, 2.0 ** -4, 2
    else:                                                     # the tanh form cancels in fp32 for t below -4: a narrower range keeps the slack sharp
        r, alpha, bias_cap = 1, 2.0 ** -(4 + (k > 128)), 1
    factor = torch.exp2(-torch.randint(0, 4, (m, 1), generator=g).double())          # 1, 1/2, 1/4, 1/8 per row
    A, W = _ints(g, (m, k), r) * factor, _ints(g, (n, k), r)
    bias = _ints(g, (n,), bias_cap)
    zero_spans = torch.arange(1, n // 32, 3)
    for s in zero_spans.tolist():
        W[32 * s:32 * s + 32] = 0.0
        bias[32 * s:32 * s + 32] = 0.0
    assert r <= 7 and _exact_in(A, td) and (k * r * r * max(alpha, 1.0) + bias_cap) * 8 < EXACT, f"{what}: precondition — partial sums are not exact in fp32"
    t = (A @ W.t()) * alpha + bias
    ref = _act_formula(t, act, torch.float64, ACTQ_SLOPE)
    near = _round(ref, td)
    assert bool(torch.isfinite(near).all()) and float(near.abs().max()) < 60000.0, f"{what}: precondition — h leaves the finite range of T"
    nb = n // 32
    if exact:
        compare = torch.ones(m, n, dtype=torch.bool)
        settled = torch.ones(m, nb, dtype=torch.bool)
        grid = factor * torch.where(ref < 0, ACTQ_SLOPE if act == abi.ACT_LEAKY else 1.0, 1.0)      # every h of a row is a multiple of it
        assert bool((ref / grid == torch.round(ref / grid)).all())
        share = float((ref.abs() / grid >= ROUNDS_FROM[dtype]).double().mean())
        assert share >= 0.20, f"{what}: precondition — only {share:.1%} of the outputs lie where the storage type rounds multiples of the row's grid"
    else:
        gap, slack, denom = _slack(_act_formula(t, act, torch.float32, ACTQ_SLOPE), ref, dtype, what)
        sp = _spacing(ref, dtype)
        ambiguous = (0.5 * sp - (ref - near).abs() <= slack * denom) & (ref != 0)
        other = torch.where(ambiguous, near + torch.sign(ref - near) * sp, near)
        assert _exact_in(other, td)
        lo, hi = torch.minimum(near.abs(), other.abs()), torch.maximum(near.abs(), other.abs())
        settled = mx_scale(lo.view(m, nb, 32).amax(-1)) == mx_scale(hi.view(m, nb, 32).amax(-1))
        compare = settled.repeat_interleave(32, 1) & ~ambiguous
        share = None
    left_out = 1.0 - float(compare.double().mean())
    zero_block = torch.zeros(nb, dtype=torch.bool)
    zero_block[zero_spans] = True
    assert bool((near.view(m, nb, 32)[:, zero_block] == 0).all()) and bool(compare.view(m, nb, 32)[:, zero_block].all()), f"{what}: precondition — a zero block is left out"
    assert left_out <= 0.02, f"{what}: precondition — {left_out:.2%} of the elements are left out"
    ties = {}
    q_want, eb_want, _ = q_ref(near, ties)
    assert bool((eb_want[:, zero_block] == 127).all()) and set(q_want.view(m, nb, 32)[:, zero_block].unique().tolist()) <= {0x00, 0x80}
    assert ties["down"] > 0 and ties["up"] > 0, f"{what}: precondition — ties in both directions, got {ties}"
    assert len(eb_want[eb_want != 127].unique()) >= 3, f"{what}: precondition — the scale bytes span fewer than 3 values"
    print(f"{what} [{NAME[dtype]}]: left out {left_out:.3%}, blocks unsettled {int((~settled).sum())}, rounding share {share if share is None else round(share, 3)}, ties {ties}, "
          f"scale bytes {int(eb_want[eb_want != 127].min())}..{int(eb_want.max())}")

    R, QW = row_off + m + 3, q_col_off + n + 128          # three spare rows below, one spare 128-byte group to the right
    lds = (R + 63) // 64 * 64
    pb = PlanBuilder(lib, dev, dtype)
    aq, asc, lds_a = pb.quantize(pb.const(A.to(td)), m, k)
    wq, wsc, lds_w = pb.quantize(pb.const(W.to(td)), n, k)
    q8 = pb.buf((R, QW), torch.uint8)
    q8.fill_(Q_SENTINEL)
    sc = pb.buf((QW // 128, lds), torch.int32)
    sc.fill_(S_SENTINEL)
    c = pb.gemm(aq, wq, m, n, k, bias=pb.const(bias.float()), act=act, alpha=alpha, f8=(asc, lds_a, wsc, lds_w, 0, 0), actq=(q8, sc, QW, lds, row_off, q_col_off))
    assert c is None
    getattr(pb.ops[-1].u, abi.UNION_FIELD[abi.OP_GEMM]).act_param = ACTQ_SLOPE
    _run(pb)
    got_q = q8[row_off:row_off + m, q_col_off:q_col_off + n].cpu()
    got_eb = _scale_bytes(sc[q_col_off // 128:(q_col_off + n) // 128, row_off:], m)
    bad = (got_eb != eb_want) & settled
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} scale bytes differ from the reference; first at {tuple(bad.nonzero()[0].tolist())}"
    bad = (got_q != q_want) & compare
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(compare.sum())} compared e4m3 bytes differ from the reference; first at {tuple(bad.nonzero()[0].tolist())}"
    keep = torch.ones_like(q8, dtype=torch.bool)
    keep[row_off:row_off + m, q_col_off:q_col_off + n] = False
    assert bool((q8[keep] == Q_SENTINEL).all()), f"{what}: bytes outside the target window were written"
    keep = torch.ones_like(sc, dtype=torch.bool)
    keep[q_col_off // 128:(q_col_off + n) // 128, row_off:row_off + m] = False
    assert bool((sc[keep] == S_SENTINEL).all()), f"{what}: scale words outside the target window were written"
    return left_out, share


ACTQ_CASES = [dict(m=300, n=256, k=384, row_off=5, q_col_off=128), dict(m=260, n=512, k=128)]
ACTQ_ACTS = [(abi.ACT_NONE, abi.ACT_NONE), (abi.ACT_RELU, -1), (abi.ACT_LEAKY, -1), (abi.ACT_SILU, abi.ACT_SILU), (abi.ACT_GELU_TANH, abi.ACT_GELU_TANH)]


# ---- attention with MX fp8 output ---------------------------------------------------------------------------------------------------------
def check_attention_selector(lib, dtype, sq, sk, heads=2, L=192.0, seed=0):
    """mtx_attn_args.q8 (pre-scaled q, d = 128): q rows are +-one-hot in channel c; key j holds +L at channel j for j < 128, -L at channel j - 128 for
    128 <= j < 256, later keys are 0.  The selected key's base-2 logit is L above every other one and 2^-L is 0 in fp32: every query returns ONE
    v row, exactly — from the second half of the keys for every other query, so its running maximum moves late.  The v rows are blocks of the
    census (zero blocks, anchors, ties; -0 written as +0: a sum has no signed zero to keep).  The 16-bit output equals the selected rows, the q8
    form's bytes and scale words equal Q_ref of them."""
    dev, td = _dev(lib), TD[dtype]
    d, D = 128, heads * 128
    what = f"attention selector {sq}x{sk}, {heads} heads [{NAME[dtype]}]"
    assert sk >= 256 and L >= 160.0 and _exact_in(torch.tensor([L]), td) and float(torch.tensor(L).to(torch.float8_e4m3fn)) == L
    g = torch.Generator().manual_seed(seed)
    blocks = census(dtype)
    amax = blocks.abs().amax(-1)
    pool = blocks[(amax == 0) | ((amax >= 2.0 ** -60) & (amax <= 2.0 ** 40))] + 0.0                      # (-0 + 0 = +0); sk * 2^40 * 2^-L rounds to 0 in T: the float64 reference can return a zero of v
    pick = torch.randperm(pool.shape[0], generator=g).repeat(-(-sk * heads * 4 // pool.shape[0]))[:sk * heads * 4]      # (bf16: fewer such blocks than v rows, some come twice)
    v = pool[pick].view(sk, heads, d)
    r, h = torch.arange(sq)[:, None], torch.arange(heads)[None, :]
    sel = (r * 37 + h * 11) % 256                                         # the key a query selects: every key for 256 consecutive queries
    assert all(len(set(sel[:, i].tolist())) == 256 for i in range(heads)) and sq >= 256
    q = torch.zeros(sq, heads, d, dtype=torch.float64)
    q.scatter_(2, (sel % 128)[..., None], torch.where(sel < 128, 1.0, -1.0).double()[..., None])
    kk = torch.zeros(sk, heads, d, dtype=torch.float64)
    j = torch.arange(128)
    kk[j, :, j], kk[128 + j, :, j] = L, -L
    want = torch.stack([v[sel[:, i], i] for i in range(heads)], 1)        # [sq, heads, d]
    for i in range(heads):                                                # the float64 softmax, rounded once, is the selected row
        logits = q[:, i] @ kk[:, i].t()
        assert bool((logits.amax(1) == L).all()) and bool(((logits == L).sum(1) == 1).all()) and float(logits.topk(2, 1).values[:, 1].max()) == 0.0
        p = torch.exp2(logits - L)
        ref = (p @ v[:, i]) / p.sum(1, keepdim=True)
        assert torch.equal(_round(ref, td), want[:, i]), f"{what}: precondition — round_T(reference) is not the selected row"
    assert float(torch.tensor(-L, dtype=torch.float32).exp2()) == 0.0
    ties = {}
    q_want, eb_want, w_want = q_ref(want.view(sq, D), ties)
    have = set(q_want.unique().tolist())
    assert ties["down"] >= 100 and ties["up"] >= 100 and {0x7E, 0xFE} <= have and int((eb_want == 127).sum()) > 0, f"{what}: precondition — ties {ties}, zero blocks {int((eb_want == 127).sum())}"
    pb = PlanBuilder(lib, dev, dtype)
    qt, kt, vt = pb.const(q.view(1, sq, heads, d).to(td)), pb.const(kk.view(1, sk, heads, d).to(td)), pb.const(v.view(1, sk, heads, d).to(td))
    strides = ((sq * D, D, d), (sk * D, D, d), (sk * D, D, d), (sq * D, D, d))
    o = pb.buf((sq + 1, D), td)
    o.fill_(SENTINEL)
    pb.attention(qt, kt, vt, o, 1, heads, sq, sk, d, *strides, 1.0, q_prescaled=True)
    lds = (sq + 63) // 64 * 64
    q8 = pb.buf((sq + 1, D + 128), torch.uint8)
    q8.fill_(Q_SENTINEL)
    sc = pb.buf(((D + 128) // 128, lds), torch.int32)
    sc.fill_(S_SENTINEL)
    pb.attention(qt, kt, vt, None, 1, heads, sq, sk, d, *strides, 1.0, q_prescaled=True, q8=(q8, sc, D + 128, lds, 128))
    _run(pb)
    _assert_equal(o[:sq].cpu(), want.view(sq, D), what + ": the 16-bit output")
    assert bool((o[sq:] == SENTINEL).all())
    _assert_bytes(q8[:sq, 128:], q_want, what + ": e4m3 bytes")
    _assert_bytes(sc[1:, :sq], w_want, what + ": scale words")
    assert bool((q8[:sq, :128] == Q_SENTINEL).all()) and bool((q8[sq:] == Q_SENTINEL).all()), f"{what}: bytes outside the target window were written"
    assert bool((sc[0] == S_SENTINEL).all()) and bool((sc[1:, sq:] == S_SENTINEL).all()), f"{what}: scale words outside the target window were written"


ATTN_LONG_VARIANTS = ("mma32", "d", "q8", "q8d", "k8", "k8q", "k8v8q")


def check_attention_selector_below(lib, dtype, variant, sq=1024, sk=330, seed=0):
    """One case per variant of the long-sequence kernel (the table in csrc/attn_mma32_body.inc; `mma32` is attn_mma32_kernel without pre-scaled q — with
    it the launcher takes that kernel only for an output that is not 16-byte aligned), at the smallest shape that reaches it: one head, five full key
    tiles and a ragged one of 10.
    Channel c selects key (c * (sk - 1)) // 127 — keys of every tile, the last valid key among them: that key holds -16 at channel c, every other
    key -112, and q rows are one-hot.  The selected logit is 96 (base 2) above the rest: the other keys weigh 2^-96, their sum (< 2^-96 * sk * 448)
    is below half an fp32 ulp of the smallest nonzero e4m3 magnitude (2^-9), so the output row IS the selected v row, none of whose values is
    zero.  But every real logit lies BELOW 0, the score of a key that does not exist: one key past the ragged end admitted outweighs the selected one
    2^16 times.  A query whose key lies in a later tile moves its maximum there, by 96, far past every stale-maximum limit: without the refill of the
    accumulators' start value the earlier tiles keep weight 1, and without the rescale of O^T their rows stay in the sum.  v holds e4m3 values
    (exact in every operand type of every variant); the MX fp8 variants must give Q_ref of the selected rows: bytes in the order of the two
    half-blocks, scale bytes rounded up.  (All pre-scaled logits stay above -128: the first tile's 2^-maximum must be finite in fp32.)"""
    assert variant in ATTN_LONG_VARIANTS and sq >= 1024 and 256 <= sk < 2 * 256
    dev, td = _dev(lib), TD[dtype]
    d = 128
    what = f"attention selector below zero {sq}x{sk} [{variant}, {NAME[dtype]}]"
    prescaled, out8 = variant not in ("mma32", "q8"), variant in ("q8", "q8d", "k8q", "k8v8q")
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 256, (sk, d), generator=g, dtype=torch.uint8)
    bits[((bits & 0x7F) == 0x7F) | ((bits & 0x7F) == 0)] = 0x38           # no NaN, no zero
    v = bits.view(torch.float8_e4m3fn).double() + 0.0
    c = torch.arange(d)
    key_of = (c * (sk - 1)) // (d - 1)
    assert int(key_of[-1]) == sk - 1 and len(set(key_of.tolist())) == d and int((key_of >= sk // 64 * 64).sum()) >= 2 and int((key_of < 64).sum()) >= 2
    kk = torch.full((sk, d), -112.0, dtype=torch.float64)
    kk[key_of, c] = -16.0
    chan = (torch.arange(sq) * 37) % d
    q = torch.zeros(sq, d, dtype=torch.float64)
    q[torch.arange(sq), chan] = 1.0 if prescaled else 256.0              # not pre-scaled: the kernel multiplies by log2(e) / sqrt(128) = 0.1275
    want = v[key_of[chan]]
    logits = (q @ kk.t()) * (1.0 if prescaled else math.log2(math.e) / math.sqrt(d))
    top = logits.topk(2, 1).values
    assert float(top[:, 0].max()) <= -16.0 and float((top[:, 0] - top[:, 1]).min()) >= 96.0 and (not prescaled or float(logits.min()) > -128.0)
    assert torch.equal(logits.argmax(1), key_of[chan])
    pb = PlanBuilder(lib, dev, dtype)
    vt = pb.const(v.view(1, sk, 1, d).to(td))
    kw = dict(q_prescaled=prescaled)
    if variant in ("k8", "k8q", "k8v8q"):
        rows = max(sq, sk)
        packed = torch.zeros(rows, 2 * d, dtype=torch.uint8)              # [row][q bytes | k bytes]: the layout the rotary kernel leaves
        packed[:sq, :d] = q.float().to(torch.float8_e4m3fn).view(torch.uint8)
        packed[:sk, d:] = kk.float().to(torch.float8_e4m3fn).view(torch.uint8)
        qt = kt = pb.buf((1, rows, 1, d), td, zero=True)                  # q / k are not read in this form
        strides = ((rows * d, d, d), (rows * d, d, d), (sk * d, d, d), (sq * d, d, d))
        kw["qk_f8"] = (pb.const(packed), 0, d, 2 * d, 0)
        if variant == "k8v8q":
            kw["pv_f8"] = pb.v_f8t(vt, sk, 1, d)
    else:
        qt, kt = pb.const(q.view(1, sq, 1, d).to(td)), pb.const(kk.view(1, sk, 1, d).to(td))
        strides = ((sq * d, d, d), (sk * d, d, d), (sk * d, d, d), (sq * d, d, d))
    if out8:
        lds = (sq + 63) // 64 * 64
        q8 = pb.buf((sq + 1, d), torch.uint8)
        q8.fill_(Q_SENTINEL)
        sc = pb.buf((1, lds), torch.int32)
        sc.fill_(S_SENTINEL)
        pb.attention(qt, kt, vt, None, 1, 1, sq, sk, d, *strides, 1.0 / math.sqrt(d), q8=(q8, sc, d, lds, 0), **kw)
        _run(pb)
        q_want, _, w_want = q_ref(want)
        _assert_bytes(q8[:sq], q_want, what + ": e4m3 bytes")
        _assert_bytes(sc[:, :sq], w_want, what + ": scale words")
        assert bool((q8[sq:] == Q_SENTINEL).all()) and bool((sc[:, sq:] == S_SENTINEL).all()), f"{what}: written outside the target window"
    else:
        o = pb.buf((sq + 1, d), td)
        o.fill_(SENTINEL)
        pb.attention(qt, kt, vt, o, 1, 1, sq, sk, d, *strides, 1.0 / math.sqrt(d), **kw)
        _run(pb)
        _assert_equal(o[:sq].cpu(), want, what)
        assert bool((o[sq:] == SENTINEL).all()), f"{what}: written outside the output rows"

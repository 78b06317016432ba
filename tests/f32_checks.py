"""Exact-input checks of the fp32 kernels of csrc/f32ops.hip (attention, LayerNorm, the element-wise kernel, the two conversions; the GEMM is in
exact_checks.check_gemm_f32_exact) and of RCAN's channel attention (ca_kernel / ca_split_kernel of csrc/elementwise.hip) against float64 references.

Three kinds of cases, as in exact_checks.py and stream_checks.py:
  BITWISE — operands chosen so that every intermediate is exact in fp32 in any order and the output is one known value (at most ONE correctly
      rounded fp32 operation away from integers): the kernel's values must equal the float64 reference rounded once, zero differing elements.
  CENSUS — one carrier per position (a key, a 16-byte chunk), so that a lost or doubled one moves a whole output.
  GENERAL — random operands.  The bound is per element and measured, not chosen: the same formula evaluated with plain torch fp32 ops on the same
      inputs, its largest distance to float64 in units of max(|ref|, row max |ref| * 2^-8), times four (a kernel may sum in another order), at
      least 2^-20; plus half an fp32 spacing of the reference (the one rounding of the store).  A case fails BEFORE it looks at the kernel unless
      that slack is below 2^-10: the bound of every element then stays below 2^-10 of its row's largest value, what one term lost from a sum of 1024
      equal ones moves (averages of 1100 random values cancel: their small elements measure a slack of 2e-4, the norms 1e-6).

Every case asserts its preconditions from the reference alone, puts its outputs into sentinel-filled buffers (padding columns and a spare row or image
behind the output must come back untouched) and fills the unused columns of its inputs with garbage.  Written once, run on the simulator
(test_ops_sim.py) and on the product library (test_ops_gpu.py)."""
import math

import torch
import torch.nn.functional as F

import parity_log
from exact_checks import EXACT, ROUNDS_FROM, _assert_equal, _assert_rounding_share, _ints, _round
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _run, _sync
from stream_checks import EPS, GARBAGE, NAME, ROW_FLOOR, SENTINEL, SLACK_FLOOR, _Ew, _assert_bound, _balanced, _nonzero_ints, _signed

SHARP32 = 2.0 ** -10            # the largest slack a general case may measure (module docstring)
_FIGURES = {}


def _note(name, **figures):
    """the largest figures of the session under `name` (parity_log.record keeps six decimals of a float: figures go in as text)"""
    f = _FIGURES.setdefault(name, {})
    for k, v in figures.items():
        f[k] = max(f.get(k, 0.0), float(v))
    parity_log.record(name, **{k: f"{v:.3e}" for k, v in f.items()})


def _slack32(f32, ref, what):
    """stream_checks._slack for an fp32 kernel: the gap of the plain fp32 formula, the slack that follows and the bound's denominator"""
    denom = torch.maximum(ref.abs(), ref.abs().amax(dim=-1, keepdim=True) * ROW_FLOOR)
    assert float(denom.min()) > 0.0, f"{what}: a row of zeros has no scale"
    gap = float(((f32.double() - ref).abs() / denom).max())
    slack = max(4.0 * gap, SLACK_FLOOR)
    assert slack < SHARP32, f"{what}: precondition — the fp32 formula is {gap:.3g} from float64, slack {slack:.3g} >= {SHARP32:.3g}: these inputs are not sharp"
    return gap, slack, denom


def _assert_bound32(got, ref, denom, gap, slack, what, name):
    """stream_checks._assert_bound for an fp32 output; also prints and records the kernel's error in the units of the gap"""
    rel = float(((got.double() - ref).abs() / denom).max())
    print(f"{what}: kernel error {rel:.3g} in the units of the fp32 gap")
    _note(name + ".kernel", kernel_err_rel=rel)
    return _assert_bound(got, ref, denom, gap, slack, abi.F32, what, name)


def _untouched(whole, rows, c0, c, what):
    """whole [rows + spare, ld]: everything but columns [c0, c0 + c) of the first `rows` rows still holds the sentinel"""
    keep = torch.ones(whole.shape[-1], dtype=torch.bool, device=whole.device)
    keep[c0:c0 + c] = False
    assert bool((whole[:rows][:, keep] == SENTINEL).all()), f"{what}: columns outside the output slice were written"
    assert whole.shape[0] > rows and bool((whole[rows:] == SENTINEL).all()), f"{what}: written beyond the last output row"


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def attn_f32_on_rows_kernel(sq, sk, d):
    """the dispatch rule of attn_f32_launch (csrc/f32ops.hip): a lane per query (attn_f32_rows_kernel) or a wave per query (attn_f32_kernel)"""
    return sk <= 32 and sq >= 64 and d <= 32


ATTN_TIE_CASES = [      # (batch, heads, sq, sk, d, the kernel the case is meant for)
    (2, 3, 5, 70, 16, "wave"), (1, 2, 130, 3, 32, "rows"), (1, 1, 2, 64, 8, "wave"), (3, 2, 300, 9, 16, "rows"),
    (1, 2, 7, 129, 64, "wave"), (1, 1, 64, 32, 8, "rows"), (1, 1, 3, 1, 16, "wave"), (1, 2, 65, 33, 32, "wave"),
    (1, 2, 5, 63, 16, "wave"), (2, 1, 6, 65, 32, "wave"),                                             # one key short of / beyond a full round of the 64 lanes
    (1, 1, 63, 32, 16, "wave"), (1, 1, 64, 32, 16, "rows"), (1, 1, 63, 33, 32, "wave"), (1, 1, 64, 33, 32, "wave"),      # both sides of sk <= 32 && sq >= 64
    (1, 1, 64, 9, 64, "wave"),                                                                        # ... && d <= 32
]
ATTN_CENSUS_CASES = [(1, 2, 5, 70, 16, "wave"), (2, 1, 70, 9, 32, "rows"), (1, 1, 3, 129, 64, "wave"), (1, 1, 66, 32, 8, "rows"), (1, 1, 4, 200, 8, "wave")]


def _attn_launch(pb, q, k, v, scale):
    """q [b, sq, heads, d], k / v [b, sk, heads, d] (float64, exact in fp32).  q and k are the two halves of one fused projection (k_off) whose
    other rows hold garbage, v has a wider row stride, the output is a column slice (o_off, wider strides) of a sentinel-filled buffer with one
    spare row behind it.  -> a function to call after the run: it checks the surroundings and returns the output [b, sq, heads, d]"""
    b, sq, heads, d = q.shape
    sk, dm, rows = k.shape[1], heads * d, max(sq, k.shape[1])
    assert bool((q.float().double() == q).all()) and bool((k.float().double() == k).all()) and bool((v.float().double() == v).all())
    qk = torch.full((b, rows, 2 * dm), GARBAGE, dtype=torch.float32)
    qk[:, :sq, :dm], qk[:, :sk, dm:] = q.reshape(b, sq, dm).float(), k.reshape(b, sk, dm).float()
    ldv, ldo, o_off = dm + 8, dm + 16, 8
    vb = torch.full((b, sk, ldv), GARBAGE, dtype=torch.float32)
    vb[..., :dm] = v.reshape(b, sk, dm).float()
    whole = pb.buf((b * sq + 1, ldo), torch.float32)
    whole.fill_(SENTINEL)
    qkt = pb.const(qk)
    pb.attention(qkt, qkt, pb.const(vb), whole, b, heads, sq, sk, d, (rows * 2 * dm, 2 * dm, d), (rows * 2 * dm, 2 * dm, d), (sk * ldv, ldv, d),
                 (sq * ldo, ldo, d), scale, k_off=dm, o_off=o_off)

    def result(what):
        _untouched(whole, b * sq, o_off, dm, what)
        return whole[:b * sq, o_off:o_off + dm].cpu().reshape(b, sq, heads, d)
    return result


def _assert_kernel(case, what):
    b, heads, sq, sk, d, kernel = case
    rule = "rows" if attn_f32_on_rows_kernel(sq, sk, d) else "wave"
    assert rule == kernel, f"{what}: the case is meant for the {kernel} kernel, the dispatch rule gives the {rule} kernel"


def check_attn_f32_ties(lib, late_max=False, seed=0):
    """attn_f32_kernel<8|16|32|64> and attn_f32_rows_kernel<8|16|32>, BITWISE.  q rows are 4 * one-hot, scale = 0.25, k holds 0 / -512 / -1024, so
    every score is 0, -512 or -1024 and, the maximum subtracted, expf returns exactly 1 or exactly 0 (asserted for torch's fp32 exp; a kernel whose
    expf(-512) is not 0 fails the comparison).  v holds integers in [-64, 64]: the output is (sum of v over the keys tied at the maximum) / (their
    number), exact integers below 2^24 and ONE fp32 division, which HIP rounds correctly by default (the Makefile sets no fast-math flag) — and
    float64 division rounded to fp32 equals the correctly rounded fp32 division (53 >= 2 * 24 + 2).  Zero differing elements.
    Column (batch, head, channel) of k holds its upper level at 1, 3, 8, 7, 2, 11 or all of its keys, so the tie sets of the family cover those
    sizes.  late_max: the first three quarters of the keys are clamped to at most -512 — where a key of the last quarter holds 0 the running
    maximum moves late and corr = expf(-512) = 0 has to erase what was accumulated.
    Preconditions over the family (a case with one key has tie sets of one alone): tie sets of size 1 and of 8 or more; 20 % of the outputs are no integers; late_max: 20 % of the rows have their maximum in the last quarter alone."""
    g = torch.Generator().manual_seed(seed + (100 if late_max else 0))
    dev = _dev(lib)
    assert float(torch.exp(torch.tensor(-512.0))) == 0.0 and float(torch.exp(torch.tensor(0.0))) == 1.0
    pb = PlanBuilder(lib, dev, abi.F32)
    checks, sizes, fractional, moved = [], [], [], []
    for case in ATTN_TIE_CASES:
        b, heads, sq, sk, d, _ = case
        what = f"fp32 attention, tie sets{' (late maximum)' if late_max else ''} {b}x{heads}x{sq}x{sk} d{d}"
        _assert_kernel(case, what)
        assert sk * 64 < EXACT
        hot = torch.randint(0, d, (b, sq, heads), generator=g)
        q = torch.zeros(b, sq, heads, d, dtype=torch.float64)
        q.scatter_(3, hot[..., None], 4.0)
        col = torch.arange(b * heads * d).view(b, 1, heads, d) + seed
        top = torch.tensor([1, 3, 8, 7, 2, 11, sk])[col % 7].clamp(1, sk)                          # keys at the upper level of this column
        upper = torch.where(col % 5 == 4, -512.0, 0.0).double()
        lower = torch.where(upper < 0, -1024.0, -512.0 * torch.randint(1, 3, (b, sk, heads, d), generator=g)).double()
        k = torch.where(torch.rand(b, sk, heads, d, generator=g).argsort(dim=1) < top, upper, lower)
        if late_max:
            k[:, :sk * 3 // 4].clamp_(max=-512.0)
        v = _ints(g, (b, sk, heads, d), 64)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.25
        mx = s.amax(dim=-1, keepdim=True)
        assert bool(((s == mx) | (s <= mx - 512.0)).all()) and set(s.unique().tolist()) <= {0.0, -512.0, -1024.0}
        tie = (s == mx).double()
        count = tie.sum(-1)                                                                            # [b, heads, sq]
        ref = (torch.einsum("bhqk,bkhd->bqhd", tie, v) / count.permute(0, 2, 1)[..., None]).float().double()
        sizes += count.flatten().tolist()
        fractional.append(ref != ref.round())
        if late_max and sk >= 4:
            moved.append((s[..., sk * 3 // 4:].amax(-1) > s[..., :sk * 3 // 4].amax(-1)).flatten())
        checks.append((what, _attn_launch(pb, q, k, v, 0.25), ref))
    share = float(torch.cat([f.flatten() for f in fractional]).double().mean())
    assert 1.0 in sizes and max(sizes) >= 8.0 and share >= 0.20, f"precondition — tie sets {sorted(set(sizes))}, {share:.1%} of the outputs are no integers"
    if late_max:
        late = float(torch.cat(moved).double().mean())
        assert late >= 0.20, f"precondition — only {late:.1%} of the rows have their maximum in the last quarter of the keys"
    _run(pb)
    for what, result, ref in checks:
        _assert_equal(result(what), ref, what)
    return share


def check_attn_f32_census(lib, seed=0):
    """the key census of exact_checks.check_attention_census on the fp32 kernels, BITWISE: q = 0, so every score is 0 and every probability 1;
    v[j, c] = 64 where c = hash(j).  Every output is 64 * count_c / sk after one division: a key dropped or counted twice moves one channel."""
    g = torch.Generator().manual_seed(seed)
    pb = PlanBuilder(lib, _dev(lib), abi.F32)
    checks = []
    for case in ATTN_CENSUS_CASES:
        b, heads, sq, sk, d, _ = case
        for name, hashed in (("j % d", lambda j: j % d), ("(j // d) % d", lambda j: (j // d) % d)):
            what = f"fp32 attention census {b}x{heads}x{sq}x{sk} d{d}, hash {name}"
            _assert_kernel(case, what)
            j = torch.arange(sk)
            v = torch.zeros(b, sk, heads, d, dtype=torch.float64)
            v[:, j, :, hashed(j)] = 64.0
            count = torch.bincount(hashed(j), minlength=d).double()
            assert float(count.sum()) == sk and sk * 64 < EXACT
            ref = (64.0 * count / sk).float().double().expand(b, sq, heads, d)
            checks.append((what, _attn_launch(pb, torch.zeros(b, sq, heads, d, dtype=torch.float64), _ints(g, (b, sk, heads, d), 3), v, 1.0 / math.sqrt(d)), ref))
    _run(pb)
    for what, result, ref in checks:
        _assert_equal(result(what), ref, what)


def check_attn_f32_general(lib, sq, sk, d, batch=1, heads=2, kernel=None, seed=0):
    """GENERAL: random normal q / k / v against float64 softmax attention (SAM's two aspect ratios, reduced: few queries against many keys and the
    reverse), bound per element (module docstring).  Returns the kernel's largest error in fp32 spacings."""
    g = torch.Generator().manual_seed(seed)
    what = f"fp32 attention {batch}x{heads}x{sq}x{sk} d{d}"
    _assert_kernel((batch, heads, sq, sk, d, kernel), what)
    q, k, v = (torch.randn(batch, n, heads, d, generator=g).double() for n in (sq, sk, sk))
    scale = float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32))

    def formula(dt):
        p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.to(dt), k.to(dt)) * scale, dim=-1)
        return torch.einsum("bhqk,bkhd->bqhd", p, v.to(dt))
    ref = formula(torch.float64)
    gap, slack, denom = _slack32(formula(torch.float32), ref, what)
    pb = PlanBuilder(lib, _dev(lib), abi.F32)
    result = _attn_launch(pb, q, k, v, scale)
    _run(pb)
    return _assert_bound32(result(what), ref, denom, gap, slack, what, "attention_f32.general.fp32_gap")


ATTN_GENERAL_CASES = [dict(sq=9, sk=1100, d=16, kernel="wave"), dict(sq=9, sk=1100, d=32, kernel="wave"),
                      dict(sq=1100, sk=9, d=16, kernel="rows"), dict(sq=1100, sk=9, d=32, kernel="rows")]


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def norm_f32_in_registers(c, ldx, aligned=True):
    """the path rule of norm_f32_kernel (csrc/f32ops.hip): the row stays in registers between the passes (16-byte loads), or the element loop"""
    return c % 4 == 0 and c <= 1280 and ldx % 4 == 0 and aligned


def _launch_norm(lib, x, c, ldx_extra, ldy_extra, misaligned, gamma, beta, eps, out_dtype, act, registers, what):
    """x [rows, c] float64 (exact in fp32) -> (y [rows, c] as the kernel left it, on the host).  The input rows lie ldx_extra garbage columns apart,
    `misaligned` one float into their buffer; y is the left part of a sentinel-filled buffer with one spare row, checked here."""
    dev = _dev(lib)
    rows, ldx, ldy = x.shape[0], c + ldx_extra, c + ldy_extra
    assert bool((x.float().double() == x).all()), f"{what}: precondition — the inputs are not exact in fp32"
    pb = PlanBuilder(lib, dev, abi.F32)
    flat = pb.buf((rows * ldx + 4,), torch.float32)
    flat.fill_(GARBAGE)
    xb = flat[1:1 + rows * ldx].view(rows, ldx) if misaligned else flat[:rows * ldx].view(rows, ldx)
    assert xb.data_ptr() % 16 == (4 if misaligned else 0)
    xb[:, :c] = x.float().to(dev)
    if registers is not None:
        assert norm_f32_in_registers(c, ldx, not misaligned) == registers, f"{what}: the case is meant for the {'register' if registers else 'element-loop'} path"
    yb = pb.buf((rows + 1, ldy), torch.float32 if out_dtype is None else TD[out_dtype])
    yb.fill_(SENTINEL)
    pb.norm(xb, yb, rows, c, ldx=ldx, ldy=ldy, gamma=pb.const(gamma.float()) if gamma is not None else None,
            beta=pb.const(beta.float()) if beta is not None else None, eps=eps, act=act, dtype=abi.F32, out_dtype=out_dtype)
    _run(pb)
    _untouched(yb, rows, 0, c, what)
    return yb[:rows, :c].cpu()


def check_norm_f32_balanced(lib, rows, c, ldx_extra=0, ldy_extra=8, misaligned=False, gamma=True, beta=True, out_dtype=None, act=abi.ACT_NONE,
                            registers=None, first=0, seed=0):
    """norm_f32_kernel<float|bf16|f16>, BITWISE, eps = 0.  Rows from stream_checks._balanced: m - a on half of the columns, m + a on the other half,
    a a power of two — so mean = m, variance = a^2, rstd = 1 / a and (x - mean) * rstd = +-1, all exact; with integer gamma in [-7, 7] and integer
    beta the output is the integer +-gamma + beta.  out_dtype BF16 / F16: beta is wide enough for 20 % of the outputs to lie where the 16-bit type
    rounds integers, and the bytes must equal ref.float().to(T): ONE rounding.
    Activations: mtx_norm_args (include/mtx_hip.h) has an `act` ("activation applied last") but no act_param, and MTX_ACT_LEAKY's slope IS
    act_param — so in a norm the slope is 0 and LEAKY is RELU; that is what is asserted for both (negative results come out as zero)."""
    g = torch.Generator().manual_seed(seed)
    what = f"fp32 layernorm balanced {rows}x{c} ldx +{ldx_extra}{' misaligned' if misaligned else ''} -> {NAME[out_dtype] if out_dtype is not None else 'f32'} act {act}"
    x, m, a = _balanced(g, rows, c, first)
    if rows >= 4:
        assert {0.0, 64.0} <= set(m.abs().flatten().tolist()), f"{what}: needs a row with mean 0 and one with |mean| = 64"
    assert c * float(x.abs().max()) < EXACT and c * float((a * a).max()) < EXACT, f"{what}: precondition — the sums are not exact in fp32"
    assert torch.equal(x.sum(-1, keepdim=True), c * m) and torch.equal(((x - m) ** 2).sum(-1, keepdim=True), c * a * a)
    spread = 100 if out_dtype is None else int(2.5 * ROUNDS_FROM[out_dtype])
    gm = _nonzero_ints(g, (c,), 7) if gamma else None
    bt = _ints(g, (c,), spread) if beta else None
    d = x - x.mean(-1, keepdim=True)
    t = d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True)))
    assert bool((t.abs() == 1.0).all())
    if gm is not None:
        t = t * gm
    if bt is not None:
        t = t + bt
    assert bool((t == t.round()).all())
    if act != abi.ACT_NONE:
        assert act in (abi.ACT_RELU, abi.ACT_LEAKY)
        assert float((t < 0).double().mean()) >= 0.2, f"{what}: precondition — hardly any negative result"
        t = t.clamp_min(0.0)
    ref = t
    if out_dtype is not None:
        ref = _round(t, TD[out_dtype])
        if beta:
            _assert_rounding_share(ref, out_dtype, what)
    got = _launch_norm(lib, x, c, ldx_extra, ldy_extra, misaligned, gm, bt, 0.0, out_dtype, act, registers, what)
    _assert_equal(got, ref, what)


NORM_F32_BALANCED = [
    dict(rows=9, c=4, registers=True), dict(rows=9, c=252, registers=True), dict(rows=5, c=256, registers=True), dict(rows=7, c=260, ldx_extra=4, registers=True),
    dict(rows=7, c=1280, registers=True), dict(rows=7, c=1284, registers=False), dict(rows=7, c=200, ldx_extra=56, registers=True),
    dict(rows=7, c=200, ldx_extra=1, registers=False), dict(rows=7, c=74, registers=False), dict(rows=1, c=1152, registers=True, first=3),
    dict(rows=7, c=200, ldx_extra=56, misaligned=True, registers=False),                        # a view one float into its buffer
    dict(rows=7, c=1280, misaligned=True, registers=False),
    dict(rows=7, c=260, gamma=False, registers=True), dict(rows=7, c=260, beta=False, registers=True), dict(rows=7, c=260, gamma=False, beta=False, registers=True),
    dict(rows=7, c=74, gamma=False, registers=False), dict(rows=7, c=74, beta=False, registers=False), dict(rows=7, c=74, gamma=False, beta=False, registers=False),
    dict(rows=7, c=200, out_dtype=abi.BF16, registers=True), dict(rows=7, c=200, out_dtype=abi.F16, registers=True),
    dict(rows=7, c=1284, out_dtype=abi.BF16, registers=False), dict(rows=7, c=74, out_dtype=abi.F16, ldx_extra=3, registers=False),
    dict(rows=7, c=260, act=abi.ACT_RELU, registers=True), dict(rows=7, c=260, act=abi.ACT_LEAKY, registers=True),
    dict(rows=7, c=74, act=abi.ACT_RELU, registers=False), dict(rows=7, c=74, act=abi.ACT_LEAKY, out_dtype=abi.F16, registers=False),
]


def _ln_formula(x, c, gamma, beta, dt):
    """(x - mean) * rstd * gamma + beta in the order of the kernel, two-pass variance, eps = the production 1e-6, in precision dt"""
    x = x.to(dt)
    d = x - x.sum(-1, keepdim=True) / c
    t = d * (1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / c + EPS))
    if gamma is not None:
        t = t * gamma.to(dt)
    return t + beta.to(dt) if beta is not None else t


def check_norm_f32_bounded(lib, rows, c, family, ldx_extra=0, misaligned=False, registers=None, seed=0):
    """family "census": row r is zero except for ONE 16-byte chunk (four floats, position r % (c / 4)) that holds a power of two and so carries both
    sums alone — a chunk lost from or doubled in either pass moves the whole row; a factor gamma only, so that the small values of the empty chunks
    stay visible.  family "general": random normal rows (x 3, + 1) with gamma and beta.  Both with the production eps = 1e-6 and the measured bound
    of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    what = f"fp32 layernorm {family} {rows}x{c}"
    if family == "census":
        assert c % 4 == 0 and rows >= c // 4, f"{what}: every chunk position must be the only carrier once"
        r = torch.arange(rows)
        x = torch.zeros(rows, c, dtype=torch.float64)
        x.view(rows, c // 4, 4)[r, r % (c // 4)] = torch.exp2(((r // (c // 4) + r) % 7 - 2).double())[:, None]
        assert int((x != 0).sum()) == 4 * rows
        gamma, beta = _signed(g, (c,), 0.5, 1.5).float().double(), None
    else:
        x = (torch.randn(rows, c, generator=g) * 3 + 1).double()
        gamma, beta = _signed(g, (c,), 0.5, 1.5).float().double(), _signed(g, (c,), 2.0, 4.0).float().double()
    ref = _ln_formula(x, c, gamma, beta, torch.float64)
    gap, slack, denom = _slack32(_ln_formula(x, c, gamma, beta, torch.float32), ref, what)
    got = _launch_norm(lib, x, c, ldx_extra, 8, misaligned, gamma, beta, 1e-6, None, abi.ACT_NONE, registers, what)
    return _assert_bound32(got, ref, denom, gap, slack, what, f"norm_f32.{family}.fp32_gap")


NORM_F32_BOUNDED = [
    dict(rows=50, c=200, family="census", ldx_extra=56, registers=True), dict(rows=66, c=256, family="census", registers=True),
    dict(rows=320, c=1280, family="census", registers=True), dict(rows=321, c=1284, family="census", registers=False),
    dict(rows=50, c=200, family="census", misaligned=True, registers=False),
    dict(rows=7, c=200, family="general", ldx_extra=56, registers=True), dict(rows=5, c=1152, family="general", registers=True),
    dict(rows=5, c=1284, family="general", registers=False), dict(rows=9, c=75, family="general", registers=False),
    dict(rows=5, c=576, family="general", misaligned=True, registers=False),
]


# ---- element-wise and conversions -----------------------------------------------------------------------------------------------------------
EW_F32_BLOCK_CAP = 16384          # ew_f32_launch (csrc/f32ops.hip): at most this many workgroups of 256 threads, one element per thread and trip


class _Ew32(_Ew):
    """stream_checks._Ew for an fp32 plan"""

    def __init__(self, lib):
        self.lib, self.dtype, self.dev, self.td = lib, abi.F32, _dev(lib), torch.float32
        self.host = torch.device("cpu")
        self.pb = PlanBuilder(lib, self.dev, abi.F32)
        self.checks = []


def check_ew_f32_exact(lib, seed=0):
    """ew_f32_kernel on integers, zero differing elements: ADD, MUL, COPY, ACT (RELU; LEAKY with slope 0.25), ROW_GATHER by a map with repeats and out of
    order, SHUFFLE2_ADD without a skip, with one skip image for every sample (lds = 0) and with a skip per sample (lds = the image size).  lda, ldb and
    ldy all differ and are wider than c (an odd c: the kernel has no vector path to be aligned for)."""
    e = _Ew32(lib)
    g = torch.Generator().manual_seed(seed)
    n, h, w, c = 3, 5, 7, 13
    a, b = _ints(g, (n, h, w, c), 1 << 22), _ints(g, (n, h, w, c), 1 << 22)
    fa, fb = _ints(g, (n, h, w, c), 4000), _ints(g, (n, h, w, c), 4000)
    leaky = torch.where(a > 0, a, a * 0.25)
    assert float((fa * fb).abs().max()) < EXACT and bool((leaky.float().double() == leaky).all()) and float((a < 0).double().mean()) > 0.2
    for name, kind, va, vb, ref, kw in (("add", abi.EW_ADD, a, b, a + b, {}), ("mul", abi.EW_MUL, fa, fb, fa * fb, {}), ("copy", abi.EW_COPY, a, None, a, {}),
                                        ("relu", abi.EW_ACT, a, None, a.clamp_min(0.0), dict(act=abi.ACT_RELU)),
                                        ("leaky 0.25", abi.EW_ACT, a, None, leaky, dict(act=abi.ACT_LEAKY, act_param=0.25))):
        o, whole = e.out(n, h, w, c, c0=3, extra=6)                                            # ldy = 22
        e.pb.ew(kind, e.inp(va, c0=2, extra=2), b=e.inp(vb, c0=1, extra=5) if vb is not None else None, out=o, label=name, **kw)      # lda = 17, ldb = 19
        e.expect(o, ref, name, whole)
    src_rows, rows, cc = 45, 37, 11
    src = _nonzero_ints(g, (src_rows, cc), 1 << 20)
    idx = torch.randint(0, 6, (rows,), generator=g) * 8 + torch.arange(rows) % 5
    assert len(set(idx.tolist())) < rows and bool((idx[1:] < idx[:-1]).any()) and int(idx.max()) < src_rows
    sa = e.inp(src.view(1, 1, src_rows, cc), extra=6)                                          # lda = 17
    dst = e.pb.buf((rows + 3, cc + 9), torch.float32)                                          # ldy = 20
    dst.fill_(SENTINEL)
    e.pb.row_gather(sa.t, dst, e.pb.hold(idx.to(torch.int32).to(e.dev)), rows, cc, lda=sa.ld, ldy=dst.shape[-1])
    e.expect(dst[:rows, :cc], src[idx], "row_gather (repeats, out of order)", dst)
    cols = _nonzero_ints(g, (n, h, w, 4 * c), 1 << 20)
    shuffled = cols.view(n, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c)      # column (dy * 2 + dx) * c + ch -> pixel (2 y + dy, 2 x + dx)
    skip1, skipn = _ints(g, (1, 2 * h, 2 * w, c), 1 << 20), _ints(g, (n, 2 * h, 2 * w, c), 1 << 20)
    assert not torch.equal(skipn[0], skipn[1]) and not torch.equal(skipn[1], skipn[2])
    for name, skip, ref in (("no skip", None, shuffled), ("one skip image (lds = 0)", skip1, shuffled + skip1), ("a skip per sample", skipn, shuffled + skipn)):
        ca = e.inp(cols, c0=0, extra=3)                                                        # lda = 4 c + 3
        sk = e.inp(skip, c0=2, extra=4) if skip is not None else None                          # ldb = c + 6
        o, whole = e.out(n, 2 * h, 2 * w, c, c0=1, extra=3)                                    # ldy = c + 4
        args = abi.EwArgs()
        args.a, args.b, args.s, args.y = ca.ptr, (sk.ptr if sk is not None else None), None, o.ptr
        args.n, args.h, args.w, args.c = n, h, w, c
        args.lda, args.ldb, args.ldy = ca.ld, (sk.ld if sk is not None else 0), o.ld
        args.lds = 4 * h * w * sk.ld if (sk is not None and skip.shape[0] == n) else 0
        args.kind, args.act, args.act_param, args.i0, args.i1, args.dtype = abi.EW_SHUFFLE2_ADD, 0, 0.0, 0, 0, abi.F32
        e.pb._add(abi.OP_EW, args, "shuffle2_add")
        e.expect(o, ref, f"shuffle2_add, {name}", whole)
    e.run()


def check_ew_f32_grid_stride(lib):
    """more elements than ew_f32_launch starts threads (SAM's per-box high-resolution features are): the grid-stride loop takes a second trip.  A copy
    between two row strides of values that are their own index: an element the loop skips keeps the sentinel, a wrong stride lands on the wrong index."""
    e = _Ew32(lib)
    rows, c = 16407, 256
    assert EW_F32_BLOCK_CAP * 256 < rows * c < 2 * EW_F32_BLOCK_CAP * 256 and rows * c >= 4_200_000 and rows * c < EXACT
    src = e.pb.buf((1, 1, rows, c + 3), torch.float32)
    src.fill_(GARBAGE)
    src[0, 0, :, 1:1 + c] = torch.arange(rows * c, dtype=torch.float32, device=e.dev).view(rows, c)
    o, whole = e.out(1, 1, rows, c, c0=2, extra=3)
    e.pb.ew(abi.EW_COPY, Act(src, 1, 1, rows, c, 1), out=o)
    _run(e.pb)
    got = o.torch().reshape(rows * c)
    bad = got != torch.arange(rows * c, dtype=torch.float32, device=e.dev)
    assert not bool(bad.any()), f"copy of {rows * c} elements: {int(bad.sum())} differ, the first at {int(bad.nonzero()[0])} (got {float(got[bad][0])})"
    assert bool((whole[:1, ..., :2] == SENTINEL).all()) and bool((whole[:1, ..., 2 + c:] == SENTINEL).all()) and bool((whole[1:] == SENTINEL).all())


def _all_patterns(td):
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(td)


def check_cvt_f32_all_patterns(lib, src_dtype):
    """cvt_f32_kernel<f16|bf16> on all 65536 bit patterns of the source type (subnormals, infinities, NaNs): the fp32 bit patterns must equal
    torch's .float(), NaNs compared as NaN"""
    dev, td = _dev(lib), TD[src_dtype]
    what = f"cvt {NAME[src_dtype]} -> f32"
    x = _all_patterns(td).view(256, 256)
    pb = PlanBuilder(lib, dev, abi.F32)
    src = pb.buf((256, 256 + 8), td)
    src.fill_(GARBAGE)
    src[:, :256] = x.to(dev)
    whole = pb.buf((256 + 1, 256 + 5), torch.float32)
    whole.fill_(SENTINEL)
    args = abi.EwArgs()
    args.a, args.b, args.s, args.y = src.data_ptr(), None, None, whole.data_ptr()
    args.n, args.h, args.w, args.c = 1, 1, 256, 256
    args.lda, args.ldb, args.ldy, args.lds = src.shape[-1], 0, whole.shape[-1], 0
    args.kind, args.act, args.act_param, args.i0, args.i1, args.dtype = abi.EW_CVT_F32, 0, 0.0, src_dtype, 0, abi.F32
    pb._add(abi.OP_EW, args, "cvt_f32")
    _run(pb)
    _untouched(whole, 256, 0, 256, what)
    got, want = whole[:256, :256].cpu(), x.float()
    assert int(torch.isnan(want).sum()) > 100 and int(torch.isinf(want).sum()) == 2
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaNs in other places"
    bad = (got.view(torch.int32) != want.view(torch.int32)) & ~torch.isnan(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of 65536 bit patterns differ, the first is source pattern {int(x.view(torch.int16)[bad][0]) & 0xFFFF:#06x}"


def _cvt16_census(td):
    """fp32 values around everything the 16-bit type T does: every finite value of T, the midpoint between every two neighbours (a tie: to even), one
    fp32 ulp either side of each midpoint; above the largest finite value the midpoint to the next power of two (where IEEE rounding turns to infinity),
    one ulp either side, twice the largest value, the largest fp32 value and infinity, of both signs; below the smallest subnormal half of it (a tie: to
    zero), one ulp either side, a quarter of it and the smallest fp32 subnormal, of both signs; and -0.  -> float32 [N]"""
    fin = _all_patterns(td).float()
    fin = fin[torch.isfinite(fin)].double().unique()
    mid = (fin[1:] + fin[:-1]) / 2
    assert bool((mid.float().double() == mid).all()), "the midpoints are exact in fp32"
    mid = mid.float()
    inf = torch.tensor(float("inf"))
    top, step, tiny = float(fin[-1]), float(fin[-1] - fin[-2]), float(fin[fin > 0][0])
    edge = torch.tensor([top + step / 2, min(2 * top, float(torch.finfo(torch.float32).max)), tiny / 2, tiny / 4], dtype=torch.float64)
    assert bool((edge.float().double() == edge).all())
    edge = edge.float()
    edge = torch.cat([edge, torch.nextafter(edge, inf), torch.nextafter(edge, -inf), torch.tensor([torch.finfo(torch.float32).max, float("inf"), 2.0 ** -149])])
    return torch.cat([fin.float(), mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), edge, -edge, torch.tensor([-0.0])])


def check_cvt_16_census(lib, dtype):
    """cvt_16_kernel<f16|bf16> on the census of _cvt16_census, copies = 1 .. 4 side by side, ldy > copies * c, lda > c: the bit patterns must equal
    torch's .to(T) — round to nearest, ties to even, subnormals kept.  ONE documented difference: the library's conversion to f16 saturates at
    +-65504 instead of overflowing to infinity (from_f32<_Float16>, csrc/mtx_device.h; MTX_EW_CVT_16 in include/mtx_hip.h), so for f16 the reference is
    x.clamp(-65504, 65504).to(T) — asserted here to be the same bytes as x.to(T) wherever |x| < 65520, i.e. wherever IEEE rounding stays finite.
    bf16 has no such clamp: its overflow edge must give infinity.  (NaN is left out: the f16 clamp is a v_med3_f32 on hardware and a pair of compares on
    the simulator, which treat a NaN differently.)"""
    dev, td = _dev(lib), TD[dtype]
    x = _cvt16_census(td)
    c = 515
    rows = (x.numel() + c - 1) // c
    x = torch.cat([x, torch.ones(rows * c - x.numel())]).view(rows, c)
    plain = x.to(td)
    want = x.clamp(-65504.0, 65504.0).to(td) if dtype == abi.F16 else plain
    stays = x.abs() < (65520.0 if dtype == abi.F16 else float("inf"))
    assert torch.equal(want.view(torch.int16)[stays], plain.view(torch.int16)[stays]), "the clamp of the contract changes nothing where IEEE rounding stays finite"
    assert int(torch.isinf(plain).sum()) >= 8 and int((plain.float() != x).sum()) > 100000 and int(((plain == 0) & (x != 0)).sum()) >= 4
    pb = PlanBuilder(lib, dev, dtype)
    src = pb.buf((rows, c + 5), torch.float32)
    src.fill_(GARBAGE)
    src[:, :c] = x.to(dev)
    outs = []
    for copies in (1, 2, 3, 4):
        whole = pb.buf((rows + 1, copies * c + 3), td)
        whole.fill_(SENTINEL)
        pb.cvt16(src, whole, rows, c, copies=copies, lda=c + 5)
        outs.append(whole)
    _run(pb)
    for copies, whole in zip((1, 2, 3, 4), outs):
        what = f"cvt f32 -> {NAME[dtype]}, {copies} copies"
        _untouched(whole, rows, 0, copies * c, what)
        for j in range(copies):
            got = whole[:rows, j * c:(j + 1) * c].cpu()
            bad = got.view(torch.int16) != want.view(torch.int16)
            if bool(bad.any()):
                i = tuple(int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{what}, copy {j}: {int(bad.sum())} of {x.numel()} values differ; first {float(x[i])!r} ({int(x.view(torch.int32)[i]) & 0xFFFFFFFF:#010x}): "
                                     f"got {int(got.view(torch.int16)[i]) & 0xFFFF:#06x}, want {int(want.view(torch.int16)[i]) & 0xFFFF:#06x}")


def check_cvt_16_refusals(lib, dtype):
    """the launcher reports five copies and ldy < copies * c as errors and starts nothing: the destination keeps its sentinel.  (The destination is a view
    into a buffer large enough for what a launch that was NOT refused would write.)"""
    dev, td = _dev(lib), TD[dtype]
    rows, c = 6, 24
    for copies, ldy, why in ((5, 5 * c + 8, "five copies"), (2, 2 * c - 1, "ldy < copies * c"), (1, c - 8, "ldy < c")):
        pb = PlanBuilder(lib, dev, dtype)
        big = pb.buf((rows * 8 * c,), td)
        big.fill_(SENTINEL)
        src = pb.buf((rows, c), torch.float32)
        src.fill_(1.0)
        pb.cvt16(src, big[:rows * ldy].view(rows, ldy), rows, c, copies=copies)
        try:
            _run(pb)
        except ModelError as err:
            assert "CVT_16" in str(err), f"{why}: refused with another message: {err}"
        else:
            raise AssertionError(f"cvt f32 -> {NAME[dtype]}: {why} was not refused")
        _sync(lib)
        assert bool((big == SENTINEL).all()), f"cvt f32 -> {NAME[dtype]}: {why} was refused, but the destination was written"


# ---- RCAN channel attention -----------------------------------------------------------------------------------------------------------------
def ca_on_split_kernel(c, cr, split):
    """the dispatch rule of ca_launch (csrc/elementwise.hip), pool-before-conv form: MTX_CA_SPLIT workgroups per image need a scratch and C * Cr <= 1024"""
    return split and c * cr <= 1024


def _ca_mlp(g, m, c, cr):
    """squeeze / excite weights for the pooled vectors m [n, c] of the reference: small dyadic fractions; b1 makes every even hidden unit live on every
    image; w2 and b2 are scaled by a power of two so that the largest |z| lies in (1, 2] -> (w1, b1, w2, b2), all exact in fp32"""
    w1 = _ints(g, (cr, c), 4) / 64.0
    h0 = m @ w1.t()
    b1 = torch.where(torch.arange(cr) % 2 == 0, torch.ceil(-h0.amin(0)) + 1.0, _ints(g, (cr,), 4) / 4.0)
    w2, b2 = _ints(g, (c, cr), 4) / 8.0, _ints(g, (c,), 8) / 4.0
    z = torch.relu(h0 + b1) @ w2.t() + b2
    f = 2.0 ** -math.ceil(math.log2(float(z.abs().max()) / 2.0))
    return w1, b1, w2 * f, b2 * f


def _ca_z(m, w1, b1, w2, b2):
    """-> (the pre-sigmoid value z [n, c], the hidden units before the ReLU) in the precision of m"""
    dt = m.dtype
    pre = m @ w1.to(dt).t() + b1.to(dt)
    return torch.relu(pre) @ w2.to(dt).t() + b2.to(dt), pre


def _logit(s):
    s = s.double()
    return torch.log(s / (1.0 - s))


def _ca_bound(z, s32, what):
    """The kernel stores s = sigmoid(z) in fp32, so the comparison is made in logit space, log(s / (1 - s)) against z in float64.  One rounding of s
    alone is worth 2^-25 / (s (1 - s)) there — 2.4e-7 at z = 0, 5.7e-7 at |z| = 2 — whatever |z| is, so the scale of an image's bound is its largest
    |z| (in (1, 2] by construction: beyond it the fp32 sigmoid saturates and the comparison stops seeing anything — a precondition), not the
    element's own.  gap: the torch fp32 formula's distance from float64 in those units; slack = 4 gap, at least stream_checks' floor 2^-20.
    -> (gap, slack, bound [n, 1] in logit units)"""
    scale = z.abs().amax(dim=1, keepdim=True)
    assert 1.0 < float(z.abs().max()) <= 2.0 and float(scale.min()) > 0.25, f"{what}: precondition — max |z| {float(z.abs().max())} must lie in (1, 2]"
    gap = float(((_logit(s32) - z).abs() / scale).max())
    slack = max(4.0 * gap, SLACK_FLOOR)
    return gap, slack, slack * scale


def _assert_ca(s_got, z, gap, slack, bound, what, name):
    s_got = s_got.double()
    assert bool(((s_got > 0) & (s_got < 1)).all()), f"{what}: a factor outside (0, 1)"
    err = (_logit(s_got) - z).abs()
    worst = float(err.max())
    print(f"{what}: fp32 gap {gap:.3g}, slack {slack:.3g}, bound {float(bound.min()):.3g} .. {float(bound.max()):.3g}, kernel error {worst:.3g} logit units")
    _note(name, fp32_gap=gap, slack=slack, kernel_err_logit=worst)
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {z.numel()} factors beyond {float(bound[i[0]]):.3g} logit units; first at {i}: "
                             f"logit {float(_logit(s_got)[i])}, want {float(z[i])}; worst {worst:.3g}")
    return worst


def _assert_sharp(z, perturbed, bound, what):
    """every perturbed reference differs from the true one by at least 64 bounds in at least one channel of every image"""
    for name, zp in perturbed:
        ratio = ((zp - z).abs().amax(dim=1, keepdim=True) / bound).min()
        assert float(ratio) >= 64.0, f"{what}: precondition — the reference with {name} is only {float(ratio):.1f} bounds away: the case would not see it"


def _rerun(lib, plan, s_buf, n, what):
    """a second run of the same plan into a NaN-filled output gives the same bytes (the split kernel's arrival counters are back at zero, the result
    does not depend on who arrived last)"""
    first = s_buf.clone()
    s_buf[:n] = float("nan")
    plan.run()
    _sync(lib)
    assert torch.equal(s_buf[:n], first[:n]), f"{what}: a second run of the plan differs in {int((s_buf[:n] != first[:n]).sum())} factors"
    assert bool((s_buf[n:] == SENTINEL).all()), f"{what}: written beyond the last image"


def check_ca_exact(lib, dtype, n, h, w, c, cr, tiles, split=True, canvas=None, inv_hw_dev=False, expect_split=None, seed=0):
    """ca_kernel / ca_split_kernel, pool-before-conv form.  t holds integers in [0, 3] on the image (zeros beyond it on a canvas, garbage in the unused
    channels of its pixel stride), the conv weights integers in [-2, 2], the bias an integer, chan_sum an integer split of the true channel totals over
    `tiles` rows: with 9 c 6 h w < 2^24 every sum is exact in fp32 in any order and the pooled mean is one exact integer times inv_hw.  The reference
    is computed twice in float64 — F.conv2d + mean, and the kernel's decomposition (totals - border strips + corners), which must agree exactly —
    and the second is then PERTURBED: each corner pixel, one pixel of each border strip, one chan_sum row dropped in turn.  Preconditions: every
    perturbed reference is at least 64 bounds away in every image; at least half of the hidden units are live.  Bound: _ca_bound."""
    g = torch.Generator().manual_seed(seed)
    dev, td = _dev(lib), TD[dtype]
    H, W = canvas if canvas else (h, w)
    what = f"channel attention {n}x{h}x{w}x{c} / {cr}, {tiles} sum rows, {'split' if split else 'single'}{' canvas' if canvas else ''}{' inv_hw_dev' if inv_hw_dev else ''} [{NAME[dtype]}]"
    if expect_split is not None:
        assert ca_on_split_kernel(c, cr, split) == expect_split, f"{what}: the case is meant for {'ca_split_kernel' if expect_split else 'ca_kernel'}"
    assert 9 * c * 6 * h * w < EXACT, f"{what}: precondition — the sums are not exact in fp32"
    t = torch.randint(0, 4, (n, h, w, c), generator=g).double()
    wt = _ints(g, (c, c, 3, 3), 2)
    bias = _ints(g, (c,), 8)
    total = t.sum((1, 2))
    cs = _ints(g, (n, tiles, c), 9)
    cs[:, -1] = total - cs[:, :-1].sum(1)
    assert torch.equal(cs.sum(1), total)
    strips = [t[:, 0].sum(1), t[:, h - 1].sum(1), t[:, :, 0].sum(1), t[:, :, w - 1].sum(1)]          # top row, bottom row, left column, right column
    corners = [t[:, 0, 0], t[:, 0, w - 1], t[:, h - 1, 0], t[:, h - 1, w - 1]]

    def pooled(total_, strips_, corners_):
        """mean(conv3x3(t) + bias) from the channel totals, by linearity (include/mtx_hip.h, mtx_ca_args.t)"""
        s = torch.zeros(n, c, dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                dy, dx = ky - 1, kx - 1
                st = total_.clone()
                if dy:
                    st = st - strips_[0 if dy == 1 else 1]              # a tap one row DOWN never reads row 0 for an in-image output
                if dx:
                    st = st - strips_[2 if dx == 1 else 3]
                if dy and dx:
                    st = st + corners_[(2 if dy == -1 else 0) + (1 if dx == -1 else 0)]
                s = s + st @ wt[:, :, ky, kx].t()
        return bias + s / (h * w)
    u = F.conv2d(t.permute(0, 3, 1, 2), wt, None, padding=1)
    m = pooled(total, strips, corners)
    assert torch.equal(m, bias + u.sum((2, 3)) / (h * w)), f"{what}: the decomposed reference is not the conv's mean"
    w1, b1, w2, b2 = _ca_mlp(g, m, c, cr)
    z, pre = _ca_z(m, w1, b1, w2, b2)
    assert float((pre > 0).double().mean()) >= 0.5, f"{what}: precondition — only {float((pre > 0).double().mean()):.0%} of the hidden units are live"
    m32 = F.conv2d(t.float().permute(0, 3, 1, 2), wt.float(), bias.float(), padding=1).mean((2, 3))
    gap, slack, bound = _ca_bound(z, torch.sigmoid(_ca_z(m32, w1, b1, w2, b2)[0]), what)
    perturbed = []
    for k in range(4):
        perturbed.append((f"corner {k} dropped", _ca_z(pooled(total, strips, [cn * (j != k) for j, cn in enumerate(corners)]), w1, b1, w2, b2)[0]))
        px = (w if k < 2 else h) * 5 // 8
        pixel = t[:, (0, h - 1)[k], px] if k < 2 else t[:, px, (0, w - 1)[k - 2]]
        perturbed.append((f"pixel {px} of border strip {k} dropped", _ca_z(pooled(total, [sp - pixel * (j == k) for j, sp in enumerate(strips)], corners), w1, b1, w2, b2)[0]))
    row = tiles * 5 // 8
    perturbed.append((f"chan_sum row {row} dropped", _ca_z(pooled(total - cs[:, row], strips, corners), w1, b1, w2, b2)[0]))
    _assert_sharp(z, perturbed, bound, what)

    pb = PlanBuilder(lib, dev, dtype)
    tb = pb.act(n, H, W, c, ld=c + 8)
    tb.t.fill_(GARBAGE)
    tb.t[..., :c] = 0.0
    tb.t[:, :h, :w, :c] = t.to(td)
    wpk = pb.const(wt.permute(0, 2, 3, 1).reshape(c, 9, c), td)
    valid = None
    if canvas:
        valid = pb.buf((2,), torch.int32)
        valid.copy_(torch.tensor([h, w], dtype=torch.int32))
    inv_dev = None
    if inv_hw_dev:
        inv_dev = pb.buf((1,), torch.float32)
        inv_dev.fill_(1.0 / (h * w))
    s_buf = pb.buf((n + 1, c), torch.float32)
    s_buf.fill_(SENTINEL)
    pb.channel_attention(pb.const(cs.float()), pb.const(w1.float()), pb.const(b1.float()), pb.const(w2.float()), pb.const(b2.float()), s_buf, n, tiles, c, cr,
                         GARBAGE if inv_hw_dev else 1.0 / (h * w), inv_hw_dev=inv_dev, before_conv=(tb, wpk, pb.const(bias.float())), valid_hw=valid, split=split)
    plan = _run(pb)
    assert bool((s_buf[n:] == SENTINEL).all()), f"{what}: written beyond the last image"
    worst = _assert_ca(s_buf[:n].cpu(), z, gap, slack, bound, what, "channel_attention.exact.fp32_gap")
    _rerun(lib, plan, s_buf, n, what)
    return worst


CA_CASES = [
    dict(n=2, h=37, w=29, c=64, cr=4, tiles=5, split=True, expect_split=True), dict(n=2, h=37, w=29, c=64, cr=4, tiles=5, split=False, expect_split=False),
    # a side above 480: sixteen pixels in flight in ca_kernel's strip loop; more than 960 sum rows: its 16-row unrolled loop
    dict(n=1, h=3, w=530, c=64, cr=16, tiles=1000, split=True, expect_split=True), dict(n=1, h=3, w=530, c=64, cr=16, tiles=1000, split=False, expect_split=False),
    # a side above 224: eight in flight; sum rows across several shares of the split kernel
    dict(n=1, h=230, w=5, c=64, cr=4, tiles=193, split=True, expect_split=True), dict(n=1, h=230, w=5, c=64, cr=4, tiles=193, split=False, expect_split=False),
    dict(n=2, h=2, w=3, c=8, cr=2, tiles=1, split=True, expect_split=True),
    dict(n=2, h=21, w=40, c=32, cr=8, tiles=65, canvas=(64, 64), split=True, expect_split=True),          # a device-side valid_hw
    dict(n=2, h=21, w=40, c=32, cr=8, tiles=65, canvas=(64, 64), split=False, expect_split=False),
    dict(n=2, h=37, w=29, c=64, cr=4, tiles=5, split=True, inv_hw_dev=True, expect_split=True),
    dict(n=1, h=37, w=29, c=64, cr=32, tiles=5, split=True, expect_split=False),                          # C * Cr > 1024: ca_kernel even with a scratch
]


def check_ca_pooled_exact(lib, n, c, cr, tiles, hw=37 * 29, seed=0):
    """ca_kernel without t (the plain pooled mean; the launcher's fp16 instantiation): chan_sum holds integers in [0, 2000], so the totals are exact in
    any order and the pooled mean is one integer times inv_hw.  The tile counts leave a remainder in each of the kernel's reduction loops (c % 4 == 0 and
    c <= 256: 1024 / (c / 4) row subsets, sixteen rows in flight, then one at a time; otherwise 1024 / c subsets of single loads).  Same weights, bound
    and preconditions as check_ca_exact, with one chan_sum row dropped as the perturbation."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev(lib)
    what = f"channel attention of pooled sums {n}x{c} / {cr}, {tiles} sum rows"
    per = 1024 // (c // 4) if (c % 4 == 0 and c <= 256) else max(1024 // c, 1)
    assert tiles % per and (tiles < per or tiles % (16 * per) >= per or per == 1), f"{what}: meant to leave a remainder in the reduction loops"
    cs = torch.randint(0, 2001, (n, tiles, c), generator=g).double()
    assert tiles * 2000 < EXACT
    total = cs.sum(1)
    m = total / hw
    w1, b1, w2, b2 = _ca_mlp(g, m, c, cr)
    z, pre = _ca_z(m, w1, b1, w2, b2)
    assert float((pre > 0).double().mean()) >= 0.5, f"{what}: precondition — only {float((pre > 0).double().mean()):.0%} of the hidden units are live"
    m32 = cs.float().sum(1) * torch.tensor(1.0 / hw, dtype=torch.float32)
    gap, slack, bound = _ca_bound(z, torch.sigmoid(_ca_z(m32, w1, b1, w2, b2)[0]), what)
    row = tiles * 5 // 8
    _assert_sharp(z, [(f"chan_sum row {r} dropped", _ca_z((total - cs[:, r]) / hw, w1, b1, w2, b2)[0]) for r in (0, row, tiles - 1)], bound, what)
    pb = PlanBuilder(lib, dev, abi.F16)
    s_buf = pb.buf((n + 1, c), torch.float32)
    s_buf.fill_(SENTINEL)
    pb.channel_attention(pb.const(cs.float()), pb.const(w1.float()), pb.const(b1.float()), pb.const(w2.float()), pb.const(b2.float()), s_buf, n, tiles, c, cr, 1.0 / hw)
    plan = _run(pb)
    assert bool((s_buf[n:] == SENTINEL).all()), f"{what}: written beyond the last image"
    worst = _assert_ca(s_buf[:n].cpu(), z, gap, slack, bound, what, "channel_attention.pooled.fp32_gap")
    _rerun(lib, plan, s_buf, n, what)
    return worst


CA_POOLED_CASES = [dict(n=2, c=64, cr=4, tiles=1100), dict(n=2, c=100, cr=10, tiles=727), dict(n=3, c=30, cr=3, tiles=75), dict(n=2, c=512, cr=32, tiles=5)]

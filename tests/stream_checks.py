"""Exact-input checks of the streaming kernels — csrc/norm.hip (LayerNorm, RMSNorm, adaLN, GroupNorm) and ew_kernel of csrc/elementwise.hip —
against float64 references.

Norms cannot be exact (a square root and a division), but their inputs can be chosen so that the statistics are: a BALANCED row holds m - a on
half of its columns and m + a on the other half (m a small integer, a a power of two), so mean = m and sum (x - mean)^2 = C a^2 whatever the
summation order; a CENSUS row (pixel) is zero except for one 16-byte chunk (one pixel) that carries both sums alone, so a chunk lost from or
doubled in either pass moves the whole row.  What is left of the kernel's freedom is a few fp32 roundings and ONE rounding to the storage
type T, hence the bound per element

    |y - ref| <= 0.5 * spacing_T(ref) + slack * max(|ref|, row max |ref| * 2^-8)

where slack is measured, not chosen: the same formula evaluated with plain torch fp32 ops on the same inputs, its largest distance to the
float64 reference in the units of the bound's second term, times four (a kernel may sum in another order), at least 2^-20.  The case fails
BEFORE it looks at the kernel unless slack < 2^-4 of T's relative spacing (2^-(MANT + 1)): inputs with a cancellation are not sharp.

The element-wise kinds move or combine integers: the expected output is the float64 result rounded once to T, zero differing elements.
Every output lies inside a sentinel-filled buffer — padding columns and one spare image behind it — that must come back untouched.

Every case asserts its preconditions from the reference alone.  Same layout as exact_checks.py: written once, run on the simulator and on
the product library."""
import torch
import torch.nn.functional as F

import parity_log
from exact_checks import EXACT, INT_CAP, MANT, _assert_equal, _assert_rounding_share, _ints, _round, _spacing, operand_range
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder
from op_checks import TD, _dev, _run

EPS = float(torch.tensor(1e-6, dtype=torch.float32))     # the value the kernel receives (mtx_norm_args.eps is a float)
SLACK_FLOOR = 2.0 ** -20
ROW_FLOOR = 2.0 ** -8
SENTINEL, GARBAGE = -123.0, 7.0                          # outputs' surroundings / inputs' unused columns (both exact in bf16 and f16)
PATTERNS = ((0, 1), (64, 1), (3, 2), (-64, 1), (0, 4), (-5, 8), (7, 4))      # (m, a) of a balanced row: m = 0; |m| = 64 with a = 1 (the mean far above the deviation); others
NAME = {abi.BF16: "bf16", abi.F16: "f16", abi.F32: "f32"}
_FIGURES = {}


def _note(name, dtype, gap, slack, worst):
    """the largest figures of the session per storage type: fp32 formula against float64 (gap), the slack that follows, the kernel's error in spacings of T"""
    f = _FIGURES.setdefault(name, {})
    for key, v in (("fp32_gap", gap), ("slack", slack), ("kernel_err_spacings", worst)):
        k = f"{NAME[dtype]}_{key}"
        f[k] = max(f.get(k, 0.0), float(v))
    parity_log.record(name, **{k: (round(v, 4) if k.endswith("spacings") else f"{v:.3e}") for k, v in f.items()})      # (record keeps six decimals of a float)


def _exact_in(v, td):
    return bool((v.to(td).double() == v).all())


def _balanced(g, groups, count, first=0):
    """[groups, count] float64: group i holds m_i - a_i on a random half of its positions and m_i + a_i on the other half -> (values, m, a)"""
    assert count % 2 == 0
    pat = torch.tensor(PATTERNS, dtype=torch.float64, device=g.device)[(torch.arange(groups, device=g.device) + first) % len(PATTERNS)]
    m, a = pat[:, 0:1], pat[:, 1:2]
    rank = torch.rand(groups, count, generator=g, device=g.device).argsort(dim=1)
    return m + a * torch.where(rank < count // 2, -1.0, 1.0).double(), m, a


def _signed(g, shape, lo, hi):
    """random sign times uniform [lo, hi): values that cannot cancel against a smaller term"""
    mag = torch.rand(shape, generator=g, device=g.device) * (hi - lo) + lo
    return mag * (torch.randint(0, 2, shape, generator=g, device=g.device) * 2 - 1)


def _slack(f32, ref, dtype, what):
    """slack and the bound's denominator from the reference and its plain fp32 evaluation (see the module docstring); asserts the sharpness precondition"""
    denom = torch.maximum(ref.abs(), ref.abs().amax(dim=-1, keepdim=True) * ROW_FLOOR)
    assert float(denom.min()) > 0.0, f"{what}: a row of zeros has no scale"
    gap = float(((f32.double() - ref).abs() / denom).max())
    slack = max(4.0 * gap, SLACK_FLOOR)
    limit = 2.0 ** -4 * 2.0 ** -(MANT[dtype] + 1)
    assert slack < limit, f"{what}: precondition — the fp32 formula is {gap:.3g} from float64, slack {slack:.3g} >= {limit:.3g}: these inputs are not sharp"
    return gap, slack, denom


def _assert_bound(got, ref, denom, gap, slack, dtype, what, name):
    err = (got.double() - ref).abs()
    sp = _spacing(ref, dtype)
    bad = err > 0.5 * sp + slack * denom
    worst = float((err / sp).max())
    print(f"{what} [{NAME[dtype]}]: fp32 gap {gap:.3g}, slack {slack:.3g}, kernel error {worst:.4f} spacings")
    _note(name, dtype, gap, slack, worst)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements beyond half a spacing of the storage type + {slack:.3g} relative; "
                             f"first at {i}: got {float(got[i])}, want {float(ref[i])}; worst {worst:.4f} spacings")
    return worst


# ---- row norms ----------------------------------------------------------------------------------------------------------------------------
def norm_is_full_form(c, affine, act=abi.ACT_NONE):
    """the dispatch rule of norm_launch (csrc/norm.hip): the straight-line kernel or the general one"""
    per_lane = (c // 8 + 63) // 64
    return c % 512 == 0 and per_lane in (2, 4, 6, 12) and not affine and act == abi.ACT_NONE


def _norm_formula(x, c, kind, gamma, beta, ms, mh, dt):
    """(x - mean) * rstd [* gamma + beta] [* (1 + scale) + shift] in the order of the kernel, two-pass variance, in precision dt"""
    x = x.to(dt)
    d = x - x.sum(-1, keepdim=True) / c if kind == 0 else x
    t = d * (1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / c + EPS))
    if gamma is not None:
        t = t * gamma.to(dt)
    if beta is not None:
        t = t + beta.to(dt)
    if ms is not None:
        t = t * (1.0 + ms.to(dt))
    if mh is not None:
        t = t + mh.to(dt)
    return t


def check_norm_exact(lib, dtype, rows, c, kind=0, family="balanced", affine=False, modulate=False, rows_per=None, ldx_extra=0, ldy_extra=0,
                     misaligned=False, expect_full=None, seed=0):
    """family: "balanced" or "census" (module docstring).  affine: fp32 gamma (and beta for LayerNorm); misaligned: both passed through a view
    one float into their buffer (the scalar affine path).  modulate: adaLN rows scale / shift in T, row r reads modulation row r // rows_per.
    expect_full: the kernel form the case is meant for.  Returns the kernel's largest error in spacings of T."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator(device=dev).manual_seed(seed)
    what = f"{'rmsnorm' if kind else 'layernorm'} {family} {rows}x{c}"
    if expect_full is not None:
        assert norm_is_full_form(c, affine) == expect_full, f"{what}: the case is meant for the {'straight-line' if expect_full else 'general'} kernel"
    if family == "balanced":
        x, m, a = _balanced(g, rows, c)
        assert {0.0, 64.0} <= set(m.abs().flatten().tolist()), f"{what}: needs a row with mean 0 and one with |mean| = 64"
        assert c * float(x.abs().max()) < EXACT and c * float((x * x).max() if kind else (a * a).max()) < EXACT, f"{what}: precondition — the sums are not exact in fp32"
        if kind == 0:
            assert torch.equal(x.sum(-1, keepdim=True), c * m) and torch.equal(((x - m) ** 2).sum(-1, keepdim=True), c * a * a)
        else:
            assert torch.equal((x * x).sum(-1, keepdim=True), c * (m * m + a * a))
    else:
        assert family == "census" and rows >= c // 8, f"{what}: every chunk position must be the only carrier once"
        r = torch.arange(rows, device=dev)
        v = torch.exp2(((r // (c // 8) + r) % 7 - 2).double())                      # 1/4 .. 16
        x = torch.zeros(rows, c, dtype=torch.float64, device=dev)
        x.view(rows, c // 8, 8)[r, r % (c // 8)] = v[:, None]
        assert int((x != 0).sum()) == 8 * rows
    assert _exact_in(x, td), f"{what}: precondition — the inputs are not exact in the storage type"
    gamma = beta = ms = mh = ms_rows = mh_rows = None
    if affine:
        gamma = _signed(g, (c,), 0.5, 1.5).float()
        beta = _signed(g, (c,), 2.0, 4.0).float() if kind == 0 and family == "balanced" else None      # census: factors only, so that the
    if modulate:
        rows_per = rows_per or max(rows // 2, 1)
        nmod = (rows + rows_per - 1) // rows_per
        ms = (torch.rand((nmod, c), generator=g, device=dev) - 0.5).to(td)
        mh = _signed(g, (nmod, c), 9.0, 12.0).to(td) if family == "balanced" else None               # small values of the empty chunks stay visible in T
        which = torch.arange(rows, device=dev) // rows_per
        ms_rows, mh_rows = ms[which], (mh[which] if mh is not None else None)
    ref = _norm_formula(x, c, kind, gamma, beta, ms_rows, mh_rows, torch.float64)
    f32 = _norm_formula(x, c, kind, gamma, beta, ms_rows, mh_rows, torch.float32)
    gap, slack, denom = _slack(f32, ref, dtype, what)
    del f32, ms_rows, mh_rows

    pb = PlanBuilder(lib, dev, dtype)
    xb = pb.buf((rows, c + ldx_extra), td)
    xb.fill_(GARBAGE)
    xb[:, :c] = x.to(td)
    yb = pb.buf((rows, c + ldy_extra), td)
    yb.fill_(SENTINEL)

    def vec(v_):
        if v_ is None:
            return None
        if not misaligned:
            t = pb.const(v_)
            assert t.data_ptr() % 16 == 0
            return t
        t = pb.const(torch.cat([v_.new_zeros(1), v_]))[1:]
        assert t.data_ptr() % 16 == 4, "meant for the scalar affine path"
        return t
    pb.norm(xb, yb, rows, c, ldx=c + ldx_extra, ldy=c + ldy_extra, gamma=vec(gamma), beta=vec(beta), eps=1e-6, kind=kind,
            mod_scale=pb.const(ms) if modulate else None, mod_shift=pb.const(mh) if mh is not None else None,
            rows_per=rows_per if modulate else 0, ldmod=c if modulate else 0)
    _run(pb)
    assert bool((yb[:, c:] == SENTINEL).all()), f"{what}: the padding columns of y were written"
    return _assert_bound(yb[:, :c], ref, denom, gap, slack, dtype, what, "norm.exact.fp32_gap")


def check_norm_forms_equal(lib, dtype, rows, c, kind=0, seed=0):
    """csrc/norm.hip: the straight-line kernel and the general one give identical bytes — the same modulated rows once plainly and once with gamma = 1"""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator(device=dev).manual_seed(seed)
    assert norm_is_full_form(c, False) and not norm_is_full_form(c, True)
    x = (torch.randn(rows, c, generator=g, device=dev) * 2 + 0.5).to(td)
    rows_per = max(rows // 2, 1)
    nmod = (rows + rows_per - 1) // rows_per
    ms, mh = torch.randn(nmod, c, generator=g, device=dev).to(td), torch.randn(nmod, c, generator=g, device=dev).to(td)
    pb = PlanBuilder(lib, dev, dtype)
    xt, mst, mht = pb.const(x), pb.const(ms), pb.const(mh)
    outs = []
    for gamma in (None, pb.const(torch.ones(c, device=dev))):
        y = pb.buf((rows, c), td)
        y.fill_(SENTINEL)
        pb.norm(xt, y, rows, c, gamma=gamma, eps=1e-6, kind=kind, mod_scale=mst, mod_shift=mht, rows_per=rows_per, ldmod=c)
        outs.append(y)
    _run(pb)
    assert bool(torch.isfinite(outs[0].float()).all()) and float(outs[0].float().abs().max()) > 1.0
    assert torch.equal(outs[0], outs[1]), f"norm {rows}x{c}: {int((outs[0] != outs[1]).sum())} elements differ between the straight-line and the general kernel"


NORM_CASES = [
    dict(rows=5, c=8, affine=True, expect_full=False),
    dict(rows=7, c=144, affine=True, expect_full=False),
    dict(rows=6, c=1024, modulate=True, expect_full=True),                                # NCH = 2
    dict(rows=5, c=1536, modulate=True, expect_full=False),                               # whole 512-chunks, three per lane: NCH = 4, not FULL
    dict(rows=7, c=3072, modulate=True, rows_per=3, expect_full=True),                    # three modulation rows, the last one short
    dict(rows=5, c=4096, affine=True, expect_full=False),                                 # NCH = 12, not FULL
    dict(rows=7, c=5120, affine=True, modulate=True, rows_per=4, expect_full=False),
    dict(rows=6, c=6144, expect_full=True),
    dict(rows=7, c=144, kind=1, affine=True),                                             # RMSNorm
    dict(rows=5, c=3072, kind=1, modulate=True, rows_per=2, expect_full=True),
    dict(rows=7, c=144, affine=True, ldx_extra=8, ldy_extra=16),
    dict(rows=6, c=1024, modulate=True, ldx_extra=16, ldy_extra=8, expect_full=True),
    dict(rows=7, c=144, affine=True, misaligned=True),                                    # the scalar affine path
    dict(rows=5, c=1536, affine=True, misaligned=True, modulate=True),
    dict(rows=18, c=144, family="census", affine=True),
    dict(rows=384, c=3072, family="census", modulate=True, rows_per=100, expect_full=True),
    dict(rows=640, c=5120, family="census", affine=True, expect_full=False),
    dict(rows=768, c=6144, family="census", expect_full=True),
]
NORM_CASES_GPU = [
    dict(rows=8704, c=3072, modulate=True, rows_per=4352, expect_full=True),
    dict(rows=4001, c=1152, affine=True, expect_full=False),
]


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------
def _groupnorm_formula(x, groups, gamma, beta, dt):
    """x [n, hw, c] -> (x - mean_g) * rstd_g * gamma + beta with two-pass statistics per (image, group), in precision dt"""
    n, hw, c = x.shape
    cg = c // groups
    xg = x.to(dt).view(n, hw, groups, cg).permute(0, 2, 1, 3).reshape(n, groups, hw * cg)      # one contiguous row per (image, group)
    d = xg - xg.mean(-1, keepdim=True)
    t = d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS))
    t = t.view(n, groups, hw, cg).permute(0, 2, 1, 3).reshape(n, hw, c) * gamma.to(dt)
    return t + beta.to(dt) if beta is not None else t


def check_groupnorm_exact(lib, dtype, n, h, w, c, groups, family="balanced", seed=0):
    """balanced groups or the pixel census (module docstring), gn_stats / gn_finalize / gn_apply without SiLU.  Census: image i is zero except for
    pixel i of the positions 0, PIX - 1, PIX, two in between and hw - 1 (PIX = MTX_GN_PIX_PER_BLOCK), whose channels all hold a power of two."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)      # inputs, references and the fp32 gap on the host: the same preconditions on the simulator and on hardware
    hw, cg, pix = h * w, c // groups, abi.GN_PIX_PER_BLOCK
    what = f"groupnorm {family} {n}x{h}x{w}x{c} / {groups}"
    assert hw % pix and hw > pix, f"{what}: needs a ragged last statistics block"
    if family == "balanced":
        v, m, a = _balanced(g, n * groups, cg * hw)
        x = v.view(n, groups, hw, cg).permute(0, 2, 1, 3).reshape(n, hw, c).contiguous()
        assert {0.0, 64.0} <= set(m.abs().flatten().tolist())
        blocks = F.pad(x * x, (0, 0, 0, -hw % pix)).view(n, -1, pix, c).sum(2)
        assert float(blocks.max()) < EXACT, f"{what}: precondition — a workgroup's fp32 partial of x^2 reaches {float(blocks.max())}"
        xg = x.view(n, hw, groups, cg)
        mg, ag, cnt = m.view(n, groups), a.view(n, groups), float(cg * hw)             # integer sums: exact in float64 whatever the order of a reduction
        assert torch.equal(xg.sum(dim=(1, 3)), cnt * mg) and torch.equal((xg * xg).sum(dim=(1, 3)), cnt * (mg * mg + ag * ag)), f"{what}: mean != m or var != a^2"
    else:
        positions = [0, pix - 1, pix, hw - 1, pix // 3, pix + (hw - pix) // 2]
        assert family == "census" and n >= 6 and len(set(positions)) == 6 and max(positions) == hw - 1
        x = torch.zeros(n, hw, c, dtype=torch.float64)
        for i in range(n):
            x[i, positions[i % 6]] = 2.0 ** (i % 5 - 1)
        assert int((x != 0).sum()) == n * c
    assert _exact_in(x, td), f"{what}: precondition — the inputs are not exact in the storage type"
    gamma = _signed(g, (c,), 0.5, 1.5).float()
    beta = _signed(g, (c,), 2.0, 4.0).float() if family == "balanced" else None         # census: a factor only, so that the small values of the empty pixels stay visible in T
    ref = _groupnorm_formula(x, groups, gamma, beta, torch.float64)
    gap, slack, denom = _slack(_groupnorm_formula(x, groups, gamma, beta, torch.float32), ref, dtype, what)
    pb = PlanBuilder(lib, dev, dtype)
    xa = pb.act(n, h, w, c)
    xa.t.copy_(x.view(n, h, w, c).to(td))
    out = pb.buf((n + 1, h, w, c), td)
    out.fill_(SENTINEL)
    pb.groupnorm(xa, pb.const(gamma), pb.const(beta) if beta is not None else None, groups, 1e-6, abi.ACT_NONE, out=Act(out[:n], n, h, w, c))
    _run(pb)
    assert bool((out[n:] == SENTINEL).all()), f"{what}: written beyond the last image"
    return _assert_bound(out[:n].view(n, hw, c).cpu(), ref, denom, gap, slack, dtype, what, "groupnorm.exact.fp32_gap")


GROUPNORM_CASES = [
    dict(n=2, h=40, w=30, c=128, groups=32),                        # four channels per group: a 16-byte chunk spans two groups
    dict(n=2, h=33, w=35, c=256, groups=32),
    dict(n=1, h=40, w=30, c=512, groups=32),
    dict(n=2, h=33, w=35, c=64, groups=1),
    dict(n=6, h=40, w=30, c=128, groups=32, family="census"),
    dict(n=7, h=33, w=35, c=256, groups=32, family="census"),
    dict(n=6, h=33, w=35, c=512, groups=32, family="census"),
    dict(n=6, h=40, w=30, c=64, groups=1, family="census"),
]


# ---- element-wise kinds -------------------------------------------------------------------------------------------------------------------
EW_THREAD_CAP = 2048 * 4 * 256          # ew_launch (csrc/elementwise.hip): at most this many threads, one 16-byte chunk per thread and trip


def _nonzero_ints(g, shape, r):
    """integers in [-r, -1] and [1, r]: a zero in the output can only be padding"""
    return (torch.randint(1, r + 1, shape, generator=g, device=g.device) * (torch.randint(0, 2, shape, generator=g, device=g.device) * 2 - 1)).double()


class _Ew:
    """one plan of element-wise launches: inputs as channel slices of wider buffers with garbage around them, outputs as slices of sentinel-filled buffers
    with one spare image behind them; after the run every output equals its float64 reference and every sentinel survives"""

    def __init__(self, lib, dtype):
        self.lib, self.dtype, self.dev, self.td = lib, dtype, _dev(lib), TD[dtype]
        self.host = torch.device("cpu")          # operands and references are made on the host: the same numbers on the simulator and on hardware
        self.pb = PlanBuilder(lib, self.dev, dtype)
        self.checks = []

    def inp(self, v, c0=0, extra=8):
        """v [n, h, w, c] float64 -> Act over channels [c0, c0 + c) of a buffer `extra` channels wider"""
        assert _exact_in(v, self.td), "precondition — an operand is not exact in the storage type"
        n, h, w, c = v.shape
        t = self.pb.buf((n, h, w, c0 + c + extra), self.td)
        t.fill_(GARBAGE)
        t[..., c0:c0 + c] = v.to(self.td)
        return Act(t, n, h, w, c, c0)

    def out(self, n, h, w, c, c0=0, extra=8, spare=1):
        t = self.pb.buf((n + spare, h, w, c0 + c + extra), self.td)
        t.fill_(SENTINEL)
        return Act(t[:n], n, h, w, c, c0), t

    def expect(self, out, ref, what, whole=None):
        """out: an Act (or a 2-D tensor) the launch writes; ref: float64, already rounded to T where the op rounds; whole: the sentinel-filled buffer around it"""
        self.checks.append((out, ref, what, whole))

    def run(self):
        _run(self.pb)
        for out, ref, what, whole in self.checks:
            got = out.torch() if isinstance(out, Act) else out
            assert tuple(got.shape) == tuple(ref.shape), f"{what}: output shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
            _assert_equal(got.cpu(), ref, f"{what} [{NAME[self.dtype]}]")
            if whole is not None:
                keep = torch.ones(whole.shape[-1], dtype=torch.bool, device=whole.device)
                if isinstance(out, Act):
                    keep[out.c0:out.c0 + out.c] = False
                    rows = out.n
                else:
                    keep[:out.shape[-1]] = False
                    rows = out.shape[0]
                assert bool((whole[:rows][..., keep] == SENTINEL).all()), f"{what}: columns outside the output slice were written"
                assert bool((whole[rows:] == SENTINEL).all()), f"{what}: written beyond the last output row"


def check_ew_copy_gather(lib, dtype, seed=0):
    """MTX_EW_COPY channel slice -> channel slice (the YOLO concat pattern: c0 > 0 on both sides, ld != c); MTX_EW_ROW_GATHER by a permutation and by a
    map with repeats, lda != ldy"""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    n, h, w, c = 2, 5, 7, 24
    x = _nonzero_ints(g, (n, h, w, c), 120)
    o, whole = e.out(n, h, w, c, c0=16, extra=8)
    e.pb.ew(abi.EW_COPY, e.inp(x, c0=8, extra=16), out=o, label="copy")
    e.expect(o, x, "copy slice -> slice", whole)
    src_rows, rows, cc = 45, 37, 40
    src = _nonzero_ints(g, (src_rows, cc), 120)
    for name, idx in (("permutation", torch.randperm(src_rows, generator=g, device=e.host)[:rows]),
                      ("repeats", torch.randint(0, 5, (rows,), generator=g, device=e.host) * 9)):
        assert (name == "repeats") == (len(set(idx.tolist())) < rows) and bool((idx != torch.arange(rows, device=e.host)).any())
        a = e.inp(src.view(1, 1, src_rows, cc), extra=24)                               # lda = 64
        dst = e.pb.buf((rows + 3, cc + 8), e.td)                                        # ldy = 48
        dst.fill_(SENTINEL)
        e.pb.row_gather(a.t, dst, e.pb.hold(idx.to(torch.int32).to(e.dev)), rows, cc, lda=a.ld, ldy=dst.shape[-1])
        e.expect(dst[:rows, :cc], src[idx], f"row_gather ({name})", dst)
    e.run()


def _im2col_ref(x, k, s):
    """[n, h, w, c] -> ([n * oh * ow, k * k * c] in the tap-major column order tap * c + ch, oh, ow) from F.unfold, whose own order is ch * k * k + tap;
    the order is then checked against the definition of MTX_EW_IM2COL (include/mtx_hip.h), tap by tap"""
    n, h, w, c = x.shape
    pd = k // 2
    u = F.unfold(x.permute(0, 3, 1, 2), k, padding=pd, stride=s)
    oh, ow = (h + 2 * pd - k) // s + 1, (w + 2 * pd - k) // s + 1
    assert u.shape == (n, c * k * k, oh * ow)
    ref = u.view(n, c, k * k, oh * ow).permute(0, 3, 2, 1).reshape(n * oh * ow, k * k * c)
    r5 = ref.view(n, oh, ow, k * k, c)
    xp = F.pad(x, (0, 0, pd, pd, pd, pd))
    for tap in range(k * k):
        ky, kx = tap // k, tap % k
        want = xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s]
        assert torch.equal(r5[:, :, :, tap], want), f"the im2col reference is not in the column order tap * C + c (tap {tap})"
    return ref, oh, ow


def check_ew_im2col(lib, dtype, seed=0):
    """MTX_EW_IM2COL: k = 1 and 3, stride 1 and 2, odd h and w, with a row map (a subset of the output pixels in shuffled order, some twice) and without, ldy > k * k * C"""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    for k, s, n, h, w, c, mapped in ((3, 1, 2, 7, 9, 16, False), (3, 2, 2, 7, 9, 16, True), (1, 1, 1, 5, 7, 24, True), (1, 2, 2, 5, 7, 8, False),
                                     (3, 2, 1, 8, 6, 8, False), (3, 1, 1, 9, 5, 24, True)):
        x = _nonzero_ints(g, (n, h, w, c), 120)
        ref, oh, ow = _im2col_ref(x, k, s)
        rows = n * oh * ow
        idx = None
        if mapped:
            sub = torch.randperm(rows, generator=g, device=e.host)[:rows * 2 // 3]
            idx = torch.cat([sub, sub])[:rows]
            assert len(set(idx.tolist())) < rows and bool((idx != torch.arange(rows, device=e.host)).any())
            ref = ref[idx]
        ldy = k * k * c + 8
        dst = e.pb.buf((rows + 2, ldy), e.td)
        dst.fill_(SENTINEL)
        e.pb.im2col(e.inp(x, c0=8), dst, k, s, ldy, row_map=e.pb.hold(idx.to(torch.int32).to(e.dev)) if mapped else None)
        e.expect(dst[:rows, :k * k * c], ref, f"im2col k{k} s{s} {n}x{h}x{w}x{c}{' mapped' if mapped else ''}", dst)
    e.run()


def _im2col_patch_ref(x, k, s):
    """_im2col_ref without padding (MTX_EW_IM2COL_PATCH): oh = (h - k) // s + 1, the pixels a last partial patch would need are dropped"""
    n, h, w, c = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), k, padding=0, stride=s)
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    assert u.shape == (n, c * k * k, oh * ow)
    ref = u.view(n, c, k * k, oh * ow).permute(0, 3, 2, 1).reshape(n * oh * ow, k * k * c)
    r5 = ref.view(n, oh, ow, k * k, c)
    for tap in range(k * k):
        ky, kx = tap // k, tap % k
        want = x[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s]
        assert torch.equal(r5[:, :, :, tap], want), f"the im2col_patch reference is not in the column order tap * C + c (tap {tap})"
    return ref, oh, ow


def check_ew_im2col_patch(lib, dtype, seed=0):
    """MTX_EW_IM2COL_PATCH, the unpadded im2col behind the patch embeddings: k = s in {2, 4, 14} and k != s (3 / 2), h and w that leave remainder pixels,
    h == k, C = 8 and 24, ldy > k * k * C, without a row map, with a shuffled one (a subset, some rows twice) and with the window-major order of
    sam_common.window_order for a 4 x 4 grid of 2 x 2 windows (SAM 3's patch embedding); an image smaller than the patch is refused"""
    import pytest
    from mangatranslator_amd.core.ml.sam_common import window_order
    from mangatranslator_amd.utils.exceptions import ModelError
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    for k, s, n, h, w, c, mapped in ((2, 2, 2, 16, 16, 8, "windows"), (2, 2, 1, 5, 7, 24, None), (4, 4, 1, 9, 14, 24, "shuffled"), (4, 4, 2, 4, 19, 8, None),
                                     (14, 14, 1, 14, 30, 8, "shuffled"), (14, 14, 2, 29, 15, 8, None), (3, 2, 2, 8, 7, 8, None), (3, 2, 1, 3, 10, 24, "shuffled")):
        x = _nonzero_ints(g, (n, h, w, c), 120)
        ref, oh, ow = _im2col_patch_ref(x, k, s)
        assert (oh, ow) == ((h - k) // s + 1, (w - k) // s + 1) and oh >= 1 and ow >= 1
        rows = n * oh * ow
        idx = None
        if mapped == "windows":
            assert (oh, ow) == (8, 8)
            order = torch.from_numpy(window_order(oh, ow, 2))
            assert order[:4].tolist() == [0, 1, 8, 9] and sorted(order.tolist()) == list(range(64))           # the first window: two tokens of row 0, two of row 1
            idx = torch.cat([order + i * oh * ow for i in range(n)])
        elif mapped == "shuffled":
            sub = torch.randperm(rows, generator=g, device=e.host)[:max(rows * 2 // 3, 1)]
            idx = torch.cat([sub, sub])[:rows]
            assert rows < 2 or (len(set(idx.tolist())) < rows and bool((idx != torch.arange(rows, device=e.host)).any()))
        if idx is not None:
            ref = ref[idx]
        ldy = k * k * c + 8
        dst = e.pb.buf((rows + 2, ldy), e.td)
        dst.fill_(SENTINEL)
        e.pb.im2col(e.inp(x, c0=8), dst, k, s, ldy, row_map=e.pb.hold(idx.to(torch.int32).to(e.dev)) if idx is not None else None, pad=False)
        e.expect(dst[:rows, :k * k * c], ref, f"im2col_patch k{k} s{s} {n}x{h}x{w}x{c}{' ' + mapped if mapped else ''}", dst)
    e.run()
    for h, w in ((3, 9), (9, 3)):                                                          # csrc/elementwise.hip, ew_launch: nothing is launched
        r = _Ew(lib, dtype)
        dst = r.pb.buf((4, 4 * 4 * 8 + 8), r.td)
        dst.fill_(SENTINEL)
        r.pb.im2col(r.inp(_nonzero_ints(g, (1, h, w, 8), 120)), dst, 4, 4, dst.shape[-1], pad=False)
        with pytest.raises(ModelError, match="elementwise: im2col_patch needs an image of at least k x k"):
            _run(r.pb)
        assert bool((dst == SENTINEL).all()), "a refused im2col_patch wrote"


def check_ew_im2col_patch_embed(lib, dtype, seed=0):
    """A patch embedding as the ViT graphs build it — packing.patch_embed_rows(w), MTX_EW_IM2COL_PATCH on a 3-channel image padded to 8 channels, one GEMM —
    equals F.conv2d(x, w, stride=p) rounded once to T: integer pixels and weights under precondition (a) of check_gemm_exact (every partial sum exact in
    fp32).  The padding channels hold GARBAGE, which the zero columns of the packed filter must cancel; h and w leave remainder pixels."""
    from mangatranslator_amd.core.ml.packing import patch_embed_rows
    host, dev, td = torch.device("cpu"), _dev(lib), TD[dtype]
    g = torch.Generator(device=host).manual_seed(seed)
    for p, n, h, w, cout in ((4, 2, 18, 11, 24), (14, 1, 30, 43, 40)):
        what = f"patch embedding p{p} {n}x{h}x{w} -> {cout}"
        r, alpha = operand_range(dtype, p * p * 3)
        x, wt = _ints(g, (n, h, w, 3), r), _ints(g, (cout, 3, p, p), r)
        assert p * p * 3 * float(x.abs().max()) * float(wt.abs().max()) * alpha < EXACT, f"{what}: precondition (a)"
        ref = _round(F.conv2d(x.permute(0, 3, 1, 2), wt, stride=p).permute(0, 2, 3, 1) * alpha, td)
        oh, ow = ref.shape[1], ref.shape[2]
        assert (oh, ow) == (h // p, w // p) and h % p and w % p
        _assert_rounding_share(ref, dtype, what)
        pb = PlanBuilder(lib, dev, dtype)
        xb = pb.act(n, h, w, 8)
        xb.t.fill_(GARBAGE)
        xb.t[..., :3] = x.to(td)
        wk = patch_embed_rows(wt.float())
        assert wk.shape == (cout, p * p * 8) and bool((wk.view(cout, p * p, 8)[:, :, 3:] == 0).all())
        rows, kk = n * oh * ow, p * p * 8
        cols = pb.buf((rows, kk), td)
        cols.fill_(SENTINEL)
        pb.im2col(xb, cols, p, p, kk, pad=False)
        out = pb.gemm(cols, pb.const(wk, td), rows, cout, kk, alpha=alpha)
        _run(pb)
        _assert_equal(out.view(n, oh, ow, cout).cpu(), ref, f"{what} [{NAME[dtype]}]")


def check_ew_resample(lib, dtype, seed=0):
    """MTX_EW_UPSAMPLE2X with and without b; MTX_EW_MAXPOOL 5/1, 2/2 on odd sizes, 3/2 on odd and even sizes, the SPPF chain inside one buffer, an all-negative
    input; MTX_EW_AVGPOOL2 (ceil mode, divisor = the taps inside) on h odd, w odd, both odd and 1 x 1"""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    nchw = lambda v: v.permute(0, 3, 1, 2)
    nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()
    n, h, w, c = 2, 5, 7, 24
    x = _nonzero_ints(g, (n, h, w, c), 120)
    up = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    o, whole = e.out(n, 2 * h, 2 * w, c, c0=8)
    e.pb.ew(abi.EW_UPSAMPLE2X, e.inp(x), out=o)
    e.expect(o, up, "upsample2x", whole)
    b = _ints(g, (n, 2 * h, 2 * w, c), INT_CAP[dtype])
    big = _ints(g, (n, h, w, c), INT_CAP[dtype])
    o, whole = e.out(n, 2 * h, 2 * w, c)
    e.pb.ew(abi.EW_UPSAMPLE2X, e.inp(big), b=e.inp(b, c0=16), out=o)
    e.expect(o, _round(big.repeat_interleave(2, 1).repeat_interleave(2, 2) + b, e.td), "upsample2x + b", whole)

    for k, s, hh, ww, negative in ((5, 1, 5, 7, False), (5, 1, 6, 4, True), (2, 2, 5, 7, False), (2, 2, 9, 3, True), (3, 2, 7, 9, False), (3, 2, 8, 6, False),
                                   (3, 2, 7, 6, True)):
        v = _nonzero_ints(g, (n, hh, ww, c), 120)
        if negative:
            v = -v.abs()
        ref = nhwc(F.max_pool2d(nchw(v), k, s, k // 2 if k % 2 else 0))
        oh, ow = ref.shape[1], ref.shape[2]
        o, whole = e.out(n, oh, ow, c, c0=8, spare=-(-n * (oh + 1) * (ow + 1) // (oh * ow)) - n)      # room for one more output row and column: a wrong size must not leave the buffer
        e.pb.ew(abi.EW_MAXPOOL, e.inp(v, c0=8), out=o, i0=k, i1=s)
        e.expect(o, ref, f"maxpool {k}/{s} {hh}x{ww}{' all negative' if negative else ''}", whole)
    # SPPF: slice j -> slice j + 1 of one buffer, three times
    cat, whole = e.out(n, h, w, 4 * c, extra=8)
    cat.t[..., :c] = x.to(e.td)
    refs = [x]
    for j in range(3):
        e.pb.ew(abi.EW_MAXPOOL, cat.slice(j * c, c), out=cat.slice((j + 1) * c, c), i0=5, i1=1)
        refs.append(nhwc(F.max_pool2d(nchw(refs[-1]), 5, 1, 2)))
    e.expect(cat, torch.cat(refs, -1), "maxpool 5/1, the SPPF chain", whole)

    for hh, ww in ((5, 6), (4, 7), (7, 9), (1, 1), (1, 4)):
        v = _ints(g, (n, hh, ww, c), 64) * 4.0
        ref = nhwc(F.avg_pool2d(nchw(v), 2, 2, ceil_mode=True, count_include_pad=False))
        assert _exact_in(ref, e.td), "avgpool2: the averages of multiples of 4 over 1, 2 or 4 taps are integers the storage type holds"
        o, whole = e.out(n, (hh + 1) // 2, (ww + 1) // 2, c, c0=8)
        e.pb.ew(abi.EW_AVGPOOL2, e.inp(v), out=o)
        e.expect(o, ref, f"avgpool2 {hh}x{ww}", whole)
    e.run()


def check_ew_dwconv(lib, dtype, seed=0):
    """MTX_EW_DWCONV: k = 3 and 7, integer weights and bias, ACT_NONE and ACT_RELU, C = 8 and 72, an image smaller than the kernel; sums inside T's integer
    range (plain equality) and beyond it (one rounding, at least 20 % of the outputs where T rounds)"""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    wide, _ = operand_range(dtype, 49, with_alpha=False, spread=2.0)
    for k, n, h, w, c, act, r, beyond in ((3, 2, 9, 11, 8, abi.ACT_NONE, 3, False), (3, 1, 6, 5, 72, abi.ACT_RELU, 3, False),
                                          (7, 1, 5, 6, 8, abi.ACT_RELU, 2, False), (7, 1, 5, 6, 72, abi.ACT_NONE, 2, False),
                                          (7, 2, 13, 15, 72, abi.ACT_NONE, wide, True), (7, 1, 16, 12, 8, abi.ACT_RELU, wide, True)):
        what = f"dwconv k{k} {n}x{h}x{w}x{c} act {act}"
        x, wt = _ints(g, (n, h, w, c), r), _ints(g, (c, 1, k, k), r)
        bias = _ints(g, (c,), 64)
        reach = min(k, h) * min(k, w) * r * r + 64
        assert reach < EXACT
        v = F.conv2d(x.permute(0, 3, 1, 2), wt, bias, padding=k // 2, groups=c).permute(0, 2, 3, 1)
        if act == abi.ACT_RELU:
            v = v.clamp_min(0.0)
        if beyond:
            ref = _round(v, e.td)
            _assert_rounding_share(ref, dtype, what)
        else:
            assert reach <= INT_CAP[dtype], f"{what}: meant to stay inside the storage type's integer range"
            ref = v
        o, whole = e.out(n, h, w, c, c0=8)
        taps = e.pb.const(wt.view(c, k * k).t().contiguous().to(e.td))                  # [k * k][C], tap = dy * k + dx
        e.pb.dwconv(e.inp(x, c0=16), taps, e.pb.const(bias.float()), k, act=act, out=o)
        e.expect(o, ref, what, whole)
    e.run()


def check_ew_arith(lib, dtype, seed=0):
    """MTX_EW_ADD / SUB / MUL / SCALE_RES / GATE_RES on integers, three images, ldb != c: one rounding of the exact result.  s of SCALE_RES (fp32 powers of two)
    and of GATE_RES (T) is indexed by IMAGE, s[n * lds + c] — GATE_RES by rows_per is spelled as n = rows / rows_per images of rows_per pixels."""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.host).manual_seed(seed)
    n, h, w, c = 3, 5, 7, 24
    cap = INT_CAP[dtype]
    a, b = _ints(g, (n, h, w, c), cap), _ints(g, (n, h, w, c), cap)
    f = int(cap ** 0.5) * 3
    fa, fb = _ints(g, (n, h, w, c), f), _ints(g, (n, h, w, c), f)
    lds = c + 8
    s32 = torch.zeros(n, lds, dtype=torch.float64, device=e.host)
    s32[:, :c] = torch.exp2(torch.randint(-2, 4, (n, c), generator=g, device=e.host).double())
    gate = torch.zeros(n, lds, dtype=torch.float64, device=e.host)
    gate[:, :c] = _ints(g, (n, c), f)
    assert not torch.equal(s32[0], s32[1]) and not torch.equal(gate[1], gate[2]), "the per-image index of s must matter"
    sb, gb = s32[:, None, None, :c], gate[:, None, None, :c]
    cases = (("add", abi.EW_ADD, a, b, None, a + b), ("sub", abi.EW_SUB, a, b, None, a - b), ("mul", abi.EW_MUL, fa, fb, None, fa * fb),
             ("scale_res", abi.EW_SCALE_RES, a, b, e.pb.const(s32.float()), a * sb + b),
             ("gate_res", abi.EW_GATE_RES, fa, b, e.pb.const(gate.to(e.td)), b + fa * gb))
    for name, kind, va, vb, s, v in cases:
        assert float(v.abs().max()) * 4 < EXACT
        ref = _round(v, e.td)
        assert float((ref != v).double().mean()) > 0.05, f"{name}: precondition — hardly any result needs rounding"
        o, whole = e.out(n, h, w, c, c0=8)
        e.pb.ew(kind, e.inp(va, c0=8), b=e.inp(vb, extra=16), s=s, out=o, lds=lds if s is not None else 0)
        e.expect(o, ref, name, whole)
    # GATE_RES by token rows (the DiT form): 3 * 35 rows, rows_per = 35
    rows = n * h * w
    o, whole = e.out(n, 1, h * w, c)
    e.pb.ew(abi.EW_GATE_RES, e.inp(fa.view(n, 1, h * w, c)), b=e.inp(b.view(n, 1, h * w, c)), s=e.pb.const(gate.to(e.td)), out=o, lds=lds)
    e.expect(o, _round(b + fa * gb, e.td).view(n, 1, h * w, c), f"gate_res over {rows} rows, rows_per {h * w}", whole)
    o, whole = e.out(1, 1, rows, c, c0=8)                                                # lds = 0: one gate row for every image (the YOLO layer scale)
    e.pb.ew(abi.EW_GATE_RES, e.inp(fa.view(1, 1, rows, c)), b=e.inp(b.view(1, 1, rows, c)), s=e.pb.const(gate[2].to(e.td)), out=o, lds=0)
    e.expect(o, _round(b + fa * gate[2, :c], e.td).view(1, 1, rows, c), "gate_res, one row of s", whole)
    e.run()


def check_ew_grid_stride(lib, dtype, seed=0):
    """more 16-byte chunks than ew_launch starts threads: the grid-stride loop takes a second trip (a channel-slice copy, compared in T)"""
    e = _Ew(lib, dtype)
    g = torch.Generator(device=e.dev).manual_seed(seed)
    rows, c = 16400, 1024
    assert EW_THREAD_CAP < rows * c // 8 < 2 * EW_THREAD_CAP
    src = e.pb.buf((1, 1, rows, c + 16), e.td)
    src.copy_(torch.randint(-120, 121, src.shape, generator=g, device=e.dev))
    o, whole = e.out(1, 1, rows, c, c0=8)
    e.pb.ew(abi.EW_COPY, Act(src, 1, 1, rows, c, 8), out=o)
    _run(e.pb)
    bad = int((o.torch() != src[..., 8:8 + c]).sum())
    assert bad == 0, f"copy of {rows * c // 8} chunks: {bad} elements differ"
    assert bool((whole[:1, ..., :8] == SENTINEL).all()) and bool((whole[:1, ..., 8 + c:] == SENTINEL).all()) and bool((whole[1:] == SENTINEL).all())

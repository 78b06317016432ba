"""Exact-arithmetic checks of the matrix-pipe kernels (GEMM, conv, attention) against float64 references.

On integer-valued operands every product and every fp32 partial sum below 2^24 is exact in ANY summation order, so the result of a
GEMM or a conv is one known value per element and the only freedom a kernel has left is WHERE it rounds to the 16-bit storage type.
Those rounding points are a contract (include/mtx_hip.h, mtx_gemm_args / mtx_conv2d_args); here they are restated on a float64
reference — `.float().to(T)` at each documented point — and the kernel's bytes must equal it: zero differing elements.  A wrong
rounding mode, a lost or doubled k element, a K-slice merge that loses bits, a tile written twice: each moves at least one element.

Every case asserts its own preconditions FROM THE REFERENCE ALONE before it looks at the kernel, so a shape that stops testing
anything fails loudly: (a) exactness — the largest possible partial sum is below 2^24; (b) the f16 range — max |ref| < 60000;
(c) at least 20 % of the outputs lie where T really rounds integers (|v| >= 2^8 for bf16, >= 2^11 for f16).

Attention cannot be exact (a division), but on dyadic operands its numerator and denominator are: what is left is ONE rounding to T
plus a few fp32 ulp of the reciprocal — the bound is (0.5 + 2^-10) spacings of T at the reference value.

Same layout as op_checks.py: written once, run on the simulator (small shapes) and on the product library (production shapes)."""
import math

import torch
import torch.nn.functional as F

from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from op_checks import TD, _dev, _run, _sync

EXACT = float(1 << 24)                                   # integers below are exact in fp32, sums of them in any order
ROUNDS_FROM = {abi.BF16: 256.0, abi.F16: 2048.0}         # T's spacing exceeds 1 from here on: integers really get rounded
INT_CAP = {abi.BF16: 256, abi.F16: 2048}                 # every integer up to here is representable in T (bias / residual range)
SIGMA = {abi.BF16: 400.0, abi.F16: 3000.0}               # aimed standard deviation of the accumulators: about half of them beyond ROUNDS_FROM
F16_LIMIT = 60000.0
MANT = {abi.BF16: 7, abi.F16: 10, abi.F32: 23}
MIN_EXP = {abi.BF16: -126, abi.F16: -14, abi.F32: -126}


def _ints(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g, device=g.device).double()


def _round(v, td):
    """one rounding to the storage type, of float64 values that are exact in fp32"""
    return v.float().to(td).double()


def _act(v, act, slope):
    if act == abi.ACT_NONE:
        return v
    if act == abi.ACT_RELU:
        return v.clamp_min(0.0)
    assert act == abi.ACT_LEAKY and math.log2(slope) == int(math.log2(slope)), "exact cases: NONE, RELU, LEAKY with a power-of-two slope"
    return torch.where(v > 0, v, v * slope)


def operand_range(dtype, k, cap=64, with_alpha=True, spread=1.0):
    """integer range r ([-r, r], variance r (r + 1) / 3) and power-of-two alpha that put the standard deviation sqrt(k) r (r + 1) / 3 * alpha
    of a K-long sum of products just above spread * SIGMA[dtype]: the smallest such figure over r <= cap and alpha = 2^j (a conv has no alpha: the smallest r)"""
    best, target = None, spread * SIGMA[dtype]
    for r in range(1, cap + 1):
        s = math.sqrt(k) * r * (r + 1) / 3.0
        alpha = 1.0
        if not with_alpha:
            if s >= target:
                return r, 1.0
            continue
        while s * alpha < target:
            alpha *= 2.0
        if best is None or s * alpha < best[0] or (s * alpha == best[0] and alpha < best[2]):
            best = (s * alpha, r, alpha)
    return best[1], best[2]


def _assert_rounding_share(ref, dtype, what):
    if dtype == abi.F16:
        assert float(ref.abs().max()) < F16_LIMIT, f"{what}: precondition (b) — max |ref| {float(ref.abs().max())} leaves the f16 range"
    share = float((ref.abs() >= ROUNDS_FROM[dtype]).double().mean())
    assert share >= 0.20, f"{what}: precondition (c) — only {share:.1%} of the outputs lie where the storage type rounds"
    return share


def _assert_equal(got, ref, what):
    got = got.double()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ from the float64 reference with the contract's rounding; "
                             f"first at {i}: got {float(got[i])}, want {float(ref[i])}")


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
def check_gemm_exact(lib, dtype, m, n, k, act=abi.ACT_NONE, with_bias=True, with_res=False, with_gate=False, out_f32=False, batch=1,
                     seed=0, flags=0, runs=1, expect_split=None, w_lo=False, res_f32=False, f8=False, slope=0.25):
    """The contract of the 16-bit and fp8-operand GEMM kernels (include/mtx_hip.h, mtx_gemm_args):
         t = act(alpha * acc + bias);  16-bit output: t = round_T(t);  with a gate and / or a residual: c = round_T(t * gate + res), else c = t;
         fp32 output: no rounding at all.
    f8: the operands go through mtx_quantize_mx first (integers in [-7, 7] survive MX e4m3 exactly: the block scale is a power of two and 7
    has three significant bits).  w_lo: W = w + w_lo, both halves integer.  Returns the share of outputs beyond T's integer range."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator(device=dev).manual_seed(seed)          # operands and the float64 reference live on the device: production shapes stay cheap
    what = f"gemm {batch}x{m}x{n}x{k}"
    r, alpha = operand_range(dtype, k * (2 if w_lo else 1), cap=7 if f8 else 64)
    a, w = _ints(g, (batch, m, k), r), _ints(g, (batch, n, k), r)
    wl = _ints(g, (batch, n, k), r) if w_lo else None
    b = _ints(g, (n,), INT_CAP[dtype]) if with_bias else None
    wsum = w + wl if w_lo else w
    bound = k * float(a.abs().max()) * float(wsum.abs().max()) * alpha + (float(b.abs().max()) if b is not None else 0.0)
    assert bound < EXACT, f"{what}: precondition (a) — partial sums up to {bound} are not exact in fp32"
    t = torch.einsum("bmk,bnk->bmn", a, wsum) * alpha
    if b is not None:
        t = t + b
    t = _act(t, act, slope)
    if not out_f32:
        t = _round(t, td)
    gate = res = None
    rows_per = max(m // 2, 1)
    if with_gate:
        gate = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64, device=dev)[torch.randint(0, 4, ((m + rows_per - 1) // rows_per, n), generator=g, device=dev)]
    if with_res:
        res = _ints(g, (batch, m, n), INT_CAP[dtype])
    if gate is not None or res is not None:
        bound = float(t.abs().max()) * (2.0 if gate is not None else 1.0) + (INT_CAP[dtype] if res is not None else 0.0)
        assert bound < EXACT, f"{what}: precondition (a) — the gate / residual stage reaches {bound}"
        if gate is not None:
            t = t * gate.repeat_interleave(rows_per, dim=0)[:m]
        if res is not None:
            t = t + res
        if not out_f32:
            t = _round(t, td)
    ref = t
    share = None if out_f32 else _assert_rounding_share(ref, dtype, what)      # an fp32 output is never rounded: (b) and (c) do not apply

    pb = PlanBuilder(lib, dev, dtype)
    at, wt = pb.const(a.to(td)), pb.const(w.to(td))
    kw = {}
    if f8:
        assert batch == 1 and not w_lo
        at, asc, lds_a = pb.quantize(at, m, k)
        wt, wsc, lds_w = pb.quantize(wt, n, k)
        kw["f8"] = (asc, lds_a, wsc, lds_w, 0, 0)
    if w_lo:
        kw["w_lo"] = pb.const(wl.to(td))
    rt = None
    if res is not None:
        rt = pb.const(res.float() if res_f32 else res.to(td))
    out = pb.gemm(at, wt, m, n, k, bias=pb.const(b.float()) if b is not None else None, act=act, res=rt, res_f32=res_f32,
                  gate=pb.const(gate.to(td)) if gate is not None else None, gate_rows_per=rows_per,
                  alpha=alpha, batch=batch, a_bs=m * k, w_bs=n * k, c_bs=m * n, res_bs=m * n, out_f32=out_f32, flags=flags, **kw)
    getattr(pb.ops[-1].u, abi.UNION_FIELD[abi.OP_GEMM]).act_param = slope
    plan = _run(pb)
    if expect_split is not None:
        got = lib.gemm_last_split()           # None in expect_split = any value; "sliced" = at least two K slices
        ok = all(e is None or (e == "sliced" and s >= 2) or e == s for e, s in zip(expect_split, got))
        assert ok, f"launch split {got} != {tuple(expect_split)}"
    _assert_equal(out.view(batch, m, n), ref, what)
    first = out.clone()
    for _ in range(runs - 1):
        out.fill_(float("nan"))
        plan.run()
        _sync(lib)
        assert torch.equal(out, first), "a second run of the same plan differs (stale scratch read, or an order-dependent sum)"
    return share


def check_gemm_exact_beyond_4gb(lib, dtype, m, n, k, seed=0):
    """rows generated on the device; the row blocks at the start, around the 4 GB byte offset and at the end must equal the float64 product"""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator(device=dev).manual_seed(seed)
    r, alpha = operand_range(dtype, k)
    pb = PlanBuilder(lib, dev, dtype)
    at = pb.buf((m, k), td)
    step = 1 << 16
    for r0 in range(0, m, step):
        at[r0:r0 + step] = torch.randint(-r, r + 1, (min(step, m - r0), k), device=dev, generator=g).to(td)
    w = _ints(torch.Generator().manual_seed(seed + 1), (n, k), r).to(dev)
    assert k * r * r * alpha < EXACT
    out = pb.gemm(at, pb.const(w.to(td)), m, n, k, alpha=alpha)
    _run(pb)
    edge = (1 << 32) // (k * at.element_size())        # first row whose bytes start beyond 4 GB
    assert 300 < edge < m - 517
    for r0 in (0, edge - 300, m - 517):
        rows = slice(r0, r0 + 517)
        ref = _round(at[rows].double() @ w.t() * alpha, td)
        _assert_rounding_share(ref, dtype, f"gemm rows {r0}..")
        _assert_equal(out[rows], ref, f"gemm beyond 4 GB, rows {r0}..")


def gemm_f32_kernel_form(m, k, lda, ldw, a_off=0, a_bs=0, w_bs=0, flags=0):
    """the dispatch rule of gemm_f32_launch (csrc/f32ops.hip), for operands whose buffers start on a 16-byte boundary"""
    if (m <= 128 and k >= 1024 and k % 4 == 0 and lda % 4 == 0 and ldw % 4 == 0 and a_off % 4 == 0 and a_bs % 4 == 0 and w_bs % 4 == 0
            and not flags & abi.GEMM_FORCE_TILE256):
        return "few rows"
    return "matrix pipe" if m >= 256 or flags & abi.GEMM_FORCE_TILE256 else "vector ALU"


GEMM_F32_CASES = [
    dict(form="vector ALU", m=203, n=77, k=50),
    dict(form="vector ALU", m=40, n=24, k=32, bt=3),
    dict(form="matrix pipe", m=300, n=70, k=50, ld_extra=1),                                  # unaligned lda: scalar loads
    dict(form="matrix pipe", m=513, n=129, k=256),
    dict(form="matrix pipe", m=260, n=33, k=18, bt=2),
    dict(form="matrix pipe", m=40, n=9, k=24, flags=abi.GEMM_FORCE_TILE256),
    dict(form="few rows", m=37, n=50, k=1024),
    dict(form="few rows", m=72, n=19, k=2048, bt=2),
    # the shapes the table left out
    dict(form="matrix pipe", m=300, n=70, k=260),                                             # aligned lda: 16-byte loads, then a 4-wide scalar tail in the last K step
    dict(form="matrix pipe", m=260, n=33, k=37, ld_extra=3),                                  # odd K on an aligned lda: the last k pair is half filled
    dict(form="matrix pipe", m=257, n=65, k=37),                                              # odd K, odd lda
    dict(form="few rows", m=37, n=50, k=1028),                                                # K % 256 != 0: the last lane round is partial (one lane)
    dict(form="few rows", m=72, n=19, k=1100, bt=2, res_shared=True),                         # ... (19 lanes); one residual for both batches
    dict(form="vector ALU", m=37, n=50, k=1028, ld_extra=1),                                  # lda % 4 != 0: few rows and a long K, yet the tiled kernel
    dict(form="vector ALU", m=30, n=4, k=8, bt=5, w_bs_extra=5, c_slice=(7, 3)),              # per-batch weights with a batch stride, output into a column slice
    dict(form="matrix pipe", m=260, n=33, k=20, bt=2, w_bs_extra=4, res_shared=True, c_slice=(8, 8)),
    dict(form="few rows", m=9, n=19, k=1024, bt=2, w_bs_extra=8, pick=(3, 2), c_slice=(4, 4)),
    dict(form="vector ALU", m=5, n=16, k=16, pick=(9, 2)),                                    # rows picked out of a wider matrix (a_off, lda)
    dict(form="matrix pipe", m=300, n=24, k=16, pick=(2, 1), res_shared=True, bt=2),
]
_SENTINEL = -123.0


def check_gemm_f32_exact(lib, seed=0):
    """the fp32 GEMM of csrc/f32ops.hip on integer operands: no rounding anywhere, every kernel form check_f32_ops names — the vector-ALU form, the
    matrix-pipe form (from 256 rows up or forced; aligned and unaligned lda, a K that ends inside a 16-byte load, inside a k pair), few rows with a long
    K (whole and partial lane rounds) — with bias, RELU, alpha and a residual; per-batch weights with a batch stride (w_bs_extra), a residual shared by
    all batches (res_shared), rows picked out of a wider matrix (pick = (rows per group NT, which one): lda = NT * row, a_off) and an output into a
    column slice of a sentinel-filled buffer (c_slice = (extra columns, c_off)) with one spare row behind it.  Every case states the kernel form it is
    meant for and asserts it from the dispatch rule."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev(lib)
    pb = PlanBuilder(lib, dev, abi.F32)
    checks = []
    for case in GEMM_F32_CASES:
        cfg = dict(ld_extra=0, bt=1, flags=0, w_bs_extra=None, res_shared=False, pick=None, c_slice=None)
        cfg.update(case)
        m, n, k, bt = cfg["m"], cfg["n"], cfg["k"], cfg["bt"]
        name = ", ".join(f"{key} {v}" for key, v in case.items())
        r = 31
        row = k + cfg["ld_extra"]
        nt, which = cfg["pick"] or (1, 0)
        a_full = _ints(g, (bt, m, nt, row), r)                                               # the unused columns and rows hold integers of the same range
        a, lda, a_off, a_bs = a_full[:, :, which, :k], nt * row, which * row, m * nt * row
        if cfg["w_bs_extra"] is None:
            w_full = _ints(g, (n * k,), r)
            w, w_bs = w_full.view(1, n, k).expand(bt, n, k), 0
        else:
            w_bs = n * k + cfg["w_bs_extra"]
            w_full = _ints(g, (bt, w_bs), r)
            w = w_full[:, :n * k].view(bt, n, k)
            assert bt > 1 and not torch.equal(w[0], w[1])
        b = _ints(g, (n,), 4096)
        res = _ints(g, (m, n) if cfg["res_shared"] else (bt, m, n), 4096)
        assert k * r * r * 0.5 + 4096 + 4096 < EXACT
        form = gemm_f32_kernel_form(m, k, lda, k, a_off, a_bs, w_bs, cfg["flags"])
        assert form == cfg["form"], f"fp32 gemm ({name}): the case is meant for the {cfg['form']} kernel, the dispatch rule gives {form}"
        ref = F.relu(torch.einsum("bmk,bnk->bmn", a, w) * 0.5 + b) + res
        whole = None
        if cfg["c_slice"]:
            extra, c_off = cfg["c_slice"]
            ldc = n + extra
            assert c_off + n <= ldc
            whole = pb.buf((bt * m + 1, ldc), torch.float32)
            whole.fill_(_SENTINEL)
            pb.gemm(pb.const(a_full.float()), pb.const(w_full.float()), m, n, k, lda=lda, a_off=a_off, out=whole, ldc=ldc, c_off=c_off, bias=pb.const(b.float()),
                    act=abi.ACT_RELU, res=pb.const(res.float()), batch=bt, a_bs=a_bs, w_bs=w_bs, c_bs=m * ldc, res_bs=0 if cfg["res_shared"] else m * n,
                    alpha=0.5, flags=cfg["flags"])
            out = whole[:bt * m, c_off:c_off + n]
        else:
            out = pb.gemm(pb.const(a_full.float()), pb.const(w_full.float()), m, n, k, lda=lda, a_off=a_off, bias=pb.const(b.float()), act=abi.ACT_RELU,
                          res=pb.const(res.float()), batch=bt, a_bs=a_bs, w_bs=w_bs, c_bs=m * n, res_bs=0 if cfg["res_shared"] else m * n, alpha=0.5,
                          flags=cfg["flags"])
        checks.append((name, out, ref, (bt, m, n), whole, cfg["c_slice"]))
    _run(pb)
    for name, out, ref, shape, whole, c_slice in checks:
        _assert_equal(out.cpu().reshape(shape), ref, f"fp32 gemm ({name})")
        if whole is not None:
            keep = torch.ones(whole.shape[-1], dtype=torch.bool, device=whole.device)
            keep[c_slice[1]:c_slice[1] + shape[2]] = False
            assert bool((whole[:, keep] == _SENTINEL).all()), f"fp32 gemm ({name}): columns outside the output slice were written"
            assert bool((whole[-1] == _SENTINEL).all()), f"fp32 gemm ({name}): written beyond the last output row"


# ---- conv ---------------------------------------------------------------------------------------------------------------------------------
def conv_runs_on_c64_kernel(cin, cout, ksize, stride, with_res, with_sum, act_after_res):
    """the dispatch rule of csrc/conv_c64.hip (conv_c64_applicable) for tensors below 4 GB: which kernel — hence which rounding contract — a conv gets"""
    return ksize == 3 and stride == 1 and cin <= 64 and cout <= 64 and not act_after_res and not (with_sum and with_res)


def check_conv_exact(lib, dtype, n, h, w, cin, cout, ksize, stride, act=abi.ACT_NONE, with_res=False, pixel_shuffle=0, with_sum=False,
                     ldx_extra=0, seed=0, with_scale=False, scales=(0.5, 1.0, 2.0), spread=1.0, pad_mode=0, act_after_res=False, res_broadcast=False,
                     canvas=None, expect_c64=None, slope=0.125):
    """The contract of the two conv kernels (include/mtx_hip.h, mtx_conv2d_args), v = conv(x) + bias in fp32, res_scale = 0.5:
         generic kernel:   t = round_T(act(v));  y = t, or with out_scale / a residual y = round_T(out_scale * t + res_scale * res)
                           (act_after_res: t = round_T(v), y = round_T(act(t + res_scale * res)))
         64 -> 64 kernel:  y = round_T(out_scale * act(v) + res_scale * res): ONE rounding
         chan_sum on both: the sums of round_T(act(v)), exact because integer sums below 2^24 are.
    canvas = (H, W): the image is the top-left h x w of a zero canvas and the size comes from a device-side valid_hw: zeros beyond the image.
    scales: the per-channel out_scale factors are drawn from these (products with integers must stay exact: powers of two, small integers).
    spread: widens the operand range (RELU and factors below 1 both take outputs out of the range where T rounds)."""
    g = torch.Generator().manual_seed(seed)
    dev, td = _dev(lib), TD[dtype]
    what = f"conv {n}x{h}x{w} {cin}->{cout} k{ksize} s{stride}"
    c64 = conv_runs_on_c64_kernel(cin, cout, ksize, stride, with_res, with_sum, act_after_res)
    if expect_c64 is not None:
        assert c64 == expect_c64, f"{what}: the case is meant for the {'64 -> 64' if expect_c64 else 'generic'} kernel"
    kk = cin * ksize * ksize
    r, _ = operand_range(dtype, kk, with_alpha=False, spread=spread)
    H, W = canvas if canvas else (h, w)
    x = torch.zeros(n, H, W, cin, dtype=torch.float64)
    x[:, :h, :w] = _ints(g, (n, h, w, cin), r)
    wt = _ints(g, (cout, cin, ksize, ksize), r)
    b = _ints(g, (cout,), INT_CAP[dtype])
    assert kk * r * r + INT_CAP[dtype] < EXACT, f"{what}: precondition (a)"
    xi = x[:, :h, :w].permute(0, 3, 1, 2)                                         # the image alone: its own zero padding
    if pad_mode == 1:
        assert stride == 2 and ksize == 3
        v = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, b, stride=2, padding=0)
    else:
        v = F.conv2d(xi, wt, b, stride=stride, padding=ksize // 2)
    v = v.permute(0, 2, 3, 1)                                                     # [n, ho, wo, cout]
    ho, wo = v.shape[1], v.shape[2]
    osc = None
    if with_scale:
        osc = torch.tensor(scales, dtype=torch.float64)[torch.randint(0, len(scales), (n, cout), generator=g)]

    def shuffled(t_):                                                             # channel (dy * 2 + dx) * cout / 4 + c -> pixel (2 oy + dy, 2 ox + dx), channel c
        if not pixel_shuffle:
            return t_
        cps = cout // 4
        return t_.reshape(n, ho, wo, 2, 2, cps).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * ho, 2 * wo, cps)

    res = None
    if with_res:
        rs = (1 if res_broadcast else n, (2 if pixel_shuffle else 1) * (ho if not canvas else H), (2 if pixel_shuffle else 1) * (wo if not canvas else W),
              cout // 4 if pixel_shuffle else cout)
        res = _ints(g, rs, INT_CAP[dtype])
    res_img = res[:, :shuffled(v).shape[1], :shuffled(v).shape[2]] if res is not None else None
    post = with_scale or with_res
    if c64:
        pre = _act(v, act, slope)
        summed = _round(pre, td)
    else:
        pre = summed = _round(v if (act_after_res and with_res) else _act(v, act, slope), td)
    if post:
        f = pre * osc[:, None, None, :] if with_scale else pre
        f = shuffled(f)
        if with_res:
            f = f + 0.5 * res_img
            if act_after_res:
                f = _act(f, act, slope)
        assert float(f.abs().max()) * 4 < EXACT                                   # (quarter steps from res_scale and the factors included)
        ref = _round(f, td)
    else:
        ref = shuffled(summed)
    _assert_rounding_share(ref, dtype, what)
    if with_sum:
        assert not (act_after_res and with_res)
        reach = float(summed.abs().sum(dim=(1, 2)).max()) if c64 else float(summed.abs().max()) * 256        # any split of an image / one 16 x 16 tile per row
        assert reach < EXACT, f"{what}: precondition (a) — a partial channel sum may reach {reach}"
        want_sum = summed.sum(dim=(1, 2))

    pb = PlanBuilder(lib, dev, dtype)
    xb = pb.act(n, H, W, cin, ld=cin + ldx_extra)
    xb.t[..., :cin] = x.to(td)
    if ldx_extra:
        xb.t[..., cin:] = 7.0   # garbage in the unused channels must not leak
    wpk = pb.const(wt.permute(0, 2, 3, 1).reshape(cout, ksize * ksize, cin), td)
    bias = pb.const(b, torch.float32)
    rb = None
    if with_res:
        rb = pb.act(*res.shape)
        rb.t.copy_(res.to(td))
    valid = None
    if canvas:
        assert stride == 1 and not pixel_shuffle
        valid = pb.buf((2,), torch.int32)
        valid.copy_(torch.tensor([h, w], dtype=torch.int32))
    cs = None
    if with_sum:
        tiles = pb.conv_tiles(xb, ksize, stride, cout=cout, with_res=with_res, with_scale=with_scale, act=act, pixel_shuffle=pixel_shuffle)
        cs = pb.buf((n, tiles, cout), torch.float32, zero=True)
        cs.fill_(777.0)          # the conv owns every row: stale values must not survive a launch
    y = pb.conv2d(xb, wpk, bias, cout, ksize, stride, act=act, act_param=slope, res=rb, res_scale=0.5, pixel_shuffle=pixel_shuffle, chan_sum=cs,
                  out_scale=pb.const(osc, torch.float32) if with_scale else None, pad_mode=pad_mode, act_after_res=act_after_res,
                  res_broadcast=res_broadcast, valid_hw=valid)
    _run(pb)
    out = y.torch().cpu()
    oh, ow = ref.shape[1], ref.shape[2]
    _assert_equal(out[:, :oh, :ow], ref, what)
    if canvas:
        assert float(out[:, oh:].abs().max()) == 0.0 and float(out[:, :, ow:].abs().max()) == 0.0, f"{what}: nonzero output beyond the image"
    if with_sum:
        _assert_equal(cs.cpu().double().sum(dim=1), want_sum, what + " chan_sum")


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def _spacing(ref, dtype):
    """distance between neighbouring values of T at |ref| (float64 tensor)"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** MIN_EXP[dtype]))).clamp_min(MIN_EXP[dtype])
    return torch.exp2(e - MANT[dtype])


def _assert_one_rounding(got, ref, dtype, what):
    """|got - ref| <= (0.5 + 2^-10) spacings of T at |ref|: one rounding to T, plus the fp32 reciprocal and exp2 at integer arguments (each a few
    fp32 ulp, i.e. 2^-15 or less of a bf16 spacing and 2^-12 of an f16 one)"""
    ratio = (got.double() - ref).abs() / _spacing(ref, dtype)
    worst = float(ratio.max())
    assert worst <= 0.5 + 2.0 ** -10, f"{what}: off by {worst:.4f} spacings of the storage type at {int(ratio.argmax())} ({int((ratio > 0.5 + 2.0 ** -10).sum())} elements beyond the bound)"
    return worst


ATTN_LAYOUTS = ("dense", "fused_qkv", "windows", "fused_kv", "fused_qk_sep_v", "o_slice", "head_major", "narrow_o_ss", "narrow_o_off")
ATTN_TAIL_ROWS = 64                     # poisoned / sentinel rows behind every buffer: one key tile, so a load that lost its guard meets NaN inside the allocation
UNIT_SCALE = 0.6931471824645996         # the fp32 value whose fp32 product with the launcher's log2(e) constant is exactly 1: integer logits stay integers without MTX_ATTN_Q_PRESCALED
assert float(torch.tensor(UNIT_SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)) == 1.0


def attention_layout(layout, batch, heads, sq, sk, d):
    """Where the four operands of a call live (C = heads * d, ld = row stride in elements):
         fused_qkv       q | k | v in the rows of one [batch * max(sq, sk), 3C + 8] buffer, o in [rows, C]     (SAM 3, FLUX, the manga-ocr encoder)
         windows         fused_qkv with sq == sk == the window's tokens: window b + 1 starts right behind window b  (SAM 2.1, YOLO11 area attention)
         fused_kv        q apart, k | v in [sk, 2C]                                                               (manga-ocr cross attention)
         fused_qk_sep_v  q | k in [rows, 2C], v in [rows, C + 8]: k_ss != v_ss                                    (RT-DETR, the SAM decoder)
         o_slice         fused_qkv, o at column 2C of a [rows, 5C] buffer                                         (the FLUX single block)
         head_major      [batch, heads, s, d], every operand with its own row, sequence and batch padding: twelve different strides
         narrow_o_ss     fused_qkv with o_ss = C + 4; narrow_o_off: o four elements into rows of C + 8: 8-byte stores only
    -> {operand: (buffer, offset, (bs, ss, hs))} in elements"""
    C, smax = heads * d, max(sq, sk)
    if layout == "dense":
        return {"q": ("q", 0, (sq * C, C, d)), "k": ("k", 0, (sk * C, C, d)), "v": ("v", 0, (sk * C, C, d)), "o": ("o", 0, (sq * C, C, d))}
    if layout == "head_major":
        spec = {}
        for i, (x, s) in enumerate((("q", sq), ("k", sk), ("v", sk), ("o", sq))):
            ss = d + 8 * i
            hs = (s + 1 + i) * ss
            spec[x] = (x, 0, (heads * hs + 8 * (i + 1), ss, hs))
        strides = [st for _, _, three in spec.values() for st in three]
        assert len(set(strides)) == 12, f"head_major: two of the twelve strides are equal: {strides}"
        return spec
    if layout == "fused_kv":
        return {"q": ("q", 0, (sq * C, C, d)), "k": ("kv", 0, (sk * 2 * C, 2 * C, d)), "v": ("kv", C, (sk * 2 * C, 2 * C, d)), "o": ("o", 0, (sq * C, C, d))}
    if layout == "fused_qk_sep_v":
        return {"q": ("qk", 0, (smax * 2 * C, 2 * C, d)), "k": ("qk", C, (smax * 2 * C, 2 * C, d)), "v": ("v", 0, (sk * (C + 8), C + 8, d)),
                "o": ("o", 0, (sq * C, C, d))}
    if layout == "windows":
        assert sq == sk and sq % 64, "windows: one window of tokens on both sides, not a multiple of the key tile"
    ld = 3 * C + 8
    spec = {"q": ("qkv", 0, (smax * ld, ld, d)), "k": ("qkv", C, (smax * ld, ld, d)), "v": ("qkv", 2 * C, (smax * ld, ld, d)), "o": ("o", 0, (sq * C, C, d))}
    if layout == "o_slice":
        spec["o"] = ("o", 2 * C, (sq * 5 * C, 5 * C, d))
    elif layout == "narrow_o_ss":
        spec["o"] = ("o", 0, (sq * (C + 4), C + 4, d))
    elif layout == "narrow_o_off":
        spec["o"] = ("o", 4, (sq * (C + 8), C + 8, d))
    else:
        assert layout in ("fused_qkv", "windows"), layout
    return spec


def attention_route(cus, batch, heads, sq, sk, d, layout="dense", prescaled=False):
    """launch_attn_t (csrc/attention.hip) restated: what mtx_attention_last_route must report for a 16-bit call without fp8 operands on `cus` compute
    units, from buffers that start on a 16-byte boundary -> (kernel, flags, n_full, split)"""
    pre = abi.ATTN_ROUTE_PRESCALED if prescaled else 0
    if not (d == 128 and sq >= 1024 and sk >= 256):
        grid = batch * heads * ((sq + 127) // 128)
        return (32 if d <= 32 else 64 if d <= 64 else 96 if d <= 96 else 128), pre, grid, 1
    _, off, (bs, ss, hs) = attention_layout(layout, batch, heads, sq, sk, d)["o"]
    wide = prescaled and ss % 8 == 0 and hs % 8 == 0 and bs % 8 == 0 and off % 8 == 0
    total, ntiles = batch * heads * ((sq + 255) // 256), (sk + 63) // 64
    rem = total % cus
    split = min(cus // rem if rem > 0 and total > cus else 1, 8, ntiles // 2)
    n_full, split = (total, 1) if split < 2 else (total - rem, split)
    return abi.ATTN_ROUTE_LONG, pre | (abi.ATTN_ROUTE_WIDE_STORE if wide else 0), n_full, split


def compute_units(lib):
    """the CU count the launchers see: mtx_device_info's, or the simulator's 3 (csrc/mtx_device.h)"""
    if lib.is_simulator:
        return 3
    import ctypes as C
    cus = C.c_int(0)
    lib.check(lib.mtx_device_info(C.byref(cus), None, None, 0), "mtx_device_info")
    return cus.value


def _assert_route(lib, route, what):
    """route: None, or (kernel, flags, n_full, split) where None = any value and a split of ">=2" = any key split"""
    if route is None:
        return
    got = lib.attention_last_route()
    ok = all(e is None or (e == ">=2" and g >= 2) or e == g for e, g in zip(route, got))
    assert ok, f"{what}: the launch took (kernel, flags, n_full, split) = {got}, the case is written for {tuple(route)}"


def _launch_attention_layout(lib, dtype, q, k, v, prescaled, layout, route, scale):
    """the operands placed as attention_layout says, every element around them NaN (inputs) or _SENTINEL (output), ATTN_TAIL_ROWS such rows behind each buffer"""
    dev, td = _dev(lib), TD[dtype]
    batch, sq, heads, d = q.shape
    sk = k.shape[1]
    what = f"attention {layout} {batch}x{heads}x{sq}x{sk} d{d}"
    spec = attention_layout(layout, batch, heads, sq, sk, d)
    shape = {"q": (batch, sq, heads, d), "k": (batch, sk, heads, d), "v": (batch, sk, heads, d), "o": (batch, sq, heads, d)}
    size = {}
    for x, (name, off, (bs, ss, hs)) in spec.items():
        b_, s_, h_, _ = shape[x]
        assert off + d <= ss and min(bs, ss, hs) >= d, f"{what}: operand {x} overlaps itself"
        extent = off + (b_ - 1) * bs + (s_ - 1) * ss + (h_ - 1) * hs + d
        size[name] = max(size.get(name, 0), extent + ATTN_TAIL_ROWS * ss + 8)
    pb = PlanBuilder(lib, dev, dtype)
    bufs = {name: pb.buf((n,), td) for name, n in size.items()}
    view = lambda t, x: t.as_strided(shape[x], spec[x][2] + (1,), spec[x][1])
    for name, t in bufs.items():
        t.fill_(_SENTINEL if name == "o" else float("nan"))
    for x, val in (("q", q), ("k", k), ("v", v)):
        view(bufs[spec[x][0]], x).copy_(val.to(td))
    for name, t in bufs.items():                                 # what the call must not read is NaN, all of it: the operands do not overlap
        if name != "o":
            inside = sum(math.prod(shape[x]) for x in "qkv" if spec[x][0] == name)
            assert int(t.isnan().sum()) == t.numel() - inside, f"{what}: operands overlap in buffer {name}"
    ptr_off = {x: spec[x][1] for x in spec}
    assert all(t.data_ptr() % 16 == 0 for t in bufs.values())
    pb.attention(bufs[spec["q"][0]], bufs[spec["k"][0]], bufs[spec["v"][0]], bufs["o"], batch, heads, sq, sk, d,
                 spec["q"][2], spec["k"][2], spec["v"][2], spec["o"][2], scale, q_off=ptr_off["q"], k_off=ptr_off["k"], v_off=ptr_off["v"],
                 o_off=ptr_off["o"], q_prescaled=prescaled)
    _run(pb)
    _assert_route(lib, route, what)
    written = torch.zeros(bufs["o"].numel(), dtype=torch.bool, device=dev)
    view(written, "o").fill_(True)
    assert int(written.sum()) == math.prod(shape["o"])
    assert bool((bufs["o"][~written] == _SENTINEL).all()), f"{what}: written outside the output ({int((bufs['o'][~written] != _SENTINEL).sum())} elements)"
    return view(bufs["o"], "o")


def _launch_attention(lib, dtype, q, k, v, f8_scores, prescaled, layout="dense", route=None, scale=None):
    """q [b, sq, heads, d], k / v [b, sk, heads, d] (float64 on the device, values exact in T and, with f8_scores, in e4m3) -> the kernel's output.
    layout: where the operands live (attention_layout); "dense" = four private buffers, as the cases of the first round of exact tests had them"""
    dev, td = _dev(lib), TD[dtype]
    batch, sq, heads, d = q.shape
    sk = k.shape[1]
    D = heads * d
    if layout != "dense":
        assert not f8_scores
        return _launch_attention_layout(lib, dtype, q, k, v, prescaled, layout, route, 1.0 / math.sqrt(d) if scale is None else scale)
    pb = PlanBuilder(lib, dev, dtype)
    o = pb.buf((batch, sq, heads, d), td, zero=True)
    if f8_scores:
        assert batch == 1 and d == 128 and prescaled
        rows = max(sq, sk)
        packed = torch.zeros(rows, 2 * D, dtype=torch.uint8)                              # [row][q bytes | k bytes]: the layout the rotary kernel leaves
        packed[:sq, :D] = q[0].cpu().float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(sq, D)
        packed[:sk, D:] = k[0].cpu().float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(sk, D)
        unused = pb.buf((1, rows, heads, d), td, zero=True)                              # q / k are not read in this form
        pb.attention(unused, unused, pb.const(v.to(td)), o, 1, heads, sq, sk, d, (rows * D, D, d), (rows * D, D, d), (sk * D, D, d), (sq * D, D, d),
                     1.0, q_prescaled=True, qk_f8=(pb.const(packed), 0, D, 2 * D, 0))
    else:
        pb.attention(pb.const(q.to(td)), pb.const(k.to(td)), pb.const(v.to(td)), o, batch, heads, sq, sk, d,
                     (sq * D, D, d), (sk * D, D, d), (sk * D, D, d), (sq * D, D, d), 1.0 / math.sqrt(d) if scale is None else scale, q_prescaled=prescaled)
    _run(pb)
    _assert_route(lib, route, f"attention {batch}x{heads}x{sq}x{sk} d{d}")
    return o


def check_attention_census(lib, dtype, batch, heads, sq, sk, d, prescaled=False, f8_scores=False, seed=0, layout="dense", route=None):
    """Key census: q = 0, so every score is 0 and every probability 1; v[j, :, c] = 64 where c = hash(j) and 0 elsewhere.  Every output row is
    then 64 * count_c / sk: a key dropped or counted twice moves one channel by 64 / sk — about 128 / sk of its value, far above the rounding.
    Two hashes, j % d and (j // d) % d, so that every key is told apart from its neighbours and from the keys d away.
    layout: where the operands live (attention_layout); route: what mtx_attention_last_route must report (_assert_route)."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev(lib)
    worst = 0.0
    for hashed in (lambda j: j % d, lambda j: (j // d) % d):
        q = torch.zeros(batch, sq, heads, d, dtype=torch.float64, device=dev)
        k = _ints(g, (batch, sk, heads, d), 3).to(dev)
        j = torch.arange(sk)
        v = torch.zeros(batch, sk, heads, d, dtype=torch.float64)
        v[:, j, :, hashed(j)] = 64.0
        count = torch.bincount(hashed(j), minlength=d).double()
        ref = (64.0 * count / sk).to(dev).expand(batch, sq, heads, d)
        o = _launch_attention(lib, dtype, q, k, v.to(dev), f8_scores, prescaled, layout, route)
        worst = max(worst, _assert_one_rounding(o, ref, dtype, f"attention census {layout} {batch}x{heads}x{sq}x{sk} d{d}"))
    return worst


def check_attention_dyadic(lib, dtype, batch, heads, sq, sk, d, f8_scores=False, late_max=False, seed=0, layout="dense", route=None, prescaled=True):
    """Dyadic softmax (MTX_ATTN_Q_PRESCALED; with f8_scores the e4m3 score path at qk_f8_exp = 0): q rows are +-one-hot, k holds integers in
    [-3, 3], v integers in [-4, 4].  The base-2 logits are then integers, every probability is a power of two whatever maximum the kernel
    subtracts, and numerator and denominator are exact in fp32 (sk * 4 * 2^6 < 2^24).  late_max: the first three quarters of the keys are clamped
    to [-1, 1], so the running maximum has to move late.  prescaled = False: the same logits through the scaling kernels, at UNIT_SCALE.
    layout, route: as in check_attention_census."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev(lib)
    assert sk * 4 * 64 < EXACT
    hot = torch.randint(0, d, (batch, sq, heads), generator=g)
    sign = torch.randint(0, 2, (batch, sq, heads), generator=g).double() * 2 - 1
    q = torch.zeros(batch, sq, heads, d, dtype=torch.float64)
    q.scatter_(3, hot[..., None], sign[..., None])
    k = _ints(g, (batch, sk, heads, d), 3)
    if late_max:
        k[:, :sk * 3 // 4].clamp_(-1, 1)
    v = _ints(g, (batch, sk, heads, d), 4)
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    o = _launch_attention(lib, dtype, q, k, v, f8_scores, prescaled, layout, route, scale=1.0 if prescaled else UNIT_SCALE)
    worst = 0.0
    for bi in range(batch):
        for hd in range(heads):                                                          # head by head: the float64 score matrix of 24 heads would not fit
            logits = q[bi, :, hd] @ k[bi, :, hd].t()
            p = torch.exp2(logits - logits.amax(dim=1, keepdim=True))
            ref = (p @ v[bi, :, hd]) / p.sum(dim=1, keepdim=True)
            worst = max(worst, _assert_one_rounding(o[bi, :, hd], ref, dtype, f"dyadic attention {sq}x{sk} d{d}, batch {bi} head {hd}"))
    return worst


# ---- attention through the layouts the model graphs use (attention_layout), every case with the route it is written for -------------------
# kernel: the short kernel's padded head width, or "long"; wide: the long-sequence kernel's 16-byte row stores (pre-scaled q and an aligned output only).
# at_256 = (n_full, split) on 256 compute units: the key-split tail and attn_merge_kernel; at_3 the same on the simulator's three.  gpu_only: left out of
# the simulator tier — the 43 to 84 heads that fill 256 compute units cost it many times what its other long-sequence cases do, and on 3 compute units
# they would be cut differently anyway (there every long-sequence case with total % 3 == 1 goes through split 3 and the merge).
_L = abi.ATTN_ROUTE_LONG
ATTN_LAYOUT_CASES = [
    # the short kernel, its four widths through fused_qkv and one more layout each
    dict(layout="fused_qkv", batch=1, heads=3, sq=70, sk=150, d=8, kernel=32),
    dict(layout="fused_kv", batch=2, heads=3, sq=5, sk=100, d=8, kernel=32, prescaled=True),
    dict(layout="fused_qkv", batch=1, heads=2, sq=9, sk=100, d=40, kernel=64, prescaled=True),
    dict(layout="windows", batch=3, heads=2, sq=196, sk=196, d=40, kernel=64),
    dict(layout="head_major", batch=2, heads=2, sq=70, sk=150, d=40, kernel=64),
    dict(layout="fused_qkv", batch=1, heads=2, sq=70, sk=150, d=88, kernel=96),
    dict(layout="fused_qk_sep_v", batch=2, heads=2, sq=70, sk=150, d=88, kernel=96, prescaled=True),
    dict(layout="fused_qkv", batch=1, heads=2, sq=70, sk=150, d=104, kernel=128),
    dict(layout="fused_qkv", batch=2, heads=2, sq=130, sk=100, d=128, kernel=128, prescaled=True),
    dict(layout="head_major", batch=1, heads=3, sq=9, sk=100, d=104, kernel=128),
    dict(layout="o_slice", batch=2, heads=2, sq=70, sk=150, d=128, kernel=128),
    dict(layout="fused_kv", batch=1, heads=2, sq=1, sk=70, d=128, kernel=128),
    dict(layout="narrow_o_ss", batch=2, heads=2, sq=70, sk=150, d=104, kernel=128),
    dict(layout="narrow_o_off", batch=1, heads=2, sq=9, sk=100, d=16, kernel=32),
    dict(layout="fused_qkv", batch=1, heads=1, sq=1030, sk=200, d=128, kernel=128),                    # long queries, short keys: still the short kernel
    # the long-sequence kernel (d = 128, sq >= 1024, sk >= 256)
    dict(layout="fused_qkv", batch=1, heads=2, sq=1030, sk=330, d=128, kernel=_L, prescaled=True, wide=True, at_3=(9, 3)),      # on the simulator's 3 compute units: n_full 9, split 3, the merge
    dict(layout="fused_qk_sep_v", batch=1, heads=1, sq=1100, sk=449, d=128, kernel=_L, wide=False),
    dict(layout="narrow_o_ss", batch=1, heads=1, sq=1030, sk=330, d=128, kernel=_L, prescaled=True, wide=False),
    dict(layout="fused_qkv", batch=1, heads=2, sq=1030, sk=330, d=128, kernel=_L, wide=False),
    dict(layout="fused_qk_sep_v", batch=1, heads=2, sq=1100, sk=449, d=128, kernel=_L, prescaled=True, wide=True),
    dict(layout="head_major", batch=1, heads=2, sq=1100, sk=449, d=128, kernel=_L, prescaled=True, wide=True),
    dict(layout="head_major", batch=2, heads=2, sq=1100, sk=449, d=128, kernel=_L, wide=False),
    dict(layout="fused_qkv", batch=2, heads=2, sq=1030, sk=330, d=128, kernel=_L, prescaled=True, wide=True),
    dict(layout="o_slice", batch=2, heads=2, sq=1030, sk=330, d=128, kernel=_L, prescaled=True, wide=True),
    dict(layout="narrow_o_off", batch=1, heads=2, sq=1030, sk=330, d=128, kernel=_L, prescaled=True, wide=False, at_3=(9, 3)),     # the merge writes 8-byte aligned rows
    dict(layout="narrow_o_ss", batch=2, heads=2, sq=1030, sk=330, d=128, kernel=_L, wide=False),
    # the key-split tail
    dict(layout="fused_qkv", batch=1, heads=65, sq=1024, sk=256, d=128, kernel=_L, prescaled=True, wide=True, at_256=(256, 2), gpu_only=True),      # total 260, rem 4: 64 clamped by ntiles / 2
    dict(layout="fused_qkv", batch=1, heads=65, sq=1024, sk=1000, d=128, kernel=_L, prescaled=True, wide=True, at_256=(256, 8), gpu_only=True),     # ... clamped by 8; ragged last key tile
    dict(layout="fused_qkv", batch=1, heads=84, sq=1024, sk=640, d=128, kernel=_L, prescaled=True, wide=True, at_256=(256, 3), gpu_only=True),      # total 336, rem 80
    dict(layout="fused_qkv", batch=1, heads=43, sq=1300, sk=1000, d=128, kernel=_L, prescaled=True, wide=True, at_256=(256, 8), gpu_only=True),     # 6 query blocks, the last one partial; rem 2
    dict(layout="narrow_o_off", batch=1, heads=65, sq=1024, sk=256, d=128, kernel=_L, prescaled=True, wide=False, at_256=(256, 2), gpu_only=True),  # the merge writes 8-byte aligned rows
    dict(layout="fused_qkv", batch=1, heads=65, sq=1024, sk=320, d=128, kernel=_L, wide=False, at_256=(256, 2), gpu_only=True),                      # the scaling kernel's partials
]


def attention_case_id(case):
    return f"{case['layout']}-{case['batch']}x{case['heads']}x{case['sq']}x{case['sk']}-d{case['d']}{'-prescaled' if case.get('prescaled') else ''}"


def check_attention_layout_case(lib, dtype, kind, case, seed=0):
    """one row of ATTN_LAYOUT_CASES as a key census (kind "census") or a dyadic softmax ("dyadic"); the route comes from launch_attn_t's rule at the
    device's CU count, must be the one the row is written for, and the launch must report it"""
    import pytest
    shape = {key: case[key] for key in ("batch", "heads", "sq", "sk", "d")}
    prescaled = case.get("prescaled", False)
    route = attention_route(compute_units(lib), layout=case["layout"], prescaled=prescaled, **shape)
    assert route[0] == case["kernel"], f"{attention_case_id(case)}: written for kernel {case['kernel']}, the launch rule gives {route[0]}"
    if case["kernel"] == _L:
        assert bool(route[1] & abi.ATTN_ROUTE_WIDE_STORE) == case["wide"], f"{attention_case_id(case)}: written for {'16' if case['wide'] else '8'}-byte stores"
    if "at_3" in case:
        assert attention_route(3, layout=case["layout"], prescaled=prescaled, **shape)[2:] == case["at_3"]
    if "at_256" in case:
        assert attention_route(256, layout=case["layout"], prescaled=prescaled, **shape)[2:] == case["at_256"]
        if route[3] < 2:
            pytest.skip(f"{attention_case_id(case)} reaches the key split on 256 compute units as (n_full, split) = {case['at_256']}; "
                        f"on the {compute_units(lib)} of this device the launch rule gives split {route[3]}: no partials, no merge")
    if kind == "census":
        return check_attention_census(lib, dtype, prescaled=prescaled, seed=seed, layout=case["layout"], route=route, **shape)
    assert kind == "dyadic"
    return check_attention_dyadic(lib, dtype, prescaled=prescaled, seed=seed, layout=case["layout"], route=route, **shape)


# ---- the conv cases of both tiers (the GPU tier adds the page-scale shapes) -------------------------------------------------------------
CONV_CASES = [
    # the configurations of test_conv (SiLU has no exact form: LEAKY with a power-of-two slope or RELU in its place)
    dict(n=1, h=20, w=19, cin=64, cout=64, ksize=3, stride=1, act=abi.ACT_RELU),
    dict(n=2, h=9, w=33, cin=16, cout=24, ksize=3, stride=1, with_res=True),
    dict(n=1, h=17, w=18, cin=72, cout=136, ksize=3, stride=1, act=abi.ACT_LEAKY, ldx_extra=8),
    dict(n=1, h=21, w=35, cin=48, cout=96, ksize=3, stride=2, act=abi.ACT_LEAKY),
    dict(n=1, h=16, w=16, cin=128, cout=64, ksize=1, stride=1, act=abi.ACT_LEAKY),
    dict(n=1, h=10, w=18, cin=32, cout=128, ksize=3, stride=1, pixel_shuffle=2, with_res=True),
    dict(n=2, h=18, w=20, cin=64, cout=64, ksize=3, stride=1, with_sum=True, act=abi.ACT_RELU),
    dict(n=2, h=52, w=50, cin=64, cout=64, ksize=3, stride=1, with_sum=True, act=abi.ACT_RELU),
    dict(n=1, h=50, w=67, cin=40, cout=64, ksize=3, stride=1, ldx_extra=8),
    dict(n=1, h=40, w=24, cin=64, cout=64, ksize=3, stride=1, with_res=True, with_sum=True),
    # the 64 -> 64 persistent kernel (ONE rounding), border tiles only and with interior tiles
    dict(n=2, h=21, w=19, cin=64, cout=64, ksize=3, stride=1, with_res=True, expect_c64=True),
    dict(n=1, h=52, w=50, cin=64, cout=64, ksize=3, stride=1, with_res=True, act=abi.ACT_RELU, expect_c64=True),
    dict(n=2, h=21, w=19, cin=64, cout=64, ksize=3, stride=1, act=abi.ACT_RELU, with_sum=True, with_scale=True, spread=1.5, expect_c64=True),
    dict(n=2, h=52, w=50, cin=64, cout=64, ksize=3, stride=1, with_res=True, with_scale=True, expect_c64=True),
    dict(n=2, h=52, w=50, cin=64, cout=64, ksize=3, stride=1, with_sum=True, with_scale=True, scales=(0.5, 1.0, 3.0), expect_c64=True),   # 3 v != 3 round(v): one rounding on interior AND border tiles
    dict(n=3, h=20, w=36, cin=64, cout=64, ksize=3, stride=1, with_res=True, res_broadcast=True, expect_c64=True),
    dict(n=1, h=21, w=40, cin=64, cout=64, ksize=3, stride=1, with_res=True, with_scale=True, canvas=(64, 64), expect_c64=True),
    dict(n=1, h=20, w=34, cin=64, cout=64, ksize=3, stride=1, pixel_shuffle=2, with_res=True, expect_c64=True),
    dict(n=1, h=20, w=34, cin=32, cout=64, ksize=3, stride=1, ldx_extra=8, act=abi.ACT_LEAKY, expect_c64=True),
    # the generic kernel (rounds act(..) first)
    dict(n=2, h=21, w=19, cin=64, cout=64, ksize=3, stride=1, act=abi.ACT_RELU, with_sum=True, with_scale=True, with_res=True, spread=1.5, expect_c64=False),
    dict(n=1, h=17, w=23, cin=32, cout=72, ksize=3, stride=1, act=abi.ACT_LEAKY, with_sum=True, with_scale=True, scales=(0.5, 1.0, 3.0), expect_c64=False),
    dict(n=2, h=21, w=35, cin=48, cout=96, ksize=3, stride=2, pad_mode=1, expect_c64=False),
    dict(n=1, h=20, w=36, cin=32, cout=72, ksize=3, stride=2, pad_mode=1, act=abi.ACT_RELU, with_res=True, expect_c64=False),
    dict(n=2, h=19, w=22, cin=64, cout=64, ksize=3, stride=1, act=abi.ACT_RELU, with_res=True, act_after_res=True, expect_c64=False),
    dict(n=1, h=16, w=24, cin=96, cout=32, ksize=1, stride=1, act=abi.ACT_LEAKY, with_res=True, act_after_res=True, expect_c64=False),
    dict(n=3, h=18, w=20, cin=24, cout=72, ksize=3, stride=1, with_res=True, res_broadcast=True, expect_c64=False),
    dict(n=2, h=10, w=18, cin=32, cout=128, ksize=3, stride=1, pixel_shuffle=2, with_res=True, res_broadcast=True, expect_c64=False),
    dict(n=2, h=21, w=40, cin=32, cout=48, ksize=3, stride=1, act=abi.ACT_RELU, with_sum=True, with_res=True, canvas=(48, 64), expect_c64=False),
    dict(n=1, h=13, w=30, cin=128, cout=64, ksize=1, stride=1, with_sum=True, canvas=(32, 32), expect_c64=False),
]

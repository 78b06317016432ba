"""Exact-input checks of the kernels between a page and the three detectors — deform_attn_kernel and box_refine_kernel (csrc/detr.hip),
yolo_decode_kernel, mask_count_kernel / mask_pick_kernel, resize_thresh_kernel, img_kernel and the letterbox branch of preproc_kernel
(csrc/elementwise.hip) — against float64 references written from the contracts in include/mtx_hip.h.

All of them are index arithmetic plus a few fp32 operations, and each feeds a discrete decision (a box for NMS, a 0/1 mask, a mask index, a
sampling point), so the inputs are chosen to make the expected output EXACT wherever that is possible and the assertion is zero differing
elements; where it is not, the bound is derived below from documented instruction accuracy, never from what a kernel returned.  The fp32
facts used: IEEE add / multiply / fused multiply-add round once (relative 2^-24 = u); division and 1 / x are allowed 1 ulp (2 u); expf and
logf 1 ulp; __expf(x) is the hardware exp2 (1 ulp) of the fp32 product x * log2(e), whose two roundings (the constant and the product) move
the argument by at most 2 u |x| log2(e), i.e. the exponential by the relative amount 2 u |x|; a compiler may fuse a multiply into an add.

Every case asserts its preconditions FROM THE REFERENCE ALONE before it looks at the kernel.  Every output lies inside a sentinel-filled
buffer (padding columns where a leading dimension allows them and one spare row / image behind it) that must come back untouched, and the
unused columns of the inputs hold garbage (stream_checks.SENTINEL, GARBAGE).

1. Deformable attention (mtx_detr kind 0).
   out[r, h] = sum_p softmax(aw[r, h])[p] * bilinear(value_level(p)[h], ref.xy + off[p] * ref.wh * offset_scale / points), pixel coordinate
   loc * size - 0.5 (grid_sample, align_corners = False), taps outside a map contribute zero.
   Geometry: level sizes are powers of two, points = 4 and offset_scale = 0.5 (the factor is 1/8), ref w / h in {1/8, 1/4}, cx / cy multiples
   of 1/64, offsets integers: every location is a multiple of 1/64, so is every pixel coordinate and every bilinear weight, a product of two
   weights is a multiple of 2^-12, and all fp32 steps of the contract are exact.  Value maps hold integers up to 100; with the point weights
   w in {1} (ONE-HOT: one logit 0, the others -200, whose exponential is 0 in fp32), {1 / LP} (UNIFORM, LP a power of two) every term is a
   multiple of q = 2^-12 / LP and the case asserts sum |terms| / q < 2^24: the sum is exact in any order, the output is the float64 sample
   rounded once to T, zero differing elements.
   GENERAL (LP = 12, logits multiples of 1/16 in [-8, 8], so that aw - max is exact): with M the largest tap magnitude,
     e_p = __expf(aw_p - max): relative 2 u * 16 + 2 u = 2^-19 + 2^-23 (|argument| <= 16);   den: (LP - 1) additions of positive terms, u each;
     1 / den: 2 u;  e_p / den: u;  so a weight carries 2 (2^-19 + 2^-23) + (LP + 2) u;  times the two (exact) bilinear weights: 2 u;  each of the
     4 LP taps one product (u) and one addition (u of a partial sum that is at most M, since the weights sum to 1):
     |fp32 result - reference| <= E = M (2^-18 + 2^-22 + (5 LP + 4) u).
   The kernel rounds that result to T.  If it stays in the reference's binade the total is 0.5 spacing_T(ref) + E; if E carries it over a
   power of two, that power is itself a value of T, so the rounding moves it by at most E again.  Bound: 0.5 spacing_T(ref) + 2 E.

2. Box refinement (kinds 1, 2).  ref_out = sigmoid(x), x = delta + log(x1 / x2) with v = clamp(ref, 0, 1), x1 = max(v, 1e-5), x2 = max(1 - v, 1e-5)
   (kind 2: x is given).  x = 0 gives 1 / (1 + 1) = 0.5, x = 200 gives 1 / (1 + 0) = 1, x = -200 gives 1 / inf = 0, all exactly.
   Otherwise: 1 - v rounds once (u), the quotient 2 u, so the argument of the logarithm is 3 u off and the logarithm 3 u absolutely, plus its
   own ulp, at most 2^-20 since |log| < 16; the sum with delta rounds once: dx = 3 u + 2^-20 + u |x|.  e = expf(-x) is 2 u off relatively.
   s = 1 / (1 + e) moves by s (1 - s) for a unit change of x or a unit relative change of e, and 1 + e and the division round the result
   itself (3 u):   |ref_out - sigmoid(x)| <= s (1 - s) (dx + 2 u) + 3 u s.   (kind 2: dx = 0.)   The T copy is within half a spacing of T
   of the fp32 value the kernel wrote.

3. YOLO head decode.  box = (x + 0.5 -+ d) * stride with d = sum_k k softmax(bins)[k]; scores = sigmoid; mask coefficients copied.
   ONE-HOT bins (0 and -200): e in {1, 0}, d = k exactly; EQUAL bins with reg_max = 16: 16 ones, d = 120 / 16 = 7.5; strides are powers of two:
   the box is exact.  GENERAL bins (multiples of 1/16 in T, multiples of 2^-12 in fp32: bin - max is exact): e_k 2 u, e_k * k u, reg_max - 1
   additions of positive terms in either sum, the quotient 2 u:  d is (2 + 1 + R - 1) u + (2 + R - 1) u + 2 u = (2 R + 5) u off relatively
   (R = reg_max), d <= R - 1, and (x + 0.5 -+ d) rounds once:  |box - ref| <= stride ((R - 1) (2 R + 5) u + u |ref / stride|).
   Scores (|x| <= 16): e = __expf(-x) is 2^-19 + 2^-23 off relatively, as in 1:  |score - s| <= s (1 - s) (2^-19 + 2^-23) + 3 u s.

4. Mask selection.  counts = (|logit0 > +delta|, |logit0 > -delta|), strict; sel = 0 if au == 0 or float32(ai) / float32(au) >= thresh, else
   1 + argmax(iou[1:4]) with the first maximum winning.  Integers: everything is exact.

5. Resize + threshold.  Source index max(0, (dst + 0.5) * scale - 0.5), scale = source / destination size, bilinear, mask = value > thresh.
   EXACT family: integer sources, dyadic scales: every interpolated value is exact, ties with thresh included (they give 0).
   GENERAL family: the kernel's index is off by at most df = u * 16 (scale, relative u, times an index below 16) + 2^-21 (the product) + 2^-21
   (the subtraction; a fused multiply-add only drops one of these) = 2^-19; the fractional part is then exact and 1 - fraction rounds by at
   most 2^-25.  The interpolant is continuous and piecewise linear with slope at most G (the largest difference of neighbouring source
   pixels) along either axis, and its seven fp32 operations round by u V each (V the largest source magnitude):
     |kernel value - reference| <= D = 2 G (2^-19 + 2^-25) + 7 u V.   Pixels within D of thresh are left out, at most 1 % of them.

6. Page boundary conversions.  HWC_U8_TO_NHWC: float32(b) / 255 is ONE fp32 division, then * mul + add, one rounding to T.  For (1, 0) nothing
   rounds; for (2, -1) the product by two is exact, so the fused and the two-step form round the same real number once (asserted).
   NHWC_TO_HWC_U8: trunc(clamp(v * mul + add, 0, 1) * 255) with the product in fp32, over every finite T value in [-0.5, 1.5].  (1, 0) is the
   identity; for (0.5, 0.5) the product by the power of two 0.5 is exact (also for T's subnormals, which are fp32 normals), so v / 2 + 0.5 is
   one rounding of the same real number fused or not: the numpy fp32 expression below is what any compilation computes.
   valid_hw: a destination pixel whose first source pixel (y * u, x * u) lies beyond the valid size is zero in all c_pad channels; one that
   straddles the edge (odd valid size, u = 2) is converted whole, as the super-resolution call site relies on (it pads the source).

7. Letterbox.  Bilinear resize (same index as 5) of the uint8 levels, rounded half to even, placed on a canvas of 114, BGR -> RGB, / 255.
   EXACT family: dyadic ratios, all weights dyadic, the value exact, many of them k + 0.5.  The kernel multiplies by float32(1 / 255) where the
   reference divides; the case asserts that both give the same T for all 256 levels.
   GENERAL family: as in 5 with indices below 128: df = u * 128 + 2^-18 + 2^-18 = 2^-16;  D = (Gy + Gx) (2^-16 + 2^-25) + 7 u * 255.  Pixels
   within D of a half-integer are left out, at most 1 %.

Same layout as exact_checks.py, stream_checks.py and operand_checks.py: written once, run on the simulator and on the product library."""
import numpy as np
import torch
import torch.nn.functional as F

import parity_log
from exact_checks import EXACT, _assert_equal, _round, _spacing
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder
from op_checks import TD, _dev, _run, _sync
from stream_checks import GARBAGE, SENTINEL

U = 2.0 ** -24
NAME = {abi.BF16: "bf16", abi.F16: "f16", abi.F32: "f32"}
BYTE_SENTINEL = 0xA5
_FIGURES = {}


def _note(name, **figures):
    """the largest figures of the session under one parity_log name"""
    f = _FIGURES.setdefault(name, {})
    for k, v in figures.items():
        f[k] = max(f.get(k, 0.0), float(v))
    parity_log.record(name, **{k: float(f"{v:.4g}") for k, v in f.items()})


def _exact_in(v, td):
    return bool((v.to(td).double() == v).all())


def _guarded(pb, rows, ld, dt, fill=SENTINEL):
    """[rows + 1, ld] filled with the sentinel: the output occupies [:rows, :cols]"""
    t = pb.buf((rows + 1, ld), dt)
    t.fill_(fill)
    return t


def _assert_guard(t, rows, cols, what, fill=SENTINEL):
    assert bool((t[rows:] == fill).all()), f"{what}: the spare row behind the output was written"
    assert bool((t[:rows, cols:] == fill).all()), f"{what}: the padding columns of the output were written"


def _assert_bytes(got, ref, what):
    got, ref = got.cpu(), ref.cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ; first at {i}: got {int(got[i])}, want {int(ref[i])}")


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements beyond the derived bound; first at {i}: got {float(got[i])}, "
                             f"want {float(ref[i])} +- {float(bound[i]):.3g}")
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


# ---- 1. deformable attention --------------------------------------------------------------------------------------------------------------
POINTS, OFFSET_SCALE, VALUE_CAP = 4, 0.5, 100


def _deform_ref(values, off, w, ref, shapes):
    """values[l]: [H_l * W_l, heads, d]; off: [R, heads, L, P, 2]; w: [R, heads, L, P] point weights; ref: [R, 4] -> (out, sum |terms|) [R, heads, d]
    and the pixel coordinates (px, py) [R, heads, L, P].  float64 throughout, straight from the contract."""
    rows, heads, _, pts, _ = off.shape
    d = values[0].shape[-1]
    out = torch.zeros(rows, heads, d, dtype=torch.float64, device=off.device)
    mass = torch.zeros_like(out)
    hh = torch.arange(heads, device=off.device)[None, :, None]
    pxs, pys = [], []
    for l, (H, W) in enumerate(shapes):
        lx = ref[:, 0, None, None] + off[:, :, l, :, 0] * ref[:, 2, None, None] * (OFFSET_SCALE / pts)
        ly = ref[:, 1, None, None] + off[:, :, l, :, 1] * ref[:, 3, None, None] * (OFFSET_SCALE / pts)
        px, py = lx * W - 0.5, ly * H - 0.5
        x0, y0 = torch.floor(px), torch.floor(py)
        ax, ay = px - x0, py - y0
        pxs.append(px)
        pys.append(py)
        for t in range(4):
            xx, yy = x0 + (t & 1), y0 + (t >> 1)
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            wt = w[:, :, l] * (ax if t & 1 else 1 - ax) * (ay if t >> 1 else 1 - ay) * inside
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
            for p in range(pts):                                   # one point at a time: the GPU-only case stays small
                term = wt[:, :, p, None] * values[l][idx[:, :, p:p + 1], hh][:, :, 0]
                out += term
                mass += term.abs()
    return out, mass, torch.stack(pxs, 2), torch.stack(pys, 2)


def _sides(p, size):
    """which of the issue's positions a pixel coordinate takes along one axis"""
    return {"below": p < -1, "low_edge": (p > -1) & (p < 0), "high_edge": (p > size - 1) & (p < size), "above": p >= size,
            "integer": (p == torch.floor(p)) & (p >= 0) & (p <= size - 1)}


def check_deform_attn(lib, dtype, rows, heads, d, shapes, family="onehot", shared=True, ld_value_extra=0, ld_out_extra=0, edges=False, seed=0):
    """family "onehot" / "uniform" (exact) or "general" (derived bound), see 1 of the module docstring.  shared: off and aw in one buffer, aw
    starting at column heads * LP * 2, both with its leading dimension (how the decoder passes them).  edges: the case must cover every position
    of a sampling point relative to its map in a ONE-HOT row.  Returns the kernel's largest error in spacings of T (0 in the exact families)."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    L, P = len(shapes), POINTS
    LP = L * P
    what = f"deform_attn {family} rows {rows} heads {heads} d {d} levels {shapes}"
    assert all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes), f"{what}: level sizes are powers of two"
    c = heads * d
    values = [torch.randint(-VALUE_CAP, VALUE_CAP + 1, (h * w, heads, d), generator=g).double().to(dev) for h, w in shapes]
    off = torch.randint(-12, 13, (rows, heads, L, P, 2), generator=g).double()
    ref = torch.empty(rows, 4, dtype=torch.float64)
    ref[:, :2] = torch.randint(0, 65, (rows, 2), generator=g).double() / 64
    ref[:, 2:] = torch.tensor([0.125, 0.25], dtype=torch.float64)[torch.randint(0, 2, (rows, 2), generator=g)]
    ref[0::7, 0], ref[1::7, 0], ref[2::7, 1], ref[3::7, 1] = 0.0, 1.0, 0.0, 1.0          # reference points on the border (row 0: cx = 0)
    ref[4::7, :2] = torch.tensor([1.0, 0.0], dtype=torch.float64)                        # ... and in a corner
    rh = torch.arange(rows)[:, None] * heads + torch.arange(heads)[None, :]
    hot = rh % LP
    if family == "onehot":
        logits = torch.full((rows, heads, LP), -200.0, dtype=torch.float64)
        logits.scatter_(2, hot[..., None], 0.0)
        w = torch.zeros(rows, heads, LP, dtype=torch.float64).scatter_(2, hot[..., None], 1.0)
        q = 2.0 ** -12
        assert rows * heads < LP or set(hot.flatten().tolist()) == set(range(LP)), f"{what}: the hot index must visit every (level, point)"
    elif family == "uniform":
        assert LP & (LP - 1) == 0, f"{what}: L * P must be a power of two"
        logits = ((torch.arange(rows) % 9 - 4).double() / 2)[:, None, None].expand(rows, heads, LP).contiguous()     # a constant per row
        w = torch.full((rows, heads, LP), 1.0 / LP, dtype=torch.float64)
        q = 2.0 ** -12 / LP
    else:
        assert family == "general"
        logits = torch.randint(-128, 129, (rows, heads, LP), generator=g).double() / 16
        w = torch.softmax(logits, dim=-1)
        q = None
    assert _exact_in(logits, td) and _exact_in(off, td) and all(_exact_in(v, td) for v in values), f"{what}: precondition — the inputs are not exact in the storage type"
    off, ref, w = off.to(dev), ref.to(dev), w.to(dev)
    want, mass, px, py = _deform_ref(values, off, w.view(rows, heads, L, P), ref, shapes)
    if q is not None:
        assert bool((mass / q == torch.floor(mass / q)).all()) and float(mass.max()) / q < EXACT, f"{what}: precondition — the taps' sum is not exact in fp32"
        want = _round(want, td)
        assert rows < 8 or float((want != 0).double().mean()) > 0.3, f"{what}: precondition — too few outputs are nonzero"
    if edges:
        assert family == "onehot"
        hot_l = (hot // P).to(dev)
        hx, hy = px.flatten(2).gather(2, hot.to(dev)[..., None])[..., 0], py.flatten(2).gather(2, hot.to(dev)[..., None])[..., 0]
        Wl = torch.tensor([s[1] for s in shapes], device=dev)[hot_l].double()
        Hl = torch.tensor([s[0] for s in shapes], device=dev)[hot_l].double()
        sx, sy = _sides(hx, Wl), _sides(hy, Hl)
        for k in sx:
            assert int(sx[k].sum()) > 0 and int(sy[k].sum()) > 0, f"{what}: precondition — no hot sampling point is '{k}' in x and in y"
        assert int(((sx["low_edge"] | sx["high_edge"]) & (sy["low_edge"] | sy["high_edge"])).sum()) > 0, f"{what}: precondition — no hot point in a corner"
        assert int((sx["below"] & (want.abs().sum(-1) == 0)).sum()) > 0
        cxh = ref[:, 0, None].expand(rows, heads)
        assert int((cxh == 0).sum()) > 0 and int((cxh == 1).sum()) > 0, f"{what}: precondition — no reference point on the border"

    pb = PlanBuilder(lib, dev, dtype)
    ldv, ldo = c + ld_value_extra, c + ld_out_extra
    vb = pb.buf((sum(h * w for h, w in shapes) + 1, ldv), td)
    vb.fill_(GARBAGE)
    vb[:-1, :c] = torch.cat([v.reshape(-1, c) for v in values]).to(td)
    refb = pb.buf((rows, 8), torch.float32)
    refb.fill_(GARBAGE)
    refb[:, :4] = ref.float()
    if shared:
        ld = heads * LP * 3 + 8
        ob = pb.buf((rows, ld), td)
        ob.fill_(GARBAGE)
        ob[:, :heads * LP * 2] = off.reshape(rows, -1).to(td)
        ob[:, heads * LP * 2:heads * LP * 3] = logits.reshape(rows, -1).to(td).to(dev)
        offb, awb, kw = ob, ob[:, heads * LP * 2:], dict(ld_off=ld, ld_aw=ld)
    else:
        offb, awb, kw = pb.const(off.reshape(rows, -1).to(td)), pb.const(logits.reshape(rows, -1).to(td)), {}
    out = _guarded(pb, rows, ldo, td)
    pb.deform_attention(vb, offb, awb, refb, out, rows, heads, d, shapes, P, OFFSET_SCALE, ld_value=ldv, ld_out=ldo, **kw)
    _run(pb)
    _assert_guard(out, rows, c, what)
    got = out[:rows, :c].view(rows, heads, d)
    if q is not None:
        _assert_equal(got, want, what)
        return 0.0
    e = VALUE_CAP * (2.0 ** -18 + 2.0 ** -22 + (5 * LP + 4) * U)
    sp = _spacing(want, dtype)
    err = (got.double() - want).abs()
    worst, share = float((err / sp).max()), float((err / (0.5 * sp + 2 * e)).max())      # (spacings: large only where the reference is near zero)
    print(f"{what} [{NAME[dtype]}]: fp32 term {2 * e:.3g}, kernel error {worst:.4f} spacings, {share:.3f} of the derived bound")
    _note("detr.deform_attn", **{f"{NAME[dtype]}_kernel_err_spacings": worst, f"{NAME[dtype]}_err_over_bound": share, "fp32_term": 2 * e})
    _assert_within(got, want, 0.5 * sp + 2 * e, what)
    return worst


LEVELS4 = [(8, 16), (4, 8), (2, 4), (1, 2)]
DEFORM_CASES = [
    dict(rows=300, heads=8, d=32, shapes=LEVELS4, family="onehot", edges=True, ld_value_extra=8, ld_out_extra=16),
    dict(rows=37, heads=8, d=8, shapes=LEVELS4, family="onehot", shared=False),
    dict(rows=1, heads=1, d=8, shapes=[(8, 16)], family="onehot"),
    dict(rows=23, heads=1, d=32, shapes=[(4, 8)], family="onehot", ld_out_extra=8),
    dict(rows=300, heads=8, d=32, shapes=LEVELS4, family="uniform", ld_value_extra=16),
    dict(rows=37, heads=8, d=8, shapes=LEVELS4[:2], family="uniform", shared=False, ld_out_extra=8),
    dict(rows=1, heads=8, d=32, shapes=LEVELS4, family="uniform"),
    dict(rows=300, heads=8, d=32, shapes=LEVELS4[:3], family="general"),
    dict(rows=37, heads=1, d=8, shapes=LEVELS4[:3], family="general", shared=False, ld_value_extra=8),
]
DEFORM_CASES_GPU = [
    dict(rows=4100, heads=8, d=256, shapes=[(1, 2)], family="onehot"),      # 4100 * 8 * 32 threads' worth > 4096 * 256: a second grid-stride trip
]


# ---- 2. box refinement --------------------------------------------------------------------------------------------------------------------
EPS5 = float(np.float32(1e-5))


def check_box_refine(lib, dtype, rows, kind=1, ld_delta=8, with_t=True, seed=0):
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    what = f"box_refine kind {kind} rows {rows} ld_delta {ld_delta}"
    one = np.float32(1.0)
    if kind == 1:
        edge = np.array([0.0, 1.0, -0.25, 1.5, 1e-5, np.nextafter(np.float32(1e-5), np.float32(0)), np.nextafter(np.float32(1e-5), one),
                         one - np.float32(1e-5), np.nextafter(one - np.float32(1e-5), np.float32(0)), np.nextafter(one - np.float32(1e-5), one), 0.5], dtype=np.float32)
        dl = torch.tensor([0.0, 32.0, -32.0, 1.0, -0.5], dtype=torch.float64)
        r = torch.rand(rows, 4, generator=g).float()
        delta = torch.randint(-64, 65, (rows, 4), generator=g).double() / 16
        i = torch.arange(rows * 4).view(rows, 4)
        sel = (i % 3 == 0)                                          # a third of the elements walk through edge x delta
        r[sel] = torch.from_numpy(edge)[(i[sel] // 3) % len(edge)]
        delta[sel] = dl[(i[sel] // 3 // len(edge)) % len(dl)]
        assert _exact_in(delta, td)
        v = r.double().clamp(0.0, 1.0)
        lg = torch.log(v.clamp_min(EPS5) / (1.0 - v).clamp_min(EPS5))
        x = delta + lg
        assert float(lg.abs().max()) < 16.0
        dx = 3 * U + 2.0 ** -20 + U * x.abs()
    else:
        anchors = torch.tensor([0.0, 200.0, -200.0], dtype=torch.float64)
        x = (torch.rand(rows, 4, generator=g).double() * 24 - 12).float().double()
        i = torch.arange(rows * 4).view(rows, 4)
        sel = (i % 3 == 0)
        x[sel] = anchors[(i[sel] // 3) % 3]
        r, delta, dx = x.float(), None, torch.zeros_like(x)
    s = torch.sigmoid(x)
    bound = s * (1 - s) * (dx + 2 * U) + 3 * U * s
    if kind == 2:
        s = torch.where(x == -200.0, torch.zeros_like(s), s)       # float64 keeps 1e-87; fp32 cannot
        for a, b in ((0.0, 0.5), (200.0, 1.0), (-200.0, 0.0)):      # the exact anchors
            bound[x == a] = 0.0
            assert bool((s[x == a] == b).all()) and (rows < 3 or int((x == a).sum()) > 0)

    pb = PlanBuilder(lib, dev, dtype)
    rin = pb.buf((rows, 8), torch.float32)
    rin.fill_(GARBAGE)
    rin[:, :4] = r
    rout = _guarded(pb, rows, 8, torch.float32)
    rt = _guarded(pb, rows, 8, td) if with_t else None
    db = None
    if delta is not None:
        db = pb.buf((rows, ld_delta), td)
        db.fill_(GARBAGE)
        db[:, :4] = delta.to(td)
    pb.box_refine(rin, rout, rt, rows, delta=db, ld_delta=ld_delta)
    _run(pb)
    _assert_guard(rout, rows, 8, what)
    got = rout[:rows].cpu()
    assert bool((got[:, 4:] == 0).all()), f"{what}: columns 4..7 of ref_out must be zero"
    worst = _assert_within(got[:, :4], s, bound, what)             # a bound of zero: the exact anchors
    print(f"{what} [{NAME[dtype]}]: worst error {worst:.3f} of the derived bound")
    _note("detr.box_refine", **{f"kind{kind}_err_over_bound": worst})
    if with_t:
        _assert_guard(rt, rows, 8, what + " (T copy)")
        t = rt[:rows].cpu().double()
        assert bool((t[:, 4:] == 0).all()), f"{what}: columns 4..7 of the T copy must be zero"
        assert bool(((t - got.double()).abs() <= 0.5 * _spacing(got.double(), dtype)).all()), f"{what}: the T copy is not one rounding of the fp32 result"
    return worst


BOX_CASES = [dict(rows=1), dict(rows=256, ld_delta=24), dict(rows=257, with_t=False), dict(rows=300, ld_delta=24),
             dict(rows=1, kind=2), dict(rows=257, kind=2), dict(rows=300, kind=2, with_t=False)]


# ---- 3. YOLO head decode ------------------------------------------------------------------------------------------------------------------
def check_yolo_decode(lib, dtype, shapes, strides, family="onehot", nc=1, nm=32, reg_max=16, padded=True, ld_extra=0, box_f32=False, images=1, image=0, seed=0):
    """family: "onehot" / "equal" (exact boxes, exact scores from the logits 0 / +-200) or "general" (derived bounds).  padded: the class slice
    starts at 4 * reg_max and the mask coefficients 8 channels later (what the models pass); otherwise the packed layout (offsets 0)."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    R, nb = reg_max, 4 * reg_max
    what = f"yolo_decode {family} levels {shapes} nc {nc} nm {nm} {'padded' if padded else 'packed'}{' box_f32' if box_f32 else ''} image {image}/{images}"
    assert all(s & (s - 1) == 0 for s in strides) and nc <= 8
    cls_off, mc_off = (nb, nb + 8) if padded else (0, 0)
    chans = (nb + 8 + nm) if padded else (nb + nc + nm)
    ld = (chans + 7) // 8 * 8 + ld_extra
    pb = PlanBuilder(lib, dev, dtype)
    levels, box32, wants, bounds = [], [], [], []
    a0 = 0
    for (h, w), st in zip(shapes, strides):
        A = h * w
        ai = a0 + torch.arange(A)
        if family == "onehot":
            hot = (ai[:, None] * 4 + torch.arange(4)[None, :] * 5 + ai[:, None] // 4) % R
            bins = torch.full((A, 4, R), -200.0, dtype=torch.float64).scatter_(2, hot[..., None], 0.0)
            dist = hot.double()
        elif family == "equal":
            bins = ((ai % 7 - 3).double() / 2)[:, None, None].expand(A, 4, R).contiguous()
            dist = torch.full((A, 4), (R - 1) / 2.0, dtype=torch.float64)
        else:
            scale = 4096 if box_f32 else 16
            bins = torch.randint(-4 * scale, 4 * scale + 1, (A, 4, R), generator=g).double() / scale
            dist = (torch.softmax(bins, -1) * torch.arange(R).double()).sum(-1)
        if family == "general":
            cls = torch.randint(-256, 257, (A, nc), generator=g).double() / 16
            score = torch.sigmoid(cls)
            sb = score * (1 - score) * (2.0 ** -19 + 2.0 ** -23) + 3 * U * score
        else:
            cls = torch.tensor([0.0, 200.0, -200.0], dtype=torch.float64)[(ai[:, None] + torch.arange(nc)[None, :]) % 3]
            score = torch.tensor([0.5, 1.0, 0.0], dtype=torch.float64)[(ai[:, None] + torch.arange(nc)[None, :]) % 3]
            sb = torch.zeros_like(score)
        mc = torch.randn(A, nm, generator=g).to(td).double()
        ax, ay = (torch.arange(A) % w).double() + 0.5, (torch.arange(A) // w).double() + 0.5
        box = torch.stack([ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]], 1) * st
        bb = st * ((R - 1) * (2 * R + 5) * U + U * (box / st).abs()) if family == "general" else torch.zeros_like(box)
        if box_f32:
            assert family == "general"
            bins_t = bins.to(td).double()
            moved = (((torch.softmax(bins_t, -1) * torch.arange(R).double()).sum(-1) - dist).abs() * st > 4 * bb.max()).double().mean()
            assert float(moved) > 0.5, f"{what}: precondition — rounding the logits to T must move the boxes"
        else:
            assert _exact_in(bins, td)
        assert _exact_in(cls, td)
        wants.append(torch.cat([box, score, mc], 1))
        bounds.append(torch.cat([bb, sb, torch.zeros_like(mc)], 1))
        lv = pb.act(images, h, w, chans, ld=ld)
        lv.t.fill_(GARBAGE)
        co = cls_off or nb
        mo = mc_off or co + nc
        for im in range(images):                      # the other image holds the same head altered: reading it would move every output
            mine = im == image
            rowsv = lv.t[im].view(A, ld)
            rowsv[:, :nb] = (torch.rand(A, nb, generator=g) * 8 - 4).to(td) if box_f32 else (bins.reshape(A, nb) if mine else bins.reshape(A, nb).roll(1, 1)).to(td)
            rowsv[:, co:co + nc] = (cls if mine else -cls).to(td)
            rowsv[:, mo:mo + nm] = (mc if mine else mc + 1.0).to(td)
        levels.append(lv)
        if box_f32:
            b32 = pb.buf((images, A, nb), torch.float32)
            for im in range(images):
                b32[im] = (bins.reshape(A, nb) if im == image else bins.reshape(A, nb).roll(1, 1)).float()
            assert bool((b32[image].double().cpu() == bins.reshape(A, nb)).all())
            box32.append(b32)
        a0 += A
    want, bound = torch.cat(wants), torch.cat(bounds)
    total, cols = want.shape
    assert total % 256 != 0 and all((h * w) % 256 for h, w in shapes), f"{what}: anchor counts must be ragged"
    outb = pb.buf((images * total + 1, cols), torch.float32)
    outb.fill_(SENTINEL)
    out = outb[image * total:(image + 1) * total]
    pb.yolo_decode(levels, strides, nc, nm, R, out, cls_off=cls_off, mc_off=mc_off, box_f32=box32 if box_f32 else None, image=image)
    _run(pb)
    rest = torch.ones(images * total + 1, dtype=torch.bool)
    rest[image * total:(image + 1) * total] = False
    assert bool((outb.cpu()[rest] == SENTINEL).all()), f"{what}: rows of out beyond this image were written"
    got = out.cpu().double()
    _assert_equal(got[:, 4 + nc:], want[:, 4 + nc:], what + " (mask coefficients)")
    if family != "general":
        _assert_equal(got, want, what)
        return 0.0
    worst_b = _assert_within(got[:, :4], want[:, :4], bound[:, :4], what + " (boxes)")
    worst_s = _assert_within(got[:, 4:4 + nc], want[:, 4:4 + nc], bound[:, 4:4 + nc], what + " (scores)")
    print(f"{what} [{NAME[dtype]}]: boxes {worst_b:.3f}, scores {worst_s:.3f} of the derived bounds")
    _note("yolo_decode.general", box_err_over_bound=worst_b, score_err_over_bound=worst_s)
    return max(worst_b, worst_s)


YOLO3 = dict(shapes=[(20, 13), (7, 5), (3, 2)], strides=[8, 16, 32])
YOLO_CASES = [
    dict(**YOLO3, family="onehot", nc=1, nm=32),
    dict(**YOLO3, family="onehot", nc=3, nm=0, padded=False, ld_extra=8),
    dict(**YOLO3, family="equal", nc=3, nm=32, padded=False),
    dict(shapes=[(13, 20)], strides=[8], family="onehot", nc=1, nm=32, ld_extra=16),
    dict(shapes=[(17, 16), (5, 7), (3, 2), (1, 3)], strides=[4, 8, 16, 32], family="onehot", nc=3, nm=32),
    dict(shapes=[(17, 16), (5, 7), (3, 2), (1, 3)], strides=[4, 8, 16, 32], family="equal", nc=1, nm=0),
    dict(**YOLO3, family="general", nc=3, nm=32),
    dict(**YOLO3, family="general", nc=1, nm=32, box_f32=True),
    dict(**YOLO3, family="onehot", nc=1, nm=32, images=2, image=1),
    dict(**YOLO3, family="general", nc=1, nm=32, box_f32=True, images=2, image=1),
]


# ---- 4. mask selection --------------------------------------------------------------------------------------------------------------------
IOU_PATTERNS = [(9.0, 0.5, 0.5, 0.2, 1), (9.0, 0.2, 0.5, 0.5, 2), (9.0, 0.1, 0.2, 0.3, 3), (9.0, 0.3, 0.2, 0.1, 1), (9.0, 0.4, 0.4, 0.4, 1), (9.0, 0.1, 0.3, 0.2, 2)]


def check_mask_select(lib, n, pix, seed=0):
    dev = _dev(lib)
    g = torch.Generator().manual_seed(seed)
    what = f"mask_select n {n} pix {pix}"
    delta, thresh = np.float32(0.05), np.float32(0.98)
    assert np.float32(98) / np.float32(100) == thresh and np.float32(97) / np.float32(100) < thresh
    inf = np.float32(np.inf)
    above = np.array([np.nextafter(delta, inf), 1.0, 30.0], dtype=np.float32)                                         # counted twice
    between = np.array([delta, np.nextafter(delta, -inf), 0.0, np.nextafter(-delta, inf)], dtype=np.float32)          # counted once: +delta itself is not above
    below = np.array([-delta, np.nextafter(-delta, -inf), -30.0], dtype=np.float32)                                   # never: -delta itself is not above
    targets = [(0, 0), (98, 100), (97, 100), (pix, pix), (0, pix), (pix // 2, pix), (99, 100), (1, 3)]
    logits = np.empty((n, pix, 4), dtype=np.float32)
    want_counts = np.empty((n, 2), dtype=np.int32)
    for i in range(n):
        hi, lo = targets[i % len(targets)]
        lo = min(lo, pix)
        hi = min(hi, lo)
        v = np.concatenate([above[np.arange(hi) % 3], between[np.arange(lo - hi) % 4], below[np.arange(pix - lo) % 3]])
        v = v[torch.randperm(pix, generator=g).numpy()]
        logits[i, :, 0] = v
        logits[i, :, 1], logits[i, :, 2], logits[i, :, 3] = -v, 1.0, -1.0                  # channels that would change the counts if read
        want_counts[i] = (int((v > delta).sum()), int((v > -delta).sum()))
        assert tuple(want_counts[i]) == (hi, lo)
    iou = np.array([IOU_PATTERNS[(i // 2) % len(IOU_PATTERNS)][:4] for i in range(n)], dtype=np.float32)
    ai, au = want_counts[:, 0].astype(np.float32), want_counts[:, 1].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        stable = (au == 0) | (ai / au >= thresh)
    best = 1 + np.argmax(iou[:, 1:], axis=1)                        # numpy: the first maximum
    want_sel = np.where(stable, 0, best).astype(np.int32)
    if n >= 65:
        assert set(want_sel.tolist()) == {0, 1, 2, 3} and bool((want_counts[:, 1] == 0).any())
        assert any(tuple(c) == (98, 100) and s == 0 for c, s in zip(want_counts.tolist(), want_sel.tolist()))
        assert any(tuple(c) == (97, 100) and s > 0 for c, s in zip(want_counts.tolist(), want_sel.tolist()))
        seen = {IOU_PATTERNS[(i // 2) % len(IOU_PATTERNS)] for i in range(n) if not stable[i]}
        assert len(seen) == len(IOU_PATTERNS), f"{what}: precondition — every IoU pattern must decide once"

    pb = PlanBuilder(lib, dev, abi.BF16)
    lt, it = pb.const(torch.from_numpy(logits)), pb.const(torch.from_numpy(iou))
    counts = pb.buf((n + 1, 2), torch.int32)
    counts.fill_(int(GARBAGE))
    counts[n:] = int(SENTINEL)
    sel = pb.buf((n + 1,), torch.int32)
    sel.fill_(int(SENTINEL))
    pb.mask_select(lt, it, counts, sel, n, pix, delta=float(delta), thresh=float(thresh))
    plan = _run(pb)
    first = (counts.cpu().clone(), sel.cpu().clone())
    plan.run()
    _sync(lib)
    assert torch.equal(counts.cpu(), first[0]) and torch.equal(sel.cpu(), first[1]), f"{what}: a second run of the same plan gives other counts"
    assert bool((first[0][n:] == int(SENTINEL)).all()) and int(first[1][n]) == int(SENTINEL), f"{what}: written behind counts / sel"
    _assert_bytes(first[0][:n], torch.from_numpy(want_counts), what + " (counts)")
    _assert_bytes(first[1][:n], torch.from_numpy(want_sel), what + " (sel)")


MASK_CASES = [dict(n=1, pix=1), dict(n=65, pix=255), dict(n=1, pix=16384), dict(n=65, pix=16385), dict(n=3, pix=100)]


# ---- 5. resize + threshold ----------------------------------------------------------------------------------------------------------------
SRC_TD = {abi.F32: torch.float32, abi.BF16: torch.bfloat16, abi.F16: torch.float16}


def _resize_ref(maps, roi, hd, wd):
    """maps [n, hs, ws] float64 -> bilinear (align_corners = False) resize of the window to [n, hd, wd]"""
    ry, rx, rh, rw = roi
    return F.interpolate(maps[:, None, ry:ry + rh, rx:rx + rw], (hd, wd), mode="bilinear", align_corners=False)[:, 0]


def _crop_boxes(n, hd, wd):
    """fractional edges with an integer y1 (inclusive) and x2 (exclusive), an empty box, a box larger than the page"""
    b = [(wd / 8 + 0.5, float(hd // 8), float(wd - wd // 4), hd - hd / 4 + 0.5), (wd / 2.0, 1.0, wd / 2.0, hd - 1.0), (-5.0, -7.5, wd + 100.0, hd + 3.0)]
    return torch.tensor([b[i % 3] for i in range(n)], dtype=torch.float32)


def _apply_crop(mask, boxes):
    n, hd, wd = mask.shape
    x, y = torch.arange(wd).double()[None, None, :], torch.arange(hd).double()[None, :, None]
    b = boxes.double()[:, :, None, None]
    return mask & (x >= b[:, 0]) & (x < b[:, 2]) & (y >= b[:, 1]) & (y < b[:, 3])


def _launch_resize(lib, maps, layout, src_dtype, roi, hd, wd, thresh, boxes, what):
    """maps [n_maps, hs, ws] float64 laid out as the models do (see check_resize_exact) -> uint8 [n, hd, wd] from the kernel"""
    dev, sd = _dev(lib), SRC_TD[src_dtype]
    n_maps, hs, ws = maps.shape
    n = 3 if layout == "shared" else n_maps
    pb = PlanBuilder(lib, dev, abi.BF16)
    kw = {}
    if layout == "plain":
        src = pb.const(torch.cat([maps, torch.full((1, hs, ws), 2 * thresh + 1000.0, dtype=torch.float64)]).to(sd))
    elif layout == "sam":
        sel = (torch.arange(n) * 3 + 1) % 4
        s4 = (2 * thresh - maps)[..., None].repeat(1, 1, 1, 4)               # the other channels hold the map mirrored at thresh
        s4[torch.arange(n), :, :, sel] = maps
        assert _exact_in(s4, sd)
        src, kw = pb.const(s4.to(sd)), dict(pix_stride=4, sel=pb.const(sel.int()))
    elif layout == "proto":
        src, kw = pb.const(maps.permute(1, 2, 0).contiguous().to(sd)), dict(pix_stride=n, batch_stride=1)
    else:
        assert layout == "shared" and n_maps == 1
        src, kw = pb.const(maps[0].to(sd)), dict(batch_stride=0)
    if roi != (0, 0, hs, ws):
        kw["roi"] = roi
    if boxes is not None:
        kw["crop_xyxy"] = pb.const(boxes)
    dst = pb.buf((n + 1, hd, wd), torch.uint8)
    dst.fill_(BYTE_SENTINEL)
    pb.resize_threshold(src, dst, n, hs, ws, hd, wd, thresh, src_dtype, **kw)
    _run(pb)
    assert bool((dst[n] == BYTE_SENTINEL).all()), f"{what}: the spare image behind dst was written"
    return dst[:n].cpu()


def check_resize_exact(lib, src_dtype, layout, hs, ws, hd, wd, thresh=0.0, roi=None, crop=False, seed=0):
    """layout: "plain" [n, hs, ws]; "sam" [n, hs, ws, 4] with a channel picked per sample; "proto" [hs, ws, n] (batch_stride 1, pix_stride n);
    "shared" one map for all samples (batch_stride 0).  roi: (y, x, h, w) strictly inside the map, which holds +-1000 outside it."""
    g = torch.Generator().manual_seed(seed)
    what = f"resize_threshold exact {layout} {NAME[src_dtype]} {hs}x{ws} -> {hd}x{wd} thresh {thresh} roi {roi} crop {crop}"
    n_maps = 1 if layout == "shared" else 3
    roi = roi or (0, 0, hs, ws)
    ry, rx, rh, rw = roi
    maps = 1000.0 * (1 - 2 * ((torch.arange(hs)[:, None] + torch.arange(ws)[None, :]) % 2)).double().expand(n_maps, hs, ws).contiguous()
    maps[:, ry:ry + rh, rx:rx + rw] = thresh + torch.tensor([-4.0, 0.0, 0.0, 4.0, 1.0, -2.0], dtype=torch.float64)[torch.randint(0, 6, (n_maps, rh, rw), generator=g)]
    assert _exact_in(maps, SRC_TD[src_dtype]) and float(thresh) == float(np.float32(thresh))
    for s_, d_ in ((rh, hd), (rw, wd)):
        assert s_ / d_ == 2.0 ** round(np.log2(s_ / d_)), f"{what}: the scale must be dyadic"
    val = _resize_ref(maps, roi, hd, wd)
    assert bool((val * 64 == torch.floor(val * 64)).all()), f"{what}: precondition — the interpolated values are not exact"
    ties = float((val == thresh).double().mean())
    assert 0.02 < ties and 0.1 < float((val > thresh).double().mean()) < 0.9, f"{what}: precondition — needs ties with thresh ({ties:.1%}) and both outcomes"
    n = 3
    mask = (val > thresh).expand(n, hd, wd)
    boxes = None
    if crop:
        boxes = _crop_boxes(n, hd, wd)
        x2, y1 = int(boxes[0, 2]), int(boxes[0, 1])
        x1, y2 = int(boxes[0, 0]) + 1, int(boxes[0, 3]) + 1                 # the first column / the first row beyond
        assert float(boxes[0, 2]) == x2 < wd and float(boxes[0, 1]) == y1 > 0, f"{what}: box 0 needs an integer right and top edge inside the page"
        assert all(bool(m.any()) for m in (mask[0, y1:y2, x2], mask[0, y1:y2, x1 - 1], mask[0, y1, x1:x2], mask[0, y1 - 1, x1:x2], mask[0, y2, x1:x2])), \
            f"{what}: precondition — the uncropped mask must be set just outside and on every edge of box 0"
        mask = _apply_crop(mask, boxes)
        assert not bool(mask[1].any()) and bool(mask[0].any()) and bool(mask[2].any())
    got = _launch_resize(lib, maps, layout, src_dtype, roi, hd, wd, thresh, boxes, what)
    _assert_bytes(got, mask.to(torch.uint8), what)


RESIZE_CASES = [
    dict(src_dtype=abi.F32, layout="plain", hs=16, ws=16, hd=64, wd=64),
    dict(src_dtype=abi.BF16, layout="plain", hs=16, ws=16, hd=32, wd=32, thresh=3.0),
    dict(src_dtype=abi.F16, layout="plain", hs=32, ws=32, hd=16, wd=16, thresh=3.0, crop=True),
    dict(src_dtype=abi.F32, layout="sam", hs=8, ws=12, hd=32, wd=48, crop=True),
    dict(src_dtype=abi.BF16, layout="sam", hs=16, ws=16, hd=64, wd=64, thresh=3.0),
    dict(src_dtype=abi.F16, layout="proto", hs=16, ws=16, hd=32, wd=32, crop=True),
    dict(src_dtype=abi.BF16, layout="proto", hs=20, ws=24, hd=32, wd=48, roi=(5, 7, 8, 12), crop=True, thresh=3.0),
    dict(src_dtype=abi.F32, layout="shared", hs=16, ws=16, hd=64, wd=64, crop=True),
    dict(src_dtype=abi.F16, layout="shared", hs=40, ws=36, hd=16, wd=16, roi=(3, 2, 32, 32), crop=True),
    dict(src_dtype=abi.F32, layout="plain", hs=24, ws=20, hd=64, wd=64, roi=(4, 1, 16, 16), thresh=3.0),
]


def check_resize_general(lib, roi=None, thresh=0.0, seed=0):
    """non-dyadic scales from fp32 sources of magnitude 8 .. 64 and random sign, see 5 of the module docstring; returns the share left out"""
    g = torch.Generator().manual_seed(seed)
    hs = ws = 16
    hd, wd = 37, 29
    roi = roi or (0, 0, hs, ws)
    what = f"resize_threshold general roi {roi} -> {hd}x{wd}"
    maps = ((torch.rand(3, hs, ws, generator=g) * 56 + 8) * (torch.randint(0, 2, (3, hs, ws), generator=g) * 2 - 1)).float().double()
    val = _resize_ref(maps, roi, hd, wd)
    win = maps[:, roi[0]:roi[0] + roi[2], roi[1]:roi[1] + roi[3]]
    G = max(float((win[:, 1:] - win[:, :-1]).abs().max()), float((win[:, :, 1:] - win[:, :, :-1]).abs().max()))
    D = 2 * G * (2.0 ** -19 + 2.0 ** -25) + 7 * U * float(win.abs().max())
    out = (val - thresh).abs() <= D
    share = float(out.double().mean())
    assert share < 0.01, f"{what}: precondition — {share:.2%} of the pixels lie within {D:.3g} of thresh"
    got = _launch_resize(lib, maps, "plain", abi.F32, roi, hd, wd, thresh, None, what)
    want = (val > thresh).to(torch.uint8)
    print(f"{what}: distance {D:.3g}, share left out {share:.3%} (cap 1 %)")
    _note("resize_threshold.general", left_out_share=share, distance=D)
    _assert_bytes(torch.where(out, want, got), want, what)
    return share


# ---- 6. page boundary conversions ---------------------------------------------------------------------------------------------------------
def _valid_mask(h, w, u, valid):
    """destination pixels that keep their value: the first source pixel lies inside the valid size"""
    vh, vw = valid if valid is not None else (h, w)
    return ((torch.arange(h // u) * u < vh)[:, None] & (torch.arange(w // u) * u < vw)[None, :])


def check_u8_to_nhwc(lib, dtype, mul, add, n=2, h=16, w=16, unshuffle=1, c_pad=8, valid=None):
    dev, td = _dev(lib), TD[dtype]
    what = f"image_convert u8 -> nhwc [{NAME[dtype]}] n {n} {h}x{w} u {unshuffle} c_pad {c_pad} mul {mul} add {add} valid {valid}"
    i = np.arange(n * h * w).reshape(n, h, w)
    src = np.stack([(i * (2 * c + 1) + 17 * c + 5 * (i // (h * w))) % 256 for c in range(3)], -1).astype(np.uint8)
    assert h * w < 256 or all(len(np.unique(src[k, :, :, c])) == 256 for k in range(n) for c in range(3)), f"{what}: every byte value in every channel"
    v = src.astype(np.float32) / np.float32(255)
    two = v * np.float32(mul) + np.float32(add)
    fused = (v.astype(np.float64) * mul + add).astype(np.float32)
    assert np.array_equal(two, fused), f"{what}: precondition — the fused and the two-step form must agree"
    u = unshuffle
    want = F.pixel_unshuffle(torch.from_numpy(two).permute(0, 3, 1, 2), u).permute(0, 2, 3, 1).to(td)        # c * u * u + dy * u + dx
    want = F.pad(want, (0, c_pad - 3 * u * u)) * _valid_mask(h, w, u, valid)[None, :, :, None].to(td)
    pb = PlanBuilder(lib, dev, dtype)
    dst = _guarded(pb, n * (h // u) * (w // u), c_pad, td)
    vt = pb.const(torch.tensor(valid, dtype=torch.int32)) if valid is not None else None
    pb.image_convert(abi.IMG_HWC_U8_TO_NHWC, pb.const(torch.from_numpy(src)), dst, n, h, w, c_pad, unshuffle=u, mul=mul, add=(add, add, add), valid_hw=vt)
    _run(pb)
    _assert_guard(dst, n * (h // u) * (w // u), c_pad, what)
    _assert_equal(dst[:-1].view(want.shape).cpu(), want.double(), what)


def _census(td):
    """every finite value of the 16-bit type in [-0.5, 1.5]"""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(td).float()
    return v[torch.isfinite(v) & (v >= -0.5) & (v <= 1.5)]


def check_nhwc_to_u8(lib, dtype, mul, add, c_pad=8):
    dev, td = _dev(lib), TD[dtype]
    what = f"image_convert nhwc -> u8 [{NAME[dtype]}] census mul {mul} add {add}"
    v = _census(td)
    w = 128
    h = (v.numel() + w - 1) // w
    v = torch.cat([v, v[:h * w - v.numel()]])
    assert v.numel() > 20000 and float(v.min()) == -0.5 and float(v.max()) == 1.5
    x = torch.stack([v, v.roll(1), v.flip(0)], -1).view(1, h, w, 3)
    t = x.numpy() * np.float32(mul) + np.float32(add)
    assert np.array_equal(t, (x.numpy().astype(np.float64) * mul + add).astype(np.float32)), f"{what}: precondition — one rounding, fused or not"
    want = torch.from_numpy((np.clip(t, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8))
    pb = PlanBuilder(lib, dev, dtype)
    a = pb.act(1, h, w, c_pad)
    a.t.fill_(GARBAGE)
    a.t[..., :3] = x.to(td)
    dst = _guarded(pb, h * w, 3, torch.uint8, fill=BYTE_SENTINEL)
    pb.image_convert(abi.IMG_NHWC_TO_HWC_U8, a.t, dst, 1, h, w, c_pad, mul=mul, add=(add, add, add))
    _run(pb)
    _assert_guard(dst, h * w, 3, what, fill=BYTE_SENTINEL)
    _assert_bytes(dst[:-1].view(1, h, w, 3), want, what)


def check_nchw(lib, dtype, n=2, h=6, w=10, unshuffle=1, c_pad=8, valid=None, seed=0):
    """MTX_IMG_NCHW_F32_TO_NHWC and back through MTX_IMG_NHWC_TO_NCHW_F32 on integers: both exact; n = 2 exercises the (n * 3 + c) plane index"""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    what = f"image_convert nchw [{NAME[dtype]}] n {n} {h}x{w} u {unshuffle} valid {valid}"
    u = unshuffle
    x = torch.randint(-60, 61, (n, 3, h, w), generator=g).double()
    add = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    want = F.pixel_unshuffle(x * 2.0 + add.view(1, 3, 1, 1), u).permute(0, 2, 3, 1)
    want = F.pad(want, (0, c_pad - 3 * u * u)) * _valid_mask(h, w, u, valid)[None, :, :, None]
    assert _exact_in(want, td)
    pb = PlanBuilder(lib, dev, dtype)
    pix = n * (h // u) * (w // u)
    dst = _guarded(pb, pix, c_pad, td)
    vt = pb.const(torch.tensor(valid, dtype=torch.int32)) if valid is not None else None
    pb.image_convert(abi.IMG_NCHW_F32_TO_NHWC, pb.const(x.float()), dst, n, h, w, c_pad, unshuffle=u, mul=2.0, add=tuple(add.tolist()), valid_hw=vt)
    back = None
    if u == 1 and valid is None:
        back = _guarded(pb, n * 3, h * w, torch.float32)
        pb.image_convert(abi.IMG_NHWC_TO_NCHW_F32, dst, back, n, h, w, c_pad, mul=0.5, add=(-0.5, -1.0, -1.5))
    _run(pb)
    _assert_guard(dst, pix, c_pad, what)
    _assert_equal(dst[:-1].view(want.shape).cpu(), want, what)
    if back is not None:
        _assert_guard(back, n * 3, h * w, what + " (back)")
        _assert_equal(back[:-1].view(n, 3, h, w).cpu(), x, what + " (back)")


def check_u8_round_trip_large(lib, dtype, side=1450):
    """GPU only: more than 8192 * 256 pixels through kind 3 and back through kind 2 (a second grid-stride trip in both); the bytes used are those
    the T grid returns unchanged, taken from the reference alone"""
    dev, td = _dev(lib), TD[dtype]
    what = f"image_convert round trip {side}x{side} [{NAME[dtype]}]"
    assert side * side > 8192 * 256
    b = np.arange(256, dtype=np.float32)
    back = (np.clip((torch.from_numpy(b / np.float32(255)).to(td).float().numpy()), 0, 1) * np.float32(255)).astype(np.uint8)
    keep = torch.from_numpy(np.nonzero(back == np.arange(256))[0].astype(np.uint8))
    assert keep.numel() >= 64, f"{what}: precondition — only {keep.numel()} byte values survive the T grid"
    g = torch.Generator().manual_seed(0)
    src = keep[torch.randint(0, keep.numel(), (1, side, side, 3), generator=g)]
    pb = PlanBuilder(lib, dev, dtype)
    a = pb.act(1, side, side, 8)
    st = pb.const(src)
    pb.image_convert(abi.IMG_HWC_U8_TO_NHWC, st, a.t, 1, side, side, 8)
    dst = _guarded(pb, side * side, 3, torch.uint8, fill=BYTE_SENTINEL)
    pb.image_convert(abi.IMG_NHWC_TO_HWC_U8, a.t, dst, 1, side, side, 8)
    _run(pb)
    _assert_guard(dst, side * side, 3, what, fill=BYTE_SENTINEL)
    assert bool((a.t[..., 3:] == 0).all()), f"{what}: padding channels must be zero"
    _assert_bytes(dst[:-1].view(src.shape), src, what)


# ---- 7. letterbox -------------------------------------------------------------------------------------------------------------------------
def check_letterbox(lib, dtype, h, w, new_h, new_w, pad=(0, 0, 0, 0), exact=True, seed=0):
    """pad: (top, bottom, left, right).  exact: dyadic ratios, zero differing elements; otherwise pixels within the derived distance of a
    half-integer are left out (7 of the module docstring).  Returns the share left out."""
    dev, td = _dev(lib), TD[dtype]
    g = torch.Generator().manual_seed(seed)
    top, bottom, left, right = pad
    oh, ow = new_h + top + bottom, new_w + left + right
    what = f"letterbox [{NAME[dtype]}] {h}x{w} -> {new_h}x{new_w} pad {pad}"
    levels = np.arange(256, dtype=np.float32)
    lut = torch.from_numpy(levels * (np.float32(1) / np.float32(255))).to(td)
    assert torch.equal(lut, (torch.arange(256).double() / 255).to(td)), f"{what}: precondition — * (1 / 255) and / 255 must agree in T"
    yy, xx = torch.arange(h)[:, None], torch.arange(w)[None, :]
    if exact:
        img = torch.randint(0, 256, (h, w, 3), generator=g)
    else:       # a distinct smooth ramp per channel plus a little noise: the gradient G stays small
        img = torch.stack([(2 * yy + xx) // 2 + 10, 220 - yy - xx, 3 * yy // 2 + 40 + 0 * xx], -1)
        img = (img + torch.randint(-4, 5, (h, w, 3), generator=g)).clamp(0, 255)
    assert not torch.equal(img[..., 0], img[..., 2])
    rgb = img.flip(-1).permute(2, 0, 1)[None].double()                       # the source is BGR
    val = F.interpolate(rgb, (new_h, new_w), mode="bilinear", align_corners=False) if (new_h, new_w) != (h, w) else rgb
    frac = val - torch.floor(val)
    if exact:
        assert bool((val * 256 == torch.floor(val * 256)).all()), f"{what}: precondition — the interpolated values are not exact"
        half_even = int(((frac == 0.5) & (torch.floor(val) % 2 == 0)).sum())
        assert (new_h, new_w) == (h, w) or half_even >= 10, f"{what}: precondition — only {half_even} values k + 0.5 with k even"
        out = torch.zeros_like(val, dtype=torch.bool)
        share = 0.0
    else:
        Gy = float((rgb[:, :, 1:] - rgb[:, :, :-1]).abs().max())
        Gx = float((rgb[:, :, :, 1:] - rgb[:, :, :, :-1]).abs().max())
        assert max(h, w) <= 128
        D = (Gy + Gx) * (2.0 ** -16 + 2.0 ** -25) + 7 * U * 255
        out = (frac - 0.5).abs() <= D
        share = float(out.double().mean())
        print(f"{what}: distance {D:.3g}, share left out {share:.3%} (cap 1 %)")
        _note("letterbox.general", left_out_share=share, distance=D)
        assert share < 0.01, f"{what}: precondition — {share:.2%} of the pixels lie within {D:.3g} of a half-integer"
    level = torch.round(val)                                                 # half to even
    canvas = torch.full((oh, ow, 3), 114, dtype=torch.long)
    canvas[top:top + new_h, left:left + new_w] = level[0].permute(1, 2, 0).long()
    want = F.pad(lut[canvas], (0, 5))
    skip = torch.zeros(oh, ow, 8, dtype=torch.bool)
    skip[top:top + new_h, left:left + new_w, :3] = out[0].permute(1, 2, 0)

    pb = PlanBuilder(lib, dev, dtype)
    buf = _guarded(pb, oh * ow, 8, td)
    dst = Act(buf[:-1].view(1, oh, ow, 8), 1, oh, ow, 3)
    pb.letterbox(pb.const(img.to(torch.uint8)), dst, h, w, new_h, new_w, top, left)
    _run(pb)
    _assert_guard(buf, oh * ow, 8, what)
    got = buf[:-1].view(oh, ow, 8).cpu()
    _assert_equal(torch.where(skip, want, got), want.double(), what)
    return share


LETTERBOX_CASES = [
    dict(h=24, w=40, new_h=48, new_w=80, pad=(0, 0, 0, 0)),
    dict(h=48, w=80, new_h=24, new_w=40, pad=(4, 4, 0, 0)),
    dict(h=16, w=16, new_h=64, new_w=64, pad=(3, 4, 5, 6)),
    dict(h=19, w=27, new_h=19, new_w=27, pad=(2, 3, 0, 1)),                 # identity size: a pure copy / flip
    dict(h=37, w=91, new_h=26, new_w=64, pad=(3, 3, 0, 0), exact=False),
    dict(h=50, w=70, new_h=64, new_w=90, pad=(0, 1, 3, 3), exact=False),
]

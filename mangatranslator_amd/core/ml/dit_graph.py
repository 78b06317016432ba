"""What the FLUX.1-Kontext (core/ml/flux.py) and FLUX.2-Klein (core/ml/flux2.py) step graphs share, and nothing else: the holder of one
linear's weight (16-bit or MX fp8), its one-off quantisation at load, the recorder of the ops both MMDiTs are wired from, and the cache
of modulation rows.  Parameter names, block wiring, lane placement and the decisions about who writes which fp8 operand stay in the
model files.

One rule for fp8 operands, at every site: a producer's rows are quantised only if some consumer's weight is on the fp8 path — by the
producer itself where the model says so (same bytes), else by a `mtx_quantize_mx` launch behind it."""
import math

import torch

from ...hip.plan import Act, PlanBuilder


def _rows(t2d, r0, r1, c0=0, c=None):
    """Act view of rows [r0, r1) and columns [c0, c0+c) of a [R, LD] buffer."""
    v = t2d[r0:r1]
    return Act(v.view(1, 1, r1 - r0, t2d.shape[1]), 1, 1, r1 - r0, c if c is not None else t2d.shape[1] - c0, c0)


class Weight:
    """one linear's weight: the 16-bit [N, K] tensor, or (fp8) its MX copy — e4m3 bytes [N, K] + E8M0 scale plane [K / 128, lds], the 16-bit
    tensor dropped: half the resident bytes — and the fp32 bias, where the model has one"""

    def __init__(self, w16=None, q=None, scale=None, lds=0, bias=None):
        self.w16, self.q, self.scale, self.lds, self.bias = w16, q, scale, lds, bias
        self.fp8 = q is not None


def quantize_weight(lib, device, dtype, w16: torch.Tensor, bias=None) -> Weight:
    """the MX fp8 copy of a 16-bit weight, made once at load by a plan of its own"""
    n, k = w16.shape
    pb = PlanBuilder(lib, device, dtype)
    q, scale, lds = pb.quantize(w16, n, k)
    pb.build().run()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return Weight(q=q, scale=scale, lds=lds, bias=bias)


class DiTStep:
    """Buffers and op recording of one denoising step over a [T, D] token buffer.  The buffers are allocated once, through the builder given
    here; every recording method takes the builder it records on, so that several plans (the head / body / skip plans of Kontext's
    first-block cache) can share them."""

    def __init__(self, pb: PlanBuilder, T, D, H, n_vec, rope_tab: torch.Tensor, fp8: bool, fused_quant: bool):
        """rope_tab: fp32 [T, 2, hd / 2] cos | sin.  fp8: some linear runs on the fp8 kernel (the twins exist).  fused_quant: the adaLN norms
        write their consumers' fp8 operand themselves"""
        self.T, self.D, self.H, self.hd = T, D, H, D // H
        self.lds = (T + 63) // 64 * 64                  # row stride of every twin's scale plane
        self.fp8, self.fused_quant = fp8, fused_quant
        self.mod = pb.buf((n_vec, D), pb.tdtype)
        # rotary tables [2][T, 2, hd/2]: plain (k heads) and pre-multiplied by softmax scale * log2(e) (q heads), so q leaves the
        # norm+rope kernel as base-2 logit factors after its ONE rounding and the attention kernel spends no VALU slot on scaling
        q_fold = (1.0 / math.sqrt(self.hd)) * 1.4426950408889634
        self.cs = pb.hold(torch.stack([rope_tab, rope_tab * q_fold]).to(pb.device).contiguous())[0]
        self.x = pb.buf((T, D), pb.tdtype)
        self.nrm = pb.buf((T, D), pb.tdtype)
        self.nrm8 = self.twin(pb, D)

    def twin(self, pb, k):
        """fp8 twin of a [T, k] GEMM input: (e4m3 bytes, scale plane); None on the all-16-bit graph"""
        return (pb.buf((self.T, k), torch.uint8), pb.buf((k // 128, self.lds), torch.int32, zero=True)) if self.fp8 else None

    def quant(self, pb, src, ld, k, dst, r0, r1, label, c0=0):
        """rows [r0, r1), columns [c0, c0 + k) of src [T, ld] into the same place of its twin"""
        pb.quantize(src, r1 - r0, k, ldx=ld, x_off=r0 * ld + c0, q=dst[0], scale=dst[1], row_off=r0, lds=self.lds, ldq=ld, q_col_off=c0, label=label)

    def linear(self, pb, src, src8, w: Weight, r0, r1, n, k, out, ldc=None, c_col=0, label="linear", actq=None, **epi):
        """out[r0:r1, c_col : c_col + n] = epilogue(src[r0:r1, :k] W^T + bias) on the 16-bit or the fp8 kernel, as the weight says.  epi: the
        epilogue extras of `PlanBuilder.gemm` (gate, res, act, glu, ...); with actq (fp8 only) the result leaves as the MX fp8 operand of
        the next linear and `out` is not written"""
        m, ldc = r1 - r0, (ldc or n)
        if w.fp8:
            pb.gemm(src8[0], w.q, m, n, k, out=None if actq is not None else out, ldc=ldc, a_off=r0 * k, c_off=r0 * ldc + c_col, bias=w.bias,
                    f8=(src8[1], self.lds, w.scale, w.lds, r0, 0), label=label + ".f8", actq=actq, **epi)
        else:
            pb.gemm(src, w.w16, m, n, k, out=out, ldc=ldc, a_off=r0 * k, c_off=r0 * ldc + c_col, bias=w.bias, label=label, **epi)

    def adaln(self, pb, r0, r1, shift_i, scale_i, label, consumers=()):
        """adaLN LayerNorm of rows [r0, r1) of x into nrm.  With fp8 consumers the kernel writes their MX fp8 operand itself (mtx_norm_args.q:
        bit-identical to a quantiser pass over its 16-bit output, which is then only written if some consumer still reads 16-bit)"""
        D, mod = self.D, self.mod
        any8 = any(w.fp8 for w in consumers)
        to8 = any8 and self.fused_quant
        need16 = not to8 or any(not w.fp8 for w in consumers)
        pb.norm(self.x, self.nrm if need16 else None, r1 - r0, D, eps=1e-6, kind=0, mod_scale=mod[scale_i], mod_shift=mod[shift_i], rows_per=r1 - r0,
                ldmod=D, x_off=r0 * D, y_off=r0 * D, label=label, q8=self.nrm8 if to8 else None, q_row_off=r0, lds_q=self.lds)
        if any8 and not to8:
            self.quant(pb, self.nrm, D, D, self.nrm8, r0, r1, label + ".q")

    def rope(self, pb, buf, r0, r1, gamma_qk, label, qk_f8=None):
        """per-head RMSNorm + RoPE over the q AND k column slices (the first 2 D columns) of rows [r0, r1) of buf in one launch.
        qk_f8: e4m3 [T, 2 D] twin of the result, q times 8 (the operand of `attention(qk_f8=)`)"""
        pb.qk_norm_rope(_rows(buf, r0, r1, 0, 2 * self.D), self.cs[r0:], self.T * self.hd, gamma_qk, self.hd, self.H,
                        y8=(qk_f8[r0:], 2 * self.D, 8.0) if qk_f8 is not None else None, label=label)

    def attention(self, pb, src, out_t, label, q8=None, qk_f8=None, pv_f8=None):
        """joint attention over q | k | v in the first 3 D columns of src, into the first D columns of out_t.  q8: the twin of out_t — the rows
        leave as the MX fp8 operand of the projection that follows (mtx_attn_args.q8) and out_t is not written.  qk_f8: the rotary kernel's
        e4m3 twin, scores on the fp8 instruction; pv_f8 (with q8 and qk_f8): e4m3 V^T scratch [D, lds], P V on it too"""
        T, D, H, hd, ld, out_ld = self.T, self.D, self.H, self.hd, src.shape[1], out_t.shape[1]
        pv = pb.v_f8t(src, T, H, ld, v_off=2 * D, out=pv_f8, label=label + ".v_f8t") if (pv_f8 is not None and q8 is not None) else None
        pb.attention(src, src, src, None if q8 is not None else out_t, 1, H, T, T, hd, (0, ld, hd), (0, ld, hd), (0, ld, hd), (0, out_ld, hd),
                     1.0 / math.sqrt(hd), k_off=D, v_off=2 * D, label=label, q_prescaled=True,
                     q8=(q8[0], q8[1], out_ld, self.lds, 0) if q8 is not None else None,
                     qk_f8=(qk_f8, 0, D, 2 * D, -3) if qk_f8 is not None else None, pv_f8=pv)


class ModulationCache:
    """[n_vec, D] modulation rows of one denoising step by a key the model supplies (timestep, guidance, prompt): computed once per step of a
    schedule by the model's modulation plan (M = 1 GEMVs that stream every adaLN weight) instead of every step of every region"""

    def __init__(self, build_plan, n_vec, bound=256):
        self._build_plan, self._plan, self._rows, self.n_vec, self.bound = build_plan, None, {}, n_vec, bound

    def get(self, key, fill) -> torch.Tensor:
        """fill(plan): writes the plan's inputs for `key`; the plan leaves the rows in `plan.mods`"""
        if len(self._rows) > self.bound:          # a few schedules x prompts at most; never grow without bound
            self._rows.clear()
        if key not in self._rows:
            if self._plan is None:
                self._plan = self._build_plan()
            fill(self._plan)
            self._plan.run()
            self._rows[key] = self._plan.mods.view(self.n_vec, -1).clone()
        return self._rows[key]

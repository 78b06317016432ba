"""What the ViT-shaped graphs share (SAM-2.1's Hiera and SAM 3's ViT-L trunks, manga-ocr's encoder): the three ops of a pre-norm block in the
two arithmetics of the residual stream, and the page pre-plan (antialiased uint8 resize, then normalise)."""
import torch

from ...hip import abi
from ...hip.plan import PlanBuilder


def trunk_helpers(pb, eps, tdt, dtype, stream32):
    """(layer_norm, linear, close_branch) of a pre-norm ViT trunk recorded on `pb` with `tdt` / `dtype` as the storage type: every linear carries
    its weight triple (w, w_lo, bias) (core/ml/packing.py `linear`); with `stream32` the projections that close a branch take the fp32 residual in
    their epilogue and write fp32, and the LayerNorms read fp32 and round once, to the storage type of the GEMM that follows"""

    def layer_norm(x, rows, c, wb, label):
        """the operand of the linears that follow: [rows, c] of the storage type"""
        y = pb.buf((rows, c), tdt)
        if not stream32:
            return pb.norm(x, y, rows, c, ldy=c, gamma=wb[0], beta=wb[1], eps=eps, label=label)
        return pb.norm(x, y, rows, c, gamma=wb[0], beta=wb[1], eps=eps, dtype=abi.F32, out_dtype=dtype, label=label)

    def linear(a, wb, rows, n_out, k, label, **kw):
        return pb.gemm(a, wb[0], rows, n_out, k, bias=wb[2], w_lo=wb[1], label=label, **kw)

    def close_branch(a, wb, rows, n_out, k, res, label, **kw):
        """stream <- res + a @ W^T + b"""
        if not stream32:
            return linear(a, wb, rows, n_out, k, label, res=res, **kw)
        return linear(a, wb, rows, n_out, k, label, res=res, res_f32=True, out_f32=True, **kw)

    return layer_norm, linear, close_branch


def resize_normalise_plan(lib, device, dtype, h, w, img, mean, std, widen_f16=False):
    """the plan that takes a uint8 page [h, w, 3] (its `.page`) to `img`, a model's normalised input `Act`.  The HF image processors resize the
    uint8 page with torchvision's antialiased bilinear `resize`, i.e. ATen's fixed-point uint8 kernel (horizontal pass, uint8 intermediate,
    vertical pass), then rescale and normalise in fp32: the two passes run with ATen's own taps (core/image/device_tail.py
    aten_aa_bilinear_tables, pinned against the installed torch), the normalisation in the preprocess kernel at identity size.
    widen_f16 (an fp32 `img`; the pre-processing kernel writes 16-bit pixels): normalised into a staged f16 image, then widened into `img`"""
    from ..image.device_tail import aten_aa_bilinear_tables
    pb = PlanBuilder(lib, device, dtype)
    page = pb.buf((h, w, 3), torch.uint8)
    cur, cur_w = page, w
    for axis, (src, dst) in enumerate(((w, img.w), (h, img.h))):
        if src != dst:
            b, t, k, bits = aten_aa_bilinear_tables(src, dst)
            out_h, out_w = (h, dst) if axis == 0 else (dst, cur_w)
            tmp = pb.buf((out_h, out_w, 3), torch.uint8)
            pb.resample_u8(cur, tmp, out_h, out_w, 3, cur_w * 3, out_w * 3, pb.const(torch.from_numpy(b.reshape(-1))), pb.const(torch.from_numpy(t.reshape(-1))),
                           k, axis, bits, label="pre.resize_" + "hv"[axis])
            cur, cur_w = tmp, out_w
    if widen_f16:
        staged = PlanBuilder(lib, device, abi.F16).act(1, img.h, img.w, 8, zero=True)
        pb.hold(staged.t)
        a = pb.preprocess(cur, staged, img.h, img.w, mean, std, label="pre.normalise")
        pb.ops[-1].u.pre.dtype = abi.F16
        pb.cvt_f32(a, abi.F16, label="pre.widen", out=img)
    else:
        pb.preprocess(cur, img, img.h, img.w, mean, std, label="pre.normalise")
    plan = pb.build()
    plan.page = page
    return plan

"""The kernels' weight layouts, in one place: every model file of core/ml packs through these functions.

They take fp32 CPU tensors and return tensors; they know nothing of any model's key names (`layer_norm` / `linear` read the two keys every
checkpoint uses, `.weight` and `.bias`).  The cast to a model's storage type stays with the caller or with `on_device`: f32 -> f16 / bf16 is
round-to-nearest-even wherever it runs, so the order of the cast and the move does not change a byte.  A change here is checked by dumping
the toy models before and after with tools/plan_dump.py --weights (the model layer).
"""
import torch


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def conv_taps(w: torch.Tensor, cin_pad: int = 0, cout_pad: int = 0, cout_round: int = 1) -> torch.Tensor:
    """conv filters [Cout, Cin, kh, kw] -> fp32 [co_p, kh * kw, ci_p], tap-major and channel-contiguous, zero-padded: the conv kernel's packing.
    ci_p = max(Cin rounded up to 8, cin_pad), co_p = max(Cout rounded up to cout_round, cout_pad)"""
    co, ci, kh, kw = w.shape
    out = torch.zeros(max(_round_up(co, cout_round), cout_pad), kh * kw, max(_round_up(ci, 8), cin_pad), dtype=torch.float32)
    out[:co, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)
    return out


def padded_bias(b: torch.Tensor, co_p: int = 0) -> torch.Tensor:
    """bias [Cout] -> fp32 [max(Cout, co_p)], zero-padded"""
    out = torch.zeros(max(b.shape[0], co_p), dtype=torch.float32)
    out[:b.shape[0]] = b
    return out


def convt2x2_as_conv1x1(wt: torch.Tensor, bt: torch.Tensor, then_w=None, then_b=None):
    """ConvTranspose2d(k=2, s=2) weights [Cin, Cout, 2, 2] -> (w [4 Cout', 1, Cin], b [4 Cout']) of the 1x1 conv whose output rows
    ((dy * 2 + dx) * Cout' + co) the pixel-shuffle store scatters; `then_w` [Cout', Cout] / `then_b`: a 1x1 conv applied right after it, folded
    in (two chained linear maps)."""
    w = wt.permute(2, 3, 1, 0)                                         # [dy, dx, Cout, Cin]
    b = bt
    if then_w is not None:
        w = torch.einsum("oc,yxci->yxoi", then_w, w)
        b = then_w @ bt + then_b
    co, ci = w.shape[2], w.shape[3]
    return w.reshape(4 * co, 1, ci), b.repeat(4)


def patch_embed_rows(w: torch.Tensor) -> torch.Tensor:
    """patch-embedding filter [C, 3, p, p] -> [C, p * p * 8]: the rows of a GEMM over im2col columns of p * p taps x 8 channels (3 real)"""
    c, ci, p, _ = w.shape
    wk = torch.zeros(c, p * p, 8)
    wk[:, :, :ci] = w.permute(0, 2, 3, 1).reshape(c, p * p, ci)
    return wk.reshape(c, p * p * 8)


def on_device(t: torch.Tensor, device, dtype=torch.float32) -> torch.Tensor:
    """a tensor of the model on the device, contiguous and in storage of its own: a view into a checkpoint (a safetensors file maps tensors at any
    byte) may not have the 16-byte alignment the kernels want, and on the "cpu" simulator device `.to` alone would hand that view back"""
    return t.to(device=device, dtype=dtype, copy=True).contiguous()


def layer_norm(sd: dict, key: str, device):
    """(gamma, beta) fp32 of the LayerNorm at `key`"""
    return on_device(sd[key + ".weight"], device), on_device(sd[key + ".bias"], device)


def hi_lo(w: torch.Tensor, device, dtype, hilo: bool = False):
    """matrix [N, K] of a linear as the GEMM takes it: (W, None) in `dtype`, or with `hilo` the pair (W_hi, W_lo), W_lo = round(W - W_hi)"""
    if not hilo:
        return on_device(w, device, dtype), None
    hi = w.to(dtype)
    return on_device(hi, device, dtype), on_device(w - hi.float(), device, dtype)


def linear(sd: dict, *keys, device, dtype, hilo: bool = False):
    """(W, W_lo, bias) of the linear at `keys` — several keys stacked along N: q | k | v as one GEMM — with W as `hi_lo` gives it and the bias fp32"""
    return (*hi_lo(torch.cat([sd[k + ".weight"] for k in keys], 0), device, dtype, hilo), on_device(torch.cat([sd[k + ".bias"] for k in keys], 0), device))

"""Checks of the decode-step kernels (csrc/decode.hip: MTX_OP_DECODE_ATTN, MTX_OP_ROWLIN), written once and run on the simulator
(tests/test_manga_ocr_sim.py) and on the product library (tests/test_manga_ocr_gpu.py).

Decode attention, exact: with all keys equal the softmax is uniform (every weight is exp(0) = 1, every merge factor too), the numerator is a sum of
integers and the denominator a power of two, so the output is ONE rounding of an exactly known mean: zero differing elements.
Decode attention, random: against fp32 torch on the same 16-bit inputs.  The bound is half a spacing of T at the reference (the one rounding) plus
the fp32 softmax's own error over at most 300 keys, 300 * 2^-23 of the largest value.
Skinny linear, exact: integer operands make every partial sum exact in any order, so the kernel must give the bytes of mtx_gemm (whose rounding
points tests/exact_checks.py pins); on random data both are held to float64 with the bound of their common contract.
Skinny linears, contract: `check_rowlin_contract_exact` holds MTX_OP_ROWLIN and MTX_OP_ROWLIN_WIDE to float64 with those rounding points directly,
for every (RT, NW) instantiation (`rowlin_tiling` restates the launchers' rule), so that neither mtx_gemm nor the other linear is the witness."""
import ctypes as C

import pytest
import torch

from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _run, _sync

TD = dict(TD)
TD[abi.F32] = torch.float32               # the decode kernels also come in fp32 (the recogniser's precision "high")
MANT = {abi.BF16: 7, abi.F16: 10, abi.F32: 23}
HEADS, D = 2, 64
HD = HEADS * D


def _bits(t):
    return t.contiguous().view(torch.int16)


NAN_BITS = 0x7FC1                    # a NaN bit pattern of both 16-bit types


def _src_table(max_len, slots, rows):
    """rows 0 and 1 share a parent over the first half of the history, the last row walks through the slots (a permuted row)"""
    src = torch.zeros(max_len, slots, dtype=torch.int32)
    for r in range(rows):
        src[:, r] = r
    if rows >= 2:
        src[: max_len // 2, 1] = 0
    if rows >= 3:
        src[:, rows - 1] = (torch.arange(max_len) + rows - 1) % rows
    return src


def _attn_ref(qkv, kc, vc, src, pos, rows, scale, heads=HEADS):
    """fp32 torch on the same 16-bit inputs: [rows, heads * D]"""
    HEADS, HD = heads, heads * D
    out = torch.zeros(rows, HD, dtype=torch.float64)
    qkv = qkv.double().cpu()
    kc, vc, src = kc.double().cpu(), vc.double().cpu(), src.cpu().long()
    for r in range(rows):
        q, k_own, v_own = qkv[r, :HD], qkv[r, HD:2 * HD], qkv[r, 2 * HD:3 * HD]
        K = torch.cat([kc[torch.arange(pos), src[:pos, r]], k_own[None]], 0).view(pos + 1, HEADS, D)
        V = torch.cat([vc[torch.arange(pos), src[:pos, r]], v_own[None]], 0).view(pos + 1, HEADS, D)
        s = torch.einsum("hd,jhd->hj", q.view(HEADS, D), K).float() * scale
        p = torch.softmax(s, dim=-1)
        out[r] = torch.einsum("hj,jhd->hd", p.double(), V).reshape(HD)
    return out


class _AttnRig:
    def __init__(self, lib, dtype, rows, slots, max_len, d=D, heads=HEADS, pad_qkv=0, pad_o=0):
        self.lib, self.dev, self.td = lib, _dev(lib), TD[dtype]
        self.rows, self.slots, self.max_len = rows, slots, max_len
        HD = self.hd = heads * D
        self.ld_qkv, self.ld_o = 3 * HD + pad_qkv, HD + pad_o          # row strides; the padding columns belong to the test
        pb = PlanBuilder(lib, self.dev, dtype)
        self.qkv = pb.buf((rows, self.ld_qkv), self.td, zero=True)
        self.kc = pb.buf((max_len, slots, HD), self.td)
        self.vc = pb.buf((max_len, slots, HD), self.td)
        self.pos = pb.buf((1,), torch.int32, zero=True)
        self.src = pb.buf((max_len, slots), torch.int32, zero=True)
        self.o = pb.buf((rows, self.ld_o), self.td, zero=True)
        self.scale = 0.125
        pb.decode_attention(self.qkv, self.kc, self.vc, self.pos, self.src, self.o, rows, slots, HD // d, d, max_len, self.scale,
                            ld_qkv=self.ld_qkv, ld_o=self.ld_o)
        self.pb = pb
        self.plan = None

    def run(self):
        if self.plan is None:
            self.plan = self.pb.build()
        self.plan.run()
        _sync(self.lib)


def check_decode_attn_exact(lib, dtype, n_keys, seed=0, rows=3, slots=4, heads=HEADS):
    """all keys equal, integer values: the mean over n_keys (a power of two) is exact; the kernel's bytes must equal its one rounding"""
    assert n_keys & (n_keys - 1) == 0 and 1 <= rows <= slots <= 8
    pos = n_keys - 1
    HD = heads * D
    g = torch.Generator().manual_seed(seed)
    rig = _AttnRig(lib, dtype, rows, slots, max_len=n_keys, heads=heads)
    td = rig.td
    k0 = torch.randint(-3, 4, (HD,), generator=g).double()
    q = torch.randint(-3, 4, (rows, HD), generator=g).double()
    v_own = torch.randint(-64, 65, (rows, HD), generator=g).double()
    vc = torch.randint(-64, 65, (n_keys, slots, HD), generator=g).double()
    src = torch.randint(0, rows, (n_keys, slots), generator=g, dtype=torch.int32)
    rig.qkv.copy_(torch.cat([q, k0.expand(rows, HD), v_own], 1).to(td))
    rig.kc.copy_(k0.expand(n_keys, slots, HD).to(td))
    rig.vc.copy_(vc.to(td))
    rig.src.copy_(src)
    rig.pos.fill_(pos)
    rig.run()
    ref = torch.zeros(rows, HD, dtype=torch.float64)
    for r in range(rows):
        ref[r] = (vc[torch.arange(pos), src[:pos, r].long()].sum(0) + v_own[r]) / n_keys
    assert float(ref.abs().max()) * n_keys < float(1 << 24)
    ref = ref.float().to(td).double()
    got = rig.o.double().cpu()
    bad = int((got != ref).sum())
    assert bad == 0, f"decode attention, {n_keys} equal keys, rows={rows} heads={heads}: {bad} of {ref.numel()} elements differ from the rounded exact mean"


def check_decode_attn_random(lib, dtype, rows, pos, seed=0, slots=4, heads=HEADS):
    """returns the largest error relative to its bound"""
    max_len = 304
    HD = heads * D
    g = torch.Generator().manual_seed(seed * 1000 + rows * 31 + pos)
    rig = _AttnRig(lib, dtype, rows, slots, max_len, heads=heads)
    td = rig.td
    kc = torch.randn(max_len, slots, HD, generator=g).to(td)
    vc = torch.randn(max_len, slots, HD, generator=g).to(td)
    for c in (kc, vc):
        cb = c.view(torch.int16)              # (shares the storage)
        cb[pos:] = NAN_BITS                   # nothing at or beyond pos may be read ...
        cb[:, rows:] = NAN_BITS               # ... and no slot that holds no row
    src = _src_table(max_len, slots, rows)
    if rows >= 3:
        assert len(set(src[:rows, rows - 1].tolist())) == rows, "the last row must walk through every slot that holds a row"
    qkv = (torch.randn(rows, 3 * HD, generator=g) * 1.5).to(td)
    rig.qkv.copy_(qkv); rig.kc.copy_(kc); rig.vc.copy_(vc); rig.src.copy_(src); rig.pos.fill_(pos)
    rig.run()

    def compare(qkv_now, kc_ref, vc_ref, src_now, pos_now):
        got = rig.o.double().cpu()
        assert bool(torch.isfinite(got).all()), f"decode attention R={rows} pos={pos_now}: non-finite output (a cache entry beyond pos or a free slot was read)"
        ref = _attn_ref(qkv_now, kc_ref, vc_ref, src_now, pos_now, rows, rig.scale, heads)
        vmax = float(qkv_now[:, 2 * HD:].double().abs().max().clamp_min(vc_ref[:pos_now, :rows].double().abs().max() if pos_now else 0.0))
        bound = ref.abs() * 2.0 ** -(MANT[dtype] + 1) * (1 + 2.0 ** -6) + 300 * 2.0 ** -23 * vmax
        ratio = float(((got - ref).abs() / bound).max())
        assert ratio <= 1.0, f"decode attention R={rows} heads={heads} pos={pos_now}: error {ratio:.2f} x the bound (one rounding + fp32 softmax)"
        return ratio

    worst = compare(qkv, kc, vc, src, pos)
    # only cache[pos][0..rows) has changed, and it holds the rows' k and v
    want_k, want_v = kc.clone(), vc.clone()
    want_k[pos, :rows] = qkv[:, HD:2 * HD]
    want_v[pos, :rows] = qkv[:, 2 * HD:]
    assert torch.equal(_bits(rig.kc.cpu()), _bits(want_k)) and torch.equal(_bits(rig.vc.cpu()), _bits(want_v)), \
        f"decode attention R={rows} pos={pos}: the caches changed elsewhere than at [pos][0..rows), or hold other values there"
    # a second launch of the SAME plan at pos + 1 reads what the first wrote, through a reordered table
    src2 = src.clone()
    src2[pos, :rows] = (torch.arange(rows, dtype=torch.int32) + 1) % rows
    qkv2 = (torch.randn(rows, 3 * HD, generator=g) * 1.5).to(td)
    rig.qkv.copy_(qkv2); rig.src.copy_(src2); rig.pos.fill_(pos + 1)
    rig.run()
    worst = max(worst, compare(qkv2, want_k, want_v, src2, pos + 1))
    return worst


def check_decode_attn_padded_strides(lib, dtype, rows=5, slots=8, heads=3, pos=33, seed=0):
    """ld_qkv = 3 HD + 16 and ld_o = HD + 8: the bytes of the unpadded case; NaN in the padding of qkv is not read, the padding of o keeps
    its sentinel"""
    max_len = pos + 3
    HD = heads * D
    g = torch.Generator().manual_seed(seed + rows)
    plain = _AttnRig(lib, dtype, rows, slots, max_len, heads=heads)
    wide = _AttnRig(lib, dtype, rows, slots, max_len, heads=heads, pad_qkv=16, pad_o=8)
    assert (wide.ld_qkv, wide.ld_o) == (3 * HD + 16, HD + 8)
    td = plain.td
    kc = torch.randn(max_len, slots, HD, generator=g).to(td)
    vc = torch.randn(max_len, slots, HD, generator=g).to(td)
    src = _src_table(max_len, slots, rows)
    qkv = (torch.randn(rows, 3 * HD, generator=g) * 1.5).to(td)
    padded = torch.full((rows, wide.ld_qkv), float("nan")).to(td)
    padded[:, :3 * HD] = qkv
    sentinel = torch.full((rows, wide.ld_o), 7.0).to(td)
    for rig, q, o0 in ((plain, qkv, torch.zeros(rows, HD).to(td)), (wide, padded, sentinel)):
        rig.qkv.copy_(q); rig.kc.copy_(kc); rig.vc.copy_(vc); rig.src.copy_(src); rig.pos.fill_(pos); rig.o.copy_(o0)
        rig.run()
    want, got = plain.o.cpu(), wide.o.cpu()
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0
    what = f"decode attention with padded strides R={rows} heads={heads}"
    assert torch.equal(got[:, :HD].contiguous().view(torch.uint8), want.view(torch.uint8)), f"{what}: differs from the unpadded case"
    assert torch.equal(got[:, HD:].contiguous().view(torch.uint8), sentinel[:, HD:].contiguous().view(torch.uint8)), f"{what}: the padding of o was written"
    assert torch.equal(wide.kc.cpu().view(torch.uint8), plain.kc.cpu().view(torch.uint8)) and torch.equal(wide.vc.cpu().view(torch.uint8), plain.vc.cpu().view(torch.uint8))


def check_decode_attn_refuses_d32(lib):
    rig = _AttnRig(lib, abi.BF16, 1, 4, 8, d=32)
    args = rig.pb.ops[-1].u.dattn
    rc = lib.mtx_decode_attention(C.byref(args), C.c_void_p(0))
    assert rc != 0 and "64" in lib.last_error()
    with pytest.raises(ModelError):
        lib.check(rc, "mtx_decode_attention")
    with pytest.raises(ModelError):
        rig.run()


# ---- skinny-row linear ---------------------------------------------------------------------------------------------------------------------
def _rowlin_pair(lib, dtype, a, w, bias, res, act, alpha, out_f32):
    """(row_linear output, gemm output) on the same operands"""
    dev, td = _dev(lib), TD[dtype]
    rows, k = a.shape
    n = w.shape[0]
    pb = PlanBuilder(lib, dev, dtype)
    at, wt = pb.const(a.to(td)), pb.const(w.to(td))
    bt = pb.const(bias.float()) if bias is not None else None
    rt = pb.const(res.to(td)) if res is not None else None
    y1 = pb.row_linear(at, wt, rows, n, k, bias=bt, act=act, res=rt, alpha=alpha, out_f32=out_f32)
    y2 = pb.gemm(at, wt, rows, n, k, bias=bt, act=act, res=rt, alpha=alpha, out_f32=out_f32)
    _run(pb)
    return y1.cpu(), y2.cpu()


def check_rowlin_exact(lib, dtype, rows, n, k, out_f32, seed=0):
    """small-integer operands, bias, erf-GELU and a residual: bit-identical to mtx_gemm"""
    g = torch.Generator().manual_seed(seed + rows * 7 + n)
    a = torch.randint(-2, 3, (rows, k), generator=g).double()
    w = torch.randint(-2, 3, (n, k), generator=g).double()
    bias = torch.randint(-8, 9, (n,), generator=g).double()
    res = torch.randint(-64, 65, (rows, n), generator=g).double()
    alpha = 0.125
    assert k * 4 + 8 < (1 << 24)
    y1, y2 = _rowlin_pair(lib, dtype, a, w, bias, res, abi.ACT_GELU, alpha, out_f32)
    assert y1.dtype == (torch.float32 if out_f32 else TD[dtype])
    v = (a @ w.t()) * alpha + bias
    want = 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))
    assert float(want.abs().max()) > 4.0                                  # the activation really sees values away from zero
    same = torch.equal(y1.view(torch.int32 if out_f32 else torch.int16), y2.view(torch.int32 if out_f32 else torch.int16))
    assert same, (f"row linear {rows}x{n}x{k} ({'fp32' if out_f32 else '16-bit'} out): {int((y1 != y2).sum())} elements differ from mtx_gemm; "
                  f"max |diff| {float((y1.double() - y2.double()).abs().max())}")
    # and mtx_gemm is not the only witness: the float64 value, within one (two) roundings
    want = want + res
    tol = (2.0 ** -MANT[dtype] * (want.abs() + res.abs() + 1) if not out_f32 else 1e-5 * (want.abs() + 1))
    assert bool(((y1.double() - want).abs() <= tol).all())


def check_rowlin_random(lib, dtype, rows, n, k, out_f32, seed=0):
    """random operands: the skinny kernel and mtx_gemm both within the bound of their contract against float64; returns the worst ratio"""
    td = TD[dtype]
    g = torch.Generator().manual_seed(seed + rows * 7 + n)
    a = torch.randn(rows, k, generator=g).to(td).double()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(td).double()
    bias = torch.randn(n, generator=g).float().double()
    res = torch.randn(rows, n, generator=g).to(td).double()
    y1, y2 = _rowlin_pair(lib, dtype, a, w, bias, res, abi.ACT_GELU, 1.0, out_f32)
    v = a @ w.t() + bias
    t = 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))
    ref = t + res
    acc_err = k * 2.0 ** -23 * (a.abs() @ w.abs().t()) + 2.0 ** -22 * (v.abs() + 1)          # fp32 sums in any order, the fp32 epilogue (GELU's slope is below 1.13)
    half = 2.0 ** -(MANT[dtype] + 1) * (1 + 2.0 ** -6)
    bound = 1.13 * acc_err + (0.0 if out_f32 else half * (t.abs() + ref.abs()))                # two roundings: of t, of t + res
    worst = 0.0
    for name, y in (("row linear", y1), ("gemm", y2)):
        ratio = float(((y.double() - ref).abs() / bound).max())
        assert ratio <= 1.0, f"{name} {rows}x{n}x{k}: error {ratio:.2f} x the contract's bound against float64"
        worst = max(worst, ratio)
    return worst


def rowlin_tiling(rows, n, wide):
    """rowlin_launch's / rowlin_wide_launch's rule restated: (RT, NW) of rowlin_kernel<T, RT, NW> / rowlin_wide_kernel<T, RT, NW>"""
    nw = 4 if n >= 4096 else (2 if n >= 2048 else 1)
    if wide:
        assert 1 <= rows <= 32
        return (8 if rows <= 8 else (16 if rows <= 16 else 32)), nw
    assert 1 <= rows <= 8
    return (1 if rows == 1 else (4 if rows <= 4 else 8)), nw


C_SENTINEL, RES_PAD = -77.0, 999.0
_CONTRACT_OPERANDS = {}


def _contract_operands(dtype, n, k):
    """integer operands for 17 rows and their float64 product, built once per (dtype, n, k) and shared, never modified: a case reads its
    leading rows"""
    import exact_checks as ec
    key = (dtype, n, k)
    if key not in _CONTRACT_OPERANDS:
        g = torch.Generator().manual_seed(n * 7 + k)
        rng = abi.F16 if dtype == abi.F32 else dtype               # fp32 storage rounds nowhere: the f16 operand range serves
        r, alpha = ec.operand_range(rng, k, spread=1.5)             # (RELU zeroes half of the outputs: the spread keeps precondition (c))
        a, w = ec._ints(g, (17, k), r), ec._ints(g, (n, k), r)
        bias, res = ec._ints(g, (n,), ec.INT_CAP[rng]), ec._ints(g, (17, n), ec.INT_CAP[rng])
        assert k * r * r * alpha + ec.INT_CAP[rng] < ec.EXACT, "precondition (a): partial sums are not exact in fp32"
        _CONTRACT_OPERANDS[key] = (a, w, bias, res, alpha, a @ w.t())
    return _CONTRACT_OPERANDS[key]


def check_rowlin_contract_exact(lib, dtype, rows, n, k, wide, out_f32, expect):
    """the skinny linears against float64 with the contract's rounding points, not against mtx_gemm or each other: integer operands, a
    power-of-two alpha, an integer bias and residual, RELU;  t = round_T(act(alpha acc + bias)), c = round_T(t + res);  an fp32 output and
    fp32 storage round nowhere.  Zero differing elements; the output lies in a sentinel-filled buffer (ldc = n + 5, a spare row) and the
    residual has ldres = n + 3.  `expect` = the (RT, NW) instantiation the case is meant for.  Returns the rounding share (None: no rounding)"""
    import exact_checks as ec
    assert rowlin_tiling(rows, n, wide) == expect, f"rows={rows} n={n} runs {rowlin_tiling(rows, n, wide)}, the case is meant for {expect}"
    assert k % 8 == 0
    dev, td = _dev(lib), TD[dtype]
    out_f32 = out_f32 or dtype == abi.F32
    a, w, bias, res, alpha, acc = _contract_operands(dtype, n, k)
    a, res, acc = a[:rows], res[:rows], acc[:rows]
    t = (acc * alpha + bias).clamp_min(0.0)
    what = f"{'wide ' if wide else ''}row linear {rows}x{n}x{k} (RT, NW) = {expect}, {'fp32' if out_f32 else '16-bit'} out"
    share = None
    if out_f32:
        ref = t + res
        assert float(ref.abs().max()) < ec.EXACT
    else:
        ref = ec._round(ec._round(t, td) + res, td)
        share = ec._assert_rounding_share(ref, dtype, what)
    assert float((t > 0).double().mean()) > 0.3 and float((t == 0).double().mean()) > 0.3, "RELU must see both signs"
    pb = PlanBuilder(lib, dev, dtype)
    otd = torch.float32 if out_f32 else td
    out = pb.const(torch.full((rows + 1, n + 5), C_SENTINEL).to(otd))
    res_t = torch.full((rows, n + 3), RES_PAD, dtype=torch.float64)
    res_t[:, :n] = res
    op = pb.row_linear_wide if wide else pb.row_linear
    op(pb.const(a.to(td)), pb.const(w.to(td)), rows, n, k, out=out, ldc=n + 5, bias=pb.const(bias.float()), act=abi.ACT_RELU, res=pb.const(res_t.to(td)),
       ldres=n + 3, alpha=alpha, out_f32=out_f32)
    _run(pb)
    got = out.cpu().double()
    ec._assert_equal(got[:rows, :n], ref, what)
    got[:rows, :n] = C_SENTINEL
    assert bool((got == C_SENTINEL).all()), f"{what}: the buffer changed outside the result"
    return share


# ---- the model against the transformers oracle -----------------------------------------------------------------------------------------------------
# Tiny configuration used throughout: ViT hidden 128 / 2 layers / 2 heads / MLP 512 / 64 px / patch 16 (17 tokens); BERT decoder hidden 128 /
# 2 layers / 2 heads / MLP 512 / vocabulary 512 / 64 positions; initializer_range 0.3; torch.manual_seed(seed) before construction; the image from
# torch.Generator().manual_seed(100 + seed).  The oracle is the HF model in fp32 on the CPU.
import functools

from mangatranslator_amd.core.ml import manga_ocr as mo

START, EOS, PAD = 2, 3, 0
TINY = dict(e=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, image_size=64, patch_size=16),
            d=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=512, max_position_embeddings=64))
REAL = dict(e=dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, image_size=224, patch_size=16),
            d=dict(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072, vocab_size=6144, max_position_embeddings=512))
GEN = dict(num_beams=4, no_repeat_ngram_size=3, length_penalty=2.0, early_stopping=True, max_length=24)


@functools.lru_cache(maxsize=12)
def oracle(seed, real=False):
    """(HF model, pixel values [1, 3, S, S]) — built once per seed and shared, never modified"""
    from transformers import BertConfig, VisionEncoderDecoderConfig, VisionEncoderDecoderModel, ViTConfig
    dims = REAL if real else TINY
    rng = 0.02 if real else 0.3
    enc = ViTConfig(initializer_range=rng, **dims["e"])
    dec = BertConfig(is_decoder=True, add_cross_attention=True, initializer_range=rng, **dims["d"])
    cfg = VisionEncoderDecoderConfig.from_encoder_decoder_configs(enc, dec)
    cfg.decoder_start_token_id, cfg.pad_token_id, cfg.eos_token_id = START, PAD, EOS
    torch.manual_seed(seed)
    model = VisionEncoderDecoderModel(cfg).eval()
    S = dims["e"]["image_size"]
    pixels = torch.randn(1, 3, S, S, generator=torch.Generator().manual_seed(100 + seed))
    return model, pixels


def config_dict(model, gen=None):
    c = model.config.to_dict()
    c.update(gen or {})
    return c


def hip_model(lib, model, dtype, rows, gen=None, **kw):
    hp = mo.hparams_from_config(config_dict(model, gen))
    sd = mo.normalise_state_dict({k: v for k, v in model.state_dict().items()}, hp)
    return mo.MangaOcrHip(sd, hp, [f"t{i}" for i in range(hp["vocab"])], device=_dev(lib), lib=lib, dtype=dtype, rows=rows, **kw)


@torch.no_grad()
def oracle_logp(model, pixels, seqs):
    """log-probs [rows, len, vocab] of the HF model for the token rows `seqs` in one fp32 pass"""
    ids = torch.tensor(seqs, dtype=torch.long)
    out = model(pixel_values=pixels.expand(ids.shape[0], -1, -1, -1), decoder_input_ids=ids)
    return torch.log_softmax(out.logits.float(), dim=-1)


def fixed_prefix(n, vocab):
    return [START] + [(37 * i * i + 11 * i + 5) % (vocab - 4) + 4 for i in range(1, n)]


def _err(got, ref):
    d = (got.double() - ref.double()).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def check_teacher_forced(lib, dtype, seed, n=20, real=False, compare=None):
    """a fixed prefix pushed through the step graph one token at a time with R = 1; log_softmax at every position against the oracle's one pass.
    -> (max, rms) absolute log-prob error"""
    model, pixels = oracle(seed, real)
    vocab = model.config.decoder.vocab_size
    prefix = fixed_prefix(n, vocab)
    ref = oracle_logp(model, pixels, [prefix])[0]
    hip = hip_model(lib, model, dtype, rows=1, gen=dict(max_length=n + 1))
    try:
        hip.encode_pixels(pixels[0])
        got = torch.stack([hip.step(mo.BeamStep(i, [prefix[i]], [0]))[0] for i in range(n)])
    finally:
        hip.close()
    assert bool(torch.isfinite(got).all())
    keep = list(range(n)) if compare is None else compare
    return _err(got[keep], ref[keep])


def check_lockstep_beams(lib, dtype, seed):
    """`beam_search` driven by the ORACLE's log-probs (R = 4); the device step is fed the same tokens, position and ancestry at every step and its
    log-probs for all four rows are compared at every step -> (max, rms, number of steps at which the beams were reordered)"""
    model, pixels = oracle(seed)
    gen = dict(GEN)
    hip = hip_model(lib, model, dtype, rows=4, gen=gen)
    errs, reorders = [], 0
    try:
        hip.encode_pixels(pixels[0])

        def step_fn(st):
            nonlocal reorders
            ref = oracle_logp(model, pixels, st.sequences)[:, -1]
            got = hip.step(st)
            errs.append((got.double() - ref.double()).abs())
            reorders += int(st.parents != list(range(4)))
            return ref
        mo.beam_search(step_fn, hip.gen)
    finally:
        hip.close()
    d = torch.stack(errs)
    return float(d.max()), float(d.pow(2).mean().sqrt()), reorders


def decided_prefix(seed, delta, n=20):
    """(oracle greedy tokens, number of leading steps whose top-1 / top-2 log-prob gap stays >= delta) — from the oracle alone"""
    model, pixels = oracle(seed)
    seq, decided, open_ = [START], 0, True
    for _ in range(n):
        lp = oracle_logp(model, pixels, [seq])[0, -1]
        top = torch.topk(lp, 2)
        if open_ and float(top.values[0] - top.values[1]) >= delta:
            decided += 1
        else:
            open_ = False
        seq.append(int(top.indices[0]))
    return seq, decided


def check_greedy_tokens(lib, dtype, seed, delta, n=20):
    """the device's own greedy tokens equal the oracle's over the decided prefix -> its length"""
    model, pixels = oracle(seed)
    want, decided = decided_prefix(seed, delta, n)
    hip = hip_model(lib, model, dtype, rows=1, gen=dict(max_length=n + 1))
    try:
        hip.encode_pixels(pixels[0])
        seq = [START]
        for i in range(decided):
            seq.append(int(torch.argmax(hip.step(mo.BeamStep(i, [seq[-1]], [0]))[0])))
    finally:
        hip.close()
    assert seq == want[:decided + 1], f"seed {seed}: greedy tokens {seq} != oracle {want[:decided + 1]} over the decided prefix ({decided} steps, delta {delta})"
    return decided


def stage_directory(root, seed=0, gen=None, historical=False):
    """a synthetic staged `manga-ocr-base`: config.json, model.safetensors, vocab.txt, preprocessor_config.json"""
    import json
    from safetensors.torch import save_file
    model, _ = oracle(seed)
    root.mkdir(parents=True, exist_ok=True)
    cfg = config_dict(model, gen if gen is not None else dict(GEN, max_length=12))
    (root / "config.json").write_text(json.dumps(cfg, default=str))
    sd = {k: v.clone().contiguous() for k, v in model.state_dict().items()}
    if historical:
        back = {"attention.q_proj": "attention.attention.query", "attention.k_proj": "attention.attention.key", "attention.v_proj": "attention.attention.value",
                "attention.o_proj": "attention.output.dense", "mlp.fc1": "intermediate.dense", "mlp.fc2": "output.dense"}
        ren = {}
        for k, v in sd.items():
            if k.startswith("encoder.layers."):
                _, _, n, rest = k.split(".", 3)
                for new, old in back.items():
                    if rest.startswith(new + "."):
                        rest = old + rest[len(new):]
                        break
                k = f"encoder.encoder.layer.{n}.{rest}"
            ren[k] = v
        sd = ren
        sd["decoder.bert.embeddings.position_ids"] = torch.arange(64).view(1, -1)
    save_file(sd, str(root / "model.safetensors"))
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [chr(0x3042 + i) for i in range(80)] + [str(i % 10) for i in range(427)]
    (root / "vocab.txt").write_text("\n".join(vocab[:512]) + "\n", encoding="utf-8")
    (root / "preprocessor_config.json").write_text(json.dumps({"image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5], "size": 64}))
    return root

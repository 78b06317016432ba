"""FLUX's prompt encoders as libmtx_hip plans: Qwen3 (FLUX.2-Klein), T5-XXL and CLIP-L (FLUX.1-Kontext).

The reference keeps these three networks in `transformers` and runs them on first use (core/image/inpainting.py:846-873 Kontext, :1110-1124
Klein).  Here they are restated on the kernels the other graphs use, around ONE attention (include/mtx_hip.h, MTX_OP_REL_ATTN):

    o[i, h] = sum_j softmax_j( scale * q[i, h] . k[j, g] + rel[h][j - i + S - 1] ) v[j, g]     over j < min(S, n_keys)

    encoder   rel                                                          n_keys                   scale
    Qwen3     causal table (0 for j <= i, masked above)                    the prompt's real tokens d^-0.5
    T5        bucketed bias of block 0, shared by all blocks               S (diffusers: no mask)   1
    CLIP      causal table                                                 S                        d^-0.5

Storage is bf16 (the reference's GPU dtype; T5 overflows f16 and refuses it), the residual stream fp32 (`vit_common.trunk_helpers(...,
stream32=True)`, as PaddleOCR-VL's decoder).  Plans are eager and built once per sequence length; the embedding rows are gathered on the host,
so a vocabulary table never goes to the device.  `close()` frees the weights and the plans.

Two rewrites keep the device code as it is:
  quick_gelu(h) = h * sigmoid(1.702 h)  ->  fc1 packed as 1.702 W, 1.702 b with MTX_ACT_SILU, fc2's weight as W / 1.702 (the same function)
  gated GELU                            ->  MTX_EW_ACT (tanh GELU) on the wi_0 half of the fused wi_0 | wi_1 output, MTX_EW_MUL with the other
"""
import math
from typing import Dict, Sequence

import torch

from ...hip import abi
from ...hip.lib import get_library
from ...hip.plan import Act, PlanBuilder
from ...utils.exceptions import ModelError
from . import packing, vit_common
from .paddle_ocr_vl import interleave_rows

QUICK_GELU = 1.702
_TDT = {abi.BF16: torch.bfloat16, abi.F16: torch.float16}


def _get(config, name, default=None):
    """a field of a `transformers` config object or of its dict"""
    if isinstance(config, dict):
        return config.get(name, default)
    return getattr(config, name, default)


def causal_table(heads: int, s: int) -> torch.Tensor:
    """fp32 [heads, 2 s - 1]: entry j - i + s - 1 is 0 for j <= i and masked above"""
    t = torch.full((heads, 2 * s - 1), abi.REL_MASKED, dtype=torch.float32)
    t[:, :s] = 0.0
    return t


def t5_relative_buckets(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """bucket of the offsets rel = j - i, bidirectional, as transformers' T5Attention._relative_position_bucket: half the buckets per sign, the
    first half of those one offset each, the rest log-spaced up to max_distance and clamped to the last bucket"""
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    n = rel.abs()
    exact = nb // 2
    large = exact + (torch.log(n.float().clamp_min(1.0) / exact) / math.log(max_distance / exact) * (nb - exact)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return out + torch.where(n < exact, n, large)


def t5_relative_table(weight: torch.Tensor, s: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """relative_attention_bias.weight [num_buckets, heads] -> fp32 [heads, 2 s - 1], entry j - i + s - 1"""
    rel = torch.arange(2 * s - 1) - (s - 1)
    return weight.float()[t5_relative_buckets(rel, num_buckets, max_distance)].t().contiguous()


def rope_table(s: int, theta: float, d: int) -> torch.Tensor:
    """fp32 [s][2][d / 2] cos | sin of the positions 0 .. s - 1"""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    ang = torch.arange(s, dtype=torch.float)[:, None] * inv
    return torch.stack([ang.cos(), ang.sin()], 1).contiguous()


class _Encoder:
    """what the three share: the library, the device, the storage type, the plans per sequence length"""
    WHAT = "text encoder"

    def __init__(self, device, lib, dtype):
        if dtype not in _TDT:
            raise ModelError(f"{self.WHAT}: storage dtype must be bf16 or f16")
        self.lib = lib if lib is not None else get_library()
        self.device, self.dtype, self.tdt = torch.device(device), dtype, _TDT[dtype]
        self._plans: Dict[int, object] = {}

    def _c(self, t, dtype=None):
        return packing.on_device(t, self.device, dtype if dtype is not None else self.tdt)

    def _lin(self, *ws, bias=None, scale=1.0):
        """(W, None, bias) of a linear whose matrices are stacked along N; `scale` multiplies W and the bias in fp32, before the one rounding"""
        w = torch.cat([w.float() for w in ws], 0) * scale if scale != 1.0 else torch.cat([w.float() for w in ws], 0)
        b = None if bias is None else self._c(torch.cat([x.float() for x in bias], 0) * scale, torch.float32)
        return (self._c(w), None, b)

    def _plan(self, s: int):
        if self.W is None:
            raise ModelError(f"{self.WHAT}: closed")
        if not 1 <= s <= abi.REL_ATTN_SMAX:
            raise ModelError(f"{self.WHAT}: a sequence of {s} tokens is not served (1 .. {abi.REL_ATTN_SMAX})")
        if s not in self._plans:
            self._plans[s] = self._build(s)
        return self._plans[s]

    def _run(self, plan):
        plan.run()
        if not self.lib.is_simulator:
            torch.cuda.synchronize(self.device)

    def _ids(self, ids, vocab):
        ids = torch.as_tensor(ids, dtype=torch.long).reshape(-1).cpu()
        if ids.numel() < 1 or int(ids.min()) < 0 or int(ids.max()) >= vocab:
            raise ModelError(f"{self.WHAT}: token ids must lie in 0 .. {vocab - 1}")
        return ids

    def close(self):
        for p in self._plans.values():
            p.close()
        self._plans, self.W = {}, None


class Qwen3EncoderHip(_Encoder):
    """the first max(taps) decoder layers of Qwen3ForCausalLM; `encode_ids` returns the streams after the layers `taps` side by side"""
    WHAT = "Qwen3 prompt encoder"

    def __init__(self, state_dict: dict, config, taps: Sequence[int] = (9, 18, 27), device="cuda", lib=None, dtype: int = abi.BF16):
        super().__init__(device, lib, dtype)
        self.C, self.heads = int(_get(config, "hidden_size")), int(_get(config, "num_attention_heads"))
        self.kv = int(_get(config, "num_key_value_heads", self.heads))
        self.d = int(_get(config, "head_dim") or self.C // self.heads)
        self.I, self.eps = int(_get(config, "intermediate_size")), float(_get(config, "rms_norm_eps", 1e-6))
        rp = _get(config, "rope_parameters") or {}
        self.theta = float(_get(config, "rope_theta") or rp.get("rope_theta", 10000.0))
        self.taps = tuple(int(t) for t in taps)
        n_layers = int(_get(config, "num_hidden_layers"))
        if self.d != 128:
            raise ModelError(f"{self.WHAT}: head_dim {self.d} is not served (128)")
        if self.heads % self.kv:
            raise ModelError(f"{self.WHAT}: {self.heads} heads over {self.kv} kv heads")
        if not self.taps or list(self.taps) != sorted(set(self.taps)) or self.taps[0] < 1 or self.taps[-1] >= n_layers:
            raise ModelError(f"{self.WHAT}: taps {self.taps} must be increasing layer counts below the last layer ({n_layers}): hidden_states[k] is "
                             f"the un-normed stream after k layers only there")
        sd, M = state_dict, "model."
        self.embed = sd[M + "embed_tokens.weight"].detach().cpu()          # host: only the prompt's rows are gathered
        if self.embed.shape[1] != self.C:
            raise ModelError(f"{self.WHAT}: the embedding table does not match hidden_size")
        f32 = torch.float32
        self.W = []
        for i in range(self.taps[-1]):                                     # only the layers a tap needs
            p = f"{M}layers.{i}."
            a = p + "self_attn."
            g = lambda k: sd[k].detach().float()          # (where the checkpoint lives: a tensor already on the device is packed there)
            self.W.append(dict(
                n1=self._c(g(p + "input_layernorm.weight"), f32), n2=self._c(g(p + "post_attention_layernorm.weight"), f32),
                # the rotary kernel turns interleaved pairs, the wheel the halves: the projection rows AND the per-head gains are permuted alike
                qkv=self._lin(interleave_rows(g(a + "q_proj.weight"), self.heads, self.d), interleave_rows(g(a + "k_proj.weight"), self.kv, self.d),
                              g(a + "v_proj.weight")),
                qk_gain=self._c(torch.cat([interleave_rows(g(a + "q_norm.weight"), 1, self.d), interleave_rows(g(a + "k_norm.weight"), 1, self.d)]), f32),
                o=self._lin(g(a + "o_proj.weight")), gu=self._lin(g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")),
                down=self._lin(g(p + "mlp.down_proj.weight"))))

    def _build(self, S: int):
        C, heads, kv, d, I = self.C, self.heads, self.kv, self.d, self.I
        qw = (heads + 2 * kv) * d
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        f32 = torch.float32
        xa, xb = pb.buf((S, C), f32, zero=True), pb.buf((S, C), f32)
        n_keys = pb.buf((1,), torch.int32, zero=True)
        rope, table = pb.const(rope_table(S, self.theta, d)), pb.const(causal_table(heads, S))
        _, linear, close = vit_common.trunk_helpers(pb, self.eps, self.tdt, self.dtype, stream32=True)
        a16, b16 = pb.buf((S, C), self.tdt), pb.buf((S, C), self.tdt)
        qkv, o = pb.buf((S, qw), self.tdt), pb.buf((S, heads * d), self.tdt)
        gu, mid = pb.buf((S, 2 * I), self.tdt), pb.buf((1, 1, S, I), self.tdt)
        outs = []
        for i, L in enumerate(self.W):
            tag = f"qwen{i}"
            pb.norm(xa, a16, S, C, gamma=L["n1"], eps=self.eps, kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm1")
            linear(a16, L["qkv"], S, qw, C, tag + ".qkv", out=qkv)
            pb.qk_norm_rope(Act(qkv.view(1, 1, S, qw), 1, 1, S, (heads + kv) * d), rope, 0, L["qk_gain"], d, heads, eps=self.eps, label=tag + ".qk_norm_rope")
            pb.rel_attention(qkv, qkv, qkv, o, S, heads, kv, d, (qw, d), (qw, d), (qw, d), (heads * d, d), d ** -0.5, rel=table, n_keys=n_keys,
                             k_off=heads * d, v_off=(heads + kv) * d, label=tag + ".attn")
            close(o, L["o"], S, C, heads * d, xa, tag + ".o_proj", out=xb)
            pb.norm(xb, b16, S, C, gamma=L["n2"], eps=self.eps, kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm2")
            linear(b16, L["gu"], S, 2 * I, C, tag + ".gate_up", out=gu)
            g4 = gu.view(1, 1, S, 2 * I)
            pb.ew(abi.EW_SWIGLU, Act(g4, 1, 1, S, I, 0), b=Act(g4, 1, 1, S, I, I), out=Act(mid, 1, 1, S, I), label=tag + ".swiglu")
            close(mid.view(S, I), L["down"], S, C, I, xb, tag + ".down", out=xa)
            if i + 1 in self.taps:
                outs.append(pb.cvt16(xa, pb.buf((S, C), self.tdt), S, C, label=f"tap{i + 1}"))
        plan = pb.build()
        plan.x0, plan.n_keys, plan.outs = xa, n_keys, outs
        return plan

    def encode_ids(self, ids, n_valid: int) -> torch.Tensor:
        """ids [S] (right-padded), n_valid = the number of real tokens -> [S, len(taps) * hidden] of the storage type, tap-major on the feature
        axis (prompt_embeds.export_klein's layout)"""
        ids = self._ids(ids, self.embed.shape[0])
        S = int(ids.numel())
        if not 1 <= int(n_valid) <= S:
            raise ModelError(f"{self.WHAT}: n_valid must be 1 .. {S}")
        plan = self._plan(S)
        plan.x0.copy_(self.embed[ids].float())
        plan.n_keys.fill_(int(n_valid))
        self._run(plan)
        return torch.cat(plan.outs, 1)


class T5EncoderHip(_Encoder):
    """T5EncoderModel with gated-GELU feed-forwards (T5 v1.1 / XXL)"""
    WHAT = "T5 prompt encoder"

    def __init__(self, state_dict: dict, config, device="cuda", lib=None, dtype: int = abi.BF16):
        if dtype == abi.F16:
            raise ModelError(f"{self.WHAT}: f16 storage is refused (T5's activations overflow it); use bf16")
        super().__init__(device, lib, dtype)
        self.C, self.heads, self.d = int(_get(config, "d_model")), int(_get(config, "num_heads")), int(_get(config, "d_kv"))
        self.F, self.eps = int(_get(config, "d_ff")), float(_get(config, "layer_norm_epsilon", 1e-6))
        self.buckets, self.max_distance = int(_get(config, "relative_attention_num_buckets", 32)), int(_get(config, "relative_attention_max_distance", 128))
        n_layers = int(_get(config, "num_layers"))
        ff = str(_get(config, "feed_forward_proj", "gated-gelu"))
        if ff != "gated-gelu":
            raise ModelError(f"{self.WHAT}: feed_forward_proj {ff!r} is not served (gated-gelu)")
        if self.d != 64:
            raise ModelError(f"{self.WHAT}: d_kv {self.d} is not served (64)")
        sd = state_dict
        g = lambda k: sd[k].detach().float()          # (where the checkpoint lives: a tensor already on the device is packed there)
        self.embed = (sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"]).detach().cpu()
        self.bias = g("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").cpu()          # [buckets, heads], host: a table per S
        if tuple(self.bias.shape) != (self.buckets, self.heads):
            raise ModelError(f"{self.WHAT}: the relative attention bias is not [{self.buckets}, {self.heads}]")
        f32 = torch.float32
        layers = []
        for i in range(n_layers):
            p = f"encoder.block.{i}.layer."
            a, m = p + "0.SelfAttention.", p + "1.DenseReluDense."
            layers.append(dict(n1=self._c(g(p + "0.layer_norm.weight"), f32), n2=self._c(g(p + "1.layer_norm.weight"), f32),
                               qkv=self._lin(g(a + "q.weight"), g(a + "k.weight"), g(a + "v.weight")), o=self._lin(g(a + "o.weight")),
                               wi=self._lin(g(m + "wi_0.weight"), g(m + "wi_1.weight")), wo=self._lin(g(m + "wo.weight"))))
        self.W = dict(layers=layers, final=self._c(g("encoder.final_layer_norm.weight"), f32))

    def _build(self, S: int):
        C, heads, d, F = self.C, self.heads, self.d, self.F
        inner = heads * d
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        f32 = torch.float32
        xa, xb = pb.buf((S, C), f32, zero=True), pb.buf((S, C), f32)
        table = pb.const(t5_relative_table(self.bias, S, self.buckets, self.max_distance))
        _, linear, close = vit_common.trunk_helpers(pb, self.eps, self.tdt, self.dtype, stream32=True)
        a16, b16 = pb.buf((S, C), self.tdt), pb.buf((S, C), self.tdt)
        qkv, o = pb.buf((S, 3 * inner), self.tdt), pb.buf((S, inner), self.tdt)
        wi, mid = pb.buf((S, 2 * F), self.tdt), pb.buf((1, 1, S, F), self.tdt)
        st = (3 * inner, d)
        for i, L in enumerate(self.W["layers"]):
            tag = f"t5.{i}"
            pb.norm(xa, a16, S, C, gamma=L["n1"], eps=self.eps, kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm1")
            linear(a16, L["qkv"], S, 3 * inner, C, tag + ".qkv", out=qkv)
            pb.rel_attention(qkv, qkv, qkv, o, S, heads, heads, d, st, st, st, (inner, d), 1.0, rel=table, k_off=inner, v_off=2 * inner, label=tag + ".attn")
            close(o, L["o"], S, C, inner, xa, tag + ".o", out=xb)
            pb.norm(xb, b16, S, C, gamma=L["n2"], eps=self.eps, kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm2")
            linear(b16, L["wi"], S, 2 * F, C, tag + ".wi", out=wi)
            w4 = wi.view(1, 1, S, 2 * F)
            gate = Act(w4, 1, 1, S, F, 0)
            pb.ew(abi.EW_ACT, gate, out=gate, act=abi.ACT_GELU_TANH, label=tag + ".gelu")
            pb.ew(abi.EW_MUL, gate, b=Act(w4, 1, 1, S, F, F), out=Act(mid, 1, 1, S, F), label=tag + ".gate")
            close(mid.view(S, F), L["wo"], S, C, F, xb, tag + ".wo", out=xa)
        out = pb.norm(xa, pb.buf((S, C), self.tdt), S, C, gamma=self.W["final"], eps=self.eps, kind=1, dtype=abi.F32, out_dtype=self.dtype, label="t5.final_norm")
        plan = pb.build()
        plan.x0, plan.out = xa, out
        return plan

    def encode_ids(self, ids) -> torch.Tensor:
        """ids [S] (diffusers pads to 512 and passes no mask: every position is a key) -> [S, d_model] of the storage type"""
        ids = self._ids(ids, self.embed.shape[0])
        plan = self._plan(int(ids.numel()))
        plan.x0.copy_(self.embed[ids].float())
        self._run(plan)
        return plan.out.clone()


class ClipTextHip(_Encoder):
    """CLIPTextModel; `pooled` returns pooler_output, the final-LayerNorm row of the end-of-text token"""
    WHAT = "CLIP prompt encoder"

    def __init__(self, state_dict: dict, config, device="cuda", lib=None, dtype: int = abi.BF16):
        super().__init__(device, lib, dtype)
        self.C, self.heads = int(_get(config, "hidden_size")), int(_get(config, "num_attention_heads"))
        self.F, self.eps = int(_get(config, "intermediate_size")), float(_get(config, "layer_norm_eps", 1e-5))
        self.eos = int(_get(config, "eos_token_id", 2))
        self.d = self.C // self.heads
        act = str(_get(config, "hidden_act", "quick_gelu"))
        if act not in ("quick_gelu", "gelu"):
            raise ModelError(f"{self.WHAT}: hidden_act {act!r} is not served (quick_gelu, gelu)")
        if self.d != 64:
            raise ModelError(f"{self.WHAT}: head width {self.d} is not served (64)")
        quick = act == "quick_gelu"
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}
        g = lambda k: sd[k].detach().float()          # (where the checkpoint lives: a tensor already on the device is packed there)
        self.embed, self.pos = sd["embeddings.token_embedding.weight"].detach().cpu(), g("embeddings.position_embedding.weight").cpu()
        layers = []
        for i in range(int(_get(config, "num_hidden_layers"))):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            k1 = QUICK_GELU if quick else 1.0
            layers.append(dict(
                ln1=(self._c(g(p + "layer_norm1.weight"), torch.float32), self._c(g(p + "layer_norm1.bias"), torch.float32)),
                ln2=(self._c(g(p + "layer_norm2.weight"), torch.float32), self._c(g(p + "layer_norm2.bias"), torch.float32)),
                qkv=self._lin(g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight"),
                              bias=(g(a + "q_proj.bias"), g(a + "k_proj.bias"), g(a + "v_proj.bias"))),
                o=self._lin(g(a + "out_proj.weight"), bias=(g(a + "out_proj.bias"),)),
                fc1=self._lin(g(p + "mlp.fc1.weight"), bias=(g(p + "mlp.fc1.bias"),), scale=k1),
                fc2=(self._c(g(p + "mlp.fc2.weight") / k1), None, self._c(g(p + "mlp.fc2.bias"), torch.float32))))
        self.act = abi.ACT_SILU if quick else abi.ACT_GELU
        self.W = dict(layers=layers, final=(self._c(g("final_layer_norm.weight"), torch.float32), self._c(g("final_layer_norm.bias"), torch.float32)))

    def _build(self, S: int):
        C, heads, d, F = self.C, self.heads, self.d, self.F
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        x = pb.buf((S, C), torch.float32, zero=True)
        x0 = x
        table = pb.const(causal_table(heads, S))
        layer_norm, linear, close = vit_common.trunk_helpers(pb, self.eps, self.tdt, self.dtype, stream32=True)
        st = (3 * C, d)
        for i, L in enumerate(self.W["layers"]):
            tag = f"clip{i}"
            qkv = linear(layer_norm(x, S, C, L["ln1"], tag + ".ln1"), L["qkv"], S, 3 * C, C, tag + ".qkv")
            o = pb.rel_attention(qkv, qkv, qkv, pb.buf((S, C), self.tdt), S, heads, heads, d, st, st, st, (C, d), d ** -0.5, rel=table,
                                 k_off=C, v_off=2 * C, label=tag + ".attn")
            x1 = close(o, L["o"], S, C, C, x, tag + ".out_proj")
            h = linear(layer_norm(x1, S, C, L["ln2"], tag + ".ln2"), L["fc1"], S, F, C, tag + ".fc1", act=self.act)
            x = close(h, L["fc2"], S, C, F, x1, tag + ".fc2")
        out = layer_norm(x, S, C, self.W["final"], "clip.final_ln")
        plan = pb.build()
        plan.x0, plan.out = x0, out
        return plan

    def pool_index(self, ids: torch.Tensor) -> int:
        """the row pooler_output takes: argmax(ids) when the config's eos_token_id is 2 (the legacy rule the published CLIP-L config triggers),
        else the first position holding eos_token_id"""
        if self.eos == 2:
            return int(ids.argmax())
        hit = (ids == self.eos).nonzero().reshape(-1)
        return int(hit[0]) if hit.numel() else 0

    def encode_ids(self, ids) -> torch.Tensor:
        """ids [S <= positions] -> last_hidden_state [S, hidden] of the storage type"""
        ids = self._ids(ids, self.embed.shape[0])
        S = int(ids.numel())
        if S > self.pos.shape[0]:
            raise ModelError(f"{self.WHAT}: {S} tokens exceed the {self.pos.shape[0]} positions")
        plan = self._plan(S)
        plan.x0.copy_(self.embed[ids].float() + self.pos[:S])
        self._run(plan)
        return plan.out.clone()

    def pooled(self, ids) -> torch.Tensor:
        ids = self._ids(ids, self.embed.shape[0])
        return self.encode_ids(ids)[self.pool_index(ids)].clone()

"""FLUX.1-Kontext (MMDiT + VAE + flow-match Euler) on libmtx_hip — SURVEY.md §8 row a7.

The object `ModelManager.load_flux_kontext_sdnq()` hands to `FluxKontextInpainter`; called with the
diffusers pipeline shape (reference core/image/inpainting.py:877-887):
    pipeline(image=PIL, width=, height=, num_inference_steps=, guidance_scale=, generator=,
             output_type="pt", max_area=, prompt_embeds=, pooled_prompt_embeds=).images[0]  -> CHW float 0..1
Weights carry diffusers' names (FluxTransformer2DModel / AutoencoderKL state dicts); the architecture
followed is restated in oracle/flux_ref.py.

Graph design (MI355X-first):
  * text and image tokens live in ONE [T, D] buffer (text rows first): the double-stream blocks work on
    row ranges, the single-stream blocks on the whole buffer — the reference's torch.cat / split per block
    do not exist.  q, k, v come from one fused [3D, D] GEMM per stream; per-head RMSNorm + 3-axis RoPE is
    one in-place kernel over the q and k column slices; attention reads q/k/v through strides.
  * every gated residual `x + gate * f(x)` is the GEMM epilogue (gate row broadcast + residual), GELU-tanh
    and bias likewise; AdaLayerNorm = the row-norm kernel with the (1 + scale), shift vectors fused.
  * single-stream blocks write attention output and MLP activations into column slices of one [T, 5D]
    buffer, so `proj_out(cat(attn, mlp))` is a plain GEMM.
  * the modulation vectors depend only on (timestep, guidance, pooled prompt): they are computed once per
    step of a schedule (M = 1 GEMVs that stream 6.4 GB of weights at full size) and cached, instead of
    every step of every region.
  * fp8 (`FluxDiTHip(fp8=True)`, opt-in): the block linears run on the MX-scaled fp8 matrix instructions (gemm.hip gemm256_f8_kernel) from
    weights quantised once at load; the adaLN norms, the joint attention and the MLP-in GEMMs (bias + GELU-tanh + quantisation in the epilogue,
    mtx_gemm_args.actq_*) write the next linear's e4m3 operand themselves into fp8 twins of the buffers above.  Everything else stays bf16 / fp32.
  * the ops a block is wired from (linear, adaLN norm, norm + RoPE, joint attention, quantiser pass), the weight holder and the modulation cache
    are core/ml/dit_graph.py's, shared with FLUX.2-Klein; this file keeps the parameter names, the block wiring, the side lane, the MLP-in
    epilogue and the decisions about who writes which fp8 operand.
  * VAE: NHWC 3x3 convs with fused bias / residual, GroupNorm+SiLU kernels, nearest-2x fused into a copy,
    Downsample2D's asymmetric pad as a conv mode; the single-head mid-block attention (d = 512) runs as
    GEMM -> row softmax -> GEMM.
"""
import math
import threading
from types import SimpleNamespace

import numpy as np
import torch

from ...hip import abi
from ...hip.lib import get_library
from ...hip.plan import Act, PlanBuilder, PlanCache, residual_distance
from ...utils.exceptions import ModelError
from . import packing
from .dit_graph import DiTStep, ModulationCache, Weight, _rows, quantize_weight


def sinusoid(value: float, dim=256) -> np.ndarray:
    half = dim // 2
    freqs = np.exp(-math.log(10000.0) * np.arange(half, dtype=np.float32) / half).astype(np.float32)
    a = np.float32(value) * freqs
    return np.concatenate([np.cos(a), np.sin(a)]).astype(np.float32)


def rope_table(ids: np.ndarray, axes_dim, theta=10000.0) -> np.ndarray:
    """ids [S,3] -> fp32 [S, 2, D/2]: cos | sin of every rotary pair."""
    cos, sin = [], []
    for i, d in enumerate(axes_dim):
        freqs = 1.0 / (theta ** (np.arange(0, d, 2, dtype=np.float64) / d))
        ang = ids[:, i].astype(np.float64)[:, None] * freqs[None]
        cos.append(np.cos(ang))
        sin.append(np.sin(ang))
    return np.stack([np.concatenate(cos, 1), np.concatenate(sin, 1)], 1).astype(np.float32)


def flow_sigmas(steps: int, image_seq_len: int) -> np.ndarray:
    """FlowMatchEulerDiscreteScheduler with dynamic exponential shifting (FluxKontextPipeline defaults)."""
    s = np.linspace(1.0, 1.0 / steps, steps)
    m = (1.15 - 0.5) / (4096 - 256)
    mu = image_seq_len * m + (0.5 - m * 256)
    s = math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))
    return np.append(s, 0.0).astype(np.float32)


def image_ids(h2, w2, first) -> np.ndarray:
    ids = np.zeros((h2, w2, 3), np.float32)
    ids[..., 0] = first
    ids[..., 1] = np.arange(h2)[:, None]
    ids[..., 2] = np.arange(w2)[None, :]
    return ids.reshape(-1, 3)


FP8_ALL = ("qkv", "to_out", "ff1", "ff2", "proj_mlp", "proj_out")      # the block linears by kind (both streams of a double block share a kind)


class FluxDiTHip:
    def __init__(self, provider, cfg: dict, device, lib=None, text_stream_on_side_lane: bool = True,
                 fp8=False, fused_quant=True, act_epilogue=True, attn_q8=True):
        """provider(name) -> tensor with diffusers' FluxTransformer2DModel parameter of that name.
        text_stream_on_side_lane: run the double-stream blocks' text ops beside the image ops (plan lanes); False keeps one lane.
        fp8: False (the bf16 graph), True (= every block linear) or a tuple of kinds out of FP8_ALL: those linears run on the MX-scaled fp8
        matrix instructions (gemm.hip gemm256_f8_kernel) — weights quantised once here (e4m3 + one E8M0 scale per 32 k, biases stay fp32), activations
        by the kernel that produces them.  Embedders, modulation GEMVs, norm_out / proj_out and all normalisation / softmax / residual arithmetic
        stay bf16 / fp32.  The three switches below only choose WHO writes an fp8 operand (same bytes either way; False = a separate
        mtx_quantize_mx launch behind the producer, for A/Bs):
        fused_quant: the adaLN norms write it (mtx_norm_args.q);  act_epilogue: ff1 / ff1_ctx / proj_mlp apply bias + GELU(tanh) and write it from
        the GEMM's registers (mtx_gemm_args.actq_*; needs 4 d % 256 == 0 and the MLP's second linear on fp8 too);  attn_q8: the joint attention
        writes it (mtx_attn_args.q8; head dim 128 and T >= 1024 only)."""
        self.side_lane = text_stream_on_side_lane
        self.lib = lib if lib is not None else get_library()
        self.device = torch.device(device)
        self.dtype, self.tdt = abi.BF16, torch.bfloat16
        self.cfg = cfg
        D, H = cfg["d"], cfg["heads"]
        self.hd = D // H
        if self.hd not in (64, 128) or sum(cfg["axes_dim"]) != self.hd:
            raise ModelError("FLUX DiT: head dim must be 64 or 128 and equal sum(axes_dims_rope)")
        self.fp8 = FP8_ALL if fp8 is True else tuple(fp8 or ())
        if any(k not in FP8_ALL for k in self.fp8):
            raise ModelError(f"FLUX DiT: fp8 kinds must come from {FP8_ALL}, got {self.fp8}")
        if self.fp8 and D % 128:
            raise ModelError("FLUX DiT fp8 path: d must be a multiple of 128")
        self.fused_quant = bool(fused_quant)
        self.act_epilogue = bool(act_epilogue) and (4 * D) % 256 == 0
        self.attn_q8 = bool(attn_q8) and self.hd == 128
        g = lambda n, dt=None: provider(n).detach().to(self.device, dt if dt is not None else self.tdt).contiguous()
        f32 = torch.float32
        W = {}
        for nm in ("x_embedder", "context_embedder", "proj_out"):
            W[nm] = (g(nm + ".weight"), g(nm + ".bias", f32))
        for e in ("timestep_embedder", "guidance_embedder", "text_embedder"):
            for l in ("linear_1", "linear_2"):
                W[f"{e}.{l}"] = (g(f"time_text_embed.{e}.{l}.weight"), g(f"time_text_embed.{e}.{l}.bias", f32))
        # all AdaLN projections stacked: one [n_vec * D, D] GEMV per step of a schedule
        mods_w, mods_b = [], []
        for i in range(cfg["layers"]):
            for nm in ("norm1", "norm1_context"):
                mods_w.append(g(f"transformer_blocks.{i}.{nm}.linear.weight")); mods_b.append(g(f"transformer_blocks.{i}.{nm}.linear.bias", f32))
        for i in range(cfg["single_layers"]):
            mods_w.append(g(f"single_transformer_blocks.{i}.norm.linear.weight")); mods_b.append(g(f"single_transformer_blocks.{i}.norm.linear.bias", f32))
        mods_w.append(g("norm_out.linear.weight")); mods_b.append(g("norm_out.linear.bias", f32))
        W["mods"] = (torch.cat(mods_w, 0).contiguous(), torch.cat(mods_b, 0).contiguous())
        self.n_vec = W["mods"][0].shape[0] // D
        self.blocks, self.singles = [], []
        cat3 = lambda p, names, kind="qkv": self._weight(torch.cat([g(f"{p}.{n}.weight") for n in names], 0).contiguous(), kind,
                                                         torch.cat([g(f"{p}.{n}.bias", f32) for n in names], 0).contiguous())
        lin = lambda name, kind: self._weight(g(name + ".weight"), kind, g(name + ".bias", f32))
        for i in range(cfg["layers"]):
            p = f"transformer_blocks.{i}"
            self.blocks.append(dict(
                qkv=cat3(p + ".attn", ("to_q", "to_k", "to_v")), cqkv=cat3(p + ".attn", ("add_q_proj", "add_k_proj", "add_v_proj")),
                nqk=torch.cat([g(p + ".attn.norm_q.weight", f32), g(p + ".attn.norm_k.weight", f32)]).contiguous(),
                cnqk=torch.cat([g(p + ".attn.norm_added_q.weight", f32), g(p + ".attn.norm_added_k.weight", f32)]).contiguous(),
                out=lin(p + ".attn.to_out.0", "to_out"), cout=lin(p + ".attn.to_add_out", "to_out"),
                ff1=lin(p + ".ff.net.0.proj", "ff1"), ff2=lin(p + ".ff.net.2", "ff2"),
                cff1=lin(p + ".ff_context.net.0.proj", "ff1"), cff2=lin(p + ".ff_context.net.2", "ff2")))
        for i in range(cfg["single_layers"]):
            p = f"single_transformer_blocks.{i}"
            self.singles.append(dict(qkv=cat3(p + ".attn", ("to_q", "to_k", "to_v")),
                                     nqk=torch.cat([g(p + ".attn.norm_q.weight", f32), g(p + ".attn.norm_k.weight", f32)]).contiguous(),
                                     mlp=lin(p + ".proj_mlp", "proj_mlp"), out=lin(p + ".proj_out", "proj_out")))
        self.W = W
        self._plans = PlanCache(6)           # a DiT plan pins ~T x 15 D bytes of activations: a few crop resolutions only
        self._mods = ModulationCache(self._build_mod_plan, self.n_vec)

    def _weight(self, w16: torch.Tensor, kind: str, bias) -> Weight:
        """one block linear: the 16-bit weight, or — for a kind on the fp8 path — its MX fp8 copy"""
        return quantize_weight(self.lib, self.device, self.dtype, w16, bias) if kind in self.fp8 else Weight(w16, bias=bias)

    # ---- modulation vectors of one (timestep, guidance, pooled) ------------------------------------------
    def _build_mod_plan(self):
        D, W = self.cfg["d"], self.W
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        tin = pb.buf((2, 256), self.tdt)                     # sinusoids of timestep*1000 and guidance*1000
        pooled = pb.buf((1, self.cfg["pooled_dim"]), self.tdt)
        embs = []
        for row, (e, src, k) in enumerate((("timestep_embedder", tin, 256), ("guidance_embedder", tin, 256), ("text_embedder", pooled, self.cfg["pooled_dim"]))):
            off = row * 256 if src is tin and row < 2 else 0
            h = pb.gemm(src, W[f"{e}.linear_1"][0], 1, D, k, bias=W[f"{e}.linear_1"][1], act=abi.ACT_SILU, a_off=off, label=f"temb.{e}.1")
            embs.append(pb.gemm(h, W[f"{e}.linear_2"][0], 1, D, D, bias=W[f"{e}.linear_2"][1], label=f"temb.{e}.2"))
        a = lambda t: Act(t.view(1, 1, 1, D), 1, 1, 1, D)
        s1 = pb.ew(abi.EW_ADD, a(embs[0]), b=a(embs[1]), label="temb.sum1")
        st = pb.ew(abi.EW_ADD, s1, b=a(embs[2]), act=abi.ACT_SILU, label="temb.sum2.silu")       # silu(temb) feeds every AdaLN
        mods = pb.gemm(st.t.view(1, D), W["mods"][0], 1, self.n_vec * D, D, bias=W["mods"][1], label="adaln.all")
        plan = pb.build()
        plan.tin, plan.pooled, plan.mods = tin, pooled, mods
        return plan

    def modulation(self, timestep: float, guidance: float, pooled: torch.Tensor, pooled_key=None) -> torch.Tensor:
        """[n_vec, D] bf16 modulation rows for one denoising step, cached per (timestep, guidance, pooled prompt).
        `pooled_key` identifies the pooled-prompt CONTENT (callers hash it once per image, not once per step)."""
        if pooled_key is None:
            pooled_key = hash(pooled.detach().float().cpu().numpy().tobytes())
        key = (round(float(timestep), 7), round(float(guidance), 5), pooled_key)

        def fill(mp):
            tin = np.stack([sinusoid(timestep * 1000.0), sinusoid(guidance * 1000.0)])
            mp.tin.copy_(torch.from_numpy(tin).to(self.device, self.tdt))
            mp.pooled.copy_(pooled.reshape(1, -1).to(self.device, self.tdt))
        return self._mods.get(key, fill)

    # ---- one denoising step as a plan ----------------------------------------------------------------------
    def _build(self, t_txt, h2, w2, n_ref, cached: bool = False):
        """One denoising step.  cached=False: ONE plan (what every round measured).  cached=True (first-block cache, reference
        core/ml/model_manager.py:1159-1162): the same ops as three plans over shared buffers — `head` (embedders, double block 0, the
        residual-distance probe), `body` (this step's first residual kept, blocks 1.., the whole-stack residual kept, output layers) and
        `skip` (cached whole-stack residual added, output layers) — so that the host can choose between `body` and `skip` after `head`."""
        cfg, W = self.cfg, self.W
        D, H = cfg["d"], cfg["heads"]
        t_noise = h2 * w2
        t_img = t_noise * (1 + n_ref)
        T = t_txt + t_img
        new_pb = lambda: PlanBuilder(self.lib, self.device, self.dtype, lanes=self.side_lane)
        pb = new_pb()
        lat = pb.buf((t_img, cfg["in_channels"]), self.tdt)       # [noise tokens ; reference tokens]
        ctx_in = pb.buf((t_txt, cfg["joint_dim"]), self.tdt)      # prompt embeddings
        ids = np.concatenate([np.zeros((t_txt, 3), np.float32)] + [image_ids(h2, w2, k) for k in range(1 + n_ref)])
        g = DiTStep(pb, T, D, H, self.n_vec, torch.from_numpy(rope_table(ids, cfg["axes_dim"])), bool(self.fp8), self.fused_quant)
        x, nrm, nrm8, mod, lds = g.x, g.nrm, g.nrm8, g.mod, g.lds
        qkv = pb.buf((T, 3 * D), self.tdt)
        o = pb.buf((T, D), self.tdt)
        hid = pb.buf((T, 4 * D), self.tdt)
        cat = pb.buf((T, 5 * D), self.tdt)
        vel = pb.buf((t_noise, cfg["in_channels"]), torch.float32)
        o8, hid8, cat8 = g.twin(pb, D), g.twin(pb, 4 * D), g.twin(pb, 5 * D)      # fp8 twins of the GEMM inputs (nrm8 is the recorder's)
        on = lambda *kinds: all(k in self.fp8 for k in kinds)
        ep_ff, ep_mlp = self.act_epilogue and on("ff1", "ff2"), self.act_epilogue and on("proj_mlp", "proj_out")      # who writes hid8 / cat8[:, D:]
        aq8_dbl, aq8_sgl = self.attn_q8 and T >= 1024 and on("to_out"), self.attn_q8 and T >= 1024 and on("proj_out")  # who writes o8 / cat8[:, :D]

        def embed(pb):
            pb.gemm(ctx_in, W["context_embedder"][0], t_txt, D, cfg["joint_dim"], bias=W["context_embedder"][1], out=x, label="context_embedder")
            pb.gemm(lat, W["x_embedder"][0], t_img, D, cfg["in_channels"], bias=W["x_embedder"][1], out=x, c_off=t_txt * D, label="x_embedder")

        def mlp_in(pb, w, r0, r1, out, c_col, dst8, fused, consumer, label):
            """Linear + bias + GELU(tanh) of rows [r0, r1) of nrm into out[:, c_col : c_col + 4 D].  An fp8 consumer reads the twin dst8 instead: written by
            this GEMM's epilogue (fused: no 16-bit result exists) or by a quantiser launch behind it"""
            ldc = out.shape[1]
            if fused:
                g.linear(pb, nrm, nrm8, w, r0, r1, 4 * D, D, None, ldc=ldc, c_col=c_col, act=abi.ACT_GELU_TANH, label=label,
                         actq=(dst8[0], dst8[1], ldc, lds, r0, c_col))
                return
            g.linear(pb, nrm, nrm8, w, r0, r1, 4 * D, D, out, ldc=ldc, c_col=c_col, act=abi.ACT_GELU_TANH, label=label)
            if consumer.fp8:
                g.quant(pb, out, ldc, 4 * D, dst8, r0, r1, label + ".q", c0=c_col)

        # Double-stream blocks: the text stream's ops (512 rows: GEMMs of 24 - 96 tiles that cannot fill the chip, 4 % of a step when run in
        # line) go to the plan's SIDE lane and run beside the image stream's ops; the lanes meet at the joint attention and at the next block.
        # The two streams touch disjoint row ranges of every shared buffer.
        def double_block(pb, i, B):
            b0 = i * 12
            tag = f"dbl{i}"
            with pb.side():
                g.adaln(pb, 0, t_txt, b0 + 6, b0 + 7, tag + ".norm1_ctx", (B["cqkv"],))
                g.linear(pb, nrm, nrm8, B["cqkv"], 0, t_txt, 3 * D, D, qkv, label=tag + ".qkv_ctx")
                g.rope(pb, qkv, 0, t_txt, B["cnqk"], tag + ".rope_qk_ctx")
            g.adaln(pb, t_txt, T, b0 + 0, b0 + 1, tag + ".norm1", (B["qkv"],))
            g.linear(pb, nrm, nrm8, B["qkv"], t_txt, T, 3 * D, D, qkv, label=tag + ".qkv")
            g.rope(pb, qkv, t_txt, T, B["nqk"], tag + ".rope_qk")
            pb.join()
            g.attention(pb, qkv, o, tag + ".attn", q8=o8 if aq8_dbl else None)
            if on("to_out") and not aq8_dbl:
                g.quant(pb, o, D, D, o8, 0, T, tag + ".attn.q")
            with pb.side():
                g.linear(pb, o, o8, B["cout"], 0, t_txt, D, D, x, gate=mod[b0 + 8], gate_rows_per=t_txt, res=x, label=tag + ".to_add_out")
                g.adaln(pb, 0, t_txt, b0 + 9, b0 + 10, tag + ".norm2_ctx", (B["cff1"],))
                mlp_in(pb, B["cff1"], 0, t_txt, hid, 0, hid8, ep_ff, B["cff2"], tag + ".ff1_ctx")
                g.linear(pb, hid, hid8, B["cff2"], 0, t_txt, D, 4 * D, x, gate=mod[b0 + 11], gate_rows_per=t_txt, res=x, label=tag + ".ff2_ctx")
            g.linear(pb, o, o8, B["out"], t_txt, T, D, D, x, gate=mod[b0 + 2], gate_rows_per=t_img, res=x, res_off=t_txt * D, label=tag + ".to_out")
            g.adaln(pb, t_txt, T, b0 + 3, b0 + 4, tag + ".norm2", (B["ff1"],))
            mlp_in(pb, B["ff1"], t_txt, T, hid, 0, hid8, ep_ff, B["ff2"], tag + ".ff1")
            g.linear(pb, hid, hid8, B["ff2"], t_txt, T, D, 4 * D, x, gate=mod[b0 + 5], gate_rows_per=t_img, res=x, res_off=t_txt * D, label=tag + ".ff2")

        s0 = cfg["layers"] * 12

        def single_block(pb, i, S):
            b0 = s0 + i * 3
            tag = f"sgl{i}"
            g.adaln(pb, 0, T, b0 + 0, b0 + 1, tag + ".norm", (S["qkv"], S["mlp"]))
            g.linear(pb, nrm, nrm8, S["qkv"], 0, T, 3 * D, D, qkv, label=tag + ".qkv")
            mlp_in(pb, S["mlp"], 0, T, cat, D, cat8, ep_mlp, S["out"], tag + ".proj_mlp")
            g.rope(pb, qkv, 0, T, S["nqk"], tag + ".rope_qk")
            g.attention(pb, qkv, cat, tag + ".attn", q8=cat8 if aq8_sgl else None)
            if on("proj_out") and not aq8_sgl:          # the attention half of the concatenation: its own quantiser pass over columns [0, D)
                g.quant(pb, cat, 5 * D, D, cat8, 0, T, tag + ".attn.q")
            g.linear(pb, cat, cat8, S["out"], 0, T, D, 5 * D, x, gate=mod[b0 + 2], gate_rows_per=T, res=x, label=tag + ".proj_out")

        f0 = s0 + cfg["single_layers"] * 3

        def output_layers(pb):
            pb.norm(x, nrm, t_noise, D, eps=1e-6, kind=0, mod_scale=mod[f0], mod_shift=mod[f0 + 1], rows_per=t_noise, ldmod=D,
                    x_off=t_txt * D, y_off=t_txt * D, label="norm_out")
            pb.gemm(nrm, W["proj_out"][0], t_noise, cfg["in_channels"], D, bias=W["proj_out"][1], a_off=t_txt * D, out=vel, out_f32=True, label="proj_out")

        def finish(plan):
            plan.lat, plan.ctx_in, plan.mod, plan.vel, plan.x = lat, ctx_in, mod, vel, x
            plan.t_noise, plan.t_img, plan.T = t_noise, t_img, T
            return plan

        if not cached:
            embed(pb)
            for i, B in enumerate(self.blocks):
                double_block(pb, i, B)
            pb.join()                 # the single-stream blocks read every row
            for i, S in enumerate(self.singles):
                single_block(pb, i, S)
            output_layers(pb)
            return finish(pb.build())

        # ---- first-block cache: three plans over the buffers above ------------------------------------------------------------------
        rows2d = lambda t, r0, r1: _rows(t, r0, r1)
        x0 = pb.buf((t_img, D), self.tdt)              # image stream before block 0
        first_prev = pb.buf((t_img, D), self.tdt, zero=True)      # first-block residual of the last COMPUTED step
        x1 = pb.buf((T, D), self.tdt)                  # both streams after block 0
        whole = pb.buf((T, D), self.tdt, zero=True)    # whole-stack residual of the last computed step (x after the last block - x1)
        embed(pb)
        pb.ew(abi.EW_COPY, rows2d(x, t_txt, T), out=rows2d(x0, 0, t_img), label="cache.keep_x0")
        double_block(pb, 0, self.blocks[0])
        pb.join()
        parts = pb.residual_dist(x, x0, first_prev, t_img, D, after_off=t_txt * D, label="cache.probe")
        head = finish(pb.build())
        pb_b = new_pb()
        pb_b.ew(abi.EW_SUB, rows2d(x, t_txt, T), b=rows2d(x0, 0, t_img), out=rows2d(first_prev, 0, t_img), label="cache.keep_first_residual")
        pb_b.ew(abi.EW_COPY, rows2d(x, 0, T), out=rows2d(x1, 0, T), label="cache.keep_x1")
        for i, B in enumerate(self.blocks[1:], start=1):
            double_block(pb_b, i, B)
        pb_b.join()
        for i, S in enumerate(self.singles):
            single_block(pb_b, i, S)
        pb_b.ew(abi.EW_SUB, rows2d(x, 0, T), b=rows2d(x1, 0, T), out=rows2d(whole, 0, T), label="cache.keep_whole_residual")
        output_layers(pb_b)
        body = finish(pb_b.build())
        pb_c = new_pb()
        pb_c.ew(abi.EW_ADD, rows2d(x, 0, T), b=rows2d(whole, 0, T), out=rows2d(x, 0, T), label="cache.apply_whole_residual")
        output_layers(pb_c)
        skip = finish(pb_c.build())
        head.body, head.skip, head.parts = body, skip, parts
        head.cache_buffers = (x0, first_prev, x1, whole)
        return head

    def plan_for(self, t_txt, h2, w2, n_ref=1, cached: bool = False):
        """cached: the three-plan form of the first-block cache (`.body`, `.skip`, `.parts` hang off the returned head plan)"""
        key = (t_txt, h2, w2, n_ref) + (("cached",) if cached else ())
        if key not in self._plans:
            self._plans[key] = self._build(t_txt, h2, w2, n_ref, cached)
        return self._plans[key]

    def flops_per_step(self, t_txt, h2, w2, n_ref=1):
        cfg = self.cfg
        D = cfg["d"]
        t_img = h2 * w2 * (1 + n_ref)
        T = t_txt + t_img
        dbl = cfg["layers"] * (2 * T * D * 3 * D + 2 * T * D * D + 2 * 2 * T * D * 4 * D)
        sgl = cfg["single_layers"] * (2 * T * D * 3 * D + 2 * T * D * 4 * D + 2 * T * 5 * D * D)
        attn = (cfg["layers"] + cfg["single_layers"]) * 4 * T * T * D
        return dict(gemm=dbl + sgl, attention=attn, attention_per_layer=4 * T * T * D, tokens=T)


class FluxVAEHip:
    def __init__(self, provider, cfg: dict, device, lib=None):
        self.lib = lib if lib is not None else get_library()
        self.device = torch.device(device)
        self.dtype, self.tdt = abi.BF16, torch.bfloat16
        self.cfg = cfg
        self.p = provider
        self._w = {}
        self._plans = PlanCache(12)

    def _conv_w(self, name, cout_pad=0):
        if name not in self._w:
            w = self.p(name + ".weight").detach().float().cpu()
            wt = packing.conv_taps(w, cout_pad=cout_pad)
            bt = packing.padded_bias(self.p(name + ".bias").detach().float().cpu(), cout_pad)
            self._w[name] = (packing.on_device(wt, self.device, self.tdt), packing.on_device(bt, self.device), wt.shape[0], w.shape[2])
        return self._w[name]

    def _vec(self, name):
        if name not in self._w:
            self._w[name] = packing.on_device(self.p(name).detach(), self.device)
        return self._w[name]

    def _lin(self, name):
        if name not in self._w:
            self._w[name] = (packing.on_device(self.p(name + ".weight").detach(), self.device, self.tdt), packing.on_device(self.p(name + ".bias").detach(), self.device))
        return self._w[name]

    def _conv(self, pb, x, name, stride=1, res=None, pad_mode=0, cout_pad=0):
        w, b, co, k = self._conv_w(name, cout_pad)
        return pb.conv2d(x, w, b, co, ksize=k, stride=stride, res=res, pad_mode=pad_mode, label=name)

    def _gn(self, pb, x, name, silu=True):
        return pb.groupnorm(x, self._vec(name + ".weight"), self._vec(name + ".bias"), self.cfg["groups"], 1e-6,
                            abi.ACT_SILU if silu else abi.ACT_NONE, label=name)

    def _res(self, pb, x, p, cout):
        h = self._conv(pb, self._gn(pb, x, p + ".norm1"), p + ".conv1")
        sc = self._conv(pb, x, p + ".conv_shortcut") if x.c != cout else x
        return self._conv(pb, self._gn(pb, h, p + ".norm2"), p + ".conv2", res=sc)

    def _attn(self, pb, x, p):
        C, T = x.c, x.h * x.w
        t = self._gn(pb, x, p + ".group_norm", silu=False)
        q = pb.gemm(t.t, self._lin(p + ".to_q")[0], T, C, C, bias=self._lin(p + ".to_q")[1], label=p + ".q")
        Tp = (T + 7) // 8 * 8                  # H/8 x W/8 tokens: a multiple of 4, not always of 8 (e.g. a 1296 x 784 Klein crop)
        k = pb.buf((Tp, C), self.tdt, zero=True)
        pb.gemm(t.t, self._lin(p + ".to_k")[0], T, C, C, bias=self._lin(p + ".to_k")[1], out=k, label=p + ".k")
        v = pb.gemm(t.t, self._lin(p + ".to_v")[0], T, C, C, bias=self._lin(p + ".to_v")[1], label=p + ".v")
        s = pb.buf((T, Tp), self.tdt, zero=True)
        pb.gemm(q, k, T, Tp, C, out=s, ldc=Tp, label=p + ".qk")          # the padded key rows are zero and are masked out of the softmax
        sa = Act(s.view(1, 1, T, Tp), 1, 1, T, Tp)
        pb.ew(abi.EW_SOFTMAX_ROWS, sa, out=sa, act_param=1.0 / math.sqrt(C), i0=T if Tp != T else 0, label=p + ".softmax")
        vt = pb.buf((C, Tp), self.tdt, zero=True)
        pb.ew(abi.EW_TRANSPOSE, Act(v.view(1, 1, T, C), 1, 1, T, C), out=Act(vt.view(1, 1, C, Tp), 1, 1, C, Tp), label=p + ".v_t")
        o = pb.gemm(s, vt, T, C, Tp, label=p + ".pv")
        out = pb.act(x.n, x.h, x.w, C)
        pb.gemm(o, self._lin(p + ".to_out.0")[0], T, C, C, bias=self._lin(p + ".to_out.0")[1], res=x.t, out=out.t, label=p + ".out")
        return out

    def _mid(self, pb, x, p):
        x = self._res(pb, x, p + ".resnets.0", x.c)
        x = self._attn(pb, x, p + ".attentions.0")
        return self._res(pb, x, p + ".resnets.1", x.c)

    def encoder_plan(self, h, w):
        key = ("enc", h, w)
        if key not in self._plans:
            ch = self.cfg["ch"]
            pb = PlanBuilder(self.lib, self.device, self.dtype)
            src = pb.buf((1, h, w, 3), torch.uint8)
            x0 = pb.act(1, h, w, 8)
            pb.image_convert(abi.IMG_HWC_U8_TO_NHWC, src, x0.t, 1, h, w, 8, mul=2.0, add=(-1.0, -1.0, -1.0), label="vae.in")
            x = self._conv(pb, x0, "encoder.conv_in")
            for i, c in enumerate(ch):
                for j in range(2):
                    x = self._res(pb, x, f"encoder.down_blocks.{i}.resnets.{j}", c)
                if i < len(ch) - 1:
                    x = self._conv(pb, x, f"encoder.down_blocks.{i}.downsamplers.0.conv", stride=2, pad_mode=1)
            x = self._mid(pb, x, "encoder.mid_block")
            x = self._conv(pb, self._gn(pb, x, "encoder.conv_norm_out"), "encoder.conv_out")
            if self.cfg.get("quant_conv"):                       # AutoencoderKLFlux2: 1x1 conv over the moments
                x = self._conv(pb, x, "quant_conv")
            plan = pb.build()
            plan.src, plan.moments = src, x
            self._plans[key] = plan
        return self._plans[key]

    def decoder_plan(self, h8, w8):
        key = ("dec", h8, w8)
        if key not in self._plans:
            rc = list(reversed(self.cfg["ch"]))
            pb = PlanBuilder(self.lib, self.device, self.dtype)
            z = pb.act(1, h8, w8, self.cfg.get("latent", 16))
            x = self._conv(pb, self._conv(pb, z, "post_quant_conv"), "decoder.conv_in") if self.cfg.get("quant_conv") else self._conv(pb, z, "decoder.conv_in")
            x = self._mid(pb, x, "decoder.mid_block")
            for i, c in enumerate(rc):
                for j in range(3):
                    x = self._res(pb, x, f"decoder.up_blocks.{i}.resnets.{j}", c)
                if i < len(rc) - 1:
                    x = self._conv(pb, pb.ew(abi.EW_UPSAMPLE2X, x, label=f"decoder.up{i}.nearest"), f"decoder.up_blocks.{i}.upsamplers.0.conv")
            y = self._conv(pb, self._gn(pb, x, "decoder.conv_norm_out"), "decoder.conv_out", cout_pad=8)
            out = pb.buf((1, 3, y.h, y.w), torch.float32)
            pb.image_convert(abi.IMG_NHWC_TO_NCHW_F32, y.t, out, 1, y.h, y.w, 8, mul=0.5, add=(0.5, 0.5, 0.5), label="vae.out")
            plan = pb.build()
            plan.z, plan.out, plan.raw = z, out, y
            self._plans[key] = plan
        return self._plans[key]


PROMPTS_KEPT = 4                      # encoded prompts a pipeline keeps beside the stored one (`set_text_encoder`)


class FluxKontextHip:
    """diffusers-pipeline-shaped callable built from the two graphs above."""

    def __init__(self, dit: FluxDiTHip, vae: FluxVAEHip, graph: bool = True):
        self.transformer, self.vae = dit, vae
        self.device = dit.device
        self._execution_device = dit.device
        self._graph = graph and not dit.lib.is_simulator
        self._lock = threading.Lock()
        self._embeds = None
        self._stored_prompt, self._text_encoder, self._encoded = None, None, {}
        self.calls = 0                # pipeline invocations (benchmarks assert the expected number of FLUX regions ran)
        self.completed = 0            # ... that returned an image (a call that raised is caught by the OSB stage and becomes a flat fill)
        # First-block cache (reference core/ml/model_manager.py:1159-1162: nunchaku's apply_cache_on_pipe(pipeline, residual_diff_threshold=)).
        # 0 = off: every step runs every block through the one-plan graph (byte-identical to the builds before round 5).  > 0: after double
        # block 0 the image stream's residual is compared with the last computed step's (mean |difference| / mean |previous|); below the
        # threshold the other 56 blocks are skipped and the cached whole-stack residual is added.  `FluxKontextInpainter` sets it for
        # backend "nunchaku" only, like the reference.  Parity with nunchaku's implementation is UNPINNED (the wheel is not installable here).
        self.residual_diff_threshold = 0.0
        self.cache_stats = {"steps": 0, "skipped": 0}      # over the pipeline's lifetime; `last["skipped_steps"]` holds the last call's count

    def set_prompt_embeds(self, prompt_embeds: torch.Tensor, pooled: torch.Tensor, prompt=None):
        """T5 / CLIP embeddings of the (fixed) prompt — computed once per process by the caller.  prompt: the text they encode (the stored
        file's metadata), which `encode_prompt` compares against once a text encoder is attached"""
        self._embeds = (prompt_embeds.reshape(-1, prompt_embeds.shape[-1]), pooled.reshape(-1))
        self._stored_prompt = prompt

    def set_text_encoder(self, fn):
        """fn(prompt) -> (T5 sequence [512, 4096], CLIP pooled [768]): `encode_prompt` calls it for a prompt other than the stored one and keeps
        the last few results; None detaches it (a foreign prompt then gets the stored tensors, as before the hook existed)"""
        self._text_encoder, self._encoded = fn, {}

    def encode_prompt(self, prompt=None, prompt_2=None, device=None, **kw):
        if self._text_encoder is not None and prompt is not None and prompt != self._stored_prompt:
            if prompt not in self._encoded:
                if len(self._encoded) >= PROMPTS_KEPT:
                    self._encoded.pop(next(iter(self._encoded)))
                seq, pooled = self._text_encoder(prompt)
                self._encoded[prompt] = (seq.reshape(-1, seq.shape[-1]).to(self.device), pooled.reshape(-1).to(self.device))
            seq, pooled = self._encoded[prompt]
            return seq[None], pooled[None], None
        if self._embeds is None:
            raise ModelError("no prompt embeddings: the loader encodes the fixed prompt once when the snapshot's text_encoder/, text_encoder_2/, tokenizer/, tokenizer_2/ "
                             "folders are staged next to transformer/ (core/ml/prompt_embeds.py); otherwise run `python tools/export_prompt_embeds.py kontext <pipeline "
                             "snapshot>` (writes prompt_embeds.safetensors) or hand the tensors to set_prompt_embeds()")
        return self._embeds[0][None], self._embeds[1][None], None

    @torch.no_grad()
    def __call__(self, image=None, width=None, height=None, num_inference_steps=8, guidance_scale=2.5, generator=None,
                 output_type="pt", max_area=None, prompt_embeds=None, pooled_prompt_embeds=None, latents=None, **kw):
        self.calls += 1
        if prompt_embeds is None:
            prompt_embeds, pooled_prompt_embeds, _ = self.encode_prompt()
        pe = prompt_embeds.reshape(-1, prompt_embeds.shape[-1])
        pooled = pooled_prompt_embeds.reshape(-1)
        img_dev = image if torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 else None      # already on the device, already at size
        if img_dev is not None:
            img = img_dev
        else:
            img = np.asarray(image.convert("RGB").resize((width, height))) if hasattr(image, "convert") else np.asarray(image)
        H, W = int(img.shape[0]), int(img.shape[1])
        if H % 16 or W % 16:
            raise ModelError(f"FLUX Kontext needs H, W multiples of 16, got {W}x{H}")
        h8, w8, h2, w2 = H // 8, W // 8, H // 16, W // 16
        dit, vae = self.transformer, self.vae
        vc = vae.cfg
        with self._lock:
            enc = vae.encoder_plan(H, W)
            enc.src.copy_((img_dev if img_dev is not None else torch.from_numpy(np.array(img, dtype=np.uint8)).to(self.device)).reshape(1, H, W, 3))
            enc.run(graph=self._graph)
            mean = enc.moments.t[0, :, :, :16].float().permute(2, 0, 1)[None]
            ref = (mean - vc["shift_factor"]) * vc["scaling_factor"]
            pack = lambda t: t.view(1, 16, h2, 2, w2, 2).permute(0, 2, 4, 1, 3, 5).reshape(h2 * w2, 64)
            if latents is None:
                latents = torch.randn((1, 16, h8, w8), generator=generator, dtype=torch.float32,
                                      device=generator.device if generator is not None else "cpu")
            lat = pack(latents.to(self.device, torch.float32))
            threshold = float(kw.get("residual_diff_threshold", self.residual_diff_threshold) or 0.0)
            plan = dit.plan_for(pe.shape[0], h2, w2, 1, cached=threshold > 0.0)
            plan.ctx_in.copy_(pe.to(self.device, dit.tdt))
            plan.lat[plan.t_noise:].copy_(pack(ref).to(dit.tdt))
            sig = flow_sigmas(num_inference_steps, h2 * w2)
            pooled_dev = pooled.to(self.device, dit.tdt)
            pooled_key = hash(pooled_dev.float().cpu().numpy().tobytes())
            have_cache, skipped = False, []               # the cache lives for ONE call, like the reference's cache context
            for i in range(num_inference_steps):
                plan.mod.copy_(dit.modulation(float(sig[i]), float(guidance_scale), pooled_dev, pooled_key))
                plan.lat[: plan.t_noise].copy_(lat.to(dit.tdt))
                plan.run(graph=self._graph)
                if threshold > 0.0:
                    # `plan` was the head (embedders, block 0, probe): the one host decision of the step
                    use = have_cache and residual_distance(plan.parts) < threshold
                    (plan.skip if use else plan.body).run(graph=self._graph)
                    have_cache = True
                    skipped.append(bool(use))
                lat = lat + (float(sig[i + 1]) - float(sig[i])) * plan.vel
            self.cache_stats["steps"] += num_inference_steps
            self.cache_stats["skipped"] += sum(skipped)
            z = lat.view(1, h2, w2, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(1, 16, h8, w8) / vc["scaling_factor"] + vc["shift_factor"]
            dec = vae.decoder_plan(h8, w8)
            dec.z.t.copy_(z.permute(0, 2, 3, 1).to(dit.tdt))
            dec.run(graph=self._graph)
            out = dec.out[0].clamp(0, 1).clone()
            self.last = dict(latents=lat, sigmas=sig, skipped_steps=sum(skipped), skipped=skipped)
        self.completed += 1
        return SimpleNamespace(images=[out])


# ---- parameter inventories (diffusers names) ------------------------------------------------------------
KONTEXT_DIT_CFG = dict(d=3072, heads=24, layers=19, single_layers=38, in_channels=64, joint_dim=4096, pooled_dim=768, axes_dim=(16, 56, 56))
KONTEXT_VAE_CFG = dict(ch=(128, 256, 512, 512), groups=32, scaling_factor=0.3611, shift_factor=0.1159)


def dit_param_shapes(cfg: dict) -> dict:
    D, hd = cfg["d"], cfg["d"] // cfg["heads"]
    s = {}

    def lin(name, dout, din):
        s[name + ".weight"], s[name + ".bias"] = (dout, din), (dout,)

    lin("x_embedder", D, cfg["in_channels"]); lin("context_embedder", D, cfg["joint_dim"]); lin("proj_out", cfg["in_channels"], D)
    for e, din in (("timestep_embedder", 256), ("guidance_embedder", 256), ("text_embedder", cfg["pooled_dim"])):
        lin(f"time_text_embed.{e}.linear_1", D, din); lin(f"time_text_embed.{e}.linear_2", D, D)
    for i in range(cfg["layers"]):
        p = f"transformer_blocks.{i}"
        lin(p + ".norm1.linear", 6 * D, D); lin(p + ".norm1_context.linear", 6 * D, D)
        for n in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"):
            lin(f"{p}.attn.{n}", D, D)
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            s[f"{p}.attn.{n}.weight"] = (hd,)
        for ff in ("ff", "ff_context"):
            lin(f"{p}.{ff}.net.0.proj", 4 * D, D); lin(f"{p}.{ff}.net.2", D, 4 * D)
    for i in range(cfg["single_layers"]):
        p = f"single_transformer_blocks.{i}"
        lin(p + ".norm.linear", 3 * D, D); lin(p + ".proj_mlp", 4 * D, D); lin(p + ".proj_out", D, 5 * D)
        for n in ("to_q", "to_k", "to_v"):
            lin(f"{p}.attn.{n}", D, D)
        s[f"{p}.attn.norm_q.weight"] = s[f"{p}.attn.norm_k.weight"] = (hd,)
    lin("norm_out.linear", 2 * D, D)
    return s


def vae_param_shapes(cfg: dict) -> dict:
    ch = cfg["ch"]
    s = {}

    def conv(name, co, ci, k=3):
        s[name + ".weight"], s[name + ".bias"] = (co, ci, k, k), (co,)

    def gn(name, c):
        s[name + ".weight"] = s[name + ".bias"] = (c,)

    def res(p, ci, co):
        gn(p + ".norm1", ci); conv(p + ".conv1", co, ci); gn(p + ".norm2", co); conv(p + ".conv2", co, co)
        if ci != co:
            conv(p + ".conv_shortcut", co, ci, 1)

    def mid(p, c):
        res(p + ".resnets.0", c, c); res(p + ".resnets.1", c, c)
        gn(p + ".attentions.0.group_norm", c)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            s[f"{p}.attentions.0.{n}.weight"], s[f"{p}.attentions.0.{n}.bias"] = (c, c), (c,)

    conv("encoder.conv_in", ch[0], 3)
    c = ch[0]
    for i, co in enumerate(ch):
        for j in range(2):
            res(f"encoder.down_blocks.{i}.resnets.{j}", c, co); c = co
        if i < len(ch) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c, c)
    mid("encoder.mid_block", c); gn("encoder.conv_norm_out", c); conv("encoder.conv_out", 32, c)
    rc = list(reversed(ch))
    conv("decoder.conv_in", rc[0], 16)
    c = rc[0]
    mid("decoder.mid_block", c)
    for i, co in enumerate(rc):
        for j in range(3):
            res(f"decoder.up_blocks.{i}.resnets.{j}", c, co); c = co
        if i < len(rc) - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c)
    gn("decoder.conv_norm_out", c); conv("decoder.conv_out", 3, c)
    return s


BROADCAST_BUCKET_BYTES = 1 << 30
BROADCAST_ENTRY_ALIGN_BYTES = 256


def broadcast_in_buckets(entries, make, device, src: int = 0, bucket_bytes: int = None) -> dict:
    """Start-up weight broadcast of a model that is built tensor by tensor: `entries` = [(name, shape, dtype)] in an order every rank
    agrees on; rank `src` fills each tensor through `make(name, out_view)`; the tensors travel in flat per-dtype buckets of at most
    `bucket_bytes` — FLUX.1-Kontext's 24 GB are ~25 collectives instead of ~1 000 per-tensor ones (xGMI rings are per-link bound: few
    large transfers) — and every rank gets name -> view into its bucket (the views keep their bucket alive).
    gloo (CPU dry runs) stages the buckets through host memory."""
    import torch.distributed as dist
    bucket_bytes = bucket_bytes or BROADCAST_BUCKET_BYTES
    rank = dist.get_rank()
    nccl = dist.get_backend() == "nccl"
    out, groups = {}, {}
    for name, shape, dt in entries:
        groups.setdefault(dt, []).append((name, tuple(shape)))
    for dt, items in groups.items():
        esz = torch.empty((), dtype=dt).element_size()
        align = BROADCAST_ENTRY_ALIGN_BYTES // esz           # every entry starts on a 256-byte boundary of its bucket (the allocator's own granule):
        padded = lambda shape: -(-int(np.prod(shape)) // align) * align      # the GEMM / conv kernels take 16-byte vector loads and LDS-DMA from these views
        start = 0
        while start < len(items):
            end, n = start, 0
            while end < len(items) and (end == start or (n + padded(items[end][1])) * esz <= bucket_bytes):
                n += padded(items[end][1])                   # the padding counts toward the bucket size
                end += 1
            flat = torch.empty(n, dtype=dt, device=device)
            views, off = [], 0
            for name, shape in items[start:end]:
                k = int(np.prod(shape))
                views.append((name, flat[off:off + k].view(shape)))
                off += padded(shape)
            if rank == src:
                for name, v in views:
                    make(name, v)
            if nccl:
                dist.broadcast(flat, src=src)
            else:
                h = flat.cpu()
                dist.broadcast(h, src=src)
                flat.copy_(h)
            out.update(views)
            start = end
    return out


def synthetic_provider(shapes: dict, device, seed: int, broadcast: bool = False):
    """Seeded random-init parameters generated on `device` one tensor at a time (benchmarks: there is no
    checkpoint on the box).  With `broadcast` and more than one rank, rank 0 generates every tensor up front (in the order of `shapes`)
    and the set travels in flat buckets (`broadcast_in_buckets`) — the start-up weight broadcast of the page-sharded deployment."""
    gen = torch.Generator(device=device).manual_seed(seed)

    def dtype_of(name):
        return torch.bfloat16 if len(shapes[name]) >= 2 else torch.float32

    def fresh(name):
        shp = shapes[name]
        if len(shp) >= 2:
            fan = int(np.prod(shp[1:]))
            return torch.randn(shp, device=device, generator=gen, dtype=torch.float32).mul_(1.0 / math.sqrt(fan)).to(torch.bfloat16)
        if name.endswith("running_var"):
            return 0.5 + 1.5 * torch.rand(shp, device=device, generator=gen)
        if "norm" in name and name.endswith("weight"):
            return 1.0 + 0.1 * torch.randn(shp, device=device, generator=gen)
        return 0.02 * torch.randn(shp, device=device, generator=gen)

    if broadcast:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            ready = broadcast_in_buckets([(n, shapes[n], dtype_of(n)) for n in shapes], lambda n, v: v.copy_(fresh(n)), device)
            return lambda name: ready[name]
    return fresh

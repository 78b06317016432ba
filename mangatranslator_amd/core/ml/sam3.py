"""SAM 3's tracker (ViT-L image encoder with axial rotary attention + the box-prompted mask decoder) on libmtx_hip.

This is the model object behind `ModelManager.load_sam3()` (reference core/ml/model_manager.py:1012-1046 loads HF `Sam3TrackerModel` /
`Sam3TrackerProcessor` from `facebook/sam3`; the operator calls it at core/image/detection.py:1661-1666 exactly as it calls SAM-2.1).
Weights use the HF `Sam3TrackerModel.state_dict()` key names; the network followed is transformers' models/sam3/modeling_sam3.py (cited as
`hf3:<line>`) and models/sam3_tracker/modeling_sam3_tracker.py (`hft:<line>`).  Everything after the encoder — prompt embedding, two-way
decoder, stability rule, fused upsample + threshold, the pre- and post-plans and the arithmetic modes — is core/ml/sam_common.py, shared with
SAM-2.1; what is here is the trunk and the neck.

Graph design:
  * one token order from the patch embedding to the neck: WINDOW-MAJOR (windows row-major, row-major inside).  Every op but attention is
    per token; the 24 x 24 window layers read each window as a contiguous [576, C] slab; the global layers do not care about the order once
    their rotary table is permuted the same way, so window partition / unpartition (hf3:641-700) vanish.
  * patch embedding (hf3:542-638) = unpadded im2col (MTX_EW_IM2COL_PATCH, emitted in window-major order) + GEMM with the TILED position
    table as the GEMM residual, then `backbone.layer_norm`.
  * q / k / v are one [3 d, d] GEMM; the axial rotary turn (hf3:409-486) is MTX_EW_QK_ROPE in place on the q | k columns with a per-row
    cos | sin table built here (`rope_table`): window-local positions at scale 1 for window layers, raster positions times window / grid for
    global ones.  The q heads read a copy pre-multiplied by softmax scale * log2(e); the attention runs with `q_prescaled`.
  * neck (hf3:985-1053; the 0.5x level is never read by the tracker and is not built): ConvTranspose2d(k=2, s=2) = 1x1 conv + pixel-shuffle
    store; what is linear after linear is folded at load — `proj1` into the transposed conv before it, `conv_s0` / `conv_s1` (hft:1083-1084)
    into the 3x3 `proj2` before them — and each 3x3 stays a conv.  The no-mask dense prompt is folded into the level-2 bias.
"""
import math

import numpy as np
import torch

from ...hip import abi
from ...hip.plan import Act, PlanBuilder
from ...utils.exceptions import ModelError
from . import packing
from .sam_common import SamHipBase, _cfg_get, window_order

SAM3_MEAN = (0.5, 0.5, 0.5)          # IMAGENET_STANDARD_MEAN / _STD of Sam3ImageProcessorFast
SAM3_STD = (0.5, 0.5, 0.5)
LOG2E = 1.4426950408889634


def vit_hparams(config) -> dict:
    """Pull the numbers the graph needs out of an HF Sam3TrackerConfig (or an equivalent dict tree)."""
    vc = _cfg_get(config, "vision_config")
    bb = _cfg_get(vc, "backbone_config")
    pe = _cfg_get(config, "prompt_encoder_config")
    md = _cfg_get(config, "mask_decoder_config")
    img = _cfg_get(bb, "image_size")
    img = img[0] if isinstance(img, (list, tuple)) else img
    pre = _cfg_get(bb, "pretrain_image_size")
    pre = pre[0] if isinstance(pre, (list, tuple)) else pre
    return dict(
        image_size=int(img), vit_patch=int(_cfg_get(bb, "patch_size")), dim=int(_cfg_get(bb, "hidden_size")),
        heads=int(_cfg_get(bb, "num_attention_heads")), mlp=int(_cfg_get(bb, "intermediate_size")), layers=int(_cfg_get(bb, "num_hidden_layers")),
        window=int(_cfg_get(bb, "window_size")), global_layers=list(_cfg_get(bb, "global_attn_indexes")), pretrain=int(pre),
        theta=float(_cfg_get(bb, "rope_theta")), ln_eps=float(_cfg_get(bb, "layer_norm_eps")), layer_scale=_cfg_get(bb, "layer_scale_init_value"),
        act=str(_cfg_get(bb, "hidden_act", "gelu")),
        fpn_dim=int(_cfg_get(vc, "fpn_hidden_size")), scale_factors=[float(s) for s in _cfg_get(vc, "scale_factors")],
        feature_sizes=[list(s) for s in _cfg_get(vc, "backbone_feature_sizes")],
        dec_dim=int(_cfg_get(md, "hidden_size")), dec_heads=int(_cfg_get(md, "num_attention_heads")),
        dec_layers=int(_cfg_get(md, "num_hidden_layers")), dec_mlp=int(_cfg_get(md, "mlp_dim")),
        dec_down=int(_cfg_get(md, "attention_downsample_rate")),
        stab_delta=float(_cfg_get(md, "dynamic_multimask_stability_delta")),
        stab_thresh=float(_cfg_get(md, "dynamic_multimask_stability_thresh")),
        patch=int(_cfg_get(pe, "patch_size")),
    )


def rope_table(grid: int, window: int, layer_window: int, d: int, theta: float) -> torch.Tensor:
    """cos | sin rows, fp32 [grid * grid][2][d / 2], of the tokens in WINDOW-MAJOR order (windows of `window`) for one layer kind:
    `layer_window` = window for a window layer (positions inside the window, scale 1), 0 for a global layer (positions on the whole grid times
    window / grid).  Pair k < d / 4 turns by x * theta^(-4 k / d), pair k >= d / 4 by y * theta^(-4 (k - d / 4) / d) — the arithmetic of
    Sam3ViTRotaryEmbedding (hf3:415-436) term for term, so the entries equal its buffers bit for bit."""
    end = layer_window if layer_window else grid
    scale = window / end
    freqs = 1.0 / (theta ** (torch.arange(0, d, 4)[: (d // 4)].float() / d))
    flat = torch.arange(end * end, dtype=torch.long)
    xs = (flat % end) * scale
    ys = torch.div(flat, end, rounding_mode="floor") * scale
    ang = torch.cat([torch.outer(xs, freqs).float(), torch.outer(ys, freqs).float()], dim=-1)           # [end * end, d / 2], one per pair
    tab = torch.stack([ang.cos(), ang.sin()], dim=1)                                                      # [end * end, 2, d / 2]
    if layer_window:
        return tab.repeat((grid // window) ** 2, 1, 1).contiguous()
    return tab[torch.from_numpy(window_order(grid, grid, window))].contiguous()


class Sam3Hip(SamHipBase):
    NAME = "SAM 3"
    MEAN, STD = SAM3_MEAN, SAM3_STD

    def _hparams(self, config):
        if _cfg_get(config, "tracker_config") is not None:             # a Sam3VideoConfig-style tree: the tracker is one branch of it
            config = _cfg_get(config, "tracker_config")
        hp = vit_hparams(config)
        S, p, win = hp["image_size"], hp["vit_patch"], hp["window"]
        g = S // p
        if hp["layer_scale"] is not None:
            raise ModelError("SAM 3: a trunk with layer scale (layer_scale_init_value) is not built")
        if hp["act"] != "gelu":
            raise ModelError(f"SAM 3: trunk activation {hp['act']!r} is not built")
        if S % p or g % win or hp["pretrain"] % p:
            raise ModelError(f"SAM 3: a {S}-pixel input in {p}-pixel patches must give a grid that {win}-token windows tile without padding")
        if hp["dim"] % hp["heads"] or hp["dim"] // hp["heads"] not in (64, 128):
            raise ModelError("SAM 3: the trunk's head size must be 64 or 128")
        if hp["scale_factors"][:3] != [4.0, 2.0, 1.0] or hp["feature_sizes"] != [[4 * g, 4 * g], [2 * g, 2 * g], [g, g]]:
            raise ModelError("SAM 3: the neck must start with the 4x, 2x and 1x levels of the trunk's grid")
        if S // hp["patch"] != g:
            raise ModelError("SAM 3: the prompt encoder's embedding grid must be the trunk's grid")
        return hp

    def _pack(self, sd):
        hp, W = self.hp, {}
        C, g, P = hp["dim"], hp["image_size"] // hp["vit_patch"], hp["pretrain"] // hp["vit_patch"]
        pk, win = hp["vit_patch"], hp["window"]
        bbp = "vision_encoder.backbone."
        # patch embed as GEMM over im2col rows: K = p * p taps x 8 channels (3 real), no bias
        W["pe"] = (*self._cw(packing.patch_embed_rows(sd[bbp + "embeddings.patch_embeddings.projection.weight"])), None)       # [C, 3, p, p]
        # position table: the pre-training grid TILED over the input grid (hf3:588-616), stored in window-major order
        pos = sd[bbp + "embeddings.position_embeddings"].reshape(P, P, C)
        idx = torch.arange(g) % P
        pos = pos[idx][:, idx].reshape(g * g, C)
        self.order = torch.from_numpy(window_order(g, g, win))
        W["pos"] = self._c(pos[self.order])
        W["ln_pre"] = self._ln(sd, bbp + "layer_norm")
        self.layers = []
        for li in range(hp["layers"]):
            p = f"{bbp}layers.{li}."
            a = p + "attention."
            self.layers.append(dict(idx=li, win=0 if li in hp["global_layers"] else win, ln1=self._ln(sd, p + "layer_norm1"), ln2=self._ln(sd, p + "layer_norm2"),
                                    qkv=self._lin(sd, a + "q_proj", a + "k_proj", a + "v_proj"), proj=self._lin(sd, a + "o_proj"),
                                    fc1=self._lin(sd, p + "mlp.fc1"), fc2=self._lin(sd, p + "mlp.fc2")))
        # rotary tables [2][T][2][d / 2]: the plain copy (k heads), then the one the q heads read (times softmax scale * log2(e))
        d = C // hp["heads"]
        fold = (1.0 / math.sqrt(d)) * LOG2E
        self.rope = {}
        for lw in sorted({L["win"] for L in self.layers}):
            t = rope_table(g, win, lw, d, hp["theta"])
            self.rope[lw] = self._c(torch.stack([t, t * fold]), torch.float32)
        # neck: per level [transposed convs] -> proj1 (1x1) -> proj2 (3x3) [-> conv_s0 / conv_s1]
        D = hp["fpn_dim"]
        nk = "vision_encoder.neck.fpn_layers."

        def conv3(w, b, then_w=None, then_b=None, cout_round=1):
            """3x3 conv [Co, Ci, 3, 3] (+ a 1x1 conv applied right after it, folded in) in the conv kernel's packing [Co][tap][Ci]"""
            if then_w is not None:
                w, b = torch.einsum("oc,cikl->oikl", then_w, w), then_w @ b + then_b
            taps = packing.conv_taps(w, cout_round=cout_round)
            return (self._c(taps), self._c(packing.padded_bias(b, taps.shape[0]), torch.float32))

        def conv1(wt, bt, then_w=None, then_b=None):
            w, b = packing.convt2x2_as_conv1x1(wt, bt, then_w, then_b)
            return (self._c(w), self._c(b, torch.float32))

        p1 = [(sd[f"{nk}{i}.proj1.weight"].reshape(D, -1), sd[f"{nk}{i}.proj1.bias"]) for i in range(3)]
        s0 = (sd["mask_decoder.conv_s0.weight"].reshape(-1, D), sd["mask_decoder.conv_s0.bias"])
        s1 = (sd["mask_decoder.conv_s1.weight"].reshape(-1, D), sd["mask_decoder.conv_s1.bias"])
        W["n0_up1"] = conv1(sd[f"{nk}0.scale_layers.0.weight"], sd[f"{nk}0.scale_layers.0.bias"])
        W["n0_up2"] = conv1(sd[f"{nk}0.scale_layers.2.weight"], sd[f"{nk}0.scale_layers.2.bias"], *p1[0])
        W["n1_up"] = conv1(sd[f"{nk}1.scale_layers.0.weight"], sd[f"{nk}1.scale_layers.0.bias"], *p1[1])
        W["n2_p1"] = (*self._cw(p1[2][0]), self._c(p1[2][1], torch.float32))
        # what the decoder adds to the image embedding before its first layer: the no-mask dense prompt, and `no_memory_embedding` where the
        # tracker adds it to that level — hft:1007 adds it to the LAST level the neck built, which is the embedding only when the configuration
        # lists no level after the 1x one (with the shipped four scale factors it lands on the 0.5x level, which nothing reads)
        fold2 = sd["prompt_encoder.no_mask_embed.weight"].reshape(-1)
        if len(hp["scale_factors"]) == 3:
            fold2 = fold2 + sd["no_memory_embedding"].reshape(-1)
        W["n0_p2"] = conv3(sd[f"{nk}0.proj2.weight"], sd[f"{nk}0.proj2.bias"], *s0, cout_round=8)
        W["n1_p2"] = conv3(sd[f"{nk}1.proj2.weight"], sd[f"{nk}1.proj2.bias"], *s1)
        W["n2_p2"] = conv3(sd[f"{nk}2.proj2.weight"], sd[f"{nk}2.proj2.bias"] + fold2)
        self._pack_prompt_decoder(sd, W)
        if W["n0_p2"][0].shape[0] != W["upscale_conv2"][0].shape[0] // 4 or W["n1_p2"][0].shape[0] != W["upscale_conv1"][0].shape[0] // 4:
            raise ModelError("SAM 3: conv_s0 / conv_s1 do not match the mask decoder's upscaling widths")
        self.W = W

    # ------------------------------------------------------------------------------------------
    def _build_encoder(self):
        hp, W = self.hp, self.W
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        S, pk, C, heads, win = hp["image_size"], hp["vit_patch"], hp["dim"], hp["heads"], hp["window"]
        g = S // pk
        T, d, K = g * g, C // heads, pk * pk * 8
        s32 = self.stream32
        img = pb.act(1, S, S, 8)
        layer_norm, linear, close_branch = self._trunk_helpers(pb, hp["ln_eps"])
        cols = pb.buf((T, K), self.tdt)
        order = pb.hold(self.order.to(torch.int32).to(self.device))
        pb.im2col(img, cols, pk, pk, K, row_map=order, pad=False, label="patch_im2col")
        x = close_branch(cols, W["pe"], T, C, K, pb.const(W["pos"].float()) if s32 else W["pos"], "patch_embed")
        # `backbone.layer_norm` opens the residual stream (hf3:842): in the stream's own type
        if s32:
            x = pb.norm(x, pb.buf((T, C), torch.float32), T, C, gamma=W["ln_pre"][0], beta=W["ln_pre"][1], eps=hp["ln_eps"], dtype=abi.F32, label="ln_pre")
        else:
            x = pb.norm(x, pb.buf((T, C), self.tdt), T, C, gamma=W["ln_pre"][0], beta=W["ln_pre"][1], eps=hp["ln_eps"], label="ln_pre")
        for L in self.layers:
            tag = f"layer{L['idx']}"
            wtok = L["win"] * L["win"] if L["win"] else T
            nwin = T // wtok
            ln1 = layer_norm(x, T, C, L["ln1"], tag + ".ln1")
            qkv = linear(ln1, L["qkv"], T, 3 * C, C, tag + ".qkv")
            pb.qk_rope(Act(qkv.view(1, 1, T, 3 * C), 1, 1, T, 2 * C), self.rope[L["win"]], d, q_heads=heads, ld_cs=T * d, label=tag + ".rope")
            o = pb.buf((T, C), self.tdt)
            st = (wtok * 3 * C, 3 * C, d)
            pb.attention(qkv, qkv, qkv, o, nwin, heads, wtok, wtok, d, st, st, st, (wtok * C, C, d), 1.0 / math.sqrt(d),
                         k_off=C, v_off=2 * C, q_prescaled=True, label=tag + ".attn")
            x1 = close_branch(o, L["proj"], T, C, C, x, tag + ".proj")
            ln2 = layer_norm(x1, T, C, L["ln2"], tag + ".ln2")
            h = linear(ln2, L["fc1"], T, hp["mlp"], C, tag + ".fc1", act=abi.ACT_GELU)
            x = close_branch(h, L["fc2"], T, C, hp["mlp"], x1, tag + ".fc2")
        # ---- neck -------------------------------------------------------------------------------------
        D = hp["fpn_dim"]
        if s32:                     # the trunk's output is the fp32 stream: rounded once, to the neck's operand type
            x = pb.cvt16(x, pb.buf((T, C), self.tdt), T, C, copies=1, label="neck.cvt")
        to_raster = pb.hold(self._gather_map(g, g, win, 0))
        xr = pb.act(1, g, g, C)
        pb.row_gather(x, xr.t, to_raster, T, C, label="neck.to_raster")

        def up(xa, wb, act, label):
            return pb.conv2d(xa, wb[0], wb[1], wb[0].shape[0], ksize=1, pixel_shuffle=2, act=act, label=label)

        def conv3(xa, wb, label):
            return pb.conv2d(xa, wb[0], wb[1], wb[0].shape[0], ksize=3, label=label)

        t0 = up(up(xr, W["n0_up1"], abi.ACT_GELU, "neck0.up1_gelu"), W["n0_up2"], abi.ACT_NONE, "neck0.up2_proj1")
        feat_s0 = conv3(t0, W["n0_p2"], "neck0.proj2_s0")
        feat_s1 = conv3(up(xr, W["n1_up"], abi.ACT_NONE, "neck1.up_proj1"), W["n1_p2"], "neck1.proj2_s1")
        l2 = pb.act(1, g, g, D)
        linear(xr.t, W["n2_p1"], T, D, C, "neck2.proj1", out=l2.t)
        src = conv3(l2, W["n2_p2"], "neck2.proj2")
        plan = pb.build()
        plan.img, plan.feat_s0, plan.feat_s1, plan.src = img, feat_s0, feat_s1, src
        return plan

"""SAM-2.1 (Hiera image encoder + box-prompted mask decoder) on libmtx_hip.

This is the model object behind `ModelManager.load_sam2()` (reference
core/ml/model_manager.py:982-1010 loads HF `Sam2Model`/`Sam2Processor`; the operator
`_process_simple_bubbles`, reference core/image/detection.py:475-511, calls
processor -> model(multimask_output=False) -> post_process_masks -> boolean masks).
Weights use the HF `Sam2Model.state_dict()` key names; the network definition followed is
transformers' modeling_sam2.py (cited per function below as `hf:<line>`).

Everything after the encoder (and the model object's public surface) is `SamHipBase`, core/ml/sam_common.py, shared with SAM 3; this file
holds the Hiera trunk and its neck.

Graph design (MI355X-first):
  * tokens are kept in WINDOW-MAJOR order for a whole Hiera stage: every op except attention is
    per-token, global attention is permutation-equivariant, so window partition / unpartition
    (hf:397-452) vanish — attention reads each window as a contiguous [ws*ws, C] slab through
    strides.  Layouts change only where the window size does (one row-gather per change).
  * patch embedding = im2col (emitted directly in window-major order) + GEMM with the
    bicubic-interpolated position table fused as the GEMM residual (hf:106-137, 638-644).
  * q-pooling = NHWC 2x2 max-pool over [windows, ws, ws, C] views (hf:295-303, 337-341).
  * FPN neck 1x1 convs are GEMMs; conv_s0/conv_s1 (hf:1608-1609) are folded into the level-0/1
    lateral convs at load time (two chained linear maps), no_memory_embedding and the
    no-mask dense prompt are folded into the level-2 bias.
  * mask decoder: k/q projections of (keys + image PE) are split as W*keys + (W*PE): the PE part is
    a per-layer constant table fused as a batch-broadcast GEMM residual.  ConvTranspose2d(k=2,s=2)
    = 1x1 conv + pixel-shuffle store addressing.  Mask logits stay fp32; the stability rule
    (hf:1265-1311) picks a channel per box on the device and the bilinear upsample to page size is
    fused with the > 0 threshold, writing the page-resolution bitmask directly.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ...hip import abi
from ...hip.plan import Act, PlanBuilder
from ...utils.exceptions import ModelError
from . import packing
from .sam_common import SamHipBase, _cfg_get, window_order      # noqa: F401  (window_order is part of this module's surface)

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def hiera_hparams(config) -> dict:
    """Pull the numbers the graph needs out of an HF Sam2Config (or an equivalent dict tree)."""
    vc = _cfg_get(config, "vision_config")
    bb = _cfg_get(vc, "backbone_config")
    pe = _cfg_get(config, "prompt_encoder_config")
    md = _cfg_get(config, "mask_decoder_config")
    img = _cfg_get(bb, "image_size")
    img = img[0] if isinstance(img, (list, tuple)) else img
    return dict(
        image_size=int(img), embed=list(_cfg_get(bb, "embed_dim_per_stage")), blocks=list(_cfg_get(bb, "blocks_per_stage")),
        heads=list(_cfg_get(bb, "num_attention_heads_per_stage")), windows=list(_cfg_get(bb, "window_size_per_stage")),
        global_blocks=list(_cfg_get(bb, "global_attention_blocks")), q_pool_stages=int(_cfg_get(bb, "num_query_pool_stages")),
        mlp_ratio=float(_cfg_get(bb, "mlp_ratio")), ln_eps=float(_cfg_get(bb, "layer_norm_eps")),
        fpn_dim=int(_cfg_get(vc, "fpn_hidden_size")), top_down=list(_cfg_get(vc, "fpn_top_down_levels")),
        dec_dim=int(_cfg_get(md, "hidden_size")), dec_heads=int(_cfg_get(md, "num_attention_heads")),
        dec_layers=int(_cfg_get(md, "num_hidden_layers")), dec_mlp=int(_cfg_get(md, "mlp_dim")),
        dec_down=int(_cfg_get(md, "attention_downsample_rate")),
        stab_delta=float(_cfg_get(md, "dynamic_multimask_stability_delta")),
        stab_thresh=float(_cfg_get(md, "dynamic_multimask_stability_thresh")),
        patch=int(_cfg_get(pe, "patch_size")),
    )


class Sam2Hip(SamHipBase):
    NAME = "SAM-2"
    MEAN, STD = IMAGENET_MEAN, IMAGENET_STD

    def _hparams(self, config):
        return hiera_hparams(config)

    def _pack(self, sd):
        hp, W = self.hp, {}
        S = hp["image_size"]
        g0 = S // 4
        C0 = hp["embed"][0]
        bbp = "vision_encoder.backbone."
        # patch embed as GEMM over im2col rows: K = 49 taps x 8 channels (3 real)
        W["pe"] = (*self._cw(packing.patch_embed_rows(sd[bbp + "patch_embed.projection.weight"])),          # [C0, 3, 7, 7] -> [C0, 392]
                   self._c(sd[bbp + "patch_embed.projection.bias"], torch.float32))
        # position table (hf:638-644), stored in the first stage's window-major order
        pos = F.interpolate(sd[bbp + "pos_embed"], size=(g0, g0), mode="bicubic")
        win = sd[bbp + "pos_embed_window"]
        pos = pos + win.tile([1, 1, g0 // win.shape[2], g0 // win.shape[3]])
        pos = pos[0].permute(1, 2, 0).reshape(g0 * g0, C0)
        order0 = torch.from_numpy(window_order(g0, g0, hp["windows"][0]))
        W["pos"] = self._c(pos[order0])
        # blocks
        self.blocks = []
        total = 0
        for si, nb in enumerate(hp["blocks"]):
            for bi in range(nb):
                p = f"{bbp}blocks.{total}."
                dim = hp["embed"][si - 1] if (si > 0 and bi == 0) else hp["embed"][si]
                dim_out = hp["embed"][si]
                win_sz = hp["windows"][si - 1] if (si > 0 and bi == 0) else hp["windows"][si]
                if total in hp["global_blocks"]:
                    win_sz = 0
                pool = 0 < si <= hp["q_pool_stages"] and bi == 0
                blk = dict(dim=dim, dim_out=dim_out, win=win_sz, pool=pool, heads=hp["heads"][si], idx=total,
                           stage_end=(bi == nb - 1))
                for nm in ("layer_norm1", "layer_norm2"):
                    blk[nm] = self._ln(sd, p + nm)
                for nm, key in (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("fc1", "mlp.proj_in"), ("fc2", "mlp.proj_out")):
                    blk[nm] = self._lin(sd, p + key)
                    blk[nm + "_n"] = sd[p + key + ".weight"].shape[0]
                if dim != dim_out:
                    blk["skip"] = self._lin(sd, p + "proj")
                self.blocks.append(blk)
                total += 1
        # neck (hf:216-265): convs[n-i] serves level i; levels 0/1 are folded with conv_s0/conv_s1
        n = len(hp["embed"]) - 1
        D = hp["fpn_dim"]
        lat = {}
        for i in range(n + 1):
            lat[i] = (sd[f"vision_encoder.neck.convs.{n - i}.weight"].reshape(D, -1), sd[f"vision_encoder.neck.convs.{n - i}.bias"])
        ws0, bs0 = sd["mask_decoder.conv_s0.weight"].reshape(-1, D), sd["mask_decoder.conv_s0.bias"]
        ws1, bs1 = sd["mask_decoder.conv_s1.weight"].reshape(-1, D), sd["mask_decoder.conv_s1.bias"]
        W["neck0"] = (*self._cw(ws0 @ lat[0][0]), self._c(ws0 @ lat[0][1] + bs0, torch.float32))
        W["neck1"] = (*self._cw(ws1 @ lat[1][0]), self._c(ws1 @ lat[1][1] + bs1, torch.float32))
        fold = sd["no_memory_embedding"].reshape(-1) + sd["prompt_encoder.no_mask_embed.weight"].reshape(-1)
        if 2 in hp["top_down"]:
            W["neck2"] = (*self._cw(lat[2][0]), self._c(lat[2][1] + fold, torch.float32))
            W["neck3"] = (*self._cw(lat[3][0]), self._c(lat[3][1], torch.float32))
        else:
            W["neck2"] = (*self._cw(lat[2][0]), self._c(lat[2][1] + fold, torch.float32))
            W["neck3"] = None
        self._pack_prompt_decoder(sd, W)
        self.W = W

    def _build_encoder(self):
        hp, W = self.hp, self.W
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        S = hp["image_size"]
        g = S // 4
        img = pb.act(1, S, S, 8)
        C0 = hp["embed"][0]
        win0 = hp["windows"][0]
        T = g * g
        # "hilo": every trunk / neck linear carries its weight pair (w, w_lo, bias) — one launch, one operand.  "stream32": the residual stream x
        # stays fp32 from the patch embedding to the neck — the projections that close a branch (attn.proj, mlp.proj_out) take the fp32 residual
        # in their epilogue and write fp32; the LayerNorms read fp32 and round once, to the storage type of the GEMM that follows.  Measured on
        # the fp32 oracle with the roundings injected (Hiera-L): with hi + lo weights the stream's 96 roundings are 90 % of what
        # is left of the trunk's error.  Neither part adds a launch to the "fast" op list (round 5's form added six per block).
        s32 = self.stream32
        f32 = torch.float32

        cols = pb.buf((T, 392), self.tdt)
        order0 = pb.hold(torch.from_numpy(window_order(g, g, win0).astype(np.int32)).to(self.device))
        pb.im2col(img, cols, 7, 4, 392, row_map=order0, label="patch_im2col")
        eps = hp["ln_eps"]
        layer_norm, linear, close_branch = self._trunk_helpers(pb, eps)
        x = close_branch(cols, W["pe"], T, C0, 392, pb.const(W["pos"].float()) if s32 else W["pos"], "patch_embed")
        layout, hs = win0, g
        feats = {}
        stage = 0
        for blk in self.blocks:
            dim, dout, heads = blk["dim"], blk["dim_out"], blk["heads"]
            d = dout // heads
            win = blk["win"]
            tag = f"blk{blk['idx']}"
            if win and win != layout:
                m = pb.hold(self._gather_map(hs, hs, layout, win))
                x = pb.row_gather(x, pb.buf((T, dim), f32 if s32 else self.tdt), m, T, dim, label=tag + ".relayout", dtype=abi.F32 if s32 else None)
                layout = win
            ln1 = layer_norm(x, T, dim, blk["layer_norm1"], tag + ".ln1")
            qkv = linear(ln1, blk["qkv"], T, 3 * dout, dim, tag + ".qkv")
            wtok = win * win if win else T
            nwin = T // wtok
            if dim != dout and not blk["pool"]:
                raise ModelError("SAM-2: a channel change without q-pooling is not built")
            if blk["pool"]:
                if not win:
                    raise ModelError("SAM-2: q-pooling inside a global-attention block is not supported")
                res_full = linear(ln1, blk["skip"], T, dout, dim, tag + ".skip")
                res = pb.ew(abi.EW_MAXPOOL, Act(res_full.view(nwin, win, win, dout), nwin, win, win, dout), i0=2, i1=2, label=tag + ".skip_pool")
                qv = Act(qkv.view(nwin, win, win, 3 * dout), nwin, win, win, dout, 0)
                qp = pb.ew(abi.EW_MAXPOOL, qv, i0=2, i1=2, label=tag + ".q_pool")
                Tq, sq = T // 4, wtok // 4
                q_t, q_str = qp.t, (sq * dout, dout, d)
                res_t = pb.cvt_f32(res, self.dtype, label=tag + ".skip_f32").t.view(Tq, dout) if s32 else res.t
            else:
                Tq, sq = T, wtok
                q_t, q_str = qkv, (wtok * 3 * dout, 3 * dout, d)
                res_t = x
            o = pb.buf((Tq, dout), self.tdt)
            kv_str = (wtok * 3 * dout, 3 * dout, d)
            pb.attention(q_t, qkv, qkv, o, nwin, heads, sq, wtok, d, q_str, kv_str, kv_str, (sq * dout, dout, d),
                         1.0 / math.sqrt(d), k_off=dout, v_off=2 * dout, label=tag + ".attn")
            x1 = close_branch(o, blk["proj"], Tq, dout, dout, res_t, tag + ".proj")
            ln2 = layer_norm(x1, Tq, dout, blk["layer_norm2"], tag + ".ln2")
            hdim = blk["fc1_n"]
            h = linear(ln2, blk["fc1"], Tq, hdim, dout, tag + ".fc1", act=abi.ACT_GELU)
            x = close_branch(h, blk["fc2"], Tq, dout, hdim, x1, tag + ".fc2")
            if blk["pool"]:
                T, hs, layout = Tq, hs // 2, win // 2
            if blk["stage_end"]:
                feats[stage] = (x, T, hs, layout, dout)
                stage += 1
        # ---- neck ---------------------------------------------------------------------------------
        D = hp["fpn_dim"]

        def lateral(level, wb, cout):
            xt, Tn, hn, lay, cin = feats[level]
            if s32:                 # the stage output is the fp32 stream: rounded once, to the lateral projection's operand type
                xt = pb.cvt16(xt, pb.buf((Tn, cin), self.tdt), Tn, cin, copies=1, label=f"neck{level}.cvt")
            y = linear(xt, wb, Tn, cout, cin, f"neck{level}")
            m = pb.hold(self._gather_map(hn, hn, lay, 0))
            r = pb.act(1, hn, hn, cout)
            pb.row_gather(y, r.t, m, Tn, cout, label=f"neck{level}.to_raster")
            return r

        c0 = W["neck0"][0].shape[0]
        c1 = W["neck1"][0].shape[0]
        feat_s0 = lateral(0, W["neck0"], c0)
        feat_s1 = lateral(1, W["neck1"], c1)
        lat2 = lateral(2, W["neck2"], D)
        if W["neck3"] is not None:
            lat3 = lateral(3, W["neck3"], D)
            src = pb.ew(abi.EW_UPSAMPLE2X, lat3, b=lat2, label="fpn_top_down")
        else:
            src = lat2
        plan = pb.build()
        plan.img, plan.feat_s0, plan.feat_s1, plan.src = img, feat_s0, feat_s1, src
        return plan


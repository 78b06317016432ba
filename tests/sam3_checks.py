"""SAM 3 parity: libmtx_hip graph vs HF transformers Sam3TrackerModel on CPU fp32, and MTX_EW_QK_ROPE vs its formula.

The oracle is the reference's own third-party implementation (transformers' `Sam3TrackerModel`, what the reference loads from
`facebook/sam3`), run on CPU fp32 with seeded weights; the network is NOT restated.  Two small pieces around it ARE, because
`Sam3TrackerProcessor` needs torchvision, which is absent: `preprocess` (resize to S x S with antialiased bilinear on uint8 levels, / 255,
mean = std = 0.5; boxes scaled by S / W, S / H — PARITY UNPINNED for the rounding of the uint8 resize, as for SAM-2) and the post-processing
(bilinear align_corners=False to page size, > 0), which is `oracle.sam2_ref.post_process` unchanged.

`check_sam3` IS `sam2_checks.check_sam2` — same statements, same bounds — pointed at this oracle and at `Sam3Hip`.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import sam2_checks as sc
from mangatranslator_amd.core.ml.sam3 import Sam3Hip
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act, PlanBuilder
from oracle import sam2_ref

stats = sc.stats
last = sc.last


def make_config(size: str = "tiny"):
    from transformers import Sam3TrackerConfig
    from transformers.models.sam3.configuration_sam3 import Sam3VisionConfig, Sam3ViTConfig
    from transformers.models.sam3_tracker.configuration_sam3_tracker import Sam3TrackerMaskDecoderConfig, Sam3TrackerPromptEncoderConfig
    if size == "tiny":         # 8 x 8 grid, four 16-token windows, a tiled 4 x 4 position table; the neck ends at the 1x level, so that
        # `no_memory_embedding` reaches the image embedding (with the shipped four levels the tracker adds it to the unread 0.5x level)
        bb = Sam3ViTConfig(hidden_size=128, num_attention_heads=2, intermediate_size=296, num_hidden_layers=4, global_attn_indexes=[1, 3],
                           image_size=112, patch_size=14, pretrain_image_size=56, window_size=4)
        vc = Sam3VisionConfig(backbone_config=bb, fpn_hidden_size=32, backbone_feature_sizes=[[32, 32], [16, 16], [8, 8]], scale_factors=[4.0, 2.0, 1.0])
        return Sam3TrackerConfig(vision_config=vc, prompt_encoder_config=Sam3TrackerPromptEncoderConfig(hidden_size=32, image_size=112, patch_size=14),
                                 mask_decoder_config=Sam3TrackerMaskDecoderConfig(hidden_size=32, mlp_dim=64, num_attention_heads=2, iou_head_hidden_dim=32))
    if size == "real_dims":    # the shipped widths (1024 / 16 heads / 4736, window 24, fpn 256, default decoder, four neck levels) at 8 layers and a
        # 672-pixel input: 48 x 48 grid, 4 windows of 576 tokens, global attention over 2304 tokens, a tiled 24 x 24 position table
        bb = Sam3ViTConfig(num_hidden_layers=8, global_attn_indexes=[3, 7], image_size=672, pretrain_image_size=336)
        vc = Sam3VisionConfig(backbone_config=bb, backbone_feature_sizes=[[192, 192], [96, 96], [48, 48]])
        return Sam3TrackerConfig(vision_config=vc, prompt_encoder_config=Sam3TrackerPromptEncoderConfig(image_size=672),
                                 mask_decoder_config=Sam3TrackerMaskDecoderConfig())
    raise ValueError(size)


def make_model(size: str = "tiny", seed: int = 0):
    """HF Sam3TrackerModel with seeded weights.  `no_memory_embedding` initialises to zero and is re-seeded so that its path is exercised."""
    from transformers import Sam3TrackerModel
    torch.manual_seed(seed)
    cfg = make_config(size)
    m = Sam3TrackerModel(cfg).eval().float()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.no_memory_embedding.copy_(torch.randn(m.no_memory_embedding.shape, generator=g) * 0.02)
        for name, p in m.named_parameters():      # widen the default init so signals survive the trunk (as oracle/sam2_ref.py does)
            if p.dim() >= 2 and "embed" not in name:
                p.mul_(2.0)
    return m, cfg


def preprocess(page_u8: np.ndarray, boxes_xyxy: np.ndarray, size: int):
    h, w, _ = page_u8.shape
    x = torch.from_numpy(np.ascontiguousarray(page_u8)).permute(2, 0, 1)[None]
    x = F.interpolate(x, (size, size), mode="bilinear", antialias=True, align_corners=False)
    x = (x.float() / 255.0 - 0.5) / 0.5
    b = torch.as_tensor(boxes_xyxy, dtype=torch.float32).clone().reshape(-1, 2, 2)
    b[..., 0] = b[..., 0] * (size / w)
    b[..., 1] = b[..., 1] * (size / h)
    return x, b.reshape(1, -1, 4)


@torch.no_grad()
def run(model, page_u8: np.ndarray, boxes_xyxy: np.ndarray):
    size = model.config.prompt_encoder_config.image_size
    pv, ib = preprocess(page_u8, boxes_xyxy, size)
    out = model(pixel_values=pv, input_boxes=ib, multimask_output=False)
    h, w, _ = page_u8.shape
    return dict(pred_masks=out.pred_masks, iou_scores=out.iou_scores, masks=sam2_ref.post_process(out.pred_masks, h, w), pixel_values=pv, input_boxes=ib)


_shared = {"models": {}, "runs": {}, "gains": {}}


def _calibration_key(model):
    return float(model.mask_decoder.output_hypernetworks_mlps[0].proj_out.weight.detach().double().abs().sum())


class _Oracle:
    """what `check_sam2` asks of `oracle.sam2_ref`: make_model(size, seed) and run(model, page, boxes)"""
    make_model, run = staticmethod(make_model), staticmethod(run)


class _SharedOracle:
    """the same, for tests that compare several arithmetic modes with ONE seeded model: the model is built once per (size, seed) and a forward
    pass is computed once per (model state, page, boxes).  A pass `check_sam2` spies on (its calibrated second pass) always runs: the spy's
    capture is what the check reads."""

    @staticmethod
    def make_model(size, seed):
        if (size, seed) not in _shared["models"]:
            _shared["models"][(size, seed)] = make_model(size, seed)
        return _shared["models"][(size, seed)]

    @staticmethod
    def run(model, page_u8, boxes_xyxy):
        key = (id(model), _calibration_key(model), page_u8.tobytes(), np.asarray(boxes_xyxy).tobytes())
        spied = "_dynamic_multimask_via_stability" in vars(model.mask_decoder)
        if spied or key not in _shared["runs"]:
            _shared["runs"][key] = run(model, page_u8, boxes_xyxy)
        return _shared["runs"][key]


_calibrate_logits = sc.calibrate_logits


def _calibrate_once(model, ref, target_std=5.0):
    """`sam2_checks.calibrate_logits` for a shared model: applied the first time, and only then — every mode is compared on the same weights"""
    if id(model) not in _shared["gains"]:
        _shared["gains"][id(model)] = _calibrate_logits(model, ref, target_std)
    return _shared["gains"][id(model)]


@contextlib.contextmanager
def _pointed_at_sam3(oracle):
    old = sc.sr, sc.Sam2Hip, sc.calibrate_logits
    sc.sr, sc.Sam2Hip = oracle, Sam3Hip
    if oracle is _SharedOracle:
        sc.calibrate_logits = _calibrate_once
    try:
        yield
    finally:
        sc.sr, sc.Sam2Hip, sc.calibrate_logits = old


def check_sam3(lib, device, size="tiny", share_oracle=False, **kw):
    """`sam2_checks.check_sam2` (its arguments, statements and default bounds: low-res logits rel err < 0.08, page-mask mismatch < 1 %, no pixel
    wrong outside the measured error band, and with `calibrated` the decisive stability choices) on Sam3Hip against HF Sam3TrackerModel"""
    with _pointed_at_sam3(_SharedOracle if share_oracle else _Oracle):
        return sc.check_sam2(lib, device, size, **kw)


# ---- MTX_EW_QK_ROPE ---------------------------------------------------------------------------------------------------------------------
_TDT = {abi.BF16: torch.bfloat16, abi.F16: torch.float16}
_ULP = {abi.BF16: 2.0 ** -7, abi.F16: 2.0 ** -10}          # one unit in the last place of a value in [1, 2)


def run_qk_rope(lib, device, dtype, qkv, cs, heads, d, q_table=True):
    """the op through PlanBuilder.qk_rope, in place on the q | k columns of a [rows, 3 * heads * d] buffer; cs = fp32 [2][rows][2][d / 2] (plain
    copy, then the q heads' copy) -> the buffer after the launch"""
    rows = qkv.shape[0]
    pb = PlanBuilder(lib, device, dtype)
    buf = pb.const(qkv.to(_TDT[dtype]))
    tab = pb.const(cs.float())
    pb.qk_rope(Act(buf.view(1, 1, rows, 3 * heads * d), 1, 1, rows, 2 * heads * d), tab, d, q_heads=heads if q_table else 0, ld_cs=rows * d if q_table else 0)
    pb.build().run()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return buf.float().cpu()


def rope_formula(qkv_f32, cs, heads, d):
    """fp32: (x0, x1) -> (x0 c - x1 s, x1 c + x0 s) per interleaved pair; q heads with table copy 1, k heads with copy 0, v untouched"""
    rows = qkv_f32.shape[0]
    x = qkv_f32.clone().view(rows, 3, heads, d // 2, 2)
    out = x.clone()
    for part, copy in ((0, 1), (1, 0)):
        c, s = cs[copy][:, 0][:, None, :], cs[copy][:, 1][:, None, :]                   # [rows, 1, d / 2]
        x0, x1 = x[:, part, :, :, 0], x[:, part, :, :, 1]
        out[:, part, :, :, 0] = x0 * c - x1 * s
        out[:, part, :, :, 1] = x1 * c + x0 * s
    return out.view(rows, 3 * heads * d)


def check_qk_rope_exact(lib, device, dtype, d, rows=5, heads=3, seed=0):
    """table entries from {0, +-1, +-0.5} and small-integer q / k: every product and sum is exact in fp32 and representable in the storage type,
    so the result must equal the formula BIT FOR BIT; the v slice holds a sentinel that must come back untouched"""
    g = torch.Generator().manual_seed(seed + d)
    vals = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5])
    cs = vals[torch.randint(0, 5, (2, rows, 2, d // 2), generator=g)]
    qkv = torch.randint(-8, 9, (rows, 3 * heads * d), generator=g).float()
    qkv[:, 2 * heads * d:] = 77.0
    want = rope_formula(qkv, cs, heads, d)
    assert torch.equal(want, want.to(_TDT[dtype]).float())                                  # the test's own premise: nothing to round
    assert not torch.equal(cs[0], cs[1])
    got = run_qk_rope(lib, device, dtype, qkv, cs, heads, d)
    assert torch.equal(got[:, 2 * heads * d:], qkv[:, 2 * heads * d:]), "the v slice was touched"
    assert torch.equal(got, want), f"qk_rope exact d={d}: {(got != want).sum().item()} values differ"


def check_qk_rope_random(lib, device, dtype, d, rows=37, heads=2, seed=0):
    """random q / k and angles: within 1 ulp of the storage type of `apply_rotary_pos_emb_2d`'s fp32 result rounded once (the kernel and torch
    may contract x0 c - x1 s differently: a last-bit difference in fp32 can move the rounded value by one step, not more)"""
    from transformers.models.sam3.modeling_sam3 import apply_rotary_pos_emb_2d
    g = torch.Generator().manual_seed(seed + d)
    ang = torch.rand(rows, d // 2, generator=g) * 6.28
    tab = torch.stack([ang.cos(), ang.sin()], 1)
    cs = torch.stack([tab, tab])                                                            # both copies plain: the HF function knows one table
    tdt = _TDT[dtype]
    qkv = torch.randn(rows, 3 * heads * d, generator=g).to(tdt).float()
    x = qkv.view(rows, 3, heads, d)
    cos, sin = ang.cos().repeat_interleave(2, -1), ang.sin().repeat_interleave(2, -1)       # [rows, d], Sam3ViTRotaryEmbedding's layout
    q_ref, k_ref = apply_rotary_pos_emb_2d(x[:, 0].transpose(0, 1)[None], x[:, 1].transpose(0, 1)[None], cos=cos, sin=sin)     # [1, heads, rows, d]
    want = torch.stack([q_ref[0].transpose(0, 1), k_ref[0].transpose(0, 1)], 1).reshape(rows, 2 * heads * d).to(tdt).float()
    got = run_qk_rope(lib, device, dtype, qkv, cs, heads, d)
    assert torch.equal(got[:, 2 * heads * d:], qkv[:, 2 * heads * d:])
    got = got[:, :2 * heads * d]
    ulp = torch.maximum(torch.abs(want), torch.full_like(want, 2.0 ** -14)).log2().floor().exp2() * _ULP[dtype]
    worst = ((got - want).abs() / ulp).max().item()
    assert worst <= 1.0, f"qk_rope random d={d}: {worst} ulp"

"""CPU tier: SAM 3 on the kernel simulator — the rotary op against its formula, the host's rotary tables against transformers' buffers, the
whole graph (pre-process, ViT trunk, neck, two-way mask decoder, stability selection, fused upsample + threshold) against HF transformers'
Sam3TrackerModel on CPU fp32 (the reference's own third-party implementation), and the manager / operator path."""
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import sam3_checks as s3
from mangatranslator_amd.hip import abi

DTYPES = [pytest.param(abi.BF16, id="bf16"), pytest.param(abi.F16, id="f16")]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qk_rope_exact(emu_lib, dtype, d):
    """5 rows (not a multiple of the kernel's 4 rows per thread), 3 heads, row stride 3 * heads * d with a sentinel in the v slice: bit for bit"""
    s3.check_qk_rope_exact(emu_lib, "cpu", dtype, d)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qk_rope_random(emu_lib, dtype, d):
    s3.check_qk_rope_random(emu_lib, "cpu", dtype, d)


def test_rope_tables_equal_transformers_buffers():
    """the host's cos | sin rows of a window layer and of a global layer, tokens in window-major order, are `Sam3ViTRotaryEmbedding`'s buffers
    (one entry per interleaved pair) permuted — to fp32 equality"""
    from transformers.models.sam3.modeling_sam3 import Sam3ViTRotaryEmbedding
    from mangatranslator_amd.core.ml.sam3 import rope_table
    from mangatranslator_amd.core.ml.sam_common import window_order
    cfg = s3.make_config("real_dims").vision_config.backbone_config
    grid, win, d = 48, cfg.window_size, cfg.hidden_size // cfg.num_attention_heads
    order = torch.from_numpy(window_order(grid, grid, win))
    for lw, end in ((win, win), (0, grid)):
        hf = Sam3ViTRotaryEmbedding(cfg, end_x=end, end_y=end, scale=cfg.window_size / end)
        cos, sin = hf.rope_embeddings_cos[:, 0::2], hf.rope_embeddings_sin[:, 0::2]                 # [end * end, d / 2]
        assert torch.equal(cos, hf.rope_embeddings_cos[:, 1::2])
        want = torch.stack([cos, sin], 1)
        want = want.repeat((grid // win) ** 2, 1, 1) if lw else want[order]
        got = rope_table(grid, win, lw, d, cfg.rope_theta)
        assert got.dtype == torch.float32 and got.shape == (grid * grid, 2, d // 2) and torch.equal(got, want)
    # window-major row 600 is the token 24 places into the second window: local (x, y) = (0, 1) at scale 1, raster (24, 1) at scale 1 / 2
    assert order[600].item() == 1 * 48 + 24
    assert torch.equal(rope_table(grid, win, win, d, cfg.rope_theta)[600, 0, :d // 4], torch.ones(d // 4))          # x = 0: cos 1


def test_sam3_tiny(emu_lib):
    err, mism = s3.check_sam3(emu_lib, "cpu", "tiny", h=300, w=200, n_boxes=3, seed=0)


def test_sam3_tiny_one_box_landscape(emu_lib):
    s3.check_sam3(emu_lib, "cpu", "tiny", h=120, w=260, n_boxes=1, seed=3)


def test_sam3_tiny_high_precision(emu_lib):
    """precision "high" with f16 storage and logits at a trained model's spread: no decided pixel wrong, and a logit rms below "fast"'s"""
    s3.check_sam3(emu_lib, "cpu", "tiny", h=300, w=200, n_boxes=3, seed=0, dtype=abi.F16, calibrated=True)
    fast = s3.stats["logit_abs_err_rms"]
    s3.check_sam3(emu_lib, "cpu", "tiny", h=300, w=200, n_boxes=3, seed=0, dtype=abi.F16, calibrated=True, precision="high")
    assert s3.stats["logit_abs_err_rms"] < fast, (fast, s3.stats["logit_abs_err_rms"])
    assert s3.stats["decided_pixels_wrong"] == 0 and s3.stats["wrong_beyond_1_logit"] == 0


def test_layer_scale_is_refused():
    from mangatranslator_amd.core.ml.sam3 import Sam3Hip
    from mangatranslator_amd.utils.exceptions import ModelError
    cfg = s3.make_config("tiny")
    cfg.vision_config.backbone_config.layer_scale_init_value = 0.1
    with pytest.raises(ModelError, match="layer scale"):
        Sam3Hip({}, cfg, device="cpu", lib=types.SimpleNamespace(is_simulator=True))


@pytest.mark.parametrize("layout", ["plain", "prefixed"])
def test_manager_loads_sam3_and_the_operator_uses_it(emu_lib, tmp_path, monkeypatch, layout):
    """reference model_manager.py:1012-1046 / detection.py:1661-1666: a staged checkpoint (`Sam3TrackerModel.state_dict()` names, bare or under
    `tracker_model.` beside a `detector_model.` key) loads as the (processor, model) pair, and `detect_speech_bubbles(seg_model="sam3")` returns
    its masks — not the detector's, and never SAM 2.1's"""
    from PIL import Image
    from safetensors.torch import save_file
    import mangatranslator_amd.hip.lib as libmod
    from mangatranslator_amd.core.image import detection
    from mangatranslator_amd.core.ml import model_manager as mm
    from mangatranslator_amd.utils.exceptions import ModelError
    from test_detection_flow import _Boxes, _Model
    monkeypatch.setattr(libmod, "_lib", emu_lib)
    monkeypatch.setattr(mm, "_model_manager", None)
    monkeypatch.setattr(mm.ModelManager, "_instance", None)
    m = mm.get_model_manager()
    try:
        root = tmp_path / "sam3"
        m.model_paths[mm.ModelType.SAM3] = root
        with pytest.raises(ModelError):
            m.load_sam3(token="x")                                   # nothing staged: the contract the page flow's fallback rests on
        model, cfg = s3.make_model("tiny", 0)
        cfg.save_pretrained(str(root))
        sd = {k: v.contiguous() for k, v in model.state_dict().items()}
        if layout == "prefixed":
            sd = {"tracker_model." + k: v for k, v in sd.items()}
            sd["detector_model.x"] = torch.zeros(3)
            sd["tracker_model.memory_encoder.y"] = torch.zeros(3)
        save_file(sd, str(root / "model.safetensors"))
        proc, shim = m.load_sam3()
        assert shim.hip.NAME == "SAM 3" and shim.hip.dtype == abi.F16 and shim.hip.high and m.is_loaded(mm.ModelType.SAM3)
        assert m.load_sam3()[1] is shim
        with m.front_replica(1):
            assert m.load_sam3()[1].hip.high and m.load_sam3()[1] is not shim

        H, W = 240, 300
        boxes = [[20.0, 30.0, 190.0, 120.0], [210.0, 20.0, 290.0, 90.0]]
        pm = _Model(types.SimpleNamespace(boxes=_Boxes(boxes, [0.9, 0.8], [0, 0]), masks=None, orig_shape=(H, W)), {0: "speech_bubble"})

        def boom(*a, **k):
            raise RuntimeError("not staged")

        def sam2(*a, **k):
            raise AssertionError("SAM 2.1 must not stand in for SAM 3")
        monkeypatch.setattr(m, "load_yolo_speech_bubble", lambda *a, **k: pm)
        monkeypatch.setattr(m, "load_rtdetr_conjoined_bubble", boom)
        monkeypatch.setattr(m, "load_sam2", sam2)
        monkeypatch.setattr(detection, "get_model_manager", lambda: m)
        page = s3.sc.make_page(H, W, 5)
        dets, _ = detection.detect_speech_bubbles(Path("p3.png"), image_override=Image.fromarray(page), seg_model="sam3")
        want = shim.hip.segment(page, np.asarray(boxes, np.float32)).cpu().numpy() > 0
        assert len(dets) == 2
        for d, box, w in zip(dets, boxes, want):
            clipped = detection.clip_mask_to_box(w, box, H, W) > 0
            x0, y0, x1, y1 = (int(v) for v in box)
            assert np.array_equal(np.asarray(d["sam_mask"]) > 0, clipped)
            assert not (np.asarray(d["sam_mask"]) > 0)[y0:y1, x0:x1].all()            # the fallback would be the whole rectangle
        m.unload_model(mm.ModelType.SAM3)
        assert not m.is_loaded(mm.ModelType.SAM3) and not any(isinstance(k, tuple) and k[0] is mm.ModelType.SAM3 for k in m.models)
    finally:
        monkeypatch.setattr(mm.ModelManager, "_instance", None)

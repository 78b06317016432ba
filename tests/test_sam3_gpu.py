"""GPU tier: SAM 3 on MI355X through the C ABI vs HF Sam3TrackerModel on CPU fp32, and MTX_EW_QK_ROPE vs its formula."""
import numpy as np
import pytest
import torch

import sam3_checks as s3
from mangatranslator_amd.hip import abi
from parity_log import record

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(abi.BF16, id="bf16"), pytest.param(abi.F16, id="f16")]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qk_rope_exact(hip_lib, dtype, d):
    s3.check_qk_rope_exact(hip_lib, "cuda:0", dtype, d)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qk_rope_random(hip_lib, dtype, d):
    s3.check_qk_rope_random(hip_lib, "cuda:0", dtype, d)


def test_qk_rope_many_rows(hip_lib):
    """more rows than one pass of the row grid covers (4096 row groups of 4) and more columns than one workgroup (24 heads of 128 = 384
    chunks): the grid-stride loop and the second column block"""
    s3.check_qk_rope_random(hip_lib, "cuda:0", abi.BF16, 128, rows=16389, heads=12)


def test_sam3_tiny(hip_lib):
    s3.check_sam3(hip_lib, "cuda:0", "tiny", h=300, w=200, n_boxes=3, seed=0)


def test_sam3_tiny_one_box_landscape(hip_lib):
    s3.check_sam3(hip_lib, "cuda:0", "tiny", h=120, w=260, n_boxes=1, seed=3)


def test_sam3_tiny_high_precision(hip_lib):
    s3.check_sam3(hip_lib, "cuda:0", "tiny", h=300, w=200, n_boxes=3, seed=0, dtype=abi.F16, calibrated=True)
    fast = s3.stats["logit_abs_err_rms"]
    s3.check_sam3(hip_lib, "cuda:0", "tiny", h=300, w=200, n_boxes=3, seed=0, dtype=abi.F16, calibrated=True, precision="high")
    assert s3.stats["logit_abs_err_rms"] < fast, (fast, s3.stats["logit_abs_err_rms"])
    assert s3.stats["decided_pixels_wrong"] == 0 and s3.stats["wrong_beyond_1_logit"] == 0


# measured on the MI355X against the HF fp32 oracle (docs/experiments.md, "SAM 3 on the HIP path"); every bound is twice its measured value
REAL_DIMS = {
    "bf16.fast": (dict(dtype=abi.BF16), dict(logit_tol=0.0669, abs_tol=0.909, rms_tol=0.177, mask_tol=0.00336)),
    "f16.fast": (dict(dtype=abi.F16), dict(logit_tol=0.0103, abs_tol=0.108, rms_tol=0.024, mask_tol=0.000286)),
    "f16.high": (dict(dtype=abi.F16, precision="high"), dict(logit_tol=0.00571, abs_tol=0.0564, rms_tol=0.0112, mask_tol=0.000128)),
}


@pytest.mark.parametrize("mode", list(REAL_DIMS))
def test_sam3_real_dims(hip_lib, mode):
    """The shipped widths (1024 / 16 heads / 4736, window 24, fpn 256, default decoder, four neck levels) at 8 layers on a 672-pixel input — 48 x 48
    grid, 4 windows of 576 tokens, global attention over 2304 tokens on the long-sequence d = 64 path, a tiled 24 x 24 position table — on a 768 x 512
    page with 5 boxes, logits calibrated to a trained model's spread (std 5.0), against HF `Sam3TrackerModel` on CPU fp32; one seeded model and one
    calibration for the three modes.  Hard conditions (inside `check_sam2`): the stability-based mask choice agrees on decisive boxes, and no
    page pixel differs where the fp32 logit lies farther from 0 than the measured max logit error.  Numeric bounds = twice what the MI355X
    measured (seeded-weight runs of SAM-2 varied by about that between seeds and storage types):

      mode        logit rel err (selected / all tokens)   max, logit units   rms      page-mask mismatch   bounds: rel, max, rms, mismatch
      bf16 fast   0.0161 / 0.0335                          0.455              0.0883   1.68e-3              0.0669, 0.909, 0.177, 3.36e-3
      f16 fast    0.0019 / 0.00517                         0.0539             0.0120   1.43e-4              0.0103, 0.108, 0.024, 2.86e-4
      f16 high    0.000997 / 0.00286                       0.0282             0.00559  6.42e-5              0.00571, 0.0564, 0.0112, 1.28e-4

    (the relative bound covers both of `check_sam2`'s relative statements, hence twice the larger).  f16 "high" lands below SAM-2's bar of 1e-4
    mismatching page pixels; 4 of the 5 boxes are compared in every mode (one box's stability score, 0.9804, sits at the 0.98 threshold)."""
    hip_kw, bounds = REAL_DIMS[mode]
    s3.check_sam3(hip_lib, "cuda:0", "real_dims", share_oracle=True, h=768, w=512, n_boxes=5, seed=1, calibrated=True, **bounds, **hip_kw)
    print(mode, s3.stats)
    record(f"sam3.real_dims.768x512.calibrated.{mode}", boxes=5, **s3.stats)
    assert s3.stats["decided_pixels_wrong"] == 0


def test_sam3_repeated_calls_are_bit_identical(hip_lib):
    """the same page and boxes through one model again and again (hipGraph replays after the first call): logits, the stability-based mask
    choice and the masks never change — the hazard `test_sam2_repeated_calls_are_bit_identical` guards, on SAM 3's plans"""
    from mangatranslator_amd.core.ml.sam3 import Sam3Hip
    from mangatranslator_amd.utils.synthetic_pages import make_page
    dev = torch.device("cuda:0")
    model, cfg = s3.make_model("tiny", seed=2)
    sam = Sam3Hip(model.state_dict(), cfg, device=dev, lib=hip_lib)
    pg, _b, _r = make_page(23, 512, 768, bubbles=8, osb_regions=0)
    for nb in (7, 23):
        r = np.random.default_rng(nb)
        bx = np.stack([r.integers(0, 300, nb), r.integers(0, 500, nb)], 1).astype(np.float32)
        bx = np.concatenate([bx, bx + np.stack([25 + (np.arange(nb) % 5) * 30, 32 + (np.arange(nb) % 7) * 20], 1)], 1).astype(np.float32)
        first = None
        for rep in range(8):
            got = [t.cpu() for t in sam.segment(pg, bx, return_logits=True)]
            if first is None:
                first = got
            for a, b, name in zip(first, got, ("masks", "logits", "iou", "choice")):
                assert torch.equal(a, b), (nb, rep, name)

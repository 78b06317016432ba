"""GPU tier: FLUX.1-Kontext with MX-fp8 block linears and the activation + MX-fp8 epilogue of the fp8 GEMM through the C ABI on gfx950."""
import pytest
import torch

import flux_checks as fc
import kontext_fp8_checks as kc
from parity_log import record

pytestmark = pytest.mark.gpu


def test_gemm_f8_actq_epilogue(hip_lib):
    kc.check_actq_cases(hip_lib)


def test_gemm_f8_actq_validation(hip_lib):
    kc.check_actq_validation(hip_lib)


def test_kontext_dit_step_fp8(hip_lib):
    record("flux1.dit_step.tiny.fp8", velocity_rel_err=kc.check_dit_step_fp8(hip_lib, "cuda:0"))


def test_kontext_fp8_fusions_change_nothing(hip_lib):
    kc.check_fusions_change_nothing(hip_lib, "cuda:0", layers=1, single_layers=1)


def test_kontext_fp8_off_means_off(hip_lib):
    kc.check_off_means_off(hip_lib, "cuda:0")


def test_kontext_fp8_first_block_cache(hip_lib):
    kc.check_first_block_cache_fp8(hip_lib, "cuda:0")


def test_kontext_fp8_vs_bf16_psnr(hip_lib):
    record("flux1.kontext.4steps.tiny.fp8_vs_bf16", image_psnr_db=kc.check_kontext_fp8_vs_bf16(hip_lib, "cuda:0"))


def test_full_width_shallow_fp8_vs_bf16(hip_lib):
    """FLUX.1-Kontext's width at 1 + 1 blocks, T = 512 + 2 x 24 x 33 = 2096 (ragged against 256 rows, 48 column tiles in the MLPs, K = 15360
    through the K-slice tail): the fp8 step against the bf16 step of the same weights, both on the device.  0.12 is a cap — the project's fp8
    step bound for a deeper toy network."""
    from mangatranslator_amd.core.ml import flux as fx
    from mangatranslator_amd.hip import abi
    dev, h2, w2, t_txt = "cuda:0", 24, 33, 512
    cfg = dict(fx.KONTEXT_DIT_CFG, layers=1, single_layers=1)
    get = fc.named_provider(fx.dit_param_shapes(cfg), dev, 4)
    lat, pe, pooled = kc.step_inputs(cfg, h2, w2, t_txt)
    dit16 = fx.FluxDiTHip(get, cfg, dev, lib=hip_lib)
    vel16, plan16 = kc.run_step(dit16, lat, pe, pooled, h2, w2, dev)
    del plan16, dit16
    dit8 = fx.FluxDiTHip(get, cfg, dev, lib=hip_lib, fp8=True)          # stays in scope: a plan refers to its model's weights by address
    vel8, plan = kc.run_step(dit8, lat, pe, pooled, h2, w2, dev)
    assert plan.T == 2096 and torch.isfinite(vel8).all()
    blk = kc.block_gemms(plan)
    assert len(blk) == 11 and all(g.in_dtype == abi.F8 for _, g in blk), "a block linear was left on the 16-bit kernel"
    assert sum(1 for _, g in blk if g.actq_q) == 3 and not any(o.kind == abi.OP_QUANT for o in plan.ops)
    e = fc.rel(vel8, vel16)
    print(f"full-width shallow Kontext step (1 + 1 blocks, d = 3072, T = {plan.T}): fp8 vs bf16 velocity rel err {e:.4f}")
    record("flux1.full_width_shallow.T2096.fp8_vs_bf16", velocity_rel_err=e)
    assert e < 0.12
    fc.assert_repeats(plan, dev)

"""GPU tier of manga-ocr's batched decode step: MTX_OP_ROWLIN_WIDE, MTX_OP_DECODE_ATTN_BATCH, MTX_OP_BEAM_STEP and `MangaOcrHip.generate_many` on
the product library (checks in manga_ocr_batch_checks.py).  The damaged-state check runs on the simulator tier only."""
import pytest

import manga_ocr_batch_checks as bc
from mangatranslator_amd.hip import abi

pytestmark = pytest.mark.gpu

DTYPES = [abi.BF16, abi.F16, abi.F32]


def test_new_ops_are_additive_to_abi_12(hip_lib):
    bc.check_abi(hip_lib)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", bc.WIDE_ROWS)
def test_wide_row_linear_equals_the_single_op_row_by_row(hip_lib, dtype, rows):
    for n, k in bc.WIDE_NK:
        bc.check_wide_rows(hip_lib, dtype, rows, n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_row_linear_exact(hip_lib, dtype):
    bc.check_wide_exact(hip_lib, dtype)


def test_wide_row_linear_refuses_bad_arguments(hip_lib):
    bc.check_wide_refusals(hip_lib)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("S,B", bc.ATTN_CASES)
def test_batched_decode_attention_equals_the_single_op(hip_lib, dtype, heads, S, B):
    bc.check_attn_batch(hip_lib, dtype, S, B, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 2])
def test_groups_that_sit_out_of_attention(hip_lib, dtype, heads):
    bc.check_attn_batch_sitting_out(hip_lib, dtype, heads)


def test_batched_decode_attention_refuses_bad_arguments(hip_lib):
    bc.check_attn_batch_refusals(hip_lib)


@pytest.mark.parametrize("V,B,variant", bc.BEAM_CASES)
def test_beam_step_equals_the_host_search(hip_lib, V, B, variant):
    worst = max(bc.check_beam_against_host(hip_lib, V, B, variant, seed) for seed in bc.SEEDS[(V, B, variant)])
    print(f"V={V} B={B} {variant}: largest score difference from the host search {worst:.2e}")


def test_beam_step_ties_follow_the_stated_rule(hip_lib):
    bc.check_beam_ties(hip_lib)


def test_beam_step_is_independent_of_slot_and_group_count(hip_lib):
    bc.check_beam_independence(hip_lib)


def test_beam_step_bad_rows(hip_lib):
    bc.check_beam_bad_rows(hip_lib)


def test_beam_step_refuses_bad_arguments(hip_lib):
    bc.check_beam_refusals(hip_lib)


# ---- the model, tiny configuration -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F16, abi.F32])
@pytest.mark.parametrize("S", [2, 8])
def test_batched_step_logits_equal_the_single_step(hip_lib, dtype, S):
    print(f"reordered steps: {bc.check_lockstep_logits(hip_lib, dtype, S)}")


@pytest.mark.parametrize("dtype", [abi.F16, abi.F32])
def test_generate_many_equals_generate(hip_lib, dtype):
    print(f"generated lengths {bc.check_generate_many(hip_lib, dtype)}")


def test_generate_many_refused_items(hip_lib):
    bc.check_refused_items(hip_lib)


def test_driver_reads_a_page_together(hip_lib, tmp_path, monkeypatch):
    bc.check_driver(hip_lib, tmp_path, monkeypatch)


# ---- published widths ----------------------------------------------------------------------------------------------------------------------------
def test_published_widths_logits_equal_the_single_step(hip_lib):
    print(f"reordered steps: {bc.check_lockstep_logits(hip_lib, abi.F16, 8, steps=12, real=True)}")


def test_published_widths_generate_many_equals_generate(hip_lib):
    print(f"generated lengths {bc.check_published_generate_many(hip_lib)}")


# ---- the wide linear against float64 with the contract's rounding points, for every (RT, NW) it is built for ------------------------------------
CONTRACT_K = (lambda n: 520)
CONTRACT_TYPES = [(abi.BF16, False), (abi.F16, False), (abi.F16, True), (abi.F32, True)]


@pytest.mark.parametrize("dtype,out_f32", CONTRACT_TYPES)
@pytest.mark.parametrize("n,nw", [(257, 1), (2050, 2), (4100, 4)])
@pytest.mark.parametrize("rows,rt", [(7, 8), (9, 16), (17, 32)])
def test_wide_row_linear_contract_exact(hip_lib, dtype, out_f32, n, nw, rows, rt):
    """rowlin_wide_kernel<T, RT, NW> held to float64, not to rowlin_kernel"""
    import manga_ocr_checks as mc
    share = mc.check_rowlin_contract_exact(hip_lib, dtype, rows, n, CONTRACT_K(n), True, out_f32, (rt, nw))
    print(f"wide row linear contract {rows}x{n} dtype {dtype}: rounding share {share}")

"""CPU tier of manga-ocr's batched decode step: MTX_OP_ROWLIN_WIDE, MTX_OP_DECODE_ATTN_BATCH, MTX_OP_BEAM_STEP and `MangaOcrHip.generate_many` on
the simulator (checks in manga_ocr_batch_checks.py)."""
import pytest

import manga_ocr_batch_checks as bc
from mangatranslator_amd.hip import abi

DTYPES = [abi.BF16, abi.F16, abi.F32]


def test_new_ops_are_additive_to_abi_12(emu_lib):
    bc.check_abi(emu_lib)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", bc.WIDE_ROWS)
def test_wide_row_linear_equals_the_single_op_row_by_row(emu_lib, dtype, rows):
    for n, k in bc.WIDE_NK:
        bc.check_wide_rows(emu_lib, dtype, rows, n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_row_linear_exact(emu_lib, dtype):
    bc.check_wide_exact(emu_lib, dtype)


def test_wide_row_linear_refuses_bad_arguments(emu_lib):
    bc.check_wide_refusals(emu_lib)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("S,B", bc.ATTN_CASES)
def test_batched_decode_attention_equals_the_single_op(emu_lib, dtype, heads, S, B):
    bc.check_attn_batch(emu_lib, dtype, S, B, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 2])
def test_groups_that_sit_out_of_attention(emu_lib, dtype, heads):
    bc.check_attn_batch_sitting_out(emu_lib, dtype, heads)


def test_batched_decode_attention_refuses_bad_arguments(emu_lib):
    bc.check_attn_batch_refusals(emu_lib)


@pytest.mark.parametrize("V,B,variant", bc.BEAM_CASES)
def test_beam_step_equals_the_host_search(emu_lib, V, B, variant):
    worst = max(bc.check_beam_against_host(emu_lib, V, B, variant, seed) for seed in bc.SEEDS[(V, B, variant)])
    print(f"V={V} B={B} {variant}: largest score difference from the host search {worst:.2e}")


def test_beam_step_ties_follow_the_stated_rule(emu_lib):
    bc.check_beam_ties(emu_lib)


def test_beam_step_is_independent_of_slot_and_group_count(emu_lib):
    bc.check_beam_independence(emu_lib)


def test_beam_step_bad_rows(emu_lib):
    bc.check_beam_bad_rows(emu_lib)


def test_beam_step_damaged_state(emu_lib):
    bc.check_beam_damaged_state(emu_lib)


def test_beam_step_refuses_bad_arguments(emu_lib):
    bc.check_beam_refusals(emu_lib)


# ---- the model on the simulator (tiny configuration) ------------------------------------------------------------------------------------------
def test_the_crops_end_at_different_lengths_for_the_oracle():
    print(f"oracle lengths {bc.check_oracle_lengths()}")


@pytest.mark.parametrize("dtype", [abi.F16, abi.F32])
@pytest.mark.parametrize("S", [2, 8])
def test_batched_step_logits_equal_the_single_step(emu_lib, dtype, S):
    print(f"reordered steps: {bc.check_lockstep_logits(emu_lib, dtype, S)}")


@pytest.mark.parametrize("dtype", [abi.F16, abi.F32])
def test_generate_many_equals_generate(emu_lib, dtype):
    print(f"generated lengths {bc.check_generate_many(emu_lib, dtype)}")


def test_generate_many_refused_items(emu_lib):
    bc.check_refused_items(emu_lib)


def test_driver_reads_a_page_together(emu_lib, tmp_path, monkeypatch):
    bc.check_driver(emu_lib, tmp_path, monkeypatch)


# ---- the wide linear against float64 with the contract's rounding points, for every (RT, NW) it is built for ------------------------------------
CONTRACT_K = (lambda n: 136 if n == 4100 else 520)          # the simulator tier shortens K at the widest N
CONTRACT_TYPES = [(abi.BF16, False), (abi.F16, False), (abi.F16, True), (abi.F32, True)]


@pytest.mark.parametrize("dtype,out_f32", CONTRACT_TYPES)
@pytest.mark.parametrize("n,nw", [(257, 1), (2050, 2), (4100, 4)])
@pytest.mark.parametrize("rows,rt", [(7, 8), (9, 16), (17, 32)])
def test_wide_row_linear_contract_exact(emu_lib, dtype, out_f32, n, nw, rows, rt):
    """rowlin_wide_kernel<T, RT, NW> held to float64, not to rowlin_kernel"""
    import manga_ocr_checks as mc
    share = mc.check_rowlin_contract_exact(emu_lib, dtype, rows, n, CONTRACT_K(n), True, out_f32, (rt, nw))
    print(f"wide row linear contract {rows}x{n} dtype {dtype}: rounding share {share}")

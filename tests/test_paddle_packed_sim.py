"""CPU tier of PaddleOCR-VL's packed fill: MTX_OP_SEG_ATTN, MTX_OP_CAUSAL_PREFILL_SLOTS and `PaddleOcrVlHip(..., packed_prefill=True)` on the
simulator (checks in packed_prefill_checks.py)."""
import pytest

import packed_prefill_checks as pp
from mangatranslator_amd.hip import abi
from test_paddle_ocr_vl_sim import SIM_TF as TF                # the one-crop path's measured (max, rms), sigma 0.1: the bound is twice these, unchanged

DTYPES = [abi.BF16, abi.F16]
# measured max of the PACKED path's teacher-forced error at the greedy test's sigma (0.06) on the simulator, seeds 0-7 (seed 5 gave it; the
# per-seed figures 0.003848 0.004823 0.004604 0.005481 0.003852 0.006298 0.005249 0.005979 are the one-crop path's: at the tiny widths every
# linear of both paths runs on the 128-tile family, whose rows do not depend on M).  delta = 4 x this leaves 107 of 160 steps decided
PACKED_TF_GREEDY_F16 = 0.006298
PACKED_TF_GREEDY_SEED = 5


def test_packed_ops_are_additive_to_abi_12(emu_lib):
    assert abi.ABI_VERSION == 12 and emu_lib.mtx_abi_version() == 12
    assert (abi.OP_SEG_ATTN, abi.OP_CAUSAL_PREFILL_SLOTS) == (27, 28)
    assert emu_lib.mtx_abi_sizeof(27) > 0 and emu_lib.mtx_abi_sizeof(28) > 0


# ---- MTX_OP_SEG_ATTN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", pp.SEG_WIDTHS)
@pytest.mark.parametrize("lengths", [pp.SEG_LENGTHS, pp.SEG_LENGTHS_EMPTY], ids=["tile_edges", "empty_segments"])
def test_segment_attention_equals_the_single_op(emu_lib, dtype, d, lengths):
    pp.check_segment_attention(emu_lib, dtype, d, lengths)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", pp.SEG_WIDTHS)
def test_segments_do_not_see_each_other(emu_lib, dtype, d):
    pp.check_segment_isolation(emu_lib, dtype, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_attention_damaged_tables(emu_lib, dtype):
    pp.check_segment_damaged_tables(emu_lib, dtype)


def test_segment_attention_refuses_bad_arguments(emu_lib):
    pp.check_segment_refusals(emu_lib)


# ---- MTX_OP_CAUSAL_PREFILL_SLOTS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_equals_the_single_op(emu_lib, dtype, heads, kv):
    pp.check_prefill_slots(emu_lib, dtype, heads, kv, pp.PREFILL_LENGTHS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_empty_slots(emu_lib, dtype, heads, kv):
    pp.check_prefill_slots(emu_lib, dtype, heads, kv, pp.PREFILL_LENGTHS_EMPTY, cache_bits=pp.BYTE_PATTERN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_one_row_prompts(emu_lib, dtype, heads, kv):
    pp.check_prefill_slots(emu_lib, dtype, heads, kv, pp.PREFILL_LENGTHS_ONE, tile_only=(1, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_prefill_too_long_or_damaged_writes_nothing(emu_lib, dtype):
    pp.check_prefill_nothing_written(emu_lib, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_prefill_padded_strides(emu_lib, dtype):
    pp.check_prefill_slots(emu_lib, dtype, 24, 2, [40, 0, 70, 3, 0, 0, 0, 2], pad_qkv=24, pad_o=8, pad_cache=3)


def test_packed_prefill_refuses_bad_arguments(emu_lib):
    pp.check_prefill_refusals(emu_lib)


# ---- the model, tiny configuration -------------------------------------------------------------------------------------------------------------
SEEDS = range(8)


def test_fill_does_not_depend_on_companions_slot_or_rung(emu_lib):
    alone, together = pp.check_independence_tiny(emu_lib)
    assert alone != together, "the two fills were meant to land on different rungs"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_packed_fill_teacher_forced_log_probs(emu_lib, dtype, seed):
    """the one-crop path's bounds, unchanged (SIM_TF): measured packed figures in docs/experiments.md ("PaddleOCR-VL: packed fill")"""
    mx, rms = pp.packed_teacher_forced(emu_lib, dtype, seed)
    print(f"packed fill, teacher-forced seed {seed} dtype {dtype}: max {mx:.6f} rms {rms:.6f}")
    assert mx <= 2 * TF[dtype][0] and rms <= 2 * TF[dtype][1]


def test_packed_greedy_sigma_teacher_forced_error(emu_lib):
    """the figure delta is made of, held to twice its measured value like the one-crop path's (on the seed that gave the maximum)"""
    mx, _ = pp.packed_teacher_forced(emu_lib, abi.F16, PACKED_TF_GREEDY_SEED, sigma=pp.pc.GREEDY_SIGMA)
    print(f"packed fill, teacher-forced at the greedy sigma, seed {PACKED_TF_GREEDY_SEED}: max {mx:.6f}")
    assert mx <= 2 * PACKED_TF_GREEDY_F16


@pytest.mark.parametrize("seed", SEEDS)
def test_packed_greedy_tokens_on_decided_prefixes(emu_lib, seed):
    delta = 4 * PACKED_TF_GREEDY_F16
    decided = [pp.pc.decided_prefix(s, delta)[1] for s in SEEDS]
    assert sum(decided) >= 80, f"only {sum(decided)} of 160 steps are decided at delta = {delta}"
    assert pp.check_greedy_tokens_packed(emu_lib, seed, delta) == decided[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_packed_equals_unpacked_on_decided_prefixes(emu_lib, seed):
    beyond = pp.check_decided_prefix_packed_equals_unpacked(emu_lib, seed, 4 * PACKED_TF_GREEDY_F16)
    print(f"seed {seed}: packed and unpacked {'differ' if beyond else 'agree'} beyond the decided prefix")


def test_packed_against_unpacked_generate_many(emu_lib):
    pp.check_packed_against_unpacked(emu_lib)


def test_packed_refused_items(emu_lib):
    pp.check_refused_items_packed(emu_lib)


def test_packed_driver_reads_a_page_together(emu_lib, tmp_path, monkeypatch):
    pp.check_driver_packed(emu_lib, tmp_path, monkeypatch)


def test_packed_fill_leaves_live_slots_alone(emu_lib):
    pp.check_fill_leaves_live_slots_alone(emu_lib)

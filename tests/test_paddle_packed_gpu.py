"""GPU tier of PaddleOCR-VL's packed fill: MTX_OP_SEG_ATTN, MTX_OP_CAUSAL_PREFILL_SLOTS and `PaddleOcrVlHip(..., packed_prefill=True)` on the
product library (checks in packed_prefill_checks.py)."""
import pytest

import packed_prefill_checks as pp
from mangatranslator_amd.hip import abi
from test_paddle_ocr_vl_gpu import GPU_REAL, GPU_TF as TF      # the one-crop path's measured (max, rms): the bounds are twice these, unchanged

pytestmark = pytest.mark.gpu

DTYPES = [abi.BF16, abi.F16]
# measured max of the PACKED path's teacher-forced error at the greedy test's sigma (0.06) on the MI355X, seeds 0-7: 0.003944 0.005185 0.004574
# 0.004676 0.004232 0.006054 0.005869 0.006420 (`packed_prefill_checks.packed_teacher_forced(lib, F16, seed, sigma=GREEDY_SIGMA)`; seed 7 gave it).
# delta = 4 x this leaves 107 of 160 steps decided ([20, 3, 1, 5, 20, 18, 20, 20])
PACKED_TF_GREEDY_F16 = 0.006420
PACKED_TF_GREEDY_SEED = 7


def test_packed_ops_are_additive_to_abi_12(hip_lib):
    assert abi.ABI_VERSION == 12 and hip_lib.mtx_abi_version() == 12
    assert (abi.OP_SEG_ATTN, abi.OP_CAUSAL_PREFILL_SLOTS) == (27, 28)
    assert hip_lib.mtx_abi_sizeof(27) > 0 and hip_lib.mtx_abi_sizeof(28) > 0


# ---- MTX_OP_SEG_ATTN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", pp.SEG_WIDTHS)
@pytest.mark.parametrize("lengths", [pp.SEG_LENGTHS, pp.SEG_LENGTHS_EMPTY], ids=["tile_edges", "empty_segments"])
def test_segment_attention_equals_the_single_op(hip_lib, dtype, d, lengths):
    pp.check_segment_attention(hip_lib, dtype, d, lengths)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", pp.SEG_WIDTHS)
def test_segments_do_not_see_each_other(hip_lib, dtype, d):
    pp.check_segment_isolation(hip_lib, dtype, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_attention_damaged_tables(hip_lib, dtype):
    pp.check_segment_damaged_tables(hip_lib, dtype)


def test_segment_attention_refuses_bad_arguments(hip_lib):
    pp.check_segment_refusals(hip_lib)


# ---- MTX_OP_CAUSAL_PREFILL_SLOTS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_equals_the_single_op(hip_lib, dtype, heads, kv):
    pp.check_prefill_slots(hip_lib, dtype, heads, kv, pp.PREFILL_LENGTHS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_empty_slots(hip_lib, dtype, heads, kv):
    pp.check_prefill_slots(hip_lib, dtype, heads, kv, pp.PREFILL_LENGTHS_EMPTY, cache_bits=pp.BYTE_PATTERN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pp.PREFILL_HEADS)
def test_packed_prefill_one_row_prompts(hip_lib, dtype, heads, kv):
    pp.check_prefill_slots(hip_lib, dtype, heads, kv, pp.PREFILL_LENGTHS_ONE, tile_only=(1, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_prefill_too_long_or_damaged_writes_nothing(hip_lib, dtype):
    pp.check_prefill_nothing_written(hip_lib, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_prefill_padded_strides(hip_lib, dtype):
    pp.check_prefill_slots(hip_lib, dtype, 24, 2, [40, 0, 70, 3, 0, 0, 0, 2], pad_qkv=24, pad_o=8, pad_cache=3)


def test_packed_prefill_refuses_bad_arguments(hip_lib):
    pp.check_prefill_refusals(hip_lib)


# ---- the model, tiny configuration -------------------------------------------------------------------------------------------------------------
SEEDS = range(8)


def test_fill_does_not_depend_on_companions_slot_or_rung(hip_lib):
    alone, together = pp.check_independence_tiny(hip_lib)
    assert alone != together, "the two fills were meant to land on different rungs"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_packed_fill_teacher_forced_log_probs(hip_lib, dtype, seed):
    """the one-crop path's bounds, unchanged (GPU_TF): measured packed figures in docs/experiments.md ("PaddleOCR-VL: packed fill")"""
    mx, rms = pp.packed_teacher_forced(hip_lib, dtype, seed)
    print(f"packed fill, teacher-forced seed {seed} dtype {dtype}: max {mx:.6f} rms {rms:.6f}")
    assert mx <= 2 * TF[dtype][0] and rms <= 2 * TF[dtype][1]


def test_packed_greedy_sigma_teacher_forced_error(hip_lib):
    """the figure delta is made of, held to twice its measured value like the one-crop path's (on the seed that gave the maximum)"""
    mx, _ = pp.packed_teacher_forced(hip_lib, abi.F16, PACKED_TF_GREEDY_SEED, sigma=pp.pc.GREEDY_SIGMA)
    print(f"packed fill, teacher-forced at the greedy sigma, seed {PACKED_TF_GREEDY_SEED}: max {mx:.6f}")
    assert mx <= 2 * PACKED_TF_GREEDY_F16


@pytest.mark.parametrize("seed", SEEDS)
def test_packed_greedy_tokens_on_decided_prefixes(hip_lib, seed):
    delta = 4 * PACKED_TF_GREEDY_F16
    decided = [pp.pc.decided_prefix(s, delta)[1] for s in SEEDS]
    assert sum(decided) >= 80, f"only {sum(decided)} of 160 steps are decided at delta = {delta}"
    assert pp.check_greedy_tokens_packed(hip_lib, seed, delta) == decided[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_packed_equals_unpacked_on_decided_prefixes(hip_lib, seed):
    beyond = pp.check_decided_prefix_packed_equals_unpacked(hip_lib, seed, 4 * PACKED_TF_GREEDY_F16)
    print(f"seed {seed}: packed and unpacked {'differ' if beyond else 'agree'} beyond the decided prefix")


def test_packed_against_unpacked_generate_many(hip_lib):
    pp.check_packed_against_unpacked(hip_lib)


def test_packed_refused_items(hip_lib):
    pp.check_refused_items_packed(hip_lib)


def test_packed_driver_reads_a_page_together(hip_lib, tmp_path, monkeypatch):
    pp.check_driver_packed(hip_lib, tmp_path, monkeypatch)


def test_packed_fill_leaves_live_slots_alone(hip_lib):
    pp.check_fill_leaves_live_slots_alone(hip_lib)


# ---- the model, published widths (vocabulary 8 192, f16) ---------------------------------------------------------------------------------------
def test_fill_is_independent_across_rungs_at_published_widths(hip_lib):
    pp.check_independence_published(hip_lib)


def test_packed_fill_at_published_widths(hip_lib):
    mx, rms = pp.packed_published_widths(hip_lib)
    print(f"packed fill, published widths: max {mx:.6f} rms {rms:.6f}")
    assert mx <= 2 * GPU_REAL[abi.F16][0] and rms <= 2 * GPU_REAL[abi.F16][1]

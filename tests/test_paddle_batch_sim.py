"""CPU tier of the slot-batched PaddleOCR-VL decode step: MTX_OP_CAUSAL_STEP_BATCH, MTX_OP_GREEDY_BATCH and `generate_many` on the simulator
(checks in paddle_batch_checks.py)."""
import pytest

import paddle_batch_checks as bc
import paddle_ocr_vl_checks as pc
from mangatranslator_amd.hip import abi

DTYPES = [abi.BF16, abi.F16]


def test_new_ops_are_additive_to_abi_12(emu_lib):
    assert abi.ABI_VERSION == 12 and emu_lib.mtx_abi_version() == 12
    assert (abi.OP_CAUSAL_STEP_BATCH, abi.OP_GREEDY_BATCH) == (22, 23)
    assert emu_lib.mtx_abi_sizeof(22) > 0 and emu_lib.mtx_abi_sizeof(23) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", bc.HEADS)
@pytest.mark.parametrize("slots", [1, 2, 3, 8])
def test_batched_step_equals_the_single_step(emu_lib, dtype, heads, kv, slots):
    bc.check_batch_equals_single(emu_lib, dtype, heads, kv, slots)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", bc.HEADS)
def test_slots_that_sit_out(emu_lib, dtype, heads, kv):
    bc.check_sitting_out(emu_lib, dtype, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", bc.HEADS)
def test_batched_step_selects_exactly_per_slot(emu_lib, dtype, heads, kv):
    bc.check_batch_selection(emu_lib, dtype, heads, kv)


@pytest.mark.parametrize("vocab", bc.BATCH_VOCABS)
@pytest.mark.parametrize("slots", [1, 3, 8])
def test_greedy_batch_equals_the_single_pick(emu_lib, vocab, slots):
    for shift in (range(len(bc.ROLES)) if slots == 1 else (0, 3)):
        bc.check_greedy_batch(emu_lib, vocab, slots, shift)


def test_greedy_batch_damaged_state(emu_lib):
    bc.check_greedy_batch_damaged_state(emu_lib)


def test_greedy_batch_run_of_steps(emu_lib):
    bc.check_greedy_batch_run(emu_lib)


def test_batched_ops_refuse_bad_arguments(emu_lib):
    bc.check_batch_refusals(emu_lib)


# ---- the model on the simulator (tiny configuration, f16, GREEDY_SIGMA weights of one seed) ----------------------------------------------------
@pytest.mark.parametrize("check_every", [1, 8])
def test_generate_many_equals_generate(emu_lib, check_every):
    lens = bc.check_generate_many_equals_generate(emu_lib, check_every)
    print(f"generated lengths {lens}")


def test_generate_many_other_slot_counts(emu_lib):
    bc.check_other_slot_counts(emu_lib)


def test_generate_many_refused_items(emu_lib):
    bc.check_refused_items(emu_lib)


def test_driver_reads_a_page_together(emu_lib, tmp_path, monkeypatch):
    bc.check_driver(emu_lib, tmp_path, monkeypatch)


# ---- head layouts that HEADS does not reach: G = 4, and nz > 1 where slot = blockIdx.z / nz differs from blockIdx.z ------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS)
def test_step_layouts_batched_equals_single(emu_lib, dtype, heads, kv):
    """causal_step_batch_kernel<T, G> at (G, nz) = step_layout(heads, kv), three slots; the counter check covers the ticket words kvh * nz + z"""
    pc.assert_layout(heads, kv)
    _, nz = pc.step_layout(heads, kv)
    assert kv * nz <= heads, "every ticket word lies among the words `counters()` reads"
    bc.check_batch_equals_single(emu_lib, dtype, heads, kv, 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS)
def test_step_layouts_slots_that_sit_out(emu_lib, dtype, heads, kv):
    pc.assert_layout(heads, kv)
    bc.check_sitting_out(emu_lib, dtype, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS)
def test_step_layouts_batched_selection(emu_lib, dtype, heads, kv):
    pc.assert_layout(heads, kv)
    bc.check_batch_selection(emu_lib, dtype, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS + [(16, 2)])
def test_batched_step_selects_exactly_per_head(emu_lib, dtype, heads, kv):
    pc.assert_layout(heads, kv)
    bc.check_batch_selection_per_head(emu_lib, dtype, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_step_padded_strides(emu_lib, dtype):
    bc.check_batch_padded_strides(emu_lib, dtype)


def test_greedy_batch_65_chunks(emu_lib):
    bc.check_greedy_batch_65_chunks(emu_lib)

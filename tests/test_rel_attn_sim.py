"""CPU tier of MTX_OP_REL_ATTN (csrc/relattn.hip): attention with a Toeplitz bias and a device-side key count on the simulator
(checks in rel_attn_checks.py)."""
import pytest

import rel_attn_checks as ra
from mangatranslator_amd.hip import abi

# (s, heads, kv) of the random comparison: every tile edge once, the largest size with the widest group
RANDOM = [(1, 2, 2), (33, 4, 2), (65, 8, 2), (131, 4, 2), (512, 8, 2)]


def test_rel_attention_is_additive_to_abi_12(emu_lib):
    assert abi.ABI_VERSION == 12 and emu_lib.mtx_abi_version() == 12
    assert abi.OP_REL_ATTN == 29 and emu_lib.mtx_abi_sizeof(29) > 0


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
@pytest.mark.parametrize("heads,kv", ra.HEADS)
def test_the_bias_alone_selects(emu_lib, dtype, d, heads, kv):
    assert sum(ra.check_bias_selects(emu_lib, dtype, s, heads, kv, d) for s in ra.SIZES) > 0


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
@pytest.mark.parametrize("heads,kv", ra.HEADS)
def test_the_bias_is_added_after_the_scale(emu_lib, dtype, d, heads, kv):
    for s in ra.SIZES[1:]:
        ra.check_bias_after_scale(emu_lib, dtype, s, heads, kv, d)


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
@pytest.mark.parametrize("heads,kv", ra.HEADS)
def test_the_key_limit(emu_lib, dtype, d, heads, kv):
    for s in ra.SIZES:
        ra.check_key_limit(emu_lib, dtype, s, heads, kv, d)


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
def test_masked_entries_weigh_nothing(emu_lib, dtype, d):
    for s in ra.SIZES:
        ra.check_masked_entries(emu_lib, dtype, s, 4, 2, d)


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
@pytest.mark.parametrize("s,heads,kv", RANDOM)
def test_random_tables_against_fp32(emu_lib, dtype, d, s, heads, kv):
    ra.check_random(emu_lib, dtype, s, heads, kv, d)
    ra.check_random(emu_lib, dtype, s, heads, kv, d, n_keys=max(1, s - 7), seed=1)


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("d", ra.WIDTHS)
def test_no_table_no_limit(emu_lib, dtype, d):
    ra.check_no_table(emu_lib, dtype, 77, 4, 2, d)


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("s,heads,kv", [(2, 2, 2), (77, 4, 2), (131, 8, 2), (512, 4, 2)])
def test_the_causal_table_equals_causal_attention(emu_lib, dtype, s, heads, kv):
    ra.check_equals_causal_op(emu_lib, dtype, s, heads, kv)


def test_refusals(emu_lib):
    ra.check_refusals(emu_lib)

"""CPU tier of FLUX's prompt encoders on the HIP path (core/ml/text_encoders.py) and of their wiring, on the simulator
(checks in text_encoder_checks.py)."""
import pytest

import text_encoder_checks as tc


@pytest.mark.parametrize("seed", tc.SEEDS)
def test_qwen3_within_four_floors_of_the_wheel(emu_lib, seed):
    tc.check_qwen3(emu_lib, seed)


def test_qwen3_rows_and_their_padding(emu_lib):
    tc.check_qwen3_padding(emu_lib)


@pytest.mark.parametrize("S", tc.T5_S)
@pytest.mark.parametrize("seed", tc.SEEDS)
def test_t5_within_four_floors_of_the_wheel(emu_lib, seed, S):
    tc.check_t5(emu_lib, seed, S)


def test_t5_relative_table_is_the_wheels():
    tc.check_t5_table()


def test_t5_refuses_f16(emu_lib):
    tc.check_t5_refuses_f16(emu_lib)


@pytest.mark.parametrize("eos", [2, 511])
@pytest.mark.parametrize("seed", tc.SEEDS)
def test_clip_within_four_floors_of_the_wheel(emu_lib, seed, eos):
    tc.check_clip(emu_lib, seed, eos)


def test_clip_pools_the_first_end_of_text_row(emu_lib):
    tc.check_clip(emu_lib, 0, 300)


def test_klein_prompt_wiring(emu_lib, tmp_path, monkeypatch):
    tc.check_klein_wiring(emu_lib, tmp_path, monkeypatch)


def test_kontext_prompt_wiring(emu_lib, tmp_path):
    tc.check_kontext_wiring(emu_lib, tmp_path)

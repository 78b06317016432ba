"""GPU tier of FLUX's prompt encoders on the HIP path (core/ml/text_encoders.py) and of their wiring, on the product library
(checks in text_encoder_checks.py)."""
import pytest

import text_encoder_checks as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", tc.SEEDS)
def test_qwen3_within_four_floors_of_the_wheel(hip_lib, seed):
    tc.check_qwen3(hip_lib, seed)


def test_qwen3_rows_and_their_padding(hip_lib):
    tc.check_qwen3_padding(hip_lib)


@pytest.mark.parametrize("S", tc.T5_S)
@pytest.mark.parametrize("seed", tc.SEEDS)
def test_t5_within_four_floors_of_the_wheel(hip_lib, seed, S):
    tc.check_t5(hip_lib, seed, S)


def test_t5_relative_table_is_the_wheels():
    tc.check_t5_table()


def test_t5_refuses_f16(hip_lib):
    tc.check_t5_refuses_f16(hip_lib)


@pytest.mark.parametrize("eos", [2, 511])
@pytest.mark.parametrize("seed", tc.SEEDS)
def test_clip_within_four_floors_of_the_wheel(hip_lib, seed, eos):
    tc.check_clip(hip_lib, seed, eos)


def test_clip_pools_the_first_end_of_text_row(hip_lib):
    tc.check_clip(hip_lib, 0, 300)


def test_klein_prompt_wiring(hip_lib, tmp_path, monkeypatch):
    tc.check_klein_wiring(hip_lib, tmp_path, monkeypatch)


def test_kontext_prompt_wiring(hip_lib, tmp_path):
    tc.check_kontext_wiring(hip_lib, tmp_path)


def test_published_widths_qwen3(hip_lib):
    tc.check_published_qwen3(hip_lib)


def test_published_widths_t5(hip_lib):
    tc.check_published_t5(hip_lib)


def test_published_widths_clip(hip_lib):
    tc.check_published_clip(hip_lib)
